// gfx950 LDS-DMA primitives of the kernels whose operands go global -> LDS without passing through registers
// (pg_dense.hip, pg_ngram_mid.hip, pg_ngram_scatter.hip).
// One LDS-DMA wave-instruction (global_load_lds_dword / _dwordx4) moves 4 or 16 B per lane from a per-lane global
// address to (wave-uniform LDS base in M0) + size * lane. It is counted in vmcnt, in issue order with the wave's other
// vector-memory operations. The compiler cannot tell which LDS bytes a DMA writes: before an LDS read that might touch
// them, and at control-flow joins, it waits vmcnt(0), draining every DMA in flight. Kernels that keep several tiles in
// flight therefore count the pieces themselves (vm_wait, or a literal s_waitcnt vmcnt), publish landed pieces with
// lds_barrier, and hide from the compiler either the reads (inline-asm ds_read, pg_dense.hip) or the DMA (glds16_asm).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace pg {

// The builtin pieces (g: per-lane global address, l: wave-uniform LDS base): 16 B per lane; 16 B with the non-temporal
// cache policy (aux = 2: data read once); 4 B per lane.
__device__ __forceinline__ void glds16(const void* g, void* l) { __builtin_amdgcn_global_load_lds(g, l, 16, 0, 0); }
__device__ __forceinline__ void glds16nt(const void* g, void* l) { __builtin_amdgcn_global_load_lds(g, l, 16, 0, 2); }
__device__ __forceinline__ void glds4(const void* g, void* l) { __builtin_amdgcn_global_load_lds(g, l, 4, 0, 0); }

// The 16-B piece in inline asm (-> LDS byte address lds + 16 lane): invisible to the compiler's wait bookkeeping, so
// the caller counts it (vm_wait). M0 is saved and restored inside the statement.
__device__ __forceinline__ void glds16_asm(const void* src, uint32_t lds) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(src), "s"(lds)
                 : "memory");
}

// s_waitcnt vmcnt(min(n, 23)) for a wave-uniform n (a smaller bound than needed only waits longer)
__device__ __forceinline__ void vm_wait(int n) {
    switch (n < 0 ? 0 : n) {
#define PG_VMW(k)                                                  \
    case k: asm volatile("s_waitcnt vmcnt(" #k ")" ::: "memory"); \
        break;
        PG_VMW(0) PG_VMW(1) PG_VMW(2) PG_VMW(3) PG_VMW(4) PG_VMW(5) PG_VMW(6) PG_VMW(7) PG_VMW(8) PG_VMW(9)
        PG_VMW(10) PG_VMW(11) PG_VMW(12) PG_VMW(13) PG_VMW(14) PG_VMW(15) PG_VMW(16) PG_VMW(17) PG_VMW(18)
        PG_VMW(19) PG_VMW(20) PG_VMW(21) PG_VMW(22)
#undef PG_VMW
        default: asm volatile("s_waitcnt vmcnt(23)" ::: "memory"); break;
    }
}

// the 32-bit LDS byte address of a pointer into __shared__ memory
__device__ __forceinline__ uint32_t lds_addr(const void* p) {
    return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void*)p;
}

// Workgroup barrier for LDS hand-offs only: drains this wave's LDS ops, not its global loads (__syncthreads' release
// fence also waits vmcnt(0), which would drain the LDS-DMA in flight).
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// Hide a per-lane value (a lane id, an LDS offset) from the optimiser: what is computed from it is recomputed at its
// use instead of being hoisted into registers held across a loop, and compile-time parts added to it stay immediate
// ds_read / ds_write offsets instead of being folded into one constant per use.
__device__ __forceinline__ int opaque(int v) {
    asm volatile("" : "+v"(v));
    return v;
}

}  // namespace pg
