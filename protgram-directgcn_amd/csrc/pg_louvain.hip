// One synchronous local-moving sweep of Louvain (Blondel et al.) over a symmetric integer CSR: the community task
// labels of the trainer (protgram_directgcn_trainer.py:200-220) and its fallback partitioner (:159-170) without the
// pure-Python loop over a networkx graph. Every decision is taken from the state at the start of the
// sweep (comm_in, tot, size are only read), so the result does not depend on how the rows are scheduled.
//
// For an active row i (class_hash(i) % classes == cls) and every community c among its neighbours j != i:
//   w_ic    = sum of W_ij over the neighbours j in c                       (integer adds in LDS)
//   gain(c) = two_m * w_ic - (tot[c] - [c == comm_i] * k_i) * k_i          (exact: 128-bit products)
// The row moves to the candidate of largest gain (ties: smallest id) when that gain strictly beats gain(comm_i), its
// gain of staying (w_i,own = 0 when no neighbour shares its community). A row alone in its community does not take a
// single-member community of larger id as a candidate: two such rows would otherwise swap for ever. Inactive rows
// copy comm_in.
//
// Three row paths, chosen by the row's entry count alone, all in the one launch and with no waiting between
// workgroups: up to kWaveCap entries one wave per row with a 128-slot hash table in LDS; up to kBlockCap entries the
// whole workgroup per row with a 2048-slot table; longer rows the whole workgroup with passes over community-id
// ranges of kRangeWidth ids and a directly indexed table (slow, exact for any row). A table is at most half full
// (distinct communities <= entries <= slots / 2) and every probe loop is bounded by the slot count. Integer LDS
// atomics only (compare-and-swap on the key, 64-bit add on the weight): sums do not depend on arrival order.
#include "pg_common.h"

namespace {

typedef __int128 i128;
typedef unsigned long long u64;

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kRowsPerWave = 4;
constexpr int kRowsPerBlock = kWaves * kRowsPerWave;
constexpr int kWaveSlots = 128, kWaveCap = kWaveSlots / 2;
constexpr int kBlockSlots = 2048, kBlockCap = kBlockSlots / 2;
constexpr int kRangeWidth = 2 * kBlockSlots;  // the key and the weight array together, as one array of sums
constexpr u64 kEmpty = ~0ull;                 // no community id: ids are non-negative

__device__ __forceinline__ uint32_t class_hash(int64_t i) {
    return (uint32_t)(((u64)i * 0x9E3779B97F4A7C15ull) >> 32);
}

struct Cand {
    i128 gain;
    int64_t c;  // < 0: none
};

__device__ __forceinline__ bool better(const Cand& a, const Cand& b) {  // b beats a
    return b.c >= 0 && (a.c < 0 || b.gain > a.gain || (b.gain == a.gain && b.c < a.c));
}

__device__ __forceinline__ i128 join(long long hi, long long lo) {
    return (i128)(((unsigned __int128)(u64)hi << 64) | (unsigned __int128)(u64)lo);
}

__device__ __forceinline__ Cand wave_best(Cand a) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        Cand b;
        b.gain = join(__shfl_xor((long long)(a.gain >> 64), s), __shfl_xor((long long)(u64)a.gain, s));
        b.c = __shfl_xor((long long)a.c, s);
        if (better(a, b)) a = b;
    }
    return a;
}

// what a row knows about itself and the sweep
struct RowCtx {
    int64_t ci, ki, two_m;
    bool alone;
    const int64_t* tot;
    const int64_t* size;
};

__device__ __forceinline__ i128 gain_of(const RowCtx& r, u64 w, int64_t c) {
    return (i128)r.two_m * (i128)w - (i128)(r.tot[c] - (c == r.ci ? r.ki : 0)) * (i128)r.ki;
}

// one (community, summed weight) of the row's table: the row's own community reports its weight, any other one is
// weighed against the best so far
__device__ __forceinline__ void consider(const RowCtx& r, int64_t c, u64 w, Cand& best, u64& own_w) {
    if (c == r.ci) {
        own_w = w;
        return;
    }
    if (r.alone && c > r.ci && r.size[c] == 1) return;
    const Cand b{gain_of(r, w, c), c};
    if (better(best, b)) best = b;
}

__device__ __forceinline__ bool decide(const RowCtx& r, const Cand& best, u64 own_w, int64_t* out) {
    const bool move = best.c >= 0 && best.gain > gain_of(r, own_w, r.ci);
    *out = move ? best.c : r.ci;
    return move;
}

template <int kSlots>
__device__ __forceinline__ void table_add(u64* keys, u64* vals, int64_t c, int64_t w) {
    constexpr int kShift = 32 - __builtin_ctz(kSlots);
    uint32_t s = ((uint32_t)(c ^ (c >> 32)) * 0x9E3779B1u) >> kShift;
    for (int p = 0; p < kSlots; ++p) {  // at most half the slots are taken: an empty one is always found
        const u64 old = atomicCAS(&keys[s], kEmpty, (u64)c);
        if (old == kEmpty || old == (u64)c) {
            atomicAdd(&vals[s], (u64)w);
            return;
        }
        s = (s + 1) & (kSlots - 1);
    }
}

__global__ __launch_bounds__(kBlock) void louvain_move_kernel(int64_t n_rows, const int64_t* rowptr, const int64_t* col,
                                                              const int64_t* w, const int64_t* k,
                                                              const int64_t* comm_in, const int64_t* tot,
                                                              const int64_t* size, int64_t two_m, int classes, int cls,
                                                              int64_t* comm_out, u64* moved) {
    __shared__ u64 s_key[kBlockSlots];
    __shared__ u64 s_val[kBlockSlots];  // the range passes use both arrays as sums: ids [0, 2048) and [2048, 4096)
    __shared__ int64_t s_long[kRowsPerBlock];
    __shared__ long long s_red[kWaves][3];
    __shared__ int64_t s_lim[kWaves][2];
    __shared__ u64 s_own;
    __shared__ unsigned s_moved;

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) s_moved = 0;

    // ---- rows of up to kWaveCap entries: one wave per row --------------------------------------------------------
    u64* wkey = s_key + wv * kWaveSlots;
    u64* wval = s_val + wv * kWaveSlots;
    for (int r = 0; r < kRowsPerWave; ++r) {
        const int64_t row = (int64_t)blockIdx.x * kRowsPerBlock + r * kWaves + wv;
        const bool valid = row < n_rows;
        const bool active = valid && (int)(class_hash(row) % (uint32_t)classes) == cls;
        int64_t beg = 0, deg = 0;
        if (active) {
            beg = rowptr[row];
            deg = rowptr[row + 1] - beg;
        }
        const bool shortrow = active && deg <= kWaveCap;
        if (lane == 0) {
            if (valid && !active) comm_out[row] = comm_in[row];
            s_long[r * kWaves + wv] = (active && !shortrow) ? row : -1;
        }
        wkey[lane] = kEmpty;
        wkey[lane + 64] = kEmpty;
        wval[lane] = 0;
        wval[lane + 64] = 0;
        __syncthreads();
        if (shortrow && lane < deg) {
            const int64_t j = col[beg + lane];
            if (j != row) table_add<kWaveSlots>(wkey, wval, comm_in[j], w[beg + lane]);
        }
        __syncthreads();
        if (shortrow) {
            RowCtx rc;
            rc.ci = comm_in[row];
            rc.ki = k[row];
            rc.two_m = two_m;
            rc.tot = tot;
            rc.size = size;
            rc.alone = size[rc.ci] == 1;
            Cand best{0, -1};
            u64 own_w = 0;
            for (int s = lane; s < kWaveSlots; s += 64)
                if (wkey[s] != kEmpty) consider(rc, (int64_t)wkey[s], wval[s], best, own_w);
            best = wave_best(best);
#pragma unroll
            for (int s = 32; s > 0; s >>= 1) {  // one lane at most holds the own community's weight
                const u64 o = (u64)__shfl_xor((long long)own_w, s);
                own_w = o > own_w ? o : own_w;
            }
            if (lane == 0 && decide(rc, best, own_w, &comm_out[row])) atomicAdd(&s_moved, 1u);
        }
        __syncthreads();  // the table is cleared again next round
    }

    // ---- longer rows: the whole workgroup per row ------------------------------------------------------------------
    for (int q = 0; q < kRowsPerBlock; ++q) {
        const int64_t row = s_long[q];  // the same for every thread: the loop and its barriers are uniform
        if (row < 0) continue;
        const int64_t beg = rowptr[row], end = rowptr[row + 1];
        RowCtx rc;
        rc.ci = comm_in[row];
        rc.ki = k[row];
        rc.two_m = two_m;
        rc.tot = tot;
        rc.size = size;
        rc.alone = size[rc.ci] == 1;
        Cand best{0, -1};
        u64 own_w = 0;
        if (tid == 0) s_own = 0;
        if (end - beg <= kBlockCap) {
            for (int s = tid; s < kBlockSlots; s += kBlock) {
                s_key[s] = kEmpty;
                s_val[s] = 0;
            }
            __syncthreads();
            for (int64_t e = beg + tid; e < end; e += kBlock) {
                const int64_t j = col[e];
                if (j != row) table_add<kBlockSlots>(s_key, s_val, comm_in[j], w[e]);
            }
            __syncthreads();
            for (int s = tid; s < kBlockSlots; s += kBlock)
                if (s_key[s] != kEmpty) consider(rc, (int64_t)s_key[s], s_val[s], best, own_w);
        } else {
            // the span of the neighbours' community ids, then one pass per kRangeWidth ids of it
            int64_t lo = INT64_MAX, hi = -1;
            for (int64_t e = beg + tid; e < end; e += kBlock) {
                const int64_t j = col[e];
                if (j == row) continue;
                const int64_t c = comm_in[j];
                lo = c < lo ? c : lo;
                hi = c > hi ? c : hi;
            }
#pragma unroll
            for (int s = 32; s > 0; s >>= 1) {
                const int64_t l2 = __shfl_xor((long long)lo, s), h2 = __shfl_xor((long long)hi, s);
                lo = l2 < lo ? l2 : lo;
                hi = h2 > hi ? h2 : hi;
            }
            if (lane == 0) {
                s_lim[wv][0] = lo;
                s_lim[wv][1] = hi;
            }
            __syncthreads();
            for (int v = 0; v < kWaves; ++v) {
                lo = s_lim[v][0] < lo ? s_lim[v][0] : lo;
                hi = s_lim[v][1] > hi ? s_lim[v][1] : hi;
            }
            for (int64_t base = lo; base <= hi; base += kRangeWidth) {  // hi = -1: no neighbour but the row itself
                for (int s = tid; s < kBlockSlots; s += kBlock) {
                    s_key[s] = 0;
                    s_val[s] = 0;
                }
                __syncthreads();
                for (int64_t e = beg + tid; e < end; e += kBlock) {
                    const int64_t j = col[e];
                    if (j == row) continue;
                    const int64_t d = comm_in[j] - base;
                    if (d >= 0 && d < kRangeWidth)
                        atomicAdd(d < kBlockSlots ? &s_key[d] : &s_val[d - kBlockSlots], (u64)w[e]);
                }
                __syncthreads();
                for (int s = tid; s < kRangeWidth; s += kBlock) {  // weights are positive: a sum of 0 is no neighbour
                    const u64 ws = s < kBlockSlots ? s_key[s] : s_val[s - kBlockSlots];
                    if (ws) consider(rc, base + s, ws, best, own_w);
                }
                __syncthreads();
            }
        }
        best = wave_best(best);
        if (own_w) s_own = own_w;  // one thread at most
        if (lane == 0) {
            s_red[wv][0] = (long long)(best.gain >> 64);
            s_red[wv][1] = (long long)(u64)best.gain;
            s_red[wv][2] = best.c;
        }
        __syncthreads();
        if (tid == 0) {
            for (int v = 1; v < kWaves; ++v) {
                Cand b;
                b.gain = join(s_red[v][0], s_red[v][1]);
                b.c = s_red[v][2];
                if (better(best, b)) best = b;
            }
            if (decide(rc, best, s_own, &comm_out[row])) atomicAdd(&s_moved, 1u);
        }
        __syncthreads();
    }
    __syncthreads();
    if (tid == 0 && s_moved) atomicAdd(moved, (u64)s_moved);
}

}  // namespace

extern "C" int64_t pg_louvain_row_capacity(void) { return kBlockCap; }

extern "C" int pg_louvain_move_i64(int64_t n_rows, const int64_t* rowptr, const int64_t* col, const int64_t* w,
                                   const int64_t* k, const int64_t* comm_in, const int64_t* tot, const int64_t* size,
                                   int64_t two_m, int classes, int cls, int64_t* comm_out, int64_t* moved,
                                   void* stream) {
    PG_REQUIRE(n_rows >= 0 && n_rows < (1ll << 31), "pg_louvain_move_i64: n_rows = %lld outside [0, 2^31)",
               (long long)n_rows);
    PG_REQUIRE(classes >= 1 && cls >= 0 && cls < classes, "pg_louvain_move_i64: class %d of %d", cls, classes);
    PG_REQUIRE(two_m >= 0 && two_m < (1ll << 62), "pg_louvain_move_i64: two_m = %lld outside [0, 2^62)",
               (long long)two_m);
    if (n_rows == 0) return PG_OK;
    PG_REQUIRE(rowptr && col && w && k && comm_in && tot && size && comm_out && moved,
               "pg_louvain_move_i64: null pointer");
    {   // in place a row would read a neighbour's new community: every decision is taken from the sweep's start
        const uintptr_t a = reinterpret_cast<uintptr_t>(comm_in), b = reinterpret_cast<uintptr_t>(comm_out);
        const uintptr_t bytes = (uintptr_t)n_rows * sizeof(int64_t);
        PG_REQUIRE(a + bytes <= b || b + bytes <= a, "pg_louvain_move_i64: comm_in and comm_out overlap");
    }
    const int64_t nb = (n_rows + kRowsPerBlock - 1) / kRowsPerBlock;
    hipLaunchKernelGGL(louvain_move_kernel, dim3((unsigned)nb), dim3(kBlock), 0, (hipStream_t)stream, n_rows, rowptr,
                       col, w, k, comm_in, tot, size, two_m, classes, cls, comm_out, (u64*)moved);
    return pg::check_launch("pg_louvain_move_i64");
}
