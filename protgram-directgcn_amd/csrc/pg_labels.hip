// k-hop letter reach: the trainer's closest_aa task labels (protgram_directgcn_trainer.py:239-269,
// _generate_closest_amino_acid_labels) without its per-node BFS. Every node carries a bitmask of the letters its
// n-gram contains (bit b = letter b); one hop is R_h[v] = R_{h-1}[v] | OR over the out-neighbours u of R_{h-1}[u],
// and the first h at which a letter's bit appears in R_h[v] is the length of the shortest out-path from v to a node
// that contains the letter -- what the reference's FIFO BFS with a visited set finds. OR is idempotent
// and commutative: the result is the same whatever the order of the reduction. Word work, bound by the random 4-byte
// gathers of reach_in[col[e]]: wave64, no LDS, no atomics.
#include "pg_common.h"

namespace {

constexpr int kGroup = 16;                         // lanes per row: n-gram rows have at most K ~ 20-25 successors
constexpr int kBlock = 256;                        // 4 waves
constexpr int kRowsPerBlock = kBlock / kGroup;     // 4 rows per wave, 16 per block

__global__ __launch_bounds__(256) void letter_masks_kernel(int64_t N, const int64_t* node_keys, int n, int64_t K,
                                                           const int32_t* code_bit, uint32_t* masks) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    int64_t key = node_keys[i];
    uint32_t m = 0;
    for (int j = 0; j < n && key >= 0; ++j) {  // a negative key is no window (pg_ngram_keys' -1): no letters
        const int32_t b = code_bit[key % K];
        key /= K;
        if ((uint32_t)b < 32u) m |= 1u << b;
    }
    masks[i] = m;
}

// One group of kGroup lanes per row: the lanes stride over the row's entries (longer rows loop), the group ORs by
// xor-shuffles (every lane ends with the row's word), lane 0 stores it, and lane l writes the distance bytes of the
// new bits l and l + 16. A row without entries copies reach_in[v]. No lane leaves before the shuffles: a group past
// the last row runs them on zeros. col entries must lie in [0, n_rows): the gather is not guarded (the caller checks).
__global__ __launch_bounds__(kBlock) void reach_hop_kernel(int64_t n_rows, const int64_t* rowptr, const int64_t* col,
                                                           const uint32_t* reach_in, uint32_t* reach_out, uint8_t hop,
                                                           int n_bits, uint8_t* dist, int64_t ldd,
                                                           const uint8_t* target, int64_t* labels) {
    const int lane = threadIdx.x & (kGroup - 1);
    const int64_t v = (int64_t)blockIdx.x * kRowsPerBlock + threadIdx.x / kGroup;
    const bool live = v < n_rows;
    uint32_t acc = 0, own = 0;
    if (live) {
        own = reach_in[v];
        const int64_t end = rowptr[v + 1];
        // two entries per lane and pass, both gathers in flight together: a row of up to 32 entries is one pass
        // without a branch. A missing second entry reads the row's own word instead, which the result holds anyway.
        for (int64_t e = rowptr[v] + lane; e < end; e += 2 * kGroup) {
            const int64_t c0 = col[e];
            const int64_t c1 = e + kGroup < end ? col[e + kGroup] : v;
            acc |= reach_in[c0] | reach_in[c1];
        }
    }
#pragma unroll
    for (int s = kGroup / 2; s > 0; s >>= 1) acc |= (uint32_t)__shfl_xor((int)acc, s, kGroup);
    if (!live) return;
    const uint32_t out = own | acc;
    const uint32_t fresh = out & ~own;
    if (lane == 0) {
        reach_out[v] = out;
        if (target) {
            const uint32_t t = target[v];
            if (t < 32u && ((fresh >> t) & 1u)) labels[v] = hop;
        }
    }
    if (dist && fresh) {
        uint8_t* row = dist + v * ldd;
        if (lane < n_bits && ((fresh >> lane) & 1u)) row[lane] = hop;
        if (lane + kGroup < n_bits && ((fresh >> (lane + kGroup)) & 1u)) row[lane + kGroup] = hop;
    }
}

}  // namespace

extern "C" int pg_ngram_letter_masks(int64_t n_nodes, const int64_t* node_keys, int n, int64_t K,
                                     const int32_t* code_bit, uint32_t* masks, void* stream) {
    PG_REQUIRE(n_nodes >= 0 && n >= 1 && K >= 1, "pg_ngram_letter_masks: bad arguments n_nodes=%lld n=%d K=%lld",
               (long long)n_nodes, n, (long long)K);
    // K^n must fit a signed 64-bit key (pg_ngram_keys' rule)
    double bits = 0;
    for (int j = 0; j < n; ++j) bits += __builtin_log2((double)K);
    PG_REQUIRE(bits < 62.5, "pg_ngram_letter_masks: K^n = %lld^%d does not fit a 64-bit key", (long long)K, n);
    if (n_nodes == 0) return PG_OK;
    PG_REQUIRE(node_keys && code_bit && masks, "pg_ngram_letter_masks: null pointer");
    const int64_t nb = (n_nodes + 255) / 256;
    PG_REQUIRE(nb < (1ll << 31), "pg_ngram_letter_masks: n_nodes = %lld is too large", (long long)n_nodes);
    hipLaunchKernelGGL(letter_masks_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, n_nodes, node_keys, n,
                       K, code_bit, masks);
    return pg::check_launch("pg_ngram_letter_masks");
}

extern "C" int pg_reach_hop_u32(int64_t n_rows, const int64_t* rowptr, const int64_t* col, const uint32_t* reach_in,
                                uint32_t* reach_out, int hop, int n_bits, uint8_t* dist, int64_t ldd,
                                const uint8_t* target, int64_t* labels, void* stream) {
    PG_REQUIRE(n_rows >= 0 && n_rows < (1ll << 31), "pg_reach_hop_u32: n_rows = %lld outside [0, 2^31)",
               (long long)n_rows);
    PG_REQUIRE(hop >= 1 && hop <= 255, "pg_reach_hop_u32: hop = %d outside [1, 255]", hop);
    PG_REQUIRE(n_bits >= 1 && n_bits <= 32, "pg_reach_hop_u32: n_bits = %d outside [1, 32]", n_bits);
    PG_REQUIRE(!dist || ldd >= n_bits, "pg_reach_hop_u32: ldd = %lld < n_bits = %d", (long long)ldd, n_bits);
    PG_REQUIRE(!target == !labels, "pg_reach_hop_u32: target and labels go together");
    if (n_rows == 0) return PG_OK;
    PG_REQUIRE(rowptr && col && reach_in && reach_out, "pg_reach_hop_u32: null pointer");
    {   // in place a launch could carry a bit two hops: the two buffers ping-pong
        const uintptr_t a = reinterpret_cast<uintptr_t>(reach_in), b = reinterpret_cast<uintptr_t>(reach_out);
        const uintptr_t bytes = (uintptr_t)n_rows * sizeof(uint32_t);
        PG_REQUIRE(a + bytes <= b || b + bytes <= a, "pg_reach_hop_u32: reach_in and reach_out overlap");
    }
    const int64_t nb = (n_rows + kRowsPerBlock - 1) / kRowsPerBlock;
    hipLaunchKernelGGL(reach_hop_kernel, dim3((unsigned)nb), dim3(kBlock), 0, (hipStream_t)stream, n_rows, rowptr, col,
                       reach_in, reach_out, (uint8_t)hop, n_bits, dist, ldd, target, labels);
    return pg::check_launch("pg_reach_hop_u32");
}
