// Protein-level pooling of node embeddings (the trainer's "Step 3", protgram_directgcn_trainer.py:387-398):
// row r of out is the fp32 mean of the rows E[ids[e]], e in [rowptr[r], rowptr[r + 1]), ids[e] in [0, N).
//   distinct = 0: EmbeddingProcessor.pool_ngram_embeddings_for_protein (models_utils.py:197-207): every entry with
//     its multiplicity, summed in list order (np.mean over axis 0 adds row after row);
//   distinct = 1: pool_ngram_embeddings_for_protein_fast (:209-262): every id once, summed in ascending id order
//     (the inverted index is walked by n-gram id, and `sums[prot_indices] += emb` adds once per protein).
// Each feature column is ONE sequential fp32 chain from +0.0 (that is the contract: the results match the reference
// bit for bit), so a list is never split across waves. Gather-bound: what hides the latency is rows in flight.
//   * Lists up to kLong entries: a group of G lanes (G * 16 B >= the row, 8 <= G <= 64) owns a list, fetches G ids
//     with one coalesced load and issues up to 16 row loads before the adds that consume them; the other groups of
//     the wave own other lists (gather_add).
//   * Longer lists (the tail of a skewed protein set): a whole wave owns the list. Its 64 / G lane groups load
//     DIFFERENT rows (64 / G rows per load instruction, up to 16 loads per lane in flight), then every group adds
//     all of them in list order, reading the other groups' pieces across lanes: each group carries the same chain
//     (wave_gather_add). The first blocks of the windows launch look for the long lists, so one launch runs both.
// The distinct mode removes duplicates in LDS: a presence bitmap over the N nodes, set with ds_or from the list,
// then walked in word order; the walk emits the ascending ids in chunks of 64 to gather_add<64> and clears the words
// it read. One wave and one bitmap per workgroup. (wave_gather_add measured slower there, 7.8 ms against 4.4 ms for
// 100,000 lists at F = 64: the lists are short and the cross-lane reads cost more than the latency they hide.)
// The sum never becomes -0.0 (it starts at +0.0 and x + (-x) = +0.0), so adding +0.0 for a skipped entry is the
// identity and the gather loops need no branch per entry.
#include <type_traits>

#include "pg_common.h"

namespace {

constexpr int64_t kDistinctMaxNodes = 262144;  // 32 KiB of bitmap per list (pg_pool_distinct_max_nodes)
constexpr int kStage = 128;                    // ids staged between the bitmap walk and the gather (fill < 96)
constexpr int64_t kLong = 1024;                // windows mode: longer lists get a whole wave
constexpr int kLongBlocks = 64;                // blocks of the windows launch that take the long lists

template <bool VEC>
using piece_t = std::conditional_t<VEC, float4, float>;

__device__ __forceinline__ void zero(float4& a) { a = make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ void zero(float& a) { a = 0.f; }
__device__ __forceinline__ void add(float4& a, const float4& x) {
    a.x += x.x;
    a.y += x.y;
    a.z += x.z;
    a.w += x.w;
}
__device__ __forceinline__ void add(float& a, float x) { a += x; }
__device__ __forceinline__ float4 from_lane(const float4& x, int src) {
    return make_float4(__shfl(x.x, src), __shfl(x.y, src), __shfl(x.z, src), __shfl(x.w, src));
}
__device__ __forceinline__ float from_lane(float x, int src) { return __shfl(x, src); }
// fp32 / int32 as NumPy computes it (float64 quotient rounded to float32): for 24-bit operands the double rounding is
// innocuous (53 >= 2 * 24 + 2), i.e. this is the correctly rounded fp32 quotient
__device__ __forceinline__ float mean1(float s, int c) { return (float)((double)s / (double)c); }
__device__ __forceinline__ void store_mean(float* p, const float4& a, int c) {
    *reinterpret_cast<float4*>(p) = c > 0 ? make_float4(mean1(a.x, c), mean1(a.y, c), mean1(a.z, c), mean1(a.w, c))
                                          : make_float4(0.f, 0.f, 0.f, 0.f);
}
__device__ __forceinline__ void store_mean(float* p, float a, int c) { *p = c > 0 ? mean1(a, c) : 0.f; }

// acc += E[id_j] for the chunk's entries j = 0 .. cnt-1 in that order; lane j of the group holds id_j (-1: skip).
// Row loads go out B at a time ahead of their adds; a skipped entry loads row 0 and adds +0.0.
template <int G, bool VEC>
__device__ __forceinline__ void gather_add(const float* __restrict__ E, int64_t lde, int64_t col, bool lane_on,
                                           int32_t myid, int cnt, piece_t<VEC>& acc) {
    constexpr int B = G < 16 ? G : 16;
    for (int j0 = 0; j0 < cnt; j0 += B) {
        int32_t v[B];
        piece_t<VEC> x[B];
#pragma unroll
        for (int u = 0; u < B; ++u) v[u] = __shfl(myid, j0 + u, G);
        if (lane_on) {
#pragma unroll
            for (int u = 0; u < B; ++u)
                x[u] = *reinterpret_cast<const piece_t<VEC>*>(E + (int64_t)(v[u] < 0 ? 0 : v[u]) * lde + col);
#pragma unroll
            for (int u = 0; u < B; ++u) {
                if (v[u] < 0) zero(x[u]);
                add(acc, x[u]);
            }
        }
    }
}

// The same for a chunk of up to 64 entries owned by the whole wave (all 64 lanes active; lane j holds id_j): lane
// group s loads the rows j = u * R + s, then every group adds rows 0, 1, 2, ... in order, so all R groups end with
// the same acc.
template <int G, bool VEC>
__device__ __forceinline__ void wave_gather_add(const float* __restrict__ E, int64_t lde, int64_t col, bool lane_on,
                                                int32_t myid, int cnt, piece_t<VEC>& acc) {
    constexpr int R = 64 / G;            // rows per load instruction
    constexpr int L = G < 16 ? G : 16;   // loads per lane and pass
    constexpr int RP = R * L;            // rows per pass; divides 64
    const int lane = threadIdx.x & 63, s = lane / G, gl = lane & (G - 1);
    for (int j0 = 0; j0 < cnt; j0 += RP) {
        int32_t v[L];
        piece_t<VEC> x[L];
#pragma unroll
        for (int u = 0; u < L; ++u) {
            v[u] = __shfl(myid, j0 + u * R + s);
            zero(x[u]);
        }
        if (lane_on) {
#pragma unroll
            for (int u = 0; u < L; ++u)
                if (j0 + u * R < cnt)  // wave-uniform: no loads for rows past the chunk
                    x[u] = *reinterpret_cast<const piece_t<VEC>*>(E + (int64_t)(v[u] < 0 ? 0 : v[u]) * lde + col);
#pragma unroll
            for (int u = 0; u < L; ++u)
                if (v[u] < 0) zero(x[u]);
        }
#pragma unroll
        for (int u = 0; u < L; ++u) {
            if (j0 + u * R < cnt) {  // wave-uniform
                if constexpr (R == 1) {
                    add(acc, x[u]);
                } else {
#pragma unroll
                    for (int s2 = 0; s2 < R; ++s2) add(acc, from_lane(x[u], s2 * G + gl));
                }
            }
        }
    }
}

// distinct = 0. Blocks [0, kLongBlocks): a wave per list longer than kLong (wave w looks at lists w, w + waves, ...
// of the launch order). The other blocks: G lanes per list of at most kLong entries.
template <int G, bool VEC>
__global__ __launch_bounds__(256) void pool_windows_kernel(const float* __restrict__ E, int64_t lde, int64_t N,
                                                           int64_t pieces, const int64_t* __restrict__ rowptr,
                                                           const int32_t* __restrict__ ids,
                                                           const int64_t* __restrict__ order, int64_t P,
                                                           float* __restrict__ out, int64_t ldo,
                                                           int32_t* __restrict__ counts) {
    constexpr int W = VEC ? 4 : 1;
    const int lane = threadIdx.x & 63, gl = lane & (G - 1), gbase = lane & ~(G - 1);
    if (blockIdx.x < kLongBlocks) {
        const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = kLongBlocks * 4;
        for (int64_t i0 = 0; wave + nwaves * i0 < P; i0 += 64) {
            const int64_t t = wave + nwaves * (i0 + lane);
            int64_t r = -1;
            if (t < P) {
                r = order ? order[t] : t;
                if (r < 0 || r >= P || rowptr[r + 1] - rowptr[r] <= kLong) r = -1;
            }
            uint64_t m = __ballot(r >= 0);
            while (m) {  // wave-uniform
                const int j = __builtin_ctzll(m);
                m &= m - 1;
                const int64_t rj = __shfl(r, j);
                const int64_t beg = rowptr[rj], end = rowptr[rj + 1];
                for (int64_t c0 = 0; c0 < pieces; c0 += G) {
                    const bool lane_on = N > 0 && c0 + gl < pieces;
                    const int64_t col = (c0 + gl) * W;
                    piece_t<VEC> acc;
                    zero(acc);
                    int cnt = 0;
                    for (int64_t e0 = beg; e0 < end; e0 += 64) {
                        int32_t id = -1;
                        if (e0 + lane < end) {
                            id = ids[e0 + lane];
                            if (id < 0 || id >= N) id = -1;
                        }
                        cnt += __popcll(__ballot(id >= 0));
                        const int64_t left = end - e0;
                        wave_gather_add<G, VEC>(E, lde, col, lane_on, id, left < 64 ? (int)left : 64, acc);
                    }
                    if (lane < G && c0 + gl < pieces) store_mean(out + rj * ldo + col, acc, cnt);
                    if (c0 == 0 && lane == 0) counts[rj] = cnt;
                }
            }
        }
        return;
    }
    const int64_t ngroups = ((int64_t)gridDim.x - kLongBlocks) * (256 / G);
    for (int64_t t = (((int64_t)blockIdx.x - kLongBlocks) * 256 + threadIdx.x) / G; t < P; t += ngroups) {
        const int64_t r = order ? order[t] : t;
        if (r < 0 || r >= P) continue;
        const int64_t beg = rowptr[r], end = rowptr[r + 1];
        if (end - beg > kLong) continue;
        for (int64_t c0 = 0; c0 < pieces; c0 += G) {
            const bool lane_on = N > 0 && c0 + gl < pieces;
            const int64_t col = (c0 + gl) * W;
            piece_t<VEC> acc;
            zero(acc);
            int cnt = 0;
            for (int64_t e0 = beg; e0 < end; e0 += G) {
                int32_t id = -1;
                if (e0 + gl < end) {
                    id = ids[e0 + gl];
                    if (id < 0 || id >= N) id = -1;
                }
                uint64_t m = __ballot(id >= 0) >> gbase;
                if (G < 64) m &= (1ull << (G & 63)) - 1;
                cnt += __popcll(m);
                const int64_t left = end - e0;
                gather_add<G, VEC>(E, lde, col, lane_on, id, left < G ? (int)left : G, acc);
            }
            if (c0 + gl < pieces) store_mean(out + r * ldo + col, acc, cnt);
            if (c0 == 0 && gl == 0) counts[r] = cnt;
        }
    }
}

// distinct = 1. One wave per workgroup and per list; lds = bitmap [words] | stage [kStage].
template <bool VEC>
__global__ __launch_bounds__(64) void pool_distinct_kernel(const float* __restrict__ E, int64_t lde, int64_t N,
                                                           int64_t pieces, const int64_t* __restrict__ rowptr,
                                                           const int32_t* __restrict__ ids,
                                                           const int64_t* __restrict__ order, int64_t P,
                                                           float* __restrict__ out, int64_t ldo,
                                                           int32_t* __restrict__ counts, int words) {
    extern __shared__ uint32_t lds[];
    constexpr int W = VEC ? 4 : 1;
    uint32_t* bm = lds;
    int32_t* stage = reinterpret_cast<int32_t*>(lds + words);
    const int lane = threadIdx.x;
    for (int w = lane; w < words; w += 64) bm[w] = 0;
    __syncthreads();
    for (int64_t t = blockIdx.x; t < P; t += gridDim.x) {
        const int64_t r = order ? order[t] : t;
        if (r < 0 || r >= P) continue;
        const int64_t beg = rowptr[r], end = rowptr[r + 1];
        for (int64_t c0 = 0; c0 < pieces; c0 += 64) {  // more than one pass only for rows above 64 pieces
            for (int64_t e = beg + lane; e < end; e += 64) {
                const int32_t id = ids[e];
                if (id >= 0 && id < N) atomicOr(&bm[id >> 5], 1u << (id & 31));
            }
            __syncthreads();
            const bool lane_on = c0 + lane < pieces;
            const int64_t col = (c0 + lane) * W;
            piece_t<VEC> acc;
            zero(acc);
            int cnt = 0, fill = 0;
            for (int w0 = 0; w0 < words; w0 += 64) {
                uint32_t w = 0;
                if (w0 + lane < words) {
                    w = bm[w0 + lane];
                    if (w) bm[w0 + lane] = 0;  // the bitmap is clean again when the walk ends
                }
                uint64_t m = __ballot(w != 0);
                while (m) {  // wave-uniform: the non-empty words in ascending order
                    const int j = __builtin_ctzll(m);
                    m &= m - 1;
                    const uint32_t wj = __builtin_amdgcn_readlane(w, j);  // j is wave-uniform
                    if (lane < 32 && ((wj >> lane) & 1u))
                        stage[fill + __popc(wj & ((1u << lane) - 1u))] = ((w0 + j) << 5) + lane;
                    fill += __popc(wj);
                    if (fill >= 64) {
                        __syncthreads();
                        const int32_t id = stage[lane];
                        const int32_t rest = lane < fill - 64 ? stage[64 + lane] : -1;
                        gather_add<64, VEC>(E, lde, col, lane_on, id, 64, acc);
                        cnt += 64;
                        __syncthreads();
                        if (lane < fill - 64) stage[lane] = rest;
                        fill -= 64;
                    }
                }
            }
            if (fill > 0) {
                __syncthreads();
                const int32_t id = lane < fill ? stage[lane] : -1;
                gather_add<64, VEC>(E, lde, col, lane_on, id, fill, acc);
                cnt += fill;
            }
            __syncthreads();
            if (lane_on) store_mean(out + r * ldo + col, acc, cnt);
            if (c0 == 0 && lane == 0) counts[r] = cnt;
        }
    }
}

struct PoolArgs {
    const float* E;
    int64_t lde, N, pieces;
    const int64_t* rowptr;
    const int32_t* ids;
    const int64_t* order;
    int64_t P;
    float* out;
    int64_t ldo;
    int32_t* counts;
};

template <int G, bool VEC>
void launch(hipStream_t s, const PoolArgs& a, int distinct) {
    if (distinct) {
        const int words = (int)((a.N + 31) / 32);
        const size_t lds = ((size_t)words + kStage) * 4;
        int64_t per_cu = (160 * 1024) / (int64_t)lds;  // lists in flight per CU: what the bitmaps leave room for
        per_cu = per_cu < 1 ? 1 : (per_cu > 16 ? 16 : per_cu);
        const int64_t cap = 256 * per_cu;
        hipLaunchKernelGGL((pool_distinct_kernel<VEC>), dim3((unsigned)(a.P < cap ? a.P : cap)), dim3(64), lds, s,
                           a.E, a.lde, a.N, a.pieces, a.rowptr, a.ids, a.order, a.P, a.out, a.ldo, a.counts, words);
    } else {
        const int64_t blocks = (a.P + 256 / G - 1) / (256 / G);
        hipLaunchKernelGGL((pool_windows_kernel<G, VEC>), dim3((unsigned)(kLongBlocks + (blocks < 4096 ? blocks : 4096))),
                           dim3(256), 0, s, a.E, a.lde, a.N, a.pieces, a.rowptr, a.ids, a.order, a.P, a.out, a.ldo,
                           a.counts);
    }
}

template <bool VEC>
void launch_g(hipStream_t s, const PoolArgs& a, int distinct) {
    if (a.pieces <= 8)
        launch<8, VEC>(s, a, distinct);
    else if (a.pieces <= 16)
        launch<16, VEC>(s, a, distinct);
    else if (a.pieces <= 32)
        launch<32, VEC>(s, a, distinct);
    else
        launch<64, VEC>(s, a, distinct);
}

}  // namespace

extern "C" {

int64_t pg_pool_distinct_max_nodes(void) { return kDistinctMaxNodes; }

int pg_pool_rows_f32(const float* E, int64_t lde, int64_t N, int64_t F, const int64_t* rowptr, const int32_t* ids,
                     const int64_t* order, int64_t P, int distinct, float* out, int64_t ldo, int32_t* counts,
                     uint32_t flags, void* stream) {
    const char* name = "pg_pool_rows_f32";
    (void)flags;
    PG_REQUIRE(P >= 0 && N >= 0 && F >= 0, "%s: negative size P=%lld N=%lld F=%lld", name, (long long)P, (long long)N,
               (long long)F);
    PG_REQUIRE(N < (1ll << 31), "%s: N = %lld does not fit the int32 ids", name, (long long)N);
    PG_REQUIRE(distinct == 0 || distinct == 1, "%s: distinct must be 0 or 1", name);
    PG_REQUIRE(lde >= F && ldo >= F, "%s: row strides lde=%lld ldo=%lld must be >= F=%lld", name, (long long)lde,
               (long long)ldo, (long long)F);
    if (distinct && N > kDistinctMaxNodes)
        return pg::set_error(PG_ERR_UNSUPPORTED, "%s: distinct = 1 takes N <= %lld nodes (N = %lld)", name,
                             (long long)kDistinctMaxNodes, (long long)N);
    if (P == 0 || F == 0) return PG_OK;
    // N = 0: no id is valid and E is never read (zero rows, zero counts)
    PG_REQUIRE(rowptr && ids && out && counts && (E || N == 0), "%s: null pointer", name);
    const bool vec = F % 4 == 0 && lde % 4 == 0 && ldo % 4 == 0 && pg::aligned16(E) && pg::aligned16(out);
    const PoolArgs a{E, lde, N, vec ? F / 4 : F, rowptr, ids, order, P, out, ldo, counts};
    if (vec)
        launch_g<true>((hipStream_t)stream, a, distinct);
    else
        launch_g<false>((hipStream_t)stream, a, distinct);
    return pg::check_launch(name);
}

}  // extern "C"
