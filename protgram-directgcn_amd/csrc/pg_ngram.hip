// n-gram transition producer: the window / transition extraction of
// src/pipeline/data_builder.py:38-54 (_extract_ngrams_from_sequence_tuple, _extract_edges_from_sequence_tuple)
// as integer keys on the GPU. A window of n characters maps to key = sum_j code(c_j) * K^(n-1-j) with an
// order-preserving code (code = rank of the character among the characters present), so the numeric order of
// keys is the sorted-string order the reference uses for node ids (data_builder.py:171-175). Byte work,
// HBM-bound: one block per sequence, threads stride its positions (neighbouring windows share bytes in L1).
#include "pg_common.h"

namespace {

__global__ __launch_bounds__(256) void ngram_keys_kernel(int64_t nseq, const int64_t* offsets, const uint8_t* bytes,
                                                         const int32_t* lut, int n, int64_t K, int64_t* keys,
                                                         int64_t* next_keys) {
    for (int64_t sq = blockIdx.x; sq < nseq; sq += gridDim.x) {
        const int64_t beg = offsets[sq], end = offsets[sq + 1];
        for (int64_t p = beg + threadIdx.x; p < end; p += blockDim.x) {
            int64_t key = -1, nxt = -1;
            if (p + n <= end) {
                key = 0;
                for (int j = 0; j < n; ++j) key = key * K + lut[bytes[p + j]];
                if (p + n + 1 <= end) {  // the window starting at p+1 lies in the same sequence
                    nxt = 0;
                    for (int j = 1; j <= n; ++j) nxt = nxt * K + lut[bytes[p + j]];
                }
            }
            keys[p] = key;
            next_keys[p] = nxt;
        }
    }
}

// Node id of every window (the pooling step's ngram_map.get(seq[i:i+n]), models_utils.py:202, :238-239): the same
// key as above, looked up in the level's sorted node keys (binary search) or in a dense key -> id table. A window
// that leaves its sequence, holds a character without a code (lut < 0: outside the level's alphabet) or is no node
// gets -1.
__global__ __launch_bounds__(256) void ngram_window_ids_kernel(int64_t nseq, const int64_t* offsets,
                                                               const uint8_t* bytes, const int32_t* lut, int n,
                                                               int64_t K, const int64_t* node_keys, int64_t N,
                                                               const int32_t* table, int32_t* ids) {
    for (int64_t sq = blockIdx.x; sq < nseq; sq += gridDim.x) {
        const int64_t beg = offsets[sq], end = offsets[sq + 1];
        for (int64_t p = beg + threadIdx.x; p < end; p += blockDim.x) {
            int32_t id = -1;
            if (p + n <= end) {
                int64_t key = 0;
                bool coded = true;
                for (int j = 0; j < n; ++j) {
                    const int32_t c = lut[bytes[p + j]];
                    coded = coded && c >= 0 && c < K;
                    key = key * K + c;
                }
                if (coded) {
                    if (table) {
                        id = table[key];  // key < K^n: every code is in [0, K)
                    } else {
                        int64_t lo = 0, hi = N;  // first position with node_keys[pos] >= key
                        while (lo < hi) {
                            const int64_t mid = (lo + hi) >> 1;
                            if (node_keys[mid] < key) lo = mid + 1; else hi = mid;
                        }
                        if (lo < N && node_keys[lo] == key) id = (int32_t)lo;
                    }
                }
            }
            ids[p] = id;
        }
    }
}

}  // namespace

extern "C" int pg_ngram_window_ids(int64_t nseq, const int64_t* offsets, const uint8_t* bytes, const int32_t* lut,
                                   int n, int64_t K, const int64_t* node_keys, int64_t N, const int32_t* table,
                                   int32_t* ids, void* stream) {
    PG_REQUIRE(nseq >= 0 && n >= 1 && K >= 1 && N >= 0, "pg_ngram_window_ids: bad arguments nseq=%lld n=%d K=%lld N=%lld",
               (long long)nseq, n, (long long)K, (long long)N);
    PG_REQUIRE(N < (1ll << 31), "pg_ngram_window_ids: N = %lld does not fit an int32 id", (long long)N);
    if (nseq == 0) return PG_OK;
    PG_REQUIRE(offsets && bytes && lut && ids && (table || node_keys || N == 0), "pg_ngram_window_ids: null pointer");
    double bits = 0;
    for (int j = 0; j < n; ++j) bits += __builtin_log2((double)K);
    PG_REQUIRE(bits < 62.5, "pg_ngram_window_ids: K^n = %lld^%d does not fit a 64-bit key", (long long)K, n);
    const unsigned nb = (unsigned)(nseq < 65536 ? nseq : 65536);
    hipLaunchKernelGGL(ngram_window_ids_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, nseq, offsets, bytes, lut,
                       n, K, node_keys, N, table, ids);
    return pg::check_launch("pg_ngram_window_ids");
}

extern "C" int pg_ngram_keys(int64_t nseq, const int64_t* offsets, const uint8_t* bytes, const int32_t* lut, int n,
                             int64_t K, int64_t* keys, int64_t* next_keys, void* stream) {
    PG_REQUIRE(nseq >= 0 && n >= 1 && K >= 1, "bad arguments nseq=%lld n=%d K=%lld", (long long)nseq, n, (long long)K);
    if (nseq == 0) return PG_OK;
    PG_REQUIRE(offsets && bytes && lut && keys && next_keys, "null pointer");
    // K^n must fit a signed 64-bit key
    double bits = 0;
    for (int j = 0; j < n; ++j) bits += __builtin_log2((double)K);
    PG_REQUIRE(bits < 62.5, "K^n = %lld^%d does not fit a 64-bit key", (long long)K, n);
    const unsigned nb = (unsigned)(nseq < 65536 ? nseq : 65536);
    hipLaunchKernelGGL(ngram_keys_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, nseq, offsets, bytes, lut, n, K,
                       keys, next_keys);
    return pg::check_launch("pg_ngram_keys");
}
