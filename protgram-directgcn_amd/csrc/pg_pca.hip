// PCA reduction of the pooled protein table (the trainer's "Step 5", protgram_directgcn_trainer.py:411-421,
// EmbeddingProcessor.apply_pca, models_utils.py:88-136): the two streaming passes over X [P, F] fp32. The F x F
// eigenproblem between them is solved on the host (reduce.py).
//
// pg_pca_moments_f64: S = sum (x - s)(x - s)^T, sum (x - s) and n over the valid rows, in float64, on the f64 matrix
// cores (v_mfma_f64_16x16x4_f64), without atomics: the same launch gives the same bits.
//   * The columns are cut into super-tiles of 64; a workgroup owns one row chunk and one pair (I <= J) of super-tiles
//     (one launch for the pairs I = J, one for I < J: they differ in registers and so in rows in flight).
//   * Lane l = (m = l & 15, kk = l >> 4) of a wave loads the 16 bytes X[row + kk][64 I + 4 m .. + 3]: one load
//     instruction covers 4 rows x 64 columns, 256 contiguous bytes per row. Component q of it is the A (or B) operand
//     of the MFMA tile whose 16 columns are 64 I + 4 m' + q, m' = 0..15: the 4 x 4 tiles of a pair are interleaved
//     column sets, so the lane's four values feed them without any exchange. A diagonal pair computes the 10 tiles
//     with qa <= qb; the others follow by symmetry.
//   * f64 C/D layout: lane l, register i holds D[(l >> 4) + 4 i][l & 15] (not the f32 map).
//   * The 4 waves of the workgroup take the chunk's blocks of 32 (I = J) or 16 rows round robin and add their tiles in wave order in
//     LDS; the workgroup writes one 64 x 64 partial per (chunk, pair), the diagonal pairs also their 64 column sums,
//     pair 0 the row count. pca_moments_fold_kernel adds the partials: 16 contiguous runs of chunks per output, each
//     in chunk order, then the 16 sums in order.
// pg_pca_project: out[r, c] = sum_f (x[r, f] - center[f]) W[c, f] on the fp32 matrix cores (v_mfma_f32_16x16x4_f32),
// the subtraction in fp32 before the product, one rounding to fp16 in the epilogue.
//   * W is the A operand (M = components), X the B operand (N = rows): lane (n = l & 15, g = l >> 4) loads the 16 bytes
//     X[row0 + n][f0 + 4 g .. + 3] and uses component q in MFMA step q, whose four k indices are f0 + 4 g' + q.
//   * W is staged once per workgroup in LDS (row stride F + 4 floats), in panels of at most 128 components when it does
//     not fit; tile t's row m is component 32 (t >> 1) + 8 (m >> 2) + 4 (t & 1) + (m & 3), so that a lane ends up with
//     8 consecutive components of one row in the registers of tiles 2u and 2u + 1: one 16-byte store of fp16.
#include "pg_common.h"

namespace {

typedef double d4_t __attribute__((ext_vector_type(4)));
typedef float f4_t __attribute__((ext_vector_type(4)));
typedef _Float16 h8_t __attribute__((ext_vector_type(8)));

constexpr int64_t kMaxF = 512;
constexpr int kSuper = 64;             // columns per super-tile
constexpr int kTile = kSuper * kSuper; // doubles per partial
// rows per block of a wave (MFMA steps of 4 rows; two blocks are in flight): a diagonal pair has 10 tiles of
// accumulators and one operand, which leaves registers for 32 rows at 2 waves per SIMD; the others have 16 tiles
constexpr int kRowsDiag = 32, kRowsOff = 16;
constexpr int kFoldRuns = 16;          // runs of chunks per output in the fold

struct MomentsPlan {
    int64_t chunk_rows, nchunks, npairs, chunk_stride;
    int Fs;
};

// Fixed by (P, F) alone. About 512 workgroups on the diagonal pairs (two per CU, one round) and at least 256 rows per
// chunk (P = 1301: 6 chunks, the last of 21 rows); a chunk's partials are F / rows of its input, a few per cent at the
// sizes that matter.
MomentsPlan moments_plan(int64_t P, int64_t F) {
    MomentsPlan p;
    p.Fs = (int)((F + kSuper - 1) / kSuper);
    p.npairs = (int64_t)p.Fs * (p.Fs + 1) / 2;
    int64_t want = 512 / p.Fs;
    if (want < 64) want = 64;
    int64_t rows = (P + want - 1) / want;
    rows = (rows + 63) / 64 * 64;
    if (rows < 256) rows = 256;
    p.chunk_rows = rows;
    p.nchunks = (P + rows - 1) / rows;
    p.chunk_stride = p.npairs * kTile + (int64_t)p.Fs * kSuper + 1;
    return p;
}

template <int NU>
struct Slab {
    float v[NU][4];
};

// The lane's pieces of rows rb + 4 u + kk, u < NU, at columns col .. col + 3; zeros outside the matrix and for
// rows that are skipped (bit u of `ok` clear).
template <bool VEC, int NU>
__device__ __forceinline__ void load_slab(const float* __restrict__ X, int64_t ldx, int64_t F, int64_t rb, int kk,
                                          int64_t col, unsigned ok, Slab<NU>& s) {
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        const int64_t row = rb + 4 * u + kk;
#pragma unroll
        for (int q = 0; q < 4; ++q) s.v[u][q] = 0.f;
        if ((ok >> u) & 1u) {
            if constexpr (VEC) {
                if (col < F) {
                    const float4 t = *reinterpret_cast<const float4*>(X + row * ldx + col);
                    s.v[u][0] = t.x;
                    s.v[u][1] = t.y;
                    s.v[u][2] = t.z;
                    s.v[u][3] = t.w;
                }
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (col + q < F) s.v[u][q] = X[row * ldx + col + q];
            }
        }
    }
}

template <int NU>
__device__ __forceinline__ unsigned rows_ok(const int32_t* __restrict__ counts, int64_t rb, int kk, int64_t end) {
    unsigned ok = 0;
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        const int64_t row = rb + 4 * u + kk;
        if (row < end && (!counts || counts[row] > 0)) ok |= 1u << u;
    }
    return ok;
}

// DIAG: blockIdx.y is the super-tile I of the pair (I, I); else it counts the pairs I < J.
template <bool VEC, bool DIAG>
__device__ __forceinline__ void moments_body(const float* __restrict__ X, int64_t ldx, int64_t P, int64_t F,
                                             const int32_t* __restrict__ counts, const float* __restrict__ shift,
                                             double* __restrict__ work, int64_t chunk_rows, int Fs, int64_t npairs,
                                             int64_t chunk_stride) {
    __shared__ double red[kTile];
    __shared__ double csum[4][kSuper];
    __shared__ double cnt[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = lane & 15, kk = lane >> 4;
    constexpr bool diag = DIAG;
    constexpr int kRowsPerBlock = DIAG ? kRowsDiag : kRowsOff, NU = kRowsPerBlock / 4;
    int I = (int)blockIdx.y, J = I;
    if constexpr (!DIAG) {
        int rem = (int)blockIdx.y;
        I = 0;
        while (rem >= Fs - 1 - I) {
            rem -= Fs - 1 - I;
            ++I;
        }
        J = I + 1 + rem;
    }
    const int64_t pair = (int64_t)I * Fs - (int64_t)I * (I - 1) / 2 + (J - I);  // position in the order (I, J >= I)
    const int64_t c0 = (int64_t)blockIdx.x * chunk_rows;
    const int64_t c1 = c0 + chunk_rows < P ? c0 + chunk_rows : P;
    const int64_t colA = (int64_t)kSuper * I + 4 * m, colB = (int64_t)kSuper * J + 4 * m;
    double sA[4], sB[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        sA[q] = shift && colA + q < F ? (double)shift[colA + q] : 0.0;
        sB[q] = shift && colB + q < F ? (double)shift[colB + q] : 0.0;
    }
    d4_t acc[4][4];
#pragma unroll
    for (int qa = 0; qa < 4; ++qa)
#pragma unroll
        for (int qb = 0; qb < 4; ++qb) acc[qa][qb] = d4_t{0.0, 0.0, 0.0, 0.0};
    double cs[4] = {0.0, 0.0, 0.0, 0.0};
    double nrows = 0.0;

    int64_t rb = c0 + (int64_t)kRowsPerBlock * wave;
    Slab<NU> a = {}, b = {}, an = {}, bn = {};
    unsigned ok = 0, okn = 0;
    if (rb < c1) {  // wave-uniform
        ok = rows_ok<NU>(counts, rb, kk, c1);
        load_slab<VEC>(X, ldx, F, rb, kk, colA, ok, a);
        if constexpr (!diag) load_slab<VEC>(X, ldx, F, rb, kk, colB, ok, b);
    }
    for (; rb < c1; rb += 4 * kRowsPerBlock) {
        const int64_t nb = rb + 4 * kRowsPerBlock;
        if (nb < c1) {  // the next block's loads go out before this block's MFMAs
            okn = rows_ok<NU>(counts, nb, kk, c1);
            load_slab<VEC>(X, ldx, F, nb, kk, colA, okn, an);
            if constexpr (!diag) load_slab<VEC>(X, ldx, F, nb, kk, colB, okn, bn);
        }
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const bool on = (ok >> u) & 1u;
            double da[4], db[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                da[q] = on ? (double)a.v[u][q] - sA[q] : 0.0;
                db[q] = diag ? da[q] : (on ? (double)b.v[u][q] - sB[q] : 0.0);
            }
            if constexpr (diag) {
#pragma unroll
                for (int q = 0; q < 4; ++q) cs[q] += da[q];
                nrows += on ? 1.0 : 0.0;
            }
#pragma unroll
            for (int qa = 0; qa < 4; ++qa)
#pragma unroll
                for (int qb = 0; qb < 4; ++qb)
                    if (!diag || qa <= qb)
                        acc[qa][qb] = __builtin_amdgcn_mfma_f64_16x16x4f64(da[qa], db[qb], acc[qa][qb], 0, 0, 0);
        }
        a = an;
        b = bn;
        ok = okn;
    }

    // the waves' tiles, added in wave order
    for (int w = 0; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int qa = 0; qa < 4; ++qa)
#pragma unroll
                for (int qb = 0; qb < 4; ++qb)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int row = 4 * (kk + 4 * i) + qa, col = 4 * m + qb;
                        if (w == 0)
                            red[row * kSuper + col] = acc[qa][qb][i];  // a tile that is not computed stays 0
                        else if (!diag || qa <= qb)
                            red[row * kSuper + col] += acc[qa][qb][i];
                    }
        }
        __syncthreads();
    }
    double* dst = work + (int64_t)blockIdx.x * chunk_stride;
    for (int i = threadIdx.x; i < kTile; i += 256) dst[pair * kTile + i] = red[i];
    if constexpr (diag) {
        // the four row groups of the wave in order, then the four waves in order
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const double v0 = __shfl(cs[q], m), v1 = __shfl(cs[q], m + 16), v2 = __shfl(cs[q], m + 32),
                         v3 = __shfl(cs[q], m + 48);
            if (kk == 0) csum[wave][4 * m + q] = ((v0 + v1) + v2) + v3;
        }
        const double n0 = __shfl(nrows, 0), n1 = __shfl(nrows, 16), n2 = __shfl(nrows, 32), n3 = __shfl(nrows, 48);
        if (lane == 0) cnt[wave] = ((n0 + n1) + n2) + n3;
        __syncthreads();
        if (threadIdx.x < kSuper)
            dst[npairs * kTile + (int64_t)I * kSuper + threadIdx.x] =
                ((csum[0][threadIdx.x] + csum[1][threadIdx.x]) + csum[2][threadIdx.x]) + csum[3][threadIdx.x];
        if (I == 0 && threadIdx.x == 0)
            dst[npairs * kTile + (int64_t)Fs * kSuper] = ((cnt[0] + cnt[1]) + cnt[2]) + cnt[3];
    }
}

// The diagonal pairs at 2 waves per SIMD (256 registers): the kernel is bound by the loads it has in flight.
template <bool VEC>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void pca_moments_diag_kernel(
    const float* __restrict__ X, int64_t ldx, int64_t P, int64_t F, const int32_t* __restrict__ counts,
    const float* __restrict__ shift, double* __restrict__ work, int64_t chunk_rows, int Fs, int64_t npairs,
    int64_t chunk_stride) {
    moments_body<VEC, true>(X, ldx, P, F, counts, shift, work, chunk_rows, Fs, npairs, chunk_stride);
}

template <bool VEC>
__global__ __launch_bounds__(256) void pca_moments_off_kernel(const float* __restrict__ X, int64_t ldx, int64_t P,
                                                              int64_t F, const int32_t* __restrict__ counts,
                                                              const float* __restrict__ shift,
                                                              double* __restrict__ work, int64_t chunk_rows, int Fs,
                                                              int64_t npairs, int64_t chunk_stride) {
    moments_body<VEC, false>(X, ldx, P, F, counts, shift, work, chunk_rows, Fs, npairs, chunk_stride);
}

// out[e] = the partials of output e over the chunks. 16 outputs x 16 runs of chunks per workgroup.
__global__ __launch_bounds__(256) void pca_moments_fold_kernel(const double* __restrict__ work, int64_t nchunks,
                                                               int64_t chunk_stride, int64_t F, int Fs, int64_t npairs,
                                                               double* __restrict__ out) {
    __shared__ double part[kFoldRuns][16];
    const int o = threadIdx.x & 15, run = threadIdx.x >> 4;
    const int64_t total = F * F + F + 1;
    const int64_t e = (int64_t)blockIdx.x * 16 + o;
    double sum = 0.0;
    if (e < total) {
        int64_t off;
        if (e < F * F) {
            int64_t ca = e / F, cb = e % F;
            int64_t I = ca / kSuper, J = cb / kSuper;
            int64_t la = ca % kSuper, lb = cb % kSuper;
            if (I > J || (I == J && (la & 3) > (lb & 3))) {  // the mirrored entry is the computed one
                int64_t t = I;
                I = J;
                J = t;
                t = la;
                la = lb;
                lb = t;
            }
            const int64_t pair = I * Fs - I * (I - 1) / 2 + (J - I);
            off = pair * kTile + la * kSuper + lb;
        } else if (e < F * F + F) {
            off = npairs * kTile + (e - F * F);
        } else {
            off = npairs * kTile + (int64_t)Fs * kSuper;
        }
        const int64_t per = (nchunks + kFoldRuns - 1) / kFoldRuns;
        const int64_t lo = per * run, hi = lo + per < nchunks ? lo + per : nchunks;
        for (int64_t c = lo; c < hi; ++c) sum += work[c * chunk_stride + off];
    }
    part[run][o] = sum;
    __syncthreads();
    if (run == 0 && e < total) {
        double s = part[0][o];
        for (int r = 1; r < kFoldRuns; ++r) s += part[r][o];
        out[e] = s;
    }
}

// ---- projection ---------------------------------------------------------------------------------------------------

constexpr int kPanelMax = 128;  // components per panel: 8 MFMA tiles of accumulators per wave

template <bool VEC, bool HALF>
__global__ __launch_bounds__(256) void pca_project_kernel(const float* __restrict__ X, int64_t ldx, int64_t P,
                                                          int64_t F, const int32_t* __restrict__ counts,
                                                          const float* __restrict__ center,
                                                          const float* __restrict__ W, int64_t k, void* __restrict__ out,
                                                          int64_t ldo, int Fp, int kp, int vec_out) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int ldw = Fp + 4;
    float* Ws = lds;
    float* Cs = lds + (int64_t)kp * ldw;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, g = lane >> 4;
    const int NT = kp / 16;
    for (int i = threadIdx.x; i < Fp; i += 256) Cs[i] = i < F ? center[i] : 0.f;
    const int64_t ntiles = (P + 15) / 16;
    for (int64_t pc0 = 0; pc0 < k; pc0 += kp) {
        __syncthreads();  // the previous panel has been read
        for (int i = threadIdx.x; i < kp * Fp; i += 256) {
            const int c = i / Fp, f = i - c * Fp;
            Ws[c * ldw + f] = (pc0 + c < k && f < F) ? W[(pc0 + c) * F + f] : 0.f;
        }
        __syncthreads();
        for (int64_t tile = (int64_t)blockIdx.x * 4 + wave; tile < ntiles; tile += (int64_t)gridDim.x * 4) {
            const int64_t row = tile * 16 + n;
            const bool rin = row < P;
            const bool ok = rin && (!counts || counts[row] > 0);
            f4_t acc[kPanelMax / 16];
#pragma unroll
            for (int t = 0; t < kPanelMax / 16; ++t) acc[t] = f4_t{0.f, 0.f, 0.f, 0.f};
            for (int f0 = 0; f0 < Fp; f0 += 16) {
                const int fc = f0 + 4 * g;
                float x[4] = {0.f, 0.f, 0.f, 0.f};
                if (ok) {
                    if constexpr (VEC) {
                        if (fc < F) {
                            const float4 v = *reinterpret_cast<const float4*>(X + row * ldx + fc);
                            x[0] = v.x;
                            x[1] = v.y;
                            x[2] = v.z;
                            x[3] = v.w;
                        }
                    } else {
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            if (fc + q < F) x[q] = X[row * ldx + fc + q];
                    }
                }
                const f4_t c = *reinterpret_cast<const f4_t*>(Cs + fc);
                float bq[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) bq[q] = ok ? x[q] - c[q] : 0.f;
#pragma unroll
                for (int t = 0; t < kPanelMax / 16; ++t) {
                    if (t < NT) {  // wave-uniform
                        const int comp = 32 * (t >> 1) + 8 * (n >> 2) + 4 * (t & 1) + (n & 3);
                        const f4_t a = *reinterpret_cast<const f4_t*>(Ws + comp * ldw + fc);
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[q], bq[q], acc[t], 0, 0, 0);
                    }
                }
            }
            if (!rin) continue;
            // D[4 g + i][n] of tile t is component 32 (t >> 1) + 8 g + 4 (t & 1) + i of row n
#pragma unroll
            for (int u = 0; u < kPanelMax / 32; ++u) {
                if (2 * u < NT) {
                    const int64_t cb = pc0 + 32 * u + 8 * g;
                    float v[8];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        v[i] = ok ? acc[2 * u][i] : 0.f;
                        v[4 + i] = ok ? acc[2 * u + 1][i] : 0.f;
                    }
                    if constexpr (HALF) {
                        _Float16* o = reinterpret_cast<_Float16*>(out) + row * ldo + cb;
                        if (vec_out && cb + 8 <= k) {
                            h8_t h;
#pragma unroll
                            for (int i = 0; i < 8; ++i) h[i] = (_Float16)v[i];  // round to nearest even
                            *reinterpret_cast<h8_t*>(o) = h;
                        } else {
#pragma unroll
                            for (int i = 0; i < 8; ++i)
                                if (cb + i < k) o[i] = (_Float16)v[i];
                        }
                    } else {
                        float* o = reinterpret_cast<float*>(out) + row * ldo + cb;
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            if (vec_out && cb + 4 * h + 4 <= k) {
                                *reinterpret_cast<f4_t*>(o + 4 * h) = f4_t{v[4 * h], v[4 * h + 1], v[4 * h + 2], v[4 * h + 3]};
                            } else {
#pragma unroll
                                for (int i = 0; i < 4; ++i)
                                    if (cb + 4 * h + i < k) o[4 * h + i] = v[4 * h + i];
                            }
                        }
                    }
                }
            }
        }
    }
}

template <bool VEC, bool HALF>
int launch_project(hipStream_t s, size_t lds, unsigned grid, const float* X, int64_t ldx, int64_t P, int64_t F,
                   const int32_t* counts, const float* center, const float* W, int64_t k, void* out, int64_t ldo, int Fp,
                   int kp, int vec_out) {
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&pca_project_kernel<VEC, HALF>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess)
            return pg::set_error(PG_ERR_HIP, "pg_pca_project: %zu bytes of LDS: %s", lds, hipGetErrorString(e));
    }
    hipLaunchKernelGGL((pca_project_kernel<VEC, HALF>), dim3(grid), dim3(256), lds, s, X, ldx, P, F, counts, center, W,
                       k, out, ldo, Fp, kp, vec_out);
    return PG_OK;
}

}  // namespace

extern "C" {

int64_t pg_pca_moments_workspace(int64_t P, int64_t F) {
    if (P < 0 || F < 1 || F > kMaxF) return -1;
    const MomentsPlan p = moments_plan(P, F);
    const int64_t n = p.nchunks * p.chunk_stride;
    return n > 0 ? n : 1;
}

int pg_pca_moments_f64(const float* X, int64_t ldx, int64_t P, int64_t F, const int32_t* counts, const float* shift,
                       double* out, double* work, int64_t work_doubles, void* stream) {
    const char* name = "pg_pca_moments_f64";
    PG_REQUIRE(P >= 0, "%s: negative size P=%lld", name, (long long)P);
    PG_REQUIRE(F >= 1 && F <= kMaxF, "%s: F=%lld must be in [1, %lld]", name, (long long)F, (long long)kMaxF);
    PG_REQUIRE(ldx >= F, "%s: row stride ldx=%lld must be >= F=%lld", name, (long long)ldx, (long long)F);
    PG_REQUIRE(out && work && (X || P == 0), "%s: null pointer", name);
    PG_REQUIRE(work_doubles >= pg_pca_moments_workspace(P, F), "%s: workspace of %lld doubles, %lld needed", name,
               (long long)work_doubles, (long long)pg_pca_moments_workspace(P, F));
    const MomentsPlan p = moments_plan(P, F);
    hipStream_t s = (hipStream_t)stream;
    if (p.nchunks > 0) {
        const bool vec = F % 4 == 0 && ldx % 4 == 0 && pg::aligned16(X);
        const dim3 gd((unsigned)p.nchunks, (unsigned)p.Fs), go((unsigned)p.nchunks, (unsigned)(p.npairs - p.Fs));
        if (vec)
            hipLaunchKernelGGL((pca_moments_diag_kernel<true>), gd, dim3(256), 0, s, X, ldx, P, F, counts, shift, work,
                               p.chunk_rows, p.Fs, p.npairs, p.chunk_stride);
        else
            hipLaunchKernelGGL((pca_moments_diag_kernel<false>), gd, dim3(256), 0, s, X, ldx, P, F, counts, shift,
                               work, p.chunk_rows, p.Fs, p.npairs, p.chunk_stride);
        int rc = pg::check_launch(name);
        if (rc != PG_OK) return rc;
        if (p.npairs > p.Fs) {  // the pairs I < J
            if (vec)
                hipLaunchKernelGGL((pca_moments_off_kernel<true>), go, dim3(256), 0, s, X, ldx, P, F, counts, shift,
                                   work, p.chunk_rows, p.Fs, p.npairs, p.chunk_stride);
            else
                hipLaunchKernelGGL((pca_moments_off_kernel<false>), go, dim3(256), 0, s, X, ldx, P, F, counts, shift,
                                   work, p.chunk_rows, p.Fs, p.npairs, p.chunk_stride);
            rc = pg::check_launch(name);
            if (rc != PG_OK) return rc;
        }
    }
    const int64_t total = F * F + F + 1;
    hipLaunchKernelGGL(pca_moments_fold_kernel, dim3((unsigned)((total + 15) / 16)), dim3(256), 0, s, work, p.nchunks,
                       p.chunk_stride, F, p.Fs, p.npairs, out);
    return pg::check_launch(name);
}

int pg_pca_project(const float* X, int64_t ldx, int64_t P, int64_t F, const int32_t* counts, const float* center,
                   const float* W, int64_t k, void* out, int64_t ldo, int out_dtype, void* stream) {
    const char* name = "pg_pca_project";
    PG_REQUIRE(P >= 0, "%s: negative size P=%lld", name, (long long)P);
    PG_REQUIRE(F >= 1 && F <= kMaxF, "%s: F=%lld must be in [1, %lld]", name, (long long)F, (long long)kMaxF);
    PG_REQUIRE(k >= 1 && k <= F, "%s: k=%lld must be in [1, F=%lld]", name, (long long)k, (long long)F);
    PG_REQUIRE(ldx >= F && ldo >= k, "%s: row strides ldx=%lld ldo=%lld must be >= F=%lld, k=%lld", name,
               (long long)ldx, (long long)ldo, (long long)F, (long long)k);
    PG_REQUIRE(out_dtype == 0 || out_dtype == 1, "%s: out_dtype must be 0 (fp16) or 1 (fp32)", name);
    if (P == 0) return PG_OK;
    PG_REQUIRE(X && center && W && out, "%s: null pointer", name);
    const int Fp = (int)((F + 15) / 16 * 16);
    int kp = (int)((k + 31) / 32 * 32);
    if (kp > kPanelMax) kp = kPanelMax;
    auto lds_bytes = [&](int c) { return ((size_t)c * (Fp + 4) + Fp) * sizeof(float); };
    while (kp > 32 && lds_bytes(kp) > 64 * 1024) kp -= 32;
    const bool half = out_dtype == 0;
    const int vec_out = pg::aligned16(out) && ldo % (half ? 8 : 4) == 0;
    const bool vec = F % 4 == 0 && ldx % 4 == 0 && pg::aligned16(X);
    const int64_t blocks = ((P + 15) / 16 + 3) / 4;
    const unsigned grid = (unsigned)(blocks < 1024 ? blocks : 1024);
    hipStream_t s = (hipStream_t)stream;
    int rc;
    if (vec)
        rc = half ? launch_project<true, true>(s, lds_bytes(kp), grid, X, ldx, P, F, counts, center, W, k, out, ldo, Fp,
                                               kp, vec_out)
                  : launch_project<true, false>(s, lds_bytes(kp), grid, X, ldx, P, F, counts, center, W, k, out, ldo,
                                                Fp, kp, vec_out);
    else
        rc = half ? launch_project<false, true>(s, lds_bytes(kp), grid, X, ldx, P, F, counts, center, W, k, out, ldo,
                                                Fp, kp, vec_out)
                  : launch_project<false, false>(s, lds_bytes(kp), grid, X, ldx, P, F, counts, center, W, k, out, ldo,
                                                 Fp, kp, vec_out);
    if (rc != PG_OK) return rc;
    return pg::check_launch(name);
}

}  // extern "C"
