// classify.hip -- softmax regression over a table of vectors behind the C ABI: ge_classify_* (include/geglove.h,
// "Classification").  The rows are prepared once on the device as kmeans.hip prepares them, with a column of ones behind them
// (k_cls_prepare).  An evaluation computes the logits of the training members on the fp32 matrix cores (k_cls_logits: the score
// tile of k_km_assign writing z), turns every row into its loss term and its residuals with an fp64 exp and log that the header
// spells out operation for operation (k_cls_softmax), forms the gradient as one fmaf chain per piece of 1024 members on the
// matrix cores (k_cls_gradient, the members along k) and adds the pieces in fp64 in ascending order (k_cls_piece_sum,
// k_cls_block_sums): no floating-point atomics, so every byte that comes back is a function of the input alone.  The optimiser
// is L-BFGS in fp64 on the host.  The reference has no counterpart.
#include "ge_common.h"
#include "ge_glove_internal.h"
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <deque>
#include <memory>
#include <vector>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int CLS_MAX_DIM = 1024, CLS_MAX_C = 1024;
constexpr int64_t CLS_MAX_FLOATS = (int64_t)1 << 35;         // floats of input one handle accepts, as ge_kmeans_create
constexpr int64_t CLS_MAX_LOGITS = (int64_t)1 << 33;         // n * C
constexpr int64_t CLS_SLAB_FLOATS = (int64_t)1 << 26;        // a 256 MB slab of rows per upload, and of logits per prediction chunk
constexpr int CLS_PIECE = 1024;                              // members per piece of the gradient, and per block of the loss
constexpr int CLS_HISTORY = 8, CLS_TRIALS = 30;

// ---------------------------------------------------------------------------------------------------------------------
// exp and log of the header, fp64, every operation unfused (-ffp-contract=off) and rounded to nearest even.
// ---------------------------------------------------------------------------------------------------------------------
constexpr double LN2HI = 6.93147180369123816490e-01, LN2LO = 1.90821492927058770002e-10, INVLN2 = 1.4426950408889634;
constexpr double CUT = 8.673617379884035e-19;                // 2^-60

__device__ __forceinline__ double cls_exp(double t) {       // t <= 0
    if (t < -708.0) return 0.0;
    const double k = rint(t * INVLN2);
    const double r = (t - k * LN2HI) - k * LN2LO;
    double p = 1.0 / 6227020800.0;
    p = p * r + 1.0 / 479001600.0;
    p = p * r + 1.0 / 39916800.0;
    p = p * r + 1.0 / 3628800.0;
    p = p * r + 1.0 / 362880.0;
    p = p * r + 1.0 / 40320.0;
    p = p * r + 1.0 / 5040.0;
    p = p * r + 1.0 / 720.0;
    p = p * r + 1.0 / 120.0;
    p = p * r + 1.0 / 24.0;
    p = p * r + 1.0 / 6.0;
    p = p * r + 1.0 / 2.0;
    p = p * r + 1.0;
    p = p * r + 1.0;
    return ldexp(p, (int)k);
}

__device__ __forceinline__ double cls_log(double S) {       // S >= 1
    int k;
    double f = frexp(S, &k);
    if (f < 0.70710678118654752440) { f = 2.0 * f; k = k - 1; }
    const double s = (f - 1.0) / (f + 1.0), w = s * s;
    double q = 1.0 / 25.0;
    q = q * w + 1.0 / 23.0;
    q = q * w + 1.0 / 21.0;
    q = q * w + 1.0 / 19.0;
    q = q * w + 1.0 / 17.0;
    q = q * w + 1.0 / 15.0;
    q = q * w + 1.0 / 13.0;
    q = q * w + 1.0 / 11.0;
    q = q * w + 1.0 / 9.0;
    q = q * w + 1.0 / 7.0;
    q = q * w + 1.0 / 5.0;
    q = q * w + 1.0 / 3.0;
    q = q * w + 1.0;
    const double kd = (double)k;
    return kd * LN2HI + (kd * LN2LO + (2.0 * s) * q);
}

// ---------------------------------------------------------------------------------------------------------------------
// Prepare.  k_km_prepare's walk (one wave takes 64 rows; the fp64 sum of squares of a row is a sequential chain over ascending d
// that lane r walks in LDS), writing rows of Dp4 floats: the dim prepared values, 1.0f at [dim], zeros behind it.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int PREP_ROWS = 64, PREP_COLS = 64, PREP_STRIDE = 65;

__global__ __launch_bounds__(64) void k_cls_prepare(const float *__restrict__ src, const int32_t *__restrict__ rowmap, int64_t n_rows, int32_t D,
                                                    int32_t Dp4, int32_t normalize, float *__restrict__ out, int32_t *__restrict__ flag) {
    __shared__ float tile[PREP_ROWS * PREP_STRIDE];
    __shared__ double norm[PREP_ROWS];
    const int lane = (int)threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * PREP_ROWS;
    const int rows = (int)(n_rows - row0 < PREP_ROWS ? n_rows - row0 : PREP_ROWS);
    bool bad = false;
    if (normalize == GE_CLS_COSINE) {
        double sum = 0.0;
        for (int d0 = 0; d0 < D; d0 += PREP_COLS) {
            const int d = d0 + lane;
            for (int r = 0; r < rows; ++r) {
                const int64_t s = rowmap ? (int64_t)rowmap[row0 + r] : row0 + r;
                tile[r * PREP_STRIDE + lane] = d < D ? src[s * D + d] : 0.0f;
            }
            __syncthreads();
            const int lim = D - d0 < PREP_COLS ? D - d0 : PREP_COLS;
            if (lane < rows)
                for (int c = 0; c < lim; ++c) {
                    const double x = (double)tile[lane * PREP_STRIDE + c];
                    sum += x * x;
                }
            __syncthreads();
        }
        norm[lane] = sqrt(sum);
        __syncthreads();
    }
    for (int d0 = 0; d0 < Dp4; d0 += PREP_COLS) {
        const int d = d0 + lane;
        if (d >= Dp4) break;
        for (int r = 0; r < rows; ++r) {
            const int64_t s = rowmap ? (int64_t)rowmap[row0 + r] : row0 + r;
            float x = d < D ? src[s * D + d] : 0.0f;
            bad |= !(fabsf(x) <= 3.402823466e38f);
            if (normalize == GE_CLS_COSINE) {
                const double n = norm[r];
                x = n > 0.0 ? (float)((double)x / n) : 0.0f;
            }
            out[(row0 + r) * Dp4 + d] = d == D ? 1.0f : x;
        }
    }
    if (bad) *flag = 1;
}

// ---------------------------------------------------------------------------------------------------------------------
// Logits.  The score tile of k_km_assign: a workgroup owns 64 rows and walks the C classes in tiles of 128; per 32 columns the
// row and weight panels are staged in LDS as [row][34], the next panel travelling in registers meanwhile, and wave w carries
// rows 16 w .. 16 w + 15 against the 128 classes through v_mfma_f32_16x16x4_f32: eight accumulators, each bit for bit an fmaf
// chain over ascending d (the ones column makes the bias the chain's last live product).  The epilogue writes z[row][c].
// rows: NULL (row q of the tile is position q) or the position of every row (the training members).
// ---------------------------------------------------------------------------------------------------------------------
constexpr int KL_TQ = 64, KL_TC = 128, KL_DK = 32, KL_LS = 34;
constexpr int KL_LOADS = (KL_TQ + KL_TC) * (KL_DK / 4) / 256;   // 16-byte pieces a thread moves per panel: 2 of rows, 4 of weights

__global__ __launch_bounds__(256, 3) void k_cls_logits(const float *__restrict__ X, const int32_t *__restrict__ rows, int64_t n,
                                                       const float *__restrict__ W, int32_t C, int32_t D4, float *__restrict__ z) {
    __shared__ float sq[KL_TQ * KL_LS];
    __shared__ float sx[KL_TC * KL_LS];

    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t q0 = (int64_t)blockIdx.x * KL_TQ;

    const int c4 = (tid & 7) * 4, prow = tid >> 3;
    const float *qsrc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int64_t qg = q0 + prow + 32 * i;
        qsrc[i] = qg < n ? X + (rows ? (int64_t)rows[qg] : qg) * D4 : nullptr;
    }
    f32x4 pre[KL_LOADS];
    auto fetch = [&](int ct, int d0) {
        const bool in = d0 + c4 < D4;
#pragma unroll
        for (int i = 0; i < 2; ++i)
            pre[i] = in && qsrc[i] ? *reinterpret_cast<const f32x4 *>(qsrc[i] + d0 + c4) : f32x4{0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = ct + prow + 32 * i;
            pre[2 + i] = in && c < C ? *reinterpret_cast<const f32x4 *>(W + (int64_t)c * D4 + d0 + c4) : f32x4{0, 0, 0, 0};
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int i = 0; i < KL_LOADS; ++i) {
            float *dst = (i < 2 ? sq + (prow + 32 * i) * KL_LS : sx + (prow + 32 * (i - 2)) * KL_LS) + c4;   // 8-byte aligned: KL_LS and c4 are even
            *reinterpret_cast<float2 *>(dst) = float2{pre[i][0], pre[i][1]};
            *reinterpret_cast<float2 *>(dst + 2) = float2{pre[i][2], pre[i][3]};
        }
    };

    const int qb = wave * 16;
    const int ql = qb + 4 * (lane >> 4);
    const int xa = (qb + (lane & 15)) * KL_LS + (lane >> 4);
    const int xb = (lane & 15) * KL_LS + (lane >> 4);

    fetch(0, 0);
    for (int ct = 0; ct < C; ct += KL_TC) {
        f32x4 acc[KL_TC / 16];
#pragma unroll
        for (int t = 0; t < KL_TC / 16; ++t) acc[t] = f32x4{0, 0, 0, 0};
        for (int d0 = 0; d0 < D4; d0 += KL_DK) {
            __syncthreads();
            stage();
            __syncthreads();
            if (d0 + KL_DK < D4) fetch(ct, d0 + KL_DK);
            else if (ct + KL_TC < C) fetch(ct + KL_TC, 0);
            auto step = [&](int dd) {
                const float a = sq[xa + dd];
                float b[KL_TC / 16];
#pragma unroll
                for (int t = 0; t < KL_TC / 16; ++t) b[t] = sx[xb + t * 16 * KL_LS + dd];
#pragma unroll
                for (int t = 0; t < KL_TC / 16; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b[t], acc[t], 0, 0, 0);
            };
            if (D4 - d0 >= KL_DK) {
#pragma unroll
                for (int dd = 0; dd < KL_DK; dd += 4) step(dd);
            } else {
#pragma unroll 1
                for (int dd = 0; dd < D4 - d0; dd += 4) step(dd);
            }
        }
        // C/D of the f32 form: column (class) = lane & 15, row = 4 * (lane >> 4) + register
#pragma unroll
        for (int t = 0; t < KL_TC / 16; ++t) {
            const int c = ct + t * 16 + (lane & 15);
            if (c >= C) continue;
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int64_t p = q0 + ql + reg;
                if (p < n) z[p * C + c] = acc[t][reg];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Softmax.  One row per lane, its C logits walked in ascending c three times: the maximum (fp32 compares, the first of equals),
// S (the fp64 chain over ascending c), then what the row is for.  y != NULL (an evaluation): the loss term and the residuals of
// member t.  y == NULL (a prediction): the label and its probability.  A non-finite logit raises *flag.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_cls_softmax(const float *__restrict__ z, int64_t n, int32_t C, const int32_t *__restrict__ y,
                                                    double *__restrict__ loss, float *__restrict__ r, int32_t *__restrict__ label,
                                                    float *__restrict__ prob, int32_t *__restrict__ flag) {
    const int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (t >= n) return;
    const float *zr = z + t * C;
    float m = zr[0];
    int32_t best = 0;
    bool bad = !(fabsf(m) <= 3.402823466e38f);
    for (int c = 1; c < C; ++c) {
        const float v = zr[c];
        bad |= !(fabsf(v) <= 3.402823466e38f);
        if (v > m) { m = v; best = c; }
    }
    if (bad) { *flag = 1; return; }
    double S = 0.0;
    for (int c = 0; c < C; ++c) S = S + cls_exp((double)zr[c] - (double)m);
    if (!y) {
        label[t] = best;
        prob[t] = (float)(1.0 / S);
        return;
    }
    const int32_t yt = y[t];
    loss[t] = cls_log(S) - ((double)zr[yt] - (double)m);
    float *rr = r + t * C;
    for (int c = 0; c < C; ++c) {
        const double q = cls_exp((double)zr[c] - (double)m) / S;
        const float pf = q < CUT ? 0.0f : (float)q;
        rr[c] = pf - (c == yt ? 1.0f : 0.0f);
    }
}

// the block sums of the loss: block b's terms added in ascending t by one lane, from LDS
__global__ __launch_bounds__(64) void k_cls_block_sums(const double *__restrict__ v, int64_t n, double *__restrict__ sums) {
    __shared__ double s_t[CLS_PIECE];
    const int64_t b0 = (int64_t)blockIdx.x * CLS_PIECE;
    const int cnt = (int)((n - b0 < CLS_PIECE) ? n - b0 : CLS_PIECE);
    for (int q = threadIdx.x; q < cnt; q += 64) s_t[q] = v[b0 + q];
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0;
        for (int q = 0; q < cnt; ++q) a = a + s_t[q];
        sums[blockIdx.x] = a;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Gradient.  blockIdx.x = piece (1024 consecutive members), blockIdx.y = a tile of 16 GA classes, blockIdx.z = a tile of 256
// columns; wave w of the workgroup owns columns 64 w .. 64 w + 63 of the tile as four B fragments, against GA A fragments of 16
// classes: 4 GA accumulators that stay in registers for the whole piece.  One product takes four members along k: A is 16
// classes x 4 members (lane: class lane & 15 of member lane >> 4, sixteen consecutive floats of a residual row), B is 4 members
// x 16 columns (sixteen consecutive floats of a feature row), so every accumulator element is the fmaf chain over the piece's
// members in ascending t.  Sixteen members are taken per turn: their positions are read once (lane & 15) and passed round.
// Members past the end of a piece, classes past C and columns past Dp4 enter as zeros: fmaf(0, 0, s) = s.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int KG_DW = 64, KG_DT = 256;

template <int GA>
__global__ __launch_bounds__(256) void k_cls_gradient(const float *__restrict__ X, const int32_t *__restrict__ mem, int64_t n_t,
                                                      const float *__restrict__ r, int32_t C, int32_t D4, float *__restrict__ Gp) {
    const int lane = (int)threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int d0 = (int)blockIdx.z * KG_DT + wave * KG_DW;
    if (d0 >= D4) return;                                   // the whole wave; there is no barrier below
    const int c0 = (int)blockIdx.y * 16 * GA;
    const int64_t t0 = (int64_t)blockIdx.x * CLS_PIECE;
    const int cnt = (int)(n_t - t0 < CLS_PIECE ? n_t - t0 : CLS_PIECE);
    const int kk = lane >> 4, ll = lane & 15;

    f32x4 acc[GA][4];
#pragma unroll
    for (int a = 0; a < GA; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0, 0, 0, 0};
    bool ain[GA], bin[4];
#pragma unroll
    for (int a = 0; a < GA; ++a) ain[a] = c0 + 16 * a + ll < C;
#pragma unroll
    for (int b = 0; b < 4; ++b) bin[b] = d0 + 16 * b + ll < D4;

    for (int m0 = 0; m0 < cnt; m0 += 16) {
        const int32_t mine = m0 + ll < cnt ? mem[t0 + m0 + ll] : -1;
        float av[4][GA], bv[4][4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int32_t pos = __shfl(mine, 4 * s + kk, 64);
            const bool live = pos >= 0;                     // m0 + 4 s + kk < cnt
            const float *rr = r + (t0 + m0 + 4 * s + kk) * C + c0 + ll;
            const float *xr = X + (int64_t)(live ? pos : 0) * D4 + d0 + ll;
#pragma unroll
            for (int a = 0; a < GA; ++a) av[s][a] = live && ain[a] ? rr[16 * a] : 0.0f;
#pragma unroll
            for (int b = 0; b < 4; ++b) bv[s][b] = live && bin[b] ? xr[16 * b] : 0.0f;
        }
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int a = 0; a < GA; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s][a], bv[s][b], acc[a][b], 0, 0, 0);
    }
    // C/D of the f32 form: column (dimension) = lane & 15, row (class) = 4 * (lane >> 4) + register
    float *out = Gp + (int64_t)blockIdx.x * C * D4;
#pragma unroll
    for (int a = 0; a < GA; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int d = d0 + 16 * b + ll;
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int c = c0 + 16 * a + 4 * kk + reg;
                if (c < C && d < D4) out[(int64_t)c * D4 + d] = acc[a][b][reg];
            }
        }
}

// G[c][d] = the fp64 sum from 0.0 of (double)Gp[piece][c][d] over ascending pieces; one element per lane
__global__ __launch_bounds__(256) void k_cls_piece_sum(const float *__restrict__ Gp, int64_t pieces, int64_t elems, double *__restrict__ G) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= elems) return;
    double s = 0.0;
    for (int64_t q = 0; q < pieces; ++q) s = s + (double)Gp[q * elems + e];
    G[e] = s;
}

struct DeviceBuffers {                      // freed on every way out
    std::vector<void *> ptrs;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~DeviceBuffers() { for (void *q : ptrs) (void)hipFree(q); if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
    ge_status alloc(void **q, size_t bytes) { GE_HIP(hipMalloc(q, std::max<size_t>(bytes, 16))); ptrs.push_back(*q); return GE_OK; }
    ge_status events() { GE_HIP(hipEventCreate(&e0)); GE_HIP(hipEventCreate(&e1)); return GE_OK; }
};

// the fp64 sum from 0.0 over ascending index of the unfused products
inline double dot(const std::vector<double> &a, const std::vector<double> &b) {
    double s = 0.0;
    for (size_t i = 0; i < a.size(); ++i) s = s + a[i] * b[i];
    return s;
}

struct Pair { std::vector<double> s, y; double sy; };

}  // namespace

struct ge_classifier {
    int32_t normalize = 0, device = 0, dim = 0, dp = 0, dp4 = 0, classes = 0;
    int64_t n = 0, n_t = 0, pieces = 0, zrows = 0;
    double l2 = 0.0, tolerance = 0.0;
    hipStream_t stream = nullptr;
    DeviceBuffers B;                         // everything below lives here
    float *dx = nullptr, *dw = nullptr, *dz = nullptr, *dr = nullptr, *dgp = nullptr, *dprob = nullptr;
    int32_t *dmem = nullptr, *dy = nullptr, *dlabel = nullptr, *dflag = nullptr;
    double *dloss = nullptr, *dblock = nullptr, *dg = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    std::vector<int32_t> labels;             // of every position, -1 = none
    std::vector<double> theta, grad;         // the master copy, and the gradient at it when `have`
    std::deque<Pair> H;                      // oldest first
    bool have = false;
    double loss = 0.0;
    int32_t iterations = 0, stop = 0;
    int64_t evaluations = 0;
    float logits_ms = 0, softmax_ms = 0, gradient_ms = 0;
    ~ge_classifier() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
};

namespace {

ge_status check_cfg(const ge_classify_cfg *cfg) {
    if (!cfg) return ge::fail(GE_ERR_ARG, "ge_classify_cfg is null");
    if (cfg->normalize != GE_CLS_COSINE && cfg->normalize != GE_CLS_RAW) return ge::fail(GE_ERR_ARG, "classify: unknown normalize %d", cfg->normalize);
    if (cfg->classes < 2 || cfg->classes > CLS_MAX_C) return ge::fail(GE_ERR_ARG, "classify: classes %d outside [2, %d]", cfg->classes, CLS_MAX_C);
    if (!(cfg->l2 >= 0.0) || !std::isfinite(cfg->l2)) return ge::fail(GE_ERR_ARG, "classify: l2 %g is not a finite number >= 0", cfg->l2);
    if (!(cfg->tolerance >= 0.0)) return ge::fail(GE_ERR_ARG, "classify: tolerance %g is not a number >= 0", cfg->tolerance);
    return GE_OK;
}

ge_status check_create(int64_t n_rows, int32_t dim, const int32_t *subset, int64_t n_subset, const int32_t *labels, const uint8_t *train,
                       const ge_classify_cfg *cfg) {
    GE_CHECK(check_cfg(cfg));
    if (!labels) return ge::fail(GE_ERR_ARG, "classify: labels is null");
    if (dim < 1 || dim > CLS_MAX_DIM) return ge::fail(GE_ERR_ARG, "classify: dim %d outside [1, %d]", dim, CLS_MAX_DIM);
    if (n_rows < 1 || n_rows >= INT_MAX) return ge::fail(GE_ERR_ARG, "classify: %lld rows outside [1, 2^31 - 2]", (long long)n_rows);
    if (n_rows > CLS_MAX_FLOATS / dim)
        return ge::fail(GE_ERR_ARG, "classify: %lld rows of %d floats are more than one handle holds (%lld floats)", (long long)n_rows, dim,
                        (long long)CLS_MAX_FLOATS);
    if (subset) {
        if (n_subset < 1 || n_subset > n_rows) return ge::fail(GE_ERR_ARG, "classify: a subset of %lld of %lld rows", (long long)n_subset, (long long)n_rows);
        for (int64_t i = 0; i < n_subset; ++i) {
            if (subset[i] < 0 || subset[i] >= n_rows)
                return ge::fail(GE_ERR_ARG, "classify: subset[%lld] = %d outside [0, %lld)", (long long)i, subset[i], (long long)n_rows);
            if (i > 0 && subset[i] <= subset[i - 1]) return ge::fail(GE_ERR_ARG, "classify: the subset is not strictly ascending at [%lld]", (long long)i);
        }
    }
    const int64_t n = subset ? n_subset : n_rows;
    if (n > CLS_MAX_LOGITS / cfg->classes)
        return ge::fail(GE_ERR_ARG, "classify: %lld positions times %d classes are more than 2^33 logits", (long long)n, cfg->classes);
    int64_t n_t = 0;
    for (int64_t p = 0; p < n; ++p) {
        if (labels[p] < -1 || labels[p] >= cfg->classes)
            return ge::fail(GE_ERR_ARG, "classify: labels[%lld] = %d outside [-1, %d)", (long long)p, labels[p], cfg->classes);
        n_t += labels[p] >= 0 && (!train || train[p]) ? 1 : 0;
    }
    if (n_t < 1) return ge::fail(GE_ERR_ARG, "classify: no training member (a labelled position whose train flag is set)");
    return GE_OK;
}

// rows (host: slab by slab; dev: in place) -> table[rows_out][dp4], prepared
ge_status prepare_rows(const float *host, const float *dev, const int32_t *host_map, const int32_t *dev_map, int64_t rows_out, int32_t dim,
                       int32_t dp4, int32_t normalize, float *table, hipStream_t stream) {
    const int D = dim;
    const int64_t slab_rows = std::min<int64_t>(std::max<int64_t>(PREP_ROWS, CLS_SLAB_FLOATS / D / PREP_ROWS * PREP_ROWS), rows_out);
    DeviceBuffers B;
    float *dslab = nullptr;
    int32_t *dflag = nullptr;
    if (host) GE_CHECK(B.alloc((void **)&dslab, sizeof(float) * (size_t)slab_rows * D));
    GE_CHECK(B.alloc((void **)&dflag, sizeof(int32_t)));
    GE_HIP(hipMemsetAsync(dflag, 0, sizeof(int32_t), stream));
    std::vector<float> packed;
    if (host && host_map) packed.resize((size_t)slab_rows * D);
    for (int64_t begin = 0; begin < rows_out; begin += slab_rows) {
        const int64_t rows = std::min(slab_rows, rows_out - begin);
        const float *x = dev;
        const int32_t *map = dev ? (dev_map ? dev_map + begin : nullptr) : nullptr;
        if (host) {
            const float *from = host + begin * D;
            if (host_map) {
                for (int64_t r = 0; r < rows; ++r) std::memcpy(&packed[(size_t)r * D], host + (int64_t)host_map[begin + r] * D, sizeof(float) * (size_t)D);
                from = packed.data();
            }
            GE_HIP(hipMemcpyAsync(dslab, from, sizeof(float) * (size_t)rows * D, hipMemcpyHostToDevice, stream));
            x = dslab;
        } else if (!dev_map) {
            x = dev + begin * D;
        }
        hipLaunchKernelGGL(k_cls_prepare, dim3((unsigned)((rows + PREP_ROWS - 1) / PREP_ROWS)), dim3(64), 0, stream, x, map, rows, D, dp4, normalize,
                           table + begin * dp4, dflag);
        GE_HIP(hipGetLastError());
        GE_HIP(hipStreamSynchronize(stream));                                       // the slab buffer (and `packed`) are free again
    }
    int32_t flag = 0;
    GE_HIP(hipMemcpyAsync(&flag, dflag, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    GE_HIP(hipStreamSynchronize(stream));
    if (flag) return ge::fail(GE_ERR_ARG, "classify: non-finite input (rows)");
    return GE_OK;
}

ge_status create_impl(const float *host, const float *dev, int64_t n_rows, int32_t dim, const int32_t *subset, int64_t n_subset, const int32_t *labels,
                      const uint8_t *train, const ge_classify_cfg *cfg, ge_classifier **out) {
    std::unique_ptr<ge_classifier> p(new ge_classifier);
    p->normalize = cfg->normalize; p->device = cfg->device; p->stream = (hipStream_t)cfg->stream; p->classes = cfg->classes;
    p->l2 = cfg->l2; p->tolerance = cfg->tolerance;
    p->dim = dim; p->dp = dim + 1; p->dp4 = (dim + 1 + 3) / 4 * 4; p->n = subset ? n_subset : n_rows;
    p->labels.assign(labels, labels + p->n);
    std::vector<int32_t> mem, y;
    for (int64_t q = 0; q < p->n; ++q)
        if (labels[q] >= 0 && (!train || train[q])) { mem.push_back((int32_t)q); y.push_back(labels[q]); }
    p->n_t = (int64_t)mem.size();
    p->pieces = (p->n_t + CLS_PIECE - 1) / CLS_PIECE;
    // the logits of an evaluation all at once (the gradient reads every residual); a prediction goes through the same buffer in chunks
    p->zrows = std::max<int64_t>(p->n_t, std::min<int64_t>(p->n, std::max<int64_t>(KL_TQ, CLS_SLAB_FLOATS / p->classes)));
    const size_t N = (size_t)p->n, NT = (size_t)p->n_t, C = (size_t)p->classes, D4 = (size_t)p->dp4;
    p->theta.assign(C * (size_t)p->dp, 0.0);
    p->grad.assign(C * (size_t)p->dp, 0.0);
    DeviceBuffers &B = p->B;
    int32_t *dids = nullptr;
    GE_CHECK(B.alloc((void **)&p->dx, sizeof(float) * N * D4));
    GE_CHECK(B.alloc((void **)&p->dw, sizeof(float) * C * D4));
    GE_CHECK(B.alloc((void **)&p->dz, sizeof(float) * (size_t)p->zrows * C));
    GE_CHECK(B.alloc((void **)&p->dr, sizeof(float) * NT * C));
    GE_CHECK(B.alloc((void **)&p->dgp, sizeof(float) * (size_t)p->pieces * C * D4));
    GE_CHECK(B.alloc((void **)&p->dg, sizeof(double) * C * D4));
    GE_CHECK(B.alloc((void **)&p->dloss, sizeof(double) * NT));
    GE_CHECK(B.alloc((void **)&p->dblock, sizeof(double) * (size_t)p->pieces));
    GE_CHECK(B.alloc((void **)&p->dmem, sizeof(int32_t) * NT));
    GE_CHECK(B.alloc((void **)&p->dy, sizeof(int32_t) * NT));
    GE_CHECK(B.alloc((void **)&p->dlabel, sizeof(int32_t) * (size_t)p->zrows));
    GE_CHECK(B.alloc((void **)&p->dprob, sizeof(float) * (size_t)p->zrows));
    GE_CHECK(B.alloc((void **)&p->dflag, sizeof(int32_t)));
    for (hipEvent_t &e : p->ev) GE_HIP(hipEventCreate(&e));
    if (subset && dev) {
        GE_CHECK(B.alloc((void **)&dids, sizeof(int32_t) * N));
        GE_HIP(hipMemcpyAsync(dids, subset, sizeof(int32_t) * N, hipMemcpyHostToDevice, p->stream));
    }
    GE_HIP(hipMemcpyAsync(p->dmem, mem.data(), sizeof(int32_t) * NT, hipMemcpyHostToDevice, p->stream));
    GE_HIP(hipMemcpyAsync(p->dy, y.data(), sizeof(int32_t) * NT, hipMemcpyHostToDevice, p->stream));
    GE_CHECK(prepare_rows(host, dev, subset, dids, p->n, dim, p->dp4, p->normalize, p->dx, p->stream));   // drains the stream: `mem`, `y` may go
    *out = p.release();
    return GE_OK;
}

ge_status cls_create_host(const float *rows, int64_t n_rows, int32_t dim, const int32_t *subset, int64_t n_subset, const int32_t *labels,
                          const uint8_t *train, const ge_classify_cfg *cfg, ge_classifier **out) {
    if (out) *out = nullptr;
    if (!rows || !out) return ge::fail(GE_ERR_ARG, "ge_classify_create: rows or out is null");
    GE_CHECK(check_create(n_rows, dim, subset, n_subset, labels, train, cfg));
    GE_CHECK(ge::select_device(cfg->device));
    return create_impl(rows, nullptr, n_rows, dim, subset, n_subset, labels, train, cfg, out);
}

ge_status cls_create_glove(ge_glove *h, const int32_t *subset, int64_t n_subset, const int32_t *labels, const uint8_t *train,
                           const ge_classify_cfg *cfg, ge_classifier **out) {
    if (out) *out = nullptr;
    if (!h || !out) return ge::fail(GE_ERR_ARG, "ge_glove_classify_create: handle or out is null");
    GE_CHECK(check_cfg(cfg));
    if (!labels) return ge::fail(GE_ERR_ARG, "classify: labels is null");
    float *d = nullptr;
    int32_t V = 0, D = 0, device = 0;
    GE_CHECK(ge::glove_extract_device_f32(h, &d, &V, &D, &device));   // a fresh buffer: no trainer table is written
    ge_classify_cfg own = *cfg;
    own.device = device;                                              // the rows live on the handle's device
    ge_status st = check_create(V, D, subset, n_subset, labels, train, &own);
    if (st == GE_OK) st = create_impl(nullptr, d, V, D, subset, n_subset, labels, train, &own, out);
    (void)hipFree(d);
    return st;
}

// W = (float)theta, padded to dp4, onto the device
ge_status upload_weights(ge_classifier *p, const std::vector<double> &theta, std::vector<float> &w) {
    const size_t C = (size_t)p->classes, Dp = (size_t)p->dp, D4 = (size_t)p->dp4;
    w.assign(C * D4, 0.0f);
    for (size_t c = 0; c < C; ++c)
        for (size_t d = 0; d < Dp; ++d) w[c * D4 + d] = (float)theta[c * Dp + d];
    GE_HIP(hipMemcpyAsync(p->dw, w.data(), sizeof(float) * C * D4, hipMemcpyHostToDevice, p->stream));
    return GE_OK;
}

// (f, g) at theta.  *finite = false (and f, g untouched) when a logit is not finite.
ge_status evaluate(ge_classifier *p, const std::vector<double> &theta, double *f, std::vector<double> &g, bool *finite) {
    hipStream_t stream = p->stream;
    const int32_t C = p->classes, D4 = p->dp4, Dp = p->dp;
    const int64_t NT = p->n_t, pieces = p->pieces, elems = (int64_t)C * D4;
    std::vector<float> w;
    GE_CHECK(upload_weights(p, theta, w));
    GE_HIP(hipMemsetAsync(p->dflag, 0, sizeof(int32_t), stream));
    GE_HIP(hipEventRecord(p->ev[0], stream));
    hipLaunchKernelGGL(k_cls_logits, dim3((unsigned)((NT + KL_TQ - 1) / KL_TQ)), dim3(256), 0, stream, (const float *)p->dx, (const int32_t *)p->dmem, NT,
                       (const float *)p->dw, C, D4, p->dz);
    GE_HIP(hipGetLastError());
    GE_HIP(hipEventRecord(p->ev[1], stream));
    hipLaunchKernelGGL(k_cls_softmax, dim3((unsigned)((NT + 63) / 64)), dim3(64), 0, stream, (const float *)p->dz, NT, C, (const int32_t *)p->dy, p->dloss,
                       p->dr, (int32_t *)nullptr, (float *)nullptr, p->dflag);
    GE_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_cls_block_sums, dim3((unsigned)pieces), dim3(64), 0, stream, (const double *)p->dloss, NT, p->dblock);
    GE_HIP(hipGetLastError());
    GE_HIP(hipEventRecord(p->ev[2], stream));
    const int ga = C <= 16 ? 1 : C <= 32 ? 2 : 4;
    const dim3 grid((unsigned)pieces, (unsigned)((C + 16 * ga - 1) / (16 * ga)), (unsigned)((D4 + KG_DT - 1) / KG_DT));
    if (ga == 1)
        hipLaunchKernelGGL(k_cls_gradient<1>, grid, dim3(256), 0, stream, (const float *)p->dx, (const int32_t *)p->dmem, NT, (const float *)p->dr, C, D4, p->dgp);
    else if (ga == 2)
        hipLaunchKernelGGL(k_cls_gradient<2>, grid, dim3(256), 0, stream, (const float *)p->dx, (const int32_t *)p->dmem, NT, (const float *)p->dr, C, D4, p->dgp);
    else
        hipLaunchKernelGGL(k_cls_gradient<4>, grid, dim3(256), 0, stream, (const float *)p->dx, (const int32_t *)p->dmem, NT, (const float *)p->dr, C, D4, p->dgp);
    GE_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_cls_piece_sum, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, stream, (const float *)p->dgp, pieces, elems, p->dg);
    GE_HIP(hipGetLastError());
    GE_HIP(hipEventRecord(p->ev[3], stream));
    int32_t flag = 0;
    std::vector<double> block((size_t)pieces), G((size_t)elems);
    GE_HIP(hipMemcpyAsync(&flag, p->dflag, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    GE_HIP(hipMemcpyAsync(block.data(), p->dblock, sizeof(double) * (size_t)pieces, hipMemcpyDeviceToHost, stream));
    GE_HIP(hipMemcpyAsync(G.data(), p->dg, sizeof(double) * (size_t)elems, hipMemcpyDeviceToHost, stream));
    GE_HIP(hipStreamSynchronize(stream));
    GE_HIP(hipEventElapsedTime(&p->logits_ms, p->ev[0], p->ev[1]));
    GE_HIP(hipEventElapsedTime(&p->softmax_ms, p->ev[1], p->ev[2]));
    GE_HIP(hipEventElapsedTime(&p->gradient_ms, p->ev[2], p->ev[3]));
    *finite = flag == 0;
    if (flag) return GE_OK;
    double L = 0.0;
    for (int64_t b = 0; b < pieces; ++b) L = L + block[(size_t)b];
    double reg = 0.0;
    for (int c = 0; c < C; ++c)
        for (int d = 0; d < p->dim; ++d) {
            const double v = (double)w[(size_t)c * D4 + d];
            reg = reg + v * v;
        }
    const double nt = (double)NT;
    *f = L / nt + (0.5 * p->l2) * reg;
    g.resize((size_t)C * Dp);
    for (int c = 0; c < C; ++c)
        for (int d = 0; d < Dp; ++d) {
            const double m = G[(size_t)c * D4 + d] / nt;
            g[(size_t)c * Dp + d] = d < p->dim ? m + p->l2 * (double)w[(size_t)c * D4 + d] : m;
        }
    return GE_OK;
}

ge_status cls_set_weights(ge_classifier *p, const float *weights) {
    if (!p) return ge::fail(GE_ERR_ARG, "null ge_classifier handle");
    if (!weights) return ge::fail(GE_ERR_ARG, "ge_classify_set_weights: weights is null");
    const size_t count = (size_t)p->classes * (size_t)p->dp;
    for (size_t i = 0; i < count; ++i)
        if (!std::isfinite(weights[i])) return ge::fail(GE_ERR_ARG, "classify: non-finite input (weights)");
    for (size_t i = 0; i < count; ++i) p->theta[i] = (double)weights[i];
    p->H.clear();
    p->have = false; p->loss = 0.0; p->iterations = 0; p->stop = GE_CLS_STOP_NONE; p->evaluations = 0;
    return GE_OK;
}

ge_status cls_eval(ge_classifier *p, double *loss, double *grad) {
    if (!p) return ge::fail(GE_ERR_ARG, "null ge_classifier handle");
    GE_CHECK(ge::select_device(p->device));
    double f = 0.0;
    std::vector<double> g;
    bool finite = true;
    GE_CHECK(evaluate(p, p->theta, &f, g, &finite));
    if (!finite) return ge::fail(GE_ERR_STATE, "classify: non-finite logit");
    if (loss) *loss = f;
    if (grad) std::memcpy(grad, g.data(), sizeof(double) * g.size());
    return GE_OK;
}

ge_status cls_run(ge_classifier *p, int32_t max_iter, int32_t *iterations, int32_t *stop) {
    if (max_iter < 1) return ge::fail(GE_ERR_ARG, "classify: max_iter %d is below 1", max_iter);
    if (!p) return ge::fail(GE_ERR_ARG, "null ge_classifier handle");
    GE_CHECK(ge::select_device(p->device));
    const size_t P = p->theta.size();
    bool finite = true;
    if (!p->have) {
        double f = 0.0;
        std::vector<double> g;
        GE_CHECK(evaluate(p, p->theta, &f, g, &finite));
        if (!finite) return ge::fail(GE_ERR_STATE, "classify: non-finite logit");
        p->evaluations += 1;
        p->loss = f; p->grad = g; p->have = true;
    }
    int32_t ran = 0, why = GE_CLS_STOP_NONE;
    std::vector<double> q(P), d(P), trial(P), gt, a(CLS_HISTORY);
    while (true) {
        double gmax = 0.0;
        for (size_t i = 0; i < P; ++i) gmax = std::max(gmax, std::fabs(p->grad[i]));
        if (gmax <= p->tolerance) { why = GE_CLS_STOP_GRADIENT; break; }
        if (ran >= max_iter) { why = GE_CLS_STOP_MAXITER; break; }
        // the two-loop recursion
        q = p->grad;
        for (int j = (int)p->H.size() - 1; j >= 0; --j) {
            const Pair &h = p->H[(size_t)j];
            a[(size_t)j] = dot(h.s, q) / h.sy;
            for (size_t i = 0; i < P; ++i) q[i] = q[i] - a[(size_t)j] * h.y[i];
        }
        if (!p->H.empty()) {
            const Pair &h = p->H.back();
            const double scale = h.sy / dot(h.y, h.y);
            for (size_t i = 0; i < P; ++i) q[i] = scale * q[i];
        }
        for (size_t j = 0; j < p->H.size(); ++j) {
            const Pair &h = p->H[j];
            const double b = dot(h.y, q) / h.sy;
            const double ab = a[j] - b;
            for (size_t i = 0; i < P; ++i) q[i] = q[i] + ab * h.s[i];
        }
        for (size_t i = 0; i < P; ++i) d[i] = -q[i];
        double dg = dot(d, p->grad);
        if (!(dg < 0.0)) {
            p->H.clear();
            for (size_t i = 0; i < P; ++i) d[i] = -p->grad[i];
            dg = dot(d, p->grad);
        }
        // the line search
        double alpha = !p->H.empty() ? 1.0 : 1.0 / std::max(1.0, std::sqrt(dot(p->grad, p->grad)));
        bool accepted = false;
        double ft = 0.0;
        for (int trialno = 0; trialno < CLS_TRIALS; ++trialno) {
            for (size_t i = 0; i < P; ++i) trial[i] = p->theta[i] + alpha * d[i];
            GE_CHECK(evaluate(p, trial, &ft, gt, &finite));
            p->evaluations += 1;
            if (finite && ft <= p->loss + (1e-4 * alpha) * dg) { accepted = true; break; }
            alpha = 0.5 * alpha;
        }
        if (!accepted) {
            if (!p->H.empty()) { p->H.clear(); continue; }
            why = GE_CLS_STOP_LINESEARCH;
            break;
        }
        Pair pr;
        pr.s.resize(P); pr.y.resize(P);
        for (size_t i = 0; i < P; ++i) { pr.s[i] = trial[i] - p->theta[i]; pr.y[i] = gt[i] - p->grad[i]; }
        pr.sy = dot(pr.s, pr.y);
        if (pr.sy > 1e-10 * dot(pr.y, pr.y)) {
            p->H.push_back(std::move(pr));
            if (p->H.size() > (size_t)CLS_HISTORY) p->H.pop_front();
        }
        p->theta = trial; p->loss = ft; p->grad = gt;
        p->iterations += 1;
        ++ran;
    }
    p->stop = why;
    if (iterations) *iterations = ran;
    if (stop) *stop = why;
    return GE_OK;
}

ge_status cls_predict(ge_classifier *p, int32_t *label, float *prob) {
    if (!p) return ge::fail(GE_ERR_ARG, "null ge_classifier handle");
    GE_CHECK(ge::select_device(p->device));
    hipStream_t stream = p->stream;
    const int32_t C = p->classes, D4 = p->dp4;
    std::vector<float> w;
    GE_CHECK(upload_weights(p, p->theta, w));
    GE_HIP(hipMemsetAsync(p->dflag, 0, sizeof(int32_t), stream));
    for (int64_t begin = 0; begin < p->n; begin += p->zrows) {
        const int64_t rows = std::min(p->zrows, p->n - begin);
        hipLaunchKernelGGL(k_cls_logits, dim3((unsigned)((rows + KL_TQ - 1) / KL_TQ)), dim3(256), 0, stream, (const float *)p->dx + begin * D4,
                           (const int32_t *)nullptr, rows, (const float *)p->dw, C, D4, p->dz);
        GE_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_cls_softmax, dim3((unsigned)((rows + 63) / 64)), dim3(64), 0, stream, (const float *)p->dz, rows, C, (const int32_t *)nullptr,
                           (double *)nullptr, (float *)nullptr, p->dlabel, p->dprob, p->dflag);
        GE_HIP(hipGetLastError());
        if (label) GE_HIP(hipMemcpyAsync(label + begin, p->dlabel, sizeof(int32_t) * (size_t)rows, hipMemcpyDeviceToHost, stream));
        if (prob) GE_HIP(hipMemcpyAsync(prob + begin, p->dprob, sizeof(float) * (size_t)rows, hipMemcpyDeviceToHost, stream));
    }
    int32_t flag = 0;
    GE_HIP(hipMemcpyAsync(&flag, p->dflag, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    GE_HIP(hipStreamSynchronize(stream));
    if (flag) return ge::fail(GE_ERR_STATE, "classify: non-finite logit");
    return GE_OK;
}

ge_status cls_score(ge_classifier *p, const uint8_t *mask, ge_classify_summary *summary, int64_t *confusion) {
    if (!p) return ge::fail(GE_ERR_ARG, "null ge_classifier handle");
    if (!summary) return ge::fail(GE_ERR_ARG, "ge_classify_score: summary is null");
    std::vector<int32_t> pred((size_t)p->n);
    GE_CHECK(cls_predict(p, pred.data(), nullptr));
    const size_t C = (size_t)p->classes;
    std::vector<int64_t> tp(C, 0), fp(C, 0), fn(C, 0);
    if (confusion) std::fill(confusion, confusion + C * C, (int64_t)0);
    int64_t count = 0, correct = 0;
    for (int64_t q = 0; q < p->n; ++q) {
        const int32_t y = p->labels[(size_t)q], z = pred[(size_t)q];
        if (y < 0 || (mask && !mask[q])) continue;
        ++count;
        if (confusion) confusion[(size_t)y * C + (size_t)z] += 1;
        if (y == z) { ++correct; tp[(size_t)y] += 1; }
        else { fn[(size_t)y] += 1; fp[(size_t)z] += 1; }
    }
    double sum = 0.0;
    int64_t seen = 0;
    for (size_t c = 0; c < C; ++c) {
        const int64_t den = 2 * tp[c] + fp[c] + fn[c];
        if (den == 0) continue;
        sum = sum + (double)(2 * tp[c]) / (double)den;
        ++seen;
    }
    summary->count = count;
    summary->correct = correct;
    summary->accuracy = count ? (double)correct / (double)count : 0.0;
    summary->macro_f1 = seen ? sum / (double)seen : 0.0;
    if (summary->tp) std::copy(tp.begin(), tp.end(), summary->tp);
    if (summary->fp) std::copy(fp.begin(), fp.end(), summary->fp);
    if (summary->fn) std::copy(fn.begin(), fn.end(), summary->fn);
    return GE_OK;
}

}  // namespace

extern "C" {

void ge_classify_cfg_default(ge_classify_cfg *cfg) {
    if (!cfg) return;
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->normalize = GE_CLS_COSINE;
    cfg->l2 = 1e-4;
    cfg->tolerance = 1e-4;
}
int32_t ge_classify_cfg_size(void) { return (int32_t)sizeof(ge_classify_cfg); }

ge_status ge_classify_create(const float *rows, int64_t n_rows, int32_t dim, const int32_t *subset, int64_t n_subset, const int32_t *labels,
                             const uint8_t *train, const ge_classify_cfg *cfg, ge_classifier **out) {
    GE_GUARD(cls_create_host(rows, n_rows, dim, subset, n_subset, labels, train, cfg, out));
}
ge_status ge_glove_classify_create(ge_glove *h, const int32_t *subset, int64_t n_subset, const int32_t *labels, const uint8_t *train,
                                   const ge_classify_cfg *cfg, ge_classifier **out) {
    GE_GUARD(cls_create_glove(h, subset, n_subset, labels, train, cfg, out));
}
ge_status ge_classify_set_weights(ge_classifier *p, const float *weights) { GE_GUARD(cls_set_weights(p, weights)); }
ge_status ge_classify_eval(ge_classifier *p, double *loss, double *grad) { GE_GUARD(cls_eval(p, loss, grad)); }
ge_status ge_classify_run(ge_classifier *p, int32_t max_iter, int32_t *iterations, int32_t *stop) { GE_GUARD(cls_run(p, max_iter, iterations, stop)); }
ge_status ge_classify_predict(ge_classifier *p, int32_t *label, float *prob) { GE_GUARD(cls_predict(p, label, prob)); }
ge_status ge_classify_score(ge_classifier *p, const uint8_t *mask, ge_classify_summary *summary, int64_t *confusion) {
    GE_GUARD(cls_score(p, mask, summary, confusion));
}

ge_status ge_classify_get(const ge_classifier *p, int64_t *n, int32_t *dim, int32_t *classes, int64_t *n_train, float *weights, int32_t *iterations,
                          int32_t *stop, double *loss, int64_t *evaluations) {
    if (!p) return ge::fail(GE_ERR_ARG, "null ge_classifier handle");
    if (n) *n = p->n;
    if (dim) *dim = p->dim;
    if (classes) *classes = p->classes;
    if (n_train) *n_train = p->n_t;
    if (weights) for (size_t i = 0; i < p->theta.size(); ++i) weights[i] = (float)p->theta[i];
    if (iterations) *iterations = p->iterations;
    if (stop) *stop = p->stop;
    if (loss) *loss = p->loss;
    if (evaluations) *evaluations = p->evaluations;
    return GE_OK;
}

ge_status ge_classify_last_kernel_ms(const ge_classifier *p, float *logits_ms, float *softmax_ms, float *gradient_ms) {
    if (!p) return ge::fail(GE_ERR_ARG, "null ge_classifier handle");
    if (logits_ms) *logits_ms = p->logits_ms;
    if (softmax_ms) *softmax_ms = p->softmax_ms;
    if (gradient_ms) *gradient_ms = p->gradient_ms;
    return GE_OK;
}

void ge_classify_destroy(ge_classifier *p) {
    if (!p) return;
    (void)hipSetDevice(p->device);
    delete p;
}

}  // extern "C"
