// pca.hip -- PCA of the trained vectors behind the C ABI: moments on the device (k_pca_gram, fp64 matrix cores), the
// eigen-decomposition on the host (Householder tridiagonalisation + implicit QL, fp64), the projection on the device
// (k_pca_project, fp32 matrix cores).  The reference has no counterpart (it parses `pca:` and prints it); the semantics are
// written down in include/geglove.h.
#include "ge_common.h"
#include "ge_glove_internal.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------------------------------------
// Moments.  One pass over the table: the Gram matrix of [x - x0 | 1], x0 = row 0 of the table.  The column of ones makes
// sum(x - x0) the last column of the same product; the shift costs one fp64 subtraction per staged element and takes the
// cancellation out of  S - s s^T / n  (constant input: every entry exactly 0).  Output columns are cut into blocks of 64;
// a workgroup owns one pair of blocks (bi <= bj) and one fixed range of rows, stages panels of GRAM_PANEL rows of both blocks
// through LDS as fp64 (so a panel leaves HBM once per block pair, not once per 16 x 16 tile) and its four waves each
// accumulate a 2 x 2 group of 16 x 16 tiles with v_mfma_f64_16x16x4_f64.  Tiles below the diagonal or beyond the last column
// are skipped per wave.  Rows past the range and columns past dim + 1 are zeros in LDS: the MFMA loop has no per-lane branch.
// The partial blocks of the row ranges are added by k_pca_gram_reduce in a fixed order.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int GRAM_BLOCK = 64;        // output columns per block
constexpr int GRAM_PANEL = 32;        // rows per LDS panel
constexpr int GRAM_STRIDE = 80;       // doubles between panel rows: 160 dwords = 32 mod 64, so the two rows a 32-lane group of
                                      // ds_read_b64 touches fall into different bank halves
constexpr int GRAM_TARGET_WGS = 4096; // workgroups a launch aims at: four rounds of the 4 per CU that fit, so the last round is short
constexpr int64_t SLAB_FLOATS = (int64_t)1 << 26;   // a 256 MB slab of rows per launch (host rows: per upload)

__global__ __launch_bounds__(256) void k_pca_gram(const float *__restrict__ X, const float *__restrict__ shift, int64_t n_rows,
                                                  int32_t D, int64_t chunk_rows, int32_t nb, double *__restrict__ part) {
    __shared__ double sa[GRAM_PANEL * GRAM_STRIDE];
    __shared__ double sb[GRAM_PANEL * GRAM_STRIDE];
    int p = (int)blockIdx.x, bi = 0;
    while (p >= nb - bi) { p -= nb - bi; ++bi; }
    const int bj = bi + p;
    const bool diag = bi == bj;
    const int64_t r0 = (int64_t)blockIdx.y * chunk_rows, r1 = r0 + chunk_rows < n_rows ? r0 + chunk_rows : n_rows;
    const int T = (D + 1 + 15) >> 4;                       // 16-wide tiles that hold a column of [x | 1]
    const int tid = (int)threadIdx.x, lane = tid & 63;
    // which quarter of the block a wave takes rotates with the workgroup: the quarter below the diagonal of a diagonal block is
    // empty, and it must not be the same SIMD's wave that idles in every workgroup of a CU
    const int quarter = (__builtin_amdgcn_readfirstlane(tid >> 6) + (int)blockIdx.x + (int)blockIdx.y) & 3;
    const int wm = quarter >> 1, wn = quarter & 1;
    const int ta0 = bi * 4 + wm * 2, tb0 = bj * 4 + wn * 2;
    const bool act00 = ta0 <= tb0 && tb0 < T, act01 = ta0 <= tb0 + 1 && tb0 + 1 < T;
    const bool act10 = ta0 + 1 <= tb0 && tb0 < T, act11 = ta0 + 1 <= tb0 + 1 && tb0 + 1 < T;

    const int col = tid & 63, rr = tid >> 6;
    const int ca = bi * GRAM_BLOCK + col, cb = bj * GRAM_BLOCK + col;
    const double sha = ca < D ? (double)shift[ca] : 0.0, shb = cb < D ? (double)shift[cb] : 0.0;
    const double onea = ca == D ? 1.0 : 0.0, oneb = cb == D ? 1.0 : 0.0;

    // the next panel's values travel in registers while this panel's products run
    float pa[GRAM_PANEL / 4], pb[GRAM_PANEL / 4];
    auto fetch = [&](int64_t row) {
#pragma unroll
        for (int i = 0; i < GRAM_PANEL / 4; ++i) {
            const int64_t r = row + rr + 4 * i;
            pa[i] = r < r1 && ca < D ? X[r * D + ca] : 0.0f;
            pb[i] = !diag && r < r1 && cb < D ? X[r * D + cb] : 0.0f;
        }
    };
    f64x4 acc00 = {0, 0, 0, 0}, acc01 = {0, 0, 0, 0}, acc10 = {0, 0, 0, 0}, acc11 = {0, 0, 0, 0};
    const double *pbase = diag ? sa : sb;
    const int ka = (lane >> 4) * GRAM_STRIDE + wm * 32 + (lane & 15);
    const int kb = (lane >> 4) * GRAM_STRIDE + wn * 32 + (lane & 15);
    fetch(r0);
    for (int64_t row = r0; row < r1; row += GRAM_PANEL) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < GRAM_PANEL / 4; ++i) {
            const int lr = rr + 4 * i;
            const bool in = row + lr < r1;
            sa[lr * GRAM_STRIDE + col] = in ? (ca < D ? (double)pa[i] - sha : onea) : 0.0;
            if (!diag) sb[lr * GRAM_STRIDE + col] = in ? (cb < D ? (double)pb[i] - shb : oneb) : 0.0;
        }
        __syncthreads();
        if (row + GRAM_PANEL < r1) fetch(row + GRAM_PANEL);
#pragma unroll
        for (int k4 = 0; k4 < GRAM_PANEL; k4 += 4) {
            const double a0 = sa[k4 * GRAM_STRIDE + ka], a1 = sa[k4 * GRAM_STRIDE + ka + 16];
            const double b0 = pbase[k4 * GRAM_STRIDE + kb], b1 = pbase[k4 * GRAM_STRIDE + kb + 16];
            if (act00) acc00 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc00, 0, 0, 0);
            if (act01) acc01 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc01, 0, 0, 0);
            if (act10) acc10 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc10, 0, 0, 0);
            if (act11) acc11 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc11, 0, 0, 0);
        }
    }
    // C/D of the f64 form: column = lane & 15, row = (lane >> 4) + 4 * register.  A workgroup's 64 x 64 block goes out whole.
    double *out = part + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * (GRAM_BLOCK * GRAM_BLOCK);
    const int oc = wn * 32 + (lane & 15), orow = wm * 32 + (lane >> 4);
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        const int a = orow + 4 * reg;
        if (act00) out[a * GRAM_BLOCK + oc] = acc00[reg];
        if (act01) out[a * GRAM_BLOCK + oc + 16] = acc01[reg];
        if (act10) out[(a + 16) * GRAM_BLOCK + oc] = acc10[reg];
        if (act11) out[(a + 16) * GRAM_BLOCK + oc + 16] = acc11[reg];
    }
}

// S (+)= the sum over the row ranges of every entry k_pca_gram computes, in a fixed order: the ranges are cut into eight runs,
// eight threads add one run each in ascending order, and the first adds the eight run sums in ascending order.  A workgroup
// takes 32 consecutive entries of a block pair; S is [TP][TP], TP = 64 nb.
__global__ __launch_bounds__(256) void k_pca_gram_reduce(const double *__restrict__ part, int32_t chunks, int32_t npairs, int32_t nb, int32_t T,
                                                         double *__restrict__ S, int32_t accumulate) {
    constexpr int BB = GRAM_BLOCK * GRAM_BLOCK;
    __shared__ double runs[8][32];
    const int idx = (int)blockIdx.x * 32 + ((int)threadIdx.x & 31), run = (int)threadIdx.x >> 5;
    const int per = (chunks + 7) / 8, c0 = run * per, c1 = c0 + per < chunks ? c0 + per : chunks;
    double s = 0.0;
    for (int c = c0; c < c1; ++c) s += part[(int64_t)c * npairs * BB + idx];
    runs[run][threadIdx.x & 31] = s;
    __syncthreads();
    if (run != 0) return;
    int p = idx / BB, bi = 0;
    const int e = idx - p * BB;
    while (p >= nb - bi) { p -= nb - bi; ++bi; }
    const int a = bi * GRAM_BLOCK + e / GRAM_BLOCK, b = (bi + p) * GRAM_BLOCK + e % GRAM_BLOCK;
    if (!((a >> 4) <= (b >> 4) && (b >> 4) < T)) return;
    const int64_t at = (int64_t)a * (nb * GRAM_BLOCK) + b;
    s = accumulate ? S[at] : 0.0;
#pragma unroll
    for (int r = 0; r < 8; ++r) s += runs[r][threadIdx.x & 31];
    S[at] = s;
}

// ---------------------------------------------------------------------------------------------------------------------
// Projection.  out[r][c] = sum_d (x[r][d] - mean[d]) * W[d][c].  A workgroup keeps the fp32 slab W[:, c0 .. c0 + 16 CT) in LDS
// for its whole life (column groups are the fast grid index: workgroups that read the same rows run together) and walks tiles
// of 64 rows; per 64 values of d the rows are centred in fp64, rounded to fp32 once and
// staged in LDS, and each wave carries its 16 rows through v_mfma_f32_16x16x4_f32: bit for bit an fmaf chain over ascending d.
// W arrives padded with zeros to [D4][KW] (D4 = dim rounded up to 4, KW = k rounded up to 16).
// ---------------------------------------------------------------------------------------------------------------------
constexpr int PROJ_ROWS = 64;
constexpr int PROJ_XS = 66;            // floats between staged rows: 2 mod 32, so 16 rows x 2 columns hit 32 banks
constexpr int PROJ_W_BUDGET = 16128;   // floats of W a workgroup may hold: with the staged rows under 80 KiB, two workgroups per CU
__host__ __device__ constexpr int proj_w_stride(int ct) { return ct == 1 ? 16 : ct <= 3 ? 48 : 80; }   // 16 mod 32: two rows of 16 columns hit 32 banks

template <int CT>
__global__ __launch_bounds__(256) void k_pca_project(const float *__restrict__ X, const double *__restrict__ mean,
                                                     const float *__restrict__ W, int64_t n_rows, int32_t D, int32_t D4, int32_t k,
                                                     int32_t KW, float *__restrict__ out) {
    extern __shared__ float smem[];
    constexpr int WS = proj_w_stride(CT);
    float *ws = smem, *xs = smem + (size_t)D4 * WS;
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c0 = (int)blockIdx.x * CT * 16;
    for (int idx = tid; idx < D4 * CT * 16; idx += 256) {
        const int d = idx / (CT * 16), j = idx - d * (CT * 16);
        ws[d * WS + j] = c0 + j < KW ? W[(int64_t)d * KW + c0 + j] : 0.0f;
    }
    const int col = tid & 63, rr = tid >> 6;
    const int64_t ntiles = (n_rows + PROJ_ROWS - 1) / PROJ_ROWS;
    const int xa = (wave * 16 + (lane & 15)) * PROJ_XS + (lane >> 4);
    const int wb = (lane >> 4) * WS + (lane & 15);
    // the next 64 x 64 piece of the table (and its means) travels in registers while this one's products run
    float px[PROJ_ROWS / 4];
    double pmu = 0.0;
    auto fetch = [&](int64_t tile, int d0) {
        const int d = d0 + col;
        pmu = d < D ? mean[d] : 0.0;
#pragma unroll
        for (int i = 0; i < PROJ_ROWS / 4; ++i) {
            const int64_t r = tile * PROJ_ROWS + rr + 4 * i;
            px[i] = r < n_rows && d < D ? X[r * D + d] : 0.0f;
        }
    };
    int64_t tile = blockIdx.y;
    if (tile < ntiles) fetch(tile, 0);
    for (; tile < ntiles; tile += gridDim.y) {
        const int64_t row0 = tile * PROJ_ROWS;
        f32x4 acc[CT];
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) acc[ct] = f32x4{0, 0, 0, 0};
        for (int d0 = 0; d0 < D4; d0 += 64) {
            __syncthreads();
#pragma unroll
            for (int i = 0; i < PROJ_ROWS / 4; ++i)          // columns past dim: 0 - 0; rows past the table: never stored
                xs[(rr + 4 * i) * PROJ_XS + col] = (float)((double)px[i] - pmu);
            __syncthreads();
            if (d0 + 64 < D4) fetch(tile, d0 + 64);
            else if (tile + gridDim.y < ntiles) fetch(tile + gridDim.y, 0);
            const int dlim = D4 - d0 < 64 ? D4 - d0 : 64;
            for (int dd = 0; dd < dlim; dd += 4) {
                const float a = xs[xa + dd];
#pragma unroll
                for (int ct = 0; ct < CT; ++ct)
                    acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, ws[(d0 + dd) * WS + wb + ct * 16], acc[ct], 0, 0, 0);
            }
        }
        // C/D of the f32 form: column = lane & 15, row = 4 * (lane >> 4) + register
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
            const int c = c0 + ct * 16 + (lane & 15);
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int64_t r = row0 + wave * 16 + (lane >> 4) * 4 + reg;
                if (r < n_rows && c < k) out[r * k + c] = acc[ct][reg];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Host: symmetric eigenproblem.  Householder reduction to tridiagonal form and the implicit QL iteration, as EISPACK's
// tred2 / tql2 state them.  U holds the TRANSPOSE of the working matrix (row c of U = column c), so every inner loop walks
// contiguous memory and row c ends as the eigenvector of d[c].
// ---------------------------------------------------------------------------------------------------------------------
#define V_(a, b) U[(size_t)(b) * n + (size_t)(a)]
void tridiagonalise(int n, std::vector<double> &U, std::vector<double> &d, std::vector<double> &e) {
    for (int j = 0; j < n; ++j) d[j] = V_(n - 1, j);
    for (int i = n - 1; i > 0; --i) {
        double scale = 0.0, h = 0.0;
        for (int k = 0; k < i; ++k) scale += std::fabs(d[k]);
        if (scale == 0.0) {
            e[i] = d[i - 1];
            for (int j = 0; j < i; ++j) { d[j] = V_(i - 1, j); V_(i, j) = 0.0; V_(j, i) = 0.0; }
        } else {
            for (int k = 0; k < i; ++k) { d[k] /= scale; h += d[k] * d[k]; }
            double f = d[i - 1], g = std::sqrt(h);
            if (f > 0) g = -g;
            e[i] = scale * g; h -= f * g; d[i - 1] = f - g;
            for (int j = 0; j < i; ++j) e[j] = 0.0;
            for (int j = 0; j < i; ++j) {
                f = d[j]; V_(j, i) = f; g = e[j] + V_(j, j) * f;
                const double *colj = &V_(0, j);
                for (int k = j + 1; k <= i - 1; ++k) { g += colj[k] * d[k]; e[k] += colj[k] * f; }
                e[j] = g;
            }
            f = 0.0;
            for (int j = 0; j < i; ++j) { e[j] /= h; f += e[j] * d[j]; }
            const double hh = f / (h + h);
            for (int j = 0; j < i; ++j) e[j] -= hh * d[j];
            for (int j = 0; j < i; ++j) {
                f = d[j]; g = e[j];
                double *colj = &V_(0, j);
                for (int k = j; k <= i - 1; ++k) colj[k] -= f * e[k] + g * d[k];
                d[j] = V_(i - 1, j); V_(i, j) = 0.0;
            }
        }
        d[i] = h;
    }
    for (int i = 0; i < n - 1; ++i) {                       // accumulate the transformations
        V_(n - 1, i) = V_(i, i); V_(i, i) = 1.0;
        const double h = d[i + 1];
        if (h != 0.0) {
            const double *ci = &V_(0, i + 1);
            for (int k = 0; k <= i; ++k) d[k] = ci[k] / h;
            for (int j = 0; j <= i; ++j) {
                double g = 0.0;
                double *colj = &V_(0, j);
                for (int k = 0; k <= i; ++k) g += ci[k] * colj[k];
                for (int k = 0; k <= i; ++k) colj[k] -= g * d[k];
            }
        }
        for (int k = 0; k <= i; ++k) V_(k, i + 1) = 0.0;
    }
    for (int j = 0; j < n; ++j) { d[j] = V_(n - 1, j); V_(n - 1, j) = 0.0; }
    V_(n - 1, n - 1) = 1.0;
    e[0] = 0.0;
}

bool implicit_ql(int n, std::vector<double> &U, std::vector<double> &d, std::vector<double> &e) {
    for (int i = 1; i < n; ++i) e[i - 1] = e[i];
    e[n - 1] = 0.0;
    double f = 0.0, tst1 = 0.0;
    const double eps = std::ldexp(1.0, -52);
    for (int l = 0; l < n; ++l) {
        tst1 = std::max(tst1, std::fabs(d[l]) + std::fabs(e[l]));
        int m = l;
        while (m < n - 1 && std::fabs(e[m]) > eps * tst1) ++m;
        if (m > l) {
            int iter = 0;
            do {
                if (++iter > 60) return false;
                double g = d[l], p = (d[l + 1] - g) / (2.0 * e[l]), r = std::hypot(p, 1.0);
                if (p < 0) r = -r;
                d[l] = e[l] / (p + r); d[l + 1] = e[l] * (p + r);
                const double dl1 = d[l + 1];
                double h = g - d[l];
                for (int i = l + 2; i < n; ++i) d[i] -= h;
                f += h;
                p = d[m];
                double c = 1.0, c2 = c, c3 = c, s = 0.0, s2 = 0.0;
                const double el1 = e[l + 1];
                for (int i = m - 1; i >= l; --i) {
                    c3 = c2; c2 = c; s2 = s;
                    g = c * e[i]; h = c * p; r = std::hypot(p, e[i]);
                    e[i + 1] = s * r; s = e[i] / r; c = p / r; p = c * d[i] - s * g;
                    d[i + 1] = h + s * (c * g + s * d[i]);
                    double *v0 = &U[(size_t)i * n], *v1 = &U[(size_t)(i + 1) * n];
                    for (int k = 0; k < n; ++k) { const double t = v1[k]; v1[k] = s * v0[k] + c * t; v0[k] = c * v0[k] - s * t; }
                }
                p = -s * s2 * c3 * el1 * e[l] / dl1;
                e[l] = s * p; d[l] = c * p;
            } while (std::fabs(e[l]) > eps * tst1);
        }
        d[l] += f; e[l] = 0.0;
    }
    return true;
}
#undef V_

}  // namespace

struct ge_pca {
    int32_t dim = 0, k = 0, device = 0;
    int64_t n_rows = 0;
    hipStream_t stream = nullptr;
    std::vector<double> mean, cov, eigenvalues, components;
    mutable float fit_ms = 0, transform_ms = 0;
};

namespace {

ge_status check_cfg(const ge_pca_cfg *cfg, int64_t n_rows, int32_t dim) {
    if (!cfg) return ge::fail(GE_ERR_ARG, "ge_pca_cfg is null");
    if (dim < 1 || dim > 1024) return ge::fail(GE_ERR_ARG, "pca: dim %d outside [1, 1024]", dim);
    if (n_rows < 2) return ge::fail(GE_ERR_ARG, "pca: %lld rows, need at least 2", (long long)n_rows);
    if (!(cfg->variance > 0.0 && cfg->variance <= 1.0)) return ge::fail(GE_ERR_ARG, "pca: variance %g outside (0, 1]", cfg->variance);
    if (cfg->max_components < 0) return ge::fail(GE_ERR_ARG, "pca: max_components %d is negative", cfg->max_components);
    return GE_OK;
}

// The model from finite moments (mean[dim], cov[dim*dim]); validated arguments.
ge_status build_model(const double *mean, const double *cov, int32_t dim, int64_t n_rows, const ge_pca_cfg *cfg, ge_pca **out) {
    const int n = dim;
    for (int i = 0; i < n; ++i) if (!std::isfinite(mean[i])) return ge::fail(GE_ERR_ARG, "pca: non-finite input (mean[%d])", i);
    for (size_t i = 0; i < (size_t)n * n; ++i) if (!std::isfinite(cov[i])) return ge::fail(GE_ERR_ARG, "pca: non-finite input (covariance)");
    std::unique_ptr<ge_pca> p(new ge_pca);
    p->dim = dim; p->n_rows = n_rows; p->device = cfg->device; p->stream = (hipStream_t)cfg->stream;
    p->mean.assign(mean, mean + n);
    p->cov.assign(cov, cov + (size_t)n * n);
    std::vector<double> U((size_t)n * n), d((size_t)n), e((size_t)n);
    for (int a = 0; a < n; ++a)
        for (int b = 0; b < n; ++b) U[(size_t)a * n + b] = 0.5 * (cov[(size_t)a * n + b] + cov[(size_t)b * n + a]);
    tridiagonalise(n, U, d, e);
    if (!implicit_ql(n, U, d, e)) return ge::fail(GE_ERR_STATE, "pca: the QL iteration did not converge");
    std::vector<int> order((size_t)n);
    for (int i = 0; i < n; ++i) order[(size_t)i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return d[(size_t)x] > d[(size_t)y]; });
    p->eigenvalues.resize((size_t)n);
    p->components.resize((size_t)n * n);
    for (int c = 0; c < n; ++c) {
        const double *v = &U[(size_t)order[(size_t)c] * n];
        p->eigenvalues[(size_t)c] = std::max(d[(size_t)order[(size_t)c]], 0.0);
        int big = 0;
        for (int i = 1; i < n; ++i) if (std::fabs(v[i]) > std::fabs(v[big])) big = i;
        const double sign = v[big] < 0 ? -1.0 : 1.0;
        for (int i = 0; i < n; ++i) p->components[(size_t)i * n + c] = sign * v[i];
    }
    double total = 0.0;
    for (int c = 0; c < n; ++c) total += p->eigenvalues[(size_t)c];
    int k = 1;
    if (total > 0.0) {
        const double need = cfg->variance * total;
        double cum = 0.0;
        k = n;
        for (int c = 0; c < n; ++c) { cum += p->eigenvalues[(size_t)c]; if (cum >= need) { k = c + 1; break; } }
    }
    if (cfg->max_components > 0) k = std::min(k, cfg->max_components);
    p->k = k;
    *out = p.release();
    return GE_OK;
}

struct DeviceBuffers {                      // freed on every way out
    std::vector<void *> ptrs;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~DeviceBuffers() { for (void *q : ptrs) (void)hipFree(q); if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
    ge_status alloc(void **q, size_t bytes) { GE_HIP(hipMalloc(q, std::max<size_t>(bytes, 16))); ptrs.push_back(*q); return GE_OK; }
    ge_status events() { GE_HIP(hipEventCreate(&e0)); GE_HIP(hipEventCreate(&e1)); return GE_OK; }
};

int64_t slab_rows_of(int32_t dim) { return std::max<int64_t>(GRAM_PANEL, SLAB_FLOATS / dim / GRAM_PANEL * GRAM_PANEL); }

// Moments of n_rows x dim floats: `host` rows go up slab by slab, `dev` rows are read in place -- the same slabs, the same
// row ranges, the same order of additions either way.
ge_status fit_impl(const float *host, const float *dev, int64_t n_rows, int32_t dim, const ge_pca_cfg *cfg, ge_pca **out) {
    hipStream_t stream = (hipStream_t)cfg->stream;
    const int D = dim, nb = (D + 1 + GRAM_BLOCK - 1) / GRAM_BLOCK, TP = nb * GRAM_BLOCK, T = (D + 1 + 15) / 16;
    const int npairs = nb * (nb + 1) / 2;
    const int64_t slab_rows = std::min(slab_rows_of(dim), n_rows);
    auto chunks_of = [&](int64_t rows) {
        const int64_t panels = (rows + GRAM_PANEL - 1) / GRAM_PANEL;
        return std::max<int64_t>(1, std::min<int64_t>(panels, (GRAM_TARGET_WGS + npairs - 1) / npairs));
    };
    DeviceBuffers B;
    float *dslab = nullptr, *dshift = nullptr;
    double *dpart = nullptr, *dS = nullptr;
    ge_status st = B.events();
    if (st == GE_OK && host) st = B.alloc((void **)&dslab, sizeof(float) * (size_t)slab_rows * D);
    if (st == GE_OK) st = B.alloc((void **)&dshift, sizeof(float) * (size_t)D);
    if (st == GE_OK) st = B.alloc((void **)&dpart, sizeof(double) * (size_t)chunks_of(slab_rows) * npairs * GRAM_BLOCK * GRAM_BLOCK);
    if (st == GE_OK) st = B.alloc((void **)&dS, sizeof(double) * (size_t)TP * TP);
    if (st != GE_OK) return st;
    GE_HIP(hipMemcpyAsync(dshift, host ? host : dev, sizeof(float) * (size_t)D, host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, stream));
    float total_ms = 0;
    for (int64_t begin = 0, slab = 0; begin < n_rows; begin += slab_rows, ++slab) {
        const int64_t rows = std::min(slab_rows, n_rows - begin);
        const float *x = dev ? dev + begin * D : dslab;
        if (host) GE_HIP(hipMemcpyAsync(dslab, host + begin * D, sizeof(float) * (size_t)rows * D, hipMemcpyHostToDevice, stream));
        const int64_t chunks = chunks_of(rows);
        const int64_t chunk_rows = ((rows + chunks - 1) / chunks + GRAM_PANEL - 1) / GRAM_PANEL * GRAM_PANEL;
        const int64_t used = (rows + chunk_rows - 1) / chunk_rows;                 // every range holds at least one row
        GE_HIP(hipEventRecord(B.e0, stream));
        hipLaunchKernelGGL(k_pca_gram, dim3((unsigned)npairs, (unsigned)used), dim3(256), 0, stream, x, dshift, rows, D, chunk_rows, nb, dpart);
        hipLaunchKernelGGL(k_pca_gram_reduce, dim3((unsigned)(npairs * GRAM_BLOCK * GRAM_BLOCK / 32)), dim3(256), 0, stream, dpart, (int32_t)used,
                           npairs, nb, T, dS, slab > 0 ? 1 : 0);
        GE_HIP(hipGetLastError());
        GE_HIP(hipEventRecord(B.e1, stream));
        GE_HIP(hipStreamSynchronize(stream));                                       // the slab buffer is free again
        float ms = 0;
        GE_HIP(hipEventElapsedTime(&ms, B.e0, B.e1));
        total_ms += ms;
    }
    std::vector<double> S((size_t)TP * TP);
    std::vector<float> x0((size_t)D);
    GE_HIP(hipMemcpyAsync(S.data(), dS, sizeof(double) * S.size(), hipMemcpyDeviceToHost, stream));
    GE_HIP(hipMemcpyAsync(x0.data(), dshift, sizeof(float) * (size_t)D, hipMemcpyDeviceToHost, stream));
    GE_HIP(hipStreamSynchronize(stream));
    // S = Gram of [x - x0 | 1]:  S[a][D] = sum (x_a - x0_a),  S[D][D] = n
    const double n = (double)n_rows;
    std::vector<double> mean((size_t)D), cov((size_t)D * D);
    auto s_at = [&](int a, int b) { return S[(size_t)a * TP + b]; };
    for (int a = 0; a < D; ++a) mean[(size_t)a] = (double)x0[(size_t)a] + s_at(a, D) / n;
    for (int a = 0; a < D; ++a)
        for (int b = a; b < D; ++b) {
            const double c = (s_at(a, b) - s_at(a, D) * s_at(b, D) / n) / (n - 1.0);
            cov[(size_t)a * D + b] = c; cov[(size_t)b * D + a] = c;
        }
    st = build_model(mean.data(), cov.data(), dim, n_rows, cfg, out);
    if (st == GE_OK) (*out)->fit_ms = total_ms;
    return st;
}

template <int CT>
ge_status launch_project(const float *x, const double *dmean, const float *dW, int64_t rows, int D, int D4, int k, int KW, float *dout,
                         hipStream_t stream) {
    const size_t lds = sizeof(float) * ((size_t)D4 * proj_w_stride(CT) + (size_t)PROJ_ROWS * PROJ_XS);
    GE_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_pca_project<CT>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int64_t ntiles = (rows + PROJ_ROWS - 1) / PROJ_ROWS;
    const int groups = (KW / 16 + CT - 1) / CT;
    hipLaunchKernelGGL(k_pca_project<CT>, dim3((unsigned)groups, (unsigned)std::min<int64_t>(ntiles, 512)), dim3(256), lds, stream, x, dmean, dW,
                       rows, D, D4, k, KW, dout);
    GE_HIP(hipGetLastError());
    return GE_OK;
}

ge_status transform_impl(const ge_pca *p, const float *host, const float *dev, int64_t n_rows, float *out) {
    hipStream_t stream = p->stream;
    const int D = p->dim, k = p->k, D4 = (D + 3) / 4 * 4, KW = (k + 15) / 16 * 16;
    int CT = 1;                                              // the widest slab of W that fits and is needed
    for (int ct : {2, 3, 4}) if (D4 * proj_w_stride(ct) <= PROJ_W_BUDGET && ct <= KW / 16) CT = ct;
    std::vector<float> W((size_t)D4 * KW, 0.0f);
    for (int d = 0; d < D; ++d)
        for (int c = 0; c < k; ++c) W[(size_t)d * KW + c] = (float)p->components[(size_t)d * D + c];
    const int64_t slab_rows = std::min(slab_rows_of(D), n_rows);
    DeviceBuffers B;
    float *dslab = nullptr, *dW = nullptr, *dout = nullptr;
    double *dmean = nullptr;
    ge_status st = B.events();
    if (st == GE_OK && host) st = B.alloc((void **)&dslab, sizeof(float) * (size_t)slab_rows * D);
    if (st == GE_OK) st = B.alloc((void **)&dW, sizeof(float) * W.size());
    if (st == GE_OK) st = B.alloc((void **)&dmean, sizeof(double) * (size_t)D);
    if (st == GE_OK) st = B.alloc((void **)&dout, sizeof(float) * (size_t)slab_rows * k);
    if (st != GE_OK) return st;
    GE_HIP(hipMemcpyAsync(dW, W.data(), sizeof(float) * W.size(), hipMemcpyHostToDevice, stream));
    GE_HIP(hipMemcpyAsync(dmean, p->mean.data(), sizeof(double) * (size_t)D, hipMemcpyHostToDevice, stream));
    float total_ms = 0;
    for (int64_t begin = 0; begin < n_rows; begin += slab_rows) {
        const int64_t rows = std::min(slab_rows, n_rows - begin);
        const float *x = dev ? dev + begin * D : dslab;
        if (host) GE_HIP(hipMemcpyAsync(dslab, host + begin * D, sizeof(float) * (size_t)rows * D, hipMemcpyHostToDevice, stream));
        GE_HIP(hipEventRecord(B.e0, stream));
        st = CT == 4 ? launch_project<4>(x, dmean, dW, rows, D, D4, k, KW, dout, stream)
           : CT == 3 ? launch_project<3>(x, dmean, dW, rows, D, D4, k, KW, dout, stream)
           : CT == 2 ? launch_project<2>(x, dmean, dW, rows, D, D4, k, KW, dout, stream)
                     : launch_project<1>(x, dmean, dW, rows, D, D4, k, KW, dout, stream);
        if (st != GE_OK) return st;
        GE_HIP(hipEventRecord(B.e1, stream));
        GE_HIP(hipMemcpyAsync(out + begin * k, dout, sizeof(float) * (size_t)rows * k, hipMemcpyDeviceToHost, stream));
        GE_HIP(hipStreamSynchronize(stream));
        float ms = 0;
        GE_HIP(hipEventElapsedTime(&ms, B.e0, B.e1));
        total_ms += ms;
    }
    p->transform_ms = total_ms;
    return GE_OK;
}

ge_status pca_fit_host(const float *rows, int64_t n_rows, int32_t dim, const ge_pca_cfg *cfg, ge_pca **out) {
    if (out) *out = nullptr;
    if (!rows || !out) return ge::fail(GE_ERR_ARG, "ge_pca_fit: rows or out is null");
    ge_status st = check_cfg(cfg, n_rows, dim);
    if (st == GE_OK) st = ge::select_device(cfg->device);
    if (st != GE_OK) return st;
    return fit_impl(rows, nullptr, n_rows, dim, cfg, out);
}

ge_status pca_fit_glove(ge_glove *h, const ge_pca_cfg *cfg, ge_pca **out) {
    if (out) *out = nullptr;
    if (!h || !out) return ge::fail(GE_ERR_ARG, "ge_glove_pca_fit: handle or out is null");
    if (!cfg) return ge::fail(GE_ERR_ARG, "ge_pca_cfg is null");
    float *d = nullptr;
    int32_t V = 0, D = 0, device = 0;
    ge_status st = ge::glove_extract_device_f32(h, &d, &V, &D, &device);
    if (st != GE_OK) return st;
    ge_pca_cfg own = *cfg;
    own.device = device;                                    // the rows live on the handle's device
    st = check_cfg(&own, V, D);
    if (st == GE_OK) st = fit_impl(nullptr, d, V, D, &own, out);
    (void)hipFree(d);
    return st;
}

ge_status pca_from_moments(const double *mean, const double *cov, int32_t dim, int64_t n_rows, const ge_pca_cfg *cfg, ge_pca **out) {
    if (out) *out = nullptr;
    if (!mean || !cov || !out) return ge::fail(GE_ERR_ARG, "ge_pca_from_moments: mean, cov or out is null");
    ge_status st = check_cfg(cfg, n_rows, dim);
    if (st != GE_OK) return st;
    return build_model(mean, cov, dim, n_rows, cfg, out);
}

ge_status pca_transform_host(const ge_pca *p, const float *rows, int64_t n_rows, float *out) {
    if (!p || !rows || !out) return ge::fail(GE_ERR_ARG, "ge_pca_transform: model, rows or out is null");
    if (n_rows < 1) return ge::fail(GE_ERR_ARG, "ge_pca_transform: %lld rows", (long long)n_rows);
    ge_status st = ge::select_device(p->device);
    if (st != GE_OK) return st;
    return transform_impl(p, rows, nullptr, n_rows, out);
}

ge_status pca_transform_glove(const ge_pca *p, ge_glove *h, float *out) {
    if (!p || !h || !out) return ge::fail(GE_ERR_ARG, "ge_glove_pca_transform: model, handle or out is null");
    float *d = nullptr;
    int32_t V = 0, D = 0, device = 0;
    ge_status st = ge::glove_extract_device_f32(h, &d, &V, &D, &device);
    if (st != GE_OK) return st;
    if (D != p->dim) st = ge::fail(GE_ERR_ARG, "ge_glove_pca_transform: the model has dim %d, the handle %d", p->dim, D);
    else if (device != p->device) st = ge::fail(GE_ERR_ARG, "ge_glove_pca_transform: the model is for device %d, the handle on %d", p->device, device);
    else st = transform_impl(p, nullptr, d, V, out);
    (void)hipFree(d);
    return st;
}

}  // namespace

extern "C" {

void ge_pca_cfg_default(ge_pca_cfg *cfg) {
    if (!cfg) return;
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->variance = 0.95;
}
int32_t ge_pca_cfg_size(void) { return (int32_t)sizeof(ge_pca_cfg); }

ge_status ge_pca_fit(const float *rows, int64_t n_rows, int32_t dim, const ge_pca_cfg *cfg, ge_pca **out) {
    GE_GUARD(pca_fit_host(rows, n_rows, dim, cfg, out));
}
ge_status ge_glove_pca_fit(ge_glove *h, const ge_pca_cfg *cfg, ge_pca **out) { GE_GUARD(pca_fit_glove(h, cfg, out)); }
ge_status ge_pca_from_moments(const double *mean, const double *cov, int32_t dim, int64_t n_rows, const ge_pca_cfg *cfg, ge_pca **out) {
    GE_GUARD(pca_from_moments(mean, cov, dim, n_rows, cfg, out));
}

ge_status ge_pca_get(const ge_pca *p, int32_t *dim, int32_t *k, int64_t *n_rows, const double **mean, const double **cov,
                     const double **eigenvalues, const double **components) {
    if (!p) return ge::fail(GE_ERR_ARG, "null ge_pca handle");
    if (dim) *dim = p->dim;
    if (k) *k = p->k;
    if (n_rows) *n_rows = p->n_rows;
    if (mean) *mean = p->mean.data();
    if (cov) *cov = p->cov.data();
    if (eigenvalues) *eigenvalues = p->eigenvalues.data();
    if (components) *components = p->components.data();
    return GE_OK;
}

ge_status ge_pca_transform(const ge_pca *p, const float *rows, int64_t n_rows, float *out) { GE_GUARD(pca_transform_host(p, rows, n_rows, out)); }
ge_status ge_glove_pca_transform(const ge_pca *p, ge_glove *h, float *out) { GE_GUARD(pca_transform_glove(p, h, out)); }

ge_status ge_pca_last_kernel_ms(const ge_pca *p, float *fit_ms, float *transform_ms) {
    if (!p) return ge::fail(GE_ERR_ARG, "null ge_pca handle");
    if (fit_ms) *fit_ms = p->fit_ms;
    if (transform_ms) *transform_ms = p->transform_ms;
    return GE_OK;
}

void ge_pca_destroy(ge_pca *p) { delete p; }

}  // extern "C"
