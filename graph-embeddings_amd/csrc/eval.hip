// eval.hip -- the cost of nonzeros a trainer never saw: ge_glove_eval_* (include/geglove.h, "Held-out evaluation") and the
// host-only split rule ge_holdout_mask.  A pure read of a trainer handle in whichever layout it has (ge_glove_internal.h
// EvalView): exact_update's arithmetic (ge_exact.h) stopped before the update.  Compile with -ffp-contract=off.
#include "ge_common.h"
#include "ge_cost.h"
#include "ge_glove_internal.h"
#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

namespace {

constexpr int EV_TILE = 64;        // nonzeros of one wavefront-sized workgroup: lane r owns nonzero r's sum
constexpr int EV_PIECE = 32;       // columns multiplied per pass
constexpr int EV_LD = 33;          // panel row stride in floats: lane r walking row r, and 8 (2) rows written side by side, hit 32 banks
constexpr int EV_SUM_BLOCK = 1024; // the fixed partition of cost_sum

struct EvalParams {
    const void *focus, *context;            // row tables: fp32, or bf16 (BF16 instances)
    const float *fbias, *cbias, *hub32;
    const int32_t *hub_index;               // BF16: column -> row of hub32 (fp32 master), < 0 = none; null = no masters
    int64_t fs, cs, fbs, cbs;               // strides in elements
    const int32_t *I, *J, *order;           // the set as the kernel walks it; order[k] = the caller's index (null: identity)
    const float *X;
    float *residual; double *term;          // in the caller's order
    double xmax;
    int64_t n;
    int32_t D, row_begin, cost_kind;
};

template <int VW> struct RowVec;
template <> struct RowVec<4> { float v[4]; };
template <> struct RowVec<1> { float v[1]; };

__device__ __forceinline__ float widen(uint32_t bits16) { return __uint_as_float(bits16 << 16); }

// columns [c, c + VW) of the row that starts `off` elements into `table`; is16: the table holds bf16, widened exactly.  The tables
// are kernel arguments and the rows are offsets into them, so these stay global loads (a row pointer kept in LDS would be a
// generic one, and its loads flat).
template <int VW>
__device__ __forceinline__ RowVec<VW> load_row(const void *table, int64_t off, int c, bool is16) {
    RowVec<VW> r;
    if constexpr (VW == 4) {
        if (is16) {
            const uint2 u = *reinterpret_cast<const uint2 *>(static_cast<const uint16_t *>(table) + off + c);
            r.v[0] = widen(u.x & 0xFFFFu); r.v[1] = widen(u.x >> 16); r.v[2] = widen(u.y & 0xFFFFu); r.v[3] = widen(u.y >> 16);
        } else {
            const float4 f = *reinterpret_cast<const float4 *>(static_cast<const float *>(table) + off + c);
            r.v[0] = f.x; r.v[1] = f.y; r.v[2] = f.z; r.v[3] = f.w;
        }
    } else {
        r.v[0] = is16 ? widen(static_cast<const uint16_t *>(table)[off + c]) : static_cast<const float *>(table)[off + c];
    }
    return r;
}

// One wavefront-sized workgroup owns 64 nonzeros.  Per piece of 32 columns the two rows of every nonzero are read coalesced
// (VW = 4: eight lanes per row, 16 bytes each -- 8 for bf16 --, eight nonzeros per instruction; VW = 1: a dword per lane, two
// nonzeros per instruction), the fp32 products go to the LDS panel [nonzero][33], and lane r adds nonzero r's piece in ascending d,
// carrying its partial sum over the pieces: 64 sequential sums side by side.
template <int VW, bool BF16>
__global__ __launch_bounds__(EV_TILE) void k_eval_terms(EvalParams p) {
    __shared__ float s_prod[EV_TILE * EV_LD];
    __shared__ int64_t s_foff[EV_TILE];              // where nonzero r's rows start, in elements of their tables
    __shared__ int64_t s_coff[EV_TILE];
    __shared__ int32_t s_c16[BF16 ? EV_TILE : 1];    // BF16: the context row is a bf16 row of `context` (1) or an fp32 master of `hub32` (0)
    const int lane = threadIdx.x;
    const int64_t k0 = (int64_t)blockIdx.x * EV_TILE;
    const int64_t k = (k0 + lane < p.n) ? k0 + lane : p.n - 1;       // the lanes past the end repeat the last nonzero and write nothing
    const int32_t i = p.I[k], j = p.J[k];
    const int64_t fr = (int64_t)i - p.row_begin;
    s_foff[lane] = fr * p.fs;
    if (BF16) {
        const int32_t slot = p.hub_index ? p.hub_index[j] : -1;
        s_coff[lane] = slot >= 0 ? (int64_t)slot * p.D : (int64_t)j * p.cs;
        s_c16[lane] = slot < 0;
    } else {
        s_coff[lane] = (int64_t)j * p.cs;
    }
    __syncthreads();

    constexpr int LPR = EV_PIECE / VW;       // lanes that share a row piece
    constexpr int RPI = EV_TILE / LPR;       // rows per load instruction
    constexpr int UNR = 8;                   // loads in flight per side
    const int sub = lane / LPR, col = (lane % LPR) * VW;
    const float *mine = s_prod + lane * EV_LD;
    float s = 0.0f;
    for (int c0 = 0; c0 < p.D; c0 += EV_PIECE) {
        const int c = c0 + col;
        if (c < p.D) {                        // VW = 4 only with D % 4 == 0: the whole vector lies inside the row
            for (int r0 = 0; r0 < EV_TILE; r0 += RPI * UNR) {
                RowVec<VW> f[UNR], g[UNR];
                if constexpr (BF16 && VW == 4) {
                    // A context row is 4 bf16 (8 bytes) or 4 floats of a master (16): the first 8 bytes of either come from one load
                    // and the rest from a second one only masters issue; nothing is converted before every load is out, so the
                    // two kinds of row do not wait for each other.
                    uint2 lo[UNR], hi[UNR];
                    bool c16[UNR];
#pragma unroll
                    for (int u = 0; u < UNR; ++u) {
                        const int r = r0 + u * RPI + sub;
                        c16[u] = s_c16[r] != 0;
                        f[u] = load_row<VW>(p.focus, s_foff[r], c, true);
                        const char *at = c16[u] ? reinterpret_cast<const char *>(static_cast<const uint16_t *>(p.context) + s_coff[r] + c)
                                                : reinterpret_cast<const char *>(p.hub32 + s_coff[r] + c);
                        lo[u] = *reinterpret_cast<const uint2 *>(at);
                        hi[u] = make_uint2(0u, 0u);
                        if (!c16[u]) hi[u] = *reinterpret_cast<const uint2 *>(at + 8);
                    }
#pragma unroll
                    for (int u = 0; u < UNR; ++u) {
                        g[u].v[0] = c16[u] ? widen(lo[u].x & 0xFFFFu) : __uint_as_float(lo[u].x);
                        g[u].v[1] = c16[u] ? widen(lo[u].x >> 16) : __uint_as_float(lo[u].y);
                        g[u].v[2] = c16[u] ? widen(lo[u].y & 0xFFFFu) : __uint_as_float(hi[u].x);
                        g[u].v[3] = c16[u] ? widen(lo[u].y >> 16) : __uint_as_float(hi[u].y);
                    }
                } else {
#pragma unroll
                    for (int u = 0; u < UNR; ++u) {
                        const int r = r0 + u * RPI + sub;
                        const bool c16 = BF16 && s_c16[r];
                        f[u] = load_row<VW>(p.focus, s_foff[r], c, BF16);
                        g[u] = load_row<VW>((!BF16 || c16) ? p.context : static_cast<const void *>(p.hub32), s_coff[r], c, c16);
                    }
                }
#pragma unroll
                for (int u = 0; u < UNR; ++u) {
                    float *dst = s_prod + (r0 + u * RPI + sub) * EV_LD + col;
#pragma unroll
                    for (int e = 0; e < VW; ++e) dst[e] = f[u].v[e] * g[u].v[e];
                }
            }
        }
        __syncthreads();
        if (p.D - c0 >= EV_PIECE) {           // a whole piece: the 32 reads go out together, the adds follow in order
            float v[EV_PIECE];
#pragma unroll
            for (int d = 0; d < EV_PIECE; ++d) v[d] = mine[d];
#pragma unroll
            for (int d = 0; d < EV_PIECE; ++d) s = s + v[d];
        } else {
            for (int d = 0; d < p.D - c0; ++d) s = s + mine[d];
        }
        __syncthreads();
    }

    double l; float w;
    cost_terms<true>(p.cost_kind, p.X[k], p.xmax, l, w);
    const float fb = p.fbias[fr * p.fbs], cb = p.cbias[(int64_t)j * p.cbs];
    const float ic = (float)((double)s + ((double)(fb + cb) - l));
    const float wc = w * ic;
    const double t = (0.5 * (double)wc) * (double)ic;
    if (k0 + lane < p.n) {
        const int64_t o = p.order ? (int64_t)p.order[k] : k;
        p.residual[o] = ic;
        p.term[o] = t;
    }
}

// S_b: the terms of [1024 b, 1024 (b + 1)) added in ascending k by one lane, from LDS
__global__ __launch_bounds__(64) void k_eval_block_sums(const double *term, int64_t n, double *sums) {
    __shared__ double s_t[EV_SUM_BLOCK];
    const int64_t b0 = (int64_t)blockIdx.x * EV_SUM_BLOCK;
    const int cnt = (int)((n - b0 < EV_SUM_BLOCK) ? n - b0 : EV_SUM_BLOCK);
    for (int q = threadIdx.x; q < cnt; q += 64) s_t[q] = term[b0 + q];
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0;
        for (int q = 0; q < cnt; ++q) a = a + s_t[q];
        sums[blockIdx.x] = a;
    }
}

// the (n+1)-th output of SplitMix64 seeded with `seed` (geglove.h: SM)
inline uint64_t splitmix_at(uint64_t seed, uint64_t n) {
    uint64_t z = seed + (n + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

bool aligned_to(const void *p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

struct ge_eval {
    ge_glove *glove = nullptr;
    ge::EvalView view{};
    int64_t n = 0, n_blocks = 0;
    bool sorted = false;                 // the set was reordered by focus row (order != null)
    int32_t *dI = nullptr, *dJ = nullptr, *dorder = nullptr;
    float *dX = nullptr, *dres = nullptr;
    double *dterm = nullptr, *dsums = nullptr;
    std::vector<double> sums;            // S_b on the host: the total is their sum in ascending b
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    float last_ms = 0.0f;
};

namespace {

void eval_free(ge_eval *e) {
    if (!e) return;
    (void)hipSetDevice(e->view.device);
    for (void *q : {(void *)e->dI, (void *)e->dJ, (void *)e->dorder, (void *)e->dX, (void *)e->dres, (void *)e->dterm, (void *)e->dsums})
        if (q) (void)hipFree(q);
    if (e->ev0) (void)hipEventDestroy(e->ev0);
    if (e->ev1) (void)hipEventDestroy(e->ev1);
    delete e;
}

ge_status eval_create_impl(ge_glove *h, const int32_t *I, const int32_t *J, const float *X, int64_t n, ge_eval **out) {
    if (!out) return ge::fail(GE_ERR_ARG, "out is null");
    *out = nullptr;
    if (!h) return ge::fail(GE_ERR_ARG, "null ge_glove handle");
    if (!I || !J || !X) return ge::fail(GE_ERR_ARG, "null evaluation arrays");
    if (n < 1 || n >= ((int64_t)1 << 31)) return ge::fail(GE_ERR_ARG, "an evaluation set holds 1 <= n < 2^31 nonzeros, got %lld", (long long)n);
    ge::EvalView v;
    GE_CHECK(ge::glove_eval_view(h, &v));
    bool ascending = true;
    for (int64_t k = 0; k < n; ++k) {
        if (I[k] < v.row_begin || I[k] >= v.row_end)
            return ge::fail(GE_ERR_ARG, "nonzero %lld: focus row %d outside the handle's rows [%d,%d)", (long long)k, I[k], v.row_begin, v.row_end);
        if (J[k] < 0 || J[k] >= v.vocab_size) return ge::fail(GE_ERR_ARG, "nonzero %lld: column %d outside [0,%d)", (long long)k, J[k], v.vocab_size);
        if (!std::isfinite(X[k]) || !(X[k] > 0.0f) || (v.cost_kind == GE_COST_PGLOVE && !(X[k] < 1.0f)))
            return ge::fail(GE_ERR_ARG, "nonzero %lld: value %g is not %s", (long long)k, (double)X[k],
                            v.cost_kind == GE_COST_PGLOVE ? "inside (0, 1)" : "finite and positive");
        if (k > 0 && I[k] < I[k - 1]) ascending = false;
    }

    ge_eval *e = new ge_eval;
    e->glove = h; e->view = v; e->n = n; e->n_blocks = (n + EV_SUM_BLOCK - 1) / EV_SUM_BLOCK;
    e->sums.resize((size_t)e->n_blocks);
    struct Guard { ge_eval *e; ~Guard() { if (e) eval_free(e); } } guard{e};
    // nonzeros of one focus row side by side: a wave's eight-row loads then hit the row the previous ones fetched
    std::vector<int32_t> order, sI, sJ; std::vector<float> sX;
    if (!ascending) {
        order.resize((size_t)n);
        std::iota(order.begin(), order.end(), 0);
        std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return I[a] != I[b] ? I[a] < I[b] : J[a] < J[b]; });
        sI.resize((size_t)n); sJ.resize((size_t)n); sX.resize((size_t)n);
        for (int64_t k = 0; k < n; ++k) { sI[k] = I[order[k]]; sJ[k] = J[order[k]]; sX[k] = X[order[k]]; }
        I = sI.data(); J = sJ.data(); X = sX.data();
        e->sorted = true;
    }
    GE_HIP(hipSetDevice(v.device));
    const size_t N = (size_t)n;
    GE_HIP(hipMalloc((void **)&e->dI, sizeof(int32_t) * N));
    GE_HIP(hipMalloc((void **)&e->dJ, sizeof(int32_t) * N));
    GE_HIP(hipMalloc((void **)&e->dX, sizeof(float) * N));
    GE_HIP(hipMalloc((void **)&e->dres, sizeof(float) * N));
    GE_HIP(hipMalloc((void **)&e->dterm, sizeof(double) * N));
    GE_HIP(hipMalloc((void **)&e->dsums, sizeof(double) * (size_t)e->n_blocks));
    if (e->sorted) GE_HIP(hipMalloc((void **)&e->dorder, sizeof(int32_t) * N));
    GE_HIP(hipEventCreate(&e->ev0));
    GE_HIP(hipEventCreate(&e->ev1));
    GE_HIP(hipMemcpyAsync(e->dI, I, sizeof(int32_t) * N, hipMemcpyHostToDevice, v.stream));
    GE_HIP(hipMemcpyAsync(e->dJ, J, sizeof(int32_t) * N, hipMemcpyHostToDevice, v.stream));
    GE_HIP(hipMemcpyAsync(e->dX, X, sizeof(float) * N, hipMemcpyHostToDevice, v.stream));
    if (e->sorted) GE_HIP(hipMemcpyAsync(e->dorder, order.data(), sizeof(int32_t) * N, hipMemcpyHostToDevice, v.stream));
    GE_HIP(hipStreamSynchronize(v.stream));      // the host arrays (the sorted copies among them) may go
    guard.e = nullptr;
    *out = e;
    return GE_OK;
}

ge_status eval_run_impl(ge_eval *e, float *out_residual, double *out_term, double *cost_sum) {
    if (!e) return ge::fail(GE_ERR_ARG, "null ge_eval handle");
    GE_CHECK(ge::glove_eval_view(e->glove, &e->view));          // the tables stay where they are; read again all the same
    const ge::EvalView &v = e->view;
    GE_HIP(hipSetDevice(v.device));
    EvalParams p{};
    p.focus = v.focus; p.context = v.context; p.fbias = v.fbias; p.cbias = v.cbias; p.hub32 = v.hub32; p.hub_index = v.hub_index;
    p.fs = v.focus_stride; p.cs = v.context_stride; p.fbs = v.fbias_stride; p.cbs = v.cbias_stride;
    p.I = e->dI; p.J = e->dJ; p.order = e->dorder; p.X = e->dX; p.residual = e->dres; p.term = e->dterm;
    p.xmax = v.xmax; p.n = e->n; p.D = v.dim; p.row_begin = v.row_begin; p.cost_kind = v.cost_kind;
    // 16-byte (bf16: 8-byte) row accesses where every row of every table involved starts on such a boundary
    const size_t a = v.emb16 ? 8 : 16;
    const bool wide = v.dim % 4 == 0 && v.focus_stride % 4 == 0 && v.context_stride % 4 == 0 && aligned_to(v.focus, a) &&
                      aligned_to(v.context, a) && (!v.hub32 || aligned_to(v.hub32, 16));
    const dim3 grid((unsigned)((e->n + EV_TILE - 1) / EV_TILE)), block(EV_TILE);
    GE_HIP(hipEventRecord(e->ev0, v.stream));
    if (v.emb16) {
        if (wide) hipLaunchKernelGGL((k_eval_terms<4, true>), grid, block, 0, v.stream, p);
        else      hipLaunchKernelGGL((k_eval_terms<1, true>), grid, block, 0, v.stream, p);
    } else {
        if (wide) hipLaunchKernelGGL((k_eval_terms<4, false>), grid, block, 0, v.stream, p);
        else      hipLaunchKernelGGL((k_eval_terms<1, false>), grid, block, 0, v.stream, p);
    }
    GE_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_eval_block_sums, dim3((unsigned)e->n_blocks), dim3(64), 0, v.stream, (const double *)e->dterm, e->n, e->dsums);
    GE_HIP(hipGetLastError());
    GE_HIP(hipEventRecord(e->ev1, v.stream));
    GE_HIP(hipMemcpyAsync(e->sums.data(), e->dsums, sizeof(double) * (size_t)e->n_blocks, hipMemcpyDeviceToHost, v.stream));
    if (out_residual) GE_HIP(hipMemcpyAsync(out_residual, e->dres, sizeof(float) * (size_t)e->n, hipMemcpyDeviceToHost, v.stream));
    if (out_term) GE_HIP(hipMemcpyAsync(out_term, e->dterm, sizeof(double) * (size_t)e->n, hipMemcpyDeviceToHost, v.stream));
    GE_HIP(hipStreamSynchronize(v.stream));
    GE_HIP(hipEventElapsedTime(&e->last_ms, e->ev0, e->ev1));
    double total = 0.0;
    for (int64_t b = 0; b < e->n_blocks; ++b) total = total + e->sums[(size_t)b];
    if (cost_sum) *cost_sum = total;
    return GE_OK;
}

}  // namespace

extern "C" {

ge_status ge_glove_eval_create(ge_glove *h, const int32_t *I, const int32_t *J, const float *X, int64_t n, ge_eval **out) {
    GE_GUARD(eval_create_impl(h, I, J, X, n, out));
}

ge_status ge_glove_eval_run(ge_eval *e, float *out_residual, double *out_term, double *cost_sum) {
    GE_GUARD(eval_run_impl(e, out_residual, out_term, cost_sum));
}

ge_status ge_eval_last_kernel_ms(const ge_eval *e, float *ms) {
    if (!e || !ms) return ge::fail(GE_ERR_ARG, "null argument");
    *ms = e->last_ms;
    return GE_OK;
}

ge_status ge_eval_get(const ge_eval *e, int64_t *n, int32_t *reordered) {
    if (!e) return ge::fail(GE_ERR_ARG, "null ge_eval handle");
    if (n) *n = e->n;
    if (reordered) *reordered = e->sorted ? 1 : 0;
    return GE_OK;
}

void ge_eval_destroy(ge_eval *e) { eval_free(e); }

ge_status ge_holdout_mask(uint64_t seed, int64_t n, double fraction, uint8_t *mask) {
    if (!(fraction > 0.0) || !(fraction <= 0.5)) return ge::fail(GE_ERR_ARG, "holdout fraction %g outside (0, 0.5]", fraction);
    if (n < 0 || (n > 0 && !mask)) return ge::fail(GE_ERR_ARG, "invalid n %lld or null mask", (long long)n);
    const uint64_t T = (uint64_t)std::floor(fraction * 4294967296.0);
    const uint64_t s = seed ^ 0x484F4C444F5554ull;
    for (int64_t k = 0; k < n; ++k) mask[k] = (splitmix_at(s, (uint64_t)k) >> 32) < T ? 1 : 0;
    return GE_OK;
}

}  // extern "C"
