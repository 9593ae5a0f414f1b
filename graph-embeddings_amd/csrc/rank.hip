// rank.hip -- at which place does a held-out column stand among all V columns of its row?  ge_glove_rank_* (include/geglove.h,
// "Ranking").  A pure read of a trainer handle in whichever layout it has (ge_glove_internal.h EvalView).  Per run the rows are
// staged into dense fp32 tables (k_rank_stage), the targets and the filter entries are scored pair by pair (k_rank_gather: an
// fmaf chain per lane), and every query is counted against every column on the fp32 matrix cores (k_rank_count: the score tile
// of nn.hip's k_nn_score_select with a counting epilogue).  Both scoring kernels give an fmaf chain over ascending d bit for bit,
// which is what makes  rank = 1 + dense count - filter count  exact.  The reference has no counterpart.
#include "ge_common.h"
#include "ge_glove_internal.h"
#include <algorithm>
#include <cmath>
#include <vector>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int RANK_MAX_DIM = 1024;
constexpr int64_t RANK_MAX_FILTER = (int64_t)1 << 35;        // filter entries of one set (what one launch of the gather kernel covers)

// candidate (zc, c) precedes the target (zt, j): the total order of ge_nn_* (fp32 compare, then the lower id)
__device__ __forceinline__ bool precedes(float zc, int32_t c, float zt, int32_t j) { return zc > zt || (zc == zt && c < j); }
// z from the chain's sum: one fp32 add; NaN ranks, and is reported, as -inf
__device__ __forceinline__ float z_of(float s, float bias) { const float z = s + bias; return z == z ? z : -INFINITY; }

// ---------------------------------------------------------------------------------------------------------------------
// Stage.  out[r][D4] = row `rows[r] - row_begin` (rows null: r) of a handle's table, widened from bf16 when is16, taken from the
// fp32 master when hub_index says so, padded with zeros from D to D4; bias_out[r] = that row's bias (bias_out null: none).
// One element per thread: consecutive threads write consecutive floats.
// ---------------------------------------------------------------------------------------------------------------------
struct StageParams {
    const void *table; const float *hub32, *bias;
    const int32_t *hub_index, *rows;
    float *out, *bias_out;
    int64_t n_rows, stride, bias_stride;
    int32_t D, D4, row_begin, is16;
};

__global__ __launch_bounds__(256) void k_rank_stage(StageParams p) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= p.n_rows * p.D4) return;
    const int64_t r = idx / p.D4;
    const int d = (int)(idx - r * p.D4);
    const int64_t src = p.rows ? (int64_t)p.rows[r] - p.row_begin : r;
    float x = 0.0f;
    if (d < p.D) {
        const int32_t slot = p.hub_index ? p.hub_index[src] : -1;
        if (slot >= 0) x = p.hub32[(int64_t)slot * p.D + d];
        else if (p.is16) x = __uint_as_float((uint32_t) static_cast<const uint16_t *>(p.table)[src * p.stride + d] << 16);
        else x = static_cast<const float *>(p.table)[src * p.stride + d];
    }
    p.out[idx] = x;
    if (p.bias_out && d == 0) p.bias_out[r] = p.bias[src * p.bias_stride];
}

// ---------------------------------------------------------------------------------------------------------------------
// Gather.  z for arbitrary (query, column) pairs, in the shape of eval.hip's k_eval_terms: a wavefront-sized workgroup owns 64
// pairs; per piece of 16 columns the two staged rows of every pair are read coalesced (four lanes per row, 16 bytes each,
// sixteen pairs per instruction) into the LDS panels [pair][17], and lane r walks pair r's piece in ascending d,
// s = fmaf(a[d], b[d], s), carrying s over the pieces.  The zero padding adds nothing: fmaf(0, 0, s) = s.
// filters = 0: pair e is (e, J[e]) and z goes to zt[e].  filters = 1: pair e is filter entry e, (fk[e], fidx[e]); where it is not
// the target and precedes it, one is taken off cnt[fk[e]] (an integer atomic: the dense count has counted that column).
// ---------------------------------------------------------------------------------------------------------------------
constexpr int RG_TILE = 64, RG_PIECE = 16, RG_LD = 17;

struct GatherParams {
    const float *Q, *X, *cb;                 // staged: [n][D4], [V][D4], [V]
    const int32_t *J, *fk, *fidx;
    float *zt; int32_t *cnt;
    int64_t n_pairs;
    int32_t D4, filters;
};

__global__ __launch_bounds__(RG_TILE) void k_rank_gather(GatherParams p) {
    __shared__ float s_a[RG_TILE * RG_LD];
    __shared__ float s_b[RG_TILE * RG_LD];
    __shared__ int64_t s_qoff[RG_TILE];
    __shared__ int64_t s_coff[RG_TILE];
    const int lane = (int)threadIdx.x;
    const int64_t e0 = (int64_t)blockIdx.x * RG_TILE;
    const int64_t e = e0 + lane < p.n_pairs ? e0 + lane : p.n_pairs - 1;     // the lanes past the end repeat the last pair and write nothing
    const int32_t k = p.filters ? p.fk[e] : (int32_t)e;
    const int32_t c = p.filters ? p.fidx[e] : p.J[e];
    s_qoff[lane] = (int64_t)k * p.D4;
    s_coff[lane] = (int64_t)c * p.D4;
    __syncthreads();

    const int sub = lane >> 2, col = (lane & 3) * 4;
    const float *ma = s_a + lane * RG_LD, *mb = s_b + lane * RG_LD;
    float s = 0.0f;
    for (int c0 = 0; c0 < p.D4; c0 += RG_PIECE) {
        if (c0 + col < p.D4) {                     // D4 % 4 == 0: the whole vector lies inside the row
            f32x4 f[4], g[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int r = u * 16 + sub;
                f[u] = *reinterpret_cast<const f32x4 *>(p.Q + s_qoff[r] + c0 + col);
                g[u] = *reinterpret_cast<const f32x4 *>(p.X + s_coff[r] + c0 + col);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int at = (u * 16 + sub) * RG_LD + col;
#pragma unroll
                for (int i = 0; i < 4; ++i) { s_a[at + i] = f[u][i]; s_b[at + i] = g[u][i]; }
            }
        }
        __syncthreads();
        if (p.D4 - c0 >= RG_PIECE) {               // a whole piece: the reads go out together, the chain follows in order
            float a[RG_PIECE], b[RG_PIECE];
#pragma unroll
            for (int d = 0; d < RG_PIECE; ++d) { a[d] = ma[d]; b[d] = mb[d]; }
#pragma unroll
            for (int d = 0; d < RG_PIECE; ++d) s = fmaf(a[d], b[d], s);
        } else {
            for (int d = 0; d < p.D4 - c0; ++d) s = fmaf(ma[d], mb[d], s);
        }
        __syncthreads();
    }
    if (e0 + lane >= p.n_pairs) return;
    const float z = z_of(s, p.cb[c]);
    if (!p.filters) { p.zt[e] = z; return; }
    const int32_t j = p.J[k];
    if (c != j && precedes(z, c, p.zt[k], j)) atomicSub(&p.cnt[k], 1);
}

// ---------------------------------------------------------------------------------------------------------------------
// Count.  The score tile of k_nn_score_select: a workgroup owns 64 queries (blockIdx.x, the fast index: workgroups that read
// the same candidate panels run together) and one range of whole 128-candidate tiles (blockIdx.y); per 32 columns the query and
// candidate panels are staged in LDS as [row][34] (the next panel travels in registers meanwhile), and wave w carries queries
// 16 w .. 16 w + 15 against the 128 candidates through v_mfma_f32_16x16x4_f32: eight accumulators, each bit for bit an fmaf chain
// over ascending d.  The epilogue keeps no list: every lane adds the column's bias to its 32 scores, compares them with its four
// queries' (z_target, J) and counts in four registers across the whole range; at the end the sixteen lanes that share a query
// add their counts up and one integer atomic per (query, range) goes to cnt[query].
// ---------------------------------------------------------------------------------------------------------------------
constexpr int RC_TQ = 64, RC_TC = 128, RC_DK = 32, RC_LS = 34;
constexpr int RC_LOADS = (RC_TQ + RC_TC) * (RC_DK / 4) / 256;   // 16-byte pieces a thread moves per panel: 2 of queries, 4 of candidates

__global__ __launch_bounds__(256, 3) void k_rank_count(const float *__restrict__ Q, int64_t nq, const float *__restrict__ X, const float *__restrict__ cb,
                                                       int64_t n, int32_t D4, int64_t range_len, const float *__restrict__ zt,
                                                       const int32_t *__restrict__ J, int32_t *__restrict__ cnt) {
    __shared__ float sq[RC_TQ * RC_LS];
    __shared__ float sx[RC_TC * RC_LS];

    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t q0 = (int64_t)blockIdx.x * RC_TQ;
    const int64_t c_begin = (int64_t)blockIdx.y * range_len;
    const int64_t c_end = c_begin + range_len < n ? c_begin + range_len : n;

    // what this thread stages: piece i of a panel is row (tid + 256 i) >> 3, columns 4 ((tid + 256 i) & 7) ..
    const int c4 = (tid & 7) * 4, prow = tid >> 3;
    const float *qsrc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int64_t qg = q0 + prow + 32 * i;
        qsrc[i] = qg < nq ? Q + qg * D4 : nullptr;
    }
    f32x4 pre[RC_LOADS];
    auto fetch = [&](int64_t ct, int d0) {
        const bool in = d0 + c4 < D4;
#pragma unroll
        for (int i = 0; i < 2; ++i)
            pre[i] = in && qsrc[i] ? *reinterpret_cast<const f32x4 *>(qsrc[i] + d0 + c4) : f32x4{0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t c = ct + prow + 32 * i;
            pre[2 + i] = in && c < c_end ? *reinterpret_cast<const f32x4 *>(X + c * D4 + d0 + c4) : f32x4{0, 0, 0, 0};
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int i = 0; i < RC_LOADS; ++i) {
            float *dst = (i < 2 ? sq + (prow + 32 * i) * RC_LS : sx + (prow + 32 * (i - 2)) * RC_LS) + c4;   // 8-byte aligned: RC_LS and c4 are even
            *reinterpret_cast<float2 *>(dst) = float2{pre[i][0], pre[i][1]};
            *reinterpret_cast<float2 *>(dst + 2) = float2{pre[i][2], pre[i][3]};
        }
    };

    // the four queries whose scores a lane holds: local rows 4 (lane >> 4) + reg of the wave's sixteen
    const int qb = wave * 16;
    const int ql = qb + 4 * (lane >> 4);
    float tz[4];
    int32_t tj[4], count[4];
    bool qok[4];
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        const int64_t qg = q0 + ql + reg;
        qok[reg] = qg < nq;
        tz[reg] = qok[reg] ? zt[qg] : 0.0f;
        tj[reg] = qok[reg] ? J[qg] : -1;
        count[reg] = 0;
    }
    const int xa = (qb + (lane & 15)) * RC_LS + (lane >> 4);
    const int xb = (lane & 15) * RC_LS + (lane >> 4);

    if (c_begin < c_end) fetch(c_begin, 0);
    for (int64_t ct = c_begin; ct < c_end; ct += RC_TC) {
        f32x4 acc[RC_TC / 16];
#pragma unroll
        for (int t = 0; t < RC_TC / 16; ++t) acc[t] = f32x4{0, 0, 0, 0};
        for (int d0 = 0; d0 < D4; d0 += RC_DK) {
            __syncthreads();
            stage();
            __syncthreads();
            if (d0 + RC_DK < D4) fetch(ct, d0 + RC_DK);
            else if (ct + RC_TC < c_end) fetch(ct + RC_TC, 0);
            auto step = [&](int dd) {
                const float a = sq[xa + dd];
                float b[RC_TC / 16];
#pragma unroll
                for (int t = 0; t < RC_TC / 16; ++t) b[t] = sx[xb + t * 16 * RC_LS + dd];
#pragma unroll
                for (int t = 0; t < RC_TC / 16; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b[t], acc[t], 0, 0, 0);
            };
            if (D4 - d0 >= RC_DK) {                                   // a whole panel: unrolled, so the reads of a step run ahead of its products
#pragma unroll
                for (int dd = 0; dd < RC_DK; dd += 4) step(dd);
            } else {
#pragma unroll 1
                for (int dd = 0; dd < D4 - d0; dd += 4) step(dd);
            }
        }
        // C/D of the f32 form: column (candidate) = lane & 15, row (query) = 4 * (lane >> 4) + register
#pragma unroll
        for (int t = 0; t < RC_TC / 16; ++t) {
            const int64_t c = ct + t * 16 + (lane & 15);
            const bool in = c < c_end;
            const float bias = in ? cb[c] : 0.0f;
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const float z = z_of(acc[t][reg], bias);
                count[reg] += in && (int32_t)c != tj[reg] && precedes(z, (int32_t)c, tz[reg], tj[reg]) ? 1 : 0;
            }
        }
    }
    // the sixteen lanes lane & 15 = 0 .. 15 of a quarter hold the counts of the same four queries
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        int v = count[reg];
#pragma unroll
        for (int m = 1; m < 16; m <<= 1) v += __shfl_xor(v, m, 64);
        if ((lane & 15) == 0 && qok[reg] && v) atomicAdd(&cnt[q0 + ql + reg], v);
    }
}

}  // namespace

struct ge_rank {
    ge_glove *glove = nullptr;
    ge::EvalView view{};
    int64_t n = 0, nf = 0;               // pairs; filter entries in all
    int32_t d4 = 0, ranges = 0;          // ranges: the candidate ranges of the last run's grid
    int32_t *dI = nullptr, *dJ = nullptr, *dfk = nullptr, *dfidx = nullptr, *dcnt = nullptr;
    float *dq = nullptr, *dx = nullptr, *dcb = nullptr, *dzt = nullptr;
    std::vector<int32_t> cnt;            // the counts on the host: rank = 1 + cnt
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};     // around staging, gather and count
    float stage_ms = 0.0f, gather_ms = 0.0f, count_ms = 0.0f;
};

namespace {

void rank_free(ge_rank *r) {
    if (!r) return;
    (void)hipSetDevice(r->view.device);
    for (void *q : {(void *)r->dI, (void *)r->dJ, (void *)r->dfk, (void *)r->dfidx, (void *)r->dcnt, (void *)r->dq, (void *)r->dx, (void *)r->dcb,
                    (void *)r->dzt})
        if (q) (void)hipFree(q);
    for (hipEvent_t e : r->ev)
        if (e) (void)hipEventDestroy(e);
    delete r;
}

ge_status rank_create_impl(ge_glove *h, const int32_t *I, const int32_t *J, int64_t n, const int64_t *filter_ptr, const int32_t *filter_idx,
                           ge_rank **out) {
    if (!out) return ge::fail(GE_ERR_ARG, "out is null");
    *out = nullptr;
    if (!I || !J) return ge::fail(GE_ERR_ARG, "null rank arrays");
    if (n < 1 || n >= ((int64_t)1 << 31)) return ge::fail(GE_ERR_ARG, "a rank set holds 1 <= n < 2^31 pairs, got %lld", (long long)n);
    // what needs no handle: the shape of the lists, ids below zero, the order inside a list
    int64_t nf = 0;
    if (filter_ptr) {
        if (filter_ptr[0] != 0) return ge::fail(GE_ERR_ARG, "filter_ptr[0] is %lld, not 0", (long long)filter_ptr[0]);
        for (int64_t k = 0; k < n; ++k)
            if (filter_ptr[k + 1] < filter_ptr[k]) return ge::fail(GE_ERR_ARG, "filter_ptr decreases at [%lld]", (long long)(k + 1));
        nf = filter_ptr[n];
        if (nf >= RANK_MAX_FILTER) return ge::fail(GE_ERR_ARG, "%lld filter entries are more than one set holds (2^35)", (long long)nf);
        if (nf > 0 && !filter_idx) return ge::fail(GE_ERR_ARG, "filter_idx is null");
    }
    for (int64_t k = 0; k < n; ++k) {
        if (I[k] < 0) return ge::fail(GE_ERR_ARG, "pair %lld: focus row %d out of range", (long long)k, I[k]);
        if (J[k] < 0) return ge::fail(GE_ERR_ARG, "pair %lld: column %d out of range", (long long)k, J[k]);
        if (!filter_ptr) continue;
        for (int64_t e = filter_ptr[k]; e < filter_ptr[k + 1]; ++e) {
            if (filter_idx[e] < 0) return ge::fail(GE_ERR_ARG, "pair %lld: filter id %d out of range", (long long)k, filter_idx[e]);
            if (e > filter_ptr[k] && filter_idx[e] <= filter_idx[e - 1])
                return ge::fail(GE_ERR_ARG, "pair %lld: the filter list is not strictly ascending at entry %lld", (long long)k, (long long)(e - filter_ptr[k]));
        }
    }
    if (!h) return ge::fail(GE_ERR_ARG, "null ge_glove handle");
    ge::EvalView v;
    GE_CHECK(ge::glove_eval_view(h, &v));
    if (v.dim < 1 || v.dim > RANK_MAX_DIM) return ge::fail(GE_ERR_ARG, "rank: dim %d outside [1, %d]", v.dim, RANK_MAX_DIM);
    for (int64_t k = 0; k < n; ++k) {
        if (I[k] < v.row_begin || I[k] >= v.row_end)
            return ge::fail(GE_ERR_ARG, "pair %lld: focus row %d outside the handle's rows [%d,%d)", (long long)k, I[k], v.row_begin, v.row_end);
        if (J[k] >= v.vocab_size) return ge::fail(GE_ERR_ARG, "pair %lld: column %d outside [0,%d)", (long long)k, J[k], v.vocab_size);
        // a list ascends, so its last id is its largest
        if (filter_ptr && filter_ptr[k + 1] > filter_ptr[k] && filter_idx[filter_ptr[k + 1] - 1] >= v.vocab_size)
            return ge::fail(GE_ERR_ARG, "pair %lld: filter id %d outside [0,%d)", (long long)k, filter_idx[filter_ptr[k + 1] - 1], v.vocab_size);
    }

    ge_rank *r = new ge_rank;
    r->glove = h; r->view = v; r->n = n; r->nf = nf; r->d4 = (v.dim + 3) / 4 * 4;
    struct Guard { ge_rank *r; ~Guard() { if (r) rank_free(r); } } guard{r};
    r->cnt.resize((size_t)n);
    std::vector<int32_t> fk((size_t)nf);                       // the pair of every filter entry
    for (int64_t k = 0; k < n && filter_ptr; ++k)
        for (int64_t e = filter_ptr[k]; e < filter_ptr[k + 1]; ++e) fk[(size_t)e] = (int32_t)k;
    GE_HIP(hipSetDevice(v.device));
    const size_t N = (size_t)n, V = (size_t)v.vocab_size, D4 = (size_t)r->d4;
    GE_HIP(hipMalloc((void **)&r->dI, sizeof(int32_t) * N));
    GE_HIP(hipMalloc((void **)&r->dJ, sizeof(int32_t) * N));
    GE_HIP(hipMalloc((void **)&r->dcnt, sizeof(int32_t) * N));
    GE_HIP(hipMalloc((void **)&r->dzt, sizeof(float) * N));
    GE_HIP(hipMalloc((void **)&r->dq, sizeof(float) * N * D4));
    GE_HIP(hipMalloc((void **)&r->dx, sizeof(float) * V * D4));
    GE_HIP(hipMalloc((void **)&r->dcb, sizeof(float) * V));
    if (nf > 0) {
        GE_HIP(hipMalloc((void **)&r->dfk, sizeof(int32_t) * (size_t)nf));
        GE_HIP(hipMalloc((void **)&r->dfidx, sizeof(int32_t) * (size_t)nf));
    }
    for (hipEvent_t &e : r->ev) GE_HIP(hipEventCreate(&e));
    GE_HIP(hipMemcpyAsync(r->dI, I, sizeof(int32_t) * N, hipMemcpyHostToDevice, v.stream));
    GE_HIP(hipMemcpyAsync(r->dJ, J, sizeof(int32_t) * N, hipMemcpyHostToDevice, v.stream));
    if (nf > 0) {
        GE_HIP(hipMemcpyAsync(r->dfk, fk.data(), sizeof(int32_t) * (size_t)nf, hipMemcpyHostToDevice, v.stream));
        GE_HIP(hipMemcpyAsync(r->dfidx, filter_idx, sizeof(int32_t) * (size_t)nf, hipMemcpyHostToDevice, v.stream));
    }
    GE_HIP(hipStreamSynchronize(v.stream));      // the host arrays may go
    guard.r = nullptr;
    *out = r;
    return GE_OK;
}

ge_status launch_stage(const StageParams &p, hipStream_t stream) {
    const int64_t blocks = (p.n_rows * p.D4 + 255) / 256;
    hipLaunchKernelGGL(k_rank_stage, dim3((unsigned)blocks), dim3(256), 0, stream, p);
    GE_HIP(hipGetLastError());
    return GE_OK;
}

ge_status rank_run_impl(ge_rank *r, int32_t *out_rank, float *out_score, ge_rank_summary *summary) {
    if (!r) return ge::fail(GE_ERR_ARG, "null ge_rank handle");
    GE_CHECK(ge::glove_eval_view(r->glove, &r->view));          // the tables move between epochs: read where they are now
    const ge::EvalView &v = r->view;
    GE_HIP(hipSetDevice(v.device));
    const int64_t n = r->n, V = v.vocab_size;
    const int32_t D4 = r->d4;
    hipStream_t stream = v.stream;
    GE_HIP(hipMemsetAsync(r->dcnt, 0, sizeof(int32_t) * (size_t)n, stream));

    GE_HIP(hipEventRecord(r->ev[0], stream));
    StageParams q{};
    q.table = v.focus; q.rows = r->dI; q.out = r->dq; q.n_rows = n; q.stride = v.focus_stride;
    q.D = v.dim; q.D4 = D4; q.row_begin = v.row_begin; q.is16 = v.emb16;
    GE_CHECK(launch_stage(q, stream));
    StageParams x{};
    x.table = v.context; x.hub32 = v.hub32; x.hub_index = v.emb16 ? v.hub_index : nullptr; x.bias = v.cbias;
    x.out = r->dx; x.bias_out = r->dcb; x.n_rows = V; x.stride = v.context_stride; x.bias_stride = v.cbias_stride;
    x.D = v.dim; x.D4 = D4; x.is16 = v.emb16;
    GE_CHECK(launch_stage(x, stream));

    GE_HIP(hipEventRecord(r->ev[1], stream));
    GatherParams g{};
    g.Q = r->dq; g.X = r->dx; g.cb = r->dcb; g.J = r->dJ; g.fk = r->dfk; g.fidx = r->dfidx; g.zt = r->dzt; g.cnt = r->dcnt; g.D4 = D4;
    g.n_pairs = n; g.filters = 0;
    hipLaunchKernelGGL(k_rank_gather, dim3((unsigned)((n + RG_TILE - 1) / RG_TILE)), dim3(RG_TILE), 0, stream, g);
    GE_HIP(hipGetLastError());
    if (r->nf > 0) {
        g.n_pairs = r->nf; g.filters = 1;
        hipLaunchKernelGGL(k_rank_gather, dim3((unsigned)((r->nf + RG_TILE - 1) / RG_TILE)), dim3(RG_TILE), 0, stream, g);
        GE_HIP(hipGetLastError());
    }

    GE_HIP(hipEventRecord(r->ev[2], stream));
    // candidate ranges: whole tiles of RC_TC, as many as fill the device a few times over when the query tiles alone do not
    const int64_t ctiles = (V + RC_TC - 1) / RC_TC, qtiles = (n + RC_TQ - 1) / RC_TQ;
    const int64_t want = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(ctiles, 1024), (2048 + qtiles - 1) / qtiles));
    const int64_t range_tiles = (ctiles + want - 1) / want;
    const int64_t ranges = (ctiles + range_tiles - 1) / range_tiles, range_len = range_tiles * RC_TC;
    r->ranges = (int32_t)ranges;
    hipLaunchKernelGGL(k_rank_count, dim3((unsigned)qtiles, (unsigned)ranges), dim3(256), 0, stream, (const float *)r->dq, n, (const float *)r->dx,
                       (const float *)r->dcb, V, D4, range_len, (const float *)r->dzt, (const int32_t *)r->dJ, r->dcnt);
    GE_HIP(hipGetLastError());
    GE_HIP(hipEventRecord(r->ev[3], stream));

    GE_HIP(hipMemcpyAsync(r->cnt.data(), r->dcnt, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, stream));
    if (out_score) GE_HIP(hipMemcpyAsync(out_score, r->dzt, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, stream));
    GE_HIP(hipStreamSynchronize(stream));
    GE_HIP(hipEventElapsedTime(&r->stage_ms, r->ev[0], r->ev[1]));
    GE_HIP(hipEventElapsedTime(&r->gather_ms, r->ev[1], r->ev[2]));
    GE_HIP(hipEventElapsedTime(&r->count_ms, r->ev[2], r->ev[3]));

    ge_rank_summary s{};
    s.n = n;
    double inv = 0.0, sum = 0.0;
    for (int64_t k = 0; k < n; ++k) {
        const int32_t rank = 1 + r->cnt[(size_t)k];
        if (out_rank) out_rank[k] = rank;
        inv = inv + 1.0 / (double)rank;
        sum = sum + (double)rank;
        s.hits1 += rank <= 1; s.hits10 += rank <= 10; s.hits100 += rank <= 100;
    }
    s.mrr = inv / (double)n;
    s.mean_rank = sum / (double)n;
    if (summary) *summary = s;
    return GE_OK;
}

}  // namespace

extern "C" {

ge_status ge_glove_rank_create(ge_glove *h, const int32_t *I, const int32_t *J, int64_t n, const int64_t *filter_ptr, const int32_t *filter_idx,
                               ge_rank **out) {
    GE_GUARD(rank_create_impl(h, I, J, n, filter_ptr, filter_idx, out));
}

ge_status ge_glove_rank_run(ge_rank *r, int32_t *out_rank, float *out_score, ge_rank_summary *summary) {
    GE_GUARD(rank_run_impl(r, out_rank, out_score, summary));
}

ge_status ge_rank_last_kernel_ms(const ge_rank *r, float *ms) {
    if (!r || !ms) return ge::fail(GE_ERR_ARG, "null argument");
    *ms = r->stage_ms + r->gather_ms + r->count_ms;
    return GE_OK;
}

ge_status ge_rank_last_phase_ms(const ge_rank *r, float *stage_ms, float *gather_ms, float *count_ms) {
    if (!r) return ge::fail(GE_ERR_ARG, "null ge_rank handle");
    if (stage_ms) *stage_ms = r->stage_ms;
    if (gather_ms) *gather_ms = r->gather_ms;
    if (count_ms) *count_ms = r->count_ms;
    return GE_OK;
}

ge_status ge_rank_get(const ge_rank *r, int64_t *n, int64_t *candidates, int32_t *dim, int32_t *ranges) {
    if (!r) return ge::fail(GE_ERR_ARG, "null ge_rank handle");
    if (n) *n = r->n;
    if (candidates) *candidates = r->view.vocab_size;
    if (dim) *dim = r->view.dim;
    if (ranges) *ranges = r->ranges;
    return GE_OK;
}

int32_t ge_rank_summary_size(void) { return (int32_t)sizeof(ge_rank_summary); }

void ge_rank_destroy(ge_rank *r) { rank_free(r); }

}  // extern "C"
