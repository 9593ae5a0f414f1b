// fold.hip -- embed rows that arrive after training: ge_glove_fold_* (include/geglove.h, "Fold-in") and the host-only rule
// ge_foldin_mask.  A new row (its nonzeros against the trained columns) is fitted by the AdaGrad update of GE_ARITH_FP32 with the
// other side left alone: a pure read of a trainer handle in whichever layout it has (ge_glove_internal.h EvalView).
//   one wave per row    the new row, its accumulator row, its bias and the bias accumulator stay in the registers of one wavefront
//                       from the first update of epoch 0 to the last of epoch E - 1 (ge_wave.h's lane shape); all epochs run inside
//                       one launch.  Workgroups of four waves, no LDS, no barrier, no atomics; rows are handed out longest first.
//   frozen rows         read in place through buffer resources that end with the row.  They are never written, so their loads do
//                       not depend on the updates: fold_prefetch() rows are requested ahead of the one being computed.
//   the stream          (idx, l, w) is read 64 nonzeros at a time, lane t taking entry base + t (or the entry its walk position
//                       names), and handed out with readlane; the block after the current one is read while this one is computed,
//                       its bias scalars (and, for bf16 handles with masters, its hub slots) once its ids have arrived.
// Compiled with -ffp-contract=off: the fused multiply-adds are the explicit ones.
#include "ge_cost.h"
#include "ge_glove_internal.h"
#include "ge_strata.h"
#include "ge_wave.h"

#include <algorithm>
#include <cmath>
#include <numeric>
#include <type_traits>
#include <vector>

namespace {

using namespace ge;

constexpr int FOLD_MAX_EPOCHS = 1024;
// Frozen rows in flight beside the one being computed.  Every instance stays inside 128 VGPRs (four waves per SIMD) without
// scratch: a lane that holds twelve floats of a row or more gets there with one row ahead instead of two.
constexpr int fold_prefetch(int vw, int nch) { return vw * nch >= 12 ? 1 : 2; }

// (l, w) of every nonzero of the set, once per set, as k_strata_terms
__global__ void k_fold_terms(const float *__restrict__ X, int64_t n, int kind, double xmax, double *__restrict__ L, float *__restrict__ W) {
    int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; k < n; k += stride) {
        double l; float w;
        cost_terms<true>(kind, X[k], xmax, l, w);
        L[k] = l; W[k] = w;
    }
}

struct FoldParams {
    const void *table;                   // the frozen side's rows: fp32, or bf16 (EMB16 instances)
    const float *bias, *hub32;           // its bias scalars; EMB16: the fp32 master rows
    const int32_t *hub_index;            // EMB16: id -> row of hub32, < 0 = none; null = no masters
    int64_t stride, bias_stride;         // in elements
    const int64_t *row_ptr;              // [n_rows + 1]
    const int32_t *order, *idx;          // rows by descending length; the set's ids
    const double *L; const float *W;
    float *rows, *rbias, *cost;          // results; rows and rbias hold the initial values on entry
    int64_t seed;
    int32_t n_rows, D, base, E, shuffle;
    float lr;
};

// 64 nonzeros of the stream, one per lane
struct FoldEntries { int32_t id, slot, llo, lhi; float w, fbo; };

__device__ __forceinline__ float widen16(uint32_t bits16) { return __uint_as_float(bits16 << 16); }

template <int VW, int NCH, bool EMB16>
__global__ __launch_bounds__(256, 4) void k_fold_rows(FoldParams p) {
    using V = typename Vec<VW>::T;
    constexpr int PF = fold_prefetch(VW, NCH), R = PF + 1;
    const int lane = threadIdx.x & 63;
    const int64_t place = (int64_t)blockIdx.x * 4 + rfl((int)(threadIdx.x >> 6));
    if (place >= p.n_rows) return;
    const int32_t r = rfl(p.order[place]);
    const int32_t begin = rfl((int32_t)p.row_ptr[r]);                   // the set holds fewer than 2^31 nonzeros
    const uint32_t n = (uint32_t)rfl((int32_t)(p.row_ptr[r + 1] - p.row_ptr[r]));
    const int32_t D = p.D, E = p.E;
    float *cost = p.cost + (int64_t)r * E;
    if (n == 0) {                                                       // the row keeps its initial values
        for (int e = lane; e < E; e += 64) cost[e] = 0.0f;
        return;
    }
    const bool in_last = (lane + 64 * (NCH - 1)) * VW < D;              // only the last chunk can be partial (D % VW == 0)
    const float lr = p.lr;
    uint32_t mask = 0, shift = 1;
    if (p.shuffle) strata_width(n, &mask, &shift);

    // the new row: lanes past it read 0 and store nothing
    const __amdgpu_buffer_rsrc_t mine = make_rsrc(p.rows + (int64_t)r * D, (uint32_t)D * 4u);
    V a[NCH], G[NCH];
#pragma unroll
    for (int q = 0; q < NCH; ++q) {
        a[q] = buf_load<VW, AUX_PLAIN>(mine, (lane + q * 64) * VW * 4);
#pragma unroll
        for (int t = 0; t < VW; ++t) comp<VW>(G[q], t) = 1.0f;
    }
    float fb = p.rbias[r], gfb = 1.0f;

    // entries [base_k, base_k + 64) of epoch e: where they are, then (ids, l, w)
    auto load_entries = [&](FoldEntries &s, int32_t e, uint32_t base_k) {
        uint32_t key[4] = {0, 0, 0, 0};
        if (p.shuffle) strata_keys(p.seed, e, 0u, key);
        const uint32_t k = base_k + (uint32_t)lane;
        s.id = p.base; s.slot = -1; s.llo = 0; s.lhi = 0; s.w = 0.0f; s.fbo = 0.0f;
        if (k < n) {
            const int64_t at = (int64_t)begin + (p.shuffle ? strata_walk(k, n, mask, shift, key) : k);      // < n: inside the row
            s.id = p.idx[at];
            const double l = p.L[at];
            s.llo = __double2loint(l); s.lhi = __double2hiint(l);
            s.w = p.W[at];
        }
    };
    // what the ids name: the frozen bias scalars and, where the handle keeps fp32 masters, which rows have one
    auto load_named = [&](FoldEntries &s, uint32_t base_k) {
        if (base_k + (uint32_t)lane < n) {
            s.fbo = p.bias[(int64_t)(s.id - p.base) * p.bias_stride];
            if (EMB16 && p.hub_index) s.slot = p.hub_index[s.id];
        }
    };

    V row[R][NCH];
    bool master[R];
    auto rdl = [&](int v, int t) { return __builtin_amdgcn_readlane(v, t); };
    // The frozen row of entry t into ring slot S: NCH vw-wide loads on every path (the host checks that every row of the table
    // starts on such a boundary), so the compiler can count what is in flight.  A bf16 row stays as loaded -- four bf16 in the low
    // halves of .x and .y -- and is widened when it is used.
    auto request = [&](auto S, const FoldEntries &s, int t) {
        constexpr int slot = decltype(S)::value;
        const int32_t id = rdl(s.id, t);
        master[slot] = false;
        if constexpr (EMB16) {
            const int32_t hub = rdl(s.slot, t);
            master[slot] = hub >= 0;
            if (master[slot]) {
                const __amdgpu_buffer_rsrc_t rs = make_rsrc(p.hub32 + (int64_t)hub * D, (uint32_t)D * 4u);
#pragma unroll
                for (int q = 0; q < NCH; ++q) row[slot][q] = buf_load<VW, AUX_PLAIN>(rs, (lane + q * 64) * VW * 4);
            } else {
                const uint16_t *at = static_cast<const uint16_t *>(p.table) + (int64_t)(id - p.base) * p.stride;
                const __amdgpu_buffer_rsrc_t rs = make_rsrc(at, (uint32_t)D * 2u);
#pragma unroll
                for (int q = 0; q < NCH; ++q) {
                    const int off = (lane + q * 64) * VW * 2;
                    const ge_i2 v = __builtin_amdgcn_raw_buffer_load_b64(rs, off, 0, AUX_PLAIN);
                    comp<VW>(row[slot][q], 0) = __int_as_float(v[0]);
                    comp<VW>(row[slot][q], 1) = __int_as_float(v[1]);
                }
            }
        } else {
            const float *at = static_cast<const float *>(p.table) + (int64_t)(id - p.base) * p.stride;
            const __amdgpu_buffer_rsrc_t rs = make_rsrc(at, (uint32_t)D * 4u);
#pragma unroll
            for (int q = 0; q < NCH; ++q) row[slot][q] = buf_load<VW, AUX_PLAIN>(rs, (lane + q * 64) * VW * 4);
        }
    };

    float c = 0.0f;
    // one update against the row in ring slot S
    auto update = [&](auto S, const FoldEntries &s, int t) {
        constexpr int slot = decltype(S)::value;
        const double l = __hiloint2double(rdl(s.lhi, t), rdl(s.llo, t));
        const float w = __int_as_float(rdl(__float_as_int(s.w), t)), fbo = __int_as_float(rdl(__float_as_int(s.fbo), t));
        V *b = row[slot];
        if constexpr (EMB16) {
            if (!master[slot]) {                                        // a bf16 row is widened where it lies
#pragma unroll
                for (int q = 0; q < NCH; ++q) {
                    const uint32_t lo = __float_as_uint(comp<VW>(b[q], 0)), hi = __float_as_uint(comp<VW>(b[q], 1));
                    comp<VW>(b[q], 0) = widen16(lo & 0xFFFFu); comp<VW>(b[q], 1) = widen16(lo >> 16);
                    comp<VW>(b[q], 2) = widen16(hi & 0xFFFFu); comp<VW>(b[q], 3) = widen16(hi >> 16);
                }
            }
        }
        float part = 0.0f;
#pragma unroll
        for (int q = 0; q < NCH; ++q)
#pragma unroll
            for (int t2 = 0; t2 < VW; ++t2) part = __builtin_fmaf(comp<VW>(a[q], t2), comp<VW>(b[q], t2), part);
        const float dot = wave_sum(part);
        const float ic = (float)((double)dot + ((double)(fb + fbo) - l));
        const float wc = w * ic;
        c = (float)((double)c + (0.5 * (double)wc) * (double)ic);
#pragma unroll
        for (int q = 0; q < NCH; ++q) {
#pragma unroll
            for (int t2 = 0; t2 < VW; ++t2) {
                float &av = comp<VW>(a[q], t2), &ga = comp<VW>(G[q], t2);
                const float g = wc * comp<VW>(b[q], t2);
                float na = av - (g / __builtin_sqrtf(ga)) * lr;
                if (q == NCH - 1 && !in_last) na = 0.0f;                // a lane past the row keeps 0 there whatever wc is
                av = na;
                ga = ga + g * g;
            }
        }
        fb = fb - wc / __builtin_sqrtf(gfb);
        gfb = gfb + wc * wc;
    };
    using S0 = std::integral_constant<int, 0>;
    using S1 = std::integral_constant<int, 1 % R>;
    using S2 = std::integral_constant<int, 2 % R>;
    // update t from ring slot S with the row of update t + PF requested first: AHEAD = that update exists (the steady part of a
    // block, no test), else it is looked for (the last updates of a block)
    auto step = [&](auto S, auto AHEAD, const FoldEntries &s, int t, int cnt) {
        constexpr int slot = decltype(S)::value;
        if (decltype(AHEAD)::value || t + PF < cnt) request(std::integral_constant<int, (slot + PF) % R>{}, s, t + PF);
        __builtin_amdgcn_sched_barrier(0);                              // the request goes out first; updates are not interleaved
        update(S, s, t);
        __builtin_amdgcn_sched_barrier(0);
    };

    const uint32_t blocks = (n + 63u) >> 6;
    FoldEntries cur, nxt;
    load_entries(cur, 0, 0u);
    load_named(cur, 0u);
    nxt = cur;
    for (int32_t e = 0; e < E; ++e) {
        c = 0.0f;
        for (uint32_t blk = 0; blk < blocks; ++blk) {
            const uint32_t base_k = blk << 6;
            const int cnt = (int)(n - base_k < 64u ? n - base_k : 64u);
            const bool last_of_epoch = blk + 1 == blocks;
            const bool more = !(last_of_epoch && e + 1 == E);
            const uint32_t next_k = last_of_epoch ? 0u : base_k + 64u;
            if (more) load_entries(nxt, last_of_epoch ? e + 1 : e, next_k);
            request(S0{}, cur, 0);
            if (PF > 1 && cnt > 1) request(S1{}, cur, 1);
            // what the next block's ids name: the ids were requested before this block's first rows, so waiting for them here
            // costs nothing that the first update would not wait for anyway
            if (more) load_named(nxt, next_k);
            int t = 0;
            for (; t + R + PF - 1 < cnt; t += R) {                  // every request of the group has its update: no test
                step(S0{}, std::true_type{}, cur, t, cnt);
                step(S1{}, std::true_type{}, cur, t + 1, cnt);
                if constexpr (R > 2) step(S2{}, std::true_type{}, cur, t + 2, cnt);
            }
            for (; t < cnt; t += R) {                               // the last R + PF - 1 updates at the most
                step(S0{}, std::false_type{}, cur, t, cnt);
                if (t + 1 < cnt) step(S1{}, std::false_type{}, cur, t + 1, cnt);
                if (R > 2 && t + 2 < cnt) step(S2{}, std::false_type{}, cur, t + 2, cnt);
            }
            cur = nxt;
        }
        if (lane == 0) cost[e] = c;
    }
#pragma unroll
    for (int q = 0; q < NCH; ++q) buf_store<VW>(a[q], mine, (lane + q * 64) * VW * 4);
    if (lane == 0) p.rbias[r] = fb;
}

using fold_fn = void (*)(FoldParams);
template <int VW, bool EMB16> fold_fn pick_nch(int nch) {
    switch (nch) {
        case 1: return k_fold_rows<VW, 1, EMB16>;
        case 2: return k_fold_rows<VW, 2, EMB16>;
        case 3: return k_fold_rows<VW, 3, EMB16>;
        case 4: return k_fold_rows<VW, 4, EMB16>;
    }
    return nullptr;
}
// the Hogwild lane shape: vw floats per lane, nch chunks of 64 lanes
void lane_shape(int32_t D, int *vw, int *nch) {
    *vw = D % 4 == 0 ? 4 : D % 2 == 0 ? 2 : 1;
    *nch = (D + 64 * *vw - 1) / (64 * *vw);
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

struct ge_fold {
    ge_glove *glove = nullptr;
    ge::EvalView view{};
    ge_fold_cfg cfg{};
    int64_t n_rows = 0, nnz = 0, longest = 0;
    int64_t *drow_ptr = nullptr;
    int32_t *dorder = nullptr, *didx = nullptr;
    double *dL = nullptr;
    float *dW = nullptr, *dX = nullptr, *drows = nullptr, *dbias = nullptr, *dcost = nullptr;
    std::vector<float> cost;             // [n_rows * E] on the host: cost_history is summed from it
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    float last_ms = 0.0f;
};

namespace {

void fold_free(ge_fold *f) {
    if (!f) return;
    (void)hipSetDevice(f->view.device);
    for (void *q : {(void *)f->drow_ptr, (void *)f->dorder, (void *)f->didx, (void *)f->dL, (void *)f->dW, (void *)f->dX, (void *)f->drows,
                    (void *)f->dbias, (void *)f->dcost})
        if (q) (void)hipFree(q);
    if (f->ev0) (void)hipEventDestroy(f->ev0);
    if (f->ev1) (void)hipEventDestroy(f->ev1);
    delete f;
}

ge_status fold_create_impl(ge_glove *h, const int64_t *row_ptr, const int32_t *idx, const float *X, int64_t n_rows, const ge_fold_cfg *cfg,
                           ge_fold **out) {
    if (!out) return ge::fail(GE_ERR_ARG, "out is null");
    *out = nullptr;
    if (!row_ptr || !idx || !X) return ge::fail(GE_ERR_ARG, "null fold-in arrays");
    if (!cfg) return ge::fail(GE_ERR_ARG, "null ge_fold_cfg");
    if (n_rows < 1 || n_rows >= ((int64_t)1 << 31)) return ge::fail(GE_ERR_ARG, "a fold-in set holds 1 <= n_rows < 2^31 rows, got %lld", (long long)n_rows);
    // what needs no handle: the configuration, the shape of the rows, ids below zero, the values
    if (cfg->side != GE_FOLD_FOCUS && cfg->side != GE_FOLD_CONTEXT) return ge::fail(GE_ERR_ARG, "fold: unknown side %d", cfg->side);
    if (cfg->shuffle == GE_SHUFFLE_JAVA) return ge::fail(GE_ERR_ARG, "fold: GE_SHUFFLE_JAVA has no per-row order, choose GE_SHUFFLE_NONE or GE_SHUFFLE_DEVICE");
    if (cfg->shuffle != GE_SHUFFLE_NONE && cfg->shuffle != GE_SHUFFLE_DEVICE) return ge::fail(GE_ERR_ARG, "fold: unknown shuffle %d", cfg->shuffle);
    if (cfg->epochs < 1 || cfg->epochs > FOLD_MAX_EPOCHS) return ge::fail(GE_ERR_ARG, "fold: %d epochs outside [1, %d]", cfg->epochs, FOLD_MAX_EPOCHS);
    if (n_rows * cfg->epochs >= ((int64_t)1 << 31))
        return ge::fail(GE_ERR_ARG, "fold: %lld rows x %d epochs of costs are not below 2^31", (long long)n_rows, cfg->epochs);
    if (!(cfg->learning_rate == 0.0f) && !(std::isfinite(cfg->learning_rate) && cfg->learning_rate > 0.0f))
        return ge::fail(GE_ERR_ARG, "fold: learning rate %g is neither 0 (the handle's) nor finite and positive", (double)cfg->learning_rate);
    if (row_ptr[0] != 0) return ge::fail(GE_ERR_ARG, "row_ptr[0] is %lld, not 0", (long long)row_ptr[0]);
    for (int64_t r = 0; r < n_rows; ++r)
        if (row_ptr[r + 1] < row_ptr[r]) return ge::fail(GE_ERR_ARG, "row_ptr decreases at [%lld]", (long long)(r + 1));
    const int64_t nnz = row_ptr[n_rows];
    if (nnz >= ((int64_t)1 << 31)) return ge::fail(GE_ERR_ARG, "%lld nonzeros are more than one fold-in set holds (below 2^31)", (long long)nnz);
    int64_t longest = 0;
    for (int64_t r = 0; r < n_rows; ++r) {
        longest = std::max(longest, row_ptr[r + 1] - row_ptr[r]);
        for (int64_t k = row_ptr[r]; k < row_ptr[r + 1]; ++k) {
            if (idx[k] < 0) return ge::fail(GE_ERR_ARG, "row %lld: id %d out of range", (long long)r, idx[k]);
            if (!std::isfinite(X[k]) || !(X[k] > 0.0f)) return ge::fail(GE_ERR_ARG, "row %lld: value %g is not finite and positive", (long long)r, (double)X[k]);
        }
    }
    if (!h) return ge::fail(GE_ERR_ARG, "null ge_glove handle");
    ge::EvalView v;
    GE_CHECK(ge::glove_eval_view(h, &v));
    int vw, nch;
    lane_shape(v.dim, &vw, &nch);
    if (v.dim < 1 || nch > 4) return ge::fail(GE_ERR_ARG, "fold: dim %d has no lane shape (more than four chunks)", v.dim);
    const int32_t lo = cfg->side == GE_FOLD_FOCUS ? 0 : v.row_begin, hi = cfg->side == GE_FOLD_FOCUS ? v.vocab_size : v.row_end;
    for (int64_t r = 0; r < n_rows; ++r)
        for (int64_t k = row_ptr[r]; k < row_ptr[r + 1]; ++k) {
            if (idx[k] < lo || idx[k] >= hi)
                return ge::fail(GE_ERR_ARG, "row %lld: id %d outside the frozen side's rows [%d,%d)", (long long)r, idx[k], lo, hi);
            if (v.cost_kind == GE_COST_PGLOVE && !(X[k] < 1.0f))
                return ge::fail(GE_ERR_ARG, "row %lld: value %g is not inside (0, 1)", (long long)r, (double)X[k]);
        }

    // longest first: descending length, equal lengths by ascending row
    std::vector<int32_t> order((size_t)n_rows);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return row_ptr[x + 1] - row_ptr[x] > row_ptr[y + 1] - row_ptr[y]; });

    ge_fold *f = new ge_fold;
    f->glove = h; f->view = v; f->cfg = *cfg; f->n_rows = n_rows; f->nnz = nnz; f->longest = longest;
    struct Guard { ge_fold *f; ~Guard() { if (f) fold_free(f); } } guard{f};
    f->cost.resize((size_t)(n_rows * cfg->epochs));
    GE_HIP(hipSetDevice(v.device));
    const size_t R = (size_t)n_rows, N = (size_t)std::max<int64_t>(nnz, 1), D = (size_t)v.dim;
    GE_HIP(hipMalloc((void **)&f->drow_ptr, sizeof(int64_t) * (R + 1)));
    GE_HIP(hipMalloc((void **)&f->dorder, sizeof(int32_t) * R));
    GE_HIP(hipMalloc((void **)&f->didx, sizeof(int32_t) * N));
    GE_HIP(hipMalloc((void **)&f->dL, sizeof(double) * N));
    GE_HIP(hipMalloc((void **)&f->dW, sizeof(float) * N));
    GE_HIP(hipMalloc((void **)&f->dX, sizeof(float) * N));
    GE_HIP(hipMalloc((void **)&f->drows, sizeof(float) * R * D));
    GE_HIP(hipMalloc((void **)&f->dbias, sizeof(float) * R));
    GE_HIP(hipMalloc((void **)&f->dcost, sizeof(float) * R * (size_t)cfg->epochs));
    GE_HIP(hipEventCreate(&f->ev0));
    GE_HIP(hipEventCreate(&f->ev1));
    GE_HIP(hipMemcpyAsync(f->drow_ptr, row_ptr, sizeof(int64_t) * (R + 1), hipMemcpyHostToDevice, v.stream));
    GE_HIP(hipMemcpyAsync(f->dorder, order.data(), sizeof(int32_t) * R, hipMemcpyHostToDevice, v.stream));
    if (nnz > 0) {
        GE_HIP(hipMemcpyAsync(f->didx, idx, sizeof(int32_t) * (size_t)nnz, hipMemcpyHostToDevice, v.stream));
        GE_HIP(hipMemcpyAsync(f->dX, X, sizeof(float) * (size_t)nnz, hipMemcpyHostToDevice, v.stream));
        const unsigned blocks = (unsigned)std::min<int64_t>((nnz + 255) / 256, 4096);
        hipLaunchKernelGGL(k_fold_terms, dim3(blocks), dim3(256), 0, v.stream, (const float *)f->dX, nnz, (int)v.cost_kind, v.xmax, f->dL, f->dW);
        GE_HIP(hipGetLastError());
    }
    GE_HIP(hipStreamSynchronize(v.stream));      // the host arrays may go
    guard.f = nullptr;
    *out = f;
    return GE_OK;
}

ge_status fold_run_impl(ge_fold *f, const float *init_rows, const float *init_bias, float *out_rows, float *out_bias, float *out_cost,
                        double *cost_history) {
    if (!f) return ge::fail(GE_ERR_ARG, "null ge_fold handle");
    GE_CHECK(ge::glove_eval_view(f->glove, &f->view));          // read the tables where they are now
    const ge::EvalView &v = f->view;
    const int64_t R = f->n_rows;
    const int32_t D = v.dim, E = f->cfg.epochs;
    if (init_rows)
        for (int64_t k = 0; k < R * D; ++k)
            if (!std::isfinite(init_rows[k])) return ge::fail(GE_ERR_ARG, "non-finite input: init_rows[%lld]", (long long)k);
    if (init_bias)
        for (int64_t k = 0; k < R; ++k)
            if (!std::isfinite(init_bias[k])) return ge::fail(GE_ERR_ARG, "non-finite input: init_bias[%lld]", (long long)k);
    GE_HIP(hipSetDevice(v.device));
    hipStream_t stream = v.stream;
    if (init_rows) GE_HIP(hipMemcpyAsync(f->drows, init_rows, sizeof(float) * (size_t)(R * D), hipMemcpyHostToDevice, stream));
    else GE_HIP(hipMemsetAsync(f->drows, 0, sizeof(float) * (size_t)(R * D), stream));
    if (init_bias) GE_HIP(hipMemcpyAsync(f->dbias, init_bias, sizeof(float) * (size_t)R, hipMemcpyHostToDevice, stream));
    else GE_HIP(hipMemsetAsync(f->dbias, 0, sizeof(float) * (size_t)R, stream));

    const bool focus_side = f->cfg.side == GE_FOLD_FOCUS;
    FoldParams p{};
    p.table = focus_side ? v.context : v.focus;
    p.bias = focus_side ? v.cbias : v.fbias;
    p.stride = focus_side ? v.context_stride : v.focus_stride;
    p.bias_stride = focus_side ? v.cbias_stride : v.fbias_stride;
    p.base = focus_side ? 0 : v.row_begin;
    p.hub32 = focus_side && v.emb16 ? v.hub32 : nullptr;
    p.hub_index = p.hub32 ? v.hub_index : nullptr;
    p.row_ptr = f->drow_ptr; p.order = f->dorder; p.idx = f->didx; p.L = f->dL; p.W = f->dW;
    p.rows = f->drows; p.rbias = f->dbias; p.cost = f->dcost;
    p.seed = f->cfg.seed; p.n_rows = (int32_t)R; p.D = D; p.E = E; p.shuffle = f->cfg.shuffle == GE_SHUFFLE_DEVICE ? 1 : 0;
    p.lr = f->cfg.learning_rate == 0.0f ? v.learning_rate : f->cfg.learning_rate;
    int vw, nch;
    lane_shape(D, &vw, &nch);
    // The kernel reads vw floats of a row per access (bf16 rows: vw * 2 bytes).  Every layout a handle can have starts its rows on
    // such a boundary (a record is a whole number of rows of D or D + 4 elements, a padded bf16 row a multiple of 8), so the
    // narrower loads the header allows for are never needed; a table that broke the rule is refused, not read differently.
    const size_t width = (size_t)vw * (v.emb16 ? 2 : 4);
    if (p.stride % vw != 0 || !aligned_to(p.table, width) || (p.hub32 && !aligned_to(p.hub32, 16)))
        return ge::fail(GE_ERR_STATE, "fold: the frozen rows do not start on %zu-byte boundaries (stride %lld)", width, (long long)p.stride);
    const fold_fn fn = v.emb16 ? pick_nch<4, true>(nch) : vw == 4 ? pick_nch<4, false>(nch) : vw == 2 ? pick_nch<2, false>(nch) : pick_nch<1, false>(nch);
    if (!fn || (v.emb16 && vw != 4)) return ge::fail(GE_ERR_STATE, "fold: no kernel for dim %d", D);
    GE_HIP(hipEventRecord(f->ev0, stream));
    hipLaunchKernelGGL(fn, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, stream, p);
    GE_HIP(hipGetLastError());
    GE_HIP(hipEventRecord(f->ev1, stream));
    GE_HIP(hipMemcpyAsync(f->cost.data(), f->dcost, sizeof(float) * (size_t)(R * E), hipMemcpyDeviceToHost, stream));
    if (out_rows) GE_HIP(hipMemcpyAsync(out_rows, f->drows, sizeof(float) * (size_t)(R * D), hipMemcpyDeviceToHost, stream));
    if (out_bias) GE_HIP(hipMemcpyAsync(out_bias, f->dbias, sizeof(float) * (size_t)R, hipMemcpyDeviceToHost, stream));
    GE_HIP(hipStreamSynchronize(stream));
    GE_HIP(hipEventElapsedTime(&f->last_ms, f->ev0, f->ev1));
    if (out_cost) std::copy(f->cost.begin(), f->cost.end(), out_cost);
    if (cost_history)
        for (int32_t e = 0; e < E; ++e) {
            double total = 0.0;
            for (int64_t r = 0; r < R; ++r) total = total + (double)f->cost[(size_t)(r * E + e)];
            cost_history[e] = total;
        }
    return GE_OK;
}

}  // namespace

extern "C" {

void ge_fold_cfg_default(ge_fold_cfg *cfg) {
    if (!cfg) return;
    cfg->side = GE_FOLD_FOCUS; cfg->epochs = 10; cfg->shuffle = GE_SHUFFLE_DEVICE; cfg->learning_rate = 0.0f; cfg->seed = 0;
}
int32_t ge_fold_cfg_size(void) { return (int32_t)sizeof(ge_fold_cfg); }

ge_status ge_glove_fold_create(ge_glove *h, const int64_t *row_ptr, const int32_t *idx, const float *X, int64_t n_rows, const ge_fold_cfg *cfg,
                               ge_fold **out) {
    GE_GUARD(fold_create_impl(h, row_ptr, idx, X, n_rows, cfg, out));
}

ge_status ge_glove_fold_run(ge_fold *f, const float *init_rows, const float *init_bias, float *out_rows, float *out_bias, float *out_cost,
                            double *cost_history) {
    GE_GUARD(fold_run_impl(f, init_rows, init_bias, out_rows, out_bias, out_cost, cost_history));
}

ge_status ge_fold_last_kernel_ms(const ge_fold *f, float *ms) {
    if (!f || !ms) return ge::fail(GE_ERR_ARG, "null argument");
    *ms = f->last_ms;
    return GE_OK;
}

ge_status ge_fold_get(const ge_fold *f, int64_t *n_rows, int64_t *nnz, int32_t *dim, int64_t *path) {
    if (!f) return ge::fail(GE_ERR_ARG, "null ge_fold handle");
    if (n_rows) *n_rows = f->n_rows;
    if (nnz) *nnz = f->nnz;
    if (dim) *dim = f->view.dim;
    if (path) *path = (int64_t)f->cfg.epochs * f->longest;
    return GE_OK;
}

void ge_fold_destroy(ge_fold *f) { fold_free(f); }

ge_status ge_foldin_mask(uint64_t seed, int64_t n, double fraction, uint8_t *mask) {
    if (!(fraction > 0.0) || !(fraction <= 0.5)) return ge::fail(GE_ERR_ARG, "foldin fraction %g outside (0, 0.5]", fraction);
    if (n < 0 || (n > 0 && !mask)) return ge::fail(GE_ERR_ARG, "invalid n %lld or null mask", (long long)n);
    const uint64_t T = (uint64_t)std::floor(fraction * 4294967296.0);
    const uint64_t s = seed ^ 0x464F4C44494Eull;
    for (int64_t v = 0; v < n; ++v) mask[v] = (splitmix_at(s, (uint64_t)v) >> 32) < T ? 1 : 0;
    return GE_OK;
}

}  // extern "C"
