// strata_fp32.hip -- GE_ARITH_FP32: the stratified schedule (strata.hip) with an fp32, wave-reduced update in place of ge_exact.h's.
//
// Same tiles, same sub-epochs, same walks, one wavefront per tile, updates inside a tile strictly one after another: only the
// arithmetic of one update differs, and include/geglove.h states it operation for operation (tests/strata_fp32_ref.py restates it
// in numpy).  What the kernel adds is latency hiding that the arithmetic leaves room for:
//   rows in registers   a lane holds vw * nch floats of each row (k_adagrad_runs' lane shape); the dot product is a per-lane fma
//                       chain and wave_sum.  No LDS, no barrier.
//   prefetch            the rows and the bias scalars of nonzero k + 1 are requested before nonzero k is computed and stored, and
//                       its index and (l, w) one nonzero earlier still, so the two dependent memory round trips of an update (where
//                       is it, then its rows) overlap each other and the update before.
//   forwarding          where k + 1 names the same focus (context) row as k, that side stays in registers: no load, and no store
//                       until the row changes.
// A row that k - 1 stored and k + 1 loads again is ordered by program order alone: every element is loaded and stored by the same
// lane at the same address (one lane mapping for both, rows and bias scalars alike), and a wavefront's accesses to one address
// complete in the order it issued them.  Between tiles of different sub-epochs the kernel boundary orders everything.
// Compiled with -ffp-contract=off: the fused multiply-adds are the explicit ones.
#include "ge_strata.h"
#include "ge_wave.h"

#include <cstdlib>

namespace ge {
namespace {

// (l, w) of every tile-sorted nonzero: X never changes, so the fp64 log / pow of the exact mode run once per handle.
__global__ void k_strata_terms(const float *__restrict__ X, int64_t n, int kind, double xmax, double *__restrict__ L, float *__restrict__ W) {
    int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; k < n; k += stride) {
        double l; float w;
        cost_terms<true>(kind, X[k], xmax, l, w);
        L[k] = l; W[k] = w;
    }
}

constexpr int WAIT_MEMORY = 0x0070;      // s_waitcnt immediate (gfx9 layout): vmcnt(0) lgkmcnt(0), no vector or scalar memory instruction outstanding
enum { ABLATE_NONE = 0, ABLATE_PREFETCH = 1, ABLATE_PREFETCH_AND_FORWARDING = 2 };

// One side of an update in registers: the parameter row, its accumulator row (gradSq | M1) and, with moments, M2.
template <int VW, int NCH> struct RowRegs { typename Vec<VW>::T r[NCH], g[NCH], h[NCH]; };

// One wavefront per tile, as k_adagrad_strata: workgroup a of sub-epoch `sub` walks tile (a, (a + sub) mod P).
// At most 256 VGPRs (two waves per SIMD), so that 2048 tiles are resident at once.
// ABLATE: what the measuring tool switches off (a compile-time choice, so that the paths it removes leave no wait behind).
template <int VW, int NCH, int OPT, int ABLATE>
__global__ __launch_bounds__(64, 2) void k_strata_fp32(ExactParams p, const int32_t *__restrict__ sI, const int32_t *__restrict__ sJ,
                                                       const double *__restrict__ sL, const float *__restrict__ sW,
                                                       const int32_t *__restrict__ toff, float *tile_cost,
                                                       int32_t P, int32_t sub, int64_t seed, int32_t iteration, int32_t shuffle) {
    using Regs = RowRegs<VW, NCH>;
    constexpr bool MOM = OPT != GE_OPT_ADAGRAD;
    constexpr int NB = MOM ? 6 : 4;                     // bias scalars of an update: lane b holds scalar b
    const int lane = threadIdx.x;
    const int32_t a = blockIdx.x;
    int32_t b = a + sub;
    if (b >= P) b -= P;
    const int32_t tile = a * P + b;                     // P <= 2048: below 2^22
    const int32_t begin = toff[tile];
    const uint32_t n = (uint32_t)(toff[tile + 1] - begin);
    if (n == 0) return;
    uint32_t mask = 0, shift = 1, key[4] = {0, 0, 0, 0};
    if (shuffle) { strata_width(n, &mask, &shift); strata_keys(seed, iteration, (uint32_t)tile + 1u, key); }

    const int32_t D = p.D;
    const uint32_t row_bytes = (uint32_t)D * 4u;        // the buffer resource of a row ends with the row: lanes past it read 0 and store nothing
    const bool in_last = (lane + 64 * (NCH - 1)) * VW < D;      // only the last chunk can be partial (D % VW == 0: a vector is inside or outside)
    const float lr = p.lr;
    constexpr float BETA1 = 0.9f, BETA2 = 0.999f, EPS = 1e-7f, OMB1 = 1 - BETA1, OMB2 = 1 - BETA2;   // Adam.java:45-53
    const float corr = OPT == GE_OPT_ADAM ? (float)p.correction : lr;      // Adam.java:84 | AMSGrad.java:133 uses lr itself
    // glove.hip's moment_step, restated: one element of an Adam / AMSGrad update in fp32, IEEE operations only
    auto moment_step = [&](float grad, float &m, float &v) -> float {
        m = __builtin_fmaf(BETA1, m, OMB1 * grad);
        const float vn = __builtin_fmaf(BETA2, v, OMB2 * (grad * grad));
        v = OPT == GE_OPT_AMSGRAD ? fmaxf(v, vn) : vn;
        return corr * m * (1.0f / (__builtin_sqrtf(v) + EPS));
    };

    auto load_side = [&](Regs &s, const float *row, const float *acc, const float *m2, int32_t id) {
        const __amdgpu_buffer_rsrc_t rr = make_rsrc(row + (int64_t)id * D, row_bytes);
        const __amdgpu_buffer_rsrc_t rg = make_rsrc(acc + (int64_t)id * D, row_bytes);
#pragma unroll
        for (int q = 0; q < NCH; ++q) {
            s.r[q] = buf_load<VW, AUX_SC1>(rr, (lane + q * 64) * VW * 4);
            s.g[q] = buf_load<VW, AUX_SC1>(rg, (lane + q * 64) * VW * 4);
        }
        if constexpr (MOM) {
            const __amdgpu_buffer_rsrc_t rh = make_rsrc(m2 + (int64_t)id * D, row_bytes);
#pragma unroll
            for (int q = 0; q < NCH; ++q) s.h[q] = buf_load<VW, AUX_SC1>(rh, (lane + q * 64) * VW * 4);
        }
    };
    auto store_side = [&](Regs &s, float *row, float *acc, float *m2, int32_t id) {
        const __amdgpu_buffer_rsrc_t rr = make_rsrc(row + (int64_t)id * D, row_bytes);
        const __amdgpu_buffer_rsrc_t rg = make_rsrc(acc + (int64_t)id * D, row_bytes);
#pragma unroll
        for (int q = 0; q < NCH; ++q) {
            buf_store<VW>(s.r[q], rr, (lane + q * 64) * VW * 4);
            buf_store<VW>(s.g[q], rg, (lane + q * 64) * VW * 4);
        }
        if constexpr (MOM) {
            const __amdgpu_buffer_rsrc_t rh = make_rsrc(m2 + (int64_t)id * D, row_bytes);
#pragma unroll
            for (int q = 0; q < NCH; ++q) buf_store<VW>(s.h[q], rh, (lane + q * 64) * VW * 4);
        }
    };
    // lane b's scalar of update (i, j): fbias[i], cbias[j], their accumulators, then their second moments; even lanes are the focus side
    auto bias_ptr = [&](int32_t i, int32_t j) -> float * {
        float *q = p.fbias + i;
        if (lane == 1) q = p.cbias + j;
        if (lane == 2) q = p.gsfb + i;
        if (lane == 3) q = p.gscb + j;
        if constexpr (MOM) {
            if (lane == 4) q = p.m2fb + i;
            if (lane == 5) q = p.m2cb + j;
        }
        return q;
    };
    auto bcast = [&](float v, int l) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l)); };
    auto position = [&](uint32_t k) -> int64_t {
        return (int64_t)begin + (shuffle ? strata_walk(k, n, mask, shift, key) : k);      // < n: inside the tile
    };

    constexpr bool prefetch = ABLATE == ABLATE_NONE, forwarding = ABLATE != ABLATE_PREFETCH_AND_FORWARDING;
    Regs F, C, nF, nC;
    float bs = 0.0f, nbs = 0.0f;                        // lane < NB: its bias scalar
    int64_t idx = position(0);
    int32_t i = rfl(sI[idx]), j = rfl(sJ[idx]);
    double l = sL[idx];
    float w = sW[idx];
    load_side(F, p.focus, p.gsf, p.m2f, i);
    load_side(C, p.context, p.gsc, p.m2c, j);
    if (lane < NB) bs = *bias_ptr(i, j);
    // (ni, nj, nl, nw): nonzero k + 1.  With the prefetch it is read one nonzero earlier still (its position is random under
    // shuffle: device, a memory round trip of its own), so that the rows of k + 1 can be requested at the top of k.
    int32_t ni = i, nj = j, ai = i, aj = j;
    double nl = l, al = l;
    float nw = w, aw = w;
    if (prefetch && n > 1) {
        idx = position(1);
        ni = rfl(sI[idx]); nj = rfl(sJ[idx]);
        nl = sL[idx]; nw = sW[idx];
    }
    __builtin_amdgcn_s_waitcnt(WAIT_MEMORY);            // nothing in flight at the loop's head: its waits then cover only what the loop issued
    float cost = 0.0f;
    for (uint32_t k = 0; k < n; ++k) {
        const bool has_next = k + 1 < n;
        if (!prefetch && has_next) {
            idx = position(k + 1);
            ni = rfl(sI[idx]); nj = rfl(sJ[idx]);
            nl = sL[idx]; nw = sW[idx];
        }
        if (prefetch && k + 2 < n) {                    // used when k ends
            idx = position(k + 2);
            ai = sI[idx]; aj = sJ[idx];
            al = sL[idx]; aw = sW[idx];
        }
        const bool same_f = has_next && forwarding && ni == i, same_c = has_next && forwarding && nj == j;
        const bool mine_same = (lane & 1) ? same_c : same_f;
        // what k + 1 needs and k does not leave in registers
        auto request = [&]() {
            if (has_next && !same_f) load_side(nF, p.focus, p.gsf, p.m2f, ni);
            if (has_next && !same_c) load_side(nC, p.context, p.gsc, p.m2c, nj);
            if (has_next && lane < NB && !mine_same) nbs = *bias_ptr(ni, nj);
        };
        if (prefetch) request();

        float part = 0.0f;
#pragma unroll
        for (int q = 0; q < NCH; ++q)
#pragma unroll
            for (int t = 0; t < VW; ++t) part = __builtin_fmaf(comp<VW>(F.r[q], t), comp<VW>(C.r[q], t), part);
        const float dot = wave_sum(part);
        float fb = bcast(bs, 0), cb = bcast(bs, 1), gfb = bcast(bs, 2), gcb = bcast(bs, 3);
        const float ic = (float)((double)dot + ((double)(fb + cb) - l));
        const float wc = w * ic;
        cost = (float)((double)cost + (0.5 * (double)wc) * (double)ic);
#pragma unroll
        for (int q = 0; q < NCH; ++q) {
#pragma unroll
            for (int t = 0; t < VW; ++t) {
                const float av = comp<VW>(F.r[q], t), bv = comp<VW>(C.r[q], t);
                const float g1 = wc * bv, g2 = wc * av;
                float na, nb;
                if constexpr (MOM) {
                    na = av - moment_step(g1, comp<VW>(F.g[q], t), comp<VW>(F.h[q], t));
                    nb = bv - moment_step(g2, comp<VW>(C.g[q], t), comp<VW>(C.h[q], t));
                } else {
                    float &ga = comp<VW>(F.g[q], t), &gb = comp<VW>(C.g[q], t);
                    na = av - (g1 / __builtin_sqrtf(ga)) * lr;
                    nb = bv - (g2 / __builtin_sqrtf(gb)) * lr;
                    ga = ga + g1 * g1;
                    gb = gb + g2 * g2;
                }
                // a lane past the row keeps 0 there (its accumulator reads 0, and 0 / sqrtf(0) is no number): a forwarded row feeds the next dot
                if (q == NCH - 1 && !in_last) { na = 0.0f; nb = 0.0f; }
                comp<VW>(F.r[q], t) = na;
                comp<VW>(C.r[q], t) = nb;
            }
        }
        float mine;
        if constexpr (MOM) {
            float hfb = bcast(bs, 4), hcb = bcast(bs, 5);
            fb = fb - moment_step(wc, gfb, hfb);
            cb = cb - moment_step(wc, gcb, hcb);
            mine = lane == 0 ? fb : lane == 1 ? cb : lane == 2 ? gfb : lane == 3 ? gcb : lane == 4 ? hfb : hcb;
        } else {
            fb = fb - wc / __builtin_sqrtf(gfb);
            cb = cb - wc / __builtin_sqrtf(gcb);
            gfb = gfb + wc * wc;
            gcb = gcb + wc * wc;
            mine = lane == 0 ? fb : lane == 1 ? cb : lane == 2 ? gfb : gcb;
        }
        // a side that k + 1 takes from these registers is not stored yet
        if (!same_f) store_side(F, p.focus, p.gsf, p.m2f, i);
        if (!same_c) store_side(C, p.context, p.gsc, p.m2c, j);
        if (lane < NB && !mine_same) *bias_ptr(i, j) = mine;
        if (!prefetch) request();
        if (has_next && !same_f) F = nF;
        if (has_next && !same_c) C = nC;
        bs = mine_same ? mine : nbs;
        i = ni; j = nj; l = nl; w = nw;
        if (prefetch) { ni = rfl(ai); nj = rfl(aj); nl = al; nw = aw; }
    }
    if (lane == 0) tile_cost[tile] = cost;
}

using fp32_fn = void (*)(ExactParams, const int32_t *, const int32_t *, const double *, const float *, const int32_t *, float *,
                         int32_t, int32_t, int64_t, int32_t, int32_t);
template <int VW, int OPT, int ABLATE> fp32_fn pick_nch(int nch) {
    switch (nch) {
        case 1: return k_strata_fp32<VW, 1, OPT, ABLATE>;
        case 2: return k_strata_fp32<VW, 2, OPT, ABLATE>;
        case 3: return k_strata_fp32<VW, 3, OPT, ABLATE>;
        case 4: return k_strata_fp32<VW, 4, OPT, ABLATE>;
    }
    return nullptr;
}
template <int OPT, int ABLATE = ABLATE_NONE> fp32_fn pick_vw(int vw, int nch) {
    return vw == 4 ? pick_nch<4, OPT, ABLATE>(nch) : vw == 2 ? pick_nch<2, OPT, ABLATE>(nch) : pick_nch<1, OPT, ABLATE>(nch);
}
// the Hogwild lane shape (glove.hip pick_hogwild): vw floats per lane, nch chunks of 64 lanes
void lane_shape(int32_t D, int *vw, int *nch) {
    *vw = D % 4 == 0 ? 4 : D % 2 == 0 ? 2 : 1;
    *nch = (D + 64 * *vw - 1) / (64 * *vw);
}

}  // namespace

bool strata_fp32_has_shape(int32_t dim) {
    int vw, nch;
    lane_shape(dim, &vw, &nch);
    return dim >= 1 && nch <= 4;
}

ge_status strata_fp32_prepare(Strata *st, int32_t cost_kind, double xmax, hipStream_t stream) {
    if (st->dL) return GE_OK;
    const int64_t N = (int64_t)st->src.size();
    const size_t nn = (size_t)std::max<int64_t>(N, 1);
    GE_HIP(hipMalloc((void **)&st->dL, sizeof(double) * nn));
    GE_HIP(hipMalloc((void **)&st->dW, sizeof(float) * nn));
    if (N > 0) {
        const unsigned blocks = (unsigned)std::min<int64_t>((N + 255) / 256, 4096);
        hipLaunchKernelGGL(k_strata_terms, dim3(blocks), dim3(256), 0, stream, (const float *)st->dX, N, (int)cost_kind, xmax, st->dL, st->dW);
        GE_HIP(hipGetLastError());
    }
    GE_HIP(hipStreamSynchronize(stream));
    return GE_OK;
}

void strata_fp32_launch(const Strata *st, const ExactParams &p, int32_t sub, int64_t seed, int32_t iteration, bool shuffle, hipStream_t stream) {
    int vw, nch;
    lane_shape(p.D, &vw, &nch);
    // GE_STRATA_FP32_ABLATE = 1: no prefetch; 2: no prefetch and no forwarding (AdaGrad instances only).  Same bytes either way:
    // tests/tools/strata_fp32_bench.py measures what each pays.
    const char *env = std::getenv("GE_STRATA_FP32_ABLATE");
    const int32_t ablate = env ? (int32_t)std::atoi(env) : ABLATE_NONE;
    const fp32_fn fn = p.opt == GE_OPT_ADAM    ? pick_vw<GE_OPT_ADAM>(vw, nch)
                     : p.opt == GE_OPT_AMSGRAD ? pick_vw<GE_OPT_AMSGRAD>(vw, nch)
                     : ablate == ABLATE_PREFETCH ? pick_vw<GE_OPT_ADAGRAD, ABLATE_PREFETCH>(vw, nch)
                     : ablate == ABLATE_PREFETCH_AND_FORWARDING ? pick_vw<GE_OPT_ADAGRAD, ABLATE_PREFETCH_AND_FORWARDING>(vw, nch)
                     : pick_vw<GE_OPT_ADAGRAD>(vw, nch);
    hipLaunchKernelGGL(fn, dim3((unsigned)st->P), dim3(64), 0, stream, p, (const int32_t *)st->dI, (const int32_t *)st->dJ,
                       (const double *)st->dL, (const float *)st->dW, (const int32_t *)st->dtoff, st->dcost,
                       st->P, sub, seed, iteration, shuffle ? 1 : 0);
}

}  // namespace ge
