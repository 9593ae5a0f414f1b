// strata.hip -- GE_MODE_STRATIFIED: the bit-exact update (ge_exact.h) run by P wavefronts at once, without a race.
//
// The rows are cut into P blocks and the columns into P blocks, both balanced by nonzero count (include/geglove.h states the
// rule).  In sub-epoch s worker a walks tile (a, (a + s) mod P): the P tiles of a sub-epoch share no focus row and no context
// row, so they touch disjoint table rows and the result is, bit for bit, what one wavefront gives that walks the same tiles one
// after another (ge_glove_epoch_order) -- the oracle replays exactly that.  Kernel boundaries are the only synchronisation
// between sub-epochs: no grid barrier, no cooperative launch, no kernel ever waits for another workgroup.
//
// The layout (two histograms, two scans, a stable counting sort of the nonzeros by tile) is built on the HOST, once per handle:
// it is O(N + V + P^2) of plain loops over arrays the host already holds, paid at create time.
// Compiled with -ffp-contract=off like every user of ge_exact.h.
// A handle whose arithmetic is GE_ARITH_FP32 launches k_strata_fp32 (strata_fp32.hip) on the same schedule instead.
#include "ge_strata.h"

#include <algorithm>
#include <cstring>

namespace ge {
namespace {

// One wavefront per tile: workgroup a of sub-epoch `sub` walks tile (a, (a + sub) mod P) in order and writes its fp32 cost.
// LDS: dim floats (the product row of exact_update).  An empty tile returns at once (its cost stays the 0 of create time).
__global__ __launch_bounds__(64) void k_adagrad_strata(ExactParams p, const int32_t *__restrict__ sI, const int32_t *__restrict__ sJ,
                                                       const float *__restrict__ sX, const int32_t *__restrict__ toff, float *tile_cost,
                                                       int32_t P, int32_t sub, int64_t seed, int32_t iteration, int32_t shuffle) {
    extern __shared__ float s_prod[];
    const int lane = threadIdx.x;
    const int32_t a = blockIdx.x;
    int32_t b = a + sub;
    if (b >= P) b -= P;
    const int32_t tile = a * P + b;                     // P <= 2048: below 2^22
    const int32_t begin = toff[tile];
    const uint32_t n = (uint32_t)(toff[tile + 1] - begin);
    if (n == 0) return;                                 // the whole workgroup: no barrier is left behind
    uint32_t mask = 0, shift = 1, key[4] = {0, 0, 0, 0};
    if (shuffle) { strata_width(n, &mask, &shift); strata_keys(seed, iteration, (uint32_t)tile + 1u, key); }
    float cost = 0.0f;
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t pos = shuffle ? strata_walk(k, n, mask, shift, key) : k;      // < n: inside the tile
        const int64_t idx = (int64_t)begin + pos;
        exact_update(p, sI[idx], sJ[idx], sX[idx], s_prod, lane, cost);
    }
    if (lane == 0) tile_cost[tile] = cost;
}

// the order of the sub-epochs of epoch `iteration`
void sub_epoch_order(int32_t P, int64_t seed, int32_t iteration, bool shuffle, std::vector<int32_t> *out) {
    out->resize((size_t)P);
    uint32_t mask = 0, shift = 1, key[4] = {0, 0, 0, 0};
    if (shuffle) { strata_width((uint32_t)P, &mask, &shift); strata_keys(seed, iteration, 0u, key); }
    for (int32_t t = 0; t < P; ++t) (*out)[(size_t)t] = shuffle ? (int32_t)strata_walk((uint32_t)t, (uint32_t)P, mask, shift, key) : t;
}

}  // namespace

void Strata::release() {
    for (void *q : {(void *)dI, (void *)dJ, (void *)dX, (void *)dtoff, (void *)dcost, (void *)dL, (void *)dW}) if (q) (void)hipFree(q);
    dI = dJ = dtoff = nullptr; dX = dcost = dW = nullptr; dL = nullptr;
}

// The sweep of profiles/strata_bench.json: the epoch is shortest where a tile holds a handful of nonzeros (fewer blocks leave
// wavefronts idle, more only add launches and empty tiles), so P = the largest power of two with 8 P^2 <= nnz, at most the
// owned rows and at most 2048.
int32_t strata_default_p(int32_t rows, int64_t nnz) {
    int32_t P = 1;
    while (P < 2048 && 2 * P <= rows && 8ll * (2 * P) * (2 * P) <= nnz) P *= 2;
    return P;
}

void strata_layout(Strata *st, int32_t P, int32_t V, int64_t N, const int32_t *I, const int32_t *J, const float *X,
                   std::vector<int32_t> &sI, std::vector<int32_t> &sJ, std::vector<float> &sX) {
    st->P = P;
    const size_t tiles = (size_t)P * (size_t)P;
    st->toff.assign(tiles + 1, 0);
    st->src.resize((size_t)N);
    st->sub_used.assign((size_t)P, 0);
    st->host_cost.assign(tiles, 0.0f);
    st->path = 0;
    sI.resize((size_t)N); sJ.resize((size_t)N); sX.resize((size_t)N);
    if (N > 0) {
        // r(i), c(j): nonzeros in rows below i / in columns below j
        std::vector<int64_t> r((size_t)V + 1, 0), c((size_t)V + 1, 0);
        for (int64_t k = 0; k < N; ++k) { ++r[(size_t)I[k] + 1]; ++c[(size_t)J[k] + 1]; }
        for (int32_t v = 0; v < V; ++v) { r[(size_t)v + 1] += r[(size_t)v]; c[(size_t)v + 1] += c[(size_t)v]; }
        std::vector<int32_t> rb((size_t)V), cb((size_t)V);
        for (int32_t v = 0; v < V; ++v) {               // r(v) < N wherever row v holds a nonzero, so its block is < P
            rb[(size_t)v] = (int32_t)std::min<int64_t>(r[(size_t)v] * P / N, P - 1);
            cb[(size_t)v] = (int32_t)std::min<int64_t>(c[(size_t)v] * P / N, P - 1);
        }
        for (int64_t k = 0; k < N; ++k) ++st->toff[(size_t)rb[(size_t)I[k]] * P + (size_t)cb[(size_t)J[k]] + 1];
        for (size_t t = 0; t < tiles; ++t) st->toff[t + 1] += st->toff[t];
        std::vector<int32_t> fill(st->toff.begin(), st->toff.end() - 1);
        for (int64_t k = 0; k < N; ++k) {               // ascending k: matrix order inside a tile
            const int32_t at = fill[(size_t)rb[(size_t)I[k]] * P + (size_t)cb[(size_t)J[k]]]++;
            st->src[(size_t)at] = (int32_t)k; sI[(size_t)at] = I[k]; sJ[(size_t)at] = J[k]; sX[(size_t)at] = X[k];
        }
        for (int32_t s = 0; s < P; ++s) {
            int32_t longest = 0;
            for (int32_t a = 0; a < P; ++a) {
                const size_t t = (size_t)a * P + (size_t)((a + s) % P);
                longest = std::max(longest, st->toff[t + 1] - st->toff[t]);
            }
            st->path += longest;
            st->sub_used[(size_t)s] = longest > 0;
        }
    }
}

ge_status strata_build(Strata *st, int32_t P, int32_t V, int64_t N, const int32_t *I, const int32_t *J, const float *X, hipStream_t stream) {
    std::vector<int32_t> sI, sJ;
    std::vector<float> sX;
    strata_layout(st, P, V, N, I, J, X, sI, sJ, sX);
    const size_t tiles = (size_t)P * (size_t)P;
    const size_t nn = (size_t)std::max<int64_t>(N, 1);
    GE_HIP(hipMalloc((void **)&st->dI, sizeof(int32_t) * nn));
    GE_HIP(hipMalloc((void **)&st->dJ, sizeof(int32_t) * nn));
    GE_HIP(hipMalloc((void **)&st->dX, sizeof(float) * nn));
    GE_HIP(hipMalloc((void **)&st->dtoff, sizeof(int32_t) * (tiles + 1)));
    GE_HIP(hipMalloc((void **)&st->dcost, sizeof(float) * tiles));
    if (N > 0) {
        GE_HIP(hipMemcpyAsync(st->dI, sI.data(), sizeof(int32_t) * (size_t)N, hipMemcpyHostToDevice, stream));
        GE_HIP(hipMemcpyAsync(st->dJ, sJ.data(), sizeof(int32_t) * (size_t)N, hipMemcpyHostToDevice, stream));
        GE_HIP(hipMemcpyAsync(st->dX, sX.data(), sizeof(float) * (size_t)N, hipMemcpyHostToDevice, stream));
    }
    GE_HIP(hipMemcpyAsync(st->dtoff, st->toff.data(), sizeof(int32_t) * (tiles + 1), hipMemcpyHostToDevice, stream));
    GE_HIP(hipMemsetAsync(st->dcost, 0, sizeof(float) * tiles, stream));      // a tile that holds nonzeros overwrites its cost every epoch
    GE_HIP(hipStreamSynchronize(stream));                                     // the staging vectors go out of scope
    return GE_OK;
}

ge_status strata_epoch(Strata *st, const ExactParams &p, int64_t seed, int32_t iteration, bool shuffle, hipStream_t stream,
                       hipEvent_t ev0, hipEvent_t ev1, int32_t *launches, double *cost_sum) {
    const int32_t P = st->P;
    std::vector<int32_t> subs;
    sub_epoch_order(P, seed, iteration, shuffle, &subs);
    *launches = 0;
    GE_HIP(hipEventRecord(ev0, stream));
    for (int32_t t = 0; t < P; ++t) {
        const int32_t s = subs[(size_t)t];
        if (!st->sub_used[(size_t)s]) continue;         // all P tiles empty: not launched
        if (st->arith == GE_ARITH_FP32) {
            strata_fp32_launch(st, p, s, seed, iteration, shuffle, stream);
        } else {
            hipLaunchKernelGGL(k_adagrad_strata, dim3((unsigned)P), dim3(64), sizeof(float) * (size_t)p.D, stream,
                               p, (const int32_t *)st->dI, (const int32_t *)st->dJ, (const float *)st->dX, (const int32_t *)st->dtoff, st->dcost,
                               P, s, seed, iteration, shuffle ? 1 : 0);
        }
        ++*launches;
    }
    GE_HIP(hipEventRecord(ev1, stream));
    GE_HIP(hipGetLastError());
    double total = 0.0;
    if (*launches > 0) {
        GE_HIP(hipMemcpyAsync(st->host_cost.data(), st->dcost, sizeof(float) * st->host_cost.size(), hipMemcpyDeviceToHost, stream));
        GE_HIP(hipStreamSynchronize(stream));
        for (int32_t t = 0; t < P; ++t) {               // every tile is a job: localCost += job result, in epoch order
            const int32_t s = subs[(size_t)t];
            if (!st->sub_used[(size_t)s]) continue;
            for (int32_t a = 0; a < P; ++a) total += (double)st->host_cost[(size_t)a * P + (size_t)((a + s) % P)];
        }
    } else {
        GE_HIP(hipStreamSynchronize(stream));
    }
    *cost_sum = total;
    return GE_OK;
}

void strata_order(const Strata *st, int64_t seed, int32_t iteration, bool shuffle, int32_t *out) {
    const int32_t P = st->P;
    std::vector<int32_t> subs;
    sub_epoch_order(P, seed, iteration, shuffle, &subs);
    int64_t w = 0;
    for (int32_t t = 0; t < P; ++t) {
        const int32_t s = subs[(size_t)t];
        for (int32_t a = 0; a < P; ++a) {
            const int32_t tile = a * P + (a + s) % P;
            const int32_t begin = st->toff[(size_t)tile];
            const uint32_t n = (uint32_t)(st->toff[(size_t)tile + 1] - begin);
            if (n == 0) continue;
            uint32_t mask = 0, shift = 1, key[4] = {0, 0, 0, 0};
            if (shuffle) { strata_width(n, &mask, &shift); strata_keys(seed, iteration, (uint32_t)tile + 1u, key); }
            for (uint32_t k = 0; k < n; ++k)
                out[w++] = st->src[(size_t)begin + (shuffle ? strata_walk(k, n, mask, shift, key) : k)];
        }
    }
}

}  // namespace ge
