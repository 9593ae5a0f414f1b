// ge_strata.h -- the stratified schedule of GE_MODE_STRATIFIED (include/geglove.h states its semantics): built once per handle
// (strata.hip), launched by glove.hip's epoch.
#pragma once
#include "ge_common.h"
#include "ge_exact.h"
#include <vector>

namespace ge {

struct Strata {
    int32_t P = 0;
    int64_t path = 0;                    // sum over sub-epochs of the largest tile: the schedule's length in sequential updates
    // host side: the layout as built (tile offsets, the caller's index of every sorted position) -- epoch_order and the cost sum read it
    std::vector<int32_t> toff;           // [P*P + 1]
    std::vector<int32_t> src;            // [N]
    std::vector<uint8_t> sub_used;       // [P]: sub-epoch s has a nonzero
    // device side: the nonzeros sorted by tile (stable: matrix order inside a tile), the tile offsets, one fp32 cost per tile
    int32_t *dI = nullptr, *dJ = nullptr, *dtoff = nullptr;
    float *dX = nullptr, *dcost = nullptr;
    std::vector<float> host_cost;        // [P*P], the epoch's tile costs copied back
    // GE_ARITH_FP32 (strata_fp32.hip): which arithmetic the epoch runs, and the cost terms (l, w) of every sorted nonzero, 12 bytes
    // each, computed on the first switch to fp32 (strata_fp32_prepare)
    int32_t arith = GE_ARITH_JAVA;
    double *dL = nullptr;
    float *dW = nullptr;
    void release();
};

// SplitMix64 of (seed, iteration, salt) -> four round keys of bij_mix.  salt 0: the sub-epoch order; tile id + 1: that tile's walk.
// (salt 0 gives the keys of the DETERMINISTIC mode's nonzero bijection, glove.hip bijection_keys.)
__host__ __device__ __forceinline__ void strata_keys(int64_t seed, int32_t iteration, uint32_t salt, uint32_t key[4]) {
    uint64_t z = (uint64_t)seed * 0x9E3779B97F4A7C15ULL + (uint64_t)(uint32_t)iteration * 0xD1B54A32D192ED03ULL + 0x632BE59BD9B4E019ULL
               + (uint64_t)salt * 0xA0761D6478BD642FULL;
    for (int q = 0; q < 4; ++q) {
        z += 0x9E3779B97F4A7C15ULL;
        uint64_t t = z;
        t = (t ^ (t >> 30)) * 0xBF58476D1CE4E5B9ULL;
        t = (t ^ (t >> 27)) * 0x94D049BB133111EBULL;
        t ^= t >> 31;
        key[q] = (uint32_t)t;
    }
}
// the bijection permutes [0, 2^bits), the smallest power of two that covers n (n >= 1)
__host__ __device__ __forceinline__ void strata_width(uint32_t n, uint32_t *mask, uint32_t *shift) {
    uint32_t bits = 0;
    while (bits < 31 && (1u << bits) < n) ++bits;
    *mask = (1u << bits) - 1u;
    *shift = bits > 1 ? bits / 2 : 1;
}
// position x of a keyed bijection of [0, n), cycle-walked (2^bits < 2n: fewer than two rounds expected)
__host__ __device__ __forceinline__ uint32_t strata_walk(uint32_t x, uint32_t n, uint32_t mask, uint32_t shift, const uint32_t key[4]) {
    do { x = bij_mix(x, mask, shift, key); } while (x >= n);
    return x;
}

// cfg.strata == 0: the P a handle of `rows` owned rows and `nnz` nonzeros gets (a function of these two alone)
int32_t strata_default_p(int32_t rows, int64_t nnz);

// The host half of strata_build: partition, stable sort by tile (sI, sJ, sX: the sorted nonzeros), path.  No device call.
void strata_layout(Strata *st, int32_t P, int32_t V, int64_t N, const int32_t *I, const int32_t *J, const float *X,
                   std::vector<int32_t> &sI, std::vector<int32_t> &sJ, std::vector<float> &sX);
// Partition, stable sort by tile, path; uploads on `stream` and drains it.  I, J, X: host arrays, already range-checked.
ge_status strata_build(Strata *st, int32_t P, int32_t V, int64_t N, const int32_t *I, const int32_t *J, const float *X, hipStream_t stream);

// One epoch: at most P launches on `stream` (none between ev0 and ev1 but these), the tile costs summed in epoch order.
// Returns with the stream drained; *launches = kernels launched.
ge_status strata_epoch(Strata *st, const ExactParams &p, int64_t seed, int32_t iteration, bool shuffle, hipStream_t stream,
                       hipEvent_t ev0, hipEvent_t ev1, int32_t *launches, double *cost_sum);

// out[k] = the caller's index of the k-th update of epoch `iteration` when the tiles run one after another: sub-epochs in their
// order, inside a sub-epoch a ascending, inside a tile its walk.
void strata_order(const Strata *st, int64_t seed, int32_t iteration, bool shuffle, int32_t *out);

// ---- GE_ARITH_FP32 (strata_fp32.hip; include/geglove.h states the arithmetic) ----
// a row of `dim` floats has a lane shape (vw * nch floats per lane, nch <= 4)
bool strata_fp32_has_shape(int32_t dim);
// (l, w) = cost_terms<true> of every sorted nonzero, once per handle: allocates and fills dL / dW on `stream` and drains it
ge_status strata_fp32_prepare(Strata *st, int32_t cost_kind, double xmax, hipStream_t stream);
// one sub-epoch: k_strata_fp32 in place of k_adagrad_strata, same grid (P workgroups of one wavefront)
void strata_fp32_launch(const Strata *st, const ExactParams &p, int32_t sub, int64_t seed, int32_t iteration, bool shuffle, hipStream_t stream);

}  // namespace ge
