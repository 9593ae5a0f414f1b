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
    void release();
};

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

}  // namespace ge
