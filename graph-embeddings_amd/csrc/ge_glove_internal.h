// ge_glove_internal.h -- what the other translation units of libgeglove.so may ask of a trainer handle.  Defined in glove.hip
// (struct ge_glove is private to it); used by sync.hip, pca.hip and eval.hip.
#pragma once
#include "ge_common.h"
#include <vector>

namespace ge {

// What ge_glove_extract_f32 returns, left on the device (pca.hip fits and projects it there): (focus + context) / 2 in a fresh
// buffer of vocab_size x dim floats, complete when this returns; the caller frees it.
ge_status glove_extract_device_f32(ge_glove *h, float **rows, int32_t *vocab_size, int32_t *dim, int32_t *device);

// what sync.hip needs to know about a handle
ge_status glove_sync_view(ge_glove *h, int32_t *opt, int32_t *mode, void **stream, int32_t *device);

// A Hogwild epoch in `nseg` launches (ge_sync_epoch: the hub rows of a sharded run are reconciled between them).  The chunks of
// the epoch are handed out by ticket through a keyed bijection, so tickets [n seg / nseg, n (seg + 1) / nseg) are a random nseg-th
// of the epoch; the cost accumulates on the device over the segments.  Nothing here blocks the host: glove_epoch_finish does.
// leave_blocks: workgroups NOT launched (their wavefront slots stay free for kernels running beside the epoch: the live hub-row exchange
// of a sharded run); after_reset: recorded once the ticket counter holds this segment's first ticket (a host that watches the counter
// waits for it, so that it never reads the previous epoch's value).
ge_status glove_epoch_segment(ge_glove *h, int32_t iteration, int32_t seg, int32_t nseg, int32_t leave_blocks, hipEvent_t after_reset);
// the epoch's cost once its last segment has run (drains the stream); ge_glove_last_kernel_ms then gives the launches' own time summed
ge_status glove_epoch_finish(ge_glove *h, double *cost_sum);
// the epoch's ticket counter (device memory; tickets [0, *tickets) are the epoch's chunks) and the event behind the last launch
ge_status glove_epoch_progress(ge_glove *h, const unsigned long long **counter, int64_t *tickets, hipEvent_t *done);

// the busy columns of this handle's shard (ascending; ge_layout.h `heavy`), for the small exchanges of a sharded run
const std::vector<int32_t> *glove_hub_columns(const ge_glove *h);
// their nonzero counts (ge_layout.h `heavy_count`)
const std::vector<int32_t> *glove_hub_counts(const ge_glove *h);
// the columns this handle's epoch kernel treats as hubs (resident runs that publish the row and its accumulator row by float atomics)
const std::vector<int32_t> *glove_kernel_hubs(const ge_glove *h);

// Where eval.hip reads a handle's rows and biases, whichever layout the handle has (glove.hip `view_of`): row r of a table is
// base + r * stride elements (fp32, or bf16 when emb16), a bias is bias[r * stride].  Focus-side tables start at row_begin (NOT
// rebased: the reader subtracts it).  bf16 handles: column j's context row is hub32 + hub_index[j] * dim (fp32) when
// hub_index[j] >= 0; hub_index is null when the handle keeps no masters.  Touches no device.
struct EvalView {
    const void *focus, *context;
    const float *fbias, *cbias, *hub32;
    const int32_t *hub_index;
    int64_t focus_stride, context_stride, fbias_stride, cbias_stride;
    double xmax;
    int32_t vocab_size, dim, row_begin, row_end, cost_kind, emb16, device;
    hipStream_t stream;
    float learning_rate;                 // cfg.learning_rate (fold.hip: the default step of a fold-in)
};
ge_status glove_eval_view(const ge_glove *h, EvalView *out);

}  // namespace ge
