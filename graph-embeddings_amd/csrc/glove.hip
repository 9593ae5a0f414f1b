// glove.hip -- GloVe / pGloVe AdaGrad trainer for MI355X (gfx950): kernels + C ABI.
//
// Reference semantics (J/ = src/main/java/org/uu/nl/embedding/ of Phaken/graph-embeddings):
//   Optimizer ctor           J/opt/Optimizer.java:34-64     -> k_init_java / k_fill_rows
//   Adagrad.createJob        J/opt/grad/Adagrad.java:42-98  -> k_adagrad_exact (bit-exact) / k_adagrad_runs (Hogwild)
//   GloveCost / PGloveCost   J/opt/GloveCost.java:7-20, J/opt/PGloveCost.java:7-20 -> cost_terms()
//   Optimizer.extractResult  J/opt/Optimizer.java:129-140   -> k_extract
//
// This file is compiled with -ffp-contract=off: the exact kernel must not fuse a*b+c
// (Java never does); the Hogwild kernel asks for FMAs explicitly where it wants them.
//
// Roofline: HBM.  SURVEY.md 8(d) counts read 16*D+28 / write 16*D+16 bytes per pair-update (both row pairs through HBM);
// k_adagrad_runs keeps one pair in registers per run and has to move 20 + 4 * row bytes per nonzero + 4 * row bytes per
// run (ge_glove_info.schedule_bytes).  No MFMA: sparse gather + length-D dot.

#include "ge_common.h"
#include "ge_coo.h"
#include "ge_glove_internal.h"
#include "ge_javarand.h"
#include "ge_cost.h"
#include "ge_exact.h"
#include "ge_strata.h"
#include "ge_wave.h"
#include "ge_layout.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <memory>
#include <new>
#include <type_traits>
#include <vector>

namespace {

enum { ORDER_IDENTITY = 0, ORDER_PERM = 1, ORDER_BIJECTION = 2 };

struct GloveParams {
    float *focus, *context, *fbias, *cbias;
    float *gsf, *gsc, *gsfb, *gscb;          // Adagrad.gradSq* | Adam/AMSGrad.M1*
    float *m2f, *m2c, *m2fb, *m2cb;          // Adam/AMSGrad.M2*
    double correction;                       // Adam: lr*sqrt(1-beta2^(t+1))/(1-beta1^(t+1))  (Adam.java:84), per epoch
    int32_t opt;                             // GE_OPT_*
    float *hub32;                            // bf16 embeddings: fp32 master rows of the hub columns [n_hub x D]
    const int32_t *hub_index;                // bf16 embeddings: column -> row of hub32, -1 for ordinary columns
    const int32_t *I, *J;
    const float *X;
    const int32_t *perm;
    const double *L;       // Hogwild: per-nonzero log term  (k_cost_terms)
    const float *W;        // Hogwild: per-nonzero weight
    const int32_t *bA, *bB;   // Hogwild, blocked order: resident / streamed row id per re-ordered position
    int64_t n_chunks;         // chunks of <= RUN_CHUNK nonzeros per epoch
    int64_t ticket_end;       // this launch hands out the tickets below this one (n_chunks: the whole epoch; less: one segment of it)
    int64_t n_hchunks;        // blocked order: the chunks below this one are hub columns (column-major; behind the tile chunks, if any)
    int32_t blocked;          // 1: chunk c = positions [cstart[c], cstart[c+1]) of the re-ordered arrays (ge_layout.h)
    int32_t hot_enabled;      // blocked order: hub chunks publish deltas with atomics
    int32_t flush_every;      // a hub run publishes its delta at least every this many nonzeros (general order)
    const int32_t *cstart;    // blocked order: first position of every chunk (n_chunks + 1 entries)
    const int32_t *cmeta;     // blocked order: hub chunk: flush limit of its runs; row chunk: the row that publishes by delta, or -1
    double *cost_out;      // Hogwild: one double accumulator
    unsigned long long *queue;   // Hogwild: next chunk to hand out (zeroed before every launch)
    double xmax;
    int64_t N;
    int32_t D;
    int32_t DS;            // row stride of the fp32 row tables in floats (>= RW; a multiple of RW when a row and its accumulator rows interleave)
    int32_t RW;            // row width in floats: D, or D + 4 when a row carries its bias at [D] (fat rows, Hogwild)
    int32_t ES;            // bf16 rows: bf16 elements between consecutive embedding rows (D, or 2 * DS when a row shares a record with its accumulator row)
    int32_t cost_kind;
    float lr;
    int32_t order_mode;
    uint32_t bij_mask, bij_shift;
    uint32_t bij_key[4];
    // hub tiles (k_epoch_tiles; behind everything k_adagrad_runs reads, whose argument offsets stay what they were)
    int64_t n_tchunks;        // blocked order: the first n_tchunks chunks are hub tiles (0 for every other kernel)
    const int32_t *tcols, *tlim;   // per group and slot: the column id (-1: unused) and its flush limit
    // hub panels (k_epoch_panels; behind everything the other two kernels read)
    int64_t n_pchunks;        // panel chunks of the epoch: a queue of their own (0 for every other kernel)
    int32_t n_panel_blocks;   // the blocks below this one start in the panel loop, the others join it when the main queue is empty
    uint32_t pbij_mask, pbij_shift;      // the keyed bijection over the panel tickets (same keys as the main queue's)
    unsigned long long *pqueue;          // next panel ticket (zeroed with the main counter)
    const int32_t *prow0;     // per panel chunk: where its focus rows start in prows (n_pchunks + 1 entries)
    const int32_t *prows;     // the focus rows of every panel chunk, ascending
    const int32_t *ppos;      // per panel chunk: panel, then first position and length of each of its four groups' nonzeros (9 entries)
};

// The Hogwild kernel reads (l, w) instead of X: X never changes, so the fp64 log / sqrt run once
// per nonzero at create time (one lane per nonzero) instead of once per update, and the update
// kernel keeps its registers for rows in flight.  +8 bytes read per update (0.1 % at D=200).
__global__ void k_cost_terms(const float *X, int64_t n, int kind, double xmax, double *L, float *W) {
    int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; k < n; k += stride) {
        double l; float w;
        cost_terms<false>(kind, X[k], xmax, l, w);
        L[k] = l; W[k] = w;
    }
}

// ---- epoch order ----------------------------------------------------------------------
// Keyed bijection of [0, 2^b) (odd multiply, xor-shift, add key: each step invertible),
// cycle-walked into [0, N).  2^b < 2N so the expected number of rounds is < 2.
__host__ __device__ __forceinline__ uint32_t bij_round(uint32_t x, const GloveParams &p) {
    return ge::bij_mix(x, p.bij_mask, p.bij_shift, p.bij_key);
}
__device__ __forceinline__ int64_t map_index(const GloveParams &p, int64_t k) {
    if (p.order_mode == ORDER_PERM) return p.perm[k];
    if (p.order_mode == ORDER_BIJECTION) {
        uint32_t x = (uint32_t)k;
        do { x = bij_round(x, p); } while ((int64_t)x >= p.N);
        return x;
    }
    return k;
}

// ---- init -----------------------------------------------------------------------------
// Optimizer ctor, J/opt/Optimizer.java:50-57: per row i the draws are fBias, cBias, then
// focus[i,d], context[i,d] interleaved; value = (float)(nextFloat() - 0.5) / dimension.
// Row i starts (2+2D)*i draws into the stream: jump the LCG there, then run sequentially.
// The tables are written in their final layout (no dense staging copy): a side whose pointer is null is skipped (a
// sharded handle initialises all V context rows and only its own focus rows), `stride` = floats (bf16: elements)
// between rows, bias_col >= 0 = fat rows (bias at [bias_col], the padding behind it zeroed), else the bias vectors;
// ROW16 = bf16 storage (round to nearest even), whose hub columns also get their fp32 master row.
__device__ __forceinline__ uint16_t bf16_rne(float f) {
    const uint32_t u = __builtin_bit_cast(uint32_t, f);
    return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}
template <bool ROW16>
__global__ void k_init_java(void *focus_, void *context_, float *fbias, float *cbias, int64_t bias_stride, int32_t focus_row0,
                            int32_t row0, int32_t rows, int32_t D, int64_t stride, int32_t bias_col, int32_t row_width,
                            uint64_t seed_state, const int32_t *hub_index, float *hub32) {
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    const int64_t i = (int64_t)row0 + r;
    ge::JavaRandom rng{ge::JavaRandom::jump(seed_state, (uint64_t)i * (uint64_t)(2 + 2 * D))};
    const float fd = (float)D;
    const float fb = (float)((double)rng.next_float() - 0.5) / fd;
    const float cb = (float)((double)rng.next_float() - 0.5) / fd;
    using RT = typename std::conditional<ROW16, uint16_t, float>::type;
    RT *f = focus_ ? reinterpret_cast<RT *>(focus_) + (i - focus_row0) * stride : nullptr;
    RT *c = context_ ? reinterpret_cast<RT *>(context_) + i * stride : nullptr;
    float *hub = (ROW16 && c && hub32 && hub_index[i] >= 0) ? hub32 + (int64_t)hub_index[i] * D : nullptr;
    for (int32_t d = 0; d < D; ++d) {
        const float fv = (float)((double)rng.next_float() - 0.5) / fd;
        const float cv = (float)((double)rng.next_float() - 0.5) / fd;
        if constexpr (ROW16) { if (f) f[d] = bf16_rne(fv); if (c) c[d] = bf16_rne(cv); if (hub) hub[d] = cv; }
        else { if (f) f[d] = fv; if (c) c[d] = cv; }
    }
    if constexpr (!ROW16) {
        if (bias_col >= 0) {
            if (f) { f[bias_col] = fb; for (int32_t d = bias_col + 1; d < row_width; ++d) f[d] = 0.0f; }
            if (c) { c[bias_col] = cb; for (int32_t d = bias_col + 1; d < row_width; ++d) c[d] = 0.0f; }
        }
    }
    if (bias_col < 0) {
        if (f) fbias[(i - focus_row0) * bias_stride] = fb;
        if (c) cbias[i * bias_stride] = cb;
    }
}

__global__ void k_fill(float *p, int64_t n, float v) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) p[i] = v;
}
// rows of an accumulator table in its final layout: columns [0, valid) = v, [valid, width) = 0 (fat-row padding)
__global__ void k_fill_rows(float *p, int64_t rows, int64_t stride, int32_t valid, int32_t width, float v) {
    const int64_t n = rows * width, step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
        const int64_t r = i / width; const int32_t c = (int32_t)(i - r * width);
        p[r * stride + c] = c < valid ? v : 0.0f;
    }
}

// Optimizer.extractResult: (focus + context) / 2 in fp32, widened on store for the f64 form.
template <typename OUT>
__global__ void k_extract(const float *focus, const float *context, OUT *out, int64_t n) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) out[i] = (OUT)((focus[i] + context[i]) / 2.0f);
}

// Fat rows (fp32 Hogwild tables): [row(D) | bias | 3 x 0].  Columns [col0, col0+ncols) of `rows` fat rows <-> a dense
// [rows x ncols] array: ncols = D, col0 = 0 is the row table as the API shows it, ncols = 1, col0 = D its bias vector.
template <bool TO_DENSE>
__global__ void k_fat_copy(float *fat, int64_t rows, int32_t DS, int32_t col0, int32_t ncols, float *dense) {
    const int64_t n = rows * ncols, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int64_t r = i / ncols; const int32_t c = (int32_t)(i - r * ncols);
        if constexpr (TO_DENSE) dense[i] = fat[r * DS + col0 + c];
        else fat[r * DS + col0 + c] = dense[i];
    }
}

// bf16 embeddings (BASELINE config C5): storage conversions.  Round-to-nearest-even on the way in (init, set_state).
// dense fp32 [rows x D] <-> bf16 rows `es` elements apart
__global__ void k_f32_to_bf16(const float *src, uint16_t *dst, int64_t n, int32_t D, int64_t es) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        const uint32_t u = __builtin_bit_cast(uint32_t, src[i]);       // bf16_rne, restated: calling it here makes the compiler unroll
        const int64_t r = i / D;                                        // this loop (216 -> 784 instructions for the same result)
        dst[r * es + (i - r * D)] = (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
    }
}
__global__ void k_bf16_to_f32(const uint16_t *src, float *dst, int64_t n, int32_t D, int64_t es) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) { const int64_t r = i / D; dst[i] = __builtin_bit_cast(float, (uint32_t)src[r * es + (i - r * D)] << 16); }
}
// hub rows live in the fp32 master table: dir 0 = full[col] -> hub32[idx], dir 1 = hub32[idx] -> full[col]
__global__ void k_hub_rows(float *full, float *hub32, const int32_t *hub_index, int32_t V, int32_t D, int dir) {
    const int32_t v = blockIdx.x;
    const int32_t h = hub_index[v];
    if (h < 0) return;
    for (int d = threadIdx.x; d < D; d += blockDim.x) {
        if (dir == 0) hub32[(int64_t)h * D + d] = full[(int64_t)v * D + d];
        else full[(int64_t)v * D + d] = hub32[(int64_t)h * D + d];
    }
}

// ---- exact (deterministic) kernel -------------------------------------------------------
// One wavefront walks nonzeros [k_begin, k_end) strictly in order and reproduces the Java
// arithmetic bit for bit: products in fp32, summed sequentially in d order (GloveCost.java:10-11),
// fp64 sqrt/div in the update (Adagrad.java:76-77,88-89), per-job fp32 cost accumulator (:60).
__global__ __launch_bounds__(64) void k_adagrad_exact(GloveParams p, int64_t k_begin, int64_t k_end,
                                                      float *job_cost) {
    extern __shared__ float s_prod[];
    const int lane = threadIdx.x;
    float cost = 0.0f;
    for (int64_t k = k_begin; k < k_end; ++k) {
        const int64_t idx = map_index(p, k);
        ge::exact_update(p, p.I[idx], p.J[idx], p.X[idx], s_prod, lane, cost);      // ge_exact.h: shared with k_adagrad_strata
    }
    if (lane == 0) *job_cost = cost;
}

// ---- Hogwild kernel -----------------------------------------------------------------------
// One wavefront = one sequential worker, like one Java pool thread (Adagrad.createJob walks its
// slice in order).  A worker takes a chunk of 128 nonzeros of the epoch order, sorts it by column
// in registers (bitonic network, no LDS, no barrier) and walks it sequentially:
//   * a RUN of equal j keeps context[j], gradSqContext[j], cBias[j], gradSqCBias[j] in registers --
//     loaded once, updated in place with exact sequential semantics inside the run, written once;
//   * the other side of every nonzero is streamed: 16-byte-per-lane buffer loads (row base in SGPRs,
//     hardware bounds check masks the lanes past the row), the fp32 dot is wave-reduced, the fused
//     AdaGrad update is written straight back.  The NEXT nonzero's streamed rows are requested into LDS
//     (buffer_load ... lds) before the current one waits for its own, so a request has a whole step to
//     complete (see s_setA / s_setB below for why LDS and not registers).
// (Blocked layout, the default: the resident side is the hub COLUMN in hub chunks and the focus ROW elsewhere.)
// Workers never lock (Hogwild).  ~10^4 workers are in flight where the JVM has <= #cores, so for
// HOT columns (hub nodes that sit in a large share of the nonzeros) a plain read-modify-write
// would lose most concurrent updates and training stalls (measured): their runs read
// the row with agent-coherent (sc1) loads and publish the run's DELTA with float atomic adds.
// Run-combining is what makes that affordable: same-address atomics serialise at ~25 ns per
// cache line at the memory side.
using namespace ge;   // ge_wave.h: Vec, comp, buf_load / buf_store, make_rsrc, rfl, wave_sum

// four bf16 values (8 bytes) widened to fp32
__device__ __forceinline__ float4 widen_bf16x4(float2 raw) {
    const uint32_t lo = __builtin_bit_cast(uint32_t, raw.x), hi = __builtin_bit_cast(uint32_t, raw.y);
    float4 r;
    r.x = __builtin_bit_cast(float, lo << 16); r.y = __builtin_bit_cast(float, lo & 0xFFFF0000u);
    r.z = __builtin_bit_cast(float, hi << 16); r.w = __builtin_bit_cast(float, hi & 0xFFFF0000u);
    return r;
}
#define GE_LDS(ptr) ((__attribute__((address_space(3))) void *)(ptr))
// one load-to-LDS wave instruction: lane L brings W bytes from offset `voff` of the resource to lds + L * W
template <int W> __device__ __forceinline__ void load_to_lds(__amdgpu_buffer_rsrc_t rs, float *lds, int voff) {
    static_assert(W == 16 || W == 4, "16-byte or 4-byte lanes");
    if constexpr (W == 16) __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, GE_LDS(lds), 16, voff, 0, 0, 16 /* AUX_SC1 */);
    else __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, GE_LDS(lds), 4, voff, 0, 0, 16 /* AUX_SC1 */);
}
// s_waitcnt immediate (gfx9 layout) that waits until at most n vector-memory instructions are outstanding and for nothing else
constexpr int wait_vmcnt(int n) { return (n & 15) | ((n >> 4) << 14) | 0x0F70; }

// A workgroup barrier that orders LDS accesses only: this wave's LDS operations are complete (lgkmcnt(0)) before it arrives, its
// vector-memory instructions stay in flight -- __syncthreads() would wait for those too (its fence covers global memory), and with
// them for the focus pair that stage 0 of the panel pipeline has requested for the NEXT step.
__device__ __forceinline__ void lds_barrier() {
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_waitcnt(0xC07F);       // lgkmcnt(0) and nothing else
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

constexpr int RUN_CHUNK = 128;            // nonzeros per worker chunk (2 per lane)
constexpr int KEY_PAD = 0x7FFFFFFF;       // sorts last; marks the unused tail of the last chunk
constexpr int TILE_N_AFTER = 4;           // tile_chunk: vector-memory instructions behind a focus pair's request when its image is read

// ---- hub tiles ---------------------------------------------------------------
// One tile chunk: <= 128 nonzeros of ONE group of G dense hub columns, whole focus rows, rows ascending, slot order inside a row.
// The G context pairs (row + accumulator row) stay in registers for the chunk, each with a copy as read; every focus pair streams
// through ONCE -- requested into an LDS image one row ahead, updated in registers by its <= G nonzeros, stored once -- where a
// column-major hub chunk moves it once per nonzero.  fp32 fat rows of one register chunk only (VW 4, NCH 1: D % 4 == 0, D <= 252).
// The update is the instruction sequence of epoch_walk's step with A = the context row of the slot and B = the focus row.  The
// bias of a resident row stays where it was loaded (lane D / 4, component 0: not a row element, so the row arithmetic never
// touches it) and is read from there by every update -- the G pairs take 16 G registers, the scalars none.
// A column is published when it has taken its flush limit of updates since it was read, and re-read behind the publish, exactly
// as a cut hub run; at the end of the chunk every column touched since its last read is published.
// Hub panels: the same walk as one stage of a pipeline.  The four waves of a workgroup hold the four groups of a
// panel; a focus pair enters at wave 0 from memory, is handed from wave to wave through an LDS image and leaves from wave 3 to
// memory.  Where the pair comes from and where it goes is a compile-time choice (SRC, SINK); a stage whose SRC or SINK is an LDS
// image walks the rows of `pl` (every row of the panel chunk, whether this group has a nonzero there or not) with one block barrier
// per step, `pl.lag` steps behind wave 0.
enum { PAIR_MEM = 0, PAIR_LDS = 1 };
struct PanelLink {
    const int32_t *rows;      // LDS: the focus rows of the panel chunk, ascending
    int32_t n_rows;           // read from LDS by every wave of the block: the same number in all four
    int32_t lag;              // this stage works on row t - lag at step t (its wave in the block)
    float *nextA, *nextB;     // SINK = PAIR_LDS: the two images of the next stage
    float *ring;              // KD > 1: the KD + 1 images of stage 0's request ring, RING_IMG floats each
};
constexpr int RING_IMG = 512;             // floats per image of the ring: a row's image and its accumulator row's behind it (IMG_G)
// KD: how many rows ahead stage 0 of the panel pipeline requests its focus pair.  1: one row ahead into the
// other of two images, chosen at compile time (every kernel but the ring kernel).  KD > 1: row t + KD is requested at step t into
// a ring of KD + 1 images, and the image of row t is read behind vmcnt(2 KD).
template <int G, int SRC, int SINK, int KD = 1>
__device__ __forceinline__ void tile_chunk(const GloveParams &p, const int32_t c_lo, const int32_t c_len, const int32_t grp,
                                           float *const setA, float *const setB, float *const tr_c, float *const tr_g,
                                           int32_t *const stg, double &cost_acc, const PanelLink &pl, const int lane) {
    constexpr bool PIPE = SRC == PAIR_LDS || SINK == PAIR_LDS;
    // vector-memory instructions behind a focus pair's request when its image is read: the next row's request, and in front of it
    // the two stores that ended the previous row where this stage stores (see walk_row)
    constexpr int N_AFTER = KD > 1 ? 2 * KD : SINK == PAIR_MEM ? TILE_N_AFTER : TILE_N_AFTER - 2;
    static_assert(KD == 1 || (KD >= 2 && SRC == PAIR_MEM && SINK == PAIR_LDS), "the request ring is stage 0's: it stores nothing to memory");
    static_assert(N_AFTER < 64, "vmcnt is a 6-bit counter");
    static_assert(G >= 2 && G <= 8, "two to eight resident columns");
    const int32_t D = p.D, DS = p.DS;
    const uint32_t row_bytes = (uint32_t)p.RW * 4u;
    const int bl_lane = (D / 4) & 63;                    // the lane that holds element [D], the bias
    const bool inr = lane * 4 < D, is_bl = lane == bl_lane;
    const float lr = p.lr;
    constexpr int IMG_G = 256;                           // the accumulator row's image behind the row's (epoch_walk: IMG_G)
    auto rl = [&](float v) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), bl_lane)); };

    // ---- stage: focus row, slot, weight and log term of the chunk's nonzeros into this wave's LDS strip (the chunk is in walk order:
    // nothing to sort).  The walk reads them back at wave-uniform addresses, so they take no vector register -- and no scalar
    // load from memory per nonzero either, whose latency a row of two or three nonzeros cannot hide (measured).
    // (the strip is the caller's: a __shared__ array in here would exist once per instance of this template; the lane index goes
    // through an empty asm so that the strip's addresses are computed here, per chunk, and not held in registers across the kernel)
    int s_lane = lane;
    asm volatile("" : "+v"(s_lane));
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int e = q * 64 + s_lane;
        if (e < c_len) {
            const int64_t k = (int64_t)c_lo + e;
            const long long lb = __builtin_bit_cast(long long, p.L[k]);
            stg[e] = p.bA[k]; stg[RUN_CHUNK + e] = p.bB[k]; stg[2 * RUN_CHUNK + e] = __builtin_bit_cast(int32_t, p.W[k]);
            stg[3 * RUN_CHUNK + 2 * e] = (int32_t)(lb & 0xFFFFFFFFll); stg[3 * RUN_CHUNK + 2 * e + 1] = (int32_t)(lb >> 32);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    auto staged = [&](int what, int e) { return rfl(stg[what * RUN_CHUNK + rfl(e)]); };
    auto row_at = [&](int e) { return staged(0, e); };

    // Requests a focus pair into an image.  `live` false: the same two instructions against zero-sized resources.  Issued once
    // per row on every path, like the two stores that end a row: the wait below counts them.
    auto request = [&](float *img, int32_t row, bool live) {
        const uint32_t rbytes = live ? row_bytes : 0u;
        load_to_lds<16>(make_rsrc(p.focus + (int64_t)row * DS, rbytes), img, lane * 16);
        load_to_lds<16>(make_rsrc(p.gsf + (int64_t)row * DS, rbytes), img + IMG_G, lane * 16);
        asm volatile("" ::: "memory");
    };
    int32_t n_row = 0;
    if constexpr (!PIPE) n_row = row_at(0);
    else if constexpr (SRC == PAIR_MEM) n_row = rfl(pl.rows[0]);
    int ring_cur = 0;                                    // KD > 1: the image of the row that is walked next
    if constexpr (KD == 1) {
        if constexpr (SRC == PAIR_MEM) request(setA, n_row, true);
    } else {
        // rows 0 .. KD - 1 into images 0 .. KD - 1 (a chunk shorter than that: zero-sized resources, the same 2 KD instructions)
#pragma unroll
        for (int q = 0; q < KD; ++q) {
            const bool live = q < pl.n_rows;
            request(pl.ring + q * RING_IMG, live ? rfl(pl.rows[q]) : 0, live);
        }
    }

    // ---- the G resident pairs ----
    float4 a[G], ga[G], a0[G], ga0[G];
    int32_t col[G], lim[G], cnt[G];
    auto ctx_rsrc = [&](int32_t c) { return make_rsrc(p.context + (int64_t)(c < 0 ? 0 : c) * DS, c < 0 ? 0u : row_bytes); };
    auto gsc_rsrc = [&](int32_t c) { return make_rsrc(p.gsc + (int64_t)(c < 0 ? 0 : c) * DS, c < 0 ? 0u : row_bytes); };
#pragma unroll
    for (int s = 0; s < G; ++s) {
        col[s] = rfl(p.tcols[(int64_t)grp * G + s]); lim[s] = rfl(p.tlim[(int64_t)grp * G + s]); cnt[s] = 0;
    }
#pragma unroll
    for (int s = 0; s < G; ++s) {                        // (an unused slot: zero-sized resources, still two loads)
        a[s] = buf_load<4, AUX_SC1>(ctx_rsrc(col[s]), lane * 16);
        ga[s] = buf_load<4, AUX_SC1>(gsc_rsrc(col[s]), lane * 16);
    }
#pragma unroll
    for (int s = 0; s < G; ++s) { a0[s] = a[s]; ga0[s] = ga[s]; }

    // The slot of a nonzero is wave-uniform: a switch over G unrolled bodies, never a register array indexed at run time.  (The
    // empty asm ends every case so that the compiler cannot merge the cases' tails into one access through a selected pointer --
    // which is such an index, and put the arrays into scratch.)
    auto for_slot = [&](const int s, auto &&f) {
        switch (s) {
            case 0: f(std::integral_constant<int, 0>{}); asm volatile(""); break;
            case 1: f(std::integral_constant<int, 1>{}); asm volatile(""); break;
            case 2: if constexpr (G > 2) f(std::integral_constant<int, 2>{}); asm volatile(""); break;
            case 3: if constexpr (G > 3) f(std::integral_constant<int, 3>{}); asm volatile(""); break;
            case 4: if constexpr (G > 4) f(std::integral_constant<int, 4>{}); asm volatile(""); break;
            case 5: if constexpr (G > 5) f(std::integral_constant<int, 5>{}); asm volatile(""); break;
            case 6: if constexpr (G > 6) f(std::integral_constant<int, 6>{}); asm volatile(""); break;
            case 7: if constexpr (G > 7) f(std::integral_constant<int, 7>{}); asm volatile(""); break;
            default: break;
        }
    };
    // a column's delta through this wave's LDS strip with float atomics, its bias last-writer-wins (epoch_walk: close_run, ATOMIC)
    auto publish = [&](const int32_t c, const float4 &ca, const float4 &cga, const float4 &ca0, const float4 &cga0) {
        const __amdgpu_buffer_rsrc_t rs_a = ctx_rsrc(c), rs_ga = gsc_rsrc(c);
        float4 dc, dg;
        dc.x = ca.x - ca0.x; dc.y = ca.y - ca0.y; dc.z = ca.z - ca0.z; dc.w = ca.w - ca0.w;
        dg.x = cga.x - cga0.x; dg.y = cga.y - cga0.y; dg.z = cga.z - cga0.z; dg.w = cga.w - cga0.w;
        if (is_bl) { dc.x = 0.0f; dg.x = 0.0f; }         // the bias is no part of the delta
        *reinterpret_cast<float4 *>(tr_c + lane * 4) = dc;
        *reinterpret_cast<float4 *>(tr_g + lane * 4) = dg;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int e = lane + k * 64;                  // element index; past the row the buffer check drops it
            __builtin_amdgcn_raw_ptr_buffer_atomic_fadd_f32(tr_c[e], rs_a, e * 4, 0, 0);
            __builtin_amdgcn_raw_ptr_buffer_atomic_fadd_f32(tr_g[e], rs_ga, e * 4, 0, 0);
        }
        __builtin_amdgcn_wave_barrier();
        const float ab = rl(ca.x), gab = rl(cga.x);
        if (lane == 0) {
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, ab), rs_a, D * 4, 0, AUX_SC1);
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, gab), rs_ga, D * 4, 0, AUX_SC1);
        }
    };

    float4 b, gb;                                        // the focus pair being updated
    float bb = 0.0f, gbb = 0.0f;                         // its bias and the bias's accumulator
    // One nonzero: the pair of its slot is copied out of the resident set, updated by ONE body shared by all slots, and copied
    // back (eight register moves each way: far less than a body per slot costs in registers and instruction cache).
    auto update = [&](const int s, const float w, const double l) {
        float4 ca, cga;
        // (a slot outside 0 .. G-1 cannot come out of the layout; if it did, the defaults below make the nonzero a no-op on the
        // resident set -- nothing selected, nothing written back, the publish against zero-sized resources -- not a wild access)
        int32_t c_cnt = 0, c_lim = 1, c_col = -1;
        for_slot(s, [&](auto S) { constexpr int q = decltype(S)::value; ca = a[q]; cga = ga[q]; c_cnt = cnt[q]; c_lim = lim[q]; c_col = col[q]; });
        const float ab = rl(ca.x), gab = rl(cga.x);
        float part = 0.0f;
        if (inr) {
#pragma unroll
            for (int t = 0; t < 4; ++t) part = __builtin_fmaf(comp<4>(ca, t), comp<4>(b, t), part);
        }
        part = wave_sum(part);
        const float ic = (float)((double)part + ((double)(ab + bb) - l));
        const float wc = w * ic;
        cost_acc += (0.5 * (double)wc) * (double)ic;
        const float wlr = wc * lr;
        const float nbb = bb - wc * __frsqrt_rn(gbb), ngbb = gbb + wc * wc;
        if (inr) {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const float av = comp<4>(ca, t), bv = comp<4>(b, t);
                const float grad_b = wc * av, grad_a = wc * bv;
                const float sa = comp<4>(cga, t), sb = comp<4>(gb, t);
                comp<4>(b, t)   = __builtin_fmaf(-(wlr * av), __frsqrt_rn(sb), bv);
                comp<4>(gb, t)  = __builtin_fmaf(grad_b, grad_b, sb);
                comp<4>(ca, t)  = __builtin_fmaf(-(wlr * bv), __frsqrt_rn(sa), av);
                comp<4>(cga, t) = __builtin_fmaf(grad_a, grad_a, sa);
            }
        }
        const float w2 = wc * wc;
        const float nab = ab - wc * __frsqrt_rn(gab), ngab = gab + w2;
        if (is_bl) { ca.x = nab; cga.x = ngab; }
        bb = nbb; gbb = ngbb;
        if (++c_cnt >= c_lim) {                          // a cut: publish, then what memory holds once the publish is in (same wave,
            float4 ca0, cga0;                            // same addresses: in order)
            for_slot(s, [&](auto S) { constexpr int q = decltype(S)::value; ca0 = a0[q]; cga0 = ga0[q]; });
            publish(c_col, ca, cga, ca0, cga0);
            ca = buf_load<4, AUX_SC1>(ctx_rsrc(c_col), lane * 16);
            cga = buf_load<4, AUX_SC1>(gsc_rsrc(c_col), lane * 16);
            for_slot(s, [&](auto S) { constexpr int q = decltype(S)::value; a0[q] = ca; ga0[q] = cga; });
            c_cnt = 0;
        }
        for_slot(s, [&](auto S) { constexpr int q = decltype(S)::value; a[q] = ca; ga[q] = cga; cnt[q] = c_cnt; });
    };

    // ---- the rows of the chunk ----
    // One focus row.  CUR (0 / 1) names the image that holds its pair (a compile-time choice, as in epoch_walk's step: the
    // compiler then knows that the request for the other image does not touch the one read here).
    int pos = 0;
    auto walk_row = [&](auto CUR, const int ri) {
        int32_t row;
        int nxt;                                         // where the row ends, and the row behind it
        bool more;
        if constexpr (!PIPE) {
            row = n_row;
            nxt = pos + 1;
            for (;;) {
                more = nxt < c_len;
                n_row = more ? row_at(nxt) : 0;
                if (!more || n_row != row) break;
                ++nxt;
            }
        } else {                                         // the rows are the panel chunk's; this group may have nothing in one
            row = rfl(pl.rows[ri]);
            nxt = pos;
            while (nxt < c_len && row_at(nxt) == row) ++nxt;
            more = ri + 1 < pl.n_rows;
            if constexpr (SRC == PAIR_MEM && KD == 1) n_row = more ? rfl(pl.rows[ri + 1]) : 0;
        }
        const float *const img = decltype(CUR)::value ? setB : setA;
        if constexpr (KD > 1) {
            // Row ri + KD goes into the image that row ri - 1 was read from (ring_cur - 1, cyclically): that read is complete, its
            // lgkmcnt wait is inside the asm below.  The rows of a panel chunk are distinct, and no request crosses the chunk's end.
            const bool ahead = ri + KD < pl.n_rows;
            const int32_t a_row = ahead ? rfl(pl.rows[ri + KD]) : 0;
            request(pl.ring + (ring_cur == 0 ? KD : ring_cur - 1) * RING_IMG, a_row, ahead);
            // Counted by hand: stage 0 stores nothing, so behind the request of row ri exactly the 2 loads of each of the KD later
            // requests are certain (before the first row also the 2 G loads of the resident pairs); publishes and re-reads add to them.
            __builtin_amdgcn_s_waitcnt(wait_vmcnt(N_AFTER));
            // The image is chosen at run time.  A plain LDS read would make the compiler wait for every load-to-LDS in flight
            // (vmcnt(0): it cannot tell the images apart); the asm is opaque to that bookkeeping and waits for its own reads.
            const uint32_t at = (uint32_t)(uintptr_t)GE_LDS(pl.ring + ring_cur * RING_IMG) + (uint32_t)lane * 16u;
            ge_i4 rb, rgb;
            asm volatile("ds_read_b128 %0, %2\n\tds_read_b128 %1, %2 offset:1024\n\ts_waitcnt lgkmcnt(0)"
                         : "=&v"(rb), "=&v"(rgb) : "v"(at) : "memory");
            __builtin_memcpy(&b, &rb, 16); __builtin_memcpy(&gb, &rgb, 16);
            ring_cur = ring_cur == KD ? 0 : ring_cur + 1;
        } else
        if constexpr (SRC == PAIR_MEM) {
            request(decltype(CUR)::value ? setA : setB, n_row, more);
            // Counted by hand (see epoch_walk's step): memory instructions complete in order, and behind this image's request at
            // least N_AFTER more have been issued on every path -- where this stage stores its pair, the two stores that ended the
            // previous row (before the first row: the 2 G loads of the resident pairs); then the two loads of the request just
            // above.  Publishes and re-reads in between only add to them.
            __builtin_amdgcn_s_waitcnt(wait_vmcnt(N_AFTER));
        }
        // (SRC = PAIR_LDS: the previous stage wrote the image one step ago, and the block barrier that ended that step lies between)
        asm volatile("" ::: "memory");
        if constexpr (KD == 1) {
            b = *reinterpret_cast<const float4 *>(img + lane * 4);
            gb = *reinterpret_cast<const float4 *>(img + IMG_G + lane * 4);
        }
        bb = rl(b.x); gbb = rl(gb.x);
        for (int e = pos; e < nxt; ++e) {
            const int s = staged(1, e);
            const float w = __builtin_bit_cast(float, staged(2, e));
            const unsigned lo = (unsigned)rfl(stg[3 * RUN_CHUNK + 2 * rfl(e)]), hi = (unsigned)rfl(stg[3 * RUN_CHUNK + 2 * rfl(e) + 1]);
            const double l = __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
            update(s, w, l);
        }
        // the pair goes out once: the row's lanes, the bias lane, zeros in the padding behind it (whole lines, as a streamed row's store)
        float4 ob = b, ogb = gb;
        if (!inr) {
            ob = float4{0.0f, 0.0f, 0.0f, 0.0f}; ogb = ob;
            if (is_bl) { ob.x = bb; ogb.x = gbb; }
        }
        if constexpr (SINK == PAIR_MEM) {
            buf_store<4>(ob, make_rsrc(p.focus + (int64_t)row * DS, row_bytes), lane * 16);
            buf_store<4>(ogb, make_rsrc(p.gsf + (int64_t)row * DS, row_bytes), lane * 16);
        } else {                                         // the image the next stage reads one step from now
            float *const out = decltype(CUR)::value ? pl.nextB : pl.nextA;
            *reinterpret_cast<float4 *>(out + lane * 4) = ob;
            *reinterpret_cast<float4 *>(out + IMG_G + lane * 4) = ogb;
        }
        asm volatile("" ::: "memory");
        pos = nxt;
    };
    constexpr std::integral_constant<int, 0> IMG_A{};
    constexpr std::integral_constant<int, 1> IMG_B{};
    if constexpr (!PIPE) {
        while (pos < c_len) {
            walk_row(IMG_A, 0);
            if (pos < c_len) walk_row(IMG_B, 0);
        }
    } else {
        // The pipeline: n_rows + 3 steps, one block barrier each.  This stage idles `lag` steps, walks the n_rows rows -- row ri in
        // image ri & 1, which the previous stage filled one step earlier and refills one step later -- and idles 3 - lag steps.
        // Every barrier below is reached lag + n_rows + (3 - lag) = n_rows + 3 times by every wave of the block: n_rows is one
        // LDS word that all four waves read behind the same barrier, and no barrier sits under any other condition.
        // (Only LDS travels between the stages, so the barriers order LDS alone: lds_barrier.  What the stages write to memory is
        // ordered for the next chunk by the full barrier of the ticket draw that follows.)
        for (int i = 0; i < pl.lag; ++i) lds_barrier();             // (i) lag barriers: see above
        for (int ri = 0; ri < pl.n_rows; ri += 2) {
            walk_row(IMG_A, ri);
            lds_barrier();                                          // (ii) one per row, n_rows in all
            if (ri + 1 < pl.n_rows) {
                walk_row(IMG_B, ri + 1);
                lds_barrier();                                      // (ii)
            }
        }
        for (int i = pl.lag; i < 3; ++i) lds_barrier();             // (iii) 3 - lag barriers
    }
    // ---- every column touched since it was last read ----
#pragma nounroll
    for (int s = 0; s < G; ++s)
        for_slot(s, [&](auto S) { constexpr int q = decltype(S)::value; if (cnt[q] > 0) publish(col[q], a[q], ga[q], a0[q], ga0[q]); });
}

// The walk is one inlined body that two kernels instantiate: k_adagrad_runs (TG = 0) and k_epoch_tiles<G> (TG = G), which walks
// the hub tile chunks [0, n_tchunks) of the layout with tile_chunk above and every other chunk exactly as k_adagrad_runs does.
// OPT: GE_OPT_ADAGRAD keeps one auxiliary row per side (gradSq), Adam / AMSGrad two (M1, M2).
// EMB16: the embedding rows (focus, context) are stored as bf16, everything else stays fp32 (BASELINE config C5).
//   Rows are widened to fp32 when loaded; a resident row stays fp32 in registers for its whole run and is
//   narrowed once, with STOCHASTIC rounding (an update of 1e-5 on a value of 0.1 is far below half a bf16 ulp and
//   would always round away).  Hub context rows keep an fp32 master copy (hub32) that their runs read and
//   publish into with the same atomics as in the fp32 build; they never touch the bf16 table during training.
// PANELS (k_epoch_panels): the workgroup also walks the hub panel chunks of the layout, its four waves as the four stages of
// tile_chunk's pipeline.  The panel chunks have a ticket counter of their own; a block below n_panel_blocks serves it first and the
// main queue afterwards, every other block the other way round, so whichever queue runs dry first frees its blocks for the other.
// WD: how many nonzeros ahead the ordinary walk requests its streamed pair.  1: the next nonzero's, into the other
// of two images (every kernel but k_epoch_walk2).  2: the pair of nonzero pos + 2 is requested at the top of step pos into the
// third of three images, and the image of nonzero pos is read behind vmcnt(2 N_TAB + 2 N_DMA).
template <int VW, int NCH, int OPT, bool EMB16, bool FAT, int TG, bool PANELS = false, int KD = 1, int WD = 1>
__device__ __forceinline__ void epoch_walk(const GloveParams &p, const int32_t n_workers) {
    using VT = typename Vec<VW>::T;
    static_assert(!EMB16 || VW == 4, "bf16 embeddings need dim % 4 == 0");
    constexpr bool MOM = OPT != GE_OPT_ADAGRAD;
    // FAT rows (every fp32 Hogwild table): a row is D + 4 floats, element [D] is the row's bias (in the accumulator /
    // moment tables: the bias accumulator / moment), the rest padding that stays zero.  The bias rides in the sector
    // the row's tail already occupies, so a streamed update costs four row accesses and no 4-byte ones.
    // bf16 rows (EMB16) have no fp32 row to carry the bias: both scalars ride behind the ACCUMULATOR row,
    // [gradSq (D) | the bias accumulator | the bias | 2 x 0]; the bf16 row itself stays D elements wide.
    // (FAT is chosen on the host: fp32 rows whose bias lane fits the last register chunk -- a dimension that fills its 64-lane
    // chunks exactly would need one more chunk for that one lane and keeps the separate bias tables instead.)
    int tid = (int)threadIdx.x;             // (not const: see the rounds below)
    uint32_t sr_state = 0x9E3779B9u * (uint32_t)(threadIdx.x + 1) + (uint32_t)blockIdx.x * 0x85EBCA6Bu + p.bij_key[0];
    // embedding-row access: fp32 build = plain 16-byte vectors; bf16 build = 8 bytes widened / narrowed here
    auto emb_rsrc = [&](float *base, int64_t id) {
        if constexpr (EMB16) return make_rsrc(reinterpret_cast<uint16_t *>(base) + id * p.ES, (uint32_t)p.D * 2u);
        else return make_rsrc(base + id * p.DS, (uint32_t)p.RW * 4u);
    };
    auto emb_load = [&](__amdgpu_buffer_rsrc_t rs, int q) -> VT {
        if constexpr (EMB16) return widen_bf16x4(buf_load<2, AUX_SC1>(rs, ((tid & 63) + q * 64) * 8));
        else return buf_load<VW, AUX_SC1>(rs, ((tid & 63) + q * 64) * VW * 4);
    };
    auto emb_store = [&](VT v, __amdgpu_buffer_rsrc_t rs, int q) {
        if constexpr (EMB16) {
            auto narrow = [&](float f) -> uint32_t {      // stochastic rounding: add 16 random low bits, truncate
                sr_state = sr_state * 1664525u + 1013904223u;
                return (__builtin_bit_cast(uint32_t, f) + (sr_state >> 16)) >> 16;
            };
            float2 raw;
            raw.x = __builtin_bit_cast(float, narrow(v.x) | (narrow(v.y) << 16));
            raw.y = __builtin_bit_cast(float, narrow(v.z) | (narrow(v.w) << 16));
            buf_store<2>(raw, rs, ((tid & 63) + q * 64) * 8);
        } else buf_store<VW>(v, rs, ((tid & 63) + q * 64) * VW * 4);
    };
    constexpr float BETA1 = 0.9f, BETA2 = 0.999f, EPS = 1e-7f, OMB1 = 1 - BETA1, OMB2 = 1 - BETA2;   // Adam.java:45-53
    const float corr = OPT == GE_OPT_ADAM ? (float)p.correction : p.lr;      // Adam.java:84 | AMSGrad.java:133 uses lr itself
    // one element of an Adam / AMSGrad update in fp32: new moments and the parameter step
    auto moment_step = [&](float grad, float &m, float &v) -> float {
        m = __builtin_fmaf(BETA1, m, OMB1 * grad);
        const float vn = __builtin_fmaf(BETA2, v, OMB2 * (grad * grad));
        v = OPT == GE_OPT_AMSGRAD ? fmaxf(v, vn) : vn;
        // IEEE operations only (fma, mul, add, correctly rounded sqrt and division: HIP's default for fp32 without fast-math), so that
        // tests/kernel_model.py can restate this arithmetic bit for bit; __fsqrt_rn is the 1-ulp v_sqrt_f32 in this toolchain
        return corr * m * (1.0f / (__builtin_sqrtf(v) + EPS));
    };
    const int32_t D = p.D;
    const int32_t DS = p.DS;
    const uint32_t row_bytes = (uint32_t)p.RW * 4u;
    const int bl_q = (D / VW) >> 6, bl_lane = (D / VW) & 63;     // FAT: the lane and register chunk that hold element [D]
    // FAT: which row (parameter or accumulator) and which component of that lane's vector hold the bias; its accumulator is
    // component 0 of the accumulator row's lane in both layouts
    constexpr bool BIAS_IN_ACC = EMB16;
    constexpr int BIAS_C = EMB16 ? 1 : 0;
    const float lr = p.lr;
    const int wave = rfl((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    // workers pull chunks of the epoch order from one queue.  (PANELS: every block holds a worker, and all four of its waves stay
    // for the panel chunks -- the block barriers there need them; only the ordinary loop is limited to the workers.)
    if constexpr (!PANELS) { if (wave >= n_workers) return; }
    const int64_t n_chunks = p.n_chunks;
    __shared__ float s_tr[4][2][NCH * 64 * VW];       // per-wave strip for the atomic flush (no block barrier)
    // The streamed rows of the NEXT nonzero land in LDS, not in registers (buffer_load ... lds, 16 bytes per lane): nothing
    // in the register file depends on the load, so it stays in flight across the current nonzero's arithmetic and stores
    // and is waited for only where the next step reads it (with loads into registers the compiler put the copies that merge
    // the two steps' values -- and with them the wait -- right behind the load, and every nonzero paid the full latency).
    // Two images per wave, one per array, so that the wait for one never covers the load into the other.
    // Rows that are multiples of 16 bytes travel 16 bytes per lane; the others (VW < 4) 4 bytes per lane, VW instructions per register chunk.
    constexpr int DMAW = VW == 4 ? 16 : 4;                                            // bytes per lane of one load-to-LDS
    constexpr int N_Q = VW == 4 ? 1 : VW;                                              // such loads per register chunk
    constexpr int IMG = 64 * VW;                                                       // floats per register chunk's image
    constexpr int IMG_R = EMB16 ? ((NCH + 1) / 2) * IMG : NCH * IMG;               // a bf16 row takes half the bytes
    constexpr int IMG_G = IMG_R, IMG_H = IMG_G + NCH * IMG;                          // offsets of the accumulator / second-moment images
    constexpr int IMG_B = IMG_H + (MOM ? NCH * IMG : 0);                             // three 256-byte slots for the bias scalars (not FAT)
    constexpr int SET_FLOATS = IMG_B + (FAT ? 0 : 3 * 64);
    __shared__ float s_setA[4 * SET_FLOATS], s_setB[4 * SET_FLOATS];
    double cost_acc = 0.0;
    __shared__ int32_t s_stage[TG > 0 ? 4 : 1][TG > 0 ? 5 * RUN_CHUNK : 1];      // tile_chunk's strip of staged nonzeros, one per wave
    const PanelLink no_link{nullptr, 0, 0, nullptr, nullptr};

    // The block serves its two queues one after the other (PANELS; every other kernel: the main queue alone).  `panels_first`
    // depends on the block's index only, so all four waves take the same branch in both rounds.
    const bool panels_first = PANELS && (int32_t)blockIdx.x < p.n_panel_blocks;
    // What either loop derives from the thread's index is derived inside its round: computed once at the kernel's entry it would be
    // held across the other loop, which has no register to spare for it (PANELS; every other kernel: the same values as ever).
#pragma nounroll
    for (int round = 0; round < (PANELS ? 2 : 1); ++round) {
    if constexpr (PANELS) asm volatile("" : "+v"(tid));
    if constexpr (PANELS) {
    if ((round == 0) == panels_first) {
        static_assert(!PANELS || TG == 4, "a panel is four groups of four columns, one per wave of the block");
        const int wib = rfl(tid >> 6);
        // the focus rows of one panel chunk: each has a nonzero in one of four groups of <= RUN_CHUNK nonzeros
        __shared__ int32_t s_prow[4 * RUN_CHUNK];
        __shared__ int32_t s_pticket, s_pn;
        __shared__ double s_pcost[4];
        // A block that comes from the main queue: its waves (those that never were workers included) meet here.  Reached once,
        // by every wave of the block: the round and the branch above are the same for all of them.
        __syncthreads();
        const int32_t n_pchunks = (int32_t)p.n_pchunks;
        for (;;) {
            // (the word is free again: every wave read it before barrier (b) of the previous iteration, which thread 0 has passed)
            if (tid == 0) {
                const unsigned long long t = atomicAdd(p.pqueue, 1ull);
                s_pticket = t >= (unsigned long long)n_pchunks ? -1 : (int32_t)t;
            }
            // (a) once per iteration.  The loop ends at the break below, on one LDS word that all four waves read behind this
            // barrier, so all of them leave in the same iteration.
            __syncthreads();
            const int32_t tk = rfl(s_pticket);
            if (tk < 0) break;
            uint32_t x = (uint32_t)tk;
            do { x = bij_mix(x, p.pbij_mask, p.pbij_shift, p.bij_key); } while (x >= (uint32_t)n_pchunks);
            const int32_t pc = rfl((int)x);
            const int32_t r0 = rfl(p.prow0[pc]), nr = rfl(p.prow0[pc + 1]) - r0;
            if (tid < nr) s_prow[tid] = p.prows[r0 + tid];                       // 256 threads, at most 4 * RUN_CHUNK = 512 rows
            if (tid + 256 < nr && tid + 256 < 4 * RUN_CHUNK) s_prow[tid + 256] = p.prows[r0 + tid + 256];
            if (tid == 0) s_pn = nr < 4 * RUN_CHUNK ? nr : 4 * RUN_CHUNK;
            // (b) once per iteration that passed the break above (the same iterations in every wave): the rows and their number
            // are in LDS for all four stages
            __syncthreads();
            const int32_t *const pp = p.ppos + (int64_t)pc * 9;
            const int32_t grp = rfl(pp[0]) * 4 + wib, c_lo = rfl(pp[1 + 2 * wib]), c_len = rfl(pp[2 + 2 * wib]);
            const int nx = wib < 3 ? wib + 1 : 0;          // (wave 3 has no next stage: it stores to memory)
            float *ring = nullptr;
            if constexpr (KD > 1) {
                // stage 0's request ring (wave 0 alone reads and fills it; the images of the ordinary walk stay the stages' hand-over)
                static_assert(SET_FLOATS == RING_IMG && IMG_G * 2 == RING_IMG, "an image of the ring is a focus pair's");
                __shared__ float s_ring[(KD + 1) * RING_IMG];
                ring = s_ring;
            }
            const PanelLink pl{s_prow, rfl(s_pn), wib, s_setA + nx * SET_FLOATS, s_setB + nx * SET_FLOATS, ring};
            float *const tr_c = s_tr[wib][0], *const tr_g = s_tr[wib][1];
            float *const setA = s_setA + wib * SET_FLOATS, *const setB = s_setB + wib * SET_FLOATS;
            // the stage of this wave: a compile-time source and sink each (the barriers inside are counted in tile_chunk)
            if (wib == 0) tile_chunk<TG, PAIR_MEM, PAIR_LDS, KD>(p, c_lo, c_len, grp, setA, setB, tr_c, tr_g, s_stage[wib], cost_acc, pl, tid & 63);
            else if (wib < 3) tile_chunk<TG, PAIR_LDS, PAIR_LDS>(p, c_lo, c_len, grp, setA, setB, tr_c, tr_g, s_stage[wib], cost_acc, pl, tid & 63);
            else tile_chunk<TG, PAIR_LDS, PAIR_MEM>(p, c_lo, c_len, grp, setA, setB, tr_c, tr_g, s_stage[wib], cost_acc, pl, tid & 63);
        }
        // The four stages' costs go out through wave 0, summed in stage order: with one block the epoch's cost is then the same
        // bits every run.  (c) once, behind the loop that every wave leaves in the same iteration.
        s_pcost[wib] = cost_acc;
        __syncthreads();
        if (wib == 0) cost_acc = ((s_pcost[0] + s_pcost[1]) + s_pcost[2]) + s_pcost[3];
        else cost_acc = 0.0;
        continue;
    }
    if (wave >= n_workers) continue;       // not a worker: nothing to do in the main queue
    }
    const int lane = tid & 63;
    float *const setA = s_setA + (tid >> 6) * SET_FLOATS, *const setB = s_setB + (tid >> 6) * SET_FLOATS;
    float *setC = nullptr;
    if constexpr (WD > 1) {
        // the third image of the depth-2 walk: an array of its own, like the other two (the wait for one never covers another)
        static_assert(WD == 2, "the walk is one or two nonzeros deep");
        __shared__ float s_setC[4 * SET_FLOATS];
        setC = s_setC + (tid >> 6) * SET_FLOATS;
    }
    bool inr[NCH];                          // lane holds real elements of a row (D % VW == 0)
#pragma unroll
    for (int q = 0; q < NCH; ++q) inr[q] = (lane + q * 64) * VW < D;
    for (;;) {
        unsigned long long ticket = 0;
        if (lane == 0) ticket = atomicAdd(p.queue, 1ull);
        const int64_t tk = ((int64_t)(unsigned)rfl((int)(ticket >> 32)) << 32) | (unsigned)rfl((int)(ticket & 0xFFFFFFFFull));
        if (tk >= p.ticket_end) break;          // (the queue starts at the segment's first ticket, glove_epoch_segment)

        // ---- stage: two nonzeros per lane ------------------------------------------------------
        // key = id of the RESIDENT row (sorted on, kept in registers across a run), oth = id of the
        // STREAMED row.  Blocked order: chunk c of the re-ordered arrays; chunks [0, n_hchunks) are the
        // hub columns in column-major order (resident = context row, hot), the others are the rest of
        // the matrix in row-major order (resident = focus row).  General order (Java permutation /
        // matrix order): the resident side is always the context row, hub columns are keyed ~j.
        int32_t key[2], slot[2], oth[2];
        float ww[2];
        double ll[2];
        int64_t chunk = tk;
        bool res_is_ctx = true;
        int32_t c_lo = 0, c_len = 0, c_meta = -1;
        if (p.blocked) {
            uint32_t x = (uint32_t)tk;
            if (p.order_mode == ORDER_BIJECTION) { do { x = bij_round(x, p); } while ((int64_t)x >= n_chunks); }
            chunk = rfl((int)x);
            res_is_ctx = chunk < p.n_hchunks;
            c_lo = rfl(p.cstart[chunk]); c_len = rfl(p.cstart[chunk + 1]) - c_lo; c_meta = rfl(p.cmeta[chunk]);
            if constexpr (TG > 0) {
                static_assert(VW == 4 && NCH == 1 && OPT == GE_OPT_ADAGRAD && !EMB16 && FAT, "hub tiles: fp32 AdaGrad fat rows of one register chunk");
                if (chunk < p.n_tchunks) {           // a hub tile: c_meta = its group
                    tile_chunk<TG, PAIR_MEM, PAIR_MEM>(p, c_lo, c_len, c_meta, setA, setB, s_tr[tid >> 6][0], s_tr[tid >> 6][1],
                                                       s_stage[tid >> 6], cost_acc, no_link, lane);
                    continue;
                }
            }
        }
        // a hub run is cut every flush_lim nonzeros; a long row's piece (c_meta = its id) runs whole
        const int32_t flush_lim = p.blocked ? (res_is_ctx ? c_meta : RUN_CHUNK) : p.flush_every;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int64_t k = (p.blocked ? (int64_t)c_lo : chunk * RUN_CHUNK) + q * 64 + lane;
            key[q] = KEY_PAD; oth[q] = 0; ww[q] = 0.0f; ll[q] = 0.0;
            slot[q] = q * 64 + lane;
            if (p.blocked) {
                if (q * 64 + lane < c_len) { key[q] = p.bA[k]; oth[q] = p.bB[k]; ww[q] = p.W[k]; ll[q] = p.L[k]; }
            } else if (k < p.N) {
                const int64_t idx = map_index(p, k);
                key[q] = p.J[idx]; oth[q] = p.I[idx]; ww[q] = p.W[idx]; ll[q] = p.L[idx];
            }
        }
        const int n_valid = rfl(__popcll(__ballot(key[0] != KEY_PAD)) + __popcll(__ballot(key[1] != KEY_PAD)));

        // ---- bitonic sort of (key, slot) over positions pos = q*64 + lane ---------------------
#pragma unroll
        for (int k2 = 2; k2 <= RUN_CHUNK; k2 <<= 1) {
#pragma unroll
            for (int j2 = k2 >> 1; j2 >= 1; j2 >>= 1) {
                if (j2 == 64) {
                    if (key[0] > key[1] || (key[0] == key[1] && slot[0] > slot[1])) {   // k2 == 128: ascending everywhere
                        const int32_t tkk = key[0], ts = slot[0];
                        key[0] = key[1]; slot[0] = slot[1]; key[1] = tkk; slot[1] = ts;
                    }
                } else {
#pragma unroll
                    for (int q = 0; q < 2; ++q) {
                        const int pos = q * 64 + lane;
                        const int32_t pk = __shfl_xor(key[q], j2, 64);
                        const int32_t ps = __shfl_xor(slot[q], j2, 64);
                        const bool asc = (pos & k2) == 0;
                        const bool lower = (lane & j2) == 0;
                        // total order (key, slot): the walk order is the STABLE sort of the chunk by resident row
                        const bool p_less = pk < key[q] || (pk == key[q] && ps < slot[q]);
                        const bool take = (asc == lower) ? p_less : !p_less;
                        if (take) { key[q] = pk; slot[q] = ps; }
                    }
                }
            }
        }

        // ---- table roles for this chunk (wave-uniform) ------------------------------------------
        // The update is symmetric in the two sides: A = resident, B = streamed.
        float *const A_rows = res_is_ctx ? p.context : p.focus, *const A_gs = res_is_ctx ? p.gsc : p.gsf;
        float *const A_bias = res_is_ctx ? p.cbias : p.fbias,  *const A_gsb = res_is_ctx ? p.gscb : p.gsfb;
        float *const B_rows = res_is_ctx ? p.focus : p.context, *const B_gs = res_is_ctx ? p.gsf : p.gsc;
        float *const B_bias = res_is_ctx ? p.fbias : p.cbias,  *const B_gsb = res_is_ctx ? p.gsfb : p.gscb;
        float *const A_m2 = res_is_ctx ? p.m2c : p.m2f,  *const A_m2b = res_is_ctx ? p.m2cb : p.m2fb;     // MOM only
        float *const B_m2 = res_is_ctx ? p.m2f : p.m2c,  *const B_m2b = res_is_ctx ? p.m2fb : p.m2cb;

        // ---- sequential walk ---------------------------------------------------------------------
        // Software pipeline: while nonzero `pos` is computed, the streamed rows of pos+1 and (when the
        // resident row changes there) its resident rows are already in flight.  They are requested BEFORE
        // this nonzero's stores, so waiting for them never waits for a store to retire.
        int32_t cur_id = 0; bool cur_hot = false;
        bool cur_a32 = !EMB16, n_a32 = !EMB16;       // EMB16: resident parameter row lives in hub32 (fp32) for hub chunks
        VT a[NCH], ga[NCH], ha[NCH], a0[NCH], ga0[NCH];     // ha = second moment (MOM); ga0 = gradSq as read (AdaGrad)
        float ab = 0.0f, gab = 0.0f, hab = 0.0f;
        // the resident rows' resources are rebuilt from the row id where they are used (once per run): kept in SGPRs across the
        // walk they cost 24 registers, and what does not fit there spills into vector registers
        int32_t cur_slot = 0, n_slot = 0;            // EMB16 hub chunk: the row's slot in hub32; else the row id
        auto res_rows = [&](int32_t id, int32_t slot, bool a32) -> __amdgpu_buffer_rsrc_t {
            if constexpr (EMB16) {
                if (a32) return make_rsrc(p.hub32 + (int64_t)slot * D, (uint32_t)D * 4u);      // fp32 master rows are plain
                return make_rsrc(reinterpret_cast<uint16_t *>(A_rows) + (int64_t)id * p.ES, (uint32_t)p.D * 2u);
            } else return make_rsrc(A_rows + (int64_t)id * DS, row_bytes);
        };
        auto res_gs = [&](int32_t id) { return make_rsrc(A_gs + (int64_t)id * DS, row_bytes); };
        auto res_m2 = [&](int32_t id) { return make_rsrc(A_m2 + (int64_t)id * DS, MOM ? row_bytes : 0u); };

        auto close_run = [&]() {
            // How a run's result leaves the registers:
            //   STORE   the run owns its rows (whole focus rows of a row chunk; every run of the general order on an
            //           ordinary column): rows, accumulators and bias are stored.
            //   ATOMIC  the row is shared with other workers (hub column, piece of a long focus row) and takes float
            //           atomics: the run's DELTA is added, so no worker overwrites another worker's run.
            //   RMW     a shared FOCUS row that cannot take float atomics (bf16 storage; Adam / AMSGrad): the row is re-read,
            //           the delta added and the sum stored -- the race window shrinks from the run to these few instructions.
            // Adam / AMSGrad take steps of about the learning rate whatever the gradient's size, so concurrent HUB runs must
            // not ADD their moves (measured: the cost climbs again after a few epochs); they are merged last-writer-wins,
            // parameters and moments alike, which is exactly the Java race.  The run is still cut and re-read every
            // flush_lim nonzeros, so workers on one hub stay within that many updates of each other.
            const __amdgpu_buffer_rsrc_t rs_a = res_rows(cur_id, cur_slot, cur_a32), rs_ga = res_gs(cur_id), rs_ha = res_m2(cur_id);
            const bool store_all = !cur_hot || (MOM && res_is_ctx);
            const bool rmw_row = !store_all && !res_is_ctx && (MOM || (EMB16 && !cur_a32));
            if (store_all || (rmw_row && MOM)) {
                if constexpr (FAT) {                       // the bias goes out with its row
#pragma unroll
                    for (int q = 0; q < NCH; ++q)
                        if (q == bl_q && lane == bl_lane) {
                            if (store_all) comp<VW>(BIAS_IN_ACC ? ga[q] : a[q], BIAS_C) = ab;
                            comp<VW>(ga[q], 0) = gab;
                            if constexpr (MOM) comp<VW>(ha[q], 0) = hab;
                        }
                }
#pragma unroll
                for (int q = 0; q < NCH; ++q) {
                    if (store_all) {
                        if (EMB16 && !cur_a32) emb_store(a[q], rs_a, q);
                        else buf_store<VW>(a[q], rs_a, (lane + q * 64) * VW * 4);
                    }
                    buf_store<VW>(ga[q], rs_ga, (lane + q * 64) * VW * 4);
                    if constexpr (MOM) buf_store<VW>(ha[q], rs_ha, (lane + q * 64) * VW * 4);
                }
            }
            if (rmw_row) {
#pragma unroll
                for (int q = 0; q < NCH; ++q) {
                    VT cur = (EMB16 && !cur_a32) ? emb_load(rs_a, q) : buf_load<VW, AUX_SC1>(rs_a, (lane + q * 64) * VW * 4);
#pragma unroll
                    for (int t = 0; t < VW; ++t) comp<VW>(cur, t) += comp<VW>(a[q], t) - comp<VW>(a0[q], t);
                    if (EMB16 && !cur_a32) emb_store(cur, rs_a, q);
                    else buf_store<VW>(cur, rs_a, (lane + q * 64) * VW * 4);
                }
            }
            if (!store_all && !MOM) {
                // Publish the run's delta with float atomics.  Lane L holds elements [VW*L, VW*L+VW);
                // staged through this wave's LDS strip so that every atomic wave-instruction covers 64
                // CONSECUTIVE dwords (256 B = four 64-B memory-side requests instead of sixteen).
                float *tr_c = s_tr[tid >> 6][0], *tr_g = s_tr[tid >> 6][1];
#pragma unroll
                for (int q = 0; q < NCH; ++q) {
                    VT dc, dg;
#pragma unroll
                    for (int t = 0; t < VW; ++t) {
                        comp<VW>(dc, t) = comp<VW>(a[q], t) - comp<VW>(a0[q], t);
                        comp<VW>(dg, t) = comp<VW>(ga[q], t) - comp<VW>(ga0[q], t);
                    }
                    if (!rmw_row) *reinterpret_cast<VT *>(tr_c + (lane + q * 64) * VW) = dc;
                    *reinterpret_cast<VT *>(tr_g + (lane + q * 64) * VW) = dg;
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
                for (int k = 0; k < NCH * VW; ++k) {
                    const int e = lane + k * 64;          // element index; past the row the buffer check drops it
                    if (!rmw_row) __builtin_amdgcn_raw_ptr_buffer_atomic_fadd_f32(tr_c[e], rs_a, e * 4, 0, 0);
                    __builtin_amdgcn_raw_ptr_buffer_atomic_fadd_f32(tr_g[e], rs_ga, e * 4, 0, 0);
                }
                __builtin_amdgcn_wave_barrier();
            }
            // The bias takes AdaGrad steps WITHOUT a learning rate (Adagrad.java:88-89): one run alone
            // already moves it most of the way, so concurrent runs must not add up.  The scalars are
            // merged last-writer-wins (what the Java race does), written through (sc1) like every table.
            if constexpr (FAT) {
                if (lane == 0 && !store_all) {             // the rows did not go out whole: the bias slot of each row is stored on its own
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, ab), BIAS_IN_ACC ? rs_ga : rs_a, (D + BIAS_C) * 4, 0, AUX_SC1);
                    if (!MOM) __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, gab), rs_ga, D * 4, 0, AUX_SC1);
                }
            } else if (lane == 0) {
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, ab), make_rsrc(A_bias + cur_id, 4), 0, 0, AUX_SC1);
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, gab), make_rsrc(A_gsb + cur_id, 4), 0, 0, AUX_SC1);
                if constexpr (MOM) __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, hab), make_rsrc(A_m2b + cur_id, 4), 0, 0, AUX_SC1);
            }
        };

        // decoded next nonzero + its prefetched rows
        int32_t n_oth = 0, n_key = KEY_PAD; float n_w = 0.0f; double n_l = 0.0;
        VT aN[NCH], gaN[NCH], haN[NCH]; float abN = 0.0f, gabN = 0.0f, habN = 0.0f;
        auto decode = [&](int pos) {
            const int q = pos >> 6, ln = pos & 63;
            n_key = __builtin_amdgcn_readlane(q ? key[1] : key[0], ln);
            const int sl = __builtin_amdgcn_readlane(q ? slot[1] : slot[0], ln);
            const int sq = sl >> 6, sln = sl & 63;
            n_oth = __builtin_amdgcn_readlane(sq ? oth[1] : oth[0], sln);
            n_w = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, sq ? ww[1] : ww[0]), sln));
            const long long lb = __builtin_bit_cast(long long, sq ? ll[1] : ll[0]);
            const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(lb & 0xFFFFFFFFll), sln);
            const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(lb >> 32), sln);
            n_l = __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
        };
        // WD 2: the fields of the nonzero behind the next one, decoded with the next one's left as they are.  (A wrapper, and named
        // in discarded branches only where WD is 1: decode() itself and what the walk's lambdas capture stay what they were, and
        // with them every older kernel's code, DESIGN.md 3.1.4.  The same goes for request_ahead and the third image below.)
        int32_t m_oth = 0, m_key = KEY_PAD; float m_w = 0.0f; double m_l = 0.0;
        auto decode_ahead = [&](int pos) {
            const int32_t k = n_key, o = n_oth; const float w = n_w; const double l = n_l;
            decode(pos);
            m_key = n_key; m_oth = n_oth; m_w = n_w; m_l = n_l;
            n_key = k; n_oth = o; n_w = w; n_l = l;
        };
        // Requests the streamed rows of nonzero n_oth into set SET (0: A, 1: B, 2: C).  `live` false: the same instructions against
        // zero-sized resources -- nothing is read, zeros arrive.  Issued on EVERY step, so that the number of memory
        // instructions between a request and its use is the same on every path and the wait can be counted.
        auto request_streamed = [&](auto SET, const bool live) {
            const uint32_t rbytes = live ? row_bytes : 0u, ebytes = live ? (uint32_t)p.D * 2u : 0u, four = live ? 4u : 0u;
            __amdgpu_buffer_rsrc_t rb;
            if constexpr (EMB16) rb = make_rsrc(reinterpret_cast<uint16_t *>(B_rows) + (int64_t)n_oth * p.ES, ebytes);
            else rb = make_rsrc(B_rows + (int64_t)n_oth * DS, rbytes);
            const __amdgpu_buffer_rsrc_t rg = make_rsrc(B_gs + (int64_t)n_oth * DS, rbytes);
            const __amdgpu_buffer_rsrc_t rh = make_rsrc(B_m2 + (int64_t)n_oth * DS, MOM ? rbytes : 0u);
            float *img = decltype(SET)::value ? setB : setA;
            if constexpr (WD > 1) { if constexpr (decltype(SET)::value == 2) img = setC; }
#pragma unroll
            for (int j = 0; j < (IMG_R / IMG) * N_Q; ++j)
                load_to_lds<(VW == 4 ? 16 : 4)>(rb, img + j * (IMG / N_Q), (lane + j * 64) * DMAW);
#pragma unroll
            for (int j = 0; j < NCH * N_Q; ++j) {
                load_to_lds<(VW == 4 ? 16 : 4)>(rg, img + IMG_G + j * (IMG / N_Q), (lane + j * 64) * DMAW);
                if constexpr (MOM) load_to_lds<(VW == 4 ? 16 : 4)>(rh, img + IMG_H + j * (IMG / N_Q), (lane + j * 64) * DMAW);
            }
            if constexpr (!FAT) {                  // lane 0 is the one lane inside these 4-byte resources
                load_to_lds<4>(make_rsrc(B_bias + n_oth, four), img + IMG_B, lane * 4);
                load_to_lds<4>(make_rsrc(B_gsb + n_oth, four), img + IMG_B + 64, lane * 4);
                if constexpr (MOM) load_to_lds<4>(make_rsrc(B_m2b + n_oth, four), img + IMG_B + 128, lane * 4);
            }
            asm volatile("" ::: "memory");          // issued here, not where the scheduler would like them
        };
        // WD 2: the same for the nonzero behind the next one
        auto request_ahead = [&](auto SET, const bool live) {
            const int32_t o = n_oth;
            n_oth = m_oth; request_streamed(SET, live); n_oth = o;
        };
        // waits until everything requested so far has arrived
        auto settle = [&]() { __builtin_amdgcn_s_waitcnt(wait_vmcnt(0)); asm volatile("" ::: "memory"); };
        auto request_resident = [&]() {
            const int32_t id = n_key < 0 ? ~n_key : n_key;
            n_slot = id;
            if constexpr (EMB16) {
                n_a32 = res_is_ctx && p.hot_enabled != 0;                  // hub chunk: fp32 master row
                if (n_a32) n_slot = rfl(p.hub_index[id]);
            }
            const __amdgpu_buffer_rsrc_t rsN_a = res_rows(id, n_slot, n_a32), rsN_ga = res_gs(id), rsN_ha = res_m2(id);
#pragma unroll
            for (int q = 0; q < NCH; ++q) {
                if constexpr (EMB16) {
                    // the row lives in one of two places (bf16 table / fp32 master row of a hub): BOTH loads are issued, the one that
                    // does not apply against a zero-sized resource (no traffic, zeros arrive) -- an `if` around either would put a
                    // path with no load at all in front of the hand-counted wait of the first step (tests/isa_waits.py)
                    const __amdgpu_buffer_rsrc_t r16 = make_rsrc(reinterpret_cast<uint16_t *>(A_rows) + (int64_t)id * p.ES, n_a32 ? 0u : (uint32_t)p.D * 2u);
                    const __amdgpu_buffer_rsrc_t r32 = make_rsrc(p.hub32 + (int64_t)n_slot * D, n_a32 ? (uint32_t)D * 4u : 0u);
                    VT v16 = emb_load(r16, q), v32 = buf_load<VW, AUX_SC1>(r32, (lane + q * 64) * VW * 4);
#pragma unroll
                    for (int t = 0; t < VW; ++t) comp<VW>(aN[q], t) = n_a32 ? comp<VW>(v32, t) : comp<VW>(v16, t);
                } else aN[q] = buf_load<VW, AUX_SC1>(rsN_a, (lane + q * 64) * VW * 4);
                gaN[q] = buf_load<VW, AUX_SC1>(rsN_ga, (lane + q * 64) * VW * 4);
                if constexpr (MOM) haN[q] = buf_load<VW, AUX_SC1>(rsN_ha, (lane + q * 64) * VW * 4);
            }
            if constexpr (!FAT) {
                abN  = buf_load_f32(make_rsrc(A_bias + id, 4), 0, true);
                gabN = buf_load_f32(make_rsrc(A_gsb + id, 4), 0, true);
                if constexpr (MOM) habN = buf_load_f32(make_rsrc(A_m2b + id, 4), 0, true);
            }
        };

        bool open_new = true;
        int run_len = 0;
        // the staged nonzeros have arrived before the walk starts: inside it only row traffic is pending
        asm volatile("" : "+v"(oth[0]), "+v"(oth[1]), "+v"(ww[0]), "+v"(ww[1]), "+v"(ll[0]), "+v"(ll[1]));
        bool again = false, recut = false;
        bool again2 = false;                  // WD 2: `again` of the step behind this one
        // One nonzero.  CUR (0 / 1) names the set that holds its streamed rows; the other set is requested for the next one first
        // thing, before this step waits for anything.  (WD 2: CUR is 0 / 1 / 2, and the set requested is the one that held the
        // previous nonzero's rows, for the nonzero behind the next one.)
        auto step = [&](const int pos, auto CUR) {
            constexpr std::integral_constant<int, WD == 1 ? 1 - decltype(CUR)::value : (decltype(CUR)::value + 2) % 3> NXT{};
            const int32_t b_id = n_oth, skey = n_key;
            const float w = n_w; const double l = n_l;
            // the previous nonzero had the same streamed row: what was requested before its stores is stale.  Re-read behind
            // them (same wave, same address: in order) and wait right here, so that on the common path the set is known to be
            // older than those stores and the wait for it leaves them in flight.
            // (WD 2: the set was requested in front of the stores of the two previous nonzeros, and is stale if either had this row.)
            if (again) { request_streamed(CUR, true); settle(); again = false; }
            // the previous step cut its run and this one continues on the same resident row: requested here, behind that publish
            if (recut) { request_resident(); recut = false; }
            if (open_new) {                       // the scalars of a new run; its rows follow below
                cur_id = skey < 0 ? ~skey : skey;
                // shared = other workers may hold this row too: hub columns (context side), pieces of a long focus row
                cur_hot = p.blocked ? (res_is_ctx ? p.hot_enabled != 0 : cur_id == c_meta) : skey < 0;
                cur_slot = n_slot;
                cur_a32 = n_a32;
                run_len = 0;
            }
            const bool last = pos + 1 >= n_valid;
            bool next_new = false;
            if constexpr (WD == 1) {
                if (!last) {
                    decode(pos + 1);
                    again = n_oth == b_id;
                    // a long hub run is cut every flush_lim nonzeros: publish the delta, re-read what the other workers published
                    next_new = n_key != skey || (cur_hot && run_len + 1 >= flush_lim);
                }
                request_streamed(NXT, !last);
            } else {
                // the next nonzero was decoded a step ago, and whether its set is stale was decided then
                if (!last) {
                    n_key = m_key; n_oth = m_oth; n_w = m_w; n_l = m_l;
                    again = again2;
                    next_new = n_key != skey || (cur_hot && run_len + 1 >= flush_lim);
                }
                // the one behind it: its set is requested in front of this nonzero's stores and the next one's
                const bool ahead = pos + 2 < n_valid;           // (no request crosses the end of the chunk)
                again2 = false;
                if (ahead) {
                    decode_ahead(pos + 2);
                    again2 = m_oth == n_oth || m_oth == b_id;
                }
                request_ahead(NXT, ahead);
            }
            if (open_new) {
#pragma unroll
                for (int q = 0; q < NCH; ++q) {
                    a[q] = aN[q]; ga[q] = gaN[q]; a0[q] = aN[q];
                    if constexpr (MOM) ha[q] = haN[q]; else ga0[q] = gaN[q];
                }
                ab = abN; gab = gabN; hab = habN;
                if constexpr (FAT) {
#pragma unroll
                    for (int q = 0; q < NCH; ++q)
                        if (q == bl_q) {
                            ab  = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, comp<VW>(BIAS_IN_ACC ? ga[q] : a[q], BIAS_C)), bl_lane));
                            gab = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, comp<VW>(ga[q], 0)), bl_lane));
                            if constexpr (MOM) hab = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, comp<VW>(ha[q], 0)), bl_lane));
                        }
                }
            }
            // A cut keeps the resident row: the next run must start from what memory holds once THIS run is published (its own
            // delta or stores included -- with one worker the walk stays a sequential program for any flush limit), so the row
            // is requested behind close_run(), first thing in the next step, instead (same wave, same address: in order).
            recut = next_new && n_key == skey;
            if (next_new && !recut) request_resident();     // after the copies above: it refills aN
            // this nonzero's streamed rows
            VT bl[NCH], gbl[NCH], hbl[NCH];
            float bb = 0.0f, gbb = 0.0f, hbb = 0.0f;
            // The wait is counted by hand (the compiler's own bookkeeping of loads into LDS loses them across the loop's
            // back edge).  Memory instructions complete in order, and behind this set's request at least N_AFTER more
            // have been issued on every path: the previous step's stores, one per table and register chunk (never
            // skipped: lane 0 of every chunk holds row elements), or before the first step the resident rows' loads, one per
            // table and chunk as well; then the request for the other set a few lines up.
            constexpr int N_TAB = NCH * (2 + (MOM ? 1 : 0)) + (FAT ? 0 : 2 + (MOM ? 1 : 0));
            constexpr int N_DMA = ((IMG_R / IMG) + NCH * (1 + (MOM ? 1 : 0))) * N_Q + (FAT ? 0 : 2 + (MOM ? 1 : 0));
            // (WD 2: behind this set's request stand the stores of the two previous steps and the requests of the previous step and of
            // this one; before the first steps the chunk's prologue issues as many, see below.)
            constexpr int N_AFTER = WD * (N_TAB + N_DMA);
            static_assert(N_AFTER < 64, "vmcnt is a 6-bit counter");
            __builtin_amdgcn_s_waitcnt(wait_vmcnt(N_AFTER));       // the builtin, not asm text: the compiler's bookkeeping sees it
            asm volatile("" ::: "memory");
            const float *img = decltype(CUR)::value ? setB : setA;
            if constexpr (WD > 1) { if constexpr (decltype(CUR)::value == 2) img = setC; }
#pragma unroll
            for (int q = 0; q < NCH; ++q) {
                if constexpr (EMB16) bl[q] = widen_bf16x4(*reinterpret_cast<const float2 *>(img + (lane + q * 64) * 2));
                else bl[q] = *reinterpret_cast<const VT *>(img + (lane + q * 64) * VW);
                gbl[q] = *reinterpret_cast<const VT *>(img + IMG_G + (lane + q * 64) * VW);
                if constexpr (MOM) hbl[q] = *reinterpret_cast<const VT *>(img + IMG_H + (lane + q * 64) * VW);
            }
            if constexpr (!FAT) { bb = img[IMG_B]; gbb = img[IMG_B + 64]; if constexpr (MOM) hbb = img[IMG_B + 128]; }
            VT (&b)[NCH] = bl, (&gb)[NCH] = gbl, (&hb)[NCH] = hbl;
            if constexpr (FAT) {
#pragma unroll
                for (int q = 0; q < NCH; ++q)
                    if (q == bl_q) {
                        bb  = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, comp<VW>(BIAS_IN_ACC ? gb[q] : b[q], BIAS_C)), bl_lane));
                        gbb = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, comp<VW>(gb[q], 0)), bl_lane));
                        if constexpr (MOM) hbb = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, comp<VW>(hb[q], 0)), bl_lane));
                    }
            }
            // dot product
            float part = 0.0f;
#pragma unroll
            for (int q = 0; q < NCH; ++q)
                if (inr[q]) {
#pragma unroll
                    for (int t = 0; t < VW; ++t) part = __builtin_fmaf(comp<VW>(a[q], t), comp<VW>(b[q], t), part);
                }
            part = wave_sum(part);
            const float ic = (float)((double)part + ((double)(ab + bb) - l));
            const float wc = w * ic;
            cost_acc += (0.5 * (double)wc) * (double)ic;
            const float wlr = wc * lr;
            const __amdgpu_buffer_rsrc_t rb = emb_rsrc(B_rows, b_id);
            const __amdgpu_buffer_rsrc_t rg = make_rsrc(B_gs + (int64_t)b_id * DS, row_bytes);
            const __amdgpu_buffer_rsrc_t rh = make_rsrc(B_m2 + (int64_t)b_id * DS, MOM ? row_bytes : 0u);
            // the streamed row's bias takes its step here and goes out with the row (FAT), see below for the arithmetic
            float nbb_fat = 0.0f, ngbb_fat = 0.0f, nhbb_fat = 0.0f;
            if constexpr (FAT) {
                if constexpr (!MOM) { nbb_fat = bb - wc * __frsqrt_rn(gbb); ngbb_fat = gbb + wc * wc; }
                else { float m = gbb, v = hbb; nbb_fat = bb - moment_step(wc, m, v); ngbb_fat = m; nhbb_fat = v; }
            }
#pragma unroll
            for (int q = 0; q < NCH; ++q) {
                // one store instruction per table covers the row's lanes AND the lane that holds the bias
                const bool is_bl = FAT && q == bl_q && lane == bl_lane;
                const bool tail = FAT && !inr[q] && (lane + q * 64) * VW < p.RW;     // the bias lane and the padding behind it: stored too, whole lines go out
                // The stores below are issued on EVERY path and by every lane: lanes past the row are dropped by the descriptor's
                // bounds check, not by the exec mask.  A store under `if (lane in range)` sits behind an s_cbranch_execz the
                // hand-counted wait further up cannot see past (tests/isa_waits.py counts the instructions on every path).
                {
                    VT ob{}, ogb{}, ohb{};
                    if (tail) {
                        if (is_bl) {
                            comp<VW>(ogb, 0) = ngbb_fat; comp<VW>(ohb, 0) = nhbb_fat;
                            comp<VW>(BIAS_IN_ACC ? ogb : ob, BIAS_C) = nbb_fat;     // (bf16: this lane's row store lies past the bf16 row and is dropped)
                        }
                    } else if (inr[q]) {
#pragma unroll
                        for (int t = 0; t < VW; ++t) {
                            const float av = comp<VW>(a[q], t), bv = comp<VW>(b[q], t);
                            const float grad_b = wc * av, grad_a = wc * bv;
                            if constexpr (!MOM) {
                                const float sa = comp<VW>(ga[q], t), sb = comp<VW>(gb[q], t);
                                comp<VW>(ob, t)    = __builtin_fmaf(-(wlr * av), __frsqrt_rn(sb), bv);
                                comp<VW>(ogb, t)   = __builtin_fmaf(grad_b, grad_b, sb);
                                comp<VW>(a[q], t)  = __builtin_fmaf(-(wlr * bv), __frsqrt_rn(sa), av);
                                comp<VW>(ga[q], t) = __builtin_fmaf(grad_a, grad_a, sa);
                            } else {
                                float m = comp<VW>(gb[q], t), v = comp<VW>(hb[q], t);
                                comp<VW>(ob, t) = bv - moment_step(grad_b, m, v);
                                comp<VW>(ogb, t) = m; comp<VW>(ohb, t) = v;
                                comp<VW>(a[q], t) = av - moment_step(grad_a, comp<VW>(ga[q], t), comp<VW>(ha[q], t));
                            }
                        }
                    }
                    emb_store(ob, rb, q);
                    buf_store<VW>(ogb, rg, (lane + q * 64) * VW * 4);
                    if constexpr (MOM) buf_store<VW>(ohb, rh, (lane + q * 64) * VW * 4);
                }
            }
            if constexpr (!MOM) {
                const float w2 = wc * wc;
                if constexpr (!FAT) {             // no learning rate on the biases (Adagrad.java:88-89); every lane issues the store, the
                                                  // 4-byte descriptor keeps lane 0's (no exec-mask branch in front of a counted instruction)
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, bb - wc * __frsqrt_rn(gbb)), make_rsrc(B_bias + b_id, 4), lane * 4, 0, AUX_SC1);
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, gbb + w2), make_rsrc(B_gsb + b_id, 4), lane * 4, 0, AUX_SC1);
                }
                ab = ab - wc * __frsqrt_rn(gab);
                gab = gab + w2;
            } else {                      // Adam.java:127-145: the biases take the same moment step with gradient wc
                const float nbb = bb - moment_step(wc, gbb, hbb);
                if constexpr (!FAT) {
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, nbb), make_rsrc(B_bias + b_id, 4), lane * 4, 0, AUX_SC1);
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, gbb), make_rsrc(B_gsb + b_id, 4), lane * 4, 0, AUX_SC1);
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, hbb), make_rsrc(B_m2b + b_id, 4), lane * 4, 0, AUX_SC1);
                }
                ab = ab - moment_step(wc, gab, hab);
            }
            ++run_len;
            if (last || next_new) close_run();
            open_new = next_new;
        };
        constexpr std::integral_constant<int, 0> SET_A{};
        constexpr std::integral_constant<int, 1> SET_B{};
        if constexpr (WD == 1) {
            if (n_valid > 0) { decode(0); request_streamed(SET_A, true); request_resident(); }
            for (int pos = 0; pos < n_valid; pos += 2) {
                step(pos, SET_A);
                if (pos + 1 < n_valid) step(pos + 1, SET_B);
            }
        } else {
            constexpr std::integral_constant<int, 2> SET_C{};
            if (n_valid > 0) {
                // Step 0 reads set A behind the same count as every later step: behind its request stand a step's stores against a
                // zero-sized resource (nothing is written), the request of nonzero 1, the resident rows' loads in the place of a
                // step's stores, and step 0's own request.  Step 1 finds those loads, step 0's request and stores and its own
                // request behind the request of nonzero 1.
                decode(0);
                request_streamed(SET_A, true);
                constexpr int N_TAB = NCH * (2 + (MOM ? 1 : 0)) + (FAT ? 0 : 2 + (MOM ? 1 : 0));       // as in step
#pragma unroll
                for (int j = 0; j < N_TAB; ++j) __builtin_amdgcn_raw_buffer_store_b32(lane, make_rsrc(B_rows, 0u), lane * 4, 0, AUX_SC1);
                asm volatile("" ::: "memory");
                const bool two = n_valid > 1;
                if (two) { decode_ahead(1); again2 = m_oth == n_oth; }
                request_ahead(SET_B, two);
                request_resident();
            }
            // (one way out per step, so that no path leads from the first step to the third past the second: the compiler counts
            // the instructions behind set C's request along every path it sees, and would wait for fewer than there are)
            for (int pos = 0; pos < n_valid; pos += 3) {
                step(pos, SET_A);
                if (pos + 1 >= n_valid) break;
                step(pos + 1, SET_B);
                if (pos + 2 >= n_valid) break;
                step(pos + 2, SET_C);
            }
        }
    }
    }
    if ((tid & 63) == 0 && cost_acc != 0.0) atomicAdd(p.cost_out, cost_acc);
}

template <int VW, int NCH, int OPT, bool EMB16, bool FAT>
__global__ __launch_bounds__(256, (NCH == 1 && VW == 4 && OPT == GE_OPT_ADAGRAD) ? 5 : 1) void k_adagrad_runs(GloveParams p, int32_t n_workers) {
    epoch_walk<VW, NCH, OPT, EMB16, FAT, 0>(p, n_workers);
}
// The epoch of a handle whose layout has hub tiles: three wavefronts per SIMD (at D = 200 the walk runs as fast with three as with
// five), which leaves 168 registers for the G resident pairs.  G = 4 is the largest group the compiler keeps out of
// scratch beside the ordinary walk: it takes all 168 registers of three waves per SIMD, with nothing to spare (G = 6 spills 140 bytes
// per lane, G = 8 324: DESIGN.md 3.1).  A compiler that needs one register more spills; tests/test_hub_tiles_resources.py then fails
// (no scratch, <= 168) -- the way out is then fewer live values in tile_chunk, or G = 3, not a spill.
constexpr int TILE_G = 4;                 // columns per hub-tile group: the one instance that is built
template <int G>
__global__ __launch_bounds__(256, 3) void k_epoch_tiles(GloveParams p, int32_t n_workers) {
    epoch_walk<4, 1, GE_OPT_ADAGRAD, false, true, G>(p, n_workers);
}
// The epoch of a handle whose layout has hub panels: the walk above, and the panel chunks on the four waves of a
// workgroup.  The same register budget: a stage of the pipeline holds what a tile chunk holds.
__global__ __launch_bounds__(256, 3) void k_epoch_panels(GloveParams p, int32_t n_workers) {
    epoch_walk<4, 1, GE_OPT_ADAGRAD, false, true, TILE_G, true>(p, n_workers);
}
// The panel kernel with stage 0's focus pairs requested RING_K rows ahead: the same sequential program on the
// same layout.  tests/test_hub_ring_resources.py holds its registers, its LDS and its vmcnt(2 RING_K) waits.  RING_K is the
// sweep's choice among 2, 4, 6 (profiles/hub_ring_bench.json; -DGE_RING_K=n builds another depth); LDS bounds it at 9.
#ifndef GE_RING_K
#define GE_RING_K 2
#endif
constexpr int RING_K = GE_RING_K;
static_assert(RING_K >= 2 && 2 * RING_K < 64, "vmcnt is a 6-bit counter");
__global__ __launch_bounds__(256, 3) void k_epoch_ring(GloveParams p, int32_t n_workers) {
    epoch_walk<4, 1, GE_OPT_ADAGRAD, false, true, TILE_G, true, RING_K>(p, n_workers);
}
// The ring kernel with the ordinary walk two nonzeros deep: a worker keeps two streamed pairs in flight, in three
// images per wave.  The same sequential program on the same layout; tests/test_deep_walk_resources.py holds its registers, its LDS
// (the ring kernel's and a third image per wave) and its vmcnt(8) waits.
__global__ __launch_bounds__(256, 3) void k_epoch_walk2(GloveParams p, int32_t n_workers) {
    epoch_walk<4, 1, GE_OPT_ADAGRAD, false, true, TILE_G, true, RING_K, 2>(p, n_workers);
}

// Placement probe: what an epoch does to a record table -- whole records read and written back at random rows, sc1 like the trainer's
// accesses, one wavefront per stream of rows.  The values are written back unchanged (the table is not yet initialised and nobody
// else touches it), so the only result is the time.
__global__ __launch_bounds__(256) void k_probe_records(float *tab, int64_t rows, int64_t ds, int32_t rec_bytes, int32_t iters, uint32_t seed) {
    const int lane = threadIdx.x & 63;
    uint32_t x = (uint32_t)(blockIdx.x * 4 + (threadIdx.x >> 6)) * 0x9E3779B1u + seed;       // the same in every lane of a wavefront
    for (int it = 0; it < iters; ++it) {
        x = x * 1664525u + 1013904223u;
        const int64_t r = (int64_t)(((uint64_t)(x >> 4) * (uint64_t)rows) >> 28);
        const __amdgpu_buffer_rsrc_t rs = make_rsrc(tab + r * ds, (uint32_t)rec_bytes);
        float4 v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = buf_load<4, AUX_SC1>(rs, (lane + q * 64) * 16);        // past the record: masked by the resource
#pragma unroll
        for (int q = 0; q < 4; ++q) buf_store<4>(v[q], rs, (lane + q * 64) * 16);
    }
}

using hogwild_fn = void (*)(GloveParams, int32_t);

// One wavefront spans a row: 64 lanes x VW floats x NCH chunks >= D.  A row carries its bias at element [D] (fat rows; bf16 rows:
// behind the accumulator row) when the lane that would hold it lies in the row's last 64-lane chunk.  An odd dim, or twice an odd
// number, never fills its 64-lane chunks, so VW 1 and VW 2 exist with fat rows only.
struct HogwildKernel { hogwild_fn fn; int vw, nch; bool fat; };
template <int VW, int OPT, bool BF16, bool FAT>
hogwild_fn pick_nch(int nch) {
    static_assert(VW == 4 || FAT, "no dim reaches VW < 4 without fat rows");
    switch (nch) {
        case 1: return k_adagrad_runs<VW, 1, OPT, BF16, FAT>;
        case 2: return k_adagrad_runs<VW, 2, OPT, BF16, FAT>;
        case 3: return k_adagrad_runs<VW, 3, OPT, BF16, FAT>;
        case 4: return k_adagrad_runs<VW, 4, OPT, BF16, FAT>;
        default: return nullptr;
    }
}
template <int OPT>
hogwild_fn pick_f32(int vw, int nch, bool fat) {
    if (!fat) return pick_nch<4, OPT, false, false>(nch);
    return vw == 4 ? pick_nch<4, OPT, false, true>(nch) : vw == 2 ? pick_nch<2, OPT, false, true>(nch) : pick_nch<1, OPT, false, true>(nch);
}
HogwildKernel pick_hogwild(int D, int opt, bool emb16) {
    const int vw = (D % 4 == 0) ? 4 : (D % 2 == 0) ? 2 : 1;
    const bool fat = ((D / vw) % 64) != 0;                   // false only with vw == 4: D is then a multiple of 64 vw
    const int nch = (D + 64 * vw - 1) / (64 * vw);           // the bias lane of a fat row lies inside the last chunk
    hogwild_fn fn = emb16 ? (fat ? pick_nch<4, GE_OPT_ADAGRAD, true, true>(nch) : pick_nch<4, GE_OPT_ADAGRAD, true, false>(nch))   // bf16 embeddings: AdaGrad, dim % 4 == 0
                  : opt == GE_OPT_ADAGRAD ? pick_f32<GE_OPT_ADAGRAD>(vw, nch, fat)
                  : opt == GE_OPT_ADAM ? pick_f32<GE_OPT_ADAM>(vw, nch, fat) : pick_f32<GE_OPT_AMSGRAD>(vw, nch, fat);
    return {fn, vw, nch, fat};
}

}  // namespace

// =============================================================================================
// handle
// =============================================================================================
struct ge_glove {
    ge_glove_cfg cfg{};
    int32_t rows = 0;                 // focus rows owned = row_end - row_begin
    float *tab[GE_STATE_COUNT] = {};  // device tables (several may point into one allocation: see `owned`)
    int64_t tab_count[GE_STATE_COUNT] = {};
    std::vector<void *> owned;        // every device allocation of the handle
    int32_t *dI = nullptr, *dJ = nullptr, *dperm = nullptr;
    float *dX = nullptr;
    double *dL = nullptr;             // Hogwild: log term per nonzero
    float *dW = nullptr;              // Hogwild: weight per nonzero
    double *dcost = nullptr;          // Hogwild accumulator (+ the chunk queue word and the panel queue word behind it)
    float *djob = nullptr;            // deterministic: per-job fp32 costs
    std::vector<int32_t> perm;        // host copy, GE_SHUFFLE_JAVA
    ge::JavaRandom rng{0};
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    float last_ms = 0.0f;
    int32_t last_launches = 0;
    int num_cus = 256;
    HogwildKernel hw{};               // Hogwild: the kernel instance and its lane shape (pick_hogwild)
    int hw_blocks_per_cu = 4;
    int hw_blocks = 0;
    int hw_workers = 0;
    bool blocked = false;             // Hogwild + DEVICE shuffle: the layout of ge_layout.h
    ge::BlockedLayout lay;            // its device arrays (bA, bB, L, W, border, cstart, cmeta)
    int64_t n_chunks = 0, n_hchunks = 0, n_tchunks = 0;     // n_hchunks: column-major hub chunks, behind the n_tchunks hub tiles
    int64_t n_pchunks = 0;            // hub panel chunks: a queue of their own, in front of the chunk table's
    int flush_every = RUN_CHUNK;
    bool emb16 = false;               // focus/context stored as bf16 (tab[] pointers then address uint16 data)
    bool fat = false;                 // Hogwild: a row is D + 4 floats with its bias at [D] (pick_hogwild); tab[*BIAS] are null
    int32_t rw = 0;                   // row width of the fp32 row tables in floats (D, or D + 4 when fat)
    int32_t ds = 0;                   // row stride of the fp32 row tables in floats (rw, or a multiple when the tables interleave)
    int32_t e16 = 0;                  // bf16 rows: bf16 elements of a row padded to 16 bytes (what leads a record)
    int32_t es = 0;                   // bf16 rows: bf16 elements between consecutive embedding rows (dim, or 2 * ds inside records)
    int32_t placements = 0;           // allocations tried for the record tables (both sides)
    float place_best_ms = 0.0f, place_worst_ms = 0.0f;
    float *hub32 = nullptr;           // bf16 build: fp32 master rows of the hub columns
    int32_t *dhub_index = nullptr;
    unsigned long long seg_ticket[64] = {};   // first ticket of each segment of a segmented epoch (source of small async copies)
    hipEvent_t seg_ev[128] = {};              // a segmented epoch: events around every segment's launch (created on first use), so that
    int32_t seg_timed = 0;                    //   last_ms is the kernels' own time, the exchanges between them not included
    std::vector<int32_t> host_hub_index;
    int32_t n_hub = 0;
    std::vector<int32_t> host_key;    // general order: sort key per nonzero (what the kernel stages as `key`)
    int32_t hot_cols = 0;
    int64_t hot_nnz = 0, hot_threshold = 0;
    ge::Strata strata;                // GE_MODE_STRATIFIED: the tile layout (ge_strata.h)

    bool hogwild() const { return cfg.mode == GE_MODE_HOGWILD; }
    bool stratified() const { return cfg.mode == GE_MODE_STRATIFIED; }
    bool moments() const { return cfg.opt != GE_OPT_ADAGRAD; }      // Adam / AMSGrad keep M2* next to M1*
    bool interleaved() const { return hogwild() && (cfg.layout_flags & GE_LAYOUT_SEPARATE_TABLES) == 0; }   // a side is one table of records
    template <typename T> hipError_t alloc(T **out, size_t n) {
        hipError_t e = hipMalloc((void **)out, sizeof(T) * std::max<size_t>(n, 1));
        if (e == hipSuccess) owned.push_back((void *)*out);
        return e;
    }
};

namespace {

ge_status check_handle(ge_glove *h) {
    if (!h) return ge::fail(GE_ERR_ARG, "null ge_glove handle");
    hipError_t e = hipSetDevice(h->cfg.device);
    if (e != hipSuccess) return ge::fail(GE_ERR_HIP, "hipSetDevice(%d): %s", h->cfg.device, hipGetErrorString(e));
    return GE_OK;
}
ge_status hip_failed(const char *what, hipError_t e) { return ge::fail(GE_ERR_HIP, "%s failed: %s", what, hipGetErrorString(e)); }

// a device buffer that lives as long as its scope (staging copies of the accessors), unless released to the caller
struct DeviceBuf {
    void *p = nullptr;
    DeviceBuf() = default;
    DeviceBuf(const DeviceBuf &) = delete;
    DeviceBuf &operator=(const DeviceBuf &) = delete;
    ~DeviceBuf() { if (p) (void)hipFree(p); }
    float *f32() const { return static_cast<float *>(p); }
    void *release() { void *q = p; p = nullptr; return q; }
};

// The keyed bijection (bij_round) permutes [0, 2^bits), the smallest power of two that covers `domain`.
void bijection_width(int64_t domain, uint32_t *mask, uint32_t *shift) {
    uint32_t bits = 0;
    while (bits < 31 && ((int64_t)1 << bits) < domain) ++bits;
    *mask = bits >= 32 ? 0xFFFFFFFFu : ((1u << bits) - 1u);
    *shift = bits > 1 ? bits / 2 : 1;
}
// SplitMix64 of (seed, iteration) -> four round keys
void bijection_keys(int64_t seed, int32_t iteration, uint32_t key[4]) {
    uint64_t z = (uint64_t)seed * 0x9E3779B97F4A7C15ULL + (uint64_t)(uint32_t)iteration * 0xD1B54A32D192ED03ULL + 0x632BE59BD9B4E019ULL;
    for (int q = 0; q < 4; ++q) {
        z += 0x9E3779B97F4A7C15ULL;
        uint64_t t = z;
        t = (t ^ (t >> 30)) * 0xBF58476D1CE4E5B9ULL;
        t = (t ^ (t >> 27)) * 0x94D049BB133111EBULL;
        t ^= t >> 31;
        key[q] = (uint32_t)t;
    }
}

void fill_params(const ge_glove *h, GloveParams &p, int32_t iteration) {
    p.focus = h->tab[GE_STATE_FOCUS];     p.context = h->tab[GE_STATE_CONTEXT];
    p.fbias = h->tab[GE_STATE_FBIAS];     p.cbias = h->tab[GE_STATE_CBIAS];
    p.gsf = h->tab[GE_STATE_GSQ_FOCUS];   p.gsc = h->tab[GE_STATE_GSQ_CONTEXT];
    p.gsfb = h->tab[GE_STATE_GSQ_FBIAS];  p.gscb = h->tab[GE_STATE_GSQ_CBIAS];
    p.m2f = h->tab[GE_STATE_M2_FOCUS];    p.m2c = h->tab[GE_STATE_M2_CONTEXT];
    p.m2fb = h->tab[GE_STATE_M2_FBIAS];   p.m2cb = h->tab[GE_STATE_M2_CBIAS];
    p.opt = h->cfg.opt;
    p.hub32 = h->hub32; p.hub_index = h->dhub_index;
    {   // Adam.java:84, evaluated in fp64 from the fp32 constants exactly as the Java expression does
        const float lrf = h->cfg.learning_rate, b1 = 0.9f, b2 = 0.999f;
        p.correction = (double)lrf * std::sqrt(1 - std::pow((double)b2, (double)(iteration + 1))) / (1 - std::pow((double)b1, (double)(iteration + 1)));
    }
    // focus-side tables hold rows [row_begin,row_end): rebase so that kernels index by global row id
    const int64_t off = h->cfg.row_begin;
    if (h->emb16) p.focus = reinterpret_cast<float *>(reinterpret_cast<uint16_t *>(p.focus) - off * h->es);
    else p.focus -= off * h->ds;
    p.gsf -= off * h->ds;
    if (!h->fat) { p.fbias -= off; p.gsfb -= off; }
    if (p.m2f) { p.m2f -= off * h->ds; if (!h->fat) p.m2fb -= off; }
    p.DS = h->ds; p.RW = h->rw; p.ES = h->es;
    p.I = h->dI; p.J = h->dJ; p.X = h->dX; p.perm = h->dperm;
    p.L = h->blocked ? h->lay.L : h->dL; p.W = h->blocked ? h->lay.W : h->dW;
    p.cost_out = h->dcost;
    p.queue = reinterpret_cast<unsigned long long *>(h->dcost + 1);
    p.xmax = h->cfg.xmax; p.N = h->cfg.nnz; p.D = h->cfg.dim;
    p.cost_kind = h->cfg.cost; p.lr = h->cfg.learning_rate;
    p.order_mode = h->cfg.shuffle == GE_SHUFFLE_JAVA ? ORDER_PERM
                 : h->cfg.shuffle == GE_SHUFFLE_DEVICE ? ORDER_BIJECTION : ORDER_IDENTITY;
    p.bA = h->lay.bA; p.bB = h->lay.bB; p.cstart = h->lay.cstart; p.cmeta = h->lay.cmeta; p.n_chunks = h->n_chunks;
    p.n_tchunks = h->n_tchunks; p.n_hchunks = h->n_tchunks + h->n_hchunks; p.tcols = h->lay.tcols; p.tlim = h->lay.tlim;
    p.ticket_end = h->n_chunks;
    p.n_pchunks = h->n_pchunks; p.n_panel_blocks = h->lay.panel_blocks; p.pqueue = p.queue + 1;
    p.prow0 = h->lay.prow0; p.prows = h->lay.prows; p.ppos = h->lay.ppos;
    bijection_width(h->n_pchunks, &p.pbij_mask, &p.pbij_shift);
    p.blocked = h->blocked ? 1 : 0; p.hot_enabled = h->cfg.hot_columns != GE_HOT_NONE; p.flush_every = h->flush_every;
    bijection_width(h->blocked ? h->n_chunks : h->cfg.nnz, &p.bij_mask, &p.bij_shift);      // what the keyed bijection permutes
    bijection_keys(h->cfg.seed, iteration, p.bij_key);
}

// Where the API's table `which` lives on the device and what it looks like there: table[r][c] = base[r * stride + col0 + c], c < ncols.
// Fat handles keep no bias tables: an fp32 row carries its bias at column [dim] (and the accumulator / moment row the bias's
// accumulator / moment there); a bf16 handle's rows cannot, so both scalars sit behind the ACCUMULATOR row:
// [gradSq (dim) | the bias accumulator | the bias | 2 x 0].  bf16: FOCUS / CONTEXT of a bf16 handle, `base` then addresses uint16
// elements and `stride` counts them (the hub columns of CONTEXT also have fp32 master rows in hub32).
const int FAT_HOME[GE_STATE_COUNT] = {GE_STATE_FOCUS, GE_STATE_CONTEXT, GE_STATE_FOCUS, GE_STATE_CONTEXT,
                                      GE_STATE_GSQ_FOCUS, GE_STATE_GSQ_CONTEXT, GE_STATE_GSQ_FOCUS, GE_STATE_GSQ_CONTEXT,
                                      GE_STATE_M2_FOCUS, GE_STATE_M2_CONTEXT, GE_STATE_M2_FOCUS, GE_STATE_M2_CONTEXT};
bool is_bias_table(int which) { return FAT_HOME[which] != which; }
struct TableView {
    float *base; int32_t col0, ncols; int64_t stride; bool bf16;
    bool dense() const { return !bf16 && stride == ncols; }              // the API's view is the stored bytes
    float *first() const { return base ? base + col0 : nullptr; }         // table[0][0] (fp32 views)
};
TableView view_of(const ge_glove *h, int which) {
    const int32_t D = h->cfg.dim;
    if (!is_bias_table(which)) {
        if (h->emb16 && (which == GE_STATE_FOCUS || which == GE_STATE_CONTEXT)) return {h->tab[which], 0, D, h->es, true};
        return {h->tab[which], 0, D, h->ds, false};
    }
    if (!h->fat) return {h->tab[which], 0, 1, 1, false};
    if (h->emb16) {
        const bool focus_side = which == GE_STATE_FBIAS || which == GE_STATE_GSQ_FBIAS;
        const bool the_bias = which == GE_STATE_FBIAS || which == GE_STATE_CBIAS;
        return {h->tab[focus_side ? GE_STATE_GSQ_FOCUS : GE_STATE_GSQ_CONTEXT], the_bias ? D + 1 : D, 1, h->ds, false};
    }
    return {h->tab[FAT_HOME[which]], D, 1, h->ds, false};
}

// Table `which` between its device layout and a dense fp32 device buffer of tab_count[which] floats, as the API shows it (rows
// [n x D] or a bias vector [n]), enqueued on the handle's stream.  fp32: gathered out of / scattered into the strided rows; bf16:
// widened / rounded to nearest even, the hub rows of CONTEXT from / to their fp32 masters.
enum CopyDir { TO_DENSE, FROM_DENSE };
ge_status copy_table(ge_glove *h, int which, float *dense, CopyDir dir) {
    const TableView v = view_of(h, which);
    const int64_t n = h->tab_count[which];
    const int32_t V = h->cfg.vocab_size, D = h->cfg.dim;
    if (v.bf16) {
        const dim3 grid((unsigned)std::min<int64_t>((n + 255) / 256, 8192));
        uint16_t *rows16 = reinterpret_cast<uint16_t *>(v.base);
        const bool hubs = which == GE_STATE_CONTEXT && h->n_hub > 0;
        if (dir == TO_DENSE) {
            hipLaunchKernelGGL(k_bf16_to_f32, grid, dim3(256), 0, h->stream, (const uint16_t *)rows16, dense, n, D, v.stride);
            if (hubs) hipLaunchKernelGGL(k_hub_rows, dim3((unsigned)V), dim3(64), 0, h->stream, dense, h->hub32, h->dhub_index, V, D, 1);
        } else {
            if (hubs) hipLaunchKernelGGL(k_hub_rows, dim3((unsigned)V), dim3(64), 0, h->stream, dense, h->hub32, h->dhub_index, V, D, 0);
            hipLaunchKernelGGL(k_f32_to_bf16, grid, dim3(256), 0, h->stream, (const float *)dense, rows16, n, D, v.stride);
        }
    } else {
        const dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 16384)));
        hipLaunchKernelGGL(dir == TO_DENSE ? k_fat_copy<true> : k_fat_copy<false>, grid, dim3(256), 0, h->stream,
                           v.base, n / v.ncols, (int32_t)v.stride, v.col0, v.ncols, dense);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_failed(dir == FROM_DENSE ? "state copy" : v.bf16 ? "bf16 -> fp32 conversion" : "row gather", e);
    return GE_OK;
}

// get_state / set_state: table `which` to or from the caller's dense host array; returns with the stream drained
ge_status state_io(ge_glove *h, int32_t which, float *host, int64_t count, CopyDir dir) {
    GE_CHECK(check_handle(h));
    if (which < 0 || which >= GE_STATE_COUNT || !host) return ge::fail(GE_ERR_ARG, "invalid state id %d or null buffer", which);
    if (count != h->tab_count[which]) return ge::fail(GE_ERR_ARG, "state %d holds %lld floats, caller passed %lld", which, (long long)h->tab_count[which], (long long)count);
    if (count == 0) return GE_OK;
    const TableView v = view_of(h, which);
    const size_t bytes = sizeof(float) * (size_t)count;
    DeviceBuf stage;                                                  // a dense copy on the device, unless the table is one already
    if (!v.dense()) GE_HIP(hipMalloc(&stage.p, bytes));
    float *dev = v.dense() ? v.base : stage.f32();
    hipError_t e = hipSuccess;
    if (dir == FROM_DENSE) e = hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess && !v.dense()) GE_CHECK(copy_table(h, which, dev, dir));
    if (e == hipSuccess && dir == TO_DENSE) e = hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return hip_failed("state copy", e);
    return GE_OK;
}

// (focus + context) / 2 of every row in a fresh device buffer (the caller frees it), enqueued on the handle's stream.
ge_status extract_to_device(ge_glove *h, bool f64, void **out) {
    GE_CHECK(check_handle(h));
    if (h->rows != h->cfg.vocab_size)
        return ge::fail(GE_ERR_STATE, "extract needs all focus rows on this handle (owned [%d,%d) of %d); gather shards first",
                        h->cfg.row_begin, h->cfg.row_end, h->cfg.vocab_size);
    const int64_t n = (int64_t)h->cfg.vocab_size * h->cfg.dim;
    DeviceBuf d, stage[2];
    GE_HIP(hipMalloc(&d.p, (size_t)n * (f64 ? sizeof(double) : sizeof(float))));
    const int side[2] = {GE_STATE_FOCUS, GE_STATE_CONTEXT};
    const float *src[2] = {h->tab[GE_STATE_FOCUS], h->tab[GE_STATE_CONTEXT]};
    const bool temp = !view_of(h, GE_STATE_FOCUS).dense();          // both sides share one layout
    if (temp)
        for (int s = 0; s < 2; ++s) {
            GE_HIP(hipMalloc(&stage[s].p, sizeof(float) * (size_t)n));
            GE_CHECK(copy_table(h, side[s], stage[s].f32(), TO_DENSE));
            src[s] = stage[s].f32();
        }
    const int blocks = (int)std::min<int64_t>((n + 255) / 256, 8192);
    if (f64) hipLaunchKernelGGL(k_extract<double>, dim3(blocks), dim3(256), 0, h->stream, src[0], src[1], (double *)d.p, n);
    else     hipLaunchKernelGGL(k_extract<float>,  dim3(blocks), dim3(256), 0, h->stream, src[0], src[1], d.f32(), n);
    hipError_t e = hipGetLastError();
    if (temp && e == hipSuccess) e = hipStreamSynchronize(h->stream);      // the temporaries may go once the kernel that reads them has run
    if (e != hipSuccess) return hip_failed("extract", e);
    *out = d.release();
    return GE_OK;
}

ge_status extract_impl(ge_glove *h, void *out, bool f64) {
    if (h && !out) return ge::fail(GE_ERR_ARG, "out is null");
    DeviceBuf d;
    GE_CHECK(extract_to_device(h, f64, &d.p));
    const size_t bytes = (size_t)h->cfg.vocab_size * (size_t)h->cfg.dim * (f64 ? sizeof(double) : sizeof(float));
    hipError_t e = hipMemcpyAsync(out, d.p, bytes, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return hip_failed("extract copy", e);
    return GE_OK;
}

// ---- ge_glove_create, step by step (each step takes the handle; a failed step leaves whatever it allocated to ge_glove_destroy) ----

// GE_GLOVE_TIMING=1: where ge_glove_create's time goes, to stderr (host clock; the stream is drained at each lap)
struct CreateClock {
    bool on;
    hipStream_t stream;
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    void lap(const char *what) {
        if (!on) return;
        (void)hipStreamSynchronize(stream);
        const auto n = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[ge_glove_create] %-34s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(n - t).count());
        t = n;
    }
};

// The configuration and the nonzeros as the caller passed them; [*rb, *re) = the focus rows this handle owns.
ge_status validate_config(const ge_glove_cfg *cfg, const int32_t *I, const int32_t *J, const float *X, int32_t *rb_out, int32_t *re_out) {
    if (!cfg) return ge::fail(GE_ERR_ARG, "cfg is null");
    if (cfg->vocab_size <= 0) return ge::fail(GE_ERR_ARG, "vocab_size must be > 0 (got %d)", cfg->vocab_size);
    if (cfg->dim <= 0) return ge::fail(GE_ERR_ARG, "No dimension specified (dim=%d)", cfg->dim);   // Configuration.check
    if (cfg->nnz < 0 || cfg->nnz > 0x7FFFFFFFLL) return ge::fail(GE_ERR_ARG, "nnz out of range: %lld", (long long)cfg->nnz);
    if ((int64_t)cfg->vocab_size * cfg->dim > 0x7FFFFFFFLL)
        return ge::fail(GE_ERR_ARG, "vocab_size*dim exceeds Java int range (%d x %d)", cfg->vocab_size, cfg->dim);
    if (cfg->nnz > 0 && (!I || !J || !X)) return ge::fail(GE_ERR_ARG, "I/J/X must not be null");
    if (cfg->cost != GE_COST_GLOVE && cfg->cost != GE_COST_PGLOVE) return ge::fail(GE_ERR_ARG, "Invalid cost function %d", cfg->cost);
    if (cfg->opt < GE_OPT_ADAGRAD || cfg->opt > GE_OPT_AMSGRAD) return ge::fail(GE_ERR_ARG, "Invalid optimization method %d", cfg->opt);
    if (cfg->threads < 1) return ge::fail(GE_ERR_ARG, "threads must be >= 1");
    if (cfg->mode != GE_MODE_HOGWILD && cfg->mode != GE_MODE_DETERMINISTIC && cfg->mode != GE_MODE_STRATIFIED) return ge::fail(GE_ERR_ARG, "invalid mode %d", cfg->mode);
    if (cfg->strata < 0 || cfg->strata > 2048) return ge::fail(GE_ERR_ARG, "strata must lie in [0, 2048] (got %d; 0 = the default for the matrix)", cfg->strata);
    if (cfg->strata != 0 && cfg->mode != GE_MODE_STRATIFIED) return ge::fail(GE_ERR_ARG, "strata = %d needs mode = GE_MODE_STRATIFIED", cfg->strata);
    if (cfg->shuffle < GE_SHUFFLE_JAVA || cfg->shuffle > GE_SHUFFLE_NONE) return ge::fail(GE_ERR_ARG, "invalid shuffle %d", cfg->shuffle);
    if (cfg->mode == GE_MODE_STRATIFIED && cfg->shuffle == GE_SHUFFLE_JAVA)
        return ge::fail(GE_ERR_ARG, "the stratified mode cannot follow a global Fisher-Yates order: shuffle must be device or none");
    if (cfg->workers < -(1 << 20)) return ge::fail(GE_ERR_ARG, "workers out of range");
    if (cfg->emb_dtype != GE_DTYPE_F32 && cfg->emb_dtype != GE_DTYPE_BF16) return ge::fail(GE_ERR_ARG, "invalid emb_dtype %d", cfg->emb_dtype);
    const bool emb16 = cfg->emb_dtype == GE_DTYPE_BF16;
    if (emb16 && (cfg->mode != GE_MODE_HOGWILD || cfg->shuffle != GE_SHUFFLE_DEVICE || cfg->opt != GE_OPT_ADAGRAD || cfg->dim % 4 != 0))
        return ge::fail(GE_ERR_ARG, "bf16 embeddings need mode=hogwild, shuffle=device, opt=adagrad and dim %% 4 == 0 (the reference path is fp32)");
    if (cfg->hot_columns < GE_HOT_AUTO || cfg->hot_columns > GE_HOT_ALL) return ge::fail(GE_ERR_ARG, "invalid hot_columns %d", cfg->hot_columns);
    if (cfg->hot_theta < 0 || cfg->stale_budget < 0 || cfg->flush_every < 0 || cfg->blocks_per_cu < 0 || (cfg->layout_flags & ~8191) != 0)
        return ge::fail(GE_ERR_ARG, "invalid tuning fields (hot_theta %g, stale_budget %g, flush_every %d, blocks_per_cu %d, layout_flags %d)",
                        (double)cfg->hot_theta, (double)cfg->stale_budget, cfg->flush_every, cfg->blocks_per_cu, cfg->layout_flags);
    int32_t rb = cfg->row_begin, re = cfg->row_end;
    if (rb == 0 && re == 0) re = cfg->vocab_size;
    if (rb < 0 || re > cfg->vocab_size || rb >= re) return ge::fail(GE_ERR_ARG, "invalid row range [%d,%d)", rb, re);
    const bool will_block = cfg->mode == GE_MODE_HOGWILD && cfg->shuffle == GE_SHUFFLE_DEVICE;   // blocked layout, built (and range-checked) on the device
    if (!will_block)
        for (int64_t k = 0; k < cfg->nnz; ++k) {
            if (I[k] < rb || I[k] >= re) return ge::fail(GE_ERR_ARG, "I[%lld]=%d outside owned rows [%d,%d)", (long long)k, I[k], rb, re);
            if (J[k] < 0 || J[k] >= cfg->vocab_size) return ge::fail(GE_ERR_ARG, "J[%lld]=%d outside [0,%d)", (long long)k, J[k], cfg->vocab_size);
        }
    *rb_out = rb; *re_out = re;
    return GE_OK;
}

// The kernel of a Hogwild handle and the geometry of every handle's rows and records (fat, rw, ds, e16, es): a function of cfg alone.
ge_status plan_geometry(ge_glove *h) {
    const ge_glove_cfg &cfg = h->cfg;
    const int32_t D = cfg.dim;
    h->emb16 = cfg.emb_dtype == GE_DTYPE_BF16;
    if (h->hogwild()) {
        h->hw = pick_hogwild(D, cfg.opt, h->emb16);
        if (!h->hw.fn) return ge::fail(GE_ERR_ARG, "dim %d not supported by the Hogwild kernel (max 1024 for dim%%4==0, 512 for other even dims, 256 for odd dims)", D);
        h->fat = h->hw.fat;
    } else if ((size_t)D * sizeof(float) > 64 * 1024) {
        return ge::fail(GE_ERR_ARG, "dim %d too large for deterministic mode", D);
    }
    const bool interleave = h->interleaved();
    const bool packed = (cfg.layout_flags & GE_LAYOUT_PACKED_RECORDS) != 0;
    h->rw = h->fat ? D + 4 : D;
    // An fp32 fat row as wide as the whole 64-byte lines that hold it (D = 200: 208 floats): every row store then writes whole
    // lines and a row shares no line with its accumulator row.  More bytes, less time: D = 100 (112 instead of 104 floats) 29.8 /
    // 30.4 -> 27.5 / 27.5 ms, D = 200 48.9 / 53.8 -> 47.8 / 47.8 ms (tools/r02/rw_probe.sh).  Not for bf16 rows (no
    // gain measured) and not where the padding would exceed 10 %.
    if (h->fat && !h->emb16 && !packed && D % 4 == 0) {
        const int32_t lines = (D + 1 + 15) / 16 * 16;
        if ((int64_t)lines * 10 <= (int64_t)(D + 4) * 11) h->rw = lines;
    }
    h->ds = h->rw * (interleave ? (h->moments() ? 3 : 2) : 1);
    // bf16 rows in records: [bf16 row, padded to 16 bytes | fp32 accumulator row]; e16 = bf16 elements of the padded row
    h->e16 = (D + 7) / 8 * 8;
    if (h->emb16) h->ds = interleave ? h->e16 / 2 + h->rw : h->rw;                                      // rw: the accumulator row (fat: + its two scalars)
    // A record starts on a 64-byte boundary: a wave's 16-byte-per-lane row access then covers whole 64-byte requests.  Records of
    // 1 632 bytes (D = 200) start on odd 32-byte sectors half of the time; rounding them up to 1 664 took the epoch from 60.9 to
    // 49.2 ms on one box and from 60.8 to 54.6 on another (tools/r02/align_probe.sh, kernel_ab.sh).  Rounding further
    // (128 bytes and more) gains nothing at D = 200 and loses 5 % on the 1 216-byte records of bf16 rows.  The padding is never touched.
    if (interleave && !packed) h->ds = (h->ds + 15) / 16 * 16;
    if (h->emb16) h->es = interleave ? 2 * h->ds : D;
    return GE_OK;
}

// Where the driver places a table decides which of two epoch times the handle gets (same process, same virtual
// address, 48 or 54 ms at the bench size).  So a large table is allocated up to six times, each candidate while the earlier ones
// are still held (else the driver hands the same pages back), a millisecond of what an epoch does to it is timed on each (0.91 -
// 0.97 ms on the good placements, 1.04 - 1.11 ms on the others), the fastest is kept.
struct Placement { float *block = nullptr; int tried = 0; float best_ms = 0.0f, worst_ms = 0.0f; };
ge_status place_record_table(ge_glove *h, size_t rows, Placement *out) {
    const size_t bytes = rows * (size_t)h->ds * sizeof(float);
    // Bounds: the candidates of one table together stay under 24 GB (allocating and freeing an 8 GB table costs a quarter
    // of a second) AND under half of what the device has free right now (another process may share the GPU; a candidate
    // that cannot be allocated ends the search with what there is); a table too large for a second candidate gets one.
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); free_b = 0; }
    const size_t budget = std::min<size_t>((size_t)24 << 30, free_b / 2);
    const int tries = ((h->cfg.layout_flags & GE_LAYOUT_FIRST_PLACEMENT) || bytes < ((size_t)64 << 20)) ? 1
                    : (int)std::max<size_t>(1, std::min<size_t>(6, budget / bytes));
    float *cand[6] = {}; float cand_ms[6] = {};
    int n_cand = 0, best = 0;
    for (int t = 0; t < tries; ++t) {
        if (hipMalloc((void **)&cand[t], bytes) != hipSuccess) { (void)hipGetLastError(); cand[t] = nullptr; break; }     // no room for another candidate: keep what there is
        ++n_cand;
        h->owned.push_back((void *)cand[t]);               // the handle owns every candidate until the losers are freed below
        if (tries == 1) break;
        const int32_t rec_bytes = (int32_t)std::min<int64_t>((int64_t)h->ds * 4, 4096);
        float ms_min = 1e30f;
        for (int rep = 0; rep < 3; ++rep) {
            GE_HIP(hipEventRecord(h->ev0, h->stream));
            hipLaunchKernelGGL(k_probe_records, dim3((unsigned)h->num_cus * 5), dim3(256), 0, h->stream, cand[t], (int64_t)rows, (int64_t)h->ds, rec_bytes, 384, 0x5EEDu + rep);
            GE_HIP(hipEventRecord(h->ev1, h->stream));
            GE_HIP(hipEventSynchronize(h->ev1));
            float ms = 0.0f; GE_HIP(hipEventElapsedTime(&ms, h->ev0, h->ev1));
            ms_min = std::min(ms_min, ms);
        }
        cand_ms[t] = ms_min;
        if (cand_ms[t] < cand_ms[best]) best = t;
        const float slowest = *std::max_element(cand_ms, cand_ms + t + 1);
        if (cand_ms[best] < 0.88f * slowest) break;        // both kinds seen and a fast one in hand (they lie 15 - 20 % apart)
        if (t >= 2 && cand_ms[best] > 0.98f * slowest) break;  // three candidates within 2 %: a box that has one kind only
    }
    if (n_cand == 0) return ge::fail(GE_ERR_OOM, "hipMalloc of a %zu-byte record table failed", bytes);
    for (int t = 0; t < n_cand; ++t) {
        if (t == best) continue;
        h->owned.erase(std::find(h->owned.begin(), h->owned.end(), (void *)cand[t]));
        (void)hipFree(cand[t]);
    }
    *out = {cand[best], n_cand, cand_ms[best], *std::max_element(cand_ms, cand_ms + n_cand)};
    return GE_OK;
}

// Tables, allocated once, in their final layout.  fp32 row tables: `rw` floats per row (fat rows carry the bias at [D]); unless
// GE_LAYOUT_SEPARATE_TABLES a side is ONE allocation of records [row | accumulator row (| second moment row)], stride ds = 2 or
// 3 rw.  bf16 rows: records [bf16 row padded to 16 bytes | fp32 accumulator row, fat: gradSq (D) | its bias accumulator | the
// bias | 2 x 0].
ge_status alloc_tables(ge_glove *h) {
    const int32_t V = h->cfg.vocab_size, D = h->cfg.dim;
    static const int ROWT[2][3] = {{GE_STATE_FOCUS, GE_STATE_GSQ_FOCUS, GE_STATE_M2_FOCUS}, {GE_STATE_CONTEXT, GE_STATE_GSQ_CONTEXT, GE_STATE_M2_CONTEXT}};
    static const int BIAST[2][3] = {{GE_STATE_FBIAS, GE_STATE_GSQ_FBIAS, GE_STATE_M2_FBIAS}, {GE_STATE_CBIAS, GE_STATE_GSQ_CBIAS, GE_STATE_M2_CBIAS}};
    const int n_aux = h->moments() ? 3 : 2;
    for (int side = 0; side < 2; ++side) {
        const size_t nr = side == 0 ? (size_t)h->rows : (size_t)V;
        for (int a = 0; a < n_aux; ++a) { h->tab_count[ROWT[side][a]] = (int64_t)nr * D; h->tab_count[BIAST[side][a]] = (int64_t)nr; }   // what the API shows
        if (h->interleaved()) {
            Placement pl;
            GE_CHECK(place_record_table(h, nr, &pl));
            h->placements += pl.tried; h->place_best_ms += pl.best_ms; h->place_worst_ms += pl.worst_ms;
            if (h->emb16) { h->tab[ROWT[side][0]] = pl.block; h->tab[ROWT[side][1]] = pl.block + h->e16 / 2; }     // the bf16 row leads its record
            else for (int a = 0; a < n_aux; ++a) h->tab[ROWT[side][a]] = pl.block + (size_t)a * h->rw;
        } else {
            for (int a = 0; a < n_aux; ++a) {
                if (a == 0 && h->emb16) { uint16_t *t16 = nullptr; GE_HIP(h->alloc(&t16, nr * (size_t)D)); h->tab[ROWT[side][0]] = reinterpret_cast<float *>(t16); }
                else GE_HIP(h->alloc(&h->tab[ROWT[side][a]], nr * (size_t)h->ds));
            }
        }
        if (!h->fat) for (int a = 0; a < n_aux; ++a) GE_HIP(h->alloc(&h->tab[BIAST[side][a]], nr));
    }
    return GE_OK;
}

// One wavefront = one sequential worker.  Never more workers than N/2048: a small matrix must
// not degenerate into one giant stale batch (the JVM has at most #cores updates in flight).
struct WorkerPlan { int blocks_per_cu, blocks, workers; };
WorkerPlan plan_workers_of(const ge_glove *h, hogwild_fn fn) {
    const ge_glove_cfg &cfg = h->cfg;
    const int64_t N = cfg.nnz;
    const int groups_per_block = 4;
    const int64_t chunks = (N + RUN_CHUNK - 1) / RUN_CHUNK;
    int occ = 0;
    WorkerPlan w{};
    w.blocks_per_cu = cfg.blocks_per_cu > 0 ? cfg.blocks_per_cu : 4;
    if (cfg.blocks_per_cu == 0 && hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, reinterpret_cast<const void *>(fn), 256, 0) == hipSuccess && occ > 0)
        w.blocks_per_cu = occ;                       // every worker resident: one wave of blocks
    int64_t blocks = std::min<int64_t>((chunks + 3) / 4, (int64_t)h->num_cus * w.blocks_per_cu);
    blocks = std::min<int64_t>(blocks, std::max<int64_t>(1, N / 2048 / groups_per_block));
    w.blocks = (int)std::max<int64_t>(blocks, 1);
    w.workers = w.blocks * 4;
    if (cfg.workers > 0) {                        // explicit worker count (tests, reproducibility)
        w.workers = (int)std::min<int64_t>(cfg.workers, (int64_t)h->num_cus * 32);
        w.blocks = (w.workers + 3) / 4;
    } else if (cfg.workers < 0) {                 // fill the device but leave -workers wavefront slots to kernels
        w.blocks = (int)std::max<int64_t>(1, (int64_t)w.blocks - (-(int64_t)cfg.workers + 3) / 4);   // running beside (collectives)
        w.workers = w.blocks * 4;
    }
    return w;
}
void take_plan(ge_glove *h, const WorkerPlan &w) { h->hw_blocks_per_cu = w.blocks_per_cu; h->hw_blocks = w.blocks; h->hw_workers = w.workers; }
void plan_workers(ge_glove *h) { take_plan(h, plan_workers_of(h, h->hw.fn)); }

// Hub tiles: the kernel with the tile walk exists for one lane shape; a handle of that shape that owns every focus
// row gets tiles when GE_LAYOUT_HUB_TILES asks for them, or by default from 2^25 nonzeros on (the saving is reasoned and measured at
// the bench size only; smaller handles keep their chunk table and their kernel).  GE_LAYOUT_NO_HUB_TILES: never.
// (GE_LAYOUT_HUB_PANELS on a handle too small for tiles of its own asks for the tiles its panels are made of, as GE_LAYOUT_HUB_TILES
// does -- unless GE_LAYOUT_NO_HUB_PANELS takes it back; from 2^25 nonzeros on the panels are made of the tiles the handle builds anyway)
// (GE_LAYOUT_DEEP_PANELS asks for panels as GE_LAYOUT_HUB_PANELS does; GE_LAYOUT_NO_DEEP_PANELS takes back the kernel, not the panels)
// (GE_LAYOUT_DEEP_WALK asks for everything GE_LAYOUT_DEEP_PANELS asks for, and for the depth-2 walk on top)
bool deep_asked(const ge_glove_cfg &cfg) { return (cfg.layout_flags & (GE_LAYOUT_DEEP_PANELS | GE_LAYOUT_DEEP_WALK)) != 0; }
bool tiles_forced(const ge_glove_cfg &cfg) {
    const bool panels_asked = ((cfg.layout_flags & GE_LAYOUT_HUB_PANELS) != 0 || deep_asked(cfg)) && (cfg.layout_flags & GE_LAYOUT_NO_HUB_PANELS) == 0;
    return (cfg.layout_flags & GE_LAYOUT_HUB_TILES) != 0 || (panels_asked && cfg.nnz < ((int64_t)1 << 25));
}
bool tiles_possible(const ge_glove *h) {
    const ge_glove_cfg &cfg = h->cfg;
    if (cfg.layout_flags & GE_LAYOUT_NO_HUB_TILES) return false;
    if (h->emb16 || cfg.opt != GE_OPT_ADAGRAD || !h->hw.fat || h->hw.vw != 4 || h->hw.nch != 1) return false;
    if (cfg.shuffle != GE_SHUFFLE_DEVICE || h->rows != cfg.vocab_size) return false;
    return tiles_forced(cfg) || cfg.nnz >= ((int64_t)1 << 25);
}
// Hub panels: full groups of tile columns walked four to a workgroup.  A handle that builds tiles builds panels
// from the same 2^25 nonzeros on (measured at the bench size only), or at any size when GE_LAYOUT_HUB_PANELS asks;
// GE_LAYOUT_NO_HUB_PANELS: never -- the handle is then the one it was before there were panels.
bool panels_possible(const ge_glove *h) {
    const ge_glove_cfg &cfg = h->cfg;
    if ((cfg.layout_flags & GE_LAYOUT_NO_HUB_PANELS) || !tiles_possible(h)) return false;
    return (cfg.layout_flags & GE_LAYOUT_HUB_PANELS) != 0 || deep_asked(cfg) || cfg.nnz >= ((int64_t)1 << 25);
}
// The ring kernel walks the panels of a handle that builds them by default, or under GE_LAYOUT_DEEP_PANELS; a
// handle whose panels GE_LAYOUT_HUB_PANELS alone asked for keeps k_epoch_panels, and GE_LAYOUT_NO_DEEP_PANELS wins over everything.
bool ring_possible(const ge_glove *h) {
    const ge_glove_cfg &cfg = h->cfg;
    if ((cfg.layout_flags & GE_LAYOUT_NO_DEEP_PANELS) || !panels_possible(h)) return false;
    return deep_asked(cfg) || (cfg.layout_flags & GE_LAYOUT_HUB_PANELS) == 0;
}
// The depth-2 walk is the ring kernel's, under GE_LAYOUT_DEEP_WALK only: measured at the bench size it gains 0.8 %
// on one kind of placement, nothing on the other, and ends at a higher cost on both, so no handle runs it by default.  GE_LAYOUT_NO_DEEP_WALK wins.
bool walk2_possible(const ge_glove *h) {
    const ge_glove_cfg &cfg = h->cfg;
    if ((cfg.layout_flags & GE_LAYOUT_NO_DEEP_WALK) || !ring_possible(h)) return false;
    return (cfg.layout_flags & GE_LAYOUT_DEEP_WALK) != 0;
}
// Hub columns of density >= 1 / PANEL_DENSITY_DIV join the panels of a handle that runs the ring kernel through the default
// rule (glove_layout.hip; chosen by the sweep of profiles/hub_ring_bench.json).
constexpr int PANEL_DENSITY_DIV = 16;

// The order a Hogwild epoch visits the nonzeros in.  Device shuffle: the blocked layout of ge_layout.h, built on the device.
// General order (Java permutation / matrix order): the resident side is always the context row, hub columns are keyed ~j.
// device_input: I, J, X are the device arrays of a ge_coo (blocked layout only; ge_glove_create_coo sees to that).
ge_status plan_epoch_layout(ge_glove *h, const int32_t *I, const int32_t *J, const float *X, bool device_input) {
    const ge_glove_cfg &cfg = h->cfg;
    const int32_t V = cfg.vocab_size;
    const int64_t N = cfg.nnz;
    // (0.05 -- five times the hub columns -- takes a fifth off the Hogwild lag, C2 epoch 32: 1.068 -> 1.055 of the sequential oracle's
    // cost, and is free on the faster kind of placement (48.0 -> 48.3 ms) but costs 4 - 7 % on the slower kind (54.9 -> 57 - 58.7 ms,
    // tools/r03/theta_modes.py): the default stays 0.25)
    const double theta = cfg.hot_theta > 0 ? (double)cfg.hot_theta : 0.25;
    const double stale_budget = cfg.stale_budget > 0 ? (double)cfg.stale_budget : 2000.0;
    h->blocked = cfg.shuffle == GE_SHUFFLE_DEVICE;
    if (h->blocked) {
        ge::LayoutRequest rq{};
        rq.V = V; rq.row_begin = cfg.row_begin; rq.row_end = cfg.row_end; rq.N = N; rq.cost = cfg.cost; rq.xmax = cfg.xmax;
        rq.hot_columns = cfg.hot_columns; rq.hot_theta = theta; rq.stale_budget = stale_budget; rq.flush_every = cfg.flush_every;
        rq.workers = h->hw_workers;
        rq.shared_rows = (cfg.layout_flags & GE_LAYOUT_PLAIN_LONG_ROWS) ? 0 : 1;
        rq.pack_rows = (cfg.layout_flags & GE_LAYOUT_FIXED_CUTS) ? 0 : 1;
        rq.want_hub_index = h->emb16;
        rq.device_input = device_input;
        // which columns go into tiles is decided from the counts alone; the workers then come from the kernel that will run,
        // and the flush limits from the workers (the hub threshold stays that of the ordinary kernel's workers: glove_layout.hip)
        const hogwild_fn tile_fn = k_epoch_tiles<TILE_G>;
        WorkerPlan tile_plan{};
        bool ring = false;
        if (tiles_possible(h)) {
            tile_plan = plan_workers_of(h, tile_fn);
            rq.tile_g = TILE_G; rq.tile_force = tiles_forced(cfg) ? 1 : 0; rq.tile_workers = tile_plan.workers;
            if (panels_possible(h)) {
                rq.panels = 1; rq.blocks = tile_plan.blocks;
                if (const char *e = std::getenv("GE_PANEL_BLOCKS")) rq.panel_blocks = std::max(0, std::atoi(e));     // experiments: the sweep of profiles/hub_panels_bench.json
                if (ring_possible(h)) {
                    ring = true;
                    if (!rq.tile_force) {
                        rq.panel_div = PANEL_DENSITY_DIV;
                        if (const char *e = std::getenv("GE_PANEL_DENSITY_DIV")) rq.panel_div = std::max(8, std::atoi(e));   // experiments: the sweep of profiles/hub_ring_bench.json
                    }
                }
            }
        }
        GE_CHECK(ge::build_blocked_layout(rq, I, J, X, h->stream, &h->lay));
        if (h->lay.n_tchunks > 0 || h->lay.n_pchunks > 0) { h->hw.fn = h->lay.n_pchunks > 0 ? (ring ? (walk2_possible(h) ? (hogwild_fn)k_epoch_walk2 : (hogwild_fn)k_epoch_ring) : (hogwild_fn)k_epoch_panels) : tile_fn; take_plan(h, tile_plan); }
        h->n_chunks = h->lay.n_chunks; h->n_hchunks = h->lay.n_hchunks; h->n_tchunks = h->lay.n_tchunks; h->n_pchunks = h->lay.n_pchunks;
        h->hot_cols = h->lay.hot_cols; h->hot_nnz = h->lay.hot_nnz; h->hot_threshold = h->lay.hot_threshold;
        h->flush_every = h->lay.flush_min;
        if (h->emb16) { h->host_hub_index.swap(h->lay.hub_index); h->n_hub = h->lay.n_hub; }
        return GE_OK;
    }
    std::vector<int32_t> cnt((size_t)V, 0);
    std::vector<uint8_t> hotcol((size_t)V, 0);
    if (N > 0 && cfg.hot_columns != GE_HOT_NONE) {
        const int64_t thr = cfg.hot_columns == GE_HOT_ALL ? 0
                          : std::max<int64_t>(2, (int64_t)std::ceil(theta * (double)N / (double)h->hw_workers));
        for (int64_t k = 0; k < N; ++k) ++cnt[(size_t)J[k]];
        for (int32_t v = 0; v < V; ++v)
            if (cnt[(size_t)v] >= thr && cnt[(size_t)v] > 0) { hotcol[(size_t)v] = 1; ++h->hot_cols; h->hot_nnz += cnt[(size_t)v]; }
        h->hot_threshold = thr;
    }
    h->flush_every = cfg.flush_every > 0 ? std::min<int32_t>(cfg.flush_every, RUN_CHUNK) : RUN_CHUNK;
    if (cfg.flush_every == 0)
        for (int32_t v = 0; v < V; ++v) if (hotcol[(size_t)v]) {
            const double K = std::max(1.0, (double)cnt[(size_t)v] * (double)h->hw_workers / (double)std::max<int64_t>(N, 1));
            h->flush_every = std::min<int>(h->flush_every, (int)std::min<double>(RUN_CHUNK, std::max<double>(4.0, std::floor(stale_budget / K))));
        }
    h->host_key.assign(J, J + N);
    for (int64_t k = 0; k < N; ++k) if (hotcol[(size_t)J[k]]) h->host_key[(size_t)k] = ~J[k];
    h->n_chunks = (N + RUN_CHUNK - 1) / RUN_CHUNK; h->n_hchunks = 0;
    return GE_OK;
}

// General order: the nonzeros as the caller passed them (J replaced by the hub keys), and the Hogwild kernel's cost terms.
// (The blocked layout holds its own re-ordered copies.)
ge_status upload_nonzeros(ge_glove *h, const int32_t *I, const int32_t *J, const float *X) {
    const int64_t N = h->cfg.nnz;
    const size_t nn = (size_t)std::max<int64_t>(N, 1);
    GE_HIP(h->alloc(&h->dI, nn)); GE_HIP(h->alloc(&h->dJ, nn)); GE_HIP(h->alloc(&h->dX, nn));
    if (N == 0) return GE_OK;
    GE_HIP(hipMemcpyAsync(h->dI, I, sizeof(int32_t) * (size_t)N, hipMemcpyHostToDevice, h->stream));
    GE_HIP(hipMemcpyAsync(h->dJ, h->host_key.empty() ? J : h->host_key.data(), sizeof(int32_t) * (size_t)N, hipMemcpyHostToDevice, h->stream));
    GE_HIP(hipMemcpyAsync(h->dX, X, sizeof(float) * (size_t)N, hipMemcpyHostToDevice, h->stream));
    if (h->hogwild()) {
        GE_HIP(h->alloc(&h->dL, nn)); GE_HIP(h->alloc(&h->dW, nn));
        const int blocks = (int)std::min<int64_t>((N + 255) / 256, 8192);
        hipLaunchKernelGGL(k_cost_terms, dim3(blocks), dim3(256), 0, h->stream, h->dX, N, h->cfg.cost, h->cfg.xmax, h->dL, h->dW);
    }
    GE_HIP(hipStreamSynchronize(h->stream));
    return GE_OK;
}

ge_status init_permutation(ge_glove *h) {
    const int64_t N = h->cfg.nnz;
    GE_HIP(h->alloc(&h->dperm, (size_t)std::max<int64_t>(N, 1)));
    h->perm.resize((size_t)N);
    for (int64_t k = 0; k < N; ++k) h->perm[(size_t)k] = (int32_t)k;     // Permutation ctor
    return GE_OK;
}

// Accumulators, then the parameters in the reference's draw order, straight into the final layout; the context side covers all V
// rows, the focus side only the owned rows (same values a single-GPU run would hold there).
ge_status init_state(ge_glove *h) {
    const int32_t V = h->cfg.vocab_size, D = h->cfg.dim, rb = h->cfg.row_begin;
    const uint64_t s0 = ge::JavaRandom::scramble(h->cfg.seed);
    if (h->emb16) {
        GE_HIP(h->alloc(&h->dhub_index, (size_t)V));
        GE_HIP(hipMemcpyAsync(h->dhub_index, h->host_hub_index.data(), sizeof(int32_t) * (size_t)V, hipMemcpyHostToDevice, h->stream));
        GE_HIP(h->alloc(&h->hub32, (size_t)std::max<int64_t>((int64_t)h->n_hub * D, 1)));
    }
    // Adagrad ctor: gradSq = 1 (Adagrad.java:27-33); Adam / AMSGrad ctors: every moment = 0 (new float[]).  Before the parameter
    // init: a bf16 handle's bias lives in the accumulator row and must survive the fill.
    const float v0 = h->moments() ? 0.0f : 1.0f;
    for (int t : {GE_STATE_GSQ_FOCUS, GE_STATE_GSQ_CONTEXT, GE_STATE_M2_FOCUS, GE_STATE_M2_CONTEXT}) {
        if (!h->tab[t]) continue;
        const int64_t nr = h->tab_count[t] / D;
        const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>((nr * h->rw + 255) / 256, 8192));
        hipLaunchKernelGGL(k_fill_rows, dim3(blocks), dim3(256), 0, h->stream, h->tab[t], nr, (int64_t)h->ds, h->fat ? D + 1 : D, h->rw, v0);
    }
    for (int t : {GE_STATE_GSQ_FBIAS, GE_STATE_GSQ_CBIAS, GE_STATE_M2_FBIAS, GE_STATE_M2_CBIAS}) {
        if (!h->tab[t]) continue;
        const int64_t n = h->tab_count[t];
        hipLaunchKernelGGL(k_fill, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 4096))), dim3(256), 0, h->stream, h->tab[t], n, v0);
    }
    const TableView foc = view_of(h, GE_STATE_FOCUS), ctx = view_of(h, GE_STATE_CONTEXT);
    const TableView fb = view_of(h, GE_STATE_FBIAS), cb = view_of(h, GE_STATE_CBIAS);
    const int32_t bias_col = (h->fat && !h->emb16) ? D : -1;        // fp32 fat rows: the bias is a column of the row being written
    auto launch = [&](void *f, void *c, int32_t row0, int32_t nrows) {          // hub_index / hub32: null unless bf16
        hipLaunchKernelGGL(h->emb16 ? k_init_java<true> : k_init_java<false>, dim3((unsigned)((nrows + 127) / 128)), dim3(128), 0, h->stream,
                           f, c, fb.first(), cb.first(), fb.stride, rb, row0, nrows, D, foc.stride, bias_col, h->rw, s0,
                           (const int32_t *)h->dhub_index, h->hub32);
    };
    if (h->rows == V) launch(foc.base, ctx.base, 0, V);
    else { launch(nullptr, ctx.base, 0, V); launch(foc.base, nullptr, rb, h->rows); }
    GE_HIP(hipGetLastError());
    GE_HIP(hipStreamSynchronize(h->stream));
    h->rng.s = ge::JavaRandom::jump(s0, (uint64_t)V * (uint64_t)(2 + 2 * D));
    return GE_OK;
}

ge_status ge_glove_create_impl(const ge_glove_cfg *cfg, const int32_t *I, const int32_t *J, const float *X, bool device_input, ge_glove **out) {
    if (!out) return ge::fail(GE_ERR_ARG, "out is null");
    *out = nullptr;
    int32_t rb = 0, re = 0;
    GE_CHECK(validate_config(cfg, I, J, X, &rb, &re));
    GE_CHECK(ge::select_device(cfg->device));

    std::unique_ptr<ge_glove, decltype(&ge_glove_destroy)> h(new (std::nothrow) ge_glove(), ge_glove_destroy);   // a failure below frees what the handle owns so far
    if (!h) return ge::fail(GE_ERR_OOM, "host allocation failed");
    h->cfg = *cfg;
    h->cfg.row_begin = rb; h->cfg.row_end = re;
    h->rows = re - rb;
    h->stream = (hipStream_t)cfg->stream;
    GE_CHECK(plan_geometry(h.get()));

    CreateClock clk{std::getenv("GE_GLOVE_TIMING") != nullptr, h->stream};
    hipDeviceProp_t prop;
    GE_HIP(hipGetDeviceProperties(&prop, cfg->device));
    h->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    GE_HIP(hipEventCreate(&h->ev0));
    GE_HIP(hipEventCreate(&h->ev1));

    GE_CHECK(alloc_tables(h.get()));
    clk.lap("tables (placement search)");
    GE_HIP(h->alloc(&h->dcost, 3));
    GE_HIP(h->alloc(&h->djob, (size_t)cfg->threads));
    if (h->hogwild()) {
        plan_workers(h.get());
        GE_CHECK(plan_epoch_layout(h.get(), I, J, X, device_input));
    }
    clk.lap("epoch layout");
    if (h->stratified()) {            // its own copies of the nonzeros, sorted by tile
        const int32_t P = cfg->strata > 0 ? cfg->strata : ge::strata_default_p(h->rows, cfg->nnz);
        GE_CHECK(ge::strata_build(&h->strata, P, cfg->vocab_size, cfg->nnz, I, J, X, h->stream));
    } else if (!h->blocked) GE_CHECK(upload_nonzeros(h.get(), I, J, X));
    if (cfg->shuffle == GE_SHUFFLE_JAVA) GE_CHECK(init_permutation(h.get()));
    GE_CHECK(init_state(h.get()));
    clk.lap("init and the rest");
    *out = h.release();
    return GE_OK;
}

// The trainer on a ge_coo.  The production handle (Hogwild, device shuffle) on a device-resident matrix builds its layout from the
// device arrays where they are; everything else goes through the host arrays and is ge_glove_create on them.
ge_status ge_glove_create_coo_impl(const ge_glove_cfg *cfg, const ge_coo *coo, ge_glove **out) {
    if (!out) return ge::fail(GE_ERR_ARG, "out is null");
    *out = nullptr;
    if (!cfg) return ge::fail(GE_ERR_ARG, "cfg is null");
    if (!coo) return ge::fail(GE_ERR_ARG, "null ge_coo handle");
    ge_glove_cfg c = *cfg;
    if (c.vocab_size != coo->V) return ge::fail(GE_ERR_ARG, "vocab_size %d does not match the matrix (%d)", c.vocab_size, coo->V);
    if (c.nnz != 0 && c.nnz != coo->nnz) return ge::fail(GE_ERR_ARG, "nnz %lld does not match the matrix (%lld); 0 takes it from there", (long long)c.nnz, (long long)coo->nnz);
    if (c.xmax != 0 && c.xmax != coo->max) return ge::fail(GE_ERR_ARG, "xmax %.17g does not match the matrix (%.17g); 0 takes it from there", c.xmax, coo->max);
    c.nnz = coo->nnz; c.xmax = coo->max;
    if (coo->device >= 0) {
        if (coo->device != c.device) return ge::fail(GE_ERR_ARG, "the matrix lives on device %d, the handle is asked for on device %d", coo->device, c.device);
        int32_t rb = c.row_begin, re = c.row_end;
        if (rb == 0 && re == 0) re = c.vocab_size;
        if (coo->row_begin < rb || coo->row_end > re)
            return ge::fail(GE_ERR_ARG, "the matrix holds rows [%d,%d), outside owned rows [%d,%d)", coo->row_begin, coo->row_end, rb, re);
        if (c.mode == GE_MODE_HOGWILD && c.shuffle == GE_SHUFFLE_DEVICE)
            return ge_glove_create_impl(&c, coo->dI, coo->dJ, coo->dX, true, out);
    }
    const int32_t *I = nullptr, *J = nullptr; const float *X = nullptr;
    GE_CHECK(ge_coo_get(coo, nullptr, &I, &J, &X, nullptr, nullptr));
    return ge_glove_create_impl(&c, I, J, X, false, out);
}

// start of a Hogwild epoch on the handle's stream: cost accumulator and ticket counter zeroed, ev0 behind them
ge_status begin_hogwild_epoch(ge_glove *h) {
    GE_HIP(hipMemsetAsync(h->dcost, 0, 3 * sizeof(double), h->stream));
    GE_HIP(hipEventRecord(h->ev0, h->stream));
    h->last_launches = 0;
    return GE_OK;
}
void launch_hogwild(ge_glove *h, const GloveParams &p, int blocks) {
    hipLaunchKernelGGL(h->hw.fn, dim3((unsigned)blocks), dim3(256), 0, h->stream, p, (int32_t)h->hw_workers);
    ++h->last_launches;
}

ge_status ge_glove_epoch_impl(ge_glove *h, int32_t iteration, double *cost_sum) {
    GE_CHECK(check_handle(h));
    const int64_t N = h->cfg.nnz;
    if (h->cfg.shuffle == GE_SHUFFLE_JAVA && N > 0) {
        // ExtendedRandom.shuffle(int[]), cumulative on the same array (J/util/rnd/ExtendedRandom.java:398-407)
        int32_t *a = h->perm.data();
        const int32_t n = (int32_t)N;
        for (int32_t i = 0; i < n; ++i) {
            const int32_t r = i + h->rng.next_int(n - i);
            const int32_t t = a[i]; a[i] = a[r]; a[r] = t;
        }
        GE_HIP(hipMemcpyAsync(h->dperm, a, sizeof(int32_t) * (size_t)N, hipMemcpyHostToDevice, h->stream));
    }
    GloveParams p;
    fill_params(h, p, iteration);
    if (h->stratified()) {
        ge::ExactParams e{p.focus, p.context, p.fbias, p.cbias, p.gsf, p.gsc, p.gsfb, p.gscb, p.m2f, p.m2c, p.m2fb, p.m2cb,
                          p.correction, p.xmax, p.opt, p.D, p.cost_kind, p.lr};
        double total = 0.0;
        GE_CHECK(ge::strata_epoch(&h->strata, e, h->cfg.seed, iteration, h->cfg.shuffle == GE_SHUFFLE_DEVICE, h->stream, h->ev0, h->ev1,
                                  &h->last_launches, &total));
        GE_HIP(hipEventElapsedTime(&h->last_ms, h->ev0, h->ev1));
        if (cost_sum) *cost_sum = total;
        return GE_OK;
    }
    const int T = h->cfg.mode == GE_MODE_DETERMINISTIC ? h->cfg.threads : 0;
    if (T > 0) {
        const int64_t per = N / T;
        h->last_launches = 0;
        GE_HIP(hipMemsetAsync(h->djob, 0, sizeof(float) * (size_t)T, h->stream));
        GE_HIP(hipEventRecord(h->ev0, h->stream));
        for (int t = 0; t < T; ++t) {
            const int64_t off = per * t;                                  // Adagrad.java:47
            const int64_t lines = (t == T - 1) ? per + N % T : per;       // Optimizer.java:59-63
            if (lines <= 0) continue;
            hipLaunchKernelGGL(k_adagrad_exact, dim3(1), dim3(64), sizeof(float) * (size_t)h->cfg.dim, h->stream,
                               p, off, off + lines, h->djob + t);
            ++h->last_launches;
        }
    } else {
        GE_CHECK(begin_hogwild_epoch(h));
        if (N > 0) launch_hogwild(h, p, h->hw_blocks);
    }
    GE_HIP(hipEventRecord(h->ev1, h->stream));
    GE_HIP(hipGetLastError());
    double total = 0.0;
    std::vector<float> jc((size_t)T);                                     // deterministic: one fp32 cost per job
    if (T > 0) GE_HIP(hipMemcpyAsync(jc.data(), h->djob, sizeof(float) * (size_t)T, hipMemcpyDeviceToHost, h->stream));
    else GE_HIP(hipMemcpyAsync(&total, h->dcost, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    GE_HIP(hipStreamSynchronize(h->stream));
    for (float c : jc) total += (double)c;                                // localCost += job result (Optimizer.java:89)
    GE_HIP(hipEventElapsedTime(&h->last_ms, h->ev0, h->ev1));
    if (cost_sum) *cost_sum = total;
    return GE_OK;
}

ge_status ge_glove_epoch_order_impl(ge_glove *h, int32_t iteration, int32_t *out, int64_t count) {
    if (!h || !out) return ge::fail(GE_ERR_ARG, "null argument");
    if (h->cfg.mode == GE_MODE_DETERMINISTIC) return ge::fail(GE_ERR_STATE, "epoch order is defined for GE_MODE_HOGWILD and GE_MODE_STRATIFIED handles");
    const int64_t N = h->cfg.nnz;
    if (count != N) return ge::fail(GE_ERR_ARG, "the epoch visits %lld nonzeros", (long long)N);
    if (h->stratified()) {
        ge::strata_order(&h->strata, h->cfg.seed, iteration, h->cfg.shuffle == GE_SHUFFLE_DEVICE, out);
        return GE_OK;
    }
    GloveParams p;
    fill_params(h, p, iteration);
    std::vector<int32_t> key, border, cstart;        // blocked layout: copied back from the device (a testing aid, not a hot path)
    if (h->blocked) {
        GE_CHECK(check_handle(h));
        key.resize((size_t)std::max<int64_t>(N, 1)); border.resize(key.size()); cstart.resize((size_t)h->n_chunks + 1);
        if (N > 0) {
            GE_HIP(hipMemcpy(key.data(), h->lay.bA, sizeof(int32_t) * (size_t)N, hipMemcpyDeviceToHost));
            GE_HIP(hipMemcpy(border.data(), h->lay.border, sizeof(int32_t) * (size_t)N, hipMemcpyDeviceToHost));
        }
        GE_HIP(hipMemcpy(cstart.data(), h->lay.cstart, sizeof(int32_t) * cstart.size(), hipMemcpyDeviceToHost));
    }
    std::vector<std::pair<int32_t, int32_t>> ent;      // (key, original nonzero) of one chunk, in staging order
    int64_t w = 0;
    // Panel tickets first (what a handle of one block executes): a panel chunk's rows ascending, per row its four groups in turn,
    // inside a group the slot order the positions already have.
    for (int64_t t = 0; t < h->n_pchunks; ++t) {
        uint32_t x = (uint32_t)t;
        do { x = ge::bij_mix(x, p.pbij_mask, p.pbij_shift, p.bij_key); } while ((int64_t)x >= h->n_pchunks);
        const int32_t *pp = h->lay.host_ppos.data() + (size_t)x * 9;
        int32_t at[4], end[4];
        for (int g = 0; g < 4; ++g) { at[g] = pp[1 + 2 * g]; end[g] = at[g] + pp[2 + 2 * g]; }
        for (;;) {
            int32_t row = INT32_MAX;
            for (int g = 0; g < 4; ++g) if (at[g] < end[g]) row = std::min(row, key[(size_t)at[g]]);
            if (row == INT32_MAX) break;
            for (int g = 0; g < 4; ++g) while (at[g] < end[g] && key[(size_t)at[g]] == row) out[w++] = border[(size_t)at[g]++];
        }
    }
    for (int64_t t = 0; t < h->n_chunks; ++t) {
        ent.clear();
        if (h->blocked) {
            uint32_t x = (uint32_t)t;
            do { x = bij_round(x, p); } while ((int64_t)x >= h->n_chunks);
            for (int64_t k = cstart[(size_t)x]; k < cstart[(size_t)x + 1]; ++k) ent.push_back({key[(size_t)k], border[(size_t)k]});
        } else {
            for (int64_t k = t * RUN_CHUNK; k < std::min<int64_t>((t + 1) * RUN_CHUNK, N); ++k) {
                const int64_t idx = h->cfg.shuffle == GE_SHUFFLE_JAVA ? h->perm[(size_t)k] : k;
                ent.push_back({h->host_key[(size_t)idx], (int32_t)idx});
            }
        }
        std::stable_sort(ent.begin(), ent.end(), [](const std::pair<int32_t, int32_t> &a, const std::pair<int32_t, int32_t> &b) { return a.first < b.first; });
        for (auto &e : ent) out[w++] = e.second;
    }
    if (w != N) return ge::fail(GE_ERR_STATE, "internal: epoch order covers %lld of %lld nonzeros", (long long)w, (long long)N);
    return GE_OK;
}

}  // namespace

extern "C" {

void ge_glove_cfg_default(ge_glove_cfg *cfg) {
    if (!cfg) return;
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->cost = GE_COST_GLOVE;
    cfg->opt = GE_OPT_ADAGRAD;
    cfg->learning_rate = 0.05f;
    cfg->threads = 1;
    cfg->mode = GE_MODE_HOGWILD;
    cfg->shuffle = GE_SHUFFLE_DEVICE;
}

ge_status ge_glove_extract_f32(ge_glove *h, float *out) { return extract_impl(h, out, false); }
ge_status ge_glove_extract_f64(ge_glove *h, double *out) { return extract_impl(h, out, true); }
ge_status ge_glove_get_state(ge_glove *h, int32_t which, float *out, int64_t count) { return state_io(h, which, out, count, TO_DENSE); }
ge_status ge_glove_set_state(ge_glove *h, int32_t which, const float *in, int64_t count) { return state_io(h, which, const_cast<float *>(in), count, FROM_DENSE); }

ge_status ge_glove_device_ptr(ge_glove *h, int32_t which, void **dptr, int64_t *count) {
    if (!h) return ge::fail(GE_ERR_ARG, "null ge_glove handle");
    if (which < 0 || which >= GE_STATE_COUNT || !dptr) return ge::fail(GE_ERR_ARG, "invalid state id %d or null out", which);
    const TableView v = view_of(h, which);
    if (v.bf16) return ge::fail(GE_ERR_STATE, "table %d is stored as bf16 (+ fp32 hub rows); use ge_glove_get_state/set_state", which);
    // a row table is [n x row_stride]; a bias "table" may be one column of its home table (view_of): the pointer is row 0's scalar,
    // consecutive rows are row_stride floats apart.  *count = floats from the returned pointer to the end of the last row's part.
    *dptr = v.first();
    const int64_t nr = h->tab_count[which] / v.ncols;
    if (count) *count = nr > 0 ? (nr - 1) * v.stride + (is_bias_table(which) ? 1 : h->rw) : 0;
    return GE_OK;
}

ge_status ge_glove_context_layout(ge_glove *h, ge_context_layout *out) {
    if (!h || !out) return ge::fail(GE_ERR_ARG, "null argument");
    const TableView ctx = view_of(h, GE_STATE_CONTEXT), acc = view_of(h, GE_STATE_GSQ_CONTEXT);
    const TableView cb = view_of(h, GE_STATE_CBIAS), gcb = view_of(h, GE_STATE_GSQ_CBIAS);
    out->table = ctx.base;
    out->dtype = ctx.bf16 ? GE_DTYPE_BF16 : GE_DTYPE_F32;
    out->hub_rows = ctx.bf16 ? h->hub32 : nullptr;
    out->hub_index = ctx.bf16 ? h->dhub_index : nullptr;
    out->n_hub = ctx.bf16 ? h->n_hub : 0;
    out->vocab_size = h->cfg.vocab_size; out->dim = h->cfg.dim;
    out->row_stride = (int32_t)ctx.stride;
    out->accum = acc.base;
    out->accum_stride = (int32_t)acc.stride;
    out->bias = cb.first(); out->bias_stride = (int32_t)cb.stride;
    out->accum_bias = gcb.first(); out->accum_bias_stride = (int32_t)gcb.stride;
    return GE_OK;
}

ge_status ge_glove_get_perm(ge_glove *h, int32_t *out, int64_t count) {
    if (!h || !out) return ge::fail(GE_ERR_ARG, "null argument");
    if (h->cfg.shuffle != GE_SHUFFLE_JAVA) return ge::fail(GE_ERR_STATE, "no permutation array unless shuffle == GE_SHUFFLE_JAVA");
    if (count != h->cfg.nnz) return ge::fail(GE_ERR_ARG, "perm holds %lld entries", (long long)h->cfg.nnz);
    std::memcpy(out, h->perm.data(), sizeof(int32_t) * (size_t)count);
    return GE_OK;
}

ge_status ge_glove_rng_state(ge_glove *h, uint64_t *state) {
    if (!h || !state) return ge::fail(GE_ERR_ARG, "null argument");
    *state = h->rng.s;
    return GE_OK;
}

ge_status ge_glove_last_kernel_ms(ge_glove *h, float *ms, int32_t *launches) {
    if (!h) return ge::fail(GE_ERR_ARG, "null ge_glove handle");
    if (ms) *ms = h->last_ms;
    if (launches) *launches = h->last_launches;
    return GE_OK;
}

ge_status ge_glove_set_arith(ge_glove *h, int32_t arith) {
    if (!h) return ge::fail(GE_ERR_ARG, "null ge_glove handle");
    if (arith != GE_ARITH_JAVA && arith != GE_ARITH_FP32) return ge::fail(GE_ERR_ARG, "arith must be GE_ARITH_JAVA (0) or GE_ARITH_FP32 (1) (got %d)", arith);
    if (!h->stratified()) return ge::fail(GE_ERR_STATE, "the arithmetic is a choice of GE_MODE_STRATIFIED handles");
    if (arith == GE_ARITH_FP32) {
        if (!ge::strata_fp32_has_shape(h->cfg.dim))
            return ge::fail(GE_ERR_ARG, "GE_ARITH_FP32 has no kernel for dim = %d (more than four chunks of 64 lanes)", h->cfg.dim);
        GE_CHECK(check_handle(h));
        GE_CHECK(ge::strata_fp32_prepare(&h->strata, h->cfg.cost, h->cfg.xmax, h->stream));      // first use: (l, w) per nonzero
    }
    h->strata.arith = arith;
    return GE_OK;
}
ge_status ge_glove_get_arith(const ge_glove *h, int32_t *arith) {
    if (!h || !arith) return ge::fail(GE_ERR_ARG, "null argument");
    *arith = h->strata.arith;
    return GE_OK;
}

ge_status ge_glove_tile_info(ge_glove *h, int64_t out[4]) {
    if (!h || !out) return ge::fail(GE_ERR_ARG, "null argument");
    out[0] = h->n_tchunks; out[1] = h->lay.tile_nnz; out[2] = h->lay.tile_g; out[3] = h->lay.tile_cols;
    return GE_OK;
}
ge_status ge_glove_panel_info(ge_glove *h, int64_t out[4]) {
    if (!h || !out) return ge::fail(GE_ERR_ARG, "null argument");
    out[0] = h->n_pchunks; out[1] = h->lay.panel_nnz; out[2] = h->lay.panel_cols; out[3] = h->n_pchunks > 0 ? h->lay.panel_blocks : 0;
    return GE_OK;
}

ge_status ge_glove_get_info(ge_glove *h, ge_glove_info *info) {
    if (!h || !info) return ge::fail(GE_ERR_ARG, "null argument");
    std::memset(info, 0, sizeof(*info));
    info->group_width = 64; info->vector_width = h->hw.vw; info->chunks_per_lane = h->hw.nch;
    info->blocks = h->cfg.mode == GE_MODE_HOGWILD ? h->hw_blocks : 1;
    info->groups_in_flight = h->cfg.mode == GE_MODE_HOGWILD ? h->hw_workers : 1;
    info->hot_columns = h->hot_cols; info->hot_nonzeros = h->hot_nnz; info->hot_threshold = h->hot_threshold;
    info->chunks = h->n_chunks; info->hub_chunks = h->n_hchunks; info->long_rows = h->lay.long_rows; info->shared_chunks = h->lay.shared_chunks;
    info->flush_min = h->flush_every; info->row_stride = h->ds;
    if (h->stratified()) { info->blocks = info->groups_in_flight = h->strata.P; info->strata = h->strata.P; info->strata_path = h->strata.path; }
    info->placements = h->placements; info->placement_best_ms = h->place_best_ms; info->placement_worst_ms = h->place_worst_ms;
    if (h->blocked) {
        // one row access = the bytes a wavefront's row instruction moves: the row width of the table it touches
        // (the row as the update needs it: dim + 4 floats when fat; what the line-aligned layout pads it with is not counted)
        const int64_t acc = 4ll * (h->cfg.dim + (h->fat ? 4 : 0)), emb = h->emb16 ? 2ll * h->cfg.dim : acc;
        const int64_t aux = h->cfg.opt == GE_OPT_ADAGRAD ? 1 : 2;                 // accumulator rows per side
        const int64_t pair = 2 * (emb + aux * acc) + (h->fat ? 0 : 2 * 4 * (1 + aux));   // load + store of a row, its accumulator row(s) and, unless fat, its scalars
        info->runs = h->lay.n_runs;
        // a nonzero streams a pair; inside a hub tile the pair streams once per (focus row, group) instead, inside a hub panel once
        // per (focus row, panel)
        const int64_t streamed = h->cfg.nnz - h->lay.tile_nnz + h->lay.tile_visits - h->lay.panel_nnz + h->lay.panel_visits;
        info->schedule_bytes = h->cfg.nnz * 20 + streamed * pair + h->lay.n_runs * pair;
    }
    return GE_OK;
}

}  // extern "C"
namespace ge {
ge_status glove_extract_device_f32(ge_glove *h, float **rows, int32_t *vocab_size, int32_t *dim, int32_t *device) {
    DeviceBuf d;
    GE_CHECK(extract_to_device(h, false, &d.p));
    hipError_t e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return hip_failed("extract", e);
    *rows = static_cast<float *>(d.release()); *vocab_size = h->cfg.vocab_size; *dim = h->cfg.dim; *device = h->cfg.device;
    return GE_OK;
}
ge_status glove_epoch_segment(ge_glove *h, int32_t iteration, int32_t seg, int32_t nseg, int32_t leave_blocks, hipEvent_t after_reset) {
    GE_CHECK(check_handle(h));
    if (h->cfg.mode != GE_MODE_HOGWILD || h->cfg.shuffle == GE_SHUFFLE_JAVA) return ge::fail(GE_ERR_STATE, "a segmented epoch needs a GE_MODE_HOGWILD handle with a device-side order");
    if (nseg < 1 || nseg > 64 || seg < 0 || seg >= nseg) return ge::fail(GE_ERR_ARG, "segment %d of %d", seg, nseg);
    GloveParams p;
    fill_params(h, p, iteration);
    const int64_t n = h->cfg.nnz > 0 ? h->n_chunks : 0;
    const int64_t begin = n * seg / nseg, end = n * (seg + 1) / nseg;
    if (seg == 0) {
        GE_CHECK(begin_hogwild_epoch(h));
        h->seg_timed = 0;
    }
    if (end > begin) {
        h->seg_ticket[seg] = (unsigned long long)begin;
        GE_HIP(hipMemcpyAsync(p.queue, &h->seg_ticket[seg], sizeof(unsigned long long), hipMemcpyHostToDevice, h->stream));
        p.ticket_end = end;
        if (after_reset) GE_HIP(hipEventRecord(after_reset, h->stream));
        hipEvent_t *ev = &h->seg_ev[2 * h->seg_timed];
        for (int k = 0; k < 2; ++k) if (!ev[k]) GE_HIP(hipEventCreate(&ev[k]));
        GE_HIP(hipEventRecord(ev[0], h->stream));
        launch_hogwild(h, p, std::max(1, h->hw_blocks - std::max(0, leave_blocks)));
        GE_HIP(hipEventRecord(ev[1], h->stream));
        ++h->seg_timed;
        GE_HIP(hipGetLastError());
    }
    else if (after_reset) GE_HIP(hipEventRecord(after_reset, h->stream));
    if (seg == nseg - 1) GE_HIP(hipEventRecord(h->ev1, h->stream));
    return GE_OK;
}
ge_status glove_epoch_progress(ge_glove *h, const unsigned long long **counter, int64_t *tickets, hipEvent_t *done) {
    GE_CHECK(check_handle(h));
    if (counter) *counter = reinterpret_cast<const unsigned long long *>(h->dcost + 1);
    if (tickets) *tickets = h->cfg.nnz > 0 ? h->n_chunks : 0;
    if (done) *done = h->ev1;
    return GE_OK;
}
const std::vector<int32_t> *glove_kernel_hubs(const ge_glove *h) { return (h && h->blocked && h->cfg.hot_columns != GE_HOT_NONE) ? &h->lay.hubs : nullptr; }
const std::vector<int32_t> *glove_hub_counts(const ge_glove *h) { return h ? &h->lay.heavy_count : nullptr; }
ge_status glove_epoch_finish(ge_glove *h, double *cost_sum) {
    GE_CHECK(check_handle(h));
    double total = 0.0;
    GE_HIP(hipMemcpyAsync(&total, h->dcost, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    GE_HIP(hipStreamSynchronize(h->stream));
    // ge_glove_last_kernel_ms: the launches' own time summed (what the caller's exchanges between them took is the caller's to time)
    h->last_ms = 0.0f;
    for (int32_t k = 0; k < h->seg_timed; ++k) { float ms = 0.0f; GE_HIP(hipEventElapsedTime(&ms, h->seg_ev[2 * k], h->seg_ev[2 * k + 1])); h->last_ms += ms; }
    if (cost_sum) *cost_sum = total;
    return GE_OK;
}
const std::vector<int32_t> *glove_hub_columns(const ge_glove *h) { return h ? &h->lay.heavy : nullptr; }
ge_status glove_eval_view(const ge_glove *h, EvalView *out) {
    if (!h) return ge::fail(GE_ERR_ARG, "null ge_glove handle");
    const TableView foc = view_of(h, GE_STATE_FOCUS), ctx = view_of(h, GE_STATE_CONTEXT);
    const TableView fb = view_of(h, GE_STATE_FBIAS), cb = view_of(h, GE_STATE_CBIAS);
    out->focus = foc.base; out->context = ctx.base; out->focus_stride = foc.stride; out->context_stride = ctx.stride;
    out->fbias = fb.first(); out->cbias = cb.first(); out->fbias_stride = fb.stride; out->cbias_stride = cb.stride;
    out->emb16 = ctx.bf16 ? 1 : 0;
    out->hub32 = ctx.bf16 && h->n_hub > 0 ? h->hub32 : nullptr;
    out->hub_index = out->hub32 ? h->dhub_index : nullptr;
    out->xmax = h->cfg.xmax; out->vocab_size = h->cfg.vocab_size; out->dim = h->cfg.dim;
    out->row_begin = h->cfg.row_begin; out->row_end = h->cfg.row_begin + h->rows;
    out->cost_kind = h->cfg.cost; out->device = h->cfg.device; out->stream = h->stream;
    out->learning_rate = h->cfg.learning_rate;
    return GE_OK;
}
ge_status glove_sync_view(ge_glove *h, int32_t *opt, int32_t *mode, void **stream, int32_t *device) {
    if (!h) return ge::fail(GE_ERR_ARG, "null ge_glove handle");
    *opt = h->cfg.opt; *mode = h->cfg.mode; *stream = (void *)h->stream; *device = h->cfg.device;
    return GE_OK;
}
}  // namespace ge
extern "C" {

void ge_glove_destroy(ge_glove *h) {
    if (!h) return;
    (void)hipSetDevice(h->cfg.device);
    for (hipEvent_t e : h->seg_ev) if (e) (void)hipEventDestroy(e);
    for (void *q : h->owned) (void)hipFree(q);
    h->lay.release();
    h->strata.release();
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    delete h;
}

// ---- guarded entry points (bodies above allocate on the host) ----
ge_status ge_glove_create(const ge_glove_cfg *cfg, const int32_t *I, const int32_t *J, const float *X, ge_glove **out) { GE_GUARD(ge_glove_create_impl(cfg, I, J, X, false, out)); }
ge_status ge_glove_create_coo(const ge_glove_cfg *cfg, const ge_coo *coo, ge_glove **out) { GE_GUARD(ge_glove_create_coo_impl(cfg, coo, out)); }
ge_status ge_glove_epoch(ge_glove *h, int32_t iteration, double *cost_sum) { GE_GUARD(ge_glove_epoch_impl(h, iteration, cost_sum)); }
ge_status ge_glove_epoch_order(ge_glove *h, int32_t iteration, int32_t *out, int64_t count) { GE_GUARD(ge_glove_epoch_order_impl(h, iteration, out, count)); }

}  // extern "C"
