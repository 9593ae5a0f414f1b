// match.hip -- entity matching over a table of vectors behind the C ABI: every pair of indexed rows whose score reaches a
// threshold, and the groups those pairs connect.  The table is prepared as nn.hip prepares it (k_match_prepare), the scores are
// the same fp32 chains on the fp32 matrix cores, walked over the upper triangle only with a threshold epilogue (k_match_join),
// the survivors are sorted by (a, b) (rocprim radix sort), and the connected components come from a union-find over that list
// (k_match_hook, k_match_compress).  The reference has no counterpart; the semantics are written down in include/geglove.h.
#include "ge_common.h"
#include "ge_glove_internal.h"
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>
#include <rocprim/device/device_radix_sort.hpp>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;

constexpr int MT_MAX_DIM = 1024;
constexpr int64_t MT_MAX_FLOATS = (int64_t)1 << 35;          // floats of input one index accepts (128 GiB as fp32)
constexpr int64_t MT_SLAB_FLOATS = (int64_t)1 << 26;         // a 256 MB slab of rows per upload
constexpr int64_t MT_MAX_PAIRS = (int64_t)1 << 28;           // the largest cap a run accepts
constexpr int64_t MT_MAX_ITEMS = (int64_t)1 << 30;           // workgroups of one join launch

// ---------------------------------------------------------------------------------------------------------------------
// Prepare: nn.hip's k_nn_prepare, operation for operation (the index is bit for bit ge_nn_*'s).  One wave takes 64 rows: pieces of
// 64 columns are read coalesced into LDS, lane r then walks row r of the piece in ascending d (the fp64 sum of squares is a
// sequential chain), and a second coalesced pass writes x / n rounded to fp32 once into the table, whose rows are padded with
// zeros to D4 = dim rounded up to 4 floats.  rowmap: NULL or the source row of every output row.  A non-finite value raises *flag.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int PREP_ROWS = 64, PREP_COLS = 64, PREP_STRIDE = 65;

__global__ __launch_bounds__(64) void k_match_prepare(const float *__restrict__ src, const int32_t *__restrict__ rowmap, int64_t n_rows, int32_t D,
                                                      int32_t D4, int32_t metric, float *__restrict__ out, int32_t *__restrict__ flag) {
    __shared__ float tile[PREP_ROWS * PREP_STRIDE];
    __shared__ double norm[PREP_ROWS];
    const int lane = (int)threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * PREP_ROWS;
    const int rows = (int)(n_rows - row0 < PREP_ROWS ? n_rows - row0 : PREP_ROWS);
    bool bad = false;
    if (metric == GE_NN_COSINE) {
        double sum = 0.0;
        for (int d0 = 0; d0 < D; d0 += PREP_COLS) {
            const int d = d0 + lane;
            for (int r = 0; r < rows; ++r) {
                const int64_t s = rowmap ? (int64_t)rowmap[row0 + r] : row0 + r;
                tile[r * PREP_STRIDE + lane] = d < D ? src[s * D + d] : 0.0f;
            }
            __syncthreads();
            const int lim = D - d0 < PREP_COLS ? D - d0 : PREP_COLS;
            if (lane < rows)
                for (int c = 0; c < lim; ++c) {
                    const double x = (double)tile[lane * PREP_STRIDE + c];
                    sum += x * x;
                }
            __syncthreads();
        }
        norm[lane] = sqrt(sum);
        __syncthreads();
    }
    for (int d0 = 0; d0 < D4; d0 += PREP_COLS) {
        const int d = d0 + lane;
        if (d >= D4) break;
        for (int r = 0; r < rows; ++r) {
            const int64_t s = rowmap ? (int64_t)rowmap[row0 + r] : row0 + r;
            float x = d < D ? src[s * D + d] : 0.0f;
            bad |= !(fabsf(x) <= 3.402823466e38f);
            if (metric == GE_NN_COSINE) {
                const double n = norm[r];
                x = n > 0.0 ? (float)((double)x / n) : 0.0f;
            }
            out[(row0 + r) * D4 + d] = x;
        }
    }
    if (bad) *flag = 1;
}

// ---------------------------------------------------------------------------------------------------------------------
// Join.  The tile is k_nn_score_select's: MT_TQ queries x MT_TC candidates, panels of MT_DK columns staged in LDS as
// [row][MT_LS floats] (MT_LS = 34 = 2 mod 32, so the 32 lanes one ds_read_b32 cycle serves hit 32 different banks; the next
// panel travels in registers meanwhile), wave w carrying queries 16 w .. 16 w + 15 against all MT_TC candidates through
// v_mfma_f32_16x16x4_f32: eight independent accumulators, each bit for bit an fmaf chain over ascending d.  Queries and
// candidates are the same table, and only the upper triangle is walked.
//
// The grid is a list of items.  The candidate tiles are cut into chunks of R tiles; chunk c is wanted by the query tiles
// 0 .. min(qtiles, 2 (c + 1) R) - 1 (query tile qt needs the candidate tiles from (64 qt + 1) / 128 on: those that hold a
// position above its first).  Item = (chunk, query tile), chunk-major: chunk_first[c] is the first item of chunk c, so a
// workgroup finds its chunk by bisection and its query tile by subtraction.  Every item walks at most R tiles, so no workgroup
// runs longer than R tiles after the others have finished, and the workgroups in flight together read the same candidate panels.
//
// Epilogue per candidate tile: a lane compares its 32 scores with the threshold (a NaN fails the compare, as -inf would) and
// tests a < b per element; the wave counts its survivors with a prefix sum over the lanes and, where there are any, reserves
// that many slots with ONE 64-bit integer atomic add; each survivor writes (posA << 32 | posB, score) while its slot is below
// `cap`.  The counter counts past the cap: it is the exact number of qualifying pairs.  Which slot a pair lands in depends on
// timing; the sort by key that follows does not.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int MT_TQ = 64, MT_TC = 128, MT_DK = 32, MT_LS = 34;
constexpr int MT_LOADS = (MT_TQ + MT_TC) * (MT_DK / 4) / 256;   // 16-byte pieces a thread moves per panel: 2 of queries, 4 of candidates
constexpr int MT_WG_PER_CU = 3;   // 147 VGPRs: three waves per SIMD, as the CAP 32 instance of k_nn_score_select

__global__ __launch_bounds__(256, MT_WG_PER_CU) void k_match_join(const float *__restrict__ X, int64_t n, int32_t D4, const int64_t *__restrict__ chunk_first,
                                                                  int32_t nchunks, int32_t R, float thr, u64 cap, u64 *__restrict__ counter,
                                                                  uint2 *__restrict__ keys, float *__restrict__ scores) {
    __shared__ float sq[MT_TQ * MT_LS];
    __shared__ float sx[MT_TC * MT_LS];

    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    // the item: chunk by bisection (chunk_first[0] = 0 <= item < chunk_first[nchunks]), query tile by subtraction
    const int64_t item = (int64_t)blockIdx.x;
    int lo = 0, hi = nchunks;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (chunk_first[mid] <= item) lo = mid; else hi = mid;
    }
    const int64_t qt = item - chunk_first[lo];
    const int64_t q0 = qt * MT_TQ;
    const int64_t ctiles = (n + MT_TC - 1) / MT_TC;
    const int64_t t_first = (q0 + 1) / MT_TC;                          // the first candidate tile with a position above q0
    const int64_t t_lo = (int64_t)lo * R > t_first ? (int64_t)lo * R : t_first;
    const int64_t t_hi = ((int64_t)lo + 1) * R < ctiles ? ((int64_t)lo + 1) * R : ctiles;
    const int64_t c_begin = t_lo * MT_TC;
    const int64_t c_end = t_hi * MT_TC < n ? t_hi * MT_TC : n;
    if (q0 >= n || c_begin >= c_end) return;

    // what this thread stages: piece i of a panel is row (tid + 256 i) >> 3, columns 4 ((tid + 256 i) & 7) ..
    const int c4 = (tid & 7) * 4, prow = tid >> 3;                      // rows prow, prow + 32 of the queries; prow + 32 j of the candidates
    const float *qsrc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int64_t qg = q0 + prow + 32 * i;
        qsrc[i] = qg < n ? X + qg * D4 : nullptr;
    }
    f32x4 pre[MT_LOADS];
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
        for (int i = 0; i < MT_LOADS; ++i) {
            float *dst = (i < 2 ? sq + (prow + 32 * i) * MT_LS : sx + (prow + 32 * (i - 2)) * MT_LS) + c4;   // 8-byte aligned: MT_LS and c4 are even
            *reinterpret_cast<float2 *>(dst) = float2{pre[i][0], pre[i][1]};
            *reinterpret_cast<float2 *>(dst + 2) = float2{pre[i][2], pre[i][3]};
        }
    };

    // the four queries whose scores a lane holds: local rows 4 (lane >> 4) + reg of the wave's sixteen
    const int qb = wave * 16;
    const uint32_t qa = (uint32_t)q0 + (uint32_t)(qb + 4 * (lane >> 4));
    const int xa = (qb + (lane & 15)) * MT_LS + (lane >> 4);
    const int xb = (lane & 15) * MT_LS + (lane >> 4);

    fetch(c_begin, 0);
    for (int64_t ct = c_begin; ct < c_end; ct += MT_TC) {
        f32x4 acc[MT_TC / 16];
#pragma unroll
        for (int t = 0; t < MT_TC / 16; ++t) acc[t] = f32x4{0, 0, 0, 0};
        for (int d0 = 0; d0 < D4; d0 += MT_DK) {
            __syncthreads();
            stage();
            __syncthreads();
            if (d0 + MT_DK < D4) fetch(ct, d0 + MT_DK);
            else if (ct + MT_TC < c_end) fetch(ct + MT_TC, 0);
            auto step = [&](int dd) {
                const float a = sq[xa + dd];
                float b[MT_TC / 16];
#pragma unroll
                for (int t = 0; t < MT_TC / 16; ++t) b[t] = sx[xb + t * 16 * MT_LS + dd];
#pragma unroll
                for (int t = 0; t < MT_TC / 16; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b[t], acc[t], 0, 0, 0);
            };
            if (D4 - d0 >= MT_DK) {                                   // a whole panel: unrolled, so the reads of a step run ahead of its products
#pragma unroll
                for (int dd = 0; dd < MT_DK; dd += 4) step(dd);
            } else {
#pragma unroll 1
                for (int dd = 0; dd < D4 - d0; dd += 4) step(dd);
            }
        }
        // C/D of the f32 form: column (candidate) = lane & 15, row (query) = 4 * (lane >> 4) + register.
        // bit 4 t + reg of `mask`: the pair (qa + reg, ct + 16 t + (lane & 15)) qualifies.  b < c_end <= n, and a < b, so both are rows.
        // Positions are below 2^31: the epilogue works on their 32-bit values.
        const uint32_t cl = (uint32_t)ct + (uint32_t)(lane & 15), ce = (uint32_t)c_end;
        uint32_t mask = 0;
#pragma unroll
        for (int t = 0; t < MT_TC / 16; ++t) {
            const uint32_t c = cl + 16u * t;
#pragma unroll
            for (int reg = 0; reg < 4; ++reg)
                if (c < ce && qa + reg < c && acc[t][reg] >= thr) mask |= 1u << (4 * t + reg);
        }
        if (__ballot(mask != 0) != 0) {                               // uniform over the wave
            const int mine = __popc(mask);
            int upto = mine;                                          // survivors of lanes 0 .. lane
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int v = __shfl_up(upto, off);
                if (lane >= off) upto += v;
            }
            const int total = __shfl(upto, 63);
            u64 base = 0;
            if (lane == 0) base = atomicAdd(counter, (u64)total);
            const uint32_t blo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)base);
            const uint32_t bhi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(base >> 32));
            u64 slot = (((u64)bhi << 32) | blo) + (u64)(upto - mine);
#pragma unroll
            for (int t = 0; t < MT_TC / 16; ++t)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg)
                    if (mask & (1u << (4 * t + reg))) {
                        if (slot < cap) {
                            keys[slot] = uint2{cl + 16u * t, qa + reg};          // little-endian: posA << 32 | posB
                            scores[slot] = acc[t][reg];
                        }
                        ++slot;
                    }
        }
    }
}

// the sorted keys as original row ids (ids: NULL = positions are ids)
__global__ __launch_bounds__(256) void k_match_unpack(const u64 *__restrict__ keys, int64_t m, const int32_t *__restrict__ ids, int64_t n,
                                                      int32_t *__restrict__ a, int32_t *__restrict__ b, int32_t *__restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const int64_t pa = (int64_t)(keys[i] >> 32), pb = (int64_t)(keys[i] & 0xffffffffu);
    if (pa >= n || pb >= n) { *flag = 1; return; }
    a[i] = ids ? ids[pa] : (int32_t)pa;
    b[i] = ids ? ids[pb] : (int32_t)pb;
}

// ---------------------------------------------------------------------------------------------------------------------
// Components: union-find on a parent array of positions.  parent[x] <= x always (a root is hooked under a SMALLER root, and
// shortening a path only lowers a parent), so there are no cycles, a find walks at most n parents, and the root of a component
// is its smallest position -- for any interleaving.  A hook is an integer compare-and-swap on a root (expected value = the
// root itself: a position that is no root any more never becomes one again, so the swap fails and the pair is taken up again
// from the new parent); every failed swap means another thread hooked that root, which happens at most n - 1 times in all, so a
// pair that has retried n times, or a find that has walked n parents, has met a defect: it raises *flag and gives up.
// While hooks run the parents are read and lowered with device-scope integer atomics (a plain load may be served from a CU's
// L1); k_match_compress runs in a later launch and reads them plainly.
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int32_t match_find_live(int32_t *parent, int32_t x, int64_t n, int32_t *flag) {
    int32_t p = __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (int64_t step = 0; p != x; ++step) {
        if (step >= n || p < 0 || p > x) { *flag = 1; return -1; }
        const int32_t g = __hip_atomic_load(parent + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (g < 0 || g > p) { *flag = 1; return -1; }
        if (g != p) atomicMin(parent + x, g);                         // x is no root: point it at its grandparent (still an ancestor)
        x = p; p = g;
    }
    return x;
}

__global__ __launch_bounds__(256) void k_match_init(int32_t *__restrict__ parent, int32_t *__restrict__ size, int64_t n) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p < n) { parent[p] = (int32_t)p; size[p] = 0; }
}

__global__ __launch_bounds__(256) void k_match_hook(const u64 *__restrict__ keys, int64_t m, int32_t *parent, int64_t n, int32_t *flag) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    int64_t pa = (int64_t)(keys[i] >> 32), pb = (int64_t)(keys[i] & 0xffffffffu);
    if (pa >= n || pb >= n) { *flag = 1; return; }
    int32_t u = (int32_t)pa, v = (int32_t)pb;
    for (int64_t tries = 0;; ++tries) {
        if (tries > n) { *flag = 1; return; }
        const int32_t ru = match_find_live(parent, u, n, flag);
        if (ru < 0) return;
        const int32_t rv = match_find_live(parent, v, n, flag);
        if (rv < 0) return;
        if (ru == rv) return;
        const int32_t big = ru > rv ? ru : rv, small = ru > rv ? rv : ru;
        if (atomicCAS(parent + big, big, small) == big) return;      // `big` was a root and hangs under `small` now
        u = big; v = small;
    }
}

// root[p] by a plain walk (at most n parents), label[p] = the root's original id, size[root] counts its rows
__global__ __launch_bounds__(256) void k_match_compress(const int32_t *__restrict__ parent, int64_t n, const int32_t *__restrict__ ids,
                                                        int32_t *__restrict__ label, int32_t *__restrict__ size, int32_t *__restrict__ flag) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    int64_t x = p;
    for (int64_t step = 0;; ++step) {
        const int64_t up = parent[x];
        if (up == x) break;
        if (step >= n || up < 0 || up > x) { *flag = 1; return; }
        x = up;
    }
    label[p] = ids ? ids[x] : (int32_t)x;
    atomicAdd(size + x, 1);
}

// out[0] components, out[1] components of at least two rows, out[2] rows inside those, out[3] the largest component
__global__ __launch_bounds__(256) void k_match_summary(const int32_t *__restrict__ size, int64_t n, u64 *__restrict__ out) {
    __shared__ u64 part[4];
    if (threadIdx.x < 4) part[threadIdx.x] = 0;
    __syncthreads();
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int32_t s = p < n ? size[p] : 0;                            // > 0 exactly at the roots
    if (s > 0) {
        atomicAdd(&part[0], (u64)1);
        if (s >= 2) { atomicAdd(&part[1], (u64)1); atomicAdd(&part[2], (u64)s); }
        atomicMax(&part[3], (u64)s);
    }
    __syncthreads();
    if (threadIdx.x < 3 && part[threadIdx.x]) atomicAdd(out + threadIdx.x, part[threadIdx.x]);
    if (threadIdx.x == 3 && part[3]) atomicMax(out + 3, part[3]);
}

struct DeviceBuffers {                      // freed on every way out
    std::vector<void *> ptrs;
    std::vector<hipEvent_t> ev;
    ~DeviceBuffers() { for (void *q : ptrs) (void)hipFree(q); for (hipEvent_t e : ev) (void)hipEventDestroy(e); }
    ge_status alloc(void **q, size_t bytes) { GE_HIP(hipMalloc(q, std::max<size_t>(bytes, 16))); ptrs.push_back(*q); return GE_OK; }
    ge_status events(int count) {
        for (int i = 0; i < count; ++i) { hipEvent_t e = nullptr; GE_HIP(hipEventCreate(&e)); ev.push_back(e); }
        return GE_OK;
    }
};

}  // namespace

struct ge_match {
    int32_t metric = 0, device = 0, dim = 0, d4 = 0;
    int64_t n_rows = 0, n_indexed = 0;
    hipStream_t stream = nullptr;
    std::vector<int32_t> subset;            // original row id of every indexed row; empty = all rows
    float *dx = nullptr;                    // [n_indexed][d4], prepared
    int32_t *dids = nullptr;                // `subset` on the device, or NULL
    // the last run
    int state = 0;                          // 0 = none yet, 1 = results, 2 = overflowed
    int64_t found = 0;
    std::vector<int32_t> a, b, label;
    std::vector<float> score;
    ge_match_summary summary{};
    float prepare_ms = 0, join_ms = 0, sort_ms = 0, components_ms = 0;
    ~ge_match() { if (dx) (void)hipFree(dx); if (dids) (void)hipFree(dids); }
};

namespace {

ge_status check_create(int64_t n_rows, int32_t dim, const int32_t *subset, int64_t n_subset, const ge_match_cfg *cfg) {
    if (!cfg) return ge::fail(GE_ERR_ARG, "ge_match_cfg is null");
    if (cfg->metric != GE_NN_COSINE && cfg->metric != GE_NN_DOT) return ge::fail(GE_ERR_ARG, "match: unknown metric %d", cfg->metric);
    if (dim < 1 || dim > MT_MAX_DIM) return ge::fail(GE_ERR_ARG, "match: dim %d outside [1, %d]", dim, MT_MAX_DIM);
    if (n_rows < 1 || n_rows >= INT_MAX) return ge::fail(GE_ERR_ARG, "match: %lld rows outside [1, 2^31 - 2]", (long long)n_rows);
    if (n_rows > MT_MAX_FLOATS / dim)
        return ge::fail(GE_ERR_ARG, "match: %lld rows of %d floats are more than one index holds (%lld floats)", (long long)n_rows, dim, (long long)MT_MAX_FLOATS);
    if (subset) {
        if (n_subset < 1 || n_subset > n_rows) return ge::fail(GE_ERR_ARG, "match: a subset of %lld of %lld rows", (long long)n_subset, (long long)n_rows);
        for (int64_t i = 0; i < n_subset; ++i) {
            if (subset[i] < 0 || subset[i] >= n_rows) return ge::fail(GE_ERR_ARG, "match: subset[%lld] = %d outside [0, %lld)", (long long)i, subset[i], (long long)n_rows);
            if (i > 0 && subset[i] <= subset[i - 1]) return ge::fail(GE_ERR_ARG, "match: the subset is not strictly ascending at [%lld]", (long long)i);
        }
    }
    return GE_OK;
}

// rows (host: slab by slab; dev: in place) -> table[rows_out][d4], prepared; *ms += the kernels' time
ge_status prepare_rows(const float *host, const float *dev, const int32_t *host_map, const int32_t *dev_map, int64_t rows_out, int32_t dim,
                       int32_t metric, float *table, hipStream_t stream, float *ms_out) {
    const int D = dim, D4 = (D + 3) / 4 * 4;
    const int64_t slab_rows = std::min<int64_t>(std::max<int64_t>(PREP_ROWS, MT_SLAB_FLOATS / D / PREP_ROWS * PREP_ROWS), rows_out);
    DeviceBuffers B;
    float *dslab = nullptr;
    int32_t *dflag = nullptr;
    GE_CHECK(B.events(2));
    if (host) GE_CHECK(B.alloc((void **)&dslab, sizeof(float) * (size_t)slab_rows * D));
    GE_CHECK(B.alloc((void **)&dflag, sizeof(int32_t)));
    GE_HIP(hipMemsetAsync(dflag, 0, sizeof(int32_t), stream));
    std::vector<float> packed;
    if (host && host_map) packed.resize((size_t)slab_rows * D);
    float total = 0;
    for (int64_t begin = 0; begin < rows_out; begin += slab_rows) {
        const int64_t rows = std::min(slab_rows, rows_out - begin);
        const float *x = dev;
        const int32_t *map = dev ? (dev_map ? dev_map + begin : nullptr) : nullptr;
        if (host) {
            const float *from = host + begin * D;
            if (host_map) {
                for (int64_t r = 0; r < rows; ++r) std::memcpy(&packed[(size_t)r * D], host + (int64_t)host_map[begin + r] * D, sizeof(float) * (size_t)D);
                from = packed.data();
            }
            GE_HIP(hipMemcpyAsync(dslab, from, sizeof(float) * (size_t)rows * D, hipMemcpyHostToDevice, stream));
            x = dslab;
        } else if (!dev_map) {
            x = dev + begin * D;
        }
        GE_HIP(hipEventRecord(B.ev[0], stream));
        hipLaunchKernelGGL(k_match_prepare, dim3((unsigned)((rows + PREP_ROWS - 1) / PREP_ROWS)), dim3(64), 0, stream, x, map, rows, D, D4, metric,
                           table + begin * D4, dflag);
        GE_HIP(hipGetLastError());
        GE_HIP(hipEventRecord(B.ev[1], stream));
        GE_HIP(hipStreamSynchronize(stream));                                       // the slab buffer (and `packed`) are free again
        float ms = 0;
        GE_HIP(hipEventElapsedTime(&ms, B.ev[0], B.ev[1]));
        total += ms;
    }
    int32_t flag = 0;
    GE_HIP(hipMemcpyAsync(&flag, dflag, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    GE_HIP(hipStreamSynchronize(stream));
    if (flag) return ge::fail(GE_ERR_ARG, "match: non-finite input (rows)");
    *ms_out += total;
    return GE_OK;
}

ge_status create_impl(const float *host, const float *dev, int64_t n_rows, int32_t dim, const int32_t *subset, int64_t n_subset, const ge_match_cfg *cfg,
                      ge_match **out) {
    std::unique_ptr<ge_match> p(new ge_match);
    p->metric = cfg->metric; p->device = cfg->device; p->stream = (hipStream_t)cfg->stream;
    p->dim = dim; p->d4 = (dim + 3) / 4 * 4; p->n_rows = n_rows; p->n_indexed = subset ? n_subset : n_rows;
    if (subset) p->subset.assign(subset, subset + n_subset);
    GE_HIP(hipMalloc((void **)&p->dx, sizeof(float) * (size_t)p->n_indexed * p->d4));
    if (subset) {
        GE_HIP(hipMalloc((void **)&p->dids, sizeof(int32_t) * (size_t)n_subset));
        GE_HIP(hipMemcpyAsync(p->dids, subset, sizeof(int32_t) * (size_t)n_subset, hipMemcpyHostToDevice, p->stream));
    }
    GE_CHECK(prepare_rows(host, dev, subset, p->dids, p->n_indexed, dim, p->metric, p->dx, p->stream, &p->prepare_ms));
    *out = p.release();
    return GE_OK;
}

ge_status match_create_host(const float *rows, int64_t n_rows, int32_t dim, const int32_t *subset, int64_t n_subset, const ge_match_cfg *cfg, ge_match **out) {
    if (out) *out = nullptr;
    if (!rows || !out) return ge::fail(GE_ERR_ARG, "ge_match_create: rows or out is null");
    GE_CHECK(check_create(n_rows, dim, subset, n_subset, cfg));
    GE_CHECK(ge::select_device(cfg->device));
    return create_impl(rows, nullptr, n_rows, dim, subset, n_subset, cfg, out);
}

ge_status match_create_glove(ge_glove *h, const int32_t *subset, int64_t n_subset, const ge_match_cfg *cfg, ge_match **out) {
    if (out) *out = nullptr;
    if (!h || !out) return ge::fail(GE_ERR_ARG, "ge_glove_match_create: handle or out is null");
    if (!cfg) return ge::fail(GE_ERR_ARG, "ge_match_cfg is null");
    if (cfg->metric != GE_NN_COSINE && cfg->metric != GE_NN_DOT) return ge::fail(GE_ERR_ARG, "match: unknown metric %d", cfg->metric);
    float *d = nullptr;
    int32_t V = 0, D = 0, device = 0;
    GE_CHECK(ge::glove_extract_device_f32(h, &d, &V, &D, &device));   // a fresh buffer: no trainer table is written
    ge_match_cfg own = *cfg;
    own.device = device;                                              // the rows live on the handle's device
    ge_status st = check_create(V, D, subset, n_subset, &own);
    if (st == GE_OK) st = create_impl(nullptr, d, V, D, subset, n_subset, &own, out);
    (void)hipFree(d);
    return st;
}

// the chunks of the join's grid: R candidate tiles each, chunk c wanted by min(qtiles, 2 (c + 1) R) query tiles
void plan_join(int64_t n, int32_t *R_out, std::vector<int64_t> *first) {
    const int64_t ctiles = (n + MT_TC - 1) / MT_TC, qtiles = (n + MT_TQ - 1) / MT_TQ;
    int64_t R = std::max<int64_t>(1, std::min<int64_t>(256, qtiles * ctiles / 2 / 16384));   // about 16 k items where the triangle has them
    for (;; R *= 2) {
        const int64_t nchunks = (ctiles + R - 1) / R;
        first->assign((size_t)nchunks + 1, 0);
        for (int64_t c = 0; c < nchunks; ++c) (*first)[(size_t)c + 1] = (*first)[(size_t)c] + std::min<int64_t>(qtiles, 2 * (c + 1) * R);
        if (first->back() <= MT_MAX_ITEMS) break;
    }
    *R_out = (int32_t)R;
}

ge_status match_run(ge_match *p, float threshold, int64_t max_pairs) {
    if (!(std::fabs(threshold) <= 3.402823466e38f)) return ge::fail(GE_ERR_ARG, "match: the threshold must be finite");
    if (max_pairs < 1 || max_pairs > MT_MAX_PAIRS) return ge::fail(GE_ERR_ARG, "match: max_pairs %lld outside [1, 2^28]", (long long)max_pairs);
    if (!p) return ge::fail(GE_ERR_ARG, "null ge_match handle");
    GE_CHECK(ge::select_device(p->device));
    hipStream_t stream = p->stream;
    const int64_t n = p->n_indexed;
    p->state = 0; p->found = 0; p->summary = ge_match_summary{};
    p->a.clear(); p->b.clear(); p->score.clear(); p->label.clear();
    p->join_ms = p->sort_ms = p->components_ms = 0;

    const int64_t all_pairs = n * (n - 1) / 2;                        // n < 2^31: no overflow
    const int64_t cap = std::min(max_pairs, all_pairs);               // no run finds more, so no slot at or past it is ever written
    DeviceBuffers B;
    GE_CHECK(B.events(4));
    u64 *dcount = nullptr, *dkey = nullptr, *dsum = nullptr;
    float *dscore = nullptr;
    int32_t *dflag = nullptr;
    int64_t *dfirst = nullptr;
    GE_CHECK(B.alloc((void **)&dcount, sizeof(u64)));
    GE_CHECK(B.alloc((void **)&dsum, sizeof(u64) * 4));
    GE_CHECK(B.alloc((void **)&dflag, sizeof(int32_t)));
    GE_CHECK(B.alloc((void **)&dkey, sizeof(u64) * (size_t)cap));
    GE_CHECK(B.alloc((void **)&dscore, sizeof(float) * (size_t)cap));
    GE_HIP(hipMemsetAsync(dcount, 0, sizeof(u64), stream));
    GE_HIP(hipMemsetAsync(dsum, 0, sizeof(u64) * 4, stream));
    GE_HIP(hipMemsetAsync(dflag, 0, sizeof(int32_t), stream));

    // join
    u64 found = 0;
    if (n >= 2) {
        int32_t R = 1;
        std::vector<int64_t> first;
        plan_join(n, &R, &first);
        GE_CHECK(B.alloc((void **)&dfirst, sizeof(int64_t) * first.size()));
        GE_HIP(hipMemcpyAsync(dfirst, first.data(), sizeof(int64_t) * first.size(), hipMemcpyHostToDevice, stream));
        GE_HIP(hipEventRecord(B.ev[0], stream));
        hipLaunchKernelGGL(k_match_join, dim3((unsigned)first.back()), dim3(256), 0, stream, (const float *)p->dx, n, p->d4, (const int64_t *)dfirst,
                           (int32_t)(first.size() - 1), R, threshold, (u64)cap, dcount, reinterpret_cast<uint2 *>(dkey), dscore);
        GE_HIP(hipGetLastError());
        GE_HIP(hipEventRecord(B.ev[1], stream));
        GE_HIP(hipMemcpyAsync(&found, dcount, sizeof(u64), hipMemcpyDeviceToHost, stream));
        GE_HIP(hipStreamSynchronize(stream));                         // also keeps `first` alive until its copy is done
        GE_HIP(hipEventElapsedTime(&p->join_ms, B.ev[0], B.ev[1]));
    }
    p->found = (int64_t)found;
    if ((int64_t)found > max_pairs) {
        p->state = 2;
        p->summary.pairs = (int64_t)found;
        return ge::fail(GE_ERR_OVERFLOW, "match: %lld pairs reach the threshold, more than max_pairs = %lld: raise the threshold or max_pairs", (long long)found,
                        (long long)max_pairs);
    }
    if ((int64_t)found > cap) return ge::fail(GE_ERR_STATE, "match: %lld pairs found among %lld rows", (long long)found, (long long)n);
    const int64_t m = (int64_t)found;

    // sort by key, then the keys as original ids
    u64 *dsorted = nullptr;
    float *dsscore = nullptr;
    int32_t *da = nullptr, *db = nullptr;
    if (m > 0) {
        void *dtmp = nullptr;
        size_t tmp_bytes = 0;
        unsigned end_bit = 33;
        while (end_bit < 64 && ((int64_t)1 << (end_bit - 32)) < n) ++end_bit;     // positions are below n
        GE_CHECK(B.alloc((void **)&dsorted, sizeof(u64) * (size_t)m));
        GE_CHECK(B.alloc((void **)&dsscore, sizeof(float) * (size_t)m));
        GE_CHECK(B.alloc((void **)&da, sizeof(int32_t) * (size_t)m));
        GE_CHECK(B.alloc((void **)&db, sizeof(int32_t) * (size_t)m));
        GE_HIP(rocprim::radix_sort_pairs(nullptr, tmp_bytes, (const u64 *)dkey, dsorted, (const float *)dscore, dsscore, (size_t)m, 0, end_bit, stream));
        GE_CHECK(B.alloc(&dtmp, tmp_bytes));
        GE_HIP(hipEventRecord(B.ev[0], stream));
        GE_HIP(rocprim::radix_sort_pairs(dtmp, tmp_bytes, (const u64 *)dkey, dsorted, (const float *)dscore, dsscore, (size_t)m, 0, end_bit, stream));
        hipLaunchKernelGGL(k_match_unpack, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, stream, (const u64 *)dsorted, m, (const int32_t *)p->dids, n, da, db,
                           dflag);
        GE_HIP(hipGetLastError());
        GE_HIP(hipEventRecord(B.ev[1], stream));
    }

    // components
    int32_t *dparent = nullptr, *dsize = nullptr, *dlabel = nullptr;
    GE_CHECK(B.alloc((void **)&dparent, sizeof(int32_t) * (size_t)n));
    GE_CHECK(B.alloc((void **)&dsize, sizeof(int32_t) * (size_t)n));
    GE_CHECK(B.alloc((void **)&dlabel, sizeof(int32_t) * (size_t)n));
    const dim3 rows_grid((unsigned)((n + 255) / 256));
    GE_HIP(hipEventRecord(B.ev[2], stream));
    hipLaunchKernelGGL(k_match_init, rows_grid, dim3(256), 0, stream, dparent, dsize, n);
    GE_HIP(hipGetLastError());
    if (m > 0) {
        hipLaunchKernelGGL(k_match_hook, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, stream, (const u64 *)dsorted, m, dparent, n, dflag);
        GE_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_match_compress, rows_grid, dim3(256), 0, stream, (const int32_t *)dparent, n, (const int32_t *)p->dids, dlabel, dsize, dflag);
    GE_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_match_summary, rows_grid, dim3(256), 0, stream, (const int32_t *)dsize, n, dsum);
    GE_HIP(hipGetLastError());
    GE_HIP(hipEventRecord(B.ev[3], stream));

    std::vector<int32_t> a((size_t)m), b((size_t)m), label((size_t)n);
    std::vector<float> score((size_t)m);
    u64 sum[4] = {0, 0, 0, 0};
    int32_t flag = 0;
    if (m > 0) {
        GE_HIP(hipMemcpyAsync(a.data(), da, sizeof(int32_t) * (size_t)m, hipMemcpyDeviceToHost, stream));
        GE_HIP(hipMemcpyAsync(b.data(), db, sizeof(int32_t) * (size_t)m, hipMemcpyDeviceToHost, stream));
        GE_HIP(hipMemcpyAsync(score.data(), dsscore, sizeof(float) * (size_t)m, hipMemcpyDeviceToHost, stream));
    }
    GE_HIP(hipMemcpyAsync(label.data(), dlabel, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, stream));
    GE_HIP(hipMemcpyAsync(sum, dsum, sizeof(sum), hipMemcpyDeviceToHost, stream));
    GE_HIP(hipMemcpyAsync(&flag, dflag, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    GE_HIP(hipStreamSynchronize(stream));
    if (m > 0) GE_HIP(hipEventElapsedTime(&p->sort_ms, B.ev[0], B.ev[1]));
    GE_HIP(hipEventElapsedTime(&p->components_ms, B.ev[2], B.ev[3]));
    if (flag) return ge::fail(GE_ERR_STATE, "match: the components kernels met a pair or a parent outside the index, or a walk longer than the index");
    p->a.swap(a); p->b.swap(b); p->score.swap(score); p->label.swap(label);
    p->summary.pairs = m;
    p->summary.components = (int64_t)sum[0];
    p->summary.groups = (int64_t)sum[1];
    p->summary.grouped_rows = (int64_t)sum[2];
    p->summary.largest = (int64_t)sum[3];
    p->state = 1;
    return GE_OK;
}

ge_status match_get(const ge_match *p, int64_t *n_indexed, int64_t *found, const int32_t **a, const int32_t **b, const float **score, const int32_t **label,
                    ge_match_summary *summary) {
    if (!p) return ge::fail(GE_ERR_ARG, "null ge_match handle");
    if (n_indexed) *n_indexed = p->n_indexed;
    if (found) *found = p->found;
    const bool have = p->state == 1;
    if (a) *a = have ? p->a.data() : nullptr;
    if (b) *b = have ? p->b.data() : nullptr;
    if (score) *score = have ? p->score.data() : nullptr;
    if (label) *label = have ? p->label.data() : nullptr;
    if (summary) *summary = p->summary;
    return GE_OK;
}

}  // namespace

extern "C" {

void ge_match_cfg_default(ge_match_cfg *cfg) {
    if (!cfg) return;
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->metric = GE_NN_COSINE;
}
int32_t ge_match_cfg_size(void) { return (int32_t)sizeof(ge_match_cfg); }
int32_t ge_match_summary_size(void) { return (int32_t)sizeof(ge_match_summary); }

ge_status ge_match_create(const float *rows, int64_t n_rows, int32_t dim, const int32_t *subset, int64_t n_subset, const ge_match_cfg *cfg, ge_match **out) {
    GE_GUARD(match_create_host(rows, n_rows, dim, subset, n_subset, cfg, out));
}
ge_status ge_glove_match_create(ge_glove *h, const int32_t *subset, int64_t n_subset, const ge_match_cfg *cfg, ge_match **out) {
    GE_GUARD(match_create_glove(h, subset, n_subset, cfg, out));
}
ge_status ge_match_run(ge_match *p, float threshold, int64_t max_pairs) { GE_GUARD(match_run(p, threshold, max_pairs)); }
ge_status ge_match_get(const ge_match *p, int64_t *n_indexed, int64_t *found, const int32_t **a, const int32_t **b, const float **score, const int32_t **label,
                       ge_match_summary *summary) {
    return match_get(p, n_indexed, found, a, b, score, label, summary);
}

ge_status ge_match_last_kernel_ms(const ge_match *p, float *prepare_ms, float *join_ms, float *sort_ms, float *components_ms) {
    if (!p) return ge::fail(GE_ERR_ARG, "null ge_match handle");
    if (prepare_ms) *prepare_ms = p->prepare_ms;
    if (join_ms) *join_ms = p->join_ms;
    if (sort_ms) *sort_ms = p->sort_ms;
    if (components_ms) *components_ms = p->components_ms;
    return GE_OK;
}

void ge_match_destroy(ge_match *p) { delete p; }

}  // extern "C"
