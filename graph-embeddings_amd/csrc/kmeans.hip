// kmeans.hip -- Lloyd's k-means over a table of vectors behind the C ABI: ge_kmeans_* (include/geglove.h, "Clustering").  The
// rows are prepared once on the device (k_km_prepare, as nn.hip's k_nn_prepare).  A step assigns every row to its best centroid
// on the fp32 matrix cores (k_km_assign: the score tile of nn.hip's k_nn_score_select with a running argmax for an epilogue),
// orders the rows by (label, position) with a stable radix sort, and sums every cluster's members in fp64 over a fixed
// partition (k_km_piece_sums, k_km_centroids): no floating-point atomics, so every byte that comes back is a function of the
// input alone.  The reference has no counterpart.
#include "ge_common.h"
#include "ge_glove_internal.h"
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int KM_MAX_DIM = 1024, KM_MAX_K = 65536;
constexpr int64_t KM_MAX_FLOATS = (int64_t)1 << 35;          // floats of input one handle accepts, as ge_nn_create
constexpr int64_t KM_SLAB_FLOATS = (int64_t)1 << 26;         // a 256 MB slab of rows per upload
constexpr int KM_PIECE = 1024;                               // members per piece of S_c, and positions per block of the objective

// (za, ca) comes before (zb, cb): the total order of ge_nn_* (fp32 compare, then the lower id)
__device__ __forceinline__ bool km_beats(float za, int32_t ca, float zb, int32_t cb) { return za > zb || (za == zb && ca < cb); }

// the (n+1)-th output of SplitMix64 seeded with `seed` (geglove.h: SM)
inline uint64_t splitmix_at(uint64_t seed, uint64_t n) {
    uint64_t z = seed + (n + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// ---------------------------------------------------------------------------------------------------------------------
// Prepare.  k_nn_prepare's walk: one wave takes 64 rows; pieces of 64 columns are read coalesced into LDS, lane r then walks
// row r of the piece in ascending d (the fp64 sum of squares is a sequential chain), and a second coalesced pass writes x / n
// rounded to fp32 once into the table, whose rows are padded with zeros to D4 = dim rounded up to 4 floats.  rowmap: NULL or
// the source row of every output row.  A non-finite value raises *flag (every writer stores the same 1).
// ---------------------------------------------------------------------------------------------------------------------
constexpr int PREP_ROWS = 64, PREP_COLS = 64, PREP_STRIDE = 65;

__global__ __launch_bounds__(64) void k_km_prepare(const float *__restrict__ src, const int32_t *__restrict__ rowmap, int64_t n_rows, int32_t D,
                                                   int32_t D4, int32_t metric, float *__restrict__ out, int32_t *__restrict__ flag) {
    __shared__ float tile[PREP_ROWS * PREP_STRIDE];
    __shared__ double norm[PREP_ROWS];
    const int lane = (int)threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * PREP_ROWS;
    const int rows = (int)(n_rows - row0 < PREP_ROWS ? n_rows - row0 : PREP_ROWS);
    bool bad = false;
    if (metric == GE_KM_COSINE) {
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
            if (metric == GE_KM_COSINE) {
                const double n = norm[r];
                x = n > 0.0 ? (float)((double)x / n) : 0.0f;
            }
            out[(row0 + r) * D4 + d] = x;
        }
    }
    if (bad) *flag = 1;
}

// r_p = the fp64 sum over ascending d of the unfused squares of a prepared row; one row per lane
__global__ __launch_bounds__(256) void k_km_row_squares(const float *__restrict__ X, int64_t n, int32_t D4, double *__restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const float *x = X + p * D4;
    double q = 0.0;
    for (int d = 0; d < D4; d += 4) {
        const f32x4 v = *reinterpret_cast<const f32x4 *>(x + d);
#pragma unroll
        for (int i = 0; i < 4; ++i) q = q + (double)v[i] * (double)v[i];
    }
    out[p] = q;
}

// the partition sums of the objective and of sum_sq: block b's values added in ascending p by one lane, from LDS
template <typename T>
__global__ __launch_bounds__(64) void k_km_block_sums(const T *__restrict__ v, int64_t n, double *__restrict__ sums) {
    __shared__ double s_t[KM_PIECE];
    const int64_t b0 = (int64_t)blockIdx.x * KM_PIECE;
    const int cnt = (int)((n - b0 < KM_PIECE) ? n - b0 : KM_PIECE);
    for (int q = threadIdx.x; q < cnt; q += 64) s_t[q] = (double)v[b0 + q];
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0;
        for (int q = 0; q < cnt; ++q) a = a + s_t[q];
        sums[blockIdx.x] = a;
    }
}

__global__ __launch_bounds__(256) void k_km_iota(int32_t *__restrict__ v, int64_t n) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p < n) v[p] = (int32_t)p;
}

// cen[t] = X[pos[t]]: the initial sample
__global__ __launch_bounds__(256) void k_km_take_rows(const float *__restrict__ X, const int32_t *__restrict__ pos, int64_t count, int32_t D4,
                                                      float *__restrict__ cen) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= count * D4) return;
    const int64_t t = idx / D4;
    cen[idx] = X[(int64_t)pos[t] * D4 + (idx - t * D4)];
}

// h_c of a centroid: 0 under cosine; (float)(-0.5 * sum_d cen[d]^2) under Euclid, the sum in fp64 over ascending d, unfused
__device__ __forceinline__ float km_bias_of(const float *cen, int32_t D4, int32_t metric) {
    if (metric == GE_KM_COSINE) return 0.0f;
    double q = 0.0;
    for (int d = 0; d < D4; ++d) q = q + (double)cen[d] * (double)cen[d];
    return (float)(-0.5 * q);
}

__global__ __launch_bounds__(256) void k_km_bias(const float *__restrict__ cen, int32_t K, int32_t D4, int32_t metric, float *__restrict__ h) {
    const int c = (int)(blockIdx.x * 256 + threadIdx.x);
    if (c < K) h[c] = km_bias_of(cen + (int64_t)c * D4, D4, metric);
}

// ---------------------------------------------------------------------------------------------------------------------
// Assign.  The score tile of k_nn_score_select: a workgroup owns 64 rows and walks ALL K centroids in tiles of 128; per 32
// columns the row and centroid panels are staged in LDS as [row][34] (34 = 2 mod 32: the 32 lanes one ds_read_b32 cycle serves
// hit 32 different banks), the next panel travelling in registers meanwhile, and wave w carries rows 16 w .. 16 w + 15 against
// the 128 centroids through v_mfma_f32_16x16x4_f32: eight accumulators, each bit for bit an fmaf chain over ascending d.  The
// centroid table is small and every workgroup re-reads it from the cache; the rows stream from memory once.
// Epilogue: every lane adds h_c to its 32 scores and keeps a running (z, c) for each of its four rows under the total order,
// across the whole walk; ids >= K of the last tile are never looked at.  At the end the sixteen lanes that share a row combine
// under the same order (the order is total, so the result does not depend on how they pair up), and one lane writes label and
// best.  A label that differs from the one found there counts as changed: one integer atomic per workgroup.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int KA_TQ = 64, KA_TC = 128, KA_DK = 32, KA_LS = 34;
constexpr int KA_LOADS = (KA_TQ + KA_TC) * (KA_DK / 4) / 256;   // 16-byte pieces a thread moves per panel: 2 of rows, 4 of centroids

__global__ __launch_bounds__(256, 3) void k_km_assign(const float *__restrict__ X, int64_t n, const float *__restrict__ cen, const float *__restrict__ h,
                                                      int32_t K, int32_t D4, int32_t *__restrict__ label, float *__restrict__ best,
                                                      unsigned long long *__restrict__ changed) {
    __shared__ float sq[KA_TQ * KA_LS];
    __shared__ float sx[KA_TC * KA_LS];
    __shared__ int32_t s_changed[4];

    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t q0 = (int64_t)blockIdx.x * KA_TQ;

    // what this thread stages: piece i of a panel is row (tid + 256 i) >> 3, columns 4 ((tid + 256 i) & 7) ..
    const int c4 = (tid & 7) * 4, prow = tid >> 3;
    const float *qsrc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int64_t qg = q0 + prow + 32 * i;
        qsrc[i] = qg < n ? X + qg * D4 : nullptr;
    }
    f32x4 pre[KA_LOADS];
    auto fetch = [&](int ct, int d0) {
        const bool in = d0 + c4 < D4;
#pragma unroll
        for (int i = 0; i < 2; ++i)
            pre[i] = in && qsrc[i] ? *reinterpret_cast<const f32x4 *>(qsrc[i] + d0 + c4) : f32x4{0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = ct + prow + 32 * i;
            pre[2 + i] = in && c < K ? *reinterpret_cast<const f32x4 *>(cen + (int64_t)c * D4 + d0 + c4) : f32x4{0, 0, 0, 0};
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int i = 0; i < KA_LOADS; ++i) {
            float *dst = (i < 2 ? sq + (prow + 32 * i) * KA_LS : sx + (prow + 32 * (i - 2)) * KA_LS) + c4;   // 8-byte aligned: KA_LS and c4 are even
            *reinterpret_cast<float2 *>(dst) = float2{pre[i][0], pre[i][1]};
            *reinterpret_cast<float2 *>(dst + 2) = float2{pre[i][2], pre[i][3]};
        }
    };

    // the four rows whose scores a lane holds: local rows 4 (lane >> 4) + reg of the wave's sixteen
    const int qb = wave * 16;
    const int ql = qb + 4 * (lane >> 4);
    float bz[4];
    int32_t bc[4];
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) { bz[reg] = -INFINITY; bc[reg] = INT_MAX; }
    const int xa = (qb + (lane & 15)) * KA_LS + (lane >> 4);
    const int xb = (lane & 15) * KA_LS + (lane >> 4);

    fetch(0, 0);
    for (int ct = 0; ct < K; ct += KA_TC) {
        f32x4 acc[KA_TC / 16];
#pragma unroll
        for (int t = 0; t < KA_TC / 16; ++t) acc[t] = f32x4{0, 0, 0, 0};
        for (int d0 = 0; d0 < D4; d0 += KA_DK) {
            __syncthreads();
            stage();
            __syncthreads();
            if (d0 + KA_DK < D4) fetch(ct, d0 + KA_DK);
            else if (ct + KA_TC < K) fetch(ct + KA_TC, 0);
            auto step = [&](int dd) {
                const float a = sq[xa + dd];
                float b[KA_TC / 16];
#pragma unroll
                for (int t = 0; t < KA_TC / 16; ++t) b[t] = sx[xb + t * 16 * KA_LS + dd];
#pragma unroll
                for (int t = 0; t < KA_TC / 16; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b[t], acc[t], 0, 0, 0);
            };
            if (D4 - d0 >= KA_DK) {                                   // a whole panel: unrolled, so the reads of a step run ahead of its products
#pragma unroll
                for (int dd = 0; dd < KA_DK; dd += 4) step(dd);
            } else {
#pragma unroll 1
                for (int dd = 0; dd < D4 - d0; dd += 4) step(dd);
            }
        }
        // C/D of the f32 form: column (centroid) = lane & 15, row = 4 * (lane >> 4) + register
#pragma unroll
        for (int t = 0; t < KA_TC / 16; ++t) {
            const int c = ct + t * 16 + (lane & 15);
            const bool in = c < K;
            const float bias = in ? h[c] : 0.0f;
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                float z = acc[t][reg] + bias;
                z = z == z ? z : -INFINITY;
                if (in && km_beats(z, c, bz[reg], bc[reg])) { bz[reg] = z; bc[reg] = c; }
            }
        }
    }
    // the sixteen lanes lane & 15 = 0 .. 15 of a quarter hold candidates of the same four rows
    int diff = 0;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        float z = bz[reg];
        int32_t c = bc[reg];
#pragma unroll
        for (int m = 1; m < 16; m <<= 1) {
            const float oz = __shfl_xor(z, m, 64);
            const int32_t oc = __shfl_xor(c, m, 64);
            if (km_beats(oz, oc, z, c)) { z = oz; c = oc; }
        }
        const int64_t p = q0 + ql + reg;
        if ((lane & 15) == 0 && p < n) {
            diff += label[p] != c ? 1 : 0;
            label[p] = c;
            best[p] = z;
        }
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) diff += __shfl_xor(diff, m, 64);
    if (lane == 0) s_changed[wave] = diff;
    __syncthreads();
    if (tid == 0) {
        const int total = s_changed[0] + s_changed[1] + s_changed[2] + s_changed[3];
        if (total) atomicAdd(changed, (unsigned long long)total);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Update.  `keys` are the labels in ascending order and `pos` the positions beside them (a stable sort: ascending p inside a
// label).  k_km_bounds finds where every cluster begins (a binary search per cluster: no atomics), its size and its number of
// pieces; an exclusive scan numbers the pieces; k_km_piece_sums adds one piece's members in ascending order, one dimension per
// lane; k_km_centroids adds a cluster's pieces in ascending order, divides or normalises, and computes h_c.
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int64_t km_lower_bound(const uint32_t *keys, int64_t n, uint32_t c) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (keys[mid] < c) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// thread c <= K: start[c]; c < K: sizes[c], pieces[c]; pieces[K] = 0 (so the scan's last entry is the total)
__global__ __launch_bounds__(256) void k_km_bounds(const uint32_t *__restrict__ keys, int64_t n, int32_t K, int32_t *__restrict__ start,
                                                   int32_t *__restrict__ sizes, uint32_t *__restrict__ pieces) {
    const int c = (int)(blockIdx.x * 256 + threadIdx.x);
    if (c > K) return;
    const int64_t s0 = c < K ? km_lower_bound(keys, n, (uint32_t)c) : n;
    start[c] = (int32_t)s0;
    if (c == K) { pieces[c] = 0; return; }
    const int64_t s1 = c + 1 < K ? km_lower_bound(keys, n, (uint32_t)(c + 1)) : n;
    sizes[c] = (int32_t)(s1 - s0);
    pieces[c] = (uint32_t)((s1 - s0 + KM_PIECE - 1) / KM_PIECE);
}

// blockIdx.x = piece (those past the total leave), blockIdx.y = a group of 64 dimensions; first[c] = the number of c's first piece
__global__ __launch_bounds__(64) void k_km_piece_sums(const float *__restrict__ X, const int32_t *__restrict__ pos, const int32_t *__restrict__ start,
                                                      const uint32_t *__restrict__ first, int32_t K, int32_t D4, double *__restrict__ psum) {
    const uint32_t piece = blockIdx.x;
    if (piece >= first[K]) return;
    int lo = 0, hi = K;                                   // the last c with first[c] <= piece: the cluster the piece belongs to
    while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;
        if (first[mid] <= piece) lo = mid; else hi = mid - 1;
    }
    const int c = lo;
    const int d = (int)(blockIdx.y * 64 + threadIdx.x);
    if (d >= D4) return;
    const int64_t m0 = (int64_t)start[c] + (int64_t)(piece - first[c]) * KM_PIECE;
    const int64_t m1 = m0 + KM_PIECE < (int64_t)start[c + 1] ? m0 + KM_PIECE : (int64_t)start[c + 1];
    double s = 0.0;
    int64_t m = m0;
    for (; m + 8 <= m1; m += 8) {                         // the reads go out together, the sum follows in order
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = X[(int64_t)pos[m + u] * D4 + d];
#pragma unroll
        for (int u = 0; u < 8; ++u) s = s + (double)v[u];
    }
    for (; m < m1; ++m) s = s + (double)X[(int64_t)pos[m] * D4 + d];
    psum[(int64_t)piece * D4 + d] = s;
}

__global__ __launch_bounds__(256) void k_km_centroids(const double *__restrict__ psum, const int32_t *__restrict__ sizes, const uint32_t *__restrict__ first,
                                                      int32_t D4, int32_t metric, float *__restrict__ cen, float *__restrict__ h) {
    __shared__ double s_sum[KM_MAX_DIM];
    __shared__ float s_cen[KM_MAX_DIM];
    const int c = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int32_t n_c = sizes[c];
    if (n_c == 0) return;                                 // the whole workgroup: the centroid stays
    const uint32_t p0 = first[c], p1 = first[c + 1];
    for (int d = tid; d < D4; d += 256) {
        double s = 0.0;
        for (uint32_t q = p0; q < p1; ++q) s = s + psum[(int64_t)q * D4 + d];
        s_sum[d] = s;
    }
    __syncthreads();
    double div = (double)n_c;
    if (metric == GE_KM_COSINE) {                         // every lane walks the same chain: no second barrier, the same m everywhere
        double m2 = 0.0;
        for (int d = 0; d < D4; ++d) m2 = m2 + s_sum[d] * s_sum[d];
        div = sqrt(m2);
        if (div == 0.0) return;                           // the members cancel: the centroid stays
    }
    float *out = cen + (int64_t)c * D4;
    for (int d = tid; d < D4; d += 256) {
        const float v = (float)(s_sum[d] / div);
        out[d] = v;
        s_cen[d] = v;
    }
    __syncthreads();
    if (tid == 0) h[c] = km_bias_of(s_cen, D4, metric);
}

struct DeviceBuffers {                      // freed on every way out
    std::vector<void *> ptrs;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~DeviceBuffers() { for (void *q : ptrs) (void)hipFree(q); if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
    ge_status alloc(void **q, size_t bytes) { GE_HIP(hipMalloc(q, std::max<size_t>(bytes, 16))); ptrs.push_back(*q); return GE_OK; }
    ge_status events() { GE_HIP(hipEventCreate(&e0)); GE_HIP(hipEventCreate(&e1)); return GE_OK; }
};

}  // namespace

struct ge_kmeans {
    int32_t metric = 0, device = 0, dim = 0, d4 = 0, k = 0;
    int64_t n = 0, max_pieces = 0;
    uint64_t seed = 0;
    hipStream_t stream = nullptr;
    DeviceBuffers B;                         // everything below lives here
    float *dx = nullptr, *dcen = nullptr, *dh = nullptr, *dbest = nullptr;
    int32_t *dlabel = nullptr, *diota = nullptr, *dpos = nullptr, *dstart = nullptr, *dsizes = nullptr;
    uint32_t *dkeys = nullptr, *dpieces = nullptr, *dfirst = nullptr;
    double *dblock = nullptr, *dpsum = nullptr;
    unsigned long long *dchanged = nullptr;
    void *dtmp = nullptr;
    size_t sort_bytes = 0, scan_bytes = 0;
    int sort_bits = 1;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    std::vector<double> block;               // the objective's block sums on the host
    int32_t steps = 0, converged = 0;
    double objective = 0.0, sum_sq = 0.0;
    float prepare_ms = 0, assign_ms = 0, update_ms = 0;
    ~ge_kmeans() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
};

namespace {

ge_status check_create(int64_t n_rows, int32_t dim, const int32_t *subset, int64_t n_subset, const ge_kmeans_cfg *cfg) {
    if (!cfg) return ge::fail(GE_ERR_ARG, "ge_kmeans_cfg is null");
    if (cfg->metric != GE_KM_COSINE && cfg->metric != GE_KM_EUCLID) return ge::fail(GE_ERR_ARG, "kmeans: unknown metric %d", cfg->metric);
    if (dim < 1 || dim > KM_MAX_DIM) return ge::fail(GE_ERR_ARG, "kmeans: dim %d outside [1, %d]", dim, KM_MAX_DIM);
    if (cfg->k < 1 || cfg->k > KM_MAX_K) return ge::fail(GE_ERR_ARG, "kmeans: k %d outside [1, %d]", cfg->k, KM_MAX_K);
    if (n_rows < 1 || n_rows >= INT_MAX) return ge::fail(GE_ERR_ARG, "kmeans: %lld rows outside [1, 2^31 - 2]", (long long)n_rows);
    if (n_rows > KM_MAX_FLOATS / dim)
        return ge::fail(GE_ERR_ARG, "kmeans: %lld rows of %d floats are more than one handle holds (%lld floats)", (long long)n_rows, dim,
                        (long long)KM_MAX_FLOATS);
    if (subset) {
        if (n_subset < 1 || n_subset > n_rows) return ge::fail(GE_ERR_ARG, "kmeans: a subset of %lld of %lld rows", (long long)n_subset, (long long)n_rows);
        for (int64_t i = 0; i < n_subset; ++i) {
            if (subset[i] < 0 || subset[i] >= n_rows)
                return ge::fail(GE_ERR_ARG, "kmeans: subset[%lld] = %d outside [0, %lld)", (long long)i, subset[i], (long long)n_rows);
            if (i > 0 && subset[i] <= subset[i - 1]) return ge::fail(GE_ERR_ARG, "kmeans: the subset is not strictly ascending at [%lld]", (long long)i);
        }
    }
    const int64_t n = subset ? n_subset : n_rows;
    if (cfg->k > n) return ge::fail(GE_ERR_ARG, "kmeans: k %d exceeds the %lld indexed rows", cfg->k, (long long)n);
    return GE_OK;
}

// rows (host: slab by slab; dev: in place) -> table[rows_out][d4], prepared; *ms_out += the kernel's time
ge_status prepare_rows(const float *host, const float *dev, const int32_t *host_map, const int32_t *dev_map, int64_t rows_out, int32_t dim,
                       int32_t metric, float *table, hipStream_t stream, const char *what, float *ms_out) {
    const int D = dim, D4 = (D + 3) / 4 * 4;
    const int64_t slab_rows = std::min<int64_t>(std::max<int64_t>(PREP_ROWS, KM_SLAB_FLOATS / D / PREP_ROWS * PREP_ROWS), rows_out);
    DeviceBuffers B;
    float *dslab = nullptr;
    int32_t *dflag = nullptr;
    GE_CHECK(B.events());
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
        GE_HIP(hipEventRecord(B.e0, stream));
        hipLaunchKernelGGL(k_km_prepare, dim3((unsigned)((rows + PREP_ROWS - 1) / PREP_ROWS)), dim3(64), 0, stream, x, map, rows, D, D4, metric,
                           table + begin * D4, dflag);
        GE_HIP(hipGetLastError());
        GE_HIP(hipEventRecord(B.e1, stream));
        GE_HIP(hipStreamSynchronize(stream));                                       // the slab buffer (and `packed`) are free again
        float ms = 0;
        GE_HIP(hipEventElapsedTime(&ms, B.e0, B.e1));
        total += ms;
    }
    int32_t flag = 0;
    GE_HIP(hipMemcpyAsync(&flag, dflag, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    GE_HIP(hipStreamSynchronize(stream));
    if (flag) return ge::fail(GE_ERR_ARG, "kmeans: non-finite input (%s)", what);
    *ms_out += total;
    return GE_OK;
}

// the partition sum of v[0 .. n): block sums on the device, their sum in ascending b on the host
template <typename T>
ge_status partition_sum(ge_kmeans *p, const T *v, double *out) {
    const int64_t blocks = (p->n + KM_PIECE - 1) / KM_PIECE;
    hipLaunchKernelGGL(k_km_block_sums<T>, dim3((unsigned)blocks), dim3(64), 0, p->stream, v, p->n, p->dblock);
    GE_HIP(hipGetLastError());
    GE_HIP(hipMemcpyAsync(p->block.data(), p->dblock, sizeof(double) * (size_t)blocks, hipMemcpyDeviceToHost, p->stream));
    GE_HIP(hipStreamSynchronize(p->stream));
    double a = 0.0;
    for (int64_t b = 0; b < blocks; ++b) a = a + p->block[(size_t)b];
    *out = a;
    return GE_OK;
}

ge_status restart(ge_kmeans *p) {           // new centroids are in place: their h, and no previous assign
    hipLaunchKernelGGL(k_km_bias, dim3((unsigned)((p->k + 255) / 256)), dim3(256), 0, p->stream, (const float *)p->dcen, p->k, p->d4, p->metric, p->dh);
    GE_HIP(hipGetLastError());
    GE_HIP(hipMemsetAsync(p->dlabel, 0xFF, sizeof(int32_t) * (size_t)p->n, p->stream));     // label -1 everywhere: the next assign changes n labels
    GE_HIP(hipStreamSynchronize(p->stream));
    p->steps = 0; p->converged = 0; p->objective = 0.0;
    return GE_OK;
}

ge_status create_impl(const float *host, const float *dev, int64_t n_rows, int32_t dim, const int32_t *subset, int64_t n_subset, const ge_kmeans_cfg *cfg,
                      ge_kmeans **out) {
    std::unique_ptr<ge_kmeans> p(new ge_kmeans);
    p->metric = cfg->metric; p->device = cfg->device; p->stream = (hipStream_t)cfg->stream; p->k = cfg->k; p->seed = cfg->seed;
    p->dim = dim; p->d4 = (dim + 3) / 4 * 4; p->n = subset ? n_subset : n_rows;
    const size_t N = (size_t)p->n, K = (size_t)p->k, D4 = (size_t)p->d4;
    p->max_pieces = std::min<int64_t>(p->n, p->n / KM_PIECE + p->k);           // every piece has a member, and a cluster at most one short piece
    const size_t blocks = (N + KM_PIECE - 1) / KM_PIECE;
    p->block.resize(blocks);
    DeviceBuffers &B = p->B;
    int32_t *dids = nullptr;
    GE_CHECK(B.alloc((void **)&p->dx, sizeof(float) * N * D4));
    GE_CHECK(B.alloc((void **)&p->dcen, sizeof(float) * K * D4));
    GE_CHECK(B.alloc((void **)&p->dh, sizeof(float) * K));
    GE_CHECK(B.alloc((void **)&p->dbest, sizeof(float) * N));
    GE_CHECK(B.alloc((void **)&p->dlabel, sizeof(int32_t) * N));
    GE_CHECK(B.alloc((void **)&p->diota, sizeof(int32_t) * N));
    GE_CHECK(B.alloc((void **)&p->dpos, sizeof(int32_t) * N));
    GE_CHECK(B.alloc((void **)&p->dkeys, sizeof(uint32_t) * N));
    GE_CHECK(B.alloc((void **)&p->dstart, sizeof(int32_t) * (K + 1)));
    GE_CHECK(B.alloc((void **)&p->dsizes, sizeof(int32_t) * K));
    GE_CHECK(B.alloc((void **)&p->dpieces, sizeof(uint32_t) * (K + 1)));
    GE_CHECK(B.alloc((void **)&p->dfirst, sizeof(uint32_t) * (K + 1)));
    GE_CHECK(B.alloc((void **)&p->dblock, sizeof(double) * blocks));
    GE_CHECK(B.alloc((void **)&p->dpsum, sizeof(double) * (size_t)p->max_pieces * D4));
    GE_CHECK(B.alloc((void **)&p->dchanged, sizeof(unsigned long long)));
    while ((1 << p->sort_bits) < p->k) ++p->sort_bits;                           // labels are below k
    GE_HIP(rocprim::radix_sort_pairs(nullptr, p->sort_bytes, (const uint32_t *)p->dlabel, p->dkeys, (const int32_t *)p->diota, p->dpos, N, 0,
                                     (unsigned)p->sort_bits, p->stream));
    GE_HIP(rocprim::exclusive_scan(nullptr, p->scan_bytes, (const uint32_t *)p->dpieces, p->dfirst, 0u, K + 1, rocprim::plus<uint32_t>(), p->stream));
    GE_CHECK(B.alloc(&p->dtmp, std::max(p->sort_bytes, p->scan_bytes)));
    for (hipEvent_t &e : p->ev) GE_HIP(hipEventCreate(&e));
    if (subset && dev) {
        GE_CHECK(B.alloc((void **)&dids, sizeof(int32_t) * N));
        GE_HIP(hipMemcpyAsync(dids, subset, sizeof(int32_t) * N, hipMemcpyHostToDevice, p->stream));
    }
    GE_CHECK(prepare_rows(host, dev, subset, dids, p->n, dim, p->metric, p->dx, p->stream, "rows", &p->prepare_ms));

    hipLaunchKernelGGL(k_km_iota, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, p->stream, p->diota, p->n);
    GE_HIP(hipGetLastError());
    // sum_sq: the row squares in a buffer of their own, gone after creation
    {
        DeviceBuffers T;
        double *dsq = nullptr;
        GE_CHECK(T.alloc((void **)&dsq, sizeof(double) * N));
        hipLaunchKernelGGL(k_km_row_squares, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, p->stream, (const float *)p->dx, p->n, p->d4, dsq);
        GE_HIP(hipGetLastError());
        GE_CHECK(partition_sum<double>(p.get(), dsq, &p->sum_sq));
    }
    // the keyed sample: the k positions with the smallest (SM(seed ^ key, p), p), in that order
    std::vector<int32_t> pick((size_t)p->k);
    {
        const uint64_t s = p->seed ^ (uint64_t)GE_KM_INIT_KEY;
        std::vector<std::pair<uint64_t, int32_t>> key(N);
        for (int64_t i = 0; i < p->n; ++i) key[(size_t)i] = {splitmix_at(s, (uint64_t)i), (int32_t)i};
        std::partial_sort(key.begin(), key.begin() + p->k, key.end());
        for (int t = 0; t < p->k; ++t) pick[(size_t)t] = key[(size_t)t].second;
    }
    GE_HIP(hipMemcpyAsync(p->dpos, pick.data(), sizeof(int32_t) * K, hipMemcpyHostToDevice, p->stream));       // dpos is free until the first update
    hipLaunchKernelGGL(k_km_take_rows, dim3((unsigned)((K * D4 + 255) / 256)), dim3(256), 0, p->stream, (const float *)p->dx, (const int32_t *)p->dpos,
                       (int64_t)p->k, p->d4, p->dcen);
    GE_HIP(hipGetLastError());
    GE_CHECK(restart(p.get()));              // drains the stream: `pick` may go
    *out = p.release();
    return GE_OK;
}

ge_status km_create_host(const float *rows, int64_t n_rows, int32_t dim, const int32_t *subset, int64_t n_subset, const ge_kmeans_cfg *cfg,
                         ge_kmeans **out) {
    if (out) *out = nullptr;
    if (!rows || !out) return ge::fail(GE_ERR_ARG, "ge_kmeans_create: rows or out is null");
    GE_CHECK(check_create(n_rows, dim, subset, n_subset, cfg));
    GE_CHECK(ge::select_device(cfg->device));
    return create_impl(rows, nullptr, n_rows, dim, subset, n_subset, cfg, out);
}

ge_status km_create_glove(ge_glove *h, const int32_t *subset, int64_t n_subset, const ge_kmeans_cfg *cfg, ge_kmeans **out) {
    if (out) *out = nullptr;
    if (!h || !out) return ge::fail(GE_ERR_ARG, "ge_glove_kmeans_create: handle or out is null");
    if (!cfg) return ge::fail(GE_ERR_ARG, "ge_kmeans_cfg is null");
    if (cfg->metric != GE_KM_COSINE && cfg->metric != GE_KM_EUCLID) return ge::fail(GE_ERR_ARG, "kmeans: unknown metric %d", cfg->metric);
    if (cfg->k < 1 || cfg->k > KM_MAX_K) return ge::fail(GE_ERR_ARG, "kmeans: k %d outside [1, %d]", cfg->k, KM_MAX_K);
    float *d = nullptr;
    int32_t V = 0, D = 0, device = 0;
    GE_CHECK(ge::glove_extract_device_f32(h, &d, &V, &D, &device));   // a fresh buffer: no trainer table is written
    ge_kmeans_cfg own = *cfg;
    own.device = device;                                              // the rows live on the handle's device
    ge_status st = check_create(V, D, subset, n_subset, &own);
    if (st == GE_OK) st = create_impl(nullptr, d, V, D, subset, n_subset, &own, out);
    (void)hipFree(d);
    return st;
}

ge_status km_set_centroids(ge_kmeans *p, const float *centroids) {
    if (!p) return ge::fail(GE_ERR_ARG, "null ge_kmeans handle");
    if (!centroids) return ge::fail(GE_ERR_ARG, "ge_kmeans_set_centroids: centroids is null");
    GE_CHECK(ge::select_device(p->device));
    float ms = 0;
    // into a buffer of their own first: a refused table leaves the handle as it was
    DeviceBuffers T;
    float *dnew = nullptr;
    GE_CHECK(T.alloc((void **)&dnew, sizeof(float) * (size_t)p->k * p->d4));
    GE_CHECK(prepare_rows(centroids, nullptr, nullptr, nullptr, p->k, p->dim, p->metric, dnew, p->stream, "centroids", &ms));
    GE_HIP(hipMemcpyAsync(p->dcen, dnew, sizeof(float) * (size_t)p->k * p->d4, hipMemcpyDeviceToDevice, p->stream));
    return restart(p);
}

ge_status km_step(ge_kmeans *p, int64_t *changed_out, double *objective_out) {
    if (!p) return ge::fail(GE_ERR_ARG, "null ge_kmeans handle");
    GE_CHECK(ge::select_device(p->device));
    hipStream_t stream = p->stream;
    const int64_t n = p->n;
    const int32_t K = p->k, D4 = p->d4;
    GE_HIP(hipMemsetAsync(p->dchanged, 0, sizeof(unsigned long long), stream));

    GE_HIP(hipEventRecord(p->ev[0], stream));
    hipLaunchKernelGGL(k_km_assign, dim3((unsigned)((n + KA_TQ - 1) / KA_TQ)), dim3(256), 0, stream, (const float *)p->dx, n, (const float *)p->dcen,
                       (const float *)p->dh, K, D4, p->dlabel, p->dbest, p->dchanged);
    GE_HIP(hipGetLastError());
    const int64_t blocks = (n + KM_PIECE - 1) / KM_PIECE;
    hipLaunchKernelGGL(k_km_block_sums<float>, dim3((unsigned)blocks), dim3(64), 0, stream, (const float *)p->dbest, n, p->dblock);
    GE_HIP(hipGetLastError());

    GE_HIP(hipEventRecord(p->ev[1], stream));
    GE_HIP(rocprim::radix_sort_pairs(p->dtmp, p->sort_bytes, (const uint32_t *)p->dlabel, p->dkeys, (const int32_t *)p->diota, p->dpos, (size_t)n, 0,
                                     (unsigned)p->sort_bits, stream));
    hipLaunchKernelGGL(k_km_bounds, dim3((unsigned)((K + 1 + 255) / 256)), dim3(256), 0, stream, (const uint32_t *)p->dkeys, n, K, p->dstart, p->dsizes,
                       p->dpieces);
    GE_HIP(hipGetLastError());
    GE_HIP(rocprim::exclusive_scan(p->dtmp, p->scan_bytes, (const uint32_t *)p->dpieces, p->dfirst, 0u, (size_t)K + 1, rocprim::plus<uint32_t>(), stream));
    hipLaunchKernelGGL(k_km_piece_sums, dim3((unsigned)p->max_pieces, (unsigned)((D4 + 63) / 64)), dim3(64), 0, stream, (const float *)p->dx,
                       (const int32_t *)p->dpos, (const int32_t *)p->dstart, (const uint32_t *)p->dfirst, K, D4, p->dpsum);
    GE_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_km_centroids, dim3((unsigned)K), dim3(256), 0, stream, (const double *)p->dpsum, (const int32_t *)p->dsizes,
                       (const uint32_t *)p->dfirst, D4, p->metric, p->dcen, p->dh);
    GE_HIP(hipGetLastError());
    GE_HIP(hipEventRecord(p->ev[2], stream));

    unsigned long long changed = 0;
    GE_HIP(hipMemcpyAsync(&changed, p->dchanged, sizeof(changed), hipMemcpyDeviceToHost, stream));
    GE_HIP(hipMemcpyAsync(p->block.data(), p->dblock, sizeof(double) * (size_t)blocks, hipMemcpyDeviceToHost, stream));
    GE_HIP(hipStreamSynchronize(stream));
    GE_HIP(hipEventElapsedTime(&p->assign_ms, p->ev[0], p->ev[1]));
    GE_HIP(hipEventElapsedTime(&p->update_ms, p->ev[1], p->ev[2]));
    double a = 0.0;
    for (int64_t b = 0; b < blocks; ++b) a = a + p->block[(size_t)b];
    p->objective = a;
    p->steps += 1;
    p->converged = changed == 0 ? 1 : 0;
    if (changed_out) *changed_out = (int64_t)changed;
    if (objective_out) *objective_out = a;
    return GE_OK;
}

ge_status km_run(ge_kmeans *p, int32_t max_iter, int32_t *steps_run, int32_t *converged) {
    if (max_iter < 1) return ge::fail(GE_ERR_ARG, "kmeans: max_iter %d is below 1", max_iter);
    if (!p) return ge::fail(GE_ERR_ARG, "null ge_kmeans handle");
    int32_t ran = 0;
    int64_t changed = 1;
    while (ran < max_iter && changed != 0) {
        GE_CHECK(km_step(p, &changed, nullptr));
        ++ran;
    }
    if (steps_run) *steps_run = ran;
    if (converged) *converged = changed == 0 ? 1 : 0;
    return GE_OK;
}

ge_status km_get(const ge_kmeans *p, int64_t *n, int32_t *dim, int32_t *k, int32_t *labels, float *best, float *centroids, int32_t *sizes,
                 int32_t *steps, int32_t *converged, double *objective, double *sum_sq) {
    if (!p) return ge::fail(GE_ERR_ARG, "null ge_kmeans handle");
    if (n) *n = p->n;
    if (dim) *dim = p->dim;
    if (k) *k = p->k;
    if (steps) *steps = p->steps;
    if (converged) *converged = p->converged;
    if (objective) *objective = p->objective;
    if (sum_sq) *sum_sq = p->sum_sq;
    if (!labels && !best && !centroids && !sizes) return GE_OK;
    if ((labels || best || sizes) && p->steps == 0) return ge::fail(GE_ERR_STATE, "kmeans: no step has run, there are no labels yet");
    GE_CHECK(ge::select_device(p->device));
    hipStream_t stream = p->stream;
    if (labels) GE_HIP(hipMemcpyAsync(labels, p->dlabel, sizeof(int32_t) * (size_t)p->n, hipMemcpyDeviceToHost, stream));
    if (best) GE_HIP(hipMemcpyAsync(best, p->dbest, sizeof(float) * (size_t)p->n, hipMemcpyDeviceToHost, stream));
    if (sizes) GE_HIP(hipMemcpyAsync(sizes, p->dsizes, sizeof(int32_t) * (size_t)p->k, hipMemcpyDeviceToHost, stream));
    if (centroids)
        GE_HIP(hipMemcpy2DAsync(centroids, sizeof(float) * (size_t)p->dim, p->dcen, sizeof(float) * (size_t)p->d4, sizeof(float) * (size_t)p->dim,
                                (size_t)p->k, hipMemcpyDeviceToHost, stream));
    GE_HIP(hipStreamSynchronize(stream));
    return GE_OK;
}

}  // namespace

extern "C" {

void ge_kmeans_cfg_default(ge_kmeans_cfg *cfg) {
    if (!cfg) return;
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->metric = GE_KM_COSINE;
}
int32_t ge_kmeans_cfg_size(void) { return (int32_t)sizeof(ge_kmeans_cfg); }

ge_status ge_kmeans_create(const float *rows, int64_t n_rows, int32_t dim, const int32_t *subset, int64_t n_subset, const ge_kmeans_cfg *cfg,
                           ge_kmeans **out) {
    GE_GUARD(km_create_host(rows, n_rows, dim, subset, n_subset, cfg, out));
}
ge_status ge_glove_kmeans_create(ge_glove *h, const int32_t *subset, int64_t n_subset, const ge_kmeans_cfg *cfg, ge_kmeans **out) {
    GE_GUARD(km_create_glove(h, subset, n_subset, cfg, out));
}
ge_status ge_kmeans_set_centroids(ge_kmeans *p, const float *centroids) { GE_GUARD(km_set_centroids(p, centroids)); }
ge_status ge_kmeans_step(ge_kmeans *p, int64_t *changed, double *objective) { GE_GUARD(km_step(p, changed, objective)); }
ge_status ge_kmeans_run(ge_kmeans *p, int32_t max_iter, int32_t *steps_run, int32_t *converged) { GE_GUARD(km_run(p, max_iter, steps_run, converged)); }
ge_status ge_kmeans_get(const ge_kmeans *p, int64_t *n, int32_t *dim, int32_t *k, int32_t *labels, float *best, float *centroids, int32_t *sizes,
                        int32_t *steps, int32_t *converged, double *objective, double *sum_sq) {
    GE_GUARD(km_get(p, n, dim, k, labels, best, centroids, sizes, steps, converged, objective, sum_sq));
}

ge_status ge_kmeans_last_kernel_ms(const ge_kmeans *p, float *assign_ms, float *update_ms) {
    if (!p) return ge::fail(GE_ERR_ARG, "null ge_kmeans handle");
    if (assign_ms) *assign_ms = p->assign_ms;
    if (update_ms) *update_ms = p->update_ms;
    return GE_OK;
}

void ge_kmeans_destroy(ge_kmeans *p) {
    if (!p) return;
    (void)hipSetDevice(p->device);
    delete p;
}

}  // extern "C"
