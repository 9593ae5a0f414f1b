// nn.hip -- exact top-k nearest neighbours over a table of vectors behind the C ABI: the table is prepared once on the device
// (k_nn_prepare: fp64 norms, rows normalised and rounded to fp32 once), scores are fp32 dot products on the fp32 matrix cores
// with the selection in the same kernel (k_nn_score_select), and the partial lists of the candidate ranges are merged in a
// fixed order (k_nn_merge).  The reference has no counterpart; the semantics are written down in include/geglove.h.
#include "ge_common.h"
#include "ge_glove_internal.h"
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int NN_MAX_DIM = 1024, NN_MAX_K = 128;
constexpr int64_t NN_MAX_FLOATS = (int64_t)1 << 35;          // floats of input one index accepts (128 GiB as fp32)
constexpr int64_t NN_SLAB_FLOATS = (int64_t)1 << 26;         // a 256 MB slab of rows per upload
constexpr int64_t NN_BATCH_ENTRIES = (int64_t)1 << 24;       // (query, range, slot) entries of partial lists per launch (128 MB of them)

// the order of the results: score descending as fp32 compares them, then position ascending, then (for the fill entries of
// short lists, which share one position) slot ascending -- a strict total order, so ranks are a permutation
__device__ __forceinline__ bool nn_beats(float sa, int32_t pa, int ea, float sb, int32_t pb, int eb) {
    return sa > sb || (sa == sb && (pa < pb || (pa == pb && ea < eb)));
}
__device__ __forceinline__ bool nn_beats(float sa, int32_t pa, float sb, int32_t pb) { return sa > sb || (sa == sb && pa < pb); }

// ---------------------------------------------------------------------------------------------------------------------
// Prepare.  One wave takes 64 rows: pieces of 64 columns are read coalesced into LDS, lane r then walks row r of the piece in
// ascending d (the fp64 sum of squares is a sequential chain, as the header states it), and a second coalesced pass writes
// x / n rounded to fp32 once into the index table, whose rows are padded with zeros to D4 = dim rounded up to 4 floats (so the
// score kernel reads aligned 16-byte pieces and needs no column test).  rowmap: NULL or the source row of every output row.
// A non-finite value raises *flag (every writer stores the same 1).
// ---------------------------------------------------------------------------------------------------------------------
constexpr int PREP_ROWS = 64, PREP_COLS = 64, PREP_STRIDE = 65;

__global__ __launch_bounds__(64) void k_nn_prepare(const float *__restrict__ src, const int32_t *__restrict__ rowmap, int64_t n_rows, int32_t D,
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
// Score and select.  A workgroup owns a tile of NN_TQ queries (blockIdx.x, the fast index: workgroups that read the same
// candidate panels run together) and one fixed range of candidates (blockIdx.y).  It walks the range in tiles of NN_TC
// candidates; per NN_DK columns the query and candidate panels are staged in LDS (the next panel travels in registers
// meanwhile), and wave w carries queries 16 w .. 16 w + 15 against all NN_TC candidates through v_mfma_f32_16x16x4_f32: eight
// independent accumulators, each bit for bit an fmaf chain over ascending d.
//
// LDS panels are [row][NN_LS floats], NN_LS = 34 = 2 mod 32: the 32 lanes one ds_read_b32 cycle serves read rows r .. r + 15 at
// columns c, c + 1, i.e. banks 2 r + c -- 32 different ones.
//
// Selection: every query of the tile has a list of CAP (score, position) entries, a fill count and a threshold -- its k-th best
// entry at the last compaction -- in LDS, all private to the wave that owns the query, so the epilogue needs no workgroup
// barrier.  A score that does not beat the threshold is dropped after one compare; survivors take a slot with an LDS integer
// add; when a list is full the wave ranks its entries under the total order by counting, keeps the best k in rank order and
// moves the threshold.  Which slot a survivor lands in depends on timing, the ranks do not: positions are unique.
// The partial list of (query, range) goes out sorted, short ones filled with (-inf, INT_MAX).
// ---------------------------------------------------------------------------------------------------------------------
constexpr int NN_TQ = 64, NN_TC = 128, NN_DK = 32, NN_LS = 34;
constexpr int NN_LOADS = (NN_TQ + NN_TC) * (NN_DK / 4) / 256;   // 16-byte pieces a thread moves per panel: 2 of queries, 4 of candidates
__host__ __device__ constexpr int nn_cap_of(int k) { return k <= 16 ? 32 : k <= 32 ? 64 : k <= 64 ? 128 : 256; }

// ranks of the first m entries of a list, entry lane + 64 i in lane's slot i
template <int NI>
__device__ __forceinline__ void nn_rank(const float *ls, const int32_t *lp, int m, int lane, float (&s)[NI], int32_t (&p)[NI], int (&rk)[NI]) {
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int e = lane + 64 * i;
        s[i] = e < m ? ls[e] : 0.0f;
        p[i] = e < m ? lp[e] : 0;
        rk[i] = 0;
    }
#pragma unroll 1
    for (int t = 0; t < m; ++t) {
        const float ts = ls[t];
        const int32_t tp = lp[t];
#pragma unroll
        for (int i = 0; i < NI; ++i) rk[i] += nn_beats(ts, tp, t, s[i], p[i], lane + 64 * i) ? 1 : 0;
    }
}

template <int CAP>
__global__ __launch_bounds__(256, CAP <= 32 ? 3 : CAP <= 64 ? 2 : 1) void k_nn_score_select(const float *__restrict__ Q, const int32_t *__restrict__ qpos, int64_t nq,
                                                         const float *__restrict__ X, int64_t n, int32_t D4, int64_t range_len, int32_t k,
                                                         int32_t exclude_self, int32_t *__restrict__ part_pos, float *__restrict__ part_score) {
    constexpr int NI = CAP > 64 ? CAP / 64 : 1;
    __shared__ float sq[NN_TQ * NN_LS];
    __shared__ float sx[NN_TC * NN_LS];
    __shared__ float ls[NN_TQ * CAP];
    __shared__ int32_t lp[NN_TQ * CAP];
    __shared__ float thr_s[NN_TQ];
    __shared__ int32_t thr_p[NN_TQ];
    __shared__ int32_t cnt[NN_TQ];

    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t q0 = (int64_t)blockIdx.x * NN_TQ;
    const int64_t c_begin = (int64_t)blockIdx.y * range_len;
    const int64_t c_end = c_begin + range_len < n ? c_begin + range_len : n;

    // the wave's own lists
    const int qb = wave * 16;
    if (lane < 16) { cnt[qb + lane] = 0; thr_s[qb + lane] = -INFINITY; thr_p[qb + lane] = INT_MAX; }

    // what this thread stages: piece i of a panel is row (tid + 256 i) >> 3, columns 4 ((tid + 256 i) & 7) ..
    const int c4 = (tid & 7) * 4, prow = tid >> 3;                      // rows prow, prow + 32 of the queries; prow + 32 j of the candidates
    const float *qsrc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int64_t qg = q0 + prow + 32 * i;
        qsrc[i] = qg < nq ? Q + (qpos ? (int64_t)qpos[qg] : qg) * D4 : nullptr;
    }
    f32x4 pre[NN_LOADS];
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
        for (int i = 0; i < NN_LOADS; ++i) {
            float *dst = (i < 2 ? sq + (prow + 32 * i) * NN_LS : sx + (prow + 32 * (i - 2)) * NN_LS) + c4;   // 8-byte aligned: NN_LS and c4 are even
            *reinterpret_cast<float2 *>(dst) = float2{pre[i][0], pre[i][1]};
            *reinterpret_cast<float2 *>(dst + 2) = float2{pre[i][2], pre[i][3]};
        }
    };

    // the four queries whose scores a lane holds: local rows 4 (lane >> 4) + reg of the wave's sixteen
    const int ql = qb + 4 * (lane >> 4);
    int32_t selfp[4];
    bool qok[4];
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        const int64_t qg = q0 + ql + reg;
        qok[reg] = qg < nq;
        selfp[reg] = exclude_self && qok[reg] ? (qpos ? qpos[qg] : (int32_t)qg) : -1;
    }
    const int xa = (qb + (lane & 15)) * NN_LS + (lane >> 4);
    const int xb = (lane & 15) * NN_LS + (lane >> 4);

    if (c_begin < c_end) fetch(c_begin, 0);
    for (int64_t ct = c_begin; ct < c_end; ct += NN_TC) {
        f32x4 acc[NN_TC / 16];
#pragma unroll
        for (int t = 0; t < NN_TC / 16; ++t) acc[t] = f32x4{0, 0, 0, 0};
        for (int d0 = 0; d0 < D4; d0 += NN_DK) {
            __syncthreads();
            stage();
            __syncthreads();
            if (d0 + NN_DK < D4) fetch(ct, d0 + NN_DK);
            else if (ct + NN_TC < c_end) fetch(ct + NN_TC, 0);
            auto step = [&](int dd) {
                const float a = sq[xa + dd];
                float b[NN_TC / 16];
#pragma unroll
                for (int t = 0; t < NN_TC / 16; ++t) b[t] = sx[xb + t * 16 * NN_LS + dd];
#pragma unroll
                for (int t = 0; t < NN_TC / 16; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b[t], acc[t], 0, 0, 0);
            };
            if (D4 - d0 >= NN_DK) {                                   // a whole panel: unrolled, so the reads of a step run ahead of its products
#pragma unroll
                for (int dd = 0; dd < NN_DK; dd += 4) step(dd);
            } else {
#pragma unroll 1
                for (int dd = 0; dd < D4 - d0; dd += 4) step(dd);
            }
        }
        // C/D of the f32 form: column (candidate) = lane & 15, row (query) = 4 * (lane >> 4) + register.
        // bit 4 t + reg of `todo`: the score in acc[t][reg] has still to go into its query's list
        float ts[4];
        int32_t tp[4];
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) { ts[reg] = thr_s[ql + reg]; tp[reg] = thr_p[ql + reg]; }
        uint32_t todo = 0;
#pragma unroll
        for (int t = 0; t < NN_TC / 16; ++t) {
            const int64_t c = ct + t * 16 + (lane & 15);
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                float s = acc[t][reg];
                s = s == s ? s : -INFINITY;                         // an overflowed sum ranks, and is reported, as -inf
                acc[t][reg] = s;
                if (c < c_end && qok[reg] && (int32_t)c != selfp[reg] && nn_beats(s, (int32_t)c, ts[reg], tp[reg])) todo |= 1u << (4 * t + reg);
            }
        }
        while (__any(todo != 0)) {
#pragma unroll
            for (int t = 0; t < NN_TC / 16; ++t)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg)
                    if (todo & (1u << (4 * t + reg))) {
                        const int slot = atomicAdd(&cnt[ql + reg], 1);
                        if (slot < CAP) {
                            ls[(ql + reg) * CAP + slot] = acc[t][reg];
                            lp[(ql + reg) * CAP + slot] = (int32_t)(ct + t * 16 + (lane & 15));
                            todo &= ~(1u << (4 * t + reg));
                        }
                    }
            __builtin_amdgcn_wave_barrier();
            if (!__any(todo != 0)) break;
            // some list is full: compact every full list of this wave to its best k, in rank order
            for (int j = 0; j < 16; ++j) {
                const int m = __builtin_amdgcn_readfirstlane(cnt[qb + j]);
                if (m < CAP) continue;
                float *lsj = ls + (qb + j) * CAP;
                int32_t *lpj = lp + (qb + j) * CAP;
                float s[NI];
                int32_t p[NI];
                int rk[NI];
                nn_rank<NI>(lsj, lpj, CAP, lane, s, p, rk);
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int i = 0; i < NI; ++i)
                    if (lane + 64 * i < CAP && rk[i] < k) {
                        lsj[rk[i]] = s[i];
                        lpj[rk[i]] = p[i];
                        if (rk[i] == k - 1) { thr_s[qb + j] = s[i]; thr_p[qb + j] = p[i]; }
                    }
                if (lane == 0) cnt[qb + j] = k;
                __builtin_amdgcn_wave_barrier();
            }
            // what is left must beat the new thresholds
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) { ts[reg] = thr_s[ql + reg]; tp[reg] = thr_p[ql + reg]; }
#pragma unroll
            for (int t = 0; t < NN_TC / 16; ++t)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg)
                    if ((todo & (1u << (4 * t + reg))) && !nn_beats(acc[t][reg], (int32_t)(ct + t * 16 + (lane & 15)), ts[reg], tp[reg]))
                        todo &= ~(1u << (4 * t + reg));
        }
    }

    // the wave's sixteen lists go out in rank order
    __builtin_amdgcn_wave_barrier();
    for (int j = 0; j < 16; ++j) {
        const int64_t qg = q0 + qb + j;
        if (qg >= nq) break;
        int m = __builtin_amdgcn_readfirstlane(cnt[qb + j]);
        m = m < CAP ? m : CAP;
        float s[NI];
        int32_t p[NI];
        int rk[NI];
        nn_rank<NI>(ls + (qb + j) * CAP, lp + (qb + j) * CAP, m, lane, s, p, rk);
        const int64_t base = (qg * gridDim.y + blockIdx.y) * k;
#pragma unroll
        for (int i = 0; i < NI; ++i)
            if (lane + 64 * i < m && rk[i] < k) { part_score[base + rk[i]] = s[i]; part_pos[base + rk[i]] = p[i]; }
        for (int e = m + lane; e < k; e += 64) { part_score[base + e] = -INFINITY; part_pos[base + e] = INT_MAX; }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Merge.  One wave per query: the running best k and the next range's k entries sit side by side in LDS, are ranked under the
// same total order and the best k kept, range after range in ascending order.  Positions become original row ids on the way out.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_nn_merge(const int32_t *__restrict__ part_pos, const float *__restrict__ part_score, int32_t ranges, int32_t k,
                                                 const int32_t *__restrict__ ids, int32_t *__restrict__ out_index, float *__restrict__ out_score) {
    constexpr int NI = 2 * NN_MAX_K / 64;
    __shared__ float ms[2 * NN_MAX_K];
    __shared__ int32_t mp[2 * NN_MAX_K];
    const int lane = (int)threadIdx.x;
    const int64_t q = blockIdx.x, base = q * ranges * k;
    for (int e = lane; e < k; e += 64) { ms[e] = part_score[base + e]; mp[e] = part_pos[base + e]; }
    for (int r = 1; r < ranges; ++r) {
        for (int e = lane; e < k; e += 64) { ms[k + e] = part_score[base + (int64_t)r * k + e]; mp[k + e] = part_pos[base + (int64_t)r * k + e]; }
        __builtin_amdgcn_wave_barrier();
        float s[NI];
        int32_t p[NI];
        int rk[NI];
        nn_rank<NI>(ms, mp, 2 * k, lane, s, p, rk);
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int i = 0; i < NI; ++i)
            if (lane + 64 * i < 2 * k && rk[i] < k) { ms[rk[i]] = s[i]; mp[rk[i]] = p[i]; }
        __builtin_amdgcn_wave_barrier();
    }
    __builtin_amdgcn_wave_barrier();
    for (int e = lane; e < k; e += 64) {
        const int32_t pos = mp[e];
        out_score[q * k + e] = ms[e];
        out_index[q * k + e] = ids && pos != INT_MAX ? ids[pos] : pos;
    }
}

struct DeviceBuffers {                      // freed on every way out
    std::vector<void *> ptrs;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~DeviceBuffers() { for (void *q : ptrs) (void)hipFree(q); if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
    ge_status alloc(void **q, size_t bytes) { GE_HIP(hipMalloc(q, std::max<size_t>(bytes, 16))); ptrs.push_back(*q); return GE_OK; }
    ge_status events() { GE_HIP(hipEventCreate(&e0)); GE_HIP(hipEventCreate(&e1)); return GE_OK; }
};

}  // namespace

struct ge_nn {
    int32_t metric = 0, device = 0, dim = 0, d4 = 0;
    int64_t n_rows = 0, n_indexed = 0;
    hipStream_t stream = nullptr;
    std::vector<int32_t> subset;            // original row id of every indexed row; empty = all rows
    float *dx = nullptr;                    // [n_indexed][d4], prepared
    int32_t *dids = nullptr;                // `subset` on the device, or NULL
    mutable float prepare_ms = 0, query_ms = 0;
    ~ge_nn() { if (dx) (void)hipFree(dx); if (dids) (void)hipFree(dids); }
};

namespace {

ge_status check_create(int64_t n_rows, int32_t dim, const int32_t *subset, int64_t n_subset, const ge_nn_cfg *cfg) {
    if (!cfg) return ge::fail(GE_ERR_ARG, "ge_nn_cfg is null");
    if (cfg->metric != GE_NN_COSINE && cfg->metric != GE_NN_DOT) return ge::fail(GE_ERR_ARG, "nn: unknown metric %d", cfg->metric);
    if (dim < 1 || dim > NN_MAX_DIM) return ge::fail(GE_ERR_ARG, "nn: dim %d outside [1, %d]", dim, NN_MAX_DIM);
    if (n_rows < 1 || n_rows >= INT_MAX) return ge::fail(GE_ERR_ARG, "nn: %lld rows outside [1, 2^31 - 2]", (long long)n_rows);
    if (n_rows > NN_MAX_FLOATS / dim)
        return ge::fail(GE_ERR_ARG, "nn: %lld rows of %d floats are more than one index holds (%lld floats)", (long long)n_rows, dim, (long long)NN_MAX_FLOATS);
    if (subset) {
        if (n_subset < 1 || n_subset > n_rows) return ge::fail(GE_ERR_ARG, "nn: a subset of %lld of %lld rows", (long long)n_subset, (long long)n_rows);
        for (int64_t i = 0; i < n_subset; ++i) {
            if (subset[i] < 0 || subset[i] >= n_rows) return ge::fail(GE_ERR_ARG, "nn: subset[%lld] = %d outside [0, %lld)", (long long)i, subset[i], (long long)n_rows);
            if (i > 0 && subset[i] <= subset[i - 1]) return ge::fail(GE_ERR_ARG, "nn: the subset is not strictly ascending at [%lld]", (long long)i);
        }
    }
    return GE_OK;
}

// rows (host: slab by slab; dev: in place) -> table[rows_out][d4], prepared; *ms += the kernels' time
ge_status prepare_rows(const float *host, const float *dev, const int32_t *host_map, const int32_t *dev_map, int64_t rows_out, int32_t dim,
                       int32_t metric, float *table, hipStream_t stream, const char *what, float *ms_out) {
    const int D = dim, D4 = (D + 3) / 4 * 4;
    const int64_t slab_rows = std::min<int64_t>(std::max<int64_t>(PREP_ROWS, NN_SLAB_FLOATS / D / PREP_ROWS * PREP_ROWS), rows_out);
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
        hipLaunchKernelGGL(k_nn_prepare, dim3((unsigned)((rows + PREP_ROWS - 1) / PREP_ROWS)), dim3(64), 0, stream, x, map, rows, D, D4, metric,
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
    if (flag) return ge::fail(GE_ERR_ARG, "nn: non-finite input (%s)", what);
    *ms_out += total;
    return GE_OK;
}

ge_status create_impl(const float *host, const float *dev, int64_t n_rows, int32_t dim, const int32_t *subset, int64_t n_subset, const ge_nn_cfg *cfg,
                      ge_nn **out) {
    std::unique_ptr<ge_nn> p(new ge_nn);
    p->metric = cfg->metric; p->device = cfg->device; p->stream = (hipStream_t)cfg->stream;
    p->dim = dim; p->d4 = (dim + 3) / 4 * 4; p->n_rows = n_rows; p->n_indexed = subset ? n_subset : n_rows;
    if (subset) p->subset.assign(subset, subset + n_subset);
    GE_HIP(hipMalloc((void **)&p->dx, sizeof(float) * (size_t)p->n_indexed * p->d4));
    if (subset) {
        GE_HIP(hipMalloc((void **)&p->dids, sizeof(int32_t) * (size_t)n_subset));
        GE_HIP(hipMemcpyAsync(p->dids, subset, sizeof(int32_t) * (size_t)n_subset, hipMemcpyHostToDevice, p->stream));
    }
    GE_CHECK(prepare_rows(host, dev, subset, p->dids, p->n_indexed, dim, p->metric, p->dx, p->stream, "rows", &p->prepare_ms));
    *out = p.release();
    return GE_OK;
}

ge_status nn_create_host(const float *rows, int64_t n_rows, int32_t dim, const int32_t *subset, int64_t n_subset, const ge_nn_cfg *cfg, ge_nn **out) {
    if (out) *out = nullptr;
    if (!rows || !out) return ge::fail(GE_ERR_ARG, "ge_nn_create: rows or out is null");
    GE_CHECK(check_create(n_rows, dim, subset, n_subset, cfg));
    GE_CHECK(ge::select_device(cfg->device));
    return create_impl(rows, nullptr, n_rows, dim, subset, n_subset, cfg, out);
}

ge_status nn_create_glove(ge_glove *h, const int32_t *subset, int64_t n_subset, const ge_nn_cfg *cfg, ge_nn **out) {
    if (out) *out = nullptr;
    if (!h || !out) return ge::fail(GE_ERR_ARG, "ge_glove_nn_create: handle or out is null");
    if (!cfg) return ge::fail(GE_ERR_ARG, "ge_nn_cfg is null");
    float *d = nullptr;
    int32_t V = 0, D = 0, device = 0;
    GE_CHECK(ge::glove_extract_device_f32(h, &d, &V, &D, &device));   // a fresh buffer: no trainer table is written
    ge_nn_cfg own = *cfg;
    own.device = device;                                              // the rows live on the handle's device
    ge_status st = check_create(V, D, subset, n_subset, &own);
    if (st == GE_OK) st = create_impl(nullptr, d, V, D, subset, n_subset, &own, out);
    (void)hipFree(d);
    return st;
}

template <int CAP>
void launch_score(dim3 grid, hipStream_t stream, const float *Q, const int32_t *qpos, int64_t nq, const float *X, int64_t n, int32_t D4, int64_t range_len,
                  int32_t k, int32_t exclude_self, int32_t *ppos, float *pscore) {
    hipLaunchKernelGGL(k_nn_score_select<CAP>, grid, dim3(256), 0, stream, Q, qpos, nq, X, n, D4, range_len, k, exclude_self, ppos, pscore);
}

// queries: positions in the index (qpos, NULL = 0 .. n_queries - 1 when vectors is NULL too) or values (vectors)
ge_status query_impl(ge_nn *p, const int32_t *qpos, const float *vectors, int64_t n_queries, int32_t k, int32_t exclude_self, int32_t *out_index,
                     float *out_score) {
    hipStream_t stream = p->stream;
    const int64_t n = p->n_indexed;
    const int D4 = p->d4;
    // candidate ranges: whole tiles of NN_TC, as many as fill the device a few times over when the queries alone do not
    const int64_t ctiles = (n + NN_TC - 1) / NN_TC;
    auto ranges_for = [&](int64_t nq) {
        const int64_t qtiles = (nq + NN_TQ - 1) / NN_TQ;
        const int64_t want = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(ctiles, 1024), (2048 + qtiles - 1) / qtiles));
        const int64_t range_tiles = (ctiles + want - 1) / want;
        return std::pair<int64_t, int64_t>((ctiles + range_tiles - 1) / range_tiles, range_tiles * NN_TC);
    };
    const int64_t ranges_all = ranges_for(n_queries).first;
    const int64_t batch = std::max<int64_t>(NN_TQ, std::min<int64_t>(n_queries, NN_BATCH_ENTRIES / (ranges_all * k) / NN_TQ * NN_TQ));
    const auto rb = ranges_for(std::min(batch, n_queries));
    const int64_t ranges = rb.first, range_len = rb.second;

    DeviceBuffers B;
    float *dq = nullptr, *dps = nullptr, *dos = nullptr;
    int32_t *dqpos = nullptr, *dpp = nullptr, *doi = nullptr;
    GE_CHECK(B.events());
    const int64_t nb = std::min(batch, n_queries);
    if (vectors) GE_CHECK(B.alloc((void **)&dq, sizeof(float) * (size_t)nb * D4));
    if (qpos) GE_CHECK(B.alloc((void **)&dqpos, sizeof(int32_t) * (size_t)nb));
    GE_CHECK(B.alloc((void **)&dpp, sizeof(int32_t) * (size_t)(nb * ranges * k)));
    GE_CHECK(B.alloc((void **)&dps, sizeof(float) * (size_t)(nb * ranges * k)));
    GE_CHECK(B.alloc((void **)&doi, sizeof(int32_t) * (size_t)(nb * k)));
    GE_CHECK(B.alloc((void **)&dos, sizeof(float) * (size_t)(nb * k)));
    const int CAP = nn_cap_of(k);
    float total = 0;
    for (int64_t begin = 0; begin < n_queries; begin += batch) {
        const int64_t nq = std::min(batch, n_queries - begin);
        const float *Q = p->dx;
        const int32_t *QP = nullptr;
        if (vectors) {
            float prep_ms = 0;
            GE_CHECK(prepare_rows(vectors + begin * p->dim, nullptr, nullptr, nullptr, nq, p->dim, p->metric, dq, stream, "query vectors", &prep_ms));
            total += prep_ms;
            Q = dq;
        } else if (qpos) {
            GE_HIP(hipMemcpyAsync(dqpos, qpos + begin, sizeof(int32_t) * (size_t)nq, hipMemcpyHostToDevice, stream));
            QP = dqpos;
        } else {
            Q = p->dx + begin * D4;                                   // every indexed row, in order
        }
        // without a position list the kernel takes query q for position q: shift the self test instead of building the list
        if (!vectors && !qpos && exclude_self && begin > 0) {
            std::vector<int32_t> ident((size_t)nq);
            for (int64_t i = 0; i < nq; ++i) ident[(size_t)i] = (int32_t)(begin + i);
            if (!dqpos) GE_CHECK(B.alloc((void **)&dqpos, sizeof(int32_t) * (size_t)nb));
            GE_HIP(hipMemcpyAsync(dqpos, ident.data(), sizeof(int32_t) * (size_t)nq, hipMemcpyHostToDevice, stream));
            GE_HIP(hipStreamSynchronize(stream));
            Q = p->dx; QP = dqpos;
        }
        const dim3 grid((unsigned)((nq + NN_TQ - 1) / NN_TQ), (unsigned)ranges);
        GE_HIP(hipEventRecord(B.e0, stream));
        switch (CAP) {
        case 32: launch_score<32>(grid, stream, Q, QP, nq, p->dx, n, D4, range_len, k, exclude_self, dpp, dps); break;
        case 64: launch_score<64>(grid, stream, Q, QP, nq, p->dx, n, D4, range_len, k, exclude_self, dpp, dps); break;
        case 128: launch_score<128>(grid, stream, Q, QP, nq, p->dx, n, D4, range_len, k, exclude_self, dpp, dps); break;
        default: launch_score<256>(grid, stream, Q, QP, nq, p->dx, n, D4, range_len, k, exclude_self, dpp, dps); break;
        }
        GE_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_nn_merge, dim3((unsigned)nq), dim3(64), 0, stream, dpp, dps, (int32_t)ranges, k, p->dids, doi, dos);
        GE_HIP(hipGetLastError());
        GE_HIP(hipEventRecord(B.e1, stream));
        GE_HIP(hipMemcpyAsync(out_index + begin * k, doi, sizeof(int32_t) * (size_t)(nq * k), hipMemcpyDeviceToHost, stream));
        GE_HIP(hipMemcpyAsync(out_score + begin * k, dos, sizeof(float) * (size_t)(nq * k), hipMemcpyDeviceToHost, stream));
        GE_HIP(hipStreamSynchronize(stream));
        float ms = 0;
        GE_HIP(hipEventElapsedTime(&ms, B.e0, B.e1));
        total += ms;
    }
    p->query_ms = total;
    return GE_OK;
}

ge_status check_query(const ge_nn *p, int64_t n_queries, int32_t k, int32_t exclude_self, const void *out_index, const void *out_score, const char *fn) {
    if (!p) return ge::fail(GE_ERR_ARG, "null ge_nn handle");
    if (!out_index || !out_score) return ge::fail(GE_ERR_ARG, "%s: out_index or out_score is null", fn);
    if (n_queries < 1) return ge::fail(GE_ERR_ARG, "%s: %lld queries", fn, (long long)n_queries);
    if (k < 1 || k > NN_MAX_K) return ge::fail(GE_ERR_ARG, "nn: k %d outside [1, %d]", k, NN_MAX_K);
    const int64_t candidates = p->n_indexed - (exclude_self ? 1 : 0);
    if (k > candidates) return ge::fail(GE_ERR_ARG, "nn: k %d exceeds the %lld candidates of a query", k, (long long)candidates);
    return GE_OK;
}

ge_status nn_query_rows(ge_nn *p, const int32_t *query_ids, int64_t n_queries, int32_t k, int32_t exclude_self, int32_t *out_index, float *out_score) {
    if (p && !query_ids && n_queries != p->n_indexed)
        return ge::fail(GE_ERR_ARG, "ge_nn_query_rows: query_ids is null, so n_queries must be the %lld indexed rows, not %lld", (long long)p->n_indexed,
                        (long long)n_queries);
    GE_CHECK(check_query(p, n_queries, k, exclude_self, out_index, out_score, "ge_nn_query_rows"));
    std::vector<int32_t> pos;
    if (query_ids) {
        pos.resize((size_t)n_queries);
        for (int64_t i = 0; i < n_queries; ++i) {
            const int32_t id = query_ids[i];
            int64_t at = -1;
            if (p->subset.empty()) at = id >= 0 && id < p->n_rows ? id : -1;
            else {
                const auto it = std::lower_bound(p->subset.begin(), p->subset.end(), id);
                if (it != p->subset.end() && *it == id) at = it - p->subset.begin();
            }
            if (at < 0) return ge::fail(GE_ERR_ARG, "nn: query_ids[%lld] = %d is not a row of the index", (long long)i, id);
            pos[(size_t)i] = (int32_t)at;
        }
    }
    GE_CHECK(ge::select_device(p->device));
    return query_impl(p, query_ids ? pos.data() : nullptr, nullptr, n_queries, k, exclude_self ? 1 : 0, out_index, out_score);
}

ge_status nn_query_vectors(ge_nn *p, const float *vectors, int64_t n_queries, int32_t k, int32_t *out_index, float *out_score) {
    if (p && !vectors) return ge::fail(GE_ERR_ARG, "ge_nn_query_vectors: vectors is null");
    GE_CHECK(check_query(p, n_queries, k, 0, out_index, out_score, "ge_nn_query_vectors"));
    GE_CHECK(ge::select_device(p->device));
    return query_impl(p, nullptr, vectors, n_queries, k, 0, out_index, out_score);
}

}  // namespace

extern "C" {

void ge_nn_cfg_default(ge_nn_cfg *cfg) {
    if (!cfg) return;
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->metric = GE_NN_COSINE;
}
int32_t ge_nn_cfg_size(void) { return (int32_t)sizeof(ge_nn_cfg); }

ge_status ge_nn_create(const float *rows, int64_t n_rows, int32_t dim, const int32_t *subset, int64_t n_subset, const ge_nn_cfg *cfg, ge_nn **out) {
    GE_GUARD(nn_create_host(rows, n_rows, dim, subset, n_subset, cfg, out));
}
ge_status ge_glove_nn_create(ge_glove *h, const int32_t *subset, int64_t n_subset, const ge_nn_cfg *cfg, ge_nn **out) {
    GE_GUARD(nn_create_glove(h, subset, n_subset, cfg, out));
}
ge_status ge_nn_query_rows(ge_nn *p, const int32_t *query_ids, int64_t n_queries, int32_t k, int32_t exclude_self, int32_t *out_index, float *out_score) {
    GE_GUARD(nn_query_rows(p, query_ids, n_queries, k, exclude_self, out_index, out_score));
}
ge_status ge_nn_query_vectors(ge_nn *p, const float *vectors, int64_t n_queries, int32_t k, int32_t *out_index, float *out_score) {
    GE_GUARD(nn_query_vectors(p, vectors, n_queries, k, out_index, out_score));
}

ge_status ge_nn_get(const ge_nn *p, int64_t *n_indexed, int32_t *dim, int32_t *metric) {
    if (!p) return ge::fail(GE_ERR_ARG, "null ge_nn handle");
    if (n_indexed) *n_indexed = p->n_indexed;
    if (dim) *dim = p->dim;
    if (metric) *metric = p->metric;
    return GE_OK;
}

ge_status ge_nn_last_kernel_ms(const ge_nn *p, float *prepare_ms, float *query_ms) {
    if (!p) return ge::fail(GE_ERR_ARG, "null ge_nn handle");
    if (prepare_ms) *prepare_ms = p->prepare_ms;
    if (query_ms) *query_ms = p->query_ms;
    return GE_OK;
}

void ge_nn_destroy(ge_nn *p) { delete p; }

}  // extern "C"
