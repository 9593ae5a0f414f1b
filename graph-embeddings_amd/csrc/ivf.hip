// ivf.hip -- an inverted-file (IVF-flat) neighbour index behind the C ABI: ge_ivf_* (include/geglove.h, "Inverted-file index").
// The rows are prepared as nn.hip prepares them, grouped by their best centroid (the centroids come from ge_kmeans_* or from
// the caller) and stored list after list.  A query is scored against the centroids, the lists of its nprobe best centroids are
// scanned by k_ivf_scan -- the score-and-select tile of nn.hip's k_nn_score_select, fed from a schedule of (list chunk, tile of
// the queries that probe the list) work items -- and the partial lists of a query are merged in a fixed order (k_ivf_merge).
// Scoring the centroids is the same kernel on a schedule that needs no tables (every query against every chunk of one table),
// and so is the assign of the build (k = 1).  No floating-point atomics; the reference has no counterpart.
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

constexpr int IVF_MAX_DIM = 1024, IVF_MAX_K = 128, IVF_MAX_PROBE = 128, IVF_MAX_LISTS = 65536, IVF_MAX_ITER = 1024;
constexpr int64_t IVF_MAX_FLOATS = (int64_t)1 << 35;         // floats of input one index accepts, as ge_nn_create
constexpr int64_t IVF_SLAB_FLOATS = (int64_t)1 << 26;        // a 256 MB slab of rows per upload
constexpr int64_t IVF_BATCH_ENTRIES = (int64_t)1 << 24;      // partial-list entries per batch of queries (128 MB of them)
constexpr int IVF_CHUNK = 4096;                              // rows of a list one work item scans
constexpr int IVF_PROBE_CHUNK = 1024;                        // centroids one work item of the probe (and of the assign) scores

// the order of the results: score descending as fp32 compares them, then key (original row id, or centroid id) ascending, then
// (for the fill entries of short lists, which share one key) slot ascending -- a strict total order, so ranks are a permutation
__device__ __forceinline__ bool ivf_beats(float sa, int32_t pa, int ea, float sb, int32_t pb, int eb) {
    return sa > sb || (sa == sb && (pa < pb || (pa == pb && ea < eb)));
}
__device__ __forceinline__ bool ivf_beats(float sa, int32_t pa, float sb, int32_t pb) { return sa > sb || (sa == sb && pa < pb); }

// ---------------------------------------------------------------------------------------------------------------------
// Prepare.  k_nn_prepare's walk (cosine only): one wave takes 64 rows; pieces of 64 columns are read coalesced into LDS, lane r
// then walks row r of the piece in ascending d (the fp64 sum of squares is a sequential chain), and a second coalesced pass
// writes x / n rounded to fp32 once into the table, whose rows are padded with zeros to D4.  rowmap: NULL or the source row of
// every output row.  A non-finite value raises *flag (every writer stores the same 1).
// ---------------------------------------------------------------------------------------------------------------------
constexpr int PREP_ROWS = 64, PREP_COLS = 64, PREP_STRIDE = 65;

__global__ __launch_bounds__(64) void k_ivf_prepare(const float *__restrict__ src, const int32_t *__restrict__ rowmap, int64_t n_rows, int32_t D,
                                                    int32_t D4, float *__restrict__ out, int32_t *__restrict__ flag) {
    __shared__ float tile[PREP_ROWS * PREP_STRIDE];
    __shared__ double norm[PREP_ROWS];
    const int lane = (int)threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * PREP_ROWS;
    const int rows = (int)(n_rows - row0 < PREP_ROWS ? n_rows - row0 : PREP_ROWS);
    bool bad = false;
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
    for (int d0 = 0; d0 < D4; d0 += PREP_COLS) {
        const int d = d0 + lane;
        if (d >= D4) break;
        for (int r = 0; r < rows; ++r) {
            const int64_t s = rowmap ? (int64_t)rowmap[row0 + r] : row0 + r;
            float x = d < D ? src[s * D + d] : 0.0f;
            bad |= !(fabsf(x) <= 3.402823466e38f);
            const double n = norm[r];
            out[(row0 + r) * D4 + d] = n > 0.0 ? (float)((double)x / n) : 0.0f;
        }
    }
    if (bad) *flag = 1;
}

// ---------------------------------------------------------------------------------------------------------------------
// The schedule of a scan.  Work item w = blockIdx.x is one chunk of candidate rows times one tile of up to 64 queries.
//   dense  (pairs == NULL): every one of nq queries against rows [0, n_cand) of one table cut into `chunks` chunks of chunk_len;
//          w = tile * chunks + chunk; the partial slot of (query q, chunk) is q * chunks + chunk.
//   listed: the (query, list) pairs e = q * nprobe + j of a batch, stably sorted by list (`pairs`, so queries ascend inside a
//          list), pstart[c] the first sorted pair of list c; list c is rows [off[c], off[c + 1]) of the table, cut into
//          ceil(len / chunk_len) chunks; it has tiles * chunks work items, numbered from first[c] (an exclusive scan), tile-major.
//          The partial slots of pair e are sbase[e] + chunk (an exclusive scan of the pairs' chunk counts in pair order, so the
//          slots of a query are consecutive).  Empty lists and lists nobody probes have no items.
// ---------------------------------------------------------------------------------------------------------------------
struct IvfWork {
    int64_t nq, n_cand;
    int32_t chunks, chunk_len;
    const int32_t *pairs, *pstart, *off;
    const uint32_t *first, *sbase;
    int32_t lists, nprobe;
};

// ---------------------------------------------------------------------------------------------------------------------
// Scan: score and select.  The tile of k_nn_score_select: per 32 columns the query and candidate panels are staged in LDS as
// [row][34] (34 = 2 mod 32: the 32 lanes one ds_read_b32 cycle serves hit 32 different banks), the next panel travelling in
// registers meanwhile; wave w carries queries 16 w .. 16 w + 15 of the tile against 128 candidates through
// v_mfma_f32_16x16x4_f32: eight accumulators, each bit for bit an fmaf chain over ascending d.  Selection as there: per query a
// list of CAP (score, key) entries, a fill count and a threshold in LDS, private to the wave that owns the query; survivors of
// the threshold take a slot with an LDS integer add, a full list is ranked by counting and cut to its best k.
// What differs from nn.hip:
//   - the tile's queries come through the schedule: s_row[i] is the row of Q that query i of the tile reads (-1: no such query,
//     whose slot never enters a list and writes nothing), s_slot[i] its partial slot, s_self[i] the key it must not return;
//   - the key of a candidate -- what breaks ties and what exclude_self compares -- is keys[row], the ORIGINAL row id, loaded per
//     candidate tile: across lists the order of the table is not the order of the ids.  (keys == NULL: the row number itself,
//     for the centroid table);
//   - rows past the chunk's end are never looked at (the panel holds zeros there, their scores are dropped before the lists).
// ---------------------------------------------------------------------------------------------------------------------
constexpr int IV_TQ = 64, IV_TC = 128, IV_DK = 32, IV_LS = 34;
constexpr int IV_LOADS = (IV_TQ + IV_TC) * (IV_DK / 4) / 256;   // 16-byte pieces a thread moves per panel: 2 of queries, 4 of candidates
__host__ __device__ constexpr int ivf_cap_of(int k) { return k <= 16 ? 32 : k <= 32 ? 64 : k <= 64 ? 128 : 256; }

// ranks of the first m entries of a list, entry lane + 64 i in lane's slot i
template <int NI>
__device__ __forceinline__ void ivf_rank(const float *ls, const int32_t *lp, int m, int lane, float (&s)[NI], int32_t (&p)[NI], int (&rk)[NI]) {
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
        for (int i = 0; i < NI; ++i) rk[i] += ivf_beats(ts, tp, t, s[i], p[i], lane + 64 * i) ? 1 : 0;
    }
}

template <int CAP>
__global__ __launch_bounds__(256, CAP <= 32 ? 3 : CAP <= 64 ? 2 : 1) void k_ivf_scan(IvfWork W, const float *__restrict__ Q, const int32_t *__restrict__ qrow,
                                                         const int32_t *__restrict__ qself, const float *__restrict__ X,
                                                         const int32_t *__restrict__ keys, int32_t D4, int32_t k,
                                                         int32_t *__restrict__ part_key, float *__restrict__ part_score) {
    constexpr int NI = CAP > 64 ? CAP / 64 : 1;
    __shared__ float sq[IV_TQ * IV_LS];
    __shared__ float sx[IV_TC * IV_LS];
    __shared__ float ls[IV_TQ * CAP];
    __shared__ int32_t lp[IV_TQ * CAP];
    __shared__ float thr_s[IV_TQ];
    __shared__ int32_t thr_p[IV_TQ];
    __shared__ int32_t cnt[IV_TQ];
    __shared__ int32_t s_row[IV_TQ];
    __shared__ uint32_t s_slot[IV_TQ];
    __shared__ int32_t s_self[IV_TQ];

    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    // the work item: every thread decodes it (the same few cached reads), the first 64 fill in the tile's queries
    const uint32_t w = blockIdx.x;
    int64_t c_begin, c_end;
    if (!W.pairs) {
        const uint32_t tile = w / (uint32_t)W.chunks, chunk = w % (uint32_t)W.chunks;
        c_begin = (int64_t)chunk * W.chunk_len;
        c_end = c_begin + W.chunk_len < W.n_cand ? c_begin + W.chunk_len : W.n_cand;
        if (tid < IV_TQ) {
            const int64_t q = (int64_t)tile * IV_TQ + tid;
            const bool in = q < W.nq;
            s_row[tid] = in ? (qrow ? qrow[q] : (int32_t)q) : -1;
            s_slot[tid] = in ? (uint32_t)(q * W.chunks + chunk) : 0u;
            s_self[tid] = in && qself ? qself[q] : -1;
        }
    } else {
        int lo = 0, hi = W.lists - 1;                         // the last list c with first[c] <= w: the one the item belongs to
        while (lo < hi) {
            const int mid = lo + (hi - lo + 1) / 2;
            if (W.first[mid] <= w) lo = mid; else hi = mid - 1;
        }
        const int c = lo;
        const int32_t o0 = W.off[c], o1 = W.off[c + 1];
        const uint32_t chunks = (uint32_t)((o1 - o0 + W.chunk_len - 1) / W.chunk_len);
        const uint32_t local = w - W.first[c], tile = local / chunks, chunk = local % chunks;
        c_begin = (int64_t)o0 + (int64_t)chunk * W.chunk_len;
        c_end = c_begin + W.chunk_len < (int64_t)o1 ? c_begin + W.chunk_len : (int64_t)o1;
        if (tid < IV_TQ) {
            const int64_t at = (int64_t)W.pstart[c] + (int64_t)tile * IV_TQ + tid;
            const bool in = at < (int64_t)W.pstart[c + 1];
            int32_t row = -1, self = -1;
            uint32_t slot = 0;
            if (in) {
                const int32_t e = W.pairs[at];
                const int32_t q = e / W.nprobe;
                row = qrow ? qrow[q] : q;
                self = qself ? qself[q] : -1;
                slot = W.sbase[e] + chunk;
            }
            s_row[tid] = row; s_slot[tid] = slot; s_self[tid] = self;
        }
    }

    // the wave's own lists
    const int qb = wave * 16;
    if (lane < 16) { cnt[qb + lane] = 0; thr_s[qb + lane] = -INFINITY; thr_p[qb + lane] = INT_MAX; }
    __syncthreads();

    // what this thread stages: piece i of a panel is row (tid + 256 i) >> 3, columns 4 ((tid + 256 i) & 7) ..
    const int c4 = (tid & 7) * 4, prow = tid >> 3;                      // rows prow, prow + 32 of the queries; prow + 32 j of the candidates
    const float *qsrc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int32_t r = s_row[prow + 32 * i];
        qsrc[i] = r >= 0 ? Q + (int64_t)r * D4 : nullptr;
    }
    f32x4 pre[IV_LOADS];
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
        for (int i = 0; i < IV_LOADS; ++i) {
            float *dst = (i < 2 ? sq + (prow + 32 * i) * IV_LS : sx + (prow + 32 * (i - 2)) * IV_LS) + c4;   // 8-byte aligned: IV_LS and c4 are even
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
        qok[reg] = s_row[ql + reg] >= 0;
        selfp[reg] = s_self[ql + reg];                                  // -1 or an id: no key is negative
    }
    const int xa = (qb + (lane & 15)) * IV_LS + (lane >> 4);
    const int xb = (lane & 15) * IV_LS + (lane >> 4);

    if (c_begin < c_end) fetch(c_begin, 0);
    for (int64_t ct = c_begin; ct < c_end; ct += IV_TC) {
        // the keys of this tile's candidates, asked for ahead of the products
        int32_t ckey[IV_TC / 16];
#pragma unroll
        for (int t = 0; t < IV_TC / 16; ++t) {
            const int64_t c = ct + t * 16 + (lane & 15);
            ckey[t] = c < c_end ? (keys ? keys[c] : (int32_t)c) : INT_MAX;
        }
        f32x4 acc[IV_TC / 16];
#pragma unroll
        for (int t = 0; t < IV_TC / 16; ++t) acc[t] = f32x4{0, 0, 0, 0};
        for (int d0 = 0; d0 < D4; d0 += IV_DK) {
            __syncthreads();
            stage();
            __syncthreads();
            if (d0 + IV_DK < D4) fetch(ct, d0 + IV_DK);
            else if (ct + IV_TC < c_end) fetch(ct + IV_TC, 0);
            auto step = [&](int dd) {
                const float a = sq[xa + dd];
                float b[IV_TC / 16];
#pragma unroll
                for (int t = 0; t < IV_TC / 16; ++t) b[t] = sx[xb + t * 16 * IV_LS + dd];
#pragma unroll
                for (int t = 0; t < IV_TC / 16; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b[t], acc[t], 0, 0, 0);
            };
            if (D4 - d0 >= IV_DK) {                                   // a whole panel: unrolled, so the reads of a step run ahead of its products
#pragma unroll
                for (int dd = 0; dd < IV_DK; dd += 4) step(dd);
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
        for (int t = 0; t < IV_TC / 16; ++t) {
            const bool cin = ct + t * 16 + (lane & 15) < c_end;
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                float s = acc[t][reg];
                s = s == s ? s : -INFINITY;                         // an overflowed sum ranks, and is reported, as -inf
                acc[t][reg] = s;
                if (cin && qok[reg] && ckey[t] != selfp[reg] && ivf_beats(s, ckey[t], ts[reg], tp[reg])) todo |= 1u << (4 * t + reg);
            }
        }
        while (__any(todo != 0)) {
#pragma unroll
            for (int t = 0; t < IV_TC / 16; ++t)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg)
                    if (todo & (1u << (4 * t + reg))) {
                        const int slot = atomicAdd(&cnt[ql + reg], 1);
                        if (slot < CAP) {
                            ls[(ql + reg) * CAP + slot] = acc[t][reg];
                            lp[(ql + reg) * CAP + slot] = ckey[t];
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
                ivf_rank<NI>(lsj, lpj, CAP, lane, s, p, rk);
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
            for (int t = 0; t < IV_TC / 16; ++t)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg)
                    if ((todo & (1u << (4 * t + reg))) && !ivf_beats(acc[t][reg], ckey[t], ts[reg], tp[reg])) todo &= ~(1u << (4 * t + reg));
        }
    }

    // the wave's lists go out in rank order, short ones filled; a slot of the tile without a query writes nothing
    __builtin_amdgcn_wave_barrier();
    for (int j = 0; j < 16; ++j) {
        if (__builtin_amdgcn_readfirstlane(s_row[qb + j]) < 0) continue;
        int m = __builtin_amdgcn_readfirstlane(cnt[qb + j]);
        m = m < CAP ? m : CAP;
        float s[NI];
        int32_t p[NI];
        int rk[NI];
        ivf_rank<NI>(ls + (qb + j) * CAP, lp + (qb + j) * CAP, m, lane, s, p, rk);
        const int64_t base = (int64_t)s_slot[qb + j] * k;
#pragma unroll
        for (int i = 0; i < NI; ++i)
            if (lane + 64 * i < m && rk[i] < k) { part_score[base + rk[i]] = s[i]; part_key[base + rk[i]] = p[i]; }
        for (int e = (m < k ? m : k) + lane; e < k; e += 64) { part_score[base + e] = -INFINITY; part_key[base + e] = INT_MAX; }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Merge.  One wave per query (k_nn_merge's scheme): the running best k and the next slot's k entries sit side by side in LDS,
// are ranked under the same total order and the best k kept, slot after slot in ascending order.  The slots of query q are
// [sbase[q nprobe], sbase[(q + 1) nprobe]) (listed) or [q per_q, (q + 1) per_q) (dense, sbase == NULL); none: only fill.
// Fill entries (key INT_MAX) go out as (-1, -inf); out_count = the real ones; out_cand = the sizes of the probed lists summed,
// less `minus_self` (the query's own list is always among its probed ones: probing and assigning are the same order).
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_ivf_merge(const int32_t *__restrict__ part_key, const float *__restrict__ part_score, const uint32_t *__restrict__ sbase,
                                                  int32_t per_q, int32_t nprobe, int32_t k, int32_t *__restrict__ out_index, float *__restrict__ out_score,
                                                  int32_t *__restrict__ out_count, const int32_t *__restrict__ probe, const int32_t *__restrict__ off,
                                                  int32_t minus_self, int32_t *__restrict__ out_cand) {
    constexpr int NI = 2 * IVF_MAX_K / 64;
    __shared__ float ms[2 * IVF_MAX_K];
    __shared__ int32_t mp[2 * IVF_MAX_K];
    const int lane = (int)threadIdx.x;
    const int64_t q = blockIdx.x;
    const int64_t s0 = sbase ? (int64_t)sbase[q * nprobe] : q * per_q;
    const int64_t s1 = sbase ? (int64_t)sbase[(q + 1) * nprobe] : (q + 1) * per_q;
    for (int e = lane; e < k; e += 64) {
        ms[e] = s0 < s1 ? part_score[s0 * k + e] : -INFINITY;
        mp[e] = s0 < s1 ? part_key[s0 * k + e] : INT_MAX;
    }
    for (int64_t r = s0 + 1; r < s1; ++r) {
        for (int e = lane; e < k; e += 64) { ms[k + e] = part_score[r * k + e]; mp[k + e] = part_key[r * k + e]; }
        __builtin_amdgcn_wave_barrier();
        float s[NI];
        int32_t p[NI];
        int rk[NI];
        ivf_rank<NI>(ms, mp, 2 * k, lane, s, p, rk);
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int i = 0; i < NI; ++i)
            if (lane + 64 * i < 2 * k && rk[i] < k) { ms[rk[i]] = s[i]; mp[rk[i]] = p[i]; }
        __builtin_amdgcn_wave_barrier();
    }
    __builtin_amdgcn_wave_barrier();
    int real = 0;
    for (int e = lane; e < k; e += 64) {
        const int32_t key = mp[e];
        real += key != INT_MAX ? 1 : 0;
        out_index[q * k + e] = key != INT_MAX ? key : -1;
        if (out_score) out_score[q * k + e] = ms[e];
    }
    int cand = 0;
    if (out_cand)
        for (int j = lane; j < nprobe; j += 64) {
            const int32_t c = probe[q * nprobe + j];
            cand += off[c + 1] - off[c];
        }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) { real += __shfl_xor(real, m, 64); cand += __shfl_xor(cand, m, 64); }
    if (lane == 0) {
        if (out_count) out_count[q] = real;
        if (out_cand) out_cand[q] = cand - minus_self;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The small kernels of the build and of the schedule: no atomics, every value a function of the sorted keys alone.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ivf_iota(int32_t *__restrict__ v, int64_t n) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p < n) v[p] = (int32_t)p;
}

__device__ __forceinline__ int64_t ivf_lower_bound(const uint32_t *keys, int64_t n, uint32_t c) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (keys[mid] < c) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// thread c <= L: start[c] = where key c begins among n sorted keys (start[L] = n)
__global__ __launch_bounds__(256) void k_ivf_bounds(const uint32_t *__restrict__ keys, int64_t n, int32_t L, int32_t *__restrict__ start) {
    const int c = (int)(blockIdx.x * 256 + threadIdx.x);
    if (c > L) return;
    start[c] = (int32_t)(c < L ? ivf_lower_bound(keys, n, (uint32_t)c) : n);
}

// thread c <= L: items[c] = query tiles * chunks of list c (items[L] = 0, so the scan's last entry is the total)
__global__ __launch_bounds__(256) void k_ivf_items(const int32_t *__restrict__ pstart, const int32_t *__restrict__ off, int32_t L, int32_t chunk_len,
                                                   uint32_t *__restrict__ items) {
    const int c = (int)(blockIdx.x * 256 + threadIdx.x);
    if (c > L) return;
    if (c == L) { items[c] = 0; return; }
    const int32_t pairs = pstart[c + 1] - pstart[c], len = off[c + 1] - off[c];
    items[c] = (uint32_t)((pairs + IV_TQ - 1) / IV_TQ) * (uint32_t)((len + chunk_len - 1) / chunk_len);
}

// thread e <= npairs: slots[e] = chunks of the list pair e probes (slots[npairs] = 0)
__global__ __launch_bounds__(256) void k_ivf_pair_slots(const int32_t *__restrict__ probe, const int32_t *__restrict__ off, int64_t npairs, int32_t chunk_len,
                                                        uint32_t *__restrict__ slots) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e > npairs) return;
    if (e == npairs) { slots[e] = 0; return; }
    const int32_t c = probe[e];
    slots[e] = (uint32_t)((off[c + 1] - off[c] + chunk_len - 1) / chunk_len);
}

// table[slot] = prep[pos[slot]], key[slot] = the original id of position pos[slot]; one thread per 16 bytes
__global__ __launch_bounds__(256) void k_ivf_gather(const float *__restrict__ prep, const int32_t *__restrict__ pos, const int32_t *__restrict__ ids, int64_t n,
                                                    int32_t D4, float *__restrict__ table, int32_t *__restrict__ key) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int32_t per = D4 / 4;
    if (idx >= n * per) return;
    const int64_t slot = idx / per;
    const int32_t piece = (int32_t)(idx - slot * per);
    const int32_t p = pos[slot];
    reinterpret_cast<f32x4 *>(table + slot * D4)[piece] = reinterpret_cast<const f32x4 *>(prep + (int64_t)p * D4)[piece];
    if (piece == 0) key[slot] = ids ? ids[p] : p;
}

struct DeviceBuffers {                      // freed on every way out
    std::vector<void *> ptrs;
    std::vector<hipEvent_t> evs;
    ~DeviceBuffers() { for (void *q : ptrs) (void)hipFree(q); for (hipEvent_t e : evs) (void)hipEventDestroy(e); }
    ge_status alloc(void **q, size_t bytes) { GE_HIP(hipMalloc(q, std::max<size_t>(bytes, 16))); ptrs.push_back(*q); return GE_OK; }
    ge_status event(hipEvent_t *e) { GE_HIP(hipEventCreate(e)); evs.push_back(*e); return GE_OK; }
};

}  // namespace

struct ge_ivf {
    int32_t device = 0, dim = 0, d4 = 0, lists = 0, train_steps = 0, converged = 0;
    int64_t n_rows = 0, n = 0;
    hipStream_t stream = nullptr;
    std::vector<int32_t> subset;            // original row id of every indexed row; empty = all rows
    std::vector<int32_t> label, slot_of;    // by position: the list, and the row of the table
    std::vector<int32_t> off;               // [lists + 1]
    std::vector<int32_t> top_chunks;        // the chunk counts of the lists, descending, the first IVF_MAX_PROBE of them
    DeviceBuffers B;                        // the four below live here
    float *dx = nullptr, *dcen = nullptr;   // [n][d4] in list order; [lists][d4]
    int32_t *dkey = nullptr, *doff = nullptr;
    mutable float build_ms = 0, probe_ms = 0, scan_ms = 0, merge_ms = 0;
};

namespace {

bool all_finite(const float *v, int64_t count) {
    for (int64_t i = 0; i < count; ++i)
        if (!(std::fabs(v[i]) <= 3.402823466e38f)) return false;
    return true;
}

ge_status check_create(int64_t n_rows, int32_t dim, const int32_t *subset, int64_t n_subset, const ge_ivf_cfg *cfg) {
    if (!cfg) return ge::fail(GE_ERR_ARG, "ge_ivf_cfg is null");
    if (cfg->metric == GE_NN_DOT) return ge::fail(GE_ERR_ARG, "ivf: no quantiser for dot");
    if (cfg->metric != GE_NN_COSINE) return ge::fail(GE_ERR_ARG, "ivf: unknown metric %d", cfg->metric);
    if (dim < 1 || dim > IVF_MAX_DIM) return ge::fail(GE_ERR_ARG, "ivf: dim %d outside [1, %d]", dim, IVF_MAX_DIM);
    if (n_rows < 1 || n_rows >= INT_MAX) return ge::fail(GE_ERR_ARG, "ivf: %lld rows outside [1, 2^31 - 2]", (long long)n_rows);
    if (n_rows > IVF_MAX_FLOATS / dim)
        return ge::fail(GE_ERR_ARG, "ivf: %lld rows of %d floats are more than one index holds (%lld floats)", (long long)n_rows, dim, (long long)IVF_MAX_FLOATS);
    if (subset) {
        if (n_subset < 1 || n_subset > n_rows) return ge::fail(GE_ERR_ARG, "ivf: a subset of %lld of %lld rows", (long long)n_subset, (long long)n_rows);
        for (int64_t i = 0; i < n_subset; ++i) {
            if (subset[i] < 0 || subset[i] >= n_rows) return ge::fail(GE_ERR_ARG, "ivf: subset[%lld] = %d outside [0, %lld)", (long long)i, subset[i], (long long)n_rows);
            if (i > 0 && subset[i] <= subset[i - 1]) return ge::fail(GE_ERR_ARG, "ivf: the subset is not strictly ascending at [%lld]", (long long)i);
        }
    }
    const int64_t n = subset ? n_subset : n_rows;
    if (cfg->lists < 1 || cfg->lists > IVF_MAX_LISTS) return ge::fail(GE_ERR_ARG, "ivf: %d lists outside [1, %d]", cfg->lists, IVF_MAX_LISTS);
    if (cfg->lists > n) return ge::fail(GE_ERR_ARG, "ivf: %d lists exceed the %lld indexed rows", cfg->lists, (long long)n);
    if (!cfg->centroids && (cfg->train_iterations < 0 || cfg->train_iterations > IVF_MAX_ITER))
        return ge::fail(GE_ERR_ARG, "ivf: train_iterations %d outside [0, %d]", cfg->train_iterations, IVF_MAX_ITER);
    return GE_OK;
}

// rows (host: slab by slab; dev: in place) -> table[rows_out][d4], prepared; *ms_out += the kernel's time
ge_status prepare_rows(const float *host, const float *dev, const int32_t *host_map, const int32_t *dev_map, int64_t rows_out, int32_t dim,
                       float *table, hipStream_t stream, const char *what, float *ms_out) {
    const int D = dim, D4 = (D + 3) / 4 * 4;
    const int64_t slab_rows = std::min<int64_t>(std::max<int64_t>(PREP_ROWS, IVF_SLAB_FLOATS / D / PREP_ROWS * PREP_ROWS), rows_out);
    DeviceBuffers B;
    float *dslab = nullptr;
    int32_t *dflag = nullptr;
    hipEvent_t e0, e1;
    GE_CHECK(B.event(&e0));
    GE_CHECK(B.event(&e1));
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
        GE_HIP(hipEventRecord(e0, stream));
        hipLaunchKernelGGL(k_ivf_prepare, dim3((unsigned)((rows + PREP_ROWS - 1) / PREP_ROWS)), dim3(64), 0, stream, x, map, rows, D, D4, table + begin * D4, dflag);
        GE_HIP(hipGetLastError());
        GE_HIP(hipEventRecord(e1, stream));
        GE_HIP(hipStreamSynchronize(stream));                                       // the slab buffer (and `packed`) are free again
        float ms = 0;
        GE_HIP(hipEventElapsedTime(&ms, e0, e1));
        total += ms;
    }
    int32_t flag = 0;
    GE_HIP(hipMemcpyAsync(&flag, dflag, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    GE_HIP(hipStreamSynchronize(stream));
    if (flag) return ge::fail(GE_ERR_ARG, "ivf: non-finite input (%s)", what);
    *ms_out += total;
    return GE_OK;
}

ge_status launch_scan(int cap, unsigned items, hipStream_t stream, const IvfWork &W, const float *Q, const int32_t *qrow, const int32_t *qself, const float *X,
                      const int32_t *keys, int32_t D4, int32_t k, int32_t *pkey, float *pscore) {
    const dim3 grid(items), block(256);
    switch (cap) {
    case 32: hipLaunchKernelGGL(k_ivf_scan<32>, grid, block, 0, stream, W, Q, qrow, qself, X, keys, D4, k, pkey, pscore); break;
    case 64: hipLaunchKernelGGL(k_ivf_scan<64>, grid, block, 0, stream, W, Q, qrow, qself, X, keys, D4, k, pkey, pscore); break;
    case 128: hipLaunchKernelGGL(k_ivf_scan<128>, grid, block, 0, stream, W, Q, qrow, qself, X, keys, D4, k, pkey, pscore); break;
    default: hipLaunchKernelGGL(k_ivf_scan<256>, grid, block, 0, stream, W, Q, qrow, qself, X, keys, D4, k, pkey, pscore); break;
    }
    GE_HIP(hipGetLastError());
    return GE_OK;
}

int32_t probe_chunks(int32_t lists) { return (lists + IVF_PROBE_CHUNK - 1) / IVF_PROBE_CHUNK; }

// the first k centroids of nq queries (rows qrow[.] of Q, or rows 0 .. nq - 1): the scan on the dense schedule, then the merge.
// pkey / pscore hold nq * probe_chunks(L) * k entries.
ge_status dense_topk(hipStream_t stream, const float *Q, const int32_t *qrow, int64_t nq, const float *cen, int32_t L, int32_t D4, int32_t k, int32_t *pkey,
                     float *pscore, int32_t *out_index) {
    IvfWork W = {};
    W.nq = nq; W.n_cand = L; W.chunks = probe_chunks(L); W.chunk_len = IVF_PROBE_CHUNK;
    const int64_t items = (nq + IV_TQ - 1) / IV_TQ * W.chunks;
    GE_CHECK(launch_scan(ivf_cap_of(k), (unsigned)items, stream, W, Q, qrow, nullptr, cen, nullptr, D4, k, pkey, pscore));
    hipLaunchKernelGGL(k_ivf_merge, dim3((unsigned)nq), dim3(64), 0, stream, (const int32_t *)pkey, (const float *)pscore, (const uint32_t *)nullptr, W.chunks, 0,
                       k, out_index, (float *)nullptr, (int32_t *)nullptr, (const int32_t *)nullptr, (const int32_t *)nullptr, 0, (int32_t *)nullptr);
    GE_HIP(hipGetLastError());
    return GE_OK;
}

struct KmeansGuard {
    ge_kmeans *km = nullptr;
    ~KmeansGuard() { if (km) ge_kmeans_destroy(km); }
};

// host rows, or the vectors of a trainer handle (h) which `dev` holds on the device
ge_status create_impl(const float *host, const float *dev, ge_glove *h, int64_t n_rows, int32_t dim, const int32_t *subset, int64_t n_subset,
                      const ge_ivf_cfg *cfg, ge_ivf **out) {
    std::unique_ptr<ge_ivf> p(new ge_ivf);
    p->device = cfg->device; p->stream = (hipStream_t)cfg->stream; p->lists = cfg->lists;
    p->dim = dim; p->d4 = (dim + 3) / 4 * 4; p->n_rows = n_rows; p->n = subset ? n_subset : n_rows;
    if (subset) p->subset.assign(subset, subset + n_subset);
    hipStream_t stream = p->stream;
    const size_t N = (size_t)p->n, L = (size_t)p->lists, D4 = (size_t)p->d4;

    // the centroids first: a training run holds its own copy of the rows, gone before the index allocates
    std::vector<float> trained;
    if (!cfg->centroids) {
        ge_kmeans_cfg kc;
        ge_kmeans_cfg_default(&kc);
        kc.metric = GE_KM_COSINE; kc.k = cfg->lists; kc.seed = cfg->seed; kc.device = cfg->device; kc.stream = cfg->stream;
        KmeansGuard G;
        GE_CHECK(host ? ge_kmeans_create(host, n_rows, dim, subset, n_subset, &kc, &G.km) : ge_glove_kmeans_create(h, subset, n_subset, &kc, &G.km));
        if (cfg->train_iterations > 0) GE_CHECK(ge_kmeans_run(G.km, cfg->train_iterations, &p->train_steps, &p->converged));
        trained.resize(L * (size_t)dim);
        GE_CHECK(ge_kmeans_get(G.km, nullptr, nullptr, nullptr, nullptr, nullptr, trained.data(), nullptr, nullptr, nullptr, nullptr, nullptr));
    }
    GE_CHECK(ge::select_device(p->device));

    DeviceBuffers &B = p->B;
    DeviceBuffers T;                                                               // what only the build needs
    hipEvent_t e0, e1;
    GE_CHECK(T.event(&e0));
    GE_CHECK(T.event(&e1));
    float *dprep = nullptr, *dps = nullptr;
    int32_t *dsub = nullptr, *dlabel = nullptr, *diota = nullptr, *dpos = nullptr, *dpk = nullptr;
    uint32_t *dsorted = nullptr;
    void *dtmp = nullptr;
    GE_CHECK(B.alloc((void **)&p->dx, sizeof(float) * N * D4));
    GE_CHECK(B.alloc((void **)&p->dkey, sizeof(int32_t) * N));
    GE_CHECK(B.alloc((void **)&p->doff, sizeof(int32_t) * (L + 1)));
    GE_CHECK(B.alloc((void **)&p->dcen, sizeof(float) * L * D4));
    GE_CHECK(T.alloc((void **)&dprep, sizeof(float) * N * D4));
    if (subset) {
        GE_CHECK(T.alloc((void **)&dsub, sizeof(int32_t) * N));
        GE_HIP(hipMemcpyAsync(dsub, subset, sizeof(int32_t) * N, hipMemcpyHostToDevice, stream));
    }
    GE_CHECK(prepare_rows(host, dev, subset, dsub, p->n, dim, dprep, stream, "rows", &p->build_ms));
    if (cfg->centroids) {
        GE_CHECK(prepare_rows(cfg->centroids, nullptr, nullptr, nullptr, p->lists, dim, p->dcen, stream, "centroids", &p->build_ms));
    } else {
        GE_HIP(hipMemsetAsync(p->dcen, 0, sizeof(float) * L * D4, stream));        // the padding columns
        GE_HIP(hipMemcpy2DAsync(p->dcen, sizeof(float) * D4, trained.data(), sizeof(float) * (size_t)dim, sizeof(float) * (size_t)dim, L, hipMemcpyHostToDevice,
                                stream));
        GE_HIP(hipStreamSynchronize(stream));
    }

    // everything the kernels below need is allocated first, so that the events hold kernels only
    const int32_t pch = probe_chunks(p->lists);
    const int64_t batch = std::max<int64_t>(IV_TQ, std::min<int64_t>(p->n, IVF_BATCH_ENTRIES / pch / IV_TQ * IV_TQ));
    GE_CHECK(T.alloc((void **)&dlabel, sizeof(int32_t) * N));
    GE_CHECK(T.alloc((void **)&dpk, sizeof(int32_t) * (size_t)(batch * pch)));
    GE_CHECK(T.alloc((void **)&dps, sizeof(float) * (size_t)(batch * pch)));
    GE_CHECK(T.alloc((void **)&diota, sizeof(int32_t) * N));
    GE_CHECK(T.alloc((void **)&dpos, sizeof(int32_t) * N));
    GE_CHECK(T.alloc((void **)&dsorted, sizeof(uint32_t) * N));
    int bits = 1;
    while ((1 << bits) < p->lists) ++bits;
    size_t tmp_bytes = 0;
    GE_HIP(rocprim::radix_sort_pairs(nullptr, tmp_bytes, (const uint32_t *)dlabel, dsorted, (const int32_t *)diota, dpos, N, 0, (unsigned)bits, stream));
    GE_CHECK(T.alloc(&dtmp, tmp_bytes));

    // assign: the first centroid of every row, batch by batch
    GE_HIP(hipEventRecord(e0, stream));
    for (int64_t begin = 0; begin < p->n; begin += batch) {
        const int64_t nq = std::min(batch, p->n - begin);
        GE_CHECK(dense_topk(stream, dprep + begin * D4, nullptr, nq, p->dcen, p->lists, p->d4, 1, dpk, dps, dlabel + begin));
    }

    // the lists: positions stably sorted by label, where every label begins, and the table gathered in that order
    hipLaunchKernelGGL(k_ivf_iota, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, stream, diota, p->n);
    GE_HIP(hipGetLastError());
    GE_HIP(rocprim::radix_sort_pairs(dtmp, tmp_bytes, (const uint32_t *)dlabel, dsorted, (const int32_t *)diota, dpos, N, 0, (unsigned)bits, stream));
    hipLaunchKernelGGL(k_ivf_bounds, dim3((unsigned)((L + 1 + 255) / 256)), dim3(256), 0, stream, (const uint32_t *)dsorted, p->n, p->lists, p->doff);
    GE_HIP(hipGetLastError());
    const int64_t pieces = p->n * (int64_t)(D4 / 4);
    hipLaunchKernelGGL(k_ivf_gather, dim3((unsigned)((pieces + 255) / 256)), dim3(256), 0, stream, (const float *)dprep, (const int32_t *)dpos,
                       (const int32_t *)dsub, p->n, p->d4, p->dx, p->dkey);
    GE_HIP(hipGetLastError());
    GE_HIP(hipEventRecord(e1, stream));

    // what the host keeps: labels, offsets, and where every position went
    p->label.resize(N); p->slot_of.resize(N); p->off.resize(L + 1);
    std::vector<int32_t> pos(N);
    GE_HIP(hipMemcpyAsync(p->label.data(), dlabel, sizeof(int32_t) * N, hipMemcpyDeviceToHost, stream));
    GE_HIP(hipMemcpyAsync(pos.data(), dpos, sizeof(int32_t) * N, hipMemcpyDeviceToHost, stream));
    GE_HIP(hipMemcpyAsync(p->off.data(), p->doff, sizeof(int32_t) * (L + 1), hipMemcpyDeviceToHost, stream));
    GE_HIP(hipStreamSynchronize(stream));
    float ms = 0;
    GE_HIP(hipEventElapsedTime(&ms, e0, e1));
    p->build_ms += ms;
    for (size_t s = 0; s < N; ++s) p->slot_of[(size_t)pos[s]] = (int32_t)s;
    std::vector<int32_t> chunks(L);
    for (size_t c = 0; c < L; ++c) chunks[c] = (p->off[c + 1] - p->off[c] + IVF_CHUNK - 1) / IVF_CHUNK;
    const size_t top = std::min<size_t>(L, IVF_MAX_PROBE);
    std::partial_sort(chunks.begin(), chunks.begin() + top, chunks.end(), std::greater<int32_t>());
    p->top_chunks.assign(chunks.begin(), chunks.begin() + top);
    *out = p.release();
    return GE_OK;
}

ge_status ivf_create_host(const float *rows, int64_t n_rows, int32_t dim, const int32_t *subset, int64_t n_subset, const ge_ivf_cfg *cfg, ge_ivf **out) {
    if (out) *out = nullptr;
    if (!rows || !out) return ge::fail(GE_ERR_ARG, "ge_ivf_create: rows or out is null");
    GE_CHECK(check_create(n_rows, dim, subset, n_subset, cfg));
    if (subset) {
        for (int64_t i = 0; i < n_subset; ++i)
            if (!all_finite(rows + (int64_t)subset[i] * dim, dim)) return ge::fail(GE_ERR_ARG, "ivf: non-finite input (rows)");
    } else if (!all_finite(rows, n_rows * dim)) {
        return ge::fail(GE_ERR_ARG, "ivf: non-finite input (rows)");
    }
    if (cfg->centroids && !all_finite(cfg->centroids, (int64_t)cfg->lists * dim)) return ge::fail(GE_ERR_ARG, "ivf: non-finite input (centroids)");
    GE_CHECK(ge::select_device(cfg->device));
    return create_impl(rows, nullptr, nullptr, n_rows, dim, subset, n_subset, cfg, out);
}

ge_status ivf_create_glove(ge_glove *h, const int32_t *subset, int64_t n_subset, const ge_ivf_cfg *cfg, ge_ivf **out) {
    if (out) *out = nullptr;
    if (!h || !out) return ge::fail(GE_ERR_ARG, "ge_glove_ivf_create: handle or out is null");
    if (!cfg) return ge::fail(GE_ERR_ARG, "ge_ivf_cfg is null");
    if (cfg->metric == GE_NN_DOT) return ge::fail(GE_ERR_ARG, "ivf: no quantiser for dot");
    if (cfg->metric != GE_NN_COSINE) return ge::fail(GE_ERR_ARG, "ivf: unknown metric %d", cfg->metric);
    if (cfg->lists < 1 || cfg->lists > IVF_MAX_LISTS) return ge::fail(GE_ERR_ARG, "ivf: %d lists outside [1, %d]", cfg->lists, IVF_MAX_LISTS);
    float *d = nullptr;
    int32_t V = 0, D = 0, device = 0;
    GE_CHECK(ge::glove_extract_device_f32(h, &d, &V, &D, &device));   // a fresh buffer: no trainer table is written
    ge_ivf_cfg own = *cfg;
    own.device = device;                                              // the rows live on the handle's device
    ge_status st = check_create(V, D, subset, n_subset, &own);
    if (st == GE_OK && own.centroids && !all_finite(own.centroids, (int64_t)own.lists * D)) st = ge::fail(GE_ERR_ARG, "ivf: non-finite input (centroids)");
    if (st == GE_OK) st = create_impl(nullptr, d, h, V, D, subset, n_subset, &own, out);
    (void)hipFree(d);
    return st;
}

// queries: positions in the index (qpos) or values (vectors)
ge_status query_impl(ge_ivf *p, const int32_t *qpos, const float *vectors, int64_t n_queries, int32_t k, int32_t nprobe, int32_t exclude_self,
                     int32_t *out_index, float *out_score, int32_t *out_count, int32_t *out_cand) {
    hipStream_t stream = p->stream;
    const int D4 = p->d4, L = p->lists;
    const int32_t pch = probe_chunks(L);
    int64_t slots_per_q = 0;                                           // no query of this index owns more partial slots
    for (int j = 0; j < nprobe; ++j) slots_per_q += p->top_chunks[(size_t)j];
    const int64_t per_q = std::max<int64_t>(std::max<int64_t>(slots_per_q * k, (int64_t)pch * nprobe), 1);
    const int64_t batch = std::max<int64_t>(IV_TQ, std::min<int64_t>(n_queries, IVF_BATCH_ENTRIES / per_q / IV_TQ * IV_TQ));
    const int64_t nb = std::min(batch, n_queries);
    const int64_t max_pairs = nb * nprobe;

    DeviceBuffers B;
    hipEvent_t ev[5];
    for (hipEvent_t &e : ev) GE_CHECK(B.event(&e));
    float *dq = nullptr, *dps = nullptr, *dos = nullptr;
    int32_t *dqrow = nullptr, *dqself = nullptr, *dpk = nullptr, *dprobe = nullptr, *diota = nullptr, *dpairs = nullptr, *dpstart = nullptr, *doi = nullptr,
            *dcount = nullptr, *dcand = nullptr;
    uint32_t *dsorted = nullptr, *ditems = nullptr, *dfirst = nullptr, *dslots = nullptr, *dsbase = nullptr;
    void *dtmp = nullptr;
    if (vectors) GE_CHECK(B.alloc((void **)&dq, sizeof(float) * (size_t)nb * D4));
    if (qpos) GE_CHECK(B.alloc((void **)&dqrow, sizeof(int32_t) * (size_t)nb));
    if (qpos && exclude_self) GE_CHECK(B.alloc((void **)&dqself, sizeof(int32_t) * (size_t)nb));
    GE_CHECK(B.alloc((void **)&dpk, sizeof(int32_t) * (size_t)(nb * per_q)));
    GE_CHECK(B.alloc((void **)&dps, sizeof(float) * (size_t)(nb * per_q)));
    GE_CHECK(B.alloc((void **)&dprobe, sizeof(int32_t) * (size_t)max_pairs));
    GE_CHECK(B.alloc((void **)&diota, sizeof(int32_t) * (size_t)max_pairs));
    GE_CHECK(B.alloc((void **)&dpairs, sizeof(int32_t) * (size_t)max_pairs));
    GE_CHECK(B.alloc((void **)&dsorted, sizeof(uint32_t) * (size_t)max_pairs));
    GE_CHECK(B.alloc((void **)&dslots, sizeof(uint32_t) * (size_t)(max_pairs + 1)));
    GE_CHECK(B.alloc((void **)&dsbase, sizeof(uint32_t) * (size_t)(max_pairs + 1)));
    GE_CHECK(B.alloc((void **)&dpstart, sizeof(int32_t) * (size_t)(L + 1)));
    GE_CHECK(B.alloc((void **)&ditems, sizeof(uint32_t) * (size_t)(L + 1)));
    GE_CHECK(B.alloc((void **)&dfirst, sizeof(uint32_t) * (size_t)(L + 1)));
    GE_CHECK(B.alloc((void **)&doi, sizeof(int32_t) * (size_t)(nb * k)));
    GE_CHECK(B.alloc((void **)&dos, sizeof(float) * (size_t)(nb * k)));
    GE_CHECK(B.alloc((void **)&dcount, sizeof(int32_t) * (size_t)nb));
    GE_CHECK(B.alloc((void **)&dcand, sizeof(int32_t) * (size_t)nb));
    int bits = 1;
    while ((1 << bits) < L) ++bits;
    size_t sort_bytes = 0, scan_a = 0, scan_b = 0;
    GE_HIP(rocprim::radix_sort_pairs(nullptr, sort_bytes, (const uint32_t *)dprobe, dsorted, (const int32_t *)diota, dpairs, (size_t)max_pairs, 0, (unsigned)bits,
                                     stream));
    GE_HIP(rocprim::exclusive_scan(nullptr, scan_a, (const uint32_t *)ditems, dfirst, 0u, (size_t)L + 1, rocprim::plus<uint32_t>(), stream));
    GE_HIP(rocprim::exclusive_scan(nullptr, scan_b, (const uint32_t *)dslots, dsbase, 0u, (size_t)max_pairs + 1, rocprim::plus<uint32_t>(), stream));
    const int64_t last_pairs = (n_queries - (n_queries - 1) / batch * batch) * nprobe;      // the last batch may be shorter: its scratch too
    size_t sort_last = 0, scan_last = 0;
    GE_HIP(rocprim::radix_sort_pairs(nullptr, sort_last, (const uint32_t *)dprobe, dsorted, (const int32_t *)diota, dpairs, (size_t)last_pairs, 0, (unsigned)bits,
                                     stream));
    GE_HIP(rocprim::exclusive_scan(nullptr, scan_last, (const uint32_t *)dslots, dsbase, 0u, (size_t)last_pairs + 1, rocprim::plus<uint32_t>(), stream));
    sort_bytes = std::max(sort_bytes, sort_last);
    scan_b = std::max(scan_b, scan_last);
    GE_CHECK(B.alloc(&dtmp, std::max(sort_bytes, std::max(scan_a, scan_b))));
    hipLaunchKernelGGL(k_ivf_iota, dim3((unsigned)((max_pairs + 255) / 256)), dim3(256), 0, stream, diota, max_pairs);
    GE_HIP(hipGetLastError());

    std::vector<int32_t> hrow, hself;
    float probe_ms = 0, scan_ms = 0, merge_ms = 0;
    for (int64_t begin = 0; begin < n_queries; begin += batch) {
        const int64_t nq = std::min(batch, n_queries - begin);
        const int64_t npairs = nq * nprobe;
        const float *Q = p->dx;
        if (vectors) {
            GE_CHECK(prepare_rows(vectors + begin * p->dim, nullptr, nullptr, nullptr, nq, p->dim, dq, stream, "query vectors", &probe_ms));
            Q = dq;
        } else {
            hrow.resize((size_t)nq);
            for (int64_t i = 0; i < nq; ++i) hrow[(size_t)i] = p->slot_of[(size_t)qpos[begin + i]];
            GE_HIP(hipMemcpyAsync(dqrow, hrow.data(), sizeof(int32_t) * (size_t)nq, hipMemcpyHostToDevice, stream));
            if (exclude_self) {
                hself.resize((size_t)nq);
                for (int64_t i = 0; i < nq; ++i) hself[(size_t)i] = p->subset.empty() ? qpos[begin + i] : p->subset[(size_t)qpos[begin + i]];
                GE_HIP(hipMemcpyAsync(dqself, hself.data(), sizeof(int32_t) * (size_t)nq, hipMemcpyHostToDevice, stream));
            }
        }
        // probe: the first nprobe centroids of every query, then the pairs sorted by list and the schedule
        GE_HIP(hipEventRecord(ev[0], stream));
        GE_CHECK(dense_topk(stream, Q, dqrow, nq, p->dcen, L, D4, nprobe, dpk, dps, dprobe));
        GE_HIP(rocprim::radix_sort_pairs(dtmp, sort_bytes, (const uint32_t *)dprobe, dsorted, (const int32_t *)diota, dpairs, (size_t)npairs, 0, (unsigned)bits,
                                         stream));
        hipLaunchKernelGGL(k_ivf_bounds, dim3((unsigned)((L + 1 + 255) / 256)), dim3(256), 0, stream, (const uint32_t *)dsorted, npairs, L, dpstart);
        GE_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_ivf_items, dim3((unsigned)((L + 1 + 255) / 256)), dim3(256), 0, stream, (const int32_t *)dpstart, (const int32_t *)p->doff, L,
                           IVF_CHUNK, ditems);
        GE_HIP(hipGetLastError());
        GE_HIP(rocprim::exclusive_scan(dtmp, scan_a, (const uint32_t *)ditems, dfirst, 0u, (size_t)L + 1, rocprim::plus<uint32_t>(), stream));
        hipLaunchKernelGGL(k_ivf_pair_slots, dim3((unsigned)((npairs + 1 + 255) / 256)), dim3(256), 0, stream, (const int32_t *)dprobe, (const int32_t *)p->doff,
                           npairs, IVF_CHUNK, dslots);
        GE_HIP(hipGetLastError());
        GE_HIP(rocprim::exclusive_scan(dtmp, scan_b, (const uint32_t *)dslots, dsbase, 0u, (size_t)npairs + 1, rocprim::plus<uint32_t>(), stream));
        GE_HIP(hipEventRecord(ev[1], stream));
        uint32_t items = 0, slots = 0;
        GE_HIP(hipMemcpyAsync(&items, dfirst + L, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        GE_HIP(hipMemcpyAsync(&slots, dsbase + npairs, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        GE_HIP(hipStreamSynchronize(stream));
        if ((int64_t)slots * k > nb * per_q) return ge::fail(GE_ERR_STATE, "ivf: %u partial slots of %d entries do not fit the batch's %lld", slots, k, (long long)(nb * per_q));

        GE_HIP(hipEventRecord(ev[2], stream));
        if (items > 0) {
            IvfWork W = {};
            W.chunk_len = IVF_CHUNK; W.pairs = dpairs; W.pstart = dpstart; W.off = p->doff; W.first = dfirst; W.sbase = dsbase; W.lists = L; W.nprobe = nprobe;
            GE_CHECK(launch_scan(ivf_cap_of(k), items, stream, W, Q, vectors ? nullptr : dqrow, exclude_self ? dqself : nullptr, p->dx, p->dkey, D4, k, dpk, dps));
        }
        GE_HIP(hipEventRecord(ev[3], stream));
        hipLaunchKernelGGL(k_ivf_merge, dim3((unsigned)nq), dim3(64), 0, stream, (const int32_t *)dpk, (const float *)dps, (const uint32_t *)dsbase, 0, nprobe, k, doi,
                           dos, dcount, (const int32_t *)dprobe, (const int32_t *)p->doff, exclude_self ? 1 : 0, dcand);
        GE_HIP(hipGetLastError());
        GE_HIP(hipEventRecord(ev[4], stream));
        if (out_index) GE_HIP(hipMemcpyAsync(out_index + begin * k, doi, sizeof(int32_t) * (size_t)(nq * k), hipMemcpyDeviceToHost, stream));
        if (out_score) GE_HIP(hipMemcpyAsync(out_score + begin * k, dos, sizeof(float) * (size_t)(nq * k), hipMemcpyDeviceToHost, stream));
        if (out_count) GE_HIP(hipMemcpyAsync(out_count + begin, dcount, sizeof(int32_t) * (size_t)nq, hipMemcpyDeviceToHost, stream));
        if (out_cand) GE_HIP(hipMemcpyAsync(out_cand + begin, dcand, sizeof(int32_t) * (size_t)nq, hipMemcpyDeviceToHost, stream));
        GE_HIP(hipStreamSynchronize(stream));
        float a = 0, b = 0, c = 0;
        GE_HIP(hipEventElapsedTime(&a, ev[0], ev[1]));
        GE_HIP(hipEventElapsedTime(&b, ev[2], ev[3]));
        GE_HIP(hipEventElapsedTime(&c, ev[3], ev[4]));
        probe_ms += a; scan_ms += b; merge_ms += c;
    }
    p->probe_ms = probe_ms; p->scan_ms = scan_ms; p->merge_ms = merge_ms;
    return GE_OK;
}

ge_status check_query(const ge_ivf *p, int64_t n_queries, int32_t k, int32_t nprobe, const char *fn) {
    if (!p) return ge::fail(GE_ERR_ARG, "null ge_ivf handle");
    if (n_queries < 1) return ge::fail(GE_ERR_ARG, "%s: %lld queries", fn, (long long)n_queries);
    if (k < 1 || k > IVF_MAX_K) return ge::fail(GE_ERR_ARG, "ivf: k %d outside [1, %d]", k, IVF_MAX_K);
    if (nprobe < 1 || nprobe > std::min(p->lists, IVF_MAX_PROBE))
        return ge::fail(GE_ERR_ARG, "ivf: nprobe %d outside [1, %d]", nprobe, std::min(p->lists, IVF_MAX_PROBE));
    return GE_OK;
}

ge_status ivf_query_rows(ge_ivf *p, const int32_t *query_ids, int64_t n_queries, int32_t k, int32_t nprobe, int32_t exclude_self, int32_t *out_index,
                         float *out_score, int32_t *out_count, int32_t *out_cand) {
    if (p && !query_ids && n_queries != p->n)
        return ge::fail(GE_ERR_ARG, "ge_ivf_query_rows: query_ids is null, so n_queries must be the %lld indexed rows, not %lld", (long long)p->n,
                        (long long)n_queries);
    GE_CHECK(check_query(p, n_queries, k, nprobe, "ge_ivf_query_rows"));
    std::vector<int32_t> pos((size_t)n_queries);
    for (int64_t i = 0; i < n_queries; ++i) {
        int64_t at = i;
        if (query_ids) {
            const int32_t id = query_ids[i];
            at = -1;
            if (p->subset.empty()) at = id >= 0 && id < p->n_rows ? id : -1;
            else {
                const auto it = std::lower_bound(p->subset.begin(), p->subset.end(), id);
                if (it != p->subset.end() && *it == id) at = it - p->subset.begin();
            }
            if (at < 0) return ge::fail(GE_ERR_ARG, "ivf: query_ids[%lld] = %d is not a row of the index", (long long)i, id);
        }
        pos[(size_t)i] = (int32_t)at;
    }
    GE_CHECK(ge::select_device(p->device));
    return query_impl(p, pos.data(), nullptr, n_queries, k, nprobe, exclude_self ? 1 : 0, out_index, out_score, out_count, out_cand);
}

ge_status ivf_query_vectors(ge_ivf *p, const float *vectors, int64_t n_queries, int32_t k, int32_t nprobe, int32_t *out_index, float *out_score,
                            int32_t *out_count, int32_t *out_cand) {
    if (p && !vectors) return ge::fail(GE_ERR_ARG, "ge_ivf_query_vectors: vectors is null");
    GE_CHECK(check_query(p, n_queries, k, nprobe, "ge_ivf_query_vectors"));
    if (!all_finite(vectors, n_queries * p->dim)) return ge::fail(GE_ERR_ARG, "ivf: non-finite input (query vectors)");
    GE_CHECK(ge::select_device(p->device));
    return query_impl(p, nullptr, vectors, n_queries, k, nprobe, 0, out_index, out_score, out_count, out_cand);
}

ge_status ivf_get(const ge_ivf *p, int64_t *n, int32_t *dim, int32_t *lists, int32_t *labels, int32_t *sizes, float *centroids, int32_t *train_steps,
                  int32_t *converged) {
    if (!p) return ge::fail(GE_ERR_ARG, "null ge_ivf handle");
    if (n) *n = p->n;
    if (dim) *dim = p->dim;
    if (lists) *lists = p->lists;
    if (train_steps) *train_steps = p->train_steps;
    if (converged) *converged = p->converged;
    if (labels) std::memcpy(labels, p->label.data(), sizeof(int32_t) * (size_t)p->n);
    if (sizes)
        for (int32_t c = 0; c < p->lists; ++c) sizes[c] = p->off[(size_t)c + 1] - p->off[(size_t)c];
    if (centroids) {
        GE_CHECK(ge::select_device(p->device));
        GE_HIP(hipMemcpy2DAsync(centroids, sizeof(float) * (size_t)p->dim, p->dcen, sizeof(float) * (size_t)p->d4, sizeof(float) * (size_t)p->dim,
                                (size_t)p->lists, hipMemcpyDeviceToHost, p->stream));
        GE_HIP(hipStreamSynchronize(p->stream));
    }
    return GE_OK;
}

}  // namespace

extern "C" {

void ge_ivf_cfg_default(ge_ivf_cfg *cfg) {
    if (!cfg) return;
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->metric = GE_NN_COSINE;
    cfg->train_iterations = 10;
}
int32_t ge_ivf_cfg_size(void) { return (int32_t)sizeof(ge_ivf_cfg); }

ge_status ge_ivf_create(const float *rows, int64_t n_rows, int32_t dim, const int32_t *subset, int64_t n_subset, const ge_ivf_cfg *cfg, ge_ivf **out) {
    GE_GUARD(ivf_create_host(rows, n_rows, dim, subset, n_subset, cfg, out));
}
ge_status ge_glove_ivf_create(ge_glove *h, const int32_t *subset, int64_t n_subset, const ge_ivf_cfg *cfg, ge_ivf **out) {
    GE_GUARD(ivf_create_glove(h, subset, n_subset, cfg, out));
}
ge_status ge_ivf_query_rows(ge_ivf *p, const int32_t *query_ids, int64_t n_queries, int32_t k, int32_t nprobe, int32_t exclude_self, int32_t *out_index,
                            float *out_score, int32_t *out_count, int32_t *out_candidates) {
    GE_GUARD(ivf_query_rows(p, query_ids, n_queries, k, nprobe, exclude_self, out_index, out_score, out_count, out_candidates));
}
ge_status ge_ivf_query_vectors(ge_ivf *p, const float *vectors, int64_t n_queries, int32_t k, int32_t nprobe, int32_t *out_index, float *out_score,
                               int32_t *out_count, int32_t *out_candidates) {
    GE_GUARD(ivf_query_vectors(p, vectors, n_queries, k, nprobe, out_index, out_score, out_count, out_candidates));
}
ge_status ge_ivf_get(const ge_ivf *p, int64_t *n, int32_t *dim, int32_t *lists, int32_t *labels, int32_t *sizes, float *centroids, int32_t *train_steps,
                     int32_t *converged) {
    GE_GUARD(ivf_get(p, n, dim, lists, labels, sizes, centroids, train_steps, converged));
}

ge_status ge_ivf_last_kernel_ms(const ge_ivf *p, float *build_ms, float *probe_ms, float *scan_ms, float *merge_ms) {
    if (!p) return ge::fail(GE_ERR_ARG, "null ge_ivf handle");
    if (build_ms) *build_ms = p->build_ms;
    if (probe_ms) *probe_ms = p->probe_ms;
    if (scan_ms) *scan_ms = p->scan_ms;
    if (merge_ms) *merge_ms = p->merge_ms;
    return GE_OK;
}

void ge_ivf_destroy(ge_ivf *p) {
    if (!p) return;
    (void)hipSetDevice(p->device);
    delete p;
}

}  // extern "C"
