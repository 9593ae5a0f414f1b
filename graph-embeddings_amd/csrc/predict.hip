// predict.hip -- which columns does the model expect in a row?  ge_glove_predict_* (include/geglove.h, "Prediction"): the K best
// candidate columns of every query row under the score ge_glove_rank_* ranks by, z = focus[i] . context[c] + cBias[c], with the
// row's known positives (and optionally the row itself) left out and the candidates optionally confined to a subset.  A pure
// read of a trainer handle in whichever layout it has (ge_glove_internal.h EvalView).  Per run the query rows and the candidate
// rows are staged into dense fp32 tables (k_predict_stage), scored on the fp32 matrix cores with the selection in the same
// kernel (k_predict_select: the score tile and the per-query lists of nn.hip's k_nn_score_select, with the bias and a filter
// test in the epilogue), and the partial lists of the candidate ranges are merged in a fixed order (k_predict_merge).  The score
// tile gives the fmaf chain over ascending d bit for bit, so a prediction's score is the z ge_glove_rank_run reports for it and
// its place in the list is its rank.  The reference has no counterpart.
#include "ge_common.h"
#include "ge_glove_internal.h"
#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int PD_MAX_DIM = 1024, PD_MAX_K = 128;
constexpr int64_t PD_MAX_FILTER = (int64_t)1 << 35;          // filter entries of one set, as a rank set
constexpr int64_t PD_BATCH_ENTRIES = (int64_t)1 << 24;       // (query, range, slot) entries of partial lists per launch (128 MB of them)

// the order of the results, the total order of ge_nn_*: score descending as fp32 compares them, then position ascending, then
// (for the fill entries of short lists, which share one position) slot ascending
__device__ __forceinline__ bool pd_beats(float sa, int32_t pa, int ea, float sb, int32_t pb, int eb) {
    return sa > sb || (sa == sb && (pa < pb || (pa == pb && ea < eb)));
}
__device__ __forceinline__ bool pd_beats(float sa, int32_t pa, float sb, int32_t pb) { return sa > sb || (sa == sb && pa < pb); }

// ---------------------------------------------------------------------------------------------------------------------
// Stage.  out[r][D4] = row `rows[r] - row_begin` (rows null: r) of a handle's table, widened from bf16 when is16, taken from the
// fp32 master when hub_index says so, padded with zeros from D to D4; bias_out[r] = that row's bias (bias_out null: none).
// One element per thread: consecutive threads write consecutive floats.  With rows = the candidate subset the context table
// arrives in candidate positions.
// ---------------------------------------------------------------------------------------------------------------------
struct StageParams {
    const void *table; const float *hub32, *bias;
    const int32_t *hub_index, *rows;
    float *out, *bias_out;
    int64_t n_rows, stride, bias_stride;
    int32_t D, D4, row_begin, is16;
};

__global__ __launch_bounds__(256) void k_predict_stage(StageParams p) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= p.n_rows * p.D4) return;
    const int64_t r = idx / p.D4;
    const int d = (int)(idx - r * p.D4);
    const int64_t src = p.rows ? (int64_t)p.rows[r] - p.row_begin : r;
    float x = 0.0f;
    if (d < p.D) {
        const int32_t slot = p.hub_index ? p.hub_index[src] : -1;
        if (slot >= 0) x = p.hub32[(int64_t)slot * p.D + d];
        else if (p.is16) x = __uint_as_float((uint32_t) static_cast<const uint16_t *>(p.table)[src * p.stride + d] << 16);
        else x = static_cast<const float *>(p.table)[src * p.stride + d];
    }
    p.out[idx] = x;
    if (p.bias_out && d == 0) p.bias_out[r] = p.bias[src * p.bias_stride];
}

// ---------------------------------------------------------------------------------------------------------------------
// Score and select.  The tile of k_nn_score_select: a workgroup owns PD_TQ queries (blockIdx.x, the fast index: workgroups that
// read the same candidate panels run together) and one range of whole PD_TC-candidate tiles (blockIdx.y); per PD_DK columns the
// query and candidate panels are staged in LDS as [row][PD_LS] (the next panel travels in registers meanwhile; PD_LS = 34 = 2 mod
// 32 keeps the 32 lanes of a ds_read_b32 cycle on 32 banks), and wave w carries queries 16 w .. 16 w + 15 against the PD_TC
// candidates through v_mfma_f32_16x16x4_f32: eight accumulators, each bit for bit an fmaf chain over ascending d.
//
// Epilogue: z = chain + cb[candidate] in one fp32 add, NaN to -inf.  Every query of the tile has a list of CAP (z, position)
// entries, a fill count and a threshold -- its k-th best entry at the last compaction -- in LDS, private to the wave that owns
// the query.  A z that does not beat the threshold is dropped after one compare.  One that does is tested against the query's
// filter list and dropped when found there.  The test reads an LDS bitmask of 128 bits per query, one bit per candidate of the
// tile: every query keeps a cursor into its ascending list (positions, global memory; it starts at the first entry inside the
// range, found by one binary search) and the next entry's position; a tile that reaches that position has the wave walk the
// list on, 64 entries per read, setting bits until it leaves the tile.  Lists of any length; a tile without filter entries --
// nearly every tile of a sparse list -- costs one LDS compare.  Survivors take a slot with an LDS integer add; when a list is full
// the wave ranks its entries under the total order by counting, keeps the best k in rank order and moves the threshold.  Which
// slot a survivor lands in depends on timing, the ranks do not: positions are unique.  Whether a candidate is filtered does not
// depend on the threshold it met, so the kept set is the best k of the range's unfiltered candidates whatever the grid.
// The partial list of (query, range) goes out sorted, short ones filled with (-inf, INT_MAX).
// ---------------------------------------------------------------------------------------------------------------------
constexpr int PD_TQ = 64, PD_TC = 128, PD_DK = 32, PD_LS = 34;
constexpr int PD_LOADS = (PD_TQ + PD_TC) * (PD_DK / 4) / 256;   // 16-byte pieces a thread moves per panel: 2 of queries, 4 of candidates
constexpr int pd_cap_of(int k) { return k <= 16 ? 32 : k <= 32 ? 64 : k <= 64 ? 128 : 256; }

// ranks of the first m entries of a list, entry lane + 64 i in lane's slot i
template <int NI>
__device__ __forceinline__ void pd_rank(const float *ls, const int32_t *lp, int m, int lane, float (&s)[NI], int32_t (&p)[NI], int (&rk)[NI]) {
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
        for (int i = 0; i < NI; ++i) rk[i] += pd_beats(ts, tp, t, s[i], p[i], lane + 64 * i) ? 1 : 0;
    }
}

// the first entry of the ascending list fpos[lo, hi) that is not below c
__device__ __forceinline__ int64_t pd_lower_bound(const int32_t *__restrict__ fpos, int64_t lo, int64_t hi, int32_t c) {
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (fpos[mid] < c) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

struct SelectParams {
    const float *Q, *X, *cb;                 // staged: [nq][D4], [n][D4], [n]
    const int32_t *selfpos;                  // [nq]: the position a query must not return, or -1
    const int64_t *fptr;                     // [nq + 1] into fpos, or null: no filter
    const int32_t *fpos;                     // filter lists in candidate positions, ascending per list
    int32_t *part_pos; float *part_score;    // [nq][ranges][k]
    int64_t nq, n, range_len;
    int32_t D4, k;
};

template <int CAP>
__global__ __launch_bounds__(256, CAP <= 32 ? 3 : CAP <= 64 ? 2 : 1) void k_predict_select(SelectParams P) {
    constexpr int NI = CAP > 64 ? CAP / 64 : 1;
    __shared__ float sq[PD_TQ * PD_LS];
    __shared__ float sx[PD_TC * PD_LS];
    __shared__ float ls[PD_TQ * CAP];
    __shared__ int32_t lp[PD_TQ * CAP];
    __shared__ float thr_s[PD_TQ];
    __shared__ int32_t thr_p[PD_TQ];
    __shared__ int32_t cnt[PD_TQ];
    __shared__ int32_t f_cur[PD_TQ];                                   // the first entry of the query's list not yet behind the walk
    __shared__ int32_t f_len[PD_TQ];                                   // the length of the list (below 2^31: its positions are distinct)
    __shared__ int32_t f_next[PD_TQ];                                  // that entry's position, INT_MAX at the end
    __shared__ uint32_t fmask[PD_TQ * (PD_TC / 32)];                   // bit b of a query's 128: candidate ct + b is in its list

    const float *__restrict__ Q = P.Q;
    const float *__restrict__ X = P.X;
    const float *__restrict__ cb = P.cb;
    const int64_t nq = P.nq;
    const int32_t D4 = P.D4, k = P.k;

    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t q0 = (int64_t)blockIdx.x * PD_TQ;
    const int64_t c_begin = (int64_t)blockIdx.y * P.range_len;
    const int64_t c_end = c_begin + P.range_len < P.n ? c_begin + P.range_len : P.n;

    // the wave's own lists, and where its queries' filter lists enter the range
    const int qb = wave * 16;
    if (lane < 16) {
        const int64_t qg = q0 + qb + lane;
        const bool has = P.fptr && qg < nq;
        cnt[qb + lane] = 0; thr_s[qb + lane] = -INFINITY; thr_p[qb + lane] = INT_MAX;
        const int64_t lo = has ? P.fptr[qg] : 0, hi = has ? P.fptr[qg + 1] : 0;
        const int64_t cur = pd_lower_bound(P.fpos, lo, hi, (int32_t)c_begin);
        f_cur[qb + lane] = (int32_t)(cur - lo); f_len[qb + lane] = (int32_t)(hi - lo);
        f_next[qb + lane] = cur < hi ? P.fpos[cur] : INT_MAX;
    }
    fmask[qb * (PD_TC / 32) + lane] = 0;                               // 16 queries x 4 words: one word per lane
    bool dirty = false;                                                // wave-uniform: the wave's masks hold bits of an earlier tile

    // what this thread stages: piece i of a panel is row (tid + 256 i) >> 3, columns 4 ((tid + 256 i) & 7) ..
    const int c4 = (tid & 7) * 4, prow = tid >> 3;                      // rows prow, prow + 32 of the queries; prow + 32 j of the candidates
    const float *qsrc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int64_t qg = q0 + prow + 32 * i;
        qsrc[i] = qg < nq ? Q + qg * D4 : nullptr;
    }
    f32x4 pre[PD_LOADS];
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
        for (int i = 0; i < PD_LOADS; ++i) {
            float *dst = (i < 2 ? sq + (prow + 32 * i) * PD_LS : sx + (prow + 32 * (i - 2)) * PD_LS) + c4;   // 8-byte aligned: PD_LS and c4 are even
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
        selfp[reg] = qok[reg] ? P.selfpos[qg] : -1;
    }
    const int xa = (qb + (lane & 15)) * PD_LS + (lane >> 4);
    const int xb = (lane & 15) * PD_LS + (lane >> 4);

    if (c_begin < c_end) fetch(c_begin, 0);
    for (int64_t ct = c_begin; ct < c_end; ct += PD_TC) {
        f32x4 acc[PD_TC / 16];
#pragma unroll
        for (int t = 0; t < PD_TC / 16; ++t) acc[t] = f32x4{0, 0, 0, 0};
        for (int d0 = 0; d0 < D4; d0 += PD_DK) {
            __syncthreads();
            stage();
            __syncthreads();
            if (d0 + PD_DK < D4) fetch(ct, d0 + PD_DK);
            else if (ct + PD_TC < c_end) fetch(ct + PD_TC, 0);
            auto step = [&](int dd) {
                const float a = sq[xa + dd];
                float b[PD_TC / 16];
#pragma unroll
                for (int t = 0; t < PD_TC / 16; ++t) b[t] = sx[xb + t * 16 * PD_LS + dd];
#pragma unroll
                for (int t = 0; t < PD_TC / 16; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b[t], acc[t], 0, 0, 0);
            };
            if (D4 - d0 >= PD_DK) {                                   // a whole panel: unrolled, so the reads of a step run ahead of its products
#pragma unroll
                for (int dd = 0; dd < PD_DK; dd += 4) step(dd);
            } else {
#pragma unroll 1
                for (int dd = 0; dd < D4 - d0; dd += 4) step(dd);
            }
        }
        // the filter masks of this tile: the queries whose next filter entry lies inside it walk their lists on
        if (dirty) { fmask[qb * (PD_TC / 32) + lane] = 0; dirty = false; }
        const int32_t first = (int32_t)ct, last = (int32_t)(ct + (PD_TC - 1));          // ct is a multiple of PD_TC below 2^31: no overflow
        const int32_t nx = f_next[qb + (lane & 15)];                   // a position is below INT_MAX, so INT_MAX is no entry
        const uint32_t need = (uint32_t)__ballot(lane < 16 && nx != INT_MAX && nx <= last);
        const bool masked = need != 0;                                 // wave-uniform: some query of the wave has filter entries in this tile
        if (masked) {
            __builtin_amdgcn_wave_barrier();
#pragma unroll 1
            for (uint32_t left = need; left != 0; left &= left - 1) {
                const int j = __builtin_ctz(left);
                const int32_t *__restrict__ list = P.fpos + P.fptr[q0 + qb + j];             // wave-uniform, as cur and len
                int cur = __builtin_amdgcn_readfirstlane(f_cur[qb + j]);
                const int len = __builtin_amdgcn_readfirstlane(f_len[qb + j]);
                for (;;) {                                              // 64 entries per read; an entry is never below ct: the walk is monotone
                    const bool have = cur + lane < len;
                    const int32_t v = have ? list[cur + lane] : INT_MAX;
                    const bool inside = have && v <= last;
                    if (inside) atomicOr(&fmask[(qb + j) * (PD_TC / 32) + ((v - first) >> 5)], 1u << ((v - first) & 31));
                    const int found = __popcll(__ballot(inside));       // the list ascends: the entries inside are the first `found`
                    cur += found;
                    if (found < 64) {
                        if (lane == found) { f_cur[qb + j] = cur; f_next[qb + j] = v; }
                        break;
                    }
                }
            }
            dirty = true;
            __builtin_amdgcn_wave_barrier();
        }
        // C/D of the f32 form: column (candidate) = lane & 15, row (query) = 4 * (lane >> 4) + register.
        // bit 4 t + reg of `todo`: the z in acc[t][reg] has still to go into its query's list
        float ts[4];
        int32_t tp[4];
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) { ts[reg] = thr_s[ql + reg]; tp[reg] = thr_p[ql + reg]; }
        uint32_t todo = 0;
#pragma unroll
        for (int t = 0; t < PD_TC / 16; ++t) {
            const int64_t c = ct + t * 16 + (lane & 15);
            const bool in = c < c_end;
            const float bias = in ? cb[c] : 0.0f;
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                float z = acc[t][reg] + bias;
                z = z == z ? z : -INFINITY;                         // an overflowed sum ranks, and is reported, as -inf
                acc[t][reg] = z;
                if (in && qok[reg] && (int32_t)c != selfp[reg] && pd_beats(z, (int32_t)c, ts[reg], tp[reg])) todo |= 1u << (4 * t + reg);
            }
        }
        if (masked) {
            // the filter test, for what beat its threshold only: candidate ct + 16 t + (lane & 15) is bit 16 (t & 1) + (lane & 15) of word t >> 1
#pragma unroll 1
            for (int reg = 0; reg < 4; ++reg) {                         // a query at a time: four words in flight, not sixteen
                if ((todo & (0x11111111u << reg)) == 0) continue;
                uint32_t gone = 0;
#pragma unroll
                for (int i = 0; i < PD_TC / 32; ++i) {
                    const uint32_t w = fmask[(ql + reg) * (PD_TC / 32) + i] >> (lane & 15);
                    gone |= ((w & 1u) << (8 * i)) | (((w >> 16) & 1u) << (8 * i + 4));
                }
                todo &= ~(gone << reg);
            }
        }
        while (__any(todo != 0)) {
#pragma unroll
            for (int t = 0; t < PD_TC / 16; ++t)
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
                pd_rank<NI>(lsj, lpj, CAP, lane, s, p, rk);
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
            for (int t = 0; t < PD_TC / 16; ++t)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg)
                    if ((todo & (1u << (4 * t + reg))) && !pd_beats(acc[t][reg], (int32_t)(ct + t * 16 + (lane & 15)), ts[reg], tp[reg]))
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
        pd_rank<NI>(ls + (qb + j) * CAP, lp + (qb + j) * CAP, m, lane, s, p, rk);
        const int64_t base = (qg * gridDim.y + blockIdx.y) * k;
#pragma unroll
        for (int i = 0; i < NI; ++i)
            if (lane + 64 * i < m && rk[i] < k) { P.part_score[base + rk[i]] = s[i]; P.part_pos[base + rk[i]] = p[i]; }
        for (int e = m + lane; e < k; e += 64) { P.part_score[base + e] = -INFINITY; P.part_pos[base + e] = INT_MAX; }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Merge.  One wave per query, as k_nn_merge: the running best k and the next range's k entries sit side by side in LDS, are
// ranked under the same total order and the best k kept, range after range in ascending order.  On the way out positions become
// column ids (ids[pos]; ids null: the position is the id), the fill entries become (-1, -inf) and their number gives the count.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_predict_merge(const int32_t *__restrict__ part_pos, const float *__restrict__ part_score, int32_t ranges, int32_t k,
                                                      const int32_t *__restrict__ ids, int32_t *__restrict__ out_index, float *__restrict__ out_score,
                                                      int32_t *__restrict__ out_count) {
    constexpr int NI = 2 * PD_MAX_K / 64;
    __shared__ float ms[2 * PD_MAX_K];
    __shared__ int32_t mp[2 * PD_MAX_K];
    const int lane = (int)threadIdx.x;
    const int64_t q = blockIdx.x, base = q * ranges * k;
    for (int e = lane; e < k; e += 64) { ms[e] = part_score[base + e]; mp[e] = part_pos[base + e]; }
    for (int r = 1; r < ranges; ++r) {
        for (int e = lane; e < k; e += 64) { ms[k + e] = part_score[base + (int64_t)r * k + e]; mp[k + e] = part_pos[base + (int64_t)r * k + e]; }
        __builtin_amdgcn_wave_barrier();
        float s[NI];
        int32_t p[NI];
        int rk[NI];
        pd_rank<NI>(ms, mp, 2 * k, lane, s, p, rk);
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int i = 0; i < NI; ++i)
            if (lane + 64 * i < 2 * k && rk[i] < k) { ms[rk[i]] = s[i]; mp[rk[i]] = p[i]; }
        __builtin_amdgcn_wave_barrier();
    }
    __builtin_amdgcn_wave_barrier();
    int real = 0;
    for (int e = lane; e < k; e += 64) {
        const int32_t pos = mp[e];
        const bool fill = pos == INT_MAX;
        real += fill ? 0 : 1;
        out_score[q * k + e] = fill ? -INFINITY : ms[e];
        out_index[q * k + e] = fill ? -1 : (ids ? ids[pos] : pos);
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) real += __shfl_xor(real, m, 64);
    if (lane == 0) out_count[q] = real;
}

struct RunBuffers {                         // what one run allocates; freed on every way out
    std::vector<void *> ptrs;
    ~RunBuffers() { for (void *q : ptrs) (void)hipFree(q); }
    ge_status alloc(void **q, size_t bytes) { GE_HIP(hipMalloc(q, std::max<size_t>(bytes, 16))); ptrs.push_back(*q); return GE_OK; }
};

}  // namespace

struct ge_predict {
    ge_glove *glove = nullptr;
    ge::EvalView view{};
    int64_t n = 0, m = 0, nf = 0;        // queries; candidates |S|; filter entries inside S in all
    int32_t d4 = 0, has_filter = 0, ranges = 0;
    int32_t *dI = nullptr, *dsub = nullptr, *dself = nullptr, *dfpos = nullptr;
    int64_t *dfptr = nullptr;
    float *dq = nullptr, *dx = nullptr, *dcb = nullptr;
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};     // around staging; around select and merge of a batch
    float stage_ms = 0.0f, select_ms = 0.0f, merge_ms = 0.0f;
};

namespace {

void predict_free(ge_predict *p) {
    if (!p) return;
    (void)hipSetDevice(p->view.device);
    for (void *q : {(void *)p->dI, (void *)p->dsub, (void *)p->dself, (void *)p->dfpos, (void *)p->dfptr, (void *)p->dq, (void *)p->dx, (void *)p->dcb})
        if (q) (void)hipFree(q);
    for (hipEvent_t e : p->ev)
        if (e) (void)hipEventDestroy(e);
    delete p;
}

ge_status predict_create_impl(ge_glove *h, const int32_t *I, int64_t n, const int64_t *filter_ptr, const int32_t *filter_idx, const int32_t *subset,
                              int64_t n_subset, int32_t exclude_self, ge_predict **out) {
    if (!out) return ge::fail(GE_ERR_ARG, "out is null");
    *out = nullptr;
    if (!I) return ge::fail(GE_ERR_ARG, "null query rows");
    if (n < 1 || n >= ((int64_t)1 << 31)) return ge::fail(GE_ERR_ARG, "a prediction set holds 1 <= n < 2^31 query rows, got %lld", (long long)n);
    // what needs no handle: the shape of the lists, ids below zero, the order inside a list and inside the subset
    int64_t nf_in = 0;
    if (filter_ptr) {
        if (filter_ptr[0] != 0) return ge::fail(GE_ERR_ARG, "filter_ptr[0] is %lld, not 0", (long long)filter_ptr[0]);
        for (int64_t k = 0; k < n; ++k)
            if (filter_ptr[k + 1] < filter_ptr[k]) return ge::fail(GE_ERR_ARG, "filter_ptr decreases at [%lld]", (long long)(k + 1));
        nf_in = filter_ptr[n];
        if (nf_in >= PD_MAX_FILTER) return ge::fail(GE_ERR_ARG, "%lld filter entries are more than one set holds (2^35)", (long long)nf_in);
        if (nf_in > 0 && !filter_idx) return ge::fail(GE_ERR_ARG, "filter_idx is null");
    }
    for (int64_t k = 0; k < n; ++k) {
        if (I[k] < 0) return ge::fail(GE_ERR_ARG, "query %lld: focus row %d out of range", (long long)k, I[k]);
        if (!filter_ptr) continue;
        for (int64_t e = filter_ptr[k]; e < filter_ptr[k + 1]; ++e) {
            if (filter_idx[e] < 0) return ge::fail(GE_ERR_ARG, "query %lld: filter id %d out of range", (long long)k, filter_idx[e]);
            if (e > filter_ptr[k] && filter_idx[e] <= filter_idx[e - 1])
                return ge::fail(GE_ERR_ARG, "query %lld: the filter list is not strictly ascending at entry %lld", (long long)k, (long long)(e - filter_ptr[k]));
        }
    }
    if (subset) {
        if (n_subset < 1 || n_subset >= ((int64_t)1 << 31)) return ge::fail(GE_ERR_ARG, "predict: a subset of %lld columns", (long long)n_subset);
        for (int64_t i = 0; i < n_subset; ++i) {
            if (subset[i] < 0) return ge::fail(GE_ERR_ARG, "predict: subset[%lld] = %d out of range", (long long)i, subset[i]);
            if (i > 0 && subset[i] <= subset[i - 1]) return ge::fail(GE_ERR_ARG, "predict: the subset is not strictly ascending at [%lld]", (long long)i);
        }
    }
    if (!h) return ge::fail(GE_ERR_ARG, "null ge_glove handle");
    ge::EvalView v;
    GE_CHECK(ge::glove_eval_view(h, &v));
    if (v.dim < 1 || v.dim > PD_MAX_DIM) return ge::fail(GE_ERR_ARG, "predict: dim %d outside [1, %d]", v.dim, PD_MAX_DIM);
    for (int64_t k = 0; k < n; ++k) {
        if (I[k] < v.row_begin || I[k] >= v.row_end)
            return ge::fail(GE_ERR_ARG, "query %lld: focus row %d outside the handle's rows [%d,%d)", (long long)k, I[k], v.row_begin, v.row_end);
        // a list ascends, so its last id is its largest
        if (filter_ptr && filter_ptr[k + 1] > filter_ptr[k] && filter_idx[filter_ptr[k + 1] - 1] >= v.vocab_size)
            return ge::fail(GE_ERR_ARG, "query %lld: filter id %d outside [0,%d)", (long long)k, filter_idx[filter_ptr[k + 1] - 1], v.vocab_size);
    }
    if (subset && subset[n_subset - 1] >= v.vocab_size)
        return ge::fail(GE_ERR_ARG, "predict: subset[%lld] = %d outside [0,%d)", (long long)(n_subset - 1), subset[n_subset - 1], v.vocab_size);

    // everything from here on is in candidate positions: the filter lists (ids outside S dropped; ascending ids stay ascending
    // positions) and the query's own column
    const int64_t M = subset ? n_subset : (int64_t)v.vocab_size;
    auto position = [&](int32_t id) -> int32_t {
        if (!subset) return id;
        const int32_t *it = std::lower_bound(subset, subset + n_subset, id);
        return it != subset + n_subset && *it == id ? (int32_t)(it - subset) : -1;
    };
    std::vector<int64_t> fptr;
    std::vector<int32_t> fpos, selfpos((size_t)n, -1);
    if (filter_ptr) {
        fptr.assign((size_t)n + 1, 0);
        fpos.reserve((size_t)nf_in);
        for (int64_t k = 0; k < n; ++k) {
            for (int64_t e = filter_ptr[k]; e < filter_ptr[k + 1]; ++e) {
                const int32_t at = position(filter_idx[e]);
                if (at >= 0) fpos.push_back(at);
            }
            fptr[(size_t)k + 1] = (int64_t)fpos.size();
        }
    }
    if (exclude_self)
        for (int64_t k = 0; k < n; ++k) selfpos[(size_t)k] = position(I[k]);

    ge_predict *p = new ge_predict;
    p->glove = h; p->view = v; p->n = n; p->m = M; p->nf = (int64_t)fpos.size(); p->d4 = (v.dim + 3) / 4 * 4; p->has_filter = filter_ptr ? 1 : 0;
    struct Guard { ge_predict *p; ~Guard() { if (p) predict_free(p); } } guard{p};
    GE_HIP(hipSetDevice(v.device));
    const size_t N = (size_t)n, D4 = (size_t)p->d4;
    GE_HIP(hipMalloc((void **)&p->dI, sizeof(int32_t) * N));
    GE_HIP(hipMalloc((void **)&p->dself, sizeof(int32_t) * N));
    GE_HIP(hipMalloc((void **)&p->dq, sizeof(float) * N * D4));
    GE_HIP(hipMalloc((void **)&p->dx, sizeof(float) * (size_t)M * D4));
    GE_HIP(hipMalloc((void **)&p->dcb, sizeof(float) * (size_t)M));
    if (subset) GE_HIP(hipMalloc((void **)&p->dsub, sizeof(int32_t) * (size_t)M));
    if (filter_ptr) {
        GE_HIP(hipMalloc((void **)&p->dfptr, sizeof(int64_t) * (N + 1)));
        GE_HIP(hipMalloc((void **)&p->dfpos, std::max<size_t>(sizeof(int32_t) * fpos.size(), 16)));
    }
    for (hipEvent_t &e : p->ev) GE_HIP(hipEventCreate(&e));
    GE_HIP(hipMemcpyAsync(p->dI, I, sizeof(int32_t) * N, hipMemcpyHostToDevice, v.stream));
    GE_HIP(hipMemcpyAsync(p->dself, selfpos.data(), sizeof(int32_t) * N, hipMemcpyHostToDevice, v.stream));
    if (subset) GE_HIP(hipMemcpyAsync(p->dsub, subset, sizeof(int32_t) * (size_t)M, hipMemcpyHostToDevice, v.stream));
    if (filter_ptr) {
        GE_HIP(hipMemcpyAsync(p->dfptr, fptr.data(), sizeof(int64_t) * (N + 1), hipMemcpyHostToDevice, v.stream));
        if (!fpos.empty()) GE_HIP(hipMemcpyAsync(p->dfpos, fpos.data(), sizeof(int32_t) * fpos.size(), hipMemcpyHostToDevice, v.stream));
    }
    GE_HIP(hipStreamSynchronize(v.stream));      // the host arrays may go
    guard.p = nullptr;
    *out = p;
    return GE_OK;
}

ge_status launch_stage(const StageParams &p, hipStream_t stream) {
    const int64_t blocks = (p.n_rows * p.D4 + 255) / 256;
    hipLaunchKernelGGL(k_predict_stage, dim3((unsigned)blocks), dim3(256), 0, stream, p);
    GE_HIP(hipGetLastError());
    return GE_OK;
}

template <int CAP>
void launch_select(dim3 grid, hipStream_t stream, const SelectParams &s) {
    hipLaunchKernelGGL(k_predict_select<CAP>, grid, dim3(256), 0, stream, s);
}

ge_status predict_run_impl(ge_predict *p, int32_t K, int32_t *out_index, float *out_score, int32_t *out_count) {
    if (K < 1 || K > PD_MAX_K) return ge::fail(GE_ERR_ARG, "predict: K %d outside [1, %d]", K, PD_MAX_K);
    if (!p) return ge::fail(GE_ERR_ARG, "null ge_predict handle");
    GE_CHECK(ge::glove_eval_view(p->glove, &p->view));          // the tables move between epochs: read where they are now
    const ge::EvalView &v = p->view;
    GE_HIP(hipSetDevice(v.device));
    const int64_t n = p->n, M = p->m;
    const int32_t D4 = p->d4;
    hipStream_t stream = v.stream;

    // candidate ranges: whole tiles of PD_TC, as many as fill the device a few times over when the query tiles alone do not
    const int64_t ctiles = (M + PD_TC - 1) / PD_TC;
    auto ranges_for = [&](int64_t nq) {
        const int64_t qtiles = (nq + PD_TQ - 1) / PD_TQ;
        const int64_t want = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(ctiles, 1024), (2048 + qtiles - 1) / qtiles));
        const int64_t range_tiles = (ctiles + want - 1) / want;
        return std::pair<int64_t, int64_t>((ctiles + range_tiles - 1) / range_tiles, range_tiles * PD_TC);
    };
    // queries per launch: fewer queries can mean more ranges, so the batch shrinks until its own grid keeps the partial lists inside
    // PD_BATCH_ENTRIES (one query tile against the most ranges there can be, 1024, at K = 128 is half of that: it ends)
    int64_t nb = n;
    auto rb = ranges_for(nb);
    while (nb > PD_TQ && nb * rb.first * K > PD_BATCH_ENTRIES) {
        nb = std::max<int64_t>(PD_TQ, std::min<int64_t>(nb - PD_TQ, PD_BATCH_ENTRIES / (rb.first * K) / PD_TQ * PD_TQ));
        rb = ranges_for(nb);
    }
    const int64_t batch = nb, ranges = rb.first, range_len = rb.second;
    p->ranges = (int32_t)ranges;

    RunBuffers B;
    float *dps = nullptr, *dos = nullptr;
    int32_t *dpp = nullptr, *doi = nullptr, *doc = nullptr;
    GE_CHECK(B.alloc((void **)&dpp, sizeof(int32_t) * (size_t)(nb * ranges * K)));
    GE_CHECK(B.alloc((void **)&dps, sizeof(float) * (size_t)(nb * ranges * K)));
    GE_CHECK(B.alloc((void **)&doi, sizeof(int32_t) * (size_t)(nb * K)));
    GE_CHECK(B.alloc((void **)&dos, sizeof(float) * (size_t)(nb * K)));
    GE_CHECK(B.alloc((void **)&doc, sizeof(int32_t) * (size_t)nb));

    GE_HIP(hipEventRecord(p->ev[0], stream));
    StageParams q{};
    q.table = v.focus; q.rows = p->dI; q.out = p->dq; q.n_rows = n; q.stride = v.focus_stride;
    q.D = v.dim; q.D4 = D4; q.row_begin = v.row_begin; q.is16 = v.emb16;
    GE_CHECK(launch_stage(q, stream));
    StageParams x{};
    x.table = v.context; x.hub32 = v.hub32; x.hub_index = v.emb16 ? v.hub_index : nullptr; x.bias = v.cbias; x.rows = p->dsub;
    x.out = p->dx; x.bias_out = p->dcb; x.n_rows = M; x.stride = v.context_stride; x.bias_stride = v.cbias_stride;
    x.D = v.dim; x.D4 = D4; x.is16 = v.emb16;
    GE_CHECK(launch_stage(x, stream));
    GE_HIP(hipEventRecord(p->ev[1], stream));

    const int CAP = pd_cap_of(K);
    float select_ms = 0.0f, merge_ms = 0.0f;
    for (int64_t begin = 0; begin < n; begin += batch) {
        const int64_t nq = std::min(batch, n - begin);
        SelectParams s{};
        s.Q = p->dq + begin * D4; s.X = p->dx; s.cb = p->dcb; s.selfpos = p->dself + begin;
        s.fptr = p->has_filter ? p->dfptr + begin : nullptr; s.fpos = p->dfpos;
        s.part_pos = dpp; s.part_score = dps; s.nq = nq; s.n = M; s.range_len = range_len; s.D4 = D4; s.k = K;
        const dim3 grid((unsigned)((nq + PD_TQ - 1) / PD_TQ), (unsigned)ranges);
        GE_HIP(hipEventRecord(p->ev[2], stream));
        switch (CAP) {
        case 32: launch_select<32>(grid, stream, s); break;
        case 64: launch_select<64>(grid, stream, s); break;
        case 128: launch_select<128>(grid, stream, s); break;
        default: launch_select<256>(grid, stream, s); break;
        }
        GE_HIP(hipGetLastError());
        GE_HIP(hipEventRecord(p->ev[3], stream));
        hipLaunchKernelGGL(k_predict_merge, dim3((unsigned)nq), dim3(64), 0, stream, (const int32_t *)dpp, (const float *)dps, (int32_t)ranges, K,
                           (const int32_t *)p->dsub, doi, dos, doc);
        GE_HIP(hipGetLastError());
        GE_HIP(hipEventRecord(p->ev[4], stream));
        if (out_index) GE_HIP(hipMemcpyAsync(out_index + begin * K, doi, sizeof(int32_t) * (size_t)(nq * K), hipMemcpyDeviceToHost, stream));
        if (out_score) GE_HIP(hipMemcpyAsync(out_score + begin * K, dos, sizeof(float) * (size_t)(nq * K), hipMemcpyDeviceToHost, stream));
        if (out_count) GE_HIP(hipMemcpyAsync(out_count + begin, doc, sizeof(int32_t) * (size_t)nq, hipMemcpyDeviceToHost, stream));
        GE_HIP(hipStreamSynchronize(stream));
        float a = 0.0f, b = 0.0f;
        GE_HIP(hipEventElapsedTime(&a, p->ev[2], p->ev[3]));
        GE_HIP(hipEventElapsedTime(&b, p->ev[3], p->ev[4]));
        select_ms += a; merge_ms += b;
    }
    GE_HIP(hipEventElapsedTime(&p->stage_ms, p->ev[0], p->ev[1]));
    p->select_ms = select_ms; p->merge_ms = merge_ms;
    return GE_OK;
}

}  // namespace

extern "C" {

ge_status ge_glove_predict_create(ge_glove *h, const int32_t *I, int64_t n, const int64_t *filter_ptr, const int32_t *filter_idx, const int32_t *subset,
                                  int64_t n_subset, int32_t exclude_self, ge_predict **out) {
    GE_GUARD(predict_create_impl(h, I, n, filter_ptr, filter_idx, subset, n_subset, exclude_self, out));
}

ge_status ge_glove_predict_run(ge_predict *p, int32_t K, int32_t *out_index, float *out_score, int32_t *out_count) {
    GE_GUARD(predict_run_impl(p, K, out_index, out_score, out_count));
}

ge_status ge_predict_last_kernel_ms(const ge_predict *p, float *stage_ms, float *select_ms, float *merge_ms) {
    if (!p) return ge::fail(GE_ERR_ARG, "null ge_predict handle");
    if (stage_ms) *stage_ms = p->stage_ms;
    if (select_ms) *select_ms = p->select_ms;
    if (merge_ms) *merge_ms = p->merge_ms;
    return GE_OK;
}

ge_status ge_predict_get(const ge_predict *p, int64_t *n, int64_t *candidates, int32_t *dim, int32_t *ranges) {
    if (!p) return ge::fail(GE_ERR_ARG, "null ge_predict handle");
    if (n) *n = p->n;
    if (candidates) *candidates = p->m;
    if (dim) *dim = p->view.dim;
    if (ranges) *ranges = p->ranges;
    return GE_OK;
}

void ge_predict_destroy(ge_predict *p) { predict_free(p); }

}  // extern "C"
