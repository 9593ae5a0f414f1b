// align.hip -- alignment of two vertex sets behind the C ABI: every (source, target) pair of rows whose score reaches a threshold,
// and the one-to-one assignment a greedy walk over those candidates in descending score would make.  Both sets are prepared as
// nn.hip prepares rows (k_align_prepare), the scores are match.hip's fp32 chains on the fp32 matrix cores, walked over the
// rectangle source x target with a threshold epilogue (k_align_join), the survivors are sorted three times (rocprim radix sort:
// by (a, b), per source best first, per target best first), and the assignment comes from synchronous rounds of the
// locally-dominant rule (k_align_point, k_align_pair).  The reference has no counterpart; the semantics are written down in
// include/geglove.h, section "Alignment".
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

constexpr int AL_MAX_DIM = 1024;
constexpr int64_t AL_MAX_FLOATS = (int64_t)1 << 35;          // floats of input one index accepts (128 GiB as fp32)
constexpr int64_t AL_SLAB_FLOATS = (int64_t)1 << 26;         // a 256 MB slab of rows per upload
constexpr int64_t AL_MAX_PAIRS = (int64_t)1 << 28;           // the largest cap a run accepts
constexpr int64_t AL_MAX_ITEMS = (int64_t)1 << 30;           // workgroups of one join launch
constexpr int AL_BATCH = 8;                                  // assignment rounds the host enqueues between two looks at the counters

// ---------------------------------------------------------------------------------------------------------------------
// Prepare: k_match_prepare (hence nn.hip's k_nn_prepare), operation for operation.  One wave takes 64 rows: pieces of 64 columns
// are read coalesced into LDS, lane r then walks row r of the piece in ascending d (the fp64 sum of squares is a sequential
// chain), and a second coalesced pass writes x / n rounded to fp32 once into the table, whose rows are padded with zeros to
// D4 = dim rounded up to 4 floats.  rowmap: NULL or the source row of every output row.  A non-finite value raises *flag.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int PREP_ROWS = 64, PREP_COLS = 64, PREP_STRIDE = 65;

__global__ __launch_bounds__(64) void k_align_prepare(const float *__restrict__ src, const int32_t *__restrict__ rowmap, int64_t n_rows, int32_t D,
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
// Join.  The tile and its staging are k_match_join's: AL_TQ queries x AL_TC candidates, panels of AL_DK columns staged in LDS as
// [row][AL_LS floats] (AL_LS = 34 = 2 mod 32: the 32 lanes one ds_read_b32 cycle serves hit 32 different banks; the next panel
// travels in registers meanwhile), wave w carrying queries 16 w .. 16 w + 15 against all AL_TC candidates through
// v_mfma_f32_16x16x4_f32: eight independent accumulators, each bit for bit an fmaf chain over ascending d.  Queries come from
// the source table, candidates from the target table: the whole rectangle is walked.
//
// The grid is a list of equally long items.  The candidate tiles are cut into chunks of R tiles, and every chunk is wanted by
// every query tile: item = chunk * qtiles + query tile, chunk-major, so a workgroup finds both by one division, no workgroup runs
// longer than R tiles, and the workgroups in flight together read the same candidate panels.
//
// Epilogue per candidate tile: a lane compares its 32 scores with the threshold (a NaN fails the compare, as -inf would) and
// masks the rows past either table's end (they are staged as zeros and would score 0); the wave counts its survivors with a
// prefix sum over the lanes and, where there are any, reserves that many slots with ONE 64-bit integer atomic add; each survivor
// writes (posA << 32 | posB, score) while its slot is below `cap`.  The counter counts past the cap: it is the exact number of
// candidates.  Which slot a pair lands in depends on timing; the sort by key that follows does not.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int AL_TQ = 64, AL_TC = 128, AL_DK = 32, AL_LS = 34;
constexpr int AL_LOADS = (AL_TQ + AL_TC) * (AL_DK / 4) / 256;   // 16-byte pieces a thread moves per panel: 2 of queries, 4 of candidates
constexpr int AL_WG_PER_CU = 3;   // three waves per SIMD, as k_match_join

__global__ __launch_bounds__(256, AL_WG_PER_CU) void k_align_join(const float *__restrict__ XA, int64_t nA, const float *__restrict__ XB, int64_t nB,
                                                                  int32_t D4, int64_t qtiles, int32_t R, float thr, u64 cap, u64 *__restrict__ counter,
                                                                  uint2 *__restrict__ keys, float *__restrict__ scores) {
    __shared__ float sq[AL_TQ * AL_LS];
    __shared__ float sx[AL_TC * AL_LS];

    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    const int64_t item = (int64_t)blockIdx.x;
    const int64_t chunk = item / qtiles, qt = item - chunk * qtiles;
    const int64_t q0 = qt * AL_TQ;
    const int64_t ctiles = (nB + AL_TC - 1) / AL_TC;
    const int64_t t_lo = chunk * R;
    const int64_t t_hi = (chunk + 1) * R < ctiles ? (chunk + 1) * R : ctiles;
    const int64_t c_begin = t_lo * AL_TC;
    const int64_t c_end = t_hi * AL_TC < nB ? t_hi * AL_TC : nB;
    if (q0 >= nA || c_begin >= c_end) return;

    // what this thread stages: piece i of a panel is row (tid + 256 i) >> 3, columns 4 ((tid + 256 i) & 7) ..
    const int c4 = (tid & 7) * 4, prow = tid >> 3;                      // rows prow, prow + 32 of the queries; prow + 32 j of the candidates
    const float *qsrc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int64_t qg = q0 + prow + 32 * i;
        qsrc[i] = qg < nA ? XA + qg * D4 : nullptr;
    }
    f32x4 pre[AL_LOADS];
    auto fetch = [&](int64_t ct, int d0) {
        const bool in = d0 + c4 < D4;
#pragma unroll
        for (int i = 0; i < 2; ++i)
            pre[i] = in && qsrc[i] ? *reinterpret_cast<const f32x4 *>(qsrc[i] + d0 + c4) : f32x4{0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t c = ct + prow + 32 * i;
            pre[2 + i] = in && c < c_end ? *reinterpret_cast<const f32x4 *>(XB + c * D4 + d0 + c4) : f32x4{0, 0, 0, 0};
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int i = 0; i < AL_LOADS; ++i) {
            float *dst = (i < 2 ? sq + (prow + 32 * i) * AL_LS : sx + (prow + 32 * (i - 2)) * AL_LS) + c4;   // 8-byte aligned: AL_LS and c4 are even
            *reinterpret_cast<float2 *>(dst) = float2{pre[i][0], pre[i][1]};
            *reinterpret_cast<float2 *>(dst + 2) = float2{pre[i][2], pre[i][3]};
        }
    };

    // the four queries whose scores a lane holds: local rows 4 (lane >> 4) + reg of the wave's sixteen
    const int qb = wave * 16;
    const uint32_t qa = (uint32_t)q0 + (uint32_t)(qb + 4 * (lane >> 4));
    const int xa = (qb + (lane & 15)) * AL_LS + (lane >> 4);
    const int xb = (lane & 15) * AL_LS + (lane >> 4);

    fetch(c_begin, 0);
    for (int64_t ct = c_begin; ct < c_end; ct += AL_TC) {
        f32x4 acc[AL_TC / 16];
#pragma unroll
        for (int t = 0; t < AL_TC / 16; ++t) acc[t] = f32x4{0, 0, 0, 0};
        for (int d0 = 0; d0 < D4; d0 += AL_DK) {
            __syncthreads();
            stage();
            __syncthreads();
            if (d0 + AL_DK < D4) fetch(ct, d0 + AL_DK);
            else if (ct + AL_TC < c_end) fetch(ct + AL_TC, 0);
            auto step = [&](int dd) {
                const float a = sq[xa + dd];
                float b[AL_TC / 16];
#pragma unroll
                for (int t = 0; t < AL_TC / 16; ++t) b[t] = sx[xb + t * 16 * AL_LS + dd];
#pragma unroll
                for (int t = 0; t < AL_TC / 16; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b[t], acc[t], 0, 0, 0);
            };
            if (D4 - d0 >= AL_DK) {                                   // a whole panel: unrolled, so the reads of a step run ahead of its products
#pragma unroll
                for (int dd = 0; dd < AL_DK; dd += 4) step(dd);
            } else {
#pragma unroll 1
                for (int dd = 0; dd < D4 - d0; dd += 4) step(dd);
            }
        }
        // C/D of the f32 form: column (candidate) = lane & 15, row (query) = 4 * (lane >> 4) + register.
        // bit 4 t + reg of `mask`: the pair (qa + reg, ct + 16 t + (lane & 15)) qualifies; a < nA and b < c_end <= nB, so both are rows.
        // Positions are below 2^31: the epilogue works on their 32-bit values.
        const uint32_t cl = (uint32_t)ct + (uint32_t)(lane & 15), ce = (uint32_t)c_end, qe = (uint32_t)nA;
        uint32_t mask = 0;
#pragma unroll
        for (int t = 0; t < AL_TC / 16; ++t) {
            const uint32_t c = cl + 16u * t;
#pragma unroll
            for (int reg = 0; reg < 4; ++reg)
                if (c < ce && qa + reg < qe && acc[t][reg] >= thr) mask |= 1u << (4 * t + reg);
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
            for (int t = 0; t < AL_TC / 16; ++t)
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

// ---------------------------------------------------------------------------------------------------------------------
// Orders.  Candidate i of the list sorted by (posA, posB) gets two more keys: posA << 32 | ~key(s) and posB << 32 | ~key(s),
// key = the monotone 32-bit image of s + 0.0f (the sum turns -0 into +0, so equal scores have equal keys).  A STABLE sort of
// the indices i by either key lists every source's (target's) candidates best first, ties in ascending i: ascending b within
// a source, ascending a within a target.  The candidates' original ids are written here too.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_align_keys(const u64 *__restrict__ keys, const float *__restrict__ score, int64_t m,
                                                    const int32_t *__restrict__ ida, int64_t nA, const int32_t *__restrict__ idb, int64_t nB,
                                                    u64 *__restrict__ by_a, u64 *__restrict__ by_b, uint32_t *__restrict__ index, int32_t *__restrict__ a,
                                                    int32_t *__restrict__ b, int32_t *__restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const u64 pa = keys[i] >> 32, pb = keys[i] & 0xffffffffu;
    if ((int64_t)pa >= nA || (int64_t)pb >= nB) { *flag = 1; return; }
    const uint32_t u = __float_as_uint(score[i] + 0.0f);
    const uint32_t image = u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);   // ascends with the score
    by_a[i] = (pa << 32) | (u64)(~image);
    by_b[i] = (pb << 32) | (u64)(~image);
    index[i] = (uint32_t)i;
    a[i] = ida[pa];
    b[i] = idb[pb];
}

// first[v] = the first entry of vertex v in a list sorted by (vertex << 32 | ...), v = 0 .. n (first[n] = m): a bisection of at
// most 64 steps
__global__ __launch_bounds__(256) void k_align_rowptr(const u64 *__restrict__ sorted, int64_t m, int64_t n, int32_t *__restrict__ first) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v > n) return;
    int64_t lo = 0, hi = m;                                              // the answer lies in [lo, hi]
    for (int step = 0; step < 64 && lo < hi; ++step) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)(sorted[mid] >> 32) < v) lo = mid + 1; else hi = mid;
    }
    first[v] = (int32_t)lo;
}

// ---------------------------------------------------------------------------------------------------------------------
// Assignment: synchronous rounds of the locally-dominant rule.  Vertices 0 .. nA - 1 are the sources, nA .. nA + nB - 1 the
// targets.  k_align_point: every free vertex moves its cursor along its own list past partners that are assigned already and
// points at the first free one (-1: none is left).  k_align_pair (a later launch, so every pointer is visible): a free source p
// whose target points back at it takes it: mate[p] and mate[q] are plain stores to addresses no other thread of the launch
// writes or reads.  A pointer at q is only ever set in a round in which q is free, and q's own pointer is fresh in that round,
// so no stale pointer is compared.  Under the strict total order of the header the best candidate with both ends free is a
// mutual pointer, so a round assigns at least one pair while one is left, and the set of all rounds is the greedy walk's.
// A cursor only moves forward inside [first[v], first[v + 1]): all rounds together read each list once.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_align_init(int32_t *__restrict__ mate, int32_t *__restrict__ point, int32_t *__restrict__ cursor,
                                                    int32_t *__restrict__ pair, uint8_t *__restrict__ flags, const int32_t *__restrict__ first_a,
                                                    const int32_t *__restrict__ first_b, int64_t nA, int64_t nB) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= nA + nB) return;
    mate[v] = -1; point[v] = -1;
    cursor[v] = first_a ? (v < nA ? first_a[v] : first_b[v - nA]) : 0;
    if (v < nA) { pair[v] = -1; flags[v] = 0; }
}

__global__ __launch_bounds__(256) void k_align_point(const u64 *__restrict__ keys, int64_t m, const uint32_t *__restrict__ list_a,
                                                     const uint32_t *__restrict__ list_b, const int32_t *__restrict__ first_a,
                                                     const int32_t *__restrict__ first_b, int64_t nA, int64_t nB, const int32_t *__restrict__ mate,
                                                     int32_t *__restrict__ cursor, int32_t *__restrict__ point, int32_t *__restrict__ flag) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= nA + nB || mate[v] >= 0) return;
    const bool is_a = v < nA;
    const uint32_t *list = is_a ? list_a : list_b;
    const int64_t end = is_a ? first_a[v + 1] : first_b[v - nA + 1];
    int64_t c = cursor[v];
    if (c < 0 || c > end || end > m) { *flag = 1; return; }             // a cursor outside its list
    int32_t to = -1;
    for (; c < end; ++c) {                                                // at most the list's length, over all rounds
        const int64_t i = list[c];
        if (i >= m) { *flag = 1; return; }
        const int64_t other = is_a ? nA + (int64_t)(keys[i] & 0xffffffffu) : (int64_t)(keys[i] >> 32);
        if (is_a ? other >= nA + nB : other >= nA) { *flag = 1; return; }
        if (mate[other] < 0) { to = (int32_t)other; break; }
    }
    cursor[v] = (int32_t)c;
    point[v] = to;
}

// *made += the pairs of this round; bit 1 of flags marks the pairs of round 1: the mutual ones
__global__ __launch_bounds__(256) void k_align_pair(const int32_t *__restrict__ point, const int32_t *__restrict__ cursor, const uint32_t *__restrict__ list_a,
                                                    int64_t nA, int32_t *__restrict__ mate, int32_t *__restrict__ pair, uint8_t *__restrict__ flags,
                                                    int32_t first_round, u64 *__restrict__ made) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool take = false;
    if (p < nA && mate[p] < 0) {
        const int32_t q = point[p];
        if (q >= 0 && point[q] == (int32_t)p) {
            take = true;
            mate[p] = q;
            mate[q] = (int32_t)p;
            pair[p] = (int32_t)list_a[cursor[p]];                        // the candidate's place in the (a, b) order
            flags[p] = first_round ? 3 : 1;
        }
    }
    const u64 ballot = __ballot(take);
    if ((threadIdx.x & 63) == 0 && ballot) atomicAdd(made, (u64)__popcll(ballot));
}

// the assignment as original row ids and score bits
__global__ __launch_bounds__(256) void k_align_result(const int32_t *__restrict__ mate, const int32_t *__restrict__ pair, const float *__restrict__ score,
                                                      int64_t m, const int32_t *__restrict__ ida, int64_t nA, const int32_t *__restrict__ idb, int64_t nB,
                                                      int32_t *__restrict__ target_of, float *__restrict__ target_score, int32_t *__restrict__ source_of,
                                                      int32_t *__restrict__ flag) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= nA + nB) return;
    const int64_t w = mate[v];
    if (v < nA) {
        if (w >= 0 && (w < nA || w >= nA + nB || pair[v] < 0 || pair[v] >= m)) { *flag = 1; return; }
        target_of[v] = w >= 0 ? idb[w - nA] : -1;
        target_score[v] = w >= 0 ? score[pair[v]] : 0.0f;
    } else {
        if (w >= nA) { *flag = 1; return; }
        source_of[v - nA] = w >= 0 ? ida[w] : -1;
    }
}

// out[0] assigned, out[1] mutual, out[2] sources with candidates, out[3] targets with candidates, out[4] sources with two or more
__global__ __launch_bounds__(256) void k_align_summary(const uint8_t *__restrict__ flags, const int32_t *__restrict__ first_a,
                                                       const int32_t *__restrict__ first_b, int64_t nA, int64_t nB, u64 *__restrict__ out) {
    __shared__ u64 part[5];
    if (threadIdx.x < 5) part[threadIdx.x] = 0;
    __syncthreads();
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v < nA) {
        const int32_t have = first_a[v + 1] - first_a[v];
        if (flags[v] & 1) atomicAdd(&part[0], (u64)1);
        if (flags[v] & 2) atomicAdd(&part[1], (u64)1);
        if (have >= 1) atomicAdd(&part[2], (u64)1);
        if (have >= 2) atomicAdd(&part[4], (u64)1);
    } else if (v < nA + nB) {
        if (first_b[v - nA + 1] - first_b[v - nA] >= 1) atomicAdd(&part[3], (u64)1);
    }
    __syncthreads();
    if (threadIdx.x < 5 && part[threadIdx.x]) atomicAdd(out + threadIdx.x, part[threadIdx.x]);
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

struct ge_align {
    int32_t metric = 0, device = 0, dim = 0, d4 = 0;
    int64_t n_rows = 0, nA = 0, nB = 0;
    hipStream_t stream = nullptr;
    float *dxa = nullptr, *dxb = nullptr;   // [nA][d4], [nB][d4], prepared
    int32_t *dida = nullptr, *didb = nullptr;   // the original row id of every source and target position
    // the last run
    int state = 0;                          // 0 = none yet, 1 = results, 2 = overflowed
    int64_t found = 0;
    std::vector<int32_t> a, b, target_of, source_of;
    std::vector<float> score, target_score;
    std::vector<uint8_t> flags;
    ge_align_summary summary{};
    float prepare_ms = 0, join_ms = 0, sort_ms = 0, assign_ms = 0;
    int32_t rounds = 0;
    ~ge_align() { for (void *q : {(void *)dxa, (void *)dxb, (void *)dida, (void *)didb}) if (q) (void)hipFree(q); }
};

namespace {

ge_status check_set(const char *name, const int32_t *set, int64_t count, int64_t n_rows) {
    if (!set) return ge::fail(GE_ERR_ARG, "align: the %s set is null", name);
    if (count < 1 || count > n_rows) return ge::fail(GE_ERR_ARG, "align: a %s set of %lld of %lld rows", name, (long long)count, (long long)n_rows);
    for (int64_t i = 0; i < count; ++i) {
        if (set[i] < 0 || set[i] >= n_rows) return ge::fail(GE_ERR_ARG, "align: %s[%lld] = %d outside [0, %lld)", name, (long long)i, set[i], (long long)n_rows);
        if (i > 0 && set[i] <= set[i - 1]) return ge::fail(GE_ERR_ARG, "align: the %s set is not strictly ascending at [%lld]", name, (long long)i);
    }
    return GE_OK;
}

ge_status check_create(int64_t n_rows, int32_t dim, const int32_t *source, int64_t n_source, const int32_t *target, int64_t n_target, const ge_align_cfg *cfg) {
    if (!cfg) return ge::fail(GE_ERR_ARG, "ge_align_cfg is null");
    if (cfg->metric != GE_NN_COSINE && cfg->metric != GE_NN_DOT) return ge::fail(GE_ERR_ARG, "align: unknown metric %d", cfg->metric);
    if (dim < 1 || dim > AL_MAX_DIM) return ge::fail(GE_ERR_ARG, "align: dim %d outside [1, %d]", dim, AL_MAX_DIM);
    if (n_rows < 1 || n_rows >= INT_MAX) return ge::fail(GE_ERR_ARG, "align: %lld rows outside [1, 2^31 - 2]", (long long)n_rows);
    if (n_rows > AL_MAX_FLOATS / dim)
        return ge::fail(GE_ERR_ARG, "align: %lld rows of %d floats are more than one index holds (%lld floats)", (long long)n_rows, dim, (long long)AL_MAX_FLOATS);
    GE_CHECK(check_set("source", source, n_source, n_rows));
    GE_CHECK(check_set("target", target, n_target, n_rows));
    for (int64_t i = 0, j = 0; i < n_source && j < n_target;) {        // both ascend: one merge walk
        if (source[i] == target[j]) return ge::fail(GE_ERR_ARG, "align: the source and target sets share row %d", source[i]);
        if (source[i] < target[j]) ++i; else ++j;
    }
    return GE_OK;
}

// rows (host: slab by slab; dev: in place), picked by a map -> table[rows_out][d4], prepared; *ms += the kernels' time
ge_status prepare_rows(const float *host, const float *dev, const int32_t *host_map, const int32_t *dev_map, int64_t rows_out, int32_t dim, int32_t metric,
                       float *table, hipStream_t stream, float *ms_out) {
    const int D = dim, D4 = (D + 3) / 4 * 4;
    const int64_t slab_rows = std::min<int64_t>(std::max<int64_t>(PREP_ROWS, AL_SLAB_FLOATS / D / PREP_ROWS * PREP_ROWS), rows_out);
    DeviceBuffers B;
    float *dslab = nullptr;
    int32_t *dflag = nullptr;
    GE_CHECK(B.events(2));
    if (host) GE_CHECK(B.alloc((void **)&dslab, sizeof(float) * (size_t)slab_rows * D));
    GE_CHECK(B.alloc((void **)&dflag, sizeof(int32_t)));
    GE_HIP(hipMemsetAsync(dflag, 0, sizeof(int32_t), stream));
    std::vector<float> packed;
    if (host) packed.resize((size_t)slab_rows * D);
    float total = 0;
    for (int64_t begin = 0; begin < rows_out; begin += slab_rows) {
        const int64_t rows = std::min(slab_rows, rows_out - begin);
        const float *x = dev;
        const int32_t *map = dev ? dev_map + begin : nullptr;
        if (host) {
            for (int64_t r = 0; r < rows; ++r) std::memcpy(&packed[(size_t)r * D], host + (int64_t)host_map[begin + r] * D, sizeof(float) * (size_t)D);
            GE_HIP(hipMemcpyAsync(dslab, packed.data(), sizeof(float) * (size_t)rows * D, hipMemcpyHostToDevice, stream));
            x = dslab;
        }
        GE_HIP(hipEventRecord(B.ev[0], stream));
        hipLaunchKernelGGL(k_align_prepare, dim3((unsigned)((rows + PREP_ROWS - 1) / PREP_ROWS)), dim3(64), 0, stream, x, map, rows, D, D4, metric,
                           table + begin * D4, dflag);
        GE_HIP(hipGetLastError());
        GE_HIP(hipEventRecord(B.ev[1], stream));
        GE_HIP(hipStreamSynchronize(stream));                                       // the slab buffer and `packed` are free again
        float ms = 0;
        GE_HIP(hipEventElapsedTime(&ms, B.ev[0], B.ev[1]));
        total += ms;
    }
    int32_t flag = 0;
    GE_HIP(hipMemcpyAsync(&flag, dflag, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    GE_HIP(hipStreamSynchronize(stream));
    if (flag) return ge::fail(GE_ERR_ARG, "align: non-finite input (rows)");
    *ms_out += total;
    return GE_OK;
}

ge_status create_impl(const float *host, const float *dev, int64_t n_rows, int32_t dim, const int32_t *source, int64_t n_source, const int32_t *target,
                      int64_t n_target, const ge_align_cfg *cfg, ge_align **out) {
    std::unique_ptr<ge_align> p(new ge_align);
    p->metric = cfg->metric; p->device = cfg->device; p->stream = (hipStream_t)cfg->stream;
    p->dim = dim; p->d4 = (dim + 3) / 4 * 4; p->n_rows = n_rows; p->nA = n_source; p->nB = n_target;
    GE_HIP(hipMalloc((void **)&p->dxa, sizeof(float) * (size_t)p->nA * p->d4));
    GE_HIP(hipMalloc((void **)&p->dxb, sizeof(float) * (size_t)p->nB * p->d4));
    GE_HIP(hipMalloc((void **)&p->dida, sizeof(int32_t) * (size_t)p->nA));
    GE_HIP(hipMalloc((void **)&p->didb, sizeof(int32_t) * (size_t)p->nB));
    GE_HIP(hipMemcpyAsync(p->dida, source, sizeof(int32_t) * (size_t)p->nA, hipMemcpyHostToDevice, p->stream));
    GE_HIP(hipMemcpyAsync(p->didb, target, sizeof(int32_t) * (size_t)p->nB, hipMemcpyHostToDevice, p->stream));
    GE_CHECK(prepare_rows(host, dev, source, p->dida, p->nA, dim, p->metric, p->dxa, p->stream, &p->prepare_ms));
    GE_CHECK(prepare_rows(host, dev, target, p->didb, p->nB, dim, p->metric, p->dxb, p->stream, &p->prepare_ms));
    *out = p.release();
    return GE_OK;
}

ge_status align_create_host(const float *rows, int64_t n_rows, int32_t dim, const int32_t *source, int64_t n_source, const int32_t *target, int64_t n_target,
                            const ge_align_cfg *cfg, ge_align **out) {
    if (out) *out = nullptr;
    if (!rows || !out) return ge::fail(GE_ERR_ARG, "ge_align_create: rows or out is null");
    GE_CHECK(check_create(n_rows, dim, source, n_source, target, n_target, cfg));
    GE_CHECK(ge::select_device(cfg->device));
    return create_impl(rows, nullptr, n_rows, dim, source, n_source, target, n_target, cfg, out);
}

ge_status align_create_glove(ge_glove *h, const int32_t *source, int64_t n_source, const int32_t *target, int64_t n_target, const ge_align_cfg *cfg,
                             ge_align **out) {
    if (out) *out = nullptr;
    if (!h || !out) return ge::fail(GE_ERR_ARG, "ge_glove_align_create: handle or out is null");
    if (!cfg) return ge::fail(GE_ERR_ARG, "ge_align_cfg is null");
    if (cfg->metric != GE_NN_COSINE && cfg->metric != GE_NN_DOT) return ge::fail(GE_ERR_ARG, "align: unknown metric %d", cfg->metric);
    float *d = nullptr;
    int32_t V = 0, D = 0, device = 0;
    GE_CHECK(ge::glove_extract_device_f32(h, &d, &V, &D, &device));   // a fresh buffer: no trainer table is written
    ge_align_cfg own = *cfg;
    own.device = device;                                              // the rows live on the handle's device
    ge_status st = check_create(V, D, source, n_source, target, n_target, &own);
    if (st == GE_OK) st = create_impl(nullptr, d, V, D, source, n_source, target, n_target, &own, out);
    (void)hipFree(d);
    return st;
}

// the chunks of the join's grid: R candidate tiles each, every chunk wanted by every query tile
int32_t plan_join(int64_t nA, int64_t nB, int64_t *items) {
    const int64_t ctiles = (nB + AL_TC - 1) / AL_TC, qtiles = (nA + AL_TQ - 1) / AL_TQ;
    int64_t R = std::max<int64_t>(1, std::min<int64_t>(256, qtiles * ctiles / 16384));   // about 16 k items where the rectangle has them
    while ((ctiles + R - 1) / R * qtiles > AL_MAX_ITEMS) R *= 2;
    *items = (ctiles + R - 1) / R * qtiles;
    return (int32_t)R;
}

ge_status sort_pairs(DeviceBuffers &B, const u64 *kin, u64 *kout, const uint32_t *vin, uint32_t *vout, int64_t m, unsigned end_bit, hipStream_t stream) {
    void *dtmp = nullptr;
    size_t tmp_bytes = 0;
    GE_HIP(rocprim::radix_sort_pairs(nullptr, tmp_bytes, kin, kout, vin, vout, (size_t)m, 0, end_bit, stream));
    GE_CHECK(B.alloc(&dtmp, tmp_bytes));
    GE_HIP(rocprim::radix_sort_pairs(dtmp, tmp_bytes, kin, kout, vin, vout, (size_t)m, 0, end_bit, stream));
    return GE_OK;
}

unsigned key_bits(int64_t n) {                                        // bits of a key whose upper word is a position below n
    unsigned end_bit = 33;
    while (end_bit < 64 && ((int64_t)1 << (end_bit - 32)) < n) ++end_bit;
    return end_bit;
}

ge_status align_run(ge_align *p, float threshold, int64_t max_pairs) {
    if (!(std::fabs(threshold) <= 3.402823466e38f)) return ge::fail(GE_ERR_ARG, "align: the threshold must be finite");
    if (max_pairs < 1 || max_pairs > AL_MAX_PAIRS) return ge::fail(GE_ERR_ARG, "align: max_pairs %lld outside [1, 2^28]", (long long)max_pairs);
    if (!p) return ge::fail(GE_ERR_ARG, "null ge_align handle");
    GE_CHECK(ge::select_device(p->device));
    hipStream_t stream = p->stream;
    const int64_t nA = p->nA, nB = p->nB, nV = nA + nB;
    p->state = 0; p->found = 0; p->summary = ge_align_summary{};
    p->a.clear(); p->b.clear(); p->score.clear(); p->target_of.clear(); p->target_score.clear(); p->flags.clear(); p->source_of.clear();
    p->join_ms = p->sort_ms = p->assign_ms = 0; p->rounds = 0;

    const int64_t cap = std::min(max_pairs, nA * nB);                 // nA + nB < 2^31: no overflow; no run finds more, so no slot at or past it is written
    DeviceBuffers B;
    GE_CHECK(B.events(6));
    u64 *dcount = nullptr, *dkey = nullptr, *dsum = nullptr, *dmade = nullptr;
    float *dscore = nullptr;
    int32_t *dflag = nullptr;
    GE_CHECK(B.alloc((void **)&dcount, sizeof(u64)));
    GE_CHECK(B.alloc((void **)&dsum, sizeof(u64) * 5));
    GE_CHECK(B.alloc((void **)&dmade, sizeof(u64) * AL_BATCH));
    GE_CHECK(B.alloc((void **)&dflag, sizeof(int32_t)));
    GE_CHECK(B.alloc((void **)&dkey, sizeof(u64) * (size_t)cap));
    GE_CHECK(B.alloc((void **)&dscore, sizeof(float) * (size_t)cap));
    GE_HIP(hipMemsetAsync(dcount, 0, sizeof(u64), stream));
    GE_HIP(hipMemsetAsync(dsum, 0, sizeof(u64) * 5, stream));
    GE_HIP(hipMemsetAsync(dflag, 0, sizeof(int32_t), stream));

    // join
    u64 found = 0;
    {
        int64_t items = 0;
        const int32_t R = plan_join(nA, nB, &items);
        GE_HIP(hipEventRecord(B.ev[0], stream));
        hipLaunchKernelGGL(k_align_join, dim3((unsigned)items), dim3(256), 0, stream, (const float *)p->dxa, nA, (const float *)p->dxb, nB, p->d4,
                           (nA + AL_TQ - 1) / AL_TQ, R, threshold, (u64)cap, dcount, reinterpret_cast<uint2 *>(dkey), dscore);
        GE_HIP(hipGetLastError());
        GE_HIP(hipEventRecord(B.ev[1], stream));
        GE_HIP(hipMemcpyAsync(&found, dcount, sizeof(u64), hipMemcpyDeviceToHost, stream));
        GE_HIP(hipStreamSynchronize(stream));
        GE_HIP(hipEventElapsedTime(&p->join_ms, B.ev[0], B.ev[1]));
    }
    p->found = (int64_t)found;
    if ((int64_t)found > max_pairs) {
        p->state = 2;
        p->summary.candidates = (int64_t)found;
        return ge::fail(GE_ERR_OVERFLOW, "align: %lld candidates reach the threshold, more than max_pairs = %lld: raise the threshold or max_pairs",
                        (long long)found, (long long)max_pairs);
    }
    if ((int64_t)found > cap) return ge::fail(GE_ERR_STATE, "align: %lld candidates found among %lld x %lld rows", (long long)found, (long long)nA, (long long)nB);
    const int64_t m = (int64_t)found;

    // the three orders, the candidates' ids, and where each vertex's list begins
    u64 *dk1 = nullptr, *dkb = nullptr, *dsa = nullptr, *dsb = nullptr;
    float *ds1 = nullptr;
    uint32_t *dindex = nullptr, *dla = nullptr, *dlb = nullptr;
    int32_t *da = nullptr, *db = nullptr, *dfa = nullptr, *dfb = nullptr;
    if (m > 0) {
        GE_CHECK(B.alloc((void **)&dk1, sizeof(u64) * (size_t)m));
        GE_CHECK(B.alloc((void **)&ds1, sizeof(float) * (size_t)m));
        GE_CHECK(B.alloc((void **)&dkb, sizeof(u64) * (size_t)m));
        GE_CHECK(B.alloc((void **)&dsa, sizeof(u64) * (size_t)m));
        GE_CHECK(B.alloc((void **)&dsb, sizeof(u64) * (size_t)m));
        GE_CHECK(B.alloc((void **)&dindex, sizeof(uint32_t) * (size_t)m));
        GE_CHECK(B.alloc((void **)&dla, sizeof(uint32_t) * (size_t)m));
        GE_CHECK(B.alloc((void **)&dlb, sizeof(uint32_t) * (size_t)m));
        GE_CHECK(B.alloc((void **)&da, sizeof(int32_t) * (size_t)m));
        GE_CHECK(B.alloc((void **)&db, sizeof(int32_t) * (size_t)m));
        GE_CHECK(B.alloc((void **)&dfa, sizeof(int32_t) * (size_t)(nA + 1)));
        GE_CHECK(B.alloc((void **)&dfb, sizeof(int32_t) * (size_t)(nB + 1)));
        void *dtmp = nullptr;
        size_t tmp_bytes = 0;
        GE_HIP(rocprim::radix_sort_pairs(nullptr, tmp_bytes, (const u64 *)dkey, dk1, (const float *)dscore, ds1, (size_t)m, 0, key_bits(nA), stream));
        GE_CHECK(B.alloc(&dtmp, tmp_bytes));
        GE_HIP(hipEventRecord(B.ev[2], stream));
        GE_HIP(rocprim::radix_sort_pairs(dtmp, tmp_bytes, (const u64 *)dkey, dk1, (const float *)dscore, ds1, (size_t)m, 0, key_bits(nA), stream));
        u64 *dka = dkey;                                              // the unsorted slots are free again: m <= cap
        hipLaunchKernelGGL(k_align_keys, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, stream, (const u64 *)dk1, (const float *)ds1, m,
                           (const int32_t *)p->dida, nA, (const int32_t *)p->didb, nB, dka, dkb, dindex, da, db, dflag);
        GE_HIP(hipGetLastError());
        GE_CHECK(sort_pairs(B, dka, dsa, dindex, dla, m, key_bits(nA), stream));
        GE_CHECK(sort_pairs(B, dkb, dsb, dindex, dlb, m, key_bits(nB), stream));
        hipLaunchKernelGGL(k_align_rowptr, dim3((unsigned)((nA + 256) / 256)), dim3(256), 0, stream, (const u64 *)dsa, m, nA, dfa);
        GE_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_align_rowptr, dim3((unsigned)((nB + 256) / 256)), dim3(256), 0, stream, (const u64 *)dsb, m, nB, dfb);
        GE_HIP(hipGetLastError());
        GE_HIP(hipEventRecord(B.ev[3], stream));
    }

    // assignment: rounds in batches of AL_BATCH; an empty round changes nothing, so those after the first empty one are harmless
    int32_t *dmate = nullptr, *dpoint = nullptr, *dcursor = nullptr, *dpair = nullptr, *dtarget_of = nullptr, *dsource_of = nullptr;
    uint8_t *dflags = nullptr;
    float *dtarget_score = nullptr;
    GE_CHECK(B.alloc((void **)&dmate, sizeof(int32_t) * (size_t)nV));
    GE_CHECK(B.alloc((void **)&dpoint, sizeof(int32_t) * (size_t)nV));
    GE_CHECK(B.alloc((void **)&dcursor, sizeof(int32_t) * (size_t)nV));
    GE_CHECK(B.alloc((void **)&dpair, sizeof(int32_t) * (size_t)nA));
    GE_CHECK(B.alloc((void **)&dflags, (size_t)nA));
    GE_CHECK(B.alloc((void **)&dtarget_of, sizeof(int32_t) * (size_t)nA));
    GE_CHECK(B.alloc((void **)&dtarget_score, sizeof(float) * (size_t)nA));
    GE_CHECK(B.alloc((void **)&dsource_of, sizeof(int32_t) * (size_t)nB));
    const dim3 all_grid((unsigned)((nV + 255) / 256)), a_grid((unsigned)((nA + 255) / 256));
    GE_HIP(hipEventRecord(B.ev[4], stream));
    hipLaunchKernelGGL(k_align_init, all_grid, dim3(256), 0, stream, dmate, dpoint, dcursor, dpair, dflags, (const int32_t *)dfa, (const int32_t *)dfb, nA, nB);
    GE_HIP(hipGetLastError());
    int32_t rounds = 0;
    const int64_t most = std::min(nA, nB);                            // every assigning round makes a pair, and there are at most `most` pairs
    for (bool done = m == 0; !done;) {
        u64 made[AL_BATCH];
        GE_HIP(hipMemsetAsync(dmade, 0, sizeof(made), stream));
        for (int r = 0; r < AL_BATCH; ++r) {
            hipLaunchKernelGGL(k_align_point, all_grid, dim3(256), 0, stream, (const u64 *)dk1, m, (const uint32_t *)dla, (const uint32_t *)dlb,
                               (const int32_t *)dfa, (const int32_t *)dfb, nA, nB, (const int32_t *)dmate, dcursor, dpoint, dflag);
            GE_HIP(hipGetLastError());
            hipLaunchKernelGGL(k_align_pair, a_grid, dim3(256), 0, stream, (const int32_t *)dpoint, (const int32_t *)dcursor, (const uint32_t *)dla, nA, dmate,
                               dpair, dflags, (int32_t)(rounds == 0 && r == 0), dmade + r);
            GE_HIP(hipGetLastError());
        }
        GE_HIP(hipMemcpyAsync(made, dmade, sizeof(made), hipMemcpyDeviceToHost, stream));
        GE_HIP(hipStreamSynchronize(stream));
        for (int r = 0; r < AL_BATCH && !done; ++r) {
            ++rounds;
            if (made[r] == 0) done = true;
            else if (rounds > most) return ge::fail(GE_ERR_STATE, "align: round %d still assigns, past the bound of %lld assigning rounds", rounds, (long long)most);
        }
    }
    if (m > 0) {
        hipLaunchKernelGGL(k_align_summary, all_grid, dim3(256), 0, stream, (const uint8_t *)dflags, (const int32_t *)dfa, (const int32_t *)dfb, nA, nB, dsum);
        GE_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_align_result, all_grid, dim3(256), 0, stream, (const int32_t *)dmate, (const int32_t *)dpair, (const float *)ds1, m,
                       (const int32_t *)p->dida, nA, (const int32_t *)p->didb, nB, dtarget_of, dtarget_score, dsource_of, dflag);
    GE_HIP(hipGetLastError());
    GE_HIP(hipEventRecord(B.ev[5], stream));

    std::vector<int32_t> a((size_t)m), b((size_t)m), target_of((size_t)nA), source_of((size_t)nB);
    std::vector<float> score((size_t)m), target_score((size_t)nA);
    std::vector<uint8_t> flags((size_t)nA);
    u64 sum[5] = {0, 0, 0, 0, 0};
    int32_t flag = 0;
    if (m > 0) {
        GE_HIP(hipMemcpyAsync(a.data(), da, sizeof(int32_t) * (size_t)m, hipMemcpyDeviceToHost, stream));
        GE_HIP(hipMemcpyAsync(b.data(), db, sizeof(int32_t) * (size_t)m, hipMemcpyDeviceToHost, stream));
        GE_HIP(hipMemcpyAsync(score.data(), ds1, sizeof(float) * (size_t)m, hipMemcpyDeviceToHost, stream));
    }
    GE_HIP(hipMemcpyAsync(target_of.data(), dtarget_of, sizeof(int32_t) * (size_t)nA, hipMemcpyDeviceToHost, stream));
    GE_HIP(hipMemcpyAsync(target_score.data(), dtarget_score, sizeof(float) * (size_t)nA, hipMemcpyDeviceToHost, stream));
    GE_HIP(hipMemcpyAsync(flags.data(), dflags, (size_t)nA, hipMemcpyDeviceToHost, stream));
    GE_HIP(hipMemcpyAsync(source_of.data(), dsource_of, sizeof(int32_t) * (size_t)nB, hipMemcpyDeviceToHost, stream));
    GE_HIP(hipMemcpyAsync(sum, dsum, sizeof(sum), hipMemcpyDeviceToHost, stream));
    GE_HIP(hipMemcpyAsync(&flag, dflag, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    GE_HIP(hipStreamSynchronize(stream));
    if (m > 0) GE_HIP(hipEventElapsedTime(&p->sort_ms, B.ev[2], B.ev[3]));
    GE_HIP(hipEventElapsedTime(&p->assign_ms, B.ev[4], B.ev[5]));
    p->rounds = rounds;
    if (flag) return ge::fail(GE_ERR_STATE, "align: the assignment kernels met a candidate outside the sets or a cursor outside its list");
    p->a.swap(a); p->b.swap(b); p->score.swap(score);
    p->target_of.swap(target_of); p->target_score.swap(target_score); p->flags.swap(flags); p->source_of.swap(source_of);
    p->summary.candidates = m;
    p->summary.assigned = (int64_t)sum[0];
    p->summary.mutual = (int64_t)sum[1];
    p->summary.sources_with_candidates = (int64_t)sum[2];
    p->summary.targets_with_candidates = (int64_t)sum[3];
    p->summary.ambiguous_sources = (int64_t)sum[4];
    p->state = 1;
    return GE_OK;
}

ge_status align_get(const ge_align *p, int64_t *n_source, int64_t *n_target, int64_t *found, const int32_t **a, const int32_t **b, const float **score,
                    const int32_t **target_of, const float **target_score, const uint8_t **flags, const int32_t **source_of, ge_align_summary *summary) {
    if (!p) return ge::fail(GE_ERR_ARG, "null ge_align handle");
    if (n_source) *n_source = p->nA;
    if (n_target) *n_target = p->nB;
    if (found) *found = p->found;
    const bool have = p->state == 1;
    if (a) *a = have ? p->a.data() : nullptr;
    if (b) *b = have ? p->b.data() : nullptr;
    if (score) *score = have ? p->score.data() : nullptr;
    if (target_of) *target_of = have ? p->target_of.data() : nullptr;
    if (target_score) *target_score = have ? p->target_score.data() : nullptr;
    if (flags) *flags = have ? p->flags.data() : nullptr;
    if (source_of) *source_of = have ? p->source_of.data() : nullptr;
    if (summary) *summary = p->summary;
    return GE_OK;
}

}  // namespace

extern "C" {

void ge_align_cfg_default(ge_align_cfg *cfg) {
    if (!cfg) return;
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->metric = GE_NN_COSINE;
}
int32_t ge_align_cfg_size(void) { return (int32_t)sizeof(ge_align_cfg); }
int32_t ge_align_summary_size(void) { return (int32_t)sizeof(ge_align_summary); }

ge_status ge_align_create(const float *rows, int64_t n_rows, int32_t dim, const int32_t *source, int64_t n_source, const int32_t *target, int64_t n_target,
                          const ge_align_cfg *cfg, ge_align **out) {
    GE_GUARD(align_create_host(rows, n_rows, dim, source, n_source, target, n_target, cfg, out));
}
ge_status ge_glove_align_create(ge_glove *h, const int32_t *source, int64_t n_source, const int32_t *target, int64_t n_target, const ge_align_cfg *cfg,
                                ge_align **out) {
    GE_GUARD(align_create_glove(h, source, n_source, target, n_target, cfg, out));
}
ge_status ge_align_run(ge_align *p, float threshold, int64_t max_pairs) { GE_GUARD(align_run(p, threshold, max_pairs)); }
ge_status ge_align_get(const ge_align *p, int64_t *n_source, int64_t *n_target, int64_t *found, const int32_t **a, const int32_t **b, const float **score,
                       const int32_t **target_of, const float **target_score, const uint8_t **flags, const int32_t **source_of, ge_align_summary *summary) {
    return align_get(p, n_source, n_target, found, a, b, score, target_of, target_score, flags, source_of, summary);
}

ge_status ge_align_last_kernel_ms(const ge_align *p, float *prepare_ms, float *join_ms, float *sort_ms, float *assign_ms, int32_t *rounds) {
    if (!p) return ge::fail(GE_ERR_ARG, "null ge_align handle");
    if (prepare_ms) *prepare_ms = p->prepare_ms;
    if (join_ms) *join_ms = p->join_ms;
    if (sort_ms) *sort_ms = p->sort_ms;
    if (assign_ms) *assign_ms = p->assign_ms;
    if (rounds) *rounds = p->rounds;
    return GE_OK;
}

void ge_align_destroy(ge_align *p) { delete p; }

}  // extern "C"
