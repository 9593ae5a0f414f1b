// glove_layout.hip -- builds the blocked epoch layout of the Hogwild trainer on the device (ge_layout.h).
//
// Replaces four serial O(N) host passes of round 1 (range check, column count, placement, flush limits).  Pipeline, all on
// the handle's stream (N = nonzeros, V = vocabulary, rows = focus rows owned):
//   upload I, J, X (a device-resident ge_coo is read in place instead) -> k_scan_input (range check + column histogram, wave-aggregated atomics)
//   -> host: hub columns, their dense rank, their flush limits                      O(V)
//   -> k_sort_keys (key = hub ? rank(j) : n_hub + i, per-row count of the rest)     O(N)
//   -> rocprim::radix_sort_pairs (stable: column-major hubs, then the rest grouped by row in matrix order)
//   -> host: rows packed whole into chunks, long rows cut into pieces               O(rows + chunks)
//   -> k_place (position, bA, bB, L, W, border per nonzero; the cost terms are computed here, once per nonzero)
// Roofline: HBM streaming + one radix sort; runs once per handle.
#include "ge_layout.h"
#include "ge_cost.h"

#include <algorithm>
#include <cmath>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>

namespace {

__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }

// one atomicAdd per distinct key per wavefront (the hub columns / the row a wavefront sits in would otherwise
// serialise 64 atomics on one address)
__device__ __forceinline__ void wave_count(int32_t *cnt, int32_t key, bool active) {
    bool todo = active;
    for (;;) {
        const unsigned long long m = __ballot(todo);
        if (!m) break;
        const int leader = __ffsll((long long)m) - 1;
        const int32_t k0 = __shfl(key, leader, 64);
        const bool same = todo && key == k0;
        const unsigned long long ms = __ballot(same);
        if (lane_id() == leader) atomicAdd(cnt + k0, (int32_t)__popcll(ms));
        todo = todo && !same;
    }
}

__global__ __launch_bounds__(256) void k_scan_input(const int32_t *I, const int32_t *J, int64_t N, int32_t rb, int32_t re,
                                                    int32_t V, int32_t *col_cnt, unsigned long long *first_bad) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < N; base += stride) {
        const int64_t k = base + threadIdx.x;
        const bool act = k < N;
        const int32_t i = act ? I[k] : rb, j = act ? J[k] : 0;
        const bool bad = act && (i < rb || i >= re || j < 0 || j >= V);
        if (bad) atomicMin(first_bad, (unsigned long long)k);
        wave_count(col_cnt, j, act && !bad);
    }
}

// Keys, ascending: tiles [0, tile_keys) = ((group * rows + row) * tile_g + slot), the other hub columns tile_keys + rank, the rest
// tile_keys + n_hub + row.  tile_slot[j] = group * tile_g + slot of a tile column, else -1 (null: the handle has no tiles);
// hub_rank[j] ranks the hub columns outside the tiles.  tile_cnt counts the nonzeros of every (group, row).
__global__ __launch_bounds__(256) void k_sort_keys(const int32_t *I, const int32_t *J, int64_t N, int32_t rb,
                                                   const int32_t *hub_rank, int32_t n_hub, uint32_t *key, int32_t *val, int32_t *row_cnt,
                                                   const int32_t *tile_slot, int32_t tile_g, int32_t rows, uint32_t tile_keys, int32_t *tile_cnt) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < N; base += stride) {
        const int64_t k = base + threadIdx.x;
        const bool act = k < N;
        int32_t r = 0; bool rest = false;
        if (act) {
            const int32_t j = J[k];
            const int32_t h = hub_rank[j];
            const int32_t ts = tile_slot ? tile_slot[j] : -1;
            r = I[k] - rb;
            rest = h < 0 && ts < 0;
            if (ts >= 0) {
                const int32_t g = ts / tile_g;
                key[k] = (uint32_t)(((int64_t)g * rows + r) * tile_g + (ts - g * tile_g));
                atomicAdd(tile_cnt + (int64_t)g * rows + r, 1);
            } else key[k] = tile_keys + (rest ? (uint32_t)n_hub + (uint32_t)r : (uint32_t)h);
            val[k] = (int32_t)k;
        }
        wave_count(row_cnt, r, rest);
    }
}

// positions: tiles [0, nT) and the other hub columns [nT, nH) lie where the sort put them; the rest follows its row's place
__global__ __launch_bounds__(256) void k_place(const int32_t *I, const int32_t *J, const float *X, int64_t N, int32_t rb,
                                               const uint32_t *skey, const int32_t *sval, int32_t n_hub, int64_t nH,
                                               const int32_t *row_src, const int32_t *row_dst, int kind, double xmax,
                                               int32_t *bA, int32_t *bB, double *L, float *W, int32_t *border,
                                               uint32_t tile_keys, int32_t tile_g) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < N; t += stride) {
        const int32_t k = sval[t];
        const int32_t i = I[k], j = J[k];
        int64_t pos; int32_t a, b;
        if (skey[t] < tile_keys) { pos = t; a = i; b = (int32_t)(skey[t] % (uint32_t)tile_g); }      // T: resident side = the group, bB = slot
        else if (skey[t] - tile_keys < (uint32_t)n_hub) { pos = t; a = j; b = i; }                 // H: column-major, positions [nT, nH)
        else { const int32_t r = i - rb; pos = (int64_t)row_dst[r] + (t - nH - row_src[r]); a = i; b = j; }
        double l; float w;
        cost_terms<false>(kind, X[k], xmax, l, w);
        bA[pos] = a; bB[pos] = b; L[pos] = l; W[pos] = w; border[pos] = k;
    }
}

// Hub tiles: the cuts of an epoch.  Inside a tile chunk the column in slot s is published and re-read every tlim[s] of its updates,
// so a chunk with n_s nonzeros in slot s has sum_s n_s / tlim[s] cuts (one lane per chunk; G <= 8).
__global__ __launch_bounds__(256) void k_tile_cuts(const int32_t *bB, const int32_t *cstart, const int32_t *cmeta, const int32_t *tlim,
                                                   int64_t n_tchunks, int32_t G, unsigned long long *cuts) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n_tchunks; c += stride) {
        const int32_t *lim = tlim + (int64_t)cmeta[c] * G;
        unsigned long long n = 0;
        for (int32_t s = 0; s < G; ++s) {
            int32_t cnt = 0;
            for (int32_t k = cstart[c]; k < cstart[c + 1]; ++k) cnt += bB[k] == s;
            n += (unsigned long long)(cnt / lim[s]);
        }
        if (n) atomicAdd(cuts, n);
    }
}

struct Dev {            // frees every temporary of one build
    std::vector<void *> p;
    ~Dev() { for (void *q : p) (void)hipFree(q); }
    template <typename T> hipError_t alloc(T **out, size_t n) {
        hipError_t e = hipMalloc((void **)out, sizeof(T) * std::max<size_t>(n, 1));
        if (e == hipSuccess) p.push_back((void *)*out);
        return e;
    }
};

// Workgroups that start in the panel loop: the panels' share of the epoch's TIME, so that both queues run dry together and panel
// chunks and ordinary chunks alternate through the whole epoch.  (Hub columns trained in a phase of their own, before or behind
// everything else, cost convergence: at C2's shape with forced panels the second epoch's cost is 4 % above the column-major walk's
// with every workgroup starting in the panel loop, 0.2 % with 600 of 768.)  The panel loop is a dependent chain: a pipeline step
// lasts as long as its busiest stage, so a (row, panel) visit counts the largest number of nonzeros one of the four groups has in
// that row, a chunk three more steps, and a workgroup does one step at a time; the main queue's nonzeros go four to a workgroup at
// a time.  PANEL_STEP_COST is a panel update's time over an ordinary one's (its focus pair comes from LDS, not from memory), fitted
// to the two measured optima: 192 workgroups at the bench size (sweep 24 / 82 / 96 / 192 / 384) and 600 at C2's shape (500 / 600 /
// 700 / 760 / 768); profiles/hub_panels_bench.json.  The panels' share of the schedule's BYTES, doubled -- the first guess -- gives
// 82 at the bench size, where the panel loop is then the long pole and the epoch slower than without panels.
constexpr double PANEL_STEP_COST = 0.8;
// The ring kernel keeps the constant: with panels down to density 1/16 the bench handle gets 284 workgroups.  The
// sweep there (206: 46.8 ms, 250: 45.0, 270: 45.3, 284: 45.6, 300: 46.0, 320: 46.4; parent 46.5; profiles/hub_ring_bench.json) has
// its best near 250 on the slower kind of placement, but on the faster kind 261 gave no gain and 284 did, and C2's shape needs its
// 578 for convergence: one constant for both kernels.

int grid_for(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 16384)); }

}  // namespace

namespace ge {

void BlockedLayout::release() {
    for (void *q : {(void *)bA, (void *)bB, (void *)border, (void *)L, (void *)W, (void *)cstart, (void *)cmeta, (void *)tcols, (void *)tlim,
                    (void *)prow0, (void *)prows, (void *)ppos}) if (q) (void)hipFree(q);
    bA = bB = border = cstart = cmeta = tcols = tlim = prow0 = prows = ppos = nullptr; L = nullptr; W = nullptr;
}

ge_status build_blocked_layout(const LayoutRequest &rq, const int32_t *I, const int32_t *J, const float *X,
                               hipStream_t stream, BlockedLayout *out) {
    struct Clock {           // GE_GLOVE_TIMING=1 (see ge_glove_create)
        bool on = std::getenv("GE_GLOVE_TIMING") != nullptr;
        hipStream_t stream = nullptr;
        std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
        void lap(const char *what) {
            if (!on) return;
            (void)hipStreamSynchronize(stream);
            const auto n = std::chrono::steady_clock::now();
            std::fprintf(stderr, "[ge_glove_create]   layout: %-24s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(n - t).count());
            t = n;
        }
    } clk;
    clk.stream = stream;
    const int64_t N = rq.N;
    const int32_t V = rq.V, rb = rq.row_begin, rows = rq.row_end - rq.row_begin;
    Dev tmp;
    int32_t *dI = nullptr, *dJ = nullptr; float *dX = nullptr;
    int32_t *d_col = nullptr, *d_row = nullptr; unsigned long long *d_bad = nullptr;
    if (rq.device_input) { dI = const_cast<int32_t *>(I); dJ = const_cast<int32_t *>(J); dX = const_cast<float *>(X); }      // read only, in place
    else { GE_HIP(tmp.alloc(&dI, (size_t)N)); GE_HIP(tmp.alloc(&dJ, (size_t)N)); GE_HIP(tmp.alloc(&dX, (size_t)N)); }
    GE_HIP(tmp.alloc(&d_col, (size_t)V)); GE_HIP(tmp.alloc(&d_row, (size_t)rows)); GE_HIP(tmp.alloc(&d_bad, 1));
    if (N > 0 && !rq.device_input) {
        GE_HIP(hipMemcpyAsync(dI, I, sizeof(int32_t) * (size_t)N, hipMemcpyHostToDevice, stream));
        GE_HIP(hipMemcpyAsync(dJ, J, sizeof(int32_t) * (size_t)N, hipMemcpyHostToDevice, stream));
        GE_HIP(hipMemcpyAsync(dX, X, sizeof(float) * (size_t)N, hipMemcpyHostToDevice, stream));
    }
    GE_HIP(hipMemsetAsync(d_col, 0, sizeof(int32_t) * (size_t)V, stream));
    GE_HIP(hipMemsetAsync(d_row, 0, sizeof(int32_t) * (size_t)rows, stream));
    GE_HIP(hipMemsetAsync(d_bad, 0xFF, sizeof(unsigned long long), stream));
    if (N > 0) hipLaunchKernelGGL(k_scan_input, dim3(grid_for(N)), dim3(256), 0, stream, dI, dJ, N, rb, rq.row_end, V, d_col, d_bad);
    GE_HIP(hipGetLastError());
    std::vector<int32_t> cnt((size_t)V);
    unsigned long long bad = ~0ull;
    GE_HIP(hipMemcpyAsync(cnt.data(), d_col, sizeof(int32_t) * (size_t)V, hipMemcpyDeviceToHost, stream));
    GE_HIP(hipMemcpyAsync(&bad, d_bad, sizeof(bad), hipMemcpyDeviceToHost, stream));
    GE_HIP(hipStreamSynchronize(stream));
    clk.lap("upload + column counts");
    if (bad != ~0ull) {
        const int64_t k = (int64_t)bad;
        if (rq.device_input) {               // the offending entry comes back from the device for the message
            int32_t bi = 0, bj = 0;
            GE_HIP(hipMemcpy(&bi, dI + k, sizeof(int32_t), hipMemcpyDeviceToHost));
            GE_HIP(hipMemcpy(&bj, dJ + k, sizeof(int32_t), hipMemcpyDeviceToHost));
            if (bi < rb || bi >= rq.row_end) return ge::fail(GE_ERR_ARG, "I[%lld]=%d outside owned rows [%d,%d)", (long long)k, bi, rb, rq.row_end);
            return ge::fail(GE_ERR_ARG, "J[%lld]=%d outside [0,%d)", (long long)k, bj, V);
        }
        if (I[k] < rb || I[k] >= rq.row_end) return ge::fail(GE_ERR_ARG, "I[%lld]=%d outside owned rows [%d,%d)", (long long)k, I[k], rb, rq.row_end);
        return ge::fail(GE_ERR_ARG, "J[%lld]=%d outside [0,%d)", (long long)k, J[k], V);
    }

    // ---- hub columns: count(j) * workers >= theta * N; their flush limits ----
    std::vector<int32_t> hub_rank((size_t)V, -1);
    std::vector<int32_t> hubs;                     // hub columns, ascending
    out->hot_cols = 0; out->hot_nnz = 0; out->hot_threshold = 0; out->n_runs = 0;
    // The columns a SHARDED run reconciles inside the epoch (ge_sync_epoch): busy enough that a rank pushes them hard within one epoch.
    // Independent of this handle's worker count (that is about concurrency INSIDE the GPU): count >= N / 20 480 -- what the hub rule
    // gives a full device, 0.25 N / 5 120 -- and at least 256.
    int64_t heavy_thr;
    {
        int64_t div = 20480, floor_n = 256;
        if (const char *e = std::getenv("GE_SYNC_HEAVY_DIV")) div = std::max<int64_t>(1, std::atoll(e));          // experiments (tools/r03/heavy_probe.sh)
        if (const char *e = std::getenv("GE_SYNC_HEAVY_MIN")) floor_n = std::max<int64_t>(1, std::atoll(e));
        // more ranks, more contributors to a row that is summed once per epoch: from four ranks on the set grows with the number of ranks
        // (this handle's share of the rows tells it: 1/8 of them -> twice the divisor).  Six ranks with the eight-rank threshold of the
        // plain rule were 7 % behind the single GPU at epoch 12, with their own 3 % (profiles/r03_six_ranks_hub_threshold.json); the epoch
        // kernel does not mind twice the hub columns on a shard (48.0 ms either way at the bench size).
        const int64_t shards = rq.row_end > rq.row_begin ? std::max<int64_t>(1, (int64_t)V / (int64_t)(rq.row_end - rq.row_begin)) : 1;
        if (shards > 4 && !std::getenv("GE_SYNC_HEAVY_DIV")) div = div * shards / 4;
        heavy_thr = std::max<int64_t>(floor_n, N / div);
    }
    // Hub tiles: which columns go into tiles needs only the counts, and decides which kernel runs and so how many
    // workers are in flight; the flush limits follow from that number.
    int32_t workers = std::max(rq.workers, 1);
    const int32_t G = rq.tile_g;
    std::vector<int32_t> tile_slot;                // [V] group * G + slot of a tile column, else -1; empty: no tiles
    std::vector<int32_t> tcols, tlim;              // per group and slot: column (-1: unused), flush limit
    std::vector<int32_t> hubsR;                    // the hub columns outside the tiles, ascending: the H part
    int32_t n_tgroups = 0;
    out->n_tchunks = 0; out->tile_nnz = 0; out->tile_visits = 0; out->tile_g = 0; out->tile_cols = 0; out->n_tgroups = 0;
    out->n_pchunks = 0; out->panel_nnz = 0; out->panel_visits = 0; out->n_panels = 0; out->panel_cols = 0; out->panel_blocks = 0;
    out->host_prow0.clear(); out->host_ppos.clear();
    int32_t n_panels = 0;                          // hub panels: groups [0, 4 n_panels) of the tile columns
    auto hub_threshold = [&](int32_t wk) -> int64_t {
        int64_t thr = rq.hot_columns == GE_HOT_ALL ? 0
                    : std::max<int64_t>(2, (int64_t)std::ceil(rq.hot_theta * (double)N / (double)std::max(wk, 1)));
        // a shard of a larger run: every column the exchange inside the epoch covers is a hub HERE too, i.e. moved by atomic adds only,
        // so that the other ranks' deltas can be added to it while the epoch kernel runs (the live exchange, sync.hip)
        if (rq.row_end - rq.row_begin < V) thr = std::min(thr, heavy_thr);
        return thr;
    };
    if (N > 0 && rq.hot_columns != GE_HOT_NONE) {
        if (G >= 2) {
            const int64_t thr_t = hub_threshold(rq.workers);
            // Mid-density columns: where the ring kernel walks the panels, hub columns down to density 1 / panel_div
            // are eligible -- for PANELS only: a tile group of four saves less at that density than its extra context loads cost.
            const int64_t div = (!rq.tile_force && rq.panels && G == 4 && rq.panel_div > 8) ? (int64_t)rq.panel_div : 8;
            std::vector<int32_t> el;               // eligible columns, densest first
            for (int32_t v = 0; v < V; ++v)
                if (cnt[(size_t)v] >= thr_t && cnt[(size_t)v] > 0 && (rq.tile_force || (int64_t)cnt[(size_t)v] * div >= (int64_t)rows)) el.push_back(v);
            std::stable_sort(el.begin(), el.end(), [&](int32_t a, int32_t b) { return cnt[(size_t)a] > cnt[(size_t)b]; });
            size_t n_dense = el.size();            // the columns of density >= 1/8 (all of them unless panel_div admits more): a prefix
            if (div > 8) { n_dense = 0; while (n_dense < el.size() && (int64_t)cnt[(size_t)el[n_dense]] * 8 >= (int64_t)rows) ++n_dense; }
            // The sort key is 32 bits wide, and the build counts the nonzeros of every (group, row) in a dense table (4 bytes each, on
            // the device and on the host): bounded under the default gate (columns of density >= 1/8: at most 8 N / rows columns,
            // so at most 2 N pairs), not under GE_LAYOUT_HUB_TILES.  Too large: no tiles by default, an error where they were asked for.
            auto too_large = [&](uint64_t groups) {
                return groups * (uint64_t)rows * (uint64_t)G + (uint64_t)V + (uint64_t)rows >= ((uint64_t)1 << 32) || groups * (uint64_t)rows > ((uint64_t)1 << 28);
            };
            // Of `adm` admitted columns the full sixteens are panels; of the rest only the dense ones stay, as tile groups, and the
            // others go back to the column-major hub chunks.  Past the table's bound the sparsest sixteen are dropped until it
            // holds; with no mid-density column left this is the rule of a handle without them.
            size_t adm = el.size(), n_el = 0;
            for (;;) {
                n_el = std::max(adm / 16 * 16, n_dense);
                if (n_el % (size_t)G == 1) --n_el; // a last group of one column stays with the ordinary hub chunks
                if (adm <= n_dense || !too_large((n_el + (size_t)G - 1) / (size_t)G)) break;
                adm = std::max(n_dense, adm / 16 * 16 - (adm % 16 == 0 ? 16 : 0));
            }
            const uint64_t groups = (n_el + (size_t)G - 1) / (size_t)G;
            if (too_large(groups)) {
                if (rq.tile_force && n_el >= 2)
                    return ge::fail(GE_ERR_ARG, "layout hub_tiles: %llu column groups x %d rows are too many for the tile build (forced tiles are for small matrices)",
                                    (unsigned long long)groups, rows);
                n_el = 0;
            }
            if (n_el >= 2) {
                n_tgroups = (int32_t)groups;
                tile_slot.assign((size_t)V, -1); tcols.assign((size_t)n_tgroups * G, -1); tlim.assign((size_t)n_tgroups * G, LAYOUT_CHUNK);
                // only full panels of four full groups; what is left over stays tile chunks
                if (rq.panels && G == 4) n_panels = (int32_t)(n_el / (size_t)G / 4);
                for (size_t k = 0; k < n_el; ++k) {
                    tile_slot[(size_t)el[k]] = (int32_t)k; tcols[k] = el[k];
                    (k < (size_t)n_panels * 16 ? out->panel_nnz : out->tile_nnz) += cnt[(size_t)el[k]];
                }
                out->n_panels = n_panels; out->panel_cols = n_panels * 16;
                out->tile_g = G; out->tile_cols = (int32_t)n_el - out->panel_cols; out->n_tgroups = n_tgroups;
                workers = std::max(rq.tile_workers, 1);
            }
        }
        // The hub columns are those of the ordinary kernel's worker count whether tiles are built or not: which columns publish
        // by delta does not depend on how the dense ones among them are walked (and a handle sized after this one's threshold, as
        // the replay of bench.py --dump-outputs is, stays what it was).  The flush limits below take the workers that will run.
        const int64_t thr = hub_threshold(rq.workers);
        for (int32_t v = 0; v < V; ++v)
            if (cnt[(size_t)v] >= thr && cnt[(size_t)v] > 0) {
                hubs.push_back(v); out->hot_nnz += cnt[(size_t)v];
                if (tile_slot.empty() || tile_slot[(size_t)v] < 0) { hub_rank[(size_t)v] = (int32_t)hubsR.size(); hubsR.push_back(v); }
            }
        out->hot_cols = (int32_t)hubs.size();
        out->hot_threshold = thr;
    }
    out->workers = workers;
    const int32_t n_hub = (int32_t)hubsR.size();
    const uint32_t tile_keys = (uint32_t)((uint64_t)n_tgroups * (uint64_t)rows * (uint64_t)std::max(G, 1));
    // Concurrent runs on one hub column add their deltas; each delta is stale by the length of the run.  Summing K
    // concurrent runs of m updates behaves like one step K*m times too long and diverges once K*m*(lr*w*|row|^2) passes
    // ~1 (measured: K*m = 39k diverges, 10k is stable at the bench scale).  A hub run is therefore cut -- delta
    // published, row re-read -- every m_j updates with K_j * m_j <= stale_budget, K_j = count_j * workers / N.
    auto flush_limit = [&](int32_t col) -> int32_t {
        if (rq.flush_every > 0) return std::min<int32_t>(rq.flush_every, LAYOUT_CHUNK);
        const double K = std::max(1.0, (double)cnt[(size_t)col] * (double)workers / (double)std::max<int64_t>(N, 1));
        return (int32_t)std::min<double>(LAYOUT_CHUNK, std::max<double>(4.0, std::floor(rq.stale_budget / K)));
    };
    out->flush_min = rq.flush_every > 0 ? std::min<int32_t>(rq.flush_every, LAYOUT_CHUNK) : LAYOUT_CHUNK;
    for (int32_t c : hubs) out->flush_min = std::min(out->flush_min, flush_limit(c));
    if (rq.want_hub_index) { out->hub_index = hub_rank; out->n_hub = n_hub; }
    out->hubs = hubs;
    out->heavy.clear(); out->heavy_count.clear();
    for (int32_t v = 0; v < V; ++v) if (cnt[(size_t)v] >= heavy_thr) { out->heavy.push_back(v); out->heavy_count.push_back(cnt[(size_t)v]); }

    // ---- stable sort: hubs column-major, the rest grouped by row ----
    clk.lap("hub columns (host)");
    int32_t *d_rank = nullptr; uint32_t *d_key = nullptr, *d_skey = nullptr; int32_t *d_val = nullptr, *d_sval = nullptr;
    GE_HIP(tmp.alloc(&d_rank, (size_t)V));
    GE_HIP(tmp.alloc(&d_key, (size_t)N)); GE_HIP(tmp.alloc(&d_skey, (size_t)N));
    GE_HIP(tmp.alloc(&d_val, (size_t)N)); GE_HIP(tmp.alloc(&d_sval, (size_t)N));
    GE_HIP(hipMemcpyAsync(d_rank, hub_rank.data(), sizeof(int32_t) * (size_t)V, hipMemcpyHostToDevice, stream));
    std::vector<int32_t> rcnt((size_t)rows, 0);
    int32_t *d_tslot = nullptr, *d_tcnt = nullptr;
    std::vector<int32_t> tcnt;                           // hub tiles: nonzeros of every (group, row)
    if (n_tgroups > 0) {
        // The staleness rule K m <= stale_budget with the K of a tile: a worker inside ANY chunk of the group holds all its columns,
        // so K_g = group nonzeros * workers / N workers hold column j at once (not count_j * workers / N as in a column-major
        // chunk), each for m of its own updates of j.  One limit per group.
        for (int32_t g = 4 * n_panels; g < n_tgroups; ++g) {      // (a panel's limits follow from its chunks: below, behind the sort)
            int64_t gn = 0;
            for (int s = 0; s < G; ++s) if (tcols[(size_t)g * G + s] >= 0) gn += cnt[(size_t)tcols[(size_t)g * G + s]];
            const double K = std::max(1.0, (double)gn * (double)workers / (double)std::max<int64_t>(N, 1));
            const int32_t m = rq.flush_every > 0 ? std::min<int32_t>(rq.flush_every, LAYOUT_CHUNK)
                                                 : (int32_t)std::min<double>(LAYOUT_CHUNK, std::max<double>(4.0, std::floor(rq.stale_budget / K)));
            for (int s = 0; s < G; ++s) if (tcols[(size_t)g * G + s] >= 0) tlim[(size_t)g * G + s] = m;
            out->flush_min = std::min(out->flush_min, m);
        }
        tcnt.assign((size_t)n_tgroups * (size_t)rows, 0);
        GE_HIP(tmp.alloc(&d_tslot, (size_t)V)); GE_HIP(tmp.alloc(&d_tcnt, tcnt.size()));
        GE_HIP(hipMemcpyAsync(d_tslot, tile_slot.data(), sizeof(int32_t) * (size_t)V, hipMemcpyHostToDevice, stream));
        GE_HIP(hipMemsetAsync(d_tcnt, 0, sizeof(int32_t) * tcnt.size(), stream));
    }
    if (N > 0) {
        hipLaunchKernelGGL(k_sort_keys, dim3(grid_for(N)), dim3(256), 0, stream, dI, dJ, N, rb, d_rank, n_hub, d_key, d_val, d_row,
                           d_tslot, std::max(G, 1), rows, tile_keys, d_tcnt);
        GE_HIP(hipGetLastError());
        if (n_tgroups > 0) GE_HIP(hipMemcpyAsync(tcnt.data(), d_tcnt, sizeof(int32_t) * tcnt.size(), hipMemcpyDeviceToHost, stream));
        unsigned bits = 1;
        while (bits < 32 && ((uint64_t)1 << bits) < (uint64_t)tile_keys + (uint64_t)n_hub + (uint64_t)rows) ++bits;
        size_t tmp_bytes = 0;
        GE_HIP(rocprim::radix_sort_pairs(nullptr, tmp_bytes, d_key, d_skey, d_val, d_sval, (size_t)N, 0, bits, stream));
        void *d_tmp = nullptr;
        GE_HIP(tmp.alloc((char **)&d_tmp, tmp_bytes));
        GE_HIP(rocprim::radix_sort_pairs(d_tmp, tmp_bytes, d_key, d_skey, d_val, d_sval, (size_t)N, 0, bits, stream));
        GE_HIP(hipMemcpyAsync(rcnt.data(), d_row, sizeof(int32_t) * (size_t)rows, hipMemcpyDeviceToHost, stream));
    }
    GE_HIP(hipStreamSynchronize(stream));

    // ---- chunk table ----
    clk.lap("sort");
    const int64_t nP = out->panel_nnz, nT = nP + out->tile_nnz, nH = out->hot_nnz, nR = N - nH;      // positions: panels [0, nP), tiles [nP, nT), other hubs [nT, nH), the rest
    std::vector<int32_t> cfill, cmeta;                   // per chunk: positions in it, meta
    // P: per panel the focus rows in ascending order; a row with a nonzero in any of the four groups belongs to the chunk, and the
    // chunk closes where the next row would take one of the groups past 128 nonzeros.  Runs: every column of the panel is loaded
    // once per chunk; cuts are counted by k_tile_cuts over the (chunk, group) ranges, which are contiguous group by group.
    std::vector<int32_t> prow0{0}, prows, ppos;          // see ge_layout.h
    std::vector<int32_t> sub_start, sub_meta;            // the (chunk, group) ranges in position order, as a chunk table of their own
    std::vector<int64_t> panel_chunks((size_t)n_panels, 0);
    int64_t panel_steps = 0;                             // pipeline steps weighted by their busiest stage (see PANEL_STEP_COST)
    {
        int64_t gbase = 0;                               // first position of the panel's first group
        for (int32_t pn = 0; pn < n_panels; ++pn) {
            int64_t gpos[4], gn[4];
            for (int w = 0; w < 4; ++w) {
                gn[w] = 0;
                for (int s = 0; s < G; ++s) gn[w] += cnt[(size_t)tcols[((size_t)pn * 4 + w) * G + s]];
                gpos[w] = w ? gpos[w - 1] + gn[w - 1] : gbase;
            }
            gbase = gpos[3] + gn[3];
            const size_t first = ppos.size() / 9;
            int32_t fill[4] = {0, 0, 0, 0}; bool open = false;
            auto close = [&]() {
                if (!open) return;
                ppos.push_back(pn);
                for (int w = 0; w < 4; ++w) { ppos.push_back((int32_t)gpos[w]); ppos.push_back(fill[w]); gpos[w] += fill[w]; fill[w] = 0; }
                prow0.push_back((int32_t)prows.size());
                out->n_runs += 4 * G; ++panel_chunks[(size_t)pn];
                open = false;
            };
            const int32_t *tc[4];
            for (int w = 0; w < 4; ++w) tc[w] = tcnt.data() + ((size_t)pn * 4 + w) * (size_t)rows;
            for (int32_t r = 0; r < rows; ++r) {
                const int32_t c[4] = {tc[0][r], tc[1][r], tc[2][r], tc[3][r]};
                if (!(c[0] | c[1] | c[2] | c[3])) continue;
                if (fill[0] + c[0] > LAYOUT_CHUNK || fill[1] + c[1] > LAYOUT_CHUNK || fill[2] + c[2] > LAYOUT_CHUNK || fill[3] + c[3] > LAYOUT_CHUNK) close();
                for (int w = 0; w < 4; ++w) fill[w] += c[w];
                prows.push_back(rb + r); open = true; ++out->panel_visits;
                panel_steps += std::max(std::max(c[0], c[1]), std::max(c[2], c[3]));
            }
            close();
            for (int w = 0; w < 4; ++w)                  // this panel's ranges, group by group
                for (size_t c = first; c < ppos.size() / 9; ++c) { sub_start.push_back(ppos[c * 9 + 1 + 2 * w]); sub_meta.push_back(pn * 4 + w); }
            if (gpos[3] != gbase) return ge::fail(GE_ERR_STATE, "internal: panel %d covers %lld of its positions", pn, (long long)(gpos[3] - gbase));
        }
        sub_start.push_back((int32_t)nP);
        if (gbase != nP) return ge::fail(GE_ERR_STATE, "internal: panel counts cover %lld of %lld nonzeros", (long long)gbase, (long long)nP);
    }
    out->n_pchunks = (int64_t)ppos.size() / 9;
    if (n_panels > 0) {
        // Workgroups that start in the panel loop: the panels' share of the epoch's time (see PANEL_STEP_COST), unless the caller
        // names the number.
        int32_t pb = rq.panel_blocks;
        const double w_panels = PANEL_STEP_COST * (double)(panel_steps + 3 * out->n_pchunks), w_main = (double)(N - nP) / 4.0;
        if (clk.on) std::fprintf(stderr, "[ge_glove_create]   layout: panel steps %lld, chunks %lld, main nonzeros %lld\n", (long long)panel_steps, (long long)out->n_pchunks, (long long)(N - nP));
        if (pb <= 0) pb = (int32_t)std::lround(w_panels / std::max(w_panels + w_main, 1.0) * (double)rq.blocks);
        out->panel_blocks = std::max(1, std::min(pb, std::max(rq.blocks, 1)));
        if (clk.on) std::fprintf(stderr, "[ge_glove_create]   layout: %d panels, %d of %d workgroups start in the panel loop\n", n_panels, out->panel_blocks, rq.blocks);
        // The staleness rule with the K of a panel: every block inside the panel holds all its columns, and of the blocks in the
        // panel loop the panel's share of the panel chunks are inside it.
        for (int32_t pn = 0; pn < n_panels; ++pn) {
            const double K = std::max(1.0, (double)out->panel_blocks * (double)panel_chunks[(size_t)pn] / (double)std::max<int64_t>(out->n_pchunks, 1));
            const int32_t m = rq.flush_every > 0 ? std::min<int32_t>(rq.flush_every, LAYOUT_CHUNK)
                                                 : (int32_t)std::min<double>(LAYOUT_CHUNK, std::max<double>(4.0, std::floor(rq.stale_budget / K)));
            for (int k = 0; k < 16; ++k) tlim[(size_t)pn * 16 + k] = m;
            out->flush_min = std::min(out->flush_min, m);
        }
    }
    // T: per group the focus rows in ascending order, packed whole; a chunk closes where the next row would overflow it.
    // Runs: the worker loads every column of the group once per chunk (counted here); a column is published and re-read when
    // it has taken its limit of updates since it was last read (counted by k_tile_cuts once the chunks are placed).
    {
        int64_t placed = nP;
        for (int32_t g = 4 * n_panels; g < n_tgroups; ++g) {
            int32_t used = 0;
            for (int s = 0; s < G; ++s) if (tcols[(size_t)g * G + s] >= 0) ++used;
            int32_t fill = 0;
            auto close = [&]() {
                if (!fill) return;
                cfill.push_back(fill); cmeta.push_back(g);
                out->n_runs += used;
                fill = 0;
            };
            const int32_t *tc = tcnt.data() + (size_t)g * (size_t)rows;
            for (int32_t r = 0; r < rows; ++r) {
                const int32_t c = tc[r];
                if (!c) continue;
                if (fill + c > LAYOUT_CHUNK) close();
                fill += c; placed += c; ++out->tile_visits;
            }
            close();
        }
        if (placed != nT) return ge::fail(GE_ERR_STATE, "internal: tile counts cover %lld of %lld nonzeros", (long long)placed, (long long)nT);
    }
    out->n_tchunks = (int64_t)cfill.size();
    // H: fixed cuts; a chunk's flush limit is the smallest limit among the columns inside it
    {
        int64_t pos = nT; size_t hc = 0; int64_t col_end = nT + (n_hub ? cnt[(size_t)hubsR[0]] : 0);
        while (pos < nH) {
            const int64_t end = std::min<int64_t>(pos + LAYOUT_CHUNK, nH);
            int32_t m = LAYOUT_CHUNK;
            int64_t q = pos;
            int32_t seg[LAYOUT_CHUNK]; int n_seg = 0;      // nonzeros of each column inside the chunk
            while (q < end) {
                while (col_end <= q) { ++hc; col_end += cnt[(size_t)hubsR[hc]]; }
                m = std::min(m, flush_limit(hubsR[hc]));
                const int64_t q2 = std::min(end, col_end);
                seg[n_seg++] = (int32_t)(q2 - q);
                q = q2;
            }
            for (int k = 0; k < n_seg; ++k) out->n_runs += (seg[k] + m - 1) / m;     // a run per column, cut every m nonzeros
            cfill.push_back((int32_t)(end - pos)); cmeta.push_back(m);
            pos = end;
        }
    }
    out->n_hchunks = (int64_t)cfill.size() - out->n_tchunks;
    // R: rows packed whole (best fit over a few open chunks); a long row takes consecutive chunks of its own and leaves
    // its last, partial one open for whole rows behind it
    std::vector<int32_t> row_src((size_t)rows), row_chunk((size_t)rows, -1), row_off((size_t)rows, 0);
    out->long_rows = 0; out->shared_chunks = 0;
    {
        int64_t src = 0;
        constexpr int OPEN = 16;
        int32_t open[OPEN]; int n_open = 0;
        int32_t cur = -1;                                 // pack_rows == 0: the one chunk being filled
        for (int32_t r = 0; r < rows; ++r) {
            row_src[(size_t)r] = (int32_t)src;
            const int32_t len = rcnt[(size_t)r];
            src += len;
            if (len == 0) continue;
            if (!rq.pack_rows) {                          // round-1 layout: cut every 128 positions, rows may straddle chunks
                if (cur < 0 || cfill[(size_t)cur] == LAYOUT_CHUNK) { cur = (int32_t)cfill.size(); cfill.push_back(0); cmeta.push_back(-1); }
                row_chunk[(size_t)r] = cur; row_off[(size_t)r] = cfill[(size_t)cur];
                int32_t left = len;
                while (left > 0) {
                    if (cfill[(size_t)cur] == LAYOUT_CHUNK) { cur = (int32_t)cfill.size(); cfill.push_back(0); cmeta.push_back(-1); }
                    const int32_t take = std::min(left, LAYOUT_CHUNK - cfill[(size_t)cur]);
                    cfill[(size_t)cur] += take; left -= take; ++out->n_runs;
                }
                continue;
            }
            if (len > LAYOUT_CHUNK) {
                ++out->long_rows;
                const int32_t id = rq.shared_rows ? rb + r : -1;
                row_chunk[(size_t)r] = (int32_t)cfill.size(); row_off[(size_t)r] = 0;
                int32_t left = len;
                while (left > 0) {
                    const int32_t take = std::min(left, LAYOUT_CHUNK);
                    cfill.push_back(take); cmeta.push_back(id); ++out->shared_chunks; ++out->n_runs;
                    left -= take;
                }
                if (cfill.back() < LAYOUT_CHUNK) {        // the partial last piece stays open
                    if (n_open == OPEN) { int f = 0; for (int o = 1; o < OPEN; ++o) if (cfill[(size_t)open[o]] > cfill[(size_t)open[f]]) f = o; open[f] = open[--n_open]; }
                    open[n_open++] = (int32_t)cfill.size() - 1;
                }
                continue;
            }
            int best = -1;
            for (int o = 0; o < n_open; ++o) {
                const int32_t room = LAYOUT_CHUNK - cfill[(size_t)open[o]];
                if (room >= len && (best < 0 || room < LAYOUT_CHUNK - cfill[(size_t)open[best]])) best = o;
            }
            if (best < 0) {
                if (n_open == OPEN) { int f = 0; for (int o = 1; o < OPEN; ++o) if (cfill[(size_t)open[o]] > cfill[(size_t)open[f]]) f = o; open[f] = open[--n_open]; }
                open[n_open] = (int32_t)cfill.size(); best = n_open++;
                cfill.push_back(0); cmeta.push_back(-1);
            }
            const int32_t c = open[best];
            row_chunk[(size_t)r] = c; row_off[(size_t)r] = cfill[(size_t)c];
            cfill[(size_t)c] += len; ++out->n_runs;
            if (cfill[(size_t)c] == LAYOUT_CHUNK) open[best] = open[--n_open];
        }
        if (src != nR) return ge::fail(GE_ERR_STATE, "internal: row counts cover %lld of %lld nonzeros", (long long)src, (long long)nR);
    }
    const int64_t n_chunks = (int64_t)cfill.size();
    std::vector<int32_t> cstart((size_t)n_chunks + 1);
    {
        int64_t pos = nP;                               // (the panel chunks lie in front of the chunk table's positions)
        for (int64_t c = 0; c < n_chunks; ++c) { cstart[(size_t)c] = (int32_t)pos; pos += cfill[(size_t)c]; }
        cstart[(size_t)n_chunks] = (int32_t)pos;
        if (pos != N) return ge::fail(GE_ERR_STATE, "internal: chunks cover %lld of %lld nonzeros", (long long)pos, (long long)N);
    }
    std::vector<int32_t> row_dst((size_t)rows, 0);
    for (int32_t r = 0; r < rows; ++r) if (row_chunk[(size_t)r] >= 0) row_dst[(size_t)r] = cstart[(size_t)row_chunk[(size_t)r]] + row_off[(size_t)r];

    // ---- placement ----
    clk.lap("chunk table (host)");
    int32_t *d_src = nullptr, *d_dst = nullptr;
    GE_HIP(tmp.alloc(&d_src, (size_t)rows)); GE_HIP(tmp.alloc(&d_dst, (size_t)rows));
    GE_HIP(hipMemcpyAsync(d_src, row_src.data(), sizeof(int32_t) * (size_t)rows, hipMemcpyHostToDevice, stream));
    GE_HIP(hipMemcpyAsync(d_dst, row_dst.data(), sizeof(int32_t) * (size_t)rows, hipMemcpyHostToDevice, stream));
    const size_t np = (size_t)std::max<int64_t>(N, 1);
    hipError_t e = hipMalloc((void **)&out->bA, sizeof(int32_t) * np);
    if (e == hipSuccess) e = hipMalloc((void **)&out->bB, sizeof(int32_t) * np);
    if (e == hipSuccess) e = hipMalloc((void **)&out->border, sizeof(int32_t) * np);
    if (e == hipSuccess) e = hipMalloc((void **)&out->L, sizeof(double) * np);
    if (e == hipSuccess) e = hipMalloc((void **)&out->W, sizeof(float) * np);
    if (e == hipSuccess) e = hipMalloc((void **)&out->cstart, sizeof(int32_t) * ((size_t)n_chunks + 1));
    if (e == hipSuccess) e = hipMalloc((void **)&out->cmeta, sizeof(int32_t) * (size_t)std::max<int64_t>(n_chunks, 1));
    if (e == hipSuccess) e = hipMemcpyAsync(out->cstart, cstart.data(), sizeof(int32_t) * ((size_t)n_chunks + 1), hipMemcpyHostToDevice, stream);
    if (e == hipSuccess && n_chunks) e = hipMemcpyAsync(out->cmeta, cmeta.data(), sizeof(int32_t) * (size_t)n_chunks, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess && N > 0) {
        hipLaunchKernelGGL(k_place, dim3(grid_for(N)), dim3(256), 0, stream, dI, dJ, dX, N, rb, d_skey, d_sval, n_hub, nH, d_src, d_dst,
                           rq.cost, rq.xmax, out->bA, out->bB, out->L, out->W, out->border, tile_keys, std::max(G, 1));
        e = hipGetLastError();
    }
    unsigned long long cuts = 0, *d_cuts = nullptr;
    if (e == hipSuccess && n_tgroups > 0) {
        e = hipMalloc((void **)&out->tcols, sizeof(int32_t) * tcols.size());
        if (e == hipSuccess) e = hipMalloc((void **)&out->tlim, sizeof(int32_t) * tlim.size());
        if (e == hipSuccess) e = tmp.alloc(&d_cuts, 1);
        if (e == hipSuccess) e = hipMemcpyAsync(out->tcols, tcols.data(), sizeof(int32_t) * tcols.size(), hipMemcpyHostToDevice, stream);
        if (e == hipSuccess) e = hipMemcpyAsync(out->tlim, tlim.data(), sizeof(int32_t) * tlim.size(), hipMemcpyHostToDevice, stream);
        if (e == hipSuccess) e = hipMemsetAsync(d_cuts, 0, sizeof(unsigned long long), stream);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_tile_cuts, dim3(grid_for(out->n_tchunks)), dim3(256), 0, stream, out->bB, out->cstart, out->cmeta, out->tlim,
                               out->n_tchunks, G, d_cuts);
            e = hipGetLastError();
        }
        if (e == hipSuccess && n_panels > 0) {
            int32_t *d_ss = nullptr, *d_sm = nullptr;
            e = tmp.alloc(&d_ss, sub_start.size());
            if (e == hipSuccess) e = tmp.alloc(&d_sm, sub_meta.size());
            if (e == hipSuccess) e = hipMalloc((void **)&out->prow0, sizeof(int32_t) * prow0.size());
            if (e == hipSuccess) e = hipMalloc((void **)&out->prows, sizeof(int32_t) * std::max<size_t>(prows.size(), 1));
            if (e == hipSuccess) e = hipMalloc((void **)&out->ppos, sizeof(int32_t) * std::max<size_t>(ppos.size(), 1));
            if (e == hipSuccess) e = hipMemcpyAsync(d_ss, sub_start.data(), sizeof(int32_t) * sub_start.size(), hipMemcpyHostToDevice, stream);
            if (e == hipSuccess && !sub_meta.empty()) e = hipMemcpyAsync(d_sm, sub_meta.data(), sizeof(int32_t) * sub_meta.size(), hipMemcpyHostToDevice, stream);
            if (e == hipSuccess) e = hipMemcpyAsync(out->prow0, prow0.data(), sizeof(int32_t) * prow0.size(), hipMemcpyHostToDevice, stream);
            if (e == hipSuccess && !prows.empty()) e = hipMemcpyAsync(out->prows, prows.data(), sizeof(int32_t) * prows.size(), hipMemcpyHostToDevice, stream);
            if (e == hipSuccess && !ppos.empty()) e = hipMemcpyAsync(out->ppos, ppos.data(), sizeof(int32_t) * ppos.size(), hipMemcpyHostToDevice, stream);
            if (e == hipSuccess && !sub_meta.empty()) {      // the cuts of the panel chunks: the same count over their (chunk, group) ranges
                hipLaunchKernelGGL(k_tile_cuts, dim3(grid_for((int64_t)sub_meta.size())), dim3(256), 0, stream, out->bB, d_ss, d_sm, out->tlim,
                                   (int64_t)sub_meta.size(), G, d_cuts);
                e = hipGetLastError();
            }
        }
        if (e == hipSuccess) e = hipMemcpyAsync(&cuts, d_cuts, sizeof(cuts), hipMemcpyDeviceToHost, stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    out->n_runs += (int64_t)cuts;
    clk.lap("placement kernel");
    if (e != hipSuccess) {
        out->release();
        return ge::fail(e == hipErrorOutOfMemory ? GE_ERR_OOM : GE_ERR_HIP, "blocked layout build failed: %s", hipGetErrorString(e));
    }
    out->P = N; out->n_chunks = n_chunks;
    out->host_prow0.swap(prow0); out->host_ppos.swap(ppos);
    return GE_OK;
}

}  // namespace ge
