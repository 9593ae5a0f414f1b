// synth.hip -- the synthetic co-occurrence matrix of SURVEY.md 8(d), generated on the device (ge_synth_coo; the recipe is
// written out in include/geglove.h).  Integer and bit operations only, so tests/synth_ref.py holds the result to the last bit.
//
// The matrix is the diagonal of the owned rows plus the first M = nnz - rows distinct valid keys (i, j) of a counter-based
// stream of draws t = 0, 1, ...  The draws are taken in RANGES [T0, T1); per range, all on the caller's stream:
//   k_draw          one draw per thread: three SplitMix64 values, the relabel gather, key = (i - row_begin) * V + j (64 bit;
//                   a void draw gets the sentinel rows * V, one past the largest key); value = t
//   radix_sort_pairs (rocPRIM, stable, on the key bits only) of  [what is kept so far | the range]:  among equal keys the
//                   kept entry, else the smallest t, comes first -- the key's first occurrence
//   k_heads         flags the first entry of every run of equal keys and marks its draw in a flag array indexed by t - T0
//   inclusive_scan  over those flags in t order: the draw at which the count reaches what is still missing is the cut t*
//   too few:        the first occurrences are compacted into the new kept list and the next range is drawn
//   enough:         k_heads again with t <= t*, exclusive_scan, k_emit writes I, J, X (X recomputed from t, never stored).
// The diagonal enters as kept entries with t = -1, so it is merged by the same sort.  Which ranges were drawn does not show in
// the result: it is a function of the arguments alone.
// Roofline: HBM streaming; the radix sort of 16-byte pairs dominates.  Peak device memory: 32 bytes per
// sorted entry (two buffers of key + t; the scans live in the idle buffer) + 12 per nonzero of the result + 4 V.
#include "ge_coo.h"

#include <cstring>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

namespace {

constexpr uint64_t SM_GOLD = 0x9E3779B97F4A7C15ull;

// the (n+1)-th output of SplitMix64 seeded with `seed`
__host__ __device__ __forceinline__ uint64_t splitmix_at(uint64_t seed, uint64_t n) {
    uint64_t z = seed + (n + 1) * SM_GOLD;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

struct Recipe {
    uint64_t sigma;          // the shard's stream
    int32_t V, row_begin, rows, B;
    uint64_t sentinel;       // rows * V
};

__global__ __launch_bounds__(256) void k_relabel_keys(uint64_t seed, int32_t V, uint64_t *key, int32_t *val) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < V; v += stride) { key[v] = splitmix_at(seed, (uint64_t)v); val[v] = (int32_t)v; }
}

__global__ __launch_bounds__(256) void k_diagonal(Recipe rc, uint64_t *key, int64_t *val) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < rc.rows; r += stride) {
        key[r] = (uint64_t)r * (uint64_t)rc.V + (uint64_t)(rc.row_begin + r);
        val[r] = -1;
    }
}

// draws [T0, T0 + R) -> key[q], val[q] = t for q = t - T0
__global__ __launch_bounds__(256) void k_draw(Recipe rc, const int32_t *relabel, int64_t T0, int64_t R, uint64_t *key, int64_t *val) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < R; q += stride) {
        const uint64_t t = (uint64_t)(T0 + q);
        const uint64_t a = splitmix_at(rc.sigma, t), b = splitmix_at(rc.sigma ^ 0x5A5A5A5Aull, t);
        const uint32_t ri = (uint32_t)(((a >> 32) * (uint64_t)rc.rows) >> 32);                 // < rows
        const uint32_t k = (uint32_t)(((b >> 32) * (uint64_t)rc.B) >> 32);                      // < B <= 31
        const uint32_t lo = (uint32_t)b;
        const uint32_t r = k == 0 ? 0u : ((1u << k) - 1u) + (lo >> (32u - k));                  // never a shift by 32
        uint64_t kk = rc.sentinel;
        if (r < (uint32_t)rc.V) {
            const int32_t j = relabel[r];
            if (j != rc.row_begin + (int32_t)ri) kk = (uint64_t)ri * (uint64_t)rc.V + (uint64_t)j;
        }
        key[q] = kk; val[q] = (int64_t)t;
    }
}

// head[p] = 1 where sorted entry p is the first of its key, is no void draw and was drawn at t <= t_max; such a draw of this
// range also sets flag[t - T0] (flag: zeroed by the caller, or null)
__global__ __launch_bounds__(256) void k_heads(const uint64_t *skey, const int64_t *sval, int64_t n, uint64_t sentinel, int64_t T0, int64_t t_max,
                                               uint32_t *head, uint32_t *flag) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += stride) {
        const uint64_t k = skey[p];
        const int64_t t = sval[p];
        const bool h = k != sentinel && (p == 0 || skey[p - 1] != k) && t <= t_max;
        head[p] = h ? 1u : 0u;
        if (h && flag && t >= T0) flag[t - T0] = 1u;
    }
}

// the draw at which the running count of new keys reaches `need` (>= 1): exactly one q has flag[q] and cum[q] == need
__global__ __launch_bounds__(256) void k_find_cut(const uint32_t *flag, const uint32_t *cum, int64_t R, uint32_t need, int64_t *out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < R; q += stride)
        if (flag[q] && cum[q] == need) *out = q;
}

__global__ __launch_bounds__(256) void k_compact(const uint64_t *skey, const int64_t *sval, const uint32_t *head, const uint32_t *pos, int64_t n,
                                                 uint64_t *okey, int64_t *oval) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += stride)
        if (head[p]) { okey[pos[p]] = skey[p]; oval[pos[p]] = sval[p]; }
}

// pos[p] < nnz for every head (the caller checked the total)
__global__ __launch_bounds__(256) void k_emit(Recipe rc, const uint64_t *skey, const int64_t *sval, const uint32_t *head, const uint32_t *pos, int64_t n,
                                              int32_t *I, int32_t *J, float *X) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += stride) {
        if (!head[p]) continue;
        const uint64_t k = skey[p];
        const int64_t t = sval[p];
        float x = 0.2f;                                                                         // the diagonal
        if (t >= 0) {
            const uint64_t c = splitmix_at(rc.sigma ^ 0x0F0F0F0Full, (uint64_t)t);
            const uint32_t e = 3u + (uint32_t)(((c >> 32) * 10ull) >> 32);
            x = fminf(__uint_as_float(((127u - e) << 23) | (uint32_t)(c & 0x7FFFFFull)), 0.2f);
        }
        const uint32_t o = pos[p];
        I[o] = rc.row_begin + (int32_t)(k / (uint64_t)rc.V); J[o] = (int32_t)(k % (uint64_t)rc.V); X[o] = x;
    }
}

int grid_for(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 16384)); }

// every device buffer of one ge_synth_coo call: frees what is left, remembers the most that was held at once
struct Pool {
    std::vector<std::pair<void *, size_t>> live;
    size_t held = 0, peak = 0;
    ~Pool() { for (auto &q : live) (void)hipFree(q.first); }
    template <typename T> hipError_t alloc(T **out, size_t n) {
        const size_t bytes = sizeof(T) * std::max<size_t>(n, 1);
        const hipError_t e = hipMalloc((void **)out, bytes);
        if (e == hipSuccess) { live.emplace_back((void *)*out, bytes); held += bytes; peak = std::max(peak, held); }
        return e;
    }
    void free(void *q) {
        for (size_t k = 0; k < live.size(); ++k) if (live[k].first == q) { held -= live[k].second; (void)hipFree(q); live.erase(live.begin() + (long)k); return; }
    }
    void release(void *q) {      // the caller keeps q
        for (size_t k = 0; k < live.size(); ++k) if (live[k].first == q) { live.erase(live.begin() + (long)k); return; }
    }
};

// device time between start() and stop(), summed over the stretches of one call
struct DeviceTime {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipStream_t stream = nullptr;
    float ms = 0.0f;
    ~DeviceTime() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
    hipError_t start() { return hipEventRecord(e0, stream); }
    hipError_t stop() {          // drains the stream
        hipError_t e = hipEventRecord(e1, stream);
        if (e == hipSuccess) e = hipEventSynchronize(e1);
        float d = 0.0f;
        if (e == hipSuccess) e = hipEventElapsedTime(&d, e0, e1);
        ms += d;
        return e;
    }
};

unsigned bit_length(uint64_t v) { unsigned b = 0; while (v) { ++b; v >>= 1; } return b; }

ge_status check_args(const ge_synth_cfg *cfg, int32_t *rb_out, int32_t *re_out) {
    if (!cfg) return ge::fail(GE_ERR_ARG, "cfg is null");
    const int32_t V = cfg->vocab_size;
    if (V < 1) return ge::fail(GE_ERR_ARG, "vocab_size must be >= 1 (got %d)", V);
    int32_t rb = cfg->row_begin, re = cfg->row_end;
    if (rb == 0 && re == 0) re = V;
    if (rb < 0 || rb >= re || re > V) return ge::fail(GE_ERR_ARG, "invalid row range [%d,%d) for vocab_size %d", rb, re, V);
    const int64_t rows = re - rb;
    if (cfg->nnz < rows || cfg->nnz > 0x7FFFFFFFLL)
        return ge::fail(GE_ERR_ARG, "nnz out of range: %lld (the diagonal of %lld rows is part of it; nnz < 2^31)", (long long)cfg->nnz, (long long)rows);
    if (cfg->nnz - rows > rows * ((int64_t)V - 1))
        return ge::fail(GE_ERR_ARG, "nnz %lld exceeds the %lld cells of %lld rows x %d columns", (long long)cfg->nnz, (long long)(rows * (int64_t)V), (long long)rows, V);
    *rb_out = rb; *re_out = re;
    return GE_OK;
}

ge_status synth_impl(const ge_synth_cfg *cfg, ge_coo **out) {
    if (!out) return ge::fail(GE_ERR_ARG, "out is null");
    *out = nullptr;
    int32_t rb = 0, re = 0;
    GE_CHECK(check_args(cfg, &rb, &re));
    GE_CHECK(ge::select_device(cfg->device));
    const hipStream_t stream = (hipStream_t)cfg->stream;
    const int32_t V = cfg->vocab_size, rows = re - rb;
    const int64_t nnz = cfg->nnz, M = nnz - rows;
    const int64_t budget = 8 * M + 1024;
    Recipe rc{};
    rc.sigma = cfg->seed + 0x1000003ull * (uint64_t)(rb + 1);
    rc.V = V; rc.row_begin = rb; rc.rows = rows; rc.B = (int32_t)bit_length((uint64_t)V);
    rc.sentinel = (uint64_t)rows * (uint64_t)V;
    const unsigned key_bits = std::max(1u, bit_length(rc.sentinel));

    Pool pool;
    DeviceTime clock;
    clock.stream = stream;
    GE_HIP(hipEventCreate(&clock.e0));
    GE_HIP(hipEventCreate(&clock.e1));

    // ---- the relabelling: argsort of V SplitMix64 values, stable ----
    int32_t *relabel = nullptr;
    {
        uint64_t *k_in = nullptr, *k_out = nullptr; int32_t *v_in = nullptr; void *tmp = nullptr;
        GE_HIP(pool.alloc(&relabel, (size_t)V));
        GE_HIP(pool.alloc(&k_in, (size_t)V)); GE_HIP(pool.alloc(&k_out, (size_t)V)); GE_HIP(pool.alloc(&v_in, (size_t)V));
        size_t tmp_bytes = 0;
        GE_HIP(rocprim::radix_sort_pairs(nullptr, tmp_bytes, k_in, k_out, v_in, relabel, (size_t)V, 0, 64, stream));
        GE_HIP(pool.alloc((char **)&tmp, tmp_bytes));
        GE_HIP(clock.start());
        hipLaunchKernelGGL(k_relabel_keys, dim3(grid_for(V)), dim3(256), 0, stream, cfg->seed ^ 0x77777777ull, V, k_in, v_in);
        GE_HIP(hipGetLastError());
        GE_HIP(rocprim::radix_sort_pairs(tmp, tmp_bytes, k_in, k_out, v_in, relabel, (size_t)V, 0, 64, stream));
        GE_HIP(clock.stop());
        pool.free(tmp); pool.free(k_in); pool.free(k_out); pool.free(v_in);
    }

    // ---- kept so far: the diagonal, t = -1 ----
    uint64_t *kept_key = nullptr; int64_t *kept_val = nullptr;
    int64_t kept = rows;
    GE_HIP(pool.alloc(&kept_key, (size_t)kept)); GE_HIP(pool.alloc(&kept_val, (size_t)kept));
    GE_HIP(clock.start());
    hipLaunchKernelGGL(k_diagonal, dim3(grid_for(rows)), dim3(256), 0, stream, rc, kept_key, kept_val);
    GE_HIP(hipGetLastError());
    GE_HIP(clock.stop());

    int32_t *dI = nullptr, *dJ = nullptr; float *dX = nullptr;
    int64_t T = 0, draws = 0;
    // the first range from M with the margin measured at the C2 shape (1.25 draws per key); later ranges from what is missing
    const int64_t first = std::min<int64_t>(budget, M + M / 4 + 1024);
    constexpr int64_t RANGE_MAX = (int64_t)1 << 30;              // entries of one range: the scans count in 32 bits
    for (;;) {
        const int64_t need = nnz - kept;                         // > 0 except for M = 0, which draws nothing
        int64_t R = 0;
        if (need > 0) {
            if (T >= budget)
                return ge::fail(GE_ERR_ARG, "too dense: %lld of %lld distinct keys within the budget of %lld draws (V %d, rows %d)",
                                (long long)(kept - rows), (long long)M, (long long)budget, V, rows);
            R = T == 0 ? first : std::max<int64_t>(2 * need + 1024, first / 4);
            R = std::min<int64_t>(std::min<int64_t>(R, budget - T), RANGE_MAX);
        }
        const int64_t n = kept + R;
        uint64_t *kA = nullptr, *kB = nullptr; int64_t *vA = nullptr, *vB = nullptr; void *tmp = nullptr;
        GE_HIP(pool.alloc(&kA, (size_t)n)); GE_HIP(pool.alloc(&vA, (size_t)n));
        GE_HIP(pool.alloc(&kB, (size_t)n)); GE_HIP(pool.alloc(&vB, (size_t)n));
        rocprim::double_buffer<uint64_t> keys(kA, kB);
        rocprim::double_buffer<int64_t> vals(vA, vB);
        size_t sort_bytes = 0, scan_bytes = 0, scan2_bytes = 0;
        GE_HIP(rocprim::radix_sort_pairs(nullptr, sort_bytes, keys, vals, (size_t)n, 0, key_bits, stream));
        GE_HIP(rocprim::inclusive_scan(nullptr, scan_bytes, (uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)std::max<int64_t>(R, 1), rocprim::plus<uint32_t>(), stream));
        GE_HIP(rocprim::exclusive_scan(nullptr, scan2_bytes, (uint32_t *)nullptr, (uint32_t *)nullptr, 0u, (size_t)n, rocprim::plus<uint32_t>(), stream));
        const size_t tmp_bytes = std::max(sort_bytes, std::max(scan_bytes, scan2_bytes));
        GE_HIP(pool.alloc((char **)&tmp, tmp_bytes));
        int64_t *d_cut = nullptr;
        GE_HIP(pool.alloc(&d_cut, 1));

        GE_HIP(clock.start());
        GE_HIP(hipMemcpyAsync(kA, kept_key, sizeof(uint64_t) * (size_t)kept, hipMemcpyDeviceToDevice, stream));
        GE_HIP(hipMemcpyAsync(vA, kept_val, sizeof(int64_t) * (size_t)kept, hipMemcpyDeviceToDevice, stream));
        if (R > 0) {
            hipLaunchKernelGGL(k_draw, dim3(grid_for(R)), dim3(256), 0, stream, rc, relabel, T, R, kA + kept, vA + kept);
            GE_HIP(hipGetLastError());
        }
        size_t sb = tmp_bytes;
        GE_HIP(rocprim::radix_sort_pairs(tmp, sb, keys, vals, (size_t)n, 0, key_bits, stream));
        const uint64_t *skey = keys.current(); const int64_t *sval = vals.current();
        // the idle buffers hold the scans: head | pos (n each) in the keys' one, flag | cum (R each) in the values' one
        uint32_t *head = reinterpret_cast<uint32_t *>(keys.alternate()), *pos = head + n;
        uint32_t *flag = reinterpret_cast<uint32_t *>(vals.alternate()), *cum = flag + R;
        uint32_t new_keys = 0;
        if (R > 0) {
            GE_HIP(hipMemsetAsync(flag, 0, sizeof(uint32_t) * (size_t)R, stream));
            hipLaunchKernelGGL(k_heads, dim3(grid_for(n)), dim3(256), 0, stream, skey, sval, n, rc.sentinel, T, INT64_MAX, head, flag);
            GE_HIP(hipGetLastError());
            sb = tmp_bytes;
            GE_HIP(rocprim::inclusive_scan(tmp, sb, flag, cum, (size_t)R, rocprim::plus<uint32_t>(), stream));
            GE_HIP(hipMemcpyAsync(&new_keys, cum + (R - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        }
        GE_HIP(clock.stop());

        const bool enough = (int64_t)new_keys >= need;
        int64_t t_cut = INT64_MAX;                               // not enough: every first occurrence of the range is kept (head as it stands)
        if (enough) {
            int64_t q = -1;
            if (need > 0) {
                GE_HIP(clock.start());
                GE_HIP(hipMemsetAsync(d_cut, 0xFF, sizeof(int64_t), stream));
                hipLaunchKernelGGL(k_find_cut, dim3(grid_for(R)), dim3(256), 0, stream, flag, cum, R, (uint32_t)need, d_cut);
                GE_HIP(hipGetLastError());
                GE_HIP(hipMemcpyAsync(&q, d_cut, sizeof(int64_t), hipMemcpyDeviceToHost, stream));
                GE_HIP(clock.stop());
                if (q < 0 || q >= R) return ge::fail(GE_ERR_STATE, "internal: no cut among %lld draws", (long long)R);
            }
            t_cut = T + q;
            draws = t_cut + 1;
        }
        GE_HIP(clock.start());
        if (enough) {                                            // the heads again, now only up to the cut
            hipLaunchKernelGGL(k_heads, dim3(grid_for(n)), dim3(256), 0, stream, skey, sval, n, rc.sentinel, T, t_cut, head, (uint32_t *)nullptr);
            GE_HIP(hipGetLastError());
        }
        sb = tmp_bytes;
        GE_HIP(rocprim::exclusive_scan(tmp, sb, head, pos, 0u, (size_t)n, rocprim::plus<uint32_t>(), stream));
        uint32_t last[2] = {0, 0};
        GE_HIP(hipMemcpyAsync(&last[0], pos + (n - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        GE_HIP(hipMemcpyAsync(&last[1], head + (n - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        GE_HIP(clock.stop());
        const int64_t total = (int64_t)last[0] + (int64_t)last[1];
        if (total != (enough ? nnz : kept + (int64_t)new_keys))
            return ge::fail(GE_ERR_STATE, "internal: %lld distinct keys where %lld were counted", (long long)total, (long long)(enough ? nnz : kept + (int64_t)new_keys));
        pool.free(kept_key); pool.free(kept_val); kept_key = nullptr; kept_val = nullptr;
        if (enough) {
            GE_HIP(pool.alloc(&dI, (size_t)nnz)); GE_HIP(pool.alloc(&dJ, (size_t)nnz)); GE_HIP(pool.alloc(&dX, (size_t)nnz));
            GE_HIP(clock.start());
            hipLaunchKernelGGL(k_emit, dim3(grid_for(n)), dim3(256), 0, stream, rc, skey, sval, head, pos, n, dI, dJ, dX);
            GE_HIP(hipGetLastError());
            GE_HIP(clock.stop());
            break;
        }
        GE_HIP(pool.alloc(&kept_key, (size_t)total)); GE_HIP(pool.alloc(&kept_val, (size_t)total));
        GE_HIP(clock.start());
        hipLaunchKernelGGL(k_compact, dim3(grid_for(n)), dim3(256), 0, stream, skey, sval, head, pos, n, kept_key, kept_val);
        GE_HIP(hipGetLastError());
        GE_HIP(clock.stop());
        kept = total;
        T += R;
        pool.free(tmp); pool.free(d_cut); pool.free(kA); pool.free(kB); pool.free(vA); pool.free(vB);
    }

    std::unique_ptr<ge_coo> c(new (std::nothrow) ge_coo());
    if (!c) return ge::fail(GE_ERR_OOM, "host allocation failed");
    pool.release(dI); pool.release(dJ); pool.release(dX);
    c->dI = dI; c->dJ = dJ; c->dX = dX;
    c->nnz = nnz; c->V = V; c->max = (double)0.2f;
    c->device = cfg->device; c->row_begin = rb; c->row_end = re;
    c->host_ready = false;
    c->draws = draws; c->kernel_ms = clock.ms; c->peak_bytes = (int64_t)pool.peak;
    *out = c.release();
    return GE_OK;
}

}  // namespace

// the arrays of a device-resident result, copied down once; row_ptr from I (sorted by row)
ge_status ge_coo::to_host() {
    std::lock_guard<std::mutex> guard(host_lock);
    if (host_ready) return GE_OK;
    try { row_ptr.assign((size_t)V + 1, 0); } catch (const std::bad_alloc &) { return ge::fail(GE_ERR_OOM, "host allocation failed"); }
    if (!reserve(nnz)) return ge::fail(GE_ERR_OOM, "host allocation failed for the COO (%lld entries)", (long long)nnz);
    GE_CHECK(ge::select_device(device));
    GE_HIP(hipMemcpy(I.get(), dI, sizeof(int32_t) * (size_t)nnz, hipMemcpyDeviceToHost));
    GE_HIP(hipMemcpy(J.get(), dJ, sizeof(int32_t) * (size_t)nnz, hipMemcpyDeviceToHost));
    GE_HIP(hipMemcpy(X.get(), dX, sizeof(float) * (size_t)nnz, hipMemcpyDeviceToHost));
    const int32_t *hI = I.get();
    for (int64_t k = 0; k < nnz; ++k) ++row_ptr[(size_t)hI[k] + 1];
    for (int32_t v = 0; v < V; ++v) row_ptr[(size_t)v + 1] += row_ptr[(size_t)v];
    host_ready = true;
    return GE_OK;
}

extern "C" {

void ge_synth_cfg_default(ge_synth_cfg *cfg) {
    if (!cfg) return;
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->seed = 0xC0FFEEull;
}

int32_t ge_synth_cfg_size(void) { return (int32_t)sizeof(ge_synth_cfg); }

ge_status ge_synth_coo(const ge_synth_cfg *cfg, ge_coo **out) { GE_GUARD(synth_impl(cfg, out)); }

ge_status ge_coo_device(const ge_coo *c, int32_t *device, const int32_t **dI, const int32_t **dJ, const float **dX) {
    if (!c) return ge::fail(GE_ERR_ARG, "null ge_coo handle");
    if (device) *device = c->device;
    if (dI) *dI = c->dI;
    if (dJ) *dJ = c->dJ;
    if (dX) *dX = c->dX;
    return GE_OK;
}

ge_status ge_coo_synth_stats(const ge_coo *c, int64_t *draws, float *kernel_ms, int64_t *peak_bytes) {
    if (!c) return ge::fail(GE_ERR_ARG, "null ge_coo handle");
    if (c->device < 0) return ge::fail(GE_ERR_STATE, "not a generated matrix");
    if (draws) *draws = c->draws;
    if (kernel_ms) *kernel_ms = c->kernel_ms;
    if (peak_bytes) *peak_bytes = c->peak_bytes;
    return GE_OK;
}

}  // extern "C"
