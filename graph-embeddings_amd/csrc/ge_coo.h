// ge_coo.h -- the co-occurrence matrix handle behind ge_coo: filled on the host by ge_bca_build (bca.hip), on the device by
// ge_synth_coo (synth.hip), read in place by ge_glove_create_coo (glove.hip).  Internal to libgeglove.so.
#pragma once
#include "ge_common.h"

#include <algorithm>
#include <cstdlib>
#include <memory>
#include <mutex>
#include <vector>
#include <sys/mman.h>

struct ge_coo {
    int64_t nnz = 0;
    int32_t V = 0;
    struct Free { void operator()(void *q) const { std::free(q); } };
    std::unique_ptr<int32_t[], Free> I, J;      // nnz entries each; left uninitialised until the device copy fills them
    std::unique_ptr<float[], Free> X;           //   (a value-initialising container would touch 12 bytes per entry once more)
    int64_t capacity = 0;                       // entries each array has room for (>= nnz)
    // Fresh host memory costs more than the copy into it: 520 MB of J and X arrive in 9 ms once their pages exist and in 35 - 60 ms when
    // every page is met for the first time (tools/r03/pinned_probe.py).  The arrays are therefore allocated BEFORE the main launch, from
    // the sample's estimate of the total, and their pages are touched by host threads while the device works.
    bool reserve(int64_t entries) {
        const size_t bytes = ((size_t)std::max<int64_t>(entries, 1) * 4 + 4095) / 4096 * 4096;
        void *q[3] = {nullptr, nullptr, nullptr};
        for (int k = 0; k < 3; ++k)
            if (posix_memalign(&q[k], (size_t)1 << 21, bytes) != 0) { for (int j = 0; j < k; ++j) std::free(q[j]); return false; }
        for (int k = 0; k < 3; ++k) (void)madvise(q[k], bytes, MADV_HUGEPAGE);      // where the system allows it: 2 MB pages, 512 times fewer faults
        I.reset(static_cast<int32_t *>(q[0])); J.reset(static_cast<int32_t *>(q[1])); X.reset(static_cast<float *>(q[2]));
        capacity = (int64_t)(bytes / 4);
        return true;
    }
    // one write per 4 KB page of the first `entries` entries of the three arrays, slice t of n
    void touch(int64_t entries, int t, int n) {
        const int64_t pages = (std::min(entries, capacity) * 4 + 4095) / 4096;
        for (int a = 0; a < 3; ++a) {
            volatile char *base = a == 0 ? reinterpret_cast<char *>(I.get()) : a == 1 ? reinterpret_cast<char *>(J.get()) : reinterpret_cast<char *>(X.get());
            for (int64_t pg = pages * t / n, p1 = pages * (t + 1) / n; pg < p1; ++pg) base[pg * 4096] = 0;
        }
    }
    std::vector<int64_t> row_ptr;
    double max = 0;

    // A device-resident result (ge_synth_coo): the arrays live in dI / dJ / dX on `device`, sorted by (i, j); the host arrays above
    // stay empty until the first ge_coo_get copies them down (to_host, synth.hip).  device = -1: host-resident (ge_bca_build).
    int32_t device = -1;
    int32_t row_begin = 0, row_end = 0;         // the rows the generator was asked for
    int32_t *dI = nullptr, *dJ = nullptr;
    float *dX = nullptr;
    bool host_ready = true;
    std::mutex host_lock;                       // ge_coo_get takes a const handle from any thread
    int64_t draws = 0, peak_bytes = 0;          // ge_coo_synth_stats
    float kernel_ms = 0.0f;
    ge_status to_host();
    ~ge_coo() { for (void *q : {(void *)dI, (void *)dJ, (void *)dX}) if (q) (void)hipFree(q); }
};
