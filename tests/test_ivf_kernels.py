"""What the compiler made of the inverted-file kernels, read from the metadata of the built library's gfx950 code objects (no GPU
needed): every k_ivf_ kernel is there, none uses scratch or spills, and the LDS and registers of the four scan instances fit
the occupancy DESIGN.md 3.13 states.  Metadata only: no instruction is searched for."""
import re

import test_kernel_resources as KR

# list capacity -> workgroups of 256 threads per CU, as k_nn_score_select
CLAIMED = {32: 3, 64: 2, 128: 1, 256: 1}
LDS_PER_CU, REGS_PER_LANE = 160 * 1024, 512
SMALL = ("k_ivf_prepare", "k_ivf_merge", "k_ivf_iota", "k_ivf_bounds", "k_ivf_items", "k_ivf_pair_slots", "k_ivf_gather")


def _ivf_kernels():
    meta = {k: v for k, v in KR._kernel_metadata().items() if "k_ivf_" in k}
    small = {}
    for name in SMALL:
        hits = [v for k, v in meta.items() if re.search(r"\d+%sE" % name, k)]
        assert len(hits) == 1, (name, sorted(meta))
        small[name] = hits[0]
    scan = {int(re.search(r"k_ivf_scanILi(\d+)E", k).group(1)): v for k, v in meta.items() if "k_ivf_scanILi" in k}
    assert len(meta) == len(small) + len(scan), sorted(meta)
    return small, scan


def test_the_kernels_are_in_the_code_object_without_scratch():
    small, scan = _ivf_kernels()
    assert sorted(scan) == sorted(CLAIMED), sorted(scan)
    for name, m in list(small.items()) + [("scan<%d>" % c, m) for c, m in scan.items()]:
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m.get("sgpr_spill_count", 0) == 0, (name, m)


def test_lds_and_registers_fit_the_claimed_occupancy():
    small, scan = _ivf_kernels()
    for cap, wgs in CLAIMED.items():
        m = scan[cap]
        granule = (m["vgpr_count"] + 7) // 8 * 8                   # registers are allocated in eights
        print("k_ivf_scan<%d>: %d B of LDS, %d registers per lane, %d workgroup(s) per CU claimed" % (cap, m["group_segment_fixed_size"], m["vgpr_count"], wgs))
        # the panels, the lists, and per query: threshold, count, row, slot, self -- 24 bytes
        want = (64 + 128) * 34 * 4 + 64 * cap * 8 + 64 * 24
        assert want <= m["group_segment_fixed_size"] <= want + 64, (cap, m)
        assert m["group_segment_fixed_size"] * wgs <= LDS_PER_CU, (cap, m)
        assert m["group_segment_fixed_size"] * (wgs + 1) > LDS_PER_CU or wgs == 1, (cap, m)     # and LDS is what sets it
        assert granule * wgs <= REGS_PER_LANE, (cap, m)            # a workgroup puts one wave on each SIMD
    assert small["k_ivf_merge"]["group_segment_fixed_size"] == 2 * 128 * 8
    assert small["k_ivf_gather"]["group_segment_fixed_size"] == 0
