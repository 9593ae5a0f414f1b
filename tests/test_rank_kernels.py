"""What the compiler made of the ranking kernels, read from the built library's gfx950 code objects (no GPU needed):
k_rank_stage, k_rank_gather and k_rank_count are there, none uses scratch or spills, and the LDS and registers of each fit the
occupancy DESIGN.md 3.9 states."""
import re

import test_kernel_resources as KR

LDS_PER_CU, REGS_PER_LANE, SIMDS = 160 * 1024, 512, 4
# k_rank_gather (wavefront-sized workgroups) as k_eval_terms, four waves per SIMD; k_rank_count (four waves per
# workgroup) three workgroups per CU, i.e. three waves per SIMD
GATHER_WAVES_PER_SIMD = 4
COUNT_WORKGROUPS_PER_CU = 3


def _rank_kernels():
    meta = KR._kernel_metadata()
    out = {}
    for name in ("k_rank_stage", "k_rank_gather", "k_rank_count"):
        hits = [v for k, v in meta.items() if re.search(r"\d+%sE" % name, k)]
        assert len(hits) == 1, (name, [k for k in meta if "k_rank" in k])
        out[name] = hits[0]
    return out


def test_the_kernels_are_in_the_code_object_without_scratch():
    for name, m in _rank_kernels().items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)


def test_lds_and_registers_fit_the_claimed_occupancy():
    k = _rank_kernels()
    for name, m in k.items():
        print("%s: %d B of LDS, %d registers per lane" % (name, m["group_segment_fixed_size"], m["vgpr_count"]))
    granule = lambda m: (m["vgpr_count"] + 7) // 8 * 8                   # registers are allocated in eights
    g = k["k_rank_gather"]
    assert g["group_segment_fixed_size"] * GATHER_WAVES_PER_SIMD * SIMDS <= LDS_PER_CU, g
    assert granule(g) * GATHER_WAVES_PER_SIMD <= REGS_PER_LANE, g
    assert g["group_segment_fixed_size"] == 2 * 64 * 17 * 4 + 2 * 64 * 8            # the two panels [64][17] and the row offsets
    c = k["k_rank_count"]
    panels = (64 + 128) * 34 * 4                                          # 26 112 B
    assert panels <= c["group_segment_fixed_size"] < panels + 1024, c    # the panels and under 1 KB more
    assert c["group_segment_fixed_size"] * COUNT_WORKGROUPS_PER_CU <= LDS_PER_CU, c
    assert granule(c) * COUNT_WORKGROUPS_PER_CU <= REGS_PER_LANE, c       # one wave of each workgroup per SIMD
    assert k["k_rank_stage"]["group_segment_fixed_size"] == 0
