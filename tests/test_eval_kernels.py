"""What the compiler made of the held-out evaluation kernels, read from the built library's gfx950 code objects (no GPU
needed): the four instances of k_eval_terms (16-byte / dword row accesses x fp32 / bf16 rows) and k_eval_block_sums are there,
none uses scratch or spills, and the LDS and registers of each fit the occupancy DESIGN.md 3.8 states."""
import re

import test_kernel_resources as KR

# wavefront-sized workgroups, at least this many resident per SIMD (16 per CU)
CLAIMED_WAVES_PER_SIMD = 4
LDS_PER_CU, REGS_PER_LANE, SIMDS = 160 * 1024, 512, 4


def _eval_kernels():
    meta = {k: v for k, v in KR._kernel_metadata().items() if "k_eval_" in k}
    terms = {}
    for k, v in meta.items():
        m = re.search(r"k_eval_termsILi(\d+)ELb([01])E", k)
        if m:
            terms[(int(m.group(1)), bool(int(m.group(2))))] = v
    sums = {k: v for k, v in meta.items() if re.search(r"\d+k_eval_block_sumsE", k)}
    return terms, sums


def test_the_kernels_are_in_the_code_object_without_scratch():
    terms, sums = _eval_kernels()
    assert sorted(terms) == [(1, False), (1, True), (4, False), (4, True)] and len(sums) == 1, (sorted(terms), sorted(sums))
    for name, m in [("terms<%d,%s>" % k, v) for k, v in terms.items()] + list(sums.items()):
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)


def test_lds_and_registers_fit_the_claimed_occupancy():
    terms, sums = _eval_kernels()
    for name, m in [("terms<%d,%s>" % k, v) for k, v in terms.items()] + list(sums.items()):
        granule = (m["vgpr_count"] + 7) // 8 * 8                       # registers are allocated in eights
        print("%s: %d B of LDS, %d registers per lane" % (name, m["group_segment_fixed_size"], m["vgpr_count"]))
        assert m["group_segment_fixed_size"] * CLAIMED_WAVES_PER_SIMD * SIMDS <= LDS_PER_CU, (name, m)
        assert granule * CLAIMED_WAVES_PER_SIMD <= REGS_PER_LANE, (name, m)
    for k, m in terms.items():                                         # the panel [64][33] floats and the row pointers, nothing more
        assert 64 * 33 * 4 + 2 * 64 * 8 <= m["group_segment_fixed_size"] <= 64 * 33 * 4 + 2 * 64 * 8 + 64 * 4, (k, m)
