"""What the compiler made of the alignment kernels, read from the kernel metadata of the built library's gfx950 code object (no
GPU, no disassembly): they are there, none uses scratch or spills, and k_align_join's LDS and registers fit the three workgroups
per CU that DESIGN.md 3.16 claims."""
from test_kernel_resources import _kernel_metadata

KERNELS = ("k_align_prepare", "k_align_join", "k_align_keys", "k_align_rowptr", "k_align_init", "k_align_point", "k_align_pair", "k_align_result",
           "k_align_summary")
WORKGROUPS_PER_CU = 3
LDS_PER_CU, VGPRS_PER_SIMD = 160 * 1024, 512


def _ours():
    meta = _kernel_metadata()
    out = {}
    for want in KERNELS:
        hits = [v for k, v in meta.items() if want in k]
        assert len(hits) == 1, (want, [k for k in meta if want in k])
        out[want] = hits[0]
    assert sorted(k for k in meta if "k_align_" in k) == sorted(k for k in meta if any(want in k for want in KERNELS))     # and no other
    return out


def test_the_kernels_are_in_the_code_object_without_scratch_or_spills():
    for name, m in _ours().items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)


def test_join_fits_the_claimed_workgroups_per_cu():
    m = _ours()["k_align_join"]
    # the panels alone: (64 + 128) rows of 34 floats
    assert m["group_segment_fixed_size"] == (64 + 128) * 34 * 4
    assert m["group_segment_fixed_size"] * WORKGROUPS_PER_CU <= LDS_PER_CU
    # a workgroup is four waves, one per SIMD: WORKGROUPS_PER_CU waves share a SIMD's registers (allocated in blocks of 8)
    assert (m["vgpr_count"] + 7) // 8 * 8 * WORKGROUPS_PER_CU <= VGPRS_PER_SIMD, m
