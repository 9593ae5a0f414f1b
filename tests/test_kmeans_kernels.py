"""What the compiler made of the clustering kernels, read from the built library's gfx950 code objects (no GPU needed): the
k_km_ kernels are there, none uses scratch or spills, the assign kernel runs on the fp32 matrix cores, neither it nor the sum
kernels hold a floating-point atomic instruction, and the LDS and registers fit the occupancy DESIGN.md 3.10 states."""
import os
import re
import subprocess
import tempfile

import pytest

import test_kernel_resources as KR

LDS_PER_CU, REGS_PER_LANE = 160 * 1024, 512
# k_km_assign (four waves per workgroup) three workgroups per CU, i.e. three waves per SIMD, set by the registers
ASSIGN_WORKGROUPS_PER_CU = 3
NAMES = ("k_km_prepare", "k_km_row_squares", "k_km_iota", "k_km_take_rows", "k_km_bias", "k_km_assign", "k_km_bounds", "k_km_piece_sums",
         "k_km_centroids")
SUMS = ("k_km_piece_sums", "k_km_centroids", "k_km_block_sums")


def _km_kernels():
    meta = {k: v for k, v in KR._kernel_metadata().items() if "k_km_" in k}
    out = {}
    for name in NAMES:
        hits = [v for k, v in meta.items() if re.search(r"\d+%sE" % name, k)]
        assert len(hits) == 1, (name, sorted(meta))
        out[name] = hits[0]
    sums = {k: v for k, v in meta.items() if "k_km_block_sumsI" in k}
    assert len(sums) == 2, sorted(meta)                                   # the objective's (float) and sum_sq's (double)
    out.update(sums)
    return out


def test_the_kernels_are_in_the_code_object_without_scratch():
    for name, m in _km_kernels().items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)


def test_lds_and_registers_fit_the_claimed_occupancy():
    k = _km_kernels()
    for name, m in k.items():
        print("%s: %d B of LDS, %d registers per lane" % (name, m["group_segment_fixed_size"], m["vgpr_count"]))
    a = k["k_km_assign"]
    granule = (a["vgpr_count"] + 7) // 8 * 8                              # registers are allocated in eights
    panels = (64 + 128) * 34 * 4                                          # 26 112 B
    assert panels <= a["group_segment_fixed_size"] <= panels + 64, a     # the panels and the four change counts: no lists
    assert a["group_segment_fixed_size"] * ASSIGN_WORKGROUPS_PER_CU <= LDS_PER_CU, a
    assert granule * ASSIGN_WORKGROUPS_PER_CU <= REGS_PER_LANE, a         # one wave of each workgroup per SIMD
    assert a["group_segment_fixed_size"] * 6 <= LDS_PER_CU                # LDS alone would let six in: the registers set the occupancy
    assert k["k_km_piece_sums"]["group_segment_fixed_size"] == 0
    assert k["k_km_centroids"]["group_segment_fixed_size"] == 1024 * 8 + 1024 * 4


def _is_float_atomic(m):
    memory = "atomic" in m or re.match(r"ds_(add|sub|min|max|pk_add|cmpst|wrxchg)", m)
    return bool(memory and re.search(r"_f(16|32|64)|bf16|fmin|fmax", m))


def test_instructions():
    objdump = os.path.join(KR.LLVM, "llvm-objdump")
    if not (os.path.exists(objdump) and os.path.exists(os.path.join(KR.LLVM, "llvm-objcopy"))):
        pytest.skip("llvm-objdump / llvm-objcopy not found under " + KR.LLVM)
    if not os.path.exists(KR.LIB):
        pytest.skip("libgeglove.so not built")
    import isa_waits as W
    assert _is_float_atomic("global_atomic_add_f32") and _is_float_atomic("ds_add_rtn_f64") and _is_float_atomic("global_atomic_pk_add_bf16")
    assert not _is_float_atomic("global_atomic_add_x2") and not _is_float_atomic("ds_read_b32") and not _is_float_atomic("v_add_f64")
    found = {}
    with tempfile.TemporaryDirectory() as tmp:
        for co in KR._gfx950_code_objects(tmp):
            asm = subprocess.run([objdump, "-d", "--mcpu=gfx950", co], check=True, capture_output=True, text=True).stdout
            if "k_km_" not in asm:
                continue
            for name, ins in W.parse_kernels(asm).items():
                if "k_km_" in name:
                    found[name] = [mn for _, mn, _ in ins]
    assign = [v for k, v in found.items() if re.search(r"\d+k_km_assignE", k)]
    assert len(assign) == 1, sorted(found)
    assert sum(m.startswith("v_mfma_f32_16x16x4") for m in assign[0]) >= 8      # eight accumulators per wave
    sums = [v for k, v in found.items() if any(s in k for s in SUMS)]
    assert len(sums) == 4, sorted(found)
    for body in found.values():
        assert not any(m.startswith("scratch_") for m in body)
    for body in assign + sums:
        assert not any(_is_float_atomic(m) for m in body), [m for m in body if _is_float_atomic(m)]
