"""What the compiler made of the nearest-neighbour kernels, read from the built library's gfx950 code objects (no GPU needed):
all three are there, none uses scratch or spills, the score kernel runs on the fp32 matrix cores, neither it nor the merge holds
an atomic memory instruction, and the LDS and registers of each instance fit the occupancy DESIGN.md 3.5 states."""
import os
import re
import subprocess
import tempfile

import pytest

import test_kernel_resources as KR

# list capacity -> workgroups of 256 threads per CU
CLAIMED = {32: 3, 64: 2, 128: 1, 256: 1}
LDS_PER_CU, REGS_PER_LANE = 160 * 1024, 512


def _nn_kernels():
    meta = {k: v for k, v in KR._kernel_metadata().items() if "k_nn_" in k}
    prepare = {k: v for k, v in meta.items() if re.search(r"\d+k_nn_prepareE", k)}
    score = {int(re.search(r"k_nn_score_selectILi(\d+)E", k).group(1)): v for k, v in meta.items() if "k_nn_score_selectILi" in k}
    merge = {k: v for k, v in meta.items() if re.search(r"\d+k_nn_mergeE", k)}
    return prepare, score, merge


def test_the_three_kernels_are_in_the_code_object_without_scratch():
    prepare, score, merge = _nn_kernels()
    assert len(prepare) == 1 and len(merge) == 1 and sorted(score) == sorted(CLAIMED), (sorted(prepare), sorted(score), sorted(merge))
    for name, m in list(prepare.items()) + list(merge.items()) + [("score<%d>" % c, m) for c, m in score.items()]:
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)


def test_lds_and_registers_fit_the_claimed_occupancy():
    _, score, _ = _nn_kernels()
    for cap, wgs in CLAIMED.items():
        m = score[cap]
        granule = (m["vgpr_count"] + 7) // 8 * 8                   # registers are allocated in eights
        print("k_nn_score_select<%d>: %d B of LDS, %d registers per lane, %d workgroup(s) per CU claimed" % (cap, m["group_segment_fixed_size"], m["vgpr_count"], wgs))
        assert m["group_segment_fixed_size"] * wgs <= LDS_PER_CU, (cap, m)
        assert m["group_segment_fixed_size"] * (wgs + 1) > LDS_PER_CU or wgs == 1, (cap, m)     # and LDS is what sets it
        assert granule * wgs <= REGS_PER_LANE, (cap, m)            # a workgroup puts one wave on each SIMD


def test_instructions():
    objdump = os.path.join(KR.LLVM, "llvm-objdump")
    if not (os.path.exists(objdump) and os.path.exists(os.path.join(KR.LLVM, "llvm-objcopy"))):
        pytest.skip("llvm-objdump / llvm-objcopy not found under " + KR.LLVM)
    if not os.path.exists(KR.LIB):
        pytest.skip("libgeglove.so not built")
    import isa_waits as W
    found = {}
    with tempfile.TemporaryDirectory() as tmp:
        for co in KR._gfx950_code_objects(tmp):
            asm = subprocess.run([objdump, "-d", "--mcpu=gfx950", co], check=True, capture_output=True, text=True).stdout
            if "k_nn_" not in asm:
                continue
            for name, ins in W.parse_kernels(asm).items():
                if "k_nn_" in name:
                    found[name] = [mn for _, mn, _ in ins]
    score = [v for k, v in found.items() if "k_nn_score_selectILi" in k]
    merge = [v for k, v in found.items() if re.search(r"\d+k_nn_mergeE", k)]
    prepare = [v for k, v in found.items() if re.search(r"\d+k_nn_prepareE", k)]
    assert len(score) == len(CLAIMED) and len(merge) == 1 and len(prepare) == 1, sorted(found)
    for s in score:
        assert sum(m.startswith("v_mfma_f32_16x16x4") for m in s) >= 8          # eight accumulators per wave
    for body in score + merge + prepare:
        assert not any(m.startswith("scratch_") for m in body)
    for body in score + merge:
        assert not any("atomic" in m for m in body)                 # selection by rank under a total order: nothing depends on arrival
