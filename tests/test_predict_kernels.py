"""What the compiler made of the prediction kernels, read from the built library's gfx950 code objects (no GPU needed):
k_predict_stage, the four k_predict_select instances and k_predict_merge are there, none uses scratch or spills, and the LDS and
registers of each fit the occupancy DESIGN.md 3.11 states -- that of the k_nn_score_select instance with the same CAP; the select
kernel runs on the fp32 matrix cores and no kernel holds an atomic memory instruction."""
import os
import re
import subprocess
import tempfile

import pytest

import test_kernel_resources as KR

LDS_PER_CU, REGS_PER_LANE = 160 * 1024, 512
# workgroups of four waves per CU (= waves per SIMD) by the capacity of a query's list: the __launch_bounds__ of nn.hip
WORKGROUPS_PER_CU = {32: 3, 64: 2, 128: 1, 256: 1}
PANELS = (64 + 128) * 34 * 4                                              # the query and candidate panels, 26 112 B


def _predict_kernels():
    meta = KR._kernel_metadata()
    out = {}
    for name in ("k_predict_stage", "k_predict_merge"):
        hits = [v for k, v in meta.items() if re.search(r"\d+%sE" % name, k)]
        assert len(hits) == 1, (name, [k for k in meta if "k_predict" in k])
        out[name] = hits[0]
    for cap in WORKGROUPS_PER_CU:
        hits = [v for k, v in meta.items() if re.search(r"\d+k_predict_selectILi%dEE" % cap, k)]
        assert len(hits) == 1, (cap, [k for k in meta if "k_predict" in k])
        out["k_predict_select<%d>" % cap] = hits[0]
    assert len([k for k in meta if "k_predict" in k]) == len(out), [k for k in meta if "k_predict" in k]
    return out


def test_the_kernels_are_in_the_code_object_without_scratch():
    for name, m in _predict_kernels().items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)


def test_lds_and_registers_fit_the_claimed_occupancy():
    k = _predict_kernels()
    for name, m in k.items():
        print("%s: %d B of LDS, %d registers per lane" % (name, m["group_segment_fixed_size"], m["vgpr_count"]))
    granule = lambda m: (m["vgpr_count"] + 7) // 8 * 8                   # registers are allocated in eights
    for cap, groups in WORKGROUPS_PER_CU.items():
        m = k["k_predict_select<%d>" % cap]
        lists = 64 * cap * 8                                              # (z, position) of every slot
        # the panels, the lists, and per query a threshold (8 B), a fill count (4 B), the cursor into its filter list, the list's
        # length and its next position (12 B) and the tile's filter mask (16 B)
        assert m["group_segment_fixed_size"] == PANELS + lists + 64 * 40, (cap, m)
        assert m["group_segment_fixed_size"] * groups <= LDS_PER_CU, (cap, m)
        assert granule(m) * groups <= REGS_PER_LANE, (cap, m)            # one wave of each workgroup per SIMD
    assert k["k_predict_stage"]["group_segment_fixed_size"] == 0
    assert k["k_predict_merge"]["group_segment_fixed_size"] == 2 * 128 * 8          # two lists of 128 entries side by side


def test_the_nn_instances_keep_their_occupancy_beside_them():
    """The same CAP gives the same workgroups per CU in both files (the claim of DESIGN.md 3.11)."""
    meta = KR._kernel_metadata()
    for cap, groups in WORKGROUPS_PER_CU.items():
        hits = [v for k, v in meta.items() if re.search(r"\d+k_nn_score_selectILi%dEE" % cap, k)]
        assert len(hits) == 1
        assert hits[0]["group_segment_fixed_size"] * groups <= LDS_PER_CU and (hits[0]["vgpr_count"] + 7) // 8 * 8 * groups <= REGS_PER_LANE


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
            if "k_predict_" not in asm:
                continue
            for name, ins in W.parse_kernels(asm).items():
                if "k_predict_" in name:
                    found[name] = [mn for _, mn, _ in ins]
    select = [v for k, v in found.items() if "k_predict_selectILi" in k]
    assert len(select) == len(WORKGROUPS_PER_CU) and len(found) == len(select) + 2, sorted(found)
    for s in select:
        assert sum(m.startswith("v_mfma_f32_16x16x4") for m in s) >= 8          # eight accumulators per wave, no scalar fallback
    for body in found.values():
        assert not any(m.startswith("scratch_") for m in body)
        assert not any("atomic" in m for m in body)                 # the list slots and the mask bits are LDS integer operations
