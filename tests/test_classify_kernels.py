"""What the compiler made of the classification kernels, read from the built library's gfx950 code objects (no GPU needed): the
k_cls_ kernels are there, none uses scratch or spills, the logits and the gradient kernels run on the fp32 matrix cores, no
k_cls_ kernel holds a floating-point atomic instruction, and the LDS and registers fit the occupancy DESIGN.md 3.14 states."""
import os
import re
import subprocess
import tempfile

import pytest

import test_kernel_resources as KR
from test_kmeans_kernels import _is_float_atomic

LDS_PER_CU, REGS_PER_LANE = 160 * 1024, 512
# k_cls_logits three workgroups (of four waves) per CU as k_km_assign, set by the registers; k_cls_gradient, which
# uses no LDS, four waves per SIMD in its widest instance (four class fragments) and more in the narrower ones
LOGITS_WORKGROUPS_PER_CU, GRADIENT_WAVES_PER_SIMD = 3, 4
PLAIN = ("k_cls_prepare", "k_cls_logits", "k_cls_softmax", "k_cls_block_sums", "k_cls_piece_sum")
GRADIENTS = ("k_cls_gradientILi1EE", "k_cls_gradientILi2EE", "k_cls_gradientILi4EE")


def _cls_kernels():
    meta = {k: v for k, v in KR._kernel_metadata().items() if "k_cls_" in k}
    out = {}
    for name in PLAIN:
        hits = [v for k, v in meta.items() if re.search(r"\d+%sE" % name, k)]
        assert len(hits) == 1, (name, sorted(meta))
        out[name] = hits[0]
    for name in GRADIENTS:
        hits = [v for k, v in meta.items() if name in k]
        assert len(hits) == 1, (name, sorted(meta))
        out[name] = hits[0]
    assert len(out) == len(meta), sorted(meta)                            # and no other k_cls_ kernel
    return out


def _granule(m):
    return (m["vgpr_count"] + 7) // 8 * 8                                  # registers are allocated in eights


def test_the_kernels_are_in_the_code_object_without_scratch():
    for name, m in _cls_kernels().items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)


def test_lds_and_registers_fit_the_claimed_occupancy():
    k = _cls_kernels()
    for name, m in k.items():
        print("%s: %d B of LDS, %d registers per lane" % (name, m["group_segment_fixed_size"], m["vgpr_count"]))
    a = k["k_cls_logits"]
    panels = (64 + 128) * 34 * 4                                          # 26 112 B
    assert a["group_segment_fixed_size"] == panels, a                      # the two panels and nothing else
    assert a["group_segment_fixed_size"] * LOGITS_WORKGROUPS_PER_CU <= LDS_PER_CU, a
    assert _granule(a) * LOGITS_WORKGROUPS_PER_CU <= REGS_PER_LANE, a      # one wave of each workgroup per SIMD
    for name in GRADIENTS:
        assert k[name]["group_segment_fixed_size"] == 0, name              # fragments come straight from memory, sums stay in registers
        assert _granule(k[name]) * GRADIENT_WAVES_PER_SIMD <= REGS_PER_LANE, (name, k[name])
    assert _granule(k["k_cls_gradientILi1EE"]) * 8 <= REGS_PER_LANE        # the narrowest instance fills a SIMD's eight wave slots
    assert k["k_cls_softmax"]["group_segment_fixed_size"] == 0 and _granule(k["k_cls_softmax"]) * 8 <= REGS_PER_LANE
    assert k["k_cls_piece_sum"]["group_segment_fixed_size"] == 0
    assert k["k_cls_block_sums"]["group_segment_fixed_size"] == 1024 * 8


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
            if "k_cls_" not in asm:
                continue
            for name, ins in W.parse_kernels(asm).items():
                if "k_cls_" in name:
                    found[name] = [mn for _, mn, _ in ins]
    assert len(found) == len(PLAIN) + len(GRADIENTS), sorted(found)
    logits = [v for k, v in found.items() if re.search(r"\d+k_cls_logitsE", k)]
    assert len(logits) == 1, sorted(found)
    assert sum(m.startswith("v_mfma_f32_16x16x4") for m in logits[0]) >= 8        # eight accumulators per wave
    for name in GRADIENTS:
        body = [v for k, v in found.items() if name in k]
        assert len(body) == 1 and sum(m.startswith("v_mfma_f32_16x16x4") for m in body[0]) >= 1, name
    for name, body in found.items():
        assert not any(m.startswith("scratch_") for m in body), name
        assert not any(_is_float_atomic(m) for m in body), (name, [m for m in body if _is_float_atomic(m)])
