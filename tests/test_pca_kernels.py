"""What the compiler made of the two PCA kernels, read from the built library's gfx950 code objects (no GPU needed): both are
there, neither uses scratch or spills, and the Gram kernel runs on the fp64 matrix cores (the projection on the fp32 ones)."""
import os
import re
import subprocess
import tempfile

import pytest

import test_kernel_resources as KR


def _pca_kernels():
    meta = {k: v for k, v in KR._kernel_metadata().items() if "k_pca_" in k}
    gram = {k: v for k, v in meta.items() if re.search(r"\d+k_pca_gramE", k)}
    project = {k: v for k, v in meta.items() if "k_pca_projectILi" in k}
    return gram, project


def test_both_kernels_are_in_the_code_object_without_scratch():
    gram, project = _pca_kernels()
    assert len(gram) == 1, sorted(gram)
    assert len(project) == 4, sorted(project)                      # one instance per number of 16-column tiles a wave carries
    for name, m in list(gram.items()) + list(project.items()):
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
    (g,) = gram.values()
    assert g["group_segment_fixed_size"] * 4 <= 160 * 1024 and g["vgpr_count"] <= 128, g      # four workgroups per CU: LDS and registers


def test_matrix_core_instructions():
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
            if "k_pca_" not in asm:
                continue
            for name, ins in W.parse_kernels(asm).items():
                if "k_pca_" in name:
                    found[name] = [mn for _, mn, _ in ins]
    gram = [v for k, v in found.items() if re.search(r"\d+k_pca_gramE", k)]
    project = [v for k, v in found.items() if "k_pca_projectILi" in k]
    assert len(gram) == 1 and len(project) == 4, sorted(found)
    assert sum(m.startswith("v_mfma_f64_16x16x4") for m in gram[0]) >= 4
    assert not any(m.startswith("scratch_") for m in gram[0])
    assert not any("atomic" in m for m in gram[0])                 # fixed-order reduction: no floating-point atomics in the moment pass
    for p in project:
        assert any(m.startswith("v_mfma_f32_16x16x4") for m in p) and not any(m.startswith("scratch_") for m in p)
