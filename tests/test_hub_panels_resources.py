"""What the compiler made of k_epoch_panels, the epoch kernel of a handle with hub panels (csrc/glove.hip), read from the built
library's gfx950 code object (no GPU needed):
  * one kernel of its own name (neither k_epoch_tiles nor k_adagrad_runs: those are counted elsewhere and stay what they were);
  * launch-bounded for three wavefronts per SIMD: at most 168 registers, nothing in scratch, three workgroups in a CU's 160 KB of LDS;
  * its walks wait for an LDS image with a hand-counted `s_waitcnt`: vmcnt(4) in the ordinary walk and in a tile chunk (the two stores
    that end a row or step, then the two loads of the next request), vmcnt(2) in stage 0 of the panel pipeline, which stores nothing
    to memory -- behind its image's request only the next row's request is certain.  The path analysis of tests/isa_waits.py holds
    every one of them to its count on every path.
Skipped where the LLVM tools of the ROCm image are missing.
"""
import os
import subprocess
import tempfile

import pytest

import test_kernel_resources as R

TILE_N_AFTER = 4       # csrc/glove.hip: a walk that stores its pair to memory
PIPE_N_AFTER = 2       # stage 0 of the panel pipeline: SINK = PAIR_LDS
GROUP = 2              # loads into LDS per request: the row and its accumulator row


def test_panel_kernel_keeps_its_state_in_registers():
    meta = R._kernel_metadata()
    panels = {k: v for k, v in meta.items() if "k_epoch_panels" in k}
    assert len(panels) == 1, sorted(panels)
    (name, m), = panels.items()
    assert "k_adagrad_runs" not in name and "k_epoch_tiles" not in name
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
    assert m["vgpr_count"] <= 168, (name, m)
    assert m["group_segment_fixed_size"] * 3 <= 160 * 1024, (name, m)
    assert len([k for k in meta if "k_adagrad_runs" in k]) == 56
    assert len([k for k in meta if "k_epoch_tiles" in k]) == 1


def test_panel_kernel_waits_hold_on_every_path():
    import isa_waits as W
    objdump = os.path.join(R.LLVM, "llvm-objdump")
    if not (os.path.exists(objdump) and os.path.exists(os.path.join(R.LLVM, "llvm-objcopy"))):
        pytest.skip("llvm-objdump / llvm-objcopy not found under " + R.LLVM)
    if not os.path.exists(R.LIB):
        pytest.skip("libgeglove.so not built")
    seen = 0
    with tempfile.TemporaryDirectory() as tmp:
        for co in R._gfx950_code_objects(tmp):
            asm = subprocess.run([objdump, "-d", "--mcpu=gfx950", co], check=True, capture_output=True, text=True).stdout
            if "k_epoch_panels" not in asm:
                continue
            for name, ins in W.parse_kernels(asm).items():
                if "k_epoch_panels" not in name:
                    continue
                seen += 1
                state, problems = W.analyse(ins, GROUP)
                assert not problems, (name, problems)

                def hand(n):
                    return [i for i, (_, mn, ops) in enumerate(ins)
                            if mn == "s_waitcnt" and W._vmcnt(ops) == n and any(m.startswith("ds_read") for _, m, _ in ins[i + 1:i + 8])]
                # two unrolled steps of the ordinary walk and two unrolled rows of a tile chunk; two unrolled rows of stage 0
                for n, least in ((TILE_N_AFTER, 4), (PIPE_N_AFTER, 2)):
                    found = hand(n)
                    assert len(found) >= least, "%s: expected vmcnt(%d) in front of image reads, found %d" % (name, n, len(found))
                    for i in found:
                        assert state[i] is not None, (name, i)
                        assert state[i][GROUP] >= n, ("%s: on some path only %d vector-memory instructions follow the request this vmcnt(%d) at %#x waits for"
                                                      % (name, state[i][GROUP], n, ins[i][0]))
                    assert min(state[i][GROUP] for i in found) == n, (name, n, [state[i][GROUP] for i in found])
                # a workgroup barrier per pipeline step, and none of them in scratch-spilling code
                assert sum(1 for _, mn, _ in ins if mn == "s_barrier") >= 4
                assert not any(mn.startswith("scratch_") for _, mn, _ in ins)
                # no looser wait in front of a read of an image
                counted = set(hand(TILE_N_AFTER)) | set(hand(PIPE_N_AFTER))
                for i, (_, mn, ops) in enumerate(ins):
                    if mn == "s_waitcnt" and W._vmcnt(ops) is not None and state[i] is not None and i not in counted:
                        if any(m.startswith("ds_read_b128") for _, m, _ in ins[i + 1:i + 4]):
                            assert W._vmcnt(ops) <= TILE_N_AFTER, "%s: vmcnt(%d) at %#x in front of LDS reads" % (name, W._vmcnt(ops), ins[i][0])
    assert seen == 1
