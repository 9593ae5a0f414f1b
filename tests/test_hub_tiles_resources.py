"""What the compiler made of k_epoch_tiles, the epoch kernel of a handle with hub tiles (csrc/glove.hip), read from the built
library's gfx950 code object (no GPU needed):
  * it is launch-bounded for three wavefronts per SIMD: at most 168 registers, and nothing in scratch -- the G resident pairs are
    register arrays that must never be indexed at run time;
  * three of its workgroups fit a CU's 160 KB of LDS;
  * it is a kernel of its own name: the 56 instances of k_adagrad_runs are what they were;
  * its walks wait for an LDS image with a hand-counted `s_waitcnt vmcnt(4)` -- the ordinary walk's (N_AFTER = 4 for this lane shape)
    and the tile walk's (TILE_N_AFTER = 4: the two stores that end a focus row, or the loads of the resident pairs, then the two loads
    of the next row's request).  The path analysis of tests/isa_waits.py holds every one of them to that count on every path.
Skipped where the LLVM tools of the ROCm image are missing.
"""
import os
import subprocess
import tempfile

import pytest

import test_kernel_resources as R

TILE_N_AFTER = 4       # csrc/glove.hip
GROUP = 2              # loads into LDS per request: the row and its accumulator row


def _tile_kernels(meta):
    return {k: v for k, v in meta.items() if "k_epoch_tiles" in k}


def test_tile_kernel_keeps_its_state_in_registers():
    meta = R._kernel_metadata()
    tiles = _tile_kernels(meta)
    assert len(tiles) == 1, sorted(tiles)                                    # one G is built
    (name, m), = tiles.items()
    assert "k_adagrad_runs" not in name
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
    assert m["vgpr_count"] <= 168, (name, m)
    assert m["group_segment_fixed_size"] * 3 <= 160 * 1024, (name, m)
    assert len([k for k in meta if "k_adagrad_runs" in k]) == 56


def test_tile_kernel_waits_hold_on_every_path():
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
            if "k_epoch_tiles" not in asm:
                continue
            for name, ins in W.parse_kernels(asm).items():
                if "k_epoch_tiles" not in name:
                    continue
                seen += 1
                assert W.n_after(4, 1, 0, False, True) == TILE_N_AFTER           # both walks of this kernel count to the same number
                state, problems = W.analyse(ins, GROUP)
                assert not problems, (name, problems)
                hand = [i for i, (_, mn, ops) in enumerate(ins)
                        if mn == "s_waitcnt" and W._vmcnt(ops) == TILE_N_AFTER and any(m.startswith("ds_read") for _, m, _ in ins[i + 1:i + 8])]
                # two unrolled steps of the ordinary walk and two unrolled rows of the tile walk (the compiler may duplicate a row's code)
                assert len(hand) >= 4, "%s: expected vmcnt(%d) in front of the image reads of both walks, found %d" % (name, TILE_N_AFTER, len(hand))
                for i in hand:
                    assert state[i] is not None, (name, i)
                    assert state[i][GROUP] >= TILE_N_AFTER, ("%s: on some path only %d vector-memory instructions follow the request this vmcnt(%d) at %#x waits for"
                                                             % (name, state[i][GROUP], TILE_N_AFTER, ins[i][0]))
                assert min(state[i][GROUP] for i in hand) == TILE_N_AFTER, (name, [state[i][GROUP] for i in hand])
                # no looser wait in front of a read of an image
                for i, (_, mn, ops) in enumerate(ins):
                    if mn == "s_waitcnt" and W._vmcnt(ops) is not None and state[i] is not None and i not in hand:
                        if any(m.startswith("ds_read_b128") for _, m, _ in ins[i + 1:i + 4]):
                            assert W._vmcnt(ops) <= TILE_N_AFTER, "%s: vmcnt(%d) at %#x in front of LDS reads" % (name, W._vmcnt(ops), ins[i][0])
    assert seen == 1
