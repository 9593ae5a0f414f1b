"""What the compiler made of k_epoch_walk2, the ring kernel whose ordinary walk keeps the streamed pairs of two nonzeros in flight
(csrc/glove.hip), read from the built library's gfx950 code object (no GPU needed):
  * one kernel of its own name; k_adagrad_runs, k_epoch_tiles, k_epoch_panels and k_epoch_ring are as many as they were (56 / 1 / 1 / 1);
  * launch-bounded for three wavefronts per SIMD: at most 168 registers, nothing in scratch, three workgroups in a CU's 160 KB of
    LDS with a third image (2 KB) for each of the four waves beside everything k_epoch_ring holds;
  * a step reads the image of nonzero p behind a hand-counted `s_waitcnt vmcnt(8)`: behind that image's request stand the stores of
    steps p - 2 and p - 1 and the requests of nonzeros p + 1 and p + 2, two instructions each, and before the first steps of a
    chunk its prologue issues as many.  The path analysis of tests/isa_waits.py, with a window of two requests (four loads into
    LDS), holds the count on every path, the chunk's first steps included;
  * stage 0 of the panel pipeline keeps its vmcnt(2 RING_K) and the tile chunk its vmcnt(4), as in k_epoch_ring.
Skipped where the LLVM tools of the ROCm image are missing.
"""
import os
import subprocess
import tempfile

import pytest

import test_kernel_resources as R
from test_hub_ring_resources import GROUP, TILE_N_AFTER, _ring_k

NAME = "k_epoch_walk2"
WD = 2                                  # nonzeros the walk requests ahead
N_WALK = WD * (GROUP + GROUP)           # per step two stores and one request of two loads: N_TAB = N_DMA = 2 for fp32 fat rows
OTHERS = {"k_adagrad_runs": 56, "k_epoch_tiles": 1, "k_epoch_panels": 1, "k_epoch_ring": 1}


def test_deep_walk_kernel_keeps_its_state_in_registers():
    meta = R._kernel_metadata()
    mine = {k: v for k, v in meta.items() if NAME in k}
    assert len(mine) == 1, sorted(mine)
    (name, m), = mine.items()
    assert not any(s in name for s in OTHERS)
    for s, n in OTHERS.items():
        assert len([k for k in meta if s in k]) == n, s
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
    assert m["vgpr_count"] <= 168, (name, m)
    assert m["group_segment_fixed_size"] * 3 <= 160 * 1024, (name, m)
    ring, = [v for k, v in meta.items() if "k_epoch_ring" in k]
    assert m["group_segment_fixed_size"] == ring["group_segment_fixed_size"] + 4 * 2048, (m, ring)


def test_deep_walk_waits_hold_on_every_path():
    import isa_waits as W
    K = _ring_k()
    assert 2 * K != N_WALK, "the ring's waits and the walk's cannot be told apart by their counts"
    objdump = os.path.join(R.LLVM, "llvm-objdump")
    if not (os.path.exists(objdump) and os.path.exists(os.path.join(R.LLVM, "llvm-objcopy"))):
        pytest.skip("llvm-objdump / llvm-objcopy not found under " + R.LLVM)
    if not os.path.exists(R.LIB):
        pytest.skip("libgeglove.so not built")
    seen = 0
    with tempfile.TemporaryDirectory() as tmp:
        for co in R._gfx950_code_objects(tmp):
            asm = subprocess.run([objdump, "-d", "--mcpu=gfx950", co], check=True, capture_output=True, text=True).stdout
            if NAME not in asm:
                continue
            for name, ins in W.parse_kernels(asm).items():
                if NAME not in name:
                    continue
                seen += 1
                two, problems = W.analyse(ins, WD * GROUP)        # behind the request before the two most recent ones: the walk's image
                assert not problems, (name, problems)
                ring_st, problems = W.analyse(ins, 2 * K)         # behind the (2 K + 1)-th most recent load into LDS: stage 0's row
                assert not problems, (name, problems)
                near, problems = W.analyse(ins, GROUP)            # behind the request before the most recent one: the tile chunk's
                assert not problems, (name, problems)

                def hand(n):
                    return [i for i, (_, mn, ops) in enumerate(ins)
                            if mn == "s_waitcnt" and W._vmcnt(ops) == n and any(m.startswith("ds_read_b128") for _, m, _ in ins[i + 1:i + 8])]
                def asm_pair(i):
                    """The ring's opaque block behind wait i (tests/test_hub_ring_resources.py)."""
                    for j in range(i + 1, i + 6):
                        blk = ins[j:j + 3]
                        if [mn for _, mn, _ in blk] == ["ds_read_b128", "ds_read_b128", "s_waitcnt"] and blk[2][2].strip() == "lgkmcnt(0)" \
                                and blk[0][2].split(",")[-1].strip() == blk[1][2].split(",")[-1].replace("offset:1024", "").strip():
                            return j
                    return None
                # the ordinary walk: three unrolled steps, one per image, each behind vmcnt(8)
                walk = hand(N_WALK)
                assert len(walk) >= 3, "%s: expected three vmcnt(%d) in front of image reads, found %d" % (name, N_WALK, len(walk))
                for i in walk:
                    assert two[i] is not None, (name, i)
                    assert two[i][WD * GROUP] >= N_WALK, ("%s: on some path only %d vector-memory instructions follow the request this vmcnt(%d) at %#x waits for"
                                                          % (name, two[i][WD * GROUP], N_WALK, ins[i][0]))
                assert min(two[i][WD * GROUP] for i in walk) == N_WALK, (name, [two[i][WD * GROUP] for i in walk])
                # stage 0 of the panel pipeline and the tile chunk, as in k_epoch_ring
                ring = [i for i in hand(2 * K) if asm_pair(i) is not None]
                assert len(ring) >= 2, (name, len(ring))
                for i in ring:
                    assert ring_st[i] is not None and ring_st[i][2 * K] >= 2 * K, (name, hex(ins[i][0]), ring_st[i])
                assert min(ring_st[i][2 * K] for i in ring) == 2 * K
                tile = [i for i in hand(TILE_N_AFTER) if i not in ring]
                assert len(tile) >= 2, (name, len(tile))
                for i in tile:
                    assert near[i] is not None and near[i][GROUP] >= TILE_N_AFTER, (name, hex(ins[i][0]), near[i])
                assert min(near[i][GROUP] for i in tile) == TILE_N_AFTER
                assert not any(mn.startswith("scratch_") for _, mn, _ in ins)
                # no looser wait in front of a read of an image, and none in front of the walk's that is not the hand-counted one
                counted = set(walk) | set(ring) | set(tile)
                for i, (_, mn, ops) in enumerate(ins):
                    if mn == "s_waitcnt" and W._vmcnt(ops) is not None and near[i] is not None and i not in counted:
                        if any(m.startswith("ds_read_b128") for _, m, _ in ins[i + 1:i + 4]):
                            assert W._vmcnt(ops) <= TILE_N_AFTER, "%s: vmcnt(%d) at %#x in front of LDS reads" % (name, W._vmcnt(ops), ins[i][0])
                # ... and no tighter wait of the compiler's own right behind a walk's wait (it would take a pair out of flight every step)
                for i in walk:
                    for _, mn, ops in ins[i + 1:i + 4]:
                        assert not (mn == "s_waitcnt" and W._vmcnt(ops) is not None and W._vmcnt(ops) < N_WALK), (name, hex(ins[i][0]), mn, ops)
    assert seen == 1
