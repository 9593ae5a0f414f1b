"""What the compiler made of k_epoch_ring, the panel kernel whose stage 0 keeps the focus pairs of RING_K rows in flight
(csrc/glove.hip), read from the built library's gfx950 code object (no GPU needed):
  * one kernel of its own name; k_adagrad_runs, k_epoch_tiles and k_epoch_panels are as many as they were (56 / 1 / 1);
  * launch-bounded for three wavefronts per SIMD: at most 168 registers, nothing in scratch, three workgroups in a CU's 160 KB of LDS
    with the ring's RING_K + 1 images;
  * stage 0 reads the image of row t behind a hand-counted `s_waitcnt vmcnt(2 RING_K)`: it stores nothing to memory, so behind
    the request of row t only the two loads of each of the RING_K later requests are certain.  The path analysis of
    tests/isa_waits.py, with a window of 2 RING_K loads into LDS, holds the count on every path; the ordinary walk's and the tile
    chunk's vmcnt(4) are held with the window of one request, as in k_epoch_panels;
  * the image is chosen at run time and read by `ds_read_b128` from inline asm: no wait the compiler made stands in front of it.
Skipped where the LLVM tools of the ROCm image are missing.
"""
import os
import re
import subprocess
import tempfile

import pytest

import test_kernel_resources as R

GROUP = 2              # loads into LDS per request: the row and its accumulator row
TILE_N_AFTER = 4       # csrc/glove.hip: a walk that stores its pair to memory
NAME = "k_epoch_ring"


def _ring_k():
    """RING_K of csrc/glove.hip: the default of the GE_RING_K macro."""
    src = open(os.path.join(R.REPO, "graph-embeddings_amd", "csrc", "glove.hip")).read()
    m = re.search(r"#define GE_RING_K (\d+)", src)
    assert m, "csrc/glove.hip no longer defines GE_RING_K"
    return int(m.group(1))


def test_ring_kernel_keeps_its_state_in_registers():
    meta = R._kernel_metadata()
    ring = {k: v for k, v in meta.items() if NAME in k}
    assert len(ring) == 1, sorted(ring)
    (name, m), = ring.items()
    assert not any(s in name for s in ("k_epoch_panels", "k_epoch_tiles", "k_adagrad_runs"))
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
    assert m["vgpr_count"] <= 168, (name, m)
    assert m["group_segment_fixed_size"] * 3 <= 160 * 1024, (name, m)
    panels = [v for k, v in meta.items() if "k_epoch_panels" in k]
    assert len(panels) == 1
    # the ring: RING_K + 1 images of 2 KB beside everything k_epoch_panels holds
    assert m["group_segment_fixed_size"] == panels[0]["group_segment_fixed_size"] + (_ring_k() + 1) * 2048, (m, panels[0])
    assert len([k for k in meta if "k_adagrad_runs" in k]) == 56
    assert len([k for k in meta if "k_epoch_tiles" in k]) == 1


def test_ring_kernel_waits_hold_on_every_path():
    import isa_waits as W
    K = _ring_k()
    assert 2 <= K <= 9 and 2 * K < 64
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
                deep, problems = W.analyse(ins, 2 * K)       # behind the (2 K + 1)-th most recent load into LDS: the request of row t
                assert not problems, (name, problems)
                near, problems = W.analyse(ins, GROUP)
                assert not problems, (name, problems)

                def hand(n):
                    return [i for i, (_, mn, ops) in enumerate(ins)
                            if mn == "s_waitcnt" and W._vmcnt(ops) == n and any(m.startswith("ds_read") for _, m, _ in ins[i + 1:i + 8])]
                def asm_pair(i):
                    """Where the asm's block stands behind wait i: two 16-byte reads from one address register and `s_waitcnt
                    lgkmcnt(0)` right behind them (the compiler cannot split the block; its own image reads wait later and looser)."""
                    for j in range(i + 1, i + 6):
                        blk = ins[j:j + 3]
                        if [mn for _, mn, _ in blk] == ["ds_read_b128", "ds_read_b128", "s_waitcnt"] and blk[2][2].strip() == "lgkmcnt(0)" \
                                and blk[0][2].split(",")[-1].strip() == blk[1][2].split(",")[-1].replace("offset:1024", "").strip():
                            return j
                    return None
                # stage 0: two unrolled rows (the image the pair is handed on in alternates), each reading its ring image
                ring = [i for i in hand(2 * K) if asm_pair(i) is not None]
                assert len(ring) >= 2, "%s: expected vmcnt(%d) in front of the ring's image reads, found %d" % (name, 2 * K, len(ring))
                if 2 * K != TILE_N_AFTER:
                    assert ring == hand(2 * K), (name, "a vmcnt(%d) in front of an LDS read that is not the ring's" % (2 * K))
                for i in ring:
                    assert deep[i] is not None, (name, i)
                    assert deep[i][2 * K] >= 2 * K, ("%s: on some path only %d vector-memory instructions follow the request this vmcnt(%d) at %#x waits for"
                                                     % (name, deep[i][2 * K], 2 * K, ins[i][0]))
                assert min(deep[i][2 * K] for i in ring) == 2 * K, (name, [deep[i][2 * K] for i in ring])
                # the ordinary walk's two unrolled steps and the tile chunk's two unrolled rows, as in k_epoch_panels
                walk = [i for i in hand(TILE_N_AFTER) if i not in ring]
                assert len(walk) >= 4, "%s: expected vmcnt(%d) in front of image reads, found %d" % (name, TILE_N_AFTER, len(walk))
                for i in walk:
                    assert near[i] is not None and near[i][GROUP] >= TILE_N_AFTER, (name, hex(ins[i][0]), near[i])
                assert min(near[i][GROUP] for i in walk) == TILE_N_AFTER
                assert sum(1 for _, mn, _ in ins if mn == "s_barrier") >= 4
                assert not any(mn.startswith("scratch_") for _, mn, _ in ins)
                # no looser wait in front of a read of an image: the ring's reads take 2 K, every other one at most the walk's 4
                counted = set(ring) | set(walk)
                for i, (_, mn, ops) in enumerate(ins):
                    if mn == "s_waitcnt" and W._vmcnt(ops) is not None and near[i] is not None and i not in counted:
                        if any(m.startswith("ds_read_b128") for _, m, _ in ins[i + 1:i + 4]):
                            assert W._vmcnt(ops) <= TILE_N_AFTER, "%s: vmcnt(%d) at %#x in front of LDS reads" % (name, W._vmcnt(ops), ins[i][0])
                # ... and no tighter wait of the compiler's own next to a ring read (a vmcnt(0) there would drain the ring every row)
                for i in ring:
                    for _, mn, ops in ins[i - 8:i] + ins[i + 1:i + 4]:
                        assert not (mn == "s_waitcnt" and W._vmcnt(ops) is not None and W._vmcnt(ops) < 2 * K), (name, hex(ins[i][0]), mn, ops)
    assert seen == 1
