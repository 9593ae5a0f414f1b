"""What the compiler made of the trainer kernel, read from the built library's gfx950 code objects (no GPU needed).

The walk of k_adagrad_runs keeps a resident row pair in registers and counts its own memory waits; two ways of losing that
silently were met while it was written and are pinned here:
  * a construct that makes the compiler keep the run's scalars in an indexed private array puts 400 - 900 bytes of scratch under every
    lane and triples the epoch (seen with `lane == 0 ? ab : lane == 1 ? gab : hab` in close_run) -- no instance may use scratch
    beyond the handful of spill slots the launch-bounded instances have outside the walk;
  * the bench instance (fp32 fat rows, four floats per lane, one register chunk) must fit five waves per SIMD: 96 registers.
Skipped where the LLVM tools of the ROCm image are missing.
"""
import os
import re
import struct
import subprocess
import tempfile

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "graph-embeddings_amd", "lib", "libgeglove.so")
LLVM = "/opt/rocm/lib/llvm/bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _kernel_metadata():
    """{kernel name: {field: int}} for every kernel of every gfx950 code object in libgeglove.so's .hip_fatbin."""
    objcopy, readelf = os.path.join(LLVM, "llvm-objcopy"), os.path.join(LLVM, "llvm-readelf")
    if not (os.path.exists(objcopy) and os.path.exists(readelf)):
        pytest.skip("llvm-objcopy / llvm-readelf not found under " + LLVM)
    if not os.path.exists(LIB):
        pytest.skip("libgeglove.so not built")
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        fat = os.path.join(tmp, "fatbin.bin")
        subprocess.run([objcopy, "--dump-section", ".hip_fatbin=" + fat, LIB, os.path.join(tmp, "discard")], check=True)
        blob = open(fat, "rb").read()
        pos = 0
        while True:
            at = blob.find(MAGIC, pos)
            if at < 0:
                break
            (count,) = struct.unpack_from("<Q", blob, at + len(MAGIC))
            cur = at + len(MAGIC) + 8
            for _ in range(count):
                offset, size, tlen = struct.unpack_from("<QQQ", blob, cur)
                cur += 24
                triple = blob[cur:cur + tlen].decode()
                cur += tlen
                if "gfx950" not in triple or size == 0:
                    continue
                elf = os.path.join(tmp, "co.elf")
                open(elf, "wb").write(blob[at + offset:at + offset + size])
                notes = subprocess.run([readelf, "--notes", elf], check=True, capture_output=True, text=True).stdout
                for block in notes.split("    .name:")[1:]:
                    name = block.split()[0]
                    # a kernel's fields surround its .name line: take them from the text between the neighbouring .args / .name markers
                    start = notes.index("    .name:" + block[:len(name) + 12])
                    head = notes.rfind("- .", 0, start)
                    tail = notes.find("\n  - .", start)
                    text = notes[head:tail if tail > 0 else len(notes)]
                    out[name] = {k: int(v) for k, v in re.findall(r"\.(private_segment_fixed_size|vgpr_count|vgpr_spill_count|group_segment_fixed_size):\s+(\d+)", text)}
            pos = at + len(MAGIC)
    return out


def _gfx950_code_objects(tmp):
    """Paths of the gfx950 code objects of libgeglove.so's .hip_fatbin, written under tmp."""
    objcopy = os.path.join(LLVM, "llvm-objcopy")
    fat = os.path.join(tmp, "fatbin.bin")
    subprocess.run([objcopy, "--dump-section", ".hip_fatbin=" + fat, LIB, os.path.join(tmp, "discard")], check=True)
    blob = open(fat, "rb").read()
    out, pos = [], 0
    while True:
        at = blob.find(MAGIC, pos)
        if at < 0:
            return out
        (count,) = struct.unpack_from("<Q", blob, at + len(MAGIC))
        cur = at + len(MAGIC) + 8
        for _ in range(count):
            offset, size, tlen = struct.unpack_from("<QQQ", blob, cur)
            cur += 24
            triple = blob[cur:cur + tlen].decode()
            cur += tlen
            if "gfx950" in triple and size:
                path = os.path.join(tmp, "co%d.elf" % len(out))
                open(path, "wb").write(blob[at + offset:at + offset + size])
                out.append(path)
        pos = at + len(MAGIC)


def test_hand_counted_wait_holds_on_every_path():
    """VERDICT r02 #4 / ADVICE r02: the walk of k_adagrad_runs waits for an LDS image with `s_waitcnt vmcnt(N_AFTER)`, which is long
    enough only if at least N_AFTER vector-memory instructions follow the image's request on EVERY path (glove.hip, "The wait is
    counted by hand").  Every instance is disassembled and the minimum over all control-flow paths computed (tests/isa_waits.py);
    the counted stores are issued unconditionally in the source for exactly this reason (lanes past the row are dropped by the
    descriptor, not by an exec-mask branch), so the minimum EQUALS N_AFTER -- a compiler or code change that drops, predicates or
    moves one of them fails here instead of letting a wave read a stale image."""
    import isa_waits as W
    objdump = os.path.join(LLVM, "llvm-objdump")
    if not (os.path.exists(objdump) and os.path.exists(os.path.join(LLVM, "llvm-objcopy"))):
        pytest.skip("llvm-objdump / llvm-objcopy not found under " + LLVM)
    if not os.path.exists(LIB):
        pytest.skip("libgeglove.so not built")
    seen = 0
    with tempfile.TemporaryDirectory() as tmp:
        for co in _gfx950_code_objects(tmp):
            asm = subprocess.run([objdump, "-d", "--mcpu=gfx950", co], check=True, capture_output=True, text=True).stdout
            if "k_adagrad_runs" not in asm:
                continue
            for name, ins in W.parse_kernels(asm).items():
                targs = W.template_args(name)
                if targs is None:
                    continue
                seen += 1
                n = W.n_after(*targs)
                group = W.n_tab_dma(*targs)[1]
                state, problems = W.analyse(ins, group)
                assert not problems, (name, problems)
                # the hand-counted waits: vmcnt(N_AFTER) with the image's ds_reads right behind them -- one per unrolled step
                hand = []
                for i, (_, mn, ops) in enumerate(ins):
                    if mn == "s_waitcnt" and W._vmcnt(ops) == n and any(m.startswith("ds_read") for _, m, _ in ins[i + 1:i + 8]):
                        hand.append(i)
                assert len(hand) >= 2, "%s: expected vmcnt(%d) in front of the image reads of both unrolled steps, found %d" % (name, n, len(hand))
                for i in hand:
                    assert state[i] is not None, (name, i)
                    k2 = state[i][group]
                    assert k2 >= n, ("%s: on some path only %d vector-memory instructions follow the request this vmcnt(%d) at %#x waits for"
                                     % (name, k2, n, ins[i][0]))
                assert min(state[i][group] for i in hand) == n, (name, "N_AFTER is no longer the tight count", [state[i][group] for i in hand], n)
                # every wait in front of a read of an image (whatever its immediate) must cover that image's request
                for i, (_, mn, ops) in enumerate(ins):
                    if mn == "s_waitcnt" and W._vmcnt(ops) is not None and state[i] is not None and i not in hand:
                        if any(m.startswith("ds_read_b128") or m.startswith("ds_read_b64") for _, m, _ in ins[i + 1:i + 4]) and W._vmcnt(ops) > n:
                            assert False, "%s: vmcnt(%d) at %#x in front of LDS reads is looser than N_AFTER = %d" % (name, W._vmcnt(ops), ins[i][0], n)
                if targs == (4, 1, 0, False, True):                       # the bench instance: nothing of the walk in scratch
                    assert not any(mn.startswith("scratch_") for _, mn, _ in ins), name
    assert seen == 56, "expected every instance of k_adagrad_runs, analysed %d" % seen


def test_wait_analysis_sees_a_predicated_store():
    """The analysis itself, on a six-line loop: one load into LDS per request, one store per step, vmcnt(2) in front of the read.
    With the store issued unconditionally two instructions follow the request in use on every path; behind an s_cbranch_execz
    the path that skips it has one, and the wait no longer covers the request."""
    import isa_waits as W

    def listing(guarded):
        rows = ["buffer_load_dwordx4 v1, s[0:3], 0 offen lds",        # request image A
                "buffer_load_dwordx4 v[8:11], v1, s[12:15], 0 offen", # the resident row
                "buffer_load_dwordx4 v1, s[4:7], 0 offen lds",        # loop: request the other image
                "s_waitcnt vmcnt(2)",                                   #   wait for this one: the store and the request behind it
                "ds_read_b128 v[4:7], v2"]
        rows += ["s_cbranch_execz 1"] if guarded else []
        rows += ["buffer_store_dwordx4 v[4:7], v1, s[8:11], 0 offen",
                 "s_cbranch_scc1 %d" % (65536 - (6 if guarded else 5)),  # back to the request
                 "s_endpgm"]
        text = "0000000000001000 <k>:\n"
        for k, r in enumerate(rows):
            text += "\t%s // %012X: 00000000\n" % (r, 0x1000 + 4 * k)
        return W.parse_kernels(text)["k"]

    for guarded, want in ((False, 2), (True, 1)):
        ins = listing(guarded)
        st, problems = W.analyse(ins, 1)
        assert not problems
        wait = [i for i, (_, m, _) in enumerate(ins) if m == "s_waitcnt"][0]
        assert st[wait][1] == want, (guarded, st[wait])


def test_trainer_kernel_instances_keep_their_state_in_registers():
    meta = {k: v for k, v in _kernel_metadata().items() if "k_adagrad_runs" in k}
    assert len(meta) == 56, "expected every (vector width, chunks, optimiser, bf16, fat) instance, found %d" % len(meta)
    for name, m in meta.items():
        assert m["private_segment_fixed_size"] <= 64, (name, m)          # spill slots of the launch-bounded instances: 20 - 28 bytes
    bench = [v for k, v in meta.items() if "ILi4ELi1ELi0ELb0ELb1E" in k]      # <VW 4, NCH 1, AdaGrad, fp32, fat>
    assert len(bench) == 1
    assert bench[0]["vgpr_count"] <= 96 and bench[0]["vgpr_spill_count"] == 0 and bench[0]["private_segment_fixed_size"] == 0, bench[0]
    # two LDS images per wave (row + accumulator row, 1 KB each) x 4 waves + the atomic strips: five workgroups fit a CU's 160 KB
    assert bench[0]["group_segment_fixed_size"] * 5 <= 160 * 1024, bench[0]


def _reachable_instances():
    """Every instance a Hogwild handle can run, from the lane-shape rule over every dim up to past the largest one accepted."""
    import kernel_model as K
    return {inst for D in range(1, 1100) for inst in K.instances(D)}


def test_every_reachable_trainer_instance_is_in_the_code_object():
    """pick_hogwild's 56 targets (16 lane shapes x 3 optimisers + 8 bf16 shapes) are all compiled for gfx950, and nothing else is: VW 1 / VW 2
    without fat rows is not instantiated because no dim reaches it (an odd dim, or twice an odd number, never fills 64 lanes)."""
    import kernel_model as K
    reach = _reachable_instances()
    assert len(reach) == 56
    assert len({i for i in reach if not i[3]}) == 48 and len({i for i in reach if i[3]}) == 8
    names = [k for k in _kernel_metadata() if "k_adagrad_runs" in k]
    for inst in sorted(reach):
        hits = [k for k in names if K.mangled(inst) in k]
        assert len(hits) == 1, (inst, K.mangled(inst), hits)
    unreachable = [k for k in names if not any(K.mangled(i) in k for i in reach)]
    assert not unreachable and len(names) == 56


def test_shape_table_covers_every_reachable_instance():
    """tests/kernel_model.py SHAPE_DIMS is what the GPU shape tests (test_kernel_shapes_gpu.py) iterate over: its dims reach all 56
    instances, each dim sits in the shape it is listed under, and the lane-63 dims put the bias in the last lane of the last
    chunk.  Leaving out the dims of any one shape leaves instances uncovered -- checked here for every shape."""
    import kernel_model as K
    reach = _reachable_instances()

    def covered(dims):
        return {inst for D in dims for inst in K.instances(D)}

    assert covered(K.SHAPE_TABLE_DIMS) == reach
    assert len(K.SHAPE_DIMS) == 16 and len(K.SHAPE_TABLE_DIMS) == 28
    for shape, dims in K.SHAPE_DIMS.items():
        vw, nch, fat = shape
        for D in dims:
            assert K.lane_shape(D) == shape, (D, shape)
        assert dims[0] == min(D for D in range(1, 1100) if K.lane_shape(D) == shape), (shape, dims)      # the smallest dim of its shape
        if fat:
            assert (max(dims) // vw) % 64 == 63 and max(dims) // (64 * vw) == nch - 1, (shape, dims)
        else:
            assert dims == (256 * nch,)
        others = [D for D in K.SHAPE_TABLE_DIMS if D not in dims]
        assert covered(others) < reach, ("dropping", shape, "loses no instance")
    # the largest dims accepted, and the first refused, of each vector width
    assert K.lane_shape(255) == (1, 4, True) and K.lane_shape(257) is None
    assert K.lane_shape(510) == (2, 4, True) and K.lane_shape(514) is None
    assert K.lane_shape(1024) == (4, 4, False) and K.lane_shape(1028) is None
