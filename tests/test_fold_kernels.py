"""Fold-in without a GPU: what the compiler made of k_fold_rows (every instance a handle can reach is in the gfx950 code object,
without scratch, spills or LDS, at four waves per SIMD), properties of the numpy model of the section (tests/fold_ref.py), and
whether that model is of any use: rows folded in from zero against the oracle's trained tables fit their own nonzeros better
than the rows the oracle trained."""
import re

import numpy as np

import fold_ref as FR
import kernel_model as KM
import oracle as O
import test_kernel_resources as KR
from geglove import synth

VGPRS_PER_SIMD_LANE = 512           # gfx950: 512 registers per lane of a SIMD, shared by its resident waves
CLAIMED_WAVES_PER_SIMD = 4


def _instances():
    out = {}
    for name, m in KR._kernel_metadata().items():
        hit = re.search(r"11k_fold_rowsILi(\d+)ELi(\d+)ELb(\d)EE", name)            # <VW, NCH, EMB16>
        if hit:
            out[tuple(int(g) for g in hit.groups())] = m
    return out


def test_every_reachable_instance_is_in_the_code_object_at_four_waves_per_simd():
    got = _instances()
    want = set()
    for D in KM.SHAPE_TABLE_DIMS:
        vw, nch, _ = KM.lane_shape(D)
        want.add((vw, nch, 0))
        if D in KM.BF16_DIMS:
            want.add((4, nch, 1))
    assert len(want) == 16 and want == set(got), (sorted(want - set(got)), sorted(set(got) - want))
    for inst in sorted(want):
        m = got[inst]
        granule = (m["vgpr_count"] + 7) // 8 * 8                       # registers are allocated in eights
        print("k_fold_rows<%d, %d, %s>: %d registers per lane, %d B of scratch" % (inst[0], inst[1], "bf16" if inst[2] else "fp32",
                                                                                 m["vgpr_count"], m["private_segment_fixed_size"]))
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (inst, m)
        assert m["group_segment_fixed_size"] == 0, (inst, m)
        assert granule * CLAIMED_WAVES_PER_SIMD <= VGPRS_PER_SIMD_LANE, (inst, m)
    assert KM.lane_shape(1028) is None                                  # five chunks: ge_glove_fold_create refuses the dim


def _small_set(seed, V=40, D=6, lengths=(0, 1, 2, 5, 9, 0, 3)):
    rng = np.random.default_rng(seed)
    table = (rng.standard_normal((V, D)) * 0.3).astype(np.float32)
    bias = (rng.standard_normal(V) * 0.1).astype(np.float32)
    row_ptr = np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)
    idx = rng.integers(0, V, row_ptr[-1]).astype(np.int32)
    X = (0.01 + 0.4 * rng.random(row_ptr[-1])).astype(np.float32)
    init = (rng.standard_normal((len(lengths), D)) * 0.1).astype(np.float32)
    init_b = (rng.standard_normal(len(lengths)) * 0.1).astype(np.float32)
    return D, row_ptr, idx, X, table, bias, init, init_b


def _permuted(row_ptr, idx, X, perm):
    lens = np.diff(row_ptr)[perm]
    ptr = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    take = np.concatenate([np.arange(row_ptr[r], row_ptr[r + 1]) for r in perm]).astype(np.int64)
    return ptr, idx[take], X[take]


def test_a_permuted_set_gives_permuted_results():
    D, row_ptr, idx, X, table, bias, init, init_b = _small_set(1)
    kw = dict(xmax=0.2, epochs=3, shuffle="device", seed=7, lr=0.05)
    rows, fb, c, hist = FR.fold(D, row_ptr, idx, X, table, bias, init_rows=init, init_bias=init_b, **kw)
    perm = np.array([4, 0, 6, 2, 1, 5, 3])
    ptr2, idx2, X2 = _permuted(row_ptr, idx, X, perm)
    rows2, fb2, c2, hist2 = FR.fold(D, ptr2, idx2, X2, table, bias, init_rows=init[perm], init_bias=init_b[perm], **kw)
    assert np.array_equal(FR.bits(rows2), FR.bits(rows[perm])) and np.array_equal(FR.bits(fb2), FR.bits(fb[perm]))
    assert np.array_equal(FR.bits(c2), FR.bits(c[perm]))
    assert np.allclose(hist, hist2, rtol=1e-12)                        # the same terms summed in another order
    assert np.any(FR.bits(rows) != FR.bits(init))


def test_an_empty_row_returns_its_init_and_zero_costs():
    D, row_ptr, idx, X, table, bias, init, init_b = _small_set(2)
    rows, fb, c, _ = FR.fold(D, row_ptr, idx, X, table, bias, xmax=0.2, epochs=4, shuffle="none", init_rows=init, init_bias=init_b)
    for r in (0, 5):
        assert np.array_equal(FR.bits(rows[r]), FR.bits(init[r])) and fb[r] == init_b[r] and not c[r].any()
    rows, fb, c, _ = FR.fold(D, row_ptr, idx, X, table, bias, xmax=0.2, epochs=4, shuffle="none")
    assert not rows[0].any() and fb[0] == 0 and not c[0].any()


def test_epochs_in_one_call_are_not_two_calls():
    """There is no resume: the accumulators restart with every run, so 4 epochs differ from 2 epochs continued by 2 more -- while
    the first two epochs of the longer run are the shorter run's."""
    D, row_ptr, idx, X, table, bias, _, _ = _small_set(3)
    kw = dict(xmax=0.2, shuffle="none", lr=0.05)
    r4, b4, c4, _ = FR.fold(D, row_ptr, idx, X, table, bias, epochs=4, **kw)
    r2, b2, c2, _ = FR.fold(D, row_ptr, idx, X, table, bias, epochs=2, **kw)
    r22, b22, c22, _ = FR.fold(D, row_ptr, idx, X, table, bias, epochs=2, init_rows=r2, init_bias=b2, **kw)
    assert np.array_equal(FR.bits(c4[:, :2]), FR.bits(c2))
    live = np.diff(row_ptr) > 0
    # (a continued run's very first cost term is the long run's: it is taken before the first update meets the fresh accumulators)
    assert np.all(np.any(FR.bits(r4[live]) != FR.bits(r22[live]), axis=1)) and np.all(c4[live, 3] != c22[live, 1])


def _cost64(rows, fb, row_ptr, idx, X, table, bias, xmax):
    """The GloVe cost of every row on its own nonzeros in plain fp64."""
    out = np.zeros(len(rows))
    for r in range(len(rows)):
        k = slice(int(row_ptr[r]), int(row_ptr[r + 1]))
        x = X[k].astype(np.float64)
        w = np.where(x > xmax, 1.0, (x / xmax) ** 0.75)
        ic = table[idx[k]].astype(np.float64) @ rows[r].astype(np.float64) + fb[r] + bias[idx[k]] - np.log(x)
        out[r] = np.sum(0.5 * w * ic * ic)
    return out


def test_folded_rows_fit_their_nonzeros_better_than_the_trained_rows():
    """The oracle trains synthetic_coo(300, 4000, seed=9) at D = 50 for 30 epochs; every vertex's own row is then folded in from
    zero against the trained context side (E = 50, lr 0.05, shuffle none)."""
    V, D, E = 300, 50, 50
    I, J, X, xmax = synth.synthetic_coo(V, 4000, seed=9)
    g = O.Glove(V, D, I, J, X, xmax, seed=5)
    for _ in range(30):
        g.epoch()
    st = {k: np.ascontiguousarray(v, np.float32) for k, v in g.state().items()}
    g.close()
    order = np.argsort(I, kind="stable")
    row_ptr = np.concatenate(([0], np.cumsum(np.bincount(I, minlength=V)))).astype(np.int64)
    idx, Xs = J[order].astype(np.int32), X[order].astype(np.float32)
    table, bias = st["context"].reshape(V, D), st["cbias"]
    rows, fb, c, hist = FR.fold(D, row_ptr, idx, Xs, table, bias, xmax=xmax, epochs=E, shuffle="none", lr=0.05)
    trained = _cost64(st["focus"].reshape(V, D), st["fbias"], row_ptr, idx, Xs, table, bias, xmax)
    folded = _cost64(rows, fb, row_ptr, idx, Xs, table, bias, xmax)
    start = _cost64(np.zeros((V, D), np.float32), np.zeros(V, np.float32), row_ptr, idx, Xs, table, bias, xmax)
    print("fp64 cost on the rows' own nonzeros: from zero %.6g, folded %.6g, trained %.6g; %d of %d rows worse than their trained row"
          % (start.sum(), folded.sum(), trained.sum(), int(np.sum(folded > trained)), V))
    print("cost_history (the bit model): epoch 0 %.6g, 1 %.6g, 5 %.6g, 20 %.6g, 49 %.6g" % (hist[0], hist[1], hist[5], hist[20], hist[49]))
    # The bit model on the CPU (printed above): 1048.12 from the zero start, 336.867 folded, 415.804 trained -- a fifth to spare --
    # and 0 of 300 rows worse than their trained row.  A plain-numpy restatement gave 1048, 337 and 416.
    assert folded.sum() < trained.sum()
    # cost_history of the bit model (each epoch's running cost, taken before its updates): 681.371, 600.037, .. 484.257 (5),
    # 402.723 (20), 350.589 (49)
    assert np.all(np.diff(hist[1:]) <= 0), hist
