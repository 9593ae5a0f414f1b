"""ge_synth_coo on the device against the recipe in numpy (tests/synth_ref.py): I, J, X and the draw count are equal bytes on
every shape -- the recipe is integer-only, so there is no tolerance anywhere in this file -- and the trainer created from the
device-resident matrix in place (ge_glove_create_coo) equals the trainer created from the arrays ge_coo_get returns.

Each shape is the smallest that reaches one way of going wrong (the issue's list):
  (64, all, 64)                  M = 0, the diagonal only, no draw
  (3, [1,2), 3)                  one owned row
  (64, all, 2000)                the hub column full; 2.66 draws per key, past the first range (1.25 M + 1024): later ranges merge
  (65, all, 2000)                V = 2^k + 1: void ranks in the top octave
  (1000, [250,500), 30000)       a shard with row_begin > 0
  (70001, [69000,69100), 5000)   keys past 2^32 (as i * V + j)
  (70001, all, 75001)            added here: keys past 2^32 as the library forms them, (i - row_begin) * V + j
  (4097, all, 300000), 2 seeds   more than one block of every kernel, several radix passes
"""
import ctypes as C

import numpy as np
import pytest

import geglove
from geglove import capi
from helpers import make_config
import synth_ref as R

pytestmark = pytest.mark.gpu

SEED = 0xC0FFEE
SHAPES = [
    (64, 0, 64, 64, SEED),
    (3, 1, 2, 3, SEED),
    (64, 0, 64, 2000, SEED),
    (65, 0, 65, 2000, SEED),
    (1000, 250, 500, 30000, SEED),
    (70001, 69000, 69100, 5000, SEED),
    (70001, 0, 70001, 75001, SEED),
    (4097, 0, 4097, 300000, SEED),
    (4097, 0, 4097, 300000, 12345),
]
BIG = (4097, 0, 4097, 300000, SEED)


def _generate(V, rb, re_, nnz, seed):
    return capi.synth_coo(V, nnz, rows=(rb, re_), seed=seed)


def _assert_equal_bytes(got, want, what):
    for name, g, w in zip("IJX", got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        bad = np.flatnonzero(g.view(np.uint32) != w.view(np.uint32))
        assert bad.size == 0, "%s %s: %d of %d entries differ, first at %d: %r vs %r" % (what, name, bad.size, g.size, bad[0], g[bad[0]], w[bad[0]])


@pytest.mark.parametrize("V,rb,re_,nnz,seed", SHAPES)
def test_equal_to_the_model(gpu, V, rb, re_, nnz, seed):
    want = R.model(V, rb, re_, nnz, seed)
    coo = _generate(V, rb, re_, nnz, seed)
    I, J, X, row_ptr, mx = coo.get()
    draws, kernel_ms, peak = coo.stats()
    print("V %d rows [%d,%d) nnz %d seed %#x: %d draws (model %d), %.3f ms on the device, peak %d bytes" % (V, rb, re_, nnz, seed, draws, want[3], kernel_ms, peak))
    assert coo.nnz == nnz and len(I) == nnz
    _assert_equal_bytes((I, J, X), want[:3], "(%d,[%d,%d),%d)" % (V, rb, re_, nnz))
    assert draws == want[3]
    assert mx == float(np.float32(0.2))
    assert kernel_ms > 0 and peak >= 12 * nnz
    coo.close()


def test_keys_past_32_bits_are_reached():
    """i * V + j passes 2^32 at the shard of V = 70001; the library keys a draw by (i - row_begin) * V + j, which passes 2^32 only
    with all rows of that V owned -- hence the added shape."""
    V, rb, re_, nnz, seed = SHAPES[5]
    assert (re_ - 1) * V > 2 ** 32 > (re_ - rb) * V
    V, rb, re_, nnz, seed = SHAPES[6]
    I, J, X, draws = R.model(V, rb, re_, nnz, seed)
    assert int(((I.astype(np.int64) - rb) * V + J).max()) > 2 ** 32


def test_second_range_runs_at_the_hub_shape():
    """The first range is min(budget, M + M / 4 + 1024) draws (synth.hip); this shape needs more, so kept keys meet new draws."""
    V, rb, re_, nnz, seed = SHAPES[2]
    M = nnz - (re_ - rb)
    assert R.model(V, rb, re_, nnz, seed)[3] > M + M // 4 + 1024
    hub, count, most = R.hub_column(R.model(V, rb, re_, nnz, seed)[1], V)
    assert count == most == re_ - rb


def test_too_dense_is_refused(gpu):
    with pytest.raises(R.TooDense):
        R.model(64, 0, 64, 4096)
    with pytest.raises(capi.GeError) as e:
        capi.synth_coo(64, 4096)
    assert e.value.status == capi.GE_ERR_ARG and "too dense" in str(e.value)


def test_equal_arguments_give_equal_bytes(gpu):
    V, rb, re_, nnz, seed = SHAPES[4]
    a = _generate(V, rb, re_, nnz, seed); b = _generate(V, rb, re_, nnz, seed)
    ga, gb = a.get(), b.get()
    for x, y in zip(ga[:4], gb[:4]):
        assert x.tobytes() == y.tobytes()
    assert a.stats()[0] == b.stats()[0]
    other = _generate(V, rb, re_, nnz, seed + 1).get()
    assert other[1].tobytes() != ga[1].tobytes()                # and the seed matters


def test_shards_share_the_relabelling(gpu):
    V, nnz = 1000, 30000
    hubs = []
    for rb, re_ in ((250, 500), (500, 750)):
        I, J, X, row_ptr, mx = _generate(V, rb, re_, nnz, SEED).get()
        _assert_equal_bytes((I, J, X), R.model(V, rb, re_, nnz, SEED)[:3], "shard [%d,%d)" % (rb, re_))
        hub, count, most = R.hub_column(J, V)
        assert count == most == re_ - rb                        # rank 0's column is the busiest of this shard
        hubs.append(hub)
    assert hubs[0] == hubs[1]


def test_host_views_after_device_views(gpu):
    V, rb, re_, nnz, seed = SHAPES[4]
    coo = _generate(V, rb, re_, nnz, seed)
    dev, dI, dJ, dX = coo.device_views()
    assert dev == 0 and dI and dJ and dX and len({dI, dJ, dX}) == 3
    first = coo.get(); again = coo.get()
    assert coo.device_views() == (dev, dI, dJ, dX)              # the device arrays stay where they are
    for x, y in zip(first[:4], again[:4]):
        assert x.tobytes() == y.tobytes()
    I, J, X, row_ptr, mx = first
    _assert_equal_bytes((I, J, X), R.model(V, rb, re_, nnz, seed)[:3], "host views")
    assert row_ptr.shape == (V + 1,) and row_ptr[0] == 0 and row_ptr[-1] == nnz
    assert np.array_equal(row_ptr, np.concatenate([[0], np.cumsum(np.bincount(I, minlength=V))]))
    coo.close()


# ---- the trainer on the device-resident matrix ----

INFO_KEYS = ("group_width", "vector_width", "blocks", "groups_in_flight", "hot_columns", "hot_nonzeros", "hot_threshold", "chunks", "hub_chunks",
             "long_rows", "shared_chunks", "flush_min", "row_stride", "runs", "schedule_bytes")


@pytest.fixture(scope="module")
def big(gpu):
    V, rb, re_, nnz, seed = BIG
    coo = _generate(V, rb, re_, nnz, seed)
    I, J, X, row_ptr, mx = coo.get()
    yield coo, geglove.CooMatrix(V, I, J, X, mx)
    coo.close()


@pytest.mark.parametrize("method", ["glove", "pglove"])
def test_trainer_layout_equals_the_array_route(big, method):
    coo, host = big
    cfg = make_config(16, method=method, seed=7)
    a = geglove.Adagrad(geglove.DeviceCooMatrix(coo), cfg, cfg.costFunction())
    b = geglove.Adagrad(host, cfg, cfg.costFunction())
    ia, ib = a.info(), b.info()
    assert {k: ia[k] for k in INFO_KEYS} == {k: ib[k] for k in INFO_KEYS}
    assert ia["chunks"] > ia["hub_chunks"] > 0 and ia["hot_columns"] > 0 and ia["groups_in_flight"] > 1
    for it in (0, 3):
        assert a.epoch_order(it).tobytes() == b.epoch_order(it).tobytes()
    a.close(); b.close()


@pytest.mark.parametrize("method", ["glove", "pglove"])
def test_trainer_one_worker_epoch_is_bit_equal(gpu, big, method):
    _, host = big
    V, rb, re_, nnz, seed = BIG
    cfg = make_config(16, method=method, seed=7, workers=1)
    coo = _generate(V, rb, re_, nnz, seed)                      # a matrix of its own: destroyed before the first epoch
    a = geglove.Adagrad(geglove.DeviceCooMatrix(coo), cfg, cfg.costFunction())
    coo.close()
    b = geglove.Adagrad(host, cfg, cfg.costFunction())
    ca, cb = a.epoch(0), b.epoch(0)
    assert np.isfinite(ca) and np.float64(ca).tobytes() == np.float64(cb).tobytes()
    sa, sb = a.state(), b.state()
    assert set(sa) == set(capi.STATE_NAMES) and len(sa) == 8
    for name in capi.STATE_NAMES:
        assert sa[name].tobytes() == sb[name].tobytes(), name
    a.close(); b.close()


def test_trainer_host_route_is_ge_glove_create(big):
    """A deterministic, Java-order handle cannot read the device arrays in place: it takes the host route and equals ge_glove_create."""
    coo, host = big
    cfg = make_config(16, method="glove", seed=7, mode="deterministic", shuffle="java")
    a = geglove.Adagrad(geglove.DeviceCooMatrix(coo), cfg, cfg.costFunction())
    b = geglove.Adagrad(host, cfg, cfg.costFunction())
    ca, cb = a.epoch(0), b.epoch(0)
    assert np.float64(ca).tobytes() == np.float64(cb).tobytes()
    assert a.perm().tobytes() == b.perm().tobytes()
    sa, sb = a.state(), b.state()
    for name in capi.STATE_NAMES:
        assert sa[name].tobytes() == sb[name].tobytes(), name
    a.close(); b.close()


def test_trainer_refuses_a_mismatch(big):
    coo, host = big
    V, nnz = BIG[0], BIG[3]
    L = capi.lib()

    def create(**kw):
        cfg = capi.GloveCfg(); L.ge_glove_cfg_default(C.byref(cfg))
        cfg.vocab_size, cfg.dim = V, 16
        for k, v in kw.items():
            setattr(cfg, k, v)
        h = C.c_void_p()
        st = L.ge_glove_create_coo(C.byref(cfg), coo.handle, C.byref(h))
        err = L.ge_last_error().decode()
        if st == capi.GE_OK:
            L.ge_glove_destroy(h)
        return st, err

    assert create()[0] == capi.GE_OK                            # nnz = 0, xmax = 0: both taken from the matrix
    assert create(nnz=nnz, xmax=float(np.float32(0.2)))[0] == capi.GE_OK
    for kw, msg in ((dict(nnz=nnz - 1), "nnz"), (dict(xmax=0.25), "xmax"), (dict(vocab_size=V + 1), "vocab_size"), (dict(device=1), "device"),
                    (dict(row_begin=0, row_end=V - 1), "rows")):
        st, err = create(**kw)
        assert st == capi.GE_ERR_ARG and msg in err, (kw, st, err)
