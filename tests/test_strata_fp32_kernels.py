"""GE_ARITH_FP32 without a GPU: what the compiler made of k_strata_fp32 (every instance a dim can reach is in the gfx950 code
object, none uses scratch, all leave room for two waves per SIMD), and the numpy model of the arithmetic
(tests/strata_fp32_ref.py) against the oracle replaying the same stratified order in Java's arithmetic."""
import re

import numpy as np
import pytest

import kernel_model as KM
import oracle as O
import strata_ref as S
import strata_fp32_ref as R
import test_kernel_resources as KR
from geglove import synth
from helpers import cost_kind

VGPRS_PER_SIMD_LANE = 512           # gfx950: 512 registers per lane of a SIMD, shared by its resident waves
CLAIMED_WAVES_PER_SIMD = 2          # 256 CUs x 4 SIMDs x 2: P = 2048 tiles resident at once


def _instances():
    out = {}
    for name, m in KR._kernel_metadata().items():
        hit = re.search(r"13k_strata_fp32ILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)EE", name)      # <VW, NCH, OPT, ABLATE>
        if hit and int(hit.group(4)) == 0:                                               # ABLATE 0: what an epoch runs
            out[tuple(int(g) for g in hit.groups()[:3])] = m
    return out


def test_every_reachable_instance_is_in_the_code_object_without_scratch_at_two_waves_per_simd():
    got = _instances()
    want = set()
    for D in KM.SHAPE_TABLE_DIMS:
        vw, nch, _ = KM.lane_shape(D)
        want |= {(vw, nch, opt) for opt in KM.OPTS}
    assert len(want) == 36 and want <= set(got), sorted(want - set(got))
    for inst in sorted(want):
        m = got[inst]
        granule = (m["vgpr_count"] + 7) // 8 * 8                       # registers are allocated in eights
        print("k_strata_fp32<%d, %d, %s>: %d registers per lane, %d B of scratch" % (inst[0], inst[1], KM.OPTS[inst[2]], m["vgpr_count"],
                                                                                   m["private_segment_fixed_size"]))
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (inst, m)
        assert m["group_segment_fixed_size"] == 0, (inst, m)           # no LDS product row
        assert granule * CLAIMED_WAVES_PER_SIMD <= VGPRS_PER_SIMD_LANE, (inst, m)
    assert KM.lane_shape(1028) is None                                  # five chunks: ge_glove_set_arith refuses the dim


def test_cost_terms_are_the_exact_modes():
    """x > xmax weighs 1, pGloVe weighs x, GloVe takes libm's pow."""
    l, w = R.cost_terms(False, 0.3, 0.2)
    assert w == np.float32(1) and l == np.log(np.float64(np.float32(0.3)))
    l, w = R.cost_terms(True, 0.15, 0.2)
    x = np.float32(0.15)
    assert w == x and l == np.log(np.float64(np.float32(x / np.float32(np.float32(1) - x))))
    xs = (0.01 + 0.19 * np.random.default_rng(0).random(2000)).astype(np.float32)
    ws = np.array([R.cost_terms(False, x, 0.2)[1] for x in xs])
    assert np.array_equal(ws, np.power(xs.astype(np.float64) / 0.2, 0.75).astype(np.float32))


# Measured on the CPU (this test prints them): the largest relative gap of a per-epoch cost sum over the 5 epochs is
#   glove 1.264e-08 (epoch 3), pglove 7.450e-09 (epoch 3)
# so the bound is 8 x 1.264e-08 = 1.011e-07.  fp32 round-off through a few thousand updates leaves that much room for other inputs; the
# number comes from this comparison of model and oracle alone, never from device output.
LARGEST_GAP_SEEN = 1.264e-08
GAP_BOUND = 8 * LARGEST_GAP_SEEN


@pytest.mark.parametrize("method", ["glove", "pglove"])
def test_the_fp32_model_trains_what_the_oracle_trains(method):
    """5 epochs on synthetic_coo(300, 4000, seed=9), D = 50, P = 16, shuffle: device, AdaGrad: the model (fp32 arithmetic) and the
    oracle (Java's), each on its own tables from the same start, in the same stratified order.  The relative gap of every epoch's
    cost sum stays below GAP_BOUND = 8 x the largest gap measured (glove 1.264e-08, pglove 7.450e-09:
    1.011e-07)."""
    V, D, P, seed = 300, 50, 16, 5
    I, J, X, xmax = synth.synthetic_coo(V, 4000, seed=9)
    model = S.Model(I, J, P)
    g = O.Glove(V, D, I, J, X, xmax, cost=cost_kind(method), seed=seed)
    ref = {k: np.ascontiguousarray(v, np.float32) for k, v in g.state().items()}
    g.close()
    mine = {k: v.copy() for k, v in ref.items()}
    for it in range(5):
        want = 0.0
        for nz in model.jobs(seed, it, "device"):
            if len(nz):
                want += float(O.adagrad_job(D, I[nz], J[nz], X[nz], xmax, cost_kind(method), ref))
        got = R.epoch(model, seed, it, "device", "adagrad", D, I, J, X, xmax, mine, pglove=method == "pglove")
        gap = abs(got - want) / abs(want)
        print("%s epoch %d: oracle %.17g, fp32 model %.17g, relative gap %.3e" % (method, it, want, got, gap))
        assert gap <= GAP_BOUND, (method, it, got, want, gap)
