"""Calls in flight, on the host: the oracle's saved prefix (``prefix_cores``), the condition that lets a saved-P case tell
the two answers apart, and the checkers of tests/outstanding.py on fp32 numpy emulations -- a correct accumulation of two
calls passes, planted defects of the kinds test_gpu_outstanding.py looks for are rejected.  numpy and the oracle only: runs
where the HIP library is not built."""
import numpy as np
import pytest

import fp32_bound as fb
import outstanding as ost
from oracle import tt_oracle as orc

P, Q, R = ost.P, ost.Q, ost.RANKS


def _two_calls(seed, n1=6000, n2=700):
    rng = np.random.default_rng(seed)
    cores = fb.scaled_cores(rng, P, Q, R)
    return rng, cores, ost.call_inputs(rng, P, Q, n1), ost.call_inputs(rng, P, Q, n2)


def _refs(cores, call, route="scalar"):
    ids, offs, dy = call
    ref = orc.tt_dense_backward64(ids, offs, dy, cores, P, Q, R)
    return ref, [fb.grad_depth(route, Q, R, t, n) for t, (_, _, n) in enumerate(ref)]


def _g32(cores, call):
    ids, offs, dy = call
    return orc.tt_dense_backward(ids, offs, dy, cores, P, Q, R, acc_dtype=np.float32)


def _rejects(fn):
    with pytest.raises(AssertionError, match="over the fp32 bound"):
        fn()


# ---------------------------------------------------------------------------------------------------------------------
# the oracle's prefix_cores
# ---------------------------------------------------------------------------------------------------------------------
def test_no_prefix_cores_is_todays_oracle_bit_for_bit():
    rng, cores, (ids, offs, dy), _ = _two_calls(1, n1=3000)
    w = fb.sample_weights(rng, ids.shape[0])
    for kw in ({}, {"weights": w}, {"mode": "mean", "pad": int(ids[5])}):
        a = orc.tt_dense_backward64(ids, offs, dy, cores, P, Q, R, **kw)
        b = orc.tt_dense_backward64(ids, offs, dy, cores, P, Q, R, prefix_cores=None, **kw)
        c = orc.tt_dense_backward64(ids, offs, dy, cores, P, Q, R, prefix_cores=cores, **kw)   # the forward's cores = today's
        if "weights" in kw:
            for x in (b, c):
                assert np.array_equal(a[1][0], x[1][0]) and np.array_equal(a[1][1], x[1][1])
            a, b, c = a[0], b[0], c[0]
        for (v, m, n), (v2, m2, n2), (v3, m3, n3) in zip(a, b, c):
            assert np.array_equal(v, v2) and np.array_equal(m, m2) and np.array_equal(n, n2)
            assert np.array_equal(v, v3) and np.array_equal(m, m3) and np.array_equal(n, n3)
    # ... and what it was before the argument existed: the chain written out as _backward64 had it
    n = ids.shape[0]
    rowidx, f, _ = orc._id_factors(ids, offs, None, "sum", None)
    ii = orc.split_index(ids, P)
    v, c64 = orc._rows64(ii, cores, Q, R, False)
    dv = f[:, None] * dy.astype(np.float64)[rowidx]
    want = [np.zeros(x.shape) for x in cores]
    for t in (2, 1):
        dc = dv.reshape(n, v[t - 1].shape[1], Q[t] * R[t + 1])
        np.add.at(want[t], ii[t], np.matmul(v[t - 1].transpose(0, 2, 1), dc).reshape(n, -1))
        dv = np.matmul(dc, c64[t][ii[t]].reshape(n, R[t], Q[t] * R[t + 1]).transpose(0, 2, 1))
    np.add.at(want[0], ii[0], dv.reshape(n, -1))
    for t, (got, _, _) in enumerate(orc.tt_dense_backward64(ids, offs, dy, cores, P, Q, R)):
        assert np.array_equal(got, want[t]), f"dG{t}"


@pytest.mark.parametrize("shape", [([3, 4, 5], [2, 3, 2], [1, 3, 2, 1]), ([4, 6], [3, 2], [1, 5, 1])],
                         ids=["three_cores", "two_cores"])
def test_prefix_cores_agrees_with_an_einsum_written_out(shape):
    p, q, Rk = shape
    rng = np.random.default_rng(2)
    W = fb.scaled_cores(rng, p, q, Rk)        # the forward's cores
    Wn = ost.fresh_prefix(rng, W, p, q, Rk)   # the cores now (the last core unchanged)
    n = 57
    ids = rng.integers(0, int(np.prod(p)), size=n).astype(np.int64)
    offs = np.array([0, 5, 5, 6, 30, n], dtype=np.int64)
    dy = fb.scaled_dy(rng, offs.shape[0] - 1, int(np.prod(q)))
    rowidx = orc.rowidx_from_offsets(offs, n)
    dig = orc.split_index(ids, p)
    want = [np.zeros(x.shape) for x in W]
    mags = [np.zeros(x.shape) for x in W]
    for sel, dst in ((lambda x: np.asarray(x, dtype=np.float64), want), (lambda x: np.abs(np.asarray(x, dtype=np.float64)), mags)):
        if len(p) == 3:
            d3 = sel(dy)[rowidx].reshape(n, q[0], q[1], q[2])
            g0s, g1s = sel(W[0])[dig[0]].reshape(n, q[0], Rk[1]), sel(W[1])[dig[1]].reshape(n, Rk[1], q[1], Rk[2])
            g0n, g1n = sel(Wn[0])[dig[0]].reshape(n, q[0], Rk[1]), sel(Wn[1])[dig[1]].reshape(n, Rk[1], q[1], Rk[2])
            g2 = sel(Wn[2])[dig[2]].reshape(n, Rk[2], q[2])
            p_saved = np.einsum("nar,nrbs->nabs", g0s, g1s)                    # the forward's P
            np.add.at(dst[2], dig[2], np.einsum("nabs,nabc->nsc", p_saved, d3).reshape(n, -1))
            dp = np.einsum("nabc,nsc->nabs", d3, g2)                           # no prefix enters dP
            np.add.at(dst[1], dig[1], np.einsum("nar,nabs->nrbs", g0n, dp).reshape(n, -1))
            np.add.at(dst[0], dig[0], np.einsum("nabs,nrbs->nar", dp, g1n).reshape(n, -1))
        else:   # two cores: v[0] is the first core's row itself
            d2 = sel(dy)[rowidx].reshape(n, q[0], q[1])
            g0s = sel(W[0])[dig[0]].reshape(n, q[0], Rk[1])
            g1 = sel(Wn[1])[dig[1]].reshape(n, Rk[1], q[1])
            np.add.at(dst[1], dig[1], np.einsum("nar,nab->nrb", g0s, d2).reshape(n, -1))
            np.add.at(dst[0], dig[0], np.einsum("nab,nrb->nar", d2, g1).reshape(n, -1))
    got = orc.tt_dense_backward64(ids, offs, dy, Wn, p, q, Rk, prefix_cores=W)
    plain = orc.tt_dense_backward64(ids, offs, dy, Wn, p, q, Rk)
    u64 = 2.0 ** -53
    for t in range(len(p)):
        v, m, cnt = got[t]
        # two float64 evaluations of one sum of at most n q0 q1 R products of four factors: gamma64 of that depth, per element
        depth = n * int(np.prod(q)) * max(Rk) + 8
        assert np.all(np.abs(v - want[t]) <= 2 * depth * u64 * mags[t] + 1e-300), f"dG{t}"
        assert np.all(np.abs(m - mags[t]) <= 2 * depth * u64 * mags[t] + 1e-300), f"mag of dG{t}"
        assert np.array_equal(cnt, np.bincount(dig[t], minlength=p[t]))
    # only the last core's gradient sees the prefix (three cores; with two, dG1 is formed with v[0] = the saved row)
    for t in range(len(p) - 1):
        assert np.array_equal(got[t][0], plain[t][0]), f"dG{t} must not depend on the prefix"
    assert np.abs(got[-1][0] - plain[-1][0]).max() > 0


# ---------------------------------------------------------------------------------------------------------------------
# the separation condition of the saved-P cases
# ---------------------------------------------------------------------------------------------------------------------
def test_saved_and_current_prefix_are_apart_on_the_module_table():
    rng, cores, (ids, offs, dy), _ = _two_calls(3)
    now = ost.fresh_prefix(rng, cores, P, Q, R)
    saved, current = ost.saved_prefix_refs(ids, offs, dy, cores, now, P, Q, R)
    depth = fb.grad_depth("grouped", Q, R, 2, saved[2][2])
    s = ost.assert_separated(saved, current, depth, "module table")
    print(f"separation on p={P}: {s:.1%}")
    for t in (0, 1):   # and nothing else depends on it
        assert np.array_equal(saved[t][0], current[t][0])


@pytest.mark.parametrize("case", ost.SAVED_P_ROUTES, ids=[c[0] for c in ost.SAVED_P_ROUTES])
def test_saved_and_current_prefix_are_apart_on_every_route_shape(case):
    key, p, q, r, n_ids, _, _, _, rk, _ = case
    Rt, Rk = [1] + r + [1], [1] + (rk or r) + [1]
    rng = np.random.default_rng(len(key) + n_ids)
    cores = fb.scaled_cores(rng, p, q, Rt)
    ids, offs, dy = ost.call_inputs(rng, p, q, n_ids)
    now = ost.fresh_prefix(rng, cores, p, q, Rt)
    saved, current = ost.saved_prefix_refs(ids, offs, dy, cores, now, p, q, Rt)
    s = ost.assert_separated(saved, current, fb.grad_depth(ost.route_of(case), q, Rk, 2, saved[2][2]), key)
    print(f"separation on {key}: {s:.1%}")


# ---------------------------------------------------------------------------------------------------------------------
# the checkers: a correct accumulation passes, planted defects are rejected
# ---------------------------------------------------------------------------------------------------------------------
def test_a_correct_fp32_accumulation_of_two_calls_passes_with_one_more_rounding():
    _, cores, c1, c2 = _two_calls(4)
    (r1, d1), (r2, d2) = _refs(cores, c1), _refs(cores, c2)
    g1, g2 = _g32(cores, c1), _g32(cores, c2)
    both = [(a + b).astype(np.float32) for a, b in zip(g1, g2)]
    worst = ost.assert_summed(both, [r1, r2], [d1, d2], "two calls")
    ost.assert_summed([(b + a).astype(np.float32) for a, b in zip(g1, g2)], [r2, r1], [d2, d1], "two calls, other order")
    twice = [(a + a).astype(np.float32) for a in g1]   # retain_graph: the same backward added twice
    ost.assert_summed(twice, [r1, r1], [d1, d1], "one call twice")
    print(f"two calls: largest err/(u mag) {worst:.2f}")


def test_a_sum_that_drops_the_second_call_on_its_own_rows_is_rejected():
    _, cores, c1, c2 = _two_calls(5)
    (r1, d1), (r2, d2) = _refs(cores, c1), _refs(cores, c2)
    g1, g2 = _g32(cores, c1), _g32(cores, c2)
    bad = []
    only2 = 0
    for t in range(3):
        rows = (r1[t][2] == 0) & (r2[t][2] > 0)   # rows only the second call touches
        only2 += int(rows.sum())
        s = (g1[t] + g2[t]).astype(np.float32)
        s[rows] = g1[t][rows]
        bad.append(s)
    assert only2 > 0
    _rejects(lambda: ost.assert_summed(bad, [r1, r2], [d1, d2], "dropped"))
    # ... also when only ONE core's rows are dropped
    for t in range(3):
        if ((r1[t][2] == 0) & (r2[t][2] > 0)).any():
            one = [(a + b).astype(np.float32) for a, b in zip(g1, g2)]
            one[t] = bad[t]
            _rejects(lambda: ost.assert_summed(one, [r1, r2], [d1, d2], f"dropped in core {t}"))


def test_the_wrong_prefix_is_rejected_both_ways():
    rng, cores, (ids, offs, dy), _ = _two_calls(6)
    now = ost.fresh_prefix(rng, cores, P, Q, R)
    saved, current = ost.saved_prefix_refs(ids, offs, dy, cores, now, P, Q, R)
    depth = [fb.grad_depth("grouped", Q, R, t, saved[t][2]) for t in range(3)]

    def check(got, ref):
        for t, (v, m, _) in enumerate(ref):
            fb.assert_fp32_grade(got[t], v, m, depth[t], f"dG{t}", "core row")

    g_saved = [x[0].astype(np.float32) for x in saved]       # one rounding of the exact answer: a correct fp32 result
    g_current = [x[0].astype(np.float32) for x in current]
    check(g_saved, saved)
    check(g_current, current)
    _rejects(lambda: check(g_current, saved))    # P recomputed from the cores of the backward where the plan's is expected
    _rejects(lambda: check(g_saved, current))    # a stale P where no plan was handed over


def test_a_gradient_applied_twice_is_rejected_where_the_probe_expects_once():
    _, cores, c1, _ = _two_calls(7, n1=3000)
    r1, d1 = _refs(cores, c1)
    g1 = _g32(cores, c1)
    lr = 0.05
    once = orc.sgd_step(cores, g1, lr)
    twice = orc.sgd_step(once, g1, lr)
    st0 = [np.zeros_like(c) for c in cores]
    a_once, s_once = orc.adagrad_step(cores, st0, g1, lr, 1e-3)
    a_twice, s_twice = orc.adagrad_step(a_once, s_once, g1, lr, 1e-3)
    for t, (v, m, n) in enumerate(r1):
        delta = fb.gamma(d1[t]) * m
        fb.assert_sgd_grade(once[t], cores[t], v, delta, lr, f"SGD core {t}")
        _rejects(lambda: fb.assert_sgd_grade(twice[t], cores[t], v, delta, lr, f"SGD core {t}"))
        fb.assert_adagrad_grade(a_once[t], s_once[t], cores[t], st0[t], v, delta, lr, 1e-3, f"Adagrad core {t}")
        _rejects(lambda: fb.assert_adagrad_grade(a_twice[t], s_twice[t], cores[t], st0[t], v, delta, lr, 1e-3, f"Adagrad core {t}"))
