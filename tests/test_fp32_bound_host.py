"""The per-element fp32 bound of tests/fp32_bound.py on the host: correct fp32 evaluations pass it in several summation
orders, and small planted defects fail it -- among them some that the max-relative tolerances of the GPU tests accept.
numpy and the oracle only: runs where the HIP library is not built."""
import numpy as np
import pytest

import fp32_bound as fb
from oracle import tt_oracle as orc

P, Q, R = [23, 290, 310], [4, 5, 5], [1, 16, 16, 1]
D = int(np.prod(Q))


def _case(seed=0, n_ids=4000, cores="scaled"):
    rng = np.random.default_rng(seed)
    c = fb.scaled_cores(rng, P, Q, R) if cores == "scaled" else fb.uniform_cores(rng, P, Q, R)
    ids, offs = fb.skewed_bags(rng, P, n_ids)
    B = offs.shape[0] - 1
    return rng, c, ids, offs, fb.scaled_dy(rng, B, D)


def _lens(offs):
    return np.diff(offs)


def _bags32(rows, ids, offs, f=None, reverse=False):
    """fp32 bag sums of per-id fp32 rows, one id at a time (in position order or reversed)."""
    rowidx = orc.rowidx_from_offsets(offs, ids.shape[0])
    rows = rows if f is None else (rows * f[:, None]).astype(np.float32)
    order = np.arange(ids.shape[0])[::-1] if reverse else np.arange(ids.shape[0])
    out = np.zeros((offs.shape[0] - 1, D), dtype=np.float32)
    np.add.at(out, rowidx[order], rows[order])
    return out


def _rows_right_first(ids, cores):
    """A . (B . C) in fp32."""
    i0, i1, i2 = orc.split_index(ids, P)
    n = ids.shape[0]
    bc = np.matmul(cores[1][i1].reshape(n, R[1] * Q[1], R[2]), cores[2][i2].reshape(n, R[2], Q[2]))  # [n, r1 q1, q2]
    bc = bc.reshape(n, R[1], Q[1] * Q[2])
    return np.matmul(cores[0][i0].reshape(n, Q[0], R[1]), bc).reshape(n, D)


def _fwd_check(got, want, mag, offs, route="scalar", reduce=False):
    return fb.assert_fp32_grade(got, want, mag, fb.bag_depth(route, R, _lens(offs), reduce=reduce), "forward", rows="bag")


def _grad_check(got, ref, scaled=False):
    worst = 0.0
    for t, (g, (v, m, n)) in enumerate(zip(got, ref)):
        worst = max(worst, fb.assert_fp32_grade(g, v, m, fb.grad_depth("scalar", Q, R, t, n, scaled=scaled),
                                                f"dG{t}", rows="core row"))
    return worst


def _old_forward_accepts(got, want):
    np.testing.assert_allclose(got, want, atol=1e-4 * max(1.0, float(np.abs(want).max())), rtol=1e-5)


def _old_grads_accept(got, want, rel=1e-4):   # test_gpu_parity.py::assert_grads_close, restated
    for a, b in zip(got, want):
        scale = max(float(np.abs(b).max()), 1e-6)
        assert float(np.abs(a - b).max()) <= rel * scale + 1e-6


def _bf16(x):
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    b = ((b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return b.view(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# correct fp32 passes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cores", ["scaled", "uniform"])
def test_correct_fp32_forward_passes_in_three_orders(cores):
    _, c, ids, offs, _ = _case(1, cores=cores)
    want, mag = orc.tt_forward64(ids, offs, c, P, Q, R)
    left = orc.tt_rows(ids, c, P, Q, R)
    worst = [_fwd_check(_bags32(left, ids, offs), want, mag, offs),                      # (A.B).C
             _fwd_check(_bags32(_rows_right_first(ids, c), ids, offs), want, mag, offs),  # A.(B.C)
             _fwd_check(_bags32(left, ids, offs, reverse=True), want, mag, offs),       # bags summed backwards
             _fwd_check(orc.tt_forward(ids, offs, c, P, Q, R), want, mag, offs)]
    # the per-bag MFMA kernels' depth (one accumulator over the bag) is larger still: these pass it too
    _fwd_check(_bags32(left, ids, offs), want, mag, offs, route="per_bag")
    print(f"forward ({cores}): largest err/(u mag) {max(worst):.2f}, row depth {fb.row_depth('scalar', R)}, "
          f"bag depths up to {int(fb.bag_depth('scalar', R, _lens(offs)).max())}")


@pytest.mark.parametrize("mode", ["weighted", "mean_pad"])
def test_correct_fp32_weighted_and_mean_bags_pass(mode):
    rng, c, ids, offs, dy = _case(2)
    w = fb.sample_weights(rng, ids.shape[0]) if mode == "weighted" else None
    pad = int(ids[5]) if mode == "mean_pad" else None
    want, mag = orc.tt_forward64(ids, offs, c, P, Q, R, weights=w, mode="sum" if w is not None else "mean", pad=pad)
    rowidx, f, keep = orc._id_factors(ids, offs, w, "sum" if w is not None else "mean", pad)
    if w is None:   # mean: 1 / kept in fp32, then the product (ttemb_bag.hip:192)
        kept = np.bincount(rowidx[keep], minlength=offs.shape[0] - 1)
        f = np.where(keep, np.float32(1.0) / np.maximum(kept, 1).astype(np.float32)[rowidx], 0).astype(np.float32)
    rows = orc.tt_rows(ids, c, P, Q, R)
    worst = max(_fwd_check(_bags32(rows, ids, offs, f.astype(np.float32), reverse=rev), want, mag, offs, reduce=True)
                for rev in (False, True))
    print(f"forward ({mode}): largest err/(u mag) {worst:.2f}")


def test_correct_fp32_gradients_pass_summed_one_id_at_a_time():
    _, c, ids, offs, dy = _case(3)
    ref = orc.tt_dense_backward64(ids, offs, dy, c, P, Q, R)
    fwd = orc.tt_dense_backward(ids, offs, dy, c, P, Q, R, acc_dtype=np.float32)
    # ids reversed (bags reversed with them): the same gradient summed in the other order
    n = ids.shape[0]
    roffs = (n - offs[::-1]).astype(np.int64)
    rev = orc.tt_dense_backward(ids[::-1].copy(), roffs, dy[::-1].copy(), c, P, Q, R, acc_dtype=np.float32)
    worst = max(_grad_check(fwd, ref), _grad_check(rev, ref),
                _grad_check(orc.tt_dense_backward(ids, offs, dy, c, P, Q, R), ref))
    depths = [int(fb.grad_depth("scalar", Q, R, 2, x[2]).max()) for x in ref[2:]]
    print(f"gradients: largest err/(u mag) {worst:.2f}, dG2 depths up to {depths[0]}")


def test_correct_fp32_weight_gradient_and_steps_pass():
    rng, c, ids, offs, dy = _case(4)
    w = fb.sample_weights(rng, ids.shape[0])
    ref, (wv, wm) = orc.tt_dense_backward64(ids, offs, dy, c, P, Q, R, weights=w)
    rows = orc.tt_rows(ids, c, P, Q, R)
    rowidx = orc.rowidx_from_offsets(offs, ids.shape[0])
    wg = np.einsum("nd,nd->n", dy[rowidx], rows, dtype=np.float32)
    fb.assert_fp32_grade(wg, wv, wm, fb.wgrad_depth("scalar", Q, R), "w.grad", rows="id")
    # the fused steps from an fp32 gradient
    g32 = orc.tt_dense_backward(ids, offs, dy, c, P, Q, R, acc_dtype=np.float32)
    lr, eps = 0.05, 1e-3
    st0 = [(rng.random(x.shape) * 1e-6).astype(np.float32) for x in c]
    new_c, new_s = orc.adagrad_step(c, st0, g32, lr, eps)
    for t, (v, m, n) in enumerate(orc.tt_dense_backward64(ids, offs, dy, c, P, Q, R)):
        delta = fb.gamma(fb.grad_depth("scalar", Q, R, t, n)) * m
        fb.assert_sgd_grade(orc.sgd_step(c, g32, lr)[t], c[t], v, delta, lr, f"sgd core {t}")
        fb.assert_adagrad_grade(new_c[t], new_s[t], c[t], st0[t], v, delta, lr, eps, f"adagrad core {t}")
        fb.assert_untouched(new_c[t], c[t], n, f"adagrad core {t}")


# ---------------------------------------------------------------------------------------------------------------------
# planted defects are rejected
# ---------------------------------------------------------------------------------------------------------------------
def _rejects(fn):
    with pytest.raises(AssertionError, match="over the fp32 bound"):
        fn()


def test_bf16_cores_are_rejected_everywhere_and_on_the_small_rows_only():
    _, c, ids, offs, _ = _case(5)
    want, mag = orc.tt_forward64(ids, offs, c, P, Q, R)
    _rejects(lambda: _fwd_check(orc.tt_forward(ids, offs, [_bf16(x) for x in c], P, Q, R), want, mag, offs))
    # bf16 rows for the ids whose row is small (product of the three row scales under 1e-4 of the largest)
    rows = orc.tt_rows(ids, c, P, Q, R)
    rows_bf = orc.tt_rows(ids, [_bf16(x) for x in c], P, Q, R)
    size = np.abs(orc.tt_forward64(ids, np.arange(ids.shape[0] + 1), c, P, Q, R)[1]).max(axis=1)
    small = size < 1e-4 * size.max()
    assert 0.1 < small.mean() < 0.95
    got = _bags32(np.where(small[:, None], rows_bf, rows), ids, offs)
    _rejects(lambda: _fwd_check(got, want, mag, offs))
    _old_forward_accepts(got, want)   # the gap: today's forward tolerance does not see it


def test_bf16_forward_on_the_uniform_initialiser_is_rejected():
    _, c, ids, _, _ = _case(6, cores="uniform")
    offs = np.arange(ids.shape[0] + 1)   # rows: entries of about 0.02
    want, mag = orc.tt_forward64(ids, offs, c, P, Q, R)
    got = orc.tt_forward(ids, offs, [_bf16(x) for x in c], P, Q, R)
    _rejects(lambda: _fwd_check(got, want, mag, offs))
    np.testing.assert_allclose(got, want, atol=1e-4, rtol=1e-5)   # the gap: atol 1e-4 of test_gpu_weighted / _padding


def test_a_digit_decoded_off_by_one_is_rejected():
    _, c, ids, offs, _ = _case(7)
    want, mag = orc.tt_forward64(ids, offs, c, P, Q, R)
    b = int(np.nonzero(_lens(offs) == 2)[0][3])
    bad = ids.copy()
    k = int(offs[b])
    bad[k] = bad[k] + 1 if bad[k] % P[2] != P[2] - 1 else bad[k] - 1
    got = orc.tt_forward(bad, offs, c, P, Q, R)
    assert np.abs(got - orc.tt_forward(ids, offs, c, P, Q, R)).max() > 0
    _rejects(lambda: _fwd_check(got, want, mag, offs))


def test_a_dropped_contribution_to_a_cold_row_is_rejected():
    _, c, ids, offs, dy = _case(8)
    ref = orc.tt_dense_backward64(ids, offs, dy, c, P, Q, R)
    good = orc.tt_dense_backward(ids, offs, dy, c, P, Q, R, acc_dtype=np.float32)
    digits = orc.split_index(ids, P)
    rowidx = orc.rowidx_from_offsets(offs, ids.shape[0])
    t = 1
    cold = np.nonzero((ref[t][2] >= 1) & (ref[t][2] <= 2))[0]
    assert cold.size
    # the id on a cold row of core 1 whose contribution is smallest: drop it
    cand = np.nonzero(np.isin(digits[t], cold))[0]
    contrib = [np.abs(orc.tt_dense_backward(ids[[k]], np.array([0, 1]), dy[rowidx[[k]]], c, P, Q, R)[t]).max() for k in cand]
    k = int(cand[int(np.argmin(contrib))])
    keep = np.ones(ids.shape[0], dtype=bool)
    keep[k] = False
    lens = np.bincount(rowidx[keep], minlength=offs.shape[0] - 1)
    offs2 = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    dropped = orc.tt_dense_backward(ids[keep], offs2, dy, c, P, Q, R, acc_dtype=np.float32)
    _rejects(lambda: _grad_check(dropped, ref))
    _old_grads_accept(dropped, [x[0] for x in ref])   # the gap: 1e-4 of the largest gradient does not see it
    _grad_check(good, ref)


def test_a_mean_that_counts_the_pads_is_rejected():
    _, c, ids, offs, _ = _case(9)
    pad = int(ids[7])
    want, mag = orc.tt_forward64(ids, offs, c, P, Q, R, mode="mean", pad=pad)
    rowidx = orc.rowidx_from_offsets(offs, ids.shape[0])
    lens = np.maximum(_lens(offs), 1).astype(np.float32)
    f = np.where(ids != pad, np.float32(1) / lens[rowidx], 0).astype(np.float32)
    got = _bags32(orc.tt_rows(ids, c, P, Q, R), ids, offs, f)
    _rejects(lambda: _fwd_check(got, want, mag, offs, reduce=True))


def test_a_weight_applied_twice_is_rejected():
    rng, c, ids, offs, _ = _case(10)
    w = fb.sample_weights(rng, ids.shape[0])
    want, mag = orc.tt_forward64(ids, offs, c, P, Q, R, weights=w)
    got = _bags32(orc.tt_rows(ids, c, P, Q, R), ids, offs, (w * w).astype(np.float32))
    _rejects(lambda: _fwd_check(got, want, mag, offs, reduce=True))


def test_adagrad_without_the_new_square_is_rejected():
    rng, c, ids, offs, dy = _case(11)
    ref = orc.tt_dense_backward64(ids, offs, dy, c, P, Q, R)
    g32 = orc.tt_dense_backward(ids, offs, dy, c, P, Q, R, acc_dtype=np.float32)
    lr, eps = 0.05, 1e-3
    st0 = [(rng.random(x.shape) * 1e-6).astype(np.float32) for x in c]
    t = 2
    v, m, n = ref[t]
    delta = fb.gamma(fb.grad_depth("scalar", Q, R, t, n)) * m
    s_new = (st0[t] + g32[t] * g32[t]).astype(np.float32)
    w_bad = (c[t] - np.float32(lr) * g32[t] / (np.sqrt(st0[t]) + np.float32(eps))).astype(np.float32)
    _rejects(lambda: fb.assert_adagrad_grade(w_bad, s_new, c[t], st0[t], v, delta, lr, eps, "adagrad"))
