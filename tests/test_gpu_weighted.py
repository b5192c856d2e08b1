"""Weighted (mode="sum" with per_sample_weights) and mean bags on the GPU, against torch.nn.functional.embedding_bag over
the module's full_weight() (autograd through the cores for their gradients, through the weights for w.grad).  Tolerances
as in test_gpu_parity.py: forward atol 1e-4 (+ rtol 1e-5), gradients 1e-4 of their largest magnitude, fused steps 1e-5."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (name, p, q, inner ranks, nnz, wanted route of the rows lookup without its route flags, prefix-in-chain flag or None)
CASES = [("grouped", [23, 29, 31], [4, 5, 5], [16, 16], 8192, 3, False),
         ("prefix_in_chain", [60, 70, 70], [4, 5, 5], [16, 16], 8192, 3, True),
         ("wide", [23, 29, 31], [4, 4, 8], [64, 64], 8192, 4, None),
         ("padded12", [23, 29, 31], [4, 5, 5], [12, 12], 8192, 3 | 32, None),
         ("per_bag_rt", [23, 29, 31], [6, 4, 4], [16, 16], 1000, 2, None),
         ("two_core", [90, 110], [8, 8], [16], 2000, 2 | 16, None),
         ("four_core", [7, 6, 5, 6], [2, 4, 4, 4], [16, 16, 16], 1000, 1 | 16, None),
         ("scalar", [23, 29, 31], [32, 2, 2], [16, 16], 500, 0, None)]
SMALL = ([23, 29, 31], [4, 5, 5], [16, 16])


@pytest.fixture(scope="module")
def nat():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import ttemb_native
    yield ttemb_native
    ttemb_native.set_exact_grid(0)
    ttemb_native.set_piece_limits(0, 0)


@pytest.fixture(scope="module")
def ops(nat):
    from FBTT import tt_embeddings_ops
    return tt_embeddings_ops


def _emb(ops, p, q, r, mode="sum", **kw):
    kw.setdefault("sparse", False)
    kw.setdefault("use_cache", False)
    emb = ops.TTEmbeddingBag(int(np.prod(p)), int(np.prod(q)), r, p, q, weight_dist="uniform", mode=mode, **kw)
    return emb


def _inputs(rows, nnz, seed, mean=4, long_bag=0):
    """Ragged bags with empty ones, repeated ids, weights with zeros and negative values (and one bag of `long_bag` ids
    between short ones)."""
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, rows, size=nnz)
    ids[::5] = ids[0]   # one id many times over, with different weights
    lens = list(rng.integers(0, 2 * mean + 1, size=2 * (nnz // mean) + 8))
    lens[::7] = [0] * len(lens[::7])
    if long_bag:
        lens = lens[:3] + [long_bag] + lens[3:]
    offs = np.concatenate([[0], np.cumsum(lens)])
    offs = offs[offs < nnz]
    offs = np.concatenate([offs, [nnz, nnz]]).astype(np.int64)   # (a trailing empty bag)
    w = rng.standard_normal(nnz).astype(np.float32)
    w[::11] = 0.0
    return torch.tensor(ids).cuda(), torch.tensor(offs).cuda(), torch.tensor(w).cuda()


def _reference(ops, emb, idx, offs, mode, w, dy, absolute=False):
    """``absolute``: the same sums over the absolute values of cores, weights and dy -- per gradient entry the sum of the
    magnitudes of its terms, which bounds the rounding error of any fp32 summation order of those terms."""
    mag = (lambda t: t.abs()) if absolute else (lambda t: t)
    cores = [mag(c.detach()).clone().requires_grad_(True) for c in emb.tt_cores]
    full = ops.tt_matrix_to_full(emb.tt_p_shapes, emb.tt_q_shapes, emb.tt_ranks, cores, [1, 0, 2, 3])
    wr = None if w is None else mag(w.detach()).clone().requires_grad_(True)
    out = F.embedding_bag(idx, full, offs, mode=mode, per_sample_weights=wr, include_last_offset=True)
    out.backward(mag(dy))
    return out.detach(), [c.grad for c in cores], (None if wr is None else wr.grad)


def _close_grad(got, want):
    torch.testing.assert_close(got, want, rtol=0, atol=1e-4 * max(float(want.abs().max()), 1e-6))


def _close_step(got, want, lr_g):
    torch.testing.assert_close(got, want, rtol=0, atol=1e-5 + 1e-4 * float(lr_g.abs().max()))


def _dy(B, D, seed):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(B, D, generator=g) - 0.5) * 0.2).cuda()


@pytest.mark.parametrize("mode", ["sum", "mean"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_forward_and_gradients_on_every_route(nat, ops, case, mode):
    name, p, q, r, nnz, want_fam, prefix = case
    emb = _emb(ops, p, q, r, mode)
    idx, offs, w = _inputs(int(np.prod(p)), nnz, seed=len(name))
    B, D = offs.numel() - 1, emb.embedding_dim
    fam = nat.kernel_family(emb._shape, nnz, nnz if mode == "sum" else B, True)
    assert fam & ~nat.FAMILY_ROUTE_FLAGS == want_fam, (name, fam)
    if prefix is not None:
        assert bool(fam & nat.FAMILY_PREFIX_IN_CHAIN) == prefix, (name, fam)
    wt = w.clone().requires_grad_(True) if mode == "sum" else None
    out = emb(idx, offs, per_sample_weights=wt)
    dy = _dy(B, D, 3)
    out.backward(dy)
    want, grads, wgrad = _reference(ops, emb, idx, offs, mode, w if mode == "sum" else None, dy)
    torch.testing.assert_close(out.detach(), want, rtol=1e-5, atol=1e-4)
    for c, g in zip(emb.tt_cores, grads):
        _close_grad(c.grad, g)
    if mode == "sum":
        _close_grad(wt.grad, wgrad)


@pytest.mark.parametrize("mode", ["sum", "mean"])
def test_long_bag_beside_short_ones(nat, ops, mode):
    p, q, r = SMALL
    emb = _emb(ops, p, q, r, mode)
    idx, offs, w = _inputs(int(np.prod(p)), 230000, seed=5, long_bag=200000)
    assert int((offs[1:] - offs[:-1]).max()) >= 200000
    wt = w.clone().requires_grad_(True) if mode == "sum" else None
    out = emb(idx, offs, per_sample_weights=wt)
    dy = _dy(offs.numel() - 1, emb.embedding_dim, 4)
    out.backward(dy)
    want, grads, wgrad = _reference(ops, emb, idx, offs, mode, w if mode == "sum" else None, dy)
    torch.testing.assert_close(out.detach(), want, rtol=1e-5, atol=1e-4 * max(1.0, float(want.abs().max())))
    # A core gradient entry here is a sum of ~10^5 fp32 terms (one id occurs 46 000 times) whose magnitudes add up to ~100x
    # the largest entry, summed in an order of its own on each side (the default backward's order is not fixed run to run).
    # Its error is bounded by the sum of the terms' magnitudes, not by the entry: 1e-4 of the largest such sum.  (A wrong
    # division by the bag length would be off by a factor of up to 200 000, far outside this.)
    _, mags, _ = _reference(ops, emb, idx, offs, mode, w if mode == "sum" else None, dy, absolute=True)
    for c, g, m in zip(emb.tt_cores, grads, mags):
        torch.testing.assert_close(c.grad, g, rtol=0, atol=1e-4 * float(m.max()))
    if mode == "sum":
        _close_grad(wt.grad, wgrad)


@pytest.mark.parametrize("mode", ["sum", "mean"])
def test_no_ids_and_empty_bags(nat, ops, mode):
    p, q, r = SMALL
    emb = _emb(ops, p, q, r, mode)
    idx = torch.empty(0, dtype=torch.int64, device="cuda")
    offs = torch.zeros(6, dtype=torch.int64, device="cuda")
    wt = torch.empty(0, device="cuda", requires_grad=True) if mode == "sum" else None
    out = emb(idx, offs, per_sample_weights=wt)
    assert tuple(out.shape) == (5, emb.embedding_dim) and not bool(out.any())
    out.backward(torch.ones_like(out))
    for c in emb.tt_cores:
        assert not bool(c.grad.any())
    empty = emb(idx, torch.zeros(1, dtype=torch.int64, device="cuda"),
                per_sample_weights=torch.empty(0, device="cuda") if mode == "sum" else None)
    assert tuple(empty.shape) == (0, emb.embedding_dim)


def test_argument_checks(nat, ops):
    p, q, r = SMALL
    idx, offs, w = _inputs(int(np.prod(p)), 100, seed=1)
    mean = _emb(ops, p, q, r, "mean")
    with pytest.raises(ValueError):
        mean(idx, offs, per_sample_weights=w)
    emb = _emb(ops, p, q, r)
    for bad in (w[:-1], w.double(), w.cpu(), w.view(10, 10)):
        with pytest.raises(ValueError):
            emb(idx, offs, per_sample_weights=bad)
    with pytest.raises(ValueError):
        _emb(ops, p, q, r, "max")


def test_weights_of_one_on_bags_of_one_change_no_bit(nat, ops):
    p, q, r = [60, 70, 70], [4, 5, 5], [16, 16]
    emb = _emb(ops, p, q, r, sparse=True)
    idx = torch.randint(0, int(np.prod(p)), (8192,), device="cuda")
    ar = torch.arange(8193, device="cuda")
    with torch.no_grad():
        plain = emb(idx, ar)
        weighted = emb(idx, ar, per_sample_weights=torch.ones(8192, device="cuda"))
    assert torch.equal(plain, weighted)


@pytest.mark.parametrize("mode", ["sum", "mean"])
@pytest.mark.parametrize("optimizer", ["sgd", "adagrad"])
def test_fused_steps_match_the_dense_gradient(nat, ops, mode, optimizer):
    p, q, r = SMALL
    lr, eps = 0.05, 1e-3
    opt = ops.OptimType.SGD if optimizer == "sgd" else ops.OptimType.EXACT_ADAGRAD
    emb = _emb(ops, p, q, r, mode, sparse=True, optimizer=opt, learning_rate=lr, eps=eps)
    idx, offs, w = _inputs(int(np.prod(p)), 20000, seed=9)
    start = [c.detach().clone() for c in emb.tt_cores]
    dy = _dy(offs.numel() - 1, emb.embedding_dim, 6)
    _, grads, _ = _reference(ops, emb, idx, offs, mode, w if mode == "sum" else None, dy)
    emb(idx, offs, per_sample_weights=w if mode == "sum" else None).backward(dy)
    for c, c0, g in zip(emb.tt_cores, start, grads):
        if optimizer == "sgd":
            _close_step(c.detach(), c0 - lr * g, lr * g)
        else:
            big = g.abs() > 1e-3 * float(g.abs().max())
            torch.testing.assert_close(c.detach()[big], (c0 - lr * g / (g.abs() + eps))[big], rtol=0, atol=1e-5)
    if optimizer == "adagrad":
        for st, g in zip(emb.optimizer_state, grads):
            torch.testing.assert_close(st, g * g, rtol=2e-4, atol=1e-4 * float((g * g).max()))


def _exact_run(nat, ops, mode, grid, garbage):
    p, q, r = SMALL
    nat.set_exact_grid(grid)
    try:
        torch.manual_seed(0)
        emb = _emb(ops, p, q, r, mode, sparse=True, optimizer=ops.OptimType.EXACT_ADAGRAD, learning_rate=0.05,
                   deterministic=True)
        idx, offs, w = _inputs(int(np.prod(p)), 30000, seed=2, long_bag=3000)
        with torch.no_grad():   # (the workspace exists at its full size) ...
            emb(idx, offs, per_sample_weights=w if mode == "sum" else None)
        if garbage:   # ... and holds garbage
            emb._ws.buf.copy_(torch.randint(0, 256, emb._ws.buf.shape, dtype=torch.uint8, device="cuda"))
        wt = w.clone().requires_grad_(True) if mode == "sum" else None
        out = emb(idx, offs, per_sample_weights=wt)
        out.backward(_dy(offs.numel() - 1, emb.embedding_dim, 8))
        torch.cuda.synchronize()
        return ([out.detach()] + ([wt.grad] if wt is not None else []) + [c.detach().clone() for c in emb.tt_cores]
                + [s.clone() for s in emb.optimizer_state])
    finally:
        nat.set_exact_grid(0)


@pytest.mark.parametrize("mode", ["sum", "mean"])
def test_exact_mode_is_bit_reproducible(nat, ops, mode):
    a = _exact_run(nat, ops, mode, 0, False)
    for grid, garbage in ((0, True), (1, True), (3, False)):
        b = _exact_run(nat, ops, mode, grid, garbage)
        for x, y in zip(a, b):
            assert torch.equal(x, y), (grid, garbage)


@pytest.mark.parametrize("mode", ["sum", "mean"])
def test_no_host_synchronisation(nat, ops, mode):
    p, q, r = SMALL
    emb = _emb(ops, p, q, r, mode, sparse=True)
    idx, offs, w = _inputs(int(np.prod(p)), 20000, seed=4)
    wt = w.clone().requires_grad_(True) if mode == "sum" else None
    dy = _dy(offs.numel() - 1, emb.embedding_dim, 1)
    emb(idx, offs, per_sample_weights=wt).backward(dy)   # (first call: workspace and scratch exist)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        emb(idx, offs, per_sample_weights=wt).backward(dy)
    finally:
        torch.cuda.set_sync_debug_mode("default")


@pytest.mark.parametrize("mode", ["sum", "mean"])
def test_live_row_cache(nat, ops, mode):
    p, q, r = SMALL
    n = int(np.prod(p))
    emb = _emb(ops, p, q, r, mode, use_cache=True, cache_size=300, hashtbl_size=n)
    idx, offs, w = _inputs(n, 6000, seed=12)
    with torch.no_grad():
        emb(idx, offs, per_sample_weights=w if mode == "sum" else None)   # warm-up statistics
    emb.cache_populate()
    assert not emb.warmup
    wt = w.clone().requires_grad_(True) if mode == "sum" else None
    out = emb(idx, offs, per_sample_weights=wt)
    dy = _dy(offs.numel() - 1, emb.embedding_dim, 2)
    out.backward(dy)
    # the cached rows equal the TT rows right after cache_populate(): the full table is the reference
    want, grads, wgrad = _reference(ops, emb, idx, offs, mode, w if mode == "sum" else None, dy)
    torch.testing.assert_close(out.detach(), want, rtol=1e-5, atol=1e-4)
    if mode == "sum":
        _close_grad(wt.grad, wgrad)
    assert emb.cache_weight.grad is not None and bool(emb.cache_weight.grad.any())


@pytest.mark.parametrize("mode", ["sum", "mean"])
def test_several_tables(nat, ops, mode):
    p, q, r = SMALL
    Tn, B = 3, 700
    emb = ops.TableBatchedTTEmbeddingBag(Tn, int(np.prod(p)), 100, r, p, q, sparse=False, use_cache=False,
                                         weight_dist="uniform", mode=mode)
    g = np.random.default_rng(3)
    lens = g.integers(0, 9, size=Tn * B)
    lens[::13] = 0
    offs = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int64).cuda()
    nnz = int(offs[-1])
    idx = torch.tensor(g.integers(0, int(np.prod(p)), size=nnz)).cuda()
    w = torch.tensor(g.standard_normal(nnz).astype(np.float32)).cuda().requires_grad_(mode == "sum")
    out = emb(idx, offs, per_sample_weights=w if mode == "sum" else None)
    assert tuple(out.shape) == (Tn, B, 100)
    dy = (torch.rand(Tn, B, 100, device="cuda") - 0.5) * 0.2
    out.backward(dy)
    bounds = offs[::B].tolist()
    for k in range(Tn):
        cores = [c.detach()[k:k + 1].clone().requires_grad_(True) for c in emb.tt_cores]
        full = ops.tt_matrix_to_full(p, q, emb.tt_ranks, cores, [1, 0, 2, 3])
        lo, hi = bounds[k], bounds[k + 1]
        wk = w.detach()[lo:hi] if mode == "sum" else None
        o = F.embedding_bag(idx[lo:hi], full, offs[k * B:(k + 1) * B + 1] - lo, mode=mode, per_sample_weights=wk,
                            include_last_offset=True)
        torch.testing.assert_close(out[k].detach(), o.detach(), rtol=1e-5, atol=1e-4)
        o.backward(dy[k])
        for c, cr in zip(emb.tt_cores, cores):
            _close_grad(c.grad[k:k + 1], cr.grad)


@pytest.mark.parametrize("mode", ["sum", "mean"])
def test_inference_and_pieces(nat, ops, mode):
    p, q, r = SMALL
    emb = _emb(ops, p, q, r, mode, sparse=True)
    idx, offs, w = _inputs(int(np.prod(p)), 20000, seed=21)
    want, _, _ = _reference(ops, emb, idx, offs, mode, w if mode == "sum" else None,
                            torch.zeros(offs.numel() - 1, emb.embedding_dim, device="cuda"))
    with torch.no_grad():
        out = emb(idx, offs, per_sample_weights=w if mode == "sum" else None)
    torch.testing.assert_close(out, want, rtol=1e-5, atol=1e-4)
    nat.set_piece_limits(rows=3000, ids=5000)
    try:
        emb2 = _emb(ops, p, q, r, mode, sparse=False)
        emb2.load_state_dict(emb.state_dict())
        wt = w.clone().requires_grad_(True) if mode == "sum" else None
        out = emb2(idx, offs, per_sample_weights=wt)
        dy = _dy(offs.numel() - 1, emb.embedding_dim, 7)
        out.backward(dy)
        torch.cuda.synchronize()
    finally:
        nat.set_piece_limits(0, 0)
    want, grads, wgrad = _reference(ops, emb2, idx, offs, mode, w if mode == "sum" else None, dy)
    torch.testing.assert_close(out.detach(), want, rtol=1e-5, atol=1e-4)
    for c, g in zip(emb2.tt_cores, grads):
        _close_grad(c.grad, g)
    if mode == "sum":
        _close_grad(wt.grad, wgrad)


def test_data_parallel_step_with_weights(nat, ops):
    from ttemb_dist import TTDataParallel
    p, q, r = SMALL
    lr = 0.2
    emb = _emb(ops, p, q, r, learning_rate=lr)
    dp = TTDataParallel(emb)
    idx, offs, w = _inputs(int(np.prod(p)), 20000, seed=31)
    start = [c.detach().clone() for c in emb.tt_cores]
    dy = _dy(offs.numel() - 1, emb.embedding_dim, 9)
    _, grads, _ = _reference(ops, emb, idx, offs, "sum", w, dy)
    emb(idx, offs, per_sample_weights=w).backward(dy)
    dp.step()
    torch.cuda.synchronize()
    for c, c0, g in zip(emb.tt_cores, start, grads):
        _close_step(c.detach(), c0 - lr * g, lr * g)
