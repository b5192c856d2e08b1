"""padding_idx and fixed-length 2-D bags on the GPU, against torch.nn.functional.embedding_bag(..., padding_idx=p) over the
module's full_weight() (autograd through the cores for their gradients, through the weights for w.grad).  Tolerances as in
test_gpu_weighted.py: forward atol 1e-4 (+ rtol 1e-5), gradients 1e-4 of their largest magnitude, fused steps 1e-5."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# the CASES of test_gpu_weighted.py: (name, p, q, inner ranks, nnz)
CASES = [("grouped", [23, 29, 31], [4, 5, 5], [16, 16], 8192),
         ("prefix_in_chain", [60, 70, 70], [4, 5, 5], [16, 16], 8192),
         ("wide", [23, 29, 31], [4, 4, 8], [64, 64], 8192),
         ("padded12", [23, 29, 31], [4, 5, 5], [12, 12], 8192),
         ("per_bag_rt", [23, 29, 31], [6, 4, 4], [16, 16], 1000),
         ("two_core", [90, 110], [8, 8], [16], 2000),
         ("four_core", [7, 6, 5, 6], [2, 4, 4, 4], [16, 16, 16], 1000),
         ("scalar", [23, 29, 31], [32, 2, 2], [16, 16], 500)]
SMALL = ([23, 29, 31], [4, 5, 5], [16, 16])


@pytest.fixture(scope="module")
def nat():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import ttemb_native
    yield ttemb_native
    ttemb_native.set_exact_grid(0)


@pytest.fixture(scope="module")
def ops(nat):
    from FBTT import tt_embeddings_ops
    return tt_embeddings_ops


def _emb(ops, p, q, r, mode="sum", **kw):
    kw.setdefault("sparse", False)
    kw.setdefault("use_cache", False)
    return ops.TTEmbeddingBag(int(np.prod(p)), int(np.prod(q)), r, p, q, weight_dist="uniform", mode=mode, **kw)


def _pad_of(p):
    """A pad id in the middle of the table, and the stride of its G0 row."""
    L0 = int(np.prod(p[1:]))
    return (p[0] // 2) * L0 + 7 % L0, L0


def _inputs(p, nnz, seed, share, mean=4):
    """Ragged bags with empty ones and repeated ids; no id but the pad in the pad's G0 row.  With ``share`` > 0: about that
    share of pad ids, pads at the first and last place of every third bag, bags made only of pad ids (every tenth, and every
    other bag of one id)."""
    rows = int(np.prod(p))
    pad, L0 = _pad_of(p)
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, rows, size=nnz)
    ids[::5] = ids[0]
    same = ids // L0 == pad // L0
    ids[same] = (ids[same] + L0) % rows
    lens = list(rng.integers(0, 2 * mean + 1, size=2 * (nnz // mean) + 8))
    lens[::7] = [0] * len(lens[::7])
    offs = np.concatenate([[0], np.cumsum(lens)])
    offs = offs[offs < nnz]
    offs = np.concatenate([offs, [nnz, nnz]]).astype(np.int64)
    if share > 0:
        ids[rng.random(nnz) < share] = pad
        starts, ends = offs[:-1], offs[1:]
        for b in range(0, len(starts), 3):
            if ends[b] > starts[b]:
                ids[starts[b]] = pad
                ids[ends[b] - 1] = pad
        for b in range(1, len(starts), 10):
            ids[starts[b]:ends[b]] = pad
        ones = np.nonzero(ends - starts == 1)[0]
        ids[starts[ones[::2]]] = pad
    w = rng.standard_normal(nnz).astype(np.float32)
    return torch.tensor(ids).cuda(), torch.tensor(offs).cuda(), torch.tensor(w).cuda(), pad


def _reference(ops, emb, idx, offs, mode, w, dy, pad):
    cores = [c.detach().clone().requires_grad_(True) for c in emb.tt_cores]
    full = ops.tt_matrix_to_full(emb.tt_p_shapes, emb.tt_q_shapes, emb.tt_ranks, cores, [1, 0, 2, 3])
    wr = None if w is None else w.detach().clone().requires_grad_(True)
    out = F.embedding_bag(idx, full, offs, mode=mode, per_sample_weights=wr, include_last_offset=True, padding_idx=pad)
    out.backward(dy)
    return out.detach(), [c.grad for c in cores], (None if wr is None else wr.grad)


def _close_grad(got, want):
    torch.testing.assert_close(got, want, rtol=0, atol=1e-4 * max(float(want.abs().max()), 1e-6))


def _close_step(got, want, lr_g):
    torch.testing.assert_close(got, want, rtol=0, atol=1e-5 + 1e-4 * float(lr_g.abs().max()))


def _dy(B, D, seed):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(B, D, generator=g) - 0.5) * 0.2).cuda()


def _want_route(nat, emb, nnz, B, weighted):
    fam = nat.kernel_family(emb._shape, nnz, B, False) & 7
    return "partition" if not weighted and fam in (nat.FAMILY_GROUPED, nat.FAMILY_GROUPED_WIDE) else "masked"


@pytest.mark.parametrize("share", [0.0, 0.3])
@pytest.mark.parametrize("kind", ["sum", "mean", "weighted"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_forward_and_gradients_on_every_route(nat, ops, case, kind, share):
    name, p, q, r, nnz = case
    idx, offs, w, pad = _inputs(p, nnz, seed=len(name), share=share)
    mode = "mean" if kind == "mean" else "sum"
    # the 30 % cases name the pad by its negative alias
    emb = _emb(ops, p, q, r, mode, padding_idx=pad - int(np.prod(p)) if share else pad)
    assert emb.padding_idx == pad
    B, D = offs.numel() - 1, emb.embedding_dim
    wt = w.clone().requires_grad_(True) if kind == "weighted" else None
    out = emb(idx, offs, per_sample_weights=wt)
    route = _want_route(nat, emb, nnz, B, kind == "weighted")
    assert emb._last_pad_route == route, (name, kind)
    if name == "grouped" and kind != "weighted":
        assert route == "partition"
    if name == "scalar":
        assert route == "masked"
    dy = _dy(B, D, 3)
    out.backward(dy)
    want, grads, wgrad = _reference(ops, emb, idx, offs, mode, w if kind == "weighted" else None, dy, pad)
    torch.testing.assert_close(out.detach(), want, rtol=1e-5, atol=1e-4)
    for c, g in zip(emb.tt_cores, grads):
        _close_grad(c.grad, g)
    if kind == "weighted":
        _close_grad(wt.grad, wgrad)
        assert not bool(wt.grad[idx == pad].any())


@pytest.mark.parametrize("mode", ["sum", "mean"])
@pytest.mark.parametrize("partition", [True, False])
def test_only_pad_ids(nat, ops, mode, partition):
    p, q, r = SMALL
    idx, offs, _, pad = _inputs(p, 20000, seed=2, share=0.0)
    idx = torch.full_like(idx, pad)
    emb = _emb(ops, p, q, r, mode, padding_idx=pad)
    emb._pad_partition = partition
    out = emb(idx, offs)
    assert emb._last_pad_route == ("partition" if partition else "masked")
    assert not bool(out.any())
    out.backward(torch.ones_like(out))
    for c in emb.tt_cores:
        assert not bool(c.grad.any())


@pytest.mark.parametrize("mode", ["sum", "mean"])
@pytest.mark.parametrize("optimizer", ["sgd", "adagrad"])
@pytest.mark.parametrize("partition", [True, False])
def test_fused_steps_leave_the_pad_row_alone(nat, ops, mode, optimizer, partition):
    p, q, r = SMALL
    lr, eps = 0.05, 1e-3
    opt = ops.OptimType.SGD if optimizer == "sgd" else ops.OptimType.EXACT_ADAGRAD
    idx, offs, _, pad = _inputs(p, 20000, seed=9, share=0.3)
    emb = _emb(ops, p, q, r, mode, sparse=True, optimizer=opt, learning_rate=lr, eps=eps, padding_idx=pad)
    emb._pad_partition = partition
    start = [c.detach().clone() for c in emb.tt_cores]
    state0 = [s.clone() for s in emb.optimizer_state]
    dy = _dy(offs.numel() - 1, emb.embedding_dim, 6)
    _, grads, _ = _reference(ops, emb, idx, offs, mode, None, dy, pad)
    emb(idx, offs).backward(dy)
    assert emb._last_pad_route == ("partition" if partition else "masked")
    for c, c0, g in zip(emb.tt_cores, start, grads):
        if optimizer == "sgd":
            _close_step(c.detach(), c0 - lr * g, lr * g)
        else:
            big = g.abs() > 1e-3 * float(g.abs().max())
            torch.testing.assert_close(c.detach()[big], (c0 - lr * g / (g.abs() + eps))[big], rtol=0, atol=1e-5)
    prow = pad // _pad_of(p)[1]
    assert not bool(grads[0][0, prow].any())   # (no other id touches the pad's G0 row)
    assert torch.equal(emb.tt_cores[0].detach()[0, prow], start[0][0, prow])
    if optimizer == "adagrad":
        assert torch.equal(emb.optimizer_state[0][0, prow], state0[0][0, prow])
        for st, g in zip(emb.optimizer_state, grads):
            torch.testing.assert_close(st, g * g, rtol=2e-4, atol=1e-4 * float((g * g).max()))


@pytest.mark.parametrize("mode", ["sum", "mean"])
def test_two_d_bags_are_the_one_d_call(nat, ops, mode):
    p, q, r = SMALL
    B, N = 4096, 10
    pad, _ = _pad_of(p)
    g = torch.Generator().manual_seed(1)
    idx2 = torch.randint(0, int(np.prod(p)), (B, N), generator=g).cuda()
    idx2[torch.rand(B, N, generator=g).cuda() < 0.3] = pad
    idx2[::17] = pad
    ar = torch.arange(0, B * N + 1, N, device="cuda")
    w2 = torch.randn(B, N, generator=g).cuda()
    # bit for bit where the lookup is (exact mode: the default grouped forward adds a bag's rows in an order of its own)
    for padding_idx in (None, pad):
        for exact in (True, False):
            emb = _emb(ops, p, q, r, mode, sparse=True, padding_idx=padding_idx, deterministic=exact)
            same = torch.equal if exact else (lambda x, y: torch.allclose(x, y, rtol=1e-6, atol=1e-6))
            with torch.no_grad():
                assert same(emb(idx2), emb(idx2.flatten(), ar)), (padding_idx, exact)
                if mode == "sum":
                    assert same(emb(idx2, per_sample_weights=w2), emb(idx2.flatten(), ar, per_sample_weights=w2.flatten()))
    emb = _emb(ops, p, q, r, mode, padding_idx=pad)
    out = emb(idx2)
    assert tuple(out.shape) == (B, emb.embedding_dim)
    dy = _dy(B, emb.embedding_dim, 2)
    out.backward(dy)
    want, grads, _ = _reference(ops, emb, idx2.flatten(), ar, mode, None, dy, pad)
    torch.testing.assert_close(out.detach(), want, rtol=1e-5, atol=1e-4)
    for c, gr in zip(emb.tt_cores, grads):
        _close_grad(c.grad, gr)


def test_two_d_argument_checks(nat, ops):
    p, q, r = SMALL
    idx2 = torch.randint(0, int(np.prod(p)), (8, 5), device="cuda")
    for padding_idx in (None, 3):
        emb = _emb(ops, p, q, r, padding_idx=padding_idx)
        with pytest.raises(ValueError):
            emb(idx2.flatten())
        with pytest.raises(ValueError):
            emb(idx2, torch.arange(0, 41, 5, device="cuda"))
        with pytest.raises(ValueError):
            emb(idx2, per_sample_weights=torch.ones(40, device="cuda"))
        with pytest.raises(ValueError):
            emb(idx2.view(2, 4, 5))
    tables = ops.TableBatchedTTEmbeddingBag(3, int(np.prod(p)), 100, r, p, q, use_cache=False, padding_idx=3)
    with pytest.raises(ValueError):
        tables(idx2)   # 8 rows are not 3 * B bags


def test_no_host_synchronisation(nat, ops):
    p, q, r = SMALL
    idx, offs, _, pad = _inputs(p, 20000, seed=4, share=0.3)
    emb = _emb(ops, p, q, r, sparse=True, padding_idx=pad)
    dy = _dy(offs.numel() - 1, emb.embedding_dim, 1)
    emb(idx, offs).backward(dy)   # (first call: workspace and scratch exist)
    assert emb._last_pad_route == "partition"
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        emb(idx, offs).backward(dy)
    finally:
        torch.cuda.set_sync_debug_mode("default")


def _exact_run(ops, mode):
    p, q, r = SMALL
    torch.manual_seed(0)
    idx, offs, _, pad = _inputs(p, 30000, seed=2, share=0.3)
    emb = _emb(ops, p, q, r, mode, sparse=True, optimizer=ops.OptimType.EXACT_ADAGRAD, learning_rate=0.05,
               deterministic=True, padding_idx=pad)
    out = emb(idx, offs)
    assert emb._last_pad_route == "masked"
    dy = _dy(offs.numel() - 1, emb.embedding_dim, 8)
    out.backward(dy)
    torch.cuda.synchronize()
    return [out.detach()] + [c.detach().clone() for c in emb.tt_cores] + [s.clone() for s in emb.optimizer_state]


@pytest.mark.parametrize("mode", ["sum", "mean"])
def test_exact_mode_is_bit_reproducible(nat, ops, mode):
    a, b = _exact_run(ops, mode), _exact_run(ops, mode)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("mode", ["sum", "mean"])
def test_live_row_cache(nat, ops, mode):
    p, q, r = SMALL
    n = int(np.prod(p))
    idx, offs, _, pad = _inputs(p, 6000, seed=12, share=0.3)
    emb = _emb(ops, p, q, r, mode, use_cache=True, cache_size=300, hashtbl_size=n, padding_idx=pad)
    with torch.no_grad():
        emb(idx, offs)   # warm-up statistics
    emb.cache_populate()
    assert not emb.warmup
    out = emb(idx, offs)
    assert emb._last_pad_route == "masked"
    dy = _dy(offs.numel() - 1, emb.embedding_dim, 2)
    out.backward(dy)
    want, grads, _ = _reference(ops, emb, idx, offs, mode, None, dy, pad)
    torch.testing.assert_close(out.detach(), want, rtol=1e-5, atol=1e-4)
    assert emb.cache_weight.grad is not None and bool(emb.cache_weight.grad.any())


@pytest.mark.parametrize("mode", ["sum", "mean"])
def test_several_tables(nat, ops, mode):
    p, q, r = SMALL
    Tn, B = 3, 700
    pad, _ = _pad_of(p)
    emb = ops.TableBatchedTTEmbeddingBag(Tn, int(np.prod(p)), 100, r, p, q, sparse=False, use_cache=False,
                                         weight_dist="uniform", mode=mode, padding_idx=pad)
    g = np.random.default_rng(3)
    lens = g.integers(0, 9, size=Tn * B)
    lens[::13] = 0
    offs = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int64).cuda()
    nnz = int(offs[-1])
    ids = g.integers(0, int(np.prod(p)), size=nnz)
    ids[g.random(nnz) < 0.3] = pad
    idx = torch.tensor(ids).cuda()
    out = emb(idx, offs)
    assert tuple(out.shape) == (Tn, B, 100) and emb._last_pad_route == "masked"
    dy = (torch.rand(Tn, B, 100, device="cuda") - 0.5) * 0.2
    out.backward(dy)
    bounds = offs[::B].tolist()
    for k in range(Tn):
        cores = [c.detach()[k:k + 1].clone().requires_grad_(True) for c in emb.tt_cores]
        full = ops.tt_matrix_to_full(p, q, emb.tt_ranks, cores, [1, 0, 2, 3])
        lo, hi = bounds[k], bounds[k + 1]
        o = F.embedding_bag(idx[lo:hi], full, offs[k * B:(k + 1) * B + 1] - lo, mode=mode, include_last_offset=True,
                            padding_idx=pad)
        torch.testing.assert_close(out[k].detach(), o.detach(), rtol=1e-5, atol=1e-4)
        o.backward(dy[k])
        for c, cr in zip(emb.tt_cores, cores):
            _close_grad(c.grad[k:k + 1], cr.grad)


@pytest.mark.parametrize("mode", ["sum", "mean"])
def test_inference(nat, ops, mode):
    p, q, r = SMALL
    idx, offs, _, pad = _inputs(p, 20000, seed=21, share=0.3)
    emb = _emb(ops, p, q, r, mode, sparse=True, padding_idx=pad)
    want, _, _ = _reference(ops, emb, idx, offs, mode, None,
                            torch.zeros(offs.numel() - 1, emb.embedding_dim, device="cuda"), pad)
    with torch.no_grad():
        out = emb(idx, offs)
    assert emb._last_pad_route == "partition"
    torch.testing.assert_close(out, want, rtol=1e-5, atol=1e-4)


def test_data_parallel_step(nat, ops):
    from ttemb_dist import TTDataParallel
    p, q, r = SMALL
    lr = 0.2
    idx, offs, _, pad = _inputs(p, 20000, seed=31, share=0.3)
    emb = _emb(ops, p, q, r, learning_rate=lr, padding_idx=pad)
    dp = TTDataParallel(emb)
    start = [c.detach().clone() for c in emb.tt_cores]
    dy = _dy(offs.numel() - 1, emb.embedding_dim, 9)
    _, grads, _ = _reference(ops, emb, idx, offs, "sum", None, dy, pad)
    emb(idx, offs).backward(dy)
    assert emb._last_pad_route == "partition"
    dp.step()
    torch.cuda.synchronize()
    for c, c0, g in zip(emb.tt_cores, start, grads):
        _close_step(c.detach(), c0 - lr * g, lr * g)
