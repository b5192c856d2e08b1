"""Max bags (``forward(..., mode="max")``) on the GPU.

C ABI level: ``ttemb_bag_max`` / ``ttemb_bag_max_backward`` against the numpy restatement below, BIT FOR BIT (output, argmax,
d_rows): first-position rule, NaN rule, pads.

Module level: against ``F.embedding_bag(mode="max")`` over the full table, autograd through ``tt_matrix_to_full``.  Forward
rtol 1e-5 / atol 1e-4 (max is 1-Lipschitz in the rows, so the rows' tolerance carries over), gradients 1e-4 of their largest
magnitude, fused steps 1e-5, as test_gpu_weighted.py.  Where the reference's largest values of DIFFERENT ids in a (bag,
column) lie within 2e-4 of each other (each side may be off by the forward tolerance) either id may win: ``dOut`` is set to
zero there for both sides -- at most 0.5 % of the non-empty (bag, column) pairs, asserted -- and everything else is compared
in full.  The cores are drawn normal(0, s) with s = (0.09 / prod(inner ranks))^(1 / (2 T)): row entries of standard deviation
0.3 (the "uniform" initialiser's all-positive rows of 0.02 +- a few 1e-3 would tie everywhere)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_gpu_padding as tp
import test_gpu_weighted as tw

pytestmark = pytest.mark.gpu

CASES, SMALL = tw.CASES, tw.SMALL
_close_grad, _close_step, _dy = tw._close_grad, tw._close_step, tw._dy
TIE, TIE_SHARE = 2e-4, 0.005


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


# ---------------------------------------------------------------------------------------
# C ABI level: bit for bit against numpy
# ---------------------------------------------------------------------------------------
def _walk(rows, keep):
    """The rule, literally: walk the kept positions in order; a later one wins only with a strictly larger value, or as the
    first NaN over a number.  -> (values [D], local positions [D]; -1 without a kept position)."""
    D = rows.shape[1]
    best, pos = np.zeros(D, np.float32), np.full(D, -1, np.int64)
    for i in range(rows.shape[0]):
        if not keep[i]:
            continue
        v = rows[i]
        take = (pos < 0) | (v > best) | (np.isnan(v) & ~np.isnan(best))
        best, pos = np.where(take, v, best), np.where(take, i, pos)
    return best, pos


def _closed_form(rows, keep):
    """The same winners without the walk (long bags): the first NaN of a column, else the first occurrence of its maximum."""
    D = rows.shape[1]
    k = np.nonzero(keep)[0]
    if k.size == 0:
        return np.zeros(D, np.float32), np.full(D, -1, np.int64)
    r = rows[k]
    nan = np.isnan(r)
    with np.errstate(invalid="ignore"):
        first_max = np.argmax(np.where(nan, -np.inf, r), axis=0)
    local = np.where(nan.any(axis=0), np.argmax(nan, axis=0), first_max)
    return r[local, np.arange(D)], k[local]


def _np_bag_max(rows, offs, ids=None, pad=None):
    nnz, D = rows.shape
    B = offs.size - 1
    out, arg = np.zeros((B, D), np.float32), np.full((B, D), -1, np.int32)
    keep = np.ones(nnz, bool) if ids is None else ids != pad
    for b in range(B):
        n0, n1 = int(offs[b]), int(offs[b + 1])
        if n1 <= n0:
            continue
        v, p = (_walk if n1 - n0 <= 64 else _closed_form)(rows[n0:n1], keep[n0:n1])
        out[b] = np.where(p >= 0, v, np.float32(0.0))
        arg[b] = np.where(p >= 0, p + n0, -1)
    return out, arg


def _np_bag_max_backward(d_out, arg, nnz):
    d_rows = np.zeros((nnz, d_out.shape[1]), np.float32)
    b, d = np.nonzero(arg >= 0)
    d_rows[arg[b, d], d] = d_out[b, d]   # (one writer each: a position lies in one bag)
    return d_rows


def test_the_two_numpy_forms_agree():
    rng = np.random.default_rng(0)
    for trial in range(20):
        rows = (rng.integers(-3, 4, size=(40, 8)) / 4).astype(np.float32)
        rows[rng.random(rows.shape) < 0.1] = np.nan
        rows[rng.random(rows.shape) < 0.1] = -0.0
        keep = rng.random(40) < (0.8 if trial else 0.0)
        a, b = _walk(rows, keep), _closed_form(rows, keep)
        assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1])


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32 if t.dtype == torch.float32 else np.int32)


def _abi_inputs(D, seed):
    """Ragged bags with empty ones, bags of one and a 200 000-id bag between short ones; rows copied from a small table of
    quarter-integer values (repeated ids: exact ties across positions everywhere), +0.0 and -0.0, all-negative bags, NaN
    planted first / in the middle / last, the long bag's maximum planted in its first, a middle and its last chunk."""
    rng = np.random.default_rng(seed)
    nnz = 230000
    lens = list(rng.integers(0, 9, size=2 * (nnz // 4) + 8))
    lens[::7] = [0] * len(lens[::7])
    lens[1::9] = [1] * len(lens[1::9])
    lens = lens[:3] + [200000] + lens[3:]
    offs = np.concatenate([[0], np.cumsum(lens)])
    offs = np.concatenate([offs[offs < nnz], [nnz, nnz]]).astype(np.int64)
    table = (rng.integers(-6, 7, size=(300, D)) / 4).astype(np.float32)
    table[rng.random(table.shape) < 0.05] = -0.0
    ids = rng.integers(0, 300, size=nnz)
    ids[::5] = ids[0]
    rows = table[ids].copy()
    starts, ends = offs[:-1], offs[1:]
    short = np.nonzero((ends - starts >= 3) & (ends - starts < 100))[0]
    for b in short[::11]:   # all-negative bags
        rows[starts[b]:ends[b]] = -np.abs(rows[starts[b]:ends[b]]) - 1
    for j, b in enumerate(short[5::13]):   # NaN first / middle / last, in a few columns
        at = (starts[b], (starts[b] + ends[b]) // 2, ends[b] - 1)[j % 3]
        rows[at, :: 3] = np.nan
    for b in short[7::17]:   # an exact tie of the bag's maximum planted at two positions
        rows[starts[b] + 1, 0] = rows[ends[b] - 1, 0] = 50.0
    lb = int(np.argmax(ends - starts))
    n0, n1 = int(starts[lb]), int(ends[lb])
    assert n1 - n0 == 200000
    rows[n0 + 5, 0] = 100.0                 # first chunk
    rows[n0 + 100000, 1] = 100.0            # a middle chunk
    rows[n1 - 1, 2] = 100.0                 # the last chunk
    rows[n0 + 700, 3] = rows[n0 + 150000, 3] = 100.0    # the same maximum in two chunks: the first wins
    if D > 4:
        rows[n0 + 90000, 4] = np.nan        # a NaN deep inside the long bag
        rows[n0 + 1000, 5] = rows[n0 + 199000, 5] = np.nan
    return rows, offs, ids


@pytest.mark.parametrize("D", [4, 100, 128, 1024])
def test_abi_bit_exact_against_numpy(nat, D):
    rows, offs, ids = _abi_inputs(D, seed=D)
    nnz, B = rows.shape[0], offs.size - 1
    pad = int(ids[0])   # (a fifth of the positions hold it)
    d_out = np.random.default_rng(1).standard_normal((B, D)).astype(np.float32)
    r, o, i, g = (torch.tensor(x).cuda() for x in (rows, offs, ids, d_out))
    ws = nat.Workspace()
    for padded in (False, True):
        want_out, want_arg = _np_bag_max(rows, offs, ids if padded else None, pad)
        want_rows = _np_bag_max_backward(d_out, want_arg, nnz)
        assert (want_arg[np.argmax(offs[1:] - offs[:-1]), :4] >= 0).all()
        for grid, garbage in ((0, False), (0, True), (1, True), (3, False)):
            nat.set_exact_grid(grid)
            try:
                out = torch.full((B, D), 7.0, device="cuda")
                arg = torch.full((B, D), -7, dtype=torch.int32, device="cuda")
                d_rows = torch.full((nnz, D), 7.0, device="cuda")
                if garbage and ws.buf is not None:
                    ws.buf.copy_(torch.randint(0, 256, ws.buf.shape, dtype=torch.uint8, device="cuda"))
                nat.bag_max(r, o, out, arg, ws, i if padded else None, pad)
                nat.bag_max_backward(g, arg, o, d_rows)
                torch.cuda.synchronize()
            finally:
                nat.set_exact_grid(0)
            assert np.array_equal(_bits(arg), want_arg), (padded, grid, garbage)
            assert np.array_equal(_bits(out), want_out.view(np.uint32)), (padded, grid, garbage)
            assert np.array_equal(_bits(d_rows), want_rows.view(np.uint32)), (padded, grid, garbage)


def test_abi_argument_checks(nat):
    ws = nat.Workspace()
    rows = torch.zeros(8, 6, device="cuda")
    offs = torch.tensor([0, 8], device="cuda")
    with pytest.raises(RuntimeError, match="multiple of 4"):
        nat.bag_max(rows, offs, torch.zeros(1, 6, device="cuda"), torch.zeros(1, 6, dtype=torch.int32, device="cuda"), ws)
    rows = torch.zeros(8, 8, device="cuda")
    with pytest.raises(ValueError):
        nat.bag_max(rows, offs, torch.zeros(1, 8, device="cuda"), torch.zeros(1, 8, dtype=torch.int64, device="cuda"), ws)
    odd = torch.zeros(8 * 8 + 1, device="cuda")[1:].view(8, 8)   # 4-byte, not 16-byte aligned
    with pytest.raises(RuntimeError, match="aligned"):
        nat.bag_max(odd, offs, torch.zeros(1, 8, device="cuda"), torch.zeros(1, 8, dtype=torch.int32, device="cuda"), ws)


# ---------------------------------------------------------------------------------------
# module level: against F.embedding_bag(mode="max")
# ---------------------------------------------------------------------------------------
def _emb(ops, p, q, r, mode="sum", **kw):
    kw.setdefault("sparse", False)
    kw.setdefault("use_cache", False)
    emb = ops.TTEmbeddingBag(int(np.prod(p)), int(np.prod(q)), r, p, q, weight_dist="uniform", mode=mode, **kw)
    s = (0.09 / float(np.prod(r))) ** (1.0 / (2 * len(p)))
    g = torch.Generator().manual_seed(1234)
    with torch.no_grad():
        for c in emb.tt_cores:
            c.copy_((torch.randn(c.shape, generator=g) * s).to(c.device))
    return emb


def _full(ops, emb, cores):
    return ops.tt_matrix_to_full(emb.tt_p_shapes, emb.tt_q_shapes, emb.tt_ranks, cores, [1, 0, 2, 3])


def _mask_near_ties(full, idx, offs, dy, pad=None):
    """``dy`` with zeros where, in the reference's table, positions of DIFFERENT ids lie within TIE of the bag's maximum
    (either may win on the other side).  Asserts the share of such (bag, column) pairs among the non-empty ones."""
    B, D = offs.numel() - 1, full.shape[1]
    lens = offs[1:] - offs[:-1]
    bag = torch.repeat_interleave(torch.arange(B, device=idx.device), lens)
    kept = torch.ones_like(idx, dtype=torch.bool) if pad is None else idx != pad
    rows = full.detach()[idx]
    top = torch.full((B, D), -float("inf"), device=idx.device)
    top.scatter_reduce_(0, bag[kept][:, None].expand(-1, D), rows[kept], "amax")
    near = kept[:, None] & (rows >= top[bag] - TIE)
    big = idx.max() + 1
    lo = torch.full((B, D), int(big), dtype=torch.int64, device=idx.device)
    hi = torch.full((B, D), -1, dtype=torch.int64, device=idx.device)
    ids = idx[:, None].expand(-1, D)
    lo.scatter_reduce_(0, bag[:, None].expand(-1, D), torch.where(near, ids, big), "amin")
    hi.scatter_reduce_(0, bag[:, None].expand(-1, D), torch.where(near, ids, -1), "amax")
    ambiguous = (hi >= 0) & (lo != hi)
    nonempty = int((hi >= 0).sum())
    share = int(ambiguous.sum()) / max(nonempty, 1)
    print(f"near ties: {int(ambiguous.sum())} of {nonempty} non-empty (bag, column) pairs = {100 * share:.3f} %")
    assert share <= TIE_SHARE, f"{100 * share:.3f} % of the (bag, column) pairs are near ties: choose other inputs"
    return torch.where(ambiguous, torch.zeros_like(dy), dy)


def _reference(ops, emb, idx, offs, dy, pad=None):
    """-> (reference output, core gradients, the dOut both sides use)."""
    cores = [c.detach().clone().requires_grad_(True) for c in emb.tt_cores]
    full = _full(ops, emb, cores)
    out = F.embedding_bag(idx, full, offs, mode="max", include_last_offset=True, padding_idx=pad)
    dy = _mask_near_ties(full, idx, offs, dy, pad)
    out.backward(dy)
    return out.detach(), [c.grad for c in cores], dy


def _check_call(ops, emb, idx, offs, seed, pad=None, call=None):
    B, D = offs.numel() - 1, emb.embedding_dim
    want, grads, dy = _reference(ops, emb, idx, offs, _dy(B, D, seed), pad)
    out = emb(idx, offs, mode="max") if call is None else call()
    assert tuple(out.shape) == (B, D)
    out.backward(dy)
    torch.testing.assert_close(out.detach(), want, rtol=1e-5, atol=1e-4)
    for c, g in zip(emb.tt_cores, grads):
        _close_grad(c.grad, g)
    return out.detach()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_forward_and_gradients_on_every_route(nat, ops, case):
    name, p, q, r, nnz, want_fam, prefix = case
    emb = _emb(ops, p, q, r)
    idx, offs, _ = tw._inputs(int(np.prod(p)), nnz, seed=len(name))
    fam = nat.kernel_family(emb._shape, nnz, nnz, True)   # the rows lookup: nnz bags of one
    assert fam & ~nat.FAMILY_ROUTE_FLAGS == want_fam, (name, fam)
    if prefix is not None:
        assert bool(fam & nat.FAMILY_PREFIX_IN_CHAIN) == prefix, (name, fam)
    _check_call(ops, emb, idx, offs, 3)


def test_bags_of_ten(nat, ops):
    p, q, r = SMALL
    emb = _emb(ops, p, q, r)
    idx, offs, _ = tw._inputs(int(np.prod(p)), 40960, seed=5, mean=10)
    _check_call(ops, emb, idx, offs, 4)


def test_ties_go_to_the_first_position_and_empty_bags_give_zeros(nat, ops):
    p, q, r = SMALL
    emb = _emb(ops, p, q, r)
    D = emb.embedding_dim
    idx = torch.tensor([5, 9, 5, 9, 5], device="cuda")
    offs = torch.tensor([0, 0, 3, 3, 5, 5], device="cuda")
    out = emb(idx, offs, mode="max")
    rows = emb.full_weight().detach()[idx]
    assert not bool(out[0].any()) and not bool(out[2].any()) and not bool(out[4].any())
    torch.testing.assert_close(out[1].detach(), torch.maximum(rows[0], rows[1]), rtol=1e-5, atol=1e-4)
    none = emb(torch.empty(0, dtype=torch.int64, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda"), mode="max")
    assert tuple(none.shape) == (3, D) and not bool(none.any())
    none.backward(torch.ones_like(none))
    assert all(not bool(c.grad.any()) for c in emb.tt_cores)
    assert tuple(emb(idx[:0], offs[:1], mode="max").shape) == (0, D)


@pytest.mark.parametrize("optimizer", ["sgd", "adagrad", "adam"])
def test_fused_steps_match_the_dense_gradient(nat, ops, optimizer):
    p, q, r = SMALL
    lr, eps = 0.05, 1e-3
    opt = {"sgd": ops.OptimType.SGD, "adagrad": ops.OptimType.EXACT_ADAGRAD, "adam": ops.OptimType.ADAM}[optimizer]
    emb = _emb(ops, p, q, r, sparse=True, optimizer=opt, learning_rate=lr, eps=eps)
    idx, offs, _ = tw._inputs(int(np.prod(p)), 20000, seed=9)
    start = [c.detach().clone() for c in emb.tt_cores]
    _, grads, dy = _reference(ops, emb, idx, offs, _dy(offs.numel() - 1, emb.embedding_dim, 6))
    emb(idx, offs, mode="max").backward(dy)
    for c, c0, g in zip(emb.tt_cores, start, grads):
        if optimizer == "sgd":
            _close_step(c.detach(), c0 - lr * g, lr * g)
        else:   # the first step of Adagrad and of Adam from zero state: lr g / (|g| + eps)
            big = g.abs() > 1e-3 * float(g.abs().max())
            torch.testing.assert_close(c.detach()[big], (c0 - lr * g / (g.abs() + eps))[big], rtol=0, atol=1e-5)
    if optimizer == "adagrad":
        for st, g in zip(emb.optimizer_state, grads):
            torch.testing.assert_close(st, g * g, rtol=2e-4, atol=1e-4 * float((g * g).max()))


@pytest.mark.parametrize("partition", [True, False])
def test_padding_on_both_routes(nat, ops, partition):
    p, q, r = SMALL
    idx, offs, _, pad = tp._inputs(p, 20000, seed=2, share=0.3)
    emb = _emb(ops, p, q, r, padding_idx=pad)
    emb._pad_partition = partition
    out = _check_call(ops, emb, idx, offs, 5, pad)
    assert emb._last_pad_route == ("partition" if partition else "masked")
    lens = offs[1:] - offs[:-1]
    bag = torch.repeat_interleave(torch.arange(lens.numel(), device="cuda"), lens)
    kept = torch.zeros(lens.numel(), dtype=torch.int64, device="cuda").index_add_(0, bag, (idx != pad).long())
    only_pads = (lens > 0) & (kept == 0)
    assert int(only_pads.sum()) > 10 and not bool(out[only_pads].any())
    # a call made of pads alone
    emb.zero_grad()
    out = emb(torch.full_like(idx, pad), offs, mode="max")
    assert emb._last_pad_route == ("partition" if partition else "masked") and not bool(out.any())
    out.backward(torch.ones_like(out))
    assert all(not bool(c.grad.any()) for c in emb.tt_cores)


@pytest.mark.parametrize("optimizer", ["sgd", "adagrad"])
@pytest.mark.parametrize("partition", [True, False])
def test_fused_steps_leave_the_pad_row_alone(nat, ops, optimizer, partition):
    p, q, r = SMALL
    lr, eps = 0.05, 1e-3
    opt = ops.OptimType.SGD if optimizer == "sgd" else ops.OptimType.EXACT_ADAGRAD
    idx, offs, _, pad = tp._inputs(p, 20000, seed=9, share=0.3)
    emb = _emb(ops, p, q, r, sparse=True, optimizer=opt, learning_rate=lr, eps=eps, padding_idx=pad)
    emb._pad_partition = partition
    start = [c.detach().clone() for c in emb.tt_cores]
    state0 = [s.clone() for s in emb.optimizer_state]
    _, grads, dy = _reference(ops, emb, idx, offs, _dy(offs.numel() - 1, emb.embedding_dim, 6), pad)
    emb(idx, offs, mode="max").backward(dy)
    assert emb._last_pad_route == ("partition" if partition else "masked")
    for c, c0, g in zip(emb.tt_cores, start, grads):
        if optimizer == "sgd":
            _close_step(c.detach(), c0 - lr * g, lr * g)
        else:
            big = g.abs() > 1e-3 * float(g.abs().max())
            torch.testing.assert_close(c.detach()[big], (c0 - lr * g / (g.abs() + eps))[big], rtol=0, atol=1e-5)
    prow = pad // tp._pad_of(p)[1]
    assert not bool(grads[0][0, prow].any())   # (no other id touches the pad's G0 row)
    assert torch.equal(emb.tt_cores[0].detach()[0, prow], start[0][0, prow])
    if optimizer == "adagrad":
        assert torch.equal(emb.optimizer_state[0][0, prow], state0[0][0, prow])


def test_two_d_bags_are_the_one_d_call(nat, ops):
    p, q, r = SMALL
    emb = _emb(ops, p, q, r)
    nbr = torch.randint(0, int(np.prod(p)), (900, 10), device="cuda")
    offs = torch.arange(0, 9001, 10, device="cuda")
    out = _check_call(ops, emb, nbr.reshape(-1), offs, 7, call=lambda: emb(nbr, mode="max"))
    with torch.no_grad():
        assert torch.equal(out, emb(nbr.reshape(-1), offs, mode="max"))
    with pytest.raises(ValueError):
        emb(nbr, offs, mode="max")


def test_two_tables(nat, ops):
    p, q, r = SMALL
    Tn, B = 2, 700
    emb = ops.TableBatchedTTEmbeddingBag(Tn, int(np.prod(p)), 100, r, p, q, sparse=False, use_cache=False,
                                         weight_dist="uniform")
    g = torch.Generator().manual_seed(4)
    s = (0.09 / float(np.prod(r))) ** (1.0 / 6)
    with torch.no_grad():
        for c in emb.tt_cores:
            c.copy_((torch.randn(c.shape, generator=g) * s).to(c.device))
    rng = np.random.default_rng(3)
    lens = rng.integers(0, 9, size=Tn * B)
    lens[::13] = 0
    offs = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int64).cuda()
    nnz = int(offs[-1])
    idx = torch.tensor(rng.integers(0, int(np.prod(p)), size=nnz)).cuda()
    out = emb(idx, offs, mode="max")
    assert tuple(out.shape) == (Tn, B, 100)
    dy = (torch.rand(Tn, B, 100, device="cuda") - 0.5) * 0.2
    bounds = offs[::B].tolist()
    refs = []
    for k in range(Tn):
        cores = [c.detach()[k:k + 1].clone().requires_grad_(True) for c in emb.tt_cores]
        full = ops.tt_matrix_to_full(p, q, emb.tt_ranks, cores, [1, 0, 2, 3])
        lo, hi = bounds[k], bounds[k + 1]
        offs_k = offs[k * B:(k + 1) * B + 1] - lo
        o = F.embedding_bag(idx[lo:hi], full, offs_k, mode="max", include_last_offset=True)
        torch.testing.assert_close(out[k].detach(), o.detach(), rtol=1e-5, atol=1e-4)
        dy[k] = _mask_near_ties(full, idx[lo:hi], offs_k, dy[k])
        o.backward(dy[k])
        refs.append(cores)
    out.backward(dy)
    for k in range(Tn):
        for c, cr in zip(emb.tt_cores, refs[k]):
            _close_grad(c.grad[k:k + 1], cr.grad)


def test_no_grad(nat, ops):
    p, q, r = SMALL
    emb = _emb(ops, p, q, r, sparse=True)
    idx, offs, _ = tw._inputs(int(np.prod(p)), 20000, seed=21)
    want = F.embedding_bag(idx, emb.full_weight().detach(), offs, mode="max", include_last_offset=True)
    with torch.no_grad():
        out = emb(idx, offs, mode="max")
    assert not out.requires_grad
    torch.testing.assert_close(out, want, rtol=1e-5, atol=1e-4)


def _exact_run(nat, ops, grid, garbage, pad):
    p, q, r = SMALL
    nat.set_exact_grid(grid)
    try:
        emb = _emb(ops, p, q, r, sparse=True, optimizer=ops.OptimType.EXACT_ADAGRAD, learning_rate=0.05, deterministic=True,
                   padding_idx=pad)
        idx, offs, _ = tw._inputs(int(np.prod(p)), 30000, seed=2, long_bag=3000)
        with torch.no_grad():   # (the workspace exists at its full size) ...
            emb(idx, offs, mode="max")
        if garbage:   # ... and holds garbage
            emb._ws.buf.copy_(torch.randint(0, 256, emb._ws.buf.shape, dtype=torch.uint8, device="cuda"))
        out = emb(idx, offs, mode="max")
        out.backward(_dy(offs.numel() - 1, emb.embedding_dim, 8))
        torch.cuda.synchronize()
        return [out.detach()] + [c.detach().clone() for c in emb.tt_cores] + [s.clone() for s in emb.optimizer_state]
    finally:
        nat.set_exact_grid(0)


@pytest.mark.parametrize("padded", [False, True])
def test_exact_mode_is_bit_reproducible(nat, ops, padded):
    pad = int(tw._inputs(int(np.prod(SMALL[0])), 30000, seed=2, long_bag=3000)[0][0]) if padded else None
    a = _exact_run(nat, ops, 0, False, pad)
    assert bool(a[0].any())
    for grid, garbage in ((0, True), (1, True), (3, False)):
        b = _exact_run(nat, ops, grid, garbage, pad)
        for x, y in zip(a, b):
            assert torch.equal(x, y), (grid, garbage)


@pytest.mark.parametrize("padded", [False, True])
def test_no_host_synchronisation(nat, ops, padded):
    p, q, r = SMALL
    if padded:
        idx, offs, _, pad = tp._inputs(p, 20000, seed=4, share=0.3)
    else:
        (idx, offs, _), pad = tw._inputs(int(np.prod(p)), 20000, seed=4), None
    emb = _emb(ops, p, q, r, sparse=True, padding_idx=pad)
    dy = _dy(offs.numel() - 1, emb.embedding_dim, 1)
    emb(idx, offs, mode="max").backward(dy)   # (first call: workspace and scratch exist)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        emb(idx, offs, mode="max").backward(dy)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if padded:
        assert emb._last_pad_route == "partition"


def test_a_poisoned_plan_gives_nan_never_numbers(nat, ops):
    """ttemb_set_spin_limit(-1): every bounded wait of the rows lookup's grouping pass expires, its rows are NaN -- and so is
    every element of every non-empty max bag (a NaN is never swallowed).  With the default limit the numbers are back."""
    p, q, r = [125, 140, 140], [4, 5, 5], [16, 16]
    emb = _emb(ops, p, q, r)
    n = 20000
    idx = torch.randperm(int(np.prod(p)))[:n].cuda()
    offs = torch.arange(0, n + 1, 4, device="cuda")
    nat.set_path(nat.PATH_FAST3)
    assert nat.kernel_family(emb._shape, n, n) & ~nat.FAMILY_ROUTE_FLAGS == nat.FAMILY_GROUPED
    nat.status()   # nothing pending
    nat.set_spin_limit(-1)
    try:
        out = emb(idx, offs, mode="max").detach()
        torch.cuda.synchronize()
    finally:
        nat.set_spin_limit(0)
    assert bool(torch.isnan(out).all()), "max bags over the rows of a poisoned plan must not return numbers"
    with pytest.raises(RuntimeError, match="gave up waiting"):
        nat.status()
    nat.status()   # consumed
    with torch.no_grad():
        out = emb(idx, offs, mode="max")
    want = F.embedding_bag(idx, emb.full_weight().detach(), offs, mode="max", include_last_offset=True)
    torch.testing.assert_close(out, want, rtol=1e-5, atol=1e-4)
    nat.status()


@pytest.mark.parametrize("mode,kind", [("sum", "plain"), ("sum", "weighted"), ("sum", "padded"), ("sum", "two_d"),
                                       ("mean", "plain"), ("mean", "padded"), ("mean", "two_d")])
def test_per_call_sum_and_mean_are_the_constructed_module(nat, ops, mode, kind):
    """Bit for bit, outputs and gradients -- in exact mode, where both are a function of the inputs alone (the default
    backward adds with float atomics: its gradients are not bit-stable run to run, whichever module runs it)."""
    p, q, r = SMALL
    other = "mean" if mode == "sum" else "sum"
    pad = None
    if kind == "padded":
        idx, offs, w, pad = tp._inputs(p, 20000, seed=6, share=0.3)
    else:
        idx, offs, w = tw._inputs(int(np.prod(p)), 20000, seed=6)
    a = _emb(ops, p, q, r, mode, padding_idx=pad, deterministic=True)    # constructed with the mode
    b = _emb(ops, p, q, r, other, padding_idx=pad, deterministic=True)   # the other one, the mode given per call
    args = (idx[:19990].view(1999, 10),) if kind == "two_d" else (idx, offs)
    kw = {"per_sample_weights": w} if kind == "weighted" else {}
    out_a, out_b = a(*args, **kw), b(*args, mode=mode, **kw)
    assert b.mode == other and a._last_pad_route == b._last_pad_route
    dy = _dy(out_a.shape[0], out_a.shape[1], 2)
    out_a.backward(dy)
    out_b.backward(dy)
    assert bool(out_a.any()) and torch.equal(out_a, out_b)
    for x, y in zip(a.tt_cores, b.tt_cores):
        assert torch.equal(x.grad, y.grad)


def test_per_call_mode_never_writes_the_modules_mode(nat, ops):
    """``forward(mode=...)`` is an argument of the call, not a state of the module: a "sum" module called with "mean" and
    with "sum", 1-D ids with offsets (8 ids in 3 bags, the middle one empty) and 2-D ids, never assigns ``mode`` -- a second
    thread or a ``capture()`` reading it meanwhile sees the constructor's -- and its "mean" is the constructed "mean" module's
    (the file's forward tolerance)."""
    p, q, r = [10, 10, 10], [2, 2, 4], [4, 4]
    writes = []

    class Recording(ops.TTEmbeddingBag):
        def __setattr__(self, name, value):
            if name == "mode" and "mode" in self.__dict__:   # (the first assignment is the constructor's)
                writes.append(value)
            super().__setattr__(name, value)

    ref = _emb(ops, p, q, r, "mean")
    e = Recording(1000, 16, r, p, q, use_cache=False, sparse=False)
    with torch.no_grad():
        for c, c0 in zip(e.tt_cores, ref.tt_cores):
            c.copy_(c0)
    assert e.mode == "sum" and writes == []
    idx = torch.tensor([3, 999, 17, 500, 3, 42, 0, 731], device="cuda")
    offs = torch.tensor([0, 5, 5, 8], device="cuda")
    for call in ((idx, offs), (idx.view(2, 4),)):
        mean, total = e(*call, mode="mean"), e(*call, mode="sum")
        assert bool(mean.any())
        torch.testing.assert_close(total, e(*call), rtol=1e-5, atol=1e-4)
        torch.testing.assert_close(mean, ref(*call), rtol=1e-5, atol=1e-4)
    assert not bool(e(idx, offs, mode="mean")[1].any())   # the empty bag
    assert writes == [] and e.mode == "sum"
