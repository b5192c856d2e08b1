"""Captured pooled lookups on the GPU: ``emb.capture_bags(...)`` -- weighted, mean, max, padded and 2-D bags through one pair
of HIP graphs -- with its staging launch (``ttemb_stage_bags``) and the count-aware pooling calls (``ttemb_*_n``).

References.  SGD: ``F.embedding_bag`` over the module's full table with autograd through ``tt_matrix_to_full`` (the recipe of
test_gpu_weighted.py::_reference, ``padding_idx=`` for the padded kinds), computed from the captured module's cores before
each step.  Tolerances from there: forward rtol 1e-5 / atol 1e-4, ``w.grad`` within 1e-4 of its largest magnitude, the cores
after the step within 1e-5 + 1e-4 max|lr g| of ``w0 - lr g_ref``.  Max bags: where the reference's largest values of
DIFFERENT ids of a (bag, column) lie within 2e-4 of each other either id may win, and ``dOut`` is zero there for both sides
(test_gpu_max.py; its 0.5 % bound on the share of such pairs is 2 % here: this table's rows have a standard deviation of
0.13 and one bag of 1100 ids over 800 rows, so more of them lie close).  Adagrad and Adam: the eager twin module (the
existing code path) on the same live ids, offsets, weights and mode; cores and optimiser state within
1e-5 + 1e-4 max|delta|, ``delta`` the twin's own change of that tensor in the step -- what ``lr g`` is for SGD.

Figures of the first run (max |captured - reference|) are printed by every test before it asserts."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_gpu_capture_variable as tv

pytestmark = pytest.mark.gpu

P, Q, R, N_EMB, D, CAP = tv.P, tv.Q, tv.R, tv.N_EMB, tv.D, tv.CAP
SENTINEL = tv.SENTINEL
W_SENTINEL = -12345.5
PAD = 5
LIVE = 1500
TIE, TIE_SHARE = 2e-4, 0.02


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    import FBTT.tt_embeddings_ops as m
    return m


@pytest.fixture(scope="module")
def nat():
    assert torch.cuda.is_available()
    import ttemb_native
    return ttemb_native


def _dev(a):
    return torch.tensor(a).cuda()


def _offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def _long_bag_lengths(rng, n, long_bag=1100):
    """Ragged bags of 0..4 ids that sum to n, with one bag of ``long_bag`` ids (it crosses two 512-id chunk edges) between a
    short and an empty one."""
    lens = list(tv._ragged_lengths(rng, n - long_bag - 2, CAP - 8))
    at = min(5, len(lens))
    lens[at:at] = [2, long_bag, 0]
    assert sum(lens) == n and len(lens) <= CAP and sum(lens[:at + 1]) < 512
    return np.asarray(lens, dtype=np.int64)


# ---------------------------------------------------------------------------------------------------------------------
# 1. ttemb_stage_bags against numpy
# ---------------------------------------------------------------------------------------------------------------------
def _stage_bags_ref(ids, offs, w, B_live, fanout, idx_buf, w_buf, B_cap):
    """numpy restatement of ttemb_stage_bags: tv._stage_ref plus the generated offsets of a fanout and the weights."""
    if fanout:
        offs = np.arange(B_live + 1, dtype=np.int64) * fanout
    idx, o, n = tv._stage_ref(ids, offs, B_live, idx_buf, B_cap)
    wo = w_buf.copy()
    if w is not None:
        wo[:n] = w
    return idx, o, wo, n


def _stage_and_compare(nat, ids, offs, w, B_live, fanout):
    n = ids.size
    idx_buf, w_buf = np.full(CAP, SENTINEL, dtype=np.int64), np.full(CAP, W_SENTINEL, dtype=np.float32)
    t_idx, t_w = _dev(idx_buf), _dev(w_buf)
    t_off = torch.full((CAP + 1,), SENTINEL, dtype=torch.int64, device="cuda")
    t_cnt = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    nat.stage_bags(_dev(ids), None if offs is None else _dev(offs), None if w is None else _dev(w), t_idx, t_off,
                   None if w is None else t_w, t_cnt, fanout=fanout, B_live=B_live)
    torch.cuda.synchronize()
    want_idx, want_off, want_w, want_cnt = _stage_bags_ref(ids, offs, w, B_live, fanout, idx_buf, w_buf, CAP)
    assert np.array_equal(t_idx.cpu().numpy(), want_idx), (n, "ids / the untouched tail")
    assert np.array_equal(t_off.cpu().numpy(), want_off), (n, "offsets / their padded tail")
    assert np.array_equal(t_w.cpu().numpy(), want_w), (n, "weights / the untouched tail")
    assert int(t_cnt.item()) == want_cnt, n


def _stage_ids(rng, n, dtype):
    ids = rng.integers(0, 2 ** 31 - 1, size=n).astype(dtype)
    if dtype == np.int64 and n:
        ids[0] = 2 ** 40 + 5   # (past int32: the int64 path copies all 64 bits)
    if n > 1:
        ids[1] = -3            # (a negative int32 is sign-extended)
    return ids


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weights"])
@pytest.mark.parametrize("bags", ["ragged", "bags_of_one"])
@pytest.mark.parametrize("dtype", [np.int64, np.int32], ids=["int64", "int32"])
def test_stage_bags_against_numpy(nat, dtype, bags, weighted):
    rng = np.random.default_rng(3)
    for n in (0, 1, 63, 64, 65, 4095, 4096):
        ids = _stage_ids(rng, n, dtype)
        w = rng.standard_normal(n).astype(np.float32) if weighted else None
        if bags == "bags_of_one":
            offs, B_live = (None, n) if n % 2 else (np.arange(n + 1).astype(dtype), n)   # (both ways of saying it)
        else:
            lens = tv._ragged_lengths(rng, n, CAP) if n else np.zeros(3, dtype=np.int64)
            offs, B_live = _offsets(lens).astype(dtype), lens.size
        _stage_and_compare(nat, ids, offs, w, B_live, 0)


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weights"])
@pytest.mark.parametrize("fanout", [1, 3, 10])
@pytest.mark.parametrize("dtype", [np.int64, np.int32], ids=["int64", "int32"])
def test_stage_bags_generates_the_offsets_of_a_fanout(nat, dtype, fanout, weighted):
    """rows * fanout ids, no offsets: 0, N, 2N, ... up to the live rows, the id count past them.  Sizes: no row, one row, 21
    rows, and the most rows whose ids stay just under / reach the capacity."""
    rng = np.random.default_rng(4)
    for rows in (0, 1, 21, (CAP - 1) // fanout, CAP // fanout):
        n = rows * fanout
        ids = _stage_ids(rng, n, dtype)
        w = rng.standard_normal(n).astype(np.float32) if weighted else None
        _stage_and_compare(nat, ids, None, w, rows, fanout)


# ---------------------------------------------------------------------------------------------------------------------
# 2. count-aware pooling, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pool_inputs():
    """Capacity 4096 with 1500 live ids: short and empty bags around one bag of 1100 ids (it begins before position 512 and
    crosses the chunk edges 512 and 1024), then bags past the live ids -- two empty ones at 1500 and one [1500, 4096) that lies wholly
    past the count.  Everything at a position >= 1500 of the inputs is NaN / an id of its own: reading it would show."""
    rng = np.random.default_rng(21)
    lens = _long_bag_lengths(rng, LIVE)
    live_bags = lens.size
    offs = np.concatenate([_offsets(lens), [LIVE, LIVE, CAP]]).astype(np.int64)
    B = offs.size - 1
    rows = rng.standard_normal((CAP, D)).astype(np.float32)
    rows[30] = rows[25]             # equal values inside the long bag: the first position has to win
    w = rng.standard_normal(CAP).astype(np.float32)
    w[::11] = 0.0
    ids = rng.integers(0, N_EMB, size=CAP).astype(np.int64)
    ids[rng.random(CAP) < 0.3] = PAD
    rows[LIVE:], w[LIVE:] = np.nan, np.nan
    dy = ((rng.random((B, D)) - 0.5) * 0.1).astype(np.float32)
    # a second set of offsets that spans the whole capacity, for nnz_dev = NULL
    full_lens = _long_bag_lengths(rng, CAP)
    full = dict(offs=_dev(_offsets(full_lens)), rows=_dev(np.nan_to_num(rows, nan=0.25)), w=_dev(np.nan_to_num(w, nan=-0.5)))
    full["dy"] = _dev(((rng.random((full_lens.size, D)) - 0.5) * 0.1).astype(np.float32))
    return dict(offs=_dev(offs), B=B, live_bags=live_bags, rows=_dev(rows), w=_dev(w), ids=_dev(ids), dy=_dev(dy),
                cnt=torch.tensor([LIVE], dtype=torch.int32, device="cuda"), full=full)


def _f(shape, fill=W_SENTINEL):
    return torch.full(shape, fill, dtype=torch.float32, device="cuda")


def test_counted_reduce_is_the_live_call_bit_for_bit(nat, pool_inputs):
    x, ws = pool_inputs, nat.Workspace()
    B, offs, cnt = x["B"], x["offs"], x["cnt"]
    out, want = _f((B, D)), _f((B, D))
    nat.bag_reduce(x["rows"], x["w"], offs, out, ws, nnz_dev=cnt, counted=True)
    nat.bag_reduce(x["rows"][:LIVE], x["w"][:LIVE], offs, want, ws)
    assert torch.equal(out, want) and bool(torch.isfinite(out).all())
    assert bool((out[x["live_bags"]:] == 0).all())          # bags past the live ids are empty
    # backward, with and without the weight gradient
    for with_dw in (True, False):
        d_rows, d_w = _f((CAP, D)), (_f((CAP,)) if with_dw else None)
        r_rows, r_w = _f((LIVE, D)), (_f((LIVE,)) if with_dw else None)
        nat.bag_reduce_backward(x["dy"], x["w"], offs, d_rows, ws, rows=x["rows"] if with_dw else None, d_weights=d_w,
                                nnz_dev=cnt, counted=True)
        nat.bag_reduce_backward(x["dy"], x["w"][:LIVE], offs, r_rows, ws, rows=x["rows"][:LIVE] if with_dw else None,
                                d_weights=r_w)
        assert torch.equal(d_rows[:LIVE], r_rows) and bool((d_rows[LIVE:] == W_SENTINEL).all())
        if with_dw:
            assert torch.equal(d_w[:LIVE], r_w) and bool((d_w[LIVE:] == W_SENTINEL).all())
    # nnz_dev = NULL: the existing entry point at full size
    fx = x["full"]
    Bf = fx["offs"].numel() - 1
    out, want = _f((Bf, D)), _f((Bf, D))
    nat.bag_reduce(fx["rows"], fx["w"], fx["offs"], out, ws, nnz_dev=None, counted=True)
    nat.bag_reduce(fx["rows"], fx["w"], fx["offs"], want, ws)
    assert torch.equal(out, want)
    d_rows, d_w, r_rows, r_w = _f((CAP, D)), _f((CAP,)), _f((CAP, D)), _f((CAP,))
    nat.bag_reduce_backward(fx["dy"], fx["w"], fx["offs"], d_rows, ws, rows=fx["rows"], d_weights=d_w, counted=True)
    nat.bag_reduce_backward(fx["dy"], fx["w"], fx["offs"], r_rows, ws, rows=fx["rows"], d_weights=r_w)
    assert torch.equal(d_rows, r_rows) and torch.equal(d_w, r_w)


@pytest.mark.parametrize("padded", [False, True], ids=["unpadded", "padded"])
def test_counted_max_is_the_live_call_bit_for_bit(nat, pool_inputs, padded):
    x, ws = pool_inputs, nat.Workspace()
    B, offs, cnt = x["B"], x["offs"], x["cnt"]
    ids = x["ids"] if padded else None
    i32 = lambda shape: torch.full(shape, -99, dtype=torch.int32, device="cuda")
    out, arg, want, want_arg = _f((B, D)), i32((B, D)), _f((B, D)), i32((B, D))
    nat.bag_max(x["rows"], offs, out, arg, ws, ids, PAD, nnz_dev=cnt, counted=True)
    nat.bag_max(x["rows"][:LIVE], offs, want, want_arg, ws, None if ids is None else ids[:LIVE], PAD)
    assert torch.equal(out, want) and torch.equal(arg, want_arg) and bool(torch.isfinite(out).all())
    assert bool((out[x["live_bags"]:] == 0).all()) and bool((arg[x["live_bags"]:] == -1).all())
    assert int(arg.max()) < LIVE
    d_rows, r_rows = _f((CAP, D)), _f((LIVE, D))
    nat.bag_max_backward(x["dy"], arg, offs, d_rows, nnz_dev=cnt, counted=True)
    nat.bag_max_backward(x["dy"], want_arg, offs, r_rows)
    assert torch.equal(d_rows[:LIVE], r_rows) and bool((d_rows[LIVE:] == W_SENTINEL).all())
    fx = x["full"]
    Bf = fx["offs"].numel() - 1
    out, arg, want, want_arg = _f((Bf, D)), i32((Bf, D)), _f((Bf, D)), i32((Bf, D))
    nat.bag_max(fx["rows"], fx["offs"], out, arg, ws, ids, PAD, nnz_dev=None, counted=True)
    nat.bag_max(fx["rows"], fx["offs"], want, want_arg, ws, ids, PAD)
    assert torch.equal(out, want) and torch.equal(arg, want_arg)
    d_rows, r_rows = _f((CAP, D)), _f((CAP, D))
    nat.bag_max_backward(fx["dy"], arg, fx["offs"], d_rows, counted=True)
    nat.bag_max_backward(fx["dy"], want_arg, fx["offs"], r_rows)
    assert torch.equal(d_rows, r_rows)


@pytest.mark.parametrize("mean", [False, True], ids=["sum", "mean"])
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weights"])
def test_counted_pad_weights_is_the_live_call_bit_for_bit(nat, pool_inputs, weighted, mean):
    x = pool_inputs
    offs, cnt = x["offs"], x["cnt"]
    w = x["w"] if weighted else None
    out, want = _f((CAP,)), _f((LIVE,))
    nat.pad_weights(x["ids"], offs, w, PAD, mean, out, nnz_dev=cnt, counted=True)
    nat.pad_weights(x["ids"][:LIVE], offs, None if w is None else w[:LIVE], PAD, mean, want)
    assert torch.equal(out[:LIVE], want) and bool(torch.isfinite(want).all())
    assert bool((out[LIVE:] == W_SENTINEL).all())
    # offsets that leave positions outside every bag, in front and behind: zeros there, up to the count and no further
    inner = torch.tensor([40, 47, 47, 1200, 1300], device="cuda")
    out, want = _f((CAP,)), _f((LIVE,))
    nat.pad_weights(x["ids"], inner, w, PAD, mean, out, nnz_dev=cnt, counted=True)
    nat.pad_weights(x["ids"][:LIVE], inner, None if w is None else w[:LIVE], PAD, mean, want)
    assert torch.equal(out[:LIVE], want) and bool((out[:40] == 0).all()) and bool((out[1300:LIVE] == 0).all())
    assert bool((out[LIVE:] == W_SENTINEL).all())
    fx = x["full"]
    wf = fx["w"] if weighted else None
    out, want = _f((CAP,)), _f((CAP,))
    nat.pad_weights(x["ids"], fx["offs"], wf, PAD, mean, out, nnz_dev=None, counted=True)
    nat.pad_weights(x["ids"], fx["offs"], wf, PAD, mean, want)
    assert torch.equal(out, want)


# ---------------------------------------------------------------------------------------------------------------------
# captured bags against their references
# ---------------------------------------------------------------------------------------------------------------------
# kind -> (mode, weighted, padded, fanout)
KINDS = {"weighted_sum": ("sum", True, False, None), "mean": ("mean", False, False, None), "max": ("max", False, False, None),
         "padded_sum": ("sum", False, True, None), "padded_mean": ("mean", False, True, None),
         "padded_max": ("max", False, True, None), "fanout8_padded_mean": ("mean", False, True, 8),
         "fanout8_padded_weighted_sum": ("sum", True, True, 8)}
# live sizes of the steps: (ids, what kind of bags, int32 ids and offsets)
STEPS = ((4096, "long", False), (1000, "ragged", True), (17, "ragged", False), (0, "empty", False), (4095, "ones", False))


def _pair(ops, optimizer, padded, **kw):
    return tv._pair(ops, optimizer, **(dict(kw, padding_idx=PAD) if padded else kw))


def _call(rng, n, bags, kind, int32=False):
    """One call of n ids for ``kind``: (ids, offsets or None, weights or None, the offsets a reference needs)."""
    mode, weighted, padded, fanout = KINDS[kind]
    if fanout:
        n = (n // fanout) * fanout
    ids = rng.integers(0, N_EMB, size=n).astype(np.int64)   # (a small table: duplicate ids in every call)
    if fanout:
        lens = np.full(n // fanout, fanout, dtype=np.int64)
    elif bags == "long":
        lens = _long_bag_lengths(rng, n)
    elif bags == "ragged":
        lens = tv._ragged_lengths(rng, n, CAP)
    elif bags == "empty":
        lens = np.zeros(3, dtype=np.int64)
    else:
        lens = np.ones(n, dtype=np.int64)
    offs = _offsets(lens)
    if padded and n:
        ids[rng.random(n) < 0.3] = PAD
        b = int(np.flatnonzero(lens > 0)[1 if (lens > 0).sum() > 1 else 0])
        ids[offs[b]:offs[b + 1]] = PAD           # one bag of pads only
    w = None
    if weighted:
        w = rng.standard_normal(n).astype(np.float32)
        w[::11] = 0.0
    it = np.int32 if int32 else np.int64
    t_ids = _dev(ids.astype(it))
    if fanout:
        t_ids, t_w = t_ids.view(n // fanout, fanout), (None if w is None else _dev(w).view(n // fanout, fanout))
        return t_ids, None, t_w, _dev(offs)
    t_offs = None if bags == "ones" else _dev(offs.astype(it))   # ("ones": without offsets, one bag per id)
    return t_ids, t_offs, (None if w is None else _dev(w)), _dev(offs)


def _mask_near_ties(full, idx, offs, dy, pad):
    """test_gpu_max.py::_mask_near_ties with this file's bound on the share (module docstring)."""
    B = offs.numel() - 1
    lens = offs[1:] - offs[:-1]
    bag = torch.repeat_interleave(torch.arange(B, device=idx.device), lens)
    kept = torch.ones_like(idx, dtype=torch.bool) if pad is None else idx != pad
    rows = full.detach()[idx]
    top = torch.full((B, D), -float("inf"), device=idx.device)
    top.scatter_reduce_(0, bag[kept][:, None].expand(-1, D), rows[kept], "amax")
    near = kept[:, None] & (rows >= top[bag] - TIE)
    big = int(idx.max()) + 1
    lo = torch.full((B, D), big, dtype=torch.int64, device=idx.device)
    hi = torch.full((B, D), -1, dtype=torch.int64, device=idx.device)
    ids = idx[:, None].expand(-1, D)
    lo.scatter_reduce_(0, bag[:, None].expand(-1, D), torch.where(near, ids, big), "amin")
    hi.scatter_reduce_(0, bag[:, None].expand(-1, D), torch.where(near, ids, -1), "amax")
    ambiguous = (hi >= 0) & (lo != hi)
    share = int(ambiguous.sum()) / max(int((hi >= 0).sum()), 1)
    print(f" near ties {100 * share:.3f} %", end="")
    assert share <= TIE_SHARE, f"{100 * share:.3f} % of the (bag, column) pairs are near ties: choose other inputs"
    return torch.where(ambiguous, torch.zeros_like(dy), dy)


def _reference(ops, emb, idx, offs, mode, w, dy, pad):
    """F.embedding_bag over the full table, autograd through the cores and the weights -> (output, core gradients, the weight
    gradient, the dOut both sides use)."""
    cores = [c.detach().clone().requires_grad_(True) for c in emb.tt_cores]
    full = ops.tt_matrix_to_full(emb.tt_p_shapes, emb.tt_q_shapes, emb.tt_ranks, cores, [1, 0, 2, 3])
    wr = None if w is None else w.detach().clone().requires_grad_(True)
    out = F.embedding_bag(idx, full, offs, mode=mode, per_sample_weights=wr, include_last_offset=True, padding_idx=pad)
    if mode == "max":
        dy = _mask_near_ties(full, idx, offs, dy, pad)
    out.backward(dy)
    return out.detach(), [c.grad for c in cores], (None if wr is None else wr.grad), dy


def _dy(rng, B):
    return _dev(((rng.random((B, D)) - 0.5) * 0.05).astype(np.float32))


def _tensors(m):
    """Everything a step may move: cores, optimiser state, Adam's step words."""
    adam = [*m.optimizer_state_v, m.adam_step] if hasattr(m, "optimizer_state_v") else []
    return [*m.tt_cores, *[s for s in m.optimizer_state if s.numel()], *adam]


def _no_id_step(b, cap, ids, offs, w, B_live):
    """A call without ids: zeros, an empty weight gradient, and a backward that leaves everything bit-identical."""
    before = [t.detach().clone() for t in _tensors(b)]
    wt = None if w is None else w.clone().requires_grad_(True)
    cap.output.fill_(float("nan"))
    out = cap(ids, offs, wt)
    assert tuple(out.shape) == (B_live, D) and bool((out == 0).all())
    out.backward(torch.ones_like(out))
    torch.cuda.synchronize()
    for t, t0 in zip(_tensors(b), before):
        assert torch.equal(t.detach(), t0)
    if wt is not None:
        assert wt.grad is not None and wt.grad.shape == wt.shape and wt.grad.numel() == 0


def _sgd_step(ops, b, cap, kind, call, rng, label):
    """One captured SGD step against F.embedding_bag + autograd on the cores the module holds right now."""
    mode, weighted, padded, fanout = KINDS[kind]
    ids, offs, w, offs_ref = call
    n, B_live = ids.numel(), offs_ref.numel() - 1
    if n == 0:
        return _no_id_step(b, cap, ids, offs, w, B_live)
    lr = float(b.learning_rate)
    w0 = [c.detach().clone() for c in b.tt_cores]
    want, grads, wgrad, dy = _reference(ops, b, ids.reshape(-1).long(), offs_ref, mode, None if w is None else w.reshape(-1),
                                        _dy(rng, B_live), PAD if padded else None)
    wt = None if w is None else w.clone().requires_grad_(True)
    out = cap(ids, offs, wt)
    assert tuple(out.shape) == (B_live, D)
    print(f"\n  {label} n={n:5d} bags={B_live:5d} out {float((out.detach() - want).abs().max()):.2e}", end="")
    torch.testing.assert_close(out.detach(), want, rtol=1e-5, atol=1e-4)
    out.backward(dy)
    torch.cuda.synchronize()
    if wt is not None:
        got, ref = wt.grad.reshape(-1), wgrad
        print(f" w.grad {float((got - ref).abs().max()):.2e} of {float(ref.abs().max()):.2e}", end="")
        torch.testing.assert_close(got, ref, rtol=0, atol=1e-4 * max(float(ref.abs().max()), 1e-6))
    for c, c0, g in zip(b.tt_cores, w0, grads):
        print(f" core {float((c.detach() - (c0 - lr * g)).abs().max()):.2e}", end="")
        torch.testing.assert_close(c.detach(), c0 - lr * g, rtol=0, atol=1e-5 + 1e-4 * float((lr * g).abs().max()))
    return out


def _twin_step(a, b, cap, kind, call, rng, label):
    """One captured step against the eager twin ``a`` (Adagrad / Adam; also the exact and first-position tests)."""
    mode, weighted, padded, fanout = KINDS[kind]
    ids, offs, w, offs_ref = call
    n, B_live = ids.numel(), offs_ref.numel() - 1
    if n == 0:
        return _no_id_step(b, cap, ids, offs, w, B_live)
    dy = _dy(rng, B_live)
    before = [t.detach().clone() for t in _tensors(a)]
    wa, wb = (None, None) if w is None else (w.clone().requires_grad_(True), w.clone().requires_grad_(True))
    out_a = a(ids.long(), None if fanout else offs_ref, per_sample_weights=wa, mode=mode)
    out_b = cap(ids, offs, wb)
    assert out_b.shape == out_a.shape
    print(f"\n  {label} n={n:5d} bags={B_live:5d} out {float((out_b - out_a).detach().abs().max()):.2e}", end="")
    torch.testing.assert_close(out_b.detach(), out_a.detach(), rtol=1e-5, atol=1e-4)
    out_a.backward(dy)
    out_b.backward(dy)
    torch.cuda.synchronize()
    if wa is not None:
        print(f" w.grad {float((wb.grad - wa.grad).abs().max()):.2e}", end="")
        torch.testing.assert_close(wb.grad, wa.grad, rtol=0, atol=1e-4 * max(float(wa.grad.abs().max()), 1e-6))
    for ta, tb, t0 in zip(_tensors(a), _tensors(b), before):
        if ta.dtype == torch.int32:     # Adam's step words: t itself must be equal
            assert int(ta[0, 0]) == int(tb[0, 0])
            continue
        delta = float((ta.detach() - t0).abs().max())
        print(f" {float((tb.detach() - ta.detach()).abs().max()):.2e}/{delta:.1e}", end="")
        torch.testing.assert_close(tb.detach(), ta.detach(), rtol=0, atol=1e-5 + 1e-4 * delta)
    return out_b


def _force(nat, b, family):
    nat.set_path(nat.PATH_PER_BAG if family == "per_bag" else nat.PATH_FAST3)
    fam = nat.kernel_family(b._shape, CAP, CAP, True) & 7
    assert fam == (nat.FAMILY_PER_BAG if family == "per_bag" else nat.FAMILY_GROUPED)


def _capture(b, kind, nnz=CAP, B=CAP, variable=True):
    mode, weighted, padded, fanout = KINDS[kind]
    if fanout:
        B = nnz // fanout
    return b.capture_bags(nnz, B, mode=mode, weighted=weighted, fanout=fanout, variable=variable)


# 3. ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["per_bag", "grouped"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_captured_bags_train_like_the_reference_sgd(ops, nat, kind, family):
    """Five SGD steps of live sizes 4096 (ragged, with the 1100-id bag) -> 1000 (ragged with empty bags, duplicate ids, int32)
    -> 17 -> 0 ids in 3 empty bags -> 4095 (one bag per id, no offsets) through ONE pair of graphs captured at capacity 4096."""
    _, b = _pair(ops, "SGD", KINDS[kind][2])
    try:
        _force(nat, b, family)
        cap = _capture(b, kind)
        assert cap.route == ("mean" if kind == "mean" else "rows")
        rng = np.random.default_rng(2)
        for n, bags, i32 in STEPS:
            _sgd_step(ops, b, cap, kind, _call(rng, n, bags, kind, i32), rng, f"{kind}/{family}")
        nat.status()
    finally:
        nat.set_path(nat.PATH_AUTO)


@pytest.mark.parametrize("family", ["per_bag", "grouped"])
@pytest.mark.parametrize("kind", ["weighted_sum", "padded_mean"])
@pytest.mark.parametrize("optimizer", ["EXACT_ADAGRAD", "ADAM"])
def test_captured_bags_train_like_the_eager_twin(ops, nat, optimizer, kind, family):
    """The same five steps with fused Adagrad and Adam against the eager module; a call without ids does not advance Adam's t."""
    a, b = _pair(ops, optimizer, KINDS[kind][2])
    try:
        _force(nat, b, family)
        cap = _capture(b, kind)
        rng = np.random.default_rng(2)
        for n, bags, i32 in STEPS:
            _twin_step(a, b, cap, kind, _call(rng, n, bags, kind, i32), rng, f"{kind}/{optimizer}/{family}")
            if optimizer == "ADAM":
                assert a.adam_steps() == b.adam_steps()
        if optimizer == "ADAM":
            assert b.adam_steps() == [len(STEPS) - 1]
        nat.status()
    finally:
        nat.set_path(nat.PATH_AUTO)


# 4. ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["weighted_sum", "max"])
def test_fixed_capture(ops, nat, kind):
    """``variable=False``: 256 ids in 80 ragged bags, every call exactly that size; two steps through the same graphs."""
    _, b = _pair(ops, "SGD", False)
    rng = np.random.default_rng(8)
    lens = rng.multinomial(256, np.ones(78) / 78)
    lens = np.concatenate([lens[:30], [0], lens[30:], [0]]).astype(np.int64)
    assert lens.size == 80 and lens.sum() == 256
    cap = _capture(b, kind, 256, 80, variable=False)
    assert cap.nnz_dev is None and cap.variable is False
    for step in range(2):
        ids = rng.integers(0, N_EMB, size=256).astype(np.int64)
        w = rng.standard_normal(256).astype(np.float32) if kind == "weighted_sum" else None
        offs = _dev(_offsets(lens))
        out = _sgd_step(ops, b, cap, kind, (_dev(ids), offs, None if w is None else _dev(w), offs), rng, f"fixed {kind}")
        assert out.data_ptr() == cap.output.data_ptr() and tuple(out.shape) == (80, D)
    with pytest.raises(ValueError, match="exactly"):
        cap(_dev(ids[:255]), offs, None if w is None else _dev(w[:255]))
    nat.status()


# 5. ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["weighted_sum", "padded_mean", "max"])
def test_exact_mode_equals_the_eager_twin_bit_for_bit(ops, nat, kind):
    """OptimType.EXACT_SGD with ``variable=False``: the graphs hold the exact kernels, and an exact-mode eager call takes the
    same masked rows, so output, weight gradient and cores are torch.equal.  ``variable=True`` is refused as capture() refuses it."""
    mode, weighted, padded, fanout = KINDS[kind]
    a, b = _pair(ops, "EXACT_SGD", padded)
    with pytest.raises(RuntimeError, match="exact mode.*no device id count"):
        _capture(b, kind, variable=True)
    rng = np.random.default_rng(12)
    lens = tv._ragged_lengths(rng, 300, 200)
    cap = _capture(b, kind, 300, lens.size, variable=False)
    assert cap.exact
    for step in range(2):
        ids = rng.integers(0, N_EMB, size=300).astype(np.int64)
        if padded:
            ids[rng.random(300) < 0.3] = PAD
            ids[0:lens[0]] = PAD
        offs, dy = _dev(_offsets(lens)), _dy(rng, lens.size)
        w = _dev(rng.standard_normal(300).astype(np.float32)) if weighted else None
        wa, wb = (None, None) if w is None else (w.clone().requires_grad_(True), w.clone().requires_grad_(True))
        out_a = a(_dev(ids), offs, per_sample_weights=wa, mode=mode)
        out_b = cap(_dev(ids), offs, wb)
        assert torch.equal(out_a.detach(), out_b.detach())
        out_a.backward(dy)
        out_b.backward(dy)
        torch.cuda.synchronize()
        if wa is not None:
            assert torch.equal(wa.grad, wb.grad)
        assert all(torch.equal(ca.data, cb.data) for ca, cb in zip(a.tt_cores, b.tt_cores))
        assert not torch.equal(b.tt_cores[1].data, torch.zeros_like(b.tt_cores[1].data))


# 6. ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["per_bag", "grouped"])
@pytest.mark.parametrize("kind", ["weighted_sum", "padded_max"])
def test_stale_buffers_are_never_read(ops, nat, kind, family):
    """After a full-capacity call every static buffer is filled with NaN; a 17-id ragged call then returns finite numbers that
    pass the checks of the training test, and the rows of ``d_output`` past the live bags still hold their NaN."""
    _, b = _pair(ops, "SGD", KINDS[kind][2])
    try:
        _force(nat, b, family)
        cap = _capture(b, kind)
        rng = np.random.default_rng(5)
        _sgd_step(ops, b, cap, kind, _call(rng, CAP, "long", kind), rng, f"{kind}/{family}")
        for t in (cap.output, cap.d_output, cap.rows, cap.d_rows, cap.weights, cap.d_weights, cap.pool_weights,
                  cap.d_weights_out):
            if t is not None:
                t.fill_(float("nan"))
        call = _call(rng, 17, "ragged", kind)
        out = _sgd_step(ops, b, cap, kind, call, rng, f"{kind}/{family}")
        assert bool(torch.isfinite(out).all())
        assert all(bool(torch.isfinite(c.data).all()) for c in b.tt_cores)
        assert bool(torch.isnan(cap.d_output[call[3].numel() - 1:]).all())
        nat.status()
    finally:
        nat.set_path(nat.PATH_AUTO)


# 7. ------------------------------------------------------------------------------------------------------------------
def test_the_first_position_wins_through_the_graphs(ops, nat):
    """A max bag that holds the same id twice: both positions carry the same values, the first one is the winner and alone
    receives ``d_rows`` -- the cores move as the eager twin's (two winners would move them twice as far), and a second replay
    of the same call returns the same bits.  One kernel family for both sides."""
    a, b = _pair(ops, "SGD", False)
    try:
        nat.set_path(nat.PATH_PER_BAG)
        cap = b.capture_bags(64, 16, mode="max", variable=True)
        ids = _dev(np.array([7, 7, 3, 9, 9, 9, 4, 11, 12, 12], dtype=np.int64))
        offs = _dev(np.array([0, 2, 3, 6, 6, 10], dtype=np.int64))
        rng = np.random.default_rng(1)
        dy = _dy(rng, 5)
        w0 = [c.detach().clone() for c in a.tt_cores]
        first = cap(ids, offs).detach().clone()
        out_a, out_b = a(ids, offs, mode="max"), cap(ids, offs)
        assert torch.equal(out_b.detach(), first)          # a second replay of the same call: the same bits
        torch.testing.assert_close(out_b.detach(), out_a.detach(), rtol=1e-5, atol=1e-4)
        out_a.backward(dy)
        out_b.backward(dy)
        torch.cuda.synchronize()
        for ca, cb, c0 in zip(a.tt_cores, b.tt_cores, w0):
            delta = float((ca.data - c0).abs().max())
            assert delta > 0
            print(f" core {float((cb.data - ca.data).abs().max()):.2e}/{delta:.1e}", end="")
            torch.testing.assert_close(cb.data, ca.data, rtol=0, atol=1e-5 + 1e-4 * delta)
        nat.status()
    finally:
        nat.set_path(nat.PATH_AUTO)


# 8. ------------------------------------------------------------------------------------------------------------------
def test_no_host_synchronisation(ops, nat):
    _, b = _pair(ops, "SGD", False)
    cap = _capture(b, "weighted_sum")
    rng = np.random.default_rng(6)
    ids, offs, w, offs_ref = _call(rng, 1000, "ragged", "weighted_sum")
    dy = _dy(rng, offs_ref.numel() - 1)
    wt = w.clone().requires_grad_(True)
    cap(ids, offs, wt).backward(dy)   # (first call: autograd's own set-up)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        cap(ids, offs, wt).backward(dy)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert wt.grad is not None and bool(torch.isfinite(wt.grad).all())


# 9. ------------------------------------------------------------------------------------------------------------------
def test_guards_raise_before_anything_is_launched(ops, nat):
    _, b = _pair(ops, "SGD", False)
    i64 = lambda *shape: torch.zeros(shape, dtype=torch.int64, device="cuda")
    f32 = lambda *shape: torch.ones(shape, dtype=torch.float32, device="cuda")
    plain = b.capture_bags(64, 32, mode="mean", variable=True)
    weighted = b.capture_bags(64, 32, weighted=True, variable=True)
    fan = b.capture_bags(64, 16, mode="mean", fanout=4, variable=True)
    before = [c.detach().clone() for c in b.tt_cores]
    staged = [t.clone() for t in (plain.indices, plain.offsets, plain.nnz_dev, weighted.weights, fan.offsets)]
    offs = torch.tensor([0, 3, 8], device="cuda")
    for cap, args, match in ((plain, (i64(8), offs, f32(8)), "weighted=False"),          # weights to an unweighted capture
                             (weighted, (i64(8), offs), "weighted=True"),                # none to a weighted one
                             (weighted, (i64(8), offs, f32(7)), "per_sample_weights"),   # weights of another shape
                             (plain, (i64(2, 4),), "2-D"),                               # 2-D without fanout
                             (fan, (i64(2, 3),), "fanout=4"),                            # a wrong second dimension
                             (fan, (i64(8),), "fanout=4"),                               # 1-D with fanout
                             (fan, (i64(2, 4), offs), "offsets"),                        # offsets with a 2-D call
                             (plain, (i64(65), torch.tensor([0, 65], device="cuda")), "nnz=64"),
                             (plain, (i64(40),), "B=32"),                                # bags of one: 40 bags
                             (fan, (i64(17, 4),), "nnz=64"),
                             (plain, (i64(10), torch.arange(34, device="cuda").clamp(max=10)), "B=32")):
        with pytest.raises(ValueError, match=match):
            cap(*args)
    b.padding_idx = 3
    with pytest.raises(RuntimeError, match="capture_bags\\(\\) again"):
        plain(i64(8), offs)
    b.padding_idx = None
    b.mode = "mean"
    with pytest.raises(RuntimeError, match="capture_bags\\(\\) again"):
        weighted(i64(8), offs, f32(8))
    b.mode = "sum"
    b.learning_rate = 0.5
    with pytest.raises(RuntimeError, match="capture_bags\\(\\) again"):
        plain(i64(8), offs)
    b.learning_rate = 0.1
    torch.cuda.synchronize()
    for t, t0 in zip((plain.indices, plain.offsets, plain.nnz_dev, weighted.weights, fan.offsets), staged):
        assert torch.equal(t, t0)          # nothing was staged
    assert all(torch.equal(c.detach(), c0) for c, c0 in zip(b.tt_cores, before))
    assert plain(i64(8), offs).shape == (2, D) and fan(i64(3, 4)).shape == (3, D)      # and the captures still serve
