"""Captured pooled lookups on the distinct ids of every call, on the GPU: ``emb.capture_bags(..., dedup=True)`` with the first
node of its route, ``ttemb_unique_ids_n``, and the pools that read a device id count, ``ttemb_bag_reduce_mapped_n`` /
``ttemb_bag_reduce_mapped_backward_n`` (include/ttemb_unique_n.h).

The pass is integer work: it is compared bit for bit with numpy (``np.unique(..., return_inverse=True)``, a stable argsort,
the run starts) and with ``ttemb_unique_ids`` run on the live part, sentinels around every range it may write.  The ``_n``
pools are compared bit for bit with their parents run on the live part.  The captured steps use the references and the
tolerances of test_gpu_capture_bags.py (its module docstring): SGD against ``F.embedding_bag`` over the full table -- forward
rtol 1e-5 / atol 1e-4, ``w.grad`` within 1e-4 of its largest magnitude and exactly 0 at a pad, cores within
1e-5 + 1e-4 max|lr g| --, Adagrad and Adam against the eager twin called with ``dedup=True`` within 1e-5 + 1e-4 max|delta|,
Adam's t equal.

Shapes are those of test_gpu_capture_variable.py: an 800-row table, D = 100, capacity 4096 (ids repeat about five times at
full size; the tile of the pass is 256 positions, the chunk of the pools 512).

Figures of the first run (max |captured - reference|) are printed by every test before it asserts."""
import gc
from unittest import mock

import numpy as np
import pytest
import torch

import test_gpu_capture_bags as tb
import test_gpu_capture_variable as tv

pytestmark = pytest.mark.gpu

N_EMB, D, CAP, PAD = tb.N_EMB, tb.D, tb.CAP, tb.PAD
SENTINEL, W_SENTINEL, I32_SENTINEL = tb.SENTINEL, tb.W_SENTINEL, -424242
COUNTS = (0, 1, 255, 256, 257, 1500, 4096)      # the tile is 256 positions: edges, mid-tile and the whole capacity
BADARG, WORKSPACE = -1, -2
# the unweighted sum: not among test_gpu_capture_bags.KINDS (its helpers look the kind up there)
EXTRA_KINDS = {"sum": ("sum", False, False, None)}
# (kind, pad_route): every kind the dedup route serves, the padded ones on both pad routes
SERVED = [("sum", None), ("mean", None), ("weighted_sum", None), ("padded_mean", "masked"), ("padded_mean", "partition"),
          ("fanout8_padded_mean", "masked"), ("fanout8_padded_mean", "partition"),
          ("fanout8_padded_weighted_sum", "masked"), ("fanout8_padded_weighted_sum", "partition")]
SERVED_IDS = [k if r is None else f"{k}-{r}" for k, r in SERVED]


@pytest.fixture(scope="module")
def nat():
    assert torch.cuda.is_available()
    import ttemb_native
    yield ttemb_native
    ttemb_native.set_exact_grid(0)


@pytest.fixture(scope="module")
def ops(nat):
    import FBTT.tt_embeddings_ops as m
    return m


@pytest.fixture(autouse=True)
def _kinds():
    with mock.patch.dict(tb.KINDS, EXTRA_KINDS):
        yield


_dev = tb._dev


# ---------------------------------------------------------------------------------------------------------------------
# 1. ttemb_unique_ids_n against numpy and against ttemb_unique_ids
# ---------------------------------------------------------------------------------------------------------------------
def _pass_ref(live):
    """(unique, inverse, perm, seg) of the live ids: np.unique, a stable argsort and the run starts."""
    uniq, inv = np.unique(live, return_inverse=True)
    perm = np.argsort(live, kind="stable")
    srt = live[perm]
    heads = np.flatnonzero(np.concatenate([[True], srt[1:] != srt[:-1]])) if live.size else np.zeros(0, dtype=np.int64)
    seg = np.concatenate([heads, [live.size]]).astype(np.int64)
    return uniq.astype(np.int64), inv.reshape(-1).astype(np.int32), perm.astype(np.int32), seg


def _pass_buffers(size):
    return (torch.full((size,), SENTINEL, dtype=torch.int64, device="cuda"),
            torch.full((size,), I32_SENTINEL, dtype=torch.int32, device="cuda"),
            torch.full((size,), I32_SENTINEL, dtype=torch.int32, device="cuda"),
            torch.full((size + 1,), SENTINEL, dtype=torch.int64, device="cuda"),
            torch.full((1,), I32_SENTINEL, dtype=torch.int32, device="cuda"))


def _run_pass(nat, ids, rows, c, counted):
    """The pass on the first c of ``ids``: with the count word on the whole buffer, or with NULL on buffers cut to c.
    Returns the five outputs as numpy, the sizes they were allocated with in front."""
    if counted:
        I, size, word = _dev(ids), ids.size, torch.tensor([c], dtype=torch.int32, device="cuda")
    else:
        I, size, word = _dev(ids[:c].copy()), c, None
    outs = _pass_buffers(size)
    nat.unique_ids_n(I, rows, *outs, nat.Workspace(), nnz_dev=word)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in outs]


def _check_pass(got, live, label):
    uniq, inv, perm, seg, count = got
    n = live.size
    want_u, want_inv, want_perm, want_seg = _pass_ref(live)
    U = want_u.size
    assert int(count[0]) == U, label
    assert np.array_equal(uniq[:U], want_u), label
    assert np.array_equal(inv[:n], want_inv), label
    assert np.array_equal(perm[:n], want_perm), label
    assert np.array_equal(seg[:U + 1], want_seg) and int(seg[U]) == n, label
    # what the contract says is not written holds its sentinels
    assert np.all(uniq[U:] == SENTINEL) and np.all(inv[n:] == I32_SENTINEL) and np.all(seg[U + 1:] == SENTINEL), label


def _stale_ids(rng, rows, c):
    """CAP ids: c live ones in [2, rows), then what earlier calls left -- an id smaller than every live one, and a block of
    one repeated id that is live, too.  Reading either would change the answer."""
    ids = rng.integers(2, rows, size=CAP).astype(np.int64)
    half = c + (CAP - c) // 2
    ids[c:half] = 0
    ids[half:] = ids[0] if c else 1
    return ids


@pytest.mark.parametrize("counted", [True, False], ids=["nnz_dev", "NULL"])
@pytest.mark.parametrize("c", COUNTS)
def test_unique_ids_n_against_numpy_and_unique_ids(nat, c, counted):
    rng = np.random.default_rng(100 + c)
    ids = _stale_ids(rng, N_EMB, c)
    live = ids[:c]
    outs = []
    try:
        for grid in (1, 0):
            nat.set_exact_grid(grid)
            got = _run_pass(nat, ids, N_EMB, c, counted)
            _check_pass(got, live, f"c={c} grid={grid}")
            outs.append(got)
    finally:
        nat.set_exact_grid(0)
    for a, b in zip(*outs):        # the grid decides who computes a word, never what it is (perm past the count included)
        assert np.array_equal(a, b)
    # the parent on the live part: bit for bit
    I = _dev(live.copy())
    parent = _pass_buffers(c)
    nat.unique_ids(I, N_EMB, *parent, nat.Workspace())
    torch.cuda.synchronize()
    U = int(parent[4].item())
    uniq, inv, perm, seg, count = outs[0]
    assert int(count[0]) == U
    for mine, theirs, k in ((uniq, parent[0], U), (inv, parent[1], c), (perm, parent[2], c), (seg, parent[3], U + 1)):
        assert np.array_equal(mine[:k], theirs.cpu().numpy()[:k])
    nat.status()


@pytest.mark.parametrize("rows", [1024, 1], ids=["power_of_two", "one_row"])
def test_unique_ids_n_at_the_edges_of_the_key_range(nat, rows):
    """``rows`` an exact power of two with ids at ``rows - 1`` (the dead key is one bit above them), and a table of one row
    (one key bit, every live id 0)."""
    rng = np.random.default_rng(7)
    c = 1500
    ids = rng.integers(0, rows, size=CAP).astype(np.int64)
    ids[:c:3] = rows - 1
    ids[c:] = rows - 1              # stale: the largest id of the table
    for counted in (True, False):
        _check_pass(_run_pass(nat, ids, rows, c, counted), ids[:c], f"rows={rows} counted={counted}")
    nat.status()


def test_unique_ids_n_refuses_bad_arguments_and_leaves_the_status_clean(nat):
    L = nat.LIB
    nnz, rows = 1000, 20677
    I = torch.randint(0, rows, (nnz,), device="cuda")
    uniq, inv, perm, seg, cnt = _pass_buffers(nnz)
    word = torch.tensor([600], dtype=torch.int32, device="cuda")
    need = nat.unique_ids_n_workspace_bytes(nnz, rows)
    assert need > 40960 + 2 * nnz * 8            # the keys and the sorted keys, then the tile counts and the sort's storage
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    p = lambda t: t.data_ptr()
    # (indices, nnz_cap, nnz_dev, rows, unique_out, inverse_out, perm_out, seg_out, count_dev, ws, ws_bytes, stream)
    good = [p(I), nnz, p(word), rows, p(uniq), p(inv), p(perm), p(seg), p(cnt), p(ws), need, None]
    for k, v in ((1, -1), (1, 2 ** 31), (3, 0), (0, None), (4, None), (5, None), (6, None), (7, None), (8, None), (9, None)):
        args = list(good)
        args[k] = v
        assert L.ttemb_unique_ids_n(*args) == BADARG, (k, v)
        assert b"ttemb_unique_ids_n" in L.ttemb_last_error()
    for nbytes in (16, 40960, need - 1):
        args = list(good)
        args[10] = nbytes
        assert L.ttemb_unique_ids_n(*args) == WORKSPACE, nbytes
    assert L.ttemb_unique_ids_n_workspace_bytes(-1, rows) == BADARG and L.ttemb_unique_ids_n_workspace_bytes(8, 0) == BADARG
    torch.cuda.synchronize()
    assert int(cnt) == I32_SENTINEL              # nothing was launched by any of it
    assert L.ttemb_unique_ids_n(*good) == 0
    torch.cuda.synchronize()
    nat.status()
    assert int(cnt) == np.unique(I[:600].cpu().numpy()).shape[0]


# ---------------------------------------------------------------------------------------------------------------------
# 2. the _n pools are the parents on the live part, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pool_case():
    """Capacity 4096: ragged bags with one bag of 1100 ids (it crosses the chunk edges 512 and 1024) that span the whole
    capacity, ids of which one holds every second position of [0, 2400) -- 750 of the first 1500 positions, 1200 in all: a
    segment of the sorted list that is summed in chunks for every count from 1500 on -- rows for every distinct id, weights
    and a gradient."""
    rng = np.random.default_rng(31)
    lens = tb._long_bag_lengths(rng, CAP)
    offs = tb._offsets(lens)
    ids = rng.integers(1, N_EMB, size=CAP).astype(np.int64)
    ids[:2400:2] = 0
    rows = rng.standard_normal((CAP, D)).astype(np.float32)
    w = rng.standard_normal(CAP).astype(np.float32)
    w[::11] = 0.0
    dy = ((rng.random((lens.size, D)) - 0.5) * 0.1).astype(np.float32)
    return dict(ids=ids, offs=offs, rows=_dev(rows), w=_dev(w), dy=_dev(dy), B=lens.size)


def _staged_offsets(offs, c):
    """What ttemb_stage_bags leaves for a call of c ids: the offsets clamped to c (every bag past the live ones is empty)."""
    return np.minimum(offs, c).astype(np.int64)


@pytest.mark.parametrize("weighted", [False, True], ids=["no_weights", "weights"])
@pytest.mark.parametrize("c", COUNTS)
def test_counted_mapped_pools_are_the_live_calls_bit_for_bit(nat, pool_case, c, weighted):
    x, ws = pool_case, nat.Workspace()
    B = x["B"]
    offs = _dev(_staged_offsets(x["offs"], c))
    word = torch.tensor([c], dtype=torch.int32, device="cuda")
    # the pass on the live ids (with the count word: its outputs past the count are sentinels, which the pools must not read)
    uniq, inv, perm, seg, cnt = _pass_buffers(CAP)
    nat.unique_ids_n(_dev(x["ids"]), N_EMB, uniq, inv, perm, seg, cnt, ws, nnz_dev=word)
    torch.cuda.synchronize()
    U = int(cnt.item())
    if c >= 1500:
        assert int((x["ids"][:c] == 0).sum()) > 512          # the segment that is summed in chunks
    w = x["w"] if weighted else None
    wl = None if w is None else w[:c]
    nan_tail = lambda t: torch.cat([t[:c], torch.full_like(t[c:], float("nan"))])
    w_n = None if w is None else nan_tail(w)                   # a weight past the count would poison the sums
    # forward
    out, want = tb._f((B, D)), tb._f((B, D))
    nat.bag_reduce_mapped(x["rows"], inv, w_n, offs, out, ws, nnz_dev=word, counted=True)
    if c:
        nat.bag_reduce_mapped(x["rows"], inv[:c], wl, offs, want, ws)
    else:
        want.zero_()
    torch.cuda.synchronize()
    assert torch.equal(out, want) and bool(torch.isfinite(out).all())
    # backward: d_rows[0:U] and d_weights[0:c], sentinels behind them
    d_rows, d_w = tb._f((CAP, D)), (tb._f((CAP,)) if weighted else None)
    r_rows, r_w = tb._f((CAP, D)), (tb._f((CAP,)) if weighted else None)
    nat.bag_reduce_mapped_backward(x["dy"], w_n, inv, perm, seg, cnt, offs, d_rows, ws, rows=x["rows"] if weighted else None,
                                   d_weights=d_w, nnz_dev=word, counted=True)
    if c:
        nat.bag_reduce_mapped_backward(x["dy"], wl, inv[:c], perm[:c], seg[:c + 1], cnt, offs, r_rows[:c], ws,
                                       rows=x["rows"][:c] if weighted else None, d_weights=None if r_w is None else r_w[:c])
    torch.cuda.synchronize()
    assert torch.equal(d_rows[:U], r_rows[:U]) and bool((d_rows[U:] == W_SENTINEL).all())
    assert bool(torch.isfinite(d_rows[:U]).all())
    if weighted:
        assert torch.equal(d_w[:c], r_w[:c]) and bool((d_w[c:] == W_SENTINEL).all())
    # nnz_dev = NULL through the new entry points: the parents at full size
    if c == CAP:
        out2, d_rows2 = tb._f((B, D)), tb._f((CAP, D))
        nat.bag_reduce_mapped(x["rows"], inv, w, offs, out2, ws, nnz_dev=None, counted=True)
        nat.bag_reduce_mapped_backward(x["dy"], w, inv, perm, seg, cnt, offs, d_rows2, ws, counted=True)
        torch.cuda.synchronize()
        assert torch.equal(out2, want) and torch.equal(d_rows2[:U], r_rows[:U])
    nat.status()


# ---------------------------------------------------------------------------------------------------------------------
# 3. captured steps against the references
# ---------------------------------------------------------------------------------------------------------------------
def _capture(b, kind, pad_route=None, nnz=CAP, B=CAP, variable=True):
    mode, weighted, padded, fanout = tb.KINDS[kind]
    if fanout:
        B = nnz // fanout
    cap = b.capture_bags(nnz, B, mode=mode, weighted=weighted, fanout=fanout, variable=variable, pad_route=pad_route, dedup=True)
    assert cap.route == "dedup" and cap.dedup is True
    assert cap.pad_route == (pad_route if padded else None)
    for t, dtype, size in ((cap.uids, torch.int64, nnz), (cap.inverse, torch.int32, nnz), (cap.perm, torch.int32, nnz),
                           (cap.seg, torch.int64, nnz + 1), (cap.unique_count, torch.int32, 1)):
        assert t.dtype == dtype and t.numel() == size
    assert tuple(cap.rows.shape) == (nnz, D) and tuple(cap.d_rows.shape) == (nnz, D)
    return cap


def _distinct(ids, kind, pad_route):
    """How many ids the TT kernels look up: the distinct ones, without the pad where the pads are compacted away."""
    flat = ids.reshape(-1).cpu().numpy()
    if tb.KINDS[kind][2] and pad_route == "partition":
        flat = flat[flat != PAD]
    return np.unique(flat).size


def _sgd_step(ops, b, cap, kind, call, rng, label):
    """test_gpu_capture_bags._sgd_step, plus: the weight gradient is exactly 0 at the pad positions, and the count word
    holds the number of distinct ids."""
    mode, weighted, padded, fanout = tb.KINDS[kind]
    ids, offs, w, offs_ref = call
    n, B_live = ids.numel(), offs_ref.numel() - 1
    if n == 0:
        return tb._no_id_step(b, cap, ids, offs, w, B_live)
    lr = float(b.learning_rate)
    w0 = [c.detach().clone() for c in b.tt_cores]
    want, grads, wgrad, dy = tb._reference(ops, b, ids.reshape(-1).long(), offs_ref, mode, None if w is None else w.reshape(-1),
                                           tb._dy(rng, B_live), PAD if padded else None)
    wt = None if w is None else w.clone().requires_grad_(True)
    out = cap(ids, offs, wt)
    assert tuple(out.shape) == (B_live, D)
    print(f"\n  {label} n={n:5d} bags={B_live:5d} out {float((out.detach() - want).abs().max()):.2e}", end="")
    torch.testing.assert_close(out.detach(), want, rtol=1e-5, atol=1e-4)
    assert int(cap.unique_count.item()) == _distinct(ids, kind, cap.pad_route)
    out.backward(dy)
    torch.cuda.synchronize()
    if wt is not None:
        got, ref = wt.grad.reshape(-1), wgrad
        print(f" w.grad {float((got - ref).abs().max()):.2e} of {float(ref.abs().max()):.2e}", end="")
        torch.testing.assert_close(got, ref, rtol=0, atol=1e-4 * max(float(ref.abs().max()), 1e-6))
        if padded:
            at_pads = got[ids.reshape(-1) == PAD]
            assert at_pads.numel() > 0 and bool((at_pads == 0).all())
    for c, c0, g in zip(b.tt_cores, w0, grads):
        print(f" core {float((c.detach() - (c0 - lr * g)).abs().max()):.2e}", end="")
        torch.testing.assert_close(c.detach(), c0 - lr * g, rtol=0, atol=1e-5 + 1e-4 * float((lr * g).abs().max()))
    return out


def _twin_step(a, b, cap, kind, call, rng, label):
    """test_gpu_capture_bags._twin_step with the eager twin on ITS dedup route."""
    mode, weighted, padded, fanout = tb.KINDS[kind]
    ids, offs, w, offs_ref = call
    n, B_live = ids.numel(), offs_ref.numel() - 1
    if n == 0:
        return tb._no_id_step(b, cap, ids, offs, w, B_live)
    dy = tb._dy(rng, B_live)
    before = [t.detach().clone() for t in tb._tensors(a)]
    wa, wb = (None, None) if w is None else (w.clone().requires_grad_(True), w.clone().requires_grad_(True))
    out_a = a(ids.long(), None if fanout else offs_ref, per_sample_weights=wa, mode=mode, dedup=True)
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
    for ta, tb_, t0 in zip(tb._tensors(a), tb._tensors(b), before):
        if ta.dtype == torch.int32:     # Adam's step words: t itself must be equal
            assert int(ta[0, 0]) == int(tb_[0, 0])
            continue
        delta = float((ta.detach() - t0).abs().max())
        print(f" {float((tb_.detach() - ta.detach()).abs().max()):.2e}/{delta:.1e}", end="")
        torch.testing.assert_close(tb_.detach(), ta.detach(), rtol=0, atol=1e-5 + 1e-4 * delta)
    return out_b


@pytest.mark.parametrize("family", ["per_bag", "grouped"])
@pytest.mark.parametrize("kind,pad_route", SERVED, ids=SERVED_IDS)
def test_captured_dedup_bags_train_like_the_reference_sgd(ops, nat, kind, pad_route, family):
    """The five SGD steps of test_gpu_capture_bags.STEPS -- 4096 ids (with the 1100-id bag) -> 1000 (ragged, int32) -> 17 -> 0
    -> 4095 bags of one without offsets -- through ONE pair of graphs captured at capacity 4096 with ``dedup=True``."""
    _, b = tb._pair(ops, "SGD", tb.KINDS[kind][2])
    try:
        tb._force(nat, b, family)
        cap = _capture(b, kind, pad_route)
        rng = np.random.default_rng(2)
        for n, bags, i32 in tb.STEPS:
            _sgd_step(ops, b, cap, kind, tb._call(rng, n, bags, kind, i32), rng, f"{kind}/{pad_route}/{family}")
        nat.status()
    finally:
        nat.set_path(nat.PATH_AUTO)


@pytest.mark.parametrize("family", ["per_bag", "grouped"])
@pytest.mark.parametrize("kind,pad_route", [("mean", None), ("weighted_sum", None), ("padded_mean", "masked"),
                                            ("fanout8_padded_weighted_sum", "partition")],
                         ids=["mean", "weighted_sum", "padded_mean-masked", "fanout8_padded_weighted_sum-partition"])
@pytest.mark.parametrize("optimizer", ["EXACT_ADAGRAD", "ADAM"])
def test_captured_dedup_bags_train_like_the_eager_dedup_twin(ops, nat, optimizer, kind, pad_route, family):
    """The same five steps with fused Adagrad and Adam against the eager module called with ``dedup=True``; a call without ids
    does not advance Adam's t."""
    a, b = tb._pair(ops, optimizer, tb.KINDS[kind][2])
    try:
        tb._force(nat, b, family)
        cap = _capture(b, kind, pad_route)
        rng = np.random.default_rng(2)
        for n, bags, i32 in tb.STEPS:
            _twin_step(a, b, cap, kind, tb._call(rng, n, bags, kind, i32), rng, f"{kind}/{optimizer}/{family}")
            if optimizer == "ADAM":
                assert a.adam_steps() == b.adam_steps()
        if optimizer == "ADAM":
            assert b.adam_steps() == [len(tb.STEPS) - 1]
        nat.status()
    finally:
        nat.set_path(nat.PATH_AUTO)


@pytest.mark.parametrize("kind,pad_route", [("mean", None), ("padded_mean", "partition"), ("weighted_sum", None)],
                         ids=["mean", "padded_mean-partition", "weighted_sum"])
def test_fixed_capture(ops, nat, kind, pad_route):
    """``variable=False``: 256 ids in 80 ragged bags, every call exactly that size; the pass reads no count word, or (partition)
    the kept count.  Two steps through the same graphs."""
    padded = tb.KINDS[kind][2]
    _, b = tb._pair(ops, "SGD", padded)
    rng = np.random.default_rng(8)
    lens = rng.multinomial(256, np.ones(78) / 78)
    lens = np.concatenate([lens[:30], [0], lens[30:], [0]]).astype(np.int64)
    assert lens.size == 80 and lens.sum() == 256
    offs_np = tb._offsets(lens)
    cap = _capture(b, kind, pad_route, 256, 80, variable=False)
    assert cap.nnz_dev is None and cap.variable is False
    for step in range(2):
        ids = rng.integers(0, N_EMB // 8, size=256).astype(np.int64)      # (100 rows: most ids come more than once)
        if padded:
            ids[rng.random(256) < 0.3] = PAD
        w = rng.standard_normal(256).astype(np.float32) if tb.KINDS[kind][1] else None
        offs = _dev(offs_np)
        out = _sgd_step(ops, b, cap, kind, (_dev(ids), offs, None if w is None else _dev(w), offs), rng, f"fixed {kind}")
        assert out.data_ptr() == cap.output.data_ptr() and tuple(out.shape) == (80, D)
    nat.status()


@pytest.mark.parametrize("family", ["per_bag", "grouped"])
@pytest.mark.parametrize("kind", ["sum", "mean"])
def test_all_distinct_and_one_repeated_id(ops, nat, kind, family):
    """800 ids that are all distinct (U = n: the map is a permutation), then 1000 positions of ONE id (U = 1: a segment of
    1000 positions, summed in two chunks), ragged bags both."""
    _, b = tb._pair(ops, "SGD", False)
    try:
        tb._force(nat, b, family)
        cap = _capture(b, kind)
        rng = np.random.default_rng(12)
        for ids in (rng.permutation(N_EMB).astype(np.int64), np.full(1000, 37, dtype=np.int64)):
            offs = _dev(tb._offsets(tv._ragged_lengths(rng, ids.size, CAP)))
            _sgd_step(ops, b, cap, kind, (_dev(ids), offs, None, offs), rng, f"{kind}/{family}")
            assert int(cap.unique_count.item()) == (N_EMB if ids.size == N_EMB else 1)
        nat.status()
    finally:
        nat.set_path(nat.PATH_AUTO)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the TT kernels see distinct ids only
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["per_bag", "grouped"])
@pytest.mark.parametrize("kind,pad_route", [("mean", None), ("padded_mean", "masked"), ("padded_mean", "partition"),
                                            ("weighted_sum", None)],
                         ids=["mean", "padded_mean-masked", "padded_mean-partition", "weighted_sum"])
def test_the_tt_kernels_see_distinct_ids_only(ops, nat, kind, pad_route, family):
    """After a full-capacity call every static buffer is filled with NaN or a sentinel; a 1000-id ragged call then passes the
    checks of the training test, the count word holds the numpy count, and no row past it was written in ``rows`` /
    ``d_rows`` -- the lookup and its backward ran on the distinct ids alone.  The grouped family writes nothing past the
    count (a bag of one has exactly one writer, its id).  The per-bag forward walks all ``nnz`` bags of one and stores zeros
    for those the count leaves empty, as it does for every captured lookup: there ``rows[U:]`` is exactly 0 -- no row was
    looked up -- and ``d_rows[U:]`` still holds its sentinel."""
    _, b = tb._pair(ops, "SGD", tb.KINDS[kind][2])
    try:
        tb._force(nat, b, family)
        cap = _capture(b, kind, pad_route)
        rng = np.random.default_rng(5)
        _sgd_step(ops, b, cap, kind, tb._call(rng, CAP, "long", kind), rng, f"{kind}/{family}")
        for t in (cap.output, cap.d_output, cap.d_sums, cap.rows, cap.d_rows, cap.weights, cap.weights_k, cap.pool_weights,
                  cap.d_weights, cap.d_weights_out):
            if t is not None:
                t.fill_(float("nan"))
        cap.uids.fill_(SENTINEL)
        cap.seg.fill_(SENTINEL)
        cap.inverse.fill_(0)          # (a valid row: a read past the count would bring rows[0] along)
        call = tb._call(rng, 1000, "ragged", kind)
        out = _sgd_step(ops, b, cap, kind, call, rng, f"{kind}/{family}")
        U = _distinct(call[0], kind, pad_route)
        assert int(cap.unique_count.item()) == U and 0 < U < 1000
        assert bool(torch.isfinite(out).all()) and all(bool(torch.isfinite(c.data).all()) for c in b.tt_cores)
        assert bool(torch.isfinite(cap.rows[:U]).all())
        assert bool((torch.isnan(cap.rows[U:]) if family == "grouped" else cap.rows[U:] == 0).all())
        assert bool(torch.isfinite(cap.d_rows[:U]).all()) and bool(torch.isnan(cap.d_rows[U:]).all())
        assert bool((cap.uids[U:] == SENTINEL).all()) and bool((cap.seg[U + 1:] == SENTINEL).all())
        kept = int((call[0] != PAD).sum()) if pad_route == "partition" else call[0].numel()
        assert bool((cap.inverse[kept:] == 0).all())
        nat.status()
    finally:
        nat.set_path(nat.PATH_AUTO)


# ---------------------------------------------------------------------------------------------------------------------
# 5. a replay synchronises nothing and allocates nothing
# ---------------------------------------------------------------------------------------------------------------------
def test_no_host_synchronisation_and_no_allocation(ops, nat):
    _, b = tb._pair(ops, "SGD", True)
    cap = _capture(b, "padded_mean", "partition")
    rng = np.random.default_rng(6)
    ids, offs, w, offs_ref = tb._call(rng, 1000, "ragged", "padded_mean")
    dy = tb._dy(rng, offs_ref.numel() - 1)
    for _ in range(2):            # (the first calls: autograd's own set-up, and what it lets go of)
        cap(ids, offs).backward(dy)
    torch.cuda.synchronize()
    gc.collect()
    before = torch.cuda.memory_allocated()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(10):
            cap(ids, offs).backward(dy)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before
    assert all(bool(torch.isfinite(c.data).all()) for c in b.tt_cores)
    nat.status()


# ---------------------------------------------------------------------------------------------------------------------
# 6. refusals, and the two routes side by side
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_raise_before_anything_is_launched(ops, nat):
    _, b = tb._pair(ops, "SGD", False)
    with pytest.raises(ValueError, match="dedup with mode='max'"):
        b.capture_bags(64, 32, mode="max", variable=True, dedup=True)
    with pytest.raises(ValueError, match="2\\^20 ids"):
        b.capture_bags((1 << 20) + 1, 32, mode="mean", variable=True, dedup=True)
    _, exact = tb._pair(ops, "EXACT_SGD", False)
    with pytest.raises(RuntimeError, match="exact mode.*no device id count"):
        exact.capture_bags(64, 32, mode="mean", variable=False, dedup=True)
    assert exact.capture_bags(64, 32, mode="mean", variable=False).route == "mean"      # without the keyword: as before
    _, on = tb._pair(ops, "SGD", False, dedup=True)
    with pytest.raises(ValueError, match=r"capture_bags\(\) on a dedup=True module"):
        on.capture_bags(64, 32, mode="mean", dedup=True)
    with pytest.raises(TypeError):
        b.capture_bags(64, 32, "mean", False, None, True, None, True)      # keyword-only
    cached = ops.TTEmbeddingBag(N_EMB, D, tb.R, tb.P, tb.Q, sparse=True, use_cache=True, cache_size=10, hashtbl_size=40)
    cached.warmup = False           # (what cache_populate() leaves)
    with pytest.raises(RuntimeError, match="live row cache"):
        cached.capture_bags(64, 32, mode="mean", dedup=True)
    plain = b.capture_bags(64, 32, mode="mean", variable=True)              # today's graphs, untouched by the keyword
    assert plain.route == "mean" and plain.dedup is False and plain.uids is None and plain.rows is None


@pytest.mark.parametrize("kind", ["mean", "weighted_sum"])
def test_two_captures_with_and_without_dedup_agree(ops, nat, kind):
    """One module, two captures: the same call through both gives results within the forward tolerance of each other, and the
    same step from the same cores ends within the core tolerance (1e-5 + 1e-4 max|delta|)."""
    mode, weighted, _, _ = tb.KINDS[kind]
    _, b = tb._pair(ops, "SGD", False)
    plain = b.capture_bags(CAP, CAP, mode=mode, weighted=weighted, variable=True)
    dedup = _capture(b, kind)
    rng = np.random.default_rng(4)
    ids, offs, w, offs_ref = tb._call(rng, 1000, "ragged", kind)
    dy = tb._dy(rng, offs_ref.numel() - 1)
    start = [c.detach().clone() for c in b.tt_cores]
    ends, outs = [], []
    for cap in (plain, dedup):
        with torch.no_grad():
            for c, c0 in zip(b.tt_cores, start):
                c.copy_(c0)
        out = cap(ids, offs, w)
        outs.append(out.detach().clone())
        out.backward(dy)
        torch.cuda.synchronize()
        ends.append([c.detach().clone() for c in b.tt_cores])
    print(f"\n  {kind} out {float((outs[0] - outs[1]).abs().max()):.2e}", end="")
    torch.testing.assert_close(outs[1], outs[0], rtol=1e-5, atol=1e-4)
    for c0, ca, cb in zip(start, *ends):
        delta = float((ca - c0).abs().max())
        print(f" core {float((cb - ca).abs().max()):.2e}/{delta:.1e}", end="")
        torch.testing.assert_close(cb, ca, rtol=0, atol=1e-5 + 1e-4 * delta)
    nat.status()
