"""Captured padded bags on the partition route, on the GPU: ``emb.capture_bags(..., pad_route="partition")`` with its first
graph node ``ttemb_compact_bags`` and the way back of the weight gradient, ``ttemb_expand_kept``.

The two kernels are integer and copy work: they are compared with a numpy restatement bit for bit, sentinels around every
range they may write, and with ``ttemb_drop_padding`` run on the live part.  The captured steps use the references and the
tolerances of test_gpu_capture_bags.py (its module docstring): SGD against ``F.embedding_bag(padding_idx=)`` over the full
table -- forward rtol 1e-5 / atol 1e-4, ``w.grad`` within 1e-4 of its largest magnitude and exactly 0 at a pad, cores within
1e-5 + 1e-4 max|lr g| --, Adagrad and Adam against the eager twin within 1e-5 + 1e-4 max|delta|, Adam's t equal.

The all-pad call (every id of a call is the pad, which the host cannot know): the backward graph replays with a kept count
of 0.  Every kernel of the lookups stops at that count (``live_count``) or works from the group counters the decode step
filled from it, so no core row gets a gradient and the dense SGD / Adagrad step runs on g = 0 -- the state a table-batched
window without ids leaves, which test_gpu_parity.py already holds to zero gradients.  Tested here for SGD and Adagrad; Adam
takes a step on g = 0 there and is not part of that test.

Figures of the first run (max |captured - reference|) are printed by every test before it asserts."""
import gc
import weakref
from unittest import mock

import numpy as np
import pytest
import torch

import test_gpu_capture_bags as tb
import test_gpu_capture_variable as tv

pytestmark = pytest.mark.gpu

N_EMB, D, CAP, PAD = tb.N_EMB, tb.D, tb.CAP, tb.PAD
SENTINEL, W_SENTINEL, MAP_SENTINEL = tb.SENTINEL, tb.W_SENTINEL, -424242
COUNTS = (0, 1, 255, 256, 257, 1500, 4096)      # the tile is 256 positions: edges, mid-tile and the whole capacity
# the 1-D weighted padded call: not among test_gpu_capture_bags.KINDS (its helpers look the kind up there)
EXTRA_KINDS = {"padded_weighted_sum": ("sum", True, True, None)}
ROUTES = {"padded_sum": "plain", "padded_mean": "mean", "fanout8_padded_mean": "mean", "padded_max": "rows",
          "fanout8_padded_weighted_sum": "rows", "padded_weighted_sum": "rows"}


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


@pytest.fixture(autouse=True)
def _kinds():
    with mock.patch.dict(tb.KINDS, EXTRA_KINDS):
        yield


_dev = tb._dev


# ---------------------------------------------------------------------------------------------------------------------
# 1. ttemb_compact_bags against numpy and against ttemb_drop_padding
# ---------------------------------------------------------------------------------------------------------------------
def _layout(rng):
    """Bags over all 4096 positions: ragged bags with empty ones up to a bag edge exactly at 256, more up to an edge exactly
    at 512, 300 empty bags that all start at 512 (the offsets loop strides by 256), a few short bags, one bag of 1100 ids
    (it crosses four tile edges), ragged bags for the rest.  Returns (offsets, a non-empty bag to fill with pads)."""
    lens = [*tv._ragged_lengths(rng, 256, 200), *tv._ragged_lengths(rng, 256, 200), *([0] * 300),
            *tv._ragged_lengths(rng, 38, 40), 1100, *tv._ragged_lengths(rng, CAP - 512 - 38 - 1100, 2000)]
    offs = tb._offsets(np.asarray(lens, dtype=np.int64))
    assert offs[-1] == CAP and 256 in offs and 512 in offs and int((offs == 512).sum()) > 256
    assert int(np.flatnonzero(np.diff(offs) == 1100)[0]) > 0
    pads_only = int(np.flatnonzero(np.diff(offs) > 1)[3])      # (inside the first tile)
    return offs, pads_only


def _staged(offs, c):
    """The offsets as ttemb_stage_bags leaves them for a call of the first c ids: the bags that end at or before c, one more
    up to c, and c in every word behind them."""
    live = offs[offs <= c]
    out = np.full(offs.size, c, dtype=np.int64)
    out[:live.size] = live
    return out


def _compact_ref(ids, offs, w, c, pad):
    """numpy restatement of ttemb_compact_bags: (kept ids, their weights, offsets_out, map[:c], kept)."""
    o = np.clip(offs, 0, c)
    n = np.arange(c)
    keep = (n >= o[0]) & (n < o[-1]) & (ids[:c] != pad)
    before = np.concatenate([[0], np.cumsum(keep)]).astype(np.int64)
    return (ids[:c][keep], None if w is None else w[:c][keep], before[o], np.where(keep, before[:-1], -1).astype(np.int32),
            int(keep.sum()))


@pytest.fixture(scope="module")
def compact_inputs():
    rng = np.random.default_rng(31)
    offs, pads_only = _layout(rng)
    ids = rng.integers(0, N_EMB, size=CAP).astype(np.int64)
    ids[rng.random(CAP) < 0.3] = PAD
    ids[offs[pads_only]:offs[pads_only + 1]] = PAD
    ids[7], ids[300] = -3, 2 ** 40 + PAD            # (the RAW id is compared: neither is the pad)
    w = rng.standard_normal(CAP).astype(np.float32)
    w[::13] = 0.0
    assert 0.2 < float((ids == PAD).mean()) < 0.4
    return ids, offs, w


@pytest.mark.parametrize("counted", [True, False], ids=["nnz_dev", "NULL"])
@pytest.mark.parametrize("layout", ["full", "staged", "inner"])
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weights"])
def test_compact_bags_against_numpy_and_drop_padding(nat, compact_inputs, weighted, layout, counted):
    """Every live count at capacity 4096 (``NULL``: the buffers cut to the count, the capacity IS the count).  ``full``: the
    offsets span the capacity and are clamped to the count; ``staged``: as staging leaves them, the count in every word of
    the tail; ``inner``: offsets[0] > 0 and offsets[B] short of the count -- positions outside every bag are dropped."""
    ids0, offs0, w0 = compact_inputs
    ws = nat.Workspace()
    for c in COUNTS:
        cap = CAP if counted else c
        offs = offs0 if layout == "full" else _staged(offs0, c)
        if layout == "inner":
            offs = np.clip(offs, min(3, c), max(c - 5, min(3, c)))
        ids, w = ids0[:cap].copy(), w0[:cap].copy()
        ids[c:], w[c:] = 777, np.nan                  # behind the count: ids that would be kept, weights that would show
        want_ids, want_w, want_offs, want_map, kept = _compact_ref(ids, offs, w if weighted else None, c, PAD)
        t_ids, t_offs, t_w = _dev(ids), _dev(offs), (_dev(w) if weighted else None)
        ids_k = torch.full((cap,), SENTINEL, dtype=torch.int64, device="cuda")
        offs_k = torch.full((offs.size,), SENTINEL, dtype=torch.int64, device="cuda")
        w_k = tb._f((cap,)) if weighted else None
        map_k = torch.full((cap,), MAP_SENTINEL, dtype=torch.int32, device="cuda")
        kept_dev = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        cnt = torch.tensor([c], dtype=torch.int32, device="cuda") if counted else None
        nat.compact_bags(t_ids, t_offs, t_w, PAD, ids_k, offs_k, w_k, map_k, kept_dev, ws, nnz_dev=cnt)
        torch.cuda.synchronize()
        what = (c, layout, kept)
        assert int(kept_dev.item()) == kept, what
        assert np.array_equal(ids_k[:kept].cpu().numpy(), want_ids), what
        assert bool((ids_k[kept:] == SENTINEL).all()), (what, "indices_out past the kept count")
        assert np.array_equal(offs_k.cpu().numpy(), want_offs), what
        assert np.array_equal(map_k[:c].cpu().numpy(), want_map), what
        assert bool((map_k[c:] == MAP_SENTINEL).all()), (what, "map_out past the count")
        if weighted:
            assert np.array_equal(w_k[:kept].cpu().numpy().view(np.int32), want_w.view(np.int32)), what
            assert bool((w_k[kept:] == W_SENTINEL).all()), (what, "weights_out past the kept count")
        # ttemb_drop_padding on the live part: the same kept ids, bags and count
        d_ids, d_rows = torch.empty(c, dtype=torch.int64, device="cuda"), torch.empty(c, dtype=torch.int64, device="cuda")
        d_offs, d_kept = torch.empty_like(offs_k), torch.empty_like(kept_dev)
        nat.drop_padding(t_ids[:c], t_offs, PAD, d_ids, d_rows, d_offs, d_kept, ws)
        assert torch.equal(d_kept, kept_dev) and torch.equal(d_offs, offs_k), what
        assert torch.equal(d_ids[:kept], ids_k[:kept]), what


# ---------------------------------------------------------------------------------------------------------------------
# 2. ttemb_expand_kept against numpy
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counted", [True, False], ids=["nnz_dev", "NULL"])
def test_expand_kept_against_numpy(nat, compact_inputs, counted):
    ids, offs, _ = compact_inputs
    rng = np.random.default_rng(32)
    for c in COUNTS:
        cap = CAP if counted else c
        _, _, _, m, kept = _compact_ref(ids, offs, None, c, PAD)
        src = rng.standard_normal(cap).astype(np.float32)
        src[kept:] = np.nan                              # (past the kept count: nothing of it may arrive)
        full_map = np.full(cap, 0, dtype=np.int32)       # (behind the count: a valid place, so a read past it would show)
        full_map[:c] = m
        out = tb._f((cap,))
        cnt = torch.tensor([c], dtype=torch.int32, device="cuda") if counted else None
        nat.expand_kept(_dev(src), _dev(full_map), out, nnz_dev=cnt)
        torch.cuda.synchronize()
        want = np.where(m >= 0, src[np.maximum(m, 0)], np.float32(0)).astype(np.float32)
        got = out.cpu().numpy()
        assert np.array_equal(got[:c].view(np.int32), want.view(np.int32)), c
        assert bool((got[:c][m < 0].view(np.int32) == 0).all()) and bool(np.isfinite(got[:c]).all()), c
        assert bool((got[c:] == W_SENTINEL).all()), (c, "out past the count")


# ---------------------------------------------------------------------------------------------------------------------
# captured steps
# ---------------------------------------------------------------------------------------------------------------------
def _capture(b, kind, nnz=CAP, B=CAP, variable=True):
    mode, weighted, padded, fanout = tb.KINDS[kind]
    if fanout:
        B = nnz // fanout
    cap = b.capture_bags(nnz, B, mode=mode, weighted=weighted, fanout=fanout, variable=variable, pad_route="partition")
    assert cap.pad_route == "partition" and cap.route == ROUTES[kind]
    if ROUTES[kind] != "rows":      # the two [nnz, D] buffers of the masked route are not there
        assert cap.rows is None and cap.d_rows is None
    return cap


def _sgd_step(ops, b, cap, kind, call, rng, label):
    """test_gpu_capture_bags._sgd_step, plus: the weight gradient is exactly 0 at the pad positions."""
    mode, weighted, padded, fanout = tb.KINDS[kind]
    ids, offs, w, offs_ref = call
    n, B_live = ids.numel(), offs_ref.numel() - 1
    if n == 0:
        return tb._no_id_step(b, cap, ids, offs, w, B_live)
    lr = float(b.learning_rate)
    w0 = [c.detach().clone() for c in b.tt_cores]
    want, grads, wgrad, dy = tb._reference(ops, b, ids.reshape(-1).long(), offs_ref, mode, None if w is None else w.reshape(-1),
                                           tb._dy(rng, B_live), PAD)
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
        at_pads = got[ids.reshape(-1) == PAD]
        assert at_pads.numel() > 0 and bool((at_pads == 0).all())
    for c, c0, g in zip(b.tt_cores, w0, grads):
        print(f" core {float((c.detach() - (c0 - lr * g)).abs().max()):.2e}", end="")
        torch.testing.assert_close(c.detach(), c0 - lr * g, rtol=0, atol=1e-5 + 1e-4 * float((lr * g).abs().max()))
    return out


# 3. ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["per_bag", "grouped"])
@pytest.mark.parametrize("kind", list(ROUTES))
def test_partitioned_bags_train_like_the_reference_sgd(ops, nat, kind, family):
    """The five SGD steps of test_gpu_capture_bags.STEPS -- 4096 ids (with the 1100-id bag) -> 1000 (ragged, int32) -> 17 -> 0
    -> 4095 bags of one -- through ONE pair of graphs captured at capacity 4096 with ``pad_route="partition"``; every call
    has about 30 % pads and one bag of pads only."""
    _, b = tb._pair(ops, "SGD", True)
    try:
        tb._force(nat, b, family)
        cap = _capture(b, kind)
        rng = np.random.default_rng(2)
        for n, bags, i32 in tb.STEPS:
            _sgd_step(ops, b, cap, kind, tb._call(rng, n, bags, kind, i32), rng, f"{kind}/{family}")
        nat.status()
    finally:
        nat.set_path(nat.PATH_AUTO)


@pytest.mark.parametrize("family", ["per_bag", "grouped"])
@pytest.mark.parametrize("kind", ["padded_mean", "padded_weighted_sum"])
@pytest.mark.parametrize("optimizer", ["EXACT_ADAGRAD", "ADAM"])
def test_partitioned_bags_train_like_the_eager_twin(ops, nat, optimizer, kind, family):
    """The same five steps with fused Adagrad and Adam against the eager module; a call without ids does not advance Adam's t."""
    a, b = tb._pair(ops, optimizer, True)
    try:
        tb._force(nat, b, family)
        cap = _capture(b, kind)
        rng = np.random.default_rng(2)
        for n, bags, i32 in tb.STEPS:
            tb._twin_step(a, b, cap, kind, tb._call(rng, n, bags, kind, i32), rng, f"{kind}/{optimizer}/{family}")
            if optimizer == "ADAM":
                assert a.adam_steps() == b.adam_steps()
        if optimizer == "ADAM":
            assert b.adam_steps() == [len(tb.STEPS) - 1]
        nat.status()
    finally:
        nat.set_path(nat.PATH_AUTO)


# 4. ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["padded_mean", "padded_weighted_sum"])
def test_fixed_capture(ops, nat, kind):
    """``variable=False``: 256 ids in 80 ragged bags, every call exactly that size; the compaction reads no count word
    (``nnz_dev = NULL``), everything behind it the kept count.  Two steps through the same graphs."""
    _, b = tb._pair(ops, "SGD", True)
    rng = np.random.default_rng(8)
    lens = rng.multinomial(256, np.ones(78) / 78)
    lens = np.concatenate([lens[:30], [0], lens[30:], [0]]).astype(np.int64)
    assert lens.size == 80 and lens.sum() == 256
    offs_np = tb._offsets(lens)
    cap = _capture(b, kind, 256, 80, variable=False)
    assert cap.nnz_dev is None and cap.variable is False and cap.kept_dev is not None
    for step in range(2):
        ids = rng.integers(0, N_EMB, size=256).astype(np.int64)
        ids[rng.random(256) < 0.3] = PAD
        first = int(np.flatnonzero(lens > 0)[0])
        ids[offs_np[first]:offs_np[first + 1]] = PAD        # one bag of pads only
        w = rng.standard_normal(256).astype(np.float32) if kind == "padded_weighted_sum" else None
        offs = _dev(offs_np)
        out = _sgd_step(ops, b, cap, kind, (_dev(ids), offs, None if w is None else _dev(w), offs), rng, f"fixed {kind}")
        assert out.data_ptr() == cap.output.data_ptr() and tuple(out.shape) == (80, D)
        assert bool((out[first] == 0).all())
        assert int(cap.kept_dev.item()) == int((ids != PAD).sum())
    nat.status()


# 5. ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["per_bag", "grouped"])
@pytest.mark.parametrize("kind", ["padded_mean", "padded_weighted_sum", "padded_max"])
def test_stale_buffers_are_never_read(ops, nat, kind, family):
    """After a full-capacity call every static buffer is filled with NaN or a sentinel; a 17-id ragged call then returns finite
    numbers that pass the checks of the training test, and nothing past the kept count / the count was written."""
    _, b = tb._pair(ops, "SGD", True)
    try:
        tb._force(nat, b, family)
        cap = _capture(b, kind)
        rng = np.random.default_rng(5)
        _sgd_step(ops, b, cap, kind, tb._call(rng, CAP, "long", kind), rng, f"{kind}/{family}")
        for t in (cap.output, cap.d_output, cap.d_sums, cap.rows, cap.d_rows, cap.weights, cap.weights_k, cap.d_weights,
                  cap.d_weights_out):
            if t is not None:
                t.fill_(float("nan"))
        cap.ids_k.fill_(SENTINEL)
        if cap.map is not None:
            cap.map.fill_(0)          # (a valid place: a read past the count would bring d_weights[0] along)
        call = tb._call(rng, 17, "ragged", kind)
        out = _sgd_step(ops, b, cap, kind, call, rng, f"{kind}/{family}")
        n, kept = call[0].numel(), int((call[0] != PAD).sum())
        assert bool(torch.isfinite(out).all())
        assert all(bool(torch.isfinite(c.data).all()) for c in b.tt_cores)
        assert bool(torch.isnan(cap.d_output[call[3].numel() - 1:]).all())
        assert int(cap.kept_dev.item()) == kept and bool((cap.ids_k[kept:] == SENTINEL).all())
        if cap.weights_k is not None:
            assert bool(torch.isfinite(cap.weights_k[:kept]).all()) and bool(torch.isnan(cap.weights_k[kept:]).all())
            assert bool(torch.isnan(cap.d_weights_out[n:]).all()) and bool((cap.map[n:] == 0).all())
        if cap.rows is not None:   # (rows past the kept ids are empty bags of one: the lookup writes zeros there)
            assert bool(torch.isfinite(cap.rows[:kept]).all()) and bool(torch.isnan(cap.d_rows[kept:]).all())
        nat.status()
    finally:
        nat.set_path(nat.PATH_AUTO)


# 6. ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["per_bag", "grouped"])
@pytest.mark.parametrize("kind", ["padded_mean", "padded_weighted_sum", "padded_max"])
@pytest.mark.parametrize("optimizer", ["SGD", "EXACT_ADAGRAD"])
def test_a_call_of_pads_only(ops, nat, optimizer, kind, family):
    """40 ids in 10 bags, every one the pad: zeros of shape [10, D]; the backward graph replays with a kept count of 0 and
    leaves cores and optimiser state bit-identical (module docstring), the weight gradient is all zeros, and no fault is
    pending.  After a real step, so that the plan and the workspace hold the leftovers of a full call."""
    _, b = tb._pair(ops, optimizer, True)
    try:
        tb._force(nat, b, family)
        cap = _capture(b, kind)
        rng = np.random.default_rng(9)
        ids, offs, w, offs_ref = tb._call(rng, 1000, "ragged", kind)
        cap(ids, offs, w).backward(tb._dy(rng, offs_ref.numel() - 1))
        torch.cuda.synchronize()
        before = [t.detach().clone() for t in tb._tensors(b)]
        pads = torch.full((40,), PAD, dtype=torch.int64, device="cuda")
        offs = torch.arange(0, 41, 4, device="cuda")
        wt = torch.ones(40, device="cuda").requires_grad_(True) if tb.KINDS[kind][1] else None
        cap.output.fill_(float("nan"))
        out = cap(pads, offs, wt)
        assert tuple(out.shape) == (10, D) and bool((out == 0).all())
        out.backward(torch.ones_like(out))
        torch.cuda.synchronize()
        assert int(cap.kept_dev.item()) == 0
        for t, t0 in zip(tb._tensors(b), before):
            assert torch.equal(t.detach(), t0)
        if wt is not None:
            assert wt.grad.shape == wt.shape and bool((wt.grad == 0).all())
        nat.status()
    finally:
        nat.set_path(nat.PATH_AUTO)


# 7. ------------------------------------------------------------------------------------------------------------------
def test_no_host_synchronisation(ops, nat):
    _, b = tb._pair(ops, "SGD", True)
    cap = _capture(b, "padded_weighted_sum")
    rng = np.random.default_rng(6)
    ids, offs, w, offs_ref = tb._call(rng, 1000, "ragged", "padded_weighted_sum")
    dy = tb._dy(rng, offs_ref.numel() - 1)
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


def test_guards_raise_before_anything_is_launched(ops, nat):
    _, plain = tb._pair(ops, "SGD", False)
    with pytest.raises(ValueError, match="padding_idx"):
        plain.capture_bags(64, 32, mode="mean", variable=True, pad_route="partition")
    _, exact = tb._pair(ops, "EXACT_SGD", True)
    with pytest.raises(RuntimeError, match="exact mode.*no device id count"):
        exact.capture_bags(64, 32, mode="mean", variable=False, pad_route="partition")
    assert exact.capture_bags(64, 32, mode="mean", variable=False, pad_route="masked").pad_route == "masked"
    _, b = tb._pair(ops, "SGD", True)
    with pytest.raises(ValueError, match="pad_route must be"):
        b.capture_bags(64, 32, mode="mean", variable=True, pad_route="rows")
    masked = b.capture_bags(64, 32, mode="mean", variable=True)            # today's graphs, untouched by the keyword
    assert masked.route == "rows" and masked.pad_route == "masked" and masked.ids_k is None
    cap = b.capture_bags(64, 32, weighted=True, variable=True, pad_route="partition")
    i64 = lambda *shape: torch.zeros(shape, dtype=torch.int64, device="cuda")
    f32 = lambda *shape: torch.ones(shape, dtype=torch.float32, device="cuda")
    offs = torch.tensor([0, 3, 8], device="cuda")
    assert cap(i64(8) + 7, offs, f32(8)).shape == (2, D)
    torch.cuda.synchronize()
    held = (cap.indices, cap.offsets, cap.weights, cap.nnz_dev, cap.ids_k, cap.offsets_k, cap.weights_k, cap.map, cap.kept_dev)
    staged = [t.clone() for t in held]
    before = [c.detach().clone() for c in b.tt_cores]
    for args, match in (((i64(8), offs), "weighted=True"),
                        ((i64(8), offs, f32(7)), "per_sample_weights"),
                        ((i64(65), torch.tensor([0, 65], device="cuda"), f32(65)), "nnz=64"),
                        ((i64(40), None, f32(40)), "B=32")):
        with pytest.raises(ValueError, match=match):
            cap(*args)
    b.padding_idx = 3
    with pytest.raises(RuntimeError, match="capture_bags\\(\\) again"):
        cap(i64(8), offs, f32(8))
    b.padding_idx = PAD
    torch.cuda.synchronize()
    for t, t0 in zip(held, staged):
        assert torch.equal(t, t0)          # nothing was staged, nothing compacted
    assert all(torch.equal(c.detach(), c0) for c, c0 in zip(b.tt_cores, before))
    assert cap(i64(8) + 7, offs, f32(8)).shape == (2, D)      # and the capture still serves


# 8. ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["capture", "capture_bags", "capture_bags_partition"])
def test_a_fixed_capture_dies_with_its_last_reference(ops, nat, which):
    """A ``variable=False`` call hands out a VIEW of the static output, not the buffer itself: the buffer never gets the
    replay node as its grad_fn, so no cycle capture -> output -> node -> capture keeps the graphs alive for the cyclic
    collector to destroy at a moment of its choosing (inside somebody's stream capture, for one).  With the collector off,
    the capture is gone when its last reference is."""
    _, b = tb._pair(ops, "SGD", which != "capture")
    ids = torch.arange(10, 74, device="cuda")
    offs = torch.arange(0, 65, 2, device="cuda")
    gc.collect()
    gc.disable()
    try:
        if which == "capture":
            cap = b.capture(64, 32, offs)
            out = cap(ids, offs)
        else:
            cap = b.capture_bags(64, 32, mode="mean", pad_route="partition" if which.endswith("partition") else None)
            out = cap(ids, offs)
        assert out.data_ptr() == cap.output.data_ptr() and tuple(out.shape) == (32, D) and cap.output.grad_fn is None
        out.backward(torch.ones_like(out))
        torch.cuda.synchronize()
        alive = weakref.ref(cap)
        del out, cap
        assert alive() is None
    finally:
        gc.enable()
