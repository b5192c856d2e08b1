"""Captured lookups of variable size on the GPU: ``ttemb_stage_call`` against a numpy restatement, and
``emb.capture(nnz, B, variable=True)`` against the eager module, step after step with a different live size each.

Exact mode (``OptimType.EXACT_SGD``) is NOT served by ``variable=True``: the exact entry points take no device id count
(``include/ttemb.h``: ``ttemb_backward_*_exact`` have no ``nnz_dev``), their backward sorts every staged position and cuts
the sorted list into fixed chunks, so ids left over from an earlier call would move the chunk edges and with them the
summation order -- a call shorter than the capacity would not be ``torch.equal`` to the eager call.  ``capture`` refuses it
with an error that says so (the rule of the issue for a route that does not honour the count); the EXACT_SGD case below
asserts that refusal, and that the fixed-size capture of the same module still works."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

P, Q, R = [8, 10, 10], [4, 5, 5], [16, 16]
N_EMB, D = 800, 100
CAP = 4096
SENTINEL = -7777777777


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


def _ragged_lengths(rng, n, max_bags):
    """Bag lengths 0..4 that sum to n, at most max_bags of them, with an empty bag inside and at the end when there is room."""
    lens = []
    left = n
    while left > 0:
        k = int(min(left, rng.integers(0, 5)))
        lens.append(k)
        left -= k
    lens = lens[:max_bags - 3] + ([sum(lens[max_bags - 3:])] if len(lens) > max_bags - 3 else [])
    lens.insert(len(lens) // 2, 0)
    lens.append(0)
    assert sum(lens) == n and len(lens) <= max_bags
    return np.asarray(lens, dtype=np.int64)


# ---------------------------------------------------------------------------------------------------------------------
# ttemb_stage_call alone
# ---------------------------------------------------------------------------------------------------------------------
def _stage_ref(ids, offs, B_live, idx_buf, B_cap):
    """numpy restatement of ttemb_stage_call: (indices_out, offsets_out, count)."""
    n = ids.size
    idx = idx_buf.copy()
    idx[:n] = ids.astype(np.int64)
    o = np.full(B_cap + 1, n, dtype=np.int64)
    o[:B_live + 1] = np.arange(B_live + 1) if offs is None else offs.astype(np.int64)
    return idx, o, n


@pytest.mark.parametrize("bags", ["no_offsets", "bags_of_one", "ragged"])
@pytest.mark.parametrize("dtype", [np.int64, np.int32], ids=["int64", "int32"])
def test_stage_call_against_numpy(nat, dtype, bags):
    rng = np.random.default_rng(3)
    for n in (0, 1, 63, 64, 65, 4095, 4096):
        ids = rng.integers(0, 2 ** 31 - 1, size=n).astype(dtype)
        if dtype == np.int64 and n:
            ids[0] = 2 ** 40 + 5   # (past int32: the int64 path copies all 64 bits)
        if n > 1:
            ids[1] = -3            # (a negative int32 is sign-extended)
        if bags == "no_offsets":
            offs, B_live = None, n
        elif bags == "bags_of_one":
            offs, B_live = np.arange(n + 1).astype(dtype), n
        else:
            lens = _ragged_lengths(rng, n, CAP) if n else np.zeros(3, dtype=np.int64)
            offs = np.concatenate([[0], np.cumsum(lens)]).astype(dtype)
            B_live = lens.size
        idx_buf = np.full(CAP, SENTINEL, dtype=np.int64)
        t_idx, t_off = _dev(idx_buf), torch.full((CAP + 1,), SENTINEL, dtype=torch.int64, device="cuda")
        t_cnt = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        nat.stage_call(_dev(ids), None if offs is None else _dev(offs), t_idx, t_off, t_cnt)
        torch.cuda.synchronize()
        want_idx, want_off, want_cnt = _stage_ref(ids, offs, B_live, idx_buf, CAP)
        assert np.array_equal(t_idx.cpu().numpy(), want_idx), (n, "ids / the untouched tail")
        assert np.array_equal(t_off.cpu().numpy(), want_off), (n, "offsets / their padded tail")
        assert int(t_cnt.item()) == want_cnt, n


def test_stage_call_refuses_bad_sizes_without_a_launch(nat):
    t_idx = torch.full((64,), SENTINEL, dtype=torch.int64, device="cuda")
    t_off = torch.full((33,), SENTINEL, dtype=torch.int64, device="cuda")
    t_cnt = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    ids65, ids40 = torch.zeros(65, dtype=torch.int64, device="cuda"), torch.zeros(40, dtype=torch.int64, device="cuda")
    offs34 = torch.zeros(34, dtype=torch.int64, device="cuda")
    for args, kw, word in (((ids65, None), {}, "capacity"),              # n_live > nnz_cap
                           ((ids40, None), {}, "capacity"),              # bags of one: B_live = 40 > B_cap = 32
                           ((ids40, offs34), {}, "capacity"),            # B_live = 33 > B_cap
                           ((ids40[:8], None), {"B_live": 5}, "bag"),    # no offsets, B_live != n_live
                           ((ids40[:8], offs34[:4]), {"B_live": -1}, "negative")):
        with pytest.raises(RuntimeError, match=word):
            nat.stage_call(*args, t_idx, t_off, t_cnt, **kw)
    with pytest.raises(ValueError):
        nat.stage_call(ids40[:8].float(), None, t_idx, t_off, t_cnt)
    torch.cuda.synchronize()
    assert bool((t_idx == SENTINEL).all()) and bool((t_off == SENTINEL).all()) and int(t_cnt.item()) == -1


# ---------------------------------------------------------------------------------------------------------------------
# captured against eager
# ---------------------------------------------------------------------------------------------------------------------
def _pair(ops, optimizer, p=P, q=Q, r=R, n_emb=N_EMB, scale=None, weight_dist="normal", lr=0.1, **kw):
    """Two modules with identical cores.  ``scale=None``: every core is brought to a standard deviation of 0.2 -- the O(0.2)
    entries test_gpu_module.py gets from its x300 on the products table, whose initialiser's spread depends on the table's
    size.  On this 800-row table a core-0 row collects the gradients of ~512 ids of a full call through float atomics; with
    entries of 0.2 one id adds ~1e-2 to an element and the order of the 512 adds moves lr g by ~lr 6e-8 6 = 4e-8, well inside
    the absolute bound of 1e-6 the fixed-size test uses (its ids are unique: one add per element)."""
    if optimizer == "ADAM":   # weight decay on: a step moves every element, also those no id touches
        kw = dict(kw, weight_decay=0.01)
        lr = 0.01
    mk = lambda: ops.TTEmbeddingBag(n_emb, int(np.prod(q)), r, p, q, optimizer=getattr(ops.OptimType, optimizer), sparse=True,
                                    use_cache=False, weight_dist=weight_dist, learning_rate=lr, **kw)
    torch.manual_seed(11)
    a, b = mk(), mk()
    for ca, cb in zip(a.tt_cores, b.tt_cores):
        ca.data.mul_(scale if scale is not None else 0.2 / float(ca.data.std()))
        cb.data.copy_(ca.data)
    return a, b


def _batch(rng, n, kind, n_emb=N_EMB, d=D):
    """(ids, offsets or None, offsets for the eager call, dY) of a call of n ids."""
    ids = rng.integers(0, n_emb, size=n).astype(np.int64)   # (a small table: duplicate ids in every call)
    if kind == "ragged":
        lens = _ragged_lengths(rng, n, CAP)
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    else:
        offs = np.arange(n + 1, dtype=np.int64)
    dy = ((rng.random((offs.size - 1, d)) - 0.5) * 0.05).astype(np.float32)
    return _dev(ids), (_dev(offs) if kind == "ragged" else None), _dev(offs), _dev(dy)


STEPS = ((4096, "ones"), (1000, "ragged"), (17, "ragged"), (1, "ones"), (4095, "ones"))


def _train_and_compare(a, cap, steps, rng, out_tol, core_tol, n_emb=N_EMB):
    for n, kind in steps:
        ids, offs, offs_eager, dy = _batch(rng, n, kind, n_emb)
        out_a = a(ids, offs_eager)
        out_b = cap(ids, offs)
        assert out_b.shape == out_a.shape
        print(f"\n  n={n:6d} rows max diff {float((out_b - out_a).detach().abs().max()):.3e} of {float(out_a.detach().abs().max()):.2e}", end="")
        torch.testing.assert_close(out_b, out_a, **out_tol(out_a))
        out_a.backward(dy)
        out_b.backward(dy)
        torch.cuda.synchronize()
        for ca, cb in zip(a.tt_cores, cap.module.tt_cores):
            print(f" cores {float((cb.data - ca.data).abs().max()):.3e}", end="")
            torch.testing.assert_close(cb.data, ca.data, **core_tol(ca.data))


@pytest.mark.parametrize("family", ["per_bag", "grouped"])
@pytest.mark.parametrize("optimizer", ["SGD", "EXACT_ADAGRAD", "ADAM", "EXACT_SGD"])
def test_variable_capture_trains_like_the_eager_module(ops, nat, optimizer, family):
    """Five training steps of live sizes 4096 -> 1000 (ragged bags, duplicate ids, empty bags) -> 17 -> 1 -> 4095 through ONE
    pair of graphs captured at capacity 4096, against the eager module on the live ids.  Tolerances: those of
    test_gpu_module.py::test_captured_lookup_trains_like_the_eager_module (float atomics: summation order only)."""
    a, b = _pair(ops, optimizer)
    try:
        nat.set_path(nat.PATH_PER_BAG if family == "per_bag" else nat.PATH_FAST3)
        if optimizer == "EXACT_SGD":   # the documented refusal (module docstring); the fixed-size capture is untouched
            with pytest.raises(RuntimeError, match="exact mode.*no device id count"):
                b.capture(CAP, CAP, variable=True)
            ids, _, offs, dy = _batch(np.random.default_rng(2), 256, "ones")
            cap = b.capture(256, 256)
            out_a, out_b = a(ids, offs), cap(ids)
            assert torch.equal(out_a, out_b)
            out_a.backward(dy)
            out_b.backward(dy)
            torch.cuda.synchronize()
            assert all(torch.equal(ca.data, cb.data) for ca, cb in zip(a.tt_cores, b.tt_cores))
            return
        fam = nat.kernel_family(b._shape, CAP, CAP, True) & 7
        assert fam == (nat.FAMILY_PER_BAG if family == "per_bag" else nat.FAMILY_GROUPED)
        cap = b.capture(CAP, CAP, variable=True)
        sgd = optimizer == "SGD"
        _train_and_compare(a, cap, STEPS, np.random.default_rng(2),
                           lambda ref: dict(rtol=1e-5, atol=1e-6 if sgd else 1e-5),
                           lambda ref: dict(rtol=1e-4, atol=1e-6 if sgd else 2e-5))
        if optimizer == "ADAM":
            assert a.adam_steps() == [len(STEPS)] and b.adam_steps() == [len(STEPS)]
        nat.status()
    finally:
        nat.set_path(nat.PATH_AUTO)


def test_variable_capture_on_the_forward_that_forms_its_prefix_products(ops, nat):
    """Plain SGD on the products shape at capacity 20 000 (1.1 ids per group: the chain kernel forms the prefix products
    itself), live sizes 20 000 -> 7 001."""
    p, n_emb, cap_n = [125, 140, 140], 2449029, 20000
    a, b = _pair(ops, "SGD", p=p, n_emb=n_emb, lr=0.05, scale=300.0)
    try:
        nat.set_path(nat.PATH_FAST3)
        fam = nat.kernel_family(b._shape, cap_n, cap_n, True)
        assert fam & 7 == nat.FAMILY_GROUPED and fam & nat.FAMILY_PREFIX_IN_CHAIN
        cap = b.capture(cap_n, cap_n, variable=True)
        # (tolerances of test_gpu_module.py::test_captured_lookup_on_the_grouped_chain, the fixed capture of this shape and size)
        _train_and_compare(a, cap, ((20000, "ones"), (7001, "ones")), np.random.default_rng(14),
                           lambda ref: dict(rtol=1e-5, atol=2e-6), lambda ref: dict(rtol=1e-4, atol=1e-6), n_emb)
        nat.status()
    finally:
        nat.set_path(nat.PATH_AUTO)


def test_variable_capture_on_the_wide_rank_chain(ops, nat):
    """Rank 64: the wide-rank chain works off the grouping pass's counts, so it honours the device count; live sizes
    1024 -> 333 at capacity 1024.  Tolerances of test_gpu_module.py::test_captured_lookup_on_the_wide_rank_chain."""
    p, q, r = [20, 15, 30], [5, 5, 4], [64, 64]
    n_emb = int(np.prod(p))
    a, b = _pair(ops, "SGD", p=p, q=q, r=r, n_emb=n_emb, scale=1.0, weight_dist="uniform", lr=0.05)
    assert nat.kernel_family(b._shape, 1024, 1024, True) & 7 == nat.FAMILY_GROUPED_WIDE
    cap = b.capture(1024, 1024, variable=True)
    _train_and_compare(a, cap, ((1024, "ones"), (333, "ones")), np.random.default_rng(6),
                       lambda ref: dict(rtol=1e-5, atol=1e-5 * float(ref.detach().abs().max())),
                       lambda ref: dict(rtol=1e-4, atol=1e-5 * float(ref.abs().max())), n_emb)
    nat.status()


@pytest.mark.parametrize("family", ["per_bag", "grouped"])
@pytest.mark.parametrize("optimizer", ["EXACT_ADAGRAD", "ADAM"])
def test_stale_rows_of_the_static_buffers_are_never_read(ops, nat, optimizer, family):
    """Rows past the live bags are not cleared between calls.  With NaN in all of ``output`` and ``d_output`` before a
    17-id step, the returned rows, the cores and the optimiser state are finite and equal to eager."""
    a, b = _pair(ops, optimizer)
    try:
        nat.set_path(nat.PATH_PER_BAG if family == "per_bag" else nat.PATH_FAST3)
        cap = b.capture(CAP, CAP, variable=True)
        rng = np.random.default_rng(5)
        _train_and_compare(a, cap, ((4096, "ones"),), rng, lambda ref: dict(rtol=1e-5, atol=1e-5),
                           lambda ref: dict(rtol=1e-4, atol=2e-5))   # (a full call first: every id slot and row has been used)
        cap.output.fill_(float("nan"))
        cap.d_output.fill_(float("nan"))
        ids, offs, offs_eager, dy = _batch(rng, 17, "ragged")
        out_a, out_b = a(ids, offs_eager), cap(ids, offs)
        assert bool(torch.isfinite(out_b).all())
        torch.testing.assert_close(out_b, out_a, rtol=1e-5, atol=1e-5)
        out_a.backward(dy)
        out_b.backward(dy)
        torch.cuda.synchronize()
        assert bool(torch.isnan(cap.d_output[dy.shape[0]:]).all())   # (the stale rows are still what they were)
        states = lambda e: [*e.optimizer_state] + ([*e.optimizer_state_v] if optimizer == "ADAM" else [])
        for ta, tb in zip([*a.tt_cores, *states(a)], [*b.tt_cores, *states(b)]):
            assert bool(torch.isfinite(tb.data).all())
            torch.testing.assert_close(tb.data, ta.data, rtol=1e-4, atol=2e-5)
    finally:
        nat.set_path(nat.PATH_AUTO)


@pytest.mark.parametrize("optimizer", ["SGD", "EXACT_ADAGRAD", "ADAM"])
def test_a_call_without_ids_is_a_no_op(ops, nat, optimizer):
    """0 ids in 3 empty bags: zeros [3, D]; after backward cores, state and Adam's t are bit-identical to before."""
    _, b = _pair(ops, optimizer)
    cap = b.capture(CAP, CAP, variable=True)
    rng = np.random.default_rng(9)
    ids, offs, _, dy = _batch(rng, 50, "ragged")
    cap(ids, offs).backward(dy)   # (a real step first: Adam's moments are not zero, its t is 1)
    torch.cuda.synchronize()
    state = [*b.tt_cores, *b.optimizer_state] + ([*b.optimizer_state_v, b.adam_step] if optimizer == "ADAM" else [])
    before = [t.detach().clone() for t in state]
    cap.output.fill_(float("nan"))
    out = cap(torch.zeros(0, dtype=torch.int64, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda"))
    assert out.shape == (3, D) and bool((out == 0).all())
    out.backward(torch.ones_like(out))
    torch.cuda.synchronize()
    for t, t0 in zip(state, before):
        assert torch.equal(t.detach(), t0)
    if optimizer == "ADAM":
        assert b.adam_steps() == [1]
    out = cap(torch.zeros(0, dtype=torch.int32, device="cuda"))   # (without offsets: no bag at all)
    assert out.shape == (0, D)
    out.backward(torch.ones_like(out))
    torch.cuda.synchronize()
    assert all(torch.equal(t.detach(), t0) for t, t0 in zip(state, before))


def test_int32_ids_and_offsets_give_what_int64_give(ops, nat):
    a, b = _pair(ops, "SGD")
    cap_a, cap_b = a.capture(CAP, CAP, variable=True), b.capture(CAP, CAP, variable=True)
    rng = np.random.default_rng(4)
    for n, kind in ((1000, "ragged"), (65, "ones")):
        ids, offs, _, dy = _batch(rng, n, kind)
        out_a = cap_a(ids, offs)
        out_b = cap_b(ids.int(), None if offs is None else offs.int())
        torch.testing.assert_close(out_b, out_a, rtol=1e-5, atol=1e-6)
        out_a.backward(dy)
        out_b.backward(dy)
        torch.cuda.synchronize()
        assert torch.equal(cap_a.indices[:n], cap_b.indices[:n]) and torch.equal(cap_a.offsets, cap_b.offsets)
        for ca, cb in zip(a.tt_cores, b.tt_cores):
            torch.testing.assert_close(cb.data, ca.data, rtol=1e-4, atol=1e-6)


def test_refusals(ops, nat):
    _, b = _pair(ops, "SGD")
    with pytest.raises(ValueError, match="offsets"):
        b.capture(64, 32, torch.arange(33, device="cuda"), variable=True)
    cap = b.capture(64, 32, variable=True)
    before = (cap.indices.clone(), cap.offsets.clone(), cap.nnz_dev.clone())
    i64 = lambda n: torch.zeros(n, dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError, match="nnz=64"):
        cap(i64(65), torch.tensor([0, 65], device="cuda"))
    with pytest.raises(ValueError, match="B=32"):
        cap(i64(40))                       # bags of one: 40 bags
    with pytest.raises(ValueError, match="B=32"):
        cap(i64(10), torch.arange(34, device="cuda").clamp(max=10))
    torch.cuda.synchronize()
    for t, t0 in zip((cap.indices, cap.offsets, cap.nnz_dev), before):
        assert torch.equal(t, t0)          # nothing was staged
    assert cap(i64(64), torch.arange(33, device="cuda") * 2).shape == (32, D)
    # the refusals of every captured lookup are still in place
    b.eps = 1e-3
    with pytest.raises(RuntimeError, match="capture\\(\\) again"):
        cap(i64(4))
    b.eps = 1.0e-10
    b.learning_rate = 0.5
    with pytest.raises(RuntimeError, match="capture\\(\\) again"):
        cap(i64(4))
    mk = lambda **kw: ops.TTEmbeddingBag(N_EMB, D, R, P, Q, sparse=True, weight_dist="normal", **kw)
    with pytest.raises(AssertionError, match="mode"):
        mk(use_cache=False, mode="mean").capture(64, 32, variable=True)
    with pytest.raises(AssertionError, match="padding_idx"):
        mk(use_cache=False, padding_idx=3).capture(64, 32, variable=True)
    with pytest.raises(AssertionError, match="single table"):
        ops.TableBatchedTTEmbeddingBag(2, N_EMB, D, R, P, Q, sparse=True).capture(64, 32, variable=True)
    cached = mk(use_cache=True, cache_size=100, hashtbl_size=400)
    cap_c = cached.capture(64, 32, variable=True)
    cap_c(torch.arange(20, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    assert int(cached.cache_freq.sum().item()) == 20   # warm-up statistics count through the captured call
    cached.cache_populate()
    with pytest.raises(RuntimeError, match="live cache"):
        cap_c(i64(4))
    with pytest.raises(AssertionError, match="live row cache"):
        cached.capture(64, 32, variable=True)
    adam = mk(use_cache=False, optimizer=ops.OptimType.ADAM)
    cap_m = adam.capture(64, 32, variable=True)
    adam.betas = (0.5, 0.999)
    with pytest.raises(RuntimeError, match="capture\\(\\) again"):
        cap_m(i64(4))


def test_the_fixed_capture_still_takes_exactly_its_size(ops):
    _, b = _pair(ops, "SGD")
    cap = b.capture(64, 64)
    assert cap.variable is False and cap.nnz_dev is None
    with pytest.raises(RuntimeError):
        cap(torch.zeros(63, dtype=torch.int64, device="cuda"))
    assert cap(torch.zeros(64, dtype=torch.int64, device="cuda")).shape == (64, D)
