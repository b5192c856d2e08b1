"""Device-resident learning rate on the GPU: a ``capturable=True`` module -- eager, through a fixed capture and through a
``variable=True`` capture, with a new rate every step and nothing re-captured -- against a twin with identical cores built
without the flag, stepped eagerly with ``set_learning_rate()`` called to match.  The two differ only in where the rate comes
from; the float32 value is the same on both sides (``fill_`` on a float32 word and the ctypes ``float`` argument round the
same way).  Where the kernels are deterministic (flat steps, exact mode) the comparison is ``torch.equal``; on the default
routes (float atomics: summation order only) it uses the tolerances the existing capture tests apply to the same shapes."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

P, Q, R = [8, 10, 10], [4, 5, 5], [16, 16]
N_EMB, D = 800, 100
CAP = 4096


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


def _word(x):
    return torch.full((1,), x, dtype=torch.float32, device="cuda")


# ---------------------------------------------------------------------------------------------------------------------
# bit for bit: the flat steps
# ---------------------------------------------------------------------------------------------------------------------
RATES2 = (0.1, 0.025)


def _flat_inputs(n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda: torch.randn(n, device="cuda", generator=g)
    return r(), r().abs(), r().abs(), r()   # weights, state (>= 0), second state (>= 0), gradients


@pytest.mark.parametrize("n", [1, 3, 4, 1027])
def test_flat_sgd_and_adagrad_steps_bit_for_bit(nat, n):
    """``ttemb_flat_step`` against ``ttemb_sgd_step``, ``ttemb_sgd_step_guarded`` (a clear and a set skip word) and
    ``ttemb_adagrad_step``: two consecutive steps at 0.1 then 0.025 on the same random weights, state and gradients."""
    w0, s0, _, g = _flat_inputs(n, n)
    lr = _word(0.0)
    clear, set_ = torch.zeros(1, device="cuda"), torch.ones(1, device="cuda")
    for name in ("sgd", "guarded", "guarded_skipped", "adagrad"):
        wa, wb, sa, sb = w0.clone(), w0.clone(), s0.clone(), s0.clone()
        for rate in RATES2:
            lr.fill_(rate)
            if name == "sgd":
                nat.sgd_step(wa, g, rate)
                nat.sgd_step(wb, g, lr)
            elif name == "adagrad":
                nat.adagrad_step(wa, sa, g, rate, 1e-8)
                nat.adagrad_step(wb, sb, g, lr, 1e-8)
            else:
                skip = clear if name == "guarded" else set_
                nat.sgd_step_guarded(wa, g, rate, skip)
                nat.sgd_step_guarded(wb, g, lr, skip)
        torch.cuda.synchronize()
        assert torch.equal(wa, wb) and torch.equal(sa, sb), name
        assert torch.equal(wa, w0) == (name == "guarded_skipped"), name


@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
@pytest.mark.parametrize("decoupled", [False, True], ids=["adam", "adamw"])
@pytest.mark.parametrize("n", [1, 3, 4, 1027])
def test_flat_adam_step_bit_for_bit(nat, n, decoupled, grad_scale):
    """``ttemb_flat_step`` (Adam) against ``ttemb_adam_step``: weights, both moments and ``step[0]`` after two steps."""
    w0, m0, v0, g = _flat_inputs(n, 100 + n)
    lr = _word(0.0)
    a = [w0.clone(), m0.clone(), v0.clone(), nat.new_adam_step("cuda")]
    b = [w0.clone(), m0.clone(), v0.clone(), nat.new_adam_step("cuda")]
    for rate in RATES2:
        lr.fill_(rate)
        nat.adam_step(*a, g, nat.make_adam(rate, 1e-8, (0.9, 0.999), 0.01, decoupled), grad_scale)
        # (the rate of the descriptor's hyper-parameters is ignored: 123 would be seen at once)
        nat.adam_step(*b, g, nat.make_adam(123.0, 1e-8, (0.9, 0.999), 0.01, decoupled), grad_scale, lr=lr)
    torch.cuda.synchronize()
    for ta, tb in zip(a, b):
        assert torch.equal(ta, tb)
    assert int(b[3][0]) == 2 and not torch.equal(b[0], w0)


def test_a_null_rate_word_is_refused_with_nothing_launched(nat):
    import ctypes
    w, _, _, g = _flat_inputs(8, 1)
    w0 = w.clone()
    d = nat.StepDesc()   # (kind SGD, lr_dev null)
    rc = nat.LIB.ttemb_flat_step(w.data_ptr(), None, None, None, g.data_ptr(), 8, 1.0, ctypes.byref(d), None, None)
    assert rc == -1 and b"lr_dev" in nat.LIB.ttemb_last_error()
    torch.cuda.synchronize()
    assert torch.equal(w, w0)


# ---------------------------------------------------------------------------------------------------------------------
# modules: a capturable one and its eager twin
# ---------------------------------------------------------------------------------------------------------------------
def _pair(ops, optimizer, p=P, q=Q, r=R, n_emb=N_EMB, scale=None, weight_dist="normal", lr=0.1, tables=0, **kw):
    """(twin, capturable) with identical cores, brought to a standard deviation of 0.2 as in
    test_gpu_capture_variable.py::_pair (``scale``: a plain factor instead).  ADAM / ADAMW: weight decay 0.01, lr 0.01.

    ADAM's ``eps``.  Twin and capturable module sum the same gradient g in two orders (float atomics), d apart.  An SGD step
    carries that into the cores as lr d -- what the cited tolerances were set for.  Adam's step is lr m^ / (sqrt(v^) + eps),
    at t = 1 lr g / (|g| + eps), whose slope in g is lr eps / (|g| + eps)^2 <= lr / eps: with the module default eps = 1e-10
    an element whose g + wd w nearly cancels turns d ~ 1e-9 into a difference of up to 2 lr, whatever the rate's source (one
    element in 307 200 of the rank-64 table did).  The comparison is made well-conditioned instead of wider: eps is chosen
    so that lr / eps equals the SGD rate of the same case (``lr`` as passed in: 0.1 on the small tables, 0.05 on the wide
    and the products table), i.e. Adam passes on at most what the SGD case of the same shape does, and the SGD tolerances
    hold for it.  Every term the rate enters (lr / (1 - b1^t), the decoupled lr wd w) stays first order in the result."""
    opt = "ADAM" if optimizer == "ADAMW" else optimizer
    if opt == "ADAM":
        kw = dict(kw, weight_decay=0.01, decoupled_weight_decay=optimizer == "ADAMW", eps=0.01 / lr)
        lr = 0.01
    args = (n_emb, int(np.prod(q)), r, p, q)
    common = dict(optimizer=getattr(ops.OptimType, opt), sparse=True, use_cache=False, weight_dist=weight_dist, learning_rate=lr, **kw)
    mk = ((lambda **k: ops.TableBatchedTTEmbeddingBag(tables, *args, **common, **k)) if tables
          else (lambda **k: ops.TTEmbeddingBag(*args, **common, **k)))
    torch.manual_seed(11)
    a, b = mk(), mk(capturable=True)
    for ca, cb in zip(a.tt_cores, b.tt_cores):
        ca.data.mul_(scale if scale is not None else 0.2 / float(ca.data.std()))
        cb.data.copy_(ca.data)
    return a, b, lr


def _ragged_offsets(rng, n, bags):
    """``bags`` bag boundaries over n ids, with an empty bag inside and one at the end."""
    cuts = np.sort(rng.integers(0, n + 1, size=bags - 3))
    offs = np.concatenate([[0], cuts, [n, n]]).astype(np.int64)
    offs = np.insert(offs, bags // 2, offs[bags // 2])
    assert offs.size == bags + 1 and offs[-1] == n
    return offs


def _batch(rng, n, kind, n_emb=N_EMB, d=D):
    ids = rng.integers(0, n_emb, size=n).astype(np.int64)   # (small tables: duplicate ids in every call)
    offs = _ragged_offsets(rng, n, max(4, n // 3)) if kind == "ragged" else np.arange(n + 1, dtype=np.int64)
    dy = ((rng.random((offs.size - 1, d)) - 0.5) * 0.05).astype(np.float32)
    return _dev(ids), _dev(offs), _dev(dy)


def _states(e):
    """The optimiser state that holds anything (SGD registers empty buffers)."""
    return [t for t in [*e.optimizer_state] + ([*e.optimizer_state_v] if hasattr(e, "optimizer_state_v") else []) if t.numel()]


def _steps_and_compare(a, b, call_b, steps, rng, out_tol, core_tol, n_emb=N_EMB, d=D, exact=False):
    """Every step: the rate goes to the twin and to the capturable module as a float, both are stepped, rows and cores are
    compared (each figure is printed before it is asserted)."""
    for n, kind, rate in steps:
        ids, offs, dy = _batch(rng, n, kind, n_emb, d) if not callable(kind) else kind(rng)
        a.set_learning_rate(rate)
        b.set_learning_rate(rate)
        out_a, out_b = a(ids, offs), call_b(ids, offs)
        assert out_b.shape == out_a.shape
        print(f"\n  n={ids.numel():6d} lr={rate:.5f} rows {float((out_b - out_a).detach().abs().max()):.3e}", end="")
        if exact:
            assert torch.equal(out_b, out_a)
        else:
            torch.testing.assert_close(out_b, out_a, **out_tol(out_a))
        out_a.backward(dy.view(out_a.shape))
        out_b.backward(dy.view(out_b.shape))
        torch.cuda.synchronize()
        for ta, tb in zip([*a.tt_cores, *_states(a)], [*b.tt_cores, *_states(b)]):
            print(f" {float((tb.data - ta.data).abs().max()):.2e}", end="")
            if exact:
                assert torch.equal(tb.data, ta.data)
            else:
                torch.testing.assert_close(tb.data, ta.data, **core_tol(ta.data))


# ---- exact mode: bit for bit ----
@pytest.mark.parametrize("via", ["eager", "capture"])
@pytest.mark.parametrize("optimizer,deterministic", [("EXACT_SGD", None), ("EXACT_ADAGRAD", True), ("ADAM", True)])
def test_exact_mode_bit_for_bit(ops, nat, optimizer, deterministic, via):
    """800 rows, 256 ids with duplicates in ragged bags, three steps at 0.1, 0.05, 0.05: outputs, cores and optimiser
    state ``torch.equal`` to the eager twin, eagerly and through a fixed-size capture."""
    a, b, _ = _pair(ops, optimizer, deterministic=deterministic)
    assert b._exact_active()
    rng = np.random.default_rng(21)
    offs = _dev(_ragged_offsets(rng, 256, 80))

    def call(r):
        ids = _dev(r.integers(0, N_EMB, size=256).astype(np.int64))
        return ids, offs, _dev(((r.random((80, D)) - 0.5) * 0.05).astype(np.float32))

    if via == "capture":
        cap = b.capture(256, 80, offs)
        assert cap.exact
        graphs = (cap.fwd_graph, cap.bwd_graph)
    _steps_and_compare(a, b, cap if via == "capture" else b, [(256, call, rate) for rate in (0.1, 0.05, 0.05)], rng, None, None,
                       exact=True)
    if via == "capture":
        assert cap.fwd_graph is graphs[0] and cap.bwd_graph is graphs[1]   # nothing was re-captured
    if optimizer == "ADAM":
        assert a.adam_steps() == b.adam_steps() == [3]


# ---- the small table on the per-bag and the grouped route ----
@pytest.mark.parametrize("via", ["eager", "fixed", "variable"])
@pytest.mark.parametrize("family", ["per_bag", "grouped"])
@pytest.mark.parametrize("optimizer", ["SGD", "EXACT_ADAGRAD", "ADAM", "ADAMW"])
def test_small_table_follows_a_schedule(ops, nat, optimizer, family, via):
    """Four steps of 4096, 1000 (ragged, empty bags), 17 and 1 ids at rates lr, lr/2, lr/2, lr/8 (the fixed capture: 4096
    ids every step), eager, through ``capture(4096, 4096)`` and through ``capture(4096, 4096, variable=True)``; the graphs
    at the end are the objects ``capture()`` made.  Tolerances:
    test_gpu_capture_variable.py::test_variable_capture_trains_like_the_eager_module, which takes them from
    test_gpu_module.py::test_captured_lookup_trains_like_the_eager_module (rows rtol 1e-5, atol 1e-6 for SGD else 1e-5;
    cores rtol 1e-4, atol 1e-6 for SGD else 2e-5)."""
    a, b, lr = _pair(ops, optimizer)
    rates = (lr, lr / 2, lr / 2, lr / 8)
    sizes = ((4096, "ones"), (1000, "ragged"), (17, "ragged"), (1, "ones"))
    try:
        nat.set_path(nat.PATH_PER_BAG if family == "per_bag" else nat.PATH_FAST3)
        fam = nat.kernel_family(b._shape, CAP, CAP, True) & 7
        assert fam == (nat.FAMILY_PER_BAG if family == "per_bag" else nat.FAMILY_GROUPED)
        if via == "eager":
            call_b = b
        else:
            cap = b.capture(CAP, CAP, variable=via == "variable")
            graphs = (cap.fwd_graph, cap.bwd_graph)
            call_b = cap
            if via == "fixed":
                sizes = ((4096, "ones"),) * 4
                call_b = lambda ids, offs: cap(ids)
        sgd = optimizer == "SGD"
        _steps_and_compare(a, b, call_b, [(n, k, r) for (n, k), r in zip(sizes, rates)], np.random.default_rng(2),
                           lambda ref: dict(rtol=1e-5, atol=1e-6 if sgd else 1e-5),
                           lambda ref: dict(rtol=1e-4, atol=1e-6 if sgd else 2e-5))
        if via != "eager":
            assert cap.fwd_graph is graphs[0] and cap.bwd_graph is graphs[1]   # nothing was re-captured
        if optimizer in ("ADAM", "ADAMW"):
            assert a.adam_steps() == b.adam_steps() == [4]
        assert float(b.lr_dev) == np.float32(lr / 8)
        nat.status()
    finally:
        nat.set_path(nat.PATH_AUTO)


# ---- one small case per other route that reaches a different stepping kernel ----
SMALL_TOL = (lambda sgd: (lambda ref: dict(rtol=1e-5, atol=1e-6 if sgd else 1e-5)),
             lambda sgd: (lambda ref: dict(rtol=1e-4, atol=1e-6 if sgd else 2e-5)))


def _two_steps(ops, nat, optimizer, sizes, tol=None, via="eager", path=None, expect=None, **pair_kw):
    a, b, lr = _pair(ops, optimizer, **pair_kw)
    n_emb, d = pair_kw.get("n_emb", N_EMB), int(np.prod(pair_kw.get("q", Q)))
    sgd = optimizer == "SGD"
    out_tol, core_tol = tol if tol is not None else (SMALL_TOL[0](sgd), SMALL_TOL[1](sgd))
    try:
        if path is not None:
            nat.set_path(path)
        if expect is not None:
            expect(b)
        call_b = b
        if via == "variable":
            cap = b.capture(sizes[0], sizes[0], variable=True)
            graphs = (cap.fwd_graph, cap.bwd_graph)
            call_b = cap
        _steps_and_compare(a, b, call_b, [(sizes[0], "ones", lr), (sizes[1], "ones", lr / 4)], np.random.default_rng(6),
                           out_tol, core_tol, n_emb, d)
        if via == "variable":
            assert cap.fwd_graph is graphs[0] and cap.bwd_graph is graphs[1]
        if optimizer == "ADAM":
            assert a.adam_steps() == b.adam_steps()
        nat.status()
    finally:
        nat.set_path(nat.PATH_AUTO)
    return a, b


@pytest.mark.parametrize("optimizer", ["SGD", "ADAM"])
def test_wide_rank_chain(ops, nat, optimizer):
    """Rank 64, 1024 then 333 ids through a variable capture.  Tolerances of
    test_gpu_module.py::test_captured_lookup_on_the_wide_rank_chain (relative to the largest entry)."""
    p, q, r = [20, 15, 30], [5, 5, 4], [64, 64]

    def expect(b):
        assert nat.kernel_family(b._shape, 1024, 1024, True) & 7 == nat.FAMILY_GROUPED_WIDE

    _two_steps(ops, nat, optimizer, (1024, 333), via="variable", expect=expect, p=p, q=q, r=r, n_emb=int(np.prod(p)), scale=1.0,
               weight_dist="uniform", lr=0.05, tol=(lambda ref: dict(rtol=1e-5, atol=1e-5 * float(ref.detach().abs().max())),
                                                    lambda ref: dict(rtol=1e-4, atol=1e-5 * float(ref.abs().max()))))


@pytest.mark.parametrize("optimizer", ["SGD", "ADAM"])
def test_products_table_where_the_chain_forms_its_prefix_products(ops, nat, optimizer):
    """20 000 then 7 001 ids at capacity 20 000 on the products shape.  Tolerances of
    test_gpu_module.py::test_captured_lookup_on_the_grouped_chain (rows atol 2e-6, cores atol 1e-6; ADAM: the 1e-5 / 2e-5 of
    test_captured_lookup_trains_like_the_eager_module, whose Adam step divides by sqrt(v))."""
    sgd = optimizer == "SGD"

    def expect(b):
        fam = nat.kernel_family(b._shape, 20000, 20000, True)
        assert fam & 7 == nat.FAMILY_GROUPED and fam & nat.FAMILY_PREFIX_IN_CHAIN

    _two_steps(ops, nat, optimizer, (20000, 7001), via="variable", path=nat.PATH_FAST3, expect=expect, p=[125, 140, 140], n_emb=2449029,
               lr=0.05, scale=300.0, tol=(lambda ref: dict(rtol=1e-5, atol=2e-6 if sgd else 1e-5),
                                          lambda ref: dict(rtol=1e-4, atol=1e-6 if sgd else 2e-5)))


@pytest.mark.parametrize("optimizer", ["SGD", "ADAM", "EXACT_ADAGRAD"])
def test_padded_rank(ops, nat, optimizer):
    """Rank 12 rides on the rank-16 grouped kernels through padded cores: gradients into scratch, then the step kernel.
    Tolerances of test_gpu_module.py::test_captured_lookup_trains_like_the_eager_module (same table, same sizes)."""
    def expect(b):
        assert nat.kernel_family(b._shape, 4096, 4096, True) & nat.FAMILY_PADDED

    _two_steps(ops, nat, optimizer, (4096, 777), path=nat.PATH_FAST3, expect=expect, r=[12, 12])


@pytest.mark.parametrize("shape", ["T2", "T4"])
@pytest.mark.parametrize("optimizer", ["SGD", "ADAM", "EXACT_ADAGRAD"])
def test_two_and_four_core_tables(ops, nat, optimizer, shape):
    """The shapes of the golden cases tt_tiny_T2 / tt_tiny_T4 (a merged 3-core view, or the scalar kernels: gradients into
    scratch, then the step kernel).  Tolerances as test_padded_rank."""
    p, q, r = ([6, 7], [4, 3], [5]) if shape == "T2" else ([3, 2, 4, 3], [2, 2, 3, 2], [3, 4, 2])
    _two_steps(ops, nat, optimizer, (300, 41), p=p, q=q, r=r, n_emb=int(np.prod(p)))


@pytest.mark.parametrize("optimizer", ["SGD", "ADAM", "EXACT_ADAGRAD"])
def test_a_call_in_pieces(ops, nat, optimizer):
    """Piece limits of 1 400 ids: 4096 ids run as three pieces, whose summed gradient is stepped once.  Tolerances as
    test_padded_rank."""
    nat.set_piece_limits(1400, 1400)
    try:
        def expect(b):
            assert nat.plan_bytes(b._shape, 4096) == 0   # (a call in pieces keeps no plan: include/ttemb.h)

        _two_steps(ops, nat, optimizer, (4096, 3000), path=nat.PATH_FAST3, expect=expect)
    finally:
        nat.set_piece_limits(0, 0)


@pytest.mark.parametrize("optimizer", ["SGD", "ADAM"])
def test_windows_of_two_tables(ops, nat, optimizer):
    """``num_tables=2``: each table steps inside the finalize kernel of its own window.  Tolerances as test_padded_rank."""
    a, b, lr = _pair(ops, optimizer, tables=2)
    sgd = optimizer == "SGD"
    rng = np.random.default_rng(8)
    for n, rate in ((3000, lr), (500, lr / 4)):
        B = n // 2
        ids = _dev(rng.integers(0, N_EMB, size=n).astype(np.int64))
        offs = _dev(np.arange(n + 1, dtype=np.int64))
        dy = _dev(((rng.random((2, B, D)) - 0.5) * 0.05).astype(np.float32))
        assert nat.window_workspace_bytes(b._shape, nat.OP_BACKWARD, n, n, B) >= 0   # (served as windows, no host split)
        a.set_learning_rate(rate)
        b.set_learning_rate(rate)
        out_a, out_b = a(ids, offs), b(ids, offs)
        torch.testing.assert_close(out_b, out_a, rtol=1e-5, atol=1e-6 if sgd else 1e-5)
        out_a.backward(dy)
        out_b.backward(dy)
        torch.cuda.synchronize()
        for ta, tb in zip([*a.tt_cores, *_states(a)], [*b.tt_cores, *_states(b)]):
            print(f" {float((tb.data - ta.data).abs().max()):.2e}", end="")
            torch.testing.assert_close(tb.data, ta.data, rtol=1e-4, atol=1e-6 if sgd else 2e-5)
    if optimizer == "ADAM":
        assert a.adam_steps() == b.adam_steps() == [2, 2]
    nat.status()


# ---- the rate from a tensor, the rate 0 ----
def test_a_tensor_rate_costs_no_synchronisation(ops, nat):
    """``set_learning_rate(tensor)`` and a captured step under ``set_sync_debug_mode("error")`` (as
    test_gpu_module.py::test_table_batched runs its lookups); the result is the twin's at 0.05.  Tolerances of
    test_gpu_module.py::test_captured_lookup_trains_like_the_eager_module (SGD)."""
    a, b, _ = _pair(ops, "SGD")
    cap = b.capture(256, 256)
    ids, offs, dy = _batch(np.random.default_rng(3), 256, "ones")
    rate = torch.tensor([0.05], device="cuda")
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        b.set_learning_rate(rate)
        out_b = cap(ids)
        out_b.backward(dy)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    a.set_learning_rate(0.05)
    out_a = a(ids, offs)
    out_a.backward(dy)
    torch.cuda.synchronize()
    torch.testing.assert_close(out_b, out_a, rtol=1e-5, atol=1e-6)
    for ca, cb in zip(a.tt_cores, b.tt_cores):
        torch.testing.assert_close(cb.data, ca.data, rtol=1e-4, atol=1e-6)
    assert float(b.lr_dev) == np.float32(0.05) and b._lr_mirror is None
    rate.fill_(0.5)               # the module holds a copy: the caller's tensor is free again
    torch.cuda.synchronize()
    assert float(b.lr_dev) == np.float32(0.05)


def test_rate_zero_leaves_every_core_as_it_was(ops, nat):
    _, b, _ = _pair(ops, "SGD")
    ids, offs, dy = _batch(np.random.default_rng(4), 1000, "ragged")
    before = [c.data.clone() for c in b.tt_cores]
    b.set_learning_rate(0.0)
    b(ids, offs).backward(dy)
    torch.cuda.synchronize()
    assert float(b.lr_dev) == 0.0
    assert all(torch.equal(c.data, c0) for c, c0 in zip(b.tt_cores, before))
    b.set_learning_rate(0.1)      # ... and the same call at 0.1 does move them
    b(ids, offs).backward(dy)
    torch.cuda.synchronize()
    assert not any(torch.equal(c.data, c0) for c, c0 in zip(b.tt_cores, before))


# ---- unchanged behaviour and refusals ----
def test_refusals(ops, nat):
    a, b, _ = _pair(ops, "SGD")
    ids, _, dy = _batch(np.random.default_rng(5), 64, "ones")
    cap_a, cap_b = a.capture(64, 64), b.capture(64, 64)
    cap_a(ids).backward(dy)
    a.set_learning_rate(0.05)     # without capturable the rate is part of the captured backward, as before
    with pytest.raises(RuntimeError, match="learning rate / eps are part of the captured backward: capture\\(\\) again"):
        cap_a(ids)
    b.set_learning_rate(0.05)
    cap_b(ids).backward(dy)
    b.eps = 1e-3                  # eps still is
    with pytest.raises(RuntimeError, match="capture\\(\\) again"):
        cap_b(ids)
    b.eps = 1.0e-10
    cap_b(ids).backward(dy)
    b.lr_dev = b.lr_dev.clone()   # the graphs hold the old word by address
    with pytest.raises(RuntimeError, match="re-allocated after capture\\(\\)"):
        cap_b(ids)
    with pytest.raises(ValueError, match="capturable=True is not supported"):
        ops.TTEmbeddingBag(N_EMB, D, R, P, Q, sparse=True, use_cache=True, cache_size=10, hashtbl_size=40, capturable=True)
    torch.cuda.synchronize()
