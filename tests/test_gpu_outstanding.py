"""Lookups whose backward comes later.  Every other GPU test runs one lookup as forward, its own backward, then the next
call; here several forwards are open before a backward runs, a backward runs after other calls have used (and re-allocated)
the workspace, and a backward runs after the cores have moved.  What must hold (include/ttemb.h at ttemb_plan_bytes,
DESIGN.md "Calls in flight"): a plan owns the grouping and the prefix products P of its forward; everything else of a call
lives in the shared workspace and dies with the call; a backward handed the plan differentiates at the forward's P, one
without a plan forms P from the cores it is given.

Part 1 is the C ABI (several plans on one workspace), part 2 the module (several lookups through one TTEmbeddingBag before
backward).  Every numeric check is the per-element fp32 bound of tests/fp32_bound.py against the float64 oracle, or a bit
equality; every case first asserts the kernel family and the route flags it means to run, every "workspace grew" case the
new buffer, every saved-P case that its two possible answers are apart (tests/outstanding.py)."""
import zlib

import numpy as np
import pytest
import torch

import adam_bound as ab
import fp32_bound as fb
import outstanding as ost
from oracle import tt_oracle as orc

pytestmark = pytest.mark.gpu

LR, EPS = 0.05, 1e-3
WORST = {}   # case -> largest err / (u mag) seen (printed at the end of the module: a record, not a threshold)
_REFS = {}   # oracle results shared between the cases that use the same inputs; never modified


@pytest.fixture(scope="module")
def nat():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import ttemb_native
    yield ttemb_native
    ttemb_native.set_path(ttemb_native.PATH_AUTO)
    ttemb_native.set_piece_limits(0, 0)
    ttemb_native.set_wide_slab_min_ids(0)
    for k in sorted(WORST):
        print(f"\n  {k:34s} largest err/(u mag) {WORST[k]:.2f}", end="")


@pytest.fixture(scope="module")
def ops(nat):
    from FBTT import tt_embeddings_ops
    return tt_embeddings_ops


def _dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


def _np(ts):
    return [t.detach().cpu().numpy() for t in ts]


def _note(key, r):
    WORST[key] = max(WORST.get(key, 0.0), r)


def _route(fam, nat):
    return {nat.FAMILY_SCALAR: "scalar", nat.FAMILY_PER_BAG: "per_bag", nat.FAMILY_PER_BAG_RT: "per_bag",
            nat.FAMILY_GROUPED: "grouped", nat.FAMILY_GROUPED_WIDE: "wide"}[fam & 7]


def _crc(cores):
    """Identity of a set of cores for the memo keys: an expectation belongs to the cores it was computed from."""
    h = 0
    for c in cores:
        h = zlib.crc32(np.ascontiguousarray(c).tobytes(), h)
    return h


def _memo(key, make):
    if key not in _REFS:
        _REFS[key] = make()
    return _REFS[key]


# =====================================================================================================================
# 1. C ABI: several plans on one workspace
# =====================================================================================================================
# plan-less controls among the routes: (key, p, q, inner ranks, ids, path, family & 7, flags, kernel ranks, wide form)
CONTROLS = [
    ("small3", [23, 290, 310], [4, 5, 5], [16, 16], 1600, "auto", 1, 0, None, None),   # (2.5 x 1 600 stays under the crossover)
    ("generic", [23, 290, 310], [4, 5, 5], [16, 16], 4000, "generic", 0, 0, None, None),
    ("pieces", [30, 35, 400], [4, 5, 5], [16, 16], 12000, "pieces", 3, 0, None, None),
]
PIECE_ROWS, PIECE_IDS = 900, 700


def _select(nat, case):
    """The process-wide knobs of a case's route."""
    path, form = case[5], case[9]
    nat.set_path({"auto": nat.PATH_AUTO, "generic": nat.PATH_GENERIC, "fast3": nat.PATH_FAST3, "pieces": nat.PATH_FAST3}[path])
    if path == "pieces":
        nat.set_piece_limits(PIECE_ROWS, PIECE_IDS)
    else:
        nat.set_piece_limits(0, 0)
    nat.set_wide_slab_min_ids(0 if form is None else (1 if form == "lds_slabs" else 1 << 40))


class AbiCall:
    """One lookup at the C ABI: its inputs on the device, its own plan tensor (None where the route keeps none), its oracle."""

    def __init__(self, nat, case, cores, n_ids, seed):
        self.nat, self.case, self.cores = nat, case, cores
        self.key, self.p, self.q, r = case[0], case[1], case[2], case[3]
        self.R, self.Rk = [1] + r + [1], [1] + (case[8] or r) + [1]
        rng = np.random.default_rng(seed)
        self.ids, self.offs, self.dy = ost.call_inputs(rng, self.p, self.q, n_ids)
        self.nnz, self.B, self.D = self.ids.shape[0], self.offs.shape[0] - 1, int(np.prod(self.q))
        self.shape = nat.make_shape(self.p, self.q, self.R)
        self.seed = (self.key if not self.key.startswith("wide") else "wide", tuple(self.p), n_ids, seed, _crc(cores))
        self.I, self.O, self.dY = _dev(self.ids), _dev(self.offs), _dev(self.dy)
        self.plan = None
        self.pieces = 0

    def assert_route(self):
        nat, case = self.nat, self.case
        _select(nat, case)
        fam = nat.kernel_family(self.shape, self.nnz, self.B, True)
        assert fam & 7 == case[6] and fam & case[7] == case[7], (self.key, self.nnz, fam)
        if self.key == "fast3":   # the plain grouped kernels: neither chain kernel forms products of its own
            assert fam & nat.FAMILY_ROUTE_FLAGS == 0, (self.key, self.nnz, fam)
        if case[5] == "pieces":
            assert nat.plan_bytes(self.shape, self.nnz) == 0   # a call in pieces keeps no plan
            self.pieces = -(-self.nnz // PIECE_IDS) + -(-self.B // PIECE_ROWS) + 1
        self.route = _route(fam, nat)
        keeps_plan = case[6] >= 3 and case[5] != "pieces"
        assert (nat.plan_bytes(self.shape, self.nnz) > 0) == keeps_plan, (self.key, self.nnz)
        return keeps_plan

    def forward(self, c, ws):
        if self.assert_route():
            self.plan = self.nat.new_plan(self.shape, self.nnz, self.I.device)
        self.out = torch.full((self.B, self.D), float("nan"), device="cuda")
        self.nat.forward(self.shape, c, self.I, None, self.O, self.nnz, None, self.B, self.out, ws, self.plan)
        return self.out

    def backward(self, c, ws, plan="own"):
        _select(self.nat, self.case)
        g = [torch.full_like(x, float("nan")) for x in c]
        self.nat.backward_dense(self.shape, c, self.I, None, self.nnz, None, self.B, self.dY, g, ws,
                                self.plan if plan == "own" else plan, self.O)
        return g

    def refs(self):
        """(forward value, mag), per-core (value, mag, n) at the call's cores; memoised (the key names the cores)."""
        return _memo(self.seed, lambda: (orc.tt_forward64(self.ids, self.offs, self.cores, self.p, self.q, self.R),
                                         orc.tt_dense_backward64(self.ids, self.offs, self.dy, self.cores, self.p, self.q, self.R)))

    def depth(self, t, n):
        return fb.grad_depth(self.route, self.q, self.Rk, t, n, merged=len(self.p) != 3, pieces=self.pieces)

    def check_forward(self, what):
        (want, mag), _ = self.refs()
        depth = fb.bag_depth(self.route, self.Rk, np.diff(self.offs), pieces=self.pieces)
        _note(self.key, fb.assert_fp32_grade(self.out.cpu().numpy(), want, mag, depth, f"{self.key} {what} forward", "bag"))

    def check_grads(self, g, what, ref=None):
        ref = self.refs()[1] if ref is None else ref
        for t, (v, m, n) in enumerate(ref):
            got = g[t].cpu().numpy()
            _note(self.key, fb.assert_fp32_grade(got, v, m, self.depth(t, n), f"{self.key} {what} dG{t}", "core row"))
            fb.assert_untouched(got, np.zeros_like(got), n, f"{self.key} {what} dG{t}")


def _case_cores(case, seed=0):
    key, p, q, r = case[0], case[1], case[2], case[3]
    return _memo(("cores", key if not key.startswith("wide") else "wide", tuple(p), seed),
                 lambda: fb.scaled_cores(np.random.default_rng(1000 + seed + len(p) * 7 + r[0]), p, q, [1] + r + [1]))


@pytest.fixture
def restore(nat):
    yield
    nat.set_path(nat.PATH_AUTO)
    nat.set_piece_limits(0, 0)
    nat.set_wide_slab_min_ids(0)


ABI_ROUTES = ost.PLAN_ROUTES + CONTROLS
# Sizes of the three calls: n, about 2.5 n, about n / 3.  Where 2.5 n does not outgrow the 25 % of slack a Workspace
# allocates (tables sized by the number of groups dominate these workspaces), the middle call is larger: 2.8 n for the padded
# ranks.  The third call of the two AUTO-path routes stays past the 4 096-id crossover.
MIDDLE = {"padded_12_to_16": 2.8}
THIRD = {"padded_12_to_16": 5000, "merged_2core": 4500}
# Some routes cannot outgrow it with ids of the same route at a size a quick test can check: prefix_in_chain leaves its route
# at 16 400 ids and would need 24 000; group_products_in_chain would need 60 000 ids of a rank-32 chain and the wide chain
# 30 000 of a rank-64 one (float64 partials of hundreds of MB in the oracle); a call in pieces sizes its tables by the piece.
# There a fourth forward follows the middle one on the same Workspace: a grouped call on a larger table (17 500 groups: its
# tables need 23 MB, more than twice what any of these routes holds), which makes Workspace.get hand out a new buffer the
# way any larger call does.  It is checked against the oracle like the others and never gets a backward.
OUTGROWN_BY_ANOTHER_CALL = ("prefix_in_chain", "group_products_in_chain", "wide_e_table", "wide_lds_slabs", "pieces")
LARGER_TABLE = ("larger_table", [125, 140, 140], [4, 5, 5], [16, 16], 6000, "fast3", 3, 0, None, None)


@pytest.mark.parametrize("order", ["fifo", "lifo"])
@pytest.mark.parametrize("case", ABI_ROUTES, ids=[c[0] for c in ABI_ROUTES])
def test_three_forwards_then_their_backwards_on_one_workspace(nat, restore, case, order):
    """Forwards A, B, C (n, 2.5 n and n / 3 ids: other grouping layouts, regions of one call over another's; B, or on
    the routes of OUTGROWN_BY_ANOTHER_CALL a larger call behind it, makes the Workspace re-allocate), then the dense backwards in the order of the forwards or reversed.  After each backward: that call's
    forward output, kept since before the other calls ran, and its gradient alone."""
    n = case[4]
    cores = _case_cores(case)
    c = [_dev(x) for x in cores]
    ws = nat.Workspace()
    sizes = (n, int(MIDDLE.get(case[0], 2.5) * n), THIRD.get(case[0], n // 3))
    calls = [AbiCall(nat, case, cores, size, seed) for seed, size in enumerate(sizes)]
    calls[0].forward(c, ws)
    before = ws.buf.data_ptr()
    calls[1].forward(c, ws)
    if case[0] in OUTGROWN_BY_ANOTHER_CALL:
        assert ws.buf.data_ptr() == before, f"{case[0]}: the middle forward re-allocates by itself: take the route off the list"
        big_cores = _case_cores(LARGER_TABLE)
        filler = AbiCall(nat, LARGER_TABLE, big_cores, LARGER_TABLE[4], 0)
        filler.forward([_dev(x) for x in big_cores], ws)
        torch.cuda.synchronize()
        filler.check_forward("the larger call")
    assert ws.buf.data_ptr() != before, f"{case[0]}: the workspace was not re-allocated after the first forward"
    calls[2].forward(c, ws)
    plans = [x.plan for x in calls if x.plan is not None]
    assert len({pl.data_ptr() for pl in plans}) == len(plans)
    for k in ((0, 1, 2) if order == "fifo" else (2, 1, 0)):
        g = calls[k].backward(c, ws)
        torch.cuda.synchronize()
        calls[k].check_forward(f"{order} call {k}")
        calls[k].check_grads(g, f"{order} call {k}")
    nat.status()


@pytest.mark.parametrize("between", ["wide", "per_bag"])
def test_another_shape_runs_between_a_forward_and_its_backward(nat, restore, between):
    """A grouped 4.5.5 / 16 forward; on the same Workspace the forward AND backward of a wide 5.5.4 / 64 call (or of a per-bag
    call); then the first call's backward."""
    first_case = ost.PLAN_ROUTES[0]
    other_case = ost.PLAN_ROUTES[5] if between == "wide" else CONTROLS[0]
    cores, other_cores = _case_cores(first_case), _case_cores(other_case)
    c, oc = [_dev(x) for x in cores], [_dev(x) for x in other_cores]
    ws = nat.Workspace()
    first = AbiCall(nat, first_case, cores, first_case[4], 0)
    other = AbiCall(nat, other_case, other_cores, other_case[4], 0)
    first.forward(c, ws)
    other.forward(oc, ws)
    g_other = other.backward(oc, ws)
    g = first.backward(c, ws)
    torch.cuda.synchronize()
    other.check_forward(f"between ({between})")
    other.check_grads(g_other, f"between ({between})")
    first.check_forward(f"around {between}")
    first.check_grads(g, f"around {between}")
    nat.status()


@pytest.mark.parametrize("case", ost.PLAN_ROUTES, ids=[c[0] for c in ost.PLAN_ROUTES])
def test_a_backward_leaves_the_plan_as_the_forward_wrote_it(nat, restore, case):
    cores = _case_cores(case)
    c = [_dev(x) for x in cores]
    ws = nat.Workspace()
    call = AbiCall(nat, case, cores, case[4], 0)
    call.forward(c, ws)
    torch.cuda.synchronize()
    kept = call.plan.clone()
    for k in range(2):   # (not compared with each other: these routes sum with float atomics)
        g = call.backward(c, ws)
        torch.cuda.synchronize()
        assert torch.equal(call.plan, kept), f"{case[0]}: dense backward {k} wrote into the plan"
        call.check_grads(g, f"dense backward {k}")
    cs = [x.clone() for x in c]
    nat.backward_sgd(call.shape, cs, call.I, None, call.nnz, None, call.B, call.dY, LR, ws, call.plan, call.O)
    torch.cuda.synchronize()
    assert torch.equal(call.plan, kept), f"{case[0]}: the fused SGD backward wrote into the plan"
    for t, (v, m, n) in enumerate(call.refs()[1]):
        _note(case[0], fb.assert_sgd_grade(cs[t].cpu().numpy(), cores[t], v, fb.gamma(call.depth(t, n)) * m, LR, f"{case[0]} SGD core {t}"))
    nat.status()


# The merged 2- and 4-core tables are not here: their plan's P belongs to the 3-core VIEW the table runs on, not to the
# table's own chain (see outstanding.SAVED_P_ROUTES).
@pytest.mark.parametrize("case", ost.SAVED_P_ROUTES, ids=[c[0] for c in ost.SAVED_P_ROUTES])
def test_a_backward_on_the_plan_differentiates_at_the_forwards_prefix(nat, restore, case):
    """Forward with cores W; cores 0 and 1 overwritten with fresh draws W' (core 2 stays); then the backward WITH the plan is
    the gradient at the forward's P = G0[i0].G1[i1] (only dG2 sees it), the backward WITHOUT a plan the gradient at W'."""
    key, p, q, r, n = case[:5]
    W = _case_cores(case, seed=1)
    call = AbiCall(nat, case, W, n, 3)
    Wn = _memo(("fresh", call.seed), lambda: ost.fresh_prefix(np.random.default_rng(77), W, p, q, call.R))
    saved, current = _memo(("sp", call.seed), lambda: ost.saved_prefix_refs(call.ids, call.offs, call.dy, W, Wn, p, q, call.R))
    c = [_dev(x) for x in W]
    ws = nat.Workspace()
    call.forward(c, ws)
    ost.assert_separated(saved, current, call.depth(2, saved[2][2]), key)   # (on the host: the two answers exclude each other)
    for t in (0, 1):
        c[t].copy_(_dev(Wn[t]))
    g_plan = call.backward(c, ws)
    g_none = call.backward(c, ws, plan=None)
    torch.cuda.synchronize()
    call.check_forward("saved P")
    call.check_grads(g_plan, "with the plan (saved P)", ref=saved)
    call.check_grads(g_none, "without a plan (current P)", ref=current)
    nat.status()


def test_two_fused_sgd_steps_after_two_forwards(nat, restore):
    """Forwards 1 and 2 at W0 (grouped route, a plan each); the fused SGD backward of 1 gives W1, read back; the fused SGD
    backward of 2 then steps from W1: the expectation is W1 - lr g with g the oracle's gradient at (cores W1, prefix of W0).
    (The C ABI form of this case: W1 is the fp32 tensor the first step left, so the first step's error does not enter the
    second's bound.)  What this case pins is that the second step starts from W1 and that a plan survives another call's
    fused step.  It does NOT tell the two prefixes apart: W1 is one small step from W0, and inside the step's bound the
    saved-P and current-P expectations need not exclude each other (the share on which the gradients do is printed, no
    condition) -- test_a_backward_on_the_plan_differentiates_at_the_forwards_prefix does that, under its condition."""
    case = ost.PLAN_ROUTES[0]
    W0 = _case_cores(case)
    c = [_dev(x) for x in W0]
    ws = nat.Workspace()
    one, two = AbiCall(nat, case, W0, 20000, 0), AbiCall(nat, case, W0, 6666, 2)
    one.forward(c, ws)
    two.forward(c, ws)
    nat.backward_sgd(one.shape, c, one.I, None, one.nnz, None, one.B, one.dY, LR, ws, one.plan, one.O)
    torch.cuda.synchronize()
    W1 = _np(c)
    for t, (v, m, n) in enumerate(one.refs()[1]):
        _note("two_steps", fb.assert_sgd_grade(W1[t], W0[t], v, fb.gamma(one.depth(t, n)) * m, LR, f"step 1 core {t}"))
        fb.assert_untouched(W1[t], W0[t], n, f"step 1 core {t}")
    nat.backward_sgd(two.shape, c, two.I, None, two.nnz, None, two.B, two.dY, LR, ws, two.plan, two.O)
    torch.cuda.synchronize()
    W2 = _np(c)
    ref = orc.tt_dense_backward64(two.ids, two.offs, two.dy, W1, two.p, two.q, two.R, prefix_cores=W0)
    plain = orc.tt_dense_backward64(two.ids, two.offs, two.dy, W1, two.p, two.q, two.R)
    # (a record, not a condition: see the docstring)
    print(f"\n  two steps: saved-P and current-P expectations apart on {ost.separation(ref, plain, two.depth(2, ref[2][2])):.1%}", end="")
    for t, (v, m, n) in enumerate(ref):
        _note("two_steps", fb.assert_sgd_grade(W2[t], W1[t], v, fb.gamma(two.depth(t, n)) * m, LR, f"step 2 core {t}"))
        fb.assert_untouched(W2[t], W1[t], n, f"step 2 core {t}")
    one.check_forward("two steps, call 1")
    two.check_forward("two steps, call 2")
    nat.status()


# =====================================================================================================================
# 2. module: several lookups through one TTEmbeddingBag before backward
# =====================================================================================================================
P, Q, R = ost.P, ost.Q, ost.RANKS
N_EMB, D = int(np.prod(P)), int(np.prod(Q))
N_BIG, N_SMALL = 6000, 700   # grouped / per bag: both kernel families in one autograd graph
PAD = 1234567 % N_EMB

# variant -> (constructor keywords, per-call mode or None, weighted, padded, 2-D, bags of one under the pooling, _use_lean)
VARIANTS = {
    "sum_lean": ({}, None, False, False, False, False, True),
    "sum_general": ({}, None, False, False, False, False, False),
    "weighted": ({}, None, True, False, False, True, True),
    "mean": ({"mode": "mean"}, None, False, False, False, False, True),
    "max": ({}, "max", False, False, False, True, True),
    "pad_partition": ({"padding_idx": PAD}, None, False, True, False, False, True),
    "pad_masked": ({"padding_idx": PAD}, None, False, True, False, True, True),
    "two_d": ({}, None, False, False, True, False, True),
    "exact": ({"deterministic": True}, None, False, False, False, False, True),
}


def _module_cores(seed=0):
    return _memo(("module cores", seed), lambda: fb.scaled_cores(np.random.default_rng(500 + seed), P, Q, R))


def _emb(ops, variant, sparse, cores=None, **kw):
    ctor = dict(VARIANTS[variant][0])
    ctor.update(kw)
    emb = ops.TTEmbeddingBag(N_EMB, D, R[1:3], P, Q, sparse=sparse, use_cache=False, weight_dist="uniform",
                             learning_rate=LR, eps=EPS, **ctor)
    emb._use_lean = VARIANTS[variant][6]
    if variant.startswith("pad_"):
        emb._pad_partition = variant == "pad_partition"
    with torch.no_grad():
        for c, x in zip(emb.tt_cores, _module_cores() if cores is None else cores):
            c.copy_(_dev(x)[None])
    return emb


class Lookup:
    """One call through a module: inputs (tests/fp32_bound.py), the call itself, and its float64 oracle with depths."""

    def __init__(self, variant, n_ids, seed, zero_dy=False):
        self.variant, self.n_ids, self.seed = variant, n_ids, seed
        _, self.mode, self.weighted, self.padded, self.two_d, self.ones, _ = VARIANTS[variant]
        self.ctor_mode = VARIANTS[variant][0].get("mode", "sum")
        rng = np.random.default_rng(9000 + seed + n_ids)
        if self.two_d:
            ids = fb.skewed_bags(rng, P, n_ids, long_bag=0)[0]
            self.L = 3
            ids = ids[: (ids.shape[0] // self.L) * self.L]
            offs = np.arange(0, ids.shape[0] + 1, self.L, dtype=np.int64)
        else:
            ids, offs = fb.skewed_bags(rng, P, n_ids)
        if self.padded:
            ids[::13] = PAD
        self.ids, self.offs = ids, offs
        self.nnz, self.B = ids.shape[0], offs.shape[0] - 1
        self.dy = fb.scaled_dy(rng, self.B, D)
        self.w = fb.sample_weights(rng, self.nnz) if self.weighted else None
        if zero_dy:
            self.dy = np.zeros_like(self.dy)
        self.I, self.O = _dev(ids), _dev(offs)
        self.wt = None
        self.key = (variant, n_ids, seed, zero_dy)

    def run(self, emb, nat):
        """The forward, after asserting the kernels it will take."""
        nat.set_path(nat.PATH_AUTO)
        fam = nat.kernel_family(emb._shape, self.nnz, self.nnz if self.ones else self.B, True)
        want = nat.FAMILY_GROUPED if self.nnz > 4096 else nat.FAMILY_PER_BAG
        if self.variant != "exact":   # (the exact kernels are no family of the plain dispatch)
            assert fam & 7 == want, (self.variant, self.nnz, fam)
        self.route = "exact" if self.variant == "exact" else _route(fam, nat)
        self.wt = _dev(self.w).requires_grad_(True) if self.weighted else None
        if self.two_d:
            out = emb(self.I.view(-1, self.L))
        else:
            out = emb(self.I, self.O, per_sample_weights=self.wt, mode=self.mode)
        if self.padded:
            expect = "partition" if (self.variant == "pad_partition" and self.nnz > 4096) else "masked"
            assert emb._last_pad_route == expect, (self.variant, self.nnz, emb._last_pad_route)
            self.pad_route = expect
        if self.variant == "exact":   # the route of this variant: the exact kernels' autograd node, nothing else
            assert type(out.grad_fn).__name__.startswith("_ExactLookup"), type(out.grad_fn).__name__
        self.out = out
        return out

    # ---- oracle ----
    def _kw(self):
        return dict(weights=self.w, mode=self.ctor_mode, pad=PAD if self.padded else None)

    def _max_refs(self, cores):
        """mode="max" in float64: the winner of every (bag, column) from the float64 rows; dY is zeroed beforehand on the
        pairs whose two largest rows are closer than the rows' own fp32 bound (the winner is not defined there)."""
        ones = np.arange(self.nnz + 1, dtype=np.int64)
        rows, rmag = orc.tt_forward64(self.ids, ones, cores, P, Q, R)
        slack = fb.gamma(fb.row_depth("grouped", R) + 2) * rmag
        want, mag = np.zeros((self.B, D)), np.zeros((self.B, D))
        d_rows = np.zeros((self.nnz, D), dtype=np.float32)
        ties, dy = 0, self.dy.copy()
        for b in range(self.B):
            lo, hi = int(self.offs[b]), int(self.offs[b + 1])
            if hi == lo:
                continue
            seg = rows[lo:hi]
            win = np.argmax(seg, axis=0)
            cols = np.arange(D)
            top = seg[win, cols]
            want[b], mag[b] = top, rmag[lo:hi][win, cols]
            if hi - lo > 1:
                rest = seg.copy()
                rest[win, cols] = -np.inf
                second = np.argmax(rest, axis=0)
                near = top - rest[second, cols] <= slack[lo:hi][win, cols] + slack[lo:hi][second, cols]
                ties += int(near.sum())
                dy[b, near] = 0.0
            d_rows[lo + win, cols] = dy[b]
        assert ties <= 0.01 * self.B * D, f"{ties} near ties among the bag maxima: choose other inputs"   # (an id twice in a bag is one)
        return (want, mag), orc.tt_dense_backward64(self.ids, ones, d_rows, cores, P, Q, R), dy

    def refs(self, cores):
        def make():
            if self.mode == "max":
                return self._max_refs(cores)
            return (orc.tt_forward64(self.ids, self.offs, cores, P, Q, R, **self._kw()),
                    orc.tt_dense_backward64(self.ids, self.offs, self.dy, cores, P, Q, R, **self._kw()))
        got = _memo(("lookup", self.key, _crc(cores)), make)
        fwd, g = got[:2]
        if self.mode == "max":
            self.dy = got[2]   # (the masked dY belongs to the oracle's answer: every Lookup of these inputs runs with it)
        wref = None
        if self.weighted:
            g, wref = g
        return fwd, g, wref

    def prepare(self, cores):
        """(max: the oracle decides which dY elements are zeroed as near ties, so it runs before dY goes to the device)"""
        self.refs(cores)
        self.dY = _dev(self.dy)

    def fwd_depth(self):
        """Of the route run() asserted and of "grouped", as test_module_paths_within_the_fp32_bound takes it.  A max bag is
        ONE looked-up row (a bag of one), whatever the bag's length."""
        lens = np.ones(self.B, dtype=np.int64) if self.mode == "max" else np.diff(self.offs)
        reduce = self.weighted or (self.padded and self.pad_route == "masked")
        d = np.maximum(fb.bag_depth(self.route, R, lens, reduce=reduce), fb.bag_depth("grouped", R, lens, reduce=reduce))
        return d + (2 if self.ctor_mode == "mean" else 0)

    def grad_depths(self, ref):
        out = []
        for t, (_, _, n) in enumerate(ref):
            out.append(np.maximum(fb.grad_depth(self.route, Q, R, t, n, scaled=True), fb.grad_depth("grouped", Q, R, t, n, scaled=True)))
        return out

    def check_forward(self, cores, what, got=None):
        (want, mag), _, _ = self.refs(cores)
        got = self.out if got is None else got
        _note("module_" + self.variant, fb.assert_fp32_grade(got.detach().cpu().numpy(), want, mag, self.fwd_depth(),
                                                             f"{self.variant} {what} forward", "bag"))

    def check_wgrad(self, cores, what, times=1):
        if not self.weighted:
            return
        _, _, (wv, wm) = self.refs(cores)
        depth = max(fb.wgrad_depth(self.route, Q, R), fb.wgrad_depth("grouped", Q, R)) + (times - 1)
        _note("module_" + self.variant, fb.assert_fp32_grade(self.wt.grad.cpu().numpy(), times * wv, times * wm, depth,
                                                             f"{self.variant} {what} w.grad", "id"))


def _pair(variant, big_first=True, zero_second=False):
    a, b = Lookup(variant, N_BIG, 1), Lookup(variant, N_SMALL, 2, zero_dy=zero_second)
    return (a, b) if big_first else (b, a)


def _check_core_grads(emb, cores, calls, what, variant):
    refs = [x.refs(cores)[1] for x in calls]
    depths = [x.grad_depths(r) for x, r in zip(calls, refs)]
    got = [c.grad[0].cpu().numpy() for c in emb.tt_cores]
    _note("module_" + variant, ost.assert_summed(got, refs, depths, f"{variant} {what}"))


@pytest.mark.parametrize("how", ["joint", "joint_small_first", "first_then_second", "second_then_first"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_two_lookups_before_backward_dense(nat, ops, variant, how):
    """o1 = emb(...), o2 = emb(...) (about 6 000 ids grouped and 700 per bag, created in either order), then ONE
    autograd.backward over both, or two separate backwards in either order: every c.grad is g1 + g2 within the bound of
    one more rounding, rows neither call touches are exact zeros, both outputs (read after the other forward ran) and each
    call's w.grad are its own."""
    cores = _module_cores()
    emb = _emb(ops, variant, sparse=False)
    one, two = _pair(variant, big_first=how != "joint_small_first")
    for x in (one, two):
        x.prepare(cores)
    o1 = one.run(emb, nat)
    o2 = two.run(emb, nat)
    if how.startswith("joint"):
        torch.autograd.backward([o1, o2], [one.dY, two.dY])
    elif how == "first_then_second":
        o1.backward(one.dY)
        o2.backward(two.dY)
    else:
        o2.backward(two.dY)
        o1.backward(one.dY)
    torch.cuda.synchronize()
    for x in (one, two):
        x.check_forward(cores, how)
        x.check_wgrad(cores, how)
    _check_core_grads(emb, cores, [one, two], how, variant)
    nat.status()


@pytest.mark.parametrize("variant", ["sum_general", "weighted", "mean", "max", "pad_partition"])
def test_retain_graph_runs_one_backward_twice(nat, ops, variant):
    cores = _module_cores()
    emb = _emb(ops, variant, sparse=False)
    one = Lookup(variant, N_BIG, 1)
    one.prepare(cores)
    o1 = one.run(emb, nat)
    o1.backward(one.dY, retain_graph=True)
    o1.backward(one.dY)
    torch.cuda.synchronize()
    one.check_forward(cores, "retain_graph")
    one.check_wgrad(cores, "retain_graph", times=2)
    _check_core_grads(emb, cores, [one, one], "retain_graph", variant)   # 2 g1, one more rounding
    nat.status()


def _state(emb):
    return [s[0].clone() for s in emb.optimizer_state]


@pytest.mark.parametrize("zero_first", [True, False], ids=["zero_first", "real_first"])
@pytest.mark.parametrize("optimizer", ["SGD", "EXACT_ADAGRAD"])
@pytest.mark.parametrize("variant", ["sum_lean", "sum_general", "weighted", "max", "pad_partition"])
def test_fused_steps_with_two_lookups_open(nat, ops, variant, optimizer, zero_first):
    """sparse=True.  Forward 1, forward 2; the backward of 2 carries dY = 0 -- an exactly zero gradient, and w - lr 0 and
    s + 0^2 are exact, so it must leave cores and state bit for bit (whenever it runs) -- and the backward of 1 is the
    oracle's step for call 1 alone."""
    cores = _module_cores()
    adagrad = optimizer == "EXACT_ADAGRAD"
    emb = _emb(ops, variant, sparse=True, optimizer=getattr(ops.OptimType, optimizer))
    st0 = [np.zeros_like(c) for c in cores]
    one, two = _pair(variant, zero_second=True)
    for x in (one, two):
        x.prepare(cores)
    o1 = one.run(emb, nat)
    o2 = two.run(emb, nat)
    if not zero_first:
        o1.backward(one.dY)
    torch.cuda.synchronize()
    before = [c.detach()[0].clone() for c in emb.tt_cores], (_state(emb) if adagrad else [])
    o2.backward(two.dY)
    torch.cuda.synchronize()
    for t, c in enumerate(emb.tt_cores):
        assert torch.equal(c.detach()[0], before[0][t]), f"{variant}: the zero-gradient backward changed core {t}"
    for t, s in enumerate(before[1]):
        assert torch.equal(emb.optimizer_state[t][0], s), f"{variant}: the zero-gradient backward changed state {t}"
    if zero_first:
        o1.backward(one.dY)
        torch.cuda.synchronize()
    one.check_forward(cores, "fused")
    two.check_forward(cores, "fused")
    ref = one.refs(cores)[1]
    for t, ((v, m, n), d) in enumerate(zip(ref, one.grad_depths(ref))):
        got, delta = emb.tt_cores[t].detach()[0].cpu().numpy(), fb.gamma(d) * m
        what = f"{variant} {optimizer} core {t}"
        if adagrad:
            s = emb.optimizer_state[t][0].cpu().numpy()
            _note("fused_" + variant, fb.assert_adagrad_grade(got, s, cores[t], st0[t], v, delta, LR, EPS, what))
            fb.assert_untouched(s, st0[t], n, what + " state")
        else:
            _note("fused_" + variant, fb.assert_sgd_grade(got, cores[t], v, delta, LR, what))
        fb.assert_untouched(got, cores[t], n, what)
    nat.status()


@pytest.mark.parametrize("empty_first", [True, False], ids=["empty_first", "real_first"])
def test_adam_with_an_empty_lookup_open(nat, ops, empty_first):
    """ADAM: a zero gradient still advances t, so the second call is an EMPTY one (0 ids, B bags) -- the documented no-op
    that leaves t, the moments and the cores alone."""
    cores = _module_cores()
    emb = _emb(ops, "sum_lean", sparse=True, optimizer=ops.OptimType.ADAM)
    one = Lookup("sum_lean", N_BIG, 1)
    one.prepare(cores)
    B2 = 40
    o1 = one.run(emb, nat)
    o2 = emb(torch.empty(0, dtype=torch.int64, device="cuda"), torch.zeros(B2 + 1, dtype=torch.int64, device="cuda"))
    dy2 = _dev(fb.scaled_dy(np.random.default_rng(3), B2, D))
    if not empty_first:
        o1.backward(one.dY)
    torch.cuda.synchronize()
    before = [x.clone() for x in list(emb.tt_cores) + list(emb.optimizer_state) + list(emb.optimizer_state_v)] + [emb.adam_step[:, 0].clone()]
    o2.backward(dy2)
    torch.cuda.synchronize()
    after = list(emb.tt_cores) + list(emb.optimizer_state) + list(emb.optimizer_state_v) + [emb.adam_step[:, 0]]
    for k, (a, b) in enumerate(zip(after, before)):
        assert torch.equal(a.detach(), b.detach()), f"the empty call's backward changed tensor {k}"
    if empty_first:
        o1.backward(one.dY)
        torch.cuda.synchronize()
    assert int(emb.adam_step[0, 0]) == 1
    assert torch.equal(o2.detach(), torch.zeros_like(o2))
    one.check_forward(cores, "adam")
    hp = ab.Hyper(LR, EPS)
    ref = one.refs(cores)[1]
    for t, ((v, m, n), d) in enumerate(zip(ref, one.grad_depths(ref))):
        z = np.zeros_like(cores[t])
        r = ab.assert_adam_grade(emb.tt_cores[t].detach()[0].cpu().numpy(), emb.optimizer_state[t][0].cpu().numpy(),
                                 emb.optimizer_state_v[t][0].cpu().numpy(), cores[t], z, z, v, fb.gamma(d) * m, 1, hp,
                                 f"adam core {t}")
        _note("fused_adam (err / bound)", r)
    nat.status()


@pytest.mark.parametrize("n_train", [2000, N_BIG], ids=["per_bag", "grouped"])
@pytest.mark.parametrize("variant", ["sum_lean", "weighted"])
def test_an_inference_forward_between_forward_and_backward(nat, ops, variant, n_train):
    cores = _module_cores()
    emb = _emb(ops, variant, sparse=False)
    one, big = Lookup(variant, n_train, 5), Lookup(variant, 60000, 6)
    one.prepare(cores)
    o1 = one.run(emb, nat)
    before = emb._ws.buf.data_ptr()
    with torch.no_grad():
        nat.set_path(nat.PATH_AUTO)
        assert nat.kernel_family(emb._shape, big.nnz, big.nnz if big.ones else big.B, True) & 7 == nat.FAMILY_GROUPED
        big.route = "grouped"
        inf = emb(big.I, big.O, per_sample_weights=_dev(big.w) if big.weighted else None)
    assert emb._ws.buf.data_ptr() != before, "the inference forward did not re-allocate the module's workspace"
    o1.backward(one.dY)
    torch.cuda.synchronize()
    big.check_forward(cores, "inference", got=inf)
    one.check_forward(cores, "around an inference forward")
    one.check_wgrad(cores, "around an inference forward")
    _check_core_grads(emb, cores, [one], "around an inference forward", variant)
    nat.status()


def _backward_all(outs, dys, how):
    """One autograd.backward over every output, or one backward per output in the order of the forwards or reversed."""
    if how == "joint":
        torch.autograd.backward(list(outs), list(dys))
    else:
        pairs = list(zip(outs, dys))
        for o, dy in (pairs if how == "in_order" else pairs[::-1]):
            o.backward(dy)


HOW = ["joint", "in_order", "reversed"]


@pytest.mark.parametrize("how", HOW)
def test_three_tables_two_lookups_before_backward(nat, ops, how):
    """TableBatchedTTEmbeddingBag with three tables (one window per table, bounds read on the device), two calls, one
    backward over both."""
    Tn = 3
    rng = np.random.default_rng(61)
    tabs = [fb.scaled_cores(rng, P, Q, R) for _ in range(Tn)]
    emb = ops.TableBatchedTTEmbeddingBag(Tn, N_EMB, D, R[1:3], P, Q, sparse=False, use_cache=False, weight_dist="uniform")
    with torch.no_grad():
        for t, c in enumerate(emb.tt_cores):
            c.copy_(_dev(np.stack([tabs[k][t] for k in range(Tn)])))
    nat.set_path(nat.PATH_AUTO)
    calls = []
    for n_ids in (N_BIG, N_SMALL):
        parts = [fb.skewed_bags(rng, P, n_ids // Tn * (k + 1) // 2 + 200, long_bag=0) for k in range(Tn)]
        B = max(o.shape[0] - 1 for _, o in parts)
        lens = [np.concatenate([np.diff(o), np.zeros(B - (o.shape[0] - 1), dtype=np.int64)]) for _, o in parts]
        ids = np.concatenate([i for i, _ in parts])
        offs = np.concatenate([[0], np.cumsum(np.concatenate(lens))]).astype(np.int64)
        assert nat.window_workspace_bytes(emb._shape, nat.OP_BACKWARD, ids.shape[0], Tn * B, B) >= 0   # the windows serve it
        calls.append((ids, offs, B, fb.scaled_dy(rng, Tn * B, D).reshape(Tn, B, D)))
    outs = [emb(_dev(ids), _dev(offs)) for ids, offs, _, _ in calls]
    _backward_all(outs, [_dev(dy) for _, _, _, dy in calls], how)
    torch.cuda.synchronize()
    for k in range(Tn):
        refs, depths = [], []
        for (ids, offs, B, dy), out in zip(calls, outs):
            ids_k = ids[offs[k * B]:offs[(k + 1) * B]]
            offs_k = offs[k * B:(k + 1) * B + 1] - offs[k * B]
            want, mag = orc.tt_forward64(ids_k, offs_k, tabs[k], P, Q, R)
            _note("module_tables", fb.assert_fp32_grade(out[k].detach().cpu().numpy(), want, mag,
                                                        fb.bag_depth("grouped", R, np.diff(offs_k)), f"table {k} forward", "bag"))
            ref = orc.tt_dense_backward64(ids_k, offs_k, dy[k], tabs[k], P, Q, R)
            refs.append(ref)
            depths.append([fb.grad_depth("grouped", Q, R, t, n) for t, (_, _, n) in enumerate(ref)])
        got = [c.grad[k].cpu().numpy() for c in emb.tt_cores]
        _note("module_tables", ost.assert_summed(got, refs, depths, f"table {k}"))
    nat.status()


@pytest.mark.parametrize("how", HOW)
def test_data_parallel_bucket_takes_two_lookups_before_its_step(nat, ops, how):
    """TTDataParallel at world size 1: the first backward writes the flat bucket, the second is added to it; after
    dp.step() the cores are W - lr (g1 + g2)."""
    from ttemb_dist import TTDataParallel
    cores = _module_cores()
    emb = _emb(ops, "sum_lean", sparse=False)
    dp = TTDataParallel(emb)
    assert dp.world == 1
    one, two = _pair("sum_lean")
    for x in (one, two):
        x.prepare(cores)
    o1 = one.run(emb, nat)
    o2 = two.run(emb, nat)
    assert type(o1.grad_fn).__name__.startswith("_BucketLookup"), type(o1.grad_fn).__name__
    _backward_all([o1, o2], [one.dY, two.dY], how)
    dp.step()
    torch.cuda.synchronize()
    one.check_forward(cores, "bucket")
    two.check_forward(cores, "bucket")
    refs = [x.refs(cores)[1] for x in (one, two)]
    depths = [x.grad_depths(r) for x, r in zip((one, two), refs)]
    for t, (v, m, n, d) in enumerate(ost.summed(refs, depths)):
        got = emb.tt_cores[t].detach()[0].cpu().numpy()
        _note("module_bucket", fb.assert_sgd_grade(got, cores[t], v, fb.gamma(d) * m, LR, f"bucket core {t}"))
        fb.assert_untouched(got, cores[t], n, f"bucket core {t}")
    nat.status()


@pytest.mark.parametrize("how", HOW)
def test_live_row_cache_two_lookups_before_backward(nat, ops, how):
    """A live row cache: the cached ids' gradient goes to cache_weight.grad, the others' to the cores; both tensors take
    two calls."""
    cores = _module_cores()
    emb = ops.TTEmbeddingBag(N_EMB, D, R[1:3], P, Q, sparse=False, use_cache=True, cache_size=300, hashtbl_size=N_EMB,
                             weight_dist="uniform", learning_rate=LR)
    with torch.no_grad():
        for c, x in zip(emb.tt_cores, cores):
            c.copy_(_dev(x)[None])
    one, two = _pair("sum_general")
    with torch.no_grad():
        emb(one.I, one.O)   # warm-up statistics
        emb(two.I, two.O)
    emb.cache_populate()
    assert not emb.warmup
    torch.cuda.synchronize()
    hashtbl, state = emb.hashtbl.cpu().numpy(), emb.cache_state.cpu().numpy()
    cache_rows = emb.cache_weight.detach().cpu().numpy()
    nat.set_path(nat.PATH_AUTO)
    for x in (one, two):
        x.dY = _dev(x.dy)
        x.route = _route(nat.kernel_family(emb._shape, x.nnz, x.B, False), nat)   # (a live cache: the row-index form)
    assert one.route == "grouped" and two.route != "grouped", (one.route, two.route)
    o1, o2 = emb(one.I, one.O), emb(two.I, two.O)
    _backward_all([o1, o2], [one.dY, two.dY], how)
    torch.cuda.synchronize()
    refs, depths = [], []
    cv, cm, cn = np.zeros(cache_rows.shape), np.zeros(cache_rows.shape), np.zeros(cache_rows.shape[0], dtype=np.int64)
    for x, out in ((one, o1), (two, o2)):
        is_tt, loc = orc.cache_lookup(x.ids, hashtbl, state)
        assert 0 < (~is_tt).sum() < x.nnz   # ids on both sides: in the cache and in the cores
        keep = is_tt.astype(np.float32)   # the TT part of the call is the weighted call with weight 0 on the cached ids
        want, mag = orc.tt_forward64(x.ids, x.offs, cores, P, Q, R, weights=keep)
        rowidx = orc.rowidx_from_offsets(x.offs, x.nnz)
        np.add.at(want, rowidx[~is_tt], cache_rows[loc[~is_tt]].astype(np.float64))
        np.add.at(mag, rowidx[~is_tt], np.abs(cache_rows[loc[~is_tt]]).astype(np.float64))
        depth = np.maximum(fb.bag_depth("grouped", R, np.diff(x.offs)), fb.bag_depth(x.route, R, np.diff(x.offs))) + np.diff(x.offs)[:, None]
        _note("module_cache", fb.assert_fp32_grade(out.detach().cpu().numpy(), want, mag, depth, "cache forward", "bag"))
        ref, _ = orc.tt_dense_backward64(x.ids, x.offs, x.dy, cores, P, Q, R, weights=keep)
        refs.append(ref)
        depths.append(x.grad_depths(ref))
        np.add.at(cv, loc[~is_tt], x.dy.astype(np.float64)[rowidx[~is_tt]])
        np.add.at(cm, loc[~is_tt], np.abs(x.dy).astype(np.float64)[rowidx[~is_tt]])
        np.add.at(cn, loc[~is_tt], 1)
    _check = [c.grad[0].cpu().numpy() for c in emb.tt_cores]
    _note("module_cache", ost.assert_summed(_check, refs, depths, "cache"))
    got = emb.cache_weight.grad.cpu().numpy()
    _note("module_cache", fb.assert_fp32_grade(got, cv, cm, cn[:, None] + 2, "cache_weight.grad", "cache row"))
    fb.assert_untouched(got, np.zeros_like(got), cn, "cache_weight.grad")
    nat.status()


@pytest.mark.parametrize("kind", ["capture", "capture_bags_mean"])
def test_an_eager_lookup_between_a_captured_forward_and_its_backward(nat, ops, kind):
    """A captured lookup owns its workspace and plan: an eager call of three times the size through the same module (with
    dY = 0, so that it may not move the cores) between the captured forward and the captured backward changes nothing."""
    cores = _module_cores()
    emb = _emb(ops, "sum_lean", sparse=True)
    mean = kind == "capture_bags_mean"
    one = Lookup("mean" if mean else "sum_lean", N_BIG, 7)
    eager = Lookup("sum_lean", 3 * N_BIG, 8, zero_dy=True)
    one.prepare(cores)
    eager.prepare(cores)
    nat.set_path(nat.PATH_AUTO)
    assert nat.kernel_family(emb._shape, one.nnz, one.B, True) & 7 == nat.FAMILY_GROUPED
    one.route = "grouped"
    cap = emb.capture_bags(one.nnz, one.B, mode="mean") if mean else emb.capture(one.nnz, one.B, one.O)
    out = cap(one.I, one.O)
    first = out.detach().clone()
    o2 = eager.run(emb, nat)
    o2.backward(eager.dY)
    torch.cuda.synchronize()
    for t, c in enumerate(emb.tt_cores):
        assert np.array_equal(c.detach()[0].cpu().numpy().view(np.uint32), cores[t].view(np.uint32)), \
            f"the eager zero-gradient step changed core {t}"
    eager.check_forward(cores, "eager between")
    one.check_forward(cores, f"{kind} before the eager call", got=first)
    one.check_forward(cores, f"{kind} after the eager call", got=out)
    out.backward(one.dY)
    torch.cuda.synchronize()
    ref = one.refs(cores)[1]
    for t, ((v, m, n), d) in enumerate(zip(ref, one.grad_depths(ref))):
        got = emb.tt_cores[t].detach()[0].cpu().numpy()
        _note("captured_" + kind, fb.assert_sgd_grade(got, cores[t], v, fb.gamma(d) * m, LR, f"{kind} core {t}"))
        fb.assert_untouched(got, cores[t], n, f"{kind} core {t}")
    # the documented overwrite: the results of two calls are views of ONE static buffer
    again = cap(one.I, one.O)
    assert again.data_ptr() == out.data_ptr()
    nat.status()
