"""Every lookup route against the float64 oracle, element by element, with the fp32 rounding bound of tests/fp32_bound.py
(depth taken from the kernel that ran).  Inputs where a per-element check matters: core rows scaled by 10^U(-3, 0) with
mixed signs (and the module's uniform / approx-uniform initialisers), dY rows scaled per bag, weights with zeros and
negative values, skewed ids (hot rows, rows touched once, rows not touched), bags of 0 / 1 / 2 / 3 / 7 ids and one of 600.
Each case first asserts which route it takes, so that no case drifts onto another kernel silently."""
import numpy as np
import pytest
import torch

import fp32_bound as fb
from abi_check import EPS, LR, WORST, _abi_run, _check_all, _dev, _inputs, _note, _route
from oracle import tt_oracle as orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nat():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import ttemb_native
    yield ttemb_native
    ttemb_native.set_path(ttemb_native.PATH_AUTO)
    ttemb_native.set_piece_limits(0, 0)
    ttemb_native.set_wide_slab_min_ids(0)
    for k in sorted(WORST):
        print(f"\n  {k:28s} largest err/(u mag) {WORST[k]:.2f}", end="")


# (key, p, q, inner ranks, ids, path, wanted family without route flags, route flag that must be set or None, kernel ranks)
ABI_CASES = [
    ("generic", [23, 290, 310], [4, 5, 5], [16, 16], 4000, "generic", 0, None, None),
    ("small3", [23, 290, 310], [4, 5, 5], [16, 16], 2000, "auto", 1, None, None),
    ("rt3", [23, 290, 310], [6, 4, 4], [16, 16], 2000, "auto", 2, None, None),
    ("fast3", [8, 20, 3000], [4, 5, 5], [16, 16], 20000, "fast3", 3, None, None),
    ("prefix_in_chain", [41, 50, 30], [4, 5, 5], [16, 16], 6000, "fast3", 3, "prefix", None),
    ("group_products_in_chain", [41, 50, 30], [8, 4, 4], [32, 32], 6000, "fast3", 3, "group_products", None),
    ("padded_12_to_16", [40, 50, 60], [4, 5, 5], [12, 12], 12000, "auto", 3 | 32, None, [16, 16]),
    ("merged_2core", [7, 33], [16, 8], [16], 9000, "auto", 3 | 16, None, None),
    ("merged_4core", [12, 9, 14, 11], [5, 5, 2, 2], [16, 16, 16], 15000, "fast3", 3 | 16, None, None),
]


@pytest.mark.parametrize("case", ABI_CASES, ids=[c[0] for c in ABI_CASES])
def test_route_within_the_fp32_bound(nat, case):
    key, p, q, r, n_ids, path, want_fam, flag, rk = case
    R, Rk = [1] + r + [1], [1] + (rk or r) + [1]
    nat.set_path({"auto": nat.PATH_AUTO, "generic": nat.PATH_GENERIC, "fast3": nat.PATH_FAST3}[path])
    cores, ids, offs, dy, st0 = _inputs(p, q, R, n_ids, seed=len(key) + n_ids)
    shape = nat.make_shape(p, q, R)
    fam = nat.kernel_family(shape, ids.shape[0], offs.shape[0] - 1, True)
    assert fam & ~nat.FAMILY_ROUTE_FLAGS == want_fam, (key, fam)
    if flag == "prefix":
        assert fam & nat.FAMILY_PREFIX_IN_CHAIN, (key, fam)
    if flag == "group_products":
        assert fam & nat.FAMILY_GROUP_PRODUCTS_IN_CHAIN, (key, fam)
    res = _abi_run(nat, p, q, R, cores, ids, offs, dy, st0, plan=want_fam & 7 >= 3)
    route = _route(fam, nat)
    if len(p) != 3:   # a merged table: depths of the real chain, plus the split of the merged core's gradient
        _check_all(key, route, p, q, R, Rk, cores, ids, offs, dy, st0, *res, merged=True)
    else:
        _check_all(key, route, p, q, R, Rk, cores, ids, offs, dy, st0, *res)


@pytest.mark.parametrize("form", ["e_table", "lds_slabs"])
@pytest.mark.parametrize("shape", [(5, 5, 4, 64, 64), (4, 4, 8, 256, 256)])
def test_wide_rank_chain_within_the_fp32_bound(nat, shape, form):
    q, R = list(shape[:3]), [1, shape[3], shape[4], 1]
    p = [13, 50, 40]
    nat.set_path(nat.PATH_FAST3)
    nat.set_wide_slab_min_ids(1 if form == "lds_slabs" else 1 << 40)
    cores, ids, offs, dy, st0 = _inputs(p, q, R, 3000, seed=sum(shape))
    fam = nat.kernel_family(nat.make_shape(p, q, R), ids.shape[0], offs.shape[0] - 1, True)
    assert fam & 7 == nat.FAMILY_GROUPED_WIDE, fam
    res = _abi_run(nat, p, q, R, cores, ids, offs, dy, st0, plan=True)
    _check_all(f"wide_r{shape[3]}_{form}", "wide", p, q, R, R, cores, ids, offs, dy, st0, *res)


def test_call_in_pieces_within_the_fp32_bound(nat):
    p, q, R = [30, 35, 400], [4, 5, 5], [1, 16, 16, 1]
    nat.set_path(nat.PATH_FAST3)
    cores, ids, offs, dy, st0 = _inputs(p, q, R, 12000, seed=17)
    shape = nat.make_shape(p, q, R)
    assert nat.plan_bytes(shape, ids.shape[0]) > 0
    nat.set_piece_limits(900, 700)
    assert nat.plan_bytes(shape, ids.shape[0]) == 0   # a call in pieces keeps no plan
    assert nat.kernel_family(shape, ids.shape[0], offs.shape[0] - 1, True) & 7 == nat.FAMILY_GROUPED
    B = offs.shape[0] - 1
    pieces = -(-ids.shape[0] // 700) + -(-B // 900) + 1
    res = _abi_run(nat, p, q, R, cores, ids, offs, dy, st0)
    _check_all("pieces", "grouped", p, q, R, R, cores, ids, offs, dy, st0, *res, pieces=pieces)


# Adagrad behind the routes that write gradients first and step them afterwards, one launch for every core: padded ranks, the
# merged views of a 4-core and of a 2-core table on the grouped kernels, a call in pieces, and the tiny 2- and 4-core tables
# of test_gpu_device_lr.py on whatever kernels the library picks for them (none of which steps by itself).  Shapes and id
# counts of test_gpu_device_lr.py (test_padded_rank, test_two_and_four_core_tables, test_a_call_in_pieces); the grouped
# merged views need the larger tables of ABI_CASES.  One id per bag, as there.
# (key, p, q, inner ranks, ids, path, piece limit, family & 7 or None, route flag that must be set, kernel ranks)
STEP_CASES = [
    ("padded_rank", [8, 10, 10], [4, 5, 5], [12, 12], 4096, "fast3", 0, 3, 32, [16, 16]),
    ("merged_4core", [12, 9, 14, 11], [5, 5, 2, 2], [16, 16, 16], 4096, "fast3", 0, 3, 16, None),
    ("lifted_2core", [7, 33], [16, 8], [16], 4096, "fast3", 0, 3, 16, None),
    ("pieces", [8, 10, 10], [4, 5, 5], [16, 16], 4096, "fast3", 1400, 3, 0, None),
    ("tiny_2core", [6, 7], [4, 3], [5], 300, "auto", 0, None, 0, None),
    ("tiny_4core", [3, 2, 4, 3], [2, 2, 3, 2], [3, 4, 2], 300, "auto", 0, None, 0, None),
]


@pytest.mark.parametrize("case", STEP_CASES, ids=[c[0] for c in STEP_CASES])
def test_adagrad_step_behind_a_gradient_writing_route(nat, case):
    """The rate by value and from a device word: cores and state of both against the float64 oracle, per element, with the
    bound the fused Adagrad case of test_route_within_the_fp32_bound uses.  The two results are not compared with each
    other: these routes sum with float atomics, so two runs of ONE call differ as well, by up to twice that bound on these
    ill-conditioned inputs (test_gpu_device_lr.py compares the twins on the same routes, on inputs its tolerances fit)."""
    key, p, q, r, n, path, limit, want_fam, flag, rk = case
    R, Rk = [1] + r + [1], [1] + (rk or r) + [1]
    rng = np.random.default_rng(len(key) + n)
    cores = fb.scaled_cores(rng, p, q, R)
    ids = rng.integers(0, int(np.prod(p)), size=n).astype(np.int64)
    offs = np.arange(n + 1, dtype=np.int64)
    dy = fb.scaled_dy(rng, n, int(np.prod(q)))
    st0 = [(rng.random(c.shape) * 1e-6).astype(np.float32) for c in cores]
    shape, ws = nat.make_shape(p, q, R), nat.Workspace()
    try:
        nat.set_path(nat.PATH_FAST3 if path == "fast3" else nat.PATH_AUTO)
        nat.set_piece_limits(limit, limit)
        fam = nat.kernel_family(shape, n, n, True)
        assert fam & 7 == (want_fam if want_fam is not None else fam & 7) and fam & flag == flag, (key, fam)
        # ... and not the one route whose last kernel applies the step itself (grouped, no view, one piece)
        assert fam & 7 != nat.FAMILY_GROUPED or fam & (nat.FAMILY_MERGED | nat.FAMILY_PADDED) or limit, (key, fam)
        if limit:
            assert nat.plan_bytes(shape, n) == 0   # a call in pieces keeps no plan
        I, O, dY = _dev(ids), _dev(offs), _dev(dy)
        got = []
        for lr in (LR, torch.full((1,), LR, dtype=torch.float32, device="cuda")):
            ca, st = [_dev(x) for x in cores], [_dev(x) for x in st0]
            nat.backward_adagrad(shape, ca, st, I, None, n, None, n, dY, lr, EPS, ws, None, O)
            torch.cuda.synchronize()
            got.append(([x.cpu().numpy() for x in ca], [x.cpu().numpy() for x in st]))
        nat.status()
    finally:
        nat.set_path(nat.PATH_AUTO)
        nat.set_piece_limits(0, 0)
    route = _route(fam, nat)
    pieces = 2 * -(-n // limit) + 1 if limit else 0
    ref = orc.tt_dense_backward64(ids, offs, dy, cores, p, q, R)
    for t, (v, m, cnt) in enumerate(ref):
        delta = fb.gamma(fb.grad_depth(route, q, Rk, t, cnt, merged=len(p) != 3, pieces=pieces)) * m
        for (ada, ada_st), src in zip(got, ("by value", "device word")):
            what = f"{key} Adagrad, rate {src}, core {t}"
            _note("step_" + key, fb.assert_adagrad_grade(ada[t], ada_st[t], cores[t], st0[t], v, delta, LR, EPS, what))
            fb.assert_untouched(ada[t], cores[t], cnt, what)
            fb.assert_untouched(ada_st[t], st0[t], cnt, what + " state")


def test_three_table_windows_within_the_fp32_bound(nat):
    p, q, R = [20, 25, 300], [4, 5, 5], [1, 16, 16, 1]
    nat.set_path(nat.PATH_AUTO)
    rng = np.random.default_rng(33)
    T = 3
    tabs = [fb.scaled_cores(rng, p, q, R) for _ in range(T)]
    parts = [fb.skewed_bags(rng, p, 3000, long_bag=600 if k == 1 else 0) for k in range(T)]
    B = max(o.shape[0] - 1 for _, o in parts)
    ids, lens = [], []
    for i, o in parts:   # every table B bags (the shorter lists padded with empty bags)
        ids.append(i)
        lens.append(np.concatenate([np.diff(o), np.zeros(B - (o.shape[0] - 1), dtype=np.int64)]))
    ids = np.concatenate(ids)
    offs = np.concatenate([[0], np.cumsum(np.concatenate(lens))]).astype(np.int64)
    D = int(np.prod(q))
    dy = fb.scaled_dy(rng, T * B, D)
    shape, ws = nat.make_shape(p, q, R), nat.Workspace()
    assert nat.window_workspace_bytes(shape, nat.OP_BACKWARD, ids.shape[0], T * B, B) > 0
    I, O, dY = _dev(ids), _dev(offs), _dev(dy)
    out = torch.full((T * B, D), float("nan"), device="cuda")
    for k in range(T):
        c = [_dev(x) for x in tabs[k]]
        nat.forward_window(shape, c, I, O, k * B, B, out, ws)
        g = [torch.full_like(x, float("nan")) for x in c]
        nat.backward_window(shape, c, I, O, k * B, B, dY, ws, d_cores=g)
        cs = [x.clone() for x in c]
        nat.backward_window(shape, cs, I, O, k * B, B, dY, ws, lr=LR)
        st0 = [(rng.random(x.shape) * 1e-6).astype(np.float32) for x in tabs[k]]
        ca, st = [x.clone() for x in c], [_dev(s) for s in st0]
        nat.backward_window(shape, ca, I, O, k * B, B, dY, ws, opt_state=st, lr=LR, eps=EPS)
        torch.cuda.synchronize()
        ids_k = ids[offs[k * B]:offs[(k + 1) * B]]
        offs_k = offs[k * B:(k + 1) * B + 1] - offs[k * B]
        fam = nat.kernel_family(shape, ids_k.shape[0], B, True)
        h = lambda ts: [x.cpu().numpy() for x in ts]
        _check_all("windows", _route(fam, nat) if fam & 7 >= 3 else "grouped", p, q, R, R, tabs[k], ids_k, offs_k,
                   dy[k * B:(k + 1) * B], st0, out.cpu().numpy()[k * B:(k + 1) * B], h(g), h(cs), h(ca), h(st))


def test_exact_mode_within_the_fp32_bound(nat):
    p, q, R = [23, 290, 310], [4, 5, 5], [1, 16, 16, 1]
    shape, ws = nat.make_shape(p, q, R), nat.Workspace()
    assert nat.exact_unsupported_reason(shape) is None
    cores, ids, offs, dy, st0 = _inputs(p, q, R, 8000, seed=5)
    c = [_dev(x) for x in cores]
    I, O, dY = _dev(ids), _dev(offs), _dev(dy)
    B = offs.shape[0] - 1
    out = torch.full((B, int(np.prod(q))), float("nan"), device="cuda")
    nat.forward_exact(shape, c, I, O, B, out, ws)
    g = [torch.full_like(x, float("nan")) for x in c]
    nat.backward_exact(shape, c, I, O, B, dY, ws, d_cores=g)
    cs = [x.clone() for x in c]
    nat.backward_exact(shape, cs, I, O, B, dY, ws, lr=LR)
    ca, st = [x.clone() for x in c], [_dev(s) for s in st0]
    nat.backward_exact(shape, ca, I, O, B, dY, ws, opt_state=st, lr=LR, eps=EPS)
    torch.cuda.synchronize()
    h = lambda ts: [x.cpu().numpy() for x in ts]
    _check_all("exact", "exact", p, q, R, R, cores, ids, offs, dy, st0, out.cpu().numpy(), h(g), h(cs), h(ca), h(st))


# ---------------------------------------------------------------------------------------------------------------------
# through TTEmbeddingBag: weighted sum, mean, padding_idx (partition and zero-weight routes), 2-D bags, no_grad
# ---------------------------------------------------------------------------------------------------------------------
MODULE_CASES = [   # (key, p, q, inner ranks, ids, mode, weighted, init, padding route or None, 2-D bags)
    ("weighted_sum_scaled", [23, 290, 310], [4, 5, 5], [16, 16], 8000, "sum", True, "scaled", None, False),
    ("weighted_sum_uniform", [23, 290, 310], [4, 5, 5], [16, 16], 8000, "sum", True, "uniform", None, False),
    ("mean_approx_uniform", [23, 290, 310], [4, 5, 5], [16, 16], 8000, "mean", False, "approx-uniform", None, False),
    ("mean_pad_partition", [23, 290, 310], [4, 5, 5], [16, 16], 14000, "mean", False, "scaled", "partition", False),
    ("sum_pad_zero_weight", [23, 290, 310], [4, 5, 5], [16, 16], 8000, "sum", False, "scaled", "masked", False),
    ("weighted_pad", [23, 290, 310], [4, 5, 5], [16, 16], 3000, "sum", True, "scaled", "masked", False),
    ("two_d_mean", [23, 290, 310], [4, 5, 5], [16, 16], 6000, "mean", False, "scaled", None, True),
]


@pytest.mark.parametrize("case", MODULE_CASES, ids=[c[0] for c in MODULE_CASES])
def test_module_paths_within_the_fp32_bound(nat, case):
    from FBTT import tt_embeddings_ops as ops
    key, p, q, r, n_ids, mode, weighted, init, pad_route, two_d = case
    R = [1] + r + [1]
    nat.set_path(nat.PATH_AUTO)
    rng = np.random.default_rng(len(key))
    n_emb, D = int(np.prod(p)), int(np.prod(q))
    if two_d:
        ids = fb.skewed_bags(rng, p, n_ids, long_bag=0)[0]
        L = 3
        ids = ids[: (ids.shape[0] // L) * L]
        offs = np.arange(0, ids.shape[0] + 1, L, dtype=np.int64)
    else:
        ids, offs = fb.skewed_bags(rng, p, n_ids)
    pad = None
    if pad_route is not None:
        pad = int(ids[11])
        ids[::13] = pad
    torch.manual_seed(len(key))
    emb = ops.TTEmbeddingBag(n_emb, D, r, p, q, sparse=False, use_cache=False, mode=mode, padding_idx=pad,
                             weight_dist="uniform" if init == "scaled" else init)
    if pad_route is not None:
        emb._pad_partition = pad_route == "partition"
    if init == "scaled":
        with torch.no_grad():
            for c, x in zip(emb.tt_cores, fb.scaled_cores(rng, p, q, R)):
                c.copy_(_dev(x)[None])
    cores = [c.detach()[0].cpu().numpy().copy() for c in emb.tt_cores]
    w = fb.sample_weights(rng, ids.shape[0]) if weighted else None
    B, nnz = offs.shape[0] - 1, ids.shape[0]
    dy = fb.scaled_dy(rng, B, D)
    I, O = _dev(ids), _dev(offs)
    wt = _dev(w).requires_grad_(True) if weighted else None
    fam = nat.kernel_family(emb._shape, nnz, nnz if weighted else B, True)
    route = _route(fam, nat)
    if two_d:
        out = emb(I.view(-1, L), per_sample_weights=None)
    else:
        out = emb(I, O, per_sample_weights=wt)
    if pad_route is not None:
        assert emb._last_pad_route == pad_route, (key, emb._last_pad_route)
    out.backward(_dev(dy))
    torch.cuda.synchronize()
    with torch.no_grad():   # the inference forward (no plan, no autograd node)
        inf = (emb(I.view(-1, L)) if two_d else emb(I, O, per_sample_weights=wt.detach() if weighted else None)).cpu().numpy()
    lens = np.diff(offs)
    reduce = weighted or pad_route == "masked"
    # (the pad routes look up the kept ids only, which may take another family: the larger depth of the two)
    depth = np.maximum(fb.bag_depth(route, R, lens, reduce=reduce), fb.bag_depth("grouped", R, lens, reduce=reduce))
    depth = depth + (2 if mode == "mean" else 0)
    want, mag = orc.tt_forward64(ids, offs, cores, p, q, R, weights=w, mode=mode, pad=pad)
    for got, what in ((out.detach().cpu().numpy(), "forward"), (inf, "no_grad forward")):
        _note("module_" + key, fb.assert_fp32_grade(got, want, mag, depth, f"{key} {what}", "bag"))
    ref = orc.tt_dense_backward64(ids, offs, dy, cores, p, q, R, weights=w, mode=mode, pad=pad)
    if weighted:
        ref, (wv, wm) = ref
        _note("module_" + key, fb.assert_fp32_grade(wt.grad.cpu().numpy(), wv, wm, fb.wgrad_depth(route, q, R),
                                                    f"{key} w.grad", "id"))
    for t, ((v, m, n), c) in enumerate(zip(ref, emb.tt_cores)):
        g = c.grad[0].cpu().numpy()
        depth = np.maximum(fb.grad_depth(route, q, R, t, n, scaled=True), fb.grad_depth("grouped", q, R, t, n, scaled=True))
        _note("module_" + key, fb.assert_fp32_grade(g, v, m, depth, f"{key} dG{t}", "core row"))
        fb.assert_untouched(g, np.zeros_like(g), n, f"{key} dG{t}")
