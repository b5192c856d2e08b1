"""The dedup route on the GPU: the pass that finds the distinct ids, bit-exact against numpy; the pooling
kernels that read rows through the map, against float64 numpy; the module on every lookup route, per element against the
float64 oracle with the depths of tests/fp32_bound.py and tests/dedup_bound.py; modes, plumbing, refusals and the
``Eff_TTEmbedding`` drop-in."""
import numpy as np
import pytest
import torch

import adam_bound as ab
import dedup_bound as db
import fp32_bound as fb
from oracle import tt_oracle as orc
from test_gpu_weighted import CASES, SMALL

pytestmark = pytest.mark.gpu

LR, EPS = 0.05, 1e-3
BADARG, WORKSPACE = -1, -2


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


def _dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


def _route(fam, nat):
    return {nat.FAMILY_SCALAR: "scalar", nat.FAMILY_PER_BAG: "per_bag", nat.FAMILY_PER_BAG_RT: "per_bag",
            nat.FAMILY_GROUPED: "grouped", nat.FAMILY_GROUPED_WIDE: "wide"}[fam & 7]


# ---------------------------------------------------------------------------------------------------------------------
# 1. the pass
# ---------------------------------------------------------------------------------------------------------------------
def _unique_on_device(nat, ids, rows, ws=None):
    nnz = ids.shape[0]
    I = _dev(ids.astype(np.int64))
    uniq = torch.full((nnz,), -7, dtype=torch.int64, device="cuda")
    inv = torch.full((nnz,), -7, dtype=torch.int32, device="cuda")
    perm = torch.full((nnz,), -7, dtype=torch.int32, device="cuda")
    seg = torch.full((nnz + 1,), -7, dtype=torch.int64, device="cuda")
    count = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    nat.unique_ids(I, rows, uniq, inv, perm, seg, count, ws or nat.Workspace())
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in (uniq, inv, perm, seg, count)]


def _check_pass(got, ids):
    uniq, inv, perm, seg, count = got
    nnz = ids.shape[0]
    want_u, want_inv, want_cnt = np.unique(ids, return_inverse=True, return_counts=True)
    U = want_u.shape[0]
    assert int(count[0]) == U
    assert np.array_equal(uniq[:U], want_u)
    assert np.array_equal(inv, want_inv.reshape(-1).astype(np.int32))
    assert np.array_equal(perm, np.argsort(ids, kind="stable").astype(np.int32))
    assert np.array_equal(seg[:U + 1], np.concatenate([[0], np.cumsum(want_cnt)]).astype(np.int64))
    assert int(seg[U]) == nnz
    # nothing past U / U + 1 is written (the header says so)
    assert np.all(uniq[U:] == -7) and np.all(seg[U + 1:] == -7)


def _pass_cases():
    rng = np.random.default_rng(0)
    rows = 23 * 29 * 31
    cases = [(f"nnz{n}", rng.integers(0, rows, size=n), rows) for n in (0, 1, 2, 255, 256, 257, 5000)]
    cases.append(("all_equal", np.full(2000, 777), rows))
    cases.append(("all_distinct", rng.permutation(rows)[:5000], rows))
    cases.append(("from_300", rng.choice(rows, 300, replace=False)[rng.integers(0, 300, size=5000)], rows))
    big = 2 ** 31 + 5
    cases.append(("rows_past_2_31", np.array([big - 1, 0, 2 ** 31, big - 2, 5])[rng.integers(0, 5, size=3000)], big))
    return cases


PASS_CASES = _pass_cases()


@pytest.mark.parametrize("case", PASS_CASES, ids=[c[0] for c in PASS_CASES])
def test_the_pass_is_bit_exact_against_numpy_under_both_grids(nat, case):
    _, ids, rows = case
    ids = np.asarray(ids, dtype=np.int64)
    outs = []
    try:
        for grid in (0, 1):
            nat.set_exact_grid(grid)
            got = _unique_on_device(nat, ids, rows)
            _check_pass(got, ids)
            outs.append(got)
    finally:
        nat.set_exact_grid(0)
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


def test_the_pass_refuses_bad_arguments_and_leaves_the_status_clean(nat):
    L = nat.LIB
    nnz, rows = 1000, 20677
    I = torch.randint(0, rows, (nnz,), device="cuda")
    uniq, seg = torch.empty(nnz, dtype=torch.int64, device="cuda"), torch.empty(nnz + 1, dtype=torch.int64, device="cuda")
    inv, perm = torch.empty(nnz, dtype=torch.int32, device="cuda"), torch.empty(nnz, dtype=torch.int32, device="cuda")
    cnt = torch.empty(1, dtype=torch.int32, device="cuda")
    need = nat.unique_ids_workspace_bytes(nnz, rows)
    assert need > 40960 + nnz * 8
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    p = lambda t: t.data_ptr()
    good = [p(I), nnz, rows, p(uniq), p(inv), p(perm), p(seg), p(cnt), p(ws), need, None]
    for k, v in ((1, -1), (1, 2 ** 31), (2, 0), (0, None), (3, None), (4, None), (5, None), (6, None), (7, None), (8, None)):
        args = list(good)
        args[k] = v
        assert L.ttemb_unique_ids(*args) == BADARG, (k, v)
    for nbytes in (16, 40960, need - 1):
        args = list(good)
        args[9] = nbytes
        assert L.ttemb_unique_ids(*args) == WORKSPACE, nbytes
    assert L.ttemb_unique_ids(*good) == 0
    torch.cuda.synchronize()
    nat.status()   # no fault word was raised by any of it
    assert int(cnt) == np.unique(I.cpu().numpy()).shape[0]


# ---------------------------------------------------------------------------------------------------------------------
# 2. the mapped pool alone
# ---------------------------------------------------------------------------------------------------------------------
def _ragged(rng, nnz, long_bag, first=0, last=None, mean=4):
    """Bags of 0 .. 2 mean ids with empty ones, one bag of ``long_bag`` ids between short ones, a trailing empty bag; the
    positions before ``first`` and from ``last`` on lie outside every bag."""
    last = nnz if last is None else last
    lens = list(rng.integers(0, 2 * mean + 1, size=2 * (nnz // mean) + 8))
    lens[::7] = [0] * len(lens[::7])
    if long_bag:
        lens = lens[:3] + [long_bag] + lens[3:]
    offs = first + np.concatenate([[0], np.cumsum(lens)])
    offs = offs[offs < last]
    return np.concatenate([offs, [last, last]]).astype(np.int64)


def _hub_ids(rng, rows, nnz):
    """One id (``ids[0]``) at every 5th position and nowhere else, the rest drawn from 300 other values."""
    pool = rng.choice(rows, 301, replace=False)
    ids = pool[rng.integers(0, 300, size=nnz)]
    ids[::5] = pool[300]
    return ids.astype(np.int64)


def _bag_of(offs, nnz):
    bag = np.searchsorted(offs, np.arange(nnz), side="right") - 1
    inside = (np.arange(nnz) >= offs[0]) & (np.arange(nnz) < offs[-1])
    return np.where(inside, bag, -1)


@pytest.fixture(scope="module")
def pool_case():
    """The inputs and the float64 reference of the mapped pool, computed once: 8 192 positions, one id at every 5th of them
    (1 639 repeats: four chunks of its segment), ragged bags with one of 1 300 positions, three positions outside every bag
    at either end."""
    rng = np.random.default_rng(11)
    nnz, D = 8192, 100
    ids = _hub_ids(rng, 20677, nnz)
    offs = _ragged(rng, nnz, 1300, first=3, last=nnz - 3)
    B = offs.shape[0] - 1
    uniq, inv, cnt = np.unique(ids, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    U = uniq.shape[0]
    assert cnt.max() == 1639 and np.diff(offs).max() == 1300 and np.diff(offs).min() == 0
    rows = (fb.signed_magnitudes(rng, (nnz, D)) * 10.0 ** rng.uniform(-3, 0, size=(nnz, 1))).astype(np.float32)
    rows[U:] = np.nan
    w = fb.sample_weights(rng, nnz)
    dy = fb.scaled_dy(rng, B, D)
    bag = _bag_of(offs, nnz)
    perm = np.argsort(ids, kind="stable")
    seg = np.full(nnz + 1, -1, dtype=np.int64)
    seg[:U + 1] = np.concatenate([[0], np.cumsum(cnt)])
    ref = {}
    for weighted in (False, True):
        f = w.astype(np.float64) if weighted else np.ones(nnz)
        f = np.where(bag >= 0, f, 0.0)
        r64 = rows[inv].astype(np.float64)
        out, omag = np.zeros((B, D)), np.zeros((B, D))
        np.add.at(out, bag[bag >= 0], (f[:, None] * r64)[bag >= 0])
        np.add.at(omag, bag[bag >= 0], np.abs(f[:, None] * r64)[bag >= 0])
        g = np.where(bag[:, None] >= 0, dy[np.maximum(bag, 0)].astype(np.float64), 0.0)
        dr, drmag = np.zeros((U, D)), np.zeros((U, D))
        np.add.at(dr, inv, f[:, None] * g)
        np.add.at(drmag, inv, np.abs(f[:, None] * g))
        ref[weighted] = (out, omag, dr, drmag)
    dw = np.sum(g * r64, axis=1)
    dwmag = np.sum(np.abs(g * r64), axis=1)
    return dict(nnz=nnz, D=D, B=B, U=U, ids=ids, offs=offs, inv=inv, perm=perm, seg=seg, cnt=cnt, rows=rows, w=w, dy=dy,
                ref=ref, dw=dw, dwmag=dwmag)


def _run_pool(nat, c, weighted):
    nnz, D, B, U = c["nnz"], c["D"], c["B"], c["U"]
    ws = nat.Workspace()
    rows, offs, dy = _dev(c["rows"]), _dev(c["offs"]), _dev(c["dy"])
    w = _dev(c["w"]) if weighted else None
    inv, perm, seg = _dev(c["inv"].astype(np.int32)), _dev(c["perm"].astype(np.int32)), _dev(c["seg"])
    count = torch.tensor([U], dtype=torch.int32, device="cuda")
    out = torch.full((B, D), float("nan"), device="cuda")
    nat.bag_reduce_mapped(rows, inv, w, offs, out, ws)
    d_rows = torch.full((nnz, D), float("nan"), device="cuda")
    d_w = torch.full((nnz,), float("nan"), device="cuda")
    nat.bag_reduce_mapped_backward(dy, w, inv, perm, seg, count, offs, d_rows, ws, rows=rows, d_weights=d_w)
    # the unmapped pool on the expanded rows (rows[map]): the bits the mapped forward has to give
    expanded = rows[inv.long()].contiguous()
    plain = torch.full((B, D), float("nan"), device="cuda")
    nat.bag_reduce(expanded, w if weighted else torch.ones(nnz, device="cuda"), offs, plain, ws)
    torch.cuda.synchronize()
    return out, d_rows, d_w, plain


@pytest.mark.parametrize("weighted", [False, True], ids=["no_weights", "weights"])
def test_mapped_pool_against_float64_and_bit_identical_under_one_workgroup(nat, pool_case, weighted):
    c = pool_case
    U, D = c["U"], c["D"]
    try:
        nat.set_exact_grid(0)
        out, d_rows, d_w, plain = _run_pool(nat, c, weighted)
        nat.set_exact_grid(1)
        again = _run_pool(nat, c, weighted)
    finally:
        nat.set_exact_grid(0)
    for a, b in zip((out, d_rows[:U], d_w), (again[0], again[1][:U], again[2])):
        assert torch.equal(a, b)
    assert torch.equal(out, plain)
    want, mag, dr, drmag = c["ref"][weighted]
    lens = np.diff(c["offs"])[:, None]
    r = fb.assert_fp32_grade(out.cpu().numpy(), want, mag, lens + lens // 512 + 2, "mapped forward", "bag")
    m = c["cnt"][:, None]
    got = d_rows.cpu().numpy()
    r2 = fb.assert_fp32_grade(got[:U], dr, drmag, db.segment_depth(m), "mapped backward", "distinct id")
    r3 = fb.assert_fp32_grade(d_w.cpu().numpy(), c["dw"], c["dwmag"], D + 8, "mapped w.grad", "position")
    print(f"\n  mapped pool weighted={weighted}: largest err/(u mag) forward {r:.2f}, d_rows {r2:.2f}, w.grad {r3:.2f}", end="")
    # the NaN planted in rows[U:] reached nothing, and no row >= U of d_rows was written
    assert np.isfinite(out.cpu().numpy()).all() and np.isfinite(got[:U]).all() and np.isfinite(d_w.cpu().numpy()).all()
    assert np.isnan(got[U:]).all()
    # positions outside every bag: no weight gradient
    outside = _bag_of(c["offs"], c["nnz"]) < 0
    assert outside.sum() == 6 and not d_w.cpu().numpy()[outside].any()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the module on every route
# ---------------------------------------------------------------------------------------------------------------------
def _module(ops, p, q, r, cores, table_batched=0, **kw):
    kw.setdefault("use_cache", False)
    n, D = int(np.prod(p)), int(np.prod(q))
    if table_batched:
        emb = ops.TableBatchedTTEmbeddingBag(table_batched, n, D, r, p, q, weight_dist="uniform", **kw)
    else:
        emb = ops.TTEmbeddingBag(n, D, r, p, q, weight_dist="uniform", **kw)
    with torch.no_grad():
        for c, x in zip(emb.tt_cores, cores):
            c.copy_(_dev(x) if x.ndim == 3 else _dev(x)[None])
    return emb


def _grad_depths(route, p, q, R, ids):
    """Per core: (depth [p_t, 1], distinct ids per row) on the dedup route (tests/dedup_bound.py)."""
    return [(db.dedup_grad_depth(route, q, R, t, n, m), n) for t, (n, m) in enumerate(db.touch_counts(ids, p))]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_module_on_every_route_within_the_fp32_bound(nat, ops, case):
    name, p, q, r, nnz, want_fam, prefix = case
    R = [1] + r + [1]
    rng = np.random.default_rng(len(name) + nnz)
    n_emb, D = int(np.prod(p)), int(np.prod(q))
    ids = _hub_ids(rng, n_emb, nnz)
    offs = _ragged(rng, nnz, 0)
    B = offs.shape[0] - 1
    w = fb.sample_weights(rng, nnz)
    dy = fb.scaled_dy(rng, B, D)
    cores = fb.scaled_cores(rng, p, q, R)
    I, O, dY = _dev(ids), _dev(offs), _dev(dy)
    # the rows lookup: nnz bags of one without a row index, behind the count
    shape = nat.make_shape(p, q, R)
    fam = nat.kernel_family(shape, nnz, nnz, True)
    assert fam & ~nat.FAMILY_ROUTE_FLAGS == want_fam, (name, fam)
    if prefix is not None:
        assert bool(fam & nat.FAMILY_PREFIX_IN_CHAIN) == prefix, (name, fam)
    route = _route(fam, nat)
    U = np.unique(ids).shape[0]

    emb = _module(ops, p, q, r, cores, sparse=False, dedup=True)
    wt = _dev(w).requires_grad_(True)
    out = emb(I, O, per_sample_weights=wt)
    out.backward(dY)
    torch.cuda.synchronize()
    assert int(emb._last_unique) == U
    lens = np.diff(offs)
    want, mag = orc.tt_forward64(ids, offs, cores, p, q, R, weights=w)
    worst = fb.assert_fp32_grade(out.detach().cpu().numpy(), want, mag, fb.bag_depth(route, R, lens, reduce=True),
                                 f"{name} forward", "bag")
    ref, (wv, wm) = orc.tt_dense_backward64(ids, offs, dy, cores, p, q, R, weights=w)
    worst = max(worst, fb.assert_fp32_grade(wt.grad.cpu().numpy(), wv, wm, fb.wgrad_depth(route, q, R), f"{name} w.grad", "id"))
    depths = _grad_depths(route, p, q, R, ids)
    deltas = []
    for t, ((v, m, _), (depth, n), c) in enumerate(zip(ref, depths, emb.tt_cores)):
        g = c.grad[0].cpu().numpy()
        worst = max(worst, fb.assert_fp32_grade(g, v, m, depth, f"{name} dG{t}", "core row"))
        fb.assert_untouched(g, np.zeros_like(g), n, f"{name} dG{t}")
        deltas.append(fb.gamma(depth) * m)

    sgd = _module(ops, p, q, r, cores, sparse=True, dedup=True, learning_rate=LR)
    sgd(I, O, per_sample_weights=_dev(w)).backward(dY)
    ada = _module(ops, p, q, r, cores, sparse=True, dedup=True, learning_rate=LR, eps=EPS, optimizer=ops.OptimType.EXACT_ADAGRAD)
    ada(I, O, per_sample_weights=_dev(w)).backward(dY)
    adam = _module(ops, p, q, r, cores, sparse=True, dedup=True, learning_rate=LR, eps=EPS, optimizer=ops.OptimType.ADAM)
    adam(I, O, per_sample_weights=_dev(w)).backward(dY)
    torch.cuda.synchronize()
    assert adam.adam_steps() == [1]
    hp = ab.Hyper(LR, EPS)
    for t, ((v, _, _), (_, n), delta) in enumerate(zip(ref, depths, deltas)):
        host = lambda x: x.detach()[0].cpu().numpy()
        z = np.zeros_like(cores[t])
        worst = max(worst, fb.assert_sgd_grade(host(sgd.tt_cores[t]), cores[t], v, delta, LR, f"{name} SGD core {t}"))
        fb.assert_untouched(host(sgd.tt_cores[t]), cores[t], n, f"{name} SGD core {t}")
        worst = max(worst, fb.assert_adagrad_grade(host(ada.tt_cores[t]), host(ada.optimizer_state[t]), cores[t], z, v, delta,
                                                   LR, EPS, f"{name} Adagrad core {t}"))
        ab.assert_adam_grade(host(adam.tt_cores[t]), host(adam.optimizer_state[t]), host(adam.optimizer_state_v[t]), cores[t],
                             z, z, v, delta, 1, hp, f"{name} Adam core {t}")
    print(f"\n  dedup {name}: {U} distinct of {nnz}, largest err/(u mag) {worst:.2f}", end="")


# ---------------------------------------------------------------------------------------------------------------------
# 4. modes and plumbing, on the small grouped shape
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    p, q, r = SMALL
    R = [1] + r + [1]
    rng = np.random.default_rng(21)
    nnz = 8192
    ids = _hub_ids(rng, int(np.prod(p)), nnz)
    offs = _ragged(rng, nnz, 600)
    return dict(p=p, q=q, r=r, R=R, nnz=nnz, ids=ids, offs=offs, w=fb.sample_weights(rng, nnz),
                dy=fb.scaled_dy(rng, offs.shape[0] - 1, int(np.prod(q))), cores=fb.scaled_cores(rng, p, q, R), rng=rng)


def _check_call(nat, s, cores, ids, offs, out, grads, w=None, wgrad=None, mode="sum", pad=None, dy=None, what=""):
    """One table's forward and (``grads``: per-core numpy or None) dense gradients of a dedup call against the oracle."""
    p, q, R = s["p"], s["q"], s["R"]
    nnz = ids.shape[0]
    route = _route(nat.kernel_family(nat.make_shape(p, q, R), nnz, nnz, True), nat)
    lens = np.diff(offs)
    depth = fb.bag_depth(route, R, lens, reduce=True) + (2 if mode == "mean" else 0)
    want, mag = orc.tt_forward64(ids, offs, cores, p, q, R, weights=w, mode=mode, pad=pad)
    fb.assert_fp32_grade(out, want, mag, depth, f"{what} forward", "bag")
    if grads is None:
        return
    ref = orc.tt_dense_backward64(ids, offs, dy, cores, p, q, R, weights=w, mode=mode, pad=pad)
    if w is not None:
        ref, (wv, wm) = ref
        if wgrad is not None:
            fb.assert_fp32_grade(wgrad, wv, wm, fb.wgrad_depth(route, q, R), f"{what} w.grad", "id")
    for t, ((v, m, _), (d, _)) in enumerate(zip(ref, _grad_depths(route, p, q, R, ids))):
        fb.assert_fp32_grade(grads[t], v, m, d + (2 if mode == "mean" else 0), f"{what} dG{t}", "core row")


@pytest.mark.parametrize("kind", ["sum", "mean", "weighted", "pad_sum", "pad_mean", "pad_weighted"])
def test_modes_through_the_module(nat, ops, small, kind):
    s = small
    ids, offs = s["ids"], s["offs"]
    pad = int(ids[0]) if kind.startswith("pad") else None   # the hub id is the pad
    mode = "mean" if kind.endswith("mean") else "sum"
    w = s["w"] if kind.endswith("weighted") else None
    emb = _module(ops, s["p"], s["q"], s["r"], s["cores"], sparse=False, dedup=True, mode=mode, padding_idx=pad)
    wt = None if w is None else _dev(w).requires_grad_(True)
    out = emb(_dev(ids), _dev(offs), per_sample_weights=wt)
    out.backward(_dev(s["dy"]))
    with torch.no_grad():
        inf = emb(_dev(ids), _dev(offs), per_sample_weights=None if w is None else _dev(w))
    assert inf.grad_fn is None and int(emb._last_unique) == np.unique(ids).shape[0]
    torch.cuda.synchronize()
    grads = [c.grad[0].cpu().numpy() for c in emb.tt_cores]
    _check_call(nat, s, s["cores"], ids, offs, out.detach().cpu().numpy(), grads, w, None if wt is None else wt.grad.cpu().numpy(),
                mode, pad, s["dy"], kind)
    _check_call(nat, s, s["cores"], ids, offs, inf.cpu().numpy(), None, w, None, mode, pad, what=kind + " no_grad")


def test_two_dimensional_indices(nat, ops, small):
    s = small
    N = 8
    ids = s["ids"][: (s["nnz"] // N) * N]
    offs = np.arange(0, ids.shape[0] + 1, N, dtype=np.int64)
    dy = fb.scaled_dy(s["rng"], offs.shape[0] - 1, 100)
    emb = _module(ops, s["p"], s["q"], s["r"], s["cores"], sparse=False, mode="mean")
    out = emb(_dev(ids).view(-1, N), dedup=True)
    out.backward(_dev(dy))
    torch.cuda.synchronize()
    _check_call(nat, s, s["cores"], ids, offs, out.detach().cpu().numpy(), [c.grad[0].cpu().numpy() for c in emb.tt_cores],
                mode="mean", dy=dy, what="2-D mean")


def test_two_tables(nat, ops, small):
    s = small
    rng = np.random.default_rng(8)
    p, q, R = s["p"], s["q"], s["R"]
    B = 300
    parts = []
    for k in range(2):
        ids = _hub_ids(rng, int(np.prod(p)), 1500)
        offs = _ragged(rng, 1500, 0)[: B + 1]
        parts.append((ids[: offs[-1]], offs))
    ids = np.concatenate([a for a, _ in parts])
    offs = np.concatenate([parts[0][1], parts[0][1][-1] + parts[1][1][1:]])
    cores2 = [np.stack([a, b]) for a, b in zip(fb.scaled_cores(rng, p, q, R), fb.scaled_cores(rng, p, q, R))]
    w = fb.sample_weights(rng, ids.shape[0])
    dy = fb.scaled_dy(rng, 2 * B, 100).reshape(2, B, 100)
    emb = _module(ops, p, q, s["r"], cores2, table_batched=2, sparse=False, dedup=True)
    out = emb(_dev(ids), _dev(offs), per_sample_weights=_dev(w))
    assert tuple(out.shape) == (2, B, 100)
    out.backward(_dev(dy))
    torch.cuda.synchronize()
    lo = 0
    for k, (ids_k, offs_k) in enumerate(parts):
        hi = lo + ids_k.shape[0]
        _check_call(nat, s, [c[k] for c in cores2], ids_k, offs_k, out[k].detach().cpu().numpy(),
                    [c.grad[k].cpu().numpy() for c in emb.tt_cores], w[lo:hi], None, "sum", None, dy[k], f"table {k}")
        lo = hi
    assert int(emb._last_unique) == np.unique(parts[1][0]).shape[0]   # the last dedup call: the second table's


def test_constructor_default_and_per_call_override(nat, ops, small, monkeypatch):
    """Which route a call takes is read off the calls of the pass (the plain bag sums of the grouped kernels are not
    bit-reproducible from call to call, so the outputs cannot tell)."""
    s = small
    p, q, R = s["p"], s["q"], s["R"]
    I, O = _dev(s["ids"]), _dev(s["offs"])
    on = _module(ops, p, q, s["r"], s["cores"], sparse=False, dedup=True)
    off = _module(ops, p, q, s["r"], s["cores"], sparse=False)
    passes = []
    real = nat.unique_ids
    monkeypatch.setattr(nat, "unique_ids", lambda *a, **k: (passes.append(1), real(*a, **k))[1])
    lens = np.diff(s["offs"])
    want, mag = orc.tt_forward64(s["ids"], s["offs"], s["cores"], p, q, R)
    plain_depth = fb.bag_depth(_route(nat.kernel_family(off._shape, s["nnz"], lens.shape[0], True), nat), R, lens)
    with torch.no_grad():
        for emb, kw in ((off, {}), (off, {"dedup": None}), (off, {"dedup": False}), (on, {"dedup": False})):
            out = emb(I, O, **kw)
            assert not passes and emb._last_unique is None, kw   # the route of before
            fb.assert_fp32_grade(out.cpu().numpy(), want, mag, plain_depth, f"plain call {kw}", "bag")
        a = on(I, O)
        assert len(passes) == 1 and on._last_unique is not None
        b = on(I, O, dedup=None)
        c = off(I, O, dedup=True)
        assert len(passes) == 3 and off._last_unique is not None
    assert torch.equal(a, b) and torch.equal(a, c)   # (the dedup route IS reproducible: every sum has its order)
    _check_call(nat, s, s["cores"], s["ids"], s["offs"], a.cpu().numpy(), None, what="per-call dedup")


def test_two_lookups_before_one_backward_add_their_gradients(nat, ops, small):
    s = small
    p, q, R = s["p"], s["q"], s["R"]
    rng = np.random.default_rng(4)
    emb = _module(ops, p, q, s["r"], s["cores"], sparse=False, dedup=True)
    calls = []
    loss = 0
    for k in range(2):
        ids = _hub_ids(rng, int(np.prod(p)), 3000 + 500 * k)
        offs = _ragged(rng, ids.shape[0], 0)
        dy = fb.scaled_dy(rng, offs.shape[0] - 1, 100)
        loss = loss + (emb(_dev(ids), _dev(offs)) * _dev(dy)).sum()
        calls.append((ids, offs, dy))
    loss.backward()
    torch.cuda.synchronize()
    route = _route(nat.kernel_family(emb._shape, 3000, 3000, True), nat)
    refs = [orc.tt_dense_backward64(ids, offs, dy, s["cores"], p, q, R) for ids, offs, dy in calls]
    depths = [_grad_depths(route, p, q, R, ids) for ids, _, _ in calls]
    for t, c in enumerate(emb.tt_cores):
        v = refs[0][t][0] + refs[1][t][0]
        m = refs[0][t][1] + refs[1][t][1]
        d = np.maximum(depths[0][t][0], depths[1][t][0]) + 1   # one accumulation into .grad (fp32_bound.py)
        fb.assert_fp32_grade(c.grad[0].cpu().numpy(), v, m, d, f"two lookups dG{t}", "core row")


@pytest.mark.parametrize("kind", ["weighted", "mean", "pad_mean"])
def test_no_host_synchronisation(nat, ops, small, kind):
    s = small
    pad = int(s["ids"][0]) if kind.startswith("pad") else None
    mode = "mean" if kind.endswith("mean") else "sum"
    emb = _module(ops, s["p"], s["q"], s["r"], s["cores"], sparse=True, dedup=True, mode=mode, padding_idx=pad)
    I, O, dY = _dev(s["ids"]), _dev(s["offs"]), _dev(s["dy"])
    wt = _dev(s["w"]).requires_grad_(True) if kind == "weighted" else None
    emb(I, O, per_sample_weights=wt).backward(dY)   # (first call: workspace and scratch exist)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        emb(I, O, per_sample_weights=wt).backward(dY)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    nat.status()


def test_a_call_without_ids(nat, ops, small):
    s = small
    emb = _module(ops, s["p"], s["q"], s["r"], s["cores"], sparse=False, dedup=True)
    idx = torch.empty(0, dtype=torch.int64, device="cuda")
    offs = torch.zeros(6, dtype=torch.int64, device="cuda")
    out = emb(idx, offs)
    assert tuple(out.shape) == (5, 100) and not bool(out.any()) and int(emb._last_unique) == 0
    out.backward(torch.ones_like(out))
    for c in emb.tt_cores:
        assert c.grad is None or not bool(c.grad.any())


# ---------------------------------------------------------------------------------------------------------------------
# 5. refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_module_serving_plain_calls(nat, ops, small):
    s = small
    p, q, r = s["p"], s["q"], s["r"]
    I, O = _dev(s["ids"][:2000]), _dev(np.arange(2001, dtype=np.int64))
    with torch.no_grad():
        want = _module(ops, p, q, r, s["cores"], sparse=False)(I, O)

    def still_serves(emb, **kw):
        with torch.no_grad():
            assert torch.equal(emb(I, O, dedup=False, **kw), want)

    exact = _module(ops, p, q, r, s["cores"], sparse=False, deterministic=True)
    with pytest.raises(ValueError, match="exact mode"):
        exact(I, O, dedup=True)
    exact.deterministic = False
    still_serves(exact)

    plain = _module(ops, p, q, r, s["cores"], sparse=False)
    with pytest.raises(ValueError, match="mode='max'"):
        plain(I, O, mode="max", dedup=True)
    big = torch.zeros(1, dtype=torch.int64, device="cuda").expand((1 << 24) + 1)
    with pytest.raises(ValueError, match="row window"):
        plain(big, None, dedup=True)
    still_serves(plain)

    with pytest.raises(ValueError, match="dedup=True with use_cache=True"):
        _module(ops, p, q, r, s["cores"], use_cache=True, dedup=True)
    cached = _module(ops, p, q, r, s["cores"], sparse=False, use_cache=True, cache_size=300, hashtbl_size=int(np.prod(p)))
    with torch.no_grad():
        cached(I, O, dedup=True)   # a warming cache is no obstacle
    cached.cache_populate()
    assert not cached.warmup
    with pytest.raises(ValueError, match="live row cache"):
        cached(I, O, dedup=True)
    with torch.no_grad():   # (the cached rows come from other kernels: the oracle's bound, not the plain call's bits)
        _check_call(nat, s, s["cores"], s["ids"][:2000], np.arange(2001, dtype=np.int64), cached(I, O, dedup=False).cpu().numpy(),
                    None, what="live cache, dedup=False")

    on = _module(ops, p, q, r, s["cores"], sparse=True, dedup=True)
    with pytest.raises(ValueError, match=r"capture\(\) on a dedup=True module"):
        on.capture(2000, 2000)
    with pytest.raises(ValueError, match=r"capture_bags\(\) on a dedup=True module"):
        on.capture_bags(2000, 500, mode="mean")
    with pytest.raises(ValueError, match="mode='max'"):
        on(I, O, mode="max")
    still_serves(on)
    torch.cuda.synchronize()
    nat.status()


# ---------------------------------------------------------------------------------------------------------------------
# 6. Eff_TTEmbedding
# ---------------------------------------------------------------------------------------------------------------------
def test_eff_tt_embedding_looks_up_each_distinct_id_once(nat, small):
    from Efficient_TT.efficient_tt import Eff_TTEmbedding
    s = small
    p, q, r, R = s["p"], s["q"], s["r"], s["R"]
    n = 4000
    ids = s["ids"][:n]
    offs = np.arange(n + 1, dtype=np.int64)
    dy = fb.scaled_dy(np.random.default_rng(6), n, 100)
    I, dY = _dev(ids), _dev(dy)
    uniq, inverse = torch.unique(I, sorted=True, return_inverse=True)
    route = _route(nat.kernel_family(nat.make_shape(p, q, R), n, n, True), nat)
    want, mag = orc.tt_forward64(ids, offs, s["cores"], p, q, R)
    ref = orc.tt_dense_backward64(ids, offs, dy, s["cores"], p, q, R)
    depths = _grad_depths(route, p, q, R, ids)

    def run(dedup, unique, inverse):
        emb = Eff_TTEmbedding(int(np.prod(p)), 100, r, p, q, learning_rate=LR, dedup=dedup)
        with torch.no_grad():
            for c, x in zip(emb.tt_cores, s["cores"]):
                c.copy_(_dev(x))
        out = emb(I, None, unique, inverse)
        out.backward(dY)
        torch.cuda.synchronize()
        fb.assert_fp32_grade(out.detach().cpu().numpy(), want, mag, fb.bag_depth(route, R, np.ones(n, dtype=np.int64), reduce=True),
                             "Eff forward", "id")
        for t, ((v, m, _), (d, cnt)) in enumerate(zip(ref, depths)):
            got = emb.tt_cores[t].detach().cpu().numpy()
            fb.assert_sgd_grade(got, s["cores"][t], v, fb.gamma(d) * m, LR, f"Eff SGD core {t}")
            fb.assert_untouched(got, s["cores"][t], cnt, f"Eff SGD core {t}")
        return out.detach()

    a = run(False, uniq, inverse)
    b = run(True, None, None)
    # deliberately wrong content (reversed ids, a map of zeros): nothing changes, because neither tensor is read
    c = run(False, uniq.flip(0), torch.zeros_like(inverse))
    assert torch.equal(a, b) and torch.equal(a, c)
    # one of the two alone is the call of before: every position is looked up (same rows, the plain route's bits)
    emb = Eff_TTEmbedding(int(np.prod(p)), 100, r, p, q, learning_rate=LR)
    with torch.no_grad():
        for cc, x in zip(emb.tt_cores, s["cores"]):
            cc.copy_(_dev(x))
        d = emb(I, None, uniq, None)
    fb.assert_fp32_grade(d.cpu().numpy(), want, mag, fb.bag_depth(route, R, np.ones(n, dtype=np.int64)), "Eff plain forward", "id")
