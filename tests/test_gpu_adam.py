"""The fused Adam / AdamW step on the GPU: every route of the C ABI against the float64 restatement with the bound of
tests/adam_bound.py, the properties that separate dense Adam from a shortcut (rows without ids move, the step count lives on
the device and advances once per applied step, a skipped step changes nothing), and the module against torch.optim."""
import numpy as np
import pytest
import torch

import adam_bound as ab
import fp32_bound as fb
from oracle import tt_oracle as orc

pytestmark = pytest.mark.gpu

LR, EPS = 0.05, 1e-3
U_ONE = 2.0 ** -24


@pytest.fixture(scope="module")
def nat():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import ttemb_native
    yield ttemb_native
    ttemb_native.set_path(ttemb_native.PATH_AUTO)
    ttemb_native.set_piece_limits(0, 0)


def _dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


def _host(ts):
    return [x.detach().cpu().numpy().copy() for x in ts]


def _route(fam, nat):
    return {nat.FAMILY_SCALAR: "scalar", nat.FAMILY_PER_BAG: "per_bag", nat.FAMILY_PER_BAG_RT: "per_bag",
            nat.FAMILY_GROUPED: "grouped", nat.FAMILY_GROUPED_WIDE: "wide"}[fam & 7]


# the routes of tests/test_gpu_accuracy.py's ABI_CASES, restated:
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


def _adam_steps(nat, key, p, q, R, Rk, n_ids, hp_args, steps=3, seed=0, pieces=0, want_fam=None, flag=None, route=None):
    """``steps`` consecutive fused Adam steps through ttemb_backward_adam with fresh ids per step; after every step cores, m
    and v are inside the bound of one step from the fp32 state before it, and t read back equals the steps applied.  From
    step 2 on, rows no id of the call touches have moved (dense Adam: their first moment is not zero)."""
    lr, eps, wd, decoupled = hp_args
    hp = ab.Hyper(lr, eps, (0.9, 0.999), wd, decoupled)
    nhp = nat.make_adam(lr, eps, (0.9, 0.999), wd, decoupled)
    rng = np.random.default_rng(seed)
    shape, ws = nat.make_shape(p, q, R), nat.Workspace()
    c = [_dev(x) for x in fb.scaled_cores(rng, p, q, R)]
    m, v = [torch.zeros_like(x) for x in c], [torch.zeros_like(x) for x in c]
    step = nat.new_adam_step("cuda")
    worst = 0.0
    cold_moved = False
    for t in range(1, steps + 1):
        ids, offs = fb.skewed_bags(rng, p, n_ids)
        B, nnz = offs.shape[0] - 1, ids.shape[0]
        dy = fb.scaled_dy(rng, B, int(np.prod(q)))
        fam = nat.kernel_family(shape, nnz, B, True)
        if want_fam is not None:
            assert fam & ~nat.FAMILY_ROUTE_FLAGS == want_fam, (key, fam)
        if flag == "prefix":
            assert fam & nat.FAMILY_PREFIX_IN_CHAIN, (key, fam)
        if flag == "group_products":
            assert fam & nat.FAMILY_GROUP_PRODUCTS_IN_CHAIN, (key, fam)
        w0, m0, v0 = _host(c), _host(m), _host(v)
        I, O, dY = _dev(ids), _dev(offs), _dev(dy)
        pl = nat.new_plan(shape, nnz, I.device) if (fam & 7) >= 3 else None
        out = torch.empty((B, int(np.prod(q))), device="cuda")
        nat.forward(shape, c, I, None, O, nnz, None, B, out, ws, pl)
        nat.backward_adam(shape, c, m, v, step, I, None, nnz, None, B, dY, nhp, ws, pl, O)
        torch.cuda.synchronize()
        assert int(step[0].item()) == t, f"{key}: t = {int(step[0].item())} after {t} steps"
        w1, m1, v1 = _host(c), _host(m), _host(v)
        ref = orc.tt_dense_backward64(ids, offs, dy, w0, p, q, R)
        rt = route or _route(fam, nat)
        for k, (val, mag, cnt) in enumerate(ref):
            delta = fb.gamma(fb.grad_depth(rt, q, Rk, k, cnt, merged=len(p) != 3, pieces=pieces)) * mag
            worst = max(worst, ab.assert_adam_grade(w1[k], m1[k], v1[k], w0[k], m0[k], v0[k], val, delta, t, hp,
                                                    f"{key} step {t} core {k}"))
            cold = cnt == 0
            if t >= 2 and cold.any() and np.abs(m0[k][cold]).max() > 0:
                # (by the float64 value: the bound above holds for these rows too)
                assert (np.abs(w1[k][cold] - w0[k][cold]) > 0).any(), f"{key} step {t} core {k}: rows without ids did not move"
                cold_moved = True
    assert cold_moved or steps < 2, f"{key}: no step had rows without ids that carried a first moment"
    print(f"\n  {key:28s} largest err / bound {worst:.3f}", end="")
    return c, m, v, step


@pytest.mark.parametrize("case", ABI_CASES, ids=[c[0] for c in ABI_CASES])
def test_adam_route_within_the_bound(nat, case):
    key, p, q, r, n_ids, path, want_fam, flag, rk = case
    R, Rk = [1] + r + [1], [1] + (rk or r) + [1]
    nat.set_path({"auto": nat.PATH_AUTO, "generic": nat.PATH_GENERIC, "fast3": nat.PATH_FAST3}[path])
    _adam_steps(nat, key, p, q, R, Rk, n_ids, (LR, EPS, 0.0, False), seed=len(key) + n_ids, want_fam=want_fam, flag=flag)


@pytest.mark.parametrize("hp_args", [(LR, EPS, 0.01, False), (LR, EPS, 0.01, True), (LR, 1e-8, 0.0, False)],
                         ids=["coupled_decay", "adamw", "default_eps"])
def test_adam_grouped_route_with_decay_and_default_eps(nat, hp_args):
    nat.set_path(nat.PATH_FAST3)
    _adam_steps(nat, "fast3", [8, 20, 3000], [4, 5, 5], [1, 16, 16, 1], [1, 16, 16, 1], 20000, hp_args, seed=77, want_fam=3)


def test_adam_wide_rank_and_pieces(nat):
    nat.set_path(nat.PATH_FAST3)
    q, R = [5, 5, 4], [1, 64, 64, 1]
    _adam_steps(nat, "wide_r64", [13, 50, 40], q, R, R, 3000, (LR, EPS, 0.0, False), seed=9, route="wide")
    p, q, R = [30, 35, 400], [4, 5, 5], [1, 16, 16, 1]
    nat.set_piece_limits(900, 700)
    n_ids = 12000
    pieces = -(-n_ids // 700) + -(-(n_ids // 2) // 900) + 2   # (an upper bound: at most n_ids / 2 bags)
    _adam_steps(nat, "pieces", p, q, R, R, n_ids, (LR, EPS, 0.0, False), seed=17, pieces=pieces, route="grouped")


def test_adam_window_steps_one_table(nat):
    """A table's window of a longer id list (ttemb_backward_adam_window) against the float64 step."""
    p, q, R = [20, 25, 300], [4, 5, 5], [1, 16, 16, 1]
    rng = np.random.default_rng(33)
    hp, nhp = ab.Hyper(LR, EPS), nat.make_adam(LR, EPS)
    shape, ws = nat.make_shape(p, q, R), nat.Workspace()
    parts = [fb.skewed_bags(rng, p, 3000, long_bag=0) for _ in range(2)]
    B = max(o.shape[0] - 1 for _, o in parts)
    lens = [np.concatenate([np.diff(o), np.zeros(B - (o.shape[0] - 1), dtype=np.int64)]) for _, o in parts]
    ids = np.concatenate([i for i, _ in parts])
    offs = np.concatenate([[0], np.cumsum(np.concatenate(lens))]).astype(np.int64)
    dy = fb.scaled_dy(rng, 2 * B, int(np.prod(q)))
    assert nat.window_workspace_bytes(shape, nat.OP_BACKWARD, ids.shape[0], 2 * B, B) > 0
    I, O, dY = _dev(ids), _dev(offs), _dev(dy)
    k = 1
    w0 = fb.scaled_cores(rng, p, q, R)
    c = [_dev(x) for x in w0]
    m, v, step = [torch.zeros_like(x) for x in c], [torch.zeros_like(x) for x in c], nat.new_adam_step("cuda")
    nat.backward_window(shape, c, I, O, k * B, B, dY, ws, opt_state=m, adam=(v, step, nhp))
    torch.cuda.synchronize()
    assert step.tolist()[0] == 1
    ids_k, offs_k = ids[offs[k * B]:offs[(k + 1) * B]], offs[k * B:(k + 1) * B + 1] - offs[k * B]
    for t, (val, mag, cnt) in enumerate(orc.tt_dense_backward64(ids_k, offs_k, dy[k * B:(k + 1) * B], w0, p, q, R)):
        delta = fb.gamma(fb.grad_depth("grouped", q, R, t, cnt)) * mag
        z = np.zeros_like(w0[t])
        ab.assert_adam_grade(_host(c)[t], _host(m)[t], _host(v)[t], w0[t], z, z, val, delta, 1, hp, f"window core {t}")


def test_an_empty_call_changes_nothing_and_leaves_t(nat):
    p, q, R = [8, 20, 3000], [4, 5, 5], [1, 16, 16, 1]
    nat.set_path(nat.PATH_FAST3)
    c, m, v, step = _adam_steps(nat, "fast3", p, q, R, R, 20000, (LR, EPS, 0.01, False), steps=2, seed=3)
    before = [x.clone() for x in (*c, *m, *v, step)]
    shape, ws = nat.make_shape(p, q, R), nat.Workspace()
    I, O = torch.zeros(0, dtype=torch.int64, device="cuda"), torch.zeros(5, dtype=torch.int64, device="cuda")
    nat.backward_adam(shape, c, m, v, step, I, None, 0, None, 4, torch.zeros((4, 100), device="cuda"),
                      nat.make_adam(LR, EPS, weight_decay=0.01), ws, None, O)
    torch.cuda.synchronize()
    for a, b in zip((*c, *m, *v, step), before):
        assert torch.equal(a, b)
    assert step.tolist()[0] == 2


def test_zero_state_zero_gradient_zero_eps_is_not_nan(nat):
    """eps = 0 on elements that have never seen a gradient: the update is skipped, not 0 / 0."""
    n = 4099
    w = torch.randn(n, device="cuda")
    w0 = w.clone()
    m, v, g = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    step = nat.new_adam_step("cuda")
    nat.adam_step(w, m, v, step, g, nat.make_adam(LR, 0.0))
    torch.cuda.synchronize()
    assert torch.equal(w, w0) and not torch.isnan(m).any() and not torch.isnan(v).any() and step.tolist()[0] == 1


@pytest.mark.parametrize("decoupled", [False, True], ids=["adam", "adamw"])
def test_flat_step_and_its_skip_word(nat, decoupled):
    """ttemb_adam_step: with skip = 0.0 it is the float64 step (g scaled by grad_scale first); with a non-zero skip word --
    a float 1.0 in a tensor, nothing is provoked -- weights, moments and t stay bit-identical."""
    rng = np.random.default_rng(4)
    n = 10007   # (a scalar tail behind the float4 body)
    hp, nhp = ab.Hyper(LR, EPS, (0.9, 0.999), 0.01, decoupled), nat.make_adam(LR, EPS, (0.9, 0.999), 0.01, decoupled)
    w0 = (fb.signed_magnitudes(rng, n) * 10.0 ** rng.uniform(-3, 0, size=n)).astype(np.float32)
    w, m, v, step = _dev(w0), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda"), nat.new_adam_step("cuda")
    scale = 0.5
    wh, mh, vh = w0, np.zeros(n, np.float32), np.zeros(n, np.float32)
    for t in range(1, 4):
        g = (fb.signed_magnitudes(rng, n) * 10.0 ** rng.uniform(-3, 0, size=n)).astype(np.float32)
        nat.adam_step(w, m, v, step, _dev(g), nhp, grad_scale=scale, skip=_dev(np.array([1.0], dtype=np.float32)))
        torch.cuda.synchronize()
        for got, want in ((w, wh), (m, mh), (v, vh)):
            assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)), "a skipped step wrote"
        assert step.tolist()[0] == t - 1, "a skipped step advanced t"
        nat.adam_step(w, m, v, step, _dev(g), nhp, grad_scale=scale, skip=_dev(np.array([0.0], dtype=np.float32)))
        torch.cuda.synchronize()
        assert step.tolist()[0] == t
        g64 = g.astype(np.float64) * scale
        w1, m1, v1 = w.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy()
        ab.assert_adam_grade(w1, m1, v1, wh, mh, vh, g64, U_ONE * np.abs(g64), t, hp, f"flat step {t}")
        wh, mh, vh = w1, m1, v1


# ---------------------------------------------------------------------------------------------------------------------
# module level
# ---------------------------------------------------------------------------------------------------------------------
P3, Q3, R3 = [8, 20, 3000], [4, 5, 5], [16, 16]
N3 = 8 * 20 * 3000
MLR, WD = 0.01, 0.01
VARIANTS = ("sum", "mean", "weighted", "padding", "2d", "tables3")


def _bag(opt, sparse, seed=0, tables=1, **kw):
    from FBTT.tt_embeddings_ops import TableBatchedTTEmbeddingBag, TTEmbeddingBag
    torch.manual_seed(seed)
    args = (N3, 100, R3, P3, Q3)
    kw = dict(optimizer=opt, sparse=sparse, use_cache=False, weight_dist="normal", learning_rate=MLR, eps=EPS, **kw)
    emb = TTEmbeddingBag(*args, **kw) if tables == 1 else TableBatchedTTEmbeddingBag(tables, *args, **kw)
    with torch.no_grad():
        for c in emb.tt_cores:
            c.mul_(30.0)
    return emb


def _batch(rng, n=6000):
    ids, offs = fb.skewed_bags(rng, P3, n)
    B = offs.shape[0] - 1
    return _dev(ids), _dev(offs), _dev(fb.scaled_dy(rng, B, 100))


PAD = 12345


def _variant_batches(variant, steps, seed, permute=False):
    """``steps`` calls of a variant as (args, kwargs, dY); ``permute``: the ids of every bag in another order."""
    rng, prm = np.random.default_rng(seed), np.random.default_rng(seed + 1000)
    out = []
    for _ in range(steps):
        tables = 3 if variant == "tables3" else 1
        if variant == "2d":
            ids = rng.integers(0, N3, size=(600, 8))
            w = None
            if permute:
                ids = np.take_along_axis(ids, np.argsort(prm.random(ids.shape), axis=1), axis=1)
            dy = fb.scaled_dy(rng, 600, 100)
            out.append(((_dev(ids),), {}, _dev(dy)))
            continue
        parts = [fb.skewed_bags(rng, P3, 4000, long_bag=0) for _ in range(tables)]
        B = max(o.shape[0] - 1 for _, o in parts)
        lens = np.concatenate([np.concatenate([np.diff(o), np.zeros(B - (o.shape[0] - 1), dtype=np.int64)]) for _, o in parts])
        ids = np.concatenate([i for i, _ in parts])
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        if variant == "padding":
            ids[::7] = PAD
        w = fb.sample_weights(rng, ids.shape[0]) if variant == "weighted" else None
        if permute:
            order = np.concatenate([offs[b] + prm.permutation(offs[b + 1] - offs[b]) for b in range(offs.shape[0] - 1)]).astype(np.int64)
            ids = ids[order]
            w = None if w is None else w[order]
        dy = fb.scaled_dy(rng, tables * B, 100)
        dy = dy.reshape(tables, B, 100) if tables > 1 else dy
        kw = {} if w is None else {"per_sample_weights": _dev(w)}
        out.append(((_dev(ids), _dev(offs)), kw, _dev(dy)))
    return out


def _module_kw(variant):
    return {"mean": {"mode": "mean"}, "padding": {"padding_idx": PAD}}.get(variant, {})


def _train_dense(variant, decoupled, batches):
    """sparse=False module stepped by torch.optim.Adam / AdamW on the GPU."""
    from FBTT.tt_embeddings_ops import OptimType
    emb = _bag(OptimType.SGD, False, tables=3 if variant == "tables3" else 1, **_module_kw(variant))
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls(emb.parameters(), lr=MLR, betas=(0.9, 0.999), eps=EPS, weight_decay=WD)
    for args, kw, dy in batches:
        opt.zero_grad(set_to_none=True)
        emb(*args, **kw).backward(dy)
        opt.step()
    torch.cuda.synchronize()
    return _host(emb.tt_cores)


def _train_fused(variant, decoupled, batches):
    from FBTT.tt_embeddings_ops import OptimType
    emb = _bag(OptimType.ADAM, True, tables=3 if variant == "tables3" else 1, weight_decay=WD, decoupled_weight_decay=decoupled,
               **_module_kw(variant))
    for args, kw, dy in batches:
        emb(*args, **kw).backward(dy)
    torch.cuda.synchronize()
    assert emb.adam_steps() == [len(batches)] * emb.num_tables
    return _host(emb.tt_cores)


def _diff(a, b):
    """Largest |a - b| over every core element, in units of the learning rate (an Adam step moves an element by about lr)."""
    return max(float(np.abs(x - y).max()) for x, y in zip(a, b)) / MLR


def twin_figures(variant, decoupled, steps=10, seed=21):
    """(dense against dense with the ids of each bag permuted, fused against dense) after ``steps`` steps."""
    dense = _train_dense(variant, decoupled, _variant_batches(variant, steps, seed))
    dense_perm = _train_dense(variant, decoupled, _variant_batches(variant, steps, seed, permute=True))
    fused = _train_fused(variant, decoupled, _variant_batches(variant, steps, seed))
    return _diff(dense, dense_perm), _diff(fused, dense)


# Measured before the tolerance was set (profiles/r10_adam_twins.json): what two DENSE runs with the ids of each bag permuted
# differ by after 10 steps, per (variant, decoupled), in units of lr (the fused step was 1.6e-5 ... 1.42e-3 lr from the dense
# twin in that run, at most 2.1 times the figure of its own variant)
TWIN_DENSE = {
    ("sum", False): 1.714e-04,
    ("sum", True): 1.196e-03,
    ("mean", False): 1.179e-04,
    ("mean", True): 1.022e-04,
    ("weighted", False): 7.227e-05,
    ("weighted", True): 1.093e-04,
    ("padding", False): 2.048e-04,
    ("padding", True): 1.542e-04,
    ("2d", False): 1.537e-05,
    ("2d", True): 1.565e-05,
    ("tables3", False): 1.632e-04,
    ("tables3", True): 3.582e-04,
}
TWIN_MARGIN = 4.0
# the capture and data-parallel tests run the unweighted sum with coupled decay
PLAIN_DENSE_FIGURE = TWIN_DENSE[("sum", False)]


@pytest.mark.parametrize("decoupled", [False, True], ids=["adam", "adamw"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_fused_adam_trains_like_torch_optim_on_the_dense_twin(nat, variant, decoupled):
    """The same TTEmbeddingBag twice from one seed: sparse=True with OptimType.ADAM against sparse=False stepped by
    torch.optim.Adam / AdamW on the GPU, 10 steps.  The dense twin is itself fp32 with another summation order, so the
    tolerance is TWIN_MARGIN = 4 times what two DENSE runs of THIS variant differ by when the ids of each bag are permuted:
    the figure measured first and kept in profiles/r10_adam_twins.json (1.5e-5 lr for 2-D bags up to 1.196e-3 lr for the sum
    under AdamW), or the one this very run measures when that is larger (one sample of a noise figure can come out low).
    Units of lr: an Adam step moves an element by about lr."""
    dd, fd = twin_figures(variant, decoupled)
    print(f"\n  {variant:10s} {'adamw' if decoupled else 'adam':6s} dense/dense {dd:.3e} lr, fused/dense {fd:.3e} lr", end="")
    assert fd <= TWIN_MARGIN * max(TWIN_DENSE[(variant, decoupled)], dd), (variant, fd, dd)


def test_deterministic_adam_is_bit_reproducible(nat):
    from FBTT.tt_embeddings_ops import OptimType
    runs = []
    for _ in range(2):
        emb = _bag(OptimType.ADAM, True, deterministic=True, weight_decay=WD)
        rng = np.random.default_rng(8)
        for _ in range(3):
            I, O, dY = _batch(rng)
            emb(I, O).backward(dY)
        torch.cuda.synchronize()
        assert emb.adam_steps() == [3]
        runs.append(_host([*emb.tt_cores, *emb.optimizer_state, *emb.optimizer_state_v]))
    for a, b in zip(*runs):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.abs(runs[0][3]).max() > 0 and np.abs(runs[0][6]).max() > 0


@pytest.mark.parametrize("n", [2048, 20000], ids=["per_bag", "grouped"])
def test_captured_adam_steps_like_the_eager_module(nat, n):
    """capture() leaves cores, m, v and t bit-identical (weight decay on: a step on the zero gradient would move them), and
    5 replayed steps equal 5 eager steps of a twin; t = 5 afterwards -- a step count kept on the host would stay frozen in the
    captured backward."""
    from FBTT.tt_embeddings_ops import OptimType
    a, b = (_bag(OptimType.ADAM, True, weight_decay=WD) for _ in range(2))
    state = lambda e: [*e.tt_cores, *e.optimizer_state, *e.optimizer_state_v, e.adam_step]
    before = [x.detach().clone() for x in state(b)]
    cap = b.capture(n, n)
    torch.cuda.synchronize()
    for x, y in zip(state(b), before):
        assert torch.equal(x.detach(), y), "capture() changed the module"
    rng = np.random.default_rng(12)
    offs = torch.arange(n + 1, device="cuda")
    for _ in range(5):
        ids = _dev(rng.integers(0, N3, size=n))
        dy = _dev(fb.scaled_dy(rng, n, 100))
        a(ids, offs).backward(dy)
        cap(ids).backward(dy)
    torch.cuda.synchronize()
    assert a.adam_steps() == [5] and b.adam_steps() == [5]
    d = _diff(_host(a.tt_cores), _host(b.tt_cores))
    print(f"\n  captured/eager {d:.3e} lr", end="")
    assert d <= TWIN_MARGIN * PLAIN_DENSE_FIGURE
    b.weight_decay = 0.0
    with pytest.raises(RuntimeError, match="capture\\(\\) again"):
        cap(ids)


@pytest.mark.parametrize("overlap", [False, True])
def test_data_parallel_adam_at_world_size_one(nat, overlap):
    """TTDataParallel.step() on an ADAM module (world size 1: no process group) against the fused module, 4 steps."""
    from FBTT.tt_embeddings_ops import OptimType
    from ttemb_dist import TTDataParallel
    fused = _bag(OptimType.ADAM, True, weight_decay=WD)
    dense = _bag(OptimType.ADAM, False, weight_decay=WD)
    dp = TTDataParallel(dense)
    rng = np.random.default_rng(6)
    for _ in range(4):
        I, O, dY = _batch(rng, 20000)
        fused(I, O).backward(dY)
        dense(I, O).backward(dY)
        dp.step(overlap=overlap)
    dp.flush()
    torch.cuda.synchronize()
    assert dense.adam_steps() == [4]
    d = _diff(_host(fused.tt_cores), _host(dense.tt_cores))
    print(f"\n  data-parallel/fused {d:.3e} lr", end="")
    assert d <= TWIN_MARGIN * PLAIN_DENSE_FIGURE
    assert float(dense.optimizer_state[1].abs().max()) > 0 and float(dense.optimizer_state_v[1].abs().max()) > 0


def test_tt_adam_backward_shim_steps_like_the_float64_adam(nat):
    """tt_embeddings.tt_adam_backward (the addition beside the reference's functions): two steps of a one-table call against
    the float64 step with the bound of adam_bound; t counts them."""
    import tt_embeddings as ext
    p, q, R = [23, 290, 310], [4, 5, 5], [1, 16, 16, 1]
    rng = np.random.default_rng(55)
    hp = ab.Hyper(LR, EPS, (0.9, 0.999), 0.01, True)
    cores = [_dev(x).unsqueeze(0).contiguous() for x in fb.scaled_cores(rng, p, q, R)]
    m, v = [torch.zeros_like(c) for c in cores], [torch.zeros_like(c) for c in cores]
    step = torch.zeros((1, 4), dtype=torch.int32, device="cuda")
    L = _dev(np.array([290 * 310, 310, 1], dtype=np.int64))
    empty64, empty32 = torch.empty(0, dtype=torch.int64, device="cuda"), torch.empty(0, dtype=torch.int32, device="cuda")
    for t in (1, 2):
        ids, offs = fb.skewed_bags(rng, p, 4000)
        B = offs.shape[0] - 1
        dy = fb.scaled_dy(rng, B, 100)
        w0, m0, v0 = (_host([x[0] for x in ts]) for ts in (cores, m, v))
        i2, rowidx, tableidx, ntt, loc = ext.preprocess_indices_sync(_dev(ids), _dev(offs), 1, True, empty64, empty32)
        ext.tt_adam_backward(1000, 100, LR, EPS, 0.9, 0.999, 0.01, True, p, q, R, L, ntt, i2, rowidx, tableidx,
                             _dev(dy).unsqueeze(0), m, v, step, cores)
        torch.cuda.synchronize()
        assert step.tolist()[0][0] == t
        fam = nat.kernel_family(nat.make_shape(p, q, R), ids.shape[0], B, False)
        for k, (val, mag, cnt) in enumerate(orc.tt_dense_backward64(ids, offs, dy, w0, p, q, R)):
            delta = fb.gamma(fb.grad_depth(_route(fam, nat), q, R, k, cnt)) * mag
            ab.assert_adam_grade(_host([cores[k][0]])[0], _host([m[k][0]])[0], _host([v[k][0]])[0], w0[k], m0[k], v0[k], val,
                                 delta, t, hp, f"tt_adam_backward step {t} core {k}")
    # a call without ids leaves everything, t included
    before = [x.clone() for x in (*cores, *m, *v, step)]
    ext.tt_adam_backward(1000, 100, LR, EPS, 0.9, 0.999, 0.01, True, p, q, R, L, 0, empty64, empty64, empty64,
                         torch.zeros((1, 3, 100), device="cuda"), m, v, step, cores)
    torch.cuda.synchronize()
    for a, b in zip((*cores, *m, *v, step), before):
        assert torch.equal(a, b)
