"""Host checks of the fused Adam / AdamW step: the float64 restatement against torch.optim, the acceptance bound
(tests/adam_bound.py) on a correct fp32 Adam and on planted defects, and the module's constructor / state layout."""
import numpy as np
import pytest
import torch

import adam_bound as ab
import fp32_bound as fb
from oracle import tt_oracle as orc

P, Q, R = [23, 290, 310], [4, 5, 5], [1, 16, 16, 1]
D = int(np.prod(Q))
LR, EPS = 0.05, 1e-3
STEPS = (1, 2, 5)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the float64 restatement is torch.optim.Adam / AdamW
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decoupled", [False, True], ids=["adam", "adamw"])
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_float64_adam_is_torch_optim(decoupled, wd):
    rng = np.random.default_rng(5)
    cores = [rng.standard_normal(s) for s in ((7, 24), (11, 80), (5, 20))]
    hp = ab.Hyper(LR, EPS, (0.9, 0.999), wd, decoupled)
    params = [torch.tensor(c, dtype=torch.float64, requires_grad=True) for c in cores]
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls(params, lr=hp.lr, betas=(hp.b1, hp.b2), eps=hp.eps, weight_decay=hp.wd)
    w = [c.copy() for c in cores]
    m = [np.zeros_like(c) for c in cores]
    v = [np.zeros_like(c) for c in cores]
    for t in range(1, 6):
        grads = [rng.standard_normal(c.shape) * 10.0 ** rng.uniform(-3, 0) for c in cores]
        for p, g in zip(params, grads):
            p.grad = torch.tensor(g)
        opt.step()
        for k in range(3):
            w[k], m[k], v[k] = ab.adam64(w[k], m[k], v[k], grads[k], t, hp)
            got = params[k].detach().numpy()
            assert np.abs(w[k] - got).max() <= 1e-12 * np.abs(got).max(), (t, k)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the acceptance bound: a correct fp32 Adam passes, planted defects do not
# ---------------------------------------------------------------------------------------------------------------------
def _grads(seed, cores32):
    """Fresh ids and dY, the float64 gradient with its bound, and the fp32 gradient summed in three orders."""
    rng = np.random.default_rng(seed)
    ids, offs = fb.skewed_bags(rng, P, 2000)
    dy = fb.scaled_dy(rng, offs.shape[0] - 1, D)
    ref = orc.tt_dense_backward64(ids, offs, dy, cores32, P, Q, R)
    n = ids.shape[0]
    roffs = (n - offs[::-1]).astype(np.int64)
    g32 = [orc.tt_dense_backward(ids, offs, dy, cores32, P, Q, R, acc_dtype=np.float32),
           orc.tt_dense_backward(ids[::-1].copy(), roffs, dy[::-1].copy(), cores32, P, Q, R, acc_dtype=np.float32),
           orc.tt_dense_backward(ids, offs, dy, cores32, P, Q, R)]
    out = []
    for t, (val, mag, cnt) in enumerate(ref):
        delta = fb.gamma(fb.grad_depth("scalar", Q, R, t, cnt)) * mag
        out.append((val, delta, cnt, [np.asarray(g[t], dtype=np.float32) for g in g32]))
    return out


def _trajectory(hp, steps=5, seed=40):
    """fp32 Adam over ``steps`` steps with fresh ids per step: per step and core (w0, m0, v0, g64, delta, cnt, g32s)."""
    rng = np.random.default_rng(seed)
    w = fb.scaled_cores(rng, P, Q, R)
    m = [np.zeros_like(c) for c in w]
    v = [np.zeros_like(c) for c in w]
    hist = []
    for t in range(1, steps + 1):
        gr = _grads(seed + t, w)
        hist.append([(w[k], m[k], v[k]) + gr[k] for k in range(3)])
        nxt = [ab.adam32(w[k], m[k], v[k], gr[k][3][0], t, hp) for k in range(3)]
        w, m, v = [x[0] for x in nxt], [x[1] for x in nxt], [x[2] for x in nxt]
    return hist


HYPERS = {"adam": ab.Hyper(LR, EPS), "adam_wd": ab.Hyper(LR, EPS, wd=0.01), "adamw": ab.Hyper(LR, EPS, wd=0.01, decoupled=True)}
_TRAJ = {}


def _traj(name):
    if name not in _TRAJ:
        _TRAJ[name] = _trajectory(HYPERS[name])
    return _TRAJ[name]


@pytest.mark.parametrize("name", sorted(HYPERS))
def test_correct_fp32_adam_passes_at_steps_1_2_5_in_three_orders(name):
    hp, worst, wide = HYPERS[name], 0.0, 0.0
    for t in STEPS:
        for k, (w0, m0, v0, g, delta, cnt, g32s) in enumerate(_traj(name)[t - 1]):
            for g32 in g32s:
                w1, m1, v1 = ab.adam32(w0, m0, v0, g32, t, hp)
                worst = max(worst, ab.assert_adam_grade(w1, m1, v1, w0, m0, v0, g, delta, t, hp, f"{name} step {t} core {k}"))
            # the condition under which the GPU check says something: few elements with a bound near the size of a step
            frac = ab.wide_fraction(w0, m0, v0, g, delta, t, hp)
            wide = max(wide, frac)
            assert frac <= 0.01, f"{name} step {t} core {k}: {frac:.2%} of the elements have a bound wider than 10 % of lr"
    print(f"{name}: largest err / bound {worst:.3f}; at most {wide:.3%} of a core's elements with a bound > 0.1 lr")


def _rejects(fn):
    with pytest.raises(AssertionError, match="over the fp32 bound"):
        fn()


def _defect_step(defect, w0, m0, v0, g32, cnt, t, hp):
    f = np.float32
    if defect == "no_bias_correction":
        w1, m1, v1 = ab.adam32(w0, m0, v0, g32, t, hp)
        return (w0 - f(hp.lr) * m1 / (np.sqrt(v1) + f(hp.eps))).astype(f), m1, v1   # (wd = 0 in this case)
    if defect == "v_from_g":
        w1, m1, _ = ab.adam32(w0, m0, v0, g32, t, hp)
        return w1, m1, (f(hp.b2) * v0 + f(1 - hp.b2) * g32).astype(f)
    if defect == "coupled_as_decoupled":
        other = ab.Hyper(hp.lr, hp.eps, (hp.b1, hp.b2), hp.wd, not hp.decoupled)
        return ab.adam32(w0, m0, v0, g32, t, other)
    if defect == "touched_rows_only":
        w1, m1, v1 = ab.adam32(w0, m0, v0, g32, t, hp)
        cold = cnt == 0
        w1, m1, v1 = w1.copy(), m1.copy(), v1.copy()
        w1[cold], m1[cold], v1[cold] = w0[cold], m0[cold], v0[cold]
        return w1, m1, v1
    if defect == "t_twice":
        w1, m1, v1 = ab.adam32(w0, m0, v0, g32, 2 * t, hp)
        return w1, m1, v1
    raise AssertionError(defect)


@pytest.mark.parametrize("defect", ["no_bias_correction", "v_from_g", "coupled_as_decoupled", "touched_rows_only", "t_twice"])
def test_a_planted_defect_is_rejected(defect):
    name = "adam_wd" if defect == "coupled_as_decoupled" else "adam"
    hp = HYPERS[name]
    t = 2   # (step 2: the first step whose untouched rows carry a first moment)
    k = 1
    w0, m0, v0, g, delta, cnt, g32s = _traj(name)[t - 1][k]
    assert (cnt == 0).any() and np.abs(m0[cnt == 0]).max() > 0, "step 2 needs rows without ids that moved in step 1"
    w1, m1, v1 = _defect_step(defect, w0, m0, v0, g32s[0], cnt, t, hp)
    _rejects(lambda: ab.assert_adam_grade(w1, m1, v1, w0, m0, v0, g, delta, t, hp, defect))


def test_zero_gradient_zero_state_zero_eps_is_not_nan():
    hp = ab.Hyper(LR, 0.0)
    z = np.zeros((3, 4), dtype=np.float32)
    w = np.ones((3, 4), dtype=np.float32)
    w1, m1, v1 = ab.adam32(w, z, z, z, 1, hp)
    assert np.array_equal(w1, w) and not np.isnan(m1).any() and not np.isnan(v1).any()


# ---------------------------------------------------------------------------------------------------------------------
# 3. constructor, state layout, exported symbols
# ---------------------------------------------------------------------------------------------------------------------
def _module(opt, **kw):
    from FBTT.tt_embeddings_ops import TTEmbeddingBag
    return TTEmbeddingBag(1000, 16, [4, 4], [10, 10, 10], [2, 2, 4], optimizer=opt, use_cache=False, **kw)


def test_adam_state_layout():
    from FBTT.tt_embeddings_ops import OptimType, TableBatchedTTEmbeddingBag
    m = _module(OptimType.ADAM, betas=(0.8, 0.99), weight_decay=0.01, decoupled_weight_decay=True)
    sd = m.state_dict()
    for t, c in enumerate(m.tt_cores):
        assert sd[f"optimizer_state.optimizer_state{t}"].shape == c.shape
        assert sd[f"optimizer_state_v.optimizer_state_v{t}"].shape == c.shape
    assert sd["adam_step"].shape == (1, 4) and sd["adam_step"].dtype == torch.int32
    assert m.betas == (0.8, 0.99) and m.weight_decay == 0.01 and m.decoupled_weight_decay is True
    tb = TableBatchedTTEmbeddingBag(3, 1000, 16, [4, 4], [10, 10, 10], [2, 2, 4], optimizer=OptimType.ADAM)
    assert tb.state_dict()["adam_step"].shape == (3, 4)
    # round trip restores m, v and t
    for k, v in sd.items():
        if k.startswith("optimizer_state") or k == "adam_step":
            v.copy_(torch.arange(v.numel(), dtype=torch.float32).reshape(v.shape).to(v.dtype))
    m2 = _module(OptimType.ADAM)
    m2.load_state_dict(m.state_dict())
    for k, v in m2.state_dict().items():
        assert torch.equal(v, m.state_dict()[k]), k


def test_other_optimizers_keep_their_state_dict_keys():
    from FBTT.tt_embeddings_ops import OptimType
    base = ["L", "cache_state", "hashtbl", "optimizer_state.optimizer_state0", "optimizer_state.optimizer_state1",
            "optimizer_state.optimizer_state2", "tt_cores.0", "tt_cores.1", "tt_cores.2"]   # the keys before ADAM had a meaning
    for opt in OptimType:
        if opt != OptimType.ADAM:
            assert sorted(_module(opt).state_dict().keys()) == base, opt
    extra = sorted(set(_module(OptimType.ADAM).state_dict().keys()) - set(base))
    assert extra == ["adam_step", "optimizer_state_v.optimizer_state_v0", "optimizer_state_v.optimizer_state_v1",
                     "optimizer_state_v.optimizer_state_v2"]


def test_adam_with_a_trained_row_cache_is_refused():
    from FBTT.tt_embeddings_ops import OptimType, TTEmbeddingBag
    with pytest.raises(ValueError, match="per-row optimiser"):
        TTEmbeddingBag(1000, 16, [4, 4], [10, 10, 10], [2, 2, 4], optimizer=OptimType.ADAM, sparse=True, use_cache=True)
    with pytest.raises(ValueError, match="betas"):
        _module(OptimType.ADAM, betas=(0.9, 1.0))


def test_exported_symbols_and_binding():
    import ttemb_native as nat
    for name in ("ttemb_backward_adam", "ttemb_backward_adam_window", "ttemb_backward_adam_exact", "ttemb_adam_step"):
        assert name in nat.EXPORTED_SYMBOLS and hasattr(nat.LIB, name)
    assert nat.LIB.ttemb_abi_version() == 4
    hp = nat.make_adam(0.05, 1e-3, (0.9, 0.999), 0.01, True)
    assert hp.decoupled == 1 and hp.beta2 == 0.999 and abs(hp.lr - 0.05) < 1e-8


def test_tt_adam_backward_is_added_beside_the_reference_functions():
    import inspect

    import tt_embeddings
    sig = inspect.signature(tt_embeddings.tt_adam_backward)
    assert list(sig.parameters)[-4:] == ["exp_avg", "exp_avg_sq", "step", "tt_cores"]
