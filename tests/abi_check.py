"""What test_gpu_accuracy.py and test_gpu_shape_matrix.py share: the inputs where a per-element check matters, a run of the
forward, the dense backward and the fused SGD / Adagrad steps through the C ABI (whole, or with the forward in its two
phases), and the check of everything such a run returns against the float64 oracle with the bound of tests/fp32_bound.py."""
import numpy as np
import torch

import fp32_bound as fb
from oracle import tt_oracle as orc

LR, EPS = 0.05, 1e-3
WORST = {}   # route -> largest err / (u mag) seen (test_gpu_accuracy.py prints it at the end of the module)


def _dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


def _note(key, r):
    WORST[key] = max(WORST.get(key, 0.0), r)


def _route(fam, nat):
    return {nat.FAMILY_SCALAR: "scalar", nat.FAMILY_PER_BAG: "per_bag", nat.FAMILY_PER_BAG_RT: "per_bag",
            nat.FAMILY_GROUPED: "grouped", nat.FAMILY_GROUPED_WIDE: "wide"}[fam & 7]


def _inputs(p, q, R, n_ids, seed, long_bag=600):
    rng = np.random.default_rng(seed)
    cores = fb.scaled_cores(rng, p, q, R)
    ids, offs = fb.skewed_bags(rng, p, n_ids, long_bag)
    dy = fb.scaled_dy(rng, offs.shape[0] - 1, int(np.prod(q)))
    st0 = [(rng.random(c.shape) * 1e-6).astype(np.float32) for c in cores]
    return cores, ids, offs, dy, st0


def _check_all(key, route, p, q, R, Rk, cores, ids, offs, dy, st0, out, grads, sgd, ada, ada_st, merged=False, pieces=0,
               note=None, oracle=None):
    """forward, dense gradients, fused SGD cores, fused Adagrad cores and state against the float64 oracle.  ``R`` is the
    table's ranks (oracle), ``Rk`` the ranks the kernels ran (padded).  ``note(key, ratio)``: where the largest
    err / (u mag) of every check goes (this module's WORST when not given); ``oracle``: ``(tt_forward64(...),
    tt_dense_backward64(...))`` of these very inputs where the caller has them already (computed here when not given)."""
    _note = note or globals()["_note"]
    lens = np.diff(offs)
    (want, mag), ref = oracle or (orc.tt_forward64(ids, offs, cores, p, q, R),
                                  orc.tt_dense_backward64(ids, offs, dy, cores, p, q, R))
    _note(key, fb.assert_fp32_grade(out, want, mag, fb.bag_depth(route, Rk, lens, pieces=pieces), key + " forward", "bag"))
    for t, (v, m, n) in enumerate(ref):
        depth = fb.grad_depth(route, q, Rk, t, n, merged=merged, pieces=pieces)
        if grads is not None:
            _note(key, fb.assert_fp32_grade(grads[t], v, m, depth, f"{key} dG{t}", "core row"))
            fb.assert_untouched(grads[t], np.zeros_like(grads[t]), n, f"{key} dG{t}")
        delta = fb.gamma(depth) * m
        if sgd is not None:
            _note(key, fb.assert_sgd_grade(sgd[t], cores[t], v, delta, LR, f"{key} SGD core {t}"))
            fb.assert_untouched(sgd[t], cores[t], n, f"{key} SGD core {t}")
        if ada is not None:
            _note(key, fb.assert_adagrad_grade(ada[t], ada_st[t], cores[t], st0[t], v, delta, LR, EPS, f"{key} Adagrad core {t}"))
            fb.assert_untouched(ada[t], cores[t], n, f"{key} Adagrad core {t}")
            fb.assert_untouched(ada_st[t], st0[t], n, f"{key} Adagrad state {t}")


def _abi_run(nat, p, q, R, cores, ids, offs, dy, st0, plan=False, two_phase=False):
    """forward, dense gradients, fused SGD and fused Adagrad through the C ABI (ids with their offsets, no row index).
    ``two_phase``: the forward as its id-only half (``phase=1``: the grouping into the plan) and its lookup half
    (``phase=2``), the three backwards on that plan."""
    shape, ws = nat.make_shape(p, q, R), nat.Workspace()
    c = [_dev(x) for x in cores]
    I, O, dY = _dev(ids), _dev(offs), _dev(dy)
    B, nnz = offs.shape[0] - 1, ids.shape[0]
    pl = nat.new_plan(shape, nnz, I.device) if plan else None
    out = torch.full((B, int(np.prod(q))), float("nan"), device="cuda")
    if two_phase:
        assert pl is not None, "a two-phase forward leaves its grouping in a plan"
        nat.forward(shape, c, I, None, O, nnz, None, B, out, ws, pl, phase=1)
        nat.forward(shape, c, I, None, O, nnz, None, B, out, ws, pl, phase=2)
    else:
        nat.forward(shape, c, I, None, O, nnz, None, B, out, ws, pl)
    g = [torch.full_like(x, float("nan")) for x in c]
    nat.backward_dense(shape, c, I, None, nnz, None, B, dY, g, ws, pl, O)
    cs = [x.clone() for x in c]
    nat.backward_sgd(shape, cs, I, None, nnz, None, B, dY, LR, ws, pl, O)
    ca, st = [x.clone() for x in c], [_dev(s) for s in st0]
    nat.backward_adagrad(shape, ca, st, I, None, nnz, None, B, dY, LR, EPS, ws, pl, O)
    torch.cuda.synchronize()
    h = lambda ts: [x.cpu().numpy() for x in ts]
    return out.cpu().numpy(), h(g), h(cs), h(ca), h(st)
