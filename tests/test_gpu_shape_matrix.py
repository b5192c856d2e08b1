"""Every compiled kernel shape in every form it can reach (tests/shape_matrix.py) against the float64 oracle, element by
element, with the fp32 rounding bound of tests/fp32_bound.py: forward per bag, every core-row gradient, the fused SGD cores,
the fused Adagrad cores and state, and bit-identical rows where no id touches.  Inputs as in test_gpu_accuracy.py (row scales
of 10^U(-3, 0), skewed ids, cold rows, one bag of 600 ids).  Each case first asserts the family, the route flags and -- through
the backward workspace query, for the forms no flag reports -- the form it lands on.  The largest err / (u mag) per case is
printed at the end of the module; DESIGN.md section 2 keeps the table."""
import numpy as np
import pytest
import torch

import shape_matrix as sm
from abi_check import _abi_run, _check_all, _inputs
from oracle import tt_oracle as orc

pytestmark = pytest.mark.gpu

WORST = {}   # case key -> largest err / (u mag) of any element of any of its checks


@pytest.fixture(scope="module")
def nat():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import ttemb_native
    yield ttemb_native
    ttemb_native.set_path(ttemb_native.PATH_AUTO)
    ttemb_native.set_piece_limits(0, 0)
    ttemb_native.set_wide_slab_min_ids(0)
    forms = {c.key: c for c in sm.CASES}
    for k in WORST:
        print(f"\n  {k:28s} {' + '.join(forms[k].forms):50s} largest err/(u mag) {WORST[k]:.2f}", end="")


_SOLVED = {}   # the inputs of the last table and their float64 answers: consecutive cases on one table share them, unchanged


def _solved(case, R):
    key = (tuple(case.p), tuple(case.q), tuple(case.r), case.n_ids)
    if key not in _SOLVED:
        _SOLVED.clear()
        seed = sum(case.p) + 7 * sum(case.q) + sum(case.r) + case.n_ids
        cores, ids, offs, dy, st0 = _inputs(case.p, case.q, R, case.n_ids, seed=seed)
        _SOLVED[key] = (cores, ids, offs, dy, st0, (orc.tt_forward64(ids, offs, cores, case.p, case.q, R),
                                                   orc.tt_dense_backward64(ids, offs, dy, cores, case.p, case.q, R)))
    return _SOLVED[key]


def _note(key, r):
    WORST[key] = max(WORST.get(key, 0.0), r)


@pytest.mark.parametrize("case", sm.CASES, ids=[c.key for c in sm.CASES])
def test_shape_and_form_within_the_fp32_bound(nat, case):
    assert (sm.SCALAR, sm.PER_BAG, sm.PER_BAG_RT, sm.GROUPED, sm.WIDE, sm.MERGED, sm.PADDED, sm.PREFIX, sm.PRODUCTS) == (
        nat.FAMILY_SCALAR, nat.FAMILY_PER_BAG, nat.FAMILY_PER_BAG_RT, nat.FAMILY_GROUPED, nat.FAMILY_GROUPED_WIDE,
        nat.FAMILY_MERGED, nat.FAMILY_PADDED, nat.FAMILY_PREFIX_IN_CHAIN, nat.FAMILY_GROUP_PRODUCTS_IN_CHAIN)
    R = [1] + case.r + [1]
    nat.set_path({"auto": nat.PATH_AUTO, "generic": nat.PATH_GENERIC, "fast3": nat.PATH_FAST3}[case.path])
    nat.set_piece_limits(*case.pieces)
    nat.set_wide_slab_min_ids(case.wide_slab)
    cores, ids, offs, dy, st0, oracle = _solved(case, R)
    nnz, B = ids.shape[0], offs.shape[0] - 1
    shape = nat.make_shape(case.p, case.q, R)
    # family, flags, form
    fam = nat.kernel_family(shape, nnz, B, True)
    assert fam & ~nat.FAMILY_ROUTE_FLAGS == case.family, (case.key, fam)
    assert fam & nat.FAMILY_ROUTE_FLAGS == case.flags, (case.key, fam)
    grouped = case.family & 7 >= nat.FAMILY_GROUPED
    assert (nat.plan_bytes(shape, nnz) > 0) == grouped, case.key
    form = sm.backward_form(case)
    if form is not None:   # an E table or none, one dG2 slab or one per tile: what the backward's workspace holds
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        extra = nat.workspace_bytes(shape, nat.OP_BACKWARD, nnz, B) - nat.workspace_bytes(shape, nat.OP_FORWARD, nnz, B)
        assert extra == sm.backward_tables_bytes(case.p, case.q, case.r, nnz, form, cus), (case.key, form, extra)
    if case.family & 7 == nat.FAMILY_GROUPED:   # (the rules of the forms no query answers: ids per group against 8 / 16 / 64)
        view = [case.p[0], 1, case.p[1]] if len(case.p) == 2 else case.p
        assert sm.grouped_forms(view, list(case.inst[:3]), case.inst[4], nnz, sm.FAST3[case.inst], case.two_phase) == case.forms
    # the run, every element checked
    try:
        res = _abi_run(nat, case.p, case.q, R, cores, ids, offs, dy, st0, plan=grouped, two_phase=case.two_phase)
        nat.status()
    except RuntimeError as e:   # a faulted device serves no later case: the module ends here, with the case's name
        if "illegal memory access" in str(e) or "HIP error" in str(e):
            pytest.exit(f"{case.key}: the device faulted, no further case is started on it: {e}", returncode=3)
        raise
    assert all(np.isfinite(x).all() for x in [res[0]] + [a for part in res[1:] for a in part]), case.key
    _check_all(case.key, sm.route_of(case), case.p, case.q, R, R, cores, ids, offs, dy, st0, *res,
               merged=bool(case.family & nat.FAMILY_MERGED), note=_note, oracle=oracle)
