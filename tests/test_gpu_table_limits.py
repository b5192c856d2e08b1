"""The lookup kernels on the table-size limits their dispatch allows (tests/table_limits.py), and one step past each.

An "edge" table sits on one limit of the grouped kernels (rows < 2^31 - 1, p2 <= 4096, p1 < 65536, p0 p1 <= 2^21 groups,
p0 p1 q0 q1 R2 4 < 2^31 bytes) and runs on them; the "over" table beside it must be answered by another family.  The ids of a
call are fb.skewed_bags' with the ids that sit on the limits placed among them (table_limits.limit_ids: row 0, the last two
rows, the corners of the first and the last group, the ids around 2^31 and 2^32), each once alone in a bag and once inside a
bag of several ids.  Every result is checked per element against the float64 oracle with the bounds of tests/fp32_bound.py
for the route that ran, as in test_gpu_accuracy.py: no tolerance of its own.  Each case first asserts its kernel family."""
import time

import numpy as np
import pytest
import torch

import fp32_bound as fb
import table_limits as tl
from oracle import tt_oracle as orc

pytestmark = pytest.mark.gpu

LR, EPS = 0.05, 1e-3
WORST = {}   # case -> [family, largest err / (u mag), seconds]


@pytest.fixture
def nat():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import ttemb_native
    yield ttemb_native
    ttemb_native.set_path(ttemb_native.PATH_AUTO)
    ttemb_native.set_piece_limits(0, 0)
    ttemb_native.set_wide_slab_min_ids(0)


@pytest.fixture
def report(request):
    """Per case: the family that ran, the largest err / (u mag) and the wall time."""
    key, t0 = request.node.name, time.perf_counter()
    WORST[key] = [None, 0.0, 0.0]
    yield WORST[key]
    fam, worst, _ = WORST[key]
    print(f"\n  {key}: family {fam}, largest err/(u mag) {worst:.2f}, {time.perf_counter() - t0:.1f} s", end="")


def _dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


def _host(ts):
    return [x.cpu().numpy() for x in ts]


def _route(fam, nat):
    return {nat.FAMILY_SCALAR: "scalar", nat.FAMILY_PER_BAG: "per_bag", nat.FAMILY_PER_BAG_RT: "per_bag",
            nat.FAMILY_GROUPED: "grouped", nat.FAMILY_GROUPED_WIDE: "wide"}[fam & 7]


def _check_all(rep, key, route, p, q, R, cores, ids, offs, dy, st0, out, grads, sgd, ada, ada_st):
    """test_gpu_accuracy.py's _check_all: forward, dense gradients, fused SGD cores, fused Adagrad cores and state against
    the float64 oracle, rows no id touches bit-identical."""
    note = lambda r: rep.__setitem__(1, max(rep[1], r))
    lens = np.diff(offs)
    # The oracle depends on a table only through the core rows the ids name: it runs on the table of those rows alone (digit
    # d of core t -> its rank among the digits in use), so its float64 copies follow the ids, not the 14 M floats of a core.
    # Rows no id names are compared bit for bit below, which is all the bound asks of them (value 0, magnitude 0).
    digits = orc.split_index(ids, p)
    used = [np.unique(d) for d in digits]
    pc = [int(u.size) for u in used]
    idc = np.zeros_like(ids)
    for u, d in zip(used, digits):
        idc = idc * u.size + np.searchsorted(u, d)
    cc = [c[u] for c, u in zip(cores, used)]
    want, mag = orc.tt_forward64(idc, offs, cc, pc, q, R)
    note(fb.assert_fp32_grade(out, want, mag, fb.bag_depth(route, R, lens), key + " forward", "bag"))
    ref = orc.tt_dense_backward64(idc, offs, dy, cc, pc, q, R)
    for t, (v, m, n) in enumerate(ref):
        u = used[t]
        assert u.size > 0 and n.all(), f"{key}: core {t}"
        n_all = np.zeros(p[t], dtype=np.int64)
        n_all[u] = n
        depth = fb.grad_depth(route, q, R, t, n)
        note(fb.assert_fp32_grade(grads[t][u], v, m, depth, f"{key} dG{t}", "touched core row"))
        fb.assert_untouched(grads[t], np.zeros_like(grads[t]), n_all, f"{key} dG{t}")
        delta = fb.gamma(depth) * m
        note(fb.assert_sgd_grade(sgd[t][u], cc[t], v, delta, LR, f"{key} SGD core {t}"))
        fb.assert_untouched(sgd[t], cores[t], n_all, f"{key} SGD core {t}")
        note(fb.assert_adagrad_grade(ada[t][u], ada_st[t][u], cc[t], st0[t][u], v, delta, LR, EPS, f"{key} Adagrad core {t}"))
        fb.assert_untouched(ada[t], cores[t], n_all, f"{key} Adagrad core {t}")
        fb.assert_untouched(ada_st[t], st0[t], n_all, f"{key} Adagrad state {t}")


def _abi_run(nat, p, q, R, cores, ids, offs, dy, st0, plan=False):
    """test_gpu_accuracy.py's _abi_run: forward, dense gradients, fused SGD and fused Adagrad through the C ABI (ids with
    their offsets, no row index), onto NaN-filled outputs."""
    shape, ws = nat.make_shape(p, q, R), nat.Workspace()
    c = [_dev(x) for x in cores]
    I, O, dY = _dev(ids), _dev(offs), _dev(dy)
    B, nnz = offs.shape[0] - 1, ids.shape[0]
    pl = nat.new_plan(shape, nnz, I.device) if plan else None
    out = torch.full((B, int(np.prod(q))), float("nan"), device="cuda")
    nat.forward(shape, c, I, None, O, nnz, None, B, out, ws, pl)
    g = [torch.full_like(x, float("nan")) for x in c]
    nat.backward_dense(shape, c, I, None, nnz, None, B, dY, g, ws, pl, O)
    cs = [x.clone() for x in c]
    nat.backward_sgd(shape, cs, I, None, nnz, None, B, dY, LR, ws, pl, O)
    ca, st = [x.clone() for x in c], [_dev(s) for s in st0]
    nat.backward_adagrad(shape, ca, st, I, None, nnz, None, B, dY, LR, EPS, ws, pl, O)
    torch.cuda.synchronize()
    nat.status()
    return out.cpu().numpy(), _host(g), _host(cs), _host(ca), _host(st)


def _run_case(nat, rep, key, want):
    """The call ``tl.CALLS[key]``: ``want(fam)`` asserts its family; then the four results within the bound of the route that
    runs."""
    table, n_ids, seed = tl.CALLS[key]
    p, q, r = tl.TABLES[table]
    R = [1] + r + [1]
    cores, ids, offs, dy, st0 = tl.call_inputs(p, q, R, n_ids, seed)
    fam = nat.kernel_family(nat.make_shape(p, q, R), ids.shape[0], offs.shape[0] - 1, True)
    rep[0] = fam
    want(fam)
    res = _abi_run(nat, p, q, R, cores, ids, offs, dy, st0, plan=fam & 7 >= 3)
    _check_all(rep, key, _route(fam, nat), p, q, R, cores, ids, offs, dy, st0, *res)


# (table, which chain kernels a call of its size (tl.CALLS) takes: the route flags of the host answer)
EDGE_CASES = [
    ("rows_edge", ("prefix", "group_products")),       # rows = 2^31 - 2: uint32 ids, uu / (p1 p2), the clamp at rows
    ("p2_edge", ()),                                   # p2 = 4096: i2 = 4095 in the sort key and the dG2 reduce's counters
    ("p1_edge", ("prefix",)),                          # p1 = 65535: grid.y, the p1 >= 256 form of the finalize kernel
    ("groups_edge", ("prefix",)),                      # 512 ranges x 2^12 groups: the last group is 2^21 - 1
    ("groups_ragged", ("prefix",)),                    # 510 ranges, the last one short
    ("bytes_edge", ("prefix",)),                       # the last prefix product ends 2048 bytes below 2 GiB
    ("wide_edge", ()),                                 # the same on the wide-rank chain (rank 64)
]


@pytest.mark.parametrize("case", EDGE_CASES, ids=[c[0] for c in EDGE_CASES])
def test_grouped_kernels_on_their_limit(nat, report, case):
    table, flags = case
    assert table in tl.EDGE_TABLES
    nat.set_path(nat.PATH_FAST3)
    grouped = nat.FAMILY_GROUPED_WIDE if table == "wide_edge" else nat.FAMILY_GROUPED

    def want(fam):
        assert fam & 7 == grouped, (table, fam)
        assert bool(fam & nat.FAMILY_PREFIX_IN_CHAIN) == ("prefix" in flags), (table, fam)
        assert bool(fam & nat.FAMILY_GROUP_PRODUCTS_IN_CHAIN) == ("group_products" in flags), (table, fam)
    _run_case(nat, report, table, want)


# (table, family under PATH_FAST3, family under PATH_AUTO)
OVER_CASES = [
    ("rows_over", 0, 0),        # 2^31 rows: no 32-bit family takes it, the scalar kernels decode 64-bit ids
    ("rows_far_over", 0, 0),    # 2^33 rows: ids past 2^32
    ("p2_over", 0, 1),
    ("p1_over", 0, 1),
    ("groups_over", 0, 1),
    ("bytes_over", 0, 1),
    ("wide_over", 0, 1),
]


@pytest.mark.parametrize("path", ["fast3", "auto"])
@pytest.mark.parametrize("case", OVER_CASES, ids=[c[0] for c in OVER_CASES])
def test_one_step_past_a_limit_another_family_answers(nat, report, case, path):
    table, fam_fast3, fam_auto = case
    nat.set_path(nat.PATH_FAST3 if path == "fast3" else nat.PATH_AUTO)

    def want(fam):
        assert fam & 7 not in (nat.FAMILY_GROUPED, nat.FAMILY_GROUPED_WIDE), (table, path, fam)
        assert fam == (fam_fast3 if path == "fast3" else fam_auto), (table, path, fam)
    _run_case(nat, report, f"{table}_{path}", want)


@pytest.mark.parametrize("path", ["auto", "per_bag"])
@pytest.mark.parametrize("table", ["rows_edge", "rows_edge_rt"])
def test_per_bag_kernels_on_the_last_table_with_32_bit_ids(nat, report, table, path):
    """2^31 - 2 rows on the per-bag MFMA kernels: the templated ones (the 32-bit split of ttemb_small3.inc) and the
    run-time-shape ones of ttemb_rt3.inc (q = 6, 4, 4)."""
    nat.set_path(nat.PATH_AUTO if path == "auto" else nat.PATH_PER_BAG)
    fam_want = nat.FAMILY_PER_BAG_RT if table == "rows_edge_rt" else nat.FAMILY_PER_BAG

    def want(fam):
        assert fam == fam_want, (table, path, fam)
    _run_case(nat, report, f"{table}_{path}", want)


@pytest.mark.parametrize("table", ["rows_over", "rows_far_over"])
def test_exact_mode_on_tables_of_2_31_rows_and_more(nat, report, table):
    """The exact kernels decode 64-bit ids: dense gradients, SGD and Adagrad within the "exact" depths on tables of 2^31 and
    2^33 rows, and a second run bit-identical to the first."""
    p, q, r = tl.TABLES[table]
    R = [1] + r + [1]
    shape, ws = nat.make_shape(p, q, R), nat.Workspace()
    assert nat.exact_unsupported_reason(shape) is None
    _, n_ids, seed = tl.CALLS[table + "_exact"]
    cores, ids, offs, dy, st0 = tl.call_inputs(p, q, R, n_ids, seed)
    assert ids.max() == tl.rows_of(p) - 1 >= 2 ** 31 - 1   # (past what an int32 or, at 2^33 rows, a uint32 holds)
    I, O, dY = _dev(ids), _dev(offs), _dev(dy)
    B = offs.shape[0] - 1
    report[0] = "exact"

    def run():
        c = [_dev(x) for x in cores]
        out = torch.full((B, int(np.prod(q))), float("nan"), device="cuda")
        nat.forward_exact(shape, c, I, O, B, out, ws)
        g = [torch.full_like(x, float("nan")) for x in c]
        nat.backward_exact(shape, c, I, O, B, dY, ws, d_cores=g)
        cs = [x.clone() for x in c]
        nat.backward_exact(shape, cs, I, O, B, dY, ws, lr=LR)
        ca, st = [x.clone() for x in c], [_dev(s) for s in st0]
        nat.backward_exact(shape, ca, I, O, B, dY, ws, opt_state=st, lr=LR, eps=EPS)
        torch.cuda.synchronize()
        nat.status()
        return [out, *g, *cs, *ca, *st]
    first, second = run(), run()
    for k, (a, b) in enumerate(zip(first, second)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{table}: result {k} differs between two runs"
    h = _host(first)
    _check_all(report, table + " exact", "exact", p, q, R, cores, ids, offs, dy, st0, h[0], h[1:4], h[4:7], h[7:10], h[10:13])


@pytest.mark.parametrize("family", ["per_bag", "grouped"])
def test_captured_int32_ids_up_to_the_last_row(nat, report, family):
    """``capture(nnz, B, variable=True)`` on the table of 2^31 - 2 rows with int32 ids, rows - 1 = 2^31 - 3 among them (the
    largest positive value ``ttemb_stage_call`` can widen), against the eager module on int64 ids.  Tolerances: those of
    test_gpu_capture_variable.py::test_variable_capture_trains_like_the_eager_module for plain SGD (float atomics:
    summation order only), on cores brought to the same spread (standard deviation 0.2)."""
    from FBTT import tt_embeddings_ops as ops
    p, q, r = tl.TABLES["rows_edge"]
    rows, cap_n = tl.rows_of(p), 4096
    mk = lambda: ops.TTEmbeddingBag(rows, int(np.prod(q)), r, p, q, optimizer=ops.OptimType.SGD, sparse=True, use_cache=False,
                                    weight_dist="normal", learning_rate=0.1)
    torch.manual_seed(11)
    a, b = mk(), mk()
    for ca, cb in zip(a.tt_cores, b.tt_cores):
        ca.data.mul_(0.2 / float(ca.data.std()))
        cb.data.copy_(ca.data)
    nat.set_path(nat.PATH_AUTO if family == "per_bag" else nat.PATH_FAST3)
    fam = nat.kernel_family(b._shape, cap_n, cap_n, True)
    report[0] = fam
    assert fam & 7 == (nat.FAMILY_PER_BAG if family == "per_bag" else nat.FAMILY_GROUPED), fam
    cap = b.capture(cap_n, cap_n, variable=True)
    rng = np.random.default_rng(8)
    for n_ids in (4000, 300):
        ids, offs = fb.skewed_bags(rng, p, n_ids, long_bag=0)
        tl.place_limit_ids(ids, offs, tl.limit_ids(p))
        assert ids.max() == rows - 1 == 2 ** 31 - 3 and ids.shape[0] <= cap_n
        dy = _dev(((rng.random((offs.shape[0] - 1, int(np.prod(q)))) - 0.5) * 0.05).astype(np.float32))
        out_a = a(_dev(ids), _dev(offs))
        out_b = cap(_dev(ids.astype(np.int32)), _dev(offs.astype(np.int32)))
        torch.testing.assert_close(out_b, out_a, rtol=1e-5, atol=1e-6)
        out_a.backward(dy)
        out_b.backward(dy)
        torch.cuda.synchronize()
        assert torch.equal(cap.indices[:ids.shape[0]], _dev(ids))   # (widened without a sign: rows - 1 stays positive)
        for ca, cb in zip(a.tt_cores, b.tt_cores):
            torch.testing.assert_close(cb.data, ca.data, rtol=1e-4, atol=1e-6)
            scale = float(ca.data.abs().max())
            report[1] = max(report[1], float((cb.data - ca.data).abs().max()) / (fb.U * scale))
    nat.status()
