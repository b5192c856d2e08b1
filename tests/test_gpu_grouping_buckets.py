"""The two-launch grouping pass (decode into fixed-capacity range buckets, overflow blocks on per-range lists, then place) on
the id distributions that fill its buckets unevenly: uniform, everything in one range, one hot range, duplicates and ragged
bags, calls in pieces, several tables, graph replay over several calls, and an expired wait.  Tolerances as in
test_gpu_parity.py: forward atol 1e-4 (+ rtol 1e-5), dense gradients 1e-4 of their largest magnitude."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import seeded_cores

pytestmark = pytest.mark.gpu

P, Q, R = [125, 140, 140], [4, 5, 5], [1, 16, 16, 1]   # the products table: 17 500 groups in 274 ranges of 64
ROWS = P[0] * P[1] * P[2]


@pytest.fixture(scope="module")
def nat():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import ttemb_native
    ttemb_native.set_path(ttemb_native.PATH_FAST3)
    yield ttemb_native
    ttemb_native.set_path(ttemb_native.PATH_AUTO)
    ttemb_native.set_piece_limits(0, 0)
    ttemb_native.set_spin_limit(0)


@pytest.fixture(scope="module")
def orc():
    from oracle import tt_oracle
    return tt_oracle


@pytest.fixture(scope="module")
def cores():
    return seeded_cores(P, Q, R, 5, 0.3)


def ids_in_range(rng, n, r):
    """n ids whose group i1 * p0 + i0 lies in range r (groups 64 r ... 64 r + 63)."""
    g = rng.integers(64 * r, min(64 * r + 64, P[0] * P[1]), size=n)
    i1, i0 = g // P[0], g % P[0]
    return i0 * (P[1] * P[2]) + i1 * P[2] + rng.integers(0, P[2], size=n)


def ragged(rng, n, mean=3):
    lens = rng.integers(0, 2 * mean + 1, size=n)
    lens[::7] = 0
    offs = np.concatenate([[0], np.cumsum(lens)])
    offs = offs[offs < n]
    return np.concatenate([offs, [n, n]]).astype(np.int64)


def check(nat, orc, cores, ids, offs, ws=None, backward=True):
    shape = nat.make_shape(P, Q, R)
    assert nat.kernel_family(shape, len(ids), len(offs) - 1) & ~nat.FAMILY_ROUTE_FLAGS == nat.FAMILY_GROUPED
    ws = ws or nat.Workspace()
    c = [torch.as_tensor(x).cuda() for x in cores]
    idx, o = torch.as_tensor(ids, dtype=torch.int64).cuda(), torch.as_tensor(offs).cuda()
    n, B, D = len(ids), len(offs) - 1, int(np.prod(Q))
    plan = torch.empty(nat.plan_bytes(shape, n), dtype=torch.uint8, device="cuda")
    out = torch.zeros((B, D), device="cuda")
    nat.forward(shape, c, idx, None, o, n, None, B, out, ws, plan=plan)
    want = orc.tt_forward(ids, offs, cores, P, Q, R)
    torch.testing.assert_close(out.cpu(), torch.as_tensor(want, dtype=torch.float32), rtol=1e-5, atol=1e-4)
    if backward:
        d_out = np.random.default_rng(n).random((B, D)).astype(np.float32) - 0.5
        grads = [torch.zeros_like(x) for x in c]
        nat.backward_dense(shape, c, idx, None, n, None, B, torch.as_tensor(d_out).cuda(), grads, ws, plan=plan, offsets=o)
        for g, w in zip(grads, orc.tt_dense_backward(ids, offs, d_out, cores, P, Q, R)):
            torch.testing.assert_close(g.cpu(), torch.as_tensor(w, dtype=torch.float32), rtol=0,
                                       atol=1e-4 * max(float(np.abs(w).max()), 1e-6))


def test_uniform_ids_at_the_headline_size(nat, orc, cores):
    rng = np.random.default_rng(1)
    ids = rng.choice(ROWS, size=409600, replace=False).astype(np.int64)
    check(nat, orc, cores, ids, np.arange(409601, dtype=np.int64))


def test_every_id_in_one_range(nat, orc, cores):
    """Nearly every id goes to overflow blocks: one long list per bank's share of the slices."""
    rng = np.random.default_rng(2)
    for r in (0, 273):   # (the last range holds 28 groups)
        ids = ids_in_range(rng, 60000, r)
        check(nat, orc, cores, ids, np.arange(60001, dtype=np.int64))


def test_one_hot_range_among_uniform_ones(nat, orc, cores):
    rng = np.random.default_rng(3)
    ids = np.concatenate([rng.integers(0, ROWS, size=50000), ids_in_range(rng, 30000, 100)])
    rng.shuffle(ids)
    check(nat, orc, cores, ids, np.arange(len(ids) + 1, dtype=np.int64))


def test_duplicates_ragged_and_empty_bags_odd_size(nat, orc, cores):
    rng = np.random.default_rng(4)
    n = 12345   # not a multiple of the slice size
    ids = rng.integers(0, ROWS, size=n)
    ids[::5] = ids[0]
    ids[1::9] = ids_in_range(rng, len(ids[1::9]), 7)
    check(nat, orc, cores, ids, ragged(rng, n))


def test_a_call_in_pieces(nat, orc, cores):
    rng = np.random.default_rng(5)
    n = 30000
    ids = np.concatenate([rng.integers(0, ROWS, size=n // 2), ids_in_range(rng, n - n // 2, 50)])
    nat.set_piece_limits(rows=4000, ids=7000)
    try:
        check(nat, orc, cores, ids, ragged(rng, n))
    finally:
        nat.set_piece_limits(0, 0)


def test_several_tables(nat):
    from FBTT import tt_embeddings_ops as ops
    Tn, B = 3, 6000
    emb = ops.TableBatchedTTEmbeddingBag(Tn, ROWS, 100, R[1:-1], P, Q, sparse=False, use_cache=False, weight_dist="uniform")
    g = np.random.default_rng(6)
    lens = g.integers(0, 5, size=Tn * B)
    lens[::13] = 0
    offs = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int64).cuda()
    nnz = int(offs[-1])
    ids = g.integers(0, ROWS, size=nnz)
    ids[::3] = ids_in_range(g, len(ids[::3]), 200)
    idx = torch.tensor(ids).cuda()
    shape = nat.make_shape(P, Q, R)
    for k in range(Tn):   # every table's window takes the grouped kernels
        n_k = int(offs[(k + 1) * B] - offs[k * B])
        assert nat.kernel_family(shape, n_k, B) & ~nat.FAMILY_ROUTE_FLAGS == nat.FAMILY_GROUPED, n_k
    out = emb(idx, offs)
    dy = (torch.rand(Tn, B, 100, device="cuda") - 0.5) * 0.2
    out.backward(dy)
    bounds = offs[::B].tolist()
    for k in range(Tn):
        cs = [c.detach()[k:k + 1].clone().requires_grad_(True) for c in emb.tt_cores]
        full = ops.tt_matrix_to_full(P, Q, emb.tt_ranks, cs, [1, 0, 2, 3])
        lo, hi = bounds[k], bounds[k + 1]
        o = F.embedding_bag(idx[lo:hi], full, offs[k * B:(k + 1) * B + 1] - lo, mode="sum", include_last_offset=True)
        torch.testing.assert_close(out[k].detach(), o.detach(), rtol=1e-5, atol=1e-4)
        o.backward(dy[k])
        for c, cr in zip(emb.tt_cores, cs):
            torch.testing.assert_close(c.grad[k:k + 1], cr.grad, rtol=0, atol=1e-4 * max(float(cr.grad.abs().max()), 1e-6))


def test_graph_replay_over_several_calls(nat, orc, cores):
    """One captured forward, replayed on skewed and uniform id sets in turn: every replay is a new call number, so the list
    heads and counters a replay before left (other tags) must read as empty."""
    shape = nat.make_shape(P, Q, R)
    n = 40000
    D = int(np.prod(Q))
    ws = nat.Workspace()
    c = [torch.as_tensor(x).cuda() for x in cores]
    idx = torch.zeros(n, dtype=torch.int64, device="cuda")
    o = torch.arange(n + 1, dtype=torch.int64, device="cuda")
    plan = torch.empty(nat.plan_bytes(shape, n), dtype=torch.uint8, device="cuda")
    out = torch.zeros((n, D), device="cuda")
    rng = np.random.default_rng(7)
    sets = [ids_in_range(rng, n, 3), rng.integers(0, ROWS, size=n), ids_in_range(rng, n, 3),
            np.concatenate([rng.integers(0, ROWS, size=n // 2), ids_in_range(rng, n - n // 2, 90)])]
    idx.copy_(torch.as_tensor(sets[1]))
    nat.forward(shape, c, idx, None, o, n, None, n, out, ws, plan=plan)   # (warm-up outside the capture: the workspace exists)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(gr, stream=s):
            nat.forward(shape, c, idx, None, o, n, None, n, out, ws, plan=plan)
    torch.cuda.current_stream().wait_stream(s)
    offs = np.arange(n + 1, dtype=np.int64)
    for ids in sets + sets[::-1]:
        idx.copy_(torch.as_tensor(ids))
        gr.replay()
        torch.cuda.synchronize()
        want = orc.tt_forward(ids, offs, cores, P, Q, R)
        torch.testing.assert_close(out.cpu(), torch.as_tensor(want, dtype=torch.float32), rtol=1e-5, atol=1e-4)


def test_an_expired_wait_still_poisons_with_overflow_lists(nat, orc, cores):
    """A call whose decode step writes overflow blocks (one range holds far more ids than its buckets) and whose place step's
    look-back expires: NaN rows and the error, never a plausible table.  A call with the default limit runs first on the same
    workspace, so that the counters carry the next call's tag and the decode step does not need its bounded take-over."""
    shape = nat.make_shape(P, Q, R)
    rng = np.random.default_rng(8)
    n = 30000
    ids = np.concatenate([rng.integers(0, ROWS, size=n // 2), ids_in_range(rng, n - n // 2, 10)])
    lay = nat.grouping_layout(shape, n)
    assert (n - n // 2) / lay["banks"] > 4 * lay["cap"], lay   # range 10 overflows its buckets in every bank
    offs = np.arange(n + 1, dtype=np.int64)
    ws = nat.Workspace()
    check(nat, orc, cores, ids, offs, ws=ws, backward=False)
    c = [torch.as_tensor(x).cuda() for x in cores]
    idx, o = torch.as_tensor(ids).cuda(), torch.as_tensor(offs).cuda()
    plan = torch.empty(nat.plan_bytes(shape, n), dtype=torch.uint8, device="cuda")
    out = torch.zeros((n, int(np.prod(Q))), device="cuda")
    nat.status()
    nat.set_spin_limit(-1)
    try:
        nat.forward(shape, c, idx, None, o, n, None, n, out, ws, plan=plan)
        torch.cuda.synchronize()
    finally:
        nat.set_spin_limit(0)
    assert bool(torch.isnan(out).all()), "a forward whose grouping pass gave up must not return numbers"
    with pytest.raises(RuntimeError, match="look-back of the place step"):
        nat.status()
    check(nat, orc, cores, ids, offs, ws=ws, backward=False)   # the same workspace, the default limit: the oracle's numbers


def test_calls_of_varying_size_on_one_workspace(nat, orc, cores):
    """Calls of different sizes on one workspace move the grouping tables: each call's buckets and overflow blocks lie where
    the call before left entries of multi-id bags (row | kMultiBit).  No such entry may read as a tagged word of a later call."""
    rng = np.random.default_rng(9)
    ws = nat.Workspace()
    for n in (30000, 21000, 37000, 12345, 30000):
        ids = np.concatenate([rng.integers(0, ROWS, size=n // 2), ids_in_range(rng, n - n // 2, int(rng.integers(0, 274)))])
        rng.shuffle(ids)
        check(nat, orc, cores, ids, ragged(rng, n), ws=ws, backward=False)
