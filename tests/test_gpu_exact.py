"""Exact mode on the GPU: the exact kernels against the CPU oracle, bit identity across runs / workspace contents / grid
sizes / concurrent work / graph replay, and exact training through the module.  Tolerances as in test_gpu_parity.py."""
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (p, q, inner ranks): small-p variants of products, papers100M r32, 4.4.8 / 8, rank 12, a 2-core table and two 4-core
# tables (a merged pair: the reference scripts' q = 2.4.4.4 at rank 16, and one whose best pair is not the first)
SHAPES = [([23, 29, 31], [4, 5, 5], [16, 16]), ([11, 13, 17], [8, 4, 4], [32, 32]), ([9, 10, 12], [4, 4, 8], [8, 8]),
          ([23, 29, 31], [4, 5, 5], [12, 12]), ([90, 110], [8, 8], [16]), ([7, 6, 5, 6], [2, 4, 4, 4], [16, 16, 16]),
          ([9, 8, 3, 4], [4, 4, 2, 2], [8, 4, 8])]
PRODUCTS = ([125, 140, 140], [4, 5, 5], [16, 16])
FOUR_CORE = ([50, 60, 60, 60], [2, 4, 4, 4], [16, 16, 16])   # the reference scripts' 4-core table


@pytest.fixture(scope="module")
def nat():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import ttemb_native
    yield ttemb_native
    ttemb_native.set_exact_grid(0)


@pytest.fixture(scope="module")
def orc():
    from oracle import tt_oracle
    return tt_oracle


def _cores(p, q, r, seed):
    rng = np.random.default_rng(seed)
    R = [1] + list(r) + [1]
    return [((rng.random((p[t], R[t] * q[t] * R[t + 1])) - 0.5) * 0.8).astype(np.float32) for t in range(len(p))]


def _ids(rows, n, seed, heavy=0):
    """Zipf ids (heavy duplicates), plus `heavy` copies of one id spread over the list."""
    rng = np.random.default_rng(seed)
    ids = (rng.zipf(1.3, size=n) - 1) % rows
    if heavy:
        ids = np.concatenate([ids, np.full(heavy, rows // 3)])
        rng.shuffle(ids)
    return ids.astype(np.int64)


def _offsets(n, seed, mean=4):
    """Ragged bags with empty ones among them."""
    rng = np.random.default_rng(seed + 1)
    lens = rng.integers(0, 2 * mean + 1, size=n // mean + 8)
    lens[::7] = 0
    offs = np.concatenate([[0], np.cumsum(lens)])
    offs = offs[offs < n]
    return np.concatenate([offs, [n]]).astype(np.int64)


def _dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


def _run(nat, p, q, r, cores, ids, offs, dy, lr=0.05, eps=1e-3):
    """forward, dense gradients, SGD-updated cores, Adagrad-updated cores and state, all through the exact calls."""
    shape = nat.make_shape(p, q, r)
    ws = nat.Workspace()
    c = [_dev(x) for x in cores]
    I, O = _dev(ids), _dev(offs)
    B = len(offs) - 1
    out = torch.empty((B, int(np.prod(q))), dtype=torch.float32, device="cuda")
    nat.forward_exact(shape, c, I, O, B, out, ws)
    dY = _dev(dy)
    g = [torch.empty_like(x) for x in c]
    nat.backward_exact(shape, c, I, O, B, dY, ws, d_cores=g)
    cs = [x.clone() for x in c]
    nat.backward_exact(shape, cs, I, O, B, dY, ws, lr=lr)
    ca = [x.clone() for x in c]
    st = [torch.full_like(x, 0.25) for x in c]
    nat.backward_exact(shape, ca, I, O, B, dY, ws, opt_state=st, lr=lr, eps=eps)
    torch.cuda.synchronize()
    return out, g, cs, ca, st


@pytest.mark.parametrize("case", range(len(SHAPES)))
def test_exact_against_oracle(nat, orc, case):
    p, q, r = SHAPES[case]
    cores = _cores(p, q, r, case)
    rows = int(np.prod(p))
    ids = _ids(rows, 3000, case, heavy=600)   # 600 copies of one id: its rows' lists cross several chunks
    offs = _offsets(len(ids), case)
    B = len(offs) - 1
    dy = ((np.random.default_rng(case + 7).random((B, int(np.prod(q)))) - 0.5)).astype(np.float32)
    out, g, cs, ca, st = _run(nat, p, q, r, cores, ids, offs, dy)
    R = [1] + r + [1]
    want = orc.tt_forward(ids, offs, cores, p, q, R)
    np.testing.assert_allclose(out.cpu().numpy(), want, atol=1e-4, rtol=1e-5)
    grads = orc.tt_dense_backward(ids, offs, dy, cores, p, q, R)
    for t, (a, b) in enumerate(zip(g, grads)):
        scale = max(float(np.abs(b).max()), 1e-6)
        assert float(np.abs(a.cpu().numpy() - b).max()) <= 1e-4 * scale, f"dense grad of core {t}"
    for t, (a, b) in enumerate(zip(cs, orc.sgd_step(cores, grads, 0.05))):
        assert float(np.abs(a.cpu().numpy() - b).max()) <= 1e-5 + 1e-4 * 0.05 * float(np.abs(grads[t]).max())
    new_c, new_s = orc.adagrad_step(cores, [np.full_like(x, 0.25) for x in cores], grads, 0.05, 1e-3)
    for t in range(len(cores)):
        np.testing.assert_allclose(ca[t].cpu().numpy(), new_c[t], atol=1e-5, rtol=1e-5)
        np.testing.assert_allclose(st[t].cpu().numpy(), new_s[t], atol=1e-5, rtol=1e-4)
    # rows no id touches stay bitwise as they were, and so does their state
    for t, x in enumerate(orc.split_index(ids, p)):
        untouched = np.setdiff1d(np.arange(p[t]), x)
        assert np.array_equal(cs[t].cpu().numpy()[untouched], cores[t][untouched])
        assert np.array_equal(ca[t].cpu().numpy()[untouched], cores[t][untouched])
        assert np.all(st[t].cpu().numpy()[untouched] == np.float32(0.25))


def test_exact_one_id_repeated_100k_times(nat, orc):
    p, q, r = PRODUCTS
    cores = _cores(p, q, r, 11)
    ids = _ids(int(np.prod(p)), 2000, 11, heavy=100_000)
    offs = _offsets(len(ids), 11, mean=16)
    B = len(offs) - 1
    dy = ((np.random.default_rng(3).random((B, 100)) - 0.5) * 0.1).astype(np.float32)
    out, g, cs, _, _ = _run(nat, p, q, r, cores, ids, offs, dy)
    R = [1] + r + [1]
    np.testing.assert_allclose(out.cpu().numpy(), orc.tt_forward(ids, offs, cores, p, q, R), atol=1e-4, rtol=1e-5)
    grads = orc.tt_dense_backward(ids, offs, dy, cores, p, q, R)
    for a, b in zip(g, grads):
        assert float(np.abs(a.cpu().numpy() - b).max()) <= 1e-4 * float(np.abs(b).max())


def test_exact_no_ids(nat):
    p, q, r = SHAPES[0]
    cores = _cores(p, q, r, 0)
    offs = np.zeros(5, dtype=np.int64)
    ids = np.zeros(0, dtype=np.int64)
    out, g, cs, ca, st = _run(nat, p, q, r, cores, ids, offs, np.ones((4, 100), np.float32))
    assert torch.count_nonzero(out) == 0
    for t in range(3):
        assert torch.count_nonzero(g[t]) == 0
        assert np.array_equal(cs[t].cpu().numpy(), cores[t]) and np.array_equal(ca[t].cpu().numpy(), cores[t])
        assert bool((st[t] == 0.25).all())


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("table", ["products", "four_core"])
def test_exact_is_bit_reproducible(nat, table):
    """409 600 Zipf ids in ragged bags: two runs, a NaN-filled workspace, a 7-workgroup grid and a matmul on a side stream
    all give the same bits."""
    p, q, r = PRODUCTS if table == "products" else FOUR_CORE
    D = int(np.prod(q))
    cores = _cores(p, q, r, 5)
    ids = _ids(int(np.prod(p)), 409_600, 5)
    offs = _offsets(len(ids), 5)
    B = len(offs) - 1
    dy = ((np.random.default_rng(9).random((B, D)) - 0.5) * 0.1).astype(np.float32)
    shape = nat.make_shape(p, q, r)
    I, O, dY = _dev(ids), _dev(offs), _dev(dy)

    def once(ws):
        c = [_dev(x) for x in cores]
        out = torch.empty((B, D), dtype=torch.float32, device="cuda")
        nat.forward_exact(shape, c, I, O, B, out, ws)
        g = [torch.empty_like(x) for x in c]
        nat.backward_exact(shape, c, I, O, B, dY, ws, d_cores=g)
        nat.backward_exact(shape, c, I, O, B, dY, ws, lr=0.1)
        torch.cuda.synchronize()
        return [out] + g + c

    ws = nat.Workspace()
    ref = once(ws)
    assert _same(ref, once(ws)), "two runs differ"
    ws.buf.view(torch.uint8).fill_(0xFF)   # NaN bytes wherever the workspace is read before it is written
    assert _same(ref, once(ws)), "the workspace's previous contents changed a result"
    nat.set_exact_grid(7)
    try:
        assert _same(ref, once(nat.Workspace())), "the grid size changed a result"
    finally:
        nat.set_exact_grid(0)
    side = torch.cuda.Stream()
    a = torch.randn(4096, 4096, device="cuda")
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(4):
            a = a @ a * 1e-3
    got = once(ws)
    torch.cuda.synchronize()
    assert _same(ref, got), "concurrent work changed a result"


def _module(seed=0, shape=PRODUCTS, scale=30.0, **kw):
    from FBTT.tt_embeddings_ops import OptimType, TTEmbeddingBag
    p, q, r = shape
    torch.manual_seed(seed)
    args = dict(optimizer=OptimType.EXACT_SGD, learning_rate=1e-3, sparse=True, use_cache=False, weight_dist="normal")
    args.update(kw)
    m = TTEmbeddingBag(int(np.prod(p)), int(np.prod(q)), r, p, q, **args)
    for c in m.tt_cores:
        c.data.mul_(scale)
    return m


def _batch(step, n=20_000, rows=125 * 140 * 140, bag_mean=4):
    ids = _dev(_ids(rows, n, 100 + step))
    offs = _dev(_offsets(n, 100 + step, bag_mean))
    dy = torch.randn((offs.numel() - 1, 100), device="cuda", generator=torch.Generator("cuda").manual_seed(step)) * 0.1
    return ids, offs, dy


def test_exact_sgd_training_is_reproducible(nat):
    runs = []
    for _ in range(2):
        m = _module(seed=1)
        for step in range(5):
            ids, offs, dy = _batch(step)
            m(ids, offs).backward(dy)
        torch.cuda.synchronize()
        runs.append([c.detach().clone() for c in m.tt_cores])
    assert all(bool(torch.isfinite(c).all()) for c in runs[0])
    assert _same(*runs)


def test_exact_dense_adagrad_under_deterministic_algorithms(nat):
    from FBTT.tt_embeddings_ops import OptimType
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        runs = []
        for _ in range(2):
            m = _module(seed=2, optimizer=OptimType.EXACT_ADAGRAD, sparse=False)
            opt = torch.optim.Adagrad(m.tt_cores.parameters(), lr=0.05)
            for step in range(5):
                ids, offs, dy = _batch(step)
                opt.zero_grad()
                m(ids, offs).backward(dy)
                opt.step()
            torch.cuda.synchronize()
            runs.append([c.detach().clone() for c in m.tt_cores])
        assert all(bool(torch.isfinite(c).all()) for c in runs[0])
        assert _same(*runs)
    finally:
        torch.use_deterministic_algorithms(prev)


def test_exact_three_tables(nat, orc):
    from FBTT.tt_embeddings_ops import OptimType, TableBatchedTTEmbeddingBag
    p, q, r = SHAPES[0]
    runs = []
    for _ in range(2):
        torch.manual_seed(4)
        m = TableBatchedTTEmbeddingBag(3, int(np.prod(p)), 100, r, p, q, optimizer=OptimType.EXACT_SGD,
                                       learning_rate=0.1, weight_dist="normal")
        for c in m.tt_cores:
            c.data.mul_(30.0)
        cores0 = [[c.detach()[k].cpu().numpy().copy() for c in m.tt_cores] for k in range(3)]
        rng = np.random.default_rng(6)
        B = 50
        lens = rng.integers(0, 6, size=3 * B)
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        ids = rng.integers(0, int(np.prod(p)), size=int(offs[-1])).astype(np.int64)
        out = m(_dev(ids), _dev(offs))
        for k in range(3):
            o = offs[k * B:(k + 1) * B + 1]
            want = orc.tt_forward(ids[o[0]:o[-1]], o - o[0], cores0[k], p, q, [1] + r + [1])
            np.testing.assert_allclose(out[k].detach().cpu().numpy(), want, atol=1e-4, rtol=1e-5)
        dy = ((rng.random(tuple(out.shape)) - 0.5) * 0.1).astype(np.float32)
        out.backward(_dev(dy))
        torch.cuda.synchronize()
        for k in range(3):   # each table's fused SGD step against the oracle's
            o = offs[k * B:(k + 1) * B + 1]
            g = orc.tt_dense_backward(ids[o[0]:o[-1]], o - o[0], dy[k], cores0[k], p, q, [1] + r + [1])
            for t, want in enumerate(orc.sgd_step(cores0[k], g, 0.1)):
                got = m.tt_cores[t].detach()[k].cpu().numpy()
                assert float(np.abs(got - want).max()) <= 1e-5 + 1e-4 * 0.1 * float(np.abs(g[t]).max()), (k, t)
        runs.append([c.detach().clone() for c in m.tt_cores])
    assert _same(*runs)


def test_exact_captured_lookup_replays_the_exact_kernels(nat):
    n = 409_600   # Zipf ids in ragged bags
    ids, offs, dy = _batch(0, n)
    eager, cap_m = _module(seed=3), _module(seed=3)
    out_e = eager(ids, offs)
    out_e.backward(dy)
    cap = cap_m.capture(n, offs.numel() - 1, offs)
    assert cap.exact
    out_c = cap(ids, offs)
    assert torch.equal(out_e.detach(), out_c.detach())
    out_c.backward(dy)
    torch.cuda.synchronize()
    assert _same([c.detach() for c in eager.tt_cores], [c.detach() for c in cap_m.tt_cores])


def test_exact_does_not_synchronise(nat):
    m = _module(seed=5)
    ids, offs, dy = _batch(1)
    m(ids, offs).backward(dy)   # first call: workspace, size queries
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        m(ids, offs).backward(dy)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()


def test_exact_unsupported_rank(nat, orc):
    p, q, r = [11, 13, 17], [4, 5, 5], [64, 64]
    m = _module(seed=6, shape=(p, q, r), scale=3.0)
    ids = _dev(_ids(int(np.prod(p)), 500, 1))
    offs = _dev(np.arange(501, dtype=np.int64))
    with pytest.raises(RuntimeError, match="exact mode"):
        m(ids, offs)
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            out = m(ids, offs)
        assert any("exact mode" in str(x.message) for x in w)
    finally:
        torch.use_deterministic_algorithms(prev)
    cores = [c.detach()[0].cpu().numpy() for c in m.tt_cores]
    want = orc.tt_forward(ids.cpu().numpy(), offs.cpu().numpy(), cores, p, q, [1] + r + [1])
    np.testing.assert_allclose(out.detach().cpu().numpy(), want, atol=1e-4, rtol=1e-4)
