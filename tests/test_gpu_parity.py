"""GPU parity: the HIP path (through the C ABI, via ttemb_native) against the golden
vectors generated from the reference and against the CPU oracle on seeded inputs.

Tolerances (north-star: forward within 1e-4 in fp32):
  forward      atol 1e-4 (+ rtol 1e-5 for the O(10) magnitudes of the golden cores)
  dense grads  rtol 1e-4 of the gradient's max magnitude (summation order differs)
  fused steps  atol 1e-5 on the updated cores
Integer work (index split, partition, hash) is compared bit-exactly.
"""
import hashlib

import numpy as np
import pytest
import torch

from conftest import RANK_CASES, ROW_CASES, TINY_CASES, golden_cores, load_golden, rank_case_cores, seeded_cores

pytestmark = pytest.mark.gpu

PATHS = ["generic", "auto", "fast3"]
# (q0, q1, q2, r1, r2) of the MFMA path: the BASELINE.json shapes, then the other 3-core shapes of the reference's scripts
FAST3_SHAPES = {(4, 5, 5, 16, 16), (4, 4, 8, 8, 8), (8, 4, 4, 32, 32), (4, 4, 8, 16, 16), (8, 4, 4, 16, 16),
                (4, 5, 5, 32, 32), (4, 4, 8, 32, 32), (5, 4, 5, 16, 16), (5, 5, 4, 16, 16), (5, 5, 4, 32, 32), (5, 5, 4, 8, 8), (4, 5, 5, 8, 8)}


@pytest.fixture(scope="module")
def nat():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import ttemb_native
    return ttemb_native


@pytest.fixture(scope="module")
def orc():
    from oracle import tt_oracle
    return tt_oracle


def dev(x, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(x))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


def set_path(nat, path, q=None, R=None):
    """Select the kernel family; forcing the MFMA path on a shape it does not cover skips the test."""
    if path == "fast3":
        key = (tuple(int(x) for x in q) + tuple(int(x) for x in R[1:-1])) if q is not None and len(q) == 3 else None
        if key not in FAST3_SHAPES:
            pytest.skip("shape outside the fast 3-core path")
    nat.set_path({"auto": nat.PATH_AUTO, "generic": nat.PATH_GENERIC, "fast3": nat.PATH_FAST3}[path])


def run_forward(nat, p, q, R, cores, indices, offsets):
    shape = nat.make_shape(p, q, R)
    ws = nat.Workspace()
    c = [dev(x) for x in cores]
    idx, offs = dev(indices, torch.int64), dev(offsets, torch.int64)
    B, nnz = offs.numel() - 1, idx.numel()
    rowidx = torch.empty(nnz, dtype=torch.int64, device="cuda")
    nat.preprocess(idx, offs, B, True, None, None, None, rowidx, None, None, ws)
    out = torch.full((B, int(np.prod(q))), float("nan"), device="cuda")
    nat.forward(shape, c, idx, rowidx, offs, nnz, None, B, out, ws)
    torch.cuda.synchronize()
    return out.cpu().numpy(), rowidx


def run_backward_dense(nat, p, q, R, cores, indices, offsets, d_output):
    shape = nat.make_shape(p, q, R)
    ws = nat.Workspace()
    c = [dev(x) for x in cores]
    idx, offs = dev(indices, torch.int64), dev(offsets, torch.int64)
    B, nnz = offs.numel() - 1, idx.numel()
    rowidx = torch.empty(nnz, dtype=torch.int64, device="cuda")
    nat.preprocess(idx, offs, B, True, None, None, None, rowidx, None, None, ws)
    grads = [torch.full_like(x, float("nan")) for x in c]
    nat.backward_dense(shape, c, idx, rowidx, nnz, None, B, dev(d_output), grads, ws)
    torch.cuda.synchronize()
    return [g.cpu().numpy() for g in grads]


def assert_grads_close(got, want, rel=1e-4):
    for t, (a, b) in enumerate(zip(got, want)):
        scale = max(float(np.abs(b).max()), 1e-6)
        err = float(np.abs(a - b).max())
        assert err <= rel * scale + 1e-6, f"core {t}: max err {err:.3e} vs scale {scale:.3e}"


# ---------------------------------------------------------------------------------------
# golden vectors (reference tt_matrix_to_full / autograd)
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", TINY_CASES)
def test_forward_golden(nat, name, path):
    g = load_golden(name)
    set_path(nat, path, g["q"], g["R"])
    out, rowidx = run_forward(nat, g["p"], g["q"], g["R"], golden_cores(g), g["indices"], g["offsets"])
    np.testing.assert_allclose(out, g["out"], rtol=1e-5, atol=1e-4)
    from oracle import tt_oracle
    assert (rowidx.cpu().numpy() == tt_oracle.rowidx_from_offsets(g["offsets"], g["indices"].shape[0])).all()


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", ROW_CASES)
def test_rows_of_baseline_configs(nat, name, path):
    g = load_golden(name)
    set_path(nat, path, g["q"], g["R"])
    cores = seeded_cores(g["p"], g["q"], g["R"], g["seed"], g["core_scale"])
    h = hashlib.sha256()   # (the file carries the SHA-256 of the cores its rows were computed from, as the rank cases do)
    for c in cores:
        h.update(np.ascontiguousarray(c).tobytes())
    assert h.hexdigest() == str(g["cores_sha256"]), "RNG drift: regenerate the golden vectors"
    n = g["indices"].shape[0]
    out, _ = run_forward(nat, g["p"], g["q"], g["R"], cores, g["indices"], np.arange(n + 1))
    np.testing.assert_allclose(out, g["rows"], rtol=1e-5, atol=1e-4)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", TINY_CASES)
def test_backward_dense_golden(nat, name, path):
    g = load_golden(name)
    set_path(nat, path, g["q"], g["R"])
    grads = run_backward_dense(nat, g["p"], g["q"], g["R"], golden_cores(g), g["indices"], g["offsets"],
                               g["d_output"])
    assert_grads_close(grads, [g[f"grad{t}"] for t in range(len(grads))])


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", TINY_CASES)
def test_fused_sgd_and_adagrad_golden(nat, name, path):
    g = load_golden(name)
    set_path(nat, path, g["q"], g["R"])
    p, q, R = g["p"], g["q"], g["R"]
    shape = nat.make_shape(p, q, R)
    ws = nat.Workspace()
    idx, offs = dev(g["indices"], torch.int64), dev(g["offsets"], torch.int64)
    B, nnz = offs.numel() - 1, idx.numel()
    rowidx = torch.empty(nnz, dtype=torch.int64, device="cuda")
    nat.preprocess(idx, offs, B, True, None, None, None, rowidx, None, None, ws)
    d_out = dev(g["d_output"])
    c = [dev(x) for x in golden_cores(g)]
    nat.backward_sgd(shape, c, idx, rowidx, nnz, None, B, d_out, float(g["lr"]), ws)
    for t in range(len(c)):
        np.testing.assert_allclose(c[t].cpu().numpy(), g[f"sgd{t}"], rtol=0, atol=1e-5)
    c = [dev(x) for x in golden_cores(g)]
    st = [torch.zeros_like(x) for x in c]
    nat.backward_adagrad(shape, c, st, idx, rowidx, nnz, None, B, d_out, float(g["lr"]), float(g["eps"]), ws)
    for t in range(len(c)):
        want_state = g[f"ada_state{t}"]
        np.testing.assert_allclose(st[t].cpu().numpy(), want_state, rtol=2e-4,
                                   atol=1e-4 * float(np.abs(want_state).max()))
        # rows the batch never touched have g == 0 exactly -> unchanged; touched entries move by
        # lr * sign(g) on the first step (state == g^2), up to rounding of tiny gradients
        got, want = c[t].cpu().numpy(), g[f"ada{t}"]
        big = np.abs(g[f"grad{t}"]) > 1e-3 * np.abs(g[f"grad{t}"]).max()
        np.testing.assert_allclose(got[big], want[big], rtol=0, atol=1e-5)
        untouched = g[f"grad{t}"] == 0
        assert (got[untouched] == golden_cores(g)[t][untouched]).all()


# ---------------------------------------------------------------------------------------
# seeded random inputs vs the CPU oracle
# ---------------------------------------------------------------------------------------
CONFIGS = {
    "arxiv": ([56, 60, 51], [4, 4, 8], [1, 8, 8, 1], 169343),
    "products": ([125, 140, 140], [4, 5, 5], [1, 16, 16, 1], 2449029),
    "papers": ([500, 560, 400], [8, 4, 4], [1, 32, 32, 1], 111059956),
    "arxiv_r16": ([125, 140, 140], [4, 4, 8], [1, 16, 16, 1], 2449029),   # the run scripts' ogbn-arxiv shape (D = 128, rank 16)
    "two_core": ([300, 400], [8, 8], [1, 12, 1], 120000),
    "four_core": ([20, 25, 30, 10], [2, 4, 4, 2], [1, 6, 10, 4, 1], 150000),
}


def random_case(cfg, n_bags, mean_len, seed, unique=False):
    p, q, R, n_emb = CONFIGS[cfg]
    rng = np.random.default_rng(seed)
    cores = [(rng.standard_normal((p[t], R[t] * q[t] * R[t + 1])) * 0.3).astype(np.float32)
             for t in range(len(p))]
    if mean_len is None:
        lens = np.ones(n_bags, dtype=np.int64)
    else:
        lens = np.clip(np.round(rng.normal(mean_len, mean_len, n_bags)), 0, None).astype(np.int64)
    nnz = int(lens.sum())
    if unique:
        idx = rng.choice(n_emb, size=nnz, replace=False).astype(np.int64)
    else:
        idx = rng.integers(0, n_emb, size=nnz, dtype=np.int64)
        if nnz > 10:  # force duplicates and the two extreme ids
            idx[1] = idx[0]
            idx[2] = 0
            idx[3] = n_emb - 1
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    D = int(np.prod(q))
    d_out = (rng.random((n_bags, D)).astype(np.float32) - 0.5) * 0.2
    return p, q, R, cores, idx, offsets, d_out


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("cfg,n_bags,mean_len", [
    ("arxiv", 256, None), ("products", 2048, None), ("products", 700, 4.0), ("papers", 512, None),
    ("papers", 300, 3.0), ("two_core", 500, 2.0), ("four_core", 500, 2.0), ("products", 1, None),
    ("products", 63, None), ("products", 65, 1.0),
])
def test_forward_backward_vs_oracle(nat, orc, cfg, n_bags, mean_len, path):
    set_path(nat, path, CONFIGS[cfg][1], CONFIGS[cfg][2])
    p, q, R, cores, idx, offsets, d_out = random_case(cfg, n_bags, mean_len, seed=sum(map(ord, cfg)) + n_bags)
    out, _ = run_forward(nat, p, q, R, cores, idx, offsets)
    want = orc.tt_forward(idx, offsets, cores, p, q, R)
    np.testing.assert_allclose(out, want, rtol=1e-5, atol=1e-4)
    grads = run_backward_dense(nat, p, q, R, cores, idx, offsets, d_out)
    assert_grads_close(grads, orc.tt_dense_backward(idx, offsets, d_out, cores, p, q, R))


@pytest.mark.parametrize("path", PATHS)
def test_empty_and_degenerate_inputs(nat, orc, path):
    p, q, R, _ = CONFIGS["products"]
    set_path(nat, path, q, R)
    _, _, _, cores, _, _, _ = random_case("products", 4, None, seed=5)
    # no ids at all: output is all zeros, grads are all zeros
    out, _ = run_forward(nat, p, q, R, cores, np.zeros(0, np.int64), np.zeros(6, np.int64))
    assert out.shape == (5, 100) and (out == 0).all()
    grads = run_backward_dense(nat, p, q, R, cores, np.zeros(0, np.int64), np.zeros(6, np.int64),
                               np.ones((5, 100), np.float32))
    assert all((g == 0).all() for g in grads)
    # one bag holding every id, surrounded by empty bags
    idx = np.array([7, 7, 7, 2449028, 0, 19600], dtype=np.int64)
    offsets = np.array([0, 0, 6, 6], dtype=np.int64)
    out, _ = run_forward(nat, p, q, R, cores, idx, offsets)
    np.testing.assert_allclose(out, orc.tt_forward(idx, offsets, cores, p, q, R), rtol=1e-5, atol=1e-4)
    assert (out[0] == 0).all() and (out[2] == 0).all()


def test_flat_optimizer_steps(nat):
    rng = np.random.default_rng(0)
    for n in (1, 3, 4, 1000, 198400, 198403):
        w = rng.standard_normal(n).astype(np.float32)
        g = rng.standard_normal(n).astype(np.float32)
        s = rng.random(n).astype(np.float32)
        wt, gt = dev(w), dev(g)
        nat.sgd_step(wt, gt, 0.05)
        np.testing.assert_allclose(wt.cpu().numpy(), w - np.float32(0.05) * g, rtol=0, atol=1e-6)
        wt, st = dev(w), dev(s)
        nat.adagrad_step(wt, st, gt, 0.05, 1e-10)
        s2 = s + g * g
        np.testing.assert_allclose(st.cpu().numpy(), s2, rtol=1e-6)
        np.testing.assert_allclose(wt.cpu().numpy(), w - np.float32(0.05) * g / (np.sqrt(s2) + np.float32(1e-10)),
                                   rtol=1e-5, atol=1e-6)


# ---------------------------------------------------------------------------------------
# full-size properties (BASELINE.json sizes; the oracle is too slow / big here)
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,n_ids", [("arxiv", 40000), ("products", 60000), ("papers", 30000)])
def test_fast_path_medium_batches_with_duplicates_and_bags(nat, orc, cfg, n_ids):
    """The grouped MFMA path on batches big enough to have full chunks, several chunks per group,
    duplicate ids and multi-id bags (atomic row accumulation), against the oracle."""
    p, q, R, n_emb = CONFIGS[cfg]
    set_path(nat, "fast3", q, R)
    rng = np.random.default_rng(5 + n_ids)
    cores = [(rng.standard_normal((p[t], R[t] * q[t] * R[t + 1])) * 0.3).astype(np.float32) for t in range(3)]
    # half the ids from 300 dense windows (big groups), half uniform; then duplicates
    starts = rng.integers(0, n_emb - 400, size=300)
    local = (starts[:, None] + rng.integers(0, 400, size=(300, n_ids // 600))).reshape(-1)
    idx = np.concatenate([local, rng.integers(0, n_emb, size=n_ids - local.shape[0])]).astype(np.int64)
    idx[:1000] = idx[1000:2000]
    rng.shuffle(idx)
    lens = rng.integers(0, 4, size=n_ids)
    lens = lens[np.cumsum(lens) <= n_ids]
    idx = idx[: int(lens.sum())]
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    B = offsets.shape[0] - 1
    D = int(np.prod(q))
    out, _ = run_forward(nat, p, q, R, cores, idx, offsets)
    np.testing.assert_allclose(out, orc.tt_forward(idx, offsets, cores, p, q, R), rtol=1e-5, atol=2e-4)
    d_out = ((rng.random((B, D)) - 0.5) * 0.1).astype(np.float32)
    grads = run_backward_dense(nat, p, q, R, cores, idx, offsets, d_out)
    assert_grads_close(grads, orc.tt_dense_backward(idx, offsets, d_out, cores, p, q, R), rel=2e-4)


@pytest.mark.parametrize("p,q,R", [([5, 6, 7], [4, 5, 5], [1, 16, 16, 1]), ([3, 4, 6], [8, 4, 4], [1, 32, 32, 1]),
                                   ([9, 8, 5], [4, 4, 8], [1, 8, 8, 1])])
def test_fast_path_huge_groups_and_bags(nat, orc, p, q, R):
    """Few (i0, i1) groups with ~1000 ids each (tens of chunks per group, groups that span several wavefronts'
    descriptor ranges), one id repeated thousands of times, one bag holding thousands of ids, empty bags."""
    set_path(nat, "fast3", q, R)
    n_emb = int(np.prod(p))
    rng = np.random.default_rng(11 + p[0])
    cores = [(rng.standard_normal((p[t], R[t] * q[t] * R[t + 1])) * 0.3).astype(np.float32) for t in range(3)]
    idx = rng.integers(0, n_emb, size=30000).astype(np.int64)
    idx[5000:9000] = idx[0]                      # 4000 copies of one id
    lens = np.concatenate([[0, 6000, 0, 1], rng.integers(0, 3, size=40000)])
    lens = lens[np.cumsum(lens) <= idx.shape[0]]
    idx = idx[: int(lens.sum())]
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    B, D = offsets.shape[0] - 1, int(np.prod(q))
    out, _ = run_forward(nat, p, q, R, cores, idx, offsets)
    want = orc.tt_forward(idx, offsets, cores, p, q, R)
    np.testing.assert_allclose(out, want, rtol=1e-4, atol=1e-4 * float(np.abs(want).max()))
    d_out = ((rng.random((B, D)) - 0.5) * 0.1).astype(np.float32)
    grads = run_backward_dense(nat, p, q, R, cores, idx, offsets, d_out)
    assert_grads_close(grads, orc.tt_dense_backward(idx, offsets, d_out, cores, p, q, R), rel=2e-4)


@pytest.mark.parametrize("p,q,R,n_ids", [
    ([125, 140, 140], [4, 4, 8], [1, 16, 16, 1], 40000),   # run_ogbn-arxiv scripts: D = 128 at rank 16
    ([40, 30, 50], [8, 4, 4], [1, 16, 16, 1], 30000),
    ([30, 20, 40], [4, 5, 5], [1, 32, 32, 1], 30000),
    ([25, 30, 35], [4, 4, 8], [1, 32, 32, 1], 30000),
    ([7, 300, 900], [4, 4, 8], [1, 16, 16, 1], 20000),      # p2 near the reduce kernel's bucket limit
    ([50, 80, 100], [5, 4, 5], [1, 16, 16, 1], 40000),      # q0 = 5: three groups per MFMA tile in prefix / epilogue
    ([9, 7, 30], [5, 4, 5], [1, 16, 16, 1], 9000),
    ([60, 50, 60], [5, 5, 4], [1, 16, 16, 1], 40000),       # q0 q1 = 25: the E product's last K-step is padded
    ([4, 9, 11], [5, 5, 4], [1, 16, 16, 1], 7000),
])
def test_fast_path_script_shapes(nat, orc, p, q, R, n_ids):
    """The other (q, rank) shapes the reference's run scripts train with, on the grouped MFMA path: uniform ids plus
    dense windows, duplicates, multi-id and empty bags, against the oracle."""
    set_path(nat, "fast3", q, R)
    n_emb = int(np.prod(p))
    rng = np.random.default_rng(17 + p[0] + R[1])
    cores = [(rng.standard_normal((p[t], R[t] * q[t] * R[t + 1])) * 0.3).astype(np.float32) for t in range(3)]
    starts = rng.integers(0, n_emb - 300, size=100)
    local = (starts[:, None] + rng.integers(0, 300, size=(100, n_ids // 200))).reshape(-1)
    idx = np.concatenate([local, rng.integers(0, n_emb, size=n_ids - local.shape[0])]).astype(np.int64)
    idx[:500] = idx[500:1000]
    rng.shuffle(idx)
    lens = rng.integers(0, 4, size=n_ids)
    lens = lens[np.cumsum(lens) <= n_ids]
    idx = idx[: int(lens.sum())]
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    B, D = offsets.shape[0] - 1, int(np.prod(q))
    out, _ = run_forward(nat, p, q, R, cores, idx, offsets)
    want = orc.tt_forward(idx, offsets, cores, p, q, R)
    np.testing.assert_allclose(out, want, rtol=1e-4, atol=1e-4 * max(1.0, float(np.abs(want).max())))
    d_out = ((rng.random((B, D)) - 0.5) * 0.1).astype(np.float32)
    grads = run_backward_dense(nat, p, q, R, cores, idx, offsets, d_out)
    assert_grads_close(grads, orc.tt_dense_backward(idx, offsets, d_out, cores, p, q, R), rel=2e-4)


def _random_bags(rng, n_emb, n_ids):
    """ids with duplicates, bag lengths 0..3 with a long bag and empty bags in between"""
    lens = np.concatenate([[0, 37, 0], rng.integers(0, 4, size=n_ids)])
    lens = lens[np.cumsum(lens) <= n_ids]
    nnz = int(lens.sum())
    idx = rng.integers(0, n_emb, size=nnz).astype(np.int64)
    if nnz > 8:
        idx[: nnz // 8] = idx[nnz // 8: 2 * (nnz // 8)]
        idx[-1], idx[-2] = n_emb - 1, 0
    return idx, np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


@pytest.mark.parametrize("seed", range(12))
def test_random_shapes_generic(nat, orc, seed):
    """Seeded sweep of table shapes the wave-per-id kernels must take: T in {2, 3, 4}, q factors 1..8, ranks 1..24
    (not multiples of 4), p factors down to 1; D a multiple of 4 as the reference requires."""
    rng = np.random.default_rng(1000 + seed)
    T = int(rng.integers(2, 5))
    p = [int(x) for x in rng.integers(1, 40, size=T)]
    q = [int(x) for x in rng.integers(1, 9, size=T)]
    if int(np.prod(q)) % 4:   # embedding_dim must be a multiple of 4, as in the reference (tt_embeddings_cuda.cu:993)
        q[int(rng.integers(0, T))] *= 4
    R = [1] + [int(x) for x in rng.integers(1, 25, size=T - 1)] + [1]
    nat.set_path(nat.PATH_GENERIC)
    cores = [(rng.standard_normal((p[t], R[t] * q[t] * R[t + 1])) * 0.4).astype(np.float32) for t in range(T)]
    idx, offsets = _random_bags(rng, int(np.prod(p)), int(rng.integers(1, 3000)))
    out, _ = run_forward(nat, p, q, R, cores, idx, offsets)
    want = orc.tt_forward(idx, offsets, cores, p, q, R)
    np.testing.assert_allclose(out, want, rtol=1e-4, atol=1e-4 * max(1.0, float(np.abs(want).max())))
    d_out = ((rng.random(want.shape) - 0.5) * 0.2).astype(np.float32)
    grads = run_backward_dense(nat, p, q, R, cores, idx, offsets, d_out)
    assert_grads_close(grads, orc.tt_dense_backward(idx, offsets, d_out, cores, p, q, R), rel=2e-4)


@pytest.mark.parametrize("p,q,r,n_ids", [([300, 500], [8, 16], 16, 30000), ([90, 4000], [10, 10], 16, 20000),
                                         ([7, 33], [16, 8], 16, 9000), ([1000, 60], [10, 10], 16, 50000)])
def test_two_core_tables_on_the_grouped_path(nat, orc, p, q, r, n_ids):
    """2-core tables (FBTT/tt_embeddings_cuda.cu:757-779 are the reference's 2-core forms) lifted onto the 3-core MFMA
    kernels with an identity middle core: q = 8,16 / 10,10 / 16,8 at rank 16, groups = values of i0.  Ragged bags and
    duplicates against the oracle; AUTO and the forced MFMA path give the same kernels from ~4 k ids on."""
    R = [1, r, 1]
    rng = np.random.default_rng(p[0] + q[0])
    cores = [(rng.standard_normal((p[t], R[t] * q[t] * R[t + 1])) * 0.3).astype(np.float32) for t in range(2)]
    idx, offsets = _random_bags(rng, int(np.prod(p)), n_ids)
    want = orc.tt_forward(idx, offsets, cores, p, q, R)
    d_out = ((rng.random(want.shape) - 0.5) * 0.2).astype(np.float32)
    want_g = orc.tt_dense_backward(idx, offsets, d_out, cores, p, q, R)
    for path in (nat.PATH_AUTO, nat.PATH_FAST3):
        nat.set_path(path)
        out, _ = run_forward(nat, p, q, R, cores, idx, offsets)
        np.testing.assert_allclose(out, want, rtol=1e-4, atol=1e-4 * max(1.0, float(np.abs(want).max())))
        grads = run_backward_dense(nat, p, q, R, cores, idx, offsets, d_out)
        assert_grads_close(grads, want_g, rel=2e-4)
    nat.set_path(nat.PATH_AUTO)


@pytest.mark.parametrize("with_rowidx", [False, True])
@pytest.mark.parametrize("name", RANK_CASES)
def test_rank_sweep_golden(nat, name, with_rowidx):
    """The (q, rank) points of the reference's rank sweep (run_script.sh:250-288: q = 5,5,4 at 8 ... 256, q = 4,4,8 at
    64 ... 256) against vectors from the reference's tt_matrix_to_full + autograd, on whatever kernels AUTO picks for the
    shape (ids with and without a row index: the per-bag MFMA kernels take instantiated shapes only in the second form)."""
    g = load_golden(name)
    cores = rank_case_cores(g)
    p, q, R = [int(x) for x in g["p"]], [int(x) for x in g["q"]], [int(x) for x in g["R"]]
    nat.set_path(nat.PATH_AUTO)
    shp, ws = nat.make_shape(p, q, R), nat.Workspace()
    c = [dev(x) for x in cores]
    di, do = dev(g["indices"], torch.int64), dev(g["offsets"], torch.int64)
    B, nnz = do.numel() - 1, di.numel()
    rowidx = None
    if with_rowidx:
        rowidx = torch.empty(nnz, dtype=torch.int64, device="cuda")
        nat.preprocess(di, do, B, True, None, None, None, rowidx, None, None, ws)
    out = torch.full((B, int(np.prod(q))), float("nan"), device="cuda")
    nat.forward(shp, c, di, rowidx, do, nnz, None, B, out, ws)
    np.testing.assert_allclose(out.cpu().numpy(), g["out"], rtol=1e-4, atol=1e-4)
    grads = [torch.full_like(x, float("nan")) for x in c]
    nat.backward_dense(shp, c, di, rowidx, nnz, None, B, dev(g["d_output"]), grads, ws, None, do)
    torch.cuda.synchronize()
    got = [x.cpu().numpy() for x in grads]
    assert_grads_close([got[0], got[2]], [g["grad0"], g["grad2"]], rel=2e-4)
    err = float(np.abs(got[1].reshape(-1)[::61] - g["grad1_every61"]).max())
    assert err <= 2e-4 * float(g["grad1_absmax"]) + 1e-6, f"core 1: {err:.3e}"


@pytest.mark.parametrize("shape", sorted(FAST3_SHAPES))
@pytest.mark.parametrize("n_ids", [1, 700, 3000])
def test_small_batches_on_the_per_bag_mfma_kernels(nat, orc, shape, n_ids):
    """Below the grouped path's crossover AUTO runs every instantiated 3-core shape on the per-bag MFMA kernels (one wavefront
    per bag, no grouping, forward in one launch) when the ids come with their offsets and no row index -- what the module
    passes.  Ragged bags (empty ones, one of 37 ids), duplicates: forward, dense gradients, fused SGD against the oracle."""
    q, R = list(shape[:3]), [1, shape[3], shape[4], 1]
    nat.set_path(nat.PATH_AUTO)
    rng = np.random.default_rng(5 * n_ids + sum(shape))
    p = [int(rng.integers(2, 40)), int(rng.integers(2, 40)), int(rng.integers(2, 200))]
    cores = [(rng.standard_normal((p[t], R[t] * q[t] * R[t + 1])) * 0.3).astype(np.float32) for t in range(3)]
    idx, offsets = _random_bags(rng, int(np.prod(p)), n_ids)
    B, nnz, D = offsets.shape[0] - 1, idx.shape[0], int(np.prod(q))
    shp, ws = nat.make_shape(p, q, R), nat.Workspace()
    c = [dev(x) for x in cores]
    di, do = dev(idx, torch.int64), dev(offsets, torch.int64)
    out = torch.full((B, D), float("nan"), device="cuda")
    nat.forward(shp, c, di, None, do, nnz, None, B, out, ws)
    want = orc.tt_forward(idx, offsets, cores, p, q, R)
    np.testing.assert_allclose(out.cpu().numpy(), want, rtol=1e-4, atol=1e-4 * max(1.0, float(np.abs(want).max())))
    d_out = ((rng.random(want.shape) - 0.5) * 0.2).astype(np.float32)
    grads = [torch.full_like(x, float("nan")) for x in c]
    nat.backward_dense(shp, c, di, None, nnz, None, B, dev(d_out), grads, ws, None, do)
    torch.cuda.synchronize()
    want_g = orc.tt_dense_backward(idx, offsets, d_out, cores, p, q, R)
    assert_grads_close([g.cpu().numpy() for g in grads], want_g, rel=2e-4)
    lr = 0.05
    nat.backward_sgd(shp, c, di, None, nnz, None, B, dev(d_out), lr, ws, None, do)
    torch.cuda.synchronize()
    for t in range(3):
        np.testing.assert_allclose(c[t].cpu().numpy(), cores[t] - np.float32(lr) * want_g[t], rtol=0,
                                   atol=1e-5 + 2e-4 * float(np.abs(lr * want_g[t]).max()))


@pytest.mark.parametrize("q,r", [([5, 5, 4], 256), ([5, 5, 4], 128), ([4, 4, 8], 256), ([4, 5, 5], 8)])
def test_generic_kernels_take_the_rank_sweep_of_the_run_scripts(nat, orc, q, r):
    """run_script.sh:250-288 sweeps --tt-rank up to 256,256 with q = 5,5,4 / 4,4,8: the wave-per-id kernels need up to
    80 KB of LDS per wavefront there (gfx950 has 160 KB per CU; the launch is allowed per kernel).  Forward and dense
    backward against the oracle on a small table."""
    nat.set_path(nat.PATH_GENERIC)
    p, R = [6, 7, 9], [1, r, r, 1]
    rng = np.random.default_rng(r + q[2])
    cores = [(rng.standard_normal((p[t], R[t] * q[t] * R[t + 1])) * (0.3 if t == 0 else 0.3 / np.sqrt(r))).astype(np.float32)
             for t in range(3)]
    idx, offsets = _random_bags(rng, int(np.prod(p)), 600)
    out, _ = run_forward(nat, p, q, R, cores, idx, offsets)
    want = orc.tt_forward(idx, offsets, cores, p, q, R)
    np.testing.assert_allclose(out, want, rtol=1e-4, atol=1e-4 * max(1.0, float(np.abs(want).max())))
    d_out = ((rng.random(want.shape) - 0.5) * 0.2).astype(np.float32)
    grads = run_backward_dense(nat, p, q, R, cores, idx, offsets, d_out)
    assert_grads_close(grads, orc.tt_dense_backward(idx, offsets, d_out, cores, p, q, R), rel=2e-4)


@pytest.mark.parametrize("shape", sorted(FAST3_SHAPES))
@pytest.mark.parametrize("seed", [0, 1])
def test_random_tables_fast_path(nat, orc, shape, seed):
    """Every instantiated (q, ranks) shape of the grouped MFMA path on random table factorisations (p0, p1 from 1 up,
    p2 up to 300) and random bags."""
    q, R = list(shape[:3]), [1, shape[3], shape[4], 1]
    set_path(nat, "fast3", q, R)
    rng = np.random.default_rng(77 * seed + sum(shape))
    p = [int(rng.integers(1, 60)), int(rng.integers(1, 60)), int(rng.integers(1, 300))]
    cores = [(rng.standard_normal((p[t], R[t] * q[t] * R[t + 1])) * 0.3).astype(np.float32) for t in range(3)]
    idx, offsets = _random_bags(rng, int(np.prod(p)), int(rng.integers(500, 20000)))
    out, _ = run_forward(nat, p, q, R, cores, idx, offsets)
    want = orc.tt_forward(idx, offsets, cores, p, q, R)
    np.testing.assert_allclose(out, want, rtol=1e-4, atol=1e-4 * max(1.0, float(np.abs(want).max())))
    d_out = ((rng.random(want.shape) - 0.5) * 0.2).astype(np.float32)
    grads = run_backward_dense(nat, p, q, R, cores, idx, offsets, d_out)
    assert_grads_close(grads, orc.tt_dense_backward(idx, offsets, d_out, cores, p, q, R), rel=2e-4)


# the wide-rank chain (ttemb_wide3.inc): the upper half of the reference's rank sweep on the grouped path
WIDE3_SHAPES = [(5, 5, 4, 64, 64), (5, 5, 4, 128, 128), (5, 5, 4, 256, 256), (4, 4, 8, 64, 64), (4, 4, 8, 128, 128), (4, 4, 8, 256, 256)]


@pytest.fixture(params=["e_table", "lds_slabs"])
def wide_backward_form(request, nat):
    """The two backward forms of the wide-rank chain: an E row per id + the reduce kernel (what a call of a few thousand ids
    takes by the library's rule), and the dG2 reduction inside the chunk kernel (LDS slabs: taken from 8 ids per slab row on --
    forced here with the diagnostic, so that the unit tests' small calls reach wide3_bwd_slab_kernel)."""
    nat.set_wide_slab_min_ids(1 if request.param == "lds_slabs" else 1 << 40)
    yield request.param
    nat.set_wide_slab_min_ids(0)


@pytest.mark.parametrize("shape", WIDE3_SHAPES)
@pytest.mark.parametrize("seed", [0, 1])
def test_random_tables_wide_rank_chain(nat, orc, shape, seed, wide_backward_form):
    """Ranks 64 / 128 / 256 forced onto the grouped path (GEMM prefix, per-chunk forward, per-group backward, E reduce
    by column slices or dG2 slabs in LDS, dG1 / dG0 GEMMs): random table factorisations incl. p0 q0 that is no multiple of 64,
    empty groups, bags of several ids, repeated ids (p2 < 90 with thousands of ids: most chunks hold ids with EQUAL i2 -- the
    slab kernel's tag rounds)."""
    q, R = list(shape[:3]), [1, shape[3], shape[4], 1]
    rng = np.random.default_rng(1234 * seed + sum(shape))
    p = [int(rng.integers(1, 30)), int(rng.integers(1, 12)), int(rng.integers(1, 90))]
    cores = [(rng.standard_normal((p[t], R[t] * q[t] * R[t + 1])) * (0.3 if t != 1 else 0.05)).astype(np.float32) for t in range(3)]
    idx, offsets = _random_bags(rng, int(np.prod(p)), int(rng.integers(300, 4000)))
    nat.set_path(nat.PATH_FAST3)
    try:
        out, _ = run_forward(nat, p, q, R, cores, idx, offsets)
        want = orc.tt_forward(idx, offsets, cores, p, q, R)
        np.testing.assert_allclose(out, want, rtol=1e-4, atol=1e-4 * max(1.0, float(np.abs(want).max())))
        d_out = ((rng.random(want.shape) - 0.5) * 0.2).astype(np.float32)
        grads = run_backward_dense(nat, p, q, R, cores, idx, offsets, d_out)
        assert_grads_close(grads, orc.tt_dense_backward(idx, offsets, d_out, cores, p, q, R), rel=2e-4)
    finally:
        nat.set_path(nat.PATH_AUTO)


@pytest.mark.parametrize("shape", [(5, 5, 4, 64, 64), (4, 4, 8, 128, 128)])
@pytest.mark.parametrize("kind", ["few_groups", "one_i1_full", "windows"])
def test_wide_rank_chain_on_frontiers_that_leave_groups_empty(nat, orc, shape, kind, wide_backward_form):
    """The wide-rank GEMMs walk the non-empty groups only: frontiers that touch a few (i0, i1) groups, that fill every
    group of ONE i1 (that batch takes the plain form, the others the compacted one or nothing), and METIS-like windows of
    consecutive ids; p0 q0 is no multiple of 64 and some values of i1 hold no id at all."""
    q, R = list(shape[:3]), [1, shape[3], shape[4], 1]
    p = [27, 9, 31]
    rng = np.random.default_rng(9 + sum(shape))
    cores = [(rng.standard_normal((p[t], R[t] * q[t] * R[t + 1])) * (0.3 if t != 1 else 0.05)).astype(np.float32) for t in range(3)]
    n_emb, per_i0 = int(np.prod(p)), p[1] * p[2]
    if kind == "few_groups":       # 11 groups out of 243, several ids each, some ids repeated
        groups = rng.choice(p[0] * p[1], size=11, replace=False)
        idx = (groups[rng.integers(0, 11, size=900)] // p[1]) * per_i0 + (groups[rng.integers(0, 11, size=900)] % p[1]) * p[2]
        idx = idx + rng.integers(0, p[2], size=900)
    elif kind == "one_i1_full":    # every i0 of i1 = 4 (a full batch), plus a handful of ids elsewhere
        i0 = np.repeat(np.arange(p[0]), 12)
        idx = np.concatenate([i0 * per_i0 + 4 * p[2] + rng.integers(0, p[2], size=i0.size), rng.integers(0, n_emb, size=40)])
    else:                          # windows of consecutive ids
        starts = rng.choice(n_emb - 64, size=20, replace=False)
        idx = (starts[:, None] + np.arange(48)[None, :]).reshape(-1)
    idx = idx.astype(np.int64)
    offsets = np.arange(idx.size + 1, dtype=np.int64)
    nat.set_path(nat.PATH_FAST3)
    try:
        out, _ = run_forward(nat, p, q, R, cores, idx, offsets)
        want = orc.tt_forward(idx, offsets, cores, p, q, R)
        np.testing.assert_allclose(out, want, rtol=1e-4, atol=1e-4 * max(1.0, float(np.abs(want).max())))
        d_out = ((rng.random(want.shape) - 0.5) * 0.2).astype(np.float32)
        grads = run_backward_dense(nat, p, q, R, cores, idx, offsets, d_out)
        assert_grads_close(grads, orc.tt_dense_backward(idx, offsets, d_out, cores, p, q, R), rel=2e-4)
    finally:
        nat.set_path(nat.PATH_AUTO)


@pytest.mark.parametrize("shape", [(5, 5, 4, 128, 128), (4, 4, 8, 256, 256)])
def test_wide_rank_gemms_keep_fp32_accuracy(nat, shape, wide_backward_form):
    """The GEMMs of the wide-rank chain carry their fp32 products on the bf16 matrix pipe (operands split into three
    bf16 planes, eight of nine partial products, ttemb_wide3.inc).  Against a float64 restatement the forward and the
    dense gradients must be as close as fp32 arithmetic is -- a few 1e-7 of the largest value, where a two-plane split
    would sit at 1e-5 and plain bf16 at 1e-3."""
    q, R = list(shape[:3]), [1, shape[3], shape[4], 1]
    rng = np.random.default_rng(4242 + sum(shape))
    p = [13, 5, 40]
    cores = [(rng.standard_normal((p[t], R[t] * q[t] * R[t + 1])) * (0.3 if t != 1 else 0.05)).astype(np.float32) for t in range(3)]
    n = int(np.prod(p))
    idx = rng.integers(0, n, size=3000).astype(np.int64)
    offsets = np.arange(idx.size + 1, dtype=np.int64)
    c64 = [c.astype(np.float64) for c in cores]
    i0, i1, i2 = idx // (p[1] * p[2]), (idx // p[2]) % p[1], idx % p[2]
    a = c64[0][i0].reshape(-1, q[0], R[1])
    b = c64[1][i1].reshape(-1, R[1], q[1], R[2])
    c = c64[2][i2].reshape(-1, R[2], q[2])
    pre = np.einsum("nar,nrbs->nabs", a, b)
    want = np.einsum("nabs,nsc->nabc", pre, c).reshape(idx.size, -1)
    nat.set_path(nat.PATH_FAST3)
    try:
        out, _ = run_forward(nat, p, q, R, cores, idx, offsets)
        err = float(np.abs(out.astype(np.float64) - want).max()) / float(np.abs(want).max())
        assert err < 2e-6, err
        d_out = ((rng.random(want.shape) - 0.5) * 0.2).astype(np.float32)
        grads = run_backward_dense(nat, p, q, R, cores, idx, offsets, d_out)
        d64 = d_out.astype(np.float64).reshape(idx.size, q[0], q[1], q[2])
        g2 = np.zeros_like(c64[2])
        np.add.at(g2, i2, np.einsum("nabs,nabc->nsc", pre, d64).reshape(idx.size, -1))
        dpre = np.einsum("nabc,nsc->nabs", d64, c)
        g1 = np.zeros_like(c64[1])
        np.add.at(g1, i1, np.einsum("nar,nabs->nrbs", a, dpre).reshape(idx.size, -1))
        g0 = np.zeros_like(c64[0])
        np.add.at(g0, i0, np.einsum("nabs,nrbs->nar", dpre, b).reshape(idx.size, -1))
        for got, ref in zip(grads, (g0, g1, g2)):
            e = float(np.abs(got.astype(np.float64) - ref).max()) / float(np.abs(ref).max())
            assert e < 5e-6, e
    finally:
        nat.set_path(nat.PATH_AUTO)


@pytest.mark.parametrize("name", [n for n in RANK_CASES if any(f"r{r}" in n for r in (64, 128, 256))])
def test_rank_sweep_golden_on_the_wide_rank_chain(nat, name, wide_backward_form):
    """The rank 64 / 128 / 256 points of the reference's rank sweep, forced onto the grouped wide-rank chain, against the
    vectors from the reference's tt_matrix_to_full + autograd."""
    g = load_golden(name)
    cores = rank_case_cores(g)
    p, q, R = [int(x) for x in g["p"]], [int(x) for x in g["q"]], [int(x) for x in g["R"]]
    nat.set_path(nat.PATH_FAST3)
    try:
        shp, ws = nat.make_shape(p, q, R), nat.Workspace()
        c = [dev(x) for x in cores]
        di, do = dev(g["indices"], torch.int64), dev(g["offsets"], torch.int64)
        B, nnz = do.numel() - 1, di.numel()
        out = torch.full((B, int(np.prod(q))), float("nan"), device="cuda")
        nat.forward(shp, c, di, None, do, nnz, None, B, out, ws)
        np.testing.assert_allclose(out.cpu().numpy(), g["out"], rtol=1e-4, atol=1e-4)
        grads = [torch.full_like(x, float("nan")) for x in c]
        nat.backward_dense(shp, c, di, None, nnz, None, B, dev(g["d_output"]), grads, ws, None, do)
        torch.cuda.synchronize()
        got = [x.cpu().numpy() for x in grads]
        assert_grads_close([got[0], got[2]], [g["grad0"], g["grad2"]], rel=2e-4)
        err = float(np.abs(got[1].reshape(-1)[::61] - g["grad1_every61"]).max())
        assert err <= 2e-4 * float(g["grad1_absmax"]) + 1e-6, f"core 1: {err:.3e}"
    finally:
        nat.set_path(nat.PATH_AUTO)


@pytest.mark.parametrize("p,q,R,n_ids,path", [
    ([10, 12, 30, 40], [2, 4, 4, 4], [1, 16, 16, 16, 1], 30000, "fast3"),   # run scripts: q = 2,4,4,4 -> (8, 4, 4) at rank 16
    ([50, 60, 60, 60], [2, 4, 4, 4], [1, 16, 16, 16, 1], 60000, "auto"),    # the scripts' own table (10.8 M rows)
    ([9, 7, 20, 30], [2, 2, 5, 5], [1, 8, 16, 16, 1], 20000, "fast3"),      # (4, 5, 5) at rank 16, r1 = 8
    ([6, 5, 25, 33], [4, 2, 4, 4], [1, 16, 16, 16, 1], 9000, "fast3"),
    ([12, 9, 14, 11], [5, 5, 2, 2], [1, 16, 16, 16, 1], 30000, "fast3"),    # q0 q1 = 25: the LAST two cores merge -> (5, 5, 4)
    ([50, 60, 60, 60], [5, 5, 2, 2], [1, 16, 16, 16, 1], 50000, "auto"),    # the scripts' own products 4-core table
    ([7, 8, 9, 13], [5, 5, 2, 2], [1, 16, 16, 8, 1], 8000, "fast3"),        # r3 = 8 inside the merged pair
    ([6, 7, 9, 5], [4, 4, 8, 1], [1, 16, 16, 4, 1], 9000, "fast3"),         # last pair, 128 rows in the merged operand
])
def test_four_core_tables_on_the_grouped_path(nat, orc, p, q, R, n_ids, path):
    """4-core tables whose first two cores merge into a virtual first core of a covered 3-core shape: the grouped
    kernels on (G0.G1, G2, G3), the gradient of the virtual core split back onto G0 and G1.  Against the oracle's
    4-core forward / backward (dense and fused SGD), windows + duplicates + ragged bags."""
    nat.set_path({"auto": nat.PATH_AUTO, "fast3": nat.PATH_FAST3}[path])
    n_emb = int(np.prod(p))
    rng = np.random.default_rng(5 + p[0] + n_ids)
    cores = [(rng.standard_normal((p[t], R[t] * q[t] * R[t + 1])) * 0.35).astype(np.float32) for t in range(4)]
    starts = rng.integers(0, n_emb - 300, size=60)
    local = (starts[:, None] + rng.integers(0, 300, size=(60, n_ids // 120))).reshape(-1)
    idx = np.concatenate([local, rng.integers(0, n_emb, size=n_ids - local.shape[0])]).astype(np.int64)
    idx[:300] = idx[300:600]
    rng.shuffle(idx)
    lens = rng.integers(0, 4, size=n_ids)
    lens = lens[np.cumsum(lens) <= n_ids]
    idx = idx[: int(lens.sum())]
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    B, D = offsets.shape[0] - 1, int(np.prod(q))
    shape = nat.make_shape(p, q, R)
    assert nat.plan_bytes(shape, idx.shape[0]) > 0, "the 4-core table did not map onto the grouped path"
    out, _ = run_forward(nat, p, q, R, cores, idx, offsets)
    want = orc.tt_forward(idx, offsets, cores, p, q, R)
    np.testing.assert_allclose(out, want, rtol=1e-4, atol=1e-4 * max(1.0, float(np.abs(want).max())))
    d_out = ((rng.random((B, D)) - 0.5) * 0.1).astype(np.float32)
    grads = run_backward_dense(nat, p, q, R, cores, idx, offsets, d_out)
    wg = orc.tt_dense_backward(idx, offsets, d_out, cores, p, q, R)
    assert_grads_close(grads, wg, rel=3e-4)
    # fused SGD through the same mapping (gradients into scratch, one step kernel over the four real cores)
    c = [dev(x) for x in cores]
    ws = nat.Workspace()
    ti, to = dev(idx, torch.int64), dev(offsets, torch.int64)
    nat.backward_sgd(shape, c, ti, None, idx.shape[0], None, B, dev(d_out), 0.05, ws, None, to)
    torch.cuda.synchronize()
    for t in range(4):
        scale = max(float(np.abs(wg[t]).max()), 1e-6)
        np.testing.assert_allclose(c[t].cpu().numpy(), cores[t] - np.float32(0.05) * wg[t], rtol=0, atol=0.05 * 3e-4 * scale + 2e-6)


@pytest.mark.parametrize("cfg,N", [("products", 409600), ("arxiv", 169343), ("papers", 819200), ("arxiv_r16", 169343)])
def test_full_size_properties(nat, orc, cfg, N):
    """BASELINE.json sizes (products: the frontier of a 2048-seed batch; arxiv: every node, the full-graph pattern of
    gcn_gat_partition.py; papers: ids beyond 2^24) through size-independent properties."""
    set_path(nat, "auto")
    p, q, R, n_emb = CONFIGS[cfg]
    D = int(np.prod(q))
    rng = np.random.default_rng(77)
    cores = [(rng.standard_normal((p[t], R[t] * q[t] * R[t + 1])) * (0.3 if cfg != "papers" else 0.15)).astype(np.float32)
             for t in range(3)]
    idx = (np.arange(N) if N == n_emb else rng.choice(n_emb, size=N, replace=False)).astype(np.int64)
    if N == n_emb:
        rng.shuffle(idx)
    out, _ = run_forward(nat, p, q, R, cores, idx, np.arange(N + 1))
    # spot rows against the oracle
    pick = rng.choice(N, size=512, replace=False)
    want = orc.tt_rows(idx[pick], cores, p, q, R)
    np.testing.assert_allclose(out[pick], want, rtol=1e-5, atol=1e-4 * max(1.0, float(np.abs(want).max())))
    # permutation equivariance: looking ids up in another order permutes the rows, bit for bit
    perm = rng.permutation(N)
    out_p, _ = run_forward(nat, p, q, R, cores, idx[perm], np.arange(N + 1))
    assert np.array_equal(out_p, out[perm])
    # bag additivity: bags of 4 equal the sum of the 4 single rows
    n4 = N // 4 * 4
    out4, _ = run_forward(nat, p, q, R, cores, idx[:n4], np.arange(0, n4 + 1, 4))
    ref4 = out[:n4].reshape(-1, 4, D).sum(1)
    np.testing.assert_allclose(out4, ref4, rtol=1e-5, atol=2e-4 * max(1.0, float(np.abs(ref4).max())))
    # backward: linear in d_output, and consistent with a directional derivative of the forward
    d1 = ((rng.random((N, D)) - 0.5) * 0.1).astype(np.float32)
    d2 = ((rng.random((N, D)) - 0.5) * 0.1).astype(np.float32)
    g1 = run_backward_dense(nat, p, q, R, cores, idx, np.arange(N + 1), d1)
    g2 = run_backward_dense(nat, p, q, R, cores, idx, np.arange(N + 1), d2)
    g12 = run_backward_dense(nat, p, q, R, cores, idx, np.arange(N + 1), d1 + d2)
    assert_grads_close(g12, [a + b for a, b in zip(g1, g2)], rel=2e-4)
    eps = 3e-3
    direction = [rng.standard_normal(c.shape).astype(np.float32) for c in cores]
    plus, _ = run_forward(nat, p, q, R, [c + eps * d for c, d in zip(cores, direction)], idx, np.arange(N + 1))
    minus, _ = run_forward(nat, p, q, R, [c - eps * d for c, d in zip(cores, direction)], idx, np.arange(N + 1))
    fd = float(((plus.astype(np.float64) - minus) * d1).sum() / (2 * eps))
    an = float(sum((g.astype(np.float64) * d).sum() for g, d in zip(g1, direction)))
    assert abs(fd - an) <= 2e-3 * max(abs(an), 1.0), (fd, an)


@pytest.mark.parametrize("live,wide", [(0, False), (1, False), (7000, False), (0, True), (1, True), (2500, True)])
def test_fast_path_with_a_device_side_live_count(nat, orc, live, wide):
    """The launch is sized by nnz, the kernels use the device-side count (what ttemb_preprocess leaves behind): only
    the first `live` ids exist.  0 and 1 are the degenerate ends (no chunk at all / one chunk of one id); rows are
    derived from `offsets` (rowidx NULL) and the two-phase forward (group, then lookup) must give the same.  `wide`: the
    same on the wide-rank chain (q = 5,5,4 at rank 64 on a small table)."""
    p, q, R, n_emb = CONFIGS["products"]
    if wide:
        p, q, R = [23, 12, 40], [5, 5, 4], [1, 64, 64, 1]
        n_emb = int(np.prod(p))
        nat.set_path(nat.PATH_FAST3)
    else:
        set_path(nat, "fast3", q, R)
    rng = np.random.default_rng(3 + live)
    cores = [(rng.standard_normal((p[t], R[t] * q[t] * R[t + 1])) * (0.05 if wide and t == 1 else 0.3)).astype(np.float32) for t in range(3)]
    N = 3000 if wide else 9000
    idx = rng.integers(0, n_emb, size=N).astype(np.int64)
    offsets = np.arange(N + 1, dtype=np.int64)
    shape = nat.make_shape(p, q, R)
    ws = nat.Workspace()
    c = [dev(x) for x in cores]
    d_idx, d_offs = dev(idx, torch.int64), dev(offsets, torch.int64)
    cnt = torch.tensor([live], dtype=torch.int32, device="cuda")
    want = np.zeros((N, 100), dtype=np.float32)
    want[:live] = orc.tt_rows(idx[:live], cores, p, q, R) if live else 0.0
    outs = []
    for two_phase in (False, True):
        out = torch.full((N, 100), float("nan"), device="cuda")
        plan = nat.new_plan(shape, N, out.device)
        if two_phase:
            nat.forward(shape, c, d_idx, None, d_offs, N, cnt, N, out, ws, plan, phase=1)
            nat.forward(shape, c, d_idx, None, d_offs, N, cnt, N, out, ws, plan, phase=2)
        else:
            nat.forward(shape, c, d_idx, None, d_offs, N, cnt, N, out, ws, plan)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        # bags of one id are written by exactly one writer: this call for live ids, ttemb_cache_forward for the rest
        np.testing.assert_allclose(got[:live], want[:live], rtol=1e-5, atol=1e-4)
        outs.append(got[:live])
        d_out = ((rng.random((N, 100)) - 0.5) * 0.1).astype(np.float32)
        grads = [torch.full_like(x, float("nan")) for x in c]
        nat.backward_dense(shape, c, d_idx, None, N, cnt, N, dev(d_out), grads, ws, plan, d_offs)
        torch.cuda.synchronize()
        ref = orc.tt_dense_backward(idx[:live], np.arange(live + 1), d_out[:live], cores, p, q, R)
        assert_grads_close([g.cpu().numpy() for g in grads], ref, rel=2e-4)
    # the whole forward of a sparse-group frontier forms its prefix products inside the chain kernel (with a permuted K order),
    # the two-phase forward in a launch of their own: the same rows up to the order of the fp32 sums
    np.testing.assert_allclose(outs[0], outs[1], rtol=2e-6, atol=2e-6)


# ---------------------------------------------------------------------------------------
# run-time (q, ranks): every 3-core shape without an instantiated template runs the per-bag MFMA kernels of
# ttemb_rt3.inc (2- / 4-core tables through their 3-core view), not the wave-per-id scalar kernels
# ---------------------------------------------------------------------------------------
RT_SHAPES = [
    ([30, 35, 40], [4, 5, 5], [12, 12]),       # the products factorisation at a rank between the instantiated ones
    ([30, 35, 40], [4, 5, 5], [24, 24]),
    ([20, 25, 30], [4, 5, 5], [48, 48]),
    ([30, 35, 40], [2, 5, 10], [16, 16]),      # q shapes no template has
    ([30, 35, 40], [3, 4, 8], [16, 24]),
    ([20, 20, 20], [4, 5, 5], [6, 7]),         # ranks that are not multiples of the MFMA K
    ([12, 15, 10, 11], [2, 4, 4, 4], [12, 12, 12]),   # 4 cores: (G0.G1, G2, G3), merged q = 8,4,4 at rank 12
    ([90, 120], [8, 16], [12]),                # 2 cores lifted onto three with the identity in the middle
    ([25, 30, 35], [4, 16, 2], [8, 8]),        # q0 q1 = 64: four row tiles of P
]


def _run_ids_offsets(nat, p, q, R, cores, indices, offsets, d_output):
    """forward + dense backward the way the module calls them: ids + offsets, no row index"""
    shape = nat.make_shape(p, q, R)
    ws = nat.Workspace()
    c = [dev(x) for x in cores]
    idx, offs = dev(indices, torch.int64), dev(offsets, torch.int64)
    B, nnz = offs.numel() - 1, idx.numel()
    out = torch.full((B, int(np.prod(q))), float("nan"), device="cuda")
    nat.forward(shape, c, idx, None, offs, nnz, None, B, out, ws)
    grads = [torch.full_like(x, float("nan")) for x in c]
    nat.backward_dense(shape, c, idx, None, nnz, None, B, dev(d_output), grads, ws, None, offs)
    torch.cuda.synchronize()
    return out.cpu().numpy(), [g.cpu().numpy() for g in grads]


@pytest.mark.parametrize("n_ids", [700, 20000])
@pytest.mark.parametrize("p,q,r", RT_SHAPES)
def test_shapes_off_the_instantiated_list(nat, orc, p, q, r, n_ids):
    """Shapes without a template -- ranks 12 / 24 / 48, q = 2,5,10 / 3,4,8, ranks that are not multiples of 4, a 4-core and
    a 2-core table off the listed shapes -- run the run-time-shape per-bag MFMA kernels at every batch size (the kernel
    family is asked from the library, not assumed) and match the oracle; ragged bags, duplicates, empty bags."""
    T = len(p)
    R = [1] + list(r) + [1]
    shape = nat.make_shape(p, q, R)
    rng = np.random.default_rng(sum(p) + sum(q) + sum(r) + n_ids)
    idx, offsets = _random_bags(rng, int(np.prod(p)), n_ids)
    fam = nat.kernel_family(shape, int(idx.shape[0]), int(offsets.shape[0] - 1), True) & ~nat.FAMILY_ROUTE_FLAGS
    # past the grouped crossover a 3-core table whose q shape is instantiated at a higher rank rides on the grouped kernels
    # through zero-padded cores (4,5,5 at 12 -> 16, 24 -> 32, (6, 7) -> 8); everything else runs the run-time-shape kernels
    padded = T == 3 and tuple(q) == (4, 5, 5) and max(r) <= 32 and idx.shape[0] >= 4096
    if padded:
        assert fam == nat.FAMILY_GROUPED | nat.FAMILY_PADDED, f"kernel family {fam}"
    else:
        assert fam & ~nat.FAMILY_MERGED == nat.FAMILY_PER_BAG_RT, f"kernel family {fam}"
        assert bool(fam & nat.FAMILY_MERGED) == (T != 3)
    assert nat.kernel_family(shape, int(idx.shape[0]), int(offsets.shape[0] - 1), False) & ~nat.FAMILY_ROUTE_FLAGS in (
        nat.FAMILY_SCALAR, nat.FAMILY_GROUPED | nat.FAMILY_PADDED)   # (a row index, no offsets: no per-bag kernels)
    cores = [(rng.standard_normal((p[t], R[t] * q[t] * R[t + 1])) * 0.4).astype(np.float32) for t in range(T)]
    want = orc.tt_forward(idx, offsets, cores, p, q, R)
    d_out = ((rng.random(want.shape) - 0.5) * 0.2).astype(np.float32)
    out, grads = _run_ids_offsets(nat, p, q, R, cores, idx, offsets, d_out)
    np.testing.assert_allclose(out, want, rtol=1e-4, atol=1e-4 * max(1.0, float(np.abs(want).max())))
    assert_grads_close(grads, orc.tt_dense_backward(idx, offsets, d_out, cores, p, q, R), rel=2e-4)
    # the scalar kernels (forced) agree: same rows, same gradients
    nat.set_path(nat.PATH_GENERIC)
    assert nat.kernel_family(shape, int(idx.shape[0]), int(offsets.shape[0] - 1), True) == nat.FAMILY_SCALAR
    out_s, grads_s = _run_ids_offsets(nat, p, q, R, cores, idx, offsets, d_out)
    nat.set_path(nat.PATH_AUTO)
    np.testing.assert_allclose(out, out_s, rtol=1e-4, atol=1e-4 * max(1.0, float(np.abs(want).max())))
    assert_grads_close(grads, grads_s, rel=2e-4)


def test_runtime_shape_module_trains(orc):
    """The drop-in class on a rank-12 table (fused SGD in backward) against the oracle's closed form."""
    import FBTT.tt_embeddings_ops as ops
    torch.manual_seed(3)
    p, q, r = [30, 35, 40], [4, 5, 5], [12, 12]
    n, lr = int(np.prod(p)), 0.1
    emb = ops.TTEmbeddingBag(n, 100, r, p, q, sparse=True, use_cache=False, weight_dist="normal", learning_rate=lr)
    for c in emb.tt_cores:
        c.data.mul_(60.0)
    cores = [c.detach()[0].cpu().numpy().copy() for c in emb.tt_cores]
    rng = np.random.default_rng(3)
    ids = rng.integers(0, n, size=5000).astype(np.int64)
    offs = np.arange(5001, dtype=np.int64)
    out = emb(torch.tensor(ids).cuda(), torch.tensor(offs).cuda())
    R = [1] + r + [1]
    np.testing.assert_allclose(out.detach().cpu().numpy(), orc.tt_forward(ids, offs, cores, p, q, R), rtol=1e-4, atol=1e-4)
    d_out = ((rng.random((5000, 100)) - 0.5) * 0.1).astype(np.float32)
    out.backward(torch.tensor(d_out).cuda())
    g = orc.tt_dense_backward(ids, offs, d_out, cores, p, q, R)
    for c, c0, gr in zip(emb.tt_cores, cores, g):
        np.testing.assert_allclose(c.detach()[0].cpu().numpy(), c0 - np.float32(lr) * gr, rtol=0,
                                   atol=1e-5 + 2e-4 * float(np.abs(lr * gr).max()))


# ---------------------------------------------------------------------------------------
# calls past one 32-bit row window: the grouped path in pieces (reference: batch_count chunks, tt_embeddings_cuda.cu:1011-1027)
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,ids", [(900, 0), (0, 700), (1500, 1100), (64, 4000)])
@pytest.mark.parametrize("q,r", [([4, 5, 5], [16, 16]), ([8, 4, 4], [32, 32]), ([5, 5, 4], [64, 64])])
def test_small_call_cut_into_pieces(nat, orc, q, r, rows, ids):
    """The piece machinery on a small ragged call, cut by the diagnostic limits: by rows, by ids, by both, and with a row
    window so small that runs of empty bags and multi-id bags straddle the cuts.  Forward rows, dense gradient, fused SGD
    against the oracle; same results as the uncut call.  Fused dG2 (rank 16), E table (rank 32) and wide-rank (64) chains."""
    p = [30, 35, 40]
    R = [1] + r + [1]
    D = int(np.prod(q))
    rng = np.random.default_rng(rows + ids + r[0])
    # ragged bags with long runs of empty bags and a few long bags
    lens = rng.integers(0, 3, size=9000)
    lens[rng.integers(0, 9000, size=40)] = 25
    lens[2000:2300] = 0
    lens[5000:5100] = 0
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    nnz = int(offsets[-1])
    idx = rng.integers(0, int(np.prod(p)), size=nnz).astype(np.int64)
    idx[: nnz // 8] = idx[nnz // 8: 2 * (nnz // 8)]
    cores = [(rng.standard_normal((p[t], R[t] * q[t] * R[t + 1])) * 0.3).astype(np.float32) for t in range(3)]
    want = orc.tt_forward(idx, offsets, cores, p, q, R)
    d_out = ((rng.random(want.shape) - 0.5) * 0.2).astype(np.float32)
    want_g = orc.tt_dense_backward(idx, offsets, d_out, cores, p, q, R)
    nat.set_path(nat.PATH_FAST3)
    shape = nat.make_shape(p, q, R)
    assert nat.plan_bytes(shape, nnz) > 0
    nat.set_piece_limits(rows, ids)
    if ids:
        assert nat.plan_bytes(shape, nnz) == 0   # a call in pieces keeps no plan
    out, grads = _run_ids_offsets(nat, p, q, R, cores, idx, offsets, d_out)
    np.testing.assert_allclose(out, want, rtol=1e-4, atol=1e-4 * max(1.0, float(np.abs(want).max())))
    assert_grads_close(grads, want_g, rel=2e-4)
    if r[0] >= 64:   # the wide chain's other backward form (dG2 slabs in LDS, no E table), piece by piece
        nat.set_wide_slab_min_ids(1)
        try:
            _, grads = _run_ids_offsets(nat, p, q, R, cores, idx, offsets, d_out)
        finally:
            nat.set_wide_slab_min_ids(0)
        assert_grads_close(grads, want_g, rel=2e-4)
    # fused SGD through the C ABI: summed gradient, one step
    ws = nat.Workspace()
    c = [dev(x) for x in cores]
    t_idx, t_offs = dev(idx, torch.int64), dev(offsets, torch.int64)
    nat.backward_sgd(shape, c, t_idx, None, nnz, None, offsets.shape[0] - 1, dev(d_out), 0.05, ws, None, t_offs)
    torch.cuda.synchronize()
    for t in range(3):
        np.testing.assert_allclose(c[t].cpu().numpy(), cores[t] - np.float32(0.05) * want_g[t], rtol=0,
                                   atol=1e-5 + 2e-4 * float(np.abs(0.05 * want_g[t]).max()))
    nat.set_piece_limits(0, 0)
    nat.set_path(nat.PATH_AUTO)


def test_call_past_2_24_rows_stays_on_the_grouped_path(nat, orc):
    """B = 2^24 + 4096 bags of one id on the arxiv shape (an 8.6 GB output: past 2^24 rows AND past 2 GiB): the call runs
    on the grouped kernels in pieces.  Spot rows against the oracle (first / last rows, rows around the cuts), the
    permutation property on the whole tensor, and the dense gradient of a sparse d_output against the oracle's."""
    p, q, r, n_emb = [56, 60, 51], [4, 4, 8], [8, 8], 169343
    R, D = [1] + r + [1], 128
    B = (1 << 24) + 4096
    shape = nat.make_shape(p, q, R)
    assert nat.kernel_family(shape, B, B, True) & ~nat.FAMILY_ROUTE_FLAGS == nat.FAMILY_GROUPED
    assert nat.kernel_family(shape, B, B, False) != nat.FAMILY_GROUPED   # (no bag boundaries: no pieces)
    assert nat.plan_bytes(shape, B) == 0
    rng = np.random.default_rng(24)
    cores = [(rng.standard_normal((p[t], R[t] * q[t] * R[t + 1])) * 0.3).astype(np.float32) for t in range(3)]
    c = [dev(x) for x in cores]
    g = torch.Generator(device="cuda").manual_seed(24)
    idx = torch.randint(0, n_emb, (B,), generator=g, device="cuda", dtype=torch.int64)
    offs = torch.arange(B + 1, dtype=torch.int64, device="cuda")
    ws = nat.Workspace()
    out = torch.empty((B, D), device="cuda")
    out.fill_(float("nan"))
    nat.forward(shape, c, idx, None, offs, B, None, B, out, ws)
    torch.cuda.synchronize()
    rows_per_piece = (2 ** 31 - 1) // (4 * D)   # 4 194 303: the 2 GiB window decides at D = 128
    spots = np.unique(np.concatenate([np.arange(64), np.arange(B - 64, B), rng.integers(0, B, size=3000)] +
                                     [np.arange(k * rows_per_piece - 40, k * rows_per_piece + 40) for k in range(1, 5)] +
                                     [np.arange((1 << 24) - 40, (1 << 24) + 40)]))
    spots = spots[(spots >= 0) & (spots < B)]
    t_sp = torch.tensor(spots, device="cuda")
    got = out[t_sp].cpu().numpy()
    want = orc.tt_rows(idx[t_sp].cpu().numpy(), cores, p, q, R)
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-4)
    assert not bool(torch.isnan(out[::997]).any())
    # permutation property: looking the ids up in another order permutes the rows (checked on every row, block by block)
    perm = torch.randperm(B, generator=g, device="cuda")
    out2 = torch.empty_like(out)
    nat.forward(shape, c, idx[perm].contiguous(), None, offs, B, None, B, out2, ws)
    torch.cuda.synchronize()
    for b0 in range(0, B, 1 << 22):
        sl = slice(b0, min(B, b0 + (1 << 22)))
        assert torch.equal(out2[sl], out[perm[sl]])
    del out2
    # dense backward of a d_output with 40 000 non-zero rows (the other rows contribute exact zeros): the oracle's gradient
    # of those rows alone is the whole gradient
    hot = np.unique(np.concatenate([rng.integers(0, B, size=40000), spots[:200]]))
    d_out = out   # reuse the 8.6 GB buffer
    d_out.zero_()
    vals = ((rng.random((hot.shape[0], D)) - 0.5) * 0.2).astype(np.float32)
    d_out[torch.tensor(hot, device="cuda")] = torch.tensor(vals, device="cuda")
    grads = [torch.full_like(x, float("nan")) for x in c]
    nat.backward_dense(shape, c, idx, None, B, None, B, d_out, grads, ws, None, offs)
    torch.cuda.synchronize()
    hot_ids = idx[torch.tensor(hot, device="cuda")].cpu().numpy()
    want_g = orc.tt_dense_backward(hot_ids, np.arange(hot.shape[0] + 1, dtype=np.int64), vals, cores, p, q, R)
    assert_grads_close([x.cpu().numpy() for x in grads], want_g, rel=2e-4)


def test_fused_backward_at_the_full_409600_ids_against_the_oracle(nat, orc):
    """BASELINE.json configs[1] at its full size -- 409 600 unique uniform ids on the products table, bag length 1 -- through
    the fused chunk kernel: the dense gradient against the oracle's, which takes the batch in eight sub-batches and sums
    (a gradient is additive over ids), and the fused SGD step against the closed form on the same sum."""
    p, q, R, n_emb = CONFIGS["products"]
    n = 409600
    rng = np.random.default_rng(409600)
    cores = [(rng.standard_normal((p[t], R[t] * q[t] * R[t + 1])) * 0.3).astype(np.float32) for t in range(3)]
    idx = rng.choice(n_emb, size=n, replace=False).astype(np.int64)
    offsets = np.arange(n + 1, dtype=np.int64)
    d_out = ((rng.random((n, int(np.prod(q)))) - 0.5) * 0.1).astype(np.float32)
    shape = nat.make_shape(p, q, R)
    assert nat.kernel_family(shape, n, n, True) & ~nat.FAMILY_ROUTE_FLAGS == nat.FAMILY_GROUPED
    want = [np.zeros_like(c, dtype=np.float64) for c in cores]
    for k in range(8):
        sl = slice(k * n // 8, (k + 1) * n // 8)
        part = orc.tt_dense_backward(idx[sl], np.arange(sl.stop - sl.start + 1, dtype=np.int64), d_out[sl], cores, p, q, R)
        for t in range(3):
            want[t] += part[t]
    want = [w.astype(np.float32) for w in want]
    _, grads = _run_ids_offsets(nat, p, q, R, cores, idx, offsets, d_out)
    assert_grads_close(grads, want, rel=2e-4)
    c = [dev(x) for x in cores]
    nat.backward_sgd(shape, c, dev(idx, torch.int64), None, n, None, n, dev(d_out), 0.05, nat.Workspace(), None, dev(offsets, torch.int64))
    torch.cuda.synchronize()
    for t in range(3):
        np.testing.assert_allclose(c[t].cpu().numpy(), cores[t] - np.float32(0.05) * want[t], rtol=0,
                                   atol=1e-5 + 2e-4 * float(np.abs(0.05 * want[t]).max()))


@pytest.mark.parametrize("q,r,Rpad", [([4, 5, 5], [12, 12], 16), ([4, 5, 5], [20, 28], 32), ([4, 4, 8], [48, 40], 64),
                                      ([5, 5, 4], [3, 5], 8), ([5, 5, 4], [100, 100], 128)])
def test_ranks_off_the_list_ride_on_the_grouped_path(nat, orc, q, r, Rpad):
    """Any rank in [2, 256] of an instantiated q shape (tuning_SAGE.py:213 searches that interval) runs the grouped MFMA
    kernels of the next listed rank through zero-padded cores: forward rows, dense gradients (with the forward's plan, as the
    module reuses it) and the fused SGD step against the oracle on the ORIGINAL cores; unequal ranks, ranks that are not
    multiples of 4, narrow and wide chains."""
    p = [40, 50, 60]
    R = [1] + r + [1]
    shape = nat.make_shape(p, q, R)
    rng = np.random.default_rng(sum(r) + Rpad)
    idx, offsets = _random_bags(rng, int(np.prod(p)), 30000)
    nnz, B = int(idx.shape[0]), int(offsets.shape[0] - 1)
    fam = nat.kernel_family(shape, nnz, B, True) & ~nat.FAMILY_ROUTE_FLAGS
    want_fam = (nat.FAMILY_GROUPED_WIDE if Rpad >= 64 else nat.FAMILY_GROUPED) | nat.FAMILY_PADDED
    assert fam == want_fam, f"kernel family {fam}"
    assert nat.plan_bytes(shape, nnz) > 0
    cores = [(rng.standard_normal((p[t], R[t] * q[t] * R[t + 1])) * (0.4 if Rpad < 64 else 0.1)).astype(np.float32) for t in range(3)]
    want = orc.tt_forward(idx, offsets, cores, p, q, R)
    d_out = ((rng.random(want.shape) - 0.5) * 0.2).astype(np.float32)
    want_g = orc.tt_dense_backward(idx, offsets, d_out, cores, p, q, R)
    c = [dev(x) for x in cores]
    t_idx, t_offs, t_d = dev(idx, torch.int64), dev(offsets, torch.int64), dev(d_out)
    ws = nat.Workspace()
    plan = nat.new_plan(shape, nnz, t_idx.device)
    out = torch.full((B, int(np.prod(q))), float("nan"), device="cuda")
    nat.forward(shape, c, t_idx, None, t_offs, nnz, None, B, out, ws, plan)
    grads = [torch.full_like(x, float("nan")) for x in c]
    nat.backward_dense(shape, c, t_idx, None, nnz, None, B, t_d, grads, ws, plan, t_offs)
    torch.cuda.synchronize()
    np.testing.assert_allclose(out.cpu().numpy(), want, rtol=1e-4, atol=1e-4 * max(1.0, float(np.abs(want).max())))
    assert_grads_close([g.cpu().numpy() for g in grads], want_g, rel=2e-4)
    nat.backward_sgd(shape, c, t_idx, None, nnz, None, B, t_d, 0.05, ws, plan, t_offs)
    torch.cuda.synchronize()
    for t in range(3):
        np.testing.assert_allclose(c[t].cpu().numpy(), cores[t] - np.float32(0.05) * want_g[t], rtol=0,
                                   atol=1e-5 + 2e-4 * float(np.abs(0.05 * want_g[t]).max()))


# ---------------------------------------------------------------------------------------
# a bounded device-side wait that runs out fails loud (include/ttemb.h: ttemb_status / ttemb_set_spin_limit)
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", [False, True])
def test_an_expired_wait_gives_nan_and_an_error_never_plausible_numbers(nat, orc, wide):
    """ttemb_set_spin_limit(-1): every bounded wait of the grouping pass expires (the look-back of every range but the first;
    on a fresh workspace the counter take-over too).  The forward must give NaN rows, a backward on that plan NaN gradients,
    a FUSED backward must leave parameters and optimizer state untouched (the host hears of the fault: nothing is lost, the
    step can be repeated) -- also on the routes that write gradients and step afterwards (ranks off the list) --, the next
    call TTEMB_E_HIP -- and the call after that, with the default limit, the oracle's numbers again on the same workspace."""
    p, q = [125, 140, 140], ([5, 5, 4] if wide else [4, 5, 5])
    R = [1, 64, 64, 1] if wide else [1, 16, 16, 1]
    rng = np.random.default_rng(11)
    cores = seeded_cores(p, q, R, 5, 0.3)
    n = 20000
    ids = rng.choice(p[0] * p[1] * p[2], size=n, replace=False).astype(np.int64)
    offs = np.arange(n + 1, dtype=np.int64)
    shape = nat.make_shape(p, q, R)
    nat.set_path(nat.PATH_FAST3)
    assert nat.kernel_family(shape, n, n) & ~nat.FAMILY_ROUTE_FLAGS in (nat.FAMILY_GROUPED, nat.FAMILY_GROUPED_WIDE)
    ws = nat.Workspace()
    c = [dev(x) for x in cores]
    idx, o = dev(ids), dev(offs)
    D = int(np.prod(q))
    plan = torch.empty(nat.plan_bytes(shape, n), dtype=torch.uint8, device="cuda")
    out = torch.zeros((n, D), device="cuda")
    nat.status()   # nothing pending
    nat.set_spin_limit(-1)
    nat.forward(shape, c, idx, None, o, n, None, n, out, ws, plan=plan)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()), "a forward whose grouping pass gave up must not return numbers"
    # the backward on the poisoned plan: NaN gradients (dense) ...
    d_out = torch.ones((n, D), device="cuda")
    grads = [torch.zeros_like(x) for x in c]
    with pytest.raises(RuntimeError, match="gave up waiting"):
        nat.backward_dense(shape, c, idx, None, n, None, n, d_out, grads, ws, plan=plan, offsets=o)   # the fault surfaces here, once
    nat.backward_dense(shape, c, idx, None, n, None, n, d_out, grads, ws, plan=plan, offsets=o)
    torch.cuda.synchronize()
    for g in grads:
        assert bool(torch.isnan(g).all()), "gradients of a poisoned plan must be NaN"
    word = nat.poison_word(ws)
    assert int(word.item()) == 1, "the finalize kernel of a poisoned backward marks the workspace header"
    # ... and in the fused modes NOTHING: parameters and the Adagrad state stay as they were (the pinned host word exists --
    # ttemb_init ran with the first Workspace.get -- so the fault is loud without NaN weights, and the step can be repeated)
    c2 = [x.clone() for x in c]
    nat.backward_sgd(shape, c2, idx, None, n, None, n, d_out, 0.1, ws, plan=plan, offsets=o)
    st2 = [torch.full_like(x, 0.25) for x in c]
    nat.backward_adagrad(shape, c2, st2, idx, None, n, None, n, d_out, 0.1, 1e-8, ws, plan=plan, offsets=o)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(c2, c)), "a fused step on a poisoned plan must not touch the parameters"
    assert all(bool((x == 0.25).all()) for x in st2), "... nor the optimizer state"
    nat.status()   # the backwards walked no wait: nothing new
    # a backward that regroups under the limit reports again
    nat.backward_dense(shape, c, idx, None, n, None, n, d_out, grads, ws, offsets=o)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(g).all()) for g in grads)
    with pytest.raises(RuntimeError, match="gave up waiting"):
        nat.status()
    nat.status()   # consumed
    if not wide:
        # ranks off the list ride on padded cores: the grouped backward writes (NaN) gradients and a separate kernel steps --
        # it reads the header's poison word and leaves the parameters alone as well
        R12 = [1, 12, 12, 1]
        shape12 = nat.make_shape(p, q, R12)
        assert nat.kernel_family(shape12, n, n) & nat.FAMILY_PADDED
        c12 = [dev(x) for x in seeded_cores(p, q, R12, 6, 0.3)]
        keep = [x.clone() for x in c12]
        nat.backward_sgd(shape12, c12, idx, None, n, None, n, d_out, 0.1, ws, offsets=o)
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(c12, keep)), "padded route: the step after a poisoned backward must be skipped"
        with pytest.raises(RuntimeError, match="gave up waiting"):
            nat.status()
    # default limit, same workspace and plan buffer: the oracle's rows and gradients
    nat.set_spin_limit(0)
    nat.forward(shape, c, idx, None, o, n, None, n, out, ws, plan=plan)
    nat.backward_dense(shape, c, idx, None, n, None, n, d_out, grads, ws, plan=plan, offsets=o)
    torch.cuda.synchronize()
    want = orc.tt_forward(ids, offs, cores, p, q, R)
    np.testing.assert_allclose(out.cpu().numpy(), want, rtol=1e-5, atol=1e-4)
    want_g = orc.tt_dense_backward(ids, offs, np.ones((n, D), dtype=np.float32), cores, p, q, R)
    tol = 2e-4 if wide else 1e-4   # (split-bf16 GEMMs of the wide chain: fp32-grade, see test_wide_rank_gemms_keep_fp32_accuracy)
    assert_grads_close([g.cpu().numpy() for g in grads], want_g, rel=tol)
    nat.status()
    assert int(nat.poison_word(ws).item()) == 0, "a healthy backward clears the header's poison word"
    if not wide:   # ... and the padded route steps again
        nat.backward_sgd(shape12, c12, idx, None, n, None, n, d_out, 0.1, ws, offsets=o)
        torch.cuda.synchronize()
        assert not any(torch.equal(x, y) for x, y in zip(c12, keep)) and all(bool(torch.isfinite(x).all()) for x in c12)
    # A stale fault word must never meet a later call that carries the same call number: call numbers live in the workspace
    # header and two zero-filled workspaces count alike.  Call no. 1 of workspace A faults into the plan buffer; call no. 1 of
    # workspace B builds a sound plan in the SAME buffer -- the place step clears the other call's word.
    big = nat.workspace_bytes(shape, nat.OP_BACKWARD, n, n) * 2
    ws_a, ws_b = nat.Workspace(), nat.Workspace()
    ws_a.buf = torch.zeros(big, dtype=torch.uint8, device="cuda")
    ws_b.buf = torch.zeros(big, dtype=torch.uint8, device="cuda")
    nat.set_spin_limit(-1)
    nat.forward(shape, c, idx, None, o, n, None, n, out, ws_a, plan=plan)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    with pytest.raises(RuntimeError, match="gave up waiting"):
        nat.status()
    nat.set_spin_limit(0)
    nat.forward(shape, c, idx, None, o, n, None, n, out, ws_b, plan=plan)
    torch.cuda.synchronize()
    np.testing.assert_allclose(out.cpu().numpy(), want, rtol=1e-5, atol=1e-4)
    nat.status()


# ---------------------------------------------------------------------------------------
# frontiers with few ids per group: the forward forms the prefix products inside its chain kernel
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("q,r", [([8, 4, 4], [32, 32]), ([4, 4, 8], [16, 16]), ([4, 5, 5], [16, 16]), ([5, 5, 4], [16, 16]),
                                 ([4, 5, 5], [8, 8]), ([4, 4, 8], [8, 8]), ([5, 4, 5], [16, 16]), ([8, 4, 4], [16, 16])])
@pytest.mark.parametrize("p0", [40, 41])
def test_forward_with_the_prefix_products_formed_in_the_chain_kernel(nat, orc, q, r, p0):
    """~3 ids per (i0, i1) group: ttemb_forward takes fast3_forward_pfuse_kernel (asked from the library).  Batches of 16 / q0
    groups -- 2 (q0 = 8), 3 with an idle tile row (q0 = 5), 4 (q0 = 4) --, a p0 the batch size does not divide (a short
    batch at the end of every i1), the masked column tile of q1 r2 = 40 (rank 8), ragged bags with duplicates and empty bags.
    Rows against the oracle; then the dense backward and the fused SGD step ON THE FORWARD'S PLAN, whose prefix products the
    forward's chain kernel stored: gradients and cores against the oracle."""
    p = [p0, 50, 30]
    R = [1] + r + [1]
    shape = nat.make_shape(p, q, R)
    rng = np.random.default_rng(p0 + sum(q) + sum(r))
    idx, offsets = _random_bags(rng, int(np.prod(p)), 6000)
    nnz, B = int(idx.shape[0]), int(offsets.shape[0] - 1)
    nat.set_path(nat.PATH_FAST3)
    assert nat.kernel_family(shape, nnz, B, True) & ~nat.FAMILY_GROUP_PRODUCTS_IN_CHAIN == nat.FAMILY_GROUPED | nat.FAMILY_PREFIX_IN_CHAIN
    cores = [(rng.standard_normal((p[t], R[t] * q[t] * R[t + 1])) * 0.4).astype(np.float32) for t in range(3)]
    want = orc.tt_forward(idx, offsets, cores, p, q, R)
    c = [dev(x) for x in cores]
    t_idx, t_offs = dev(idx, torch.int64), dev(offsets, torch.int64)
    ws = nat.Workspace()
    plan = nat.new_plan(shape, nnz, t_idx.device)
    out = torch.full((B, int(np.prod(q))), float("nan"), device="cuda")
    nat.forward(shape, c, t_idx, None, t_offs, nnz, None, B, out, ws, plan)
    torch.cuda.synchronize()
    np.testing.assert_allclose(out.cpu().numpy(), want, rtol=1e-5, atol=1e-4)
    d_out = ((rng.random(want.shape) - 0.5) * 0.2).astype(np.float32)
    want_g = orc.tt_dense_backward(idx, offsets, d_out, cores, p, q, R)
    grads = [torch.full_like(x, float("nan")) for x in c]
    nat.backward_dense(shape, c, t_idx, None, nnz, None, B, dev(d_out), grads, ws, plan, t_offs)
    torch.cuda.synchronize()
    assert_grads_close([g.cpu().numpy() for g in grads], want_g)
    # the same gradients from a backward that builds its own plan (prefix launch): the two P tables agree
    grads2 = [torch.full_like(x, float("nan")) for x in c]
    nat.backward_dense(shape, c, t_idx, None, nnz, None, B, dev(d_out), grads2, ws, None, t_offs)
    torch.cuda.synchronize()
    assert_grads_close([g.cpu().numpy() for g in grads2], want_g)
    lr = 0.05
    c2 = [x.clone() for x in c]
    nat.backward_sgd(shape, c2, t_idx, None, nnz, None, B, dev(d_out), lr, ws, plan, t_offs)
    torch.cuda.synchronize()
    for got, w0, g in zip(c2, cores, want_g):
        np.testing.assert_allclose(got.cpu().numpy(), w0 - lr * g, rtol=0, atol=1e-5 + 1e-4 * float(np.abs(lr * g).max()))


# ---------------------------------------------------------------------------------------
# frontiers with few ids per group: the backward forms the per-group products (dG0 parts, dG1) inside its chunk kernel
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("q,r,p2", [([8, 4, 4], [32, 32], 30), ([4, 4, 8], [32, 32], 30), ([4, 5, 5], [32, 32], 35), ([5, 5, 4], [32, 32], 30),
                                   ([4, 4, 8], [16, 16], 600), ([4, 5, 5], [16, 16], 700), ([5, 5, 4], [16, 16], 700),
                                   ([8, 4, 4], [16, 16], 700), ([5, 4, 5], [16, 16], 700), ([4, 4, 8], [8, 8], 900)])
@pytest.mark.parametrize("p0", [40, 41])
def test_backward_with_the_group_products_formed_in_the_chunk_kernel(nat, orc, q, r, p2, p0):
    """~3 ids per (i0, i1) group on shapes whose dG2 reduction is not fused into the chunk kernel (rank 32; p2 past the
    register slab): ttemb_backward_* takes fast3_bwd_chunk_kernel<..., GF> -- asked from the library -- which multiplies a
    batch of 16 / q0 groups' dP with G1[i1]^T and G0^T while dP is in registers (no dP table, no epilogue launch).  Batches of
    2 / 3 (idle tile row) / 4 groups, a p0 the batch size does not divide (a short batch at the end of every i1), the narrow
    last row tile of q0 q1 = 20, groups that span several chunks (a hot group of 50 ids, another of 17), duplicate ids,
    ragged bags with empty ones.  Dense gradients, then the fused SGD step, on the forward's plan and on a plan the backward
    builds itself, against the oracle; Adagrad once."""
    p = [p0, 50, p2]
    R = [1] + r + [1]
    shape = nat.make_shape(p, q, R)
    rng = np.random.default_rng(p0 + sum(q) + sum(r) + p2)
    idx, offsets = _random_bags(rng, int(np.prod(p)), 6000)
    # two hot groups: 50 ids of group (i0 = 3, i1 = 7) -- four chunks --, 17 of the LAST group of an i1 (i0 = p0 - 1: the short batch)
    hot = lambda i0, i1, k: (i0 * p[1] + i1) * p[2] + rng.integers(0, p[2], size=k)
    idx[100:150] = hot(3, 7, 50)
    idx[300:317] = hot(p0 - 1, 11, 17)
    nnz, B = int(idx.shape[0]), int(offsets.shape[0] - 1)
    nat.set_path(nat.PATH_FAST3)
    fam = nat.kernel_family(shape, nnz, B, True)
    assert fam & nat.FAMILY_GROUP_PRODUCTS_IN_CHAIN and fam & 7 == nat.FAMILY_GROUPED, f"kernel family {fam}"
    cores = [(rng.standard_normal((p[t], R[t] * q[t] * R[t + 1])) * 0.4).astype(np.float32) for t in range(3)]
    c = [dev(x) for x in cores]
    t_idx, t_offs = dev(idx, torch.int64), dev(offsets, torch.int64)
    ws = nat.Workspace()
    plan = nat.new_plan(shape, nnz, t_idx.device)
    D = int(np.prod(q))
    out = torch.empty((B, D), device="cuda")
    nat.forward(shape, c, t_idx, None, t_offs, nnz, None, B, out, ws, plan)
    d_out = ((rng.random((B, D)) - 0.5) * 0.2).astype(np.float32)
    want_g = orc.tt_dense_backward(idx, offsets, d_out, cores, p, q, R)
    for use_plan in (plan, None):
        grads = [torch.full_like(x, float("nan")) for x in c]
        nat.backward_dense(shape, c, t_idx, None, nnz, None, B, dev(d_out), grads, ws, use_plan, t_offs)
        torch.cuda.synchronize()
        assert_grads_close([g.cpu().numpy() for g in grads], want_g)
    lr = 0.05
    c2 = [x.clone() for x in c]
    nat.backward_sgd(shape, c2, t_idx, None, nnz, None, B, dev(d_out), lr, ws, plan, t_offs)
    torch.cuda.synchronize()
    for got, w0, g in zip(c2, cores, want_g):
        np.testing.assert_allclose(got.cpu().numpy(), w0 - lr * g, rtol=0, atol=1e-5 + 1e-4 * float(np.abs(lr * g).max()))
    c3, st3 = [x.clone() for x in c], [torch.zeros_like(x) for x in c]
    nat.backward_adagrad(shape, c3, st3, t_idx, None, nnz, None, B, dev(d_out), lr, 1e-6, ws, plan, t_offs)
    torch.cuda.synchronize()
    for got, st, w0, g in zip(c3, st3, cores, want_g):
        np.testing.assert_allclose(st.cpu().numpy(), g * g, rtol=2e-4, atol=1e-6 * float((g * g).max()) + 1e-12)
        ref = w0 - lr * g / (np.sqrt(g * g) + 1e-6)
        big = np.abs(g) > 1e-3 * float(np.abs(g).max())   # (where g ~ 0 the step is lr * g / (|g| + eps): any rounding of g flips it)
        np.testing.assert_allclose(got.cpu().numpy()[big], ref[big], rtol=0, atol=2e-3 * lr)


# ---------------------------------------------------------------------------------------
# tables with many i1: the finalize kernel sums the dG0 parts with 16-byte loads over 32 lane rows (p1 >= 256)
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("q,r,p,nnz_target", [
    ([4, 5, 5], [16, 16], [16, 320, 24], 3000),     # epilogue kernel, sparse form (0.6 ids per group: parts of the non-empty groups only)
    ([4, 5, 5], [16, 16], [16, 320, 24], 45000),    # epilogue kernel, dense form (every group has a part)
    ([8, 4, 4], [32, 32], [14, 300, 20], 9000),     # the chunk kernel forms the group products (parts by the groups' counts)
    ([5, 5, 4], [64, 64], [10, 260, 30], 30000),    # wide-rank chain (slab kernel or E table by size: parts by counts, one dG1 slab per K split)
])
def test_backward_on_tables_with_many_i1(nat, orc, q, r, p, nnz_target):
    """p1 >= 256 (papers100M: 560; the reference's own papers run: 500): the dG0 sums of fast3_finalize_kernel take their
    16-byte form -- 8 threads x float4 per 32 outputs, 32 lane rows over i1 -- in all three of its modes.  Dense gradients and
    the fused SGD step against the oracle, ragged bags with duplicates."""
    R = [1] + r + [1]
    shape = nat.make_shape(p, q, R)
    rng = np.random.default_rng(sum(p) + sum(q) + nnz_target)
    idx, offsets = _random_bags(rng, int(np.prod(p)), nnz_target)
    nnz, B = int(idx.shape[0]), int(offsets.shape[0] - 1)
    nat.set_path(nat.PATH_FAST3)
    fam = nat.kernel_family(shape, nnz, B, True)
    assert fam & 7 in (nat.FAMILY_GROUPED, nat.FAMILY_GROUPED_WIDE), f"kernel family {fam}"
    cores = [(rng.standard_normal((p[t], R[t] * q[t] * R[t + 1])) * (0.4 if r[0] < 64 else 0.15)).astype(np.float32) for t in range(3)]
    c = [dev(x) for x in cores]
    t_idx, t_offs = dev(idx, torch.int64), dev(offsets, torch.int64)
    ws = nat.Workspace()
    plan = nat.new_plan(shape, nnz, t_idx.device)
    D = int(np.prod(q))
    out = torch.empty((B, D), device="cuda")
    nat.forward(shape, c, t_idx, None, t_offs, nnz, None, B, out, ws, plan)
    d_out = ((rng.random((B, D)) - 0.5) * 0.2).astype(np.float32)
    want_g = orc.tt_dense_backward(idx, offsets, d_out, cores, p, q, R)
    grads = [torch.full_like(x, float("nan")) for x in c]
    nat.backward_dense(shape, c, t_idx, None, nnz, None, B, dev(d_out), grads, ws, plan, t_offs)
    torch.cuda.synchronize()
    assert_grads_close([g.cpu().numpy() for g in grads], want_g, rel=2e-4 if r[0] >= 64 else 1e-4)
    lr = 0.05
    c2 = [x.clone() for x in c]
    nat.backward_sgd(shape, c2, t_idx, None, nnz, None, B, dev(d_out), lr, ws, plan, t_offs)
    torch.cuda.synchronize()
    for got, w0, g in zip(c2, cores, want_g):
        np.testing.assert_allclose(got.cpu().numpy(), w0 - lr * g, rtol=0, atol=1e-5 + 2e-4 * float(np.abs(lr * g).max()))


# ---------------------------------------------------------------------------------------
# windows of a longer id list: one table of a table-batched call (ttemb_*_window)
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,q,R", [
    ([10, 12, 9], [4, 4, 8], [1, 8, 8, 1]),
    ([20, 25, 30], [4, 5, 5], [1, 16, 16, 1]),
    ([12, 14, 40], [8, 4, 4], [1, 32, 32, 1]),
    ([9, 11, 13], [5, 5, 4], [1, 64, 64, 1]),      # the wide-rank chain
])
@pytest.mark.parametrize("mode", ["dense", "sgd", "adagrad"])
def test_window_calls_serve_the_tables_of_a_table_batched_call(nat, orc, p, q, R, mode):
    """Four tables looked up in one id list (`offsets` of 4 B + 1 entries, as TableBatchedTTEmbeddingBag gets them): every table
    is a window call that finds its ids through `offsets` on the device.  Ragged bags, empty bags, a table WITHOUT ids, one
    with a single id; rows of the other tables are not touched.  Forward, then dense gradients / fused SGD / fused Adagrad per
    table, against the oracle run on the host-side split."""
    nat.set_path(nat.PATH_AUTO)
    rng = np.random.default_rng(p[0] + R[1])
    n_emb, D, T, B = int(np.prod(p)), int(np.prod(q)), 4, 37
    lens = rng.integers(0, 5, size=T * B)
    lens[2 * B:3 * B] = 0                      # table 2 holds no id at all
    lens[3 * B:] = 0
    lens[3 * B + 5] = 1                        # table 3: one id
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    nnz = int(offsets[-1])
    idx = rng.integers(0, n_emb, size=nnz).astype(np.int64)
    idx[:40] = idx[40:80]                      # repeated ids
    cores = [[(rng.standard_normal((p[t], R[t] * q[t] * R[t + 1])) * 0.4).astype(np.float32) for t in range(3)] for _ in range(T)]
    shape = nat.make_shape(p, q, R)
    assert nat.window_workspace_bytes(shape, nat.OP_BACKWARD, nnz, T * B, B) > 0
    ws = nat.Workspace()
    d_idx, d_offs = dev(idx, torch.int64), dev(offsets, torch.int64)
    d_cores = [[dev(c) for c in tab] for tab in cores]
    out = torch.full((T * B, D), 7.0, device="cuda")
    for k in (1, 3):                           # two of the four first: the others' rows keep their sentinel
        nat.forward_window(shape, d_cores[k], d_idx, d_offs, k * B, B, out, ws)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[:B] == 7.0).all() and (got[2 * B:3 * B] == 7.0).all()
    for k in (0, 2):
        nat.forward_window(shape, d_cores[k], d_idx, d_offs, k * B, B, out, ws)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    split = lambda k: (idx[offsets[k * B]:offsets[(k + 1) * B]], offsets[k * B:(k + 1) * B + 1] - offsets[k * B])
    for k in range(T):
        ids_k, offs_k = split(k)
        want = orc.tt_forward(ids_k, offs_k, cores[k], p, q, R)
        np.testing.assert_allclose(got[k * B:(k + 1) * B], want, rtol=1e-4, atol=1e-4 * max(1.0, float(np.abs(want).max())))
    d_out = (rng.standard_normal((T * B, D)) * 0.5).astype(np.float32)
    d_dout = dev(d_out)
    lr, eps = 0.05, 1e-3
    for k in range(T):
        ids_k, offs_k = split(k)
        grads = orc.tt_dense_backward(ids_k, offs_k, d_out[k * B:(k + 1) * B], cores[k], p, q, R)
        if mode == "dense":
            g = [torch.full_like(c, float("nan")) for c in d_cores[k]]
            nat.backward_window(shape, d_cores[k], d_idx, d_offs, k * B, B, d_dout, ws, d_cores=g)
            torch.cuda.synchronize()
            assert_grads_close([x.cpu().numpy() for x in g], grads, rel=2e-4)
        elif mode == "sgd":
            w = [c.clone() for c in d_cores[k]]
            nat.backward_window(shape, w, d_idx, d_offs, k * B, B, d_dout, ws, lr=lr)
            torch.cuda.synchronize()
            assert_grads_close([x.cpu().numpy() for x in w], orc.sgd_step(cores[k], grads, lr), rel=2e-4)
        else:
            w = [c.clone() for c in d_cores[k]]
            st0 = [(rng.random(c.shape) * 0.1).astype(np.float32) for c in cores[k]]
            st = [dev(s) for s in st0]
            nat.backward_window(shape, w, d_idx, d_offs, k * B, B, d_dout, ws, opt_state=st, lr=lr, eps=eps)
            torch.cuda.synchronize()
            want_w, want_s = orc.adagrad_step(cores[k], st0, grads, lr, eps)
            assert_grads_close([x.cpu().numpy() for x in st], want_s, rel=2e-4)
            assert_grads_close([x.cpu().numpy() for x in w], want_w, rel=5e-4)


def test_window_calls_refuse_what_the_grouped_kernels_do_not_cover(nat):
    """A shape off the grouped kernels' list, a forced generic path: the size query answers -1 (the binding's spelling of
    TTEMB_E_UNSUPPORTED) and the caller splits the id list on the host instead."""
    nat.set_path(nat.PATH_AUTO)
    assert nat.window_workspace_bytes(nat.make_shape([7, 9, 11, 5], [2, 2, 5, 4], [5, 6, 3]), nat.OP_FORWARD, 1000, 80, 20) == -1
    assert nat.window_workspace_bytes(nat.make_shape([10, 12, 9], [4, 4, 8], [12, 12]), nat.OP_FORWARD, 1000, 80, 20) == -1
    ok = nat.make_shape([10, 12, 9], [4, 4, 8], [8, 8])
    assert nat.window_workspace_bytes(ok, nat.OP_FORWARD, 1000, 80, 20) > 0
    nat.set_path(nat.PATH_GENERIC)
    try:
        assert nat.window_workspace_bytes(ok, nat.OP_FORWARD, 1000, 80, 20) == -1
    finally:
        nat.set_path(nat.PATH_AUTO)
