"""Weighted and mean bags against what they replace, on the products table (p = 125.140.140, q = 4.5.5, r = 16.16), all
cases alternating in one process, each timed with HIP events around one training step (forward + fused SGD backward):
  frontier   409 600 ids in bags of one: plain vs per_sample_weights (the weighted call adds the [nnz, D] rows buffer,
             bag_reduce and bag_reduce_backward)
  gnn        40 960 dst bags x fanout 10 (409 600 edge ids): mode="mean" and GCN-weighted sum, against the two-step
             baseline a user writes today: look the unique frontier rows up (bags of one), then F.embedding_bag over them
             (the unique ids and the edge -> row map are computed once, outside the timed steps)
  hub        one bag holding all 409 600 ids: weighted and mean
  copy       a device-to-device copy of the rows buffer (164 MB), the bandwidth yardstick for the new kernels
Prints one JSON line per case (median ms over --iters steps after --warmup) and the bytes each new kernel moves per call
(computed from the shapes; divide by the kernel times of a `rocprofv3 --kernel-trace --stats` run of the same command).
--out writes everything as one JSON file."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "falcon-ttdforgnns_amd")]

from FBTT.tt_embeddings_ops import OptimType, TTEmbeddingBag  # noqa: E402

P, Q, R = [125, 140, 140], [4, 5, 5], [16, 16]
N_IDS, FANOUT = 409_600, 10


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    return a, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows, D = int(np.prod(P)), int(np.prod(Q))
    rng = np.random.default_rng(0)
    dev = "cuda"
    mods = {}
    for mode in ("sum", "mean"):
        torch.manual_seed(0)
        mods[mode] = TTEmbeddingBag(rows, D, R, P, Q, optimizer=OptimType.SGD, learning_rate=1e-6, use_cache=False,
                                    weight_dist="normal", mode=mode)
    ids = torch.as_tensor(rng.integers(0, rows, size=N_IDS)).to(dev)
    ones = torch.arange(N_IDS + 1, device=dev)
    w = torch.as_tensor(rng.random(N_IDS).astype(np.float32)).to(dev)
    # GNN block: dst bags of FANOUT source ids drawn from a frontier of 3x the dst count; GCN weights 1/sqrt(d_i d_j)
    n_dst = N_IDS // FANOUT
    frontier = torch.as_tensor(rng.choice(rows, size=3 * n_dst, replace=False)).to(dev)
    local = torch.as_tensor(rng.integers(0, 3 * n_dst, size=N_IDS)).to(dev)
    edge_ids = frontier[local]
    csr = torch.arange(0, N_IDS + 1, FANOUT, device=dev)
    deg = torch.as_tensor(rng.integers(1, 50, size=3 * n_dst).astype(np.float32)).to(dev)
    gcn = (1.0 / torch.sqrt(deg[local] * FANOUT)).contiguous()
    uniq, inverse = torch.unique(edge_ids, return_inverse=True)   # (outside the timed steps)
    uniq_offs = torch.arange(uniq.numel() + 1, device=dev)
    hub = torch.tensor([0, N_IDS], device=dev)
    dy = {"frontier": torch.randn(N_IDS, D, device=dev) * 1e-3, "gnn": torch.randn(n_dst, D, device=dev) * 1e-3,
          "hub": torch.randn(1, D, device=dev) * 1e-3}
    s, m = mods["sum"], mods["mean"]
    src = torch.empty(N_IDS, D, device=dev)
    dst = torch.empty_like(src)

    def baseline(weights, mode):
        r = s(uniq, uniq_offs)
        return F.embedding_bag(inverse, r, csr, mode=mode, per_sample_weights=weights, include_last_offset=True)

    cases = {
        "frontier_plain": lambda: s(ids, ones).backward(dy["frontier"]),
        "frontier_weighted": lambda: s(ids, ones, per_sample_weights=w).backward(dy["frontier"]),
        "gnn_mean": lambda: m(edge_ids, csr).backward(dy["gnn"]),
        "gnn_mean_two_step": lambda: baseline(None, "mean").backward(dy["gnn"]),
        "gnn_gcn": lambda: s(edge_ids, csr, per_sample_weights=gcn).backward(dy["gnn"]),
        "gnn_gcn_two_step": lambda: baseline(gcn, "sum").backward(dy["gnn"]),
        "hub_weighted": lambda: s(ids, hub, per_sample_weights=w).backward(dy["hub"]),
        "hub_mean": lambda: m(ids, hub).backward(dy["hub"]),
        "copy_rows_buffer": lambda: dst.copy_(src),
    }
    for fn in cases.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    ev = {k: [] for k in cases}
    for _ in range(a.iters):   # alternate the cases, one timed step each
        for k, fn in cases.items():
            ev[k].append(_timed(fn))
    torch.cuda.synchronize()
    ms = {k: float(np.median([x.elapsed_time(y) for x, y in v])) for k, v in ev.items()}
    f4, i8 = 4, 8
    rows_b = N_IDS * D * f4
    res = {
        "device": torch.cuda.get_device_name(0), "iters": a.iters, "ids": N_IDS, "D": D, "unique_frontier_rows": int(uniq.numel()),
        "step_ms": {k: round(v, 4) for k, v in ms.items()},
        "frontier_weighted_overhead_ms": round(ms["frontier_weighted"] - ms["frontier_plain"], 4),
        "frontier_weighted_overhead_pct": round(100 * (ms["frontier_weighted"] / ms["frontier_plain"] - 1), 1),
        "gnn_mean_vs_two_step": round(ms["gnn_mean"] / ms["gnn_mean_two_step"], 3),
        "gnn_gcn_vs_two_step": round(ms["gnn_gcn"] / ms["gnn_gcn_two_step"], 3),
        "copy_GBps": round(2 * rows_b / ms["copy_rows_buffer"] / 1e6, 1),
        # bytes a kernel has to move per call (reads + writes), from the shapes
        "kernel_bytes": {
            "frontier bag_reduce_kernel": rows_b + N_IDS * f4 + (N_IDS + 1) * i8 + rows_b,
            "frontier bag_reduce_backward_kernel": rows_b + N_IDS * f4 + (N_IDS + 1) * i8 + rows_b,
            "gnn_gcn bag_reduce_kernel": rows_b + N_IDS * f4 + (n_dst + 1) * i8 + n_dst * D * f4,
            "gnn_gcn bag_reduce_backward_kernel": n_dst * D * f4 + N_IDS * f4 + (n_dst + 1) * i8 + rows_b,
            "gnn_mean bag_mean_kernel": 2 * n_dst * D * f4 + (n_dst + 1) * i8,
            "hub bag_partial_kernel": rows_b + N_IDS * f4,
        },
    }
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
