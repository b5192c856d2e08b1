"""The dedup route against the route it replaces, on the products table (p = 125.140.140, q = 4.5.5, r = 16.16), one training
step (forward + fused SGD backward) timed with HIP events, `dedup=False` and `dedup=True` alternating inside one process on
one module (the per-call keyword).  Legs:
  block_weighted   a 40 960 x 10 neighbour block with per-sample weights (the GCN sum of DESIGN 4.7)
  block_mean       the same block in mean mode (dedup=False: the plain bag sums and a division)
  ones_weighted    409 600 ids in bags of one with weights (src / dst / negative lookups)
each at several duplication levels: the ids are a permutation (every id distinct: the pure overhead of the pass) or drawn
uniformly from a pool of nnz / 2, nnz / 4, nnz / 16 values.  The distinct fraction U / nnz is printed next to every time.
Prints one text line per leg and level and one JSON line at the end (median ms over --iters steps after --warmup); --out
writes the text."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "falcon-ttdforgnns_amd")]

from FBTT.tt_embeddings_ops import OptimType, TTEmbeddingBag  # noqa: E402

P, Q, R = [125, 140, 140], [4, 5, 5], [16, 16]
N_DST, FANOUT = 40_960, 10
POOLS = (0, 2, 4, 16)   # 0: a permutation; k: drawn from nnz / k values


def pool_ids(rng, rows, nnz, pool):
    """``nnz`` ids of a table of ``rows``: a permutation (``pool == 0``: every id distinct) or drawn uniformly from a pool of
    ``nnz // pool`` values.  Also the generator of ``tools/capture_bags_bench.py --dedup``."""
    if pool == 0:
        return rng.permutation(rows)[:nnz]
    return rng.choice(rows, nnz // pool, replace=False)[rng.integers(0, nnz // pool, size=nnz)]


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    return a, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows, D = int(np.prod(P)), int(np.prod(Q))
    nnz = N_DST * FANOUT
    rng = np.random.default_rng(0)
    dev = "cuda"
    torch.manual_seed(0)
    mods = {mode: TTEmbeddingBag(rows, D, R, P, Q, optimizer=OptimType.SGD, learning_rate=1e-6, use_cache=False,
                                 weight_dist="normal", mode=mode) for mode in ("sum", "mean")}
    w = torch.as_tensor(rng.random(nnz).astype(np.float32)).to(dev)
    ones = torch.arange(nnz + 1, device=dev)
    dy_block = torch.randn(N_DST, D, device=dev) * 1e-3
    dy_ones = torch.randn(nnz, D, device=dev) * 1e-3

    cases, frac = {}, {}
    for pool in POOLS:
        ids_np = pool_ids(rng, rows, nnz, pool)
        level = "distinct" if pool == 0 else f"pool_nnz/{pool}"
        frac[level] = np.unique(ids_np).shape[0] / nnz
        ids = torch.as_tensor(ids_np.astype(np.int64)).to(dev)
        nbr = ids.view(N_DST, FANOUT)
        for dedup in (False, True):
            cases[("block_weighted", level, dedup)] = (
                lambda nbr=nbr, dedup=dedup: mods["sum"](nbr, per_sample_weights=w.view(N_DST, FANOUT), dedup=dedup).backward(dy_block))
            cases[("block_mean", level, dedup)] = (
                lambda nbr=nbr, dedup=dedup: mods["mean"](nbr, dedup=dedup).backward(dy_block))
            cases[("ones_weighted", level, dedup)] = (
                lambda ids=ids, dedup=dedup: mods["sum"](ids, ones, per_sample_weights=w, dedup=dedup).backward(dy_ones))
    for fn in cases.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    ev = {k: [] for k in cases}
    for _ in range(a.iters):   # alternate the legs, one timed step each
        for k, fn in cases.items():
            ev[k].append(_timed(fn))
    torch.cuda.synchronize()
    ms = {k: float(np.median([x.elapsed_time(y) for x, y in v])) for k, v in ev.items()}
    lines = [f"# {torch.cuda.get_device_name(0)}, products table, {nnz} ids, fused SGD step, median of {a.iters} steps (ms)",
             f"# {'leg':16s} {'ids':14s} {'distinct':>9s} {'dedup=False':>12s} {'dedup=True':>11s} {'ratio':>7s}"]
    res = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "ids": nnz, "legs": []}
    for leg in ("block_weighted", "block_mean", "ones_weighted"):
        for level in frac:
            off, on = ms[(leg, level, False)], ms[(leg, level, True)]
            lines.append(f"  {leg:16s} {level:14s} {frac[level]:9.3f} {off:12.4f} {on:11.4f} {on / off:7.3f}")
            res["legs"].append({"leg": leg, "ids": level, "distinct_fraction": round(frac[level], 4), "off_ms": round(off, 4),
                                "on_ms": round(on, 4), "on_over_off": round(on / off, 3)})
    text = "\n".join(lines)
    print(text, flush=True)
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
