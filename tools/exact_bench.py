"""Exact mode against the default lookup, in one process, the two alternating: forward alone and the fused SGD step
(forward + backward) on
  products   p = 125.140.140, q = 4.5.5, r = 16.16, 409 600 ids, one per bag (the headline workload)
  ragged     the same ids in ragged bags of mean length 4
  papers     p = 500.560.400, q = 8.4.4, r = 32.32, 819 200 ids, one per bag
Prints one JSON line per case (median ms over --iters timed repetitions, exact / default ratios) and writes them all to
--out when given."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "falcon-ttdforgnns_amd")]

from FBTT.tt_embeddings_ops import OptimType, TTEmbeddingBag  # noqa: E402

CASES = {
    "products": ([125, 140, 140], [4, 5, 5], [16, 16], 409_600, 1),
    "ragged": ([125, 140, 140], [4, 5, 5], [16, 16], 409_600, 4),
    "papers": ([500, 560, 400], [8, 4, 4], [32, 32], 819_200, 1),
}


def _time(fn, iters):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def run_case(name, iters, warmup):
    p, q, r, n, mean = CASES[name]
    rows = int(np.prod(p))
    rng = np.random.default_rng(0)
    ids = torch.as_tensor(rng.integers(0, rows, size=n).astype(np.int64)).cuda()
    if mean == 1:
        offs = torch.arange(n + 1, dtype=torch.int64, device="cuda")
    else:
        lens = rng.integers(1, 2 * mean, size=2 * n // mean)
        cut = np.concatenate([[0], np.cumsum(lens)])
        cut = np.concatenate([cut[cut < n], [n]])
        offs = torch.as_tensor(cut.astype(np.int64)).cuda()
    B = offs.numel() - 1
    D = int(np.prod(q))
    dy = torch.randn(B, D, device="cuda") * 1e-3
    mods = {}
    for mode in ("default", "exact"):
        torch.manual_seed(0)
        mods[mode] = TTEmbeddingBag(rows, D, r, p, q, optimizer=OptimType.SGD, learning_rate=1e-4, use_cache=False,
                                    weight_dist="normal", deterministic=(mode == "exact"))

    def fwd(m):
        with torch.no_grad():
            m(ids, offs)

    def step(m):
        m(ids, offs).backward(dy)

    res = {"case": name, "ids": n, "bags": B}
    for what, fn in (("forward", fwd), ("sgd_step", step)):
        for m in mods.values():
            _time(lambda: fn(m), warmup)
        t = {"default": [], "exact": []}
        for _ in range(iters):   # alternate the two, one timed repetition each
            for mode, m in mods.items():
                t[mode] += _time(lambda: fn(m), 1)
        for mode in t:
            res[f"{what}_{mode}_ms"] = round(float(np.median(t[mode])), 4)
        res[f"{what}_ratio"] = round(res[f"{what}_exact_ms"] / res[f"{what}_default_ms"], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = []
    for name in a.cases.split(","):
        res = run_case(name, a.iters, a.warmup)
        print(json.dumps(res), flush=True)
        out.append(res)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "results": out}, f, indent=1)


if __name__ == "__main__":
    main()
