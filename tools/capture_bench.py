"""What a captured lookup of VARIABLE size costs, on the products table (p = 125.140.140, q = 4.5.5, r = 16.16) with fused
SGD, one training step (forward + backward with its update) of n unique ids in bags of one, n = 2 048 and 409 600:
  eager       emb(ids, offsets).backward(dy)
  fixed       emb.capture(n, n): the call of exactly n ids
  var_n       emb.capture(n, n, variable=True) at live size n: the staging launch and the device count on top of `fixed`
  var_2n      emb.capture(2n, 2n, variable=True) at live size n: launches sized by twice the live size
One process; the legs alternate (eager, fixed, var_n, var_2n, eager, ...) in blocks of --steps steps, so `fixed` and `var_n`
see the same clocks.  Per block: host_us = time to enqueue the block / steps (no synchronisation inside a block), wall_us =
time until the device has finished it / steps.  Reported: the median over --rounds blocks.  The first failure ends the run.
Prints one JSON line; --out writes it as a JSON file."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "falcon-ttdforgnns_amd")]

from FBTT.tt_embeddings_ops import OptimType, TTEmbeddingBag  # noqa: E402

P, Q, R = [125, 140, 140], [4, 5, 5], [16, 16]
SIZES = (2_048, 409_600)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50, help="steps per block")
    ap.add_argument("--rounds", type=int, default=9, help="blocks per leg")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows, D = 2_449_029, int(np.prod(Q))
    dev = "cuda"
    rng = np.random.default_rng(0)

    def module():
        torch.manual_seed(0)
        return TTEmbeddingBag(rows, D, R, P, Q, optimizer=OptimType.SGD, learning_rate=1e-6, use_cache=False, weight_dist="normal")

    res = {"device": torch.cuda.get_device_name(0), "steps_per_block": a.steps, "rounds": a.rounds, "sizes": {}}
    for n in SIZES:
        ids = torch.as_tensor(rng.choice(rows, size=n, replace=False).astype(np.int64)).to(dev)
        offs = torch.arange(n + 1, device=dev)
        dy = torch.randn(n, D, device=dev) * 1e-3
        eager = module()
        fixed = module().capture(n, n)
        var_n = module().capture(n, n, variable=True)
        var_2n = module().capture(2 * n, 2 * n, variable=True)
        legs = {
            "eager": lambda: eager(ids, offs).backward(dy),
            "fixed": lambda: fixed(ids).backward(dy),
            "var_n": lambda: var_n(ids).backward(dy),
            "var_2n": lambda: var_2n(ids).backward(dy),
        }
        for fn in legs.values():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        host = {k: [] for k in legs}
        wall = {k: [] for k in legs}
        for _ in range(a.rounds):
            for k, fn in legs.items():
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    fn()
                t1 = time.perf_counter()
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                host[k].append((t1 - t0) / a.steps * 1e6)
                wall[k].append((t2 - t0) / a.steps * 1e6)
        med = lambda v: round(float(np.median(v)), 1)
        res["sizes"][str(n)] = {
            "wall_us": {k: med(v) for k, v in wall.items()},
            "host_us": {k: med(v) for k, v in host.items()},
            "var_n_vs_fixed_wall": round(float(np.median(wall["var_n"]) / np.median(wall["fixed"])), 3),
            "var_2n_vs_var_n_wall": round(float(np.median(wall["var_2n"]) / np.median(wall["var_n"])), 3),
        }
        del fixed, var_n, var_2n, eager, legs
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
