"""The fused Adam step against what it replaces, on the products table (p = 125.140.140, q = 4.5.5, r = 16.16) at 409 600
ids and at the literal 2 048-id batch.  One process, the legs alternating, one training step (forward + backward + update)
per timed window:
  sgd            fused SGD step (sparse=True, OptimType.SGD): the headline step
  adam           fused Adam step (sparse=True, OptimType.ADAM)
  dense_fused    what a script does without it: sparse=False backward (dense core gradients to autograd) and
                 torch.optim.Adam(fused=True).step() over the cores
  dense_foreach  the same with torch.optim.Adam(foreach=True)
Per leg: GPU ms (HIP events around the step, median over --iters) and host enqueue microseconds (a host clock around the
same calls, which return before the kernels finish; median).  Prints one JSON line; --out writes it as a file.  Launch
counts come from a separate `rocprofv3 --kernel-trace --stats` run with --only LEG."""
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
ROWS, D = 2449029, 100
LEGS = ("sgd", "adam", "dense_fused", "dense_foreach")


def _module(opt, sparse):
    torch.manual_seed(0)
    return TTEmbeddingBag(ROWS, D, R, P, Q, optimizer=opt, sparse=sparse, use_cache=False, weight_dist="normal",
                          learning_rate=1e-6, eps=1e-8)


def _legs(n, only):
    rng = np.random.default_rng(n)
    ids = torch.as_tensor(rng.integers(0, ROWS, size=n)).cuda()
    offs = torch.arange(n + 1, device="cuda")
    dy = torch.randn(n, D, device="cuda") * 1e-3
    legs = {}
    if "sgd" in only:
        m = _module(OptimType.SGD, True)
        legs["sgd"] = lambda m=m: m(ids, offs).backward(dy)
    if "adam" in only:
        m = _module(OptimType.ADAM, True)
        legs["adam"] = lambda m=m: m(ids, offs).backward(dy)
    for name, kw in (("dense_fused", {"fused": True}), ("dense_foreach", {"foreach": True})):
        if name in only:
            m = _module(OptimType.SGD, False)
            opt = torch.optim.Adam(m.parameters(), lr=1e-6, **kw)

            def step(m=m, opt=opt):
                m(ids, offs).backward(dy)
                opt.step()
                opt.zero_grad(set_to_none=True)
            legs[name] = step
    return legs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--sizes", type=int, nargs="+", default=[409600, 2048])
    ap.add_argument("--only", nargs="+", default=list(LEGS), choices=LEGS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "adam_bench.py measures on a ROCm device"
    res = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "sizes": {}}
    for n in a.sizes:
        legs = _legs(n, a.only)
        for fn in legs.values():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        ev = {k: [] for k in legs}
        host = {k: [] for k in legs}
        for _ in range(a.iters):   # alternate the legs, one timed step each
            for k, fn in legs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record()
                fn()
                e1.record()
                host[k].append(time.perf_counter() - t0)
                ev[k].append((e0, e1))
        torch.cuda.synchronize()
        res["sizes"][str(n)] = {
            k: {"gpu_ms": round(float(np.median([x.elapsed_time(y) for x, y in ev[k]])), 4),
                "host_enqueue_us": round(float(np.median(host[k])) * 1e6, 1)} for k in legs}
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
