"""padding_idx against what it replaces, on the products table (p = 125.140.140, q = 4.5.5, r = 16.16): a fixed-fanout
neighbour table of 40 960 destinations x fanout 10 with about 30 % pad ids, all cases alternating in one process, each timed
with HIP events around one training step (forward + fused SGD backward):
  padded_sum / padded_mean     the 2-D call emb(table) with padding_idx: the partition route (pad ids never reach the TT
                               kernels)
  csr_sum / csr_mean           the same neighbours without the pads as a 1-D CSR call (the pads dropped on the host, once,
                               outside the timed steps)
  masked_sum / masked_mean     the padded 2-D call forced onto the masked-rows route (every id looked up as a bag of one,
                               pads weighted 0)
Prints one JSON line (median ms over --iters steps after --warmup); --out writes it as a JSON file too.  Kernel times come
from a separate `rocprofv3 --kernel-trace --stats` run of the same command."""
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
    pad = rows - 1
    rng = np.random.default_rng(0)
    dev = "cuda"
    nbr = rng.integers(0, rows - 1, size=(N_DST, FANOUT))
    deg = rng.integers(1, FANOUT + 1, size=N_DST)   # nodes with fewer neighbours than the fanout are filled with the pad
    deg[rng.random(N_DST) < 0.35] = FANOUT
    nbr[np.arange(FANOUT)[None, :] >= deg[:, None]] = pad
    table = torch.as_tensor(nbr).to(dev)
    keep = nbr != pad
    csr_ids = torch.as_tensor(nbr[keep]).to(dev)
    csr_offs = torch.as_tensor(np.concatenate([[0], np.cumsum(keep.sum(1))])).to(dev)
    mods = {}
    for mode in ("sum", "mean"):
        for padded in (True, False):
            torch.manual_seed(0)
            mods[mode, padded] = TTEmbeddingBag(rows, D, R, P, Q, optimizer=OptimType.SGD, learning_rate=1e-6,
                                                use_cache=False, weight_dist="normal", mode=mode,
                                                padding_idx=pad if padded else None)
    masked = {}
    for mode in ("sum", "mean"):
        torch.manual_seed(0)
        masked[mode] = TTEmbeddingBag(rows, D, R, P, Q, optimizer=OptimType.SGD, learning_rate=1e-6, use_cache=False,
                                      weight_dist="normal", mode=mode, padding_idx=pad)
        masked[mode]._pad_partition = False
    dy = torch.randn(N_DST, D, device=dev) * 1e-3
    cases = {}
    for mode in ("sum", "mean"):
        cases[f"padded_{mode}"] = (lambda m=mods[mode, True]: m(table).backward(dy))
        cases[f"csr_{mode}"] = (lambda m=mods[mode, False]: m(csr_ids, csr_offs).backward(dy))
        cases[f"masked_{mode}"] = (lambda m=masked[mode]: m(table).backward(dy))
    for fn in cases.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    routes = {k: m._last_pad_route for k, m in (("padded", mods["sum", True]), ("masked", masked["sum"]))}
    ev = {k: [] for k in cases}
    for _ in range(a.iters):   # alternate the cases, one timed step each
        for k, fn in cases.items():
            ev[k].append(_timed(fn))
    torch.cuda.synchronize()
    ms = {k: float(np.median([x.elapsed_time(y) for x, y in v])) for k, v in ev.items()}
    res = {
        "device": torch.cuda.get_device_name(0), "iters": a.iters, "dst": N_DST, "fanout": FANOUT,
        "ids": N_DST * FANOUT, "kept_ids": int(csr_ids.numel()), "pad_share": round(1 - csr_ids.numel() / (N_DST * FANOUT), 3),
        "routes": routes, "step_ms": {k: round(v, 4) for k, v in ms.items()},
        "padded_vs_csr": {m: round(ms[f"padded_{m}"] / ms[f"csr_{m}"], 3) for m in ("sum", "mean")},
        "padded_vs_masked": {m: round(ms[f"padded_{m}"] / ms[f"masked_{m}"], 3) for m in ("sum", "mean")},
    }
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
