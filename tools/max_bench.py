"""Max bags against what they replace, on the products table (p = 125.140.140, q = 4.5.5, r = 16.16): a fixed-fanout neighbour
table of 40 960 destinations x fanout 10 (409 600 ids), plain and with about 29 % pad ids (the table of
tools/padding_bench.py), all legs alternating in one process, each timed with HIP events around one training step (forward +
fused SGD backward):
  max / max_padded                      the call emb(nbr, mode="max") (with padding_idx: the partition route)
  two_step / two_step_padded            what a user writes without it: the bags-of-one lookup of every id, then
                                        F.embedding_bag(mode="max"[, padding_idx]) over the rows (torch's kernels, an
                                        [nnz, D] gradient filled by its scatter)
  gcn                                   the GCN-weighted sum of DESIGN 4.7 on the same ids: the same rows route with a sum
  copy_rows_buffer                      a device-to-device copy of the rows buffer (164 MB), the bandwidth yardstick
Prints one JSON line (median ms over --iters steps after --warmup) with the bytes each new kernel has to move per call
(from the shapes; divide by the kernel times of a `rocprofv3 --kernel-trace --stats` run of the same command).  --out writes
it as a JSON file."""
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
N_DST, FANOUT = 40_960, 10


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    return a, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows, D = int(np.prod(P)), int(np.prod(Q))
    nnz = N_DST * FANOUT
    pad = rows - 1
    rng = np.random.default_rng(0)
    dev = "cuda"
    nbr_np = rng.integers(0, rows - 1, size=(N_DST, FANOUT))
    padded_np = nbr_np.copy()
    deg = rng.integers(1, FANOUT + 1, size=N_DST)   # nodes with fewer neighbours than the fanout are filled with the pad
    deg[rng.random(N_DST) < 0.35] = FANOUT
    padded_np[np.arange(FANOUT)[None, :] >= deg[:, None]] = pad
    nbr, nbr_pad = torch.as_tensor(nbr_np).to(dev), torch.as_tensor(padded_np).to(dev)

    def module(padding_idx=None):
        torch.manual_seed(0)
        return TTEmbeddingBag(rows, D, R, P, Q, optimizer=OptimType.SGD, learning_rate=1e-6, use_cache=False,
                              weight_dist="normal", padding_idx=padding_idx)

    plain, padded = module(), module(pad)
    ones = torch.arange(nnz + 1, device=dev)
    csr = torch.arange(0, nnz + 1, FANOUT, device=dev)
    local = torch.arange(nnz, device=dev)
    gcn = torch.as_tensor(rng.random(nnz).astype(np.float32)).to(dev)
    dy = torch.randn(N_DST, D, device=dev) * 1e-3
    src = torch.empty(nnz, D, device=dev)
    dst = torch.empty_like(src)

    def two_step():
        r = plain(nbr.reshape(-1), ones)
        return F.embedding_bag(local, r, csr, mode="max", include_last_offset=True)

    # the two-step baseline with pads: torch compares padding_idx with the row numbers it is given, so the rows get one extra
    # (zero) row that every pad position points at (the map is built once, outside the timed steps)
    is_pad = (nbr_pad.reshape(-1) == pad)
    local_pad = torch.where(is_pad, torch.full_like(local, nnz), local)

    def two_step_padded():
        r = plain(nbr_pad.reshape(-1), ones)
        r = torch.cat([r, r.new_zeros(1, D)])
        return F.embedding_bag(local_pad, r, csr, mode="max", include_last_offset=True, padding_idx=nnz)

    cases = {
        "max": lambda: plain(nbr, mode="max").backward(dy),
        "two_step": lambda: two_step().backward(dy),
        "gcn": lambda: plain(nbr, per_sample_weights=gcn.view(N_DST, FANOUT)).backward(dy),
        "max_padded": lambda: padded(nbr_pad, mode="max").backward(dy),
        "two_step_padded": lambda: two_step_padded().backward(dy),
        "copy_rows_buffer": lambda: dst.copy_(src),
    }
    for fn in cases.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    route = padded._last_pad_route
    ev = {k: [] for k in cases}
    for _ in range(a.iters):   # alternate the legs, one timed step each
        for k, fn in cases.items():
            ev[k].append(_timed(fn))
    torch.cuda.synchronize()
    ms = {k: float(np.median([x.elapsed_time(y) for x, y in v])) for k, v in ev.items()}
    f4, i4, i8 = 4, 4, 8
    rows_b, out_b = nnz * D * f4, N_DST * D * f4
    res = {
        "device": torch.cuda.get_device_name(0), "iters": a.iters, "ids": nnz, "bags": N_DST, "D": D,
        "pad_share": round(float(is_pad.float().mean()), 3), "padded_route": route,
        "step_ms": {k: round(v, 4) for k, v in ms.items()},
        "max_vs_two_step": round(ms["max"] / ms["two_step"], 3),
        "max_padded_vs_two_step_padded": round(ms["max_padded"] / ms["two_step_padded"], 3),
        "max_vs_gcn": round(ms["max"] / ms["gcn"], 3),
        "copy_GBps": round(2 * rows_b / ms["copy_rows_buffer"] / 1e6, 1),
        # bytes a kernel has to move per call (reads + writes), from the shapes
        "kernel_bytes": {
            "bag_max_kernel": rows_b + (N_DST + 1) * i8 + out_b + N_DST * D * i4,
            "bag_max_backward_kernel": out_b + N_DST * D * i4 + (N_DST + 1) * i8 + rows_b,
        },
    }
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
