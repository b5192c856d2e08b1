"""What a learning-rate schedule costs a captured step, on the products table (p = 125.140.140, q = 4.5.5, r = 16.16) with
fused SGD and fused ADAM, one training step (forward + backward with its update) of n unique ids in bags of one, n = 2 048
and 409 600, the rate changing on EVERY step (a warm-up / cosine schedule):
  device_word   a capturable=True module: emb.set_learning_rate(lr) and the replay of ONE captured pair of graphs; the
                module writes the new rate into its device word with one fill_ per step
  recapture     a plain module: emb.set_learning_rate(lr), emb.capture(n, n) again (a synchronise, a warm-up launch and two
                graph captures), then the replay -- all the parent offers a schedule
  constant      a plain module at a constant rate: the captured step before this change, the floor of device_word
One process; the legs alternate in blocks of --steps steps.  Per block: host_us = time to enqueue the block / steps (no
synchronisation inside a block beyond what a leg does itself), wall_us = time until the device has finished it / steps.
Reported: the median over --rounds blocks.  The first failure ends the run.  Prints one JSON line; --out writes it as a
JSON file."""
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
    ap.add_argument("--steps", type=int, default=20, help="steps per block")
    ap.add_argument("--rounds", type=int, default=5, help="blocks per leg")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows, D = 2_449_029, int(np.prod(Q))
    dev = "cuda"
    rng = np.random.default_rng(0)
    res = {"device": torch.cuda.get_device_name(0), "steps_per_block": a.steps, "rounds": a.rounds, "results": {}}
    for opt in (OptimType.SGD, OptimType.ADAM):
        def module(**kw):
            torch.manual_seed(0)
            return TTEmbeddingBag(rows, D, R, P, Q, optimizer=opt, learning_rate=1e-6, use_cache=False, weight_dist="normal", **kw)

        for n in SIZES:
            ids = torch.as_tensor(rng.choice(rows, size=n, replace=False).astype(np.int64)).to(dev)
            dy = torch.randn(n, D, device=dev) * 1e-3
            word, plain, const = module(capturable=True), module(), module()
            cap_word, cap_const = word.capture(n, n), const.capture(n, n)
            tick = [0]

            def rate():   # a new float every step
                tick[0] += 1
                return 1e-6 * (1.0 + 1e-3 * (tick[0] % 1000))

            def device_word():
                word.set_learning_rate(rate())
                cap_word(ids).backward(dy)

            def recapture():
                plain.set_learning_rate(rate())
                plain.capture(n, n)(ids).backward(dy)

            legs = {"device_word": device_word, "recapture": recapture, "constant": lambda: cap_const(ids).backward(dy)}
            for fn in legs.values():
                for _ in range(a.warmup):
                    fn()
            torch.cuda.synchronize()
            graphs = (cap_word.fwd_graph, cap_word.bwd_graph)
            host = {k: [] for k in legs}
            wall = {k: [] for k in legs}
            for _ in range(a.rounds):
                for k, fn in legs.items():
                    steps = max(1, a.steps // 4) if k == "recapture" else a.steps   # (milliseconds per step: fewer of them)
                    t0 = time.perf_counter()
                    for _ in range(steps):
                        fn()
                    t1 = time.perf_counter()
                    torch.cuda.synchronize()
                    t2 = time.perf_counter()
                    host[k].append((t1 - t0) / steps * 1e6)
                    wall[k].append((t2 - t0) / steps * 1e6)
            assert (cap_word.fwd_graph, cap_word.bwd_graph) == graphs   # the device-word leg re-captured nothing
            med = lambda v: round(float(np.median(v)), 1)
            res["results"][f"{opt.value}_{n}"] = {
                "wall_us": {k: med(v) for k, v in wall.items()},
                "host_us": {k: med(v) for k, v in host.items()},
                "device_word_vs_constant_wall": round(float(np.median(wall["device_word"]) / np.median(wall["constant"])), 3),
                "recapture_vs_device_word_wall": round(float(np.median(wall["recapture"]) / np.median(wall["device_word"])), 1),
            }
            del word, plain, const, cap_word, cap_const, legs
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
