#!/usr/bin/env python3
"""Headline benchmark: TT-embedding lookups/sec on the ogbn-products configuration
(BASELINE.json configs[1]: p=[125,140,140], q=[4,5,5], r=[16,16], batch 2048).

A "step" is one pass of the hot path over one mini-batch: TTEmbeddingBag.forward on the
batch's frontier ids plus its backward with the SGD update of the TT cores -- what
sage_dgl_partition.py:train() makes the layer do per iteration.  The frontier of a
2048-seed batch with fan-out [5,10,15] is 10^5..10^6 unique ids; the
workload uses 409 600 = 2048 x 200 unique uniform ids, bag length 1, as DGL delivers them.

  python bench.py --gpus 1 --steps 50 --warmup 10
  python bench.py --gpus 1 --steps 50 --warmup 10 --dump-outputs DIR   (also writes the last timed step's outputs)
  python bench.py --gpus 1 --steps 50 --warmup 10 --full               (also every other leg: roofline, CPU baselines, ...)
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

N > 1 is data parallel (weak scaling): every rank looks up its own batch, the flattened
core gradients are summed with one RCCL all-reduce, then the fused SGD epilogue runs.
Rank 0 prints ONE JSON line.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for _p in (ROOT, os.path.join(ROOT, "falcon-ttdforgnns_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

P, Q, RANKS, N_EMB, D = [125, 140, 140], [4, 5, 5], [16, 16], 2449029, 100
F0 = 2 * Q[0] * RANKS[0] * Q[1] * RANKS[1]          # stage-1 GEMM flops per lookup
F1 = 2 * Q[0] * Q[1] * RANKS[1] * Q[2]              # stage-2 GEMM flops per lookup
FWD_FLOPS, BWD_FLOPS = F0 + F1, 3 * F0 + 2 * F1     # 13 440 / 37 120
PEAK_F32_MFMA_TFLOPS = 157.3                        # MI355X_MICROARCH.md, chip-level parameters
PEAK_HBM_GBS = 8000.0


def _launch_ranks(n):
    """`python bench.py --gpus N` without a launcher: run the same command line under torch.distributed.run."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC: RCCL across processes needs it on this driver
    env.setdefault("OMP_NUM_THREADS", "4")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.run(cmd, env=env).returncode


def spread(ms):
    """min / median / max (+ the two largest) of per-step times in ms: what tells a slow box from a few slow steps."""
    a = np.sort(np.asarray(ms, dtype=np.float64))
    return {"min": round(float(a[0]), 4), "median": round(float(np.median(a)), 4), "max": round(float(a[-1]), 4),
            "p90": round(float(a[int(0.9 * (len(a) - 1))]), 4), "n": int(len(a))}


def timed_steps(fn, n, before=None, after=None):
    """n steps between two host fences: wall clock per step, and the GPU's own clock -- one HIP event on the compute stream
    at every step boundary (torch's current stream is the stream the library launches on), so the line can tell host from
    GPU and a slow step from a slow box.  `before` / `after`: fences (after() runs before the last event is read)."""
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
    if before is not None:
        before()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    evs[0].record()
    for i in range(n):
        fn(i)
        evs[i + 1].record()
    if after is not None:
        after()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    per = [evs[i].elapsed_time(evs[i + 1]) for i in range(n)]
    return wall, per, evs[0].elapsed_time(evs[n])


SHAPES = {   # name -> (p, q, ranks, num_embeddings)
    "products_r16": ([125, 140, 140], [4, 5, 5], [16, 16], 2449029),
    "papers100M_r32": ([500, 560, 400], [8, 4, 4], [32, 32], 111059956),
    "arxiv_r8": ([56, 60, 51], [4, 4, 8], [8, 8], 169343),
}


# the reference's rank sweep (run_script.sh:250-288): the products table with q = 5,5,4 at ranks 8 ... 256 and q = 4,4,8 at
# 64 ... 256 -- ranks up to 32 run on the register-resident grouped chain, 64 and up on the wide-rank one (GEMM prefix,
# per-group backward, GEMM dG1 / dG0)
RANK_SWEEP = [([5, 5, 4], r) for r in (8, 16, 32, 64, 128, 256)] + [([4, 4, 8], r) for r in (64, 128, 256)]

# the keys of the legs `--full` adds to the line (full_legs)
FULL_LEGS = ("roofline", "cpu_baseline", "cpu_baseline_2048", "matrix", "papers_roofline", "rank_sweep", "batch2048_step",
             "metis_like_step", "dp_mode_1gpu", "cache_on_step", "sage_epoch")


def matrix_leg(nat, name, n_ids, dist_kind, iters=50):
    """One row of the §8d matrix at the C-ABI level (cores resident, buffers reused): forward only, dense backward,
    fused-SGD backward and forward + fused backward, median of `iters` HIP-event timings on the compute stream."""
    p, q, ranks, n_emb = SHAPES[name] if isinstance(name, str) else name
    R = [1] + ranks + [1]
    D = int(np.prod(q))
    rng = np.random.default_rng(5)
    if dist_kind == "arange":
        ids = np.arange(n_ids, dtype=np.int64) % n_emb
    else:
        ids = rng.choice(n_emb, size=n_ids, replace=False).astype(np.int64)
    shape = nat.make_shape(p, q, R)
    cores = [torch.from_numpy((rng.standard_normal((p[t], R[t] * q[t] * R[t + 1])) * 0.05).astype(np.float32)).cuda()
             for t in range(3)]
    idx, offs = torch.from_numpy(ids).cuda(), torch.arange(n_ids + 1, dtype=torch.int64, device="cuda")
    out = torch.empty(n_ids, D, device="cuda")
    d_out = (torch.rand(n_ids, D, device="cuda") - 0.5) * 0.1
    grads = [torch.empty_like(c) for c in cores]
    ws = nat.Workspace()
    plan = nat.new_plan(shape, n_ids, idx.device)
    fwd = lambda: nat.forward(shape, cores, idx, None, offs, n_ids, None, n_ids, out, ws, plan)
    fwd_inference = lambda: nat.forward(shape, cores, idx, None, offs, n_ids, None, n_ids, out, ws, None)   # no plan kept
    bwd_dense = lambda: nat.backward_dense(shape, cores, idx, None, n_ids, None, n_ids, d_out, grads, ws, plan, offs)
    bwd_sgd = lambda: nat.backward_sgd(shape, cores, idx, None, n_ids, None, n_ids, d_out, 1e-12, ws, plan, offs)

    def both():
        fwd()
        bwd_sgd()

    def med(fn):
        for _ in range(5):
            fn()
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
        for a, b in evs:
            a.record()
            fn()
            b.record()
        torch.cuda.synchronize()
        return float(np.median([a.elapsed_time(b) for a, b in evs])) * 1e3   # us

    def in_step():
        """forward and fused backward ALTERNATING, as a training step runs them, ONE event between the two calls: each chain's
        time with the caches in the state the other one leaves them (a backward repeated on its own keeps its 167 MB of
        gradient rows in the 256 MB memory-side cache: 103 us against ~118 in the step)."""
        for _ in range(5):
            both()
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
               for _ in range(iters)]
        for a, b, c in evs:
            a.record()
            fwd()
            b.record()
            bwd_sgd()
            c.record()
        torch.cuda.synchronize()
        return (float(np.median([a.elapsed_time(b) for a, b, c in evs])) * 1e3, float(np.median([b.elapsed_time(c) for a, b, c in evs])) * 1e3)

    fwd()   # the plan the backward legs reuse
    r = {"ids": n_ids, "ids_kind": dist_kind, "fwd_us": round(med(fwd), 1), "bwd_dense_us": round(med(bwd_dense), 1),
         "bwd_fused_sgd_us": round(med(bwd_sgd), 1), "fwd_bwd_sgd_us": round(med(both), 1)}
    r["fwd_in_step_us"], r["bwd_in_step_us"] = (round(x, 1) for x in in_step())
    r["fwd_inference_us"] = round(med(fwd_inference), 1)   # (a forward nobody's backward follows: what the module runs under no_grad)
    r["fwd_lookups_per_s"] = round(n_ids / (r["fwd_us"] * 1e-6), 1)
    r["fwd_bwd_lookups_per_s"] = round(n_ids / (r["fwd_bwd_sgd_us"] * 1e-6), 1)
    return r


def papers_roofline_leg(nat, n_ids=819200, iters=20):
    """BASELINE.json configs[4]'s table on ONE GPU (p = 500,560,400, q = 8,4,4, ranks 32,32; SURVEY.md section 8d cfg-E):
    the chain is priced against the fp32 MFMA peak (141.8 flop/B nominal, far past the ridge).  Kernel times are HIP-event
    brackets inside the library (live); HBM traffic and MFMA-busy come from committed counter passes of the same workload."""
    p, q, ranks, n_emb = SHAPES["papers100M_r32"]
    R = [1] + ranks + [1]
    Dp = int(np.prod(q))
    rng = np.random.default_rng(5)
    ids = rng.choice(n_emb, size=n_ids, replace=False).astype(np.int64)
    groups = int(np.unique(ids // p[2]).shape[0])   # (i0, i1) prefixes the frontier touches: P is formed once per group
    f0 = 2 * q[0] * ranks[0] * q[1] * ranks[1]
    f1 = 2 * q[0] * q[1] * ranks[1] * q[2]
    shape = nat.make_shape(p, q, R)
    cores = [torch.from_numpy((rng.standard_normal((p[t], R[t] * q[t] * R[t + 1])) * 0.05).astype(np.float32)).cuda() for t in range(3)]
    idx, offs = torch.from_numpy(ids).cuda(), torch.arange(n_ids + 1, dtype=torch.int64, device="cuda")
    out = torch.empty(n_ids, Dp, device="cuda")
    d_out = (torch.rand(n_ids, Dp, device="cuda") - 0.5) * 0.1
    ws, plan = nat.Workspace(), nat.new_plan(shape, n_ids, idx.device)
    t = {k: [] for k in ("group", "fwd", "bwd", "chunk", "epi", "fin")}
    for it in range(iters + 3):
        if it == 3:
            nat.profile_enable(True)
        nat.forward(shape, cores, idx, None, offs, n_ids, None, n_ids, out, ws, plan)
        nat.backward_sgd(shape, cores, idx, None, n_ids, None, n_ids, d_out, 1e-12, ws, plan, offs)
        if it >= 3:
            for k, slot in (("group", 3), ("fwd", 0), ("bwd", 1), ("chunk", 2), ("epi", 8), ("fin", 9)):
                try:
                    t[k].append(nat.profile_read(slot))
                except RuntimeError:   # no epilogue launch: the chunk kernel formed the group products itself (GROUP_PRODUCTS_IN_CHAIN)
                    t[k].append(0.0)
    nat.profile_enable(False)
    torch.cuda.synchronize()
    m = {k: float(np.median(v)) for k, v in t.items()}   # ms
    # the two calls' own times: forward and backward alternating as above with the library's brackets OFF, one HIP event
    # between the calls (the brackets put six event packets into every backward: ~10-25 us on a ~1 ms chain; `kernel_ms` keeps them)
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
           for _ in range(iters)]
    for a, b, c in evs:
        a.record()
        nat.forward(shape, cores, idx, None, offs, n_ids, None, n_ids, out, ws, plan)
        b.record()
        nat.backward_sgd(shape, cores, idx, None, n_ids, None, n_ids, d_out, 1e-12, ws, plan, offs)
        c.record()
    torch.cuda.synchronize()
    fwd_ms = float(np.median([a.elapsed_time(b) for a, b, c in evs]))
    bwd_ms = float(np.median([b.elapsed_time(c) for a, b, c in evs]))
    bracket_fwd_ms, bracket_bwd_ms = m["group"] + m["fwd"], m["bwd"]
    nominal_f, nominal_b = n_ids * (f0 + f1), n_ids * (3 * f0 + 2 * f1)
    executed_f = groups * f0 + n_ids * f1                 # P once per group
    executed_b = groups * 2 * f0 + n_ids * 2 * f1         # dG0 / dG1 products per group, dP / E per id (P is the forward's)
    tfl = lambda fl, ms: fl / (ms * 1e-3) / 1e12
    fam = nat.kernel_family(shape, n_ids, n_ids)
    r = {"bound": "mfma", "kernel_family": int(fam), "group_products_in_chunk_kernel": bool(fam & nat.FAMILY_GROUP_PRODUCTS_IN_CHAIN),
         "workload": "papers100M r32 (p = 500,560,400 q = 8,4,4), %d unique uniform ids on one GPU, fwd + fused-SGD bwd at the C ABI" % n_ids,
         "groups_touched": groups, "ids_per_group": round(n_ids / groups, 2),
         "kernel_ms": {k: round(v, 4) for k, v in m.items()},
         "fwd_ms_incl_grouping": round(fwd_ms, 4), "bwd_ms": round(bwd_ms, 4),
         "timing": "fwd / bwd: HIP events around the two C-ABI calls alternating as in a training step, library brackets off "
                   "(median of %d); kernel_ms / *_from_brackets: the library's own brackets (ttemb_profile_read), which add event packets" % iters,
         "fwd_ms_from_brackets": round(bracket_fwd_ms, 4), "bwd_ms_from_brackets": round(bracket_bwd_ms, 4),
         "peak": PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s",
         "fwd_nominal_tflops": round(tfl(nominal_f, fwd_ms), 2), "fwd_executed_tflops": round(tfl(executed_f, fwd_ms), 2),
         "bwd_nominal_tflops": round(tfl(nominal_b, bwd_ms), 2), "bwd_executed_tflops": round(tfl(executed_b, bwd_ms), 2),
         "achieved": round(tfl(executed_f + executed_b, fwd_ms + bwd_ms), 2),
         "frac": round(tfl(executed_f + executed_b, fwd_ms + bwd_ms) / PEAK_F32_MFMA_TFLOPS, 4),
         "frac_nominal": round(tfl(nominal_f + nominal_b, fwd_ms + bwd_ms) / PEAK_F32_MFMA_TFLOPS, 4),
         "algorithmic_hbm_bytes": n_ids * 2 * (8 + 4 * Dp)}
    for key, src in (("traffic", "profiles/r05_papers_traffic.json"), ("mfma_busy", "profiles/r05_papers_mfma_util.json")):
        try:
            with open(os.path.join(ROOT, src)) as fh:
                kern = json.load(fh)["kernels"]
            r[key] = {k: (v["hbm_bytes"] if key == "traffic" else v["mfma_util"]) for k, v in kern.items()}
            r[key + "_source"] = src
        except (OSError, KeyError, ValueError):
            r[key] = None
    return r


def ref_papers_invocation_leg(n_ids=819200, steps=12):
    """The reference's own papers100M run (run_script.sh:408-431): p = 400,500,600, q = 4,4,8, ranks 16,16, --sparse,
    --use-cached --cache-size 5 (gnn_model.py:98-100: 5 % of the nodes cached, hash table of num_nodes slots), batch 4096.
    One step = forward + backward with the fused update through the class with the cache LIVE; frontiers are 200-id
    windows with Zipf-distributed starts (cfg-C's generator) so that the cache has something to hit."""
    from FBTT.tt_embeddings_ops import TTEmbeddingBag
    p, q, r, n_emb, Dp = [400, 500, 600], [4, 4, 8], [16, 16], 111059956, 128
    rng = np.random.default_rng(9)
    n_win = n_emb // 200
    hot_win = rng.choice(n_win, size=40000, replace=False)   # 8 M ids' worth of recurring windows

    def frontier():
        k = n_ids // 200
        st = np.concatenate([rng.choice(hot_win, size=k // 2, replace=False), rng.choice(n_win, size=k - k // 2, replace=False)])
        st = np.unique(st)
        return torch.from_numpy((st[:, None] * 200 + np.arange(200)[None, :]).reshape(-1).astype(np.int64)).cuda()

    emb = TTEmbeddingBag(n_emb, Dp, r, p, q, sparse=True, use_cache=True, cache_size=int(0.05 * n_emb), hashtbl_size=n_emb,
                         weight_dist="normal", learning_rate=0.01, batch_count=14000)
    for _ in range(8):
        emb.update_cache(frontier())
    emb.cache_populate()
    test = [frontier() for _ in range(4)]
    keys = emb.hashtbl[emb.cache_state >= 0]
    hit = float(np.mean([float(torch.isin(b, keys).float().mean()) for b in test[:2]]))
    del keys
    times = []
    for i in range(steps + 3):
        b = test[i % len(test)]
        offs = torch.arange(b.numel() + 1, dtype=torch.int64, device="cuda")
        d = torch.full((b.numel(), Dp), 1e-3, device="cuda")
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        emb(b, offs).backward(d)
        torch.cuda.synchronize()
        if i >= 3:
            times.append(time.perf_counter() - t1)
    dt = float(np.median(times))
    n = int(np.mean([b.numel() for b in test]))
    res = {"what": "run_script.sh:408-431 (final-papers): p = 400,500,600 q = 4,4,8 ranks 16,16, sparse, LFU cache 5 % live; "
                   "fwd + bwd + fused update through the class, host-timed per step (sync on both sides)",
           "ids": n, "ms_per_step": round(dt * 1e3, 4), "lookups_per_s": round(n / dt, 1), "hit_rate": round(hit, 3),
           "cache_rows": int(emb.cache_weight.shape[0]), "hash_slots": int(emb.hashtbl.numel())}
    del emb
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--ids", type=int, default=409600, help="frontier ids per step per GPU")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also measure everything else the line reports (~45 s more): the roofline, the "
                         "CPU baselines, the batch-2048, METIS-like, data-parallel and cache-on steps, the SAGE epoch, the "
                         "matrix, the papers100M roofline and the rank sweep.  Without it those keys read null")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baselines")
    ap.add_argument("--no-extras", action="store_true",
                    help="with --full: skip the legs on other workloads, keep the roofline and the CPU baselines "
                         "(keeps a rocprofv3 summary to the headline workload)")
    ap.add_argument("--path", default="auto", choices=["auto", "generic", "fast3"])
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed as DIR/<name>.npy (float32): "
                         "a fixed seeded sample of the rows of its forward output, and the TT cores after its update")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # started plainly (`python bench.py --gpus N`): the ranks are fresh child processes, one per GPU, started
        # through torch.distributed.run BEFORE this process has touched the GPU (no HIP call has been made yet; a
        # process that has initialised the GPU must never be replaced or forked).  The launcher's rank 0 prints the
        # JSON line; this parent only relays its exit code.
        sys.exit(_launch_ranks(args.gpus))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher set WORLD_SIZE={world}")
    assert torch.cuda.is_available(), "bench.py needs a ROCm device (no CPU fallback)"
    # rehearsal of the N > 1 code path on a one-GPU box: TTEMB_BENCH_REHEARSAL=1 puts every rank on GPU 0 and
    # carries the all-reduce over gloo (RCCL needs one GPU per rank).  Never used for reported numbers.
    rehearsal = os.environ.get("TTEMB_BENCH_REHEARSAL") == "1"
    if rehearsal:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if rehearsal:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world,
                                    device_id=torch.device("cuda", local_rank))

    import ttemb_native as nat
    from FBTT.tt_embeddings_ops import TTEmbeddingBag
    from ttemb_dist import TTDataParallel
    nat.set_path({"auto": nat.PATH_AUTO, "generic": nat.PATH_GENERIC, "fast3": nat.PATH_FAST3}[args.path])

    torch.manual_seed(1234)
    N = args.ids
    emb = TTEmbeddingBag(N_EMB, D, RANKS, P, Q, sparse=(world == 1), use_cache=False, weight_dist="normal",
                         learning_rate=0.01, batch_count=N)
    dp = TTDataParallel(emb) if world > 1 else None
    if dp is not None:
        dp.broadcast_parameters(0)
    # every step updates the cores and the pre-warm below runs for a wall-clock budget: the timed steps start again from
    # these initial cores, so that what they compute depends on the arguments only
    init_cores = [c.detach().clone() for c in emb.tt_cores]
    rng = np.random.default_rng(2 + rank)
    n_sets = 4  # rotate a few frontiers so that no step re-reads the previous step's ids
    id_sets = [torch.from_numpy(rng.choice(N_EMB, size=N, replace=False).astype(np.int64)).cuda()
               for _ in range(n_sets)]
    offsets = torch.arange(N + 1, dtype=torch.int64, device="cuda")
    d_out = ((torch.rand(N, D, device="cuda") - 0.5) * 0.1)

    def step(i):
        out = emb(id_sets[i % n_sets], offsets)
        out.backward(d_out)
        if dp is not None:
            dp.step(overlap=True)   # the all-reduce runs under the next forward's grouping pass
        return out

    def fence():
        if dp is not None:
            dp.flush()              # the last step's update belongs to the timed region
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    # untimed pre-warm: the driver's --warmup 5 is ~1 ms of GPU work straight after minutes of host-side set-up (id generation,
    # the first import of torch) -- clocks, the allocator's block lists and the workspace are cold.  At least 0.3 s of the
    # headline step, untimed, before the warm-up steps the driver asked for (which stay the driver's)
    t_pw = time.perf_counter()
    n_pw = 0
    while True:
        for i in range(20):
            step(n_pw + i)
        n_pw += 20
        if dp is not None:
            dp.flush()
        torch.cuda.synchronize()
        more = time.perf_counter() - t_pw < 0.3
        if world > 1:   # every rank leaves the loop after the same round: the ranks that want more are counted
            go = torch.tensor([1.0 if more else 0.0], device="cpu" if rehearsal else "cuda")
            dist.all_reduce(go)
            more = float(go.item()) > 0.0
        if not more:
            break
    prewarm_s = time.perf_counter() - t_pw
    for i in range(args.warmup):
        step(i)
    fence()
    with torch.no_grad():
        for c, c0 in zip(emb.tt_cores, init_cores):
            c.copy_(c0)
    fence()
    ev_a, ev_b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    step_evs = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps)]
    last_out = None
    t0 = time.perf_counter()
    ev_a.record()
    for i in range(args.steps):
        if i == args.steps - 1:
            last_out = step(i)
        else:
            step(i)
        step_evs[i].record()
    if dp is not None:
        dp.flush()              # the last step's update belongs to the timed region
    ev_b.record()
    fence()
    elapsed = time.perf_counter() - t0
    gpu_ms = ev_a.elapsed_time(ev_b)   # the same region on the GPU's clock (first launch .. last kernel's end)
    step_gpu_ms = [(ev_a if i == 0 else step_evs[i - 1]).elapsed_time(step_evs[i]) for i in range(args.steps)]
    if args.dump_outputs and rank == 0:
        # the whole forward output is N x D floats (164 MB at the default N): a fixed seeded sample of its rows
        rows = np.sort(np.random.default_rng(0).choice(N, size=min(N, 65536), replace=False))
        dump = {"forward_out_rows": last_out.detach()[torch.from_numpy(rows).cuda()]}
        dump.update({f"tt_core{t}": c.detach() for t, c in enumerate(emb.tt_cores)})
        os.makedirs(args.dump_outputs, exist_ok=True)
        for name, a in dump.items():
            np.save(os.path.join(args.dump_outputs, name + ".npy"), a.float().cpu().numpy())
    del last_out
    dist_info = None
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device="cpu" if rehearsal else "cuda")
        every = [torch.zeros_like(t) for _ in range(world)]
        dist.all_gather(every, t)
        elapsed = max(float(x.item()) for x in every)   # MAX over ranks
        dist_info = {"backend": dist.get_backend(), "world_size": dist.get_world_size(),
                     "ms_per_step_by_rank": [round(float(x.item()) / args.steps * 1e3, 4) for x in every],
                     "devices": torch.cuda.device_count(), "rehearsal_on_one_gpu": rehearsal}
    value = world * N * args.steps / elapsed

    # everything else the line reports, after the timed steps; a plain run leaves it out (those keys read null)
    legs = dict.fromkeys(FULL_LEGS)
    if args.full:
        legs = full_legs(args, nat, emb, step, fence, rng, id_sets, offsets, d_out, world, rank)

    result = None
    if rank == 0:
        result = {
            "metric": "tt_embedding_lookups_per_sec", "value": round(value, 1), "unit": "lookups/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 4),
            "ms_per_step_gpu_events": round(gpu_ms / args.steps, 4), "step_gpu_ms": spread(step_gpu_ms),
            "prewarm_s": round(prewarm_s, 3), "prewarm_steps": n_pw, "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": "ogbn-products TTEmbeddingBag fwd+bwd+SGD per step, frontier of a "
                                   "2048-seed batch = 409600 unique uniform ids per GPU, bag length 1",
                       "p": P, "q": Q, "tt_ranks": RANKS, "num_embeddings": N_EMB, "ids_per_gpu_step": N,
                       "parallelism": f"dp{world}", "kernel_path": args.path},
            "dist": dist_info, "full": args.full, **legs,
        }
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        print(json.dumps(result))


def full_legs(args, nat, emb, step, fence, rng, id_sets, offsets, d_out, world, rank):
    """Everything `--full` adds to the line, run after the headline's timed steps: the roofline (ten more headline steps
    with the library's kernel brackets on, and the chain timed at the C ABI), the CPU baselines and the legs on other
    workloads.  Returns them under their keys in the line (None: a leg that --no-extras, --no-cpu-baseline or the world
    size leaves out) on rank 0, {} on the other ranks."""
    from FBTT.tt_embeddings_ops import TTEmbeddingBag
    from ttemb_dist import TTDataParallel
    N, n_sets = args.ids, len(id_sets)
    # roofline leg: kernels bracketed by HIP events on the stream they are launched on.
    # slot 0 = forward chain kernel, slot 2 = backward chunk kernel, slot 1 = all backward chain kernels,
    # slot 3 = grouping pass (counting sort + chunk table + prefix-product kernel).  Nominal work per
    # lookup: forward F0 + F1 = 13 440 flop, backward 3 F0 + 2 F1 = 37 120 flop, 408 B each
    # way (8 B id + one D-float row).  The chunk kernel's own share is the two per-id GEMMs of the backward
    # (dP and the dG2 rows: 2 F1 = 6 400 flop) over 408 algorithmic bytes = 15.7 flop/B, under the
    # fp32-MFMA ridge (157.3 TF / 8 TB/s = 19.7): it is priced against HBM.
    # Every rank runs these steps (they contain the collective); rank 0 reports its own kernel times.
    nat.profile_enable(True)
    fwd_ms, bwd_ms, chunk_ms, group_ms, epi_ms, fin_ms = [], [], [], [], [], []
    def read_slot(slot):   # (kernel families without that kernel record no bracket: not a failure of the bench)
        try:
            return nat.profile_read(slot)
        except RuntimeError:
            return float("nan")

    for i in range(10):
        step(i)
        fwd_ms.append(nat.profile_read(0))
        bwd_ms.append(nat.profile_read(1))
        chunk_ms.append(nat.profile_read(2))
        group_ms.append(nat.profile_read(3))
        epi_ms.append(read_slot(8))
        fin_ms.append(read_slot(9))
    nat.profile_enable(False)
    fence()

    legs = {}
    if rank == 0:
        fwd, bwd, chunk = float(np.mean(fwd_ms)), float(np.mean(bwd_ms)), float(np.mean(chunk_ms))
        group = float(np.mean(group_ms))
        row_bytes = 8 + 4 * D
        if chunk >= fwd:
            dom_name, dom_ms, dom_flops = "fast3_bwd_chunk_kernel", chunk, 2 * F1
        else:
            dom_name, dom_ms, dom_flops = "fast3_forward_kernel", fwd, F1
        achieved = N * row_bytes / (dom_ms * 1e-3) / 1e9
        # HBM bytes per launch of that kernel from the committed PMC passes (FETCH_SIZE / WRITE_SIZE cannot be read from
        # inside the process): NOT measured by this run -- the files are named in the line -- valid for the default workload
        traffic_src, busy_src = "profiles/r05_traffic.json", "profiles/r05_mfma_util.json"
        traffic = None
        try:
            if N == 409600 and args.path == "auto":
                with open(os.path.join(ROOT, traffic_src)) as fh:
                    traffic = json.load(fh)["kernels"][dom_name]["hbm_bytes"]
        except (OSError, KeyError, ValueError):
            traffic = None
        mfma_busy = None   # MFMA-pipe busy fraction of that kernel from the committed PMC pass (tools/mfma_util.sh)
        try:
            if N == 409600 and args.path == "auto":
                with open(os.path.join(ROOT, busy_src)) as fh:
                    mfma_busy = json.load(fh)["kernels"][dom_name]["mfma_util"]
        except (OSError, KeyError, ValueError):
            mfma_busy = None
        tf = lambda flops, ms: N * flops / (ms * 1e-3) / 1e12
        # Chain-level figures are taken from calls WITHOUT inner brackets: the forward (grouping + prefix products + lookup: four
        # launches) and the fused backward (three) at the C ABI, alternating as a step runs them, one HIP event between the two.  The brackets above put an
        # event record in front of and behind every kernel -- two or three more packets between launches that run back to back
        # otherwise: their sum overstates the chain by 3-9 us depending on the box (`*_bracket_ms` keep those sums).
        chain = matrix_leg(nat, "products_r16", N, "uniform", iters=30) if (world == 1 and N == 409600 and args.path == "auto") else None
        fwd_chain_ms = chain["fwd_in_step_us"] * 1e-3 if chain else fwd + group
        bwd_chain_ms = chain["bwd_in_step_us"] * 1e-3 if chain else bwd
        roofline = {"bound": "hbm", "kernel": dom_name, "achieved": round(achieved, 1),
                    "peak": PEAK_HBM_GBS, "unit": "GB/s",
                    "frac": round(achieved / PEAK_HBM_GBS, 4), "traffic": traffic,
                    "traffic_source": traffic_src if traffic is not None else None,
                    "kernel_mfma_busy_source": busy_src if mfma_busy is not None else None,
                    "kernel_does": ("dP and dG2-row products of the backward AND the dG2 reduction (fused; no E table)"
                                    if dom_name == "fast3_bwd_chunk_kernel" else "stage-2 product and row stores"),
                    "kernel_ms": round(dom_ms, 4), "algorithmic_bytes_per_lookup": row_bytes,
                    "kernel_flops_per_lookup": dom_flops,
                    "kernel_mfma_frac": round(tf(dom_flops, dom_ms) / PEAK_F32_MFMA_TFLOPS, 4),
                    "kernel_mfma_busy_pmc": mfma_busy,
                    "traffic_gbs": None if traffic is None else round(traffic / (dom_ms * 1e-3) / 1e9, 1),
                    "fwd_kernel_ms": round(fwd, 4), "bwd_chunk_kernel_ms": round(chunk, 4),
                    "bwd_chain_ms": round(bwd, 4), "grouping_ms": round(group, 4),
                    "bwd_epilogue_kernel_ms": None if np.isnan(epi_ms).any() else round(float(np.mean(epi_ms)), 4),
                    "bwd_finalize_kernel_ms": None if np.isnan(fin_ms).any() else round(float(np.mean(fin_ms)), 4),
                    # chain level, nominal flops (executed flops are lower: P is formed once per group)
                    "chain_times_from": ("C-ABI calls alternating as in a step, one event between forward (incl. grouping and prefix products) and fused-SGD backward, median of 30"
                                         if chain else "sums of the per-kernel brackets"),
                    "fwd_chain_ms": round(fwd_chain_ms, 4), "bwd_chain_call_ms": round(bwd_chain_ms, 4),
                    "fwd_chain_bracket_ms": round(fwd + group, 4),
                    "fwd_chain_nominal_tflops": round(tf(FWD_FLOPS, fwd_chain_ms), 3),
                    "fwd_chain_mfma_frac": round(tf(FWD_FLOPS, fwd_chain_ms) / PEAK_F32_MFMA_TFLOPS, 4),
                    "fwd_chain_mfma_frac_from_brackets": round(tf(FWD_FLOPS, fwd + group) / PEAK_F32_MFMA_TFLOPS, 4),
                    "bwd_chain_nominal_tflops": round(tf(BWD_FLOPS, bwd_chain_ms), 3),
                    "bwd_chain_mfma_frac": round(tf(BWD_FLOPS, bwd_chain_ms) / PEAK_F32_MFMA_TFLOPS, 4),
                    # the whole chain contraction, forward + backward, charged with the grouping pass as well
                    "chain_nominal_tflops": round(tf(FWD_FLOPS + BWD_FLOPS, fwd_chain_ms + bwd_chain_ms), 3),
                    "chain_mfma_frac": round(tf(FWD_FLOPS + BWD_FLOPS, fwd_chain_ms + bwd_chain_ms) / PEAK_F32_MFMA_TFLOPS, 4),
                    "fwd_row_store_gbs": round(N * row_bytes / (fwd * 1e-3) / 1e9, 1),
                    "peak_f32_mfma_tflops": PEAK_F32_MFMA_TFLOPS}
        # latency regime of the metric's "batch 2048": 2048 unique ids per step (sparse batch -> generic
        # wave-per-id kernels), same fwd + bwd + SGD step through the class
        small = None
        if world == 1 and not args.no_extras:
            ids_s = torch.from_numpy(rng.choice(N_EMB, size=2048, replace=False).astype(np.int64)).cuda()
            offs_s = torch.arange(2049, dtype=torch.int64, device="cuda")
            d_s = d_out[:2048]
            for _ in range(20):
                emb(ids_s, offs_s).backward(d_s)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(200):
                emb(ids_s, offs_s).backward(d_s)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t1) / 200
            # the same step as ONE captured graph (forward + backward + update under torch.cuda.graph: the layer does not
            # synchronise or allocate outside torch's allocator, so a caller can capture its whole training step)
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                emb(ids_s, offs_s).backward(d_s)
            for _ in range(20):
                gr.replay()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(500):
                gr.replay()
            torch.cuda.synchronize()
            dtg = (time.perf_counter() - t1) / 500
            cap = emb.capture(2048, 2048)   # forward / backward as two graph replays behind the autograd bridge
            for _ in range(20):
                cap(ids_s).backward(d_s)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(200):
                cap(ids_s).backward(d_s)
            torch.cuda.synchronize()
            dtc = (time.perf_counter() - t1) / 200
            # the headline of this leg is the EAGER figure: the reference's drivers run the layer unchanged, i.e. eager;
            # the captured forms are reported next to it
            small = {"ids": 2048, "us_per_step": round(dt * 1e6, 1), "lookups_per_s": round(2048 / dt, 1),
                     "whole_step_graph_replay_us": round(dtg * 1e6, 1),
                     "whole_step_graph_lookups_per_s": round(2048 / dtg, 1),
                     "capture_api_us_per_step": round(dtc * 1e6, 1),
                     "what": "fwd + bwd + SGD on 2048 unique ids through the class (per-bag MFMA kernels: 4 launches); "
                             "us_per_step = eager; whole_step_graph_replay_us = the same step under one torch.cuda.graph"}
        # the same step on a frontier with METIS-like id locality (2048 windows of 200 consecutive ids:
        # what `--partition 125` reordering produces, SURVEY.md §8d cfg-B3), reported next to the uniform one
        local = None
        if world == 1 and not args.no_extras:
            starts = rng.choice(N_EMB // 200 - 1, size=(N + 199) // 200, replace=False) * 200
            ids_l = torch.from_numpy((starts[:, None] + np.arange(200)[None, :]).reshape(-1)[:N].astype(np.int64)).cuda()
            for _ in range(5):
                emb(ids_l, offsets).backward(d_out)
            wall, per, gpu = timed_steps(lambda i: emb(ids_l, offsets).backward(d_out), 20)
            dt = wall / 20
            local = {"ids": N, "ms_per_step": round(dt * 1e3, 4), "lookups_per_s": round(N / dt, 1),
                     "ms_per_step_gpu_events": round(gpu / 20, 4), "step_gpu_ms": spread(per)}
        # The step N > 1 runs, on ONE GPU: dense gradients straight into the flat bucket, TTDataParallel.step (no collective at
        # world 1), one fused SGD launch over the flat weights -- so that a multi-GPU value divides by a like-for-like
        # single-GPU one (the headline N = 1 line is the fused in-backward update: a different step)
        dp1 = None
        if world == 1 and not args.no_extras:
            emb_d = TTEmbeddingBag(N_EMB, D, RANKS, P, Q, sparse=False, use_cache=False, weight_dist="normal",
                                   learning_rate=0.01, batch_count=N)
            dp_d = TTDataParallel(emb_d)

            def dstep(i):
                emb_d(id_sets[i % n_sets], offsets).backward(d_out)
                dp_d.step(overlap=True)

            for i in range(10):
                dstep(i)
            wall, per, gpu = timed_steps(dstep, 100, before=dp_d.flush, after=dp_d.flush)
            dt = wall / 100
            dp1 = {"ids": N, "ms_per_step": round(dt * 1e3, 4), "lookups_per_s": round(N / dt, 1),
                   "ms_per_step_gpu_events": round(gpu / 100, 4), "step_gpu_ms": spread(per),
                   "what": "the data-parallel step at world size 1: sparse=False, gradients into the bucket, "
                           "TTDataParallel.step(overlap=True), fused SGD over the flat weights, no collective; "
                           "the like-for-like N = 1 for `--gpus N` values (which run this step plus one all-reduce)"}
            del dp_d, emb_d
        # BASELINE.json configs[2]: the same step with the LFU row cache live (10 % of the rows cached, frontiers of
        # 200-id windows whose starts follow a Zipf law so that hot regions recur -- SURVEY.md §8d cfg-C), after a
        # counting epoch and cache_populate(); the hit rate is reported next to the step time
        cached = None
        if world == 1 and not args.no_extras:
            n_win = N_EMB // 200
            zp = 1.0 / np.arange(1, n_win + 1) ** 1.05
            zp /= zp.sum()
            perm = rng.permutation(n_win)

            def frontier():
                st = perm[rng.choice(n_win, size=N // 200, replace=False, p=zp)] * 200
                return torch.from_numpy((st[:, None] + np.arange(200)[None, :]).reshape(-1).astype(np.int64)).cuda()

            cemb = TTEmbeddingBag(N_EMB, D, RANKS, P, Q, sparse=True, use_cache=True, cache_size=int(0.1 * N_EMB),
                                  hashtbl_size=N_EMB, weight_dist="normal", learning_rate=0.01, batch_count=N)
            for _ in range(96):
                cemb.update_cache(frontier())
            cemb.cache_populate()
            test = [frontier() for _ in range(24)]
            keys = cemb.hashtbl[cemb.cache_state >= 0]
            hit = float(np.mean([float(torch.isin(b, keys).float().mean()) for b in test[:4]]))
            for b in test[:4]:
                cemb(b, offsets).backward(d_out)
            wall, per, gpu = timed_steps(lambda i: cemb(test[i], offsets).backward(d_out), len(test))
            dt = wall / len(test)
            cached = {"ids": N, "ms_per_step": round(dt * 1e3, 4), "lookups_per_s": round(N / dt, 1),
                      "ms_per_step_gpu_events": round(gpu / len(test), 4), "step_gpu_ms": spread(per),
                      "cache_rows": int(cemb.cache_weight.shape[0]), "hit_rate": round(hit, 3)}
            # the same frontiers through the cache-less module: what the cache is up against.  Per-step GPU times and the
            # per-step wall clock of the host side of every step (a step the host took long to enqueue shows in both)
            for b in test[:4]:
                emb(b, offsets).backward(d_out)
            host_us = []

            def off_step(i):
                th = time.perf_counter()
                emb(test[i], offsets).backward(d_out)
                host_us.append((time.perf_counter() - th) * 1e6)

            wall, per, gpu = timed_steps(off_step, len(test))
            dt_off = wall / len(test)
            cached["cache_off_same_frontiers_ms"] = round(dt_off * 1e3, 4)
            cached["cache_off_gpu_events_ms"] = round(gpu / len(test), 4)
            cached["cache_off_step_gpu_ms"] = spread(per)
            cached["cache_off_host_enqueue_us"] = spread(host_us)
            # ... and once more with the library's own brackets: the grouping pass of every step (profile slot 3)
            nat.profile_enable(True)
            grp = []
            for b in test:
                emb(b, offsets).backward(d_out)
                grp.append(nat.profile_read(3))
            nat.profile_enable(False)
            cached["cache_off_grouping_ms"] = spread(grp)
            # HBM-bound gather / update kernels of the cached rows and the two kernels every id pays, timed LIVE (HIP-event
            # brackets inside the library, profile slots 4-7) over the same frontiers.  Algorithmic bytes per cached row:
            # forward 8 + 4 + 4 D read + 4 D written = 812 B, backward 8 + 4 + 4 D gradient + 4 D row read + 4 D written = 1 212 B
            nat.profile_enable(True)
            kt = {4: [], 5: [], 6: [], 7: []}
            hits = []
            for b in test[:12]:
                cemb(b, offsets).backward(d_out)
                for slot in kt:
                    kt[slot].append(nat.profile_read(slot))
                hits.append(float(torch.isin(b, keys).float().mean()))
            nat.profile_enable(False)
            rows = float(np.mean(hits)) * N
            kern = {}
            for slot, name, bpr in ((6, "cached_row_gather", 8 + 4 + 8 * D), (7, "cached_row_update", 8 + 4 + 12 * D)):
                us = float(np.median(kt[slot])) * 1e3
                gbs = rows * bpr / (us * 1e-6) / 1e9
                kern[name] = {"avg_us": round(us, 1), "bytes_per_cached_row": bpr, "gbs": round(gbs, 1),
                              "frac_of_hbm_peak": round(gbs / PEAK_HBM_GBS, 3)}
            for slot, name in ((4, "probe_pass_with_lfu_update"), (5, "partition_scatter")):
                kern[name] = {"avg_us": round(float(np.median(kt[slot])) * 1e3, 1), "what": "per id of the batch, cached or not"}
            cached["kernels"] = kern
            cached["kernels_source"] = "live: HIP events around the kernels in this run (ttemb_profile_read slots 4-7), 12 steps"
            # A cached row moves 2 024 B of HBM traffic per step (forward + update) and takes one more probe than a TT row,
            # whose marginal cost on this hardware is lower (the TT step grows by ~0.34 ns per id, the cached rows' two
            # kernels cost ~0.56 ns per row at the 3.1-3.6 TB/s random 400-byte rows sustain): no hit rate pays for the cache
            # at this TT speed.  It is served for interface parity (BASELINE configs[2]), not for speed.
            cached["break_even_hit_rate"] = None
            cached["break_even_note"] = ("none: marginal cost of a cached row (gather + update kernels) exceeds that of a TT row "
                                         "at every hit rate on MI355X; see DESIGN.md section 5c")
            del cemb
        # second half of BASELINE.json's metric: SAGE epoch time on the products shapes.  DGL / OGB are not in the
        # image, so the epoch is tools/sage_epoch.py's restatement of sage_dgl_partition.py:train() around the TT
        # layer (synthetic 2.45 M-node graph, fan-out 5/10/15, batch 2048, 3 mean-SAGE layers in stock PyTorch,
        # 196 615 train nodes = 97 steps); the second epoch is reported
        epoch = None
        if world == 1 and not args.no_extras:
            sys.path.insert(0, os.path.join(ROOT, "tools"))
            import sage_epoch
            ea = argparse.Namespace(nodes=N_EMB, avg_degree=25, locality=0.5, train_nodes=196615, batch=2048,
                                    fan_out="5,10,15", hidden=256, classes=47, emb="tt", epochs=2, max_steps=0)
            epoch = sage_epoch.run(ea, quiet=True)
            epoch["what"] = ("synthetic graph + sampler + 3 mean-SAGE layers in stock PyTorch around TTEmbeddingBag "
                             "(tools/sage_epoch.py), second epoch; eval_*: the drivers' evaluation pass over the embedding "
                             "layer -- every node, 2^20 ids per call, under no_grad")
        cpu, cpu2048 = None, None
        if world == 1 and not args.no_cpu_baseline:
            from oracle import cpu_einsum
            n_cpu = 65536
            # the port does not scale with threads (one thread is within 10 % of all of them, and past ~8 threads small
            # batches get slower): the baseline is the BEST of {1, 8, all} threads, the thread count is reported
            all_thr = os.cpu_count() or 1
            tries = {}
            for thr in sorted({1, 8, all_thr}):
                tries[thr] = cpu_einsum.time_baseline(P, Q, [1] + RANKS + [1], n_cpu, N_EMB, seed=1234, budget_s=6.0, threads=thr)
            best_thr = max(tries, key=lambda k: tries[k]["lookups_per_s"])
            r = tries[best_thr]
            cpu = {"value": round(r["lookups_per_s"], 1), "unit": "lookups/s", "cores": best_thr,
                   "kind": "port",
                   "by_threads": {str(k): round(v["lookups_per_s"], 1) for k, v in tries.items()},
                   "sample": f"{r['iters']} fwd+bwd+SGD steps of {n_cpu} unique uniform ids "
                             f"(torch index_select+einsum, fp32, {r['seconds']:.1f} s at {best_thr} threads; "
                             f"best of 1 / 8 / {all_thr} threads, ~6 s each)"}
            # the metric's literal regime: N = 2048, at 1 / 8 / all host threads (the best is the baseline to beat), and
            # the 65 536-id sample on one thread
            by_thr = {}
            for thr in sorted({1, 8, all_thr}):
                rr = cpu_einsum.time_baseline(P, Q, [1] + RANKS + [1], 2048, N_EMB, seed=1234, budget_s=2.5, threads=thr)
                by_thr[str(thr)] = round(rr["lookups_per_s"], 1)
            torch.set_num_threads(all_thr)
            best = max(by_thr.values())
            cpu["one_thread_value"] = round(tries[1]["lookups_per_s"], 1)
            # BASELINE.json configs[0] (the reference's own CPU-runnable case): ogbn-arxiv shapes, batch 256, einsum on the
            # host.  The product has no CPU path (a CPU fallback would void parity), so this leg exists on the baseline
            # side only; its GPU counterpart is matrix["arxiv_r8_256"].
            pa, qa, ra, na = SHAPES["arxiv_r8"]
            rr = cpu_einsum.time_baseline(pa, qa, [1] + ra + [1], 256, na, seed=1234, budget_s=2.0, threads=8)
            torch.set_num_threads(all_thr)
            cpu["arxiv_r8_batch256"] = {"value": round(rr["lookups_per_s"], 1), "unit": "lookups/s", "cores": 8,
                                        "sample": "fwd+bwd+SGD steps of 256 unique ids, ~2 s"}
            cpu2048 = {"value": best, "unit": "lookups/s", "by_threads": by_thr, "kind": "port",
                       "sample": "fwd+bwd+SGD steps of 2048 unique uniform ids, ~2.5 s per thread count",
                       "gpu_over_cpu": None if small is None else round(small["lookups_per_s"] / best, 1)}
        matrix = None
        if world == 1 and not args.no_extras:
            matrix = {"how": "C-ABI calls, cores resident, buffers reused, median of 50 HIP-event timings (us)",
                      "products_r16_409600": chain if chain is not None else matrix_leg(nat, "products_r16", 409600, "uniform"),
                      "products_r16_2048": matrix_leg(nat, "products_r16", 2048, "uniform"),
                      "papers100M_r32_819200": matrix_leg(nat, "papers100M_r32", 819200, "uniform", iters=20),
                      "papers100M_r32_4096": matrix_leg(nat, "papers100M_r32", 4096, "uniform"),
                      "arxiv_r8_full_graph": matrix_leg(nat, "arxiv_r8", 169343, "arange"),
                      "arxiv_r8_256": matrix_leg(nat, "arxiv_r8", 256, "uniform"),
                      "papers100M_ref_q448_r16_cache5_819200": ref_papers_invocation_leg()}
        papers = None
        if world == 1 and not args.no_extras:
            papers = papers_roofline_leg(nat)
        sweep = None
        if world == 1 and not args.no_extras:
            sweep = {"how": "products table (p = 125,140,140), 409600 unique uniform ids, C-ABI calls as in `matrix`, median of 10"}
            for qs, r in RANK_SWEEP:
                sweep["q%s_r%d" % ("".join(str(x) for x in qs), r)] = matrix_leg(
                    nat, (SHAPES["products_r16"][0], qs, [r, r], N_EMB), 409600, "uniform", iters=10)
                torch.cuda.empty_cache()
        legs = {"roofline": roofline, "cpu_baseline": cpu, "cpu_baseline_2048": cpu2048, "matrix": matrix,
                "papers_roofline": papers, "rank_sweep": sweep, "batch2048_step": small, "metis_like_step": local,
                "dp_mode_1gpu": dp1, "cache_on_step": cached, "sage_epoch": epoch}
    return legs


if __name__ == "__main__":
    main()
