"""MI355X-native Tensor-Train embedding bag -- drop-in for the reference's
``FBTT.tt_embeddings_ops`` (same import path, class names, constructor arguments,
attributes and state_dict keys; reference: FBTT/tt_embeddings_ops.py:432-965).

What differs is everything underneath: the lookups, gradients, optimiser epilogues
and the LFU row cache run in ``libttemb_hip.so`` (hand-written HIP for gfx950,
C ABI in ``include/ttemb.h``) through ``ttemb_native``.  There is no
``batch_count`` chunking (the argument is accepted and ignored: partial products
never leave the chip), and no host synchronisation in ``forward`` -- the split
between TT-computed and cached ids stays on the device.

Every call form goes through one front end: ``_prepare`` (the argument checks, in one order for every form, before anything
is launched; ids and offsets as the kernels read them; the LFU statistics; the exact-mode decision) and ``_route`` (the
effective mode, ``padding_idx`` and the weights pick the lookup and the pooling around it).  Several tables are either
windows the kernels read on the device or one host split (``_each_table``); dense gradients of every autograd bridge are
delivered by ``_deliver_dense``.

No CPU fallback exists: modules can be *constructed* without a GPU (so that shape
logic, initialisers and checkpoints can be exercised anywhere) but ``forward`` on
CPU tensors raises ``RuntimeError``.
"""
from __future__ import annotations

import gc
import logging
import math
import warnings
from enum import Enum, unique
from typing import List, Optional, Sequence

import numpy as np
import torch
from torch import nn

import ttemb_native as _nat

__all__ = ["OptimType", "BufferList", "tt_matrix_to_full", "suggested_tt_shapes", "TTLookupFunction",
           "TableBatchedTTEmbeddingBag", "TTEmbeddingBag", "CapturedLookup", "CapturedBags"]

_LOG = logging.getLogger(__name__)


@unique
class OptimType(Enum):
    """Optimiser selector; value strings match the reference (tt_embeddings_ops.py:18-33).
    SGD / EXACT_SGD run the fused in-backward SGD; ADAM runs the fused Adam / AdamW step (below); everything else runs
    fused Adagrad, as the reference dispatches (:229-286).  EXACT_SGD also turns on exact mode, the reference's documented
    meaning ("deterministic updates (via sorting + segment reduction)", :20-23): see ``_ExactLookup``.

    ADAM (the reference has the member and runs Adagrad for it) is DENSE Adam, ``torch.optim.Adam`` /
    ``torch.optim.AdamW`` (``decoupled_weight_decay=True``) on the dense core gradients, without amsgrad: every element of
    every core moves on every applied step, also rows no id of the call touches -- the "untouched rows stay bit-identical"
    property of fused SGD / Adagrad does not hold for it.  The step count lives on the device (``adam_step``); a call
    without ids is a no-op that does not advance it.  DESIGN.md §4.9."""
    SGD = "sgd"
    EXACT_SGD = "exact_sgd"
    LAMB = "lamb"
    ADAM = "adam"
    EXACT_ADAGRAD = "exact_adagrad"
    EXACT_ROWWISE_ADAGRAD = "exact_row_wise_adagrad"
    LARS_SGD = "lars_sgd"
    PARTIAL_ROWWISE_ADAM = "partial_row_wise_adam"
    PARTIAL_ROWWISE_LAMB = "partial_row_wise_lamb"

    def __str__(self) -> str:
        return self.value


_SGD_LIKE = (OptimType.SGD, OptimType.EXACT_SGD)


def _step_call(m: "TableBatchedTTEmbeddingBag", table: int = 0) -> "_nat.Step":
    """The fused step of a backward on table ``table``: the rate (a capturable module: its device word, else the float), eps,
    ``state`` (None for SGD, the Adagrad state or Adam's first moment) and for Adam the second moment, the table's device
    step words and the hyper-parameters."""
    lr, eps = m._lr_arg(), float(m.eps)
    if m.optimizer in _SGD_LIKE:
        return _nat.Step(lr, eps)
    state = _nat.core_ptrs(m._states(), table)
    if m.optimizer != OptimType.ADAM:
        return _nat.Step(lr, eps, state)
    v, step0, hp = m._adam_lean()
    return _nat.Step(lr, eps, state, (_nat.core_ptrs(v, table), step0 if table == 0 else m.adam_step[table], hp))


class BufferList(nn.Module):
    """Ordered list of registered buffers named ``<name>0, <name>1, ...`` so that
    state_dict keys read ``optimizer_state.optimizer_state0`` like the reference's
    (tt_embeddings_ops.py:36-77)."""

    def __init__(self, name: str, buffers: Optional[Sequence[torch.Tensor]] = None) -> None:
        super().__init__()
        self._name = name
        self._length = 0
        for b in buffers or ():
            self.append(b)

    def append(self, buffer: torch.Tensor) -> "BufferList":
        self.register_buffer(f"{self._name}{self._length}", buffer)
        self._length += 1
        return self

    def extend(self, buffers: Sequence[torch.Tensor]) -> "BufferList":
        for b in buffers:
            self.append(b)
        return self

    def __len__(self) -> int:
        return self._length

    def __getitem__(self, index: int) -> torch.Tensor:
        if not -self._length <= index < self._length:
            raise IndexError(index)
        return getattr(self, f"{self._name}{index % self._length}")

    def __iter__(self):
        return (self[i] for i in range(self._length))


def _pad_ranks(tt_ranks: Sequence[int], T: int) -> List[int]:
    r = [int(x) for x in tt_ranks]
    return [1] + r + [1] if len(r) == T - 1 else r


def tt_matrix_to_full(tt_p_shapes: Sequence[int], tt_q_shapes: Sequence[int], tt_ranks: Sequence[int],
                      tt_cores: Sequence[torch.Tensor],
                      tt_permute: Optional[Sequence[int]] = None) -> torch.Tensor:
    """Dense ``[prod(p), prod(q)]`` table of a TT matrix (differentiable, any device).

    Same contract as the reference helper (tt_embeddings_ops.py:80-127): with
    ``tt_permute=[1, 0, 2, 3]`` core ``t`` is stored ``[p_t, R_t, q_t, R_{t+1}]``
    (the layer's layout); with ``None`` cores are already ``[R_t, p_t, q_t, R_{t+1}]``.
    """
    T = len(tt_p_shapes)
    R = _pad_ranks(tt_ranks, T)
    table = None
    for t, core in enumerate(tt_cores):
        dims = [R[t], int(tt_p_shapes[t]), int(tt_q_shapes[t]), R[t + 1]]
        if tt_permute is not None:
            stored = [dims[a] for a in tt_permute]
            g = core.reshape(stored).permute(*tt_permute)
        else:
            g = core.reshape(dims)
        # table: [P, Q, R_t] ; g: [R_t, p, q, R_{t+1}]  ->  [P, p, Q, q, R_{t+1}]
        if table is None:
            table = g.reshape(dims[1], dims[2], dims[3])
        else:
            P, Q = table.shape[0], table.shape[1]
            nxt = torch.tensordot(table, g, dims=([2], [0]))  # [P, Q, p, q, R]
            table = nxt.permute(0, 2, 1, 3, 4).reshape(P * dims[1], Q * dims[2], dims[3])
    return table.reshape(table.shape[0], table.shape[1]).float()


# --------------------------------------------------------------------------------------
# shape suggestion (reference: tt_embeddings_ops.py:369-429; sympy-free re-derivation)
# --------------------------------------------------------------------------------------
def _prime_factors(n: int) -> List[int]:
    out, f = [], 2
    while f * f <= n:
        while n % f == 0:
            out.append(f)
            n //= f
        f += 1 if f == 2 else 2
    if n > 1:
        out.append(n)
    return out


def _unordered_factorisations(n: int, d: int, lo: int = 2):
    """All non-decreasing d-tuples of integers >= lo with product n."""
    if d == 1:
        if n >= lo:
            yield (n,)
        return
    f = lo
    while f ** d <= n:
        if n % f == 0:
            for rest in _unordered_factorisations(n // f, d - 1, f):
                yield (f,) + rest
        f += 1


def _shape_entropy(factors: Sequence[int]) -> float:
    tot = float(sum(factors))
    return -sum((f / tot) * math.log(f / tot) for f in factors)


def _interleave(sorted_factors: Sequence[int]) -> List[int]:
    half = len(sorted_factors) // 2
    lo, hi = list(sorted_factors[:half]), list(sorted_factors[half:])
    out = []
    for i in range(len(hi)):
        if i < len(lo):
            out.append(lo[i])
        out.append(hi[i])
    return out


def _most_even_shape(n: int, d: int) -> List[int]:
    primes = _prime_factors(n)
    if len(primes) <= d:
        cands = [tuple(sorted(primes + [1] * (d - len(primes))))]
    else:
        cands = sorted(set(_unordered_factorisations(n, d)))
    best = max(cands, key=_shape_entropy)
    return _interleave(best)


def suggested_tt_shapes(n: int, d: int = 3, allow_round_up: bool = True) -> List[int]:
    """Factor ``n`` (optionally rounded up to a multiple of a power of ten) into ``d``
    factors that are as even as possible (maximum entropy of the normalised factors)."""
    n = int(n)
    if not allow_round_up:
        return _most_even_shape(n, d)
    best, best_h = None, -1.0
    for k in range(len(str(n))):
        step = 10 ** k
        shape = _most_even_shape(-(-n // step) * step, d)
        h = _shape_entropy(shape)
        if h > best_h + 1e-15:
            best, best_h = shape, h
    return best


# --------------------------------------------------------------------------------------
# autograd bridge
# --------------------------------------------------------------------------------------
def _f32(t: torch.Tensor) -> torch.Tensor:
    """The incoming gradient as the kernels read it: contiguous float32."""
    if t.dtype != torch.float32 or not t.is_contiguous():
        t = t.contiguous().float()
    return t


def _aligned(t: torch.Tensor) -> torch.Tensor:
    """``_f32`` at a 16-byte address: what the bag kernels' float4 accesses need (a gradient can arrive as a view)."""
    t = _f32(t)
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _deliver_dense(m: "TableBatchedTTEmbeddingBag", table: int, use_bucket: bool, run, into_grad: bool = False):
    """Dense core gradients of one table, for every bridge: ``run(dst)`` is the native backward writing one [p, row]
    gradient per core into the tensors ``dst``.  A data-parallel wrapper may have provided one flat bucket for them
    (``ttemb_dist``, ``_dense_grad_out``); where the bridge may use it (``use_bucket``) they are produced straight into it and
    nothing is handed to autograd (no AccumulateGrad, no views): returns None.  Else returns one gradient per
    [num_tables, p, row] parameter -- or, ``into_grad`` (a bridge without the cores among its inputs), adds them to ``.grad``."""
    bucket = m._dense_grad_out
    if bucket is not None and use_bucket:
        if m._bucket_filled:
            # a second backward before dp.step() (micro-batches, two lookups through one module): the kernels overwrite
            # their destination, so this one goes to scratch and is added -- what AccumulateGrad does
            more = [torch.empty_like(b) for b in bucket]
            run(more)
            torch._foreach_add_(bucket, more)
        else:
            run(bucket)
            m._bucket_filled = True
        return None
    # (a bucket the bridge may not fill on its own -- a live cache, whose cache_weight gradient goes through autograd --
    #  still receives the gradients: autograd then hands the wrapper views of it)
    grads = bucket or [torch.empty_like(c[table]) for c in m.tt_cores]
    run(grads)
    if m.num_tables == 1:
        full = [g.unsqueeze(0) for g in grads]
    else:  # only this table's slice of the [num_tables, p, row] parameter gets gradient
        full = [torch.zeros_like(c.data) for c in m.tt_cores]
        for z, g in zip(full, grads):
            z[table] = g
    if into_grad:
        for c, g in zip(m.tt_cores, full):
            c.grad = g if c.grad is None else c.grad + g
        return None
    return full


class TTLookupFunction(torch.autograd.Function):
    """forward = TT rows (+ cached rows) bag-summed; backward = fused optimiser step
    (``sparse``) or dense core gradients.  Reference: tt_embeddings_ops.py:130-366."""

    @staticmethod
    def forward(ctx, module: "TableBatchedTTEmbeddingBag", table: int, B: int, indices: torch.Tensor,
                rowidx: torch.Tensor, offsets: Optional[torch.Tensor], nnz_dev: Optional[torch.Tensor],
                cache_loc: Optional[torch.Tensor], cache_weight: Optional[torch.Tensor],
                *tt_cores: torch.Tensor) -> torch.Tensor:
        ctx.module, ctx.table, ctx.B = module, table, B
        ctx.live_cache = cache_loc is not None
        # integer inputs, never differentiated: kept on ctx directly (save_for_backward costs version bookkeeping)
        ctx.inputs = (indices, rowidx, nnz_dev, cache_loc, offsets)
        cores = _nat.core_ptrs(tt_cores, table)
        nnz = indices.numel()
        out = torch.empty((B, module.embedding_dim), dtype=torch.float32, device=indices.device)
        # the forward's grouping of the ids is kept for the backward of this very call
        ctx.plan = _nat.new_plan(module._shape, nnz, indices.device)
        pending = getattr(module, "_before_weights", None)
        if pending is None:
            _nat.forward(module._shape, cores, indices, rowidx, offsets, nnz, nnz_dev, B, out, module._ws, ctx.plan)
        else:
            # something still has to write the cores (ttemb_dist.TTDataParallel: the previous step's all-reduce +
            # update): the id-only half of the forward is enqueued first so that it overlaps with it
            if ctx.plan is not None:
                _nat.forward(module._shape, cores, indices, rowidx, offsets, nnz, nnz_dev, B, out, module._ws, ctx.plan,
                             phase=1)
            pending()
            _nat.forward(module._shape, cores, indices, rowidx, offsets, nnz, nnz_dev, B, out, module._ws, ctx.plan,
                         phase=2 if ctx.plan is not None else 0)
        if ctx.live_cache and nnz > 0:
            _nat.cache_forward(cache_loc, rowidx, 0, nnz_dev, nnz, cache_weight.data, out, offsets)
        return out

    @staticmethod
    def backward(ctx, d_output: torch.Tensor):
        m, table, B = ctx.module, ctx.table, ctx.B
        indices, rowidx, nnz_dev, cache_loc, offsets = ctx.inputs
        nnz = indices.numel()
        d_output = _f32(d_output)
        cores = _nat.core_ptrs(m.tt_cores, table)
        n_fixed = 9
        cached = ctx.live_cache and nnz > 0
        if m.sparse:
            step = _step_call(m, table)
            _nat.backward_fused(m._shape, cores, indices, rowidx, nnz, nnz_dev, B, d_output, step, m._ws, ctx.plan, offsets)
            if cached and step.state is None:   # (never Adam with a live cache: the constructor refuses that combination)
                _nat.cache_backward_sgd(cache_loc, rowidx, 0, nnz_dev, nnz, d_output, step.lr, m.cache_weight.data,
                                        nnz_dev[1:] if nnz_dev.numel() > 1 else None)
            elif cached:
                _nat.cache_backward_rowwise_adagrad(cache_loc, rowidx, 0, nnz_dev, nnz, d_output, step.lr, step.eps,
                                                    m.cache_optimizer_state, m.cache_weight.data)
            return (None,) * (n_fixed + len(m.tt_cores))
        # (for ttemb_dist: did this gradient come from a grouped backward -- the family with bounded device-side waits,
        #  whose last kernel leaves its verdict in the workspace header?  Host-side rule, launches nothing.)
        m._last_bwd_grouped = _nat.is_grouped(m._shape, nnz, B, rowidx is None)
        full = _deliver_dense(m, table, m.num_tables == 1 and not ctx.live_cache,
                              lambda dst: _nat.backward_dense(m._shape, cores, indices, rowidx, nnz, nnz_dev, B, d_output, dst,
                                                              m._ws, ctx.plan, offsets))
        if full is None:
            return (None,) * (n_fixed + len(m.tt_cores))
        d_cache = None
        if ctx.live_cache:
            d_cache = torch.empty_like(m.cache_weight.data)
            _nat.cache_backward_dense(cache_loc, rowidx, 0, nnz_dev, nnz, d_output, d_cache,
                                      nnz_dev[1:] if nnz_dev.numel() > 1 else None)
        return (None,) * (n_fixed - 1) + (d_cache,) + tuple(full)


class _TablesLookup(torch.autograd.Function):
    """``num_tables`` > 1 without a host synchronisation: every table is a *window* of the id list whose bounds the kernels
    read from ``offsets`` on the device (``ttemb_forward_window`` ...; the reference hands its kernels a per-id ``tableidx``
    instead, tt_embeddings_cuda.cu:1349-1365).  One node for the whole call: the output is the [num_tables, B, D] tensor the
    windows write their rows of; the backward runs table by table (fused step, or dense gradients of the [num_tables, p, row]
    parameters, each table's slice written by its own window)."""

    @staticmethod
    def forward(ctx, module: "TableBatchedTTEmbeddingBag", B: int, indices: torch.Tensor, offsets: torch.Tensor,
                *tt_cores: torch.Tensor) -> torch.Tensor:
        T = module.num_tables
        out = torch.empty((T, B, module.embedding_dim), dtype=torch.float32, device=indices.device)
        ctx.module, ctx.B, ctx.indices, ctx.offsets = module, B, indices, offsets
        if module._before_weights is not None:
            module._before_weights()   # a data-parallel update of the cores is pending: finish it first
        for k in range(T):
            _nat.forward_window(module._shape, _nat.core_ptrs(tt_cores, k), indices, offsets, k * B, B, out, module._ws)
        return out

    @staticmethod
    def backward(ctx, d_output: torch.Tensor):
        m, B, indices, offsets = ctx.module, ctx.B, ctx.indices, ctx.offsets
        d_output = _f32(d_output)
        T = m.num_tables
        if m.sparse:
            for k in range(T):
                step = _step_call(m, k)   # (Adam: one step count per table, advanced by that table's window)
                _nat.backward_window(m._shape, _nat.core_ptrs(m.tt_cores, k), indices, offsets, k * B, B, d_output, m._ws,
                                     opt_state=step.state, lr=step.lr, eps=step.eps, adam=step.adam)
            return (None,) * (4 + len(m.tt_cores))
        grads = [torch.empty_like(c) for c in m.tt_cores]
        for k in range(T):
            _nat.backward_window(m._shape, _nat.core_ptrs(m.tt_cores, k), indices, offsets, k * B, B, d_output, m._ws,
                                 d_cores=_nat.core_ptrs(grads, k))
        return (None,) * 4 + tuple(grads)


class _SparseLookup(torch.autograd.Function):
    """The common training call -- one table, ``sparse=True``, no live cache -- with as little Python around the two
    native calls as autograd allows: ONE tensor input (the first core, so that the node is recorded; every gradient is
    ``None`` because the update happens inside backward), bound native arguments (``ttemb_native.LeanCalls``).  Same
    kernels and results as ``TTLookupFunction``."""

    @staticmethod
    def forward(ctx, anchor: torch.Tensor, module: "TableBatchedTTEmbeddingBag", indices: torch.Tensor,
                offsets: torch.Tensor, B: int) -> torch.Tensor:
        nnz = indices.numel()
        out = torch.empty((B, module.embedding_dim), dtype=torch.float32, device=indices.device)
        ctx.module, ctx.indices, ctx.offsets, ctx.B = module, indices, offsets, B
        ctx.plan = module._lean.forward(module._cores(), indices, offsets, nnz, B, out)
        return out

    @staticmethod
    def backward(ctx, d_output: torch.Tensor):
        m = ctx.module
        d_output = _f32(d_output)
        state = None if m.optimizer in _SGD_LIKE else m._states()
        m._lean.backward(m._cores(), state, ctx.indices, ctx.offsets, ctx.indices.numel(), ctx.B, d_output,
                         m._lr_arg(), float(m.eps), ctx.plan, m._adam_lean())
        return None, None, None, None, None


class _BucketLookup(torch.autograd.Function):
    """The data-parallel step's call -- one table, ``sparse=False``, no live cache, a wrapper's flat gradient bucket attached
    (``ttemb_dist.TTDataParallel``) -- with the lean bridge of ``_SparseLookup``: one tensor input, bound native arguments.
    The forward is split around the wrapper's pending update; the backward writes the core gradients straight into the bucket
    and hands nothing back to autograd.  (Through ``TTLookupFunction`` the same step cost the host ~200 us on a slow host --
    as much as its GPU time at 409 600 ids.)  Same kernels and results."""

    @staticmethod
    def forward(ctx, anchor: torch.Tensor, module: "TableBatchedTTEmbeddingBag", indices: torch.Tensor,
                offsets: torch.Tensor, B: int) -> torch.Tensor:
        nnz = indices.numel()
        out = torch.empty((B, module.embedding_dim), dtype=torch.float32, device=indices.device)
        ctx.module, ctx.indices, ctx.offsets, ctx.B = module, indices, offsets, B
        pending = module._before_weights
        if pending is None:
            ctx.plan = module._lean.forward(module._cores(), indices, offsets, nnz, B, out)
        else:
            ctx.plan = module._lean.forward_split(module._cores(), indices, offsets, nnz, B, out, pending)
        return out

    @staticmethod
    def backward(ctx, d_output: torch.Tensor):
        m = ctx.module
        d_output = _f32(d_output)
        nnz = ctx.indices.numel()
        m._last_bwd_grouped = _nat.is_grouped(m._shape, nnz, ctx.B)
        # (no bucket: the wrapper was detached between forward and backward -- the gradients then go through .grad)
        _deliver_dense(m, 0, True, lambda dst: m._lean.backward_dense(m._cores(), ctx.indices, ctx.offsets, nnz, ctx.B,
                                                                      d_output, dst, ctx.plan), into_grad=True)
        return None, None, None, None, None


class _ExactLookup(torch.autograd.Function):
    """Exact mode: one table's lookup on the bit-reproducible kernels (``ttemb_forward_exact`` / ``ttemb_backward_*_exact``,
    include/ttemb.h "Exact mode").  Outputs, gradients, updated cores and optimizer state are a function of the inputs
    only.  Fused SGD / Adagrad (``sparse``) update the touched rows only, fused Adam every row (the exact dense gradient into
    scratch, then the elementwise step); dense gradients go to autograd, or into the
    ``_dense_grad_out`` bucket of ``ttemb_dist.TTDataParallel`` (adding to it after the first backward of a step, like the
    plain lookup).  A module with several tables runs one exact call per table on the host-split id list."""

    @staticmethod
    def forward(ctx, module: "TableBatchedTTEmbeddingBag", table: int, B: int, indices: torch.Tensor,
                offsets: torch.Tensor, *tt_cores: torch.Tensor) -> torch.Tensor:
        ctx.module, ctx.table, ctx.B, ctx.indices, ctx.offsets = module, table, B, indices, offsets
        if module._before_weights is not None:
            module._before_weights()   # a data-parallel update of the cores is pending: finish it first
        out = torch.empty((B, module.embedding_dim), dtype=torch.float32, device=indices.device)
        _nat.forward_exact(module._shape, _nat.core_ptrs(tt_cores, table), indices, offsets, B, out, module._ws)
        return out

    @staticmethod
    def backward(ctx, d_output: torch.Tensor):
        m, table, B, indices, offsets = ctx.module, ctx.table, ctx.B, ctx.indices, ctx.offsets
        d_output = _f32(d_output)
        cores = _nat.core_ptrs(m.tt_cores, table)
        n_fixed = 5
        if m.sparse:
            step = _step_call(m, table)
            _nat.backward_exact(m._shape, cores, indices, offsets, B, d_output, m._ws, opt_state=step.state, lr=step.lr,
                                eps=step.eps, adam=step.adam)
            return (None,) * (n_fixed + len(m.tt_cores))
        m._last_bwd_grouped = False   # no bounded device-side waits: nothing in the workspace header to look at
        full = _deliver_dense(m, table, m.num_tables == 1,
                              lambda dst: _nat.backward_exact(m._shape, cores, indices, offsets, B, d_output, m._ws, d_cores=dst))
        return (None,) * n_fixed + (tuple(full) if full is not None else (None,) * len(m.tt_cores))


class _WeightedBag(torch.autograd.Function):
    """``mode="sum"`` with ``per_sample_weights``: ``out[b] = sum_{i in bag b} w[i] rows[i]`` over the looked-up rows of
    bags of one (``ttemb_bag_reduce``).  The backward hands ``d_rows[i] = w[i] dOut[bag(i)]`` to the lookup's own backward
    (fused step, dense gradients, bucket, exact -- whatever produced ``rows``) and, when ``w`` needs it,
    ``w.grad[i] = <dOut[bag(i)], rows[i]>`` from the same pass.  ``rows`` is kept only for that weight gradient."""

    @staticmethod
    def forward(ctx, rows: torch.Tensor, weights: torch.Tensor, offsets: torch.Tensor,
                module: "TableBatchedTTEmbeddingBag") -> torch.Tensor:
        out = torch.empty((offsets.numel() - 1, rows.shape[1]), dtype=torch.float32, device=rows.device)
        _nat.bag_reduce(rows, weights, offsets, out, module._ws)
        ctx.module, ctx.offsets = module, offsets
        ctx.save_for_backward(weights, rows if ctx.needs_input_grad[1] else None)
        return out

    @staticmethod
    def backward(ctx, d_output: torch.Tensor):
        weights, rows = ctx.saved_tensors
        d_output = _aligned(d_output)
        d_rows = torch.empty((weights.numel(), d_output.shape[-1]), dtype=torch.float32, device=d_output.device)
        d_w = torch.empty_like(weights) if ctx.needs_input_grad[1] else None
        _nat.bag_reduce_backward(d_output, weights, ctx.offsets, d_rows, ctx.module._ws, rows=rows, d_weights=d_w)
        return d_rows, d_w, None, None


class _MappedBag(torch.autograd.Function):
    """The pool of the ``dedup`` route: ``out[b] = sum_{n in bag b} w[n] rows[map[n]]`` (``ttemb_bag_reduce_mapped``; ``w``
    None: 1) over a rows buffer that holds one row per DISTINCT id of the call -- ``uniq = (map, perm, seg, count)`` is what
    ``ttemb_unique_ids`` wrote for the call's ids and is owned by this node.  The backward sums each distinct id's gradient
    first (``d_rows[j] = sum_k w[perm[k]] dOut[bag(perm[k])]`` over the positions of id j, in position order) and hands
    ``d_rows`` to the lookup's own backward, which reads the first ``count`` rows only; ``w.grad[n] = <dOut[bag(n)],
    rows[map[n]]>``.  ``rows`` is kept only for that weight gradient."""

    @staticmethod
    def forward(ctx, rows: torch.Tensor, weights: Optional[torch.Tensor], offsets: torch.Tensor,
                module: "TableBatchedTTEmbeddingBag", uniq: tuple) -> torch.Tensor:
        out = torch.empty((offsets.numel() - 1, rows.shape[1]), dtype=torch.float32, device=rows.device)
        _nat.bag_reduce_mapped(rows, uniq[0], weights, offsets, out, module._ws)
        ctx.module, ctx.offsets, ctx.uniq, ctx.cap = module, offsets, uniq, rows.shape[0]
        ctx.save_for_backward(weights, rows if ctx.needs_input_grad[1] else None)
        return out

    @staticmethod
    def backward(ctx, d_output: torch.Tensor):
        weights, rows = ctx.saved_tensors
        map_, perm, seg, count = ctx.uniq
        d_output = _aligned(d_output)
        # one row per position of capacity, the first `count` written: the lookup's backward reads no more than those
        d_rows = torch.empty((ctx.cap, d_output.shape[-1]), dtype=torch.float32, device=d_output.device)
        d_w = torch.empty(map_.numel(), dtype=torch.float32, device=d_output.device) if ctx.needs_input_grad[1] else None
        _nat.bag_reduce_mapped_backward(d_output, weights, map_, perm, seg, count, ctx.offsets, d_rows, ctx.module._ws,
                                        rows=rows, d_weights=d_w)
        return d_rows, d_w, None, None, None


class _BagMean(torch.autograd.Function):
    """``mode="mean"``: the bag sums of the plain lookup divided by the bag lengths in place (``ttemb_bag_mean``); the
    backward divides ``dOut`` the same way into scratch for the lookup's backward.  ``sums`` is [..., B', D] with
    ``offsets`` of its B' bags."""

    @staticmethod
    def forward(ctx, sums: torch.Tensor, offsets: torch.Tensor) -> torch.Tensor:
        flat = sums.view(-1, sums.shape[-1])
        _nat.bag_mean(flat, flat, offsets)
        ctx.offsets = offsets
        ctx.mark_dirty(sums)
        return sums

    @staticmethod
    def backward(ctx, d_output: torch.Tensor):
        d_output = _aligned(d_output)
        d_sums = torch.empty_like(d_output)
        D = d_output.shape[-1]
        _nat.bag_mean(d_output.view(-1, D), d_sums.view(-1, D), ctx.offsets)
        return d_sums, None


class _BagMax(torch.autograd.Function):
    """``mode="max"``: ``out[b][d] = max_{i in bag b} rows[i][d]`` over the looked-up rows of bags of one (``ttemb_bag_max``),
    the first position winning among equal values and a NaN over every number.  Only the winners (int32 ``[B, D]``
    positions) are kept, not ``rows``: the backward hands ``d_rows[i][d] = dOut[bag(i)][d]`` at the winner, zeros elsewhere
    (every element written), to the lookup's own backward -- fused step, dense gradients, bucket, exact: whatever produced
    ``rows``.  ``indices`` / ``pad``: positions whose id is the pad are skipped (the small-call route of a padded call)."""

    @staticmethod
    def forward(ctx, rows: torch.Tensor, offsets: torch.Tensor, module: "TableBatchedTTEmbeddingBag",
                indices: Optional[torch.Tensor], pad: int) -> torch.Tensor:
        B, D = offsets.numel() - 1, rows.shape[1]
        out = torch.empty((B, D), dtype=torch.float32, device=rows.device)
        argmax = torch.empty((B, D), dtype=torch.int32, device=rows.device)
        _nat.bag_max(rows, offsets, out, argmax, module._ws, indices, pad)
        ctx.offsets, ctx.argmax, ctx.nnz = offsets, argmax, rows.shape[0]
        return out

    @staticmethod
    def backward(ctx, d_output: torch.Tensor):
        d_output = _aligned(d_output)
        d_rows = torch.empty((ctx.nnz, d_output.shape[-1]), dtype=torch.float32, device=d_output.device)
        _nat.bag_max_backward(d_output, ctx.argmax, ctx.offsets, d_rows)
        return d_rows, None, None, None, None


class _PadWeights(torch.autograd.Function):
    """The masked-rows route of a padded call: ``w'[i] = keep[i] (w[i] or 1) (1 / len'(bag(i)) for a mean)``
    (``ttemb_pad_weights``), the weights ``_WeightedBag`` then pools the bags-of-one rows with.  ``w`` is only given with
    ``mode="sum"``, where ``w'`` is ``keep * w`` and its backward the same kernel on the incoming gradient."""

    @staticmethod
    def forward(ctx, weights: Optional[torch.Tensor], indices: torch.Tensor, offsets: torch.Tensor, pad: int,
                mean: bool) -> torch.Tensor:
        out = torch.empty(indices.numel(), dtype=torch.float32, device=indices.device)
        _nat.pad_weights(indices, offsets, weights, pad, mean, out)
        ctx.indices, ctx.offsets, ctx.pad = indices, offsets, pad
        return out

    @staticmethod
    def backward(ctx, d_w: torch.Tensor):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        d_w = d_w.contiguous()
        out = torch.empty_like(d_w)
        _nat.pad_weights(ctx.indices, ctx.offsets, d_w, ctx.pad, False, out)
        return out, None, None, None, None


class _quiet_collector:
    """Around the stream captures of ``capture()`` / ``capture_bags()``: one full collection first, then none until the
    captures are done.  Python's cyclic collector runs whenever enough objects have been allocated, also in the middle of a
    capture, and it runs the destructors of whatever dead cycle it finds -- a dead cycle that holds HIP graphs or device
    memory then frees them while this thread captures, which the runtime refuses in global capture mode: the process aborts.
    (``torch.cuda.graph`` used to collect before every capture and no longer does.)"""

    def __enter__(self) -> None:
        gc.collect()
        self.was_enabled = gc.isenabled()
        gc.disable()

    def __exit__(self, *exc) -> None:
        if self.was_enabled:
            gc.enable()


class _ReplayLookup(torch.autograd.Function):
    """Autograd node of a captured lookup: forward and backward are one HIP-graph replay each.  ``n_live`` / ``B_live``: None
    for a fixed capture; the ids and bags of a ``capture(..., variable=True)`` call, already staged -- the forward then hands
    out the live rows of the static output and the backward fills the live rows of the static gradient (the rows past them
    belong to empty bags, which no kernel reads) and replays, unless the call had no id."""

    @staticmethod
    def forward(ctx, anchor: torch.Tensor, cap: "CapturedLookup", n_live: Optional[int] = None,
                B_live: Optional[int] = None) -> torch.Tensor:
        ctx.cap, ctx.n_live, ctx.B_live = cap, n_live, B_live
        cap.fwd_graph.replay()
        # (always a VIEW of the static buffer: handing out the buffer itself would give it this node as its grad_fn, a
        #  reference cycle cap -> output -> node -> cap that only the cyclic collector frees -- see _quiet_collector)
        return cap.output[:] if B_live is None else cap.output[:B_live]

    @staticmethod
    def backward(ctx, d_output: torch.Tensor):
        cap = ctx.cap
        if ctx.n_live != 0:   # a call without ids is a no-op for every optimiser and does not advance Adam's t (include/ttemb.h)
            (cap.d_output if ctx.B_live is None else cap.d_output[:ctx.B_live]).copy_(d_output)
            cap.bwd_graph.replay()
        return None, None, None, None


class CapturedLookup:
    """``emb.capture(nnz, B)``: a lookup of fixed size whose forward and whose backward (gradient + fused optimiser step)
    are each ONE HIP-graph replay -- for steps so small that Python and launch overhead are most of their time (the metric's
    literal "batch 2048": ~25 us of kernels under ~75-115 us of eager host work).  Call it like the module:
    ``out = cap(indices[, offsets])``; ``out`` is a static buffer that the next call overwrites (as with
    ``torch.cuda.make_graphed_callables``).  The workspace and plan the graphs were captured with are owned by this object,
    so other calls on the module cannot move them.  ``sparse=True`` modules with one table and no live cache.  A captured
    lookup is the unweighted ``mode="sum"`` call: it takes no ``per_sample_weights``, and a ``mode="mean"`` module is refused.

    ``variable=True``: ``nnz`` and ``B`` are CAPACITIES and every call brings its own size -- any ``indices.numel() <= nnz`` in
    ``offsets.numel() - 1 <= B`` bags (without offsets: bags of one id), int64 or int32 -- which is what a GNN's frontiers
    need.  One launch (``ttemb_stage_call``) puts the call into the static buffers, pads the offsets with empty bags and
    leaves the id count in a device word the captured kernels read; the result is ``output[:B_live]``, a view of the static
    buffer.  The launches are sized by the capacity, so pick one near the largest frontier.  Offsets come with each call,
    none at capture.  Not in exact mode: the exact backward takes no device id count.  DESIGN.md §4.11.

    The learning rate: a captured backward of a plain module bakes it in (a call after ``set_learning_rate`` raises:
    capture again).  A module built with ``capturable=True`` hands the graphs the ADDRESS of its device word ``lr_dev``
    instead: every call first brings the word up to ``module.learning_rate`` (one ``fill_`` when it changed, nothing
    otherwise), then replays -- a scheduler that changes the rate every step re-captures nothing.  DESIGN.md §4.12."""

    def __init__(self, module: "TableBatchedTTEmbeddingBag", nnz: int, B: int, offsets: Optional[torch.Tensor] = None,
                 variable: bool = False) -> None:
        assert module.sparse and module.num_tables == 1, "capture() covers the fused-optimiser mode of a single table"
        assert not (module.use_cache and not module.warmup), "capture() with a live row cache is not supported"
        assert module.mode == "sum", "capture() covers mode='sum' (unweighted)"
        assert module.padding_idx is None, "capture() does not cover padding_idx: capture a module without it"
        self.module, self.nnz, self.B = module, int(nnz), int(B)
        self.variable = bool(variable)
        if self.variable and offsets is not None:
            raise ValueError("capture(variable=True) takes no offsets: nnz and B are capacities, the offsets come with each call")
        if self.variable and not (0 < self.nnz < 2 ** 31 and self.B > 0):
            raise ValueError(f"capture(variable=True): the capacities must be positive (ids below 2^31), got nnz={nnz}, B={B}")
        if self.variable and module._exact_active():
            # (the exact backward sorts all `nnz` staged positions: stale ids past the live count would move its chunk edges,
            #  and with them the summation order -- results would no longer be those of the eager call, bit for bit)
            raise RuntimeError(
                f"capture(nnz={self.nnz}, B={self.B}, variable=True) is not served in exact mode (OptimType.EXACT_SGD / "
                "deterministic): the exact kernels take no device id count, so a call shorter than the capacity would not "
                "reproduce the eager call bit for bit.  Use variable=False, or a module outside exact mode.")
        dev = module.tt_cores[0].device
        self.indices = torch.zeros(self.nnz, dtype=torch.int64, device=dev)
        if self.variable:   # staged per call (ttemb_stage_call); until the first one: a call without ids
            self.offsets = torch.zeros(self.B + 1, dtype=torch.int64, device=dev)
            self.nnz_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        else:
            self.offsets = (torch.arange(self.B + 1, dtype=torch.int64, device=dev) if offsets is None
                            else offsets.to(dev, torch.int64).contiguous().clone())
            self.nnz_dev = None
        self.output = torch.empty((self.B, module.embedding_dim), dtype=torch.float32, device=dev)
        self.d_output = torch.zeros_like(self.output)
        self._lean = _nat.LeanCalls(module._shape, _nat.Workspace())   # private workspace: pinned for the graphs' lifetime
        cores = module._cores()
        state = None if module.optimizer in _SGD_LIKE else module._states()
        lr, eps = module._lr_arg(), float(module.eps)   # (capturable: the device word, brought up to date; held by address)
        # Adam: b1, b2 and the weight decay are baked like lr / eps; the step count is a device word the graph advances
        adam = module._adam_lean()
        self._adam_key = module._adam_key()
        self.exact = module._exact_active()   # exact mode: the graphs hold the exact kernels
        if self.exact:
            self.plan = None

            def fwd():
                _nat.forward_exact(module._shape, _nat.core_ptrs(cores), self.indices, self.offsets, self.B, self.output,
                                   self._lean.ws)

            def bwd():
                _nat.backward_exact(module._shape, _nat.core_ptrs(cores), self.indices, self.offsets, self.B, self.d_output,
                                    self._lean.ws, opt_state=None if state is None else _nat.core_ptrs(state), lr=lr, eps=eps,
                                    adam=None if adam is None else (_nat.core_ptrs(adam[0]), adam[1], adam[2]))
        else:
            # (variable: the route is chosen from the capacities, on the host; the kernels read the live count from nnz_dev)
            def fwd():
                self.plan = self._lean.forward(cores, self.indices, self.offsets, self.nnz, self.B, self.output,
                                               nnz_dev=self.nnz_dev)

            def bwd():
                self._lean.backward(cores, state, self.indices, self.offsets, self.nnz, self.B, self.d_output, lr, eps, self.plan,
                                    adam, nnz_dev=self.nnz_dev)
        # Capturing EXECUTES one backward on a zero gradient.  For SGD / Adagrad that leaves everything as it is; an Adam step
        # on g = 0 advances t, decays m and v and, with weight decay, moves the cores: all of it is put back after the
        # capture, so that a captured module equals an eager one step for step.
        saved = None
        if adam is not None:
            saved = [t.detach().clone() for t in (*cores, *state, *adam[0], module.adam_step)]
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):   # warm-up outside capture: workspace allocation, LDS-size attributes, size queries
            fwd()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        _nat.init()   # the pinned fault word exists before anything is captured (a capture must not allocate it)
        self.fwd_graph, self.bwd_graph = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        with _quiet_collector():
            with torch.cuda.graph(self.fwd_graph):
                fwd()
            with torch.cuda.graph(self.bwd_graph):   # (a zero gradient: the captured update leaves the cores as they are)
                bwd()
        if saved is not None:
            with torch.no_grad():
                for t, t0 in zip((*cores, *state, *adam[0], module.adam_step), saved):
                    t.copy_(t0)
        self._lr, self._eps = (None if module.capturable else lr), eps
        self._baked = self._pointers()

    def _pointers(self) -> tuple:
        """What the graphs hold by address: the cores, the optimiser state and a capturable module's rate word."""
        m = self.module
        ptrs = tuple(c.data_ptr() for c in m._cores())
        if m.capturable:
            ptrs += (m.lr_dev.data_ptr(),)
        if m.optimizer not in _SGD_LIKE:
            ptrs += tuple(st.data_ptr() for st in m._states())
        if m.optimizer == OptimType.ADAM:
            ptrs += tuple(st.data_ptr() for st in m.optimizer_state_v) + (m.adam_step.data_ptr(),)
        return ptrs

    def __call__(self, indices: torch.Tensor, offsets: Optional[torch.Tensor] = None) -> torch.Tensor:
        m = self.module
        if m.use_cache and not m.warmup:
            # after cache_populate() the eager module serves and trains the hot ids in cache_weight; the captured graphs
            # read and update the TT cores only -- the two would diverge silently
            raise RuntimeError("the row cache went live after capture(): captured lookups do not cover a live cache")
        if m.capturable != (self._lr is None):
            raise RuntimeError("module.capturable was changed after capture(): capture() again")
        # (a capturable module: the rate is not part of the graphs -- _adam_key() leaves it out, too)
        if ((self._lr is not None and float(m.learning_rate) != self._lr) or float(m.eps) != self._eps
                or m._adam_key() != self._adam_key):
            raise RuntimeError("learning rate / eps are part of the captured backward: capture() again after changing them "
                               "(with OptimType.ADAM also betas, weight_decay and decoupled_weight_decay)")
        if self._pointers() != self._baked:
            raise RuntimeError("tt_cores / optimizer_state were re-allocated after capture() (.to(), .data = ..., "
                               "load_state_dict into new storage): capture() again")
        if self._lr is None:
            m._refresh_lr()   # one fill_ on this stream when learning_rate changed since the last call; no synchronisation
        if self.variable:
            return self._call_variable(indices, offsets)
        if m.use_cache:   # warm-up: the LFU statistics of a captured step count like those of an eager one
            m.update_cache(indices)
        self.indices.copy_(indices)
        if offsets is not None:
            self.offsets.copy_(offsets)
        return _ReplayLookup.apply(m._cores()[0], self, None, None)

    def _call_variable(self, indices: torch.Tensor, offsets: Optional[torch.Tensor]) -> torch.Tensor:
        m = self.module
        n = indices.numel()
        B_live = n if offsets is None else offsets.numel() - 1
        # every size check before anything is launched
        if n > self.nnz:
            raise ValueError(f"{n} ids exceed the captured capacity nnz={self.nnz}: capture() again with a larger one")
        if B_live > self.B:
            raise ValueError(f"{B_live} bags exceed the captured capacity B={self.B}"
                             + (" (a call without offsets is one bag per id)" if offsets is None else "")
                             + ": capture() again with a larger one")
        if B_live < 0:
            raise ValueError("offsets must hold B + 1 entries (include_last_offset): got an empty tensor")
        if m.use_cache:   # warm-up: the LFU statistics of a captured step count like those of an eager one
            m.update_cache(indices if indices.dtype == torch.int64 else indices.long())
        _nat.stage_call(indices, offsets, self.indices, self.offsets, self.nnz_dev)
        return _ReplayLookup.apply(m._cores()[0], self, n, B_live)


class _ReplayBags(torch.autograd.Function):
    """Autograd node of captured bags: forward and backward are one HIP-graph replay each.  ``weights`` is the call's own
    tensor (None without): the staged copy is what the graphs read, this input only lets autograd ask for its gradient.
    ``n_live`` / ``B_live``: the ids and bags of the call, already staged."""

    @staticmethod
    def forward(ctx, anchor: torch.Tensor, cap: "CapturedBags", weights: Optional[torch.Tensor], n_live: int,
                B_live: int) -> torch.Tensor:
        ctx.cap, ctx.n_live, ctx.B_live = cap, n_live, B_live
        ctx.w_shape = None if weights is None else weights.shape
        cap.fwd_graph.replay()
        return cap.output[:B_live] if cap.variable else cap.output[:]   # (a view in both cases: _ReplayLookup.forward)

    @staticmethod
    def backward(ctx, d_output: torch.Tensor):
        cap = ctx.cap
        want_w = ctx.w_shape is not None and ctx.needs_input_grad[2]
        if ctx.n_live == 0:   # no id: a no-op for every optimiser, Adam's t included; the weight gradient is empty
            d_w = torch.zeros(ctx.w_shape, dtype=torch.float32, device=d_output.device) if want_w else None
            return None, None, d_w, None, None
        (cap.d_output[:ctx.B_live] if cap.variable else cap.d_output).copy_(d_output)
        cap.bwd_graph.replay()
        # (a copy: autograd may keep it as w.grad, and the next replay overwrites the static buffer)
        d_w = cap.d_weights_out[:ctx.n_live].clone().view(ctx.w_shape) if want_w else None
        return None, None, d_w, None, None


class CapturedBags(CapturedLookup):
    """``emb.capture_bags(nnz, B, mode=..., weighted=..., fanout=..., variable=...)``: the pooled calls of the module --
    ``per_sample_weights``, ``mode="mean"`` / ``"max"``, ``padding_idx``, 2-D ``indices[rows, fanout]`` -- with forward and
    backward (pool backward, TT backward, the module's fused step) as ONE HIP-graph replay each.  Call it like the module:
    ``out = cap(indices, offsets=None, per_sample_weights=None)``; ``out`` is (a view of) a static buffer that the next call
    overwrites.  The mode, ``weighted``, ``fanout`` and the module's ``padding_idx`` are fixed at capture, like the learning
    rate of a plain module (``CapturedLookup``); the graphs are linear chains on one stream.  ``sparse=True`` modules with
    one table and no live cache, every fused optimiser, ``capturable=True`` rate words, exact mode with ``variable=False``.

    Routes, chosen once from the capacities: a mean without weights and padding is the plain lookup on the staged offsets
    and ``ttemb_bag_mean`` in place; the unweighted unpadded sum is the plain lookup; everything else looks the ids up as
    bags of one into a static ``rows[nnz, D]`` and pools them (``ttemb_bag_reduce_n`` with the call's weights or those of
    ``ttemb_pad_weights_n``, ``ttemb_bag_max_n``), the backward pooling into a static ``d_rows[nnz, D]`` the lookup's
    backward takes.  A padded call takes these masked rows (every pad position is looked up, and pooled with weight 0) unless
    the capture asks for ``pad_route="partition"``.

    ``pad_route="partition"`` (a module with ``padding_idx``; not in exact mode): the FIRST node of the forward graph
    (``ttemb_compact_bags``) drops the pad ids of the staged call on the device -- kept ids, their weights and the compacted
    offsets into static buffers of their own, the kept count into a device word -- and everything behind it, in both graphs,
    runs on those with that word as its id count: routed as if the module had no padding (``cap.route``), so the unweighted
    sum and mean own no ``rows`` / ``d_rows`` at all, a mean divides by the kept lengths and a bag of pads only is an empty
    bag.  The weight gradient goes back to the call's positions by a gather (``ttemb_expand_kept``): exactly 0 at a pad.  A
    call whose ids are ALL pads replays the backward with a kept count of 0: no core row is touched, so SGD and Adagrad
    leave cores and state as they are, while Adam -- whose step is dense -- counts a step (``t`` advances, ``m`` and ``v``
    decay), as an eager call of pads only does too.  ``cap.pad_route`` tells which ("partition", "masked", None: no padding).

    ``dedup=True`` (sum and mean bags, outside exact mode, up to 2^20 ids): ``cap.route == "dedup"``.  Behind the compaction
    of a partitioned capture, the forward graph finds the distinct ids of the (kept) ids on the device
    (``ttemb_unique_ids_n``: launches and the sort's storage sized by the capacity, the live count read from the count word)
    into the static ``uids`` / ``inverse`` / ``perm`` / ``seg`` / ``unique_count``, looks ``uids`` up as bags of one into
    ``rows`` with ``unique_count`` as the count word, and pools through the map (``ttemb_bag_reduce_mapped_n``; a mean
    without pads divides afterwards).  The backward sums each distinct id's gradient into ``d_rows``
    (``ttemb_bag_reduce_mapped_backward_n``) and hands it to the lookup's backward on ``uids``.  The sort always runs over the
    whole capacity: pick one near the usual call.  DESIGN.md §4.16.

    ``variable=True``: ``nnz`` and ``B`` are capacities; one launch (``ttemb_stage_bags``) puts ids, offsets (or, with
    ``fanout``, the offsets it generates) and weights into the static buffers and leaves the id count in the device word every
    captured kernel stops at.  ``variable=False``: every call has exactly the captured size.  A call without ids replays the
    forward (zeros) and skips the backward.  The weight gradient is computed by every weighted backward and handed to
    autograd (one copy of ``n`` floats) when the call's weights require it.  DESIGN.md §4.13."""

    _MODES = ("sum", "mean", "max")
    _PAD_ROUTES = (None, "masked", "partition")
    _DEDUP_MAX_IDS = 1 << 20   # up to here the sort of ttemb_unique_ids_n consists of kernels only (include/ttemb_unique_n.h)

    @staticmethod
    def check_arguments(module: "TableBatchedTTEmbeddingBag", nnz: int, B: int, mode: Optional[str], weighted: bool,
                        fanout: Optional[int], pad_route: Optional[str] = None) -> str:
        """The argument errors of ``capture_bags``, raised before a device is touched; returns the effective mode."""
        if pad_route not in CapturedBags._PAD_ROUTES:
            raise ValueError(f"pad_route must be None, 'masked' or 'partition', got {pad_route!r}")
        if pad_route == "partition" and module.padding_idx is None:
            raise ValueError("pad_route='partition' drops the ids equal to padding_idx: this module has none")
        if mode is None:
            mode = module.mode
        elif mode not in CapturedBags._MODES:
            raise ValueError(f"mode must be 'sum', 'mean' or 'max', got {mode!r}")
        if weighted and mode != "sum":
            raise ValueError("per_sample_weights was not None: weighted bags are only supported with mode='sum' "
                             "(as in torch.nn.functional.embedding_bag)")
        if not module.sparse:
            raise ValueError("capture_bags() covers the fused-optimiser mode (sparse=True): the captured backward is the step")
        if module.num_tables != 1:
            raise ValueError(f"capture_bags() covers a single table, this module has {module.num_tables}")
        if not (0 < int(nnz) < 2 ** 31 and int(B) > 0):
            raise ValueError(f"capture_bags(): nnz and B must be positive (ids below 2^31), got nnz={nnz}, B={B}")
        if fanout is not None and (int(fanout) <= 0 or int(nnz) != int(B) * int(fanout)):
            raise ValueError(f"capture_bags(fanout={fanout}): nnz must equal B * fanout, got nnz={nnz}, B={B}")
        return mode

    @staticmethod
    def check_dedup(nnz: int, mode: str) -> None:
        """The argument errors of ``capture_bags(dedup=True)``, raised before a device is touched: what the eager dedup route
        refuses for every module (``_dedup_for``), and what the captured sort adds."""
        if mode == "max":
            raise ValueError("dedup with mode='max' is not supported: it needs a max pool that reads its rows through the map "
                             "and a masked sum per distinct id in the backward.  Use dedup=False for max bags.")
        if int(nnz) > CapturedBags._DEDUP_MAX_IDS:
            raise ValueError(f"capture_bags(nnz={nnz}, dedup=True): past 2^20 ids the sort of the distinct-id pass clears its "
                             "counters with memset nodes when it is captured, which this library keeps out of its graphs.  "
                             "Capture a smaller capacity, or use dedup=False.")

    def __init__(self, module: "TableBatchedTTEmbeddingBag", nnz: int, B: int, mode: Optional[str] = None, weighted: bool = False,
                 fanout: Optional[int] = None, variable: bool = False, pad_route: Optional[str] = None,
                 dedup: bool = False) -> None:
        mode = self.check_arguments(module, nnz, B, mode, weighted, fanout, pad_route)
        if dedup:
            self.check_dedup(nnz, mode)
        if module.use_cache and not module.warmup:
            raise RuntimeError("capture_bags() with a live row cache is not supported")
        self.module, self.nnz, self.B = module, int(nnz), int(B)
        self.mode, self.weighted, self.variable = mode, bool(weighted), bool(variable)
        self.fanout = None if fanout is None else int(fanout)
        self.pad = module.padding_idx
        self.dedup = bool(dedup)
        self._module_mode = module.mode
        self.exact = module._exact_active()   # exact mode: the graphs hold the exact kernels
        if self.variable and self.exact:
            raise RuntimeError(
                f"capture_bags(nnz={self.nnz}, B={self.B}, variable=True) is not served in exact mode (OptimType.EXACT_SGD / "
                "deterministic): the exact kernels take no device id count, so a call shorter than the capacity would not "
                "reproduce the eager call bit for bit.  Use variable=False, or a module outside exact mode.")
        part = pad_route == "partition"
        if part and self.exact:
            raise RuntimeError(
                f"capture_bags(nnz={self.nnz}, B={self.B}, pad_route='partition') is not served in exact mode "
                "(OptimType.EXACT_SGD / deterministic): the exact kernels take no device id count, and the count of the kept "
                "ids exists on the device only.  Use pad_route='masked', or a module outside exact mode.")
        if self.dedup and self.exact:
            raise RuntimeError(
                f"capture_bags(nnz={self.nnz}, B={self.B}, dedup=True) is not served in exact mode (OptimType.EXACT_SGD / "
                "deterministic): the exact kernels take no device id count, and the count of the distinct ids exists on the "
                "device only.  Use dedup=False, or a module outside exact mode.")
        # how the pads are left out: "partition" (compacted away in front of everything else), "masked" (looked up, weight 0)
        self.pad_route = "partition" if part else ("masked" if self.pad is not None else None)
        mask_pad = None if part else self.pad   # the pad id the pooling kernels have to mask; none once the ids are compacted
        nnz, B, D = self.nnz, self.B, module.embedding_dim
        dev = module.tt_cores[0].device
        f32 = dict(dtype=torch.float32, device=dev)
        # which route: "plain" (the lookup pools), "mean" (the lookup, then the division), "rows" (bags of one, then the pooling),
        # "dedup" (the distinct ids as bags of one, then the pooling through the inverse map)
        self.route = "dedup" if self.dedup else "rows" if (mode == "max" or self.weighted or mask_pad is not None) else ("mean" if mode == "mean" else "plain")
        self.indices = torch.zeros(nnz, dtype=torch.int64, device=dev)
        # until the first call: one bag that holds every id, the others empty (variable: no id at all)
        self.offsets = torch.full((B + 1,), 0 if self.variable else nnz, dtype=torch.int64, device=dev)
        self.offsets[0] = 0
        if self.fanout is not None and not self.variable:
            self.offsets.copy_(torch.arange(B + 1, dtype=torch.int64, device=dev) * self.fanout)
        self.nnz_dev = torch.zeros(1, dtype=torch.int32, device=dev) if self.variable else None
        self.weights = torch.zeros(nnz, **f32) if self.weighted else None
        # what the graphs' lookups and poolings run on: the staged call, or (partition) what ttemb_compact_bags makes of it
        # as the first node of the forward graph -- kept ids, their bags and weights, the kept count as the count word
        self.ids_k = self.offsets_k = self.weights_k = self.map = self.kept_dev = self._pad_ws = None
        ids, offs, wts, cnt = self.indices, self.offsets, self.weights, self.nnz_dev
        if part:
            self.ids_k = torch.zeros(nnz, dtype=torch.int64, device=dev)
            self.offsets_k = torch.zeros(B + 1, dtype=torch.int64, device=dev)
            self.kept_dev = torch.zeros(1, dtype=torch.int32, device=dev)
            self._pad_ws = torch.zeros(_nat.compact_bags_workspace_bytes(nnz), dtype=torch.uint8, device=dev)   # tile counts
            if self.weighted:   # (the map is the way back of the weight gradient)
                self.weights_k, self.map = torch.zeros(nnz, **f32), torch.full((nnz,), -1, dtype=torch.int32, device=dev)
            ids, offs, wts, cnt = self.ids_k, self.offsets_k, self.weights_k, self.kept_dev
        self.output = torch.zeros((B, D), **f32)
        self.d_output = torch.zeros_like(self.output)
        # a mean that divides the sums (no padding to mask): the "mean" route, and the dedup route of such a mean
        div_mean = self.route == "mean" or (self.dedup and mode == "mean" and mask_pad is None)
        self.d_sums = torch.zeros_like(self.output) if div_mean else None
        self.rows = self.d_rows = self.ones = self.pool_weights = self.argmax = self.d_weights = self.d_weights_out = None
        self.uids = self.inverse = self.perm = self.seg = self.unique_count = self._unique_ws = None
        if self.dedup:   # what ttemb_unique_ids_n writes with every forward replay, and its private workspace
            self.uids = torch.zeros(nnz, dtype=torch.int64, device=dev)
            self.inverse = torch.zeros(nnz, dtype=torch.int32, device=dev)
            self.perm = torch.zeros(nnz, dtype=torch.int32, device=dev)
            self.seg = torch.zeros(nnz + 1, dtype=torch.int64, device=dev)
            self.unique_count = torch.zeros(1, dtype=torch.int32, device=dev)
            self._unique_ws = torch.zeros(_nat.unique_ids_n_workspace_bytes(nnz, module._table_rows), dtype=torch.uint8, device=dev)
        if self.route in ("rows", "dedup"):
            # the memory these routes cost: two [nnz, D] float32 buffers (dedup: the first `unique_count` rows are used)
            self.rows, self.d_rows = torch.zeros((nnz, D), **f32), torch.zeros((nnz, D), **f32)
            self.ones = torch.arange(nnz + 1, dtype=torch.int64, device=dev)   # bags of one; the count word bounds them
            if mode == "max":
                self.argmax = torch.full((B, D), -1, dtype=torch.int32, device=dev)
            else:
                # what the pooling multiplies with: the call's weights, or those ttemb_pad_weights_n makes of them
                self.pool_weights = torch.zeros(nnz, **f32) if mask_pad is not None else wts
            if self.weighted:
                self.d_weights = torch.zeros(nnz, **f32)
                # (masked: the gradient of the masked weights goes through the mask once more, as the eager _PadWeights does;
                #  partition: the gradient of the kept weights goes back to the call's positions, ttemb_expand_kept)
                self.d_weights_out = torch.zeros(nnz, **f32) if self.pad is not None else self.d_weights
        self._lean = _nat.LeanCalls(module._shape, _nat.Workspace())   # private workspace: pinned for the graphs' lifetime
        self.plan = None
        cores = module._cores()
        state = None if module.optimizer in _SGD_LIKE else module._states()
        lr, eps = module._lr_arg(), float(module.eps)   # (capturable: the device word, brought up to date; held by address)
        adam = module._adam_lean()
        self._adam_key = module._adam_key()
        ws, shape = self._lean.ws, module._shape
        rows_route = self.route == "rows"
        # the lookup inside the graphs: (ids, bags, destination) forward, (ids, bags, gradient) backward, its count word
        # (dedup: the distinct ids as bags of one, behind their count)
        by_rows = rows_route or self.dedup
        look_ids, look_cnt = (self.uids, self.unique_count) if self.dedup else (ids, cnt)
        look_offs, look_B = (self.ones, nnz) if by_rows else (offs, B)
        look_out = self.rows if by_rows else self.output
        look_grad = self.d_rows if by_rows else (self.d_sums if self.route == "mean" else self.d_output)

        def lookup_forward():
            if self.exact:
                _nat.forward_exact(shape, _nat.core_ptrs(cores), look_ids, look_offs, look_B, look_out, ws)
            else:   # (variable: the route is chosen from the capacities, on the host; the kernels read the live count)
                self.plan = self._lean.forward(cores, look_ids, look_offs, nnz, look_B, look_out, nnz_dev=look_cnt)

        def lookup_backward():
            if self.exact:
                _nat.backward_exact(shape, _nat.core_ptrs(cores), look_ids, look_offs, look_B, look_grad, ws,
                                    opt_state=None if state is None else _nat.core_ptrs(state), lr=lr, eps=eps,
                                    adam=None if adam is None else (_nat.core_ptrs(adam[0]), adam[1], adam[2]))
            else:
                self._lean.backward(cores, state, look_ids, look_offs, nnz, look_B, look_grad, lr, eps, self.plan, adam,
                                    nnz_dev=look_cnt)

        def fwd():
            if part:   # the first node: pads out, kept count into the word every kernel behind it stops at
                _nat.compact_bags(self.indices, self.offsets, self.weights, self.pad, self.ids_k, self.offsets_k, self.weights_k,
                                  self.map, self.kept_dev, self._pad_ws, nnz_dev=self.nnz_dev)
            if self.dedup:   # the distinct ids of the (kept) ids, their count into the word the lookup stops at
                _nat.unique_ids_n(ids, module._table_rows, self.uids, self.inverse, self.perm, self.seg, self.unique_count,
                                  self._unique_ws, nnz_dev=cnt)
            lookup_forward()
            if self.dedup:
                if mask_pad is not None:
                    _nat.pad_weights(ids, offs, wts, mask_pad, mode == "mean", self.pool_weights, nnz_dev=cnt, counted=True)
                _nat.bag_reduce_mapped(self.rows, self.inverse, self.pool_weights, offs, self.output, ws, nnz_dev=cnt,
                                       counted=True)
                if div_mean:
                    _nat.bag_mean(self.output, self.output, offs)
            elif self.route == "mean":
                _nat.bag_mean(self.output, self.output, offs)
            elif rows_route and mode == "max":
                _nat.bag_max(self.rows, offs, self.output, self.argmax, ws, None if mask_pad is None else ids,
                             mask_pad or 0, nnz_dev=cnt, counted=True)
            elif rows_route:
                if mask_pad is not None:
                    _nat.pad_weights(ids, offs, wts, mask_pad, mode == "mean", self.pool_weights, nnz_dev=cnt, counted=True)
                _nat.bag_reduce(self.rows, self.pool_weights, offs, self.output, ws, nnz_dev=cnt, counted=True)

        def bwd():   # (partition: on the compacted buffers the forward replay left; dedup: on its map, positions and segments)
            if self.dedup:
                if div_mean:
                    _nat.bag_mean(self.d_output, self.d_sums, offs)
                _nat.bag_reduce_mapped_backward(self.d_sums if div_mean else self.d_output, self.pool_weights, self.inverse,
                                                self.perm, self.seg, self.unique_count, offs, self.d_rows, ws,
                                                rows=self.rows if self.weighted else None, d_weights=self.d_weights,
                                                nnz_dev=cnt, counted=True)
            elif self.route == "mean":
                _nat.bag_mean(self.d_output, self.d_sums, offs)
            elif rows_route and mode == "max":
                _nat.bag_max_backward(self.d_output, self.argmax, offs, self.d_rows, nnz_dev=cnt, counted=True)
            elif rows_route:
                _nat.bag_reduce_backward(self.d_output, self.pool_weights, offs, self.d_rows, ws,
                                         rows=self.rows if self.weighted else None, d_weights=self.d_weights, nnz_dev=cnt,
                                         counted=True)
            if by_rows and mode != "max":
                if self.weighted and mask_pad is not None:
                    _nat.pad_weights(ids, offs, self.d_weights, mask_pad, False, self.d_weights_out, nnz_dev=cnt, counted=True)
                elif self.weighted and part:   # a pad's weight gradient is exactly 0
                    _nat.expand_kept(self.d_weights, self.map, self.d_weights_out, nnz_dev=self.nnz_dev)
            lookup_backward()

        # The warm-up runs one backward on a zero gradient outside the capture (workspace growth, LDS-size attributes and size
        # queries happen there).  That leaves SGD / Adagrad as they are; an Adam step on g = 0 advances t, decays m and v and,
        # with weight decay, moves the cores: everything is put back, so that a captured module equals an eager one step for step.
        held = [*cores, *(state or ()), *((*adam[0], module.adam_step) if adam is not None else ())]
        saved = [t.detach().clone() for t in held]
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            fwd()
            bwd()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        _nat.init()   # the pinned fault word exists before anything is captured (a capture must not allocate it)
        self.fwd_graph, self.bwd_graph = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        with _quiet_collector():
            with torch.cuda.graph(self.fwd_graph):
                fwd()
            with torch.cuda.graph(self.bwd_graph):
                bwd()
        with torch.no_grad():
            for t, t0 in zip(held, saved):
                t.copy_(t0)
        self._lr, self._eps = (None if module.capturable else lr), eps
        self._baked = self._pointers()

    def __call__(self, indices: torch.Tensor, offsets: Optional[torch.Tensor] = None,
                 per_sample_weights: Optional[torch.Tensor] = None) -> torch.Tensor:
        m, w = self.module, per_sample_weights
        # every check before anything is launched
        if m.use_cache and not m.warmup:
            raise RuntimeError("the row cache went live after capture_bags(): captured bags do not cover a live cache")
        if m.capturable != (self._lr is None):
            raise RuntimeError("module.capturable was changed after capture_bags(): capture_bags() again")
        if m.padding_idx != self.pad or m.mode != self._module_mode:
            raise RuntimeError("padding_idx / mode of the module are part of the captured graphs: capture_bags() again after "
                               "changing them")
        if ((self._lr is not None and float(m.learning_rate) != self._lr) or float(m.eps) != self._eps
                or m._adam_key() != self._adam_key):
            raise RuntimeError("learning rate / eps are part of the captured backward: capture_bags() again after changing "
                               "them (with OptimType.ADAM also betas, weight_decay and decoupled_weight_decay)")
        if self._pointers() != self._baked:
            raise RuntimeError("tt_cores / optimizer_state were re-allocated after capture_bags() (.to(), .data = ..., "
                               "load_state_dict into new storage): capture_bags() again")
        if (w is not None) != self.weighted:
            raise ValueError("per_sample_weights given to bags captured with weighted=False: capture_bags(weighted=True) "
                             "serves them" if w is not None else
                             "bags captured with weighted=True need per_sample_weights with every call")
        if self.fanout is not None:
            if indices.dim() != 2 or indices.shape[1] != self.fanout:
                raise ValueError(f"bags captured with fanout={self.fanout} take 2-D indices [rows, {self.fanout}], got "
                                 f"{list(indices.shape)}")
            if offsets is not None:
                raise ValueError("offsets has to be None when indices is 2-D (bags of a fixed length)")
            B_live = indices.shape[0]
        else:
            if indices.dim() != 1:
                raise ValueError(f"indices must be 1-D (2-D calls need capture_bags(fanout=N)), got {list(indices.shape)}")
            if offsets is None and not self.variable:
                raise ValueError("offsets is required (bags captured with variable=False and without fanout)")
            if offsets is not None and offsets.dim() != 1:
                raise ValueError("offsets must be 1-D")
            B_live = indices.numel() if offsets is None else offsets.numel() - 1
        n = indices.numel()
        if B_live < 0:
            raise ValueError("offsets must hold B + 1 entries (include_last_offset): got an empty tensor")
        if w is not None and (w.dtype != torch.float32 or w.shape != indices.shape or w.device != indices.device):
            raise ValueError(f"per_sample_weights must be float32 of shape {list(indices.shape)} on {indices.device}, got "
                             f"{w.dtype} {list(w.shape)} on {w.device}")
        if not indices.is_cuda:
            raise RuntimeError("TTEmbeddingBag.forward needs tensors on a ROCm device; there is no CPU fallback")
        if self.variable:
            if n > self.nnz:
                raise ValueError(f"{n} ids exceed the captured capacity nnz={self.nnz}: capture_bags() again with a larger one")
            if B_live > self.B:
                raise ValueError(f"{B_live} bags exceed the captured capacity B={self.B}: capture_bags() again with a larger one")
        elif n != self.nnz or B_live != self.B:
            raise ValueError(f"bags captured with variable=False take exactly nnz={self.nnz} ids in B={self.B} bags, got {n} in "
                             f"{B_live}")
        if self._lr is None:
            m._refresh_lr()   # one fill_ on this stream when learning_rate changed since the last call; no synchronisation
        ids = indices.reshape(-1)
        if not ids.is_contiguous():
            ids = ids.contiguous()
        flat_w = None
        if w is not None:
            flat_w = w.detach().reshape(-1)
            if not flat_w.is_contiguous():
                flat_w = flat_w.contiguous()
        if m.use_cache:   # warm-up: the LFU statistics of a captured step count like those of an eager one
            m.update_cache(ids if ids.dtype == torch.int64 else ids.long())
        if self.variable:
            _nat.stage_bags(ids, offsets, flat_w, self.indices, self.offsets, self.weights, self.nnz_dev,
                            fanout=self.fanout or 0, B_live=B_live)
        else:
            self.indices.copy_(ids)
            if offsets is not None:
                self.offsets.copy_(offsets)
            if flat_w is not None:
                self.weights.copy_(flat_w)
        return _ReplayBags.apply(m._cores()[0], self, w, n, B_live)


# --------------------------------------------------------------------------------------
# the module
# --------------------------------------------------------------------------------------
class TableBatchedTTEmbeddingBag(nn.Module):
    """``num_tables`` TT tables with identical shapes looked up in one call.

    Constructor / attribute contract: reference tt_embeddings_ops.py:446-615.
    ``forward(indices, offsets)`` returns ``[num_tables, B, D]`` sum-pooled bags with
    ``include_last_offset`` semantics (``offsets`` has ``num_tables*B + 1`` entries).

    ``mode`` (keyword-only) and ``forward(..., per_sample_weights=w)`` follow ``torch.nn.functional.embedding_bag``:
    ``mode="sum"`` with ``w`` (float32 ``[nnz]``) pools ``w[i] * row(indices[i])``, ``mode="mean"`` divides each bag sum by
    the bag's length (an empty bag gives zeros).  Weights with ``mode="mean"`` raise ``ValueError``.  Gradients reach the
    cores through every optimiser mode, and ``w.grad`` when ``w`` requires it.

    ``forward(..., mode="max")`` (keyword-only, per call, where ``embedding_bag`` takes it) gives the element-wise maximum
    of each bag's rows -- the first position wins among equal values, a NaN in any kept position makes the element NaN, an
    empty bag gives zeros -- and sends each gradient element to the winner alone; it takes no ``per_sample_weights``.
    ``mode="sum"`` / ``"mean"`` per call run what a module constructed with that mode runs, ``None`` the constructor's mode
    (the constructor itself takes "sum" and "mean" only).  DESIGN.md §4.10.

    ``padding_idx`` (keyword-only; negative counts from the end) follows ``embedding_bag``'s: ids equal to it add nothing to
    their bag, are not counted in a mean and send no gradient (``full_weight()[padding_idx]`` is not zero: a TT table has no
    zero row).  ``forward(indices[rows, N])`` without offsets pools ``rows`` bags of N ids (``per_sample_weights`` then
    ``[rows, N]``).  Routes: DESIGN.md §4.8.
    """

    __constants__ = ["num_tables", "num_embeddings", "embedding_dim", "tt_shape", "tt_rank"]

    def __init__(self, num_tables: int, num_embeddings: int, embedding_dim: int, tt_ranks: List[int],
                 tt_p_shapes: Optional[List[int]] = None, tt_q_shapes: Optional[List[int]] = None,
                 optimizer: OptimType = OptimType.SGD, learning_rate: float = 0.1, eps: float = 1.0e-10,
                 sparse: bool = True, use_cache: bool = False, cache_size: int = 0, hashtbl_size: int = 0,
                 weight_dist: str = "approx-normal", enforce_embedding_dim: bool = False,
                 batch_count: int = 1000, *, deterministic: Optional[bool] = None, mode: str = "sum",
                 padding_idx: Optional[int] = None, betas=(0.9, 0.999), weight_decay: float = 0.0,
                 decoupled_weight_decay: bool = False, capturable: bool = False, dedup: bool = False) -> None:
        super().__init__()
        if dedup and use_cache:
            raise ValueError(
                "dedup=True with use_cache=True is not supported: the row cache partitions the ids of a call by position and "
                "its kernels take no map from positions to distinct ids.  Use use_cache=False (TTEmbeddingBag's default is "
                "True), or dedup=False with the cache.")
        # the default of forward(..., dedup=None): look up each distinct id of a call once (a plain attribute)
        self.dedup = bool(dedup)
        self._last_unique: Optional[torch.Tensor] = None   # int32 [1] on the device: the distinct ids of the last dedup call
        if capturable and use_cache and sparse:
            raise ValueError(
                "use_cache=True with sparse=True and capturable=True is not supported: once cache_populate() makes the row "
                "cache live the cached rows are trained by a per-row kernel that takes the learning rate by value, not from "
                "the device word, and capture() does not cover a live cache anyway.  Use use_cache=False, or capturable=False "
                "with the cache.")
        if optimizer == OptimType.ADAM:
            if not (0.0 <= float(betas[0]) < 1.0 and 0.0 <= float(betas[1]) < 1.0):
                raise ValueError(f"betas must lie in [0, 1), got {tuple(betas)}")
            if float(weight_decay) < 0.0:
                raise ValueError(f"weight_decay must not be negative, got {weight_decay}")
            if use_cache and sparse:
                raise ValueError(
                    "use_cache=True with sparse=True and OptimType.ADAM is not supported: once cache_populate() makes the row "
                    "cache live the cached rows are trained by a per-row optimiser of their own, and there is none for Adam "
                    "(the reference has SGD and row-wise Adagrad only).  Use use_cache=False, or SGD / Adagrad with the cache.")
        # OptimType.ADAM only (plain attributes, read at every step like learning_rate / eps)
        self.betas = (float(betas[0]), float(betas[1]))
        self.weight_decay, self.decoupled_weight_decay = float(weight_decay), bool(decoupled_weight_decay)
        self._adam_cache = None
        self._adam_lean_cache = None
        if mode not in ("sum", "mean"):
            raise ValueError(f"mode must be 'sum' or 'mean', got {mode!r}")
        self.mode = mode
        if padding_idx is not None:
            if not -num_embeddings <= int(padding_idx) < num_embeddings:
                raise ValueError(f"padding_idx must be in [-{num_embeddings}, {num_embeddings}), got {padding_idx}")
            padding_idx = int(padding_idx) % num_embeddings
        # ids equal to it are left out of their bags (a plain attribute: not part of the state dict)
        self.padding_idx: Optional[int] = padding_idx
        # exact mode (``_ExactLookup``): True / False, or None = on for OptimType.EXACT_SGD and whenever
        # torch.are_deterministic_algorithms_enabled() at call time
        self.deterministic = deterministic
        assert num_tables > 0 and num_embeddings > 0 and embedding_dim > 0
        assert num_tables == 1 or not use_cache, "cannot use cache when num_tables != 1"
        T = len(tt_ranks) + 1
        self.batch_count = batch_count  # accepted for compatibility; the kernels do not chunk
        self.tt_p_shapes: List[int] = (list(tt_p_shapes) if tt_p_shapes is not None
                                       else suggested_tt_shapes(num_embeddings, T))
        self.tt_q_shapes: List[int] = (list(tt_q_shapes) if tt_q_shapes is not None else
                                       suggested_tt_shapes(embedding_dim, T,
                                                           allow_round_up=not enforce_embedding_dim))
        assert 2 <= len(self.tt_p_shapes) <= 4
        assert len(self.tt_p_shapes) == T and len(self.tt_q_shapes) == T
        assert all(v > 0 for v in self.tt_p_shapes) and all(v > 0 for v in self.tt_q_shapes)
        assert all(v > 0 for v in tt_ranks)
        assert int(np.prod(np.array(self.tt_p_shapes, dtype=np.int64))) >= num_embeddings
        assert int(np.prod(np.array(self.tt_q_shapes, dtype=np.int64))) == embedding_dim
        self.num_tables, self.tt_ndim = num_tables, T
        self.num_embeddings, self.embedding_dim = num_embeddings, embedding_dim
        # rows the cores address (>= num_embeddings; every lookup clamps an id into them): the key range of the dedup sort
        self._table_rows = int(np.prod(np.array(self.tt_p_shapes, dtype=np.int64)))
        self.tt_ranks = [1] + [int(r) for r in tt_ranks] + [1]
        self.sparse, self.optimizer = sparse, optimizer
        self.learning_rate, self.eps = learning_rate, eps
        _LOG.info("TTEmbeddingBag p=%s q=%s R=%s sparse=%s optimizer=%s lr=%s eps=%s cache=%s/%s/%s",
                  self.tt_p_shapes, self.tt_q_shapes, self.tt_ranks, sparse, optimizer, learning_rate, eps,
                  use_cache, cache_size, hashtbl_size)
        dev = (torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available()
               else torch.device("cpu"))
        strides = [1] * T
        for t in range(T - 2, -1, -1):
            strides[t] = strides[t + 1] * self.tt_p_shapes[t + 1]
        self.register_buffer("L", torch.tensor(strides, dtype=torch.int64))
        self.tt_cores = nn.ParameterList()
        self.optimizer_state = BufferList("optimizer_state")
        for t in range(T):
            shape = [num_tables, self.tt_p_shapes[t],
                     self.tt_ranks[t] * self.tt_q_shapes[t] * self.tt_ranks[t + 1]]
            self.tt_cores.append(nn.Parameter(torch.empty(shape, device=dev, dtype=torch.float32)))
            st_shape = shape if optimizer not in _SGD_LIKE else 0
            self.optimizer_state.append(torch.zeros(st_shape, device=dev, dtype=torch.float32))
        if optimizer == OptimType.ADAM:
            # optimizer_state{t} holds the first moment m; the second moment v and the device step words (one row of four
            # int32 per table: word 0 = t, the steps applied; words 1-3 scratch of the kernels) are registered for ADAM only,
            # so every other optimiser's state_dict keys are what they were
            self.optimizer_state_v = BufferList("optimizer_state_v")
            for c in self.tt_cores:
                self.optimizer_state_v.append(torch.zeros_like(c.data))
            self.register_buffer("adam_step", torch.zeros((num_tables, 4), device=dev, dtype=torch.int32))
        # capturable (torch.optim's name): the rate of every fused step is read from the device word `lr_dev`, which captured
        # graphs hold by address.  Non-persistent: the state_dict keys of every optimiser stay what they are.  `_lr_mirror`: the
        # float last written to the word by the module itself, None = unknown (the word was set from a tensor).
        self.capturable = bool(capturable)
        self._lr_mirror: Optional[float] = None
        if self.capturable:
            self._lr_mirror = float(learning_rate)
            self.register_buffer("lr_dev", torch.full((1,), self._lr_mirror, device=dev, dtype=torch.float32), persistent=False)
        self.reset_parameters(weight_dist)
        self.use_cache = use_cache
        if use_cache:
            if cache_size <= 0:
                cache_size = int(0.1 * num_embeddings)
            if hashtbl_size <= 0:
                hashtbl_size = num_embeddings
            assert hashtbl_size >= cache_size
            self.register_buffer("hashtbl", torch.full((hashtbl_size,), -1, device=dev, dtype=torch.int64))
            self.register_buffer("cache_freq", torch.zeros(hashtbl_size, device=dev, dtype=torch.int64))
            self.register_buffer("cache_state", torch.full((hashtbl_size,), -1, device=dev, dtype=torch.int32))
            self.cache_weight = nn.Parameter(torch.zeros((cache_size, embedding_dim), device=dev,
                                                         dtype=torch.float32))
            if sparse and optimizer not in _SGD_LIKE:
                st = (cache_size, embedding_dim) if optimizer == OptimType.EXACT_ADAGRAD else (cache_size,)
                self.register_buffer("cache_optimizer_state", torch.zeros(st, device=dev, dtype=torch.float32))
            else:
                self.cache_optimizer_state = None
        else:
            self.register_buffer("hashtbl", torch.empty(0, device=dev, dtype=torch.int64))
            self.register_buffer("cache_state", torch.empty(0, device=dev, dtype=torch.int32))
            self.cache_optimizer_state = None
            self.cache_weight = None
        self.warmup = True
        self._dense_grad_out = None
        self._before_weights = None   # set by ttemb_dist.TTDataParallel while an update of the cores is pending
        self._use_windows = True      # num_tables > 1: per-table windows read on the device (False: always split on the host)
        self._pad_partition = True    # padding_idx: drop the pad ids where the grouped kernels serve (False: masked rows only)
        self._last_pad_route: Optional[str] = None   # route of the last padded call ("partition" / "masked")
        self._bucket_filled = False   # set by the backward when it wrote the core gradients into the wrapper's bucket
        self._shape = _nat.make_shape(self.tt_p_shapes, self.tt_q_shapes, self.tt_ranks)
        self._ws = _nat.Workspace()
        self._lean = _nat.LeanCalls(self._shape, self._ws)
        self._use_lean = True   # (tools/host_breakdown.py switches it off to time the general autograd bridge)
        self._core_list: Optional[tuple] = None
        self._state_list: Optional[tuple] = None
        self.register_load_state_dict_post_hook(TableBatchedTTEmbeddingBag._after_load)

    @staticmethod
    def _after_load(module, incompatible_keys) -> None:
        """Checkpoint load path (the reference has none): `warmup` is not part of the
        state dict, so it is re-derived -- a populated cache (`cache_state` holds ranks) is live."""
        if module.use_cache and module.cache_state.numel():
            module.warmup = not bool((module.cache_state >= 0).any().item())

    # ---- weights ------------------------------------------------------------------
    def full_weight(self) -> torch.Tensor:
        assert self.num_tables == 1, "full_weight() only supported for num_tables == 1 for now"
        return tt_matrix_to_full(self.tt_p_shapes, self.tt_q_shapes, self.tt_ranks,
                                 list(self.tt_cores), [1, 0, 2, 3])

    def reset_parameters(self, weight_dist: str) -> None:
        """Initialisers of the reference (tt_embeddings_ops.py:629-808), vectorised."""
        from ttemb_init import init_cores
        init_cores(self, weight_dist)

    def set_learning_rate(self, lr) -> None:
        """The rate of the steps that follow: a float -- or, on a ``capturable=True`` module, a float32 device tensor of one
        element.  A float is only noted here (``learning_rate`` is a plain attribute and may be assigned directly, too); a
        capturable module compares it with the last value it wrote to ``lr_dev`` at the start of every eager backward and
        every captured call and issues one ``fill_`` on the current stream when they differ -- no synchronisation, and
        nothing at all while the rate is unchanged.  A tensor is copied device-to-device into ``lr_dev`` right here, on the
        current stream, without a host synchronisation; ``learning_rate`` then holds that tensor (the host does not know
        the value) and the module does no refresh of its own until a float is set again.  The value in the word is not
        range-checked: a negative or NaN rate does what the arithmetic does.  DESIGN.md §4.12."""
        if isinstance(lr, torch.Tensor):
            if not self.capturable:
                raise TypeError("set_learning_rate(tensor) needs a module built with capturable=True (this one takes its "
                                "rate on the host: pass a float)")
            if lr.dtype != torch.float32 or lr.numel() != 1 or lr.device != self.lr_dev.device:
                raise ValueError(f"a tensor learning rate must be float32 with one element on {self.lr_dev.device}, got "
                                 f"{lr.dtype} {list(lr.shape)} on {lr.device}")
            with torch.no_grad():
                self.lr_dev.copy_(lr.detach().reshape(1))
            self._lr_mirror = None
        self.learning_rate = lr

    def _refresh_lr(self) -> None:
        """Bring ``lr_dev`` up to a float ``learning_rate`` (capturable modules; see ``set_learning_rate``)."""
        lr = self.learning_rate
        if isinstance(lr, torch.Tensor):   # set from a tensor: the word already holds it
            return
        lr = float(lr)
        if lr != self._lr_mirror:
            self._buffers["lr_dev"].fill_(lr)
            self._lr_mirror = lr

    def _lr_arg(self):
        """What a fused step takes as its rate: the float, or a capturable module's device word (brought up to date)."""
        if not self.capturable:
            return float(self.learning_rate)
        self._refresh_lr()
        return self._buffers["lr_dev"]

    def get_params(self):
        params = self.tt_cores
        if self.use_cache:
            params.append(self.cache_weight)
        return params

    # ---- cache --------------------------------------------------------------------
    def reset_cache(self) -> None:
        """Forget every tracked id (the reference's version is dead code: typo at :811)."""
        if self.use_cache:
            self.hashtbl.fill_(-1)
            self.cache_freq.fill_(0)
            self.cache_state.fill_(-1)
            self.warmup = True

    def _fused_probe(self) -> bool:
        """Live cache, default insert: update_cache_state and preprocess_indices_sync of a forward are ONE probe pass
        (``ttemb_preprocess_update``).  The reference-exact one-sweep insert keeps its own launch."""
        return (self.use_cache and not self.warmup and self.num_tables == 1
                and not getattr(self, "lfu_one_sweep_insert", False))

    def update_cache(self, indices: torch.Tensor) -> None:
        if self.use_cache:   # `lfu_one_sweep_insert = True` on the module selects the reference's insert bit for bit
            _nat.cache_update(indices.long().contiguous(), self.hashtbl, self.cache_freq,
                              getattr(self, "lfu_one_sweep_insert", False))

    def cache_populate(self) -> None:
        """Freeze the LFU statistics: the ``cache_size`` hottest ids get their rows
        materialised in ``cache_weight``; ends the warm-up (reference :816-830)."""
        if self.use_cache:
            _nat.cache_populate(self._shape, _nat.core_views(self.tt_cores), self.hashtbl, self.cache_freq,
                                self.cache_state, self.cache_weight.data, self._ws)
            self.warmup = False

    def capture(self, nnz: int, B: int, offsets: Optional[torch.Tensor] = None, *, variable: bool = False) -> CapturedLookup:
        """Lookup whose forward and backward replay captured HIP graphs (see ``CapturedLookup``): of exactly ``nnz`` ids in
        ``B`` bags, or, with ``variable=True``, of any size up to those capacities."""
        self._no_dedup_capture("capture")
        return CapturedLookup(self, nnz, B, offsets, variable)

    def _no_dedup_capture(self, what: str) -> None:
        if self.dedup:
            raise ValueError(f"{what}() on a dedup=True module is not supported: the pass that finds the distinct ids (a sort "
                             "whose temporary storage is sized on the host at call time) is not part of any captured graph.  "
                             "Build the module with dedup=False and pass dedup=True to the eager calls that want it.")

    def capture_bags(self, nnz: int, B: int, *, mode: Optional[str] = None, weighted: bool = False,
                     fanout: Optional[int] = None, variable: bool = False,
                     pad_route: Optional[str] = None, dedup: bool = False) -> CapturedBags:
        """Pooled lookup whose forward and backward replay captured HIP graphs (see ``CapturedBags``): ``mode`` ("sum",
        "mean", "max"; None = the module's), ``weighted`` (every call brings ``per_sample_weights``), the module's
        ``padding_idx``, ``fanout=N`` (2-D ``indices[rows, N]``, ``nnz == B * N``) -- of exactly ``nnz`` ids in ``B`` bags, or,
        with ``variable=True``, of any size up to those capacities.  ``pad_route="partition"`` (a module with
        ``padding_idx``, outside exact mode): the pad ids are dropped on the device as the first node of the forward graph and
        never reach the TT kernels; None / ``"masked"``: they are looked up and pooled with weight 0.  ``dedup=True`` (sum and
        mean bags, outside exact mode, up to 2^20 ids): the forward graph finds the distinct ids of every call on the device
        and the TT kernels look each of them up once (``cap.route == "dedup"``)."""
        self._no_dedup_capture("capture_bags")
        return CapturedBags(self, nnz, B, mode, weighted, fanout, variable, pad_route, dedup)

    # ---- lookup -------------------------------------------------------------------
    def _cores(self) -> tuple:
        """The core Parameters as a tuple (walking the ParameterList costs microseconds per call); rebuilt when ANY of the
        list's Parameter objects is no longer the cached one (2-4 identity tests)."""
        cl = self._core_list
        live = self.tt_cores._parameters
        if cl is None or len(cl) != len(live) or any(c is not live.get(str(t)) for t, c in enumerate(cl)):
            cl = self._core_list = tuple(self.tt_cores)
        return cl

    def _states(self) -> tuple:
        sl = self._state_list
        live = self.optimizer_state._buffers
        if sl is None or len(sl) != len(live) or any(b is not live.get(f"optimizer_state{t}") for t, b in enumerate(sl)):
            sl = self._state_list = tuple(self.optimizer_state)
        return sl

    def _adam_key(self) -> Optional[tuple]:
        if self.optimizer != OptimType.ADAM:
            return None
        # (capturable: the kernels read the rate from lr_dev and ignore the one in ttemb_adam_t)
        return (0.0 if self.capturable else float(self.learning_rate), float(self.eps), self.betas[0], self.betas[1],
                float(self.weight_decay), bool(self.decoupled_weight_decay))

    def _adam_params(self):
        """``ttemb_adam_t`` of the current hyper-parameters (rebuilt when one of them changed)."""
        key = self._adam_key()
        c = self._adam_cache
        if c is None or c[0] != key:
            c = self._adam_cache = (key, _nat.make_adam(key[0], key[1], key[2:4], key[4], key[5]))
        return c[1]

    def _adam_lean(self):
        """None, or (second moments, step words, hyper-parameters) of a one-table module for ``LeanCalls.backward``."""
        if self.optimizer != OptimType.ADAM:
            return None
        c = self._adam_lean_cache   # (second moments, table 0's step words, the buffer they view): rebuilt when a buffer was replaced
        live = self.optimizer_state_v._buffers
        step = self._buffers["adam_step"]
        if (c is None or c[2] is not step or len(c[0]) != len(live)
                or any(b is not live.get(f"optimizer_state_v{t}") for t, b in enumerate(c[0]))):
            c = self._adam_lean_cache = (tuple(self.optimizer_state_v), step[0], step)
        return c[0], c[1], self._adam_params()

    def adam_steps(self) -> List[int]:
        """Steps applied so far, per table (reads the device words: synchronises)."""
        assert self.optimizer == OptimType.ADAM
        return [int(x) for x in self.adam_step[:, 0].tolist()]

    def _exact_requested(self) -> bool:
        if self.deterministic is not None:
            return bool(self.deterministic)
        return self.optimizer == OptimType.EXACT_SGD or torch.are_deterministic_algorithms_enabled()

    def _exact_active(self) -> bool:
        """Whether this call runs in exact mode.  A request the exact kernels cannot serve (a shape outside their domain, a
        live row cache) raises ``RuntimeError`` -- or, under ``torch.use_deterministic_algorithms(True, warn_only=True)``,
        warns and runs the plain lookup."""
        if not self._exact_requested():
            return False
        reason = getattr(self, "_exact_reason", False)
        if reason is False:
            reason = self._exact_reason = _nat.exact_unsupported_reason(self._shape)
        if reason is None and self.use_cache and not self.warmup:
            reason = "a live row cache (after cache_populate()) is not covered by exact mode"
        if reason is None:
            return True
        if torch.is_deterministic_algorithms_warn_only_enabled():
            warnings.warn(f"TTEmbeddingBag: exact mode unavailable, running the plain lookup: {reason}")
            return False
        raise RuntimeError(f"TTEmbeddingBag: exact mode was requested but is unavailable: {reason}")

    def _lookup_one_table(self, table: int, B: int, indices: torch.Tensor, offsets: torch.Tensor, exact: bool) -> torch.Tensor:
        """[B, D] bag sums of one table through the autograd bridge that serves the call."""
        nnz = indices.numel()
        dev = indices.device
        if exact:
            return _ExactLookup.apply(self, table, B, indices, offsets, *self.tt_cores)
        live = self.use_cache and not self.warmup
        if not live:  # rows are derived from `offsets` inside the native calls: no separate launch, no tensor
            if self.num_tables == 1 and self._use_lean and not torch.is_grad_enabled():
                # inference (the drivers' evaluation passes run under no_grad): no autograd node and no plan kept -- a forward
                # that forms its prefix products in the chain kernel then stores none of them (1.08 GB at papers100M, 819 200 ids)
                if self._before_weights is not None:
                    self._before_weights()   # a data-parallel update of the cores is pending: finish it first
                out = torch.empty((B, self.embedding_dim), dtype=torch.float32, device=dev)
                self._lean.forward(self._cores(), indices, offsets, nnz, B, out, keep_plan=False)
                return out
            if self.sparse and self.num_tables == 1 and self._use_lean:
                return _SparseLookup.apply(self._cores()[0], self, indices, offsets, B)
            if not self.sparse and self.num_tables == 1 and self._use_lean and self._dense_grad_out is not None:
                return _BucketLookup.apply(self._cores()[0], self, indices, offsets, B)
            return TTLookupFunction.apply(self, table, B, indices, None, offsets, None, None, None,
                                          *self.tt_cores)
        rowidx = torch.empty(nnz, dtype=torch.int64, device=dev)
        part = torch.empty_like(indices)
        loc = torch.empty(nnz, dtype=torch.int32, device=dev)
        # [number of TT ids, "a cache row occurs twice in this batch"]: both stay on the device.  The second word lets
        # the cache backward update rows with one writer each without float atomics; it comes from per-row position
        # stamps (module scratch, any content, not part of the state dict).
        nnz_tt = torch.empty(2, dtype=torch.int32, device=dev)
        stamp = getattr(self, "_dup_stamp", None)
        if stamp is None or stamp.device != dev or stamp.numel() != self.cache_weight.shape[0]:
            stamp = self._dup_stamp = torch.empty(self.cache_weight.shape[0], dtype=torch.int32, device=dev)
        # the LFU update of this batch rides in the probe pass (_prepare() skipped update_cache for it)
        freq = self.cache_freq if self._fused_probe() else None
        _nat.preprocess(indices, offsets, B, False, self.hashtbl, self.cache_state, part, rowidx, loc, nnz_tt,
                        self._ws, stamp, 0, freq)
        return TTLookupFunction.apply(self, table, B, part, rowidx, offsets, nnz_tt, loc, self.cache_weight,
                                      *self.tt_cores)

    def _bags_of_one(self, nnz: int, dev: torch.device) -> torch.Tensor:
        """offsets 0, 1, ..., nnz (module scratch, grown when a call is longer; not part of the state dict)."""
        a = getattr(self, "_arange", None)
        if a is None or a.device != dev or a.numel() < nnz + 1:
            a = self._arange = torch.arange(nnz + 1, dtype=torch.int64, device=dev)
        return a[: nnz + 1]

    def _weighted_one_table(self, table: int, indices: torch.Tensor, offsets: torch.Tensor, weights: torch.Tensor,
                            exact: bool) -> torch.Tensor:
        """One row per id (the lookup of nnz bags of one, through whichever autograd bridge serves the call), then the
        weighted bag sums of ``_WeightedBag``."""
        nnz = indices.numel()
        rows = self._lookup_one_table(table, nnz, indices, self._bags_of_one(nnz, indices.device), exact)
        return _WeightedBag.apply(rows, weights, offsets, self)

    def _masked_one_table(self, table: int, indices: torch.Tensor, offsets: torch.Tensor, weights: Optional[torch.Tensor],
                          mode: str, exact: bool) -> torch.Tensor:
        """Masked-rows route of a padded call: the bags-of-one rows of every id, pooled with the weights of ``_PadWeights``
        (0 for a pad id, 1 / len' for a mean)."""
        w2 = _PadWeights.apply(weights, indices, offsets, self.padding_idx, mode == "mean")
        return self._weighted_one_table(table, indices, offsets, w2, exact)

    def _dedup_for(self, dedup: Optional[bool], mode: Optional[str], nnz: int) -> bool:
        """Whether this call runs on the dedup route (``dedup``: the per-call keyword, None = the constructor's).  What the
        route does not serve raises ``ValueError`` here, before anything is launched.  DESIGN.md §4.15."""
        if not (self.dedup if dedup is None else bool(dedup)):
            return False
        if (self.mode if mode is None else mode) == "max":
            raise ValueError("dedup with mode='max' is not supported: it needs a max pool that reads its rows through the map "
                             "and a masked sum per distinct id in the backward.  Use dedup=False for max bags.")
        if self.use_cache and not self.warmup:
            raise ValueError("dedup with a live row cache (after cache_populate()) is not supported: the cache partitions the "
                             "ids of a call by position.  Use dedup=False with the cache.")
        if nnz > (1 << 24) or nnz * self.embedding_dim * 4 > (1 << 31):
            raise ValueError(f"dedup: the [{nnz}, {self.embedding_dim}] rows buffer of this call is past one row window (2^24 "
                             "rows or 2 GiB), where the lookup of the distinct ids would run in pieces.  Split the call, or use "
                             "dedup=False.")
        if self._exact_active():
            raise ValueError("dedup in exact mode (OptimType.EXACT_SGD, deterministic=True, "
                             "torch.use_deterministic_algorithms) is not supported: the distinct ids are looked up behind a "
                             "device count and the exact kernels take none.  Use dedup=False in exact mode.")
        return True

    def _dedup_one_table(self, table: int, indices: torch.Tensor, offsets: torch.Tensor, weights: Optional[torch.Tensor],
                         mode: str) -> torch.Tensor:
        """The dedup route on one table: the distinct ids of the call are found on the device (``ttemb_unique_ids``), looked up
        once as bags of one behind their device count, and the bags are pooled through the inverse map (``_MappedBag``) --
        with the call's weights, with the weights of ``_PadWeights`` for a module with ``padding_idx``, without weights for
        a plain sum or mean (a mean divides the sums afterwards).  No host synchronisation."""
        nnz, dev = indices.numel(), indices.device
        uids = torch.empty_like(indices)
        inverse = torch.empty(nnz, dtype=torch.int32, device=dev)
        perm = torch.empty(nnz, dtype=torch.int32, device=dev)
        seg = torch.empty(nnz + 1, dtype=torch.int64, device=dev)
        count = torch.empty(1, dtype=torch.int32, device=dev)
        _nat.unique_ids(indices, self._table_rows, uids, inverse, perm, seg, count, self._ws)
        self._last_unique = count
        ones = self._bags_of_one(nnz, dev)
        if torch.is_grad_enabled():
            # rows past the count have neither a writer nor a reader; without a row index small calls stay on the per-bag kernels
            rows = TTLookupFunction.apply(self, table, nnz, uids, None, ones, count, None, None, *self.tt_cores)
            uniq = (inverse, perm, seg, count)
        else:   # inference: no autograd node, no plan, and the sorted positions are dropped with this frame
            if self._before_weights is not None:
                self._before_weights()   # a data-parallel update of the cores is pending: finish it first
            rows = torch.empty((nnz, self.embedding_dim), dtype=torch.float32, device=dev)
            _nat.forward(self._shape, _nat.core_ptrs(self.tt_cores, table), uids, None, ones, nnz, count, nnz, rows, self._ws, None)
            uniq = (inverse, None, None, count)
        if self.padding_idx is not None:
            weights = _PadWeights.apply(weights, indices, offsets, self.padding_idx, mode == "mean")
        out = _MappedBag.apply(rows, weights, offsets, self, uniq)
        return _BagMean.apply(out, offsets) if mode == "mean" and self.padding_idx is None else out

    def _pad_route(self, nnz: int, B: int, weighted: bool, exact: bool) -> str:
        """"partition" (pad ids never reach the TT kernels) where the row-index lookup of this size runs on the grouped
        kernels; else "masked" (see DESIGN §4.8).  Recorded in ``_last_pad_route``."""
        masked = (weighted or exact or self.num_tables != 1 or (self.use_cache and not self.warmup) or B == 0
                  or not self._pad_partition or not _nat.is_grouped(self._shape, nnz, B, False))
        route = self._last_pad_route = "masked" if masked else "partition"
        return route

    def _drop_padding(self, indices: torch.Tensor, offsets: torch.Tensor):
        """Staging of the partition route: (kept ids, their bags, the compacted offsets, the kept count -- which stays on the
        device: the lookup of the kept ids runs in the row-index form of the live cache)."""
        dev = indices.device
        ids, rows = torch.empty_like(indices), torch.empty_like(indices)
        offs = torch.empty(offsets.numel(), dtype=torch.int64, device=dev)
        kept = torch.empty(1, dtype=torch.int32, device=dev)
        _nat.drop_padding(indices, offsets, self.padding_idx, ids, rows, offs, kept, self._ws)
        return ids, rows, offs, kept

    def _max_one_table(self, table: int, indices: torch.Tensor, offsets: torch.Tensor, exact: bool) -> torch.Tensor:
        """``mode="max"`` on one table.  One row per id (the lookup of bags of one, whichever bridge serves it), then
        ``_BagMax``.  With ``padding_idx``: where ``_pad_route`` answers "partition", the pad ids are dropped first and only
        the kept ids are looked up; else every id is looked up and ``_BagMax`` skips the pad positions."""
        nnz, pad = indices.numel(), self.padding_idx
        ones = self._bags_of_one(nnz, indices.device)
        if pad is not None and self._pad_route(nnz, offsets.numel() - 1, False, exact) == "partition":
            ids, _, offs, kept = self._drop_padding(indices, offsets)   # (the kept ids' bags: not needed, one row per id)
            # kept id i -> row i of the rows buffer; the rows past the kept count have no writer and no reader (`offs` ends
            # at the kept count)
            rows = TTLookupFunction.apply(self, table, nnz, ids, ones[:nnz], ones, kept, None, None, *self.tt_cores)
            return _BagMax.apply(rows, offs, self, None, 0)
        rows = self._lookup_one_table(table, nnz, indices, ones, exact)
        if pad is None:
            return _BagMax.apply(rows, offsets, self, None, 0)
        return _BagMax.apply(rows, offsets, self, indices, pad)   # masked route: the pad positions are skipped

    def _fixed_bags(self, indices: torch.Tensor, offsets: Optional[torch.Tensor], weights: Optional[torch.Tensor]):
        """2-D ``indices[rows, N]`` without offsets: ``rows`` bags of N ids (for several tables, the num_tables * B bags
        in table-major order) -> the flat ids, offsets 0, N, 2N, ... (module scratch on the device) and flat weights."""
        if indices.dim() == 2:
            if offsets is not None:
                raise ValueError("offsets has to be None when indices is 2-D (bags of a fixed length)")
            rows, N = indices.shape
            if rows % self.num_tables != 0:
                raise ValueError(f"2-D indices: {rows} rows are not num_tables ({self.num_tables}) * B bags")
            if weights is not None and tuple(weights.shape) != (rows, N):
                raise ValueError(f"per_sample_weights must have the shape of indices {[rows, N]}, got {list(weights.shape)}")
            key = (rows, N, indices.device)
            if getattr(self, "_fixed_key", None) != key:
                self._fixed_offsets = torch.arange(rows + 1, dtype=torch.int64, device=indices.device) * N
                self._fixed_key = key
            return indices.reshape(-1), self._fixed_offsets, (None if weights is None else weights.reshape(-1))
        if indices.dim() != 1:
            raise ValueError(f"indices must be 1-D (with offsets) or 2-D (without), got {indices.dim()}-D")
        if offsets is None:
            raise ValueError("offsets is required when indices is 1-D")
        return indices, offsets, weights

    def _prepare(self, indices: torch.Tensor, offsets: Optional[torch.Tensor], weights: Optional[torch.Tensor],
                 mode: Optional[str]):
        """The prologue of every call: the arguments are checked before anything is launched, then
        ``(mode, ids, offsets, weights, B, exact)`` -- the effective mode (the per-call one, else the constructor's), 1-D
        contiguous int64 ids and offsets, flat float32 weights or None, the bags per table, whether exact mode serves the
        call -- with the LFU statistics of a warming cache updated."""
        if mode is None:
            mode = self.mode
        elif mode not in ("sum", "mean", "max"):
            raise ValueError(f"mode must be 'sum', 'mean' or 'max', got {mode!r}")
        if weights is not None and mode == "max":
            raise ValueError("per_sample_weights was not None: weighted bags are only supported with mode='sum' "
                             "(as in torch.nn.functional.embedding_bag)")
        if offsets is None or indices.dim() != 1:
            indices, offsets, weights = self._fixed_bags(indices, offsets, weights)
        if not indices.is_cuda:
            raise RuntimeError("TTEmbeddingBag.forward needs tensors on a ROCm device; there is no CPU fallback")
        if weights is not None:
            if mode != "sum":
                raise ValueError("per_sample_weights was not None: weighted bags are only supported with mode='sum' "
                                 "(as in torch.nn.functional.embedding_bag)")
            _nat._check_weights(weights, indices.numel(), indices)
            weights = weights.contiguous()
        if indices.dtype != torch.int64 or not indices.is_contiguous():
            indices = indices.long().contiguous()
        if offsets.dtype != torch.int64 or not offsets.is_contiguous():
            offsets = offsets.long().contiguous()
        B = offsets.numel() - 1
        if self.num_tables != 1:
            assert B % self.num_tables == 0
            B //= self.num_tables
        if self.use_cache and not self._fused_probe():   # (fused: the LFU update rides in the probe pass of the lookup)
            self.update_cache(indices)
        return mode, indices, offsets, weights, B, self._exact_active()

    def _route(self, mode: str, indices: torch.Tensor, offsets: torch.Tensor, weights: Optional[torch.Tensor], B: int,
               exact: bool, dedup: bool = False) -> torch.Tensor:
        """A prepared call to the kernels that serve it: [B, D] of a module with one table, else [num_tables, B, D].  Reads
        the mode it is given, never ``self.mode``."""
        T = self.num_tables
        if dedup:   # (``_dedup_for`` has refused max bags, exact mode and a live cache)
            one = lambda k, ids, offs, w: self._dedup_one_table(k, ids, offs, w, mode)
        elif mode == "max":
            one = lambda k, ids, offs, w: self._max_one_table(k, ids, offs, exact)
        elif self.padding_idx is not None:
            if self._pad_route(indices.numel(), B, weights is not None, exact) == "partition":
                # pad ids never reach the TT kernels: the lookup runs on the kept ids and the compacted bags
                ids, rows, offs, kept = self._drop_padding(indices, offsets)
                out = TTLookupFunction.apply(self, 0, B, ids, rows, offs, kept, None, None, *self.tt_cores)
                return _BagMean.apply(out, offs) if mode == "mean" else out
            one = lambda k, ids, offs, w: self._masked_one_table(k, ids, offs, w, mode, exact)
        elif weights is not None:
            one = lambda k, ids, offs, w: self._weighted_one_table(k, ids, offs, w, exact)
        else:   # the plain bag sums (no host synchronisation wherever the lookup has none); a mean divides them by the lengths
            sums = (self._lookup_one_table(0, B, indices, offsets, exact) if T == 1
                    else self._lookup_tables(indices, offsets, B, exact))
            return _BagMean.apply(sums, offsets) if mode == "mean" else sums
        return one(0, indices, offsets, weights) if T == 1 else self._each_table(one, indices, offsets, B, weights)

    def forward(self, indices: torch.Tensor, offsets: Optional[torch.Tensor] = None, warmup: bool = True, *,
                per_sample_weights: Optional[torch.Tensor] = None, mode: Optional[str] = None,
                dedup: Optional[bool] = None) -> torch.Tensor:
        """``dedup`` (keyword-only; None = the constructor's ``dedup``): look up each DISTINCT id of the call once -- the
        distinct ids are found on the device without a host synchronisation, their rows are pooled through the inverse map
        and the backward sums each distinct id's gradient before the TT backward.  Same results as
        ``dedup=False`` up to fp32 summation order.  It costs a sort of the ids and pays where ids repeat.  Measured on the
        products table (409 600 ids, fused SGD step, ``profiles/r16_dedup.txt``): a mean over a 40 960 x 10 neighbour block
        is faster at every duplication level (0.42x the plain step even with every id distinct); a weighted sum over that
        block from about 40 % distinct ids down (1.20x at 100 %, 1.02x at 43 %, 0.95x at 25 %, 0.81x at 6 %); weighted
        bags of one never at the levels measured (1.51x at 100 %, 1.01x at 6 %).  Refused with ``ValueError``: ``mode="max"``, exact mode, a live row cache, a call whose ``[nnz, D]``
        rows buffer is past one row window (2^24 rows or 2 GiB)."""
        # `warmup` is accepted and ignored, like the reference (it reads self.warmup, :862)
        dedup = self._dedup_for(dedup, mode, indices.numel())
        out = self._route(*self._prepare(indices, offsets, per_sample_weights, mode), dedup)
        return out.unsqueeze(0) if self.num_tables == 1 else out

    def _each_table(self, one, indices: torch.Tensor, offsets: torch.Tensor, B: int,
                    weights: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Several tables where no kernel reads the table bounds on the device: the id list is split on the host (one
        synchronisation) and ``one(table, ids, offsets, weights)`` gives each table's [B, D], stacked to [num_tables, B, D]."""
        if B == 0:
            return torch.zeros((self.num_tables, 0, self.embedding_dim), dtype=torch.float32, device=indices.device)
        bounds = offsets[:: B].tolist()
        outs = []
        for k in range(self.num_tables):
            lo, hi = int(bounds[k]), int(bounds[k + 1])
            offs_k = (offsets[k * B:(k + 1) * B + 1] - lo).contiguous()
            outs.append(one(k, indices[lo:hi].contiguous(), offs_k, None if weights is None else weights[lo:hi]))
        return torch.stack(outs, 0)

    def _lookup_tables(self, indices: torch.Tensor, offsets: torch.Tensor, B: int, exact: bool) -> torch.Tensor:
        """[num_tables, B, D] bag sums of a module with several tables."""
        # every table is a window of the id list, its bounds read from `offsets` on the device (no host synchronisation) -- when the
        # grouped kernels serve the shape; else one plain lookup per table of the host-split id list
        nnz = indices.numel()
        if (not exact and not self.use_cache and self._use_windows and nnz > 0 and B > 0
                and _nat.window_workspace_bytes(self._shape, _nat.OP_BACKWARD, nnz, offsets.numel() - 1, B) >= 0):
            return _TablesLookup.apply(self, B, indices, offsets, *self.tt_cores)
        return self._each_table(lambda k, ids, offs, w: self._lookup_one_table(k, B, ids, offs, exact), indices, offsets, B)


class TTEmbeddingBag(TableBatchedTTEmbeddingBag):
    """TT embedding lookup for exactly one table; ``forward`` returns ``[B, D]``
    (reference: tt_embeddings_ops.py:918-965)."""

    def __init__(self, num_embeddings: int, embedding_dim: int, tt_ranks: List[int],
                 tt_p_shapes: Optional[List[int]] = None, tt_q_shapes: Optional[List[int]] = None,
                 optimizer: OptimType = OptimType.SGD, learning_rate: float = 0.1, eps: float = 1.0e-10,
                 sparse: bool = True, use_cache: bool = True, cache_size: int = 0, hashtbl_size: int = 0,
                 weight_dist: str = "approx-normal", enforce_embedding_dim: bool = False,
                 batch_count: int = 1000, *, deterministic: Optional[bool] = None, mode: str = "sum",
                 padding_idx: Optional[int] = None, betas=(0.9, 0.999), weight_decay: float = 0.0,
                 decoupled_weight_decay: bool = False, capturable: bool = False, dedup: bool = False) -> None:
        super().__init__(1, num_embeddings, embedding_dim, tt_ranks, tt_p_shapes, tt_q_shapes, optimizer,
                         learning_rate, eps, sparse, use_cache, cache_size, hashtbl_size, weight_dist,
                         enforce_embedding_dim, batch_count, deterministic=deterministic, mode=mode,
                         padding_idx=padding_idx, betas=betas, weight_decay=weight_decay,
                         decoupled_weight_decay=decoupled_weight_decay, capturable=capturable, dedup=dedup)

    def forward(self, indices: torch.Tensor, offsets: Optional[torch.Tensor] = None, warmup: bool = True, *,
                per_sample_weights: Optional[torch.Tensor] = None, mode: Optional[str] = None,
                dedup: Optional[bool] = None) -> torch.Tensor:
        # same result as the reference's ``super().forward(...)[0]`` (:960-965) without the
        # [1, B, D] view: selecting table 0 would cost a zero-fill + copy of B*D floats in backward
        dedup = self._dedup_for(dedup, mode, indices.numel())
        return self._route(*self._prepare(indices, offsets, per_sample_weights, mode), dedup)
