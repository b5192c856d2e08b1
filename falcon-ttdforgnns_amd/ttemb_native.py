"""ctypes binding of ``libttemb_hip.so`` (the C ABI declared in ``include/ttemb.h``).

This is the only place Python touches the native library.  Everything here takes
``torch`` tensors living on a ROCm device, passes raw ``data_ptr()`` values and the
current HIP stream, and raises ``RuntimeError`` with the library's message on a
non-zero status -- the same error convention as the reference's pybind module
(``c10::Error`` -> ``RuntimeError``; FBTT/tt_embeddings.cpp:131-161).

There is no CPU fallback: if the shared library is missing the import of this
module fails, and CPU tensors are rejected.
"""
from __future__ import annotations

import ctypes
import os
from typing import List, Optional, Sequence

import torch  # noqa: F401  (loads torch's libamdhip64.so.7 first, so we share one HIP runtime)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TTEMB_LIB") or os.path.join(_HERE, "lib", "libttemb_hip.so")

MAX_CORES = 4
ABI_VERSION = 4
OP_FORWARD, OP_BACKWARD, OP_PREPROCESS, OP_CACHE_POPULATE = 0, 1, 2, 3
PATH_AUTO, PATH_GENERIC, PATH_FAST3, PATH_PER_BAG = 0, 1, 2, 3

# every symbol include/ttemb.h declares (tests check the library exports all of them)
EXPORTED_SYMBOLS = (
    "ttemb_abi_version", "ttemb_last_error", "ttemb_workspace_bytes", "ttemb_plan_bytes", "ttemb_set_path",
    "ttemb_profile_enable", "ttemb_profile_read", "ttemb_kernel_family", "ttemb_set_piece_limits", "ttemb_set_wide_slab_min_ids", "ttemb_init", "ttemb_status", "ttemb_set_spin_limit", "ttemb_grouping_layout",
    "ttemb_forward", "ttemb_forward_group", "ttemb_forward_lookup", "ttemb_backward_dense", "ttemb_backward_sgd", "ttemb_backward_adagrad",
    "ttemb_window_workspace_bytes", "ttemb_forward_window", "ttemb_backward_dense_window", "ttemb_backward_sgd_window", "ttemb_backward_adagrad_window",
    "ttemb_sgd_step", "ttemb_sgd_step_guarded", "ttemb_adagrad_step", "ttemb_cache_update", "ttemb_cache_update_one_sweep", "ttemb_cache_populate",
    "ttemb_preprocess", "ttemb_preprocess_update", "ttemb_cache_forward", "ttemb_cache_backward_sgd",
    "ttemb_cache_backward_dense", "ttemb_cache_backward_rowwise_adagrad",
    "ttemb_exact_workspace_bytes", "ttemb_exact_plan_bytes", "ttemb_set_exact_grid", "ttemb_forward_exact",
    "ttemb_backward_dense_exact", "ttemb_backward_sgd_exact", "ttemb_backward_adagrad_exact",
    "ttemb_bag_workspace_bytes", "ttemb_bag_reduce", "ttemb_bag_reduce_backward", "ttemb_bag_mean",
    "ttemb_drop_padding_workspace_bytes", "ttemb_drop_padding", "ttemb_pad_weights",
    "ttemb_backward_adam", "ttemb_backward_adam_window", "ttemb_backward_adam_exact", "ttemb_adam_step",
    "ttemb_bag_max_workspace_bytes", "ttemb_bag_max", "ttemb_bag_max_backward",
    "ttemb_stage_call",
    "ttemb_backward_step", "ttemb_backward_step_window", "ttemb_backward_step_exact", "ttemb_flat_step",
)

# every symbol include/ttemb_bags.h declares (captured pooled lookups; ttemb.h includes that header)
BAGS_SYMBOLS = ("ttemb_stage_bags", "ttemb_bag_reduce_n", "ttemb_bag_reduce_backward_n", "ttemb_bag_max_n",
                "ttemb_bag_max_backward_n", "ttemb_pad_weights_n")

# every symbol include/ttemb_pads.h declares (captured padded bags on the partition route; ttemb.h includes that header)
PADS_SYMBOLS = ("ttemb_compact_bags_workspace_bytes", "ttemb_compact_bags", "ttemb_expand_kept")

# every symbol include/ttemb_unique.h declares (the dedup route of the pooled lookups; ttemb.h includes that header)
UNIQUE_SYMBOLS = ("ttemb_unique_ids_workspace_bytes", "ttemb_unique_ids", "ttemb_bag_reduce_mapped",
                  "ttemb_bag_reduce_mapped_backward")

# every symbol include/ttemb_unique_n.h declares (the dedup route inside captured graphs; ttemb.h includes that header)
UNIQUE_N_SYMBOLS = ("ttemb_unique_ids_n_workspace_bytes", "ttemb_unique_ids_n", "ttemb_bag_reduce_mapped_n",
                    "ttemb_bag_reduce_mapped_backward_n")


class Shape(ctypes.Structure):
    """Mirror of ``ttemb_shape_t``."""
    _fields_ = [("T", ctypes.c_int32), ("p", ctypes.c_int32 * MAX_CORES),
                ("q", ctypes.c_int32 * MAX_CORES), ("R", ctypes.c_int32 * (MAX_CORES + 1))]


class AdamParams(ctypes.Structure):
    """Mirror of ``ttemb_adam_t``: the hyper-parameters of the fused Adam / AdamW step."""
    _fields_ = [("lr", ctypes.c_float), ("eps", ctypes.c_float), ("weight_decay", ctypes.c_float),
                ("decoupled", ctypes.c_int32), ("beta1", ctypes.c_double), ("beta2", ctypes.c_double)]


class StepDesc(ctypes.Structure):
    """Mirror of ``ttemb_step_t``: the step of a call that takes its learning rate from a device word."""
    _fields_ = [("kind", ctypes.c_int32), ("lr_dev", ctypes.c_void_p), ("eps", ctypes.c_float), ("state", ctypes.c_void_p),
                ("state2", ctypes.c_void_p), ("adam_step", ctypes.c_void_p), ("adam", ctypes.c_void_p)]


STEP_SGD, STEP_ADAGRAD, STEP_ADAM = 0, 1, 2


def _lr_word(lr: torch.Tensor) -> int:
    if lr.dtype != torch.float32 or lr.numel() != 1 or not lr.is_cuda:
        raise ValueError("a device learning rate is a float32 tensor of one element on a ROCm device, got "
                         f"{lr.dtype} {list(lr.shape)} on {lr.device}")
    return lr.data_ptr()


def _fill_desc(lr: torch.Tensor, eps: float, kind: int, hp=None, state=None, state2=None, words=None) -> StepDesc:
    """The one place a ``StepDesc`` is filled.  ``state`` / ``state2``: pointer arrays (a flat step passes none: its arrays
    are arguments of the call); the caller keeps everything the descriptor points at alive."""
    d = StepDesc()
    d.kind, d.lr_dev, d.eps = kind, _lr_word(lr), float(eps)
    if state is not None:
        d.state = ctypes.addressof(state)
    if state2 is not None:
        d.state2 = ctypes.addressof(state2)
    if hp is not None:
        d.adam, d.adam_step = ctypes.addressof(hp), words
    return d


def _kind(state, hp) -> int:
    return STEP_ADAM if hp is not None else (STEP_ADAGRAD if state is not None else STEP_SGD)


def step_desc(lr: torch.Tensor, eps: float = 0.0, state=None, adam=None):
    """``ttemb_step_t`` of a step whose rate is the device word ``lr``: SGD (no ``state``), Adagrad (``state``: a pointer
    array or tensors) or Adam (``state`` the first moment, ``adam = (exp_avg_sq, step words, AdamParams)``; the rate in the
    ``AdamParams`` is ignored).  Returns ``(descriptor, keep)``: ``keep`` holds what the descriptor points at."""
    st = None if state is None else _ptr_array(state)
    st2, words, hp = (None, None, None) if adam is None else (_ptr_array(adam[0]), _ptr(adam[1]), adam[2])
    return _fill_desc(lr, eps, _kind(st, hp), hp, st, st2, words), (st, st2, adam, lr)


class Step:
    """One optimiser step, as every stepping call below takes it.  ``lr``: a float, or a float32[1] device tensor (the rate
    is then read on the device: the descriptor calls); ``state``: None for SGD, the Adagrad state or Adam's first moment
    (tensors or a pointer array; one tensor for a flat step); ``adam = (exp_avg_sq, step words, AdamParams)`` makes it an
    Adam step, whose by-value rate and eps are the ``AdamParams``' own."""
    __slots__ = ("lr", "eps", "state", "state2", "words", "hp")

    def __init__(self, lr, eps: float = 0.0, state=None, adam=None) -> None:
        self.lr, self.eps, self.state = lr, eps, state
        self.state2, self.words, self.hp = adam if adam is not None else (None, None, None)

    @property
    def adam(self):
        return None if self.hp is None else (self.state2, self.words, self.hp)


def make_adam(lr: float, eps: float, betas=(0.9, 0.999), weight_decay: float = 0.0, decoupled: bool = False) -> AdamParams:
    return AdamParams(float(lr), float(eps), float(weight_decay), 1 if decoupled else 0, float(betas[0]), float(betas[1]))


def new_adam_step(device) -> torch.Tensor:
    """The device words of an Adam state (``ttemb_adam_t``'s ``step``): int32[4], word 0 = the steps applied so far."""
    return torch.zeros(4, dtype=torch.int32, device=device)


def make_shape(p: Sequence[int], q: Sequence[int], ranks: Sequence[int]) -> Shape:
    """``ranks`` may be the inner ranks (T-1 values) or the padded list (T+1 values)."""
    T = len(p)
    r = [int(x) for x in ranks]
    if len(r) == T - 1:
        r = [1] + r + [1]
    if len(q) != T or len(r) != T + 1 or not (2 <= T <= MAX_CORES):
        raise RuntimeError(f"inconsistent TT shape: p={list(p)} q={list(q)} ranks={list(ranks)}")
    s = Shape()
    s.T = T
    for t in range(T):
        s.p[t], s.q[t] = int(p[t]), int(q[t])
    for t in range(T + 1):
        s.R[t] = r[t]
    return s


def _load() -> ctypes.CDLL:
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C falcon-ttdforgnns_amd/csrc`.  There is no CPU fallback for the TT embedding path.")
    lib = ctypes.CDLL(LIB_PATH)
    vp, i64, i32, f32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_float
    shp = ctypes.POINTER(Shape)
    lib.ttemb_abi_version.restype = ctypes.c_int
    if lib.ttemb_abi_version() != ABI_VERSION:   # (before any other symbol is bound: a stale library fails HERE, with this message)
        raise ImportError(f"{LIB_PATH}: ABI version {lib.ttemb_abi_version()}, this binding needs {ABI_VERSION} -- rebuild the library "
                          "(`make -C falcon-ttdforgnns_amd/csrc`)")
    lib.ttemb_last_error.restype = ctypes.c_char_p
    lib.ttemb_workspace_bytes.restype = i64
    lib.ttemb_workspace_bytes.argtypes = [shp, i32, i64, i64]
    lib.ttemb_set_path.argtypes = [i32]
    lib.ttemb_profile_enable.argtypes = [i32]
    lib.ttemb_profile_read.argtypes = [i32, ctypes.POINTER(ctypes.c_float)]
    lib.ttemb_kernel_family.argtypes = [shp, i64, i64, i32]
    lib.ttemb_set_piece_limits.argtypes = [i64, i64]
    lib.ttemb_set_spin_limit.argtypes = [i64]
    lib.ttemb_grouping_layout.argtypes = [shp, i64, ctypes.POINTER(ctypes.c_int64)]
    lib.ttemb_set_wide_slab_min_ids.argtypes = [i64]
    lib.ttemb_status.argtypes = []
    lib.ttemb_init.argtypes = []
    lib.ttemb_plan_bytes.restype = i64
    lib.ttemb_plan_bytes.argtypes = [shp, i64]
    lib.ttemb_forward.argtypes = [shp, vp, vp, vp, vp, i64, vp, i64, vp, vp, i64, vp, i64, vp]
    lib.ttemb_forward_group.argtypes = lib.ttemb_forward.argtypes
    lib.ttemb_forward_lookup.argtypes = lib.ttemb_forward.argtypes
    lib.ttemb_backward_dense.argtypes = [shp, vp, vp, vp, vp, i64, vp, i64, vp, vp, vp, i64, vp, i64, vp]
    lib.ttemb_backward_sgd.argtypes = [shp, vp, vp, vp, vp, i64, vp, i64, vp, f32, vp, i64, vp, i64, vp]
    lib.ttemb_backward_adagrad.argtypes = [shp, vp, vp, vp, vp, vp, i64, vp, i64, vp, f32, f32, vp, i64, vp, i64, vp]
    lib.ttemb_window_workspace_bytes.restype = i64
    lib.ttemb_window_workspace_bytes.argtypes = [shp, i32, i64, i64, i64]
    lib.ttemb_forward_window.argtypes = [shp, vp, vp, vp, i64, i64, i64, i64, vp, vp, i64, vp]
    lib.ttemb_backward_dense_window.argtypes = [shp, vp, vp, vp, i64, i64, i64, i64, vp, vp, vp, i64, vp]
    lib.ttemb_backward_sgd_window.argtypes = [shp, vp, vp, vp, i64, i64, i64, i64, vp, f32, vp, i64, vp]
    lib.ttemb_backward_adagrad_window.argtypes = [shp, vp, vp, vp, vp, i64, i64, i64, i64, vp, f32, f32, vp, i64, vp]
    lib.ttemb_sgd_step.argtypes = [vp, vp, i64, f32, vp]
    lib.ttemb_sgd_step_guarded.argtypes = [vp, vp, i64, f32, vp, vp]
    lib.ttemb_adagrad_step.argtypes = [vp, vp, vp, i64, f32, f32, vp]
    lib.ttemb_cache_update.argtypes = [vp, i64, vp, vp, i64, vp]
    lib.ttemb_cache_update_one_sweep.argtypes = [vp, i64, vp, vp, i64, vp]
    lib.ttemb_cache_populate.argtypes = [shp, vp, vp, vp, vp, i64, vp, i64, vp, i64, vp]
    lib.ttemb_preprocess.argtypes = [vp, vp, i64, i64, i32, vp, vp, i64, vp, vp, vp, vp, vp, i32, vp, i64, vp]
    lib.ttemb_preprocess_update.argtypes = [vp, vp, i64, i64, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, i64, vp]
    lib.ttemb_cache_forward.argtypes = [vp, vp, vp, i64, vp, i64, vp, i64, vp, vp]
    lib.ttemb_cache_backward_sgd.argtypes = [vp, vp, i64, vp, i64, vp, i64, f32, vp, vp, vp]
    lib.ttemb_cache_backward_dense.argtypes = [vp, vp, i64, vp, i64, vp, i64, i64, vp, vp, vp]
    lib.ttemb_cache_backward_rowwise_adagrad.argtypes = [vp, vp, i64, vp, i64, vp, i64, f32, f32, vp, vp, vp]
    lib.ttemb_exact_workspace_bytes.restype = i64
    lib.ttemb_exact_workspace_bytes.argtypes = [shp, i64, i64]
    lib.ttemb_exact_plan_bytes.restype = i64
    lib.ttemb_exact_plan_bytes.argtypes = [shp, i64]
    lib.ttemb_set_exact_grid.argtypes = [i32]
    lib.ttemb_forward_exact.argtypes = [shp, vp, vp, vp, i64, i64, vp, vp, i64, vp, i64, vp]
    lib.ttemb_backward_dense_exact.argtypes = [shp, vp, vp, vp, i64, i64, vp, vp, vp, i64, vp, i64, vp]
    lib.ttemb_backward_sgd_exact.argtypes = [shp, vp, vp, vp, i64, i64, vp, f32, vp, i64, vp, i64, vp]
    lib.ttemb_backward_adagrad_exact.argtypes = [shp, vp, vp, vp, vp, i64, i64, vp, f32, f32, vp, i64, vp, i64, vp]
    adm = ctypes.POINTER(AdamParams)
    lib.ttemb_backward_adam.argtypes = [shp, vp, vp, vp, vp, vp, vp, vp, i64, vp, i64, vp, adm, vp, i64, vp, i64, vp]
    lib.ttemb_backward_adam_window.argtypes = [shp, vp, vp, vp, vp, vp, vp, i64, i64, i64, i64, vp, adm, vp, i64, vp]
    lib.ttemb_backward_adam_exact.argtypes = [shp, vp, vp, vp, vp, vp, vp, i64, i64, vp, adm, vp, i64, vp, i64, vp]
    lib.ttemb_adam_step.argtypes = [vp, vp, vp, vp, vp, i64, f32, adm, vp, vp]
    lib.ttemb_bag_workspace_bytes.restype = i64
    lib.ttemb_bag_workspace_bytes.argtypes = [i64, i64, i64]
    lib.ttemb_bag_reduce.argtypes = [vp, vp, vp, i64, i64, i64, vp, vp, i64, vp]
    lib.ttemb_bag_reduce_backward.argtypes = [vp, vp, vp, vp, i64, i64, i64, vp, vp, vp, i64, vp]
    lib.ttemb_bag_mean.argtypes = [vp, vp, vp, i64, i64, vp]
    lib.ttemb_bag_max_workspace_bytes.restype = i64
    lib.ttemb_bag_max_workspace_bytes.argtypes = [i64, i64, i64]
    lib.ttemb_bag_max.argtypes = [vp, vp, i64, vp, i64, i64, i64, vp, vp, vp, i64, vp]
    lib.ttemb_bag_max_backward.argtypes = [vp, vp, vp, i64, i64, i64, vp, vp]
    lib.ttemb_drop_padding_workspace_bytes.restype = i64
    lib.ttemb_drop_padding_workspace_bytes.argtypes = [i64, i64]
    lib.ttemb_drop_padding.argtypes = [vp, vp, i64, i64, i64, vp, vp, vp, vp, vp, i64, vp]
    lib.ttemb_pad_weights.argtypes = [vp, vp, vp, i64, i64, i64, i32, vp, vp]
    lib.ttemb_stage_call.argtypes = [vp, i32, i64, vp, i32, i64, vp, i64, vp, i64, vp, vp]
    lib.ttemb_stage_bags.argtypes = [vp, i32, i64, vp, i32, i64, i64, vp, vp, i64, vp, i64, vp, vp, vp]
    lib.ttemb_bag_reduce_n.argtypes = [vp, vp, vp, i64, vp, i64, i64, vp, vp, i64, vp]
    lib.ttemb_bag_reduce_backward_n.argtypes = [vp, vp, vp, vp, i64, vp, i64, i64, vp, vp, vp, i64, vp]
    lib.ttemb_bag_max_n.argtypes = [vp, vp, i64, vp, i64, vp, i64, i64, vp, vp, vp, i64, vp]
    lib.ttemb_bag_max_backward_n.argtypes = [vp, vp, vp, i64, vp, i64, i64, vp, vp]
    lib.ttemb_pad_weights_n.argtypes = [vp, vp, vp, i64, vp, i64, i64, i32, vp, vp]
    lib.ttemb_compact_bags_workspace_bytes.restype = i64
    lib.ttemb_compact_bags_workspace_bytes.argtypes = [i64]
    lib.ttemb_compact_bags.argtypes = [vp, vp, vp, i64, vp, i64, i64, vp, vp, vp, vp, vp, vp, i64, vp]
    lib.ttemb_expand_kept.argtypes = [vp, vp, i64, vp, vp, vp]
    lib.ttemb_unique_ids_workspace_bytes.restype = i64
    lib.ttemb_unique_ids_workspace_bytes.argtypes = [i64, i64]
    lib.ttemb_unique_ids.argtypes = [vp, i64, i64, vp, vp, vp, vp, vp, vp, i64, vp]
    lib.ttemb_bag_reduce_mapped.argtypes = [vp, i64, vp, vp, vp, i64, i64, i64, vp, vp, i64, vp]
    lib.ttemb_bag_reduce_mapped_backward.argtypes = [vp, vp, vp, i64, vp, vp, vp, vp, vp, i64, i64, i64, vp, vp, vp, i64, vp]
    lib.ttemb_unique_ids_n_workspace_bytes.restype = i64
    lib.ttemb_unique_ids_n_workspace_bytes.argtypes = [i64, i64]
    lib.ttemb_unique_ids_n.argtypes = [vp, i64, vp, i64, vp, vp, vp, vp, vp, vp, i64, vp]
    lib.ttemb_bag_reduce_mapped_n.argtypes = [vp, i64, vp, vp, vp, i64, vp, i64, i64, vp, vp, i64, vp]
    lib.ttemb_bag_reduce_mapped_backward_n.argtypes = [vp, vp, vp, i64, vp, vp, vp, vp, vp, i64, vp, i64, i64, vp, vp, vp, i64, vp]
    stp = ctypes.POINTER(StepDesc)
    lib.ttemb_backward_step.argtypes = [shp, vp, vp, vp, vp, i64, vp, i64, vp, stp, vp, i64, vp, i64, vp]
    lib.ttemb_backward_step_window.argtypes = [shp, vp, vp, vp, i64, i64, i64, i64, vp, stp, vp, i64, vp]
    lib.ttemb_backward_step_exact.argtypes = [shp, vp, vp, vp, i64, i64, vp, stp, vp, i64, vp, i64, vp]
    lib.ttemb_flat_step.argtypes = [vp, vp, vp, vp, vp, i64, f32, stp, vp, vp]
    for name in EXPORTED_SYMBOLS + BAGS_SYMBOLS + PADS_SYMBOLS + UNIQUE_SYMBOLS + UNIQUE_N_SYMBOLS:
        fn = getattr(lib, name)
        if name not in ("ttemb_last_error", "ttemb_workspace_bytes", "ttemb_plan_bytes", "ttemb_window_workspace_bytes",
                        "ttemb_exact_workspace_bytes", "ttemb_exact_plan_bytes", "ttemb_bag_workspace_bytes",
                        "ttemb_drop_padding_workspace_bytes", "ttemb_bag_max_workspace_bytes",
                        "ttemb_compact_bags_workspace_bytes", "ttemb_unique_ids_workspace_bytes",
                        "ttemb_unique_ids_n_workspace_bytes"):
            fn.restype = ctypes.c_int
    return lib


LIB = _load()
# per call family: the by-value symbols of SGD, Adagrad and Adam, then the descriptor symbol (_run_step)
_STEP_FN = {family: tuple(getattr(LIB, "ttemb_backward_" + kind + suffix) for kind in ("sgd", "adagrad", "adam", "step"))
            for family, suffix in (("plain", ""), ("window", "_window"), ("exact", "_exact"))}
_STEP_FN["flat"] = (LIB.ttemb_sgd_step, LIB.ttemb_adagrad_step, LIB.ttemb_adam_step, LIB.ttemb_flat_step)


def _check(rc: int) -> None:
    if rc != 0:
        raise RuntimeError(f"libttemb_hip: {LIB.ttemb_last_error().decode()} (status {rc})")


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("TT embedding kernels need tensors on a ROCm device; there is no CPU fallback")
    if not t.is_contiguous():
        raise RuntimeError("TT embedding kernels need contiguous tensors")
    return t.data_ptr() if t.numel() > 0 else None


def _ptr_array(ts):
    if isinstance(ts, ctypes.Array):   # already a pointer array (core_ptrs)
        return ts
    arr = (ctypes.c_void_p * MAX_CORES)()
    for i, t in enumerate(ts):
        if t.dtype != torch.float32:
            raise RuntimeError("TT cores must be float32")
        arr[i] = _ptr(t)
    return arr


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream(ref: torch.Tensor) -> int:
    """Raw hipStream_t of torch's current stream on the tensor's device."""
    if _raw_stream is not None:
        return _raw_stream(ref.device.index)
    return torch.cuda.current_stream(ref.device).cuda_stream


def _run_step(family: str, step: Step, head: tuple, ids: tuple, tail: tuple, scale: tuple = ()) -> int:
    """The one place a ``Step`` becomes a native call: picks the by-value symbol of its kind or the descriptor symbol (the
    rate is a device tensor) of ``family`` ("plain", "window", "exact": a lookup's backward; "flat": a flat epilogue) and
    orders the arguments.  ``head``: what precedes the optimiser's arrays (shape and cores; the weights), ``ids``: what lies
    between them and the rate, ``tail``: the rest.  A flat step's arrays are single tensors, ``scale = (grad_scale,)`` goes
    in front of Adam's hyper-parameters / the descriptor, and ``tail = (skip, stream)``.  Returns the status."""
    sgd, adagrad, adam, desc = _STEP_FN[family]
    flat = family == "flat"
    lr, st, hp = step.lr, step.state, step.hp
    if isinstance(lr, torch.Tensor):
        if flat:
            d = _fill_desc(lr, step.eps, _kind(st, hp), hp)
            return desc(*head, _ptr(st), _ptr(step.state2), _ptr(step.words), *ids, *scale, ctypes.byref(d), *tail)
        d, keep = step_desc(lr, step.eps, st, step.adam)
        return desc(*head, *ids, ctypes.byref(d), *tail)
    ptrs = _ptr if flat else _ptr_array
    if hp is not None:
        return adam(*head, ptrs(st), ptrs(step.state2), _ptr(step.words), *ids, *scale, ctypes.byref(hp), *tail)
    if flat and st is None and tail[0] is not None:
        return LIB.ttemb_sgd_step_guarded(*head, *ids, lr, *tail)
    if flat:   # (the by-value SGD / Adagrad epilogues take no skip word)
        assert tail[0] is None, "a by-value flat Adagrad step takes no skip word"
        tail = tail[1:]
    return sgd(*head, *ids, lr, *tail) if st is None else adagrad(*head, ptrs(st), *ids, lr, step.eps, *tail)


class _on_device:
    """`with torch.cuda.device(dev)` only when dev is not already current (the common case costs ~0)."""

    def __init__(self, dev: torch.device) -> None:
        self.ctx = None if dev.index == torch.cuda.current_device() else torch.cuda.device(dev)

    def __enter__(self):
        if self.ctx is not None:
            self.ctx.__enter__()

    def __exit__(self, *exc):
        if self.ctx is not None:
            self.ctx.__exit__(*exc)


class Workspace:
    """Grow-only scratch buffer owned by the caller (the library never allocates).

    A buffer that was handed out while a HIP graph was being captured is baked into that graph: when a later, larger call
    makes the workspace grow, such a buffer is retired (kept alive for the life of this object) instead of freed, so a
    replay never writes into memory the allocator has given to someone else."""

    def __init__(self) -> None:
        self.buf: Optional[torch.Tensor] = None
        self._in_a_graph = False
        self._retired: List[torch.Tensor] = []

    def get(self, nbytes: int, device: torch.device) -> torch.Tensor:
        if not _initialised:
            init()
        nbytes = max(int(nbytes), 256)
        if self.buf is None or self.buf.numel() < nbytes or self.buf.device != device:
            if self.buf is not None and self._in_a_graph:
                self._retired.append(self.buf)
                self._in_a_graph = False
            self.buf = torch.empty(nbytes + nbytes // 4, dtype=torch.uint8, device=device)
        if not self._in_a_graph and torch.cuda.is_current_stream_capturing():
            self._in_a_graph = True
        return self.buf


_initialised = False


def init() -> None:
    """``ttemb_init()``: the pinned host word an expired device-side wait reports to -- the library's one allocation, made
    here and never inside a lookup.  Called by the first ``Workspace.get`` of the process that is not under a stream capture
    (every lookup through this module asks its workspace first) and by ``TTEmbeddingBag.capture`` before it captures; a
    failure is not an error of the caller's (such a process reports expired waits through NaN results only)."""
    global _initialised
    if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        return   # not now: no allocation during a capture; the next eager call tries again
    _initialised = True
    LIB.ttemb_init()


_size_cache: dict = {}   # (kind, shape bytes, op, nnz, B) -> bytes; emptied when the kernel family changes


path_epoch = 0   # bumped when the kernel family changes: callers that keep their own size caches compare it


def set_path(path: int) -> None:
    global path_epoch
    _check(LIB.ttemb_set_path(path))
    _size_cache.clear()
    path_epoch += 1


def profile_enable(on: bool) -> None:
    _check(LIB.ttemb_profile_enable(1 if on else 0))


def profile_read(which: int) -> float:
    """Milliseconds of the most recent forward (0) / backward (1) chain kernel."""
    ms = ctypes.c_float(0.0)
    _check(LIB.ttemb_profile_read(which, ctypes.byref(ms)))
    return float(ms.value)


def _shape_key(shape: Optional[Shape]):
    if shape is None:
        return None
    k = getattr(shape, "_key", None)
    if k is None:
        k = shape._key = bytes(shape)
    return k


def workspace_bytes(shape: Optional[Shape], op: int, nnz: int, B: int) -> int:
    key = ("w", _shape_key(shape), op, nnz, B)
    n = _size_cache.get(key)
    if n is None:
        n = LIB.ttemb_workspace_bytes(ctypes.byref(shape) if shape is not None else None, op, nnz, B)
        if n < 0:
            _check(int(n))
        n = _size_cache[key] = int(n)
        if len(_size_cache) > 4096:
            _size_cache.clear()
    return n


def plan_bytes(shape: Shape, nnz: int) -> int:
    key = ("p", _shape_key(shape), nnz)
    n = _size_cache.get(key)
    if n is None:
        n = LIB.ttemb_plan_bytes(ctypes.byref(shape), nnz)
        if n < 0:
            _check(int(n))
        n = _size_cache[key] = int(n)
    return n


FAMILY_SCALAR, FAMILY_PER_BAG, FAMILY_PER_BAG_RT, FAMILY_GROUPED, FAMILY_GROUPED_WIDE, FAMILY_MERGED, FAMILY_PADDED = 0, 1, 2, 3, 4, 16, 32
FAMILY_PREFIX_IN_CHAIN = 64   # | on FAMILY_GROUPED: a whole forward of this size forms the prefix products in its chain kernel
FAMILY_GROUP_PRODUCTS_IN_CHAIN = 128   # | on FAMILY_GROUPED: a backward of this size forms the per-group products in its chunk kernel
FAMILY_ROUTE_FLAGS = FAMILY_PREFIX_IN_CHAIN | FAMILY_GROUP_PRODUCTS_IN_CHAIN   # which kernels of the grouped family a call of this size takes


def kernel_family(shape: Shape, nnz: int, B: int, ids_with_offsets: bool = True) -> int:
    """Which kernels a lookup of this size would run (``FAMILY_*``, ``| FAMILY_MERGED`` for a 2- / 4-core table on a
    3-core view) under the current ``set_path``; launches nothing."""
    rc = LIB.ttemb_kernel_family(ctypes.byref(shape), nnz, B, 1 if ids_with_offsets else 0)
    if rc < 0:
        _check(rc)
    return rc


def is_grouped(shape: Shape, nnz: int, B: int, ids_with_offsets: bool = True) -> bool:
    """Whether a lookup of this size runs on the grouped kernels (the family with bounded device-side waits, whose last
    backward kernel leaves its verdict in the workspace header).  The one memo of that answer; launches nothing."""
    key = ("g", _shape_key(shape), nnz, B, ids_with_offsets, path_epoch)
    g = _size_cache.get(key)
    if g is None:
        if len(_size_cache) > 4096:
            _size_cache.clear()
        g = _size_cache[key] = nnz > 0 and (kernel_family(shape, nnz, B, ids_with_offsets) & 7) in (FAMILY_GROUPED,
                                                                                                   FAMILY_GROUPED_WIDE)
    return g


def set_spin_limit(tries: int = 0) -> None:
    """Diagnostic: tries of the grouping pass's bounded device-side waits (0 = default, negative = none: every wait expires)."""
    _check(LIB.ttemb_set_spin_limit(tries))


def status() -> None:
    """Raise ``RuntimeError`` when a device-side wait of an earlier grouped lookup ran out (its results are NaN); consumes
    the fault.  The caller synchronises first when it wants the answer for everything it has enqueued."""
    _check(LIB.ttemb_status())


def grouping_layout(shape: Shape, nnz: int) -> dict:
    """DIAGNOSTIC: the grouped path's grouping layout for `nnz` ids (ttemb_grouping_layout)."""
    out = (ctypes.c_int64 * 5)()
    _check(LIB.ttemb_grouping_layout(ctypes.byref(shape), nnz, out))
    return dict(zip(("slices", "ranges", "banks", "cap", "ovf_slots"), (int(x) for x in out)))


def set_piece_limits(rows: int = 0, ids: int = 0) -> None:
    """Diagnostic: cut calls into pieces of at most ``rows`` bags / ``ids`` ids (0 = the hardware's limits)."""
    global path_epoch
    _check(LIB.ttemb_set_piece_limits(rows, ids))
    _size_cache.clear()
    path_epoch += 1


def set_wide_slab_min_ids(ids: int = 0) -> None:
    """Diagnostic: from how many ids on the wide-rank backward reduces dG2 in LDS (0 = the rule, 1 = always)."""
    global path_epoch
    _check(LIB.ttemb_set_wide_slab_min_ids(ids))
    _size_cache.clear()
    path_epoch += 1


def new_plan(shape: Shape, nnz: int, device: torch.device) -> Optional[torch.Tensor]:
    """Buffer in which forward leaves its id grouping for the matching backward (None if unused)."""
    n = plan_bytes(shape, nnz)
    return torch.empty(n, dtype=torch.uint8, device=device) if n > 0 else None


def _plan_args(plan: Optional[torch.Tensor]):
    return (None, 0) if plan is None else (plan.data_ptr(), plan.numel())


def forward(shape: Shape, cores: Sequence[torch.Tensor], indices: torch.Tensor, rowidx: torch.Tensor,
            offsets: Optional[torch.Tensor], nnz: int, nnz_dev: Optional[torch.Tensor], B: int,
            output: torch.Tensor, ws: Workspace, plan: Optional[torch.Tensor] = None, phase: int = 0) -> None:
    """phase 0 = the whole forward; 1 = the id-only half (grouping into `plan`); 2 = the lookup on that plan."""
    dev = output.device
    w = ws.get(workspace_bytes(shape, OP_FORWARD, nnz, B), dev)
    fn = (LIB.ttemb_forward, LIB.ttemb_forward_group, LIB.ttemb_forward_lookup)[phase]
    with _on_device(dev):
        _check(fn(ctypes.byref(shape), _ptr_array(cores), _ptr(indices), _ptr(rowidx),
                  _ptr(offsets), nnz, _ptr(nnz_dev), B, _ptr(output), _ptr(w), w.numel(),
                  *_plan_args(plan), _stream(output)))


def backward_dense(shape: Shape, cores: Sequence[torch.Tensor], indices, rowidx, nnz: int, nnz_dev, B: int,
                   d_output: torch.Tensor, d_cores: Sequence[torch.Tensor], ws: Workspace,
                   plan: Optional[torch.Tensor] = None, offsets: Optional[torch.Tensor] = None) -> None:
    dev = d_output.device
    w = ws.get(workspace_bytes(shape, OP_BACKWARD, nnz, B), dev)
    with _on_device(dev):
        _check(LIB.ttemb_backward_dense(ctypes.byref(shape), _ptr_array(cores), _ptr(indices), _ptr(rowidx),
                                        _ptr(offsets), nnz, _ptr(nnz_dev), B, _ptr(d_output), _ptr_array(d_cores), _ptr(w),
                                        w.numel(), *_plan_args(plan), _stream(d_output)))


def backward_fused(shape: Shape, cores, indices, rowidx, nnz: int, nnz_dev, B: int, d_output, step: Step, ws: Workspace,
                   plan: Optional[torch.Tensor] = None, offsets: Optional[torch.Tensor] = None) -> None:
    """The backward with the optimiser step ``step`` fused into it (``ttemb_backward_sgd`` / ``_adagrad`` / ``_adam``, or
    ``ttemb_backward_step`` when the rate is a device tensor)."""
    dev = d_output.device
    w = ws.get(workspace_bytes(shape, OP_BACKWARD, nnz, B), dev)
    with _on_device(dev):
        _check(_run_step("plain", step, (ctypes.byref(shape), _ptr_array(cores)),
                         (_ptr(indices), _ptr(rowidx), _ptr(offsets), nnz, _ptr(nnz_dev), B, _ptr(d_output)),
                         (_ptr(w), w.numel(), *_plan_args(plan), _stream(d_output))))


def backward_step(shape: Shape, cores, indices, rowidx, nnz: int, nnz_dev, B: int, d_output, lr: torch.Tensor, ws: Workspace,
                  plan: Optional[torch.Tensor] = None, offsets: Optional[torch.Tensor] = None, eps: float = 0.0, state=None,
                  adam=None) -> None:
    """The fused step with the rate in the device word ``lr`` (``ttemb_backward_step``): SGD, Adagrad (``state``) or Adam
    (``state`` the first moment, ``adam = (exp_avg_sq, step words, AdamParams)``)."""
    _lr_word(lr)
    backward_fused(shape, cores, indices, rowidx, nnz, nnz_dev, B, d_output, Step(lr, eps, state, adam), ws, plan, offsets)


def backward_sgd(shape: Shape, cores, indices, rowidx, nnz: int, nnz_dev, B: int, d_output, lr,
                 ws: Workspace, plan: Optional[torch.Tensor] = None, offsets: Optional[torch.Tensor] = None) -> None:
    """``lr``: a float, or a float32[1] device tensor (the rate is then read on the device: ``backward_step``)."""
    backward_fused(shape, cores, indices, rowidx, nnz, nnz_dev, B, d_output, Step(lr), ws, plan, offsets)


def backward_adagrad(shape: Shape, cores, opt_state, indices, rowidx, nnz: int, nnz_dev, B: int, d_output,
                     lr, eps: float, ws: Workspace, plan: Optional[torch.Tensor] = None,
                     offsets: Optional[torch.Tensor] = None) -> None:
    backward_fused(shape, cores, indices, rowidx, nnz, nnz_dev, B, d_output, Step(lr, eps, opt_state), ws, plan, offsets)


def backward_adam(shape: Shape, cores, exp_avg, exp_avg_sq, step: torch.Tensor, indices, rowidx, nnz: int, nnz_dev, B: int,
                  d_output, hp: AdamParams, ws: Workspace, plan: Optional[torch.Tensor] = None,
                  offsets: Optional[torch.Tensor] = None, lr: Optional[torch.Tensor] = None) -> None:
    """Fused Adam / AdamW step (``ttemb_backward_adam``): ``exp_avg`` / ``exp_avg_sq`` shaped like the cores, ``step`` the
    int32[4] device words of ``new_adam_step``.  ``lr`` (a float32[1] device tensor): the rate is read on the device and
    the one in ``hp`` ignored (``backward_step``)."""
    backward_fused(shape, cores, indices, rowidx, nnz, nnz_dev, B, d_output, Step(lr, 0.0, exp_avg, (exp_avg_sq, step, hp)), ws,
                   plan, offsets)


def _flat(weights, grads, step: Step, grad_scale: float = 1.0, skip: Optional[torch.Tensor] = None) -> None:
    with _on_device(weights.device):
        _check(_run_step("flat", step, (_ptr(weights),), (_ptr(grads), weights.numel()), (_ptr(skip), _stream(weights)),
                         (grad_scale,)))


def flat_step(weights, grads, lr: torch.Tensor, state=None, eps: float = 0.0, adam=None, grad_scale: float = 1.0,
              skip: Optional[torch.Tensor] = None) -> None:
    """A flat epilogue with the rate in the device word ``lr`` (``ttemb_flat_step``): SGD, Adagrad (``state``) or Adam
    (``state`` = exp_avg, ``adam = (exp_avg_sq, step words, AdamParams)``)."""
    _lr_word(lr)
    _flat(weights, grads, Step(lr, eps, state, adam), grad_scale, skip)


def adam_step(weights, exp_avg, exp_avg_sq, step: torch.Tensor, grads, hp: AdamParams, grad_scale: float = 1.0,
              skip: Optional[torch.Tensor] = None, lr: Optional[torch.Tensor] = None) -> None:
    """Flat Adam / AdamW epilogue (``ttemb_adam_step``): ``g = grads * grad_scale``; a non-zero device word ``skip[0]``
    leaves weights, moments and the step count as they are.  ``lr`` (a float32[1] device tensor): the rate is read on the
    device and the one in ``hp`` ignored."""
    _flat(weights, grads, Step(lr, 0.0, exp_avg, (exp_avg_sq, step, hp)), grad_scale, skip)


def sgd_step(weights: torch.Tensor, grads: torch.Tensor, lr) -> None:
    """``lr``: a float, or a float32[1] device tensor (read on the device: ``flat_step``) -- so for every flat step."""
    _flat(weights, grads, Step(lr))


HEADER_POISON_OFFSET = 32784   # TTEMB_HEADER_POISON_OFFSET


def sgd_step_guarded(weights: torch.Tensor, grads: torch.Tensor, lr, skip: torch.Tensor) -> None:
    """``weights -= lr * grads`` unless the device float ``skip[0]`` is non-zero (then nothing is written)."""
    _flat(weights, grads, Step(lr), skip=skip)


def poison_word(ws: "Workspace") -> Optional[torch.Tensor]:
    """int32[1] view of the word the last GROUPED backward on this workspace left in its header (1 = poisoned plan and the
    host hears of it); None before the workspace exists.  Meaningful only right after a grouped backward."""
    if ws.buf is None or ws.buf.numel() < HEADER_POISON_OFFSET + 4:
        return None
    return ws.buf[HEADER_POISON_OFFSET:HEADER_POISON_OFFSET + 4].view(torch.int32)


def adagrad_step(weights, state, grads, lr, eps: float) -> None:
    _flat(weights, grads, Step(lr, eps, state))


E_UNSUPPORTED = -3


def window_workspace_bytes(shape: Shape, op: int, nnz: int, bags_total: int, B: int) -> int:
    """Bytes a window call needs, or -1 when the grouped kernels do not serve such a window (the caller then splits the id
    list on the host: one plain call per table)."""
    key = ("win", _shape_key(shape), op, nnz, bags_total, B, path_epoch)
    n = _size_cache.get(key)
    if n is None:
        n = int(LIB.ttemb_window_workspace_bytes(ctypes.byref(shape), op, nnz, bags_total, B))
        if n < 0 and n != E_UNSUPPORTED:
            _check(n)
        n = _size_cache[key] = (-1 if n < 0 else n)
    return n


def forward_window(shape: Shape, cores: Sequence[torch.Tensor], indices: torch.Tensor, offsets: torch.Tensor, bag0: int, B: int,
                   output: torch.Tensor, ws: Workspace) -> None:
    """One table of a table-batched call: the bags [bag0, bag0 + B) of ``offsets`` (the whole call's) and their ids;
    ``output`` is the [bags_total, D] tensor of the whole call.  No host synchronisation."""
    nnz, bags = indices.numel(), offsets.numel() - 1
    dev = output.device
    w = ws.get(window_workspace_bytes(shape, OP_FORWARD, nnz, bags, B), dev)
    with _on_device(dev):
        _check(LIB.ttemb_forward_window(ctypes.byref(shape), _ptr_array(cores), _ptr(indices), _ptr(offsets), nnz, bags, bag0, B,
                                        _ptr(output), _ptr(w), w.numel(), _stream(output)))


def backward_window(shape: Shape, cores: Sequence[torch.Tensor], indices: torch.Tensor, offsets: torch.Tensor, bag0: int, B: int,
                    d_output: torch.Tensor, ws: Workspace, d_cores: Optional[Sequence[torch.Tensor]] = None,
                    opt_state: Optional[Sequence[torch.Tensor]] = None, lr=0.0, eps: float = 0.0, adam=None) -> None:
    """``d_cores``: dense gradients of the window's table; else the fused step (Adagrad when ``opt_state`` is given; Adam
    with ``adam = (exp_avg_sq, step, AdamParams)``, ``opt_state`` then the first moment).  ``lr``: a float, or a float32[1]
    device tensor (``ttemb_backward_step_window``: the rate is read on the device, the one of an ``AdamParams`` ignored)."""
    nnz, bags = indices.numel(), offsets.numel() - 1
    dev = d_output.device
    w = ws.get(window_workspace_bytes(shape, OP_BACKWARD, nnz, bags, B), dev)
    head = (ctypes.byref(shape), _ptr_array(cores))
    ids = (_ptr(indices), _ptr(offsets), nnz, bags, bag0, B, _ptr(d_output))
    tail = (_ptr(w), w.numel(), _stream(d_output))
    with _on_device(dev):
        if d_cores is not None:
            _check(LIB.ttemb_backward_dense_window(*head, *ids, _ptr_array(d_cores), *tail))
        else:
            _check(_run_step("window", Step(lr, eps, opt_state, adam), head, ids, tail))


def exact_workspace_bytes(shape: Shape, nnz: int, B: int) -> int:
    """Bytes the exact calls need (one workspace serves the forward and every backward), or -1 when the exact kernels do
    not cover the shape (``exact_unsupported_reason`` says why)."""
    key = ("exact", _shape_key(shape), nnz, B)
    n = _size_cache.get(key)
    if n is None:
        n = int(LIB.ttemb_exact_workspace_bytes(ctypes.byref(shape), nnz, B))
        if n < 0 and n != E_UNSUPPORTED:
            _check(n)
        n = _size_cache[key] = (-1 if n < 0 else n)
    return n


def exact_unsupported_reason(shape: Shape) -> Optional[str]:
    """None when the exact kernels cover the shape, else the library's reason."""
    n = int(LIB.ttemb_exact_workspace_bytes(ctypes.byref(shape), 0, 0))
    if n >= 0:
        return None
    if n != E_UNSUPPORTED:
        _check(n)
    return LIB.ttemb_last_error().decode()


def set_exact_grid(workgroups: int = 0) -> None:
    """Diagnostic: cap the grid of the exact kernels (0 = default).  Never changes a result."""
    _check(LIB.ttemb_set_exact_grid(workgroups))


def forward_exact(shape: Shape, cores, indices: torch.Tensor, offsets: torch.Tensor, B: int, output: torch.Tensor,
                  ws: Workspace) -> None:
    """Bit-reproducible forward (``ttemb_forward_exact``): ``output`` [B, D] fully written."""
    nnz = indices.numel()
    dev = output.device
    w = ws.get(exact_workspace_bytes(shape, nnz, B), dev)
    with _on_device(dev):
        _check(LIB.ttemb_forward_exact(ctypes.byref(shape), _ptr_array(cores), _ptr(indices), _ptr(offsets), nnz, B,
                                       _ptr(output), _ptr(w), w.numel(), None, 0, _stream(output)))


def backward_exact(shape: Shape, cores, indices: torch.Tensor, offsets: torch.Tensor, B: int, d_output: torch.Tensor,
                   ws: Workspace, d_cores=None, opt_state=None, lr=0.0, eps: float = 0.0, adam=None) -> None:
    """Bit-reproducible backward: dense gradients into ``d_cores`` (every row written), else the fused step on the rows
    the ids touch (Adagrad when ``opt_state`` is given), or dense Adam on every row with ``adam = (exp_avg_sq, step,
    AdamParams)`` and ``opt_state`` the first moment.  ``lr``: a float, or a float32[1] device tensor
    (``ttemb_backward_step_exact``: the rate is read on the device, the one of an ``AdamParams`` ignored)."""
    nnz = indices.numel()
    dev = d_output.device
    need = exact_workspace_bytes(shape, nnz, B)
    if adam is not None:   # + the gradient scratch behind it (include/ttemb.h, ttemb_backward_adam_exact)
        need = -(-need // 256) * 256 + sum(-(-(shape.p[t] * shape.R[t] * shape.q[t] * shape.R[t + 1] * 4) // 256) * 256
                                           for t in range(shape.T))
    w = ws.get(need, dev)
    head = (ctypes.byref(shape), _ptr_array(cores))
    ids = (_ptr(indices), _ptr(offsets), nnz, B, _ptr(d_output))
    tail = (_ptr(w), w.numel(), None, 0, _stream(d_output))
    with _on_device(dev):
        if d_cores is not None:
            _check(LIB.ttemb_backward_dense_exact(*head, *ids, _ptr_array(d_cores), *tail))
        else:
            _check(_run_step("exact", Step(lr, eps, opt_state, adam), head, ids, tail))


def bag_workspace_bytes(nnz: int, B: int, D: int) -> int:
    """Bytes ``bag_reduce`` needs (behind the lookups' 40 KB header: the lookups' workspace serves it too)."""
    key = ("bag", nnz, B, D)
    n = _size_cache.get(key)
    if n is None:
        n = int(LIB.ttemb_bag_workspace_bytes(nnz, B, D))
        if n < 0:
            _check(n)
        n = _size_cache[key] = n
    return n


def _check_weights(weights: torch.Tensor, nnz: int, ref: torch.Tensor) -> None:
    if weights.dtype != torch.float32 or weights.dim() != 1 or weights.numel() != nnz or weights.device != ref.device:
        raise ValueError(f"per_sample_weights must be float32 of shape [{nnz}] on {ref.device}, got "
                         f"{weights.dtype} {list(weights.shape)} on {weights.device}")


def _check_sizes(tensors, n: int) -> None:
    for t in tensors:
        if t is not None and (t.dtype != torch.float32 or t.numel() != n):
            raise ValueError(f"bag pooling: expected float32 with {n} elements, got {t.dtype} {list(t.shape)}")


def _count_word(nnz_dev: Optional[torch.Tensor]) -> Optional[int]:
    """The device id count of a ``*_n`` pooling call (``counted=True``): an int32 word on the device, or None (NULL: all ids)."""
    if nnz_dev is not None and (nnz_dev.dtype != torch.int32 or nnz_dev.numel() < 1):
        raise ValueError("bag pooling: the id count is an int32 word on the device")
    return _ptr(nnz_dev)


def bag_reduce(rows: torch.Tensor, weights: torch.Tensor, offsets: torch.Tensor, output: torch.Tensor, ws: Workspace,
               nnz_dev: Optional[torch.Tensor] = None, counted: bool = False) -> None:
    """``output[b] = sum_{i in bag b} weights[i] rows[i]`` (``ttemb_bag_reduce``): rows [nnz, D], output [B, D] fully written.
    ``counted`` (here and in the pooling calls below): the ``*_n`` entry point, whose kernels stop at the id count in the
    device word ``nnz_dev`` (None: at nnz)."""
    nnz, D = rows.shape
    B = offsets.numel() - 1
    _check_weights(weights, nnz, rows)
    _check_sizes((output,), B * D)
    dev = output.device
    w = ws.get(bag_workspace_bytes(nnz, B, D), dev)
    with _on_device(dev):
        if counted:
            _check(LIB.ttemb_bag_reduce_n(_ptr(rows), _ptr(weights), _ptr(offsets), nnz, _count_word(nnz_dev), B, D, _ptr(output),
                                          _ptr(w), w.numel(), _stream(output)))
        else:
            _check(LIB.ttemb_bag_reduce(_ptr(rows), _ptr(weights), _ptr(offsets), nnz, B, D, _ptr(output), _ptr(w), w.numel(),
                                        _stream(output)))


def bag_reduce_backward(d_output: torch.Tensor, weights: torch.Tensor, offsets: torch.Tensor, d_rows: torch.Tensor,
                        ws: Workspace, rows: Optional[torch.Tensor] = None, d_weights: Optional[torch.Tensor] = None,
                        nnz_dev: Optional[torch.Tensor] = None, counted: bool = False) -> None:
    """``d_rows[i] = weights[i] d_output[bag(i)]``, and ``d_weights[i] = <d_output[bag(i)], rows[i]>`` when ``d_weights``
    is given (then ``rows`` is needed); one pass (``ttemb_bag_reduce_backward``)."""
    nnz, D = d_rows.shape
    B = offsets.numel() - 1
    _check_weights(weights, nnz, d_rows)
    _check_sizes((d_output,), B * D)
    _check_sizes((rows,), nnz * D)
    if d_weights is not None:
        _check_sizes((d_weights,), nnz)
    dev = d_rows.device
    w = ws.get(0, dev)
    with _on_device(dev):
        if counted:
            _check(LIB.ttemb_bag_reduce_backward_n(_ptr(d_output), _ptr(weights), _ptr(rows), _ptr(offsets), nnz,
                                                   _count_word(nnz_dev), B, D, _ptr(d_rows), _ptr(d_weights), _ptr(w), w.numel(),
                                                   _stream(d_rows)))
        else:
            _check(LIB.ttemb_bag_reduce_backward(_ptr(d_output), _ptr(weights), _ptr(rows), _ptr(offsets), nnz, B, D, _ptr(d_rows),
                                                 _ptr(d_weights), _ptr(w), w.numel(), _stream(d_rows)))


def bag_mean(src: torch.Tensor, dst: torch.Tensor, offsets: torch.Tensor) -> None:
    """``dst[b] = src[b] / len(b)``, zeros for an empty bag (``ttemb_bag_mean``); ``dst`` may be ``src``."""
    D, B = src.shape[-1], offsets.numel() - 1
    _check_sizes((src, dst), B * D)
    with _on_device(dst.device):
        _check(LIB.ttemb_bag_mean(_ptr(src), _ptr(dst), _ptr(offsets), B, D, _stream(dst)))


def bag_max_workspace_bytes(nnz: int, B: int, D: int) -> int:
    """Bytes ``bag_max`` needs (behind the lookups' 40 KB header, as ``bag_workspace_bytes``)."""
    key = ("bagmax", nnz, B, D)
    n = _size_cache.get(key)
    if n is None:
        n = int(LIB.ttemb_bag_max_workspace_bytes(nnz, B, D))
        if n < 0:
            _check(n)
        n = _size_cache[key] = n
    return n


def bag_max(rows: torch.Tensor, offsets: torch.Tensor, output: torch.Tensor, argmax: torch.Tensor, ws: Workspace,
            indices: Optional[torch.Tensor] = None, pad: int = 0, nnz_dev: Optional[torch.Tensor] = None,
            counted: bool = False) -> None:
    """``output[b][d] = max_{i in bag b} rows[i][d]``, ``argmax[b][d]`` (int32) the first position that holds it, -1 and zeros
    without one (``ttemb_bag_max``).  With ``indices``, positions whose id equals ``pad`` are skipped."""
    nnz, D = rows.shape
    B = offsets.numel() - 1
    _check_sizes((rows,), nnz * D)
    _check_sizes((output,), B * D)
    if argmax.dtype != torch.int32 or argmax.numel() != B * D:
        raise ValueError(f"bag_max: output / argmax must hold [{B}, {D}] float32 / int32")
    if indices is not None and (indices.dtype != torch.int64 or indices.numel() != nnz):
        raise ValueError(f"bag_max: indices must be int64 [{nnz}]")
    dev = output.device
    w = ws.get(bag_max_workspace_bytes(nnz, B, D), dev)
    with _on_device(dev):
        if counted:
            _check(LIB.ttemb_bag_max_n(_ptr(rows), _ptr(indices), int(pad), _ptr(offsets), nnz, _count_word(nnz_dev), B, D,
                                       _ptr(output), _ptr(argmax), _ptr(w), w.numel(), _stream(output)))
        else:
            _check(LIB.ttemb_bag_max(_ptr(rows), _ptr(indices), int(pad), _ptr(offsets), nnz, B, D, _ptr(output), _ptr(argmax),
                                     _ptr(w), w.numel(), _stream(output)))


def bag_max_backward(d_output: torch.Tensor, argmax: torch.Tensor, offsets: torch.Tensor, d_rows: torch.Tensor,
                     nnz_dev: Optional[torch.Tensor] = None, counted: bool = False) -> None:
    """``d_rows[i][d] = d_output[bag(i)][d]`` where ``argmax[bag(i)][d] == i``, else 0; every element written
    (``ttemb_bag_max_backward``)."""
    nnz, D = d_rows.shape
    B = offsets.numel() - 1
    _check_sizes((d_output,), B * D)
    _check_sizes((d_rows,), nnz * D)
    if argmax.dtype != torch.int32 or argmax.numel() != B * D:
        raise ValueError(f"bag_max_backward: argmax must hold [{B}, {D}] int32")
    with _on_device(d_rows.device):
        if counted:
            _check(LIB.ttemb_bag_max_backward_n(_ptr(d_output), _ptr(argmax), _ptr(offsets), nnz, _count_word(nnz_dev), B, D,
                                                _ptr(d_rows), _stream(d_rows)))
        else:
            _check(LIB.ttemb_bag_max_backward(_ptr(d_output), _ptr(argmax), _ptr(offsets), nnz, B, D, _ptr(d_rows),
                                              _stream(d_rows)))


def drop_padding_workspace_bytes(nnz: int, B: int) -> int:
    key = ("pad", nnz, B)
    n = _size_cache.get(key)
    if n is None:
        n = int(LIB.ttemb_drop_padding_workspace_bytes(nnz, B))
        if n < 0:
            _check(n)
        n = _size_cache[key] = n
    return n


def drop_padding(indices: torch.Tensor, offsets: torch.Tensor, pad: int, indices_out: torch.Tensor, rowidx_out: torch.Tensor,
                 offsets_out: torch.Tensor, nnz_kept_dev: torch.Tensor, ws: Workspace) -> None:
    """Stable partition of the ids into those != ``pad`` inside a bag (first, input order) and the rest; ``offsets_out`` the
    compacted bags, ``nnz_kept_dev`` (int32[1]) their id count, on the device (``ttemb_drop_padding``)."""
    nnz, B = indices.numel(), offsets.numel() - 1
    if offsets_out.numel() != B + 1 or nnz_kept_dev.dtype != torch.int32 or nnz_kept_dev.numel() < 1:
        raise ValueError("drop_padding: offsets_out must have B + 1 entries and nnz_kept_dev one int32")
    dev = offsets.device
    w = ws.get(drop_padding_workspace_bytes(nnz, B), dev)
    with _on_device(dev):
        _check(LIB.ttemb_drop_padding(_ptr(indices), _ptr(offsets), nnz, B, int(pad), _ptr(indices_out), _ptr(rowidx_out),
                                      _ptr(offsets_out), _ptr(nnz_kept_dev), _ptr(w), w.numel(), _stream(offsets)))


def pad_weights(indices: torch.Tensor, offsets: torch.Tensor, weights: Optional[torch.Tensor], pad: int, mean: bool,
                weights_out: torch.Tensor, nnz_dev: Optional[torch.Tensor] = None, counted: bool = False) -> None:
    """``weights_out[i] = (indices[i] != pad) * (weights[i] or 1) * (1 / kept ids of its bag if mean)`` (``ttemb_pad_weights``)."""
    nnz = indices.numel()
    _check_sizes((weights, weights_out), nnz)
    with _on_device(weights_out.device):
        if counted:
            _check(LIB.ttemb_pad_weights_n(_ptr(indices), _ptr(offsets), _ptr(weights), nnz, _count_word(nnz_dev),
                                           offsets.numel() - 1, int(pad), 1 if mean else 0, _ptr(weights_out), _stream(weights_out)))
        else:
            _check(LIB.ttemb_pad_weights(_ptr(indices), _ptr(offsets), _ptr(weights), nnz, offsets.numel() - 1, int(pad),
                                         1 if mean else 0, _ptr(weights_out), _stream(weights_out)))


def compact_bags_workspace_bytes(nnz: int) -> int:
    key = ("compact", nnz)
    n = _size_cache.get(key)
    if n is None:
        n = int(LIB.ttemb_compact_bags_workspace_bytes(nnz))
        if n < 0:
            _check(n)
        n = _size_cache[key] = n
    return n


def compact_bags(indices: torch.Tensor, offsets: torch.Tensor, weights: Optional[torch.Tensor], pad: int,
                 indices_out: torch.Tensor, offsets_out: torch.Tensor, weights_out: Optional[torch.Tensor],
                 map_out: Optional[torch.Tensor], kept_dev: torch.Tensor, ws, nnz_dev: Optional[torch.Tensor] = None) -> None:
    """``drop_padding`` behind a device id count (``ttemb_compact_bags``): of the first ``c`` positions (``nnz_dev``; None: all)
    the ids != ``pad`` inside a bag go to ``indices_out[:kept]`` in input order, their ``weights`` (or None) to
    ``weights_out[:kept]``, the compacted bags to ``offsets_out``, ``kept`` to the int32 word ``kept_dev`` and, with
    ``map_out`` (int32 ``[nnz]``), every position's compacted place or -1 to ``map_out[:c]``.  Nothing past ``kept`` / ``c`` is
    written.  ``ws``: a ``Workspace``, or a uint8 tensor of ``compact_bags_workspace_bytes(nnz)``."""
    nnz, B = indices.numel(), offsets.numel() - 1
    if (indices.dtype != torch.int64 or offsets.dtype != torch.int64 or indices_out.dtype != torch.int64
            or offsets_out.dtype != torch.int64 or indices_out.numel() < nnz or offsets_out.numel() != B + 1):
        raise ValueError("compact_bags: ids and offsets are int64, indices_out holds nnz and offsets_out B + 1 entries")
    if kept_dev.dtype != torch.int32 or kept_dev.numel() < 1:
        raise ValueError("compact_bags: kept_dev is an int32 word on the device")
    if (weights is None) != (weights_out is None):
        raise ValueError("compact_bags: weights and weights_out come together")
    _check_sizes((weights, weights_out), nnz)
    if map_out is not None and (map_out.dtype != torch.int32 or map_out.numel() != nnz):
        raise ValueError(f"compact_bags: map_out must be int32 [{nnz}]")
    dev = offsets.device
    w = ws.get(compact_bags_workspace_bytes(nnz), dev) if isinstance(ws, Workspace) else ws
    with _on_device(dev):
        _check(LIB.ttemb_compact_bags(_ptr(indices), _ptr(offsets), _ptr(weights), nnz, _count_word(nnz_dev), B, int(pad),
                                      _ptr(indices_out), _ptr(offsets_out), _ptr(weights_out), _ptr(map_out), _ptr(kept_dev),
                                      _ptr(w), w.numel(), _stream(offsets)))


def expand_kept(src: torch.Tensor, map_: torch.Tensor, out: torch.Tensor, nnz_dev: Optional[torch.Tensor] = None) -> None:
    """``out[n] = src[map_[n]]``, 0 where ``map_[n] < 0``, for the first ``c`` positions (``nnz_dev``; None: all); the rest of
    ``out`` is not touched (``ttemb_expand_kept``: the weight gradient of compacted bags back at the call's positions)."""
    nnz = map_.numel()
    _check_sizes((src, out), nnz)
    if map_.dtype != torch.int32:
        raise ValueError(f"expand_kept: the map must be int32 [{nnz}]")
    with _on_device(out.device):
        _check(LIB.ttemb_expand_kept(_ptr(src), _ptr(map_), nnz, _count_word(nnz_dev), _ptr(out), _stream(out)))


def unique_ids_workspace_bytes(nnz: int, rows: int) -> int:
    """Bytes ``unique_ids`` needs (behind the lookups' 40 KB header: the lookups' workspace serves it too)."""
    key = ("unique", nnz, rows)
    n = _size_cache.get(key)
    if n is None:
        n = int(LIB.ttemb_unique_ids_workspace_bytes(nnz, rows))
        if n < 0:
            _check(n)
        n = _size_cache[key] = n
    return n


def unique_ids(indices: torch.Tensor, rows: int, unique_out: torch.Tensor, inverse_out: torch.Tensor, perm_out: torch.Tensor,
               seg_out: torch.Tensor, count_dev: torch.Tensor, ws) -> None:
    """The distinct ids of ``indices`` (int64 ``[nnz]``, values in ``[0, rows)``) on the device (``ttemb_unique_ids``): with U
    their number, ``unique_out[:U]`` (int64) the ids in ascending order, ``inverse_out`` (int32 ``[nnz]``) every position's
    place in it, ``perm_out`` (int32 ``[nnz]``) the positions sorted by id (stable), ``seg_out[:U + 1]`` (int64 ``[nnz + 1]``)
    where each id's positions begin in ``perm_out``, U in the int32 word ``count_dev``.  Nothing past U / U + 1 is written.  No
    host synchronisation.  ``ws``: a ``Workspace``, or a uint8 tensor of ``unique_ids_workspace_bytes(nnz, rows)``."""
    nnz = indices.numel()
    if (indices.dtype != torch.int64 or unique_out.dtype != torch.int64 or seg_out.dtype != torch.int64
            or unique_out.numel() < nnz or seg_out.numel() < nnz + 1):
        raise ValueError("unique_ids: ids, unique_out and seg_out are int64; unique_out holds nnz and seg_out nnz + 1 entries")
    for name, t in (("inverse_out", inverse_out), ("perm_out", perm_out)):
        if t.dtype != torch.int32 or t.numel() < nnz:
            raise ValueError(f"unique_ids: {name} must be int32 [{nnz}]")
    if count_dev.dtype != torch.int32 or count_dev.numel() < 1:
        raise ValueError("unique_ids: count_dev is an int32 word on the device")
    dev = seg_out.device
    w = ws.get(unique_ids_workspace_bytes(nnz, int(rows)), dev) if isinstance(ws, Workspace) else ws
    with _on_device(dev):
        _check(LIB.ttemb_unique_ids(_ptr(indices), nnz, int(rows), _ptr(unique_out), _ptr(inverse_out), _ptr(perm_out),
                                    _ptr(seg_out), _ptr(count_dev), _ptr(w), w.numel(), _stream(seg_out)))


def unique_ids_n_workspace_bytes(nnz_cap: int, rows: int) -> int:
    """Bytes ``unique_ids_n`` needs for a buffer of ``nnz_cap`` ids (behind the 40 KB header), whatever the live count."""
    key = ("unique_n", nnz_cap, rows)
    n = _size_cache.get(key)
    if n is None:
        n = int(LIB.ttemb_unique_ids_n_workspace_bytes(nnz_cap, rows))
        if n < 0:
            _check(n)
        n = _size_cache[key] = n
    return n


def unique_ids_n(indices: torch.Tensor, rows: int, unique_out: torch.Tensor, inverse_out: torch.Tensor, perm_out: torch.Tensor,
                 seg_out: torch.Tensor, count_dev: torch.Tensor, ws, nnz_dev: Optional[torch.Tensor] = None) -> None:
    """``unique_ids`` of the first ``n`` ids of ``indices`` (``ttemb_unique_ids_n``): ``n`` is read on the device from the
    int32 word ``nnz_dev`` (None: all), ``indices.numel()`` is the capacity that sizes the launches and the sort's storage.
    The outputs are those of ``unique_ids(indices[:n], ...)``; nothing past ``U`` / ``n`` / ``U + 1`` is written except
    ``perm_out[n:]``, and ``indices[n:]`` influences nothing.  Capturable: nothing on the host depends on ``n``.  ``ws``: a
    ``Workspace``, or a uint8 tensor of ``unique_ids_n_workspace_bytes(nnz_cap, rows)``."""
    nnz = indices.numel()
    if (indices.dtype != torch.int64 or unique_out.dtype != torch.int64 or seg_out.dtype != torch.int64
            or unique_out.numel() < nnz or seg_out.numel() < nnz + 1):
        raise ValueError("unique_ids_n: ids, unique_out and seg_out are int64; unique_out holds nnz and seg_out nnz + 1 entries")
    for name, t in (("inverse_out", inverse_out), ("perm_out", perm_out)):
        if t.dtype != torch.int32 or t.numel() < nnz:
            raise ValueError(f"unique_ids_n: {name} must be int32 [{nnz}]")
    if count_dev.dtype != torch.int32 or count_dev.numel() < 1:
        raise ValueError("unique_ids_n: count_dev is an int32 word on the device")
    dev = seg_out.device
    w = ws.get(unique_ids_n_workspace_bytes(nnz, int(rows)), dev) if isinstance(ws, Workspace) else ws
    with _on_device(dev):
        _check(LIB.ttemb_unique_ids_n(_ptr(indices), nnz, _count_word(nnz_dev), int(rows), _ptr(unique_out), _ptr(inverse_out),
                                      _ptr(perm_out), _ptr(seg_out), _ptr(count_dev), _ptr(w), w.numel(), _stream(seg_out)))


def _check_map(what: str, t: torch.Tensor, nnz: int, dtype=torch.int32, n: Optional[int] = None) -> None:
    n = nnz if n is None else n
    if t.dtype != dtype or t.numel() < n:
        raise ValueError(f"{what} must be {dtype} with at least {n} elements, got {t.dtype} {list(t.shape)}")


def bag_reduce_mapped(rows: torch.Tensor, map_: torch.Tensor, weights: Optional[torch.Tensor], offsets: torch.Tensor,
                      output: torch.Tensor, ws: Workspace, nnz_dev: Optional[torch.Tensor] = None, counted: bool = False) -> None:
    """``output[b] = sum_{n in bag b} weights[n] rows[map_[n]]`` (``ttemb_bag_reduce_mapped``; ``weights`` None: 1): rows
    [cap, D] holds one row per distinct id, ``map_`` (int32 ``[nnz]``) every position's row; output [B, D] fully written.
    ``counted`` (here and in the backward): the ``*_n`` entry point, whose kernels stop at the id count in ``nnz_dev``."""
    cap, D = rows.shape
    nnz, B = map_.numel(), offsets.numel() - 1
    _check_map("bag_reduce_mapped: the map", map_, nnz)
    if weights is not None:
        _check_weights(weights, nnz, rows)
    _check_sizes((rows,), cap * D)
    _check_sizes((output,), B * D)
    dev = output.device
    w = ws.get(bag_workspace_bytes(nnz, B, D), dev)
    with _on_device(dev):
        if counted:
            _check(LIB.ttemb_bag_reduce_mapped_n(_ptr(rows), cap, _ptr(map_), _ptr(weights), _ptr(offsets), nnz,
                                                 _count_word(nnz_dev), B, D, _ptr(output), _ptr(w), w.numel(), _stream(output)))
        else:
            _check(LIB.ttemb_bag_reduce_mapped(_ptr(rows), cap, _ptr(map_), _ptr(weights), _ptr(offsets), nnz, B, D, _ptr(output),
                                               _ptr(w), w.numel(), _stream(output)))


def bag_reduce_mapped_backward(d_output: torch.Tensor, weights: Optional[torch.Tensor], map_: torch.Tensor, perm: torch.Tensor,
                               seg: torch.Tensor, count_dev: torch.Tensor, offsets: torch.Tensor, d_rows: torch.Tensor,
                               ws: Workspace, rows: Optional[torch.Tensor] = None,
                               d_weights: Optional[torch.Tensor] = None, nnz_dev: Optional[torch.Tensor] = None,
                               counted: bool = False) -> None:
    """``d_rows[j] = sum_{k in [seg[j], seg[j+1])} weights[perm[k]] d_output[bag(perm[k])]`` for the ``count_dev`` distinct ids
    (rows past them are neither written nor read), and ``d_weights[n] = <d_output[bag(n)], rows[map_[n]]>`` when ``d_weights``
    is given (then ``rows`` is needed) (``ttemb_bag_reduce_mapped_backward``).  ``perm`` / ``seg`` / ``count_dev``: what
    ``unique_ids`` wrote next to ``map_`` (its ``inverse_out``)."""
    cap, D = d_rows.shape
    nnz, B = map_.numel(), offsets.numel() - 1
    _check_map("bag_reduce_mapped_backward: the map", map_, nnz)
    _check_map("bag_reduce_mapped_backward: perm", perm, nnz)
    _check_map("bag_reduce_mapped_backward: seg", seg, nnz, torch.int64, nnz + 1)
    if weights is not None:
        _check_weights(weights, nnz, d_rows)
    _check_sizes((d_output,), B * D)
    _check_sizes((rows,), cap * D)
    if d_weights is not None:
        _check_sizes((d_weights,), nnz)
    dev = d_rows.device
    # the chunk partials of the pool, and behind them one int32 per position (its bag), rounded up to 256 bytes
    w = ws.get(bag_workspace_bytes(nnz, B, D) + ((4 * nnz + 255) & ~255), dev)
    with _on_device(dev):
        if counted:
            _check(LIB.ttemb_bag_reduce_mapped_backward_n(_ptr(d_output), _ptr(weights), _ptr(rows), cap, _ptr(map_), _ptr(perm),
                                                          _ptr(seg), _count_word(count_dev), _ptr(offsets), nnz,
                                                          _count_word(nnz_dev), B, D, _ptr(d_rows), _ptr(d_weights), _ptr(w),
                                                          w.numel(), _stream(d_rows)))
        else:
            _check(LIB.ttemb_bag_reduce_mapped_backward(_ptr(d_output), _ptr(weights), _ptr(rows), cap, _ptr(map_), _ptr(perm),
                                                        _ptr(seg), _count_word(count_dev), _ptr(offsets), nnz, B, D, _ptr(d_rows),
                                                        _ptr(d_weights), _ptr(w), w.numel(), _stream(d_rows)))


def cache_update(indices: torch.Tensor, hashtbl: torch.Tensor, cache_freq: torch.Tensor, one_sweep: bool = False) -> None:
    """``one_sweep``: the reference's probe-and-insert in one pass (bit-for-bit its table, including the re-insertion of
    cached ids after evictions) instead of looking the key up in all of its probe slots first."""
    if indices.numel() == 0:
        return
    fn = LIB.ttemb_cache_update_one_sweep if one_sweep else LIB.ttemb_cache_update
    with _on_device(indices.device):
        _check(fn(_ptr(indices), indices.numel(), _ptr(hashtbl), _ptr(cache_freq), hashtbl.numel(), _stream(indices)))


def cache_populate(shape: Shape, cores, hashtbl, cache_freq, cache_state, cache_weight, ws: Workspace) -> None:
    dev = hashtbl.device
    H, C = hashtbl.numel(), cache_weight.shape[0]
    w = ws.get(workspace_bytes(shape, OP_CACHE_POPULATE, H, C), dev)
    with _on_device(dev):
        _check(LIB.ttemb_cache_populate(ctypes.byref(shape), _ptr_array(cores), _ptr(hashtbl), _ptr(cache_freq),
                                        _ptr(cache_state), H, _ptr(cache_weight), C, _ptr(w), w.numel(),
                                        _stream(hashtbl)))


def preprocess(indices, offsets, B: int, warmup: bool, hashtbl, cache_state, indices_out, rowidx_out,
               cache_loc_out, nnz_tt_dev, ws: Workspace, dup_stamp=None, epoch: int = 0, cache_freq=None) -> None:
    """``dup_stamp`` (int32[C] of scratch): ``nnz_tt_dev`` must hold two int32 and its second word tells the cache
    backward whether a cache row occurs twice in this call.  ``cache_freq``: the LFU update of the same ids rides in
    the probe pass (``ttemb_preprocess_update``; live cache only)."""
    dev = indices.device
    nnz = indices.numel()
    H = 0 if hashtbl is None else hashtbl.numel()
    need = 0 if (warmup or H == 0) else workspace_bytes(None, OP_PREPROCESS, nnz, B)
    w = ws.get(need, dev)
    if cache_freq is not None:
        if warmup or H == 0:
            raise RuntimeError("the fused probe pass serves a live cache only")
        with _on_device(dev):
            _check(LIB.ttemb_preprocess_update(_ptr(indices), _ptr(offsets), nnz, B, _ptr(hashtbl), _ptr(cache_freq),
                                               _ptr(cache_state), H, _ptr(indices_out), _ptr(rowidx_out),
                                               _ptr(cache_loc_out), _ptr(nnz_tt_dev), _ptr(dup_stamp), _ptr(w), w.numel(),
                                               _stream(indices)))
        return
    with _on_device(dev):
        _check(LIB.ttemb_preprocess(_ptr(indices), _ptr(offsets), nnz, B, 1 if warmup else 0, _ptr(hashtbl),
                                    _ptr(cache_state), H, _ptr(indices_out), _ptr(rowidx_out),
                                    _ptr(cache_loc_out), _ptr(nnz_tt_dev), _ptr(dup_stamp), epoch, _ptr(w), w.numel(),
                                    _stream(indices)))


def cache_forward(cache_loc, rowidx, start: int, start_dev, nnz: int, cache_weight, output,
                  offsets: Optional[torch.Tensor] = None) -> None:
    with _on_device(output.device):
        _check(LIB.ttemb_cache_forward(_ptr(cache_loc), _ptr(rowidx), _ptr(offsets), start, _ptr(start_dev), nnz,
                                       _ptr(cache_weight), cache_weight.shape[1], _ptr(output),
                                       _stream(output)))


def cache_backward_sgd(cache_loc, rowidx, start: int, start_dev, nnz: int, d_output, lr: float,
                       cache_weight, dup_dev=None) -> None:
    with _on_device(d_output.device):
        _check(LIB.ttemb_cache_backward_sgd(_ptr(cache_loc), _ptr(rowidx), start, _ptr(start_dev), nnz,
                                            _ptr(d_output), cache_weight.shape[1], lr, _ptr(cache_weight),
                                            _ptr(dup_dev), _stream(d_output)))


def cache_backward_dense(cache_loc, rowidx, start: int, start_dev, nnz: int, d_output,
                         d_cache_weight, dup_dev=None) -> None:
    with _on_device(d_output.device):
        _check(LIB.ttemb_cache_backward_dense(_ptr(cache_loc), _ptr(rowidx), start, _ptr(start_dev), nnz,
                                              _ptr(d_output), d_cache_weight.shape[1],
                                              d_cache_weight.shape[0], _ptr(d_cache_weight),
                                              _ptr(dup_dev), _stream(d_output)))


def cache_backward_rowwise_adagrad(cache_loc, rowidx, start: int, start_dev, nnz: int, d_output, lr: float,
                                   eps: float, state_sum, cache_weight) -> None:
    with _on_device(d_output.device):
        _check(LIB.ttemb_cache_backward_rowwise_adagrad(_ptr(cache_loc), _ptr(rowidx), start, _ptr(start_dev),
                                                        nnz, _ptr(d_output), cache_weight.shape[1], lr, eps,
                                                        _ptr(state_sum), _ptr(cache_weight),
                                                        _stream(d_output)))


_ID_DTYPES = (torch.int64, torch.int32)


def stage_call(indices: torch.Tensor, offsets: Optional[torch.Tensor], indices_out: torch.Tensor, offsets_out: torch.Tensor,
               nnz_dev_out: torch.Tensor, B_live: Optional[int] = None) -> None:
    """One call of any size into the static buffers of a captured lookup, in ONE launch (``ttemb_stage_call``): the ids
    (int64 or int32, widened) into ``indices_out[:n]`` -- the rest of it is not touched --, the offsets (int64 or int32;
    ``None``: bags of one id) into ``offsets_out[:B_live + 1]``, ``n`` into every offsets word past them and into the int32
    word ``nnz_dev_out``.  The capacities are the lengths of the two outputs; a call past them raises ``RuntimeError`` with
    nothing launched."""
    n = indices.numel()
    if B_live is None:
        B_live = n if offsets is None else offsets.numel() - 1
    if (indices.dtype not in _ID_DTYPES or (offsets is not None and offsets.dtype not in _ID_DTYPES)
            or indices_out.dtype != torch.int64 or offsets_out.dtype != torch.int64 or nnz_dev_out.dtype != torch.int32):
        raise ValueError("stage_call: ids and offsets must be int64 or int32, the staged buffers int64 and the count word int32")
    if offsets_out.numel() < 1 or nnz_dev_out.numel() < 1 or (offsets is not None and B_live > offsets.numel() - 1):
        raise ValueError("stage_call: offsets_out needs B_cap + 1 entries, nnz_dev_out one int32 and offsets B_live + 1 entries")
    with _on_device(offsets_out.device):
        rc = LIB.ttemb_stage_call(_ptr(indices), 1 if indices.dtype == torch.int32 else 0, n, _ptr(offsets),
                                  1 if offsets is not None and offsets.dtype == torch.int32 else 0, B_live, _ptr(indices_out),
                                  indices_out.numel(), _ptr(offsets_out), offsets_out.numel() - 1, _ptr(nnz_dev_out),
                                  _stream(offsets_out))
    if rc:
        _check(rc)


def stage_bags(indices: torch.Tensor, offsets: Optional[torch.Tensor], weights: Optional[torch.Tensor],
               indices_out: torch.Tensor, offsets_out: torch.Tensor, weights_out: Optional[torch.Tensor],
               nnz_dev_out: torch.Tensor, fanout: int = 0, B_live: Optional[int] = None) -> None:
    """``stage_call`` for a pooled call, in ONE launch (``ttemb_stage_bags``): also the float32 ``weights`` (``[n]``, or None)
    into ``weights_out[:n]``, and with ``fanout > 0`` (``n = B_live * fanout`` ids, no ``offsets``) the offsets
    ``0, fanout, 2 fanout, ...`` generated on the device.  ``weights`` and ``weights_out`` come together."""
    n = indices.numel()
    if B_live is None:
        B_live = n // fanout if fanout > 0 else (n if offsets is None else offsets.numel() - 1)
    if (indices.dtype not in _ID_DTYPES or (offsets is not None and offsets.dtype not in _ID_DTYPES)
            or indices_out.dtype != torch.int64 or offsets_out.dtype != torch.int64 or nnz_dev_out.dtype != torch.int32):
        raise ValueError("stage_bags: ids and offsets must be int64 or int32, the staged buffers int64 and the count word int32")
    if offsets_out.numel() < 1 or nnz_dev_out.numel() < 1 or (offsets is not None and B_live > offsets.numel() - 1):
        raise ValueError("stage_bags: offsets_out needs B_cap + 1 entries, nnz_dev_out one int32 and offsets B_live + 1 entries")
    if (weights is None) != (weights_out is None):
        raise ValueError("stage_bags: weights and weights_out come together")
    if weights is not None and (weights.dtype != torch.float32 or weights.numel() != n or weights_out.dtype != torch.float32
                                or weights_out.numel() < n):
        raise ValueError(f"stage_bags: weights must be float32 with {n} elements and weights_out float32 with room for them")
    # (a call without ids brings an empty weight tensor, which has no address: its static buffer is then left out as well)
    w_in = None if weights is None or n == 0 else _ptr(weights)
    w_out = None if w_in is None else _ptr(weights_out)
    with _on_device(offsets_out.device):
        rc = LIB.ttemb_stage_bags(_ptr(indices), 1 if indices.dtype == torch.int32 else 0, n, _ptr(offsets),
                                  1 if offsets is not None and offsets.dtype == torch.int32 else 0, B_live, int(fanout), w_in,
                                  _ptr(indices_out), indices_out.numel(), _ptr(offsets_out), offsets_out.numel() - 1, w_out,
                                  _ptr(nnz_dev_out), _stream(offsets_out))
    if rc:
        _check(rc)


def core_ptrs(tt_cores: Sequence[torch.Tensor], table: int = 0):
    """Pointer array of the per-table [p_t, row] slices of [num_tables, p_t, row] parameters: what core_views gives,
    without creating view tensors (this sits on the host path of every step)."""
    arr = (ctypes.c_void_p * MAX_CORES)()
    for i, c in enumerate(tt_cores):
        if c.dtype != torch.float32 or not c.is_cuda or not c.is_contiguous():
            raise RuntimeError("tt_cores must be contiguous float32 tensors on a ROCm device (no CPU fallback)")
        arr[i] = c.data_ptr() + (table * c.stride(0) * 4 if c.dim() == 3 and table else 0)
    return arr


def core_views(tt_cores: Sequence[torch.Tensor], table: int = 0) -> List[torch.Tensor]:
    """[num_tables, p_t, row] parameters -> contiguous per-table [p_t, row] views."""
    out = []
    for c in tt_cores:
        v = c.data if isinstance(c, torch.nn.Parameter) else c
        v = v[table] if v.dim() == 3 else v
        if not v.is_contiguous():
            raise RuntimeError("tt_cores must be contiguous")
        out.append(v)
    return out


class LeanCalls:
    """The two native calls of a training step (forward, fused-optimiser backward) of ONE single-table module with their
    invariant arguments bound once: shape reference, core / optimiser-state pointer arrays (refreshed only when a
    parameter's storage moved), workspace and plan sizes per (nnz, B).  At 2 048 ids the GPU work of a step is ~25 us, so
    every microsecond of Python between the two launches is step time."""

    def __init__(self, shape: Shape, ws: Workspace) -> None:
        self.shape, self.shape_ref, self.ws = shape, ctypes.byref(shape), ws
        self.sizes: dict = {}
        self.epoch = -1
        self.core_key, self.core_arr = None, None
        self.state_key, self.state_arr = None, None
        self.state2_key, self.state2_arr = None, None   # (Adam: the second moment)
        self.grad_key, self.grad_arr = None, None
        self.step = Step(0.0)   # (reused by every backward: no object per call)

    def _entry(self, nnz: int, B: int):
        if self.epoch != path_epoch:
            self.sizes.clear()
            self.epoch = path_epoch
        e = self.sizes.get((nnz, B))
        if e is None:
            if len(self.sizes) > 1024:
                self.sizes.clear()
            e = self.sizes[(nnz, B)] = (workspace_bytes(self.shape, OP_FORWARD, nnz, B),
                                        workspace_bytes(self.shape, OP_BACKWARD, nnz, B), plan_bytes(self.shape, nnz))
        return e

    @staticmethod
    def _ptrs(tensors, key, arr):
        k = tuple(t.data_ptr() for t in tensors)
        if k != key:
            arr = core_ptrs(tensors)   # validates dtype / device / contiguity
            key = k
        return key, arr

    def forward(self, cores, indices, offsets, nnz: int, B: int, out, keep_plan: bool = True, nnz_dev=None):
        """``keep_plan=False``: a forward whose backward never comes (inference): the plan lives and dies in the workspace.
        ``nnz_dev`` (int32[1] on the device): the live id count, <= ``nnz``; the launches are sized by ``nnz``."""
        fwd_ws, _, plan_n = self._entry(nnz, B)
        self.core_key, self.core_arr = self._ptrs(cores, self.core_key, self.core_arr)
        dev = out.device
        w = self.ws.get(fwd_ws, dev)
        plan = torch.empty(plan_n, dtype=torch.uint8, device=dev) if plan_n > 0 and keep_plan else None
        with _on_device(dev):
            rc = LIB.ttemb_forward(self.shape_ref, self.core_arr, indices.data_ptr() if nnz else None, None, offsets.data_ptr(),
                                   nnz, None if nnz_dev is None else nnz_dev.data_ptr(), B, out.data_ptr() if B else None,
                                   w.data_ptr(), w.numel(),
                                   plan.data_ptr() if plan is not None else None, plan_n if plan is not None else 0, _stream(out))
        if rc:
            _check(rc)
        return plan

    def forward_split(self, cores, indices, offsets, nnz: int, B: int, out, pending):
        """The forward of a data-parallel step (ttemb_dist): the id-only half (grouping into the plan) is enqueued, THEN
        ``pending()`` finishes the previous step's all-reduce + update, then the half that reads the cores.  A call without a
        plan (per-bag / scalar kernels, a call in pieces) has no id-only half: ``pending()``, then the whole forward."""
        fwd_ws, _, plan_n = self._entry(nnz, B)
        self.core_key, self.core_arr = self._ptrs(cores, self.core_key, self.core_arr)
        dev = out.device
        w = self.ws.get(fwd_ws, dev)
        plan = torch.empty(plan_n, dtype=torch.uint8, device=dev) if plan_n > 0 else None
        args = (self.shape_ref, self.core_arr, indices.data_ptr() if nnz else None, None, offsets.data_ptr(), nnz, None, B,
                out.data_ptr() if B else None, w.data_ptr(), w.numel(), plan.data_ptr() if plan is not None else None, plan_n,
                _stream(out))
        with _on_device(dev):
            if plan is None:
                pending()
                rc = LIB.ttemb_forward(*args)
            else:
                rc = LIB.ttemb_forward_group(*args)
                if rc == 0:
                    pending()
                    rc = LIB.ttemb_forward_lookup(*args)
        if rc:
            _check(rc)
        return plan

    def backward_dense(self, cores, indices, offsets, nnz: int, B: int, d_output, grads, plan) -> None:
        """Dense core gradients into ``grads`` (a fixed list of tensors: their pointer array is cached)."""
        _, bwd_ws, plan_n = self._entry(nnz, B)
        self.core_key, self.core_arr = self._ptrs(cores, self.core_key, self.core_arr)
        self.grad_key, self.grad_arr = self._ptrs(grads, self.grad_key, self.grad_arr)
        dev = d_output.device
        w = self.ws.get(bwd_ws, dev)
        pp, pn = (plan.data_ptr(), plan_n) if plan is not None else (None, 0)
        with _on_device(dev):
            rc = LIB.ttemb_backward_dense(self.shape_ref, self.core_arr, indices.data_ptr() if nnz else None, None, offsets.data_ptr(),
                                          nnz, None, B, d_output.data_ptr() if B else None, self.grad_arr, w.data_ptr(), w.numel(),
                                          pp, pn, _stream(d_output))
        if rc:
            _check(rc)

    def backward(self, cores, state, indices, offsets, nnz: int, B: int, d_output, lr, eps: float, plan, adam=None,
                 nnz_dev=None):
        """``adam = (exp_avg_sq, step, AdamParams)``: the fused Adam step, ``state`` then the first moment.  ``nnz_dev``: as
        in ``forward``.  ``lr``: a float, or a float32[1] device tensor -- the rate is then read on the device
        (``ttemb_backward_step``) and the one in the ``AdamParams`` ignored."""
        _, bwd_ws, plan_n = self._entry(nnz, B)
        self.core_key, self.core_arr = self._ptrs(cores, self.core_key, self.core_arr)
        dev = d_output.device
        w = self.ws.get(bwd_ws, dev)
        pp, pn = (plan.data_ptr(), plan_n) if plan is not None else (None, 0)
        if state is not None:
            self.state_key, self.state_arr = self._ptrs(state, self.state_key, self.state_arr)
            state = self.state_arr
        if adam is not None:
            self.state2_key, self.state2_arr = self._ptrs(adam[0], self.state2_key, self.state2_arr)
            adam = (self.state2_arr, adam[1], adam[2])
        self.step.__init__(lr, eps, state, adam)
        with _on_device(dev):
            rc = _run_step("plain", self.step, (self.shape_ref, self.core_arr),
                           (indices.data_ptr() if nnz else None, None, offsets.data_ptr(), nnz,
                            None if nnz_dev is None else nnz_dev.data_ptr(), B, d_output.data_ptr() if B else None),
                           (w.data_ptr(), w.numel(), pp, pn, _stream(d_output)))
        if rc:
            _check(rc)
