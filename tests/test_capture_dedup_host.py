"""Captured dedup bags, host side (no GPU): the symbols of ``include/ttemb_unique_n.h``, the parent's declarations unchanged,
the argument checks that run before any launch, the refusals of ``capture_bags(dedup=True)`` a module raises without a device,
and no spills in the new and the changed kernels.  Queries run in a child process with no device visible, like
test_dedup_host.py."""
import os
import re
import subprocess
import sys

import test_dedup_host as dh

ROOT, PKG = dh.ROOT, dh.PKG

UNIQUE_N_SYMBOLS = ("ttemb_unique_ids_n_workspace_bytes", "ttemb_unique_ids_n", "ttemb_bag_reduce_mapped_n",
                    "ttemb_bag_reduce_mapped_backward_n")


def test_the_new_symbols_are_exported_and_bound():
    dh._child("import ctypes, ttemb_native as n\n"
              f"names = {UNIQUE_N_SYMBOLS!r}\n"
              "assert tuple(n.UNIQUE_N_SYMBOLS) == names\n"
              f"assert tuple(n.UNIQUE_SYMBOLS) == {dh.UNIQUE_SYMBOLS!r}   # the parent's tuple stays\n"
              "assert not set(names) & set(n.EXPORTED_SYMBOLS + n.BAGS_SYMBOLS + n.PADS_SYMBOLS + n.UNIQUE_SYMBOLS)\n"
              "for s in names:\n"
              "    f = getattr(n.LIB, s)\n"
              "    assert f.argtypes is not None\n"
              "    assert f.restype is (ctypes.c_int64 if s.endswith('_workspace_bytes') else ctypes.c_int), s\n"
              "# each is its parent plus the count word\n"
              "assert len(n.LIB.ttemb_unique_ids_n.argtypes) == len(n.LIB.ttemb_unique_ids.argtypes) + 1 == 12\n"
              "assert len(n.LIB.ttemb_bag_reduce_mapped_n.argtypes) == len(n.LIB.ttemb_bag_reduce_mapped.argtypes) + 1 == 13\n"
              "assert len(n.LIB.ttemb_bag_reduce_mapped_backward_n.argtypes) == 18\n"
              "assert len(n.LIB.ttemb_bag_reduce_mapped_backward.argtypes) == 17\n"
              "assert n.LIB.ttemb_abi_version() == 4 and n.ABI_VERSION == 4   # additive symbols: the version stays\n"
              "assert callable(n.unique_ids_n) and callable(n.unique_ids_n_workspace_bytes)\n")


def test_the_new_header_declares_exactly_the_new_symbols_and_the_parent_abi_is_unchanged():
    with open(os.path.join(ROOT, "include", "ttemb_unique_n.h")) as f:
        mine = dh._declarations(f.read())
    assert sorted(mine) == sorted(UNIQUE_N_SYMBOLS)
    with open(os.path.join(ROOT, "include", "ttemb_unique.h")) as f:
        parents = dh._declarations(f.read())
    assert sorted(parents) == sorted(dh.UNIQUE_SYMBOLS)
    # each pool is its parent with `const int32_t* nnz_dev` behind nnz
    for name in ("ttemb_bag_reduce_mapped", "ttemb_bag_reduce_mapped_backward"):
        want = parents[name].replace(name + "(", name + "_n(").replace("int64_t nnz,", "int64_t nnz, const int32_t* nnz_dev,")
        assert mine[name + "_n"] == want, name
    with open(os.path.join(ROOT, "include", "ttemb.h")) as f:
        now_text = f.read()
    assert re.search(r'#include "ttemb_pads.h"\s*\n#include "ttemb_unique.h"\s*\n#include "ttemb_unique_n.h"', now_text)
    assert "#define TTEMB_ABI_VERSION 4" in now_text
    with open(os.path.join(ROOT, "tests", "golden", "ttemb_abi4_parent.h.txt")) as f:
        parent = dh._declarations(f.read())
    now = dh._declarations(now_text)
    assert len(parent) >= 55   # (the parser sees them)
    for name, decl in parent.items():
        assert now.get(name) == decl, name
    assert not set(now) & set(UNIQUE_N_SYMBOLS)   # ttemb.h's own set is pinned: the new ones live in their own header


def test_the_new_entry_points_check_their_arguments_before_any_launch():
    """Pointers that would fault when read (0x10 ...): the codes come back, so nothing was launched or read."""
    dh._child("import ttemb_native as n\n"
              "L = n.LIB\n"
              "P, O, W, C, N, BIG = 0x10, 0x20, 0x30, 0x40, 0x50, 1 << 20   # (never dereferenced)\n"
              "# ttemb_unique_ids_n(indices, nnz_cap, nnz_dev, rows, unique_out, inverse_out, perm_out, seg_out, count_dev, ws,\n"
              "#                    ws_bytes, stream)\n"
              "bad = {\n"
              "    'negative nnz_cap': (P, -1, N, 100, O, O, O, O, C, W, BIG, None),\n"
              "    'nnz_cap past int32': (P, 2 ** 31, N, 100, O, O, O, O, C, W, 1 << 40, None),\n"
              "    'no rows':          (P, 8, N, 0, O, O, O, O, C, W, BIG, None),\n"
              "    'null indices':     (None, 8, N, 100, O, O, O, O, C, W, BIG, None),\n"
              "    'null unique_out':  (P, 8, N, 100, None, O, O, O, C, W, BIG, None),\n"
              "    'null inverse_out': (P, 8, None, 100, O, None, O, O, C, W, BIG, None),\n"
              "    'null perm_out':    (P, 8, N, 100, O, O, None, O, C, W, BIG, None),\n"
              "    'null seg_out':     (P, 8, N, 100, O, O, O, None, C, W, BIG, None),\n"
              "    'null seg_out, no ids': (None, 0, N, 100, None, None, None, None, C, W, BIG, None),\n"
              "    'null count_dev':   (P, 8, N, 100, O, O, O, O, None, W, BIG, None),\n"
              "    'null workspace':   (P, 8, N, 100, O, O, O, O, C, None, BIG, None),\n"
              "}\n"
              "for what, args in bad.items():\n"
              "    assert L.ttemb_unique_ids_n(*args) == -1, what   # TTEMB_E_BADARG\n"
              "    assert b'ttemb_unique_ids_n' in L.ttemb_last_error(), what\n"
              "assert L.ttemb_unique_ids_n(P, 8, N, 100, O, O, O, O, C, W, 16, None) == -2   # smaller than the header\n"
              "assert L.ttemb_unique_ids_n(P, 8, N, 100, O, O, O, O, C, W, 40960, None) == -2   # TTEMB_E_WORKSPACE\n"
              "f = L.ttemb_unique_ids_n_workspace_bytes\n"
              "assert f(-1, 100) == -1 and f(8, 0) == -1 and f(2 ** 31, 100) == -1\n"
              "assert f(0, 100) == 40960 + 256   # no ids: the header and one tile count\n"
              "# ttemb_bag_reduce_mapped_n(rows, cap, map, weights, offsets, nnz, nnz_dev, B, D, output, ws, ws_bytes, stream)\n"
              "bad = {\n"
              "    'negative nnz':   (P, 8, O, None, P, -1, N, 4, 16, O, W, BIG, None),\n"
              "    'D not 4k':       (P, 8, O, None, P, 8, N, 4, 18, O, W, BIG, None),\n"
              "    'nnz past int32': (P, 8, O, None, P, 2 ** 31, N, 4, 16, O, W, 1 << 50, None),\n"
              "    'null rows':      (None, 8, O, None, P, 8, N, 4, 16, O, W, BIG, None),\n"
              "    'null map':       (P, 8, None, None, P, 8, None, 4, 16, O, W, BIG, None),\n"
              "    'no capacity':    (P, 0, O, None, P, 8, N, 4, 16, O, W, BIG, None),\n"
              "    'null offsets':   (P, 8, O, None, None, 8, N, 4, 16, O, W, BIG, None),\n"
              "    'null output':    (P, 8, O, None, P, 8, N, 4, 16, None, W, BIG, None),\n"
              "    'misaligned':     (P + 4, 8, O, None, P, 8, N, 4, 16, O, W, BIG, None),\n"
              "}\n"
              "for what, args in bad.items():\n"
              "    assert L.ttemb_bag_reduce_mapped_n(*args) == -1, what\n"
              "    assert b'ttemb_bag_reduce_mapped' in L.ttemb_last_error(), what\n"
              "assert L.ttemb_bag_reduce_mapped_n(P, 8, O, None, P, 8, N, 4, 16, O, W, 40960, None) == -2\n"
              "# ttemb_bag_reduce_mapped_backward_n(d_output, weights, rows, cap, map, perm, seg, count_dev, offsets, nnz, nnz_dev,\n"
              "#                                    B, D, d_rows, d_weights, ws, ws_bytes, stream)\n"
              "bad = {\n"
              "    'negative B':      (P, None, None, 8, O, O, O, C, P, 8, N, -4, 16, O, None, W, BIG, None),\n"
              "    'null d_output':   (None, None, None, 8, O, O, O, C, P, 8, N, 4, 16, O, None, W, BIG, None),\n"
              "    'null map':        (P, None, None, 8, None, O, O, C, P, 8, N, 4, 16, O, None, W, BIG, None),\n"
              "    'null perm':       (P, None, None, 8, O, None, O, C, P, 8, None, 4, 16, O, None, W, BIG, None),\n"
              "    'null seg':        (P, None, None, 8, O, O, None, C, P, 8, N, 4, 16, O, None, W, BIG, None),\n"
              "    'null count_dev':  (P, None, None, 8, O, O, O, None, P, 8, N, 4, 16, O, None, W, BIG, None),\n"
              "    'null d_rows':     (P, None, None, 8, O, O, O, C, P, 8, N, 4, 16, None, None, W, BIG, None),\n"
              "    'd_w without rows': (P, None, None, 8, O, O, O, C, P, 8, N, 4, 16, O, W, W, BIG, None),\n"
              "    'nnz past int32':  (P, None, None, 8, O, O, O, C, P, 2 ** 31, N, 4, 16, O, None, W, 1 << 50, None),\n"
              "}\n"
              "for what, args in bad.items():\n"
              "    assert L.ttemb_bag_reduce_mapped_backward_n(*args) == -1, what\n"
              "    assert b'ttemb_bag_reduce_mapped_backward' in L.ttemb_last_error(), what\n"
              "assert L.ttemb_bag_reduce_mapped_backward_n(P, None, None, 8, O, O, O, C, P, 8, N, 4, 16, O, None, W, 40960, None) == -2\n")


def test_the_refusals_of_capture_bags_dedup_are_raised_without_a_device():
    dh._child("import inspect, pytest, torch\n"
              "from FBTT.tt_embeddings_ops import TTEmbeddingBag, CapturedBags\n"
              "args = (1000, 16, [4, 4], [10, 10, 10], [2, 2, 4])\n"
              "sig = inspect.signature(TTEmbeddingBag.capture_bags)\n"
              "assert list(sig.parameters)[-1] == 'dedup' and sig.parameters['dedup'].default is False\n"
              "assert sig.parameters['dedup'].kind is inspect.Parameter.KEYWORD_ONLY\n"
              "plain = TTEmbeddingBag(*args, use_cache=False, sparse=True)\n"
              "with pytest.raises(ValueError, match=\"dedup with mode='max'\"):   # the eager reason\n"
              "    plain.capture_bags(16, 4, mode='max', dedup=True)\n"
              "with pytest.raises(ValueError, match='2\\\\^20 ids'):\n"
              "    plain.capture_bags((1 << 20) + 8, 4, mode='mean', dedup=True)\n"
              "with pytest.raises(ValueError, match='weighted bags are only supported'):   # the checks of every capture first\n"
              "    plain.capture_bags(16, 4, mode='mean', weighted=True, dedup=True)\n"
              "exact = TTEmbeddingBag(*args, use_cache=False, sparse=True, deterministic=True)\n"
              "for variable in (False, True):\n"
              "    with pytest.raises(RuntimeError, match='not served in exact mode'):\n"
              "        exact.capture_bags(16, 4, mode='mean', variable=variable, dedup=True)\n"
              "on = TTEmbeddingBag(*args, use_cache=False, sparse=True, dedup=True)\n"
              "for kw in ({}, {'dedup': True}):   # a dedup=True module: refused as before, with the text of before\n"
              "    with pytest.raises(ValueError, match=r'capture_bags\\(\\) on a dedup=True module is not supported: the pass'):\n"
              "        on.capture_bags(16, 4, mode='mean', **kw)\n"
              "cached = TTEmbeddingBag(*args, use_cache=True, sparse=True, cache_size=10, hashtbl_size=40)\n"
              "cached.warmup = False   # (what cache_populate() leaves)\n"
              "with pytest.raises(RuntimeError, match='live row cache'):\n"
              "    cached.capture_bags(16, 4, mode='mean', dedup=True)\n"
              "CapturedBags.check_dedup(1 << 20, 'mean')   # the largest capacity\n"
              "CapturedBags.check_dedup(16, 'sum')\n")


def test_the_new_and_the_changed_kernels_do_not_spill():
    lib = os.path.join(PKG, "lib", "libttemb_hip.so")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kres.py"), lib, "mapped", "unique_", "--fail-on-scratch"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for k in ("unique_keys_n_kernel", "unique_count_n_kernel", "unique_scatter_n_kernel", "unique_count_kernel",
              "unique_scatter_kernel", "bag_partial_mapped_kernel", "bag_reduce_mapped_kernel", "seg_partial_mapped_kernel",
              "seg_reduce_mapped_kernel", "mapped_weight_grad_kernel"):
        assert k in r.stdout, f"{k} is not in the library"
