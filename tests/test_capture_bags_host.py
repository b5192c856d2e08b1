"""Captured pooled lookups, host side (no GPU): the six new symbols, the argument checks of ``ttemb_stage_bags`` and of the
count-aware pooling calls that run before any launch, ``capture_bags``'s argument errors, and no spills in the new and
changed kernels.  Queries run in a child process with no device visible, like test_padding_host.py."""
import os
import subprocess
import sys


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "falcon-ttdforgnns_amd")

NEW_SYMBOLS = ("ttemb_stage_bags", "ttemb_bag_reduce_n", "ttemb_bag_reduce_backward_n", "ttemb_bag_max_n",
               "ttemb_bag_max_backward_n", "ttemb_pad_weights_n")


def _child(code):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", "import sys; sys.path[:0] = [sys.argv[1]]\n" + code, PKG], env=env,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def test_the_new_symbols_are_exported_and_bound():
    _child("import ctypes, ttemb_native as n\n"
           f"names = {NEW_SYMBOLS!r}\n"
           "assert tuple(n.BAGS_SYMBOLS) == names\n"
           "assert all(getattr(n.LIB, s).argtypes is not None and getattr(n.LIB, s).restype is ctypes.c_int for s in names)\n"
           "assert n.LIB.ttemb_abi_version() == 4 and n.ABI_VERSION == 4   # additive symbols: the version stays\n"
           "assert callable(n.stage_bags)\n")


def test_the_bags_header_declares_exactly_the_new_symbols():
    """include/ttemb_bags.h (which ttemb.h includes) declares the six symbols and nothing else; ttemb.h still compiles as C."""
    import re
    with open(os.path.join(ROOT, "include", "ttemb_bags.h")) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    assert sorted(re.findall(r"\bint\s+(ttemb_\w+)\s*\(", text)) == sorted(NEW_SYMBOLS)
    with open(os.path.join(ROOT, "include", "ttemb.h")) as f:
        assert '#include "ttemb_bags.h"' in f.read()


def test_stage_bags_checks_its_arguments_before_it_touches_a_pointer():
    """Pointers that would fault when read (0x10 ...): TTEMB_E_BADARG comes back, so nothing was launched or read."""
    _child("import ttemb_native as n\n"
           "f = n.LIB.ttemb_stage_bags\n"
           "P, W = 0x10, 0x20   # (never dereferenced)\n"
           "# (indices_in, i32, n_live, offsets_in, i32, B_live, fanout, weights_in, indices_out, nnz_cap, offsets_out, B_cap,\n"
           "#  weights_out, nnz_dev_out, stream)\n"
           "bad = {\n"
           "    'negative n_live':      (P, 0, -1, P, 0, 4, 0, None, P, 64, P, 32, None, P, None),\n"
           "    'negative B_live':      (P, 0, 8, P, 0, -1, 0, None, P, 64, P, 32, None, P, None),\n"
           "    'negative capacity':    (P, 0, 8, P, 0, 4, 0, None, P, -64, P, 32, None, P, None),\n"
           "    'ids over capacity':    (P, 0, 65, P, 0, 4, 0, None, P, 64, P, 32, None, P, None),\n"
           "    'bags over capacity':   (P, 0, 8, P, 0, 33, 0, None, P, 64, P, 32, None, P, None),\n"
           "    'capacity past int32':  (P, 0, 8, P, 0, 4, 0, None, P, 2 ** 31, P, 32, None, P, None),\n"
           "    'no offsets, B != n':   (P, 0, 8, None, 0, 5, 0, None, P, 64, P, 32, None, P, None),\n"
           "    'null offsets_out':     (P, 0, 8, P, 0, 4, 0, None, P, 64, None, 32, None, P, None),\n"
           "    'null count word':      (P, 0, 8, P, 0, 4, 0, None, P, 64, P, 32, None, None, None),\n"
           "    'null ids':             (None, 0, 8, P, 0, 4, 0, None, P, 64, P, 32, None, P, None),\n"
           "    'weights_in only':      (P, 0, 8, P, 0, 4, 0, W, P, 64, P, 32, None, P, None),\n"
           "    'weights_out only':     (P, 0, 8, P, 0, 4, 0, None, P, 64, P, 32, W, P, None),\n"
           "    'negative fanout':      (P, 0, 8, None, 0, 8, -1, None, P, 64, P, 32, None, P, None),\n"
           "    'fanout with offsets':  (P, 0, 8, P, 0, 4, 2, None, P, 64, P, 32, None, P, None),\n"
           "    'fanout, n mismatch':   (P, 0, 9, None, 0, 4, 2, None, P, 64, P, 32, None, P, None),\n"
           "    'fanout, n overflow':   (P, 0, 8, None, 0, 2 ** 62, 2 ** 40, None, P, 64, P, 2 ** 62, None, P, None),\n"
           "}\n"
           "for what, args in bad.items():\n"
           "    assert f(*args) == -1, what   # TTEMB_E_BADARG\n"
           "    assert b'ttemb_stage_bags' in n.LIB.ttemb_last_error(), what\n")


def test_counted_pooling_checks_its_arguments_before_any_launch():
    """The *_n calls keep the checks of their namesakes, on nnz (the capacity): each returns TTEMB_E_BADARG here."""
    _child("import ttemb_native as n\n"
           "L = n.LIB\n"
           "P, Q, C = 0x100, 0x108, 0x40   # (16-byte aligned, misaligned, a count word: never dereferenced)\n"
           "bad = [\n"
           "    # ttemb_bag_reduce_n(rows, weights, offsets, nnz, nnz_dev, B, D, output, workspace, workspace_bytes, stream)\n"
           "    (L.ttemb_bag_reduce_n, (P, P, P, -1, C, 4, 8, P, P, 1 << 20, None)),\n"
           "    (L.ttemb_bag_reduce_n, (P, P, P, 8, C, -4, 8, P, P, 1 << 20, None)),\n"
           "    (L.ttemb_bag_reduce_n, (P, P, P, 8, C, 4, 6, P, P, 1 << 20, None)),\n"
           "    (L.ttemb_bag_reduce_n, (P, P, None, 8, C, 4, 8, P, P, 1 << 20, None)),\n"
           "    (L.ttemb_bag_reduce_n, (P, None, P, 8, C, 4, 8, P, P, 1 << 20, None)),\n"
           "    (L.ttemb_bag_reduce_n, (Q, P, P, 8, C, 4, 8, P, P, 1 << 20, None)),\n"
           "    # ttemb_bag_reduce_backward_n(d_output, weights, rows, offsets, nnz, nnz_dev, B, D, d_rows, d_weights, ws, bytes, stream)\n"
           "    (L.ttemb_bag_reduce_backward_n, (P, P, P, P, -1, C, 4, 8, P, P, P, 1 << 20, None)),\n"
           "    (L.ttemb_bag_reduce_backward_n, (P, P, P, P, 8, C, 4, 0, P, P, P, 1 << 20, None)),\n"
           "    (L.ttemb_bag_reduce_backward_n, (P, P, P, P, 8, C, 4, 8, None, P, P, 1 << 20, None)),\n"
           "    (L.ttemb_bag_reduce_backward_n, (P, P, None, P, 8, C, 4, 8, P, P, P, 1 << 20, None)),   # d_weights without rows\n"
           "    (L.ttemb_bag_reduce_backward_n, (P, P, P, P, 8, C, 4, 8, Q, P, P, 1 << 20, None)),\n"
           "    # ttemb_bag_max_n(rows, indices, pad, offsets, nnz, nnz_dev, B, D, output, argmax, workspace, bytes, stream)\n"
           "    (L.ttemb_bag_max_n, (P, None, 0, P, -1, C, 4, 8, P, P, P, 1 << 20, None)),\n"
           "    (L.ttemb_bag_max_n, (P, None, 0, P, 2 ** 31, C, 4, 8, P, P, P, 1 << 40, None)),\n"
           "    (L.ttemb_bag_max_n, (P, None, 0, P, 8, C, 4, 8, P, None, P, 1 << 20, None)),\n"
           "    (L.ttemb_bag_max_n, (None, None, 0, P, 8, C, 4, 8, P, P, P, 1 << 20, None)),\n"
           "    (L.ttemb_bag_max_n, (P, None, 0, P, 8, C, 4, 8, Q, P, P, 1 << 20, None)),\n"
           "    # ttemb_bag_max_backward_n(d_output, argmax, offsets, nnz, nnz_dev, B, D, d_rows, stream)\n"
           "    (L.ttemb_bag_max_backward_n, (P, P, P, -1, C, 4, 8, P, None)),\n"
           "    (L.ttemb_bag_max_backward_n, (P, P, P, 2 ** 31, C, 4, 8, P, None)),\n"
           "    (L.ttemb_bag_max_backward_n, (P, None, P, 8, C, 4, 8, P, None)),\n"
           "    (L.ttemb_bag_max_backward_n, (P, P, P, 8, C, 4, 8, Q, None)),\n"
           "    # ttemb_pad_weights_n(indices, offsets, weights, nnz, nnz_dev, B, pad, mean, weights_out, stream)\n"
           "    (L.ttemb_pad_weights_n, (P, P, None, -1, C, 4, 0, 0, P, None)),\n"
           "    (L.ttemb_pad_weights_n, (P, P, None, 8, C, -4, 0, 0, P, None)),\n"
           "    (L.ttemb_pad_weights_n, (None, P, None, 8, C, 4, 0, 0, P, None)),\n"
           "    (L.ttemb_pad_weights_n, (P, P, None, 8, C, 4, 0, 1, None, None)),\n"
           "]\n"
           "for k, (f, args) in enumerate(bad):\n"
           "    assert f(*args) == -1, (k, f.__name__)   # TTEMB_E_BADARG\n"
           "# a workspace that is too small is its own code, as in the namesakes\n"
           "assert L.ttemb_bag_reduce_n(P, P, P, 8, C, 4, 8, P, P, 16, None) == -2\n"
           "assert L.ttemb_bag_max_n(P, None, 0, P, 8, C, 4, 8, P, P, P, 16, None) == -2\n")


def test_capture_bags_raises_its_argument_errors_without_a_device():
    _child("from FBTT.tt_embeddings_ops import TTEmbeddingBag, TableBatchedTTEmbeddingBag, CapturedBags\n"
           "import pytest\n"
           "args = (1000, 16, [4, 4], [10, 10, 10], [2, 2, 4])\n"
           "e = TTEmbeddingBag(*args, use_cache=False, sparse=True)\n"
           "for mode in ('mean', 'max'):\n"
           "    with pytest.raises(ValueError, match='weighted bags are only supported with mode=.sum.'):\n"
           "        e.capture_bags(16, 4, mode=mode, weighted=True)\n"
           "with pytest.raises(ValueError, match='weighted bags are only supported'):\n"
           "    TTEmbeddingBag(*args, use_cache=False, sparse=True, mode='mean').capture_bags(16, 4, weighted=True)\n"
           "with pytest.raises(ValueError, match='mode must be'):\n"
           "    e.capture_bags(16, 4, mode='prod')\n"
           "for nnz, B, fanout in ((16, 4, 3), (17, 4, 4), (16, 4, 0), (16, 4, -4)):\n"
           "    with pytest.raises(ValueError, match='fanout'):\n"
           "        e.capture_bags(nnz, B, fanout=fanout)\n"
           "for nnz, B in ((0, 4), (16, 0), (-1, 4), (2 ** 31, 4)):\n"
           "    with pytest.raises(ValueError, match='positive'):\n"
           "        e.capture_bags(nnz, B, variable=True)\n"
           "with pytest.raises(ValueError, match='sparse=True'):\n"
           "    TTEmbeddingBag(*args, use_cache=False, sparse=False).capture_bags(16, 4, mode='mean')\n"
           "with pytest.raises(ValueError, match='single table'):\n"
           "    TableBatchedTTEmbeddingBag(2, *args, sparse=True).capture_bags(16, 4)\n"
           "with pytest.raises(TypeError):\n"
           "    e.capture_bags(16, 4, 'mean')   # keyword-only, as the issue's signature\n"
           "# capture() is what it was: it still refuses what capture_bags() serves\n"
           "with pytest.raises(AssertionError, match='mode'):\n"
           "    TTEmbeddingBag(*args, use_cache=False, sparse=True, mode='mean').capture(16, 4)\n")


def test_pooling_and_staging_kernels_do_not_spill():
    lib = os.path.join(PKG, "lib", "libttemb_hip.so")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kres.py"), lib, "bag_", "pad_weights", "stage_bags",
                        "--fail-on-scratch"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for k in ("stage_bags_kernel", "bag_partial_kernel", "bag_reduce_kernel", "bag_reduce_backward_kernel",
              "bag_max_partial_kernel", "bag_max_kernel", "bag_max_backward_kernel", "pad_weights_kernel"):
        assert k in r.stdout, f"{k} is not in the library"
