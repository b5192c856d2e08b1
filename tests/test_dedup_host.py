"""The dedup route, host side (no GPU): the symbols of ``include/ttemb_unique.h``, the parent's declarations unchanged, the
argument checks that run before any launch, the refusals a module raises without a device, the depth helper of
tests/dedup_bound.py against a numpy emulation of the segment sum, and no spills in the new kernels.  Queries run in a child
process with no device visible, like test_capture_pads_host.py."""
import os
import re
import subprocess
import sys

import numpy as np

import dedup_bound as db
import fp32_bound as fb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "falcon-ttdforgnns_amd")

UNIQUE_SYMBOLS = ("ttemb_unique_ids_workspace_bytes", "ttemb_unique_ids", "ttemb_bag_reduce_mapped",
                  "ttemb_bag_reduce_mapped_backward")


def _child(code):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", "import sys; sys.path[:0] = [sys.argv[1]]\n" + code, PKG], env=env,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def _declarations(text):
    """{function name: its declaration with comments dropped and white space squeezed} of a C header."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    out = {}
    for piece in text.split(";"):
        m = re.search(r"((?:const\s+char\s*\*|int64_t|int)\s+(ttemb_\w+)\s*\([^{}]*\))\s*$", piece, flags=re.S)
        if m:
            out[m.group(2)] = re.sub(r"\s+", " ", m.group(1)).strip()
    return out


def test_the_unique_symbols_are_exported_and_bound():
    _child("import ctypes, ttemb_native as n\n"
           f"names = {UNIQUE_SYMBOLS!r}\n"
           "assert tuple(n.UNIQUE_SYMBOLS) == names\n"
           "for s in names:\n"
           "    f = getattr(n.LIB, s)\n"
           "    assert f.argtypes is not None\n"
           "    assert f.restype is (ctypes.c_int64 if s.endswith('_workspace_bytes') else ctypes.c_int), s\n"
           "assert len(n.LIB.ttemb_unique_ids.argtypes) == 11 and len(n.LIB.ttemb_bag_reduce_mapped.argtypes) == 12\n"
           "assert len(n.LIB.ttemb_bag_reduce_mapped_backward.argtypes) == 17\n"
           "assert n.LIB.ttemb_abi_version() == 4 and n.ABI_VERSION == 4   # additive symbols: the version stays\n"
           "assert callable(n.unique_ids) and callable(n.bag_reduce_mapped) and callable(n.bag_reduce_mapped_backward)\n")


def test_the_unique_header_declares_exactly_the_new_symbols_and_the_parent_abi_is_unchanged():
    with open(os.path.join(ROOT, "include", "ttemb_unique.h")) as f:
        assert sorted(_declarations(f.read())) == sorted(UNIQUE_SYMBOLS)
    with open(os.path.join(ROOT, "include", "ttemb.h")) as f:
        now_text = f.read()
    assert re.search(r'#include "ttemb_pads.h"\s*\n#include "ttemb_unique.h"', now_text)
    assert "#define TTEMB_ABI_VERSION 4" in now_text
    with open(os.path.join(ROOT, "tests", "golden", "ttemb_abi4_parent.h.txt")) as f:
        parent = _declarations(f.read())
    now = _declarations(now_text)
    assert len(parent) >= 55   # (the parser sees them)
    for name, decl in parent.items():
        assert now.get(name) == decl, name
    assert not set(now) & set(UNIQUE_SYMBOLS)   # ttemb.h's own set is pinned: the new ones live in their own header


def test_the_new_entry_points_check_their_arguments_before_any_launch():
    """Pointers that would fault when read (0x10 ...): the codes come back, so nothing was launched or read."""
    _child("import ttemb_native as n\n"
           "L = n.LIB\n"
           "P, O, W, C, BIG = 0x10, 0x20, 0x30, 0x40, 1 << 20   # (never dereferenced)\n"
           "# ttemb_unique_ids(indices, nnz, rows, unique_out, inverse_out, perm_out, seg_out, count_dev, ws, ws_bytes, stream)\n"
           "bad = {\n"
           "    'negative nnz':     (P, -1, 100, O, O, O, O, C, W, BIG, None),\n"
           "    'nnz past int32':   (P, 2 ** 31, 100, O, O, O, O, C, W, 1 << 40, None),\n"
           "    'no rows':          (P, 8, 0, O, O, O, O, C, W, BIG, None),\n"
           "    'null indices':     (None, 8, 100, O, O, O, O, C, W, BIG, None),\n"
           "    'null unique_out':  (P, 8, 100, None, O, O, O, C, W, BIG, None),\n"
           "    'null inverse_out': (P, 8, 100, O, None, O, O, C, W, BIG, None),\n"
           "    'null perm_out':    (P, 8, 100, O, O, None, O, C, W, BIG, None),\n"
           "    'null seg_out':     (P, 8, 100, O, O, O, None, C, W, BIG, None),\n"
           "    'null seg_out, no ids': (None, 0, 100, None, None, None, None, C, W, BIG, None),\n"
           "    'null count_dev':   (P, 8, 100, O, O, O, O, None, W, BIG, None),\n"
           "    'null workspace':   (P, 8, 100, O, O, O, O, C, None, BIG, None),\n"
           "}\n"
           "for what, args in bad.items():\n"
           "    assert L.ttemb_unique_ids(*args) == -1, what   # TTEMB_E_BADARG\n"
           "    assert b'ttemb_unique_ids' in L.ttemb_last_error(), what\n"
           "assert L.ttemb_unique_ids(P, 8, 100, O, O, O, O, C, W, 16, None) == -2   # smaller than the header\n"
           "assert L.ttemb_unique_ids_workspace_bytes(-1, 100) == -1 and L.ttemb_unique_ids_workspace_bytes(8, 0) == -1\n"
           "assert L.ttemb_unique_ids_workspace_bytes(2 ** 31, 100) == -1\n"
           "assert L.ttemb_unique_ids_workspace_bytes(0, 100) == 40960 + 256   # no ids: the header and one tile count\n"
           "# ttemb_bag_reduce_mapped(rows, cap, map, weights, offsets, nnz, B, D, output, ws, ws_bytes, stream)\n"
           "bad = {\n"
           "    'negative nnz':   (P, 8, O, None, P, -1, 4, 16, O, W, BIG, None),\n"
           "    'D not 4k':       (P, 8, O, None, P, 8, 4, 18, O, W, BIG, None),\n"
           "    'nnz past int32': (P, 8, O, None, P, 2 ** 31, 4, 16, O, W, 1 << 50, None),\n"
           "    'null rows':      (None, 8, O, None, P, 8, 4, 16, O, W, BIG, None),\n"
           "    'null map':       (P, 8, None, None, P, 8, 4, 16, O, W, BIG, None),\n"
           "    'no capacity':    (P, 0, O, None, P, 8, 4, 16, O, W, BIG, None),\n"
           "    'null offsets':   (P, 8, O, None, None, 8, 4, 16, O, W, BIG, None),\n"
           "    'null output':    (P, 8, O, None, P, 8, 4, 16, None, W, BIG, None),\n"
           "    'misaligned':     (P + 4, 8, O, None, P, 8, 4, 16, O, W, BIG, None),\n"
           "}\n"
           "for what, args in bad.items():\n"
           "    assert L.ttemb_bag_reduce_mapped(*args) == -1, what\n"
           "    assert b'ttemb_bag_reduce_mapped' in L.ttemb_last_error(), what\n"
           "assert L.ttemb_bag_reduce_mapped(P, 8, O, None, P, 8, 4, 16, O, W, 40960, None) == -2\n"
           "# ttemb_bag_reduce_mapped_backward(d_output, weights, rows, cap, map, perm, seg, count_dev, offsets, nnz, B, D,\n"
           "#                                  d_rows, d_weights, ws, ws_bytes, stream)\n"
           "bad = {\n"
           "    'negative B':      (P, None, None, 8, O, O, O, C, P, 8, -4, 16, O, None, W, BIG, None),\n"
           "    'null d_output':   (None, None, None, 8, O, O, O, C, P, 8, 4, 16, O, None, W, BIG, None),\n"
           "    'null map':        (P, None, None, 8, None, O, O, C, P, 8, 4, 16, O, None, W, BIG, None),\n"
           "    'null perm':       (P, None, None, 8, O, None, O, C, P, 8, 4, 16, O, None, W, BIG, None),\n"
           "    'null seg':        (P, None, None, 8, O, O, None, C, P, 8, 4, 16, O, None, W, BIG, None),\n"
           "    'null count_dev':  (P, None, None, 8, O, O, O, None, P, 8, 4, 16, O, None, W, BIG, None),\n"
           "    'null d_rows':     (P, None, None, 8, O, O, O, C, P, 8, 4, 16, None, None, W, BIG, None),\n"
           "    'd_w without rows': (P, None, None, 8, O, O, O, C, P, 8, 4, 16, O, W, W, BIG, None),\n"
           "    'nnz past int32':  (P, None, None, 8, O, O, O, C, P, 2 ** 31, 4, 16, O, None, W, 1 << 50, None),\n"
           "}\n"
           "for what, args in bad.items():\n"
           "    assert L.ttemb_bag_reduce_mapped_backward(*args) == -1, what\n"
           "    assert b'ttemb_bag_reduce_mapped_backward' in L.ttemb_last_error(), what\n"
           "assert L.ttemb_bag_reduce_mapped_backward(P, None, None, 8, O, O, O, C, P, 8, 4, 16, O, None, W, 40960, None) == -2\n")


def test_the_refusals_a_module_raises_without_a_device():
    _child("import pytest, torch\n"
           "from FBTT.tt_embeddings_ops import TTEmbeddingBag, TableBatchedTTEmbeddingBag\n"
           "from Efficient_TT.efficient_tt import Eff_TTEmbedding\n"
           "args = (1000, 16, [4, 4], [10, 10, 10], [2, 2, 4])\n"
           "with pytest.raises(ValueError, match='dedup=True with use_cache=True'):\n"
           "    TTEmbeddingBag(*args, dedup=True)   # (TTEmbeddingBag's use_cache defaults to True)\n"
           "with pytest.raises(ValueError, match='dedup=True with use_cache=True'):\n"
           "    TableBatchedTTEmbeddingBag(1, *args, use_cache=True, dedup=True)\n"
           "import inspect\n"
           "for cls in (TTEmbeddingBag, TableBatchedTTEmbeddingBag):\n"
           "    for fn in (cls.__init__, cls.forward):\n"
           "        assert inspect.signature(fn).parameters['dedup'].kind is inspect.Parameter.KEYWORD_ONLY\n"
           "    assert inspect.signature(cls.forward).parameters['dedup'].default is None\n"
           "on = TTEmbeddingBag(*args, use_cache=False, dedup=True)\n"
           "off = TTEmbeddingBag(*args, use_cache=False)\n"
           "assert on.dedup is True and off.dedup is False and on._last_unique is None\n"
           "assert 'dedup' not in on.state_dict() and list(on.state_dict()) == list(off.state_dict())\n"
           "with pytest.raises(ValueError, match=r'capture\\(\\) on a dedup=True module'):\n"
           "    on.capture(16, 16)\n"
           "with pytest.raises(ValueError, match=r'capture_bags\\(\\) on a dedup=True module'):\n"
           "    on.capture_bags(16, 4, mode='mean')\n"
           "ids, offs = torch.zeros(4, dtype=torch.int64), torch.arange(5)\n"
           "for m in (on, off):   # refused before the call looks at a device\n"
           "    with pytest.raises(ValueError, match=\"mode='max'\"):\n"
           "        m(ids, offs, mode='max', dedup=True)\n"
           "exact = TTEmbeddingBag(*args, use_cache=False, deterministic=True)\n"
           "with pytest.raises(ValueError, match='exact mode'):\n"
           "    exact(ids, offs, dedup=True)\n"
           "cached = TTEmbeddingBag(*args, use_cache=True, cache_size=10, hashtbl_size=40)\n"
           "cached.warmup = False   # (what cache_populate() leaves)\n"
           "with pytest.raises(ValueError, match='live row cache'):\n"
           "    cached(ids, offs, dedup=True)\n"
           "big = torch.zeros(1, dtype=torch.int64).expand((1 << 24) + 1)   # (one word behind it)\n"
           "with pytest.raises(ValueError, match='row window'):\n"
           "    off(big, None, dedup=True)\n"
           "wide = TTEmbeddingBag(8000, 512, [2, 2], [20, 20, 20], [8, 8, 8], use_cache=False)\n"
           "with pytest.raises(ValueError, match='row window'):   # 2 GiB of rows before 2^24 of them\n"
           "    wide(torch.zeros(1, dtype=torch.int64).expand((1 << 20) + 1), None, dedup=True)\n"
           "assert Eff_TTEmbedding(*args, dedup=True).dedup and not Eff_TTEmbedding(*args).dedup\n")


def _segment_sum32(terms, w):
    """The kernels' segment sum in numpy float32: the first term a product, then one fma per term; a segment of more than
    512 positions in chunks of 512 of the sorted list (here the segment starts at a chunk edge), partials added in order."""
    def run(t, wt):
        acc = np.float32(wt[0]) * np.float32(t[0])
        for k in range(1, len(t)):
            acc = np.float32(np.float64(wt[k]) * np.float64(t[k]) + np.float64(acc))   # (the product is exact in float64)
        return acc
    if len(terms) <= 512:
        return run(terms, w)
    acc = None
    for s in range(0, len(terms), 512):
        part = run(terms[s:s + 512], w[s:s + 512])
        acc = part if acc is None else np.float32(acc + part)
    return acc


def test_the_segment_depth_covers_a_correct_fp32_segment_sum_and_rejects_a_dropped_term():
    rng = np.random.default_rng(5)
    for m in (1, 2, 511, 512, 513, 1639, 5000):
        terms = (fb.signed_magnitudes(rng, m) * 10.0 ** rng.uniform(-3, 0, size=m)).astype(np.float32)
        w = fb.sample_weights(rng, m)
        exact = float(np.sum(terms.astype(np.float64) * w.astype(np.float64)))
        mag = float(np.sum(np.abs(terms.astype(np.float64) * w.astype(np.float64))))
        got = _segment_sum32(terms, w)
        fb.assert_fp32_grade(np.array([got]), np.array([exact]), np.array([mag]), db.segment_depth(m), f"segment of {m}")
        if m > 2:   # the same sum without its largest term is outside the bound (where that term is larger than the bound)
            prod = np.abs(terms.astype(np.float64) * w.astype(np.float64))
            k = int(np.argmax(prod))
            less = _segment_sum32(np.delete(terms, k), np.delete(w, k))
            if prod[k] > 2 * fb.gamma(db.segment_depth(m)) * mag:
                try:
                    fb.assert_fp32_grade(np.array([less]), np.array([exact]), np.array([mag]), db.segment_depth(m), "dropped")
                except AssertionError:
                    continue
                raise AssertionError(f"a segment sum of {m} terms without one of them passed the bound")
    assert list(db.segment_depth(np.array([1, 512, 1639]))) == [3, 515, 1644]


def test_touch_counts_and_the_row_depth():
    p, q, R = [2, 3, 4], [4, 5, 5], [1, 16, 16, 1]
    ids = np.array([0, 0, 0, 5, 5, 23, 12], dtype=np.int64)   # digits: 0 -> (0,0,0), 5 -> (0,1,1), 23 -> (1,2,3), 12 -> (1,0,0)
    (n0, m0), (n1, m1), (n2, m2) = db.touch_counts(ids, p)
    assert list(n0) == [2, 2] and list(m0) == [3, 1]
    assert list(n1) == [2, 1, 1] and list(m1) == [3, 2, 1]
    assert list(n2) == [2, 1, 0, 1] and list(m2) == [3, 2, 0, 1]
    d = db.dedup_grad_depth("grouped", q, R, 1, n1, m1)
    plain = fb.grad_depth("grouped", q, R, 1, n1, scaled=True)
    assert d.shape == (3, 1) and list((d - plain)[:, 0]) == [5, 4, 3]   # m + m // 512 + 2
    # every position its own id: the multiplicity is 1 and the distinct count is the plain count
    ids = np.arange(24, dtype=np.int64)
    for (n, m), pt in zip(db.touch_counts(ids, p), p):
        assert list(n) == [24 // pt] * pt and list(m) == [1] * pt


def test_the_new_kernels_do_not_spill():
    lib = os.path.join(PKG, "lib", "libttemb_hip.so")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kres.py"), lib, "mapped", "unique_", "--fail-on-scratch"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for k in ("unique_count_kernel", "unique_scatter_kernel", "bag_partial_mapped_kernel", "bag_reduce_mapped_kernel",
              "seg_partial_mapped_kernel", "seg_reduce_mapped_kernel", "mapped_weight_grad_kernel"):
        assert k in r.stdout, f"{k} is not in the library"
