"""Captured padded bags on the partition route, host side (no GPU): the symbols of ``include/ttemb_pads.h``, the argument
checks of ``ttemb_compact_bags`` / ``ttemb_expand_kept`` that run before any launch, the two ``pad_route`` errors of
``capture_bags`` and no spills in the new kernels.  Queries run in a child process with no device visible, like
test_capture_bags_host.py."""
import os
import re
import subprocess
import sys


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "falcon-ttdforgnns_amd")

PADS_SYMBOLS = ("ttemb_compact_bags_workspace_bytes", "ttemb_compact_bags", "ttemb_expand_kept")


def _child(code):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", "import sys; sys.path[:0] = [sys.argv[1]]\n" + code, PKG], env=env,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def test_the_pads_symbols_are_exported_and_bound():
    _child("import ctypes, ttemb_native as n\n"
           f"names = {PADS_SYMBOLS!r}\n"
           "assert tuple(n.PADS_SYMBOLS) == names\n"
           "for s in names:\n"
           "    f = getattr(n.LIB, s)\n"
           "    assert f.argtypes is not None\n"
           "    assert f.restype is (ctypes.c_int64 if s.endswith('_workspace_bytes') else ctypes.c_int), s\n"
           "assert n.LIB.ttemb_abi_version() == 4 and n.ABI_VERSION == 4   # additive symbols: the version stays\n"
           "assert callable(n.compact_bags) and callable(n.expand_kept)\n"
           "# the tile counts behind the 40 KB header: one int32 per 256 positions, as ttemb_drop_padding\n"
           "assert n.compact_bags_workspace_bytes(4096) == n.drop_padding_workspace_bytes(4096, 7) == 40960 + 256\n"
           "assert n.LIB.ttemb_compact_bags_workspace_bytes(-1) == -1\n")


def test_the_pads_header_declares_exactly_the_new_symbols():
    """include/ttemb_pads.h declares the three symbols and nothing else, and ttemb.h includes it next to ttemb_bags.h."""
    with open(os.path.join(ROOT, "include", "ttemb_pads.h")) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    assert sorted(re.findall(r"\b(?:int|int64_t)\s+(ttemb_\w+)\s*\(", text)) == sorted(PADS_SYMBOLS)
    with open(os.path.join(ROOT, "include", "ttemb.h")) as f:
        assert re.search(r'#include "ttemb_bags.h"\s*\n#include "ttemb_pads.h"', f.read())


def test_compact_bags_and_expand_kept_check_their_arguments_before_any_launch():
    """Pointers that would fault when read (0x10 ...): the codes come back, so nothing was launched or read."""
    _child("import ttemb_native as n\n"
           "L = n.LIB\n"
           "P, O, W, C, BIG = 0x10, 0x20, 0x30, 0x40, 1 << 20   # (never dereferenced)\n"
           "# ttemb_compact_bags(indices, offsets, weights, nnz, nnz_dev, B, pad, indices_out, offsets_out, weights_out, map_out,\n"
           "#                    kept_dev, workspace, workspace_bytes, stream)\n"
           "bad = {\n"
           "    'negative nnz':        (P, P, None, -1, C, 4, 5, O, O, None, None, C, W, BIG, None),\n"
           "    'negative B':          (P, P, None, 8, C, -4, 5, O, O, None, None, C, W, BIG, None),\n"
           "    'nnz past int32':      (P, P, None, 2 ** 31, C, 4, 5, O, O, None, None, C, W, 1 << 40, None),\n"
           "    'null indices':        (None, P, None, 8, C, 4, 5, O, O, None, None, C, W, BIG, None),\n"
           "    'null offsets':        (P, None, None, 8, C, 4, 5, O, O, None, None, C, W, BIG, None),\n"
           "    'null indices_out':    (P, P, None, 8, C, 4, 5, None, O, None, None, C, W, BIG, None),\n"
           "    'null offsets_out':    (P, P, None, 8, C, 4, 5, O, None, None, None, C, W, BIG, None),\n"
           "    'null kept_dev':       (P, P, None, 8, C, 4, 5, O, O, None, None, None, W, BIG, None),\n"
           "    'null workspace':      (P, P, None, 8, C, 4, 5, O, O, None, None, C, None, BIG, None),\n"
           "    'weights only':        (P, P, W, 8, C, 4, 5, O, O, None, None, C, W, BIG, None),\n"
           "    'weights_out only':    (P, P, None, 8, C, 4, 5, O, O, W, None, C, W, BIG, None),\n"
           "    'in place':            (P, P, None, 8, C, 4, 5, P, O, None, None, C, W, BIG, None),\n"
           "}\n"
           "for what, args in bad.items():\n"
           "    assert L.ttemb_compact_bags(*args) == -1, what   # TTEMB_E_BADARG\n"
           "    assert b'ttemb_compact_bags' in L.ttemb_last_error(), what\n"
           "# a workspace that is too small is its own code: smaller than the header, and no room behind it for the tile counts\n"
           "for nbytes in (16, 40960, n.compact_bags_workspace_bytes(8) - 1):\n"
           "    assert L.ttemb_compact_bags(P, P, None, 8, C, 4, 5, O, O, None, None, C, W, nbytes, None) == -2, nbytes\n"
           "# ttemb_expand_kept(src, map, nnz, nnz_dev, out, stream)\n"
           "bad = {\n"
           "    'negative nnz':   (P, O, -1, C, W, None),\n"
           "    'nnz past int32': (P, O, 2 ** 31, C, W, None),\n"
           "    'null src':       (None, O, 8, C, W, None),\n"
           "    'null map':       (P, None, 8, C, W, None),\n"
           "    'null out':       (P, O, 8, C, None, None),\n"
           "    'in place':       (P, O, 8, C, P, None),\n"
           "}\n"
           "for what, args in bad.items():\n"
           "    assert L.ttemb_expand_kept(*args) == -1, what\n"
           "    assert b'ttemb_expand_kept' in L.ttemb_last_error(), what\n")


def test_capture_bags_raises_the_pad_route_errors_without_a_device():
    _child("from FBTT.tt_embeddings_ops import TTEmbeddingBag, CapturedBags\n"
           "import inspect, pytest\n"
           "args = (1000, 16, [4, 4], [10, 10, 10], [2, 2, 4])\n"
           "plain = TTEmbeddingBag(*args, use_cache=False, sparse=True)\n"
           "padded = TTEmbeddingBag(*args, use_cache=False, sparse=True, padding_idx=5)\n"
           "with pytest.raises(ValueError, match='padding_idx'):\n"
           "    plain.capture_bags(16, 4, mode='mean', pad_route='partition')\n"
           "for m in (plain, padded):\n"
           "    with pytest.raises(ValueError, match='pad_route must be'):\n"
           "        m.capture_bags(16, 4, mode='mean', pad_route='compact')\n"
           "with pytest.raises(TypeError):\n"
           "    padded.capture_bags(16, 4, 'mean', False, None, True, 'partition')   # keyword-only\n"
           "# check_arguments: a trailing parameter with default None -- the six-argument call of today still works\n"
           "sig = inspect.signature(CapturedBags.check_arguments)\n"
           "assert list(sig.parameters)[-1] == 'pad_route' and sig.parameters['pad_route'].default is None\n"
           "assert CapturedBags.check_arguments(padded, 16, 4, 'mean', False, None) == 'mean'\n"
           "assert CapturedBags.check_arguments(padded, 16, 4, None, False, None, 'partition') == 'sum'\n"
           "assert CapturedBags.check_arguments(padded, 16, 4, None, False, None, 'masked') == 'sum'\n"
           "with pytest.raises(ValueError, match='padding_idx'):\n"
           "    CapturedBags.check_arguments(plain, 16, 4, None, False, None, 'partition')\n")


def test_compaction_kernels_do_not_spill():
    lib = os.path.join(PKG, "lib", "libttemb_hip.so")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kres.py"), lib, "compact_", "expand_kept", "pad_",
                        "--fail-on-scratch"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for k in ("compact_count_kernel", "compact_scatter_kernel", "expand_kept_kernel", "pad_count_kernel", "pad_scatter_kernel"):
        assert k in r.stdout, f"{k} is not in the library"
