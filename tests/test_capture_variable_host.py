"""Captured lookups of variable size, host side (no GPU): the new symbol and its binding, the unchanged ABI version, the
``variable`` keyword of ``capture``, and no spill in the staging kernel.  Queries run in a child process with no device
visible, like test_max_host.py."""
import os
import subprocess
import sys


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "falcon-ttdforgnns_amd")


def _child(code):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", "import sys; sys.path[:0] = [sys.argv[1]]\n" + code, PKG], env=env,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def test_stage_call_is_exported_and_bound():
    _child("import ttemb_native as n\n"
           "assert 'ttemb_stage_call' in n.EXPORTED_SYMBOLS\n"
           "f = n.LIB.ttemb_stage_call\n"
           "assert f.argtypes is not None and len(f.argtypes) == 12\n"
           "assert callable(n.stage_call)\n")


def test_abi_version_is_still_4():
    _child("import ttemb_native as n\n"
           "assert n.LIB.ttemb_abi_version() == 4 and n.ABI_VERSION == 4\n"
           "n.LIB.ttemb_stage_call   # (the library this version number belongs to has the new symbol)\n")


def test_capture_has_a_keyword_only_variable_parameter():
    _child("import inspect\n"
           "from FBTT.tt_embeddings_ops import TTEmbeddingBag, TableBatchedTTEmbeddingBag, CapturedLookup\n"
           "for cls in (TTEmbeddingBag, TableBatchedTTEmbeddingBag):\n"
           "    p = inspect.signature(cls.capture).parameters['variable']\n"
           "    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False\n"
           "assert inspect.signature(CapturedLookup.__init__).parameters['variable'].default is False\n")


def test_lean_calls_take_an_optional_device_count():
    _child("import inspect\n"
           "import ttemb_native as n\n"
           "for f in (n.LeanCalls.forward, n.LeanCalls.backward):\n"
           "    assert inspect.signature(f).parameters['nnz_dev'].default is None\n")


def test_stage_call_checks_its_sizes_before_it_touches_a_pointer():
    # no device: a call that got past the size checks would launch; these return TTEMB_E_BADARG (-1) first
    _child("import ttemb_native as n\n"
           "f = n.LIB.ttemb_stage_call\n"
           "buf = 4096   # (never dereferenced)\n"
           "for args in ((buf, 0, 5, None, 0, 5, buf, 4, buf, 8, buf, None),     # n_live > nnz_cap\n"
           "             (buf, 0, 4, buf, 0, 9, buf, 4, buf, 8, buf, None),      # B_live > B_cap\n"
           "             (buf, 0, -1, None, 0, -1, buf, 4, buf, 8, buf, None),   # negative sizes\n"
           "             (buf, 0, 4, buf, 0, -2, buf, 4, buf, 8, buf, None),\n"
           "             (buf, 0, 3, None, 0, 2, buf, 4, buf, 8, buf, None),     # no offsets: one bag per id\n"
           "             (buf, 0, 2, None, 0, 2, buf, 4, None, 8, buf, None),    # null outputs\n"
           "             (buf, 0, 2, None, 0, 2, buf, 4, buf, 8, None, None)):\n"
           "    assert f(*args) == -1, args\n"
           "    assert b'ttemb_stage_call' in n.LIB.ttemb_last_error()\n")


def test_stage_call_kernel_does_not_spill():
    lib = os.path.join(PKG, "lib", "libttemb_hip.so")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kres.py"), lib, "stage_call", "--fail-on-scratch"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "stage_call_kernel" in r.stdout, "stage_call_kernel is not in the library"
