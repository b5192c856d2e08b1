"""padding_idx and 2-D bags, host side (no GPU): the constructor's checks, the new symbols, the argument checks that run
before any launch, capture()'s refusal, and no spills in the new kernels.  Queries run in a child process with no device
visible, like test_weighted_host.py."""
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


def test_padding_idx_is_checked_and_normalised_at_construction():
    _child("from FBTT.tt_embeddings_ops import TTEmbeddingBag, TableBatchedTTEmbeddingBag\n"
           "import pytest\n"
           "args = (1000, 16, [4, 4], [10, 10, 10], [2, 2, 4])\n"
           "for bad in (1000, -1001, 5000):\n"
           "    with pytest.raises(ValueError):\n"
           "        TTEmbeddingBag(*args, use_cache=False, padding_idx=bad)\n"
           "    with pytest.raises(ValueError):\n"
           "        TableBatchedTTEmbeddingBag(2, *args, padding_idx=bad)\n"
           "for given, stored in ((None, None), (0, 0), (999, 999), (-1, 999), (-1000, 0), (7, 7)):\n"
           "    e = TTEmbeddingBag(*args, use_cache=False, padding_idx=given)\n"
           "    assert e.padding_idx == stored, (given, e.padding_idx)\n"
           "    assert TableBatchedTTEmbeddingBag(3, *args, padding_idx=given).padding_idx == stored\n"
           "plain = TTEmbeddingBag(*args, use_cache=False)\n"
           "padded = TTEmbeddingBag(*args, use_cache=False, padding_idx=-3)\n"
           "assert set(padded.state_dict()) == set(plain.state_dict())\n"
           "padded.load_state_dict(plain.state_dict())\n"
           "assert padded.padding_idx == 997\n"
           "with pytest.raises(TypeError):\n"
           "    TTEmbeddingBag(*args, None, 'sgd', 0.1, 1e-10, True, False, 0, 0, 'uniform', False, 1000, None, 'sum', 3)\n")


def test_padding_symbols_are_exported():
    _child("import ttemb_native as n\n"
           "names = ('ttemb_drop_padding_workspace_bytes', 'ttemb_drop_padding', 'ttemb_pad_weights')\n"
           "assert all(s in n.EXPORTED_SYMBOLS for s in names)\n"
           "[getattr(n.LIB, s) for s in names]\n"
           "assert n.LIB.ttemb_abi_version() == 4\n"
           "f = n.LIB.ttemb_drop_padding_workspace_bytes\n"
           "assert f(0, 0) >= 40960 and f(409600, 40960) >= f(256, 1) >= 40960\n"
           "assert f(-1, 1) == -1 and f(1, -1) == -1   # TTEMB_E_BADARG\n")


def test_arguments_are_checked_before_any_launch():
    _child("from FBTT.tt_embeddings_ops import TTEmbeddingBag\n"
           "import pytest, torch\n"
           "for pad in (None, 5):\n"
           "    e = TTEmbeddingBag(1000, 16, [4, 4], [10, 10, 10], [2, 2, 4], use_cache=False, padding_idx=pad)\n"
           "    idx = torch.zeros(12, dtype=torch.int64)\n"
           "    with pytest.raises(ValueError):\n"
           "        e(idx)   # 1-D without offsets\n"
           "    with pytest.raises(ValueError):\n"
           "        e(idx.view(3, 4), torch.arange(0, 13, 4))   # 2-D with offsets\n"
           "    with pytest.raises(ValueError):\n"
           "        e(idx.view(3, 4), per_sample_weights=torch.ones(12))\n"
           "    with pytest.raises(RuntimeError):\n"
           "        e(idx.view(3, 4))   # a valid call on CPU tensors: no CPU fallback\n")


def test_capture_refuses_padding():
    _child("from FBTT.tt_embeddings_ops import TTEmbeddingBag\n"
           "import pytest\n"
           "e = TTEmbeddingBag(1000, 16, [4, 4], [10, 10, 10], [2, 2, 4], use_cache=False, sparse=True, padding_idx=0)\n"
           "with pytest.raises(AssertionError, match='padding_idx'):\n"
           "    e.capture(16, 4)\n")


def test_padding_kernels_do_not_spill():
    lib = os.path.join(PKG, "lib", "libttemb_hip.so")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kres.py"), lib, "pad_", "partition_scatter",
                        "--fail-on-scratch"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for k in ("pad_count_kernel", "pad_scatter_kernel", "pad_weights_kernel", "partition_scatter_kernel"):
        assert k in r.stdout, f"{k} is not in the library"
