"""Device-resident learning rate, the part that needs no GPU: the additive C ABI (new symbols, version 4, every earlier
declaration unchanged against the parent's header kept as text in ``tests/golden/ttemb_abi4_parent.h.txt``), the
``capturable`` keyword's refusal, and ``state_dict()`` keys that do not depend on it."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ttemb_backward_step", "ttemb_backward_step_window", "ttemb_backward_step_exact", "ttemb_flat_step")
P, Q, R = [8, 10, 10], [4, 5, 5], [16, 16]


@pytest.fixture(scope="module")
def nat():
    import ttemb_native
    return ttemb_native


@pytest.fixture(scope="module")
def ops():
    import FBTT.tt_embeddings_ops as m
    return m


def _declarations(text):
    """{function name: its declaration with comments dropped and white space squeezed} of a C header."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    out = {}
    for piece in text.split(";"):
        m = re.search(r"((?:const\s+char\s*\*|int64_t|int)\s+(ttemb_\w+)\s*\([^{}]*\))\s*$", piece, flags=re.S)
        if m:
            out[m.group(2)] = re.sub(r"\s+", " ", m.group(1)).strip()
    return out


def _block(text, start, end):
    i = text.index(start)
    return re.sub(r"\s+", " ", text[i:text.index(end, i) + len(end)])


def test_library_exports_the_new_symbols_and_stays_abi_4(nat):
    for name in NEW_SYMBOLS:
        assert name in nat.EXPORTED_SYMBOLS
        assert getattr(nat.LIB, name) is not None
    assert nat.LIB.ttemb_abi_version() == 4 and nat.ABI_VERSION == 4


def test_every_earlier_entry_point_keeps_its_declaration():
    with open(os.path.join(ROOT, "tests", "golden", "ttemb_abi4_parent.h.txt")) as f:
        parent_text = f.read()
    with open(os.path.join(ROOT, "include", "ttemb.h")) as f:
        now_text = f.read()
    parent, now = _declarations(parent_text), _declarations(now_text)
    assert len(parent) >= 55 and "ttemb_backward_adagrad" in parent and "ttemb_adam_step" in parent   # (the parser sees them)
    for name, decl in parent.items():
        assert now.get(name) == decl, name
    assert sorted(set(now) - set(parent)) == sorted(NEW_SYMBOLS)
    assert "#define TTEMB_ABI_VERSION 4" in now_text
    for start, end in (("typedef struct ttemb_adam {", "} ttemb_adam_t;"), ("typedef struct ttemb_shape {", "} ttemb_shape_t;")):
        assert _block(now_text, start, end) == _block(parent_text, start, end)


def test_step_descriptor_mirrors_the_header(nat):
    """``ttemb_step_t``: seven fields in the header's order; pointers are 8 bytes, so the struct is 56 bytes."""
    import ctypes
    assert [f[0] for f in nat.StepDesc._fields_] == ["kind", "lr_dev", "eps", "state", "state2", "adam_step", "adam"]
    assert ctypes.sizeof(nat.StepDesc) == 56
    assert (nat.STEP_SGD, nat.STEP_ADAGRAD, nat.STEP_ADAM) == (0, 1, 2)


@pytest.mark.parametrize("optimizer", ["SGD", "EXACT_ADAGRAD", "ADAM"])
def test_state_dict_keys_do_not_depend_on_capturable(ops, optimizer):
    mk = lambda **kw: ops.TTEmbeddingBag(800, 100, R, P, Q, optimizer=getattr(ops.OptimType, optimizer), sparse=True,
                                         use_cache=False, weight_dist="normal", **kw)
    plain, cap = mk(), mk(capturable=True)
    assert list(plain.state_dict().keys()) == list(cap.state_dict().keys())
    assert "lr_dev" in dict(cap.named_buffers()) and "lr_dev" not in dict(plain.named_buffers())
    assert cap.lr_dev.dtype.is_floating_point and cap.lr_dev.numel() == 1 and float(cap.lr_dev) == pytest.approx(0.1)
    plain.load_state_dict(cap.state_dict())   # checkpoints interchange, both ways
    cap.load_state_dict(plain.state_dict())
    two = ops.TableBatchedTTEmbeddingBag(2, 800, 100, R, P, Q, sparse=True, capturable=True)
    assert "lr_dev" not in two.state_dict()


def test_capturable_with_a_trained_cache_is_refused(ops):
    with pytest.raises(ValueError, match="capturable=True is not supported.*by value"):
        ops.TTEmbeddingBag(800, 100, R, P, Q, sparse=True, use_cache=True, cache_size=10, hashtbl_size=40, capturable=True)
    # sparse=False has no fused step and ignores the flag
    ops.TTEmbeddingBag(800, 100, R, P, Q, sparse=False, use_cache=True, cache_size=10, hashtbl_size=40, capturable=True)


def test_a_tensor_rate_needs_a_capturable_module(ops):
    import torch
    emb = ops.TTEmbeddingBag(800, 100, R, P, Q, sparse=True, use_cache=False)
    with pytest.raises(TypeError, match="capturable=True"):
        emb.set_learning_rate(torch.tensor([0.05]))
    cap = ops.TTEmbeddingBag(800, 100, R, P, Q, sparse=True, use_cache=False, capturable=True)
    with pytest.raises(ValueError, match="float32 with one element"):
        cap.set_learning_rate(torch.tensor([0.05, 0.1]))
    cap.set_learning_rate(0.25)          # a float is only noted ...
    assert cap.learning_rate == 0.25 and float(cap.lr_dev) == pytest.approx(0.1)
    cap._refresh_lr()                    # ... the next step writes it
    assert float(cap.lr_dev) == 0.25 and cap._lr_mirror == 0.25
    cap.set_learning_rate(torch.tensor([0.5]))
    assert float(cap.lr_dev) == 0.5 and cap._lr_mirror is None
    cap._refresh_lr()                    # set from a tensor: no refresh of the module's own
    assert float(cap.lr_dev) == 0.5
    cap.set_learning_rate(0.125)
    cap._refresh_lr()
    assert float(cap.lr_dev) == 0.125
