"""What the step-carrying entry points refuse before they touch the device (no GPU): every malformed step -- null or
unknown descriptor, null or misaligned rate word, missing state per kind, Adam's domain and step words, the rules of the flat
steps -- sent to every entry point that can carry it, plus the well-formed empty calls.  The expected (status, message) pairs
were recorded from the commit before the step builders (tests/golden/make_step_refusals.py -> step_refusals.json); statuses
must be equal, messages too except the listed cases that now share a builder's wording.  The calls run in a child process
with no device visible and without ``ttemb_init()``, like test_capture_variable_host.py."""
import json
import os
import subprocess
import sys

import pytest


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
LIB = os.path.join(ROOT, "falcon-ttdforgnns_amd", "lib", "libttemb_hip.so")


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "step_refusals.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def now():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    code = ("import json, sys; sys.path[:0] = [sys.argv[1]]\n"
            "import make_step_refusals as m\n"
            "print(json.dumps({'cases': m.record(sys.argv[2]), 'reworded': m.REWORDED}))\n")
    r = subprocess.run([sys.executable, "-c", code, GOLDEN, LIB], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return json.loads(r.stdout)


def test_the_same_cases_are_asked_as_were_recorded(recorded, now):
    assert sorted(now["cases"]) == sorted(recorded["cases"])
    assert {k: v[0] for k, v in now["cases"].items()} == {k: v[0] for k, v in recorded["cases"].items()}   # (the symbols)
    assert len(recorded["cases"]) > 140


def test_every_entry_point_is_asked(recorded):
    """... but ttemb_backward_sgd_exact: by value SGD has no step argument that can be wrong, and even its empty call clears
    the row marks on the device."""
    symbols = {v[0] for v in recorded["cases"].values()}
    kinds = ("sgd", "adagrad", "adam", "step")
    assert symbols == ({f"ttemb_backward_{k}{s}" for k in kinds for s in ("", "_window", "_exact")}
                       | {"ttemb_sgd_step", "ttemb_sgd_step_guarded", "ttemb_adagrad_step", "ttemb_adam_step", "ttemb_flat_step"}
                       ) - {"ttemb_backward_sgd_exact"}
    assert len(symbols) == 16


def test_every_status_is_what_it_was(recorded, now):
    bad = {k: (v[1], now["cases"][k][1]) for k, v in recorded["cases"].items() if v[1] != now["cases"][k][1]}
    assert not bad, bad


def test_the_malformed_calls_are_refused_and_the_empty_ones_are_not(recorded):
    """The record itself: -1 (TTEMB_E_BADARG) for a fault; 0 for an empty well-formed call, for a negative count on the
    by-value SGD / Adagrad epilogues (they have always ignored it) and for a descriptor whose AdamParams carry a negative
    lr (a descriptor's rate is the device word)."""
    for what, (symbol, rc, msg) in recorded["cases"].items():
        ok = (what.startswith(("no ids", "no elements")) or what.startswith("negative lr") and what.endswith("descriptor")
              or what.startswith("n < 0") and symbol in ("ttemb_sgd_step", "ttemb_sgd_step_guarded", "ttemb_adagrad_step"))
        assert rc == (0 if ok else -1), (what, rc, msg)
        assert (msg == "") == ok, (what, msg)


def test_every_message_is_what_it_was_but_for_the_listed_rewordings(recorded, now):
    assert sorted(now["reworded"]) == sorted(recorded["reworded"])
    for what, (_, _, msg) in recorded["cases"].items():
        got = now["cases"][what][2]
        if what in recorded["reworded"]:
            r = recorded["reworded"][what]
            assert r["recorded"] == msg and r["now"] == now["reworded"][what] and r["recorded"] != r["now"], what
            assert got == r["now"], (what, got)
        else:
            assert got == msg, (what, got, msg)
