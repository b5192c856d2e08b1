#!/usr/bin/env python3
"""Pin what the step-carrying entry points refuse before they touch the device: tests/golden/step_refusals.json.

Every case is one malformed call (one fault each) to one of the entry points that carry an optimiser step -- plain,
window, exact and flat, by value and by descriptor -- plus the well-formed empty calls, and holds the status and the text of
``ttemb_last_error()`` that come back.  Nothing is launched and ``ttemb_init()`` is not called: buffers that are never
dereferenced are dummy addresses; what the library does read on the host (shape, pointer arrays, descriptor,
hyper-parameters) is real.  Run it against a build of the commit whose behaviour is to be pinned, with no device visible:

    HIP_VISIBLE_DEVICES=-1 ROCR_VISIBLE_DEVICES=-1 TTEMB_LIB=<parent build>/libttemb_hip.so python tests/golden/make_step_refusals.py

``REWORDED`` lists the cases whose message, not status, differs from that record on purpose: two entry points worded one
fault differently and now share the wording of the step builders (csrc/ttemb_api.hip).  tests/test_step_args_host.py runs
``record()`` on the current build and compares.
"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "step_refusals.json")
MAX_CORES = 4
SGD, ADAGRAD, ADAM = 0, 1, 2
P, Q = 0x1000, 0x1008   # a 16-byte aligned and a misaligned address: never dereferenced
BIG = 1 << 30           # a workspace size no check finds too small


class Shape(ctypes.Structure):
    _fields_ = [("T", ctypes.c_int32), ("p", ctypes.c_int32 * MAX_CORES), ("q", ctypes.c_int32 * MAX_CORES),
                ("R", ctypes.c_int32 * (MAX_CORES + 1))]


class AdamParams(ctypes.Structure):
    _fields_ = [("lr", ctypes.c_float), ("eps", ctypes.c_float), ("weight_decay", ctypes.c_float), ("decoupled", ctypes.c_int32),
                ("beta1", ctypes.c_double), ("beta2", ctypes.c_double)]


class StepDesc(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int32), ("lr_dev", ctypes.c_void_p), ("eps", ctypes.c_float), ("state", ctypes.c_void_p),
                ("state2", ctypes.c_void_p), ("adam_step", ctypes.c_void_p), ("adam", ctypes.c_void_p)]


def _shape():
    s = Shape()
    s.T = 3
    for t, (p, q) in enumerate(((10, 2), (10, 2), (10, 4))):
        s.p[t], s.q[t] = p, q
    for t, r in enumerate((1, 4, 4, 1)):
        s.R[t] = r
    return s


def _array():
    a = (ctypes.c_void_p * MAX_CORES)()
    for t in range(3):
        a[t] = P
    return a


SHAPE, CORES, STATE, STATE2 = _shape(), _array(), _array(), _array()
KEEP = []   # what a descriptor points at


def _hp(**kw):
    hp = AdamParams(0.01, 1e-8, 0.0, 0, 0.9, 0.999)
    for k, v in kw.items():
        setattr(hp, k, v)
    KEEP.append(hp)
    return hp


def _desc(kind, flat=False, **kw):
    """A well-formed descriptor of ``kind`` (a flat step's arrays are the call's arguments), then ``kw`` over it."""
    d = StepDesc()
    d.kind, d.lr_dev, d.eps = kind, P, 1e-6
    if kind != SGD and not flat:
        d.state = ctypes.addressof(STATE)
    if kind == ADAM:
        d.adam = ctypes.addressof(_hp())
        if not flat:
            d.state2, d.adam_step = ctypes.addressof(STATE2), P
    for k, v in kw.items():
        setattr(d, k, v)
    KEEP.append(d)
    return d


def _bind(lib):
    vp, i64, i32, f32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_float
    shp, adm, stp = ctypes.POINTER(Shape), ctypes.POINTER(AdamParams), ctypes.POINTER(StepDesc)
    lib.ttemb_last_error.restype = ctypes.c_char_p
    lib.ttemb_backward_sgd.argtypes = [shp, vp, vp, vp, vp, i64, vp, i64, vp, f32, vp, i64, vp, i64, vp]
    lib.ttemb_backward_adagrad.argtypes = [shp, vp, vp, vp, vp, vp, i64, vp, i64, vp, f32, f32, vp, i64, vp, i64, vp]
    lib.ttemb_backward_adam.argtypes = [shp, vp, vp, vp, vp, vp, vp, vp, i64, vp, i64, vp, adm, vp, i64, vp, i64, vp]
    lib.ttemb_backward_step.argtypes = [shp, vp, vp, vp, vp, i64, vp, i64, vp, stp, vp, i64, vp, i64, vp]
    lib.ttemb_backward_sgd_window.argtypes = [shp, vp, vp, vp, i64, i64, i64, i64, vp, f32, vp, i64, vp]
    lib.ttemb_backward_adagrad_window.argtypes = [shp, vp, vp, vp, vp, i64, i64, i64, i64, vp, f32, f32, vp, i64, vp]
    lib.ttemb_backward_adam_window.argtypes = [shp, vp, vp, vp, vp, vp, vp, i64, i64, i64, i64, vp, adm, vp, i64, vp]
    lib.ttemb_backward_step_window.argtypes = [shp, vp, vp, vp, i64, i64, i64, i64, vp, stp, vp, i64, vp]
    lib.ttemb_backward_sgd_exact.argtypes = [shp, vp, vp, vp, i64, i64, vp, f32, vp, i64, vp, i64, vp]
    lib.ttemb_backward_adagrad_exact.argtypes = [shp, vp, vp, vp, vp, i64, i64, vp, f32, f32, vp, i64, vp, i64, vp]
    lib.ttemb_backward_adam_exact.argtypes = [shp, vp, vp, vp, vp, vp, vp, i64, i64, vp, adm, vp, i64, vp, i64, vp]
    lib.ttemb_backward_step_exact.argtypes = [shp, vp, vp, vp, i64, i64, vp, stp, vp, i64, vp, i64, vp]
    lib.ttemb_sgd_step.argtypes = [vp, vp, i64, f32, vp]
    lib.ttemb_sgd_step_guarded.argtypes = [vp, vp, i64, f32, vp, vp]
    lib.ttemb_adagrad_step.argtypes = [vp, vp, vp, i64, f32, f32, vp]
    lib.ttemb_adam_step.argtypes = [vp, vp, vp, vp, vp, i64, f32, adm, vp, vp]
    lib.ttemb_flat_step.argtypes = [vp, vp, vp, vp, vp, i64, f32, stp, vp, vp]
    return lib


# ---- one caller per entry point: the step's arguments vary, everything else is a well-formed call of `n` ids ----
def _lookup(family, kind, n, lr=0.01, eps=1e-6, state=STATE, state2=STATE2, words=P, hp="ok", desc=None):
    """(symbol, arguments) of a by-value lookup backward of ``kind``, or of the descriptor call when ``desc`` is given
    ("null": a null descriptor).  n ids in n bags (a window: the first n of 2 n bags)."""
    s = ctypes.byref(SHAPE)
    hp = _hp() if hp == "ok" else hp
    step = {SGD: ((), (lr,)), ADAGRAD: ((state,), (lr, eps)), ADAM: ((state, state2, words), (hp,))}[kind]
    name = {SGD: "sgd", ADAGRAD: "adagrad", ADAM: "adam"}[kind]
    if desc is not None:
        step, name = ((), (None if desc == "null" else desc,)), "step"
    if family == "plain":
        return f"ttemb_backward_{name}", (s, CORES, *step[0], P, None, P, n, None, n, P, *step[1], P, BIG, None, 0, None)
    if family == "window":
        return f"ttemb_backward_{name}_window", (s, CORES, *step[0], P, P, n, 2 * n, 0, n, P, *step[1], P, BIG, None)
    return f"ttemb_backward_{name}_exact", (s, CORES, *step[0], P, P, n, n, P, *step[1], P, BIG, None, 0, None)


def _flat(kind, n, lr=0.01, eps=1e-6, state=P, state2=P, words=P, hp="ok", desc=None, grad_scale=1.0, skip=None, guarded=False):
    hp = _hp() if hp == "ok" else hp
    if desc is not None:
        return "ttemb_flat_step", (P, state if kind != SGD else None, state2 if kind == ADAM else None,
                                   words if kind == ADAM else None, P, n, grad_scale, None if desc == "null" else desc, skip, None)
    if kind == ADAM:
        return "ttemb_adam_step", (P, state, state2, words, P, n, grad_scale, hp, skip, None)
    if kind == ADAGRAD:
        return "ttemb_adagrad_step", (P, state, P, n, lr, eps, None)
    return ("ttemb_sgd_step_guarded", (P, P, n, lr, skip, None)) if guarded else ("ttemb_sgd_step", (P, P, n, lr, None))


LOOKUPS = ("plain", "window", "exact")


def cases():
    """{case id: (symbol, arguments)}.  Lookups are given no ids (a fault the builder misses ends as an empty call, not a
    launch) except where the body's answer is the point; the flat faults that need elements are given 8."""
    c = {}

    def every_family(what, kind, flat_n=8, **kw):   # one fault on the descriptor call of every family
        flat_kw = {k: v for k, v in kw.items() if k != "desc"}
        for fam in LOOKUPS:
            c[f"{what} / {fam} descriptor"] = _lookup(fam, kind, 0, **kw)
        d = kw.get("desc")
        if isinstance(d, StepDesc):   # the flat call's own descriptor: the same fields, no arrays
            d = _desc(d.kind, True, lr_dev=d.lr_dev, adam=d.adam)
        c[f"{what} / flat descriptor"] = _flat(kind, flat_n, desc=d, **flat_kw)

    # the descriptor itself
    every_family("null descriptor", SGD, desc="null")
    every_family("unknown kind", SGD, desc=_desc(7))
    for kind, name in ((SGD, "SGD"), (ADAGRAD, "Adagrad"), (ADAM, "Adam")):
        every_family(f"null lr_dev, {name}", kind, desc=_desc(kind, lr_dev=None))
        every_family(f"misaligned lr_dev, {name}", kind, desc=_desc(kind, lr_dev=Q))
    # state per kind: the descriptor's arrays for a lookup, the call's own buffers for a flat step
    for fam in LOOKUPS:
        c[f"Adagrad without state / {fam} descriptor"] = _lookup(fam, ADAGRAD, 0, desc=_desc(ADAGRAD, state=None))
        c[f"Adam without state / {fam} descriptor"] = _lookup(fam, ADAM, 0, desc=_desc(ADAM, state=None))
        c[f"Adam without state2 / {fam} descriptor"] = _lookup(fam, ADAM, 0, desc=_desc(ADAM, state2=None))
        c[f"Adam without adam / {fam} descriptor"] = _lookup(fam, ADAM, 0, desc=_desc(ADAM, adam=None))
        c[f"Adam without step words / {fam} descriptor"] = _lookup(fam, ADAM, 0, desc=_desc(ADAM, adam_step=None))
        c[f"misaligned step words / {fam} descriptor"] = _lookup(fam, ADAM, 0, desc=_desc(ADAM, adam_step=Q))
        c[f"Adagrad with null opt_state / {fam} by value"] = _lookup(fam, ADAGRAD, 0, state=None)
        c[f"Adam with null exp_avg / {fam} by value"] = _lookup(fam, ADAM, 0, state=None)
        c[f"Adam with null exp_avg_sq / {fam} by value"] = _lookup(fam, ADAM, 0, state2=None)
        c[f"Adam with null hp / {fam} by value"] = _lookup(fam, ADAM, 0, hp=None)
        c[f"Adam without step words / {fam} by value"] = _lookup(fam, ADAM, 0, words=None)
        c[f"misaligned step words / {fam} by value"] = _lookup(fam, ADAM, 0, words=Q)
    c["Adagrad without state / flat descriptor"] = _flat(ADAGRAD, 8, state=None, desc=_desc(ADAGRAD, True))
    c["Adam without state / flat descriptor"] = _flat(ADAM, 8, state=None, desc=_desc(ADAM, True))
    c["Adam without state2 / flat descriptor"] = _flat(ADAM, 8, state2=None, desc=_desc(ADAM, True))
    c["Adam without adam / flat descriptor"] = _flat(ADAM, 8, desc=_desc(ADAM, True, adam=None))
    c["Adam without step words / flat descriptor"] = _flat(ADAM, 8, words=None, desc=_desc(ADAM, True))
    c["misaligned step words / flat descriptor"] = _flat(ADAM, 8, words=Q, desc=_desc(ADAM, True))
    c["Adagrad with null state / flat by value"] = _flat(ADAGRAD, 8, state=None)
    c["Adam with null exp_avg / flat by value"] = _flat(ADAM, 8, state=None)
    c["Adam with null exp_avg_sq / flat by value"] = _flat(ADAM, 8, state2=None)
    c["Adam with null hp / flat by value"] = _flat(ADAM, 8, hp=None)
    c["Adam without step words / flat by value"] = _flat(ADAM, 8, words=None)
    c["misaligned step words / flat by value"] = _flat(ADAM, 8, words=Q)
    # Adam's domain (a descriptor's lr is not looked at: its negative lr is a well-formed call, here an empty one)
    for what, kw in (("beta1 = 1", dict(beta1=1.0)), ("beta2 < 0", dict(beta2=-0.1)), ("negative eps", dict(eps=-1e-8)),
                     ("negative weight_decay", dict(weight_decay=-0.1)), ("negative lr", dict(lr=-0.01))):
        for fam in LOOKUPS:
            c[f"{what} / {fam} by value"] = _lookup(fam, ADAM, 0, hp=_hp(**kw))
            c[f"{what} / {fam} descriptor"] = _lookup(fam, ADAM, 0, desc=_desc(ADAM, adam=ctypes.addressof(_hp(**kw))))
        c[f"{what} / flat by value"] = _flat(ADAM, 0, hp=_hp(**kw))
        c[f"{what} / flat descriptor"] = _flat(ADAM, 0, desc=_desc(ADAM, True, adam=ctypes.addressof(_hp(**kw))))
    # the rules of the flat steps
    c["n < 0 / ttemb_sgd_step"] = _flat(SGD, -1)
    c["n < 0 / ttemb_sgd_step_guarded"] = _flat(SGD, -1, skip=P, guarded=True)
    c["n < 0 / ttemb_adagrad_step"] = _flat(ADAGRAD, -1)
    c["n < 0 / ttemb_adam_step"] = _flat(ADAM, -1)
    for kind, name in ((SGD, "SGD"), (ADAGRAD, "Adagrad"), (ADAM, "Adam")):
        c[f"n < 0 / flat descriptor, {name}"] = _flat(kind, -1, desc=_desc(kind, True))
    c["grad_scale != 1, SGD / flat descriptor"] = _flat(SGD, 8, desc=_desc(SGD, True), grad_scale=0.5)
    c["grad_scale != 1, Adagrad / flat descriptor"] = _flat(ADAGRAD, 8, desc=_desc(ADAGRAD, True), grad_scale=0.5)
    c["skip word, Adagrad / flat descriptor"] = _flat(ADAGRAD, 8, desc=_desc(ADAGRAD, True), skip=P)
    # well-formed and empty: TTEMB_OK (the exact SGD / Adagrad calls clear their row marks even then: they are not asked)
    for kind, name in ((SGD, "SGD"), (ADAGRAD, "Adagrad"), (ADAM, "Adam")):
        for fam in LOOKUPS:
            if fam == "exact" and kind != ADAM:
                continue
            c[f"no ids, {name} / {fam} by value"] = _lookup(fam, kind, 0)
            c[f"no ids, {name} / {fam} descriptor"] = _lookup(fam, kind, 0, desc=_desc(kind))
        c[f"no elements, {name} / flat by value"] = _flat(kind, 0)
        c[f"no elements, {name} / flat descriptor"] = _flat(kind, 0, desc=_desc(kind, True))
    c["no elements / ttemb_sgd_step_guarded"] = _flat(SGD, 0, skip=P, guarded=True)
    return c


def record(lib_path):
    """{case id: [status, message]} of the library at ``lib_path`` (the message of a call that succeeds is not recorded)."""
    lib = _bind(ctypes.CDLL(lib_path))
    out = {}
    for what, (symbol, args) in cases().items():
        rc = getattr(lib, symbol)(*args)
        out[what] = [symbol, int(rc), lib.ttemb_last_error().decode() if rc != 0 else ""]
    return out


# Cases whose wording changed on purpose since the record was taken: {case id: the wording now}.  The record keeps the old one.
_EXACT_BY_VALUE = {"Adagrad with null opt_state / exact by value": "opt_state is null",
                   "Adam with null exp_avg / exact by value": "exp_avg / exp_avg_sq is null",
                   "Adam with null exp_avg_sq / exact by value": "exp_avg / exp_avg_sq is null"}
REWORDED = {
    # ttemb_backward_step_exact had its own copy of the descriptor checks, and left the rest to the by-value bodies
    "Adagrad without state / exact descriptor": "step: state is null (Adagrad)",
    "Adam without adam / exact descriptor": "step: adam is null (the hyper-parameters)",
    # the by-value exact calls checked their arrays in the exact bodies, in those bodies' words
    **_EXACT_BY_VALUE,
}


if __name__ == "__main__":
    lib_path = os.environ.get("TTEMB_LIB", os.path.join(ROOT, "falcon-ttdforgnns_amd", "lib", "libttemb_hip.so"))
    rec = record(lib_path)
    for what in REWORDED:
        assert what in rec, what
    with open(OUT, "w") as f:
        json.dump({"cases": rec, "reworded": {k: {"recorded": rec[k][2], "now": v} for k, v in REWORDED.items()}}, f, indent=1,
                  sort_keys=True)
        f.write("\n")
    print(f"{OUT}: {len(rec)} cases, {sum(1 for r in rec.values() if r[1] != 0)} refusals")
    sys.exit(0)
