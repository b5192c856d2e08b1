"""The (compiled shape x kernel form) matrix: one table of cases shared by test_shape_matrix_host.py (no GPU: every case
reaches the family, the flags and the form it names, and every instantiated shape has a case for every form it can reach)
and test_gpu_shape_matrix.py (every case through the C ABI against the float64 oracle, per element).  numpy-free: sizes only.

Forms (paths relative to falcon-ttdforgnns_amd/csrc/; the rules are read there, the host test asks the library):

  form                 what runs                                                 rule
  -------------------  --------------------------------------------------------  ----------------------------------------
  prefix_launch        whole forward, prefix products from their own launch      ttemb_fast3.hip:3629 pfuse_pays() false
  prefix_in_chain      whole forward, prefix products formed in the chain kernel :3629 n_ids < limit p0 p1 (8; 16 at q0 = 8)
  two_phase_launch     forward(phase=1), forward(phase=2): prefix launch         :3648 pfuse_pays_after_grouping() false
  two_phase_in_chain   ... the chain kernel forms them                           :3648 n_ids < 64 p0 p1
  fuse                 backward chunk kernel reduces dG2 itself, no E table      :3243 fused_dg2(): p2 <= fuse_limit()
  plain                backward chunk kernel + group epilogue                    :3857 neither fused nor GF
  gf                   backward chunk kernel forms the group products            :3842 gfuse_pays()
  replicated           E table, one dG2 slab per tile of the reduce kernel       :3211 p2 r2 q2 4 <= 256 KiB
  shared               E table, ONE dG2 slab, float atomics                      :3211 p2 r2 q2 4 > 256 KiB
  wide_forward / wide_two_phase / e_table / lds_slabs   the wide-rank chain      :3289 wide_slab(), forced by the diagnostic
  per_bag              the per-bag MFMA kernels (ttemb_small3.inc)               ttemb_api.hip:378
"""
import os
import re
from collections import namedtuple

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "falcon-ttdforgnns_amd", "csrc")

SCALAR, PER_BAG, PER_BAG_RT, GROUPED, WIDE, MERGED, PADDED, PREFIX, PRODUCTS = 0, 1, 2, 3, 4, 16, 32, 64, 128   # FAMILY_*
CUS = 256   # what the library's sizing assumes where no device can be asked (ttemb_api.hip:48), and an MI355X's count


def source_shapes():
    """The three X(a, b, c, d, e) lists as the sources spell them: {macro name: [(q0, q1, q2, r1, r2), ...]}."""
    out = {}
    for fname, names in (("ttemb_fast3.hip", ("TTEMB_FAST3_SHAPES", "TTEMB_WIDE3_SHAPES")),
                         ("ttemb_small3.inc", ("TTEMB_SMALL_ONLY_SHAPES",))):
        with open(os.path.join(CSRC, fname)) as f:
            text = f.read()
        for name in names:
            m = re.search(r"#define " + name + r"\(X\)((?:\s*\\\n\s*X\([^)]*\))+)", text)
            assert m, f"{name} not found in {fname}"
            out[name] = [tuple(int(v) for v in x.split(",")) for x in re.findall(r"X\(([^)]*)\)", m.group(1))]
    return out


# ------------------------------------------------------------------------------------------------------------------
# the rules, restated (each a few lines of ttemb_fast3.hip; the host test holds them against the library's own answers)
# ------------------------------------------------------------------------------------------------------------------
def fuse_limit(q, r2):
    """Largest p2 of the fused dG2 form, 0 where the shape has none (fuse_shape :1560, fuse_quads :1554, fused_dg2 :3251)."""
    row2 = r2 * q[2]
    if r2 > 16 or row2 % 4 or row2 // 4 > 32:
        return 0
    return 4 * (64 // (row2 // 4)) * (18 if q[0] * q[1] <= 16 and row2 >= 128 else 12)


def shared_slab(p2, q, r2):
    return p2 * r2 * q[2] * 4 > (256 << 10)   # :3211


def prefix_limit(q):
    return 16 if q[0] == 8 else 8   # :3620 (the backward's GF rule below rank 32 is the same number, :3832)


def _a256(n):
    return -(-n // 256) * 256


def backward_tables_bytes(table_p, table_q, table_r, nnz, form, cus=CUS):
    """Bytes a backward's workspace holds beyond a forward's, for a backward in ``form`` ("fuse", "replicated", "shared",
    "e_table", "lds_slabs"): the gradient scratch (ttemb_api.hip:178, :389) and the backward tables of carve_workspace
    (ttemb_fast3.hip:3389-3395).  The forms differ in the E table (nnz r2 q2 floats or nothing) and in the number of dG2
    slabs.  A 2-core table is sized on its 3-core view (p0, 1, p1), q = (q0, 1, q1), ranks (r, r), plus the identity core."""
    R = [1] + list(table_r) + [1]
    scratch = sum(_a256(table_p[t] * R[t] * table_q[t] * R[t + 1] * 4) for t in range(len(table_p)))
    if len(table_p) == 2:
        scratch += _a256(R[1] * R[1] * 4)   # the view's virtual core: once for a forward, twice for a backward
        p, q, r1, r2 = [table_p[0], 1, table_p[1]], [table_q[0], 1, table_q[1]], R[1], R[1]
    else:
        p, q, r1, r2 = list(table_p), list(table_q), R[1], R[2]
    G, row0, row1, row2 = p[0] * p[1], q[0] * r1, r1 * q[1] * r2, r2 * q[2]
    chunks = nnz // 16 + min(nnz, G) + 1
    rows = min(max((-(-nnz // 256) + 63) // 64 * 64, 512), 4096)
    if form in ("e_table", "lds_slabs"):   # the wide-rank chain: wide_k_chunk :3308, wide_slab_wpb :3269, wide_slab_shares :3277
        parts = min(max(-(-4096 // ((r1 // 64) * (q[1] * r2 // 64) * p[1])), 1), 8)
        kc = (-(-p[0] * q[0] // parts) + 31) // 32 * 32
        slices = -(-p[0] * q[0] // kc)
        js = 2 if q[2] % 8 == 0 else 1
        wpb = (160 << 10) // (p[2] * (16 * (q[2] // js) + 5) * 4)
        wpb = 4 if wpb >= 4 else (2 if wpb >= 2 else wpb)
        while wpb > 1 and (r2 // 16 * js) % wpb:
            wpb >>= 1
        shares = max(cus // ((r2 // 16 * js) // max(wpb, 1)), 1)
        slabs = shares if form == "lds_slabs" else (1 if shared_slab(p[2], q, r2) else -(-nnz // rows))
    else:
        gpw = min(max(-(-p[0] // 16), 1), 64)
        slices = -(-p[0] // gpw)
        slabs = {"fuse": min(max(-(-chunks // 16), 1), cus * 2), "replicated": -(-nnz // rows), "shared": 1}[form]
    e = 0 if form in ("fuse", "lds_slabs") else nnz * row2 * 4
    return (scratch + _a256(e) + _a256(G * q[0] * q[1] * r2 * 4) + _a256(slabs * p[2] * row2 * 4) + _a256(G * row0 * 4) +
            _a256(slices * p[1] * row1 * 4) + _a256(slices * p[1] * 4))


# ------------------------------------------------------------------------------------------------------------------
# the table
# ------------------------------------------------------------------------------------------------------------------
# key; inst: the X(...) instantiation the case runs, None off the lists; p, q, r: the table (inner ranks); path: "fast3",
# "auto" or "generic"; pieces: set_piece_limits; wide_slab: set_wide_slab_min_ids; two_phase: forward(phase=1), (phase=2);
# family: kernel_family without the route flags; flags: the route flags it answers; forms: what the case means to reach
Case = namedtuple("Case", "key inst p q r n_ids path pieces wide_slab two_phase family flags forms")

# What each grouped instantiation has beyond the forms every shape has: "pfuse" the chain kernel that forms the prefix
# products (PFuseCfg::ok :1185), "gf" the chunk kernel that forms the group products (GFuseCfg::ok :3824), "fuse" the
# chunk kernel that reduces dG2 (fuse_shape :1560).  The host test asks the library for each and compares.
FAST3 = {
    (4, 5, 5, 16, 16): "pfuse gf fuse", (4, 4, 8, 8, 8): "pfuse gf fuse", (8, 4, 4, 32, 32): "pfuse gf",
    (4, 4, 8, 16, 16): "pfuse gf fuse", (8, 4, 4, 16, 16): "pfuse gf fuse", (4, 5, 5, 32, 32): "gf",
    (4, 4, 8, 32, 32): "gf", (5, 4, 5, 16, 16): "pfuse gf fuse", (5, 5, 4, 16, 16): "pfuse gf fuse",
    (5, 5, 4, 32, 32): "gf", (5, 5, 4, 8, 8): "pfuse fuse", (4, 5, 5, 8, 8): "pfuse fuse",
    (8, 1, 16, 16, 16): "pfuse", (10, 1, 10, 16, 16): "", (16, 1, 8, 16, 16): "fuse",
}
WIDE3 = [(5, 5, 4, 64, 64), (5, 5, 4, 128, 128), (5, 5, 4, 256, 256), (4, 4, 8, 64, 64), (4, 4, 8, 128, 128), (4, 4, 8, 256, 256)]
SMALL_ONLY = list(WIDE3)   # the per-bag kernels' own list names the same six shapes

GROUPED_FORMS = ("prefix_launch", "prefix_in_chain", "two_phase_launch", "two_phase_in_chain", "fuse", "plain", "gf",
                 "replicated", "shared")
WIDE_FORMS = ("wide_forward", "wide_two_phase", "e_table", "lds_slabs")

# (form, what a shape lacks, the rule) -> the (shape, form) pairs kernel_family answers at no size
_WHY = {
    "prefix_in_chain": ("pfuse", "ttemb_fast3.hip:1185 PFuseCfg::ok: q0 <= 8, and at rank 32 only q0 = 8"),
    "two_phase_in_chain": ("pfuse", "ttemb_fast3.hip:1185 PFuseCfg::ok (:3645 asks it for the lookup half as well)"),
    "fuse": ("fuse", "ttemb_fast3.hip:1560 fuse_shape(): rank <= 16 and r2 q2 <= 128"),
    "gf": ("gf", "ttemb_fast3.hip:3824 GFuseCfg::ok: q0 <= 8, q1 > 1, q1 r2 a multiple of 16"),
}


def unreachable():
    """{(inst, form): rule line}."""
    out = {}
    for inst, has in FAST3.items():
        for form, (need, why) in _WHY.items():
            if need not in has.split():
                out[(inst, form)] = why
        if inst[4] >= 32 and "gf" in has.split():
            out[(inst, "plain")] = "ttemb_fast3.hip:3832 gfuse_limit(): no upper limit at rank 32, GF at every density"
    return out


def grouped_forms(p3, q, r2, n_ids, has, two_phase):
    """The forms a grouped call lands on, by the rules above (p3: the 3-core view's p)."""
    G, has = p3[0] * p3[1], has.split()
    if two_phase:
        fwd = "two_phase_in_chain" if "pfuse" in has and n_ids < 64 * G else "two_phase_launch"
    else:
        fwd = "prefix_in_chain" if "pfuse" in has and n_ids < prefix_limit(q) * G else "prefix_launch"
    if "fuse" in has and p3[2] <= fuse_limit(q, r2):
        return (fwd, "fuse")
    gf = "gf" in has and (r2 >= 32 or n_ids < prefix_limit(q) * G)
    return (fwd, "gf" if gf else "plain", "shared" if shared_slab(p3[2], q, r2) else "replicated")


def _name(inst):
    return "q%d%d%d_r%d" % (inst[0], inst[1], inst[2], inst[3]) if inst[1] > 1 else "q%d_%d_r%d" % (inst[0], inst[2], inst[3])


def _grouped_cases():
    cases = []
    for inst, has in FAST3.items():
        q3, r = list(inst[:3]), inst[3]
        past = fuse_limit(q3, r) + 1 if fuse_limit(q3, r) else 30   # the smallest p2 the fused form does not take
        big = (256 << 10) // (4 * r * q3[2]) + 1                    # the smallest p2 with ONE shared slab
        # (name, p0, p1, p2, ids, two-phase): >= 16 ids per group and a small p2 | < 8 per group, p2 past the fused form |
        # > 64 per group | < 64 and >= 16 per group with one shared slab
        for kind, p0, p1, p2, n_ids, two in (("dense", 10, 12, 30, 3000, False), ("sparse", 41, 50, past, 6000, False),
                                             ("phases_dense", 5, 8, past, 3000, True), ("phases_shared", 7, 9, big, 3000, True)):
            if inst[1] == 1:   # reached as users reach it: a 2-core table, lifted onto (p0, 1, p1) with the identity in the middle
                p, q, ranks, view, fam = [p0 * p1, p2], [inst[0], inst[2]], [r], [p0 * p1, 1, p2], GROUPED | MERGED
            else:
                p, q, ranks, view, fam = [p0, p1, p2], q3, [r, r], [p0, p1, p2], GROUPED
            forms = grouped_forms(view, q3, r, n_ids, has, two)
            flags = (PREFIX if "pfuse" in has.split() and n_ids < prefix_limit(q3) * view[0] * view[1] else 0) | \
                    (PRODUCTS if "gf" in forms else 0)
            cases.append(Case(f"{_name(inst)}_{kind}", inst, p, q, ranks, n_ids, "fast3", (0, 0), 0, two, fam, flags, forms))
    return cases


def _wide_cases():
    cases = []
    for inst in WIDE3:
        q, r = list(inst[:3]), inst[3]
        n_ids = 3000 if r == 64 else 1500   # (the float64 oracle on the host dominates at ranks 128 / 256)
        cases.append(Case(f"{_name(inst)}_e_table", inst, [13, 50, 40], q, [r, r], n_ids, "fast3", (0, 0), 1 << 40, False,
                          WIDE, 0, ("wide_forward", "e_table")))
        cases.append(Case(f"{_name(inst)}_lds_slabs", inst, [13, 50, 40], q, [r, r], n_ids, "fast3", (0, 0), 1, True,
                          WIDE, 0, ("wide_two_phase", "lds_slabs")))
    return cases


def _per_bag_cases():
    cases = []
    for inst in FAST3:   # below the grouped crossover (4 096 ids, ttemb_fast3.hip:3139)
        if inst[1] == 1:
            cases.append(Case(f"{_name(inst)}_per_bag", inst, [290, 310], [inst[0], inst[2]], [inst[3]], 2000, "auto", (0, 0), 0,
                              False, PER_BAG | MERGED, 0, ("per_bag",)))
        else:
            cases.append(Case(f"{_name(inst)}_per_bag", inst, [23, 290, 310], list(inst[:3]), [inst[3], inst[4]], 2000, "auto",
                              (0, 0), 0, False, PER_BAG, 0, ("per_bag",)))
    for inst in SMALL_ONLY:   # a wide rank pays on the grouped path from a handful of ids on (:3135): p2 past its limit of 4 096
        cases.append(Case(f"{_name(inst)}_per_bag", inst, [4, 5, 4097], list(inst[:3]), [inst[3], inst[4]],
                          2000 if inst[3] == 64 else 1500, "auto", (0, 0), 0, False, PER_BAG, 0, ("per_bag",)))
    # the run-time-shape kernels (ttemb_rt3.inc): a rank between the instantiated ones, a q no template has, ranks that are
    # no multiples of the MFMA K (the three kinds of test_gpu_parity.py's RT_SHAPES)
    for key, q, ranks in (("rt_rank12", [4, 5, 5], [12, 12]), ("rt_q2510", [2, 5, 10], [16, 16]), ("rt_rank6_7", [4, 5, 5], [6, 7])):
        cases.append(Case(key, None, [30, 35, 40], q, ranks, 2000, "auto", (0, 0), 0, False, PER_BAG_RT, 0, ("per_bag_rt",)))
    return cases


def _scalar_cases():
    return [Case("scalar_2core", None, [6, 7], [4, 3], [5], 600, "generic", (0, 0), 0, False, SCALAR, 0, ("scalar",)),
            Case("scalar_4core", None, [3, 2, 4, 3], [2, 2, 3, 2], [3, 4, 2], 600, "generic", (0, 0), 0, False, SCALAR, 0, ("scalar",)),
            Case("scalar_q0_17", None, [9, 8, 11], [17, 2, 2], [4, 4], 600, "generic", (0, 0), 0, False, SCALAR, 0, ("scalar",))]


CASES = _grouped_cases() + _wide_cases() + _per_bag_cases() + _scalar_cases()


def route_of(case):
    """The depth route of tests/fp32_bound.py for the case's family."""
    return {SCALAR: "scalar", PER_BAG: "per_bag", PER_BAG_RT: "per_bag", GROUPED: "grouped", WIDE: "wide"}[case.family & 7]


def backward_form(case):
    """The form the backward workspace query shows for a grouped / wide case, None for the other families."""
    for f in ("fuse", "shared", "replicated", "e_table", "lds_slabs"):
        if f in case.forms:
            return f
    return None
