"""Shared pieces of the calls-in-flight tests (test_outstanding_host.py, test_gpu_outstanding.py): expectations for
gradients that several lookups add into one tensor, and the condition that makes a saved-prefix case mean something.
Imported like fp32_bound / adam_bound; numpy and the oracle only."""
import numpy as np

import fp32_bound as fb
from oracle import tt_oracle as orc

P, Q, RANKS = [23, 290, 310], [4, 5, 5], [1, 16, 16, 1]   # the module cases' table: 6 000 ids run grouped, 700 per bag


# The C ABI routes that keep a plan: (key, p, q, inner ranks, ids, path, family & 7, flags that must be set, kernel ranks,
# wide backward form).  Shapes and id counts of test_gpu_accuracy.py (ABI_CASES, test_wide_rank_chain_...).
PLAN_ROUTES = [
    ("fast3", [8, 20, 3000], [4, 5, 5], [16, 16], 20000, "fast3", 3, 0, None, None),
    ("prefix_in_chain", [41, 50, 30], [4, 5, 5], [16, 16], 6000, "fast3", 3, 64, None, None),
    ("group_products_in_chain", [41, 50, 30], [8, 4, 4], [32, 32], 6000, "fast3", 3, 128, None, None),
    ("padded_12_to_16", [40, 50, 60], [4, 5, 5], [12, 12], 12000, "auto", 3, 32, [16, 16], None),
    ("wide_e_table", [13, 50, 40], [5, 5, 4], [64, 64], 3000, "fast3", 4, 0, None, "e_table"),
    ("wide_lds_slabs", [13, 50, 40], [5, 5, 4], [64, 64], 3000, "fast3", 4, 0, None, "lds_slabs"),
    ("merged_2core", [7, 33], [16, 8], [16], 9000, "auto", 3, 16, None, None),
    ("merged_4core", [12, 9, 14, 11], [5, 5, 2, 2], [16, 16, 16], 15000, "fast3", 3, 16, None, None),
]
# The saved-P cases: the 3-core routes among them.  A merged 2- / 4-core table runs on a 3-core VIEW, and the plan's P is
# the view's (for four cores G0.G1 merged with G2's digit, for two a lifted core): it is no v[T-2] of the table's own
# chain, so the oracle's prefix_cores does not describe it and those routes are left out.
#
# Their id counts (and the wide shape's p2) are their own: the condition of assert_separated() decides them.  The more ids
# meet in one row of dG2, the deeper its sum and the wider its bound next to the difference of the two expectations: at
# the counts above 6 000 ids on p2 = 30 are apart on 90.6 % of the elements, 12 000 on p2 = 60 on 94.0 %, the wide chain's
# 3 000 on p2 = 40 on 82 %.  With the counts below every route is past 95 % (test_outstanding_host.py asserts it).
_SAVED_P_SIZES = {"fast3": (None, 20000), "prefix_in_chain": (None, 2000), "group_products_in_chain": (None, 2000),
                  "padded_12_to_16": (None, 6000), "wide_e_table": ([13, 50, 400], 3000), "wide_lds_slabs": ([13, 50, 400], 3000)}
SAVED_P_ROUTES = [(c[0], _SAVED_P_SIZES[c[0]][0] or c[1]) + c[2:4] + (_SAVED_P_SIZES[c[0]][1],) + c[5:]
                  for c in PLAN_ROUTES if len(c[1]) == 3]


def route_of(case):
    return "wide" if case[6] == 4 else "grouped"


def call_inputs(rng, p, q, n_ids, long_bag=600):
    """ids, offsets and dY of one lookup (fp32_bound's skewed bags and scaled dY)."""
    ids, offs = fb.skewed_bags(rng, p, n_ids, long_bag)
    return ids, offs, fb.scaled_dy(rng, offs.shape[0] - 1, int(np.prod(q)))


def summed(refs, depths):
    """What k backwards leave in one gradient tensor: per core ``(value, mag, n_ids, depth)`` from the per-call oracle
    results ``refs[k][t] = (value, mag, n_ids)`` and depths ``depths[k][t]``.  Values, magnitudes and id counts add; every
    accumulation into the tensor is one more rounding, gamma(d) + u + gamma(d) u <= gamma(d + 1), so the depth is the
    largest of the calls' plus one per addition."""
    out = []
    for t in range(len(refs[0])):
        v = sum(r[t][0] for r in refs)
        m = sum(r[t][1] for r in refs)
        n = sum(r[t][2] for r in refs)
        d = depths[0][t]
        for dk in depths[1:]:
            d = np.maximum(d, dk[t])
        out.append((v, m, n, d + (len(refs) - 1)))
    return out


def assert_summed(got, refs, depths, what):
    """``got[t]`` against ``summed(refs, depths)``: the fp32 bound per element, exact zeros on the rows no call touches.
    Returns the largest err / (u mag)."""
    worst = 0.0
    for t, (v, m, n, d) in enumerate(summed(refs, depths)):
        worst = max(worst, fb.assert_fp32_grade(got[t], v, m, d, f"{what} dG{t}", "core row"))
        fb.assert_untouched(got[t], np.zeros_like(got[t]), n, f"{what} dG{t}")
    return worst


def separation(ref_saved, ref_current, depth, factor=10.0):
    """Fraction of the elements of the touched rows of the LAST core's gradient on which the saved-prefix and the
    current-prefix float64 expectations differ by more than ``factor`` times the fp32 bound (the larger of the two)."""
    (vs, ms, n), (vc, mc, _) = ref_saved[-1], ref_current[-1]
    bound = fb.gamma(np.broadcast_to(depth, vs.shape)) * np.maximum(ms, mc)
    hot = n > 0
    return float((np.abs(vs - vc)[hot] > factor * bound[hot]).mean())


def assert_separated(ref_saved, ref_current, depth, what):
    """A condition of the saved-prefix cases, not a measurement: no kernel result can satisfy both expectations."""
    s = separation(ref_saved, ref_current, depth)
    assert s >= 0.95, f"{what}: the saved-P and current-P gradients are apart on only {s:.1%} of dG2's touched elements"
    return s


def fresh_prefix(rng, cores, p, q, R):
    """W': fresh scaled draws for every core but the last, which stays."""
    new = fb.scaled_cores(rng, p, q, R)
    return new[:-1] + [cores[-1]]


def saved_prefix_refs(ids, offs, dy, w_fwd, w_now, p, q, R):
    """(expectation of a backward on the forward's plan, expectation of a backward without one), cores ``w_now``."""
    return (orc.tt_dense_backward64(ids, offs, dy, w_now, p, q, R, prefix_cores=w_fwd),
            orc.tt_dense_backward64(ids, offs, dy, w_now, p, q, R))
