"""Depth of a core gradient that went through the dedup route (tests/fp32_bound.py's rule: a value that fp32 evaluates with
at most ``d`` roundings along any term's path is within ``gamma(d) * mag`` of the exact one).

The dedup backward has two stages.

1.  The segment sum (``seg_reduce_mapped_kernel`` / ``seg_partial_mapped_kernel`` in ttemb_bag.hip).  For a distinct id j with
    ``m`` positions, ``d_rows[j] = sum_k w[perm[k]] dY[bag(perm[k])]``: the first term one product, then one fma per term
    (one rounding each), ``m`` roundings along the longest path; a segment of more than 512 positions is cut into chunks
    whose partials are added in chunk order, at most ``m // 512 + 1`` more.  With one to spare: ``m + m // 512 + 2``, the
    long-bag depth of the forward pool with ``m`` in the role of the bag length.  (Without weights the products are exact
    and the depth is one less; the bound covers both.)
2.  The TT backward on the DISTINCT ids, which reads ``d_rows`` where a plain call reads ``w dY`` expanded per position.  A
    row i of core t is touched by ``n`` distinct ids: the depth of its gradient as a function of the ``d_rows`` it reads is
    ``fb.grad_depth(route, q, R, t, n, scaled=True)`` -- ``scaled`` because the pooled call's two roundings for the weight /
    the mean's 1 / len are part of what stage 1 leaves or of ``_PadWeights`` / ``_BagMean`` in front of it.

Each term of the row's gradient is a product of core entries with ONE element of one ``d_rows[j]``, so its path runs through
the segment sum of that j and then through stage 2: relative errors (1 + gamma(a))(1 + gamma(b)) <= 1 + gamma(a + b), and
the row's depth is stage 2's plus the largest stage-1 depth among the distinct ids that touch it,

    depth(i) = grad_depth(route, q, R, t, n_distinct(i), scaled=True) + m_max(i) + m_max(i) // 512 + 2,

``m_max(i)`` the largest multiplicity among those ids.  The magnitudes are the plain call's (the oracle on absolute values):
regrouping a sum does not change the sum of its terms' magnitudes.
"""
import numpy as np

import fp32_bound as fb


def segment_depth(m):
    """Roundings of a segment sum over ``m`` positions (number or array)."""
    m = np.asarray(m, dtype=np.int64)
    return m + m // 512 + 2


def touch_counts(ids, p):
    """Per core t: (distinct ids that touch each row, the largest multiplicity among them), two int64 arrays of p[t]
    entries.  ``ids`` are the ids that reach the lookup (pads included: a pad id is looked up, with weight 0)."""
    uniq, mult = np.unique(np.asarray(ids, dtype=np.int64), return_counts=True)
    out = []
    stride = int(np.prod(p))
    for pt in p:
        stride //= pt
        digit = (uniq // stride) % pt
        n = np.bincount(digit, minlength=pt).astype(np.int64)
        m_max = np.zeros(pt, dtype=np.int64)
        np.maximum.at(m_max, digit, mult)
        out.append((n, m_max))
    return out


def dedup_grad_depth(route, q, R, t, n_distinct, m_max):
    """Depth per row of dG_t ([p_t, 1]) on the dedup route; rows no id touches get the depth of n = 0 (they are zeros)."""
    return fb.grad_depth(route, q, R, t, n_distinct, scaled=True) + segment_depth(m_max)[:, None]
