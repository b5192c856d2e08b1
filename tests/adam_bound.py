"""Float64 Adam / AdamW and the per-element acceptance bound of the fused fp32 step (the Adam sibling of
``fp32_bound.assert_adagrad_grade``).

The arithmetic, per element, t = the number of steps applied including this one (torch.optim.Adam / AdamW, no amsgrad):

    g' = g + wd w                       (coupled;  decoupled: w <- w - lr wd w and g' = g)
    m' = b1 m + (1 - b1) g' ;  v' = b2 v + (1 - b2) g'^2
    w' = w - a m' / (c sqrt(v') + eps),   a = lr / (1 - b1^t),  c = 1 / sqrt(1 - b2^t)

``lr``, ``eps`` and ``wd`` are what fp32 holds of them (as fp32_bound does for lr / eps); the betas are doubles, as the
kernels take them.

The bound.  ``g`` is the float64 gradient, ``delta`` its per-element fp32 bound (``fb.gamma(depth) * mag``).
  m'  within (1 - b1) d' + 4u(|b1 m| + |(1 - b1) g'|)              d' = delta (+ 2u(|g| + |wd w|) when coupled)
  v'  within (1 - b2)(2|g'| d' + d'^2) + 4u v'                     (4u: beta rounded to fp32, a product, a product, a sum)
  w'  within L d' + a r_m / D_min + 16u(|w| + |update|_max)
Adam's update u(g) = a m'(g) / (c sqrt(v'(g)) + eps) is NOT monotone in g once m != 0, so the spread of u over
[g' - d', g' + d'] is bounded with a DERIVATIVE bound (not by the endpoints, not by a sample):
  |du/dg| <= a [ (1 - b1) / D + |m'| c (1 - b2) |g| / (sqrt(v') D^2) ],   D = c sqrt(v') + eps
evaluated with the smallest D (v' at the smallest |g| of the interval, 0 if it straddles 0), the largest |m'| (an endpoint:
m' is linear in g) and |g| / sqrt(v') <= min(|g|_max / sqrt(v'_min), 1 / sqrt(1 - b2)); that is L.  r_m is the rounding part
of the m' bound (it reaches w' through a / D).  16u: the roundings of the kernel's element step that are relative to the
update or to w -- decay product and sum (2), sqrt, c product, eps sum, the two bias corrections rounded from double (2),
lr a, product with m', quotient, difference, v' relative 4u halved by the root (2): 13, taken as 16.
"""
import numpy as np

import fp32_bound as fb

U = fb.U


class Hyper:
    def __init__(self, lr, eps, betas=(0.9, 0.999), wd=0.0, decoupled=False):
        self.lr, self.eps, self.wd = float(np.float32(lr)), float(np.float32(eps)), float(np.float32(wd))
        self.b1, self.b2 = float(betas[0]), float(betas[1])
        self.decoupled = bool(decoupled)

    def coef(self, t):
        return self.lr / (1.0 - self.b1 ** t), 1.0 / np.sqrt(1.0 - self.b2 ** t)


def adam64(w, m, v, g, t, hp):
    """One float64 Adam / AdamW step: (w', m', v').  ``t`` counts this step."""
    w, m, v, g = (np.asarray(x, dtype=np.float64) for x in (w, m, v, g))
    if hp.decoupled:
        w = w - hp.lr * hp.wd * w
    else:
        g = g + hp.wd * w
    m = hp.b1 * m + (1.0 - hp.b1) * g
    v = hp.b2 * v + (1.0 - hp.b2) * g * g
    a, c = hp.coef(t)
    return w - a * m / (c * np.sqrt(v) + hp.eps), m, v


def adam_bounds(w0, m0, v0, g, delta, t, hp):
    """(w', m', v') in float64 and their per-element bounds (bw, bm, bv)."""
    w0, m0, v0, g, delta = (np.asarray(x, dtype=np.float64) for x in (w0, m0, v0, g, delta))
    want_w, want_m, want_v = adam64(w0, m0, v0, g, t, hp)
    wd_w = w0 - hp.lr * hp.wd * w0 if hp.decoupled else w0
    gp = g if hp.decoupled else g + hp.wd * w0
    dp = delta if hp.decoupled else delta + 2 * U * (np.abs(g) + np.abs(hp.wd * w0))
    r_m = 4 * U * (np.abs(hp.b1 * m0) + np.abs((1 - hp.b1) * gp))
    bm = (1 - hp.b1) * dp + r_m
    bv = (1 - hp.b2) * (2 * np.abs(gp) * dp + dp * dp) + 4 * U * want_v
    a, c = hp.coef(t)
    g_lo, g_hi = gp - dp, gp + dp
    g_min = np.where((g_lo <= 0) & (g_hi >= 0), 0.0, np.minimum(np.abs(g_lo), np.abs(g_hi)))
    g_max = np.maximum(np.abs(g_lo), np.abs(g_hi))
    v_min = hp.b2 * v0 + (1 - hp.b2) * g_min * g_min
    d_min = c * np.sqrt(v_min) + hp.eps
    m_max = np.maximum(np.abs(hp.b1 * m0 + (1 - hp.b1) * g_lo), np.abs(hp.b1 * m0 + (1 - hp.b1) * g_hi)) + r_m
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.minimum(np.where(v_min > 0, g_max / np.sqrt(np.maximum(v_min, 1e-300)), np.inf), 1.0 / np.sqrt(1 - hp.b2))
        lip = a * ((1 - hp.b1) / d_min + m_max * c * (1 - hp.b2) * ratio / (d_min * d_min))
        upd_max = a * m_max / d_min
    lip = np.where(d_min > 0, lip, 0.0)          # (eps = 0 and v = 0 over the whole interval: m is 0 too, the update is 0)
    upd_max = np.where(d_min > 0, upd_max, 0.0)
    bw = lip * dp + np.where(d_min > 0, a * r_m / np.maximum(d_min, 1e-300), 0.0) + 16 * U * (np.abs(wd_w) + upd_max)
    if hp.decoupled:
        bw = bw + 2 * U * np.abs(w0)
    return (want_w, want_m, want_v), (bw, bm, bv)


def assert_adam_grade(w_new, m_new, v_new, w0, m0, v0, g, delta, t, hp, what):
    """Cores and both moments after step ``t`` from (w0, m0, v0) are inside the bounds above.  Returns the largest
    err / bound."""
    (ww, wm, wv), (bw, bm, bv) = adam_bounds(w0, m0, v0, g, delta, t, hp)
    r = 0.0
    for got, want, bound, name in ((m_new, wm, bm, "m"), (v_new, wv, bv, "v"), (w_new, ww, bw, "cores")):
        fb.assert_fp32_grade(got, want, bound / fb.gamma(1), 1, f"{what} {name}")
        err = np.abs(np.asarray(got, dtype=np.float64) - want)
        r = max(r, float((err / (bound + 1e-30)).max()))
    return r


def wide_fraction(w0, m0, v0, g, delta, t, hp):
    """Fraction of elements whose w' bound is wider than 10 % of lr (where the check says little)."""
    _, (bw, _, _) = adam_bounds(w0, m0, v0, g, delta, t, hp)
    return float((bw > 0.1 * hp.lr).mean())


def adam32(w, m, v, g, t, hp):
    """A correct fp32 Adam / AdamW step in numpy float32, written the way the kernels evaluate it."""
    f = np.float32
    w, m, v, g = (np.asarray(x, dtype=np.float32) for x in (w, m, v, g))
    lr, eps, wd = f(hp.lr), f(hp.eps), f(hp.wd)
    b1, omb1, b2, omb2 = f(hp.b1), f(1.0 - hp.b1), f(hp.b2), f(1.0 - hp.b2)
    c1, c2 = f(1.0 / (1.0 - hp.b1 ** t)), f(1.0 / np.sqrt(1.0 - hp.b2 ** t))
    if hp.decoupled:
        w = w - lr * wd * w
    else:
        g = g + wd * w
    m = b1 * m + omb1 * g
    v = b2 * v + omb2 * (g * g)
    denom = np.sqrt(v) * c2 + eps
    with np.errstate(divide="ignore", invalid="ignore"):
        upd = np.where(denom > 0, (lr * c1) * m / denom, f(0))
    return (w - upd).astype(f), m.astype(f), v.astype(f)
