"""float64 references of the FedAvg, mixing, SCAFFOLD, optimizer and noise kernels of
``csrc/kernels/fl_ops.hip``, written from the formulas in ``fl_ops.h`` / ``fl_ops.hip`` and
``common.h::opt_update``. Plain numpy; nothing here calls ``myfyp_amd.ops``.

Every function takes the fp32 inputs the kernel gets (weights, betas, lr, eps already rounded to
float: scalars go through :func:`f32`) and returns float64. Where a tolerance is per coordinate the
function also returns what the bound scales with:

* a *magnitude* (``mag``): the sum of the absolute values of the terms of one output, e.g.
  ``Σ_p |w_p x_p,i|``. The caller multiplies it by the number of fp32 roundings on the longest path
  and by :func:`gamma`.
* for the optimizer, where the roundings of one output act on different quantities, *units*: the
  sum over those quantities of (roundings × magnitude), so that the bound is ``units · 2^-24``.

Rows of weight 0 are never read: they may hold NaN without changing a result.
"""

from __future__ import annotations

import math

import numpy as np

U = 2.0**-24  # unit roundoff of fp32, round to nearest


def gamma(r: int) -> float:
    """``r·u / (1 − r·u)``: the relative error of ``r`` fp32 roundings in sequence, second order
    terms included (Higham, Accuracy and Stability of Numerical Algorithms, lemma 3.1)."""
    return r * U / (1.0 - r * U)


def f32(x) -> float:
    """The double value of ``x`` rounded to float, as a C ``float`` argument arrives."""
    return float(np.float32(x))


def _a(x) -> np.ndarray:
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.asarray(x)


def _d(x) -> np.ndarray:
    return _a(x).astype(np.float64)


TINY = f32(1e-12)  # fmaxf(wsum, 1e-12f)


# --------------------------------------------------------------------------------------------
# weighted sums
# --------------------------------------------------------------------------------------------
def weighted_sum(rows, w):
    """``out[i] = Σ_k w[k]·rows[k][i]`` over the rows of weight != 0. Returns ``(out, mag)``,
    ``mag = Σ |w_k x_k,i|``."""
    w = _d(w).reshape(-1)
    n = _a(rows[0]).size
    out, mag = np.zeros(n), np.zeros(n)
    for k in range(len(w)):
        if w[k] == 0.0:
            continue  # never read
        t = w[k] * _d(rows[k]).reshape(-1)
        out += t
        mag += np.abs(t)
    return out, mag


def stacked_weighted_sum(stacked, w, scale=1.0):
    """``out[i] = scale · Σ_p w[p]·stacked[p, i]``; ``mag = |scale| · Σ |w_p x_p,i|``."""
    st = _a(stacked)
    out, mag = weighted_sum([st[p] for p in range(st.shape[0])], w)
    s = f32(scale)
    return s * out, abs(s) * mag


def nonzero(w) -> int:
    """Rows a weighted sum reads."""
    return int(np.count_nonzero(_a(w)))


def broadcast(stacked, src, mask=None):
    """``stacked[p, :n] = src`` for rows with ``mask[p] != 0`` (mask None: every row); the other
    rows and the columns from ``n = len(src)`` on are returned unchanged."""
    out = _d(stacked).copy()
    src = _d(src).reshape(-1)
    for p in range(out.shape[0]):
        if mask is None or float(_a(mask)[p]) != 0.0:
            out[p, : src.size] = src
    return out


# --------------------------------------------------------------------------------------------
# FedAvg over a stacked group
# --------------------------------------------------------------------------------------------
def fedavg_wsum(w) -> float:
    """The weight sum as the entry points form it: summed in double, rounded to float."""
    return f32(_d(w).sum())


def fedavg_reduce(stacked, w):
    """``(out, mag, wsum)``: ``out[i] = Σ_p w[p]·stacked[p, i]`` and the slot's weight sum."""
    out, mag = stacked_weighted_sum(stacked, w)
    return out, mag, fedavg_wsum(w)


def fedavg_apply(stacked, out, wsum, mask):
    """Rows with a mask bit set ``<- out / max(wsum, 1e-12)`` on the first ``len(out)`` columns;
    everything else unchanged. Returns ``(rows, mag)`` with ``mag = |out / max(wsum, 1e-12)|``."""
    rows = _d(stacked).copy()
    out = _d(out).reshape(-1)
    avg = out / max(float(wsum), TINY)
    for p in range(rows.shape[0]):
        if float(_a(mask)[p]) != 0.0:
            rows[p, : out.size] = avg
    return rows, np.abs(avg)


def fedavg_local(stacked, w, mask, n):
    """Single-launch FedAvg: the masked rows ``<- Σ_p w[p]·row_p / max(wsum, 1e-12)`` on the first
    ``n`` columns. Returns ``(rows, mag)``, ``mag = Σ |w_p x_p,i| / max(wsum, 1e-12)``."""
    st = _a(stacked)
    out, mag, wsum = fedavg_reduce(st[:, :n], w)
    rows, _ = fedavg_apply(st, out, wsum, mask)
    return rows, mag / max(wsum, TINY)


def delayed_land(stacked, snap, avg, wsum, mask, n):
    """Masked rows: ``x = row + (avg / max(wsum, 1e-12) − snap)``, ``row <- x``, ``snap <- x``
    on the first ``n`` columns; with ``avg`` None only ``snap <- row``. Returns ``(rows, snap,
    mag)``, ``mag = |row| + |avg / wsum| + |snap|`` (zeros for the snapshot, which is exact)."""
    rows, sn = _d(stacked).copy(), _d(snap).copy()
    mag = np.zeros((rows.shape[0], n))
    a = None if avg is None else _d(avg).reshape(-1)[:n] / max(float(wsum), TINY)
    for p in range(rows.shape[0]):
        if float(_a(mask)[p]) == 0.0:
            continue
        if a is None:
            sn[p, :n] = rows[p, :n]
            continue
        mag[p] = np.abs(rows[p, :n]) + np.abs(a) + np.abs(sn[p, :n])
        x = rows[p, :n] + (a - sn[p, :n])
        rows[p, :n] = x
        sn[p, :n] = x
    return rows, sn, mag


def neighbor_mix(stacked, m, n):
    """``row_p <- Σ_q m[p, q]·row_q`` over the non-zero entries of the dense ``[P, P]`` matrix, on
    the first ``n`` columns; a row whose matrix row is all zero is left alone. Returns ``(rows, mag,
    nsrc)``: ``mag[p] = Σ_q |m[p, q]·row_q|`` and the number of sources per row."""
    x = _d(stacked)
    m = _d(m)
    rows = x.copy()
    mag = np.zeros((x.shape[0], n))
    nsrc = np.count_nonzero(m, axis=1)
    for p in range(x.shape[0]):
        if nsrc[p] == 0:
            continue
        acc = np.zeros(n)
        for q in range(x.shape[0]):
            if m[p, q] != 0.0:  # rows nobody reads may hold anything
                t = m[p, q] * x[q, :n]
                acc += t
                mag[p] += np.abs(t)
        rows[p, :n] = acc
    return rows, mag, nsrc


# --------------------------------------------------------------------------------------------
# coordinate median
# --------------------------------------------------------------------------------------------
def coordinate_median(rows):
    """Per-coordinate median of K rows: the middle value for odd K, ``0.5·(a + b)`` of the middle
    two for even K. The sort is the total order of the kernel's min/max network, −0.0 below +0.0,
    so an odd-K result is one of the inputs, bit for bit. No NaN in the inputs. Returns ``(med,
    mag)`` with ``mag = |med|``."""
    x = np.stack([_d(r).reshape(-1) for r in rows])
    k = x.shape[0]
    key = np.where(x == 0.0, np.where(np.signbit(x), -1.0, 1.0) * 5e-324, x)  # −0 < +0, nothing else moves
    s = np.take_along_axis(x, np.argsort(key, axis=0, kind="stable"), axis=0)
    med = s[(k - 1) // 2] if k % 2 else 0.5 * (s[k // 2 - 1] + s[k // 2])
    return med, np.abs(med)


# --------------------------------------------------------------------------------------------
# SCAFFOLD server step
# --------------------------------------------------------------------------------------------
def scaffold_reduce(dys, dcs, w, n):
    """Packed ``[Σ w_k dy_k | Σ w_k | Σ dc_k | K]`` (2n + 2). Returns ``(buf, mag)`` in the same
    layout: ``Σ |w_k dy_k|``, ``Σ |w_k|``, ``Σ |dc_k|`` and 0 for the exact count."""
    k = len(dys)
    w = _d(w).reshape(-1)[:k] if k else np.zeros(0)
    buf, mag = np.zeros(2 * n + 2), np.zeros(2 * n + 2)
    for i in range(k):
        y, c = _d(dys[i]).reshape(-1), _d(dcs[i]).reshape(-1)
        buf[:n] += w[i] * y
        mag[:n] += np.abs(w[i] * y)
        buf[n + 1 : 2 * n + 1] += c
        mag[n + 1 : 2 * n + 1] += np.abs(c)
    buf[n], mag[n] = w.sum(), np.abs(w).sum()
    buf[2 * n + 1] = float(k)
    return buf, mag


def scaffold_apply(x_start, buf, c, c_init, glr):
    """``x = x_start + glr·buf[:n] / max(buf[n], 1e-12)``;
    ``c' = (0 if c_init else c) + buf[n+1:2n+1] / max(buf[2n+1], 1)``. Returns ``(x, c', mag_x,
    mag_c)``: ``|x_start| + |glr·buf/Σw|`` and ``|c| + |buf/K|``."""
    x0, buf = _d(x_start).reshape(-1), _d(buf).reshape(-1)
    n = x0.size
    step = buf[:n] * (f32(glr) / max(buf[n], TINY))
    dc = buf[n + 1 : 2 * n + 1] / max(buf[2 * n + 1], 1.0)
    c0 = np.zeros(n) if c_init else _d(c).reshape(-1)
    return x0 + step, c0 + dc, np.abs(x0) + np.abs(step), np.abs(c0) + np.abs(dc)


# --------------------------------------------------------------------------------------------
# optimizer (common.h::opt_update, one step from a given (w, m, v))
# --------------------------------------------------------------------------------------------
def _grad(w, grad, anchor, mu, wd):
    """The gradient the update sees, its magnitude and its roundings: ``g + mu·(w − anchor)``
    (sub, mul, add) ``+ wd·w`` (mul, add)."""
    g = _d(grad).copy()
    gm = np.abs(g)
    r = 0
    if anchor is not None and mu != 0.0:
        t = mu * (w - _d(anchor))
        g, gm, r = g + t, gm + np.abs(t), r + 3
    if wd != 0.0:
        g, gm, r = g + wd * w, gm + np.abs(wd * w), r + 2
    return g, gm, r


def _scaffold_tail(w1, units, lr, cg, cl):
    """``w −= lr·(cg − cl)``: sub, mul, sub."""
    if cg is None:
        return w1, units
    t = lr * (_d(cg) - _d(cl))
    w2 = w1 - t
    return w2, units + 2 * np.abs(t) + np.abs(w2)


def adam_step(w, grad, m, v, step, lr, beta1, beta2, eps, wd=0.0, anchor=None, mu=0.0, cg=None, cl=None):
    """One torch.optim.Adam step (L2 weight decay) with the FedProx term in the gradient and the
    SCAFFOLD correction in the update space; the bias corrections ``1 − β^t`` are formed in double
    from the float betas. Returns ``(w', m', v', units_w, units_m, units_v)``.

    Units (roundings × magnitude, so that ``|error| <= units · 2^-24`` to first order), with ``rg``
    the roundings and ``G`` the magnitude of the gradient:

    * ``m' = fma(β1, m, (1 − β1)·g)``: ``1 − β1``, the product, the fma, and g's own ``rg``, all
      acting on quantities no larger than ``M = |β1 m| + (1 − β1)·G``: ``(rg + 3)·M``.
    * ``v' = fma(β2, v, (1 − β2)·g·g)``: ``1 − β2``, two products, the fma, and g's error twice,
      on ``V = β2 v + (1 − β2)·G²``: ``(2 rg + 4)·V``.
    * ``w' = w − (lr / bc1)·(m' / (sqrt(v')·(1 / bc2s) + eps))`` with U the update:
      ``sqrt`` halves v's relative error and adds a rounding; ``bc2s`` (rounded once), its
      reciprocal, the product and the sum with eps add 4; the division 1; ``bc1`` (rounded once),
      ``lr / bc1`` and the product 3: ``|U|·(9 + units_v / (2 v'))``; m's error reaches w scaled by
      ``(lr / bc1) / denom``; the subtraction rounds w' once.
    """
    lr, b1, b2, eps, wd, mu = f32(lr), f32(beta1), f32(beta2), f32(eps), f32(wd), f32(mu)
    w, m, v = _d(w), _d(m), _d(v)
    g, gm, rg = _grad(w, grad, anchor, mu, wd)
    m1 = b1 * m + (1.0 - b1) * g
    um = (rg + 3) * (np.abs(b1 * m) + (1.0 - b1) * gm)
    v1 = b2 * v + (1.0 - b2) * g * g
    uv = (2 * rg + 4) * (b2 * v + (1.0 - b2) * gm * gm)
    bc1 = 1.0 - b1 ** int(step)
    bc2s = math.sqrt(1.0 - b2 ** int(step))
    denom = np.sqrt(v1) / bc2s + eps
    upd = (lr / bc1) * (m1 / denom)
    w1 = w - upd
    with np.errstate(divide="ignore", invalid="ignore"):
        rel_v = np.where(v1 > 0, uv / (2.0 * v1), 0.0)
    uw = np.abs(upd) * (9.0 + rel_v) + (lr / bc1) / denom * um + np.abs(w1)
    w2, uw = _scaffold_tail(w1, uw, lr, cg, cl)
    return w2, m1, v1, uw, um, uv


def sgd_step(w, grad, m, lr, momentum=0.0, wd=0.0, nesterov=False, anchor=None, mu=0.0, cg=None, cl=None):
    """One torch.optim.SGD step (dampening 0) with the same extras. ``m`` may be None when
    ``momentum == 0``: the buffer is then not touched. Returns ``(w', m', units_w, units_m)``.

    * ``m' = momentum·m + g``: a product and a sum, and g's ``rg``, on ``M = |momentum·m| + G``:
      ``(rg + 2)·M``.
    * Nesterov ``g' = g + momentum·m'``: a product and a sum more, on ``G' = G + |momentum|·M``:
      ``(2 rg + 4)·G'``; otherwise ``g' = m'``.
    * ``w' = w − lr·g'``: the product and the subtraction.
    """
    lr, mom, wd, mu = f32(lr), f32(momentum), f32(wd), f32(mu)
    w = _d(w)
    g, gm, rg = _grad(w, grad, anchor, mu, wd)
    m1, um = None, None
    if mom != 0.0:
        m0 = _d(m)
        m1 = mom * m0 + g
        mm = np.abs(mom * m0) + gm
        um = (rg + 2) * mm
        if nesterov:
            g, gm, rg = g + mom * m1, gm + abs(mom) * mm, 2 * rg + 4
        else:
            g, gm, rg = m1, mm, rg + 2
    w1 = w - lr * g
    uw = (rg + 1) * lr * gm + np.abs(w1)
    w2, uw = _scaffold_tail(w1, uw, lr, cg, cl)
    return w2, m1, uw, um


# --------------------------------------------------------------------------------------------
# scale-add-noise
# --------------------------------------------------------------------------------------------
def scale_part(t, scale):
    """The deterministic part of ``t <- scale·t + σ·N(0, 1)``: ``scale·t`` (exact in double)."""
    return f32(scale) * _d(t)


Z_CAP = math.sqrt(2.0 * 24.0 * math.log(2.0))  # Box-Muller of a uniform on a 24-bit grid: -2 ln 2^-24


def normal_cdf(z: np.ndarray) -> np.ndarray:
    return 0.5 * (1.0 + np.vectorize(math.erf, otypes=[np.float64])(z / math.sqrt(2.0)))


def _corr(a, b) -> float:
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / math.sqrt(float((a * a).sum()) * float((b * b).sum())))


def noise_stats(z, sigma, other=None) -> dict:
    """Statistics of N samples ``z`` that should be ``σ·N(0, 1)`` and independent: the largest
    ``|z|/σ``, the mean and variance in units of σ, the Kolmogorov-Smirnov distance to the normal
    CDF, the lag-1 autocorrelation, the correlation of the two halves and, with ``other`` (the
    samples of another seed), the correlation with it."""
    z = _d(z).reshape(-1) / float(sigma)
    n = z.size
    s = np.sort(z)
    cdf = normal_cdf(s)
    i = np.arange(1, n + 1, dtype=np.float64)
    out = {
        "n": n,
        "absmax": float(np.abs(z).max()),
        "mean": float(z.mean()),
        "var": float(z.var()),
        "ks": float(max((i / n - cdf).max(), (cdf - (i - 1) / n).max())),
        "lag1": _corr(z[:-1], z[1:]),
        "halves": _corr(z[: n // 2], z[n // 2 : 2 * (n // 2)]),
    }
    if other is not None:
        out["seeds"] = _corr(z, _d(other).reshape(-1) / float(sigma))
    return out


def noise_limits(n: int) -> dict:
    """Upper limits of ``|statistic|`` for N = n independent normal samples (``var`` is ``|var −
    1|``): five standard errors, and the 0.1 % point of the Kolmogorov-Smirnov statistic."""
    r = math.sqrt(n)
    return {"absmax": Z_CAP * (1 + 1e-3), "mean": 5 / r, "var": 5 * math.sqrt(2.0 / n), "ks": 1.95 / r, "lag1": 5 / r, "halves": 5 / r, "seeds": 5 / r}


def noise_check(stats: dict) -> list:
    """The names of the statistics beyond their limit (empty: all inside)."""
    lim = noise_limits(stats["n"])
    bad = []
    for k, v in stats.items():
        if k == "n":
            continue
        x = abs(v - 1.0) if k == "var" else abs(v)
        if not x <= lim[k]:
            bad.append(f"{k}: {v:.3e} (limit {lim[k]:.3e})")
    return bad
