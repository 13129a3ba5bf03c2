"""The colluding attacks (ALIE, IPM, min-max, min-sum) in numpy float64, an fp32 emulation of the
per-coordinate arithmetic of ``k_collude_stats`` / ``k_collude_write`` in the kernels' documented
order, the inputs of ``tests/test_collude_kernels_gpu.py`` and the error bounds its docstring derives.

Definitions (honest rows x_0..x_{H-1}; per coordinate μ the mean and σ the population standard
deviation; a_i = ‖μ − x_i‖², b_i = ⟨μ − x_i, σ⟩, s = ‖σ‖², d_ij = ‖x_i − x_j‖², D = max d_ij,
S = max_i Σ_j d_ij):

* alie    m = μ − z·σ
* ipm     m = r − ε·(μ − r)
* min_max m = μ − γ·σ, the largest γ >= 0 with max_i ‖m − x_i‖² <= D
* min_sum m = μ − γ·σ, the largest γ >= 0 with Σ_i ‖m − x_i‖² <= S
"""

import functools
from statistics import NormalDist

import numpy as np
import torch

U = 2.0**-24
KINDS = ("alie", "ipm", "min_max", "min_sum")
HS = [1, 2, 5, 8, 13, 16]
PS = [1, 3]
NS = [1, 3, 5, 1027, 3073]
BIG = 524291  # 2048 * 256 + 3: the grid-stride loop runs more than once, and a tail
BIG_H = 8
Z, EPS = 1.0, 0.5  # ALIE's z and IPM's ε in the kernel cases


def alie_z(k, f):
    s = k // 2 + 1 - f
    if k - f <= 0:
        return 0.0
    p = (k - f - s) / (k - f)
    return NormalDist().inv_cdf(p) if 0.0 < p < 1.0 else 0.0


def stats(x):
    """μ, σ, a, b, s, d (the H x H table), D, S of float64 rows x [H, n]."""
    x = np.asarray(x, dtype=np.float64)
    h = len(x)
    mu = x.mean(axis=0)
    sigma = np.sqrt(((x - mu) ** 2).sum(axis=0) / h)
    a = ((mu - x) ** 2).sum(axis=1)
    b = ((mu - x) * sigma).sum(axis=1)
    s = float((sigma**2).sum())
    d = np.zeros((h, h))
    for i in range(h):
        for j in range(i + 1, h):
            d[i, j] = d[j, i] = ((x[i] - x[j]) ** 2).sum()
    return dict(mu=mu, sigma=sigma, a=a, b=b, s=s, d=d, D=float(d.max()), S=float(d.sum(axis=1).max()))


def gamma_of(st, kind):
    """γ of min_max / min_sum in closed form from ``stats``."""
    a, b, s, h = st["a"], st["b"], st["s"], len(st["a"])
    if not s > 0:
        return 0.0
    if kind == "min_max":
        disc = np.maximum(0.0, b * b + s * (st["D"] - a))
        return max(0.0, float(((b + np.sqrt(disc)) / s).min()))
    return float(np.sqrt(max(0.0, st["S"] / (h * s) - 1.0)))


def oracle(x, kind, n_out=1, z=None, eps=0.5, ref=None):
    """(m float64 [n], gamma, stats dict) of the definitions above."""
    x = np.asarray(x, dtype=np.float64)
    st = stats(x)
    if kind == "alie":
        g = alie_z(len(x) + n_out, n_out) if z is None else float(z)
        return st["mu"] - g * st["sigma"], g, st
    if kind == "ipm":
        r = np.asarray(ref, dtype=np.float64)
        return r - eps * (st["mu"] - r), float(eps), st
    g = gamma_of(st, kind)
    return st["mu"] - g * st["sigma"], g, st


def constraint(x, m, kind):
    """(left-hand side, right-hand side) of the kind's constraint for a crafted row m."""
    st = stats(x)
    dist = ((np.asarray(m, dtype=np.float64) - np.asarray(x, dtype=np.float64)) ** 2).sum(axis=1)
    return (float(dist.max()), st["D"]) if kind == "min_max" else (float(dist.sum()), st["S"])


def gamma_bisect(x, kind, steps=60):
    """The largest γ >= 0 that meets the constraint, by bisection on μ − γσ (brute force)."""
    st = stats(x)
    if not st["s"] > 0:
        return 0.0

    def ok(g):
        lhs, rhs = constraint(x, st["mu"] - g * st["sigma"], kind)
        return lhs <= rhs

    hi = 1.0
    while ok(hi):
        hi *= 2.0
    lo = 0.0
    for _ in range(steps):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if ok(mid) else (lo, mid)
    return lo


def krum_choice(x, f):
    """Index Krum (m = 1) picks among float64 rows x with bound f."""
    x = np.asarray(x, dtype=np.float64)
    k = len(x)
    d = ((x[:, None, :] - x[None, :, :]) ** 2).sum(axis=2)
    cnt = min(max(1, k - f - 2), k - 1)
    score = [np.sort(np.delete(d[i], i))[:cnt].sum() for i in range(k)]
    return int(np.argmin(score))


# ---------------------------------------------------------------------------------------------
# inputs of the kernel tests
# ---------------------------------------------------------------------------------------------
def close_rows(h, n, seed):
    """Peers that start from one model: base + 1e-3 noise (fp32 torch rows)."""
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(n, generator=g)
    return [base + 1e-3 * (1 + 0.15 * i) * torch.randn(n, generator=g) for i in range(h)]


@functools.lru_cache(maxsize=None)
def case(h, n):
    """(rows fp32 [H, n], float64 numpy copy, reference row fp32 [n], stats): computed once, never written."""
    x = torch.stack(close_rows(h, n, seed=70 + h))
    g = torch.Generator().manual_seed(900 + h)
    ref = x[0] + 2e-3 * torch.randn(n, generator=g)
    x64 = x.double().numpy()
    return x, x64, ref, stats(x64)


def coefs(kind, gamma):
    """(ca, cb, cr) of m = ca·μ + cb·σ + cr·r."""
    return {"alie": (1.0, -Z, 0.0), "ipm": (-EPS, 0.0, 1.0 + EPS)}.get(kind, (1.0, -gamma, 0.0))


# ---------------------------------------------------------------------------------------------
# fp32 emulation of the kernels' per-coordinate arithmetic (collude_coord, then the write)
# ---------------------------------------------------------------------------------------------
def _fma32(a, b, c):
    """fp32 fused multiply-add: the product of two floats is exact in double."""
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(np.float32)


def emulate_coord(x32):
    """(e [H, n], δ [n], σ [n]) in fp32 in the order ``collude_coord`` documents."""
    x32 = np.asarray(x32, dtype=np.float32)
    h = np.float32(len(x32))
    u = x32 - x32[0]
    total = np.zeros_like(x32[0])
    for k in range(len(x32)):
        total = total + u[k]
    delta = total / h
    e = u - delta
    q = np.zeros_like(x32[0])
    for k in range(len(x32)):
        q = _fma32(e[k], e[k], q)
    return e, delta, np.sqrt(q / h)


def emulate_write(x32, ca, cb, cr, ref32=None):
    """m in fp32 in the order ``k_collude_write`` documents."""
    x32 = np.asarray(x32, dtype=np.float32)
    ca, cb, cr = np.float32(ca), np.float32(cb), np.float32(cr)
    _, delta, sigma = emulate_coord(x32)
    t = _fma32(cb, sigma, ca * delta)
    m = _fma32(ca, x32[0], t)
    if ref32 is not None:
        m = _fma32(cr, np.asarray(ref32, dtype=np.float32), m)
    return m


# ---------------------------------------------------------------------------------------------
# the bounds test_collude_kernels_gpu.py's docstring derives
# ---------------------------------------------------------------------------------------------
SLACK = 1.01  # second-order terms


def chain_depth(n):
    """fp32 additions behind one slab entry: 4 fused multiply-adds per grid-stride step (one per
    coordinate of a group), 6 wave steps, 3 block steps."""
    groups = (n + 3) // 4
    grid = min(512, max(1, -(-groups // 256)))
    return 4 * -(-groups // (grid * 256)) + 6 + 3


def coord_bounds(x64):
    """Per coordinate: R (the range of the honest values) and the absolute bounds of e_k, δ and σ."""
    h = len(x64)
    r = x64.max(axis=0) - x64.min(axis=0)
    return r, SLACK * (h + 3) * U * r, SLACK * (h + 1) * U * r, SLACK * (1.25 * h + 4) * U * r


def stat_bounds(x64, st, n):
    """Absolute bounds of a [H], b [H], s and relative bounds of D and S."""
    h = len(x64)
    r, be, _, bs = coord_bounds(x64)
    ben, bsn = float(np.sqrt((be**2).sum())), float(np.sqrt((bs**2).sum()))
    chain = (chain_depth(n) + 3) * U
    a, s = st["a"], st["s"]
    ba = SLACK * (2 * np.sqrt(a) * ben + ben**2 + chain * a)
    bb = SLACK * (np.sqrt(a) * bsn + np.sqrt(s) * ben + ben * bsn + chain * np.sqrt(a * s))
    bss = SLACK * (2 * np.sqrt(s) * bsn + bsn**2 + chain * s)
    rel_d = SLACK * (chain + 2 * U)
    return ba, bb, bss, rel_d


def gamma_bound(x64, st, n, kind):
    """Absolute bound of the float32 γ the device stores."""
    h = len(x64)
    s = st["s"]
    if not s > 0:
        return 0.0
    ba, bb, bss, rel_d = stat_bounds(x64, st, n)
    g = gamma_of(st, kind)
    if kind == "min_sum":
        rho = st["S"] / (h * s)  # = 1 + max_i a_i / s >= 2, so γ >= 1
        return SLACK * rho * (rel_d + bss / s) / (2 * g) + U * g
    a, b, big_d = st["a"], st["b"], st["D"]
    disc = b * b + s * (big_d - a)  # >= s D (2H − 1) / H²
    floor = s * big_d * (2 * h - 1) / h**2
    bdisc = 2 * np.abs(b) * bb + bb**2 + bss * (big_d - a) + (s + bss) * (rel_d * big_d + ba)
    gi = (b + np.sqrt(disc)) / s
    bg = (bb + bdisc / (2 * np.sqrt(floor))) / s + np.abs(gi) * bss / s
    return SLACK * float(bg.max()) + U * g


def out_bound(x64, st, ca, cb, cr, ref64=None, dgamma=0.0):
    """Per-coordinate absolute bound of an output against the float64 m = ca·μ + cb·σ + cr·r."""
    r, _, bd, bs = coord_bounds(x64)
    ca, cb, cr = abs(ca), abs(cb), abs(cr)
    sigma = st["sigma"]
    t = ca * r + cb * sigma  # |ca·δ| <= ca·R
    m1 = ca * np.abs(x64[0]) + t
    b = ca * bd + cb * bs + dgamma * sigma + U * ca * r + U * t + U * m1
    if ref64 is not None:
        b = b + U * (m1 + cr * np.abs(ref64))
    return SLACK * b + 1e-45
