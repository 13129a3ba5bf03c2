"""DnC spectral filtering in numpy float64: the oracle of the DnC tests, with ``splitmix64`` and the
tile rule in plain Python integers, the row families the tests use, an fp32 emulation of the slab
sums of ``k_dnc_sqdist`` and the error bounds ``tests/test_dnc_kernels_gpu.py``'s docstring derives.

Definitions (rows x_0..x_{K-1}, weights w; per iteration t the squared distances D over the taken
coordinates): screen, G = −½·J·D_V·J, (λ, u) its top eigenpair by 20 normalised squarings,
s_i = λ·u_i² (+inf for a screened row), the m = ceil(filter_frac·f) highest removed (the higher row
first among equals), a row kept iff every iteration keeps it, coef = float32(w / Σ_kept w)."""

import functools
import math

import numpy as np

import _collude_ref as cref

U = 2.0**-24
M64 = (1 << 64) - 1
TILE = 256
SQUARINGS = 20
DIST_RTOL = 1e-5  # the bound the Krum kernel tests hold a distance to (tests/test_robust_kernels_gpu.py)


def sm64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def tile_plan(n, seed, rnd, t, b):
    """(all_tiles, key, thr, forced, mask [T] bool) of iteration t."""
    tiles = -(-n // TILE)
    if b is None or n <= b:
        return True, 0, M64, 0, np.ones(tiles, dtype=bool)
    thr = min(M64, (b << 64) // n)
    key = sm64(sm64(sm64(seed & M64) ^ (rnd & M64)) ^ t)
    forced = sm64(key ^ M64) % tiles
    mask = np.array([sm64(key ^ tau) < thr or tau == forced for tau in range(tiles)], dtype=bool)
    return False, key, thr, forced, mask


def coord_mask(n, seed, rnd, t, b):
    return np.repeat(tile_plan(n, seed, rnd, t, b)[4], TILE)[:n]


def sqdist(x):
    x = np.asarray(x, dtype=np.float64)
    k = len(x)
    d = np.zeros((k, k))
    with np.errstate(all="ignore"):
        for i in range(k):
            for j in range(i + 1, k):
                d[i, j] = d[j, i] = ((x[i] - x[j]) ** 2).sum()
    return d


def screen(d):
    k = len(d)
    fin = np.isfinite(d)
    scr = [2 * sum(1 for b in range(k) if b != a and not fin[a, b]) > k - 1 for a in range(k)]
    for b in range(1, k):
        if not scr[b] and any(not scr[a] and not fin[a, b] for a in range(b)):
            scr[b] = True
    return np.array(scr, dtype=bool)


def gram(d):
    """−½·J·D·J, symmetrised."""
    k = len(d)
    j = np.eye(k) - 1.0 / k
    g = -0.5 * j @ d @ j
    return 0.5 * (g + g.T)


def top_eig(g):
    """(λ, u) by repeated squaring; (0, zeros) when tr G <= 0."""
    tr = float(np.trace(g))
    if len(g) <= 1 or not tr > 0.0:
        return 0.0, np.zeros(len(g))
    m = g / tr
    for _ in range(SQUARINGS):
        m = m @ m
        m = m / np.trace(m)
    col = m[:, int(np.argmax(np.diag(m)))]
    u = col / np.sqrt((col * col).sum())
    return float(u @ g @ u), u


def scores(d):
    """(s [K], λ, screened [K], u [K] (0 outside V), G of V)."""
    k = len(d)
    scr = screen(d)
    v = np.flatnonzero(~scr)
    s = np.where(scr, np.inf, 0.0)
    u_full = np.zeros(k)
    lam, g = 0.0, np.zeros((0, 0))
    if len(v) > 1:
        g = gram(d[np.ix_(v, v)])
        lam, u = top_eig(g)
        s[v] = lam * u * u
        u_full[v] = u
    return s, lam, scr, u_full, g


def removed_of(s, scr, m):
    order = sorted(range(len(s)), key=lambda a: (-s[a], -a))
    return np.array([bool(scr[a]) or a in order[:m] for a in range(len(s))])


def dnc(x, w, f, filter_frac=1.0, iters=1, b=10000, seed=0, rnd=0):
    """dict(dist, score, lam, removed, coef, out, u, g) of the definition, float64 (coef float32)."""
    x = np.asarray(x, dtype=np.float64)
    k, n = x.shape
    m = int(math.ceil(filter_frac * f))
    res = dict(dist=np.zeros((iters, k, k)), score=np.zeros((iters, k)), lam=np.zeros(iters), removed=np.full(k, -1, dtype=np.int32), u=[], g=[])
    for t in range(iters):
        d = sqdist(x[:, coord_mask(n, seed, rnd, t, b)])
        s, lam, scr, u, g = scores(d)
        res["dist"][t], res["score"][t], res["lam"][t] = d, s, lam
        res["u"].append(u)
        res["g"].append(g)
        gone = removed_of(s, scr, m)
        res["removed"][(res["removed"] < 0) & gone] = t
    w = np.asarray(w, dtype=np.float64)
    kept = res["removed"] < 0
    if not kept.any():
        kept[:] = True
    coef = np.where(kept, w / w[kept].sum(), 0.0).astype(np.float32)
    with np.errstate(all="ignore"):
        res["out"] = sum(np.float64(coef[a]) * x[a] for a in range(k) if coef[a] != 0)
    res["coef"] = coef
    return res


# ---------------------------------------------------------------------------------------------
# the conditions of an exact-selection case, and the bounds
# ---------------------------------------------------------------------------------------------
def eig_ratio(g):
    """λ₂/λ₁ of G by numpy's eigh."""
    ev = np.linalg.eigvalsh(g)
    return float(ev[-2] / ev[-1]) if len(ev) > 1 else 0.0


def margin(s, m):
    """Last removed score over first kept score (inf when the kept scores are 0 or m == 0)."""
    srt = np.sort(s)[::-1]
    if m == 0:
        return float("inf")
    return float(srt[m - 1] / srt[m]) if srt[m] > 0 else float("inf")


def bounds(d, g, lam, u):
    """(absolute bound of λ, absolute bounds of s [K_v]) for distances within DIST_RTOL of ``d``:
    ‖ΔG‖₂ <= ½‖ΔD‖_F <= η = ½·DIST_RTOL·‖D‖_F (‖J‖₂ = 1); |Δλ| <= η (Weyl); sin θ <= 2η/(λ₁ − λ₂)
    (Davis–Kahan), |Δu_i| <= δ = √2·sin θ; |Δs_i| <= η + λ·δ·(2|u_i| + δ). 1e-12 relative covers the
    double arithmetic of both sides."""
    eta = 0.5 * DIST_RTOL * float(np.sqrt((d * d).sum())) + 1e-12 * lam
    ev = np.linalg.eigvalsh(g)
    gap = float(ev[-1] - ev[-2])
    delta = math.sqrt(2.0) * 2.0 * eta / gap
    return eta, eta + lam * delta * (2.0 * np.abs(u) + delta) + 1e-12 * lam


# ---------------------------------------------------------------------------------------------
# row families: honest rows = base + 1e-3·noise, f attackers = μ − γσ of the honest rows (min-max)
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def attacked(k, f, n, seed=0, gs=1.0):
    """(rows fp32 [K, n] never written, attacker indices): honest rows base + 1e-3·noise, the
    attackers' rows μ − gs·γ·σ of the honest ones at spread positions, γ min-max's (gs = 1: the
    min-max row itself; a lone attacker or K <= 5 needs gs > 1 to dominate the top direction)."""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal(n)
    honest = (base + 1e-3 * rng.standard_normal((k - f, n))).astype(np.float32)
    bad = sorted({(1 + i * max(1, (k - 1) // max(1, f))) % k for i in range(f)})
    assert len(bad) == f
    x = np.empty((k, n), dtype=np.float32)
    if f:
        _, g, st = cref.oracle(honest.astype(np.float64), "min_max")
        x[bad] = (st["mu"] - gs * g * st["sigma"]).astype(np.float32)
    x[[i for i in range(k) if i not in bad]] = honest
    x.setflags(write=False)
    return x, bad


# ---------------------------------------------------------------------------------------------
# fp32 emulation of k_dnc_sqdist's slab sums (one grid-stride step per thread: n <= 512·1024)
# ---------------------------------------------------------------------------------------------
def emulate_dist32(x32, mask):
    """D as the kernels form it, up to the contraction of a·a + b·b into one fused multiply-add:
    per thread (dx² + dy²) + (dz² + dw²) of its group in fp32, the wave's xor butterfly, the four
    waves in order, the blocks' slabs in double."""
    x32 = np.asarray(x32, dtype=np.float32)
    k, n = x32.shape
    groups = -(-n // 4)
    grid = min(512, max(1, -(-groups // 256)))
    assert groups <= grid * 256
    pad = np.zeros((k, grid * 1024), dtype=np.float32)
    pad[:, :n] = x32
    take = np.zeros(grid * 1024, dtype=bool)
    take[:n] = np.repeat(mask, TILE)[:n]
    d = np.zeros((k, k))
    for i in range(k):
        for j in range(i + 1, k):
            e = np.where(take, pad[i] - pad[j], np.float32(0)).astype(np.float32).reshape(-1, 4)
            q = e * e
            t = ((q[:, 0] + q[:, 1]) + (q[:, 2] + q[:, 3])).astype(np.float32).reshape(grid, 4, 64)
            for off in (32, 16, 8, 4, 2, 1):
                t = (t + t[:, :, np.arange(64) ^ off]).astype(np.float32)
            wv = t[:, :, 0]
            blk = ((wv[:, 0] + wv[:, 1]).astype(np.float32) + wv[:, 2]).astype(np.float32) + wv[:, 3]
            d[i, j] = d[j, i] = blk.astype(np.float32).astype(np.float64).sum()
    return d
