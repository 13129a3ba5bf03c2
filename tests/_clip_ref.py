"""float64 oracle of ClippedGossip (``ops.clipped_gossip_into``, ``k_clip_plan``, ``k_clipped_mix``),
written from the definition and sharing no code with the package.

Definition. K rows x_0..x_{K-1}, shares W[K][K] >= 0 (diagonal ignored; an all-zero row marks a
source that is never written). N_p = {q != p : W_pq > 0}, D_pq = Σ (x_p − x_q)². Radius: fixed
(τ_p = tau) or adaptive (b): F_p = the min(b, |N_p|) members of N_p with the largest D (a non-finite
D counts as +inf, here and in the sum; of two equals the higher row is farther), δ_p = Σ_{F_p} W_pq,
τ_p² = Σ_{N_p∖F_p} W_pq D_pq / δ_p; b = 0: τ_p = +inf; F_p = N_p: τ_p = 0. Scale s_pq = 0 if D_pq is
not finite, 1 if D_pq <= τ_p², else τ_p / sqrt(D_pq). w_eff[p][q] = float32(W_pq · s_pq). Output
x_p + Σ_{q ascending, w_eff != 0} w_eff[p][q]·(x_q − x_p); a row without such a q is left as it is.

Per-element bound of the fp32 mix (``mix_bound``). With u = 2^-24 the kernel computes, for the m
sources q_1 < .. < q_m of row p,
    d_j = fl(x_qj − x_p)                = (x_qj − x_p)(1 + δ_j)             one rounding per difference
    a_j = fl(e_j · d_j + a_{j-1})       = (e_j d_j + a_{j-1})(1 + ε_j)       one per fma (a_0 = 0)
    y   = fl(x_p + a_m)                 = (x_p + a_m)(1 + ε)                 one for the final add
Term j of a_m carries (1 + δ_j)(1 + ε_j)..(1 + ε_m): at most m + 1 factors, so
    |a_m − A| <= γ_{m+1} · S,   A = Σ e_j (x_qj − x_p),  S = Σ |e_j| |x_qj − x_p|,  γ_k = k u / (1 − k u)
and |y − (x_p + A)| <= u |x_p + a_m| + |a_m − A| <= u |x_p + A| + (1 + u) γ_{m+1} S. An underflowing
step adds at most 2^-149 each: (m + 2) · 2^-149 covers them.
"""

import numpy as np

U = 2.0**-24


def sqdist(x):
    """D[K][K] in float64 from differences; symmetric, zero diagonal."""
    x = np.asarray(x, dtype=np.float64)
    k = x.shape[0]
    d = np.zeros((k, k))
    with np.errstate(all="ignore"):
        for i in range(k):
            for j in range(i + 1, k):
                diff = x[i] - x[j]
                d[i, j] = d[j, i] = np.dot(diff, diff)
    return d


def neighbours(w, p):
    return [q for q in range(w.shape[0]) if q != p and w[p, q] > 0]


def aside(dist, w, p, b):
    """F_p: the min(b, |N_p|) farthest neighbours of row p."""
    nb = neighbours(w, p)
    left, out = list(nb), []
    for _ in range(min(int(b), len(nb))):
        far = left[0]
        for q in left[1:]:
            kq = dist[p, q] if np.isfinite(dist[p, q]) else np.inf
            kf = dist[p, far] if np.isfinite(dist[p, far]) else np.inf
            if kq >= kf:  # ascending q: of two equals the higher row replaces the lower
                far = q
        out.append(far)
        left.remove(far)
    return sorted(out)


def plan(dist, w, tau=None, b=None):
    """(tau [K], tau2 [K], w_eff float32 [K][K]) from the distances."""
    assert (tau is None) != (b is None)
    w = np.asarray(w, dtype=np.float64)
    k = w.shape[0]
    taus, tau2s = np.zeros(k), np.zeros(k)
    w_eff = np.zeros((k, k), dtype=np.float32)
    with np.errstate(all="ignore"):
        for p in range(k):
            nb = neighbours(w, p)
            if tau is not None:
                t, t2 = float(tau), float(tau) * float(tau)
            elif b == 0:
                t = t2 = np.inf
            else:
                f = aside(dist, w, p, b)
                if len(f) == len(nb):
                    t = t2 = 0.0
                else:
                    delta = sum(w[p, q] for q in f)
                    s = 0.0
                    for q in nb:
                        if q not in f:
                            s += w[p, q] * (dist[p, q] if np.isfinite(dist[p, q]) else np.inf)
                    t2 = s / delta
                    t = np.sqrt(t2)
            taus[p], tau2s[p] = t, t2
            for q in nb:
                d = dist[p, q]
                if not np.isfinite(d):
                    continue
                scale = 1.0 if d <= t2 else t / np.sqrt(d)
                w_eff[p, q] = np.float32(w[p, q] * scale)
    return taus, tau2s, w_eff


def mix(x, w_eff):
    """The output rows in float64 for given effective weights (rows without a source: as they are)."""
    x = np.asarray(x, dtype=np.float64)
    out = x.copy()
    with np.errstate(all="ignore"):
        for p in range(x.shape[0]):
            srcs = [q for q in range(x.shape[0]) if w_eff[p, q] != 0]
            if not srcs:
                continue
            acc = np.zeros(x.shape[1])
            for q in srcs:
                acc = acc + np.float64(w_eff[p, q]) * (x[q] - x[p])
            out[p] = x[p] + acc
    return out


def clipped_gossip(x, w, tau=None, b=None):
    """The whole definition: (out [K][n] float64, dist, tau, tau2, w_eff)."""
    d = sqdist(x)
    taus, tau2s, w_eff = plan(d, w, tau, b)
    return mix(x, w_eff), d, taus, tau2s, w_eff


def mix_bound(x, w_eff):
    """Per-element bound [K][n] of the fp32 mix against ``mix(x, w_eff)`` (module docstring)."""
    x = np.asarray(x, dtype=np.float64)
    k = x.shape[0]
    bound = np.zeros_like(x)
    exact = mix(x, w_eff)
    with np.errstate(all="ignore"):
        for p in range(k):
            srcs = [q for q in range(k) if w_eff[p, q] != 0]
            if not srcs:
                continue  # not written: bit-identical
            m = len(srcs)
            s = sum(abs(np.float64(w_eff[p, q])) * np.abs(x[q] - x[p]) for q in srcs)
            gamma = (m + 1) * U / (1 - (m + 1) * U)
            bound[p] = U * np.abs(exact[p]) + (1 + U) * gamma * s + (m + 2) * 2.0**-149
    return bound


def mix_f32(x32, w_eff):
    """fp32 emulation of ``k_clipped_mix``'s arithmetic: fl(x_q − x_p), a fused multiply-add per
    source in ascending q (the float64 product of two floats is exact; its sum with the accumulator
    is rounded to float64 and then to float32, which differs from one rounding in rare ties only),
    then fl(x_p + acc)."""
    x32 = np.asarray(x32, dtype=np.float32)
    out = x32.copy()
    with np.errstate(all="ignore"):
        for p in range(x32.shape[0]):
            srcs = [q for q in range(x32.shape[0]) if w_eff[p, q] != 0]
            if not srcs:
                continue
            acc = np.zeros(x32.shape[1], dtype=np.float32)
            for q in srcs:
                d = (x32[q] - x32[p]).astype(np.float32)
                acc = (np.float64(w_eff[p, q]) * d.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
            out[p] = (x32[p] + acc).astype(np.float32)
    return out


def ring(k, share=None):
    """W of a ring of k rows: each row gives both neighbours ``share`` (default 1/3)."""
    w = np.zeros((k, k))
    s = 1.0 / 3.0 if share is None else share
    for p in range(k):
        for q in ((p - 1) % k, (p + 1) % k):
            if q != p:
                w[p, q] = s
    return w


def star(k):
    """Hub row 0 gives every leaf 1/k; a leaf gives the hub 1/2."""
    w = np.zeros((k, k))
    w[0, 1:] = 1.0 / k
    w[1:, 0] = 0.5
    return w


def full(k):
    w = np.full((k, k), 1.0 / k)
    np.fill_diagonal(w, 0.0)
    return w


def close_rows(k, n, seed, far=(), grade=3e-3):
    """Peers that start from one model: row i is (1 + grade·i)·base plus (1 + 0.15 i)·1e-3 of noise
    (the ``_close_rows`` of the Krum tests, graded); the rows in ``far`` are −2·base, −base instead.
    The grading is what lets a far row tell its neighbours apart: from −c·base the honest rows lie
    at (c + 1 + grade·i)·|base|, 2·grade/(c + 1) >= 2e-3 apart per index, where the noise alone
    would leave them within 1e-4 of each other. float32 [K][n]."""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal(n)
    rows = [(1 + grade * i) * base + 1e-3 * (1 + 0.15 * i) * rng.standard_normal(n) for i in range(k)]
    for t, i in enumerate(far):
        rows[i] = -(2.0 - t) * base + 1e-3 * rng.standard_normal(n)
    return np.stack(rows).astype(np.float32)


def selection_gap(dist, w, b, rows=None):
    """The smallest relative gap, over the rows (default: all), between the b-th and (b+1)-th farthest neighbour
    (inf where b is 0 or takes the whole neighbourhood): above 1e-3 the choice of F_p is not a coin toss."""
    gap = np.inf
    for p in range(w.shape[0]) if rows is None else rows:
        nb = neighbours(w, p)
        if b == 0 or b >= len(nb):
            continue
        d = np.sort(np.array([dist[p, q] for q in nb]))[::-1]
        gap = min(gap, (d[b - 1] - d[b]) / d[b - 1])
    return gap
