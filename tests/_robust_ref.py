"""Krum, the coordinate-wise trimmed mean and the coordinate-wise median in numpy float64, written
from their definitions, and the two input families of ``tests/test_robust_ref_cpu.py`` and
``tests/test_robust_oracle_gpu.py``.

Krum (K rows, weights w, f, m)
  * dist[i][j] = Σ (x_i − x_j)² from differences, in float64. The kernels form their partial sums in
    fp32, so a pair sum above FLT_MAX is +inf (``overflow=None`` keeps the float64 value: the host
    paths sum in float64); inf − inf and NaN give NaN.
  * score[i]: the ``ops.krum_neighbours(K, f)`` smallest off-diagonal entries of row i, summed in
    ascending order; a NaN orders as +inf and the lower index comes first among equals.
  * the max(1, min(m, K)) lowest scores are chosen, a NaN as +inf, the lower index winning a tie.
  * coef[i] = float32(w_i / Σ_chosen w), both in float64; float32(1) / float32(cnt) when the chosen
    weights sum to 0; 0 for a row that is not chosen.
  * mean = the fp32 fma chain Σ_k coef[k]·x_k, k ascending, over the rows with coef != 0.

Trimmed mean and median sort every coordinate in the total order
``−inf < … < −0.0 < +0.0 < … < +inf < NaN``: a NaN is the largest value, never a vote for its
neighbour, and a NaN inside the kept window makes the output NaN. The trimmed mean is the fp32 sum of
the kept values in ascending order from +0.0, divided by float32(K − 2·trim); the even-K median is
0.5·(a + b).

Exact family: rows of small integers. Every fp32 partial sum the kernels form is then an integer
below 2^24 whatever the order (``assert_exact_krum`` / ``assert_exact_trimmed`` check it per case), so
dist, score, the selection and coef are determined bit for bit, and so are the trimmed mean, the
median, and the Krum mean when the coefficients are one power of two.

Hostile family: the exact family with some rows replaced by NaN, ±inf or 3e38 rows (``hostile``).
"""

import functools

import numpy as np

from myfyp_amd.ops import krum_neighbours

FLT_MAX = float(np.finfo(np.float32).max)
BIG = 524291  # 2048 * 256 + 3: every grid-stride loop runs more than once, and a tail
# first coordinate only the second grid-stride trip of k_pairwise_sqdist reaches at n = BIG: its grid
# is 512 blocks of 256 threads, one float4 group each
SECOND_TRIP = 4 * 512 * 256

KINDS = ("nan", "pinf", "ninf", "big", "two_pinf", "two_big", "nan_tail", "nan_second_trip")


def slab_count(n):
    """Blocks (slabs) of the distance launch: min(512, ceil(ceil(n / 4) / 256))."""
    return min(512, -(-(-(-n // 4)) // 256))


# ---------------------------------------------------------------------------------------------
# oracles
# ---------------------------------------------------------------------------------------------
def _key(v):
    return np.inf if v != v else v


def krum_dist(x, overflow=FLT_MAX):
    x = np.asarray(x, dtype=np.float64)
    k = len(x)
    d = np.zeros((k, k))
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(k):
            for j in range(i + 1, k):
                diff = x[i] - x[j]
                s = float((diff * diff).sum())
                if overflow is not None and s > overflow:
                    s = np.inf
                d[i, j] = d[j, i] = s
    return d


def krum_select(d, w, f, m):
    """score, chosen (ascending indices) and coef (float32) from a distance table."""
    k = len(d)
    cnt = krum_neighbours(k, f)
    score = np.zeros(k)
    with np.errstate(invalid="ignore"):
        for i in range(k):
            others = sorted((j for j in range(k) if j != i), key=lambda j: (_key(d[i, j]), j))
            s = 0.0
            for j in others[:cnt]:
                s = s + d[i, j]
            score[i] = s
    order = sorted(range(k), key=lambda i: (_key(score[i]), i))
    chosen = sorted(order[: max(1, min(int(m), k))])
    w64 = [float(v) for v in w]
    ws = 0.0
    for i in chosen:
        ws += w64[i]
    coef = np.zeros(k, dtype=np.float32)
    for i in chosen:
        coef[i] = np.float32(w64[i] / ws) if ws > 0 else np.float32(1) / np.float32(len(chosen))
    return score, chosen, coef


def coef_mean(x, coef):
    """fp32 fma chain, k ascending; a row of coefficient 0 is never read."""
    x = np.asarray(x)
    acc = np.zeros(x.shape[1], dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(len(x)):
            if coef[k] == 0:
                continue
            acc = (np.float64(coef[k]) * x[k].astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
    return acc


def krum(x, w, f, m, overflow=FLT_MAX):
    """dict(dist, score, chosen, coef, mean) of rows x [K, n]."""
    d = krum_dist(x, overflow)
    score, chosen, coef = krum_select(d, w, f, m)
    return dict(dist=d, score=score, chosen=chosen, coef=coef, mean=coef_mean(x, coef))


def mean_is_exact(coef):
    """On the exact family: every product coef·x and every partial sum is exact when the non-zero
    coefficients are one power of two."""
    nz = coef[coef != 0]
    return len(nz) > 0 and bool(np.all(nz == nz[0])) and float(np.log2(float(nz[0]))).is_integer()


def total_sort(x):
    """Every column of float32 x [K, n] sorted in the order −inf < … < −0.0 < +0.0 < … < +inf < NaN."""
    x = np.asarray(x, dtype=np.float32)
    nan = np.isnan(x)
    val = np.where(nan, np.float32(0), x)
    order = np.lexsort((~np.signbit(x), val, nan), axis=0)  # last key first: NaN, value, −0.0 before +0.0
    return np.take_along_axis(x, order, axis=0)


def trimmed_mean(x, trim):
    s = total_sort(x)
    k = len(s)
    acc = np.zeros(s.shape[1], dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(trim, k - trim):
            acc = acc + s[r]
        return acc / np.float32(k - 2 * trim)


def median(x):
    s = total_sort(x)
    k = len(s)
    if k % 2:
        return s[(k - 1) // 2].copy()
    with np.errstate(invalid="ignore", over="ignore"):
        return np.float32(0.5) * (s[k // 2 - 1] + s[k // 2])


# ---------------------------------------------------------------------------------------------
# exactness
# ---------------------------------------------------------------------------------------------
def assert_exact_krum(x):
    """Integer rows whose largest pair distance is below 2^24: every fp32 partial sum of squared
    differences is a non-negative integer no larger, hence exact in any order."""
    x = np.asarray(x, dtype=np.float64)
    fin = x[np.all(np.isfinite(x) & (np.abs(x) < 1e30), axis=1)]
    assert np.array_equal(fin, np.round(fin))
    d = krum_dist(fin, overflow=None)
    assert d.max(initial=0.0) < 2.0**24, d.max()


def assert_exact_trimmed(x):
    """Integer values whose absolute sum over a column is below 2^24: every partial sum of kept
    values is an exact integer."""
    x = np.asarray(x, dtype=np.float64)
    fin = np.where(np.isfinite(x), x, 0.0)
    assert np.array_equal(fin, np.round(fin))
    assert np.abs(fin).sum(axis=0).max() < 2.0**24


# ---------------------------------------------------------------------------------------------
# exact family
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _exact_rows(k, n, seed, ties):
    rng = np.random.default_rng([k, n, seed])
    half = rng.integers(-2, 3, size=(k, (n + 1) // 2))
    x = np.concatenate([half, half[:, ::-1][:, n % 2 :]], axis=1).astype(np.float32)  # palindromes
    assert x.shape == (k, n)
    if ties and k >= 4:
        # row k-2 is row 1 read backwards: not the same row (n > 1), yet at the same distance from
        # every palindrome, so the two scores tie exactly
        x[1] = rng.integers(-2, 3, size=n)
        x[k - 2] = x[1][::-1]
    if ties and k >= 5:
        x[k - 1] = x[0]  # identical rows
    x.setflags(write=False)
    return x


def exact_rows(k, n, seed=0, ties=False):
    """float32 [K, n] of integers in [−2, 2] (a read-only array shared between tests: copy it)."""
    return _exact_rows(k, n, seed, ties)


@functools.lru_cache(maxsize=None)
def _trim_rows(k, n, seed):
    rng = np.random.default_rng([k, n, seed, 7])
    x = rng.integers(-2, 3, size=(k, n)).astype(np.float32)  # duplicates in every column
    x[:, 1::2] = rng.integers(-100000, 100001, size=(k, n))[:, 1::2]  # mostly distinct values
    x[:, 0] = np.where(rng.integers(0, 2, size=k) == 1, np.float32(-0.0), np.float32(0.0))  # ±0.0 mixed
    if n > 2:
        x[:, 2] = np.float32(-0.0)
    if n > 4:
        x[:, 4] = np.where(rng.integers(0, 2, size=k) == 1, np.float32(-0.0), np.float32(1.0))
    x.setflags(write=False)
    return x


def trim_rows(k, n, seed=0):
    """float32 [K, n] of integers: small ones (duplicates), large ones and ±0.0 columns."""
    return _trim_rows(k, n, seed)


# ---------------------------------------------------------------------------------------------
# hostile family
# ---------------------------------------------------------------------------------------------
def bad_rows(k, b, seed=0):
    return sorted(int(i) for i in np.random.default_rng([k, b, seed, 11]).choice(k, size=b, replace=False))


def hostile(x, kind, b, seed=0):
    """A copy of x [K, n] with b rows made hostile, and their indices. The two_* kinds replace two
    rows, the nan_* kinds put one NaN into one row (``nan_tail`` needs n % 4 != 0,
    ``nan_second_trip`` needs n = BIG)."""
    x = np.array(x, dtype=np.float32)
    k, n = x.shape
    if kind in ("two_pinf", "two_big"):
        b = 2
    if kind in ("nan_tail", "nan_second_trip"):
        b = 1
    bad = bad_rows(k, b, seed)
    if kind == "nan":
        x[bad] = np.nan
    elif kind in ("pinf", "two_pinf"):
        x[bad] = np.inf
    elif kind == "ninf":
        x[bad] = -np.inf
    elif kind in ("big", "two_big"):
        x[bad] = np.float32(3e38)
    elif kind == "nan_tail":
        assert n % 4 != 0
        x[bad[0], n - 1] = np.nan
    elif kind == "nan_second_trip":
        assert n == BIG
        x[bad[0], SECOND_TRIP] = np.nan
    else:
        raise ValueError(kind)
    return x, bad


# (K, f, m, kind, b, n) of the hostile Krum cases. f respects Krum's own condition K >= 2f + 3, so
# that a score sums more distances (K − f − 2 >= f + 1) than there can be bad rows at distance 0 of
# each other; b takes values on both sides of f.
def _hostile_krum_cases():
    out = []
    for k, fs in ((5, (1,)), (8, (1, 2)), (16, (1, 6))):
        for f in fs:
            for m in sorted({1, 3, k - f}):
                if m != 3 and f != fs[0]:
                    continue
                for kind in KINDS:
                    if kind == "nan_second_trip":
                        continue
                    for b in sorted({1, f, f + 1, f + 2}):
                        if kind.startswith("two_") and b != 2:
                            continue
                        if kind == "nan_tail" and b != 1:
                            continue
                        out.append((k, f, m, kind, b, 1027))
    out.append((5, 1, 3, "nan_second_trip", 1, BIG))
    out.append((16, 2, 4, "nan_second_trip", 1, BIG))
    return out


HOSTILE_KRUM = _hostile_krum_cases()


def hostile_b(kind, b):
    return 2 if kind.startswith("two_") else 1 if kind.startswith("nan_") else b


def scatter_nans(x, per_column, seed=0):
    """A copy of x with exactly ``per_column`` NaNs in every column, in random rows."""
    x = np.array(x, dtype=np.float32)
    k, n = x.shape
    rng = np.random.default_rng([k, n, per_column, seed, 13])
    rows = np.argsort(rng.random((k, n)), axis=0)[:per_column]
    np.put_along_axis(x, rows, np.float32(np.nan), axis=0)
    return x
