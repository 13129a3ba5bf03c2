"""The float64 oracle of ``tests/_robust_ref.py`` (Krum, trimmed mean, median under the total order
``−inf < … < −0.0 < +0.0 < … < +inf < NaN``) against the host paths: the CPU branch of
``ops.krum_into`` / ``trimmed_mean_into`` / ``median_into``, ``Krum.aggregate`` on numpy rows,
``_math.trimmed_mean`` and ``_math.coordinate_median``; and the properties of the two input families
that ``tests/test_robust_oracle_gpu.py`` relies on.

The host paths sum distances in float64, where a 3e38 row is at a finite ~1e80 of the others; the
kernels' fp32 partial sums overflow there. The oracle is compared with the host in float64
(``overflow=None``), and its fp32 rule (a pair sum above FLT_MAX is +inf) is checked on its own.
"""

import numpy as np
import pytest
import torch

import _robust_ref as R
from myfyp_amd import ops
from myfyp_amd.learning.aggregators import Krum
from myfyp_amd.learning.aggregators._math import coordinate_median, trimmed_mean
from myfyp_amd.learning.frameworks.p2pfl_model import NumpyModel

N = 37  # 37 % 4 == 1: nan_tail applies


def _cls(a):
    """0 finite, 1 +inf, 2 −inf, 3 NaN."""
    a = np.asarray(a, dtype=np.float64)
    return np.where(np.isnan(a), 3, np.where(a == np.inf, 1, np.where(a == -np.inf, 2, 0)))


def _same(got, want, rtol=0.0):
    """Same non-finite class everywhere; finite values equal (or within rtol)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    np.testing.assert_array_equal(_cls(got), _cls(want))
    fin = _cls(want) == 0
    np.testing.assert_allclose(got[fin], want[fin], rtol=rtol, atol=0)


def _rows_t(x):
    return [torch.from_numpy(np.array(r)) for r in x]


def _krum_hosts(x, w, f, m):
    """The oracle in float64 against ops.krum_into on CPU tensors and Krum.aggregate on numpy rows."""
    k = len(x)
    ref = R.krum(x, w, f, m, overflow=None)
    out = torch.empty(x.shape[1])
    dist, score, coef = ops.krum_into(_rows_t(x), [out], w, f, m)
    _same(dist.numpy(), ref["dist"], rtol=1e-12)
    _same(score.numpy(), ref["score"], rtol=1e-12)
    assert sorted(np.flatnonzero(coef.numpy() != 0)) == [i for i in ref["chosen"] if ref["coef"][i] != 0]
    np.testing.assert_array_equal(coef.numpy(), ref["coef"])
    fin = _cls(ref["mean"]) == 0
    np.testing.assert_array_equal(_cls(out.numpy()), _cls(ref["mean"]))
    big = float(np.abs(np.where(np.isfinite(x), x, 0)).max())
    np.testing.assert_allclose(out.numpy()[fin], ref["mean"][fin], rtol=0, atol=max(1, min(m, k)) * 2.0**-23 * big)
    if all(v > 0 and float(v).is_integer() for v in w):
        models = [NumpyModel(None, params=[np.array(r, dtype=np.float64)], num_samples=int(wi), contributors=[str(i)]) for i, (r, wi) in enumerate(zip(x, w))]
        with np.errstate(invalid="ignore", over="ignore"):
            got = Krum(num_byzantine=f, multi=m).aggregate(models).get_parameters()[0]
            ch = ref["chosen"]
            want = sum(x[i].astype(np.float64) * float(w[i]) for i in ch) / sum(float(w[i]) for i in ch)
        _same(got, want, rtol=1e-12)
    return ref


@pytest.mark.parametrize("k", [1, 2, 3, 5, 16])
def test_krum_oracle_equals_the_hosts_on_the_exact_family(k):
    x = R.exact_rows(k, N, ties=True)
    R.assert_exact_krum(x)
    for f in sorted({0, 1, k - 3, k - 2, k, 50}):
        for m in sorted({0, 1, 3, k - 1, k, 100}):
            for w in ([1.0] * k, [float(1 + (3 * i) % 5) for i in range(k)]):
                ref = _krum_hosts(x, w, f, m)
                # on this family the fp32 overflow rule changes nothing
                fp32 = R.krum(x, w, f, m)
                np.testing.assert_array_equal(fp32["dist"], ref["dist"])
                assert fp32["chosen"] == ref["chosen"]


def test_exact_family_ties():
    """Row K−2 is row 1 read backwards: another row, the same score, bit for bit; rows 0 and K−1
    are identical. The lower index wins both ties."""
    x = R.exact_rows(8, 1027, ties=True)
    assert not np.array_equal(x[1], x[6]) and np.array_equal(x[0], x[7])
    ref = R.krum(x, [1.0] * 8, 1, 3)
    assert ref["score"][1] == ref["score"][6] and ref["score"][0] == ref["score"][7]
    assert ref["dist"][0, 7] == 0 and ref["dist"][1, 6] > 0
    for m in range(1, 8):
        ch = R.krum(x, [1.0] * 8, 1, m)["chosen"]
        assert not (6 in ch and 1 not in ch) and not (7 in ch and 0 not in ch)


def test_zero_weights():
    x = R.exact_rows(5, N, ties=True)
    ref = _krum_hosts(x, [0.0] * 5, 1, 3)  # Krum.aggregate takes no all-zero weights: the ops only
    assert [float(ref["coef"][i]) for i in ref["chosen"]] == [float(np.float32(1) / np.float32(3))] * 3
    _, _, coef = ops.krum_into(_rows_t(x), [], [0.0] * 5, 1, 3)
    np.testing.assert_array_equal(coef.numpy(), ref["coef"])
    w = [2.0] * 5
    w[ref["chosen"][0]] = 0.0  # a chosen row of weight 0 among positive ones
    ref = R.krum(x, w, 1, 3)
    assert ref["coef"][ref["chosen"][0]] == 0 and float(ref["coef"].sum()) == 1.0
    _, _, coef = ops.krum_into(_rows_t(x), [], w, 1, 3)
    np.testing.assert_array_equal(coef.numpy(), ref["coef"])


@pytest.mark.parametrize("kind", [k for k in R.KINDS if k != "nan_second_trip"])
def test_krum_oracle_equals_the_hosts_on_the_hostile_family(kind):
    for k, f, m, kd, b, _ in R.HOSTILE_KRUM:
        if kd != kind:
            continue
        x, bad = R.hostile(R.exact_rows(k, N, ties=True), kind, b)
        assert len(bad) == R.hostile_b(kind, b)
        _krum_hosts(x, [1.0] * k, f, m)
        _krum_hosts(x, [float(1 + (3 * i) % 5) for i in range(k)], f, m)


def test_fp32_overflow_rule():
    """3e38 rows: +inf from every other row under the fp32 rule (the float64 sum is finite), 0 from
    an identical 3e38 row; two +inf rows are at NaN of each other, +inf and −inf rows at +inf."""
    x, bad = R.hostile(R.exact_rows(8, N), "two_big", 2)
    d64, d32 = R.krum_dist(x, overflow=None), R.krum_dist(x)
    honest = [i for i in range(8) if i not in bad]
    assert np.all(np.isfinite(d64)) and d64[bad[0], honest[0]] > R.FLT_MAX
    assert np.all(d32[np.ix_(bad, honest)] == np.inf) and d32[bad[0], bad[1]] == 0
    np.testing.assert_array_equal(d32[np.ix_(honest, honest)], d64[np.ix_(honest, honest)])
    x, bad = R.hostile(R.exact_rows(8, N), "two_pinf", 2)
    d = R.krum_dist(x)
    assert np.isnan(d[bad[0], bad[1]]) and np.all(d[np.ix_(bad, honest)] == np.inf)
    x[bad[1]] = -np.inf
    assert R.krum_dist(x)[bad[0], bad[1]] == np.inf


def test_cases_of_the_gpu_file_are_exact():
    """The exactness helpers hold for every case tests/test_robust_oracle_gpu.py uses."""
    import test_robust_oracle_gpu as G

    for k, n in G.DIST_CASES:
        R.assert_exact_krum(R.exact_rows(k, n))
    for k in G.SELECT_KS:
        R.assert_exact_krum(R.exact_rows(k, G.SELECT_N, ties=True))
    for k, f, m, kind, b, n in R.HOSTILE_KRUM:
        x, _ = R.hostile(R.exact_rows(k, n, ties=True), kind, b)
        R.assert_exact_krum(x)
    for k, trim, n in G.TRIM_CASES:
        R.assert_exact_trimmed(R.trim_rows(k, n))
    # the slab counts the distance cases were chosen for
    assert R.slab_count(G.N_G77) == 77 and G.N_G77 % 2 == 1 and G.N_G77 < 77 * 1024
    c16, c6 = 1024 // 120, 1024 // 15
    per = -(-77 // c16)
    assert per == 10 and 77 - 7 * per == 7  # one unrolled block of 8 and two left over; a last chunk of 7
    assert R.slab_count(G.N_G_K6) % c6 != 0 and R.slab_count(G.N_G_K6) > c6
    assert R.slab_count(R.BIG) == 512 and R.BIG > R.SECOND_TRIP


def test_oracle_alone_rejects_every_bad_row():
    """b <= f and m <= K − f (and Krum's K >= 2f + 3): no bad row is chosen, the mean is finite.
    tests/test_robust_oracle_gpu.py asserts coef[bad] == 0 and a finite output for every such case."""
    seen = 0
    for k, f, m, kind, b, n in R.HOSTILE_KRUM:
        assert k >= 2 * f + 3
        if R.hostile_b(kind, b) > f or m > k - f:
            continue
        x, bad = R.hostile(R.exact_rows(k, n, ties=True), kind, b)
        for w in ([1.0] * k, [float(1 + (3 * i) % 5) for i in range(k)]):
            ref = R.krum(x, w, f, m)
            assert all(ref["coef"][i] == 0 for i in bad) and not set(bad) & set(ref["chosen"]), (k, f, m, kind, b)
            assert np.all(np.isfinite(ref["mean"]))
        seen += 1
    assert seen > 20
    assert any(R.hostile_b(kind, b) > f for _, f, _, kind, b, _ in R.HOSTILE_KRUM)  # b > f is there too


# ---------------------------------------------------------------------------------------------
# trimmed mean and median
# ---------------------------------------------------------------------------------------------
def _trim_hosts(x, trim):
    """The oracle against ops.trimmed_mean_into on CPU tensors and _math.trimmed_mean on numpy."""
    k = len(x)
    want = R.trimmed_mean(x, trim)
    outs = [torch.empty(x.shape[1]), torch.from_numpy(np.array(x[0]))]
    rows = _rows_t(x)
    rows[0] = outs[1]  # an output that is an input
    ops.trimmed_mean_into(rows, outs, trim)
    # the torch branch sums in float64: where the kept values' fp32 sum overflows (3e38 rows) it
    # stays finite, and only there
    kept = R.total_sort(x)[trim : k - trim].astype(np.float64)
    ok = np.abs(np.where(np.isfinite(kept), kept, 0)).sum(axis=0) <= R.FLT_MAX
    assert not np.any(np.isfinite(want[~ok]))
    for o in outs:
        _same(o.numpy()[ok], want[ok])
    beta = (trim + 0.5) / k
    assert int(np.floor(beta * k)) == trim
    with np.errstate(invalid="ignore", over="ignore"):
        got = trimmed_mean([[np.array(r)] for r in x], beta)[0]
    _same(got, want)
    return want


def _median_hosts(x):
    want = R.median(x)
    out = torch.empty(x.shape[1])
    ops.median_into(_rows_t(x), [out])
    _same(out.numpy(), want)
    with np.errstate(invalid="ignore", over="ignore"):
        _same(coordinate_median([[np.array(r)] for r in x])[0], want)
    _same(ops.coordinate_median([[t] for t in _rows_t(x)])[0].numpy(), want)
    return want


@pytest.mark.parametrize("k", range(1, 17))
def test_trimmed_and_median_oracle_equals_the_hosts_on_the_exact_family(k):
    x = R.trim_rows(k, N)
    R.assert_exact_trimmed(x)
    for trim in range((k - 1) // 2 + 1):
        want = _trim_hosts(x, trim)
        # float32(sum) / float32(K − 2·trim) of the kept values, written out
        kept = np.sort(x.astype(np.float64), axis=0)[trim : k - trim]
        np.testing.assert_array_equal(want, (kept.sum(axis=0).astype(np.float32) / np.float32(k - 2 * trim)))
    _median_hosts(x)


def test_total_order():
    col = np.array([np.nan, np.inf, 1.0, 0.0, -0.0, -1.0, -np.inf, -np.nan], dtype=np.float32).reshape(-1, 1)
    s = R.total_sort(col)[:, 0]
    assert s[:6].tolist() == [-np.inf, -1.0, 0.0, 0.0, 1.0, np.inf] and np.all(np.isnan(s[6:]))
    assert np.signbit(s[2]) and not np.signbit(s[3])  # −0.0 below +0.0


def test_one_answer_for_nan_1_5():
    """(NaN, 1, 5): the NaN is the largest value, the median and the trim-1 mean are 5."""
    x = np.array([[np.nan], [1.0], [5.0]], dtype=np.float32)
    assert R.median(x)[0] == 5 and R.trimmed_mean(x, 1)[0] == 5
    assert _median_hosts(x)[0] == 5 and _trim_hosts(x, 1)[0] == 5
    two = np.array([[np.nan], [1.0]], dtype=np.float32)  # K = 2 with one NaN: the median is NaN
    assert np.isnan(_median_hosts(two)[0]) and np.isnan(_trim_hosts(two, 0)[0])


@pytest.mark.parametrize("k", [2, 3, 4, 5, 8, 16])
def test_trimmed_and_median_under_hostile_rows(k):
    base = R.trim_rows(k, N)
    tmax = (k - 1) // 2
    for kind in R.KINDS:
        if kind == "nan_second_trip":
            continue
        for b in sorted({1, max(1, tmax), min(k, tmax + 1)}):
            x, bad = R.hostile(base, kind, b)
            hostile = x != base  # NaN, ±inf and 3e38 entries
            nb = int(hostile.sum(axis=0).max())
            lo, hi = np.where(hostile, np.inf, base).min(axis=0), np.where(hostile, -np.inf, base).max(axis=0)
            for trim in range(tmax + 1):
                want = _trim_hosts(x, trim)
                if nb <= trim:
                    # at most trim hostile values per coordinate: finite, inside the honest range
                    assert np.all(np.isfinite(want)) and np.all(want >= lo) and np.all(want <= hi)
            want = _median_hosts(x)
            if nb <= tmax:
                assert np.all(np.isfinite(want)) and np.all(want >= lo) and np.all(want <= hi)
    for per in range(0, k + 1):
        x = R.scatter_nans(base, per)
        for trim in range(tmax + 1):
            want = _trim_hosts(x, trim)
            assert np.all(np.isnan(want)) if per > trim else np.all(np.isfinite(want))
        want = _median_hosts(x)
        nan_mid = per > (k - 1) // 2 if k % 2 else per >= k // 2
        assert np.all(np.isnan(want)) if nan_mid else np.all(np.isfinite(want))
