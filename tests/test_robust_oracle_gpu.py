"""``k_pairwise_sqdist<K>``, ``krum_sum_slabs`` / ``k_krum_select``, ``k_coef_mean<K>``,
``k_trimmed_mean<K>`` and ``k_coordinate_median<K>`` of ``csrc/kernels/fl_ops.hip`` against the
float64 oracle of ``tests/_robust_ref.py``, bit for bit, under hostile rows (MI355X only).

Why bits. On the exact family (rows of small integers) every fp32 partial sum the kernels form is an
integer below 2^24, whatever the order (``tests/test_robust_ref_cpu.py`` checks it for every case
here), so the distances, the scores, the selection, the coefficients, the trimmed mean and the
median are determined bit for bit: one dropped slab, one swapped pair, one kept value too many or a
tie broken the other way changes a compared number. The Krum mean is bit-determined when its
coefficients are one power of two; otherwise it is within ``min(m, K) · 2^-24 · max|x_honest|`` of
the oracle's fp32 fma chain (one rounding per fused multiply-add, coefficients that sum to 1).

Under hostile rows (NaN, ±inf, 3e38) a number is either finite and bit-equal, or in the oracle's
class (+inf, −inf, NaN). The sorts order ``−inf < … < −0.0 < +0.0 < … < +inf < NaN``.
"""

import ctypes

import numpy as np
import pytest
import torch

import _robust_ref as R

pytestmark = pytest.mark.gpu

BIG = R.BIG
# 77 slabs: at K = 16 (8 chunks of per = 10) one unrolled block of eight and two left over, and a
# last chunk of 7
N_G77 = 77 * 1024 - 5
# 70 slabs: at K = 6 (68 chunks) per = 2, the last 33 chunks are empty
N_G_K6 = 70 * 1024 - 3
DIST_NS = [1, 3, 4, 5, 1027]
DIST_EXTRA = {16: [N_G77, BIG], 6: [N_G_K6], 2: [BIG], 7: [N_G77]}
DIST_CASES = [(k, n) for k in range(2, 17) for n in DIST_NS + DIST_EXTRA.get(k, [])]
SELECT_KS = [1, 2, 3, 5, 16]
SELECT_N = 1027
TRIM_NS = [1, 7, 1001]
TRIM_EXTRA = {16: [(0, BIG), (7, BIG)], 5: [(1, BIG)]}
TRIM_CASES = [(k, t, n) for k in range(1, 17) for t in range((k - 1) // 2 + 1) for n in TRIM_NS] + [
    (k, t, n) for k, v in TRIM_EXTRA.items() for t, n in v
]


@pytest.fixture(scope="module")
def dev():
    from myfyp_amd.ops import _native

    _native.load(required=True)  # the native path must be the one under test
    return torch.device("cuda")


def _rows(x, dev, packed=False):
    """Device rows of x [K, n]: separately allocated (16-byte aligned: the float4 path) or slices of
    one packed buffer (odd n: 4-byte aligned only, the scalar path)."""
    if packed:
        buf = torch.from_numpy(np.array(x)).to(dev)
        if x.shape[1] % 2 and len(x) > 1:
            assert buf[1].data_ptr() % 16 != 0
        return [buf[i] for i in range(len(x))]
    rows = [torch.from_numpy(np.array(r)).to(dev) for r in x]
    assert all(r.data_ptr() % 16 == 0 for r in rows)
    return rows


def _np(t):
    return t.cpu().numpy()


def _assert_bits(got, want, what=""):
    """NaN exactly where the oracle has one; every other value (±inf and ±0.0 too) bit for bit."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype)
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), nan, err_msg=f"{what}: NaN pattern")
    view = np.int32 if got.dtype == np.float32 else np.int64
    bad = np.flatnonzero((got.view(view) != want.view(view)).ravel() & ~nan.ravel())
    assert bad.size == 0, f"{what}: {bad.size} values differ, first at {bad[:5]}: got {got.ravel()[bad[:5]]}, want {want.ravel()[bad[:5]]}"


# ---------------------------------------------------------------------------------------------
# distances
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(2, 17))
def test_distances_exact(dev, k):
    from myfyp_amd import ops

    for n in [n for kk, n in DIST_CASES if kk == k]:
        x = R.exact_rows(k, n)
        want = R.krum_dist(x)
        got = {}
        for packed in (False, True):
            dist = _np(ops.krum_into(_rows(x, dev, packed), [], [1.0] * k, 1, 3)[0])
            _assert_bits(dist, want, f"dist K={k} n={n} G={R.slab_count(n)} packed={packed}")
            assert np.array_equal(dist, dist.T) and np.all(np.diag(dist) == 0)
            got[packed] = dist
        assert np.array_equal(got[False], got[True])


# ---------------------------------------------------------------------------------------------
# selection
# ---------------------------------------------------------------------------------------------
def _check_mean(out, ref, x, honest, m, what):
    if R.mean_is_exact(ref["coef"]):
        _assert_bits(out, ref["mean"], what)
    else:
        atol = min(max(m, 1), len(x)) * 2.0**-24 * float(np.abs(x[honest]).max())
        err = float(np.abs(out.astype(np.float64) - ref["mean"].astype(np.float64)).max())
        assert err <= atol, (what, err, atol)


@pytest.mark.parametrize("k", SELECT_KS)
def test_selection_sweep(dev, k):
    from myfyp_amd import ops

    n = SELECT_N
    x = R.exact_rows(k, n, ties=True)
    d = R.krum_dist(x)
    rows = _rows(x, dev)
    unequal = [float(1 + (3 * i) % 5) for i in range(k)]
    out = torch.empty(n, device=dev)
    for f in sorted({0, 1, k - 3, k - 2, k, 50}):
        for m in sorted({0, 1, 3, k - 1, k, 100}):
            score, chosen, _ = R.krum_select(d, unequal, f, m)
            zero_one = [2.0] * k
            zero_one[chosen[0]] = 0.0 if len(chosen) > 1 else 2.0  # a chosen row of weight 0 among positive ones
            for w in (unequal, [0.0] * k, zero_one):
                what = f"K={k} f={f} m={m} w={w}"
                sc, ch, coef = R.krum_select(d, w, f, m)
                assert ch == chosen
                dist_t, score_t, coef_t = ops.krum_into(rows, [out], w, f, m)
                _assert_bits(_np(dist_t), d, "dist " + what)
                _assert_bits(_np(score_t), sc, "score " + what)
                _assert_bits(_np(coef_t), coef, "coef " + what)
                if w is unequal:
                    assert sorted(np.flatnonzero(_np(coef_t) != 0)) == chosen, what
                ref = dict(coef=coef, mean=R.coef_mean(x, coef))
                _check_mean(_np(out), ref, x, list(range(k)), m, "mean " + what)


@pytest.mark.parametrize("k", [2, 3, 5, 16])
def test_a_chosen_row_of_weight_zero_is_never_read(dev, k):
    """m = K chooses every row whatever the scores. The row of weight 0 is chosen with coefficient 0;
    filled with NaN it leaves the mean finite: k_coef_mean<K> skips rows of coefficient 0."""
    from myfyp_amd import ops

    n = SELECT_N
    x = np.array(R.exact_rows(k, n, ties=True))
    r = k // 2
    w = [2.0] * k
    w[r] = 0.0
    x[r] = np.nan
    ref = R.krum(x, w, 1, k)
    assert ref["chosen"] == list(range(k)) and ref["coef"][r] == 0 and np.all(np.isfinite(ref["mean"]))
    for packed in (False, True):
        rows = _rows(x, dev, packed)
        outs = [torch.empty(n, device=dev), rows[0]]
        _, _, coef = ops.krum_into(rows, outs, w, 1, k)
        _assert_bits(_np(coef), ref["coef"], "coef")
        for o in outs:
            assert np.all(np.isfinite(_np(o)))
            _check_mean(_np(o), ref, x, [i for i in range(k) if i != r], k, f"mean K={k}")


# ---------------------------------------------------------------------------------------------
# hostile rows through ops.krum_into
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def benign_dist(dev):
    """Device distances of the exact rows themselves (the hostile rows put back): computed once."""
    from myfyp_amd import ops

    cache = {}

    def get(k, n, packed):
        if (k, n, packed) not in cache:
            x = R.exact_rows(k, n, ties=True)
            cache[k, n, packed] = _np(ops.krum_into(_rows(x, dev, packed), [], [1.0] * k, 1, 3)[0])
        return cache[k, n, packed]

    return get


@pytest.mark.parametrize("k", [5, 8, 16])
def test_hostile_rows(dev, benign_dist, k):
    from myfyp_amd import ops

    cases = [c for c in R.HOSTILE_KRUM if c[0] == k]
    assert any(R.hostile_b(c[3], c[4]) <= c[1] for c in cases) and any(R.hostile_b(c[3], c[4]) > c[1] for c in cases)
    for idx, (_, f, m, kind, b, n) in enumerate(cases):
        what = f"K={k} f={f} m={m} {kind} b={b} n={n}"
        x, bad = R.hostile(R.exact_rows(k, n, ties=True), kind, b)
        honest = [i for i in range(k) if i not in bad]
        w = [1.0] * k if idx % 2 == 0 else [float(1 + (3 * i) % 5) for i in range(k)]
        packed = idx % 4 >= 2
        ref = R.krum(x, w, f, m)
        rows = _rows(x, dev, packed)
        rejected = [i for i in bad if i not in ref["chosen"]] + [i for i in honest if i not in ref["chosen"]]
        outs = [rows[ref["chosen"][0]], rows[rejected[0]]]  # alias a chosen and a rejected row
        dist, score, coef = (_np(t) for t in ops.krum_into(rows, outs, w, f, m))
        # every entry in the oracle's class: finite and bit-equal, +inf, or NaN
        _assert_bits(dist, ref["dist"], "dist " + what)
        assert np.array_equal(dist, dist.T, equal_nan=True) and np.all(np.diag(dist) == 0)
        # no NaN or inf leaks across pairs: honest-to-honest is what the benign rows give
        hh = np.ix_(honest, honest)
        assert np.array_equal(dist[hh], benign_dist(k, n, packed)[hh]), what
        _assert_bits(score, ref["score"], "score " + what)
        _assert_bits(coef, ref["coef"], "coef " + what)
        assert sorted(np.flatnonzero(coef != 0)) == ref["chosen"], what
        if len(bad) <= f:
            assert np.all(coef[bad] == 0), what
            for o in outs:
                o = _np(o)
                assert np.all(np.isfinite(o)), what
                _check_mean(o, ref, x, honest, m, "mean " + what)


# ---------------------------------------------------------------------------------------------
# trimmed mean and median
# ---------------------------------------------------------------------------------------------
def _run_trimmed(x, trim, dev, packed):
    from myfyp_amd import ops

    k, n = x.shape
    rows = _rows(x, dev, packed)
    outs = [rows[0], rows[k - 1]] if k > 1 else [rows[0], torch.empty(n, device=dev)]  # alias two of the rows
    ops.trimmed_mean_into(rows, outs, trim)
    return [_np(o) for o in outs]


def _run_median(x, dev, packed):
    from myfyp_amd import ops

    k, n = x.shape
    rows = _rows(x, dev, packed)
    outs = [torch.empty(n, device=dev), rows[k // 2]]
    ops.median_into(rows, outs)
    return [_np(o) for o in outs]


def _check_sorts(x, dev, trims, what):
    """Trimmed mean for every trim of trims, and the median, in both layouts, against the oracle."""
    for packed in (False, True):
        for trim in trims:
            want = R.trimmed_mean(x, trim)
            for o in _run_trimmed(x, trim, dev, packed):
                _assert_bits(o, want, f"trimmed {what} trim={trim} packed={packed}")
        want = R.median(x)
        for o in _run_median(x, dev, packed):
            _assert_bits(o, want, f"median {what} packed={packed}")


@pytest.mark.parametrize("k", range(1, 17))
def test_trimmed_mean_and_median_exact(dev, k):
    for n in TRIM_NS:
        _check_sorts(R.trim_rows(k, n), dev, range((k - 1) // 2 + 1), f"K={k} n={n}")
    for trim, n in TRIM_EXTRA.get(k, []):
        x = R.trim_rows(k, n)
        want = R.trimmed_mean(x, trim)
        for o in _run_trimmed(x, trim, dev, packed=True):
            _assert_bits(o, want, f"trimmed K={k} n={n} trim={trim}")


@pytest.mark.parametrize("k", [3, 5, 8, 16])
def test_trimmed_mean_infinite_rows(dev, k):
    """a rows of +inf and c rows of −inf: with at most trim at each end the output is finite and
    exact; with more it is ±inf, or NaN when both signs are kept, as the oracle says."""
    n = 1001
    tmax = (k - 1) // 2
    for a, c in [(1, 0), (0, 1), (1, 1), (tmax, tmax), (tmax + 1, 0), (0, tmax + 1), (2, 1)]:
        if a + c > k:
            continue
        x = np.array(R.trim_rows(k, n))
        idx = R.bad_rows(k, a + c, seed=a)
        x[idx[:a]] = np.inf
        x[idx[a:]] = -np.inf
        for trim in range(tmax + 1):
            want = R.trimmed_mean(x, trim)
            if a <= trim and c <= trim:
                assert np.all(np.isfinite(want))
            elif a > trim and c > trim:
                assert np.all(np.isnan(want))
            else:
                assert np.all(want == (np.inf if a > trim else -np.inf))
        _check_sorts(x, dev, range(tmax + 1), f"K={k} +inf rows {a} −inf rows {c}")


@pytest.mark.parametrize("k", [2, 3, 4, 5, 8, 15, 16])
def test_nan_sorts_last(dev, k):
    """The hostile family and NaNs scattered per coordinate, at most trim of them and more: the
    device equals the oracle under NaN-last ordering (a NaN is trimmed first, and the output is NaN
    exactly where one is kept)."""
    n = 1001
    tmax = (k - 1) // 2
    base = R.trim_rows(k, n)
    for kind in R.KINDS:
        if kind == "nan_second_trip":
            continue
        for b in sorted({1, max(1, tmax), min(k, tmax + 1)}):
            if R.hostile_b(kind, b) > k:
                continue
            x, _ = R.hostile(base, kind, b)
            _check_sorts(x, dev, range(tmax + 1), f"K={k} {kind} b={b}")
    for per in sorted({1, max(1, tmax), min(k, tmax + 1), k}):
        x = R.scatter_nans(base, per)
        want = R.median(x)
        assert np.all(np.isnan(want)) == (per > tmax)  # K = 2 with one NaN: the median is NaN
        _check_sorts(x, dev, range(tmax + 1), f"K={k} {per} NaN per coordinate")


def test_nan_second_trip(dev):
    """One NaN at a coordinate that only the second grid-stride trip of n = 524291 reaches."""
    k = 5
    x, bad = R.hostile(R.trim_rows(k, BIG), "nan_second_trip", 1)
    assert np.isnan(x[bad[0], R.SECOND_TRIP])
    for trim in (0, 1, 2):
        want = R.trimmed_mean(x, trim)
        assert np.isnan(want[R.SECOND_TRIP]) == (trim == 0) and np.isnan(want).sum() == (trim == 0)
        for o in _run_trimmed(x, trim, dev, packed=False):
            _assert_bits(o, want, f"trimmed second trip trim={trim}")
    want = R.median(x)
    for o in _run_median(x, dev, packed=True):
        _assert_bits(o, want, "median second trip")


def test_one_answer_for_nan_1_5(dev):
    """(NaN, 1, 5): 5 on the device, as on the host (tests/test_robust_ref_cpu.py)."""
    x = np.array([[np.nan], [1.0], [5.0]], dtype=np.float32)
    assert [float(o[0]) for o in _run_median(x, dev, False)] == [5.0, 5.0]
    assert [float(o[0]) for o in _run_trimmed(x, 1, dev, False)] == [5.0, 5.0]


# ---------------------------------------------------------------------------------------------
# entry points
# ---------------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments(dev):
    from myfyp_amd.ops import _native

    lib = _native.load(required=True)
    n = 64
    rows = [torch.zeros(n, device=dev) for _ in range(17)]
    out = torch.zeros(n, device=dev)
    work = torch.zeros(int(lib.myfyp_krum_grid(n, 16)) * 120, device=dev)
    dist = torch.zeros(256, dtype=torch.float64, device=dev)
    score = torch.zeros(16, dtype=torch.float64, device=dev)
    coef = torch.zeros(16, device=dev)
    src = ctypes.cast((ctypes.c_uint64 * 17)(*[r.data_ptr() for r in rows]), ctypes.c_void_p)
    dst = ctypes.cast((ctypes.c_uint64 * 17)(*[out.data_ptr()] * 17), ctypes.c_void_p)
    w = ctypes.cast((ctypes.c_float * 17)(*[1.0] * 17), ctypes.c_void_p)
    stream = torch.cuda.current_stream().cuda_stream

    def krum(k=4, p=1, n_=n, work_=work.data_ptr(), dist_=dist.data_ptr(), score_=score.data_ptr(), coef_=coef.data_ptr()):
        return lib.myfyp_krum_multi(dst, p, src, w, k, 1, 3, n_, work_, dist_, score_, coef_, stream)

    def trimmed(k=4, p=1, trim=1, n_=n):
        return lib.myfyp_trimmed_mean_multi(dst, p, src, k, trim, n_, stream)

    assert krum() == 0 and trimmed() == 0
    assert krum(k=0) == 2 and krum(k=17) == 2 and krum(p=17) == 2 and krum(n_=0) == 2
    assert krum(work_=None) == 2 and krum(dist_=None) == 2 and krum(score_=None) == 2 and krum(coef_=None) == 2
    assert trimmed(k=0) == 2 and trimmed(k=17) == 2 and trimmed(p=17) == 2 and trimmed(n_=0) == 2
    assert trimmed(trim=-1) == 2 and trimmed(trim=2) == 2 and trimmed(k=5, trim=3) == 2 and trimmed(k=1, trim=1) == 2
    torch.cuda.synchronize()
