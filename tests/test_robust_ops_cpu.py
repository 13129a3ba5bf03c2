"""``ops.trimmed_mean_into`` and ``ops.krum_into`` on CPU tensors (the torch reference path, which
is the oracle of ``tests/test_robust_kernels_gpu.py``) against float64 numpy written out here with
the formulas of ``_math.trimmed_mean`` and ``Krum.aggregate``."""

import numpy as np
import pytest
import torch

from myfyp_amd import ops

N = 37


def _rows(k, seed=0, close=False):
    g = torch.Generator().manual_seed(seed)
    if not close:
        return [torch.randn(N, generator=g) for _ in range(k)]
    base = torch.randn(N, generator=g)
    return [base + 1e-3 * (1 + 0.15 * i) * torch.randn(N, generator=g) for i in range(k)]


def _krum_numpy(x, w, f, m):
    """``Krum.aggregate`` in float64 with the distances formed from differences."""
    k = len(x)
    d = np.array([[((x[i] - x[j]) ** 2).sum() for j in range(k)] for i in range(k)])
    cnt = max(1, k - f - 2)
    scores = np.array([np.sort(np.delete(d[i], i))[:cnt].sum() for i in range(k)])
    chosen = np.argsort(scores, kind="stable")[: max(1, min(m, k))]
    coef = np.zeros(k)
    coef[chosen] = np.asarray(w, dtype=np.float64)[chosen] / sum(w[i] for i in chosen)
    return d, scores, coef, sum(coef[i] * x[i] for i in chosen)


@pytest.mark.parametrize("k", [1, 2, 3, 5, 16])
def test_trimmed_mean_into_cpu(k):
    rows = _rows(k, seed=k)
    x = np.stack([r.double().numpy() for r in rows])
    for trim in sorted({0, 1 if k > 2 else 0, (k - 1) // 2}):
        want = np.sort(x, axis=0)[trim : k - trim].mean(axis=0)
        outs = [torch.empty(N), rows[0].clone()]
        ops.trimmed_mean_into(rows, outs, trim)
        for o in outs:
            np.testing.assert_allclose(o.double().numpy(), want, rtol=0, atol=k * 2.0**-24 * np.abs(x).max())


def test_trimmed_mean_into_aliases_and_rejects_a_large_trim():
    rows = _rows(5, seed=3)
    x = np.stack([r.double().numpy() for r in rows])
    ops.trimmed_mean_into(rows, [rows[0], rows[3]], 1)  # outputs are two of the inputs
    want = np.sort(x, axis=0)[1:4].mean(axis=0)
    np.testing.assert_allclose(rows[0].double().numpy(), want, rtol=0, atol=1e-6)
    np.testing.assert_allclose(rows[3].double().numpy(), want, rtol=0, atol=1e-6)
    with pytest.raises(ValueError):
        ops.trimmed_mean_into(_rows(4), [torch.empty(N)], 2)
    with pytest.raises(ValueError):
        ops.trimmed_mean_into(_rows(1), [torch.empty(N)], 1)


# (f, m): m = 1 (classic Krum), m > K, K - f - 2 <= 0 (f large), and the harness's f = 1, m = 3
@pytest.mark.parametrize("k", [1, 2, 3, 5, 16])
@pytest.mark.parametrize("f,m", [(0, 1), (1, 3), (1, 100), (50, 2)])
def test_krum_into_cpu(k, f, m):
    rows = _rows(k, seed=10 + k, close=True)
    if k >= 3:
        rows[k // 2] = -rows[k // 2]  # a sign-flipped peer
    w = [float(1 + (3 * i) % 5) for i in range(k)]
    x = [r.double().numpy() for r in rows]
    d, scores, coef, mean = _krum_numpy(x, w, f, m)
    out = torch.empty(N)
    dist_t, score_t, coef_t = ops.krum_into(rows, [out], w, f, m)
    assert dist_t.dtype == torch.float64 and score_t.dtype == torch.float64 and coef_t.dtype == torch.float32
    np.testing.assert_allclose(dist_t.numpy(), d, rtol=1e-12, atol=0)
    np.testing.assert_allclose(score_t.numpy(), scores, rtol=1e-12, atol=0)
    np.testing.assert_array_equal(coef_t.numpy() != 0, coef != 0)
    np.testing.assert_allclose(coef_t.numpy(), coef, rtol=2.0**-23, atol=0)
    np.testing.assert_allclose(out.double().numpy(), mean, rtol=0, atol=max(1, min(m, k)) * 2.0**-23 * np.abs(np.stack(x)).max())
    if k >= 5 and m < k - 1:
        assert coef_t[k // 2] == 0  # the flipped peer is never among the chosen


def test_krum_into_selection_only_and_ties():
    rows = _rows(5, seed=2, close=True)
    before = [r.clone() for r in rows]
    _, score, coef = ops.krum_into(rows, [], [1.0] * 5, 1, 3)
    assert all(torch.equal(a, b) for a, b in zip(rows, before))
    assert int((coef != 0).sum()) == 3 and abs(float(coef.sum()) - 1.0) < 1e-6
    # identical rows: every score ties, the lower indices win
    same = [torch.ones(N) for _ in range(4)]
    _, score, coef = ops.krum_into(same, [], [1.0, 2.0, 3.0, 4.0], 1, 2)
    assert score.tolist() == [0.0] * 4
    np.testing.assert_allclose(coef.numpy(), [1 / 3, 2 / 3, 0, 0], rtol=1e-6)


def test_host_krum_takes_torch_parameters():
    """``Krum.aggregate`` on torch parameters scores through ``ops.krum_into`` and selects what the
    numpy path selects on the same values."""
    from myfyp_amd.learning.aggregators import Krum
    from myfyp_amd.learning.aggregators._math import flatten, trimmed_mean

    rows = _rows(6, seed=4, close=True)
    rows[2] = -rows[2]
    params = [[r[:30].reshape(5, 6), r[30:]] for r in rows]
    x = [flatten(p).double().numpy() for p in params]
    _, _, coef, _ = _krum_numpy(x, [1.0] * 6, 1, 3)
    _, score, coef_t = ops.krum_into([flatten(p) for p in params], [], [1.0] * 6, 1, 3)
    np.testing.assert_array_equal(coef_t.numpy() != 0, coef != 0)
    assert Krum.collective_kind == "krum"
    tm = trimmed_mean(params, 0.2)
    want = np.sort(np.stack(x), axis=0)[1:5].mean(axis=0)
    np.testing.assert_allclose(np.concatenate([t.double().numpy().ravel() for t in tm]), want, rtol=0, atol=1e-6)
    assert tm[0].shape == (5, 6)
