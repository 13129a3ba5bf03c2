"""``ops.geometric_median_into`` on CPU tensors (the float64 torch oracle of the definition in its
docstring) against an independent float64 numpy loop, its mathematical properties, the NaN rules,
and the host aggregator ``GeometricMedian`` on numpy and torch-CPU models."""

import numpy as np
import pytest
import torch

from myfyp_amd import ops
from myfyp_amd.learning.aggregators import GeometricMedian
from myfyp_amd.learning.frameworks.torch import TorchModel
from myfyp_amd.models import MLP


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _close_rows(k, n, seed, flipped=5):
    """Peers that start from one model: rows differ by ~1e-3 of their norm; one is sign-flipped."""
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(n, generator=g)
    rows = [base + 1e-3 * (1 + 0.15 * i) * torch.randn(n, generator=g) for i in range(k)]
    if flipped is not None and flipped < k:
        rows[flipped] = -base
    return rows


def _loop_ref(x, w, iters, nu):
    """The definition, written once more: plain float64 numpy over finite rows."""
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    k = len(x)
    c = (w / w.sum()).astype(np.float32)
    obj = []
    for _ in range(iters):
        r = int(np.flatnonzero(c)[0])
        z = x[r].copy()
        for j in range(k):
            if c[j] != 0:
                z = z + np.float64(c[j]) * (x[j] - x[r])
        d = np.sqrt(((x - z) ** 2).sum(axis=1))
        obj.append(float((w * d).sum()))
        beta = w / np.maximum(nu, d)
        c = (beta / beta.sum()).astype(np.float32)
    out = sum(np.float64(c[j]) * x[j] for j in range(k))
    return out, c, d, np.array(obj)


@pytest.mark.parametrize("k,n,iters", [(2, 7, 3), (5, 33, 1), (8, 1001, 3), (16, 257, 6)])
def test_oracle_matches_numpy_loop(k, n, iters):
    rows = _close_rows(k, n, seed=k)
    w = [float(1 + (3 * i) % 7) for i in range(k)]
    out = torch.empty(n)
    coef, dist, obj = ops.geometric_median_into(rows, [out], w, iters=iters, nu=1e-6)
    assert coef.dtype == torch.float32 and dist.dtype == torch.float64 and obj.dtype == torch.float64
    assert coef.shape == (k,) and dist.shape == (k,) and obj.shape == (iters,)
    want, c_ref, d_ref, o_ref = _loop_ref(torch.stack(rows).numpy(), w, iters, 1e-6)
    np.testing.assert_allclose(dist.numpy(), d_ref, rtol=1e-9)
    np.testing.assert_allclose(obj.numpy(), o_ref, rtol=1e-9)
    np.testing.assert_allclose(coef.numpy(), c_ref, rtol=2.0**-22)
    np.testing.assert_allclose(out.double().numpy(), want, rtol=0, atol=1e-6 * float(np.abs(want).max()))
    assert abs(float(coef.double().sum()) - 1) < 1e-6


def test_objective_non_increasing():
    for k, n in ((5, 33), (8, 1001)):
        rows = _close_rows(k, n, seed=3)
        w = [float(1 + i) for i in range(k)]
        obj = ops.geometric_median_into(rows, [], w, iters=12)[2].numpy()
        assert np.all(obj[1:] <= obj[:-1] * (1 + 1e-12)), obj


def test_single_row_returns_it():
    x = _randn(37, 1)
    out = torch.empty(37)
    coef, dist, obj = ops.geometric_median_into([x], [out], [3.0], iters=2)
    assert coef.tolist() == [1.0] and dist.tolist() == [0.0] and obj.tolist() == [0.0, 0.0]
    assert torch.equal(out, x)


def test_two_equal_rows_stay_at_the_midpoint():
    a, b = _randn(50, 2), _randn(50, 3)
    out = torch.empty(50)
    coef, dist, _ = ops.geometric_median_into([a, b], [out], [2.0, 2.0], iters=5)
    assert coef.tolist() == [0.5, 0.5]
    half = 0.5 * float((a.double() - b.double()).norm())
    np.testing.assert_allclose(dist.numpy(), [half, half], rtol=1e-12)
    np.testing.assert_allclose(out.double().numpy(), (0.5 * (a.double() + b.double())).numpy(), rtol=0, atol=1e-6)


def test_equilateral_triangle_lands_on_the_centroid():
    """The geometric median of an equilateral triangle is its centroid. A point at offset e from
    the centroid of a unit triangle sees distances that differ by at least 1.5·|e| (to first
    order), so the spread of the oracle's own ``dist`` bounds how far it stands from the centroid;
    on top of that the float32 coefficients and the float32 output round at 2^-24 of max|x|."""
    off = torch.tensor([5.0, -3.0, 2.0], dtype=torch.float64)
    tri = torch.tensor([[1.0, 0.0, 0.0], [-0.5, 3**0.5 / 2, 0.0], [-0.5, -(3**0.5) / 2, 0.0]], dtype=torch.float64) + off
    rows = [t.float() for t in tri]
    x64 = torch.stack(rows).double()
    cen = x64.mean(0)
    out = torch.empty(3)
    coef, dist, obj = ops.geometric_median_into(rows, [out], [1.0, 1.0, 1.0], iters=32)
    own = float(dist.max() - dist.min())
    err = float((out.double() - cen).norm())
    print(f"triangle: |out - centroid| {err:.3e}, oracle's distance spread {own:.3e}")
    assert err <= own + 8 * 2.0**-24 * float(x64.abs().max())
    assert np.all(np.diff(obj.numpy()) <= 1e-12)
    # a slightly heavier vertex moves the median by the order of the extra weight, no further
    out2 = torch.empty(3)
    ops.geometric_median_into(rows, [out2], [1.0, 1.0, 1.001], iters=32)
    assert float((out2.double() - cen).norm()) < 2e-3


def test_breakdown_point():
    """3 of 8 rows replaced by 1e3·randn: the geometric median stays within the honest rows'
    spread of their mean, the weighted mean does not. From the mean, ~3000 away, a step divides
    the distance to the honest cluster by about 3 (the outliers' share of Σβ): 32 steps arrive."""
    k, n = 8, 200
    rows = _close_rows(k, n, seed=11, flipped=None)
    for i, j in enumerate((1, 4, 6)):
        rows[j] = 1e3 * _randn(n, 50 + i)
    honest = torch.stack([rows[i] for i in range(k) if i not in (1, 4, 6)]).double()
    hmean = honest.mean(0)
    spread = float((honest - hmean).norm(dim=1).max())
    out = torch.empty(n)
    coef, _, _ = ops.geometric_median_into(rows, [out], [1.0] * k, iters=32)
    mean = torch.stack(rows).double().mean(0)
    assert float((out.double() - hmean).norm()) <= spread
    assert float((mean - hmean).norm()) > 100 * spread
    assert float(coef[[1, 4, 6]].sum()) < 1e-4


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), 3e38])
def test_non_finite_row_gets_coefficient_zero(bad):
    """A NaN row, an Inf row, and a row whose sum of squares overflows float32."""
    k, n = 5, 40
    rows = _close_rows(k, n, seed=4, flipped=None)
    rows[2] = rows[2].clone()
    rows[2][7] = bad
    out = torch.empty(n)
    coef, dist, obj = ops.geometric_median_into(rows, [out], [1.0, 2.0, 50.0, 3.0, 4.0], iters=3)
    assert float(coef[2]) == 0.0
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(obj).all())
    keep = [0, 1, 3, 4]
    out_k = torch.empty(n)
    coef_k, _, obj_k = ops.geometric_median_into([rows[i] for i in keep], [out_k], [1.0, 2.0, 3.0, 4.0], iters=3)
    assert torch.equal(coef[keep], coef_k) and torch.equal(out, out_k) and torch.equal(obj, obj_k)


def test_every_row_nan_gives_nan():
    rows = [torch.full((9,), float("nan")) for _ in range(3)]
    out = torch.zeros(9)
    coef, dist, obj = ops.geometric_median_into(rows, [out], [1.0, 1.0, 2.0], iters=3)
    assert coef.tolist() == [0.25, 0.25, 0.5]
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(dist).all())


def test_zero_weights_count_as_equal():
    rows = _close_rows(4, 30, seed=6, flipped=None)
    a = ops.geometric_median_into(rows, [], [0.0] * 4, iters=3)
    b = ops.geometric_median_into(rows, [], [1.0] * 4, iters=3)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_argument_errors():
    rows = _close_rows(3, 10, seed=1, flipped=None)
    for iters in (0, 33, -1):
        with pytest.raises(ValueError, match="iters"):
            ops.geometric_median_into(rows, [], [1.0] * 3, iters=iters)
    with pytest.raises(ValueError, match="3 rows but 2 weights"):
        ops.geometric_median_into(rows, [], [1.0, 1.0])
    with pytest.raises(ValueError, match="nu"):
        ops.geometric_median_into(rows, [], [1.0] * 3, nu=0.0)
    with pytest.raises(ValueError, match="weights"):
        ops.geometric_median_into(rows, [], [1.0, -1.0, 1.0])
    with pytest.raises(ValueError, match="iters"):
        GeometricMedian(iters=40)


def test_outs_empty_gives_the_weights_only():
    rows = _close_rows(4, 30, seed=6)
    before = [r.clone() for r in rows]
    coef, _, _ = ops.geometric_median_into(rows, [], [1.0] * 4)
    assert coef.shape == (4,) and all(torch.equal(a, b) for a, b in zip(rows, before))


class _TensorModel:
    """What an aggregator reads of a model whose parameters are torch tensors."""

    def __init__(self, params, num_samples, contributors):
        self.params, self.num_samples, self.contributors = list(params), num_samples, list(contributors)

    def get_parameters(self):
        return self.params

    def get_num_samples(self):
        return self.num_samples

    def get_contributors(self):
        return self.contributors

    def build_copy(self, params, num_samples, contributors):
        return _TensorModel(params, num_samples, contributors)


def test_aggregator_numpy_and_torch_agree():
    base = TorchModel(MLP(hidden_sizes=[8, 8], seed=0))
    shapes = [np.asarray(p).shape for p in base.get_parameters()]
    n = sum(int(np.prod(s)) for s in shapes)
    rows = _close_rows(5, n, seed=8, flipped=3)
    samples = [10, 20, 30, 40, 50]

    def split(r):
        out, at = [], 0
        for s in shapes:
            sz = int(np.prod(s))
            out.append(r[at : at + sz].reshape(s).clone())
            at += sz
        return out

    names = [f"n{i}" for i in range(5)]
    np_models = [base.build_copy(params=[p.numpy() for p in split(r)], num_samples=s, contributors=[a]) for r, s, a in zip(rows, samples, names)]
    t_models = [_TensorModel(split(r), s, [a]) for r, s, a in zip(rows, samples, names)]
    agg_np, agg_t = GeometricMedian(iters=3), GeometricMedian(iters=3)
    got_np = agg_np.aggregate(np_models)
    got_t = agg_t.aggregate(t_models)
    assert got_np.get_num_samples() == got_t.get_num_samples() == sum(samples)
    assert got_np.get_contributors() == got_t.get_contributors() == names
    assert [tuple(p.shape) for p in got_t.get_parameters()] == [tuple(s) for s in shapes]
    assert all(isinstance(p, torch.Tensor) and p.dtype == torch.float32 for p in got_t.get_parameters())
    flat_np = np.concatenate([np.asarray(p, dtype=np.float64).ravel() for p in got_np.get_parameters()])
    flat_t = torch.cat([p.double().reshape(-1) for p in got_t.get_parameters()]).numpy()
    atol = 2.0**-23 * float(np.abs(flat_np).max())  # both results are float32 roundings of one float64 vector
    np.testing.assert_allclose(flat_np, flat_t, rtol=0, atol=atol)
    want, c_ref, _, _ = _loop_ref(torch.stack(rows).numpy(), samples, 3, 1e-6)
    np.testing.assert_allclose(flat_np, want, rtol=0, atol=atol)
    assert agg_np.last_weights[0] == names == agg_t.last_weights[0]
    c_np = np.asarray(agg_np.last_weights[1])
    np.testing.assert_array_equal(c_np, agg_t.last_weights[1].numpy())
    np.testing.assert_allclose(c_np, c_ref, rtol=2.0**-22)
    assert c_np[3] < 0.1 * samples[3] / sum(samples)  # the flipped model is down-weighted (three steps, 27 % of the samples)
