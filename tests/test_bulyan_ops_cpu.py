"""``ops.bulyan_into`` off the GPU (the torch oracle) and ``bulyan_numpy``: the definition, checked
against a plain per-coordinate loop, and the properties a user relies on.

Bulyan: θ = K − 2f rows picked by iterated Krum, then per coordinate the mean of the β = K − 4f
picked values closest to their median (a window of the sorted values).
"""

import numpy as np
import pytest
import torch

from myfyp_amd import ops
from myfyp_amd.learning.aggregators import Bulyan
from myfyp_amd.learning.aggregators.bulyan import bulyan_numpy
from myfyp_amd.learning.dataset.synthetic import synthetic_mnist
from myfyp_amd.learning.frameworks.torch import TorchModel
from myfyp_amd.models import MLP

CASES = [(3, 0, 5), (7, 1, 33), (8, 1, 1001), (11, 2, 257), (16, 3, 64)]


def _loop(x, f):
    """The definition as a plain loop over float32 rows x [K, n]: (out, pick)."""
    k, n = x.shape
    theta, beta = k - 2 * f, k - 4 * f
    d = np.zeros((k, k))
    for i in range(k):
        for j in range(k):
            d[i, j] = sum((float(a) - float(b)) ** 2 for a, b in zip(x[i], x[j])) if i != j else 0.0
    remaining, pick = list(range(k)), [-1] * k
    for it in range(theta):
        r = len(remaining)
        if r == 1:
            best = remaining[0]
        else:
            cnt = min(max(r - f - 2, 1), r - 1)
            best, best_score = None, None
            for i in remaining:
                score = sum(sorted(d[i, j] for j in remaining if j != i)[:cnt])
                if best is None or score < best_score:
                    best, best_score = i, score
        pick[best] = it
        remaining.remove(best)
    out = np.zeros(n, dtype=np.float32)
    for c in range(n):
        v = sorted(np.float32(x[i, c]) for i in range(k) if pick[i] >= 0)
        m = v[(theta - 1) // 2] if theta % 2 else np.float32(0.5) * (v[theta // 2 - 1] + v[theta // 2])
        best_s, best_cost = 0, None
        for s in range(2 * f + 1):
            cost = max(np.float32(m - v[s]), np.float32(v[s + beta - 1] - m))
            if best_cost is None or cost < best_cost:
                best_s, best_cost = s, cost
        acc = np.float32(v[best_s])
        for j in range(1, beta):
            acc = np.float32(acc + v[best_s + j])
        out[c] = acc / np.float32(beta)
    return out, pick


def _rows(x):
    return [torch.from_numpy(np.ascontiguousarray(r)) for r in x]


@pytest.mark.parametrize("k,f,n", CASES)
def test_oracles_match_a_plain_loop(k, f, n):
    x = np.random.default_rng(100 * k + f).standard_normal((k, n)).astype(np.float32)
    want, pick = _loop(x, f)
    out, coef, pk, dist, score = bulyan_numpy(list(x), f)
    assert pk.tolist() == pick and pk.dtype == np.int32
    assert np.array_equal(out, want) and out.dtype == np.float32
    assert np.array_equal(coef, np.where(np.array(pick) >= 0, np.float32(1) / np.float32(k - 2 * f), np.float32(0)))
    o = torch.empty(n)
    d, s, c, p = ops.bulyan_into(_rows(x), [o], f)
    assert p.tolist() == pick and p.dtype == torch.int32 and c.dtype == torch.float32
    assert np.array_equal(o.numpy(), want)
    assert np.array_equal(c.numpy(), coef)
    np.testing.assert_allclose(d.numpy(), dist, rtol=1e-13)
    np.testing.assert_allclose(s.numpy(), score, rtol=1e-13)
    # outs may be empty: the selection only
    d2, s2, c2, p2 = ops.bulyan_into(_rows(x), [], f)
    assert torch.equal(d2, d) and torch.equal(s2, s) and torch.equal(c2, c) and torch.equal(p2, p)


def test_window_is_the_beta_values_closest_to_the_median():
    """On inputs without a cost tie the window rule equals an argsort of |v − m|."""
    rng = np.random.default_rng(0)
    for k, f in [(7, 1), (8, 1), (11, 2), (15, 3), (16, 3)]:
        x = rng.standard_normal((k, 3073)).astype(np.float32)
        out, _, pick, _, _ = bulyan_numpy(list(x), f)
        theta, beta = k - 2 * f, k - 4 * f
        v = np.sort(x[pick >= 0], axis=0)
        m = v[(theta - 1) // 2] if theta % 2 else np.float32(0.5) * (v[theta // 2 - 1] + v[theta // 2])
        costs = np.stack([np.maximum(m - v[s], v[s + beta - 1] - m) for s in range(2 * f + 1)])
        two = np.sort(costs, axis=0)[:2]
        assert (two[0] < two[1]).all(), (k, f)  # no tie between the two cheapest windows
        dev = np.abs(v - m)
        nearest = np.sort(np.argsort(dev, axis=0, kind="stable")[:beta], axis=0)
        far = np.sort(dev, axis=0)
        assert (far[beta - 1] < far[beta]).all(), (k, f)  # nor at the edge of the nearest set
        chosen = np.take_along_axis(v, nearest, axis=0)  # ascending: v is sorted and so are the indices
        acc = chosen[0].copy()
        for j in range(1, beta):
            acc = acc + chosen[j]
        assert np.array_equal(out, acc / np.float32(beta)), (k, f)


def test_single_coordinate_attack():
    """The attacker is the honest mean plus 0.5·√D·σ in coordinate 0: closer to the honest models
    than they are to each other. Classic Krum returns its row; Bulyan's error in that coordinate
    stays within the honest spread."""
    k, f, d, sigma = 7, 1, 4096, 1e-3
    rng = np.random.default_rng(7)
    honest = rng.standard_normal((k - 1, d)) * sigma
    mean = honest.mean(0)
    attacker = mean.copy()
    attacker[0] += 0.5 * np.sqrt(d) * sigma
    x = np.vstack([honest, attacker]).astype(np.float32)
    out = torch.empty(d)
    _, _, coef = ops.krum_into(_rows(x), [out], [1.0] * k, f, 1)
    assert coef.tolist() == [0.0] * (k - 1) + [1.0]
    krum_err = abs(float(out[0]) - mean[0])
    assert abs(krum_err - 0.5 * np.sqrt(d) * sigma) < 1e-6  # 0.032: the attacker's error
    ops.bulyan_into(_rows(x), [out], f)
    spread = np.abs(x[: k - 1, 0].astype(np.float64) - mean[0]).max()
    err = abs(float(out[0]) - mean[0])
    print(f"krum error {krum_err:.3e}, bulyan error {err:.3e}, largest honest deviation {spread:.3e}")
    assert err <= spread


@pytest.mark.parametrize("k", [1, 2, 3, 8, 16, 19])
def test_f_zero_is_the_mean_of_all_rows(k):
    x = np.random.default_rng(k).standard_normal((k, 37)).astype(np.float32)
    out = torch.empty(37)
    _, _, coef, pick = ops.bulyan_into(_rows(x), [out], 0)
    assert sorted(pick.tolist()) == list(range(k))
    assert np.array_equal(coef.numpy(), np.full(k, np.float32(1) / np.float32(k)))
    # θ = β = K: one window, the sorted values summed in fp32
    np.testing.assert_allclose(out.numpy().astype(np.float64), x.astype(np.float64).mean(0), rtol=0, atol=k * 2.0**-24 * np.abs(x).max())


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf"), 3e38])
@pytest.mark.parametrize("k,f", [(7, 1), (11, 2), (16, 3)])
def test_non_finite_rows_are_never_picked(k, f, bad):
    x = np.random.default_rng(5).standard_normal((k, 65)).astype(np.float32)
    rows = list(range(1, 1 + 2 * f, 2))  # f rows
    for i, r in enumerate(rows):
        if i % 2:
            x[r, 3] = bad  # one coordinate
        else:
            x[r] = bad  # the whole row
    out = torch.empty(65)
    _, _, coef, pick = ops.bulyan_into(_rows(x), [out], f)
    assert torch.isfinite(out).all()
    assert all(float(coef[r]) == 0.0 and int(pick[r]) == -1 for r in rows)
    assert int((coef != 0).sum()) == k - 2 * f
    out_np, coef_np, _, _, _ = bulyan_numpy(list(x), f)
    assert np.array_equal(out_np, out.numpy()) and np.array_equal(coef_np, coef.numpy())


def test_equal_rows_tie_towards_the_lower_index():
    row = np.random.default_rng(1).standard_normal(19).astype(np.float32)
    x = np.stack([row] * 7)
    _, _, coef, pick = ops.bulyan_into(_rows(x), [], 1)
    assert pick.tolist() == [0, 1, 2, 3, 4, -1, -1]
    assert np.array_equal(coef.numpy(), np.array([0.2] * 5 + [0.0] * 2, dtype=np.float32))
    assert bulyan_numpy(list(x), 1)[2].tolist() == [0, 1, 2, 3, 4, -1, -1]


@pytest.mark.parametrize("k,f,n", CASES)
def test_score_and_dist_are_krums(k, f, n):
    x = np.random.default_rng(k).standard_normal((k, n)).astype(np.float32)
    d, s, _, _ = ops.bulyan_into(_rows(x), [], f)
    kd, ks, _ = ops.krum_into(_rows(x), [], [1.0] * k, f, 1)
    assert torch.equal(d, kd) and torch.equal(s, ks)


def test_argument_errors():
    x = _rows(np.zeros((6, 4), dtype=np.float32))
    with pytest.raises(ValueError, match=r"4f \+ 3.*K = 6.*f = 1"):
        ops.bulyan_into(x, [], 1)
    with pytest.raises(ValueError, match="K = 6"):
        bulyan_numpy([r.numpy() for r in x], 1)
    with pytest.raises(ValueError, match="f = -1"):
        ops.bulyan_into(x, [], -1)
    with pytest.raises(ValueError):
        bulyan_numpy([r.numpy() for r in x], -1)
    with pytest.raises(ValueError, match="length"):
        ops.bulyan_into(x[:2] + [torch.zeros(5)], [], 0)
    with pytest.raises(ValueError, match="length"):
        ops.bulyan_into(x[:3], [torch.zeros(3)], 0)
    with pytest.raises(ValueError, match="length"):
        bulyan_numpy([np.zeros(4), np.zeros(4), np.zeros(3)], 0)
    with pytest.raises(ValueError):
        Bulyan(num_byzantine=-1)
    ops.bulyan_into(_rows(np.zeros((7, 4), dtype=np.float32)), [], 1)  # K = 4f + 3 is admitted


def _models(k, numpy_params, seed=3):
    data = synthetic_mnist(40, 10)
    g = torch.Generator().manual_seed(seed)
    base = MLP(hidden_sizes=[6], seed=0)
    models = []
    for i in range(k):
        m = TorchModel(MLP(hidden_sizes=[6], seed=0))
        params = [p + 1e-3 * torch.randn(p.shape, generator=g) * (-500 if i == 2 else 1) for p in base.state_dict().values()]
        params = [p.numpy() for p in params] if numpy_params else params
        models.append(m.build_copy(params=params, num_samples=10 + i, contributors=[f"n{i}"]))
    del data
    return models


def test_numpy_and_torch_aggregator_paths_agree():
    k = 7
    agg_np, agg_t = Bulyan(num_byzantine=1), Bulyan(num_byzantine=1)
    got_np = agg_np.aggregate(_models(k, True))
    models_t = _models(k, False)
    flats = [torch.cat([torch.as_tensor(p).reshape(-1).float() for p in m.get_parameters()]) for m in models_t]
    out = torch.empty_like(flats[0])
    _, _, coef, _ = ops.bulyan_into(flats, [out], 1)
    got_t = agg_t.aggregate(models_t)
    a = np.concatenate([np.asarray(p, dtype=np.float32).ravel() for p in got_np.get_parameters()])
    b = np.concatenate([np.asarray(p, dtype=np.float32).ravel() for p in got_t.get_parameters()])
    assert np.array_equal(a, b)
    assert np.array_equal(b, out.numpy())
    for agg in (agg_np, agg_t):
        addrs, c = agg.last_selection
        assert addrs == [f"n{i}" for i in range(k)]
        assert np.array_equal(np.asarray(c), coef.numpy())
        assert float(np.asarray(c)[2]) == 0.0  # the outlier is rejected
    assert got_np.get_num_samples() == sum(10 + i for i in range(k))
    assert got_np.get_contributors() == [f"n{i}" for i in range(k)]
    with pytest.raises(ValueError, match=r"K = 6.*f = 1"):
        Bulyan(num_byzantine=1).aggregate(_models(6, True))
