"""``ops.dnc_into`` off the GPU (the torch oracle), ``ops.dnc_select`` / ``dnc_tiles`` / ``dnc_check``
and ``dnc_numpy`` against the float64 oracle of ``tests/_dnc_ref.py``, and the properties a user
relies on: the parameter errors, f = 0, the tie rule, the screen, ``removed`` / ``coef`` and the
``DnC`` aggregator on numpy and torch models."""

import numpy as np
import pytest
import torch

import _dnc_ref as ref
from myfyp_amd import ops
from myfyp_amd.learning.aggregators import DnC
from myfyp_amd.learning.aggregators.dnc import dnc_numpy
from myfyp_amd.learning.frameworks.torch import TorchModel
from myfyp_amd.models import MLP

# (K, f, n, seed, gs, iters, subsample_dims)
CASES = [(3, 1, 1000, 0, 3.0, 1, None), (5, 1, 257, 0, 3.0, 2, 100), (8, 2, 3000, 0, 1.0, 1, 600), (8, 2, 3000, 0, 1.0, 3, 600),
         (16, 4, 4099, 0, 1.0, 1, None), (16, 3, 4099, 0, 1.0, 3, 1000), (19, 4, 1500, 0, 1.0, 2, 500)]


def _rows(x):
    return [torch.from_numpy(np.array(r)) for r in x]


@pytest.mark.parametrize("k,f,n,seed,gs,iters,b", CASES)
def test_oracles_agree(k, f, n, seed, gs, iters, b):
    x, bad = ref.attacked(k, f, n, seed, gs)
    w = [float(10 + i) for i in range(k)]
    want = ref.dnc(x, w, f, 1.0, iters, b, seed=5, rnd=3)
    assert sorted(np.flatnonzero(want["removed"] >= 0).tolist()) == bad
    out = torch.empty(n)
    dist, score, lam, removed, coef = ops.dnc_into(_rows(x), [out], w, f, 1.0, iters, b, seed=5, round=3)
    assert dist.shape == (iters, k, k) and dist.dtype == torch.float64 and score.shape == (iters, k) and lam.shape == (iters,)
    assert removed.dtype == torch.int32 and coef.dtype == torch.float32
    np.testing.assert_allclose(dist.numpy(), want["dist"], rtol=1e-12)
    np.testing.assert_allclose(lam.numpy(), want["lam"], rtol=1e-9)
    np.testing.assert_allclose(score.numpy(), want["score"], rtol=1e-7, atol=1e-9 * want["lam"].max())
    assert removed.tolist() == want["removed"].tolist()
    assert np.array_equal(coef.numpy(), want["coef"])
    np.testing.assert_allclose(out.numpy(), want["out"], rtol=0, atol=2.0**-23 * np.abs(x).max())
    o_np, c_np, r_np, d_np, s_np, l_np = dnc_numpy(list(x), w, f, 1.0, iters, b, seed=5, round=3)
    assert r_np.tolist() == want["removed"].tolist() and r_np.dtype == np.int32
    assert np.array_equal(c_np, want["coef"]) and o_np.dtype == np.float32
    np.testing.assert_allclose(d_np, want["dist"], rtol=1e-12)
    np.testing.assert_allclose(l_np, want["lam"], rtol=1e-9)
    np.testing.assert_allclose(s_np, want["score"], rtol=1e-7, atol=1e-9 * want["lam"].max())
    assert np.array_equal(o_np, out.numpy())
    # outs may be empty: the selection only
    again = ops.dnc_into(_rows(x), [], w, f, 1.0, iters, b, seed=5, round=3)
    assert all(torch.equal(p, q) for p, q in zip(again, (dist, score, lam, removed, coef)))


def test_tiles_follow_the_rule():
    for n, b, iters in [(4099, 600, 3), (100000, 10000, 2), (257, 1, 8)]:
        keys, thr, forced, mask = ops.dnc_tiles(n, 9, 4, iters, b)
        assert mask.shape == (iters, -(-n // 256)) and mask.dtype == bool
        for t in range(iters):
            every, key, thr_, forced_, m_ = ref.tile_plan(n, 9, 4, t, b)
            assert not every and (keys[t], thr, forced[t]) == (key, thr_, forced_)
            assert np.array_equal(mask[t], m_)
    for n, b in [(10000, 10000), (12, 10000), (4099, None)]:
        keys, thr, forced, mask = ops.dnc_tiles(n, 9, 4, 2, b)
        assert mask.all() and keys == [0, 0] and forced == [0, 0] and thr == 2**64 - 1
    a = ops.dnc_tiles(100000, 9, 4, 1, 10000)[3]
    assert not np.array_equal(a, ops.dnc_tiles(100000, 9, 5, 1, 10000)[3])  # another round
    assert not np.array_equal(a, ops.dnc_tiles(100000, 8, 4, 1, 10000)[3])  # another seed
    assert ops.splitmix64(0) == 0xE220A8397B1DCDAF


def test_select_from_distances():
    x, bad = ref.attacked(8, 2, 3000, 0)
    d = ref.sqdist(x)
    score, lam, removed, coef = ops.dnc_select(d, [1.0] * 8, 2)
    s, l, scr, _, _ = ref.scores(d)
    np.testing.assert_allclose(score[0], s, rtol=1e-7, atol=1e-9 * l)
    assert lam[0] == pytest.approx(l, rel=1e-9) and sorted(np.flatnonzero(removed >= 0).tolist()) == bad
    assert np.array_equal(coef, np.where(removed < 0, np.float32(1 / 6), np.float32(0)))
    # two iterations that disagree: the union is removed, each with its first iteration
    d2 = np.stack([d, d[::-1, ::-1]])
    _, _, removed2, coef2 = ops.dnc_select(d2, [1.0] * 8, 2)
    mirrored = [7 - i for i in bad]
    assert [int(removed2[i]) for i in bad] == [0, 0] and all(int(removed2[i]) == 1 for i in mirrored if i not in bad)
    assert int((coef2 != 0).sum()) == 8 - len(set(bad) | set(mirrored))


@pytest.mark.parametrize("k", [1, 2, 3, 8, 16, 19])
def test_f_zero_is_the_weighted_mean(k):
    x = np.random.default_rng(k).standard_normal((k, 37)).astype(np.float32)
    w = [float(1 + i) for i in range(k)]
    out = torch.empty(37)
    _, score, lam, removed, coef = ops.dnc_into(_rows(x), [out], w, 0)
    assert removed.tolist() == [-1] * k
    wn = np.array(w) / sum(w)
    assert np.array_equal(coef.numpy(), wn.astype(np.float32))
    np.testing.assert_allclose(out.numpy().astype(np.float64), (wn[:, None] * x.astype(np.float64)).sum(0), rtol=0, atol=2.0**-22 * np.abs(x).max())
    # filter_frac 0 removes nothing either
    assert ops.dnc_into(_rows(x), [], w, 3, 0.0)[3].tolist() == [-1] * k


def test_identical_rows_tie_towards_the_higher_row():
    row = np.random.default_rng(1).standard_normal(19).astype(np.float32)
    x = np.stack([row] * 7)
    _, score, lam, removed, coef = ops.dnc_into(_rows(x), [], [1.0] * 7, 2)
    assert score.tolist() == [[0.0] * 7] and lam.tolist() == [0.0]
    assert removed.tolist() == [-1, -1, -1, -1, -1, 0, 0]
    assert np.array_equal(coef.numpy(), np.array([0.2] * 5 + [0.0] * 2, dtype=np.float32))
    assert dnc_numpy(list(x), [1.0] * 7, 2)[2].tolist() == removed.tolist()
    # filter_frac rounds up: ceil(0.5 · 3) = 2 rows per iteration, two iterations
    assert ops.dnc_into(_rows(x), [], [1.0] * 7, 3, 0.5, 2)[3].tolist() == [-1, -1, -1, -1, -1, 0, 0]


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
@pytest.mark.parametrize("whole", [True, False])
def test_a_non_finite_row_is_screened(bad, whole):
    x, att = ref.attacked(8, 2, 3000, 0)
    x = x.copy()
    victim = 5
    assert victim not in att
    if whole:
        x[victim] = bad
    else:
        x[victim, 17] = bad
    out = torch.empty(3000)
    w = [1.0] * 8
    dist, score, lam, removed, coef = ops.dnc_into(_rows(x), [out], w, 2, subsample_dims=None)
    assert torch.isfinite(out).all() and torch.isfinite(lam).all()
    assert float(score[0, victim]) == float("inf") and int(removed[victim]) == 0 and float(coef[victim]) == 0.0
    # the screened row counts towards m = 2: one more row goes, an attacker
    gone = np.flatnonzero(removed.numpy() >= 0).tolist()
    assert len(gone) == 2 and (set(gone) - {victim}) <= set(att)
    want = ref.dnc(x, w, 2, 1.0, 1, None)
    assert removed.tolist() == want["removed"].tolist() and np.array_equal(coef.numpy(), want["coef"])
    o_np, c_np, r_np, _, _, _ = dnc_numpy(list(x), w, 2, subsample_dims=None)
    assert r_np.tolist() == removed.tolist() and np.array_equal(c_np, coef.numpy()) and np.array_equal(o_np, out.numpy())


def test_more_screened_rows_than_m_all_go():
    x = ref.attacked(8, 2, 3000, 0)[0].copy()
    x[[0, 4, 6]] = float("nan")
    _, score, _, removed, coef = ops.dnc_into(_rows(x), [], [1.0] * 8, 1, subsample_dims=None)
    assert removed.tolist() == [0, -1, -1, -1, 0, -1, 0, -1]
    assert np.array_equal(coef.numpy(), np.where(removed.numpy() < 0, np.float32(0.2), np.float32(0)))


def test_all_rows_bad_fall_back_to_the_weighted_mean():
    x = np.full((4, 9), np.nan, dtype=np.float32)
    w = [1.0, 2.0, 3.0, 4.0]
    _, score, _, removed, coef = ops.dnc_into(_rows(x), [], w, 1)
    assert removed.tolist() == [0, 0, 0, 0] and bool(torch.isinf(score).all())
    assert np.array_equal(coef.numpy(), (np.array(w) / 10.0).astype(np.float32))
    assert np.array_equal(dnc_numpy(list(x), w, 1)[1], coef.numpy())


def test_argument_errors():
    x = _rows(np.zeros((6, 4), dtype=np.float32))
    w = [1.0] * 6
    for kw, word in [(dict(f=-1), "f = -1"), (dict(f=1.5), "integer"), (dict(f=1, filter_frac=-0.1), "filter_frac"),
                     (dict(f=1, filter_frac=float("nan")), "filter_frac"), (dict(f=1, filter_frac=float("inf")), "filter_frac"),
                     (dict(f=1, iters=0), "iters"), (dict(f=1, iters=9), "iters"), (dict(f=1, iters=1.5), "iters"),
                     (dict(f=1, subsample_dims=0), "subsample_dims"), (dict(f=1, subsample_dims=2.5), "subsample_dims"),
                     (dict(f=6), r"K = 6.*m = .* 6"), (dict(f=2, iters=3), r"K = 6, iters = 3"), (dict(f=1, filter_frac=6.0), "K = 6")]:
        with pytest.raises(ValueError, match=word):
            ops.dnc_into(x, [], w, **kw)
        kw = dict(kw)
        with pytest.raises(ValueError, match=word):
            ops.dnc_check(6, kw.pop("f"), kw.pop("filter_frac", 1.0), kw.pop("iters", 1), kw.pop("subsample_dims", 10000))
    with pytest.raises(ValueError, match="weights"):
        ops.dnc_into(x, [], w[:5], 1)
    with pytest.raises(ValueError, match="length"):
        ops.dnc_into(x[:2] + [torch.zeros(5)], [], [1.0] * 3, 0)
    with pytest.raises(ValueError, match="length"):
        ops.dnc_into(x[:3], [torch.zeros(3)], [1.0] * 3, 0)
    with pytest.raises(ValueError, match="K = 6"):
        dnc_numpy([r.numpy() for r in x], w, 6)
    for kw in (dict(num_byzantine=-1), dict(filter_frac=-1.0), dict(iters=0), dict(iters=9), dict(subsample_dims=0)):
        with pytest.raises(ValueError):
            DnC(**kw)
    assert ops.dnc_check(6, 5, 1.0, 1, None) == 5 and ops.dnc_check(7, 3, 0.5, 3, 1) == 2  # iters · m = K − 1 is admitted


def _models(k, numpy_params, seed=3):
    g = torch.Generator().manual_seed(seed)
    base = MLP(hidden_sizes=[6], seed=0)
    models = []
    for i in range(k):
        m = TorchModel(MLP(hidden_sizes=[6], seed=0))
        params = [p + 1e-3 * torch.randn(p.shape, generator=g) * (-500 if i == 2 else 1) for p in base.state_dict().values()]
        params = [p.numpy() for p in params] if numpy_params else params
        models.append(m.build_copy(params=params, num_samples=10 + i, contributors=[f"n{i}"]))
    return models


def test_numpy_and_torch_aggregator_paths_agree():
    k = 7
    agg_np, agg_t = DnC(num_byzantine=1, subsample_dims=2000, seed=4), DnC(num_byzantine=1, subsample_dims=2000, seed=4)
    assert agg_np.collective_kind == "dnc" and agg_np.partial_aggregation is False and agg_np.round == 0
    got_np = agg_np.aggregate(_models(k, True))
    models_t = _models(k, False)
    flats = [torch.cat([torch.as_tensor(p).reshape(-1).float() for p in m.get_parameters()]) for m in models_t]
    assert flats[0].numel() > 2000  # the subsample is a real one
    out = torch.empty_like(flats[0])
    coef = ops.dnc_into(flats, [out], [10.0 + i for i in range(k)], 1, subsample_dims=2000, seed=4, round=0)[4]
    got_t = agg_t.aggregate(models_t)
    a = np.concatenate([np.asarray(p, dtype=np.float32).ravel() for p in got_np.get_parameters()])
    b = np.concatenate([np.asarray(p, dtype=np.float32).ravel() for p in got_t.get_parameters()])
    assert np.array_equal(a, b)
    assert np.array_equal(b, out.numpy())
    for agg in (agg_np, agg_t):
        addrs, c = agg.last_selection
        assert addrs == [f"n{i}" for i in range(k)]
        assert np.array_equal(np.asarray(c), coef.numpy())
        assert float(np.asarray(c)[2]) == 0.0 and int((np.asarray(c) != 0).sum()) == k - 1  # the outlier is removed
    assert got_np.get_num_samples() == sum(10 + i for i in range(k))
    assert got_np.get_contributors() == [f"n{i}" for i in range(k)]
    with pytest.raises(ValueError, match=r"K = 2"):
        DnC(num_byzantine=2).aggregate(_models(2, True))


def test_clear_advances_the_round_and_the_subsample():
    agg = DnC(num_byzantine=1, subsample_dims=2000)
    agg.clear()
    agg.clear()
    assert agg.round == 2
    models = _models(7, True)
    flats = [np.concatenate([np.asarray(p, dtype=np.float32).ravel() for p in m.get_parameters()]) for m in models]
    agg.aggregate(models)
    ws = [10.0 + i for i in range(7)]
    d2 = dnc_numpy(flats, ws, 1, subsample_dims=2000, round=2)[3]
    d0 = dnc_numpy(flats, ws, 1, subsample_dims=2000, round=0)[3]
    assert not np.array_equal(d0, d2)  # another round measures other coordinates
    assert np.array_equal(np.asarray(agg.last_selection[1]), dnc_numpy(flats, ws, 1, subsample_dims=2000, round=2)[1])
