"""The float64 ClippedGossip oracle (``tests/_clip_ref.py``) pinned on the CPU, and the package's
CPU implementations (``ops.clipped_gossip_into`` on CPU tensors, ``clipped_gossip_numpy``) against it."""

import numpy as np
import pytest
import torch

import _clip_ref as ref
from myfyp_amd import ops
from myfyp_amd.learning.aggregators import ClippedGossip, NeighborAvg
from myfyp_amd.learning.aggregators.clipped_gossip import clipped_gossip_numpy


def _full_matrix(w):
    """NeighborAvg's matrix of the shares w: the self share on the diagonal."""
    m = np.array(w, dtype=np.float64)
    np.fill_diagonal(m, 0.0)
    np.fill_diagonal(m, 1.0 - m.sum(1))
    return m


@pytest.mark.parametrize("topology", ["ring", "star", "full"])
def test_no_clipping_is_plain_mixing(topology):
    """b = 0 (τ = +inf) and a huge fixed τ: ``W_full @ x`` to float64 rounding."""
    k, n = 6, 257
    x = ref.close_rows(k, n, seed=1, far=(2,)).astype(np.float64)
    w = NeighborAvg(topology=topology).mixing_matrix(k)
    want = w @ x
    shares = w.copy()
    np.fill_diagonal(shares, 0.0)
    for kw in ({"b": 0}, {"tau": 1e30}):
        out, _, taus, _, w_eff = ref.clipped_gossip(x, shares, **kw)
        assert np.array_equal(w_eff, shares.astype(np.float32))
        assert np.all(taus == (np.inf if "b" in kw else 1e30))
        # the oracle mixes with float32 shares: compare with the same shares
        np.testing.assert_allclose(out, _full_matrix(w_eff.astype(np.float64)) @ x, rtol=0, atol=16 * 2.0**-53 * np.abs(x).max())
        np.testing.assert_allclose(out, want, rtol=0, atol=2.0**-24 * np.abs(x).max() * 11)  # float32(W) against W


@pytest.mark.parametrize("kw", [{"tau": 0.05}, {"b": 1}, {"b": 2}])
def test_moves_no_farther_than_the_radius(kw):
    k, n = 7, 301
    x = ref.close_rows(k, n, seed=2, far=(3,)).astype(np.float64)
    for w in (ref.ring(k), ref.star(k), ref.full(k)):
        out, d, taus, _, w_eff = ref.clipped_gossip(x, w, **kw)
        w32 = w.astype(np.float32).astype(np.float64)
        for p in range(k):
            moved = np.linalg.norm(out[p] - x[p])
            reach = sum(w32[p, q] * min(np.sqrt(d[p, q]), taus[p]) for q in ref.neighbours(w, p))
            assert moved <= reach * (1 + 1e-6), (p, moved, reach)
    # the far row pulls an honest ring neighbour by at most its share of the radius, not of the distance
    out, d, taus, _, _ = ref.clipped_gossip(x, ref.ring(k), **kw)
    assert np.linalg.norm(out[2] - x[2]) < 0.01 * np.sqrt(d[2, 3]) / 3


def test_nonfinite_rows_reach_no_finite_row():
    k, n = 6, 50
    x = ref.close_rows(k, n, seed=3).astype(np.float64)
    x[1, 7] = np.nan
    x[4, :] = np.inf
    for w in (ref.ring(k), ref.full(k)):
        for kw in ({"tau": 0.1}, {"b": 1}, {"b": 2}, {"b": 0}):
            out, d, taus, _, w_eff = ref.clipped_gossip(x, w, **kw)
            assert np.all(w_eff[:, 1] == 0) and np.all(w_eff[:, 4] == 0)
            assert np.all(w_eff[1] == 0) and np.all(w_eff[4] == 0)  # a non-finite row is left as it is
            assert np.array_equal(out[1], x[1], equal_nan=True) and np.array_equal(out[4], x[4])
            for p in (0, 2, 3, 5):
                assert np.isfinite(out[p]).all()
            # the same rows without the two: every finite row mixes only its finite neighbours
            keep = [0, 2, 3, 5]
            w_eff2 = w_eff[np.ix_(keep, keep)]
            np.testing.assert_array_equal(ref.mix(x[keep], w_eff2), out[keep])


def test_radius_zero_when_every_neighbour_may_be_hostile():
    k, n = 5, 33
    x = ref.close_rows(k, n, seed=4).astype(np.float64)
    out, _, taus, _, w_eff = ref.clipped_gossip(x, ref.ring(k), b=2)  # a ring row has two neighbours
    assert np.all(taus == 0) and not w_eff.any() and np.array_equal(out, x)
    out, _, taus, _, w_eff = ref.clipped_gossip(x, ref.star(k), b=1)  # a leaf has one, the hub four
    assert np.all(taus[1:] == 0) and taus[0] > 0 and not w_eff[1:].any() and np.array_equal(out[1:], x[1:])
    # a coincident neighbour (D = 0) is inside a radius of 0
    x[1] = x[0]
    _, _, _, _, w_eff = ref.clipped_gossip(x, ref.ring(k), tau=0.0)
    assert w_eff[0, 1] == np.float32(1.0 / 3.0) and w_eff[1, 0] == np.float32(1.0 / 3.0) and w_eff[0, 4] == 0


def test_tie_rule_higher_row_is_farther():
    # rows 1, 2, 3 at the same distance 4 from row 0, row 4 nearer
    x = np.zeros((5, 3))
    x[1, 0] = x[2, 1] = x[3, 2] = 2.0
    x[4, 0] = 1.0
    w = np.zeros((5, 5))
    w[0, 1:] = 0.2
    d = ref.sqdist(x)
    assert ref.aside(d, w, 0, 1) == [3] and ref.aside(d, w, 0, 2) == [2, 3] and ref.aside(d, w, 0, 3) == [1, 2, 3]
    _, _, taus, tau2s, w_eff = ref.clipped_gossip(x, w, b=2)
    assert tau2s[0] == pytest.approx((0.2 * 4 + 0.2 * 1) / 0.4)
    # a non-finite distance counts as the largest, and ties with another by index
    x[2, 1] = np.nan
    d = ref.sqdist(x)
    assert ref.aside(d, w, 0, 1) == [2]
    x[1, 0] = np.inf
    d = ref.sqdist(x)
    assert ref.aside(d, w, 0, 1) == [2] and ref.aside(d, w, 0, 2) == [1, 2]
    for kw in ({"b": 1}, {"b": 2}, {"tau": 1.0}):
        got = ops.clip_plan(d, w.astype(np.float32), kw.get("tau"), kw.get("b"))
        want = ref.plan(d, w.astype(np.float32), **kw)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[2])


@pytest.mark.parametrize("k", [2, 5, 16])
def test_fp32_emulation_stays_inside_the_bound(k):
    """The bound the GPU test uses holds for an fp32 emulation of the kernel's arithmetic."""
    for n, seed in ((5, 11), (1025, 12)):
        x32 = ref.close_rows(k, n, seed=seed, far=(1,))
        for w in (ref.ring(k), ref.full(k)):
            for kw in ({"tau": 0.02}, {"b": 1}, {"b": 0}):
                _, _, _, _, w_eff = ref.clipped_gossip(x32, w.astype(np.float32), **kw)
                got = ref.mix_f32(x32, w_eff).astype(np.float64)
                want = ref.mix(x32, w_eff)
                bound = ref.mix_bound(x32, w_eff)
                assert np.all(np.abs(got - want) <= bound)
                if k > 2 and "tau" in kw:
                    assert np.abs(got - want).max() > 0  # the emulation does round
                    assert bound.max() < 64 * ref.U * np.abs(x32).max() * 11  # and the bound is of rounding size


def _cases():
    for k, n, far in ((1, 9, ()), (2, 1, ()), (3, 4, (0,)), (6, 257, (2,)), (9, 64, (1, 6)), (17, 40, (5,))):
        x32 = ref.close_rows(k, n, seed=20 + k, far=far)
        for name, w in (("ring", ref.ring(k)), ("star", ref.star(k)), ("full", ref.full(k))):
            if k == 1:
                w = np.zeros((1, 1))
            for kw in ({"tau": 0.03}, {"b": 1}, {"b": 2}, {"b": 0}):
                yield k, n, name, x32, w.astype(np.float32), kw


def _same_plan(taus, w_eff, taus_ref, w_eff_ref, what):
    np.testing.assert_allclose(taus, taus_ref, rtol=1e-12, atol=0, err_msg=str(what))
    assert np.array_equal(w_eff != 0, w_eff_ref != 0), what
    np.testing.assert_allclose(w_eff, w_eff_ref, rtol=2.0**-23, atol=0, err_msg=str(what))


def test_ops_cpu_and_numpy_agree_with_the_oracle():
    """float64 math on both sides, which differ in the order of the distance sums only (n terms:
    n·2^-53 relative, far inside 1e-12): the radii agree to that, ``w_eff`` to one float32 rounding
    with the same zeros, the rows to float64 rounding (then rounded to the rows' float32 by ``ops``)."""
    for k, n, name, x32, w, kw in _cases():
        want, d, taus, _, w_eff = ref.clipped_gossip(x32, w, **kw)
        args = {"tau": kw.get("tau"), "num_byzantine": kw.get("b")}
        out, taus_n, w_eff_n, d_n = clipped_gossip_numpy(list(x32), w, **args)
        _same_plan(taus_n, w_eff_n, taus, w_eff, (k, n, name, kw))
        np.testing.assert_allclose(d_n, d, rtol=1e-14, atol=0)
        np.testing.assert_allclose(out, want, rtol=0, atol=1e-14 * np.abs(x32).max() * 11)
        rows = [torch.from_numpy(r.copy()) for r in x32]
        dist_t, tau_t, w_eff_t = ops.clipped_gossip_into(rows, w, **args)
        assert dist_t.dtype == torch.float64 and tau_t.dtype == torch.float64 and w_eff_t.dtype == torch.float32
        _same_plan(tau_t.numpy(), w_eff_t.numpy(), taus, w_eff, (k, n, name, kw))
        np.testing.assert_allclose(dist_t.numpy(), d, rtol=1e-14, atol=0)
        got = np.stack([r.numpy() for r in rows])
        written = w_eff.any(axis=1)
        assert np.array_equal(got[~written], x32[~written])
        np.testing.assert_allclose(got.astype(np.float64), want, rtol=0, atol=2.0**-24 * np.abs(want).max() * 1.01)


def test_argument_checks():
    rows = [torch.zeros(4), torch.ones(4)]
    w = ref.ring(2)
    for kw in ({}, {"tau": 1.0, "num_byzantine": 1}):
        with pytest.raises(ValueError, match="exactly one"):
            ops.clipped_gossip_into(rows, w, **kw)
    with pytest.raises(ValueError):
        ops.clipped_gossip_into(rows, -w, tau=1.0)
    with pytest.raises(ValueError):
        ops.clipped_gossip_into(rows, w, tau=-1.0)
    with pytest.raises(ValueError):
        ops.clipped_gossip_into(rows, w, num_byzantine=-1)
    with pytest.raises(ValueError):
        ops.clipped_gossip_into(rows, ref.ring(3), tau=1.0)
    assert torch.equal(rows[0], torch.zeros(4)) and torch.equal(rows[1], torch.ones(4))
    with pytest.raises(ValueError):
        ClippedGossip(tau=-1.0)
    with pytest.raises(ValueError):
        ClippedGossip(num_byzantine=-1)
    agg = ClippedGossip(topology="star", tau=0.5)
    assert agg.collective_kind == "neighbor" and agg.all_peers_train and agg.partial_aggregation is False
    assert agg.radius_args() == {"tau": 0.5} and ClippedGossip().radius_args() == {"num_byzantine": 1}
    assert np.array_equal(agg.mixing_matrix(5), NeighborAvg(topology="star").mixing_matrix(5))


def test_gossip_plane_aggregate_centres_on_the_own_model():
    from myfyp_amd.learning.frameworks.torch import TorchModel
    from myfyp_amd.models import MLP

    rng = np.random.default_rng(31)
    proto = TorchModel(MLP(hidden_sizes=[8, 8], seed=0))
    base = [np.asarray(p, dtype=np.float32) for p in proto.get_parameters()]
    models = []
    for i in range(4):
        scale = -10.0 if i == 3 else 1.0
        params = [(scale * b + 1e-3 * (1 + i) * rng.standard_normal(b.shape)).astype(b.dtype) for b in base]
        models.append(proto.build_copy(params=params, num_samples=10 + i, contributors=[f"n{i}"]))
    flat = np.stack([np.concatenate([np.asarray(p, dtype=np.float64).ravel() for p in m.get_parameters()]) for m in models])
    agg = ClippedGossip(node_name="n1", num_byzantine=1)
    out = agg.aggregate(models)
    order = [1, 0, 2, 3]  # the own model first
    w = np.zeros((4, 4), dtype=np.float32)
    w[0, 1:] = 0.25
    want, _, taus, _, w_eff = ref.clipped_gossip(flat[order], w, b=1)
    got = np.concatenate([np.asarray(p, dtype=np.float64).ravel() for p in out.get_parameters()])
    np.testing.assert_allclose(got, want[0], rtol=0, atol=2.0**-24 * np.abs(want[0]).max() * 1.01)
    addrs, tau_got, w_got = agg.last_clipping
    assert addrs == ["n1", "n0", "n2", "n3"] and w_got[0, 3] < 0.05 * w[0, 3] and w_got[0, 1] == w[0, 1]
    _same_plan(tau_got, w_got, taus, w_eff, "gossip")
    assert sorted(out.get_contributors()) == ["n0", "n1", "n2", "n3"] and out.get_num_samples() == 46
    assert np.linalg.norm(got - flat[1]) < 0.05 * np.linalg.norm(flat[3] - flat[1])  # the far model barely pulls
    # the own model is not among them: NeighborAvg's plain mean
    other = ClippedGossip(node_name="elsewhere").aggregate(models)
    plain = NeighborAvg(node_name="elsewhere").aggregate(models)
    for a, b in zip(other.get_parameters(), plain.get_parameters()):
        assert np.array_equal(np.asarray(a), np.asarray(b))
