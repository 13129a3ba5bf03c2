"""The float64 DnC oracle (``tests/_dnc_ref.py``) pinned on the CPU: the eigenpair by repeated
squaring against ``numpy.linalg.eigh``, −½·J·D·J against the explicitly centred Gram matrix, the
tile rule, min-max rows (DnC removes exactly the attackers where Krum picks one), and an fp32
emulation of the slab sums inside the bound the kernel tests use."""

import math

import numpy as np
import pytest

import _collude_ref as cref
import _dnc_ref as ref

# (K, f, n, seed, gs): min-max rows proper (gs = 1) where two or more of K >= 8 collude; a lone attacker, or
# K <= 5, shows in the top direction only when it goes gs times as far
MINMAX = [(8, 2, 3000, 0, 1.0), (11, 3, 2048, 1, 1.0), (16, 4, 4099, 0, 1.0), (16, 2, 777, 0, 1.0)]
FAMILIES = MINMAX + [(3, 1, 1000, 0, 3.0), (5, 1, 257, 0, 3.0), (8, 1, 1000, 1, 3.0)]


@pytest.mark.parametrize("k,f,n,seed,gs", FAMILIES)
def test_eigenpair_matches_eigh(k, f, n, seed, gs):
    x, _ = ref.attacked(k, f, n, seed, gs)
    g = ref.gram(ref.sqdist(x))
    ratio = ref.eig_ratio(g)
    assert ratio <= 0.9, ratio
    lam, u = ref.top_eig(g)
    ev, vec = np.linalg.eigh(g)
    v = vec[:, -1] * np.sign(vec[:, -1] @ u)
    assert abs(lam - ev[-1]) <= 1e-12 * ev[-1]
    assert np.abs(u - v).max() <= 1e-10
    assert abs((u * u).sum() - 1) <= 1e-14


def test_eigenpair_degenerate():
    assert ref.top_eig(np.zeros((4, 4))) == (0.0, pytest.approx(np.zeros(4)))
    lam, u = ref.top_eig(np.diag([3.0, 1.0, 0.0]))
    assert lam == pytest.approx(3.0) and np.abs(u).tolist() == pytest.approx([1.0, 0.0, 0.0])


@pytest.mark.parametrize("k,f,n,seed,gs", FAMILIES)
def test_double_centring_is_the_centred_gram(k, f, n, seed, gs):
    x = ref.attacked(k, f, n, seed, gs)[0].astype(np.float64)
    c = x - x.mean(axis=0)
    want = c @ c.T
    got = ref.gram(ref.sqdist(x))
    assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()
    # the score is the squared projection on the top right singular vector
    lam, u = ref.top_eig(got)
    _, sv, vt = np.linalg.svd(c, full_matrices=False)
    assert lam == pytest.approx(sv[0] ** 2, rel=1e-9)
    assert lam * u * u == pytest.approx((c @ vt[0]) ** 2, rel=1e-6, abs=1e-9 * lam)


def test_splitmix64_known_values():
    # the published test vector of splitmix64 seeded with 0: the first output is sm64(0)
    assert ref.sm64(0) == 0xE220A8397B1DCDAF
    assert ref.sm64(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4


def test_tile_mask():
    n, b = 1_000_003, 10000
    tiles = -(-n // 256)
    p = b / n
    seen = []
    for rnd in (0, 1):
        for t in (0, 1, 2):
            every, key, thr, forced, mask = ref.tile_plan(n, 7, rnd, t, b)
            assert not every and mask.shape == (tiles,) and mask[forced]
            assert thr == (b << 64) // n and forced == ref.sm64(key ^ ref.M64) % tiles
            # Bernoulli(p) per tile: within 5 standard deviations, plus the forced tile
            assert abs(int(mask.sum()) - p * tiles) <= 5 * math.sqrt(tiles * p * (1 - p)) + 1
            seen.append(mask)
    for i in range(len(seen)):
        for j in range(i + 1, len(seen)):
            assert not np.array_equal(seen[i], seen[j])  # another iteration, another round: another subsample
    assert np.array_equal(ref.tile_plan(n, 7, 1, 2, b)[4], seen[-1])  # and a function of (seed, round, t) only
    for nn, bb in [(10000, 10000), (5, 10000), (123456, None)]:
        every, _, _, _, mask = ref.tile_plan(nn, 7, 0, 0, bb)
        assert every and mask.all() and len(mask) == -(-nn // 256)
    # p so small that nothing passes the hash: the forced tile alone
    every, _, _, forced, mask = ref.tile_plan(3000, 3, 0, 0, 1)
    assert not every and mask.sum() >= 1 and mask[forced]
    assert ref.coord_mask(1000, 3, 0, 0, 300).shape == (1000,)


@pytest.mark.parametrize("k,f,n,seed,gs", MINMAX)
@pytest.mark.parametrize("b", [None, 600])
def test_dnc_removes_exactly_the_min_max_attackers(k, f, n, seed, gs, b):
    x, bad = ref.attacked(k, f, n, seed, gs)
    honest = [i for i in range(k) if i not in bad]
    # the crafted row meets min-max's constraint: a distance-based defence sees nothing unusual ...
    lhs, rhs = cref.constraint(x[honest].astype(np.float64), x[bad[0]].astype(np.float64), "min_max")
    assert lhs <= rhs * (1 + 1e-5)
    # ... Krum with the same f selects a crafted row (tests/test_collude_ref_cpu.py), and DnC removes them
    assert cref.krum_choice(x, f) in bad
    res = ref.dnc(x, [1.0] * k, f, 1.0, 1, b, seed=1, rnd=0)
    assert sorted(np.flatnonzero(res["removed"] >= 0).tolist()) == bad
    assert ref.margin(res["score"][0], f) >= 2.0
    assert res["coef"][bad].tolist() == [0.0] * f and res["coef"].sum() == pytest.approx(1.0, rel=1e-6)
    want = x[honest].astype(np.float64).mean(axis=0)
    assert np.abs(res["out"] - want).max() <= 1e-6 * np.abs(want).max()


def test_iterations_intersect():
    k, f, n = 16, 2, 4099
    x, bad = ref.attacked(k, f, n, 0)
    res = ref.dnc(x, list(range(1, k + 1)), f, 1.0, 3, 600, seed=2, rnd=5)
    gone = np.flatnonzero(res["removed"] >= 0)
    assert set(bad) <= set(gone.tolist()) and len(gone) <= 3 * f
    assert all(res["removed"][i] == 0 for i in bad)  # the first iteration already removes them
    kept = res["removed"] < 0
    w = np.arange(1, k + 1, dtype=np.float64)
    assert res["coef"] == pytest.approx(np.where(kept, w / w[kept].sum(), 0).astype(np.float32), rel=1e-7)


@pytest.mark.parametrize("k,f,n,seed,gs", FAMILIES)
@pytest.mark.parametrize("b", [None, 600])
def test_fp32_slab_sums_stay_inside_the_bound(k, f, n, seed, gs, b):
    """The distances of an fp32 emulation of the slab sums are within DIST_RTOL of float64, and the
    scores and λ they give are within the bounds derived from that."""
    x, _ = ref.attacked(k, f, n, seed, gs)
    mask = ref.tile_plan(n, 1, 0, 0, b)[4]
    d64 = ref.sqdist(x.astype(np.float64)[:, np.repeat(mask, 256)[:n]])
    d32 = ref.emulate_dist32(x, mask)
    off = d64 > 0
    assert (np.abs(d32 - d64)[off] / d64[off]).max() <= ref.DIST_RTOL
    s64, lam64, _, u, g = ref.scores(d64)
    s32, lam32, _, _, _ = ref.scores(d32)
    b_lam, b_s = ref.bounds(d64, g, lam64, u)
    worst = max(abs(lam32 - lam64) / b_lam, float((np.abs(s32 - s64) / b_s).max()))
    print(f"K={k} f={f} n={n} b={b}: worst error over bound {worst:.3e}")
    assert abs(lam32 - lam64) <= b_lam and (np.abs(s32 - s64) <= b_s).all()
