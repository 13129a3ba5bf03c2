"""The float64 oracle of the colluding attacks (``tests/_collude_ref.py``) against brute force, the
fp32 emulation of the kernels' per-coordinate arithmetic against the bounds
``tests/test_collude_kernels_gpu.py`` derives (on exactly that file's inputs), ``alie_z`` against
the paper's table, and what the attacks are for: Krum picks the crafted row, not a sign-flipped one.
"""

import numpy as np
import pytest

import _collude_ref as cr
from _collude_ref import BIG, BIG_H, EPS, HS, KINDS, NS, Z


def _rows(h, n, seed):
    return np.stack([r.double().numpy() for r in cr.close_rows(h, n, seed)])


@pytest.mark.parametrize("kind", ["min_max", "min_sum"])
@pytest.mark.parametrize("h,n", [(2, 5), (3, 64), (6, 1027), (13, 3073), (16, 257)])
def test_closed_form_gamma_against_bisection(kind, h, n):
    x = _rows(h, n, 11 + h)
    st = cr.stats(x)
    g = cr.gamma_of(st, kind)
    assert g > 0
    assert abs(g - cr.gamma_bisect(x, kind)) <= 1e-9 * g
    lhs, rhs = cr.constraint(x, st["mu"] - g * st["sigma"], kind)
    assert abs(lhs - rhs) <= 1e-12 * rhs  # the binding constraint is met with equality
    assert abs(st["b"].sum()) <= 1e-12 * np.sqrt(st["a"].sum() * st["s"]) * h
    assert abs(st["a"].sum() - h * st["s"]) <= 1e-12 * h * st["s"]
    # a_i <= ((H−1)/H)² D: the discriminant's lower bound
    assert (st["a"] <= ((h - 1) / h) ** 2 * st["D"] * (1 + 1e-12)).all()
    disc = st["b"] ** 2 + st["s"] * (st["D"] - st["a"])
    assert (disc >= st["s"] * st["D"] * (2 * h - 1) / h**2 * (1 - 1e-12)).all()


@pytest.mark.parametrize("kind", ["min_max", "min_sum"])
def test_degenerate_rows_give_gamma_zero(kind):
    one = _rows(1, 33, 3)
    m, g, st = cr.oracle(one, kind)
    assert g == 0.0 and np.array_equal(m, one[0])
    same = np.repeat(one, 4, axis=0)
    m, g, st = cr.oracle(same, kind)
    assert g == 0.0 and st["s"] == 0.0 and np.array_equal(m, one[0])


def test_alie_z_table():
    from myfyp_amd import ops

    for (k, f), want in {(8, 2): 0.0, (16, 3): 0.09656, (16, 7): 0.76471, (50, 12): 0.33604}.items():
        assert abs(cr.alie_z(k, f) - want) <= 5e-6
        assert ops.alie_z(k, f) == pytest.approx(cr.alie_z(k, f), abs=1e-15)
    assert ops.alie_z(4, 4) == 0.0 and ops.alie_z(3, 2) == 0.0  # the fraction is not inside (0, 1)


def test_ipm_and_alie_definitions():
    x = _rows(5, 40, 8)
    r = x[0] + 1e-3
    m, g, st = cr.oracle(x, "ipm", eps=0.5, ref=r)
    np.testing.assert_allclose(m, -0.5 * x.mean(axis=0) + 1.5 * r, rtol=0, atol=1e-15)
    m, g, st = cr.oracle(x, "alie", n_out=3)
    assert g == cr.alie_z(8, 3)
    np.testing.assert_allclose(m, x.mean(axis=0) - g * x.std(axis=0), rtol=0, atol=1e-15)


def _emulation_case(kind, h, n):
    x, x64, ref, st = cr.case(h, n)
    x32 = x.numpy()
    r, be, bd, bs = cr.coord_bounds(x64)
    e, delta, sigma = cr.emulate_coord(x32)
    assert (np.abs(e.astype(np.float64) - (x64 - st["mu"])) <= be).all()
    assert (np.abs(delta.astype(np.float64) - (st["mu"] - x64[0])) <= bd).all()
    assert (np.abs(sigma.astype(np.float64) - st["sigma"]) <= bs).all()
    g64 = cr.gamma_of(st, kind) if kind in ("min_max", "min_sum") else 0.0
    ca, cb, c_r = cr.coefs(kind, float(np.float32(g64)))
    ref32 = ref.numpy() if kind == "ipm" else None
    ref64 = ref.double().numpy() if kind == "ipm" else None
    m = cr.emulate_write(x32, ca, cb, c_r, ref32)
    cb64 = -g64 if kind in ("min_max", "min_sum") else cb  # γ unrounded: its float32 rounding is dgamma
    m64 = ca * st["mu"] + cb64 * st["sigma"] + (c_r * ref64 if kind == "ipm" else 0.0)
    bound = cr.out_bound(x64, st, ca, cb, c_r, ref64, dgamma=cr.U * g64)
    assert (np.abs(m.astype(np.float64) - m64) <= bound).all()
    return float((np.abs(m.astype(np.float64) - m64) / bound).max())


@pytest.mark.parametrize("kind", KINDS)
def test_fp32_emulation_stays_inside_the_bounds(kind):
    worst = max(_emulation_case(kind, h, n) for h in HS for n in NS)
    worst = max(worst, _emulation_case(kind, BIG_H, BIG))
    assert worst <= 1.0


def test_rounding_mu_would_break_the_bound():
    """``x_k − fl(mean)`` with the mean formed from the raw fp32 values has an error of u·|x|, not of
    u·R: the bound of e_k tells the two forms apart."""
    h, n = 8, 3073
    x, x64, _, st = cr.case(h, n)
    _, be, _, _ = cr.coord_bounds(x64)
    mu32 = x.numpy().mean(axis=0, dtype=np.float32)
    naive = x.numpy() - mu32
    assert (np.abs(naive.astype(np.float64) - (x64 - st["mu"])) > be).any()


def _krum_case(h, a, n, seed):
    g = np.random.default_rng(seed)
    x = g.standard_normal(n) + 1e-3 * g.standard_normal((h, n))  # every honest row the same spread
    out = {}
    for kind, z in (("min_max", None), ("min_sum", None), ("alie", 1.0)):
        m, _, _ = cr.oracle(x, kind, n_out=a, z=z)
        out[kind] = cr.krum_choice(np.concatenate([x, np.repeat(m[None], a, axis=0)]), a)
    flipped = np.repeat(-x[:1], a, axis=0)
    out["sign_flip"] = cr.krum_choice(np.concatenate([x, flipped]), a)
    return out


@pytest.mark.parametrize("h,a,n", [(6, 2, 1027), (13, 3, 3073)])
def test_krum_picks_the_crafted_row_not_the_flipped_one(h, a, n):
    """Honest rows base + 1e-3·N(0, 1): with f = the attackers, Krum's choice is an attacker's row
    under min-max, min-sum and ALIE (z = 1), and an honest one under a sign flip. A property of the
    inputs and the definitions: no code of the package runs here."""
    got = _krum_case(h, a, n, seed=21 + h)
    assert got["min_max"] >= h and got["min_sum"] >= h and got["alie"] >= h
    assert got["sign_flip"] < h


def test_emulated_fma_is_fused():
    a, b, c = np.float32(1 + 2.0**-12), np.float32(1 - 2.0**-12), np.float32(-1.0)
    assert cr._fma32(a, b, c) == np.float32(-(2.0**-24))  # a·b rounds to 1 in fp32: an unfused form gives 0
