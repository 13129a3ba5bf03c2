"""``ops.collude_into`` off the GPU: the float64 torch path against the numpy oracle
(``tests/_collude_ref.py``), its argument checks and the degenerate cases."""

import numpy as np
import pytest
import torch

import _collude_ref as cr
from myfyp_amd import ops


def _rows(h, n, seed):
    return cr.close_rows(h, n, seed)


@pytest.mark.parametrize("kind", cr.KINDS)
@pytest.mark.parametrize("h,p,n", [(2, 1, 5), (5, 3, 257), (8, 2, 1027), (16, 1, 64)])
def test_against_the_oracle(kind, h, p, n):
    rows = _rows(h, n, 3 + h)
    keep = [r.clone() for r in rows]
    ref = rows[0] + 1e-3
    outs = [torch.full((n,), float("nan")) for _ in range(p)]
    gamma, stat = ops.collude_into(rows, outs, kind, ref=ref if kind == "ipm" else None)
    x64 = torch.stack(rows).double().numpy()
    m, g, st = cr.oracle(x64, kind, n_out=p, ref=ref.double().numpy())
    assert gamma.dtype == torch.float32 and gamma.shape == (1,) and stat.dtype == torch.float64 and stat.shape == (2 * h + 3,)
    assert abs(float(gamma[0]) - g) <= 2.0**-23 * abs(g)  # one float32 rounding of γ
    for o in outs:
        assert torch.equal(o, outs[0])
        np.testing.assert_allclose(o.double().numpy(), m, rtol=0, atol=2.0**-23 * np.abs(m).max())  # one float32 rounding of m
    for r, k0 in zip(rows, keep):
        assert torch.equal(r, k0)
    if kind in ("min_max", "min_sum"):
        want = np.concatenate([st["a"], st["b"], [st["s"], st["D"], st["S"]]])
        np.testing.assert_allclose(stat.numpy(), want, rtol=1e-9, atol=1e-12 * np.sqrt(st["a"].max() * st["s"]))
        lhs, rhs = cr.constraint(x64, outs[0].double().numpy(), kind)
        assert lhs <= rhs * (1 + 1e-4)
    else:
        assert not stat.any()


def test_explicit_z_and_default_z():
    rows = _rows(6, 33, 1)
    out = [torch.empty(33), torch.empty(33)]
    gamma, _ = ops.collude_into(rows, out, "alie")
    assert float(gamma[0]) == pytest.approx(ops.alie_z(8, 2))
    gamma, _ = ops.collude_into(rows, out, "alie", z=1.25)
    assert float(gamma[0]) == 1.25
    x = torch.stack(rows).double()
    want = x.mean(dim=0) - 1.25 * x.std(dim=0, unbiased=False)
    np.testing.assert_allclose(out[0].double().numpy(), want.numpy(), rtol=0, atol=2.0**-23 * float(want.abs().max()))


def test_argument_errors():
    rows = _rows(3, 9, 2)
    out = [torch.empty(9)]
    with pytest.raises(ValueError, match="unknown colluding attack"):
        ops.collude_into(rows, out, "sign_flip")
    with pytest.raises(ValueError, match="at least one honest row"):
        ops.collude_into([], out, "alie")
    with pytest.raises(ValueError, match="ipm needs ref"):
        ops.collude_into(rows, out, "ipm")
    with pytest.raises(ValueError, match="also an honest row"):
        ops.collude_into(rows, [torch.empty(9), rows[1]], "min_max")
    with pytest.raises(ValueError, match="share one length"):
        ops.collude_into(rows, [torch.empty(8)], "min_max")
    assert all(torch.isfinite(r).all() for r in rows)


@pytest.mark.parametrize("kind", ["min_max", "min_sum", "alie"])
def test_one_honest_row_and_equal_rows(kind):
    row = _rows(1, 17, 4)[0]
    for rows in ([row], [row.clone() for _ in range(4)]):
        out = torch.empty(17)
        gamma, stat = ops.collude_into(rows, [out], kind, z=1.0)
        assert torch.equal(out, row)  # σ = 0: m = μ
        if kind != "alie":
            assert float(gamma[0]) == 0.0 and float(stat[2 * len(rows)]) == 0.0


def test_twenty_rows_take_the_torch_path(monkeypatch):
    from myfyp_amd.ops import _native

    def boom(*a, **k):
        raise AssertionError("the native library was asked for")

    monkeypatch.setattr(_native, "load", boom)
    rows = _rows(20, 65, 6)
    out = torch.empty(65)
    gamma, stat = ops.collude_into(rows, [out], "min_max")
    x64 = torch.stack(rows).double().numpy()
    m, g, _ = cr.oracle(x64, "min_max")
    assert stat.shape == (43,) and abs(float(gamma[0]) - g) <= 2.0**-23 * g
    np.testing.assert_allclose(out.double().numpy(), m, rtol=0, atol=2.0**-23 * np.abs(m).max())
