"""The geometric-median kernels of ``csrc/kernels/fl_ops.hip`` (``k_gm_dist<K>``, ``k_gm_reweight``,
then ``k_coef_mean<K>``) against float64 (MI355X only, except the emulation test, which is CPU).

One Weiszfeld step is checked at a time: the float64 reference is fed the coefficients the device
itself held before the step (``iters = t`` gives them: a call is deterministic), so the bounds
below are bounds of ONE step, not of an error that compounds.

Bound on a distance ``d_k = ‖x_k − z‖``, relative.

* The kernel never forms ``z``. Per coordinate it takes ``u_j = x_j − x_r`` (one rounding,
  ``2^-24·|u_j|``), ``m = Σ_j c_j u_j`` by at most K fused multiply-adds (each rounds at
  ``2^-24`` of a partial sum no larger than ``Σ c_j |u_j|``) and ``u_k − m`` (one more rounding).
  The error vector of ``x_k − z`` therefore has norm at most
  ``2^-24·[(K + 2)·Σ_j c_j ‖x_j − x_r‖ + 2·‖x_k − x_r‖]``, and ``|‖a + e‖ − ‖a‖| <= ‖e‖``:
  relative to ``d_k`` at most ``2(K + 2)·2^-24·(Σ_j c_j ‖x_j − x_r‖ + ‖x_k − x_r‖) / d_k``,
  computed below from float64.
* The sum of squares: every term is positive, so an fp32 addition chain of depth L is within
  ``(L + 3)·2^-24`` relative (the 3: the squares and the sum inside a group of four); the chain is
  one add per grid-stride step, 6 wave steps and 3 block steps, and the slab sum is in double.
  A relative error e of ``d²`` is e/2 of ``d``.

``objective`` is a positively weighted sum of the ``d_k``: within the largest of their bounds.
``coef_k = β_k / Σβ`` with ``β_k = ŵ_k / max(ν, d_k)``: within ``bound_k + max_j bound_j`` of the
reference's, plus the two float32 roundings of the coefficients themselves (``2^-23``), with 1 % for
the second-order terms. Output: K fused multiply-adds with coefficients that sum to 1:
``K·2^-24·max|x|``.

``test_bound_holds_for_fp32_emulation`` checks on the CPU, for exactly these inputs, that an fp32
emulation of the kernel's per-coordinate arithmetic stays inside the bound, and that the form
``x_k − Σ_j c_j x_j`` (z rounded to fp32) does not at (K = 2, n = 7): the bound can tell them apart.
"""

import functools

import numpy as np
import pytest
import torch

BIG = 524291  # 2048 * 256 + 3: the grid-stride loop runs more than once, and a tail
KS = [1, 2, 5, 8, 16]
NS = [1, 7, 1001, BIG]
NU = 1e-6
U = 2.0**-24


@pytest.fixture(scope="module")
def dev():
    from myfyp_amd.ops import _native

    _native.load(required=True)  # the native path must be the one under test
    return torch.device("cuda")


def _close_rows(k, n, seed, flipped=5):
    """Peers that start from one model: rows differ by ~1e-3 of their norm; one is sign-flipped."""
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(n, generator=g)
    rows = [base + 1e-3 * (1 + 0.15 * i) * torch.randn(n, generator=g) for i in range(k)]
    if flipped is not None and flipped < k:
        rows[flipped] = -base
    return rows


def _weights(k):
    return [float(1 + (3 * i) % 7) for i in range(k)]


def _flipped(k):
    """The flipped row where K > 3: row 5 as in ``_close_rows``, row 3 where there is no row 5."""
    return None if k <= 3 else (5 if k > 5 else 3)


@functools.lru_cache(maxsize=None)
def _case(k, n):
    """(rows fp32 [K, n], float64 copy): computed once, never written."""
    x = torch.stack(_close_rows(k, n, seed=40 + k, flipped=_flipped(k)))
    return x, x.double().numpy()


def _step64(x64, what, c):
    """One step of the definition in float64 from the float32 coefficients ``c``: d, objective,
    next coefficients (float64, unrounded), and the two norms the bound needs."""
    k = len(x64)
    c = np.asarray(c, dtype=np.float64)
    nz = [j for j in range(k) if c[j] != 0]
    r = nz[0]
    u = x64 - x64[r]
    m = np.zeros_like(x64[0])
    for j in nz:
        m += c[j] * u[j]
    d = np.sqrt(((u - m) ** 2).sum(axis=1))
    un = np.sqrt((u**2).sum(axis=1))
    beta = what / np.maximum(NU, d)
    return d, float((what * d).sum()), beta / beta.sum(), float((c * un).sum()), un


def _dist_bound(k, n, d, a, un):
    groups = (n + 3) // 4
    grid = min(512, max(1, -(-groups // 256)))
    depth = -(-groups // (grid * 256)) + 6 + 3
    chain = 0.5 * (depth + 3) * U
    with np.errstate(divide="ignore", invalid="ignore"):
        elem = np.where(d > 0, 2 * (k + 2) * U * (a + un) / d, 0.0)
    return chain + elem


def _coefs64(x64, w, iters):
    """float32 coefficients c^0 .. c^iters of the float64 definition."""
    what = np.asarray(w, dtype=np.float64)
    cs = [(what / what.sum()).astype(np.float32)]
    for _ in range(iters):
        cs.append(_step64(x64, what, cs[-1])[2].astype(np.float32))
    return cs


def _fma32(a, b, c):
    """fp32 fused multiply-add: the product of two floats is exact in double."""
    return (np.float64(a) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _emulate(x32, c, reference_row):
    """The per-coordinate fp32 arithmetic of ``k_gm_dist`` (or of the form that rounds z), the
    squares in fp32, their sum in double: the sum's own chain is the bound's other term."""
    k = len(x32)
    nz = [j for j in range(k) if c[j] != 0]
    if reference_row:
        u = x32 - x32[nz[0]]
        m = np.zeros_like(x32[0])
        for j in nz:
            m = _fma32(c[j], u[j], m)
        diff = u - m
    else:
        z = np.zeros_like(x32[0])
        for j in nz:
            z = _fma32(c[j], x32[j], z)
        diff = x32 - z
    return np.sqrt((diff * diff).astype(np.float64).sum(axis=1))


def test_bound_holds_for_fp32_emulation():
    worst = {True: 0.0, False: 0.0}
    rejected = {}
    for k in KS:
        for n in NS:
            x, x64 = _case(k, n)
            what = np.asarray(_weights(k))
            for c in _coefs64(x64, _weights(k), 2):  # the coefficients the three steps start from
                d, _, _, a, un = _step64(x64, what, c)
                bound = _dist_bound(k, n, d, a, un)
                for ref_row in (True, False):
                    got = _emulate(x.numpy(), c, ref_row)
                    with np.errstate(divide="ignore", invalid="ignore"):
                        rel = np.where(d > 0, np.abs(got - d) / d, np.abs(got))
                    worst[ref_row] = max(worst[ref_row], float(rel.max()))
                    if ref_row:
                        assert np.all(rel <= bound), (k, n, rel, bound)
                    elif np.any(rel > bound):
                        rejected[(k, n)] = float((rel / bound).max())
    print(f"fp32 emulation, worst relative error of d: reference-row {worst[True]:.2e}, z rounded {worst[False]:.2e}; "
          f"z-rounded form outside the bound at {sorted(rejected)}")
    assert (2, 7) in rejected, rejected


def _run(rows, outs, w, iters):
    from myfyp_amd import ops

    coef, dist, obj = ops.geometric_median_into(rows, outs, w, iters=iters, nu=NU)
    return coef.cpu().numpy(), dist.cpu().numpy(), obj.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_steps_against_float64(dev, k):
    w = _weights(k)
    what = np.asarray(w)
    fl = _flipped(k)
    for n in NS:
        x, x64 = _case(k, n)
        xd = x.to(dev)
        rows = [xd[i].clone() for i in range(k)]
        c_prev = (what / what.sum()).astype(np.float32)  # c^0: the same double division, rounded once
        objs = []
        for t in range(3):
            coef, dist, obj = _run(rows, [], w, t + 1)
            d, o, c_next, a, un = _step64(x64, what, c_prev)
            bound = _dist_bound(k, n, d, a, un)
            with np.errstate(divide="ignore", invalid="ignore"):
                rel = np.where(d > 0, np.abs(dist - d) / d, np.abs(dist))
            rel_o = abs(obj[t] - o) / o if o > 0 else abs(obj[t])
            tol_c = 1.01 * (bound + bound.max()) + 2 * U
            rel_c = np.abs(coef.astype(np.float64) - c_next) / c_next
            print(f"geomed K={k} n={n} step {t}: d rel err {rel.max():.2e} (worst err/bound {(rel / bound).max():.3f}), "
                  f"obj {rel_o:.2e} (bound {bound.max():.2e}), coef {rel_c.max():.2e} (worst err/bound {(rel_c / tol_c).max():.3f})")
            assert np.all(rel <= bound), (n, t, rel, bound)
            assert rel_o <= bound.max(), (n, t, rel_o)
            assert np.all(rel_c <= tol_c), (n, t, rel_c, tol_c)
            assert np.array_equal(obj[:t], np.array(objs)), (n, t)  # the earlier steps of a longer call: bit-equal
            objs.append(obj[t])
            c_prev = coef
        if fl is not None:
            share = w[fl] / sum(w)
            ref = _coefs64(x64, w, 3)[-1]
            assert ref[fl] < 0.01 * share, (ref[fl], share)  # the definition itself down-weights it
            print(f"geomed K={k} n={n}: flipped coefficient {coef[fl]:.2e} (float64 {ref[fl]:.2e}) of share {share:.3f}")
            assert coef[fl] < 0.01 * share, (n, coef[fl], share)
        # the outputs alias rows, a kept one and the flipped one among them
        alias = [0] if k == 1 else sorted({0, k - 1, fl if fl is not None else 1})
        coef_a, dist_a, obj_a = _run(rows, [rows[i] for i in alias], w, 3)
        assert np.array_equal(coef_a, coef) and np.array_equal(dist_a, dist) and np.array_equal(obj_a, obj)
        want = (coef.astype(np.float64)[:, None] * x64).sum(axis=0)
        atol = k * U * float(np.abs(x64).max())
        for i in alias:
            err = float(np.abs(rows[i].double().cpu().numpy() - want).max())
            print(f"geomed K={k} n={n}: out max err {err:.2e} (bound {atol:.2e})")
            assert err <= atol, (n, i, err, atol)


@pytest.mark.gpu
def test_unaligned_rows_bit_equal(dev):
    """Rows ``buf[i]`` of a ``[K, 1001]`` buffer: the odd rows are 4-byte aligned only, so every
    vector access has to be given up; the arithmetic is the same."""
    k, n = 8, 1001
    x, x64 = _case(k, n)
    buf = x.to(dev)
    assert buf[1].data_ptr() % 16 != 0
    al = [buf[i].clone() for i in range(k)]
    assert all(t.data_ptr() % 16 == 0 for t in al)
    out_un, out_al = torch.empty(n + 1, device=dev)[1:], torch.empty(n, device=dev)
    assert out_un.data_ptr() % 16 != 0
    got_un = _run([buf[i] for i in range(k)], [out_un], _weights(k), 3)
    got_al = _run(al, [out_al], _weights(k), 3)
    for a, b in zip(got_un, got_al):
        assert np.array_equal(a, b)
    assert torch.equal(out_un, out_al)


@pytest.mark.gpu
def test_deterministic(dev):
    x, _ = _case(8, BIG)
    rows = [r.clone() for r in x.to(dev)]
    got = []
    for _ in range(2):
        outs = [torch.empty(BIG, device=dev), torch.empty(BIG, device=dev)]
        coef, dist, obj = _run(rows, outs, _weights(8), 3)
        got.append((coef, dist, obj, outs[0].cpu().numpy(), outs[1].cpu().numpy()))
    for a, b in zip(*got):
        assert np.array_equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), 3e38])
def test_non_finite_row(dev, bad):
    """A NaN row, an Inf row and a row whose sum of squares overflows: coefficient exactly 0, the
    others as if the row were not there, finite outputs."""
    k, n = 5, 1001
    x, x64 = _case(k, n)
    xd = x.to(dev).clone()
    xd[2, 500] = bad
    rows = [xd[i].clone() for i in range(k)]
    w = [1.0, 2.0, 50.0, 3.0, 4.0]
    out = torch.empty(n, device=dev)
    coef, dist, obj = _run(rows, [out, rows[2]], w, 3)
    assert coef[2] == 0
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(rows[2]).all()) and np.all(np.isfinite(obj))
    keep = [0, 1, 3, 4]
    coef4, _, obj4 = _run([rows[i] for i in keep], [], [w[i] for i in keep], 3)
    # the same fp32 arithmetic on the same rows; only the order of the double additions over the
    # slabs differs (1024 / K chunks), which can move a float32 coefficient by an ulp per step, and
    # an ulp of a coefficient moves the next step's distances by a few 2^-24: 1e-5 is far outside
    np.testing.assert_allclose(coef[keep], coef4, rtol=1e-5)
    np.testing.assert_allclose(obj, obj4, rtol=1e-5)
    assert abs(float(coef.astype(np.float64).sum()) - 1) <= k * U


@pytest.mark.gpu
def test_every_row_nan(dev):
    rows = [torch.full((1001,), float("nan"), device=dev) for _ in range(3)]
    out = torch.zeros(1001, device=dev)
    coef, dist, obj = _run(rows, [out], [1.0, 1.0, 2.0], 3)
    assert coef.tolist() == [0.25, 0.25, 0.5]
    assert bool(torch.isnan(out).all()) and np.all(np.isnan(dist)) and np.all(obj == 0)


@pytest.mark.gpu
@pytest.mark.parametrize("iters", [1, 32])
def test_iteration_counts(dev, iters):
    k, n = 8, 1001
    x, x64 = _case(k, n)
    rows = [r.clone() for r in x.to(dev)]
    out = torch.empty(n, device=dev)
    coef, dist, obj = _run(rows, [out], _weights(k), iters)
    assert obj.shape == (iters,) and np.all(np.isfinite(obj)) and np.all(np.isfinite(dist))
    assert abs(float(coef.astype(np.float64).sum()) - 1) <= k * U
    assert obj[-1] <= obj[0]
    want = (coef.astype(np.float64)[:, None] * x64).sum(axis=0)
    assert float(np.abs(out.double().cpu().numpy() - want).max()) <= k * U * float(np.abs(x64).max())


@pytest.mark.gpu
def test_argument_errors_native(dev):
    from myfyp_amd import ops

    rows = [torch.zeros(8, device=dev) for _ in range(3)]
    with pytest.raises(ValueError, match="iters"):
        ops.geometric_median_into(rows, [], [1.0] * 3, iters=33)
    with pytest.raises(ValueError, match="3 rows but 2 weights"):
        ops.geometric_median_into(rows, [], [1.0, 1.0])
