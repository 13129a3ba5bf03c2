"""The float64 references of the FL kernels (``tests/_fl_ops_ref.py``) pinned against independent
implementations on the CPU: the CPU branches of ``myfyp_amd.ops`` (fed float64 tensors, so they
work in float64 too), ``torch.optim.Adam`` / ``SGD`` in float64, ``numpy.median`` and a dense
``M @ rows``. Both sides are float64: ``rtol = 1e-12`` of the magnitude the reference returns. The
one fp32 branch is ``ops.coordinate_median`` (it sorts ``.float()`` copies): exact for odd K, one
fp32 rounding of ``0.5·(a + b)`` for even K. Also here: the semantics the GPU tests rely on, checked
on the reference alone, and the noise statistics checked on numpy's own normal samples."""

import numpy as np
import pytest
import torch

import _fl_ops_ref as R

RTOL = 1e-12


def _rng(seed):
    return np.random.default_rng(seed)


def _f32(rng, *shape):
    return rng.standard_normal(shape).astype(np.float32)


def _t64(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64).copy())


def _close(got, want, mag, what, rtol=RTOL):
    got, want, mag = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64), np.asarray(mag, dtype=np.float64)
    err = np.abs(got - want)
    lim = rtol * mag + 1e-300
    worst = float((err / lim).max()) if err.size else 0.0
    print(f"{what}: max err {float(err.max()) if err.size else 0.0:.3e}, {worst:.3f} of the bound")
    assert np.all(err <= lim), (what, float(err.max()))


@pytest.mark.parametrize("k,n", [(1, 5), (5, 1001)])
def test_weighted_sums(k, n):
    from myfyp_amd import ops

    rng = _rng(k)
    x = _f32(rng, k, n)
    w = rng.random(k).astype(np.float32)
    if k > 2:
        w[1] = 0.0
    out, mag = R.weighted_sum(list(x), w)
    got = ops.weighted_average([[_t64(x[i])] for i in range(k)], [float(v) for v in w])[0]
    _close(got.numpy(), out, mag, "weighted_average")
    out, mag = R.stacked_weighted_sum(x, w, 0.25)
    dst = torch.empty(n, dtype=torch.float64)
    ops.stacked_weighted_sum(_t64(x), _t64(w), dst, scale=0.25)
    _close(dst.numpy(), out, mag, "stacked_weighted_sum")
    _close(out, 0.25 * (w.astype(np.float64)[:, None] * x.astype(np.float64)).sum(0), mag, "dense")


def test_zero_weight_rows_are_not_read():
    rng = _rng(0)
    x = _f32(rng, 4, 9)
    w = np.array([0.5, 0.0, 0.25, 0.0], dtype=np.float32)
    clean = R.stacked_weighted_sum(x, w, 2.0)
    x[1] = np.nan
    x[3] = np.inf
    for a, b in zip(clean, R.stacked_weighted_sum(x, w, 2.0)):
        assert np.array_equal(a, b)
    for a, b in zip(R.weighted_sum([x[0], x[2]], w[[0, 2]]), R.weighted_sum(list(x), w)):
        assert np.array_equal(a, b)
    out, mag, wsum = R.fedavg_reduce(x, w)
    assert np.all(np.isfinite(out)) and wsum == 0.75
    # the CPU branches of ops keep the same contract
    from myfyp_amd import ops

    dst = torch.empty(9, dtype=torch.float64)
    ops.stacked_weighted_sum(_t64(x), _t64(w), dst, scale=2.0)
    _close(dst.numpy(), clean[0], clean[1], "stacked_weighted_sum with NaN rows of weight 0")
    got = ops.weighted_average([[_t64(r)] for r in x], [float(v) for v in w])[0]
    _close(got.numpy(), *R.weighted_sum(list(x), w), "weighted_average with NaN rows of weight 0")
    mask = np.array([1, 1, 0, 0], dtype=np.float32)
    rows, mag = R.fedavg_local(x, w, mask, 9)
    assert np.all(np.isfinite(rows[:2])) and np.array_equal(rows[0], rows[1])
    # unmasked rows come back unchanged, NaN and Inf included
    assert np.array_equal(rows[2], x[2].astype(np.float64)) and np.all(np.isinf(rows[3]))
    m = np.zeros((4, 4), dtype=np.float32)
    m[0, 0] = m[0, 2] = 0.5
    m[2, 0] = 1.0
    mixed, _, nsrc = R.neighbor_mix(x, m, 9)
    assert list(nsrc) == [2, 0, 1, 0] and np.all(np.isfinite(mixed[[0, 2]]))
    assert np.all(np.isnan(mixed[1])) and np.array_equal(mixed[2], x[0].astype(np.float64))


def test_fedavg_and_masks():
    rng = _rng(1)
    p, n, ld = 5, 11, 13
    x = _f32(rng, p, ld)
    w = np.array([3, 0, 1, 2, 5], dtype=np.float32)
    mask = np.array([1, 1, 0, 1, 0], dtype=np.float32)
    out, mag, wsum = R.fedavg_reduce(x[:, :n], w)
    assert wsum == 11.0
    rows, amag = R.fedavg_apply(x, out, wsum, mask)
    want = (w.astype(np.float64)[:, None] * x[:, :n].astype(np.float64)).sum(0) / 11.0
    for r in range(p):
        if mask[r]:
            _close(rows[r, :n], want, np.abs(want), "fedavg apply")
            assert np.array_equal(rows[r, n:], x[r, n:].astype(np.float64))
        else:
            assert np.array_equal(rows[r], x[r].astype(np.float64))  # unmasked rows unchanged
    loc, lmag = R.fedavg_local(x, w, mask, n)
    assert np.array_equal(loc, rows)
    assert np.all(lmag >= np.abs(want) * (1 - 1e-15))
    # all weights zero: the sums are 0 and apply divides by 1e-12
    out0, _, wsum0 = R.fedavg_reduce(x[:, :n], np.zeros(p, dtype=np.float32))
    rows0, _ = R.fedavg_apply(x, out0, wsum0, mask)
    assert wsum0 == 0.0 and not out0.any() and not rows0[0, :n].any()
    rows1, _ = R.fedavg_apply(x, np.full(n, 1e-12, dtype=np.float32), 0.0, mask)
    _close(rows1[0, :n], np.full(n, R.f32(1e-12) / R.TINY), np.ones(n), "apply at wsum 0")
    # broadcast against ops' CPU branch
    from myfyp_amd import ops

    st = torch.from_numpy(x.copy())
    ops.broadcast_rows(torch.from_numpy(x[2, :n].copy()), st[:, :n], torch.from_numpy(mask))
    assert np.array_equal(R.broadcast(x, x[2, :n], mask), st.numpy().astype(np.float64))
    st = torch.from_numpy(x.copy())
    ops.broadcast_rows(torch.from_numpy(x[2, :n].copy()), st[:, :n])
    assert np.array_equal(R.broadcast(x, x[2, :n]), st.numpy().astype(np.float64))


def test_delayed_land():
    rng = _rng(2)
    p, n, ld, lds = 3, 7, 8, 9
    x, sn, avg = _f32(rng, p, ld), _f32(rng, p, lds), _f32(rng, n)
    mask = np.array([1, 0, 1], dtype=np.float32)
    rows, snap, mag = R.delayed_land(x, sn, avg, 4.0, mask, n)
    for r in (0, 2):
        want = x[r, :n].astype(np.float64) + avg.astype(np.float64) / 4.0 - sn[r, :n].astype(np.float64)
        _close(rows[r, :n], want, mag[r], "delayed land")
        assert np.array_equal(rows[r, :n], snap[r, :n])
        assert np.array_equal(rows[r, n:], x[r, n:].astype(np.float64)) and np.array_equal(snap[r, n:], sn[r, n:].astype(np.float64))
    assert np.array_equal(rows[1], x[1].astype(np.float64)) and np.array_equal(snap[1], sn[1].astype(np.float64))
    rows, snap, mag = R.delayed_land(x, sn, None, None, mask, n)
    assert np.array_equal(rows, x.astype(np.float64)) and not mag.any()
    assert np.array_equal(snap[0, :n], x[0, :n].astype(np.float64)) and np.array_equal(snap[1], sn[1].astype(np.float64))


@pytest.mark.parametrize("p", [1, 3, 16])
def test_neighbor_mix(p):
    rng = _rng(p)
    n, ld = 10, 12
    x = _f32(rng, p, ld)
    m = rng.random((p, p)).astype(np.float32)
    m /= m.sum(1, keepdims=True)
    if p > 2:
        m[1] = 0.0
    rows, mag, nsrc = R.neighbor_mix(x, m, n)
    want = m.astype(np.float64) @ x.astype(np.float64)
    for r in range(p):
        if nsrc[r]:
            _close(rows[r, :n], want[r, :n], mag[r], "mix")
            assert np.array_equal(rows[r, n:], x[r, n:].astype(np.float64))
        else:
            assert np.array_equal(rows[r], x[r].astype(np.float64))


@pytest.mark.parametrize("k", [1, 2, 3, 4, 7, 8, 15, 16])
def test_coordinate_median(k):
    from myfyp_amd import ops

    rng = _rng(k)
    x = np.round(_f32(rng, k, 257) * 2) / 2  # halves: plenty of ties and zeros
    x[0, :5] = [np.inf, -np.inf, 0.0, -0.0, 1.0]
    x = x.astype(np.float32)
    med, mag = R.coordinate_median(list(x))
    with np.errstate(invalid="ignore"):
        want = np.median(x.astype(np.float64), axis=0)
    ok = ~np.isnan(want)  # inf and -inf in the middle of an even K
    assert ok.sum() >= 250
    assert np.array_equal(med[ok], want[ok])
    got = ops.coordinate_median([[torch.from_numpy(x[i].copy())] for i in range(k)])[0].numpy().astype(np.float64)
    if k % 2:
        assert np.array_equal(got, med)
    else:
        fin = np.isfinite(med)
        assert np.array_equal(got[~fin & ok], med[~fin & ok])
        _close(got[fin], med[fin], mag[fin], "median, even K", rtol=R.gamma(1))
    # the total order: -0.0 sorts below +0.0, and an odd-K result carries the sign of the input it is
    z = [np.array([0.0], dtype=np.float32), np.array([-0.0], dtype=np.float32), np.array([-0.0], dtype=np.float32)]
    assert np.signbit(R.coordinate_median(z)[0][0])
    assert not np.signbit(R.coordinate_median([z[0], z[0], z[1]])[0][0])


@pytest.mark.parametrize("k", [0, 1, 5, 16])
def test_scaffold(k):
    from myfyp_amd import ops

    rng = _rng(10 + k)
    n = 33
    dys, dcs = _f32(rng, k, n), _f32(rng, k, n)
    w = (rng.random(k) * 10).astype(np.float32)
    buf, mag = R.scaffold_reduce(list(dys), list(dcs), w, n)
    got = torch.full((2 * n + 2,), float("nan"), dtype=torch.float64)
    ops.scaffold_reduce(got, [_t64(r) for r in dys], [_t64(r) for r in dcs], [float(v) for v in w])
    _close(got.numpy(), buf, mag + 1.0, "scaffold_reduce")
    assert buf[2 * n + 1] == k and (k > 0 or not buf.any())
    x0, c = _f32(rng, n), _f32(rng, n)
    b32 = buf.astype(np.float32)  # apply reads the fp32 buffer the all-reduce delivered
    for c_init in (False, True):
        x, c1, mx, mc = R.scaffold_apply(x0, b32, c, c_init, 0.7)
        outs = [torch.empty(n, dtype=torch.float64) for _ in range(2)]
        ct = torch.full((n,), float("nan"), dtype=torch.float64) if c_init else _t64(c)
        ops.scaffold_apply(outs, _t64(x0), _t64(b32), ct, c_init, R.f32(0.7))
        for o in outs:
            _close(o.numpy(), x, mx, "scaffold_apply x")
        _close(ct.numpy(), c1, mc, "scaffold_apply c")
        if k == 0:  # an empty round: x_start back, c unchanged
            assert np.array_equal(x, x0.astype(np.float64))
            assert np.array_equal(c1, np.zeros(n) if c_init else c.astype(np.float64))


def _opt_inputs(seed, n=65):
    rng = _rng(seed)
    w, g, a, cg, cl = (_f32(rng, n) for _ in range(5))
    m = 0.1 * _f32(rng, n)
    v = (0.01 * rng.random(n) + 1e-4).astype(np.float32)
    return w, g, m, v, a, cg, cl


EXTRAS = [dict(), dict(wd=0.01), dict(mu=0.1), dict(scaf=True), dict(wd=0.01, mu=0.1, scaf=True)]


@pytest.mark.parametrize("step", [1, 2, 1000])
@pytest.mark.parametrize("ex", EXTRAS, ids=lambda e: "+".join(e) or "plain")
def test_adam(step, ex):
    from myfyp_amd import ops

    w, g, m, v, a, cg, cl = _opt_inputs(step)
    lr, b1, b2, eps = R.f32(1e-2), R.f32(0.9), R.f32(0.999), R.f32(1e-8)
    wd, mu, scaf = R.f32(ex.get("wd", 0.0)), R.f32(ex.get("mu", 0.0)), ex.get("scaf", False)
    w1, m1, v1, uw, um, uv = R.adam_step(w, g, m, v, step, lr, b1, b2, eps, wd, a if mu else None, mu, cg if scaf else None, cl if scaf else None)
    assert np.all(uw > 0) and np.all(um > 0) and np.all(uv > 0)
    pw, pm, pv = _t64(w), _t64(m), _t64(v)
    ops.adam_step(pw, _t64(g), pm, pv, step, lr, b1, b2, eps, wd, anchor=_t64(a) if mu else None, c_global=_t64(cg) if scaf else None,
                  c_local=_t64(cl) if scaf else None, mu=mu)
    _close(pw.numpy(), w1, uw, "adam w (ops)")
    _close(pm.numpy(), m1, um, "adam m (ops)")
    _close(pv.numpy(), v1, uv, "adam v (ops)")
    if not mu and not scaf:  # torch.optim.Adam knows weight decay only
        p = torch.nn.Parameter(_t64(w))
        opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
        opt.state[p] = {"step": torch.tensor(float(step - 1)), "exp_avg": _t64(m), "exp_avg_sq": _t64(v)}
        p.grad = _t64(g)
        opt.step()
        _close(p.detach().numpy(), w1, uw, "adam w (torch.optim)")
        _close(opt.state[p]["exp_avg"].numpy(), m1, um, "adam m (torch.optim)")
        _close(opt.state[p]["exp_avg_sq"].numpy(), v1, uv, "adam v (torch.optim)")


@pytest.mark.parametrize("mom,nesterov", [(0.0, False), (0.9, False), (0.9, True)])
@pytest.mark.parametrize("ex", EXTRAS, ids=lambda e: "+".join(e) or "plain")
def test_sgd(mom, nesterov, ex):
    from myfyp_amd import ops

    w, g, m, v, a, cg, cl = _opt_inputs(7)
    lr, mom = R.f32(0.05), R.f32(mom)
    wd, mu, scaf = R.f32(ex.get("wd", 0.0)), R.f32(ex.get("mu", 0.0)), ex.get("scaf", False)
    w1, m1, uw, um = R.sgd_step(w, g, m if mom else None, lr, mom, wd, nesterov, a if mu else None, mu, cg if scaf else None, cl if scaf else None)
    pw, pm = _t64(w), _t64(m)
    ops.sgd_step(pw, _t64(g), pm if mom else None, lr, mom, wd, nesterov, anchor=_t64(a) if mu else None, c_global=_t64(cg) if scaf else None,
                 c_local=_t64(cl) if scaf else None, mu=mu)
    _close(pw.numpy(), w1, uw, "sgd w (ops)")
    if mom:
        _close(pm.numpy(), m1, um, "sgd m (ops)")
    else:
        assert m1 is None and um is None
    if not mu and not scaf:
        p = torch.nn.Parameter(_t64(w))
        opt = torch.optim.SGD([p], lr=lr, momentum=mom, weight_decay=wd, nesterov=nesterov)
        if mom:
            opt.state[p] = {"momentum_buffer": _t64(m)}
        p.grad = _t64(g)
        opt.step()
        _close(p.detach().numpy(), w1, uw, "sgd w (torch.optim)")
        if mom:
            _close(opt.state[p]["momentum_buffer"].numpy(), m1, um, "sgd m (torch.optim)")


def test_scale_part_is_exact():
    t = _f32(_rng(3), 100)
    assert np.array_equal(R.scale_part(t, -1.0), -t.astype(np.float64))
    assert np.array_equal(R.scale_part(t, 0.5).astype(np.float32), t * np.float32(0.5))


def test_noise_statistics_on_numpy_normals():
    """float64 normal samples of the GPU test's size from numpy's generator, seeds 3 and 4, meet
    every threshold the GPU test applies to the kernel's samples; a sample with a defect does not."""
    n = 1 << 20
    a = _rng(3).standard_normal(n)
    b = _rng(4).standard_normal(n)
    for z, other in ((a, b), (b, a)):
        st = R.noise_stats(0.5 * z, 0.5, 0.5 * other)
        print(st)
        lim = R.noise_limits(n)
        assert st["absmax"] <= lim["absmax"]
        assert R.noise_check(st) == []
    assert any(s.startswith("seeds") for s in R.noise_check(R.noise_stats(a, 1.0, a + 0.1 * b)))
    assert any(s.startswith("var") for s in R.noise_check(R.noise_stats(1.01 * a, 1.0)))
    assert any(s.startswith("lag1") for s in R.noise_check(R.noise_stats(a + 0.01 * np.roll(a, 1), 1.0)))
    assert any(s.startswith("halves") for s in R.noise_check(R.noise_stats(np.concatenate([a[: n // 2], a[: n // 2] + 0.1 * b[: n // 2]]), 1.0)))
    assert any(s.startswith("ks") for s in R.noise_check(R.noise_stats(np.sign(a) * np.abs(a) ** 1.01, 1.0)))
    assert abs(R.Z_CAP - 5.768) < 1e-3
