"""The float64 oracle of the CNN companion kernels (``tests/_cnn_ops_ref.py``) checked against torch
itself, on the CPU, at the small shapes ``tests/test_cnn_ops_gpu.py`` uses: autograd through
``F.batch_norm`` / the pools / ``F.cross_entropy``, ``torch.optim.SGD`` and ``ops.sgd_step``."""

import pytest
import torch
import torch.nn.functional as F

import _cnn_ops_ref as R

F64 = torch.float64


def _nchw(x, n, h, w, c):
    """engine rows [n*h*w, Cp] -> torch [n, c, h, w]"""
    return x[: n * h * w, :c].reshape(n, h, w, c).permute(0, 3, 1, 2).contiguous()


@pytest.mark.parametrize("residual", ["none", "res", "bn2"])
@pytest.mark.parametrize("C,Cp,h", [(6, 8, 2), (20, 24, 1), (40, 40, 5)])
def test_batchnorm_chain_matches_autograd(C, Cp, h, residual):
    torch.manual_seed(1)
    nb, hw, B = [5, 2, 0], h * h, 5
    P, rows, eps, mom = 3, 5 * h * h, 1e-5, 0.1
    y = torch.zeros(P, rows, Cp, dtype=F64)
    y[..., :C] = torch.randn(P, rows, C, dtype=F64) * 2 + 0.5
    y2 = torch.zeros_like(y)
    y2[..., :C] = torch.randn(P, rows, C, dtype=F64)
    res = torch.zeros_like(y)
    res[..., :C] = torch.randn(P, rows, C, dtype=F64)
    dz = torch.zeros_like(y)
    dz[..., :C] = torch.randn(P, rows, C, dtype=F64)
    gamma, beta = torch.rand(P, C, dtype=F64) + 0.5, torch.randn(P, C, dtype=F64)
    gamma2, beta2 = torch.rand(P, C, dtype=F64) + 0.5, torch.randn(P, C, dtype=F64)
    rmean, rvar = torch.randn(P, C, dtype=F64), torch.rand(P, C, dtype=F64) + 0.5

    def stats_of(t):  # two partial rows, as a conv epilogue would leave them
        st = torch.zeros(P, 2, 2, Cp, dtype=F64)
        for p in range(P):
            v = t[p, : nb[p] * hw]
            k = v.shape[0] // 2
            for r, part in enumerate((v[:k], v[k:])):
                st[p, r, 0], st[p, r, 1] = part.sum(0), (part * part).sum(0)
        return st

    ss, ms, rm, rv, st_new = R.bn_finalize(stats_of(y), nb, hw, gamma, beta, rmean, rvar, C, Cp, eps, mom, 1)
    ss2, ms2, _, _, _ = R.bn_finalize(stats_of(y2), nb, hw, gamma2, beta2, rmean, rvar, C, Cp, eps, mom, 1)
    assert not st_new.any()
    assert not ss[:, :, C:].any() and not ms[:, :, C:].any()
    out, _ = R.bn_act(y, ss, res if residual == "res" else None, y2 if residual == "bn2" else None, ss2 if residual == "bn2" else None, 1, nb, hw)
    g, _ = R.bn_bwd_g(dz, out, y, None, nb, hw)
    g_mss, _ = R.bn_bwd_g(dz, None, y, ss, nb, hw)
    sums = R.bn_bwd_sums(g, y, ms, nb, hw)
    dgamma, dbeta, coef = R.bn_bwd_finalize(sums, nb, hw, gamma, ms, C, Cp)
    dy, _ = R.bn_bwd_apply(g, y, ms, coef, nb, hw)
    assert not coef[:, :, C:].any()

    for p in range(2):
        n = nb[p]
        xt = _nchw(y[p], n, h, h, C).requires_grad_(True)
        gt, bt = gamma[p].clone().requires_grad_(True), beta[p].clone().requires_grad_(True)
        rmt, rvt = rmean[p].clone(), rvar[p].clone()
        z = F.batch_norm(xt, rmt, rvt, gt, bt, True, mom, eps)
        if residual == "res":
            z = z + _nchw(res[p], n, h, h, C)
        if residual == "bn2":
            z = z + F.batch_norm(_nchw(y2[p], n, h, h, C), None, None, gamma2[p], beta2[p], True, mom, eps)
        o = F.relu(z)
        (o * _nchw(dz[p], n, h, h, C)).sum().backward()
        tol = dict(rtol=1e-9, atol=1e-9)
        assert torch.allclose(_nchw(out[p], n, h, h, C), o.detach(), **tol)
        assert torch.isnan(out[p, n * hw:]).all()
        assert torch.allclose(rm[p], rmt, **tol) and torch.allclose(rv[p], rvt, **tol)
        assert torch.allclose(dgamma[p], gt.grad, **tol) and torch.allclose(dbeta[p], bt.grad, **tol)
        assert torch.allclose(_nchw(dy[p], n, h, h, C), xt.grad, **tol)
        assert torch.isnan(dy[p, n * hw:]).all()
        if residual == "none":  # the recomputed mask is this BN's own output sign
            assert torch.equal(torch.nan_to_num(g_mss[p]), torch.nan_to_num(g[p]))
        # evaluation mode: running statistics, nothing moves
        sse, _, rme, rve, st_e = R.bn_finalize(stats_of(y), nb, hw, gamma, beta, rmean, rvar, C, Cp, eps, mom, 0)
        oe, _ = R.bn_act(y, sse, None, None, None, 0, nb, hw)
        ze = F.batch_norm(_nchw(y[p], n, h, h, C), rmean[p].clone(), rvar[p].clone(), gamma[p], beta[p], False, mom, eps)
        assert torch.allclose(_nchw(oe[p], n, h, h, C), ze, **tol)
        assert torch.equal(rme, rmean) and torch.equal(rve, rvar) and torch.equal(st_e, stats_of(y))
    # the peer without samples: statistics kept, nothing written
    assert torch.equal(rm[2], rmean[2]) and torch.equal(rv[2], rvar[2])
    assert torch.isnan(out[2]).all() and torch.isnan(dy[2]).all()
    assert not dgamma[2].any() and not dbeta[2].any()


def test_batchnorm_single_element_uses_biased_variance():
    st = torch.zeros(1, 1, 2, 8, dtype=F64)
    st[0, 0, 0, :3], st[0, 0, 1, :3] = torch.tensor([1.0, -2.0, 0.5]), torch.tensor([1.0, 4.0, 0.25])
    one, zero = torch.ones(1, 3, dtype=F64), torch.zeros(1, 3, dtype=F64)
    _, ms, rm, rv, _ = R.bn_finalize(st, [1], 1, one, zero, zero, one, 3, 8, 0.25, 0.5, 1)
    assert torch.equal(rm[0], torch.tensor([0.5, -1.0, 0.25], dtype=F64))
    assert torch.equal(rv[0], torch.full((3,), 0.5, dtype=F64))  # var = 0, not 0/0
    assert torch.equal(ms[0, 1, :3], torch.full((3,), 2.0, dtype=F64))


def test_relu_bwd_and_colsum_match_torch():
    torch.manual_seed(2)
    nb, hw = [3, 1, 0], 4
    x = torch.randn(3, 12, 24, dtype=F64)
    mask = torch.randn(3, 12, 24, dtype=F64).clamp_min(0)
    out = R.relu_bwd(x, mask, nb, hw)
    cs = R.colsum(x, nb, hw, 20)
    for p in range(3):
        r = nb[p] * hw
        assert torch.equal(out[p, :r], x[p, :r] * (mask[p, :r] > 0))
        assert torch.isnan(out[p, r:]).all()
        assert torch.allclose(cs[p], x[p, :r, :20].sum(0), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("H,W", [(4, 4), (6, 2), (5, 5)])
def test_maxpool_matches_autograd_with_ties(H, W):
    torch.manual_seed(3)
    nb, B, Cp = [3, 2, 0], 3, 8
    x = torch.randint(0, 2, (3, B, H, W, Cp)).double() / 8  # 0 or 1/8, as after a ReLU: three windows in four tie
    dy = torch.randint(-32, 33, (3, B, H // 2, W // 2, Cp)).double() / 8
    out = R.maxpool2(x, nb)
    dx = R.maxpool2_bwd(x, dy, nb)
    ties = 0
    for p in range(2):
        n = nb[p]
        xt = x[p, :n].permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        o = F.max_pool2d(xt, 2)
        (o * dy[p, :n].permute(0, 3, 1, 2)).sum().backward()
        assert torch.equal(out[p, :n].permute(0, 3, 1, 2), o.detach())
        got = dx[p, :n].permute(0, 3, 1, 2)
        He, We = H // 2 * 2, W // 2 * 2
        assert torch.equal(got[:, :, :He, :We], xt.grad[:, :, :He, :We])
        assert torch.isnan(got[:, :, He:]).all() and torch.isnan(got[:, :, :, We:]).all()  # odd edge: never written
        assert not xt.grad[:, :, He:].any() and not xt.grad[:, :, :, We:].any()
        assert torch.isnan(out[p, n:]).all() and torch.isnan(dx[p, n:]).all()
        w = R.windows(x[p:p + 1, :n])
        ties += int(((w == w.max(0).values).sum(0) > 1).sum())
    assert ties > 0.5 * 5 * (H // 2) * (W // 2) * Cp
    assert torch.isnan(out[2]).all() and torch.isnan(dx[2]).all()
    # the negative control used on the GPU really differs
    last = R.maxpool2_bwd(x, dy, nb, last=True)
    assert not torch.equal(torch.nan_to_num(last), torch.nan_to_num(dx))


@pytest.mark.parametrize("hw", [1, 4, 16, 25])
def test_avgpool_matches_autograd(hw):
    torch.manual_seed(4)
    nb, B, Cp = [4, 1, 0], 4, 24
    x = torch.randn(3, B, hw, Cp, dtype=F64)
    dy = torch.randn(3, B, Cp, dtype=F64)
    out, _ = R.avgpool(x, nb)
    dx, _ = R.avgpool_bwd(dy, nb, hw)
    side = int(hw ** 0.5)
    for p in range(2):
        n = nb[p]
        xt = x[p, :n].reshape(n, side, side, Cp).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        o = F.adaptive_avg_pool2d(xt, 1).flatten(1)
        (o * dy[p, :n]).sum().backward()
        assert torch.allclose(out[p, :n], o.detach(), rtol=1e-12, atol=1e-12)
        assert torch.allclose(dx[p, :n].reshape(n, side, side, Cp).permute(0, 3, 1, 2), xt.grad, rtol=1e-12, atol=1e-12)
    assert torch.isnan(out[2]).all() and torch.isnan(dx[2]).all() and torch.isnan(out[1, 1:]).all()


@pytest.mark.parametrize("K,Lp", [(10, 16), (16, 16)])
def test_xent_matches_cross_entropy(K, Lp):
    torch.manual_seed(5)
    nb, B = [5, 3, 0], 5
    logits = torch.randn(3, B, Lp, dtype=F64) * 2
    labels = torch.randint(0, K, (3, B))
    loss, correct, conf, dl = R.xent(logits, labels, nb, K)
    for p in range(2):
        n = nb[p]
        z = logits[p, :n, :K].clone().requires_grad_(True)
        ce = F.cross_entropy(z, labels[p, :n], reduction="sum")
        (ce / n).backward()
        assert torch.allclose(loss[p], ce.detach(), rtol=1e-12)
        assert torch.allclose(dl[p, :n, :K], z.grad, rtol=1e-10, atol=1e-14)
        assert not dl[p, n:].any() and not dl[p, :, K:].any()
        pred = z.argmax(1)
        assert correct[p] == float((pred == labels[p, :n]).sum())
        want = torch.zeros(16, 16, dtype=torch.int64)
        for y, a in zip(labels[p, :n].tolist(), pred.tolist()):
            want[y, a] += 1
        assert torch.equal(conf[p], want)
    assert loss[2] == 0 and correct[2] == 0 and not conf[2].any() and not dl[2].any()


@pytest.mark.parametrize("momentum,wd,nesterov", [(0.0, 0.0, False), (0.9, 5e-4, False), (0.9, 5e-4, True), (0.5, 0.0, True)])
def test_sgd_update_matches_torch_optim(momentum, wd, nesterov):
    torch.manual_seed(6)
    w0 = torch.randn(300, dtype=F64)
    grads = [torch.randn(300, dtype=F64) for _ in range(3)]
    pt = w0.clone().requires_grad_(True)
    opt = torch.optim.SGD([pt], lr=0.05, momentum=momentum, weight_decay=wd, nesterov=nesterov)
    w, m = w0.clone(), torch.zeros(300, dtype=F64)
    for g in grads:
        pt.grad = g.clone()
        opt.step()
        w, m = R.sgd_update(w, g, m, 0.05, momentum, wd, nesterov)
        assert torch.allclose(w, pt.detach(), rtol=1e-12, atol=1e-12)
    if momentum == 0.0:
        assert not m.any()


@pytest.mark.parametrize("momentum,nesterov", [(0.0, False), (0.9, False), (0.9, True)])
def test_sgd_update_fedprox_scaffold_match_ops_sgd_step(momentum, nesterov):
    from myfyp_amd import ops

    torch.manual_seed(7)
    w0, anchor, cg, cl = (torch.randn(64, dtype=F64) for _ in range(4))
    pw, pm = w0.clone(), torch.zeros(64, dtype=F64)
    w, m = w0.clone(), torch.zeros(64, dtype=F64)
    for _ in range(3):
        g = torch.randn(64, dtype=F64)
        ops.sgd_step(pw, g, pm, 0.05, momentum, 1e-3, nesterov, anchor, cg, cl, 0.1)
        w, m = R.sgd_update(w, g, m, 0.05, momentum, 1e-3, nesterov, 0.1, anchor, cg, cl)
        assert torch.allclose(w, pw, rtol=1e-12, atol=1e-12)
        if momentum:
            assert torch.allclose(m, pm, rtol=1e-12, atol=1e-12)


def test_shadow_layout_and_column_maps():
    torch.manual_seed(8)
    cout, cin, rs, cp = 4, 3, 9, 8
    w = torch.randn(cout, cin, rs, dtype=F64)
    sh = R.wf_shadow(w, cp)
    want = torch.zeros(cout, rs, cp, dtype=F64)
    want[:, :, :cin] = w.permute(0, 2, 1)  # [cout][R][S][cin], zero padding channels
    assert torch.equal(sh, want)
    gf = torch.randn(cout, rs, cp, dtype=F64)
    assert torch.equal(R.wf_grad_to_torch(gf, cin), gf[:, :, :cin].permute(0, 2, 1))
    # fc behind a shuffled flatten: engine channel t2e[ct] holds torch column ct
    cin, cp = 20, 24
    t2e = torch.randperm(cp)[:cin]
    e2t = torch.full((cp,), -1, dtype=torch.int64)
    e2t[t2e] = torch.arange(cin)
    w = torch.randn(cout, cin, 1, dtype=F64)
    sh = R.wf_shadow(w, cp, e2t)
    x_t = torch.randn(cin, dtype=F64)
    x_e = torch.zeros(cp, dtype=F64)
    x_e[t2e] = x_t
    assert torch.allclose(sh[:, 0] @ x_e, w[:, :, 0] @ x_t, rtol=1e-12)  # same layer output in either order
    assert int((sh[0, 0] == 0).sum()) == cp - cin
    gf = torch.randn(cout, 1, cp, dtype=F64)
    assert torch.equal(R.wf_grad_to_torch(gf, cin, t2e)[:, :, 0], gf[:, 0][:, t2e])


def test_opt_step_composes_update_and_shadow():
    torch.manual_seed(9)
    P, ps = 3, 64
    seg = dict(off=4, n=2 * 3 * 4, kind=1, cout=2, cin=3, R=2, S=2, cp_in=8, zero_after=1, wf_off=8, e2t=None, t2e=None)
    vec = dict(off=40, n=10, kind=0, cout=0, cin=0, R=0, S=0, cp_in=0, zero_after=0, wf_off=0, e2t=None, t2e=None)
    w, g, m, gf = (torch.randn(P, ps, dtype=F64) for _ in range(4))
    gf = torch.randn(P, 80, dtype=F64)
    sh = torch.full((P, 80), R.NAN, dtype=F64)
    hp = dict(lr=0.1, momentum=0.9, weight_decay=0.0, nesterov=False, mu=0.0)
    w1, g1, m1, gf1, sh1 = R.opt_step(w, g, m, gf, sh, [seg, vec], hp, [1, 0, 1], 1)
    assert torch.equal(w1[1], w[1]) and torch.equal(m1[1], m[1]) and torch.isnan(sh1[1]).all() and torch.equal(gf1[1], gf[1])
    for p in (0, 2):
        gt = gf[p, 8:72].reshape(2, 4, 8)[:, :, :3].permute(0, 2, 1).reshape(-1)
        ww, mm = R.sgd_update(w[p, 4:28], gt, m[p, 4:28], **hp)
        assert torch.equal(w1[p, 4:28], ww) and torch.equal(m1[p, 4:28], mm)
        assert torch.equal(sh1[p, 8:72], R.wf_shadow(ww.reshape(2, 3, 4), 8).reshape(-1))
        assert torch.isnan(sh1[p, :8]).all() and torch.isnan(sh1[p, 72:]).all()
        assert not gf1[p, 8:72].any() and torch.equal(gf1[p, :8], gf[p, :8])
        assert torch.equal(g1[p], g[p])  # zero_after = 0 on the plain segment
        assert torch.equal(w1[p, :4], w[p, :4]) and torch.equal(w1[p, 28:40], w[p, 28:40]) and torch.equal(w1[p, 50:], w[p, 50:])
    w2, _, m2, gf2, sh2 = R.opt_step(w, g, m, gf, sh, [seg, vec], hp, None, 0)
    assert torch.equal(w2, w) and torch.equal(m2, m) and torch.equal(gf2, gf)
    assert torch.equal(sh2[1, 8:72], R.wf_shadow(w[1, 4:28].reshape(2, 3, 4), 8).reshape(-1))


def test_tolerance_helpers():
    v = torch.tensor([1.0, 1.5, 2.0, 0.75, -3.0, 0.0], dtype=F64)
    assert torch.equal(R.ulp_bf16(v)[:5], torch.tensor([2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8, 2.0 ** -6], dtype=F64))
    for x in (1.0, 1.5, 0.75, 3.0):  # the spacing really is bf16's
        nxt = torch.tensor(x, dtype=torch.bfloat16).view(torch.int16) + 1
        assert float(nxt.view(torch.bfloat16)) - x == float(R.ulp_bf16(torch.tensor([x]))[0])
    ref = torch.tensor([1.0, 100.0, R.NAN], dtype=F64)
    assert R.fp32_bound(ref, ref.float()) == 2.0 ** -22 * 100.0
    assert R.fp32_bound(ref, (ref + 1e-3).float()) == pytest.approx(4e-3, rel=1e-2)
