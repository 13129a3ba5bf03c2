"""Pins the float64 oracle of the implicit-GEMM conv kernels (``tests/_conv_ref.py``) on the CPU:
against torch's float64 convolutions and autograd, and — for the input families the GPU test calls
exact — the proof that they are: the fp32 evaluation of the same formula in two summation orders
equals the float64 result bit for bit, and ``sum |term| / unit < 2^24`` for every accumulated
quantity (then every partial sum, in any order, is a multiple of ``unit`` that fp32 holds)."""

import pytest
import torch
import torch.nn.functional as F

import _conv_ref as C

F64, F32 = torch.float64, torch.float32
LIM = 2.0 ** 24

# H, W, R, S, stride, pad, cin, cout: non-square images and filters, both strides, pads 0 / 1 / 2,
# channel counts that are no multiple of 8
GEOM = [(5, 7, 3, 3, 1, 1, 3, 6), (9, 6, 3, 3, 2, 1, 6, 20), (9, 6, 5, 5, 2, 2, 8, 5), (7, 5, 1, 3, 1, 1, 4, 7), (7, 5, 3, 1, 1, 0, 4, 7),
        (6, 9, 1, 1, 2, 0, 10, 3), (1, 1, 1, 1, 1, 0, 12, 10), (8, 5, 5, 5, 1, 2, 3, 4), (7, 7, 3, 3, 2, 0, 5, 5), (4, 6, 3, 3, 1, 2, 2, 3)]


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("H,W,R,S,stride,pad,cin,cout", GEOM)
def test_convolutions_match_torch_float64(H, W, R, S, stride, pad, cin, cout):
    g = C.gen(H * 100 + W * 10 + R + cin)
    n = 3
    Ho, Wo = C.out_hw(H, W, R, S, stride, pad)
    x = torch.randn(n, H, W, cin, generator=g, dtype=F64)
    w = torch.randn(cout, R, S, cin, generator=g, dtype=F64)  # Wf layout
    dy = torch.randn(n, Ho, Wo, cout, generator=g, dtype=F64)
    wt = w.permute(0, 3, 1, 2).contiguous()  # torch order [cout][cin][R][S]
    y = C.conv_acc(x, w, stride, pad, Ho, Wo)
    torch.testing.assert_close(y, _nhwc(F.conv2d(_nchw(x), wt, stride=stride, padding=pad)), rtol=1e-12, atol=1e-12)
    dx = C.conv_dgrad(dy, w, H, W, stride, pad)
    dx_t = torch.nn.grad.conv2d_input((n, cin, H, W), wt, _nchw(dy), stride=stride, padding=pad)
    torch.testing.assert_close(dx, _nhwc(dx_t), rtol=1e-12, atol=1e-12)
    dw = C.conv_wgrad(dy, x, R, S, stride, pad)
    dw_t = torch.nn.grad.conv2d_weight(_nchw(x), wt.shape, _nchw(dy), stride=stride, padding=pad)
    torch.testing.assert_close(dw, dw_t.permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)
    # the other summation order is the same function
    torch.testing.assert_close(C.conv_acc(x, w, stride, pad, Ho, Wo, 1), y, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(C.conv_dgrad(dy, w, H, W, stride, pad, 1), dx, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(C.conv_wgrad(dy, x, R, S, stride, pad, 1), dw, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("H,W,R,S,stride,pad,cin,cout", GEOM[:5])
def test_grouped_forward_epilogue_statistics_and_prologue(H, W, R, S, stride, pad, cin, cout):
    g = C.gen(7 + H + cin)
    B, nb = 4, [4, 2, 0]
    cpi, cpo = C.cp(cin), C.cp(cout)
    Ho, Wo = C.out_hw(H, W, R, S, stride, pad)
    y = C.pad_channels(C.normal(g, C.P, B, H, W, cpi), cin)
    y[1, 2:] = C.NAN  # rows past a peer's batch are never read
    y[2] = C.NAN
    w = C.pad_channels(C.normal(g, C.P, cpo, R, S, cpi), cin)
    w[:, cout:] = 0
    bias, resid = C.normal(g, C.P, cpo), C.normal(g, C.P, B, Ho, Wo, cpo)
    ss = C.pad_channels(C.coeffs(g, C.P, cpi, "randn"), cin)
    out, v, stats = C.forward(y, w, nb, stride, pad, Ho, Wo, cout, bias, resid, True, ss)
    for p, n in enumerate(nb):
        assert torch.isnan(out[p, n:]).all() and torch.isnan(v[p, n:]).all()
        if n == 0:
            assert float(stats[p].abs().max()) == 0.0
            continue
        a = torch.relu(y[p, :n, ..., :cin] * ss[p, 0, :cin] + ss[p, 1, :cin]).to(torch.bfloat16).double()
        wt = w[p, :cout, :, :, :cin].permute(0, 3, 1, 2).contiguous()
        ref = _nhwc(F.conv2d(_nchw(a), wt, bias[p, :cout], stride=stride, padding=pad))
        ref = torch.relu(ref + resid[p, :n, ..., :cout])
        torch.testing.assert_close(v[p, :n, ..., :cout], ref, rtol=1e-12, atol=1e-12)
        assert float(v[p, :n, ..., cout:].abs().max() if cpo > cout else 0.0) == 0.0  # residual there is dropped
        assert torch.equal(out[p, :n], v[p, :n].float().to(torch.bfloat16).double())
        torch.testing.assert_close(stats[p, 0, :cout], ref.sum((0, 1, 2)), rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(stats[p, 1, :cout], ref.pow(2).sum((0, 1, 2)), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("two,use_ss,with_resid,stride", [(False, False, False, 1), (True, False, True, 2), (True, True, True, 1), (False, True, False, 2)])
def test_bn_backward_sums_match_autograd(two, use_ss, with_resid, stride):
    """The producer of the conv's input is ``a = relu(bn0(y0) [+ bn1(y1)])`` (batch statistics); the
    gradient that reaches it is dX of the conv plus a skip gradient. autograd's dgamma / dbeta of the
    BatchNorms are the epilogue's ``sum g * xhat`` / ``sum g``. Ternary dY, weights and skip gradient
    keep ``g`` an integer, which the bf16 rounding leaves alone."""
    g_ = C.gen(11 + two + 2 * use_ss)
    H, W, R, S, pad, cin, cout, n = 7, 5, 3, 3, 1, 5, 6, 3
    cpi, cpo = C.cp(cin), C.cp(cout)
    Ho, Wo = C.out_hw(H, W, R, S, stride, pad)
    ys = [torch.randn(n, H, W, cin, generator=g_, dtype=F64) * 2 + 0.5 for _ in range(2 if two else 1)]
    gam = [(torch.rand(cin, generator=g_, dtype=F64) + 0.5).requires_grad_() for _ in ys]
    bet = [torch.randn(cin, generator=g_, dtype=F64).requires_grad_() for _ in ys]
    eps = 1e-5
    mean = [t.mean((0, 1, 2)) for t in ys]
    inv = [1 / torch.sqrt(t.var((0, 1, 2), unbiased=False) + eps) for t in ys]
    xhat = [(t - m) * i for t, m, i in zip(ys, mean, inv)]  # statistics held constant: the sums are partial derivatives
    z = sum(xh * ga + be for xh, ga, be in zip(xhat, gam, bet))
    a = torch.relu(z)
    w = C.ternary(g_, cout, R, S, cin)
    dy = C.ternary(g_, n, Ho, Wo, cout)
    skip = C.ternary(g_, n, H, W, cin) if with_resid else None
    out = F.conv2d(_nchw(a), w.permute(0, 3, 1, 2).contiguous(), stride=stride, padding=pad)
    loss = (out * _nchw(dy)).sum() + ((a * skip).sum() if with_resid else 0.0)
    loss.backward()

    def slab(t, c, cpad):  # one live peer in the grouped layout
        o = torch.zeros(1, *t.shape[:-1], cpad, dtype=F64)
        o[0, ..., :c] = t.detach()
        return o

    wf = torch.zeros(1, cpo, R, S, cpi, dtype=F64)
    wf[0, :cout, :, :, :cin] = w
    ms = [slab(torch.stack([m, i]), cin, cpi) for m, i in zip(mean, inv)]
    kw = dict(resid=slab(skip, cin, cpi) if with_resid else None, y0=slab(ys[0], cin, cpi), ms0=ms[0])
    if two:
        kw.update(y1=slab(ys[1], cin, cpi), ms1=ms[1])
    if use_ss and not two:  # the mask recomputed from y0 needs the whole pre-activation in one BN
        sc = gam[0].detach() * inv[0]
        kw["mask_ss"] = slab(torch.stack([sc, bet[0].detach() - mean[0] * sc]), cin, cpi)
    else:
        kw["mask"] = slab(a, cin, cpi)
    gout, v, sums = C.dgrad(slab(dy, cout, cpo), wf, [n], H, W, stride, pad, cin, **kw)
    assert torch.equal(C.bf16(v), v)  # integers: the rounding is the identity
    assert float(gout[0, ..., :cin].abs().sum()) > 0
    for i in range(len(ys)):
        torch.testing.assert_close(sums[0, 0, :cin], bet[i].grad, rtol=1e-9, atol=1e-9)
        torch.testing.assert_close(sums[0, 1 + i, :cin], gam[i].grad, rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("H,W,R,S,pad,cin,cout", [(5, 7, 3, 3, 1, 8, 16), (7, 5, 5, 5, 2, 8, 8), (6, 4, 1, 3, 1, 16, 8), (4, 6, 3, 1, 0, 8, 8)])
def test_flipped_weights_turn_the_forward_conv_into_the_stride1_dgrad(H, W, R, S, pad, cin, cout):
    """Mode 4: ``dX = conv(dY, wt_flip(Wf))`` with ``pad' = R - 1 - pad`` (square filters; for R != S
    the two paddings differ, which one ``pad`` cannot express: those go through mode 1)."""
    g = C.gen(H + W + R)
    Ho, Wo = C.out_hw(H, W, R, S, 1, pad)
    w, dy = C.ternary(g, cout, R, S, cin), C.ternary(g, 2, Ho, Wo, cout)
    wt = C.wt_flip(w)
    assert wt.shape == (cin, R, S, cout)
    for r in range(R):
        for s in range(S):
            assert torch.equal(wt[:, r, s, :], w[:, R - 1 - r, S - 1 - s, :].t())
    if R == S:
        assert torch.equal(C.conv_acc(dy, wt, 1, R - 1 - pad, H, W), C.conv_dgrad(dy, w, H, W, 1, pad))


@pytest.mark.parametrize("H,W,R,S,pad,cin,cout", [(9, 6, 3, 3, 1, 8, 16), (6, 9, 1, 1, 0, 8, 8), (9, 6, 5, 5, 2, 8, 8), (8, 7, 3, 3, 0, 8, 8), (7, 8, 1, 3, 1, 8, 8)])
def test_parity_class_weights_turn_forward_convs_into_the_stride2_dgrad(H, W, R, S, pad, cin, cout):
    """Mode 5: dX pixel (2 hh + ph, 2 ww + pw) of class (ph, pw) only sees the taps r = r0 (mod 2),
    s = s0 (mod 2); walking the class's block ``[ci][i'][j'][co]`` of ``wt_flip_parity`` over dY as a
    forward conv gives the dgrad."""
    g = C.gen(H * W + R)
    Ho, Wo = C.out_hw(H, W, R, S, 2, pad)
    w, dy = C.ternary(g, cout, R, S, cin), C.ternary(g, 2, Ho, Wo, cout)
    flat = C.wt_flip_parity(w, pad)
    ref = C.conv_dgrad(dy, w, H, W, 2, pad)
    dx = torch.zeros_like(ref)
    off = 0
    for c in range(4):
        ph, pw = c >> 1, c & 1
        rr, ss = C.parity_taps(R, S, pad, c)
        if not (rr and ss):
            continue
        blk = flat[off:off + cin * len(rr) * len(ss) * cout].reshape(cin, len(rr), len(ss), cout)
        off += blk.numel()
        for i, r in enumerate(rr):
            for j, s in enumerate(ss):
                for h in range(ph, H, 2):
                    oh = (h + pad - r) // 2
                    if not 0 <= oh < Ho:
                        continue
                    for x_ in range(pw, W, 2):
                        ow = (x_ + pad - s) // 2
                        if 0 <= ow < Wo:
                            dx[:, h, x_] += dy[:, oh, ow] @ blk[:, i, j, :].t()
    assert off == flat.numel() == w.numel()
    assert torch.equal(dx, ref)


def test_finalize_tail_is_the_cnn_ops_finalize_of_the_sums():
    g = C.gen(3)
    Cc, Cp, nb, hw = 6, 8, [4, 2, 0], 35
    stats = torch.zeros(C.P, 2, Cp, dtype=F64)
    for p, n in enumerate(nb):
        v = torch.randn(max(n, 1) * hw, Cc, generator=g, dtype=F64) * (n > 0)
        stats[p, 0, :Cc], stats[p, 1, :Cc] = v.sum(0), (v * v).sum(0)
    gamma, beta = torch.rand(C.P, Cc, generator=g, dtype=F64) + 0.5, torch.randn(C.P, Cc, generator=g, dtype=F64)
    rm, rv = torch.full((C.P, Cc), 0.5, dtype=F64), torch.full((C.P, Cc), 2.0, dtype=F64)
    ss, ms, rm1, rv1 = C.fin_fwd(stats, nb, hw, gamma, beta, rm, rv, Cc, Cp, 1e-5, 0.1)
    for p, n in enumerate(nb):
        cnt = max(1, n * hw)
        mean = stats[p, 0, :Cc] / cnt
        var = (stats[p, 1, :Cc] / cnt - mean * mean).clamp_min(0)
        torch.testing.assert_close(ms[p, 0, :Cc], mean)
        torch.testing.assert_close(ss[p, 0, :Cc], gamma[p] / torch.sqrt(var + 1e-5))
        if n == 0:
            assert torch.equal(rm1[p], rm[p]) and torch.equal(rv1[p], rv[p])
        else:
            torch.testing.assert_close(rv1[p], 0.9 * rv[p] + 0.1 * var * cnt / (cnt - 1))
    assert float(ss[:, :, Cc:].abs().max()) == 0.0
    dgamma, dbeta, coef = C.fin_bwd(stats, nb, hw, gamma, ms, Cc, Cp)
    assert torch.equal(dgamma, stats[:, 1, :Cc]) and torch.equal(dbeta, stats[:, 0, :Cc])
    torch.testing.assert_close(coef[0, 1, :Cc], stats[0, 0, :Cc] / (nb[0] * hw))


# ---------------------------------------------------------------------------------------------
# the exact families are exact
# ---------------------------------------------------------------------------------------------
_units, _on_grid = C.units, C.on_grid


def _same(a, b):
    ok = ~torch.isnan(b)
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a.double()[ok], b[ok])


@pytest.mark.parametrize("family", C.FAMILIES)
@pytest.mark.parametrize("name", list(C.FWD))
def test_forward_family_is_exact_in_fp32(name, family):
    d = C.fwd_inputs(name, family)
    out, v, stats = C.fwd_oracle(d)
    ua, uw = _units(family, d["pro_ss"] is not None)
    unit = ua * uw
    a = d["x"] if d["pro_ss"] is None else C.prologue(d["x"], d["pro_ss"])
    assert _on_grid(a, ua) and _on_grid(d["w"], uw) and float(torch.nan_to_num(a).abs().max()) <= 256 * ua  # bf16 holds the operand
    assert torch.equal(a.float().to(torch.bfloat16).double(), a)
    mag = C.forward(a.abs(), d["w"].abs(), d["nb"], d["stride"], d["pad"], d["Ho"], d["Wo"], d["cpo"],
                    None if d["bias"] is None else d["bias"].abs(), None if d["resid"] is None else d["resid"].abs())[1]
    assert float(torch.nan_to_num(mag).max()) / unit < LIM  # every accumulator, bias and residual included
    rows = torch.nan_to_num(v).reshape(C.P, -1, d["cpo"])
    assert float(rows.abs().sum(1).max()) / unit < LIM  # sum x
    sq_exact = C.sq_exact(d, v)  # sum x^2: exact where the GPU test asserts equality
    if family == "ternary":
        assert sq_exact
    for order in (0, 1):
        o32, v32, s32 = C.fwd_oracle(d, dtype=F32, order=order)
        assert _same(v32, v) and _same(o32, out), f"order {order}"
        assert torch.equal(s32[:, 0].double(), stats[:, 0])
        if sq_exact:
            assert torch.equal(s32[:, 1].double(), stats[:, 1])
    assert float(stats[0].abs().max()) > 0


@pytest.mark.parametrize("family", C.FAMILIES)
@pytest.mark.parametrize("name", list(C.DGRAD))
def test_dgrad_family_is_exact_in_fp32(name, family):
    d = C.dgrad_inputs(name, family)
    out, v, sums = C.dgrad_oracle(d)
    ua, uw = _units(family, False)
    unit = ua * uw
    assert _on_grid(d["dy"], ua) and _on_grid(d["w"], uw)
    mag = C.dgrad(d["dy"].abs(), d["w"].abs(), d["nb"], d["H"], d["W"], d["stride"], d["pad"], d["cpi"], None if d["resid"] is None else d["resid"].abs())[1]
    assert float(torch.nan_to_num(mag).max()) / unit < LIM
    g = torch.nan_to_num(out).reshape(C.P, -1, d["cpi"])
    assert _on_grid(g, unit)  # the rounded gradient stays on the accumulator's grid (bf16 spacing >= unit above 2)
    assert float(g.abs().sum(1).max()) / unit < LIM  # sum g
    xh_exact = d["y0"] is not None and C.xhat_exact(d, out)  # exact where the GPU test asserts equality
    if family == "ternary" and d["y0"] is not None:
        assert xh_exact
    if family == "ternary":  # integers below 256: the bf16 rounding is the identity
        assert float(g.abs().max()) < 256
    for order in (0, 1):
        o32, v32, s32 = C.dgrad_oracle(d, dtype=F32, order=order)
        assert _same(v32, v) and _same(o32, out), f"order {order}"
        assert torch.equal(s32[:, 0].double(), sums[:, 0])
        if xh_exact:
            assert torch.equal(s32.double(), sums)
    assert float(torch.nan_to_num(out).abs().max()) > 0


@pytest.mark.parametrize("family", C.FAMILIES)
@pytest.mark.parametrize("kind,name", [(k, n) for k, t in (("fwd", C.FWD), ("dgrad", C.DGRAD), ("wgrad", C.WGRAD)) for n in t])
def test_single_element_changes_are_visible(kind, name, family):
    """The GPU test's sensitivity controls: what the kernel is compared with changes when one operand
    element moves by one grid unit (the rounded output alone, and with the sums it also produces)."""
    d = C.inputs(kind, name, family)
    base = C.oracle(kind, d)
    ctl = C.controls(kind, d)
    assert set(ctl) == {"corner", "lastk", "lastrow"}
    for label, over in ctl.items():
        assert C.differs(C.oracle(kind, d, **over), base), label


@pytest.mark.parametrize("family", C.FAMILIES)
@pytest.mark.parametrize("name", list(C.WGRAD))
def test_wgrad_family_is_exact_in_fp32(name, family):
    d = C.wgrad_inputs(name, family)
    gw = C.wgrad_oracle(d)
    ua, uw = _units(family, d["pro_ss"] is not None)
    unit = ua * uw
    a = d["x"] if d["pro_ss"] is None else C.prologue(d["x"], d["pro_ss"])
    assert _on_grid(a, ua) and _on_grid(d["dy"], uw) and torch.equal(a.float().to(torch.bfloat16).double(), a)
    mag = C.wgrad(d["dy"].abs(), a.abs(), d["nb"], d["R"], d["S"], d["stride"], d["pad"])
    # + the value the accumulating launches start from (the GPU test's BASE)
    assert (float(mag.max()) + C.BASE) / unit < LIM
    for order in (0, 1):
        assert torch.equal(C.wgrad_oracle(d, dtype=F32, order=order).double(), gw), f"order {order}"
    assert float(gw[0].abs().max()) > 0 and float(gw[2].abs().max()) == 0.0
    if d["cpo"] > d["cout"]:
        assert float(gw[:, d["cout"]:].abs().max()) == 0.0
    if d["cpi"] > d["cin"]:
        assert float(gw[..., d["cin"]:].abs().max()) == 0.0
