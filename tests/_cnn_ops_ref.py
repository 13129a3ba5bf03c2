"""Plain references of the CNN companion kernels (``csrc/kernels/cnn_ops.hip``), one per kernel,
written from the definition of each op in the engine's layout: NHWC with the channels padded to
``Cp``, one slab per peer, ``nb[p]`` valid samples per peer.

Conventions shared by every function here:

* tensors are dense CPU tensors with a leading peer axis (``[P, rows, Cp]``, ``[P, B, H, W, Cp]``);
  the GPU tests place them into strided device buffers themselves;
* ``dtype`` is the precision the formula is evaluated in: float64 is the oracle, float32 is the
  "plain torch fp32 evaluation" whose distance to the oracle sizes the fp32 tolerances;
* an output element the kernel must leave alone (rows at or beyond ``nb[p] * hw``, the whole slab of
  a peer with ``nb = 0``, the last row / column of an odd max-pool input) is NaN in the reference:
  the tests pre-fill their outputs with a sentinel and require it to survive exactly there.
"""

import torch

NAN = float("nan")


# ---------------------------------------------------------------------------------------------
# tolerances
# ---------------------------------------------------------------------------------------------
def ulp_bf16(v):
    """Spacing of bf16 (8 significant bits) at ``|v|``; the smallest normal spacing at zero."""
    _, e = torch.frexp(v.double().abs().clamp_min(2.0 ** -126))  # |v| = m * 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(v, dtype=torch.float64), e - 8)


def bf16_bound(ref64, big):
    """|out - ref64| allowed for a bf16 output computed in fp32: one bf16 ulp (half an ulp of RNE plus
    one rounding boundary the fp32 error may cross) + 2^-20 * M, M = the element's largest |term|."""
    return ulp_bf16(ref64) + 2.0 ** -20 * big


def fp32_bound(ref64, ref32):
    """Four times the largest error of the plain fp32 evaluation, floored at 2^-22 * max|ref64|."""
    ok = ~torch.isnan(ref64)
    err = float((ref32.double() - ref64)[ok].abs().max()) if ok.any() else 0.0
    top = float(ref64[ok].abs().max()) if ok.any() else 0.0
    return max(4.0 * err, 2.0 ** -22 * top)


# ---------------------------------------------------------------------------------------------
# input gather
# ---------------------------------------------------------------------------------------------
def input_prep(xs, ys, perm, offset, B, C, Cp, scale, stopped=None):
    """``xs[p]``: uint8 ``[n_p, H, W, C]``, ``ys[p]``: int64 ``[n_p]``, ``perm``: ``[P, n]`` or None.
    Sample ``b`` of peer ``p`` is dataset row ``perm[p][offset + b]`` (``offset + b`` without a
    permutation); ``valid = clamp(n_p - offset, 0, B)`` rows exist, the rest of the batch is zero.
    Returns ``out`` (bf16 values ``[P, B, H, W, Cp]``, exactly ``bf16(fp32(scale) * u8)``), ``labels``
    (``[P, B]``, -1 = not written) and ``nb``. A stopped peer reports ``nb = 0``; its batch is staged
    all the same and simply not used."""
    P = len(xs)
    H, W = xs[0].shape[1:3]
    out = torch.zeros(P, B, H, W, Cp, dtype=torch.float64)
    labels = torch.full((P, B), -1, dtype=torch.int64)
    nb = []
    s32 = torch.tensor(scale, dtype=torch.float32).double()
    for p in range(P):
        valid = max(0, min(B, xs[p].shape[0] - offset))
        for b in range(valid):
            idx = int(perm[p][offset + b]) if perm is not None else offset + b
            # the fp32 product is the exact product rounded once to fp32, then once more to bf16
            out[p, b, :, :, :C] = (s32 * xs[p][idx].double()).float().to(torch.bfloat16).double()
            labels[p, b] = ys[p][idx]
        nb.append(0 if stopped is not None and stopped[p] else valid)
    return out, labels, nb


# ---------------------------------------------------------------------------------------------
# BatchNorm forward
# ---------------------------------------------------------------------------------------------
def _padded(v, Cp, dtype):
    """[P, C] -> [P, Cp], zero in the padding channels."""
    out = torch.zeros(v.shape[0], Cp, dtype=dtype)
    out[:, : v.shape[1]] = v.to(dtype)
    return out


def bn_finalize(stats, nb, hw, gamma, beta, rmean, rvar, C, Cp, eps, momentum, train, dtype=torch.float64, count=None):
    """``stats``: ``[P, rows, 2, Cp]`` partial (sum, sum of squares) rows. Training: batch mean and
    biased variance over ``cnt = nb * hw`` elements, running statistics moved by ``momentum`` towards
    the mean and the *unbiased* variance (``cnt = 1``: the biased one) unless the peer has no sample;
    evaluation: the running statistics. Returns ``ss`` = (scale, shift) and ``ms`` = (mean, 1/std),
    both ``[P, 2, Cp]`` with zero padding channels, the new running statistics and the new ``stats``
    (re-zeroed in training, untouched in evaluation). ``count`` overrides the divisor (negative
    controls)."""
    P = stats.shape[0]
    ss = torch.zeros(P, 2, Cp, dtype=dtype)
    ms = torch.zeros(P, 2, Cp, dtype=dtype)
    rm, rv = rmean.to(dtype).clone(), rvar.to(dtype).clone()
    g, b = gamma.to(dtype), beta.to(dtype)
    for p in range(P):
        if train:
            n = nb[p] * hw
            cnt = max(1, n) if count is None else count(n)
            s = stats[p, :, 0, :C].to(dtype).sum(0)
            sq = stats[p, :, 1, :C].to(dtype).sum(0)
            mean = s / cnt
            var = (sq / cnt - mean * mean).clamp_min(0)
            if n > 0:
                unbiased = var * cnt / (cnt - 1) if cnt > 1 else var
                rm[p] = (1 - momentum) * rm[p] + momentum * mean
                rv[p] = (1 - momentum) * rv[p] + momentum * unbiased
        else:
            mean, var = rm[p], rv[p]
        inv = 1 / torch.sqrt(var + eps)
        ss[p, 0, :C] = g[p] * inv
        ss[p, 1, :C] = b[p] - mean * g[p] * inv
        ms[p, 0, :C] = mean
        ms[p, 1, :C] = inv
    new_stats = torch.zeros_like(stats) if train else stats.clone()
    return ss, ms, rm, rv, new_stats


def _blank_tail(out, nb, hw):
    for p, n in enumerate(nb):
        out[p, n * hw:] = NAN
    return out


def bn_act(y, ss, res, y2, ss2, relu, nb, hw, dtype=torch.float64):
    """``out = act(y * scale + shift [+ res] [+ y2 * scale2 + shift2])`` on rows ``< nb * hw`` of
    ``[P, rows, Cp]``. Returns ``(out, M)``, M = the largest |term| of each element."""
    sc, sh = ss[:, None, 0].to(dtype), ss[:, None, 1].to(dtype)
    terms = [y.to(dtype) * sc, sh.expand_as(y)]
    if res is not None:
        terms.append(res.to(dtype))
    if y2 is not None:
        terms += [y2.to(dtype) * ss2[:, None, 0].to(dtype), ss2[:, None, 1].to(dtype).expand_as(y)]
    out = sum(terms)
    if relu:
        out = out.clamp_min(0)
    big = torch.stack([t.abs() for t in terms]).max(0).values
    return _blank_tail(out.clone(), nb, hw), big


# ---------------------------------------------------------------------------------------------
# BatchNorm backward
# ---------------------------------------------------------------------------------------------
def bn_bwd_g(dz, mask, y, mss, nb, hw, dtype=torch.float64, live=None):
    """The gradient that reaches the BatchNorm output: ``dz`` where the following ReLU was live
    (``mask > 0``, or ``y * sc + sh > 0`` recomputed from ``mss`` = that BN's (scale, shift)), all of
    ``dz`` without a ReLU. Returns ``(g, margin)``; ``margin`` is ``|y * sc + sh|`` for the ``mss``
    form (None otherwise). ``live`` overrides the comparison (negative controls)."""
    live = live or (lambda t: t > 0)
    margin = None
    if mss is not None:
        a = y.to(dtype) * mss[:, None, 0].to(dtype) + mss[:, None, 1].to(dtype)
        keep, margin = live(a), a.abs()
    elif mask is not None:
        keep = live(mask.to(dtype))
    else:
        keep = torch.ones_like(dz, dtype=torch.bool)
    g = torch.where(keep, dz.to(dtype), torch.zeros((), dtype=dtype))
    return _blank_tail(g, nb, hw), margin


def bn_bwd_sums(g, y, ms, nb, hw, dtype=torch.float64):
    """``(sum g, sum g * xhat)`` over the valid rows, ``xhat = (y - mean) / std``: ``[P, 2, Cp]``."""
    P, _, Cp = g.shape
    out = torch.zeros(P, 2, Cp, dtype=dtype)
    for p in range(P):
        r = nb[p] * hw
        gp = g[p, :r].to(dtype)
        xh = (y[p, :r].to(dtype) - ms[p, 0].to(dtype)) * ms[p, 1].to(dtype)
        out[p, 0] = gp.sum(0)
        out[p, 1] = (gp * xh).sum(0)
    return out


def bn_bwd_finalize(sums, nb, hw, gamma, ms, C, Cp, dtype=torch.float64, count=None):
    """``sums``: ``[P, 2, Cp]``, or partial rows ``[P, rows, 2, Cp]`` that are added up first.
    ``dgamma = sum g * xhat``, ``dbeta = sum g`` (``[P, C]``, to be *added* to the gradient) and the
    apply coefficients ``coef = (gamma / std, sum g / cnt, sum g * xhat / cnt)`` (``[P, 3, Cp]``, zero
    padding channels), ``cnt = max(1, nb * hw)``."""
    P = sums.shape[0]
    coef = torch.zeros(P, 3, Cp, dtype=dtype)
    s = sums.to(dtype)
    if s.dim() == 4:
        s = s.sum(1)
    for p in range(P):
        cnt = max(1, nb[p] * hw) if count is None else count(nb[p] * hw)
        coef[p, 0, :C] = gamma[p].to(dtype) * ms[p, 1, :C].to(dtype)
        coef[p, 1, :C] = s[p, 0, :C] / cnt
        coef[p, 2, :C] = s[p, 1, :C] / cnt
    return s[:, 1, :C].clone(), s[:, 0, :C].clone(), coef


def bn_bwd_apply(g, y, ms, coef, nb, hw, dtype=torch.float64):
    """``dy = (gamma / std) * (g - mean(g) - xhat * mean(g * xhat))``. Returns ``(dy, M)``."""
    mean, inv = ms[:, None, 0].to(dtype), ms[:, None, 1].to(dtype)
    k1, mg, mgx = (coef[:, None, i].to(dtype) for i in range(3))
    gg = torch.nan_to_num(g.to(dtype), nan=0.0)
    xh = (y.to(dtype) - mean) * inv
    terms = [k1 * gg, (k1 * mg).expand_as(gg), k1 * xh * mgx]
    dy = k1 * (gg - mg - xh * mgx)
    big = torch.stack([t.abs() for t in terms]).max(0).values
    return _blank_tail(dy.clone(), nb, hw), big


def relu_bwd(dz, mask, nb, hw, dtype=torch.float64):
    return bn_bwd_g(dz, mask, None, None, nb, hw, dtype)[0]


def colsum(x, nb, hw, C, dtype=torch.float64, drop_last=False):
    """Column sums over the valid rows, channels ``< C``: ``[P, C]``."""
    out = torch.zeros(x.shape[0], C, dtype=dtype)
    for p in range(x.shape[0]):
        r = nb[p] * hw - (1 if drop_last and nb[p] > 0 else 0)
        out[p] = x[p, :r, :C].to(dtype).sum(0)
    return out


# ---------------------------------------------------------------------------------------------
# pooling
# ---------------------------------------------------------------------------------------------
def windows(x):
    """[P, B, H, W, Cp] -> the four window members, order (0,0), (0,1), (1,0), (1,1): [4, P, B, Ho, Wo, Cp]."""
    Ho, Wo = x.shape[2] // 2, x.shape[3] // 2
    return torch.stack([x[:, :, dh:2 * Ho:2, dw:2 * Wo:2] for dh in (0, 1) for dw in (0, 1)])


def maxpool2(x, nb, dtype=torch.float64):
    """2x2 / stride 2 max pool (floor: an odd last row / column is dropped): [P, B, Ho, Wo, Cp]."""
    out = windows(x.to(dtype)).max(0).values
    for p, n in enumerate(nb):
        out[p, n:] = NAN
    return out


def maxpool2_bwd(x, dy, nb, dtype=torch.float64, last=False):
    """``dy`` goes to the first maximal member of its window in the order (0,0), (0,1), (1,0), (1,1),
    the other three members get zero; an odd last row / column belongs to no window and is not
    written. ``last``: route to the last maximum instead (negative control)."""
    w = windows(x.to(dtype))
    hit = w == w.max(0).values
    if last:
        hit = hit.flip(0)
    first = hit & (hit.cumsum(0) == 1)
    if last:
        first = first.flip(0)
    dx = torch.full(x.shape, NAN, dtype=dtype)
    Ho, Wo = x.shape[2] // 2, x.shape[3] // 2
    k = 0
    for dh in (0, 1):
        for dw in (0, 1):
            dx[:, :, dh:2 * Ho:2, dw:2 * Wo:2] = torch.where(first[k], dy.to(dtype), torch.zeros((), dtype=dtype))
            k += 1
    for p, n in enumerate(nb):
        dx[p, n:] = NAN
    return dx


def avgpool(x, nb, dtype=torch.float64):
    """Global average over ``hw``: ``[P, B, hw, Cp] -> [P, B, Cp]``. Returns ``(out, M)``."""
    xd = x.to(dtype)
    out = xd.sum(2) / x.shape[2]
    big = xd.abs().sum(2)  # the running sum is the largest intermediate
    for p, n in enumerate(nb):
        out[p, n:] = NAN
    return out, big


def avgpool_bwd(dy, nb, hw, dtype=torch.float64):
    """``[P, B, Cp] -> [P, B, hw, Cp]``, every position gets ``dy / hw``. Returns ``(dx, M)``."""
    dx = (dy.to(dtype) / hw)[:, :, None].expand(-1, -1, hw, -1).clone()
    big = dy.to(dtype).abs()[:, :, None].expand(-1, -1, hw, -1).clone()
    for p, n in enumerate(nb):
        dx[p, n:] = NAN
    return dx, big


# ---------------------------------------------------------------------------------------------
# log-softmax + NLL head
# ---------------------------------------------------------------------------------------------
def xent(logits, labels, nb, K, dtype=torch.float64):
    """``logits``: ``[P, B, Lp]`` (classes ``< K``), ``labels``: ``[P, B]``. Per peer: the loss *sum* and
    the number of correct rows over the ``nb`` valid rows, the confusion matrix ``[16, 16]`` indexed
    (label, prediction), and ``dlogits = (softmax - onehot) / nb``, zero in rows ``>= nb`` and columns
    ``>= K``. Returns ``(loss [P], correct [P], confusion [P, 16, 16], dlogits [P, B, Lp])``."""
    P, B, Lp = logits.shape
    loss = torch.zeros(P, dtype=dtype)
    correct = torch.zeros(P, dtype=dtype)
    conf = torch.zeros(P, 16, 16, dtype=torch.int64)
    dl = torch.zeros(P, B, Lp, dtype=dtype)
    for p in range(P):
        n = nb[p]
        for b in range(n):
            z = logits[p, b, :K].to(dtype)
            y = int(labels[p, b])
            lse = torch.logsumexp(z, 0)
            loss[p] += lse - z[y]
            pred = int(torch.argmax(z))
            correct[p] += float(pred == y)
            conf[p, y, pred] += 1
            sm = torch.exp(z - lse)
            sm[y] -= 1
            dl[p, b, :K] = sm / n
    return loss, correct, conf, dl


# ---------------------------------------------------------------------------------------------
# optimizer + bf16 weight shadow
# ---------------------------------------------------------------------------------------------
def sgd_update(w, g, m, lr, momentum=0.0, weight_decay=0.0, nesterov=False, mu=0.0, anchor=None, cg=None, cl=None, dtype=torch.float64):
    """One SGD step on flat tensors (torch.optim.SGD semantics, momentum buffer starting at zero):
    FedProx adds ``mu * (w - anchor)`` to the gradient, weight decay adds ``wd * w``, then momentum
    (``m = momentum * m + g``; Nesterov steps along ``g + momentum * m``), ``w -= lr * step``; SCAFFOLD's
    correction is applied in the update space, ``w -= lr * (cg - cl)``. Returns ``(w, m)``."""
    w0, g, m = w.to(dtype), g.to(dtype), m.to(dtype)
    if anchor is not None and mu != 0.0:
        g = g + mu * (w0 - anchor.to(dtype))
    if weight_decay != 0.0:
        g = g + weight_decay * w0
    if momentum != 0.0:
        m = momentum * m + g
        g = g + momentum * m if nesterov else m
    w1 = w0 - lr * g
    if cg is not None:
        w1 = w1 - lr * (cg.to(dtype) - cl.to(dtype))
    return w1, m


def wf_grad_to_torch(gf, cin, t2e=None):
    """Gradient of one conv / fc layer in the shadow's layout ``[cout, R*S, cp_in]`` -> torch order
    ``[cout, cin, R*S]``: torch input channel ``ct`` is engine channel ``t2e[ct]`` (``ct`` without a map)."""
    cols = torch.as_tensor(t2e, dtype=torch.int64) if t2e is not None else torch.arange(cin)
    return gf[:, :, cols].permute(0, 2, 1)


def wf_shadow(w, cp_in, e2t=None):
    """Master weights ``[cout, cin, R*S]`` (torch order) -> shadow values ``[cout, R*S, cp_in]``: engine
    channel ``ci`` holds torch channel ``e2t[ci]`` (``ci`` itself without a map), zero where the map is
    negative or ``ci >= cin``. The caller rounds to bf16."""
    cout, cin, rs = w.shape
    out = torch.zeros(cout, rs, cp_in, dtype=w.dtype)
    for ci in range(cp_in):
        tc = int(e2t[ci]) if e2t is not None else (ci if ci < cin else -1)
        if tc >= 0:
            out[:, :, ci] = w[:, tc, :]
    return out


def opt_step(w, g, m, gf, shadow, segs, hp, active, update, anchor=None, cg=None, cl=None, dtype=torch.float64):
    """The whole fused pass on ``[P, ps]`` buffers. ``segs``: dicts with ``off, n, kind, cout, cin, R, S,
    cp_in, zero_after, wf_off, e2t, t2e``; a plain segment (kind 0) takes its gradient from ``g`` at
    ``off``, a conv / fc segment (kind 1) from ``gf`` at ``wf_off`` in the shadow's layout. Inactive
    peers are left alone; ``update = 0`` only refreshes the shadows from the weights. Returns new
    ``(w, g, m, gf, shadow)``; ``shadow`` holds unrounded values in the positions it covers."""
    w, g, m, gf, shadow = w.to(dtype).clone(), g.to(dtype).clone(), m.to(dtype).clone(), gf.to(dtype).clone(), shadow.to(dtype).clone()
    for p in range(w.shape[0]):
        if active is not None and not active[p]:
            continue
        for s in segs:
            sl = slice(s["off"], s["off"] + s["n"])
            extra = {k: (v[p, sl] if v is not None else None) for k, v in (("anchor", anchor), ("cg", cg), ("cl", cl))}
            if s["kind"] == 0:
                if update:
                    w[p, sl], m[p, sl] = sgd_update(w[p, sl], g[p, sl], m[p, sl], dtype=dtype, **hp, **extra)
                    if s["zero_after"]:
                        g[p, sl] = 0
                continue
            rs, nf = s["R"] * s["S"], s["cout"] * s["R"] * s["S"] * s["cp_in"]
            fl = slice(s["wf_off"], s["wf_off"] + nf)
            if update:
                gt = wf_grad_to_torch(gf[p, fl].reshape(s["cout"], rs, s["cp_in"]), s["cin"], s["t2e"]).reshape(-1)
                w[p, sl], m[p, sl] = sgd_update(w[p, sl], gt, m[p, sl], dtype=dtype, **hp, **extra)
                if s["zero_after"]:
                    gf[p, fl] = 0
            shadow[p, fl] = wf_shadow(w[p, sl].reshape(s["cout"], s["cin"], rs), s["cp_in"], s["e2t"]).reshape(-1)
    return w, g, m, gf, shadow
