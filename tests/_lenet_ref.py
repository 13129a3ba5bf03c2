"""Plain float64 model of one fused LeNet-5 step (``csrc/kernels/lenet_fused.hip``: ``k_lenet_step<2>``
and ``k_lenet_fc_grad<2>`` behind ``lenet_fused_step``) for ``P`` peers, written from the definition
of each operation in the kernel's layouts. Index arithmetic only (``_conv_ref.conv_acc`` /
``conv_dgrad`` / ``conv_wgrad``, matrix products, ``_cnn_ops_ref.maxpool2`` / ``maxpool2_bwd`` /
``xent`` / ``sgd_update``): no torch convolution, no autograd. ``rnd`` is the rounding applied exactly
where the kernel stores bf16 (round to nearest even); ``rnd = ident`` switches every rounding off
(``tests/test_lenet_ref_cpu.py`` holds that form to ``myfyp_amd.models.LeNet5`` under autograd).

Layouts
-------
* shadow / ``gf`` (bf16 / fp32, "Wf"): conv ``[cp_out][tap][8]`` (c1: 8 x 25 x 8 with 6 x 25 x 3 real,
  c2: 16 x 25 x 8 with 16 x 25 x 6 real), fc1 ``[120][400]`` in ENGINE column order ``(y, x, c)``
  (engine column ``k`` is torch column ``E2T[k]``), fc2 ``[88][120]`` (84 real rows), fc3 ``[16][88]``
  (10 x 84 real); each at its ``w_*`` offset.
* params / ``g`` / momentum (fp32, torch order): weights at ``t_*`` (``[co][ci][tap]``, fc row-major),
  biases at ``b_*``.
* ``act`` per image: ``p2 | z3 | z4 | dz3 | dz4 | dlogits`` = 400 | 128 | 96 | 128 | 96 | 16 bf16 values.
* ``part``: one fp32 record per workgroup (2 images): ``dW1 [8][25][8] | dW2 [16][25][8] | db1 [16] | db2 [16]``.

Rules (the integer families hit every one of them constantly)
-------------------------------------------------------------
* a pooling window's gradient goes to its FIRST maximum in the order (0,0), (0,1), (1,0), (1,1);
* a pooled value ``max(acc) + bias <= 0`` passes nothing (the mask is ``> 0``);
* the fc ReLU masks are ``stored (bf16) activation > 0``;
* the predicted class is the first maximum of the logits;
* rows at or beyond ``valid = clamp(n_p - offset, 0, B)`` are a zero image with no label: the forward
  still runs on them (their activations are what the biases give), ``dlogits`` and everything behind it
  is zero for them.

Every backward stage is its own function of its upstream tensors, so the GPU test can feed it what
the kernel itself exported.
"""

import torch

import _cnn_ops_ref as O
import _conv_ref as C

F64 = torch.float64
P = 3
IPW = 2
IH, Z1, P1H, Z2, P2H = 32, 28, 14, 10, 5
F0, F1, F2, F3 = 400, 120, 84, 10
A_P2, A_Z3, A_Z4, A_DZ3, A_DZ4, A_DL, A_W = 0, 400, 528, 624, 752, 848, 864
PR_W1, PR_W2, PR_B1, PR_B2, PR_N = 0, 1600, 4800, 4816, 4832
NAN = float("nan")
LAYERS = ("c1", "c2", "f1", "f2", "f3")
# torch shapes [cout, cin, taps] and Wf shapes [cp_out, taps, cp_in]
TSHAPE = {"c1": (6, 3, 25), "c2": (16, 6, 25), "f1": (F1, F0, 1), "f2": (F2, F1, 1), "f3": (F3, F2, 1)}
WSHAPE = {"c1": (8, 25, 8), "c2": (16, 25, 8), "f1": (F1, 1, F0), "f2": (88, 1, F1), "f3": (16, 1, 88)}
# fc1: engine column (y, x, c) <-> torch column (c, y, x)
E2T = torch.tensor([(k % 16) * 25 + k // 16 for k in range(F0)])
T2E = torch.tensor([(t % 25) * 16 + t // 25 for t in range(F0)])
MAPS = {"f1": (E2T, T2E)}


def ident(t):
    return t


bf16 = C.bf16


def _numel(s):
    return s[0] * s[1] * s[2]


def layout():
    """Offsets of one peer's rows. Gaps of different sizes between the tensors; the shadow offsets keep
    the alignment the kernel's vector loads need (16 bytes), the torch-order ones are odd on purpose."""
    lay, o = {}, 8
    for i, n in enumerate(LAYERS):
        lay["w_" + n] = o
        o += _numel(WSHAPE[n]) + 8 * (i + 1)
    lay["shadow_n"] = o
    o = 3
    for i, n in enumerate(LAYERS):
        lay["t_" + n] = o
        o += _numel(TSHAPE[n]) + 2 + i
        lay["b_" + n] = o
        o += TSHAPE[n][0] + 1 + i
    lay["params_n"] = o
    return lay


LAY = layout()


# ---------------------------------------------------------------------------------------------
# parameters: torch-order dict <-> Wf layout <-> flat rows
# ---------------------------------------------------------------------------------------------
def to_wf(W, e2t=E2T):
    """Torch-order weights ``{layer: [P, cout, cin, taps]}`` -> Wf values ``{layer: [P, cp_out, taps, cp_in]}``
    (zero padding). ``e2t``: fc1's column map (a negative control passes the identity)."""
    out = {}
    for n in LAYERS:
        cpo, taps, cpi = WSHAPE[n]
        t = torch.zeros(W[n].shape[0], cpo, taps, cpi, dtype=F64)
        for p in range(W[n].shape[0]):
            t[p, : TSHAPE[n][0]] = O.wf_shadow(W[n][p].to(F64), cpi, e2t if n == "f1" else None)
        out[n] = t
    return out


def real_mask(n):
    """[cp_out, taps, cp_in] bool: the Wf positions that hold a real weight."""
    cout, cin, _ = TSHAPE[n]
    m = torch.zeros(WSHAPE[n], dtype=torch.bool)
    m[:cout, :, :cin] = True
    return m


def pack_wf(E, fill=NAN):
    """Wf dict -> [P, shadow_n]; ``fill`` in the gaps, and (if ``E`` holds NaN there) in the padding."""
    Pn = E["c1"].shape[0]
    out = torch.full((Pn, LAY["shadow_n"]), fill, dtype=F64)
    for n in LAYERS:
        out[:, LAY["w_" + n]: LAY["w_" + n] + _numel(WSHAPE[n])] = E[n].reshape(Pn, -1)
    return out


def unpack_wf(flat):
    """[P, shadow_n] -> Wf dict."""
    return {n: flat[:, LAY["w_" + n]: LAY["w_" + n] + _numel(WSHAPE[n])].reshape(flat.shape[0], *WSHAPE[n]) for n in LAYERS}


def pack_params(W, b, fill=NAN):
    """Torch-order weights and biases -> [P, params_n]."""
    Pn = W["c1"].shape[0]
    out = torch.full((Pn, LAY["params_n"]), fill, dtype=F64)
    for n in LAYERS:
        out[:, LAY["t_" + n]: LAY["t_" + n] + _numel(TSHAPE[n])] = W[n].reshape(Pn, -1)
        out[:, LAY["b_" + n]: LAY["b_" + n] + TSHAPE[n][0]] = b[n]
    return out


def unpack_params(flat):
    Pn = flat.shape[0]
    W = {n: flat[:, LAY["t_" + n]: LAY["t_" + n] + _numel(TSHAPE[n])].reshape(Pn, *TSHAPE[n]) for n in LAYERS}
    b = {n: flat[:, LAY["b_" + n]: LAY["b_" + n] + TSHAPE[n][0]] for n in LAYERS}
    return W, b


def wf_to_torch(E, t2e=T2E):
    """Wf-layout gradients -> torch order (``_cnn_ops_ref.wf_grad_to_torch`` per layer and peer)."""
    out = {}
    for n in LAYERS:
        cout, cin, _ = TSHAPE[n]
        out[n] = torch.stack([O.wf_grad_to_torch(E[n][p, :cout], cin, t2e if n == "f1" else None) for p in range(E[n].shape[0])])
    return out


def shadow_of(master_flat, e2t=E2T):
    """[P, params_n] master rows -> the unrounded shadow values [P, shadow_n]: NaN in the gaps and in
    every padding position (the fused optimizer writes real weights only). The caller rounds."""
    W, _ = unpack_params(master_flat)
    E = to_wf(W, e2t)
    for n in LAYERS:
        E[n][:, ~real_mask(n)] = NAN
    return pack_wf(E)


# ---------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------
def _pad_last(t, n):
    out = torch.zeros(*t.shape[:-1], n, dtype=F64)
    out[..., : t.shape[-1]] = t
    return out


def _per_peer(fn, *ts):
    return torch.stack([fn(*(t[p] for t in ts)) for p in range(ts[0].shape[0])])


def forward(x, E, b, rnd=bf16):
    """``x``: [P, B, 32, 32, 8] (``_cnn_ops_ref.input_prep``), ``E``: Wf weights, ``b``: biases {layer: [P, cout]}.
    conv + bias + ReLU + pool twice (the pool runs on the accumulators, the bias is added to the
    maximum), three fc layers. Returns every stored tensor and the accumulators the pooling looked at."""
    Pn, B = x.shape[:2]
    full = [B] * Pn
    r = {}
    r["acc1"] = _per_peer(lambda xp, w: C.conv_acc(xp, w.reshape(8, 5, 5, 8), 1, 0, Z1, Z1), x, E["c1"])
    m1 = O.maxpool2(r["acc1"], full) + _pad_last(b["c1"], 8)[:, None, None, None]
    r["live1"] = m1 > 0
    r["p1"] = rnd(m1.clamp_min(0))  # [P, B, 14, 14, 8], channels 6, 7 zero
    r["acc2"] = _per_peer(lambda a, w: C.conv_acc(a, w.reshape(16, 5, 5, 8), 1, 0, Z2, Z2), r["p1"], E["c2"])
    m2 = O.maxpool2(r["acc2"], full) + b["c2"][:, None, None, None]
    r["live2"] = m2 > 0  # [P, B, 5, 5, 16]
    r["p2"] = rnd(m2.clamp_min(0)).reshape(Pn, B, F0)  # engine order (y, x, c)
    r["z3"] = fc_fwd(r["p2"], E["f1"][:, :, 0], b["f1"], True, rnd)
    r["z4"] = fc_fwd(r["z3"], E["f2"][:, :F2, 0], b["f2"], True, rnd)
    r["logits"] = fc_fwd(r["z4"], E["f3"][:, :F3, 0, :F2], b["f3"], False, ident)  # fp32 in the kernel: not rounded
    return r


def fc_fwd(a, w, bias, relu, rnd=bf16):
    """``a`` [P, B, K] x ``w`` [P, N, K] + ``bias`` [P, N]."""
    v = torch.einsum("pbk,pnk->pbn", a, w) + bias[:, None]
    return rnd(v.clamp_min(0)) if relu else v


def head(logits, labels, valid, rnd=bf16):
    """``(loss sum [P], correct [P], confusion [P, 16, 16], dlogits [P, B, 16])`` over the valid rows;
    ``dlogits = rnd((softmax - onehot) / valid)``, zero in rows ``>= valid`` and columns ``>= 10``."""
    loss, correct, conf, dl = O.xent(_pad_last(logits, 16), labels, valid, F3)
    return loss, correct, conf, rnd(dl)


# ---------------------------------------------------------------------------------------------
# backward, one function per stage; each takes its upstream
# ---------------------------------------------------------------------------------------------
def fc_bwd(up, w, stored=None, rnd=bf16):
    """``up`` [P, B, N] x ``w`` [P, N, K]; with ``stored`` the ReLU mask ``stored > 0``."""
    g = torch.einsum("pbn,pnk->pbk", up, w)
    if stored is not None:
        g = torch.where(stored > 0, g, torch.zeros((), dtype=F64))
    return rnd(g)


def bwd_fc3(dl, z4, E, rnd=bf16):
    return fc_bwd(dl[..., :F3], E["f3"][:, :F3, 0, :F2], z4, rnd)


def bwd_fc2(dz4, z3, E, rnd=bf16):
    return fc_bwd(dz4, E["f2"][:, :F2, 0], z3, rnd)


def bwd_fc1(dz3, E):
    """dp2 [P, B, 400]: an fp32 accumulator in the kernel, not rounded."""
    return fc_bwd(dz3, E["f1"][:, :, 0], None, ident)


def pool_bwd(dp, acc, live, last=False):
    """Masked pooled gradient ``[P, B, h, w, C]`` -> ``(dz [P, B, 2h, 2w, C] unrounded, db [P, C])``.
    ``last``: route to the last maximum (negative control)."""
    Pn, B = dp.shape[:2]
    g = torch.where(live, dp, torch.zeros((), dtype=F64))
    return O.maxpool2_bwd(acc, g, [B] * Pn, last=last), g.sum((1, 2, 3))


def bwd_pool2(dp2, f, rnd=bf16, last=False):
    """``(dz2 = rnd(...) [P, B, 10, 10, 16], db2 [P, 16])``; the bias gradient sums the UNROUNDED dp2."""
    dz, db = pool_bwd(dp2.reshape(*dp2.shape[:2], P2H, P2H, 16), f["acc2"], f["live2"], last)
    return rnd(dz), db


def bwd_conv2_w(dz2, p1):
    """dW2 [P, 16, 25, 8] (Wf layout)."""
    return _per_peer(lambda d, a: C.conv_wgrad(d, a, 5, 5, 1, 0).reshape(16, 25, 8), dz2, p1)


def bwd_conv2_d(dz2, E, rnd=bf16):
    """dp1 = rnd(conv2 dgrad) [P, B, 14, 14, 8]."""
    return rnd(_per_peer(lambda d, w: C.conv_dgrad(d, w.reshape(16, 5, 5, 8), P1H, P1H, 1, 0), dz2, E["c2"]))


def bwd_pool1(dp1, f, last=False):
    """``(dz1 [P, B, 28, 28, 8], db1 [P, 8])``: dp1 is bf16 already, nothing is rounded again."""
    return pool_bwd(dp1, f["acc1"], f["live1"], last)


def bwd_conv1_w(dz1, x):
    """dW1 [P, 8, 25, 8] (Wf layout)."""
    return _per_peer(lambda d, a: C.conv_wgrad(d, a, 5, 5, 1, 0).reshape(8, 25, 8), dz1, x)


def fc_wgrad(dz, a):
    """Sums over the whole batch of the stored values: ``(dW [P, N, K], db [P, N])``."""
    return torch.einsum("pbn,pbk->pnk", dz, a), dz.sum(1)


def conv_backward(dz3, f, x, E, rnd=bf16, last=False):
    """Everything behind dz3: ``{dp2, dz2, dp1, dz1, gW1, gW2, gb1, gb2}``."""
    r = {"dp2": bwd_fc1(dz3, E)}
    r["dz2"], r["gb2"] = bwd_pool2(r["dp2"], f, rnd, last)
    r["m2"] = torch.where(f["live2"], r["dp2"].reshape(f["live2"].shape), torch.zeros((), dtype=F64))  # what db2 sums
    r["gW2"] = bwd_conv2_w(r["dz2"], f["p1"])
    r["dp1"] = bwd_conv2_d(r["dz2"], E, rnd)
    r["dz1"], r["gb1"] = bwd_pool1(r["dp1"], f, last)
    r["m1"] = torch.where(f["live1"], r["dp1"], torch.zeros((), dtype=F64))  # what db1 sums
    r["gW1"] = bwd_conv1_w(r["dz1"], x)
    return r


def fc_grads(blk, dtype=F64):
    """``blk`` {p2, z3, z4, dz3, dz4, dl}: [P, B, *] stored values -> fc weight / bias gradients."""
    t = {k: v.to(dtype) for k, v in blk.items()}
    g = {}
    g["gW_f1"], g["gb_f1"] = fc_wgrad(t["dz3"][..., :F1], t["p2"])
    g["gW_f2"], g["gb_f2"] = fc_wgrad(t["dz4"][..., :F2], t["z3"][..., :F1])
    g["gW_f3"], g["gb_f3"] = fc_wgrad(t["dl"][..., :F3], t["z4"][..., :F2])
    return g


def pack_grads(cv, fc):
    """Stage results -> ``(gf [P, shadow_n], g [P, params_n])`` as a gradients-only launch leaves them:
    NaN wherever the kernel writes nothing (gaps, padded channels / rows / columns, the weights' torch slots)."""
    Pn = cv["gW1"].shape[0]
    E = {n: torch.full((Pn, *WSHAPE[n]), NAN, dtype=F64) for n in LAYERS}
    E["c1"][:, :6, :, :3] = cv["gW1"][:, :6, :, :3]
    E["c2"][:, :, :, :6] = cv["gW2"][:, :, :, :6]
    E["f1"][:, :, 0] = fc["gW_f1"]
    E["f2"][:, :F2, 0] = fc["gW_f2"]
    E["f3"][:, :F3, 0, :F2] = fc["gW_f3"]
    g = torch.full((Pn, LAY["params_n"]), NAN, dtype=F64)
    for n, v in (("c1", cv["gb1"][:, :6]), ("c2", cv["gb2"]), ("f1", fc["gb_f1"]), ("f2", fc["gb_f2"]), ("f3", fc["gb_f3"])):
        g[:, LAY["b_" + n]: LAY["b_" + n] + TSHAPE[n][0]] = v
    return pack_wf(E), g


def grads_to_torch(gf, g, t2e=T2E):
    """A gradients-only launch's ``(gf, g)`` -> one torch-order row [P, params_n] (NaN in the gaps)."""
    W = wf_to_torch(unpack_wf(gf), t2e)
    _, b = unpack_params(g)
    return pack_params(W, b)


# ---------------------------------------------------------------------------------------------
# act block
# ---------------------------------------------------------------------------------------------
ACT_COLS = {"p2": (A_P2, F0), "z3": (A_Z3, 128), "z4": (A_Z4, 96), "dz3": (A_DZ3, 128), "dz4": (A_DZ4, 96), "dl": (A_DL, 16)}


def act_split(act):
    """[P, B, 864] -> {name: [P, B, width]} (z3 / dz3 padded to 128, z4 / dz4 to 96: padding is zero)."""
    return {k: act[..., o: o + n] for k, (o, n) in ACT_COLS.items()}


def act_pack(blk):
    Pn, B = blk["p2"].shape[:2]
    out = torch.zeros(Pn, B, A_W, dtype=F64)
    for k, (o, n) in ACT_COLS.items():
        out[..., o: o + blk[k].shape[-1]] = blk[k]
    return out


# ---------------------------------------------------------------------------------------------
# the fused optimizer step
# ---------------------------------------------------------------------------------------------
def opt_step(master, mom, grad, valid, hp, anchor=None, cg=None, cl=None, dtype=F64):
    """[P, params_n] rows (NaN in the gaps stays NaN): ``sgd_update`` per element for every peer with
    ``valid > 0``. Returns ``(master, mom)``; the shadow is ``bf16(shadow_of(master))``."""
    w, m = master.to(dtype).clone(), mom.to(dtype).clone()
    for p in range(master.shape[0]):
        if valid[p] <= 0:
            continue
        ex = {k: (v[p] if v is not None else None) for k, v in (("anchor", anchor), ("cg", cg), ("cl", cl))}
        w[p], m[p] = O.sgd_update(master[p], grad[p], mom[p], dtype=dtype, **hp, **ex)
    return w, m


OPT_VARIANTS = {
    # every constant is an fp32 value, so the kernel and the float64 oracle see the same hyperparameters
    "plain": dict(lr=0.125, momentum=0.0, weight_decay=0.0, nesterov=False, mu=0.0),
    "momentum_nesterov_wd": dict(lr=0.0625, momentum=0.875, weight_decay=0.015625, nesterov=True, mu=0.0),
    "fedprox": dict(lr=0.0625, momentum=0.0, weight_decay=0.0, nesterov=False, mu=0.25),
    "scaffold": dict(lr=0.0625, momentum=0.5, weight_decay=0.0, nesterov=False, mu=0.0),
}


# ---------------------------------------------------------------------------------------------
# exactness: sum |term| / unit of an accumulation
# ---------------------------------------------------------------------------------------------
def lowbit(t):
    """Per element: the value of the lowest set bit of a float64 (inf for 0)."""
    m, e = torch.frexp(t.to(F64))
    n = (m.abs() * 2.0 ** 53).to(torch.int64)
    low = (n & -n).to(F64) * torch.ldexp(torch.ones_like(m), e - 53)
    return torch.where(t == 0, torch.full_like(low, float("inf")), low)


def gunit(t, dims=None):
    """The coarsest power-of-two grid that holds every element (over ``dims``; 1.0 for all-zero)."""
    u = lowbit(t)
    u = u.amin(dims) if dims is not None else u.min()
    return torch.where(torch.isinf(u), torch.ones_like(u), u)


def mm_ratio(a, w):
    """``a`` [P, B, N] x ``w`` [P, N, K]: the worst ``sum |term| / unit`` over the output elements; the
    unit is (grid of the row of ``a``) x (grid of the peer's ``w``): one output row only sees its own ``a`` row."""
    s = torch.einsum("pbn,pnk->pbk", a.abs(), w.abs()).amax(2)
    return float((s / (gunit(a, 2) * gunit(w, (1, 2))[:, None])).max())


def conv_ratio(kind, a, w_or_b, *geom):
    """The same for a convolution, per image. ``kind`` fwd: conv_acc(a, w); dgrad: conv_dgrad(a, w)."""
    fn = C.conv_acc if kind == "fwd" else C.conv_dgrad
    worst = 0.0
    for p in range(a.shape[0]):
        s = fn(a[p].abs(), w_or_b[p].abs(), *geom).amax((1, 2, 3))
        worst = max(worst, float((s / (gunit(a[p], (1, 2, 3)) * gunit(w_or_b[p]))).max()))
    return worst


def stage_ratios(r, E, dl=None, dz4=None, dz3=None):
    """``sum |term| / unit`` of every accumulation compared bit for bit, on the given upstreams (default:
    the oracle's own)."""
    dl = r["dl"] if dl is None else dl
    dz4 = r["dz4"] if dz4 is None else dz4
    dz3 = r["dz3"] if dz3 is None else dz3
    P = r["x"].shape[0]
    w1, w2 = E["c1"].reshape(P, 8, 5, 5, 8), E["c2"].reshape(P, 16, 5, 5, 8)
    f1, f2, f3 = E["f1"][:, :, 0], E["f2"][:, :F2, 0], E["f3"][:, :F3, 0, :F2]
    return {
        "conv1": conv_ratio("fwd", r["x"], w1, 1, 0, Z1, Z1),
        "conv2": conv_ratio("fwd", r["p1"], w2, 1, 0, Z2, Z2),
        "fc1": mm_ratio(r["p2"], f1.transpose(1, 2)),
        "fc2": mm_ratio(r["z3"][..., :F1], f2.transpose(1, 2)),
        "fc3": mm_ratio(r["z4"][..., :F2], f3.transpose(1, 2)),
        "dl.W3": mm_ratio(dl[..., :F3], f3),
        "dz4.W2": mm_ratio(dz4[..., :F2], f2),
        "dz3.W1": mm_ratio(dz3[..., :F1], f1),
        "conv2 dgrad": conv_ratio("dgrad", bwd_pool2(bwd_fc1(dz3, E), r)[0], w2, P1H, P1H, 1, 0),
    }


EXACT_LIM = C.LIM / 16  # headroom: the kernel's dlogits may sit one bf16 ulp off the oracle's


# ---------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------
OFFSET = 5
BATCHES = (2, 8, 66)
ODD_VALID = {2: 1, 8: 3, 66: 37}
EXACT_FAMILIES = ("pix3", "pix7")
CASES = [(B, fam) for B in BATCHES for fam in EXACT_FAMILIES] + [(8, "randn")]
EVAL_CASES = [(2, "pix7"), (8, "pix3"), (66, "pix7")]  # ``case(..., train=False)``: identity order, other data
DENSITY = {"c1": 0.5, "c2": 0.3, "f1": 0.1, "f2": 0.25, "f3": 0.5}
F3_SCALE = 2.0 ** -14
CONV_BIAS = {"pix3": -6.0, "pix7": -14.0}  # the maximum of four symmetric sums is positive 85 % of the time: shift the conv biases


def _sparse_ternary(g, density, *shape):
    return C.ternary(g, *shape) * (torch.rand(*shape, generator=g) < density)


def weights(family, seed):
    """``(W, b)`` in torch order, float64, every value a bf16 (so master = shadow). Exact families:
    sparse ternary weights, ternary biases, fc3 times 2^-11. randn: normals scaled by 1 / sqrt(K)."""
    g = C.gen(seed)
    W, b = {}, {}
    for n in LAYERS:
        cout, cin, taps = TSHAPE[n]
        if family == "randn":
            W[n] = C.normal(g, P, cout, cin, taps, scale=(cin * taps) ** -0.5)
            b[n] = C.normal(g, P, cout, scale=0.1)
        else:
            s = F3_SCALE if n == "f3" else 1.0
            W[n] = _sparse_ternary(g, DENSITY[n], P, cout, cin, taps) * s
            b[n] = C.ternary(g, P, cout) * s + (CONV_BIAS[family] if n in ("c1", "c2") else 0.0)
    return W, b


def case(B, family, train=True):
    """One launch's inputs: 3 peers with ``valid = [B, odd, 0]`` (the last because ``offset >= n``), a
    non-identity permutation (``train``; evaluation reads rows ``offset + b``), and 255 / label -7 in
    every dataset row no valid batch index reaches."""
    seed = 1000 * B + sum(map(ord, family)) + (0 if train else 7)
    g = C.gen(seed)
    valid = [B, ODD_VALID[B], 0]
    n = [OFFSET + B + 3, OFFSET + ODD_VALID[B], OFFSET - 2]
    nmax = max(n)
    hi = {"pix3": 4, "pix7": 8, "randn": 256}[family]
    xs, ys, perm = [], [], torch.zeros(P, nmax, dtype=torch.int64)
    for p in range(P):
        pm = torch.randperm(n[p], generator=g)
        if train and valid[p] > 0:
            assert not torch.equal(pm, torch.arange(n[p]))
        x = torch.full((n[p], IH, IH, 3), 255, dtype=torch.uint8)
        y = torch.full((n[p],), -7, dtype=torch.int64)
        for bb in range(valid[p]):
            idx = int(pm[OFFSET + bb]) if train else OFFSET + bb
            # noise under a random 4 x 4 block mask per channel: images that differ in structure, so the
            # predicted class varies over the batch
            keep = (torch.rand(4, 4, 3, generator=g) < 0.6).repeat_interleave(8, 0).repeat_interleave(8, 1)
            x[idx] = (torch.randint(0, hi, (IH, IH, 3), generator=g) * keep).to(torch.uint8)
            y[idx] = int(torch.randint(0, F3, (1,), generator=g))
        perm[p, : n[p]] = pm
        perm[p, n[p]:] = pm[0]  # padding of the permutation row: a poisoned dataset row (position 0 < offset)
        xs.append(x)
        ys.append(y)
    W, b = weights(family, seed + 1)
    scale = 1.0 / 255 if family == "randn" else 1.0
    # every other valid row is labelled with the class the oracle predicts, the rest with another one:
    # the correct count is neither zero nor the batch
    x, _, nb = O.input_prep(xs, ys, perm if train else None, OFFSET, B, 3, 8, scale)
    pred = forward(x, to_wf(W), b)["logits"].argmax(2)
    for p in range(P):
        for bb in range(valid[p]):
            idx = int(perm[p, OFFSET + bb]) if train else OFFSET + bb
            if bb % 2 == 0:
                ys[p][idx] = int(pred[p, bb])
            elif int(ys[p][idx]) == int(pred[p, bb]):
                ys[p][idx] = (int(pred[p, bb]) + 1) % F3
    return dict(B=B, family=family, train=train, valid=valid, n=n, offset=OFFSET, scale=scale, xs=xs, ys=ys, perm=perm if train else None, W=W, b=b)


def oracle(c, rnd=bf16, E=None, **over):
    """The whole step on case ``c`` (overrides: ``xs``, ``ys``, ``W``, ``b``): forward tensors, head, every
    backward stage from the oracle's own upstream, ``gf`` / ``g`` and the ``act`` block."""
    k = dict(c, **over)
    x, labels, nb = O.input_prep(k["xs"], k["ys"], k["perm"], k["offset"], k["B"], 3, 8, k["scale"])
    if rnd is ident:  # the unrounded model sees the unrounded input too
        x = torch.zeros_like(x)
        for p in range(P):
            for bb in range(nb[p]):
                idx = int(k["perm"][p][k["offset"] + bb]) if k["perm"] is not None else k["offset"] + bb
                x[p, bb, :, :, :3] = k["xs"][p][idx].double() * k["scale"]
    E = to_wf(k["W"]) if E is None else E
    r = dict(x=x, labels=labels, nb=nb, E=E)
    r.update(forward(x, E, k["b"], rnd))
    r["loss"], r["correct"], r["conf"], r["dl"] = head(r["logits"], labels, nb, rnd)
    r["dz4"] = bwd_fc3(r["dl"], r["z4"], E, rnd)
    r["dz3"] = bwd_fc2(r["dz4"], r["z3"], E, rnd)
    r.update(conv_backward(r["dz3"], r, x, E, rnd))
    r["blk"] = {"p2": r["p2"], "z3": r["z3"], "z4": r["z4"], "dz3": r["dz3"], "dz4": r["dz4"], "dl": r["dl"]}
    r.update(fc_grads(r["blk"]))
    r["gf"], r["g"] = pack_grads(r, r)
    r["act"] = act_pack(r["blk"])
    return r


def results(r):
    """What a launch leaves behind, as a tuple for ``_conv_ref.differs``."""
    return (r["act"], r["gf"], r["g"], r["loss"], r["correct"])


def single_changes(c, r):
    """{label: overrides for ``_lenet_ref.oracle``}: one pixel, one weight per layer, one label. An fc
    weight is taken between a live input and a live output unit of peer 0's first image."""
    idx = int(c["perm"][0, c["offset"]]) if c["perm"] is not None else c["offset"]
    xs = [t.clone() for t in c["xs"]]
    xs[0][idx, 16, 16, 1] += 1
    ys = [t.clone() for t in c["ys"]]
    ys[0][idx] = (int(ys[0][idx]) + 1) % F3
    out = {"pixel": {"xs": xs}, "label": {"ys": ys}}
    for n in LAYERS:
        unit = F3_SCALE if n == "f3" else 1.0
        co, ci, tap = 1, 1, 12
        if n[0] == "f":
            src, dst = {"f1": ("p2", "z3"), "f2": ("z3", "z4"), "f3": ("z4", "z4")}[n]
            ci, co, tap = int(r[src][0, 0].nonzero()[0]), int(r[dst][0, 0].nonzero()[0]) % TSHAPE[n][0], 0
            ci = int(E2T[ci]) if n == "f1" else ci
        out["w_" + n] = {"W": dict(c["W"], **{n: C.bump(c["W"][n], (0, co, ci, tap), unit)})}
    return out
