"""Plain references of the implicit-GEMM convolution kernels (``csrc/kernels/conv.hip``), written
from the definition of each operation in the engine's layouts:

* activations ``[n, H, W, Cp]`` (NHWC, ``Cp = round_up(C, 8)``, padding channels zero);
* the weight shadow ``Wf[Cp_out, R, S, Cp_in]`` and the weight gradient in the same layout;
* one slab per peer (leading peer axis), ``nb[p]`` valid samples per peer.

Everything is index arithmetic over the taps in ``dtype`` (float64 is the oracle, float32 the plain
evaluation that sizes the fp32 tolerances and proves the exact input families exact); no torch
convolution is called. ``H, W, R, S`` are separate everywhere. An output element the kernel must
leave alone (samples at or beyond ``nb[p]``) is NaN, as in ``_cnn_ops_ref``.

The exact input families (``ternary`` and ``eighths``) live here too, so that the CPU test can prove
about the very tensors the GPU test uploads that every accumulated quantity is exact in fp32.
"""

import torch

import _cnn_ops_ref as O

NAN = float("nan")
F64 = torch.float64


def cp(c):
    return (c + 7) // 8 * 8


def out_hw(H, W, R, S, stride, pad):
    return (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1


def bf16(t):
    """Round to nearest even to bf16, returned in the input's dtype."""
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


# ---------------------------------------------------------------------------------------------
# the three convolutions of one peer (dense, no batch masking)
# ---------------------------------------------------------------------------------------------
def _taps(R, S, order):
    taps = [(r, s) for r in range(R) for s in range(S)]
    return taps[::-1] if order else taps


def _padded(x, R, S, stride, pad, Ho, Wo):
    """x [n, H, W, C] inside a zero frame that holds every tap of every output pixel."""
    n, H, W, C = x.shape
    hh = pad + max(H, (Ho - 1) * stride - pad + R)
    ww = pad + max(W, (Wo - 1) * stride - pad + S)
    xp = torch.zeros(n, hh, ww, C, dtype=x.dtype)
    xp[:, pad:pad + H, pad:pad + W] = x
    return xp


def _mm(a, b, order):
    """a [..., k] @ b [k, m]; ``order`` 1 walks k backwards (another summation order)."""
    if order:
        a, b = a.flip(-1), b.flip(0)
    return a @ b


def conv_acc(x, w, stride, pad, Ho, Wo, order=0):
    """``acc[n, oh, ow, co] = sum_{r, s, ci} x[n, oh*stride - pad + r, ow*stride - pad + s, ci] * w[co, r, s, ci]``."""
    Co, R, S, _ = w.shape
    xp = _padded(x, R, S, stride, pad, Ho, Wo)
    acc = torch.zeros(x.shape[0], Ho, Wo, Co, dtype=x.dtype)
    for r, s in _taps(R, S, order):
        win = xp[:, r:r + stride * (Ho - 1) + 1:stride, s:s + stride * (Wo - 1) + 1:stride]
        acc = acc + _mm(win, w[:, r, s, :].t(), order)
    return acc


def conv_dgrad(dy, w, H, W, stride, pad, order=0):
    """The transpose of ``conv_acc`` in x: ``dx[n, h, w, ci] = sum dy[n, oh, ow, co] * w[co, r, s, ci]``
    over the (oh, r), (ow, s) with ``oh*stride - pad + r = h``, ``ow*stride - pad + s = w``."""
    n, Ho, Wo, Co = dy.shape
    _, R, S, Ci = w.shape
    hh = pad + max(H, (Ho - 1) * stride - pad + R)
    ww = pad + max(W, (Wo - 1) * stride - pad + S)
    dxp = torch.zeros(n, hh, ww, Ci, dtype=dy.dtype)
    for r, s in _taps(R, S, order):
        dxp[:, r:r + stride * (Ho - 1) + 1:stride, s:s + stride * (Wo - 1) + 1:stride] += _mm(dy, w[:, r, s, :], order)
    return dxp[:, pad:pad + H, pad:pad + W].clone()


def conv_wgrad(dy, x, R, S, stride, pad, order=0):
    """``dW[co, r, s, ci] = sum_{n, oh, ow} dy[n, oh, ow, co] * x[n, oh*stride - pad + r, ow*stride - pad + s, ci]``."""
    n, Ho, Wo, Co = dy.shape
    Ci = x.shape[-1]
    xp = _padded(x, R, S, stride, pad, Ho, Wo)
    g = torch.zeros(Co, R, S, Ci, dtype=dy.dtype)
    d2 = dy.reshape(-1, Co).t()
    for r, s in _taps(R, S, order):
        win = xp[:, r:r + stride * (Ho - 1) + 1:stride, s:s + stride * (Wo - 1) + 1:stride].reshape(-1, Ci)
        g[:, r, s, :] = _mm(d2, win, order)
    return g


# ---------------------------------------------------------------------------------------------
# grouped forward
# ---------------------------------------------------------------------------------------------
def prologue(y, ss, dtype=F64):
    """The A operand of a launch with ``pro_ss``: ``bf16(relu(y * sc + sh))`` per channel (one fused
    multiply-add, so one rounding). ``y``: [P, n, H, W, Cp], ``ss``: [P, 2, Cp]."""
    sc, sh = ss[:, 0].to(dtype)[:, None, None, None], ss[:, 1].to(dtype)[:, None, None, None]
    return bf16((y.to(dtype) * sc + sh).clamp_min(0))


def forward(x, w, nb, stride, pad, Ho, Wo, ncol_valid=None, bias=None, resid=None, relu=False, pro_ss=None, dtype=F64, order=0):
    """``x``: [P, B, H, W, Cpi], ``w``: [P, Cpo, R, S, Cpi], ``bias``: [P, Cpo], ``resid``: [P, B, Ho, Wo, Cpo].
    ``v = acc (+ bias) (+ resid)``, ReLU, columns ``>= ncol_valid`` zero. Returns ``(out, v, stats)``:
    ``out = bf16(v)`` with NaN at samples ``>= nb[p]``, ``v`` the unrounded values (same holes) and
    ``stats`` [P, 2, Cpo] = (sum v, sum v^2) over the valid samples — the kernel's BatchNorm
    statistics see the fp32 values before the rounding."""
    P, B = x.shape[:2]
    Cpo = w.shape[1]
    ncol_valid = Cpo if ncol_valid is None else ncol_valid
    v = torch.full((P, B, Ho, Wo, Cpo), NAN, dtype=dtype)
    stats = torch.zeros(P, 2, Cpo, dtype=dtype)
    a = x if pro_ss is None else prologue(x, pro_ss, dtype)
    for p in range(P):
        n = nb[p]
        if n == 0:
            continue
        t = conv_acc(a[p, :n].to(dtype), w[p].to(dtype), stride, pad, Ho, Wo, order)
        if bias is not None:
            t = t + bias[p].to(dtype)
        if resid is not None:
            t = t + resid[p, :n].to(dtype)
        if relu:
            t = t.clamp_min(0)
        t[..., ncol_valid:] = 0
        v[p, :n] = t
        stats[p, 0] = t.reshape(-1, Cpo).sum(0)
        stats[p, 1] = (t * t).reshape(-1, Cpo).sum(0)
    return bf16(v), v, stats


# ---------------------------------------------------------------------------------------------
# grouped dgrad (+ BatchNorm-backward epilogue)
# ---------------------------------------------------------------------------------------------
def dgrad(dy, w, nb, H, W, stride, pad, ncol_valid=None, resid=None, mask=None, mask_ss=None, y0=None, ms0=None, y1=None, ms1=None,
          dtype=F64, order=0, live=None, round_g=True):
    """``dX = conv_transpose(dY, w)`` — one expression for every way the engine runs it (mode 1 at
    stride 1 and by parity class at stride 2, mode 4 with flipped weights, mode 5 by parity class
    with class-flipped weights). ``dy``: [P, B, Ho, Wo, Cpo], ``w``: [P, Cpo, R, S, Cpi].

    With ``y0`` the BatchNorm-backward epilogue: ``g = bf16(acc + resid) * [mask > 0]`` where the mask
    is ``mask`` or ``fma(y0, sc, sh)`` from ``mask_ss`` [P, 2, Cpi], and the sums over the *rounded* g:
    ``sum g``, ``sum (g * (y0 - mean0)) * inv0`` and the same with ``y1`` (``ms`` = [P, 2, Cpi] mean | inv).
    Returns ``(out, v, sums)``: ``out`` rounded with NaN holes, ``v`` unrounded, ``sums`` [P, 3, Cpi]
    (zeros without ``y0``). ``live`` overrides the mask comparison and ``round_g = False`` sums the
    unrounded gradient (negative controls)."""
    P, B = dy.shape[:2]
    Cpi = w.shape[-1]
    ncol_valid = Cpi if ncol_valid is None else ncol_valid
    live = live or (lambda t: t > 0)
    v = torch.full((P, B, H, W, Cpi), NAN, dtype=dtype)
    out = v.clone()
    sums = torch.zeros(P, 3, Cpi, dtype=dtype)
    for p in range(P):
        n = nb[p]
        if n == 0:
            continue
        t = conv_dgrad(dy[p, :n].to(dtype), w[p].to(dtype), H, W, stride, pad, order)
        if resid is not None:
            t = t + resid[p, :n].to(dtype)
        t[..., ncol_valid:] = 0
        v[p, :n] = t
        if y0 is None:
            out[p, :n] = bf16(t)
            continue
        if mask is not None:
            t = torch.where(live(mask[p, :n].to(dtype)), t, torch.zeros((), dtype=dtype))
        elif mask_ss is not None:
            pre = y0[p, :n].to(dtype) * mask_ss[p, 0].to(dtype) + mask_ss[p, 1].to(dtype)
            t = torch.where(live(pre), t, torch.zeros((), dtype=dtype))
        g = bf16(t)
        out[p, :n] = g
        if not round_g:
            g = t
        sums[p, 0] = g.reshape(-1, Cpi).sum(0)
        sums[p, 1] = ((g * (y0[p, :n].to(dtype) - ms0[p, 0].to(dtype))) * ms0[p, 1].to(dtype)).reshape(-1, Cpi).sum(0)
        if y1 is not None:
            sums[p, 2] = ((g * (y1[p, :n].to(dtype) - ms1[p, 0].to(dtype))) * ms1[p, 1].to(dtype)).reshape(-1, Cpi).sum(0)
    return out, v, sums


# ---------------------------------------------------------------------------------------------
# grouped wgrad
# ---------------------------------------------------------------------------------------------
def wgrad(dy, x, nb, R, S, stride, pad, pro_ss=None, dtype=F64, order=0):
    """``dW`` [P, Cpo, R, S, Cpi] over each peer's valid samples (zero for ``nb = 0``: what the sum
    is; whether the kernel stores it is the launch's ``accumulate`` contract, see the GPU test)."""
    P = dy.shape[0]
    a = x if pro_ss is None else prologue(x, pro_ss, dtype)
    g = torch.zeros(P, dy.shape[-1], R, S, x.shape[-1], dtype=dtype)
    for p in range(P):
        n = nb[p]
        if n:
            g[p] = conv_wgrad(dy[p, :n].to(dtype), a[p, :n].to(dtype), R, S, stride, pad, order)
    return g


# ---------------------------------------------------------------------------------------------
# weight flips (pure permutations)
# ---------------------------------------------------------------------------------------------
def wt_flip(w):
    """``Wt[ci, r, s, co] = Wf[co, R-1-r, S-1-s, ci]`` ([..., Cpo, R, S, Cpi] -> [..., Cpi, R, S, Cpo])."""
    return w.flip(-3, -2).transpose(-4, -1).contiguous()


def parity_taps(R, S, pad, c):
    """Taps (rows, columns) of parity class ``c = 2 ph + pw`` of a stride-2 dgrad, in the flipped
    order the class's forward conv walks them."""
    r0, s0 = ((c >> 1) + pad) & 1, ((c & 1) + pad) & 1
    return list(range(r0, R, 2))[::-1], list(range(s0, S, 2))[::-1]


def wt_flip_parity(w, pad):
    """One peer's ``Wf`` [Cpo, R, S, Cpi] -> the four classes' ``[ci][tR][tS][co]`` blocks, concatenated
    in class order (flat); classes without taps take no room."""
    _, R, S, _ = w.shape
    blocks = []
    for c in range(4):
        rr, ss = parity_taps(R, S, pad, c)
        if rr and ss:
            blocks.append(w[:, rr][:, :, ss].permute(3, 1, 2, 0).reshape(-1))
    return torch.cat(blocks) if blocks else w.new_zeros(0)


# ---------------------------------------------------------------------------------------------
# fused finalize tail: the cnn_ops oracles on the oracle's sums
# ---------------------------------------------------------------------------------------------
def fin_fwd(stats, nb, hw, gamma, beta, rmean, rvar, C, Cp, eps, momentum, train=True, dtype=F64, count=None):
    """``stats`` [P, 2, Cp] -> ``(ss, ms, rmean, rvar)`` of ``_cnn_ops_ref.bn_finalize``."""
    ss, ms, rm, rv, _ = O.bn_finalize(stats[:, None].to(dtype), nb, hw, gamma, beta, rmean, rvar, C, Cp, eps, momentum, train, dtype, count)
    return ss, ms, rm, rv


def fin_bwd(sums2, nb, hw, gamma, ms, C, Cp, dtype=F64, count=None):
    """``sums2`` [P, 2, Cp] (sum g, sum g xhat) -> ``(dgamma, dbeta, coef)`` of ``_cnn_ops_ref.bn_bwd_finalize``."""
    return O.bn_bwd_finalize(sums2.to(dtype), nb, hw, gamma, ms, C, Cp, dtype, count)


# ---------------------------------------------------------------------------------------------
# input families
# ---------------------------------------------------------------------------------------------
def gen(seed):
    return torch.Generator().manual_seed(seed)


def ternary(g, *shape):
    return torch.randint(-1, 2, shape, generator=g).double()


def eighths(g, *shape, lim=4):
    return torch.randint(-8 * lim, 8 * lim + 1, shape, generator=g).double() / 8


def pow2(g, *shape):
    return torch.tensor([0.5, 1.0, 2.0], dtype=F64)[torch.randint(0, 3, shape, generator=g)]


def normal(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16).double()


def data(g, family, *shape, role="x"):
    """One operand of ``family``. ternary: everything in {-1, 0, 1} (weights of a K > 144 sum: nonzero
    with probability 144 / K). eighths: |x| <= 4 (activations,
    gradients, residuals) and |w| <= 1 in eighths. randn: bf16-rounded normals, weights scaled by
    ``1/sqrt(K)`` through ``role = ('w', K)``."""
    if family == "ternary":
        t = ternary(g, *shape)
        if role != "x" and role[1] > 144:  # long sums: thin the weights so that sum x^2 stays below 2^24 units
            t = t * (torch.rand(*shape, generator=g) < 144.0 / role[1])
        return t
    if family == "eighths":
        return eighths(g, *shape, lim=1 if role != "x" else 4)
    return normal(g, *shape, scale=1.0 if role == "x" else role[1] ** -0.5)


def pad_channels(t, c):
    """Zero the padding channels (last axis) ``>= c``."""
    t = t.clone()
    t[..., c:] = 0
    return t


def coeffs(g, P, Cp, family, lim=2):
    """Per-channel (scale | shift) or (inv | mean)-like pairs [P, 2, Cp]: first row powers of two, second
    row eighths with |v| <= lim (exact families), or positive scales and normal shifts (randn)."""
    if family == "randn":
        return torch.stack([torch.rand(P, Cp, generator=g).double() + 0.5, torch.randn(P, Cp, generator=g).double() * 0.5], 1).float().double()
    return torch.stack([pow2(g, P, Cp), torch.randint(-int(8 * lim), int(8 * lim) + 1, (P, Cp), generator=g).double() / 8], 1)


# ---------------------------------------------------------------------------------------------
# cases shared by the CPU and the GPU test (the CPU test proves their exactness conditions)
# ---------------------------------------------------------------------------------------------
P = 3
FAMILIES = ("ternary", "eighths")
BASE = 3.0  # what an accumulating wgrad launch finds in its gradient slab (on every family's grid)


def nbatch(n):
    """[full, partial, none]: the engine gives a peer past its data (and an inactive slot) nb = 0."""
    return [n, max(1, n // 2), 0]


def case(cin, cout, H, W, R, S, stride, pad, n, ops=""):
    Ho, Wo = out_hw(H, W, R, S, stride, pad)
    return dict(cin=cin, cout=cout, H=H, W=W, R=R, S=S, stride=stride, pad=pad, n=n, ops=ops, Ho=Ho, Wo=Wo, cpi=cp(cin), cpo=cp(cout))


# forward. ops: b bias, l ReLU, r residual, t BN statistics (spread rows), 1 statistics in one row,
# p BN prologue, z a bias of zeros (the runtime-flag epilogue on otherwise specialised operands)
FWD = {
    "k8_1x1_5x7_v6": case(8, 6, 5, 7, 1, 1, 1, 0, 3, "t"),               # K 8, ncol 8 (6 valid), one partial 128-row tile
    "k72_5x7_v20_all": case(8, 20, 5, 7, 3, 3, 1, 1, 5, "blrt"),         # K 72, ncol 24 (20 valid), M 175
    "k72_5x7_v20_relu": case(8, 20, 5, 7, 3, 3, 1, 1, 5, "l"),           # ReLU alone
    "k72_5x7_c64": case(8, 64, 5, 7, 3, 3, 1, 1, 5, "t"),                # ncol 64, SPEC 32
    "k72_5x7_c64_plain": case(8, 64, 5, 7, 3, 3, 1, 1, 5, ""),           # SPEC 0
    "k72_5x7_c64_plain_z": case(8, 64, 5, 7, 3, 3, 1, 1, 5, "z"),
    "k72_5x7_c64_z": case(8, 64, 5, 7, 3, 3, 1, 1, 5, "tz"),             # same operands, runtime flags
    "k200_5x5_9x6_s2": case(8, 64, 9, 6, 5, 5, 2, 2, 9, "r"),            # K 200 (no multiple of 64), stride 2, odd H, pad 2
    "k576_5x7_c72": case(64, 72, 5, 7, 3, 3, 1, 1, 8, "1"),              # K 576, wide tile partial, M 280 > 256, SPEC 32
    "k576_5x7_c72_plain": case(64, 72, 5, 7, 3, 3, 1, 1, 8, ""),         # wide SPEC 0 (the evaluation forward)
    "k576_5x7_c72_plain_z": case(64, 72, 5, 7, 3, 3, 1, 1, 8, "z"),
    "k576_5x7_c72_z": case(64, 72, 5, 7, 3, 3, 1, 1, 8, "1z"),
    "k144_5x7_c72_pro": case(16, 72, 5, 7, 3, 3, 1, 1, 8, "pt"),         # generic forward with the BN prologue
    "k1152_9x6_s2_c136": case(128, 136, 9, 6, 3, 3, 2, 1, 3, "tl"),      # K 1152 (stage ring wraps), two wide tiles
    "k48_1x3_5x7": case(16, 16, 5, 7, 1, 3, 1, 1, 4, "b"),               # R != S
    "k48_3x1_5x7_p0": case(16, 16, 5, 7, 3, 1, 1, 0, 4, "r"),
    "fc_400_120": case(400, 120, 1, 1, 1, 1, 1, 0, 37, "bl"),            # LeNet's layer-wise fc path
    "fc_120_84": case(120, 84, 1, 1, 1, 1, 1, 0, 37, "bl"),
    "fc_84_10": case(84, 10, 1, 1, 1, 1, 1, 0, 37, "b"),
    "halo_8x32": case(64, 64, 8, 32, 3, 3, 1, 1, 3, "t"),                # k_conv_fwd_halo, SPEC 32
    "halo_8x32_plain": case(64, 64, 8, 32, 3, 3, 1, 1, 3, ""),           # SPEC 0
    "halo_8x32_plain_z": case(64, 64, 8, 32, 3, 3, 1, 1, 3, "z"),
    "halo_8x32_z": case(64, 64, 8, 32, 3, 3, 1, 1, 3, "tzr"),            # runtime flags, residual
    "halo_8x32_pro": case(64, 64, 8, 32, 3, 3, 1, 1, 2, "pt"),          # prologue in the patch
    "halo_8x32_pro_plain": case(64, 64, 8, 32, 3, 3, 1, 1, 2, "p"),     # prologue, SPEC 0
    "halo_8x32_pro_plain_z": case(64, 64, 8, 32, 3, 3, 1, 1, 2, "pz"),
    "halo_8x32_pro_z": case(64, 64, 8, 32, 3, 3, 1, 1, 2, "ptz"),       # prologue, runtime flags
}

# dgrad of the conv cin -> cout. ops: r residual, m materialised mask, s mask from y0 (mask_ss),
# 1 / 2 BatchNorm-backward sums of one / two BatchNorms, z a bias of zeros
DGRAD = {
    "k72_5x7": case(8, 24, 5, 7, 3, 3, 1, 1, 5, ""),
    "k72_5x7_m1": case(8, 24, 5, 7, 3, 3, 1, 1, 5, "m1"),
    "k48_1x3_5x7_m1": case(16, 24, 5, 7, 1, 3, 1, 1, 4, "m1"),           # R != S: mode 1 only (mode 4 rejects it)
    "k48_3x1_5x7_p0": case(16, 24, 5, 7, 3, 1, 1, 0, 4, ""),
    "s2_1x3_9x6_rm1": case(16, 24, 9, 6, 1, 3, 2, 1, 3, "rm1"),          # R != S at stride 2: parity classes, modes 1 and 5
    "s2_3x1_9x6_p0": case(16, 24, 9, 6, 3, 1, 2, 0, 3, "s2"),
    "k200_5x5_9x6": case(8, 16, 9, 6, 5, 5, 1, 2, 3, "rs2"),
    "c20_5x7_v": case(20, 24, 5, 7, 3, 3, 1, 1, 5, "rm1"),               # ncol_valid 20 < ncol 24
    "s2_9x6_c64": case(64, 72, 9, 6, 3, 3, 2, 1, 5, ""),                 # stride 2, odd and even extents, M 270; SPEC 0
    "s2_9x6_c64_z": case(64, 72, 9, 6, 3, 3, 2, 1, 5, "z"),
    "s2_9x6_c64_rm1": case(64, 72, 9, 6, 3, 3, 2, 1, 5, "rm1"),          # SPEC 11
    "s2_9x6_c64_rm1z": case(64, 72, 9, 6, 3, 3, 2, 1, 5, "rm1z"),
    "s2_9x6_c136_rm1": case(136, 64, 9, 6, 3, 3, 2, 1, 3, "rm1"),        # wide SPEC 11
    "s2_9x6_c136_rm1z": case(136, 64, 9, 6, 3, 3, 2, 1, 3, "rm1z"),
    "s2_9x6_c136": case(136, 64, 9, 6, 3, 3, 2, 1, 3, ""),               # wide SPEC 0 (the projections' plain dgrad)
    "s2_9x6_c136_z": case(136, 64, 9, 6, 3, 3, 2, 1, 3, "z"),
    "s2_9x6_c136_s2": case(136, 64, 9, 6, 3, 3, 2, 1, 3, "s2"),
    "s2_1x1_9x6": case(16, 24, 9, 6, 1, 1, 2, 0, 3, "m2"),               # the projection: three classes without taps
    "s1_5x7_c136_m1": case(136, 64, 5, 7, 3, 3, 1, 1, 8, "m1"),          # wide SPEC 10, M 280
    "s1_5x7_c136_m1z": case(136, 64, 5, 7, 3, 3, 1, 1, 8, "m1z"),        # the same operands, runtime flags
    "s1_5x7_c136_rm1": case(136, 64, 5, 7, 3, 3, 1, 1, 8, "rm1"),        # wide SPEC 11
    "s1_5x7_c136_rm1z": case(136, 64, 5, 7, 3, 3, 1, 1, 8, "rm1z"),
    "halo_8x32_rm1": case(64, 64, 8, 32, 3, 3, 1, 1, 3, "rm1"),          # k_conv_fwd_halo<4>, SPEC 11
    "halo_8x32_s1": case(64, 64, 8, 32, 3, 3, 1, 1, 3, "s1"),            # SPEC 18
    "halo_8x32_s1z": case(64, 64, 8, 32, 3, 3, 1, 1, 3, "s1z"),          # the same operands, runtime flags
    "halo_8x32_rs2": case(64, 64, 8, 32, 3, 3, 1, 1, 3, "rs2"),          # runtime flags
    "halo_8x32_rm1z": case(64, 64, 8, 32, 3, 3, 1, 1, 3, "rm1z"),
}

# wgrad. ops: p BN prologue on x. The halo shapes are the smallest the dispatch condition allows.
WGRAD = {
    "k8_1x1_5x7": case(8, 6, 5, 7, 1, 1, 1, 0, 3, ""),
    "k8_1x1_5x7_c72": case(8, 72, 5, 7, 1, 1, 1, 0, 3, ""),              # 128 x 64 tile (a 1x1 projection's shape)
    "k72_5x7": case(8, 20, 5, 7, 3, 3, 1, 1, 5, ""),
    "k72_5x7_pro": case(8, 20, 5, 7, 3, 3, 1, 1, 5, "p"),
    "k200_5x5_9x6_s2": case(8, 64, 9, 6, 5, 5, 2, 2, 9, ""),
    "k576_5x7_c72": case(64, 72, 5, 7, 3, 3, 1, 1, 4, ""),
    "k48_1x3_5x7": case(16, 16, 5, 7, 1, 3, 1, 1, 4, ""),
    "k48_3x1_5x7_p0": case(16, 16, 5, 7, 3, 1, 1, 0, 4, ""),
    "fc_400_120": case(400, 120, 1, 1, 1, 1, 1, 0, 37, ""),
    "halo_4x4": case(64, 64, 4, 4, 3, 3, 1, 1, 9, ""),                   # four images per K step, the last step partial
    "halo_8x8_c128": case(128, 64, 8, 8, 3, 3, 1, 1, 3, ""),
    "halo_4x16": case(64, 128, 4, 16, 3, 3, 1, 1, 3, ""),
    "halo_8x16": case(64, 64, 8, 16, 3, 3, 1, 1, 3, "p"),
    "halo_2x32": case(64, 64, 2, 32, 3, 3, 1, 1, 5, ""),
    "halo_2x32_pro": case(128, 128, 2, 32, 3, 3, 1, 1, 5, "p"),
}


def _seed(name, family):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(name + family)) % 100003


def _ss(g, c, Cp, family, lim=2):
    """(scale | shift)-like constants with zero padding channels."""
    return pad_channels(coeffs(g, P, Cp, family, lim), c)


def fwd_inputs(name, family):
    c = FWD[name]
    g = gen(_seed(name, family))
    B, K = c["n"], c["R"] * c["S"] * c["cin"]
    d = dict(c, nb=nbatch(B), family=family)
    d["x"] = pad_channels(data(g, family, P, B, c["H"], c["W"], c["cpi"]), c["cin"])
    w = pad_channels(data(g, family, P, c["cpo"], c["R"], c["S"], c["cpi"], role=("w", K)), c["cin"])
    w[:, c["cout"]:] = 0
    d["w"] = w
    ops = c["ops"]
    d["bias"] = data(g, family, P, c["cpo"]) if "b" in ops else (torch.zeros(P, c["cpo"], dtype=F64) if "z" in ops else None)
    d["resid"] = data(g, family, P, B, c["Ho"], c["Wo"], c["cpo"]) if "r" in ops else None  # padding channels too: the kernel zeroes them
    # the prologue's operand is never negative, so the sums grow with K: small shifts keep sum x^2 exact
    d["pro_ss"] = _ss(g, c["cin"], c["cpi"], family, 0.5) if "p" in ops else None
    d["relu"] = "l" in ops
    return d


def fwd_oracle(d, dtype=F64, order=0, **over):
    k = dict(d, **over)
    return forward(k["x"], k["w"], k["nb"], k["stride"], k["pad"], k["Ho"], k["Wo"], k["cout"], k["bias"], k["resid"], k["relu"], k["pro_ss"], dtype, order)


def dgrad_inputs(name, family):
    c = DGRAD[name]
    g = gen(_seed(name, family))
    B, K = c["n"], c["R"] * c["S"] * c["cout"]
    d = dict(c, nb=nbatch(B), family=family)
    d["dy"] = pad_channels(data(g, family, P, B, c["Ho"], c["Wo"], c["cpo"]), c["cout"])
    w = pad_channels(data(g, family, P, c["cpo"], c["R"], c["S"], c["cpi"], role=("w", K)), c["cin"])
    w[:, c["cout"]:] = 0
    d["w"] = w
    ops = c["ops"]
    shape = (P, B, c["H"], c["W"], c["cpi"])
    d["resid"] = data(g, family, *shape) if "r" in ops else None
    d["mask"] = data(g, family, *shape) if "m" in ops else None  # negative values too: only > 0 is live
    d["mask_ss"] = _ss(g, c["cin"], c["cpi"], family) if "s" in ops else None
    nbn = 2 if "2" in ops else (1 if "1" in ops else 0)
    for i in range(2):
        on = i < nbn
        d[f"y{i}"] = pad_channels(data(g, family, *shape), c["cin"]) if on else None
        d[f"ms{i}"] = _ss(g, c["cin"], c["cpi"], family).flip(1).contiguous() if on else None  # [mean | inv]
    d["zero_bias"] = "z" in ops
    return d


def dgrad_oracle(d, dtype=F64, order=0, live=None, round_g=True, **over):
    k = dict(d, **over)
    return dgrad(k["dy"], k["w"], k["nb"], k["H"], k["W"], k["stride"], k["pad"], k["cin"], k["resid"], k["mask"], k["mask_ss"], k["y0"], k["ms0"],
                 k["y1"], k["ms1"], dtype, order, live, round_g)


def wgrad_inputs(name, family):
    c = WGRAD[name]
    g = gen(_seed(name, family))
    B = c["n"]
    d = dict(c, nb=nbatch(B), family=family)
    d["dy"] = pad_channels(data(g, family, P, B, c["Ho"], c["Wo"], c["cpo"], role=("w", B * c["Ho"] * c["Wo"])), c["cout"])
    d["x"] = pad_channels(data(g, family, P, B, c["H"], c["W"], c["cpi"]), c["cin"])
    d["pro_ss"] = _ss(g, c["cin"], c["cpi"], family) if "p" in c["ops"] else None
    return d


def wgrad_oracle(d, dtype=F64, order=0, **over):
    k = dict(d, **over)
    return wgrad(k["dy"], k["x"], k["nb"], k["R"], k["S"], k["stride"], k["pad"], k["pro_ss"], dtype, order)


def bump(t, idx, unit):
    """``t`` with the element at ``idx`` moved by one grid unit (sensitivity controls)."""
    t = t.clone()
    t[idx] += unit
    return t


def _bump_act(d, key, idx, unit):
    """Bump activation ``d[key][idx]``; behind a BN prologue walk the channel down until the operand
    ``bf16(relu(y * sc + sh))`` really moves (a clipped element would hide the change)."""
    t = bump(d[key], idx, unit)
    if d.get("pro_ss") is None or key != "x":
        return t
    base = prologue(d[key], d["pro_ss"])
    idx = list(idx)
    while torch.equal(torch.nan_to_num(prologue(t, d["pro_ss"])), torch.nan_to_num(base)):
        idx[-1] -= 1
        assert idx[-1] >= 0
        t = bump(d[key], tuple(idx), unit)
    return t


def controls(kind, d):
    """Single-element changes of one grid unit that the exact comparisons must see:
    ``{label: overrides}`` for ``fwd_oracle`` / ``dgrad_oracle`` / ``wgrad_oracle``.

    * corner: the corner pixel of the first sample (it reaches the output only through border taps);
    * lastk:  the last channel of the last K chunk (forward / dgrad: the weight of the last tap, last
      input channel, last output channel; wgrad, whose K runs over pixels: the last pixel of peer 0);
    * lastrow: the last pixel of the partial peer's last valid sample."""
    u = 1.0 if d["family"] == "ternary" else 0.125
    last = d["nb"][1] - 1
    if kind == "fwd":
        c = d["cin"] - 1
        return {"corner": {"x": _bump_act(d, "x", (0, 0, 0, 0, c), u)},
                "lastk": {"w": bump(d["w"], (0, d["cout"] - 1, d["R"] - 1, d["S"] - 1, c), u)},
                "lastrow": {"x": _bump_act(d, "x", (1, last, d["H"] - 1, d["W"] - 1, c), u)}}
    if kind == "dgrad":
        c = d["cout"] - 1
        ci = d["cin"] - 1  # the last output column that the ReLU mask leaves alive somewhere
        if d["y0"] is not None:
            alive = torch.nan_to_num(dgrad_oracle(d, dy=torch.ones_like(d["dy"]), w=torch.ones_like(d["w"]), resid=None)[0][0]).abs().sum((0, 1, 2))
            ci = int(alive[:d["cin"]].nonzero().max())
        first = lambda pad, taps: max(0, -((taps - 1 - pad) // d["stride"]))  # the first dY row / column with a tap inside the image
        return {"corner": {"dy": bump(d["dy"], (0, 0, first(d["pad"], d["R"]), first(d["pad"], d["S"]), c), u)},
                "lastk": {"w": bump(d["w"], (0, c, d["R"] - 1, d["S"] - 1, ci), u)},
                # the last dY pixel with a tap inside the image (with pad >= R the very last sees padding only)
                "lastrow": {"dy": bump(d["dy"], (1, last, min(d["Ho"] - 1, (d["H"] - 1 + d["pad"]) // d["stride"]),
                                                 min(d["Wo"] - 1, (d["W"] - 1 + d["pad"]) // d["stride"]), c), u)}}
    c = d["cin"] - 1
    return {"corner": {"x": _bump_act(d, "x", (0, 0, 0, 0, c), u)},
            "lastk": {"x": _bump_act(d, "x", (0, d["nb"][0] - 1, d["H"] - 1, d["W"] - 1, c), u)},
            "lastrow": {"x": _bump_act(d, "x", (1, last, d["H"] - 1, d["W"] - 1, c), u)}}


LIM = 2.0 ** 24  # sum |term| / unit below this: every partial sum is a multiple of unit that fp32 holds


def units(family, pro):
    """(grid unit of the activation operand, of the weight-like operand) of an exact family; behind a
    BN prologue the operand is ``relu(y * 2^k + eighths)``."""
    if family == "ternary":
        return (0.125 if pro else 1.0), 1.0
    return (0.0625 if pro else 0.125), 0.125


def on_grid(t, unit):
    t = torch.nan_to_num(t, nan=0.0)
    return torch.equal(torch.round(t / unit) * unit, t)


def sq_exact(d, v):
    """Is ``sum v^2`` of forward case ``d`` (``v``: the oracle's unrounded values) exact in fp32?"""
    ua, uw = units(d["family"], d["pro_ss"] is not None)
    rows = torch.nan_to_num(v).reshape(P, -1, d["cpo"])
    return float((rows * rows).sum(1).max()) / (ua * uw) ** 2 < LIM


def xhat_exact(d, out):
    """Are the ``sum (g * (y - mean)) * inv`` of dgrad case ``d`` (``out``: the oracle's rounded g) exact
    in fp32? g sits on the accumulator's grid ``unit`` (bf16 spacing is >= unit above 2), ``y - mean`` on
    eighths and ``inv`` is 1/2, 1 or 2: both products are exact and the terms sit on ``unit / 16``."""
    ua, uw = units(d["family"], False)
    unit = ua * uw / 16
    g = torch.nan_to_num(out)
    ok = True
    for i in range(2):
        if d[f"y{i}"] is None:
            continue
        ms = d[f"ms{i}"][:, None, None, None]
        t = (g * (torch.nan_to_num(d[f"y{i}"]) - ms[..., 0, :])) * ms[..., 1, :]
        ok = ok and on_grid(t, unit) and float(t.reshape(P, -1, d["cpi"]).abs().sum(1).max()) / unit < LIM
    return ok


def inputs(kind, name, family):
    return {"fwd": fwd_inputs, "dgrad": dgrad_inputs, "wgrad": wgrad_inputs}[kind](name, family)


def oracle(kind, d, **kw):
    """What a launch of case ``d`` leaves in memory, as a tuple: the rounded output, and the column
    sums if the case collects them; the weight gradient."""
    if kind == "fwd":
        out, _, stats = fwd_oracle(d, **kw)
        return (out, stats) if ("t" in d["ops"] or "1" in d["ops"]) else (out,)
    if kind == "dgrad":
        out, _, sums = dgrad_oracle(d, **kw)
        return (out, sums) if d["y0"] is not None else (out,)
    return (wgrad_oracle(d, **kw),)


def differs(a, b):
    """Two oracle results (tensors or tuples of tensors, NaN = hole) are not the same."""
    a, b = (a if isinstance(a, tuple) else (a,)), (b if isinstance(b, tuple) else (b,))
    return any(not torch.equal(torch.nan_to_num(x.double(), nan=12345.0), torch.nan_to_num(y.double(), nan=12345.0)) for x, y in zip(a, b))
