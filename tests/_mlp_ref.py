"""Plain float64 model of the fused MLP engine's shuffle, gather and bf16 step kernels
(``csrc/kernels/mlp_fused.hip``: ``feistel_perm``, ``mlp_gather_epoch``, ``mlp_sync_shadow``, ``mlp_fc1_fwd``,
``mlp_head``, ``mlp_wgrad_opt``), written from the definition of each operation. Python integers and
NumPy for the shuffle, torch float64 matrix products for the step; no autograd, nothing from
``myfyp_amd``. The optimizer is ``_fl_ops_ref.adam_step`` / ``sgd_step`` (the oracle of ``opt_update``).

``rnd`` is the rounding applied exactly where the kernels store bf16 (round to nearest even);
``rnd = ident`` switches every rounding off (``tests/test_mlp_ref_cpu.py`` holds that form to
``myfyp_amd.models.MLP`` under float64 autograd).

Rules
-----
* ``H1 = rnd(relu(X W1s^T + b1))``, ``H2 = rnd(relu(H1 W2s^T + b2))``, ``logits = H2 W3s^T + b3``: ``W?s`` are the
  bf16 shadow weights, the biases come from the fp32 master row;
* the predicted class is the FIRST maximum of the logits;
* ``dlogits = rnd((softmax - onehot) / rows)`` for the valid rows and the columns below D3, zero elsewhere;
* ``dH2 = rnd(dlogits W3s * [H2 > 0])``, ``dH1 = rnd(dH2 W2s * [H1 > 0])``: the masks are the stored activations;
* the six gradients are plain sums over the batch of products of those bf16 operands.

Every stage is its own function of its upstream tensors, so the GPU test can feed it what the kernel
itself exported.

The softmax bound ``eps_sm``
----------------------------
``mlp_head`` forms ``logp = logit - (mx + __logf(sum __expf(logit - mx)))`` and ``d = (__expf(logp) - onehot) / rows`` in
fp32 with the fast intrinsics: ``__expf(x) = exp2(x * log2(e))`` and ``__logf(x) = log2(x) * ln 2`` on the hardware
``v_exp_f32`` / ``v_log_f32``. The kernel guides list both among the 8-cycle transcendental instructions
but give no accuracy figure; the figure used here is the 1 ulp (2^-23 relative) the public CDNA ISA
reference states for them. With ``u = 2^-24``, ``R = max logit - min logit`` of a row and ``L = max |logit|``:

* ``__expf(x)``, ``x`` in ``[-R, 0]``: the product with ``log2(e)`` (rounded constant, rounded product) moves the exponent
  by at most ``2 u |x| log2(e)``, i.e. the result by ``2 u R`` relatively, and ``v_exp_f32`` adds ``2 u``:
  ``e_exp = 2 u (1 + R)``;
* the sum of at most 16 terms by a 4-level butterfly: ``4 u`` more, so ``se`` in ``[1, 16]`` is off by ``e_exp + 4 u``
  relatively, which is what ``log`` passes on as an absolute error;
* ``v_log_f32`` is off by ``2 u |log2 se| <= 8 u``, the product with ``ln 2`` (rounded constant and product) by
  ``2 u ln 16``: ``e_lse = e_exp + 4 u + 8 u ln 2 + 2 u ln 16``;
* ``mx + lse`` rounds once on at most ``L + ln 16``, ``logit - (...)`` once on ``|logp| <= R + ln 16``:
  ``eps_lp = e_lse + u (L + R + 2 ln 16)``: the bound of one row's loss term;
* ``__expf(logp) = p``: the argument's error ``eps_lp`` and the two product roundings ``2 u |logp|`` act relatively on
  ``p <= 1`` (``p |ln p| <= 1/e``), ``v_exp_f32`` adds ``2 u p``, the subtraction of the one-hot and the division by
  ``rows`` one ``u`` each on at most 1: ``eps_sm = eps_lp + 2 u / e + 2 u + 2 u``.

:func:`eps_softmax` returns ``(eps_lp, eps_sm)`` for a block of logits; a logit that is itself only known to
``e_z`` (random inputs: ``gamma(K) sum |term|``) adds ``2 e_z`` to both.
"""

import math

import numpy as np
import torch

import _cnn_ops_ref as O
import _fl_ops_ref as R

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
P = 3
M32 = 0xFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF
GOLD64 = 0x9E3779B97F4A7C15
GOLD32 = 0x9E3779B9
LIM = 2.0 ** 24
EVAL_CHUNK = 512
gamma, U = R.gamma, R.U
ulp_bf16 = O.ulp_bf16


def ident(t):
    return t


def bf16(t):
    """Round to nearest even to bf16, returned in the input's dtype."""
    return t.to(F32).to(BF).to(t.dtype)


# ---------------------------------------------------------------------------------------------
# the epoch shuffle
# ---------------------------------------------------------------------------------------------
def mix32(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def half_bits(n):
    """Half the width of the Feistel block: the smallest even bit count >= 2 that covers ``n - 1``."""
    bits = max(2, (n - 1).bit_length())
    return (bits + 1) // 2


def feistel_perm(i, n, key):
    """Position ``i`` of the keyed permutation of ``[0, n)``: four balanced Feistel rounds on ``2 * half_bits(n)``
    bits, walked again from the result while it lies at or beyond ``n``."""
    if n <= 1:
        return 0
    half = half_bits(n)
    mask = (1 << half) - 1
    k0, k1 = key & M32, (key >> 32) & M32
    y = i
    while True:
        left, right = y >> half, y & mask
        for r in range(4):
            f = mix32(right ^ (k1 if r & 1 else k0) ^ ((GOLD32 * (r + 1)) & M32)) & mask
            left, right = right, left ^ f
        y = (left << half) | right
        if y < n:
            return y


def _mix32_np(x):
    m = np.uint64(M32)
    x = x & m
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & m
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & m
    x = x ^ (x >> np.uint64(16))
    return x


def feistel_perm_np(n, key):
    """The whole permutation ``[feistel_perm(i, n, key) for i in range(n)]`` as an int64 array (uint64 lanes)."""
    if n <= 1:
        return np.zeros(n, dtype=np.int64)
    half = np.uint64(half_bits(n))
    mask = np.uint64((1 << int(half)) - 1)
    ks = (np.uint64(key & M32), np.uint64((key >> 32) & M32))
    y = np.arange(n, dtype=np.uint64)
    todo = np.ones(n, dtype=bool)
    while todo.any():
        v = y[todo]
        left, right = v >> half, v & mask
        for r in range(4):
            f = _mix32_np(right ^ ks[r & 1] ^ np.uint64((GOLD32 * (r + 1)) & M32)) & mask
            left, right = right, left ^ f
        y[todo] = (left << half) | right
        todo = y >= np.uint64(n)
    return y.astype(np.int64)


def peer_key(seed, p):
    """The key of peer slot ``p`` under the epoch seed."""
    return (seed ^ ((GOLD64 * (p + 1)) & M64)) & M64


def epoch_perm(n, seed, p):
    return feistel_perm_np(n, peer_key(seed, p))


# ---------------------------------------------------------------------------------------------
# the epoch gather
# ---------------------------------------------------------------------------------------------
def gather(xs, ys, n, order, xb_rows, active=None, fill=float("nan")):
    """``xs[p]``: uint8 ``[>= n_p, D0]``, ``ys[p]``: int ``[>= n_p]``. ``order``: an int (the epoch seed of the native
    shuffle) or one index array per peer. Row ``i < min(n_p, xb_rows)`` of an active peer's slab is dataset row
    ``perm_p[i]``; every other row keeps ``fill``. Returns ``(Xb, Xb16, Yb)``: ``[P, xb_rows, D0]`` twice (a uint8
    pixel is the same number as bf16) and ``[P, xb_rows]``, float64."""
    Pn, D0 = len(xs), xs[0].shape[1]
    Xb = torch.full((Pn, xb_rows, D0), fill, dtype=F64)
    Yb = torch.full((Pn, xb_rows), fill, dtype=F64)
    for p in range(Pn):
        if active is not None and not active[p]:
            continue
        rows = min(n[p], xb_rows)
        if rows <= 0:
            continue
        perm = epoch_perm(n[p], order, p) if isinstance(order, int) else np.asarray(order[p])
        idx = torch.as_tensor(perm[:rows], dtype=torch.int64)
        Xb[p, :rows] = xs[p][idx].double()
        Yb[p, :rows] = ys[p][idx].double()
    return Xb, Xb.clone(), Yb


# ---------------------------------------------------------------------------------------------
# exactness
# ---------------------------------------------------------------------------------------------
def lsb(x):
    """The value of the lowest set bit of each float64 element (inf for zero)."""
    m, e = torch.frexp(x.abs())
    mi = (m * 2.0 ** 53).to(torch.int64)
    low = (mi & -mi).double()
    return torch.where(x == 0, torch.full_like(x, float("inf")), torch.ldexp(low, e - 53))


def _min_lsb(t, dim):
    return lsb(t).amin(dim)


def exactness(A, W, b=None, unit=None):
    """``sum_k |A[r, k] W[n, k]| (+ |b[n]|)`` over the grid ``unit`` the terms of output ``[r, n]`` lie on: below
    ``2^24`` every fp32 partial sum of that output, in any order, is exact. Without ``unit`` the grid is the
    product of the finest bit of row ``r`` of ``A`` and of row ``n`` of ``W`` (and the bias's own bit): every term
    is a multiple of it. Returns the ratio ``[rows, N]`` (0 where there is no term at all)."""
    mag = A.abs() @ W.abs().t()
    if b is not None:
        mag = mag + b.abs()
    if unit is None:
        unit = _min_lsb(A, 1)[:, None] * _min_lsb(W, 1)[None, :]
        if b is not None:
            unit = torch.minimum(unit, lsb(b)[None, :].expand_as(unit))
        unit = torch.where(torch.isfinite(unit), unit, torch.ones_like(unit))
    return mag / unit


# ---------------------------------------------------------------------------------------------
# stages (one peer, valid rows only)
# ---------------------------------------------------------------------------------------------
def fc_pre(A, Ws, b):
    """``A Ws^T + b`` and ``sum |term|`` of each element."""
    return A @ Ws.t() + b, A.abs() @ Ws.abs().t() + b.abs()


def fc(A, Ws, b, rnd=bf16):
    return rnd((A @ Ws.t() + b).clamp_min(0))


def logits(H2, W3s, b3):
    return H2 @ W3s.t() + b3


def head(z, y):
    """``z``: ``[rows, D3]``, ``y``: ``[rows]``. Returns the loss terms ``[rows]``, the predictions (first maximum) and
    the softmax."""
    lse = torch.logsumexp(z, 1)
    loss = lse - z.gather(1, y[:, None])[:, 0]
    mx = z.amax(1, keepdim=True)
    idx = torch.arange(z.shape[1])[None, :].expand_as(z)
    pred = torch.where(z == mx, idx, torch.full_like(idx, z.shape[1])).amin(1)
    return loss, pred, torch.exp(z - lse[:, None])


def dlogits(z, y, rows=None, rnd=bf16):
    """``rnd((softmax - onehot) / rows)``, ``[rows, 16]`` with zeros in the columns ``>= D3``."""
    n, D3 = z.shape
    sm = head(z, y)[2].clone()
    sm[torch.arange(n), y] -= 1.0
    out = torch.zeros(n, 16, dtype=F64)
    out[:, :D3] = rnd(sm / (n if rows is None else rows))
    return out


def dgrad(dup, Ws, act, rnd=bf16):
    """``rnd(dup Ws * [act > 0])``: ``dup`` ``[rows, N]``, ``Ws`` ``[N, K]``, ``act`` ``[rows, K]``."""
    return rnd(torch.where(act > 0, dup @ Ws, torch.zeros((), dtype=F64)))


def dgrad_mag(dup, Ws):
    return dup.abs() @ Ws.abs()


def wgrads(X, H1, H2, dH1, dH2, dlog, D3, dtype=F64):
    """The six gradients (and with ``dtype = F64`` their ``sum |term|``) from the stage tensors of the valid rows."""
    c = lambda t: t.to(dtype)
    dl = c(dlog[:, :D3])
    g = {"W1": c(dH1).t() @ c(X), "b1": c(dH1).sum(0), "W2": c(dH2).t() @ c(H1), "b2": c(dH2).sum(0), "W3": dl.t() @ c(H2), "b3": dl.sum(0)}
    return {k: v.double() for k, v in g.items()}


def wgrad_mags(X, H1, H2, dH1, dH2, dlog, D3):
    return wgrads(X.abs(), H1.abs(), H2.abs(), dH1.abs(), dH2.abs(), dlog.abs(), D3)


def eps_softmax(z, e_z=0.0):
    """``(eps_lp, eps_sm)`` of the module docstring for the logits ``z`` ``[rows, D3]`` (the worst row)."""
    if z.numel() == 0:
        return 0.0, 0.0
    rng = float((z.amax(1) - z.amin(1)).max())
    top = float(z.abs().max())
    ln16 = math.log(16.0)
    e_exp = 2 * U * (1 + rng)
    e_lse = e_exp + 4 * U + 8 * U * math.log(2.0) + 2 * U * ln16
    eps_lp = e_lse + U * (top + rng + 2 * ln16) + 2 * e_z
    return eps_lp, eps_lp + 2 * U / math.e + 4 * U


def step(case, p, rnd=bf16, rows=None, step_idx=None):
    """One training step of peer ``p``: every stage tensor of the valid rows, the loss terms, the predictions
    and the six gradients. ``rnd = ident``: the unrounded model."""
    X, y = batch(case, p, rows, step_idx)
    Ws = {k: (rnd(v[p]) if k[0] == "W" else v[p]) for k, v in case["W"].items()}
    D3 = case["D"][3]
    out = {"X": X, "y": y, "rows": X.shape[0]}
    out["H1"] = fc(X, Ws["W1"], Ws["b1"], rnd)
    out["H2"] = fc(out["H1"], Ws["W2"], Ws["b2"], rnd)
    out["z"] = logits(out["H2"], Ws["W3"], Ws["b3"])
    if X.shape[0]:
        out["loss"], out["pred"], _ = head(out["z"], y)
    else:
        out["loss"], out["pred"] = torch.zeros(0, dtype=F64), torch.zeros(0, dtype=torch.int64)
    out["dlog"] = dlogits(out["z"], y, rnd=rnd)
    out["dH2"] = dgrad(out["dlog"][:, :D3], Ws["W3"], out["H2"], rnd)
    out["dH1"] = dgrad(out["dH2"], Ws["W2"], out["H1"], rnd)
    out["g"] = wgrads(X, out["H1"], out["H2"], out["dH1"], out["dH2"], out["dlog"], D3)
    return out


def eval_chunk(case, p, base, rnd=bf16):
    """Rows ``[base, base + 512)`` of peer ``p``'s test set: ``(loss terms, correct, confusion [16, 16], logits)``."""
    nt = case["n_test"][p] if case["active"][p] else 0
    rows = max(0, min(EVAL_CHUNK, nt - base))
    X, y = case["xt"][p][base: base + rows].double(), case["yt"][p][base: base + rows].long()
    Ws = {k: (rnd(v[p]) if k[0] == "W" else v[p]) for k, v in case["W"].items()}
    z = logits(fc(fc(X, Ws["W1"], Ws["b1"], rnd), Ws["W2"], Ws["b2"], rnd), Ws["W3"], Ws["b3"])
    conf = torch.zeros(16, 16, dtype=torch.int64)
    if rows == 0:
        return torch.zeros(0, dtype=F64), 0, conf, z
    loss, pred, _ = head(z, y)
    for a, b in zip(y.tolist(), pred.tolist()):
        conf[a, b] += 1
    return loss, int((pred == y).sum()), conf, z


# ---------------------------------------------------------------------------------------------
# parameter rows
# ---------------------------------------------------------------------------------------------
NAMES = ("W1", "b1", "W2", "b2", "W3", "b3")


def shapes(D):
    D0, D1, D2, D3 = D
    return {"W1": (D1, D0), "b1": (D1,), "W2": (D2, D1), "b2": (D2,), "W3": (D3, D2), "b3": (D3,)}


def offsets(D):
    """The engine's contiguous row: W1 | b1 | W2 | b2 | W3 | b3. Returns ``(offsets, numel)``."""
    off, o = {}, 0
    for k, s in shapes(D).items():
        off[k] = o
        o += int(np.prod(s))
    return off, o


def pack(W, D):
    """``{name: [P, ...]}`` -> ``[P, numel]`` float64."""
    return torch.cat([W[k].reshape(W[k].shape[0], -1) for k in NAMES], 1)


def unpack(flat, D):
    off, _ = offsets(D)
    return {k: flat[..., off[k]: off[k] + int(np.prod(s))].reshape(*flat.shape[:-1], *s) for k, s in shapes(D).items()}


# ---------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------
PIXELS = (0, 1, 2, 3)  # and 200 for one pixel in 16: fc1 sums beyond 8 bits, so the bf16 rounding decides
NNZ = 64  # non-zero weights of a row in the exact families: the sums stay far below 2^24 units at every width


def bpad(B):
    return (B + 31) // 32 * 32


def valid_rows(B):
    """[full, partial, none]: the partial peer holds an odd number of rows below ``B`` (``B = 1``: one row)."""
    return [B, (B // 2) | 1 if B > 1 else 1, 0]


def _unit(K, rms):
    return 2.0 ** -math.ceil(math.log2(2.0 * math.sqrt(K) * rms))


def units(D):
    """The grids of the ``exact`` family: fc1's sums are integers times ``u[0]``, fc2's times ``u[0] u[1]``, fc3's
    times ``u[0] u[1] u[2]`` (powers of two that keep the activations and logits of order 1)."""
    rms = math.sqrt(200.0 ** 2 / 16 + 3.5 * 15 / 16)
    return _unit(min(D[0], NNZ), rms), _unit(min(D[1], NNZ) / 2, 1.0), _unit(min(D[2], NNZ) / 2, 1.0)


def _weights(g, D, family):
    D0, D1, D2, D3 = D
    W = {}
    if family == "randn":
        sc = {"W1": 1.0 / (math.sqrt(D0) * 96.0), "W2": 1.5 / math.sqrt(D1), "W3": 1.5 / math.sqrt(D2)}
        for k, s in shapes(D).items():
            t = torch.randn(P, *s, generator=g) * (sc[k] if k[0] == "W" else 0.25)
            W[k] = t.float().double()  # the fp32 master row
        return W
    u = units(D)
    grid = {"W1": u[0], "b1": u[0] * 16, "W2": u[1], "b2": u[0] * u[1] * 64, "W3": u[2], "b3": u[0] * u[1] * u[2] * 256}
    for k, s in shapes(D).items():
        lim = 3 if k[0] == "W" else 4
        W[k] = torch.randint(-lim, lim + 1, (P, *s), generator=g).double() * grid[k]
        if k[0] == "W" and s[1] > NNZ:
            W[k] = W[k] * (torch.rand(P, *s, generator=g) < NNZ / s[1])
    if family == "exact_tie" and D3 > 1:  # classes 0 and 1 always tie: the first one wins
        W["W3"][:, 1] = W["W3"][:, 0]
        W["b3"][:, 1] = W["b3"][:, 0]
    return W


def _pixels(g, family, *shape):
    if family == "randn":
        return torch.randint(0, 256, shape, generator=g).to(torch.uint8)
    x = torch.tensor(PIXELS, dtype=torch.uint8)[torch.randint(0, len(PIXELS), shape, generator=g)]
    return torch.where(torch.randint(0, 16, shape, generator=g) == 0, torch.tensor(200, dtype=torch.uint8), x)


def case(D, B, family, step=0, n_test=(517, 70, 512), active=(1, 1, 1), seed=0):
    """3 peers. Training: peer ``p`` holds ``step * B + valid_rows(B)[p]`` samples, already in epoch order (the
    batch buffer's rows), so step ``step`` sees ``[B, odd < B, 0]`` valid rows. Test: ``n_test`` rows per peer.
    ``W``: ``{name: [P, ...]}`` float64 values of the fp32 master (``exact``: bf16 values, the shadow is the same)."""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * D[0] + 31 * D[1] + 17 * D[2] + 5 * D[3] + B + 3 * step + sum(map(ord, family)))
    rows = valid_rows(B)
    n = [step * B + r for r in rows]
    c = dict(D=tuple(D), B=B, Bpad=bpad(B), family=family, step=step, rows=rows, n=n, n_test=list(n_test), active=list(active))
    c["W"] = _weights(g, D, family)
    c["xb"] = [_pixels(g, family, n[p], D[0]) for p in range(P)]
    c["yb"] = [torch.randint(0, D[3], (n[p],), generator=g) for p in range(P)]
    c["xt"] = [_pixels(g, family, n_test[p], D[0]) for p in range(P)]
    c["yt"] = [torch.randint(0, D[3], (n_test[p],), generator=g) for p in range(P)]
    return c


def batch(case, p, rows=None, step_idx=None):
    """The valid rows of peer ``p`` at step ``step_idx`` (default: the case's step) as ``(X float64, y int64)``."""
    s = case["step"] if step_idx is None else step_idx
    lo = s * case["B"]
    r = max(0, min(case["B"], case["n"][p] - lo)) if case["active"][p] else 0
    if rows is not None:
        r = rows
    return case["xb"][p][lo: lo + r].double(), case["yb"][p][lo: lo + r].long()


# the training cases of tests/test_mlp_fused_gpu.py: (D0, D1, D2, D3), B, step. Every head instantiation
# (256,128) (128,64) (256,256) (512,256) (128,128) (64,64) (512,128), every D0 of {8, 40, 784, 1032, 2048}, every D3
# of {1, 10, 16} and every B of {1, 32, 40, 256} appears at least once; 784-256-128-10 at B = 40.
TRAIN_CASES = [
    ((784, 256, 128, 10), 40, 0),
    ((8, 128, 64, 1), 1, 0),
    ((40, 256, 256, 16), 32, 1),
    ((1032, 512, 256, 10), 40, 0),
    ((2048, 128, 128, 16), 32, 0),
    ((40, 64, 64, 10), 256, 0),
    ((784, 512, 128, 1), 32, 1),
    ((8, 256, 128, 16), 256, 0),
    ((1032, 64, 64, 10), 1, 0),
    ((2048, 256, 128, 10), 40, 1),
    ((784, 128, 64, 16), 32, 0),
    ((40, 128, 128, 10), 40, 0),
]
FAMILIES = ("exact", "randn")
# evaluation: (dims, family, n_test, active)
EVAL_CASES = [
    ((784, 256, 128, 10), "exact", (517, 70, 512), (1, 1, 1)),
    ((40, 128, 64, 16), "exact_tie", (512, 517, 70), (1, 1, 0)),
    ((1032, 64, 64, 1), "exact", (70, 512, 517), (1, 1, 1)),
]


def case_id(c):
    return "-".join(map(str, c[0])) + f"-B{c[1]}" + (f"-s{c[2]}" if len(c) > 2 and not isinstance(c[2], tuple) else "")


# ---------------------------------------------------------------------------------------------
# optimizer (the oracle of opt_update lives in _fl_ops_ref)
# ---------------------------------------------------------------------------------------------
OPT_VARIANTS = {
    "sgd": dict(kind=1, lr=2.0 ** -6, momentum=0.0, wd=0.0, nesterov=False),
    "nesterov_wd": dict(kind=1, lr=2.0 ** -6, momentum=0.9, wd=5e-4, nesterov=True),
    "adam_t0": dict(kind=0, lr=1e-3, t0=0),
    "adam_t7": dict(kind=0, lr=1e-3, t0=7, wd=1e-4),
    "fedprox": dict(kind=1, lr=2.0 ** -6, momentum=0.9, wd=0.0, nesterov=False, mu=0.01),
    "scaffold": dict(kind=0, lr=1e-3, t0=3, scaffold=True),
}
BETA1, BETA2, EPS = 0.9, 0.999, 1e-8


def opt_step(hp, w, g, m, v, step, anchor=None, cg=None, cl=None):
    """One optimizer step on flat float64 arrays through ``_fl_ops_ref``. Returns ``(w', m', v', units_w, units_m,
    units_v)`` (``None`` for what the variant does not touch)."""
    mu = hp.get("mu", 0.0)
    if hp["kind"] == 0:
        return R.adam_step(w, g, m, v, hp.get("t0", 0) + step + 1, hp["lr"], BETA1, BETA2, EPS, hp.get("wd", 0.0), anchor, mu, cg, cl)
    w1, m1, uw, um = R.sgd_step(w, g, m, hp["lr"], hp["momentum"], hp.get("wd", 0.0), hp["nesterov"], anchor, mu, cg, cl)
    return w1, m1, None, uw, um, None


# ---------------------------------------------------------------------------------------------
# a whole epoch of plain SGD (one peer)
# ---------------------------------------------------------------------------------------------
def mm64(a, b):
    return a @ b


def mm32_permuted(g):
    """The same products with the sum accumulated in fp32 over a permuted reduction axis: what any other
    accumulation order of a kernel may do to a sum."""
    def mm(a, b):
        idx = torch.randperm(a.shape[1], generator=g)
        return (a[:, idx].float() @ b[idx].float()).double()

    return mm


def _opt_f32(hp, w, g, m, v, k):
    """One ``torch.optim`` step of one tensor with every operation in fp32 (the twin's optimizer). ``k``: the step count
    from 1. Returns ``(w', m', v')`` as float64 values of fp32 numbers."""
    t = lambda a: torch.tensor(R.f32(a), dtype=F32)
    w, g = w.float(), g.float()
    wd = hp.get("wd", 0.0)
    if wd != 0.0:
        g = g + t(wd) * w
    if hp["kind"] == 0:
        b1, b2 = R.f32(BETA1), R.f32(BETA2)
        m = t(b1) * m.float() + t(1.0 - b1) * g
        v = t(b2) * v.float() + t(1.0 - b2) * g * g
        w = w - t(R.f32(hp["lr"]) / (1.0 - b1 ** k)) * (m / (v.sqrt() * t(1.0 / math.sqrt(1.0 - b2 ** k)) + t(EPS)))
        return w.double(), m.double(), v.double()
    mom = hp.get("momentum", 0.0)
    if mom != 0.0:
        m = t(mom) * m.float() + g
        g = g + t(mom) * m if hp.get("nesterov", False) else m
        m = m.double()
    return (w - t(hp["lr"]) * g).double(), m, v


def epoch(W, x, y, perm, B, hp, rnd=bf16, mm=mm64, f32=False, state=None):
    """``W``: one peer's ``{name: float64}`` master values, ``x`` ``[n, D0]``, ``y`` ``[n]``, ``perm`` the epoch order. One pass in
    batches of ``B`` (the last one partial), one step of the optimizer ``hp`` (an ``OPT_VARIANTS`` entry without extras,
    through :func:`opt_step`) after each; the bf16 roundings of :func:`step` and no other (``rnd = ident``: none at all).
    ``state``: ``(m, v, steps done)`` of an earlier epoch of the same fit (default: zero moments, no step done).
    Returns ``(W', (m', v', steps done))``.

    ``f32`` (with ``mm = mm32_permuted(g)``): everything the kernels hold in fp32 is fp32 here too: every sum (the
    products, the bias gradients, the softmax) accumulated in fp32, in another order where ``mm`` does it, the
    optimizer in fp32 arithmetic and the master row and the moments rounded to fp32 after each update. Against the
    float64 run this measures the oracle's own sensitivity: the floor below which two correct fp32 implementations
    of the epoch cannot be told apart."""
    W = {k: v.clone() for k, v in W.items()}
    D3 = W["b3"].shape[0]
    zero = torch.zeros((), dtype=F64)
    if state is None:
        state = ({k: torch.zeros_like(v) for k, v in W.items()}, {k: torch.zeros_like(v) for k, v in W.items()}, 0)
    m, v, done = dict(state[0]), dict(state[1]), state[2]
    for s in range(0, len(perm), B):
        idx = torch.as_tensor(perm[s: s + B], dtype=torch.int64)
        X, yy = x[idx].double(), y[idx].long()
        rows = X.shape[0]
        w1, w2, w3 = rnd(W["W1"]), rnd(W["W2"]), rnd(W["W3"])
        H1 = rnd((mm(X, w1.t()) + W["b1"]).clamp_min(0))
        H2 = rnd((mm(H1, w2.t()) + W["b2"]).clamp_min(0))
        z = mm(H2, w3.t()) + W["b3"]
        if f32:
            sm = torch.softmax(z.float(), 1)
            sm[torch.arange(rows), yy] -= 1.0
            dl = rnd((sm / rows).double())
        else:
            dl = dlogits(z, yy, rnd=rnd)[:, :D3]
        dH2 = rnd(torch.where(H2 > 0, mm(dl, w3), zero))
        dH1 = rnd(torch.where(H1 > 0, mm(dH2, w2), zero))
        one = torch.ones(rows, 1, dtype=F64)
        bsum = (lambda t: mm(t.t(), one)[:, 0]) if f32 else (lambda t: t.sum(0))
        g = {"W1": mm(dH1.t(), X), "b1": bsum(dH1), "W2": mm(dH2.t(), H1), "b2": bsum(dH2), "W3": mm(dl.t(), H2), "b3": bsum(dl)}
        for k in W:
            if f32:
                W[k], m[k], v[k] = _opt_f32(hp, W[k], g[k], m[k], v[k], done + 1)
            else:
                o = opt_step(dict(hp, t0=0), W[k].numpy(), g[k].numpy(), m[k].numpy(), v[k].numpy(), done)
                W[k] = torch.from_numpy(np.asarray(o[0], dtype=np.float64))
                m[k] = m[k] if o[1] is None else torch.from_numpy(np.asarray(o[1], dtype=np.float64))
                v[k] = v[k] if o[2] is None else torch.from_numpy(np.asarray(o[2], dtype=np.float64))
        done += 1
    return W, (m, v, done)


def sgd_epoch(W, x, y, perm, B, lr, rnd=bf16, mm=mm64, f32=False):
    """One epoch of plain SGD, ``w -= fp32(lr) * g`` after each batch: :func:`epoch` with that optimizer. Returns the
    new master values."""
    return epoch(W, x, y, perm, B, dict(kind=1, lr=lr, momentum=0.0, wd=0.0, nesterov=False), rnd, mm, f32)[0]


def rel_update(got, ref, start):
    """``|(got - start) - (ref - start)| / |ref - start|`` in the 2-norm: the relative update error of one tensor."""
    return float(((got - start) - (ref - start)).norm() / ((ref - start).norm() + 1e-300))


# ---------------------------------------------------------------------------------------------
# the fp32 epoch kernels (mlp_persistent_f32.hip, mlp_persistent_f32v2.hip) and mlp_eval_f32
# ---------------------------------------------------------------------------------------------
# D1 = 256 and D2 = 128 are fixed there. What follows is the float64 model (``rnd = ident``) with the per-element
# bounds of those kernels' fp32 arithmetic, u = 2^-24, gamma(k) = k u / (1 - k u).
#
# Forward. On the ``exact`` / ``exact_tie`` weight family with the pixel family above every term of H1, H2 and the
# logits is an integer multiple of ``units(D)``'s grid and ``sum |term| / unit < 2^24`` (:func:`grid_ratios`), so
# every fp32 partial sum is exact in ANY order, whichever way the K steps, the K parts, the waves and the heads
# split it: the kernel's H1, H2 and logits ARE the float64 ones, and with them the relu masks, the first maximum
# and the ties. W1 / b1 reach the bf16 MFMA as ``split3``'s hi + mid + lo (exact), X as bf16 (exact).
#
# Layout 3's H2 (``headr32``) splits BOTH operands and keeps six of the nine cross terms. bf16 has 8 significant
# bits, so RNE leaves ``|mid| <= 2^-8 |x|`` and ``|lo| <= 2^-16 |x|``; the dropped ``mid lo + lo mid + lo lo`` are at most
# ``(2^-23 + 2^-32) |a b|`` per product (:data:`L3_DROP`; the worst case, reached when both remainders sit at half
# an ulp: about one fp32 ulp of the product, not 2^-32 of it). On the grid H1 has at most 16 significant bits
# and W2 at most 3: ``lo(H1) = mid(W2) = lo(W2) = 0``, the dropped terms vanish and H2 is exact there too.
# :func:`h2_l3` emulates the six terms; :func:`h2_l3_bound` is the bound for arbitrary fp32 operands.
#
# Softmax / dlogits. Layout 1's heads: ``e = __expf(z - mx)`` (``v_exp_f32``), ``se`` by a 4-level butterfly,
# ``p = e * v_rcp_f32(se)``, ``d = p / rows`` and for the true class ``-(sum_{c != y} p_c) / rows`` (a second butterfly);
# ``logp = z - (mx + __logf(se))`` for the loss, as ``mlp_head``: ``eps_lp`` of the module docstring holds unchanged.
# With R the row's logit range: ``z - mx`` rounds once (u R on the exponent), ``__expf`` is ``e_exp = 2 u (1 + R)``:
# ``a = e_exp + u R`` relative on e; se adds 4 u; ``v_rcp_f32`` 1 ulp = 2 u (the CDNA ISA reference's figure, the source
# the module docstring cites for ``v_exp`` / ``v_log``); the product u: p is off by ``2 a + 7 u`` (relative, p <= 1);
# the true class's butterfly 4 u more on a sum <= 1; the IEEE division by rows u:
# ``eps_A = 2 a + 12 u``. Layouts 2 and 3 (and no other instruction sequence exists) use the library ``expf`` / ``logf``
# (1 ulp each, within what ``eps_lp`` allows the fast pair) and ``p = expf(logp)``: ``eps_lp`` on the argument acts on
# p <= 1, ``expf`` 2 u, the butterfly 4 u, the division u: ``eps_B = eps_lp + 7 u``. :func:`eps_softmax32` returns
# ``eps_dl = max(eps_A, eps_B)``: ``|rows * dlogits - (softmax - onehot)| <= eps_dl`` for every layout.
#
# Backward. A sum of K products in ANY order (any split into partial sums; additions of exact zeros are exact) is
# off by at most ``gamma(K) sum |term|``: each term passes one product rounding at most (none in an fma chain) and at
# most K - 1 additions. With exact masks, recursively (:func:`bounds32`):
#   ``e_dl = eps_dl / rows``
#   ``e_dH2 = [H2 > 0] (gamma(16) |dl| |W3| + e_dl colsum |W3|)``         (f32 MFMA over the 16 class slots)
#   ``e_dH1 = [H1 > 0] (gamma(128) |dH2| |W2| + e_dH2 |W2|)``
#   ``dW3, db3, dW2, db2``: ``gamma(rows) sum |term| + sum_r e(upstream)[r] |other operand[r]|``   (f32 MFMA over the batch)
#   ``dW1, db1``: dH1 enters as hi + mid + lo against the exact X (column D0 = 1 carries db1): ``3 rows`` exact products,
#   ``sum |term| <= (1 + 2^-7) |dH1| X``: ``(gamma(3 rows) + 12 u) (1 + 2^-7) sum |term| + sum_r e_dH1[r] X[r]``. The 12 u: neither
#   guide nor the ISA reference says how ``v_mfma_f32_16x16x32_bf16`` rounds when it adds its 32 products to C, and the
#   one-row check below finds it one ulp off the correctly rounded sum in 0.3 % of the elements; so each of the
#   at most 6 such instructions an element passes (3 terms x 2 batch tiles of 32 rows) is taken as faithful only:
#   2 u of the sum of the sizes of everything added so far.
# Everything is evaluated on the oracle's own values; the kernel's differ from them by the bounds themselves, a
# second-order term below 2^-10 of each bound: the factor :data:`SECOND`.
#
# One valid row. The other rows of dlogits, dH2 and dH1 are exact zeros, so db3, db2 and db1 ARE the kernel's
# dlogits, dH2 and dH1 of that row (db1: ``lo + mid + hi`` against the bias input 1 reassembles dH1 exactly), and dW3 and
# dW2 are their products with the exact H2 and H1 rounded ONCE, bit for bit: the f32 MFMA's fma onto 0
# (:func:`outer32`). For dW1 ``lo x`` is exact (16 bits), ``+ mid x`` is exact (``(mid + lo) x`` has at most 16 + 8 bits) and
# ``+ hi x`` is the one inexact addition, of the exact ``dH1 x``. If the bf16 MFMA rounded that sum to nearest, dW1 would
# be ``outer32`` too. MI355X: it is in 99.7 % of the elements and the OTHER fp32 neighbour of the exact product in
# the rest (658 of 200 704 at D0 = 784 in layout 1 at every K split, 846 in layouts 2 and 3), so the instruction
# rounds faithfully, not to nearest, and the check is the faithful one: ``|dW1 - dH1 x| <= 2^-23 |dH1 x|``, one ulp at
# most (:data:`FAITHFUL`). db1 passes the same split, so a term missing from the split is missing from both and
# cannot show in that comparison: the GPU test looks at db1's low significand byte for it. The K splits divide X's
# columns, never the batch: the same holds in every layout. fp32 denormals are left out of the bit comparison:
# below 2^-100 the check is an absolute 2^-100.
#
# ``upd32`` (mlp_f32_common.h), one element, every operation an fma or a single rounded product (:func:`upd32`):
#   ``g1 = fma(wdmu, w, g)``: u |g1| (exact when wdmu = 0); FedProx ``e = fl(-mu anchor)``: u |e|, ``g2 = g1 + e``: u |g2|;
#   SGD: ``m' = fma(mom, m, g)``: u |m'| + dg; Nesterov ``g' = fma(mom, m', g)``: u |g'| + mom bm + dg; ``w' = fma(-lr, g', w)``:
#   u |w'| + lr dg'; SCAFFOLD ``e = fl(cg - cl)``, ``w'' = fma(-lr, e, w')``: u |w''| + lr u |e| more.
#   Adam: ``1 - beta`` is exact in fp32 (Sterbenz); ``m' = fma(b1, m, fl(c1 g))``: u |m'| + u c1 |g| + c1 dg;
#   ``v' = fma(b2, v, fl(c2 fl(g g)))``: u v' + c2 (2 u g^2 + 2 |g| dg);
#   ``den = fma(v_sqrt_f32(v'), inv, eps)``: ``v_sqrt_f32`` 1 ulp = 2 u (same source), ``inv = fp32(1 / sqrt(1 - b2^k))`` formed
#   in double and trusted to 1 ulp (2 u): d_den = inv d_sq + 2 u sq inv + u den with
#   d_sq = 2 u sq + min(sqrt(bv), bv / sq) (+ 2^-60: a denormal v' may be flushed, sqrt <= 2^-63);
#   ``q = fl(m' v_rcp_f32(den))``: dq = bm / den + |q| (d_den / den + 2 u + u); ``w' = fma(-lr_t, q, w)`` with ``lr_t =
#   fp32(lr / (1 - b1^k))`` to 1 ulp: bw = u |w'| + lr_t dq + 2 u lr_t |q|.
# These are NOT ``opt_update``'s unit counts (``_fl_ops_ref``): that code divides and calls ``sqrtf``.
#
# Loss sum. Each valid row adds ``-logp``, off by ``eps_lp``; the lanes, waves and epochs add the n terms in fp32 in
# some tree: ``n eps_lp + gamma(n) sum loss`` (:func:`loss_bound`). The same for ``mlp_eval_f32`` (library ``expf`` / ``logf``).
SECOND = 1.0 + 2.0 ** -10
L3_DROP = 2.0 ** -23 + 2.0 ** -32
PD1, PD2 = 256, 128
TINY32 = 2.0 ** -100
FAITHFUL = 2.0 ** -23  # one fp32 ulp, relative: the bf16 MFMA's accumulation (section comment)


# ``randn32``: the ``randn`` family with each tensor scaled by a power of two (the product of the three matrices' factors is
# 1: the logits keep their size). At lr 1e-4 the unscaled family's updates of the biases, of W2 and of W3 over 3
# steps are of the order of the fp32 rounding of the master row itself (the twin's floor was 1e-3 for b1 and
# 5e-4 for W2 at D0 = 40); with these factors every tensor's floor is below 1e-4 (asserted by
# ``test_mlp_ref_cpu.py`` for every case of part (d)).
RANDN32_SCALE = {"W1": 16.0, "W2": 0.125, "W3": 0.5, "b1": 2.0 ** -10, "b2": 2.0 ** -10, "b3": 2.0 ** -10}
# ``randn16``: the same matrices with larger b2 and b3, for part (d) of the bf16 epoch kernel's tests (section below)
RANDN16_SCALE = dict(RANDN32_SCALE, b2=2.0 ** -7, b3=2.0 ** -4)

# The cases of tests/test_mlp_f32_oracle_gpu.py: shapes (D0, D3, B), layouts (gang layout, owner K split, the H1 / dH2
# fragment switches), and the training rows of the two peers.
F32_MAIN, F32_RAGGED = (784, 10, 64), (40, 16, 24)
F32_SHAPES = [F32_MAIN, F32_RAGGED, (8, 1, 32), (32, 10, 24), (792, 16, 32), (784, 1, 24)]  # every D0, D3 and B on the shipping layout
F32_LAYOUTS = {"v1ks1": (1, 1, -1), "v1ks1_rows": (1, 1, 0), "v1ks2": (1, 2, -1), "v1ks4": (1, 4, -1), "v1ks8": (1, 8, -1), "v2": (2, 1, -1),
               "v3ks1": (3, 1, -1), "v3ks2": (3, 2, -1)}
F32_ONE_STEP = {64: [(1, 64), (2, 63), (31, 33), (32, 1)], 32: [(1, 32), (2, 31)], 24: [(1, 24), (2, 23)]}  # one step of that many rows
F32_STEPS = {64: [(100, 128), (150, 192), (300, 320)], 32: [(50, 64), (80, 96), (150, 160)], 24: [(40, 48), (60, 72), (110, 120)]}  # 2, 3, 5 steps: partial, full
F32_LEARN = {64: (150, 300), 32: (80, 150), 24: (60, 110)}  # 3 and 5 steps, the last one partial
F32_LEARN_HP = {"sgd": dict(kind=1, lr=1e-4, momentum=0.0, wd=0.0, nesterov=False), "nesterov_wd": dict(kind=1, lr=1e-4, momentum=0.9, wd=5e-4, nesterov=True)}
# ((D0, D3), family, test rows of the two peers, case seed: one at which the tying classes 0 and 1 are the maximum of many rows)
F32_EVAL = [((784, 10), "exact", (517, 70), 0), ((40, 16), "exact_tie", (1, 512), 2), ((792, 16), "exact_tie", (517, 1), 1), ((8, 1), "exact", (70, 512), 0)]


def f32_layout_cases():
    """``(layout, shape)``: every layout at the main and at the ragged shape, every shape on the shipping layout."""
    return [(l, s) for l in F32_LAYOUTS for s in (F32_MAIN, F32_RAGGED)] + [("v1ks1", s) for s in F32_SHAPES[2:]]


def epoch_perm32(n, ep, p, seed=0):
    """The pinned epoch order of peer ``p`` in the fp32 oracle tests."""
    return torch.randperm(n, generator=torch.Generator().manual_seed(1000 * ep + 10 * seed + p)).numpy()


def dims32(D0, D3):
    return (D0, PD1, PD2, D3)


def f32_family(D3):
    """The grid family of a training case: with 16 classes the one whose classes 0 and 1 tie in every row."""
    return "exact_tie" if D3 == 16 else "exact"


def learn_refs(c, p, hp, epochs=1):
    """Part (d): peer ``p``'s float64 epoch(s) under the pinned orders and the fp32 twin's: ``(ref, alt)``."""
    out = []
    for kw in (dict(), dict(mm=mm32_permuted(torch.Generator().manual_seed(p)), f32=True)):
        W, st = c["W"][p], None
        for ep in range(epochs):
            W, st = epoch(W, c["x"][p], c["y"][p], epoch_perm32(c["n"][p], ep, p), c["B"], hp, rnd=ident, state=st, **kw)
        out.append(W)
    return out


def case32(D0, D3, B, family, n, n_test=(4, 4), seed=0):
    """2 peers of the fp32 engine with their own weights (peers 0 and 1 of :func:`_weights`) and data: ``n[p]``
    training rows and ``n_test[p]`` test rows of the family's pixels, labels uniform in ``[0, D3)``."""
    D = dims32(D0, D3)
    g = torch.Generator().manual_seed(7 + 1000003 * seed + 7919 * D0 + 5 * D3 + B + 131 * n[0] + 257 * n[1] + 17 * sum(n_test) + sum(map(ord, family)))
    scale = {"randn32": RANDN32_SCALE, "randn16": RANDN16_SCALE}.get(family)
    W = _weights(g, D, "randn" if scale else family)
    if scale:
        W = {k: v * scale[k] for k, v in W.items()}
        family = "randn"
    c = dict(D=D, B=B, family=family, n=list(n), n_test=list(n_test), W=[{k: v[p] for k, v in W.items()} for p in range(2)])
    c["x"] = [_pixels(g, family, n[p], D0) for p in range(2)]
    c["y"] = [torch.randint(0, D3, (n[p],), generator=g) for p in range(2)]
    c["xt"] = [_pixels(g, family, n_test[p], D0) for p in range(2)]
    c["yt"] = [torch.randint(0, D3, (n_test[p],), generator=g) for p in range(2)]
    return c


def forward32(W, X):
    H1 = fc(X, W["W1"], W["b1"], ident)
    H2 = fc(H1, W["W2"], W["b2"], ident)
    return H1, H2, logits(H2, W["W3"], W["b3"])


def grid_ratios(W, X, D):
    """``sum |term| / unit`` of the worst fc1, fc2 and fc3 sum of the rows ``X`` on ``units(D)``'s grid (and an assertion that
    every sum lies on it): all three below 2^24 make the fp32 forward exact in any order."""
    u = units(D)
    H1, H2, _ = forward32(W, X)
    out = []
    for A, w, b, unit in ((X, W["W1"], W["b1"], u[0]), (H1, W["W2"], W["b2"], u[0] * u[1]), (H2, W["W3"], W["b3"], u[0] * u[1] * u[2])):
        pre = fc_pre(A, w, b)[0]
        assert torch.equal(pre / unit, (pre / unit).round()), "a sum off its grid"
        out.append(float(exactness(A, w, b, unit).max()) if A.shape[0] else 0.0)
    return out


def split3(x):
    """``split3`` of mlp_f32_common.h on float64 values of fp32 numbers: ``(hi, mid, lo)``, bf16 each, ``hi + mid + lo == x``."""
    hi = bf16(x)
    r = x - hi
    mid = bf16(r)
    return hi, mid, bf16(r - mid)


def h2_l3(H1, W2, b2):
    """Layout 3's H2 before the relu, in exact arithmetic: six of the nine cross terms of the two splits."""
    ah, am, al = split3(H1)
    bh, bm, bl = split3(W2)
    return al @ bh.t() + ah @ bl.t() + am @ bm.t() + am @ bh.t() + ah @ bm.t() + ah @ bh.t() + b2


def h2_l3_bound(H1, W2, b2):
    """``|H2 of layout 3 - relu(H1 W2^T + b2)|`` for arbitrary fp32 operands: the dropped cross terms, 6 * 256 exact
    products summed in fp32 in some order, and the bias addition."""
    mag = H1.abs() @ W2.abs().t()
    return SECOND * ((L3_DROP + gamma(6 * PD1) * (1 + 2.0 ** -7)) * mag + U * (mag + b2.abs()))


def eps_softmax32(z):
    """``(eps_lp, eps_dl)`` of the section comment for the logits ``z`` (the worst row)."""
    if z.numel() == 0:
        return 0.0, 0.0
    eps_lp = eps_softmax(z)[0]
    rng = float((z.amax(1) - z.amin(1)).max())
    a = 2 * U * (1 + rng) + U * rng
    return eps_lp, max(2 * a + 12 * U, eps_lp + 7 * U)


def step32(W, X, y):
    """One step of one peer in float64: the stage tensors, the loss terms, the predictions (first maximum), the six
    gradients, and ``eps_lp`` / ``eps_dl`` of its logits. ``dlog`` is ``[rows, D3]``."""
    D3 = W["b3"].shape[0]
    rows = X.shape[0]
    H1, H2, z = forward32(W, X)
    loss, pred, _ = head(z, y)
    dl = dlogits(z, y, rnd=ident)[:, :D3]
    dH2 = dgrad(dl, W["W3"], H2, ident)
    dH1 = dgrad(dH2, W["W2"], H1, ident)
    pad = torch.zeros(rows, 16, dtype=F64)
    pad[:, :D3] = dl
    s = dict(X=X, y=y, rows=rows, H1=H1, H2=H2, z=z, loss=loss, pred=pred, dlog=dl, dH2=dH2, dH1=dH1)
    s["g"] = wgrads(X, H1, H2, dH1, dH2, pad, D3)
    s["eps_lp"], s["eps_dl"] = eps_softmax32(z)
    return s


def bounds32(s, W):
    """The per-element bounds of the six gradients of :func:`step32`'s step (section comment, "Backward")."""
    rows, X, H1, H2 = s["rows"], s["X"], s["H1"], s["H2"]
    dl, dH2, dH1 = s["dlog"].abs(), s["dH2"].abs(), s["dH1"].abs()
    W3a, W2a = W["W3"].abs(), W["W2"].abs()
    e_dl = s["eps_dl"] / rows
    e_dH2 = (H2 > 0) * (gamma(16) * (dl @ W3a) + e_dl * W3a.sum(0)[None, :])
    e_dH1 = (H1 > 0) * (gamma(PD2) * (dH2 @ W2a) + e_dH2 @ W2a)
    gw, g1 = gamma(rows), (gamma(3 * rows) + 12 * U) * (1 + 2.0 ** -7)
    b = {
        "W3": gw * (dl.t() @ H2) + e_dl * H2.sum(0)[None, :].expand(dl.shape[1], -1),
        "b3": gw * dl.sum(0) + rows * e_dl,
        "W2": gw * (dH2.t() @ H1) + e_dH2.t() @ H1,
        "b2": gw * dH2.sum(0) + e_dH2.sum(0),
        "W1": g1 * (dH1.t() @ X) + e_dH1.t() @ X,
        "b1": g1 * dH1.sum(0) + e_dH1.sum(0),
    }
    return {k: SECOND * v for k, v in b.items()}


def outer32(d, a):
    """``fp32(d[i] * a[j])``: the exact product of two fp32 vectors (48 bits: exact in float64), rounded once."""
    return (d[:, None] * a[None, :]).float().double()


def loss_bound(losses, eps_lp):
    """Bound of the fp32 sum of the rows' loss terms (any tree) against their float64 sum."""
    n = losses.numel()
    return SECOND * (n * eps_lp + gamma(max(n, 1)) * float(losses.abs().sum()))


def moments32(hp, w, gs, bs, k0=0):
    """The moments after ``upd32`` steps on the gradients ``gs`` (each known to its ``bs``) with the weights frozen (``lr = 0``, no
    weight decay), from zero moments, the first step being optimizer step ``k0 + 1``: ``(m, v, bm, bv)``. Each step's bound
    is :func:`upd32`'s plus the previous step's carried through the recursion's own factor (beta1 / beta2, or the
    momentum)."""
    assert R.f32(hp["lr"]) == 0.0 and hp.get("wd", 0.0) == 0.0
    m, v = torch.zeros_like(w), torch.zeros_like(w)
    bm, bv = torch.zeros_like(w), torch.zeros_like(w)
    cm, cv = (R.f32(BETA1), R.f32(BETA2)) if hp["kind"] == 0 else (R.f32(hp["momentum"]), 0.0)
    for i, (g, b) in enumerate(zip(gs, bs)):
        w1, m, v, _, bm1, bv1 = upd32(hp, w, g, m, v, k0 + i + 1, dg=b)
        assert torch.equal(w1, w)
        bm, bv = bm1 + cm * bm, bv1 + cv * bv
    return m, v, bm, bv


def _hp32(hp):
    return {k: (R.f32(v) if isinstance(v, float) else v) for k, v in hp.items()}


def adam_coeffs(hp, k):
    """``(lr_t, inv)`` of ``persist::BiasCorr`` at optimizer step ``k`` (from 1): formed in double from the fp32 betas,
    rounded to fp32."""
    b1, b2 = R.f32(BETA1), R.f32(BETA2)
    return R.f32(R.f32(hp["lr"]) / (1.0 - b1 ** k)), R.f32(1.0 / math.sqrt(1.0 - b2 ** k))


def adam_w32(hp, w, m1, v1, k, bm=0.0, bv=0.0, coeffs=None):
    """The weight after ``upd32``'s Adam tail from the new moments ``m1``, ``v1`` (known to ``bm``, ``bv``) at step ``k``:
    ``(w', bound)``. ``coeffs``: ``(lr_t, inv, relative bound of lr_t, of inv)`` where the kernel forms them otherwise than
    ``persist::BiasCorr`` (:func:`adam_coeffs16`); the default is ``adam_coeffs`` trusted to one ulp each."""
    lr_t, inv, r_lr, r_inv = coeffs if coeffs is not None else (*adam_coeffs(hp, k), 2 * U, 2 * U)
    eps = R.f32(EPS)
    sq = torch.sqrt(v1)
    d_sq = 2 * U * sq + torch.minimum(torch.sqrt(torch.as_tensor(bv, dtype=F64) + 0 * sq), torch.as_tensor(bv, dtype=F64) / sq.clamp_min(1e-300)) + 2.0 ** -60
    den = sq * inv + eps
    d_den = inv * d_sq + r_inv * sq * inv + U * den
    q = m1 / den
    dq = bm / den + q.abs() * (d_den / den + 3 * U)
    w1 = w - lr_t * q
    return w1, SECOND * (U * w1.abs() + lr_t * dq + r_lr * lr_t * q.abs())


def upd32(hp, w, g, m, v, k, anchor=None, cg=None, cl=None, dg=0.0):
    """``upd32`` of mlp_f32_common.h on float64 values of the kernel's fp32 inputs (``g`` known to ``dg``): one step, ``k``
    the optimizer step from 1. ``hp``: an ``OPT_VARIANTS`` entry (``mu`` with ``anchor``: FedProx; ``cg`` / ``cl``: SCAFFOLD in
    update space). Returns ``(w', m', v', bw, bm, bv)``, the bounds absolute (section comment); ``m'`` is ``m`` where the
    variant leaves it alone, ``v'`` is ``v`` under SGD."""
    hp = _hp32(hp)
    wdmu = R.f32(hp.get("wd", 0.0) + (hp.get("mu", 0.0) if anchor is not None else 0.0))
    zero = torch.zeros_like(w)
    dg = dg + zero
    if wdmu != 0.0:
        g = g + wdmu * w
        dg = dg + U * g.abs()
    if anchor is not None:
        e = -hp["mu"] * anchor
        g = g + e
        dg = dg + U * e.abs() + U * g.abs()
    if hp["kind"] == 0:
        b1, b2 = R.f32(BETA1), R.f32(BETA2)
        m1 = b1 * m + (1.0 - b1) * g
        bm = U * m1.abs() + (1.0 - b1) * (U * g.abs() + dg)
        v1 = b2 * v + (1.0 - b2) * g * g
        bv = U * v1 + (1.0 - b2) * (2 * U * g * g + 2 * g.abs() * dg)
        w1, bw = adam_w32(hp, w, m1, v1, k, bm, bv)
        bm, bv = SECOND * bm, SECOND * bv
    else:
        mom, lr = hp.get("momentum", 0.0), hp["lr"]
        m1, v1, bm, bv = m, v, zero, zero
        gu, dgu = g, dg
        if mom != 0.0:
            m1 = mom * m + g
            bm = U * m1.abs() + dg
            gu, dgu = m1, bm
            if hp.get("nesterov", False):
                gu = mom * m1 + g
                dgu = U * gu.abs() + mom * bm + dg
            bm = SECOND * bm
        w1 = w - lr * gu
        bw = SECOND * (U * w1.abs() + lr * dgu)
    if cg is not None:
        e = cg - cl
        w1 = w1 - hp["lr"] * e
        bw = bw + SECOND * (U * w1.abs() + hp["lr"] * U * e.abs())
    return w1, m1, v1, bw, bm, bv


# ---------------------------------------------------------------------------------------------
# the bf16 epoch kernel (mlp_persistent.hip, mlp_persistent_epoch<BP, ADAM>)
# ---------------------------------------------------------------------------------------------
# D1 = 256 and D2 = 128 are fixed there too. The model is :func:`step`'s (bf16 where the kernel stores bf16: the
# matrices as the MFMA reads them, H1, H2, dlogits, dH2, dH1; the biases and every sum in fp32), per peer of a
# ``case32``, with an INTERVAL for everything behind the fast softmax.
#
# Forward. On the ``exact`` / ``exact_tie`` family the matrices are bf16 values already and every term of the three
# sums is a multiple of ``units(D)``'s grid; a bf16 rounding of a multiple of a power of two is one again, so the
# rounded H1 and H2 stay on the grid. With ``sum |term| / unit < 2^24`` (:func:`grid_ratios16`) the kernel's fp32 sums
# are exact however the 8 waves, the K steps and the MFMA split them: H1, H2, the logits, the relu masks and
# the first maximum are the oracle's, bit for bit.
#
# dlogits. ``mlp_persistent_epoch``'s head forms ``logp`` and ``d = (__expf(logp) - onehot) / rows`` exactly as ``mlp_head``
# does, so ``eps_sm`` of the module docstring holds unchanged: the fp32 ``d`` lies within ``e = eps_sm / rows`` of
# ``(softmax - onehot) / rows``, and, rounding being monotone, the stored bf16 value lies in
# ``[bf16(ref - e), bf16(ref + e)]``: one value for most elements, two neighbours where ``ref`` sits within ``e`` of a
# rounding boundary (the element "straddles"). With one class ``__expf(0) = exp2(0) = 1`` and ``__logf(1) = 0``
# exactly: ``d`` is an exact zero and the interval is ``[0, 0]``.
#
# dH2, dH1. ``dlogits W3`` has at most 16 terms, ``dH2 W2`` 128; on the grid of the finest bit of their own terms
# (:func:`_iratio`, taken over both ends of each interval) ``sum |term| / unit < 2^24``, so these fp32 sums are exact
# in any order as well, whichever value each upstream element took. An exact sum is monotone in each operand:
# the sum lies between the sums of the ends chosen by the sign of the weight (:func:`_isum`), the mask is exact, the
# bf16 rounding is monotone: ``dH2`` in ``[bf16(lo), bf16(hi)]``, and ``dH1`` from that in the same way.
#
# Gradients. The reference is the float64 sum over the batch of the products of the central values
# (``bf16(ref)`` carried through). The kernel's operand differs from the central one by at most the interval's
# width, so a gradient element's radius is ``sum_rows width[row] |other operand[row]|`` (nothing of second order: the
# other operand is exact), plus ``gamma(Bpad) sum |term|`` for the fp32 sum over the batch (two chained 32-row MFMAs,
# or Bpad scalar additions for db2 and db3, or 4 additions, two shuffles and up to four LDS atomics in arrival
# order for db1: any tree of at most Bpad additions; the MFMA's own rounding, faithful only, is 2 u per
# instruction and there are two at most). Where the element's own terms satisfy the exactness condition above
# (the finest bit of any dH row times the finest bit of the other operand's column, both ends of the intervals
# taken) that term is dropped: every order gives the same bits, the atomics of db1 included (elsewhere db1's
# arrival order is inside ``gamma(Bpad) >= gamma(4)`` like any other order). :func:`bounds16`.
#
# Reading the gradient. One Adam step at ``lr = 0`` without weight decay from fresh state leaves ``m = fl(c1 g)`` with
# ``c1 = 1 - beta1`` (exact in fp32, Sterbenz), ``v = fl(c2 fl(g g))`` and ``w`` bit-equal (``fma(-0, q, w)``): ``|m - c1 g_ref| <=
# c1 radius + u |c1 g|``. ``v`` against the kernel's own ``m``: ``g = (m / c1)(1 + d)``, ``|d| <= u``, so ``v = c2 (m / c1)^2`` within
# ``4 u`` relative (2 u from ``d``, the two product roundings) and an absolute 2^-125 where fp32 flushes.
#
# Bias correction. ``persist::bias_corr`` forms ``lr_t = lr / (1.f - __powf(beta1, k))`` and ``inv = 1.f / sqrtf(1.f -
# __powf(beta2, k))`` in fp32. ``__powf`` is taken as good to one ulp, the figure this module already assumes for
# ``v_exp_f32`` / ``v_log_f32`` (2 u relative): ``|b - beta^k| <= 2 u beta^k``. ``1 - b`` is exact for ``b >= 1/2`` and rounds once
# otherwise, so ``1 - beta^k`` is off by ``r(beta) = 2 u beta^k / (1 - beta^k) + u`` relative: at k = 1 about
# ``2 u beta2 / (1 - beta2) = 1.2e-4`` for beta2 and 18 u for beta1. The division rounds once (u): ``lr_t`` to ``r(beta1) + u``.
# ``sqrtf`` is taken as 1 ulp (2 u) on a value off by ``r(beta2)``, half of which it passes on, and the division
# rounds once: ``inv`` to ``r(beta2) / 2 + 3 u``. :func:`adam_coeffs16` returns both values, formed in double from the
# fp32 betas, with these bounds; ``adam_w32`` carries them into the weight. They tell step k from step k + 1 easily:
# at k = 20 ``lr_t`` changes by 1.4 % and ``inv`` by 2.4 % per step, the bounds are 4e-7 and 3e-6.
#
# Moments over several steps with the weights frozen: :func:`moments16`, the recursions ``m' = fma(b1, m, fl(c1 g))`` and
# ``v' = fma(b2, v, fl(c2 fl(g g)))`` with ``g`` known to its radius ``dg``; unlike ``upd32``'s bound the one of ``v`` keeps ``dg^2``: a
# radius here may be as large as the element itself (a gradient that cancels).
BF16_SHAPES = [(784, 10, 32), (784, 10, 64), (40, 16, 24), (776, 16, 40), (264, 10, 48), (1024, 10, 32), (8, 1, 32)]
BF16_MAIN = BF16_SHAPES[:2]
BF16_ONE_STEP = {**F32_ONE_STEP, 40: [(1, 40), (2, 39)], 48: [(1, 48), (2, 33)]}
BF16_STEPS = {**F32_STEPS, 40: [(70, 80), (100, 120), (170, 200)], 48: [(80, 96), (110, 144), (200, 240)]}
BF16_LEARN = {**F32_LEARN, 40: (100, 190)}
BF16_LEARN_SHAPES = [(784, 10, 64), (40, 16, 24), (776, 16, 40)]
# Part (d): ``randn16`` weights at lr 2e-5. bf16 makes the epoch chaotic in places (a relu, a stored activation or
# a shadow weight that rounds the other way moves a tensor by 1e-5 to 1e-2 of its update), and which of those a
# correct implementation meets depends on its accumulation order. At this learning rate and with these bias
# scales one term common to every fp32 implementation dominates the twin's floor of every tensor: the fp32
# rounding of the master row after each update (floors 2e-5 to 4e-4). Case seed 0 of the two wide shapes
# holds a near-tie that the twin itself takes the other way (floor 6e-3, over the cap): seed 1.
BF16_LEARN_SEED = {(784, 10, 64): 1, (776, 16, 40): 1}
BF16_LEARN_HP = {"sgd": dict(kind=1, lr=2e-5, momentum=0.0, wd=0.0, nesterov=False), "sgd_wd": dict(kind=1, lr=2e-5, momentum=0.0, wd=5e-4, nesterov=False)}
BF16_OPT = {"sgd": dict(kind=1, lr=2.0 ** -6, momentum=0.0, wd=0.0, nesterov=False), "sgd_wd": dict(kind=1, lr=2.0 ** -6, momentum=0.0, wd=5e-4, nesterov=False),
            "adam": dict(kind=0, lr=1e-3), "adam_wd": dict(kind=0, lr=1e-3, wd=1e-4)}
BF16_OPT_CASE = ((784, 10, 64), (31, 33))  # part (b): the main shape, both peers a partial batch across the 32-row tile
BF16_EDGE = ((784, 10, 32), (33, 150))  # part (e): 2 steps beside 5
BF16_GANG = (40, 16, 24)  # part (e): 8 peers (4 cases of 2, the seeds below) and 9
BF16_GANG_ROWS, BF16_GANG_SEEDS = (23, 24), (0, 1, 2, 3, 4)
BF16_SEED = {(40, 16, 24, (1, 24)): 1}  # (D0, D3, B, n) -> case seed, where seed 0 misses a cap of test_mlp_ref_cpu.py


def bf16_grid_cases():
    """Every grid case of tests/test_mlp_bf16_epoch_oracle_gpu.py: ``(D0, D3, B, n, seed)``."""
    out = []
    for D0, D3, B in BF16_SHAPES:
        pairs = list(BF16_ONE_STEP[B])
        pairs += BF16_STEPS[B] if (D0, D3, B) in BF16_MAIN else BF16_STEPS[B][1:2]
        out += [(D0, D3, B, n, BF16_SEED.get((D0, D3, B, n), 0)) for n in pairs]
    out.append((*BF16_OPT_CASE[0], BF16_OPT_CASE[1], 0))
    out.append((*BF16_EDGE[0], BF16_EDGE[1], 0))
    out += [(*BF16_GANG, BF16_GANG_ROWS, s) for s in BF16_GANG_SEEDS]
    return list(dict.fromkeys(out))


def forward16(W, X):
    H1 = fc(X, bf16(W["W1"]), W["b1"])
    H2 = fc(H1, bf16(W["W2"]), W["b2"])
    return H1, H2, logits(H2, bf16(W["W3"]), W["b3"])


def grid_ratios16(W, X, D):
    """:func:`grid_ratios` with H1 and H2 rounded to bf16 as the kernel stores them."""
    u = units(D)
    H1, H2, _ = forward16(W, X)
    out = []
    for A, w, b, unit in ((X, W["W1"], W["b1"], u[0]), (H1, W["W2"], W["b2"], u[0] * u[1]), (H2, W["W3"], W["b3"], u[0] * u[1] * u[2])):
        pre = fc_pre(A, w, b)[0]
        assert torch.equal(pre / unit, (pre / unit).round()), "a sum off its grid"
        out.append(float(exactness(A, w, b, unit).max()) if A.shape[0] else 0.0)
    return out


def _isum(lo, hi, Wm):
    """The range of ``sum_n d[r, n] Wm[n, k]`` over ``d`` in ``[lo, hi]``: each end chosen by the sign of the weight."""
    Wp, Wn = Wm.clamp_min(0), Wm.clamp_max(0)
    return lo @ Wp + hi @ Wn, hi @ Wp + lo @ Wn


def _log2_lsb(t):
    return torch.log2(lsb(t))  # +inf for zero


def _iratio(lo, hi, Wm):
    """``sum |term| / unit`` of every element of ``d Wm`` for ``d`` anywhere in ``[lo, hi]``: the sizes from the larger end, the unit
    the finest bit of any term either end can give (the lowest bit of a product is the product of the lowest
    bits). ``[rows, K]``; 0 where there is no term."""
    mag = torch.maximum(lo.abs(), hi.abs()) @ Wm.abs()
    ed = torch.minimum(_log2_lsb(lo), _log2_lsb(hi))
    e = (ed[:, :, None] + _log2_lsb(Wm)[None, :, :]).amin(1)
    unit = torch.where(torch.isfinite(e), torch.exp2(e), torch.ones_like(e))
    return mag / unit


def step16(W, X, y):
    """One step of one peer as the bf16 epoch kernel takes it (section comment): the exact forward, the loss terms, the
    predictions, ``eps_lp`` / ``eps_sm``, and for ``dlog`` ``[rows, D3]``, ``dH2`` and ``dH1`` the central value with the interval
    ``*_lo`` / ``*_hi`` the kernel's own value lies in; ``g``: the six gradients of the central values; ``inexact``: how many
    elements of the two dgrad sums miss the exactness condition."""
    D3 = W["b3"].shape[0]
    rows = X.shape[0]
    W3, W2 = bf16(W["W3"]), bf16(W["W2"])
    H1, H2, z = forward16(W, X)
    loss, pred, sm = head(z, y)
    eps_lp, eps_sm = eps_softmax(z)
    ref = sm.clone()
    ref[torch.arange(rows), y] -= 1.0
    ref = ref / rows
    e = 0.0 if D3 == 1 else eps_sm / rows
    s = dict(X=X, y=y, rows=rows, H1=H1, H2=H2, z=z, loss=loss, pred=pred, eps_lp=eps_lp, eps_sm=eps_sm)
    s["dlog"], s["dlog_lo"], s["dlog_hi"] = bf16(ref), bf16(ref - e), bf16(ref + e)
    m2, m1 = H2 > 0, H1 > 0
    lo, hi = _isum(s["dlog_lo"], s["dlog_hi"], W3)
    s["dH2"], s["dH2_lo"], s["dH2_hi"] = bf16(m2 * (s["dlog"] @ W3)), bf16(m2 * lo), bf16(m2 * hi)
    lo, hi = _isum(s["dH2_lo"], s["dH2_hi"], W2)
    s["dH1"], s["dH1_lo"], s["dH1_hi"] = bf16(m1 * (s["dH2"] @ W2)), bf16(m1 * lo), bf16(m1 * hi)
    s["inexact"] = int((_iratio(s["dlog_lo"], s["dlog_hi"], W3) >= LIM).sum()) + int((_iratio(s["dH2_lo"], s["dH2_hi"], W2) >= LIM).sum())
    pad = torch.zeros(rows, 16, dtype=F64)
    pad[:, :D3] = s["dlog"]
    s["g"] = wgrads(X, H1, H2, s["dH1"], s["dH2"], pad, D3)
    return s


def straddle(s):
    """The fraction of the elements of dlog, dH2 and dH1 whose interval holds more than one value."""
    return {k: float((s[k + "_lo"] != s[k + "_hi"]).double().mean()) for k in ("dlog", "dH2", "dH1")}


def bounds16(s, Bpad):
    """The radius of each of the six gradients of :func:`step16`'s step (section comment, "Gradients")."""
    out = {}
    one = torch.ones(s["rows"], 1, dtype=F64)
    for up, other, kw, kb in (("dlog", s["H2"], "W3", "b3"), ("dH2", s["H1"], "W2", "b2"), ("dH1", s["X"], "W1", "b1")):
        lo, hi = s[up + "_lo"], s[up + "_hi"]
        wid, big = hi - lo, torch.maximum(lo.abs(), hi.abs())
        eu = torch.minimum(_log2_lsb(lo), _log2_lsb(hi)).amin(0)  # the finest bit of each column of the upstream, over the batch
        for k, A in ((kw, other), (kb, one)):
            mag = big.t() @ A.abs()
            e = eu[:, None] + _log2_lsb(A).amin(0)[None, :]
            unit = torch.where(torch.isfinite(e), torch.exp2(e), torch.ones_like(e))
            r = wid.t() @ A.abs() + torch.where(mag / unit < LIM, torch.zeros_like(mag), gamma(Bpad) * mag)
            out[k] = r[:, 0] if k == kb else r
    return out


C1, C2 = 1.0 - R.f32(BETA1), 1.0 - R.f32(BETA2)  # exact in fp32
FLUSH32 = 2.0 ** -125


def adam_coeffs16(hp, k):
    """``(lr_t, inv, relative bound of lr_t, relative bound of inv)`` of ``persist::bias_corr`` at optimizer step ``k`` (from 1):
    the values in double from the fp32 betas, the bounds of the section comment ("Bias correction")."""
    b1, b2 = R.f32(BETA1), R.f32(BETA2)
    r = lambda b: 2 * U * b ** k / (1.0 - b ** k) + U
    return R.f32(hp["lr"]) / (1.0 - b1 ** k), 1.0 / math.sqrt(1.0 - b2 ** k), SECOND * (r(b1) + U), SECOND * (r(b2) / 2 + 3 * U)


def adam_moments16(hp, w, g, dg, m, v, bm, bv):
    """One step of the kernel's ``upd<true>`` moments from ``m``, ``v`` (known to ``bm``, ``bv``) on the gradient ``g`` (known to ``dg``), the
    weight-decay fma included: ``(m', v', bm', bv')``."""
    wd = R.f32(hp.get("wd", 0.0))
    if wd != 0.0:
        g = g + wd * w
        dg = dg + U * g.abs()
    b1, b2 = R.f32(BETA1), R.f32(BETA2)
    m1 = b1 * m + C1 * g
    bm1 = b1 * bm + U * m1.abs() + C1 * (U * g.abs() + dg)
    v1 = b2 * v + C2 * g * g
    top = (g.abs() + dg) ** 2
    bv1 = b2 * bv + U * v1 + C2 * (2 * g.abs() * dg + dg * dg + 2 * U * top) + FLUSH32
    return m1, v1, SECOND * bm1, SECOND * bv1


def moments16(hp, w, gs, rs):
    """The moments after the steps ``gs`` (radii ``rs``) from zero moments with the weights frozen: ``(m, v, bm, bv)``."""
    assert R.f32(hp["lr"]) == 0.0 and hp.get("wd", 0.0) == 0.0
    m, v, bm, bv = (torch.zeros_like(w) for _ in range(4))
    for g, r in zip(gs, rs):
        m, v, bm, bv = adam_moments16(hp, w, g, r, m, v, bm, bv)
    return m, v, bm, bv


def learn_refs16(c, p, hp):
    """Part (d) of the bf16 file: peer ``p``'s float64 epoch with the kernel's bf16 roundings under the pinned order, and the
    fp32 twin's: ``(ref, alt)``."""
    out = []
    for kw in (dict(), dict(mm=mm32_permuted(torch.Generator().manual_seed(p)), f32=True)):
        out.append(epoch(c["W"][p], c["x"][p], c["y"][p], epoch_perm32(c["n"][p], 0, p), c["B"], hp, **kw)[0])
    return out
