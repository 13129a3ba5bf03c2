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


def sgd_epoch(W, x, y, perm, B, lr, rnd=bf16, mm=mm64, f32=False):
    """``W``: one peer's ``{name: float64}`` master values, ``x`` ``[n, D0]``, ``y`` ``[n]``, ``perm`` the epoch order. One pass in
    batches of ``B`` (the last one partial), ``w -= fp32(lr) * g`` after each; the bf16 roundings of :func:`step` and no
    other. Returns the new master values.

    ``f32`` (with ``mm = mm32_permuted(g)``): everything the kernels hold in fp32 is fp32 here too: every sum (the
    products, the bias gradients, the softmax) accumulated in fp32, in another order where ``mm`` does it, and the
    master row rounded to fp32 after each update. Against the float64 run this measures the oracle's own
    sensitivity: the floor below which two correct fp32 implementations of the epoch cannot be told apart."""
    W = {k: v.clone() for k, v in W.items()}
    D3 = W["b3"].shape[0]
    lr = R.f32(lr)
    zero = torch.zeros((), dtype=F64)
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
            W[k] = (W[k].float() - torch.tensor(lr, dtype=F32) * g[k].float()).double() if f32 else W[k] - lr * g[k]
    return W


def rel_update(got, ref, start):
    """``|(got - start) - (ref - start)| / |ref - start|`` in the 2-norm: the relative update error of one tensor."""
    return float(((got - start) - (ref - start)).norm() / ((ref - start).norm() + 1e-300))
