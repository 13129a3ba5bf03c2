"""The fused MLP engine's shuffle, gather and bf16 step kernels (``csrc/kernels/mlp_fused.hip``) driven directly
through the ``mlp_debug_*`` entry points with a hand-built ``MLPArgs``, against the float64 oracle of
``tests/_mlp_ref.py``, stage by stage.

BIT-EXACT comparisons:

* the gather: ``Yb`` (labels ``arange(n)``, so it reads back the permutation) equals ``feistel_perm`` under the peer's
  key; ``Xb`` / ``Xb16`` rows are the source rows; rows at or beyond ``n``, inactive peers and every gap keep their
  fill; ``flags_zero`` is zero over exactly ``flags_per_peer`` words per peer; the result does not depend on
  the grid cap or on the destination type;
* ``mlp_sync_shadow``: ``shadow = bf16(params)``, ``w2t = shadow W2`` transposed;
* the ``exact`` family's forward (``tests/test_mlp_ref_cpu.py`` proves ``sum |term| / unit < 2^24`` for fc1, fc2 and fc3
  of every case used here): ``H1``, ``H1T``, ``H2T`` of the valid rows, the correct count, the confusion matrix;
* exact zeros in rows ``[rows, Bpad)`` of every stage tensor and in the ``dlogT`` columns ``>= D3``;
* ``dH2T`` / ``dH1T`` wherever the exactness condition holds on the kernel's own upstream tensors;
* ``m`` of two launches from the same state; everything of a peer without rows (and of every peer at a step
  past its last); the shadow and ``w2t`` against the kernel's own new master.

BOUNDED comparisons (each prints its worst ``|err| / bound``):

* random-normal forward, ``dH2T`` and ``dH1T``: each stored value lies in ``[bf16(ref - e), bf16(ref + e)]``,
  ``e = gamma(K) sum |term|`` from the float64 terms of that element, recomputed from the kernel's own upstream;
* the loss sum and ``dlogT`` at the softmax bounds derived in ``_mlp_ref``'s docstring;
* the six gradients (read out as the momentum of an SGD step from ``m = 0``: ``m_new = g`` exactly) against
  the float64 sums over the kernel's own stage tensors, at ``gamma(Bpad) sum |term|``;
* master, ``m`` and ``v`` after the fused optimizer against ``_fl_ops_ref`` at that module's bounds.

Set-up: 3 peers with valid rows ``[B, odd < B, 0]``, per-peer strides larger than each slab wherever the
layout has a stride (``S``, ``xb_rows``, ``h1_rows``, ``perm_stride``), ``MARK`` in every gap and in every element of
every output, inputs cloned and compared bit for bit after each launch.
"""

import ctypes
import functools

import numpy as np
import pytest
import torch

import _mlp_ref as M

pytestmark = pytest.mark.gpu

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
P = M.P
GAP = 64
MARK = 776.0  # a bf16 value
YMARK = -7
c_int, c_int64, c_float, c_void_p = ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p


class OptParams(ctypes.Structure):
    _fields_ = [("kind", c_int), ("lr", c_float), ("beta1", c_float), ("beta2", c_float), ("eps", c_float), ("weight_decay", c_float),
                ("momentum", c_float), ("nesterov", c_int), ("mu", c_float), ("scaf_upd", c_int)]


class MLPArgs(ctypes.Structure):
    """Mirror of ``csrc/kernels/mlp_fused.h::MLPArgs`` (guarded by ``mlp_debug_args_abi``)."""

    _fields_ = ([(k, c_int) for k in ("P", "D0", "D1", "D2", "D3", "D0pad")]
                + [(k, c_int64) for k in ("S", "numel", "off_w1", "off_b1", "off_w2", "off_b2", "off_w3", "off_b3")]
                + [(k, c_void_p) for k in ("params", "shadow", "w2t", "m", "v", "anchor", "cg", "cl", "Xp", "Yp", "n", "perm")]
                + [("perm_stride", c_int64), ("shuffle_native", c_int), ("seed", c_void_p), ("Xb", c_void_p), ("Xb16", c_void_p), ("Yb", c_void_p),
                   ("xb_rows", c_int64), ("flags_zero", c_void_p), ("flags_per_peer", c_int), ("Xtp", c_void_p), ("Ytp", c_void_p), ("n_t", c_void_p),
                   ("ctl", c_void_p), ("active", c_void_p), ("t0", c_void_p), ("H1", c_void_p), ("h1_rows", c_int)]
                + [(k, c_void_p) for k in ("H1T", "XT", "H2T", "dH2T", "dH1T", "dlogT")]
                + [("B", c_int), ("Bpad", c_int), ("loss_acc", c_void_p), ("correct_acc", c_void_p), ("conf", c_void_p), ("opt", OptParams),
                   ("debug_giveup", c_int), ("f32_ks", c_int), ("f32_variant", c_int)])


@functools.lru_cache(maxsize=None)
def _lib():
    from myfyp_amd.ops import _native

    lib = _native.load(required=True)
    abi = (ctypes.c_longlong * 10)()
    assert lib.mlp_debug_args_abi(abi) == 10
    want = (ctypes.sizeof(MLPArgs), MLPArgs.params.offset, MLPArgs.perm_stride.offset, MLPArgs.flags_per_peer.offset, MLPArgs.ctl.offset,
            MLPArgs.h1_rows.offset, MLPArgs.B.offset, MLPArgs.opt.offset, MLPArgs.f32_variant.offset, ctypes.sizeof(OptParams))
    assert tuple(abi) == want, f"MLPArgs layout mismatch between the test's mirror and the native library: {tuple(abi)} vs {want}"
    assert lib.mlp_debug_args_size() == ctypes.sizeof(MLPArgs)
    return lib


@pytest.fixture(scope="module")
def lib():
    return _lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.view({BF: torch.int16, F32: torch.int32}.get(t.dtype, t.dtype))


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _ptrs(ts):
    return torch.tensor([t.data_ptr() for t in ts], dtype=torch.int64, device="cuda")


def _row(vals, S, dtype):
    """dense [P, n] float64 -> device [P, S], MARK in the tail."""
    out = torch.full((vals.shape[0], S), MARK, dtype=dtype, device="cuda")
    out[:, : vals.shape[1]] = vals.to(dtype).cuda()
    return out


def _flat(n, dtype, fill=MARK):
    return torch.full((n + GAP,), fill, dtype=dtype, device="cuda")


WORST = {}


def _report(name, ratio):
    WORST[name] = max(WORST.get(name, 0.0), ratio)
    print(f"{name}: worst |err| / bound {ratio:.3f}")


def _ratio(err, bound):
    """max err / bound with 0 / 0 = 0 (an exact zero against a zero bound passes, anything else does not)."""
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(r.max()) if r.numel() else 0.0


# ---------------------------------------------------------------------------------------------
# one step's device state
# ---------------------------------------------------------------------------------------------
class Dev:
    """The operands of one case on the device: inputs (with copies to compare against afterwards), optimizer
    state and freshly poisoned outputs."""

    def __init__(self, c, hp=None, m0=None, v0=None, extras=None, evaluate=False):
        self.c = c
        D0, D1, D2, D3 = c["D"]
        self.off, self.numel = M.offsets(c["D"])
        self.S = (self.numel + 63) // 64 * 64 + GAP
        B, Bp = c["B"], c["Bpad"]
        self.xb_rows = (c["step"] + 1) * B + 3
        self.h1_rows = (M.EVAL_CHUNK if evaluate else Bp) + 3
        master = M.pack(c["W"], c["D"])
        self.params = _row(master, self.S, F32)
        self.shadow = _row(M.bf16(master), self.S, BF)
        w2 = M.bf16(c["W"]["W2"]).transpose(1, 2).reshape(P, -1)
        self.w2t = _flat(P * D1 * D2, BF)
        self.w2t[: P * D1 * D2] = w2.reshape(-1).to(BF).cuda()
        zeros = torch.zeros(P, self.numel, dtype=F64)
        self.m = _row(zeros if m0 is None else m0, self.S, F32)
        self.v = _row(zeros if v0 is None else v0, self.S, F32)
        self.extras = {k: _row(t, self.S, F32) for k, t in (extras or {}).items()}
        # the epoch's batches: rows at or beyond n hold pixel 255 and label 0, which no kernel may read
        self.Xb = torch.full((P, self.xb_rows, D0), 255, dtype=torch.uint8, device="cuda")
        self.Yb = torch.zeros(P, self.xb_rows, dtype=torch.int32, device="cuda")
        for p in range(P):
            self.Xb[p, : c["n"][p]] = c["xb"][p].cuda()
            self.Yb[p, : c["n"][p]] = c["yb"][p].to(torch.int32).cuda()
        self.xt = [t.cuda() for t in c["xt"]]
        self.yt = [t.to(torch.int32).cuda() for t in c["yt"]]
        self.xtab, self.ytab = _ptrs(self.xt), _ptrs(self.yt)
        t0 = (hp or {}).get("t0", 0)
        self.ctl = torch.tensor([[c["active"][p], c["n"][p], t0, c["n_test"][p]] for p in range(P)], dtype=torch.int32, device="cuda")
        self.hp = hp or dict(kind=1, lr=2.0 ** -10, momentum=0.9, wd=0.0, nesterov=False)
        self.inputs = dict(Xb=self.Xb, Yb=self.Yb, ctl=self.ctl, xtab=self.xtab, ytab=self.ytab, **{f"xt{p}": t for p, t in enumerate(self.xt)},
                           **{f"yt{p}": t for p, t in enumerate(self.yt)}, **self.extras)
        self.saved = {k: t.clone() for k, t in self.inputs.items()}
        self.state0 = {k: getattr(self, k).clone() for k in ("params", "shadow", "w2t", "m", "v")}
        self.poison()

    def poison(self):
        c = self.c
        D0, D1, D2, D3 = c["D"]
        Bp = c["Bpad"]
        self.H1 = _flat(P * self.h1_rows * D1, BF)
        self.H1T, self.H2T = _flat(P * D1 * Bp, BF), _flat(P * D2 * Bp, BF)
        self.dH1T, self.dH2T, self.dlogT = _flat(P * D1 * Bp, BF), _flat(P * D2 * Bp, BF), _flat(P * 16 * Bp, BF)
        self.loss = torch.tensor([0.0] * P + [MARK] * 2, dtype=F32, device="cuda")
        self.correct = torch.tensor([0] * P + [YMARK] * 2, dtype=torch.int32, device="cuda")
        self.conf_all = torch.ones(256 + P * 256 + 256, dtype=torch.int32, device="cuda")  # slack on both sides

    def args(self, conf=False):
        c, a = self.c, MLPArgs()
        a.P, (a.D0, a.D1, a.D2, a.D3), a.D0pad = P, c["D"], c["D"][0]
        a.S, a.numel = self.S, self.numel
        for k, name in (("off_w1", "W1"), ("off_b1", "b1"), ("off_w2", "W2"), ("off_b2", "b2"), ("off_w3", "W3"), ("off_b3", "b3")):
            setattr(a, k, self.off[name])
        for k in ("params", "shadow", "w2t", "m", "v", "Xb", "Yb", "ctl", "H1", "H1T", "H2T", "dH2T", "dH1T", "dlogT"):
            setattr(a, k, getattr(self, k).data_ptr())
        for k in ("anchor", "cg", "cl"):
            setattr(a, k, self.extras[k].data_ptr() if k in self.extras else None)
        a.xb_rows, a.h1_rows, a.B, a.Bpad = self.xb_rows, self.h1_rows, c["B"], c["Bpad"]
        a.Xtp, a.Ytp = self.xtab.data_ptr(), self.ytab.data_ptr()
        a.loss_acc, a.correct_acc = self.loss.data_ptr(), self.correct.data_ptr()
        a.conf = self.conf_all[256:].data_ptr() if conf else None
        hp, o = self.hp, a.opt
        o.kind, o.lr, o.beta1, o.beta2, o.eps = hp["kind"], hp["lr"], M.BETA1, M.BETA2, M.EPS
        o.weight_decay, o.momentum, o.nesterov, o.mu = hp.get("wd", 0.0), hp.get("momentum", 0.0), int(hp.get("nesterov", False)), hp.get("mu", 0.0)
        o.scaf_upd = int("cg" in self.extras)
        return a

    def intact(self):
        torch.cuda.synchronize()
        for k, t in self.inputs.items():
            assert _same(t, self.saved[k]), f"the launch overwrote its input {k}"

    def host(self):
        """Everything the launches wrote, on the host as float64; the gaps are checked on the way."""
        torch.cuda.synchronize()
        c = self.c
        D0, D1, D2, D3 = c["D"]
        Bp = c["Bpad"]
        h = {}
        for k, d in (("H1T", D1), ("H2T", D2), ("dH1T", D1), ("dH2T", D2), ("dlogT", 16)):
            t = getattr(self, k).cpu()
            assert (t[P * d * Bp:] == MARK).all(), f"the gap behind {k} was written"
            h[k[:-1]] = t[: P * d * Bp].reshape(P, d, Bp).transpose(1, 2).double()  # [P, Bpad, d]
        t = self.H1.cpu()
        assert (t[P * self.h1_rows * D1:] == MARK).all(), "the gap behind H1 was written"
        t = t[: P * self.h1_rows * D1].reshape(P, self.h1_rows, D1).double()
        h["H1rm"] = t
        for k in ("params", "shadow", "m", "v"):
            t = getattr(self, k).cpu()
            assert (t[:, self.numel:] == MARK).all(), f"the gap behind {k} was written"
            h[k] = t[:, : self.numel].double()
        t = self.w2t.cpu()
        assert (t[P * D1 * D2:] == MARK).all(), "the gap behind w2t was written"
        h["w2t"] = t[: P * D1 * D2].reshape(P, D1, D2).double()
        ls, cr = self.loss.cpu(), self.correct.cpu()
        assert (ls[P:] == MARK).all() and (cr[P:] == YMARK).all()
        h["loss"], h["correct"] = ls[:P].double(), cr[:P].tolist()
        ca = self.conf_all.cpu()
        assert (ca[:256] == 1).all() and (ca[256 + P * 256:] == 1).all(), "the confusion matrix was written out of range"
        h["conf"] = ca[256: 256 + P * 256].reshape(P, 16, 16).long() - 1
        return h


def _train(lib, d, step=None):
    a = d.args()
    assert lib.mlp_debug_train_step(ctypes.byref(a), d.c["step"] if step is None else step, _stream()) == 0
    h = d.host()
    d.intact()
    return h


CASES = [(D, B, s, f) for D, B, s in M.TRAIN_CASES for f in M.FAMILIES]
IDS = [M.case_id(c) + "-" + c[3] for c in CASES]


@functools.lru_cache(maxsize=None)
def _run(D, B, s, family):
    """One SGD step (momentum 0.9 from ``m = 0``, lr 2^-10, no weight decay: ``m_new`` is the gradient itself) of the
    case, shared by the tests."""
    c = M.case(D, B, family, s)
    d = Dev(c)
    return c, d, _train(_lib(), d)


def _weights(c, p):
    """Peer ``p``'s operands as the kernels see them: bf16 shadow weights, fp32 biases."""
    return {k: (M.bf16(v[p]) if k[0] == "W" else v[p]) for k, v in c["W"].items()}


def _within(name, got, pre, e, act=None, relu=False):
    """Every stored bf16 ``got`` lies in ``[bf16(f(pre - e)), bf16(f(pre + e))]``, ``f`` the ReLU or the mask ``act > 0``."""
    f = (lambda t: t.clamp_min(0)) if relu else (lambda t: t if act is None else torch.where(act > 0, t, torch.zeros((), dtype=F64)))
    lo, hi, ref = M.bf16(f(pre - e)), M.bf16(f(pre + e)), f(pre)
    bad = (got < lo) | (got > hi)
    _report(name, _ratio((got - ref).abs(), M.ulp_bf16(ref) / 2 + e))
    # MI355X: worst |err| / (ulp / 2 + e) 1.000 (randn H1, dH2), 0.998 (dH1), 0.996 (randn H2): the bf16 rounding itself
    assert not bad.any(), f"{name}: {int(bad.sum())} values outside their interval, first at {bad.nonzero()[0].tolist()}: {got[bad][0]} vs {ref[bad][0]}"
    return int((got != M.bf16(ref)).sum())


def _equal(name, got, ref):
    bad = got != ref
    assert not bad.any(), f"{name}: {int(bad.sum())} elements differ, first at {bad.nonzero()[0].tolist()}: {got[bad][0]} vs {ref[bad][0]}"


# ---------------------------------------------------------------------------------------------
# forward, loss, dlogits
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,B,s,family", CASES, ids=IDS)
def test_forward(D, B, s, family):
    """``exact``: H1, H1T, H2T of the valid rows and the correct count bit for bit from the inputs. ``randn``: H1 from the
    inputs and H2 from the kernel's own H1 inside ``[bf16(ref - e), bf16(ref + e)]``, ``e = gamma(K + 4) sum |term|``. Both: exact
    zeros in rows ``[rows, Bpad)``, ``H1T = H1`` transposed, a peer without rows writes nothing."""
    c, d, k = _run(D, B, s, family)
    Bp = c["Bpad"]
    for p in range(P):
        rows = c["rows"][p]
        if rows == 0:
            for name in ("H1", "H2", "dH1", "dH2", "dlog"):
                assert (k[name][p] == MARK).all(), f"{name}: written for a peer without rows"
            assert (k["H1rm"][p] == MARK).all() and k["loss"][p] == 0 and k["correct"][p] == 0
            continue
        W = _weights(c, p)
        assert (k["H1rm"][p, Bp:] == MARK).all(), "H1 rows beyond Bpad were written"
        _equal("H1T vs H1", k["H1"][p], k["H1rm"][p, :Bp])
        for name in ("H1", "H2", "dH1", "dH2", "dlog"):
            assert not k[name][p, rows:].any(), f"{name}: rows of invalid samples are not exact zeros"
        r = M.step(c, p)
        if family == "exact":
            _equal(f"H1[{p}]", k["H1"][p, :rows], r["H1"])
            _equal(f"H2[{p}]", k["H2"][p, :rows], r["H2"])
            assert k["correct"][p] == int((r["pred"] == r["y"]).sum())
        else:
            pre, mag = M.fc_pre(r["X"], W["W1"], W["b1"])
            n1 = _within(f"randn H1[{p}]", k["H1"][p, :rows], pre, M.gamma(D[0] + 4) * mag, relu=True)
            pre, mag = M.fc_pre(k["H1"][p, :rows], W["W2"], W["b2"])
            n2 = _within(f"randn H2[{p}]", k["H2"][p, :rows], pre, M.gamma(D[1] + 4) * mag, relu=True)
            print(f"values off the oracle's own rounding: H1 {n1}, H2 {n2}")
            z = M.logits(k["H2"][p, :rows], W["W3"], W["b3"])
            _, pred, _ = M.head(z, r["y"])
            top2 = z.topk(min(2, D[3]), 1)[0]
            clear = torch.ones(rows, dtype=torch.bool) if D[3] == 1 else (top2[:, 0] - top2[:, 1]) > 2 * M.gamma(D[2] + 4) * M.fc_pre(k["H2"][p, :rows], W["W3"], W["b3"])[1].amax(1)
            lo, hi = int(((pred == r["y"]) & clear).sum()), int(((pred == r["y"]) | ~clear).sum())
            assert lo <= k["correct"][p] <= hi


@pytest.mark.parametrize("D,B,s,family", CASES, ids=IDS)
def test_loss_and_dlogits(D, B, s, family):
    """From the kernel's own H2: the loss sum at ``rows * eps_lp`` plus the fp32 summation, ``dlogT`` at one bf16 ulp plus
    ``eps_sm / rows`` (``_mlp_ref``'s docstring derives both); exact zeros in the columns ``>= D3``. Controls: a row dropped from
    the loss, ``1 / Bpad`` or ``1 / (rows - 1)`` in place of ``1 / rows``."""
    c, d, k = _run(D, B, s, family)
    for p in range(2):
        rows, Bp = c["rows"][p], c["Bpad"]
        W = _weights(c, p)
        H2 = k["H2"][p, :rows]
        y = M.batch(c, p)[1]
        z, zmag = M.fc_pre(H2, W["W3"], W["b3"])
        e_z = 0.0 if family == "exact" else float((M.gamma(D[2] + 4) * zmag).max())
        if family == "exact":
            assert float(M.exactness(H2, W["W3"], W["b3"], float(np.prod(M.units(D)))).max()) < M.LIM
        eps_lp, eps_sm = M.eps_softmax(z, e_z)
        loss = M.head(z, y)[0]
        bound = rows * eps_lp + M.gamma(10 + Bp // 16) * float(loss.abs().sum())
        err = abs(float(k["loss"][p]) - float(loss.sum()))
        _report(f"loss[{p}]", err / bound)
        assert err <= bound  # MI355X: worst |err| / bound 0.126
        if rows > 1 and float(loss[-1]) > 4 * bound:
            assert abs(float(k["loss"][p]) - float(loss[:-1].sum())) > bound, "the loss without its last row passes too"
        ref = M.dlogits(z, y, rnd=M.ident)
        got = k["dlog"][p, :rows]
        assert not got[:, D[3]:].any(), "dlogits columns >= D3 are not exact zeros"
        bnd = M.ulp_bf16(ref) + eps_sm / rows
        _report(f"dlogits[{p}]", _ratio((got - ref).abs(), bnd))
        assert ((got - ref).abs() <= bnd).all()  # MI355X: worst |err| / bound 0.500 (the bf16 rounding itself)
        if D[3] > 1:
            for label, wrong in (("1 / Bpad", rows / Bp), ("1 / (rows - 1)", rows / max(1, rows - 1))):
                if wrong != 1.0 and rows <= 64:  # beyond that 1 / (rows - 1) is within a bf16 ulp of 1 / rows
                    assert ((got - ref * wrong).abs() > bnd).any(), f"dlogits scaled by {label} passes too"


# ---------------------------------------------------------------------------------------------
# dH2, dH1 from the kernel's own upstream
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,B,s,family", CASES, ids=IDS)
def test_dgrads_from_the_kernels_own_upstream(D, B, s, family):
    """``dH2 = bf16(dlog W3s * [H2 > 0])`` from the kernel's dlogT and H2T, ``dH1 = bf16(dH2 W2s * [H1 > 0])`` from its dH2T and
    H1: inside ``[bf16(ref - e), bf16(ref + e)]`` (``e = gamma(32) sum |term|`` and ``gamma(D2) sum |term|``), bit-equal where the
    exactness condition holds on those inputs. Controls: the mask of every unit on, the masks of the rows
    rolled by one, one class / one unit dropped from the sum."""
    c, d, k = _run(D, B, s, family)
    for p in range(2):
        rows = c["rows"][p]
        W = _weights(c, p)
        H1, H2, dl, dH2, dH1 = (k[n][p, :rows] for n in ("H1", "H2", "dlog", "dH2", "dH1"))
        for name, up, w, act, got, K in (("dH2", dl[:, : D[3]], W["W3"], H2, dH2, 32), ("dH1", dH2, W["W2"], H1, dH1, D[2])):
            pre, mag = up @ w, M.dgrad_mag(up, w)
            _within(f"{name}[{p}]", got, pre, M.gamma(K) * mag, act=act)
            exact = M.exactness(up, w.t().contiguous()) < M.LIM
            ref = M.dgrad(up, w, act)
            bad = exact & (got != ref)
            print(f"{name}[{p}]: exactness holds on {float(exact.double().mean()):.2f} of the elements")
            assert not bad.any(), f"{name}: {int(bad.sum())} elements with exact sums differ"
            if not ref.any():
                continue  # D3 = 1: the softmax of one class has no gradient
            e = M.gamma(K) * mag
            outside = lambda alt: bool(((got < M.bf16(alt - e)) | (got > M.bf16(alt + e))).any())
            live = torch.ones_like(act)
            assert outside(M.dgrad(up, w, live, M.ident)), f"{name}: every unit live passes too"
            if rows > 1:
                assert outside(M.dgrad(up, w, act.roll(1, 0), M.ident)), f"{name}: the masks of another row pass too"
            j = int(up.abs().sum(0).argmax())
            up2 = up.clone()
            up2[:, j] = 0
            assert outside(M.dgrad(up2, w, act, M.ident)), f"{name}: one term dropped from the sum passes too"


# ---------------------------------------------------------------------------------------------
# gradients
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,B,s,family", CASES, ids=IDS)
def test_gradients(D, B, s, family):
    """``m`` after one SGD step from ``m = 0`` (momentum 0.9: ``m_new = 0.9 * 0 + g`` exactly) against the float64 sums over the
    kernel's own dH1T / dH2T / dlogT / H1T / H2T and the uint8 batch, at ``gamma(Bpad) sum |term|`` per element. Control: the
    last valid row dropped from the sums fails. The peer without rows: m, v, params, shadow, w2t untouched."""
    c, d, k = _run(D, B, s, family)
    for p in range(2):
        rows = c["rows"][p]
        X = M.batch(c, p)[0]
        st = [k[n][p, :rows] for n in ("H1", "H2", "dH1", "dH2", "dlog")]
        g64, mag = M.wgrads(X, *st, D[3]), M.wgrad_mags(X, *st, D[3])
        got = M.unpack(k["m"][p], D)
        for name in M.NAMES:
            bound = M.gamma(c["Bpad"]) * mag[name]
            err = (got[name] - g64[name]).abs()
            _report(f"d{name}[{p}]", _ratio(err, bound))
            # MI355X: worst |err| / bound 0.126 (dW3), 0.053 (dW2), 0.042 (dW1), below 0.01 for the biases
            assert (err <= bound).all(), f"d{name}: {float(err.max()):.3e}"
        if rows > 1:
            short = M.wgrads(X[:-1], *[t[:-1] for t in st], D[3])
            for name in ("W1", "b1", "W2", "b2", "W3", "b3"):
                if g64[name].any() and (short[name] != g64[name]).any():
                    assert ((got[name] - short[name]).abs() > M.gamma(c["Bpad"]) * mag[name]).any(), f"d{name} without the last row passes too"
        assert not k["v"][p].any(), "SGD wrote v"
    for name in ("params", "shadow", "m", "v"):
        assert _same(getattr(d, name)[2], d.state0[name][2]), f"the peer without rows: {name} was written"
    n2 = D[1] * D[2]
    assert _same(d.w2t[2 * n2: 3 * n2], d.state0["w2t"][2 * n2: 3 * n2])
    # shadow and w2t: bf16 of the kernel's own new master
    for p in range(2):
        _equal("shadow", k["shadow"][p], M.bf16(k["params"][p]))
        _equal("w2t", k["w2t"][p], M.unpack(k["shadow"][p], D)["W2"].t())
        if g64["W2"].any():
            assert (k["params"][p] != d.state0["params"][p, : d.numel].cpu().double()).any()


@pytest.mark.parametrize("D,B,s,family", [CASES[1], CASES[4], CASES[11], CASES[14]], ids=[IDS[1], IDS[4], IDS[11], IDS[14]])
def test_second_launch_and_step_past_the_end(lib, D, B, s, family):
    """Two launches from the same state give bit-identical m, params, shadow and stage tensors (no atomics in the
    gradients); a launch at a step past every peer's last writes nothing at all."""
    c, d, k = _run(D, B, s, family)
    d2 = Dev(c)
    k2 = _train(lib, d2)
    for name in ("m", "params", "shadow", "w2t", "H1", "H2", "dH1", "dH2", "dlog"):
        assert torch.equal(k[name], k2[name]), name
    assert k2["correct"] == k["correct"]
    before = {n: getattr(d2, n).clone() for n in ("params", "shadow", "w2t", "m", "v")}
    d2.poison()
    k3 = _train(lib, d2, step=c["step"] + 1)
    for n, t in before.items():
        assert _same(getattr(d2, n), t), f"a step past the last wrote {n}"
    for name in ("H1", "H2", "dH1", "dH2", "dlog", "H1rm"):
        assert (k3[name] == MARK).all(), name
    assert not k3["loss"].any() and k3["correct"] == [0] * P


# ---------------------------------------------------------------------------------------------
# fused optimizer
# ---------------------------------------------------------------------------------------------
OPT_CASES = [CASES[1], CASES[5], CASES[15]]  # 784-256-128-10 B 40, 40-256-256-16 B 32 step 1, 8-256-128-16 B 256 (randn)


@pytest.mark.parametrize("D,B,s,family", OPT_CASES, ids=[IDS[1], IDS[5], IDS[15]])
@pytest.mark.parametrize("variant", list(M.OPT_VARIANTS))
def test_fused_optimizer(lib, D, B, s, family, variant):
    """From the gradient read out by the SGD launch: params, m and v after a launch with random optimizer state against
    ``_fl_ops_ref.sgd_step`` / ``adam_step`` at that module's bounds (``units * u / (1 - 32 u)``). Bit-exact: the shadow and w2t
    are bf16 of the kernel's own new master; the peer without rows is untouched. Control: half the gradient fails."""
    c, d0, k0 = _run(D, B, s, family)
    hp = M.OPT_VARIANTS[variant]
    g = torch.Generator().manual_seed(len(variant) + D[0] + B)
    n = d0.numel
    rnd = lambda sc: (torch.randn(P, n, generator=g) * sc).double()
    m0, v0 = rnd(0.01), rnd(0.01) ** 2
    extras = {}
    if "mu" in hp:
        extras["anchor"] = (M.pack(c["W"], D) + rnd(0.05)).float().double()
    if hp.get("scaffold"):
        extras["cg"], extras["cl"] = rnd(0.01), rnd(0.01)
    d = Dev(c, hp=hp, m0=m0, v0=v0, extras=extras)
    k = _train(lib, d)
    w0 = d.state0["params"][:, :n].cpu().double()
    m0, v0 = d.state0["m"][:, :n].cpu().double(), d.state0["v"][:, :n].cpu().double()
    ex = {kk: t[:, :n].cpu().double() for kk, t in d.extras.items()}
    scale = M.U / (1.0 - 32 * M.U)
    for p in range(2):
        grad = k0["m"][p]
        E = {kk: t[p].numpy() for kk, t in ex.items()}
        w1, m1, v1, uw, um, uv = M.opt_step(hp, w0[p].numpy(), grad.numpy(), m0[p].numpy(), v0[p].numpy(), c["step"], E.get("anchor"), E.get("cg"), E.get("cl"))
        wl = M.opt_step(hp, w0[p].numpy(), 0.5 * grad.numpy(), m0[p].numpy(), v0[p].numpy(), c["step"], E.get("anchor"), E.get("cg"), E.get("cl"))[0]
        for name, got, want, units in (("params", k["params"][p], w1, uw), ("m", k["m"][p], m1, um), ("v", k["v"][p], v1, uv)):
            if want is None:
                assert _same(getattr(d, name)[p], d.state0[name][p]), f"{variant} wrote {name}"
                continue
            err = (got - torch.from_numpy(want)).abs()
            bound = torch.from_numpy(np.asarray(units)) * scale
            _report(f"{variant} {name}[{p}]", _ratio(err, bound))
            # MI355X: params 0.999 (sgd), 0.993 (nesterov_wd), 0.992 (fedprox), 0.991 (adam_t7), 0.987 (adam_t0), 0.963 (scaffold): the
            # rounding of the new master itself; m at most 0.632, v 0.717. With the bias corrections formed in float
            # (1 - __powf(beta, t)) adam_t0 at t = 2 missed the params bound by a factor 4.17
            assert (err <= bound).all(), f"{variant} {name}: {float((err / bound).max()):.2f} bounds"
        assert ((k["params"][p] - torch.from_numpy(wl)).abs() > torch.from_numpy(uw) * scale).any(), "half the gradient passes too"
        _equal("shadow", k["shadow"][p], M.bf16(k["params"][p]))
        _equal("w2t", k["w2t"][p], M.unpack(k["shadow"][p], D)["W2"].t())
    for name in ("params", "shadow", "m", "v"):
        assert _same(getattr(d, name)[2], d.state0[name][2]), f"the peer without rows: {name} was written"


# ---------------------------------------------------------------------------------------------
# evaluation
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,family,n_test,active", M.EVAL_CASES, ids=[f"{c[0][0]}-{c[1]}" for c in M.EVAL_CASES])
def test_evaluation(lib, D, family, n_test, active):
    """``mlp_debug_eval_chunk`` at base 0 and 512, n_test of 70, 512 and 517, a confusion buffer pre-filled with ones.
    Bit-exact: the correct count and the confusion matrix (ties go to the lowest index), nothing outside
    ``[p][16][16]``, no training tensor, parameter or optimizer state written. Bounded: the loss."""
    c = M.case(D, 32, family, n_test=n_test, active=active)
    d = Dev(c, evaluate=True)
    a = d.args(conf=True)
    want_conf = torch.zeros(P, 16, 16, dtype=torch.int64)
    for base in (0, 512):
        d.loss[:P] = 0
        d.correct[:P] = 0
        assert lib.mlp_debug_eval_chunk(ctypes.byref(a), base, _stream()) == 0
        k = d.host()
        d.intact()
        for p in range(P):
            loss, correct, conf, z = M.eval_chunk(c, p, base)
            want_conf[p] += conf
            assert k["correct"][p] == correct, (p, base)
            rows = z.shape[0]
            eps_lp, _ = M.eps_softmax(z)
            bound = rows * eps_lp + M.gamma(10 + 32) * float(loss.abs().sum())
            err = abs(float(k["loss"][p]) - float(loss.sum()))
            if rows:
                _report(f"eval loss[{p}] base {base}", err / bound)
            assert err <= bound  # MI355X: worst |err| / bound 0.053
        assert torch.equal(k["conf"], want_conf), f"confusion matrix after base {base}"
        for name in ("H1", "H2", "dH1", "dH2", "dlog"):
            assert (k[name] == MARK).all(), f"evaluation wrote {name}T"
    assert int(want_conf.sum()) == sum(n for n, act in zip(n_test, active) if act)
    for name in ("params", "shadow", "w2t", "m", "v"):
        assert _same(getattr(d, name), d.state0[name]), f"evaluation wrote {name}"


# ---------------------------------------------------------------------------------------------
# shadow refresh
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [(40, 64, 64, 10), (1032, 512, 256, 10)], ids=["2k", "660k"])
def test_sync_shadow(lib, D):
    """``shadow = bf16(params)`` over ``numel`` elements per peer (660k: more than the capped grid covers in one pass) and
    ``w2t = shadow W2`` transposed, bit for bit; the gaps keep their fill; params untouched."""
    c = M.case(D, 32, "randn")
    d = Dev(c)
    d.shadow.fill_(MARK)
    d.w2t.fill_(MARK)
    a = d.args()
    assert lib.mlp_debug_sync_shadow(ctypes.byref(a), _stream()) == 0
    k = d.host()
    d.intact()
    assert _same(d.params, d.state0["params"])
    _equal("shadow", k["shadow"], M.bf16(k["params"]))
    for p in range(P):
        _equal("w2t", k["w2t"][p], M.unpack(k["shadow"][p], D)["W2"].t())
    assert (k["shadow"] != MARK).any()


# ---------------------------------------------------------------------------------------------
# gather and shuffle
# ---------------------------------------------------------------------------------------------
XMARK = 0xAB
SEEDS = (0x0123456789ABCDEF, 0xF00DFACE5EED0001)
# (n per peer, active, D0): every n of {1, 2, 3, 4, 5, 16, 17, 64, 100, 255, 256, 257, 1000, 4097} and every D0 of {8, 40, 784, 1032, 2048}
GATHER_CASES = [
    ((1, 2, 3), (1, 1, 1), 8),
    ((4, 5, 16), (1, 1, 1), 40),
    ((17, 64, 100), (1, 0, 1), 784),
    ((255, 256, 257), (1, 1, 1), 1032),
    ((1000, 4097, 64), (1, 1, 1), 2048),
    ((100, 1000, 17), (1, 1, 0), 8),
]


class GatherDev:
    def __init__(self, n, active, D0, seed_of_data=0):
        g = torch.Generator().manual_seed(D0 + sum(n) + seed_of_data)
        self.n, self.active, self.D0 = n, active, D0
        self.xs = [torch.randint(0, 256, (k, D0), generator=g).to(torch.uint8).cuda() for k in n]
        self.ys = [torch.arange(k, dtype=torch.int32).cuda() for k in n]
        self.xtab, self.ytab = _ptrs(self.xs), _ptrs(self.ys)
        self.ctl = torch.tensor([[active[p], n[p], 0, 0] for p in range(P)], dtype=torch.int32, device="cuda")
        self.seed = torch.zeros(2, dtype=torch.int64, device="cuda")
        self.stride = max(n) + 5
        self.perm = torch.zeros(P, self.stride, dtype=torch.int32, device="cuda")
        self.inputs = dict(xtab=self.xtab, ytab=self.ytab, ctl=self.ctl, seed=self.seed, perm=self.perm, **{f"x{p}": t for p, t in enumerate(self.xs)},
                           **{f"y{p}": t for p, t in enumerate(self.ys)})

    def launch(self, lib, order, xb_rows, bf, fpp, max_wgs):
        """One gather into fresh outputs. Returns ``(X [P, xb_rows, D0], Y [P, xb_rows])`` on the device, gaps checked."""
        D0 = self.D0
        native = isinstance(order, int)
        if native:
            self.seed[0] = order - (1 << 64) if order >= 1 << 63 else order
        else:
            self.perm.fill_(0)  # the gap holds an in-range row: a stray read stays inside the dataset
            for p in range(P):
                self.perm[p, : self.n[p]] = torch.as_tensor(order[p], dtype=torch.int32).cuda()
        saved = {k: t.clone() for k, t in self.inputs.items()}
        X = _flat(P * xb_rows * D0, BF) if bf else _flat(P * xb_rows * D0, torch.uint8, XMARK)
        Y = _flat(P * xb_rows, torch.int32, YMARK)
        flags = _flat(P * fpp, torch.int32, YMARK) if fpp else None
        a = MLPArgs()
        a.P, a.D0, a.D0pad = P, D0, D0
        a.Xp, a.Yp, a.ctl, a.perm, a.perm_stride = self.xtab.data_ptr(), self.ytab.data_ptr(), self.ctl.data_ptr(), self.perm.data_ptr(), self.stride
        a.shuffle_native, a.seed = int(native), self.seed.data_ptr()
        a.Xb, a.Xb16, a.Yb, a.xb_rows = (None if bf else X.data_ptr()), (X.data_ptr() if bf else None), Y.data_ptr(), xb_rows
        a.flags_zero, a.flags_per_peer = (flags.data_ptr() if fpp else None), fpp
        assert lib.mlp_debug_gather_epoch(ctypes.byref(a), max_wgs, _stream()) == 0
        torch.cuda.synchronize()
        for k, t in self.inputs.items():
            assert _same(t, saved[k]), f"the gather overwrote its input {k}"
        assert (X[P * xb_rows * D0:] == (MARK if bf else XMARK)).all() and (Y[P * xb_rows:] == YMARK).all(), "the gap behind Xb / Yb was written"
        if fpp:
            assert not flags[: P * fpp].any(), "flags_zero: a word of a peer's flag block is not zero"
            assert (flags[P * fpp:] == YMARK).all(), "flags_zero: the gap behind the flag block was written"
        return X[: P * xb_rows * D0].reshape(P, xb_rows, D0), Y[: P * xb_rows].reshape(P, xb_rows)

    def check(self, X, Y, order, xb_rows, bf):
        """Against the oracle's permutation, bit for bit (the rows are compared on the device)."""
        fill = MARK if bf else XMARK
        for p in range(P):
            rows = min(self.n[p], xb_rows) if self.active[p] else 0
            assert (X[p, rows:] == fill).all() and (Y[p, rows:] == YMARK).all(), f"peer {p}: rows at or beyond n (or of an inactive peer) were written"
            if rows == 0:
                continue
            perm = M.epoch_perm(self.n[p], order, p) if isinstance(order, int) else np.asarray(order[p])
            assert sorted(perm.tolist()) == list(range(self.n[p]))
            assert Y[p, :rows].cpu().tolist() == perm[:rows].tolist(), f"peer {p}: Yb is not the oracle's permutation"
            src = self.xs[p][torch.as_tensor(perm[:rows], dtype=torch.int64).cuda()]
            assert torch.equal(X[p, :rows], src.to(BF) if bf else src), f"peer {p}: a gathered row differs from its source row"


@pytest.mark.parametrize("n,active,D0", GATHER_CASES, ids=["-".join(map(str, c[0])) + f"-D{c[2]}" for c in GATHER_CASES])
def test_gather_and_shuffle(lib, n, active, D0):
    """Both destinations (uint8 ``Xb``, bf16 ``Xb16`` with the flag block), two seeds, ``xb_rows`` beyond the largest ``n`` and
    ``xb_rows = 50``, the full grid and the grid capped at one workgroup per peer (every row block from the stride
    loop), and pinned permutations with ``perm_stride > n``. ``Yb[:n]`` is the oracle's ``feistel_perm`` (so a permutation),
    the rows are the source rows, everything else keeps its fill, and the cap changes nothing."""
    d = GatherDev(n, active, D0)
    g = torch.Generator().manual_seed(5)
    pinned = [torch.randperm(k, generator=g).numpy() for k in n]
    for bf, fpp in ((False, 0), (True, 37), (True, 300)):
        for order in (*SEEDS, pinned):
            for xb_rows in (max(n) + 3, 50):
                full = None
                for max_wgs in (0, P):
                    X, Y = d.launch(lib, order, xb_rows, bf, fpp, max_wgs)
                    d.check(X, Y, order, xb_rows, bf)
                    if full is not None:
                        assert torch.equal(_bits(X), _bits(full[0])) and torch.equal(Y, full[1]), "the capped grid gathers something else"
                    full = (X, Y)
    # the seeds and the peers give different orders (n >= 16: two orders of a handful of rows may coincide)
    for p in range(P):
        if n[p] >= 16:
            assert M.epoch_perm(n[p], SEEDS[0], p).tolist() != M.epoch_perm(n[p], SEEDS[1], p).tolist()
            assert M.epoch_perm(n[p], SEEDS[0], p).tolist() != M.epoch_perm(n[p], SEEDS[0], (p + 1) % P).tolist()


def test_gather_controls(lib):
    """The comparison above fails for the key of another peer, for the seed itself in place of the peer's key and for
    another epoch's seed."""
    n, active, D0 = (255, 256, 257), (1, 1, 1), 40
    d = GatherDev(n, active, D0)
    X, Y = d.launch(lib, SEEDS[0], 260, False, 0, 0)
    d.check(X, Y, SEEDS[0], 260, False)
    for label, wrong in (("another peer's key", [M.epoch_perm(n[p], SEEDS[0], p + 1) for p in range(P)]),
                         ("the bare seed", [M.feistel_perm_np(n[p], SEEDS[0]) for p in range(P)]),
                         ("another epoch's seed", [M.epoch_perm(n[p], SEEDS[1], p) for p in range(P)])):
        with pytest.raises(AssertionError):
            d.check(X, Y, wrong, 260, False)
