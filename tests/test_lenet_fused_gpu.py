"""``lenet_fused_step`` (``csrc/kernels/lenet_fused.hip``: ``k_lenet_step<2>`` + ``k_lenet_fc_grad<2>``) driven
directly with a hand-built ``LenetArgs`` against the float64 oracle of ``tests/_lenet_ref.py``, stage by stage.

BIT-EXACT comparisons (``tests/test_lenet_ref_cpu.py`` proves ``sum |term| / unit < 2^24 / 16`` for every
exact case used here, so every partial sum in any order is exact in fp32 and one RNE rounding to bf16
decides the stored value):

* forward: the ``p2 | z3 | z4`` columns of ``act`` for the valid rows; ``nb``; the correct count; the
  confusion matrix (evaluation);
* ``dz4`` and ``dz3``: each recomputed by the oracle from what the kernel itself exported upstream
  (``dl``, then ``dz4``), after asserting the stage's exactness condition on those very inputs;
* exact zeros: ``dl | dz4 | dz3`` of invalid rows, ``dl`` columns >= 10, gradients of the peer without
  samples, the ``part`` records of workgroups without a valid image;
* ``gf`` / ``g`` of the conv layers = the sequential fp32 sum of the workgroups' ``part`` records;
* determinism of ``gf | g | act`` over two launches; the shadow = ``bf16(`` the kernel's own new master ``)``.

BOUNDED comparisons (worst measured ``|err| / bound`` next to each assertion):

* the loss sum: ``2^-18 * (1 + max|z|)`` per valid row, as ``test_cnn_ops_gpu.test_xent``;
* ``dlogits``: ``bf16_bound(ref, 1 / valid)`` (one bf16 ulp + 2^-20 / valid);
* fc weight / bias gradients: the float64 sums over the kernel's exported ``act`` block, at ``fp32_bound``
  against the fp32 evaluation of the same sums;
* conv weight / bias gradients: the oracle's backward from the kernel's exported ``dz3`` (dp2, dz2, dp1,
  dz1 are exact on those inputs, asserted), at ``fp32_bound`` for the dW1, dW2, db1, db2 sums;
* master rows and momentum after the fused optimizer: ``sgd_update`` in float64 at ``fp32_bound``.

The kernel exports neither p1 nor dz2 / dp1 / dz1; they are pinned through the quantities above (one
wrong element of any of them moves a gradient sum by far more than ``fp32_bound``: the tie-rule
control shows it).

Set-up: 3 peers, per-peer strides larger than each slab, ``MARK`` in every gap and in every element
of ``gf | g | part | act`` (the kernel must leave alone what it has no business writing), valid = [B, odd, 0].
"""

import ctypes
import functools

import pytest
import torch

import _cnn_ops_ref as O
import _conv_ref as C
import _lenet_ref as L

pytestmark = pytest.mark.gpu

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
P = L.P
GAP = 64
MARK = 776.0  # a bf16 value
LAY = L.LAY
EXACT = [(B, f) for B, f in L.CASES if f != "randn"]


@pytest.fixture(scope="module")
def lib():
    from myfyp_amd.parallel.cnn_engine import _lib

    return _lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.view({BF: torch.int16, F32: torch.int32}.get(t.dtype, t.dtype))


@functools.lru_cache(maxsize=None)
def _host(B, family, train=True):
    c = L.case(B, family, train)
    return c, L.oracle(c)


def _buf(vals, dtype):
    """dense [P, n] float64 -> device [P, n + GAP], MARK in the gap."""
    out = torch.full((vals.shape[0], vals.shape[1] + GAP), MARK, dtype=dtype, device="cuda")
    out[:, : vals.shape[1]] = vals.to(dtype).cuda()
    return out


class Dev:
    """The device operands of one case (inputs, with copies to compare against afterwards)."""

    def __init__(self, c):
        self.c, B = c, c["B"]
        self.xs = [x.cuda() for x in c["xs"]]
        self.ys = [y.cuda() for y in c["ys"]]
        self.xtab = torch.tensor([t.data_ptr() for t in self.xs], dtype=torch.int64, device="cuda")
        self.ytab = torch.tensor([t.data_ptr() for t in self.ys], dtype=torch.int64, device="cuda")
        self.n = torch.tensor(c["n"], dtype=torch.int32, device="cuda")
        self.perm = None
        if c["perm"] is not None:  # the gap holds in-range rows too (poisoned ones): a stray read stays inside the dataset
            self.perm = torch.cat([c["perm"], c["perm"][:, :1].expand(-1, GAP)], 1).to(torch.int32).cuda()
        self.shadow = _buf(L.pack_wf(L.to_wf(c["W"]), fill=MARK), BF)
        self.params = _buf(L.pack_params(c["W"], c["b"], fill=MARK), F32)
        self.inputs = dict(shadow=self.shadow, params=self.params, n=self.n, **{f"x{p}": t for p, t in enumerate(self.xs)},
                           **{f"y{p}": t for p, t in enumerate(self.ys)})
        if self.perm is not None:
            self.inputs["perm"] = self.perm
        self.saved = {k: t.clone() for k, t in self.inputs.items()}

    def intact(self, skip=()):
        torch.cuda.synchronize()
        for k, t in self.inputs.items():
            if k not in skip:
                assert torch.equal(_bits(t), _bits(self.saved[k])), f"the launch overwrote its input {k}"


class Out:
    """Freshly poisoned outputs."""

    def __init__(self, B):
        f = lambda n, dt: torch.full((P, n + GAP), MARK, dtype=dt, device="cuda")
        self.B = B
        self.gf, self.g = f(LAY["shadow_n"], F32), f(LAY["params_n"], F32)
        self.act, self.part = f(B * L.A_W, BF), f((B // 2) * L.PR_N, F32)
        self.stats = torch.tensor([0.0, 0.0, MARK, MARK] * P + [MARK] * 4, dtype=F32, device="cuda")
        self.nb = torch.full((P + 2,), -5, dtype=torch.int32, device="cuda")
        self.conf_all = torch.ones(256 + P * 256 + 256, dtype=torch.int32, device="cuda")  # slack on both sides
        self.conf = self.conf_all[256: 256 + P * 256]

    def host(self):
        torch.cuda.synchronize()
        B = self.B
        h = {}
        for k, n in (("gf", LAY["shadow_n"]), ("g", LAY["params_n"]), ("act", B * L.A_W), ("part", (B // 2) * L.PR_N)):
            t = getattr(self, k).cpu()
            assert (t[:, n:] == MARK).all(), f"the gap behind {k} was written"
            h[k] = t[:, :n]
        h["act"] = h["act"].reshape(P, B, L.A_W)
        h["part"] = h["part"].reshape(P, B // 2, L.PR_N)
        st = self.stats.cpu()
        assert (st[4 * P:] == MARK).all() and (st[: 4 * P].reshape(P, 4)[:, 2:] == MARK).all(), "stats slots 2, 3 were written"
        h["stats"] = st[: 4 * P].reshape(P, 4).double()
        nb = self.nb.cpu()
        assert (nb[P:] == -5).all()
        h["nb"] = nb[:P].tolist()
        ca = self.conf_all.cpu()
        assert (ca[:256] == 1).all() and (ca[256 + P * 256:] == 1).all(), "the confusion matrix was written out of range"
        h["conf"] = ca[256: 256 + P * 256].reshape(P, 16, 16).long() - 1
        return h


def _args(d, o, train=1, conf=False, opt=None):
    from myfyp_amd.parallel.cnn_engine import LenetArgs

    c, a = d.c, LenetArgs()
    a.xs, a.ys, a.n_samples = d.xtab.data_ptr(), d.ytab.data_ptr(), d.n.data_ptr()
    a.perm, a.perm_ps = (d.perm.data_ptr(), d.perm.shape[1]) if d.perm is not None else (None, 0)
    a.offset, a.B, a.scale = c["offset"], c["B"], c["scale"]
    shadow, params = (opt["shadow"], opt["master"]) if opt else (d.shadow, d.params)
    a.shadow, a.shadow_ps, a.params, a.params_ps = shadow.data_ptr(), shadow.shape[1], params.data_ptr(), params.shape[1]
    for n in L.LAYERS:
        for k in ("w_", "b_", "t_"):
            setattr(a, k + n, LAY[k + n])
    a.gf, a.gf_ps, a.g, a.g_ps = o.gf.data_ptr(), o.gf.shape[1], o.g.data_ptr(), o.g.shape[1]
    a.act, a.act_ps, a.part, a.part_ps = o.act.data_ptr(), o.act.shape[1], o.part.data_ptr(), o.part.shape[1]
    a.stats, a.nb, a.confusion = o.stats.data_ptr(), o.nb.data_ptr(), o.conf.data_ptr() if conf else None
    a.train = train
    if opt:
        hp = opt["hp"]
        a.wmaster, a.mom, a.shadow_rw = params.data_ptr(), opt["mom"].data_ptr(), shadow.data_ptr()
        a.anchor, a.cg, a.cl = (opt[k].data_ptr() if opt.get(k) is not None else None for k in ("anchor", "cg", "cl"))
        a.opt_kind, a.opt_lr, a.opt_beta1, a.opt_beta2, a.opt_eps = 1, hp["lr"], 0.9, 0.999, 1e-8
        a.opt_wd, a.opt_momentum, a.opt_nesterov, a.opt_mu = hp["weight_decay"], hp["momentum"], int(hp["nesterov"]), hp["mu"]
        a.f1_e2t = opt["e2t"].data_ptr()
    return a


def _launch(lib, d, o, **kw):
    a = _args(d, o, **kw)
    assert lib.lenet_fused_step(ctypes.byref(a), P, L.IPW, _stream()) == 0
    return o.host()


@functools.lru_cache(maxsize=None)
def _grad_run(B, family):
    """One gradients-only launch (``mom = nullptr``, ``train = 1``) of the case, shared by the tests."""
    from myfyp_amd.parallel.cnn_engine import _lib

    c, r = _host(B, family)
    d = Dev(c)
    k = _launch(_lib(), d, Out(B))
    d.intact()
    return d, k


def _blk(k):
    return L.act_split(k["act"].double())


def _equal(name, got, ref):
    bad = got.double() != ref
    assert not bad.any(), f"{name}: {int(bad.sum())} elements differ, first at {bad.nonzero()[0].tolist()}: {got[bad][0]} vs {ref[bad][0]}"


WORST = {}


def _bounded(name, got, ref64, ref32, wrong64=None, fill=MARK):
    """``got`` against ``ref64`` at ``fp32_bound(ref64, ref32)``; NaN in the reference = still ``fill``."""
    hole = torch.isnan(ref64)
    assert (got[hole] == fill).all(), f"{name}: an element the kernel has no business writing was written"
    bound = O.fp32_bound(ref64, ref32)
    err = float((got.double() - ref64)[~hole].abs().max())
    ratio = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
    WORST[name] = max(WORST.get(name, 0.0), ratio)
    print(f"{name}: |err| {err:.3e}, bound {bound:.3e}, |err| / bound {ratio:.3f}")
    assert err <= bound, f"{name}: {err:.3e} > {bound:.3e}"  # MI355X: the worst ratio of each caller is noted at its call
    if wrong64 is not None:
        assert float((got.double() - wrong64)[~hole].abs().max()) > bound, f"{name}: the wrong reference passes too"


def _layer_slices(n):
    return slice(LAY["w_" + n], LAY["w_" + n] + L._numel(L.WSHAPE[n])), slice(LAY["b_" + n], LAY["b_" + n] + L.TSHAPE[n][0])


def _conv_grads32(cv, f, x):
    """The fp32 evaluation of the four conv gradient sums on the float64 stage tensors."""
    return {"gW2": L.bwd_conv2_w(cv["dz2"].float(), f["p1"].float()), "gW1": L.bwd_conv1_w(cv["dz1"].float(), x.float()),
            "gb2": cv["m2"].float().sum((1, 2, 3)), "gb1": cv["m1"].float().sum((1, 2, 3))}


# ---------------------------------------------------------------------------------------------
# gradients-only mode
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,family", EXACT)
def test_forward_and_head(B, family):
    """Bit-exact: p2 | z3 | z4 of the valid rows, nb, correct (CPU proof: conv1, conv2, fc1, fc2, fc3 exact).
    Bounded: loss (2^-18 (1 + max|z|) per row), dlogits (bf16_bound(ref, 1 / valid))."""
    c, r = _host(B, family)
    d, k = _grad_run(B, family)
    kb = _blk(k)
    assert k["nb"] == r["nb"] == c["valid"]
    for p in range(P):
        v = r["nb"][p]
        for name in ("p2", "z3", "z4"):
            _equal(f"{name}[{p}]", kb[name][p, :v], L.act_split(r["act"])[name][p, :v])
        assert torch.isfinite(k["act"][p].float()).all()  # invalid rows: a zero image's forward, times dz = 0 in the fc sums
        for name in ("dl", "dz4", "dz3"):
            assert not kb[name][p, v:].any(), f"{name}: rows of invalid images are not exact zeros"
        assert not kb["dl"][p, :, L.F3:].any()
    assert torch.equal(k["stats"][:, 1], r["correct"])
    z = r["logits"]
    bound = torch.tensor([sum(2.0 ** -18 * (1 + float(z[p, b].abs().max())) for b in range(r["nb"][p])) for p in range(P)], dtype=F64)
    err = (k["stats"][:, 0] - r["loss"]).abs()
    print(f"loss: worst |err| / bound {float((err[:2] / bound[:2]).max()):.3f}")
    assert (err <= bound).all()  # MI355X: worst |err| / bound 0.068
    short = O.xent(L._pad_last(z, 16), r["labels"], [max(0, n - 1) for n in r["nb"]], L.F3)[0]
    assert ((k["stats"][:, 0] - short).abs() > bound)[:2].all()
    # dlogits
    ref = O.xent(L._pad_last(z, 16), r["labels"], r["nb"], L.F3)[3]
    for p in range(2):
        v = r["nb"][p]
        bnd = O.bf16_bound(ref[p, :v], torch.full_like(ref[p, :v], 1.0 / v))
        ratio = float(((kb["dl"][p, :v] - ref[p, :v]).abs() / bnd).max())
        print(f"dlogits[{p}]: worst |err| / bound {ratio:.3f}")
        WORST["dlogits"] = max(WORST.get("dlogits", 0.0), ratio)
        assert ratio <= 1.0  # MI355X: worst |err| / bound 0.499 (the bf16 rounding itself)
        if v > 1:
            assert ((kb["dl"][p, :v] - ref[p, :v] * v / (v - 1)).abs() > bnd).any(), "dlogits divided by valid - 1 passes too"
    # controls: one pixel / one weight of conv1, conv2, fc1, fc2 moved by a unit changes the oracle's forward
    for label, over in L.single_changes(c, r).items():
        if label in ("label", "w_f3"):
            continue
        kk = dict(c, **over)
        x = O.input_prep(kk["xs"], kk["ys"], kk["perm"], kk["offset"], B, 3, 8, kk["scale"])[0]
        f = L.forward(x, L.to_wf(kk["W"]), kk["b"])
        assert any(C.differs(f[n][0, :B], kb[n][0, :B, : f[n].shape[-1]]) for n in ("p2", "z3", "z4")), label


@pytest.mark.parametrize("B,family", EXACT)
def test_fc_dgrads_from_the_kernels_own_upstream(B, family):
    """Bit-exact: dz4 = bf16(mask * dl . W3) from the kernel's dl, dz3 = bf16(mask * dz4 . W2) from the kernel's
    dz4; the exactness condition of each stage is asserted on those inputs."""
    c, r = _host(B, family)
    d, k = _grad_run(B, family)
    kb, E = _blk(k), r["E"]
    ratios = L.stage_ratios(r, E, dl=kb["dl"], dz4=kb["dz4"][..., :L.F2], dz3=kb["dz3"][..., :L.F1])
    for name in ("dl.W3", "dz4.W2"):
        assert ratios[name] < C.LIM, f"{name}: not exact on the kernel's own upstream"
    dz4 = L.bwd_fc3(kb["dl"], r["z4"], E)
    _equal("dz4", kb["dz4"][..., :L.F2], dz4)
    dz3 = L.bwd_fc2(kb["dz4"][..., :L.F2], r["z3"], E)
    _equal("dz3", kb["dz3"][..., :L.F1], dz3)
    assert not kb["dz4"][..., L.F2:].any() and not kb["dz3"][..., L.F1:].any()
    assert dz4[0].any() and dz3[0].any() and (dz4[0] == 0).any()
    # controls: one weight moved by a unit; the masks >= 0 instead of > 0
    W3 = dict(c["W"], f3=C.bump(c["W"]["f3"], (0, 0, int(r["z4"][0, 0].nonzero()[0]), 0), L.F3_SCALE))
    assert C.differs(L.bwd_fc3(kb["dl"], r["z4"], L.to_wf(W3)), kb["dz4"][..., :L.F2])
    W2 = dict(c["W"], f2=C.bump(c["W"]["f2"], (0, int(kb["dz4"][0, 0].nonzero()[0]), int(r["z3"][0, 0].nonzero()[0]), 0), 1.0))
    assert C.differs(L.bwd_fc2(kb["dz4"][..., :L.F2], r["z3"], L.to_wf(W2)), kb["dz3"][..., :L.F1])
    assert C.differs(L.bwd_fc3(kb["dl"], r["z4"] + 1, E), kb["dz4"][..., :L.F2])  # every unit live: the mask matters


@pytest.mark.parametrize("B,family", EXACT)
def test_gradients(B, family):
    """Bounded (fp32_bound): the fc sums over the kernel's exported act block; the conv sums of the oracle's
    backward from the kernel's dz3 (dp2, dz2, dp1, dz1 exact on it: asserted). Bit-exact: padding and gaps keep
    the marker, records of workgroups without a valid image are zero, gf / g of the conv layers are the
    sequential fp32 sum of the records."""
    c, r = _host(B, family)
    d, k = _grad_run(B, family)
    kb, E = _blk(k), r["E"]
    kdz3 = kb["dz3"][..., :L.F1]
    ratios = L.stage_ratios(r, E, dl=kb["dl"], dz4=kb["dz4"][..., :L.F2], dz3=kdz3)
    for name in ("dz3.W1", "conv2 dgrad"):
        assert ratios[name] < C.LIM, f"{name}: not exact on the kernel's own upstream"
    cv = L.conv_backward(kdz3, r, r["x"], E)
    fc64, fc32 = L.fc_grads(kb), L.fc_grads(kb, F32)
    cv32 = _conv_grads32(cv, r, r["x"])
    gf64, g64 = L.pack_grads(cv, fc64)
    gf32, g32 = L.pack_grads(dict(cv, **cv32), fc32)
    wrong = L.conv_backward(kdz3, r, r["x"], E, last=True)  # the tie rule reversed
    gfw, gw = L.pack_grads(wrong, fc64)
    for n in L.LAYERS:
        ws, bs = _layer_slices(n)
        conv = n in ("c1", "c2")
        # MI355X: worst |err| / bound 0.250 (dW_c1, B = 66), 0.178 (dW_f3, B = 66); every other sum came out equal to float64's
        _bounded(f"dW_{n}", k["gf"][:, ws], gf64[:, ws], gf32[:, ws], gfw[:, ws] if conv else None)
        _bounded(f"db_{n}", k["g"][:, bs], g64[:, bs], g32[:, bs])
    # everything outside the layers' slabs
    hole = torch.isnan(gf64)
    assert (k["gf"][hole] == MARK).all() and (k["g"][torch.isnan(g64)] == MARK).all()
    assert int(hole[0].sum()) == LAY["shadow_n"] - (450 + 2400 + 48000 + 10080 + 840)
    # fc: one batch row dropped from the sums must fail (B = 66: the second trip and the tail of the K loop)
    drop = L.fc_grads({kk: v[:, : B - 1] for kk, v in kb.items()})
    ws, _ = _layer_slices("f3")
    gfd = L.pack_grads(cv, drop)[0]
    assert float((k["gf"][0, ws].double() - gfd[0, ws]).nan_to_num().abs().max()) > O.fp32_bound(gf64[:, ws], gf32[:, ws])
    # part records
    written = torch.zeros(L.PR_N, dtype=torch.bool)
    written[: L.PR_W2] = L.real_mask("c1").reshape(-1)
    written[L.PR_W2: L.PR_B1] = L.real_mask("c2").reshape(-1)
    written[L.PR_B1: L.PR_B1 + 6] = True
    written[L.PR_B2:] = True
    part = k["part"]
    assert (part[:, :, ~written] == MARK).all(), "a padding entry of a part record was written"
    for p in range(P):
        for w in range(B // 2):
            if 2 * w >= r["nb"][p]:
                assert not part[p, w, written].any(), f"peer {p} workgroup {w} has no valid image but a non-zero record"
    assert part[0, 0, written].any()
    s = torch.zeros(P, L.PR_N, dtype=F32)
    for w in range(B // 2):
        s = s + part[:, w]
    for n, lo, hi in (("c1", 0, L.PR_W2), ("c2", L.PR_W2, L.PR_B1)):
        ws, bs = _layer_slices(n)
        m = L.real_mask(n).reshape(-1)
        assert torch.equal(k["gf"][:, ws][:, m], s[:, lo:hi][:, m]), f"gf of {n} is not the sequential sum of the records"
    assert torch.equal(k["g"][:, _layer_slices("c1")[1]], s[:, L.PR_B1: L.PR_B1 + 6]) and torch.equal(k["g"][:, _layer_slices("c2")[1]], s[:, L.PR_B2:])


@pytest.mark.parametrize("B,family", [(8, "pix3"), (66, "pix7")])
def test_second_launch_is_bit_identical(lib, B, family):
    """The kernel claims "no atomics" for the gradients: gf, g and act of a second launch on re-poisoned
    outputs are bit-identical."""
    d, k = _grad_run(B, family)
    k2 = _launch(lib, d, Out(B))
    d.intact()
    for name in ("gf", "g", "act", "part"):
        assert torch.equal(_bits(k[name]), _bits(k2[name])), name
    assert k2["nb"] == k["nb"]


def test_randn_sanity(lib):
    """Random normal weights, u8 pixels x 1/255: every stage recomputed from the kernel's own upstream, compared
    at the bounds only (bf16_bound with M = sum |term|; fp32_bound for the fc sums)."""
    B = 8
    c, r = _host(B, "randn")
    d, k = _grad_run(B, "randn")
    kb, E, b = _blk(k), r["E"], c["b"]
    assert k["nb"] == r["nb"]
    f1, f2, f3 = E["f1"][:, :, 0], E["f2"][:, :L.F2, 0], E["f3"][:, :L.F3, 0, :L.F2]

    def close(name, got, ref, big, rows):
        worst = 0.0
        for p in range(2):
            v = rows[p]
            worst = max(worst, float(((got[p, :v] - ref[p, :v]).abs() / O.bf16_bound(ref[p, :v], big[p, :v])).max()))
        print(f"randn {name}: worst |err| / bound {worst:.3f}")
        WORST["randn " + name] = worst
        assert worst <= 1.0, name  # MI355X: z3 0.499, z4 0.498, dlogits 0.496, dz4 0.500, dz3 0.497

    mm = lambda a, w: torch.einsum("pbk,pnk->pbn", a.abs(), w.abs())
    close("z3", kb["z3"][..., :L.F1], L.fc_fwd(kb["p2"], f1, b["f1"], True, L.ident), mm(kb["p2"], f1) + b["f1"].abs()[:, None], r["nb"])
    close("z4", kb["z4"][..., :L.F2], L.fc_fwd(kb["z3"][..., :L.F1], f2, b["f2"], True, L.ident), mm(kb["z3"][..., :L.F1], f2) + b["f2"].abs()[:, None], r["nb"])
    lg = L.fc_fwd(kb["z4"][..., :L.F2], f3, b["f3"], False)
    dl = O.xent(L._pad_last(lg, 16), r["labels"], r["nb"], L.F3)[3]
    # the fp32 logits carry 2^-20 * sum|term| of error, which the softmax passes on at most once
    big = (1.0 + mm(kb["z4"][..., :L.F2], f3).amax(2, keepdim=True)) / torch.tensor([max(1, n) for n in r["nb"]], dtype=F64)[:, None, None]
    close("dlogits", kb["dl"], dl, big.expand_as(dl), r["nb"])
    live = lambda g, z: torch.where(z > 0, g, torch.zeros((), dtype=F64))
    mmT = lambda a, w: torch.einsum("pbn,pnk->pbk", a.abs(), w.abs())
    close("dz4", kb["dz4"][..., :L.F2], L.bwd_fc3(kb["dl"], kb["z4"][..., :L.F2], E, L.ident), mmT(kb["dl"][..., :L.F3], f3), r["nb"])
    close("dz3", kb["dz3"][..., :L.F1], L.bwd_fc2(kb["dz4"][..., :L.F2], kb["z3"][..., :L.F1], E, L.ident), mmT(kb["dz4"][..., :L.F2], f2), r["nb"])
    # p2 from the inputs: p1 may sit one bf16_bound off (it is not exported), conv2 passes that on through |W2|
    M1 = O.maxpool2(L._per_peer(lambda a, w: C.conv_acc(a.abs(), w.abs().reshape(8, 5, 5, 8), 1, 0, L.Z1, L.Z1), r["x"], E["c1"]), [B] * P) + 1.0
    e1 = O.bf16_bound(r["p1"], M1)
    w2 = E["c2"].reshape(P, 16, 5, 5, 8)
    e2 = O.maxpool2(L._per_peer(lambda a, w: C.conv_acc(a, w.abs(), 1, 0, L.Z2, L.Z2), e1, w2), [B] * P)
    M2 = O.maxpool2(L._per_peer(lambda a, w: C.conv_acc(a.abs(), w.abs(), 1, 0, L.Z2, L.Z2), r["p1"], w2), [B] * P) + 1.0
    bound = (O.bf16_bound(r["p2"].reshape(M2.shape), M2) + e2).reshape(P, B, L.F0)
    worst = max(float(((kb["p2"][p, :v] - r["p2"][p, :v]).abs() / bound[p, :v]).max()) for p, v in enumerate(r["nb"][:2]))
    print(f"randn p2: worst |err| / bound {worst:.3f}")
    assert worst <= 1.0  # MI355X: 0.000 (p2 equal to the oracle's)
    fc64, fc32 = L.fc_grads(kb), L.fc_grads(kb, F32)
    cv0 = {"gW1": torch.full((P, 8, 25, 8), L.NAN, dtype=F64), "gW2": torch.full((P, 16, 25, 8), L.NAN, dtype=F64), "gb1": torch.full((P, 8), L.NAN, dtype=F64),
           "gb2": torch.full((P, 16), L.NAN, dtype=F64)}
    gf64, g64 = L.pack_grads(cv0, fc64)
    gf32, g32 = L.pack_grads(cv0, fc32)
    for n in ("f1", "f2", "f3"):
        ws, bs = _layer_slices(n)
        _bounded(f"randn dW_{n}", k["gf"][:, ws], gf64[:, ws], gf32[:, ws])  # MI355X: worst |err| / bound 0.063 (f1); biases 0.000
        _bounded(f"randn db_{n}", k["g"][:, bs], g64[:, bs], g32[:, bs])


# ---------------------------------------------------------------------------------------------
# fused optimizer
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,family", [(8, "pix3"), (66, "pix7")])
@pytest.mark.parametrize("variant", list(L.OPT_VARIANTS))
def test_fused_optimizer(lib, B, family, variant):
    """Bounded (fp32_bound): master rows and momentum against sgd_update in float64 on the gradients of the
    gradients-only launch (mapped to torch order by the oracle's maps). Bit-exact: shadow = bf16(the kernel's
    own new master) at every real weight's Wf position, everything else (padding, gaps, biases' absence, the
    whole peer without samples) untouched."""
    c, r = _host(B, family)
    d, k = _grad_run(B, family)
    hp = L.OPT_VARIANTS[variant]
    g = C.gen(17 + B)
    grad = L.grads_to_torch(k["gf"].double().masked_fill(k["gf"] == MARK, L.NAN), k["g"].double().masked_fill(k["g"] == MARK, L.NAN))
    real = ~torch.isnan(L.pack_params(c["W"], c["b"]))
    assert torch.equal(~torch.isnan(grad), real)
    rnd32 = lambda *s: torch.randn(*s, generator=g).double()
    n = LAY["params_n"]
    mom0 = torch.where(real, rnd32(P, n) * 0.125, torch.full((P, n), L.NAN, dtype=F64))
    extra = {"anchor": None, "cg": None, "cl": None}
    if variant == "fedprox":
        extra["anchor"] = d.params.cpu()[:, :n].double() + rnd32(P, n) * 0.25
    if variant == "scaffold":
        extra["cg"], extra["cl"] = rnd32(P, n) * 0.1, rnd32(P, n) * 0.1
    extra = {kk: (None if v is None else v.float().double()) for kk, v in extra.items()}
    opt = dict(hp=hp, master=d.params.clone(), shadow=d.shadow.clone(), mom=_buf(mom0.nan_to_num(nan=MARK), F32),
               e2t=L.E2T.to(torch.int32).cuda(), **{kk: (None if v is None else _buf(v, F32)) for kk, v in extra.items()})
    mom_before = opt["mom"].clone()
    k2 = _launch(lib, d, Out(B), opt=opt)
    d.intact()
    assert (k2["gf"] == MARK).all() and (k2["g"] == MARK).all(), "the fused optimizer also wrote gradients"
    km, kmom, ksh = opt["master"].cpu(), opt["mom"].cpu(), opt["shadow"].cpu()
    assert (km[:, n:] == MARK).all() and (kmom[:, n:] == MARK).all() and (ksh[:, LAY["shadow_n"]:] == MARK).all()
    master0 = d.params.cpu()[:, :n].double().masked_fill(~real, L.NAN)
    mom0 = mom_before.cpu()[:, :n].double().masked_fill(~real, L.NAN)
    w64, m64 = L.opt_step(master0, mom0, grad, r["nb"], hp, **extra)
    w32, m32 = L.opt_step(master0, mom0, grad, r["nb"], hp, dtype=F32, **extra)
    w_lazy, _ = L.opt_step(master0, mom0, grad * 0.5, r["nb"], hp, **extra)  # half the gradient: must fail
    _bounded(f"master[{variant}]", km[:, :n], w64, w32, w_lazy)  # MI355X: worst |err| / bound 0.081 plain, 0.184 nesterov, 0.132 fedprox, 0.250 scaffold
    _bounded(f"momentum[{variant}]", kmom[:, :n], m64, m32)  # MI355X: 0.170 nesterov, 0.168 scaffold, 0.000 without momentum
    assert float((km[:2, :n].double() - master0[:2]).nan_to_num().abs().max()) > 0
    # shadow: bf16 of the kernel's own new master at every real weight, untouched elsewhere
    want = L.shadow_of(km[:, :n].double().masked_fill(~real, L.NAN))
    got = ksh[:, : LAY["shadow_n"]]
    at = ~torch.isnan(want)
    assert torch.equal(got[at].double(), want[at].to(BF).double()), "shadow != bf16(new master)"
    assert torch.equal(_bits(got[~at]), _bits(d.shadow.cpu()[:, : LAY["shadow_n"]][~at])), "a shadow padding entry or gap was written"
    unmapped = L.shadow_of(km[:, :n].double().masked_fill(~real, L.NAN), e2t=torch.arange(L.F0))
    assert not torch.equal(got[at].double(), unmapped[at].to(BF).double()), "fc1's columns left unmapped pass too"
    # the peer without samples: untouched
    for name, new, old in (("master", opt["master"], d.params), ("momentum", opt["mom"], mom_before), ("shadow", opt["shadow"], d.shadow)):
        assert torch.equal(_bits(new[2]), _bits(old[2])), f"the peer without samples: {name} was written"


# ---------------------------------------------------------------------------------------------
# evaluation
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,family", L.EVAL_CASES)
def test_evaluation(lib, B, family):
    """``train = 0``, identity order, a confusion buffer pre-filled with ones. Bit-exact: nb, correct, confusion;
    act, gf, g, part untouched. Bounded: the loss sum as in the training head."""
    c, r = _host(B, family, False)
    assert c["perm"] is None
    d = Dev(c)
    k = _launch(lib, d, Out(B), train=0, conf=True)
    d.intact()
    assert k["nb"] == r["nb"] == c["valid"]
    assert torch.equal(k["stats"][:, 1], r["correct"]) and 0 < float(r["correct"][0])
    assert torch.equal(k["conf"], r["conf"])
    assert int(r["conf"].sum()) == sum(r["nb"]) and (B < 8 or (r["conf"][0].sum(0) > 0).sum() > 1)
    z = r["logits"]
    bound = torch.tensor([sum(2.0 ** -18 * (1 + float(z[p, b].abs().max())) for b in range(r["nb"][p])) for p in range(P)], dtype=F64)
    err = (k["stats"][:, 0] - r["loss"]).abs()
    print(f"eval loss: worst |err| / bound {float((err[:2] / bound[:2]).max()):.3f}")
    assert (err <= bound).all()  # MI355X: worst |err| / bound 0.061
    short = O.xent(L._pad_last(z, 16), r["labels"], [max(0, n - 1) for n in r["nb"]], L.F3)[0]
    assert ((k["stats"][:, 0] - short).abs() > bound)[:2].all()
    for name in ("act", "gf", "g", "part"):
        assert (k[name] == MARK).all(), f"evaluation wrote {name}"


# ---------------------------------------------------------------------------------------------
# argument checks
# ---------------------------------------------------------------------------------------------
def test_rejects_bad_arguments(lib):
    """``lenet_fused_step`` returns 1 for a null argument block, ``peers <= 0``, ``ipw != 2`` (0 included: it
    must not reach the ``B % ipw`` check) and ``B`` odd or not positive, and launches nothing (bit-exact: every
    output keeps its fill)."""
    c, _ = _host(2, "pix3")
    d, o = Dev(c), Out(2)
    a = _args(d, o)
    s = _stream()
    assert lib.lenet_fused_step(None, P, 2, s) == 1
    assert lib.lenet_fused_step(ctypes.byref(a), 0, 2, s) == 1 and lib.lenet_fused_step(ctypes.byref(a), -1, 2, s) == 1
    for ipw in (1, 4, 0, 3):
        assert lib.lenet_fused_step(ctypes.byref(a), P, ipw, s) == 1
    a.B = 3
    assert lib.lenet_fused_step(ctypes.byref(a), P, 2, s) == 1
    a.B = 0
    assert lib.lenet_fused_step(ctypes.byref(a), P, 2, s) == 1
    h = o.host()  # nothing was launched: every output still holds its fill
    for name in ("act", "gf", "g", "part"):
        assert (h[name] == MARK).all()
    assert h["nb"] == [-5] * P and not h["stats"][:, :2].any()
    d.intact()
