"""The fp32 epoch kernels (csrc/kernels/mlp_persistent_f32.hip, layouts 1 and 3 at every owner K split, and
mlp_persistent_f32v2.hip, layout 2) and ``mlp_eval_f32`` against the float64 oracle of ``tests/_mlp_ref.py``, element
by element. Nothing here compares one kernel variant with another or with fp32 torch; every tolerance is a bound
derived in ``_mlp_ref``'s section on the fp32 kernels (forward exact on the dyadic grid, ``eps_softmax32``, ``bounds32``,
``upd32``, ``loss_bound``), or 8 times the oracle's own fp32 sensitivity, printed beside the kernel's figure (part d).
``tests/test_mlp_ref_cpu.py`` holds the oracle itself to float64 autograd and asserts the exactness condition and the
sensitivity cap of every case used here.

Two peers per engine with their own weights, data, row counts and epoch orders, driven as the other fp32 tests
drive the kernel (``TorchLearner`` on ``MLPGroup``, pinned permutations, ``force_f32_variant`` / ``force_f32_ks``), state read
back from the flat parameters, ``g.m``, ``g.v`` and the raw sums of ``g._fetch``. A fit is run once per configuration and
shared by the tests that need it.

(a) one SGD step with momentum 0.9 from ``m = 0``: ``m`` IS the gradient. All six tensors per element, the new weights
    from the kernel's own ``m``, the loss sum and the correct count (ties to the lowest class where D3 = 16). With one
    valid row dW3 and dW2 are the singly rounded outer products of the kernel's own db3 and db2 with the exact H2
    and H1, bit for bit, in every layout (the K splits divide X's columns, never the batch). dW1 is within one ulp
    of the exact db1 x X: the derivation (lo x + mid x exact, + hi x rounds once) would make it the rounded product
    too, but the bf16 MFMA rounds that last sum faithfully, not to nearest: MI355X, 0.3 % of the elements are
    the other neighbour, in every layout. db1 passes through the same split (the bias input 1): a lo term lost from
    the split shows as a db1 whose low significand byte is zero in a third of its elements, not in one of 256.
(b) one step of every optimizer variant from the gradient of (a): ``w``, ``m``, ``v`` at ``upd32``'s bounds; Adam's second
    epoch (``t0 > 0``): the weights from the kernel's own moments and its own first-epoch weights.
(c) ``lr = 0``: 2, 3 and 5 steps on the grid, the weights come back bit-equal, SGD with momentum 1 leaves the sum of
    the steps' gradients in ``m``, Adam its recursions in ``m`` and ``v`` (also across the two epochs of one fit).
(d) real learning rates on random weights, 3 and 5 steps: relative update error per tensor against the float64
    epoch within 8 times the fp32 twin's.
(e) ``mlp_eval_f32``: confusion matrix exact (ties included), loss within its bound.

Mutations tried against this file (neither is in the tree): ``mfma3`` without its ``lo`` term fails (a) with one row (db1's
low byte zero in 29 to 40 % of its elements) and (d) (b3 at 1.5 to 3.6 times its limit wherever the forward takes ``mfma3``, and a relu
of H2 that falls the other way, 1.8e-2, in three layouts); ``rows_at`` one short on a partial last batch fails
(a), (c) and (d), by orders of magnitude.
"""

import threading

import numpy as np
import pytest
import torch

import _mlp_ref as M

pytestmark = pytest.mark.gpu

U = M.U
GRAD_HP = dict(kind=1, lr=2.0 ** -10, momentum=0.9, wd=0.0, nesterov=False)  # (a): m = fmaf(0.9, 0, g) = g
FROZEN = {"sgdm1": dict(kind=1, lr=0.0, momentum=1.0, wd=0.0, nesterov=False), "adam": dict(kind=0, lr=0.0)}
VARIANTS = {
    "sgd": M.OPT_VARIANTS["sgd"],
    "nesterov_wd": M.OPT_VARIANTS["nesterov_wd"],
    "adam_t0": M.OPT_VARIANTS["adam_t0"],
    "adam_wd": dict(kind=0, lr=1e-3, wd=1e-4),
    "fedprox": M.OPT_VARIANTS["fedprox"],
    "scaffold_sgd": dict(kind=1, lr=2.0 ** -6, momentum=0.9, wd=0.0, nesterov=False, scaffold=True),
}


@pytest.fixture(scope="module")
def lib():
    from myfyp_amd.ops import _native

    return _native.load(required=True)


@pytest.fixture(autouse=True)
def fp32_settings(lib):
    from myfyp_amd.parallel.mlp_engine import MLPGroup
    from myfyp_amd.settings import Settings

    old = (Settings.MLP_PRECISION, Settings.GANG_WINDOW, Settings.USE_FUSED_KERNELS)
    Settings.MLP_PRECISION, Settings.GANG_WINDOW, Settings.USE_FUSED_KERNELS = "fp32", 5.0, True
    MLPGroup.reset_all()
    yield
    lib.mlp_set_f32_h1_frag(-1)
    lib.mlp_set_f32_dh2_frag(-1)
    MLPGroup.reset_all()
    Settings.MLP_PRECISION, Settings.GANG_WINDOW, Settings.USE_FUSED_KERNELS = old


_CASES, _FITS = {}, {}  # cases and fits by configuration: computed once, never modified


def _case(*key):
    if key not in _CASES:
        _CASES[key] = M.case32(*key)
    return _CASES[key]


def _spec(hp):
    if hp["kind"] == 0:
        return {"name": "adam", "lr": hp["lr"], "weight_decay": hp.get("wd", 0.0)}
    return {"name": "sgd", "lr": hp["lr"], "momentum": hp["momentum"], "weight_decay": hp.get("wd", 0.0), "nesterov": hp["nesterov"]}


def _extras(c, hp, dev):
    """FedProx anchors / SCAFFOLD control variates of the two peers (fp32 values), as the engine takes them and as
    float64 dictionaries."""
    if "mu" not in hp and not hp.get("scaffold"):
        return None, [{}, {}]
    numel = M.offsets(c["D"])[1]
    dev_side, ref = [], []
    for p in range(2):
        g = torch.Generator().manual_seed(90 + p)
        flat = M.pack({k: v[None] for k, v in c["W"][p].items()}, c["D"])[0]
        if "mu" in hp:
            a = (flat + 0.01 * torch.randn(numel, generator=g).double()).float()
            dev_side.append({"anchor": a.to(dev).contiguous(), "mu": hp["mu"]})
            ref.append({"anchor": M.unpack(a.double(), c["D"])})
        else:
            cg, cl = (1e-3 * torch.randn(numel, generator=g)).float(), (1e-3 * torch.randn(numel, generator=g)).float()
            dev_side.append({"c_global": cg.to(dev).contiguous(), "c_local": cl.to(dev).contiguous()})
            ref.append({"cg": M.unpack(cg.double(), c["D"]), "cl": M.unpack(cl.double(), c["D"])})
    return dev_side, ref


def _learners(c, spec):
    from myfyp_amd.learning.dataset.p2pfl_dataset import P2PFLDataset
    from myfyp_amd.learning.frameworks.torch import TorchLearner, TorchModel
    from myfyp_amd.models import MLP

    out = []
    for p in range(2):
        m = MLP(input_size=c["D"][0], out_channels=c["D"][3])
        with torch.no_grad():
            for i, l in enumerate(m.linear_layers()):
                l.weight.copy_(c["W"][p][f"W{i + 1}"])
                l.bias.copy_(c["W"][p][f"b{i + 1}"])
        m.optimizer_spec = lambda spec=spec: dict(spec)
        split = lambda x, y: {"image": np.ascontiguousarray(x.numpy()), "label": y.numpy().astype(np.int64)}
        data = P2PFLDataset.from_arrays(split(c["x"][p], c["y"][p]), split(c["xt"][p], c["yt"][p]))
        out.append(TorchLearner(TorchModel(m), data, f"o{p}", batch_size=c["B"]))
    assert all(l._engine is not None for l in out), "fp32 engine not attached"
    return out


def _all(learners, what, extras=None):
    # every peer from its own thread: the group gangs the calls into one launch
    def run(i, l):
        if extras is None:
            getattr(l, what)()
        else:
            l._engine.fit(l, l._optimizer_spec(), extras[i])

    ts = [threading.Thread(target=run, args=(i, l)) for i, l in enumerate(learners)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    torch.cuda.synchronize()


def _group(lib, learners, layout):
    """The learners' group on ``layout``; skips where the layout rejects the shape."""
    variant, ks, frag = M.F32_LAYOUTS[layout]
    g = learners[0]._engine.group
    assert g.precision == "fp32" and g.uses_persistent()
    g.force_f32_ks, g.force_f32_variant = ks, variant
    if g.f32_ks() != ks:
        pytest.skip(f"K split {ks} is instantiated for the 64-row batch tile only (B {g.B}: the launch takes K split {g.f32_ks()})")
    if g.f32_variant() != variant:
        pytest.skip(f"layout {variant} rejects this shape (v3_supported / mlp_f32v2_supported): the launch takes layout {g.f32_variant()}")
    return g


def _fit(lib, layout, ckey, hp, epochs=1, same_perm=False, fresh=False):
    """One fit of the two peers of case ``ckey`` on ``layout``: per peer the start and end weights, ``m``, ``v`` (float64
    dictionaries), the fit's loss sum and correct count as the device wrote them, and the references of the extras."""
    from myfyp_amd.parallel.mlp_engine import MLPGroup

    key = (layout, ckey, tuple(sorted(hp.items())), epochs, same_perm)
    if key in _FITS and not fresh:
        return _FITS[key]
    dev = torch.device("cuda")
    c = _case(*ckey)
    variant, ks, frag = M.F32_LAYOUTS[layout]
    lib.mlp_set_f32_h1_frag(frag)
    lib.mlp_set_f32_dh2_frag(frag)
    MLPGroup.reset_all()
    learners = _learners(c, _spec(hp))
    g = _group(lib, learners, layout)
    n = c["n"]

    def perm_fn(ep):
        out = torch.zeros(g.capacity, g.nmax, dtype=torch.int32)
        for p, l in enumerate(learners):
            out[l._engine.slot, : n[p]] = torch.from_numpy(M.epoch_perm32(n[p], 0 if same_perm else ep, p)).to(torch.int32)
        return out.to(dev)

    g.perm_fn = perm_fn
    for l in learners:
        l.set_epochs(epochs)
    extras, ext_ref = _extras(c, hp, dev)
    sums, fetch = [], g._fetch

    def fetch_and_keep(k, with_conf):
        r = fetch(k, with_conf)
        sums.append((r[0].copy(), r[1].copy()))
        return r

    g._fetch = fetch_and_keep
    _all(learners, "fit", extras)
    g.resolver.flush()  # the fit's sums are fetched by the resolver thread
    assert g.f32_ks() == ks and g.f32_variant() == variant and g.recoveries() == 0
    if layout == "v1ks1" and ckey[:3] == M.F32_MAIN:
        assert lib.mlp_f32_h1_frag_last() == (0 if extras is not None else 1), "the shipping path is the fragment hand-off"
    if layout == "v1ks1_rows":
        assert lib.mlp_f32_h1_frag_last() == 0 and lib.mlp_f32_dh2_frag_last() == 0
    assert len(sums) == 1, f"{len(sums)} fit results fetched"
    numel = M.offsets(c["D"])[1]
    out = []
    for p, l in enumerate(learners):
        s = l._engine.slot
        rd = lambda t: M.unpack(t.detach().cpu().double()[:numel], c["D"])
        out.append(dict(w0=c["W"][p], w=rd(l.flat_params()), m=rd(g.m[s]), v=rd(g.v[s]), loss=float(sums[0][0][s]), correct=int(sums[0][1][s]), ext=ext_ref[p]))
        for k in ("w", "m", "v"):
            assert all(torch.isfinite(t).all() for t in out[-1][k].values()), f"peer {p} {k}: not finite"
    if not fresh:
        _FITS[key] = out
    return out


def _within(what, got, ref, bound):
    err = (got - ref).abs()
    bad = err > bound
    ratio = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    if bad.any():
        i = int((err / bound.clamp_min(1e-300)).flatten().argmax())
        pytest.fail(f"{what}: {int(bad.sum())} of {err.numel()} elements beyond the bound, worst at flat index {i}: got {float(got.flatten()[i])!r}, "
                    f"reference {float(ref.flatten()[i])!r}, error {float(err.flatten()[i]):.3e}, bound {float(bound.flatten()[i]):.3e} ({ratio:.1f} x)")
    return ratio


def _bits(what, got, ref):
    """Equal as fp32 numbers; below 2^-100 (fp32 denormals are not specified for the MFMA) within 2^-100."""
    big = ref.abs() >= M.TINY32
    bad = (big & (got != ref)) | (~big & ((got - ref).abs() > M.TINY32))
    if bad.any():
        i = int(bad.flatten().nonzero()[0])
        rel = float(((got - ref).abs() / ref.abs().clamp_min(1e-300))[big].max()) if big.any() else 0.0
        pytest.fail(f"{what}: {int(bad.sum())} of {bad.numel()} elements are not the singly rounded product, first at flat index {i}: got {float(got.flatten()[i])!r}, "
                    f"want {float(ref.flatten()[i])!r}; largest relative difference 2^{np.log2(max(rel, 1e-300)):.1f}")


def _steps(c, p, same_perm=False, epochs=1):
    """The oracle's steps of peer ``p`` with the weights frozen at the start: one ``step32`` per batch of every epoch."""
    out = []
    for ep in range(epochs):
        perm = M.epoch_perm32(c["n"][p], 0 if same_perm else ep, p)
        for s in range(0, c["n"][p], c["B"]):
            idx = torch.as_tensor(perm[s: s + c["B"]], dtype=torch.int64)
            out.append(M.step32(c["W"][p], c["x"][p][idx].double(), c["y"][p][idx].long()))
    return out


def _check_sums(what, r, steps):
    losses = torch.cat([s["loss"] for s in steps])
    want, bound = float(losses.sum()), M.loss_bound(losses, max(s["eps_lp"] for s in steps))
    print(f"{what}: loss sum {r['loss']!r}, float64 {want!r}, error {abs(r['loss'] - want):.3e}, bound {bound:.3e}")
    assert abs(r["loss"] - want) <= bound, f"{what}: loss sum {r['loss']!r}, float64 {want!r}, bound {bound:.3e}"
    correct = sum(int((s["pred"] == s["y"]).sum()) for s in steps)
    assert r["correct"] == correct, f"{what}: correct count {r['correct']}, the oracle's {correct}"


def _ckey(shape, n, family=None):
    D0, D3, B = shape
    return (D0, D3, B, family or M.f32_family(D3), tuple(n))


_LAYOUT_CASES = M.f32_layout_cases()
_IDS = [f"{l}-{s[0]}-{s[1]}-B{s[2]}" for l, s in _LAYOUT_CASES]


# ---------------------------------------------------------------------------------------------
# (a) one step: the gradients per element
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,shape", _LAYOUT_CASES, ids=_IDS)
def test_one_step_gradients_per_element(lib, layout, shape):
    """Valid rows 1, 2, 31, 32, 33, 63, 64 as far as B allows, two peers per fit. ``m`` against the float64 gradient at
    ``bounds32``; ``v`` untouched; ``w`` from the kernel's own ``m`` at ``upd32``'s bound (one fma: u |w'|); the loss sum at
    ``loss_bound``; the correct count exactly. One row: the weight gradients bit for bit (module docstring)."""
    worst = {}
    for n in M.F32_ONE_STEP[shape[2]]:
        c = _case(*_ckey(shape, n))
        fit = _fit(lib, layout, _ckey(shape, n), GRAD_HP)
        for p, r in enumerate(fit):
            what = f"{layout} {shape} peer {p} rows {n[p]}"
            (s,) = _steps(c, p)
            bnd = M.bounds32(s, c["W"][p])
            for k in M.NAMES:
                worst[k] = max(worst.get(k, 0.0), _within(f"{what} d{k}", r["m"][k], s["g"][k], bnd[k]))
                assert not r["v"][k].any(), f"{what}: SGD wrote v of {k}"
                w1, _, _, bw, _, _ = M.upd32(GRAD_HP, r["w0"][k], r["m"][k], torch.zeros_like(r["m"][k]), r["v"][k], 1)
                _within(f"{what} new {k}", r["w"][k], w1, bw)
            if shape[1] > 1:
                assert all(float(r["m"][k].abs().max()) > 0 for k in M.NAMES), f"{what}: a gradient tensor is all zero"
            _check_sums(what, r, [s])
            if n[p] == 1:
                for k, b, a in (("W3", "b3", "H2"), ("W2", "b2", "H1")):
                    _bits(f"{what} d{k} = fp32(d{b} x {a})", r["m"][k], M.outer32(r["m"][b], s[a][0]))
                exact = r["m"]["b1"][:, None] * s["X"][0][None, :]  # (24 x 8 bits: exact in float64)
                _within(f"{what} dW1 = faithful(db1 x X)", r["m"]["W1"], exact, M.FAITHFUL * exact.abs() + M.TINY32)
                # db1 reaches m through the same three-term split as dW1 (the bias input 1), so the check above cannot
                # see a term missing from BOTH. But then db1 = hi + mid, and mid keeps the top 8 bits of the remainder
                # wherever they lie: its lowest bit is at or above bit 8 with probability 1/2 * 1/2 + 1/4 * 1/4 + ... =
                # 1/3, so a third of the elements have a zero low byte (29 % and 40 % measured with the term taken
                # out), where a sum of 128 unrelated fp32 products has one once in 256. At 64 elements or more, one
                # in 8 is 2e-10 improbable for the intact split and 5 standard deviations below the broken one's mean.
                bits = r["m"]["b1"].float().view(torch.int32)
                nz = bits != 0
                if int(nz.sum()) >= 64:
                    short = float(((bits & 0xFF) == 0)[nz].double().mean())
                    print(f"{what}: the low byte of db1 is zero in {100 * short:.1f} % of its {int(nz.sum())} non-zero elements")
                    assert short < 0.125, f"{what}: the low 8 significand bits of db1 are zero in {100 * short:.0f} % of its elements: the split lost its lo term"
                same = float((r["m"]["W1"] == M.outer32(r["m"]["b1"], s["X"][0])).double().mean())
                print(f"{what}: dW1 is the correctly rounded db1 x X in {100 * same:.2f} % of its elements")
    print(f"{layout} {shape}: largest error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def test_the_fit_is_deterministic(lib):
    """The same fit again: equal bits (what lets part (b) take its gradient from the run of part (a))."""
    key = _ckey(M.F32_MAIN, (31, 33))
    a, b = _fit(lib, "v1ks1", key, GRAD_HP), _fit(lib, "v1ks1", key, GRAD_HP, fresh=True)
    for p in range(2):
        for what in ("w", "m"):
            assert all(torch.equal(a[p][what][k], b[p][what][k]) for k in M.NAMES), f"peer {p} {what}"
        assert a[p]["loss"] == b[p]["loss"] and a[p]["correct"] == b[p]["correct"]


# ---------------------------------------------------------------------------------------------
# (b) one step of every optimizer variant from the kernel's own gradient
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("layout", ["v1ks1", "v2", "v3ks1"])
def test_optimizer_variants_per_element(lib, layout, variant):
    """Rows 31 and 33 of the main shape. ``w``, ``m`` and ``v`` of the variant's fit against ``upd32`` in float64 applied to the
    gradient the kernel left in ``m`` in part (a)'s fit (the kernel is deterministic), at ``upd32``'s bounds. (With an extra
    term layout 1 takes its row-image kernels.)"""
    hp = VARIANTS[variant]
    key = _ckey(M.F32_MAIN, (31, 33))
    base, fit = _fit(lib, layout, key, GRAD_HP), _fit(lib, layout, key, hp)
    for p, (b, r) in enumerate(zip(base, fit)):
        for k in M.NAMES:
            zero = torch.zeros_like(b["m"][k])
            e = r["ext"]
            w1, m1, v1, bw, bm, bv = M.upd32(hp, r["w0"][k], b["m"][k], zero, zero, 1, e["anchor"][k] if "anchor" in e else None,
                                            e["cg"][k] if "cg" in e else None, e["cl"][k] if "cg" in e else None)
            what = f"{layout} {variant} peer {p} {k}"
            _within(f"{what}: w", r["w"][k], w1, bw)
            _within(f"{what}: m", r["m"][k], m1, bm)
            _within(f"{what}: v", r["v"][k], v1, bv)
            assert not torch.equal(r["w"][k], r["w0"][k]), f"{what}: the weights did not move"


@pytest.mark.parametrize("layout", ["v1ks1", "v2", "v3ks1"])
def test_adam_second_epoch_uses_its_own_step_count(lib, layout):
    """Two one-step epochs of one Adam fit: the weights after the second epoch against ``upd32``'s tail at optimizer step
    2 (``lr / (1 - beta1^2)``, ``1 / sqrt(1 - beta2^2)``) applied to the kernel's own final moments and its own weights after
    the first epoch (the one-epoch fit of the same configuration), at the unit bound. At step 1's coefficients
    the update would be 1.9 times as large."""
    hp = VARIANTS["adam_t0"]
    key = _ckey(M.F32_MAIN, (31, 33))
    one, two = _fit(lib, layout, key, hp), _fit(lib, layout, key, hp, epochs=2)
    for p in range(2):
        for k in M.NAMES:
            w2, bw = M.adam_w32(hp, one[p]["w"][k], two[p]["m"][k], two[p]["v"][k], 2)
            _within(f"{layout} peer {p} {k}", two[p]["w"][k], w2, bw)
            upd = (w2 - one[p]["w"][k]).abs()
            assert float((bw / upd.clamp_min(1e-300)).median()) < 2.0 ** -10, "a bound that cannot tell step 2 from step 1"


# ---------------------------------------------------------------------------------------------
# (c) several steps with the weights frozen
# ---------------------------------------------------------------------------------------------
def _frozen(lib, layout, shape, n, opt, epochs=1):
    hp = FROZEN[opt]
    c = _case(*_ckey(shape, n))
    fit = _fit(lib, layout, _ckey(shape, n), hp, epochs=epochs)
    for p, r in enumerate(fit):
        what = f"{layout} {shape} {opt} peer {p} n {n[p]} epochs {epochs}"
        steps = _steps(c, p, epochs=epochs)
        assert len(steps) == epochs * -(-n[p] // shape[2])
        bnds = [M.bounds32(s, c["W"][p]) for s in steps]
        ratios = []
        for k in M.NAMES:
            assert torch.equal(r["w"][k], r["w0"][k]), f"{what}: lr = 0 and {k} moved"
            m, v, bm, bv = M.moments32(hp, r["w0"][k], [s["g"][k] for s in steps], [b[k] for b in bnds])
            ratios.append(_within(f"{what} m of {k}", r["m"][k], m, bm))
            _within(f"{what} v of {k}", r["v"][k], v, bv)
        _check_sums(what, r, steps)
        print(f"{what}: largest error / bound of m " + ", ".join(f"{k} {v:.3f}" for k, v in zip(M.NAMES, ratios)))


@pytest.mark.parametrize("opt", list(FROZEN))
@pytest.mark.parametrize("layout,shape", _LAYOUT_CASES, ids=_IDS)
def test_frozen_weights_every_step_per_element(lib, layout, shape, opt):
    """``lr = 0``: every step's forward stays on the grid. 2, 3 and 5 steps with the last batch partial (peer 0) and full
    (peer 1) at the main shape and on the shipping layout, 3 steps elsewhere. ``w`` bit-equal to the start; SGD with
    momentum 1: ``m`` is the sum of the steps' gradients in step order; Adam: the beta recursions of ``m`` and ``v``; both at
    the bounds of (a) carried through ``moments32``. Loss sum and correct count over the epoch."""
    pairs = M.F32_STEPS[shape[2]]
    for n in pairs if shape == M.F32_MAIN or layout == "v1ks1" else pairs[1:2]:
        _frozen(lib, layout, shape, n, opt)


@pytest.mark.parametrize("layout", ["v1ks1", "v2", "v3ks1"])
def test_frozen_weights_moments_carry_over_epochs(lib, layout):
    """Two epochs of one Adam fit at ``lr = 0``, 3 steps each (other orders): the moments of the six steps' recursion, the
    loss sum and the correct count of both epochs."""
    _frozen(lib, layout, M.F32_MAIN, M.F32_STEPS[64][1], "adam", epochs=2)


# ---------------------------------------------------------------------------------------------
# (d) real learning rates
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hp", list(M.F32_LEARN_HP))
@pytest.mark.parametrize("layout", list(M.F32_LAYOUTS))
@pytest.mark.parametrize("shape", [M.F32_MAIN, M.F32_RAGGED], ids=["main", "ragged"])
def test_learning_epoch_within_the_oracles_sensitivity(lib, shape, layout, hp):
    """``randn32`` weights, SGD at 1e-4 and SGD + momentum + Nesterov + weight decay, 3 steps (peer 0) and 5 steps (peer 1),
    the last batch partial: the relative update error of each tensor against the float64 epoch within 8 times the
    fp32 twin's (both printed). A stale weight, a step applied twice or a batch out of order moves a tensor by
    the order of 1 / steps."""
    B = shape[2]
    key = _ckey(shape, M.F32_LEARN[B], "randn32")
    c = _case(*key)
    fit = _fit(lib, layout, key, M.F32_LEARN_HP[hp])
    bad = []
    for p, r in enumerate(fit):
        ref, alt = M.learn_refs(c, p, M.F32_LEARN_HP[hp])
        for k in M.NAMES:
            floor, rel = M.rel_update(alt[k], ref[k], r["w0"][k]), M.rel_update(r["w"][k], ref[k], r["w0"][k])
            print(f"{layout} {shape} {hp} peer {p} {k}: oracle floor {floor:.3e}, kernel {rel:.3e}, kernel / (8 floor) {rel / (8 * floor):.3f}")
            assert 8 * floor < 1e-3
            if not rel <= 8 * floor:
                bad.append((p, k, rel, floor))
    assert not bad, bad


# ---------------------------------------------------------------------------------------------
# (e) mlp_eval_f32
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,family,n_test,seed", M.F32_EVAL, ids=[f"{c[0][0]}-{c[1]}" for c in M.F32_EVAL])
def test_eval_f32_on_the_grid(lib, D, family, n_test, seed):
    """Test splits of 1, 70, 512 and 517 rows (64-row chunks: one row, a ragged chunk, whole chunks, whole chunks and a
    ragged one). The confusion matrix against the oracle's first maximum, ties included; the loss sum within
    ``loss_bound`` (library ``expf`` / ``logf``: within ``eps_lp``); the correct count."""
    from myfyp_amd.parallel.mlp_engine import MLPGroup

    MLPGroup.reset_all()
    c = _case(D[0], D[1], 64, family, (4, 4), tuple(n_test), seed)
    learners = _learners(c, _spec(GRAD_HP))
    g = learners[0]._engine.group
    got, fetch = [], g._fetch

    def fetch_and_keep(k, with_conf):
        r = fetch(k, with_conf)
        got.append(tuple(None if t is None else t.copy() for t in r))
        return r

    g._fetch = fetch_and_keep
    _all(learners, "evaluate")
    g.resolver.flush()
    assert len(got) == 1 and got[0][2] is not None
    for p, l in enumerate(learners):
        s = l._engine.slot
        X, y = c["xt"][p].double(), c["yt"][p].long()
        _, _, z = M.forward32(c["W"][p], X)
        loss, pred, _ = M.head(z, y)
        conf = torch.zeros(16, 16, dtype=torch.int64)
        for a, b in zip(y.tolist(), pred.tolist()):
            conf[a, b] += 1
        assert torch.equal(torch.from_numpy(got[0][2][s].astype(np.int64)), conf), f"peer {p}: confusion matrix"
        assert int(got[0][1][s]) == int((pred == y).sum())
        want, bound = float(loss.sum()), M.loss_bound(loss, M.eps_softmax32(z)[0])
        print(f"{D} {family} peer {p} n_test {n_test[p]}: loss sum {float(got[0][0][s])!r}, float64 {want!r}, bound {bound:.3e}")
        assert abs(float(got[0][0][s]) - want) <= bound
