"""The bf16 epoch kernel (csrc/kernels/mlp_persistent.hip, ``mlp_persistent_epoch<BP, ADAM>``) against the float64
oracle of ``tests/_mlp_ref.py`` (section "the bf16 epoch kernel"), element by element. Nothing here compares the
kernel with another kernel or with fp32 torch: the forward is exact on the dyadic grid, everything behind the
fast softmax lies in the interval ``step16`` derives for it, a gradient within ``bounds16``'s radius of the central
one, the optimizer within ``adam_moments16`` / ``adam_w32`` with ``adam_coeffs16`` / ``upd32``, the loss sum within ``loss_bound``; part
(d) within 8 times the oracle's own fp32 sensitivity, printed beside the kernel's figure. ``tests/test_mlp_ref_cpu.py``
asserts the oracle's conditions (exactness, the three caps, the floor) for every case used here.

Two peers per engine with their own weights, data, row counts and pinned epoch orders (``TorchLearner`` on ``MLPGroup``,
``Settings.MLP_PRECISION = "bf16"``), state read back from the flat parameters, ``g.m``, ``g.v``, ``g.shadow``, ``g.w2t`` and the raw
sums of ``g._fetch``. One fit per configuration, shared by the tests that need it. Before every fit ``m``, ``v``, ``shadow`` and
``w2t`` of every slot are filled with a pattern: a fresh fit must not read it, SGD must leave ``m`` zero and ``v`` alone,
an idle peer must keep every byte; after every fit ``shadow`` is ``bf16(master)`` and ``w2t`` its transposed W2, bit for bit.

(a) one Adam step at ``lr = 0`` (``m = fl(c1 g)``: the gradient to one ulp), every shape: the six gradients per element, ``v``
    from the kernel's own ``m``, the loss sum, the correct count (ties to the lowest class where D3 = 16); with one
    valid row the kernel's own bf16 dlogits, dH2 and dH1 recovered bit for bit from the bias moments, each inside
    the oracle's interval and dH2, dH1 equal to the rounded exact sums of the kernel's own upstream, and the
    weight moments the singly rounded ``c1 d a``; one class: every gradient, moment and the loss exactly 0.
(b) one step at real learning rates (sgd, sgd + wd, adam, adam + wd) and Adam's second epoch from the state the
    same fit left after its first.
(c) ``lr = 0``, 2, 3 and 5 steps, the last one partial: the weights bit-equal, ``m`` and ``v`` the recursions over the
    per-step oracle gradients, also across the two epochs of one fit.
(d) real learning rate, random weights, 3 and 5 steps, sgd and sgd + wd: the relative update per tensor.
(e) an inactive peer, a peer without rows, 2 steps beside 5, 8 peers (slots 0 and 7), and the two shapes the gang
    cannot take: (1024, 10, 64) (LDS) and 9 peers (a capacity of 16 gangs of 17 workgroups is more than the 256 CUs
    hold, so the second block group of the launch never runs on this device; the test says so and stops).

Arithmetic-only mutations tried against this file on MI355X (none is in the tree), and the parts that caught each:

* ``k = t0 + t + 2`` in ``bias_corr``: (b), Adam and Adam + wd (``w'`` from the kernel's own moments), and (b)'s second epoch.
  Parts (a) and (c) run at ``lr = 0`` and cannot see it.
* ``upd`` without its weight-decay fma: (b), sgd + wd and adam + wd, and nothing else.
* the head's db2 loop stopping at ``BP - 1``: (a) at the shapes with a full 32- or 64-row batch ((784, 10, 32),
  (784, 10, 64), (1024, 10, 32)), (c) there, across two epochs and beside a shorter peer, (d) at (784, 10, 64).
* ``rows_at`` one short on a partial batch: (a), (b), (c) and (d) at every shape, and (e) (29 of the 31 tests).

Largest ``|error| / bound`` observed on MI355X per part: (a) 0.951 for the five tensors behind dlogits at every shape
(the read-out's half ulp where the radius is zero), b3 0.74 to 0.95; (b) sgd ``w`` 0.999, sgd + wd 0.997 (one fma's
half ulp), adam ``m`` 0.48, ``v`` 0.64, ``w`` 0.11, adam + wd ``m`` 0.57, ``v`` 0.71, ``w`` 0.11, the second epoch's ``w`` 0.90: ``bias_corr``'s
fp32 ``__powf`` stays inside the bound derived from one ulp, so the kernel keeps it; (c) ``m`` 0.94, ``v`` 0.92 (W1 and W2, the
biases below 0.8); (d) kernel / (8 floor) 0.125 (the kernel's error is the floor itself) for most tensors, 0.65 at
most (W1 of the 5-step peer of (776, 16, 40)); loss sums below 0.19 of ``loss_bound``.
"""

import threading

import numpy as np
import pytest
import torch

import _mlp_ref as M

pytestmark = pytest.mark.gpu

U, C1, C2 = M.U, M.C1, M.C2
GRAD_HP = dict(kind=0, lr=0.0)  # (a), (c): m = fl(c1 g), v = fl(c2 fl(g g)), the weights bit-equal
FILL = dict(m=0.25, v=0.75, shadow=3.0, w2t=5.0)


@pytest.fixture(scope="module")
def lib():
    from myfyp_amd.ops import _native

    return _native.load(required=True)


@pytest.fixture(autouse=True)
def bf16_settings(lib):
    from myfyp_amd.parallel.mlp_engine import MLPGroup
    from myfyp_amd.settings import Settings

    old = (Settings.MLP_PRECISION, Settings.GANG_WINDOW, Settings.USE_FUSED_KERNELS)
    Settings.MLP_PRECISION, Settings.GANG_WINDOW, Settings.USE_FUSED_KERNELS = "bf16", 5.0, True
    MLPGroup.reset_all()
    yield
    MLPGroup.reset_all()
    Settings.MLP_PRECISION, Settings.GANG_WINDOW, Settings.USE_FUSED_KERNELS = old


_CASES, _FITS = {}, {}  # cases and fits by configuration: computed once, never modified


def _case(*key):
    if key not in _CASES:
        _CASES[key] = M.case32(*key[:5], seed=key[5])
    return _CASES[key]


def _ckey(shape, n, family=None, seed=None):
    D0, D3, B = shape
    n = tuple(n)
    return (D0, D3, B, family or M.f32_family(D3), n, M.BF16_SEED.get((D0, D3, B, n), 0) if seed is None else seed)


def _spec(hp):
    if hp["kind"] == 0:
        return {"name": "adam", "lr": hp["lr"], "weight_decay": hp.get("wd", 0.0)}
    return {"name": "sgd", "lr": hp["lr"], "momentum": 0.0, "weight_decay": hp.get("wd", 0.0), "nesterov": False}


def _learners(peers, spec, B, empty=()):
    """``peers``: ``(case, peer of the case)`` per learner; ``empty``: the learners whose training split has no rows."""
    from myfyp_amd.learning.dataset.p2pfl_dataset import P2PFLDataset
    from myfyp_amd.learning.frameworks.torch import TorchLearner, TorchModel
    from myfyp_amd.models import MLP

    out = []
    for i, (c, p) in enumerate(peers):
        m = MLP(input_size=c["D"][0], out_channels=c["D"][3])
        with torch.no_grad():
            for j, l in enumerate(m.linear_layers()):
                l.weight.copy_(c["W"][p][f"W{j + 1}"])
                l.bias.copy_(c["W"][p][f"b{j + 1}"])
        m.optimizer_spec = lambda spec=spec: dict(spec)
        split = lambda x, y: {"image": np.ascontiguousarray(x.numpy()), "label": y.numpy().astype(np.int64)}
        rows = 0 if i in empty else c["n"][p]
        data = P2PFLDataset.from_arrays(split(c["x"][p][:rows], c["y"][p][:rows]), split(c["xt"][p], c["yt"][p]))
        out.append(TorchLearner(TorchModel(m), data, f"b{i}", batch_size=B))
    assert all(l._engine is not None for l in out), "bf16 engine not attached"
    return out


def _run(learners, who):
    # every fitting peer from its own thread: the group gangs the calls into one launch
    ts = [threading.Thread(target=learners[i].fit) for i in who]
    [t.start() for t in ts]
    [t.join() for t in ts]
    torch.cuda.synchronize()


def _fit(ckeys, hp, epochs=1, who=None, empty=(), count=None):
    """One fit of the peers of the cases ``ckeys`` (two each), the learners ``who`` fitting (default: all). Per learner the
    start weights and, after each epoch (the last entry: the end of the fit), the weights, ``m`` and ``v`` as float64
    dictionaries; the fit's loss sum and correct count as the device wrote them; ``idle``: whether every byte of its
    rows of ``params``, ``m``, ``v``, ``shadow`` and ``w2t`` survived the fit."""
    from myfyp_amd.parallel.mlp_engine import MLPGroup

    ckeys = ckeys if isinstance(ckeys[0], tuple) else (ckeys,)
    key = (ckeys, tuple(sorted(hp.items())), epochs, who, tuple(empty), count)
    if key in _FITS:
        return _FITS[key]
    dev = torch.device("cuda")
    peers = [(_case(*k), p) for k in ckeys for p in range(2)][:count]
    D, B = peers[0][0]["D"], peers[0][0]["B"]
    MLPGroup.reset_all()
    learners = _learners(peers, _spec(hp), B, empty)
    who = tuple(range(len(learners))) if who is None else who
    g = learners[0]._engine.group
    assert g.precision == "bf16" and g.uses_persistent()
    slots = [l._engine.slot for l in learners]
    n = [0 if i in empty else c["n"][p] for i, (c, p) in enumerate(peers)]
    g.expect(fit_slots={slots[i] for i in who})
    for name, val in FILL.items():
        getattr(g, name).fill_(val)
    before = {name: getattr(g, name).detach().clone() for name in ("params", *FILL)}
    snaps = []

    def perm_fn(ep):
        if ep:  # the state the epochs so far left (stream-ordered behind them)
            snaps.append(tuple(t.detach().clone() for t in (g.params, g.m, g.v)))
        out = torch.zeros(g.capacity, g.nmax, dtype=torch.int32)
        for i, (c, p) in enumerate(peers):
            if n[i]:
                out[slots[i], : n[i]] = torch.from_numpy(M.epoch_perm32(n[i], ep, p)).to(torch.int32)
        return out.to(dev)

    g.perm_fn = perm_fn
    for l in learners:
        l.set_epochs(epochs)
    sums, fetch = [], g._fetch

    def fetch_and_keep(k, with_conf):
        r = fetch(k, with_conf)
        sums.append((r[0].copy(), r[1].copy()))
        return r

    g._fetch = fetch_and_keep
    _run(learners, who)
    g.resolver.flush()  # the fit's sums are fetched by the resolver thread
    assert g.uses_persistent() and len(sums) == 1 and len(snaps) == epochs - 1
    snaps.append((g.params, g.m, g.v))
    after = {name: getattr(g, name).detach().clone() for name in ("params", *FILL)}
    numel = M.offsets(D)[1]
    rd = lambda t, s: M.unpack(t[s].detach().cpu().double()[:numel], D)
    out = []
    for i, (c, p) in enumerate(peers):
        s = slots[i]
        r = dict(w0=c["W"][p], ep=[dict(w=rd(sn[0], s), m=rd(sn[1], s), v=rd(sn[2], s)) for sn in snaps], loss=float(sums[0][0][s]), correct=int(sums[0][1][s]),
                 idle=all(torch.equal(before[k][s], after[k][s]) for k in before), n=n[i], slot=s)
        r.update(r["ep"][-1])
        what = f"{ckeys[i // 2]} learner {i}"
        if i in who and n[i] > 0:
            assert all(torch.isfinite(t).all() for k in ("w", "m", "v") for t in r[k].values()), f"{what}: not finite"
            row = after["params"][s, :numel]
            assert torch.equal(after["shadow"][s, :numel], row.to(torch.bfloat16)), f"{what}: shadow is not bf16(master)"
            assert (after["shadow"][s, numel:] == FILL["shadow"]).all(), f"{what}: the padding of the shadow row was written"
            w2 = M.unpack(row, D)["W2"].to(torch.bfloat16)
            assert torch.equal(after["w2t"][s], w2.t().contiguous().reshape(-1)), f"{what}: w2t is not the transposed bf16 W2"
            if hp["kind"] == 1:
                assert not after["m"][s, :numel].any(), f"{what}: SGD from fresh state left a non-zero m"
                assert torch.equal(after["v"][s], before["v"][s]), f"{what}: SGD touched v"
        else:
            assert r["idle"], f"{what}: an idle peer's state changed"
            assert r["loss"] == 0.0 and r["correct"] == 0, f"{what}: an idle peer has statistics"
        out.append(r)
    idle_slots = [s for s in range(g.capacity) if s not in slots]
    assert all(torch.equal(before[k][idle_slots], after[k][idle_slots]) for k in before), "a slot without a peer was written"
    _FITS[key] = out
    return out


def _within(what, got, ref, bound):
    err = (got - ref).abs()
    ratio = err / bound.clamp_min(1e-300)
    ratio = torch.where((err == 0) & (bound == 0), torch.zeros_like(err), ratio)
    worst = float(ratio.max()) if err.numel() else 0.0
    bad = err > bound
    if bad.any():
        i = int(ratio.flatten().argmax())
        pytest.fail(f"{what}: {int(bad.sum())} of {err.numel()} elements beyond the bound, worst at flat index {i}: got {float(got.flatten()[i])!r}, "
                    f"reference {float(ref.flatten()[i])!r}, error {float(err.flatten()[i]):.3e}, bound {float(bound.flatten()[i]):.3e}")
    return worst


def _bits(what, got, ref):
    bad = got != ref
    if bad.any():
        i = int(bad.flatten().nonzero()[0])
        pytest.fail(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at flat index {i}: got {float(got.flatten()[i])!r}, want {float(ref.flatten()[i])!r}")


def _f32(t):
    return t.float().double()


def _steps(c, p, epochs=1, n=None):
    """The oracle's steps of peer ``p`` with the weights frozen at the start: one ``step16`` per batch of every epoch."""
    out = []
    n = c["n"][p] if n is None else n
    for ep in range(epochs):
        perm = M.epoch_perm32(n, ep, p)
        for s in range(0, n, c["B"]):
            idx = torch.as_tensor(perm[s: s + c["B"]], dtype=torch.int64)
            out.append(M.step16(c["W"][p], c["x"][p][idx].double(), c["y"][p][idx].long()))
    return out


def _check_sums(what, r, steps):
    losses = torch.cat([s["loss"] for s in steps])
    want, bound = float(losses.sum()), M.loss_bound(losses, max(s["eps_lp"] for s in steps))
    print(f"{what}: loss sum {r['loss']!r}, float64 {want!r}, error / bound {abs(r['loss'] - want) / max(bound, 1e-300):.3f}")
    assert abs(r["loss"] - want) <= bound, f"{what}: loss sum {r['loss']!r}, float64 {want!r}, bound {bound:.3e}"
    correct = sum(int((s["pred"] == s["y"]).sum()) for s in steps)
    assert r["correct"] == correct, f"{what}: correct count {r['correct']}, the oracle's {correct}"


def _v_from_m(what, r):
    """``v = fl(c2 fl(g g))`` of the very ``g`` whose ``fl(c1 g)`` is the kernel's ``m`` (``_mlp_ref``: "Reading the gradient")."""
    for k in M.NAMES:
        want = C2 * (r["m"][k] / C1) ** 2
        _within(f"{what}: v of {k} from the kernel's own m", r["v"][k], want, M.SECOND * 4 * U * want + M.FLUSH32)


def _recover(what, m):
    """The bf16 vector ``d`` with ``fl(c1 d) == m``, bit for bit."""
    d = M.bf16(m / C1)
    _bits(f"{what}: no bf16 value d gives fl(c1 d) = m", m, _f32(C1 * d))
    return d


def _check_one_step(what, r, c, p, worst):
    """Part (a) for one peer of a one-step fit under ``GRAD_HP``."""
    D3, Bpad = c["D"][3], M.bpad(c["B"])
    (s,) = _steps(c, p)
    for k in M.NAMES:
        assert torch.equal(r["w"][k], r["w0"][k]), f"{what}: lr = 0 and {k} moved"
    _check_sums(what, r, [s])
    if D3 == 1:
        assert all(not r[x][k].any() for x in ("m", "v") for k in M.NAMES), f"{what}: one class and a non-zero moment"
        assert r["loss"] == 0.0, f"{what}: one class and a loss of {r['loss']!r}"
        return
    bnd = M.bounds16(s, Bpad)
    for k in M.NAMES:
        ref = C1 * s["g"][k]
        worst[k] = max(worst.get(k, 0.0), _within(f"{what} d{k}", r["m"][k], ref, C1 * bnd[k] + M.SECOND * U * (ref.abs() + C1 * bnd[k]) + M.FLUSH32))
        assert float(r["m"][k].abs().max()) > 0, f"{what}: d{k} is all zero"
    _v_from_m(what, r)
    if s["rows"] != 1:
        return
    W3, W2 = c["W"][p]["W3"], c["W"][p]["W2"]
    d3, d2, d1 = (_recover(f"{what} db{i}", r["m"][f"b{i}"]) for i in (3, 2, 1))
    for name, d, own in (("dlog", d3, None), ("dH2", d2, M.bf16((s["H2"][0] > 0) * (d3 @ W3))), ("dH1", d1, M.bf16((s["H1"][0] > 0) * (d2 @ W2)))):
        lo, hi = s[name + "_lo"][0], s[name + "_hi"][0]
        assert ((lo <= d) & (d <= hi)).all(), f"{what}: the kernel's {name} leaves the oracle's interval in {int(((d < lo) | (d > hi)).sum())} elements"
        if own is not None:
            _bits(f"{what}: {name} is not the rounded exact sum of the kernel's own upstream", d, own)
    for k, d, a in (("W3", d3, s["H2"][0]), ("W2", d2, s["H1"][0]), ("W1", d1, s["X"][0])):
        _bits(f"{what}: m of {k} is not fl(c1 d a)", r["m"][k], _f32(C1 * (d[:, None] * a[None, :])))


# ---------------------------------------------------------------------------------------------
# (a) one step: the gradients per element
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", M.BF16_SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_one_step_gradients_per_element(lib, shape):
    """Valid rows 1, 2, 31, 32, 33, 63, 64 as far as B allows (B = 40: 1, 2, 39, 40; B = 48: 1, 2, 33, 48), two peers
    per fit (module docstring, (a))."""
    worst = {}
    for n in M.BF16_ONE_STEP[shape[2]]:
        key = _ckey(shape, n)
        for p, r in enumerate(_fit(key, GRAD_HP)):
            _check_one_step(f"{shape} peer {p} rows {n[p]}", r, _case(*key), p, worst)
    print(f"{shape}: largest error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


# ---------------------------------------------------------------------------------------------
# (b) one step at real learning rates
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(M.BF16_OPT))
def test_one_step_of_every_optimizer_variant(lib, variant):
    """Rows 31 and 33 of (784, 10, 64) on the grid. SGD: ``w'`` from the oracle gradient with its radius through ``upd32`` (the
    weight-decay fma included). Adam: ``m'`` and ``v'`` from the oracle gradient through ``adam_moments16``, ``w'`` from the kernel's own
    new moments through ``adam_w32``'s tail with ``adam_coeffs16`` at step 1."""
    hp = M.BF16_OPT[variant]
    shape, n = M.BF16_OPT_CASE
    key = _ckey(shape, n)
    c = _case(*key)
    worst = {}
    for p, r in enumerate(_fit(key, hp)):
        (s,) = _steps(c, p)
        bnd = M.bounds16(s, M.bpad(shape[2]))
        for k in M.NAMES:
            what = f"{variant} peer {p} {k}"
            w0, zero = r["w0"][k], torch.zeros_like(r["w0"][k])
            if hp["kind"] == 1:
                w1, _, _, bw, _, _ = M.upd32(hp, w0, s["g"][k], zero, zero, 1, dg=bnd[k])
            else:
                m1, v1, bm, bv = M.adam_moments16(hp, w0, s["g"][k], bnd[k], zero, zero, zero, zero)
                worst["m"] = max(worst.get("m", 0.0), _within(f"{what}: m", r["m"][k], m1, bm))
                worst["v"] = max(worst.get("v", 0.0), _within(f"{what}: v", r["v"][k], v1, bv))
                w1, bw = M.adam_w32(hp, w0, r["m"][k], r["v"][k], 1, coeffs=M.adam_coeffs16(hp, 1))
            worst["w"] = max(worst.get("w", 0.0), _within(f"{what}: w", r["w"][k], w1, bw))
            assert not torch.equal(r["w"][k], w0), f"{what}: the weights did not move"
        _check_sums(f"{variant} peer {p}", r, [s])
    print(f"{variant}: largest error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def test_adam_second_epoch_uses_its_own_step_count(lib):
    """Two one-step epochs of one Adam fit (the second: ``fresh = 0``, ``t0 = 1``): the final weights against ``adam_w32``'s tail at
    optimizer step 2 with ``adam_coeffs16`` applied to the kernel's own final moments and the weights the same fit held
    after its first epoch. At step 1's or step 3's coefficients the update is 1.9 or 0.7 times as large."""
    hp = M.BF16_OPT["adam"]
    shape, n = M.BF16_OPT_CASE
    worst = 0.0
    for p, r in enumerate(_fit(_ckey(shape, n), hp, epochs=2)):
        for k in M.NAMES:
            first, last = r["ep"][0], r["ep"][1]
            assert not torch.equal(first["w"][k], r["w0"][k]) and not torch.equal(first["m"][k], last["m"][k])
            w2, bw = M.adam_w32(hp, first["w"][k], last["m"][k], last["v"][k], 2, coeffs=M.adam_coeffs16(hp, 2))
            worst = max(worst, _within(f"peer {p} {k}", last["w"][k], w2, bw))
            upd = (w2 - first["w"][k]).abs()
            assert float((bw / upd.clamp_min(1e-300)).median()) < 2.0 ** -10, "a bound that cannot tell step 2 from step 1"
    print(f"second epoch: largest error / bound {worst:.3f}")


# ---------------------------------------------------------------------------------------------
# (c) several steps with the weights frozen
# ---------------------------------------------------------------------------------------------
def _frozen(shape, n, epochs=1):
    key = _ckey(shape, n)
    c = _case(*key)
    for p, r in enumerate(_fit(key, GRAD_HP, epochs=epochs)):
        what = f"{shape} peer {p} n {n[p]} epochs {epochs}"
        steps = _steps(c, p, epochs=epochs)
        assert len(steps) == epochs * -(-n[p] // shape[2])
        _check_sums(what, r, steps)
        if shape[1] == 1:
            assert all(not r[x][k].any() for x in ("m", "v") for k in M.NAMES) and r["loss"] == 0.0, f"{what}: one class"
            continue
        bnds = [M.bounds16(s, M.bpad(shape[2])) for s in steps]
        ratios = {}
        for k in M.NAMES:
            assert torch.equal(r["w"][k], r["w0"][k]), f"{what}: lr = 0 and {k} moved"
            m, v, bm, bv = M.moments16(GRAD_HP, r["w0"][k], [s["g"][k] for s in steps], [b[k] for b in bnds])
            ratios[k] = (_within(f"{what} m of {k}", r["m"][k], m, bm), _within(f"{what} v of {k}", r["v"][k], v, bv))
        print(f"{what}: largest error / bound (m, v) " + ", ".join(f"{k} {a:.3f} {b:.3f}" for k, (a, b) in ratios.items()))


@pytest.mark.parametrize("shape", M.BF16_SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_frozen_weights_every_step_per_element(lib, shape):
    """``lr = 0``: every step's forward stays on the grid. 2, 3 and 5 steps with the last batch partial (peer 0) and full (peer
    1) at the two main shapes, 3 steps elsewhere: Adam's ``m`` and ``v`` are the beta recursions over the per-step oracle
    gradients with their radii (``moments16``); the loss sum and the correct count of the epoch."""
    pairs = M.BF16_STEPS[shape[2]]
    for n in pairs if shape in M.BF16_MAIN else pairs[1:2]:
        _frozen(shape, n)


def test_frozen_weights_moments_carry_over_epochs(lib):
    """Two epochs of one fit at ``lr = 0``, 3 steps each in other orders: the recursion over the six steps."""
    _frozen(M.BF16_MAIN[1], M.BF16_STEPS[64][1], epochs=2)


# ---------------------------------------------------------------------------------------------
# (d) real learning rates
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hp", list(M.BF16_LEARN_HP))
@pytest.mark.parametrize("shape", M.BF16_LEARN_SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_learning_epoch_within_the_oracles_sensitivity(lib, shape, hp):
    """``randn16`` weights, SGD and SGD + weight decay, 3 steps (peer 0) and 5 steps (peer 1), the last batch partial: the
    relative update error of each tensor against the float64 epoch with the kernel's bf16 roundings, within 8 times
    the fp32 twin's (both printed)."""
    key = _ckey(shape, M.BF16_LEARN[shape[2]], "randn16", M.BF16_LEARN_SEED.get(shape, 0))
    c = _case(*key)
    bad = []
    for p, r in enumerate(_fit(key, M.BF16_LEARN_HP[hp])):
        ref, alt = M.learn_refs16(c, p, M.BF16_LEARN_HP[hp])
        for k in M.NAMES:
            floor, rel = M.rel_update(alt[k], ref[k], r["w0"][k]), M.rel_update(r["w"][k], ref[k], r["w0"][k])
            print(f"{shape} {hp} peer {p} {k}: oracle floor {floor:.3e}, kernel {rel:.3e}, kernel / (8 floor) {rel / (8 * floor):.3f}")
            assert 8 * floor <= 1e-2
            if not rel <= 8 * floor:
                bad.append((p, k, rel, floor))
    assert not bad, bad


# ---------------------------------------------------------------------------------------------
# (e) edges
# ---------------------------------------------------------------------------------------------
def test_fewer_steps_than_the_neighbour(lib):
    """33 rows beside 150 at B = 32: 2 steps (the second one row) beside 5. Part (c)'s checks on both peers."""
    _frozen(*M.BF16_EDGE)


@pytest.mark.parametrize("idle", ["inactive", "no_rows"])
def test_an_idle_peer_keeps_every_byte(lib, idle):
    """Peer 1 does not fit (``ctl.x = 0``), or fits without a single training row (``ctl.y = 0``): every byte of its ``params``, ``m``, ``v``,
    ``shadow`` and ``w2t`` rows is unchanged, its loss sum and correct count are 0 (asserted in ``_fit``); peer 0 beside it passes
    part (a)."""
    shape = M.BF16_SHAPES[0]
    key = _ckey(shape, M.BF16_ONE_STEP[32][1])
    fit = _fit(key, GRAD_HP, who=(0,)) if idle == "inactive" else _fit(key, GRAD_HP, empty=(1,))
    assert fit[1]["idle"] and not fit[0]["idle"]
    _check_one_step(f"{shape} beside an idle peer ({idle})", fit[0], _case(*key), 0, {})


def test_eight_peers_fill_the_first_block_group(lib):
    """8 peers at (40, 16, 24), 23 and 24 rows, four cases of two peers: part (a) on slots 0 and 7."""
    keys = tuple(_ckey(M.BF16_GANG, M.BF16_GANG_ROWS, seed=s) for s in M.BF16_GANG_SEEDS[:4])
    fit = _fit(keys, GRAD_HP)
    assert sorted(r["slot"] for r in fit) == list(range(8))
    worst = {}
    for i in (0, 7):
        j = next(j for j, r in enumerate(fit) if r["slot"] == i)
        _check_one_step(f"{M.BF16_GANG} slot {i}", fit[j], _case(*keys[j // 2]), j % 2, worst)
    print("8 peers: largest error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def test_shapes_the_gang_cannot_take(lib):
    """(1024, 10, 64): the owner's X tile exceeds the LDS limit. 9 peers: the capacity doubles to 16 and 16 gangs of 17
    workgroups must be co-resident, one per CU: more than the device has, so the engine takes the step path and
    the launch's second block group (``p >= 8``) never runs here. Both are the engine's decision, stated, not skipped."""
    from myfyp_amd.parallel.mlp_engine import MLPGroup

    c = _case(*_ckey((1024, 10, 64), (4, 4)))
    learners = _learners([(c, 0), (c, 1)], _spec(GRAD_HP), 64)
    g = learners[0]._engine.group
    assert g.precision == "bf16" and not g.uses_persistent()
    MLPGroup.reset_all()
    keys = [_ckey(M.BF16_GANG, M.BF16_GANG_ROWS, seed=s) for s in M.BF16_GANG_SEEDS]
    peers = [(_case(*k), p) for k in keys for p in range(2)][:9]
    learners = _learners(peers, _spec(GRAD_HP), M.BF16_GANG[2])
    g = learners[0]._engine.group
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert g.precision == "bf16" and g.capacity == 16 and sorted(l._engine.slot for l in learners) == list(range(9))
    assert g.uses_persistent() == (17 * g.capacity <= cus), f"capacity {g.capacity}, {cus} CUs"
    if g.uses_persistent():  # a device that holds 16 gangs: part (a) on slots 0, 7 and 8
        fit = _fit(tuple(keys), GRAD_HP, count=9)
        for i in (0, 7, 8):
            j = next(j for j, r in enumerate(fit) if r["slot"] == i)
            _check_one_step(f"{M.BF16_GANG} slot {i} of 9", fit[j], _case(*keys[j // 2]), j % 2, {})
