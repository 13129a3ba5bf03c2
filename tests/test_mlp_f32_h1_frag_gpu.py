"""H1 handed from the owners to the heads in MFMA fragment order in the fp32 epoch kernel
(csrc/kernels/mlp_persistent_f32.hip, layout 1, K split 1, fused forward): with ``mlp_set_f32_h1_frag(1)`` /
``MYFYP_F32_H1_FRAG=1`` owner ``g`` publishes its 16 H1 columns as ``h1f[parity][g][mt][lane]``, one ``float4``
per lane holding ``H1[16 mt + c][16 g + 4h .. 4h + 3]`` (``h = lane >> 4``, ``c = lane & 15``), head wave
``g / 2`` loads them straight into the registers of its H2 MFMAs, and the heads accumulate H2 and dH2
transposed (the MFMA's two operands swapped), so that the partial logits run from registers and dH2 is the
owners' fragment as it leaves the MFMA. The values entering every MFMA and their order do not change, so
every parameter, every optimizer moment and the epoch's loss and accuracy sums must be bit-identical with
the switch at 1 and at 0 (the loss sum because the heads add their waves' sums in wave order with one
atomicAdd per epoch; one per wave landed in arrival order and differed in the last bits from run to run:
1352.1985 against 1352.1982 in the first run of this file). The mode is a template argument of the kernel: K splits > 1, layouts 2 and 3,
extra-term epochs and launches with the dH2 fragment image switched off keep the row image, and the
launch reports mode 0 there.

Small shapes: 2 peers (3 for the retry case), at most 300 samples per peer. The mode-0 fit of a shape is
computed once and shared by the cases that compare against it.
"""

import numpy as np
import pytest
import torch

from _mlp_f32_fit import _all, _keep_fit_sums, _pin_perms, _setup, _torch_reference, dev, fp32_settings, lib  # noqa: F401 (fixtures)
from _mlp_f32_fit import _assert_same as _same_core

pytestmark = pytest.mark.gpu

ADAM = {"name": "adam", "lr": 1e-3}
SGDM = {"name": "sgd", "lr": 1e-4, "momentum": 0.9}
PROX = {"name": "sgd", "lr": 1e-3, "momentum": 0.9}  # (the FedProx spec of test_mlp_f32_gpu.py)
# samples per peer that give 1, 2, 3 and 5 steps per epoch, the last batch partial
PER_PEER = {64: [40, 100, 150, 300], 32: [20, 50, 80, 150], 24: [20, 40, 60, 110]}


_REF = {}  # mode-0 fits, by shape


def _run(lib, dev, mode, P, B, per_peer, spec, D0=784, ks=1, variant=1, epochs=2, seed=21, dh2=-1, giveup=None, torch_ref=False, prox=False, w2chk=False):
    """One seeded fit with the switch at `mode` (and the dH2 switch at `dh2`; -1: its default, on): every
    peer's flat parameters, the moments the engine keeps across the fit's epochs, the fit's loss and
    accuracy sums as the kernel accumulated them, the recovery count and what the launch reported.
    `prox`: one FedProx epoch (anchors a fixed perturbation of the initial weights). `w2chk`: also the
    owners' W2 replica after the last epoch and the heads' W2. `torch_ref`: also the largest relative
    update error of any parameter tensor against fp32 autograd + torch.optim.Adam on the same batches
    (`rel`), and that reference's own error: the same measure between it and the same torch run in fp64
    (`ref_err`)."""
    from myfyp_amd.ops import _native
    from myfyp_amd.parallel.mlp_engine import MLPGroup

    lib.mlp_set_f32_h1_frag(mode)
    lib.mlp_set_f32_dh2_frag(dh2)
    MLPGroup.reset_all()
    learners, refs, g, n = _setup(dev, P, B, per_peer, seed, spec, D0, ks, variant)
    perms = _pin_perms(dev, g, learners, n)
    p0 = [[p.detach().clone() for p in l.model.get_model().parameters()] for l in learners]
    for l in learners:
        l.set_epochs(epochs)
    if giveup is not None:
        g.debug_giveup(learners[giveup[0]]._engine.slot, at_end=giveup[1])
    extras = None
    if prox:
        gen = torch.Generator(device="cpu").manual_seed(9)
        extras = [{"anchor": (f + 0.01 * torch.randn(f.shape, generator=gen).to(dev)).contiguous(), "mu": 0.5} for f in (l.flat_params().detach() for l in learners)]
    chk = None
    if w2chk:
        chk = torch.full((g.capacity, 128, 256), float("nan"), device=dev)
        with g.lock:
            g._ensure_engine()
            _native.check(lib.mlp_engine_set_w2chk(g._engine, chk.data_ptr()), "set_w2chk")
    sums = _keep_fit_sums(g)
    try:
        _all(learners, "fit", extras)
    finally:
        if w2chk:
            with g.lock:
                lib.mlp_engine_set_w2chk(g._engine, None)
    _all(learners, "evaluate")  # results fetched: give-up status checked
    assert g.f32_ks() == ks and g.f32_variant() == variant, (g.f32_ks(), g.f32_variant())
    assert len(sums) == 1, f"{len(sums)} fit results fetched"
    slots = [l._engine.slot for l in learners]
    out = {
        "params": [l.flat_params().detach().clone() for l in learners],
        "m": [g.m[s].detach().clone() for s in slots],
        "v": [g.v[s].detach().clone() for s in slots],
        "loss": [sums[0][0][s] for s in slots],
        "correct": [int(sums[0][1][s]) for s in slots],
        "recoveries": g.recoveries(),
        "frag": lib.mlp_f32_h1_frag_last(),
    }
    if giveup is not None:
        g.debug_giveup(None)
    if w2chk:
        off_w2 = 256 * D0 + 256
        out["replica"] = [chk[s].clone() for s in slots]
        out["w2"] = [g.params[s, off_w2 : off_w2 + 128 * 256].view(128, 256).clone() for s in slots]
    if torch_ref:
        out["rel"], out["ref_err"] = _torch_reference(learners, refs, p0, perms, B, spec, epochs)
    return out


def _mode0(lib, dev, P, B, per_peer, spec, **kw):
    """The mode-0 fit of a shape, computed once; never modified."""
    key = (P, B, per_peer, spec["name"], spec["lr"]) + tuple(sorted(kw.items()))
    if key not in _REF:
        _REF[key] = _run(lib, dev, 0, P, B, per_peer, spec, **kw)
        assert _REF[key]["frag"] == 0, f"mode 0 asked for, the launch reported {_REF[key]['frag']}"
    return _REF[key]


def _assert_same(a, b, adam, loss_bits=True):
    """Bit-equal parameters, moments, loss sums and correct counts. `loss_bits=False` (layouts 2 and 3,
    where both runs take the same kernel): the loss sum within 2^-20 relative, as those layouts add it up
    with one float atomicAdd per wave or workgroup, in arrival order: at most 16 additions of positive
    terms, each rounding by at most 2^-24 of the sum."""
    _same_core(a, b, adam)
    for i, (x, y) in enumerate(zip(a["loss"], b["loss"])):
        assert np.isfinite(x) and x > 0, f"peer {i}: loss sum {x}"
        if loss_bits:
            assert x.tobytes() == y.tobytes(), f"peer {i}: loss sums {x!r} and {y!r}"
        else:
            assert abs(float(x) - float(y)) <= 2.0**-20 * float(x), f"peer {i}: loss sums {x!r} and {y!r}"
    assert a["correct"] == b["correct"], (a["correct"], b["correct"])


@pytest.mark.parametrize("B,per_peer", [(B, n) for B in (64, 32, 24) for n in PER_PEER[B]])
@pytest.mark.parametrize("spec", [ADAM, SGDM], ids=["adam", "sgdm"])
def test_h1_frag_bit_identical_to_mode0(lib, dev, spec, B, per_peer):
    """D0 = 784 (the K24 kernel), two epochs, 2 peers. B 64 and B 32 (Bpad 32: two batch tiles), and B 24,
    whose Bpad is 32 too, so that every step leaves rows past the batch inside the last tile (zero in the
    image as in the row image). Per epoch 1, 2, 3 and 5 steps, the last one partial: one step publishes
    H1 from the prologue only, two and more also from C2."""
    on = _run(lib, dev, 1, 2, B, per_peer, spec)
    assert on["frag"] == 1, f"mode 1 asked for, the launch reported {on['frag']}"
    _assert_same(on, _mode0(lib, dev, 2, B, per_peer, spec), spec["name"] == "adam")


@pytest.mark.parametrize("B,last", [(64, 1), (64, 15), (64, 17), (64, 33), (64, 63), (32, 1), (32, 17)])
def test_h1_frag_row_mask(lib, dev, B, last):
    """Two steps per epoch, the second with `last` rows: with H2 transposed the row mask is taken from the
    lane's c (row 16 mt + c), no longer from the accumulator index (row 16 mt + 4h + i). Row counts on
    both sides of the tile boundaries and one row short of the batch."""
    on = _run(lib, dev, 1, 2, B, B + last, ADAM)
    assert on["frag"] == 1, f"mode 1 asked for, the launch reported {on['frag']}"
    _assert_same(on, _mode0(lib, dev, 2, B, B + last, ADAM), True)


@pytest.mark.parametrize("D0", [736, 768, 792])
@pytest.mark.parametrize("spec", [ADAM, SGDM], ids=["adam", "sgdm"])
def test_h1_frag_input_width(lib, dev, spec, D0):
    """D0 = 736: 24 K steps, the kernel without a register-resident K step 24; 768 and 792: with it
    (the bias column alone in K step 24, and beside 24 input columns). 150 samples: 3 steps."""
    on = _run(lib, dev, 1, 2, 64, 150, spec, D0=D0)
    assert on["frag"] == 1, f"mode 1 asked for, the launch reported {on['frag']}"
    assert lib.mlp_f32_k24_last() == (1 if D0 >= 768 else 0)
    _assert_same(on, _mode0(lib, dev, 2, 64, 150, spec, D0=D0), spec["name"] == "adam")


def test_h1_frag_giveup_recovered_by_retry_launch(lib, dev):
    """3 peers, mode 1. The engine's bounded-wait test hook makes one peer's gang give up on its first
    attempt: the retry launch reproduces the unforced fit bit for bit, moments included, and both equal
    the mode-0 fit."""
    ok = _run(lib, dev, 1, 3, 64, 300, ADAM, epochs=1)
    rec = _run(lib, dev, 1, 3, 64, 300, ADAM, epochs=1, giveup=(1, False))
    assert ok["recoveries"] == 0 and rec["recoveries"] == 1, (ok["recoveries"], rec["recoveries"])
    assert ok["frag"] == rec["frag"] == 1, (ok["frag"], rec["frag"])
    _assert_same(ok, rec, True)
    _assert_same(ok, _mode0(lib, dev, 3, 64, 300, ADAM, epochs=1), True)


@pytest.mark.parametrize("B,per_peer", [(64, 100), (64, 300), (32, 50), (32, 150)])
def test_h1_frag_w2_replica_is_bit_identical(lib, dev, B, per_peer):
    """The owners' W2 replica (updated from their own H1 slice and the dH2 fragments) equals the heads' W2
    (updated from the H1 fragments the heads stored themselves and their transposed dH2) bit for bit
    after 2 and after 5 steps (one epoch; the debug write-back runs the last deferred update)."""
    on = _run(lib, dev, 1, 2, B, per_peer, ADAM, epochs=1, w2chk=True)
    assert on["frag"] == 1, f"mode 1 asked for, the launch reported {on['frag']}"
    for i, (rep, w2) in enumerate(zip(on["replica"], on["w2"])):
        assert torch.isfinite(rep).all(), f"peer {i}: the replica was not written"
        assert torch.equal(rep, w2), f"peer {i}: {int((rep != w2).sum())} replica elements differ from the heads' W2"


@pytest.mark.parametrize("B", [64, 32, 24])
def test_h1_frag_matches_torch_adam(lib, dev, B):
    """One Adam case per B against fp32 autograd + torch.optim.Adam on the same batches, relative
    update error < 1e-3 (the bound of test_f32_epoch_matches_torch_adam), run twice: equal bits.

    The data seed is the first of 21, 22, ... at which that reference reproduces itself (the rule of
    test_mlp_f32_k24_gpu.py): the same torch run in fp64 must agree with the fp32 one to 1e-4, a tenth
    of the bound, so that the reference's own rounding cannot use the bound up. The criterion looks at
    torch alone, never at the kernel's result."""
    for seed in (21, 22, 23, 24):
        on = _run(lib, dev, 1, 2, B, 300, ADAM, seed=seed, torch_ref=True)
        print(f"B {B} seed {seed}: relative update error vs fp32 torch {on['rel']:.3e}, fp32 torch vs fp64 torch {on['ref_err']:.3e}")
        if on["ref_err"] < 1e-4:
            break
    else:
        pytest.fail(f"B {B}: no data seed with a reproducible fp32 reference")
    assert on["frag"] == 1, f"mode 1 asked for, the launch reported {on['frag']}"
    again = _run(lib, dev, 1, 2, B, 300, ADAM, seed=seed)
    _assert_same(on, again, True)
    _assert_same(on, _mode0(lib, dev, 2, B, 300, ADAM, seed=seed), True)
    assert on["rel"] < 1e-3, f"B {B}: relative update error {on['rel']:.2e}"


@pytest.mark.parametrize("B,ks", [(64, 2), (32, 2), (64, 4), (64, 8)])
def test_h1_frag_k_splits_keep_the_row_image(lib, dev, B, ks):
    """Owner K split 2 and the cross-XCD splits 4 / 8: the K parts' partial slices are summed row by row,
    the row image stays. Mode 1 asked for: the launch reports 0 and equals the mode-0 fit."""
    on = _run(lib, dev, 1, 2, B, 150, ADAM, ks=ks)
    assert on["frag"] == 0, f"K split {ks}, mode 1 asked for: the launch reported {on['frag']}"
    _assert_same(on, _mode0(lib, dev, 2, B, 150, ADAM, ks=ks), True)


@pytest.mark.parametrize("variant", [2, 3])
@pytest.mark.parametrize("B", [64, 32])
def test_h1_frag_layouts_2_and_3_keep_the_row_image(lib, dev, B, variant):
    """Layout 2 (owners only) and layout 3 (row heads): mode 1 asked for, the launch reports 0, and the fit
    equals the one with mode 0 asked for bit for bit."""
    on = _run(lib, dev, 1, 2, B, 150, ADAM, variant=variant)
    assert on["frag"] == 0, f"layout {variant}, mode 1 asked for: the launch reported {on['frag']}"
    _assert_same(on, _mode0(lib, dev, 2, B, 150, ADAM, variant=variant), True, loss_bits=False)


def test_h1_frag_fedprox_on_layout1_keeps_the_row_image(lib, dev):
    """FedProx (SGD with momentum) forced onto layout 1: the instantiations with the extra gradient term
    have no fragment form."""
    on = _run(lib, dev, 1, 2, 64, 150, PROX, prox=True)
    assert on["frag"] == 0, f"extra-term epoch, mode 1 asked for: the launch reported {on['frag']}"
    _assert_same(on, _mode0(lib, dev, 2, 64, 150, PROX, prox=True), False)


@pytest.mark.parametrize("B", [64, 32])
def test_h1_frag_needs_the_dh2_fragments(lib, dev, B):
    """mlp_set_f32_dh2_frag(0) with H1 mode 1: the fragment kernels have the dH2 fragment path compiled
    in, so the launch takes the row-image kernels, reports 0 and equals the run with both switches off."""
    on = _run(lib, dev, 1, 2, B, 150, ADAM, dh2=0)
    assert on["frag"] == 0 and lib.mlp_f32_dh2_frag_last() == 0, (on["frag"], lib.mlp_f32_dh2_frag_last())
    _assert_same(on, _mode0(lib, dev, 2, B, 150, ADAM, dh2=0), True)
