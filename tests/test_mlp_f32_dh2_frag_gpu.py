"""dH2 handed from the heads to the owners in MFMA fragment order in the fp32 epoch kernel
(csrc/kernels/mlp_persistent_f32.hip, layout 1): with ``mlp_set_f32_dh2_frag(1)`` /
``MYFYP_F32_DH2_FRAG=1`` head ``hd`` publishes its 16 dH2 columns as ``dh2f[parity][hd][mt][lane]``, one
``float4`` per lane holding ``dH2[16 mt + c][16 hd + 4h .. 4h + 3]`` (``h = lane >> 4``, ``c = lane & 15``):
the A operands of owner wave ``hd``'s four dH1 MFMAs on batch tile ``mt``. The owners' C1 loads them
straight into registers instead of staging the ``[b][128]`` tile through LDS, and the deferred W2-replica
update reads the same image. The values entering every MFMA and their order do not change, so every
parameter and optimizer moment after a fit must be bit-identical with the switch at 1 and at 0.
Layouts 2 and 3 keep the tile: the launch reports mode 0 there.

Small shapes: 2 peers (3 for the retry case), at most 300 samples per peer. The mode-0 fit of a shape is
computed once and shared by the cases that compare against it.
"""

import pytest
import torch

from _mlp_f32_fit import _all, _assert_same, _pin_perms, _setup, _torch_reference, dev, fp32_settings, lib  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

ADAM = {"name": "adam", "lr": 1e-3}
SGDM = {"name": "sgd", "lr": 1e-4, "momentum": 0.9}
PROX = {"name": "sgd", "lr": 1e-3, "momentum": 0.9}  # (the FedProx spec of test_mlp_f32_gpu.py)
# samples per peer that give 1, 2 and 5 steps per epoch, the last batch partial (B 64 also 3 steps: 150)
PER_PEER = {64: [40, 100, 150, 300], 32: [20, 50, 150], 24: [20, 40, 110]}


_REF = {}  # mode-0 fits, by shape


def _run(lib, dev, mode, P, B, per_peer, spec, D0=784, ks=1, variant=1, epochs=2, seed=21, giveup=None, torch_ref=False, prox=False, w2chk=False):
    """One seeded fit with the switch at `mode`: every peer's flat parameters, the moments the engine
    keeps across the fit's epochs, the recovery count and what the launch reported. `prox`: one FedProx
    epoch (anchors a fixed perturbation of the initial weights). `w2chk`: also the owners' W2 replica
    after the last epoch and the heads' W2. `torch_ref`: also the largest relative update error of any
    parameter tensor against fp32 autograd + torch.optim.Adam on the same batches (`rel`), and that
    reference's own error: the same measure between it and the same torch run in fp64 (`ref_err`)."""
    from myfyp_amd.ops import _native
    from myfyp_amd.parallel.mlp_engine import MLPGroup

    lib.mlp_set_f32_dh2_frag(mode)
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
    try:
        _all(learners, "fit", extras)
    finally:
        if w2chk:
            with g.lock:
                lib.mlp_engine_set_w2chk(g._engine, None)
    _all(learners, "evaluate")  # results fetched: give-up status checked
    assert g.f32_ks() == ks and g.f32_variant() == variant, (g.f32_ks(), g.f32_variant())
    slots = [l._engine.slot for l in learners]
    out = {
        "params": [l.flat_params().detach().clone() for l in learners],
        "m": [g.m[s].detach().clone() for s in slots],
        "v": [g.v[s].detach().clone() for s in slots],
        "recoveries": g.recoveries(),
        "frag": lib.mlp_f32_dh2_frag_last(),
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


@pytest.mark.parametrize("B,per_peer", [(B, n) for B in (64, 32, 24) for n in PER_PEER[B]])
@pytest.mark.parametrize("spec", [ADAM, SGDM], ids=["adam", "sgdm"])
def test_dh2_frag_bit_identical_to_mode0(lib, dev, spec, B, per_peer):
    """D0 = 784 (fused forward, the K24 kernel), two epochs, 2 peers. B 64 and B 32 (Bpad 32: two batch
    tiles), and B 24, whose Bpad is 32 too, so that every step leaves rows past the batch inside the last
    tile (they are zero in the image as in the tile). Per epoch 1, 2 and 5 steps, the last one partial:
    one step never runs the deferred replica update, two run it once (B 64 also 150 samples: 64, 64, 22)."""
    on = _run(lib, dev, 1, 2, B, per_peer, spec)
    assert on["frag"] == 1, f"mode 1 asked for, the launch reported {on['frag']}"
    _assert_same(on, _mode0(lib, dev, 2, B, per_peer, spec), spec["name"] == "adam")


@pytest.mark.parametrize("B", [64, 32])
@pytest.mark.parametrize("spec", [ADAM, SGDM], ids=["adam", "sgdm"])
def test_dh2_frag_narrow_input(lib, dev, spec, B):
    """D0 = 96: four K steps, so half of every owner's waves have none, C2 runs its guarded body and there
    is no K step 24. 150 samples: 3 steps at B 64, 5 at B 32."""
    on = _run(lib, dev, 1, 2, B, 150, spec, D0=96)
    assert on["frag"] == 1, f"mode 1 asked for, the launch reported {on['frag']}"
    _assert_same(on, _mode0(lib, dev, 2, B, 150, spec, D0=96), spec["name"] == "adam")


@pytest.mark.parametrize("B,ks", [(64, 2), (32, 2), (64, 4), (64, 8)])
def test_dh2_frag_k_splits(lib, dev, B, ks):
    """Owner K split 2 and the cross-XCD splits 4 / 8 (instantiated for the 64-row tile), selected as in
    test_mlp_f32_gpu.py: the heads' image is written through to every XCD, every owner of a column group
    loads the same fragments. (K split 1 is every other case of this file.)"""
    on = _run(lib, dev, 1, 2, B, 150, ADAM, ks=ks)
    assert on["frag"] == 1, f"mode 1 asked for, the launch reported {on['frag']}"
    _assert_same(on, _mode0(lib, dev, 2, B, 150, ADAM, ks=ks), True)


def test_dh2_frag_fedprox_on_layout1(lib, dev):
    """FedProx (SGD with momentum) forced onto layout 1: the instantiations with the extra gradient term."""
    on = _run(lib, dev, 1, 2, 64, 150, PROX, prox=True)
    assert on["frag"] == 1, f"mode 1 asked for, the launch reported {on['frag']}"
    _assert_same(on, _mode0(lib, dev, 2, 64, 150, PROX, prox=True), False)


def test_dh2_frag_giveup_recovered_by_retry_launch(lib, dev):
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
def test_dh2_frag_w2_replica_is_bit_identical(lib, dev, B, per_peer):
    """The owners' W2 replica, updated from dH2 re-read out of the fragment image, equals the heads' W2
    bit for bit after 2 and after 5 steps (one epoch; the debug write-back runs the last deferred update)."""
    on = _run(lib, dev, 1, 2, B, per_peer, ADAM, epochs=1, w2chk=True)
    assert on["frag"] == 1, f"mode 1 asked for, the launch reported {on['frag']}"
    for i, (rep, w2) in enumerate(zip(on["replica"], on["w2"])):
        assert torch.isfinite(rep).all(), f"peer {i}: the replica was not written"
        assert torch.equal(rep, w2), f"peer {i}: {int((rep != w2).sum())} replica elements differ from the heads' W2"


@pytest.mark.parametrize("B", [64, 32])
def test_dh2_frag_matches_torch_adam(lib, dev, B):
    """One Adam case per Bpad against fp32 autograd + torch.optim.Adam on the same batches, relative
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


@pytest.mark.parametrize("B", [64, 32])
def test_dh2_frag_layout3_keeps_the_tile(lib, dev, B):
    """Layout 3 (row heads) keeps the staged tile: with mode 1 asked for the launch reports 0, and the fit
    equals the one with mode 0 asked for bit for bit."""
    on = _run(lib, dev, 1, 2, B, 150, ADAM, variant=3)
    assert on["frag"] == 0, f"layout 3, mode 1 asked for: the launch reported {on['frag']}"
    _assert_same(on, _mode0(lib, dev, 2, B, 150, ADAM, variant=3), True)
