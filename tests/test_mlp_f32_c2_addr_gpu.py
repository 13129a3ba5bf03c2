"""The input width as a compile-time constant of the fp32 epoch kernel (csrc/kernels/mlp_persistent_f32.hip,
owner32's ``D0C``; ``mlp_set_f32_static_d0`` / ``MYFYP_F32_STATIC_D0``). At D0 = 784 the launch that takes the
fused K24 fragment kernels takes the instantiation built for that width: the X tile's row strides are
instruction immediates, no K step below 24 tests a column against D0, and the address multiplies are gone.
The values entering every MFMA and every optimizer update, and their order, do not change, so every
parameter, every optimizer moment and the epoch's loss and accuracy sums must be bit-identical with the
switch at 1 and at 0. At every other width the switch must fall back: the launch reports the run-time
kernel and the fit is the same whatever the switch says.

The straight body's address arithmetic itself (one base per address family and step, constant deltas) has
no switch: the guarded body of tests/test_mlp_f32_c2_pipeline_gpu.py and the float64 oracle of
tests/test_mlp_f32_oracle_gpu.py are its independent references.

Small shapes: 1 or 3 peers, layout 1, owner K split 1, 2 epochs, at most 340 samples per peer. The
switch-off fit of a shape is computed once and shared by the cases that compare against it.
"""

import numpy as np
import pytest

from _mlp_f32_fit import _all, _keep_fit_sums, _pin_perms, _setup, _torch_reference, dev, fp32_settings, lib  # noqa: F401 (fixtures)
from _mlp_f32_fit import _assert_same as _same_core

pytestmark = pytest.mark.gpu

ADAM = {"name": "adam", "lr": 1e-3}
SGDM = {"name": "sgd", "lr": 1e-4, "momentum": 0.9}
# samples per peer that give 1, 2, 3 and 6 steps per epoch, the last batch shorter than B
PER_PEER = {64: {1: 40, 2: 100, 3: 150, 6: 340}, 32: {1: 20, 2: 50, 3: 80, 6: 170}}
FALLBACK_WIDTHS = [736, 760, 768, 792]


_FITS = {}  # fits by (switch, shape): each computed once, never modified
_SEED = {}  # the data seed of a width (_width_seed's rule)


def _run(lib, dev, switch, P, B, per_peer, spec, D0=784, seed=21, epochs=2, torch_ref=False):
    """One seeded fit with the switch at `switch`: every peer's flat parameters, the moments the engine
    keeps across the fit's epochs, the fit's loss and accuracy sums as the kernel accumulated them, and
    what the launch reported. `torch_ref`: also the largest relative update error of any parameter tensor
    against fp32 autograd + torch.optim.Adam on the same batches (`rel`), and that reference's own error:
    the same measure between it and the same torch run in fp64 (`ref_err`)."""
    from myfyp_amd.parallel.mlp_engine import MLPGroup

    lib.mlp_set_f32_static_d0(switch)
    MLPGroup.reset_all()
    learners, refs, g, n = _setup(dev, P, B, per_peer, seed, spec, D0)
    perms = _pin_perms(dev, g, learners, n)
    p0 = [[p.detach().clone() for p in l.model.get_model().parameters()] for l in learners]
    for l in learners:
        l.set_epochs(epochs)
    sums = _keep_fit_sums(g)
    _all(learners, "fit")
    _all(learners, "evaluate")  # results fetched: give-up status checked
    assert g.recoveries() == 0
    assert len(sums) == 1, f"{len(sums)} fit results fetched"
    assert lib.mlp_f32_fwd_fuse_last() == 1 and lib.mlp_f32_h1_frag_last() == 1, "the epoch launch did not take the fused fragment kernels"
    slots = [l._engine.slot for l in learners]
    out = {
        "params": [l.flat_params().detach().clone() for l in learners],
        "m": [g.m[s].detach().clone() for s in slots],
        "v": [g.v[s].detach().clone() for s in slots],
        "loss": [sums[0][0][s] for s in slots],
        "correct": [int(sums[0][1][s]) for s in slots],
        "static": lib.mlp_f32_static_d0_last(),
        "k24": lib.mlp_f32_k24_last(),
    }
    if torch_ref:
        out["rel"], out["ref_err"] = _torch_reference(learners, refs, p0, perms, B, spec, epochs)
    return out


def _fit(lib, dev, switch, P, B, per_peer, spec, D0=784, seed=21):
    """The fit of a shape with the switch at `switch`, computed once; never modified."""
    key = (switch, P, B, per_peer, spec["name"], D0, seed)
    if key not in _FITS:
        _FITS[key] = _run(lib, dev, switch, P, B, per_peer, spec, D0=D0, seed=seed)
    return _FITS[key]


def _assert_same(a, b, adam):
    """Bit-equal parameters, moments, loss sums and correct counts."""
    _same_core(a, b, adam)
    for i, (x, y) in enumerate(zip(a["loss"], b["loss"])):
        assert np.isfinite(x) and x > 0, f"peer {i}: loss sum {x}"
        assert x.tobytes() == y.tobytes(), f"peer {i}: loss sums {x!r} and {y!r}"
    assert a["correct"] == b["correct"], (a["correct"], b["correct"])


@pytest.mark.parametrize("steps", [1, 2, 3, 6])
@pytest.mark.parametrize("spec", [ADAM, SGDM], ids=["adam", "sgdm"])
@pytest.mark.parametrize("B", [64, 32])
@pytest.mark.parametrize("P", [1, 3])
def test_static_d0_bit_identical_to_the_run_time_width(lib, dev, P, B, spec, steps):
    """D0 = 784, two epochs (the second starts from the first's written-back moments). One step: no next
    batch is staged and H1 comes from the prologue only; two and three steps: both parities of the
    staged tile and of the exchange slabs; six: the steady state. The last batch of every epoch is
    shorter than B (40 / 36 / 22 / 20 rows at B = 64, 20 / 18 / 16 / 10 at B = 32), so the zero rows of
    the staged tile and the bias inputs of the rows past the batch are exercised in every case. One
    peer and three peers in a launch."""
    per_peer = PER_PEER[B][steps]
    on = _run(lib, dev, 1, P, B, per_peer, spec)
    assert on["static"] == 1 and on["k24"] == 1, f"switch 1 at D0 784: the launch reported static {on['static']}, K24 {on['k24']}"
    off = _fit(lib, dev, 0, P, B, per_peer, spec)
    assert off["static"] == 0, f"switch 0 asked for, the launch reported {off['static']}"
    _assert_same(on, off, spec["name"] == "adam")


def _width_seed(lib, dev, D0):
    """The data seed of a width: the first of 21, 22, ... whose fp32 torch run agrees with its own fp64
    run to 1e-4, a tenth of the bound, so that the reference's own rounding cannot use the bound up (the
    rule of test_mlp_f32_k24_gpu.py; it looks at torch alone, never at the kernel's result). The
    switch-on fit made on the way is kept, with its error against fp32 torch."""
    if D0 not in _SEED:
        for seed in (21, 22, 23, 24):
            on = _run(lib, dev, 1, 2, 64, 300, ADAM, D0=D0, seed=seed, torch_ref=True)
            print(f"D0 {D0} seed {seed}: relative update error vs fp32 torch {on['rel']:.3e}, fp32 torch vs fp64 torch {on['ref_err']:.3e}")
            if on["ref_err"] < 1e-4:
                break
        else:
            pytest.fail(f"D0 {D0}: no data seed with a reproducible fp32 reference")
        _SEED[D0] = seed
        _FITS[(1, 2, 64, 300, "adam", D0, seed)] = on
    return _SEED[D0]


@pytest.mark.parametrize("D0", FALLBACK_WIDTHS)
def test_static_d0_falls_back_at_other_widths(lib, dev, D0):
    """Widths the static kernel is not built for, Adam, B = 64, 300 samples per peer (five steps), 2
    peers. 736: no K step 24 (the bias chunk inside register K step 23 of wave 7); 760: likewise, with
    three data chunks in front of it; 768: a multiple of 32, the bias column opens K step 24 alone;
    792: K step 24 with three data chunks and the bias column in its last chunk. With the switch at 1
    the launch reports the run-time kernel and the fit equals the switch-0 fit bit for bit; it is
    reproduced bit for bit by a second run, and lies within 1e-3 (relative update error, the bound of
    test_f32_epoch_matches_torch_adam) of fp32 autograd + torch.optim.Adam on the same batches."""
    seed = _width_seed(lib, dev, D0)
    on = _fit(lib, dev, 1, 2, 64, 300, ADAM, D0=D0, seed=seed)
    assert on["static"] == 0, f"D0 {D0}, switch 1: the launch reported the static-width kernel"
    assert on["k24"] == (1 if D0 >= 768 else 0), f"D0 {D0}: the launch reported K24 mode {on['k24']}"
    off = _fit(lib, dev, 0, 2, 64, 300, ADAM, D0=D0, seed=seed)
    assert off["static"] == 0
    _assert_same(on, off, True)
    again = _run(lib, dev, 1, 2, 64, 300, ADAM, D0=D0, seed=seed)
    _assert_same(again, on, True)
    assert on["rel"] < 1e-3, f"D0 {D0}: relative update error {on['rel']:.2e}"


@pytest.mark.parametrize("B", [64, 32])
def test_static_d0_matches_torch_and_reproduces(lib, dev, B):
    """D0 = 784 with the static-width kernel, Adam, 300 samples per peer: relative update error against
    fp32 autograd + torch.optim.Adam < 1e-3 (the same bound and seed rule), and a second run bit-equal."""
    for seed in (21, 22, 23, 24):
        on = _run(lib, dev, 1, 2, B, 300, ADAM, seed=seed, torch_ref=True)
        print(f"B {B} seed {seed}: relative update error vs fp32 torch {on['rel']:.3e}, fp32 torch vs fp64 torch {on['ref_err']:.3e}")
        if on["ref_err"] < 1e-4:
            break
    else:
        pytest.fail(f"B {B}: no data seed with a reproducible fp32 reference")
    assert on["static"] == 1
    again = _run(lib, dev, 1, 2, B, 300, ADAM, seed=seed)
    assert again["static"] == 1
    _assert_same(again, on, True)
    assert on["rel"] < 1e-3, f"B {B}: relative update error {on['rel']:.2e}"
