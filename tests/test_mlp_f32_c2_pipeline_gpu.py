"""C2's straight K steps in the owners of the fp32 epoch kernel (csrc/kernels/mlp_persistent_f32.hip, the
fused-forward instantiations): the dH1 split fragments are read from LDS once per step, ahead of the
K-step loop, and every straight K step's dW1 MFMAs take them from registers (the first step of a
software pipeline over the K steps; docs/PERFORMANCE.md, "dH1 fragments read once per step"). Every
accumulator still receives the same terms in the same order, so every parameter and optimizer moment
after a fit must be bit-identical over the three builds of C2 that a launch can take:

* straight body, K step 24 in registers (``mlp_set_f32_c2_straight(1)``, ``mlp_set_f32_k24(1)``),
* straight body, K step 24 in LDS (``mlp_set_f32_k24(0)``),
* the guarded body (``mlp_set_f32_c2_straight(0)``), which the change does not touch: the reference.

Small shapes: 2 peers, layout 1, owner K split 1, fused forward, 2 epochs, at most 300 samples per
peer. The guarded fit of a shape is computed once and shared by the cases that compare against it.
"""

import pytest

from _mlp_f32_fit import _all, _assert_same, _pin_perms, _setup, _torch_reference, dev, fp32_settings, lib  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

ADAM = {"name": "adam", "lr": 1e-3}
SGDM = {"name": "sgd", "lr": 1e-4, "momentum": 0.9}
# (c2_straight, k24) asked for; the guarded body is the reference
STRAIGHT_BUILDS = [(1, 1), (1, 0)]
GUARDED = (0, 0)
WIDTHS = [736, 760, 768, 784, 792]


_FITS = {}  # fits by (build, shape): each computed once, never modified
_SEED = {}  # the data seed of a width (test_input_widths' rule)


def _run(lib, dev, build, B, per_peer, spec, D0=784, seed=21, torch_ref=False, P=2, epochs=2):
    """One seeded fit with C2 as `build` = (c2_straight, k24) asks: every peer's flat parameters and
    the moments the engine keeps across the fit's epochs, with the path the launch reported asserted.
    `torch_ref`: also the largest relative update error of any parameter tensor against fp32 autograd +
    torch.optim.Adam on the same batches (`rel`), and that reference's own error: the same measure
    between it and the same torch run in fp64 (`ref_err`)."""
    from myfyp_amd.parallel.mlp_engine import MLPGroup

    straight, k24 = build
    lib.mlp_set_f32_k24(k24)
    lib.mlp_set_f32_c2_straight(straight)
    lib.mlp_set_f32_fwd_fuse(1)
    MLPGroup.reset_all()
    learners, refs, g, n = _setup(dev, P, B, per_peer, seed, spec, D0)
    perms = _pin_perms(dev, g, learners, n)
    p0 = [[p.detach().clone() for p in l.model.get_model().parameters()] for l in learners]
    for l in learners:
        l.set_epochs(epochs)
    _all(learners, "fit")
    _all(learners, "evaluate")  # results fetched: give-up status checked
    assert g.recoveries() == 0
    assert lib.mlp_f32_fwd_fuse_last() == 1, "the epoch launch did not take the fused forward"
    assert lib.mlp_f32_c2_straight_last() == straight, f"C2 body {straight} asked for, the launch reported {lib.mlp_f32_c2_straight_last()}"
    # K step 24 in registers needs the straight body and a K step 24 (D0 >= 768)
    want_k24 = k24 if straight == 1 and D0 >= 768 else 0
    assert lib.mlp_f32_k24_last() == want_k24, f"D0 {D0}, build {build}: the launch reported K24 mode {lib.mlp_f32_k24_last()}"
    slots = [l._engine.slot for l in learners]
    out = {
        "params": [l.flat_params().detach().clone() for l in learners],
        "m": [g.m[s].detach().clone() for s in slots],
        "v": [g.v[s].detach().clone() for s in slots],
    }
    if torch_ref:
        out["rel"], out["ref_err"] = _torch_reference(learners, refs, p0, perms, B, spec, epochs)
    return out


def _fit(lib, dev, build, B, per_peer, spec, D0=784, seed=21):
    """The fit of a shape with one build of C2, computed once; never modified."""
    key = (build, B, per_peer, spec["name"], D0, seed)
    if key not in _FITS:
        _FITS[key] = _run(lib, dev, build, B, per_peer, spec, D0=D0, seed=seed)
    return _FITS[key]


def _width_seed(lib, dev, D0):
    """The data seed of a width: the first of 21, 22, ... whose fp32 torch run agrees with its own fp64
    run to 1e-4, a tenth of the bound, so that the reference's own rounding cannot use the bound up (the
    rule of test_mlp_f32_k24_gpu.py; it looks at torch alone, never at the kernel's result). The
    straight-body fit made on the way is kept, with its error against fp32 torch."""
    if D0 not in _SEED:
        for seed in (21, 22, 23, 24):
            on = _run(lib, dev, (1, 1), 64, 300, ADAM, D0=D0, seed=seed, torch_ref=True)
            print(f"D0 {D0} seed {seed}: relative update error vs fp32 torch {on['rel']:.3e}, fp32 torch vs fp64 torch {on['ref_err']:.3e}")
            if on["ref_err"] < 1e-4:
                break
        else:
            pytest.fail(f"D0 {D0}: no data seed with a reproducible fp32 reference")
        _SEED[D0] = seed
        _FITS[((1, 1), 64, 300, "adam", D0, seed)] = on
    return _SEED[D0]


@pytest.mark.parametrize("steps", ["one", "two", "five"])
@pytest.mark.parametrize("spec", [ADAM, SGDM], ids=["adam", "sgdm"])
@pytest.mark.parametrize("B", [64, 32])
def test_pipeline_bit_identical_over_the_builds(lib, dev, B, spec, steps):
    """D0 = 784. B - 24 samples per peer: one step (a pipeline over the K steps has its prologue and
    epilogue meet here, and nothing real is staged for a next step); B + 36: two steps, the second partial (36 rows at B = 64; at
    B = 32 it is three steps, the last with 4 rows); 4 B + 44: five steps, the last with 44 rows
    (B = 32: six steps, the last with 12)."""
    per_peer = {"one": B - 24, "two": B + 36, "five": 4 * B + 44}[steps]
    ref = _fit(lib, dev, GUARDED, B, per_peer, spec)
    for build in STRAIGHT_BUILDS:
        _assert_same(_fit(lib, dev, build, B, per_peer, spec), ref, spec["name"] == "adam")


@pytest.mark.parametrize("D0", WIDTHS)
def test_pipeline_input_widths(lib, dev, D0):
    """Where the bias column and the padding fall in the straight K steps, Adam, B = 64, 300 samples
    per peer (five steps). 736 and 760: no K step 24; the bias chunk lies inside register K step 23 of
    wave 7, that wave's last. 768: K step 24 holds only the bias column. 784: the
    benchmark's width. 792: the bias column in chunk 3 of K step 24. Bit identity over the three
    builds, and the straight build against fp32 autograd + torch.optim.Adam on the same batches:
    relative update error < 1e-3 (the bound of test_f32_epoch_matches_torch_adam)."""
    seed = _width_seed(lib, dev, D0)
    on = _fit(lib, dev, (1, 1), 64, 300, ADAM, D0=D0, seed=seed)
    ref = _fit(lib, dev, GUARDED, 64, 300, ADAM, D0=D0, seed=seed)
    _assert_same(on, ref, True)
    _assert_same(_fit(lib, dev, (1, 0), 64, 300, ADAM, D0=D0, seed=seed), ref, True)
    assert on["rel"] < 1e-3, f"D0 {D0}: relative update error {on['rel']:.2e}"


@pytest.mark.parametrize("B,D0", [(64, d) for d in WIDTHS] + [(32, 784)])
def test_pipeline_reproducible(lib, dev, B, D0):
    """The same fit twice with the same seeds: bit-equal. A missed LDS ordering between a read that
    moved ahead (the dH1 fragments, read before the K-step loop) and a store of C1 or of the staging
    shows up as run-to-run differences."""
    seed = _width_seed(lib, dev, D0) if B == 64 else 21
    first = _fit(lib, dev, (1, 1), B, 300, ADAM, D0=D0, seed=seed)
    again = _run(lib, dev, (1, 1), B, 300, ADAM, D0=D0, seed=seed)
    _assert_same(again, first, True)
