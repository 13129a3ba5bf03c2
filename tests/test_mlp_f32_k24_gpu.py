"""K step 24 register-resident on its wave in the owners of the fp32 epoch kernel
(csrc/kernels/mlp_persistent_f32.hip, the ``K24`` instantiations): at D0 >= 768 wave 0 of an owner holds K step
24 (the last pixel columns, the bias column, padding) beside its three register-resident K steps. With
``mlp_set_f32_k24(1)`` / ``MYFYP_F32_K24=1`` it takes that K step's weights and moments from LDS into
registers before the step loop and returns them after it, instead of a round trip per step. The same
operations run on the same values, so every parameter and optimizer moment after a fit must be
bit-identical with the switch at 1 and at 0. The body needs the fused forward and C2's straight body;
without either, or without a K step 24 (D0 < 768), the launch reports mode 0.

Small shapes: 2 peers (3 for the retry cases), layout 1, owner K split 1, at most 300 samples per
peer. The mode-0 fit of a shape is computed once and shared by the cases that compare against it.
"""

import copy
import threading

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ADAM = {"name": "adam", "lr": 1e-3}
SGDM = {"name": "sgd", "lr": 1e-4, "momentum": 0.9}
MODES = [1]  # the modes the kernel has beside 0


@pytest.fixture(scope="module")
def lib():
    from myfyp_amd.ops import _native

    return _native.load(required=True)


@pytest.fixture(scope="module")
def dev(lib):
    return torch.device("cuda")


@pytest.fixture(autouse=True)
def fp32_settings(lib):
    from myfyp_amd.parallel.mlp_engine import MLPGroup
    from myfyp_amd.settings import Settings

    old = (Settings.MLP_PRECISION, Settings.GANG_WINDOW, Settings.USE_FUSED_KERNELS)
    Settings.MLP_PRECISION, Settings.GANG_WINDOW, Settings.USE_FUSED_KERNELS = "fp32", 5.0, True
    MLPGroup.reset_all()
    yield
    lib.mlp_set_f32_k24(-1)
    lib.mlp_set_f32_c2_straight(-1)
    lib.mlp_set_f32_fwd_fuse(-1)
    MLPGroup.reset_all()
    Settings.MLP_PRECISION, Settings.GANG_WINDOW, Settings.USE_FUSED_KERNELS = old


_DATA = {}
_REF = {}  # mode-0 fits, by shape


def _dataset(D0, n_train, seed):
    """MNIST-like uint8 rows of width D0: the synthetic 28 x 28 images, flattened and resampled to D0
    columns (D0 = 784: the images themselves)."""
    from myfyp_amd.learning.dataset.p2pfl_dataset import P2PFLDataset
    from myfyp_amd.learning.dataset.synthetic import synthetic_mnist

    key = (D0, n_train, seed)
    if key not in _DATA:
        base = synthetic_mnist(n_train, 200, seed=seed)
        if D0 != 784:
            cols = (np.arange(D0) * 784) // D0
            split = lambda tr: {"image": np.ascontiguousarray(base.column("image", tr).reshape(-1, 784)[:, cols]), "label": base.column("label", tr)}
            base = P2PFLDataset.from_arrays(split(True), split(False))
        _DATA[key] = base
    return _DATA[key]


def _setup(dev, P, B, per_peer, seed, spec, D0):
    """P peers of `per_peer` training samples each on layout 1 at owner K split 1; SGD runs start from
    half-scale weights, as the other fp32 tests do."""
    from myfyp_amd.learning.dataset.partition_strategies import RandomIIDPartitionStrategy
    from myfyp_amd.learning.frameworks.torch import TorchLearner, TorchModel
    from myfyp_amd.models import MLP

    parts = _dataset(D0, P * per_peer, seed).generate_partitions(P, RandomIIDPartitionStrategy)
    learners, refs = [], []
    for i in range(P):
        m = MLP(input_size=D0, seed=50 + i)
        if spec["name"] == "sgd":
            with torch.no_grad():
                for prm in m.parameters():
                    prm.mul_(0.5)
        m.optimizer_spec = lambda spec=spec: dict(spec)
        refs.append(copy.deepcopy(m).to(dev))
        learners.append(TorchLearner(TorchModel(m), parts[i], f"s{i}", batch_size=B))
    assert all(l._engine is not None for l in learners), "fp32 engine not attached"
    g = learners[0]._engine.group
    assert g.precision == "fp32" and g.uses_persistent()
    g.force_f32_ks = 1
    g.force_f32_variant = 1
    assert g.f32_ks() == 1 and g.f32_variant() == 1
    n = [parts[i].get_num_samples() for i in range(P)]
    assert n == [per_peer] * P, n
    return learners, refs, g, n


def _pin_perms(dev, g, learners, n, seed=0):
    perms = {}

    def perm_fn(ep):
        out = torch.zeros(g.capacity, g.nmax, dtype=torch.int32)
        for i, l in enumerate(learners):
            perms[(ep, i)] = torch.randperm(n[i], generator=torch.Generator().manual_seed(1000 * ep + 10 * seed + i))
            out[l._engine.slot, : n[i]] = perms[(ep, i)].to(torch.int32)
        return out.to(dev)

    g.perm_fn = perm_fn
    return perms


def _all(learners, what):
    # every peer from its own thread: the group gangs the calls into one launch (a lone caller
    # would wait out Settings.GANG_WINDOW for the others)
    ts = [threading.Thread(target=getattr(l, what)) for l in learners]
    [t.start() for t in ts]
    [t.join() for t in ts]
    torch.cuda.synchronize()


def _run(lib, dev, mode, P, B, per_peer, spec, D0=784, fuse=1, straight=1, epochs=2, seed=21, giveup=None, torch_ref=False):
    """One seeded fit with the switch at `mode` (None: the default, whatever the environment sets):
    every peer's flat parameters, the moments the engine keeps across the fit's epochs, the recovery
    count and what the launch reported. `torch_ref`: also the largest relative update error of any
    parameter tensor against fp32 autograd + the torch optimizer on the same batches (`rel`), and that
    reference's own error: the same measure between it and the same torch run in fp64 (`ref_err`)."""
    from myfyp_amd.parallel.mlp_engine import MLPGroup

    lib.mlp_set_f32_k24(-1 if mode is None else mode)
    lib.mlp_set_f32_c2_straight(straight)
    lib.mlp_set_f32_fwd_fuse(fuse)
    MLPGroup.reset_all()
    learners, refs, g, n = _setup(dev, P, B, per_peer, seed, spec, D0)
    perms = _pin_perms(dev, g, learners, n)
    p0 = [[p.detach().clone() for p in l.model.get_model().parameters()] for l in learners]
    for l in learners:
        l.set_epochs(epochs)
    if giveup is not None:
        g.debug_giveup(learners[giveup[0]]._engine.slot, at_end=giveup[1])
    _all(learners, "fit")
    _all(learners, "evaluate")  # results fetched: give-up status checked
    assert lib.mlp_f32_fwd_fuse_last() == fuse, "the epoch launch did not take the forward asked for"
    slots = [l._engine.slot for l in learners]
    out = {
        "params": [l.flat_params().detach().clone() for l in learners],
        "m": [g.m[s].detach().clone() for s in slots],
        "v": [g.v[s].detach().clone() for s in slots],
        "recoveries": g.recoveries(),
        "k24": lib.mlp_f32_k24_last(),
    }
    if giveup is not None:
        g.debug_giveup(None)
    if torch_ref:
        worst, ref_err = 0.0, 0.0
        for i, l in enumerate(learners):
            x, y = l.device_data(True)
            ref64 = copy.deepcopy(refs[i]).double()
            d = {}
            for ref, dt in ((refs[i], torch.float32), (ref64, torch.float64)):
                opt = torch.optim.Adam(ref.parameters(), lr=spec["lr"])
                for ep in range(epochs):
                    perm = perms[(ep, i)].to(x.device)
                    for s in range(0, perm.numel(), B):
                        idx = perm[s : s + B]
                        h = x[idx].reshape(idx.numel(), -1).to(dt)
                        for layer in ref.layers:
                            h = layer(h)
                        opt.zero_grad()
                        F.cross_entropy(torch.log_softmax(h, dim=1), y[idx]).backward()  # (MLP.forward, in dt)
                        opt.step()
                d[dt] = [pr.detach().double() - pz.double() for pr, pz in zip(ref.parameters(), p0[i])]
            for pe, pz, d_r, d_64 in zip(l.model.get_model().parameters(), p0[i], d[torch.float32], d[torch.float64]):
                d_e = pe.detach().double() - pz.double()
                worst = max(worst, ((d_e - d_r).norm() / (d_r.norm() + 1e-30)).item())
                ref_err = max(ref_err, ((d_r - d_64).norm() / (d_64.norm() + 1e-30)).item())
        out["rel"], out["ref_err"] = worst, ref_err
    return out


def _mode0(lib, dev, P, B, per_peer, spec, D0=784, epochs=2, seed=21):
    """The mode-0 fit of a shape (fused forward, straight body), computed once; never modified."""
    key = (P, B, per_peer, spec["name"], D0, epochs, seed)
    if key not in _REF:
        _REF[key] = _run(lib, dev, 0, P, B, per_peer, spec, D0=D0, epochs=epochs, seed=seed)
        assert _REF[key]["k24"] == 0, f"mode 0 asked for, the launch reported {_REF[key]['k24']}"
    return _REF[key]


def _assert_same(a, b, adam):
    for key in ("params", "m") + (("v",) if adam else ()):
        for i, (x, y) in enumerate(zip(a[key], b[key])):
            assert torch.isfinite(x).all(), f"peer {i} {key}: not finite"
            assert torch.equal(x, y), f"peer {i} {key}: {int((x != y).sum())} elements differ, max {float((x - y).abs().max()):.3e}"
    assert all(float(p.abs().max()) > 0 for p in a["params"])
    assert a["m"][0].abs().max() > 0  # the moments were written back


@pytest.mark.parametrize("per_peer", [40, 100, 300])
@pytest.mark.parametrize("spec", [ADAM, SGDM], ids=["adam", "sgdm"])
@pytest.mark.parametrize("B", [64, 32])
@pytest.mark.parametrize("mode", MODES)
def test_k24_bit_identical_to_mode0(lib, dev, mode, B, spec, per_peer):
    """D0 = 784, fused forward, two epochs, 2 peers. 40 samples: one step at B = 64 (K step 24's state
    is loaded, updated once and returned; the second epoch starts from the written-back moments), 100:
    two steps, the second partial, 300: four full steps and a 44-row batch (B = 32: 2, 4 and 10 steps,
    the last with 8, 4 and 12 rows)."""
    on = _run(lib, dev, mode, 2, B, per_peer, spec)
    assert on["k24"] == mode, f"mode {mode} asked for, the launch reported {on['k24']}"
    _assert_same(on, _mode0(lib, dev, 2, B, per_peer, spec), spec["name"] == "adam")


@pytest.mark.parametrize("D0", [768, 776, 792, 760])
@pytest.mark.parametrize("mode", MODES)
def test_k24_input_widths(lib, dev, mode, D0):
    """Where the bias column and the padding fall in K step 24. 768: it holds only the bias column, in
    chunk 0, and its second half is all padding. 776: 8 pixel columns, the bias column in chunk 1, the
    second half still all padding. 792: 24 pixel columns, the bias column in chunk 3, the last of the
    second half (784, the other tests' width, has it in chunk 2). 760: 24 K steps, no K step 24: the launch reports mode 0 and the results are equal all the same.
    Each width also against fp32 autograd + torch.optim.Adam on the same batches, relative update
    error < 1e-3 (the bound of test_f32_epoch_matches_torch_adam).

    The data seed is the first of 21, 22, ... at which that reference reproduces itself: the same
    torch run in fp64 must agree with the fp32 one to 1e-4, a tenth of the bound, so that the
    reference's own rounding cannot use the bound up. Measured at D0 = 776 with seed 21: peer 0's fp32
    torch run is 0.6e-2 .. 2.3e-2 (per tensor) from its fp64 run, and the kernel, mode 0 and mode 1
    alike (same bits), 1.1e-2 from the former and 1.4e-2 from the latter, while peer 1 sits at
    1e-6 .. 5e-6 on all three; seed 22 is alike (fp32 torch 2.3e-2 from fp64 torch), seed 23 is taken
    (kernel 5.6e-6 from fp32 torch, fp32 torch 3.1e-6 from fp64 torch). Widths 768, 792 and 760 take
    seed 21 (1e-6 .. 1.4e-5). Such a ten-step Adam trajectory amplifies rounding (Adam turns a
    near-zero gradient into a full-size update of either sign), whoever does the rounding. The
    criterion looks at torch alone, never at the kernel's result."""
    for seed in (21, 22, 23, 24):
        on = _run(lib, dev, mode, 2, 64, 300, ADAM, D0=D0, seed=seed, torch_ref=True)
        print(f"D0 {D0} mode {mode} seed {seed}: relative update error vs fp32 torch {on['rel']:.3e}, fp32 torch vs fp64 torch {on['ref_err']:.3e}")
        if on["ref_err"] < 1e-4:
            break
    else:
        pytest.fail(f"D0 {D0}: no data seed with a reproducible fp32 reference")
    want = mode if D0 >= 768 else 0
    assert on["k24"] == want, f"D0 {D0}, mode {mode} asked for: the launch reported {on['k24']}, expected {want}"
    _assert_same(on, _mode0(lib, dev, 2, 64, 300, ADAM, D0=D0, seed=seed), True)
    assert on["rel"] < 1e-3, f"D0 {D0}: relative update error {on['rel']:.2e}"


@pytest.mark.parametrize("off", ["fwd_fuse", "c2_straight"])
@pytest.mark.parametrize("mode", MODES)
def test_k24_needs_the_fused_forward_and_the_straight_body(lib, dev, mode, off):
    """With the separate forward, or with the guarded C2 body, the launch falls back to mode 0: it
    reports 0, and the fit equals the mode-0 fit of the default switches bit for bit."""
    on = _run(lib, dev, mode, 2, 64, 300, ADAM, fuse=0 if off == "fwd_fuse" else 1, straight=0 if off == "c2_straight" else 1)
    assert on["k24"] == 0, f"{off} off, mode {mode} asked for: the launch reported {on['k24']}"
    _assert_same(on, _mode0(lib, dev, 2, 64, 300, ADAM), True)


@pytest.mark.parametrize("at_end", [False, True])
def test_k24_giveup_recovered_by_retry_launch(lib, dev, at_end):
    """The default mode, 3 peers. The engine's bounded-wait test hook makes one peer's gang give up on
    its first attempt (at entry, or at the gang commit after every step ran, when K step 24's state is
    back in LDS but nothing is stored): the retry launch reproduces the unforced fit bit for bit,
    moments included."""
    ok = _run(lib, dev, None, 3, 64, 300, ADAM, epochs=1)
    rec = _run(lib, dev, None, 3, 64, 300, ADAM, epochs=1, giveup=(1, at_end))
    assert ok["recoveries"] == 0 and rec["recoveries"] == 1, (ok["recoveries"], rec["recoveries"])
    assert ok["k24"] == rec["k24"] == max(MODES), (ok["k24"], rec["k24"])
    _assert_same(ok, rec, True)
