"""What the A/B tests of the fp32 epoch kernel's switches share (tests/test_mlp_f32_{fwd_fuse, c2_straight,
c2_pipeline, k24, dh2_frag, h1_frag, c2_addr}_gpu.py): the fixtures, a seeded fit's set-up on small shapes, the
torch reference of such a fit and the bit-equality check. A test module imports the fixtures by name
(``from _mlp_f32_fit import lib, dev, fp32_settings``) and keeps its own ``_run``: the switches it sets and
what it collects differ from file to file.
"""

import copy
import threading

import numpy as np
import pytest
import torch
import torch.nn.functional as F

SWITCHES = ("mlp_set_plain_pub", "mlp_set_f32_fwd_fuse", "mlp_set_f32_c2_straight", "mlp_set_f32_k24", "mlp_set_f32_dh2_frag",
            "mlp_set_f32_h1_frag", "mlp_set_f32_static_d0")


@pytest.fixture(scope="module")
def lib():
    from myfyp_amd.ops import _native

    return _native.load(required=True)


@pytest.fixture(scope="module")
def dev(lib):
    return torch.device("cuda")


@pytest.fixture(autouse=True)
def fp32_settings(lib):
    """fp32 persistent epochs for the test, and afterwards every switch back at the environment's value,
    whichever of them the test set."""
    from myfyp_amd.parallel.mlp_engine import MLPGroup
    from myfyp_amd.settings import Settings

    old = (Settings.MLP_PRECISION, Settings.GANG_WINDOW, Settings.USE_FUSED_KERNELS)
    Settings.MLP_PRECISION, Settings.GANG_WINDOW, Settings.USE_FUSED_KERNELS = "fp32", 5.0, True
    MLPGroup.reset_all()
    yield
    for name in SWITCHES:
        getattr(lib, name)(-1)
    MLPGroup.reset_all()
    Settings.MLP_PRECISION, Settings.GANG_WINDOW, Settings.USE_FUSED_KERNELS = old


_DATA = {}


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


def _setup(dev, P, B, per_peer, seed, spec, D0=784, ks=1, variant=1):
    """P peers of `per_peer` training samples each on gang layout `variant` at owner K split `ks`; SGD
    runs start from half-scale weights, as the other fp32 tests do. Returns the learners, a copy of each
    initial model on the device (for a torch reference), the group and the sample counts."""
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
    g.force_f32_ks = ks
    g.force_f32_variant = variant
    assert g.f32_ks() == ks and g.f32_variant() == variant
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


def _all(learners, what, extras=None):
    # every peer from its own thread: the group gangs the calls into one launch (a lone caller
    # would wait out Settings.GANG_WINDOW for the others)
    def run(i, l):
        if extras is None:
            getattr(l, what)()
        else:
            l._engine.fit(l, l._optimizer_spec(), extras[i])

    ts = [threading.Thread(target=run, args=(i, l)) for i, l in enumerate(learners)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    torch.cuda.synchronize()


def _keep_fit_sums(g):
    """The fit's result as the device wrote it: from now on every fit result the group fetches is appended
    to the returned list as (per-slot loss sums (fp32), per-slot correct counts), before the engine divides
    them by the sample count."""
    sums, fetch = [], g._fetch

    def fetch_and_keep(k, with_conf):
        r = fetch(k, with_conf)
        if not with_conf:
            sums.append((r[0].copy(), r[1].copy()))
        return r

    g._fetch = fetch_and_keep
    return sums


def _torch_reference(learners, refs, p0, perms, B, spec, epochs):
    """The fitted learners against torch on the same batches. `rel`: the largest relative update error of
    any parameter tensor (from the initial values `p0`) against fp32 autograd + torch.optim.Adam run on
    `refs`; `ref_err`: that reference's own error, the same measure between it and the same torch run in
    fp64."""
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
    return worst, ref_err


def _assert_same(a, b, adam):
    """Two fits' parameters and moments (`v` for Adam only): finite and bit-equal, and written at all."""
    for key in ("params", "m") + (("v",) if adam else ()):
        for i, (x, y) in enumerate(zip(a[key], b[key])):
            assert torch.isfinite(x).all(), f"peer {i} {key}: not finite"
            assert torch.equal(x, y), f"peer {i} {key}: {int((x != y).sum())} elements differ, max {float((x - y).abs().max()):.3e}"
    assert all(float(p.abs().max()) > 0 for p in a["params"])
    assert a["m"][0].abs().max() > 0  # the moments were written back
