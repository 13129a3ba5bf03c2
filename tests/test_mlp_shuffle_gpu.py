"""The fused MLP engine's epoch shuffle and batch path, through the engine.

* Host keys (default fp32 engine, native shuffle): the 64-bit keys the engine draws from Python's ``random``
  (``MLPGroup._run_fit_batch``: the epoch's key, then the key of the epoch ahead) are the keys the gather kernel
  uses, in every ``MYFYP_PREP_GATHER`` mode: two fits of two epochs give bit-identical parameters to the same fits
  with ``perm_fn`` returning the oracle's ``feistel_perm(., n_p, peer_key(seed_e, slot_p))``. Controls: another peer's key
  and the previous epoch's key fed through ``perm_fn`` give other parameters.
* ``set_seed``: the same seed gives the same training, another seed another.
* bf16 engine, one epoch of plain SGD: the persistent epoch kernel and the 3-launch step path against a
  whole-epoch run of the float64 oracle (``_mlp_ref.sgd_epoch``), at 8 times the oracle's own sensitivity to
  the accumulation order of its sums.
"""

import random
import threading

import numpy as np
import pytest
import torch

import _mlp_ref as M

pytestmark = pytest.mark.gpu

SIZES = (150, 97, 64)
B = 32


@pytest.fixture(scope="module")
def dev():
    from myfyp_amd.ops import _native

    _native.load(required=True)
    return torch.device("cuda")


@pytest.fixture(autouse=True)
def engine_settings():
    from myfyp_amd.parallel.mlp_engine import MLPGroup
    from myfyp_amd.settings import Settings

    old = (Settings.MLP_PRECISION, Settings.GANG_WINDOW, Settings.USE_FUSED_KERNELS)
    Settings.MLP_PRECISION, Settings.GANG_WINDOW, Settings.USE_FUSED_KERNELS = "fp32", 5.0, True
    MLPGroup.reset_all()
    yield
    MLPGroup.reset_all()
    Settings.MLP_PRECISION, Settings.GANG_WINDOW, Settings.USE_FUSED_KERNELS = old


def _learners(sizes, spec, scale=1.0, epochs=1):
    """One learner per entry of ``sizes``, each on a synthetic dataset of its own of exactly that many samples."""
    from myfyp_amd.learning.dataset.synthetic import synthetic_mnist
    from myfyp_amd.learning.frameworks.torch import TorchLearner, TorchModel
    from myfyp_amd.models import MLP

    learners = []
    for i, n in enumerate(sizes):
        m = MLP(seed=70 + i)
        if scale != 1.0:
            with torch.no_grad():
                for prm in m.parameters():
                    prm.mul_(scale)
        m.optimizer_spec = lambda spec=spec: dict(spec)
        l = TorchLearner(TorchModel(m), synthetic_mnist(n, 40, seed=20 + i), f"s{i}", batch_size=B)
        l.set_epochs(epochs)
        learners.append(l)
    assert all(l._engine is not None for l in learners), "the fused engine is not attached"
    g = learners[0]._engine.group
    assert [l.device_data(True)[0].shape[0] for l in learners] == list(sizes)
    return learners, g


def _fit_all(learners):
    ts = [threading.Thread(target=l.fit) for l in learners]
    [t.start() for t in ts]
    [t.join() for t in ts]
    torch.cuda.synchronize()


def _params(learners):
    return [l.flat_params().detach().clone() for l in learners]


def _pin(g, learners, sizes, seeds, key_of=M.peer_key, shift=0):
    """``perm_fn`` that returns the oracle's permutation for the e-th epoch the engine runs (over all fits) under
    ``seeds[e + shift]``."""
    count = [0]

    def perm_fn(ep):
        seed = seeds[max(0, count[0] + shift)]
        count[0] += 1
        out = torch.zeros(g.capacity, g.nmax, dtype=torch.int32)
        for l, n in zip(learners, sizes):
            slot = l._engine.slot
            out[slot, :n] = torch.from_numpy(M.feistel_perm_np(n, key_of(seed, slot)).astype(np.int32))
        return out.cuda()

    g.perm_fn = perm_fn


def _two_fits(sizes, spec, native_seed=None, pin=None):
    from myfyp_amd.parallel.mlp_engine import MLPGroup

    MLPGroup.reset_all()
    learners, g = _learners(sizes, spec, epochs=2)
    if pin is not None:
        _pin(g, learners, sizes, **pin)
    if native_seed is not None:
        random.seed(native_seed)
    for _ in range(2):
        _fit_all(learners)
    out = _params(learners)
    MLPGroup.reset_all()
    return out


@pytest.mark.parametrize("prep", ["0", "1", "2"])
def test_host_keys_are_the_kernels_keys(dev, monkeypatch, prep):
    """3 peers of 150, 97 and 64 samples, Adam, two fits of two epochs under ``random.seed(k)``. The engine draws the first
    epoch's key, then one key ahead per epoch, and keeps the key drawn ahead across fits: epoch e of the run uses
    draw e of the stream."""
    monkeypatch.setenv("MYFYP_PREP_GATHER", prep)
    monkeypatch.setenv("MYFYP_PREP_GATHER_WGS", "3")
    spec = {"name": "adam", "lr": 1e-3}
    k = 24680 + int(prep)
    native = _two_fits(SIZES, spec, native_seed=k)
    random.seed(k)
    seeds = [random.getrandbits(64) for _ in range(5)]  # 4 epochs + the key drawn ahead of a fifth
    pinned = _two_fits(SIZES, spec, pin=dict(seeds=seeds))
    for a, b in zip(native, pinned):
        assert torch.equal(a, b), "the native shuffle is not feistel_perm under the keys the host drew"
    # controls: the comparison tells a wrong peer key and a stale epoch key apart
    wrong_peer = _two_fits(SIZES, spec, pin=dict(seeds=seeds, key_of=lambda s, p: M.peer_key(s, p + 1)))
    stale = _two_fits(SIZES, spec, pin=dict(seeds=seeds, shift=-1))
    for other, label in ((wrong_peer, "another peer's key"), (stale, "the previous epoch's key")):
        assert not any(torch.equal(a, b) for a, b in zip(native, other)), f"{label} gives the same training"


def test_set_seed(dev):
    """Two runs after the same ``set_seed`` are bit-identical (the models are seeded on their own); a run after another
    seed differs for every peer."""
    from myfyp_amd.utils.seed import set_seed

    spec = {"name": "adam", "lr": 1e-3}
    runs = []
    for seed in (11, 11, 12):
        set_seed(seed)
        runs.append(_two_fits(SIZES, spec))
    for a, b, c in zip(*runs):
        assert torch.equal(a, b)
        assert not torch.equal(a, c)


EPOCH_N = (160, 139)


@pytest.mark.parametrize("persistent", [None, False], ids=["persistent", "steps"])
def test_bf16_epoch_against_the_oracle(dev, persistent):
    """bf16 engine, one epoch of plain SGD (lr 1e-2, weights scaled by 0.05 as in ``test_kernels_gpu``; at lr 1e-3 the
    fp32 rounding of the master row alone puts the floor of b1 at 5e-3, and 8 times that is vacuous), 2 peers of 160 and
    139 samples (5 steps, the second peer's last one partial), B = 32, pinned permutations: the relative update
    error per tensor of the persistent epoch kernel and of the step path against ``_mlp_ref.sgd_epoch`` in float64.

    The bound is 8 times the oracle's own sensitivity (the same epoch with everything the kernels hold in fp32
    held in fp32: its sums accumulated in fp32 over a permuted reduction axis, the master row rounded after each
    update; against its float64 run): both kernels are free in their accumulation order.
    The floor and both kernels' values are printed per tensor. MI355X (floor | persistent | steps):

    ====== ======== ======== ========  ======== ======== ========
    tensor peer 0                      peer 1
    ====== ======== ======== ========  ======== ======== ========
    W1     4.54e-06 4.54e-06 4.54e-06  4.06e-06 4.06e-06 4.06e-06
    b1     4.37e-04 4.36e-04 4.37e-04  5.87e-04 5.88e-04 5.87e-04
    W2     1.57e-05 1.57e-05 1.57e-05  5.11e-06 5.12e-06 5.17e-06
    b2     1.54e-05 1.54e-05 1.54e-05  1.69e-05 1.69e-05 1.69e-05
    W3     1.50e-04 1.50e-04 1.50e-04  2.51e-06 2.49e-06 2.51e-06
    b3     8.69e-08 1.07e-07 8.69e-08  2.78e-07 1.71e-07 2.78e-07
    ====== ======== ======== ========  ======== ======== ========

    The floor and the kernels agree this closely because one term dominates all three: the fp32 rounding of the
    master row, which the float64 run does not have. The largest bound, 8 x 5.9e-4 for b1, is below 1e-2 and
    far below one batch row missing from a bias gradient (1 / 32)."""
    from myfyp_amd.parallel.mlp_engine import MLPGroup
    from myfyp_amd.settings import Settings

    Settings.MLP_PRECISION = "bf16"
    MLPGroup.reset_all()
    lr = 1e-2
    learners, g = _learners(EPOCH_N, {"name": "sgd", "lr": lr}, scale=0.05)
    assert g.precision == "bf16"
    g.persistent = persistent
    assert g.uses_persistent() == (persistent is not False)
    perms = [torch.randperm(n, generator=torch.Generator().manual_seed(40 + i)) for i, n in enumerate(EPOCH_N)]

    def perm_fn(ep):
        out = torch.zeros(g.capacity, g.nmax, dtype=torch.int32)
        for l, pm in zip(learners, perms):
            out[l._engine.slot, : pm.numel()] = pm.to(torch.int32)
        return out.cuda()

    g.perm_fn = perm_fn
    D = (784, 256, 128, 10)
    start = [p.cpu().double() for p in _params(learners)]
    _fit_all(learners)
    after = [p.cpu().double() for p in _params(learners)]
    for i, l in enumerate(learners):
        x, y = l.device_data(True)
        x, y = x.reshape(x.shape[0], -1).cpu(), y.cpu()
        W0 = M.unpack(start[i], D)
        ref = M.sgd_epoch(W0, x, y, perms[i].numpy(), B, lr)
        alt = M.sgd_epoch(W0, x, y, perms[i].numpy(), B, lr, mm=M.mm32_permuted(torch.Generator().manual_seed(i)), f32=True)
        got = M.unpack(after[i], D)
        for name in M.NAMES:
            floor = M.rel_update(alt[name], ref[name], W0[name])
            rel = M.rel_update(got[name], ref[name], W0[name])
            print(f"peer {i} {name}: oracle floor {floor:.3e}, kernel {rel:.3e}, kernel / (8 floor) {rel / (8 * floor):.3f}")
            assert 8 * floor <= 1e-2, "the floor makes the bound vacuous"
            assert rel <= 8 * floor, f"peer {i} {name}: relative update error {rel:.3e} > 8 x {floor:.3e}"
