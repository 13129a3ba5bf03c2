"""The owners' fused next-step forward of the fp32 epoch kernel (csrc/kernels/mlp_persistent_f32.hip,
``FUSE``): the forward of step t + 1 is accumulated inside C2 of step t, per wave, on the K steps the
wave has just updated and the columns of X(t + 1) it has just staged. Every wave adds its K steps in
the order of the separate forward and the cross-wave sum runs in wave order, so H1 — and with it
every parameter and optimizer moment after an epoch — must be bit-identical to the separate forward
(``mlp_set_f32_fwd_fuse(0)`` / ``MYFYP_F32_FWD_FUSE=0``). Small shapes: 2 peers (8 for the one-launch
gang packing), a few hundred samples each.
"""

import ctypes

import pytest

from _mlp_f32_fit import _all, _assert_same, _pin_perms, _setup, dev, fp32_settings, lib  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

ADAM = {"name": "adam", "lr": 1e-3}
SGDM = {"name": "sgd", "lr": 1e-4, "momentum": 0.9}


def _run(lib, dev, fuse, P, B, per_peer, spec, epochs=2, seed=21, giveup=None):
    """One seeded fit with the switch at `fuse`: every peer's flat parameters, the moments the engine
    keeps across the fit's epochs, the gangs' placement verdicts and the recovery count."""
    from myfyp_amd.parallel.mlp_engine import MLPGroup

    lib.mlp_set_f32_fwd_fuse(fuse)
    MLPGroup.reset_all()
    learners, _, g, n = _setup(dev, P, B, per_peer, seed, spec)
    _pin_perms(dev, g, learners, n)
    for l in learners:
        l.set_epochs(epochs)
    if giveup is not None:
        g.debug_giveup(learners[giveup[0]]._engine.slot, at_end=giveup[1])
    _all(learners, "fit")
    _all(learners, "evaluate")  # results fetched: give-up status checked
    assert lib.mlp_f32_fwd_fuse_last() == fuse, "the epoch launch did not take the path asked for"
    seen = (ctypes.c_int * 64)()
    assert lib.mlp_debug_plain_seen(seen) == 0
    slots = [l._engine.slot for l in learners]
    out = {
        "params": [l.flat_params().detach().clone() for l in learners],
        "m": [g.m[s].detach().clone() for s in slots],
        "v": [g.v[s].detach().clone() for s in slots],
        "seen": [seen[s] for s in slots],
        "recoveries": g.recoveries(),
    }
    if giveup is not None:
        g.debug_giveup(None)
    return out


@pytest.mark.parametrize("per_peer", [300, 600])
@pytest.mark.parametrize("spec", [ADAM, SGDM], ids=["adam", "sgdm"])
@pytest.mark.parametrize("B", [64, 32])
def test_fused_forward_bit_identical(lib, dev, B, spec, per_peer):
    """Two epochs, 2 peers: 300 samples are 4 full steps and a 44-row batch at B = 64 (9 and 12 rows at
    B = 32), 600 are 9 full steps and a 24-row batch: the partial batch's rows_at(t + 1) masking in the
    fused reduction and the last step, which accumulates and publishes nothing."""
    fused = _run(lib, dev, 1, 2, B, per_peer, spec)
    sep = _run(lib, dev, 0, 2, B, per_peer, spec)
    _assert_same(fused, sep, spec["name"] == "adam")
    assert fused["m"][0].abs().max() > 0  # the moments were written back


@pytest.mark.parametrize("per_peer", [40, 64, 100, 128])
def test_fused_forward_edge_step_counts(lib, dev, per_peer):
    """n <= B: one step, the prologue forward only and no fused iteration; B < n <= 2B: exactly one
    fused iteration (a partial and a full second batch)."""
    fused = _run(lib, dev, 1, 2, 64, per_peer, ADAM)
    sep = _run(lib, dev, 0, 2, 64, per_peer, ADAM)
    _assert_same(fused, sep, True)


def test_fused_forward_eight_peers_one_launch(lib, dev):
    """The headline's gang packing: 8 peers in one launch, every gang on one XCD (hand-offs kept in
    L2, persist::gang_same_xcd), 150 samples per peer."""
    fused = _run(lib, dev, 1, 8, 64, 150, ADAM)
    sep = _run(lib, dev, 0, 8, 64, 150, ADAM)
    assert fused["seen"] == [1] * 8 and sep["seen"] == [1] * 8, (fused["seen"], sep["seen"])
    _assert_same(fused, sep, True)


@pytest.mark.parametrize("at_end", [False, True])
def test_fused_forward_giveup_recovered_by_retry_launch(lib, dev, at_end):
    """The engine's bounded-wait test hook makes one peer's gang give up on its first attempt (at
    entry, or at the gang commit after every fused step ran): it stores nothing, and the retry launch
    reproduces the unforced fit bit for bit, moments included; the other peers are unaffected."""
    ok = _run(lib, dev, 1, 3, 64, 300, ADAM, epochs=1)
    rec = _run(lib, dev, 1, 3, 64, 300, ADAM, epochs=1, giveup=(1, at_end))
    assert ok["recoveries"] == 0 and rec["recoveries"] == 1, (ok["recoveries"], rec["recoveries"])
    _assert_same(ok, rec, True)
