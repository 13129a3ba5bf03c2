"""The ClippedGossip kernels of ``csrc/kernels/fl_ops.hip`` (``k_pairwise_sqdist<K>``, ``k_clip_plan``,
``k_clipped_mix<K>``) through ``ops.clipped_gossip_into`` against the float64 oracle of
``tests/_clip_ref.py`` (MI355X only).

Bounds. Distances: ``rtol = 1e-5`` off the diagonal, the project's bound for ``k_pairwise_sqdist``
(``tests/test_robust_kernels_gpu.py``); the diagonal is 0 and the matrix symmetric, exactly. Plan:
τ² is a positively weighted sum of distances over a sum of weights, so it carries the distances'
1e-5 (the double arithmetic adds ~1e-16); τ = sqrt(τ²) and the scale τ / sqrt(D) halve that for
each of τ² and D: 1e-5 together, and one float32 rounding (6e-8) of w_eff: ``rtol = 2e-5`` for τ and
for w_eff wherever a clip is active. Where the reference's D is below τ² by more than 2e-5 the
kernel's D is below its τ² too, the scale is exactly 1 and ``w_eff == float32(W)``. In adaptive mode
the inputs are such that the reference's b-th and (b+1)-th farthest neighbours of every row are
more than 1e-3 apart (asserted), so the kernel sets the same neighbours aside. Mix: the
per-element bound derived in ``tests/_clip_ref.py``, against the oracle fed the kernel's own ``w_eff``.
"""

import ctypes

import numpy as np
import pytest
import torch

import _clip_ref as ref

pytestmark = pytest.mark.gpu

MID = 70001  # several slabs of the distance kernel
BIG = 524291  # 512 * 256 * 4 + 3: the distance kernel's grid-stride loop runs twice, and a tail


@pytest.fixture(scope="module")
def dev():
    from myfyp_amd.ops import _native

    _native.load(required=True)  # the native path must be the one under test
    return torch.device("cuda")


def _args(kw):
    return {"tau": kw.get("tau"), "num_byzantine": kw.get("b")}


def _aligned(x32, dev):
    rows = [torch.from_numpy(r.copy()).to(dev) for r in x32]
    assert all(t.data_ptr() % 16 == 0 for t in rows)
    return rows


def _offset(x32, dev):
    """The same rows, each one float past a 16-byte boundary: the scalar path."""
    k, n = x32.shape
    ld = (n + 1 + 3) // 4 * 4 + 4
    buf = torch.zeros(k * ld, dtype=torch.float32, device=dev)
    rows = [buf[i * ld + 1 : i * ld + 1 + n] for i in range(k)]
    for r, src in zip(rows, x32):
        r.copy_(torch.from_numpy(src.copy()))
    assert all(t.data_ptr() % 16 == 4 for t in rows)
    return rows


def _run(rows, w, kw):
    from myfyp_amd import ops

    dist, tau, w_eff = ops.clipped_gossip_into(rows, w, **_args(kw))
    return np.stack([r.cpu().numpy() for r in rows]), dist.cpu().numpy(), tau.cpu().numpy(), w_eff.cpu().numpy()


def _fixed_tau(x32, w):
    """A radius between the honest distances and the far rows': some neighbours inside, some clipped."""
    d = ref.sqdist(x32)
    nb = np.array([d[p, q] for p in range(len(x32)) for q in ref.neighbours(w, p) if np.isfinite(d[p, q])])
    return 1.01 * float(np.sqrt(np.median(nb))) if nb.size else 1.0


def _check(x32, w, kw, dev, what):
    """One call on aligned rows against the oracle; the offset rows and a repeat call bit-equal."""
    k, n = x32.shape
    w = np.asarray(w, dtype=np.float32)
    _, d_ref, tau_ref, tau2_ref, w_ref = ref.clipped_gossip(x32, w, **kw)
    if "b" in kw:
        gap = ref.selection_gap(d_ref, w, kw["b"])
        assert gap > 1e-3, (what, gap)  # the reference's own choice of F_p is not a coin toss
    got, dist, tau, w_eff = _run(_aligned(x32, dev), w, kw)

    # distances
    off = ~np.eye(k, dtype=bool)
    assert np.all(np.diag(dist) == 0) and np.array_equal(dist, dist.T), what
    rel = np.abs(dist[off] - d_ref[off]) / d_ref[off] if k > 1 else np.zeros(1)
    rel_d = float(rel.max())
    assert rel_d <= 1e-5, (what, rel_d)

    # plan
    rel_t = rel_w = 0.0
    for p in range(k if k > 1 else 0):  # one row: nothing is launched, no radius is formed
        if np.isfinite(tau_ref[p]) and tau_ref[p] > 0:
            rel_t = max(rel_t, abs(tau[p] - tau_ref[p]) / tau_ref[p])
        else:
            assert tau[p] == tau_ref[p], (what, p, tau[p], tau_ref[p])  # +inf and 0 are exact
        for q in range(k):
            if q == p or not w[p, q] > 0:
                assert w_eff[p, q] == 0, (what, p, q)  # zeros of W
            elif d_ref[p, q] * (1 + 2e-5) < tau2_ref[p]:
                assert w_eff[p, q] == w[p, q], (what, p, q, w_eff[p, q], w[p, q])  # inside the radius: the share itself
            else:
                assert w_ref[p, q] > 0 or w_eff[p, q] == 0, (what, p, q)
                if w_ref[p, q] > 0:
                    rel_w = max(rel_w, abs(float(w_eff[p, q]) - float(w_ref[p, q])) / float(w_ref[p, q]))
    assert rel_t <= 2e-5 and rel_w <= 2e-5, (what, rel_t, rel_w)

    # mix, against the oracle fed the kernel's own w_eff
    want = ref.mix(x32, w_eff)
    bound = ref.mix_bound(x32, w_eff)
    err = np.abs(got.astype(np.float64) - want)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"clip {what}: dist rel {rel_d:.2e} (1e-5), tau rel {rel_t:.2e}, w_eff rel {rel_w:.2e} (2e-5), mix err/bound {worst:.3f}")
    assert np.all(err <= bound), (what, worst)
    unwritten = ~w_eff.any(axis=1)
    assert np.array_equal(got[unwritten].view(np.uint32), x32[unwritten].view(np.uint32)), what  # sources only: bit-identical

    # the result does not depend on alignment, and a repeat call gives the same bits
    for rows in (_offset(x32, dev), _aligned(x32, dev)):
        got2, dist2, tau2, w_eff2 = _run(rows, w, kw)
        assert np.array_equal(got2.view(np.uint32), got.view(np.uint32)), what
        assert np.array_equal(dist2, dist) and np.array_equal(tau2, tau) and np.array_equal(w_eff2, w_eff), what
    return w_eff


def _topology(name, k):
    if k == 1:
        return np.zeros((1, 1))
    return {"ring": ref.ring, "star": ref.star, "full": ref.full}[name](k)


def _far(k):
    return () if k < 3 else (1,) if k < 8 else (1, k - 2)


def _rows(k, n, seed, far, w, b=None):
    """``close_rows`` from the first seed at which the reference's choice of every F_p is clear
    (a handful of coordinates can put two neighbours within 1e-3 of each other by chance)."""
    for s in range(seed, seed + 20):
        x32 = ref.close_rows(k, n, seed=s, far=far)
        if b is None or ref.selection_gap(ref.sqdist(x32), np.asarray(w), b) > 1e-3:
            return x32
    raise AssertionError(("no seed gives a clear selection", k, n, seed, b))


@pytest.mark.parametrize("k", [1, 2, 3, 5, 8, 16])
def test_plan_and_mix_against_the_oracle(dev, k):
    sizes = [1, 3, 4, 5, 1023, 1025] + ([MID, BIG] if k in (5, 16) else [])
    for i, n in enumerate(sizes):
        name = ("ring", "star", "full")[(i + k) % 3]
        w = _topology(name, k)
        x32 = _rows(k, n, 100 * k + i, _far(k), w, b=1)
        modes = [{"tau": _fixed_tau(x32, w)}, {"b": 1}] if n not in (MID, BIG) else [{"b": 1} if n == MID else {"tau": _fixed_tau(x32, w)}]
        for kw in modes:
            _check(x32, w, kw, dev, (k, n, name, kw))


@pytest.mark.parametrize("name", ["ring", "star", "full"])
def test_topologies_and_attacker_bounds(dev, name):
    k, n = 8, 1025
    w = _topology(name, k)
    x32 = ref.close_rows(k, n, seed=7, far=(1, 6))
    for kw in ({"b": 0}, {"b": 1}, {"b": 2}, {"b": 3}, {"tau": 0.0}, {"tau": 1e30}, {"tau": _fixed_tau(x32, w)}):
        w_eff = _check(x32, w, kw, dev, (name, kw))
        if kw in ({"b": 0}, {"tau": 1e30}):
            assert np.array_equal(w_eff, w.astype(np.float32))  # plain mixing in difference form
        if kw == {"tau": 0.0} or (kw == {"b": 2} and name == "ring") or (kw.get("b", 0) >= 1 and name == "star"):
            assert not w_eff[1:].any()  # the whole neighbourhood may be hostile: the row keeps its model
        if kw == {"b": 2} and name == "full":
            assert np.all(w_eff[0, [1, 6]] < 0.05 * w[0, 1]) and np.all(w_eff[0, [2, 3, 4, 5, 7]] > 0.5 * w[0, 2])


def test_source_only_rows(dev):
    """Rows 2 and 5 have an all-zero row of W: their neighbours read them, nobody writes them."""
    k, n = 7, 1023
    x32 = ref.close_rows(k, n, seed=8, far=(2,))
    w = ref.ring(k)
    w[2] = 0
    w[5] = 0
    for kw in ({"b": 1}, {"tau": _fixed_tau(x32, w)}):
        w_eff = _check(x32, w, kw, dev, ("sources", kw))
        assert not w_eff[2].any() and not w_eff[5].any()
        assert w_eff[1, 2] > 0 and w_eff[3, 2] > 0 and w_eff[4, 5] > 0  # still read (clipped: row 2 is far)
        assert w_eff[1, 2] < 0.01 * w[1, 2]


def test_mix_grid_stride(dev):
    """2048 · 256 · 4 + 5 coordinates: the mix kernel's grid-stride loop runs twice, with a tail."""
    n = 2048 * 256 * 4 + 5
    x32 = ref.close_rows(2, n, seed=9)
    x32[1, -3:] += 7.0
    _check(x32, ref.ring(2), {"tau": 1.0}, dev, ("grid-stride", n))


@pytest.mark.parametrize("offset", [False, True])
def test_bit_exact_dyadic_case(dev, offset):
    """Small-integer rows, a leaf differing from the hub in one coordinate by 2, 4, 8, 16; shares
    0.25 and 0.5; τ = 4: the scales are 1, 1, 0.5, 0.25 and every product is exact, so the distances,
    ``w_eff`` and the rows equal the float64 oracle bit for bit."""
    k, n = 5, 37
    rng = np.random.default_rng(5)
    x32 = np.tile(rng.integers(-8, 9, size=n).astype(np.float32), (k, 1))
    for q, c in zip(range(1, k), (2.0, 4.0, 8.0, 16.0)):
        x32[q, 3 + 8 * q] += c
    w = np.zeros((k, k), dtype=np.float32)
    w[0, 1:] = 0.25
    w[1:, 0] = 0.5
    want, d_ref, tau_ref, _, w_ref = ref.clipped_gossip(x32, w, tau=4.0)
    assert np.array_equal(w_ref[0, 1:], np.float32([0.25, 0.25, 0.125, 0.0625])) and np.array_equal(w_ref[1:, 0], np.float32([0.5, 0.5, 0.25, 0.125]))
    got, dist, tau, w_eff = _run((_offset if offset else _aligned)(x32, dev), w, {"tau": 4.0})
    assert np.array_equal(dist, d_ref) and np.array_equal(tau, tau_ref) and np.array_equal(w_eff, w_ref)
    assert np.array_equal(got.astype(np.float64), want)
    assert not np.array_equal(got, x32)


def test_nonfinite_rows(dev):
    """Row 1 holds a NaN, row 4 is 1e30 (its differences overflow fp32): neither reaches a
    neighbour, every other row stays finite and mixes its finite neighbours as the oracle says, and
    both are left as they are where they are written rows."""
    k, n = 6, 1025
    x32 = ref.close_rows(k, n, seed=10)
    x32[1, 77] = np.nan
    x32[4, :] = 1e30
    w = ref.ring(k).astype(np.float32)
    for kw in ({"tau": _fixed_tau(x32[[0, 2, 3, 5]], ref.full(4))}, {"b": 1}, {"b": 0}):
        got, dist, tau, w_eff = _run(_aligned(x32, dev), w, kw)
        assert not w_eff[:, 1].any() and not w_eff[:, 4].any() and not w_eff[1].any() and not w_eff[4].any(), kw
        assert np.array_equal(got[[1, 4]].view(np.uint32), x32[[1, 4]].view(np.uint32)), kw
        finite = [0, 2, 3, 5]
        assert np.isfinite(got[finite]).all(), kw
        err = np.abs(got.astype(np.float64) - ref.mix(x32, w_eff))[finite]
        assert np.all(err <= ref.mix_bound(x32, w_eff)[finite]), kw
        # rows 0 and 2 neighbour the NaN row and a finite one: the finite one's share is the oracle's
        _, _, _, _, w_ref = ref.clipped_gossip(x32, w, **kw)
        for p, q in ((0, 5), (2, 3)):
            if "tau" in kw or kw["b"] == 0:
                np.testing.assert_allclose(w_eff[p, q], w_ref[p, q], rtol=2e-5, atol=0)
                assert w_eff[p, q] > 0
        if kw == {"b": 1}:  # the NaN neighbour is the one set aside: the radius is the finite neighbour's distance
            np.testing.assert_allclose(tau[[0, 2]], np.sqrt([ref.sqdist(x32)[0, 5], ref.sqdist(x32)[2, 3]]), rtol=2e-5, atol=0)
            assert w_eff[0, 5] == w[0, 5] and w_eff[2, 3] == w[2, 3]


def test_rejects_launch_nothing(dev):
    from myfyp_amd import ops
    from myfyp_amd.ops import _native

    lib = _native.load(required=True)
    k, n = 17, 64
    x = torch.arange(k * n, dtype=torch.float32, device=dev).reshape(k, n)
    before = x.clone()
    dist = torch.full((k * k,), -1.0, dtype=torch.float64, device=dev)
    tau = torch.full((k,), -1.0, dtype=torch.float64, device=dev)
    w_eff = torch.full((k * k,), -1.0, dtype=torch.float32, device=dev)
    work = torch.zeros(1 << 16, dtype=torch.float32, device=dev)
    ptrs = (ctypes.c_uint64 * k)(*[x[i].data_ptr() for i in range(k)])
    stream = torch.cuda.current_stream().cuda_stream

    def call(kk, w, mode, t, b, nn, rows=ptrs):
        w = np.ascontiguousarray(w, dtype=np.float32)
        return int(lib.myfyp_clipped_gossip(ctypes.cast(rows, ctypes.c_void_p), kk, w.ctypes.data, mode, float(t), b, nn, work.data_ptr(), dist.data_ptr(),
                                            tau.data_ptr(), w_eff.data_ptr(), stream))

    bad = ref.ring(4)
    bad[1, 2] = -0.25
    nan = ref.ring(4)
    nan[0, 1] = np.nan
    for args in ((17, ref.ring(17), 0, 1.0, 0, n), (0, ref.ring(2), 0, 1.0, 0, n), (4, ref.ring(4), 0, 1.0, 0, 0), (4, bad, 0, 1.0, 0, n),
                 (4, nan, 1, 0.0, 1, n), (4, ref.ring(4), 0, -1.0, 0, n), (4, ref.ring(4), 0, float("nan"), 0, n), (4, ref.ring(4), 1, 0.0, -1, n),
                 (4, ref.ring(4), 2, 1.0, 1, n)):
        assert call(*args) == 2, args
        assert lib.myfyp_last_error()
    rows = [x[i] for i in range(4)]
    for kw in ({}, {"tau": 1.0, "num_byzantine": 1}):
        with pytest.raises(ValueError, match="exactly one"):
            ops.clipped_gossip_into(rows, ref.ring(4), **kw)
    with pytest.raises(ValueError):
        ops.clipped_gossip_into(rows, bad, tau=1.0)
    torch.cuda.synchronize()
    assert torch.equal(x, before) and bool((dist == -1).all()) and bool((tau == -1).all()) and bool((w_eff == -1).all())
    # one row: nothing to do, and it succeeds
    assert call(1, np.zeros((1, 1)), 1, 0.0, 1, n) == 0
    torch.cuda.synchronize()
    assert torch.equal(x, before) and bool((dist == -1).all())
    d1, t1, w1 = ops.clipped_gossip_into([x[0]], np.zeros((1, 1)), num_byzantine=1)
    assert float(d1) == 0 and float(w1) == 0 and torch.equal(x, before)
