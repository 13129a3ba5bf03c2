"""The DnC kernels of ``csrc/kernels/fl_ops.hip`` (``k_dnc_sqdist<K>``, ``k_dnc_select``, then
``k_coef_mean<K>``) against the float64 oracle of ``tests/_dnc_ref.py`` — MI355X only.

``dist``. With every tile taken and one iteration the slabs are ``k_pairwise_sqdist``'s, so ``dist``
is ``ops.krum_into``'s bit for bit. Otherwise the same fp32 chain over fewer coordinates: every term
is positive, a chain of depth L is within (L + 3)·2^-24 relative, the slab sum is in double — the
bound the Krum kernel tests hold a distance to, ε = 1e-5 relative (``tests/test_robust_kernels_gpu.py``).

``lam`` and ``score``, from D's bound. G = −½·J·D·J is linear in D and ‖J‖₂ = 1, so a perturbation
|ΔD_ij| <= ε·D_ij moves G by ‖ΔG‖₂ <= ½‖ΔD‖₂ <= ½‖ΔD‖_F <= η = ½·ε·‖D‖_F. Repeated squaring (2^20-th
power of G, normalised) leaves (λ₂/λ₁)^(2^20) of the other directions: nothing in double for
λ₂/λ₁ <= 0.9, so both sides hold the top eigenpair of their G to double rounding (1e-12 relative
covers the double arithmetic: 20 squarings of a 16 × 16 matrix). Weyl: |Δλ| <= η. Davis–Kahan (Yu,
Wang, Samworth 2015): sin θ <= 2η / (λ₁ − λ₂) between the two top eigenvectors, so with the signs
aligned |Δu_i| <= δ = √2·sin θ, and s_i = λ·u_i² does not see the sign:
|Δs_i| <= |Δλ|·u_i'² + λ·|u_i'² − u_i²| <= η + λ·δ·(2|u_i| + δ).

``removed`` and ``coef`` are exact. That is a condition on the case, not a measurement: each case
first asserts that the oracle has λ₂/λ₁ <= 0.9 and that the last removed score is at least twice the
first kept score in every iteration (the bounds above are ~1e-4 of λ; a factor 2 is far outside
them), and the seeds are chosen so that every case meets it. ``coef`` is
``float32(w_k / Σ_kept w)`` with the sum in double in ascending row order on both sides.

``out``: ``k_coef_mean<K>``'s bound, one fused multiply-add per kept row with coefficients that sum
to 1: ``kept · 2^-24 · max|x|`` against the float64 ``Σ coef_k·x_k``.

Rows: honest = base + 1e-3·noise, attackers = μ − gs·γ·σ with min-max's γ (``_dnc_ref.attacked``).
"""

import functools

import numpy as np
import pytest
import torch

import _dnc_ref as ref
from myfyp_amd import ops

U = 2.0**-24
BIG = 600_001  # past one grid stride of the 512-block grid (512 · 256 · 4 coordinates), ragged tail

# (K, f, n, seed, gs, iters, subsample_dims); the seeds are the lowest that meet the condition above
ALL_TILES = [(k, f, n, seed, gs, 1, None) for (k, f, gs), by_n in {
    (3, 1, 3.0): {255: 0, 256: 0, 257: 0, 1000: 0},
    (3, 1, 8.0): {1: 0, 3: 0},  # three points on a line: the mean follows the attacker, which has to go far to stand out
    (5, 1, 3.0): {1: 1, 3: 0, 255: 0, 256: 0, 257: 0, 1000: 0, BIG: 0},
    (8, 2, 1.0): {255: 0, 256: 1, 257: 1, 1000: 0},
    (8, 2, 3.0): {1: 1, 3: 1},
    (16, 3, 1.0): {255: 0, 256: 0, 257: 0, 1000: 0, BIG: 0},
    (16, 3, 3.0): {1: 0, 3: 0},
}.items() for n, seed in by_n.items()]
MORE = [(8, 2, 1000, 0, 1.0, 3, None), (16, 3, 257, 0, 1.0, 3, None), (8, 2, 1000, 0, 1.0, 1, 300), (8, 2, 1000, 0, 1.0, 3, 300),
        (16, 3, 1000, 0, 1.0, 3, 500), (3, 1, 257, 0, 3.0, 1, 100), (5, 1, 1000, 0, 3.0, 3, 300), (16, 3, BIG, 0, 1.0, 1, 10000),
        (16, 3, BIG, 0, 1.0, 3, 10000), (5, 1, BIG, 0, 3.0, 3, 10000)]
CASES = ALL_TILES + MORE
SEED, ROUND = 11, 2  # of the subsample


@pytest.fixture(scope="module")
def dev():
    from myfyp_amd.ops import _native

    _native.load(required=True)  # the native path must be the one under test
    return torch.device("cuda")


def _weights(k):
    return [float(5 + (3 * i) % 7) for i in range(k)]


@functools.lru_cache(maxsize=None)
def _case(k, f, n, seed, gs, iters, b):
    """(rows fp32 [K, n], attackers, oracle dict): computed once, never written."""
    x, bad = ref.attacked(k, f, n, seed, gs)
    return x, bad, ref.dnc(x, _weights(k), f, 1.0, iters, b, seed=SEED, rnd=ROUND)


def condition(want, f, iters):
    """(largest λ₂/λ₁, smallest removed/kept score margin) over the iterations."""
    return max(ref.eig_ratio(g) for g in want["g"]), min(ref.margin(want["score"][t], f) for t in range(iters))


def _dev_rows(x, dev):
    return [torch.from_numpy(np.array(r)).to(dev) for r in x]


def _check(got, x, want, f, iters, label):
    dist, score, lam, removed, coef = [t.cpu().numpy() for t in got]
    worst = 0.0
    for t in range(iters):
        d = want["dist"][t]
        pos = d > 0
        assert np.all(dist[t][~pos] == 0) and np.array_equal(dist[t], dist[t].T)
        rel = float((np.abs(dist[t] - d)[pos] / d[pos]).max())
        assert rel <= ref.DIST_RTOL, (label, t, rel)
        b_lam, b_s = ref.bounds(d, want["g"][t], want["lam"][t], want["u"][t])
        e_lam = abs(lam[t] - want["lam"][t]) / b_lam
        e_s = float((np.abs(score[t] - want["score"][t]) / b_s).max())
        worst = max(worst, e_lam, e_s)
        assert e_lam <= 1 and e_s <= 1, (label, t, e_lam, e_s)
    assert removed.tolist() == want["removed"].tolist(), label
    assert np.array_equal(coef, want["coef"]), label
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("k,f,n,seed,gs,iters,b", CASES)
def test_selection_and_output(dev, k, f, n, seed, gs, iters, b):
    x, bad, want = _case(k, f, n, seed, gs, iters, b)
    ratio, margin = condition(want, f, iters)
    assert ratio <= 0.9 and margin >= 2.0, (ratio, margin)  # the condition of an exact selection
    assert sorted(np.flatnonzero(want["removed"] >= 0).tolist()) == bad
    rows = _dev_rows(x, dev)
    outs = [torch.full((n,), float("nan"), device=dev) for _ in range(3)]
    got = ops.dnc_into(rows, outs, _weights(k), f, 1.0, iters, b, seed=SEED, round=ROUND)
    assert got[0].shape == (iters, k, k) and got[0].dtype == torch.float64 and got[1].shape == (iters, k) and got[2].shape == (iters,)
    assert got[3].dtype == torch.int32 and got[4].dtype == torch.float32
    worst = _check(got, x, want, f, iters, (k, f, n, iters, b))
    if iters == 1 and (b is None or n <= b):
        kd = ops.krum_into(rows, [], [1.0] * k, f, 1)[0]
        assert torch.equal(got[0][0], kd)  # the same bits
    kept = int((want["coef"] != 0).sum())
    bound = kept * U * float(np.abs(x).max())
    err = float(np.abs(outs[0].cpu().numpy().astype(np.float64) - want["out"]).max())
    print(f"K={k} f={f} n={n} iters={iters} b={b}: lambda2/lambda1 {ratio:.3f}, margin {margin:.2f}, worst score/lam error over bound "
          f"{worst:.3e}, out error {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    assert all(torch.equal(o, outs[0]) for o in outs[1:])
    for r, r0 in zip(rows, x):
        assert np.array_equal(r.cpu().numpy(), r0)  # the rows are only read


@pytest.mark.gpu
@pytest.mark.parametrize("k,n", [(2, 1), (2, 3), (2, 257), (2, 1000), (16, 1000), (1, 5), (1, 1000)])
def test_f_zero_is_the_weighted_mean(dev, k, n):
    x = np.random.default_rng(k + n).standard_normal((k, n)).astype(np.float32)
    w = _weights(k)
    out = torch.empty(n, device=dev)
    dist, score, lam, removed, coef = ops.dnc_into(_dev_rows(x, dev), [out], w, 0)
    assert removed.tolist() == [-1] * k
    wn = np.array(w) / sum(w)
    assert np.array_equal(coef.cpu().numpy(), wn.astype(np.float32))
    want = (coef.cpu().numpy().astype(np.float64)[:, None] * x.astype(np.float64)).sum(0)
    assert float(np.abs(out.cpu().numpy() - want).max()) <= k * U * float(np.abs(x).max())
    d64 = ref.sqdist(x)
    if k > 1:
        off = ~np.eye(k, dtype=bool)
        assert float((np.abs(dist[0].cpu().numpy() - d64)[off] / d64[off]).max()) <= ref.DIST_RTOL
    else:
        assert dist.tolist() == [[[0.0]]] and score.tolist() == [[0.0]] and lam.tolist() == [0.0]


@pytest.mark.gpu
@pytest.mark.parametrize("k,f,n,seed,gs,iters,b", [(8, 2, 257, 0, 1.0, 1, None), (16, 3, 1001, 0, 1.0, 3, 500), (5, 1, 255, 0, 3.0, 1, None),
                                                  (3, 1, 3, 0, 3.0, 1, None)])
def test_unaligned_packed_rows(dev, k, f, n, seed, gs, iters, b):
    """Row i of a packed [K, n] buffer with odd n is only 4-byte aligned (the scalar path): the
    same bits as aligned copies."""
    x = _case(k, f, n, seed, gs, iters, b)[0]
    w = _weights(k)
    packed = torch.from_numpy(np.array(x)).to(dev).contiguous()
    rows_u = [packed[i] for i in range(k)]
    assert any(r.data_ptr() % 16 for r in rows_u)
    rows_a = _dev_rows(x, dev)
    assert all(r.data_ptr() % 16 == 0 for r in rows_a)
    out_a = torch.empty(n, device=dev)
    out_u = torch.empty(k, n, device=dev)
    ra = ops.dnc_into(rows_a, [out_a], w, f, 1.0, iters, b, seed=SEED, round=ROUND)
    ru = ops.dnc_into(rows_u, [out_u[1], out_u[2]], w, f, 1.0, iters, b, seed=SEED, round=ROUND)
    assert all(torch.equal(p, q) for p, q in zip(ra, ru))
    assert torch.equal(out_u[1], out_a) and torch.equal(out_u[2], out_a)


@pytest.mark.gpu
def test_two_calls_give_the_same_bits(dev):
    k, f, n, seed, gs, iters, b = 16, 3, BIG, 0, 1.0, 3, 10000
    rows = _dev_rows(_case(k, f, n, seed, gs, iters, b)[0], dev)
    a, c = torch.empty(n, device=dev), torch.empty(n, device=dev)
    ra = ops.dnc_into(rows, [a], _weights(k), f, 1.0, iters, b, seed=SEED, round=ROUND)
    rb = ops.dnc_into(rows, [c], _weights(k), f, 1.0, iters, b, seed=SEED, round=ROUND)
    assert torch.equal(a, c) and all(torch.equal(p, q) for p, q in zip(ra, rb))
    # another round draws another subsample
    rc = ops.dnc_into(rows, [], _weights(k), f, 1.0, iters, b, seed=SEED, round=ROUND + 1)
    assert not torch.equal(rc[0], ra[0]) and torch.equal(rc[3], ra[3])


@pytest.mark.gpu
def test_subsample_is_the_oracles_tiles(dev):
    """Rows that differ in one tile only: the distance of an iteration is non-zero exactly when the
    oracle's mask takes that tile."""
    n, iters, b = 40 * 256, 8, 2000
    masks = ops.dnc_tiles(n, SEED, ROUND, iters, b)[3]
    tiles = [t for t in range(40) if 0 < masks[:, t].sum() < iters][:3]
    assert tiles
    for tile in tiles:
        x = np.zeros((2, n), dtype=np.float32)
        x[1, tile * 256 : (tile + 1) * 256] = 1.0
        dist = ops.dnc_into(_dev_rows(x, dev), [], [1.0, 1.0], 0, 1.0, iters, b, seed=SEED, round=ROUND)[0]
        assert dist[:, 0, 1].tolist() == [256.0 if masks[t, tile] else 0.0 for t in range(iters)]


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_a_non_finite_row_is_removed(dev, bad):
    k, f, n = 8, 2, 1000
    x, att = ref.attacked(k, f, n, 0, 1.0)
    x = x.copy()
    x[5, 17] = bad
    w = _weights(k)
    out = torch.empty(n, device=dev)
    dist, score, lam, removed, coef = ops.dnc_into(_dev_rows(x, dev), [out], w, f, subsample_dims=None)
    want = ref.dnc(x, w, f, 1.0, 1, None)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(lam).all())
    assert float(score[0, 5]) == float("inf") and int(removed[5]) == 0 and float(coef[5]) == 0.0
    assert removed.tolist() == want["removed"].tolist() and np.array_equal(coef.cpu().numpy(), want["coef"])
    kept = int((want["coef"] != 0).sum())
    assert float(np.abs(out.cpu().numpy().astype(np.float64) - want["out"]).max()) <= kept * U * float(np.abs(x[want["coef"] != 0]).max())
    # every row bad: nothing is kept, the weights of all rows come back
    y = np.full((4, 9), np.nan, dtype=np.float32)
    _, s2, _, r2, c2 = ops.dnc_into(_dev_rows(y, dev), [], [1.0, 2.0, 3.0, 4.0], 1)
    assert r2.tolist() == [0, 0, 0, 0] and bool(torch.isinf(s2).all())
    assert np.array_equal(c2.cpu().numpy(), (np.array([1.0, 2.0, 3.0, 4.0]) / 10.0).astype(np.float32))


@pytest.mark.gpu
def test_identical_rows_tie_towards_the_higher_row(dev):
    row = np.random.default_rng(1).standard_normal(1027).astype(np.float32)
    x = np.stack([row] * 7)
    _, score, lam, removed, coef = ops.dnc_into(_dev_rows(x, dev), [], [1.0] * 7, 2)
    assert score.tolist() == [[0.0] * 7] and lam.tolist() == [0.0]
    assert removed.tolist() == [-1, -1, -1, -1, -1, 0, 0]
    assert np.array_equal(coef.cpu().numpy(), np.array([0.2] * 5 + [0.0] * 2, dtype=np.float32))


@pytest.mark.gpu
def test_argument_errors_native(dev):
    """The C entry point refuses bad arguments with a message before any launch."""
    import ctypes

    from myfyp_amd.ops import _native

    lib = _native.load(required=True)
    n = 8
    rows = [torch.zeros(n, device=dev) for _ in range(17)]
    out = torch.full((n,), 7.0, device=dev)
    src = (ctypes.c_uint64 * 17)(*[r.data_ptr() for r in rows])
    dst = (ctypes.c_uint64 * 1)(out.data_ptr())
    w = (ctypes.c_float * 17)(*([1.0] * 17))
    keys = (ctypes.c_uint64 * 8)()
    work = torch.empty(8 * 4096, device=dev)
    dist = torch.empty(8 * 17 * 17, dtype=torch.float64, device=dev)
    score = torch.empty(8 * 17, dtype=torch.float64, device=dev)
    lam = torch.empty(8, dtype=torch.float64, device=dev)
    removed = torch.full((17,), 5, dtype=torch.int32, device=dev)
    coef = torch.empty(17, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    vp = ctypes.c_void_p

    def call(k_, m_, iters_, n_, p_=1, work_=work.data_ptr(), removed_=removed.data_ptr(), all_=1, keys_=ctypes.cast(keys, vp)):
        rc = lib.myfyp_dnc_multi(ctypes.cast(dst, vp), p_, ctypes.cast(src, vp), ctypes.cast(w, vp), k_, m_, iters_, keys_, 2**64 - 1, keys_, all_, n_,
                                 work_, dist.data_ptr(), score.data_ptr(), lam.data_ptr(), removed_, coef.data_ptr(), st)
        return rc, lib.myfyp_last_error().decode()

    for args, word in [((6, 6, 1, n), "iters * m < K"), ((6, 2, 3, n), "iters * m < K"), ((6, -1, 1, n), "m >= 0"), ((6, 1, 0, n), "iters"),
                       ((6, 1, 9, n), "iters"), ((17, 1, 1, n), "1..16 rows"), ((0, 0, 1, n), "1..16 rows"), ((6, 1, 1, 0), "n >= 1"),
                       ((6, 1, 1, n, 17), "1..16 rows"), ((6, 1, 1, n, 1, None), "required"), ((6, 1, 1, n, 1, work.data_ptr(), None), "required"),
                       ((6, 1, 1, n, 1, work.data_ptr(), removed.data_ptr(), 0, None), "keys")]:
        rc, msg = call(*args)
        assert rc == 2 and word in msg, (args, rc, msg)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((removed == 5).all())  # nothing was launched
    with pytest.raises(ValueError, match="K = 6"):
        ops.dnc_into(rows[:6], [out], [1.0] * 6, 6)
