"""Every row count K of every robust aggregator of ``csrc/kernels/fl_ops.hip``, on rows that take the
float4 path and on rows that take the scalar path (MI355X only).

The host side of ``fl_ops.hip`` turns the run-time K (and Bulyan's f, and the alignment of the rows)
into template arguments through one dispatcher. The kernel tests of each family visit a handful of K;
a dispatcher can be wrong at exactly the values they skip, so this file visits all of them, K from the
family's lowest to 16, at two sizes: n = 5 (less than two float4 groups, all tail) and n = 1027 (257
groups: two blocks, so more than one slab to sum, and n % 4 = 3). Rows are laid out once 16-byte aligned
and once as the rows of a packed ``[K, n]`` buffer (n is odd: the odd rows are 4-byte aligned only).

(a) every device output of the unaligned call is bit-equal to the aligned call's (``fl_ops.h``);
(b) the aligned call agrees with the family's oracle. Inputs, oracles, comparison helpers and bounds
    are those of ``test_robust_oracle_gpu.py`` (median, trimmed mean, Krum: bit for bit, which gives
    (a) as well) and of ``test_{bulyan,geomed,dnc,clip,collude}_kernels_gpu.py``; none is new here.
"""

import functools

import numpy as np
import pytest
import torch

import _collude_ref as cr
import _dnc_ref as dref
import _robust_ref as R
import test_bulyan_kernels_gpu as B
import test_clip_kernels_gpu as C
import test_collude_kernels_gpu as A
import test_dnc_kernels_gpu as D
import test_geomed_kernels_gpu as G
import test_robust_oracle_gpu as O
from myfyp_amd import ops

pytestmark = pytest.mark.gpu

NS = [5, 1027]
KS = range(1, 17)


@pytest.fixture(scope="module")
def dev():
    from myfyp_amd.ops import _native

    _native.load(required=True)  # the native path must be the one under test
    return torch.device("cuda")


def _layouts(x, dev):
    """(aligned rows, rows of a packed buffer) of x [K, n], n odd."""
    x = np.asarray(x)
    assert x.shape[1] % 2
    return O._rows(x, dev), O._rows(x, dev, packed=True)


def _same_bits(ra, ru, what):
    for a, u in zip(ra, ru):
        assert a.dtype == u.dtype and torch.equal(a.view(torch.uint8), u.view(torch.uint8)), what


@pytest.mark.parametrize("k", KS)
def test_median_and_trimmed_mean(dev, k):
    for n in NS:
        O._check_sorts(R.trim_rows(k, n), dev, sorted({0, (k - 1) // 2}), f"K={k} n={n}")  # both layouts against the oracle's bits


@pytest.mark.parametrize("k", KS)
def test_krum_with_its_mean(dev, k):
    f, m = 1, 3
    w = [float(1 + (3 * i) % 5) for i in range(k)]
    for n in NS:
        x = R.exact_rows(k, n)
        want = R.krum(x, w, f, m)
        means = {}
        for packed in (False, True):
            what = f"K={k} n={n} packed={packed}"
            out = torch.empty(k + 1, n, device=dev)[1] if packed else torch.empty(n, device=dev)
            dist, score, coef = ops.krum_into(O._rows(x, dev, packed), [out], w, f, m)
            O._assert_bits(O._np(dist), want["dist"], "dist " + what)
            O._assert_bits(O._np(score), want["score"], "score " + what)
            O._assert_bits(O._np(coef), want["coef"], "coef " + what)
            assert sorted(np.flatnonzero(O._np(coef) != 0)) == want["chosen"], what
            means[packed] = O._np(out)
            O._check_mean(means[packed], want, x, list(range(k)), m, "mean " + what)
        assert np.array_equal(means[False].view(np.uint32), means[True].view(np.uint32)), (k, n)


@pytest.mark.parametrize("k", KS)
def test_bulyan(dev, k):
    for f in [f for f in range(4) if f == 0 or k >= 4 * f + 3]:
        for n in NS:
            what = f"K={k} f={f} n={n}"
            x, _, coef, pick, mean64, _ = B._case(k, f, n)
            rows_a, rows_u = _layouts(x, dev)
            out_a, out_u = torch.empty(n, device=dev), torch.empty(2, n, device=dev)[1]
            ra = ops.bulyan_into(rows_a, [out_a], f)
            ru = ops.bulyan_into(rows_u, [out_u], f)
            _same_bits([*ra, out_a], [*ru, out_u], what)
            assert np.array_equal(ra[3].cpu().numpy(), pick), what
            assert np.array_equal(ra[2].cpu().numpy(), coef), what
            bound = (k - 4 * f) * B.U * float(np.abs(x).max())
            assert float(np.abs(out_a.cpu().numpy().astype(np.float64) - mean64).max()) <= bound, what


@pytest.mark.parametrize("k", KS)
def test_geometric_median(dev, k):
    w = G._weights(k)
    what = np.asarray(w)
    for n in NS:
        x, x64 = G._case(k, n)
        rows_a, rows_u = _layouts(x.numpy(), dev)
        out_a, out_u = torch.empty(n, device=dev), torch.empty(2, n, device=dev)[1]
        c_prev = (what / what.sum()).astype(np.float32)
        for t in range(2):  # the steps of test_steps_against_float64, with its bounds
            coef, dist, obj = G._run(rows_a, [out_a], w, t + 1)
            d, o, c_next, a, un = G._step64(x64, what, c_prev)
            bound = G._dist_bound(k, n, d, a, un)
            with np.errstate(divide="ignore", invalid="ignore"):
                rel = np.where(d > 0, np.abs(dist - d) / d, np.abs(dist))
            rel_o = abs(obj[t] - o) / o if o > 0 else abs(obj[t])
            rel_c = np.abs(coef.astype(np.float64) - c_next) / c_next
            assert np.all(rel <= bound) and rel_o <= bound.max(), (k, n, t, rel, rel_o, bound)
            assert np.all(rel_c <= 1.01 * (bound + bound.max()) + 2 * G.U), (k, n, t, rel_c)
            c_prev = coef
        want = (coef.astype(np.float64)[:, None] * x64).sum(axis=0)
        assert float(np.abs(out_a.double().cpu().numpy() - want).max()) <= k * G.U * float(np.abs(x64).max()), (k, n)
        got_u = G._run(rows_u, [out_u], w, 2)
        for p, q in zip((coef, dist, obj), got_u):
            assert np.array_equal(p, q), (k, n)
        assert torch.equal(out_a, out_u), (k, n)


@functools.lru_cache(maxsize=None)
def _dnc_case(k, f, n, iters, b):
    """The first (gs, seed) of the kernel tests' generator at which the oracle's selection is exact
    (the condition of test_dnc_kernels_gpu.test_selection_and_output)."""
    for gs in (1.0, 3.0, 8.0):
        for seed in range(4):
            x, bad, want = D._case(k, f, n, seed, gs, iters, b)
            ratio, margin = D.condition(want, f, iters)
            if ratio <= 0.9 and margin >= 2.0 and sorted(np.flatnonzero(want["removed"] >= 0).tolist()) == bad:
                return x, want
    raise AssertionError(("no input with an exact selection", k, f, n, iters, b))


@pytest.mark.parametrize("k", KS)
def test_dnc(dev, k):
    w = D._weights(k)
    f = 0 if k < 3 else 1 if k < 8 else 2 if k < 16 else 3
    for n, iters, b in [(5, 1, None), (1027, 1, None), (1027, 2 if 2 * f < k else 1, 300)]:  # the last: 5 tiles, a subsample
        label = (k, f, n, iters, b)
        if f == 0:
            x, _, want = D._case(k, 0, n, 0, 1.0, iters, b)  # no attacker, nothing to select: any seed does
        else:
            x, want = _dnc_case(k, f, n, iters, b)
        rows_a, rows_u = _layouts(x, dev)
        out_a, out_u = torch.empty(n, device=dev), torch.empty(2, n, device=dev)[1]
        ra = ops.dnc_into(rows_a, [out_a], w, f, 1.0, iters, b, seed=D.SEED, round=D.ROUND)
        ru = ops.dnc_into(rows_u, [out_u], w, f, 1.0, iters, b, seed=D.SEED, round=D.ROUND)
        _same_bits([*ra, out_a], [*ru, out_u], label)
        if f > 0:
            D._check(ra, x, want, f, iters, label)
        else:  # nothing to remove (test_f_zero_is_the_weighted_mean): every row kept, its share of the weights
            assert ra[3].tolist() == [-1] * k, label
            assert np.array_equal(ra[4].cpu().numpy(), (np.array(w) / sum(w)).astype(np.float32)), label
            off = ~np.eye(k, dtype=bool)
            for t in range(iters if k > 1 else 0):
                d64 = want["dist"][t]
                assert float((np.abs(ra[0][t].cpu().numpy() - d64)[off] / d64[off]).max()) <= dref.DIST_RTOL, label
        kept = int((want["coef"] != 0).sum())
        err = float(np.abs(out_a.cpu().numpy().astype(np.float64) - want["out"]).max())
        assert err <= kept * D.U * float(np.abs(x).max()), (label, err)


@pytest.mark.parametrize("k", range(2, 17))
def test_clipped_gossip(dev, k):
    for i, n in enumerate(NS):
        w = C._topology(("ring", "star", "full")[(i + k) % 3], k)
        x32 = C._rows(k, n, 100 * k + i, C._far(k), w, b=1)
        for kw in ({"tau": C._fixed_tau(x32, w)}, {"b": 1}):
            what = (k, n, kw)
            C._check(x32, w, kw, dev, what)  # the oracle, and rows one float past a 16-byte boundary
            got_a = C._run(O._rows(x32, dev), np.asarray(w, dtype=np.float32), kw)
            got_u = C._run(O._rows(x32, dev, packed=True), np.asarray(w, dtype=np.float32), kw)
            assert np.array_equal(got_a[0].view(np.uint32), got_u[0].view(np.uint32)), what
            for p, q in zip(got_a[1:], got_u[1:]):
                assert np.array_equal(p, q), what


@pytest.mark.parametrize("kind", cr.KINDS)
@pytest.mark.parametrize("h", KS)
def test_collude(dev, h, kind):
    for n in NS:
        A._check(dev, kind, h, 1, n)
        x, _, ref, _ = cr.case(h, n)
        rows_a, rows_u = _layouts(x.numpy(), dev)
        r_dev = ref.to(dev) if kind == "ipm" else None
        out_a, out_u = torch.empty(n, device=dev), torch.empty(2, n, device=dev)[1]
        ra = ops.collude_into(rows_a, [out_a], kind, z=A.Z, eps=A.EPS, ref=r_dev)
        ru = ops.collude_into(rows_u, [out_u], kind, z=A.Z, eps=A.EPS, ref=r_dev)
        _same_bits([*ra, out_a], [*ru, out_u], (kind, h, n))
