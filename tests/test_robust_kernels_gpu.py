"""The trimmed-mean and Krum kernels of ``csrc/kernels/fl_ops.hip`` (``k_trimmed_mean<K>``,
``k_pairwise_sqdist<K>``, ``k_krum_select``, ``k_coef_mean<K>``) against float64 (MI355X only).

Bounds. Trimmed mean: a sequential fp32 sum of at most K terms and one division, each rounding at
most 2^-24 of a partial sum no larger than K·max|x|/K after the division: ``K · 2^-24 · max|x|``.
Distances: every term is positive, so an fp32 addition chain of depth L is within (L + 3)·2^-24
relative; the chain here is one add per grid-stride step, 6 wave steps and 3 block steps, and the
slab sum is in double, far inside ``rtol = 1e-5``. Krum mean: m fused multiply-adds with
coefficients that sum to 1: ``m · 2^-24 · max|x|``.
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BIG = 524291  # 2048 * 256 + 3: the grid-stride loop runs more than once, and a tail


@pytest.fixture(scope="module")
def dev():
    from myfyp_amd.ops import _native

    _native.load(required=True)  # the native path must be the one under test
    return torch.device("cuda")


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _trim_ref(x64, trim):
    k = x64.shape[0]
    return torch.sort(x64, dim=0)[0][trim : k - trim].mean(dim=0)


def _check_trimmed(rows, trim):
    from myfyp_amd import ops

    k = len(rows)
    x64 = torch.stack(rows).double()
    want = _trim_ref(x64, trim)
    atol = k * 2.0**-24 * float(x64.abs().max())
    outs = [rows[0], rows[k - 1]] if k > 1 else [rows[0], torch.empty_like(rows[0])]  # aliases two of the rows
    ops.trimmed_mean_into(rows, outs, trim)
    for o in outs:
        err = float((o.double() - want).abs().max())
        print(f"trimmed K={k} trim={trim} n={rows[0].numel()}: max err {err:.3e} (bound {atol:.3e})")
        assert err <= atol, (k, trim, rows[0].numel(), err, atol)


@pytest.mark.parametrize("k", [1, 2, 5, 8, 16])
def test_trimmed_mean(dev, k):
    for n in (1, 7, 1001, BIG):
        for trim in sorted({0, 1 if k > 2 else 0, (k - 1) // 2}):
            x = _randn((k, n), 100 * k + trim).to(dev)
            _check_trimmed([x[i].clone() for i in range(k)], trim)


def _close_rows(k, n, seed, flipped=5):
    """Peers that start from one model: rows differ by ~1e-3 of their norm; one is sign-flipped."""
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(n, generator=g)
    rows = [base + 1e-3 * (1 + 0.15 * i) * torch.randn(n, generator=g) for i in range(k)]
    if flipped is not None and flipped < k:
        rows[flipped] = -base
    return rows


def _krum_ref(x64, w, f, m):
    """float64 distances from differences, scores, the m best (stable order) and their coefficients."""
    k = x64.shape[0]
    d = torch.zeros(k, k, dtype=torch.float64)
    for i in range(k):
        for j in range(i + 1, k):
            d[i, j] = d[j, i] = float((x64[i] - x64[j]).square().sum())
    d = d.numpy()
    cnt = min(max(1, k - f - 2), k - 1)
    scores = np.array([np.sort(np.delete(d[i], i))[:cnt].sum() for i in range(k)])
    chosen = np.argsort(scores, kind="stable")[: max(1, min(m, k))]
    coef = np.zeros(k)
    coef[chosen] = np.asarray(w, dtype=np.float64)[chosen] / sum(w[i] for i in chosen)
    return d, scores, coef


def _check_distances(rows, f=1, m=3, flipped=5):
    from myfyp_amd import ops

    k = len(rows)
    x64 = torch.stack(rows).double()
    d_ref, s_ref, coef_ref = _krum_ref(x64, [1.0] * k, f, m)
    srt = np.sort(s_ref)
    gaps = (srt[1:] - srt[:-1]) / srt[1:]
    assert gaps.min() > 1e-3, gaps  # the reference's own order is not a coin toss
    dist, score, coef = ops.krum_into(rows, [], [1.0] * k, f, m)
    dist, score, coef = dist.cpu().numpy(), score.cpu().numpy(), coef.cpu().numpy()
    off = ~np.eye(k, dtype=bool)
    rel = np.abs(dist[off] - d_ref[off]) / d_ref[off]
    print(f"krum K={k} n={rows[0].numel()}: max rel distance err {rel.max():.3e} (bound 1e-5), min score gap {gaps.min():.3e}")
    assert rel.max() <= 1e-5, rel.max()
    assert np.all(np.diag(dist) == 0) and np.array_equal(dist, dist.T)
    np.testing.assert_array_equal(np.argsort(score, kind="stable"), np.argsort(s_ref, kind="stable"))
    np.testing.assert_array_equal(coef != 0, coef_ref != 0)
    assert coef[flipped] == 0
    np.testing.assert_allclose(coef, coef_ref, rtol=2.0**-23, atol=0)


def test_krum_distances_close_rows(dev):
    _check_distances([r.to(dev) for r in _close_rows(8, BIG, seed=1)])


def test_unaligned_rows(dev):
    """Rows ``buf[i]`` of a ``[K, 1001]`` buffer: the odd rows are 4-byte aligned only, so every
    vector access has to be given up."""
    from myfyp_amd import ops

    k, n = 8, 1001
    buf = torch.stack(_close_rows(k, n, seed=1)).to(dev)
    assert buf[1].data_ptr() % 16 != 0
    rows = [buf[i] for i in range(k)]
    _check_distances(rows)
    # the weighted mean of the chosen rows, written over unaligned rows
    x64 = buf.double().clone()
    w = [float(1 + i) for i in range(k)]
    _, _, coef = ops.krum_into(rows, [buf[1], buf[4]], w, 1, 3)
    want = (coef.double().view(-1, 1) * x64).sum(0)
    atol = 3 * 2.0**-24 * float(x64.abs().max())
    for i in (1, 4):
        assert float((buf[i].double() - want).abs().max()) <= atol
    # an aligned copy of the same rows gives the same distances, bit for bit
    x = torch.stack(_close_rows(k, n, seed=1)).to(dev)
    al = [x[i].clone() for i in range(k)]
    assert all(t.data_ptr() % 16 == 0 for t in al)
    d_al = ops.krum_into(al, [], [1.0] * k, 1, 3)[0]
    d_un = ops.krum_into([x[i] for i in range(k)], [], [1.0] * k, 1, 3)[0]
    assert torch.equal(d_al, d_un)
    # trimmed mean over unaligned rows, two of them the outputs
    y = _randn((k, n), 7).to(dev)
    for trim in (0, 1, 3):
        yy = y.clone()
        _check_trimmed([yy[i] for i in range(k)], trim)


@pytest.mark.parametrize("k,n", [(1, 1001), (2, 7), (16, 1001), (16, BIG), (5, 1)])
def test_krum_mean(dev, k, n):
    """The outputs alias the live rows; unequal sample weights are honoured."""
    from myfyp_amd import ops

    rows = [r.to(dev) for r in _close_rows(k, n, seed=20 + k, flipped=3)]
    x64 = torch.stack(rows).double()
    w = [float(1 + (3 * i) % 7) for i in range(k)]
    m = 3
    _, _, coef_ref = _krum_ref(x64.cpu(), w, 1, m)
    outs = rows if k <= 2 else [rows[0], rows[3], rows[k - 1]]  # chosen and rejected rows among them
    dist, score, coef = ops.krum_into(rows, outs, w, 1, m)
    np.testing.assert_array_equal(coef.cpu().numpy() != 0, coef_ref != 0)
    np.testing.assert_allclose(coef.cpu().numpy(), coef_ref, rtol=2.0**-23, atol=0)
    want = (coef.double().view(-1, 1) * x64).sum(0)
    atol = min(m, k) * 2.0**-24 * float(x64.abs().max())
    for o in outs:
        err = float((o.double() - want).abs().max())
        print(f"krum mean K={k} n={n}: max err {err:.3e} (bound {atol:.3e})")
        assert err <= atol, (err, atol)


def test_krum_deterministic(dev):
    from myfyp_amd import ops

    src = [r.to(dev) for r in _close_rows(8, BIG, seed=3)]
    got = []
    for _ in range(2):
        out = [torch.empty(BIG, device=dev), torch.empty(BIG, device=dev)]
        dist, score, coef = ops.krum_into(src, out, [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0], 1, 3)
        got.append((dist, score, coef, out[0], out[1]))
    for a, b in zip(*got):
        assert torch.equal(a, b)
