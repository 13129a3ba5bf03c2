"""The oracle of the fused MLP engine's shuffle, gather and bf16 step kernels (``tests/_mlp_ref.py``), checked
on its own, without a GPU:

* the keyed Feistel shuffle is a bijection at every size, mixes like a random permutation, and gives every
  peer its own order;
* with the bf16 rounding switched off, ``step`` is float64 autograd of ``myfyp_amd.models.MLP`` + cross-entropy;
* every ``exact`` case the GPU tests compare bit for bit satisfies the exactness condition they rely on, and
  its evaluation logits have one maximum per row (but in the case built to tie).
"""

import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _mlp_ref as M

F64 = torch.float64
KEYS = (0, 0x0123456789ABCDEF, 0xFFFFFFFFFFFFFFFF, 0x9E3779B97F4A7C15)


def _is_perm(a, n):
    return a.shape == (n,) and np.array_equal(np.sort(a), np.arange(n))


def test_feistel_is_a_bijection_at_every_small_size():
    """n = 1 .. 2050 (every block width up to 12 bits, both sides of each power of two), three keys."""
    for key in KEYS[:3]:
        for n in range(1, 2051):
            assert _is_perm(M.feistel_perm_np(n, key), n), (n, key)


@pytest.mark.parametrize("n", [4095, 4096, 4097, 60000, 65536, 65537, 2 ** 20 + 1])
def test_feistel_is_a_bijection_at_large_sizes(n):
    for key in KEYS[:3]:
        assert _is_perm(M.feistel_perm_np(n, key), n), (n, key)


def test_scalar_and_vectorised_forms_agree():
    """Every position for n <= 256, 64 positions (both ends and a stride) of every larger n up to 2050 and of
    the large sizes, two keys."""
    for key in KEYS[1:3]:
        for n in list(range(1, 2051)) + [4097, 60000, 65537, 2 ** 20 + 1]:
            v = M.feistel_perm_np(n, key)
            pos = range(n) if n <= 256 else sorted({0, 1, n - 2, n - 1, *range(0, n, max(1, n // 60))})
            for i in pos:
                assert M.feistel_perm(i, n, key) == v[i], (n, key, i)
    assert M.feistel_perm(0, 1, 5) == 0 and M.feistel_perm(0, 0, 5) == 0 and M.half_bits(2) == 1 and M.half_bits(5) == 2 and M.half_bits(17) == 3


def test_feistel_mixes_like_a_random_permutation():
    """n = 60000, four keys. At most 10 fixed points (Poisson(1): P(> 10) < 1e-7); Spearman |rho| between i and
    perm[i] below 5 / sqrt(n - 1), five standard deviations of a random permutation's rho."""
    n = 60000
    i = np.arange(n, dtype=np.float64)
    for key in KEYS:
        perm = M.feistel_perm_np(n, key)
        fixed = int((perm == np.arange(n)).sum())
        rho = float(np.corrcoef(i, perm.astype(np.float64))[0, 1])  # both are rank vectors already
        print(f"key {key:#x}: {fixed} fixed points, rho {rho:.2e} (limit {5 / math.sqrt(n - 1):.2e})")
        assert fixed <= 10
        assert abs(rho) < 5 / math.sqrt(n - 1)


def test_peers_and_epochs_get_their_own_order():
    seed = 0x5DEECE66D1234567
    for n in (97, 60000):
        orders = [tuple(M.epoch_perm(n, seed, p)) for p in range(16)]
        assert len(set(orders)) == 16
        assert tuple(M.epoch_perm(n, seed + 1, 0)) not in orders
    assert len({M.peer_key(seed, p) for p in range(16)}) == 16
    assert M.peer_key(0, 0) == 0x9E3779B97F4A7C15 and M.peer_key(0, 1) == (2 * 0x9E3779B97F4A7C15) % 2 ** 64


def test_gather_oracle():
    g = torch.Generator().manual_seed(1)
    n = [5, 3, 4]
    xs = [torch.randint(0, 256, (k, 8), generator=g).to(torch.uint8) for k in n]
    ys = [torch.arange(k) for k in n]
    Xb, Xb16, Yb = M.gather(xs, ys, n, 77, 4, active=[1, 1, 0], fill=-1.0)
    assert torch.equal(Xb, Xb16)
    for p in range(2):
        perm = [M.feistel_perm(i, n[p], M.peer_key(77, p)) for i in range(n[p])]
        rows = min(4, n[p])
        assert Yb[p, :rows].tolist() == perm[:rows] and (Yb[p, rows:] == -1).all()
        assert torch.equal(Xb[p, :rows], xs[p][perm[:rows]].double()) and (Xb[p, rows:] == -1).all()
    assert (Xb[2] == -1).all() and (Yb[2] == -1).all()
    pinned = M.gather(xs, ys, n, [np.array([4, 0, 1, 2, 3]), np.array([2, 1, 0]), np.arange(4)], 4, fill=-1.0)[2]
    assert pinned[0].tolist() == [4, 0, 1, 2] and pinned[1].tolist() == [2, 1, 0, -1] and pinned[2].tolist() == [0, 1, 2, 3]


@pytest.mark.parametrize("D,B", [((40, 64, 64, 10), 8), ((8, 128, 64, 1), 5), ((72, 128, 128, 16), 33)])
def test_step_without_rounding_is_autograd(D, B):
    """Full and partial batches, D3 of 1, 10 and 16: the loss, the logits and all six gradients (rtol 1e-12)."""
    from myfyp_amd.models import MLP

    c = M.case(D, B, "randn")
    for p in range(2):
        r = M.step(c, p, rnd=M.ident)
        assert r["rows"] == c["rows"][p] and (p == 0 or r["rows"] < B)
        m = MLP(input_size=D[0], hidden_sizes=[D[1], D[2]], out_channels=D[3]).double()
        lin = m.linear_layers()
        with torch.no_grad():
            for i, l in enumerate(lin):
                l.weight.copy_(c["W"][f"W{i + 1}"][p])
                l.bias.copy_(c["W"][f"b{i + 1}"][p])
        x = r["X"]
        for layer in m.layers:  # MLP.forward itself casts its input to float
            x = layer(x)
        loss = F.cross_entropy(x, r["y"])
        loss.backward()
        kw = dict(rtol=1e-12, atol=1e-300)
        torch.testing.assert_close(r["z"], x.detach(), **kw)
        torch.testing.assert_close(r["loss"].sum() / r["rows"], loss.detach(), **kw)
        assert torch.equal(r["pred"], x.detach().argmax(1)) or D[3] == 1
        for i, l in enumerate(lin):
            # a sum of cancelling terms: relative to the sum of the absolute terms' size, as autograd's own order differs
            for name, got, want in ((f"W{i + 1}", r["g"][f"W{i + 1}"], l.weight.grad), (f"b{i + 1}", r["g"][f"b{i + 1}"], l.bias.grad)):
                scale = float(want.abs().max())
                assert float((got - want).abs().max()) <= 1e-12 * max(scale, 1e-300), name
            assert D[3] == 1 or float(l.weight.grad.abs().max()) > 0


def test_head_rules():
    """The first maximum wins; dlogits is zero beyond D3 and sums to zero over the classes of a row."""
    z = torch.tensor([[1.0, 3.0, 3.0, -1.0], [2.0, 2.0, 2.0, 2.0], [0.0, -1.0, 5.0, 5.0]], dtype=F64)
    y = torch.tensor([1, 3, 2])
    loss, pred, sm = M.head(z, y)
    assert pred.tolist() == [1, 0, 2]
    d = M.dlogits(z, y, rnd=M.ident)
    assert d.shape == (3, 16) and not d[:, 4:].any() and float(d.sum(1).abs().max()) < 1e-15
    torch.testing.assert_close(loss, F.cross_entropy(z, y, reduction="none"), rtol=1e-14, atol=0)
    assert float((d[:, :4] * 3 - (sm - F.one_hot(y, 4))).abs().max()) < 1e-15
    lp, smb = M.eps_softmax(z)
    assert 0 < lp < smb < 2.0 ** -17


def test_lsb_and_exactness():
    x = torch.tensor([0.0, 1.0, 3.0, 6.0, 0.375, -2.0 ** -20, 257.0], dtype=F64)
    assert M.lsb(x).tolist() == [float("inf"), 1.0, 1.0, 2.0, 0.125, 2.0 ** -20, 1.0]
    A = torch.tensor([[2.0, 6.0], [0.0, 0.0]], dtype=F64)
    W = torch.tensor([[0.5, 0.25]], dtype=F64)
    assert M.exactness(A, W).tolist() == [[(1.0 + 1.5) / 0.5], [0.0]]
    assert M.exactness(A, W, unit=0.125).tolist() == [[20.0], [0.0]]


def _exact_cases():
    return [(D, B, s) for D, B, s in M.TRAIN_CASES]


@pytest.mark.parametrize("D,B,s", _exact_cases(), ids=[M.case_id(c) for c in _exact_cases()])
def test_exact_training_cases_are_exact(D, B, s):
    """``sum |term| / unit < 2^24`` for every fc1, fc2 and fc3 sum of every peer: any fp32 summation order gives the
    exact sum, so one rounding to bf16 decides each stored activation. Also: the family exercises that
    rounding (some fc1 sums need more than 8 bits) and both sides of each ReLU."""
    c = M.case(D, B, "exact", s)
    u = M.units(D)
    worst = [0.0, 0.0, 0.0]
    for p in range(M.P):
        r = M.step(c, p)
        W = {k: v[p] for k, v in c["W"].items()}
        assert torch.equal(M.bf16(W["W1"]), W["W1"]) and torch.equal(M.bf16(W["W2"]), W["W2"]) and torch.equal(M.bf16(W["W3"]), W["W3"])
        assert all(torch.equal(W[k].float().double(), W[k]) for k in W)
        if r["rows"] == 0:
            continue
        for i, (A, w, b, unit) in enumerate(((r["X"], W["W1"], W["b1"], u[0]), (r["H1"], W["W2"], W["b2"], u[0] * u[1]),
                                             (r["H2"], W["W3"], W["b3"], u[0] * u[1] * u[2]))):
            pre, _ = M.fc_pre(A, w, b)
            assert torch.equal(pre / unit, (pre / unit).round()), "a sum off its grid"
            worst[i] = max(worst[i], float(M.exactness(A, w, b, unit).max()))
        if p == 0 and D[0] > 8:
            pre = M.fc_pre(r["X"], W["W1"], W["b1"])[0].clamp_min(0)
            assert (M.bf16(pre) != pre).any(), "no fc1 sum needs rounding"
        if r["rows"] > 1:
            assert (r["H1"] > 0).any() and (r["H1"] == 0).any() and (r["H2"] > 0).any() and (r["H2"] == 0).any()
    print("sum |term| / unit / 2^24: fc1 %.2e, fc2 %.2e, fc3 %.2e" % tuple(w / M.LIM for w in worst))
    assert max(worst) < M.LIM


@pytest.mark.parametrize("D,family,n_test,active", M.EVAL_CASES, ids=[f"{c[0][0]}-{c[1]}" for c in M.EVAL_CASES])
def test_exact_evaluation_cases(D, family, n_test, active):
    """Exactness of the three sums on the test rows, and one maximum per row of logits, but in the case built to
    tie, where ties exist and the first index is the prediction."""
    c = M.case(D, 32, family, n_test=n_test, active=active)
    u = M.units(D)
    ties = 0
    for p in range(M.P):
        W = {k: v[p] for k, v in c["W"].items()}
        X = c["xt"][p].double()
        H1 = M.fc(X, W["W1"], W["b1"])
        H2 = M.fc(H1, W["W2"], W["b2"])
        for A, w, b, unit in ((X, W["W1"], W["b1"], u[0]), (H1, W["W2"], W["b2"], u[0] * u[1]), (H2, W["W3"], W["b3"], u[0] * u[1] * u[2])):
            assert float(M.exactness(A, w, b, unit).max()) < M.LIM
        for base in (0, 512):
            loss, correct, conf, z = M.eval_chunk(c, p, base)
            rows = z.shape[0]
            assert rows == (max(0, min(512, n_test[p] - base)) if active[p] else 0) and int(conf.sum()) == rows
            if rows == 0:
                continue
            tied = (z == z.amax(1, keepdim=True)).sum(1) > 1
            if family == "exact_tie":
                ties += int(tied.sum())
                pred = conf.sum(0).nonzero()[:, 0].tolist()
                assert 1 not in pred, "a tie went to the second index"
            else:
                assert D[3] == 1 or not tied.any()
    if family == "exact_tie":
        assert ties > 10
