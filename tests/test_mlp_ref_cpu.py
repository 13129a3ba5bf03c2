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


# ---------------------------------------------------------------------------------------------
# the fp32 epoch kernels' oracle (tests/test_mlp_f32_oracle_gpu.py)
# ---------------------------------------------------------------------------------------------
def _f32_grid_cases():
    out = []
    for D0, D3, B in M.F32_SHAPES:
        out += [(D0, D3, B, n) for n in M.F32_ONE_STEP[B] + M.F32_STEPS[B]]
    return out


@pytest.mark.parametrize("D0,D3,B,n", _f32_grid_cases(), ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_f32_grid_training_cases_are_exact(D0, D3, B, n):
    """Every training case of parts (a), (b) and (c): all rows of both peers, H1 and H2 NOT rounded (the fp32 kernel
    keeps them in fp32): ``sum |term| / unit < 2^24`` at fc1, fc2 and fc3, every value an fp32 number. With D3 = 16 the
    family is ``exact_tie``: classes 0 and 1 tie in every row."""
    c = M.case32(D0, D3, B, M.f32_family(D3), n)
    for p in range(2):
        W, X = c["W"][p], c["x"][p].double()
        assert all(torch.equal(v.float().double(), v) for v in W.values())
        r = M.grid_ratios(W, X, c["D"])
        H1, H2, z = M.forward32(W, X)
        assert all(torch.equal(t.float().double(), t) for t in (H1, H2, z))
        assert max(r) < M.LIM, r
        if D3 == 16:
            assert torch.equal(z[:, 0], z[:, 1])
        if X.shape[0] > 8:
            assert (H1 > 0).any() and (H1 == 0).any() and (H2 > 0).any() and (H2 == 0).any()
    print("sum |term| / unit / 2^24: fc1 %.2e, fc2 %.2e, fc3 %.2e" % tuple(x / M.LIM for x in r))


@pytest.mark.parametrize("D,family,n_test,seed", M.F32_EVAL, ids=[f"{c[0][0]}-{c[1]}" for c in M.F32_EVAL])
def test_f32_grid_evaluation_cases_are_exact(D, family, n_test, seed):
    """The test rows of part (e): exact at fc1, fc2 and fc3, and in the tie family more than 10 rows whose maximum is
    shared by classes 0 and 1."""
    c = M.case32(D[0], D[1], 64, family, (4, 4), n_test, seed)
    ties = 0
    for p in range(2):
        X = c["xt"][p].double()
        assert max(M.grid_ratios(c["W"][p], X, c["D"])) < M.LIM
        z = M.forward32(c["W"][p], X)[2]
        ties += int(((z == z.amax(1, keepdim=True)).sum(1) > 1).sum())
    assert family != "exact_tie" or ties > 10


def _torch_mlp(W, D):
    from myfyp_amd.models import MLP

    m = MLP(input_size=D[0], hidden_sizes=[D[1], D[2]], out_channels=D[3]).double()
    with torch.no_grad():
        for i, l in enumerate(m.linear_layers()):
            l.weight.copy_(W[f"W{i + 1}"])
            l.bias.copy_(W[f"b{i + 1}"])
    return m


@pytest.mark.parametrize("name", ["nesterov_wd", "adam"])
def test_epoch_without_rounding_is_autograd_with_torch_optim(name):
    """Two epochs of one fit (the moments and the step count carried over), 3 steps each, the last batch partial:
    float64 autograd + ``torch.optim`` with the fp32 values of the hyperparameters."""
    f = M.R.f32
    hp = M.F32_LEARN_HP["nesterov_wd"] if name == "nesterov_wd" else dict(kind=0, lr=1e-3, wd=1e-4)
    c = M.case32(40, 10, 24, "randn32", (60, 60))
    W, x, y = c["W"][0], c["x"][0], c["y"][0]
    perms = [M.epoch_perm32(60, ep, 0) for ep in range(2)]
    got, st = M.epoch(W, x, y, perms[0], 24, hp, rnd=M.ident)
    got, st = M.epoch(got, x, y, perms[1], 24, hp, rnd=M.ident, state=st)
    assert st[2] == 6
    m = _torch_mlp(W, c["D"])
    if name == "adam":
        opt = torch.optim.Adam(m.parameters(), lr=f(hp["lr"]), betas=(f(M.BETA1), f(M.BETA2)), eps=f(M.EPS), weight_decay=f(hp["wd"]))
    else:
        opt = torch.optim.SGD(m.parameters(), lr=f(hp["lr"]), momentum=f(hp["momentum"]), weight_decay=f(hp["wd"]), nesterov=True)
    for perm in perms:
        for s in range(0, 60, 24):
            idx = torch.as_tensor(perm[s: s + 24])
            h = x[idx].double()
            for layer in m.layers:
                h = layer(h)
            opt.zero_grad()
            F.cross_entropy(h, y[idx].long()).backward()
            opt.step()
    for i, l in enumerate(m.linear_layers()):
        for k, want in ((f"W{i + 1}", l.weight), (f"b{i + 1}", l.bias)):
            upd = float((want.detach() - W[k]).abs().max())
            assert upd > 0 and float((got[k] - want.detach()).abs().max()) <= 1e-9 * upd, k


def test_sgd_epoch_is_the_plain_sgd_epoch():
    c = M.case32(40, 10, 24, "randn32", (60, 60))
    perm = M.epoch_perm32(60, 0, 0)
    a = M.sgd_epoch(c["W"][0], c["x"][0], c["y"][0], perm, 24, 1e-2)
    b = M.epoch(c["W"][0], c["x"][0], c["y"][0], perm, 24, dict(kind=1, lr=1e-2, momentum=0.0, wd=0.0, nesterov=False))[0]
    assert all(torch.equal(a[k], b[k]) for k in M.NAMES) and not torch.equal(a["W1"], c["W"][0]["W1"])


def test_split3_and_the_cross_terms_layout_3_drops():
    """``split3`` is exact with ``|mid| <= 2^-8 |x|`` and ``|lo| <= 2^-16 |x|``; the three dropped cross terms reach beyond 2^-26
    of a product (so neither 2^-32 nor 2^-26 bounds them) and stay within ``L3_DROP``; on the grid they vanish; for random
    fp32 operands the six-term H2 is within :func:`h2_l3_bound` of the exact one."""
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(1 << 16, generator=g) * torch.exp2(torch.randint(-20, 20, (1 << 16,), generator=g).float())).double()
    hi, mid, lo = M.split3(x)
    assert torch.equal(hi + mid + lo, x)
    assert float((mid.abs() / x.abs()).max()) <= 2.0 ** -8 and float((lo.abs() / x.abs()).max()) <= 2.0 ** -16
    a, b = x[: 1 << 15], x[1 << 15:]
    (ah, am, al), (bh, bm, bl) = M.split3(a), M.split3(b)
    drop = ((am * bl + al * bm + al * bl).abs() / (a * b).abs()).max()
    print(f"largest dropped part of a product: 2^{math.log2(float(drop)):.2f}")
    assert 2.0 ** -26 < float(drop) <= M.L3_DROP
    c = M.case32(784, 10, 64, "exact", (64, 64))
    W = c["W"][0]
    H1 = M.forward32(W, c["x"][0].double())[0]
    assert torch.equal(M.h2_l3(H1, W["W2"], W["b2"]), H1 @ W["W2"].t() + W["b2"])
    H1r = torch.randn(64, 256, generator=g).float().double().clamp_min(0)
    W2r, b2r = torch.randn(128, 256, generator=g).float().double() / 16, torch.randn(128, generator=g).float().double()
    err = (M.h2_l3(H1r, W2r, b2r) - (H1r @ W2r.t() + b2r)).abs()
    assert float(err.max()) > 0 and (err <= M.h2_l3_bound(H1r, W2r, b2r)).all()


def _fma(a, b, c):
    return (a * b + c).float().double()


def _r(t):
    return t.float().double()


@pytest.mark.parametrize("D0,D3,B,rows", [(784, 10, 64, 64), (40, 16, 24, 23), (8, 1, 32, 1), (40, 10, 24, 1)])
def test_f32_emulated_step_stays_inside_the_bounds(D0, D3, B, rows):
    """One step on the grid with every sum accumulated in fp32 over a permuted reduction axis and the softmax in fp32:
    the forward is the float64 one bit for bit, the six gradients are within :func:`bounds32`; with one row the weight
    gradients are :func:`outer32` of the bias gradients."""
    c = M.case32(D0, D3, B, M.f32_family(D3), (rows, rows))
    for p in range(2):
        W, X, y = c["W"][p], c["x"][p].double(), c["y"][p].long()
        s = M.step32(W, X, y)
        mm = M.mm32_permuted(torch.Generator().manual_seed(p))
        H1 = (mm(X, W["W1"].t()) + W["b1"]).float().double().clamp_min(0)
        H2 = (mm(H1, W["W2"].t()) + W["b2"]).float().double().clamp_min(0)
        z = (mm(H2, W["W3"].t()) + W["b3"]).float().double()
        assert torch.equal(H1, s["H1"]) and torch.equal(H2, s["H2"]) and torch.equal(z, s["z"])
        sm = torch.softmax(z.float(), 1)
        sm[torch.arange(rows), y] -= 1.0
        dl = (sm / rows).double()
        assert float((dl * rows - s["dlog"] * rows).abs().max()) <= s["eps_dl"]
        zero = torch.zeros((), dtype=F64)
        dH2 = torch.where(H2 > 0, mm(dl, W["W3"]), zero)
        dH1 = torch.where(H1 > 0, mm(dH2, W["W2"]), zero)
        one = torch.ones(rows, 1, dtype=F64)
        g = {"W1": mm(dH1.t(), X), "b1": mm(dH1.t(), one)[:, 0], "W2": mm(dH2.t(), H1), "b2": mm(dH2.t(), one)[:, 0], "W3": mm(dl.t(), H2), "b3": mm(dl.t(), one)[:, 0]}
        bnd = M.bounds32(s, W)
        for k in M.NAMES:
            err = (g[k] - s["g"][k]).abs()
            assert (err <= bnd[k]).all(), (k, float((err / bnd[k].clamp_min(1e-300)).max()))
            # (one batch row missing from a sum moves it by about 1 / rows >= 2^-6 of its size)
            assert D3 == 1 or float(bnd[k].max()) < 2.0 ** -10 * float(s["g"][k].abs().max()), f"{k}: a bound that says nothing"
        if rows == 1:
            for k, b, a in (("W3", "b3", H2), ("W2", "b2", H1), ("W1", "b1", X)):
                assert torch.equal(g[k], M.outer32(g[b], a[0]))


@pytest.mark.parametrize("variant", list(M.OPT_VARIANTS))
def test_upd32_emulation_stays_inside_its_bounds(variant):
    """``upd32``'s operation sequence emulated in fp32 (each fma rounded once, sqrt and the reciprocal correctly rounded)
    against :func:`upd32` in float64, for every optimizer variant, from non-zero moments at step 4."""
    hp = dict(M.OPT_VARIANTS[variant], t0=3)
    g = torch.Generator().manual_seed(11)
    n = 4096
    w, gr = _r(torch.randn(n, generator=g) * 0.1), _r(torch.randn(n, generator=g) * torch.exp2(torch.randint(-30, 0, (n,), generator=g).float()))
    m, v = _r(torch.randn(n, generator=g) * 1e-3), _r(torch.rand(n, generator=g) * 1e-6)
    anchor = _r(w + 0.01 * torch.randn(n, generator=g)) if "mu" in hp else None
    cg, cl = (_r(torch.randn(n, generator=g) * 1e-3), _r(torch.randn(n, generator=g) * 1e-3)) if hp.get("scaffold") else (None, None)
    k = 4
    w1, m1, v1, bw, bm, bv = M.upd32(hp, w, gr, m, v, k, anchor, cg, cl)
    h = M._hp32(hp)
    wdmu = M.R.f32(h.get("wd", 0.0) + (h.get("mu", 0.0) if anchor is not None else 0.0))
    ge = _fma(torch.full_like(w, wdmu), w, gr)
    if anchor is not None:
        ge = _r(ge + _r(-h["mu"] * anchor))
    if hp["kind"] == 0:
        b1, b2 = M.R.f32(M.BETA1), M.R.f32(M.BETA2)
        lr_t, inv = M.adam_coeffs(hp, k)
        me = _fma(torch.full_like(w, b1), m, _r((1.0 - b1) * ge))
        ve = _fma(torch.full_like(w, b2), v, _r((1.0 - b2) * _r(ge * ge)))
        den = _fma(_r(torch.sqrt(ve)), torch.full_like(w, inv), torch.full_like(w, M.R.f32(M.EPS)))
        we = _fma(torch.full_like(w, -lr_t), _r(me * _r(1.0 / den)), w)
    else:
        me, ve, gu = m, v, ge
        if h["momentum"] != 0.0:
            me = _fma(torch.full_like(w, h["momentum"]), m, ge)
            gu = _fma(torch.full_like(w, h["momentum"]), me, ge) if h["nesterov"] else me
        we = _fma(torch.full_like(w, -h["lr"]), gu, w)
    if cg is not None:
        we = _fma(torch.full_like(w, -h["lr"]), _r(cg - cl), we)
    for name, got, want, b in (("w", we, w1, bw), ("m", me, m1, bm), ("v", ve, v1, bv)):
        err = (got - want).abs()
        assert (err <= b).all(), (name, float((err / b.clamp_min(1e-300)).max()))
    assert not torch.equal(we, w) and float((bw / w1.abs().clamp_min(1e-30)).median()) < 2.0 ** -20


@pytest.mark.parametrize("hp", list(M.F32_LEARN_HP))
@pytest.mark.parametrize("shape", [M.F32_MAIN, M.F32_RAGGED], ids=["main", "ragged"])
def test_f32_learning_cases_are_not_chaotic(shape, hp):
    """Part (d)'s cases: the twin's floor (fp32 sums in another order, fp32 optimizer and master row, against the
    float64 epoch) is below 1e-4 for every tensor of both peers, so 8 times it still sees a single stale step."""
    D0, D3, B = shape
    c = M.case32(D0, D3, B, "randn32", M.F32_LEARN[B])
    for p in range(2):
        ref, alt = M.learn_refs(c, p, M.F32_LEARN_HP[hp])
        floors = {k: M.rel_update(alt[k], ref[k], c["W"][p][k]) for k in M.NAMES}
        print(f"peer {p}: " + ", ".join(f"{k} {v:.2e}" for k, v in floors.items()))
        assert 0 < max(floors.values()) < 1e-4, floors


# ---------------------------------------------------------------------------------------------
# the bf16 epoch kernel's oracle (tests/test_mlp_bf16_epoch_oracle_gpu.py)
# ---------------------------------------------------------------------------------------------
def _steps16(c, p):
    perm = M.epoch_perm32(c["n"][p], 0, p)
    for s in range(0, c["n"][p], c["B"]):
        idx = torch.as_tensor(perm[s: s + c["B"]], dtype=torch.int64)
        yield M.step16(c["W"][p], c["x"][p][idx].double(), c["y"][p][idx].long())


@pytest.mark.parametrize("D0,D3,B,n,seed", M.bf16_grid_cases(), ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_bf16_grid_cases_meet_the_oracles_conditions(D0, D3, B, n, seed):
    """Every grid case of the bf16 file, both peers, every step of the first epoch order: the forward with H1 and H2
    rounded to bf16 is exact (``sum |term| / unit < 2^24`` at fc1, fc2, fc3), no element of the two dgrad sums misses the
    exactness condition whichever end of its interval each upstream element takes, and the interval oracle stays
    sharp: every tensor's radius is at most 2^-5 of its gradient in the 2-norm, at most 5 % of dlog and at most
    25 % of dH1 straddle. (A case over a cap gets another seed in ``BF16_SEED``; the caps stay.)"""
    c = M.case32(D0, D3, B, M.f32_family(D3), n, seed=seed)
    worst = dict(dlog=0.0, dH2=0.0, dH1=0.0, radius=0.0)
    for p in range(2):
        W = c["W"][p]
        assert all(torch.equal(M.bf16(W[k]), W[k]) for k in ("W1", "W2", "W3")) and all(torch.equal(v.float().double(), v) for v in W.values())
        assert max(M.grid_ratios16(W, c["x"][p].double(), c["D"])) < M.LIM
        for s in _steps16(c, p):
            assert s["inexact"] == 0
            assert torch.equal(s["z"].float().double(), s["z"])
            for k in ("dlog", "dH2", "dH1"):
                assert ((s[k + "_lo"] <= s[k]) & (s[k] <= s[k + "_hi"])).all()
            if D3 == 16:
                assert torch.equal(s["z"][:, 0], s["z"][:, 1])
            for k, v in M.straddle(s).items():
                worst[k] = max(worst[k], v)
            if D3 == 1:
                assert all(not s[k].any() for k in ("dlog_lo", "dlog_hi", "dH1_lo", "dH1_hi")) and not s["loss"].any()
                continue
            b = M.bounds16(s, M.bpad(B))
            for k in M.NAMES:
                assert float(s["g"][k].norm()) > 0
                worst["radius"] = max(worst["radius"], float(b[k].norm() / s["g"][k].norm()))
    print(", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert worst["radius"] <= 2.0 ** -5 and worst["dlog"] <= 0.05 and worst["dH1"] <= 0.25


@pytest.mark.parametrize("D0,D3,B,rows", [(784, 10, 64, 64), (40, 16, 24, 23), (776, 16, 40, 40), (264, 10, 48, 33), (784, 10, 32, 1)])
def test_bf16_emulated_step_stays_inside_the_intervals(D0, D3, B, rows):
    """The kernel's step emulated with every sum in fp32 over a permuted reduction axis, the softmax in fp32 and a
    perturbation of ``0.9 eps_sm / rows`` of either sign on every dlogits element before its rounding: H1, H2 and the
    logits are the oracle's bit for bit, dlog, dH2 and dH1 lie in their intervals, the six gradients within
    :func:`bounds16` of the central ones; and the radius is sharp enough to see one batch row missing."""
    c = M.case32(D0, D3, B, M.f32_family(D3), (rows, rows))
    for p in range(2):
        W, X, y = c["W"][p], c["x"][p].double(), c["y"][p].long()
        s = M.step16(W, X, y)
        mm = M.mm32_permuted(torch.Generator().manual_seed(p))
        H1 = M.bf16((mm(X, W["W1"].t()) + W["b1"]).float().double().clamp_min(0))
        H2 = M.bf16((mm(H1, W["W2"].t()) + W["b2"]).float().double().clamp_min(0))
        z = (mm(H2, W["W3"].t()) + W["b3"]).float().double()
        assert torch.equal(H1, s["H1"]) and torch.equal(H2, s["H2"]) and torch.equal(z, s["z"])
        sm = torch.softmax(z.float(), 1).double()
        sm[torch.arange(rows), y] -= 1.0
        sign = torch.randint(0, 2, sm.shape, generator=torch.Generator().manual_seed(5 + p)).double() * 2 - 1
        dl = M.bf16(((sm + 0.9 * s["eps_sm"] * sign) / rows).float().double())
        zero = torch.zeros((), dtype=F64)
        dH2 = M.bf16(torch.where(H2 > 0, mm(dl, W["W3"]), zero))
        dH1 = M.bf16(torch.where(H1 > 0, mm(dH2, W["W2"]), zero))
        for k, t in (("dlog", dl), ("dH2", dH2), ("dH1", dH1)):
            assert ((s[k + "_lo"] <= t) & (t <= s[k + "_hi"])).all(), k
        assert rows == 1 or (dl != s["dlog"]).any(), "the perturbation moved nothing"
        one = torch.ones(rows, 1, dtype=F64)
        g = {"W1": mm(dH1.t(), X), "b1": mm(dH1.t(), one)[:, 0], "W2": mm(dH2.t(), H1), "b2": mm(dH2.t(), one)[:, 0], "W3": mm(dl.t(), H2), "b3": mm(dl.t(), one)[:, 0]}
        bnd = M.bounds16(s, M.bpad(B))
        for k in M.NAMES:
            err = (g[k] - s["g"][k]).abs()
            assert (err <= bnd[k]).all(), (k, float((err / bnd[k].clamp_min(1e-300)).max()))
            assert float(bnd[k].norm()) < 2.0 ** -5 * float(s["g"][k].norm()) / max(1.0, rows / 32), f"{k}: a radius that says nothing"


def test_bf16_bias_correction_bounds():
    """``adam_coeffs16`` against ``persist::bias_corr`` emulated in fp32 (``pow`` correctly rounded, then each fp32 operation):
    inside the bounds at k = 1 .. 40 and at 1000; the bounds tell every k from k + 1 by a factor of 100 at least."""
    hp = dict(kind=0, lr=1e-3)
    f = np.float32
    b1, b2 = f(M.BETA1), f(M.BETA2)
    for k in list(range(1, 41)) + [1000]:
        lr_t, inv, r_lr, r_inv = M.adam_coeffs16(hp, k)
        e_lr = f(hp["lr"]) / (f(1) - f(float(b1) ** k))
        e_inv = f(1) / np.sqrt(f(1) - f(float(b2) ** k), dtype=f)
        assert abs(float(e_lr) - lr_t) <= r_lr * lr_t and abs(float(e_inv) - inv) <= r_inv * inv, k
        nxt = M.adam_coeffs16(hp, k + 1)
        if k <= 40:
            assert abs(nxt[0] - lr_t) > 100 * r_lr * lr_t and abs(nxt[1] - inv) > 100 * r_inv * inv, k
    assert 1.1e-4 < 2 * M.adam_coeffs16(hp, 1)[3] < 1.3e-4


def test_bf16_moments_emulation_stays_inside_its_bounds():
    """Five steps of the kernel's ``upd<true>`` moment recursions emulated in fp32 on gradients moved by up to their radius,
    some radii as large as the element: within :func:`moments16`; one step with weight decay within :func:`adam_moments16`."""
    g = torch.Generator().manual_seed(13)
    n = 4096
    w = _r(torch.randn(n, generator=g) * 0.1)
    gs = [_r(torch.randn(n, generator=g) * torch.exp2(torch.randint(-20, 0, (n,), generator=g).float())) for _ in range(5)]
    rs = [x.abs() * torch.exp2(torch.randint(-12, 1, (n,), generator=g).float()).double() * (torch.rand(n, generator=g) < 0.3) for x in gs]
    b1, b2 = M.R.f32(M.BETA1), M.R.f32(M.BETA2)
    for wd in (0.0, 1e-4):
        hp = dict(kind=0, lr=0.0 if wd == 0.0 else 1e-3, wd=wd)
        me, ve = torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64)
        steps = 5 if wd == 0.0 else 1
        for x, r in zip(gs[:steps], rs[:steps]):
            gk = _r(x + r * (torch.rand(n, generator=g).double() * 2 - 1))
            gk = torch.where((gk - x).abs() <= r, gk, x)
            gk = _fma(torch.full_like(w, M.R.f32(wd)), w, gk)
            me = _fma(torch.full_like(w, b1), me, _r(M.C1 * gk))
            ve = _fma(torch.full_like(w, b2), ve, _r(M.C2 * _r(gk * gk)))
        if wd == 0.0:
            m, v, bm, bv = M.moments16(hp, w, gs, rs)
        else:
            zero = torch.zeros_like(w)
            m, v, bm, bv = M.adam_moments16(hp, w, gs[0], rs[0], zero, zero, zero, zero)
        assert ((me - m).abs() <= bm).all() and ((ve - v).abs() <= bv).all()
        if wd:  # where the radius is zero the bound is a few ulps: it sees the weight-decay term
            assert float((bm / m.abs().clamp_min(1e-300))[rs[0] == 0].median()) < 2.0 ** -20


@pytest.mark.parametrize("hp", list(M.BF16_LEARN_HP))
@pytest.mark.parametrize("shape", M.BF16_LEARN_SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_bf16_learning_cases_are_not_chaotic(shape, hp):
    """Part (d)'s cases of the bf16 file: 8 times the twin's floor is at most 1e-2 for every tensor of both peers (a
    stale weight or a step applied twice moves a tensor by the order of 1 / steps)."""
    D0, D3, B = shape
    c = M.case32(D0, D3, B, "randn16", M.BF16_LEARN[B], seed=M.BF16_LEARN_SEED.get(shape, 0))
    for p in range(2):
        ref, alt = M.learn_refs16(c, p, M.BF16_LEARN_HP[hp])
        floors = {k: M.rel_update(alt[k], ref[k], c["W"][p][k]) for k in M.NAMES}
        print(f"peer {p}: " + ", ".join(f"{k} {v:.2e}" for k, v in floors.items()))
        assert 0 < 8 * max(floors.values()) <= 1e-2, floors
