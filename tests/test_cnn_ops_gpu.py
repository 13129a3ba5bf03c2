"""Every stand-alone kernel of ``csrc/kernels/cnn_ops.hip`` against the float64 oracle of
``tests/_cnn_ops_ref.py``, driven directly through the ``cnn_*`` C entry points on tensors of a few
kilobytes.

Common set-up: 3 peers with ``nb = [B, partial, 0]``, a per-peer stride larger than the used extent,
NaN in every input row at or beyond ``nb * hw`` (a kernel that reads one poisons its result) and a
sentinel in every output (NaN, or a marker for integers and accumulators) that must survive where
the kernel has nothing to write.

Tolerances (``_cnn_ops_ref.bf16_bound`` / ``fp32_bound``): exact cases use eighths with |x| <= 4 and
dyadic coefficients, so every fp32 intermediate is exact in any order and the output must equal the
rounded oracle; rounded bf16 outputs get one bf16 ulp + 2^-20 * M; fp32 reductions and finalizes get
four times the error of the plain torch fp32 evaluation of the same formula (floor 2^-22 * max|ref|).
Each tolerance-based assertion is paired with the same comparison against a deliberately wrong
reference, which must fail. The "MI355X:" comments give worst observed error / bound.
"""

import pytest
import torch

import _cnn_ops_ref as R

pytestmark = pytest.mark.gpu

F64, BF = torch.float64, torch.bfloat16
P = 3
GAP = 64  # elements between one peer's used extent and the next peer's slab (keeps 16-byte alignment)
CCP = [(6, 8), (20, 24), (40, 40), (64, 64)]  # Cp/8 = 1, 3, 5, 8: the middle two do not divide 256
HWS = [1, 4, 25]


@pytest.fixture(scope="module")
def lib():
    from myfyp_amd.parallel.cnn_engine import _lib

    return _lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _eighths(g, *shape, lim=4):
    return torch.randint(-8 * lim, 8 * lim + 1, shape, generator=g).double() / 8


def _normal(g, *shape):
    return torch.randn(*shape, generator=g).to(BF).double()  # what the kernel will read


def _data(g, exact, *shape):
    return _eighths(g, *shape) if exact else _normal(g, *shape)


def _pow2(g, *shape):
    return torch.tensor([0.5, 1.0, 2.0], dtype=F64)[torch.randint(0, 3, shape, generator=g)]


def _poison(t, nb, per):
    """NaN in the rows no kernel may read: [P, rows, ...] rows >= nb * per."""
    t = t.clone()
    for p, n in enumerate(nb):
        t[p, n * per:] = R.NAN
    return t


def _dev(t, dtype=BF, fill=R.NAN, gap=GAP):
    """dense [P, ...] -> device [P, stride] buffer, ``fill`` in the gap between peers."""
    flat = t.reshape(t.shape[0], -1)
    buf = torch.full((t.shape[0], flat.shape[1] + gap), fill, dtype=dtype, device="cuda")
    buf[:, : flat.shape[1]] = flat.to(dtype).cuda()
    return buf


def _out(shape, dtype=BF, fill=R.NAN, gap=GAP):
    n = 1
    for s in shape[1:]:
        n *= s
    return torch.full((shape[0], n + gap), fill, dtype=dtype, device="cuda")


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device="cuda")


def _f32(t):
    return t.to(torch.float32).contiguous().cuda()


def _same_fill(t, fill):
    return torch.isnan(t) if fill != fill else t == fill


def _read(buf, ref, fill=R.NAN):
    """Device buffer -> dense float64 like ``ref``; asserts that the gap and every element the
    reference marks NaN still hold the sentinel, and that everything else was written."""
    torch.cuda.synchronize()
    n = ref[0].numel()
    host = buf.cpu()
    assert _same_fill(host[:, n:], fill).all(), "the gap between peers was written"
    got = host[:, :n].reshape(ref.shape).double()
    hole = torch.isnan(ref)
    assert _same_fill(got[hole], fill).all(), "an element beyond the valid extent was written"
    if fill != fill:
        assert not torch.isnan(got[~hole]).any(), "a valid element was not written (or a poisoned row was read)"
    return got, ~hole


def _exact(name, buf, ref64, ref32=None, fill=R.NAN):
    """Bit-for-bit (up to the sign of zero) against the oracle rounded to the buffer's type."""
    got, ok = _read(buf, ref64, fill)
    if ref32 is not None:  # the case really is exact: the fp32 evaluation loses nothing
        assert torch.equal(ref32.double()[ok], ref64[ok]), f"{name}: the exact case is not exact in fp32"
    want = ref64.to(buf.dtype).double()
    bad = (got != want) & ok
    assert not bad.any(), f"{name}: {int(bad.sum())} elements differ, first at {bad.nonzero()[0].tolist()}"


def _bf16_close(name, buf, ref64, big, wrong64):
    got, ok = _read(buf, ref64)
    bound = R.bf16_bound(torch.nan_to_num(ref64), torch.nan_to_num(big))
    err = (got - ref64).abs()
    ratio = float((err / bound)[ok].max()) if ok.any() else 0.0
    print(f"{name}: worst |err| / bound = {ratio:.3f}")
    assert ratio <= 1.0, f"{name}: {ratio:.3f} x the bf16 bound"
    w_ok = ok & ~torch.isnan(wrong64)
    assert ((got - wrong64).abs() > bound)[w_ok].any(), f"{name}: the wrong reference passes too"


def _fp32_close(name, got, ref64, ref32, wrong64):
    bound = R.fp32_bound(ref64, ref32)
    err = float((got.double() - ref64).abs().max())
    print(f"{name}: |err| {err:.3e}, bound {bound:.3e}, ratio {err / bound:.3f}")
    assert err <= bound, f"{name}: {err:.3e} > {bound:.3e}"
    assert float((got.double() - wrong64).abs().max()) > bound, f"{name}: the wrong reference passes too"


def _fp32_equal(name, got, ref64, ref32):
    assert torch.equal(ref32.double(), ref64), f"{name}: the exact case is not exact in fp32"
    bad = got.double() != ref64
    assert not bad.any(), f"{name}: {int(bad.sum())} elements differ, first at {bad.nonzero()[0].tolist()}"


# ---------------------------------------------------------------------------------------------
# input gather
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_perm", [False, True])
@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("offset,stop_peer", [(0, None), (4, None), (0, 1)])
def test_input_prep(lib, C, use_perm, offset, stop_peer):
    g = _gen(10 + C)
    B, H, W, Cp, scale, MARK = 4, 3, 2, 8, 1.0 / 255.0, -7
    n_samples = [9, 5, 3]  # offset 4: a full batch, a partial batch of one, no batch at all
    xs = [torch.randint(0, 256, (n, H, W, C), generator=g, dtype=torch.uint8) for n in n_samples]
    ys = [torch.randint(0, 10, (n,), generator=g) for n in n_samples]
    perm_ps = 12
    perm = torch.zeros(P, perm_ps, dtype=torch.int32)
    for p, n in enumerate(n_samples):
        perm[p, :n] = torch.randperm(n, generator=g).int()
    stopped = [p == stop_peer for p in range(P)] if stop_peer is not None else None
    ref, ref_labels, ref_nb = R.input_prep(xs, ys, perm if use_perm else None, offset, B, C, Cp, scale, stopped)

    xd, yd = [x.cuda() for x in xs], [y.cuda() for y in ys]
    xp = torch.tensor([x.data_ptr() for x in xd], dtype=torch.int64, device="cuda")
    yp = torch.tensor([y.data_ptr() for y in yd], dtype=torch.int64, device="cuda")
    permd = perm.cuda() if use_perm else None
    out = _out(ref.shape)
    labels, nb = _i32([MARK] * (P * B)), _i32([MARK] * P)
    stop = _i32([5 if s else 0 for s in stopped]) if stopped else None  # fit id 5 everywhere: peer stop_peer is told to stop
    fit = _i32([5] * P) if stopped else None
    nsd = _i32(n_samples)
    rc = lib.cnn_input_prep(xp.data_ptr(), yp.data_ptr(), nsd.data_ptr(), permd.data_ptr() if use_perm else None, perm_ps, offset, B,
                            H, W, C, Cp, scale, out.data_ptr(), out.shape[1], labels.data_ptr(), nb.data_ptr(), P, _stream(),
                            stop.data_ptr() if stopped else None, fit.data_ptr() if stopped else None)
    assert rc == 0
    _exact("input_prep", out, ref)  # includes: zero rows beyond the valid count, zero padding channels
    assert nb.cpu().tolist() == ref_nb
    got_labels = labels.cpu().reshape(P, B).long()
    written = ref_labels >= 0
    assert torch.equal(got_labels[written], ref_labels[written])
    assert (got_labels[~written] == MARK).all(), "labels beyond the valid count are left alone"
    if offset == 4:
        assert ref_nb == [4, 1, 0]
    if stop_peer is not None:
        assert ref_nb[stop_peer] == 0 and nb.cpu().tolist()[stop_peer] == 0


# ---------------------------------------------------------------------------------------------
# BatchNorm forward
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("C,Cp", [(6, 8), (70, 72)])
@pytest.mark.parametrize("case", ["train", "train_single", "train_exact", "eval"])
def test_bn_finalize(lib, case, C, Cp, rows):
    g = _gen(20 + C + rows)
    train = int(case != "eval")
    exact = case == "train_exact"
    nb, hw = {"train": ([5, 2, 0], 4), "train_single": ([5, 1, 0], 1), "train_exact": ([2, 1, 0], 1), "eval": ([5, 2, 0], 4)}[case]
    eps, mom = (0.25, 0.25) if exact else (1e-5, 0.1)
    # partial (sum, sum of squares) rows of real data, as fp32; the empty peer's rows hold leftovers
    stats = torch.zeros(P, rows, 2, Cp, dtype=F64)
    for p in range(P):
        n = max(1, nb[p] * hw)
        x = _eighths(g, n, Cp) if exact else _normal(g, n, Cp) * 2 + 0.5
        for r in range(rows):
            part = x[r::rows]
            stats[p, r, 0], stats[p, r, 1] = part.sum(0), (part * part).sum(0)
    stats = stats.float().double()
    gamma = _pow2(g, P, C) if exact else torch.rand(P, C, generator=g).double() + 0.5
    beta = _eighths(g, P, C) if exact else torch.randn(P, C, generator=g).double()
    rmean = _eighths(g, P, C) if exact else torch.randn(P, C, generator=g).double()
    rvar = _eighths(g, P, C).abs() + 0.5 if exact else torch.rand(P, C, generator=g).double() + 0.5
    args = (nb, hw, gamma, beta, rmean, rvar, C, Cp, eps, mom, train)
    ref = R.bn_finalize(stats, *args)
    ref32 = R.bn_finalize(stats, *args, dtype=torch.float32)
    if train:  # wrong divisor
        wrong = R.bn_finalize(stats, *args, count=lambda n: max(1, n) + 1)
    else:  # wrong running variance
        wrong = R.bn_finalize(stats, nb, hw, gamma, beta, rmean, rvar * 1.01, C, Cp, eps, mom, 0)

    st = _dev(stats, torch.float32, fill=3.0, gap=8)
    run_ps, param_ps = C + 2, C + 3
    gm, bt = _dev(gamma, torch.float32, gap=3), _dev(beta, torch.float32, gap=3)
    rm, rv = _dev(rmean, torch.float32, fill=3.0, gap=2), _dev(rvar, torch.float32, fill=3.0, gap=2)
    ss = torch.full((P, 2, Cp), R.NAN, dtype=torch.float32, device="cuda")
    ms = torch.full((P, 2, Cp), R.NAN, dtype=torch.float32, device="cuda")
    nbd = _i32(nb)
    rc = lib.cnn_bn_finalize(st.data_ptr(), st.shape[1], rows, nbd.data_ptr(), hw, gm.data_ptr(), bt.data_ptr(), param_ps, rm.data_ptr(), rv.data_ptr(),
                             run_ps, C, Cp, eps, mom, train, ss.data_ptr(), ms.data_ptr(), P, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    got_ss, got_ms = ss.cpu(), ms.cpu()
    got_rm, got_rv, got_st = rm.cpu(), rv.cpu(), st.cpu()
    # padding channels are zero, the gaps keep their marker
    assert not got_ss[:, :, C:].any() and not got_ms[:, :, C:].any()
    assert (got_rm[:, C:] == 3.0).all() and (got_rv[:, C:] == 3.0).all() and (got_st[:, rows * 2 * Cp:] == 3.0).all()
    new_stats = got_st[:, : rows * 2 * Cp].reshape(P, rows, 2, Cp)
    if train:
        assert not new_stats.any(), "the accumulator rows are re-armed, the empty peer's too"
    else:
        assert torch.equal(new_stats.double(), stats), "evaluation leaves the accumulator rows alone"
        assert torch.equal(got_rm[:, :C], rmean.float()) and torch.equal(got_rv[:, :C], rvar.float())
    # a peer without samples keeps its running statistics bit for bit
    assert torch.equal(got_rm[2, :C], rmean[2].float()) and torch.equal(got_rv[2, :C], rvar[2].float())
    if exact:
        # cnt = 2 and 1: mean, biased and unbiased variance and the running updates are exact; with
        # cnt = 1 the unbiased variance is the biased one (0), not 0/0
        _fp32_equal("bn_finalize mean", got_ms[:, 0], ref[1][:, 0], ref32[1][:, 0])
        _fp32_equal("bn_finalize rmean", got_rm[:, :C], ref[2], ref32[2])
        _fp32_equal("bn_finalize rvar", got_rv[:, :C], ref[3], ref32[3])
        assert torch.equal(ref[3][1], 0.75 * rvar[1])
    # MI355X, worst |err| / bound over all cases: ss 0.42, ms 0.18, rmean 0.25, rvar 0.25
    _fp32_close(f"bn_finalize[{case}] ss", got_ss, ref[0], ref32[0], wrong[0])
    _fp32_close(f"bn_finalize[{case}] ms", got_ms, ref[1], ref32[1], wrong[1])
    if train:
        _fp32_close(f"bn_finalize[{case}] rmean", got_rm[:, :C], ref[2], ref32[2], wrong[2])
        _fp32_close(f"bn_finalize[{case}] rvar", got_rv[:, :C], ref[3], ref32[3], wrong[3])


def _ss(g, exact, C, Cp):
    """a BN's (scale, shift) rows [P, 2, Cp], zero in the padding channels"""
    ss = torch.zeros(P, 2, Cp, dtype=F64)
    ss[:, 0, :C] = _pow2(g, P, C) * torch.tensor([1.0, -1.0], dtype=F64)[torch.randint(0, 2, (P, C), generator=g)] if exact \
        else torch.randn(P, C, generator=g).float().double()
    ss[:, 1, :C] = _eighths(g, P, C) if exact else torch.randn(P, C, generator=g).float().double()
    return ss


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "random"])
@pytest.mark.parametrize("hw", HWS)
@pytest.mark.parametrize("C,Cp", CCP)
def test_bn_act(lib, C, Cp, hw, exact):
    g = _gen(30 + Cp + hw)
    B, nb = 5, [5, 2, 0]
    rows = B * hw
    y, res, y2 = (_poison(_data(g, exact, P, rows, Cp), nb, hw) for _ in range(3))
    ss, ss2 = _ss(g, exact, C, Cp), _ss(g, exact, C, Cp)
    yd, rd, y2d = _dev(y), _dev(res), _dev(y2)
    ssd, ss2d, nbd = _f32(ss), _f32(ss2), _i32(nb)
    for name, r_, y2_, relu in [("plain", None, None, 0), ("relu", None, None, 1), ("res", res, None, 1), ("bn2", None, y2, 1), ("res+bn2", res, y2, 0)]:
        ref, big = R.bn_act(y, ss, r_, y2_, ss2 if y2_ is not None else None, relu, nb, hw)
        out = _out(ref.shape)
        # max_rows = 1 sizes the grid only: one block walks all nb * hw rows
        rc = lib.cnn_bn_act(yd.data_ptr(), yd.shape[1], ssd.data_ptr(), rd.data_ptr() if r_ is not None else None, rd.shape[1],
                            y2d.data_ptr() if y2_ is not None else None, y2d.shape[1], ss2d.data_ptr() if y2_ is not None else None, relu,
                            nbd.data_ptr(), 1, hw, Cp, out.data_ptr(), out.shape[1], P, _stream())
        assert rc == 0
        if exact:
            ref32, _ = R.bn_act(y, ss, r_, y2_, ss2 if y2_ is not None else None, relu, nb, hw, dtype=torch.float32)
            _exact(f"bn_act[{name}]", out, ref, ref32)
        else:
            wrong, _ = R.bn_act(y, ss * 1.01, r_, y2_, ss2 if y2_ is not None else None, relu, nb, hw)  # scale and shift 1 % off
            _bf16_close(f"bn_act[{name}]", out, ref, big, wrong)  # MI355X: worst |err| / bound 0.50
        if r_ is None and y2_ is None:
            got, _ = _read(out, ref)
            assert not got[:2, :, C:].nan_to_num().any(), "padding channels: zero scale and shift give zero"


# ---------------------------------------------------------------------------------------------
# BatchNorm backward: reduce -> finalize -> apply
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gout_on", [True, False], ids=["gout", "nogout"])
@pytest.mark.parametrize("form", ["mask", "nomask", "mss"])
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "random"])
@pytest.mark.parametrize("nblk", [1, 3])
@pytest.mark.parametrize("hw", HWS)
@pytest.mark.parametrize("C,Cp", CCP)
def test_bn_backward_chain(lib, C, Cp, hw, nblk, exact, form, gout_on):
    g = _gen(40 + Cp + hw + nblk)
    nb = [4, 2, 0] if exact else [5, 2, 0]
    exact_div = exact and hw in (1, 4)  # cnt = nb * hw a power of two: the means and dy are exact too
    rows = nb[0] * hw
    dz, y = (_poison(_data(g, exact, P, rows, Cp), nb, hw) for _ in range(2))
    mask = _poison(_data(g, exact, P, rows, Cp).clamp_min(0), nb, hw)  # a ReLU output: about half zeros
    ms = torch.zeros(P, 2, Cp, dtype=F64)
    ms[:, 0, :C] = _eighths(g, P, C, lim=2) if exact else torch.randn(P, C, generator=g).float().double()
    ms[:, 1, :C] = _pow2(g, P, C) if exact else (torch.rand(P, C, generator=g) + 0.5).float().double()
    mss = _ss(g, exact, C, Cp) if form == "mss" else None
    gamma = _pow2(g, P, C) if exact else (torch.rand(P, C, generator=g) + 0.5).float().double()
    mk = mask if form == "mask" else None
    nr = lib.conv_bnb_rows()
    param_ps, part_ps = C + 3, nr * 2 * Cp + 16
    PRE = 0.5  # dgamma / dbeta are accumulated into

    dzd, yd, mkd = _dev(dz), _dev(y), _dev(mask)
    msd, mssd, nbd = _f32(ms), (_f32(mss) if mss is not None else None), _i32(nb)
    gmd = _dev(gamma, torch.float32, gap=3)
    part = torch.zeros(P, part_ps, dtype=torch.float32, device="cuda")
    part[:, nr * 2 * Cp:] = R.NAN
    mk_ptr = mkd.data_ptr() if mk is not None else None
    mss_ptr = mssd.data_ptr() if mss is not None else None

    # --- reduce -------------------------------------------------------------------------------
    ref_g, margin = R.bn_bwd_g(dz, mk, y, mss, nb, hw)
    if margin is not None:  # a pre-activation within fp32 noise of zero may fall on either side
        mbig = torch.maximum((y * mss[:, None, 0]).abs(), mss[:, None, 1].abs().expand_as(y))
        unsure = torch.nan_to_num(margin, nan=1.0) < 2.0 ** -20 * torch.nan_to_num(mbig)
        if exact:
            unsure = torch.zeros_like(unsure)  # y * sc + sh is exact, zero included
        assert float(unsure.float().mean()) <= 1e-3 and not unsure.any()  # random normal inputs give none
    gout = _out(ref_g.shape) if gout_on else None
    rc = lib.cnn_bn_bwd_reduce(dzd.data_ptr(), dzd.shape[1], mk_ptr, mkd.shape[1], yd.data_ptr(), yd.shape[1], msd.data_ptr(), nbd.data_ptr(), hw, Cp,
                               part.data_ptr(), part_ps, nblk, gout.data_ptr() if gout_on else None, gout.shape[1] if gout_on else 0, P, _stream(), mss_ptr)
    assert rc == 0
    if gout_on:
        _exact("bn_bwd gout", gout, ref_g)  # a bf16 value or zero: exact in every case
    torch.cuda.synchronize()
    host = part.cpu()
    assert torch.isnan(host[:, nr * 2 * Cp:]).all()
    got_sums = host[:, : nr * 2 * Cp].reshape(P, nr, 2, Cp).double().sum(1)
    sums, sums32 = R.bn_bwd_sums(ref_g, y, ms, nb, hw), R.bn_bwd_sums(ref_g, y, ms, nb, hw, dtype=torch.float32)
    assert not got_sums[2].any(), "the peer without samples adds nothing"
    if exact:
        _fp32_equal("bn_bwd sums", got_sums, sums, sums32)
    else:
        short = [max(0, n - 1) for n in nb]  # the last sample's rows dropped
        wrong = R.bn_bwd_sums(ref_g, y, ms, short, hw)
        _fp32_close("bn_bwd sums", got_sums, sums, sums32, wrong)  # MI355X: worst |err| / bound 0.56

    # --- finalize on the GPU's own partial sums -------------------------------------------------
    def finalize(part_buf):
        dga = torch.full((P, param_ps), PRE, dtype=torch.float32, device="cuda")
        dbe = torch.full((P, param_ps), PRE, dtype=torch.float32, device="cuda")
        coef = torch.full((P, 3, Cp), R.NAN, dtype=torch.float32, device="cuda")
        rc = lib.cnn_bn_bwd_finalize(part_buf.data_ptr(), part_ps, nr, nbd.data_ptr(), hw, gmd.data_ptr(), param_ps, msd.data_ptr(), dga.data_ptr(),
                                     dbe.data_ptr(), C, Cp, coef.data_ptr(), P, _stream())
        assert rc == 0
        torch.cuda.synchronize()
        left = part_buf.cpu()
        assert not left[:, : nr * 2 * Cp].any(), "the accumulator rows are re-armed"
        assert torch.isnan(left[:, nr * 2 * Cp:]).all()
        dga, dbe, coef = dga.cpu(), dbe.cpu(), coef.cpu()
        assert (dga[:, C:] == PRE).all() and (dbe[:, C:] == PRE).all() and not coef[:, :, C:].any()
        return dga[:, :C], dbe[:, :C], coef

    def check_finalize(tag, got, rows_in):
        """``rows_in``: the accumulator rows [P, nr, 2, Cp] the kernel was given (fp32 values)"""
        ref = R.bn_bwd_finalize(rows_in, nb, hw, gamma, ms, C, Cp)
        ref32 = R.bn_bwd_finalize(rows_in, nb, hw, gamma, ms, C, Cp, dtype=torch.float32)
        wrong = R.bn_bwd_finalize(rows_in, nb, hw, gamma * 1.01, ms, C, Cp, count=lambda n: max(1, n) + 1)  # gamma 1 % off, wrong count
        for i, nm in enumerate(("dgamma", "dbeta")):
            want = ref[i] + PRE
            if exact:
                _fp32_equal(f"{tag} {nm}", got[i], want, ref32[i] + PRE)
            else:
                _fp32_close(f"{tag} {nm}", got[i], want, ref32[i] + PRE, PRE + ref[i] * 0.99)  # MI355X: worst |err| / bound 0.25
        if exact_div:
            _fp32_equal(f"{tag} coef", got[2], ref[2], ref32[2])
        else:
            _fp32_close(f"{tag} coef", got[2], ref[2], ref32[2], wrong[2])  # MI355X: worst |err| / bound 0.25

    fin = finalize(part)
    assert torch.equal(fin[0][2], torch.full((C,), PRE)) and torch.equal(fin[1][2], torch.full((C,), PRE)), "no samples: nothing to add"
    check_finalize("bn_bwd_finalize[chain]", fin, host[:, : nr * 2 * Cp].reshape(P, nr, 2, Cp).double())

    # --- finalize alone: partial sums spread over every accumulator row -------------------------
    spread = _eighths(g, P, nr, 2, Cp) if exact else torch.randn(P, nr, 2, Cp, generator=g).float().double()
    part2 = torch.zeros(P, part_ps, dtype=torch.float32, device="cuda")
    part2[:, : nr * 2 * Cp] = spread.reshape(P, -1).float().cuda()
    part2[:, nr * 2 * Cp:] = R.NAN
    check_finalize("bn_bwd_finalize[rows]", finalize(part2), spread)

    # --- apply: on the GPU's own coefficients (chain) and on the oracle's (alone) -----------------
    for tag, coef in (("chain", fin[2]), ("alone", R.bn_bwd_finalize(sums, nb, hw, gamma, ms, C, Cp)[2].float())):
        coefd = coef.contiguous().cuda()
        ref_dy, big = R.bn_bwd_apply(ref_g, y, ms, coef.double(), nb, hw)
        dy = _out(ref_dy.shape)
        rc = lib.cnn_bn_bwd_apply(dzd.data_ptr(), dzd.shape[1], mk_ptr, mkd.shape[1], yd.data_ptr(), yd.shape[1], msd.data_ptr(), coefd.data_ptr(),
                                  nbd.data_ptr(), 1, hw, Cp, dy.data_ptr(), dy.shape[1], P, _stream(), mss_ptr)
        assert rc == 0
        if exact_div:
            ref32, _ = R.bn_bwd_apply(ref_g, y, ms, coef.double(), nb, hw, dtype=torch.float32)
            _exact(f"bn_bwd_apply[{tag}]", dy, ref_dy, ref32)
        else:
            if form == "mask":  # the mask taken as >= 0 (a ReLU output holds exact zeros)
                wg, _ = R.bn_bwd_g(dz, mk, y, mss, nb, hw, live=lambda t: t >= 0)
                wrong, _ = R.bn_bwd_apply(wg, y, ms, coef.double(), nb, hw)
            else:  # no stored mask to get wrong (a random pre-activation is never exactly zero): gamma / std 1 % off
                wrong = ref_dy * 1.01
            _bf16_close(f"bn_bwd_apply[{tag}]", dy, ref_dy, big, wrong)  # MI355X: worst |err| / bound 0.50
        got, _ = _read(dy, ref_dy)
        assert not got[:2, :, C:].nan_to_num().any(), "padding channels: zero coefficients give zero"


@pytest.mark.parametrize("hw", HWS)
@pytest.mark.parametrize("C,Cp", CCP)
def test_relu_bwd(lib, C, Cp, hw):
    g = _gen(50 + Cp + hw)
    nb = [5, 2, 0]
    rows = nb[0] * hw
    dz = _poison(_normal(g, P, rows, Cp), nb, hw)
    mask = _poison(_normal(g, P, rows, Cp).clamp_min(0), nb, hw)
    dzd, mkd, nbd = _dev(dz), _dev(mask), _i32(nb)
    ref = R.relu_bwd(dz, mask, nb, hw)
    out = _out(ref.shape)
    rc = lib.cnn_relu_bwd(dzd.data_ptr(), dzd.shape[1], mkd.data_ptr(), mkd.shape[1], nbd.data_ptr(), 1, hw, Cp, out.data_ptr(), out.shape[1], P, _stream())
    assert rc == 0
    _exact("relu_bwd", out, ref)
    got, ok = _read(out, ref)
    assert (got[ok] == 0).float().mean() > 0.3 and (got[ok] != 0).float().mean() > 0.3


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "random"])
@pytest.mark.parametrize("nblk", [1, 3])
@pytest.mark.parametrize("hw", HWS)
@pytest.mark.parametrize("C,Cp", CCP)
def test_colsum(lib, C, Cp, hw, nblk, exact):
    g = _gen(60 + Cp + hw)
    nb, PRE = [5, 2, 0], 0.5
    x = _poison(_data(g, exact, P, nb[0] * hw, Cp), nb, hw)
    xd, nbd = _dev(x), _i32(nb)
    out_ps = Cp + 5
    out = torch.full((P, out_ps), PRE, dtype=torch.float32, device="cuda")
    rc = lib.cnn_colsum(xd.data_ptr(), xd.shape[1], nbd.data_ptr(), hw, Cp, C, out.data_ptr(), out_ps, nblk, P, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    got = out.cpu()
    assert (got[:, C:] == PRE).all(), "padding channels and the gap are not accumulated into"
    assert (got[2] == PRE).all()
    ref, ref32 = R.colsum(x, nb, hw, C) + PRE, R.colsum(x, nb, hw, C, dtype=torch.float32) + PRE
    if exact:
        _fp32_equal("colsum", got[:, :C], ref, ref32)
    else:
        _fp32_close("colsum", got[:, :C], ref, ref32, R.colsum(x, nb, hw, C, drop_last=True) + PRE)  # MI355X: worst |err| / bound 0.16


# ---------------------------------------------------------------------------------------------
# pooling
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,fill", [(4, 4, R.NAN), (6, 2, R.NAN), (5, 5, 0.0), (5, 5, R.NAN)])
@pytest.mark.parametrize("Cp", [8, 24])
def test_maxpool2(lib, H, W, Cp, fill):
    g = _gen(70 + H + Cp)
    B, nb = 3, [3, 2, 0]
    x = torch.randint(0, 2, (P, B, H, W, Cp), generator=g).double() / 8  # 0 or 1/8, as after a ReLU: three windows in four tie
    dy = _eighths(g, P, B, H // 2, W // 2, Cp)
    w = R.windows(x[:2])
    assert ((w == w.max(0).values).sum(0) > 1).float().mean() > 0.5
    xd, dyd, nbd = _dev(_poison(x, nb, 1)), _dev(_poison(dy, nb, 1)), _i32(nb)
    ref = R.maxpool2(x, nb)
    out = _out(ref.shape)
    rc = lib.cnn_maxpool2(0, xd.data_ptr(), xd.shape[1], None, 0, nbd.data_ptr(), B, H, W, Cp, out.data_ptr(), out.shape[1], P, _stream())
    assert rc == 0
    _exact("maxpool2 fwd", out, ref)
    # backward: dy to the first maximum; with odd H / W the last row / column belongs to no window
    # and is never written (the engine keeps it zero), which the NaN-filled run shows directly
    ref_dx = R.maxpool2_bwd(x, dy, nb)
    dx = _out(ref_dx.shape, fill=fill)
    rc = lib.cnn_maxpool2(1, xd.data_ptr(), xd.shape[1], dyd.data_ptr(), dyd.shape[1], nbd.data_ptr(), B, H, W, Cp, dx.data_ptr(), dx.shape[1], P, _stream())
    assert rc == 0
    _exact("maxpool2 bwd", dx, ref_dx, fill=fill)
    got, ok = _read(dx, ref_dx, fill)
    last = R.maxpool2_bwd(x, dy, nb, last=True)
    assert (got != last)[ok].any(), "first-maximum and last-maximum routing differ on these inputs"


@pytest.mark.parametrize("hw", [1, 4, 16, 25])
@pytest.mark.parametrize("Cp", [8, 24])
def test_avgpool(lib, hw, Cp):
    g = _gen(80 + hw + Cp)
    B, nb = 4, [4, 1, 0]
    exact = hw != 25  # 1 / hw is a power of two
    x = _data(g, exact, P, B, hw, Cp)
    dy = _data(g, exact, P, B, Cp)
    xd, dyd, nbd = _dev(_poison(x, nb, 1)), _dev(_poison(dy, nb, 1)), _i32(nb)
    ref, big = R.avgpool(x, nb)
    out = _out(ref.shape)
    rc = lib.cnn_avgpool(0, xd.data_ptr(), xd.shape[1], nbd.data_ptr(), B, hw, Cp, out.data_ptr(), out.shape[1], P, _stream())
    assert rc == 0
    ref_dx, big_dx = R.avgpool_bwd(dy, nb, hw)
    dx = _out(ref_dx.shape)
    rc = lib.cnn_avgpool(1, dyd.data_ptr(), dyd.shape[1], nbd.data_ptr(), B, hw, Cp, dx.data_ptr(), dx.shape[1], P, _stream())
    assert rc == 0
    if exact:
        _exact("avgpool fwd", out, ref, R.avgpool(x, nb, dtype=torch.float32)[0])
        _exact("avgpool bwd", dx, ref_dx, R.avgpool_bwd(dy, nb, hw, dtype=torch.float32)[0])
    else:  # wrong references: the mean over one position fewer
        _bf16_close("avgpool fwd", out, ref, big, ref * hw / (hw - 1))  # MI355X: worst |err| / bound 0.49
        _bf16_close("avgpool bwd", dx, ref_dx, big_dx, ref_dx * hw / (hw - 1))  # MI355X: worst |err| / bound 0.48


# ---------------------------------------------------------------------------------------------
# log-softmax + NLL head
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["train", "eval"])
@pytest.mark.parametrize("K,Lp", [(10, 16), (16, 16)])
def test_xent(lib, K, Lp, form):
    g = _gen(90 + K)
    B, nb = 5, [5, 3, 0]
    logits = _eighths(g, P, B, Lp)
    top = torch.randint(0, K, (P, B), generator=g)
    logits.scatter_(2, top[..., None], logits[..., :K].max(2, keepdim=True).values + 0.125)  # a unique maximum per row
    logits[..., K:] = R.NAN  # padding columns are never read
    labels = torch.where(torch.rand(P, B, generator=g) < 0.5, top, torch.randint(0, K, (P, B), generator=g))
    loss, correct, conf, dl = R.xent(logits, labels, nb, K)
    lgd, lbd, nbd = _dev(_poison(logits, nb, 1)), _i32(labels.reshape(-1).tolist()), _i32(nb)
    pre = torch.tensor([[0.5, 3.0, 7.0, 9.0]] * P)
    stats = pre.clone().cuda()
    confd = torch.ones(P, 16, 16, dtype=torch.int32, device="cuda") if form == "eval" else None
    dld = _out(dl.shape) if form == "train" else None
    rc = lib.cnn_xent(lgd.data_ptr(), lgd.shape[1], Lp, K, lbd.data_ptr(), B, nbd.data_ptr(), stats.data_ptr(), confd.data_ptr() if confd is not None else None,
                      dld.data_ptr() if dld is not None else None, dld.shape[1] if dld is not None else 0, P, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    got = stats.cpu().double() - pre.double()
    assert not got[:, 2:].any() and not got[2].any()
    assert torch.equal(got[:, 1], correct)
    assert 0 < correct[0] < B
    # 2^-18 * (1 + max|z|) per valid row: __expf / __logf scale their argument in fp32
    bound = torch.tensor([sum(2.0 ** -18 * (1 + float(logits[p, b, :K].abs().max())) for b in range(nb[p])) for p in range(P)], dtype=F64)
    err = (got[:, 0] - loss).abs()
    print(f"xent loss: |err| {err.tolist()}, bound {bound.tolist()}")  # MI355X: worst |err| / bound 0.009
    assert (err <= bound).all()
    short, _, _, _ = R.xent(logits, labels, [n - 1 if n else 0 for n in nb], K)  # one valid row dropped
    assert ((got[:, 0] - short).abs() > bound)[:2].all()
    if form == "eval":
        assert torch.equal(confd.cpu().long() - 1, conf)
    else:
        # rows >= nb (the whole empty peer) and columns >= K are written as exact zeros
        host = dld.cpu()[:, : B * Lp].reshape(P, B, Lp)
        for p in range(P):
            assert (host[p, nb[p]:] == 0).all()
        assert (host[:, :, K:] == 0).all()
        wrong = dl * torch.tensor([n / (n - 1) if n > 1 else 1.0 for n in nb], dtype=F64)[:, None, None]  # divided by nb - 1
        big = torch.tensor([1.0 / max(1, n) for n in nb], dtype=F64)[:, None, None].expand_as(dl)
        _bf16_close("xent dlogits", dld, dl, big, wrong)  # MI355X: worst |err| / bound 0.49


def test_xent_rejects_unsupported_widths(lib):
    t = torch.zeros(64, dtype=torch.int32, device="cuda")  # never read: both calls return before any launch
    assert lib.cnn_xent(t.data_ptr(), 32, 32, 17, t.data_ptr(), 1, t.data_ptr(), t.data_ptr(), None, None, 0, 1, _stream()) == 1
    assert lib.cnn_xent(t.data_ptr(), 8, 8, 10, t.data_ptr(), 1, t.data_ptr(), t.data_ptr(), None, None, 0, 1, _stream()) == 1


def test_row_kernels_reject_channel_counts_not_a_multiple_of_8(lib):
    t = torch.zeros(256, dtype=torch.float32, device="cuda")  # never touched: every call returns before any launch
    p, s = t.data_ptr(), _stream()
    assert lib.cnn_bn_act(p, 64, p, None, 0, None, 0, None, 1, p, 1, 1, 12, p, 64, 1, s) == 1
    assert lib.cnn_bn_bwd_reduce(p, 64, None, 0, p, 64, p, p, 1, 12, p, 64, 1, None, 0, 1, s, None) == 1
    assert lib.cnn_bn_bwd_apply(p, 64, None, 0, p, 64, p, p, p, 1, 1, 12, p, 64, 1, s, None) == 1
    assert lib.cnn_relu_bwd(p, 64, p, 64, p, 1, 1, 12, p, 64, 1, s) == 1
    assert lib.cnn_colsum(p, 64, p, 1, 12, 12, p, 64, 1, 1, s) == 1
    torch.cuda.synchronize()
    assert not t.any()


# ---------------------------------------------------------------------------------------------
# fused SGD + bf16 shadow refresh
# ---------------------------------------------------------------------------------------------
def _opt_layout(g, zero_after):
    """Five segments in one flat parameter vector: a 3x3 conv with 3 input channels (rows of 27:
    scalar passes), a 3x3 conv with 8 at a 16-byte aligned offset (float4 passes), the same conv one
    float further (scalar fallback; its shadow on an 8-byte boundary: scalar shadow pass), a 1x1 fc
    with 20 torch columns in 24 engine channels behind a shuffled column map, and a plain vector of
    300 (two chunks, the second partial)."""
    t2e = torch.randperm(24, generator=g)[:20]
    e2t = torch.full((24,), -1, dtype=torch.int64)
    e2t[t2e] = torch.arange(20)
    z = dict(zero_after=zero_after, e2t=None, t2e=None)
    segs = [
        dict(off=0, n=54, kind=1, cout=2, cin=3, R=3, S=3, cp_in=8, wf_off=0, **z),
        dict(off=56, n=144, kind=1, cout=2, cin=8, R=3, S=3, cp_in=8, wf_off=144, **z),
        dict(off=201, n=144, kind=1, cout=2, cin=8, R=3, S=3, cp_in=8, wf_off=292, **z),
        dict(off=348, n=60, kind=1, cout=3, cin=20, R=1, S=1, cp_in=24, wf_off=440, zero_after=zero_after, e2t=e2t, t2e=t2e),
        dict(off=409, n=300, kind=0, cout=0, cin=0, R=0, S=0, cp_in=0, wf_off=0, **z),
    ]
    work = [(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1), (3, 0), (3, 1), (3, 2), (4, 0), (4, 1)]
    return segs, work, 720, 520  # ps, gf_ps = shadow_ps


def _opt_device_tables(segs, work):
    from myfyp_amd.parallel.cnn_engine import Segment

    keep, rows = [], []
    for s in segs:
        maps = [0, 0]
        if s["e2t"] is not None:
            keep += [_i32(s["e2t"].tolist()), _i32(s["t2e"].tolist())]
            maps = [keep[-2].data_ptr(), keep[-1].data_ptr()]
        rows.append(Segment(s["off"], s["n"], s["kind"], s["cout"], s["cin"], s["R"], s["S"], s["cp_in"], 8, s["zero_after"], 0, s["wf_off"], *maps))
    arr = (Segment * len(rows))(*rows)
    segd = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()
    workd = torch.tensor(work, dtype=torch.int32).reshape(-1, 2).cuda()
    return segd, workd, keep


OPT_VARIANTS = {
    "plain": dict(momentum=0.0, weight_decay=0.0, nesterov=False, mu=0.0),
    "momentum_wd": dict(momentum=0.5, weight_decay=0.25, nesterov=False, mu=0.0),
    "nesterov": dict(momentum=0.5, weight_decay=0.0, nesterov=True, mu=0.0),
    "fedprox_scaffold": dict(momentum=0.0, weight_decay=0.0, nesterov=False, mu=0.5),
}


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "random"])
@pytest.mark.parametrize("zero_after", [1, 0])
@pytest.mark.parametrize("variant", list(OPT_VARIANTS))
def test_opt_step(lib, variant, zero_after, exact):
    g = _gen(100)
    segs, work, ps, fps = _opt_layout(g, zero_after)
    segd, workd, _keep = _opt_device_tables(segs, work)
    hp = dict(lr=0.25 if exact else 0.05, **OPT_VARIANTS[variant])
    if not exact and hp["momentum"]:
        hp.update(momentum=0.9, weight_decay=hp["weight_decay"] and 5e-4)
    extras = variant == "fedprox_scaffold"

    def rnd(n, lim=4):
        return _eighths(g, P, n, lim=lim) if exact else torch.randn(P, n, generator=g).float().double()

    w, m, gr = rnd(ps), torch.zeros(P, ps, dtype=F64), rnd(ps)
    gf = rnd(fps)
    anchor, cg, cl = (rnd(ps, lim=1) for _ in range(3)) if extras else (None, None, None)
    active = [1, 0, 1]
    wd_, md_, grd, gfd = _f32(w), _f32(m), _f32(gr), _f32(gf)
    ad, cgd, cld = (_f32(t) for t in (anchor, cg, cl)) if extras else (None, None, None)
    shadow = torch.full((P, fps), R.NAN, dtype=BF, device="cuda")
    sh_ref = torch.full((P, fps), R.NAN, dtype=F64)
    actd = _i32(active)

    def launch(update, act):
        rc = lib.cnn_opt_step(wd_.data_ptr(), grd.data_ptr(), md_.data_ptr(), ps, gfd.data_ptr(), fps, segd.data_ptr(), workd.data_ptr(), len(work), 1,
                              hp["lr"], hp["momentum"], hp["weight_decay"], int(hp["nesterov"]), hp["mu"], ad.data_ptr() if extras else None,
                              cgd.data_ptr() if extras else None, cld.data_ptr() if extras else None, update, shadow.data_ptr(), fps,
                              act.data_ptr() if act is not None else None, P, _stream())
        assert rc == 0
        torch.cuda.synchronize()

    covered = torch.zeros(fps, dtype=torch.bool)
    for s in segs:
        if s["kind"] == 1:
            covered[s["wf_off"]: s["wf_off"] + s["cout"] * s["R"] * s["S"] * s["cp_in"]] = True

    def check_shadow(peers):
        """the shadow is bf16(master weight) in [cout][R][S][cp_in] order, zero in the padding channels"""
        host, wnow = shadow.cpu(), wd_.cpu().double()
        for p in range(P):
            if p not in peers:
                assert torch.isnan(host[p]).all(), "an inactive peer's shadow was written"
                continue
            assert torch.isnan(host[p, ~covered]).all(), "the shadow was written outside its layers"
            for s in segs[:4]:
                rs, nf = s["R"] * s["S"], s["cout"] * s["R"] * s["S"] * s["cp_in"]
                want = R.wf_shadow(wnow[p, s["off"]: s["off"] + s["n"]].reshape(s["cout"], s["cin"], rs), s["cp_in"], s["e2t"])
                got = host[p, s["wf_off"]: s["wf_off"] + nf].reshape(s["cout"], rs, s["cp_in"])
                assert torch.equal(got.double(), want.to(BF).double()), f"shadow of the segment at {s['off']}"
                pad = (want == 0).all(0).all(0)
                assert int(pad.sum()) >= s["cp_in"] - s["cin"] and (got[:, :, pad] == 0).all()

    in_seg = torch.zeros(ps, dtype=torch.bool)
    for s in segs:
        in_seg[s["off"]: s["off"] + s["n"]] = True

    for step in range(2):  # the second step starts from the first one's momentum
        before = [t.cpu().clone() for t in (wd_, md_, grd, gfd)]
        ref = R.opt_step(w, gr, m, gf, sh_ref, segs, hp, active, 1, anchor, cg, cl)
        ref32 = R.opt_step(w, gr, m, gf, sh_ref, segs, hp, active, 1, anchor, cg, cl, dtype=torch.float32)
        wrong = list(R.opt_step(w, gr, m, gf, sh_ref, segs, dict(hp, lr=hp["lr"] * 1.01), active, 1, anchor, cg, cl))  # lr 1 % off
        wrong[2] = ref[2] * 1.01  # the step size does not enter the momentum buffer: the buffer itself 1 % off
        launch(1, actd)
        got = [t.cpu() for t in (wd_, md_, grd, gfd)]
        # the inactive peer and everything between the segments: bit-unchanged
        for a, b in zip(got, before):
            assert torch.equal(a[1], b[1])
        assert torch.equal(got[0][:, ~in_seg], before[0][:, ~in_seg]) and torch.equal(got[1][:, ~in_seg], before[1][:, ~in_seg])
        # consumed gradients: re-zeroed, or left exactly as they were
        assert torch.equal(got[2].double(), ref[1]) and torch.equal(got[3].double(), ref[3])
        if zero_after:
            assert not got[2][0, 409:709].any() and not got[3][0, covered].any() and torch.equal(got[3][:, ~covered], before[3][:, ~covered])
        else:
            assert torch.equal(got[2], before[2]) and torch.equal(got[3], before[3])
        for i, k, nm in ((0, 0, "w"), (1, 2, "m")):  # got is (w, m, g, gf), the reference (w, g, m, gf, shadow)
            if exact:
                _fp32_equal(f"opt_step[{variant}] {nm} step {step}", got[i], ref[k], ref32[k])
            elif nm == "w" or hp["momentum"]:
                _fp32_close(f"opt_step[{variant}] {nm} step {step}", got[i], ref[k], ref32[k], wrong[k])  # MI355X: worst |err| / bound 0.24 (w), 0.19 (m)
            else:
                assert not got[i].any()
        check_shadow((0, 2))
        # carry on from the kernel's own fp32 state with fresh gradients
        w, m = got[0].double(), got[1].double()
        gr, gf = rnd(ps), rnd(fps)
        grd.copy_(_f32(gr))
        gfd.copy_(_f32(gf))

    # update = 0: only the shadow changes, for every peer
    before = [t.cpu().clone() for t in (wd_, md_, grd, gfd)]
    launch(0, None)
    for a, b in zip([t.cpu() for t in (wd_, md_, grd, gfd)], before):
        assert torch.equal(a, b)
    check_shadow((0, 1, 2))
