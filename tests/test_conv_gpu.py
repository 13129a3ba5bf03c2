"""Every kernel of ``csrc/kernels/conv.hip`` against the float64 oracle of ``tests/_conv_ref.py``, driven
directly through ``conv_gemm_launch`` / ``conv_wgrad_launch`` / the flip launchers.

The kernels multiply bf16 operands and accumulate in fp32. With operands on a coarse dyadic grid
(``_conv_ref.FAMILIES``; ``tests/test_conv_ref_cpu.py`` proves the condition for every case used
here) each product and each partial sum is exact in fp32 in ANY order — tile order, split-K atomics,
stage rings, spread accumulator rows — so the kernel must equal the oracle bit for bit after one
round-to-nearest-even to bf16, and an fp32 gradient or column sum must equal it exactly:

* ternary: outputs, sum x, sum x^2, the BN-backward sums and the weight gradients are all exact;
* eighths: accumulators, outputs (the bf16 rounding is exercised), sum x, sum g and the weight
  gradients are exact; sum x^2 and sum g * xhat are exact only in the cases where their terms stay
  below 2^24 grid units (``_conv_ref.sq_exact`` / ``xhat_exact``, asserted there too); elsewhere
  they get ``_cnn_ops_ref.fp32_bound`` (four times the error of the torch fp32 evaluation of the
  same formula) with a wrong reference that must fail;
* randn: one sanity case per kernel family at ``bf16_bound`` (one bf16 ulp + 2^-20 * M, M = the
  element's sum of |term|, which no partial sum exceeds: 2^-20 * M is 16 fp32 roundings that all go
  the same way; the chains here are 3 to 18 MFMA accumulations long).

Common set-up: 3 peers with ``nbatch = [n, partial, 0]`` (the engine hands a peer past its data, and
an inactive slot, ``nb = 0``), a per-peer stride larger than the slab, NaN in every input row at or
beyond a peer's valid extent, NaN (bf16 outputs) or a marker (fp32 accumulators) wherever the kernel
has nothing to write. The device operands are built once per case and shared by every variant;
after each test they must still hold what was uploaded. Every exact group also checks the oracle with ONE operand element moved by
one grid unit (``_conv_ref.controls``): it must differ from what the kernel wrote.
"""

import ctypes
import functools

import pytest
import torch

import _cnn_ops_ref as O
import _conv_ref as C

pytestmark = pytest.mark.gpu

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
P = C.P
GAP = 64  # elements between one peer's slab and the next (keeps 16-byte alignment)
MARK = 777.0  # marker in the gaps of fp32 accumulators (and in a gradient slab that is to be stored)
NAN = C.NAN


@pytest.fixture(scope="module")
def lib():
    from myfyp_amd.parallel.cnn_engine import _lib

    return _lib()


# conv_set_dma code, conv_set_dma_wgs, conv_set_fwd_halo: the codes of test_cnn_engine_gpu's conv_dma
# fixture, plus one workgroup per column tile and peer running every M tile
VARIANTS = {"dma": (1, 0, 1), "dma_persist": (1, 3, 1), "dma_wgs1": (1, 1, 1), "regstage": (0, 0, 0), "dma128x64s3": (3, 0, 1),
            "dma256x64s3": (7, 0, 1), "dma256x128s3": (9, 0, 1), "wgrad2": (32, 0, 1), "wgrad3": (64, 0, 1)}


@pytest.fixture(params=list(VARIANTS))
def variant(request, lib):
    dma, wgs, halo = VARIANTS[request.param]
    old = lib.conv_set_dma(dma), lib.conv_set_dma_wgs(wgs), lib.conv_set_fwd_halo(halo)
    yield request.param
    lib.conv_set_dma(old[0])
    lib.conv_set_dma_wgs(old[1])
    lib.conv_set_fwd_halo(old[2])


# the weight gradient's kernels: register-staged (default), the 2- / 3-stage DMA rings, the halo
# kernel switched off, and the halo kernel with one register stage in flight instead of two
WVARIANTS = {"reg": (1, 1, 2), "dma2": (32, 1, 2), "dma3": (64, 1, 2), "nohalo": (1, 0, 2), "pf1": (1, 1, 1)}


@pytest.fixture(params=list(WVARIANTS))
def wvariant(request, lib):
    dma, halo, pf = WVARIANTS[request.param]
    old = lib.conv_set_dma(dma), lib.conv_set_wgrad_halo(halo), lib.conv_set_wgrad_pf(pf)
    yield request.param
    lib.conv_set_dma(old[0])
    lib.conv_set_wgrad_halo(old[1])
    lib.conv_set_wgrad_pf(old[2])


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _args():
    from myfyp_amd.parallel.cnn_engine import ConvGemmArgs

    return ConvGemmArgs()


def _wargs():
    from myfyp_amd.parallel.cnn_engine import WgradArgs

    return WgradArgs()


# ---------------------------------------------------------------------------------------------
# buffers
# ---------------------------------------------------------------------------------------------
def _poison(t, nb):
    """NaN in the samples no kernel may read: [P, B, ...] samples >= nb[p]."""
    t = t.clone()
    for p, n in enumerate(nb):
        t[p, n:] = NAN
    return t


def _dev(t, dtype=BF, fill=NAN, gap=GAP):
    """dense [P, ...] -> device [P, stride] buffer, ``fill`` in the gap between peers."""
    flat = t.reshape(t.shape[0], -1)
    buf = torch.full((t.shape[0], flat.shape[1] + gap), fill, dtype=dtype, device="cuda")
    buf[:, : flat.shape[1]] = flat.to(dtype).cuda()
    return buf


def _out(n, dtype=BF, fill=NAN, slab=None, gap=GAP):
    """[P, n + gap] output: ``fill`` in the gap, ``slab`` (default ``fill``) in the n used elements."""
    buf = torch.full((P, n + gap), fill, dtype=dtype, device="cuda")
    if slab is not None:
        buf[:, :n] = slab
    return buf


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device="cuda")


def _is(t, fill):
    return torch.isnan(t) if fill != fill else t == fill


def _read(buf, ref, fill=NAN):
    """Device buffer -> dense float64 like ``ref``; the gap and every element the reference marks NaN
    must still hold ``fill``, everything else must have been written."""
    torch.cuda.synchronize()
    n = ref[0].numel()
    host = buf.cpu()
    assert _is(host[:, n:], fill).all(), "the gap between peers was written"
    got = host[:, :n].reshape(ref.shape).double()
    hole = torch.isnan(ref)
    assert _is(got[hole], fill).all(), "an element beyond the valid extent was written"
    if fill != fill:
        assert not torch.isnan(got[~hole]).any(), "a valid element was not written (or a poisoned row was read)"
    return got, ~hole


def _exact(name, buf, ref, fill=NAN):
    """Bit for bit (up to the sign of zero) against the oracle rounded to the buffer's type; returns
    the buffer as float64 with NaN in the holes (comparable with another oracle result)."""
    got, ok = _read(buf, ref, fill)
    want = ref.to(buf.dtype).double()
    bad = (got != want) & ok
    assert not bad.any(), f"{name}: {int(bad.sum())} elements differ, first at {bad.nonzero()[0].tolist()}: {got[bad][0]} vs {want[bad][0]}"
    return torch.where(ok, got, torch.full_like(got, NAN))


def _rows(buf, rows, *shape):
    """Spread accumulator rows [P][rows][shape] summed on the host in float64; the gap keeps MARK."""
    torch.cuda.synchronize()
    n = rows
    for s in shape:
        n *= s
    host = buf.cpu()
    assert (host[:, n:] == MARK).all(), "the gap between the peers' accumulator rows was written"
    return host[:, :n].reshape(P, rows, *shape).double().sum(1)


def _equal(name, got, ref):
    bad = got.double() != ref
    assert not bad.any(), f"{name}: {int(bad.sum())} elements differ, first at {bad.nonzero()[0].tolist()}: {got[bad][0]} vs {ref[bad][0]}"


def _fp32_close(name, got, ref64, ref32, wrong64):
    bound = O.fp32_bound(ref64, ref32)
    err = float((got.double() - ref64).abs().max())
    print(f"{name}: |err| {err:.3e}, bound {bound:.3e}, ratio {err / bound:.3f}")
    assert err <= bound, f"{name}: {err:.3e} > {bound:.3e}"
    assert float((got.double() - wrong64).abs().max()) > bound, f"{name}: the wrong reference passes too"


def _bf16_close(name, buf, ref64, big, wrong64):
    got, ok = _read(buf, ref64)
    bound = O.bf16_bound(torch.nan_to_num(ref64), torch.nan_to_num(big))
    ratio = float(((got - ref64).abs() / bound)[ok].max())
    print(f"{name}: worst |err| / bound = ratio {ratio:.3f}")
    assert ratio <= 1.0, f"{name}: {ratio:.3f} x the bf16 bound"
    assert ((got - wrong64).abs() > bound)[ok & ~torch.isnan(wrong64)].any(), f"{name}: the wrong reference passes too"


# ---------------------------------------------------------------------------------------------
# cases: inputs, oracle, controls and device operands, built once and shared by every variant
# ---------------------------------------------------------------------------------------------
_USED = []  # the cases the running test took its operands from


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


@pytest.fixture(autouse=True)
def _operands_intact():
    """The device operands are built once per case and shared by every variant: a kernel that wrote
    into one of them must fail the test that ran it, not a later one."""
    _USED.clear()
    yield
    torch.cuda.synchronize()
    for k in _USED:
        for key, t in list(k["dev"].items()) + [("nbatch", k["nbd"])]:
            if t is not None:
                assert torch.equal(_bits(t), _bits(k["dev0"][key])), f"the launch overwrote its operand {key}"


def _prep(kind, name, family):
    k = _build(kind, name, family)
    _USED.append(k)
    return k


@functools.lru_cache(maxsize=None)
def _build(kind, name, family):
    d = C.inputs(kind, name, family)
    nb = d["nb"]
    k = {"d": d, "nbd": _i32(nb)}
    exact = family in C.FAMILIES
    if kind == "fwd":
        k["ref"] = C.fwd_oracle(d)
        k["ref32"] = C.fwd_oracle(d, dtype=F32) if family == "eighths" else None
        k["sq_exact"] = exact and C.sq_exact(d, k["ref"][1])
        k["dev"] = {"x": _dev(_poison(d["x"], nb)), "w": _dev(d["w"]),
                    "bias": None if d["bias"] is None else _dev(d["bias"], F32),
                    "resid": None if d["resid"] is None else _dev(_poison(d["resid"], nb)),
                    "pro_ss": None if d["pro_ss"] is None else _dev(d["pro_ss"], F32)}
    elif kind == "dgrad":
        k["ref"] = C.dgrad_oracle(d)
        k["ref32"] = C.dgrad_oracle(d, dtype=F32) if family == "eighths" else None
        k["wrong"] = C.dgrad_oracle(d, round_g=False) if family == "eighths" else None
        k["xh_exact"] = exact and d["y0"] is not None and C.xhat_exact(d, k["ref"][0])
        k["dev"] = {"dy": _dev(_poison(d["dy"], nb)), "w": _dev(d["w"])}
        for key in ("resid", "mask", "y0", "y1"):
            k["dev"][key] = None if d[key] is None else _dev(_poison(d[key], nb))
        for key in ("mask_ss", "ms0", "ms1"):
            k["dev"][key] = None if d[key] is None else _dev(d[key], F32, gap=(GAP if key == "mask_ss" else 0))
        k["dev"]["bias"] = _dev(torch.zeros(P, d["cpi"], dtype=F64), F32) if d["zero_bias"] else None
    else:
        k["ref"] = C.wgrad_oracle(d)
        k["dev"] = {"dy": _dev(_poison(d["dy"], nb)), "x": _dev(_poison(d["x"], nb)),
                    "pro_ss": None if d["pro_ss"] is None else _dev(d["pro_ss"], F32)}
    k["ctl"] = {label: C.oracle(kind, d, **over) for label, over in C.controls(kind, d).items()} if exact else {}
    k["dev0"] = {key: (None if t is None else t.clone()) for key, t in k["dev"].items()}
    k["dev0"]["nbatch"] = k["nbd"].clone()
    return k


def _ptr(t):
    return None if t is None else t.data_ptr()


def _ps(t):
    return 0 if t is None else t.shape[1]


# ---------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------
def _fwd_args(lib, k):
    d, dv = k["d"], k["dev"]
    a = _args()
    a.src, a.src_ps, a.src_h, a.src_w, a.src_c = dv["x"].data_ptr(), dv["x"].shape[1], d["H"], d["W"], d["cpi"]
    a.out_h, a.out_w, a.R, a.S, a.stride, a.pad = d["Ho"], d["Wo"], d["R"], d["S"], d["stride"], d["pad"]
    a.wt, a.wt_ps, a.ncol, a.ncol_valid = dv["w"].data_ptr(), dv["w"].shape[1], d["cpo"], d["cout"]
    a.bias, a.bias_ps, a.resid, a.resid_ps = _ptr(dv["bias"]), _ps(dv["bias"]), _ptr(dv["resid"]), _ps(dv["resid"])
    a.relu, a.pro_ss, a.pro_ss_ps = int(d["relu"]), _ptr(dv["pro_ss"]), _ps(dv["pro_ss"])
    a.nbatch, a.max_batch = k["nbd"].data_ptr(), d["n"]
    out = _out(d["n"] * d["Ho"] * d["Wo"] * d["cpo"])
    a.out, a.out_ps = out.data_ptr(), out.shape[1]
    rows, st = 0, None
    if "t" in d["ops"] or "1" in d["ops"]:
        rows = 1 if "1" in d["ops"] else lib.conv_gemm_stats_rows(d["n"], d["Ho"], d["Wo"])
        st = _out(rows * 2 * d["cpo"], F32, MARK, 0.0)
        a.stats, a.stats_ps, a.stats_rows = st.data_ptr(), st.shape[1], rows
    return a, out, st, rows


def _check_stats(name, k, st, rows):
    """Column sums [sum x | sum x^2] of the fp32 values before the rounding; returns the exact part."""
    d, (ref_out, _, ref_st) = k["d"], k["ref"]
    got = _rows(st, rows, 2, d["cpo"])
    _equal(f"{name} sum x", got[:, 0], ref_st[:, 0])
    if k["sq_exact"]:  # every ternary case, and the eighths cases whose squares stay below 2^24 units
        _equal(f"{name} sum x^2", got[:, 1], ref_st[:, 1])
        return got
    wrong = (torch.nan_to_num(ref_out) ** 2).reshape(P, -1, d["cpo"]).sum(1)  # the squares of the ROUNDED outputs
    for p in range(2):  # MI355X: worst |err| / bound 0.40
        _fp32_close(f"{name} sum x^2 peer {p}", got[p, 1], ref_st[p, 1], k["ref32"][2][p, 1], wrong[p])
    assert float(got[2].abs().max()) == 0.0
    return got[:, :1]


@pytest.mark.parametrize("family", C.FAMILIES)
@pytest.mark.parametrize("name", list(C.FWD))
def test_forward_exact(lib, variant, name, family):
    k = _prep("fwd", name, family)
    a, out, st, rows = _fwd_args(lib, k)
    assert lib.conv_gemm_launch(0, ctypes.byref(a), P, _stream()) == 0
    seen = (_exact(name, out, k["ref"][0]),)
    if st is not None:
        seen += (_check_stats(name, k, st, rows),)
    for label, ctl in k["ctl"].items():
        want = ctl if len(seen) == 1 or seen[1].shape[1] == 2 else (ctl[0], ctl[1][:, :1])
        assert C.differs(seen, want), f"{name}: the {label} control equals the kernel's output"


@pytest.mark.parametrize("name", ["k72_5x7_v20_all", "k200_5x5_9x6_s2", "halo_8x32", "halo_8x32_pro"])
def test_forward_randn(lib, variant, name):
    k = _prep("fwd", name, "randn")
    d = k["d"]
    a, out, st, rows = _fwd_args(lib, k)
    assert lib.conv_gemm_launch(0, ctypes.byref(a), P, _stream()) == 0
    act = d["x"] if d["pro_ss"] is None else C.prologue(d["x"], d["pro_ss"])
    absd = {key: (None if d[key] is None else d[key].abs()) for key in ("bias", "resid")}
    big = C.fwd_oracle(d, x=act.abs(), w=d["w"].abs(), pro_ss=None, relu=False, **absd)[1]
    w0 = d["w"].clone()
    w0[:, :, 0, 0, 0] = 0  # one tap-channel product missing
    _bf16_close(name, out, k["ref"][0], big, C.fwd_oracle(d, w=w0)[0])  # MI355X: worst |err| / bound 1.00 (one bf16 ulp)


# ---------------------------------------------------------------------------------------------
# fused BatchNorm finalize in the forward conv's last workgroup
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["k72_5x7_c64", "k576_5x7_c72", "halo_8x32"])
def test_forward_finalize_tail(lib, variant, name):
    k = _prep("fwd", name, "ternary")
    d = k["d"]
    g = C.gen(5)
    cout, cpo, hw = d["cout"], d["cpo"], d["Ho"] * d["Wo"]
    gamma, beta = (torch.rand(P, cout, generator=g) + 0.5).double(), torch.randn(P, cout, generator=g).double()  # fp32 values
    rmean, rvar = torch.randn(P, cout, generator=g).double(), (torch.rand(P, cout, generator=g) + 0.5).double()
    eps, mom = 1e-5, 0.1
    a, out, st, rows = _fwd_args(lib, k)
    cnt = torch.zeros(P * lib.conv_fin_words(), dtype=torch.int32, device="cuda")
    gm, bt = _dev(gamma, F32, gap=3), _dev(beta, F32, gap=3)
    rm, rv = _dev(rmean, F32, MARK, gap=2), _dev(rvar, F32, MARK, gap=2)
    ss = torch.full((P, 2, cpo), NAN, dtype=F32, device="cuda")
    ms = torch.full((P, 2, cpo), NAN, dtype=F32, device="cuda")
    a.fin_cnt, a.fin_gamma0, a.fin_beta, a.fin_param_ps = cnt.data_ptr(), gm.data_ptr(), bt.data_ptr(), gm.shape[1]
    a.fin_rmean, a.fin_rvar, a.fin_run_ps, a.fin_ss, a.fin_ms = rm.data_ptr(), rv.data_ptr(), rm.shape[1], ss.data_ptr(), ms.data_ptr()
    a.fin_C0, a.fin_train, a.fin_eps, a.fin_momentum = cout, 1, eps, mom
    assert lib.conv_gemm_launch(0, ctypes.byref(a), P, _stream()) == 0
    _exact(name, out, k["ref"][0])
    assert float(_rows(st, rows, 2, cpo).abs().max()) == 0.0, "the accumulator rows are not re-armed"
    assert int(cnt.abs().max()) == 0, "the arrival counters are not re-armed"
    stats = k["ref"][2]  # exact in this family: the tail starts from the oracle's sums
    args = (d["nb"], hw, gamma, beta, rmean, rvar, cout, cpo, eps, mom)
    ref, ref32 = C.fin_fwd(stats, *args), C.fin_fwd(stats, *args, dtype=F32)
    wrong = C.fin_fwd(stats, *args, count=lambda n: max(1, n) + 1)
    got = ss.cpu(), ms.cpu(), rm.cpu()[:, :cout], rv.cpu()[:, :cout]
    assert (rm.cpu()[:, cout:] == MARK).all() and (rv.cpu()[:, cout:] == MARK).all()
    assert torch.equal(got[2][2].double(), rmean[2]) and torch.equal(got[3][2].double(), rvar[2])  # no samples: kept bit for bit
    # MI355X, worst |err| / bound: ss 0.23, ms 0.18, rmean 0.22, rvar 0.25
    for nm, g_, r, r32, w in zip(("ss", "ms", "rmean", "rvar"), got, ref, ref32, wrong):
        _fp32_close(f"{name} fin {nm}", g_, r, r32, w)


@pytest.mark.parametrize("name", ["k72_5x7_c64_plain", "halo_8x32_plain"])
def test_forward_finalize_tail_eval(lib, variant, name):
    """Evaluation (``fin_train = 0``, no statistics collected): the constants come from the running
    statistics, which stay as they are."""
    k = _prep("fwd", name, "eighths")
    d = k["d"]
    g = C.gen(7)
    cout, cpo, hw = d["cout"], d["cpo"], d["Ho"] * d["Wo"]
    gamma, beta = (torch.rand(P, cout, generator=g) + 0.5).double(), torch.randn(P, cout, generator=g).double()
    rmean, rvar = torch.randn(P, cout, generator=g).double(), (torch.rand(P, cout, generator=g) + 0.5).double()
    a, out, _, _ = _fwd_args(lib, k)
    cnt = torch.zeros(P * lib.conv_fin_words(), dtype=torch.int32, device="cuda")
    gm, bt = _dev(gamma, F32, gap=3), _dev(beta, F32, gap=3)
    rm, rv = _dev(rmean, F32, MARK, gap=2), _dev(rvar, F32, MARK, gap=2)
    ss = torch.full((P, 2, cpo), NAN, dtype=F32, device="cuda")
    ms = torch.full((P, 2, cpo), NAN, dtype=F32, device="cuda")
    a.fin_cnt, a.fin_gamma0, a.fin_beta, a.fin_param_ps = cnt.data_ptr(), gm.data_ptr(), bt.data_ptr(), gm.shape[1]
    a.fin_rmean, a.fin_rvar, a.fin_run_ps, a.fin_ss, a.fin_ms = rm.data_ptr(), rv.data_ptr(), rm.shape[1], ss.data_ptr(), ms.data_ptr()
    a.fin_C0, a.fin_train, a.fin_eps, a.fin_momentum = cout, 0, 1e-5, 0.1
    assert lib.conv_gemm_launch(0, ctypes.byref(a), P, _stream()) == 0
    _exact(name, out, k["ref"][0])
    assert int(cnt.abs().max()) == 0, "the arrival counters are not re-armed"
    assert torch.equal(rm.cpu()[:, :cout].double(), rmean) and torch.equal(rv.cpu()[:, :cout].double(), rvar)
    none = torch.zeros(P, 2, cpo, dtype=F64)
    ref = C.fin_fwd(none, d["nb"], hw, gamma, beta, rmean, rvar, cout, cpo, 1e-5, 0.1, train=False)
    ref32 = C.fin_fwd(none, d["nb"], hw, gamma, beta, rmean, rvar, cout, cpo, 1e-5, 0.1, train=False, dtype=F32)
    wrong = C.fin_fwd(none, d["nb"], hw, gamma, beta, rmean, rvar * 1.01, cout, cpo, 1e-5, 0.1, train=False)
    _fp32_close(f"{name} fin eval ss", ss.cpu(), ref[0], ref32[0], wrong[0])  # MI355X: worst |err| / bound 0.12
    _fp32_close(f"{name} fin eval ms", ms.cpu(), ref[1], ref32[1], wrong[1])  # MI355X: worst |err| / bound 0.12


# ---------------------------------------------------------------------------------------------
# weight flips
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cout,cin,R,S", [(24, 8, 3, 3), (72, 136, 3, 3), (16, 16, 1, 3), (16, 16, 3, 1), (64, 8, 5, 5), (8, 8, 1, 1)])
def test_weight_flip_is_the_permutation(lib, cout, cin, R, S):
    w = torch.arange(P * cout * R * S * cin, dtype=F64).reshape(P, cout, R, S, cin) % 251 - 125  # bf16 holds |v| <= 256
    src = _dev(w)
    dst = _out(w[0].numel())
    assert lib.conv_wt_flip_launch(src.data_ptr(), src.shape[1], dst.data_ptr(), dst.shape[1], cout, cin, R, S, P, _stream()) == 0
    _exact("flip", dst, C.wt_flip(w))
    for pad in (0, 1, 2):
        dst = _out(w[0].numel())
        assert lib.conv_wt_flip_parity_launch(src.data_ptr(), src.shape[1], dst.data_ptr(), dst.shape[1], cout, cin, R, S, pad, P, _stream()) == 0
        _exact(f"parity flip pad {pad}", dst, torch.stack([C.wt_flip_parity(w[p], pad) for p in range(P)]))


# ---------------------------------------------------------------------------------------------
# dgrad
# ---------------------------------------------------------------------------------------------
def _dgrad_args(lib, k, mode):
    """mode 1: the dgrad kernels on the Wf shadow; 4 / 5: forward-shaped over dY with the flip
    launchers' weights (what the engine runs at stride 1 / stride 2)."""
    d, dv = k["d"], k["dev"]
    b = _args()
    b.src, b.src_ps, b.src_h, b.src_w, b.src_c = dv["dy"].data_ptr(), dv["dy"].shape[1], d["Ho"], d["Wo"], d["cpo"]
    b.out_h, b.out_w, b.R, b.S, b.stride, b.pad = d["H"], d["W"], d["R"], d["S"], d["stride"], d["pad"]
    wt = dv["w"]
    if mode != 1:
        wt = _out(d["w"][0].numel())
        flip = lib.conv_wt_flip_launch if mode == 4 else lib.conv_wt_flip_parity_launch
        extra = () if mode == 4 else (d["pad"],)
        assert flip(dv["w"].data_ptr(), dv["w"].shape[1], wt.data_ptr(), wt.shape[1], d["cpo"], d["cpi"], d["R"], d["S"], *extra, P, _stream()) == 0
        if mode == 4:
            b.pad = d["R"] - 1 - d["pad"]
    b.wt, b.wt_ps, b.ncol, b.ncol_valid = wt.data_ptr(), wt.shape[1], d["cpi"], d["cin"]
    b.bias, b.bias_ps, b.resid, b.resid_ps = _ptr(dv["bias"]), _ps(dv["bias"]), _ptr(dv["resid"]), _ps(dv["resid"])
    b.nbatch, b.max_batch = k["nbd"].data_ptr(), d["n"]
    out = _out(d["n"] * d["H"] * d["W"] * d["cpi"])
    b.out, b.out_ps = out.data_ptr(), out.shape[1]
    parts, nr = [], lib.conv_bnb_rows()
    if d["y0"] is not None:
        parts = [_out(nr * 2 * d["cpi"], F32, MARK, 0.0) for _ in range(2 if d["y1"] is not None else 1)]
        b.bnb_rows, b.bnb_part_ps = nr, parts[0].shape[1]
        b.bnb_mask, b.bnb_mask_ps = _ptr(dv["mask"]), _ps(dv["mask"])
        b.bnb_mask_ss, b.bnb_mask_ss_ps = _ptr(dv["mask_ss"]), _ps(dv["mask_ss"])
        b.bnb_y0, b.bnb_y0_ps, b.bnb_ms0, b.bnb_part0 = dv["y0"].data_ptr(), dv["y0"].shape[1], dv["ms0"].data_ptr(), parts[0].data_ptr()
        if d["y1"] is not None:
            b.bnb_y1, b.bnb_y1_ps, b.bnb_ms1, b.bnb_part1 = dv["y1"].data_ptr(), dv["y1"].shape[1], dv["ms1"].data_ptr(), parts[1].data_ptr()
    return b, out, parts, nr, wt


def _dgrad_mode(d, shaped):
    return 1 if not shaped else (4 if d["stride"] == 1 else 5)


def _dgrad_rejected(lib, k, mode, variant):
    """Mode 5 exists on the LDS-DMA kernel only, and mode 4's single pad cannot express a non-square
    filter (R-1-pad != S-1-pad): the launcher returns 1 and nothing is written."""
    d = k["d"]
    if not ((mode == 5 and VARIANTS[variant][0] == 0) or (mode == 4 and d["R"] != d["S"])):
        return False
    b, out, parts, nr, _ = _dgrad_args(lib, k, mode)
    assert lib.conv_gemm_launch(mode, ctypes.byref(b), P, _stream()) == 1
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and all(bool((p_[:, : nr * 2 * d["cpi"]] == 0).all()) for p_ in parts)
    return True


def _check_bnb(name, k, parts, nr):
    """[sum g | sum g * xhat_i] per BatchNorm; returns the exact part as the oracle lays it out."""
    d, ref = k["d"], k["ref"][2]
    got = [_rows(p_, nr, 2, d["cpi"]) for p_ in parts]
    for i, g in enumerate(got):
        _equal(f"{name} sum g (BN {i})", g[:, 0], ref[:, 0])
        if k["xh_exact"]:  # every ternary case, and the eighths cases whose terms stay below 2^24 units
            _equal(f"{name} sum g xhat{i}", g[:, 1], ref[:, 1 + i])
        else:
            for p in range(2):  # MI355X: worst |err| / bound 0.00 (the sums come out exact)
                _fp32_close(f"{name} sum g xhat{i} peer {p}", g[p, 1], ref[p, 1 + i], k["ref32"][2][p, 1 + i], k["wrong"][2][p, 1 + i])
            assert float(g[2].abs().max()) == 0.0
    if not k["xh_exact"]:
        return got[0][:, :1]
    full = torch.zeros_like(ref)
    full[:, 0] = got[0][:, 0]
    for i, g in enumerate(got):
        full[:, 1 + i] = g[:, 1]
    return full


@pytest.mark.parametrize("family", C.FAMILIES)
@pytest.mark.parametrize("shaped", [False, True], ids=["dgrad", "as_forward"])
@pytest.mark.parametrize("name", list(C.DGRAD))
def test_dgrad_exact(lib, variant, name, shaped, family):
    k = _prep("dgrad", name, family)
    d = k["d"]
    mode = _dgrad_mode(d, shaped)
    if _dgrad_rejected(lib, k, mode, variant):
        return
    b, out, parts, nr, _ = _dgrad_args(lib, k, mode)
    assert lib.conv_gemm_launch(mode, ctypes.byref(b), P, _stream()) == 0
    seen = (_exact(f"{name} mode {mode}", out, k["ref"][0]),)
    if parts:
        seen += (_check_bnb(f"{name} mode {mode}", k, parts, nr),)
    for label, ctl in k["ctl"].items():
        want = ctl if len(seen) == 1 or seen[1].shape[1] == 3 else (ctl[0], ctl[1][:, :1])
        assert C.differs(seen, want), f"{name}: the {label} control equals the kernel's output"


@pytest.mark.parametrize("shaped", [False, True], ids=["dgrad", "as_forward"])
@pytest.mark.parametrize("name", ["k72_5x7", "s2_9x6_c64_rm1", "s1_5x7_c136_rm1", "halo_8x32_rm1"])
def test_dgrad_randn(lib, variant, name, shaped):
    k = _prep("dgrad", name, "randn")
    d = k["d"]
    mode = _dgrad_mode(d, shaped)
    if _dgrad_rejected(lib, k, mode, variant):
        return
    b, out, _, _, _ = _dgrad_args(lib, k, mode)
    assert lib.conv_gemm_launch(mode, ctypes.byref(b), P, _stream()) == 0
    big = C.dgrad_oracle(d, dy=d["dy"].abs(), w=d["w"].abs(), resid=None if d["resid"] is None else d["resid"].abs(), mask=None, y0=None, y1=None)[1]
    w0 = d["w"].clone()
    w0[:, 0, 0, 0, :] = 0  # one tap of one output channel missing
    _bf16_close(f"{name} mode {mode}", out, k["ref"][0], big, C.dgrad_oracle(d, w=w0)[0])  # MI355X: worst |err| / bound 1.00 (one bf16 ulp)


@pytest.mark.parametrize("shaped", [False, True], ids=["dgrad", "as_forward"])
@pytest.mark.parametrize("name", ["k72_5x7_m1", "s2_9x6_c64_rm1", "s1_5x7_c136_rm1", "halo_8x32_rs2"])
def test_dgrad_finalize_tail(lib, variant, name, shaped):
    """The BN-backward finalize in the dgrad's last workgroup: dgamma / dbeta are added to, the apply
    coefficients stored, rows and counters re-armed."""
    k = _prep("dgrad", name, "ternary")
    d = k["d"]
    mode = _dgrad_mode(d, shaped)
    if _dgrad_rejected(lib, k, mode, variant):
        return
    g = C.gen(6)
    cin, cpi, hw = d["cin"], d["cpi"], d["H"] * d["W"]
    b, out, parts, nr, _ = _dgrad_args(lib, k, mode)
    cnt = torch.zeros(P * lib.conv_fin_words(), dtype=torch.int32, device="cuda")
    b.fin_cnt = cnt.data_ptr()
    gammas, dgs, dbs, coefs = [], [], [], []
    for i in range(len(parts)):
        gammas.append((torch.rand(P, cin, generator=g) + 0.5).double())  # fp32 values
        gm = _dev(gammas[i], F32, gap=3)
        dgs.append(_out(cin, F32, MARK, 0.25, gap=3))
        dbs.append(_out(cin, F32, MARK, 0.25, gap=3))
        coefs.append(torch.full((P, 3, cpi), NAN, dtype=F32, device="cuda"))
        b.fin_param_ps = gm.shape[1]
        setattr(b, f"fin_gamma{i}", gm.data_ptr())
        setattr(b, f"fin_dgamma{i}", dgs[i].data_ptr())
        setattr(b, f"fin_dbeta{i}", dbs[i].data_ptr())
        setattr(b, f"fin_coef{i}", coefs[i].data_ptr())
        setattr(b, f"fin_C{i}", cin)
        gammas[i] = (gammas[i], gm)  # keep the device copy alive
    assert lib.conv_gemm_launch(mode, ctypes.byref(b), P, _stream()) == 0
    _exact(f"{name} mode {mode}", out, k["ref"][0])
    assert all(float(_rows(p_, nr, 2, cpi).abs().max()) == 0.0 for p_ in parts), "the accumulator rows are not re-armed"
    assert int(cnt.abs().max()) == 0, "the arrival counters are not re-armed"
    sums = k["ref"][2]
    for i in range(len(parts)):
        s2 = torch.stack([sums[:, 0], sums[:, 1 + i]], 1)  # exact in this family
        ms = d[f"ms{i}"]
        args = (d["nb"], hw, gammas[i][0], ms, cin, cpi)
        ref, ref32, wrong = C.fin_bwd(s2, *args), C.fin_bwd(s2, *args, dtype=F32), C.fin_bwd(s2, *args, count=lambda n: max(1, n) + 1)
        dg, db = dgs[i].cpu(), dbs[i].cpu()
        assert (dg[:, cin:] == MARK).all() and (db[:, cin:] == MARK).all()
        _equal(f"{name} dgamma{i}", dg[:, :cin], 0.25 + ref[0])  # sums of eighths: the += is exact
        _equal(f"{name} dbeta{i}", db[:, :cin], 0.25 + ref[1])
        # MI355X: worst |err| / bound 0.16
        _fp32_close(f"{name} fin coef{i}", coefs[i].cpu(), ref[2], ref32[2], wrong[2])


# ---------------------------------------------------------------------------------------------
# wgrad
# ---------------------------------------------------------------------------------------------
def _wgrad_launch(lib, k, want_splits, expect=0):
    """``want_splits`` 1: one split, plain stores into a slab full of MARK; > 1: split-K atomics into
    a slab that holds BASE. Returns the gradient buffer and its expected content."""
    d, dv = k["d"], k["dev"]
    M = d["n"] * d["Ho"] * d["Wo"]
    k_per = max(64, ((M + want_splits - 1) // want_splits + 63) // 64 * 64)
    splits = (M + k_per - 1) // k_per
    acc = int(want_splits > 1)
    n = d["cpo"] * d["R"] * d["S"] * d["cpi"]
    grad = _out(n, F32, MARK, C.BASE if acc else MARK)
    c = _wargs()
    c.dy, c.dy_ps, c.x, c.x_ps = dv["dy"].data_ptr(), dv["dy"].shape[1], dv["x"].data_ptr(), dv["x"].shape[1]
    c.H, c.W, c.x_c, c.Ho, c.Wo, c.dy_c = d["H"], d["W"], d["cpi"], d["Ho"], d["Wo"], d["cpo"]
    c.R, c.S, c.stride, c.pad = d["R"], d["S"], d["stride"], d["pad"]
    c.grad, c.grad_ps, c.accumulate, c.k_per_split = grad.data_ptr(), grad.shape[1], acc, k_per
    c.nbatch, c.max_batch = k["nbd"].data_ptr(), d["n"]
    c.pro_ss, c.pro_ss_ps = _ptr(dv["pro_ss"]), _ps(dv["pro_ss"])
    assert lib.conv_wgrad_launch(ctypes.byref(c), P, splits, _stream()) == expect
    return grad, acc


def _wgrad_expect(ref, acc):
    """accumulate: BASE + dW everywhere (a peer without rows adds nothing). Store: dW, and the slab
    of a peer without rows keeps what it held — k_conv_wgrad* return before the store when a split
    has no rows. The engine never consumes that slab: cnn_opt_step skips a peer with nb = 0 (it
    neither updates nor re-zeroes), and every later step with rows stores or re-zeroes first."""
    want = ref + C.BASE if acc else ref.clone()
    if not acc:
        want[2] = NAN
    return want


@pytest.mark.parametrize("family", C.FAMILIES)
@pytest.mark.parametrize("splits", [1, 2, 3])
@pytest.mark.parametrize("name", list(C.WGRAD))
def test_wgrad_exact(lib, wvariant, name, splits, family):
    k = _prep("wgrad", name, family)
    grad, acc = _wgrad_launch(lib, k, splits)
    seen = _exact(name, grad, _wgrad_expect(k["ref"], acc), MARK)
    for label, ctl in k["ctl"].items():
        assert C.differs(seen, _wgrad_expect(ctl[0], acc)), f"{name}: the {label} control equals the kernel's gradient"


@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("name", ["k72_5x7", "k72_5x7_pro", "halo_8x16", "halo_2x32"])
def test_wgrad_randn(lib, wvariant, name, splits):
    """fp32 gradient of bf16 operands: 2^-20 * M (the bf16_bound without the output's bf16 ulp)."""
    k = _prep("wgrad", name, "randn")
    d = k["d"]
    grad, acc = _wgrad_launch(lib, k, splits)
    want = _wgrad_expect(k["ref"], acc)
    got, ok = _read(grad, want, MARK)
    act = d["x"] if d["pro_ss"] is None else C.prologue(d["x"], d["pro_ss"])
    big = C.wgrad_oracle(d, dy=d["dy"].abs(), x=act.abs(), pro_ss=None) + (C.BASE if acc else 0.0)
    bound = 2.0 ** -20 * big + 2.0 ** -126
    ratio = float(((got - want).abs() / bound)[ok].max())
    print(f"wgrad {name}: worst |err| / bound = ratio {ratio:.3f}")  # MI355X: worst |err| / bound 0.12
    assert ratio <= 1.0
    x0 = d["x"].clone()
    x0[:, :, 0, 0, :] = 0  # the first pixel of every sample missing
    wrong = _wgrad_expect(C.wgrad_oracle(d, x=x0), acc)
    assert ((got - wrong).abs() > bound)[ok].any(), "the wrong reference passes too"


# ---------------------------------------------------------------------------------------------
# rejected arguments
# ---------------------------------------------------------------------------------------------
def _set(obj, **kw):
    for key, v in kw.items():
        setattr(obj, key, v)


@pytest.mark.parametrize("what", ["src_c", "ncol", "peers", "mode2", "mode3", "mode7", "mode-1", "mode4_stride2", "mode4_nonsquare", "mode5_stride1", "pro_mode4",
                                  "pro_mode5", "fin_ncol", "offsets"])
def test_conv_gemm_launch_rejects(lib, what):
    k = _prep("fwd", "k144_5x7_c72_pro", "ternary")
    a, out, st, rows = _fwd_args(lib, k)
    mode, peers, want = 0, P, 1
    if what == "src_c":
        a.src_c = 12
    elif what == "ncol":
        a.ncol = 68
    elif what == "peers":
        peers = 0
    elif what.startswith("mode") and "_" not in what:
        mode = int(what[4:])
    elif what == "mode4_stride2":
        _set(a, pro_ss=None, stride=2)
        mode = 4
    elif what == "mode4_nonsquare":  # one pad cannot be both R-1-pad and S-1-pad
        _set(a, pro_ss=None, R=1, pad=0)
        mode = 4
    elif what == "mode5_stride1":
        _set(a, pro_ss=None)
        mode = 5
    elif what == "pro_mode4":
        mode = 4
    elif what == "pro_mode5":
        _set(a, stride=2)
        mode = 5
    elif what == "fin_ncol":  # the finalize tail holds 4 channels per thread of a 256-thread workgroup
        cnt = torch.zeros(P * lib.conv_fin_words(), dtype=torch.int32, device="cuda")
        _set(a, fin_cnt=cnt.data_ptr(), ncol=1032)
    else:  # 32-bit byte offsets of the gathers: one peer's source must stay below 2 GiB
        _set(a, max_batch=2 ** 24)
        want = 3
    assert lib.conv_gemm_launch(mode, ctypes.byref(a), peers, _stream()) == want
    torch.cuda.synchronize()
    assert torch.isnan(out).all(), "a rejected launch wrote its output"
    assert float(_rows(st, rows, 2, k["d"]["cpo"]).abs().max()) == 0.0


@pytest.mark.parametrize("what", ["x_c", "dy_c", "k_per_split", "splits_no_accumulate", "splits0", "peers", "offsets"])
def test_conv_wgrad_launch_rejects(lib, what):
    k = _prep("wgrad", "k72_5x7", "ternary")
    d, dv = k["d"], k["dev"]
    grad = _out(d["cpo"] * 9 * d["cpi"], F32, MARK)
    c = _wargs()
    c.dy, c.dy_ps, c.x, c.x_ps = dv["dy"].data_ptr(), dv["dy"].shape[1], dv["x"].data_ptr(), dv["x"].shape[1]
    c.H, c.W, c.x_c, c.Ho, c.Wo, c.dy_c = d["H"], d["W"], d["cpi"], d["Ho"], d["Wo"], d["cpo"]
    c.R, c.S, c.stride, c.pad = 3, 3, 1, 1
    c.grad, c.grad_ps, c.accumulate, c.k_per_split = grad.data_ptr(), grad.shape[1], 1, 64
    c.nbatch, c.max_batch = k["nbd"].data_ptr(), d["n"]
    peers, splits, want = P, 3, 1
    if what == "x_c":
        c.x_c = 12
    elif what == "dy_c":
        c.dy_c = 20
    elif what == "k_per_split":
        c.k_per_split = 96
    elif what == "splits_no_accumulate":
        c.accumulate = 0
    elif what == "splits0":
        splits = 0
    elif what == "peers":
        peers = 0
    else:
        c.max_batch, want = 2 ** 24, 3
    assert lib.conv_wgrad_launch(ctypes.byref(c), peers, splits, _stream()) == want
    torch.cuda.synchronize()
    assert (grad == MARK).all(), "a rejected launch wrote its gradient"
