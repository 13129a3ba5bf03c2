"""The FedAvg, mixing, median, SCAFFOLD, optimizer and noise kernels of ``csrc/kernels/fl_ops.hip``
against the float64 references of ``tests/_fl_ops_ref.py`` (MI355X only).

Bounds. ``u = 2^-24``; a chain of r fp32 roundings is within ``γ_r = r·u / (1 − r·u)`` of the
magnitude the reference returns (the sum of the absolute values of an output's terms). Every count
below is of the longest path of one output and assumes no fused multiply-add; a contracted
``a·b + c`` has one rounding instead of two, so the bounds hold either way. Nothing is measured.

* Weighted sums over the nz rows of weight != 0 (``k_weighted_sum``, ``k_stacked_weighted_sum``,
  ``k_fedavg_reduce``, ``k_neighbor_mix`` with nz the sources of a row): the first product is added
  to 0 exactly, so the first term sees its product and nz − 1 sums: ``γ_nz · Σ|w_p x_p|``; the
  scale of ``k_stacked_weighted_sum`` is one more: ``γ_(nz+1)``.
* ``k_fedavg_apply``: ``inv = 1 / max(wsum, 1e-12)`` and the product, on the sums the kernel was
  given: ``γ_2 · |out / wsum|``. ``k_fedavg_local`` is both in one thread: ``γ_(nz+2) · Σ|w_p x_p| / wsum``.
  Two evaluations of that expression in the same order (local, and reduce + apply) are compared
  with the same bound.
* ``k_fedavg_delayed_land``: inv, ``avg·inv``, the difference with the snapshot and the sum with
  the row, each on a quantity no larger than ``|row| + |avg/wsum| + |snap|``: ``γ_4`` of it.
* ``k_coordinate_median``: min and max are exact, so odd K returns an input bit for bit; even K
  rounds ``a + b`` once (``0.5·`` is exact): ``γ_1 · |median|``.
* ``k_scaffold_reduce``: K fused multiply-adds, ``γ_K · Σ|w_k dy_k|``; K − 1 sums for ``Σ dc_k`` and
  ``Σ w_k`` (``γ_K`` is used). ``k_scaffold_apply``: ``glr / max(Σw, 1e-12)`` and one fma:
  ``γ_2 · (|x_start| + |step|)``; ``1 / K``, the product and the sum: ``γ_3 · (|c| + |Σdc / K|)``.
* ``k_opt_step``: the reference returns *units* (roundings × magnitude summed over the quantities
  they act on, derived in ``_fl_ops_ref.adam_step`` / ``sgd_step``); no path has more than 32
  roundings, so the bound is ``units · u / (1 − 32u)``. The bias corrections count one rounding each:
  they are formed in double and rounded once. One step from a random non-zero ``(w, m, v)`` with
  ``|update| ≳ |w|``, so that an error in the update is not hidden behind the rounding of ``w``.
* Exact, compared as ``int32`` bits: broadcast, the snapshot of delayed land, mixing with a
  permutation matrix (weights 1.0: ``0 + 1·x``; no −0.0 among the inputs), the median for odd K
  (the reference orders −0.0 below +0.0 as ``v_min_f32`` / ``v_max_f32`` do), ``scale·t`` for
  scale −1 and 0.5, and every row, padding column and guard cell a kernel must not touch (they
  hold a NaN with a payload).
* Noise (``k_scale_add_noise``, σ > 0, from zeros, N = 2^20): ``|z|/σ <= sqrt(2·24·ln 2)·(1 + 1e-3)``,
  the largest Box-Muller radius of a uniform on a 24-bit grid with the fast intrinsics' error;
  ``|mean| <= 5σ/√N``; ``|var/σ² − 1| <= 5·√(2/N)``; Kolmogorov-Smirnov distance to the normal CDF
  ``<= 1.95/√N``; lag-1 autocorrelation, the correlation between seeds 3 and 4 and between the two
  halves each ``<= 5/√N``. The seeds are fixed, so a pass is a pass for good; float64 normal samples
  of the same size from ``numpy.random.default_rng(3)`` and ``(4)`` meet every one of these
  thresholds (``tests/test_fl_ops_ref_cpu.py::test_noise_statistics_on_numpy_normals``).

Sizes: n in {1, 3, 4, 5, 1027} and one size per kernel just past where its grid-stride loop runs
twice with a tail for the float4 kernels; {1, 7, 1001, 524291} for the scalar kernels. Layouts of a
stacked buffer: ``ld == n``; ``ld`` the next multiple of 4; that plus 1; and a multiple of 4 with
the base advanced by one float (4-byte aligned only: the scalar path has to be taken).
"""

import ctypes

import numpy as np
import pytest
import torch

import _fl_ops_ref as R

pytestmark = pytest.mark.gpu

F4_NS = (1, 3, 4, 5, 1027)
WRAP = 4 * 2048 * 256 + 7  # grid capped at 2048 blocks of 256 float4 lanes
WRAP_APPLY = 4 * 256 * 256 + 7  # fedavg_apply / broadcast_rows: capped at 256 blocks
WRAP_LAND = 512 * 256 + 3  # delayed_land: 512 blocks of scalar lanes
SCALAR_NS = (1, 7, 1001, 524291)
LAYOUTS = ("packed", "pad4", "pad4p1", "shift")
SENTINEL = 0x7FC12345  # a quiet NaN with a payload


@pytest.fixture(scope="module")
def dev():
    from myfyp_amd.ops import _native

    _native.load(required=True)  # the native path must be the one under test
    return torch.device("cuda")


def _lib():
    from myfyp_amd import ops

    return ops.fast_lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _rng(seed):
    return np.random.default_rng(seed)


def _f32(rng, *shape):
    return rng.standard_normal(shape).astype(np.float32)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _sentinel(count, dev):
    return torch.full((count,), SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(t):
    return t.detach().cpu().numpy()


def _within(got, want, mag, r, what, units=False):
    """|got − want| <= γ_r·mag per coordinate (units: mag·u/(1 − 32u)); prints the worst case."""
    g = _np(got).astype(np.float64).reshape(-1)
    want, mag = np.asarray(want, dtype=np.float64).reshape(-1), np.asarray(mag, dtype=np.float64).reshape(-1)
    assert g.shape == want.shape == mag.shape, (what, g.shape, want.shape, mag.shape)
    assert np.all(np.isfinite(g)), f"{what}: non-finite output"
    err = np.abs(g - want)
    bound = mag * (R.U / (1.0 - 32 * R.U) if units else R.gamma(r))
    i = int(np.argmax(err - bound))
    print(f"{what}: max err {err.max():.3e}; worst coordinate {i}: err {err[i]:.3e} (bound {bound[i]:.3e})")
    assert np.all(err <= bound), (what, i, err[i], bound[i])


class Flat:
    """n floats at ``off`` floats past a 16-byte-aligned base, sentinels before and behind."""

    def __init__(self, dev, n, off=0, data=None):
        self.flat = _sentinel(off + n + 5, dev)
        self.off, self.n = off, n
        self.v = self.flat[off : off + n]
        if data is not None:
            self.v.copy_(_dev(data, dev))
        self.orig = self.flat.clone()
        assert self.flat.data_ptr() % 16 == 0 and self.v.data_ptr() % 16 == (4 * off) % 16

    @property
    def ptr(self):
        return self.v.data_ptr()

    def guards_ok(self, written=True):
        keep = torch.ones_like(self.flat, dtype=torch.bool)
        if written:
            keep[self.off : self.off + self.n] = False
        return torch.equal(_bits(self.flat)[keep], _bits(self.orig)[keep])


class Stacked:
    """``x`` [P, n] in a [P + 1, ld] buffer: padding columns, a guard row and the floats around it
    hold the sentinel. ``shift``: the base is 4 bytes past a 16-byte boundary."""

    def __init__(self, dev, x, layout, ld=None):
        self.P, self.n = x.shape
        n4 = (self.n + 3) // 4 * 4
        self.ld = ld if ld is not None else {"packed": self.n, "pad4": n4, "pad4p1": n4 + 1, "shift": n4}[layout]
        self.off = 1 if layout == "shift" else 0
        self.flat = _sentinel(self.off + (self.P + 1) * self.ld + 3, dev)
        self.view = self.flat[self.off : self.off + (self.P + 1) * self.ld].view(self.P + 1, self.ld)
        self.view[: self.P, : self.n] = _dev(x, dev)
        self.orig = self.flat.clone()
        assert self.ptr % 16 == 4 * self.off

    @property
    def ptr(self):
        return self.view.data_ptr()

    @property
    def rows(self):
        return self.view[: self.P, : self.n]

    def untouched_ok(self, written=(), ncols=None):
        """Everything but the first ``ncols`` (default n) columns of the ``written`` rows is as it was."""
        keep = torch.ones_like(self.flat, dtype=torch.bool)
        kv = keep[self.off : self.off + (self.P + 1) * self.ld].view(self.P + 1, self.ld)
        for p in written:
            kv[p, : self.n if ncols is None else ncols] = False
        return torch.equal(_bits(self.flat)[keep], _bits(self.orig)[keep])


def _weights_case(rng, p, n, poison=True):
    """[P, n] rows and weights with zeros; the rows of weight 0 hold NaN and Inf."""
    x = _f32(rng, p, n)
    w = (rng.integers(1, 6, size=p)).astype(np.float32)
    if p >= 3:
        w[1] = 0.0
    if p >= 6:
        w[p - 3] = 0.0
    if poison:
        for j, r in enumerate(np.flatnonzero(w == 0)):
            x[r] = np.nan if j % 2 == 0 else np.inf
    return x, w


def _sizes(wrap):
    return [(n, 5) for n in F4_NS] + [(wrap, 3)]


# --------------------------------------------------------------------------------------------
# weighted sums
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_stacked_weighted_sum(dev, layout):
    from myfyp_amd import ops

    for n, p in _sizes(WRAP):
        x, w = _weights_case(_rng(n), p, n)
        st = Stacked(dev, x, layout)
        out = Flat(dev, n, off=st.off)
        ops.stacked_weighted_sum(st.rows, _dev(w, dev), out.v, scale=0.25)
        want, mag = R.stacked_weighted_sum(x, w, 0.25)
        _within(out.v, want, mag, R.nonzero(w) + 1, f"stacked_weighted_sum {layout} n={n} P={p}")
        assert out.guards_ok() and st.untouched_ok()
    # one row; and all weights zero: nothing is read, the sums are 0
    x = _f32(_rng(0), 1, 1027)
    st, out = Stacked(dev, x, layout), Flat(dev, 1027)
    ops.stacked_weighted_sum(st.rows, _dev(np.float32([3.0]), dev), out.v, scale=-0.5)
    want, mag = R.stacked_weighted_sum(x, np.float32([3.0]), -0.5)
    _within(out.v, want, mag, 2, f"stacked_weighted_sum {layout} P=1")
    x = np.full((4, 1027), np.nan, dtype=np.float32)
    st = Stacked(dev, x, layout)
    ops.stacked_weighted_sum(st.rows, torch.zeros(4, device=dev), out.v, scale=2.0)
    assert not bool(out.v.any()) and out.guards_ok() and st.untouched_ok()


def _layer_views(dev, x, off):
    """Rows as views ``off`` floats into flat buffers: layers at an odd offset of a flat model."""
    bufs = [Flat(dev, x.shape[1], off=off, data=x[k]) for k in range(x.shape[0])]
    return bufs, [[b.v] for b in bufs]


@pytest.mark.parametrize("off", [0, 1, 2])
def test_weighted_average(dev, off):
    from myfyp_amd import ops

    for n, k in _sizes(WRAP):
        x, w = _weights_case(_rng(100 + n), k, n)
        bufs, models = _layer_views(dev, x, off)
        got = ops.weighted_average(models, [float(v) for v in w])[0]
        want, mag = R.weighted_sum(list(x), w)
        _within(got, want, mag, R.nonzero(w), f"weighted_average off={off} n={n} K={k}")
        assert all(b.guards_ok(written=False) for b in bufs)


def test_weighted_sum_misaligned_output(dev):
    """The entry point itself: rows aligned (the caller says so), the output 4-byte aligned only."""
    lib = _lib()
    for n in (5, 1027):
        x, w = _weights_case(_rng(n), 5, n)
        rows = [Flat(dev, n, data=x[k]) for k in range(5)]
        ptrs = torch.tensor([r.ptr for r in rows], dtype=torch.int64, device=dev)
        wd = _dev(w, dev)
        want, mag = R.weighted_sum(list(x), w)
        for off in (0, 1, 3):
            out = Flat(dev, n, off=off)
            assert lib.myfyp_weighted_sum(out.ptr, ptrs.data_ptr(), wd.data_ptr(), 5, n, 1, _stream()) == 0
            _within(out.v, want, mag, R.nonzero(w), f"weighted_sum out off={off} n={n}")
            assert out.guards_ok()


# --------------------------------------------------------------------------------------------
# broadcast
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_broadcast_rows(dev, layout):
    from myfyp_amd import ops

    for n, p in [(n, 4) for n in F4_NS] + [(WRAP_APPLY, 3)]:
        rng = _rng(n)
        x, s = _f32(rng, p, n), _f32(rng, n)
        s[0] = -0.0
        sb = s.view(np.int32)
        sb[-1] = 0x7FC00055  # a NaN payload travels too
        for mask in (None, np.float32([1, 0, 1, 1][:p])):
            st = Stacked(dev, x, layout)
            src = Flat(dev, n, off=st.off, data=s)
            ops.broadcast_rows(src.v, st.rows, None if mask is None else _dev(mask, dev))
            written = [r for r in range(p) if mask is None or mask[r] != 0]
            for r in written:
                assert _same_bits(st.view[r, :n], src.v), (layout, n, r)
            assert st.untouched_ok(written) and src.guards_ok(written=False)
            want = R.broadcast(x, s, mask).astype(np.float32)
            assert np.array_equal(_np(st.rows).view(np.int32), want.view(np.int32))
        print(f"broadcast_rows {layout} n={n} P={p}: bit exact")


# --------------------------------------------------------------------------------------------
# FedAvg reduce / apply / local
# --------------------------------------------------------------------------------------------
def _host(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a, a.ctypes.data


def _fedavg_case(n, p, seed):
    x, w = _weights_case(_rng(seed), p, n)
    mask = np.ones(p, dtype=np.float32)
    mask[p - 1] = 0.0
    if p > 3:
        mask[3] = 0.0
    return x, w, mask


@pytest.mark.parametrize("layout", LAYOUTS)
def test_fedavg_reduce_apply_local(dev, layout):
    lib = _lib()
    for n, p in [(n, 8) for n in F4_NS] + [(WRAP_APPLY, 3), (WRAP, 3)]:
        x, w, mask = _fedavg_case(n, p, seed=n)
        wk, wp = _host(w)
        mk, mp = _host(mask)
        nz = R.nonzero(w)
        tag = f"{layout} n={n} P={p}"
        # reduce into [out | wsum]
        st = Stacked(dev, x, layout)
        buf = Flat(dev, n + 1, off=st.off)
        assert lib.myfyp_fedavg_stacked_reduce(buf.ptr, st.ptr, p, n, st.ld, wp, _stream()) == 0
        want, mag, wsum = R.fedavg_reduce(x, w)
        _within(buf.v[:n], want, mag, nz, f"fedavg_reduce {tag}")
        assert float(buf.v[n]) == wsum and buf.guards_ok() and st.untouched_ok()
        # apply on the sums the kernel made
        sums = buf.flat.clone()
        assert lib.myfyp_fedavg_stacked_apply(st.ptr, buf.ptr, p, n, st.ld, mp, _stream()) == 0
        rows, amag = R.fedavg_apply(x, _np(buf.v[:n]), wsum, mask)
        written = [r for r in range(p) if mask[r] != 0]
        for r in written:
            _within(st.view[r, :n], rows[r, :n], amag, 2, f"fedavg_apply {tag} row {r}")
            assert _same_bits(st.view[r, :n], st.view[written[0], :n])
        assert st.untouched_ok(written) and _same_bits(buf.flat, sums)
        # local: one launch
        lo = Stacked(dev, x, layout)
        assert lib.myfyp_fedavg_stacked_local(lo.ptr, p, n, lo.ld, wp, mp, _stream()) == 0
        lrows, lmag = R.fedavg_local(x, w, mask, n)
        for r in written:
            _within(lo.view[r, :n], lrows[r, :n], lmag, nz + 2, f"fedavg_local {tag} row {r}")
        _within(lo.view[written[0], :n], _np(st.view[written[0], :n]).astype(np.float64), lmag, nz + 2, f"fedavg_local vs reduce+apply {tag}")
        assert lo.untouched_ok(written)


def test_fedavg_edges(dev):
    lib = _lib()
    n = 1027
    # all weights zero: sums 0, weight sum 0, apply divides by 1e-12
    x = np.full((4, n), np.nan, dtype=np.float32)
    st, buf = Stacked(dev, x, "pad4"), Flat(dev, n + 1)
    zk, zp = _host(np.zeros(4))
    mk, mp = _host([1, 0, 1, 1])
    assert lib.myfyp_fedavg_stacked_reduce(buf.ptr, st.ptr, 4, n, st.ld, zp, _stream()) == 0
    assert not bool(buf.v.any()) and st.untouched_ok()
    assert lib.myfyp_fedavg_stacked_apply(st.ptr, buf.ptr, 4, n, st.ld, mp, _stream()) == 0
    rows, _ = R.fedavg_apply(x, np.zeros(n), 0.0, mk)
    assert not bool(st.view[0, :n].any()) and not rows[0, :n].any() and st.untouched_ok([0, 2, 3])
    sums = _f32(_rng(5), n) * np.float32(1e-12)
    buf = Flat(dev, n + 1, data=np.append(sums, np.float32(0.0)))
    assert lib.myfyp_fedavg_stacked_apply(st.ptr, buf.ptr, 4, n, st.ld, mp, _stream()) == 0
    rows, amag = R.fedavg_apply(x, sums, 0.0, mk)
    _within(st.view[2, :n], rows[2, :n], amag, 2, "fedavg_apply at wsum 0 (divides by 1e-12)")
    lo = Stacked(dev, x, "pad4")
    assert lib.myfyp_fedavg_stacked_local(lo.ptr, 4, n, lo.ld, zp, mp, _stream()) == 0
    assert not bool(lo.view[0, :n].any()) and lo.untouched_ok([0, 2, 3])
    # P = 1, and P = 64 with only mask bits 0 and 63 set
    for p in (1, 64):
        x = _f32(_rng(p), p, n)
        w = np.linspace(1, 2, p).astype(np.float32)
        mask = np.zeros(p, dtype=np.float32)
        mask[0] = mask[p - 1] = 1.0
        wk, wp = _host(w)
        mk, mp = _host(mask)
        lo = Stacked(dev, x, "pad4p1")
        assert lib.myfyp_fedavg_stacked_local(lo.ptr, p, n, lo.ld, wp, mp, _stream()) == 0
        rows, lmag = R.fedavg_local(x, w, mask, n)
        for r in {0, p - 1}:
            _within(lo.view[r, :n], rows[r, :n], lmag, p + 2, f"fedavg_local P={p} row {r}")
        assert lo.untouched_ok({0, p - 1})
        st, buf = Stacked(dev, x, "pad4"), Flat(dev, n + 1)
        assert lib.myfyp_fedavg_stacked_reduce(buf.ptr, st.ptr, p, n, st.ld, wp, _stream()) == 0
        want, mag, wsum = R.fedavg_reduce(x, w)
        _within(buf.v[:n], want, mag, p, f"fedavg_reduce P={p}")
        assert float(buf.v[n]) == wsum
        assert lib.myfyp_fedavg_stacked_apply(st.ptr, buf.ptr, p, n, st.ld, mp, _stream()) == 0
        rows, amag = R.fedavg_apply(x, _np(buf.v[:n]), wsum, mask)
        for r in {0, p - 1}:
            _within(st.view[r, :n], rows[r, :n], amag, 2, f"fedavg_apply P={p} row {r}")
        assert st.untouched_ok({0, p - 1})
    # P = 0 and P = 65: status 2, nothing written
    x = _f32(_rng(9), 2, n)
    wk, wp = _host(np.ones(65))
    for p in (0, 65):
        st, sn, buf, b2 = Stacked(dev, x, "pad4"), Stacked(dev, x, "pad4"), Flat(dev, n + 1), Flat(dev, n + 1)
        s = _stream()
        assert lib.myfyp_fedavg_stacked_reduce(buf.ptr, st.ptr, p, n, st.ld, wp, s) == 2
        assert lib.myfyp_fedavg_bucket_reduce(buf.ptr, buf.ptr + 4 * n, st.ptr, p, n, st.ld, wp, s) == 2
        assert lib.myfyp_fedavg_bucket_reduce2(buf.ptr, buf.ptr + 4 * n, b2.ptr, b2.ptr + 4 * n, st.ptr, p, n, st.ld, wp, s) == 2
        assert lib.myfyp_fedavg_stacked_apply(st.ptr, buf.ptr, p, n, st.ld, wp, s) == 2
        assert lib.myfyp_fedavg_stacked_local(st.ptr, p, n, st.ld, wp, wp, s) == 2
        assert lib.myfyp_fedavg_delayed_land(st.ptr, sn.ptr, sn.ld, buf.ptr, buf.ptr + 4 * n, p, n, st.ld, wp, s) == 2
        assert st.untouched_ok() and sn.untouched_ok() and buf.guards_ok(written=False) and b2.guards_ok(written=False)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_fedavg_reduce2_and_null_slot(dev, layout):
    lib = _lib()
    for n in (3, 5, 1027):
        x, w, _ = _fedavg_case(n, 8, seed=50 + n)
        wk, wp = _host(w)
        st = Stacked(dev, x, layout)
        want, mag, wsum = R.fedavg_reduce(x, w)
        # [wsum, pad x3 | data]; the copy lies at another alignment than the first output
        a, b = Flat(dev, 4 + n), Flat(dev, 4 + n, off=st.off)
        assert lib.myfyp_fedavg_bucket_reduce2(a.ptr + 16, a.ptr, b.ptr + 16, b.ptr, st.ptr, 8, n, st.ld, wp, _stream()) == 0
        _within(a.v[4:], want, mag, R.nonzero(w), f"fedavg_reduce2 {layout} n={n}")
        assert _same_bits(a.v[4:], b.v[4:]) and float(a.v[0]) == wsum and _same_bits(a.v[:1], b.v[:1])
        pad = _sentinel(3, dev)
        assert _same_bits(a.v[1:4], pad) and _same_bits(b.v[1:4], pad) and a.guards_ok() and b.guards_ok() and st.untouched_ok()
        # null slots: only the sums are written
        c, d = Flat(dev, 4 + n), Flat(dev, 4 + n)
        assert lib.myfyp_fedavg_bucket_reduce2(c.ptr + 16, None, d.ptr + 16, None, st.ptr, 8, n, st.ld, wp, _stream()) == 0
        assert lib.myfyp_fedavg_bucket_reduce(d.ptr + 16, None, st.ptr, 8, n, st.ld, wp, _stream()) == 0
        pad = _sentinel(4, dev)
        assert _same_bits(c.v[4:], a.v[4:]) and _same_bits(d.v[4:], a.v[4:]) and _same_bits(c.v[:4], pad) and _same_bits(d.v[:4], pad)


def test_fedavg_buckets_match_unbucketed(dev):
    """Two buckets over one row range as the weights plane lays them out ([wsum, pad x3 | data],
    the second bucket with a null slot): reduce + apply per bucket == the unbucketed pair, bit for bit."""
    lib = _lib()
    n, p = 1027, 8
    x, w, mask = _fedavg_case(n, p, seed=77)
    wk, wp = _host(w)
    mk, mp = _host(mask)
    one, buf = Stacked(dev, x, "pad4"), Flat(dev, n + 1)
    assert lib.myfyp_fedavg_stacked_reduce(buf.ptr, one.ptr, p, n, one.ld, wp, _stream()) == 0
    assert lib.myfyp_fedavg_stacked_apply(one.ptr, buf.ptr, p, n, one.ld, mp, _stream()) == 0
    two, bb = Stacked(dev, x, "pad4"), Flat(dev, 4 + n)
    ranges = [(0, 512), (512, n)]
    for k, (b0, b1) in enumerate(ranges):
        assert lib.myfyp_fedavg_bucket_reduce(bb.ptr + 4 * (4 + b0), bb.ptr if k == 0 else None, two.ptr + 4 * b0, p, b1 - b0, two.ld, wp, _stream()) == 0
    assert _same_bits(bb.v[4:], buf.v[:n]) and _same_bits(bb.v[:1], buf.v[n:]) and bb.guards_ok()
    for b0, b1 in ranges:
        assert lib.myfyp_fedavg_bucket_apply(two.ptr + 4 * b0, bb.ptr + 4 * (4 + b0), bb.ptr, p, b1 - b0, two.ld, mp, _stream()) == 0
    assert _same_bits(two.flat, one.flat)
    assert two.untouched_ok([r for r in range(p) if mask[r] != 0])


# --------------------------------------------------------------------------------------------
# delayed land
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 5, 1027, WRAP_LAND])
def test_fedavg_delayed_land(dev, n):
    lib = _lib()
    rng = _rng(n)
    p = 3
    x, sn, avg = _f32(rng, p, n), _f32(rng, p, n), 4.0 * _f32(rng, n)
    mask = np.float32([1, 0, 1])
    mk, mp = _host(mask)
    for off in (0, 1):
        st = Stacked(dev, x, "shift" if off else "pad4", ld=n + 3)
        snap = Stacked(dev, sn, "pad4", ld=n + 1)  # ld_snap != ld
        ab = Flat(dev, 4 + n, data=np.concatenate([np.float32([4.0, 0, 0, 0]), avg]))
        assert lib.myfyp_fedavg_delayed_land(st.ptr, snap.ptr, snap.ld, ab.ptr + 16, ab.ptr, p, n, st.ld, mp, _stream()) == 0
        rows, snaps, mag = R.delayed_land(x, sn, avg, 4.0, mask, n)
        for r in (0, 2):
            _within(st.view[r, :n], rows[r, :n], mag[r], 4, f"delayed_land n={n} off={off} row {r}")
            assert _same_bits(st.view[r, :n], snap.view[r, :n])
        assert st.untouched_ok([0, 2]) and snap.untouched_ok([0, 2]) and ab.guards_ok(written=False)
        # nothing pending: the snapshot only
        st, snap = Stacked(dev, x, "shift" if off else "pad4", ld=n + 3), Stacked(dev, sn, "pad4", ld=n + 1)
        assert lib.myfyp_fedavg_delayed_land(st.ptr, snap.ptr, snap.ld, None, None, p, n, st.ld, mp, _stream()) == 0
        assert st.untouched_ok() and snap.untouched_ok([0, 2])
        for r in (0, 2):
            assert _same_bits(snap.view[r, :n], st.view[r, :n])
    print(f"delayed_land n={n}: snapshot bit exact, unmasked rows and padding untouched")


# --------------------------------------------------------------------------------------------
# neighbour mix
# --------------------------------------------------------------------------------------------
def _mix(lib, st, p, n, m):
    mk, mp = _host(m)
    return lib.myfyp_neighbor_mix_stacked(st.ptr, p, n, st.ld, mp, _stream())


def _check_mix(dev, lib, x, m, n, what, extra_ld=0):
    p = x.shape[0]
    n4 = (n + 3) // 4 * 4
    st = Stacked(dev, x, "pad4", ld=n4 + extra_ld)
    assert _mix(lib, st, p, n, m) == 0
    rows, mag, nsrc = R.neighbor_mix(x, m, n)
    mixed = [r for r in range(p) if nsrc[r]]
    for r in mixed:
        _within(st.view[r, :n], rows[r, :n], mag[r], int(nsrc[r]), f"{what} row {r} ({nsrc[r]} sources)")
    assert st.untouched_ok(mixed, ncols=n4)  # the kernel mixes the padding up to 4·ceil(n/4), nothing beyond
    return st


@pytest.mark.parametrize("p", range(1, 17))
def test_neighbor_mix_dense(dev, p):
    rng = _rng(p)
    n = 1027
    m = (rng.random((p, p)) + 0.05).astype(np.float32)
    m = (m / m.sum(1, keepdims=True)).astype(np.float32)
    _check_mix(dev, _lib(), _f32(rng, p, n), m, n, f"neighbor_mix P={p} n={n}", extra_ld=4 * (p % 2))


def test_neighbor_mix_sizes_and_structure(dev):
    lib = _lib()
    for n in F4_NS + (WRAP,):
        rng = _rng(n)
        m = np.float32([[0.5, 0.25, 0.25], [0.0, 0.75, 0.25], [0.125, 0.0, 0.875]])
        _check_mix(dev, lib, _f32(rng, 3, n), m, n, f"neighbor_mix P=3 n={n}", extra_ld=4)
    # cyclic shift: row p takes row p + 1 only; exact unless a thread reads a row already written
    for p, n in ((16, 1027), (3, WRAP), (2, 5)):
        x = _f32(_rng(p), p, n)
        m = np.zeros((p, p), dtype=np.float32)
        for r in range(p):
            m[r, (r + 1) % p] = 1.0
        st = Stacked(dev, x, "pad4")
        assert _mix(lib, st, p, n, m) == 0
        assert _same_bits(st.rows, _dev(np.roll(x, -1, axis=0), dev)) and st.untouched_ok(range(p), ncols=st.ld)
        print(f"neighbor_mix cyclic shift P={p} n={n}: bit exact")
    # an all-zero matrix row is left alone; a row nobody reads may hold NaN
    p, n = 5, 1027
    x = _f32(_rng(3), p, n)
    x[2] = np.nan
    m = np.zeros((p, p), dtype=np.float32)
    m[0, [0, 1]] = 0.5
    m[1, [1, 3, 4]] = [0.5, 0.25, 0.25]
    m[4, [0, 4]] = [0.75, 0.25]  # rows 2 (NaN) and 3 are idle; nobody reads row 2
    _check_mix(dev, lib, x, m, n, "neighbor_mix idle and dead rows", extra_ld=8)


def test_neighbor_mix_rejects(dev):
    lib = _lib()
    n = 1027
    x = _f32(_rng(1), 3, n)
    m = np.full((17, 17), 1.0 / 17, dtype=np.float32)
    cases = {
        "P = 17": (Stacked(dev, x, "pad4"), 17, n),
        "P = 0": (Stacked(dev, x, "pad4"), 0, n),
        "ld % 4 != 0": (Stacked(dev, x, "pad4p1"), 3, n),
        "ld < 4·ceil(n/4)": (Stacked(dev, x[:, :1024], "packed"), 3, n),
        "misaligned base": (Stacked(dev, x, "shift"), 3, n),
    }
    for what, (st, p, nn) in cases.items():  # every one returns before the matrix is read
        assert _mix(lib, st, p, nn, m) == 2, what
        assert st.untouched_ok(), what
    assert b"aligned" in lib.myfyp_last_error()


# --------------------------------------------------------------------------------------------
# coordinate median
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 3, 4, 7, 8, 15, 16])
def test_coordinate_median(dev, k):
    from myfyp_amd import ops

    for n in SCALAR_NS:
        rng = _rng(1000 * k + n)
        x = (np.round(_f32(rng, k, n) * 4) / 4).astype(np.float32)  # quarters: ties and zeros everywhere
        x[x == 0] = np.where(rng.random(int((x == 0).sum())) < 0.5, np.float32(-0.0), np.float32(0.0))
        if n >= 7:
            x[0, 0], x[k - 1, 1], x[0, 2], x[k - 1, 2] = np.inf, -np.inf, np.inf, np.inf
            x[:, 3], x[:, 4] = -0.0, 0.0
            x[0, 4] = -0.0
            x[k // 2, 5], x[0, 6] = -0.0, 0.0
        buf = _dev(x, dev)  # rows of a packed [K, n] buffer: 4-byte aligned for odd n
        rows = [buf[i] for i in range(k)]
        fresh = Flat(dev, n, off=1)
        outs = [rows[0], fresh.v, rows[k - 1]] if k > 1 else [rows[0], fresh.v]  # two of them alias input rows
        med, mag = R.coordinate_median(list(x))
        assert not np.isnan(med).any()
        ops.median_into(rows, outs)
        for o in outs:
            if k % 2:
                assert np.array_equal(_np(o).view(np.int32), med.astype(np.float32).view(np.int32)), (k, n)
            else:
                fin = np.isfinite(med)
                g = _np(o)
                assert np.array_equal(g[~fin], med[~fin].astype(np.float32))
                _within(torch.from_numpy(g[fin]), med[fin], mag[fin], 1, f"median K={k} n={n}")
        assert fresh.guards_ok()
        for i in range(1, k - 1):
            assert np.array_equal(_np(buf[i]).view(np.int32), x[i].view(np.int32))  # the other rows are inputs only
        if k % 2:
            print(f"median K={k} n={n}: bit exact")


# --------------------------------------------------------------------------------------------
# SCAFFOLD
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1, 5, 16])
def test_scaffold_reduce(dev, k):
    from myfyp_amd import ops

    for n in SCALAR_NS if k == 5 else SCALAR_NS[:3]:
        rng = _rng(10 * n + k)
        dys, dcs = _f32(rng, k, n), _f32(rng, k, n)
        w = (rng.random(k) * 10 + 0.5).astype(np.float32)
        buf = Flat(dev, 2 * n + 2)
        ops.scaffold_reduce(buf.v, [_dev(r, dev) for r in dys], [_dev(r, dev) for r in dcs], [float(v) for v in w])
        want, mag = R.scaffold_reduce(list(dys), list(dcs), w, n)
        assert buf.guards_ok() and float(buf.v[2 * n + 1]) == k
        if k == 0:
            assert not bool(buf.v.any())  # zeros, weight sum 0, count 0
        else:
            _within(buf.v, want, mag, k, f"scaffold_reduce K={k} n={n}")


@pytest.mark.parametrize("p", [1, 3, 16])
def test_scaffold_apply(dev, p):
    from myfyp_amd import ops

    for n in SCALAR_NS:
        rng = _rng(n + p)
        k = 5
        want, _ = R.scaffold_reduce(list(_f32(rng, k, n)), list(_f32(rng, k, n)), (rng.random(k) + 0.5).astype(np.float32), n)
        packed = want.astype(np.float32)
        x0, c0 = _f32(rng, n), _f32(rng, n)
        for c_init in (False, True):
            xs = Flat(dev, n, off=1, data=x0)
            fresh = [Flat(dev, n) for _ in range(p - 1)]
            c = Flat(dev, n, data=np.full(n, np.nan, dtype=np.float32) if c_init else c0)  # c_init: what c held must not show
            outs = [xs.v] + [f.v for f in fresh]  # the first output is x_start itself
            ops.scaffold_apply(outs, xs.v, _dev(packed, dev), c.v, c_init, 0.7)
            x, c1, mx, mc = R.scaffold_apply(x0, packed, c0, c_init, 0.7)
            _within(xs.v, x, mx, 2, f"scaffold_apply P={p} n={n} c_init={c_init} x")
            _within(c.v, c1, mc, 3, f"scaffold_apply P={p} n={n} c_init={c_init} c")
            assert all(_same_bits(f.v, xs.v) and f.guards_ok() for f in fresh) and xs.guards_ok() and c.guards_ok()


def test_scaffold_empty_round_and_rejects(dev):
    from myfyp_amd import ops

    n = 1001
    rng = _rng(4)
    x0, c0 = _f32(rng, n), _f32(rng, n)
    buf = Flat(dev, 2 * n + 2)
    ops.scaffold_reduce(buf.v, [], [], [])
    xs, c, out = Flat(dev, n, data=x0), Flat(dev, n, data=c0), Flat(dev, n)
    ops.scaffold_apply([out.v], xs.v, buf.v, c.v, False, 0.7)
    assert _same_bits(out.v, xs.v) and _same_bits(c.v, _dev(c0, dev)) and xs.guards_ok(written=False)
    print("scaffold: a K = 0 buffer gives x_start back and leaves c alone, bit for bit")
    lib = _lib()
    tab = (ctypes.c_uint64 * 17)(*([xs.ptr] * 17))
    tp = ctypes.cast(tab, ctypes.c_void_p)
    wk, wp = _host(np.ones(17))
    before = buf.flat.clone()
    assert lib.myfyp_scaffold_reduce(buf.ptr, tp, tp, wp, 17, n, _stream()) == 2
    assert lib.myfyp_scaffold_apply(tp, 0, xs.ptr, buf.ptr, c.ptr, 0, 0.7, n, _stream()) == 2
    assert lib.myfyp_scaffold_apply(tp, 17, xs.ptr, buf.ptr, c.ptr, 0, 0.7, n, _stream()) == 2
    assert _same_bits(buf.flat, before) and xs.guards_ok(written=False) and _same_bits(c.v, _dev(c0, dev))


# --------------------------------------------------------------------------------------------
# optimizer
# --------------------------------------------------------------------------------------------
EXTRAS = [dict(), dict(wd=0.01), dict(mu=0.1), dict(scaf=True), dict(wd=0.01, mu=0.1, scaf=True)]
_ids = lambda e: "+".join(e) or "plain"  # noqa: E731


def _opt_inputs(seed, n):
    """A random non-zero state: |w| ~ 1e-2 against an update of a few 1e-3 at lr = 1e-2."""
    rng = _rng(seed)
    w = 0.01 * _f32(rng, n)
    g, a, cg, cl = _f32(rng, n), 0.01 * _f32(rng, n), 0.1 * _f32(rng, n), 0.1 * _f32(rng, n)
    m = 0.1 * _f32(rng, n)
    v = (0.01 * rng.random(n) + 1e-4).astype(np.float32)
    return w, g, m, v, a, cg, cl


def _adam_case(dev, n, step, ex, seed):
    from myfyp_amd import ops

    w, g, m, v, a, cg, cl = _opt_inputs(seed, n)
    lr, b1, b2, eps = 1e-2, 0.9, 0.999, 1e-8
    wd, mu, scaf = ex.get("wd", 0.0), ex.get("mu", 0.0), ex.get("scaf", False)
    w1, m1, v1, uw, um, uv = R.adam_step(w, g, m, v, step, lr, b1, b2, eps, wd, a if mu else None, mu, cg if scaf else None, cl if scaf else None)
    pw, pm, pv = Flat(dev, n, data=w), Flat(dev, n, off=1, data=m), Flat(dev, n, data=v)
    sh = torch.zeros(n + 2, dtype=torch.bfloat16, device=dev)
    gd, ad, cgd, cld = (_dev(t, dev) for t in (g, a, cg, cl))
    ops.adam_step(pw.v, gd, pm.v, pv.v, step, lr, b1, b2, eps, wd, shadow=sh[:n], anchor=ad if mu else None, c_global=cgd if scaf else None,
                  c_local=cld if scaf else None, mu=mu)
    tag = f"adam {_ids(ex)} step={step} n={n}"
    _within(pm.v, m1, um, 0, f"{tag} m", units=True)
    _within(pv.v, v1, uv, 0, f"{tag} v", units=True)
    _within(pw.v, w1, uw, 0, f"{tag} w", units=True)
    assert pw.guards_ok() and pm.guards_ok() and pv.guards_ok()
    # the shadow is the parameter the kernel wrote, rounded to nearest even
    assert torch.equal(sh[:n].view(torch.int16), pw.v.to(torch.bfloat16).view(torch.int16)) and not bool(sh[n:].any())
    for t, t0 in ((gd, g), (ad, a), (cgd, cg), (cld, cl)):
        assert np.array_equal(_np(t), t0)


@pytest.mark.parametrize("ex", EXTRAS, ids=_ids)
@pytest.mark.parametrize("step", [1, 2, 10, 1000, 100000])
def test_adam_step(dev, step, ex):
    _adam_case(dev, 1001, step, ex, seed=step)


@pytest.mark.parametrize("n", [1, 7, 524291])
def test_adam_step_sizes(dev, n):
    _adam_case(dev, n, 2, EXTRAS[-1], seed=n)
    _adam_case(dev, n, 10, EXTRAS[0], seed=n + 1)


@pytest.mark.parametrize("ex", EXTRAS, ids=_ids)
@pytest.mark.parametrize("mom,nesterov", [(0.0, False), (0.9, False), (0.9, True)])
def test_sgd_step(dev, mom, nesterov, ex):
    from myfyp_amd import ops

    for n in SCALAR_NS:
        w, g, m, v, a, cg, cl = _opt_inputs(n + 5, n)
        lr = 0.05
        wd, mu, scaf = ex.get("wd", 0.0), ex.get("mu", 0.0), ex.get("scaf", False)
        w1, m1, uw, um = R.sgd_step(w, g, m if mom else None, lr, mom, wd, nesterov, a if mu else None, mu, cg if scaf else None, cl if scaf else None)
        pw, pm = Flat(dev, n, off=1, data=w), Flat(dev, n, data=m)
        gd, ad, cgd, cld = (_dev(t, dev) for t in (g, a, cg, cl))
        ops.sgd_step(pw.v, gd, pm.v, lr, mom, wd, nesterov, anchor=ad if mu else None, c_global=cgd if scaf else None, c_local=cld if scaf else None, mu=mu)
        tag = f"sgd {_ids(ex)} momentum={mom} nesterov={nesterov} n={n}"
        _within(pw.v, w1, uw, 0, f"{tag} w", units=True)
        if mom:
            _within(pm.v, m1, um, 0, f"{tag} m", units=True)
        else:
            assert _same_bits(pm.flat, pm.orig)  # momentum == 0 leaves the buffer alone
        assert pw.guards_ok() and pm.guards_ok()


# --------------------------------------------------------------------------------------------
# scale-add-noise
# --------------------------------------------------------------------------------------------
def test_scale_part_exact(dev):
    from myfyp_amd import ops

    for n in SCALAR_NS:
        t0 = _f32(_rng(n), n)
        t0[0] = -0.0
        for scale in (-1.0, 0.5):
            t = Flat(dev, n, off=n % 2, data=t0)
            ops.scale_add_noise(t.v, scale, 0.0, seed=9)
            want = R.scale_part(t0, scale).astype(np.float32)
            assert np.array_equal(_np(t.v).view(np.int32), want.view(np.int32)) and t.guards_ok()
    print("scale_add_noise sigma=0: scale * t bit exact for scale -1 and 0.5")


def test_noise_statistics(dev):
    from myfyp_amd import ops

    n, sigma = 1 << 20, 0.5
    z = {}
    for seed in (3, 4):
        t = torch.zeros(n, device=dev)
        ops.scale_add_noise(t, 1.0, sigma, seed=seed)
        again = torch.zeros(n, device=dev)
        ops.scale_add_noise(again, 1.0, sigma, seed=seed)
        assert _same_bits(t, again)  # the same seed twice
        short = Flat(dev, 1001, off=1, data=np.zeros(1001, dtype=np.float32))
        ops.scale_add_noise(short.v, 1.0, sigma, seed=seed)
        assert _same_bits(short.v, t[:1001]) and short.guards_ok()  # a sample depends on (seed, index) only
        z[seed] = _np(t)
        assert np.all(np.isfinite(z[seed]))
    assert not np.array_equal(z[3], z[4])
    lim = R.noise_limits(n)
    for seed, other in ((3, 4), (4, 3)):
        st = R.noise_stats(z[seed], sigma, z[other])
        for key, val in st.items():
            if key != "n":
                print(f"noise seed {seed} {key}: {val:.4e} (limit {lim[key]:.4e}{', of |var - 1|' if key == 'var' else ''})")
        assert R.noise_check(st) == []
    # scale and noise together: scale * t + the same samples. Two roundings: the sample read back from
    # the run from zeros carries its own, and the sum one more (a contracted sum adds the unrounded sample)
    t0 = _f32(_rng(1), 1001)
    t = _dev(t0, dev)
    ops.scale_add_noise(t, -1.0, sigma, seed=3)
    _within(t, R.scale_part(t0, -1.0) + z[3][:1001].astype(np.float64), np.abs(t0) + np.abs(z[3][:1001]), 2, "scale * t + noise")
