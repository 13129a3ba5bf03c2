"""The Bulyan kernels of ``csrc/kernels/fl_ops.hip`` (``k_pairwise_sqdist<K>``, ``k_bulyan_select``,
``k_bulyan_mean<K, F>``) against the oracle (``ops.bulyan_into`` on CPU rows) — MI355X only.

Selection: ``pick`` and ``coef`` equal the oracle's exactly; ``dist`` and ``score`` are the bits
``ops.krum_into`` gives on the same rows (the slab sum is shared).

Output bound. Per coordinate the kernel sorts the θ picked values (exact), takes the median
(``0.5f·(a + b)``: one rounding) and the window costs (one rounding each) as the oracle does in
fp32, so both choose the same window; the window's β values are summed in ascending order, β − 1
roundings of partial sums no larger than β·max|x| (2^-24 relative, half an ulp each), and the sum
is divided by β (half an ulp of a quotient no larger than max|x|). Against the float64 mean of the
oracle's window that is at most ``((β − 1) + 1)·2^-24·max|x| = β·2^-24·max|x|``.

Rows of small integers make every sum, median and cost exact, so the outputs are the oracle's
``float32(sum) / float32(β)`` bit for bit, tied window costs included.
"""

import functools

import numpy as np
import pytest
import torch

from myfyp_amd import ops

U = 2.0**-24
# K with the largest admissible f, and f = 0 at K = 1, 2, 16
KF = [(3, 0), (7, 1), (8, 1), (11, 2), (15, 3), (16, 3), (1, 0), (2, 0), (16, 0)]
NS = [1, 3, 5, 1027, 3073]  # the last two: more than one block of 256 x 4 coordinates, ragged tail


@pytest.fixture(scope="module")
def dev():
    from myfyp_amd.ops import _native

    _native.load(required=True)  # the native path must be the one under test
    return torch.device("cuda")


def _window64(x, pick, f):
    """float64 mean of the oracle's window per coordinate, and whether a coordinate has tied costs."""
    k = len(x)
    theta, beta = k - 2 * f, k - 4 * f
    v = np.sort(x[np.asarray(pick) >= 0], axis=0)
    m = v[(theta - 1) // 2] if theta % 2 else np.float32(0.5) * (v[theta // 2 - 1] + v[theta // 2])
    costs = np.stack([np.maximum(m - v[s], v[s + beta - 1] - m) for s in range(2 * f + 1)])
    s = np.argmin(costs, axis=0)  # the first minimum: the lowest s wins a tie
    mean = np.stack([np.take_along_axis(v, (s + j)[None], axis=0)[0].astype(np.float64) for j in range(beta)]).sum(0) / beta
    tied = (np.ptp(np.sort(costs, axis=0)[:2], axis=0) == 0) if f > 0 else np.zeros(x.shape[1], dtype=bool)
    return mean, tied


@functools.lru_cache(maxsize=None)
def _case(k, f, n, integers=False):
    """(rows fp32 [K, n], oracle out, coef, pick, float64 window mean, tied mask): computed once, never written."""
    rng = np.random.default_rng(1000 * k + 10 * f + n % 7)
    x = rng.integers(-6, 7, size=(k, n)).astype(np.float32) if integers else rng.standard_normal((k, n)).astype(np.float32)
    out = torch.empty(n)
    _, _, coef, pick = ops.bulyan_into([torch.from_numpy(r) for r in x], [out], f)
    mean64, tied = _window64(x, pick.tolist(), f)
    return x, out.numpy(), coef.numpy(), pick.numpy(), mean64, tied


def _dev_rows(x, dev):
    return [torch.from_numpy(r).to(dev) for r in x]


@pytest.mark.gpu
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("k,f", KF)
def test_selection_and_output(dev, k, f, n):
    x, want, coef, pick, mean64, _ = _case(k, f, n)
    rows = _dev_rows(x, dev)
    outs = [torch.full((n,), float("nan"), device=dev) for _ in range(3)]
    d, s, c, p = ops.bulyan_into(rows, outs, f)
    assert p.dtype == torch.int32 and c.dtype == torch.float32 and d.dtype == torch.float64 and d.shape == (k, k)
    assert np.array_equal(p.cpu().numpy(), pick)
    assert np.array_equal(c.cpu().numpy(), coef)
    kd, ks, _ = ops.krum_into(rows, [], [1.0] * k, f, 1)
    assert torch.equal(d, kd) and torch.equal(s, ks)  # the same bits
    bound = (k - 4 * f) * U * float(np.abs(x).max())
    got = outs[0].cpu().numpy()
    err = float(np.abs(got.astype(np.float64) - mean64).max())
    print(f"K={k} f={f} n={n}: max error {err:.3e}, bound {bound:.3e}, the oracle's bits: {np.array_equal(got, want)}")
    assert err <= bound
    assert float(np.abs(want.astype(np.float64) - mean64).max()) <= bound  # the oracle itself
    assert all(torch.equal(o, outs[0]) for o in outs[1:])
    for r, r0 in zip(rows, x):
        assert np.array_equal(r.cpu().numpy(), r0)  # the rows are only read


@pytest.mark.gpu
@pytest.mark.parametrize("k,f", [(7, 1), (8, 1), (11, 2), (15, 3), (16, 3), (16, 0), (3, 0)])
def test_integer_rows_are_bit_exact(dev, k, f):
    n = 1027
    x, want, coef, pick, _, tied = _case(k, f, n, True)
    assert f == 0 or tied.any()  # coordinates whose two cheapest windows cost the same
    out = torch.empty(n, device=dev)
    _, _, c, p = ops.bulyan_into(_dev_rows(x, dev), [out], f)
    assert np.array_equal(p.cpu().numpy(), pick) and np.array_equal(c.cpu().numpy(), coef)
    assert np.array_equal(out.cpu().numpy(), want)


@pytest.mark.gpu
@pytest.mark.parametrize("k,f,n", [(8, 1, 1027), (16, 3, 3073), (11, 2, 5), (3, 0, 3)])
def test_unaligned_packed_rows(dev, k, f, n):
    """Row i of a packed [K, n] buffer with odd n is only 4-byte aligned: same bits as aligned copies."""
    x = _case(k, f, n)[0]
    packed = torch.from_numpy(x).to(dev).contiguous()
    rows_u = [packed[i] for i in range(k)]
    assert any(r.data_ptr() % 16 for r in rows_u)
    rows_a = _dev_rows(x, dev)
    assert all(r.data_ptr() % 16 == 0 for r in rows_a)
    out_a = torch.empty(n, device=dev)
    out_u = torch.empty(k, n, device=dev)  # unaligned outputs too
    ra = ops.bulyan_into(rows_a, [out_a], f)
    ru = ops.bulyan_into(rows_u, [out_u[1], out_u[2]] if k > 2 else [out_u[1]], f)
    assert all(torch.equal(a, b) for a, b in zip(ra, ru))
    assert torch.equal(out_u[1], out_a)
    # aligned rows into an unaligned output: the scalar stores of the same values
    ops.bulyan_into(rows_a, [out_u[1]], f)
    assert torch.equal(out_u[1], out_a)


@pytest.mark.gpu
@pytest.mark.parametrize("k,f,n", [(8, 1, 3073), (16, 3, 1027), (7, 1, 5)])
def test_outputs_may_alias_the_rows(dev, k, f, n):
    x = _case(k, f, n)[0]
    sep = torch.empty(n, device=dev)
    ops.bulyan_into(_dev_rows(x, dev), [sep], f)
    rows = _dev_rows(x, dev)
    ops.bulyan_into(rows, rows, f)  # every row is an output
    assert all(torch.equal(r, sep) for r in rows)


@pytest.mark.gpu
@pytest.mark.parametrize("k,f,n", [(8, 1, 1027), (16, 3, 3073), (11, 2, 3)])
def test_unpicked_rows_are_never_read(dev, k, f, n):
    """The mean kernel takes the selection from ``coef`` and skips the other rows: NaN written over
    them after the selection does not reach the output."""
    x = _case(k, f, n)[0]
    rows = _dev_rows(x, dev)
    want = torch.empty(n, device=dev)
    _, _, coef, pick = ops.bulyan_into(rows, [want], f)
    for i in range(k):
        if int(pick[i]) < 0:
            rows[i].fill_(float("nan"))
    got = torch.empty(n, device=dev)
    ops.bulyan_mean_into(rows, [got], coef, f)
    assert torch.equal(got, want)


@pytest.mark.gpu
def test_non_finite_rows(dev):
    """At most f rows of NaN, Inf or overflowing values: never picked, the output finite."""
    k, f, n = 11, 2, 1027
    for bad in (float("nan"), float("inf"), 3e38):
        x = _case(k, f, n)[0].copy()
        x[2] = bad
        x[9, 5] = bad
        out = torch.empty(n, device=dev)
        _, _, coef, pick = ops.bulyan_into(_dev_rows(x, dev), [out], f)
        assert torch.isfinite(out).all()
        assert coef[2] == 0 and coef[9] == 0 and int((coef != 0).sum()) == k - 2 * f
        cpu = torch.empty(n)
        _, _, _, pick_cpu = ops.bulyan_into([torch.from_numpy(r) for r in x], [cpu], f)
        assert torch.equal(pick.cpu(), pick_cpu)
        mean64, _ = _window64(x, pick_cpu.tolist(), f)
        bound = (k - 4 * f) * U * float(np.abs(x[pick_cpu.numpy() >= 0]).max())
        assert float(np.abs(out.cpu().numpy().astype(np.float64) - mean64).max()) <= bound


@pytest.mark.gpu
def test_two_calls_give_the_same_bits(dev):
    k, f, n = 16, 3, 3073
    rows = _dev_rows(_case(k, f, n)[0], dev)
    a, b = torch.empty(n, device=dev), torch.empty(n, device=dev)
    ra = ops.bulyan_into(rows, [a], f)
    rb = ops.bulyan_into(rows, [b], f)
    assert torch.equal(a, b) and all(torch.equal(p, q) for p, q in zip(ra, rb))


@pytest.mark.gpu
def test_argument_errors_native(dev):
    """The C entry point refuses bad arguments with a message before any launch."""
    import ctypes

    from myfyp_amd.ops import _native

    lib = _native.load(required=True)
    k, n = 6, 8
    rows = [torch.zeros(n, device=dev) for _ in range(17)]
    out = torch.full((n,), 7.0, device=dev)
    src = (ctypes.c_uint64 * 17)(*[r.data_ptr() for r in rows])
    dst = (ctypes.c_uint64 * 1)(out.data_ptr())
    work = torch.empty(4096, device=dev)
    dist = torch.empty(17 * 17, dtype=torch.float64, device=dev)
    score = torch.empty(17, dtype=torch.float64, device=dev)
    pick = torch.full((17,), 5, dtype=torch.int32, device=dev)
    coef = torch.empty(17, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def call(k_, f_, n_, p_=1, work_=work.data_ptr(), pick_=pick.data_ptr()):
        rc = lib.myfyp_bulyan_multi(ctypes.cast(dst, ctypes.c_void_p), p_, ctypes.cast(src, ctypes.c_void_p), k_, f_, n_, work_, dist.data_ptr(),
                                    score.data_ptr(), pick_, coef.data_ptr(), st)
        return rc, lib.myfyp_last_error().decode()

    for args, word in [((k, 1, n), "4f + 3"), ((k, -1, n), "f >= 0"), ((17, 0, n), "1..16 rows"), ((0, 0, n), "1..16 rows"), ((7, 1, 0), "n >= 1"),
                       ((7, 1, n, 17), "1..16 rows"), ((7, 1, n, 1, None), "required"), ((7, 1, n, 1, work.data_ptr(), None), "required")]:
        rc, msg = call(*args)
        assert rc == 2 and word in msg, (args, rc, msg)
    rc = lib.myfyp_bulyan_mean_multi(ctypes.cast(dst, ctypes.c_void_p), 1, ctypes.cast(src, ctypes.c_void_p), k, 1, n, coef.data_ptr(), st)
    assert rc == 2 and "4f + 3" in lib.myfyp_last_error().decode()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((pick == 5).all())  # nothing was launched
    with pytest.raises(ValueError, match=r"K = 6.*f = 1"):
        ops.bulyan_into(rows[:6], [out], 1)
    with pytest.raises(ValueError, match="f = -1"):
        ops.bulyan_into(rows[:7], [out], -1)
    with pytest.raises(ValueError, match="length"):
        ops.bulyan_into(rows[:7], [torch.zeros(n + 1, device=dev)], 1)
