"""The colluding-attack kernels of ``csrc/kernels/fl_ops.hip`` (``k_collude_stats<K>``,
``k_collude_solve``, ``k_collude_write<K>``, behind ``k_pairwise_sqdist<K>``) against float64 on the
same fp32 rows (MI355X only). Inputs, oracle and the bounds below live in ``tests/_collude_ref.py``;
``tests/test_collude_ref_cpu.py`` checks on the CPU, for exactly these inputs, that an fp32 emulation
of the kernels' per-coordinate arithmetic stays inside them.

u = 2^-24. Per coordinate, R is the range of the H honest values (so |x_k − x_0|, |e_k| <= R and
σ <= R/2). The kernels never form μ: they take u_k = x_k − x_0, δ = (Σ u_k)/H, e_k = u_k − δ
(= x_k − μ) and σ = sqrt((Σ e_k²)/H).

* Differences to x_0 round once: u·|u_k|. δ: H − 1 additions and a division behind them, at most
  (H + 1)·u·R. e_k = u_k − δ: the two errors and one more rounding, (H + 3)·u·R =: ε_e.
* σ is the norm of (e_0 .. e_{H-1}) over sqrt(H): an error vector of entries <= ε_e moves it by at
  most ε_e; its H fused multiply-adds, the division and the root add (H/2 + 2)·u·σ <= (H/4 + 1)·u·R.
  Together (1.25 H + 4)·u·R =: ε_σ.
* a_i = Σ e_i², s = Σ σ²: positive terms. A term's error is 2|e|ε_e + ε_e², over the vector at most
  2·sqrt(a_i)·‖ε_e‖ + ‖ε_e‖² (Cauchy-Schwarz, ‖·‖ over the coordinates); an fp32 chain of positive
  terms of depth L is within (L + 3)·u relative, with L = 4 fused multiply-adds per grid-stride step
  (one per coordinate of a group), 6 wave steps and 3 block steps. The slab sums are in double.
* b_i = −Σ e_i σ has mixed signs: absolutely sqrt(a_i)·‖ε_σ‖ + sqrt(s)·‖ε_e‖ + ‖ε_e‖‖ε_σ‖ for the
  factors and the same (L + 3)·u times Σ|e_i σ| <= sqrt(a_i·s) for the chain.
* d_ij (``k_pairwise_sqdist``): a difference rounds once, 2u on its square, then the chain:
  (L + 3 + 2)·u relative, for D and S (maxima, sums in double) alike.
* min-sum: γ = sqrt(ρ − 1), ρ = S/(H s) = 1 + max_i a_i/s >= 2, so γ >= 1 and |Δγ| <= Δρ/(2γ) with
  Δρ = ρ·(rel S + Δs/s). min-max: γ = min_i (b_i + sqrt(disc_i))/s with
  disc_i = b_i² + s(D − a_i) >= s·D·(2H − 1)/H² (a_i <= ((H−1)/H)²·D), so
  |Δγ| <= max_i [(Δb_i + Δdisc_i / (2 sqrt(s D (2H−1)/H²))) / s + γ_i Δs/s],
  Δdisc_i = 2|b_i|Δb_i + Δb_i² + Δs(D − a_i) + (s + Δs)(ΔD + Δa_i). Both plus u·γ: γ is stored as float.
* Output m = fma(ca, x_0, t), t = fma(cb, σ, ca·δ) (and fma(cr, r, m)):
  |ca|·(H + 1)uR + |cb|·ε_σ + |Δγ|·σ for the operands, u·(|ca|R + |t| + |ca x_0| + |t|) for the
  three roundings and u·(|m| + |cr r|) for the reference's. 1 % covers the second-order terms.

There is no NaN screening in the kernels, and no NaN here.
"""

import ctypes

import numpy as np
import pytest
import torch

import _collude_ref as cr
from _collude_ref import BIG, BIG_H, EPS, HS, KINDS, NS, PS, Z

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from myfyp_amd.ops import _native

    _native.load(required=True)  # the native path must be the one under test
    return torch.device("cuda")


def _run(dev, kind, x, ref, p):
    from myfyp_amd import ops

    rows = [r.to(dev).contiguous() for r in x]
    keep = [r.clone() for r in rows]
    outs = [torch.full_like(rows[0], float("nan")) for _ in range(p)]
    gamma, stat = ops.collude_into(rows, outs, kind, z=Z, eps=EPS, ref=ref.to(dev) if kind == "ipm" else None)
    torch.cuda.synchronize()
    for r, k0 in zip(rows, keep):
        assert torch.equal(r, k0)  # the rows are unchanged
    for o in outs[1:]:
        assert torch.equal(o, outs[0])  # all P outputs are bit-equal
    return outs[0].cpu(), float(gamma.cpu()[0]), stat.cpu().numpy()


def _check(dev, kind, h, p, n):
    x, x64, ref, st = cr.case(h, n)
    out, gamma, stat = _run(dev, kind, x, ref, p)
    ref64 = ref.double().numpy()
    if kind in ("min_max", "min_sum"):
        ba, bb, bss, rel_d = cr.stat_bounds(x64, st, n)
        a, b, s, big_d, big_s = stat[:h], stat[h : 2 * h], stat[2 * h], stat[2 * h + 1], stat[2 * h + 2]
        ea, eb = np.abs(a - st["a"]), np.abs(b - st["b"])
        g64 = cr.gamma_of(st, kind)
        bg = cr.gamma_bound(x64, st, n, kind)
        print(f"{kind} H={h} P={p} n={n}: a {ea.max():.3e}/{ba.max():.3e} b {eb.max():.3e}/{bb.max():.3e} s {abs(s - st['s']):.3e}/{bss:.3e} "
              f"D {abs(big_d - st['D']):.3e}/{rel_d * st['D']:.3e} S {abs(big_s - st['S']):.3e}/{rel_d * st['S']:.3e} gamma {gamma:.7g} vs {g64:.7g}: {abs(gamma - g64):.3e}/{bg:.3e}")
        assert (ea <= ba).all() and (eb <= bb).all() and abs(s - st["s"]) <= bss
        assert abs(big_d - st["D"]) <= rel_d * st["D"] and abs(big_s - st["S"]) <= rel_d * st["S"]
        assert abs(gamma - g64) <= bg
        if h == 1:
            assert gamma == 0.0 and s == 0.0
        ca, cb, c_r = 1.0, -g64, 0.0
        dg = bg
    else:
        assert gamma == (Z if kind == "alie" else EPS)
        assert not stat.any()
        ca, cb, c_r = cr.coefs(kind, 0.0)
        dg = 0.0
    m64 = ca * st["mu"] + cb * st["sigma"] + (c_r * ref64 if kind == "ipm" else 0.0)
    bound = cr.out_bound(x64, st, ca, cb, c_r, ref64 if kind == "ipm" else None, dg)
    err = np.abs(out.double().numpy() - m64)
    print(f"{kind} H={h} P={p} n={n}: out worst err/bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all()


@pytest.mark.parametrize("h", HS)
@pytest.mark.parametrize("kind", KINDS)
def test_against_float64(dev, kind, h):
    for p in PS:
        for n in NS:
            _check(dev, kind, h, p, n)


@pytest.mark.parametrize("kind", KINDS)
def test_grid_stride_with_a_tail(dev, kind):
    _check(dev, kind, BIG_H, 1, BIG)


def _int_rows(h, n, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(-8, 9, (n,), generator=g).float() * 16.0 for _ in range(h)]  # multiples of 16: every mean over H <= 16 is exact


@pytest.mark.parametrize("h", [1, 2, 4, 8, 16])
def test_ipm_bit_exact_on_small_integers(dev, h):
    from myfyp_amd import ops

    n = 1027
    rows = _int_rows(h, n, 5 + h)
    ref = _int_rows(1, n, 99)[0]
    out = torch.empty(n, device=dev)
    gamma, _ = ops.collude_into([r.to(dev) for r in rows], [out], "ipm", eps=0.5, ref=ref.to(dev))
    mu = torch.stack(rows).double().mean(dim=0)
    want = (ref.double() - 0.5 * (mu - ref.double())).float()
    assert torch.equal(out.cpu(), want)
    assert float(gamma.cpu()[0]) == 0.5


def test_alie_bit_exact_on_two_integer_rows(dev):
    from myfyp_amd import ops

    n = 1027
    rows = _int_rows(2, n, 31)
    out = torch.empty(n, device=dev)
    gamma, _ = ops.collude_into([r.to(dev) for r in rows], [out], "alie", z=2.0)
    x = torch.stack(rows).double()
    want = (x.mean(dim=0) - 2.0 * (x[0] - x[1]).abs() / 2).float()  # σ = |x_0 − x_1| / 2 is exact
    assert torch.equal(out.cpu(), want)
    assert float(gamma.cpu()[0]) == 2.0


@pytest.mark.parametrize("kind", KINDS)
def test_alignment_does_not_change_the_bits(dev, kind):
    """Rows sliced from a packed [H, n] buffer with odd n (scalar path) against separately
    allocated rows (vector path), and a second call."""
    from myfyp_amd import ops

    h, n = 5, 1027
    x, _, ref, _ = cr.case(h, n)
    packed = x.to(dev).contiguous()
    sliced = [packed[i] for i in range(h)]
    assert any(r.data_ptr() % 16 for r in sliced)
    apart = [x[i].to(dev).clone() for i in range(h)]
    assert not any(r.data_ptr() % 16 for r in apart)
    r_dev = ref.to(dev)
    res = []
    for rows in (sliced, apart, apart):
        outs_packed = torch.empty(2, n, device=dev)
        outs = [outs_packed[1]] if rows is sliced else [torch.empty(n, device=dev)]
        gamma, stat = ops.collude_into(rows, outs, kind, z=Z, eps=EPS, ref=r_dev if kind == "ipm" else None)
        res.append((outs[0].cpu().numpy().tobytes(), gamma.cpu().numpy().tobytes(), stat.cpu().numpy().tobytes()))
    assert res[0] == res[1] == res[2]


def test_entry_point_rejects_bad_arguments(dev):
    from myfyp_amd.ops import _native

    lib = _native.load(required=True)
    n = 64
    rows = [torch.zeros(n, device=dev) for _ in range(17)]
    out = torch.zeros(n, device=dev)
    work = torch.zeros(int(lib.myfyp_collude_work(n, 16)), device=dev)
    gamma = torch.zeros(1, device=dev)
    stat = torch.zeros(40, dtype=torch.float64, device=dev)
    src = (ctypes.c_uint64 * 17)(*[r.data_ptr() for r in rows])
    dst = (ctypes.c_uint64 * 1)(out.data_ptr())
    stream = torch.cuda.current_stream().cuda_stream

    def call(k, p, kind, ref):
        return lib.myfyp_collude_multi(ctypes.cast(dst, ctypes.c_void_p), p, ctypes.cast(src, ctypes.c_void_p), k, kind, 1.0, -1.0, 0.0, ref, n,
                                       work.data_ptr(), gamma.data_ptr(), stat.data_ptr(), stream)

    assert call(17, 1, 2, None) == 2
    assert call(0, 1, 2, None) == 2
    assert call(4, 17, 2, None) == 2
    assert call(4, 1, 1, None) == 2  # ipm without the reference row
    assert call(4, 1, 7, None) == 2
    assert call(4, 1, 2, None) == 0
    torch.cuda.synchronize()
