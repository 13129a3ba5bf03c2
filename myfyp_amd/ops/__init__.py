"""Fused device ops (HIP, gfx950) with PyTorch reference implementations for CPU hosts.

Every op takes/returns torch tensors. Device tensors go to the hand-written kernels in
``csrc/kernels`` (through :mod:`myfyp_amd.ops._native`); CPU tensors use the reference math below,
which is also the numerics oracle in ``tests/test_kernels_gpu.py``.

Ops
---
* ``weighted_average``  — FedAvg reduction over K models (multi-tensor, one launch per layer list)
* ``stacked_weighted_sum`` / ``broadcast_rows`` — reductions over a ``[P, N]`` stacked flat buffer
  (co-located peers) feeding / consuming the RCCL all-reduce
* ``coordinate_median`` — FedMedian (register sorting network, K ≤ 16)
* ``trimmed_mean_into`` — coordinate-wise trimmed mean (the median's sorting network, K ≤ 16)
* ``krum_into`` — (Multi-)Krum: pairwise squared distances from differences, selection and the
  weighted mean of the chosen rows, all on the device (K ≤ 16); returns ``(dist, score, coef)``
* ``geometric_median_into`` — geometric median (RFA, smoothed Weiszfeld): a screen of non-finite
  rows, then per step the distances to the current point and the reweighting, all on the device
  (K ≤ 16); returns ``(coef, dist, objective)``
* ``bulyan_into`` — Bulyan: Krum's distances, θ = K − 2f rows picked by iterated Krum, then per
  coordinate the mean of the K − 4f picked values closest to their median, all on the device
  (K ≤ 16); returns ``(dist, score, coef, pick)``
* ``dnc_into`` — DnC spectral filtering: per iteration Krum's distances over a subsample of the
  coordinates, the top eigenpair of the centred Gram matrix ``−½·J·D·J``, the rows of largest
  projection removed, then the weighted mean of the rows kept, all on the device (K ≤ 16); returns
  ``(dist, score, lam, removed, coef)``
* ``clipped_gossip_into`` — ClippedGossip: Krum's distances, per row a clipping radius and the
  clipped neighbour weights, then the mix in place, all on the device (K ≤ 16); returns
  ``(dist, tau, w_eff)``
* ``adam_step`` / ``sgd_step`` — fused optimizers over a flat buffer, optionally with the FedProx
  proximal term and the SCAFFOLD control-variate correction fused in (K5, K8, K13)
* ``scale_add_noise`` — attack injection (sign flip / Gaussian noise, K14)
* ``collude_into`` — colluding omniscient attacks (ALIE, IPM, min-max, min-sum, K14): one crafted
  row from the honest rows' mean and spread written into the attackers' rows, γ solved on the
  device (≤ 16 honest rows); returns ``(gamma, stat)``
"""

from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence

import torch

from myfyp_amd.ops import _native

__all__ = [
    "weighted_average",
    "stacked_weighted_sum",
    "broadcast_rows",
    "coordinate_median",
    "trimmed_mean_into",
    "krum_into",
    "geometric_median_into",
    "bulyan_into",
    "dnc_into",
    "clipped_gossip_into",
    "collude_into",
    "alie_z",
    "adam_step",
    "sgd_step",
    "scale_add_noise",
    "native_available",
]


def native_available() -> bool:
    return _native.available()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _lib():
    return _native.load(required=True)


def fast_lib():
    """Native library with GIL-holding bindings for launch-only entry points (see _native.load_fast)."""
    return _native.load_fast()


def check(rc: int, what: str) -> None:
    _native.check(rc, what)


# ---------------------------------------------------------------------------------------------
# aggregation
# ---------------------------------------------------------------------------------------------
def weighted_average(param_lists: Sequence[Sequence[torch.Tensor]], norm_weights: Sequence[float]) -> List[torch.Tensor]:
    """``out[l] = Σ_k w_k · params[k][l]`` (weights already normalised)."""
    k = len(param_lists)
    out: List[torch.Tensor] = []
    dev = param_lists[0][0].device
    if dev.type != "cuda":
        for layer in range(len(param_lists[0])):
            acc = torch.zeros_like(param_lists[0][layer], dtype=torch.float64)
            for p, w in zip(param_lists, norm_weights):
                if w != 0:  # as on the device: a model of weight 0 is never read
                    acc += p[layer].double() * w
            out.append(acc.to(param_lists[0][layer].dtype))
        return out
    lib = _lib()
    w = torch.tensor(list(norm_weights), dtype=torch.float32, device=dev)
    for layer in range(len(param_lists[0])):
        srcs = [p[layer].contiguous().float() for p in param_lists]
        dst = torch.empty_like(srcs[0])
        ptrs = torch.tensor([s.data_ptr() for s in srcs], dtype=torch.int64, device=dev)
        # a layer view at an odd offset of a flat buffer is only 4-byte aligned: the kernel reads its row
        # pointers from device memory, so the vector path is chosen here, from the pointers in hand
        aligned = all(s.data_ptr() % 16 == 0 for s in srcs)
        _native.check(lib.myfyp_weighted_sum(dst.data_ptr(), ptrs.data_ptr(), w.data_ptr(), k, dst.numel(), int(aligned), _stream()), "weighted_sum")
        out.append(dst.to(param_lists[0][layer].dtype))
    return out


def stacked_weighted_sum(stacked: torch.Tensor, weights: torch.Tensor, out: torch.Tensor, scale: float = 1.0) -> torch.Tensor:
    """``out[n] = scale · Σ_p weights[p] · stacked[p, n]`` for a ``[P, N]`` fp32 buffer. Rows of
    weight 0 are never read (a peer that did not train may hold anything)."""
    if stacked.device.type != "cuda":
        keep = weights != 0
        out.copy_((weights[keep].view(-1, 1).to(stacked.dtype) * stacked[keep]).sum(0) * scale)
        return out
    lib = _lib()
    p, n = stacked.shape
    _native.check(
        lib.myfyp_stacked_weighted_sum(out.data_ptr(), stacked.data_ptr(), p, n, stacked.stride(0), weights.data_ptr(), float(scale), _stream()),
        "stacked_weighted_sum",
    )
    return out


def broadcast_rows(src: torch.Tensor, stacked: torch.Tensor, mask: Optional[torch.Tensor] = None, shadow: Optional[torch.Tensor] = None) -> None:
    """``stacked[p, :] = src`` for every row p with ``mask[p] != 0`` (and the bf16 shadow copy)."""
    if stacked.device.type != "cuda":
        rows = range(stacked.shape[0]) if mask is None else [i for i in range(stacked.shape[0]) if float(mask[i]) != 0]
        for r in rows:
            stacked[r].copy_(src)
            if shadow is not None:
                shadow[r].copy_(src.to(shadow.dtype))
        return
    lib = _lib()
    p, n = stacked.shape
    _native.check(lib.myfyp_broadcast_rows(stacked.data_ptr(), src.data_ptr(), p, n, stacked.stride(0), _ptr(mask), _stream()), "broadcast_rows")
    if shadow is not None:
        shadow.copy_(stacked.to(shadow.dtype))


def coordinate_median(param_lists: Sequence[Sequence[torch.Tensor]]) -> List[torch.Tensor]:
    k = len(param_lists)
    out: List[torch.Tensor] = []
    dev = param_lists[0][0].device
    if dev.type != "cuda" or k > 16:
        for layer in range(len(param_lists[0])):
            st = torch.stack([p[layer].float() for p in param_lists])
            s, _ = torch.sort(st, dim=0)
            med = s[(k - 1) // 2] if k % 2 else 0.5 * (s[k // 2 - 1] + s[k // 2])
            out.append(med.to(param_lists[0][layer].dtype))
        return out
    for layer in range(len(param_lists[0])):
        srcs = [p[layer].contiguous().float().reshape(-1) for p in param_lists]
        dst = torch.empty_like(srcs[0])
        median_into(srcs, [dst])
        out.append(dst.view_as(param_lists[0][layer]).to(param_lists[0][layer].dtype))
    return out


def _host_ptrs(ts: Sequence[torch.Tensor]) -> ctypes.c_void_p:
    """Host table of device row pointers (the native entry points pass it as a kernel argument)."""
    arr = (ctypes.c_uint64 * max(1, len(ts)))(*[t.data_ptr() for t in ts])
    return ctypes.cast(arr, ctypes.c_void_p), arr  # keep arr alive across the call


def median_into(rows: Sequence[torch.Tensor], outs: Sequence[torch.Tensor]) -> None:
    """``outs[p] = coordinate-wise median(rows)`` for 1-D fp32 rows; on the GPU one launch
    (``k_coordinate_median<K>``) for K <= 16 rows and <= 16 outputs, which may alias the rows.

    On every device a coordinate is sorted in the order ``-inf < ... < -0.0 < +0.0 < ... < +inf < NaN``:
    a NaN is the largest value, so the median is NaN only when a NaN reaches the middle (more than
    ``(K - 1) // 2`` of them in one coordinate), and the even-K median is ``0.5 * (a + b)``."""
    k = len(rows)
    if rows[0].device.type == "cuda" and k <= 16 and len(outs) <= 16 and all(t.is_contiguous() and t.dtype == torch.float32 for t in [*rows, *outs]):
        src, keep_s = _host_ptrs(rows)
        dst, keep_d = _host_ptrs(outs)
        _native.check(_lib().myfyp_coordinate_median_multi(dst, len(outs), src, k, rows[0].numel(), _stream()), "coordinate_median_multi")
        return
    s, _ = torch.sort(torch.stack([r.float() for r in rows]), dim=0)
    med = s[(k - 1) // 2] if k % 2 else 0.5 * (s[k // 2 - 1] + s[k // 2])
    for o in outs:
        o.copy_(med)


def _native_rows(rows: Sequence[torch.Tensor], outs: Sequence[torch.Tensor]) -> bool:
    """Rows and outputs the row-pointer kernels take: device, <= 16 each, contiguous fp32."""
    return (rows[0].device.type == "cuda" and len(rows) <= 16 and len(outs) <= 16
            and all(t.is_contiguous() and t.dtype == torch.float32 for t in [*rows, *outs]))


def trimmed_mean_into(rows: Sequence[torch.Tensor], outs: Sequence[torch.Tensor], trim: int) -> None:
    """``outs[p] = mean(sorted(rows)[trim : K - trim])`` per coordinate for 1-D fp32 rows
    (``0 <= 2·trim < K``); on the GPU one launch (``k_trimmed_mean<K>``) for K <= 16 rows and
    <= 16 outputs, which may alias the rows. Elsewhere: sort and mean in float64.

    On every device a coordinate is sorted in the order ``-inf < ... < -0.0 < +0.0 < ... < +inf < NaN``:
    a NaN is the largest value and is trimmed first; with more than ``trim`` of them in one
    coordinate a NaN is kept and that output is NaN."""
    k = len(rows)
    trim = int(trim)
    if trim < 0 or 2 * trim >= k:
        raise ValueError(f"trimmed mean of {k} rows cannot drop {trim} from each end")
    if _native_rows(rows, outs):
        if not outs or rows[0].numel() == 0:
            return
        src, keep_s = _host_ptrs(rows)
        dst, keep_d = _host_ptrs(outs)
        _native.check(_lib().myfyp_trimmed_mean_multi(dst, len(outs), src, k, trim, rows[0].numel(), _stream()), "trimmed_mean_multi")
        return
    s, _ = torch.sort(torch.stack([r.double() for r in rows]), dim=0)
    mean = s[trim : k - trim].sum(dim=0) / (k - 2 * trim)
    for o in outs:
        o.copy_(mean)


def krum_neighbours(k: int, f: int) -> int:
    """Distances a Krum score sums: the ``K - f - 2`` nearest rows, at least 1, at most the K - 1 others."""
    return min(max(1, k - int(f) - 2), k - 1)


def krum_into(rows: Sequence[torch.Tensor], outs: Sequence[torch.Tensor], weights: Sequence[float], f: int, m: int):
    """(Multi-)Krum over 1-D fp32 rows: squared distances from differences, per row the score over
    its :func:`krum_neighbours` nearest rows, the ``max(1, min(m, K))`` lowest scores chosen (the
    lower index wins a tie, a NaN score orders last), ``outs[p] = Σ_k coef[k]·rows[k]`` with
    ``coef[k] = w_k / Σ_chosen w`` (0 for the others). Returns ``(dist [K, K] float64, score [K]
    float64, coef [K] float32)`` on the rows' device; ``outs=[]`` gives the selection only.

    On the GPU (K <= 16 rows, <= 16 outputs, which may alias the rows) it is three launches —
    ``k_pairwise_sqdist<K>``, ``k_krum_select``, ``k_coef_mean<K>`` — that only enqueue: the host
    learns the selection when it reads a returned tensor. Elsewhere: float64 torch math (the oracle)."""
    k = len(rows)
    if len(weights) != k:
        raise ValueError(f"{k} rows but {len(weights)} weights")
    dev = rows[0].device
    if _native_rows(rows, outs):
        lib = _lib()
        n = rows[0].numel()
        pairs = k * (k - 1) // 2
        work = torch.empty(max(1, int(lib.myfyp_krum_grid(n, k)) * pairs), dtype=torch.float32, device=dev)
        dist = torch.empty(k, k, dtype=torch.float64, device=dev)
        score = torch.empty(k, dtype=torch.float64, device=dev)
        coef = torch.empty(k, dtype=torch.float32, device=dev)
        src, keep_s = _host_ptrs(rows)
        dst, keep_d = _host_ptrs(outs)
        w = (ctypes.c_float * k)(*[float(x) for x in weights])
        _native.check(lib.myfyp_krum_multi(dst, len(outs), src, ctypes.cast(w, ctypes.c_void_p), k, int(f), int(m), n, work.data_ptr(), dist.data_ptr(),
                                           score.data_ptr(), coef.data_ptr(), _stream()), "krum_multi")
        return dist, score, coef
    x = [r.double() for r in rows]
    dist = torch.zeros(k, k, dtype=torch.float64, device=dev)
    for i in range(k):
        for j in range(i + 1, k):
            dist[i, j] = dist[j, i] = (x[i] - x[j]).square().sum()
    cnt = krum_neighbours(k, f)
    score = torch.zeros(k, dtype=torch.float64, device=dev)
    inf = float("inf")
    for i in range(k):
        others = [float(dist[i, j]) for j in range(k) if j != i]
        others.sort(key=lambda v: inf if v != v else v)  # stable; NaN last
        score[i] = float(sum(others[:cnt]))  # ascending order
    sc = [float(v) for v in score]
    order = sorted(range(k), key=lambda i: (inf if sc[i] != sc[i] else sc[i], i))
    chosen = sorted(order[: max(1, min(int(m), k))])
    wsum = float(sum(float(weights[i]) for i in chosen))
    coef64 = torch.zeros(k, dtype=torch.float64)
    for i in chosen:
        coef64[i] = float(weights[i]) / wsum if wsum > 0 else 1.0 / len(chosen)
    coef = coef64.float().to(dev)
    if outs:
        mean = torch.zeros_like(x[0])
        for i in chosen:
            mean += float(coef[i]) * x[i]
        for o in outs:
            o.copy_(mean)
    return dist, score, coef


def _clip_check(w, k: int, tau, num_byzantine) -> None:
    """The arguments of a ClippedGossip call, checked before anything is launched or written."""
    import numpy as np

    if (tau is None) == (num_byzantine is None):
        raise ValueError("clipped gossip takes exactly one of tau and num_byzantine")
    if tau is not None and not float(tau) >= 0:
        raise ValueError(f"clipped gossip: the radius tau must be >= 0, got {tau}")
    if num_byzantine is not None and (int(num_byzantine) != num_byzantine or num_byzantine < 0):
        raise ValueError(f"clipped gossip: num_byzantine must be an integer >= 0, got {num_byzantine}")
    if w.shape != (k, k):
        raise ValueError(f"clipped gossip: {k} rows but a weight matrix of shape {w.shape}")
    if not (np.isfinite(w).all() and (w >= 0).all()):
        raise ValueError("clipped gossip: the weights must be finite and >= 0")


def clip_plan(dist, w, tau: Optional[float] = None, num_byzantine: Optional[int] = None):
    """ClippedGossip's radii and clipped weights from the squared distances ``dist [K, K]`` and the
    shares ``w [K, K]`` (numpy, float64 math): ``(tau [K] float64, w_eff [K, K] float32)``. Row p's
    neighbours are the ``q != p`` with ``w[p, q] > 0``. With ``tau`` every radius is ``tau``; with
    ``num_byzantine = b`` the ``min(b, |N_p|)`` farthest neighbours (a non-finite distance counts as
    +inf, the higher row is the farther of two equals) are set aside and ``τ_p² = Σ_rest w·D /
    Σ_aside w`` (``b == 0``: +inf; nobody left: 0). ``w_eff[p, q] = float32(w[p, q] · s)`` with
    ``s = 1`` where ``D <= τ_p²``, else ``τ_p / sqrt(D)``, and 0 at a non-finite distance."""
    import numpy as np

    w = np.asarray(w, dtype=np.float64)
    k = w.shape[0]
    dist = np.asarray(dist, dtype=np.float64)
    if dist.shape != (k, k):
        raise ValueError(f"clipped gossip: w is {w.shape} and dist {dist.shape}, both must be [K, K]")
    _clip_check(w, k, tau, num_byzantine)
    taus = np.zeros(k)
    w_eff = np.zeros((k, k), dtype=np.float32)
    inf = float("inf")
    with np.errstate(all="ignore"):
        for p in range(k):
            nb = [q for q in range(k) if q != p and w[p, q] > 0]
            key = {q: float(dist[p, q]) if np.isfinite(dist[p, q]) else inf for q in nb}
            if tau is not None:
                tp = float(tau)
                tp2 = tp * tp
            elif num_byzantine == 0:
                tp = tp2 = inf
            elif num_byzantine >= len(nb):
                tp = tp2 = 0.0
            else:
                aside = set(sorted(nb, key=lambda q: (key[q], q))[len(nb) - int(num_byzantine):])
                delta = float(sum(w[p, q] for q in nb if q in aside))  # ascending q
                rest = np.float64(0.0)
                for q in nb:
                    if q not in aside:
                        rest = rest + w[p, q] * key[q]
                tp2 = float(rest / delta)
                tp = float(np.sqrt(tp2))
            taus[p] = tp
            for q in nb:
                d = float(dist[p, q])
                if np.isfinite(d):
                    w_eff[p, q] = np.float32(w[p, q] * (1.0 if d <= tp2 else tp / np.sqrt(d)))
    return taus, w_eff


def clipped_gossip_into(rows: Sequence[torch.Tensor], w, tau: Optional[float] = None, num_byzantine: Optional[int] = None):
    """ClippedGossip (He, Karimireddy, Jaggi, 2022) over 1-D fp32 rows, in place: row p moves towards
    each neighbour by at most its radius, ``x_p ← x_p + Σ_q w_eff[p, q]·(x_q − x_p)`` (q ascending;
    a q of ``w_eff`` 0 never enters the sum), with the radii and ``w_eff`` of :func:`clip_plan` from
    the squared distances (from differences) and ``w [K, K]`` taken as float32: ``w[p, q]`` is the
    share row p gives neighbour q, the diagonal is ignored and a row of zeros marks a source that
    is never written. Exactly one of ``tau`` (fixed radius) and ``num_byzantine`` (adaptive radius)
    is given. Returns ``(dist [K, K] float64, tau [K] float64, w_eff [K, K] float32)`` on the rows'
    device.

    On the GPU (K <= 16 rows) it is three launches — ``k_pairwise_sqdist<K>``, ``k_clip_plan``,
    ``k_clipped_mix<K>`` — that only enqueue: the host learns the plan when it reads a returned
    tensor. Elsewhere: float64 torch math (the definition)."""
    import numpy as np

    k = len(rows)
    w32 = np.ascontiguousarray(np.asarray(w, dtype=np.float32))
    _clip_check(w32, k, tau, num_byzantine)
    dev = rows[0].device
    if _native_rows(rows, []):
        lib = _lib()
        n = rows[0].numel()
        alloc = torch.zeros if k == 1 else torch.empty  # one row: nothing is launched
        work = torch.empty(max(1, int(lib.myfyp_krum_grid(n, k)) * (k * (k - 1) // 2)), dtype=torch.float32, device=dev)
        dist = alloc(k, k, dtype=torch.float64, device=dev)
        taus = alloc(k, dtype=torch.float64, device=dev)
        w_eff = alloc(k, k, dtype=torch.float32, device=dev)
        src, keep_s = _host_ptrs(rows)
        mode, t, b = (0, float(tau), 0) if tau is not None else (1, 0.0, int(num_byzantine))
        _native.check(lib.myfyp_clipped_gossip(src, k, w32.ctypes.data, mode, t, b, n, work.data_ptr(), dist.data_ptr(), taus.data_ptr(),
                                               w_eff.data_ptr(), _stream()), "clipped_gossip")
        return dist, taus, w_eff
    x = [r.detach().double() for r in rows]
    dist = torch.zeros(k, k, dtype=torch.float64, device=dev)
    for i in range(k):
        for j in range(i + 1, k):
            dist[i, j] = dist[j, i] = (x[i] - x[j]).square().sum()
    taus, w_eff = clip_plan(dist.cpu().numpy(), w32, tau, num_byzantine)
    with torch.no_grad():
        for p in range(k):
            srcs = [q for q in range(k) if w_eff[p, q] != 0]
            if not srcs:
                continue
            acc = torch.zeros_like(x[p])
            for q in srcs:
                acc += float(w_eff[p, q]) * (x[q] - x[p])
            rows[p].copy_(x[p] + acc)
    return dist, torch.from_numpy(taus).to(dev), torch.from_numpy(w_eff).to(dev)


def bulyan_check(k: int, f: int) -> int:
    """The attacker bound of a Bulyan call, checked: ``f >= 0`` and ``K >= 4f + 3``. With ``f == 0``
    nothing is rejected or trimmed (the result is the mean of all rows), so any ``K >= 1`` does."""
    if int(f) != f or f < 0:
        raise ValueError(f"Bulyan: the attacker bound f must be an integer >= 0, got f = {f} (K = {k})")
    f = int(f)
    if k < 1 or (f > 0 and k < 4 * f + 3):
        raise ValueError(f"Bulyan needs K >= 4f + 3 models: K = {k}, f = {f} needs {4 * f + 3}")
    return f


def bulyan_select(dist, f: int):
    """Bulyan's stage 1 on a K x K table of squared distances (anything ``float()`` reads): θ = K − 2f
    rounds, each scoring every remaining row by the sum, in ascending order, of its
    ``clamp(r − f − 2, 1, r − 1)`` smallest distances to the other remaining rows (r of them remain; a
    NaN orders as +inf) and picking the lowest score, the lower index winning a tie. Returns
    ``(pick, score)``: the round each row was picked at (−1: never) and the first round's scores."""
    k = len(dist)
    inf = float("inf")
    d = [[float(dist[i][j]) for j in range(k)] for i in range(k)]
    remaining = list(range(k))
    pick = [-1] * k
    first = [0.0] * k
    for it in range(k - 2 * f):
        r = len(remaining)
        cnt = min(max(r - f - 2, 1), r - 1)
        scores = {}
        for i in remaining:
            others = [d[i][j] for j in remaining if j != i]
            others.sort(key=lambda v: inf if v != v else v)  # stable; NaN last
            scores[i] = float(sum(others[:cnt]))
        if it == 0:
            first = [scores[i] for i in range(k)]
        best = min(remaining, key=lambda i: (inf if scores[i] != scores[i] else scores[i], i))
        pick[best] = it
        remaining.remove(best)
    return pick, first


def _bulyan_stage2(picked: Sequence[torch.Tensor], outs: Sequence[torch.Tensor], k: int, f: int) -> None:
    """Stage 2 of :func:`bulyan_into` over the θ picked rows, in fp32 torch math."""
    theta, beta = k - 2 * f, k - 4 * f
    v, _ = torch.sort(torch.stack([r.float().reshape(-1) for r in picked]), dim=0)
    m = v[(theta - 1) // 2] if theta % 2 else 0.5 * (v[theta // 2 - 1] + v[theta // 2])
    best, mean = None, None
    for s in range(2 * f + 1):
        cost = torch.maximum(m - v[s], v[s + beta - 1] - m)
        acc = v[s].clone()
        for j in range(1, beta):
            acc += v[s + j]
        if best is None:
            best, mean = cost, acc
        else:
            better = cost < best
            best = torch.where(better, cost, best)
            mean = torch.where(better, acc, mean)
    mean = mean / torch.tensor(float(beta), dtype=torch.float32, device=mean.device)
    for o in outs:
        o.copy_(mean)


def bulyan_mean_into(rows: Sequence[torch.Tensor], outs: Sequence[torch.Tensor], coef: torch.Tensor, f: int) -> None:
    """Stage 2 of :func:`bulyan_into` alone, from a selection already made: ``coef [K]`` is != 0
    for exactly the K − 2f picked rows, and the others are never read. On the GPU one launch
    (``k_bulyan_mean<K, f>``) that takes ``coef`` from device memory."""
    k = len(rows)
    f = bulyan_check(k, f)
    if not outs:
        return
    if _native_rows(rows, outs) and coef.device == rows[0].device and coef.dtype == torch.float32 and coef.is_contiguous() and coef.numel() == k:
        src, keep_s = _host_ptrs(rows)
        dst, keep_d = _host_ptrs(outs)
        _native.check(_lib().myfyp_bulyan_mean_multi(dst, len(outs), src, k, f, rows[0].numel(), coef.data_ptr(), _stream()), "bulyan_mean_multi")
        return
    on = coef.tolist()
    if sum(1 for c in on if c != 0) != k - 2 * f:
        raise ValueError(f"Bulyan: coef must mark K - 2f = {k - 2 * f} rows, got {sum(1 for c in on if c != 0)}")
    _bulyan_stage2([rows[i] for i in range(k) if on[i] != 0], outs, k, f)


def bulyan_into(rows: Sequence[torch.Tensor], outs: Sequence[torch.Tensor], f: int):
    """Bulyan (El Mhamdi, Guerraoui, Rouault, 2018) over 1-D fp32 rows with at most ``f`` attackers
    (``K >= 4f + 3``; ``f == 0`` takes any K). Sample weights are not used.

    Stage 1: squared distances from differences (Krum's), then θ = K − 2f rows picked by iterated
    Krum (:func:`bulyan_select`). Stage 2, per coordinate over the picked rows only, in fp32: the
    values sorted, ``m`` their median (the mean of the middle two for an even θ), the window of
    β = K − 4f consecutive values starting at ``s`` in ``[0, 2f]`` that minimises
    ``max(m − v[s], v[s+β−1] − m)`` (the lowest ``s`` wins a tie): the β values closest to the
    median; ``outs[p]`` = their sum, taken in ascending order, divided by β. With at most f
    non-finite rows those are never picked. The row order matters only through exact ties, which
    are common in the last rounds: a score over one nearest row is the same for the two closest
    rows left. Returns ``(dist [K, K] float64, score [K] float64: Krum's
    score for the same f, coef [K] float32: 1/θ for a picked row and 0 otherwise, pick [K] int32: the
    round a row was picked at, −1 otherwise)`` on the rows' device; ``outs=[]`` gives the selection only.

    On the GPU (K <= 16 rows, <= 16 outputs, which may alias the rows) it is three launches —
    ``k_pairwise_sqdist<K>``, ``k_bulyan_select``, ``k_bulyan_mean<K, f>`` — that only enqueue.
    Elsewhere: torch math, the distances in float64 (the oracle)."""
    k = len(rows)
    f = bulyan_check(k, f)
    dev = rows[0].device
    n = rows[0].numel()
    if n < 1 or any(t.numel() != n for t in [*rows, *outs]):
        raise ValueError(f"Bulyan: rows and outputs must share one length >= 1, got {[t.numel() for t in [*rows, *outs]]}")
    if _native_rows(rows, outs):
        lib = _lib()
        work = torch.empty(max(1, int(lib.myfyp_krum_grid(n, k)) * (k * (k - 1) // 2)), dtype=torch.float32, device=dev)
        dist = torch.empty(k, k, dtype=torch.float64, device=dev)
        score = torch.empty(k, dtype=torch.float64, device=dev)
        coef = torch.empty(k, dtype=torch.float32, device=dev)
        pick = torch.empty(k, dtype=torch.int32, device=dev)
        src, keep_s = _host_ptrs(rows)
        dst, keep_d = _host_ptrs(outs)
        _native.check(lib.myfyp_bulyan_multi(dst, len(outs), src, k, f, n, work.data_ptr(), dist.data_ptr(), score.data_ptr(), pick.data_ptr(),
                                             coef.data_ptr(), _stream()), "bulyan_multi")
        return dist, score, coef, pick
    x = [r.double().reshape(-1) for r in rows]
    dist = torch.zeros(k, k, dtype=torch.float64)
    for i in range(k):
        for j in range(i + 1, k):
            dist[i, j] = dist[j, i] = float((x[i] - x[j]).square().sum())
    picks, first = bulyan_select(dist.tolist(), f)
    theta, beta = k - 2 * f, k - 4 * f
    pick = torch.tensor(picks, dtype=torch.int32)
    coef = torch.where(pick >= 0, torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(theta), dtype=torch.float32), torch.zeros((), dtype=torch.float32))
    score = torch.tensor(first, dtype=torch.float64)
    if outs:
        _bulyan_stage2([rows[i] for i in range(k) if picks[i] >= 0], outs, k, f)
    return dist.to(dev), score.to(dev), coef.to(dev), pick.to(dev)


DNC_MAX_ITERS = 8
DNC_TILE = 256  # coordinates per subsample tile: one wave's 64 float4 groups
DNC_SQUARINGS = 20
_M64 = (1 << 64) - 1


def splitmix64(x: int) -> int:
    """``splitmix64`` of ``fl_ops.hip`` on a Python int (mod 2^64)."""
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def dnc_check(k: int, f, filter_frac, iters, subsample_dims) -> int:
    """The parameters of a DnC call, checked; returns ``m = ceil(filter_frac · f)``, the rows one
    iteration removes. Valid: ``f`` an integer >= 0, ``filter_frac`` finite and >= 0, ``1 <= iters
    <= 8``, ``subsample_dims`` None or an integer >= 1, and ``iters · m < K``."""
    import math

    if isinstance(f, bool) or int(f) != f or f < 0:
        raise ValueError(f"DnC: the attacker bound f must be an integer >= 0, got f = {f} (K = {k})")
    ff = float(filter_frac)
    if not math.isfinite(ff) or ff < 0:
        raise ValueError(f"DnC: filter_frac must be finite and >= 0, got {filter_frac}")
    if isinstance(iters, bool) or int(iters) != iters or not 1 <= iters <= DNC_MAX_ITERS:
        raise ValueError(f"DnC: iters must be an integer in [1, {DNC_MAX_ITERS}], got {iters}")
    if subsample_dims is not None and (isinstance(subsample_dims, bool) or int(subsample_dims) != subsample_dims or subsample_dims < 1):
        raise ValueError(f"DnC: subsample_dims must be None or an integer >= 1, got {subsample_dims}")
    m = int(math.ceil(ff * int(f)))
    if k < 1 or int(iters) * m >= k:
        raise ValueError(f"DnC needs iters · m < K models: K = {k}, iters = {iters}, m = ceil({filter_frac} · {f}) = {m}")
    return m


def _dnc_keys(n: int, seed: int, round: int, iters: int, subsample_dims):
    """``(all_tiles, keys, thr, forced)`` of :func:`dnc_tiles`, without the masks."""
    tiles = (int(n) + DNC_TILE - 1) // DNC_TILE
    if subsample_dims is None or n <= subsample_dims:
        return True, [0] * iters, _M64, [0] * iters
    thr = min(_M64, (int(subsample_dims) << 64) // int(n))
    kr = splitmix64(splitmix64(int(seed) & _M64) ^ (int(round) & _M64))
    keys = [splitmix64(kr ^ t) for t in range(iters)]
    forced = [splitmix64(kt ^ _M64) % tiles for kt in keys]
    return False, keys, thr, forced


def dnc_tiles(n: int, seed: int, round: int, iters: int, subsample_dims):
    """The coordinate subsample of a DnC call over rows of length ``n``: per iteration t the tiles of
    256 consecutive coordinates that enter the distances. ``T = ceil(n / 256)`` tiles. With
    ``subsample_dims`` None or ``n <= subsample_dims`` every tile is taken and nothing is hashed
    (keys and forced tiles 0, thr 2^64 − 1). Otherwise ``thr = min(2^64 − 1, floor(subsample_dims ·
    2^64 / n))`` (the quotient taken in integers), ``k_r = sm(sm(seed) ^ round)``, ``k_t = sm(k_r ^
    t)`` and tile τ is taken iff ``sm(k_t ^ τ) < thr`` or ``τ == sm(k_t ^ (2^64 − 1)) mod T``: one
    tile is forced, so no iteration is empty. Returns ``(keys [iters], thr, forced [iters], mask
    [iters, T] bool)``."""
    import numpy as np

    tiles = (int(n) + DNC_TILE - 1) // DNC_TILE
    every, keys, thr, forced = _dnc_keys(n, seed, round, iters, subsample_dims)
    mask = np.ones((iters, tiles), dtype=bool)
    if not every:
        with np.errstate(over="ignore"):
            for t in range(iters):
                x = np.arange(tiles, dtype=np.uint64) ^ np.uint64(keys[t])
                x = x + np.uint64(0x9E3779B97F4A7C15)
                x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
                x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
                x = x ^ (x >> np.uint64(31))
                mask[t] = x < np.uint64(thr)
                mask[t, forced[t]] = True
    return keys, thr, forced, mask


def dnc_select(dist, weights, m: int):
    """Steps 1–5 of DnC on squared distances ``dist [iters, K, K]`` (or ``[K, K]``: one iteration),
    in float64 on the host, as ``k_dnc_select`` does them. Per iteration:

    1. screen: row i when more than half of its K − 1 distances are non-finite; then, j ascending,
       an unscreened row j with a non-finite distance to an unscreened row i < j. V: the others.
    2. centre: ``G = −½·J·D_V·J`` (row means, then their mean, then symmetrised); ``K_v <= 1`` or
       ``tr G <= 0``: λ = 0 and every score on V is 0.
    3. ``M = G / tr G``; 20 times ``M <- M·M`` (inner index ascending), ``M <- M / tr M``;
       ``j* = argmax M_jj`` (the lowest on a tie), ``u = M[:, j*] / |M[:, j*]|``, ``λ = uᵀGu``,
       ``s_i = λ·u_i²``; a screened row scores +inf.
    4. the m highest scores are removed, the higher row first among equals; screened rows always.
    5. a row is kept iff every iteration keeps it: ``coef_k = float32(w_k / Σ_kept w)``, 0 for the
       others; nothing kept: ``w / Σ w`` over all rows.

    Returns ``(score [iters, K] float64, lam [iters] float64, removed [K] int32: the first iteration
    that removed the row or −1, coef [K] float32)`` as numpy arrays."""
    import numpy as np

    d_all = np.asarray(dist, dtype=np.float64)
    if d_all.ndim == 2:
        d_all = d_all[None]
    iters, k = d_all.shape[0], d_all.shape[1]
    score = np.zeros((iters, k))
    lam = np.zeros(iters)
    removed = np.full(k, -1, dtype=np.int32)
    with np.errstate(all="ignore"):
        for it in range(iters):
            d = d_all[it]
            fin = np.isfinite(d)
            scr = [2 * sum(1 for b in range(k) if b != a and not fin[a, b]) > k - 1 for a in range(k)]
            for b in range(1, k):
                if not scr[b] and any(not scr[a] and not fin[a, b] for a in range(b)):
                    scr[b] = True
            v = [a for a in range(k) if not scr[a]]
            kv = len(v)
            s = np.zeros(k)
            if kv > 1:
                dv = d[np.ix_(v, v)]
                r = np.array([sum(float(x) for x in row) for row in dv]) / kv
                c = sum(float(x) for x in r) / kv
                a_ = -0.5 * (((dv - r[:, None]) - r[None, :]) + c)
                g = 0.5 * (a_ + a_.T)
                tr = sum(float(g[q, q]) for q in range(kv))
                if tr > 0.0:
                    mm = g / tr
                    for _ in range(DNC_SQUARINGS):
                        acc = np.zeros_like(mm)
                        for q in range(kv):
                            acc = acc + mm[:, q : q + 1] * mm[q : q + 1, :]
                        mm = acc / sum(float(acc[q, q]) for q in range(kv))
                    js = int(np.argmax(np.diag(mm)))
                    col = mm[:, js]
                    u = col / np.sqrt(sum(float(x) * float(x) for x in col))
                    lam[it] = float(u @ (g @ u))
                    s[v] = lam[it] * u * u
            s[[a for a in range(k) if scr[a]]] = np.inf
            score[it] = s
            order = sorted(range(k), key=lambda a: (-s[a], -a))
            for a in range(k):
                if (scr[a] or a in order[: int(m)]) and removed[a] < 0:
                    removed[a] = it
    w = np.array([float(x) for x in weights], dtype=np.float64)
    kept = removed < 0
    coef = np.zeros(k)
    if not kept.any():
        coef = w / w.sum() if w.sum() > 0 else np.full(k, 1.0 / k)
    else:
        ws = float(sum(w[a] for a in range(k) if kept[a]))
        coef[kept] = w[kept] / ws if ws > 0 else 1.0 / int(kept.sum())
    return score, lam, removed, coef.astype(np.float32)


def dnc_into(rows: Sequence[torch.Tensor], outs: Sequence[torch.Tensor], weights: Sequence[float], f: int, filter_frac: float = 1.0, iters: int = 1,
             subsample_dims: Optional[int] = 10000, seed: int = 0, round: int = 0):
    """Divide-and-Conquer (DnC; Shejwalkar & Houmansadr, NDSS 2021) over 1-D fp32 rows with at most
    ``f`` attackers: ``iters`` times, on a fresh subsample of the coordinates (:func:`dnc_tiles`), the
    squared distances from differences, then :func:`dnc_select` — the rows' projections on the top
    singular direction of the centred model matrix, read off the K × K centred Gram matrix
    ``−½·J·D·J``, and the ``m = ceil(filter_frac · f)`` largest removed. ``outs[p] = Σ_k coef[k]·
    rows[k]`` over the rows every iteration kept, ``coef[k] = w_k / Σ_kept w``. ``f == 0`` gives the
    sample-weighted mean. A row with NaN / Inf coordinates spoils only its own distances: it is
    screened and removed. Returns ``(dist [iters, K, K] float64, score [iters, K] float64, lam [iters]
    float64, removed [K] int32, coef [K] float32)`` on the rows' device; ``outs=[]`` gives the
    selection only.

    Deviation from the paper: the subsample is Bernoulli per tile of 256 coordinates (plus one
    forced tile), not exactly ``subsample_dims`` coordinates.

    On the GPU (K <= 16 rows, <= 16 outputs, which may alias the rows) it is three launches —
    ``k_dnc_sqdist<K>``, ``k_dnc_select``, ``k_coef_mean<K>`` — that only enqueue (K == 1: the mean
    alone). Elsewhere: float64 torch math (the oracle)."""
    import numpy as np

    k = len(rows)
    if len(weights) != k:
        raise ValueError(f"{k} rows but {len(weights)} weights")
    m = dnc_check(k, f, filter_frac, iters, subsample_dims)
    iters = int(iters)
    dev = rows[0].device
    n = rows[0].numel()
    if n < 1 or any(t.numel() != n for t in [*rows, *outs]):
        raise ValueError(f"DnC: rows and outputs must share one length >= 1, got {[t.numel() for t in [*rows, *outs]]}")
    if _native_rows(rows, outs):
        lib = _lib()
        every, keys, thr, forced = _dnc_keys(n, seed, round, iters, subsample_dims)
        work = torch.empty(max(1, iters * int(lib.myfyp_krum_grid(n, k)) * (k * (k - 1) // 2)), dtype=torch.float32, device=dev)
        if k == 1:  # no pair, no selection launch: the one row is the result
            dist = torch.zeros(iters, 1, 1, dtype=torch.float64, device=dev)
            score = torch.zeros(iters, 1, dtype=torch.float64, device=dev)
            lam = torch.zeros(iters, dtype=torch.float64, device=dev)
            removed = torch.full((1,), -1, dtype=torch.int32, device=dev)
            coef = torch.ones(1, dtype=torch.float32, device=dev)
        else:
            dist = torch.empty(iters, k, k, dtype=torch.float64, device=dev)
            score = torch.empty(iters, k, dtype=torch.float64, device=dev)
            lam = torch.empty(iters, dtype=torch.float64, device=dev)
            removed = torch.empty(k, dtype=torch.int32, device=dev)
            coef = torch.empty(k, dtype=torch.float32, device=dev)
        src, keep_s = _host_ptrs(rows)
        dst, keep_d = _host_ptrs(outs)
        w = (ctypes.c_float * k)(*[float(x) for x in weights])
        ka = (ctypes.c_uint64 * iters)(*keys)
        fa = (ctypes.c_uint64 * iters)(*forced)
        _native.check(lib.myfyp_dnc_multi(dst, len(outs), src, ctypes.cast(w, ctypes.c_void_p), k, m, iters, ctypes.cast(ka, ctypes.c_void_p), thr,
                                          ctypes.cast(fa, ctypes.c_void_p), int(every), n, work.data_ptr(), dist.data_ptr(), score.data_ptr(),
                                          lam.data_ptr(), removed.data_ptr(), coef.data_ptr(), _stream()), "dnc_multi")
        return dist, score, lam, removed, coef
    _, _, _, mask = dnc_tiles(n, seed, round, iters, subsample_dims)
    x = torch.stack([r.detach().double().reshape(-1) for r in rows])
    dist = torch.zeros(iters, k, k, dtype=torch.float64)
    for t in range(iters):
        take = torch.from_numpy(np.repeat(mask[t], DNC_TILE)[:n]).to(x.device)
        xt = x[:, take]
        for i in range(k):
            for j in range(i + 1, k):
                dist[t, i, j] = dist[t, j, i] = float((xt[i] - xt[j]).square().sum())
    score, lam, removed, coef = dnc_select(dist.numpy(), weights, m)
    if outs:
        mean = torch.zeros(n, dtype=torch.float64, device=x.device)
        for i in range(k):
            if coef[i] != 0:
                mean += float(coef[i]) * x[i]
        for o in outs:
            o.copy_(mean.view_as(o))
    return (dist.to(dev), torch.from_numpy(score).to(dev), torch.from_numpy(lam).to(dev), torch.from_numpy(removed).to(dev),
            torch.from_numpy(coef).to(dev))


GEOMED_MAX_ITERS = 32


def geometric_median_into(rows: Sequence[torch.Tensor], outs: Sequence[torch.Tensor], weights: Sequence[float], iters: int = 3, nu: float = 1e-6):
    """Geometric median (RFA: Pillutla et al., 2019) of 1-D fp32 rows by ``iters`` smoothed
    Weiszfeld steps; ``outs[p] = Σ_k coef[k]·rows[k]``. Coefficients are float32 after every step.

    Screen: a row whose ``Σ x²`` is not a finite float32 (NaN, Inf, overflow) is invalid for the
    call; ``ŵ_k = w_k`` for valid rows (1 where every valid weight is 0), 0 otherwise;
    ``c = ŵ/Σŵ``. With no valid row ``c = w/Σw`` (or ``1/K``), no step runs, ``dist`` is NaN and
    the output is the plain mean. Step t: ``r`` the lowest row with ``c_r != 0``,
    ``z = x_r + Σ_j c_j (x_j − x_r)`` over the rows of coefficient != 0, ``d_k = ‖x_k − z‖``,
    ``objective[t] = Σ ŵ_k d_k`` over ``ŵ_k != 0``, ``β_k = ŵ_k / max(nu, d_k)`` (0 where ``d_k``
    is not finite), ``c = β/Σβ`` (kept where ``Σβ`` is 0 or not finite). Returns ``(coef [K]
    float32, dist [K] float64: the last step's d, objective [iters] float64)`` on the rows' device;
    ``outs=[]`` gives the weights only.

    On the GPU (K <= 16 rows, <= 16 outputs, which may alias the rows) it is ``2(iters + 1) + 1``
    launches — ``k_gm_dist<K>`` and ``k_gm_reweight`` for the screen and per step, then
    ``k_coef_mean<K>`` — that only enqueue. Elsewhere: float64 torch math (the oracle)."""
    k = len(rows)
    iters = int(iters)
    nu = float(nu)
    if len(weights) != k:
        raise ValueError(f"{k} rows but {len(weights)} weights")
    if k < 1:
        raise ValueError("geometric median of no rows")
    if not 1 <= iters <= GEOMED_MAX_ITERS:
        raise ValueError(f"iters must be in 1..{GEOMED_MAX_ITERS}, got {iters}")
    if not (nu > 0 and nu != float("inf")):
        raise ValueError(f"nu must be finite and > 0, got {nu}")
    ws = [float(x) for x in weights]
    if not all(0 <= x < float("inf") for x in ws):
        raise ValueError("weights must be finite and >= 0")
    dev = rows[0].device
    if _native_rows(rows, outs):
        lib = _lib()
        n = rows[0].numel()
        work = torch.empty(int(lib.myfyp_geomed_work(n, k)), dtype=torch.float32, device=dev)
        coef = torch.empty(k, dtype=torch.float32, device=dev)
        dist = torch.empty(k, dtype=torch.float64, device=dev)
        obj = torch.empty(iters, dtype=torch.float64, device=dev)
        src, keep_s = _host_ptrs(rows)
        dst, keep_d = _host_ptrs(outs)
        w = (ctypes.c_float * k)(*ws)
        _native.check(lib.myfyp_geomed_multi(dst, len(outs), src, ctypes.cast(w, ctypes.c_void_p), k, iters, nu, n, work.data_ptr(), coef.data_ptr(),
                                             dist.data_ptr(), obj.data_ptr(), _stream()), "geomed_multi")
        return coef, dist, obj
    x = [r.double().reshape(-1) for r in rows]
    w = torch.tensor(ws, dtype=torch.float64)
    valid = torch.isfinite(torch.stack([xi.square().sum() for xi in x]).float().cpu())
    dist = torch.full((k,), float("nan"), dtype=torch.float64)
    obj = torch.zeros(iters, dtype=torch.float64)
    if not bool(valid.any()):
        coef = (w / w.sum() if float(w.sum()) > 0 else torch.full((k,), 1.0 / k, dtype=torch.float64)).float()
        iters = 0
    else:
        what = torch.where(valid, w, torch.zeros_like(w))
        if float(what.sum()) == 0:
            what = valid.double()
        coef = (what / what.sum()).float()
    for t in range(iters):
        c = coef.double().tolist()
        nz = [j for j in range(k) if c[j] != 0]
        xr = x[nz[0]]
        m = torch.zeros_like(xr)
        for j in nz:
            m += c[j] * (x[j] - xr)
        dist = torch.stack([((xi - xr) - m).square().sum().sqrt() for xi in x]).cpu()
        live = what != 0
        obj[t] = (what[live] * dist[live]).sum()
        beta = torch.where(torch.isfinite(dist), what / dist.clamp(min=nu), torch.zeros_like(what))
        bs = float(beta.sum())
        if bs > 0 and bs != float("inf"):
            coef = (beta / bs).float()
    if outs:
        c = coef.double().tolist()
        mean = torch.zeros_like(x[0])
        for j in range(k):
            if c[j] != 0:
                mean += c[j] * x[j]
        for o in outs:
            o.copy_(mean)
    return coef.to(dev), dist.to(dev), obj.to(dev)


COLLUDE_KINDS = ("alie", "ipm", "min_max", "min_sum")


def alie_z(k: int, f: int) -> float:
    """ALIE's default z for ``k`` peers of which ``f`` attack (Baruch et al., 2019):
    ``Φ⁻¹((k − f − s) / (k − f))`` with ``s = ⌊k/2 + 1⌋ − f`` the honest peers the attackers must
    win over; 0 where that fraction is not inside (0, 1)."""
    from statistics import NormalDist

    k, f = int(k), int(f)
    s = k // 2 + 1 - f
    if k - f <= 0:
        return 0.0
    p = (k - f - s) / (k - f)
    return float(NormalDist().inv_cdf(p)) if 0.0 < p < 1.0 else 0.0


def collude_into(rows: Sequence[torch.Tensor], outs: Sequence[torch.Tensor], kind: str, z: Optional[float] = None, eps: float = 0.5,
                 ref: Optional[torch.Tensor] = None):
    """A colluding, omniscient attack: the crafted row ``m`` of the honest 1-D fp32 ``rows``, stored
    into every one of ``outs`` (the attackers' rows). With μ and σ the per-coordinate mean and
    population standard deviation of the H honest values:

    * ``alie``    — ``m = μ − z·σ``; ``z`` defaults to :func:`alie_z` of ``(H + len(outs), len(outs))``
    * ``ipm``     — ``m = ref − eps·(μ − ref)``, ``ref`` the model the round started from
    * ``min_max`` — ``m = μ − γ·σ`` with the largest γ >= 0 for which ``max_i ‖m − x_i‖² <= D``,
      ``D = max_ij ‖x_i − x_j‖²``: ``γ = min_i (b_i + sqrt(max(0, b_i² + s·(D − a_i)))) / s``
    * ``min_sum`` — the same with ``Σ_i ‖m − x_i‖² <= S``, ``S = max_i Σ_j ‖x_i − x_j‖²``:
      ``γ = sqrt(max(0, S/(H·s) − 1))``

    where ``a_i = ‖μ − x_i‖²``, ``b_i = ⟨μ − x_i, σ⟩`` and ``s = ‖σ‖²``; ``s = 0`` gives γ = 0. There
    is no NaN screening. Returns ``(gamma [1] float32: γ, ALIE's z or IPM's eps; stat [2H + 3]
    float64: a, b, s, D, S for min_max / min_sum, zeros otherwise)`` on the rows' device.

    On the GPU (H <= 16 rows, <= 16 outputs) it is one launch for ``alie`` / ``ipm``
    (``k_collude_write<H>``) and four for ``min_max`` / ``min_sum`` (``k_pairwise_sqdist<H>``,
    ``k_collude_stats<H>``, ``k_collude_solve``, ``k_collude_write<H>``) that only enqueue: γ never
    leaves the device. Elsewhere: float64 torch math (the oracle)."""
    if kind not in COLLUDE_KINDS:
        raise ValueError(f"unknown colluding attack {kind!r}; choose from {COLLUDE_KINDS}")
    h = len(rows)
    if h < 1:
        raise ValueError("a colluding attack needs at least one honest row")
    if not outs:
        raise ValueError("a colluding attack needs at least one output row")
    if kind == "ipm" and ref is None:
        raise ValueError("ipm needs ref, the model the round started from")
    n = rows[0].numel()
    if n < 1 or any(t.numel() != n for t in [*rows, *outs]) or (ref is not None and ref.numel() != n):
        raise ValueError("colluding attack: rows, outputs and ref must share one length >= 1")
    row_ptrs = {t.data_ptr() for t in rows}
    if any(o.data_ptr() in row_ptrs for o in outs):
        raise ValueError("colluding attack: an output is also an honest row")
    dev = rows[0].device
    zz = float(alie_z(h + len(outs), len(outs)) if z is None else z)
    eps = float(eps)
    ca, cb, cr = {"alie": (1.0, -zz, 0.0), "ipm": (-eps, 0.0, 1.0 + eps)}.get(kind, (1.0, 0.0, 0.0))
    if _native_rows(rows, outs) and (ref is None or (ref.device == dev and ref.is_contiguous() and ref.dtype == torch.float32)):
        lib = _lib()
        solve = kind in ("min_max", "min_sum")
        work = torch.empty(max(1, int(lib.myfyp_collude_work(n, h))), dtype=torch.float32, device=dev) if solve else None
        gamma = torch.empty(1, dtype=torch.float32, device=dev)
        stat = torch.empty(2 * h + 3, dtype=torch.float64, device=dev) if solve else torch.zeros(2 * h + 3, dtype=torch.float64, device=dev)
        src, keep_s = _host_ptrs(rows)
        dst, keep_d = _host_ptrs(outs)
        _native.check(lib.myfyp_collude_multi(dst, len(outs), src, h, COLLUDE_KINDS.index(kind), ca, cb, cr, _ptr(ref if kind == "ipm" else None), n,
                                              _ptr(work), gamma.data_ptr(), stat.data_ptr(), _stream()), "collude_multi")
        return gamma, stat
    x = torch.stack([r.detach().double().reshape(-1) for r in rows])
    mu = x.mean(dim=0)
    sigma = ((x - mu).square().sum(dim=0) / h).sqrt()
    stat = torch.zeros(2 * h + 3, dtype=torch.float64)
    if kind == "alie":
        g, m = zz, mu - zz * sigma
    elif kind == "ipm":
        r = ref.detach().double().reshape(-1)
        g, m = eps, r - eps * (mu - r)
    else:
        a = (mu - x).square().sum(dim=1)
        b = ((mu - x) * sigma).sum(dim=1)
        s = float(sigma.square().sum())
        d = torch.zeros(h, h, dtype=torch.float64)
        for i in range(h):
            for j in range(i + 1, h):
                d[i, j] = d[j, i] = float((x[i] - x[j]).square().sum())
        big_d, big_s = float(d.max()), float(d.sum(dim=1).max())
        g = 0.0
        if s > 0:
            if kind == "min_max":
                g = max(0.0, min((float(b[i]) + max(0.0, float(b[i]) ** 2 + s * (big_d - float(a[i]))) ** 0.5) / s for i in range(h)))
            else:
                g = max(0.0, big_s / (h * s) - 1.0) ** 0.5
        m = mu - g * sigma
        stat[:h], stat[h : 2 * h], stat[2 * h], stat[2 * h + 1], stat[2 * h + 2] = a.cpu(), b.cpu(), s, big_d, big_s
    with torch.no_grad():
        for o in outs:
            o.copy_(m.view_as(o))
    return torch.tensor([g], dtype=torch.float32, device=dev), stat.to(dev)


def scaffold_reduce(buf: torch.Tensor, dys: Sequence[torch.Tensor], dcs: Sequence[torch.Tensor], weights: Sequence[float]) -> None:
    """``buf = [Σ w_k Δy_k | Σ w_k | Σ Δc_k | K]`` (2n + 2 floats) from the local contributors."""
    n = (buf.numel() - 2) // 2
    k = len(dys)
    if buf.device.type == "cuda" and k <= 16:
        y, keep_y = _host_ptrs(dys)
        c, keep_c = _host_ptrs(dcs)
        w = (ctypes.c_float * max(1, k))(*weights)
        _native.check(_lib().myfyp_scaffold_reduce(buf.data_ptr(), y, c, ctypes.cast(w, ctypes.c_void_p), k, n, _stream()), "scaffold_reduce")
        return
    buf.zero_()
    for dy, dc, wt in zip(dys, dcs, weights):
        buf[:n].add_(dy, alpha=wt)
        buf[n + 1 : 2 * n + 1].add_(dc)
    buf[n] = float(sum(weights))
    buf[2 * n + 1] = float(k)


def scaffold_apply(outs: Sequence[torch.Tensor], x_start: torch.Tensor, buf: torch.Tensor, c: torch.Tensor, c_init: bool, global_lr: float) -> None:
    """``outs[p] = x_start + η_g · buf[:n] / buf[n]``; ``c = (0 if c_init else c) + buf[n+1:2n+1] / buf[2n+1]``."""
    n = x_start.numel()
    if buf.device.type == "cuda" and len(outs) <= 16:
        o, keep = _host_ptrs(outs)
        _native.check(_lib().myfyp_scaffold_apply(o, len(outs), x_start.data_ptr(), buf.data_ptr(), c.data_ptr(), int(c_init), float(global_lr), n, _stream()),
                      "scaffold_apply")
        return
    x_new = torch.addcmul(x_start, buf[:n], global_lr / buf[n : n + 1].clamp_min(1e-12))
    dc = buf[n + 1 : 2 * n + 1] / buf[2 * n + 1 : 2 * n + 2].clamp_min(1.0)
    if c_init:
        c.copy_(dc)
    else:
        c.add_(dc)
    for t in outs:
        t.copy_(x_new)


# ---------------------------------------------------------------------------------------------
# optimizers (flat fp32 buffers)
# ---------------------------------------------------------------------------------------------
def _corrected_grad(param, grad, anchor, mu):
    """FedProx's proximal gradient term (SCAFFOLD is applied in the update space: _scaffold_step)."""
    g = grad
    if anchor is not None and mu != 0.0:
        g = g + mu * (param - anchor)
    return g


def _scaffold_step(param, c_global, c_local, lr: float) -> None:
    """SCAFFOLD correction in the update space: ``w -= lr·(c − c_i)`` after the optimizer step
    (``opt_update`` in ``csrc/kernels/common.h`` explains why not in Adam's gradient)."""
    if c_global is not None and c_local is not None:
        param.sub_(c_global - c_local, alpha=lr)


def adam_step(
    param: torch.Tensor,
    grad: torch.Tensor,
    exp_avg: torch.Tensor,
    exp_avg_sq: torch.Tensor,
    step: int,
    lr: float = 1e-3,
    beta1: float = 0.9,
    beta2: float = 0.999,
    eps: float = 1e-8,
    weight_decay: float = 0.0,
    shadow: Optional[torch.Tensor] = None,
    anchor: Optional[torch.Tensor] = None,
    c_global: Optional[torch.Tensor] = None,
    c_local: Optional[torch.Tensor] = None,
    mu: float = 0.0,
) -> None:
    """One Adam step (torch.optim.Adam semantics, L2 ``weight_decay``), in place, step ≥ 1."""
    if param.device.type != "cuda":
        g = _corrected_grad(param, grad, anchor, mu)
        if weight_decay:
            g = g + weight_decay * param
        exp_avg.mul_(beta1).add_(g, alpha=1 - beta1)
        exp_avg_sq.mul_(beta2).addcmul_(g, g, value=1 - beta2)
        bc1 = 1 - beta1**step
        bc2 = 1 - beta2**step
        denom = (exp_avg_sq / bc2).sqrt_().add_(eps)
        param.addcdiv_(exp_avg, denom, value=-lr / bc1)
        _scaffold_step(param, c_global, c_local, lr)
        if shadow is not None:
            shadow.copy_(param.to(shadow.dtype))
        return
    lib = _lib()
    _native.check(
        lib.myfyp_adam_step(
            param.data_ptr(), grad.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), _ptr(shadow), param.numel(),
            lr, beta1, beta2, eps, weight_decay, int(step), _ptr(anchor), _ptr(c_global), _ptr(c_local), float(mu), _stream(),
        ),
        "adam_step",
    )


def sgd_step(
    param: torch.Tensor,
    grad: torch.Tensor,
    momentum_buf: Optional[torch.Tensor],
    lr: float,
    momentum: float = 0.0,
    weight_decay: float = 0.0,
    nesterov: bool = False,
    anchor: Optional[torch.Tensor] = None,
    c_global: Optional[torch.Tensor] = None,
    c_local: Optional[torch.Tensor] = None,
    mu: float = 0.0,
) -> None:
    """One SGD(+momentum, +nesterov) step (torch.optim.SGD semantics; buffer starts at 0)."""
    if param.device.type != "cuda":
        g = _corrected_grad(param, grad, anchor, mu)
        if weight_decay:
            g = g + weight_decay * param
        if momentum != 0.0 and momentum_buf is not None:
            momentum_buf.mul_(momentum).add_(g)
            g = g + momentum * momentum_buf if nesterov else momentum_buf
        param.add_(g, alpha=-lr)
        _scaffold_step(param, c_global, c_local, lr)
        return
    lib = _lib()
    _native.check(
        lib.myfyp_sgd_step(
            param.data_ptr(), grad.data_ptr(), _ptr(momentum_buf), param.numel(), lr, momentum, weight_decay, int(nesterov),
            _ptr(anchor), _ptr(c_global), _ptr(c_local), float(mu), _stream(),
        ),
        "sgd_step",
    )


def scale_add_noise(t: torch.Tensor, scale: float, sigma: float, seed: int = 0) -> None:
    """``t = scale·t + σ·N(0,1)`` in place (sign flip: scale=-1, σ=0)."""
    if t.device.type != "cuda" or t.dtype != torch.float32 or not t.is_contiguous():
        g = torch.Generator(device="cpu").manual_seed(seed)
        noise = torch.randn(t.shape, generator=g, dtype=torch.float32).to(t.device, t.dtype) if sigma else 0.0
        t.mul_(scale).add_(noise * sigma if sigma else 0.0)
        return
    lib = _lib()
    _native.check(lib.myfyp_scale_add_noise(t.data_ptr(), t.numel(), float(scale), float(sigma), int(seed), _stream()), "scale_add_noise")
