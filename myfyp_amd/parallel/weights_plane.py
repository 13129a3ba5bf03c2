"""Round-level weight collectives executed by a local gang leader (see ``federation.py``).

All functions receive ``arrived: {addr: payload}`` for the co-located peers that reached the gang
and run identically on every rank (same call order ⇒ matching RCCL collectives).
"""

from __future__ import annotations

import os
import time
from typing import Any, Dict, List, Optional, Tuple

import numpy as np
import torch

from myfyp_amd import ops
from myfyp_amd.management.tracing import mark, traced
from myfyp_amd.parallel.federation import Federation


# ---------------------------------------------------------------------------------------------
# learner state access
# ---------------------------------------------------------------------------------------------
def state_tensors(learner) -> List[torch.Tensor]:
    """Device tensors that define a peer's model: flat trainable vector + floating buffers."""
    out = [learner.flat_params()]
    module = learner.model.get_model()
    for b in module.buffers():
        if b.is_floating_point():
            out.append(b)
    return out


def on_device(dev: torch.device):
    """Make ``dev`` the thread's current GPU (no-op for CPU members)."""
    import contextlib

    return torch.cuda.device(dev) if dev.type == "cuda" else contextlib.nullcontext()


def mesh_rank_of(learner) -> int:
    r = getattr(learner, "mesh_rank", None)
    return 0 if r is None else int(r)


def _by_mesh_rank(fed: Federation, addrs, learners) -> Dict[int, List[Tuple[str, Any]]]:
    out: Dict[int, List[Tuple[str, Any]]] = {r: [] for r in fed.mesh_members}
    for a, lr in zip(addrs, learners):
        r = mesh_rank_of(lr)
        if r not in out:
            raise RuntimeError(f"peer {a} sits on mesh rank {r}, which left the mesh")
        out[r].append((a, lr))
    return out


def _stacked_group(learners) -> Optional[Any]:
    """Return the shared MLPGroup when every learner is a row of one stacked buffer."""
    groups = {id(getattr(lr, "_engine", None) and lr._engine.group) for lr in learners}
    if len(groups) != 1 or getattr(learners[0], "_engine", None) is None:
        return None
    return learners[0]._engine.group


# ---------------------------------------------------------------------------------------------
# initial model (reference: init_model gossip, start_learning_stage.py:82-112)
# ---------------------------------------------------------------------------------------------
def sync_initial_model(fed: Federation, arrived: Dict[str, Any], initiator: str) -> None:
    """Every peer adopts the initiator's weights: local copy + one RCCL broadcast per dtype (the
    state tensors are packed into one flat buffer each, so ResNet-18's ~100 tensors cost one
    guarded broadcast and one agreement gather, not one per tensor: ADVICE r3)."""
    learners = {a: fed.local_nodes[a].learner for a in arrived if a in fed.local_nodes}
    if fed.mesh is not None:
        _mesh_initial_model(fed, learners, initiator)
        return

    def run() -> None:
        # the initiator's rank, or (if it died) the lowest survivor: every survivor agrees on it
        src_rank = fed.peers.get(initiator, min(fed.members))
        if src_rank not in fed.members:
            src_rank = min(fed.members)
        ref_addr = initiator if initiator in learners else next(iter(learners))
        src = state_tensors(learners[ref_addr])
        groups: Dict[Any, List[int]] = {}
        for i, t in enumerate(src):
            groups.setdefault((t.dtype, t.device), []).append(i)
        bufs: List[Any] = [None] * len(src)
        for idx in groups.values():
            flat = torch.cat([src[i].detach().reshape(-1) for i in idx])
            fed.broadcast_(flat, src_rank)
            for i, part in zip(idx, torch.split(flat, [src[i].numel() for i in idx])):
                bufs[i] = part.view_as(src[i])
        with torch.no_grad():
            for a, lr in learners.items():
                for dst, s in zip(state_tensors(lr), bufs):
                    dst.copy_(s)

    fed.run_aggregation(run)


def _mesh_initial_model(fed: Federation, learners: Dict[str, Any], initiator: str) -> None:
    """Device mesh: pack the initiator's state tensors per dtype on its device, ONE RCCL broadcast
    per dtype from its mesh rank, unpack into every peer of every device."""
    ref_addr = initiator if initiator in learners else next(iter(learners))
    root_r = mesh_rank_of(learners[ref_addr])
    root = fed.mesh_position(root_r)
    src = state_tensors(learners[ref_addr])
    groups: Dict[Any, List[int]] = {}
    for i, t in enumerate(src):
        groups.setdefault(t.dtype, []).append(i)
    per_rank: Dict[int, List[Any]] = {r: [None] * len(src) for r in fed.mesh_members}
    for dt, idx in groups.items():
        numel = sum(src[i].numel() for i in idx)
        flats = []
        for r in fed.mesh_members:
            dev = fed.devices[r]
            if r == root_r:
                flats.append(torch.cat([src[i].detach().reshape(-1) for i in idx]).to(dev))
            else:
                flats.append(torch.empty(numel, dtype=dt, device=dev))
        fed.mesh.broadcast_(flats, root)
        fed.mesh_track("broadcast")
        for r, flat in zip(fed.mesh_members, flats):
            for i, part in zip(idx, torch.split(flat, [src[i].numel() for i in idx])):
                per_rank[r][i] = part.view_as(src[i])
    with torch.no_grad():
        for a, lr in learners.items():
            r = mesh_rank_of(lr)
            with on_device(fed.devices[r]):
                for dst, s_ in zip(state_tensors(lr), per_rank[r]):
                    dst.copy_(s_)


# ---------------------------------------------------------------------------------------------
# votes
# ---------------------------------------------------------------------------------------------
def gather_votes(fed: Federation, arrived: Dict[str, Dict[str, int]]) -> Dict[str, Dict[str, int]]:
    allv: Dict[str, Dict[str, int]] = {}
    for part in fed.all_gather_object(dict(arrived)):
        allv.update(part)
    return allv


# ---------------------------------------------------------------------------------------------
# aggregation
# ---------------------------------------------------------------------------------------------
_COMM_STREAMS: Dict[int, "torch.cuda.Stream"] = {}


def comm_stream(dev: torch.device) -> "torch.cuda.Stream":
    """The side HIP stream that carries the weight collectives of ``dev`` (one per device)."""
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    st = _COMM_STREAMS.get(idx)
    if st is None:
        st = _COMM_STREAMS[idx] = torch.cuda.Stream(device=idx)
    return st


def bucket_ranges(n: int, bucket_bytes: int) -> List[Tuple[int, int]]:
    """[b0, b1) ranges over n floats; every b0 is a multiple of 4 (float4 kernels stay aligned)."""
    step = max(4, (bucket_bytes // 4) // 4 * 4)
    return [(b0, min(n, b0 + step)) for b0 in range(0, n, step)] or [(0, 0)]


class _Delayed:
    """Delayed-averaging state of one stacked group or of the generic per-learner path."""

    def __init__(self) -> None:
        self.snap: Optional[torch.Tensor] = None  # round-r local rows (stacked: [capacity, n])
        self.snaps: Dict[str, torch.Tensor] = {}  # generic path: addr -> packed row
        self.buf: Optional[torch.Tensor] = None  # [wsum, pad x3 | Σ w x_r] (stacked) / [Σ w x_r | Σ w] (generic)
        self.done = None  # event on the side stream: the round-r all-reduce has landed in buf
        self.pending = False


def _delayed_state(fed: Federation, key) -> _Delayed:
    table = fed.__dict__.setdefault("_delayed", {})
    st = table.get(key)
    if st is None:
        st = table[key] = _Delayed()
    return st


def _stacked_mean_cuda(fed: Federation, group, w: np.ndarray, mask: np.ndarray, final: bool) -> None:
    """FedAvg of a stacked ``[capacity, S]`` group on the GPU, host never waits.

    * one rank: one ``k_fedavg_local`` launch (weighted mean written into every masked row);
    * several ranks, ``OVERLAP_COLLECTIVES``: per bucket a reduce launch (which also writes the
      failover's retained copy) and an async all-reduce on RCCL's stream, ordered after that launch,
      then per bucket wait + apply launch — bucket k's all-reduce overlaps bucket k+1's reduce and
      bucket k-1's apply. These run on the compute stream itself: the next epoch needs the average,
      and a side stream only put two more cross-stream hops on the round's critical path
      (``profiles/r6k_forced_trace``);
    * ``DELAYED_AVERAGING`` (opt-in, not on the last round): land the previous round's average as
      ``x += avg - snap`` and take the new snapshot (one launch), then reduce + all-reduce the
      snapshot on the side stream while the next round trains from the local weights.
    """
    from myfyp_amd.settings import Settings

    fast = ops.fast_lib()
    n, P, S = group.numel, group.capacity, group.S
    dev = group.params.device
    cur = torch.cuda.current_stream(dev)
    wp, mp = w.ctypes.data, mask.ctypes.data
    base = group.params.data_ptr()
    delayed = bool(Settings.DELAYED_AVERAGING)
    st = _delayed_state(fed, id(group)) if (delayed or getattr(fed, "_delayed", {}).get(id(group))) else None
    landed = False
    if st is not None and st.pending:  # land round r-1's average (and re-snapshot) in one launch
        cur.wait_event(st.done)
        ops.check(fast.myfyp_fedavg_delayed_land(base, st.snap.data_ptr(), n, st.buf.data_ptr() + 16, st.buf.data_ptr(), P, n, S, mp, cur.cuda_stream),
                  "fedavg_delayed_land")
        st.pending, landed = False, True
    if delayed and not final:
        if st.snap is None or tuple(st.snap.shape) != (P, n):
            # zeros: rows of unused capacity slots are read (with weight 0) by the reduce
            st.snap = torch.zeros(P, n, dtype=torch.float32, device=dev)
            st.buf = torch.zeros(n + 4, dtype=torch.float32, device=dev)
            landed = False
        if not landed:  # first delayed round: snapshot only
            ops.check(fast.myfyp_fedavg_delayed_land(base, st.snap.data_ptr(), n, None, None, P, n, S, mp, cur.cuda_stream), "fedavg_snapshot")
        snap_ptr, sbuf = st.snap.data_ptr(), st.buf
        works = _bucketed_reduce(fed, fast, comm_stream(dev), cur, snap_ptr, n, n, P, wp, sbuf, apply=None)
        st.done = torch.cuda.Event()
        st.done.record(comm_stream(dev))
        st.pending = True

        def retry() -> None:  # the snapshot rows are intact: reduce them again over the survivors
            c = torch.cuda.current_stream(dev)
            # the failed bucketed reduce / all-reduce wrote sbuf on the comm stream
            c.wait_stream(comm_stream(dev))
            ops.check(fast.myfyp_fedavg_bucket_reduce(sbuf.data_ptr() + 16, sbuf.data_ptr(), snap_ptr, P, n, n, w.ctypes.data, c.cuda_stream),
                      "fedavg_bucket_reduce")
            fed.all_reduce_(sbuf)
            st.done = torch.cuda.Event()
            st.done.record(c)

        fed.defer_confirm(works, retry)
        return
    if fed.solo:  # nothing to all-reduce: weighted mean and write-back in one launch
        mark("agg:launch")
        ops.check(fast.myfyp_fedavg_stacked_local(base, P, n, S, wp, mp, cur.cuda_stream), "fedavg_local")
        mark("agg:launched")
        return
    if not Settings.OVERLAP_COLLECTIVES:
        buf = group.fedavg_buffer()
        ops.check(fast.myfyp_fedavg_stacked_reduce(buf.data_ptr(), base, P, n, S, wp, cur.cuda_stream), "fedavg_reduce")
        fed.all_reduce_(buf)
        ops.check(fast.myfyp_fedavg_stacked_apply(base, buf.data_ptr(), P, n, S, mp, cur.cuda_stream), "fedavg_apply")
        return
    buf = getattr(group, "_wp_bucket_buf", None)
    if buf is None or buf.numel() != n + 4:
        buf = group._wp_bucket_buf = torch.zeros(n + 4, dtype=torch.float32, device=dev)
    keep = None
    if fed._guarded():  # retained local partial sums: a failed all-reduce is re-run from them
        keep = getattr(group, "_wp_keep_buf", None)
        if keep is None or keep.numel() != n + 4:
            keep = group._wp_keep_buf = torch.zeros(n + 4, dtype=torch.float32, device=dev)
    # on the compute stream: the next epoch needs the average anyway, and the buckets still pipeline
    # (bucket k's all-reduce runs on RCCL's stream while bucket k + 1 reduces); a side stream only
    # added two cross-stream hops to the round's critical path (profiles/r6k_forced_trace)
    side = os.environ.get("MYFYP_FEDAVG_SIDE", "0") == "1"  # A/B: the side-stream pipeline of round 5
    works = _bucketed_reduce(fed, fast, comm_stream(dev) if side else cur, cur, base, S, n, P, wp, buf, apply=(base, S, mp), keep=keep)
    if keep is not None:

        def retry() -> None:  # survivors: all-reduce the retained local partials, apply again
            c = torch.cuda.current_stream(dev)
            c.wait_stream(comm_stream(dev))
            buf.copy_(keep)
            fed.all_reduce_(buf)
            ops.check(fast.myfyp_fedavg_bucket_apply(base, buf.data_ptr() + 16, buf.data_ptr(), P, n, S, mask.ctypes.data, c.cuda_stream),
                      "fedavg_bucket_apply")

        fed.defer_confirm(works, retry)


def _bucketed_reduce(fed: Federation, fast, cs, cur, src: int, ld: int, n: int, P: int, wp: int, buf: torch.Tensor, apply, keep=None) -> list:
    """Side-stream pipeline over ``bucket_ranges``: reduce launch + async all-reduce per bucket,
    then (``apply`` = (dst, ld, mask)) per bucket wait + apply launch. ``buf`` = [wsum, pad x3 | data];
    bucket 0's all-reduce carries the weight sum, so apply k needs only buckets 0 and k. ``keep``
    (failover) receives a copy of each bucket's local partial sum before its all-reduce. Returns
    the all-reduce works (confirmed later by the collective guard)."""
    from myfyp_amd.settings import Settings

    same = cs.cuda_stream == cur.cuda_stream  # critical path: everything on the compute stream
    if not same:
        cs.wait_stream(cur)  # the rows are final on the compute stream
    bp = buf.data_ptr()
    kp = keep.data_ptr() if keep is not None else None
    ranges = bucket_ranges(n, Settings.BUCKET_BYTES)
    works = []
    timed = fed.comm.timed("fedavg_pipeline")
    ev0, ev1 = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) if timed else (None, None)
    if timed:
        ev0.record(cs)
    with torch.cuda.stream(cs):
        for k, (b0, b1) in enumerate(ranges):
            if kp is None:
                ops.check(fast.myfyp_fedavg_bucket_reduce(bp + 4 * (4 + b0), bp if k == 0 else None, src + 4 * b0, P, b1 - b0, ld, wp, cs.cuda_stream),
                          "fedavg_bucket_reduce")
            else:  # the retained copy from the same pass (no device copy behind it)
                ops.check(fast.myfyp_fedavg_bucket_reduce2(bp + 4 * (4 + b0), bp if k == 0 else None, kp + 4 * (4 + b0), kp if k == 0 else None,
                                                           src + 4 * b0, P, b1 - b0, ld, wp, cs.cuda_stream), "fedavg_bucket_reduce2")
            lo = 0 if k == 0 else 4 + b0
            works.append(fed.all_reduce_async(buf[lo : 4 + b1]))
        for k, (b0, b1) in enumerate(ranges):
            if works[k] is not None:
                works[k].wait()
            if apply is not None:
                dst, dld, mp = apply
                ops.check(fast.myfyp_fedavg_bucket_apply(dst + 4 * b0, bp + 4 * (4 + b0), bp, P, b1 - b0, dld, mp, cs.cuda_stream), "fedavg_bucket_apply")
    if timed:
        ev1.record(cs)
    fed.comm.device("fedavg_pipeline", 4 * (n + 1), ev0, ev1)  # resolved lazily by the node monitor (sampled timing)
    if not same:
        buf.record_stream(cs)
        if keep is not None:
            keep.record_stream(cs)
        if apply is not None:
            cur.wait_stream(cs)  # stream-level: the next kernel on the compute stream sees the average
    return works


@traced("aggregate_mean")
def aggregate_mean(fed: Federation, arrived: Dict[str, Tuple[float, Any]], final: bool = True) -> Tuple[float, List[str]]:
    """Sample-weighted mean of the trainers' models (weight 0 for non-trainers), result into every
    local peer. Stacked groups on the GPU: see ``_stacked_mean_cuda`` (side-stream bucketed
    pipeline, optional delayed averaging). ``final`` marks the experiment's last round (delayed
    averaging flushes and aggregates exactly there)."""
    from myfyp_amd.settings import Settings

    t0 = time.perf_counter()

    def run() -> Tuple[float, List[str]]:
        mark("agg:run")
        addrs = [a for a in arrived if a in fed.local_nodes]  # a peer may die after arriving
        learners = [fed.local_nodes[a].learner for a in addrs]
        weights = [float(arrived[a][0]) for a in addrs]
        contributors = [a for a, w in zip(addrs, weights) if w > 0]
        if fed.mesh is not None:
            mut = _MeshMutation(fed, addrs)
            out = _mesh_mean(fed, addrs, learners, weights, final)
            if mut.before:
                mut.apply()
            return out, contributors
        group = _stacked_group(learners)
        dev = learners[0].flat_params().device
        if group is not None and dev.type == "cuda":
            w = np.zeros(group.capacity, dtype=np.float32)
            mask = np.zeros(group.capacity, dtype=np.float32)
            for lr, wt in zip(learners, weights):
                w[lr._engine.slot] = wt
                mask[lr._engine.slot] = 1.0
            _stacked_mean_cuda(fed, group, w, mask, final)
            total_w = float(sum(weights))  # local share; the global Σw stays on the device
        elif group is not None:
            wm = torch.zeros(2, group.capacity, dtype=torch.float32)
            for lr, wt in zip(learners, weights):
                wm[0, lr._engine.slot] = wt
                wm[1, lr._engine.slot] = 1.0
            n = group.numel
            buf = torch.empty(n + 1, dtype=torch.float32, device=dev)
            ops.stacked_weighted_sum(group.params[:, :n], wm[0], buf[:n], 1.0)
            buf[n:].fill_(float(sum(weights)))
            fed.all_reduce_(buf)
            total = buf[n:].clone()
            buf[:n].div_(total.clamp_min(1e-12))
            ops.broadcast_rows(buf[:n], group.params[:, :n], wm[1])
            total_w = total
        else:
            total_w = _generic_mean(fed, addrs, learners, weights, final, bool(Settings.DELAYED_AVERAGING))
        return total_w, contributors

    # the side-stream pipeline's all-reduces stay unconfirmed until the next weights section (or
    # shutdown): by then the next local epoch is already queued behind them, so the host's wait for
    # them never leaves the GPU idle (see Federation.confirm_collectives)
    total_w, contributors = fed.run_aggregation(run)
    fed.record("aggregate", time.perf_counter() - t0)
    return total_w, contributors


def _mesh_mean(fed: Federation, addrs, learners, weights, final: bool = True) -> float:
    """FedAvg over a device mesh. Stacked engine groups (one per mesh rank): ONE native call.
    With ``OVERLAP_COLLECTIVES`` (default) it is the bucketed exchange on each device's comm
    stream (``rmesh_fedavg_bucketed``: reduce, per-bucket grouped all-reduce, the compute stream
    waiting per bucket for its apply; ``DELAYED_AVERAGING`` runs it beside the next local epoch and
    lands it a round later — see :func:`_mesh_mean_bucketed`); otherwise per device reduce launch,
    one grouped RCCL all-reduce and per device apply launch on the compute streams
    (``rmesh_fedavg``). Other learners: per device partial sums, one mesh all-reduce, unpack.

    The all-reduce is out of place, so every device keeps its local partial sum [Σ w x | Σ w]. The
    mesh guard (``parallel/mesh_guard.py``) confirms the collective at the next weights section;
    if it failed (asynchronous RCCL error, or a device that never completed it within
    ``COLLECTIVE_TIMEOUT``), the mesh is rebuilt over the responsive devices and ``retry`` re-runs
    the all-reduce of the retained partial sums over them and re-applies: the survivors' average
    of the round, i.e. the models that arrived (``aggregator.py:177-208``)."""
    wt_of = dict(zip(addrs, weights))
    ranks = _by_mesh_rank(fed, addrs, learners)
    groups = {r: {id(lr._engine.group): lr._engine.group for _, lr in v if getattr(lr, "_engine", None) is not None} for r, v in ranks.items()}
    stacked = all(len(g) == 1 and len(groups[r]) == 1 for r, g in groups.items() if ranks[r]) and all(
        getattr(lr, "_engine", None) is not None for v in ranks.values() for _, lr in v)
    numels = {next(iter(g.values())).numel for g in groups.values() if g}
    from myfyp_amd.settings import Settings

    if stacked and len(numels) == 1 and (Settings.OVERLAP_COLLECTIVES or Settings.DELAYED_AVERAGING or getattr(fed, "_mesh_delayed", None)):
        return _mesh_mean_bucketed(fed, ranks, groups, numels.pop(), wt_of, float(sum(weights)), bool(Settings.DELAYED_AVERAGING) and not final)
    if stacked and len(numels) == 1 and all(next(iter(g.values())).params.is_cuda for g in groups.values() if g):
        n = numels.pop()
        per: Dict[int, tuple] = {}  # mesh rank -> (params, partial, result, P, ld, w, mask)
        for r in fed.mesh_members:
            if ranks[r]:
                g = next(iter(groups[r].values()))
                wr = np.zeros(g.capacity, dtype=np.float32)
                mr = np.zeros(g.capacity, dtype=np.float32)
                for a, lr in ranks[r]:
                    wr[lr._engine.slot] = wt_of[a]
                    mr[lr._engine.slot] = 1.0
                with on_device(g.device):
                    out = getattr(g, "_mesh_out", None)
                    if out is None or out.numel() != n + 1:
                        out = g._mesh_out = torch.empty(n + 1, dtype=torch.float32, device=g.device)
                    per[r] = (g.params, g.fedavg_buffer(), out, g.capacity, g.S, wr, mr)
            else:  # no live peer on this device (yet in the mesh): contributes zeros
                scratch = fed.mesh_scratch(r, n + 1)
                per[r] = (scratch, scratch, fed.mesh_scratch(r, n + 1, "out"), 0, n, np.zeros(0, np.float32), np.zeros(0, np.float32))

        def cols(k: int, rs) -> list:
            return [per[r][k] for r in rs]

        rs = list(fed.mesh_members)
        fed.mesh.fedavg_stacked(cols(0, rs), cols(1, rs), cols(3, rs), n, cols(4, rs), np.concatenate(cols(5, rs)),
                                np.concatenate(cols(6, rs)), outs=cols(2, rs))

        def retry() -> None:  # over the current (rebuilt) mesh: the survivors' retained partials
            live = [r for r in fed.mesh_members if r in per]
            fed.mesh.fedavg_retry(cols(0, live), cols(1, live), cols(2, live), cols(3, live), n, cols(4, live), np.concatenate(cols(6, live)))

        fed.mesh_track("fedavg", retry)
        return float(sum(weights))
    ref = _pack(learners[0])
    n = ref.numel()
    accs: Dict[int, torch.Tensor] = {}
    for r in fed.mesh_members:
        dev = fed.devices[r]
        with on_device(dev):
            acc = torch.zeros(n + 1, dtype=torch.float32, device=dev)
            for a, lr in ranks[r]:
                if wt_of[a] > 0:
                    acc[:n].add_(_pack(lr), alpha=wt_of[a])
            acc[n] = float(sum(wt_of[a] for a, _ in ranks[r]))
        accs[r] = acc  # retained partial sum (the all-reduce below works on a copy)

    def reduce_unpack() -> None:
        live = [r for r in fed.mesh_members if r in accs]
        outs = []
        for r in live:
            with on_device(fed.devices[r]):
                outs.append(accs[r].clone())
        fed.mesh.all_reduce_(outs)
        for r, out in zip(live, outs):
            with on_device(fed.devices[r]):
                avg = out[:n] / out[n].clamp_min(1e-12)
                for a, lr in ranks[r]:
                    if a in fed.local_nodes:
                        _unpack_into(lr, avg)

    reduce_unpack()
    fed.mesh_track("fedavg", reduce_unpack)
    return float(sum(weights))


def _mesh_buf(g, name: str, numel: int) -> torch.Tensor:
    """A zero-initialised fp32 buffer cached on an engine group (its device)."""
    t = getattr(g, name, None)
    if t is None or t.numel() != numel:
        with on_device(g.params.device):
            t = torch.zeros(numel, dtype=torch.float32, device=g.params.device)
        setattr(g, name, t)
    return t


def _mesh_mean_bucketed(fed: Federation, ranks, groups, n: int, wt_of, total_w: float, delayed: bool) -> float:
    """Bucketed, overlapped mesh FedAvg of stacked engine groups.

    ``rmesh_fedavg_bucketed``: per device the weighted partial sums [Σw, pad | Σ w x] go to a
    retained buffer (``keep``) on the device's comm stream, each bucket of ``BUCKET_BYTES`` is
    all-reduced (grouped over the mesh) as soon as it is reduced, and the compute stream waits per
    bucket for its apply — bucket k's apply overlaps bucket k + 1's all-reduce, and the next local
    epoch is queued behind the applies without the host waiting.

    Delayed averaging (``DELAYED_AVERAGING``, not on the last round; the ranks path's semantics,
    ``_stacked_mean_cuda``): round r - 1's exchanged average is landed as x += avg - snap together
    with the new snapshot (``rmesh_delayed_land``, one launch per device), then the snapshot rows
    are exchanged on the comm streams with no apply and nothing waiting: the whole exchange runs
    beside round r + 1's local epoch. The mesh guard watches the comm streams then.

    Failure: the guard's ``retry`` re-runs the exchange from the retained ``keep`` buffers over the
    rebuilt mesh (``rmesh_fedavg_bucketed_retry``) and re-applies — the survivors' average."""
    from myfyp_amd.settings import Settings

    bucket = max(4, int(Settings.BUCKET_BYTES) // 4)
    per: Dict[int, tuple] = {}  # mesh rank -> (params, keep, out, P, ld, w, mask, snap)
    for r in fed.mesh_members:
        if ranks[r]:
            g = next(iter(groups[r].values()))
            wr = np.zeros(g.capacity, dtype=np.float32)
            mr = np.zeros(g.capacity, dtype=np.float32)
            for a, lr in ranks[r]:
                wr[lr._engine.slot] = wt_of[a]
                mr[lr._engine.slot] = 1.0
            snap = _mesh_buf(g, "_mesh_snap", g.capacity * n) if (delayed or getattr(fed, "_mesh_delayed", None)) else None
            per[r] = (g.params, _mesh_buf(g, "_mesh_keep4", n + 4), _mesh_buf(g, "_mesh_out4", n + 4), g.capacity, g.S, wr, mr, snap)
        else:  # no live peer on this device (yet in the mesh): contributes zeros
            scratch = fed.mesh_scratch(r, n + 4, "keep4")
            per[r] = (scratch, scratch, fed.mesh_scratch(r, n + 4, "out4"), 0, n, np.zeros(0, np.float32), np.zeros(0, np.float32), scratch)

    def cols(k: int, rs) -> list:
        return [per[r][k] for r in rs]

    rs = list(fed.mesh_members)
    comm = [comm_stream(fed.devices[r]) if fed.devices[r].type == "cuda" else None for r in rs]
    mask = np.concatenate(cols(6, rs))
    if getattr(fed, "_mesh_delayed", None) is not None:  # land round r - 1's exchanged average
        fed.mesh.delayed_land(cols(0, rs), cols(7, rs), cols(2, rs), cols(3, rs), n, cols(4, rs), n, mask, True)
        fed._mesh_delayed = None
        landed = True
    else:
        landed = False
    if delayed:
        if not landed:  # first delayed round: snapshot only
            fed.mesh.delayed_land(cols(0, rs), cols(7, rs), cols(2, rs), cols(3, rs), n, cols(4, rs), n, mask, False)
        fed.mesh.fedavg_bucketed(cols(7, rs), cols(1, rs), cols(2, rs), cols(3, rs), n, [n] * len(rs), np.concatenate(cols(5, rs)), mask, comm, bucket,
                                 apply=False)
        fed._mesh_delayed = True

        def retry_delayed() -> None:  # survivors: the retained partial sums again, landed next round
            live = [r for r in fed.mesh_members if r in per]
            fed.mesh.fedavg_bucketed_retry(cols(7, live), cols(1, live), cols(2, live), cols(3, live), n, [n] * len(live), np.concatenate(cols(6, live)),
                                           apply=False)

        fed.mesh_track("fedavg (delayed)", retry_delayed, streams=comm)
        return total_w
    fed.mesh.fedavg_bucketed(cols(0, rs), cols(1, rs), cols(2, rs), cols(3, rs), n, cols(4, rs), np.concatenate(cols(5, rs)), mask, comm, bucket, apply=True)

    def retry() -> None:  # over the current (rebuilt) mesh: the survivors' retained partials
        live = [r for r in fed.mesh_members if r in per]
        fed.mesh.fedavg_bucketed_retry(cols(0, live), cols(1, live), cols(2, live), cols(3, live), n, cols(4, live), np.concatenate(cols(6, live)))

    fed.mesh_track("fedavg", retry)
    return total_w


def _generic_mean(fed: Federation, addrs, learners, weights, final: bool, delayed: bool) -> float:
    """Per-learner path (CPU, or models outside a stacked engine group); same delayed-averaging
    semantics as the stacked kernels, in torch ops."""
    st = _delayed_state(fed, "generic") if (delayed or getattr(fed, "_delayed", {}).get("generic")) else None
    if st is not None and st.pending:  # land: x += avg_{r-1} - snap_{r-1}
        avg = st.buf[:-1] / st.buf[-1].clamp_min(1e-12)
        for a, lr in zip(addrs, learners):
            if a in st.snaps:
                _unpack_into(lr, _pack(lr) + (avg - st.snaps[a]))
        st.pending = False
    rows = [_pack(lr) for lr in learners]
    n = rows[0].numel()
    acc = torch.zeros(n + 1, dtype=torch.float32, device=rows[0].device)
    for r, wt in zip(rows, weights):
        if wt > 0:
            acc[:n].add_(r, alpha=wt)
    acc[n] = sum(weights)
    fed.all_reduce_(acc)
    total_w = float(acc[n])
    if delayed and not final:  # keep the local weights; the average lands next round
        st.snaps = dict(zip(addrs, rows))
        st.buf = acc
        st.pending = True
        return total_w
    avg = acc[:n] / max(total_w, 1e-12)
    for lr in learners:
        _unpack_into(lr, avg)
    return total_w


class _MeshMutation:
    """Mutation-testing knob of the mesh aggregations (``MYFYP_DEBUG_MESH_SCALE``, default 1; never
    set in normal runs): every peer's aggregation update is scaled, x <- x_before + s·(x_agg -
    x_before), so the mesh result is off by (s - 1) of its update while the non-mesh path the GPU
    tests compare against is not. Used once to show that the mesh aggregator tests catch a 5 %
    update error (``profiles/r6_mutation``)."""

    def __init__(self, fed: Federation, addrs) -> None:
        import os

        v = os.environ.get("MYFYP_DEBUG_MESH_SCALE")
        self.scale = float(v) if v else 1.0
        self.before = {}
        if self.scale != 1.0:
            for a in addrs:
                if a in fed.local_nodes:
                    lr = fed.local_nodes[a].learner
                    self.before[a] = (lr, _pack(lr).clone())

    def apply(self) -> None:
        for lr, x0 in self.before.values():
            _unpack_into(lr, x0 + self.scale * (_pack(lr) - x0))


def _pack(learner) -> torch.Tensor:
    return torch.cat([t.detach().reshape(-1).float() for t in state_tensors(learner)])


def _unpack_into(learner, flat: torch.Tensor) -> None:
    off = 0
    with torch.no_grad():
        for t in state_tensors(learner):
            t.copy_(flat[off : off + t.numel()].view_as(t).to(t.dtype))
            off += t.numel()


@traced("aggregate_neighbors")
def aggregate_neighbors(fed: Federation, arrived: Dict[str, Any], aggregator) -> List[str]:
    """Topology mixing ``x_i ← Σ_j W_ij x_j`` (see ``NeighborAvg``): co-located rows are combined
    with the ``weighted_average`` kernel, rows of neighbours on other ranks arrive through one
    grouped batch of point-to-point sends/receives (RCCL over xGMI; gloo on CPU). Every rank calls
    this with the same peer list, so the P2P pattern matches by construction. A ``ClippedGossip``
    takes the same sources and exchange, then moves every local row towards each source by at most
    its radius (``ops.clipped_gossip_into``) and publishes ``last_clipping``."""
    t0 = time.perf_counter()
    return fed.run_aggregation(lambda: _neighbors(fed, arrived, aggregator, t0))


def _neighbors(fed: Federation, arrived: Dict[str, Any], aggregator, t0: float) -> List[str]:
    peers = fed.all_peers()
    index = {a: i for i, a in enumerate(peers)}
    w = aggregator.mixing_matrix(len(peers))
    local = [a for a in peers if a in arrived and a in fed.local_nodes]
    if not local:
        fed.record("aggregate", time.perf_counter() - t0)
        return []
    learners = [fed.local_nodes[a].learner for a in local]
    if fed.mesh is not None and fed.mesh_size > 1:
        _mesh_neighbors(fed, peers, index, w, local, learners, aggregator)
        fed.record("aggregate", time.perf_counter() - t0)
        return local
    group = _stacked_group(learners)
    clipped = getattr(aggregator, "clipped", False)  # ClippedGossip: the same plan of sources, clipped per neighbour
    if clipped and fed.solo and group is not None and group.params.is_cuda and all(len(state_tensors(lr)) == 1 for lr in learners):
        # the live rows of the stacked engine buffer, in place: three launches, no pack or unpack
        src = {a: lr.flat_params() for a, lr in zip(local, learners)}
        _publish_clipping(fed, aggregator, _clipped_mix(aggregator, peers, index, w, local, src))
        fed.record("aggregate", time.perf_counter() - t0)
        return local
    if not clipped and fed.solo and group is not None and group.params.is_cuda and group.capacity <= 16 and group.S % 4 == 0:
        # every neighbour is a row of the same stacked engine buffer: the whole mixing step is one
        # in-place kernel (row p <- Σ_q M[p, q] row q); no per-peer pack / average / unpack launches
        mix = np.zeros((group.capacity, group.capacity), dtype=np.float32)
        local_set = set(local)
        for a, lr in zip(local, learners):
            i = index[a]
            nz = [j for j in np.nonzero(w[i])[0] if peers[j] in local_set]  # one rank: the sources are the local arrivals
            ws = np.array([w[i, j] for j in nz], dtype=np.float64)
            ws = ws / ws.sum()
            for j, x in zip(nz, ws):
                mix[lr._engine.slot, fed.local_nodes[peers[j]].learner._engine.slot] += x
        stream = torch.cuda.current_stream(group.params.device).cuda_stream
        ops.check(ops.fast_lib().myfyp_neighbor_mix_stacked(group.params.data_ptr(), group.capacity, group.numel, group.S, mix.ctypes.data, stream),
                  "neighbor_mix")
        fed.record("aggregate", time.perf_counter() - t0)
        return local
    rows = {a: _pack(fed.local_nodes[a].learner) for a in local}
    ref = rows[local[0]]
    # point-to-point plan: every (local peer, remote rank) edge sends once; every remote neighbour is received once
    sends, recvs = {}, {}
    for a in local:
        i = index[a]
        for j in np.nonzero(w[i])[0]:
            b = peers[j]
            rb = fed.peers[b]
            if j == i or rb == fed.rank:
                continue
            sends[(a, rb)] = rows[a]
            if b not in recvs:
                recvs[b] = torch.empty_like(ref)
    if sends or recvs:
        import torch.distributed as dist

        # per rank pair, sends and receives are both ordered by the source peer's index (NCCL ignores tags)
        pg = fed.group
        ops_ = [dist.P2POp(dist.isend, t, rb, group=pg, tag=index[a]) for (a, rb), t in sorted(sends.items(), key=lambda kv: (index[kv[0][0]], kv[0][1]))]
        ops_ += [dist.P2POp(dist.irecv, t, fed.peers[b], group=pg, tag=index[b]) for b, t in sorted(recvs.items(), key=lambda kv: index[kv[0]])]
        fed.batch_p2p_(ops_)
    src = dict(rows)
    src.update(recvs)
    if clipped:
        # the packed local rows are written in place; the received rows are sources only
        _publish_clipping(fed, aggregator, _clipped_mix(aggregator, peers, index, w, local, src))
        for a in local:
            _unpack_into(fed.local_nodes[a].learner, rows[a])
        fed.record("aggregate", time.perf_counter() - t0)
        return local
    mixed = {}
    for a in local:
        i = index[a]
        nz = [j for j in np.nonzero(w[i])[0] if peers[j] in src]
        ws = np.array([w[i, j] for j in nz], dtype=np.float64)
        ws = ws / ws.sum()  # a dead neighbour's share folds back proportionally
        mixed[a] = ops.weighted_average([[src[peers[j]]] for j in nz], [float(x) for x in ws])[0]
    for a in local:
        _unpack_into(fed.local_nodes[a].learner, mixed[a])
    fed.record("aggregate", time.perf_counter() - t0)
    return local


def _mesh_neighbors(fed: Federation, peers, index, w, local, learners, aggregator=None) -> None:
    """Topology mixing over a device mesh: every row a peer needs from another device arrives by
    ONE grouped RCCL send/recv exchange (``rmesh_p2p``); the mix runs on the receiving device
    (a ``ClippedGossip``: one clipped mix per receiving device, the received rows as sources only)."""
    lr_of = dict(zip(local, learners))
    rank = {a: mesh_rank_of(lr_of[a]) for a in local}
    rows = {}
    for a in local:
        with on_device(fed.devices[rank[a]]):
            rows[a] = _pack(lr_of[a])
    # (source peer, destination mesh rank) pairs, in one deterministic order for both sides
    need = sorted({(peers[j], rank[a]) for a in local for j in np.nonzero(w[index[a]])[0]
                   if peers[j] in rank and rank[peers[j]] != rank[a]}, key=lambda x: (index[x[0]], x[1]))
    got: Dict[Tuple[str, int], torch.Tensor] = {}
    ops_ = []
    for b, rd in need:
        buf = torch.empty_like(rows[b], device=fed.devices[rd])
        got[(b, rd)] = buf
        ops_.append(("send", fed.mesh_position(rank[b]), fed.mesh_position(rd), rows[b]))
        ops_.append(("recv", fed.mesh_position(rd), fed.mesh_position(rank[b]), buf))
    if ops_:
        fed.mesh.p2p_(ops_)
        fed.mesh_track("p2p")
    if getattr(aggregator, "clipped", False):
        for rd in sorted(set(rank.values())):
            here = [a for a in local if rank[a] == rd]
            src = {a: rows[a] for a in here}
            src.update({b: t for (b, r), t in got.items() if r == rd})
            with on_device(fed.devices[rd]):
                _publish_clipping(fed, aggregator, _clipped_mix(aggregator, peers, index, w, here, src), here)
                for a in here:
                    _unpack_into(lr_of[a], rows[a])
        return
    mixed = {}
    for a in local:
        i = index[a]
        nz = [j for j in np.nonzero(w[i])[0] if peers[j] in rank]
        ws = np.array([w[i, j] for j in nz], dtype=np.float64)
        ws = ws / ws.sum()  # a dead neighbour's share folds back proportionally
        srcs = [rows[peers[j]] if rank[peers[j]] == rank[a] else got[(peers[j], rank[a])] for j in nz]
        with on_device(fed.devices[rank[a]]):
            mixed[a] = ops.weighted_average([[t] for t in srcs], [float(x) for x in ws])[0]
    for a in local:
        with on_device(fed.devices[rank[a]]):
            _unpack_into(lr_of[a], mixed[a])


def _clipped_mix(aggregator, peers, index, w, targets, src):
    """One ``ops.clipped_gossip_into`` call over the rows of ``src`` (address -> flat fp32 row), in
    peer order: the rows of ``targets`` are written in place, every other row is a source only (an
    all-zero row of W). Row ``a``'s shares are ``w[a, b]`` over its present sources (itself
    included), renormalised as the plain mix does, so an absent neighbour's share folds back
    proportionally; the self share is implicit. Returns ``(addresses in row order, tau, w_eff)``."""
    order = sorted(src, key=lambda a: index[a])
    row = {a: r for r, a in enumerate(order)}
    shares = np.zeros((len(order), len(order)), dtype=np.float64)
    for a in targets:
        i = index[a]
        nz = [j for j in np.nonzero(w[i])[0] if peers[j] in src]
        total = float(sum(w[i, j] for j in nz))
        for j in nz:
            if j != i:
                shares[row[a], row[peers[j]]] = w[i, j] / total
    with torch.no_grad():
        _, tau, w_eff = ops.clipped_gossip_into([src[a] for a in order], shares, **aggregator.radius_args())
    return order, tau, w_eff


def _publish_clipping(fed: Federation, aggregator, clipping, addrs=None) -> None:
    """``last_clipping = (addresses in row order, tau, w_eff)`` on the round's aggregator and on the
    aggregators of the local peers among ``addrs`` (default: the rows). Device tensors: reading
    them is the caller's synchronisation."""
    written = [a for a in (clipping[0] if addrs is None else addrs) if a in fed.local_nodes]
    for a in written:
        fed.local_nodes[a].aggregator.last_clipping = clipping
    # the round's aggregator is usually one peer's own: on a mesh it keeps the plan of that peer's device
    owners = [a for a, node in fed.local_nodes.items() if node.aggregator is aggregator]
    if not owners or set(owners) & set(written):
        aggregator.last_clipping = clipping


# aggregator kinds reduced on the device (no wire models, no host copies)
DEVICE_KINDS = ("mean", "neighbor", "scaffold", "median", "krum", "trimmed_mean", "geometric_median", "bulyan", "dnc")


def _scaffold_cb(learner):
    for cb in getattr(learner, "callbacks", []):
        if cb.get_name() == "scaffold":
            return cb
    raise ValueError("SCAFFOLD aggregation needs the 'scaffold' callback on every learner")


@traced("aggregate_scaffold")
def aggregate_scaffold(fed: Federation, arrived: Dict[str, Tuple[float, Any]], aggregator) -> None:
    """SCAFFOLD server step on the device (reference math: ``p2pfl/learning/aggregators/
    scaffold.py:76-111``): x ← x_start + η_g·Σ n_i Δy_i / Σ n_i, c ← c + mean(Δc_i).

    One packed device buffer [Σ n_iΔy_i | Σ n_i | Σ Δc_i | count] reduced over the local trainers,
    ONE all-reduce over the live ranks, then every local peer's flat parameters are set to the new
    global model and its callbacks receive the new global control variate (a device tensor).
    x_start is a trainer's round-start snapshot (the callback's x0) or a non-trainer's current
    weights — identical on every rank, since every peer starts the round from the last aggregate."""
    t0 = time.perf_counter()
    fed.run_aggregation(lambda: _scaffold(fed, arrived, aggregator))
    fed.record("aggregate", time.perf_counter() - t0)


def _mesh_scaffold(fed: Federation, arrived: Dict[str, Tuple[float, Any]], aggregator) -> None:
    """SCAFFOLD server step over a device mesh: per device the packed local reduction, ONE mesh
    all-reduce, per device the apply (new model into its peers, its copy of the control variate)."""
    addrs = [a for a in arrived if a in fed.local_nodes]
    learners = [fed.local_nodes[a].learner for a in addrs]
    ranks = _by_mesh_rank(fed, addrs, learners)
    n = learners[0].flat_params().numel()
    bufs, x_starts = [], {}
    for r in fed.mesh_members:
        dev = fed.devices[r]
        dys, dcs, ws = [], [], []
        with on_device(dev):
            for a, lr in ranks[r]:
                wt = float(arrived[a][0])
                cb = _scaffold_cb(lr)
                if wt > 0 and cb.delta_y is not None:
                    dys.append(cb.delta_y)
                    dcs.append(cb.delta_c)
                    ws.append(wt)
                    x_starts.setdefault(r, cb.x0)
            buf = torch.zeros(2 * n + 2, dtype=torch.float32, device=dev)
            if dys:
                ops.scaffold_reduce(buf, dys, dcs, ws)
        bufs.append(buf)
    fed.mesh.all_reduce_(bufs)
    fed.mesh_track("scaffold all_reduce")
    cdev = fed.__dict__.setdefault("_mesh_c", {})
    for r, buf in zip(fed.mesh_members, bufs):
        if not ranks[r]:
            continue
        dev = fed.devices[r]
        with on_device(dev):
            x_start = x_starts.get(r)
            if x_start is None:  # the round-start model: every peer starts the round from it
                src = next((v for v in x_starts.values()), None)
                x_start = src.to(dev) if src is not None else ranks[r][0][1].flat_params().detach().clone()
            c_prev = cdev.get(r)
            c_init = c_prev is None or c_prev.numel() != n
            c_new = torch.empty(n, dtype=torch.float32, device=dev) if c_init else c_prev
            flats = [lr.flat_params() for _, lr in ranks[r]]
            with torch.no_grad():
                ops.scaffold_apply(flats, x_start, buf, c_new, c_init, aggregator.global_lr)
            cdev[r] = c_new
            gc = ranks[r][0][1].split_flat(c_new)
            for a, lr in ranks[r]:
                fed.local_nodes[a].aggregator._c_dev = c_new
                lr.get_model().add_info("scaffold", {"global_c": gc})
                lr.update_callbacks_with_model_info()


def _scaffold(fed: Federation, arrived: Dict[str, Tuple[float, Any]], aggregator) -> None:
    if fed.mesh is not None:  # (a one-device mesh too: its collectives still run through RCCL)
        mut = _MeshMutation(fed, list(arrived))
        _mesh_scaffold(fed, arrived, aggregator)
        if mut.before:
            mut.apply()
        return
    addrs = [a for a in arrived if a in fed.local_nodes]
    learners = {a: fed.local_nodes[a].learner for a in addrs}
    flats = [learners[a].flat_params() for a in addrs]
    n = flats[0].numel()
    dys, dcs, ws = [], [], []
    x_start = None
    for a in addrs:
        w = float(arrived[a][0])
        cb = _scaffold_cb(learners[a])
        if w > 0 and cb.delta_y is not None:
            dys.append(cb.delta_y)
            dcs.append(cb.delta_c)
            ws.append(w)
            if x_start is None:
                x_start = cb.x0
    if x_start is None:  # no local trainer: this rank's peers still hold the round-start model
        x_start = flats[0].detach().clone()
    # one reduction launch -> ONE all-reduce of [Σ n_iΔy_i | Σ n_i | Σ Δc_i | count] -> one apply
    # launch that writes the new model into every local peer and updates the control variate
    buf = torch.empty(2 * n + 2, dtype=torch.float32, device=flats[0].device)
    ops.scaffold_reduce(buf, dys, dcs, ws)
    fed.all_reduce_(buf)
    c_prev = getattr(aggregator, "_c_dev", None)
    c_init = c_prev is None or c_prev.numel() != n
    c_new = torch.empty(n, dtype=torch.float32, device=buf.device) if c_init else c_prev
    with torch.no_grad():
        ops.scaffold_apply(flats, x_start, buf, c_new, c_init, aggregator.global_lr)
    gc = learners[addrs[0]].split_flat(c_new)  # same architecture on every peer: one set of views
    for a in addrs:
        lr = learners[a]
        fed.local_nodes[a].aggregator._c_dev = c_new
        lr.get_model().add_info("scaffold", {"global_c": gc})
        lr.update_callbacks_with_model_info()


@traced("aggregate_median")
def aggregate_median(fed: Federation, arrived: Dict[str, Tuple[float, Any]]) -> None:
    """Coordinate-wise median of the trainers' models on the device (``fedmedian.py:56-62``):
    the local trainers' flat rows are packed into a [k_max, n] buffer, ONE all-gather over the live
    ranks (RCCL) collects every trainer's row, and ONE ``k_coordinate_median<K>`` launch (sorting
    network in registers, <= 16 models) writes the result into every local peer. With a single
    rank the kernel reads the live rows directly (no packing copy)."""
    t0 = time.perf_counter()
    fed.run_aggregation(lambda: _median(fed, arrived))
    fed.record("aggregate", time.perf_counter() - t0)


def _mesh_median(fed: Federation, arrived: Dict[str, Tuple[float, Any]]) -> None:
    """Coordinate median over a device mesh: every device packs its trainers' rows ([k_max, n],
    zero-padded), ONE mesh all-gather, then per device one median launch into its peers."""
    addrs = [a for a in arrived if a in fed.local_nodes]
    learners = [fed.local_nodes[a].learner for a in addrs]
    ranks = _by_mesh_rank(fed, addrs, learners)
    trainers = {r: [(a, lr) for a, lr in v if float(arrived[a][0]) > 0] for r, v in ranks.items()}
    counts = [len(trainers[r]) for r in fed.mesh_members]
    if not sum(counts):
        return
    kmax = max(counts)
    n = _pack(learners[0]).numel()
    sends, recvs = [], []
    for r in fed.mesh_members:
        dev = fed.devices[r]
        with on_device(dev):
            s_ = torch.zeros(kmax, n, dtype=torch.float32, device=dev)
            for i, (a, lr) in enumerate(trainers[r]):
                s_[i].copy_(_pack(lr))
            sends.append(s_)
            recvs.append(torch.empty(len(counts) * kmax, n, dtype=torch.float32, device=dev))
    fed.mesh.all_gather_(recvs, sends)
    fed.mesh_track("median all_gather")
    for r, recv in zip(fed.mesh_members, recvs):
        if not ranks[r]:
            continue
        with on_device(fed.devices[r]):
            rows = [recv[q * kmax + i] for q, c in enumerate(counts) for i in range(c)]
            med = torch.empty(n, dtype=torch.float32, device=recv.device)
            ops.median_into(rows, [med])
            for _, lr in ranks[r]:
                _unpack_into(lr, med)


def _median(fed: Federation, arrived: Dict[str, Tuple[float, Any]]) -> None:
    if fed.mesh is not None:  # (a one-device mesh too: its collectives still run through RCCL)
        mut = _MeshMutation(fed, list(arrived))
        _mesh_median(fed, arrived)
        if mut.before:
            mut.apply()
        return
    addrs = [a for a in arrived if a in fed.local_nodes]
    learners = {a: fed.local_nodes[a].learner for a in addrs}
    trainers = [a for a in addrs if float(arrived[a][0]) > 0]
    counts = fed.all_gather_object(len(trainers))
    kmax = max(1, max(counts))
    flat_only = all(len(state_tensors(learners[a])) == 1 for a in addrs)  # no floating buffers
    rows_of = (lambda a: learners[a].flat_params()) if flat_only else (lambda a: _pack(learners[a]))
    if fed.solo:  # every trainer is local: median straight from the live rows into every peer
        if not trainers:
            return
        if flat_only:
            ops.median_into([rows_of(a) for a in trainers], [learners[a].flat_params() for a in addrs])
        else:
            med = torch.empty_like(_pack(learners[addrs[0]]))
            ops.median_into([rows_of(a) for a in trainers], [med])
            for a in addrs:
                _unpack_into(learners[a], med)
        return
    ref = rows_of(addrs[0])
    n = ref.numel()
    send = torch.zeros(kmax, n, dtype=torch.float32, device=ref.device)
    for i, a in enumerate(trainers):
        send[i].copy_(rows_of(a))
    recv = torch.empty(len(counts) * kmax, n, dtype=torch.float32, device=ref.device)
    fed.all_gather_into_tensor_(recv, send)
    rows = [recv[r * kmax + i] for r, c in enumerate(counts) for i in range(c)]
    if not rows:
        return
    if flat_only:
        ops.median_into(rows, [learners[a].flat_params() for a in addrs])
    else:
        med = torch.empty(n, dtype=torch.float32, device=ref.device)
        ops.median_into(rows, [med])
        for a in addrs:
            _unpack_into(learners[a], med)


# ---------------------------------------------------------------------------------------------
# robust aggregation: coordinate-wise trimmed mean, (Multi-)Krum, the geometric median and Bulyan
# ---------------------------------------------------------------------------------------------
ROBUST_MAX_ROWS = 16  # rows the device kernels take (ops.trimmed_mean_into / krum_into / geometric_median_into / bulyan_into)


@traced("aggregate_trimmed_mean")
def aggregate_trimmed_mean(fed: Federation, arrived: Dict[str, Tuple[float, Any]], aggregator) -> None:
    """Coordinate-wise trimmed mean of the trainers' models on the device (host math:
    ``_math.trimmed_mean``), laid out as :func:`aggregate_median`: the local trainers' rows packed
    into a [k_max, n] buffer, ONE all-gather over the live ranks, ONE ``k_trimmed_mean<K>`` launch
    into every local peer. ``trim = floor(beta·K)`` with K this round's trainers; ``2·trim >= K``
    raises the host aggregator's ``ValueError`` on every rank, before any collective."""
    t0 = time.perf_counter()
    fed.run_aggregation(lambda: _robust(fed, arrived, aggregator, "trimmed_mean"))
    fed.record("aggregate", time.perf_counter() - t0)


@traced("aggregate_krum")
def aggregate_krum(fed: Federation, arrived: Dict[str, Tuple[float, Any]], aggregator) -> None:
    """(Multi-)Krum over the trainers' models on the device (host math: ``Krum.aggregate``): the
    all-gather of :func:`aggregate_median`, then ``ops.krum_into`` — distances from differences,
    selection and the sample-weighted mean of the chosen rows written into every local peer, the
    selection never leaving the device on the round's path. Every rank reduces the same gathered
    buffer with the same grid, so all of them choose the same peers, bit for bit. Afterwards every
    local node's aggregator carries ``last_selection = (trainer addresses in row order, coef)``;
    ``coef`` is the device tensor (reading it is the caller's synchronisation), 0 for a rejected peer."""
    t0 = time.perf_counter()
    fed.run_aggregation(lambda: _robust(fed, arrived, aggregator, "krum"))
    fed.record("aggregate", time.perf_counter() - t0)


@traced("aggregate_geometric_median")
def aggregate_geometric_median(fed: Federation, arrived: Dict[str, Tuple[float, Any]], aggregator) -> None:
    """Geometric median of the trainers' models on the device (host math:
    ``GeometricMedian.aggregate``): the all-gather of :func:`aggregate_median`, then
    ``ops.geometric_median_into`` — the screen, ``aggregator.iters`` smoothed Weiszfeld steps and
    the weighted mean written into every local peer, no coefficient leaving the device on the
    round's path. Every rank reduces the same gathered buffer with the same grid, so all of them
    reach the same coefficients, bit for bit. Afterwards every local node's aggregator carries
    ``last_weights = (trainer addresses in row order, coef)``; ``coef`` is the device tensor
    (reading it is the caller's synchronisation), small for a down-weighted peer."""
    t0 = time.perf_counter()
    fed.run_aggregation(lambda: _robust(fed, arrived, aggregator, "geometric_median"))
    fed.record("aggregate", time.perf_counter() - t0)


@traced("aggregate_bulyan")
def aggregate_bulyan(fed: Federation, arrived: Dict[str, Tuple[float, Any]], aggregator) -> None:
    """Bulyan over the trainers' models on the device (host math: ``Bulyan.aggregate``): the
    all-gather of :func:`aggregate_median`, then ``ops.bulyan_into`` — Krum's distances, K − 2f rows
    picked by iterated Krum and, per coordinate, the mean of the K − 4f picked values closest to
    their median written into every local peer, the selection never leaving the device on the
    round's path. ``K < 4f + 3`` with K this round's trainers raises the host aggregator's
    ``ValueError`` on every rank, before any collective. Every rank reduces the same gathered buffer
    with the same grid, so all of them pick the same peers, bit for bit. Afterwards every local
    node's aggregator carries ``last_selection = (trainer addresses in row order, coef)``; ``coef``
    is the device tensor (reading it is the caller's synchronisation), 0 for a rejected peer."""
    t0 = time.perf_counter()
    fed.run_aggregation(lambda: _robust(fed, arrived, aggregator, "bulyan"))
    fed.record("aggregate", time.perf_counter() - t0)


@traced("aggregate_dnc")
def aggregate_dnc(fed: Federation, arrived: Dict[str, Tuple[float, Any]], aggregator, round_: int) -> None:
    """DnC spectral filtering over the trainers' models on the device (host math: ``DnC.aggregate``):
    the all-gather of :func:`aggregate_median`, then ``ops.dnc_into`` — per iteration the distances
    over the coordinate subsample of ``(seed, round_, iteration)``, the top eigenpair of the centred
    Gram matrix and the rows of largest projection removed, then the sample-weighted mean of the
    rows kept written into every local peer, the selection never leaving the device on the round's
    path. ``round_`` is stored as ``aggregator.round`` on the aggregator given and on every local
    node's aggregator, so all ranks draw the same subsample. Bad parameters (``iters · m >= K`` with K
    this round's trainers) raise ``ValueError`` on every rank, before any collective. Every rank
    reduces the same gathered buffer with the same grid, so all of them remove the same peers, bit
    for bit. Afterwards every local node's aggregator carries ``last_selection = (trainer addresses
    in row order, coef)``; ``coef`` is the device tensor (reading it is the caller's
    synchronisation), 0 for a removed peer."""
    t0 = time.perf_counter()
    aggregator.round = int(round_)
    for node in fed.local_nodes.values():
        if getattr(node.aggregator, "collective_kind", None) == "dnc":
            node.aggregator.round = int(round_)
    fed.run_aggregation(lambda: _robust(fed, arrived, aggregator, "dnc"))
    fed.record("aggregate", time.perf_counter() - t0)


def _dnc_check(aggregator, k: int) -> None:
    ops.dnc_check(k, aggregator.f, aggregator.filter_frac, aggregator.iters, aggregator.subsample_dims)


def _trim_count(aggregator, k: int) -> int:
    trim = int(np.floor(aggregator.beta * k))
    if 2 * trim >= k:
        raise ValueError("beta too large for the number of models")
    return trim


def _robust_into(kind: str, aggregator, rows, outs, ws):
    """The device op of ``kind``; Krum, the geometric median and Bulyan return their ``coef`` device tensor."""
    with torch.no_grad():
        if kind == "trimmed_mean":
            ops.trimmed_mean_into(rows, outs, _trim_count(aggregator, len(rows)))
            return None
        if kind == "geometric_median":
            return ops.geometric_median_into(rows, outs, ws, aggregator.iters, aggregator.nu)[0]
        if kind == "bulyan":
            return ops.bulyan_into(rows, outs, aggregator.f)[2]
        if kind == "dnc":
            return ops.dnc_into(rows, outs, ws, aggregator.f, aggregator.filter_frac, aggregator.iters, aggregator.subsample_dims, aggregator.seed,
                                aggregator.round)[4]
        return ops.krum_into(rows, outs, ws, aggregator.f, aggregator.m)[2]


def _int_buffers(learner) -> List[torch.Tensor]:
    return [b for b in learner.model.get_model().buffers() if not b.is_floating_point()]


def _row_fns(learners, kind: str):
    """(live, row_of): ``live`` when a peer's model is its flat parameter vector alone, so the
    kernels read and write the live rows; otherwise ``row_of`` packs a copy (flat parameters, then
    the floating buffers ``_unpack_into`` takes back). The host ``Krum`` measures every tensor of
    ``get_parameters()`` — the whole ``state_dict``, BatchNorm's integer ``num_batches_tracked``
    included — so the Krum row carries those counters too, behind everything that is unpacked: the
    device and the host then score the same vector and select the same peers. The geometric median
    Bulyan and DnC measure distances too, and take the same rows."""
    whole = kind in ("krum", "geometric_median", "bulyan", "dnc")
    live = all(len(state_tensors(lr)) == 1 and not (whole and _int_buffers(lr)) for lr in learners)
    if live:
        return True, lambda lr: lr.flat_params()
    if whole:
        return False, lambda lr: torch.cat([_pack(lr)] + [b.detach().reshape(-1).float() for b in _int_buffers(lr)])
    return False, _pack


def _publish_selection(fed: Federation, addrs, aggregator, order, coef) -> None:
    if coef is None:
        return
    # Krum, Bulyan and DnC publish a selection, the geometric median its weights
    attr = "last_weights" if getattr(aggregator, "collective_kind", None) == "geometric_median" else "last_selection"
    setattr(aggregator, attr, (list(order), coef))
    for a in addrs:
        if a in fed.local_nodes:
            setattr(fed.local_nodes[a].aggregator, attr, (list(order), coef))


def _robust(fed: Federation, arrived: Dict[str, Tuple[float, Any]], aggregator, kind: str) -> None:
    if fed.mesh is not None:  # (a one-device mesh too: its collectives still run through RCCL)
        mut = _MeshMutation(fed, list(arrived))
        _mesh_robust(fed, arrived, aggregator, kind)
        if mut.before:
            mut.apply()
        return
    addrs = [a for a in arrived if a in fed.local_nodes]
    learners = {a: fed.local_nodes[a].learner for a in addrs}
    trainers = [a for a in addrs if float(arrived[a][0]) > 0]
    # every rank learns K, the row order (rank, then local order) and the sample weights
    gathered = fed.all_gather_object([(a, float(arrived[a][0])) for a in trainers])
    counts = [len(g) for g in gathered]
    order = [a for g in gathered for a, _ in g]
    ws = [w for g in gathered for _, w in g]
    if not order:
        return
    if kind == "trimmed_mean":
        _trim_count(aggregator, len(order))  # the same K on every rank: all of them raise, or none
    if kind == "bulyan":
        ops.bulyan_check(len(order), aggregator.f)  # likewise
    if kind == "dnc":
        _dnc_check(aggregator, len(order))  # likewise
    live, row_of = _row_fns(list(learners.values()), kind)

    def reduce_rows(rows) -> None:
        if live:
            coef = _robust_into(kind, aggregator, rows, [learners[a].flat_params() for a in addrs], ws)
        else:
            res = torch.empty_like(rows[0])
            coef = _robust_into(kind, aggregator, rows, [res], ws)
            for a in addrs:
                _unpack_into(learners[a], res)
        _publish_selection(fed, addrs, aggregator, order, coef)

    if fed.solo:  # every trainer is local: straight from the live rows into every peer
        reduce_rows([row_of(learners[a]) for a in trainers])
        return
    kmax = max(1, max(counts))
    ref = row_of(learners[addrs[0]])
    n = ref.numel()
    send = torch.zeros(kmax, n, dtype=torch.float32, device=ref.device)
    for i, a in enumerate(trainers):
        send[i].copy_(row_of(learners[a]))
    recv = torch.empty(len(counts) * kmax, n, dtype=torch.float32, device=ref.device)
    fed.all_gather_into_tensor_(recv, send)
    reduce_rows([recv[r * kmax + i] for r, c in enumerate(counts) for i in range(c)])


def _mesh_robust(fed: Federation, arrived: Dict[str, Tuple[float, Any]], aggregator, kind: str) -> None:
    """Trimmed mean / Krum / geometric median / Bulyan over a device mesh, in the manner of ``_mesh_median``: every device
    packs its trainers' rows ([k_max, n], zero-padded), ONE mesh all-gather, then per device the op
    into a result vector unpacked into its peers. Every device reduces the same gathered rows in the
    same order, so a Krum selection is the same on all of them."""
    addrs = [a for a in arrived if a in fed.local_nodes]
    learners = [fed.local_nodes[a].learner for a in addrs]
    ranks = _by_mesh_rank(fed, addrs, learners)
    trainers = {r: [(a, lr) for a, lr in v if float(arrived[a][0]) > 0] for r, v in ranks.items()}
    counts = [len(trainers[r]) for r in fed.mesh_members]
    order = [a for r in fed.mesh_members for a, _ in trainers[r]]
    ws = [float(arrived[a][0]) for a in order]
    if not order:
        return
    if kind == "trimmed_mean":
        _trim_count(aggregator, len(order))
    if kind == "bulyan":
        ops.bulyan_check(len(order), aggregator.f)
    if kind == "dnc":
        _dnc_check(aggregator, len(order))
    _, row_of = _row_fns(learners, kind)
    kmax = max(counts)
    n = row_of(learners[0]).numel()
    sends, recvs = [], []
    for r in fed.mesh_members:
        dev = fed.devices[r]
        with on_device(dev):
            s_ = torch.zeros(kmax, n, dtype=torch.float32, device=dev)
            for i, (a, lr) in enumerate(trainers[r]):
                s_[i].copy_(row_of(lr))
            sends.append(s_)
            recvs.append(torch.empty(len(counts) * kmax, n, dtype=torch.float32, device=dev))
    fed.mesh.all_gather_(recvs, sends)
    fed.mesh_track(f"{kind} all_gather")
    for r, recv in zip(fed.mesh_members, recvs):
        if not ranks[r]:
            continue
        with on_device(fed.devices[r]):
            rows = [recv[q * kmax + i] for q, c in enumerate(counts) for i in range(c)]
            res = torch.empty(n, dtype=torch.float32, device=recv.device)
            coef = _robust_into(kind, aggregator, rows, [res], ws)
            for _, lr in ranks[r]:
                _unpack_into(lr, res)
            _publish_selection(fed, [a for a, _ in ranks[r]], aggregator, order, coef)


# ---------------------------------------------------------------------------------------------
# colluding attacks (fault_injection.ColludingAttack): ALIE, IPM, min-max, min-sum
# ---------------------------------------------------------------------------------------------
@traced("collude")
def collude(fed: Federation, weights: Dict[str, float], attackers, kind: str, z: Optional[float] = None, eps: float = 0.5,
            refs: Optional[Dict[str, torch.Tensor]] = None):
    """Rewrite the attackers' rows in place, on the device, between the local epoch and the round's
    aggregation (a ``Federation.pre_aggregation_hooks`` entry calls this with its ``weights``: the
    local peers' sample weights, 0 for a non-trainer). The attackers are omniscient and collude:
    all of them that trained this round receive the one row ``ops.collude_into`` crafts from the
    honest trainers' rows (the trainers that are not attackers), in the row order of ``_robust``:
    rank first, then local order. Laid out as ``_robust`` / ``_mesh_robust``: one rank reads the live
    rows and writes the local attackers' rows directly; several ranks gather order and counts (one
    ``all_gather_object``) and the honest rows (one ``all_gather_into_tensor_``), and every rank
    computes the same row, γ included bit for bit, and writes its own attackers; a mesh gathers once
    and computes per device. An attacker that did not train this round is left alone; with no honest
    trainer or no attacking trainer nothing happens, on every rank. The launches go to the current
    stream of the rows' device: behind the epoch the gang leader enqueued, ahead of the aggregation.

    ``refs`` (IPM): ``{addr: row}`` snapshots from :func:`collude_snapshot`, the model the round
    started from. Returns ``(honest addresses in row order, attacker addresses, gamma, stat)`` with
    the device tensors of ``ops.collude_into`` (reading them is the caller's synchronisation), or
    None when nothing happened."""
    attackers = set(attackers)
    return fed.run_aggregation(lambda: _collude(fed, weights, attackers, kind, z, eps, refs or {}))


def collude_snapshot(fed: Federation, attackers) -> Dict[str, torch.Tensor]:
    """Device copies of the rows of the local ``attackers`` (one per device), in the layout
    :func:`collude` reads: taken at a round's start they are IPM's reference model."""
    local = [a for a in fed.local_order if a in fed.local_nodes]
    learners = [fed.local_nodes[a].learner for a in local]
    if not learners:
        return {}
    _, row_of = _row_fns(learners, "krum")
    out: Dict[str, torch.Tensor] = {}
    seen = set()
    for a, lr in zip(local, learners):
        if a not in attackers:
            continue
        key = mesh_rank_of(lr) if fed.mesh is not None else 0
        if key in seen:
            continue
        seen.add(key)
        dev = lr.flat_params().device
        with on_device(dev), torch.no_grad():
            out[a] = row_of(lr).detach().clone()
    return out


def _collude_ref(refs: Dict[str, torch.Tensor], dev: torch.device) -> Optional[torch.Tensor]:
    for t in refs.values():
        if t.device == dev:
            return t
    for t in refs.values():  # a device without an attacker of its own: a copy of another's snapshot
        return t.to(dev)
    return None


def _collude_write(kind: str, rows, targets, live: bool, z, eps, ref, n_attackers: int):
    """``ops.collude_into`` from ``rows`` into the ``targets`` learners (a scratch row when this rank
    or device hosts no attacker: it still publishes γ). ALIE's default z counts every attacker."""
    if kind == "alie" and z is None:
        z = ops.alie_z(len(rows) + n_attackers, n_attackers)
    with torch.no_grad():
        if kind == "ipm" and ref is None:  # nothing to write here, and no reference to compute from
            return torch.tensor([float(eps)], dtype=torch.float32, device=rows[0].device), torch.zeros(2 * len(rows) + 3, dtype=torch.float64, device=rows[0].device)
        if live and targets:
            return ops.collude_into(rows, [lr.flat_params() for lr in targets], kind, z=z, eps=eps, ref=ref)
        res = torch.empty_like(rows[0])
        out = ops.collude_into(rows, [res], kind, z=z, eps=eps, ref=ref)
        for lr in targets:
            _unpack_into(lr, res)
        return out


def _collude(fed: Federation, weights: Dict[str, float], attackers: set, kind: str, z, eps, refs):
    if kind not in ops.COLLUDE_KINDS:
        raise ValueError(f"unknown colluding attack {kind!r}; choose from {ops.COLLUDE_KINDS}")
    if fed.mesh is not None:
        return _mesh_collude(fed, weights, attackers, kind, z, eps, refs)
    addrs = [a for a in weights if a in fed.local_nodes]
    learners = {a: fed.local_nodes[a].learner for a in addrs}
    trainers = [a for a in addrs if float(weights[a]) > 0]
    honest = [a for a in trainers if a not in attackers]
    mine = [a for a in trainers if a in attackers]
    # every rank learns H, the row order (rank, then local order) and who attacks this round
    gathered = fed.all_gather_object((honest, mine))
    counts = [len(h) for h, _ in gathered]
    order = [a for h, _ in gathered for a in h]
    attacking = [a for _, m in gathered for a in m]
    if not order or not attacking:
        return None
    live, row_of = _row_fns(list(learners.values()), "krum")
    targets = [learners[a] for a in mine]
    if fed.solo:  # every honest trainer is local: straight from the live rows
        rows = [row_of(learners[a]) for a in honest]
        dev = rows[0].device
        with on_device(dev):
            gamma, stat = _collude_write(kind, rows, targets, live, z, eps, _collude_ref(refs, dev), len(attacking))
        return order, attacking, gamma, stat
    kmax = max(1, max(counts))
    ref_row = row_of(learners[addrs[0]])
    n, dev = ref_row.numel(), ref_row.device
    send = torch.zeros(kmax, n, dtype=torch.float32, device=dev)
    for i, a in enumerate(honest):
        send[i].copy_(row_of(learners[a]))
    recv = torch.empty(len(counts) * kmax, n, dtype=torch.float32, device=dev)
    fed.all_gather_into_tensor_(recv, send)
    rows = [recv[r * kmax + i] for r, c in enumerate(counts) for i in range(c)]
    with on_device(dev):
        gamma, stat = _collude_write(kind, rows, targets, live, z, eps, _collude_ref(refs, dev), len(attacking))
    return order, attacking, gamma, stat


def _mesh_collude(fed: Federation, weights: Dict[str, float], attackers: set, kind: str, z, eps, refs):
    """:func:`collude` over a device mesh, in the manner of ``_mesh_robust``: every device packs its
    honest trainers' rows ([k_max, n], zero-padded), ONE mesh all-gather, then per device the crafted
    row into a result vector unpacked into its attackers. Returns the first device's tensors."""
    addrs = [a for a in weights if a in fed.local_nodes]
    learners = [fed.local_nodes[a].learner for a in addrs]
    ranks = _by_mesh_rank(fed, addrs, learners)
    trainers = {r: [(a, lr) for a, lr in v if float(weights[a]) > 0] for r, v in ranks.items()}
    honest = {r: [(a, lr) for a, lr in v if a not in attackers] for r, v in trainers.items()}
    mine = {r: [(a, lr) for a, lr in v if a in attackers] for r, v in trainers.items()}
    counts = [len(honest[r]) for r in fed.mesh_members]
    order = [a for r in fed.mesh_members for a, _ in honest[r]]
    attacking = [a for r in fed.mesh_members for a, _ in mine[r]]
    if not order or not attacking:
        return None
    _, row_of = _row_fns(learners, "krum")
    kmax = max(counts)
    n = row_of(learners[0]).numel()
    sends, recvs = [], []
    for r in fed.mesh_members:
        dev = fed.devices[r]
        with on_device(dev):
            s_ = torch.zeros(kmax, n, dtype=torch.float32, device=dev)
            for i, (a, lr) in enumerate(honest[r]):
                s_[i].copy_(row_of(lr))
            sends.append(s_)
            recvs.append(torch.empty(len(counts) * kmax, n, dtype=torch.float32, device=dev))
    fed.mesh.all_gather_(recvs, sends)
    fed.mesh_track("collude all_gather")
    first = None
    for r, recv in zip(fed.mesh_members, recvs):
        if not ranks[r]:
            continue
        with on_device(fed.devices[r]):
            rows = [recv[q * kmax + i] for q, c in enumerate(counts) for i in range(c)]
            res = _collude_write(kind, rows, [lr for _, lr in mine[r]], False, z, eps, _collude_ref(refs, recv.device), len(attacking))
            first = first or res
    return order, attacking, first[0], first[1]


def aggregate_generic(fed: Federation, arrived: Dict[str, Tuple[float, Any]], aggregator) -> Any:
    """Any aggregator: all-gather the trainers' wire models and reduce identically on every rank."""
    return fed.run_aggregation(lambda: _generic(fed, arrived, aggregator))


def _generic(fed: Federation, arrived: Dict[str, Tuple[float, Any]], aggregator) -> Any:
    local_models = {a: p[1] for a, p in arrived.items() if p[1] is not None}
    everything: Dict[str, Any] = {}
    for part in fed.all_gather_object(local_models):
        everything.update(part)
    models = [everything[a] for a in sorted(everything)]
    if not models:
        return None
    agg = aggregator.aggregate(models)
    for a in arrived:
        if a in fed.local_nodes:
            fed.local_nodes[a].learner.set_model(agg)
    return agg
