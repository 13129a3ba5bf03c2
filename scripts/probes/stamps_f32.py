"""Phase timing of the fp32 persistent MLP epoch kernel (MYFYP_NATIVE_LIB=build/stamps/libmyfyp_hip.so).
PEERS grouped peers (default 8), B = 64, two fits; per-step phase durations (us) of peer 0's owner 0
and head 0, and the hand-off latencies between them. The owner K split follows the engine's choice
(MYFYP_F32_KS forces one; at K split > 1 owner 0 is column group 0's K part 0, whose stamp 2 comes
after the in-XCD reduction of the K parts and the reduced slice's publish)."""
import ctypes
import os
import sys
import threading

sys.path.insert(0, os.getcwd())
import numpy as np
import torch

from myfyp_amd.learning.dataset.partition_strategies import RandomIIDPartitionStrategy
from myfyp_amd.learning.dataset.synthetic import synthetic_mnist
from myfyp_amd.learning.frameworks.torch import TorchModel
from myfyp_amd.learning.frameworks.torch.torch_learner import TorchLearner
from myfyp_amd.models import MLP
from myfyp_amd.ops import _native
from myfyp_amd.settings import Settings

Settings.USE_FUSED_KERNELS = True
Settings.MLP_PRECISION = "fp32"
lib = _native.load(required=True)
assert hasattr(lib, "mlp_debug_persistent_f32_stamps"), "not the stamped library"
lib.mlp_debug_persistent_f32_stamps.argtypes = [ctypes.c_void_p]
lib.mlp_debug_persistent_f32_stamps.restype = ctypes.c_int
P, B = int(os.environ.get("PEERS", "8")), 64
parts = synthetic_mnist(60000, 10000, seed=1).generate_partitions(8, RandomIIDPartitionStrategy)
ls = [TorchLearner(TorchModel(MLP(seed=i)), parts[i], f"p{i}", batch_size=B, device="cuda") for i in range(P)]
g = ls[0]._engine.group
assert g.uses_persistent()
print(f"peers {P}, owner K split {g.f32_ks()}, variant {g.f32_variant()}")
for it in range(2):
    ths = [threading.Thread(target=l.fit) for l in ls]
    [t.start() for t in ths]
    [t.join() for t in ths]
torch.cuda.synchronize()
st = np.zeros((2, 128, 18), dtype=np.uint64)  # g_p32_stamps[2][128][18]
assert lib.mlp_debug_persistent_f32_stamps(st.ctypes.data) == 0
st = st.astype(np.int64)
fuse_last = getattr(lib, "mlp_f32_fwd_fuse_last", None)
fused = fuse_last is not None and fuse_last() == 1
print("owner forward:", "fused into C2 (MYFYP_F32_FWD_FUSE=1)" if fused else "separate")
# owner stamps of step t. Separate forward: 0 step start, 7 forward K loop done, 1 reduced + stored,
# 2 flag published, 3 W2 replica done, 4 dH2 seen, 5 C1 done, 6 C2 done (after the step's barrier).
# Fused: 0 step start, 3, 4, 5 as above, 6 C2 with the fused forward done (this wave's, no barrier),
# then H1(t + 1)'s reduction and publish, stamped as step t + 1's 1 and 2.
if fused:
    print("owner: W2 replica | wait dH2 | dH2 load+C1+split | C2 + fused fwd | reduce+stores | flag publish | step")
else:
    print("owner: fwd K loop | reduce+stores | flag publish | W2 replica | wait dH2 | dH2 load+C1+split | C2 (dW1+Adam+X) | step")
print("head : wait H1 | H1 load | H2+PL | PL publish | wait PL | softmax | dH2+publish | off-path | step")
rows = []
for t in range(2, 14):
    o, h, o1 = st[0, t], st[1, t], st[0, t + 1]
    if fused:
        seq = [o[0], o[3], o[4], o[5], o[6], o1[1], o1[2]]
    else:
        seq = [o[0], o[7], o[1], o[2], o[3], o[4], o[5], o[6]]
    do = np.diff(np.array(seq)) / 100.0
    dh = np.diff(h[:9]) / 100.0
    step_o = (o1[0] - o[0]) / 100.0
    step_h = (st[1, t + 1, 0] - h[0]) / 100.0
    rows.append(np.concatenate([do, [step_o], dh, [step_h]]))
    print(f"t={t:2d} owner {' '.join(f'{x:5.2f}' for x in do)} | {step_o:5.2f}   head {' '.join(f'{x:5.2f}' for x in dh)} | {step_h:5.2f}")
m = np.median(np.array(rows), axis=0)
no = len(do) + 1
print("median owner", " ".join(f"{x:5.2f}" for x in m[:no]), " head", " ".join(f"{x:5.2f}" for x in m[no:]))
straight_last = getattr(lib, "mlp_f32_c2_straight_last", None)
if straight_last is not None:
    print("C2 body:", "straight (MYFYP_F32_C2_STRAIGHT=1)" if straight_last() == 1 else "guarded")
if fused:
    # owner slot 8: the end of C2 as lane 0 of wave 1 sees it. Wave 1 owns three K steps, thread 0's wave 0
    # four (K step 24): slot 6 minus slot 8 is how long waves 1..7 wait for wave 0 at the step's barrier
    w1 = np.array([[(st[0, t, 8] - st[0, t, 5]) / 100.0, (st[0, t, 6] - st[0, t, 8]) / 100.0] for t in range(2, 14)])
    print("C2 + fused fwd of wave 1 (us):", " ".join(f"{x:5.2f}" for x in w1[:, 0]), "| median", f"{np.median(w1[:, 0]):5.2f}")
    print("wave 0 ends C2 after wave 1 by (us):", " ".join(f"{x:5.2f}" for x in w1[:, 1]), "| median", f"{np.median(w1[:, 1]):5.2f}")
    # owner slots 10..17: the same point of every wave (lane 0 of waves 0..7), from the end of C1
    wv = np.array([[(st[0, t, 10 + w] - st[0, t, 5]) / 100.0 for w in range(8)] for t in range(2, 14)])
    print("C2 + fused fwd per wave, medians (us): " + " ".join(f"w{w} {np.median(wv[:, w]):5.2f}" for w in range(8)))
    print("last wave ends C2 (us after C1), median:", f"{np.median(wv.max(axis=1)):5.2f}", "| wave 0 after the last of waves 1..7, median:",
          f"{np.median(wv[:, 0] - wv[:, 1:].max(axis=1)):5.2f}")
    k24_last = getattr(lib, "mlp_f32_k24_last", None)
    if k24_last is not None:
        print("K step 24:", "registers (MYFYP_F32_K24=1)" if k24_last() == 1 else "LDS-resident, guarded")
frag_last = getattr(lib, "mlp_f32_dh2_frag_last", None)
if frag_last is not None:
    print("dH2 hand-off:", "fragment image (MYFYP_F32_DH2_FRAG=1)" if frag_last() == 1 else "[b][128] tile staged through LDS")
h1_frag_last = getattr(lib, "mlp_f32_h1_frag_last", None)
if h1_frag_last is not None:
    # (fragment image: the heads' "H1 load" ends when the loads are issued, their latency is in "H2+PL")
    print("H1 hand-off:", "fragment image, H2 and dH2 transposed (MYFYP_F32_H1_FRAG=1)" if h1_frag_last() == 1 else "[b][256] image staged through LDS")
static_d0_last = getattr(lib, "mlp_f32_static_d0_last", None)
if static_d0_last is not None:
    print("input width:", "compile-time constant 784 (MYFYP_F32_STATIC_D0=1)" if static_d0_last() == 1 else "run-time value")
print("owner H1 published -> head H1 seen (us; fused: negative while the head is still in step t - 1):", [round((st[1, t, 1] - st[0, t, 2]) / 100.0, 2) for t in range(2, 10)])
print("head dH2 published -> owner dH2 seen (us):", [round((st[0, t, 4] - st[1, t, 7]) / 100.0, 2) for t in range(2, 10)])
print("head PL published -> head PL all seen (us):", [round((st[1, t, 5] - st[1, t, 4]) / 100.0, 2) for t in range(2, 10)])
