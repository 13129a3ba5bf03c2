"""The fused LeNet-5 oracle (``tests/_lenet_ref.py``) checked on the CPU, and the conditions under which
``tests/test_lenet_fused_gpu.py`` may compare the kernel with it bit for bit.

* Validity: with every bf16 rounding switched off the oracle's loss, gradients (mapped to torch order
  through its own Wf / ``T2E`` / stride-88 maps) and one SGD step equal ``myfyp_amd.models.LeNet5`` in
  float64 under autograd to 1e-10 relative, on random normal inputs (no ties).
* Exactness: for every exact case of ``_lenet_ref.CASES`` each accumulation the GPU test compares bit
  for bit satisfies ``sum |term| / unit < 2^24 / 16``, evaluated on the oracle's own tensors, so every
  partial sum in ANY order is a multiple of the unit that fp32 holds (16 x headroom: the kernel's
  dlogits may sit a bf16 ulp off the oracle's).

  EXACT stages: conv1, conv2 (so p1, p2 and both argmax images), fc1, fc2, fc3 (z3, z4 and the fp32
  logits); ``dl . W3`` (dz4), ``dz4 . W2`` (dz3), ``dz3 . W1`` (dp2, held unrounded in fp32, hence dz2 =
  bf16(dp2)), the conv2 dgrad (dp1) and through it dz1. BOUNDED stages: the loss sum (``__expf`` /
  ``__logf``), dlogits (one bf16 ulp), and every weight / bias gradient sum (2^20 .. 2^27 units:
  ``fp32_bound``).
* Coverage: every exact case has tied maxima in both pools, pooled values that are exactly 0 (mask
  ``> 0``), fc activations that are exactly 0, and 20 % .. 80 % live units per layer.
* Controls: one pixel, one weight of each layer or one label moved changes the oracle's outputs.
"""

import copy
import functools
import math

import pytest
import torch

import _cnn_ops_ref as O
import _conv_ref as C
import _lenet_ref as L

F64 = torch.float64
EXACT = [(B, f) for B, f in L.CASES if f != "randn"]


@functools.lru_cache(maxsize=None)
def _case(B, family, train=True):
    c = L.case(B, family, train)
    return c, L.oracle(c)


# ---------------------------------------------------------------------------------------------
# validity against the torch model
# ---------------------------------------------------------------------------------------------
def _model(c, p):
    from myfyp_amd.models import LeNet5

    m = LeNet5(input_scale=c["scale"]).double()
    with torch.no_grad():
        for n, mod in zip(L.LAYERS, (m.conv1, m.conv2, m.fc1, m.fc2, m.fc3)):
            mod.weight.copy_(c["W"][n][p].reshape(mod.weight.shape))
            mod.bias.copy_(c["b"][n][p])
    return m


def _logits64(m, xu8, scale):
    """``LeNet5.forward`` in float64 up to the logits (the model itself scales in fp32 and takes the
    log-softmax in fp32; ``test_oracle_matches_the_torch_model`` holds this copy to it)."""
    F = torch.nn.functional
    x = xu8.permute(0, 3, 1, 2).double() * scale
    x = F.max_pool2d(F.relu(m.conv1(x)), 2)
    x = F.max_pool2d(F.relu(m.conv2(x)), 2).flatten(1)
    return m.fc3(F.relu(m.fc2(F.relu(m.fc1(x)))))


def _params_flat(m, grad=False):
    mods = (m.conv1, m.conv2, m.fc1, m.fc2, m.fc3)
    pick = (lambda t: t.grad) if grad else (lambda t: t.detach())
    W = {n: pick(mod.weight).reshape(1, *L.TSHAPE[n]).clone() for n, mod in zip(L.LAYERS, mods)}
    b = {n: pick(mod.bias).reshape(1, -1).clone() for n, mod in zip(L.LAYERS, mods)}
    return L.pack_params(W, b)[0]


def _rel(a, b):
    ok = ~torch.isnan(b)
    assert torch.equal(ok, ~torch.isnan(a))
    return float((a[ok] - b[ok]).abs().max() / b[ok].abs().max())


@pytest.mark.parametrize("opt", ["plain", "momentum_nesterov_wd"])
def test_oracle_matches_the_torch_model(opt):
    c = L.case(8, "randn")
    r = L.oracle(c, rnd=L.ident)
    grad = L.grads_to_torch(r["gf"], r["g"])
    hp = L.OPT_VARIANTS[opt]
    master = L.pack_params(c["W"], c["b"])
    mom0 = torch.where(torch.isnan(master), master, torch.zeros_like(master))
    w1, m1 = L.opt_step(master, mom0, grad, r["nb"], hp)
    for p in range(2):
        v = r["nb"][p]
        idx = c["perm"][p, c["offset"]: c["offset"] + v]
        xu8, y = c["xs"][p][idx], c["ys"][p][idx]
        m = _model(c, p)
        sgd = torch.optim.SGD(m.parameters(), lr=hp["lr"], momentum=hp["momentum"], weight_decay=hp["weight_decay"], nesterov=hp["nesterov"])
        logits = _logits64(m, xu8, c["scale"])
        with torch.no_grad():  # the copy above is the model's forward
            assert float((copy.deepcopy(m).float()(xu8).double().exp() - torch.softmax(logits, 1)).abs().max()) < 1e-5
        loss = torch.nn.functional.cross_entropy(logits, y, reduction="sum")
        (loss / v).backward()
        assert abs(float(loss.detach()) - float(r["loss"][p])) <= 1e-10 * float(loss.detach())
        assert float(r["correct"][p]) == float((logits.argmax(1) == y).sum())
        assert _rel(grad[p], _params_flat(m, grad=True)) < 1e-10
        sgd.step()
        assert _rel(w1[p], _params_flat(m)) < 1e-10
    assert torch.equal(torch.nan_to_num(w1[2]), torch.nan_to_num(master[2]))  # the peer without samples keeps its parameters


def test_layout_maps_are_permutations_and_round_trip():
    assert torch.equal(L.E2T[L.T2E], torch.arange(L.F0)) and torch.equal(L.T2E[L.E2T], torch.arange(L.F0))
    c = L.case(2, "randn")
    E = L.to_wf(c["W"])
    back = L.wf_to_torch(E)
    for n in L.LAYERS:
        assert torch.equal(back[n], c["W"][n])
        assert not E[n][:, ~L.real_mask(n)].any()
    flat = L.pack_params(c["W"], c["b"])
    sh = L.shadow_of(flat)
    assert torch.equal(torch.nan_to_num(sh), torch.nan_to_num(torch.where(torch.isnan(sh), sh, L.pack_wf(E))))
    # offsets: shadow tensors 16-byte aligned and disjoint, torch-order tensors disjoint
    for n in L.LAYERS:
        assert L.LAY["w_" + n] % 8 == 0
    assert int((~torch.isnan(sh[0])).sum()) == sum(L._numel(L.TSHAPE[n]) for n in L.LAYERS)
    assert int((~torch.isnan(flat[0])).sum()) == sum(L._numel(L.TSHAPE[n]) + L.TSHAPE[n][0] for n in L.LAYERS)


# ---------------------------------------------------------------------------------------------
# exactness proofs
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,family,train", [(B, f, True) for B, f in EXACT] + [(B, f, False) for B, f in L.EVAL_CASES])
def test_exact_stages_stay_below_the_fp32_limit(B, family, train):
    c, r = _case(B, family, train)
    ratios = L.stage_ratios(r, r["E"])
    print({k: f"2^{math.log2(max(v, 1.0)):.1f}" for k, v in ratios.items()})
    for k, v in ratios.items():
        assert v < L.EXACT_LIM, f"{k}: sum|term| / unit = 2^{math.log2(v):.1f}"
    for k in ("p1", "p2", "z3", "z4", "dl", "dz4", "dz3", "dz2", "dp1"):  # stored values: bf16
        assert torch.equal(C.bf16(r[k]), r[k])
    for k in ("logits", "dp2"):  # held in fp32, unrounded
        assert torch.equal(r[k].float().double(), r[k])
    # the weight-gradient sums are NOT exact: they are compared at fp32_bound
    big = torch.einsum("pbn,pbk->pnk", r["dz3"].abs(), r["p2"].abs()).amax((1, 2)) / (L.gunit(r["dz3"], (1, 2)) * L.gunit(r["p2"], (1, 2)))
    if B == 66:
        assert float(big.max()) > L.EXACT_LIM


def test_the_exactness_measure_sees_a_fine_grid():
    a = torch.tensor([[[1.0, 2.0 ** -20]]], dtype=F64)
    w = torch.ones(1, 2, 1, dtype=F64)
    assert L.mm_ratio(a, w) == 2.0 ** 20 + 1
    assert float(L.gunit(torch.tensor([0.0, 6.0, 0.5], dtype=F64))) == 0.5 and float(L.gunit(torch.zeros(3, dtype=F64))) == 1.0


# ---------------------------------------------------------------------------------------------
# coverage
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,family", EXACT)
def test_cases_hit_ties_zeros_and_live_units(B, family):
    c, r = _case(B, family)
    for p in range(2):
        v = r["nb"][p]
        for acc, bias, cout in ((r["acc1"][p, :v], c["b"]["c1"][p], 6), (r["acc2"][p, :v], c["b"]["c2"][p], 16)):
            w = O.windows(acc[None, ..., :cout])[:, 0]
            top = w.max(0).values
            assert ((w == top).sum(0) > 1).any(), "no tied pooling window"
            assert (top + bias == 0).any(), "no pooled value that is exactly 0"
            # a tie whose FIRST and LAST maximum differ and whose value is live: the tie rule is visible
            assert (((w == top).sum(0) > 1) & (top + bias > 0)).any()
        for k, n in (("z3", L.F1), ("z4", L.F2)):
            assert (r[k][p, :v, :n] == 0).any()
    for k, sl in (("p1", 6), ("p2", L.F0), ("z3", L.F1), ("z4", L.F2)):
        live = torch.cat([(r[k][p, : r["nb"][p]][..., :sl] > 0).reshape(-1) for p in range(2)]).float().mean()
        assert 0.2 <= float(live) <= 0.8, f"{k}: {float(live):.2f} live"
    for p in range(2):
        assert 0 < float(r["correct"][p]) and (r["nb"][p] == 1 or float(r["correct"][p]) < r["nb"][p])
    assert r["nb"] == [B, L.ODD_VALID[B], 0] and r["nb"][1] % 2 == 1
    # the peer without samples: zero images, nothing behind dlogits
    assert not r["dl"][2].any() and not r["gf"][2].nan_to_num().any() and float(r["loss"][2]) == 0.0
    # the partial peer's invalid rows: their forward is the biases' (finite), their gradients zero
    assert not r["dl"][1, r["nb"][1]:].any() and not r["dz3"][1, r["nb"][1]:].any()


@pytest.mark.parametrize("B,family", EXACT[:2])
def test_wrong_rules_change_the_oracle(B, family):
    """The tie rule, the ``> 0`` masks and the first-maximum prediction are visible in the outputs."""
    c, r = _case(B, family)
    E = r["E"]
    last = L.conv_backward(r["dz3"], r, r["x"], E, last=True)
    assert C.differs(last["gW2"], r["gW2"]) and C.differs(last["gW1"], r["gW1"])
    ge = dict(r, live2=(O.maxpool2(r["acc2"], [B] * 3) + c["b"]["c2"][:, None, None, None]) >= 0)
    assert C.differs(L.bwd_pool2(r["dp2"], ge)[0], r["dz2"])


# ---------------------------------------------------------------------------------------------
# controls
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,family", EXACT[:2])
def test_single_element_changes_are_visible(B, family):
    c, r = _case(B, family)
    for label, over in L.single_changes(c, r).items():
        assert C.differs(L.results(L.oracle(c, **over)), L.results(r)), label
