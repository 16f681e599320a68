"""The table-free form of the Dense instance of the fused backward launch (xt_bwd_dense_lean_set, default 1).

The switch changes how the weight-gradient blocks ADDRESS their rows and where the bias sums take the fp32 dy from, never
a sum's order, so EVERY comparison here is np.array_equal of the switch at 1 against the switch at 0 on the same inputs:
dx, dW | db and the reported path of xt_layer_bwd, and the parameters, Adam moments, step state (gradient norm, clip
factor) and loss accumulator of a PpoCnn after one PPO step and after a 2-epoch ppo_train (eager, captured, replayed) --
the latter cover the squared-norm partials the weight-gradient blocks leave for the optimiser.

xt_layer_bwd cases, (K, N) at B: 32-row steps of the reduction over B
  (3136, 256) at 1      one partial step
  (3136, 256) at 33     two steps, the second ragged
  (3136, 256) at 129    five steps: wraps the four register stages
  (3136, 256) at 320    the benchmark's shape
  (576, 64) at 50       nine row tiles, one column tile
  (64, 64) at 200       a single tile: its bias block is its only block
  (64, 64) at 200, split in two slabs (an extra case): a block's row range ends inside the tensor
dy carries exact zeros (every fifth row and a sprinkling of entries), so a dropped or doubled row would show.
Through the net: B = 33 and 40 (step + train), and one step at B = 261, the smallest kind of batch at which the lean
launch has fewer head blocks than head tiles.
"""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

from oracle import nets

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PPO_CFG = dict(LR=2.5e-4, LOSS_CLIPPING=0.1, ENTROPY_LOSS=0.003, VF_CLIP=5.0, CRITIC_LOSS_COEF=1.0,
               MAX_GRAD_NORM=5.0, BATCH_SIZE=64, NUM_SGD_ITER=2)
# (K, N, B, msplit asked for, producer's activation)
LAYER_CASES = [(3136, 256, 1, 1, "relu"), (3136, 256, 33, 1, "tanh"), (3136, 256, 129, 1, "relu"),
               (3136, 256, 320, 2, "tanh"), (576, 64, 50, 1, "relu"), (64, 64, 200, 1, "tanh"), (64, 64, 200, 2, "relu")]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _header_int(name):
    with open(os.path.join(ROOT, "include", "xt_mi355x.h")) as f:
        return int(re.search(r"#define\s+{}\s+(\d+)".format(name), f.read()).group(1))


@pytest.fixture(autouse=True)
def _switch_back_on():
    from xingtian_amd import lib as L
    L.require_gpu()
    yield
    torch.cuda.synchronize()
    L.set_bwd_dense_lean(True)


@functools.lru_cache(maxsize=None)
def _layer_case(k, n, b, msplit, act, wx6=1):
    """{switch: (dx, dwb, path)} of one xt_layer_bwd per setting on the same device buffers' contents"""
    from xingtian_amd import lib as L
    lib = L.load()
    rng = np.random.default_rng(k + 7 * n + 13 * b + msplit)
    z = rng.standard_normal((b, k)).astype(np.float32)
    x = nets.act_fwd(z.astype(np.float64), act).astype(np.float32)
    w = (rng.standard_normal((k, n)) / np.sqrt(k)).astype(np.float32)
    dy = rng.standard_normal((b, n)).astype(np.float32)
    dy[::5] = 0.0
    dy[rng.random((b, n)) < 0.05] = 0.0
    g = L.ConvGeom()
    g.H = g.W = g.KH = g.KW = g.S = g.OH = g.OW = 1
    g.PT = g.PL = 0
    g.C, g.N, g.act = k, n, L.ACT["relu"]
    nw = (k + 1) * n
    xd, dyd, wd = _dev(x), _dev(dy), _dev(w)
    old = L.set_tuning(dense_wgrad_x6=wx6)
    out = {}
    try:
        for on in (0, 1):
            L.set_bwd_dense_lean(on)
            dx = torch.full((b * k,), float("nan"), dtype=torch.float32, device="cuda")
            dwb = torch.full((nw,), float("nan"), dtype=torch.float32, device="cuda")
            slabs = torch.full((msplit * nw,), float("nan"), dtype=torch.float32, device="cuda")
            path = ctypes.c_int32(-1)
            L.check(lib.xt_layer_bwd(ctypes.byref(g), b, L.ptr(xd), None, L.ptr(dyd), L.ptr(wd), L.ACT[act], None,
                                     L.ptr(dx), L.ptr(dwb), L.ptr(slabs), msplit, msplit, None, ctypes.byref(path)),
                    "xt_layer_bwd")
            torch.cuda.synchronize()
            out[on] = (dx.cpu().numpy().copy(), dwb.cpu().numpy().copy(), path.value)
    finally:
        L.set_tuning(**old)
        L.set_bwd_dense_lean(True)
    ref_b = dy.astype(np.float64).sum(0)
    return out, ref_b


@pytest.mark.parametrize("k,n,b,msplit,act", LAYER_CASES, ids=["k%d_n%d_b%d_s%d" % c[:4] for c in LAYER_CASES])
def test_layer_bwd_switch_on_against_off(k, n, b, msplit, act):
    out, ref_b = _layer_case(k, n, b, msplit, act)
    for on in (0, 1):      # both settings stay on the Dense instance: no case falls to another kernel
        assert out[on][2] & 0xFF == _header_int("XT_BWD_PATH_PF_GENERIC"), (on, out[on][2])
    assert out[1][2] == out[0][2]
    assert np.isfinite(out[1][0]).all() and np.isfinite(out[1][1]).all()
    assert np.array_equal(out[1][0], out[0][0])
    assert np.array_equal(out[1][1], out[0][1])
    # (the bias gradient is there at all: float64 column sums of dy, fp32 rounding of at most b additions)
    assert np.abs(out[1][1][k * n:] - ref_b).max() <= 1e-6 * b * np.abs(ref_b).max() + 1e-30


@pytest.mark.parametrize("k,n,b,msplit,act", [LAYER_CASES[2], LAYER_CASES[5]], ids=["k3136_b129", "k64_b200"])
def test_layer_bwd_fp32_weight_gradient_switch_on_against_off(k, n, b, msplit, act):
    """dense_wgrad_x6 = 0: the lean prologue does not depend on the bf16x6 stage"""
    out, _ = _layer_case(k, n, b, msplit, act, wx6=0)
    assert out[1][2] == out[0][2] and out[1][2] & 0xFF == _header_int("XT_BWD_PATH_PF_GENERIC")
    assert np.isfinite(out[1][1]).all()
    assert np.array_equal(out[1][0], out[0][0])
    assert np.array_equal(out[1][1], out[0][1])


# ------------------------------------------------------------------ through the net
def _rollout(rng, n):
    obs = rng.integers(0, 256, (n, 84, 84, 4)).astype(np.uint8)
    action = rng.integers(0, 4, n).astype(np.int32)
    logits = rng.standard_normal((n, 4))
    lsm = logits - np.log(np.exp(logits).sum(-1, keepdims=True))
    logp = np.take_along_axis(lsm, action[:, None].astype(np.int64), 1).astype(np.float32)
    adv = rng.standard_normal((n, 1))
    old_v = rng.standard_normal((n, 1)).astype(np.float32)
    target_v = old_v.astype(np.float64) + rng.standard_normal((n, 1))
    return obs, [action, logp, adv, old_v, target_v]


def _net(b):
    from xingtian_amd.model import netspec
    from xingtian_amd.model.hip_net import HipActorCritic
    return HipActorCritic(netspec.ppo_cnn((84, 84, 4), 4, (256,), "relu", True), max_batch=b, seed=0)


def _load(net, seed):
    params = nets.init_params(nets.ppo_cnn_spec((84, 84, 4), 4, (256,), "relu", True), seed=seed, bias_scale=0.05)
    net.set_weights({k: v.reshape(net.spec.names[k][1]) for k, v in params.items()})
    net.reset_optimizer()


def _snapshot(net, acc):
    torch.cuda.synchronize()
    return dict(params=net.params.detach().cpu().numpy().copy(), m=net.adam_m.cpu().numpy().copy(),
                v=net.adam_v.cpu().numpy().copy(), state=net.adam_state.cpu().numpy().copy(),
                acc=acc.cpu().numpy().copy())


def _same(a, b):
    for key in ("params", "m", "v", "state", "acc"):
        assert np.array_equal(a[key], b[key]), key


def test_ppo_step_with_shared_head_blocks_switch_on_against_off():
    """B = 261: 245 input-gradient + 196 weight-gradient blocks leave 71 of the 512 workgroup slots for the 132 head
    weight-gradient tiles (33 chunks of 8 samples, the last one of 5), so with the switch at 1 a head block walks two tiles:
    gradients (head slabs included, through the reduction), parameters, moments and step state are those of the switch at 0"""
    from xingtian_amd import lib as L
    b = 261
    rng = np.random.default_rng(77)
    obs, lab = _rollout(rng, b)
    net = _net(b)
    c = net.make_ppo_cfg(dict(PPO_CFG, BATCH_SIZE=b))
    lab_d = [_dev(lab[0])] + [_dev(a.reshape(-1)) for a in lab[1:]]
    obs_d = net.to_device_obs(obs)
    out = {}
    for on in (False, True):
        L.set_bwd_dense_lean(on)
        _load(net, seed=9)
        lo = net.ppo_step(c, obs_d, None, *lab_d, apply=True)
        out[on] = _snapshot(net, lo)
        out[on]["grads"] = net.grads.cpu().numpy().copy()
    assert np.isfinite(out[True]["grads"]).all() and out[True]["grads"].any()
    assert np.array_equal(out[True]["grads"], out[False]["grads"])
    _same(out[True], out[False])


@pytest.mark.parametrize("b", [33, 40])
def test_ppo_step_then_train_switch_on_against_off(b):
    """one applied PPO step, then a 2-epoch ppo_train on 2 b + 14 rows (minibatches of b, b and 14 rows) eager, captured
    and replayed: parameters, Adam moments, step state and loss accumulator with the switch at 1 are those with it at 0;
    the two settings never share a cached graph"""
    from xingtian_amd import lib as L
    rng = np.random.default_rng(500 + b)
    n = 2 * b + 14
    obs, lab = _rollout(rng, n)
    idx = rng.permutation(n)[:b].astype(np.int32)
    perms = np.stack([rng.permutation(n) for _ in range(2)]).astype(np.int32)
    cfg = dict(PPO_CFG, BATCH_SIZE=b, NUM_SGD_ITER=2)
    net = _net(b)
    c = net.make_ppo_cfg(cfg)
    lab_d = [_dev(lab[0])] + [_dev(a.reshape(-1)) for a in lab[1:]]
    obs_d = net.to_device_obs(obs)

    def step():
        _load(net, seed=5)
        lo = net.ppo_step(c, obs_d, _dev(idx), *lab_d, apply=True)
        return _snapshot(net, lo)

    def train(use_graph):
        _load(net, seed=5)
        acc = net.ppo_train(c, obs_d, _dev(perms), *lab_d, use_graph=use_graph)
        s = _snapshot(net, acc)
        assert s["acc"][1] == 6.0
        return s

    L.set_bwd_dense_lean(False)
    ref_step, ref_train = step(), train(False)
    ref_graph = train(True)
    captures_off = L.graph_cache_info(net.handle)["captures"]
    L.set_bwd_dense_lean(True)
    got_step, eager = step(), train(False)
    first = train(True)                                # capture + first launch
    captures_on = L.graph_cache_info(net.handle)["captures"]
    assert captures_on == 2 * captures_off >= 2        # (its own graphs)
    again = train(True)                                # cached replay
    assert L.graph_cache_info(net.handle)["captures"] == captures_on
    assert np.isfinite(ref_train["params"]).all() and ref_step["state"].any()
    _same(got_step, ref_step)
    for got in (ref_graph, eager, first, again):
        _same(got, ref_train)
