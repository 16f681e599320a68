"""xt_tuning.bwd_fuse21: PpoCnn's conv2 input gradient fused into conv1's weight gradient.

The input-gradient blocks of conv2's fused backward launch keep their 512 pixels of d(act1) in registers (accumulator x
relu' from conv1's sign mask, split exactly into three bf16 planes) and run conv1's weight-gradient loop on them: d(act1) is
never written and conv1's own weight-gradient launch disappears.  The values that enter conv1's weight gradient are the
same fp32 numbers as before; only which 512 positions a slab sums, and in what order, changes.

Batch sizes (100 class positions = 2x2 patches per sample, 128 per block):
  B = 1   one partial tile, the single slab goes straight to the gradient buffer
  B = 6   600 class positions: tile 3 covers 384..511 = three samples, the last tile is ragged
  B = 13  several three-sample tiles plus a ragged tail
and, with the knob at 1 (fused where the flattened first-layer weight gradient would run: >= 200 workgroups of 512 positions):
  B = 254 the last size that keeps the two launches (ceil(25400 / 128) = 199 blocks)
  B = 255 the first size that fuses (200 blocks, the last one ragged), against the oracle

Bound for conv1's kernel and bias gradient against the float64 oracle: err_fused <= max(1e-5, 2 * err_unfused), where
err_unfused is the same step with the knob at 0 on the same inputs; every other tensor stays under the suite's 1e-5 bar.
Conv2's weight-gradient body is reused unchanged, so conv2's gradient is held bitwise like those of conv3, Dense and heads.

Measured rel_err of conv1's gradient against the oracle on MI355X, fused / unfused (the test prints them):
  B = 1   kernel 4.71e-07 / 4.74e-07   bias 4.56e-07 / 5.29e-07
  B = 6   kernel 5.82e-07 / 5.85e-07   bias 7.11e-07 / 6.27e-07
  B = 13  kernel 7.74e-07 / 7.80e-07   bias 8.39e-07 / 8.16e-07
One step at B = 320, knob 1 against knob 0: conv1's kernel / bias gradient differ by 2.1e-7 / 1.7e-7 relative, every other
gradient is bitwise equal.  (The knob ships at 0: DESIGN.md section 4 says why.)
"""
import functools

import numpy as np
import pytest
import torch

from oracle import nets

pytestmark = pytest.mark.gpu

PPO_CFG = dict(LR=2.5e-4, LOSS_CLIPPING=0.1, ENTROPY_LOSS=0.003, VF_CLIP=5.0, CRITIC_LOSS_COEF=1.0,
               MAX_GRAD_NORM=5.0, BATCH_SIZE=64, NUM_SGD_ITER=2)
SENTINEL = 12345.0
L0 = "shared_conv_layer_0"


def rel_err(got, ref):
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    return np.linalg.norm((got - ref).ravel()) / (np.linalg.norm(ref.ravel()) + 1e-30)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _rollout(rng, n, dim, a_dim):
    obs = rng.integers(0, 256, (n, dim, dim, 4)).astype(np.uint8)
    action = rng.integers(0, a_dim, n).astype(np.int32)
    logits = rng.standard_normal((n, a_dim))
    lsm = logits - np.log(np.exp(logits).sum(-1, keepdims=True))
    logp = np.take_along_axis(lsm, action[:, None].astype(np.int64), 1).astype(np.float32)
    adv = rng.standard_normal((n, 1))
    old_v = rng.standard_normal((n, 1)).astype(np.float32)
    target_v = old_v.astype(np.float64) + rng.standard_normal((n, 1))
    return obs, [action, logp, adv, old_v, target_v]


def _load_oracle_params(net, ospec, seed):
    params = nets.init_params(ospec, seed=seed, bias_scale=0.05)
    net.set_weights({k: v.reshape(net.spec.names[k][1]) for k, v in params.items()})
    return params


def _slab_region(net, layer):
    """(float offset, slab capacity, floats per slab) of a layer's weight-gradient slabs in the workspace"""
    import ctypes
    from xingtian_amd import lib as L
    off = (ctypes.c_int64 * 4)()
    L.check(net.lib.xt_net_layer_offsets(net.handle, layer, off), "xt_net_layer_offsets")
    lay = net.spec.layers[layer]
    return int(off[2]), int(off[3]), (lay.KH * lay.KW * lay.C + 1) * lay.N


def _ppo_step_with_knob(knob, spec, ospec, obs, lab, idx, b, slabs_used):
    """one eager PPO gradient step on a fresh net; layer 0's d(act) region is NaN before it and the slab region behind the
    `slabs_used` slabs the fused launch writes carries a sentinel"""
    from xingtian_amd import lib as L
    from xingtian_amd.model.hip_net import HipActorCritic
    old = L.set_tuning(bwd_fuse21=knob)
    try:
        net = HipActorCritic(spec, max_batch=b, seed=0)
        _load_oracle_params(net, ospec, seed=7)
        dact = net.layer_buffers(0, b)[1]
        dact.fill_(float("nan"))
        so, cap, per = _slab_region(net, 0)
        tail = net.workspace[so + slabs_used * per: so + cap * per]
        tail.fill_(SENTINEL)
        c = net.make_ppo_cfg(dict(PPO_CFG, BATCH_SIZE=b))
        lo = net.ppo_step(c, net.to_device_obs(obs), _dev(idx), _dev(lab[0]), _dev(lab[1].reshape(-1)),
                          _dev(lab[2].reshape(-1)), _dev(lab[3].reshape(-1)), _dev(lab[4].reshape(-1)), apply=False)
        torch.cuda.synchronize()
        return dict(loss=float(lo.cpu().numpy()[0]), grads=net.grads_dict(), dact=dact.cpu().numpy().copy(),
                    tail_ok=bool((tail == SENTINEL).all().item()), tail_len=int(tail.numel()))
    finally:
        L.set_tuning(**old)


@functools.lru_cache(maxsize=None)
def _case(b, knob=2):
    """oracle (float64) + the step with the knob at 0 and at `knob` on the same inputs, computed once per batch size"""
    from xingtian_amd.model import netspec
    spec = netspec.ppo_cnn((84, 84, 4), 4, (256,), "relu", True)
    ospec = nets.ppo_cnn_spec((84, 84, 4), 4, (256,), "relu", True)
    rng = np.random.default_rng(100 + b)
    n = b + 5
    obs, lab = _rollout(rng, n, 84, 4)
    idx = rng.permutation(n)[:b].astype(np.int32)
    params = nets.init_params(ospec, seed=7, bias_scale=0.05)
    orc = nets.PpoLearnerOracle(ospec, params, dict(PPO_CFG, BATCH_SIZE=b), np.float64)
    ref = orc.step(obs[idx], lab[0][idx], lab[1][idx].astype(np.float32), lab[2][idx].astype(np.float32),
                   lab[3][idx].astype(np.float32), lab[4][idx].astype(np.float32), apply=False)
    nslab = (100 * b + 127) // 128
    used = nslab if nslab > 1 else 0          # (a single slab is written to the gradient buffer itself)
    off = _ppo_step_with_knob(0, spec, ospec, obs, lab, idx, b, used)
    on = _ppo_step_with_knob(knob, spec, ospec, obs, lab, idx, b, used)
    return ref, off, on


BATCHES = [(1, 2), (6, 2), (13, 2), (255, 1)]      # (batch, knob)


@pytest.mark.parametrize("b,knob", BATCHES)
def test_fused_step_matches_the_float64_oracle(b, knob):
    ref, off, on = _case(b, knob)
    assert abs(on["loss"] - ref["loss"]) <= 1e-4 * max(1.0, abs(ref["loss"])), (on["loss"], ref["loss"])
    for k, r in ref["grads"].items():
        e_on = rel_err(on["grads"][k].reshape(r.shape), r)
        e_off = rel_err(off["grads"][k].reshape(r.shape), r)
        if k.startswith(L0):
            print("bwd_fuse21 B=%d %s rel_err fused %.3e unfused %.3e" % (b, k, e_on, e_off))
            assert e_on <= max(1e-5, 2 * e_off), (k, e_on, e_off)
        else:
            assert e_on < 1e-5, (k, e_on)


@pytest.mark.parametrize("b,knob", BATCHES)
def test_knob_on_against_knob_off(b, knob):
    """everything but conv1's gradient comes from launches (or blocks) the knob does not change: bitwise equal"""
    _, off, on = _case(b, knob)
    assert on["loss"] == off["loss"]
    for k, g in off["grads"].items():
        if k.startswith(L0):
            assert np.isfinite(on["grads"][k]).all(), k
            continue
        assert np.array_equal(on["grads"][k], g), k


@pytest.mark.parametrize("b,knob", BATCHES)
def test_fused_path_ran_and_never_writes_dact1(b, knob):
    _, off, on = _case(b, knob)
    assert np.isnan(on["dact"]).all()                     # the NaN prefill of d(act1) survived the fused step ...
    for k, g in on["grads"].items():
        assert np.isfinite(g).all(), k                    # ... and no gradient was computed from it
    assert np.isfinite(off["dact"]).all()                 # knob 0: conv2's input gradient writes the region
    assert on["tail_len"] > 0 and on["tail_ok"]           # nothing behind the slabs the launch owns was touched


def test_knob_at_1_keeps_the_two_launches_below_200_blocks():
    """B = 254 is 199 blocks of 128 patches (= 199 ranges of 512 positions: the flattened first-layer weight gradient is not
    selected either): with the knob at 1 d(act1) is written and every gradient is bitwise the knob-0 one.  And the library's
    default is 0: at B = 256 a step without any knob set is the two-launch step."""
    from xingtian_amd import lib as L
    from xingtian_amd.model import netspec
    assert L.get_tuning()["bwd_fuse21"] == 0
    spec = netspec.ppo_cnn((84, 84, 4), 4, (256,), "relu", True)
    ospec = nets.ppo_cnn_spec((84, 84, 4), 4, (256,), "relu", True)
    for b, knob in ((254, 1), (256, None)):
        rng = np.random.default_rng(100 + b)
        obs, lab = _rollout(rng, b + 5, 84, 4)
        idx = rng.permutation(b + 5)[:b].astype(np.int32)
        nslab = (100 * b + 127) // 128
        off = _ppo_step_with_knob(0, spec, ospec, obs, lab, idx, b, nslab)
        on = _ppo_step_with_knob(knob if knob is not None else L.get_tuning()["bwd_fuse21"], spec, ospec, obs, lab, idx, b, nslab)
        assert np.isfinite(on["dact"]).all(), (b, knob)
        assert on["loss"] == off["loss"]
        for k, g in off["grads"].items():
            assert np.array_equal(on["grads"][k], g), (b, knob, k)


def test_graph_replay_is_bitwise_the_eager_update():
    """ppo_train with BATCH_SIZE 6 on 13 samples, 2 epochs (minibatches of 6, 6 and 1 row), knob at 2"""
    from xingtian_amd import lib as L
    from xingtian_amd.model import netspec
    from xingtian_amd.model.hip_net import HipActorCritic
    spec = netspec.ppo_cnn((84, 84, 4), 4, (256,), "relu", True)
    ospec = nets.ppo_cnn_spec((84, 84, 4), 4, (256,), "relu", True)
    cfg = dict(PPO_CFG, BATCH_SIZE=6, NUM_SGD_ITER=2)
    rng = np.random.default_rng(3)
    n = 13
    obs, lab = _rollout(rng, n, 84, 4)
    perms = np.stack([rng.permutation(n) for _ in range(2)]).astype(np.int32)
    results = []

    def run(net, bufs, use_graph):
        _load_oracle_params(net, ospec, seed=11)
        net.reset_optimizer()
        acc = net.ppo_train(net.make_ppo_cfg(cfg), *bufs, use_graph=use_graph)
        torch.cuda.synchronize()
        a = acc.cpu().numpy()
        assert a[1] == 6.0
        results.append((a[0] / a[1], net.params.cpu().numpy().copy()))

    def mkbufs(net):
        return [net.to_device_obs(obs), _dev(perms), _dev(lab[0]), _dev(lab[1].reshape(-1)), _dev(lab[2].reshape(-1)),
                _dev(lab[3].reshape(-1)), _dev(lab[4].reshape(-1))]

    old = L.set_tuning(bwd_fuse21=2)
    try:
        net_e = HipActorCritic(spec, max_batch=6, seed=0)
        dact = net_e.layer_buffers(0, 6)[1]
        dact.fill_(float("nan"))
        run(net_e, mkbufs(net_e), False)                   # eager enqueue
        assert torch.isnan(dact).all().item()              # every minibatch took the fused path
        net = HipActorCritic(spec, max_batch=6, seed=0)
        bufs = mkbufs(net)
        run(net, bufs, True)                               # capture + first launch
        run(net, bufs, True)                               # cached graph replay from the same initial state
    finally:
        L.set_tuning(**old)
    assert np.isfinite(results[0][1]).all()
    assert np.array_equal(results[0][1], results[1][1])
    assert np.array_equal(results[1][1], results[2][1])
    assert results[0][0] == results[1][0] == results[2][0]


def _ineligible(which):
    """(net factory, step function) of a net the fused path must leave alone"""
    from xingtian_amd.model import netspec
    from xingtian_amd.model.hip_net import HipActorCritic
    rng = np.random.default_rng(5)
    if which == "impala_opt":
        n, tlen = 8, 4
        spec = netspec.impala_cnn_opt((84, 84, 4), 4, 0.0, 255.0)
        ospec = nets.impala_cnn_opt_spec((84, 84, 4), 4, 0.0, 255.0)
        obs = rng.integers(0, 256, (n, 84, 84, 4)).astype(np.uint8)
        bp = rng.standard_normal((n, 4)).astype(np.float32)
        act = rng.integers(0, 4, n).astype(np.int32)
        done = (rng.random(n) < 0.05).astype(np.uint8)
        rew = rng.choice([-2.0, 0.0, 1.0, 3.0], n).astype(np.float32)

        def step(net):
            c = net.make_impala_cfg(5e-4, 40.0, tlen)
            return net.impala_step(c, _dev(obs), _dev(bp), _dev(act), _dev(done), _dev(rew), apply=False)
    else:
        dim, act_name = (42, "relu") if which == "cnn42" else (84, "tanh")
        n = 7
        spec = netspec.ppo_cnn((dim, dim, 4), 4, (64,), act_name, True)
        ospec = nets.ppo_cnn_spec((dim, dim, 4), 4, (64,), act_name, True)
        obs, lab = _rollout(rng, n + 5, dim, 4)
        idx = rng.permutation(n + 5)[:n].astype(np.int32)

        def step(net):
            c = net.make_ppo_cfg(dict(PPO_CFG, BATCH_SIZE=n))
            return net.ppo_step(c, net.to_device_obs(obs), _dev(idx), _dev(lab[0]), _dev(lab[1].reshape(-1)),
                                _dev(lab[2].reshape(-1)), _dev(lab[3].reshape(-1)), _dev(lab[4].reshape(-1)), apply=False)
    return (lambda: HipActorCritic(spec, max_batch=n, seed=0)), ospec, step, n


@pytest.mark.parametrize("which", ["cnn84_tanh", "cnn42", "impala_opt"])
def test_ineligible_nets_keep_the_two_launches(which):
    """tanh PpoCnn (no sign mask), the 42x42 PpoCnn (another first layer) and ImpalaCnnOpt (SAME padding, 16 channels): with
    the knob at 2 layer 0's d(act) region is written and the gradients are bitwise those of the knob at 0"""
    from xingtian_amd import lib as L
    make, ospec, step, n = _ineligible(which)
    got = {}
    for knob in (0, 2):
        old = L.set_tuning(bwd_fuse21=knob)
        try:
            net = make()
            _load_oracle_params(net, ospec, seed=5)
            dact = net.layer_buffers(0, n)[1]
            dact.fill_(float("nan"))
            step(net)
            torch.cuda.synchronize()
            assert torch.isfinite(dact).all().item(), (which, knob)
            got[knob] = net.grads.detach().cpu().numpy().copy()
        finally:
            L.set_tuning(**old)
    assert np.isfinite(got[2]).all()
    assert np.array_equal(got[0], got[2])
