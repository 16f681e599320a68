"""conv123_u8_valid_fwd_flat_kernel: PpoCnn's conv1 -> conv2 -> conv3 forward in one launch, blocks owning runs of whole
conv3 rows.

The fused launch changes no sum's order, so EVERY comparison is np.array_equal: act1, the relu sign-mask words, act2 and
act3 of the stand-alone entry xt_conv123_valid_fwd against xt_conv12_valid_fwd + xt_layer_fwd(layer 2, no K split), and a
whole PPO step / forward / 2-epoch train of a PpoCnn with xt_net_set_fwd_fuse123_flat on against off.

Stand-alone cases: B = 1, 2, 3, 7, 5 through a gather, 29 and 343 (more blocks than CUs), each with the automatic split
and with 1, 7 and 8 conv3 rows per block (a run inside one sample, exactly one sample, a run that crosses a sample).
Through the net: B = 208 (inside the envelope: the fused launch runs when the switch is on), B = 40 and 33 (conv2's own
forward is split over K there: both settings take the separate launches).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import nets

pytestmark = pytest.mark.gpu

PPO_CFG = dict(LR=2.5e-4, LOSS_CLIPPING=0.1, ENTROPY_LOSS=0.003, VF_CLIP=5.0, CRITIC_LOSS_COEF=1.0,
               MAX_GRAD_NORM=5.0, BATCH_SIZE=64, NUM_SGD_ITER=2)
OHOW1, OHOW2, OHOW3 = 20 * 20, 9 * 9, 7 * 7
KEYS = ("act1", "mask", "act2", "act3")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _geoms(L):
    g0, g1, g2 = L.ConvGeom(), L.ConvGeom(), L.ConvGeom()
    g0.H, g0.W, g0.C, g0.KH, g0.KW, g0.S, g0.PT, g0.PL, g0.OH, g0.OW, g0.N = 84, 84, 4, 8, 8, 4, 0, 0, 20, 20, 32
    g1.H, g1.W, g1.C, g1.KH, g1.KW, g1.S, g1.PT, g1.PL, g1.OH, g1.OW, g1.N = 20, 20, 32, 4, 4, 2, 0, 0, 9, 9, 32
    g2.H, g2.W, g2.C, g2.KH, g2.KW, g2.S, g2.PT, g2.PL, g2.OH, g2.OW, g2.N = 9, 9, 32, 3, 3, 1, 0, 0, 7, 7, 64
    g0.act = g1.act = g2.act = L.ACT["relu"]
    return g0, g1, g2, L.InputXform(1, 0.0, 255.0)


@functools.lru_cache(maxsize=None)
def _inputs(b, gather):
    rng = np.random.default_rng(3000 + b)
    pool = 8 if gather else b
    frames = _dev(rng.integers(0, 256, (pool, 84, 84, 4)).astype(np.uint8))
    idx = None
    if gather:
        rows = rng.permutation(pool)[:b].astype(np.int32)
        rows[b - 1] = rows[1]                                  # one repeated row
        idx = _dev(rows)
    mk = lambda shape, s: _dev((rng.standard_normal(shape) * s).astype(np.float32))
    bias = lambda n: _dev((rng.standard_normal(n) * 0.5 - 0.2).astype(np.float32))      # both signs after every layer
    return frames, idx, (mk((256, 32), 0.06), bias(32), mk((512, 32), 0.05), bias(32), mk((288, 64), 0.05), bias(64))


def _outputs(b, fill):
    f = float("nan") if fill else 0.0
    return (torch.full((b * OHOW1, 32), f, dtype=torch.float32, device="cuda"),
            torch.full((b * OHOW1,), -1 if fill else 0, dtype=torch.int32, device="cuda"),
            torch.full((b * OHOW2, 32), f, dtype=torch.float32, device="cuda"),
            torch.full((b * OHOW3, 64), f, dtype=torch.float32, device="cuda"))


def _host(ts):
    torch.cuda.synchronize()
    return dict(zip(KEYS, (t.cpu().numpy() for t in ts)))


@functools.lru_cache(maxsize=None)
def _reference(b, gather):
    """the conv12 launch, then conv3's own (the reference is computed once per batch and shared by the row splits)"""
    from xingtian_amd import lib as L
    lib = L.load()
    g0, g1, g2, xf = _geoms(L)
    frames, idx, (w0, b0, w1, b1, w2, b2) = _inputs(b, gather)
    a1, m, a2, a3 = _outputs(b, False)
    st = L.stream_ptr()
    L.check(lib.xt_conv12_valid_fwd(ctypes.byref(g0), ctypes.byref(xf), ctypes.byref(g1), b, L.ptr(frames), L.ptr(idx),
                                    L.ptr(w0), L.ptr(b0), L.ptr(a1), L.ptr(m), L.ptr(w1), L.ptr(b1), L.ptr(a2), 0, st),
            "xt_conv12_valid_fwd")
    L.check(lib.xt_layer_fwd(ctypes.byref(g2), None, b, L.ptr(a2), None, L.ptr(w2), L.ptr(b2), L.ptr(a3), None, 1, st),
            "xt_layer_fwd")
    return _host((a1, m, a2, a3))


@functools.lru_cache(maxsize=None)
def _fused(b, rows, gather):
    """the fused launch into a NaN / 0xFFFFFFFF prefill"""
    from xingtian_amd import lib as L
    lib = L.load()
    g0, g1, g2, xf = _geoms(L)
    frames, idx, (w0, b0, w1, b1, w2, b2) = _inputs(b, gather)
    a1, m, a2, a3 = _outputs(b, True)
    L.check(lib.xt_conv123_valid_fwd(ctypes.byref(g0), ctypes.byref(xf), ctypes.byref(g1), ctypes.byref(g2), b, L.ptr(frames),
                                     L.ptr(idx), L.ptr(w0), L.ptr(b0), L.ptr(a1), L.ptr(m), L.ptr(w1), L.ptr(b1), L.ptr(a2),
                                     L.ptr(w2), L.ptr(b2), L.ptr(a3), rows, L.stream_ptr()), "xt_conv123_valid_fwd")
    return _host((a1, m, a2, a3))


LAYER_CASES = [(b, rows, gather) for b, gather in ((1, False), (2, False), (3, False), (7, False), (5, True), (29, False),
                                                   (343, False)) for rows in (0, 1, 7, 8)]


@pytest.mark.parametrize("b,rows,gather", LAYER_CASES)
def test_fused_launch_is_bitwise_the_separate_launches(b, rows, gather):
    ref, got = _reference(b, gather), _fused(b, rows, gather)
    assert all((ref[k] > 0).any() and (ref[k] == 0).any() for k in ("act1", "act2", "act3"))
    words = ref["mask"].view(np.uint32)
    assert ((words != 0) & (words != 0xFFFFFFFF)).any()                    # both mask values occur
    for k in KEYS:
        assert np.array_equal(got[k], ref[k]), (k, int((got[k] != ref[k]).sum()))


@pytest.mark.parametrize("b,rows,gather", [c for c in LAYER_CASES if c[0] in (3, 7)])
def test_every_output_is_written(b, rows, gather):
    """no element of the NaN / 0xFFFFFFFF prefill is left: every row of the three activations and every mask word has an
    owner (the halo rows two blocks compute are stored by exactly one of them, or the owner's value would not matter)"""
    got = _fused(b, rows, gather)
    assert not any(np.isnan(got[k]).any() for k in ("act1", "act2", "act3"))
    assert not (got["mask"].view(np.uint32) == 0xFFFFFFFF).any()


def test_outside_the_envelope_is_refused():
    from xingtian_amd import lib as L
    lib = L.load()
    g0, g1, g2, xf = _geoms(L)
    one = torch.zeros(1, device="cuda")
    args = lambda gc, b, rows: (ctypes.byref(g0), ctypes.byref(xf), ctypes.byref(g1), ctypes.byref(gc), b, L.ptr(one), None,
                                L.ptr(one), L.ptr(one), L.ptr(one), None, L.ptr(one), L.ptr(one), L.ptr(one), L.ptr(one),
                                L.ptr(one), L.ptr(one), rows, L.stream_ptr())
    assert lib.xt_conv123_valid_fwd(*args(g2, 8, 9)) != 0                  # a run of 9 rows that touches three samples
    assert lib.xt_conv123_valid_fwd(*args(g2, 2, 10)) != 0                 # more than 64 conv3 positions
    g2.N = 32
    assert lib.xt_conv123_valid_fwd(*args(g2, 1, 0)) != 0                  # another third layer
    torch.cuda.synchronize()


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


def _specs():
    from xingtian_amd.model import netspec
    return (netspec.ppo_cnn((84, 84, 4), 4, (256,), "relu", True), nets.ppo_cnn_spec((84, 84, 4), 4, (256,), "relu", True))


def _net(b, on, seed):
    from xingtian_amd.model.hip_net import HipActorCritic
    spec, ospec = _specs()
    net = HipActorCritic(spec, max_batch=b, seed=0)
    net.set_fwd_fuse123_flat(on)
    assert net.fwd_fuse123_flat_on is bool(on) and net.fwd_fuse12_flat_on is True
    params = nets.init_params(ospec, seed=seed, bias_scale=0.05)
    net.set_weights({k: v.reshape(net.spec.names[k][1]) for k, v in params.items()})
    return net


def _state(net):
    torch.cuda.synchronize()
    return dict(params=net.params.detach().cpu().numpy().copy(), adam_m=net.adam_m.cpu().numpy().copy(),
                adam_v=net.adam_v.cpu().numpy().copy(), adam_state=net.adam_state.cpu().numpy().copy())


@functools.lru_cache(maxsize=None)
def _step_case(b):
    """one forward and one applied ppo_step per switch setting, from the same seed"""
    rng = np.random.default_rng(400 + b)
    obs, lab = _rollout(rng, b + 5)
    idx = rng.permutation(b + 5)[:b].astype(np.int32)
    out = {}
    for on in (False, True):
        net = _net(b, on, seed=7)
        logits, value = net.forward(obs[:b])
        torch.cuda.synchronize()
        fwd = (logits.cpu().numpy().copy(), value.cpu().numpy().copy())
        fwd_took = net.last_step_report()["fwd_fuse123"]
        c = net.make_ppo_cfg(dict(PPO_CFG, BATCH_SIZE=b))
        lo = net.ppo_step(c, net.to_device_obs(obs), _dev(idx), _dev(lab[0]), _dev(lab[1].reshape(-1)),
                          _dev(lab[2].reshape(-1)), _dev(lab[3].reshape(-1)), _dev(lab[4].reshape(-1)), apply=True)
        torch.cuda.synchronize()
        out[on] = dict(fwd=fwd, loss=lo.cpu().numpy().copy(), grads=net.grads_dict(), state=_state(net),
                       took=(fwd_took, net.last_step_report()["fwd_fuse123"]))
    return out


@pytest.mark.parametrize("b", [208, 40, 33])
def test_ppo_step_and_forward_switch_on_against_off(b):
    r = _step_case(b)
    assert r[False]["took"] == (0, 0)
    assert r[True]["took"] == ((1, 1) if b == 208 else (0, 0))     # the report says which forward ran
    for on_v, off_v in zip(r[True]["fwd"], r[False]["fwd"]):
        assert np.isfinite(on_v).all() and np.array_equal(on_v, off_v)
    assert np.isfinite(r[True]["loss"]).all() and np.array_equal(r[True]["loss"], r[False]["loss"])      # every loss term
    for k, g in r[False]["grads"].items():
        assert np.array_equal(r[True]["grads"][k], g), k
    for k, v in r[False]["state"].items():
        assert np.isfinite(v).all() and np.array_equal(r[True]["state"][k], v), k
    assert (r[True]["state"]["adam_m"] != 0).any()                             # (the step did run)


def _train_setup(b, n, seed):
    cfg = dict(PPO_CFG, BATCH_SIZE=b, NUM_SGD_ITER=2)
    rng = np.random.default_rng(seed)
    obs, lab = _rollout(rng, n)
    perms = np.stack([rng.permutation(n) for _ in range(2)]).astype(np.int32)
    params = nets.init_params(_specs()[1], seed=11, bias_scale=0.05)
    steps = 2 * ((n + b - 1) // b)

    def run(net, bufs, use_graph):
        net.set_weights({k: v.reshape(net.spec.names[k][1]) for k, v in params.items()})
        net.reset_optimizer()
        acc = net.ppo_train(net.make_ppo_cfg(cfg), *bufs, use_graph=use_graph)
        torch.cuda.synchronize()
        a = acc.cpu().numpy().copy()
        assert a[1] == float(steps)
        return dict(_state(net), loss_acc=a)

    def mkbufs(net):
        return [net.to_device_obs(obs), _dev(perms), _dev(lab[0]), _dev(lab[1].reshape(-1)), _dev(lab[2].reshape(-1)),
                _dev(lab[3].reshape(-1)), _dev(lab[4].reshape(-1))]

    return run, mkbufs


def _same(got, ref):
    for k, v in ref.items():
        assert np.isfinite(v).all() and np.array_equal(got[k], v), k


@pytest.mark.parametrize("b,n", [(208, 250), (40, 90), (33, 80)])
def test_train_eager_captured_and_replayed_against_switch_off(b, n):
    """2 epochs (minibatches of b rows and a shorter last one): eager, captured and replayed updates with the switch on
    are bitwise the eager update with it off"""
    from xingtian_amd import lib as L
    run, mkbufs = _train_setup(b, n, seed=5)
    net_off = _net(b, False, seed=11)
    ref = run(net_off, mkbufs(net_off), False)
    net = _net(b, True, seed=11)
    bufs = mkbufs(net)
    _same(run(net, bufs, False), ref)
    _same(run(net, bufs, True), ref)                   # capture + first launch
    captured = L.graph_cache_info(net.handle)["captures"]
    assert captured >= 1
    _same(run(net, bufs, True), ref)                   # cached replay
    assert L.graph_cache_info(net.handle)["captures"] == captured


def test_flipping_the_switch_between_trains_never_replays_the_other_graph():
    from xingtian_amd import lib as L
    run, mkbufs = _train_setup(208, 250, seed=6)
    net_off = _net(208, False, seed=11)
    ref = run(net_off, mkbufs(net_off), False)
    net = _net(208, True, seed=11)
    bufs = mkbufs(net)
    _same(run(net, bufs, True), ref)
    captured = L.graph_cache_info(net.handle)["captures"]
    assert net.last_step_report()["fwd_fuse123"] in (0, 1)           # (the last minibatch is short: either form)
    net.set_fwd_fuse123_flat(False)
    _same(run(net, bufs, True), ref)                   # the other setting: its own graphs
    assert L.graph_cache_info(net.handle)["captures"] == 2 * captured
    net.set_fwd_fuse123_flat(True)
    _same(run(net, bufs, True), ref)                   # back: the first graphs, replayed
    assert L.graph_cache_info(net.handle)["captures"] == 2 * captured
