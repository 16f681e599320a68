"""conv12_u8_valid_fwd_flat_kernel: PpoCnn's conv1 -> conv2 forward in one launch over row-aligned flat tiles.

The fused launch changes no sum's order (the output position is not a reduction axis in the forward pass), so EVERY
comparison here is np.array_equal against the two launches it replaces: act1, the relu sign-mask words and act2 of the
stand-alone entry xt_conv12_valid_fwd against xt_layer_fwd_ex(layer 0) + xt_layer_fwd(layer 1, no K split), and a whole
PPO step / forward / 2-epoch train of a PpoCnn with xt_net_set_fwd_fuse12_flat on against off.

Stand-alone cases (T = 9 B rows of conv2 output over all samples; a block owns a run of whole rows):
  B = 1, 4 rows per block    blocks of 4, 4, 1 rows: pieces inside one sample, a one-row block, oy = 8 owning conv1 rows 18 / 19
  B = 2, 11 rows per block   blocks span two samples; the last block is short (7 rows)
  B = 3, 12 rows per block   blocks of 9 + 3, 6 + 6 and 3 rows: 560 conv1 positions (18 tiles: the third tile slot of waves
                             0 and 1) and the largest LDS footprint a launch can have.  (A run of 12 rows starts at a
                             multiple of 12, never at oy = 8, so the 1 + 9 + 2 split of 600 positions cannot occur.)
  B = 7, 11 rows per block   block 4 has 1 + 9 + 1 rows: three pieces
  B = 5, gather              idx = a permutation with one repeated row of an 8-row pool
  B = 29, automatic split    261 rows on 256 blocks of 1 or 2 rows
  B = 343, automatic split   3087 rows: more than 12 per block on 256 blocks, so 258 blocks of 11 or 12 rows
Through the net: B = 40 and B = 33 (the second layer's forward is split over K there, so both settings must take the two
launches) and B = 208 (inside the envelope: the fused launch runs when the switch is on).
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
OHOW1, OHOW2 = 20 * 20, 9 * 9


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _geoms(L):
    g0, g1 = L.ConvGeom(), L.ConvGeom()
    g0.H, g0.W, g0.C, g0.KH, g0.KW, g0.S, g0.PT, g0.PL, g0.OH, g0.OW, g0.N = 84, 84, 4, 8, 8, 4, 0, 0, 20, 20, 32
    g1.H, g1.W, g1.C, g1.KH, g1.KW, g1.S, g1.PT, g1.PL, g1.OH, g1.OW, g1.N = 20, 20, 32, 4, 4, 2, 0, 0, 9, 9, 32
    g0.act = g1.act = L.ACT["relu"]
    return g0, g1, L.InputXform(1, 0.0, 255.0)


@functools.lru_cache(maxsize=None)
def _layers_case(b, rows_per_block, gather):
    """(two launches, fused launch) -> dict(act1, mask, act2) of host arrays each; the fused outputs start from a NaN /
    0xFFFFFFFF prefill"""
    from xingtian_amd import lib as L
    lib = L.load()
    g0, g1, xf = _geoms(L)
    rng = np.random.default_rng(1000 * b + rows_per_block)
    pool = 8 if gather else b
    frames = _dev(rng.integers(0, 256, (pool, 84, 84, 4)).astype(np.uint8))
    idx = None
    if gather:
        rows = rng.permutation(pool)[:b].astype(np.int32)
        rows[b - 1] = rows[1]                                  # one repeated row
        idx = _dev(rows)
    w0 = _dev((rng.standard_normal((256, 32)) * 0.06).astype(np.float32))
    b0 = _dev((rng.standard_normal(32) * 0.5 - 0.2).astype(np.float32))      # some negative biases: both mask values occur
    w1 = _dev((rng.standard_normal((512, 32)) * 0.05).astype(np.float32))
    b1 = _dev((rng.standard_normal(32) * 0.5 - 0.2).astype(np.float32))
    st = L.stream_ptr()

    def outputs(fill):
        act1 = torch.full((b * OHOW1, 32), float("nan") if fill else 0.0, dtype=torch.float32, device="cuda")
        mask = torch.full((b * OHOW1,), -1 if fill else 0, dtype=torch.int32, device="cuda")
        act2 = torch.full((b * OHOW2, 32), float("nan") if fill else 0.0, dtype=torch.float32, device="cuda")
        return act1, mask, act2

    ra1, rm, ra2 = outputs(False)
    written = ctypes.c_int32(0)
    L.check(lib.xt_layer_fwd_ex(ctypes.byref(g0), ctypes.byref(xf), b, L.ptr(frames), L.ptr(idx), L.ptr(w0), L.ptr(b0),
                                L.ptr(ra1), None, 1, st, L.ptr(rm), ctypes.byref(written), None), "xt_layer_fwd_ex")
    assert written.value == 1
    L.check(lib.xt_layer_fwd(ctypes.byref(g1), None, b, L.ptr(ra1), None, L.ptr(w1), L.ptr(b1), L.ptr(ra2), None, 1, st),
            "xt_layer_fwd")
    fa1, fm, fa2 = outputs(True)
    L.check(lib.xt_conv12_valid_fwd(ctypes.byref(g0), ctypes.byref(xf), ctypes.byref(g1), b, L.ptr(frames), L.ptr(idx),
                                    L.ptr(w0), L.ptr(b0), L.ptr(fa1), L.ptr(fm), L.ptr(w1), L.ptr(b1), L.ptr(fa2),
                                    rows_per_block, st), "xt_conv12_valid_fwd")
    torch.cuda.synchronize()
    host = lambda ts: dict(zip(("act1", "mask", "act2"), (t.cpu().numpy() for t in ts)))
    return host((ra1, rm, ra2)), host((fa1, fm, fa2))


LAYER_CASES = [(1, 4, False), (2, 11, False), (3, 12, False), (7, 11, False), (5, 0, True), (29, 0, False), (343, 0, False)]


@pytest.mark.parametrize("b,rows,gather", LAYER_CASES)
def test_fused_launch_is_bitwise_the_two_launches(b, rows, gather):
    ref, got = _layers_case(b, rows, gather)
    assert (ref["act1"] > 0).any() and (ref["act2"] > 0).any()
    words = ref["mask"].view(np.uint32)
    assert ((words != 0) & (words != 0xFFFFFFFF)).any()                    # both mask values occur
    for k in ("act1", "mask", "act2"):
        assert np.array_equal(got[k], ref[k]), (k, int((got[k] != ref[k]).sum()))


@pytest.mark.parametrize("b,rows,gather", LAYER_CASES[:4])
def test_every_output_is_written(b, rows, gather):
    """no element of the NaN / 0xFFFFFFFF prefill is left: every act1 row and mask word has an owner (the halo rows two
    blocks compute are stored by exactly one of them, or the owner's value would not matter), and so has every act2 row"""
    _, got = _layers_case(b, rows, gather)
    assert not np.isnan(got["act1"]).any()
    assert not np.isnan(got["act2"]).any()
    assert not (got["mask"].view(np.uint32) == 0xFFFFFFFF).any()


def test_outside_the_envelope_is_refused():
    from xingtian_amd import lib as L
    lib = L.load()
    g0, g1, xf = _geoms(L)
    one = torch.zeros(1, device="cuda")
    args = lambda ga, gb, rows: (ctypes.byref(ga), ctypes.byref(xf), ctypes.byref(gb), 1, L.ptr(one), None, L.ptr(one),
                                 L.ptr(one), L.ptr(one), None, L.ptr(one), L.ptr(one), L.ptr(one), rows, L.stream_ptr())
    assert lib.xt_conv12_valid_fwd(*args(g0, g1, 13)) != 0                 # more than 12 rows per block
    g1.N = 64
    assert lib.xt_conv12_valid_fwd(*args(g0, g1, 0)) != 0                  # another second layer
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
    assert net.fwd_fuse12_flat_on is True
    net.set_fwd_fuse12_flat(on)
    params = nets.init_params(ospec, seed=seed, bias_scale=0.05)
    net.set_weights({k: v.reshape(net.spec.names[k][1]) for k, v in params.items()})
    return net


@functools.lru_cache(maxsize=None)
def _step_case(b):
    """one applied ppo_step and one forward per switch setting, from the same seed"""
    rng = np.random.default_rng(200 + b)
    obs, lab = _rollout(rng, b + 5)
    idx = rng.permutation(b + 5)[:b].astype(np.int32)
    out = {}
    for on in (False, True):
        net = _net(b, on, seed=7)
        logits, value = net.forward(obs[:b])
        torch.cuda.synchronize()
        fwd = (logits.cpu().numpy().copy(), value.cpu().numpy().copy())
        c = net.make_ppo_cfg(dict(PPO_CFG, BATCH_SIZE=b))
        lo = net.ppo_step(c, net.to_device_obs(obs), _dev(idx), _dev(lab[0]), _dev(lab[1].reshape(-1)),
                          _dev(lab[2].reshape(-1)), _dev(lab[3].reshape(-1)), _dev(lab[4].reshape(-1)), apply=True)
        torch.cuda.synchronize()
        out[on] = dict(fwd=fwd, loss=lo.cpu().numpy().copy(), grads=net.grads_dict(),
                       params=net.params.detach().cpu().numpy().copy())
    return out


@pytest.mark.parametrize("b", [40, 33, 208])
def test_ppo_step_switch_on_against_off(b):
    r = _step_case(b)
    assert np.isfinite(r[True]["loss"]).all() and np.isfinite(r[True]["params"]).all()
    assert np.array_equal(r[True]["loss"], r[False]["loss"])               # every loss term
    for k, g in r[False]["grads"].items():
        assert np.array_equal(r[True]["grads"][k], g), k
    assert np.array_equal(r[True]["params"], r[False]["params"])
    assert not np.array_equal(r[True]["params"], _initial_params())        # (the step did move them)


@functools.lru_cache(maxsize=None)
def _initial_params():
    net = _net(1, True, seed=7)
    return net.params.detach().cpu().numpy().copy()


@pytest.mark.parametrize("b", [40, 33, 208])
def test_forward_switch_on_against_off(b):
    r = _step_case(b)
    for on_v, off_v in zip(r[True]["fwd"], r[False]["fwd"]):
        assert np.isfinite(on_v).all()
        assert np.array_equal(on_v, off_v)


def test_train_graph_replay_against_eager_and_switch_off():
    """2 epochs on 80 rows with batch 33 (minibatches of 33, 33 and 14 rows): eager, captured and replayed updates with the
    switch on are bitwise the eager update with it off; the two settings never share a cached graph"""
    from xingtian_amd import lib as L
    cfg = dict(PPO_CFG, BATCH_SIZE=33, NUM_SGD_ITER=2)
    rng = np.random.default_rng(3)
    n = 80
    obs, lab = _rollout(rng, n)
    perms = np.stack([rng.permutation(n) for _ in range(2)]).astype(np.int32)
    _, ospec = _specs()
    params = nets.init_params(ospec, seed=11, bias_scale=0.05)

    def run(net, bufs, use_graph):
        net.set_weights({k: v.reshape(net.spec.names[k][1]) for k, v in params.items()})
        net.reset_optimizer()
        acc = net.ppo_train(net.make_ppo_cfg(cfg), *bufs, use_graph=use_graph)
        torch.cuda.synchronize()
        a = acc.cpu().numpy()
        assert a[1] == 6.0
        return a[0], net.params.detach().cpu().numpy().copy()

    def mkbufs(net):
        return [net.to_device_obs(obs), _dev(perms), _dev(lab[0]), _dev(lab[1].reshape(-1)), _dev(lab[2].reshape(-1)),
                _dev(lab[3].reshape(-1)), _dev(lab[4].reshape(-1))]

    net_off = _net(33, False, seed=11)
    ref = run(net_off, mkbufs(net_off), False)
    net = _net(33, True, seed=11)
    bufs = mkbufs(net)
    eager = run(net, bufs, False)
    first = run(net, bufs, True)                       # capture + first launch
    captured = L.graph_cache_info(net.handle)["captures"]
    again = run(net, bufs, True)                       # cached replay
    assert L.graph_cache_info(net.handle)["captures"] == captured >= 1
    net.set_fwd_fuse12_flat(False)
    other = run(net, bufs, True)                       # the other setting: its own graph
    assert L.graph_cache_info(net.handle)["captures"] == 2 * captured
    assert np.isfinite(ref[1]).all()
    for got in (eager, first, again, other):
        assert got[0] == ref[0]
        assert np.array_equal(got[1], ref[1])
