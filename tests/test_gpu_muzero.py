"""GPU tests of the MuZero learner (``MuzeroMlp``): the loss head and the conditioned dynamics layer stand-alone, the whole
unrolled step against the float64 restatement of ``tests/muzero_helpers.py`` at the standing bars (loss 1e-4, every
gradient tensor 1e-5), determinism, TF Adam over three trains, inference, the CPU replica, checkpoints and the algorithm
end to end.  Every measured deviation is printed before it is asserted."""
import ctypes
import os
import random

import numpy as np
import pytest
import torch

from tests import muzero_helpers as MH
from tests.dqn_helpers import rel_max

pytestmark = pytest.mark.gpu

PONG = dict(value_range=(-21, 21), reward_range=(-2, 2))            # supports 7 / 3
DEFAULT = dict(value_range=(0, 60000), reward_range=(-300, 300))    # supports 305 / 26
GUARD = 16


def _lib():
    from xingtian_amd import lib as L
    return L, L.load()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _guarded(n, dtype, sentinel):
    """a device buffer of n elements between two runs of GUARD sentinel words -> (whole, view of the n)"""
    whole = torch.full((n + 2 * GUARD,), sentinel, dtype=dtype, device="cuda")
    return whole, whole[GUARD:GUARD + n]


def _guards_intact(whole, n, sentinel):
    w = whole.cpu().numpy()
    return bool((w[:GUARD] == sentinel).all() and (w[GUARD + n:] == sentinel).all())


def _tmax_for(c_top):
    """tmax (tmin = 0) whose compressed value is c_top, by bisection"""
    lo, hi = 0.0, 1e7
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if MH.compress(mid) < c_top else (lo, mid)
    return hi


# ---------------------------------------------------------------------- 1. xt_mz_loss alone
ROW_SPLITS = {1: (1, 1), 3: (3, 1), 64: (2, 32), 65: (5, 13), 1025: (5, 205)}


@pytest.mark.parametrize("n", [2, 3, 7, 26, 64, 65, 305])
def test_loss_head_against_its_float64_twin(n):
    L, lib = _lib()
    rng = np.random.default_rng(n)
    worst = dict(p=0.0, dz=0.0, row=0.0, loss=0.0)
    for rows, (nblk, b) in ROW_SPLITS.items():
        for mode in ("dense", "scalar", "scalar_top", "eps"):
            s_cols = nblk + 1
            z = (rng.standard_normal((rows, n)) * 2.0).astype(np.float32)
            tmin = -3.0
            # natural support: compress(tmax - tmin) in (n - 2, n - 1]; "scalar_top": it lies in [n - 1, n), so the target at
            # max floors onto n - 1 and floor + 1 would leave the row
            tmax = tmin + _tmax_for(n - 1.5 if mode != "scalar_top" else n - 0.75)
            if mode in ("dense", "eps"):
                t = rng.random((b, s_cols, n)).astype(np.float32)
                t /= t.sum(axis=-1, keepdims=True)
                if mode == "eps":        # logits spread over 60, the target's mass on a bin whose probability is below 1e-10
                    z[:, 0], z[:, 1:] = 30.0, -30.0 - rng.random((rows, n - 1)).astype(np.float32)
                    t[:] = 0.0
                    t[:, :, n - 1] = 1.0
                rows_t = np.stack([t[r % b, r // b] for r in range(rows)]).astype(np.float64)
                td, ts = _dev(t), None
            else:
                sc = rng.uniform(tmin, tmax, (b, s_cols))
                sc.flat[0], sc.flat[-1] = tmax + 1.0, tmin - 1.0          # at max (clipped) and at min
                if sc.size > 2:
                    sc.flat[1] = tmin                                     # compresses to the exact integer 0
                th = MH.two_hot(sc, n, tmin, tmax)
                rows_t = np.stack([th[r % b, r // b] for r in range(rows)])
                td, ts = None, _dev(sc)
            scale0, scale_rest = 1.0, 0.2
            p_ref, dz_ref, row_ref = MH.loss_twin(z, nblk, b, rows_t, scale0, scale_rest)
            pw, p = _guarded(rows * n, torch.float32, -7.0)
            dw, dz = _guarded(rows * n, torch.float32, -7.0)
            rw, rl = _guarded(rows, torch.float64, -7.0)
            lw, lo = _guarded(1, torch.float64, -7.0)
            zd = _dev(z)                 # (named: a temporary would be freed, and its block reused, before the call)
            L.check(lib.xt_mz_loss(L.ptr(zd), nblk, b, n, s_cols, L.ptr(td), L.ptr(ts), tmin, tmax, scale0, scale_rest,
                                   L.ptr(p), L.ptr(dz), L.ptr(rl), L.ptr(lo), L.stream_ptr()), "xt_mz_loss")
            torch.cuda.synchronize()
            assert _guards_intact(pw, rows * n, -7.0) and _guards_intact(dw, rows * n, -7.0)
            assert _guards_intact(rw, rows, -7.0) and _guards_intact(lw, 1, -7.0)
            errs = dict(p=rel_max(p.cpu().numpy(), p_ref.reshape(-1)), dz=rel_max(dz.cpu().numpy(), dz_ref.reshape(-1)),
                        row=rel_max(rl.cpu().numpy(), row_ref), loss=rel_max(lo.cpu().numpy(), [row_ref.sum()]))
            if mode == "eps":
                assert abs(row_ref[0] * b * n - 23.02585) < 1e-3      # -log(1e-10): the epsilon sits inside the log
            for k, v in errs.items():
                worst[k] = max(worst[k], v)
            assert errs["p"] <= MH.BAR_GRAD and errs["dz"] <= MH.BAR_GRAD, (rows, mode, errs)
            assert errs["row"] <= MH.BAR_LOSS and errs["loss"] <= MH.BAR_LOSS, (rows, mode, errs)
    print("xt_mz_loss N={}: worst p {p:.2e} dz {dz:.2e} rowloss {row:.2e} loss {loss:.2e}".format(n, **worst))


def test_loss_head_refusals():
    L, lib = _lib()
    p = ctypes.c_void_p(4096)
    err = lambda: lib.xt_last_error().decode()      # noqa: E731
    assert lib.xt_mz_loss(p, 1, 4, 1, 1, p, None, 0.0, 1.0, 1.0, 1.0, None, p, p, None, None) != 0 and "N 1" in err()
    assert lib.xt_mz_loss(p, 3, 4, 7, 2, p, None, 0.0, 1.0, 1.0, 1.0, None, p, p, None, None) != 0 and "S = 2" in err()
    assert lib.xt_mz_loss(p, 1, 4, 7, 1, None, p, 1.0, 1.0, 1.0, 1.0, None, p, p, None, None) != 0 and "tmax" in err()


# ---------------------------------------------------------------------- 2. the conditioned layer, bit for bit
def _cond_case(L, lib, hidden, a, b, nblk, n, actions, c, with_pred, rng):
    m = nblk * b
    h = rng.standard_normal((m, hidden)).astype(np.float32)
    h[rng.random((m, hidden)) < 0.3] = 0.0                       # relu'(h) = 0 there
    w = (rng.standard_normal((hidden + a, n)) * 0.3).astype(np.float32)
    bias = (rng.standard_normal(n) * 0.1).astype(np.float32)
    dy = rng.standard_normal((m, n)).astype(np.float32)
    gp = rng.standard_normal((m, hidden)).astype(np.float32) if with_pred else None
    acts_rows = np.array([actions[r % b, r // b] for r in range(m)])
    yw, y = _guarded(m * n, torch.float32, 9.5)
    # (named device tensors: a temporary would be freed, and its block reused, before the call)
    hd, ad, wd, bd, dyd = _dev(h), _dev(actions.astype(np.int32)), _dev(w), _dev(bias), _dev(dy)
    gpd = None if gp is None else _dev(gp)
    L.check(lib.xt_mz_cond_fwd(L.ptr(hd), L.ptr(ad), nblk, nblk, b, hidden, a, n, L.ptr(wd), L.ptr(bd), 1, L.ptr(y),
                               L.stream_ptr()), "xt_mz_cond_fwd")
    gw, g = _guarded(m * hidden, torch.float32, 9.5)
    count = (hidden + a + 1) * n
    ww, dwb = _guarded(count, torch.float32, 9.5)               # the sentinel: rows of untaken actions must be WRITTEN as zero
    nslab = (m + MH.WGRAD_ROWS - 1) // MH.WGRAD_ROWS
    slabs = torch.full((nslab * count,), 3.25, dtype=torch.float32, device="cuda")
    wt = torch.zeros(n * hidden, dtype=torch.float32, device="cuda")
    L.check(lib.xt_mz_cond_bwd(L.ptr(hd), L.ptr(ad), nblk, nblk, b, hidden, a, n, L.ptr(wd), L.ptr(dyd), L.ptr(gpd), c, L.ptr(g),
                               L.ptr(dwb), L.ptr(slabs), L.ptr(wt), L.stream_ptr()), "xt_mz_cond_bwd")
    torch.cuda.synchronize()
    assert _guards_intact(yw, m * n, 9.5) and _guards_intact(gw, m * hidden, 9.5) and _guards_intact(ww, count, 9.5)
    y_ref = MH.cond_fwd_twin(h, acts_rows, w, bias, hidden)
    g_ref, dwb_ref = MH.cond_bwd_twin(h, acts_rows, w, dy, gp, c, hidden, a)
    tag = (hidden, a, b, nblk, c, with_pred)
    assert np.array_equal(y.cpu().numpy().view(np.uint32), y_ref.reshape(-1).view(np.uint32)), ("fwd", tag)
    assert np.array_equal(g.cpu().numpy().view(np.uint32), g_ref.reshape(-1).view(np.uint32)), ("join", tag)
    got = dwb.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), dwb_ref.view(np.uint32)), ("wgrad", tag)
    return got.reshape(hidden + a + 1, n)


@pytest.mark.parametrize("hidden", [4, 16, 256])
def test_conditioned_layer_bit_for_bit(hidden):
    L, lib = _lib()
    rng = np.random.default_rng(hidden)
    n = {4: 64, 16: 36, 256: 40}[hidden]
    for a in (1, 2, 6, 18):
        for b in (1, 3, 33):
            acts = rng.integers(0, a, (b, 1))
            _cond_case(L, lib, hidden, a, b, 1, n, acts, 1.0, True, rng)                 # k = 0: the join factor is 1
            _cond_case(L, lib, hidden, a, b, 1, n, acts, 0.5, True, rng)                 # k >= 1: halved
            one = np.full((b, 1), a - 1)
            dwb = _cond_case(L, lib, hidden, a, b, 1, n, one, 0.5, False, rng)           # every row takes one action
            if a >= 2:
                assert not dwb[hidden:hidden + a - 1].any() and dwb[hidden + a - 1].any()      # the others read zero, not 9.5
                never = rng.integers(0, a - 1, (b, 1)) + 1                                  # action 0 is never taken
                dwb = _cond_case(L, lib, hidden, a, b, 1, n, never, 1.0, True, rng)
                assert not dwb[hidden].any()
        # stacked blocks (the step's layout: actions [B, nblk]) and more than one slab of rows
        _cond_case(L, lib, hidden, a, 33, 5, n, rng.integers(0, a, (33, 5)), 0.5, True, rng)


# ---------------------------------------------------------------------- 3. the whole step against float64
def _step_case(spec, b, obs_type, seed, tag):
    from xingtian_amd.model.muzero.muzero_model import HipMuzero, obs_as_network_input
    net = HipMuzero(spec, max_batch=b, seed=seed)
    w = MH.seeded_weights(spec, seed)
    net.set_weights(w)
    obs, actions, tv, tr, tp = MH.make_batch(spec, b, seed + 1, obs_type)
    if obs_type == "int8":
        assert (obs >= 128).any()
    loss = float(net.grad_step(obs_as_network_input(spec, obs, obs_type), actions, tv, tr, tp).item())
    grads = net.get_gradients()
    twin = MH.Twin(spec, w)
    loss_ref, grads_ref = twin.loss_and_grads(MH.network_input(spec, obs, obs_type), actions, tv, tr, tp)
    errs = MH.grad_errors(grads, grads_ref)
    worst = max(errs.items(), key=lambda kv: kv[1][0] if kv[1][1] == "rel" else 0.0)
    eloss = abs(loss - loss_ref) / abs(loss_ref)
    print("mz step {}: loss {:.3e} (ref {:.6f}), worst gradient {} {:.3e}".format(tag, eloss, loss_ref, worst[0], worst[1][0]))
    assert np.isfinite(loss) and eloss <= MH.BAR_LOSS, (tag, loss, loss_ref)
    for k, (e, kind) in errs.items():
        assert e <= (MH.BAR_GRAD if kind == "rel" else 1e-12), (tag, k, e, kind)
    return net, twin


@pytest.mark.parametrize("supports", ["pong", "default"])
@pytest.mark.parametrize("unroll", [1, 2, 5])
@pytest.mark.parametrize("b", [1, 3, 32, 33])
def test_step_mlp_against_float64(b, unroll, supports):
    from xingtian_amd.model.muzero.muzero_model import mlp_spec
    spec = mlp_spec((4,), 2, 64, 4, unroll, **(PONG if supports == "pong" else DEFAULT))
    assert (spec.value_support, spec.reward_support) == ((7, 3) if supports == "pong" else (305, 26))
    _step_case(spec, b, "float32", 10 * b + unroll, "mlp B{} U{} {}".format(b, unroll, supports))


# ---------------------------------------------------------------------- 4. determinism, 5. three trains
def test_two_steps_from_the_same_state_give_the_same_bits():
    from xingtian_amd.model.muzero.muzero_model import HipMuzero, mlp_spec, obs_as_network_input
    for spec, b, ot in ((mlp_spec((4,), 2, 64, 4, 5, **DEFAULT), 33, "float32"), (mlp_spec((8,), 6, 64, 16, 2, **PONG), 5, "float32")):
        obs, actions, tv, tr, tp = MH.make_batch(spec, b, 21, ot)
        x = obs_as_network_input(spec, obs, ot)
        runs = []
        for _ in range(2):
            net = HipMuzero(spec, max_batch=b, seed=4)
            net.set_weights(MH.seeded_weights(spec, 4))
            net.grad_step(x, actions, tv, tr, tp)
            g1 = net.grads.cpu().numpy().copy()
            net.grad_step(x, actions, tv, tr, tp)             # again on the same net: nothing stale feeds the second pass
            assert np.array_equal(g1.view(np.uint32), net.grads.cpu().numpy().view(np.uint32))
            net.apply()
            runs.append((g1, net.params.cpu().numpy().copy()))
        assert np.array_equal(runs[0][0].view(np.uint32), runs[1][0].view(np.uint32))
        assert np.array_equal(runs[0][1].view(np.uint32), runs[1][1].view(np.uint32))


def test_three_trains_follow_tf_adam():
    from xingtian_amd.model.muzero.muzero_model import HipMuzero, mlp_spec
    spec = mlp_spec((4,), 2, 64, 4, 5, **PONG)
    net = HipMuzero(spec, max_batch=32, seed=2, lr=1e-3)
    w = {k: v.astype(np.float64) for k, v in MH.seeded_weights(spec, 2).items()}
    net.set_weights(w)
    m = {k: np.zeros_like(v) for k, v in w.items()}
    v2 = {k: np.zeros_like(v) for k, v in w.items()}
    for t in (1, 2, 3):
        obs, actions, tv, tr, tp = MH.make_batch(spec, 32, 50 + t)
        loss = net.train_step(obs, actions, tv, tr, tp)
        loss_ref, g = MH.Twin(spec, w).loss_and_grads(obs.astype(np.float64), actions, tv, tr, tp)
        for k in w:
            w[k], m[k], v2[k] = MH.adam_tf(w[k], g[k], m[k], v2[k], t)
        got = net.get_weights()
        worst = max(rel_max(got[k], w[k]) for k in w)
        print("train {}: loss {:.3e}, worst parameter tensor {:.3e}".format(t, abs(loss - loss_ref) / abs(loss_ref), worst))
        assert abs(loss - loss_ref) / abs(loss_ref) <= MH.BAR_LOSS and worst <= MH.BAR_ADAM


# ---------------------------------------------------------------------- 6. inference, replica, checkpoint
def _model(name, state_dim, action_dim, device, **cfg):
    from xingtian_amd.model import model_builder
    info = {"model_name": name, "state_dim": list(state_dim), "action_dim": action_dim, "type": "learner" if device == "gpu" else None,
            "model_config": dict(cfg, DEVICE=device, SEED=11)}
    return model_builder(info)


def test_inference_and_cpu_replica():
    args, cfg = ("MuzeroMlp", (4,), 2), dict(value_min=-21, value_max=21, reward_min=-2, reward_max=2)
    obs = np.random.default_rng(0).standard_normal((5, 4)).astype(np.float32)
    learner, replica = _model(*args, "gpu", **cfg), _model(*args, "cpu", **cfg)
    spec = learner.spec
    # same seed -> same initial weights
    for k, v in learner.get_weights().items():
        assert np.array_equal(v, replica.get_weights()[k]), k
    learner.set_weights(MH.seeded_weights(spec, 9))
    replica.set_weights(learner.get_weights())                    # what the learner publishes
    assert replica.net.inference_only and not hasattr(replica.net, "train_step")
    twin = MH.Twin(spec, learner.get_weights())
    x64 = MH.network_input(spec, obs, learner.obs_type)
    p, v, h = learner.net.initial(learner._input(obs))
    for got, ref, cpu in zip((p, v, h), twin.initial(x64), replica.net.initial(replica._input(obs))):
        assert rel_max(got, ref) <= MH.BAR_LOSS and rel_max(cpu, ref) <= MH.BAR_LOSS
    acts = np.arange(5) % spec.action_dim
    for got, ref, cpu in zip(learner.net.recurrent(h, acts), twin.recurrent(h, acts), replica.net.recurrent(h, acts)):
        assert rel_max(got, ref) <= MH.BAR_LOSS and rel_max(cpu, ref) <= MH.BAR_LOSS
    # the reference's three methods
    out = learner.initial_inference(obs[:1])
    ref_v = learner.value_transform(twin.initial(x64[:1])[1][0], spec.value_support, spec.value_min, spec.value_max)
    assert isinstance(out.value, float) and abs(out.value - ref_v) <= 1e-4 * max(1.0, abs(ref_v)) and out.reward == 0
    rec = learner.recurrent_inference(out.hidden_state, 1)
    rr = twin.recurrent(out.hidden_state[None], [1])
    assert abs(rec.reward - learner.value_transform(rr[1][0], spec.reward_support, spec.reward_min, spec.reward_max)) <= 1e-4
    vals = learner.value_inference(obs)
    assert vals.shape == (5,) and abs(vals[0] - out.value) <= 1e-4 * max(1.0, abs(out.value))
    cpu_vals = replica.value_inference(obs)
    assert np.abs(vals - cpu_vals).max() <= 1e-4 * max(1.0, np.abs(vals).max())
    with pytest.raises(RuntimeError, match="inference-only"):
        replica.train([obs, None, None], [None, None, None])


def test_checkpoint_resume_is_bit_exact(tmp_path):
    cfg = dict(value_min=-21, value_max=21, reward_min=-2, reward_max=2)
    a = _model("MuzeroMlp", (4,), 2, "gpu", **cfg)
    batches = [MH.make_batch(a.spec, 16, 80 + i) for i in range(3)]
    train = lambda mdl, bt: mdl.train([bt[0], bt[1], np.ones((16, 1))], [bt[2], bt[3], bt[4]])      # noqa: E731
    train(a, batches[0])
    train(a, batches[1])
    path = a.save_model(str(tmp_path / "actor_00001"))
    b = _model("MuzeroMlp", (4,), 2, "gpu", **cfg)
    b.load_model(path)
    assert b.optimizer_restored
    la, lb = train(a, batches[2]), train(b, batches[2])
    assert la == lb
    for k, v in a.get_weights().items():
        assert np.array_equal(v.view(np.uint32), b.get_weights()[k].view(np.uint32)), k
    # a list in the reference's order is taken as well
    c = _model("MuzeroMlp", (4,), 2, "gpu", **cfg)
    c.set_weights(list(a.get_weights().values()))
    assert all(np.array_equal(v, c.get_weights()[k]) for k, v in a.get_weights().items())


# ---------------------------------------------------------------------- 7. the algorithm end to end (MuzeroMlp)
def _trajectory(rng, length, a):
    visits = rng.random((length, a))
    return dict(cur_state=[rng.standard_normal(4).astype(np.float32) for _ in range(length)],
                action=[int(x) for x in rng.integers(0, a, length)], reward=[float(x) for x in rng.uniform(-2, 2, length)],
                root_value=[float(x) for x in rng.uniform(-21, 21, length)],
                target_value=[float(x) for x in rng.uniform(-21, 21, length)],
                child_visits=[list(v / v.sum()) for v in visits])


def test_algorithm_prepares_trains_and_updates_priorities():
    from xingtian_amd.algorithm import alg_builder
    info = dict(model_name="MuzeroMlp", state_dim=[4], action_dim=2, type="learner",
                model_config=dict(reward_min=-2, reward_max=2, value_min=-21, value_max=21, SEED=3))
    cfg = {"train_per_checkpoint": 100, "prepare_times_per_train": 10, "BUFFER_SIZE": 8, "BATCH_SIZE": 8, "instance_num": 1,
           "agent_num": 1}
    alg = alg_builder("Muzero", {"actor": info}, cfg)
    spec = alg.actor.spec
    rng = np.random.default_rng(5)
    random.seed(5)
    assert alg.train() == 0                                    # not enough trajectories yet
    for i in range(8):
        alg.prepare_data(_trajectory(rng, 8 + i, 2))
    assert alg.buff.len() == 8
    before = alg.actor.get_weights()
    outer_before = [alg.buff._sum[i] for i in range(8)]
    loss = alg.train()
    lb = alg.last_batch
    loss_ref, _ = MH.Twin(spec, before).loss_and_grads(MH.network_input(spec, lb["image"], "float32"), lb["actions"], lb["values"],
                                                       lb["rewards"], lb["policies"])
    print("Muzero.train: loss {} vs host-path {} ({:.3e})".format(loss, loss_ref, abs(loss - loss_ref) / abs(loss_ref)))
    assert np.isfinite(loss) and abs(loss - loss_ref) / abs(loss_ref) <= MH.BAR_LOSS
    # every sampled position carries |value(after the train) - target|; the trajectory priorities were written at the
    # batch positions 0 .. 7 (the reference's quirk), each one the mean priority of its trajectory
    after = MH.Twin(spec, alg.actor.get_weights())
    v_support = after.initial(MH.network_input(spec, lb["image"], "float32"))[1]
    last_at = {}
    for i, (g, pos, _) in enumerate(lb["traj_pos"]):
        last_at[(id(g), pos)] = i
    for (gid, pos), i in last_at.items():
        g = lb["traj_pos"][i][0]
        want = max(abs(alg.actor.value_transform(v_support[i], spec.value_support, spec.value_min, spec.value_max)
                       - lb["values"][i, 0]), 1e-5)
        assert abs(g["pos_buff"]._sum[pos] - want) <= 1e-3 * max(1.0, want), (i, pos)
    outer_after = [alg.buff._sum[i] for i in range(8)]
    assert outer_after != outer_before
    assert abs(outer_after[7] - lb["traj_pos"][7][0]["pos_buff"].weight()) <= 1e-12


def test_cnn_builds_only_as_the_replica_and_wrong_observations_are_refused():
    from xingtian_amd.model import model_builder
    from xingtian_amd.model.muzero.muzero_model import HipMuzero, mlp_spec
    info = dict(model_name="MuzeroCnn", state_dim=[84, 84, 4], action_dim=6, type="learner",
                model_config=dict(reward_min=-2, reward_max=2, value_min=-21, value_max=21, obs_type="int8", DEVICE="gpu"))
    with pytest.raises(NotImplementedError, match="Dense representation chains"):
        model_builder(info)
    # an observation array of another element size or width never reaches a kernel
    spec = mlp_spec((4,), 2, 64, 4, 2, **PONG)
    net = HipMuzero(spec, max_batch=4, seed=1)
    obs, actions, tv, tr, tp = MH.make_batch(spec, 4, 1)
    for bad in (obs.astype(np.uint8), obs.astype(np.float64), obs[:, :3].copy(), torch.zeros((4, 4), dtype=torch.uint8, device="cuda")):
        with pytest.raises(TypeError, match="float32"):
            net.grad_step(bad, actions, tv, tr, tp)
        with pytest.raises(TypeError, match="float32"):
            net.initial(bad)
