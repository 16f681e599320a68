"""GPU tests (run with -m gpu on an MI355X) of continuous-action PPO on the default host path and of the fused DiagGaussian
head, through ``alg_builder("PPO")``:

  mlp3   PpoMlp (3,)  A = 1, tanh (64, 64), separate trunks        examples/pendulum_ppo.yaml's network
  mlp5   PpoMlp (5,)  A = 3, tanh (32,), shared trunk
  mlp11  PpoMlp (11,) A = 6, tanh [128, 64]: the last layer has K = 128 and one tile -> split-K, PART instance
  cnn    PpoCnn [84, 84, 3] uint8, A = 8, relu, hidden [256], shared trunk

1. a DiagGaussian rollout (float actions, vector widths that are no multiple of 4) is streamed by prepare_data;
2. the streamed update equals the uploaded one bit for bit (same kernels on the same device bytes);
3. raw trajectories (value [T+1] / reward / done): one ragged GAE per rollout, bit-exact against oracle.returns.gae;
4. pinned sources, buffer growth, [n, A] float actions and device-side padding of the observation width;
5. GAUSS_FUSED_HEAD against the float64 oracle with the bars of test_gpu_learner.py::test_gauss_ppo_mlp_update_vs_oracle
   (loss 1e-5, every gradient 1e-4, loss after train 1e-4, weight deltas 5e-3), graph replay, fallbacks outside the envelope;
6. switch hygiene and TRAIN_STATS with the fused head (helpers and tolerances of tests/test_gpu_train_stats.py)."""
import ctypes

import numpy as np
import pytest
import torch

import test_gpu_train_stats as TS
from oracle import nets, returns
from test_gpu_heads_branch import decode_head_path
from test_gpu_learner import rel_err

pytestmark = pytest.mark.gpu

BATCH, EPOCHS = 40, 3
OCFG = dict(LR=0.0003, LOSS_CLIPPING=0.2, ENTROPY_LOSS=0.01, VF_CLIP=10.0, CRITIC_LOSS_COEF=1.0, MAX_GRAD_NORM=5.0,
            BATCH_SIZE=BATCH, NUM_SGD_ITER=EPOCHS)
SHAPES = {
    "mlp3": dict(model_name="PpoMlp", state_dim=[3], action_dim=1, act="tanh", hidden=[64, 64], share=False, lens=(37, 50, 23)),
    "mlp5": dict(model_name="PpoMlp", state_dim=[5], action_dim=3, act="tanh", hidden=[32], share=True, lens=(37, 50, 23)),
    "mlp11": dict(model_name="PpoMlp", state_dim=[11], action_dim=6, act="tanh", hidden=[128, 64], share=False,
                  lens=(37, 50, 23)),
    "cnn": dict(model_name="PpoCnn", state_dim=[84, 84, 3], action_dim=8, act="relu", hidden=[256], share=True,
                lens=(25, 31), input_dtype="uint8"),
}
GAUSS_FUSED = 4         # XT_HEAD_PATH_PPO_GAUSS_FUSED


def build(kind, **over):
    from xingtian_amd.algorithm import alg_builder
    s = SHAPES[kind]
    cfg = dict(OCFG, VF_SHARE_LAYERS=s["share"], activation=s["act"], hidden_sizes=list(s["hidden"]),
               action_type="DiagGaussian", SEED=5, USE_HIP_GRAPH=False)
    cfg.update(over)
    actor = dict(model_name=s["model_name"], state_dim=list(s["state_dim"]), action_dim=s["action_dim"],
                 input_dtype=s.get("input_dtype", "float32"), model_config=cfg)
    return alg_builder("PPO", {"actor": actor}, {"instance_num": len(s["lens"]), "agent_num": 1})


@pytest.fixture(autouse=True)
def _model_defaults_stay():
    """The model constructor writes the keys of its model_config into its module's constants (the reference's
    import_config), where they would become the defaults of every later test that leaves a key out: put them back."""
    import xingtian_amd.model.ppo.ppo as M
    keys = ("LR", "BATCH_SIZE", "CRITIC_LOSS_COEF", "ENTROPY_LOSS", "LOSS_CLIPPING", "MAX_GRAD_NORM", "NUM_SGD_ITER", "SUMMARY",
            "VF_CLIP")
    saved = {k: getattr(M, k) for k in keys}
    yield
    for k, v in saved.items():
        setattr(M, k, v)


_ROLLOUTS = {}


def rollout(kind):
    """trajectories of unequal length whose total (110 / 56) is no multiple of the batch, injected shuffles; built once"""
    if kind in _ROLLOUTS:
        return _ROLLOUTS[kind]
    s = SHAPES[kind]
    rng = np.random.default_rng(zlib_seed(kind))
    sd, ad = tuple(s["state_dim"]), s["action_dim"]
    trajs = []
    for t in s["lens"]:
        obs = rng.integers(0, 256, (t,) + sd).astype(np.uint8) if s.get("input_dtype") == "uint8" \
            else rng.uniform(-1, 1, (t,) + sd).astype(np.float32)
        value = rng.standard_normal((t + 1, 1)).astype(np.float32)
        reward = rng.standard_normal(t)
        done = rng.random(t) < 0.1
        adv, old_v, tgt = returns.gae(value, reward.copy(), done)
        trajs.append(dict(cur_state=obs, action=rng.standard_normal((t, ad)).astype(np.float32),
                          logp=(-np.abs(rng.standard_normal((t, 1))) - 0.5).astype(np.float32), adv=adv, old_value=old_v,
                          target_value=tgt, value=value, reward=reward, done=done))
    n = sum(s["lens"])
    perms = np.stack([rng.permutation(n) for _ in range(EPOCHS)]).astype(np.int32)
    _ROLLOUTS[kind] = dict(trajs=trajs, perms=perms, n=n)
    return _ROLLOUTS[kind]


def zlib_seed(kind):
    import zlib
    return zlib.crc32(("gauss_stream_" + kind).encode())


WITH_ADV = ("cur_state", "action", "logp", "adv", "old_value", "target_value")
RAW = ("cur_state", "action", "logp", "value", "reward", "done")


def feed(alg, kind, keys=WITH_ADV):
    r = rollout(kind)
    for tr in r["trajs"]:
        alg.prepare_data({k: tr[k] for k in keys})
    return alg.train(perms=r["perms"])


def state_bits(alg):
    net = alg.actor.net
    torch.cuda.synchronize()
    return [net.params.cpu().numpy().view(np.uint32).copy(), net.adam_m.cpu().numpy().view(np.uint32).copy(),
            net.adam_v.cpu().numpy().view(np.uint32).copy()]


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def set_logstd(alg, seed=1):
    """a non-zero pi_logstd (the constructor's is zero), the same for every net of a comparison"""
    w = alg.get_weights()
    w["pi_logstd"] = (np.random.default_rng(seed).standard_normal(w["pi_logstd"].shape) * 0.3).astype(np.float32)
    alg.set_weights(w)
    return alg.get_weights()


# ---------------------------------------------------------------- 1, 2: the rollout is streamed, and nothing changes
@pytest.mark.parametrize("kind", sorted(SHAPES))
def test_gauss_rollout_is_streamed_and_gives_the_bits_of_the_uploaded_update(kind):
    r = rollout(kind)
    out = {}
    for stream in (True, False):
        alg = build(kind, STREAM_INGEST=stream)
        set_logstd(alg)
        assert bool(alg.actor.stream_ingest) == stream
        losses = []
        for rep in range(2):                       # (the second update streams into the other buffer set)
            for tr in r["trajs"]:
                alg.prepare_data({k: tr[k] for k in WITH_ADV})
            if stream:
                assert alg.actor.ingested() == r["n"]
            else:
                assert alg.actor.ingested() == 0
            losses.append(np.float32(alg.train(perms=r["perms"])).tobytes())
        out[stream] = (losses, state_bits(alg))
        assert alg.actor.net.last_head_path() == TS_L().NET_HEAD_GAUSS       # (the default head: the three launches)
    assert out[True][0] == out[False][0]
    assert same(out[True][1], out[False][1])


def TS_L():
    from xingtian_amd import lib
    return lib


# ---------------------------------------------------------------- 3: raw trajectories, GAE once per rollout on the device
@pytest.mark.parametrize("kind", ["mlp3", "mlp11"])
def test_raw_gauss_trajectories_get_one_ragged_gae_bit_exact(kind):
    r = rollout(kind)
    n = r["n"]
    algs = {}
    for stream in (True, False):
        alg = algs[stream] = build(kind, STREAM_INGEST=stream)
        set_logstd(alg)
        loss = feed(alg, kind, RAW)
        assert np.isfinite(loss)
    dev = algs[True].actor._ingest.last.dev
    torch.cuda.synchronize()
    cat = lambda k: np.concatenate([tr[k] for tr in r["trajs"]]).reshape(-1)
    assert np.array_equal(dev["adv"][:n].cpu().numpy(), cat("adv"))                  # oracle.returns.gae, float64
    assert np.array_equal(dev["target_v"][:n].cpu().numpy(), cat("target_value"))
    assert np.array_equal(dev["old_v"][:n].cpu().numpy(), cat("old_value"))
    assert np.array_equal(dev["action"][:n].cpu().numpy(), np.concatenate([tr["action"] for tr in r["trajs"]]))
    assert same(state_bits(algs[True]), state_bits(algs[False]))


# ---------------------------------------------------------------- 4: pinned sources, growth, [n, A] actions, padded width
def test_gauss_ingest_from_a_recycled_pinned_slot_grows_twice_and_pads_on_the_device():
    from xingtian_amd.ingest import PPO_FIELDS, RolloutIngest, ppo_fields
    assert ppo_fields("Categorical", 6) is PPO_FIELDS and ppo_fields("DiagGaussian", 6)[1:] == PPO_FIELDS[1:]
    assert ppo_fields("DiagGaussian", 6)[0] == ("action", torch.float32, 6)
    rng = np.random.default_rng(23)
    w, a = 11, 6
    ing = RolloutIngest("cuda:0", n_epochs=2, initial_capacity=16, obs_u8=False, fields=ppo_fields("DiagGaussian", a),
                        pad_channels=(12, 0))
    slot = torch.empty((64, w), dtype=torch.float32, pin_memory=True)
    parts = []
    for t in (10, 9, 30, 7):                   # 16 -> 32 -> 64 rows
        obs = rng.standard_normal((t, w)).astype(np.float32)
        m = (rng.standard_normal((t, a)).astype(np.float32), rng.standard_normal((t, 1)).astype(np.float32),
             rng.standard_normal((t, 1)), rng.standard_normal((t, 1)).astype(np.float32), rng.standard_normal((t, 1)))
        slot.numpy()[:t] = obs
        ing.put(slot.numpy()[:t], *m, pinned=True)
        slot.zero_()
        parts.append((obs, m))
    n, dev = ing.finish()
    torch.cuda.synchronize()
    assert n == 56 and ing.sets[0].cap == 64
    obs = dev["obs"][:n].cpu().numpy()
    assert obs.shape == (n, 12) and not obs[:, w:].any()
    assert np.array_equal(obs[:, :w], np.concatenate([p[0] for p in parts]))
    assert dev["action"].shape[1:] == (a,)
    assert np.array_equal(dev["action"][:n].cpu().numpy(), np.concatenate([p[1][0] for p in parts]))
    for j, k in enumerate(("old_logp", "adv", "old_v", "target_v"), start=1):
        assert np.array_equal(dev[k][:n].cpu().numpy(), np.concatenate([p[1][j] for p in parts]).reshape(-1)), k


# ---------------------------------------------------------------- 5: the fused head against the float64 oracle
def oracle_for(kind, w0, a_dim=None, hidden=None):
    s = SHAPES[kind]
    sd, ad = tuple(s["state_dim"]), a_dim or s["action_dim"]
    hid = tuple(hidden or s["hidden"])
    if s["model_name"] == "PpoMlp":
        ospec = nets.ppo_mlp_spec(sd, ad, hid, s["act"], s["share"], action_type="DiagGaussian")
    else:
        ospec = dict(nets.ppo_cnn_spec(sd, ad, hid, s["act"], s["share"]), action_type="DiagGaussian")
    shapes = nets.init_params(ospec)
    return nets.PpoLearnerOracle(ospec, {k: w0[k].reshape(shapes[k].shape) for k in shapes}, OCFG, np.float64)


def step_and_train_vs_oracle(alg, kind, orc, w0, a_dim=None):
    """one ppo_step(apply=False) and a three-epoch train() against the oracle -> the head path of the step"""
    r = rollout(kind)
    net = alg.actor.net
    cat = lambda k: np.concatenate([tr[k] for tr in r["trajs"]])
    obs = cat("cur_state")
    action = cat("action")
    if a_dim:
        action = np.random.default_rng(3).standard_normal((r["n"], a_dim)).astype(np.float32)
    lab = [action, cat("logp"), cat("adv"), cat("old_value"), cat("target_value")]
    d = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()
    c = net.make_ppo_cfg(OCFG)
    out = net.ppo_step(c, net.to_device_obs(obs), d(np.arange(BATCH), np.int32), d(action, np.float32),
                       d(lab[1].reshape(-1), np.float32), d(lab[2].reshape(-1), np.float64), d(lab[3].reshape(-1), np.float32),
                       d(lab[4].reshape(-1), np.float64), apply=False).cpu().numpy()
    path = net.last_head_path()
    ref = orc.step(obs[:BATCH], action[:BATCH], lab[1][:BATCH], lab[2][:BATCH].astype(np.float32), lab[3][:BATCH],
                   lab[4][:BATCH].astype(np.float32), apply=False)
    print("gauss_stream", kind, "step loss", out[0], "oracle", ref["loss"])
    assert abs(out[0] - ref["loss"]) < 1e-5 * max(1.0, abs(ref["loss"]))
    g = net.grads_dict()
    for k, rr in ref["grads"].items():
        e = rel_err(g[k].reshape(rr.shape), rr)
        print("gauss_stream", kind, "grad", k, "%.2e" % e)
        assert e < 1e-4, (k, e)
    lo = 0
    for tr in r["trajs"]:
        t = len(tr["cur_state"])
        alg.prepare_data(dict({k: tr[k] for k in WITH_ADV}, action=action[lo:lo + t]))
        lo += t
    loss = alg.train(perms=r["perms"])
    ref_loss = orc.train([obs], lab, r["perms"])
    print("gauss_stream", kind, "train loss", loss, "oracle", ref_loss)
    assert abs(loss - ref_loss) < 1e-4 * max(1.0, abs(ref_loss))
    w1 = alg.get_weights()
    for k, rr in orc.net.params.items():
        got, init = w1[k].reshape(rr.shape), w0[k].reshape(rr.shape)
        e = rel_err(got - init, rr - init)
        print("gauss_stream", kind, "delta", k, "%.2e" % e)
        assert e < 5e-3, (k, e)
    return path


@pytest.mark.parametrize("kind", sorted(SHAPES))
def test_gauss_fused_head_step_and_train_vs_oracle(kind):
    alg = build(kind, GAUSS_FUSED_HEAD=True)
    assert alg.actor.net.gauss_fused_on and alg.actor.stream_ingest
    w0 = set_logstd(alg)
    path = step_and_train_vs_oracle(alg, kind, oracle_for(kind, w0), w0)
    s = SHAPES[kind]
    family, nq, part, shared, am = decode_head_path(path)
    feat = s["hidden"][-1]
    assert (family, nq, shared, am) == (GAUSS_FUSED, 1 if feat <= 64 else 4, int(s["share"]), 0), hex(path)
    # mlp11: Dense 128 -> 64 at 40 rows is one tile over four K steps -> two slabs, finished by the head; cnn: Dense
    # 3136 -> 256 splits as in the categorical PpoCnn step.  The part bit is asserted so that the cases cannot drift.
    assert part == (1 if kind in ("mlp11", "cnn") else 0), (kind, hex(path))
    assert decode_head_path(alg.actor.net.last_head_path())[0] == GAUSS_FUSED       # (the train's steps too)


@pytest.mark.parametrize("kind,over,a_dim", [("mlp5", dict(), 9), ("mlp3", dict(hidden_sizes=[600]), None)],
                         ids=["a9", "hidden600"])
def test_gauss_fused_switch_outside_the_envelope_keeps_the_three_launches(kind, over, a_dim):
    from xingtian_amd.algorithm import alg_builder
    s = SHAPES[kind]
    cfg = dict(OCFG, VF_SHARE_LAYERS=s["share"], activation=s["act"], hidden_sizes=list(s["hidden"]),
               action_type="DiagGaussian", SEED=5, USE_HIP_GRAPH=False, GAUSS_FUSED_HEAD=True)
    cfg.update(over)
    actor = dict(model_name=s["model_name"], state_dim=list(s["state_dim"]), action_dim=a_dim or s["action_dim"],
                 input_dtype="float32", model_config=cfg)
    alg = alg_builder("PPO", {"actor": actor}, {"instance_num": len(s["lens"]), "agent_num": 1})
    assert alg.actor.net.gauss_fused_on
    w0 = set_logstd(alg)
    path = step_and_train_vs_oracle(alg, kind, oracle_for(kind, w0, a_dim, over.get("hidden_sizes")), w0, a_dim)
    assert path == TS_L().NET_HEAD_GAUSS and alg.actor.net.last_head_path() == TS_L().NET_HEAD_GAUSS


@pytest.mark.parametrize("kind", ["mlp11", "cnn"])
def test_gauss_fused_graph_replay_equals_eager(kind):
    runs = {}
    for graph in (True, False):
        alg = build(kind, GAUSS_FUSED_HEAD=True, USE_HIP_GRAPH=graph)
        set_logstd(alg)
        losses = [np.float32(feed(alg, kind)).tobytes() for _ in range(2)]
        runs[graph] = (losses, state_bits(alg))
        assert decode_head_path(alg.actor.net.last_head_path())[0] == GAUSS_FUSED
    assert runs[True][0] == runs[False][0] and same(runs[True][1], runs[False][1])


# ---------------------------------------------------------------- 6: switch hygiene
def test_gauss_fused_switch_set_and_cleared_leaves_no_trace_and_is_part_of_the_graph_key():
    lib = TS_L()
    # set and cleared again: the bits of a net that never had the switch (two updates each, captured graphs)
    never, cleared = build("mlp11", USE_HIP_GRAPH=True), build("mlp11", USE_HIP_GRAPH=True)
    set_logstd(never), set_logstd(cleared)
    cleared.actor.net.set_gauss_fused(True)
    cleared.actor.net.set_gauss_fused(False)
    la = [np.float32(feed(never, "mlp11")).tobytes() for _ in range(2)]
    lb = [np.float32(feed(cleared, "mlp11")).tobytes() for _ in range(2)]
    assert la == lb and same(state_bits(never), state_bits(cleared))
    assert cleared.actor.net.last_head_path() == lib.NET_HEAD_GAUSS
    # The third update streams into the buffer set of the first: every pointer of its graph key repeats, only the switch
    # differs.  It must be captured anew (the head path changes, and the bits are those of the eager run).
    eager = build("mlp11", USE_HIP_GRAPH=False)
    set_logstd(eager)
    for _ in range(2):
        feed(eager, "mlp11")
    assert same(state_bits(never), state_bits(eager))
    never.actor.net.set_gauss_fused(True)
    eager.actor.net.set_gauss_fused(True)
    l_graph, l_eager = feed(never, "mlp11"), feed(eager, "mlp11")
    assert decode_head_path(never.actor.net.last_head_path())[0] == GAUSS_FUSED, "the default graph was replayed"
    assert np.float32(l_graph).tobytes() == np.float32(l_eager).tobytes() and same(state_bits(never), state_bits(eager))


def test_gauss_fused_switch_is_refused_on_a_categorical_net_and_ignored_by_its_config():
    from xingtian_amd.algorithm import alg_builder
    lib = TS_L()
    actor = dict(model_name="PpoMlp", state_dim=[8], action_dim=4, input_dtype="float32",
                 model_config=dict(OCFG, action_type="Categorical", SEED=5, GAUSS_FUSED_HEAD=True))
    alg = alg_builder("PPO", {"actor": actor}, {"instance_num": 1, "agent_num": 1})       # (the key is ignored, with a log line)
    net = alg.actor.net
    assert not net.gauss_fused_on
    assert lib.load().xt_net_set_gauss_fused(net.handle, 1) != 0
    err = lib.load().xt_last_error().decode()
    assert "xt_net_set_gauss_fused" in err and "categorical" in err, err
    with pytest.raises(RuntimeError, match="xt_net_set_gauss_fused"):
        net.set_gauss_fused(True)


def test_train_stats_with_the_fused_gauss_head_against_float64():
    """net c of tests/test_gpu_train_stats.py (PpoMlp [3], DiagGaussian A = 3) with GAUSS_FUSED_HEAD: the sums after one
    gradient-only step on 40 and on 16 rows, with that file's reference and tolerances (REL 1e-4, FLOOR 1e-6; counts exact)"""
    S = TS_L().TRAIN_STATS_SLOTS
    r = TS.rollout("c")
    ref = r["ref"]
    model = TS.build("c", GAUSS_FUSED_HEAD=True).actor
    assert model.net.gauss_fused_on
    res = TS.upload(model, "c")
    for rows in (r["perms"][0, :40], r["perms"][0, 80:96]):
        model.net.clear_train_stats()
        TS.step(model, res, rows)
        assert decode_head_path(ctypes.c_int32(model.net.last_head_path()).value)[0] == GAUSS_FUSED
        acc = model.net._tstats["acc"].cpu().numpy()
        b = len(rows)
        assert acc[S["STEPS"]] == 1.0 and acc[S["ROWS"]] == float(b)
        assert acc[S["CLIPPED"]] == float(ref["clipped"][rows].sum())
        assert acc[S["VF_CLIPPED"]] == float(ref["vf_clipped"][rows].sum())
        want = {"SURR": ref["surr"][rows].mean(), "ENT": ref["ent"][rows].mean(), "VF": 0.5 * ref["vf"][rows].mean(),
                "KL": ref["kl"][rows].mean(), "TV": ref["tv"][rows].mean(), "TV_SQ": (ref["tv"][rows] ** 2).mean(),
                "ERR": ref["err"][rows].mean(), "ERR_SQ": (ref["err"][rows] ** 2).mean()}
        for k, w in want.items():
            got = acc[S[k]] / (1.0 if k in ("SURR", "ENT", "VF") else b)
            print("gauss_stream train_stats B %2d %-6s got %+.9e ref %+.9e" % (b, k, got, w))
            assert TS.near(got, w), (k, got, w)
    # ... and a whole update through the plugin path reports them
    alg = TS.build("c", GAUSS_FUSED_HEAD=True)
    TS.feed(alg, "c")
    d = alg.train_stats()
    assert d["steps"] == 6.0 and d["rows"] == 192.0 and d["clip_fraction"] > 0.0 and np.isfinite(list(d.values())).all()
