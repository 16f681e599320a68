"""GPU tests of the per-update PPO training diagnostics (``model_config.TRAIN_STATS``, C ABI ``xt_net_set_train_stats``).

Four nets, each with SEED fixed, reach every head / loss kernel that can write the diagnostic rows:
  a  PpoMlp [8], A = 4, hidden [64, 64], separate trunks   fused head, separate trunks, features final
  b  PpoMlp [8], A = 18, shared trunk                      plain path (A > 8): heads forward + ppo_loss_kernel
  c  PpoMlp [3], DiagGaussian A = 3                        padded input, ppo_loss_gauss_kernel
  d  PpoCnn [42, 42, 4] uint8, A = 6, hidden [256]         fused head, shared trunk, deferred split-K finish
(test_the_four_nets_reach_every_head_instance asserts that from ``xt_net_last_head_path``).

The rollout has n = 96 rows, BATCH_SIZE 40 (minibatches 40 / 40 / 16), NUM_SGD_ITER 2 and injected shuffles.  Its labels
are built from the net's OWN forward so that the clip counts are exact by construction: old_logp = logp - delta with delta
cycling through {+0.02, -0.02, +0.3, -0.3} (ratio e^delta: half the rows outside a clip of 0.2) and old_v = v - eps with eps
cycling through {0.5, 2} x VF_CLIP.  ``rollout`` asserts in float64 that no row lies within 1e-3 of a clip bound.

Bars.  Exact: step / row / flag counts.  Means of the per-row quantities against numpy float64 on the fp32 logits / mean /
value of ``forward``: 1e-4 relative (the project's bar for the loss scalar) with an absolute floor of 1e-6 (about 15 fp32
ulps of an O(1) log-probability) for means near zero.  Gradient norms against the float64 norm of a gradient-only replay:
1e-5 relative (the project's gradient bar).  Everything that compares two runs of this code is bitwise."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, BATCH, EPOCHS = 96, 40, 2
CLIP, VF_CLIP, ENT_COEF, CRITIC_COEF = 0.2, 0.25, 0.01, 0.5
DELTAS = np.array([0.02, -0.02, 0.3, -0.3])
EPS = np.array([0.5, 2.0]) * VF_CLIP
REL, FLOOR, GRAD_REL = 1e-4, 1e-6, 1e-5

NETS = {
    "a": dict(model_name="PpoMlp", state_dim=[8], action_dim=4, cfg=dict(hidden_sizes=[64, 64], VF_SHARE_LAYERS=False)),
    "b": dict(model_name="PpoMlp", state_dim=[8], action_dim=18, cfg=dict(VF_SHARE_LAYERS=True)),
    "c": dict(model_name="PpoMlp", state_dim=[3], action_dim=3, cfg=dict(action_type="DiagGaussian")),
    "d": dict(model_name="PpoCnn", state_dim=[42, 42, 4], action_dim=6, input_dtype="uint8", cfg=dict(hidden_sizes=[256])),
}


def build(kind, stats=True, **over):
    """alg_builder("PPO") on net `kind`; `over` overrides / extends model_config"""
    from xingtian_amd.algorithm import alg_builder
    spec = NETS[kind]
    cfg = dict(BATCH_SIZE=BATCH, NUM_SGD_ITER=EPOCHS, SEED=7, LR=1e-3, LOSS_CLIPPING=CLIP, VF_CLIP=VF_CLIP,
               ENTROPY_LOSS=ENT_COEF, CRITIC_LOSS_COEF=CRITIC_COEF, MAX_GRAD_NORM=5.0, USE_HIP_GRAPH=False)
    cfg.update(spec["cfg"])
    if stats:
        cfg["TRAIN_STATS"] = True
    cfg.update(over)
    actor = {k: v for k, v in spec.items() if k != "cfg"}
    actor["model_config"] = cfg
    return alg_builder("PPO", {"actor": actor}, {"instance_num": 1, "agent_num": 1})


def log_softmax64(logits):
    x = logits.astype(np.float64)
    x = x - x.max(-1, keepdims=True)
    return x - np.log(np.exp(x).sum(-1, keepdims=True))


_ROLLOUTS = {}


def rollout(kind):
    """The rollout of net `kind` (built once per module, never modified): observations, labels from the net's own forward,
    the injected shuffles and the float64 per-row reference quantities."""
    if kind in _ROLLOUTS:
        return _ROLLOUTS[kind]
    spec = NETS[kind]
    gauss = spec["cfg"].get("action_type") == "DiagGaussian"
    a_dim = spec["action_dim"]
    rng = np.random.default_rng(100 + ord(kind))
    model = build(kind, stats=False).actor
    if spec.get("input_dtype") == "uint8":
        obs = rng.integers(0, 256, (N,) + tuple(spec["state_dim"])).astype(np.uint8)
    else:
        obs = rng.uniform(-1, 1, (N,) + tuple(spec["state_dim"])).astype(np.float32)
    out, value = model.net.forward(obs)
    out, value = out.cpu().numpy(), value.cpu().numpy()          # fp32 logits (mean) [N, A], value [N]
    v = value.astype(np.float64)
    if gauss:
        log_std = model.get_weights()["pi_logstd"].reshape(-1).astype(np.float32)
        std = np.exp(log_std.astype(np.float64))
        action = (out + 0.5 * np.exp(log_std) * rng.standard_normal((N, a_dim))).astype(np.float32)
        z = (action.astype(np.float64) - out.astype(np.float64)) / std
        logp = -(0.5 * np.log(2.0 * np.pi) * a_dim + 0.5 * (z * z).sum(-1) + log_std.astype(np.float64).sum())
        ent = np.full(N, (log_std.astype(np.float64) + 0.5 * (np.log(2.0 * np.pi) + 1.0)).sum())
    else:
        action = rng.integers(0, a_dim, N).astype(np.int32)
        lsm = log_softmax64(out)
        logp = np.take_along_axis(lsm, action[:, None].astype(np.int64), 1)[:, 0]
        ent = -(np.exp(lsm) * lsm).sum(-1)
    i = np.arange(N)
    old_logp = (logp - DELTAS[i % 4]).astype(np.float32)
    old_v = (v - EPS[i % 2]).astype(np.float32)
    adv = rng.standard_normal(N)
    target_v = 3.0 * v - 0.2 + 0.1 * max(v.std(), 1e-3) * rng.standard_normal(N)
    perms = np.stack([rng.permutation(N) for _ in range(EPOCHS)]).astype(np.int32)
    # ---- float64 reference per row, on the fp32 values the kernels read
    ratio = np.exp(logp - old_logp.astype(np.float64))
    dv = np.abs(v - old_v.astype(np.float64))
    # a condition on the INPUTS (no row is excluded anywhere): nothing within 1e-3 of a clip bound
    assert np.abs(ratio - (1.0 - CLIP)).min() >= 1e-3 and np.abs(ratio - (1.0 + CLIP)).min() >= 1e-3, kind
    assert np.abs(dv - VF_CLIP).min() >= 1e-3 * VF_CLIP, kind
    advf = adv.astype(np.float32).astype(np.float64)
    tv = target_v.astype(np.float32).astype(np.float64)
    surr = np.minimum(ratio * advf, np.clip(ratio, 1.0 - CLIP, 1.0 + CLIP) * advf)
    vcl = old_v.astype(np.float64) + np.clip(v - old_v.astype(np.float64), -VF_CLIP, VF_CLIP)
    vf = np.maximum((v - tv) ** 2, (vcl - tv) ** 2)
    ref = dict(surr=surr, ent=ent, vf=vf, kl=old_logp.astype(np.float64) - logp,
               clipped=(ratio < 1.0 - CLIP) | (ratio > 1.0 + CLIP), vf_clipped=dv > VF_CLIP, tv=tv, err=tv - v)
    assert ref["clipped"].sum() == N // 2 and ref["vf_clipped"].sum() == N // 2
    data = dict(cur_state=obs, action=action, logp=old_logp.reshape(-1, 1), adv=adv.reshape(-1, 1),
                old_value=old_v.reshape(-1, 1), target_value=target_v.reshape(-1, 1))
    _ROLLOUTS[kind] = dict(data=data, perms=perms, ref=ref)
    return _ROLLOUTS[kind]


def slices(perms):
    """the six minibatches of one update, in execution order"""
    return [perms[ep, s:s + BATCH] for ep in range(EPOCHS) for s in range(0, N, BATCH)]


def feed(alg, kind):
    r = rollout(kind)
    alg.prepare_data(dict(r["data"]))
    return alg.train(perms=r["perms"])


def upload(model, kind):
    d = rollout(kind)["data"]
    return model._upload([d["cur_state"]], [d["action"], d["logp"], d["adv"], d["old_value"], d["target_value"]])


def step(model, res, rows, apply=False):
    idx = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32)).to(model.net.device)
    model.net.ppo_step(model._cfg, res["obs"], idx, res["action"], res["old_logp"], res["adv"], res["old_v"],
                       res["target_v"], apply=apply)
    torch.cuda.synchronize()


def near(got, ref, rel=REL, floor=FLOOR):
    return abs(got - ref) <= max(rel * abs(ref), floor)


def one_step_errors(kind):
    """Case 1 on net `kind`: the sums after ONE gradient-only step on 40 and on 16 rows against float64.
    -> (head path, {quantity: (largest error, its bar)}); asserts the exact slots."""
    from xingtian_amd import lib as L
    S = L.TRAIN_STATS_SLOTS
    r = rollout(kind)
    ref = r["ref"]
    model = build(kind).actor
    res = upload(model, kind)
    worst = {}
    for rows in (r["perms"][0, :40], r["perms"][0, 80:96]):
        model.net.clear_train_stats()
        step(model, res, rows)
        acc = model.net._tstats["acc"].cpu().numpy()
        b = len(rows)
        assert acc[S["STEPS"]] == 1.0 and acc[S["ROWS"]] == float(b)
        assert acc[S["CLIPPED"]] == float(ref["clipped"][rows].sum()), kind
        assert acc[S["VF_CLIPPED"]] == float(ref["vf_clipped"][rows].sum()), kind
        assert acc[S["GNORM_SUM"]] == 0.0 and acc[S["GNORM_MAX"]] == 0.0 and acc[S["RESERVED"]] == 0.0   # (no norm is formed)
        want = {"SURR": ref["surr"][rows].mean(), "ENT": ref["ent"][rows].mean(), "VF": 0.5 * ref["vf"][rows].mean(),
                "KL": ref["kl"][rows].mean(), "TV": ref["tv"][rows].mean(), "TV_SQ": (ref["tv"][rows] ** 2).mean(),
                "ERR": ref["err"][rows].mean(), "ERR_SQ": (ref["err"][rows] ** 2).mean()}
        for k, w in want.items():
            got = acc[S[k]] / (1.0 if k in ("SURR", "ENT", "VF") else b)
            e, bar = abs(got - w), max(REL * abs(w), FLOOR)
            print("train_stats one step: net %s B %2d %-6s got %+.9e ref %+.9e err %.2e bar %.2e" % (kind, b, k, got, w, e, bar))
            if k not in worst or e / bar > worst[k][0] / worst[k][1]:
                worst[k] = (e, bar)
    return model.net.last_head_path(), worst


_PATHS = {}


@pytest.mark.parametrize("kind", sorted(NETS))
def test_one_step_against_float64(kind):
    path, worst = one_step_errors(kind)
    _PATHS[kind] = path
    for k, (e, bar) in worst.items():
        assert e <= bar, (kind, k, e, bar)


def test_the_four_nets_reach_every_head_instance():
    from xingtian_amd import lib as L
    for kind in sorted(NETS):
        if kind not in _PATHS:
            _PATHS[kind] = one_step_errors(kind)[0]
    assert _PATHS["b"] == L.NET_HEAD_PLAIN and _PATHS["c"] == L.NET_HEAD_GAUSS
    fused = [p for p in _PATHS.values() if (p & 0xf) == 1]          # XT_HEAD_PATH_PPO_FUSED
    part = {(p >> 8) & 1 for p in fused}                            # XT_HEAD_PART_SHIFT
    shared = {(p >> 9) & 1 for p in fused}                          # XT_HEAD_SHARED_SHIFT
    assert part == {0, 1} and shared == {0, 1}, [hex(p) for p in fused]


_NORMS = {}


def grad_norms(kind):
    """the float64 norm of the gradient of each of the six minibatches, by gradient-only replay on an untrained net"""
    if kind in _NORMS:
        return _NORMS[kind]
    r = rollout(kind)
    model = build(kind, stats=False).actor
    res = upload(model, kind)
    norms = []
    for rows in slices(r["perms"]):
        step(model, res, rows)
        g = model.net.grads_dict()
        norms.append(float(np.sqrt(sum((v.astype(np.float64) ** 2).sum() for v in g.values()))))
    _NORMS[kind] = np.array(norms)
    return _NORMS[kind]


def clip_between(norms):
    """MAX_GRAD_NORM inside the widest gap of the six norms: some steps clipped, some not, none near the bound"""
    s = np.sort(norms)
    j = int(np.argmax(s[1:] / s[:-1]))
    clip = float(np.sqrt(s[j] * s[j + 1]))
    assert s[0] < clip < s[-1] and (np.abs(norms - clip) >= 0.01 * norms).all(), (norms, clip)
    return clip


@pytest.mark.parametrize("kind", sorted(NETS))
def test_whole_update_with_zero_step_size(kind):
    r = rollout(kind)
    ref = r["ref"]
    norms = grad_norms(kind)
    clip = clip_between(norms)
    alg = build(kind, LR=0.0, MAX_GRAD_NORM=clip)
    w0 = alg.actor.net.params.cpu().numpy().copy()
    assert alg.train_stats() is None
    loss = feed(alg, kind)
    d = alg.train_stats()
    assert np.array_equal(alg.actor.net.params.cpu().numpy(), w0)          # (step size 0: every step saw the same net)
    assert d["steps"] == 6.0 and d["rows"] == 192.0
    assert d["clip_fraction"] == 0.5 and d["vf_clip_fraction"] == 0.5
    sl = slices(r["perms"])
    want = dict(approx_kl=ref["kl"].mean(), entropy=np.mean([ref["ent"][q].mean() for q in sl]),
                explained_variance=1.0 - ref["err"].var() / ref["tv"].var(),
                policy_loss=-np.mean([ref["surr"][q].mean() for q in sl]),
                value_loss=np.mean([0.5 * ref["vf"][q].mean() for q in sl]))
    for k, w in want.items():
        print("train_stats update: net %s %-18s got %+.9e ref %+.9e err %.2e" % (kind, k, d[k], w, abs(d[k] - w)))
        assert near(d[k], w), (kind, k, d[k], w)
    assert type(d["loss"]) is float and np.float32(d["loss"]) == loss and d["loss"] == float(loss)
    recombined = d["policy_loss"] - ENT_COEF * d["entropy"] + CRITIC_COEF * d["value_loss"]
    print("train_stats update: net %s loss %.9e recombined %.9e" % (kind, d["loss"], recombined))
    assert abs(d["loss"] - recombined) <= 1e-6
    print("train_stats update: net %s norms %s clip %.6e got mean %.9e max %.9e" % (kind, norms, clip, d["grad_norm"],
                                                                                  d["grad_norm_max"]))
    assert near(d["grad_norm"], norms.mean(), GRAD_REL, 0.0) and near(d["grad_norm_max"], norms.max(), GRAD_REL, 0.0)
    assert d["grad_clip_fraction"] == (norms > clip).sum() / 6.0 and 0.0 < d["grad_clip_fraction"] < 1.0


@pytest.mark.parametrize("knobs", [dict(finalize_ticket=1), dict(tail_fused=1), dict(tail_overlap=3)],
                         ids=["ticket", "fused", "overlap"])
def test_every_tail_form_keeps_the_sums(knobs):
    """The other places a single-GPU step can write the gradient norm from (the last-block finalize, the fused tail, the
    split optimiser launch of the overlapped tail) and reduce the rows in: with step size 0 the row statistics are those
    of the default form bit for bit, the gradient norms agree to the gradient bar (the forms sum the squared-norm partials
    in different groupings)."""
    from xingtian_amd import lib as L
    kind = "d"
    clip = clip_between(grad_norms(kind))
    alg = build(kind, LR=0.0, MAX_GRAD_NORM=clip)
    feed(alg, kind)
    base = alg.train_stats()
    old = L.set_tuning(**knobs)          # (read when a net is created and at every launch: set before, restored after)
    try:
        alg = build(kind, LR=0.0, MAX_GRAD_NORM=clip)
        feed(alg, kind)
        d = alg.train_stats()
        alg.actor.net.check_device_errors()
    finally:
        L.set_tuning(**old)
    for k in base:
        if k in ("grad_norm", "grad_norm_max"):
            assert near(d[k], base[k], GRAD_REL, 0.0), (k, d[k], base[k])
        elif k != "loss":
            assert d[k] == base[k], (k, d[k], base[k])
    assert near(d["loss"], base["loss"], REL, FLOOR) and 0.0 < d["grad_clip_fraction"] < 1.0


def state_of(alg):
    net = alg.actor.net
    return [net.params.cpu().numpy().copy(), net.adam_m.cpu().numpy().copy(), net.adam_v.cpu().numpy().copy(),
            net.adam_state.cpu().numpy().copy()]


def same_bits(x, y):
    return all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(x, y))


def stats_bits(d):
    return np.array([d[k] for k in sorted(d)], np.float64).tobytes()


@pytest.mark.parametrize("kind", ["a", "c", "d"])
def test_on_equals_off(kind):
    runs = {}
    for on in (True, False):
        alg = build(kind, stats=on, USE_HIP_GRAPH=True)
        losses = [feed(alg, kind) for _ in range(2)]
        assert (alg.train_stats() is not None) == on
        runs[on] = (np.array(losses, np.float32), state_of(alg))
    assert np.array_equal(runs[True][0].view(np.uint32), runs[False][0].view(np.uint32))
    assert same_bits(runs[True][1], runs[False][1])
    assert not np.array_equal(runs[True][1][0], build(kind, stats=False).actor.net.params.cpu().numpy())   # (it did train)


@pytest.mark.parametrize("kind", ["a", "d"])
def test_graph_replay_equals_eager_and_runs_repeat(kind):
    runs = []
    for graph in (True, False, True):
        alg = build(kind, USE_HIP_GRAPH=graph)
        seen = []
        for _ in range(3):                     # (update 3 replays the graph a second time)
            feed(alg, kind)
            d = alg.train_stats()
            assert d["rows"] == 192.0 and d["steps"] == 6.0          # nothing leaks from one update into the next
            assert np.isfinite(list(d.values())).all() and d["grad_norm_max"] >= d["grad_norm"] > 0.0
            seen.append(stats_bits(d))
        assert len(set(seen)) == 3             # (LR > 0: the updates differ)
        runs.append(seen)
    assert runs[0] == runs[1], "graph replay and eager differ"
    assert runs[0] == runs[2], "two identical runs differ"


def test_streaming_path_gives_the_same_stats():
    got = {}
    for stream in (False, True):
        alg = build("d", STREAM_INGEST=stream)
        assert bool(alg.actor.stream_ingest) == stream
        loss = feed(alg, "d")
        got[stream] = (np.float32(loss).tobytes(), stats_bits(alg.train_stats()))
    assert got[False] == got[True]


def test_switching_off_and_refusals():
    from xingtian_amd.model import model_builder
    on, never = build("a", USE_HIP_GRAPH=True), build("a", stats=False, USE_HIP_GRAPH=True)
    for _ in range(2):
        feed(on, "a"), feed(never, "a")
    assert on.train_stats() is not None
    on.actor.net.set_train_stats(False)        # xt_net_set_train_stats(NULL, NULL): the captured graph is not replayed
    l_on, l_never = feed(on, "a"), feed(never, "a")
    assert on.train_stats() is None
    assert np.float32(l_on).tobytes() == np.float32(l_never).tobytes() and same_bits(state_of(on), state_of(never))
    # back on: the sums are those of one update again
    on.actor.net.set_train_stats(True)
    feed(on, "a")
    assert on.train_stats()["rows"] == 192.0
    # a data-parallel tail first: refused, with a message; and DP in the configuration raises
    net = never.actor.net
    net.set_dp(0, 1)
    with pytest.raises(RuntimeError, match="data-parallel"):
        net.set_train_stats(True)
    net.set_dp(0, 0)
    assert not net.train_stats_on
    spec = NETS["a"]
    with pytest.raises(ValueError, match="TRAIN_STATS"):
        model_builder(dict(model_name=spec["model_name"], state_dim=spec["state_dim"], action_dim=spec["action_dim"],
                           model_config=dict(spec["cfg"], TRAIN_STATS=True, DP="strict", DEVICE="gpu")))
    # and the other way round: the tail is refused while the statistics are on
    with pytest.raises(RuntimeError, match="training statistics"):
        on.actor.net.set_dp(0, 1)
    assert ctypes.c_int32(on.actor.net.last_head_path()).value & 0xf == 1
