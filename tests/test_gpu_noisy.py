"""GPU tests of the noisy layers (NoisyNet): ``xt_noisy_compose`` and ``xt_noisy_grads`` alone through the C ABI on
synthetic layer tables (guard words on both sides of every buffer, plain ranges between the blocks), the determinism of
the draw, one ``dqn_step`` with every sigma 0 against a plain net, the whole noisy step against the float64 checker at the
project's standing bars (loss 1e-4, every gradient tensor 1e-5 by ``rel_max``, mu and sigma alike), and
``alg_builder("DQN")`` with ``model_config.noisy``."""
import numpy as np
import pytest
import torch

import dqn_helpers as H
import noisy_helpers as NH
import nstep_helpers as N
import per_helpers as P
from xingtian_amd.model.dqn import dqn_cnn as D

pytestmark = pytest.mark.gpu

GAMMA, CAP = NH.GAMMA, NH.CAP


@pytest.fixture(scope="module")
def L():
    from xingtian_amd import lib
    lib.require_gpu()
    lib.load()
    return lib


@pytest.fixture(autouse=True)
def _module_constants_restored():
    """import_config overrides the modules' constants for the rest of the process: put them back"""
    from xingtian_amd.algorithm.dqn import dqn
    from xingtian_amd.model.dqn import dqn_cnn, dqn_mlp
    saved = [(m, {k: v for k, v in vars(m).items() if k.isupper()}) for m in (dqn, dqn_cnn, dqn_mlp)]
    yield
    torch.cuda.synchronize()
    for m, consts in saved:
        vars(m).update(consts)


# ------------------------------------------------------------------------------------------------ xt_noisy_compose alone
@pytest.mark.parametrize("name", list(NH.TABLES))
def test_compose_against_the_host_twins(L, name):
    t = NH.table(*NH.TABLES[name])
    assert t.n_net % 1024 != 0                                # (no multiple of the pass's tile, the grid's stride)
    store = NH.store_of(t, 1)
    rc, eff, noise, after = NH.gpu_compose(t, store)
    assert rc == 0, NH.last_error()
    assert np.array_equal(NH.bits(after), NH.bits(store))     # the source store is untouched
    # the stored vectors, as f |f|, against the float64 twin on the same float32 uniforms: every element
    measured, bar = NH.vector_bar()
    x64 = NH.twin64(t, NH.SEED, NH.CALL, 0)
    used = np.zeros(t.noise_floats, bool)
    worst = 0.0
    for sl in NH.vector_slices(t):
        used[sl] = True
        worst = max(worst, float(np.abs(NH.squared(noise[sl]) - x64[sl]).max()))
    print("noisy vectors", name, "kernel max |f|f| - twin| =", worst, "| float32 NumPy restatement", measured, "| bar", bar)
    assert worst <= bar, (worst, bar)
    assert (noise[~used] == NH.SENTINEL).all()                # nothing outside the layers' vectors
    # W_eff, b_eff and every plain float: the host formula on the stored vectors, bit for bit
    assert np.array_equal(NH.bits(eff), NH.bits(D.noisy_effective(t, store, noise)))
    # given vectors instead of drawn ones: the host twin end to end, bit for bit
    given = D.noisy_vectors(t, NH.SEED, NH.CALL, 0)
    rc, eff_in, noise_out, _ = NH.gpu_compose(t, store, noise_in=given)
    assert rc == 0, NH.last_error()
    assert np.array_equal(NH.bits(eff_in), NH.bits(D.noisy_effective(t, store, given)))
    assert np.array_equal(NH.bits(noise_out[used]), NH.bits(given[used])) and (noise_out[~used] == NH.SENTINEL).all()
    # mean_only: a copy, and nothing is drawn
    rc, eff_mean, noise_mean, _ = NH.gpu_compose(t, store, mean_only=True)
    assert rc == 0, NH.last_error()
    assert np.array_equal(NH.bits(eff_mean), NH.bits(store[:t.n_net])) and (noise_mean == NH.SENTINEL).all()


def test_compose_refusals_leave_every_buffer_untouched(L):
    t = NH.table(*NH.THREE)
    store = NH.store_of(t, 2)
    far = NH.table([(12, 8), (8, 1), (8, 516)], [8, 12, 464])
    far.noisy_layers[1].w_off = far.noisy_layers[0].w_off + 8            # overlapping mean blocks
    for kw, word in ((dict(null=("store",)), "null"), (dict(null=("eff",)), "null"), (dict(null=("noise",)), "null"),
                     (dict(null=("layers",)), "null"), (dict(n_layers=0), "n_layers = 0"), (dict(n_layers=9), "n_layers = 9"),
                     (dict(n_net=t.noisy_layers[2].w_off), "leaves [0, %d)" % t.noisy_layers[2].w_off),
                     (dict(layers=far.noisy_layers), "overlap")):
        rc, eff, noise, after = NH.gpu_compose(t, store, **kw)
        assert rc != 0 and word in NH.last_error(), (kw, NH.last_error())
        assert (eff == NH.SENTINEL).all() and (noise == NH.SENTINEL).all() and np.array_equal(NH.bits(after), NH.bits(store))


# ------------------------------------------------------------------------------------------------ determinism
def test_the_draw_is_a_function_of_seed_call_stream_and_layer_alone(L):
    t = NH.table(*NH.THREE)
    store = NH.store_of(t, 3)
    _, eff, noise, _ = NH.gpu_compose(t, store)
    _, eff2, noise2, _ = NH.gpu_compose(t, store)
    assert np.array_equal(NH.bits(eff), NH.bits(eff2)) and np.array_equal(NH.bits(noise), NH.bits(noise2))
    # one layer at a time: the same vectors and the same effective block
    for nl in t.noisy_layers:
        rc, eff1, noise1, _ = NH.gpu_compose(t, store, layers=[nl])
        assert rc == 0, NH.last_error()
        for sl in (nl.f_in, nl.f_out):
            assert np.array_equal(NH.bits(noise1[sl]), NH.bits(noise[sl]))
        blk = slice(nl.w_off, nl.w_off + (nl.K + 1) * nl.N)
        assert np.array_equal(NH.bits(eff1[blk]), NH.bits(eff[blk]))
        rest = np.ones(t.n_net, bool)
        rest[blk] = False
        assert np.array_equal(NH.bits(eff1[rest]), NH.bits(store[:t.n_net][rest]))
    # another call, another stream, another seed: every vector changes
    for kw in (dict(call=NH.CALL + 1), dict(stream=1), dict(stream=2), dict(seed=NH.SEED + 1), dict(call=NH.CALL + 2 ** 32)):
        _, _, other, _ = NH.gpu_compose(t, store, **kw)
        same = [np.array_equal(other[sl], noise[sl]) for sl in NH.vector_slices(t)]
        assert all(same) if kw.get("call") == NH.CALL + 2 ** 32 else not any(same), kw      # (call: its low word)


# ------------------------------------------------------------------------------------------------ xt_noisy_grads alone
@pytest.mark.parametrize("name", list(NH.TABLES))
def test_sigma_gradients_against_the_host_twin(L, name):
    t = NH.table(*NH.TABLES[name])
    grads = NH.store_of(t, 4)
    grads[t.n_net:] = NH.SENTINEL
    noise = D.noisy_vectors(t, NH.SEED, NH.CALL, 0)
    rc, got = NH.gpu_grads(t, grads, noise)
    assert rc == 0, NH.last_error()
    want = D.noisy_sigma_grads(t, grads, noise)               # (the sentinels between the sigma blocks stay)
    assert np.array_equal(NH.bits(got), NH.bits(want))
    assert np.array_equal(NH.bits(got[:t.n_net]), NH.bits(grads[:t.n_net]))
    written = np.zeros(t.n_flat, bool)
    for nl in t.noisy_layers:
        written[nl.sigma_off:nl.sigma_off + (nl.K + 1) * nl.N] = True
    assert (got[t.n_net:][~written[t.n_net:]] == NH.SENTINEL).all() and not (got[written] == NH.SENTINEL).any()


def test_sigma_gradient_refusals_leave_the_gradient_untouched(L):
    t = NH.table(*NH.THREE)
    grads, noise = NH.store_of(t, 5), D.noisy_vectors(t, 1, 2, 0)
    bad = NH.table(*NH.THREE)
    bad.noisy_layers[2].sigma_off = 8                         # a sigma block inside the mean blocks
    for kw in (dict(null=("noise",)), dict(null=("grads",)), dict(null=("layers",)), dict(n_layers=0), dict(n_layers=9),
               dict(layers=bad.noisy_layers)):
        rc, got = NH.gpu_grads(t, grads, noise, **kw)
        assert rc != 0 and "xt_noisy_grads" in NH.last_error(), kw
        assert np.array_equal(NH.bits(got), NH.bits(grads))


# ------------------------------------------------------------------------------------------------ nets and the replay
def _nets(kind, dueling, variant, max_batch=8):
    from xingtian_amd.model.hip_net import HipActorCritic
    spec, ospec = NH.step_specs(kind, dueling, variant)
    net, target = HipActorCritic(spec, max_batch=max_batch, seed=0), HipActorCritic(spec, max_batch=max_batch, seed=0)
    net.set_weights(NH.step_weights(spec, ospec, 1, dueling))
    target.set_weights(NH.step_weights(spec, ospec, 2, dueling))
    for n in (net, target):
        n.set_noisy(NH.STEP_SEED, 0.5)
        if variant == "atoms":
            n.set_dist(NH.HEAD["atoms"][0], NH.V_MIN, NH.V_MAX)
        if variant == "quantiles":
            n.set_quant(NH.HEAD["quantiles"][1], NH.KAPPA)
    return spec, ospec, net, target


def _filled_replay(kind, net, n_step):
    from xingtian_amd.algorithm.dqn.dqn import DeviceReplay
    ring = DeviceReplay(CAP, net.device, net.to_device_obs, n_step=n_step)
    N.fill(ring, CAP, NH.RING_SEED, a_dim=NH.SHAPE[kind][1], states=NH.state_fn(kind))
    return ring


def _host(x):
    return x.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------------ sigma = 0
def test_a_step_with_every_sigma_zero_is_the_plain_nets_step(L):
    from xingtian_amd.model import netspec
    from xingtian_amd.model.hip_net import HipActorCritic
    spec, ospec, net, target = _nets("mlp3", True, "plain")
    plain_spec = netspec.dqn_mlp((3,), 2, 8, 1, True)
    pnet, ptarget = HipActorCritic(plain_spec, max_batch=8, seed=0), HipActorCritic(plain_spec, max_batch=8, seed=0)
    for noisy, plain, seed in ((net, pnet, 1), (target, ptarget, 2)):
        w = NH.step_weights(spec, ospec, seed, True)
        noisy.set_weights({k: (np.zeros_like(v) if "/sigma_" in k else v) for k, v in w.items()})
        plain.set_weights({k: v for k, v in w.items() if "/sigma_" not in k})
    ring = _filled_replay("mlp3", net, 1)
    slots = torch.tensor([3, 17, 8, 41, 29], dtype=torch.int32, device="cuda")
    args = (ring.cur_state, ring.next_state, slots, ring.action, ring.reward, ring.done, GAMMA, True, True)
    net.compose(NH.STEP_CALL, 0)
    target.compose(NH.STEP_CALL, 1)
    loss = _host(net.dqn_step(target, *args)).copy()
    net.noisy_grads()
    ploss = _host(pnet.dqn_step(ptarget, *args)).copy()
    torch.cuda.synchronize()
    assert np.array_equal(_host(net.params_eff), _host(pnet.params))         # (as values: mu + 0 * e)
    assert np.array_equal(loss[:3], ploss[:3])
    g, pg = net.grads_dict(), pnet.grads_dict()
    for k, v in pg.items():
        assert np.array_equal(g[k], v) and v.any(), k
    flat, noise = _host(net.grads), _host(net.noise)
    assert np.array_equal(NH.bits(flat), NH.bits(D.noisy_sigma_grads(spec, flat, noise)))
    assert all(g[k].any() for k in g if "/sigma_" in k)
    assert not flat[spec.noisy_layers[0].sigma_off + 3 * 8:spec.noisy_layers[0].sigma_off + 4 * 8].any()      # the padded row


# ------------------------------------------------------------------------------------------------ the whole step
@pytest.mark.parametrize("case", NH.STEP_CASES, ids=["%s_%s_%s_%s" % (k, "dueling" if du else "single", "double" if do else
                                                                      "vanilla", v) for k, du, do, v in NH.STEP_CASES])
def test_noisy_dqn_step_against_float64(L, case):
    kind, dueling, double, variant = case
    _, a_dim, b = NH.SHAPE[kind]
    n_step = 3 if variant == "nstep" else 1
    spec, ospec, net, target = _nets(kind, dueling, variant)
    ring = _filled_replay(kind, net, n_step)
    _, _, cur, nxt = NH.ring_rows(kind)
    labels = NH.host_labels(kind, n_step)
    # the effective parameters of this train, then a minibatch of rows that are well conditioned under them
    net.compose(NH.STEP_CALL, 0)
    target.compose(NH.STEP_CALL, 1)
    torch.cuda.synchronize()
    noise, t_noise = _host(net.noise).copy(), _host(target.noise).copy()
    assert not any(np.array_equal(noise[sl], t_noise[sl]) for sl in NH.vector_slices(spec))       # streams 0 and 1
    p_on = NH.oracle_params(spec, ospec, NH.effective64(spec, _host(net.params), noise))
    p_tg = NH.oracle_params(spec, ospec, NH.effective64(spec, _host(target.params), t_noise))
    ok = NH.eligible(kind, dueling, double, variant, ospec, p_on, p_tg)
    assert len(ok) >= 4 * b, len(ok)
    rng = np.random.default_rng(len(variant) + 2 * dueling + double)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    kw = dict(dist=variant == "atoms", quant=variant == "quantiles")
    if n_step > 1:
        kw.update(follow=ring.follow, n=n_step)
    args = (ring.action, ring.reward, ring.done, GAMMA, dueling, double)
    store_before, target_before = net.params.clone(), target.params.clone()
    if variant == "per":
        alpha, beta, eps = 0.6, 0.4, 1e-6
        trees = P.GpuTrees(CAP, alpha)
        assert trees.add(0, CAP) == 0
        delta = np.zeros(CAP, np.float32)
        delta[ok] = rng.uniform(0.01, 3.0, len(ok))
        assert trees.update(list(range(CAP)), delta, eps) == 0
        s0, m0, _ = trees.read()
        for _ in range(100):
            u = rng.random(b)
            if set(P.sample(s0, m0, CAP, u.tolist(), beta)[1]) <= set(ok.tolist()):
                break
        else:
            raise AssertionError("no well-conditioned prioritised draw")
        per = dict(size=CAP, u=up(u), sum_tree=trees.sum, min_tree=trees.min, max_prio=trees.max_prio, alpha=alpha, beta=beta,
                   eps=eps)
        out = net.dqn_step(target, ring.cur_state, ring.next_state, None, *args, per=per, **kw)
        net.noisy_grads()
        torch.cuda.synchronize()
        _, ref_slots, ref_w = P.sample(s0, m0, CAP, u.tolist(), beta)
        slots, w = _host(net.per_slots[:b]), _host(net.per_weights[:b])
        assert slots.tolist() == ref_slots and P.rel_err(w, ref_w) <= 1e-12
    else:
        slots, w = rng.permutation(ok)[:b], None
        out = net.dqn_step(target, ring.cur_state, ring.next_state, up(slots), *args, **kw)
        net.noisy_grads()
        torch.cuda.synchronize()
    boot, act, rew, disc, done = labels(slots)
    if n_step > 1:
        assert (boot != slots).any()
    ref = NH.step_ref(kind, dueling, double, variant, ospec, p_on, p_tg, cur[slots], nxt[boot], act, rew, disc, done, w)
    NH.assert_step(float(_host(out)[0]), net.grads_dict(), ref, spec, ospec, noise, "%s %s" % (kind, variant))
    # the step read the composed parameters: the store, the vectors and the target pair are what they were
    assert torch.equal(net.params, store_before) and torch.equal(target.params, target_before)
    assert np.array_equal(NH.bits(_host(net.noise)), NH.bits(noise)) and not bool(target.grads.any())


# ------------------------------------------------------------------------------------------------ through the plugin pair
def _build(mean=False, seed=3):
    from xingtian_amd.algorithm import alg_builder
    mc = {"noisy": True, "noisy_sigma0": 0.5, "dueling": True, "SEED": seed, "LR": 1e-2, "HIDDEN_SIZE": 8, "NUM_LAYERS": 1,
          "NOISY_PREDICT_MEAN": mean}
    info = {"actor": {"model_name": "DqnMlp", "type": "learner", "state_dim": [3], "action_dim": 2, "model_config": mc}}
    cfg = {"instance_num": 1, "agent_num": 1, "prepare_times_per_train": 1, "BUFFER_SIZE": CAP, "BATCH_SIZE": 8,
           "TARGET_UPDATE_FREQ": 3, "GAMMA": GAMMA, "double_dqn": True}
    return alg_builder("DQN", info, cfg), info


def test_dqn_algorithm_with_noisy_layers_trains_syncs_restores_and_publishes(L, tmp_path):
    from xingtian_amd.model import model_builder
    alg, info = _build()
    net = alg.actor.net
    spec = net.spec
    assert alg.device_step and alg.actor.noisy and [nl.name for nl in spec.noisy_layers] == ["dense", "dense_1", "dense_2"]
    assert net.noisy == (3, 0.5) and alg.target_actor.net.noisy == (3, 0.5) and net.params.numel() == spec.n_flat
    from xingtian_amd.model.cpu_net import CpuActorCritic
    assert np.array_equal(_host(net.params), CpuActorCritic(spec, seed=3).params)        # one seed: the replica starts equal
    msgs, _, cur, _ = NH.ring_rows("mlp3")
    for m in msgs:
        alg.prepare_data(m)
    net.lib = N.CountingLib(net.lib)
    w0 = alg.get_weights()
    sig = [k for k in w0 if "/sigma_" in k]
    assert len(sig) == 6 and sorted(w0) == sorted(spec.names)
    samples = [np.random.default_rng(s).permutation(CAP)[:8].tolist() for s in range(4)]
    target_init = alg.target_actor.net.params.clone()
    for t in range(1, 4):
        loss = alg.train_on_slots(samples[t - 1])
        assert np.isfinite(loss)
        tp = alg.target_actor.net.params
        assert torch.equal(tp, target_init) if t < 3 else torch.equal(tp, net.params)       # the sync copies the whole store
    assert alg.actor.iterations == 3 and net.lib.calls["xt_noisy_compose"] == 3 and net.lib.calls["xt_noisy_grads"] == 3
    w3 = alg.get_weights()
    for k in w0:                                              # every variable moved, the sigmas among them
        assert not np.array_equal(w3[k], w0[k]), k
    pad = spec.noisy_layers[0]
    flat = _host(net.params)
    for off in (pad.w_off, pad.sigma_off):                    # the padded input row of both blocks stays 0
        assert not flat[off + 3 * pad.N:off + 4 * pad.N].any()
    # predict on the learner: new noise per call, from a counter of its own
    x = cur[:6]
    q1, q2 = alg.actor.predict(x), alg.actor.predict(x)
    assert q1.shape == (6, 2) and not np.array_equal(q1, q2) and alg.actor.noisy_predict_calls == 2
    saved = alg.save(str(tmp_path), 1)[0]
    assert set(np.load(saved).files) >= set(spec.names) | {"keras_adam_iterations", "noisy_predict_calls"}
    loss4 = alg.train_on_slots(samples[3])
    q3 = alg.actor.predict(x)
    # a fresh pair restored from the file continues bit for bit: both call counters came back
    alg2, _ = _build()
    alg2.restore(model_name=saved)
    assert alg2.actor.iterations == 3 and alg2.actor.noisy_predict_calls == 2
    for m in msgs:
        alg2.prepare_data(m)
    assert alg2.train_on_slots(samples[3]) == loss4 and torch.equal(alg2.actor.net.params, net.params)
    assert np.array_equal(alg2.actor.predict(x), q3)
    # NOISY_PREDICT_MEAN: mu alone, call after call, and what a CPU replica of the published weights predicts
    alg3, info3 = _build(mean=True)
    alg3.actor.set_weights(alg.get_weights())
    qm = alg3.actor.predict(x)
    assert np.array_equal(alg3.actor.predict(x), qm) and not np.array_equal(qm, q3)
    published = alg.get_weights()
    assert set(sig) <= set(published)
    rep_info = dict(info3["actor"], type="explorer", model_config=dict(info3["actor"]["model_config"], DEVICE="cpu"))
    replica = model_builder(rep_info)
    replica.set_weights(published)
    got = replica.get_weights()
    assert all(np.array_equal(got[k], published[k]) for k in published)
    q_cpu = replica.predict(x)
    assert q_cpu.dtype == np.float32 and np.abs(qm - q_cpu).max() <= 1e-5 * max(1.0, np.abs(qm).max())
    # a noisy replica draws (stream 2, its own counter): differs from the mean, call from call
    noisy_rep = model_builder(dict(rep_info, model_config=dict(rep_info["model_config"], NOISY_PREDICT_MEAN=False)))
    noisy_rep.set_weights(published)
    r1, r2 = noisy_rep.predict(x), noisy_rep.predict(x)
    assert not np.array_equal(r1, r2) and not np.array_equal(r1, q_cpu)


def test_a_plain_net_allocates_and_launches_nothing_more(L):
    alg, _ = _build()
    from xingtian_amd.algorithm import alg_builder
    mc = {"dueling": True, "SEED": 3, "HIDDEN_SIZE": 8, "NUM_LAYERS": 1}
    info = {"actor": {"model_name": "DqnMlp", "type": "learner", "state_dim": [3], "action_dim": 2, "model_config": mc}}
    cfg = {"instance_num": 1, "agent_num": 1, "prepare_times_per_train": 1, "BUFFER_SIZE": CAP, "BATCH_SIZE": 8,
           "TARGET_UPDATE_FREQ": 3, "GAMMA": GAMMA, "double_dqn": True}
    plain = alg_builder("DQN", info, cfg)
    pnet = plain.actor.net
    assert pnet.params_eff is None and pnet.noise is None and pnet.params.numel() == pnet.spec.n_flat == alg.actor.net.spec.n_net
    with pytest.raises(ValueError, match="no noisy layers"):
        pnet.set_noisy(1, 0.5)
    for m in NH.ring_rows("mlp3")[0]:
        plain.prepare_data(m)
    pnet.lib = N.CountingLib(pnet.lib)
    plain.train_on_slots(list(range(8)))
    plain.actor.predict(NH.ring_rows("mlp3")[2][:4])
    assert pnet.lib.calls["xt_noisy_compose"] == 0 and pnet.lib.calls["xt_noisy_grads"] == 0
    assert "noisy_predict_calls" not in plain.actor.extra_optimizer_state()
