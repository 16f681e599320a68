"""GPU tests of the device-resident non-opt IMPALA train (``DEVICE_VTRACE``): the float64 v-trace kernel
``xt_vtrace_probs_f64`` against the host recursion, ``xt_net_keras_impala_train`` against the existing chunk-wise
``fit_in_order`` bit for bit, and the opt-in switch of ``IMPALA.train``."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GAMMA = 0.99
# import_config overrides module globals for the rest of the process: every model built here restates these
MODEL_CFG = {"NUM_LAYERS": 1, "HIDDEN_SIZE": 128, "LR": 3e-4, "ENTROPY_LOSS": 0.01}


@pytest.fixture(scope="module")
def L():
    from xingtian_amd import lib
    lib.require_gpu()
    lib.load()
    return lib


def to_rows(x, f, t):
    """[F, T, w] per-transition array -> [F * (T + 1), w] row layout (slot T of every fragment zero)"""
    x = np.asarray(x)
    out = np.zeros((f, t + 1) + x.shape[2:], dtype=x.dtype)
    out[:, :t] = x
    return out.reshape((f * (t + 1),) + x.shape[2:])


def from_rows(x, f, t):
    """[F * (T + 1), ...] row layout -> ([F, T, ...] transitions, [F, ...] slot T)"""
    x = np.asarray(x).reshape((f, t + 1) + np.asarray(x).shape[1:])
    return x[:, :t], x[:, t]


def run_vtrace(L, policy, is_logits, value, onehot, behaviour, reward, done, f, t, a, gamma=GAMMA):
    """policy / value in row layout, the rest [F, T, ...]; -> (pg_adv f32 [N], target f32 [N], debug f64 [3, N])"""
    n = f * (t + 1)
    d = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).cuda()
    dev = [d(policy, np.float32), d(value, np.float32), d(to_rows(onehot, f, t), np.float32),
           d(to_rows(behaviour, f, t), np.float32), d(to_rows(reward.reshape(f, t), f, t), np.float64),
           d(to_rows(done.reshape(f, t), f, t), np.uint8)]
    assert dev[0].numel() == n * a and dev[1].numel() == n
    pg = torch.full((n,), 7.0, dtype=torch.float32, device="cuda")
    tg = torch.full((n,), 7.0, dtype=torch.float32, device="cuda")
    dbg = torch.full((3, n), 7.0, dtype=torch.float64, device="cuda")
    L.check(L.load().xt_vtrace_probs_f64(L.ptr(dev[0]), 1 if is_logits else 0, *[L.ptr(x) for x in dev[1:]], f, t, a,
                                         gamma, L.ptr(pg), L.ptr(tg), L.ptr(dbg), L.stream_ptr()), "xt_vtrace_probs_f64")
    torch.cuda.synchronize()
    return pg.cpu().numpy(), tg.cpu().numpy(), dbg.cpu().numpy()


def softmax64(logits):
    x = np.asarray(logits, dtype=np.float64)
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def check_against_host(out, prob64, value, onehot, behaviour, reward, done, f, t):
    """asserts (a)-(e) of the kernel's contract; ``prob64`` [F, T+1, A] is the float64 target policy of the twin"""
    from xingtian_amd.algorithm.impala.impala import rho_from_probs, vtrace_from_probs, vtrace_from_rho
    pg32, tg32, dbg = out
    f64 = lambda x: np.asarray(x, dtype=np.float64)
    v = f64(value).reshape(f, t + 1, 1)
    args = (f64(reward).reshape(f, t, 1), done.reshape(f, t, 1), v[:, :-1], v[:, 1:], GAMMA)
    rho_twin = rho_from_probs(prob64[:, :-1], f64(behaviour), f64(onehot))
    pg_twin, tg_twin = vtrace_from_probs(prob64[:, :-1], f64(behaviour), f64(onehot), *args)
    (rho, rho_pad), (pg, pg_pad), (tg, tg_pad) = [from_rows(dbg[k], f, t) for k in range(3)]
    rel = np.abs(rho[..., None] - rho_twin) / rho_twin
    print("rho: max relative distance to the twin %.3g" % rel.max())
    assert rel.max() <= 1e-13                                                       # (a)
    pg_own, tg_own = vtrace_from_rho(rho[..., None], *args)
    assert np.array_equal(pg[..., None], pg_own) and np.array_equal(tg[..., None], tg_own)      # (b)
    assert np.array_equal(pg32, dbg[1].astype(np.float32)) and np.array_equal(tg32, dbg[2].astype(np.float32))   # (c)
    for got, twin in ((pg[..., None], pg_twin), (tg[..., None], tg_twin)):          # (d)
        assert np.abs(got - twin).max() <= 1e-10 * np.abs(twin).max()
    # (e) slot T of every fragment: rho = 0, pg_adv = 0, target = V_T (the bootstrap value)
    assert np.array_equal(rho_pad, np.zeros(f)) and np.array_equal(pg_pad, np.zeros(f))
    assert np.array_equal(tg_pad, v[:, t, 0])
    assert np.array_equal(from_rows(pg32, f, t)[1], np.zeros(f, np.float32))
    assert np.array_equal(from_rows(tg32, f, t)[1], np.asarray(value, np.float32).reshape(f, t + 1)[:, t])
    return rho


@pytest.mark.parametrize("f,t,a", [(1, 1, 2), (1, 2, 3), (2, 37, 6), (3, 300, 4), (5, 128, 18)])
def test_vtrace_kernel_logits_mode_vs_host_recursion(L, f, t, a):
    """xt_vtrace_probs_f64 on the forward's float32 logits against ``vtrace_from_probs`` in float64 on the float64
    numpy softmax of the same logits, for dones nowhere / at t = 0 / at t = T-1 / on every step.  Special transitions
    (flat index, where the shape has them): 0 -- behaviour probability of the taken action exactly 1 (rho = pt < 1, not
    clipped); 1 -- exactly 0 (rho clips at 1); 2 -- the taken action's logit 60 below the maximum (the 1e-10 dominates)."""
    rng = np.random.default_rng(1000 * f + 10 * t + a)
    n = f * t
    logits = (2.0 * rng.standard_normal((f, t + 1, a))).astype(np.float32)
    value = rng.standard_normal((f, t + 1)).astype(np.float32)
    act = rng.integers(0, a, (f, t))
    beh = softmax64(rng.standard_normal((f, t, a))).astype(np.float32)
    beh.reshape(n, a)[0] = np.eye(a, dtype=np.float32)[act.reshape(n)[0]]
    if n > 1:
        beh.reshape(n, a)[1] = np.eye(a, dtype=np.float32)[(act.reshape(n)[1] + 1) % a]
    if n > 2:
        row = logits[:, :t].reshape(n, a)[2].copy()
        row[act.reshape(n)[2]] = row.max() - 60.0
        logits[2 // t, 2 % t] = row
    onehot = np.eye(a, dtype=np.float32)[act]
    reward = rng.choice([-1.0, 0.0, 1.0, 0.37], (f, t))
    prob64 = softmax64(logits)
    dones = {"none": np.zeros((f, t), bool), "first": np.zeros((f, t), bool), "last": np.zeros((f, t), bool),
             "every": np.ones((f, t), bool)}
    dones["first"][:, 0] = True
    dones["last"][:, t - 1] = True
    for name, done in dones.items():
        out = run_vtrace(L, logits.reshape(-1, a), True, value.reshape(-1), onehot, beh, reward, done, f, t, a)
        rho = check_against_host(out, prob64, value, onehot, beh, reward, done, f, t).reshape(n)
        assert rho[0] < 1.0
        if n > 1:
            assert rho[1] == 1.0
        if n > 2:
            assert rho[2] < 1e-6                   # ~1e-10 / pb: the epsilon, not the probability, sets it
        if n > 50:
            assert (rho == 1.0).sum() > 5 and (rho < 1.0).sum() > 5, name


def test_vtrace_kernel_probabilities_mode_vs_executed_reference(L, golden_dir):
    """Probabilities mode on the model outputs and fragments of the EXECUTED reference (tests/golden/alg_impala.npz):
    the float32 outputs stay within 1e-6 absolute of the pg_adv / target the reference handed to its model, and they are
    the logits-mode arithmetic on the same probabilities: rho within 1e-13 relative of the float64 twin's, everything
    behind rho bit for bit the host recursion on the device's rho, rounded once to float32."""
    from oracle import gen_golden_alg as G
    z = np.load(os.path.join(golden_dir, "alg_impala.npz"))
    msgs = G.impala_plain_inputs()
    f, t = len(msgs), G.IMPALA_PLAIN_CFG[1]["episode_len"]
    a = z["pred_p"].shape[1]
    stack = lambda key: np.stack([np.asarray(m[key]) for m in msgs])
    onehot, beh, reward, done = stack("real_action"), stack("action"), stack("reward"), stack("done")
    assert z["pred_p"].dtype == np.float32 and z["pred_p"].shape == (f * (t + 1), a)
    out = run_vtrace(L, z["pred_p"], False, z["pred_v"].reshape(-1), onehot, beh, reward, done, f, t, a)
    prob64 = z["pred_p"].astype(np.float64).reshape(f, t + 1, a)
    check_against_host(out, prob64, z["pred_v"].reshape(-1), onehot, beh, reward, done, f, t)
    ncalls = int(z["train_ncalls"])
    ref_pg = np.concatenate([z["train_%d_state_1" % i] for i in range(ncalls)]).reshape(-1)
    ref_tg = np.concatenate([z["train_%d_label_1" % i] for i in range(ncalls)]).reshape(-1)
    pg, tg = from_rows(out[0], f, t)[0].reshape(-1), from_rows(out[1], f, t)[0].reshape(-1)
    print("vs executed reference: pg_adv %.3g target %.3g" % (np.abs(pg - ref_pg).max(), np.abs(tg - ref_tg).max()))
    assert np.abs(pg - ref_pg).max() <= 1e-6 and np.abs(tg - ref_tg).max() <= 1e-6


def test_vtrace_kernel_refuses_t_zero_and_launches_nothing(L):
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device="cuda")
    pg, tg = torch.full((4,), 7.0, device="cuda"), torch.full((4,), 7.0, device="cuda")
    args = [L.ptr(z(4, 2)), 1, L.ptr(z(4)), L.ptr(z(4, 2)), L.ptr(z(4, 2)), L.ptr(z(4, dt=torch.float64)),
            L.ptr(z(4, dt=torch.uint8))]
    for f, t, a in ((2, 0, 2), (2, 1025, 2), (2, 1, 65), (0, 1, 2)):
        rc = L.load().xt_vtrace_probs_f64(*args, f, t, a, GAMMA, L.ptr(pg), L.ptr(tg), None, L.stream_ptr())
        assert rc != 0 and b"xt_vtrace_probs_f64" in L.load().xt_last_error()
    torch.cuda.synchronize()
    assert torch.equal(pg, torch.full((4,), 7.0, device="cuda")) and torch.equal(tg, torch.full((4,), 7.0, device="cuda"))


def synth_fragments(rng, f, t, a, state_dim, u8):
    n = f * t
    states = (rng.integers(0, 256, (f * (t + 1),) + tuple(state_dim)).astype(np.uint8) if u8
              else rng.uniform(-1, 1, (f * (t + 1),) + tuple(state_dim)).astype(np.float32))
    beh = rng.random((n, a)) + 0.1
    return dict(states=states, onehot=np.eye(a, dtype=np.float32)[rng.integers(0, a, n)],
                behaviour=(beh / beh.sum(-1, keepdims=True)).astype(np.float32),
                reward=rng.choice([-1.0, 0.0, 1.0], (n, 1)), done=(rng.random((n, 1)) < 0.1))


def transitions(x, f, t):
    """row-layout device tensor / state array -> the F * T transition rows"""
    x = x.cpu().numpy() if torch.is_tensor(x) else x
    return from_rows(x, f, t)[0].reshape((f * t,) + x.shape[1:])


@pytest.mark.parametrize("which,batch_size", [("mlp", 64), ("mlp", 200), ("cnn", 32)])
def test_device_train_is_the_chunkwise_fit_bit_for_bit(which, batch_size):
    """``train_fragments`` on model A (one C call) against the existing ``fit_in_order`` on model B, chunk by chunk, fed
    with the float32 pg_adv / target model A trained on and the same orders: parameters, Adam slots, ``iterations`` and
    the loss are identical.  mlp: 153 rows forward in chunks of 128 + 25 (a fragment is split); BATCH_SIZE 64 -> fit
    calls of 64 / 64 / 22, BATCH_SIZE 200 -> one call of two minibatches (128 + 22).  cnn: chunks of 32 / 8 with the
    per-tensor clip and the decay active."""
    from xingtian_amd.model import model_builder
    if which == "mlp":
        f, t, a, sd = 3, 50, 3, [6]
        info = {"model_name": "ImpalaMlp", "state_dim": sd, "action_dim": a,
                "model_config": dict(MODEL_CFG, SEED=3, MAX_BATCH=128, NUM_LAYERS=2)}
        clip, decay = 0.0, 0.0
    else:
        f, t, a, sd = 2, 20, 5, [36, 36, 4]
        info = {"model_name": "ImpalaCnn", "state_dim": sd, "action_dim": a, "model_config": dict(MODEL_CFG, SEED=3)}
        clip, decay = 0.05, 0.01
    rng = np.random.default_rng(81)
    data = synth_fragments(rng, f, t, a, sd, u8=(which == "cnn"))
    n = f * t
    orders = [rng.permutation(min(batch_size, n - lo)) for lo in range(0, n, batch_size)]
    m_a, m_b = model_builder(info), model_builder(info)
    for m in (m_a, m_b):
        m.CLIPNORM, m.DECAY = clip, decay
    assert torch.equal(m_a.net.params, m_b.net.params)
    w0 = m_a.net.params.clone()
    loss_a = m_a.train_fragments(data["states"], data["onehot"], data["behaviour"], data["reward"], data["done"], t, GAMMA,
                                 batch_size, orders=orders)
    pg, tg = transitions(m_a.last_fragments["pg_adv"], f, t), transitions(m_a.last_fragments["target"], f, t)
    assert pg.dtype == np.float32 and np.isfinite(pg).all() and np.abs(pg).max() > 0
    states_t = transitions(data["states"], f, t)
    losses = [m_b.fit_in_order(states_t[lo:lo + batch_size], pg[lo:lo + batch_size], data["onehot"][lo:lo + batch_size],
                               tg[lo:lo + batch_size], order)
              for lo, order in zip(range(0, n, batch_size), orders)]
    assert loss_a == np.mean(losses) and np.isfinite(loss_a)
    assert m_a.iterations == m_b.iterations == sum((len(o) + 127) // 128 for o in orders)
    assert torch.equal(m_a.net.params, m_b.net.params) and not torch.equal(m_a.net.params, w0)
    assert torch.equal(m_a.net.adam_m, m_b.net.adam_m) and torch.equal(m_a.net.adam_v, m_b.net.adam_v)


REGISTRY_MODEL = {"actor": {"model_name": "ImpalaCnn", "state_dim": [36, 36, 4], "action_dim": 4,
                            "model_config": dict(MODEL_CFG, SEED=5)}}


def registry_alg(device_vtrace):
    from xingtian_amd.algorithm import alg_builder
    cfg = {"instance_num": 2, "agent_num": 1, "prepare_times_per_train": 2, "BATCH_SIZE": 16, "episode_len": 20,
           "GAMMA": GAMMA}
    if device_vtrace is not None:
        cfg["DEVICE_VTRACE"] = device_vtrace
    alg = alg_builder("IMPALA", REGISTRY_MODEL, cfg)
    data = synth_fragments(np.random.default_rng(63), 2, 20, 4, [36, 36, 4], u8=True)
    for k in range(2):
        tr, st = slice(20 * k, 20 * (k + 1)), slice(21 * k, 21 * (k + 1))
        alg.prepare_data({"cur_state": data["states"][st], "real_action": data["onehot"][tr],
                          "reward": [float(x) for x in data["reward"][tr, 0]], "done": [bool(x) for x in data["done"][tr, 0]],
                          "action": data["behaviour"][tr]})
    return alg, data


def test_registry_impala_takes_the_device_path_when_asked():
    """alg_builder("IMPALA", DEVICE_VTRACE: True) on the shapes of test_registry_plain_impala_end_to_end: ``train()``
    returns the loss of the composition logits read back -> float64 softmax -> float64 twin -> float32 ->
    ``fit_in_order`` on a twin model with the same shuffles."""
    from xingtian_amd.algorithm.impala.impala import vtrace_from_probs
    from xingtian_amd.model import model_builder
    from xingtian_amd.model.impala.impala_cnn import draw_fit_orders
    f, t, b = 2, 20, 16
    alg, data = registry_alg(True)
    twin = model_builder(REGISTRY_MODEL["actor"])
    assert torch.equal(twin.net.params, alg.actor.net.params)
    w0 = alg.actor.net.params.clone()
    logits, value = twin.net.forward(data["states"])
    p = softmax64(logits.cpu().numpy()).reshape(f, t + 1, -1)
    v = value.cpu().numpy().astype(np.float64).reshape(f, t + 1, 1)
    frag = lambda x: np.asarray(x, dtype=np.float64).reshape((f, t) + x.shape[1:])
    pg, tg = vtrace_from_probs(p[:, :-1], frag(data["behaviour"]), frag(data["onehot"]), frag(data["reward"]),
                               data["done"].reshape(f, t, 1), v[:, :-1], v[:, 1:], GAMMA)
    pg, tg = pg.reshape(-1).astype(np.float32), tg.reshape(-1).astype(np.float32)
    np.random.seed(9)
    orders = draw_fit_orders(f * t, b)
    states_t = transitions(data["states"], f, t)
    expect = np.mean([twin.fit_in_order(states_t[lo:lo + b], pg[lo:lo + b], data["onehot"][lo:lo + b], tg[lo:lo + b], o)
                      for lo, o in zip(range(0, f * t, b), orders)])
    np.random.seed(9)
    loss = alg.train()
    assert loss == expect and np.isfinite(loss)
    assert alg.actor.iterations == 3 and not torch.equal(alg.actor.net.params, w0)
    assert torch.equal(alg.actor.net.params, twin.net.params)
    assert alg.state == [] and alg.rewards == [] and alg.pred_a == []


@pytest.mark.parametrize("key", [None, False])
def test_registry_impala_stays_on_the_host_path_by_default(key, monkeypatch):
    alg, _ = registry_alg(key)

    def refuse(*args, **kwargs):
        raise AssertionError("the device path was taken without DEVICE_VTRACE")

    monkeypatch.setattr(type(alg.actor), "train_fragments", refuse)
    loss = alg.train()
    assert np.isfinite(loss) and alg.actor.iterations == 3 and alg.state == []


class StubActor(object):
    """predict / train of a model, counting the host path's fit calls; ``train_fragments`` must never be reached"""

    def __init__(self, a):
        self.a, self.fits = a, 0

    def predict(self, state):
        n = len(state[0])
        return [np.full((n, self.a), 1.0 / self.a, np.float32), np.zeros((n, 1), np.float32)]

    def train(self, state, label):
        self.fits += 1
        return 0.5

    def train_fragments(self, *args, **kwargs):
        raise AssertionError("the device path was taken")


class BareActor(object):
    """the same without ``train_fragments``"""
    __init__, predict, train = StubActor.__init__, StubActor.predict, StubActor.train


@pytest.mark.parametrize("case", ["t1025", "a65", "no_method", "control"])
def test_device_path_refusals_fall_back_to_the_host_path(case):
    """T = 1025, A = 65 and an actor without ``train_fragments`` take the host path although DEVICE_VTRACE is set (and
    raise nothing); the control (T = 1024, A = 64, a stub WITH the method) does reach the method."""
    from xingtian_amd.algorithm import alg_builder
    t, a = {"t1025": (1025, 2), "a65": (8, 65), "no_method": (8, 2), "control": (1024, 64)}[case]
    alg = alg_builder("IMPALA", {"actor": {"model_name": "ImpalaMlp", "state_dim": [4], "action_dim": 2,
                                           "model_config": dict(MODEL_CFG, SEED=1)}},
                      {"instance_num": 1, "agent_num": 1, "prepare_times_per_train": 1, "BATCH_SIZE": 512, "episode_len": t,
                       "GAMMA": GAMMA, "DEVICE_VTRACE": True})
    alg.actor = BareActor(a) if case == "no_method" else StubActor(a)
    assert hasattr(alg.actor, "train_fragments") == (case != "no_method")
    alg.action_dim = a
    rng = np.random.default_rng(3)
    alg.prepare_data({"cur_state": rng.uniform(-1, 1, (t + 1, 4)).astype(np.float32),
                      "real_action": np.eye(a, dtype=np.float32)[rng.integers(0, a, t)], "reward": [1.0] * t,
                      "done": [False] * t, "action": np.full((t, a), 1.0 / a, np.float32)})
    if case == "control":
        with pytest.raises(AssertionError, match="device path"):
            alg.train()
        return
    assert alg.train() == 0.5 and alg.actor.fits == (t + 511) // 512 and alg.state == []
