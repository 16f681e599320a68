"""GPU tests of the device acting path: ``act_heads_kernel`` alone (``xt_act_heads``), through ``xt_net_act`` /
``HipActorCritic.act`` and through ``model_config.PREDICT_ON_DEVICE`` of the PPO models and ``ImpalaCnnOpt``."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import act_helpers as H

pytestmark = pytest.mark.gpu

# (B, F, A): B = 5 / 7 leave a block partly filled, F = 200 is no multiple of 64, A = 3 / 18 are no powers of two
CAT_SHAPES = [(1, 64, 2), (5, 200, 3), (4, 256, 4), (7, 256, 6), (3, 256, 18), (2, 64, 64)]
GAUSS_SHAPES = [(5, 200, 1), (7, 256, 3), (4, 64, 6)]


@pytest.fixture(scope="module")
def L():
    from xingtian_amd import lib
    lib.require_gpu()
    lib.load()
    return lib


@pytest.fixture(autouse=True)
def _module_constants_restored():
    """import_config overrides the model modules' constants for the rest of the process: put them back"""
    from xingtian_amd.model.impala import impala_cnn_opt
    from xingtian_amd.model.ppo import ppo
    saved = [(m, {k: v for k, v in vars(m).items() if k.isupper()}) for m in (ppo, impala_cnn_opt)]
    yield
    torch.cuda.synchronize()
    for m, consts in saved:
        vars(m).update(consts)


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def act_heads(lib, f_pi, f_v, wpi, bpi, wv, bv, log_std=None, noise=None, seed=0, call=0, row0=0, want_noise=False):
    """one ``xt_act_heads`` launch -> dict of host arrays"""
    h = lib.load()
    b, f = f_pi.shape
    a = wpi.shape[1]
    gauss = log_std is not None
    keep = [dev(x) for x in (f_pi, f_v, wpi, bpi, wv, bv)]
    d_ls = dev(log_std) if gauss else None
    d_noise = dev(noise) if noise is not None else None
    action = torch.zeros((b, a), dtype=torch.float32, device="cuda") if gauss else \
        torch.full((b,), -1, dtype=torch.int32, device="cuda")
    logp, value = torch.zeros(b, device="cuda"), torch.zeros(b, device="cuda")
    logits = torch.zeros((b, a), device="cuda")
    nz = torch.zeros((b, a), device="cuda") if want_noise else None
    cfg = lib.ActCfg(int(seed), int(call), int(row0), 1 if want_noise else 0)
    lib.check(h.xt_act_heads(lib.ptr(keep[0]), lib.ptr(keep[1]), b, f, a, lib.ptr(keep[2]), lib.ptr(keep[3]),
                             lib.ptr(keep[4]), lib.ptr(keep[5]), lib.ptr(d_ls), ctypes.byref(cfg), lib.ptr(d_noise),
                             lib.ptr(action), lib.ptr(logp), lib.ptr(value), lib.ptr(logits), lib.ptr(nz), None),
              "xt_act_heads")
    torch.cuda.synchronize()
    out = dict(action=action.cpu().numpy(), logp=logp.cpu().numpy(), value=value.cpu().numpy(),
               logits=logits.cpu().numpy())
    if want_noise:
        out["noise"] = nz.cpu().numpy()
    return out


def heads_fwd(lib, f_pi, f_v, wpi, bpi, wv, bv):
    b, f = f_pi.shape
    a = wpi.shape[1]
    keep = [dev(x) for x in (f_pi, f_v, wpi, bpi, wv, bv)]
    logits, value = torch.zeros((b, a), device="cuda"), torch.zeros(b, device="cuda")
    lib.check(lib.load().xt_heads_fwd(lib.ptr(keep[0]), lib.ptr(keep[1]), b, f, a, lib.ptr(keep[2]), lib.ptr(keep[3]),
                                      lib.ptr(keep[4]), lib.ptr(keep[5]), lib.ptr(logits), lib.ptr(value), None),
              "xt_heads_fwd")
    torch.cuda.synchronize()
    return logits.cpu().numpy(), value.cpu().numpy()


@functools.lru_cache(maxsize=None)
def kernel_case(shape, gauss):
    """random features / head weights / injected noise of one shape, the kernel's outputs and ``xt_heads_fwd``'s on the same
    inputs: computed once, shared by G1 - G3 (nobody writes into it)"""
    from xingtian_amd import lib
    b, f, a = shape
    rng = np.random.default_rng(1000 * b + 10 * a + f + (7 if gauss else 0))
    f32 = lambda x: np.asarray(x, dtype=np.float32)
    f_pi, f_v = f32(rng.standard_normal((b, f))), f32(np.tanh(rng.standard_normal((b, f))))
    heads = (f32(rng.standard_normal((f, a)) * 0.3), f32(rng.standard_normal(a)), f32(rng.standard_normal((f, 1)) * 0.1),
             np.array([0.3], np.float32))
    log_std = f32(rng.uniform(-1.5, 0.5, a)) if gauss else None
    noise = f32(rng.standard_normal((b, a))) if gauss else f32(-np.log(-np.log(rng.random((b, a)))))
    out = act_heads(lib, f_pi, f_v, *heads, log_std=log_std, noise=noise)
    ref_logits, ref_value = heads_fwd(lib, f_pi, f_v, *heads)
    for v in list(out.values()) + [ref_logits, ref_value, noise]:
        v.setflags(write=False)
    return dict(out=out, ref_logits=ref_logits, ref_value=ref_value, noise=noise, log_std=log_std)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------ G1: the kernel alone, injected noise
@pytest.mark.parametrize("shape", CAT_SHAPES)
def test_kernel_logits_value_and_argmax(L, shape):
    c = kernel_case(shape, False)
    out = c["out"]
    assert np.array_equal(bits(out["logits"]), bits(c["ref_logits"]))
    assert np.array_equal(bits(out["value"]), bits(c["ref_value"]))
    assert out["action"].dtype == np.int32
    assert np.array_equal(out["action"], np.argmax(out["logits"] + c["noise"], axis=1))      # one float32 add, first max


@pytest.mark.parametrize("shape", GAUSS_SHAPES)
def test_kernel_gaussian_mean_value_and_action(L, shape):
    c = kernel_case(shape, True)
    out = c["out"]
    assert np.array_equal(bits(out["logits"]), bits(c["ref_logits"]))
    assert np.array_equal(bits(out["value"]), bits(c["ref_value"]))
    # mean + exp(log_std) * eps: the device's expf is within a few ulp of numpy's, product and sum are single roundings
    std = np.exp(c["log_std"].astype(np.float64))
    ref = out["logits"].astype(np.float64) + std * c["noise"]
    assert np.abs(out["action"] - ref).max() <= 8 * 2.0 ** -24 * (np.abs(ref).max() + np.abs(std * c["noise"]).max())


def test_kernel_ties_go_to_the_lowest_index(L):
    b, f = 6, 64
    z = np.zeros((b, f), np.float32)
    wv, bv = np.zeros((f, 1), np.float32), np.zeros(1, np.float32)
    for bias, want in (([0.25] * 5, 0), ([0.0, 1.0, 1.0, 0.5], 1), ([-1.0, 2.0, 0.0, 2.0, 2.0, 1.0], 1)):
        a = len(bias)
        out = act_heads(L, z, z, np.zeros((f, a), np.float32), np.array(bias, np.float32), wv, bv,
                        noise=np.zeros((b, a), np.float32))
        assert np.array_equal(out["logits"], np.tile(np.array(bias, np.float32), (b, 1)))
        assert (out["action"] == want).all(), (bias, out["action"])
    # a tie that only the noise makes: logit + noise equal at indices 1 and 3
    noise = np.tile(np.array([0.0, 1.0, 0.0, 0.5], np.float32), (b, 1))
    out = act_heads(L, z, z, np.zeros((f, 4), np.float32), np.array([0.0, 0.5, 0.0, 1.0], np.float32), wv, bv, noise=noise)
    assert (out["action"] == 1).all()
    # non-finite logits still give an index in range
    out = act_heads(L, z, z, np.zeros((f, 3), np.float32), np.array([np.nan, np.inf, -np.inf], np.float32), wv, bv,
                    noise=np.zeros((b, 3), np.float32))
    assert ((out["action"] >= 0) & (out["action"] < 3)).all()


# ------------------------------------------------------------------ G2: the loss kernel recomputes the same logp
def surrogate_terms(lib, out, a, log_std=None):
    """loss_terms[:, 0] of xt_ppo_loss / xt_ppo_loss_gauss fed the acting call's own outputs as labels (adv = 1)"""
    b = len(out["logp"])
    h = lib.load()
    keep = [dev(out["logits"]), dev(out["value"]), dev(out["action"]), dev(out["logp"]), dev(np.ones(b, np.float64)),
            dev(out["value"]), dev(out["value"].astype(np.float64))]
    d1, d2 = torch.zeros((b, a), device="cuda"), torch.zeros(b, device="cuda")
    terms = torch.full((b, 4), -7.0, device="cuda")
    if log_std is None:
        lib.check(h.xt_ppo_loss(lib.ptr(keep[0]), lib.ptr(keep[1]), b, a, None, lib.ptr(keep[2]), lib.ptr(keep[3]),
                                lib.ptr(keep[4]), lib.ptr(keep[5]), lib.ptr(keep[6]), 0.1, 0.0, 5.0, 1.0, 1.0 / b,
                                lib.ptr(d1), lib.ptr(d2), lib.ptr(terms), None), "xt_ppo_loss")
    else:
        rows = torch.zeros((b, a), device="cuda")
        d_ls = dev(log_std)
        lib.check(h.xt_ppo_loss_gauss(lib.ptr(keep[0]), lib.ptr(d_ls), lib.ptr(keep[1]), b, a, None, lib.ptr(keep[2]),
                                      lib.ptr(keep[3]), lib.ptr(keep[4]), lib.ptr(keep[5]), lib.ptr(keep[6]), 0.1, 0.0, 5.0,
                                      1.0, 1.0 / b, lib.ptr(d1), lib.ptr(d2), lib.ptr(rows), lib.ptr(terms), None),
                  "xt_ppo_loss_gauss")
    torch.cuda.synchronize()
    return terms.cpu().numpy()[:, 0]


ONE = np.array([1.0], np.float32).view(np.uint32)[0]


@pytest.mark.parametrize("shape", CAT_SHAPES)
def test_first_epoch_ratio_is_exactly_one(L, shape):
    out = kernel_case(shape, False)["out"]
    surr = surrogate_terms(L, out, shape[2])
    assert (bits(surr) == ONE).all(), surr


@pytest.mark.parametrize("shape", GAUSS_SHAPES)
def test_first_epoch_ratio_is_exactly_one_gaussian(L, shape):
    c = kernel_case(shape, True)
    surr = surrogate_terms(L, c["out"], shape[2], log_std=c["log_std"])
    assert (bits(surr) == ONE).all(), surr


@pytest.mark.parametrize("bias", [[100.0, 0.0, -100.0], [100.0, 0.0, -100.0, 50.0, -50.0, 0.0]])
def test_ratio_is_one_for_a_forced_unlikely_action(L, bias):
    b, f, a = 3, 64, len(bias)
    z = np.zeros((b, f), np.float32)
    noise = np.zeros((b, a), np.float32)
    noise[:, 2] = 1000.0                           # forces the action whose probability is e^-200
    out = act_heads(L, z, z, np.zeros((f, a), np.float32), np.array(bias, np.float32), np.zeros((f, 1), np.float32),
                    np.zeros(1, np.float32), noise=noise)
    assert (out["action"] == 2).all() and np.isfinite(out["logp"]).all()
    assert np.abs(out["logp"] + 200.0).max() < 1e-4
    assert (bits(surrogate_terms(L, out, a)) == ONE).all()


# ------------------------------------------------------------------ G3: logp against float64
def check_logp_bound(tag, logp_dev, logp_host, ref):
    e_dev, e_host = np.abs(logp_dev.reshape(-1) - ref.reshape(-1)).max(), np.abs(logp_host.reshape(-1) - ref.reshape(-1)).max()
    bound = H.logp_bound(e_host, ref)
    print("logp vs float64 [%s]: device %.3g host %.3g bound %.3g" % (tag, e_dev, e_host, bound))
    assert e_dev <= bound, (tag, e_dev, e_host, bound)
    return e_dev, e_host


@pytest.mark.parametrize("shape", CAT_SHAPES)
def test_logp_against_float64(L, shape):
    out = kernel_case(shape, False)["out"]
    ref = H.cat_logp_ref(out["logits"], out["action"])
    check_logp_bound("cat %s" % (shape,), out["logp"], H.cat_logp_host(out["logits"], out["action"]), ref)


@pytest.mark.parametrize("shape", GAUSS_SHAPES)
def test_logp_against_float64_gaussian(L, shape):
    c = kernel_case(shape, True)
    out = c["out"]
    ref = H.gauss_logp_ref(out["logits"], c["log_std"], out["action"])
    check_logp_bound("gauss %s" % (shape,), out["logp"], H.gauss_logp_host(out["logits"], c["log_std"], out["action"]), ref)


# ------------------------------------------------------------------ G4: the generator, through xt_net_act in chunks
def mlp_net(a, max_batch, action_type="Categorical"):
    from xingtian_amd.model import netspec
    from xingtian_amd.model.hip_net import HipActorCritic
    return HipActorCritic(netspec.ppo_mlp((4,), a, (64, 64), "tanh", False, action_type), max_batch=max_batch, seed=3)


def same_block(x, y):
    return x.keys() == y.keys() and all(np.array_equal(x[k].view(np.uint32), y[k].view(np.uint32)) for k in x)


@pytest.mark.parametrize("a", [2, 6, 18])
def test_generator_matches_the_restatement_across_chunks(L, a):
    b, seed, call = 300, (0xC0FFEE << 32) | 0x1234, (1 << 32) | 41
    obs = np.random.default_rng(a).standard_normal((b, 4)).astype(np.float32)
    net = mlp_net(a, 128)                                     # three chunks: 128 + 128 + 44
    out = net.act(obs, seed, call, want_noise=True)
    g = H.gumbel(seed, call, np.arange(b), a)                 # rows 128..299 at their GLOBAL index
    assert (np.abs(out["noise"].astype(np.float64) - g) <= 1e-5 * np.maximum(1.0, np.abs(g))).all()
    assert np.array_equal(out["action"], np.argmax(out["logits"] + out["noise"], axis=1))
    assert out["action"].dtype == np.int32 and out["logp"].shape == (b, 1) and out["value"].shape == (b, 1)
    # the same key and counter: the same block, bit for bit; the next call: other noise
    assert same_block(out, net.act(obs, seed, call, want_noise=True))
    nxt = net.act(obs, seed, call + 1, want_noise=True)
    assert (np.any(nxt["noise"] != out["noise"], axis=1)).sum() >= b // 2
    # chunking is invisible: one chunk of 300 on a wider net gives the same block
    wide = mlp_net(a, 512)
    assert same_block(out, wide.act(obs, seed, call, want_noise=True))
    # without want_noise the other arrays are the same, and an injected noise is the noise used
    plain = net.act(obs, seed, call)
    assert "noise" not in plain and same_block({k: out[k] for k in plain}, plain)
    inj = net.act(obs, seed, call, noise=out["noise"], want_noise=True)
    assert same_block(out, inj)


def test_generator_gaussian_matches_box_muller(L):
    b, a, seed, call = 300, 3, 99, 5
    obs = np.random.default_rng(1).standard_normal((b, 4)).astype(np.float32)
    net = mlp_net(a, 128, "DiagGaussian")
    out = net.act(obs, seed, call, want_noise=True)
    eps = H.gauss_eps(seed, call, np.arange(b), a)
    assert (np.abs(out["noise"].astype(np.float64) - eps) <= 1e-5 * np.maximum(1.0, np.abs(eps))).all()
    assert out["action"].shape == (b, a) and out["action"].dtype == np.float32
    assert same_block(out, net.act(obs, seed, call, want_noise=True))
    assert same_block(out, mlp_net(a, 512, "DiagGaussian").act(obs, seed, call, want_noise=True))


# ------------------------------------------------------------------ G5: the sampling law
@pytest.mark.parametrize("case", range(3))
def test_categorical_sampling_law(L, case):
    logits = H.LAW_LOGITS[case]
    n, f, a = H.LAW_N, 64, len(logits)
    z = np.zeros((n, f), np.float32)
    out = act_heads(L, z, z, np.zeros((f, a), np.float32), logits, np.zeros((f, 1), np.float32), np.zeros(1, np.float32),
                    seed=H.LAW_SEED, call=H.LAW_CALL)
    assert np.array_equal(out["logits"], np.tile(logits, (n, 1)))
    sig = H.categorical_law_sigmas(out["action"], logits)
    print("A = %d: largest deviation %.2f sigma" % (a, sig.max()))
    assert (sig <= 5.0).all(), sig


def test_gaussian_sampling_law(L):
    n, f, a = H.LAW_N, 64, 3
    z = np.zeros((n, f), np.float32)
    out = act_heads(L, z, z, np.zeros((f, a), np.float32), np.zeros(a, np.float32), np.zeros((f, 1), np.float32),
                    np.zeros(1, np.float32), log_std=np.zeros(a, np.float32), seed=H.LAW_SEED, call=H.LAW_CALL,
                    want_noise=True)
    sig = H.gauss_law_sigmas(out["noise"])
    print("mean %.2f, variance %.2f, correlation %.2f sigma" % sig)
    assert max(sig) <= 5.0, sig
    assert np.array_equal(out["action"], out["noise"])          # mean 0, std exp(0) = 1


# ------------------------------------------------------------------ G6: through the models
PAIRS = {
    "PpoMlp": (dict(model_name="PpoMlp", state_dim=[4], action_dim=2), dict(BATCH_SIZE=8), (5, 4), np.float32),
    "PpoCnn": (dict(model_name="PpoCnn", state_dim=[84, 84, 4], action_dim=4, input_dtype="uint8"),
               dict(BATCH_SIZE=4, VF_SHARE_LAYERS=True, hidden_sizes=[256], activation="relu"), (5, 84, 84, 4), np.uint8),
    "ImpalaCnnOpt": (dict(model_name="ImpalaCnnOpt", state_dim=[42, 42, 4], action_dim=6, input_dtype="uint8",
                          state_mean=128.0, state_std=128.0), dict(MAX_BATCH=8, sample_batch_step=5), (10, 42, 42, 4),
                     np.uint8),
}


def build(which, **extra):
    from xingtian_amd.model import model_builder
    info, cfg, _, _ = PAIRS[which]
    return model_builder(dict(info, model_config=dict(cfg, SEED=21, DEVICE="gpu", **extra)))


def observations(which, seed=0):
    _, _, shape, dtype = PAIRS[which]
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, shape).astype(dtype) if dtype == np.uint8 else rng.standard_normal(shape).astype(dtype)


def same_results(x, y):
    return len(x) == len(y) and all(p.dtype == q.dtype and p.shape == q.shape and np.array_equal(p, q) for p, q in zip(x, y))


@pytest.mark.parametrize("which", list(PAIRS))
def test_models_predict_on_the_device(L, which):
    off, on, on2 = build(which, PREDICT_ON_DEVICE=False), build(which, PREDICT_ON_DEVICE=True), build(which, PREDICT_ON_DEVICE=True)
    assert off._act is None and on._act == dict(seed=21, call=0)
    obs = observations(which)
    r_off, r_on = off.predict(obs), on.predict(obs)
    assert len(r_off) == len(r_on) and all(p.dtype == q.dtype and p.shape == q.shape for p, q in zip(r_off, r_on))
    logits, _ = on.net.forward(obs)
    logits = logits.cpu().numpy()
    a = logits.shape[1]
    if which == "ImpalaCnnOpt":
        assert np.array_equal(bits(r_off[0]), bits(r_on[0])) and np.array_equal(bits(r_off[0]), bits(logits))
        assert np.array_equal(bits(r_off[1]), bits(r_on[1])) and r_on[1].shape == (len(obs),)
        action = r_on[2]
    else:
        assert np.array_equal(bits(r_off[2]), bits(r_on[2])) and r_on[2].shape == (len(obs), 1)
        action = r_on[0]
        ref = H.cat_logp_ref(logits, action)
        check_logp_bound(which, r_on[1], H.cat_logp_host(logits, action), ref)
    assert action.dtype == np.int32 and action.shape == (len(obs),) and ((action >= 0) & (action < a)).all()
    # equal SEED: the same sequence of results over three calls (the first one of `on` is r_on)
    seq = [r_on] + [on.predict(observations(which, k)) for k in (1, 2)]
    seq2 = [on2.predict(observations(which, k)) for k in (0, 1, 2)]
    assert all(same_results(x, y) for x, y in zip(seq, seq2)) and on._act["call"] == 3


@pytest.mark.parametrize("which", list(PAIRS))
def test_key_off_is_the_path_without_the_key(L, which):
    off, bare = build(which, PREDICT_ON_DEVICE=False), build(which)
    assert off._act is None and bare._act is None
    for k in range(3):
        obs = observations(which, k)
        assert same_results(off.predict(obs), bare.predict(obs))


def test_pendulum_shape_predicts_without_reading_the_weights_back(L, monkeypatch):
    from xingtian_amd.model import model_builder
    m = model_builder(dict(model_name="PpoMlp", state_dim=[3], action_dim=1,
                           model_config=dict(action_type="DiagGaussian", BATCH_SIZE=64, SEED=2, DEVICE="gpu",
                                             PREDICT_ON_DEVICE=True)))
    log_std = m.net.get_weights()["pi_logstd"].reshape(-1)

    def no_read_back(*args, **kwargs):
        raise AssertionError("predict read the weights back")

    monkeypatch.setattr(m.net, "get_weights", no_read_back)
    obs = np.random.default_rng(0).standard_normal((10, 3)).astype(np.float32)
    action, logp, value = m.predict(obs)
    assert action.shape == (10, 1) and action.dtype == np.float32 and logp.shape == value.shape == (10, 1)
    assert logp.dtype == value.dtype == np.float32
    mean, _ = m.net.forward(obs)
    mean = mean.cpu().numpy()
    ref = H.gauss_logp_ref(mean, log_std, action)
    check_logp_bound("pendulum", logp, H.gauss_logp_host(mean, log_std, action), ref)


# ------------------------------------------------------------------ G7: refusals
def test_refusals(L):
    from xingtian_amd.model import model_builder
    h = L.load()
    net = mlp_net(65, 16)
    obs = torch.zeros((16, 4), device="cuda")
    action = torch.zeros(16, dtype=torch.int32, device="cuda")
    logp, value, logits = torch.zeros(16, device="cuda"), torch.zeros(16, device="cuda"), torch.zeros((16, 65), device="cuda")
    cfg = L.ActCfg(1, 0, 0, 0)
    call = lambda n, b: h.xt_net_act(n.handle, ctypes.byref(cfg), L.ptr(obs), None, b, None, L.ptr(action), L.ptr(logp),
                                     L.ptr(value), L.ptr(logits), None, None)
    assert call(net, 4) != 0 and b"A = 65" in h.xt_last_error()
    with pytest.raises(RuntimeError, match="A = 65"):
        net.act(np.zeros((4, 4), np.float32), 1, 0)
    ok = mlp_net(2, 16)
    assert call(ok, 0) != 0 and b"batch 0" in h.xt_last_error()
    assert call(ok, 17) != 0 and b"batch 17" in h.xt_last_error()
    assert call(ok, 16) == 0
    torch.cuda.synchronize()
    # 65 actions with the key on: the host path, as without the key
    wide = [model_builder(dict(model_name="PpoMlp", state_dim=[4], action_dim=65,
                               model_config=dict(BATCH_SIZE=8, SEED=4, DEVICE="gpu", **extra)))
            for extra in (dict(PREDICT_ON_DEVICE=True), dict())]
    assert wide[0]._act is None
    x = np.random.default_rng(0).standard_normal((5, 4)).astype(np.float32)
    assert same_results(wide[0].predict(x), wide[1].predict(x))
