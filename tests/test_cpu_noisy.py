"""CPU tests of the noisy layers (NoisyNet): the layout a noisy spec adds behind today's, the host twins of the noise draw
(Philox known answers, the law of the draw), the initial values, the CPU replica, the refusals of the configuration keys
and of the two C entries (host checks: nothing is launched), and the ABI."""
import ctypes
import os
import re

import numpy as np
import pytest

import act_helpers as A
import noisy_helpers as NH
from xingtian_amd.model import model_builder, netspec
from xingtian_amd.model.cpu_net import CpuActorCritic, initial_weights
from xingtian_amd.model.dqn import dqn_cnn as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _info(name, state_dim, a_dim, **mc):
    mc.setdefault("DEVICE", "cpu")
    return {"model_name": name, "state_dim": list(state_dim), "action_dim": a_dim, "model_config": mc}


# ------------------------------------------------------------------------------------------------ layout
SPECS = [("cnn", dict(dueling=False)), ("cnn", dict(dueling=True)), ("cnn", dict(atoms=5)), ("mlp", dict(dueling=True)),
         ("mlp", dict(quantiles=4)), ("mlp3", dict(dueling=False)), ("mlp2", dict(dueling=True))]


def _spec(kind, noisy, **kw):
    if kind == "cnn":
        return netspec.dqn_cnn((84, 84, 4), 3, noisy=noisy, **kw)
    if kind == "mlp2":                                        # two trunk layers: only the last one is noisy
        return netspec.dqn_mlp((6,), 3, 16, 2, noisy=noisy, **kw)
    return netspec.dqn_mlp((3,) if kind == "mlp3" else (4,), 3, 16, 1, noisy=noisy, **kw)


@pytest.mark.parametrize("kind,kw", SPECS, ids=["%s-%s" % (k, "-".join("%s%s" % i for i in kw.items())) for k, kw in SPECS])
def test_a_noisy_spec_adds_exactly_the_sigma_names_behind_n_net(kind, kw):
    plain, noisy = _spec(kind, False, **kw), _spec(kind, True, **kw)
    assert not hasattr(plain, "noisy_layers") and not hasattr(plain, "n_net")
    assert noisy.n_net == plain.n_flat and noisy.n_flat > noisy.n_net
    # every earlier name keeps its offset and shape, in the same order
    assert list(noisy.names.items())[:len(plain.names)] == list(plain.names.items())
    assert all(noisy.store_shape[k] == v for k, v in plain.store_shape.items())
    last = noisy.layers[-1].name
    want = [last, noisy.pi_name] + ([noisy.v_name] if kw.get("dueling") else [])
    assert last == {"cnn": "dense", "mlp": "dense", "mlp3": "dense", "mlp2": "dense_1"}[kind]
    assert [nl.name for nl in noisy.noisy_layers] == want and [nl.index for nl in noisy.noisy_layers] == list(range(len(want)))
    extra = list(noisy.names)[len(plain.names):]
    assert extra == [n + s for n in want for s in ("/sigma_kernel", "/sigma_bias")]
    width = 3 * kw.get("atoms", 1) * kw.get("quantiles", 1)
    head = noisy.noisy_layers[1]
    assert (head.K, head.N) == (noisy.feat, width) and noisy.names[noisy.pi_name + "/sigma_kernel"][1] == (noisy.feat, width)
    if kw.get("dueling"):
        assert (noisy.noisy_layers[2].K, noisy.noisy_layers[2].N) == (noisy.feat, 1)
    end = noisy.n_net
    for nl in noisy.noisy_layers:                             # the sigma blocks: 16-byte aligned, in order, no overlap
        assert nl.sigma_off % 4 == 0 and nl.sigma_off >= end and nl.w_off % 4 == 0 and nl.noise_off % 4 == 0
        assert noisy.names[nl.name + "/kernel"][0] == nl.w_off and noisy.names[nl.name + "/bias"][0] == nl.w_off + nl.K * nl.N
        assert noisy.names[nl.name + "/sigma_kernel"] == (nl.sigma_off, noisy.names[nl.name + "/kernel"][1])
        assert noisy.names[nl.name + "/sigma_bias"] == (nl.sigma_off + nl.K * nl.N, (nl.N,))
        end = nl.sigma_off + (nl.K + 1) * nl.N
    assert noisy.n_flat == NH.align4(end)
    assert noisy.n_params == sum(int(np.prod(s)) for _, s in noisy.names.values())


def test_a_model_asked_for_noisy_builds_a_noisy_net_and_a_plain_one_is_todays():
    """fails on a tree without the feature: ``noisy: true`` builds a plain net there"""
    for name, sd in (("DqnCnn", (84, 84, 4)), ("DqnMlp", (3,))):
        plain = model_builder(_info(name, sd, 2, dueling=True, SEED=1))
        noisy = model_builder(_info(name, sd, 2, dueling=True, SEED=1, noisy=True))
        ps, ns = plain.net.spec, noisy.net.spec
        today = netspec.dqn_cnn(sd, 2, True) if name == "DqnCnn" else netspec.dqn_mlp(sd, 2, dueling=True)
        assert list(ps.names.items()) == list(today.names.items()) and ps.n_flat == today.n_flat
        assert ps.store_shape == today.store_shape and not hasattr(ps, "noisy_layers")
        assert len(ns.names) == len(ps.names) + 6 and ns.n_net == ps.n_flat and noisy.net.params.size == ns.n_flat
        assert list(D.dqn_spec(_info(name, sd, 2, dueling=True, noisy=True)).names) == list(ns.names)
        assert sorted(noisy.get_weights()) == sorted(ns.names)
        # a checkpoint of the plain model loads into the noisy one: the means take it, the sigmas stay
        before = noisy.get_weights()
        noisy.set_weights(plain.get_weights())
        after = noisy.get_weights()
        for k, v in plain.get_weights().items():
            assert np.array_equal(after[k], v)
        assert all(np.array_equal(after[k], before[k]) for k in after if "sigma" in k)


# ------------------------------------------------------------------------------------------------ the draw
def test_philox_twin_reproduces_the_known_answers():
    hexs = lambda w: " ".join("%08x" % int(x) for x in np.asarray(w).reshape(-1))
    f = 0xFFFFFFFF
    assert hexs(D.noisy_philox((0, 0, 0, 0), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert hexs(D.noisy_philox((f, f, f, f), (f, f))) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    pi = ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))
    assert hexs(D.noisy_philox(*pi)) == hexs(A.philox4x32_10(*pi)) == "d16cfe09 94fdcceb 5001e420 24126ea1"
    c = (np.arange(70000, 70009), 5, np.array(3), 2)
    assert np.array_equal(D.noisy_philox(c, (0x9ABCDEF0, 0x12345678)), A.philox4x32_10(c, (0x9ABCDEF0, 0x12345678)))


def test_uniforms_take_the_documented_counter_words():
    seed, call, stream, layer, side = (0x12345678 << 32) | 0x9ABCDEF0, (7 << 32) | 41, 2, 3, 1
    u1, u2 = D.noisy_uniforms(seed, call, stream, layer, side, 9)
    assert u1.dtype == u2.dtype == np.float32
    for i in range(9):
        w = A.philox4x32_10((i >> 1, 2 * layer + side, 41, stream), (0x9ABCDEF0, 0x12345678))      # (call: its low word)
        assert u1[i] == A.uniform(w[2 * (i & 1)]) and u2[i] == A.uniform(w[2 * (i & 1) + 1])


def test_law_of_the_draw_over_65536_elements():
    n = 65536
    f = D.noisy_f(*D.noisy_uniforms(2026, 7, 0, 1, 0, n))
    assert f.dtype == np.float32 and np.isfinite(f).all()
    x = NH.squared(f)
    print("noisy draw: mean", x.mean(), "variance", x.var())
    assert abs(x.mean()) <= 0.02                              # 5 standard errors at 1 / 256
    assert abs(x.var() - 1.0) <= 0.03                         # (standard error 0.55 %)
    others = [D.noisy_f(*D.noisy_uniforms(2026, c, s, 1, 0, n)) for c, s in ((7, 1), (7, 2), (8, 0))]
    s1, s2, c1 = others
    for a, b in ((f, s1), (f, s2), (s1, s2), (f, c1)):        # streams 0, 1, 2 pairwise; calls c and c + 1
        assert (a != b).mean() > 0.99
    # the other side and another layer are other draws too
    assert (f != D.noisy_f(*D.noisy_uniforms(2026, 7, 0, 1, 1, n))).mean() > 0.99
    assert (f != D.noisy_f(*D.noisy_uniforms(2026, 7, 0, 2, 0, n))).mean() > 0.99


def test_vector_bar_is_four_times_the_float32_restatements_deviation():
    measured, bar = NH.vector_bar()
    print("noisy vectors: float32 NumPy restatement vs the float64 twin, max |f|f| - x| =", measured, "-> bar", bar)
    # the derivation: the rounding of the cosine's argument (2^-24 * 2 pi) times the largest amplitude sqrt(-2 log 2^-24)
    assert 0.0 < measured <= 2.0 ** -24 * 2 * np.pi * np.sqrt(-2 * np.log(2.0 ** -24)) * 1.5 and bar == 4.0 * measured


def test_host_compose_and_sigma_gradients_follow_the_definitions_elementwise():
    t = NH.table(*NH.THREE)
    store = NH.store_of(t, 3)
    noise = D.noisy_vectors(t, 5, 6, 1)
    eff = D.noisy_effective(t, store, noise)
    grads = NH.store_of(t, 4)
    gs = D.noisy_sigma_grads(t, grads, noise)
    touched = np.zeros(t.n_net, bool)
    for nl in t.noisy_layers:
        f_in, f_out = noise[nl.f_in], noise[nl.f_out]
        assert len(f_in) == nl.K and len(f_out) == nl.N
        for k, n in ((0, 0), (nl.K - 1, nl.N - 1), (nl.K // 2, nl.N // 3)):
            i = k * nl.N + n
            e = np.float32(f_in[k] * f_out[n])
            assert eff[nl.w_off + i] == np.float32(store[nl.w_off + i] + np.float32(store[nl.sigma_off + i] * e))
            assert gs[nl.sigma_off + i] == np.float32(grads[nl.w_off + i] * e)
        b = nl.K * nl.N + nl.N - 1
        assert eff[nl.w_off + b] == np.float32(store[nl.w_off + b] + np.float32(store[nl.sigma_off + b] * f_out[-1]))
        assert gs[nl.sigma_off + b] == np.float32(grads[nl.w_off + b] * f_out[-1])
        touched[nl.w_off:nl.w_off + (nl.K + 1) * nl.N] = True
    assert np.array_equal(NH.bits(eff[~touched]), NH.bits(store[:t.n_net][~touched])) and touched.sum() < t.n_net
    assert np.array_equal(NH.bits(gs[:t.n_net]), NH.bits(grads[:t.n_net]))


# ------------------------------------------------------------------------------------------------ initial values
@pytest.mark.parametrize("kind,kw", [("cnn", dict(dueling=True)), ("mlp3", dict(dueling=True)), ("mlp2", dict(atoms=5))])
def test_initial_values_of_a_noisy_spec(kind, kw):
    spec, plain = _spec(kind, True, noisy_sigma0=0.4, **kw), _spec(kind, False, **kw)
    w, w_plain = initial_weights(spec, 11), initial_weights(plain, 11)
    noisy = {nl.name for nl in spec.noisy_layers}
    for name, (_, shape) in spec.names.items():
        layer, _, var = name.rpartition("/")
        assert w[name].shape == tuple(shape) and w[name].dtype == np.float32
        if layer not in noisy:                                # plain layers keep glorot / zero, from the same draws
            assert np.array_equal(w[name], w_plain[name])
            continue
        p = spec.names[layer + "/kernel"][1][0]
        if var.startswith("sigma"):
            assert (w[name] == np.float32(0.4 / np.sqrt(np.float64(p)))).all()
        else:
            assert np.abs(w[name]).max() <= np.float32(1.0 / np.sqrt(p))
            if w[name].size >= 16:                            # (U(-b, b) has standard deviation 0.577 b)
                assert w[name].std() > 0.3 / np.sqrt(p)
    a, b = CpuActorCritic(spec, seed=11), CpuActorCritic(spec, seed=11)
    assert np.array_equal(a.params, b.params) and not np.array_equal(a.params, CpuActorCritic(spec, seed=12).params)
    if kind == "mlp3":                                        # the padded fourth input row of both blocks: 0
        nl = spec.noisy_layers[0]
        assert nl.K == 4 and spec.names["dense/sigma_kernel"][1] == (3, 16)
        for off in (nl.w_off, nl.sigma_off):
            assert not a.params[off + 3 * nl.N:off + 4 * nl.N].any() and a.params[off:off + 3 * nl.N].all()


# ------------------------------------------------------------------------------------------------ the CPU replica
def test_cpu_replica_round_trips_sigma_and_predicts_with_fresh_noise_per_call():
    x = np.random.default_rng(0).standard_normal((6, 3)).astype(np.float32)
    m = model_builder(_info("DqnMlp", (3,), 2, dueling=True, SEED=4, noisy=True, HIDDEN_SIZE=16))
    w = m.get_weights()
    sig = [k for k in w if "sigma" in k]
    assert len(sig) == 6
    w2 = {k: (v + 1.0 if k in sig else v) for k, v in w.items()}
    m.set_weights(w2)
    assert all(np.array_equal(m.get_weights()[k], w2[k]) for k in w2)
    m.set_weights(w)
    q1, q2 = m.predict(x), m.predict(x)
    assert q1.shape == (6, 2) and q1.dtype == np.float32 and not np.array_equal(q1, q2)
    # the same seed and the same call counter: the same noise
    again = model_builder(_info("DqnMlp", (3,), 2, dueling=True, SEED=4, noisy=True, HIDDEN_SIZE=16))
    assert np.array_equal(again.predict(x), q1) and np.array_equal(again.predict(x), q2)
    # NOISY_PREDICT_MEAN: mu alone, call after call
    mean = model_builder(_info("DqnMlp", (3,), 2, dueling=True, SEED=4, noisy=True, HIDDEN_SIZE=16, NOISY_PREDICT_MEAN=True))
    qm = mean.predict(x)
    assert np.array_equal(mean.predict(x), qm) and not np.array_equal(qm, q1)
    # every sigma 0: a plain replica of the same means, to the bit
    plain = model_builder(_info("DqnMlp", (3,), 2, dueling=True, SEED=4, HIDDEN_SIZE=16))
    plain.set_weights({k: v for k, v in w.items() if k not in sig})
    assert np.array_equal(plain.predict(x), qm)
    m.set_weights({k: np.zeros_like(w[k]) for k in sig})
    assert np.array_equal(m.predict(x), qm)


@pytest.mark.parametrize("head", ["atoms", "quantiles"])
def test_cpu_replica_still_post_processes_distributional_heads(head):
    x = np.random.default_rng(1).standard_normal((5, 4)).astype(np.float32)
    m = model_builder(_info("DqnMlp", (4,), 3, SEED=2, noisy=True, HIDDEN_SIZE=16, NOISY_PREDICT_MEAN=True, **{head: 4}))
    assert m.net.spec.action_dim == 12 and m.net.spec.noisy_layers[1].N == 12
    q = m.predict(x)
    logits = m.net.forward(x)[0].reshape(5, 3, 4)
    want = D.dist_q(logits, m.support) if head == "atoms" else D.quant_q(logits)
    assert q.shape == (5, 3) and np.array_equal(q, want)


# ------------------------------------------------------------------------------------------------ refusals
def test_configuration_refusals_name_the_key_and_the_value():
    for bad in (0.0, -0.5, float("nan"), float("inf"), "x", None, True):
        with pytest.raises(ValueError, match="noisy_sigma0 = "):
            model_builder(_info("DqnMlp", (4,), 2, noisy=True, noisy_sigma0=bad))
    with pytest.raises(ValueError, match=re.escape("noisy_sigma0 = -0.5")):
        D.dqn_spec(_info("DqnCnn", (84, 84, 4), 2, noisy=True, noisy_sigma0=-0.5))
    for bad in (1, 0, "true", None, 1.0):
        with pytest.raises(ValueError, match=re.escape("noisy = {!r}".format(bad))):
            model_builder(_info("DqnMlp", (4,), 2, noisy=bad))
    # the earlier refusals are what they were
    with pytest.raises(NotImplementedError, match="DqnCnnPong is not supported"):
        D.dqn_spec(_info("DqnCnnPong", (84, 84, 4), 2, noisy=True))
    with pytest.raises(NotImplementedError, match="dueling with atoms = 5"):
        model_builder(_info("DqnMlp", (4,), 2, noisy=True, dueling=True, atoms=5))
    with pytest.raises(NotImplementedError, match="dueling with quantiles = 4"):
        model_builder(_info("DqnMlp", (4,), 2, noisy=True, dueling=True, quantiles=4))
    plain = CpuActorCritic(netspec.dqn_mlp((4,), 2, 8, 1))
    with pytest.raises(ValueError, match="no noisy layers"):
        plain.set_noisy(1, 0.5)


def test_c_entries_refuse_bad_tables_before_any_launch():
    """host checks only: the pointers are never dereferenced, no GPU is needed"""
    from xingtian_amd import lib as L
    handle, p, q = L.load(), ctypes.c_void_p(4096), ctypes.c_void_p(8192)
    t = NH.table(*NH.THREE)
    err = lambda: handle.xt_last_error().decode()

    def compose(layers=t.noisy_layers, n_layers=None, store=p, eff=q, n_net=t.n_net, noise=p, stream=0):
        return handle.xt_noisy_compose(NH.c_table(layers) if layers is not None else None,
                                       len(layers or ()) if n_layers is None else n_layers, store, eff, n_net, noise, None,
                                       1, 2, stream, 0, None)

    def grads(layers=t.noisy_layers, n_layers=None, noise=p, g=q):
        return handle.xt_noisy_grads(NH.c_table(layers) if layers is not None else None,
                                     len(layers or ()) if n_layers is None else n_layers, noise, g, None)

    def moved(i, **kw):
        out = []
        for j, nl in enumerate(t.noisy_layers):
            c = netspec.NoisyLayer()
            for s in netspec.NoisyLayer.__slots__:
                setattr(c, s, kw[s] if (j == i and s in kw) else getattr(nl, s))
            out.append(c)
        return out

    for kw in (dict(store=None), dict(eff=None), dict(noise=None), dict(layers=None, n_layers=1)):
        assert compose(**kw) != 0 and "null" in err(), kw
    assert compose(eff=p) != 0 and "two 16-byte aligned buffers" in err()
    assert compose(store=ctypes.c_void_p(4100)) != 0 and "16-byte aligned" in err()
    for n in (0, 9, -1):
        assert compose(n_layers=n) != 0 and "n_layers = %d outside [1, 8]" % n in err()
        assert grads(n_layers=n) != 0 and "n_layers = %d outside [1, 8]" % n in err()
    for n_net in (0, -4, t.n_net + 2):
        assert compose(n_net=n_net) != 0 and "n_net = %d" % n_net in err()
    last = t.noisy_layers[2]
    end = last.w_off + (last.K + 1) * last.N
    assert compose(n_net=NH.align4(end) - 4) != 0 and "leaves [0, %d)" % (NH.align4(end) - 4) in err() and str(end) in err()
    assert compose(layers=moved(0, sigma_off=t.n_net - 4)[:1]) != 0 and "in front of n_net = %d" % t.n_net in err()
    assert compose(layers=moved(1, w_off=t.noisy_layers[0].w_off + 4)) != 0 and "mean blocks of layers 0 and 1 overlap" in err()
    assert grads(layers=moved(1, w_off=t.noisy_layers[0].w_off + 4)) != 0 and "mean blocks of layers 0 and 1 overlap" in err()
    assert compose(layers=moved(1, sigma_off=t.noisy_layers[2].sigma_off + 8)) != 0 and "sigma blocks of layers" in err()
    assert compose(layers=moved(2, noise_off=t.noisy_layers[1].noise_off + 4)) != 0 and "noise vectors of layers 1 and 2" in err()
    assert compose(layers=moved(0, w_off=t.noisy_layers[0].w_off + 2)) != 0 and "multiples of 4" in err()
    assert compose(layers=moved(0, K=0)) != 0 and "K = 0" in err()
    assert compose(layers=moved(0, N=-3)) != 0 and "N = -3" in err()
    assert compose(layers=moved(0, K=70000, N=70000)) != 0 and "below 2^31" in err()
    assert compose(layers=moved(0, index=-1)) != 0 and "index = -1" in err()
    assert compose(stream=-1) != 0 and "stream_id = -1" in err()
    assert grads(noise=None) != 0 and grads(g=None) != 0 and grads(layers=None, n_layers=1) != 0
    assert grads(g=ctypes.c_void_p(8196)) != 0 and "16-byte aligned" in err()
    assert grads(layers=moved(2, sigma_off=8)) != 0 and "in front of the end of the mean blocks" in err()


# ------------------------------------------------------------------------------------------------ ABI
def test_abi_is_12_and_the_two_entries_are_bound_with_the_headers_signatures():
    from xingtian_amd import lib as L
    with open(os.path.join(ROOT, "include", "xt_mi355x.h")) as f:
        header = f.read()
    assert re.search(r"#define XT_ABI_VERSION 12\b", header) and L.ABI_VERSION == 12
    assert int(re.search(r"#define XT_NOISY_MAX_LAYERS (\d+)", header).group(1)) == L.NOISY_MAX_LAYERS == 8
    handle = L.load()
    for name in ("xt_noisy_compose", "xt_noisy_grads"):
        m = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert m, name
        args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
        res, sig = L.SIGNATURES[name]
        assert res is ctypes.c_int32 and len(sig) == len(args), (name, len(sig), len(args))
        for a, c in zip(args, sig):
            if "*" in a:
                assert c is (ctypes.POINTER(L.NoisyLayer) if "xt_noisy_layer" in a else ctypes.c_void_p), (name, a)
            else:
                want = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64}[a.split()[0]]
                assert c is want, (name, a)
        assert getattr(handle, name)
    assert list(L.SIGNATURES)[-2:] == ["xt_noisy_compose", "xt_noisy_grads"]       # appended
    assert ctypes.sizeof(L.NoisyLayer) == 40
    fields = re.search(r"typedef struct xt_noisy_layer \{(.*?)\} xt_noisy_layer;", header, re.S).group(1)
    assert re.findall(r"\b(\w+)[,;]", fields) == [f for f, _ in L.NoisyLayer._fields_]
