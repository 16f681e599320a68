"""CPU tests of the distributional (C51) DQN head's host side: the definitions ``dist_support`` / ``dist_q`` /
``categorical_projection`` against brute force, the spec and configuration surface with its refusals, the CPU replica's
``predict``, the head test's own case table (argmax stability, the float32 restatement's deviation) and the ABI."""
import ctypes
import os
import re

import numpy as np
import pytest

import dist_helpers as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _module_constants_restored():
    """import_config overrides the modules' constants for the rest of the process: put them back"""
    from xingtian_amd.algorithm.dqn import dqn
    from xingtian_amd.model.dqn import dqn_cnn, dqn_mlp
    saved = [(m, {k: v for k, v in vars(m).items() if k.isupper()}) for m in (dqn, dqn_cnn, dqn_mlp)]
    yield
    for m, consts in saved:
        vars(m).update(consts)


def _labels(rng, b, v_min, v_max):
    span = v_max - v_min
    return rng.standard_normal(b) * span / 3.0, 0.99 ** rng.integers(1, 4, b).astype(np.float64), rng.random(b) < 0.25


# ------------------------------------------------------------------------------------------------ the definitions
@pytest.mark.parametrize("n,v_min,v_max", [(2, -1.0, 1.0), (51, -10.0, 10.0), (64, 0.0, 200.0), (256, -3.5, 7.25)])
def test_categorical_projection_equals_the_papers_scatter_where_no_b_is_an_integer(n, v_min, v_max):
    from xingtian_amd.algorithm.dqn.dqn import categorical_projection
    rng = np.random.default_rng(n)
    b = 24
    p = rng.dirichlet(np.ones(n), b).astype(np.float32)
    reward, disc, done = _labels(rng, b, v_min, v_max)
    z, delta = D.support(n, v_min, v_max)
    # no b_j may be an integer, and a clamped one is: draw every reward where nothing clamps (v_min <= R + g z_j <= v_max for
    # all j, or v_min < R < v_max on a done row), again while some b_j comes within 1e-9 of an integer
    for s in range(b):
        lo, hi = (v_min, v_max) if done[s] else (v_min * (1.0 - disc[s]), v_max * (1.0 - disc[s]))
        for _ in range(100):
            reward[s] = rng.uniform(lo + 1e-6 * (hi - lo), hi - 1e-6 * (hi - lo))
            tz = np.full(n, reward[s]) if done[s] else reward[s] + disc[s] * z
            bj = (np.clip(tz, v_min, v_max) - v_min) / delta
            if np.abs(bj - np.rint(bj)).min() > 1e-9:
                break
        else:
            raise AssertionError("no reward without an integer b_j")
    sums = np.zeros((b, n), np.float64)
    idx = np.arange(n, dtype=np.float64)
    for s in range(b):                                      # the gather form before its one rounding, for the 1e-12 bar
        tz = np.full(n, reward[s]) if done[s] else reward[s] + disc[s] * z
        bj = (np.clip(tz, v_min, v_max) - v_min) / delta
        for j in range(n):
            sums[s] += np.float64(p[s, j]) * np.maximum(0.0, 1.0 - np.abs(bj[j] - idx))
    want = D.scatter_projection(p, reward, disc, done, v_min, v_max)
    assert np.abs(sums - want).max() <= 1e-12
    got = categorical_projection(p, reward, disc, done, v_min, v_max)
    assert got.dtype == np.float32 and np.array_equal(got, sums.astype(np.float32))        # one rounding of that sum
    assert np.abs(got.sum(1, dtype=np.float64) - p.sum(1, dtype=np.float64)).max() <= n * 2.0 ** -25


def _projection_sum64(p, reward, disc, done, v_min, v_max):
    """categorical_projection before its rounding (the mass bar of 1e-12 is about the arithmetic, not the float32 store)"""
    n = p.shape[1]
    z, delta = D.support(n, v_min, v_max)
    idx = np.arange(n, dtype=np.float64)
    out = np.zeros(p.shape, np.float64)
    for s in range(p.shape[0]):
        tz = np.full(n, float(reward[s])) if done[s] else float(reward[s]) + float(disc[s]) * z
        bj = (np.clip(tz, v_min, v_max) - v_min) / delta
        for j in range(n):
            out[s] += np.float64(p[s, j]) * np.maximum(0.0, 1.0 - np.abs(bj[j] - idx))
    return out


@pytest.mark.parametrize("n,v_min,v_max", [(2, -0.25, 0.25), (51, -12.5, 12.5), (51, -10.0, 10.0), (256, -63.75, 63.75)])
def test_projection_conserves_mass_on_random_integer_clamped_done_and_gamma_zero_rows(n, v_min, v_max):
    from xingtian_amd.algorithm.dqn.dqn import categorical_projection
    rng = np.random.default_rng(7 * n)
    p = rng.dirichlet(np.ones(n), 12).astype(np.float32)
    span = v_max - v_min
    reward, disc, done = _labels(rng, 12, v_min, v_max)
    reward[:6] = [0.0, 10 * span, -10 * span, 0.3 * span, 0.1, -0.2 * span]
    disc[:6] = [1.0, 0.99, 0.99, 0.99, 0.0, 0.0]
    done[:6] = [False, False, False, True, False, False]
    mass = p.astype(np.float64).sum(1)
    s64 = _projection_sum64(p, reward, disc, done, v_min, v_max)
    assert np.abs(s64.sum(1) - mass).max() <= 1e-12
    m = categorical_projection(p, reward, disc, done, v_min, v_max)
    assert np.array_equal(m, s64.astype(np.float32))
    exact = (v_max - v_min) / (n - 1) == 0.5
    if exact:                                               # gamma = 1, R = 0: every b_j is an integer, m == p exactly
        assert np.array_equal(m[0], p[0])
    else:
        assert np.abs(m[0] - p[0]).max() <= 1e-6
    assert m[1, -1] == np.float32(mass[1]) and not m[1, :-1].any()            # all mass on the last atom
    assert m[2, 0] == np.float32(mass[2]) and not m[2, 1:].any()              # ... on the first
    assert np.count_nonzero(m[3]) <= 2 and np.count_nonzero(m[4]) <= 2        # done / gamma = 0: one point, two atoms


def test_dist_support_and_dist_q_against_float64():
    from xingtian_amd.algorithm.dqn.dqn import dist_q, dist_support
    z, delta = dist_support(51, -10.0, 10.0)
    assert z.dtype == np.float64 and delta == 20.0 / 50.0 and z[0] == -10.0 and np.array_equal(z, -10.0 + np.arange(51) * delta)
    rng = np.random.default_rng(3)
    l = (rng.standard_normal((9, 4, 51)) * 3).astype(np.float32)
    q = dist_q(l, z)
    assert q.dtype == np.float32 and q.shape == (9, 4)
    e = np.exp(l.astype(np.float64) - l.astype(np.float64).max(-1, keepdims=True))
    want = (z * e).sum(-1) / e.sum(-1)
    assert np.abs(q - want).max() <= 64 * 2.0 ** -24 * 10.0                   # 51 float32 products of magnitude <= 10
    for bad in ((1, -1.0, 1.0), (51, 1.0, 1.0), (51, 2.0, 1.0), (51, float("-inf"), 1.0), (51, 0.0, float("nan"))):
        with pytest.raises(ValueError, match="dist_support"):
            dist_support(*bad)


# ------------------------------------------------------------------------------------------------ spec and configuration
def test_atoms_absent_or_one_is_todays_spec_and_51_widens_the_q_head_only():
    from xingtian_amd.model import netspec
    for make, args, feat in ((netspec.dqn_cnn, ((84, 84, 4), 4), 256), (netspec.dqn_mlp, ((4,), 3, 32, 2), 32)):
        for dueling in (False, True):
            base, one = make(*args, dueling=dueling), make(*args, dueling=dueling, atoms=1)
            assert list(base.names.items()) == list(one.names.items()) and base.n_flat == one.n_flat
            assert (base.pi_off, base.v_off, base.action_dim, base.hidden_v) == (one.pi_off, one.v_off, one.action_dim, one.hidden_v)
        a = args[1]
        dist = make(*args, atoms=51)
        head = [k for k in dist.names if k not in [l.name + s for l in dist.layers for s in ("/kernel", "/bias")]]
        assert head == [base.pi_name + "/kernel", base.pi_name + "/bias"] and dist.hidden_v         # no named 1-wide stream
        assert dist.names[base.pi_name + "/kernel"][1] == (feat, a * 51) and dist.names[base.pi_name + "/bias"][1] == (a * 51,)
        assert (dist.action_dim, dist.n_actions, dist.atoms) == (a * 51, a, 51) and dist.pi_off == base.pi_off
        assert dist.v_off == (dist.pi_off + feat * a * 51 + a * 51 + 3) & ~3
        with pytest.raises(NotImplementedError, match="dueling stream is 1 wide.*atoms-wide"):
            make(*args, dueling=True, atoms=51)
        for bad in (0, 257, -3, 2.5, True):
            with pytest.raises(ValueError, match="atoms"):
                make(*args, atoms=bad)


def _info(name="DqnMlp", a=3, **mc):
    cfg = dict(HIDDEN_SIZE=32, NUM_LAYERS=1, SEED=5)
    cfg.update(mc)
    return {"model_name": name, "state_dim": [84, 84, 4] if name == "DqnCnn" else [4], "action_dim": a, "model_config": cfg}


def test_model_config_refusals_name_their_reason():
    from xingtian_amd.model import model_builder
    from xingtian_amd.model.dqn.dqn_cnn import dqn_spec
    for name in ("DqnMlp", "DqnCnn"):
        with pytest.raises(NotImplementedError, match="dueling stream is 1 wide.*needs an atoms-wide one"):
            model_builder(_info(name, atoms=51, dueling=True))
        for bad in (0, 257, 1.5):
            with pytest.raises(ValueError, match="atoms = .* must be an integer in \\[1, 256\\]"):
                model_builder(_info(name, atoms=bad))
        for lo, hi in ((1.0, 1.0), (2.0, -2.0), (float("nan"), 1.0), (0.0, float("inf"))):
            with pytest.raises(ValueError, match="finite v_min < v_max"):
                model_builder(_info(name, atoms=51, v_min=lo, v_max=hi))
        with pytest.raises(ValueError, match="action_dim = 65 exceeds 64"):
            model_builder(_info(name, a=65, atoms=2))
    assert dqn_spec(_info(atoms=51)).action_dim == 3 * 51 and dqn_spec(_info("DqnCnn", atoms=51)).action_dim == 3 * 51
    # the bounds are not looked at without atoms
    plain = model_builder(_info(v_min=3.0, v_max=-3.0))
    assert plain.atoms == 1 and plain.support is None and plain.net.spec.action_dim == 3


def test_cpu_replica_predict_is_dist_q_of_its_own_logits():
    from xingtian_amd.algorithm.dqn.dqn import dist_q, dist_support
    from xingtian_amd.model import model_builder
    model = model_builder(_info(atoms=51, v_min=-5.0, v_max=15.0))
    assert model.net.inference_only and (model.atoms, model.v_min, model.v_max) == (51, -5.0, 15.0)
    assert sorted(model.get_weights()) == ["dense/bias", "dense/kernel", "dense_1/bias", "dense_1/kernel"]
    assert model.get_weights()["dense_1/kernel"].shape == (32, 3 * 51)
    rng = np.random.default_rng(0)
    w = {k: (rng.standard_normal(v.shape) * 0.5).astype(np.float32) for k, v in model.get_weights().items()}
    model.set_weights(w)
    x = rng.standard_normal((9, 4)).astype(np.float32)
    q = model.predict(x)
    logits = np.asarray(model.net.forward(x)[0])
    assert q.shape == (9, 3) and q.dtype == np.float32 and logits.shape == (9, 3 * 51)
    assert np.array_equal(q, dist_q(logits.reshape(9, 3, 51), dist_support(51, -5.0, 15.0)[0]))
    h = np.maximum(x.astype(np.float64) @ w["dense/kernel"] + w["dense/bias"], 0.0)
    l64 = (h @ w["dense_1/kernel"] + w["dense_1/bias"]).reshape(9, 3, 51)
    e = np.exp(l64 - l64.max(-1, keepdims=True))
    want = (dist_support(51, -5.0, 15.0)[0] * e).sum(-1) / e.sum(-1)
    assert np.abs(q - want).max() <= 1e-4
    assert np.all(q >= -5.0) and np.all(q <= 15.0)
    # the scalar model of the same YAML without atoms keeps its [N, A] head
    assert model_builder(_info()).predict(x).shape == (9, 3)


def test_dqn_refuses_a_distributional_actor_without_the_device_step():
    from xingtian_amd.algorithm import alg_builder
    cfg = {"instance_num": 1, "agent_num": 1, "prepare_times_per_train": 1, "BUFFER_SIZE": 50, "BATCH_SIZE": 8}
    with pytest.raises(NotImplementedError, match="distributional actor \\(atoms = 51\\) needs a model with the device step.*DqnMlp"):
        alg_builder("DQN", {"actor": _info(atoms=51)}, cfg)
    alg = alg_builder("DQN", {"actor": _info()}, cfg)                          # the replica without atoms is still accepted
    assert alg.atoms == 1 and not alg.device_step


# ------------------------------------------------------------------------------------------------ the head test's table
def test_head_cases_keep_the_argmax_stable_and_hold_every_planted_row():
    seen = set()
    for shape in D.HEAD_SHAPES:
        for v in D.HEAD_VARIANTS:
            c = D.head_case(shape, *v)
            ref = D.head_ref(c)
            gap = D.argmax_gap(ref, c["planted"], c["v_max"] - c["v_min"])
            assert gap >= 1e-4, (shape, v, gap)
            seen.update(c["planted"])
            pl = c["planted"]
            if "tie" in pl and c["a"] > 1:
                assert ref["astar"][pl["tie"]] == 0 and np.ptp(ref["q_pick"][pl["tie"]]) == 0.0
            if "integer" in pl and v[2]:
                assert np.array_equal(ref["m"][pl["integer"]], ref["p"][pl["integer"]])
            if "clamp_hi" in pl:
                assert ref["m"][pl["clamp_hi"], -1] > 0.999999 and ref["m"][pl["clamp_lo"] if "clamp_lo" in pl else 0, 0] >= 0.0
    assert seen == set(D.PLANTED)


def test_head_bars_are_four_times_the_float32_restatements_deviation_and_below_the_gradient_bar():
    measured, bars = D.head_bars()
    print("dist head: float32 NumPy restatement vs float64 (rel_max)", measured, "-> bars", bars)
    for k in D.HEAD_QUANTITIES:
        assert 0.0 < measured[k] < 1e-5 and bars[k] == (min(4.0 * measured[k], 1e-5) if k == "dlogits" else 4.0 * measured[k])
    assert 4.0 * measured["dlogits"] <= 1e-5                # (a bar above the project's gradient bar would be a finding)


# ------------------------------------------------------------------------------------------------ ABI
def test_abi_header_signatures_and_exported_symbols_agree_for_the_dist_entries():
    from xingtian_amd import lib as L
    with open(os.path.join(ROOT, "include", "xt_mi355x.h")) as f:
        header = f.read()
    assert re.search(r"#define XT_ABI_VERSION 12\b", header) and L.ABI_VERSION == 12
    handle = L.load()
    assert handle.xt_abi_version() == 12
    structs = {"xt_dqn_cfg": L.DqnCfg, "xt_per_cfg": L.PerCfg, "xt_nstep_cfg": L.NstepCfg}
    for name in ("xt_dqn_loss_dist", "xt_net_set_dist", "xt_net_set_dist_wide", "xt_net_dqn_step_dist"):
        m = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert m, name
        args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
        res, sig = L.SIGNATURES[name]
        assert res is ctypes.c_int32 and len(sig) == len(args), (name, len(sig), len(args))
        for a, c in zip(args, sig):
            if "*" in a:                                  # every pointer is a void* or a typed struct pointer
                st = [s for s in structs if s in a]
                assert c is (ctypes.POINTER(structs[st[0]]) if st else ctypes.c_void_p), (name, a)
            else:
                want = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "double": ctypes.c_double}[a.split()[0]]
                assert c is want, (name, a)
        assert getattr(handle, name)
    assert len(L.SIGNATURES["xt_dqn_loss_dist"][1]) == 23 and len(L.SIGNATURES["xt_net_dqn_step_dist"][1]) == 18
    # no existing struct changed layout
    assert ctypes.sizeof(L.DqnCfg) == 40 and ctypes.sizeof(L.PerCfg) == 88 and ctypes.sizeof(L.NstepCfg) == 56
    # host refusals of the new entries: nothing is launched, no GPU is needed
    p = ctypes.c_void_p(64)
    call = lambda a, n, lo, hi: handle.xt_dqn_loss_dist(p, p, None, 4, a, n, lo, hi, None, p, p, p, 0.99, p, p, p, None, None,
                                                        None, None, None, None, None)
    for a, n, lo, hi in ((2, 1, -1.0, 1.0), (2, 257, -1.0, 1.0), (0, 51, -1.0, 1.0), (65, 51, -1.0, 1.0), (2, 51, 1.0, 1.0),
                         (2, 51, float("nan"), 1.0), (2, 51, 0.0, float("inf"))):
        assert call(a, n, lo, hi) != 0, (a, n, lo, hi)
    assert handle.xt_dqn_loss_dist(p, p, None, 4, 2, 51, -1.0, 1.0, None, p, p, p, 0.99, p, p, ctypes.c_void_p(68), None, None,
                                   None, None, None, None, None) != 0                       # out not 8-byte aligned
    assert handle.xt_dqn_loss_dist(None, p, None, 4, 2, 51, -1.0, 1.0, None, p, p, p, 0.99, p, p, p, None, None, None, None,
                                   None, None, None) != 0
    assert handle.xt_net_set_dist(None, 51, -10.0, 10.0) != 0 and handle.xt_net_set_dist_wide(None, 1) != 0
    assert handle.xt_net_dqn_step_dist(None, None, None, None, None, None, None, 16, 1, 0, None, 1, None, None, None, None, None,
                                       None) != 0
