"""CPU tests of the quantile-regression (QR-DQN) head's host side: the definitions ``quantile_midpoints`` / ``quant_q`` /
``quantile_huber`` against the float64 restatement and a finite difference, the spec and configuration surface with its
refusals, the CPU replica's ``predict``, the GPU tests' own case tables (argmax stability, planted rows, the float32
restatement's deviation, the eligible ring rows) and the ABI."""
import ctypes
import os
import re

import numpy as np
import pytest

import dqn_helpers as H
import quant_helpers as Q

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


# ------------------------------------------------------------------------------------------------ the definitions
def _loss64(theta, target, kappa):
    """sum_i (1 / N) sum_j |tau_i - [u_ij < 0]| H(u_ij) / kappa per sample in plain float64, written from the paper"""
    n = theta.shape[1]
    tau = (np.arange(n) + 0.5) / n
    u = target[:, None, :] - theta[:, :, None]
    hub = np.where(np.abs(u) <= kappa, 0.5 * u * u, kappa * (np.abs(u) - 0.5 * kappa))
    return (np.abs(tau[None, :, None] - (u < 0)) * hub / kappa).sum(axis=(1, 2)) / n


def test_midpoints_and_quant_q_against_float64():
    from xingtian_amd.algorithm.dqn.dqn import quant_q, quantile_midpoints
    for n in (1, 2, 51, 256):
        tau = quantile_midpoints(n)
        assert tau.dtype == np.float64 and np.array_equal(tau, (2.0 * np.arange(n) + 1.0) / (2.0 * n))
        assert np.array_equal(tau, Q.midpoints(n)) and abs(tau.mean() - 0.5) <= 1e-15
    with pytest.raises(ValueError, match="quantile_midpoints"):
        quantile_midpoints(0)
    rng = np.random.default_rng(3)
    th = (rng.standard_normal((9, 4, 51)) * 3).astype(np.float32)
    q = quant_q(th)
    assert q.dtype == np.float32 and q.shape == (9, 4)
    assert np.array_equal(q, Q.mean_q(th, np.float32))
    want = th.astype(np.float64).mean(-1)
    assert np.abs(q - want).max() <= 2.0 ** -24 * np.abs(want).max()                   # one rounding of the float64 mean
    assert quant_q(np.float32([[1.0, 2.0]])).tolist() == [1.5]


@pytest.mark.parametrize("shape", Q.HEAD_SHAPES, ids=["B%d_A%d_N%d" % s for s in Q.HEAD_SHAPES])
def test_quantile_huber_is_the_float32_restatement_and_within_the_bars_of_float64(shape):
    from xingtian_amd.algorithm.dqn.dqn import quantile_huber
    b, a, n = shape
    _, bars = Q.head_bars()
    for v in ((False, False, False, False), (True, True, True, False)):
        c = Q.head_case(shape, *v)
        r64, r32 = Q.head_ref(c), Q.head_ref(c, np.float32)
        rows = np.arange(b)
        theta = c["logits"].reshape(b, a, n)[rows, r64["act"]]
        target_theta = c["t_logits"].reshape(b, a, n)[rows, r64["astar"]]
        disc = c["disc"] if c["disc"] is not None else c["gamma"]
        loss_b, g = quantile_huber(theta, target_theta, c["reward"], disc, c["done"], c["kappa"])
        assert loss_b.dtype == np.float32 and g.dtype == np.float32 and g.shape == (b, n)
        assert np.array_equal(loss_b, r32["loss_b"]) and np.array_equal(g, r32["g"])
        assert H.rel_max(loss_b, r64["loss_b"]) <= bars["loss_b"] and H.rel_max(g, r64["g"]) <= bars["dlogits"]
        # the restatement against the paper's formula in plain float64 (T_j alone keeps its float32 rounding)
        want = _loss64(theta.astype(np.float64), r64["target"], c["kappa"])
        assert np.abs(r64["loss_b"] - want).max() <= 1e-13 * max(1.0, np.abs(want).max())
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="kappa must be finite and > 0"):
            quantile_huber(theta, target_theta, c["reward"], disc, c["done"], bad)


@pytest.mark.parametrize("n,kappa", [(2, 1.0), (8, 0.5), (51, 1.0), (65, 2.0)])
def test_quantile_huber_gradient_against_a_central_difference_of_the_float64_loss(n, kappa):
    """The loss is C1 in theta with |d2 loss / d theta_i^2| <= 1 / kappa (piecewise quadratic), so a central difference of
    step h is within h / kappa of the derivative; the twin's own float32 rounding adds the gradient bar of the head test
    times the largest |g| (<= 1)."""
    from xingtian_amd.algorithm.dqn.dqn import quantile_huber
    rng = np.random.default_rng(n)
    b, h = 6, 1e-6
    theta = (rng.standard_normal((b, n)) * 1.5).astype(np.float32)
    target_theta = (rng.standard_normal((b, n)) * 1.5).astype(np.float32)
    reward, disc, done = rng.standard_normal(b), 0.99 ** rng.integers(1, 4, b).astype(np.float64), rng.random(b) < 0.3
    reward[2] = 0.75
    theta[1, 0] = np.float32(reward[1])                       # with done: u exactly 0 ...
    theta[2, 0] = np.float32(0.75 - kappa)                    # ... and exactly kappa (all three exact in float32)
    done[1] = done[2] = True
    loss_b, g = quantile_huber(theta, target_theta, reward, disc, done, kappa)
    target = np.where(done[:, None], reward[:, None], reward[:, None] + disc[:, None] * target_theta.astype(np.float64))
    target = target.astype(np.float32).astype(np.float64)
    th64 = theta.astype(np.float64)
    assert (target[1] - th64[1, 0] == 0).all() and (np.abs(target[2] - th64[2, 0]) == kappa).all()
    assert np.abs(loss_b - _loss64(th64, target, kappa)).max() <= 1e-5 * max(1.0, loss_b.max())
    fd = np.zeros((b, n))
    for i in range(n):
        e = np.zeros((1, n))
        e[0, i] = h
        fd[:, i] = (_loss64(th64 + e, target, kappa) - _loss64(th64 - e, target, kappa)) / (2 * h)
    assert np.abs(g).max() <= 1.0
    assert np.abs(g - fd).max() <= h / kappa + Q.head_bars()[1]["dlogits"] + 1e-9, np.abs(g - fd).max()
    # the gradients of one sample sum to -(mean over i, j of the clipped, weighted u): a quantile that sits above every
    # target is pulled down with weight 1 - tau_i
    hi = np.full((1, n), 100.0, np.float32)
    _, g_hi = quantile_huber(hi, np.zeros((1, n), np.float32), [0.0], 1.0, [True], kappa)
    assert np.allclose(g_hi[0], 1.0 - Q.midpoints(n), rtol=0, atol=1e-6)


# ------------------------------------------------------------------------------------------------ spec and configuration
def test_quantiles_absent_or_one_is_todays_spec_and_51_widens_the_q_head_only():
    from xingtian_amd.model import netspec
    for make, args, feat in ((netspec.dqn_cnn, ((84, 84, 4), 4), 256), (netspec.dqn_mlp, ((4,), 3, 32, 2), 32)):
        for dueling in (False, True):
            base, one = make(*args, dueling=dueling), make(*args, dueling=dueling, quantiles=1)
            assert list(base.names.items()) == list(one.names.items()) and base.n_flat == one.n_flat
            assert (base.pi_off, base.v_off, base.action_dim, base.hidden_v) == (one.pi_off, one.v_off, one.action_dim, one.hidden_v)
            assert (one.atoms, one.quantiles) == (1, 1)
        a = args[1]
        quant, dist = make(*args, quantiles=51), make(*args, atoms=51)
        assert list(quant.names.items()) == list(dist.names.items()) and quant.n_flat == dist.n_flat     # the same width rule
        assert quant.names[base.pi_name + "/kernel"][1] == (feat, a * 51) and quant.names[base.pi_name + "/bias"][1] == (a * 51,)
        assert (quant.action_dim, quant.n_actions, quant.quantiles, quant.atoms) == (a * 51, a, 51, 1) and quant.hidden_v
        assert (dist.atoms, dist.quantiles) == (51, 1)
        assert quant.v_off == (quant.pi_off + feat * a * 51 + a * 51 + 3) & ~3
        with pytest.raises(NotImplementedError, match="dueling stream is 1 wide.*quantiles-wide"):
            make(*args, dueling=True, quantiles=51)
        with pytest.raises(ValueError, match="atoms = 51 together with quantiles = 8"):
            make(*args, atoms=51, quantiles=8)
        for bad in (0, 257, -3, 2.5, True):
            with pytest.raises(ValueError, match="quantiles"):
                make(*args, quantiles=bad)


def _info(name="DqnMlp", a=3, **mc):
    cfg = dict(HIDDEN_SIZE=32, NUM_LAYERS=1, SEED=5)
    cfg.update(mc)
    return {"model_name": name, "state_dim": [84, 84, 4] if name == "DqnCnn" else [4], "action_dim": a, "model_config": cfg}


def test_model_config_refusals_name_their_reason():
    from xingtian_amd.model import model_builder
    from xingtian_amd.model.dqn.dqn_cnn import dqn_spec, quant_config
    assert quant_config({}, 4) == (1, 1.0) and quant_config({"quantiles": 8}, 4) == (8, 1.0)
    assert quant_config({"quantiles": 200, "kappa": 0.25}, 64) == (200, 0.25)
    for name in ("DqnMlp", "DqnCnn"):
        with pytest.raises(NotImplementedError, match="dueling stream is 1 wide.*needs a quantiles-wide one"):
            model_builder(_info(name, quantiles=51, dueling=True))
        with pytest.raises(ValueError, match="quantiles = 8 together with atoms = 51"):
            model_builder(_info(name, quantiles=8, atoms=51))
        for bad in (0, 257, 1.5):
            with pytest.raises(ValueError, match="quantiles = .* must be an integer in \\[1, 256\\]"):
                model_builder(_info(name, quantiles=bad))
        for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-60):
            with pytest.raises(ValueError, match="kappa must be finite and > 0"):
                model_builder(_info(name, quantiles=51, kappa=bad))
        with pytest.raises(ValueError, match="action_dim = 65 exceeds 64"):
            model_builder(_info(name, a=65, quantiles=2))
    assert dqn_spec(_info(quantiles=51)).action_dim == 3 * 51 and dqn_spec(_info("DqnCnn", quantiles=51)).action_dim == 3 * 51
    # kappa is not looked at without quantiles, and atoms alone is the C51 model it was
    plain = model_builder(_info(kappa=-3.0))
    assert plain.quantiles == 1 and plain.atoms == 1 and plain.net.spec.action_dim == 3
    c51 = model_builder(_info(atoms=51))
    assert (c51.atoms, c51.quantiles) == (51, 1)


def test_cpu_replica_predict_is_quant_q_of_its_own_logits():
    from xingtian_amd.algorithm.dqn.dqn import quant_q
    from xingtian_amd.model import model_builder
    model = model_builder(_info(quantiles=8, kappa=0.5))
    assert model.net.inference_only and (model.quantiles, model.kappa, model.atoms) == (8, 0.5, 1)
    assert model.get_weights()["dense_1/kernel"].shape == (32, 3 * 8)
    rng = np.random.default_rng(0)
    w = {k: (rng.standard_normal(v.shape) * 0.5).astype(np.float32) for k, v in model.get_weights().items()}
    model.set_weights(w)
    x = rng.standard_normal((9, 4)).astype(np.float32)
    q = model.predict(x)
    logits = np.asarray(model.net.forward(x)[0])
    assert q.shape == (9, 3) and q.dtype == np.float32 and logits.shape == (9, 3 * 8)
    assert np.array_equal(q, quant_q(logits.reshape(9, 3, 8)))
    h = np.maximum(x.astype(np.float64) @ w["dense/kernel"] + w["dense/bias"], 0.0)
    want = (h @ w["dense_1/kernel"] + w["dense_1/bias"]).reshape(9, 3, 8).mean(-1)
    assert np.abs(q - want).max() <= 1e-4 * max(1.0, np.abs(want).max())
    assert model_builder(_info()).predict(x).shape == (9, 3)


def test_dqn_refuses_a_quantile_actor_without_the_device_step():
    from xingtian_amd.algorithm import alg_builder
    cfg = {"instance_num": 1, "agent_num": 1, "prepare_times_per_train": 1, "BUFFER_SIZE": 50, "BATCH_SIZE": 8}
    with pytest.raises(NotImplementedError, match="quantile actor \\(quantiles = 8\\) needs a model with the device step.*DqnMlp"):
        alg_builder("DQN", {"actor": _info(quantiles=8)}, cfg)
    alg = alg_builder("DQN", {"actor": _info()}, cfg)
    assert alg.quantiles == 1 and alg.atoms == 1 and not alg.device_step


# ------------------------------------------------------------------------------------------------ the GPU tests' tables
def test_head_cases_keep_the_argmax_stable_and_hold_every_planted_row():
    assert len(Q.HEAD_SHAPES) * len(Q.HEAD_VARIANTS) == 112 and Q.KAPPA == 1.0
    seen = set()
    for shape in Q.HEAD_SHAPES:
        b, a, n = shape
        for v in Q.HEAD_VARIANTS:
            c = Q.head_case(shape, *v)
            ref, r32 = Q.head_ref(c), Q.head_ref(c, np.float32)
            gap = Q.argmax_gap(ref, c["planted"])
            assert gap >= Q.ARGMAX_GAP, (shape, v, gap)
            assert np.array_equal(ref["astar"], r32["astar"])
            pl = c["planted"]
            assert len(pl) == min(b - 1, len(Q.PLANTED))
            seen.update(pl)
            # the sign of every u_ij is the same in both dtypes (T_j is the same float32 number in both)
            for row in range(min(b, 6)):
                u64 = Q.u_matrix(c, ref, row)
                th32 = c["logits"].reshape(b, a, n)[row, ref["act"][row]]
                u32 = r32["target"][row][None, :] - th32[:, None]
                assert u32.dtype == np.float32 and np.array_equal(np.sign(u32), np.sign(u64))
            if "done" in pl:
                assert c["done"][pl["done"]] == 1 and c["action"][pl["done"]] == -1 and ref["act"][pl["done"]] == 0
            if "clamp" in pl:
                assert c["action"][pl["clamp"]] == a and ref["act"][pl["clamp"]] == a - 1
            if "zero" in pl:
                u = Q.u_matrix(c, ref, pl["zero"])
                assert (u[n // 2] == 0).all() and c["done"][pl["zero"]] == 1
            if "kappa" in pl:
                u = Q.u_matrix(c, ref, pl["kappa"])
                assert (np.abs(u) == Q.KAPPA).any() and (u * 2 == np.rint(u * 2)).all()       # all of u on the 0.5 grid
            if "tie" in pl and a > 1:
                assert ref["astar"][pl["tie"]] == 0 and np.ptp(ref["q_pick"][pl["tie"]]) == 0.0
    assert seen == set(Q.PLANTED)


def test_head_bars_are_four_times_the_float32_restatements_deviation_and_below_the_gradient_bar():
    measured, bars = Q.head_bars()
    print("quant head: float32 NumPy restatement vs float64 (rel_max)", measured, "-> bars", bars)
    assert set(bars) == set(Q.HEAD_QUANTITIES) == {"loss_b", "dlogits", "qstar", "out"}
    for k in Q.HEAD_QUANTITIES:
        assert 0.0 < measured[k] < 1e-5 and bars[k] == (min(4.0 * measured[k], 1e-5) if k == "dlogits" else 4.0 * measured[k])
    assert 4.0 * measured["dlogits"] <= 1e-5                # (a bar above the project's gradient bar would be a finding)


def test_the_ring_leaves_a_minibatch_of_eligible_rows_in_every_whole_step_case():
    """rows whose state keeps 1e-6 from the ReLU kink and whose bootstrap row keeps twice the argmax gap, counted on the
    float64 oracle alone"""
    assert [(k, a, n) for k, a, n, _ in Q.STEP_CASES].count(("mlp", 2, 8)) == 5 and len(Q.STEP_CASES) == 12
    for case in Q.STEP_CASES:
        s = Q.step_setup(*case)
        assert len(s["ok"]) >= Q.BATCH == 32, (case, len(s["ok"]))
        assert s["spec"].action_dim == case[1] * case[2] and s["spec"].quantiles == case[2]


# ------------------------------------------------------------------------------------------------ ABI
def test_abi_header_signatures_and_exported_symbols_agree_for_the_quant_entries():
    from xingtian_amd import lib as L
    with open(os.path.join(ROOT, "include", "xt_mi355x.h")) as f:
        header = f.read()
    assert re.search(r"#define XT_ABI_VERSION 12\b", header) and L.ABI_VERSION == 12
    handle = L.load()
    structs = {"xt_dqn_cfg": L.DqnCfg, "xt_per_cfg": L.PerCfg, "xt_nstep_cfg": L.NstepCfg}
    for name in ("xt_dqn_loss_quant", "xt_net_set_quant", "xt_net_dqn_step_quant"):
        m = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert m, name
        args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
        res, sig = L.SIGNATURES[name]
        assert res is ctypes.c_int32 and len(sig) == len(args), (name, len(sig), len(args))
        for a, c in zip(args, sig):
            if "*" in a:
                st = [s for s in structs if s in a]
                assert c is (ctypes.POINTER(structs[st[0]]) if st else ctypes.c_void_p), (name, a)
            else:
                want = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "double": ctypes.c_double}[a.split()[0]]
                assert c is want, (name, a)
        assert getattr(handle, name)
    assert len(L.SIGNATURES["xt_dqn_loss_quant"][1]) == 21
    assert L.SIGNATURES["xt_net_dqn_step_quant"] == L.SIGNATURES["xt_net_dqn_step_dist"]
    assert ctypes.sizeof(L.DqnCfg) == 40 and ctypes.sizeof(L.PerCfg) == 88 and ctypes.sizeof(L.NstepCfg) == 56
    # host refusals of the new entries: nothing is launched, no GPU is needed
    p = ctypes.c_void_p(64)
    call = lambda a, n, kappa, out=p, logits=p: handle.xt_dqn_loss_quant(
        logits, p, None, 4, a, n, kappa, None, p, p, p, 0.99, p, p, out, None, None, None, None, None, None)
    for a, n, kappa in ((2, 1, 1.0), (2, 257, 1.0), (2, 0, 1.0), (0, 51, 1.0), (65, 51, 1.0), (2, 51, 0.0), (2, 51, -1.0),
                        (2, 51, float("nan")), (2, 51, float("inf")), (2, 51, 1e-60)):
        assert call(a, n, kappa) != 0, (a, n, kappa)
    assert call(2, 51, 1.0, out=ctypes.c_void_p(68)) != 0                                    # out not 8-byte aligned
    assert call(2, 51, 1.0, logits=None) != 0
    assert handle.xt_net_set_quant(None, 51, 1.0) != 0
    assert handle.xt_net_dqn_step_quant(None, None, None, None, None, None, None, 16, 1, 0, None, 1, None, None, None, None, None,
                                        None) != 0
