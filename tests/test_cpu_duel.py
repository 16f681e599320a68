"""CPU tests of the dueling distributional heads' host side (``model_config.dist_dueling``): the folded spec layout and what
stays as it was without the key, every refusal (the pinned ones of ``dueling`` with ``atoms`` / ``quantiles`` included), the
CPU replica's ``predict`` against float64, the combine's gradient twin against central differences, the head tests' own case
tables (argmax stability, the float32 restatement's deviation and the bars that follow from it) and the ABI."""
import ctypes
import os
import re

import numpy as np
import pytest

import duel_helpers as U

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


def _info(name="DqnMlp", a=3, **mc):
    cfg = dict(HIDDEN_SIZE=32, NUM_LAYERS=1, SEED=5)
    cfg.update(mc)
    return {"model_name": name, "state_dim": [84, 84, 4] if name == "DqnCnn" else [4], "action_dim": a, "model_config": cfg}


MAKERS = [("cnn", ((84, 84, 4), 4), 256), ("mlp", ((4,), 3, 32, 2), 32)]


def _make(kind):
    from xingtian_amd.model import netspec
    return netspec.dqn_cnn if kind == "cnn" else netspec.dqn_mlp


# ------------------------------------------------------------------------------------------------ spec layout
@pytest.mark.parametrize("kind,args,feat", MAKERS, ids=[m[0] for m in MAKERS])
@pytest.mark.parametrize("head", U.HEADS)
def test_spec_without_the_key_is_todays_and_with_it_the_q_head_holds_one_more_group(kind, args, feat, head):
    make, a = _make(kind), args[1]
    kw = dict(atoms=51) if head == "c51" else dict(quantiles=51)
    for other in (dict(), dict(dueling=True), kw, dict(noisy=True), dict(noisy=True, **kw)):
        base, off = make(*args, **other), make(*args, dist_dueling=False, **other)
        assert list(base.names.items()) == list(off.names.items()) and base.n_flat == off.n_flat
        assert (base.pi_off, base.v_off, base.action_dim, base.hidden_v) == (off.pi_off, off.v_off, off.action_dim, off.hidden_v)
        assert base.dist_dueling is False
    plain, duel = make(*args, **kw), make(*args, dist_dueling=True, **kw)
    assert (plain.action_dim, plain.n_actions, plain.dist_dueling) == (a * 51, a, False)        # a plain head is unaffected
    assert list(duel.names) == list(plain.names) and duel.hidden_v and duel.pi_off == plain.pi_off
    assert (duel.action_dim, duel.n_actions, duel.dist_dueling) == ((a + 1) * 51, a, True)
    assert (duel.atoms, duel.quantiles) == (plain.atoms, plain.quantiles)
    assert duel.names[duel.pi_name + "/kernel"][1] == (feat, (a + 1) * 51)
    assert duel.names[duel.pi_name + "/bias"][1] == ((a + 1) * 51,)
    assert duel.v_off == (duel.pi_off + (feat + 1) * (a + 1) * 51 + 3) & ~3 and duel.v_name + "/kernel" not in duel.names
    assert duel.n_flat == plain.n_flat + (duel.v_off - plain.v_off)
    # the existing positional calls keep working, and the keyword is the trailing one
    if kind == "cnn":
        assert make((84, 84, 4), 4, False, 51 if head == "c51" else 1, 1 if head == "c51" else 51, False, 0.5, True).dist_dueling
    else:
        assert make((4,), 3, 32, 2, False, 51 if head == "c51" else 1, 1 if head == "c51" else 51, False, 0.5, True).dist_dueling
    # noisy: the folded head is one noisy layer of its width, and no v_name appears
    noisy = make(*args, noisy=True, dist_dueling=True, **kw)
    assert [nl.name for nl in noisy.noisy_layers] == [noisy.layers[-1].name, noisy.pi_name]
    assert (noisy.noisy_layers[1].K, noisy.noisy_layers[1].N) == (feat, (a + 1) * 51)
    assert noisy.names[noisy.pi_name + "/sigma_kernel"][1] == (feat, (a + 1) * 51)
    assert not any(k.startswith(noisy.v_name + "/") for k in noisy.names)


def test_dqn_spec_and_the_models_follow_the_key():
    from xingtian_amd.model import model_builder
    from xingtian_amd.model.dqn.dqn_cnn import dqn_spec
    for name in ("DqnMlp", "DqnCnn"):
        for kw in (dict(atoms=51), dict(quantiles=8)):
            n = kw.get("atoms", kw.get("quantiles"))
            spec = dqn_spec(_info(name, dist_dueling=True, **kw))
            assert (spec.action_dim, spec.n_actions, spec.dist_dueling) == (4 * n, 3, True)
            assert dqn_spec(_info(name, **kw)).action_dim == 3 * n and not dqn_spec(_info(name, **kw)).dist_dueling
    model = model_builder(_info(atoms=51, dist_dueling=True, noisy=True))
    assert model.dist_dueling and model.net.spec.dist_dueling and not model.dueling
    assert sorted(model.get_weights()) == sorted(
        "%s/%s" % (l, v) for l in ("dense", "dense_1") for v in ("kernel", "bias", "sigma_kernel", "sigma_bias"))
    assert model.get_weights()["dense_1/kernel"].shape == (32, 4 * 51)
    assert not model_builder(_info(atoms=51)).dist_dueling


# ------------------------------------------------------------------------------------------------ refusals
def test_every_refusal_names_its_reason_and_the_pinned_ones_still_raise():
    from xingtian_amd.model import model_builder, netspec
    from xingtian_amd.model.dqn.dqn_cnn import dqn_spec
    for name in ("DqnMlp", "DqnCnn"):
        # without atoms or quantiles > 1: a ValueError that names the plain key
        for mc in (dict(dist_dueling=True), dict(dist_dueling=True, atoms=1), dict(dist_dueling=True, quantiles=1),
                   dict(dist_dueling=True, dueling=True)):
            with pytest.raises(ValueError, match="dist_dueling without atoms or quantiles > 1.*`dueling`"):
                model_builder(_info(name, **mc))
            with pytest.raises(ValueError, match="dist_dueling without atoms or quantiles > 1.*`dueling`"):
                dqn_spec(_info(name, **mc))
        # together with dueling: true the old refusal wins, with its text
        with pytest.raises(NotImplementedError, match="dueling stream is 1 wide.*needs an atoms-wide one"):
            model_builder(_info(name, atoms=51, dueling=True, dist_dueling=True))
        with pytest.raises(NotImplementedError, match="dueling stream is 1 wide.*needs a quantiles-wide one"):
            model_builder(_info(name, quantiles=51, dueling=True, dist_dueling=True))
        # the pinned refusals, now with a pointer to the key
        with pytest.raises(NotImplementedError, match="dueling with atoms = 51: the dueling stream is 1 wide.*dist_dueling"):
            model_builder(_info(name, atoms=51, dueling=True))
        with pytest.raises(NotImplementedError, match="dueling with quantiles = 51: the dueling stream is 1 wide.*dist_dueling"):
            model_builder(_info(name, quantiles=51, dueling=True))
        # 64 actions: the folded head would be 65 groups wide
        for kw in (dict(atoms=2), dict(quantiles=2)):
            with pytest.raises(ValueError, match="dist_dueling: action_dim = 64 exceeds 63"):
                model_builder(_info(name, a=64, dist_dueling=True, **kw))
            assert model_builder(_info(name, a=64, **kw)).net.spec.action_dim == 128        # (64 stays fine without the key)
        for bad in (1, 0, "yes", None):
            with pytest.raises(ValueError, match="dist_dueling = .* must be a bool"):
                model_builder(_info(name, atoms=51, dist_dueling=bad))
    for make, args in ((netspec.dqn_cnn, ((84, 84, 4), 4)), (netspec.dqn_mlp, ((4,), 3, 32, 2))):
        with pytest.raises(NotImplementedError, match="dueling stream is 1 wide.*atoms-wide"):
            make(*args, dueling=True, atoms=51, dist_dueling=True)
        with pytest.raises(NotImplementedError, match="dueling stream is 1 wide.*quantiles-wide"):
            make(*args, dueling=True, quantiles=51, dist_dueling=True)
        with pytest.raises(ValueError, match="dist_dueling without atoms or quantiles > 1"):
            make(*args, dist_dueling=True)
        with pytest.raises(ValueError, match="exceeds 63"):
            make(args[0], 64, *args[2:], atoms=2, dist_dueling=True)
        assert make(args[0], 63, *args[2:], atoms=2, dist_dueling=True).action_dim == 128


def test_dqn_refuses_a_dueling_distributional_actor_without_the_device_step():
    from xingtian_amd.algorithm import alg_builder
    cfg = {"instance_num": 1, "agent_num": 1, "prepare_times_per_train": 1, "BUFFER_SIZE": 50, "BATCH_SIZE": 8}
    with pytest.raises(NotImplementedError, match="distributional actor \\(atoms = 51\\) needs a model with the device step"):
        alg_builder("DQN", {"actor": _info(atoms=51, dist_dueling=True)}, cfg)
    with pytest.raises(NotImplementedError, match="quantile actor \\(quantiles = 8\\) needs a model with the device step"):
        alg_builder("DQN", {"actor": _info(quantiles=8, dist_dueling=True)}, cfg)


# ------------------------------------------------------------------------------------------------ the definitions
@pytest.mark.parametrize("a,n", [(1, 2), (2, 51), (3, 65), (18, 8)])
def test_combine_twin_against_float64_and_its_gradient_twin_against_central_differences(a, n):
    from xingtian_amd.model.dqn.dqn_cnn import dist_dueling_combine, dist_dueling_combine_grad
    rng = np.random.default_rng(a * n)
    b = 5
    cols = (rng.standard_normal((b, (a + 1) * n)) * 2.0).astype(np.float32)
    l = dist_dueling_combine(cols, a, n)
    assert l.dtype == np.float32 and l.shape == (b, a, n)
    assert np.array_equal(l, U.combine(cols, a, n, np.float32))               # the helpers' float32 restatement, bit for bit
    want = U.combine(cols, a, n)
    assert np.abs(l - want).max() <= 4 * 2.0 ** -24 * np.abs(cols).max() * 3
    if a == 1:
        assert np.array_equal(l[:, 0], cols[:, n:])                           # adv - mean is exactly 0
    # the gradient twin: f(cols) = sum_i g_i l[act, i] has gradient dcol = twin(g, act); central differences in float64
    act = rng.integers(0, a, b)
    g = rng.standard_normal((b, n)).astype(np.float32)
    got = dist_dueling_combine_grad(g, act, a)
    assert got.dtype == np.float32 and got.shape == (b, (a + 1) * n)
    f = lambda c: (U.combine(c, a, n)[np.arange(b), act] * g.astype(np.float64)).sum()
    c64, h = cols.astype(np.float64), 1e-3
    num = np.zeros_like(c64)
    for r in range(b):
        for k in range((a + 1) * n):
            e = np.zeros_like(c64)
            e[r, k] = h
            num[r, k] = (f(c64 + e) - f(c64 - e)) / (2 * h)
    assert np.abs(got - num).max() <= 1e-6 * max(1.0, np.abs(num).max())     # (f is linear: the differences are exact to rounding)
    dl = np.zeros((b, a, n))
    dl[np.arange(b), act] = g
    assert np.abs(U.combine_transpose(dl.reshape(b, -1), a, n) - num).max() <= 1e-8 * max(1.0, np.abs(num).max())
    assert np.abs(U.combine_grad(dl.reshape(b, -1), act, a, n) - num).max() <= 1e-8 * max(1.0, np.abs(num).max())
    assert np.array_equal(got, U.combine_grad(dl.reshape(b, -1).astype(np.float32), act, a, n, np.float32))


@pytest.mark.parametrize("head", U.HEADS)
def test_cpu_replica_predict_combines_first_and_agrees_with_float64(head):
    from xingtian_amd.model import model_builder
    from xingtian_amd.model.dqn.dqn_cnn import dist_dueling_combine, dist_q, dist_support, quant_q
    kw = dict(atoms=51, v_min=-5.0, v_max=15.0) if head == "c51" else dict(quantiles=51)
    model = model_builder(_info(dist_dueling=True, **kw))
    assert model.net.inference_only and model.dist_dueling
    assert sorted(model.get_weights()) == ["dense/bias", "dense/kernel", "dense_1/bias", "dense_1/kernel"]
    assert model.get_weights()["dense_1/kernel"].shape == (32, 4 * 51)
    rng = np.random.default_rng(0)
    w = {k: (rng.standard_normal(v.shape) * 0.5).astype(np.float32) for k, v in model.get_weights().items()}
    model.set_weights(w)
    x = rng.standard_normal((9, 4)).astype(np.float32)
    q = model.predict(x)
    cols = np.asarray(model.net.forward(x)[0])
    assert q.shape == (9, 3) and q.dtype == np.float32 and cols.shape == (9, 4 * 51)
    l32 = dist_dueling_combine(cols, 3, 51)
    assert np.array_equal(q, dist_q(l32, dist_support(51, -5.0, 15.0)[0]) if head == "c51" else quant_q(l32))
    h = np.maximum(x.astype(np.float64) @ w["dense/kernel"] + w["dense/bias"], 0.0)
    l64 = U.combine(h @ w["dense_1/kernel"] + w["dense_1/bias"], 3, 51)
    if head == "c51":
        e = np.exp(l64 - l64.max(-1, keepdims=True))
        want = (dist_support(51, -5.0, 15.0)[0] * e).sum(-1) / e.sum(-1)
    else:
        want = l64.mean(-1)
    assert np.abs(q - want).max() <= 1e-4
    # the same YAML without the key keeps the [N, A] output of its A * N wide head
    assert model_builder(_info(**kw)).predict(x).shape == (9, 3)


# ------------------------------------------------------------------------------------------------ the head tests' tables
@pytest.mark.parametrize("head", U.HEADS)
def test_head_cases_keep_the_argmax_stable_and_hold_every_planted_row(head):
    seen = set()
    for shape in U.HEAD_SHAPES:
        for v in U.HEAD_VARIANTS:
            c = U.head_case(head, shape, *v)
            b, a, n = shape
            assert c["logits"].shape == (b, (a + 1) * n)
            ref = U.head_ref(c)
            gap = U.argmax_gap(c, ref)
            assert gap >= U.min_gap(head), (head, shape, v, gap)               # no case may be skipped
            pl = c["planted"]
            seen.update(pl)
            for name in ("tie", "equal_adv"):
                if name in pl and a > 1:
                    assert ref["astar"][pl[name]] == 0 and np.ptp(ref["q_pick"][pl[name]]) == 0.0, name
            if "equal_adv" in pl:                                           # the combined rows ARE the value group
                row = pl["equal_adv"]
                l32 = U.combine(c["logits"][row:row + 1], a, n, np.float32)[0]
                assert all(np.array_equal(l32[k], c["logits"][row, a * n:]) for k in range(a))
            if "integer" in pl and v[2]:
                assert np.array_equal(ref["m"][pl["integer"]], ref["p"][pl["integer"]])
            if "clamp_hi" in pl:
                assert ref["act"][pl["clamp_hi"]] == a - 1 and ref["m"][pl["clamp_hi"], -1] > 0.999999
            if "clamp" in pl:
                assert ref["act"][pl["clamp"]] == a - 1
            if "done" in pl:
                assert ref["act"][pl["done"]] == 0
            if "zero" in pl:
                l32 = U.combine(c["logits"], a, n, np.float32)                  # (exact in the kernel's float32 combine)
                u = ref["target"][pl["zero"]].astype(np.float32)[None, :] - l32[pl["zero"], ref["act"][pl["zero"]]][:, None]
                assert (u[n // 2] == 0.0).all()
            if "kappa" in pl:
                u = ref["target"][pl["kappa"]].astype(np.float64)[None, :] - ref["l"][pl["kappa"], ref["act"][pl["kappa"]]][:, None]
                assert (np.abs(u) == U.KAPPA).any() and (u * 2 == np.round(u * 2)).all()
            # the folded gradient row: the value group is d_i, the untaken groups are equal, and the groups sum to d_i
            d3 = ref["dcols"].reshape(b, a + 1, n)
            assert np.array_equal(d3[:, a], ref["d"]) and np.abs(d3[:, :a].sum(1)).max() <= 1e-12 * max(1.0, np.abs(ref["d"]).max())
    assert seen == set(U.PLANTED[head])


@pytest.mark.parametrize("head", U.HEADS)
def test_head_bars_are_four_times_the_float32_restatements_deviation_and_the_gradient_bar_is_at_most_1e_5(head):
    measured, bars = U.head_bars(head)
    print("duel", head, "head: float32 NumPy restatement vs float64 (rel_max)", measured, "-> bars", bars)
    assert set(measured) == set(U.HEAD_QUANTITIES[head])
    for k in U.HEAD_QUANTITIES[head]:
        assert measured[k] > 0.0 and bars[k] == 4.0 * measured[k], k
    assert bars["dcols"] <= 1e-5                      # (a bar above the project's gradient bar would be a finding)


# ------------------------------------------------------------------------------------------------ ABI
def test_abi_header_signatures_and_exported_symbols_agree_for_the_four_duel_entries():
    from xingtian_amd import lib as L
    with open(os.path.join(ROOT, "include", "xt_mi355x.h")) as f:
        header = f.read()
    assert re.search(r"#define XT_ABI_VERSION 12\b", header) and L.ABI_VERSION == 12
    handle = L.load()
    assert handle.xt_abi_version() == 12
    for name in ("xt_dqn_loss_dist_duel", "xt_dqn_loss_quant_duel", "xt_net_set_duel", "xt_heads_dfeat_duel"):
        m = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert m, name
        args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
        res, sig = L.SIGNATURES[name]
        assert res is ctypes.c_int32 and len(sig) == len(args), (name, len(sig), len(args))
        for a, c in zip(args, sig):
            if "*" in a:
                assert c is ctypes.c_void_p, (name, a)
            else:
                want = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "double": ctypes.c_double}[a.split()[0]]
                assert c is want, (name, a)
        assert getattr(handle, name)
    # the _duel heads take the argument lists of the entries without it, and no existing entry changed its signature
    for base in ("xt_dqn_loss_dist", "xt_dqn_loss_quant"):
        assert L.SIGNATURES[base + "_duel"] == L.SIGNATURES[base]
        old = re.search(r"\bint %s\(([^;]*)\);" % base, header).group(1)
        new = re.search(r"\bint %s_duel\(([^;]*)\);" % base, header).group(1)
        assert " ".join(old.split()) == " ".join(new.split())
    assert len(L.SIGNATURES["xt_net_dqn_step_dist"][1]) == len(L.SIGNATURES["xt_net_dqn_step_quant"][1]) == 18
