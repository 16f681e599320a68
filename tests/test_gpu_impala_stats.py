"""GPU tests of the per-train IMPALA v-trace diagnostics (``ImpalaCnnOpt`` ``model_config.TRAIN_STATS``, C ABI
``xt_net_set_impala_stats`` / ``xt_impala_heads_stats_ex`` / ``xt_impala_loss_stats``).

Inputs and the float64 restatement come from tests/impala_stats_helpers.py (recipe, margin assertion and the tie to
``oracle.nets`` are checked on the CPU by tests/test_cpu_impala_stats.py).

Bars (the project's own, REL / FLOOR / GRAD_REL of tests/test_gpu_train_stats.py): 1e-4 relative with a 1e-6 floor for
loss-like scalars, 1e-5 for gradient norms; a sum that can cancel -- sum(vs - v), sum(ce * pg), sum(-log rho) -- is compared
with |got - ref| <= 1e-4 * sum|term| + 1e-6, sum|term| from the float64 restatement.  Counts, chunks and transitions are
exact.  Everything that compares two runs of this code is bitwise.  Every figure is printed before it is asserted."""
import ctypes

import numpy as np
import pytest
import torch

import impala_stats_helpers as H

pytestmark = pytest.mark.gpu

REL, FLOOR, GRAD_REL = 1e-4, 1e-6, 1e-5
CANCELS = (0, 3, 6)            # columns whose sum can cancel: ce * pg, vs - v, -log rho
F = 20                         # features of the stand-alone fused kernel calls (no multiple of anything)
PAD = 2                        # rows of traj_stats behind the last trajectory that must stay untouched


@pytest.fixture(autouse=True)
def _module_constants_restored():
    """model_config / alg_config keys override module-level constants (``import_config``): leave them as they were"""
    from xingtian_amd.algorithm.impala import impala_opt as alg_mod
    from xingtian_amd.model.impala import impala_cnn_opt as model_mod
    lr, batch = model_mod.LR, alg_mod.BATCH_SIZE
    yield
    model_mod.LR, alg_mod.BATCH_SIZE = lr, batch


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def nan_buf(n):
    return torch.full((max(int(n), 1),), float("nan"), dtype=torch.float32, device="cuda")


def bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def near(got, ref, rel=REL, floor=FLOOR):
    return abs(got - ref) <= max(rel * abs(ref), floor)


_INPUTS = {}


def inputs(case):
    """the recipe's inputs of one (n_traj, T, A) case with their float64 restatement (built once, never modified)"""
    if case not in _INPUTS:
        d = H.make_inputs(*case)
        rng = np.random.default_rng(1000 + sum(case))
        d["feat"] = np.maximum(rng.standard_normal((case[0] * case[1], F)), 0.0).astype(np.float32)
        d["wpi"] = (0.3 * rng.standard_normal((F, case[2]))).astype(np.float32)
        d["wv"] = (0.3 * rng.standard_normal(F)).astype(np.float32)
        d["bpi"], d["bv"] = np.zeros(case[2], np.float32), np.zeros(1, np.float32)
        d["ref"] = H.restate(d["logits"], d["baseline"], d["bp"], d["action"], d["done"], d["reward"], case[1])
        _INPUTS[case] = d
    return _INPUTS[case]


def check_rows(tag, case, rows, ref):
    """traj_stats [n_traj + PAD, 12] of one kernel call against the float64 restatement, per trajectory row"""
    n_traj, T, _ = case
    want, mags = H.traj_rows(ref)
    assert np.isnan(rows[n_traj:]).all(), (tag, "rows beyond n_traj were written")
    got = rows[:n_traj].astype(np.float64)
    assert np.isfinite(got).all()
    assert (got[:, 10] == T - 1).all() and (got[:, 11] == 0.0).all()
    assert np.array_equal(got[:, 8], want[:, 8]), (tag, "count of rho > 1", got[:, 8], want[:, 8])
    worst = (0.0, None)
    for c in range(10):
        for i in range(n_traj):
            g, w = got[i, c], want[i, c]
            bar = REL * mags[i, c] + FLOOR if c in CANCELS else max(REL * abs(w), FLOOR)
            e = abs(g - w)
            if e / bar > worst[0]:
                worst = (e / bar, (c, i, g, w, e, bar))
            assert e <= bar, (tag, "column", c, "trajectory", i, g, w, e, bar)
    print("impala_stats rows: %s case %s worst err/bar %.3e at (column, traj, got, ref, err, bar) %s" % (tag, case, *worst))
    return worst


def check_sums(tag, case, stats, rows):
    """the 16 doubles after ONE reduce over a cleared block: the rows added in trajectory order, in double -- exactly"""
    n_traj, T, _ = case
    r = rows[:n_traj].astype(np.float64)
    want = np.zeros(16)
    want[0], want[1] = 1.0, 0.0
    for i in range(n_traj):
        want[1] += r[i, 10]
        for c in range(10):
            want[2 + c] = max(want[2 + c], r[i, c]) if c == H.MAX_COL else want[2 + c] + r[i, c]
    assert np.array_equal(stats, want), (tag, stats, want)
    assert stats[1] == n_traj * (T - 1) and (stats[12:] == 0.0).all()


def device_inputs(d):
    keys = ("feat", "wpi", "bpi", "wv", "bv", "bp", "action", "reward", "logits", "baseline")
    t = {k: dev(d[k]) for k in keys}
    t["done"] = dev(d["done"].astype(np.uint8))
    return t


def run_fused(L, case, with_stats):
    n_traj, T, A = case
    d = inputs(case)
    n, nm = n_traj * T, n_traj * (T - 1)
    o = dict(dlogits=nan_buf(n * A), dbaseline=nan_buf(n), vs=nan_buf(nm), pg=nan_buf(nm), dfeat=nan_buf(n * F),
             traj_loss=nan_buf(n_traj), loss=nan_buf(1))
    path = ctypes.c_int32(-1)
    i = device_inputs(d)              # (kept alive until the launches have run)
    args = [L.ptr(i["feat"]), None, 1, 0, None, L.ACT["relu"], 0, n_traj, T, F, A, L.ptr(i["wpi"]),
            L.ptr(i["bpi"]), L.ptr(i["wv"]), L.ptr(i["bv"]), L.ptr(i["bp"]), L.ptr(i["action"]),
            L.ptr(i["done"]), L.ptr(i["reward"]), H.GAMMA, L.ACT["relu"], None,
            L.ptr(i["logits"]), L.ptr(i["baseline"]), L.ptr(o["dlogits"]), L.ptr(o["dbaseline"]), L.ptr(o["vs"]),
            L.ptr(o["pg"]), L.ptr(o["dfeat"]), L.ptr(o["traj_loss"]), L.ptr(o["loss"]), None, ctypes.byref(path)]
    if with_stats:
        o["traj_stats"] = nan_buf((n_traj + PAD) * H.K)
        o["stats"] = torch.zeros(16, dtype=torch.float64, device="cuda")
        rc = L.load().xt_impala_heads_stats_ex(*args, L.ptr(o["traj_stats"]), L.ptr(o["stats"]))
        L.check(rc, "xt_impala_heads_stats_ex")
    else:
        L.check(L.load().xt_impala_heads_ex(*args), "xt_impala_heads_ex")
    torch.cuda.synchronize()
    return o, path.value


def run_unfused(L, case, with_stats):
    n_traj, T, A = case
    d = inputs(case)
    n, nm = n_traj * T, n_traj * (T - 1)
    o = dict(dlogits=nan_buf(n * A), dbaseline=nan_buf(n), vs=nan_buf(nm), pg=nan_buf(nm), out=nan_buf(4 + n_traj))
    i = device_inputs(d)              # (kept alive until the launches have run)
    args = [L.ptr(i["logits"]), L.ptr(i["baseline"]), L.ptr(i["bp"]), L.ptr(i["action"]),
            L.ptr(i["done"]), L.ptr(i["reward"]), n_traj, T, A, H.GAMMA, L.ptr(o["dlogits"]),
            L.ptr(o["dbaseline"]), L.ptr(o["out"]), None, L.ptr(o["vs"]), L.ptr(o["pg"]), None]
    path = ctypes.c_int32(-1)
    if with_stats:
        o["traj_stats"] = nan_buf((n_traj + PAD) * H.K)
        o["stats"] = torch.zeros(16, dtype=torch.float64, device="cuda")
        rc = L.load().xt_impala_loss_stats(*args, L.ptr(o["traj_stats"]), L.ptr(o["stats"]), ctypes.byref(path))
        L.check(rc, "xt_impala_loss_stats")
    else:
        L.check(L.load().xt_impala_loss(*args), "xt_impala_loss")
    torch.cuda.synchronize()
    return o, path.value


def check_kernel(tag, case, plain, stat):
    for k in plain:                  # dlogits, dbaseline, dfeat, traj_loss, vs, pg_adv (and the loss): the existing entry's bits
        a, b = bits(plain[k]), bits(stat[k])
        assert np.array_equal(a, b), (tag, case, k)
        if k != "out":
            assert np.isfinite(plain[k].cpu().numpy()).all(), (tag, case, k)
    rows = stat["traj_stats"].cpu().numpy().reshape(-1, H.K)
    worst = check_rows(tag, case, rows, inputs(case)["ref"])
    check_sums(tag, case, stat["stats"].cpu().numpy(), rows)
    return worst


@pytest.mark.parametrize("case", H.FUSED8 + H.FUSED32, ids=lambda c: "x".join(map(str, c)))
def test_fused_kernel_rows_against_float64_and_outputs_bitwise(case):
    from xingtian_amd import lib as L
    plain, p0 = run_fused(L, case, False)
    stat, p1 = run_fused(L, case, True)
    am = 8 if case[2] <= 8 else 32
    assert p1 == p0 | L.IMPALA_PATH_STATS_BIT and (p0 & 0xf) == 2 and (p0 >> 10) & 0x3f == am, (hex(p0), hex(p1))
    check_kernel("fused AM %d" % am, case, plain, stat)


@pytest.mark.parametrize("case", H.UNFUSED, ids=lambda c: "x".join(map(str, c)))
def test_unfused_kernel_rows_against_float64_and_outputs_bitwise(case):
    from xingtian_amd import lib as L
    plain, _ = run_unfused(L, case, False)
    stat, path = run_unfused(L, case, True)
    T = case[1]
    maxt = 64 if T <= 64 else 128 if T <= 128 else 256 if T <= 256 else 1024
    assert path == L.IMPALA_PATH_LOSS | (maxt // 64) << 10 | L.IMPALA_PATH_STATS_BIT, hex(path)
    check_kernel("unfused MAXT %d" % maxt, case, plain, stat)


# ------------------------------------------------------------------ one step through the net
def check_slots(tag, acc, want, mag):
    """the running sums against float64 (`want`, `mag` of impala_stats_helpers.sums16); -> nothing, asserts"""
    from xingtian_amd import lib as L
    S = L.IMPALA_STATS_SLOTS
    assert acc[S["CHUNKS"]] == want[0] and acc[S["TRANSITIONS"]] == want[1] and acc[S["RESERVED"]] == 0.0
    assert acc[S["RHO_CLIPPED"]] == want[S["RHO_CLIPPED"]], (tag, acc[S["RHO_CLIPPED"]], want[S["RHO_CLIPPED"]])
    for k in ("PG", "ENT", "VERR_SQ", "VERR", "VS", "VS_SQ", "NEG_LOG_RHO", "RHO", "RHO_MAX"):
        g, w = acc[S[k]], want[S[k]]
        bar = REL * mag[S[k]] + FLOOR if (S[k] - 2) in CANCELS else max(REL * abs(w), FLOOR)
        print("impala_stats sums: %s %-12s got %+.9e ref %+.9e err %.2e bar %.2e" % (tag, k, g, w, abs(g - w), bar))
        assert abs(g - w) <= bar, (tag, k, g, w, bar)


@pytest.mark.parametrize("dim,a_dim,tlen,ntraj,mean,std", [(84, 4, 128, 1, 0.0, 255.0), (42, 6, 50, 2, 128.0, 128.0),
                                                            (42, 18, 5, 4, 128.0, 128.0)])
def test_one_step_through_the_net_against_the_oracle(dim, a_dim, tlen, ntraj, mean, std):
    from oracle import nets
    from xingtian_amd import lib as L
    from xingtian_amd.model import netspec
    from xingtian_amd.model.hip_net import HipActorCritic
    S = L.IMPALA_STATS_SLOTS
    n = tlen * ntraj
    net = HipActorCritic(netspec.impala_cnn_opt((dim, dim, 4), a_dim, mean, std), max_batch=n, seed=0)
    ospec = nets.impala_cnn_opt_spec((dim, dim, 4), a_dim, mean, std)
    params = nets.init_params(ospec, seed=5, bias_scale=0.05)
    net.set_weights({k: v.reshape(net.spec.names[k][1]) for k, v in params.items()})
    rng = np.random.default_rng(11)
    obs = rng.integers(0, 256, (n, dim, dim, 4)).astype(np.uint8)
    act = rng.integers(0, a_dim, n).astype(np.int32)
    done = rng.random(n) < 0.05
    rew = (2.0 * rng.standard_normal(n)).astype(np.float32)
    orc = nets.ImpalaLearnerOracle(ospec, params, dict(LR=5e-4, grad_norm_clip=40.0, sample_batch_step=tlen, BATCH_SIZE=n),
                                   np.float64)
    logits64, _ = orc.net.forward(obs)
    bp, _, margin = H.behaviour_logits(logits64.astype(np.float32), act, rng, ntraj, tlen, on_policy=False)
    out = orc.step(obs, bp, act, done, rew, apply=False)
    ref = H.restate(out["logits"], out["baseline"], bp, act, done, rew, tlen)
    assert abs(ref["terms"].sum() - out["loss"]) <= 1e-12 * abs(out["loss"])
    net.set_impala_stats(True)
    net.clear_impala_stats()
    c = net.make_impala_cfg(5e-4, 40.0, tlen)
    t = [dev(obs), dev(bp), dev(act), dev(done.astype(np.uint8)), dev(rew)]
    lo = net.impala_step(c, *t, apply=True)
    acc = net.fetch_impala_stats()
    loss = float(lo.cpu().numpy()[0])
    tag = "net %dx%d A %d T %d x %d (margin %.2e)" % (dim, dim, a_dim, tlen, ntraj, margin)
    want, mag = H.sums16([ref])
    check_slots(tag, acc, want, mag)
    assert near(loss, float(out["loss"]), REL, FLOOR)
    gn = float(out["gnorm"])
    print("impala_stats sums: %s gnorm got %.9e ref %.9e" % (tag, acc[S["GNORM_SUM"]], gn))
    assert near(acc[S["GNORM_SUM"]], gn, GRAD_REL, 0.0) and acc[S["GNORM_MAX"]] == acc[S["GNORM_SUM"]]
    assert acc[S["GNORM_CLIPPED"]] == float(gn > 40.0)
    path = net.last_head_path()
    assert path & L.IMPALA_PATH_STATS_BIT
    if a_dim > 8:                                # the unfused heads: impala_loss_kernel<64, true>
        assert path == L.IMPALA_PATH_LOSS | 1 << 10 | L.IMPALA_PATH_STATS_BIT, hex(path)
    else:
        assert (path & 0xf) == 2 and (path >> 10) & 0x3f == 8, hex(path)
    # a gradient-only step adds its rows and leaves the three gradient-norm slots alone
    net.clear_impala_stats()
    net.impala_step(c, *t, apply=False)
    acc0 = net.fetch_impala_stats()
    assert acc0[S["CHUNKS"]] == 1.0 and acc0[S["TRANSITIONS"]] == want[1] and (acc0[12:] == 0.0).all()
    net.check_device_errors()


# ------------------------------------------------------------------ whole trains through ImpalaCnnOpt
N_FR, T_M, A_M, BATCH = 100, 10, 6, 40          # 10 trajectories of 10 frames; chunks of 40 / 40 / 20 frames
ZERO_LR = [[0, 0.0], [20000, 0.0]]              # lr_schedule: linear_cosine_decay of 0 -> every Adam step size is 0


def info(stats=True, **cfg):
    mc = dict(LR=1e-3, sample_batch_step=T_M, grad_norm_clip=40.0, SEED=3, MAX_BATCH=128, USE_HIP_GRAPH=False)
    if stats:
        mc["TRAIN_STATS"] = True
    mc.update(cfg)
    return {"model_name": "ImpalaCnnOpt", "state_dim": [42, 42, 4], "input_dtype": "uint8", "state_mean": 128.0,
            "state_std": 128.0, "action_dim": A_M, "model_config": mc}


def build(stats=True, **cfg):
    from xingtian_amd.model import model_builder
    return model_builder(info(stats, **cfg))


_DATA = {}


def data():
    """the rollout of the model tests (built once, never modified): bp_logits by the recipe from the float64 logits of
    the oracle at the SEED 3 weights, and the float64 restatement of each of the three chunks at those weights"""
    if _DATA:
        return _DATA
    from oracle import nets
    model = build(stats=False)
    w0 = model.get_weights()
    ospec = nets.impala_cnn_opt_spec((42, 42, 4), A_M, 128.0, 128.0)
    shapes = nets.init_params(ospec)
    orc = nets.ImpalaLearnerOracle(ospec, {k: v.reshape(shapes[k].shape) for k, v in w0.items()},
                                   dict(LR=1e-3, grad_norm_clip=40.0, sample_batch_step=T_M, BATCH_SIZE=BATCH), np.float64)
    rng = np.random.default_rng(21)
    obs = rng.integers(0, 256, (N_FR, 42, 42, 4)).astype(np.uint8)
    act = rng.integers(0, A_M, N_FR).astype(np.int32)
    done = rng.random(N_FR) < 0.05
    rew = (2.0 * rng.standard_normal(N_FR)).astype(np.float32)
    logits64, value64 = orc.net.forward(obs)
    bp, _, margin = H.behaviour_logits(logits64.astype(np.float32), act, rng, N_FR // T_M, T_M, on_policy=False)
    chunks = []
    for lo in range(0, N_FR, BATCH):
        s = slice(lo, lo + BATCH)
        chunks.append(H.restate(logits64[s], value64[s, 0], bp[s], act[s], done[s], rew[s], T_M))
    # the float64 norm of each chunk's gradient, by gradient-only replay on the untrained net
    net = model.net
    c = net.make_impala_cfg(1e-3, 40.0, T_M)
    norms = []
    for lo in range(0, N_FR, BATCH):
        s = slice(lo, lo + BATCH)
        t = [dev(obs[s]), dev(bp[s]), dev(act[s]), dev(done[s].astype(np.uint8)), dev(rew[s])]
        net.impala_step(c, *t, apply=False)
        torch.cuda.synchronize()
        norms.append(float(np.sqrt(sum((v.astype(np.float64) ** 2).sum() for v in net.grads_dict().values()))))
    _DATA.update(obs=obs, bp=bp, action=act, done=done, reward=rew, chunks=chunks, norms=np.array(norms), margin=margin)
    return _DATA


def clip_between(norms):
    """grad_norm_clip inside the widest gap of the norms: some chunks clipped, some not, none within 1 % of the bound"""
    s = np.sort(norms)
    j = int(np.argmax(s[1:] / s[:-1]))
    clip = float(np.sqrt(s[j] * s[j + 1]))
    assert s[0] < clip < s[-1] and (np.abs(norms - clip) >= 0.01 * norms).all(), (norms, clip)
    return clip


def run_train(model, batch=BATCH, lo=0, hi=N_FR):
    """``ImpalaCnnOpt.train`` on frames [lo, hi) with chunks of `batch` frames (``train`` itself makes one chunk)"""
    d = data()
    ing = model._ingest_obj()
    ing.reset()
    ing.put(d["obs"][lo:hi], d["bp"][lo:hi], d["action"][lo:hi], d["done"][lo:hi], d["reward"][lo:hi])
    return model.train_ingested(batch)


def state_of(model):
    net = model.net
    return [net.params.cpu().numpy().copy(), net.adam_m.cpu().numpy().copy(), net.adam_v.cpu().numpy().copy(),
            net.adam_state.cpu().numpy().copy()]


def same_bits(x, y):
    return all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(x, y))


def stats_bits(d):
    return np.array([d[k] for k in sorted(d)], np.float64).tobytes()


@pytest.mark.parametrize("opt", ["adam", "rmsprop"])
def test_whole_train_with_zero_step_size(opt):
    d = data()
    norms = d["norms"]
    clip = clip_between(norms)
    over = dict(lr_schedule=ZERO_LR) if opt == "adam" else dict(LR=0.0, opt_type="rmsprop")
    model = build(grad_norm_clip=clip, **over)
    w0 = model.net.params.cpu().numpy().copy()
    assert model.train_stats() is None
    loss = run_train(model)
    s = model.train_stats()
    assert np.array_equal(model.net.params.cpu().numpy(), w0)            # (step size 0: every chunk saw the same net)
    want, mag = H.sums16(d["chunks"])
    check_slots("train " + opt, model.net.fetch_impala_stats(), want, mag)
    assert s["chunks"] == 3.0 and s["transitions"] == 90.0
    assert s["rho_clip_fraction"] == want[10] / 90.0
    assert type(s["loss"]) is float and np.float32(s["loss"]) == loss and s["loss"] == float(loss)
    recombined = s["pg_loss"] + 0.5 * s["baseline_loss"] + 0.01 * s["entropy_loss"]
    print("impala_stats train: %s loss %.9e recombined %.9e diff %.2e" % (opt, s["loss"], recombined,
                                                                         abs(s["loss"] - recombined)))
    # (1e-6 of the loss, as every bar of this file is relative: the three chunk losses are float32 sums of magnitude 13
    # to 31 here, whose own half ulp is 1e-6 to 2e-6, so an absolute 1e-6 is below what the float32 loss can carry;
    # measured on an MI355X: |diff| 2.14e-6 at loss -3.593, 6.0e-7 of it)
    assert abs(s["loss"] - recombined) <= 1e-6 * max(1.0, abs(s["loss"]))
    ref_loss = np.mean([c["terms"].sum() for c in d["chunks"]])
    assert near(s["loss"], ref_loss)
    var = lambda k: np.concatenate([c[k].ravel() for c in d["chunks"]]).var()
    assert near(s["explained_variance"], 1.0 - var("verr") / var("vs"))
    print("impala_stats train: %s norms %s clip %.6e got mean %.9e max %.9e" % (opt, norms, clip, s["grad_norm"],
                                                                               s["grad_norm_max"]))
    assert near(s["grad_norm"], norms.mean(), GRAD_REL, 0.0) and near(s["grad_norm_max"], norms.max(), GRAD_REL, 0.0)
    assert s["grad_clip_fraction"] == (norms > clip).sum() / 3.0 and 0.0 < s["grad_clip_fraction"] < 1.0
    assert model.train_stats() == s                                       # asked twice: the same dict
    model.net.check_device_errors()


_BASE = {}


def base_stats():
    """the dict of the plain form (Adam, step size 0, no graph, no in-graph tail), three chunks"""
    if not _BASE:
        clip = clip_between(data()["norms"])
        model = build(grad_norm_clip=clip, lr_schedule=ZERO_LR, IO_TAIL_IN_GRAPH=0)
        run_train(model)
        _BASE.update(clip=clip, stats=model.train_stats())
    return _BASE


def assert_same_rows(tag, d, base):
    for k in base:
        if k in ("grad_norm", "grad_norm_max"):
            print("impala_stats tails: %s %s got %.9e base %.9e" % (tag, k, d[k], base[k]))
            assert near(d[k], base[k], GRAD_REL, 0.0), (tag, k, d[k], base[k])
        elif k != "loss":
            assert d[k] == base[k], (tag, k, d[k], base[k])
    assert near(d["loss"], base["loss"], REL, FLOOR) and 0.0 < d["grad_clip_fraction"] < 1.0


@pytest.mark.parametrize("form", ["io0_graph", "io1", "io1_graph", "io2", "io2_graph", "rmsprop", "rmsprop_graph", "ticket",
                                  "fused", "overlap"])
def test_every_tail_form_keeps_the_sums(form):
    """The places an IMPALA step can write the gradient norm from and reduce the rows in (the in-graph IO tail and its
    folded form in Adam -- awaited through the mailbox, the deferred loss wait --, centred RMSProp, the ticket knob, the
    fused tail, the split optimiser launch of the overlapped tail), with the first chunk's ``acc_set`` and the later
    chunks' add: with step size 0 the row statistics are those of the plain form bit for bit, the gradient norms agree
    to the gradient bar (the forms group the squared-norm partials differently)."""
    from xingtian_amd import lib as L
    b = base_stats()
    cfg = dict(grad_norm_clip=b["clip"], lr_schedule=ZERO_LR, IO_TAIL_IN_GRAPH=0)
    knobs = {}
    if form.startswith("io"):
        cfg["IO_TAIL_IN_GRAPH"] = int(form[2])
    elif form.startswith("rmsprop"):
        cfg.update(LR=0.0, opt_type="rmsprop")
        del cfg["lr_schedule"]
    else:
        knobs = dict(ticket=dict(finalize_ticket=1), fused=dict(tail_fused=1), overlap=dict(tail_overlap=3))[form]
        cfg["IO_TAIL_IN_GRAPH"] = 2
    cfg["USE_HIP_GRAPH"] = form.endswith("_graph")
    old = L.set_tuning(**knobs)
    try:
        model = build(**cfg)
        for _ in range(2):                      # (with a graph: captured, then replayed)
            run_train(model)
            assert_same_rows(form, model.train_stats(), b["stats"])
        model.net.check_device_errors()
    finally:
        L.set_tuning(**old)


def test_one_chunk_train_counts_one_chunk():
    b = base_stats()
    model = build(grad_norm_clip=b["clip"], lr_schedule=ZERO_LR)
    loss = run_train(model, batch=N_FR)
    s = model.train_stats()
    assert s["chunks"] == 1.0 and s["transitions"] == 90.0 and s["loss"] == float(loss)
    assert s["grad_norm"] == s["grad_norm_max"] > 0.0 and s["grad_clip_fraction"] in (0.0, 1.0)
    # the same transitions at the same weights as the three chunks: the same float rows, added in one group
    for k in ("behaviour_kl", "rho_mean", "entropy", "vs_mean", "explained_variance"):
        assert abs(s[k] - b["stats"][k]) <= 1e-12 * max(1.0, abs(b["stats"][k])), (k, s[k], b["stats"][k])
    assert s["rho_max"] == b["stats"]["rho_max"] and s["rho_clip_fraction"] == b["stats"]["rho_clip_fraction"]
    assert abs(s["pg_loss"] - 3.0 * b["stats"]["pg_loss"]) <= 1e-12 * abs(s["pg_loss"])


def test_on_equals_off():
    runs = {}
    for on in (True, False):
        model = build(stats=on, USE_HIP_GRAPH=True)
        losses = [run_train(model) for _ in range(3)]
        assert (model.train_stats() is not None) == on
        runs[on] = (np.array(losses, np.float32), state_of(model), model._global_step)
    assert np.array_equal(runs[True][0].view(np.uint32), runs[False][0].view(np.uint32))
    assert same_bits(runs[True][1], runs[False][1])
    assert runs[True][2] == runs[False][2] == 9
    assert not np.array_equal(runs[True][1][0], build(stats=False).net.params.cpu().numpy())       # (it did train)


def test_graph_replay_equals_eager_and_runs_repeat():
    runs = []
    for graph in (True, False, True):
        model = build(USE_HIP_GRAPH=graph)
        seen = []
        for _ in range(3):                     # (train 3 replays the graph a second time)
            run_train(model)
            s = model.train_stats()
            assert s["chunks"] == 3.0 and s["transitions"] == 90.0          # nothing leaks from one train into the next
            assert np.isfinite(list(s.values())).all() and s["grad_norm_max"] >= s["grad_norm"] > 0.0
            seen.append(stats_bits(s))
        assert len(set(seen)) == 3             # (LR > 0: the trains differ)
        runs.append(seen)
    assert runs[0] == runs[1], "graph replay and eager differ"
    assert runs[0] == runs[2], "two identical runs differ"


def test_through_the_plugin_pair():
    """IMPALAOpt: prepare_data x 2, train, train_stats -- the bits of ImpalaCnnOpt.train on the concatenated arrays"""
    from xingtian_amd.algorithm import alg_builder
    d = data()
    alg = alg_builder("IMPALAOpt", {"actor": info()}, {"instance_num": 2, "agent_num": 1, "prepare_times_per_train": 2,
                                                      "BATCH_SIZE": 40})
    assert alg.train_stats() is None
    for lo in (0, 20):
        s = slice(lo, lo + 20)
        alg.prepare_data({"cur_state": d["obs"][s], "logit": d["bp"][s], "action": d["action"][s], "done": list(d["done"][s]),
                          "reward": list(d["reward"][s].astype(np.float64))})
    loss = alg.train()
    got = alg.train_stats()
    assert alg.train_stats() == got            # twice in a row: the same dict
    model = build()
    ref_loss = model.train(d["obs"][:40], [d["bp"][:40], d["action"][:40], d["done"][:40], d["reward"][:40]])
    ref = model.train_stats()
    assert np.float32(loss).tobytes() == np.float32(ref_loss).tobytes()
    assert got["chunks"] == 1.0 and got["transitions"] == 36.0 and stats_bits(got) == stats_bits(ref)


def test_switching_off_and_refusals():
    on, never = build(USE_HIP_GRAPH=True), build(stats=False, USE_HIP_GRAPH=True)
    for _ in range(2):
        run_train(on), run_train(never)
    assert on.train_stats() is not None
    on.net.set_impala_stats(False)             # xt_net_set_impala_stats(NULL, NULL): the captured graph is not replayed
    l_on, l_never = run_train(on), run_train(never)
    assert on.train_stats() is None
    assert np.float32(l_on).tobytes() == np.float32(l_never).tobytes() and same_bits(state_of(on), state_of(never))
    on.net.set_impala_stats(True)              # back on: the sums are those of one train again
    run_train(on)
    assert on.train_stats()["transitions"] == 90.0
    # a data-parallel tail or an exchange hook first: refused, with a message ...
    net = never.net
    hook = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p)(
        lambda g, n, u, s: 0)
    hook_p = ctypes.cast(hook, ctypes.c_void_p)
    net.set_dp(0, 1)
    with pytest.raises(RuntimeError, match="data-parallel"):
        net.set_impala_stats(True)
    net.set_dp(0, 0)
    assert net.lib.xt_net_set_grad_exchange(net.handle, hook_p, None) == 0
    with pytest.raises(RuntimeError, match="exchange hook"):
        net.set_impala_stats(True)
    assert net.lib.xt_net_set_grad_exchange(net.handle, None, None) == 0
    assert not net.impala_stats_on
    # ... and the other way round: both are refused while the statistics are on
    with pytest.raises(RuntimeError, match="v-trace statistics"):
        on.net.set_dp(0, 1)
    assert on.net.lib.xt_net_set_grad_exchange(on.net.handle, hook_p, None) != 0
    assert b"v-trace statistics" in on.net.lib.xt_last_error()
    run_train(on)                              # (still a plain single-GPU net)
    assert on.train_stats()["chunks"] == 3.0
