"""Float64 checker of the quantile-regression (QR-DQN) path and small callers of its C entries, shared by
tests/test_cpu_quant.py and tests/test_gpu_quant.py.

``quant_loss_ref`` restates DESIGN.md section 7 ("Quantile head") in a chosen dtype: float64 is the reference, float32 is
the NumPy restatement whose own deviation from float64 sets the head test's bars (``head_bars``).  T_j and the row sums
keep their defined float64-with-one-rounding in both dtypes, so the sign of every u_ij is the same in both.  The networks
are ``oracle.nets.ActorCritic`` with ``action_dim = A * N``, as tests/dist_helpers.py builds them.
"""
import ctypes
import itertools

import numpy as np

import dqn_helpers as H
from oracle import nets

GAMMA = 0.99
KAPPA = 1.0


# ----------------------------------------------------------------------------------------------- arithmetic
def midpoints(n):
    return (2.0 * np.arange(n, dtype=np.float64) + 1.0) / (2.0 * np.float64(n))


def mean_q(theta, dtype):
    """quant_q over the last axis in ``dtype``: the float64 sum over ascending i, divided by N, rounded once to ``dtype``"""
    s = np.zeros(theta.shape[:-1], np.float64)
    for i in range(theta.shape[-1]):
        s = s + theta[..., i].astype(np.float64)
    return (s / np.float64(theta.shape[-1])).astype(dtype)


def quant_loss_ref(logits, t_logits, o_logits, action, reward, disc, done, weights, a, n, kappa, dtype=np.float64):
    """The head in ``dtype``.  logits [B, A * N], taken into ``dtype`` as they come; disc float64 [B]; weights float64 [B]
    or None.  -> dict(q_pick [B,A], pick [B,A,N], astar, qstar, target [B,N], r [B,N], g [B,N], loss_b, loss, mean_loss,
    mean_q, dlogits [B, A*N], dvalue [B], act)"""
    dt = np.dtype(dtype).type
    b = logits.shape[0]
    rows = np.arange(b)
    k = dt(np.float32(kappa))
    half = dt(0.5)
    th_all = np.asarray(logits, dtype).reshape(b, a, n)
    tt_all = np.asarray(t_logits, dtype).reshape(b, a, n)
    pick = tt_all if o_logits is None else np.asarray(o_logits, dtype).reshape(b, a, n)
    qt = mean_q(tt_all, dtype)
    q_pick = qt if o_logits is None else mean_q(pick, dtype)
    astar = np.argmax(q_pick, axis=1)
    qstar = qt[rows, astar]
    tt = tt_all[rows, astar].astype(np.float64)
    r = np.asarray(reward, np.float64).reshape(b, 1)
    g = np.asarray(disc, np.float64).reshape(b, 1)
    dn = np.asarray(done).reshape(b, 1).astype(bool)
    gt = g * tt
    target = np.where(dn, r, r + gt).astype(np.float32).astype(dtype)          # one rounding, to float32, either way
    act = np.clip(np.asarray(action).reshape(b).astype(np.int64), 0, a - 1)
    th = th_all[rows, act]
    tau = midpoints(n)
    w_neg, w_pos = (1.0 - tau).astype(dtype)[None, :], tau.astype(dtype)[None, :]
    sr, sg = np.zeros((b, n), np.float64), np.zeros((b, n), np.float64)
    for j in range(n):
        u = target[:, j:j + 1] - th
        wt = np.where(u < 0, w_neg, w_pos)
        au = np.abs(u)
        hub = np.where(au <= k, half * u * u, k * (au - half * k))
        sr = sr + (wt * hub / k).astype(np.float64)
        sg = sg + (wt * np.clip(u, -k, k) / k).astype(np.float64)
    r_i, g_i = (sr / np.float64(n)).astype(dtype), (-sg / np.float64(n)).astype(dtype)
    loss_b = r_i.sum(axis=1, dtype=dtype)
    w = np.ones(b, dtype) if weights is None else np.asarray(weights, np.float64).astype(np.float32).astype(dtype)
    dl = np.zeros((b, a, n), dtype)
    dl[rows, act] = w[:, None] * g_i / dt(b)
    return dict(q_pick=q_pick, pick=pick, astar=astar, qstar=qstar, target=target, r=r_i, g=g_i, loss_b=loss_b,
                loss=(w.astype(np.float64) * loss_b.astype(np.float64)).sum() / b, mean_loss=loss_b.astype(np.float64).mean(),
                mean_q=qstar.astype(np.float64).mean(), dlogits=dl.reshape(b, a * n), dvalue=np.zeros(b, dtype), act=act)


# ----------------------------------------------------------------------------------------------- the head test's cases
HEAD_SHAPES = [(1, 1, 2), (7, 2, 32), (33, 6, 51), (5, 18, 64), (5, 3, 65), (3, 2, 256), (257, 2, 4)]
HEAD_VARIANTS = list(itertools.product([False, True], repeat=4))      # double, weighted, disc given, labels through slots
PLANTED = ("done", "clamp", "zero", "kappa", "tie")
ARGMAX_GAP = 1e-4
# seeds chosen on the CPU so that the float64 restatement's two best quant_q of every row that is not the planted tie keep
# ARGMAX_GAP * max(1, the row's largest picking-quantile magnitude) apart in every variant (tests/test_cpu_quant.py
# asserts it for every case)
HEAD_SEEDS = {(1, 1, 2): 0, (7, 2, 32): 0, (33, 6, 51): 0, (5, 18, 64): 0, (5, 3, 65): 0, (3, 2, 256): 0, (257, 2, 4): 1}


def head_case(shape, double, weighted, with_disc, through_slots):
    """-> dict of the inputs of one head call and ``planted``: name -> row.  Planted rows, as many as B - 1 allows, in this
    order: done (taken action -1); taken action A (clamped); a done row whose R is one of the taken action's quantiles
    (u_ij exactly 0 for that i); a row whose online and target quantiles lie on a 0.5 grid with T_j on it too (kappa = 1:
    |u_ij| exactly kappa for some i, j); every action's picking quantiles identical (the first index wins)."""
    b, a, n = shape
    rng = np.random.default_rng(1000 * HEAD_SEEDS[shape] + 17 * b + a + n)
    lg = lambda: (rng.standard_normal((b, a * n)) * 1.5).astype(np.float32)
    d = dict(logits=lg(), t_logits=lg(), o_logits=lg() if double else None, a=a, n=n, kappa=KAPPA, gamma=GAMMA)
    action = rng.integers(0, a, b).astype(np.int32)
    reward = rng.standard_normal(b)
    done = (rng.random(b) < 0.2).astype(np.uint8)
    disc = GAMMA ** rng.integers(1, 4, b).astype(np.float64) if with_disc else None
    planted = {}
    for row, name in enumerate(PLANTED[:max(0, min(b - 1, len(PLANTED)))]):
        planted[name] = row
        done[row] = 0
        if name == "done":
            done[row], action[row] = 1, -1
        elif name == "clamp":
            action[row] = a
        elif name == "zero":
            done[row] = 1
            reward[row] = float(d["logits"].reshape(b, a, n)[row, action[row], n // 2])
        elif name == "kappa":
            for key in ("logits", "t_logits"):
                d[key][row] = np.round(d[key][row] * 2.0) / 2.0
            if with_disc:                                   # g = 1, R = 0.5: every T_j on the grid
                reward[row], disc[row] = 0.5, 1.0
            else:                                           # done: every T_j = R = theta_0 + kappa
                done[row] = 1
                reward[row] = float(d["logits"].reshape(b, a, n)[row, action[row], 0]) + KAPPA
        elif name == "tie":
            pick = d["o_logits"] if double else d["t_logits"]
            pick[row] = np.tile(pick[row, :n], a)
    d.update(action=action, reward=reward, done=done, disc=disc, planted=planted,
             weights=rng.uniform(0.3, 1.0, b) if weighted else None)
    d["slots"] = rng.permutation(b + 5)[:b].astype(np.int32) if through_slots else None
    return d


def head_ref(c, dtype=np.float64):
    disc = c["disc"] if c["disc"] is not None else np.full(len(c["action"]), c["gamma"], np.float64)
    return quant_loss_ref(c["logits"], c["t_logits"], c["o_logits"], c["action"], c["reward"], disc, c["done"], c["weights"],
                          c["a"], c["n"], c["kappa"], dtype)


def out_of(ref):
    return np.array([ref["loss"], ref["mean_loss"], ref["mean_q"]], np.float64)


def u_matrix(c, ref, row):
    """u_ij [N, N] (float64 of the float32 operands) of one row of a case: T_j - theta_i"""
    b, a, n = len(c["action"]), c["a"], c["n"]
    th = c["logits"].reshape(b, a, n)[row, ref["act"][row]].astype(np.float64)
    return ref["target"][row].astype(np.float64)[None, :] - th[:, None]


HEAD_QUANTITIES = ("loss_b", "dlogits", "qstar", "out")
_BARS = {}


def head_bars():
    """-> (measured, bars): per quantity the largest ``rel_max`` deviation of the float32 NumPy restatement from the
    float64 one over every shape and variant of the head test, and four times that (the factor covers summation-order
    differences between NumPy and the device).  The gradient bar is capped at the project's 1e-5."""
    if not _BARS:
        worst = dict.fromkeys(HEAD_QUANTITIES, 0.0)
        for shape in HEAD_SHAPES:
            for v in HEAD_VARIANTS:
                c = head_case(shape, *v)
                r64, r32 = head_ref(c), head_ref(c, np.float32)
                assert np.array_equal(r64["astar"], r32["astar"])
                for k in HEAD_QUANTITIES:
                    e = H.rel_max(out_of(r32), out_of(r64)) if k == "out" else H.rel_max(r32[k], r64[k])
                    worst[k] = max(worst[k], e)
        _BARS["measured"] = worst
        _BARS["bars"] = {k: 4.0 * v for k, v in worst.items()}
        _BARS["bars"]["dlogits"] = min(_BARS["bars"]["dlogits"], 1e-5)
    return _BARS["measured"], _BARS["bars"]


def pick_gaps(q_pick, pick_theta):
    """per row: the gap between the two best picking quant_q over max(1, the row's largest picking-quantile magnitude)"""
    q = np.sort(np.asarray(q_pick, np.float64), axis=1)
    if q.shape[1] < 2:
        return np.full(len(q), np.inf)
    scale = np.maximum(1.0, np.abs(np.asarray(pick_theta, np.float64)).reshape(len(q), -1).max(axis=1))
    return (q[:, -1] - q[:, -2]) / scale


def argmax_gap(ref, planted):
    """smallest ``pick_gaps`` of a reference over the rows that are not the planted tie"""
    gap = pick_gaps(ref["q_pick"], ref["pick"])
    keep = np.ones(len(gap), bool)
    if "tie" in planted:
        keep[planted["tie"]] = False
    return float(gap[keep].min()) if keep.any() else np.inf


# ----------------------------------------------------------------------------------------------- networks and the ring
CAP = 50
MARGIN = 1e-6                     # distance every ReLU pre-activation of a state row keeps from the kink
RING_SEED = 11                    # the 50-row ring's messages (tests/nstep_helpers.make_messages)
BATCH = 32
STEP_VARIANTS = {"plain": (False, 1, False), "double": (False, 1, True), "per": (True, 1, False), "nstep": (False, 3, False),
                 "per_nstep": (True, 3, False)}                        # prioritised, n_step, double
# kind, A, N, variant of the whole-step tests
STEP_CASES = ([("mlp", 2, n, v) for n in (8, 51) for v in STEP_VARIANTS] + [("cnn", 4, 51, "plain"), ("cnn", 4, 51, "per_nstep")])


def spec_pair(kind, a, n, hidden=32):
    from xingtian_amd.model import netspec
    if kind == "cnn":
        return netspec.dqn_cnn((84, 84, 4), a, False, 1, n), H.oracle_spec("cnn", (84, 84, 4), a * n)
    return netspec.dqn_mlp((4,), a, hidden, 1, False, 1, n), H.oracle_spec("mlp", (4,), a * n, hidden, 1)


def state_fn(kind):
    if kind == "cnn":
        return lambda tags, nxt: np.random.default_rng(int(tags[0]) * 2 + nxt).integers(
            0, 256, (len(tags), 84, 84, 4), dtype=np.uint8)
    return lambda tags, nxt: np.random.default_rng(int(tags[0]) * 2 + nxt).standard_normal((len(tags), 4)).astype(np.float32)


_RINGS, _MARGINS, _GAPS = {}, {}, {}


def ring_rows(kind, a_dim=2):
    """-> (msgs, store) of the 50-row ring every whole-step test fills (host side only)"""
    import nstep_helpers as N
    if (kind, a_dim) not in _RINGS:
        msgs, store = N.make_messages(CAP, RING_SEED, a_dim=a_dim, states=state_fn(kind)), N.BruteStore(CAP)
        for m in msgs:
            store.add(m)
        _RINGS[(kind, a_dim)] = (msgs, store)
    return _RINGS[(kind, a_dim)]


def host_labels(kind, a_dim, n_step):
    """-> slots -> (boot, action, reward, disc, done): ``nstep_targets`` on the label rings the store implies"""
    from xingtian_amd.algorithm.dqn.dqn import nstep_targets
    msgs, store = ring_rows(kind, a_dim)
    col = lambda k, dt: np.asarray([msgs[m][k][t] for m, t in store.slot], dt)
    follow, action, reward, done = store.follow(), col("action", np.int32), col("reward", np.float64), col("done", np.uint8)
    return lambda s: nstep_targets(s, follow, action, reward, done, GAMMA, n_step, CAP)


def step_setup(kind, a, n, variant):
    """-> dict(spec, ospec, p_on, p_tg, ok): the nets' seeded parameters and the eligible slots of one whole-step case, from
    the float64 oracle alone"""
    prioritised, n_step, double = STEP_VARIANTS[variant]
    spec, ospec = spec_pair(kind, a, n)
    p_on, p_tg = H.seeded_params(ospec, 1, False), H.seeded_params(ospec, 2, False)
    labels = host_labels(kind, a, n_step)
    ok = ok_slots(kind, a, n, ospec, p_on, p_on if double else p_tg, "online" if double else "target",
                  lambda s: labels(s)[0])
    return dict(spec=spec, ospec=ospec, p_on=p_on, p_tg=p_tg, ok=ok, prioritised=prioritised, n_step=n_step, double=double)


def kink_margins(kind, a, n, ospec, p_on):
    """slot -> the smallest |pre-activation| of any ReLU unit in the float64 forward of the online net on that slot's
    state row (a unit closer to zero than float32's accumulation error may come out on the other side of the kink in any
    float32 implementation, tests/test_gpu_nstep.py)"""
    if (kind, a, n) not in _MARGINS:
        msgs, store = ring_rows(kind)
        net = nets.ActorCritic(ospec, p_on, np.float64)
        net.forward(np.stack([msgs[m]["cur_state"][t] for m, t in store.slot]))
        _MARGINS[(kind, a, n)] = np.min([np.abs(z.reshape(CAP, -1)).min(1) for _, _, z in net.cache[0]], axis=0)
    return _MARGINS[(kind, a, n)]


def ring_gaps(kind, a, n, ospec, p_pick, which):
    """slot -> ``pick_gaps`` of the picking net (float64) on that slot's next-state row.  ``which`` names the parameter
    set (the seeds are fixed: "online" is seed 1, "target" seed 2) for the cache."""
    key = (kind, a, n, which)
    if key not in _GAPS:
        msgs, store = ring_rows(kind)
        lg, _ = nets.ActorCritic(ospec, p_pick, np.float64).forward(np.stack([msgs[m]["next_state"][t] for m, t in store.slot]))
        _GAPS[key] = pick_gaps(mean_q(lg.reshape(CAP, a, n), np.float64), lg)
    return _GAPS[key]


def ok_slots(kind, a, n, ospec, p_on, p_pick, which, boot_of=lambda s: s):
    """-> the slots whose state row keeps MARGIN from the kink and whose bootstrap row keeps twice ARGMAX_GAP between the two
    best quant_q of the picking net: the minibatches are drawn among these"""
    margins, gaps = kink_margins(kind, a, n, ospec, p_on), ring_gaps(kind, a, n, ospec, p_pick, which)
    every = np.arange(CAP)
    return np.flatnonzero((margins >= MARGIN) & (gaps[np.asarray(boot_of(every))] >= 2.0 * ARGMAX_GAP)).astype(np.int32)


class QuantOracle(object):
    """``DQN.train`` of a quantile pair on two ``ActorCritic`` nets (action_dim = A * N) in ``dtype``."""

    def __init__(self, ospec, params, target_params, a, n, kappa, double, lr, clipnorm=None, dtype=np.float64):
        self.net, self.target = nets.ActorCritic(ospec, params, dtype), nets.ActorCritic(ospec, target_params, dtype)
        self.a, self.n, self.kappa, self.double, self.dtype = a, n, kappa, double, dtype
        self.opt = nets.AdamKeras(self.net.params, lr, clipnorm)

    def step(self, states, next_states, action, reward, disc, done, weights=None, apply=False):
        tl, _ = self.target.forward(next_states)
        ol = self.net.forward(next_states)[0] if self.double else None
        lg, _ = self.net.forward(states)
        out = quant_loss_ref(lg, tl, ol, action, reward, disc, done, weights, self.a, self.n, self.kappa, self.dtype)
        out["logits"] = lg
        out["grads"] = self.net.backward(out["dlogits"], out["dvalue"].reshape(-1, 1))
        if apply:
            self.opt.apply(self.net.params, out["grads"])
        return out

    def sync_target(self):
        self.target.params = type(self.net.params)((k, v.copy()) for k, v in self.net.params.items())


def assert_step(got_loss, grads, ref, spec, ospec, what=""):
    """the project's standing bars of the whole step: loss 1e-4, every gradient tensor 1e-5 by ``rel_max``"""
    errs = {h: H.rel_max(grads[h], ref["grads"][o]) for h, o in H.name_map(spec, ospec).items()}
    print("quant step", what, "loss", got_loss, float(ref["loss"]), "| gradient tensors", errs)
    assert abs(got_loss - ref["loss"]) <= 1e-4 * max(1.0, abs(ref["loss"])), (got_loss, ref["loss"])
    for h, err in errs.items():
        assert err <= 1e-5, (h, err)


# ----------------------------------------------------------------------------------------------- C entries (GPU)
def gpu_dqn_loss_quant(c, b=None, a=None, n=None, kappa=None, misalign_out=False):
    """-> (rc, dict of host arrays): xt_dqn_loss_quant on the inputs of ``head_case``; outputs start as NaN / -1 sentinels.
    Labels through ``slots`` live in rings of B + 5 entries whose unused entries hold NaN / 255 / -7.  ``out`` carries one
    float more than the launch owns; ``misalign_out`` passes it from its second float on (4-byte aligned only)."""
    import torch
    from xingtian_amd import lib as L
    dev = torch.device("cuda:0")
    up = lambda x, dt: None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(dev)
    rb, width = c["logits"].shape
    action, reward, done = c["action"], c["reward"], c["done"]
    if c["slots"] is not None:
        def ring(x, fill):
            r = np.full(rb + 5, fill, x.dtype)
            r[c["slots"]] = x
            return r
        action, reward, done = ring(action, -7), ring(reward, np.nan), ring(done, 255)
    d = dict(logits=up(c["logits"], np.float32), tl=up(c["t_logits"], np.float32), ol=up(c["o_logits"], np.float32),
             action=up(action, np.int32), reward=up(reward, np.float64), done=up(done, np.uint8),
             slots=up(c["slots"], np.int32), weights=up(c["weights"], np.float64), disc=up(c["disc"], np.float64))
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=dev)
    out = dict(dlogits=nan(rb, width), dvalue=nan(rb), out=nan(4 + 2 * rb + 1), maxq=nan(rb),
               astar=torch.full((rb,), -1, dtype=torch.int32, device=dev))
    out_ptr = ctypes.c_void_p(out["out"].data_ptr() + (4 if misalign_out else 0))
    rc = L.load().xt_dqn_loss_quant(
        L.ptr(d["logits"]), L.ptr(d["tl"]), L.ptr(d["ol"]), rb if b is None else b, c["a"] if a is None else a,
        c["n"] if n is None else n, ctypes.c_double(c["kappa"] if kappa is None else kappa), L.ptr(d["slots"]),
        L.ptr(d["action"]), L.ptr(d["reward"]), L.ptr(d["done"]), ctypes.c_double(c["gamma"]), L.ptr(out["dlogits"]),
        L.ptr(out["dvalue"]), out_ptr, L.ptr(out["astar"]), L.ptr(out["maxq"]), None, L.ptr(d["weights"]), L.ptr(d["disc"]),
        L.stream_ptr())
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in out.items()}
