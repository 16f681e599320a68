"""Float64 checker of the dueling distributional heads (``dist_dueling``: C51 and QR-DQN on a folded (A + 1) * N wide Q
head) and small callers of their C entries, shared by tests/test_cpu_duel.py and tests/test_gpu_duel.py.

The restatement is the dueling combine ("Dueling distributional heads"), followed by
``dist_helpers.dist_loss_ref`` / ``quant_helpers.quant_loss_ref`` on the combined rows, followed by the combine's transpose;
float64 is the reference, float32 the NumPy restatement whose own deviation from float64 sets the head tests' bars
(``head_bars``).  The networks are ``oracle.nets.ActorCritic`` with ``action_dim = (A + 1) * N``.  Not a test module.
"""
import ctypes
import itertools

import numpy as np

import dist_helpers as D
import dqn_helpers as H
import quant_helpers as Q
from oracle import nets

GAMMA = 0.99
KAPPA = Q.KAPPA
V_MIN, V_MAX = -10.0, 10.0        # the support of the whole-step C51 cases
HEADS = ("c51", "qr")


# ----------------------------------------------------------------------------------------------- arithmetic
def combine(cols, a, n, dtype=np.float64):
    """l[b, a, i] = v[i] + (adv[a, i] - mean_i) of folded rows ``cols`` [B, (A + 1) * N] in ``dtype``; the mean is the sum
    over ascending a, divided by A"""
    c = np.asarray(cols, dtype).reshape(-1, a + 1, n)
    s = np.zeros((c.shape[0], n), dtype)
    for k in range(a):
        s = s + c[:, k]
    mean = s / np.dtype(dtype).type(a)
    return c[:, a:a + 1] + (c[:, :a] - mean[:, None, :])


def combine_transpose(dl, a, n):
    """the transpose of ``combine`` on any gradient ``dl`` [B, A * N] w.r.t. l: dadv[a, i] = dl[a, i] - (1 / A) sum_a'
    dl[a', i], dv[i] = sum_a dl[a, i] (float64) -> [B, (A + 1) * N]"""
    g = np.asarray(dl, np.float64).reshape(-1, a, n)
    tot = g.sum(axis=1, keepdims=True)
    return np.concatenate([g - tot / a, tot], axis=1).reshape(len(g), -1)


def combine_grad(dl, act, a, n, dtype=np.float64):
    """the transpose on a gradient that is zero outside the taken action, as the kernels form it: with d_i = dl[act, i],
    dcol[a N + i] = d_i * (hot(a == act) - inv_A), inv_A = 1 / A in ``dtype``, and dcol[A N + i] = d_i"""
    dt = np.dtype(dtype).type
    g = np.asarray(dl, dtype).reshape(-1, a, n)
    d = g[np.arange(len(g)), act]
    hot = (np.arange(a)[None, :] == np.asarray(act).reshape(-1, 1)).astype(dtype)
    adv = d[:, None, :] * (hot - dt(1.0) / dt(a))[:, :, None]
    return np.concatenate([adv, d[:, None, :]], axis=1).reshape(len(g), -1)


def loss_ref(head, logits, t_logits, o_logits, action, reward, disc, done, weights, a, n, dtype=np.float64, v_min=V_MIN,
             v_max=V_MAX, kappa=KAPPA):
    """The dueling head in ``dtype`` on folded rows [B, (A + 1) * N] -> the dict of ``dist_loss_ref`` / ``quant_loss_ref`` on
    the combined rows, plus ``dcols`` [B, (A + 1) * N] (the gradient of the folded row), ``d`` [B, N] (d_i) and ``l`` [B, A, N]
    (the combined online rows)"""
    b = len(logits)
    cm = lambda x: None if x is None else combine(x, a, n, dtype).reshape(b, a * n)
    if head == "c51":
        r = D.dist_loss_ref(cm(logits), cm(t_logits), cm(o_logits), action, reward, disc, done, weights, a, n, v_min, v_max,
                            dtype)
    else:
        r = Q.quant_loss_ref(cm(logits), cm(t_logits), cm(o_logits), action, reward, disc, done, weights, a, n, kappa, dtype)
    r["dcols"] = combine_grad(r["dlogits"], r["act"], a, n, dtype)
    r["d"] = r["dlogits"].reshape(b, a, n)[np.arange(b), r["act"]]
    r["l"] = cm(logits).reshape(b, a, n)
    return r


# ----------------------------------------------------------------------------------------------- the head tests' cases
HEAD_SHAPES = [(1, 1, 2), (7, 2, 51), (33, 6, 51), (5, 18, 64), (5, 3, 65), (3, 2, 256), (257, 2, 4)]     # (B, A, N)
HEAD_VARIANTS = list(itertools.product([False, True], repeat=4))      # double, weighted, disc given, labels through slots
PLANTED = {"c51": D.PLANTED + ("equal_adv",), "qr": Q.PLANTED + ("equal_adv",)}
C51_GAP, QR_GAP = 1e-4, Q.ARGMAX_GAP
# seeds chosen on the CPU so that the float64 restatement's two best picking values of every row that is not a planted tie
# keep the gap dist_helpers / quant_helpers demand (C51: 1e-4 (v_max - v_min) between the two best dist_q; QR: ARGMAX_GAP *
# max(1, the row's largest combined picking-quantile magnitude)) in every variant; tests/test_cpu_duel.py asserts it for
# every case
HEAD_SEEDS = {"c51": {(1, 1, 2): 0, (7, 2, 51): 0, (33, 6, 51): 0, (5, 18, 64): 0, (5, 3, 65): 0, (3, 2, 256): 0,
                      (257, 2, 4): 0},
              "qr": {(1, 1, 2): 0, (7, 2, 51): 0, (33, 6, 51): 0, (5, 18, 64): 0, (5, 3, 65): 0, (3, 2, 256): 0,
                     (257, 2, 4): 0}}


def head_case(head, shape, double, weighted, with_disc, through_slots, seed=None):
    """-> dict of the inputs of one head call on folded rows and ``planted``: name -> row.  The planted rows of
    ``dist_helpers.head_case`` / ``quant_helpers.head_case`` are kept, as many as B - 1 allows and in their order (a tie
    copies the first group into all A + 1; the quantile row that needs |u_ij| = kappa gets advantages x_i + (0.5, -0.5, 0,
    ...)[a] on the 0.5 grid, so that its combined quantiles are the value group's plus a per-action constant, exactly), and
    one more follows them: ``equal_adv``, equal dyadic advantages across the actions on all three nets, so that every mean is
    exact, the combined rows are the value group bit for bit and a* = 0."""
    b, a, n = shape
    seed = HEAD_SEEDS[head][shape] if seed is None else seed
    rng = np.random.default_rng(1000 * seed + 17 * b + a + n + (500 if head == "qr" else 0))
    lg = lambda: (rng.standard_normal((b, (a + 1) * n)) * 1.5).astype(np.float32)
    d = dict(head=head, logits=lg(), t_logits=lg(), o_logits=lg() if double else None, a=a, n=n, gamma=GAMMA)
    if head == "c51":
        d["v_min"], d["v_max"] = D.head_bounds(n)
        span = d["v_max"] - d["v_min"]
        reward = rng.standard_normal(b) * span / 4.0
    else:
        d["kappa"] = KAPPA
        reward = rng.standard_normal(b)
    action = rng.integers(0, a, b).astype(np.int32)
    done = (rng.random(b) < 0.2).astype(np.uint8)
    disc = GAMMA ** rng.integers(1, 4, b).astype(np.float64) if with_disc else None
    nets3 = [k for k in ("logits", "t_logits", "o_logits") if d[k] is not None]

    def equal_adv(row, keys, grid, step=0.0):
        """adv[a, i] = x_i + c_a with x on the 1 / grid grid and c = (step, -step, 0, ...): the offsets sum to zero and every
        sum is exact, so mean_i = x_i and l[a, i] = v[i] + c_a bit for bit (step 0: the combined rows are the value group)"""
        off = np.zeros(a, np.float32)
        if a > 1:
            off[0], off[1] = step, -step
        for key in keys:
            x = np.round(d[key][row, :n] * grid) / grid
            d[key][row, :a * n] = (x[None, :] + off[:, None]).reshape(-1)

    planted = {}
    names = PLANTED[head]
    for row, name in enumerate(names[:max(0, min(b - 1, len(names)))]):
        planted[name] = row
        done[row] = 0
        if name == "done":
            done[row], action[row] = 1, -1
        elif name == "clamp_hi":
            reward[row], action[row] = 10.0 * span, a
        elif name == "clamp_lo":
            reward[row] = -10.0 * span
        elif name == "clamp":
            action[row] = a
        elif name == "integer":
            reward[row] = 0.0
            if with_disc:
                disc[row] = 1.0
        elif name == "zero":
            done[row] = 1
            reward[row] = float(combine(d["logits"][row:row + 1], a, n, np.float32)[0, action[row], n // 2])
        elif name == "kappa":
            for key in ("logits", "t_logits"):
                d[key][row] = np.round(d[key][row] * 2.0) / 2.0
            equal_adv(row, ("logits", "t_logits"), 2.0, 0.5)         # l[a, i] = v[i] + (0.5, -0.5, 0, ...)[a], on the 0.5 grid
            if with_disc:                                   # g = 1 and R on the grid: every T_j on it, and u_00 = kappa
                pick = combine((d["o_logits"] if double else d["t_logits"])[row:row + 1], a, n)[0]
                boot = combine(d["t_logits"][row:row + 1], a, n)[0, int(np.argmax(pick.mean(-1))), 0]
                reward[row] = KAPPA + float(combine(d["logits"][row:row + 1], a, n)[0, action[row], 0]) - float(boot)
                disc[row] = 1.0
            else:                                           # done: every T_j = R = theta_0 + kappa
                done[row] = 1
                reward[row] = float(combine(d["logits"][row:row + 1], a, n, np.float32)[0, action[row], 0]) + KAPPA
        elif name == "tie":
            pick = d["o_logits"] if double else d["t_logits"]
            pick[row] = np.tile(pick[row, :n], a + 1)
        elif name == "equal_adv":
            equal_adv(row, nets3, 4.0)
    d.update(action=action, reward=reward, done=done, disc=disc, planted=planted,
             weights=rng.uniform(0.3, 1.0, b) if weighted else None)
    d["slots"] = rng.permutation(b + 5)[:b].astype(np.int32) if through_slots else None
    return d


def head_ref(c, dtype=np.float64):
    disc = c["disc"] if c["disc"] is not None else np.full(len(c["action"]), c["gamma"], np.float64)
    kw = dict(v_min=c["v_min"], v_max=c["v_max"]) if c["head"] == "c51" else dict(kappa=c["kappa"])
    return loss_ref(c["head"], c["logits"], c["t_logits"], c["o_logits"], c["action"], c["reward"], disc, c["done"],
                    c["weights"], c["a"], c["n"], dtype, **kw)


def ref_gap(head, ref, span=V_MAX - V_MIN, skip=()):
    """smallest gap between the two best picking values of a reference over the rows not in ``skip``, in the measure of the
    head's own helpers (C51: relative to the support's span; QR: ``quant_helpers.pick_gaps``)"""
    if head == "c51":
        q = np.sort(np.asarray(ref["q_pick"], np.float64), axis=1)
        gap = (q[:, -1] - q[:, -2]) / span if q.shape[1] > 1 else np.full(len(q), np.inf)
    else:
        gap = Q.pick_gaps(ref["q_pick"], ref["pick"])
    keep = np.ones(len(gap), bool)
    keep[list(skip)] = False
    return float(gap[keep].min()) if keep.any() else np.inf


def argmax_gap(c, ref):
    """``ref_gap`` of a head case over the rows that are no planted tie (``tie``, ``equal_adv``)"""
    skip = [c["planted"][k] for k in ("tie", "equal_adv") if k in c["planted"]]
    return ref_gap(c["head"], ref, c["v_max"] - c["v_min"] if c["head"] == "c51" else None, skip)


def min_gap(head):
    return C51_GAP if head == "c51" else QR_GAP


HEAD_QUANTITIES = {"c51": ("m", "loss_b", "dcols", "qstar"), "qr": ("loss_b", "dcols", "qstar", "out")}
_BARS = {}


def quantity(ref, k):
    return Q.out_of(ref) if k == "out" else ref[k]


def head_bars(head):
    """-> (measured, bars): per quantity the largest ``rel_max`` deviation of the float32 NumPy restatement from the
    float64 one over every shape and variant of the head test, and four times that (the factor covers libm and
    summation-order differences between NumPy and the device).  Nothing is capped: tests/test_cpu_duel.py asserts that the
    gradient bar stays at or below the project's 1e-5."""
    if head not in _BARS:
        worst = dict.fromkeys(HEAD_QUANTITIES[head], 0.0)
        for shape in HEAD_SHAPES:
            for v in HEAD_VARIANTS:
                c = head_case(head, shape, *v)
                r64, r32 = head_ref(c), head_ref(c, np.float32)
                assert np.array_equal(r64["astar"], r32["astar"])
                for k in worst:
                    worst[k] = max(worst[k], H.rel_max(quantity(r32, k), quantity(r64, k)))
        _BARS[head] = (worst, {k: 4.0 * v for k, v in worst.items()})
    return _BARS[head]


# ----------------------------------------------------------------------------------------------- networks
def spec_pair(head, kind, a, n, hidden=32, noisy=False):
    from xingtian_amd.model import netspec
    atoms, quantiles = (n, 1) if head == "c51" else (1, n)
    if kind == "cnn":
        return (netspec.dqn_cnn((84, 84, 4), a, False, atoms, quantiles, noisy, dist_dueling=True),
                H.oracle_spec("cnn", (84, 84, 4), (a + 1) * n))
    return (netspec.dqn_mlp((4,), a, hidden, 1, False, atoms, quantiles, noisy, dist_dueling=True),
            H.oracle_spec("mlp", (4,), (a + 1) * n, hidden, 1))


class DuelOracle(object):
    """``DQN.train`` of a dueling distributional pair on two ``ActorCritic`` nets (action_dim = (A + 1) * N) in ``dtype``"""

    def __init__(self, head, ospec, params, target_params, a, n, double, lr, clipnorm=None, dtype=np.float64):
        self.net, self.target = nets.ActorCritic(ospec, params, dtype), nets.ActorCritic(ospec, target_params, dtype)
        self.head, self.a, self.n, self.double, self.dtype = head, a, n, double, dtype
        self.opt = nets.AdamKeras(self.net.params, lr, clipnorm)

    def step(self, states, next_states, action, reward, disc, done, weights=None, apply=False):
        tl, _ = self.target.forward(next_states)
        ol = self.net.forward(next_states)[0] if self.double else None
        lg, _ = self.net.forward(states)
        out = loss_ref(self.head, lg, tl, ol, action, reward, disc, done, weights, self.a, self.n, self.dtype)
        out["logits"] = lg
        out["grads"] = self.net.backward(out["dcols"], out["dvalue"].reshape(-1, 1))
        if apply:
            self.opt.apply(self.net.params, out["grads"])
        return out

    def sync_target(self):
        self.target.params = type(self.net.params)((k, v.copy()) for k, v in self.net.params.items())

    def predict(self, obs):
        """Q [B, A] in float64: the expectation / the mean of the combined rows"""
        l = combine(self.net.forward(obs)[0], self.a, self.n)
        if self.head == "qr":
            return l.mean(-1)
        e = np.exp(l - l.max(-1, keepdims=True))
        return (D.support(self.n, V_MIN, V_MAX)[0] * e).sum(-1) / e.sum(-1)


def pick_values(head, cols, a, n):
    """(Q [rows, A], combined rows [rows, A, N]) of folded float64 rows, as the bootstrap action is picked by them"""
    l = combine(cols, a, n)
    if head == "qr":
        return Q.mean_q(l, np.float64), l
    e = np.exp(l - l.max(-1, keepdims=True))
    return (D.support(n, V_MIN, V_MAX)[0] * e).sum(-1) / e.sum(-1), l


def row_gaps(head, cols, a, n):
    """per row: the gap between the two best picking values in the measure ``argmax_gap`` uses (inf with one action)"""
    q, l = pick_values(head, cols, a, n)
    if a < 2:
        return np.full(len(q), np.inf)
    if head == "qr":
        return Q.pick_gaps(q, l)
    s = np.sort(q, axis=1)
    return (s[:, -1] - s[:, -2]) / (V_MAX - V_MIN)


MARGIN = 1e-6                     # distance every ReLU pre-activation of a state row keeps from the kink
CAP, RING_SEED = 50, 11
_RINGS, _OK = {}, {}


def state_fn(kind):
    return Q.state_fn(kind)


def ring_rows(kind, a):
    """-> (msgs, store, cur rows [CAP, ...], next rows [CAP, ...]) of the 50-row ring every whole-step test fills"""
    import nstep_helpers as N
    if (kind, a) not in _RINGS:
        msgs, store = N.make_messages(CAP, RING_SEED, a_dim=a, states=state_fn(kind)), N.BruteStore(CAP)
        for m in msgs:
            store.add(m)
        cur = np.stack([msgs[m]["cur_state"][t] for m, t in store.slot])
        nxt = np.stack([msgs[m]["next_state"][t] for m, t in store.slot])
        _RINGS[(kind, a)] = (msgs, store, cur, nxt)
    return _RINGS[(kind, a)]


def host_labels(kind, a, n_step):
    """-> slots -> (boot, action, reward, disc, done): ``nstep_targets`` on the label rings the store implies"""
    from xingtian_amd.algorithm.dqn.dqn import nstep_targets
    msgs, store, _, _ = ring_rows(kind, a)
    col = lambda k, dt: np.asarray([msgs[m][k][t] for m, t in store.slot], dt)
    follow, action, reward, done = store.follow(), col("action", np.int32), col("reward", np.float64), col("done", np.uint8)
    return lambda s: nstep_targets(s, follow, action, reward, done, GAMMA, n_step, CAP)


def ok_slots(head, kind, a, n, ospec, p_on, p_pick, which, n_step=1):
    """-> the slots whose state row keeps MARGIN from every ReLU kink of the online net and whose bootstrap row keeps twice
    the head's gap between the two best picking values, on the float64 oracle alone: the minibatches are drawn among these.
    ``which`` names the picking parameters for the cache (the seeds are fixed: "online" is seed 1, "target" seed 2); other
    parameters (a noisy net's effective ones) pass None and are not cached."""
    _, _, cur, nxt = ring_rows(kind, a)

    def margins():
        net = nets.ActorCritic(ospec, p_on, np.float64)
        net.forward(cur)
        return np.min([np.abs(z.reshape(CAP, -1)).min(1) for _, _, z in net.cache[0]], axis=0)

    gaps = lambda: row_gaps(head, nets.ActorCritic(ospec, p_pick, np.float64).forward(nxt)[0], a, n)
    if which is None:
        m, g = margins(), gaps()
    else:                                                   # (the online parameters are seed 1 whatever picks)
        if (kind, a, n) not in _OK:
            _OK[(kind, a, n)] = margins()
        if (head, kind, a, n, which) not in _OK:
            _OK[(head, kind, a, n, which)] = gaps()
        m, g = _OK[(kind, a, n)], _OK[(head, kind, a, n, which)]
    boot = np.asarray(host_labels(kind, a, n_step)(np.arange(CAP))[0])
    return np.flatnonzero((m >= MARGIN) & (g[boot] >= 2.0 * min_gap(head))).astype(np.int32)


def assert_step(got_loss, grads, ref, spec, ospec, what=""):
    """the project's standing bars of the whole step: loss 1e-4, every gradient tensor 1e-5 by ``rel_max``"""
    errs = {h: H.rel_max(grads[h], ref["grads"][o]) for h, o in H.name_map(spec, ospec).items()}
    print("duel step", what, "loss", got_loss, float(ref["loss"]), "| gradient tensors", errs)
    assert abs(got_loss - ref["loss"]) <= 1e-4 * max(1.0, abs(ref["loss"])), (got_loss, ref["loss"])
    for h, err in errs.items():
        assert err <= 1e-5, (h, err)
    return errs


# ----------------------------------------------------------------------------------------------- C entries (GPU)
PAD = 2                           # rows of sentinels behind every per-sample output of ``gpu_head``


def gpu_head(c, entry=None, b=None, a=None, n=None, want_m=True):
    """-> (rc, dict of host arrays): the head entry of the case (``xt_dqn_loss_dist_duel`` / ``xt_dqn_loss_quant_duel``, or
    ``entry``: the entries without _duel take the same arguments) on the inputs of ``head_case``.  The outputs start as NaN /
    -1 sentinels and carry PAD rows more than the launch owns (``out``: one float more).  Labels through ``slots`` live in
    rings of B + 5 entries whose unused entries hold NaN / 255 / -7."""
    import torch
    from xingtian_amd import lib as L
    dev = torch.device("cuda:0")
    up = lambda x, dt: None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(dev)
    rb, width = c["logits"].shape
    head = c["head"]
    entry = entry or ("xt_dqn_loss_dist_duel" if head == "c51" else "xt_dqn_loss_quant_duel")
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
    out = dict(dlogits=nan(rb + PAD, width), dvalue=nan(rb + PAD), out=nan(4 + 2 * rb + 1), maxq=nan(rb + PAD),
               m=nan(rb + PAD, c["n"]), astar=torch.full((rb + PAD,), -1, dtype=torch.int32, device=dev))
    front = (L.ptr(d["logits"]), L.ptr(d["tl"]), L.ptr(d["ol"]), rb if b is None else b, c["a"] if a is None else a,
             c["n"] if n is None else n)
    labels = (L.ptr(d["slots"]), L.ptr(d["action"]), L.ptr(d["reward"]), L.ptr(d["done"]), ctypes.c_double(c["gamma"]),
              L.ptr(out["dlogits"]), L.ptr(out["dvalue"]), L.ptr(out["out"]), L.ptr(out["astar"]), L.ptr(out["maxq"]))
    back = (None, L.ptr(d["weights"]), L.ptr(d["disc"]), L.stream_ptr())
    if head == "c51":
        rc = getattr(L.load(), entry)(*front, ctypes.c_double(c["v_min"]), ctypes.c_double(c["v_max"]), *labels,
                                      L.ptr(out["m"]) if want_m else None, *back)
    else:
        rc = getattr(L.load(), entry)(*front, ctypes.c_double(c["kappa"]), *labels, *back)
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in out.items()}


def assert_pads_untouched(got, b):
    """every per-sample output behind row B and the float behind ``out`` kept its sentinel"""
    for k in ("dlogits", "dvalue", "maxq", "m"):
        assert np.isnan(got[k][b:]).all(), k
    assert (got["astar"][b:] == -1).all() and np.isnan(got["out"][4 + 2 * b:]).all() and np.isnan(got["out"][3])
