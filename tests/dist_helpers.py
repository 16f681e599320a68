"""Float64 checker of the distributional (C51) DQN path and small callers of its C entries, shared by
tests/test_cpu_dist.py and tests/test_gpu_dist.py.

``dist_loss_ref`` restates DESIGN.md section 7 ("Distributional head") in a chosen dtype: float64 is the reference, float32
is the NumPy restatement whose own deviation from float64 sets the head test's bars (``head_bars``).  The networks are
``oracle.nets.ActorCritic`` with ``action_dim = A * N``, as tests/dqn_helpers.py builds them with ``A``.
"""
import ctypes
import itertools

import numpy as np

import dqn_helpers as H
from oracle import nets

GAMMA = 0.99


# ----------------------------------------------------------------------------------------------- arithmetic
def support(n, v_min, v_max):
    delta = (np.float64(v_max) - np.float64(v_min)) / np.float64(n - 1)
    return np.float64(v_min) + np.arange(n, dtype=np.float64) * delta, delta


def scatter_projection(p, reward, disc, done, v_min, v_max):
    """The paper's Algorithm 1 as published, in float64: l = floor(b), u = ceil(b), m_l += p (u - b), m_u += p (b - l).
    (It drops the mass of an atom whose b is an integer: the callers avoid those.)"""
    p = np.asarray(p, np.float64)
    b, n = p.shape
    z, delta = support(n, v_min, v_max)
    m = np.zeros((b, n), np.float64)
    for s in range(b):
        for j in range(n):
            tz = float(reward[s]) if done[s] else float(reward[s]) + float(disc[s]) * z[j]
            bj = (min(max(tz, float(v_min)), float(v_max)) - float(v_min)) / delta
            l, u = int(np.floor(bj)), int(np.ceil(bj))
            m[s, l] += p[s, j] * (u - bj)
            m[s, u] += p[s, j] * (bj - l)
    return m


def dist_loss_ref(logits, t_logits, o_logits, action, reward, disc, done, weights, a, n, v_min, v_max, dtype=np.float64):
    """The head in ``dtype`` (the projection's sum is float64 either way, rounded once to ``dtype``).  logits [B, A * N];
    disc float64 [B]; weights float64 [B] or None.
    -> dict(q_pick [B,A], astar, qstar, p, m, loss_b, loss, mean_loss, mean_q, dlogits [B, A*N], dvalue [B])"""
    dt = np.dtype(dtype).type
    b = logits.shape[0]
    rows = np.arange(b)
    z, delta = support(n, v_min, v_max)
    zt = z.astype(dtype)

    def soft(l):
        l = np.asarray(l, dtype).reshape(b, a, n)
        e = np.exp(l - l.max(axis=2, keepdims=True))
        return l, e

    def q_of(e):
        return (zt * e).sum(axis=2, dtype=dtype) / e.sum(axis=2, dtype=dtype)
    _, et = soft(t_logits)
    qt = q_of(et)
    q_pick = qt if o_logits is None else q_of(soft(o_logits)[1])
    astar = np.argmax(q_pick, axis=1)
    qstar = qt[rows, astar]
    es = et[rows, astar]
    p = es / es.sum(axis=1, keepdims=True, dtype=dtype)
    r = np.asarray(reward, np.float64).reshape(b, 1)
    g = np.asarray(disc, np.float64).reshape(b, 1)
    dn = np.asarray(done).reshape(b, 1).astype(bool)
    tz = np.clip(np.where(dn, r, r + g * z[None, :]), np.float64(v_min), np.float64(v_max))
    bj = (tz - np.float64(v_min)) / delta
    idx = np.arange(n, dtype=np.float64)
    m64 = np.zeros((b, n), np.float64)
    for j in range(n):
        m64 = m64 + p[:, j:j + 1].astype(np.float64) * np.maximum(0.0, 1.0 - np.abs(bj[:, j:j + 1] - idx[None, :]))
    m = m64.astype(dtype)
    act = np.clip(np.asarray(action).reshape(b).astype(np.int64), 0, a - 1)
    l, _ = soft(logits)
    la = l[rows, act]
    mx = la.max(axis=1, keepdims=True)
    logq = (la - mx) - np.log(np.exp(la - mx).sum(axis=1, keepdims=True, dtype=dtype))
    loss_b = -(m * logq).sum(axis=1, dtype=dtype)
    mass = m.sum(axis=1, keepdims=True, dtype=dtype)
    w = np.ones(b, dtype) if weights is None else np.asarray(weights, np.float64).astype(np.float32).astype(dtype)
    dl = np.zeros((b, a, n), dtype)
    dl[rows, act] = w[:, None] * (np.exp(logq) * mass - m) / dt(b)
    return dict(q_pick=q_pick, astar=astar, qstar=qstar, p=p, m=m, loss_b=loss_b,
                loss=(w.astype(np.float64) * loss_b.astype(np.float64)).sum() / b, mean_loss=loss_b.astype(np.float64).mean(),
                mean_q=qstar.astype(np.float64).mean(), dlogits=dl.reshape(b, a * n), dvalue=np.zeros(b, dtype), act=act)


# ----------------------------------------------------------------------------------------------- the head test's cases
HEAD_SHAPES = [(1, 1, 2), (7, 2, 51), (33, 6, 51), (5, 18, 64), (5, 3, 65), (3, 2, 256), (257, 2, 4)]
HEAD_VARIANTS = list(itertools.product([False, True], repeat=4))      # double, weighted, disc given, labels through slots
PLANTED = ("done", "clamp_hi", "clamp_lo", "integer", "tie")
# seeds chosen on the CPU so that the float64 restatement's two best dist_q of every row that is not the planted tie keep
# 1e-4 (v_max - v_min) apart, in the plain and the double form (tests/test_cpu_dist.py asserts it for every case)
HEAD_SEEDS = {(1, 1, 2): 0, (7, 2, 51): 0, (33, 6, 51): 0, (5, 18, 64): 0, (5, 3, 65): 1, (3, 2, 256): 0, (257, 2, 4): 0}


def head_bounds(n):
    """delta = 0.5 exactly, so every z_j and, with g = 1 and R = 0, every b_j is exact: the all-integer row gives m == p"""
    return -(n - 1) / 4.0, (n - 1) / 4.0


def head_case(shape, double, weighted, with_disc, through_slots):
    """-> dict of the inputs of one head call and ``planted``: name -> row.  Planted rows, as many as B - 1 allows, in this
    order: done (taken action -1), clamp at v_max (taken action A), clamp at v_min, all b_j integers (only with a
    per-sample discount, which is 1 there), every action's picking logits identical (the first index wins)."""
    b, a, n = shape
    v_min, v_max = head_bounds(n)
    rng = np.random.default_rng(1000 * HEAD_SEEDS[shape] + 17 * b + a + n)
    lg = lambda: (rng.standard_normal((b, a * n)) * 1.5).astype(np.float32)
    d = dict(logits=lg(), t_logits=lg(), o_logits=lg() if double else None, a=a, n=n, v_min=v_min, v_max=v_max, gamma=GAMMA)
    span = v_max - v_min
    action = rng.integers(0, a, b).astype(np.int32)
    reward = rng.standard_normal(b) * span / 4.0
    done = (rng.random(b) < 0.2).astype(np.uint8)
    disc = GAMMA ** rng.integers(1, 4, b).astype(np.float64) if with_disc else None
    planted = {}
    for row, name in enumerate(PLANTED[:max(0, min(b - 1, len(PLANTED)))]):
        planted[name] = row
        done[row] = 0
        if name == "done":
            done[row], action[row] = 1, -1
        elif name == "clamp_hi":
            reward[row], action[row] = 10.0 * span, a
        elif name == "clamp_lo":
            reward[row] = -10.0 * span
        elif name == "integer":
            reward[row] = 0.0
            if with_disc:
                disc[row] = 1.0
        elif name == "tie":
            pick = d["o_logits"] if double else d["t_logits"]
            pick[row] = np.tile(pick[row, :n], a)
    d.update(action=action, reward=reward, done=done, disc=disc, planted=planted,
             weights=rng.uniform(0.3, 1.0, b) if weighted else None)
    d["slots"] = rng.permutation(b + 5)[:b].astype(np.int32) if through_slots else None
    return d


def head_ref(c, dtype=np.float64):
    disc = c["disc"] if c["disc"] is not None else np.full(len(c["action"]), c["gamma"], np.float64)
    return dist_loss_ref(c["logits"], c["t_logits"], c["o_logits"], c["action"], c["reward"], disc, c["done"], c["weights"],
                         c["a"], c["n"], c["v_min"], c["v_max"], dtype)


HEAD_QUANTITIES = ("m", "loss_b", "dlogits", "qstar")
_BARS = {}


def head_bars():
    """-> (measured, bars): per quantity the largest ``rel_max`` deviation of the float32 NumPy restatement from the
    float64 one over every shape and variant of the head test, and four times that (the factor covers libm and
    summation-order differences between NumPy and the device).  The gradient bar is capped at the project's 1e-5."""
    if not _BARS:
        worst = dict.fromkeys(HEAD_QUANTITIES, 0.0)
        for shape in HEAD_SHAPES:
            for v in HEAD_VARIANTS:
                c = head_case(shape, *v)
                r64, r32 = head_ref(c), head_ref(c, np.float32)
                assert np.array_equal(r64["astar"], r32["astar"])
                for k in HEAD_QUANTITIES:
                    worst[k] = max(worst[k], H.rel_max(r32[k], r64[k]))
        _BARS["measured"] = worst
        _BARS["bars"] = {k: 4.0 * v for k, v in worst.items()}
        _BARS["bars"]["dlogits"] = min(_BARS["bars"]["dlogits"], 1e-5)
    return _BARS["measured"], _BARS["bars"]


def argmax_gap(ref, planted, span):
    """smallest gap between the two best picking dist_q over the rows that are not the planted tie, relative to ``span``"""
    q = np.sort(np.asarray(ref["q_pick"], np.float64), axis=1)
    if q.shape[1] < 2:
        return np.inf
    gap = q[:, -1] - q[:, -2]
    keep = np.ones(len(gap), bool)
    if "tie" in planted:
        keep[planted["tie"]] = False
    return float(gap[keep].min() / span) if keep.any() else np.inf


# ----------------------------------------------------------------------------------------------- networks
def spec_pair(kind, a, n, hidden=32):
    from xingtian_amd.model import netspec
    if kind == "cnn":
        return netspec.dqn_cnn((84, 84, 4), a, False, n), H.oracle_spec("cnn", (84, 84, 4), a * n)
    return netspec.dqn_mlp((4,), a, hidden, 1, False, n), H.oracle_spec("mlp", (4,), a * n, hidden, 1)


class DistOracle(object):
    """``DQN.train`` of a distributional pair on two ``ActorCritic`` nets (action_dim = A * N) in ``dtype``."""

    def __init__(self, ospec, params, target_params, a, n, v_min, v_max, double, lr, clipnorm=None, dtype=np.float64):
        self.net, self.target = nets.ActorCritic(ospec, params, dtype), nets.ActorCritic(ospec, target_params, dtype)
        self.a, self.n, self.v_min, self.v_max, self.double, self.dtype = a, n, v_min, v_max, double, dtype
        self.opt = nets.AdamKeras(self.net.params, lr, clipnorm)

    def step(self, states, next_states, action, reward, disc, done, weights=None, apply=False):
        tl, _ = self.target.forward(next_states)
        ol = self.net.forward(next_states)[0] if self.double else None
        lg, _ = self.net.forward(states)
        out = dist_loss_ref(lg, tl, ol, action, reward, disc, done, weights, self.a, self.n, self.v_min, self.v_max,
                            self.dtype)
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
    print("dist step", what, "loss", got_loss, float(ref["loss"]), "| gradient tensors", errs)
    assert abs(got_loss - ref["loss"]) <= 1e-4 * max(1.0, abs(ref["loss"])), (got_loss, ref["loss"])
    for h, err in errs.items():
        assert err <= 1e-5, (h, err)


# ----------------------------------------------------------------------------------------------- C entries (GPU)
def gpu_dqn_loss_dist(c, b=None, a=None, n=None, v_min=None, v_max=None, want_m=True):
    """-> (rc, dict of host arrays): xt_dqn_loss_dist on the inputs of ``head_case``; outputs start as NaN / -1 sentinels.
    Labels through ``slots`` live in rings of B + 5 entries whose unused entries hold NaN / 255 / -7."""
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
    out = dict(dlogits=nan(rb, width), dvalue=nan(rb), out=nan(4 + 2 * rb), maxq=nan(rb), m=nan(rb, c["n"]),
               astar=torch.full((rb,), -1, dtype=torch.int32, device=dev))
    rc = L.load().xt_dqn_loss_dist(
        L.ptr(d["logits"]), L.ptr(d["tl"]), L.ptr(d["ol"]), rb if b is None else b, c["a"] if a is None else a,
        c["n"] if n is None else n, ctypes.c_double(c["v_min"] if v_min is None else v_min),
        ctypes.c_double(c["v_max"] if v_max is None else v_max), L.ptr(d["slots"]), L.ptr(d["action"]), L.ptr(d["reward"]),
        L.ptr(d["done"]), ctypes.c_double(c["gamma"]), L.ptr(out["dlogits"]), L.ptr(out["dvalue"]), L.ptr(out["out"]),
        L.ptr(out["astar"]), L.ptr(out["maxq"]), L.ptr(out["m"]) if want_m else None, None, L.ptr(d["weights"]),
        L.ptr(d["disc"]), L.stream_ptr())
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in out.items()}
