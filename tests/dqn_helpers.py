"""Float64 checker of the DQN path and small callers of its C entries, shared by tests/test_cpu_dqn.py and
tests/test_gpu_dqn.py.

The networks are ``oracle.nets.ActorCritic`` on ``impala_cnn_spec`` / ``impala_mlp_spec``: their trunks and two heads
([F,A]+[A] and [F]+[1]) are the DQN networks' (the A-wide head is the Q / advantage stream, the 1-wide head the dueling
stream; without dueling it is zero and stays zero).  Names map positionally onto the Keras names of ``netspec.dqn_*``.
"""
import ctypes
from collections import OrderedDict

import numpy as np

from oracle import nets


# ----------------------------------------------------------------------------------------------- arithmetic
def q_from_heads(logits, value, dueling):
    """Q [B, A]: the A-wide head, or s + (l - mean_a l) with the 1-wide head s."""
    if not dueling:
        return logits
    return np.asarray(value).reshape(-1, 1) + (logits - logits.mean(axis=1, keepdims=True))


def dqn_loss_ref(logits, value, t_logits, t_value, o_logits, o_value, action, reward, done, gamma, dueling, weights=None,
                 disc=None):
    """TD target and 'mse' head in the dtype of ``logits``.  o_logits None: plain DQN, else double DQN.  ``weights`` [B]:
    Keras ``sample_weight`` (L = sum_b w_b delta_b^2 / (B A), the head gradients scaled by w_b; the means of |delta| and
    of the bootstrap value stay unweighted).  ``disc`` [B]: a per-sample discount in gamma's place.  The weighted
    arithmetic runs in the kernel's order, g = 2 w delta / (B A); a weight of one changes no bit.
    -> dict(astar, maxq, y, delta, loss, abs_td, mean_maxq, dlogits [B,A], dvalue [B])"""
    dt = logits.dtype.type
    b, a = logits.shape
    rows = np.arange(b)
    qt = q_from_heads(t_logits, t_value, dueling)
    pick = qt if o_logits is None else q_from_heads(o_logits, o_value, dueling)
    astar = np.argmax(pick, axis=1)                    # first maximal index
    maxq = qt[rows, astar]
    r = np.asarray(reward, np.float64).reshape(b)
    gm = float(gamma) if disc is None else np.asarray(disc, np.float64).reshape(b)
    y = np.where(np.asarray(done).reshape(b).astype(bool), r, r + gm * maxq.astype(np.float64)).astype(dt)
    act = np.asarray(action).reshape(b).astype(np.int64)
    q = q_from_heads(logits, value, dueling)
    delta = q[rows, act] - y
    w = np.ones(b, logits.dtype) if weights is None else np.asarray(weights, logits.dtype).reshape(b)
    g = dt(2.0) * w * delta / dt(b * a)
    hot = np.zeros((b, a), logits.dtype)
    hot[rows, act] = 1
    if dueling:
        dlogits, dvalue = g[:, None] * (hot - dt(1.0) / dt(a)), g.copy()
    else:
        dlogits, dvalue = g[:, None] * hot, np.zeros(b, logits.dtype)
    return dict(astar=astar, maxq=maxq, y=y, delta=delta, loss=(w * delta * delta).sum() / dt(b * a),
                abs_td=np.abs(delta).mean(), mean_maxq=maxq.mean(), dlogits=dlogits, dvalue=dvalue)


def y_numpy1(reward, maxq, done, gamma):
    """the kernel's definition of y from ITS OWN maxq: (float)((double)r + gamma * (double)maxq), one rounding"""
    r = np.asarray(reward, np.float64)
    boot = (r + float(gamma) * np.asarray(maxq, np.float32).astype(np.float64)).astype(np.float32)
    return np.where(np.asarray(done).astype(bool), r.astype(np.float32), boot)


def rel_max(got, ref):
    """largest deviation relative to the reference tensor's largest magnitude"""
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(got, np.float64).reshape(ref.shape) - ref).max() / max(np.abs(ref).max(), 1e-30))


# ----------------------------------------------------------------------------------------------- networks
def oracle_spec(kind, state_dim, action_dim, hidden_size=128, num_layers=1):
    if kind == "cnn":
        return nets.impala_cnn_spec(tuple(state_dim), action_dim)
    return nets.impala_mlp_spec(tuple(state_dim), action_dim, hidden_size, num_layers)


def name_map(spec, ospec):
    """Keras name of ``netspec.dqn_*`` -> oracle name, positionally (a hidden 1-wide head has no Keras name)."""
    return OrderedDict(zip(spec.names, nets.init_params(ospec)))


def seeded_params(ospec, seed, dueling):
    p = nets.init_params(ospec, seed=seed, bias_scale=0.05)
    if not dueling:
        for k in (ospec["v_name"] + "/kernel", ospec["v_name"] + "/bias"):
            p[k] = np.zeros_like(p[k])
    return p


def to_keras_names(spec, ospec, params):
    return OrderedDict((h, np.asarray(params[o], np.float32).reshape(spec.names[h][1])) for h, o in name_map(spec, ospec).items())


class DqnOracle(object):
    """``DQN.train`` on two ``ActorCritic`` nets in ``dtype``: forward of the target net (and the online net) on the next
    states, online forward on the states, TD / mse head, backward, tf.keras Adam."""

    def __init__(self, ospec, params, target_params, dueling, double, gamma, lr, clipnorm=None, dtype=np.float64):
        self.net, self.target = nets.ActorCritic(ospec, params, dtype), nets.ActorCritic(ospec, target_params, dtype)
        self.dueling, self.double, self.gamma = dueling, double, gamma
        self.opt = nets.AdamKeras(self.net.params, lr, clipnorm)

    def step(self, states, next_states, action, reward, done, weights=None, disc=None, apply=True):
        """``weights`` / ``disc``: as ``dqn_loss_ref`` takes them (with ``disc``, ``next_states`` are the
        rows of the boot slots and the labels those of the walk)"""
        tl, tv = self.target.forward(next_states)
        ol, ov = self.net.forward(next_states) if self.double else (None, None)
        lg, v = self.net.forward(states)
        flat = lambda x: None if x is None else x.reshape(-1)
        out = dqn_loss_ref(lg, flat(v), tl, flat(tv), ol, flat(ov), action, reward, done, self.gamma, self.dueling, weights,
                           disc)
        out["grads"] = self.net.backward(out["dlogits"], out["dvalue"].reshape(-1, 1))
        if apply:
            self.opt.apply(self.net.params, out["grads"])
        return out

    def sync_target(self):
        self.target.params = OrderedDict((k, v.copy()) for k, v in self.net.params.items())

    def predict(self, obs):
        lg, v = self.net.forward(obs)
        return q_from_heads(lg, v.reshape(-1), self.dueling)


# ----------------------------------------------------------------------------------------------- C entries (GPU)
def gpu_replay_gather(ring, slots, b=None, row_bytes=None, capacity=None):
    """-> (rc, dst): xt_replay_gather on device tensors; ``dst`` starts as 0xA5 bytes"""
    import torch
    from xingtian_amd import lib as L
    rb = ring[0].numel() * ring.element_size() if row_bytes is None else row_bytes
    b = int(slots.numel()) if b is None else b
    dst = torch.full((max(b, 1), ring[0].numel() * ring.element_size()), 0xA5, dtype=torch.uint8, device=ring.device)
    rc = L.load().xt_replay_gather(L.ptr(ring), rb, ring.shape[0] if capacity is None else capacity, L.ptr(slots), b,
                                   L.ptr(dst), L.stream_ptr())
    torch.cuda.synchronize()
    return rc, dst


def gpu_dqn_loss(logits, value, t_logits, t_value, o_logits, o_value, action, reward, done, gamma, dueling,
                 entry="xt_dqn_loss", slots=None, weights=None, disc=None, b=None, a=None, acc=None, pad=0):
    """-> (rc, dict of host arrays): the scalar head ``entry`` (xt_dqn_loss / xt_dqn_loss_w / xt_dqn_loss_n) on host
    inputs; ``weights`` / ``disc`` go to the entries that take them (None: NULL).  The outputs start as NaN / -1
    sentinels and carry ``pad`` more rows (``out``: 2 * pad + 1 more floats) than the launch owns."""
    import torch
    from xingtian_amd import lib as L
    dev = torch.device("cuda:0")
    up = lambda x, dt: None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(dev)
    rb, ra = logits.shape
    b, a = rb if b is None else b, ra if a is None else a
    d = dict(logits=up(logits, np.float32), value=up(value, np.float32), tl=up(t_logits, np.float32),
             tv=up(t_value, np.float32), ol=up(o_logits, np.float32), ov=up(o_value, np.float32),
             action=up(action, np.int32), reward=up(reward, np.float64), done=up(done, np.uint8),
             slots=up(slots, np.int32), w=up(weights, np.float64), disc=up(disc, np.float64))
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=dev)
    n = rb + pad
    out = dict(dlogits=nan(n, ra), dvalue=nan(n), out=nan(4 + 2 * n + (1 if pad else 0)), y=nan(n), maxq=nan(n),
               astar=torch.full((n,), -1, dtype=torch.int32, device=dev))
    more = {"xt_dqn_loss": (), "xt_dqn_loss_w": (L.ptr(d["w"]),), "xt_dqn_loss_n": (L.ptr(d["w"]), L.ptr(d["disc"]))}[entry]
    assert (weights is None or len(more) >= 1) and (disc is None or len(more) == 2), entry
    rc = getattr(L.load(), entry)(L.ptr(d["logits"]), L.ptr(d["value"]), L.ptr(d["tl"]), L.ptr(d["tv"]), L.ptr(d["ol"]),
                                  L.ptr(d["ov"]), b, a, int(dueling), L.ptr(d["slots"]), L.ptr(d["action"]),
                                  L.ptr(d["reward"]), L.ptr(d["done"]), ctypes.c_double(gamma), L.ptr(out["dlogits"]),
                                  L.ptr(out["dvalue"]), L.ptr(out["out"]), L.ptr(out["y"]), L.ptr(out["astar"]),
                                  L.ptr(out["maxq"]), L.ptr(acc), *more, L.stream_ptr())
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in out.items()}
