"""Float64 restatement of the QMIX graph (xt/model/qmix/qmix_tf.py), in torch on the CPU with autograd for the gradients,
the inputs of the QMIX tests and their bars.  Written from the reference's graph: nothing here knows how the kernels split
the work.  The same functions run in float32 give the deviation the bars are formed from (profiles/qmix_parity.md)."""
import functools
from collections import OrderedDict

import numpy as np
import torch

from tests.dqn_helpers import rel_max as rel
from xingtian_amd.model.qmix.qmix_model import AGENT_VARS, QMixSpec

NEG = -999999.0
LOSS_BAR, GRAD_BAR = 1e-4, 1e-5          # the project's standing bars


def _t(a, dt):
    return torch.as_tensor(np.asarray(a), dtype=dt)


# ---------------------------------------------------------------------- the graph
def gru_ref(xg, wg_h, wc_h, h0, lens):
    """TF1 GRUCell under dynamic_rnn(sequence_length): xg [T1, S, 3H] = the input halves with biases, wg_h [H, 2H] / wc_h [H, H]
    the recurrent halves -> states [T1, S, H] (carried past the length), out (zero past it), the final state"""
    t1, s, h3 = xg.shape
    hd = h3 // 3
    h, states, outs = h0, [], []
    for t in range(t1):
        ru = torch.sigmoid(xg[t, :, :2 * hd] + h @ wg_h)
        r, u = ru[:, :hd], ru[:, hd:]
        c = torch.tanh(xg[t, :, 2 * hd:] + (r * h) @ wc_h)
        hn = u * h + (1 - u) * c
        live = (t < lens)[:, None]
        h = torch.where(live, hn, h)
        states.append(h)
        outs.append(torch.where(live, hn, torch.zeros_like(hn)))
    return torch.stack(states), torch.stack(outs), h


def agent_ref(p, scope, obs, lens, h0=None):
    """obs [B, T1, n, D] -> q [B, T1, n, A], final state [B n, H]"""
    b, t1, n, _ = obs.shape
    g = lambda v: p[scope + "/" + v]      # noqa: E731
    hd = g(AGENT_VARS[1]).shape[0]
    x = torch.relu(obs @ g(AGENT_VARS[0]) + g(AGENT_VARS[1])).permute(1, 0, 2, 3).reshape(t1, b * n, hd)
    wg, wc = g(AGENT_VARS[2]), g(AGENT_VARS[4])
    xg = torch.cat([x @ wg[:hd] + g(AGENT_VARS[3]), x @ wc[:hd] + g(AGENT_VARS[5])], -1)
    h0 = torch.zeros(b * n, hd, dtype=obs.dtype) if h0 is None else h0
    _, out, hT = gru_ref(xg, wg[hd:], wc[hd:], h0, lens)
    q = out @ g(AGENT_VARS[6]) + g(AGENT_VARS[7])
    return q.reshape(t1, b, n, -1).permute(1, 0, 2, 3), hT


def hyp_rows(p, scope, state):
    """state [R, sd] -> the raw hypernet outputs [R, n E + 2 E + 1] = w1 | b1 | w_final | v"""
    d = lambda x, k: x @ p["{}/{}/kernel".format(scope, k)] + p["{}/{}/bias".format(scope, k)]      # noqa: E731
    return torch.cat([d(torch.relu(d(state, "hyper_w1/dense")), "hyper_w1/dense_1"), d(state, "hyper_b1/dense"),
                      d(torch.relu(d(state, "hyper_w_final/dense")), "hyper_w_final/dense_1"),
                      d(torch.relu(d(state, "val_for_bias/dense")), "val_for_bias/dense_1")], 1)


def mix_ref(qs, hyp, n, e):
    r = qs.shape[0]
    w1 = hyp[:, :n * e].abs().reshape(r, n, e)
    hid = torch.nn.functional.elu(torch.einsum("rn,rne->re", qs, w1) + hyp[:, n * e:n * e + e])
    return (hid * hyp[:, n * e + e:n * e + 2 * e].abs()).sum(1) + hyp[:, -1]


def head_ref(qe, qt, avail, actions, hyp_e, hyp_t, rew, term, mask, gamma, double_q, e):
    """qe / qt [B, T1, n, A], actions int64 [B, T, n], rew / term / mask [B, T] -> loss, q_tot [R], y [R], the smallest gap between
    the two best masked eval values of a row"""
    b, t1, n, _ = qe.shape
    chosen = qe[:, :-1].gather(-1, actions[..., None])[..., 0]
    un = avail[:, 1:] == 0
    neg = torch.full_like(qt[:, 1:], NEG)
    tm = torch.where(un, neg, qt[:, 1:].detach())
    em = torch.where(un, neg, qe[:, 1:].detach())
    tq = tm.gather(-1, em.argmax(-1, keepdim=True))[..., 0] if double_q else tm.max(-1).values
    q_tot = mix_ref(chosen.reshape(-1, n), hyp_e, n, e)
    y = rew.reshape(-1) + gamma * (1 - term.reshape(-1)) * mix_ref(tq.reshape(-1, n), hyp_t, n, e).detach()
    loss = (((q_tot - y) * mask.reshape(-1)) ** 2).sum() / mask.sum()
    top = em.topk(2, -1).values if em.shape[-1] > 1 else None
    gap = float("inf") if top is None else float((top[..., 0] - top[..., 1]).min())
    return loss, q_tot, y, gap


def step_ref(spec, params, case, dt=torch.float64, gamma=0.99):
    """the whole train graph -> loss, {eval variable: gradient}, the arg-max gap, the eval q [B, T1, n, A]"""
    p = {k: _t(v, dt).requires_grad_(k.startswith("eval")) for k, v in params.items()}
    b = case["obs"].shape[0]
    lens = torch.as_tensor(np.asarray(case["lens"], np.float64).astype(np.int64))
    obs = _t(case["obs"], dt)
    qe, _ = agent_ref(p, "eval_agent", obs, lens)
    qt, _ = agent_ref(p, "target_agent", obs, lens)
    he = hyp_rows(p, "eval_mixer", _t(case["cur"], dt).reshape(b * spec.T, -1))
    ht = hyp_rows(p, "target_mixer", _t(case["nxt"], dt).reshape(b * spec.T, -1))
    loss, _, _, gap = head_ref(qe, qt, _t(case["avail"], dt), torch.as_tensor(case["actions"][..., 0].astype(np.int64)), he, ht,
                               _t(case["rewards"], dt)[..., 0], _t(case["terminated"], dt)[..., 0], _t(case["mask"], dt)[..., 0],
                               gamma, spec.double_q, spec.E)
    loss.backward()
    grads = OrderedDict((k, v.grad.numpy()) for k, v in p.items() if k.startswith("eval"))
    return float(loss.detach()), grads, gap, qe.detach().numpy()


def rmsprop_ref(params, grads, mg, ms, lr, clip, decay=0.95, eps=1.5e-7):
    """float64 centred RMSProp with tf.clip_by_norm per tensor, in place -> the tensors' norms"""
    norms = {}
    for k, g in grads.items():
        norms[k] = float(np.sqrt((g.astype(np.float64) ** 2).sum()))
        g = g * clip / max(norms[k], clip)
        ms[k] += (g * g - ms[k]) * (1 - decay)
        mg[k] += (g - mg[k]) * (1 - decay)
        params[k] -= lr * g / np.sqrt(ms[k] - mg[k] ** 2 + eps)
    return norms


# ---------------------------------------------------------------------- inputs
def make_spec(n=2, d=11, h=32, a=5, sd=7, e=8, he=16, t=4, batch=4, double_q=True):
    return QMixSpec(dict(n_agents=n, obs_shape=d, rnn_hidden_dim=h, episode_limit=t, n_actions=a, state_shape=sd,
                         mixing_embed_dim=e, hypernet_embed=he, batch_size=batch, use_double_q=double_q))


def make_params(spec, seed, scale=1.0):
    """{TF name: float32 array} of the eval and target sets: glorot-sized kernels times `scale`, small non-zero biases"""
    rng = np.random.default_rng(seed)
    out = OrderedDict()
    for which in ("eval", "target"):
        for name, (_, shape) in spec.names.items():
            lim = np.sqrt(6.0 / sum(shape)) * scale if len(shape) == 2 else 0.1
            val = rng.uniform(-lim, lim, size=shape)
            if name.endswith("gates/bias"):
                val = val + 1.0
            out[spec.tf_name(name, which + "_agent", which + "_mixer")] = val.astype(np.float32)
    return out


def make_case(spec, b, seed, reward_scale=1.0):
    """one batch in the layouts of the reference's placeholders; ragged lengths, rows with mask 0, a terminated step"""
    rng = np.random.default_rng(seed)
    t, t1, n = spec.T, spec.T + 1, spec.n
    avail = (rng.random((b, t1, n, spec.A)) < 0.6).astype(np.float32)
    first = rng.integers(0, spec.A, (b, t1, n))
    np.put_along_axis(avail, first[..., None], 1.0, -1)
    actions = first[:, :-1, :, None].astype(np.float32)
    states = rng.standard_normal((b, t1, spec.sd)).astype(np.float32)
    mask = (rng.random((b, t, 1)) < 0.8).astype(np.float32)
    mask[0, 0] = 1.0
    term = np.zeros((b, t, 1), np.float32)
    term[b - 1, t - 1] = 1.0
    lens = rng.integers(1, t1 + 1, b * n).astype(np.float64)
    lens[0] = t1
    return dict(obs=rng.standard_normal((b, t1, n, spec.D)).astype(np.float32), lens=list(lens), avail=avail, actions=actions,
                cur=states[:, :-1].copy(), nxt=states[:, 1:].copy(),
                rewards=(reward_scale * rng.standard_normal((b, t, 1))).astype(np.float32), terminated=term, mask=mask)


def train_args(case):
    return [case[k] for k in ("obs", "lens", "avail", "actions", "cur", "nxt", "rewards", "terminated", "mask")]


def gru_case(s, t1, h, ragged, seed=0):
    rng = np.random.default_rng(1000 * s + 10 * t1 + h + seed)
    f = np.float32
    lens = np.full(s, t1, np.int32)
    if ragged:
        lens = rng.integers(0, t1 + 1, s).astype(np.int32)
        lens[0], lens[-1] = t1, 0
    return dict(xg=rng.standard_normal((t1, s, 3 * h)).astype(f), wg=rng.uniform(-0.3, 0.3, (2 * h, 2 * h)).astype(f),
                wc=rng.uniform(-0.3, 0.3, (2 * h, h)).astype(f), h0=rng.uniform(-1, 1, (s, h)).astype(f), lens=lens,
                dout=rng.standard_normal((t1, s, h)).astype(f), dhT=rng.standard_normal((s, h)).astype(f))


def gru_case_ref(c, dt=torch.float64):
    """-> states, out, hT, d(xg), d(h0) of sum(out * dout) + sum(hT * dhT)"""
    hd = c["h0"].shape[1]
    xg, h0 = _t(c["xg"], dt).requires_grad_(), _t(c["h0"], dt).requires_grad_()
    st, out, hT = gru_ref(xg, _t(c["wg"], dt)[hd:], _t(c["wc"], dt)[hd:], h0, torch.as_tensor(c["lens"].astype(np.int64)))
    ((out * _t(c["dout"], dt)).sum() + (hT * _t(c["dhT"], dt)).sum()).backward()
    return [x.detach().numpy() for x in (st, out, hT, xg.grad, h0.grad)]


def mix_case(rows, n, a, e, seed=0):
    """inputs of the head alone: (B, T) = (rows / 3, 3) where 3 divides rows, else (rows, 1);
    planted: a row with one available action, an exact tie among the available maxima, raw hypernet zeros, mask 0"""
    rng = np.random.default_rng(97 * rows + 13 * n + 5 * a + e + seed)
    b, t = (rows // 3, 3) if rows % 3 == 0 else (rows, 1)
    f, p = np.float32, n * e + 2 * e + 1
    qe = rng.standard_normal((b, t + 1, n, a)).astype(f)
    qt = rng.standard_normal((b, t + 1, n, a)).astype(f)
    avail = (rng.random((b, t + 1, n, a)) < 0.7).astype(f)
    act = rng.integers(0, a, (b, t, n))
    np.put_along_axis(avail, np.concatenate([act, act[:, -1:]], 1)[..., None], 1.0, -1)
    avail[0, 1, 0] = 0.0
    avail[0, 1, 0, a - 1] = 1.0                          # a single available action
    if b > 1:
        avail[1, 1, 0] = 1.0
        qe[1, 1, 0] = np.minimum(qe[1, 1, 0], 0.5)
        qe[1, 1, 0, [a - 1, 0]] = 0.75                   # an exact tie: index 0 wins
    hyp_e = rng.standard_normal((b * t, p)).astype(f)
    hyp_t = rng.standard_normal((b * t, p)).astype(f)
    hyp_e[0, [0, n * e + e]] = 0.0                       # raw w1 and w_final entries that are exactly 0
    mask = (rng.random((b, t)) < 0.8).astype(f)
    mask[0, 0] = 1.0
    mask[b - 1, t - 1] = 0.0 if b > 1 else 1.0
    term = (rng.random((b, t)) < 0.2).astype(f)
    return dict(qe=qe, qt=qt, avail=avail, actions=act.astype(np.int32), hyp_e=hyp_e, hyp_t=hyp_t,
                rewards=rng.standard_normal((b, t)).astype(f), terminated=term, mask=mask, b=b, t=t)


def mix_case_ref(c, n, e, double_q, dt=torch.float64, gamma=0.99):
    """-> loss, q_tot, y, d(qe), d(hyp_e), the arg-max gap over the rows that are not the planted tie"""
    qe, he = _t(c["qe"], dt).requires_grad_(), _t(c["hyp_e"], dt).requires_grad_()
    loss, q_tot, y, _ = head_ref(qe, _t(c["qt"], dt), _t(c["avail"], dt), torch.as_tensor(c["actions"].astype(np.int64)), he,
                                 _t(c["hyp_t"], dt), _t(c["rewards"], dt), _t(c["terminated"], dt), _t(c["mask"], dt), gamma,
                                 double_q, e)
    loss.backward()
    return float(loss.detach()), q_tot.detach().numpy(), y.detach().numpy(), qe.grad.numpy(), he.grad.numpy()


def time_major(x):
    """[B, T1, n, .] -> [T1, B n, .]"""
    b, t1, n, k = x.shape
    return np.ascontiguousarray(x.transpose(1, 0, 2, 3).reshape(t1, b * n, k))


# ---------------------------------------------------------------------- cases and bars
GRU_CASES = [(s, t1, h, r) for s in (1, 16, 17, 33) for t1 in (1, 2, 5) for h in (32, 64) for r in (False, True)]
MIX_CASES = [(rows, n, a, e, dq) for rows, n in ((1, 1), (63, 2), (65, 5)) for a in (2, 7) for e in (8, 32) for dq in (True, False)]
STEP_CASES = [(b, n, t) for b in (1, 3, 9) for n in (2, 3) for t in (1, 4)]       # (B, n, seq_len)
STEP_SEEDS = {}      # (B, n, seq_len) -> seed, where seed 1 leaves an arg-max gap below 1e-4 (none does: test_cpu_qmix checks)


def step_inputs(b, n, t, reward_scale=1.0):
    """H = 64 for three agents, 32 for two: both widths of the recurrent kernels see the whole step; B = 3 without double-Q"""
    spec = make_spec(n=n, t=t, h=64 if n == 3 else 32, batch=b, double_q=(b != 3))
    seed = STEP_SEEDS.get((b, n, t), 1)
    return spec, make_params(spec, seed), make_case(spec, b, 100 + seed, reward_scale)


@functools.lru_cache(maxsize=None)
def bars():
    """{quantity: (float32 restatement's largest deviation from float64 over the test's cases, bar)}: the standing bar, or four
    times the deviation where that is larger (the rule of profiles/dist_head_parity.md)"""
    dev = dict(gru_fwd=0.0, gru_bwd=0.0, mix_fwd=0.0, mix_bwd=0.0, step_loss=0.0, step_grad=0.0)
    for s, t1, h, r in GRU_CASES:
        c = gru_case(s, t1, h, r)
        a, b = gru_case_ref(c), gru_case_ref(c, torch.float32)
        dev["gru_fwd"] = max([dev["gru_fwd"]] + [rel(y, x) for x, y in zip(a[:3], b[:3])])
        dev["gru_bwd"] = max([dev["gru_bwd"]] + [rel(y, x) for x, y in zip(a[3:], b[3:])])
    for rows, n, a_, e, dq in MIX_CASES:
        c = mix_case(rows, n, a_, e)
        a, b = mix_case_ref(c, n, e, dq), mix_case_ref(c, n, e, dq, torch.float32)
        dev["mix_fwd"] = max([dev["mix_fwd"]] + [rel(y, x) for x, y in zip(a[:3], b[:3])])
        dev["mix_bwd"] = max([dev["mix_bwd"]] + [rel(y, x) for x, y in zip(a[3:], b[3:])])
    for b_, n, t in STEP_CASES:
        spec, params, case = step_inputs(b_, n, t)
        l64, g64, _, _ = step_ref(spec, params, case)
        l32, g32, _, _ = step_ref(spec, params, case, torch.float32)
        dev["step_loss"] = max(dev["step_loss"], abs(l32 - l64) / abs(l64))
        dev["step_grad"] = max([dev["step_grad"]] + [rel(g32[k], g64[k]) for k in g64])
    return {k: (v, max(LOSS_BAR if k == "step_loss" else GRAD_BAR, 4.0 * v)) for k, v in dev.items()}
