"""Float64 restatement of the SCC graph (xt/model/scc/scc_tf.py), in torch on the CPU with autograd for the gradients, the
inputs of the SCC tests and their bars.  Written from the reference's graph, quirks included: the aliased (shifted) critic
state, the masked copies and the ``random`` draws of the credit loops, ``alive`` applied to both sides of the actor's
difference, TF1 Adam and RMSProp (from TF1's documented kernels; not executed against TensorFlow).  Nothing here knows how
the kernels split the work.  Run in float32 it gives the deviation the bars are formed from (profiles/scc_parity.md)."""
import functools
import random
from collections import OrderedDict

import numpy as np
import torch

from tests.qmix_helpers import _t, agent_ref, rel
from xingtian_amd.model.scc.scc_model import SCCSpec

LOSS_BAR, GRAD_BAR = 1e-4, 1e-5          # the project's standing bars


# ---------------------------------------------------------------------- the graph
def critic_ref(spec, p, scope, x):
    """_build_mixer, multi-channel: x [B, T, n (o + A)] -> v [B, T, 1]"""
    xs = x.reshape(x.shape[0], x.shape[1], spec.n, spec.o + spec.A)
    g = lambda j, k: p["{}/group{}/{}".format(scope, j, k)]      # noqa: E731
    hs, i = [], 0
    for j, cnt in enumerate(spec.groups):
        for _ in range(cnt):
            h1 = torch.relu(xs[:, :, i] @ g(j, "layer_1/kernel") + g(j, "layer_1/bias"))
            hs.append(torch.relu(h1 @ g(j, "layer_2/kernel") + g(j, "layer_2/bias")))
            i += 1
    hs = torch.cat(hs, 2) if spec.merge == "concat" else sum(hs)
    return hs @ p[scope + "/v/kernel"] + p[scope + "/v/bias"]


def critic_state(spec, obs, actions):
    """train()'s mixer_state_with_action after the aliased assignment: row t holds row min(t + 1, T - 1)"""
    b = actions.shape[0]
    onehot = np.eye(spec.A)[actions.reshape(-1).astype(np.int64)].reshape(b, -1, spec.n, spec.A)
    x = np.concatenate((obs[:, :-1], onehot), -1).reshape(b, -1, spec.n * (spec.o + spec.A))
    x[:, :-1] = x[:, 1:]
    return x


def credits_ref(spec, v_of, x, mc_times, rng):
    """get_ex_according_to_mask (n <= 2) / get_ex_according_to_mcshap_mask (n > 2) with their masked copies; `rng` stands for
    the module-level ``random`` of the reference.  x: a torch tensor; v_of(x) -> [B, T, 1]"""
    n, w, o = spec.n, spec.o + spec.A, spec.o
    out = []
    for i in range(n):
        if n <= 2:
            m = torch.ones_like(x)
            m[:, :, i * w:(i + 1) * w] = 0
            out.append(v_of(x) - v_of(m * x))
            continue
        draws = []
        for _ in range(mc_times):
            others = [a for a in range(n) if a != i]
            others = rng.sample(others, rng.randint(1, n - 1))
            m_with, m_without = torch.ones_like(x), torch.ones_like(x)
            for ag in others:
                m_with[:, :, ag * w + o:(ag + 1) * w] = 0
                m_without[:, :, ag * w + o:(ag + 1) * w] = 0
            m_without[:, :, i * w + o:(i + 1) * w] = 0
            draws.append(v_of(m_with * x) - v_of(m_without * x))
        out.append(torch.stack(draws, 0).mean(0))
    return torch.stack(out, 2)[..., 0]      # [B, T, n]


def step_ref(spec, params, case, dt=torch.float64, gamma=0.99, seed=0, mc_times=3):
    """the whole train graph -> dict(actor, mixer: the losses; grads {eval variable: gradient}; credits [B, T, n]; v [B, T];
    q: the eval agent's [B, T1, n, A])"""
    p = {k: _t(v, dt).requires_grad_(k.startswith("eval")) for k, v in params.items()}
    x = _t(critic_state(spec, case["obs"], case["actions"]), dt)
    with torch.no_grad():
        credits = credits_ref(spec, lambda y: critic_ref(spec, p, "eval_mixer", y), x, mc_times, random.Random(seed))
    rew, term, mask = (_t(case[k], dt) for k in ("rewards", "terminated", "mask"))
    v = critic_ref(spec, p, "eval_mixer", x)
    y = rew + gamma * (1.0 - term) * critic_ref(spec, p, "target_mixer", x).detach()
    mixer = (((v - y) * mask) ** 2).sum() / mask.sum()
    lens = torch.as_tensor(np.asarray(case["lens"], np.float64).astype(np.int64))
    q, _ = agent_ref(p, "eval_agent", _t(case["traj"], dt), lens)
    onehot = torch.nn.functional.one_hot(torch.as_tensor(case["actions"][..., 0].astype(np.int64)), spec.A).to(dt)
    chosen = (q[:, :-1] * onehot).sum(-1)
    alive = mask.repeat(1, 1, spec.n)
    actor = ((chosen * alive - credits * alive) ** 2).sum() / alive.sum()
    (actor + mixer).backward()
    grads = OrderedDict((k, t.grad.numpy()) for k, t in p.items() if k.startswith("eval"))
    return dict(actor=float(actor.detach()), mixer=float(mixer.detach()), grads=grads, credits=credits.numpy(),
                v=v.detach().numpy()[..., 0], q=q.detach().numpy())


def critic_case_ref(spec, params, case, dv, dt=torch.float64, seed=0):
    """the critic alone -> scalars-free view: v_eval [R], v_target [R], credits [R, n], {critic variable: d sum(dv v_eval)}"""
    p = {k: _t(v, dt).requires_grad_(k.startswith("eval_mixer")) for k, v in params.items()}
    x = _t(critic_state(spec, case["obs"], case["actions"]), dt)
    with torch.no_grad():
        credits = credits_ref(spec, lambda y: critic_ref(spec, p, "eval_mixer", y), x, 3, random.Random(seed))
        vt = critic_ref(spec, p, "target_mixer", x)
    v = critic_ref(spec, p, "eval_mixer", x)
    (v.reshape(-1) * _t(dv, dt)).sum().backward()
    grads = OrderedDict((k, t.grad.numpy()) for k, t in p.items() if k.startswith("eval_mixer"))
    return v.detach().numpy().reshape(-1), vt.numpy().reshape(-1), credits.numpy().reshape(-1, spec.n), grads


def optim_ref(params, grads, slots, step, c_lr, a_lr, mixer_clip, actor_clip):
    """float64 TF1 ApplyAdam (critic) and ApplyRMSProp (agent) behind tf.clip_by_norm per tensor, in place -> the norms.
    slots: {name: [m, v]} for the critic, {name: [ms]} for the agent; step: updates applied so far"""
    norms = {}
    t = step + 1
    alpha = c_lr * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)
    for k, g in grads.items():
        norms[k] = float(np.sqrt((g.astype(np.float64) ** 2).sum()))
        agent = k.startswith("eval_agent")
        if actor_clip > 0:      # the reference gates both clips on the actor's
            clip = actor_clip if agent else mixer_clip
            g = g * clip / max(norms[k], clip)
        if agent:
            ms, = slots[k]
            ms += (g * g - ms) * (1 - 0.9)
            params[k] -= a_lr * g / np.sqrt(ms + 1e-10)
        else:
            m, v = slots[k]
            m += (g - m) * (1 - 0.9)
            v += (g * g - v) * (1 - 0.999)
            params[k] -= alpha * m / (np.sqrt(v) + 1e-8)
    return norms


# ---------------------------------------------------------------------- inputs
def make_spec(n=2, groups=None, merge="concat", o=5, a=3, u=32, h=32, t=4, batch=4):
    cfg = dict(n_agents=n, obs_shape=o + a + n, rnn_hidden_dim=h, episode_limit=t, n_actions=a, dense_unit_number=u,
               enable_critic_multi_channel=True, channel_merge=merge, batch_size=batch, map_name="test")
    if groups:
        cfg["agent_group"] = groups
    return SCCSpec(cfg)


def make_params(spec, seed):
    """{name: float32 array}: the eval set and the target critic; glorot-sized kernels, small non-zero biases"""
    rng = np.random.default_rng(seed)
    out = OrderedDict()
    for which in ("eval", "target"):
        for name, (_, shape) in spec.names.items():
            if which == "target" and name.startswith("agent/"):
                continue
            val = rng.uniform(-1, 1, size=shape) * (np.sqrt(6.0 / sum(shape)) if len(shape) == 2 else 0.1)
            if name.endswith("gates/bias"):
                val = val + 1.0
            out[spec.tf_name(name, which + "_agent", which + "_mixer")] = val.astype(np.float32)
    return out


def make_case(spec, b, seed, zero_row=True):
    """one batch in the layouts of train()'s arguments; the last action index is used, one row has mask 0, one step terminates"""
    rng = np.random.default_rng(seed)
    t, t1, n = spec.T, spec.T + 1, spec.n
    actions = rng.integers(0, spec.A, (b, t, n, 1))
    actions[0, t - 1, 0] = spec.A - 1
    mask = np.ones((b, t, 1), np.float32)
    if zero_row and b * t > 1:
        mask[b - 1, t - 1] = 0.0
    term = np.zeros((b, t, 1), np.float32)
    term[0, t - 1] = 1.0
    lens = rng.integers(1, t1 + 1, b * n).astype(np.float64)
    lens[0] = t1
    f = np.float32
    return dict(traj=rng.standard_normal((b, t1, n, spec.D)).astype(f), obs=rng.standard_normal((b, t1, n, spec.o)).astype(f),
                lens=list(lens), avail=np.ones((b, t1, n, spec.A), f), actions=actions.astype(f), cur=None, nxt=None,
                rewards=rng.standard_normal((b, t, 1)).astype(f), terminated=term, mask=mask)


def train_args(case):
    return [case[k] for k in ("traj", "obs", "lens", "avail", "actions", "cur", "nxt", "rewards", "terminated", "mask")]


def critic_dv(case):
    """a cotangent per row for the stand-alone critic: random, exactly 0 where the mask is (the last row of the last episode)"""
    m = case["mask"].reshape(-1)
    return (np.random.default_rng(int(m.size)).standard_normal(m.size) * m).astype(np.float32)


# ---------------------------------------------------------------------- cases and bars
# (n, groups, merge, U, B, T): a pairwise subset of {(1, [1]), (2, [2]), (3, [1, 2])} x {concat, add} x {32, 128} x {(1, 1), (3, 4),
# (2, 9)}; (o, A) = (5, 3) throughout
CRITIC_CASES = [(1, (1,), "concat", 32, 1, 1), (1, (1,), "add", 128, 3, 4), (2, (2,), "concat", 128, 2, 9), (2, (2,), "add", 32, 1, 1),
                (2, (2,), "add", 32, 3, 4), (3, (1, 2), "concat", 32, 2, 9), (3, (1, 2), "add", 128, 1, 1), (3, (1, 2), "concat", 128, 3, 4),
                (1, (1,), "concat", 32, 2, 9)]
STEP_CASES = [(3, 2, 4, 32, 32), (2, 3, 3, 32, 32), (2, 3, 4, 64, 128)]      # (B, n, T, H, U)


def critic_inputs(n, groups, merge, u, b, t):
    spec = make_spec(n=n, groups=groups, merge=merge, u=u, t=t, batch=b)
    return spec, make_params(spec, 7 + n), make_case(spec, b, 70 + n)


def step_inputs(b, n, t, h=32, u=32):
    spec = make_spec(n=n, groups=(1, 2) if n == 3 else None, merge="add" if n == 3 and u == 32 else "concat", h=h, u=u, t=t, batch=b)
    return spec, make_params(spec, 1), make_case(spec, b, 101)


def _bar(dev, standing=GRAD_BAR):
    return dev, max(standing, 4.0 * dev)


@functools.lru_cache(maxsize=None)
def critic_bars(case):
    """one CRITIC_CASES entry -> {quantity: (the float32 restatement's deviation from float64 on that case's own inputs, bar)}: the
    standing bar, or four times the deviation where that is larger"""
    spec, params, inp = critic_inputs(*case)
    a, b = critic_case_ref(spec, params, inp, critic_dv(inp)), critic_case_ref(spec, params, inp, critic_dv(inp), torch.float32)
    return dict(v_eval=_bar(rel(b[0], a[0])), v_target=_bar(rel(b[1], a[1])), credits=_bar(rel(b[2], a[2])),
                grad=_bar(max(rel(b[3][k], a[3][k]) for k in a[3])))


@functools.lru_cache(maxsize=None)
def step_bars(case):
    """one STEP_CASES entry -> the same for the whole step's losses, its worst gradient tensor and the eval critic's v"""
    spec, params, inp = step_inputs(*case)
    a, b = step_ref(spec, params, inp), step_ref(spec, params, inp, torch.float32)
    return dict(actor=_bar(abs(b["actor"] - a["actor"]) / a["actor"], LOSS_BAR), mixer=_bar(abs(b["mixer"] - a["mixer"]) / a["mixer"], LOSS_BAR),
                grad=_bar(max(rel(b["grads"][k], a["grads"][k]) for k in a["grads"])), v=_bar(rel(b["v"], a["v"])))
