"""``SCCModel``: GRU agents trained against the counterfactual credits of a multi-channel critic.

Reference: xt/model/scc/scc_tf.py.  The agent is QMIX's (``Dense -> GRUCell -> Dense``); the critic is, per agent group,
``Dense(U) -> Dense(U)`` over ``[obs_i | onehot(action_i)]``, merged by concat or add into ``Dense(1)``.  One ``train`` is
``xt_scc_step`` (one critic pass that yields the TD error and every credit, the critic's backward, the agent's forward,
the actor head, BPTT) and ``xt_scc_apply`` (TF1 Adam on the critic, TF1 RMSProp on the agent, ``tf.clip_by_norm`` per
tensor).  Explorer processes, and machines without a device, get QMIX's ``CpuQmixAgent``.
"""
import ctypes
from collections import OrderedDict

import numpy as np

from xingtian_amd.model.model import XTModel, learner_device, wants_cpu_replica
from xingtian_amd.model.qmix.qmix_model import (AGENT_VARS, HIDDEN_WIDTHS, MAX_ACTIONS, MAX_AGENTS, CpuQmixAgent, _agent_weights,
                                                _assign_agent)
from xingtian_amd.model.scc import default_config as _defaults
from xingtian_amd.register import Registers

UNIT_WIDTHS = (32, 64, 128)
MAX_CRITIC_INPUT = 1024
MERGES = ("concat", "add")


class SCCSpec(object):
    """The sizes of one ``model_config`` and the flat layout of a parameter set (``xt_scc_layout``): the agent's 8 tensors, then
    ``mixer/group{j}/layer_{1,2}/{kernel,bias}`` per agent group, then ``mixer/v/{kernel,bias}``.  ``names`` maps a stem to
    (offset, shape); the variable of a set is its scope (``eval_agent``, ``explore_agent``, ``eval_mixer``, ``target_mixer``)
    in place of the stem's first word.  The critic's names are this project's own."""

    def __init__(self, cfg):
        need = ("n_agents", "obs_shape", "rnn_hidden_dim", "episode_limit", "n_actions", "dense_unit_number",
                "enable_critic_multi_channel", "channel_merge")
        missing = [k for k in need if k not in cfg]
        if missing:
            raise KeyError("SCCModel: model_config lacks {}".format(missing))
        self.n, self.D, self.H = int(cfg["n_agents"]), int(cfg["obs_shape"]), int(cfg["rnn_hidden_dim"])
        self.T, self.A, self.U = int(cfg["episode_limit"]), int(cfg["n_actions"]), int(cfg["dense_unit_number"])
        self.o = self.D - self.A - self.n
        self.batch_size = int(cfg.get("batch_size", 32))
        self.merge = cfg["channel_merge"]
        self.groups = list(cfg.get("agent_group") or _defaults.agent_groups.get(cfg.get("map_name"), [self.n]))
        if not cfg.get("use_double_q", _defaults.use_double_q):
            raise RuntimeError("double q is needed")
        if not cfg["enable_critic_multi_channel"]:
            raise ValueError("SCCModel: enable_critic_multi_channel = False (the plain critic is not additive over the agents; "
                             "the credits kernel rests on that)")
        if self.merge not in MERGES:
            raise ValueError("SCCModel: channel_merge = {!r} is neither concat nor add".format(self.merge))
        if self.U not in UNIT_WIDTHS:
            raise ValueError("SCCModel: dense_unit_number = {} (the critic kernels take 32, 64 or 128)".format(self.U))
        if self.H not in HIDDEN_WIDTHS:
            raise ValueError("SCCModel: rnn_hidden_dim = {} (the recurrent kernels take 32 or 64)".format(self.H))
        if not (1 <= self.n <= MAX_AGENTS and 1 <= self.A <= MAX_ACTIONS):
            raise ValueError("SCCModel: n_agents = {}, n_actions = {} beyond the kernels' limits ({}, {})".format(
                self.n, self.A, MAX_AGENTS, MAX_ACTIONS))
        if self.o < 1:
            raise ValueError("SCCModel: obs_shape = {} leaves a raw observation of {} columns".format(self.D, self.o))
        if self.o + self.A > MAX_CRITIC_INPUT:
            raise ValueError("SCCModel: o + n_actions = {} above {}".format(self.o + self.A, MAX_CRITIC_INPUT))
        if sum(self.groups) != self.n or min(self.groups) < 1:
            raise ValueError("SCCModel: agent_group sums to {}, n_agents = {}".format(sum(self.groups), self.n))
        if min(self.T, self.batch_size) < 1:
            raise ValueError("SCCModel: episode_limit and batch_size must be positive")
        if cfg.get("allow_mix_precision"):
            raise ValueError("SCCModel: allow_mix_precision is not supported (float32 only)")
        H, U, ka = self.H, self.U, self.o + self.A
        stems = [("agent/" + v, s) for v, s in zip(AGENT_VARS, [(self.D, H), (H,), (2 * H, 2 * H), (2 * H,), (2 * H, H), (H,),
                                                                 (H, self.A), (self.A,)])]
        for j in range(len(self.groups)):
            stems += [("mixer/group{}/layer_1/kernel".format(j), (ka, U)), ("mixer/group{}/layer_1/bias".format(j), (U,)),
                      ("mixer/group{}/layer_2/kernel".format(j), (U, U)), ("mixer/group{}/layer_2/bias".format(j), (U,))]
        stems += [("mixer/v/kernel", (U if self.merge == "add" else self.n * U, 1)), ("mixer/v/bias", (1,))]
        self.names = OrderedDict()
        off = 0
        for i, (stem, shape) in enumerate(stems):
            self.names[stem] = (off, shape)
            off = (off + int(np.prod(shape)) + 3) & ~3
            if i == 7:
                self.n_agent_flat = off
        self.n_flat = off

    def var_view(self, flat, name):
        off, shape = self.names[name]
        return flat[off:off + int(np.prod(shape))].reshape(shape)

    @staticmethod
    def tf_name(name, agent_scope="eval_agent", mixer_scope="eval_mixer"):
        stem, _, var = name.partition("/")
        return (agent_scope if stem == "agent" else mixer_scope) + "/" + var

    def initial_flat(self, seed=None):
        """glorot_uniform kernels, zero biases, the gates' bias 1 (TF1's GRUCell)"""
        rng = np.random.default_rng(seed)
        flat = np.zeros(self.n_flat, np.float32)
        for name, (_, shape) in self.names.items():
            if len(shape) == 2:
                lim = np.sqrt(6.0 / (shape[0] + shape[1]))
                self.var_view(flat, name)[...] = rng.uniform(-lim, lim, size=shape).astype(np.float32)
            elif name.endswith("gates/bias"):
                self.var_view(flat, name)[...] = 1.0
        return flat

    def desc(self, L):
        d = L.SccDesc(n_agents=self.n, obs_dim=self.D, hidden=self.H, n_actions=self.A, units=self.U, seq_len=self.T,
                      merge=MERGES.index(self.merge), multi_channel=1, n_groups=len(self.groups))
        for j, g in enumerate(self.groups):
            d.groups[j] = g
        return d


class HipScc(object):
    """Flat eval / target parameter sets, gradients and optimiser slots as torch tensors, the explore agent's prefix copy, and
    the ``xt_scc`` handle bound to them."""

    inference_only = False

    def __init__(self, spec, device="cuda:0", seed=None, c_lr=_defaults.c_lr, a_lr=_defaults.a_lr, gamma=_defaults.gamma,
                 mixer_clip=_defaults.mixer_grad_norm_clip, actor_clip=_defaults.actor_grad_norm_clip):
        import torch
        from xingtian_amd import lib as L
        L.require_gpu()
        self.torch, self.L, self.lib = torch, L, L.load()
        self.spec, self.device = spec, torch.device(device)
        d = spec.desc(L)
        offs, nt = (ctypes.c_int64 * (L.SCC_MAX_TENSORS + 1))(), ctypes.c_int32()
        L.check(self.lib.xt_scc_layout(ctypes.byref(d), offs, ctypes.byref(nt)), "xt_scc_layout")
        if [int(o) for o in offs[:nt.value + 1]] != [o for o, _ in spec.names.values()] + [spec.n_flat]:
            raise RuntimeError("SCCModel: the library's parameter layout differs from the model's")
        flat = torch.from_numpy(spec.initial_flat(seed))
        zeros = lambda k: torch.zeros(k, dtype=torch.float32, device=self.device)      # noqa: E731
        self.params = flat.to(self.device)
        self.target = flat.to(self.device)      # (the reference's target critic starts from its own draw; it is assigned before use)
        self.explore = self.params[:spec.n_agent_flat].clone()
        self.grads, self.slot1, self.slot2 = zeros(spec.n_flat), zeros(spec.n_flat), zeros(spec.n_flat)
        self.slot2[:spec.n_agent_flat] = 1.0    # RMSProp's ms starts at 1; Adam's m and v at 0
        self.state = zeros(L.SCC_STATE_FLOATS)
        self.loss_dev = torch.zeros(2, dtype=torch.float64, device=self.device)
        self.cfg = L.SccCfg(c_lr=float(c_lr), a_lr=float(a_lr), mixer_clip=float(mixer_clip), actor_clip=float(actor_clip),
                            gamma=float(gamma), beta1=_defaults.adam_beta1, beta2=_defaults.adam_beta2,
                            adam_eps=_defaults.adam_epsilon, rms_decay=_defaults.rms_decay, rms_eps=_defaults.rms_epsilon)
        handle = ctypes.c_void_p()
        L.check(self.lib.xt_scc_create(ctypes.byref(d), spec.batch_size, ctypes.byref(handle)), "xt_scc_create")
        nbytes = int(self.lib.xt_scc_workspace_bytes(handle))
        self.workspace = zeros((nbytes + 3) // 4)
        L.check(self.lib.xt_scc_bind(handle, L.ptr(self.params), L.ptr(self.target), L.ptr(self.grads), L.ptr(self.slot1),
                                     L.ptr(self.slot2), L.ptr(self.state), L.ptr(self.workspace), nbytes), "xt_scc_bind")
        self.handle = handle

    def __del__(self):
        try:
            if self.handle is not None:
                self.torch.cuda.synchronize(self.device)
                self.lib.xt_scc_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    def _dev(self, array, dtype, shape):
        a = np.ascontiguousarray(np.asarray(array).astype(dtype, copy=False).reshape(shape))
        return self.torch.from_numpy(a).to(self.device)

    def _batch(self, obs):
        b = int(np.asarray(obs).shape[0])
        if not 1 <= b <= self.spec.batch_size:
            raise ValueError("train: {} episodes, the model was built for batch_size = {}".format(b, self.spec.batch_size))
        return b

    def grad_step(self, batch_trajectories, obs, lens, actions, rewards, terminated, mask):
        """both losses and all gradients of one batch in the reference's array layouts -> a device tensor of two float64:
        actor_loss, mixer_loss"""
        L, s = self.L, self.spec
        b = self._batch(obs)
        f, t, t1 = np.float32, s.T, s.T + 1
        self._keep = (self._dev(batch_trajectories, f, (b, t1, s.n, s.D)), self._dev(obs, f, (b, t1, s.n, s.o)),
                      self._dev(np.asarray(lens, np.float64), np.int32, (b * s.n,)),
                      self._dev(np.asarray(actions, np.float64), np.int32, (b, t, s.n)), self._dev(rewards, f, (b, t)),
                      self._dev(terminated, f, (b, t)), self._dev(mask, f, (b, t)))
        with self.torch.cuda.device(self.device):
            L.check(self.lib.xt_scc_step(self.handle, *[L.ptr(x) for x in self._keep], b, ctypes.byref(self.cfg),
                                         L.ptr(self.loss_dev), L.stream_ptr()), "xt_scc_step")
        return self.loss_dev

    def critic(self, obs, actions, target=True, dv=None, raw=False):
        """the critic alone -> dict of NumPy arrays: scalars [3 (2 without the target), n, R], credits [R, n], v [R]; with
        dv [R], the critic's gradients land in ``get_gradients()``.  raw: obs is a [B, T, n (o + A)] critic state, which yields
        v alone"""
        L, s, torch = self.L, self.spec, self.torch
        b = self._batch(obs)
        r = b * s.T
        x = self._dev(obs, np.float32, (b, s.T, s.n, s.o + s.A) if raw else (b, s.T + 1, s.n, s.o))
        a = None if raw else self._dev(np.asarray(actions, np.float64), np.int32, (b, s.T, s.n))
        sc = None if raw else torch.empty((3 if target else 2, s.n, r), dtype=torch.float32, device=self.device)
        cr = None if raw else torch.empty((r, s.n), dtype=torch.float32, device=self.device)
        v = None if dv is not None else torch.empty(r, dtype=torch.float32, device=self.device)
        g = None if dv is None else self._dev(dv, np.float32, (r,))
        with torch.cuda.device(self.device):
            L.check(self.lib.xt_scc_critic(self.handle, L.ptr(self.params), L.ptr(self.target) if target else None, L.ptr(x), L.ptr(a),
                                           b, int(raw), L.ptr(sc), L.ptr(cr), L.ptr(v), L.ptr(g),
                                           None if dv is None else L.ptr(self.grads), L.stream_ptr()), "xt_scc_critic")
        host = lambda x: None if x is None else x.cpu().numpy()      # noqa: E731
        return dict(scalars=host(sc), credits=host(cr), v=host(v))

    def apply(self):
        with self.torch.cuda.device(self.device):
            self.L.check(self.lib.xt_scc_apply(self.handle, ctypes.byref(self.cfg), self.L.stream_ptr()), "xt_scc_apply")

    def sync_target(self):
        with self.torch.cuda.device(self.device):
            self.L.check(self.lib.xt_scc_sync_target(self.handle, self.L.stream_ptr()), "xt_scc_sync_target")

    def sync_explore(self):
        self.explore.copy_(self.params[:self.spec.n_agent_flat])

    def agent_forward(self, obs, hidden, lens=None, params=None):
        """obs [B, T, n, D], hidden [B n, H] -> q [B, T, n, A], hidden' (NumPy) on the explore agent (or `params`)"""
        L, s, torch = self.L, self.spec, self.torch
        obs = np.asarray(obs, np.float32)
        b, t = int(obs.shape[0]), int(obs.shape[1])
        o = self._dev(obs, np.float32, (b, t, s.n, s.D))
        h = self._dev(hidden, np.float32, (b * s.n, s.H))
        ln = None if lens is None else self._dev(np.asarray(lens, np.float64), np.int32, (b * s.n,))
        q = torch.empty((b, t, s.n, s.A), dtype=torch.float32, device=self.device)
        ho = torch.empty((b * s.n, s.H), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            L.check(self.lib.xt_scc_agent_forward(self.handle, L.ptr(self.explore if params is None else params), L.ptr(o), b, t,
                                                  L.ptr(h), L.ptr(ln), L.ptr(q), L.ptr(ho), L.stream_ptr()), "xt_scc_agent_forward")
        return q.cpu().numpy(), ho.cpu().numpy()

    # ---- weights by name
    def get_weights(self, copy=True):
        return _agent_weights(self.spec, self.explore.cpu().numpy(), "explore_agent")

    def set_weights(self, weights):
        flat = self.explore.cpu().numpy().copy()
        _assign_agent(self.spec, flat, weights)
        self.explore.copy_(self.torch.from_numpy(flat))

    def _named(self, flat, which):
        return OrderedDict((self.spec.tf_name(k, which + "_agent", which + "_mixer"), self.spec.var_view(flat, k).copy())
                           for k in self.spec.names)

    def get_train_weights(self, which="eval"):
        """{name: array} of the eval (or target) set's tensors"""
        return self._named((self.params if which == "eval" else self.target).cpu().numpy(), which)

    def set_train_weights(self, weights, which="eval"):
        dst = self.params if which == "eval" else self.target
        flat = dst.cpu().numpy().copy()
        for k in self.spec.names:
            name = self.spec.tf_name(k, which + "_agent", which + "_mixer")
            if name in weights:      # (a target set carries only the critic)
                self.spec.var_view(flat, k)[...] = np.asarray(weights[name], np.float32)
        dst.copy_(self.torch.from_numpy(flat))

    def get_gradients(self):
        return self._named(self.grads.cpu().numpy(), "eval")


@Registers.model
class SCCModel(XTModel):
    """The reference's ``SCCModel`` methods on the device network (``scene: "train"`` with a device) or on the NumPy replica of
    the explore agent (``scene: "explore"``, the reference's default, or a machine without a device)."""

    def __init__(self, model_info):
        cfg = model_info.get("model_config") or {}
        self.model_config = cfg
        self.g_type = model_info.get("scene", "explore")
        self.hi_out_val = None
        super().__init__(model_info)
        self.reset_hidden_state()

    def create_model(self, model_info):
        cfg = dict(self.model_config)
        self.spec = SCCSpec(cfg)
        self.agent_group = self.spec.groups
        seed = cfg.get("SEED")
        if self.g_type != "train" or wants_cpu_replica({"model_config": cfg}):
            self.net = CpuQmixAgent(self.spec, seed=seed)
        else:
            g = lambda k: float(cfg.get(k, getattr(_defaults, k)))      # noqa: E731
            self.net = HipScc(self.spec, device=learner_device(model_info), seed=seed, c_lr=g("c_lr"), a_lr=g("a_lr"),
                              gamma=g("gamma"), mixer_clip=g("mixer_grad_norm_clip"), actor_clip=g("actor_grad_norm_clip"))
        return self.net

    # ---- explore
    def reset_hidden_state(self):
        self.hi_out_val = np.zeros((self.spec.n, self.spec.H), np.float32)

    def infer_actions(self, agent_inputs):
        """agent_inputs [1, 1, n_agents, obs_shape] -> q [1, n_agents, n_actions]; the hidden state is carried"""
        x = np.asarray(agent_inputs, np.float32).reshape(1, 1, self.spec.n, self.spec.D)
        q, self.hi_out_val = self.net.agent_forward(x, self.hi_out_val)
        return q.reshape(-1, self.spec.n, self.spec.A)

    # ---- train
    def train(self, batch_trajectories, obs, train_obs_len, avail_actions, actions, cur_stats, target_stats, rewards, terminated,
              mask):
        """avail_actions, cur_stats and target_stats reach neither loss in the reference's graph; they are not copied"""
        self._require_learner()
        loss = self.net.grad_step(batch_trajectories, obs, train_obs_len, actions, rewards, terminated, mask)
        self.net.apply()
        actor, mixer = loss.cpu().tolist()
        return actor + mixer

    def get_mixer_output(self, critic_state):
        """critic_state [B, T, n (o + A)] -> the eval critic's v [B, T, 1]"""
        self._require_learner()
        state = np.asarray(critic_state, np.float32)
        return self.net.critic(state, None, target=False, raw=True)["v"].reshape(state.shape[0], self.spec.T, 1)

    def assign_targets(self):
        self._require_learner()
        self.net.sync_target()

    def assign_explore_agent(self):
        self._require_learner()
        self.net.sync_explore()

    # ---- checkpoints: .npz files of the explore agent's variables
    def save_explore_agent_weights(self, save_path):
        return self.save_model(save_path)

    def restore_explorer_variable(self, model_name):
        return self.load_model(model_name if str(model_name).endswith(".npz") else str(model_name) + ".npz")

    def predict(self, state):
        return self.infer_actions(state)
