"""``QMixModel``: GRU agents and the monotonic mixer of QMIX, updated on HIP kernels.

Reference: xt/model/qmix/qmix_tf.py.  Three agent parameter sets (eval, target, explore; ``Dense -> GRUCell -> Dense``
unrolled over ``episode_limit + 1`` steps from a zero state with ``dynamic_rnn(sequence_length=...)`` semantics) and two
mixers (eval, target) whose weights are ``|hypernet(state)|``.  One ``train`` is ``xt_qmix_step`` (both agents' forward in
one persistent recurrent launch, the fused head, BPTT) and ``xt_qmix_apply`` (centred RMSProp, ``tf.clip_by_norm`` per
tensor).  Explorer processes, and machines without a device, get ``CpuQmixAgent``: the explore agent's forward in NumPy.
"""
import ctypes
from collections import OrderedDict

import numpy as np

from xingtian_amd.model.model import XTModel, learner_device, wants_cpu_replica
from xingtian_amd.model.qmix import default_config as _defaults
from xingtian_amd.register import Registers

AGENT_VARS = ("dense/kernel", "dense/bias", "rnn/gru_cell/gates/kernel", "rnn/gru_cell/gates/bias",
              "rnn/gru_cell/candidate/kernel", "rnn/gru_cell/candidate/bias", "dense_1/kernel", "dense_1/bias")
MIXER_VARS = ("hyper_w1/dense/kernel", "hyper_w1/dense/bias", "hyper_w1/dense_1/kernel", "hyper_w1/dense_1/bias",
              "hyper_b1/dense/kernel", "hyper_b1/dense/bias", "hyper_w_final/dense/kernel", "hyper_w_final/dense/bias",
              "hyper_w_final/dense_1/kernel", "hyper_w_final/dense_1/bias", "val_for_bias/dense/kernel",
              "val_for_bias/dense/bias", "val_for_bias/dense_1/kernel", "val_for_bias/dense_1/bias")
HIDDEN_WIDTHS = (32, 64)
MAX_AGENTS, MAX_ACTIONS, MAX_EMBED = 32, 64, 64


class QMixSpec(object):
    """The sizes of one ``model_config`` and the flat layout of a parameter set: 22 tensors, the agent's 8 first, every
    tensor on a 16-byte boundary (``xt_qmix_layout``).  ``names`` maps ``agent/<var>`` / ``mixer/<var>`` to (offset, shape);
    the TF name of a variable is its scope (``eval_agent``, ``target_agent``, ``explore_agent``, ``eval_mixer``,
    ``target_mixer``) in place of that stem."""

    def __init__(self, cfg):
        need = ("n_agents", "obs_shape", "rnn_hidden_dim", "episode_limit", "n_actions", "state_shape", "mixing_embed_dim",
                "hypernet_embed")
        missing = [k for k in need if k not in cfg]
        if missing:
            raise KeyError("QMixModel: model_config lacks {}".format(missing))
        self.n, self.D, self.H = int(cfg["n_agents"]), int(cfg["obs_shape"]), int(cfg["rnn_hidden_dim"])
        self.T, self.A = int(cfg["episode_limit"]), int(cfg["n_actions"])
        self.sd, self.E, self.HE = int(np.prod(cfg["state_shape"])), int(cfg["mixing_embed_dim"]), int(cfg["hypernet_embed"])
        self.batch_size = int(cfg.get("batch_size", 32))
        self.double_q = bool(cfg.get("use_double_q", _defaults.use_double_q))
        if self.H not in HIDDEN_WIDTHS:
            raise ValueError("QMixModel: rnn_hidden_dim = {} (the recurrent kernels take 32 or 64)".format(self.H))
        if not (1 <= self.n <= MAX_AGENTS and 1 <= self.A <= MAX_ACTIONS and 1 <= self.E <= MAX_EMBED):
            raise ValueError("QMixModel: n_agents = {}, n_actions = {}, mixing_embed_dim = {} beyond the head kernel's limits "
                             "({}, {}, {})".format(self.n, self.A, self.E, MAX_AGENTS, MAX_ACTIONS, MAX_EMBED))
        if min(self.D, self.T, self.sd, self.HE, self.batch_size) < 1:
            raise ValueError("QMixModel: obs_shape, episode_limit, state_shape, hypernet_embed and batch_size must be positive")
        if cfg.get("allow_mix_precision"):
            raise ValueError("QMixModel: allow_mix_precision is not supported (float32 only)")
        H, n, E, HE, sd = self.H, self.n, self.E, self.HE, self.sd
        shapes = [(self.D, H), (H,), (2 * H, 2 * H), (2 * H,), (2 * H, H), (H,), (H, self.A), (self.A,),
                  (sd, HE), (HE,), (HE, E * n), (E * n,), (sd, E), (E,), (sd, HE), (HE,), (HE, E), (E,), (sd, E), (E,), (E, 1), (1,)]
        self.names = OrderedDict()
        off = 0
        for i, shape in enumerate(shapes):
            stem = "agent/" + AGENT_VARS[i] if i < 8 else "mixer/" + MIXER_VARS[i - 8]
            self.names[stem] = (off, shape)
            off = (off + int(np.prod(shape)) + 3) & ~3
            if i == 7:
                self.n_agent_flat = off
        self.n_flat = off

    def var_view(self, flat, name):
        off, shape = self.names[name]
        return flat[off:off + int(np.prod(shape))].reshape(shape)

    def tf_shapes(self, agent_scope="eval_agent", mixer_scope="eval_mixer"):
        """{TF variable name: shape} of one trainable set"""
        return OrderedDict((self.tf_name(k, agent_scope, mixer_scope), s) for k, (_, s) in self.names.items())

    @staticmethod
    def tf_name(name, agent_scope, mixer_scope):
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


def _agent_weights(spec, flat, scope):
    return OrderedDict((scope + "/" + v, spec.var_view(flat, "agent/" + v).copy()) for v in AGENT_VARS)


def _assign_agent(spec, flat, weights, scope="explore_agent"):
    """name-keyed arrays (any agent scope's names are accepted under the explore names) -> the agent's prefix of `flat`"""
    hit = [v for v in AGENT_VARS if scope + "/" + v in weights]
    if not hit:
        raise KeyError("NO node's weights could assign in self.graph {} vs {}".format(
            [scope + "/" + v for v in AGENT_VARS], list(weights.keys())))
    for v in hit:
        val = np.asarray(weights[scope + "/" + v], np.float32)
        if tuple(val.shape) != tuple(spec.names["agent/" + v][1]):
            raise KeyError("update {} encounter error: shape {} vs {}".format(v, val.shape, spec.names["agent/" + v][1]))
        spec.var_view(flat, "agent/" + v)[...] = val


def agent_forward_numpy(spec, flat, obs, hidden, lens=None):
    """obs [B, T, n, D], hidden [B n, H] -> q [B, T, n, A], hidden' in the dtype of `flat` (the float32 replica; the tests'
    float64 reference is written separately, in torch)"""
    dt = flat.dtype
    w1, b1, wg, bg, wc, bc, w2, b2 = (spec.var_view(flat, "agent/" + v) for v in AGENT_VARS)
    obs = np.asarray(obs, dt)
    b, t1, n, _ = obs.shape
    h = np.asarray(hidden, dt).reshape(b * n, spec.H).copy()
    lens = np.full(b * n, t1) if lens is None else np.asarray(lens).astype(np.int64).reshape(b * n)
    q = np.empty((b, t1, n, spec.A), dt)
    sig = lambda z: 1.0 / (1.0 + np.exp(-z))      # noqa: E731
    for t in range(t1):
        x = np.maximum(obs[:, t].reshape(b * n, -1) @ w1 + b1, 0)
        ru = sig(np.concatenate([x, h], 1) @ wg + bg)
        r, u = ru[:, :spec.H], ru[:, spec.H:]
        c = np.tanh(np.concatenate([x, r * h], 1) @ wc + bc)
        hn = u * h + (1 - u) * c
        live = (t < lens)[:, None]
        h = np.where(live, hn, h).astype(dt)
        q[:, t] = (np.where(live, hn, 0).astype(dt) @ w2 + b2).reshape(b, n, spec.A)
    return q, h


class CpuQmixAgent(object):
    """The explore agent on the host (``CpuMuzero``'s pattern): same spec, same seed -> same initial weights.  No ``train``."""

    inference_only = True

    def __init__(self, spec, seed=None):
        self.spec = spec
        self.explore = spec.initial_flat(seed)[:spec.n_agent_flat].copy()

    def get_weights(self, copy=True):
        return _agent_weights(self.spec, self.explore, "explore_agent")

    def set_weights(self, weights):
        _assign_agent(self.spec, self.explore, weights)

    def agent_forward(self, obs, hidden, lens=None):
        return agent_forward_numpy(self.spec, self.explore, obs, hidden, lens)


class HipQmix(object):
    """Flat eval / target parameter sets, gradient and RMSProp slots as torch tensors, the explore agent's prefix copy, and
    the ``xt_qmix`` handle bound to them."""

    inference_only = False

    def __init__(self, spec, device="cuda:0", seed=None, lr=_defaults.lr, gamma=_defaults.gamma, clip=_defaults.grad_norm_clip):
        import torch
        from xingtian_amd import lib as L
        L.require_gpu()
        self.torch, self.L, self.lib = torch, L, L.load()
        self.spec, self.device = spec, torch.device(device)
        d = L.QmixDesc(n_agents=spec.n, obs_dim=spec.D, hidden=spec.H, n_actions=spec.A, state_dim=spec.sd, embed=spec.E,
                       hyper_embed=spec.HE, seq_len=spec.T, double_q=int(spec.double_q))
        offs = (ctypes.c_int64 * (L.QMIX_TENSORS + 1))()
        L.check(self.lib.xt_qmix_layout(ctypes.byref(d), offs), "xt_qmix_layout")
        if [int(o) for o in offs] != [o for o, _ in spec.names.values()] + [spec.n_flat]:
            raise RuntimeError("QMixModel: the library's parameter layout differs from the model's")
        flat = torch.from_numpy(spec.initial_flat(seed))
        zeros = lambda k: torch.zeros(k, dtype=torch.float32, device=self.device)      # noqa: E731
        self.params = flat.to(self.device)
        self.target = flat.to(self.device)      # (the reference's target set starts from its own draw; it is assigned before use)
        self.explore = self.params[:spec.n_agent_flat].clone()
        self.grads, self.mg, self.ms = zeros(spec.n_flat), zeros(spec.n_flat), torch.ones(spec.n_flat, dtype=torch.float32,
                                                                                          device=self.device)
        self.state = zeros(L.QMIX_STATE_FLOATS)
        self.loss_dev = torch.zeros(1, dtype=torch.float64, device=self.device)
        self.cfg = L.QmixCfg(lr=float(lr), decay=_defaults.rms_decay, eps=_defaults.rms_epsilon, grad_norm_clip=float(clip),
                             gamma=float(gamma))
        handle = ctypes.c_void_p()
        L.check(self.lib.xt_qmix_create(ctypes.byref(d), spec.batch_size, ctypes.byref(handle)), "xt_qmix_create")
        nbytes = int(self.lib.xt_qmix_workspace_bytes(handle))
        self.workspace = zeros((nbytes + 3) // 4)
        L.check(self.lib.xt_qmix_bind(handle, L.ptr(self.params), L.ptr(self.target), L.ptr(self.grads), L.ptr(self.mg),
                                      L.ptr(self.ms), L.ptr(self.state), L.ptr(self.workspace), nbytes), "xt_qmix_bind")
        self.handle = handle

    def __del__(self):
        try:
            if self.handle is not None:
                self.torch.cuda.synchronize(self.device)
                self.lib.xt_qmix_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    def _dev(self, array, dtype, shape):
        a = np.ascontiguousarray(np.asarray(array).astype(dtype, copy=False).reshape(shape))
        return self.torch.from_numpy(a).to(self.device)

    def grad_step(self, obs, lens, avail, actions, cur_stats, target_stats, rewards, terminated, mask):
        """loss and gradients of one batch in the reference's array layouts -> the loss as a device tensor of one float64"""
        L, s = self.L, self.spec
        b = int(np.asarray(obs).shape[0])
        if not 1 <= b <= s.batch_size:
            raise ValueError("train: {} episodes, the model was built for batch_size = {}".format(b, s.batch_size))
        f, t, t1 = np.float32, s.T, s.T + 1
        self._keep = (self._dev(obs, f, (b, t1, s.n, s.D)), self._dev(np.asarray(lens, np.float64), np.int32, (b * s.n,)),
                      self._dev(avail, f, (b, t1, s.n, s.A)), self._dev(np.asarray(actions, np.float64), np.int32, (b, t, s.n)),
                      self._dev(cur_stats, f, (b, t, s.sd)), self._dev(target_stats, f, (b, t, s.sd)),
                      self._dev(rewards, f, (b, t)), self._dev(terminated, f, (b, t)), self._dev(mask, f, (b, t)))
        with self.torch.cuda.device(self.device):
            L.check(self.lib.xt_qmix_step(self.handle, *[L.ptr(x) for x in self._keep], b, ctypes.byref(self.cfg),
                                          L.ptr(self.loss_dev), L.stream_ptr()), "xt_qmix_step")
        return self.loss_dev

    def apply(self):
        with self.torch.cuda.device(self.device):
            self.L.check(self.lib.xt_qmix_apply(self.handle, ctypes.byref(self.cfg), self.L.stream_ptr()), "xt_qmix_apply")

    def sync_target(self):
        with self.torch.cuda.device(self.device):
            self.L.check(self.lib.xt_qmix_sync_target(self.handle, self.L.stream_ptr()), "xt_qmix_sync_target")

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
            L.check(self.lib.xt_qmix_agent_forward(self.handle, L.ptr(self.explore if params is None else params), L.ptr(o), b, t,
                                                   L.ptr(h), L.ptr(ln), L.ptr(q), L.ptr(ho), L.stream_ptr()), "xt_qmix_agent_forward")
        return q.cpu().numpy(), ho.cpu().numpy()

    # ---- weights by name
    def get_weights(self, copy=True):
        return _agent_weights(self.spec, self.explore.cpu().numpy(), "explore_agent")

    def set_weights(self, weights):
        flat = self.explore.cpu().numpy().copy()
        _assign_agent(self.spec, flat, weights)
        self.explore.copy_(self.torch.from_numpy(flat))

    def get_train_weights(self, which="eval"):
        """{TF name: array} of the eval (or target) set's 22 tensors"""
        flat = (self.params if which == "eval" else self.target).cpu().numpy()
        return OrderedDict((self.spec.tf_name(k, which + "_agent", which + "_mixer"), self.spec.var_view(flat, k).copy())
                           for k in self.spec.names)

    def set_train_weights(self, weights, which="eval"):
        dst = self.params if which == "eval" else self.target
        flat = dst.cpu().numpy().copy()
        for k in self.spec.names:
            self.spec.var_view(flat, k)[...] = np.asarray(weights[self.spec.tf_name(k, which + "_agent", which + "_mixer")], np.float32)
        dst.copy_(self.torch.from_numpy(flat))

    def get_gradients(self):
        flat = self.grads.cpu().numpy()
        return OrderedDict((self.spec.tf_name(k, "eval_agent", "eval_mixer"), self.spec.var_view(flat, k).copy())
                           for k in self.spec.names)


@Registers.model
class QMixModel(XTModel):
    """The reference's ``QMixModel`` methods on the device network (``scene: "train"`` with a device) or on the NumPy
    replica of the explore agent (``scene: "explore"``, the reference's default, or a machine without a device)."""

    def __init__(self, model_info):
        cfg = model_info.get("model_config") or {}
        self.model_config = cfg
        self.gamma = float(cfg.get("gamma", _defaults.gamma))
        self.lr = float(cfg.get("lr", _defaults.lr))
        self.grad_norm_clip = float(cfg.get("grad_norm_clip", _defaults.grad_norm_clip))
        self.g_type = model_info.get("scene", "explore")
        self.hi_out_val = None
        super().__init__(model_info)
        self.reset_hidden_state()

    def create_model(self, model_info):
        cfg = dict(self.model_config)
        self.spec = QMixSpec(cfg)
        seed = cfg.get("SEED")
        # (wants_cpu_replica without a `type`: model_config.DEVICE decides, else whether the machine has a device)
        if self.g_type != "train" or wants_cpu_replica({"model_config": cfg}):
            self.net = CpuQmixAgent(self.spec, seed=seed)
        else:
            self.net = HipQmix(self.spec, device=learner_device(model_info), seed=seed, lr=self.lr, gamma=self.gamma,
                               clip=self.grad_norm_clip)
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
    def train(self, batch_trajectories, train_obs_len, avail_actions, actions, cur_stats, target_stats, rewards, terminated, mask):
        self._require_learner()
        loss = self.net.grad_step(batch_trajectories, train_obs_len, avail_actions, actions, cur_stats, target_stats, rewards,
                                  terminated, mask)
        self.net.apply()
        return float(loss.item())

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
