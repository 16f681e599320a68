"""``MuzeroModel``: the three networks of MuZero and their K-step unrolled update on HIP kernels.

Reference: xt/model/muzero/muzero_model.py (``MuzeroModel`` with ``MuzeroMlp`` / ``MuzeroCnn``).  One ``train`` is

    h_0 = rep(obs);  for i < U:  t_i = dyn_trunk([h_i | onehot(a_i)]),  h_{i+1} = relu(Dense_h(t_i)),
    r_{i+1} = softmax(Dense_r(t_i));  for k <= U:  q_k = relu(Dense(h_k)),  p_k / v_k = softmax(Dense_p / Dense_v (q_k))

    ce(p, t) = -(1 / (B N)) sum_b sum_j t_bj log(p_bj + 1e-10)          (the mean runs over the support axis as well)
    L = ce(p_0, pi_0) + ce(v_0, z_0) + sum_{i < U} [ce(r_{i+1}, u_i) + ce(p_{i+1}, pi_{i+1}) + ce(v_{i+1}, z_{i+1})]

with the reward target of dynamics step i taken from column i (column U is never read), the three terms of every unroll
step carrying 1 / U in the gradient only, and ``scale_gradient(h_k, 0.5)`` behind the prediction net's read of h_k
(k >= 1): the gradient that dynamics step k sends into h_k is halved, the one from p_k / v_k is not.  ``loss_weights`` is
accepted and unused, as in the reference.  The optimiser is ``tf.train.AdamOptimizer(LR)`` (eps 1e-8, no clipping).

Weight decay: the reference adds ``1e-4 * l2_loss(w)`` over ``full_model.get_weights()`` -- NumPy copies of the INITIAL
values, so the term is a constant of the graph: it has no gradient and moves no weight.  Nothing is invented in its
place, and the loss this model reports LEAVES THE CONSTANT OUT.

The update is one C call (``xt_mz_step``, then ``xt_mz_apply``); U is ``td_step`` of the model's config (default 5).
Scalar targets become two-hot rows on the device exactly as ``conver_value`` makes them on the host (float64, one
rounding); where the reference would raise -- the compressed value an exact integer at the top of the range -- the whole
mass goes on the last bin.  Weights are keyed by Keras' automatic layer names in the reference's list order
(representation, dynamics, prediction); ``set_weights`` takes that dict or a list in that order.  Explorer processes get
the inference-only NumPy replica ``CpuMuzero`` (``initial_inference`` / ``recurrent_inference`` / ``value_inference``).
"""
import ctypes
import math
import typing
from collections import OrderedDict

import numpy as np

from xingtian_amd.model import netspec
from xingtian_amd.model.cpu_net import initial_weights
from xingtian_amd.model.model import XTModel, learner_device, wants_cpu_replica
from xingtian_amd.model.muzero import default_config as _defaults
from xingtian_amd.register import Registers

MAX_UNROLL = 16
WEIGHT_DECAY = 1e-4          # carried as the reference carries it: a constant of its graph, see the module docstring


# ---------------------------------------------------------------------- host arithmetic (muzero_utils.py, muzero_model.py)
def value_compression(value):
    return np.sign(value) * (np.sqrt(np.abs(value) + 1) - 1) + 0.001 * value


def value_decompression(value):
    return np.sign(value) * (((np.sqrt(1 + 4 * 0.001 * (np.abs(value) + 1 + 0.001)) - 1) / (2 * 0.001)) ** 2 - 1)


def support_size(vmin, vmax):
    return int(math.ceil(value_compression(vmax - vmin))) + 1


def conver_value(target_value, support, vmin, vmax):
    """scalars [B, T] -> two-hot rows [B, T, support] (float64): 1 - rest on floor, rest on floor + 1.  The device makes
    the same rows; where ``floor + 1 == support`` (the reference raises there) the whole mass goes on the last bin."""
    target_value = np.clip(np.asarray(target_value, np.float64), vmin, vmax) - vmin
    targets = np.zeros(target_value.shape[0:2] + (support,))
    value = value_compression(target_value)
    floor = np.floor(value)
    rest = value - floor
    index = floor.astype(int)
    top = index >= support - 1
    bi, ti = np.nonzero(~top)
    targets[bi, ti, index[bi, ti]] = 1 - rest[bi, ti]
    targets[bi, ti, index[bi, ti] + 1] = rest[bi, ti]
    bi, ti = np.nonzero(top)
    targets[bi, ti, support - 1] = 1.0
    return targets


def value_transform(value_support, support, vmin, vmax):
    """A categorical row over the bins 0 .. support - 1 -> the scalar it stands for: the row's mean bin, decompressed,
    shifted back by ``vmin`` and held inside [vmin, vmax].  -> a Python float (``np.asscalar`` is gone from NumPy)"""
    bins = np.arange(support)
    mean_bin = np.dot(value_support, bins)
    return float(min(max(value_decompression(mean_bin) + vmin, vmin), vmax))


class NetworkOutput(typing.NamedTuple):
    """what one inference hands the search: scalars already transformed, the policy row and the hidden state as arrays"""
    value: float
    reward: float
    policy: np.ndarray
    hidden_state: np.ndarray


# ---------------------------------------------------------------------- the three chains and the flat layout
class MuzeroSpec(object):
    """rep / dyn / pred layer chains (``netspec.Layer``), flat float32 layout (every block [K, N] kernel + [N] bias on a
    16-byte boundary, in the order rep, dyn, pred) and the name map in the reference's list order.
    dyn = trunk layers + [Dense_h, Dense_r]; pred = trunk layers + [Dense_v, Dense_p]."""

    def __init__(self, rep, dyn, pred, hidden, action_dim, unroll, value_range, reward_range, obs_kind, input_xform, state_dim):
        self.rep, self.dyn, self.pred = rep, dyn, pred
        self.hidden, self.action_dim, self.unroll = int(hidden), int(action_dim), int(unroll)
        self.value_min, self.value_max = float(value_range[0]), float(value_range[1])
        self.reward_min, self.reward_max = float(reward_range[0]), float(reward_range[1])
        if self.action_dim < 1:
            raise ValueError("MuZero: action_dim = {} below 1".format(action_dim))
        if not (1 <= self.unroll <= MAX_UNROLL):
            raise ValueError("MuZero: td_step = {} outside [1, {}]".format(unroll, MAX_UNROLL))
        if not (self.value_max > self.value_min and self.reward_max > self.reward_min):
            raise ValueError("MuZero: max <= min (value [{}, {}], reward [{}, {}])".format(
                self.value_min, self.value_max, self.reward_min, self.reward_max))
        self.value_support = support_size(self.value_min, self.value_max)
        self.reward_support = support_size(self.reward_min, self.reward_max)
        if self.value_support < 2 or self.reward_support < 2:
            raise ValueError("MuZero: support sizes {} / {} (value / reward) below 2".format(
                self.value_support, self.reward_support))
        self.obs_kind, self.input_xform, self.state_dim = obs_kind, input_xform, tuple(state_dim)
        self.names = OrderedDict()
        off = 0
        for lay in list(rep) + list(dyn) + list(pred):
            lay.param_off = off
            self.names[lay.name + "/kernel"] = (off, tuple(lay.kernel_shape))
            self.names[lay.name + "/bias"] = (off + lay.K * lay.N, (lay.N,))
            off = (off + (lay.K + 1) * lay.N + 3) & ~3
        self.n_flat = off
        self.n_params = sum(int(np.prod(s)) for _, s in self.names.values())
        self.store_shape = {}

    def var_view(self, flat, name):
        off, shape = self.names[name]
        return flat[off:off + int(np.prod(shape))].reshape(shape)

    def layers(self):
        return list(self.rep) + list(self.dyn) + list(self.pred)


def _named(lay, index, stem):
    lay.name = stem if index == 0 else "{}_{}".format(stem, index)
    return lay


def mlp_spec(state_dim, action_dim, hidden1, hidden2, unroll, value_range, reward_range, obs_type="float32"):
    """``MuzeroMlp`` (muzero_mlp.py:43-63).  Keras names in creation order: rep dense, dense_1; prediction dense_2 (trunk),
    dense_3 (v), dense_4 (p); dynamics dense_5 (trunk), dense_6 (h), dense_7 (r)."""
    state_dim = tuple(int(s) for s in (state_dim if hasattr(state_dim, "__len__") else (state_dim,)))
    if len(state_dim) != 1:
        raise ValueError("MuzeroMlp: state_dim {} is not a vector".format(state_dim))
    if state_dim[0] % 4 or hidden1 % 4 or hidden2 % 4:
        raise ValueError("MuzeroMlp: state_dim {}, HIDDEN1_UNITS {} and HIDDEN2_UNITS {} must be multiples of 4 for the "
                         "representation chain's kernels".format(state_dim[0], hidden1, hidden2))
    if obs_type not in ("float32", "uint8", "int8"):
        raise ValueError("obs_type {!r}: float32, uint8 or int8".format(obs_type))
    s = support_size
    d = netspec._dense
    rep = [_named(d("", state_dim[0], hidden1, "relu", 0), 0, "dense"), _named(d("", hidden1, hidden2, "relu", 0), 1, "dense")]
    pred = [_named(d("", hidden2, hidden1, "relu", 0), 2, "dense"),
            _named(d("", hidden1, s(*value_range), "none", 0), 3, "dense"),
            _named(d("", hidden1, action_dim, "none", 0), 4, "dense")]
    dyn = [_named(d("", hidden2 + action_dim, hidden1, "relu", 0), 5, "dense"),
           _named(d("", hidden1, hidden2, "relu", 0), 6, "dense"),
           _named(d("", hidden1, s(*reward_range), "none", 0), 7, "dense")]
    return MuzeroSpec(rep, dyn, pred, hidden2, action_dim, unroll, value_range, reward_range, "float32", (0, 0.0, 1.0), state_dim)


def cnn_spec(state_dim, action_dim, hidden_out, unroll, value_range, reward_range, obs_type="float32"):
    """``MuzeroCnn`` (muzero_cnn.py:42-67): x / 255, Conv 32 8x8/4, 32 4x4/2, 64 3x3/1 (VALID, relu), Dense HIDDEN_OUT;
    prediction Dense 128 + v + p; dynamics Dense 256, 128 + h + r.  Keras names: conv2d, conv2d_1, conv2d_2, dense;
    dense_1, dense_2 (v), dense_3 (p); dense_4, dense_5, dense_6 (h), dense_7 (r)."""
    state_dim = tuple(int(s) for s in state_dim)
    if len(state_dim) != 3:
        raise ValueError("MuzeroCnn: state_dim {} is not [H, W, C]".format(state_dim))
    if obs_type not in ("float32", "uint8", "int8"):
        raise ValueError("obs_type {!r}: float32, uint8 or int8".format(obs_type))
    h, w, c = state_dim
    if c % 4 or hidden_out % 4:
        raise ValueError("MuzeroCnn: the channel count {} and HIDDEN_OUT {} must be multiples of 4".format(c, hidden_out))
    if h < 36 or w < 36:
        raise ValueError("MuzeroCnn: a state of {} is too small for the 8x8/4, 4x4/2, 3x3/1 trunk: the smallest valid one "
                         "is [36, 36, C]".format(list(state_dim)))
    rep = []
    for i, (n, k, s) in enumerate([(32, 8, 4), (32, 4, 2), (64, 3, 1)]):
        lay = netspec._conv("", h, w, c, n, k, s, "valid", "relu", 0)
        rep.append(_named(lay, i, "conv2d"))
        h, w, c = lay.OH, lay.OW, n
    d = netspec._dense
    rep.append(_named(d("", h * w * c, hidden_out, "relu", 0), 0, "dense"))
    s = support_size
    pred = [_named(d("", hidden_out, 128, "relu", 0), 1, "dense"),
            _named(d("", 128, s(*value_range), "none", 0), 2, "dense"),
            _named(d("", 128, action_dim, "none", 0), 3, "dense")]
    dyn = [_named(d("", hidden_out + action_dim, 256, "relu", 0), 4, "dense"),
           _named(d("", 256, 128, "relu", 0), 5, "dense"),
           _named(d("", 128, hidden_out, "relu", 0), 6, "dense"),
           _named(d("", 128, s(*reward_range), "none", 0), 7, "dense")]
    kind = {"uint8": "uint8", "int8": "int8", "float32": "float32_255"}[obs_type]
    return MuzeroSpec(rep, dyn, pred, hidden_out, action_dim, unroll, value_range, reward_range, kind, (1, 0.0, 255.0), state_dim)


def obs_as_network_input(spec, obs, obs_type):
    """the observation array in the dtype the network's first layer is fed: ``int8`` wraps uint8 frames (200 -> -56), as
    feeding the reference's int8 placeholder does; MLP observations are cast to float32 on the host"""
    x = np.asarray(obs)
    if obs_type == "int8":
        x = x.view(np.int8) if x.dtype == np.uint8 else x.astype(np.int8, copy=False)
    elif obs_type == "uint8":
        x = x.astype(np.uint8, copy=False)
    else:
        x = x.astype(np.float32, copy=False)
    if spec.obs_kind == "float32":
        x = x.astype(np.float32, copy=False)
    return np.ascontiguousarray(x)


def weights_as_dict(spec, weights):
    """a name-keyed dict as it is, or a list in the reference's order (rep, dyn, pred; kernel then bias) -> dict"""
    if hasattr(weights, "keys"):
        return weights
    weights = list(weights)
    if len(weights) != len(spec.names):
        raise KeyError("set_weights: a list of {} arrays, the model has {} variables".format(len(weights), len(spec.names)))
    return OrderedDict(zip(spec.names, weights))


# ---------------------------------------------------------------------- inference-only NumPy replica
class CpuMuzero(object):
    """The three networks on the host, float32 (``cpu_net.CpuActorCritic``'s pattern): same spec, same flat layout, same
    seed -> same initial weights; loads what a GPU learner publishes.  No ``train``."""

    inference_only = True

    def __init__(self, spec, seed=None, dtype=np.float32):
        self.spec, self.dtype = spec, dtype
        self.params = np.zeros(spec.n_flat, np.float32)
        self.set_weights(initial_weights(spec, seed))

    def get_weights(self, copy=True):
        return OrderedDict((n, self.spec.var_view(self.params, n).copy()) for n in self.spec.names)

    def set_weights(self, weights):
        weights = weights_as_dict(self.spec, weights)
        hit = [k for k in weights.keys() if k in self.spec.names]
        if not hit:
            raise KeyError("NO node's weights could assign in self.graph {} vs {}".format(list(self.spec.names), list(weights.keys())))
        for name in hit:
            val = np.asarray(weights[name], np.float32)
            if tuple(val.shape) != tuple(self.spec.names[name][1]):
                raise KeyError("update {} encounter error: shape {} vs {}".format(name, val.shape, self.spec.names[name][1]))
            self.spec.var_view(self.params, name)[...] = val

    def publish_weights(self, ring, ctr_info=None, lag=0):
        return ring.publish_flat_host(self.params, self.spec, ctr_info)

    def _wb(self, lay):
        p = self.params.astype(self.dtype, copy=False)
        return (p[lay.param_off:lay.param_off + lay.K * lay.N].reshape(lay.K, lay.N),
                p[lay.param_off + lay.K * lay.N:lay.param_off + (lay.K + 1) * lay.N])

    def _dense(self, lay, x):
        w, b = self._wb(lay)
        z = x @ w + b
        return np.maximum(z, 0) if lay.act == "relu" else z

    @staticmethod
    def _softmax(z):
        e = np.exp(z - z.max(axis=-1, keepdims=True))
        return e / e.sum(axis=-1, keepdims=True)

    def represent(self, obs):
        spec = self.spec
        x = np.asarray(obs).astype(self.dtype)
        if spec.obs_kind != "float32":
            x = x / self.dtype(255.0)
        for lay in spec.rep:
            if lay.KH == 1 and lay.KW == 1 and lay.H == 1:
                x = self._dense(lay, x.reshape(x.shape[0], -1))
            else:
                w, b = self._wb(lay)
                win = np.lib.stride_tricks.sliding_window_view(x, (lay.KH, lay.KW), axis=(1, 2))[:, ::lay.S, ::lay.S]
                cols = np.ascontiguousarray(win.transpose(0, 1, 2, 4, 5, 3)).reshape(-1, lay.K)
                x = np.maximum(cols @ w + b, 0).reshape(x.shape[0], lay.OH, lay.OW, lay.N)
        return x.reshape(x.shape[0], -1)

    def predict_heads(self, h):
        q = h
        for lay in self.spec.pred[:-2]:
            q = self._dense(lay, q)
        return self._softmax(self._dense(self.spec.pred[-1], q)), self._softmax(self._dense(self.spec.pred[-2], q))

    def initial(self, obs):
        """-> policy [B, A], value support [B, V], hidden [B, H]"""
        h = self.represent(obs)
        p, v = self.predict_heads(h)
        return p, v, h

    def recurrent(self, hidden, action):
        """-> hidden [B, H], reward support [B, R], policy, value support"""
        hidden = np.asarray(hidden).astype(self.dtype).reshape(-1, self.spec.hidden)
        a = np.asarray(action).reshape(-1)
        onehot = (np.arange(self.spec.action_dim)[None, :] == a[:, None]).astype(self.dtype)
        t = np.concatenate([hidden, onehot], axis=1)
        for lay in self.spec.dyn[:-2]:
            t = self._dense(lay, t)
        h = self._dense(self.spec.dyn[-2], t)
        r = self._softmax(self._dense(self.spec.dyn[-1], t))
        p, v = self.predict_heads(h)
        return h, r, p, v


# ---------------------------------------------------------------------- the learner network on the device
class HipMuzero(object):
    """Flat parameter / gradient / Adam buffers as torch tensors and the ``xt_mz`` handle bound to them.  The handle and its
    workspace are sized for ``max_batch`` rows and grow when a larger batch arrives."""

    inference_only = False
    OPT_M, OPT_V, OPT_B1, OPT_B2, OPT_STEP = "/Adam", "/Adam_1", "beta1_power", "beta2_power", "adam_step"

    def __init__(self, spec, max_batch=32, device="cuda:0", seed=None, lr=1e-3):
        import torch
        from xingtian_amd import lib as L
        L.require_gpu()
        self.torch, self.L, self.lib = torch, L, L.load()
        self.spec, self.device = spec, torch.device(device)
        n = spec.n_flat
        flat = np.zeros(n, np.float32)
        for name, val in initial_weights(spec, seed).items():
            spec.var_view(flat, name)[...] = val
        self.params = torch.from_numpy(flat).to(self.device)
        self.grads = torch.zeros(n, dtype=torch.float32, device=self.device)
        self.adam_m = torch.zeros(n, dtype=torch.float32, device=self.device)
        self.adam_v = torch.zeros(n, dtype=torch.float32, device=self.device)
        self.adam_state = torch.zeros(8, dtype=torch.float32, device=self.device)
        self.loss_dev = torch.zeros(1, dtype=torch.float64, device=self.device)
        self.cfg = L.MzCfg(lr=float(lr), beta1=0.9, beta2=0.999, eps=1e-8)
        self.handle, self.max_batch, self.workspace = None, 0, None
        with torch.cuda.device(self.device):
            L.check(self.lib.xt_adam_state_init(L.ptr(self.adam_state), L.stream_ptr()), "xt_adam_state_init")
        self._ensure(max_batch)

    def _chain(self, layers):
        L = self.L
        arr = (L.LayerDesc * len(layers))()
        for i, lay in enumerate(layers):
            for f in ("H", "W", "C", "KH", "KW", "S", "PT", "PL", "OH", "OW", "N"):
                setattr(arr[i].g, f, getattr(lay, f))
            arr[i].g.act = L.ACT[lay.act]
            arr[i].param_off = lay.param_off
        return arr

    def _ensure(self, batch):
        if batch <= self.max_batch:
            return
        L, spec, torch = self.L, self.spec, self.torch
        if self.handle is not None:
            torch.cuda.synchronize(self.device)
            self.lib.xt_mz_destroy(self.handle)
            self.handle = None
        self._chains = [self._chain(c) for c in (spec.rep, spec.dyn, spec.pred)]
        d = L.MzDesc()
        d.n_rep, d.n_dyn, d.n_pred = len(spec.rep), len(spec.dyn), len(spec.pred)
        d.rep, d.dyn, d.pred = self._chains
        d.hidden, d.action_dim, d.unroll = spec.hidden, spec.action_dim, spec.unroll
        d.value_support, d.reward_support = spec.value_support, spec.reward_support
        d.obs_dim = spec.rep[0].C
        d.n_params = spec.n_flat
        d.value_min, d.value_max, d.reward_min, d.reward_max = spec.value_min, spec.value_max, spec.reward_min, spec.reward_max
        handle = ctypes.c_void_p()
        L.check(self.lib.xt_mz_create(ctypes.byref(d), int(batch), ctypes.byref(handle)), "xt_mz_create")
        nbytes = int(self.lib.xt_mz_workspace_bytes(handle))
        self.workspace = torch.zeros((nbytes + 3) // 4, dtype=torch.float32, device=self.device)
        L.check(self.lib.xt_mz_bind(handle, L.ptr(self.params), L.ptr(self.grads), L.ptr(self.adam_m), L.ptr(self.adam_v),
                                    L.ptr(self.adam_state), L.ptr(self.workspace), nbytes), "xt_mz_bind")
        self.handle, self.max_batch = handle, int(batch)

    def __del__(self):
        try:
            if self.handle is not None:
                self.torch.cuda.synchronize(self.device)
                self.lib.xt_mz_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    def _dev(self, array):
        return self.torch.from_numpy(np.ascontiguousarray(array)).to(self.device)

    def _obs(self, obs):
        """the observations as the device reads them: contiguous float32 [rows, obs_dim]; anything else is refused here,
        before a kernel reads past a buffer of another element size"""
        torch = self.torch
        if not torch.is_tensor(obs):
            obs = np.asarray(obs)
            if obs.dtype != np.float32:
                raise TypeError("observations must be float32 (got {})".format(obs.dtype))
            obs = self._dev(obs)
        if obs.dtype != torch.float32 or obs.dim() != 2 or int(obs.shape[1]) != self.spec.rep[0].C or not obs.is_contiguous():
            raise TypeError("observations must be a contiguous float32 [rows, {}] array (got {} {})".format(
                self.spec.rep[0].C, obs.dtype, tuple(obs.shape)))
        return obs

    # ---- the update
    def grad_step(self, obs, actions, target_value, target_reward, target_policy, idx=None):
        """forward + loss + backward of one batch (no optimiser step) -> the loss as a device tensor of one float64.
        obs: the array the first layer is fed (``obs_as_network_input``), or a device tensor of it."""
        L, torch, spec = self.L, self.torch, self.spec
        obs = self._obs(obs)
        b = int(len(idx)) if idx is not None else int(obs.shape[0])
        actions = np.asarray(actions).reshape(b, -1)
        if actions.shape[1] != spec.unroll:
            raise ValueError("train: actions carry {} columns, the model unrolls td_step = {}".format(actions.shape[1], spec.unroll))
        tv = np.asarray(target_value, np.float64).reshape(b, -1)
        tr = np.asarray(target_reward, np.float64).reshape(b, -1)
        tp = np.asarray(target_policy, np.float32).reshape(b, -1, spec.action_dim)
        if tv.shape[1] != spec.unroll + 1 or tr.shape[1] != spec.unroll + 1 or tp.shape[1] != spec.unroll + 1:
            raise ValueError("train: targets must carry td_step + 1 = {} columns".format(spec.unroll + 1))
        self._ensure(b)
        self._keep = (obs, self._dev(actions.astype(np.int32)), self._dev(tv), self._dev(tr), self._dev(tp),
                      None if idx is None else self._dev(np.asarray(idx, np.int32)))
        o, a, v, r, p, i = self._keep
        with torch.cuda.device(self.device):
            L.check(self.lib.xt_mz_step(self.handle, L.ptr(o), L.ptr(i), b, L.ptr(a), L.ptr(v), L.ptr(r), L.ptr(p),
                                        ctypes.byref(self.cfg), L.ptr(self.loss_dev), L.stream_ptr()), "xt_mz_step")
        return self.loss_dev

    def apply(self):
        with self.torch.cuda.device(self.device):
            self.L.check(self.lib.xt_mz_apply(self.handle, ctypes.byref(self.cfg), self.L.stream_ptr()), "xt_mz_apply")

    def train_step(self, obs, actions, target_value, target_reward, target_policy):
        loss = self.grad_step(obs, actions, target_value, target_reward, target_policy)
        self.apply()
        return float(loss.item())

    # ---- inference
    def initial(self, obs):
        L, torch, spec = self.L, self.torch, self.spec
        obs = self._obs(obs)
        b = int(obs.shape[0])
        self._ensure(b)
        p = torch.empty((b, spec.action_dim), dtype=torch.float32, device=self.device)
        v = torch.empty((b, spec.value_support), dtype=torch.float32, device=self.device)
        h = torch.empty((b, spec.hidden), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            L.check(self.lib.xt_mz_initial(self.handle, L.ptr(obs), None, b, L.ptr(p), L.ptr(v), L.ptr(h), L.stream_ptr()),
                    "xt_mz_initial")
        return p.cpu().numpy(), v.cpu().numpy(), h.cpu().numpy()

    def recurrent(self, hidden, action):
        L, torch, spec = self.L, self.torch, self.spec
        hid = self._dev(np.asarray(hidden, np.float32).reshape(-1, spec.hidden))
        b = int(hid.shape[0])
        act = self._dev(np.asarray(action, np.int32).reshape(b))
        self._ensure(b)
        h = torch.empty((b, spec.hidden), dtype=torch.float32, device=self.device)
        r = torch.empty((b, spec.reward_support), dtype=torch.float32, device=self.device)
        p = torch.empty((b, spec.action_dim), dtype=torch.float32, device=self.device)
        v = torch.empty((b, spec.value_support), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            L.check(self.lib.xt_mz_recurrent(self.handle, L.ptr(hid), L.ptr(act), b, L.ptr(h), L.ptr(r), L.ptr(p), L.ptr(v),
                                             L.stream_ptr()), "xt_mz_recurrent")
        return h.cpu().numpy(), r.cpu().numpy(), p.cpu().numpy(), v.cpu().numpy()

    # ---- weights and optimiser state by name
    def _views(self, flat):
        return OrderedDict((n, self.spec.var_view(flat, n)) for n in self.spec.names)

    def get_weights(self, copy=True):
        return self._views(self.params.detach().cpu().numpy().copy())

    def get_gradients(self):
        return self._views(self.grads.detach().cpu().numpy().copy())

    def set_weights(self, weights):
        weights = weights_as_dict(self.spec, weights)
        hit = [k for k in weights.keys() if k in self.spec.names]
        if not hit:
            raise KeyError("NO node's weights could assign in self.graph {} vs {}".format(list(self.spec.names), list(weights.keys())))
        flat = self.params.detach().cpu().numpy().copy()
        for name in hit:
            val = np.asarray(weights[name], np.float32)
            if tuple(val.shape) != tuple(self.spec.names[name][1]):
                raise KeyError("update {} encounter error: shape {} vs {}".format(name, val.shape, self.spec.names[name][1]))
            self.spec.var_view(flat, name)[...] = val
        self.params.copy_(self.torch.from_numpy(flat))

    def publish_weights(self, ring, ctr_info=None, lag=0):
        return ring.publish_flat_host(self.params.detach().cpu().numpy(), self.spec, ctr_info)

    def get_optimizer_state(self):
        m, v = self.adam_m.detach().cpu().numpy(), self.adam_v.detach().cpu().numpy()
        st = self.adam_state.detach().cpu().numpy()
        out = OrderedDict()
        for name in self.spec.names:
            out[name + self.OPT_M] = self.spec.var_view(m, name).copy()
            out[name + self.OPT_V] = self.spec.var_view(v, name).copy()
        out[self.OPT_B1], out[self.OPT_B2] = np.float32(st[0]), np.float32(st[1])
        out[self.OPT_STEP] = np.int64(round(float(st[5])))
        return out

    def set_optimizer_state(self, state):
        """-> False (nothing touched) unless every slot and both beta powers are present"""
        need = [n + s for n in self.spec.names for s in (self.OPT_M, self.OPT_V)] + [self.OPT_B1, self.OPT_B2]
        if any(k not in state for k in need):
            return False
        m, v = np.zeros(self.spec.n_flat, np.float32), np.zeros(self.spec.n_flat, np.float32)
        for name, (_, shape) in self.spec.names.items():
            for sfx, dst in ((self.OPT_M, m), (self.OPT_V, v)):
                val = np.asarray(state[name + sfx], np.float32)
                if tuple(val.shape) != tuple(shape):
                    raise KeyError("optimizer slot {} shape {} vs {}".format(name + sfx, val.shape, shape))
                self.spec.var_view(dst, name)[...] = val
        st = self.adam_state.detach().cpu().numpy().copy()
        st[0], st[1] = np.float32(state[self.OPT_B1]), np.float32(state[self.OPT_B2])
        st[5] = np.float32(state[self.OPT_STEP]) if self.OPT_STEP in state else 0.0
        self.adam_m.copy_(self.torch.from_numpy(m))
        self.adam_v.copy_(self.torch.from_numpy(v))
        self.adam_state.copy_(self.torch.from_numpy(st))
        return True


# ---------------------------------------------------------------------- the model plugin
@Registers.model
class MuzeroModel(XTModel):
    """Base of ``MuzeroMlp`` / ``MuzeroCnn``: the reference's public methods on the device network (learner) or on the
    NumPy replica (explorers).  The reported loss leaves the reference's constant weight-decay term out."""

    def __init__(self, model_info):
        cfg = model_info.get("model_config") or {}
        self.state_dim = model_info["state_dim"]
        self.action_dim = model_info["action_dim"]
        self.reward_min, self.reward_max = cfg.get("reward_min", -300), cfg.get("reward_max", 300)
        self.value_min, self.value_max = cfg.get("value_min", 0), cfg.get("value_max", 60000)
        self.obs_type = cfg.get("obs_type", "float32")
        self.td_step = int(cfg.get("td_step", _defaults.td_step))
        self.lr = float(cfg.get("LR", _defaults.LR))
        self.weight_decay = WEIGHT_DECAY
        super().__init__(model_info)

    def make_spec(self, model_info):
        raise NotImplementedError("MuzeroModel is the base class: use MuzeroMlp or MuzeroCnn")

    def create_model(self, model_info):
        cfg = model_info.get("model_config") or {}
        self.spec = self.make_spec(model_info)
        self.reward_support_size, self.value_support_size = self.spec.reward_support, self.spec.value_support
        seed = cfg.get("SEED")
        if wants_cpu_replica(model_info):
            self.net = CpuMuzero(self.spec, seed=seed)
        else:
            if len(self.spec.state_dim) == 3:
                raise NotImplementedError(
                    "{}: the device update takes Dense representation chains on float32 vectors only (MuzeroMlp); this "
                    "model builds as the inference-only replica (model_config DEVICE: 'cpu', or any process that is not "
                    "the learner)".format(type(self).__name__))
            self.net = HipMuzero(self.spec, max_batch=int(cfg.get("MAX_BATCH", 32)), device=learner_device(model_info),
                                 seed=seed, lr=self.lr)
        return self.net

    # ---- the reference's host helpers as methods
    def conver_value(self, target_value, support_size, min, max):      # noqa: A002  (the reference's argument names)
        return conver_value(target_value, support_size, min, max)

    def value_transform(self, value_support, support_size, min, max):  # noqa: A002
        return value_transform(value_support, support_size, min, max)

    def _input(self, obs):
        return obs_as_network_input(self.spec, obs, self.obs_type)

    # ---- update
    def train(self, state, label):
        """state = [obs [B, ...], actions [B, td_step], loss_weights [B, 1] (unused)], label = [target_value [B, td_step + 1],
        target_reward [B, td_step + 1], target_policy [B, td_step + 1, A]] -> the loss (without the constant decay term)"""
        self._require_learner()
        return self.net.train_step(self._input(state[0]), state[1], label[0], label[1], label[2])

    # ---- inference
    def initial_inference(self, input_data):
        policy, value, hidden = self.net.initial(self._input(input_data))
        value = self.value_transform(value[0], self.value_support_size, self.value_min, self.value_max)
        return NetworkOutput(value, 0, policy[0], hidden[0])

    def recurrent_inference(self, hidden_state, action):
        hidden, reward, policy, value = self.net.recurrent(np.expand_dims(hidden_state, 0), [action])
        value = self.value_transform(value[0], self.value_support_size, self.value_min, self.value_max)
        reward = self.value_transform(reward[0], self.reward_support_size, self.reward_min, self.reward_max)
        return NetworkOutput(value, reward, policy[0], hidden[0])

    def value_inference(self, input_data):
        _, value, _ = self.net.initial(self._input(input_data))
        return np.asarray([self.value_transform(v, self.value_support_size, self.value_min, self.value_max) for v in value])

    def predict(self, state):
        return self.net.initial(self._input(state))
