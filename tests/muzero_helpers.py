"""Checkers of the MuZero tests: a float64 torch restatement of the update's arithmetic, written from its semantics
(include/xt_mi355x.h, "MuZero"; the model's docstring), the float64 twin of ``xt_mz_loss``, the NumPy twin of the
conditioned dynamics layer in the kernels' own summation order (bit for bit), and TensorFlow-1 Adam in float64.

The reference's graph-building code (``MuzeroModel.build_train_graph``) does NOT execute under ``oracle/tf_shim.py``: it is
built from Keras ``Model`` / ``Input`` / ``Dense`` objects, placeholders and ``sess.run``, none of which that minimal eager
look-alike has.  So no loss or gradient of a reference train is recorded; the restatement below is the oracle for them,
and ``tests/test_cpu_muzero.py`` shows that it is not blind to the four ways of getting the unroll's gradient wrong.  The
reference's host code (value compression, ``conver_value``, ``value_transform``, ``make_target``, the prioritised
buffers, ``prepare_data`` / ``train`` / ``update_pri``) IS executed: ``tools/gen_golden_muzero.py`` records
``tests/golden/muzero_host.npz``.

Bars: the project's standing ones by ``dqn_helpers.rel_max`` -- loss 1e-4, every gradient tensor 1e-5; a tensor whose
float64 gradient is exactly zero is compared absolutely.  A float32 restatement of the same graph deviates from float64
by <= 1.4e-7 (loss) and <= 4.2e-7 (worst gradient tensor) at the shapes tried, so the bars leave more than a factor 20.
"""
import numpy as np
import torch

from tests.dqn_helpers import rel_max

BAR_LOSS, BAR_GRAD = 1e-4, 1e-5
BAR_ADAM = 2e-6       # tests/test_gpu_optim_branch.py: BAR_ELEM, the bar of Adam's element-wise outputs
F64 = torch.float64


def scale_gradient(x, s):
    return x * s + x.detach() * (1 - s)


def compress(x):
    return np.sign(x) * (np.sqrt(np.abs(x) + 1) - 1) + 0.001 * x


def two_hot(t, n, tmin, tmax):
    """float64 [..., n] rows of scalars ``t``: 1 - rest on floor, rest on floor + 1; the whole mass on bin n - 1 at the top"""
    t = np.asarray(t, np.float64)
    c = compress(np.clip(t, tmin, tmax) - tmin)
    fl = np.floor(c)
    rest = c - fl
    out = np.zeros(t.shape + (n,))
    it = np.nditer(fl, flags=["multi_index"])
    for f in it:
        i, ix = int(f), it.multi_index
        if i >= n - 1:
            out[ix + (n - 1,)] = 1.0
        else:
            out[ix + (i,)] = np.float32(1.0 - rest[ix])
            out[ix + (i + 1,)] = np.float32(rest[ix])
    return out


def ce(p, t):
    return torch.mean(torch.mean(-t * torch.log(p + 1e-10), dim=-1, keepdim=True))


def t64(x):
    return torch.as_tensor(np.asarray(x, np.float64))


def network_input(spec, obs, obs_type):
    """float64 [B, ...] as the reference's graph sees the observation: int8 wraps, the CNN divides by 255"""
    x = np.asarray(obs)
    if obs_type == "int8":
        x = x.view(np.int8) if x.dtype == np.uint8 else x.astype(np.int8)
    x = x.astype(np.float64)
    return x / 255.0 if spec.obs_kind != "float32" else x


class Twin(object):
    """The three networks in float64 on leaf tensors keyed like the model's weights."""

    def __init__(self, spec, weights):
        self.spec = spec
        self.w = {k: t64(v).requires_grad_(True) for k, v in weights.items()}

    def dense(self, lay, x):
        z = x @ self.w[lay.name + "/kernel"].reshape(-1, lay.N) + self.w[lay.name + "/bias"]      # (a whole-image conv kernel is a Dense one)
        return torch.relu(z) if lay.act == "relu" else z

    def rep(self, x):
        for lay in self.spec.rep:
            if lay.KH == 1 and lay.KW == 1 and lay.H == 1:
                x = self.dense(lay, x.reshape(x.shape[0], -1))
            else:
                k = self.w[lay.name + "/kernel"].permute(3, 2, 0, 1)          # HWIO -> OIHW
                y = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2), k, self.w[lay.name + "/bias"], stride=lay.S)
                x = torch.relu(y).permute(0, 2, 3, 1)                        # NHWC: Flatten runs in (H, W, C) order
        return x.reshape(x.shape[0], -1)

    def dyn(self, h, action):
        onehot = torch.nn.functional.one_hot(torch.as_tensor(np.asarray(action, np.int64)), self.spec.action_dim).to(F64)
        t = torch.cat([h, onehot], dim=-1)
        for lay in self.spec.dyn[:-2]:
            t = self.dense(lay, t)
        return self.dense(self.spec.dyn[-2], t), torch.softmax(self.dense(self.spec.dyn[-1], t), dim=-1)

    def pred(self, h):
        q = h
        for lay in self.spec.pred[:-2]:
            q = self.dense(lay, q)
        return torch.softmax(self.dense(self.spec.pred[-1], q), dim=-1), torch.softmax(self.dense(self.spec.pred[-2], q), dim=-1)

    def loss(self, x, actions, tv, tr, tp, hidden_scale=0.5, scale_h0=False, step_factor=True, reward_shift=0):
        """L and, through autograd, its gradient.  The keyword arguments are the four WRONG variants the blindness test
        switches on one at a time; the defaults are the definition."""
        s = self.spec
        u = s.unroll
        zv = t64(two_hot(tv, s.value_support, s.value_min, s.value_max))
        zr = t64(two_hot(tr, s.reward_support, s.reward_min, s.reward_max))
        pi = t64(tp)
        h = self.rep(t64(x))
        p, v = self.pred(h)
        if scale_h0:
            h = scale_gradient(h, hidden_scale)
        total = ce(p, pi[:, 0]) + ce(v, zv[:, 0])
        for i in range(u):
            h, r = self.dyn(h, np.asarray(actions)[:, i])
            p, v = self.pred(h)
            h = scale_gradient(h, hidden_scale)
            l = ce(r, zr[:, i + reward_shift]) + ce(p, pi[:, i + 1]) + ce(v, zv[:, i + 1])
            total = total + (scale_gradient(l, 1.0 / u) if step_factor else l)
        return total

    def loss_and_grads(self, *args, **kw):
        for t in self.w.values():
            t.grad = None
        total = self.loss(*args, **kw)
        total.backward()
        return float(total.detach()), {k: (t.grad.numpy().copy() if t.grad is not None else np.zeros(tuple(t.shape))) for k, t in self.w.items()}

    def initial(self, x):
        with torch.no_grad():
            h = self.rep(t64(x))
            p, v = self.pred(h)
        return p.numpy(), v.numpy(), h.numpy()

    def recurrent(self, hidden, action):
        with torch.no_grad():
            h, r = self.dyn(t64(hidden), action)
            p, v = self.pred(h)
        return h.numpy(), r.numpy(), p.numpy(), v.numpy()


def grad_errors(got, ref):
    """{name: (error, kind)}: relative to the reference tensor's largest magnitude, or absolute where it is exactly zero"""
    out = {}
    for k, r in ref.items():
        if np.abs(r).max() == 0.0:
            out[k] = (float(np.abs(np.asarray(got[k], np.float64)).max()), "abs")
        else:
            out[k] = (rel_max(got[k], r), "rel")
    return out


def adam_tf(p, g, m, v, t, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8):
    """one step of tf.train.AdamOptimizer in float64 -> (p, m, v); t = the step's number from 1"""
    lr_t = lr * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
    m = m + (g - m) * (1.0 - b1)
    v = v + (g * g - v) * (1.0 - b2)
    return p - lr_t * m / (np.sqrt(v) + eps), m, v


# ---------------------------------------------------------------------- xt_mz_loss in float64
def loss_twin(logits, nblk, b, target_rows, scale0, scale_rest):
    """logits [nblk * b, n] (float32 values), target_rows [nblk * b, n] float64 in the kernel's row order ->
    (p, dz, rowloss) float64"""
    z = np.asarray(logits, np.float64)
    n = z.shape[1]
    e = np.exp(z - z.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    w = target_rows / (p + 1e-10)
    s = np.where(np.arange(nblk * b) // b == 0, scale0, scale_rest).astype(np.float64)[:, None] / (b * n)
    dz = s * p * ((w * p).sum(axis=1, keepdims=True) - w)
    rowloss = -(target_rows * np.log(p + 1e-10)).sum(axis=1) / (b * n)
    return p, dz, rowloss


# ---------------------------------------------------------------------- the conditioned layer, bit for bit
WGRAD_ROWS = 128


def cond_fwd_twin(h, actions, w, bias, hidden, relu=True):
    """y = act(((sum_k ascending h_k w[k]) + w[hidden + a]) + bias) in float32, one rounding per operation"""
    h, w, bias = np.asarray(h, np.float32), np.asarray(w, np.float32), np.asarray(bias, np.float32)
    acc = np.zeros((h.shape[0], w.shape[1]), np.float32)
    for k in range(hidden):
        acc = acc + h[:, k:k + 1] * w[k][None, :]
    a = np.asarray(actions).reshape(-1)
    ok = (a >= 0) & (a < w.shape[0] - hidden)
    acc = np.where(ok[:, None], acc + w[hidden + np.clip(a, 0, w.shape[0] - hidden - 1)], acc)
    acc = acc + bias[None, :]
    return np.maximum(acc, np.float32(0)) if relu else acc


def cond_bwd_twin(h, actions, w, dy, g_pred, c, hidden, n_actions):
    """-> (g [M, hidden], dwb [(hidden + A + 1) * N]) in the kernels' order: rows ascending inside slabs of WGRAD_ROWS rows,
    the slabs ascending from 0.0f; dh over ascending n; g = relu'(h) * (g_pred + c * dh)"""
    h, w, dy = np.asarray(h, np.float32), np.asarray(w, np.float32), np.asarray(dy, np.float32)
    m, n = dy.shape
    a = np.asarray(actions).reshape(-1)
    rows = hidden + n_actions + 1
    slabs = []
    for r0 in range(0, m, WGRAD_ROWS):
        acc = np.zeros((rows, n), np.float32)
        for r in range(r0, min(r0 + WGRAD_ROWS, m)):
            acc[:hidden] = acc[:hidden] + h[r][:, None] * dy[r][None, :]
            if 0 <= a[r] < n_actions:
                acc[hidden + a[r]] = acc[hidden + a[r]] + dy[r]
            acc[rows - 1] = acc[rows - 1] + dy[r]
        slabs.append(acc)
    if len(slabs) == 1:
        dwb = slabs[0]
    else:
        dwb = np.zeros((rows, n), np.float32)
        for s in slabs:
            dwb = dwb + s
    dh = np.zeros((m, hidden), np.float32)
    for j in range(n):
        dh = dh + dy[:, j:j + 1] * w[:hidden, j][None, :]
    g = np.float32(c) * dh
    if g_pred is not None:
        g = np.asarray(g_pred, np.float32) + g
    g = np.where(h > 0, g, np.float32(0))
    return g.astype(np.float32), dwb.reshape(-1)


# ---------------------------------------------------------------------- shared inputs
def make_batch(spec, b, seed, obs_type="float32", top_and_bottom=True):
    """seeded observations, actions and targets of one train; value / reward targets touch min, max and an exact integer
    of the compressed scale when ``top_and_bottom``"""
    rng = np.random.default_rng(seed)
    u, a = spec.unroll, spec.action_dim
    if len(spec.state_dim) == 3:
        obs = rng.integers(0, 256, (b,) + spec.state_dim).astype(np.uint8)
        if obs_type == "float32":
            obs = obs.astype(np.float32)
    else:
        obs = rng.standard_normal((b,) + spec.state_dim).astype(np.float32)
    actions = rng.integers(0, a, (b, u)).astype(np.int32)
    tv = rng.uniform(spec.value_min, spec.value_max, (b, u + 1))
    tr = rng.uniform(spec.reward_min, spec.reward_max, (b, u + 1))
    if top_and_bottom:
        tv.flat[0], tv.flat[-1] = spec.value_max + 5.0, spec.value_min - 5.0
        tr.flat[0], tr.flat[-1] = spec.reward_max, spec.reward_min
        tv.flat[1] = spec.value_min + 8.024          # compresses to exactly 2 + 0.008024: not an integer, but next to one
        tr.flat[1] = spec.reward_min
    tp = rng.random((b, u + 1, a)).astype(np.float32)
    tp /= tp.sum(axis=-1, keepdims=True)
    return obs, actions, tv, tr, tp


def seeded_weights(spec, seed, bias_scale=0.05):
    """glorot kernels and NON-zero biases (a zero bias hides a wrong bias gradient's consequences in later steps)"""
    from xingtian_amd.model.cpu_net import initial_weights
    w = initial_weights(spec, seed)
    rng = np.random.default_rng(seed + 1000)
    for k in w:
        if k.endswith("/bias"):
            w[k] = (rng.standard_normal(w[k].shape) * bias_scale).astype(np.float32)
    return w
