"""``DqnCnn``: the Q-network of the ``DQN`` algorithm on HIP kernels (base class of ``DqnMlp`` too).

Reference: a Keras model with one linear output Q [N, A] -- with ``model_config.dueling`` the 1-wide stream ``s`` and
the A-wide stream ``l`` combine to Q_a = s + (l_a - mean_a l) -- compiled with ``loss='mse'`` and ``tf.keras`` Adam
(xt/model/dqn/dqn_cnn.py:45-61: ``clipnorm=10.``; xt/model/dqn/dqn_mlp.py:43-58: plain Adam).  ``predict(state)``
returns Q as float32 [N, A].  The update does not go through ``train(states, y_t)``: the algorithm keeps its replay
store on the device and one C call (``xt_net_dqn_step``) forms the TD target and the gradient there
(``train_replay``), so ``train`` is not provided.  ``train_replay`` and ``train_replay_per`` are one call of
``HipActorCritic.dqn_step``, whose keywords (``follow`` / ``n``, ``per``, ``dist``, ``quant``) choose among the five C
entries.

``model_config.atoms`` (1 unless asked for) with ``v_min`` / ``v_max`` (-10 / 10) makes the network distributional (C51,
Bellemare et al. 2017): the Q head is A * atoms wide, column a * atoms + i being the logit of atom i of action a, and
``predict`` returns the expectation of every action's softmax over the fixed support (``dist_q``).  The definitions
below (``dist_support``, ``dist_q``, ``categorical_projection``) are the host twins of the head kernel
``xt_dqn_loss_dist``: the same arithmetic in the same precision, and the tests' first reference.

``model_config.quantiles`` (1 unless asked for) with ``kappa`` (1.0) makes it a quantile-regression network instead
(QR-DQN, Dabney et al. 2018): the Q head is A * quantiles wide, column a * quantiles + i being quantile i of action a at
the midpoint tau_i = (2 i + 1) / (2 N); there is no support to choose.  ``predict`` returns the mean of every action's
quantiles (``quant_q``).  ``quantile_midpoints``, ``quant_q`` and ``quantile_huber`` are the host twins of the head kernel
``xt_dqn_loss_quant``.  A network is one or the other, never both.

``model_config.noisy`` (false unless asked for) with ``noisy_sigma0`` (0.5) and ``NOISY_PREDICT_MEAN`` (false) makes the
last trunk layer, the Q head and the dueling stream noisy (NoisyNet, Fortunato et al. 2018, factorised Gaussian): the
variables ``<layer>/kernel`` / ``bias`` hold the means, ``<layer>/sigma_kernel`` / ``sigma_bias`` are new, and the layer
runs on W_eff = mu + sigma * (f_in f_out^T) with vectors drawn from a counter-based generator keyed by (``SEED``, call,
stream).  ``noisy_philox`` ... ``noisy_sigma_grads`` are the host twins of ``xt_noisy_compose`` / ``xt_noisy_grads``
("Noisy layers"), and what the CPU replica composes with.

``model_config.dist_dueling`` (false unless asked for; with ``atoms`` or ``quantiles`` > 1 only) makes the distributional
or quantile network dueling, the architecture of Rainbow: the Q head is (A + 1) * N wide, group a < A the advantages of
action a and group A the state-value stream, and everything the two heads read as an action's logits / quantiles is
l[a, i] = v[i] + (adv[a, i] - mean_a adv[a, i]) (``dist_dueling_combine``, the host twin of what ``xt_dqn_loss_dist_duel`` /
``xt_dqn_loss_quant_duel`` do on the fly; ``dist_dueling_combine_grad`` is its transpose).  ``predict`` combines first.  The
key ``dueling`` keeps meaning the 1-wide stream of the scalar head and stays refused with ``atoms`` / ``quantiles``.
"""
import numpy as np

from xingtian_amd.model import netspec
from xingtian_amd.model.dqn.default_config import LR  # noqa: F401
from xingtian_amd.model.model import XTModel, as_numpy, build_net
from xingtian_amd.register import Registers, import_config

PONG_MESSAGE = ("DqnCnnPong is not supported: its input dtype is int8, for which the input transform has no mode "
                "(uint8 and float32 only)")


def dueling_q(logits, value, dueling):
    """Q [N, A] float32 from the two heads: the A-wide head as it is, or s + (l - mean_a l) with the 1-wide head s."""
    l = np.asarray(logits, np.float32)
    if not dueling:
        return l
    return np.asarray(value, np.float32).reshape(-1, 1) + (l - l.mean(axis=1, keepdims=True, dtype=np.float32))


def dist_support(atoms, v_min, v_max):
    """-> (z float64 [N], delta): delta = (v_max - v_min) / (N - 1), z_i = v_min + i * delta, both in float64 (product
    rounded, then sum).  ``z.astype(float32)`` is used where float32 is used."""
    n, v_min, v_max = int(atoms), np.float64(v_min), np.float64(v_max)
    if n < 2 or not (np.isfinite(v_min) and np.isfinite(v_max) and v_min < v_max):
        raise ValueError("dist_support: needs atoms >= 2 and finite v_min < v_max (got {}, {}, {})".format(atoms, v_min, v_max))
    delta = (v_max - v_min) / np.float64(n - 1)
    return v_min + np.arange(n, dtype=np.float64) * delta, delta


def dist_q(logits, z):
    """Expectation of softmax(l) over the support, float32, for logits [..., N] and the float64 support ``z`` [N]:
    mx = max l; e_i = expf(l_i - mx); Q = (sum z_i e_i) / (sum e_i) with z_i rounded to float32.  -> float32 [...]"""
    l = np.asarray(logits, np.float32)
    e = np.exp(l - l.max(axis=-1, keepdims=True), dtype=np.float32)
    zf = np.asarray(z, np.float64).astype(np.float32)
    return ((zf * e).sum(axis=-1, dtype=np.float32) / e.sum(axis=-1, dtype=np.float32)).astype(np.float32)


def categorical_projection(p, reward, disc, done, v_min, v_max):
    """The target distribution of C51 projected onto the support (Algorithm 1 of the paper in gather form), float64 with
    one rounding: for probabilities ``p`` [B, N] (float32) and per-sample labels (R, g, dn),

        Tz_j = clip(dn ? R : R + g * z_j, v_min, v_max);  b_j = (Tz_j - v_min) / delta
        m_i = (float32) sum_{j = 0..N-1, ascending} (float64)p_j * max(0, 1 - |b_j - i|)

    It equals the published l = floor(b) / u = ceil(b) scatter whenever no b_j is an integer, and keeps the mass where
    that pseudo-code drops it (l == u).  Nothing is scattered, so no order of evaluation enters.  -> m float32 [B, N]"""
    p = np.asarray(p, np.float32)
    b, n = p.shape
    z, delta = dist_support(n, v_min, v_max)
    r = np.asarray(reward, np.float64).reshape(b, 1)
    g = np.broadcast_to(np.asarray(disc, np.float64).reshape(-1, 1), (b, 1))
    dn = np.asarray(done).reshape(b, 1).astype(bool)
    gz = g * z[None, :]
    tz = np.clip(np.where(dn, r, r + gz), np.float64(v_min), np.float64(v_max))
    bj = (tz - np.float64(v_min)) / delta
    idx = np.arange(n, dtype=np.float64)
    m = np.zeros((b, n), np.float64)
    for j in range(n):                                  # ascending j: the kernel's order of summation
        m = m + p[:, j:j + 1].astype(np.float64) * np.maximum(0.0, 1.0 - np.abs(bj[:, j:j + 1] - idx[None, :]))
    return m.astype(np.float32)


def dist_dueling_combine(cols, n_actions, n):
    """The dueling combine of a folded head's output ``cols`` [B, (A + 1) * N] (float32): adv[a, i] = cols[a N + i],
    v[i] = cols[A N + i], mean_i = (sum over ascending a of adv[a, i]) / (float32)A, l[a, i] = v[i] + (adv[a, i] - mean_i).
    -> l float32 [B, A, N]"""
    a, n = int(n_actions), int(n)
    c = np.asarray(cols, np.float32).reshape(-1, a + 1, n)
    s = np.zeros((c.shape[0], n), np.float32)
    for k in range(a):                                  # ascending a: the kernel's order of summation
        s = s + c[:, k]
    mean = s / np.float32(a)
    return c[:, a:a + 1] + (c[:, :a] - mean[:, None, :])


def dist_dueling_combine_grad(d, action, n_actions):
    """The gradient of a folded row from d_i = d loss / d l[act, i] (``d`` float32 [B, N], ``action`` already inside
    [0, A)): dcol[a N + i] = d_i * (hot(a == act) - inv_A) with inv_A = 1 / (float32)A for every a < A, dcol[A N + i] = d_i.
    -> float32 [B, (A + 1) * N]"""
    a = int(n_actions)
    d = np.asarray(d, np.float32)
    hot = (np.arange(a)[None, :] == np.asarray(action).reshape(-1, 1)).astype(np.float32)
    inv_a = np.float32(1.0) / np.float32(a)
    adv = d[:, None, :] * (hot - inv_a)[:, :, None]
    return np.concatenate([adv, d[:, None, :]], axis=1).reshape(d.shape[0], -1)


def dist_dueling_config(model_config, action_dim):
    """-> ``dist_dueling`` of a DQN ``model_config`` after its checks (call it behind ``dist_config`` / ``quant_config``,
    whose refusal of ``dueling`` with ``atoms`` / ``quantiles`` comes first)"""
    return netspec.check_dist_dueling(model_config.get("dist_dueling", False), netspec.check_atoms(model_config.get("atoms", 1)),
                                      netspec.check_quantiles(model_config.get("quantiles", 1)), action_dim)


def dist_config(model_config, action_dim):
    """-> (atoms, v_min, v_max) of a DQN ``model_config`` after the checks of the distributional keys"""
    atoms = netspec.check_atoms(model_config.get("atoms", 1))
    v_min, v_max = float(model_config.get("v_min", -10.0)), float(model_config.get("v_max", 10.0))
    if atoms > 1:
        if not (np.isfinite(v_min) and np.isfinite(v_max) and v_min < v_max):
            raise ValueError("atoms = {}: the support needs finite v_min < v_max, got v_min = {}, v_max = {}".format(
                atoms, v_min, v_max))
        if bool(model_config.get("dueling", False)):
            raise NotImplementedError("dueling with atoms = {}: the dueling stream is 1 wide, a distributional dueling "
                                      "network needs an atoms-wide one; not provided (the folded form is the key "
                                      "dist_dueling)".format(atoms))
        if int(action_dim) > 64:
            raise ValueError("atoms = {}: action_dim = {} exceeds 64 (the device step's limit)".format(atoms, action_dim))
    return atoms, v_min, v_max


def quantile_midpoints(quantiles):
    """-> tau float64 [N]: tau_i = (2 i + 1) / (2 N)"""
    n = int(quantiles)
    if n < 1:
        raise ValueError("quantile_midpoints: needs quantiles >= 1 (got {})".format(quantiles))
    return (2.0 * np.arange(n, dtype=np.float64) + 1.0) / (2.0 * np.float64(n))


def quant_q(theta):
    """Mean of the quantiles [..., N] (float32): the float64 sum over ascending i, divided by N, rounded once.
    -> float32 [...]"""
    t = np.asarray(theta, np.float32)
    s = np.zeros(t.shape[:-1], np.float64)
    for i in range(t.shape[-1]):                        # ascending i: the kernel's order of summation
        s = s + t[..., i].astype(np.float64)
    return (s / np.float64(t.shape[-1])).astype(np.float32)


def quantile_huber(theta, target_theta, reward, disc, done, kappa):
    """The quantile-Huber loss of QR-DQN and its gradient, per sample, as the kernel forms them: for the online quantiles
    ``theta`` [B, N] of the taken action, the target net's quantiles ``target_theta`` [B, N] of the bootstrap action
    (float32) and per-sample labels (R, g, dn),

        T_j = (float32)(dn ? R : R + g * (float64)theta'_j);  u_ij = T_j - theta_i   (float32)
        wt_ij = u_ij < 0 ? (float32)(1 - tau_i) : (float32)tau_i
        H(u) = |u| <= kappa ? 0.5 u u : kappa (|u| - 0.5 kappa)                      (float32)
        r_i = (float32)((sum_{j ascending} (float64)(wt_ij * H(u_ij) / kappa)) / N)
        g_i = (float32)(-(sum_{j ascending} (float64)(wt_ij * clip(u_ij, -kappa, kappa) / kappa)) / N)

    -> (loss_b float32 [B] = sum_i r_i, g float32 [B, N] = d loss_b / d theta)"""
    th, tt = np.asarray(theta, np.float32), np.asarray(target_theta, np.float32)
    b, n = th.shape
    k = np.float32(kappa)
    if not (np.isfinite(k) and k > 0):
        raise ValueError("quantile_huber: kappa must be finite and > 0 (got {})".format(kappa))
    r = np.asarray(reward, np.float64).reshape(b, 1)
    g = np.broadcast_to(np.asarray(disc, np.float64).reshape(-1, 1), (b, 1))
    dn = np.asarray(done).reshape(b, 1).astype(bool)
    gt = g * tt.astype(np.float64)
    t = np.where(dn, r, r + gt).astype(np.float32)
    tau = quantile_midpoints(n)
    w_neg, w_pos = (1.0 - tau).astype(np.float32)[None, :], tau.astype(np.float32)[None, :]
    half = np.float32(0.5)
    sr, sg = np.zeros((b, n), np.float64), np.zeros((b, n), np.float64)
    for j in range(n):                                  # ascending j: the kernel's order of summation
        u = t[:, j:j + 1] - th
        wt = np.where(u < 0, w_neg, w_pos)
        au = np.abs(u)
        hub = np.where(au <= k, half * u * u, k * (au - half * k))
        sr = sr + (wt * hub / k).astype(np.float64)
        sg = sg + (wt * np.clip(u, -k, k) / k).astype(np.float64)
    r_i = (sr / np.float64(n)).astype(np.float32)
    return r_i.sum(axis=1, dtype=np.float32), (-sg / np.float64(n)).astype(np.float32)


def quant_config(model_config, action_dim):
    """-> (quantiles, kappa) of a DQN ``model_config`` after the checks of the quantile keys"""
    quantiles = netspec.check_quantiles(model_config.get("quantiles", 1))
    kappa = float(model_config.get("kappa", 1.0))
    if quantiles > 1:
        if netspec.check_atoms(model_config.get("atoms", 1)) > 1:
            raise ValueError("quantiles = {} together with atoms = {}: a Q head is quantile (QR-DQN) or categorical (C51), "
                             "not both".format(quantiles, model_config["atoms"]))
        if bool(model_config.get("dueling", False)):
            raise NotImplementedError("dueling with quantiles = {}: the dueling stream is 1 wide, a quantile dueling "
                                      "network needs a quantiles-wide one; not provided (the folded form is the key "
                                      "dist_dueling)".format(quantiles))
        if not (np.isfinite(np.float32(kappa)) and np.float32(kappa) > 0):
            raise ValueError("quantiles = {}: kappa must be finite and > 0, got kappa = {} (the pure |u| loss, kappa = 0, "
                             "is not provided)".format(quantiles, kappa))
        if int(action_dim) > 64:
            raise ValueError("quantiles = {}: action_dim = {} exceeds 64 (the device step's limit)".format(quantiles, action_dim))
    return quantiles, kappa


NOISY_STREAM_ONLINE, NOISY_STREAM_TARGET, NOISY_STREAM_PREDICT = 0, 1, 2      # counter word c3 of a noise draw


def noisy_philox(counter, key):
    """Philox4x32-10 (the constants of ``xt_common.h``): counter = four uint32 words (scalars or equal-shaped arrays), key =
    two -> uint32 array [..., 4]"""
    mask, s32 = np.uint64(0xFFFFFFFF), np.uint64(32)
    c = [np.asarray(x, dtype=np.uint64) & mask for x in np.broadcast_arrays(*counter)]
    k0, k1 = np.uint64(int(key[0]) & 0xFFFFFFFF), np.uint64(int(key[1]) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]          # 32 x 32 -> 64 bit
        c = [(p1 >> s32) ^ c[1] ^ k0, p1 & mask, (p0 >> s32) ^ c[3] ^ k1, p0 & mask]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & mask, (k1 + np.uint64(0xBB67AE85)) & mask
    return np.stack(c, axis=-1).astype(np.uint32)


def noisy_uniforms(seed, call, stream, layer, side, length):
    """-> (u1, u2) float32 [length] of vector ``side`` (0: input side, 1: output side) of noisy layer ``layer``: element i
    takes words 2 (i & 1), 2 (i & 1) + 1 of block philox(i >> 1, 2 layer + side, (uint32) call, stream) keyed by the 64-bit
    ``seed``; u = ((float)(w >> 9) + 0.5) * 2^-23, exact in float32"""
    i = np.arange(int(length), dtype=np.uint64)
    seed = int(seed) & (2 ** 64 - 1)
    w = noisy_philox((i >> np.uint64(1), 2 * int(layer) + int(side), int(call) & 0xFFFFFFFF, int(stream)),
                     (seed & 0xFFFFFFFF, seed >> 32))
    odd = (i & np.uint64(1)).astype(bool)
    uni = lambda x: ((x >> np.uint32(9)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)
    return uni(np.where(odd, w[:, 2], w[:, 0])), uni(np.where(odd, w[:, 3], w[:, 1]))


def noisy_f(u1, u2):
    """f = sgn(x) sqrt|x| of the Box-Muller normal x = sqrtf(-2 logf(u1)) * cosf(6.283185307179586f * u2), all float32"""
    u1, u2 = np.asarray(u1, np.float32), np.asarray(u2, np.float32)
    x = np.sqrt(np.float32(-2.0) * np.log(u1)) * np.cos(np.float32(6.283185307179586) * u2)
    return np.copysign(np.sqrt(np.abs(x)), x).astype(np.float32)


def noisy_vectors(spec, seed, call, stream):
    """-> float32 [spec.noise_floats]: every f_in / f_out of a noisy spec's layers, laid out as the net's noise buffer"""
    noise = np.zeros(spec.noise_floats, np.float32)
    for nl in spec.noisy_layers:
        noise[nl.f_in] = noisy_f(*noisy_uniforms(seed, call, stream, nl.index, 0, nl.K))
        noise[nl.f_out] = noisy_f(*noisy_uniforms(seed, call, stream, nl.index, 1, nl.N))
    return noise


def noisy_effective(spec, store, noise):
    """-> float32 [spec.n_net]: store[0, n_net) with W_eff = mu + sigma * (f_in f_out^T) and b_eff = mu_b + sigma_b * f_out
    over the noisy layers' blocks (e rounded, the product rounded, then the sum)"""
    store = np.asarray(store, np.float32)
    eff = store[:spec.n_net].copy()
    for nl in spec.noisy_layers:
        kn = nl.K * nl.N
        f_in, f_out = noise[nl.f_in], noise[nl.f_out]
        e = (f_in[:, None] * f_out[None, :]).reshape(-1)
        prod = store[nl.sigma_off:nl.sigma_off + kn] * e
        eff[nl.w_off:nl.w_off + kn] = store[nl.w_off:nl.w_off + kn] + prod
        prod_b = store[nl.sigma_off + kn:nl.sigma_off + kn + nl.N] * f_out
        eff[nl.w_off + kn:nl.w_off + kn + nl.N] = store[nl.w_off + kn:nl.w_off + kn + nl.N] + prod_b
    return eff


def noisy_sigma_grads(spec, grads, noise):
    """-> a copy of the store-sized gradient ``grads`` whose sigma blocks are g_sigma = dW_eff * e and g_sigma_b = db_eff *
    f_out, from its own [0, n_net) (what the backward left)"""
    out = np.array(grads, np.float32)
    for nl in spec.noisy_layers:
        kn = nl.K * nl.N
        f_in, f_out = noise[nl.f_in], noise[nl.f_out]
        e = (f_in[:, None] * f_out[None, :]).reshape(-1)
        out[nl.sigma_off:nl.sigma_off + kn] = out[nl.w_off:nl.w_off + kn] * e
        out[nl.sigma_off + kn:nl.sigma_off + kn + nl.N] = out[nl.w_off + kn:nl.w_off + kn + nl.N] * f_out
    return out


def noisy_config(model_config):
    """-> (noisy, noisy_sigma0, NOISY_PREDICT_MEAN) of a DQN ``model_config`` after the checks of the noisy keys"""
    noisy, sigma0 = netspec.check_noisy(model_config.get("noisy", False), model_config.get("noisy_sigma0", 0.5))
    return noisy, sigma0, bool(model_config.get("NOISY_PREDICT_MEAN", False))


def dqn_spec(model_info):
    """The ``NetSpec`` of a DQN model description (``model_para.actor`` of a YAML): ``DqnCnn`` / ``DqnMlp``."""
    cfg = model_info.get("model_config") or {}
    name, dueling = model_info["model_name"], bool(cfg.get("dueling", False))
    if name == "DqnCnnPong":
        raise NotImplementedError(PONG_MESSAGE)
    noisy, sigma0, _ = noisy_config(cfg)
    atoms, quantiles = dist_config(cfg, model_info["action_dim"])[0], quant_config(cfg, model_info["action_dim"])[0]
    duel = dist_dueling_config(cfg, model_info["action_dim"])
    if name == "DqnCnn":
        return netspec.dqn_cnn(tuple(model_info["state_dim"]), model_info["action_dim"], dueling, atoms, quantiles, noisy,
                               sigma0, duel)
    if name == "DqnMlp":
        from xingtian_amd.model.dqn import default_config as d
        return netspec.dqn_mlp(tuple(model_info["state_dim"]), model_info["action_dim"],
                               cfg.get("HIDDEN_SIZE", d.HIDDEN_SIZE), cfg.get("NUM_LAYERS", d.NUM_LAYERS), dueling,
                               atoms, quantiles, noisy, sigma0, duel)
    raise KeyError("no DQN model named {}".format(name))


class DqnModel(XTModel):
    CLIPNORM = 0.0

    def __init__(self, model_info, learning_rate):
        model_config = model_info.get("model_config") or {}
        self.state_dim, self.action_dim = model_info["state_dim"], model_info["action_dim"]
        self.learning_rate = learning_rate
        self.dueling = bool(model_config.get("dueling", False))
        self.atoms, self.v_min, self.v_max = dist_config(model_config, self.action_dim)
        self.support = dist_support(self.atoms, self.v_min, self.v_max)[0] if self.atoms > 1 else None
        self.quantiles, self.kappa = quant_config(model_config, self.action_dim)
        self.dist_dueling = dist_dueling_config(model_config, self.action_dim)
        self.noisy, self.noisy_sigma0, self.noisy_predict_mean = noisy_config(model_config)
        self.noisy_predict_calls = 0              # the call word of the noise ``predict`` draws on a learner net
        self.seed = model_config.get("SEED")
        # the algorithm's minibatch (model_info["max_batch"], set by DQN) bounds the training step; predict walks larger
        # inputs in chunks
        self.max_batch = int(model_config.get("MAX_BATCH", model_info.get("max_batch", 256)))
        self.iterations = 0                       # optimizer.iterations of tf.keras Adam
        super().__init__(model_info)

    def _spec(self):
        raise NotImplementedError

    def create_model(self, model_info):
        self.net = build_net(model_info, self._spec(), self.max_batch, self.seed)
        if self.atoms > 1 and not getattr(self.net, "inference_only", False):
            self.net.set_dist(self.atoms, self.v_min, self.v_max)
        if self.quantiles > 1 and not getattr(self.net, "inference_only", False):
            self.net.set_quant(self.quantiles, self.kappa)
        if self.dist_dueling and not getattr(self.net, "inference_only", False):
            self.net.set_duel(True)
        if self.noisy:
            # the key of every noise draw: SEED, or one drawn here when the configuration gives none
            key = self.seed if self.seed is not None else int(np.random.default_rng().integers(0, 2 ** 63))
            if getattr(self.net, "inference_only", False):
                self.net.set_noisy(key, self.noisy_sigma0, mean_only=self.noisy_predict_mean)
            else:
                self.net.set_noisy(key, self.noisy_sigma0)
        self.actor_var = self.net
        return True

    def extra_optimizer_state(self):
        out = {"keras_adam_iterations": np.int64(self.iterations)}
        if self.noisy:
            out["noisy_predict_calls"] = np.int64(self.noisy_predict_calls)
        return out

    def restore_extra_optimizer_state(self, arrays):
        if "keras_adam_iterations" in arrays:
            self.iterations = int(arrays["keras_adam_iterations"])
        if self.noisy and "noisy_predict_calls" in arrays:
            self.noisy_predict_calls = int(arrays["noisy_predict_calls"])

    def predict(self, state):
        """-> Q [N, A] (numpy float32); with ``atoms`` > 1 the expectation under every action's softmax (``dist_q``), with
        ``quantiles`` > 1 the mean of every action's quantiles (``quant_q``), with ``dist_dueling`` of the combined logits /
        quantiles (``dist_dueling_combine``).  A noisy model draws new noise per call
        (stream 2; the CPU replica from a counter of its own inside ``forward``) unless ``NOISY_PREDICT_MEAN``."""
        if self.noisy and not getattr(self.net, "inference_only", False):
            self.net.compose(self.noisy_predict_calls, NOISY_STREAM_PREDICT, mean_only=self.noisy_predict_mean)
            self.noisy_predict_calls += 1
        logits, value = self.net.forward(np.asarray(state))
        if self.dist_dueling:                               # the folded head: combine first, [B, A, N]
            logits = dist_dueling_combine(as_numpy(logits), self.action_dim, max(self.atoms, self.quantiles))
        if self.atoms > 1:
            return dist_q(as_numpy(logits).reshape(-1, self.action_dim, self.atoms), self.support)
        if self.quantiles > 1:
            return quant_q(as_numpy(logits).reshape(-1, self.action_dim, self.quantiles))
        return dueling_q(as_numpy(logits), as_numpy(value), self.dueling)

    def train_replay(self, target, replay, slots, gamma, double_dqn):
        """One update on the minibatch ``slots`` (int32 device tensor) of the device rings ``replay``
        (``algorithm.dqn.DeviceReplay``): ``xt_net_dqn_step`` with ``target``'s network as the target net, then tf.keras
        Adam.  Nothing synchronises.  -> the device tensor [loss, mean |TD error|, mean bootstrap Q].  A replay with
        ``n_step`` > 1 trains on n-step targets (``xt_net_dqn_step_n``).  A distributional model (``atoms`` > 1) takes
        ``xt_net_dqn_step_dist`` either way, a quantile one (``quantiles`` > 1) ``xt_net_dqn_step_quant``; the tensor is
        then [loss, mean per-sample loss, mean bootstrap Q]."""
        return self._train_step(target, replay, slots, None, gamma, double_dqn)

    def train_replay_per(self, target, replay, u, beta, gamma, double_dqn):
        """``train_replay`` on a ``PrioritizedDeviceReplay``: the minibatch is drawn on the device with the uniform draws
        ``u`` (float64 device tensor [B]) and importance exponent ``beta``, and the replay's trees take the new TD errors
        (``xt_net_dqn_step_per``), then tf.keras Adam.  Nothing synchronises.  -> the device tensor of ``train_replay``."""
        per = dict(size=replay.size(), u=u, sum_tree=replay.sum_tree, min_tree=replay.min_tree, max_prio=replay.max_prio,
                   alpha=replay.alpha, beta=beta, eps=replay.eps)
        return self._train_step(target, replay, None, per, gamma, double_dqn)

    def _train_step(self, target, replay, slots, per, gamma, double_dqn):
        """``net.dqn_step`` with the keywords the replay store (n-step) and the model (distributional, quantile) ask for, then
        tf.keras Adam.  A noisy model composes both nets' effective weights in front of it (call = ``iterations``: the online
        net on stream 0, the target net on stream 1) and forms the sigma gradients behind it: three launches more."""
        self._require_learner()
        n = getattr(replay, "n_step", 1)
        if self.noisy:
            self.net.compose(self.iterations, NOISY_STREAM_ONLINE)
            target.net.compose(self.iterations, NOISY_STREAM_TARGET)
        out = self.net.dqn_step(target.net, replay.cur_state, replay.next_state, slots, replay.action, replay.reward,
                                replay.done, gamma, self.dueling, double_dqn, follow=replay.follow if n > 1 else None, n=n,
                                per=per, dist=self.atoms > 1, quant=self.quantiles > 1)
        if self.noisy:
            self.net.noisy_grads()
        self.net.adam_keras(self.learning_rate, self.iterations, clipnorm=self.CLIPNORM)
        self.iterations += 1
        return out

    def copy_weights_from(self, other):
        """this network's parameters <- ``other``'s: one device-to-device copy of the flat buffer on a learner"""
        if getattr(self.net, "inference_only", False) or getattr(other.net, "inference_only", False):
            self.set_weights(other.get_weights())
            return
        self.net.params.copy_(other.net.params)
        self.net.touch()


@Registers.model
class DqnCnn(DqnModel):
    CLIPNORM = 10.0

    def __init__(self, model_info):
        import_config(globals(), model_info.get("model_config") or {})
        super().__init__(model_info, LR)

    def _spec(self):
        return netspec.dqn_cnn(tuple(self.state_dim), self.action_dim, self.dueling, self.atoms, self.quantiles, self.noisy,
                               self.noisy_sigma0, self.dist_dueling)
