"""Host side of the noisy-layer tests (tests/test_cpu_noisy.py, tests/test_gpu_noisy.py): synthetic layer tables over a
store with plain ranges between the blocks, the float64 twin of the noise draw, callers of the two C entries that put
guard words round every buffer, and the float64 reference of a whole noisy ``dqn_step``.  The float32 definitions under
test are the package's own host twins (``xingtian_amd.model.dqn.dqn_cnn.noisy_*``).  Not a test module."""
import ctypes
from collections import OrderedDict
from types import SimpleNamespace

import numpy as np

import dqn_helpers as H
from xingtian_amd.model import netspec
from xingtian_amd.model.dqn import dqn_cnn as D

GUARD = 16                        # guard floats on either side of every device buffer (64 bytes: alignment is kept)
SENTINEL = np.float32(-7.5)
SEED, CALL = 0x123456789ABCDEF, 41

# (K, N) of the single-layer tables: the issue's five and one head wider than a tile of the compose pass (1024 floats)
SHAPES = [(4, 4), (12, 8), (260, 4), (8, 1), (8, 516), (4, 1100)]
# one table of three layers; the plain floats in front of each block (multiples of 4).  600 floats in front of the wide
# head put a tile boundary 424 floats into its block: a span shorter than a row
THREE = ([(12, 8), (8, 1), (8, 516)], [8, 12, 464])
TABLES = OrderedDict([("%dx%d" % s, ([s], [8])) for s in SHAPES] + [("three", THREE)])


def align4(x):
    return (x + 3) & ~3


def table(shapes, plain):
    """-> a namespace shaped like a noisy ``NetSpec`` (``noisy_layers``, ``n_net``, ``n_flat``, ``noise_floats``): the mean
    blocks in table order, ``plain[i]`` plain floats in front of block i and 20 behind the last, the sigma blocks behind
    n_net in REVERSE order with 4 unused floats between them"""
    off, layers = 0, []
    for index, ((k, n), gap) in enumerate(zip(shapes, plain)):
        nl = netspec.NoisyLayer()
        nl.name, nl.index, nl.K, nl.N, nl.w_off = "l%d" % index, index, k, n, off + gap
        off = align4(nl.w_off + (k + 1) * n)
        layers.append(nl)
    n_net = off + 20
    off, noise_off = n_net + 4, 0
    for nl in reversed(layers):
        nl.sigma_off = off
        off = align4(off + (nl.K + 1) * nl.N) + 4
    for nl in layers:
        nl.noise_off = noise_off
        noise_off += align4(nl.K) + align4(nl.N)
    return SimpleNamespace(noisy_layers=layers, n_net=n_net, n_flat=off, noise_floats=noise_off)


def store_of(t, seed):
    """a store of standard-normal floats (plain ranges and unused floats included)"""
    return np.random.default_rng(seed).standard_normal(t.n_flat).astype(np.float32)


def vector_slices(t):
    return [s for nl in t.noisy_layers for s in (nl.f_in, nl.f_out)]


def twin64(t, seed, call, stream):
    """-> float64 [noise_floats]: x = sqrt(-2 log u1) cos(2 pi u2) in float64 on the SAME float32 uniforms, laid out as the
    noise buffer (f |f| of a stored vector is compared with it)"""
    out = np.zeros(t.noise_floats, np.float64)
    for nl in t.noisy_layers:
        for side, sl, n in ((0, nl.f_in, nl.K), (1, nl.f_out, nl.N)):
            u1, u2 = (u.astype(np.float64) for u in D.noisy_uniforms(seed, call, stream, nl.index, side, n))
            out[sl] = np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)
    return out


def squared(f):
    """f |f| in float64"""
    f = np.asarray(f, np.float64)
    return f * np.abs(f)


_BAR = {}


def vector_bar():
    """-> (measured, bar): the largest |f |f| - twin| of the float32 NumPy restatement over every vector element of every
    table of the compose test, and four times that (the project's rule: the factor covers the device's libm)"""
    if not _BAR:
        worst = 0.0
        for shapes, plain in TABLES.values():
            t = table(shapes, plain)
            f32, x64 = D.noisy_vectors(t, SEED, CALL, 0), twin64(t, SEED, CALL, 0)
            for sl in vector_slices(t):
                worst = max(worst, float(np.abs(squared(f32[sl]) - x64[sl]).max()))
        _BAR["measured"], _BAR["bar"] = worst, 4.0 * worst
    return _BAR["measured"], _BAR["bar"]


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


# ----------------------------------------------------------------------------------------------- C entries (GPU)
def c_table(layers):
    from xingtian_amd import lib as L
    return (L.NoisyLayer * max(len(layers), 1))(*[
        L.NoisyLayer(nl.w_off, nl.sigma_off, nl.noise_off, nl.K, nl.N, nl.index, 0) for nl in layers])


class Guarded(object):
    """a float32 device buffer with ``GUARD`` sentinel floats on either side of its body"""

    def __init__(self, body):
        import torch
        host = np.concatenate([np.full(GUARD, SENTINEL), np.asarray(body, np.float32), np.full(GUARD, SENTINEL)])
        self.dev = torch.from_numpy(host).cuda()
        self.n = len(body)

    @property
    def ptr(self):
        return ctypes.c_void_p(self.dev.data_ptr() + 4 * GUARD)

    def read(self):
        """-> the body; asserts the guards"""
        host = self.dev.cpu().numpy()
        assert (host[:GUARD] == SENTINEL).all() and (host[GUARD + self.n:] == SENTINEL).all(), "guard words overwritten"
        return host[GUARD:GUARD + self.n].copy()


def gpu_compose(t, store, seed=SEED, call=CALL, stream=0, mean_only=False, noise_in=None, layers=None, n_layers=None,
                n_net=None, null=()):
    """-> (rc, eff, noise, store afterwards): xt_noisy_compose on guarded buffers; ``eff`` and ``noise`` start as sentinels.
    ``layers``: another table than ``t.noisy_layers``; ``null``: names of pointers passed as NULL."""
    import torch
    from xingtian_amd import lib as L
    layers = t.noisy_layers if layers is None else layers
    d_store, d_eff = Guarded(store), Guarded(np.full(t.n_net, SENTINEL))
    d_noise = Guarded(np.full(t.noise_floats, SENTINEL))
    d_in = None if noise_in is None else Guarded(noise_in)
    p = dict(layers=c_table(layers), store=d_store.ptr, eff=d_eff.ptr, noise=d_noise.ptr)
    for k in null:
        p[k] = None
    rc = L.load().xt_noisy_compose(p["layers"], len(layers) if n_layers is None else n_layers, p["store"], p["eff"],
                                   t.n_net if n_net is None else n_net, p["noise"], None if d_in is None else d_in.ptr,
                                   seed, call, stream, 1 if mean_only else 0, L.stream_ptr())
    torch.cuda.synchronize()
    return rc, d_eff.read(), d_noise.read(), d_store.read()


def gpu_grads(t, grads, noise, layers=None, n_layers=None, null=()):
    """-> (rc, grads afterwards): xt_noisy_grads on guarded buffers"""
    import torch
    from xingtian_amd import lib as L
    layers = t.noisy_layers if layers is None else layers
    d_grads, d_noise = Guarded(grads), Guarded(noise)
    p = dict(layers=c_table(layers), noise=d_noise.ptr, grads=d_grads.ptr)
    for k in null:
        p[k] = None
    rc = L.load().xt_noisy_grads(p["layers"], len(layers) if n_layers is None else n_layers, p["noise"], p["grads"],
                                 L.stream_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(bits(d_noise.read()), bits(noise))
    return rc, d_grads.read()


def last_error():
    from xingtian_amd import lib as L
    return L.load().xt_last_error().decode()


# ----------------------------------------------------------------------------------------------- the whole step
def effective64(spec, store, noise):
    """float64 [n_net]: W_eff = mu + sigma * (f_in f_out^T), b_eff = mu_b + sigma_b * f_out formed in float64 from the
    float32 store and the float32 vectors the kernel stored"""
    s, z = np.asarray(store, np.float64), np.asarray(noise, np.float64)
    eff = s[:spec.n_net].copy()
    for nl in spec.noisy_layers:
        kn = nl.K * nl.N
        e = np.concatenate([np.outer(z[nl.f_in], z[nl.f_out]).reshape(-1), z[nl.f_out]])
        eff[nl.w_off:nl.w_off + kn + nl.N] += s[nl.sigma_off:nl.sigma_off + kn + nl.N] * e
    return eff


def name_map(spec, ospec):
    """``dqn_helpers.name_map`` for a noisy spec: mean name -> oracle name (the sigma names stand behind every mean name)"""
    return OrderedDict((h, o) for h, o in zip(spec.names, H.nets.init_params(ospec)) if "/sigma_" not in h)


def oracle_params(spec, ospec, eff64):
    """the oracle's parameter dict (float64) read out of a flat effective-parameter array; a hidden 1-wide head is zero"""
    p = OrderedDict((o, np.zeros_like(np.asarray(v, np.float64))) for o, v in H.nets.init_params(ospec).items())
    for h, o in name_map(spec, ospec).items():
        p[o] = np.asarray(spec.var_view(eff64, h), np.float64).reshape(p[o].shape).copy()
    return p


def sigma_grads64(spec, ospec, ref_grads, noise):
    """-> {sigma name: float64 tensor in TF shape}: g_sigma = dW_eff * e, g_sigma_b = db_eff * f_out from the oracle's
    gradients of the effective parameters and the stored vectors"""
    z, names, out = np.asarray(noise, np.float64), name_map(spec, ospec), {}
    for nl in spec.noisy_layers:
        rows = spec.names[nl.name + "/kernel"][1][0]              # (TF rows: a padded block's extra rows carry no gradient)
        dw = np.asarray(ref_grads[names[nl.name + "/kernel"]], np.float64).reshape(rows, nl.N)
        db = np.asarray(ref_grads[names[nl.name + "/bias"]], np.float64).reshape(nl.N)
        out[nl.name + "/sigma_kernel"] = dw * np.outer(z[nl.f_in][:rows], z[nl.f_out])
        out[nl.name + "/sigma_bias"] = db * z[nl.f_out]
    return out


def kink_margins(ospec, params, rows):
    """per row: the smallest |pre-activation| of any ReLU unit in the float64 forward (a unit closer to zero than float32's
    accumulation error may come out on the other side of the kink in any float32 implementation)"""
    net = H.nets.ActorCritic(ospec, params, np.float64)
    net.forward(rows)
    return np.min([np.abs(z.reshape(len(rows), -1)).min(1) for _, _, z in net.cache[0]], axis=0)


def pick_gaps(q):
    """per row: the gap between the two best picking values over max(1, the row's largest magnitude)"""
    s = np.sort(np.asarray(q, np.float64), axis=1)
    return (s[:, -1] - s[:, -2]) / np.maximum(1.0, np.abs(s).max(axis=1))


MARGIN, GAP = 1e-6, 1e-4          # what a minibatch row keeps from a ReLU kink / between its two best bootstrap values


# ---- the cases of the whole-step test: (kind, dueling, double_dqn, variant)
CAP, RING_SEED, GAMMA = 50, 11, 0.99
STEP_SEED, STEP_CALL = 77, 3                                  # key and call word of the step tests' noise
V_MIN, V_MAX, KAPPA = -10.0, 10.0, 1.0
SHAPE = {"mlp3": ((3,), 2, 5), "mlp4": ((4,), 2, 5), "cnn": ((84, 84, 4), 4, 3)}      # state_dim, A, B
STEP_CASES = ([(k, du, do, "plain") for k in SHAPE for du in (False, True) for do in (False, True)] +
              [("mlp4", False, False, v) for v in ("per", "nstep", "atoms", "quantiles")])
HEAD = {"atoms": (5, 1), "quantiles": (1, 4)}                 # variant -> (atoms, quantiles)


def step_specs(kind, dueling, variant):
    sd, a, _ = SHAPE[kind]
    atoms, quantiles = HEAD.get(variant, (1, 1))
    if kind == "cnn":
        return (netspec.dqn_cnn(sd, a, dueling, atoms, quantiles, noisy=True), H.oracle_spec("cnn", sd, a * atoms * quantiles))
    return (netspec.dqn_mlp(sd, a, 8, 1, dueling, atoms, quantiles, noisy=True),
            H.oracle_spec("mlp", sd, a * atoms * quantiles, 8, 1))


def state_fn(kind):
    sd = SHAPE[kind][0]
    if kind == "cnn":
        return lambda tags, nxt: np.random.default_rng(int(tags[0]) * 2 + nxt).integers(0, 256, (len(tags),) + sd, dtype=np.uint8)
    return lambda tags, nxt: np.random.default_rng(int(tags[0]) * 2 + nxt).standard_normal((len(tags),) + sd).astype(np.float32)


_RINGS = {}


def ring_rows(kind):
    """-> (msgs, store, cur rows [CAP, ...], next rows [CAP, ...]) of the 50-row ring every whole-step case fills"""
    import nstep_helpers as N
    if kind not in _RINGS:
        msgs, store = N.make_messages(CAP, RING_SEED, a_dim=SHAPE[kind][1], states=state_fn(kind)), N.BruteStore(CAP)
        for m in msgs:
            store.add(m)
        cur = np.stack([msgs[m]["cur_state"][t] for m, t in store.slot])
        nxt = np.stack([msgs[m]["next_state"][t] for m, t in store.slot])
        _RINGS[kind] = (msgs, store, cur, nxt)
    return _RINGS[kind]


def host_labels(kind, n_step):
    """-> slots -> (boot, action, reward, disc, done): ``nstep_targets`` on the label rings the store implies"""
    from xingtian_amd.algorithm.dqn.dqn import nstep_targets
    msgs, store, _, _ = ring_rows(kind)
    col = lambda k, dt: np.asarray([msgs[m][k][t] for m, t in store.slot], dt)
    follow, action, reward, done = store.follow(), col("action", np.int32), col("reward", np.float64), col("done", np.uint8)
    return lambda s: nstep_targets(s, follow, action, reward, done, GAMMA, n_step, CAP)


def step_weights(spec, ospec, seed, dueling):
    """Keras name -> array: the means from the oracle's seeded parameters, every sigma drawn from U(0.05, 0.3)"""
    p = H.seeded_params(ospec, seed, dueling)
    w = OrderedDict((h, np.asarray(p[o], np.float32).reshape(spec.names[h][1])) for h, o in name_map(spec, ospec).items())
    rng = np.random.default_rng(100 + seed)
    for h, (_, shape) in spec.names.items():
        if "/sigma_" in h:
            w[h] = rng.uniform(0.05, 0.3, shape).astype(np.float32)
    return w


def store_of_weights(spec, w):
    flat = np.zeros(spec.n_flat, np.float32)
    for h, v in w.items():
        spec.var_view(flat, h)[...] = v
    return flat


def pick_q(variant, logits, value, dueling, a):
    """the values the bootstrap action is picked by, float64 [rows, A]"""
    lg = np.asarray(logits, np.float64)
    if variant == "atoms":
        z = np.linspace(V_MIN, V_MAX, HEAD["atoms"][0])
        e = np.exp(lg.reshape(len(lg), a, -1) - lg.reshape(len(lg), a, -1).max(-1, keepdims=True))
        return (e * z).sum(-1) / e.sum(-1)
    if variant == "quantiles":
        return lg.reshape(len(lg), a, -1).mean(-1)
    return H.q_from_heads(lg, np.asarray(value, np.float64).reshape(-1), dueling)


def eligible(kind, dueling, double, variant, ospec, p_on, p_tg):
    """-> the slots whose state row keeps MARGIN from every ReLU kink of the online net and whose bootstrap row keeps GAP
    between the two best values of the picking net, on the float64 oracle with the given (effective) parameters"""
    _, _, cur, nxt = ring_rows(kind)
    boot = host_labels(kind, 3 if variant == "nstep" else 1)(np.arange(CAP))[0]
    margins = kink_margins(ospec, p_on, cur)
    lg, v = H.nets.ActorCritic(ospec, p_on if double else p_tg, np.float64).forward(nxt)
    gaps = pick_gaps(pick_q(variant, lg, v, dueling, SHAPE[kind][1]))
    return np.flatnonzero((margins >= MARGIN) & (gaps[boot] >= GAP)).astype(np.int32)


def step_ref(kind, dueling, double, variant, ospec, p_on, p_tg, states, nstates, act, rew, disc, done, w):
    """the float64 oracle's step on a minibatch -> dict with ``loss`` and ``grads`` (of the effective parameters)"""
    a = SHAPE[kind][1]
    if variant == "atoms":
        import dist_helpers as DH
        return DH.DistOracle(ospec, p_on, p_tg, a, HEAD["atoms"][0], V_MIN, V_MAX, double, 3e-4).step(
            states, nstates, act, rew, disc, done, w)
    if variant == "quantiles":
        import quant_helpers as QH
        return QH.QuantOracle(ospec, p_on, p_tg, a, HEAD["quantiles"][1], KAPPA, double, 3e-4).step(
            states, nstates, act, rew, disc, done, w)
    return H.DqnOracle(ospec, p_on, p_tg, dueling, double, GAMMA, 3e-4).step(
        states, nstates, act, rew, done, weights=w, disc=disc if variant == "nstep" else None, apply=False)


def assert_step(got_loss, grads, ref, spec, ospec, noise, what=""):
    """the project's standing bars: loss 1e-4, every gradient tensor 1e-5 by ``rel_max`` -- mu against the oracle's gradient
    of the effective parameters, sigma against dW_eff * e formed in float64"""
    want = OrderedDict((h, ref["grads"][o]) for h, o in name_map(spec, ospec).items())
    want.update(sigma_grads64(spec, ospec, ref["grads"], noise))
    assert set(want) == set(spec.names)
    errs = {h: H.rel_max(grads[h], r) for h, r in want.items()}
    print("noisy step", what, "loss", got_loss, float(ref["loss"]), "| gradient tensors", errs)
    assert abs(got_loss - ref["loss"]) <= 1e-4 * max(1.0, abs(ref["loss"])), (got_loss, ref["loss"])
    for h, err in errs.items():
        assert err <= 1e-5, (h, err)
        assert np.abs(want[h]).max() > 0, h                   # (a reference of zeros would compare nothing)
