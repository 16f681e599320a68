"""GPU parity tests (run with -m gpu on an MI355X) of csrc/xt_optim.hip, the launches every training step ends in, each called
on its own through the stand-alone entries of include/xt_mi355x.h: grads_finish_kernel<STATS> in its four launch forms
(xt_grads_finish_ex, plan by xt_grads_finish_plan_ex), adam_tf_clip_kernel / rmsprop_tf_clip_kernel (xt_optim_clip_ex),
norm_finalize_kernel (xt_norm_finalize_ex), the three-launch xt_adam_tf_clip and xt_adam_keras.  Every row of the case tables
carries the plan it must get (z lanes, blocks, partial slots, grid), asserted against what the library reports.

References.  The reduced gradient is compared bit for bit with a float32 numpy twin that adds in the kernel's order (lane z0
of the entry's zl lanes adds slabs z0, z0 + zl, ..., then the lanes are added in order; the library is built with
-ffp-contract=off) and, in the relative 2-norm, with the float64 sum.  Everything else is compared with float64 formulas that
take every scalar as the float32 value the kernel receives, widened, and keep the beta powers as the float32 product chain
the kernel keeps (state[0] / state[1] are compared bit for bit with that chain).  A float32 build of the same formulas gives
the "f32 oracle" figure printed beside every measured one.

Bars: 2e-6 (relative 2-norm) for element-wise outputs, the reduced gradient and a squared-norm partial slot (at most twelve
roundings of 2^-24 lie between a slot and its float64 value: the square, three adds, the eight levels of the block's tree);
1e-5 for norm, clip factor and step size; 2e-5 for loss scalars.

The tables, data and references are plain numpy: tests/test_cpu_optim_coverage.py imports this module on the CPU, checks what
the tables cover and that every comparison used here rejects a deliberately wrong twin."""
import collections
import ctypes
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BAR_ELEM, BAR_NORM, BAR_LOSS = 2e-6, 1e-5, 2e-5
CANARY = -7777.25            # gaps of dst / params / m / v, unused partial slots
PART_TAIL = 16               # canary slots behind the table's partials
GAP = 8                      # canary floats between two entries of the flat buffers
B1, B2, ADAM_EPS = 0.9, 0.999, 1e-7
LR = 0.05
RMS_DECAY, RMS_EPS = 0.99, 0.1
OPT_ADAM, OPT_RMSPROP = 0, 1
f32 = np.float32


def cdiv(a, b):
    return -(-a // b)


def align4(n):
    return (n + 3) & ~3


def case_rng(cid, salt=0):
    return np.random.default_rng(zlib.crc32(cid.encode()) + salt)


def param_like(rng, n):
    """parameters of scale 0.1 with a bounded exponent range, +-[0.05, 0.15): half an ulp of a parameter, which every
    p_new - p_old carries, is then at most 7.5e-9 -- 1.5e-7 of an update of the size of lr = 0.05"""
    return (rng.choice([-1.0, 1.0], n) * (0.05 + 0.1 * rng.random(n))).astype(np.float32)


def grad_like(rng, sign, scale=1.0):
    """a gradient of magnitude [0.5, 1.5) * scale whose signs stay those of `sign` from step to step: the moments never
    cancel, so no update is small against its parameter's rounding"""
    return (sign * (0.5 + rng.random(len(sign))) * scale).astype(np.float32)


# ---------------------------------------------------------------- comparisons (every assertion below goes through these)
def bits_differ(a, b):
    """elements of two float32 arrays whose bit patterns differ (bar: 0)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape, (a.shape, b.shape)
    return int((a.view(np.uint32) != b.view(np.uint32)).sum())


def rel2(got, ref):
    """relative error in the 2-norm against a float64 reference (absolute where the reference is all zero)"""
    got, ref = np.asarray(got, np.float64).ravel(), np.asarray(ref, np.float64).ravel()
    n = np.linalg.norm(ref)
    return float(np.linalg.norm(got - ref) / n) if n > 0 else float(np.linalg.norm(got - ref))


def rel1(got, ref):
    """relative error of a scalar (absolute where the reference is zero)"""
    got, ref = float(got), float(ref)
    return abs(got - ref) / abs(ref) if ref != 0 else abs(got - ref)


def slots_err(got, ref):
    """largest relative error of a squared-norm partial slot"""
    return max([rel1(g, r) for g, r in zip(np.asarray(got).ravel(), np.asarray(ref).ravel())] + [0.0])


def within(err, bar):
    """(a NaN is outside every bar)"""
    return bool(err <= bar)


# ---------------------------------------------------------------- gradient reduction: cases
Ent = collections.namedtuple("Ent", "count nslab zl nblk pad inplace pre")
RedCase = collections.namedtuple("RedCase", "id ents early knobs pblk0 npart grid")


def ent(count, nslab, zl, nblk, pad=4, inplace=False, pre=0):
    """count elements summed over nslab slabs of stride align4(count) + pad; zl / nblk: the expected z lanes and blocks;
    inplace: src == dst (one slab, nothing written); pre: squared-norm slots the producer has filled already"""
    assert not inplace or nslab == 1
    return Ent(count, nslab, zl, nblk, 0 if inplace else pad, inplace, pre)


def red(id, ents, early=0, knobs=None, pblk0=None, npart=None, grid=None):
    """pblk0 / npart / grid: the expected first slot of every entry, slots of the table, blocks of a form-0 launch (the
    defaults are those of a single-entry table)"""
    ents = tuple(ents)
    if len(ents) == 1 and pblk0 is None:
        pblk0, npart, grid = (0,), ents[0].pre or ents[0].nblk, ents[0].nblk
    return RedCase(id, ents, early, knobs or {}, tuple(pblk0), npart, grid)


# cols = 256 / zl float4 columns per block: 4 * cols elements (zl 1: 1024, 2: 512, 4: 256, 8: 128, 16: 64, 32: 32)
T12 = (ent(4099, 64, 8, 33), ent(1024, 1, 1, 1, inplace=True), ent(1025, 1, 1, 2, pad=0), ent(513, 2, 2, 2),
       ent(257, 4, 4, 2, pad=12), ent(33, 128, 32, 2), ent(7, 9, 8, 1), ent(2565, 3, 4, 11, pad=0), ent(513, 40, 8, 5),
       ent(6, 300, 32, 1, pad=0), ent(9000, 5, 8, 71), ent(1, 1, 1, 1))
TPRE = (ent(300, 5, 8, 3), ent(1000, 1, 1, 1, inplace=True, pre=3), ent(37, 2, 2, 1))
RED_CASES = [
    # ---- one slab
    red("r_s1_inplace_c1024", [ent(1024, 1, 1, 1, inplace=True)]),
    red("r_s1_inplace_c5", [ent(5, 1, 1, 1, inplace=True)]),
    red("r_s1_copy_c1025", [ent(1025, 1, 1, 2)]),
    # ---- zl 2 / 4, block boundary 4 * cols | 4 * cols + 1
    red("r_s2_c512", [ent(512, 2, 2, 1)]),
    red("r_s2_c513", [ent(513, 2, 2, 2, pad=0)]),
    red("r_s3_c1", [ent(1, 3, 4, 1)]),
    red("r_s4_c256", [ent(256, 4, 4, 1, pad=12)]),
    red("r_s4_c257", [ent(257, 4, 4, 2)]),
    # ---- zl 8: one round of the 8-deep batch up to 64 slabs, two from 65
    red("r_s5_c2", [ent(2, 5, 8, 1, pad=0)]),
    red("r_s8_c3", [ent(3, 8, 8, 1)]),
    red("r_s9_c4", [ent(4, 9, 8, 1)]),
    red("r_s63_c5", [ent(5, 63, 8, 1)]),
    red("r_s64_c7", [ent(7, 64, 8, 1, pad=0)]),
    red("r_s64_c4099", [ent(4099, 64, 8, 33)]),
    red("r_s65_c128", [ent(128, 65, 8, 1)]),
    red("r_s65_c129", [ent(129, 65, 8, 2, pad=12)]),
    red("r_s127_c6", [ent(6, 127, 8, 1)]),
    # ---- the deep rule (reduce_deep_lanes = 128): zl 32
    red("r_s128_c32", [ent(32, 128, 32, 1)]),
    red("r_s128_c33", [ent(33, 128, 32, 2)]),
    red("r_s250_c2400", [ent(2400, 250, 32, 75, pad=0)]),
    red("r_s256_c9", [ent(9, 256, 32, 1)]),
    red("r_s257_c10", [ent(10, 257, 32, 1, pad=0)]),
    # ---- zl 16 through the knob
    red("r_z16_s16_c64", [ent(64, 16, 16, 1)], knobs=dict(reduce_z_lanes=16)),
    red("r_z16_s20_c65", [ent(65, 20, 16, 2)], knobs=dict(reduce_z_lanes=16)),
    red("r_z16_s127_c5", [ent(5, 127, 16, 1, pad=0)], knobs=dict(reduce_z_lanes=16)),
    # ---- grids of 63 / 64 / 65 blocks (the ticket's nsub / cnt arithmetic; one more with the extra block)
    red("r_g63", [ent(8064, 5, 8, 63, pad=0)]),
    red("r_g64", [ent(8192, 5, 8, 64)]),
    red("r_g65", [ent(8193, 5, 8, 65)]),
    # ---- tables: twelve entries (the heads' entries own the first slots, as in a net), a pre-reduced entry
    red("r_t12", T12, early=0b001110000000, pblk0=(17, 50, 51, 53, 55, 57, 59, 0, 11, 16, 60, 131), npart=132, grid=132),
    red("r_t12_plain", T12, pblk0=(0, 33, 34, 36, 38, 40, 42, 43, 54, 59, 60, 131), npart=132, grid=132),
    red("r_tpre", TPRE, early=0b110, pblk0=(4, 0, 3), npart=7, grid=4),
]
RED_BY_ID = {c.id: c for c in RED_CASES}


def red_data(c):
    """inputs of a reduction case from its id alone: per entry the slabs [nslab, stride] (padding lanes NaN; None for an
    in-place entry), the offset of its dst in the flat gradient buffer, and that buffer (canaries between the entries and
    in the last float4's padding lanes; an in-place entry's gradient in place)"""
    rng = case_rng(c.id)
    offs, srcs, total = [], [], GAP
    for e in c.ents:
        offs.append(total)
        total += align4(e.count) + GAP
    flat = np.full(total, CANARY, np.float32)
    pre = {}
    for i, e in enumerate(c.ents):
        vals = rng.standard_normal((e.nslab, e.count)).astype(np.float32)
        if e.inplace:
            flat[offs[i]:offs[i] + e.count] = vals[0]
            srcs.append(None)
        else:
            s = np.full((e.nslab, align4(e.count) + e.pad), np.nan, np.float32)
            s[:, :e.count] = vals
            srcs.append(s)
        if e.pre:      # what a producer with `pre` blocks leaves: the sums of squares of its contiguous shares
            cuts = np.linspace(0, e.count, e.pre + 1).astype(int)
            pre[i] = np.array([(vals[0, a:b].astype(np.float64) ** 2).sum() for a, b in zip(cuts[:-1], cuts[1:])], np.float32)
    return dict(offs=offs, srcs=srcs, flat=flat, pre=pre, total=total)


def reduce_twin(slabs, count, zl, bug=None):
    """float32 sum of slabs [nslab, >= count] in the kernel's order.  bug: a deliberately wrong twin (test_cpu_optim_coverage)"""
    nslab = slabs.shape[0] - (1 if bug == "last_slab" else 0)
    lanes = np.zeros((zl, count), np.float32)
    for z in range(nslab):
        lanes[z % zl] += slabs[z, :count]
    r = lanes[0].copy()
    for z in range(1, zl):
        r += lanes[z]
    if bug == "float4_lane":
        r[count - 1] = 0
    if bug == "tail" and count & 3:
        r[count & ~3:] = 0
    return r


def red_reference(c, d, bug=None):
    """per entry the float32 twin and the float64 sum of dst, and the float64 squared-norm partial of every slot"""
    twin, ref64, partial = [], [], np.zeros(c.npart)
    for i, e in enumerate(c.ents):
        off = d["offs"][i]
        slabs = d["flat"][None, off:off + e.count] if e.inplace else d["srcs"][i]
        t = reduce_twin(slabs, e.count, e.zl, None if e.inplace else bug)
        twin.append(t)
        ref64.append(slabs[:, :e.count].astype(np.float64).sum(axis=0))
        if e.pre:
            partial[c.pblk0[i]:c.pblk0[i] + e.pre] = d["pre"][i]
        else:
            per = 4 * (256 // e.zl)
            for j in range(e.nblk):
                partial[c.pblk0[i] + j] = (t[j * per:(j + 1) * per].astype(np.float64) ** 2).sum()
    return dict(twin=twin, ref64=ref64, partial=partial)


def flat_expected(c, d, twin):
    """the flat gradient buffer after the launch: the twins in place, every canary where it was"""
    out = d["flat"].copy()
    for i, e in enumerate(c.ents):
        if not e.inplace:
            out[d["offs"][i]:d["offs"][i] + e.count] = twin[i]
    return out


# ---------------------------------------------------------------- float64 / float32 builds of the tail's formulas
def clip_ref(partials, clip, gs, T=np.float64, bug=None):
    """(gnorm, clip factor) of clip_scale on the double sum of the float32 partials"""
    p = np.asarray(partials, np.float32).astype(np.float64)
    if bug == "last_partial":
        p = p[:-1]
    clip, gs = T(f32(clip)), T(f32(gs))
    with np.errstate(divide="ignore"):
        gnorm = np.sqrt(T(p.sum())) * gs
        scale = clip * min(T(1) / gnorm, T(1) / clip) * (T(1) if bug == "grad_scale" else gs)
    return gnorm, scale


def advance_ref(state, lr, T=np.float64, bug=None):
    """adam_advance on a float32 state: (b1^t, b2^t) as the float32 product chain, the step size from them in T, the count"""
    b1p, b2p = f32(state[0]) * f32(B1), f32(state[1]) * f32(B2)
    if bug == "beta_power":
        b1p, b2p = f32(state[0]), f32(state[1])
    with np.errstate(divide="ignore", invalid="ignore"):
        alpha = T(f32(lr)) * np.sqrt(T(1) - T(b2p)) / (T(1) - T(b1p))
    return b1p, b2p, alpha, f32(state[5]) + f32(1)


def adam_ref(p, g, m, v, scale, alpha, T=np.float64):
    """-> m, v, p_new - p_old of one Adam step on float32 inputs, arithmetic in T"""
    p, g, m, v = (np.asarray(x, np.float32).astype(T) for x in (p, g, m, v))
    scale, alpha, eps = T(scale), T(alpha), T(f32(ADAM_EPS))
    omb1, omb2 = T(f32(1) - f32(B1)), T(f32(1) - f32(B2))
    gg = g * scale
    m = m + (gg - m) * omb1
    v = v + (gg * gg - v) * omb2
    return m, v, (p - (m * alpha) / (np.sqrt(v) + eps)) - p


def rmsprop_ref(p, g, mg, ms, scale, lr, T=np.float64):
    """-> mg, ms, p_new - p_old of one centred RMSProp step"""
    p, g, mg, ms = (np.asarray(x, np.float32).astype(T) for x in (p, g, mg, ms))
    scale, lr, eps, omd = T(scale), T(f32(lr)), T(f32(RMS_EPS)), T(f32(1) - f32(RMS_DECAY))
    gg = g * scale
    ms = ms + (gg * gg - ms) * omd
    mg = mg + (gg - mg) * omd
    return mg, ms, (p - lr * gg / np.sqrt(ms - mg * mg + eps)) - p


def keras_ref(p, g, m, v, segs, clipnorm, lr_t, T=np.float64, bug=None):
    """tf.keras Adam with per-tensor clipnorm over the segments (off, size); elements outside them are not touched"""
    p, g, m, v = (np.asarray(x, np.float32).astype(T) for x in (p, g, m, v))
    m, v, upd = m.copy(), v.copy(), np.zeros_like(p)
    clipnorm, lr_t, eps = T(f32(clipnorm)), T(f32(lr_t)), T(f32(ADAM_EPS))
    omb1, omb2 = T(f32(1) - f32(B1)), T(f32(1) - f32(B2))
    norms = [np.sqrt((g[o:o + n].astype(np.float64) ** 2).sum()) for o, n in segs]
    for k, (o, n) in enumerate(segs):
        norm = T(norms[(k + 1) % len(segs)] if bug == "neighbour_norm" and k == len(segs) - 2 else norms[k])
        scale = clipnorm / norm if clipnorm > 0 and norm > clipnorm else T(1)
        s = slice(o, o + n)
        gg = g[s] * scale
        m[s] = m[s] + (gg - m[s]) * omb1
        v[s] = v[s] + (gg * gg - v[s]) * omb2
        upd[s] = (p[s] - lr_t * m[s] / (np.sqrt(v[s]) + eps)) - p[s]
    return m, v, upd


def ppo_loss_ref(terms, ent_coef, critic_coef, inv_b, T=np.float64):
    """loss_reduce_body's PPO scalars: (loss, actor, vf, ent), and surr"""
    tot = np.asarray(terms, np.float32).astype(np.float64)[:, :3].sum(axis=0)
    inv_b, ent_coef, critic_coef = T(f32(inv_b)), T(f32(ent_coef)), T(f32(critic_coef))
    surr, ent, vf = T(tot[0]) * inv_b, T(tot[1]) * inv_b, T(0.5) * T(tot[2]) * inv_b
    actor = -surr - ent_coef * ent
    return np.array([actor + critic_coef * vf, actor, vf, ent]), surr


def ppo_rows_ref(rows):
    """the seven row sums XT_TRAIN_STATS_KL .. ERR_SQ"""
    r = np.asarray(rows, np.float32).astype(np.float64)
    fl = r[:, 1].astype(np.int64)
    return np.array([r[:, 0].sum(), (fl & 1).sum(), ((fl >> 1) & 1).sum(), r[:, 2].sum(), (r[:, 2] ** 2).sum(), r[:, 3].sum(),
                     (r[:, 3] ** 2).sum()])


def gnorm_stats_ref(stats, gnorm, clip):
    """stats_add_gnorm on slots 12 / 13 / 14"""
    out = np.array(stats, np.float64)
    out[12] += float(gnorm)
    out[13] = max(out[13], float(gnorm))
    out[14] += 1.0 if float(gnorm) > float(f32(clip)) else 0.0
    return out


# ---------------------------------------------------------------- launch forms: cases
FormCase = collections.namedtuple("FormCase", "id table loss n acc_set stats lr_dev side gs")
PPO_ENT, PPO_CRITIC = 0.003, 0.7


def form(id, table, loss, n, acc_set=0, stats=False, lr_dev=False, side="above", gs=1.0):
    """table: a RED_CASES id (early = 0 tables only: form 1 stores block b's partial in slot b); loss: "ppo" with B = n or
    "impala" with n_traj = n; side: the gradient norm lies "above" (clipped) or "below" the clip norm, ratio 2"""
    assert RED_BY_ID[table].early == 0 or any(e.pre for e in RED_BY_ID[table].ents)
    return FormCase(id, table, loss, n, acc_set, stats, lr_dev, side, gs)


FORM_CASES = [
    form("f_g1_ppo_b1", "r_s2_c512", "ppo", 1, side="below"),
    form("f_g1_impala_n1_stats", "r_s9_c4", "impala", 1, acc_set=1, stats=True, lr_dev=True),
    form("f_g63_ppo_b255_stats", "r_g63", "ppo", 255, stats=True),
    form("f_g64_ppo_b256_lrdev", "r_g64", "ppo", 256, lr_dev=True, side="below", gs=0.5),
    form("f_g65_ppo_b257_stats", "r_g65", "ppo", 257, stats=True, side="below", gs=1.0 / 3.0),
    form("f_t12_ppo_b300_stats", "r_t12_plain", "ppo", 300, stats=True, lr_dev=True),
    form("f_t12_impala_n3", "r_t12_plain", "impala", 3, acc_set=0, side="below"),
    form("f_z32_impala_n3_stats", "r_s250_c2400", "impala", 3, acc_set=1, stats=True, gs=0.5),
    form("f_tpre_ppo_b300", "r_tpre", "ppo", 300),
]
ACC0 = (0.25, 3.0)
IMPALA_TRAJ_FLOATS = 12


def form_data(c):
    """the loss block's inputs and the starting values of every buffer the forms write"""
    rng = case_rng(c.id, 1)
    d = dict(stats0=0.5 * np.arange(16, dtype=np.float64), state0=np.array([1, 1, 0, 0, 0, 0, 0, 0], np.float32))
    if c.loss == "ppo":
        t = np.zeros((c.n, 4), np.float32)       # surr around -0.5, entropy around 1, vf around 0.8: no cancellation in the loss
        t[:, 0] = -0.5 + 0.2 * rng.standard_normal(c.n)
        t[:, 1] = 1.0 + 0.1 * rng.standard_normal(c.n)
        t[:, 2] = 0.8 + 0.3 * rng.random(c.n)
        t[:, 3] = np.nan                          # (never read)
        rows = np.zeros((c.n, 4), np.float32)
        rows[:, 0] = 0.01 * rng.standard_normal(c.n)
        rows[:, 1] = rng.integers(0, 4, c.n)
        rows[:, 2] = 1.0 + rng.standard_normal(c.n)
        rows[:, 3] = 0.3 * rng.standard_normal(c.n) + 0.1
        d.update(terms=t, rows=rows, inv_b=f32(1.0 / c.n))
    else:
        d["traj_loss"] = (3.0 + rng.random(c.n)).astype(np.float32)
        ts = rng.random((c.n, IMPALA_TRAJ_FLOATS)).astype(np.float32) + 0.5
        ts[:, 10], ts[:, 11] = 7.0, 0.0
        d["traj_stats"] = ts
    return d


def impala_stats_ref(stats, ts):
    """impala_stats_reduce: column c of the rows into slot 2 + c (column 9 a maximum), 10 the transitions, a chunk"""
    out, ts = np.array(stats, np.float64), np.asarray(ts, np.float64)
    out[0] += 1.0
    out[1] += ts[:, 10].sum()
    out[2:11] += ts[:, :9].sum(axis=0)
    out[11] = max(out[11], ts[:, 9].max())
    return out


# ---------------------------------------------------------------- optimisers: cases
OptCase = collections.namedtuple("OptCase", "id opt count npartial side gs lr_dev stats")
BIG = 512 * 256 * 4 + 1029           # = 2048 * 256 + 1029: one element past one grid-stride trip of either kernel, odd tail


def opt(id, opt_type, count, npartial, side, gs=1.0, lr_dev=False, stats=False):
    """side: "below" / "above" (the norm at half / twice the clip norm) or "zero" (zero gradient, zero partials)"""
    return OptCase(id, opt_type, count, npartial, side, gs, lr_dev, stats)


OPT_CASES = [
    opt("o_adam_c1_p1", OPT_ADAM, 1, 1, "above"),
    opt("o_adam_c2_p255", OPT_ADAM, 2, 255, "below", gs=0.5),
    opt("o_adam_c3_p256", OPT_ADAM, 3, 256, "above", gs=1.0 / 3.0, stats=True),
    opt("o_adam_c4_p257", OPT_ADAM, 4, 257, "below", stats=True),
    opt("o_adam_c5_p2048", OPT_ADAM, 5, 2048, "above", gs=0.5),
    opt("o_adam_c1003_p2049", OPT_ADAM, 1003, 2049, "below", gs=1.0 / 3.0),
    opt("o_adam_c1003_p2300", OPT_ADAM, 1003, 2300, "above", stats=True),
    opt("o_adam_c1003_zero", OPT_ADAM, 1003, 257, "zero"),
    opt("o_adam_big_p2300", OPT_ADAM, BIG, 2300, "above", gs=0.5),
    opt("o_rms_c1_p2300", OPT_RMSPROP, 1, 2300, "below", lr_dev=True),
    opt("o_rms_c2_p2049", OPT_RMSPROP, 2, 2049, "above", gs=1.0 / 3.0),
    opt("o_rms_c3_p2048", OPT_RMSPROP, 3, 2048, "below", gs=0.5, stats=True),
    opt("o_rms_c4_p257", OPT_RMSPROP, 4, 257, "above", lr_dev=True, stats=True),
    opt("o_rms_c5_p256", OPT_RMSPROP, 5, 256, "below"),
    opt("o_rms_c1003_p255", OPT_RMSPROP, 1003, 255, "above", gs=0.5),
    opt("o_rms_c1003_zero", OPT_RMSPROP, 1003, 1, "zero", lr_dev=True),
    opt("o_rms_big_p1", OPT_RMSPROP, BIG, 1, "above", gs=1.0 / 3.0),
]
OPT_CLIP = 0.7
OPT_STEPS = 3


def opt_data(c):
    """parameters of scale 0.1, zero moments (the steps that follow carry their history: the update is then of the size of
    lr, comparable to the parameter), and per step a unit-normal gradient and a synthetic partial array whose norm lies on
    the case's side of the clip norm (times grad_scale)"""
    rng = case_rng(c.id, 2)
    d = dict(p=param_like(rng, c.count), m=np.zeros(c.count, np.float32), v=np.zeros(c.count, np.float32), g=[], partial=[])
    sign = rng.choice([-1.0, 1.0], c.count)
    for _ in range(OPT_STEPS):
        # (the clipped gradient is of unit size: RMSProp's step lr * g / sqrt(0.1 + ...) is then of the size of lr too)
        g = grad_like(rng, sign, 1.0 / ((0.5 if c.side == "above" else 1.0) * c.gs))
        w = rng.random(c.npartial) + 0.5
        target = {"below": 0.5, "above": 2.0, "zero": 0.0}[c.side] * OPT_CLIP / c.gs
        part = (w / w.sum() * target ** 2).astype(np.float32)
        d["g"].append(g * 0 if c.side == "zero" else g)
        d["partial"].append(part)
    return d


KerasCase = collections.namedtuple("KerasCase", "id sizes clipnorm sides")
KERAS_CASES = [
    # sizes 1 .. 17: norm (of unit normals) at most ~6; 4099: ~64; 131075 (one past a 512 x 256 grid-stride trip): ~362
    KerasCase("k_mixed_clip16", (1, 15, 16, 17, 4099, 131075), 16.0, (0, 0, 0, 0, 1, 1)),
    KerasCase("k_mixed_noclip", (1, 15, 16, 17, 4099, 131075), 0.0, (0, 0, 0, 0, 0, 0)),
    KerasCase("k_seg32", tuple(1 + (5 * i) % 11 if i % 2 else 300 + 7 * i for i in range(32)), 8.0,
              tuple(0 if i % 2 else 1 for i in range(32))),
]


def keras_data(c):
    """segments at offsets that are no multiple of 4 (canaries between them), unit-normal gradients per step"""
    rng = case_rng(c.id, 3)
    segs, off = [], 1
    for n in c.sizes:
        if off % 4 == 0:
            off += 1
        segs.append((off, n))
        off += n + 3
    total = align4(off)
    inside = np.zeros(total, bool)
    for o, n in segs:
        inside[o:o + n] = True
    pick = lambda x: np.where(inside, x, CANARY).astype(np.float32)
    sign = np.sign(rng.standard_normal(total))
    d = dict(segs=segs, total=total, inside=inside, p=pick(param_like(rng, total)),
             m=pick(np.zeros(total)), v=pick(np.zeros(total)),
             g=[pick(np.abs(rng.standard_normal(total)) * sign) for _ in range(OPT_STEPS)])
    for g in d["g"]:      # the sides the row names, ratio 1.5 or more
        for (o, n), side in zip(segs, c.sides):
            norm = np.sqrt((g[o:o + n].astype(np.float64) ** 2).sum())
            assert c.clipnorm == 0 or (norm > 1.5 * c.clipnorm if side else 1.5 * norm < c.clipnorm), (c.id, n, norm)
    return d


def keras_lr_t(step):
    """Keras Adam's step size of step `step` (1-based), formed on the host"""
    return f32(LR * np.sqrt(1.0 - float(f32(B2)) ** step) / (1.0 - float(f32(B1)) ** step))


# ---------------------------------------------------------------- device plumbing
@pytest.fixture(scope="module")
def L():
    from xingtian_amd import lib
    lib.load()
    return lib


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def plan_of(lib, c, form=0, select=0, max_partials=1 << 14):
    """xt_grads_finish_plan_ex on the case's table with placeholder (aligned, never dereferenced) addresses -> (entries,
    npartials, grid)"""
    n = len(c.ents)
    arr = (lib.GradEntry * n)()
    for i, e in enumerate(c.ents):
        arr[i].src, arr[i].dst = 4096 * (i + 1), 4096 * (i + 1) if e.inplace else 4096 * (i + 100)
        arr[i].count, arr[i].nslab, arr[i].stride, arr[i].pre = e.count, e.nslab, align4(e.count) + e.pad, e.pre
    npart, grid = ctypes.c_int32(-1), ctypes.c_int32(-1)
    lib.check(lib.load().xt_grads_finish_plan_ex(arr, n, select, c.early, form, max_partials, ctypes.byref(npart),
                                                 ctypes.byref(grid)), "xt_grads_finish_plan_ex")
    return arr, npart.value, grid.value


def assert_plan(c, arr, npart):
    for i, e in enumerate(c.ents):
        assert (arr[i].zl, arr[i].nblk, arr[i].pblk0) == (e.zl, e.nblk, c.pblk0[i]), (c.id, i, arr[i].zl, arr[i].nblk, arr[i].pblk0)
    assert npart == c.npart, (c.id, npart)


class Knobs:
    """the case's tuning knobs for the length of a with block"""
    def __init__(self, lib, knobs):
        self.lib, self.knobs = lib, knobs

    def __enter__(self):
        self.old = self.lib.set_tuning(**self.knobs) if self.knobs else {}

    def __exit__(self, *exc):
        if self.old:
            self.lib.set_tuning(**self.old)


class Tail:
    """the device buffers of one reduction table and the launches on them"""
    def __init__(self, lib, c, d):
        self.lib, self.c, self.d = lib, c, d
        self.srcs = [None if s is None else dev(s) for s in d["srcs"]]
        self.flat = dev(d["flat"])
        self.partial = torch.full((c.npart + PART_TAIL,), CANARY, device="cuda")
        for i, vals in d["pre"].items():
            self.partial[c.pblk0[i]:c.pblk0[i] + len(vals)] = dev(vals)
        self.counter = torch.zeros(lib.FINISH_COUNTER_WORDS, dtype=torch.int32, device="cuda")
        self.entries = (lib.GradEntry * len(c.ents))()
        for i, e in enumerate(c.ents):
            dst = self.flat.data_ptr() + 4 * d["offs"][i]
            E = self.entries[i]
            E.src, E.dst = dst if e.inplace else self.srcs[i].data_ptr(), dst
            E.count, E.nslab, E.stride, E.pre = e.count, e.nslab, align4(e.count) + e.pad, e.pre

    def args(self, form, **kw):
        a = self.lib.FinishArgs()
        a.form, a.partial, a.max_partials = form, self.partial.data_ptr(), self.c.npart + PART_TAIL
        for k, v in kw.items():
            setattr(a, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
        return a

    def launch(self, a, select=0):
        """-> the form that ran; asserts the plan the launch reports against the row"""
        form_out, npart = ctypes.c_int32(-9), ctypes.c_int32(-9)
        self.lib.check(self.lib.load().xt_grads_finish_ex(self.entries, len(self.c.ents), select, self.c.early, ctypes.byref(a),
                                                          None, ctypes.byref(form_out), ctypes.byref(npart)),
                       "xt_grads_finish_ex")
        assert_plan(self.c, self.entries, npart.value)
        return form_out.value


def figures(rows):
    """"name measured/bar (f32 oracle x)" of [(name, measured, bar, oracle error or None)]"""
    return "; ".join("{} {:.2e}/{:g}{}".format(n, m, b, "" if o is None else " (f32 oracle {:.2e})".format(o))
                     for n, m, b, o in rows)


def report(cid, plan, rows):
    print("OPTIM_PARITY | `{}` | {} | {} |".format(cid, plan, figures(rows)))
    for n, m, b, _ in rows:
        assert within(m, b), (cid, n, m, b)


def check_reduction(c, d, ref, flat, partial, rows, tag=""):
    """dst bit for bit against the twin (canaries included) and against float64; every partial slot; the canary tail"""
    assert not np.isnan(flat).any() and not np.isnan(partial).any(), c.id
    assert bits_differ(flat, flat_expected(c, d, ref["twin"])) == 0, c.id
    for i, e in enumerate(c.ents):
        got = flat[d["offs"][i]:d["offs"][i] + e.count]
        rows.append(("{}dst{}".format(tag, i if len(c.ents) > 1 else ""), rel2(got, ref["ref64"][i]), BAR_ELEM,
                     rel2(ref["twin"][i], ref["ref64"][i])))
        if e.pre:
            assert bits_differ(partial[c.pblk0[i]:c.pblk0[i] + e.pre], d["pre"][i]) == 0, (c.id, i)
    rows.append((tag + "partial", slots_err(partial[:c.npart], ref["partial"]), BAR_ELEM, None))
    assert (partial[c.npart:] == CANARY).all(), c.id


# ---------------------------------------------------------------- tests: reduction
@pytest.mark.parametrize("c", RED_CASES, ids=lambda c: c.id)
def test_reduction_vs_twin_and_float64(L, c):
    d = red_data(c)
    ref = red_reference(c, d)
    with Knobs(L, c.knobs):
        arr, npart, grid = plan_of(L, c)
        assert_plan(c, arr, npart)
        assert grid == c.grid, (c.id, grid)
        t = Tail(L, c, d)
        assert t.launch(t.args(0)) == 0
        flat, partial = host(t.flat), host(t.partial)
        rows = []
        check_reduction(c, d, ref, flat, partial, rows)
        if c.early:
            # the early entries first, then the rest: the same dst and the same partial slots as the one launch
            t2 = Tail(L, c, d)
            allm = (1 << len(c.ents)) - 1
            assert t2.launch(t2.args(0), select=c.early) == 0
            early_only = host(t2.partial)
            for i, e in enumerate(c.ents):
                if not (c.early >> i) & 1 and not e.pre:
                    assert (early_only[c.pblk0[i]:c.pblk0[i] + e.nblk] == CANARY).all(), (c.id, i)
            assert t2.launch(t2.args(0), select=allm & ~c.early) == 0
            assert bits_differ(host(t2.flat), flat) == 0 and bits_differ(host(t2.partial), partial) == 0, c.id
    report(c.id, "zl {} nblk {} npart {} grid {}".format("/".join(str(e.zl) for e in c.ents),
                                                         "/".join(str(e.nblk) for e in c.ents), c.npart, c.grid), rows)


# ---------------------------------------------------------------- tests: the four launch forms
def form_setup(L, c):
    rc = RED_BY_ID[c.table]
    d, fd = red_data(rc), form_data(c)
    ref = red_reference(rc, d)
    gn1, _ = clip_ref(ref["partial"].astype(np.float32), 1.0, c.gs)      # the norm, to place the clip norm on the case's side
    clip = f32(float(gn1) * (0.5 if c.side == "above" else 2.0))
    rng = case_rng(c.id, 4)
    # parameters of scale 0.1 and zero moments where an entry lies, canaries elsewhere
    pm = {k: np.full(d["total"], CANARY, np.float32) for k in "pmv"}
    for i, e in enumerate(rc.ents):
        s = slice(d["offs"][i], d["offs"][i] + e.count)
        pm["p"][s] = param_like(rng, e.count)
        pm["m"][s] = pm["v"][s] = 0
    return rc, d, fd, ref, clip, pm


class FormRun:
    """one form's buffers: two steps in a row on the same counter, state, loss accumulators and parameters"""
    def __init__(self, L, c, rc, d, fd, clip, pm, form):
        self.L, self.c, self.form, self.clip = L, c, form, clip
        self.t = Tail(L, rc, d)
        self.state = dev(fd["state0"])
        self.out = torch.full((4,), CANARY, device="cuda")
        self.acc = dev(np.array(ACC0, np.float32))
        self.stats = dev(fd["stats0"])
        self.p, self.m, self.v = dev(pm["p"]), dev(pm["m"]), dev(pm["v"])
        self.lr_dev = dev(np.array([LR], np.float32)) if c.lr_dev else None
        kw = dict(clip_norm=float(clip), grad_scale=c.gs, lr=999.0 if c.lr_dev else LR, beta1=B1, beta2=B2, eps=ADAM_EPS,
                  state=self.state, counter=self.t.counter, out=self.out, acc=self.acc)
        if c.lr_dev:
            kw["lr_dev"] = self.lr_dev
        if c.loss == "ppo":
            self.terms, self.rows = dev(fd["terms"]), dev(fd["rows"])
            kw.update(terms=self.terms, B=c.n, ent_coef=PPO_ENT, critic_coef=PPO_CRITIC, inv_b=float(fd["inv_b"]), rows=self.rows)
        else:
            self.traj_loss, self.traj_stats = dev(fd["traj_loss"]), dev(fd["traj_stats"])
            kw.update(traj_loss=self.traj_loss, n_traj=c.n, acc_set=c.acc_set, traj_stats=self.traj_stats)
        if c.stats:
            kw["stats"] = self.stats
        if form == 3:
            kw.update(params=self.p, m=self.m, v=self.v, grads_base=self.t.flat)
        self.a = self.t.args(form, **kw)

    def step(self):
        """-> the form that ran, and a host copy of everything the step may write"""
        ran = self.t.launch(self.a)
        if ran == 2:      # the optimiser's own launch behind the extra-block form
            # (one launch per entry: the canaries between the entries are no parameters; the norm goes to the statistics once,
            # as in the step's own two-launch Adam)
            L, rc = self.L, self.t.c
            for i, e in enumerate(rc.ents):
                at = lambda t: t.data_ptr() + 4 * self.t.d["offs"][i]
                L.check(L.load().xt_optim_clip_ex(OPT_ADAM, at(self.p), at(self.t.flat), at(self.m), at(self.v), e.count, 0.0,
                                                  None, B1, B2, ADAM_EPS, L.ptr(self.state), L.ptr(self.t.partial), rc.npart,
                                                  float(self.clip), self.c.gs,
                                                  L.ptr(self.stats) if self.c.stats and i == 0 else None, None),
                        "xt_optim_clip_ex")
        snap = {k: host(getattr(self, k)).copy() for k in ("state", "out", "acc", "stats", "p", "m", "v")}
        return ran, dict(snap, flat=host(self.t.flat).copy(), partial=host(self.t.partial).copy(),
                         counter=host(self.t.counter).copy())


@pytest.mark.parametrize("c", FORM_CASES, ids=lambda c: c.id)
def test_launch_forms_vs_float64_and_each_other(L, c):
    rc, d, fd, ref, clip, pm = form_setup(L, c)
    has_pre = any(e.pre for e in rc.ents)
    runs = {}
    for form in (2, 3) if has_pre else (1, 2, 3):
        _, _, grid = plan_of(L, rc, form=form)
        body = sum(e.nblk for e in rc.ents if form == 3 or not e.pre)
        assert grid == body + (1 if form >= 2 else 0), (c.id, form, grid)
        r = FormRun(L, c, rc, d, fd, clip, pm, form)
        steps = []
        for _ in range(2):
            ran, snap = r.step()
            if form == 3 and ran == 2:
                pytest.skip("the device holds fewer resident blocks than the fused grid of {} needs".format(grid))
            assert ran == form, (c.id, form, ran)
            steps.append(snap)
        runs[form] = steps
    rows = []
    # ---- every form against the float64 reference, step by step (each step's reference starts from the step's own inputs)
    for form, steps in runs.items():
        state_prev, acc_prev, stats_prev = fd["state0"], np.array(ACC0, np.float32), fd["stats0"]
        p_prev, m_prev, v_prev = pm["p"], pm["m"], pm["v"]
        for k, s in enumerate(steps):
            tag = "f{}s{}.".format(form, k + 1)
            red_rows = []
            check_reduction(rc, d, ref, s["flat"], s["partial"], red_rows, tag)
            if form == 1 and k == 0:
                rows += red_rows
            else:
                for n, m_, b, _ in red_rows:
                    assert within(m_, b), (c.id, n, m_)
            assert (s["counter"][:32 * 65] == 0).all(), (c.id, form, k)      # tickets re-armed; the sense word flips per fused launch
            assert s["counter"][32 * 65] == ((k + 1) & 1 if form == 3 else 0), (c.id, form, k)
            gn, sc = clip_ref(s["partial"][:rc.npart], clip, c.gs)
            gn32, sc32 = clip_ref(s["partial"][:rc.npart], clip, c.gs, np.float32)
            b1p, b2p, alpha, cnt = advance_ref(state_prev, LR)
            _, _, alpha32, _ = advance_ref(state_prev, LR, np.float32)
            st = s["state"]
            assert bits_differ(st[:2], np.array([b1p, b2p])) == 0 and st[5] == cnt and st[6] == 0 and st[7] == 0, (c.id, form, st)
            rows += [(tag + "gnorm", rel1(st[4], gn), BAR_NORM, rel1(gn32, gn)), (tag + "scale", rel1(st[2], sc), BAR_NORM, rel1(sc32, sc)),
                     (tag + "alpha", rel1(st[3], alpha), BAR_NORM, rel1(alpha32, alpha))]
            assert (float(gn) > float(clip)) == (c.side == "above")
            # loss block
            stats_ref = np.array(stats_prev)
            if c.loss == "ppo":
                lref, surr = ppo_loss_ref(fd["terms"], PPO_ENT, PPO_CRITIC, fd["inv_b"])
                l32, _ = ppo_loss_ref(fd["terms"], PPO_ENT, PPO_CRITIC, fd["inv_b"], np.float32)
                for j, nm in enumerate(("loss", "actor", "vf", "ent")):
                    rows.append((tag + nm, rel1(s["out"][j], lref[j]), BAR_LOSS, rel1(l32[j], lref[j])))
                acc_ref = (float(acc_prev[0]) + lref[0], float(acc_prev[1]) + 1.0)
                if c.stats:
                    stats_ref[0] += 1.0
                    stats_ref[1] += c.n
                    stats_ref[2:5] += (surr, lref[3], lref[2])
                    stats_ref[5:12] += ppo_rows_ref(fd["rows"])
            else:
                lref = fd["traj_loss"].astype(np.float64).sum()
                rows.append((tag + "loss", rel1(s["out"][0], lref), BAR_LOSS, rel1(np.cumsum(fd["traj_loss"], dtype=np.float32)[-1], lref)))
                assert (s["out"][1:] == CANARY).all(), c.id
                acc_ref = (lref, 1.0) if c.acc_set else (float(acc_prev[0]) + lref, float(acc_prev[1]) + 1.0)
                if c.stats:
                    stats_ref = impala_stats_ref(stats_ref, fd["traj_stats"])
            rows.append((tag + "acc", rel1(s["acc"][0], acc_ref[0]), BAR_LOSS, None))
            assert s["acc"][1] == acc_ref[1], (c.id, form, s["acc"])
            if c.stats:
                stats_ref = gnorm_stats_ref(stats_ref, gn, clip)
                assert s["stats"][14] == stats_ref[14] and s["stats"][15] == stats_ref[15], (c.id, form, s["stats"])
                rows.append((tag + "stats.sums", rel2(s["stats"][:12], stats_ref[:12]), BAR_ELEM, None))
                rows += [(tag + "stats.gnorm_sum", rel1(s["stats"][12], stats_ref[12]), BAR_NORM, None),
                         (tag + "stats.gnorm_max", rel1(s["stats"][13], stats_ref[13]), BAR_NORM, None)]
            else:
                assert (s["stats"] == fd["stats0"]).all(), (c.id, form)
            # the update (form 1 has no optimiser launch behind it here: its parameters stay)
            if form == 1:
                for key in ("p", "m", "v"):
                    assert bits_differ(s[key], pm[key]) == 0, (c.id, key)
            else:
                live = pm["p"] != CANARY
                g = flat_expected(rc, d, ref["twin"])
                mr, vr, ur = adam_ref(p_prev[live], g[live], m_prev[live], v_prev[live], sc, alpha)
                m32, v32, u32 = adam_ref(p_prev[live], g[live], m_prev[live], v_prev[live], sc32, alpha32, np.float32)
                upd = s["p"][live].astype(np.float64) - p_prev[live].astype(np.float64)
                rows += [(tag + "m", rel2(s["m"][live], mr), BAR_ELEM, rel2(m32, mr)), (tag + "v", rel2(s["v"][live], vr), BAR_ELEM, rel2(v32, vr)),
                         (tag + "update", rel2(upd, ur), BAR_ELEM, rel2(u32, ur))]
                for key in ("p", "m", "v"):
                    assert (s[key][~live] == CANARY).all(), (c.id, form, key)
            state_prev, acc_prev, stats_prev = s["state"], s["acc"], s["stats"]
            p_prev, m_prev, v_prev = s["p"], s["m"], s["v"]
    # ---- the forms against each other, bit for bit
    scalars = ("state", "out", "acc", "flat", "partial")
    for k in range(2):
        if 1 in runs:
            for key in scalars:
                assert bits_differ(runs[1][k][key], runs[2][k][key]) == 0, (c.id, "1 vs 2", k, key)
            assert (runs[1][k]["stats"] == runs[2][k]["stats"]).all(), (c.id, "1 vs 2 stats", k)
        for key in scalars + ("p", "m", "v"):
            assert bits_differ(runs[2][k][key], runs[3][k][key]) == 0, (c.id, "2 vs 3", k, key)
        assert (runs[2][k]["stats"] == runs[3][k]["stats"]).all(), (c.id, "2 vs 3 stats", k)
    report(c.id, "table {} forms {}".format(c.table, "/".join(str(f) for f in runs)), rows)


def test_forms_0_to_2_leave_a_pre_reduced_entry_alone_and_the_fused_tail_updates_it(L):
    """(the pre-reduced entry of r_tpre: its dst and slots stay in every form -- checked for every form by check_reduction --
    and only form 3 launches blocks for it, which apply the update: part of the bitwise 2 + clip vs 3 comparison above)"""
    rc = RED_BY_ID["r_tpre"]
    grids = [plan_of(L, rc, form=f)[2] for f in (0, 2, 3)]
    assert grids == [4, 5, 6]
    arr = plan_of(L, rc, form=3)[0]
    assert arr[1].nblk == 1 and arr[1].pblk0 == 0


# ---------------------------------------------------------------- tests: optimisers on synthetic partials
@pytest.mark.parametrize("c", OPT_CASES, ids=lambda c: c.id)
def test_optimiser_vs_float64(L, c):
    lib = L.load()
    d = opt_data(c)
    p, m, v = dev(d["p"]), dev(d["m"]), dev(d["v"])
    state = dev(np.array([1, 1, 0, 0, 0, 0, 0, 0], np.float32))
    stats0 = 0.5 * np.arange(16, dtype=np.float64)
    stats = dev(stats0)
    lr_dev = dev(np.array([LR], np.float32)) if c.lr_dev else None
    rows = []
    p_prev, m_prev, v_prev, state_prev, stats_prev = d["p"], d["m"], d["v"], host(state), stats0
    for k in range(OPT_STEPS):
        tag = "s{}.".format(k + 1)
        g, partial = dev(d["g"][k]), dev(np.concatenate([d["partial"][k], np.full(8, np.nan, np.float32)]))
        gn, sc = clip_ref(d["partial"][k], OPT_CLIP, c.gs)
        gn32, sc32 = clip_ref(d["partial"][k], OPT_CLIP, c.gs, np.float32)
        if c.opt == OPT_ADAM:
            # mode 1 of the step's tail: the one-block finalize (beta powers, step size; also norm and clip factor)
            a = L.FinishArgs()
            a.clip_norm, a.grad_scale, a.lr, a.beta1, a.beta2 = OPT_CLIP, c.gs, LR, B1, B2
            a.state = state.data_ptr()
            L.check(lib.xt_norm_finalize_ex(L.ptr(partial), c.npartial, ctypes.byref(a), None), "xt_norm_finalize_ex")
            fin_state = host(state).copy()
            b1p, b2p, alpha, cnt = advance_ref(state_prev, LR)
            _, _, alpha32, _ = advance_ref(state_prev, LR, np.float32)
            assert bits_differ(fin_state[:2], np.array([b1p, b2p])) == 0 and fin_state[5] == cnt, (c.id, fin_state)
            rows.append((tag + "alpha", rel1(fin_state[3], alpha), BAR_NORM, rel1(alpha32, alpha)))
            state[2], state[4] = CANARY, CANARY      # (the optimiser launch derives both again)
        L.check(lib.xt_optim_clip_ex(c.opt, L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), c.count, 999.0 if c.lr_dev else LR,
                                     L.ptr(lr_dev), RMS_DECAY if c.opt == OPT_RMSPROP else B1, B2,
                                     RMS_EPS if c.opt == OPT_RMSPROP else ADAM_EPS, L.ptr(state), L.ptr(partial), c.npartial,
                                     OPT_CLIP, c.gs, L.ptr(stats) if c.stats else None, None), "xt_optim_clip_ex")
        st, pn, mn, vn = host(state).copy(), host(p).copy(), host(m).copy(), host(v).copy()
        if c.opt == OPT_ADAM:
            assert bits_differ(st[[2, 4]], fin_state[[2, 4]]) == 0 and bits_differ(st[[0, 1, 3, 5, 6, 7]], fin_state[[0, 1, 3, 5, 6, 7]]) == 0
            mr, vr, ur = adam_ref(p_prev, d["g"][k], m_prev, v_prev, sc, alpha)
            m32, v32, u32 = adam_ref(p_prev, d["g"][k], m_prev, v_prev, sc32, alpha32, np.float32)
        else:
            assert bits_differ(st[[0, 1, 3, 5, 6, 7]], state_prev[[0, 1, 3, 5, 6, 7]]) == 0
            mr, vr, ur = rmsprop_ref(p_prev, d["g"][k], m_prev, v_prev, sc, LR)
            m32, v32, u32 = rmsprop_ref(p_prev, d["g"][k], m_prev, v_prev, sc32, LR, np.float32)
        assert (float(gn) > OPT_CLIP * 1.4) == (c.side == "above") and (c.side != "zero" or float(gn) == 0.0)
        upd = pn.astype(np.float64) - p_prev.astype(np.float64)
        rows += [(tag + "gnorm", rel1(st[4], gn), BAR_NORM, rel1(gn32, gn)), (tag + "scale", rel1(st[2], sc), BAR_NORM, rel1(sc32, sc)),
                 (tag + "m", rel2(mn, mr), BAR_ELEM, rel2(m32, mr)), (tag + "v", rel2(vn, vr), BAR_ELEM, rel2(v32, vr)),
                 (tag + "update", rel2(upd, ur), BAR_ELEM, rel2(u32, ur))]
        if c.stats:
            sref = gnorm_stats_ref(stats_prev, gn, OPT_CLIP)
            sg = host(stats).copy()
            assert (sg[:12] == sref[:12]).all() and sg[14] == sref[14] and sg[15] == sref[15], (c.id, sg)
            rows += [(tag + "stats.gnorm_sum", rel1(sg[12], sref[12]), BAR_NORM, None),
                     (tag + "stats.gnorm_max", rel1(sg[13], sref[13]), BAR_NORM, None)]
            stats_prev = sg
        else:
            assert (host(stats) == stats0).all(), c.id
        p_prev, m_prev, v_prev, state_prev = pn, mn, vn, st
    name = "adam_tf_clip_kernel" if c.opt == OPT_ADAM else "rmsprop_tf_clip_kernel"
    report(c.id, "{} count {} partials {} {}".format(name, c.count, c.npartial, c.side), rows)


@pytest.mark.parametrize("loss,n", [("ppo", 1), ("ppo", 255), ("ppo", 256), ("ppo", 257), ("ppo", 300), ("impala", 1), ("impala", 3)])
def test_norm_finalize_loss_block_vs_float64(L, loss, n):
    """mode 1 of net_apply with the loss arguments: the PPO scalars at B on both sides of the block's 256 threads, IMPALA's
    trajectory sum with both acc_set values"""
    lib = L.load()
    c = FormCase("nf_{}_{}".format(loss, n), None, loss, n, n & 1, False, False, "above", 0.5)
    fd = form_data(c)
    rng = case_rng(c.id, 5)
    partial = (rng.random(300) + 0.5).astype(np.float32)
    state, out, acc = dev(fd["state0"]), torch.full((4,), CANARY, device="cuda"), dev(np.array(ACC0, np.float32))
    a = L.FinishArgs()
    a.clip_norm, a.grad_scale, a.lr, a.beta1, a.beta2 = 3.0, c.gs, LR, B1, B2
    a.state, a.out, a.acc = state.data_ptr(), out.data_ptr(), acc.data_ptr()
    keep = []
    if loss == "ppo":
        keep = [dev(fd["terms"])]
        a.terms, a.B, a.ent_coef, a.critic_coef, a.inv_b = keep[0].data_ptr(), n, PPO_ENT, PPO_CRITIC, float(fd["inv_b"])
        lref = ppo_loss_ref(fd["terms"], PPO_ENT, PPO_CRITIC, fd["inv_b"])[0]
        l32 = ppo_loss_ref(fd["terms"], PPO_ENT, PPO_CRITIC, fd["inv_b"], np.float32)[0]
        acc_ref = (ACC0[0] + lref[0], ACC0[1] + 1)
    else:
        keep = [dev(fd["traj_loss"])]
        a.traj_loss, a.n_traj, a.acc_set = keep[0].data_ptr(), n, c.acc_set
        lref = np.array([fd["traj_loss"].astype(np.float64).sum()])
        l32 = np.array([np.cumsum(fd["traj_loss"], dtype=np.float32)[-1]])
        acc_ref = (lref[0], 1.0) if c.acc_set else (ACC0[0] + lref[0], ACC0[1] + 1)
    L.check(lib.xt_norm_finalize_ex(L.ptr(dev(partial)), 300, ctypes.byref(a), None), "xt_norm_finalize_ex")
    st, o, ac = host(state), host(out), host(acc)
    gn, sc = clip_ref(partial, 3.0, c.gs)
    gn32, sc32 = clip_ref(partial, 3.0, c.gs, np.float32)
    b1p, b2p, alpha, cnt = advance_ref(fd["state0"], LR)
    assert bits_differ(st[:2], np.array([b1p, b2p])) == 0 and st[5] == 1 and st[6] == 0 and ac[1] == acc_ref[1]
    rows = [("gnorm", rel1(st[4], gn), BAR_NORM, rel1(gn32, gn)), ("scale", rel1(st[2], sc), BAR_NORM, rel1(sc32, sc)),
            ("alpha", rel1(st[3], alpha), BAR_NORM, None), ("acc", rel1(ac[0], acc_ref[0]), BAR_LOSS, None)]
    rows += [("out{}".format(j), rel1(o[j], lref[j]), BAR_LOSS, rel1(l32[j], lref[j])) for j in range(len(lref))]
    assert (o[len(lref):] == CANARY).all()
    report(c.id, "norm_finalize_kernel {} n {} acc_set {}".format(loss, n, c.acc_set), rows)


ADAM3_CASES = [(1, "above", 1.0), (2, "below", 0.5), (3, "above", 1.0 / 3.0), (4, "below", 1.0), (5, "above", 0.5),
               (1003, "below", 1.0 / 3.0), (1003, "zero", 1.0), (BIG, "above", 1.0)]


def adam_tf_clip_steps(L, count, side, gs, lr=LR, steps=OPT_STEPS, seed_id=None, pscale=0.1):
    """xt_adam_tf_clip (its own squared-norm launch + finalize + adam_tf_kernel) for `steps` steps against float64 -> rows.
    The reference norm is that of the float32 gradient; the partials are the launch's own (one rounding each: inside the bar)"""
    lib = L.load()
    rng = case_rng(seed_id or "a3_{}_{}".format(count, side))
    p0 = param_like(rng, count) * f32(pscale / 0.1)
    sign = rng.choice([-1.0, 1.0], count)
    p, m, v = dev(p0), torch.zeros(count, device="cuda"), torch.zeros(count, device="cuda")
    state, scratch = torch.zeros(8, device="cuda"), torch.zeros(1024, device="cuda")
    L.check(lib.xt_adam_state_init(L.ptr(state), None), "init")
    p_prev, m_prev, v_prev, state_prev = p0, np.zeros(count, np.float32), np.zeros(count, np.float32), host(state).copy()
    rows = []
    for k in range(steps):
        tag = "s{}.".format(k + 1)
        g = grad_like(rng, sign, 0.01 if k % 2 else 1.0)
        if side == "zero":
            g *= 0
        sq = np.array([(g.astype(np.float64) ** 2).sum()])
        gn1 = float(np.sqrt(sq[0])) * float(f32(gs))
        clip = f32({"above": 0.5, "below": 2.0, "zero": 1.0}[side] * (gn1 if gn1 > 0 else 1.0))
        # (clip_ref takes float32 partials; the exact float64 sum of squares is handed over as one "partial")
        gn = np.sqrt(sq[0]) * float(f32(gs))
        with np.errstate(divide="ignore"):
            sc = float(clip) * min(1.0 / gn, 1.0 / float(clip)) * float(f32(gs))
        L.check(lib.xt_adam_tf_clip(L.ptr(p), L.ptr(dev(g)), L.ptr(m), L.ptr(v), count, lr, B1, B2, ADAM_EPS, float(clip), gs,
                                    L.ptr(state), L.ptr(scratch), None), "xt_adam_tf_clip")
        st, pn, mn, vn = host(state).copy(), host(p).copy(), host(m).copy(), host(v).copy()
        b1p, b2p, alpha, cnt = advance_ref(state_prev, lr)
        _, _, alpha32, _ = advance_ref(state_prev, lr, np.float32)
        assert bits_differ(st[:2], np.array([b1p, b2p])) == 0 and st[5] == cnt, (count, st)
        mr, vr, ur = adam_ref(p_prev, g, m_prev, v_prev, sc, alpha)
        m32, v32, u32 = adam_ref(p_prev, g, m_prev, v_prev, f32(sc), alpha32, np.float32)
        upd = pn.astype(np.float64) - p_prev.astype(np.float64)
        rows += [(tag + "gnorm", rel1(st[4], gn), BAR_NORM, None), (tag + "scale", rel1(st[2], sc), BAR_NORM, None),
                 (tag + "alpha", rel1(st[3], alpha), BAR_NORM, rel1(alpha32, alpha)),
                 (tag + "m", rel2(mn, mr), BAR_ELEM, rel2(m32, mr)), (tag + "v", rel2(vn, vr), BAR_ELEM, rel2(v32, vr)),
                 (tag + "update", rel2(upd, ur), BAR_ELEM, rel2(u32, ur))]
        p_prev, m_prev, v_prev, state_prev = pn, mn, vn, st
    return rows


@pytest.mark.parametrize("count,side,gs", ADAM3_CASES, ids=lambda x: str(x) if not isinstance(x, float) else "gs{:.2f}".format(x))
def test_adam_tf_clip_three_launch_vs_float64(L, count, side, gs):
    report("a3_c{}_{}".format(count, side), "sqnorm_partial + norm_finalize + adam_tf_kernel gs {:.3g}".format(gs),
           adam_tf_clip_steps(L, count, side, gs))


@pytest.mark.parametrize("c", KERAS_CASES, ids=lambda c: c.id)
def test_adam_keras_vs_float64(L, c):
    lib = L.load()
    d = keras_data(c)
    n = len(d["segs"])
    off = (ctypes.c_int64 * n)(*[o for o, _ in d["segs"]])
    size = (ctypes.c_int64 * n)(*[s for _, s in d["segs"]])
    p, m, v = dev(d["p"]), dev(d["m"]), dev(d["v"])
    scratch = torch.full((16 * n + 8,), CANARY, device="cuda")
    p_prev, m_prev, v_prev = d["p"], d["m"], d["v"]
    rows, ins = [], d["inside"]
    for k in range(OPT_STEPS):
        tag = "s{}.".format(k + 1)
        lr_t = keras_lr_t(k + 1)
        L.check(lib.xt_adam_keras(L.ptr(p), L.ptr(dev(d["g"][k])), L.ptr(m), L.ptr(v), n, off, size, c.clipnorm, float(lr_t),
                                  B1, B2, ADAM_EPS, L.ptr(scratch), None), "xt_adam_keras")
        pn, mn, vn = host(p).copy(), host(m).copy(), host(v).copy()
        mr, vr, ur = keras_ref(p_prev, d["g"][k], m_prev, v_prev, d["segs"], c.clipnorm, lr_t)
        m32, v32, u32 = keras_ref(p_prev, d["g"][k], m_prev, v_prev, d["segs"], c.clipnorm, lr_t, np.float32)
        upd = pn.astype(np.float64) - p_prev.astype(np.float64)
        rows += [(tag + "m", rel2(mn[ins], mr[ins]), BAR_ELEM, rel2(m32[ins], mr[ins])),
                 (tag + "v", rel2(vn[ins], vr[ins]), BAR_ELEM, rel2(v32[ins], vr[ins])),
                 (tag + "update", rel2(upd[ins], ur[ins]), BAR_ELEM, rel2(u32[ins], ur[ins]))]
        for x in (pn, mn, vn):
            assert (x[~ins] == CANARY).all(), c.id
        assert (host(scratch)[16 * n:] == CANARY).all(), c.id
        p_prev, m_prev, v_prev = pn, mn, vn
    report(c.id, "keras_seg_sqnorm_kernel + adam_keras_kernel, {} segments clipnorm {:g}".format(n, c.clipnorm), rows)
