"""GPU parity tests (run with -m gpu on an MI355X) of the fused head launches every PPO / IMPALA step runs, each called on
its own through the stand-alone entries of include/xt_mi355x.h: ppo_heads_fused_kernel<NQ, PART, SHARED> (16 instances),
impala_heads_fwd_kernel<NQ, PART> (8) + impala_vtrace_bwd_kernel<AM> (2) and heads_wgrad_partial_kernel.  Every row of
PPO_CASES / IMPALA_CASES names the instance it must take (XT_HEAD_PATH_* and the NQ / PART / SHARED / AM fields), so a
case that drifts onto another instance fails instead of passing there.  Reference: float64 on the same float32 inputs
(oracle.nets).  Output buffers are NaN-prefilled and end in a sentinel tail; float inputs end in a NaN tail.

The data and the float64 reference of every case are plain numpy (ppo_data / ppo_reference, ...):
tests/test_cpu_heads_coverage.py imports this module on the CPU, checks that every instance has cases and re-runs the
PPO references to check the gradient-branch populations and the boundary exclusions."""
import collections
import ctypes
import os
import re
import zlib

import numpy as np
import pytest
import torch

from oracle import nets

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_defines(prefix):
    """{name suffix: value} of the integer macros of include/xt_mi355x.h that start with `prefix`"""
    with open(os.path.join(ROOT, "include", "xt_mi355x.h")) as f:
        return {n: int(v) for n, v in re.findall(r"#define\s+{}(\w+)\s+(\d+)".format(prefix), f.read())}


def head_paths():
    return header_defines("XT_HEAD_PATH_")


def decode_head_path(v):
    """(family, nq, part, shared, am) of a path word"""
    s = {n: header_defines("XT_HEAD_" + n + "_")["SHIFT"] for n in ("NQ", "PART", "SHARED", "AM")}
    return v & 0xF, (v >> s["NQ"]) & 0xF, (v >> s["PART"]) & 1, (v >> s["SHARED"]) & 1, (v >> s["AM"]) & 0x3F


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------- PPO fused head: cases
PpoCase = collections.namedtuple("PpoCase", "id nq F A B shared ks act idx inv_b_mul probe")
PPO_CLIP, PPO_ENT, PPO_VF_CLIP, PPO_CRITIC = 0.1, 0.003, 0.5, 0.7
POOL_EXTRA = 13         # the label pools hold B + POOL_EXTRA rows


def ppo(id, nq, F, A, B, shared, ks=None, act="relu", idx=False, inv_b_mul=1.0, probe=False):
    """nq: the expected features-per-lane instance; ks: None = feature rows, an int or a (policy, value) pair = that many
    split-K partial slabs (PART); act: the trunk's activation (act_prev, and act_feat of the PART finish); idx: labels
    gathered through a permutation slice of a larger pool; inv_b_mul: inv_b = inv_b_mul / B; probe: one-hot feature rows
    and exactly representable weights (activation relu, act_feat none, zero trunk bias)"""
    if ks is not None and not isinstance(ks, tuple):
        ks = (ks, ks)
    return PpoCase(id, nq, F, A, B, shared, ks, "relu" if probe else act, idx, inv_b_mul, probe)


# F: 1 / 37 / 64 -> NQ 1, 65 / 100 / 128 -> NQ 2, 200 / 256 -> NQ 4, 300 / 512 -> NQ 8 (PpoCnn: F = 256 / 512, PpoMlp: 64)
PPO_CASES = [
    # ---- feature rows, shared trunk
    ppo("ppo_n1_sh_f37_a5", 1, 37, 5, 40, True, idx=True),
    ppo("ppo_n1_sh_f64_a1_probe", 1, 64, 1, 3, True, probe=True),
    ppo("ppo_n2_sh_f100_a8", 2, 100, 8, 40, True, act="tanh"),
    ppo("ppo_n2_sh_f65_a2_probe", 2, 65, 2, 40, True, idx=True, probe=True),
    ppo("ppo_n4_sh_f200_a2_invb", 4, 200, 2, 40, True, idx=True, inv_b_mul=0.5),
    ppo("ppo_n4_sh_f256_a2_probe", 4, 256, 2, 3, True, probe=True),
    ppo("ppo_n8_sh_f300_a5", 8, 300, 5, 40, True, act="tanh"),
    ppo("ppo_n8_sh_f512_a2_probe", 8, 512, 2, 40, True, probe=True),
    # ---- feature rows, separate trunks
    ppo("ppo_n1_sep_f64_a2", 1, 64, 2, 40, False, act="tanh"),
    ppo("ppo_n1_sep_f1_a2_probe", 1, 1, 2, 3, False, probe=True),
    ppo("ppo_n2_sep_f65_a5_idx", 2, 65, 5, 40, False, idx=True),
    ppo("ppo_n2_sep_f128_a2_probe", 2, 128, 2, 1, False, probe=True),
    ppo("ppo_n4_sep_f256_a8_b3", 4, 256, 8, 3, False, act="tanh"),
    ppo("ppo_n4_sep_f200_a2_probe", 4, 200, 2, 40, False, idx=True, probe=True),
    ppo("ppo_n8_sep_f512_a2", 8, 512, 2, 40, False, idx=True),
    ppo("ppo_n8_sep_f300_a2_probe", 8, 300, 2, 3, False, probe=True),
    # ---- split-K partial slabs, shared trunk
    ppo("ppo_n1_shp_f1_a1_k2", 1, 1, 1, 3, True, ks=2),
    ppo("ppo_n1_shp_f37_a2_k3_probe", 1, 37, 2, 40, True, ks=3, probe=True),
    ppo("ppo_n2_shp_f128_a2_k16", 2, 128, 2, 40, True, ks=16),
    ppo("ppo_n2_shp_f100_a1_k5_probe", 2, 100, 1, 3, True, ks=5, probe=True),
    ppo("ppo_n4_shp_f256_a5_k5", 4, 256, 5, 40, True, ks=5, idx=True),
    ppo("ppo_n4_shp_f200_a2_k16_probe", 4, 200, 2, 3, True, ks=16, probe=True),
    ppo("ppo_n8_shp_f512_a8_k3", 8, 512, 8, 40, True, ks=3),
    ppo("ppo_n8_shp_f300_a2_k2_probe", 8, 300, 2, 40, True, ks=2, idx=True, probe=True),
    # ---- split-K partial slabs, separate trunks (slab counts of the two trunks differ)
    ppo("ppo_n1_sepp_f64_a8_k3_5", 1, 64, 8, 40, False, ks=(3, 5), act="tanh"),
    ppo("ppo_n1_sepp_f37_a2_k2_probe", 1, 37, 2, 3, False, ks=2, probe=True),
    ppo("ppo_n2_sepp_f100_a1_k2_16", 2, 100, 1, 3, False, ks=(2, 16), act="tanh"),
    ppo("ppo_n2_sepp_f65_a2_k5_3_probe", 2, 65, 2, 40, False, ks=(5, 3), probe=True),
    ppo("ppo_n4_sepp_f200_a5_k1_3_b1", 4, 200, 5, 1, False, ks=(1, 3)),
    ppo("ppo_n4_sepp_f256_a2_k16_probe", 4, 256, 2, 3, False, ks=16, probe=True),
    ppo("ppo_n8_sepp_f300_a8_k16_2", 8, 300, 8, 40, False, ks=(16, 2), act="tanh", idx=True),
    ppo("ppo_n8_sepp_f512_a2_k3_1_probe", 8, 512, 2, 3, False, ks=(3, 1), probe=True),
]


def _ppo_cfg(c):
    """clip_ratio, ent_coef, vf_clip, critic_coef (a probe has no entropy term: d(logits) keeps the surrogate's signs)"""
    return PPO_CLIP, 0.0 if c.probe else PPO_ENT, PPO_VF_CLIP, PPO_CRITIC


def _log_softmax(x):
    return nets.softmax_stats(x)[1]


def ppo_data(c):
    """every input of the case as numpy arrays (float32 / int32, adv and target_v float64), from the case id alone"""
    rng = np.random.default_rng(zlib.crc32(c.id.encode()))
    B, F, A = c.B, c.F, c.A
    npool = B + POOL_EXTRA
    idx = rng.permutation(npool)[:B].astype(np.int32) if c.idx else None
    rows = idx if c.idx else np.arange(B)
    ntr = 1 if c.shared else 2
    d = dict(idx=idx, rows=rows, feat=[], parts=[], tbias=[], act_feat="none" if c.probe else c.act)
    col = (7 * np.arange(B) + 3) % F
    for t in range(ntr):
        ks = c.ks[t] if c.ks else 0
        if c.probe:
            x = np.zeros((B, F), np.float32)
            x[np.arange(B), col] = 1.0
            p = np.zeros((ks, B, F), np.float32)
            if ks:
                p[np.arange(B) % ks, np.arange(B), col] = 1.0
            tb = np.zeros(F, np.float32)
        elif ks:
            p = (rng.standard_normal((ks, B, F)) / np.sqrt(ks)).astype(np.float32)
            tb = (rng.standard_normal(F) * 0.1).astype(np.float32)
            x = None
        else:
            p, tb = np.zeros((0, B, F), np.float32), None
            x = nets.act_fwd(rng.standard_normal((B, F)), c.act).astype(np.float32)
        d["feat"].append(x)
        d["parts"].append(p)
        d["tbias"].append(tb)
    if c.probe:
        # distinct dyadic weights; the sign pattern makes every term of a probed d(features) entry point the same way
        # (see test_ppo_heads_fused_branch_vs_fp64), so its few fp32 roundings stay within 2 ulp of the result
        k = np.arange(F * A, dtype=np.float64).reshape(F, A)
        sign = np.where(np.arange(A)[None, :] == (np.arange(F) % A)[:, None], 1.0, -1.0)
        d["wpi"] = (sign * (k + 1) / 2048.0).astype(np.float32)
        d["bpi"] = ((np.arange(A) - 1) / 8.0).astype(np.float32)
        d["wv"] = ((np.arange(F) + 1) / 1024.0).astype(np.float32)
        d["bv"] = np.array([0.25], np.float32)
    else:
        d["wpi"] = (rng.standard_normal((F, A)) / np.sqrt(F)).astype(np.float32)
        d["bpi"] = (rng.standard_normal(A) * 0.1).astype(np.float32)
        d["wv"] = (rng.standard_normal(F) / np.sqrt(F)).astype(np.float32)
        d["bv"] = np.array([0.3], np.float32)
    feat64 = ppo_features(c, d)
    logits = feat64[0] @ d["wpi"].astype(np.float64) + d["bpi"]
    value = feat64[-1] @ d["wv"].astype(np.float64) + d["bv"][0]
    action = rng.integers(0, A, npool).astype(np.int32)
    old_logp = (-np.abs(rng.standard_normal(npool)) - 0.3).astype(np.float32)
    adv = rng.standard_normal(npool)
    old_v = rng.standard_normal(npool).astype(np.float32)
    target_v = rng.standard_normal(npool) * 4
    if c.probe:
        # action = the probed column's positive weight, advantage > 0, ratio ~ 1 (not clipped), old value = the value
        # exactly (so the clipped and the plain value error are the same number) and the target above it
        action[rows] = (col % A).astype(np.int32)
        logp = np.take_along_axis(_log_softmax(logits), action[rows].reshape(-1, 1).astype(np.int64), 1)[:, 0]
        old_logp[rows] = logp.astype(np.float32)
        adv[rows] = 0.5 + (np.arange(B) % 5) / 4.0
        old_v[rows] = d["wv"][col] + d["bv"][0]                     # (float32 sum, as the kernel forms it)
        target_v[rows] = old_v[rows].astype(np.float64) + 1.0 + (np.arange(B) % 7) / 8.0
    else:
        # old log-probability around the new one (ratio inside and on both sides of 1 +- clip), old / target value
        # spread over a few vf_clip around the value: all four gradient outcomes are populated
        logp = np.take_along_axis(_log_softmax(logits), action[rows].reshape(-1, 1).astype(np.int64), 1)[:, 0]
        old_logp[rows] = (logp + rng.uniform(-0.3, 0.3, B)).astype(np.float32)
        old_v[rows] = (value + rng.uniform(-3.0, 3.0, B) * PPO_VF_CLIP).astype(np.float32)
        target_v[rows] = value + rng.uniform(-4.0, 4.0, B) * PPO_VF_CLIP
    d.update(action=action, old_logp=old_logp, adv=adv, old_v=old_v, target_v=target_v)
    return d


def ppo_features(c, d):
    """float64 features of each trunk: the rows as they are, or act_feat(sum of the slabs + bias)"""
    out = []
    for t in range(len(d["feat"])):
        if c.ks:
            z = d["parts"][t].astype(np.float64).sum(0) + d["tbias"][t].astype(np.float64)
            out.append(nets.act_fwd(z, d["act_feat"]))
        else:
            out.append(d["feat"][t].astype(np.float64))
    return out


MARGIN = 1e-4


def ppo_reference(c, d):
    """float64 forward, loss gradients and per-sample terms, the population of the four gradient outcomes and the
    rows that sit within MARGIN (relative) of a branch boundary"""
    B = c.B
    clip, entc, vfc, cc = _ppo_cfg(c)
    feat = ppo_features(c, d)
    logits = feat[0] @ d["wpi"].astype(np.float64) + d["bpi"]
    value = (feat[-1] @ d["wv"].astype(np.float64) + d["bv"][0]).reshape(-1, 1)
    rows = d["rows"]
    col = lambda a: a[rows].astype(np.float64).reshape(-1, 1)
    action = d["action"][rows]
    old_logp, old_v = col(d["old_logp"]), col(d["old_v"])
    adv = col(d["adv"].astype(np.float32))                 # (the kernel reads the float64 pools as float32)
    tv = col(d["target_v"].astype(np.float32))
    _, dlg, dv, _ = nets.ppo_loss_and_grads(logits, value, action, old_logp, adv, old_v, tv, clip, entc, vfc, cc)
    dlg, dv = dlg * c.inv_b_mul, dv[:, 0] * c.inv_b_mul   # (the oracle divides by B)
    _, logp_all, ent = nets.softmax_stats(logits)
    logp = np.take_along_axis(logp_all, action.reshape(-1, 1).astype(np.int64), 1)
    ratio = np.exp(logp - old_logp)
    surr1, surr2 = ratio * adv, np.clip(ratio, 1 - clip, 1 + clip) * adv
    vf1 = np.square(value - tv)
    vf2 = np.square(old_v + np.clip(value - old_v, -vfc, vfc) - tv)
    terms = np.concatenate([np.minimum(surr1, surr2), ent, np.maximum(vf1, vf2)], 1)
    in_rng = (ratio >= 1 - clip) & (ratio <= 1 + clip)
    in_v = np.abs(value - old_v) <= vfc
    dsurr_zero = ~((surr1 <= surr2) | in_rng)
    dv_zero = ~(vf1 >= vf2) & ~in_v
    near = np.minimum(np.abs(ratio - (1 - clip)), np.abs(ratio - (1 + clip))) < MARGIN
    near |= ~in_rng & (np.abs(surr1 - surr2) < MARGIN * np.maximum(np.abs(surr1), np.abs(surr2)))
    near |= np.abs(np.abs(value - old_v) - vfc) < MARGIN * vfc
    near |= ~in_v & (np.abs(vf1 - vf2) < MARGIN * np.maximum(vf1, vf2))
    pops = dict(dsurr_adv=float((~dsurr_zero).mean()), dsurr_zero=float(dsurr_zero.mean()),
                dv_live=float((~dv_zero).mean()), dv_zero=float(dv_zero.mean()))
    return dict(feat=feat, logits=logits, value=value[:, 0], dlogits=dlg, dvalue=dv, terms=terms, keep=~near[:, 0],
                pops=pops)


# ---------------------------------------------------------------- IMPALA fused heads + v-trace: cases
ImpCase = collections.namedtuple("ImpCase", "id nq am T n_traj F A ks fwd act done probe")


def imp(id, nq, am, T, n_traj, F, A, ks=0, act="relu", done="random", probe=None):
    """nq: the forward instance expected (0: the forward launch is not run -- it holds A <= 8 -- and logits / baseline
    are inputs); am: the v-trace instance expected; ks: split-K partial slabs (PART) or 0; done: none / all / last /
    random; probe: None, "fwd" (one-hot feature rows, logits and baseline checked bit for bit) or "vtrace" (equal logits,
    every step terminal, dyadic values: vs, pg_adv and d(baseline) checked bit for bit)"""
    return ImpCase(id, nq, am, T, n_traj, F, A, ks, nq > 0, "relu" if probe == "fwd" else act, done, probe)


# T: the suffix scan runs in up to four waves (64 / 128 / 192 / 256 steps); d(features) in row blocks of 8; F >= 256: a
# second pass of the 256 threads over the feature columns.  ImpalaCnnOpt: F = 256, T = 128, split-K slabs.
IMPALA_CASES = [
    imp("imp_n1_f5_t2_a1", 1, 8, 2, 1, 5, 1, done="none"),
    imp("imp_n1_f64_t9_a3_probe", 1, 8, 9, 3, 64, 3, probe="fwd"),
    imp("imp_n1p_f64_t63_a8_k2", 1, 8, 63, 3, 64, 8, ks=2, act="tanh", done="last"),
    imp("imp_n1p_f5_t8_a3_k16_probe", 1, 8, 8, 1, 5, 3, ks=16, probe="fwd"),
    imp("imp_n2_f100_t64_a3", 2, 8, 64, 1, 100, 3),
    imp("imp_n2_f100_t65_a8_probe", 2, 8, 65, 3, 100, 8, probe="fwd", done="all"),
    imp("imp_n2p_f100_t65_a1_k16", 2, 8, 65, 1, 100, 1, ks=16, done="all"),
    imp("imp_n2p_f128_t9_a3_k2_probe", 2, 8, 9, 1, 128, 3, ks=2, probe="fwd"),
    imp("imp_n4_f256_t128_a8", 4, 8, 128, 3, 256, 8, act="tanh"),
    imp("imp_n4_f200_t129_a3_probe", 4, 8, 129, 1, 200, 3, probe="fwd"),
    imp("imp_n4p_f256_t129_a3_k2", 4, 8, 129, 3, 256, 3, ks=2),
    imp("imp_n4p_f256_t128_a8_k16_probe", 4, 8, 128, 1, 256, 8, ks=16, probe="fwd", done="last"),
    imp("imp_n8_f300_t193_a8", 8, 8, 193, 1, 300, 8, done="none"),
    imp("imp_n8_f512_t8_a1_probe", 8, 8, 8, 3, 512, 1, probe="fwd"),
    imp("imp_n8p_f512_t256_a3_k2", 8, 8, 256, 1, 512, 3, ks=2, act="tanh"),
    imp("imp_n8p_f300_t63_a8_k16_probe", 8, 8, 63, 1, 300, 8, ks=16, probe="fwd"),
    # ---- the v-trace launch alone on given logits: A <= 8 once more, then the 32-action instance
    imp("vt_am8_f64_t256_a8_probe", 0, 8, 256, 3, 64, 8, probe="vtrace"),
    imp("vt_am32_f5_t9_a9", 0, 32, 9, 3, 5, 9, done="last"),
    imp("vt_am32_f300_t65_a18", 0, 32, 65, 1, 300, 18, act="tanh"),
    imp("vt_am32_f256_t256_a32", 0, 32, 256, 3, 256, 32, done="none"),
    imp("vt_am32_f100_t193_a32", 0, 32, 193, 1, 100, 32),
    imp("vt_am32_f64_t129_a9_probe", 0, 32, 129, 3, 64, 9, probe="vtrace"),
    imp("vt_am32_f512_t2_a18_probe", 0, 32, 2, 1, 512, 18, probe="vtrace"),
]
GAMMA = 0.99


def imp_data(c):
    rng = np.random.default_rng(zlib.crc32(c.id.encode()))
    T, F, A = c.T, c.F, c.A
    n = T * c.n_traj
    d = dict(act_feat="none" if c.probe == "fwd" else c.act)
    col = (7 * np.arange(n) + 3) % F
    if c.probe == "fwd":
        x = np.zeros((n, F), np.float32)
        x[np.arange(n), col] = 1.0
        p = np.zeros((c.ks, n, F), np.float32)
        if c.ks:
            p[np.arange(n) % c.ks, np.arange(n), col] = 1.0
        tb = np.zeros(F, np.float32)
        k = np.arange(F * A, dtype=np.float64).reshape(F, A)
        wpi = (np.where((k.astype(np.int64) % 3) == 0, -1.0, 1.0) * (k + 1) / 4096.0).astype(np.float32)
        bpi = ((np.arange(A) - 1) / 8.0).astype(np.float32)
        wv = ((np.arange(F) - F // 2 + 0.5) / 1024.0).astype(np.float32)
        bv = np.array([0.25], np.float32)
    else:
        if c.ks:
            p = (rng.standard_normal((c.ks, n, F)) / np.sqrt(c.ks)).astype(np.float32)
            tb = (rng.standard_normal(F) * 0.1).astype(np.float32)
            x = None
        else:
            p, tb = np.zeros((0, n, F), np.float32), None
            x = nets.act_fwd(rng.standard_normal((n, F)), c.act).astype(np.float32)
        wpi = (rng.standard_normal((F, A)) / np.sqrt(F)).astype(np.float32)
        bpi = (rng.standard_normal(A) * 0.1).astype(np.float32)
        wv = (rng.standard_normal(F) / np.sqrt(F)).astype(np.float32)
        bv = np.array([0.3], np.float32)
    d.update(feat=x, parts=p, tbias=tb, wpi=wpi, bpi=bpi, wv=wv, bv=bv)
    d["bp"] = rng.standard_normal((n, A)).astype(np.float32)
    d["action"] = rng.integers(0, A, n).astype(np.int32)
    d["reward"] = (rng.standard_normal(n) * 2).astype(np.float32)          # (beyond +-1: the kernel clips)
    done = np.zeros((c.n_traj, T), bool)
    if c.done == "all":
        done[:] = True
    elif c.done == "last":
        done[:, T - 2] = True                                                 # (step T-1 is the bootstrap only)
    elif c.done == "random":
        done = rng.random((c.n_traj, T)) < 0.1
    d["done"] = done.reshape(-1)
    if not c.fwd:
        d["logits"] = rng.standard_normal((n, A)).astype(np.float32)
        d["baseline"] = rng.standard_normal(n).astype(np.float32)
    if c.probe == "vtrace":
        d["logits"] = np.zeros((n, A), np.float32)
        d["bp"] = np.zeros((n, A), np.float32)
        d["done"] = np.ones(n, bool)
        d["baseline"] = (((7 * np.arange(n) + 3) % 33 - 16) / 8.0).astype(np.float32)
        d["reward"] = rng.choice(np.array([-2.0, -1.0, -0.5, 0.0, 0.5, 1.0, 2.0], np.float32), n)
    return d


def imp_features(c, d):
    if c.ks:
        return nets.act_fwd(d["parts"].astype(np.float64).sum(0) + d["tbias"].astype(np.float64), d["act_feat"])
    return d["feat"].astype(np.float64)


def imp_reference(c, d):
    feat = imp_features(c, d)
    if c.fwd:
        logits = feat @ d["wpi"].astype(np.float64) + d["bpi"]
        baseline = feat @ d["wv"].astype(np.float64) + d["bv"][0]
    else:
        logits, baseline = d["logits"].astype(np.float64), d["baseline"].astype(np.float64)
    T = c.T
    out = dict(feat=feat, logits=logits, baseline=baseline, traj_loss=[], dlogits=[], dbaseline=[], vs=[], pg=[])
    for i in range(c.n_traj):                     # (per trajectory: the kernel leaves one loss sum for each)
        s = slice(i * T, (i + 1) * T)
        loss, dlg, dbl, parts = nets.impala_loss_and_grads(logits[s], baseline[s], d["bp"][s], d["action"][s], d["done"][s],
                                                           d["reward"][s], T, GAMMA)
        out["traj_loss"].append(float(loss))
        out["dlogits"].append(dlg)
        out["dbaseline"].append(dbl)
        out["vs"].append(parts["vs"][:, 0])
        out["pg"].append(parts["pg_adv"][:, 0])
    for k in ("dlogits", "dbaseline"):
        out[k] = np.concatenate(out[k], 0)
    for k in ("vs", "pg"):
        out[k] = np.stack(out[k], 0)
    out["traj_loss"] = np.array(out["traj_loss"])
    return out


# ---------------------------------------------------------------- head weight-gradient slabs: cases
WgCase = collections.namedtuple("WgCase", "id B F A shared probe")
WG_CASES = [
    WgCase("wg_b1_f1_a1", 1, 1, 1, True, False),
    WgCase("wg_b7_f63_a7_sep", 7, 63, 7, False, False),
    WgCase("wg_b8_f64_a8", 8, 64, 8, True, False),
    WgCase("wg_b9_f65_a9_sep", 9, 65, 9, False, False),
    WgCase("wg_b40_f200_a18", 40, 200, 18, True, False),
    WgCase("wg_b40_f200_a8_sep", 40, 200, 8, False, False),
    WgCase("wg_b9_f64_a1_sep", 9, 64, 1, False, False),
    WgCase("wg_b40_f65_a9_probe", 40, 65, 9, True, True),
    WgCase("wg_b7_f200_a8_sep_probe", 7, 200, 8, False, True),
]
WG_PAD = (3, 5)          # floats between the slabs of the policy / value buffers (must stay untouched)


def wg_data(c):
    rng = np.random.default_rng(zlib.crc32(c.id.encode()))
    f_pi = rng.standard_normal((c.B, c.F)).astype(np.float32)
    f_v = f_pi if c.shared else rng.standard_normal((c.B, c.F)).astype(np.float32)
    if c.probe:
        dl = np.zeros((c.B, c.A), np.float32)
        dl[c.B - 2, c.A - 1] = -1.5
        dv = np.zeros(c.B, np.float32)
    else:
        dl = rng.standard_normal((c.B, c.A)).astype(np.float32)
        dv = rng.standard_normal(c.B).astype(np.float32)
    return f_pi, f_v, dl, dv


# ---------------------------------------------------------------- GPU
SENTINEL = np.float32(-1.2345e37)
TAIL = 64
_KEEP = []


@pytest.fixture(scope="module")
def L():
    from xingtian_amd import lib
    lib.require_gpu()
    lib.load()
    return lib


@pytest.fixture(autouse=True)
def _keepalive():
    _KEEP.clear()
    yield
    torch.cuda.synchronize()
    _KEEP.clear()


def dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    _KEEP.append(t)
    return t


def in_buf(a):
    """a float input followed by TAIL NaNs: a lane that read past the end and used the value shows up"""
    a = np.ascontiguousarray(a)
    t = torch.full((a.size + TAIL,), float("nan"), dtype=torch.from_numpy(a.ravel()[:0]).dtype, device="cuda")
    t[:a.size] = torch.from_numpy(a.ravel()).cuda()
    _KEEP.append(t)
    return t


def out_buf(n, fill=float("nan")):
    """n floats prefilled with `fill`, followed by TAIL sentinel floats"""
    t = torch.full((n + TAIL,), fill, dtype=torch.float32, device="cuda")
    t[n:] = float(SENTINEL)
    _KEEP.append(t)
    return t


def split_out(t, n, what):
    a = t.cpu().numpy()
    assert (a[n:].view(np.uint32) == np.full(TAIL, SENTINEL).view(np.uint32)).all(), "store past the end of " + what
    return a[:n]


def rel_err(got, ref):
    return np.linalg.norm((np.asarray(got, np.float64) - ref).ravel()) / (np.linalg.norm(np.asarray(ref).ravel()) + 1e-30)


def assert_probe(got, ref, what):
    """every entry within 2 fp32 ulp of the float64 reference; entries whose reference is 0 exactly 0"""
    ref32 = np.abs(ref).astype(np.float32)
    tol = 2.0 * np.spacing(ref32).astype(np.float64)
    tol[ref == 0] = 0.0
    bad = np.abs(got.astype(np.float64) - ref) > tol
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    assert (ref != 0).any(), what        # (the probe reached something)


def same_bits(got, want, what):
    want = np.asarray(want, np.float32)
    assert got.shape == want.shape and (got.view(np.uint32) == want.view(np.uint32)).all(), what


def check_bars(tag, errs):
    """print every measured error next to its bar, then assert them"""
    print(tag, " ".join("{} {:.2e}/{:.0e}".format(k, e, bar) for k, (e, bar) in errs.items()))
    for k, (e, bar) in errs.items():
        assert e < bar, (tag, k, e, bar)


def dfeat_reference(dl, dv, wpi, wv, feat_pi, feat_v, act, shared):
    """float64 d(features) from GIVEN head gradients (the kernel's own: this isolates the product)"""
    dpi = dl.astype(np.float64) @ wpi.astype(np.float64).T
    dvf = dv.astype(np.float64).reshape(-1, 1) * wv.astype(np.float64).reshape(1, -1)
    if shared:
        return nets.act_bwd(dpi + dvf, feat_pi.astype(np.float64), act), None
    return nets.act_bwd(dpi, feat_pi.astype(np.float64), act), nets.act_bwd(dvf, feat_v.astype(np.float64), act)


def call_ppo(L, c, d, o):
    """one xt_ppo_heads_fused_ex call on the case's data and the output buffers `o` -> (rc, path)"""
    B, F, A = c.B, c.F, c.A
    clip, entc, vfc, cc = _ppo_cfg(c)
    cfg = L.PpoCfg()
    cfg.clip_ratio, cfg.ent_coef, cfg.vf_clip, cfg.critic_coef = clip, entc, vfc, cc
    sep = not c.shared
    p = lambda a: L.ptr(in_buf(a))
    if c.ks:
        stride = B * F
        f_pi = f_v = None
        part_pi, tb_pi = p(d["parts"][0]), p(d["tbias"][0])
        part_v, tb_v = (p(d["parts"][1]), p(d["tbias"][1])) if sep else (None, None)
        ks_pi, ks_v = c.ks[0], c.ks[1]
    else:
        stride, part_pi, part_v, tb_pi, tb_v, ks_pi, ks_v = 0, None, None, None, None, 1, 1
        f_pi = p(d["feat"][0])
        f_v = p(d["feat"][1]) if sep else None
    path = ctypes.c_int32(-1)
    rc = L.load().xt_ppo_heads_fused_ex(
        f_pi, f_v, part_pi, part_v, ks_pi, ks_v, stride, tb_pi, tb_v, L.ACT[d["act_feat"]], B, F, A, 1 if c.shared else 0,
        p(d["wpi"]), p(d["bpi"]), p(d["wv"]), p(d["bv"]), L.ptr(dev(d["idx"])) if c.idx else None, L.ptr(dev(d["action"])),
        p(d["old_logp"]), p(d["adv"]), p(d["old_v"]), p(d["target_v"]), ctypes.byref(cfg), c.inv_b_mul / B, L.ACT[c.act],
        L.ptr(o["logits"]), L.ptr(o["value"]), L.ptr(o["dlogits"]), L.ptr(o["dvalue"]), L.ptr(o["terms"]),
        L.ptr(o["df_pi"]), L.ptr(o["df_v"]) if sep else None, L.ptr(o["feat_pi"]) if c.ks else None,
        L.ptr(o["feat_v"]) if c.ks and sep else None, None, ctypes.byref(path))
    torch.cuda.synchronize()
    return rc, path.value


def ppo_outputs(c):
    B, F, A = c.B, c.F, c.A
    return dict(logits=out_buf(B * A), value=out_buf(B), dlogits=out_buf(B * A), dvalue=out_buf(B), terms=out_buf(B * 4),
                df_pi=out_buf(B * F), df_v=out_buf(B * F), feat_pi=out_buf(B * F), feat_v=out_buf(B * F))


@pytest.mark.parametrize("c", PPO_CASES, ids=[c.id for c in PPO_CASES])
def test_ppo_heads_fused_branch_vs_fp64(L, c):
    B, F, A = c.B, c.F, c.A
    d = ppo_data(c)
    ref = ppo_reference(c, d)
    o = ppo_outputs(c)
    rc, path = call_ppo(L, c, d, o)
    L.check(rc, "xt_ppo_heads_fused_ex " + c.id)
    assert decode_head_path(path) == (head_paths()["PPO_FUSED"], c.nq, 1 if c.ks else 0, 1 if c.shared else 0, 0), \
        (c.id, decode_head_path(path))
    got = {k: split_out(o[k], n, k) for k, n in (("logits", B * A), ("value", B), ("dlogits", B * A), ("dvalue", B),
                                                   ("terms", B * 4), ("df_pi", B * F), ("df_v", B * F),
                                                   ("feat_pi", B * F), ("feat_v", B * F))}
    check_ppo(c, d, ref, got)


def check_ppo(c, d, ref, got):
    """the outputs of one case (flat float32 arrays, NaN where nothing was written) against the float64 reference"""
    B, F, A = c.B, c.F, c.A
    sep = not c.shared
    written = ["logits", "value", "dlogits", "dvalue", "terms", "df_pi"] + (["df_v"] if sep else []) + \
        ((["feat_pi"] + (["feat_v"] if sep else [])) if c.ks else [])
    for k in got:        # everything the instance writes is written, the rest is untouched
        assert np.isfinite(got[k]).all() if k in written else np.isnan(got[k]).all(), (c.id, k)
    logits, dl = got["logits"].reshape(B, A), got["dlogits"].reshape(B, A)
    terms = got["terms"].reshape(B, 4)
    assert (terms[:, 3] == 0).all()
    # the features the kernel used: its own finished ones (checked below), or the input rows
    kfeat = [got["feat_pi"].reshape(B, F), got["feat_v"].reshape(B, F)][:2 if sep else 1] if c.ks else d["feat"]
    ref_dpi, ref_dv = dfeat_reference(dl, got["dvalue"], d["wpi"], d["wv"], kfeat[0], kfeat[-1], c.act, c.shared)
    if c.probe:
        col = (7 * np.arange(B) + 3) % F
        same_bits(logits, d["wpi"][col] + d["bpi"][None, :], "logits")           # (float32 sums)
        same_bits(got["value"], d["wv"][col] + d["bv"][0], "value")
        if c.ks:
            for t, k in enumerate(["feat_pi", "feat_v"][:2 if sep else 1]):
                same_bits(got[k].reshape(B, F), ref["feat"][t], k)
        # d(features): zero off the probed column (relu), there (A <= 2) two or three products of one sign: the
        # advantage is positive, so d(logit of the action) < 0 < d(other logit), the weights carry the opposite signs
        # and d(value) < 0 meets a positive value weight -- no cancellation, at most four roundings of 1/2 ulp
        assert_probe(got["df_pi"].reshape(B, F), ref_dpi, "df_pi")
        if sep:
            assert_probe(got["df_v"].reshape(B, F), ref_dv, "df_v")
    keep = ref["keep"]
    assert np.isfinite(dl).all() and np.isfinite(got["dvalue"]).all()
    # (2 % of at most 40 rows is less than one row: in effect NO row of a case may sit within MARGIN of a branch
    # boundary.  The data come from the case id alone and tests/test_cpu_heads_coverage.py checks this on the CPU; a
    # case that lands a row on a boundary gets another id (seed), never a wider margin or cap.)
    assert keep.any() and (~keep).sum() <= 0.02 * B, (c.id, int((~keep).sum()))
    errs = {"logits": (rel_err(logits, ref["logits"]), 2e-6), "value": (rel_err(got["value"], ref["value"]), 2e-6),
            "dlogits": (rel_err(dl[keep], ref["dlogits"][keep]), 1e-5),
            "dvalue": (rel_err(got["dvalue"][keep], ref["dvalue"][keep]), 1e-5),
            "df_pi": (rel_err(got["df_pi"].reshape(B, F), ref_dpi), 3e-6)}
    if sep:
        errs["df_v"] = (rel_err(got["df_v"].reshape(B, F), ref_dv), 3e-6)
    if c.ks:
        errs["feat_pi"] = (rel_err(got["feat_pi"].reshape(B, F), ref["feat"][0]), 2e-6)
        if sep:
            errs["feat_v"] = (rel_err(got["feat_v"].reshape(B, F), ref["feat"][1]), 2e-6)
    for j, k in enumerate(("surr", "ent", "vf")):
        errs["terms." + k] = (rel_err(terms[:, j], ref["terms"][:, j]), 1e-5)
    check_bars("ppo_heads {} nq {} part {} shared {} excluded {}".format(c.id, c.nq, int(bool(c.ks)), int(c.shared),
                                                                        int((~keep).sum())), errs)


def call_impala(L, c, d, o):
    T, F, A = c.T, c.F, c.A
    n = T * c.n_traj
    p = lambda a: L.ptr(in_buf(a))
    if c.fwd:
        logits, baseline = o["logits"], o["baseline"]
    else:
        logits, baseline = in_buf(d["logits"]), in_buf(d["baseline"])
    path = ctypes.c_int32(-1)
    rc = L.load().xt_impala_heads_ex(
        None if c.ks else p(d["feat"]), p(d["parts"]) if c.ks else None, c.ks if c.ks else 1, n * F if c.ks else 0,
        p(d["tbias"]) if c.ks else None, L.ACT[d["act_feat"]], 1 if c.fwd else 0, c.n_traj, T, F, A, p(d["wpi"]), p(d["bpi"]),
        p(d["wv"]), p(d["bv"]), p(d["bp"]), L.ptr(dev(d["action"])), L.ptr(dev(d["done"].astype(np.uint8))), p(d["reward"]),
        GAMMA, L.ACT[c.act], L.ptr(o["feat_w"]) if c.ks else None, L.ptr(logits), L.ptr(baseline), L.ptr(o["dlogits"]),
        L.ptr(o["dbaseline"]), L.ptr(o["vs"]), L.ptr(o["pg"]), L.ptr(o["dfeat"]), L.ptr(o["traj_loss"]), L.ptr(o["loss"]),
        None, ctypes.byref(path))
    torch.cuda.synchronize()
    return rc, path.value


def imp_outputs(c):
    n, F, A = c.T * c.n_traj, c.F, c.A
    nm = (c.T - 1) * c.n_traj
    return dict(logits=out_buf(n * A), baseline=out_buf(n), dlogits=out_buf(n * A), dbaseline=out_buf(n), vs=out_buf(nm),
                pg=out_buf(nm), dfeat=out_buf(n * F), feat_w=out_buf(n * F), traj_loss=out_buf(c.n_traj), loss=out_buf(1))


@pytest.mark.parametrize("c", IMPALA_CASES, ids=[c.id for c in IMPALA_CASES])
def test_impala_heads_vtrace_branch_vs_fp64(L, c):
    T, F, A = c.T, c.F, c.A
    n, nm = T * c.n_traj, (T - 1) * c.n_traj
    d = imp_data(c)
    ref = imp_reference(c, d)
    o = imp_outputs(c)
    rc, path = call_impala(L, c, d, o)
    L.check(rc, "xt_impala_heads_ex " + c.id)
    assert decode_head_path(path) == (head_paths()["IMPALA"], c.nq, 1 if c.ks else 0, 0, c.am), (c.id, decode_head_path(path))
    sizes = dict(logits=n * A, baseline=n, dlogits=n * A, dbaseline=n, vs=nm, pg=nm, dfeat=n * F, feat_w=n * F,
                 traj_loss=c.n_traj, loss=1)
    got = {k: split_out(o[k], sz, k) for k, sz in sizes.items()}
    check_impala(c, d, ref, got)


def check_impala(c, d, ref, got):
    """the outputs of one case (flat float32 arrays, NaN where nothing was written) against the float64 reference"""
    T, F, A = c.T, c.F, c.A
    n = T * c.n_traj
    untouched = ([] if c.fwd else ["logits", "baseline"]) + ([] if c.ks else ["feat_w"])
    for k in got:        # every row block's d(features) is written, the ragged last one included
        assert np.isnan(got[k]).all() if k in untouched else np.isfinite(got[k]).all(), (c.id, k)
    dl = got["dlogits"].reshape(c.n_traj, T, A)
    db = got["dbaseline"].reshape(c.n_traj, T)
    assert (dl[:, -1].view(np.uint32) == 0).all() and (db[:, -1].view(np.uint32) == 0).all()      # the bootstrap row: +0.0
    kfeat = got["feat_w"].reshape(n, F) if c.ks else d["feat"]
    ref_df, _ = dfeat_reference(dl.reshape(n, A), db.reshape(n), d["wpi"], d["wv"], kfeat, kfeat, c.act, True)
    errs = {}
    if c.fwd:
        errs["logits"] = (rel_err(got["logits"].reshape(n, A), ref["logits"]), 2e-6)
        errs["baseline"] = (rel_err(got["baseline"], ref["baseline"]), 2e-6)
    if c.ks:
        errs["feat"] = (rel_err(got["feat_w"].reshape(n, F), ref["feat"]), 2e-6)
    if c.probe == "fwd":
        col = (7 * np.arange(n) + 3) % F
        same_bits(got["logits"].reshape(n, A), d["wpi"][col] + d["bpi"][None, :], "logits")
        same_bits(got["baseline"], d["wv"][col] + d["bv"][0], "baseline")
        if c.ks:
            same_bits(got["feat_w"].reshape(n, F), ref["feat"], "finished features")
    if c.probe == "vtrace":
        # equal logits on both sides: rho = exp(0) = 1; every step terminal: vs = (r - V) + V, pg_adv = r - V, all dyadic
        r = np.clip(d["reward"], -1, 1).reshape(c.n_traj, T)[:, :-1]
        v = d["baseline"].reshape(c.n_traj, T)[:, :-1]
        same_bits(got["vs"].reshape(c.n_traj, T - 1), r, "vs")
        same_bits(got["pg"].reshape(c.n_traj, T - 1), r - v, "pg_adv")
        same_bits(db[:, :-1], 0.5 * (v - r), "dbaseline")
    loss = ref["traj_loss"].sum()
    errs.update({"vs": (rel_err(got["vs"].reshape(c.n_traj, T - 1), ref["vs"]), 1e-5),
                 "pg_adv": (rel_err(got["pg"].reshape(c.n_traj, T - 1), ref["pg"]), 1e-5),
                 "dlogits": (rel_err(dl.reshape(n, A), ref["dlogits"]), 1e-5),
                 "dbaseline": (rel_err(db.reshape(n), ref["dbaseline"]), 1e-5),
                 "dfeat": (rel_err(got["dfeat"].reshape(n, F), ref_df), 3e-6),
                 "loss": (abs(got["loss"][0] - loss) / max(1.0, abs(loss)), 2e-5),
                 "traj_loss": (np.max(np.abs(got["traj_loss"] - ref["traj_loss"]) / np.maximum(1.0, np.abs(ref["traj_loss"]))),
                               2e-5)})
    check_bars("impala_heads {} nq {} part {} am {}".format(c.id, c.nq, int(bool(c.ks)), c.am), errs)


@pytest.mark.parametrize("c", WG_CASES, ids=[c.id for c in WG_CASES])
def test_heads_wgrad_partial_slabs_vs_fp64(L, c):
    B, F, A = c.B, c.F, c.A
    f_pi, f_v, dl, dv = wg_data(c)
    want_chunks = cdiv(B, 8)
    st_pi, st_v = F * A + A + WG_PAD[0], F + 1 + WG_PAD[1]
    slab_pi, slab_v = out_buf(want_chunks * st_pi), out_buf(want_chunks * st_v)
    d_fpi = in_buf(f_pi)
    d_fv = d_fpi if c.shared else in_buf(f_v)
    nchunk = ctypes.c_int32(-1)
    L.check(L.load().xt_heads_wgrad_partial_ex(L.ptr(d_fpi), L.ptr(d_fv), B, F, A, L.ptr(in_buf(dl)), L.ptr(in_buf(dv)),
                                               L.ptr(slab_pi), st_pi, L.ptr(slab_v), st_v, ctypes.byref(nchunk), None),
            "xt_heads_wgrad_partial_ex " + c.id)
    torch.cuda.synchronize()
    assert nchunk.value == want_chunks
    check_wg(c, f_pi, f_v, dl, dv, split_out(slab_pi, want_chunks * st_pi, "slab_pi").reshape(want_chunks, st_pi),
             split_out(slab_v, want_chunks * st_v, "slab_v").reshape(want_chunks, st_v))


def check_wg(c, f_pi, f_v, dl, dv, spi, sv):
    """the slab buffers of one case ([chunk, stride], NaN where nothing was written) against float64"""
    B, F, A = c.B, c.F, c.A
    want_chunks = cdiv(B, 8)
    assert np.isnan(spi[:, F * A + A:]).all() and np.isnan(sv[:, F + 1:]).all(), "store between the slabs"
    spi, sv = spi[:, :F * A + A], sv[:, :F + 1]
    assert np.isfinite(spi).all() and np.isfinite(sv).all()
    if c.probe:                # one product per slab entry: exact
        b0, a0 = B - 2, A - 1
        want = np.zeros((want_chunks, F, A), np.float32)
        want[b0 // 8, :, a0] = f_pi[b0] * np.float32(-1.5)
        wb = np.zeros((want_chunks, A), np.float32)
        wb[b0 // 8, a0] = -1.5
        assert np.array_equal(spi[:, :F * A].reshape(want_chunks, F, A), want)
        assert np.array_equal(spi[:, F * A:], wb) and (sv == 0).all()
        return
    x64, xv64, dl64, dv64 = (a.astype(np.float64) for a in (f_pi, f_v, dl, dv))
    s_pi, s_v = spi.astype(np.float64).sum(0), sv.astype(np.float64).sum(0)
    # every slab holds its own chunk of 8 samples and nothing else
    for ch in range(want_chunks):
        r = slice(ch * 8, min(B, ch * 8 + 8))
        assert rel_err(spi[ch, :F * A].reshape(F, A), x64[r].T @ dl64[r]) < 3e-6, (c.id, ch)
    check_bars("heads_wgrad {} chunks {}".format(c.id, want_chunks),
               {"dWpi": (rel_err(s_pi[:F * A].reshape(F, A), x64.T @ dl64), 3e-6),
                "dbpi": (rel_err(s_pi[F * A:], dl64.sum(0)), 3e-6),
                "dWv": (rel_err(s_v[:F], xv64.T @ dv64), 3e-6),
                "dbv": (rel_err(s_v[F:], dv64.sum(keepdims=True)), 3e-6)})


def test_refused_geometries_launch_nothing(L):
    """on real buffers: a refused call returns non-zero, reports no path and leaves every output as it was"""
    c = ppo("refused_a9", 1, 64, 9, 3, True)
    o = ppo_outputs(c)
    rc, path = call_ppo(L, c, ppo_data(c), o)
    assert rc != 0 and path == 0 and "A=9 F=64" in L.load().xt_last_error().decode()
    c = ppo("refused_k17", 1, 64, 2, 3, False, ks=(2, 17))
    o2 = ppo_outputs(c)
    rc, path = call_ppo(L, c, ppo_data(c), o2)
    assert rc != 0 and path == 0 and "ksplit=2/17" in L.load().xt_last_error().decode()
    for bufs in (o, o2):
        for k, t in bufs.items():
            assert np.isnan(split_out(t, t.numel() - TAIL, k)).all(), k
    for c, msg in ((imp("refused_fwd_a9", 1, 32, 9, 1, 64, 9), "A=9 F=64"), (imp("refused_f513", 8, 8, 9, 1, 513, 3), "F=513")):
        o = imp_outputs(c)
        rc, path = call_impala(L, c, imp_data(c), o)
        assert rc != 0 and path == 0 and msg in L.load().xt_last_error().decode()
        for k, t in o.items():
            assert np.isnan(split_out(t, t.numel() - TAIL, k)).all(), k
