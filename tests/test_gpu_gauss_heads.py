"""GPU parity tests (run with -m gpu on an MI355X) of ppo_gauss_heads_fused_kernel<NQ, PART, SHARED, STATS>, the fused
head launch of a DiagGaussian PPO step (xt_net_set_gauss_fused), called on its own through xt_ppo_gauss_heads_fused_ex.
Every row of GAUSS_CASES names the instance it must take (XT_HEAD_PATH_PPO_GAUSS_FUSED and the NQ / PART / SHARED
fields), so a case that drifts onto another instance fails instead of passing there.  Reference:
oracle.nets.gauss_ppo_loss_and_grads in float64 on the same float32 inputs.  Output buffers are NaN-prefilled and end in a
sentinel tail; float inputs end in a NaN tail; what an instance does not write must stay NaN.

The data and the float64 reference of every case are plain numpy (gauss_data / gauss_reference):
tests/test_cpu_gauss_heads_coverage.py imports this module on the CPU, checks that every instance has a case and re-runs
the references to check the gradient-branch populations and the boundary exclusions.  The helpers come from
tests/test_gpu_heads_branch.py."""
import collections
import ctypes
import os
import re
import zlib

import numpy as np
import pytest
import torch

import test_gpu_heads_branch as HB
from oracle import nets
from test_gpu_heads_branch import L, _keepalive  # noqa: F401  (fixtures: the loaded library, the buffers' lifetime)
from test_gpu_heads_branch import check_bars, decode_head_path, dfeat_reference, in_buf, out_buf, rel_err, split_out

pytestmark = pytest.mark.gpu

GaussCase = collections.namedtuple("GaussCase", "id nq F A B shared ks act idx inv_b_mul stats")
CLIP, ENT, VF_CLIP, CRITIC = 0.1, 0.003, 0.5, 0.7
POOL_EXTRA = HB.POOL_EXTRA      # the label pools hold B + 13 rows
MARGIN = 1e-4


def gauss_family():
    """XT_HEAD_PATH_PPO_GAUSS_FUSED of include/xt_mi355x.h (written in parentheses there: the plain-integer XT_HEAD_PATH_*
    macros are the families of test_gpu_heads_branch.py's tables)"""
    with open(os.path.join(HB.ROOT, "include", "xt_mi355x.h")) as f:
        m = re.search(r"#define\s+XT_HEAD_PATH_PPO_GAUSS_FUSED\s+\(?(\d+)\)?", f.read())
    assert m, "include/xt_mi355x.h does not define XT_HEAD_PATH_PPO_GAUSS_FUSED"
    return int(m.group(1))


def gauss(id, nq, F, A, B, shared, ks=None, act="relu", idx=False, inv_b_mul=1.0, stats=False):
    """nq: the expected features-per-lane instance; ks: None = feature rows, an int or a (policy, value) pair = that many
    split-K partial slabs (PART); act: the trunk's activation (act_prev, and act_feat of the PART finish); idx: labels
    gathered through a permutation slice of a larger pool; inv_b_mul: inv_b = inv_b_mul / B; stats: the call passes the
    `rows` pointer (STATS instance) and the diagnostic row is checked"""
    if ks is not None and not isinstance(ks, tuple):
        ks = (ks, ks)
    return GaussCase(id, nq, F, A, B, shared, ks, act, idx, inv_b_mul, stats)


# F: 1 / 37 / 64 -> NQ 1, 65 / 100 / 128 -> NQ 2, 200 / 256 -> NQ 4, 300 / 512 -> NQ 8 (PpoMlp: F = 64, PpoCnn: 256 / 512)
GAUSS_CASES = [
    # ---- feature rows, shared trunk
    gauss("gauss_n1_sh_f37_a3_b40", 1, 37, 3, 40, True, idx=True),
    gauss("gauss_n2_sh_f100_a8_b40", 2, 100, 8, 40, True, act="tanh"),
    gauss("gauss_n4_sh_f200_a1_b40_invb", 4, 200, 1, 40, True, idx=True, inv_b_mul=0.5),
    gauss("gauss_n8_sh_f300_a6_b40_stats", 8, 300, 6, 40, True, act="tanh", stats=True),
    # ---- feature rows, separate trunks
    gauss("gauss_n1_sep_f64_a1_b40", 1, 64, 1, 40, False, act="tanh"),
    gauss("gauss_n2_sep_f65_a6_b40", 2, 65, 6, 40, False, idx=True),
    gauss("gauss_n4_sep_f256_a8_b3", 4, 256, 8, 3, False, act="tanh"),
    gauss("gauss_n8_sep_f512_a3_b40", 8, 512, 3, 40, False, idx=True),
    # ---- split-K partial slabs, shared trunk
    gauss("gauss_n1_shp_f1_a1_b3_k2", 1, 1, 1, 3, True, ks=2),
    gauss("gauss_n2_shp_f128_a3_b40_k16", 2, 128, 3, 40, True, ks=16),
    gauss("gauss_n4_shp_f256_a6_b40_k5_stats", 4, 256, 6, 40, True, ks=5, idx=True, stats=True),
    gauss("gauss_n8_shp_f512_a8_b40_k3", 8, 512, 8, 40, True, ks=3, act="tanh"),
    # ---- split-K partial slabs, separate trunks (slab counts of the two trunks differ)
    gauss("gauss_n1_sepp_f64_a8_b40_k3_5", 1, 64, 8, 40, False, ks=(3, 5), act="tanh"),
    gauss("gauss_n2_sepp_f100_a1_b3_k2_16", 2, 100, 1, 3, False, ks=(2, 16), act="tanh"),
    gauss("gauss_n4_sepp_f200_a6_b1_k5_3", 4, 200, 6, 1, False, ks=(5, 3)),
    gauss("gauss_n8_sepp_f300_a3_b40_k16_2_stats", 8, 300, 3, 40, False, ks=(16, 2), act="tanh", idx=True, stats=True),
]


def align4(a):
    return (a + 3) // 4 * 4


def gauss_data(c):
    """every input of the case as numpy arrays (float32, idx int32, adv and target_v float64), from the case id alone"""
    rng = np.random.default_rng(zlib.crc32(c.id.encode()))
    B, F, A = c.B, c.F, c.A
    npool = B + POOL_EXTRA
    idx = rng.permutation(npool)[:B].astype(np.int32) if c.idx else None
    rows = idx if c.idx else np.arange(B)
    d = dict(idx=idx, rows=rows, feat=[], parts=[], tbias=[], act_feat=c.act)
    for t in range(1 if c.shared else 2):
        ks = c.ks[t] if c.ks else 0
        if ks:
            p = (rng.standard_normal((ks, B, F)) / np.sqrt(ks)).astype(np.float32)
            tb = (rng.standard_normal(F) * 0.1).astype(np.float32)
            x = None
        else:
            p, tb = np.zeros((0, B, F), np.float32), None
            x = nets.act_fwd(rng.standard_normal((B, F)), c.act).astype(np.float32)
        d["feat"].append(x)
        d["parts"].append(p)
        d["tbias"].append(tb)
    d["wpi"] = (rng.standard_normal((F, A)) / np.sqrt(F)).astype(np.float32)
    d["bpi"] = (rng.standard_normal(A) * 0.1).astype(np.float32)
    d["wv"] = (rng.standard_normal(F) / np.sqrt(F)).astype(np.float32)
    d["bv"] = np.array([0.3], np.float32)
    d["log_std"] = (0.4 * rng.standard_normal(A)).astype(np.float32)
    feat64 = HB.ppo_features(c, d)
    mean = feat64[0] @ d["wpi"].astype(np.float64) + d["bpi"]
    value = feat64[-1] @ d["wv"].astype(np.float64) + d["bv"][0]
    ls = d["log_std"].astype(np.float64)
    action = rng.standard_normal((npool, A)).astype(np.float32)
    old_logp = (-np.abs(rng.standard_normal(npool)) - 0.3).astype(np.float32)
    adv = rng.standard_normal(npool)
    old_v = rng.standard_normal(npool).astype(np.float32)
    target_v = rng.standard_normal(npool) * 4
    # the action around the mean, the old log-probability around the new one (ratio inside and on both sides of 1 +- clip),
    # old / target value spread over a few vf_clip around the value: all four gradient outcomes are populated
    action[rows] = (mean + np.exp(ls) * rng.standard_normal((B, A))).astype(np.float32)
    zz = (action[rows].astype(np.float64) - mean) / np.exp(ls)
    logp = -(0.5 * np.log(2.0 * np.pi) * A + 0.5 * np.square(zz).sum(-1) + ls.sum())
    old_logp[rows] = (logp + rng.uniform(-0.3, 0.3, B)).astype(np.float32)
    old_v[rows] = (value + rng.uniform(-3.0, 3.0, B) * VF_CLIP).astype(np.float32)
    target_v[rows] = value + rng.uniform(-4.0, 4.0, B) * VF_CLIP
    d.update(action=action, old_logp=old_logp, adv=adv, old_v=old_v, target_v=target_v)
    return d


def gauss_reference(c, d):
    """float64 forward, loss gradients, pi_logstd rows and per-sample terms, the population of the four gradient outcomes
    and the rows that sit within MARGIN (relative) of a branch boundary"""
    feat = HB.ppo_features(c, d)
    mean = feat[0] @ d["wpi"].astype(np.float64) + d["bpi"]
    value = (feat[-1] @ d["wv"].astype(np.float64) + d["bv"][0]).reshape(-1, 1)
    rows = d["rows"]
    col = lambda a: a[rows].astype(np.float64).reshape(-1, 1)
    action = d["action"][rows].astype(np.float64)
    old_logp, old_v = col(d["old_logp"]), col(d["old_v"])
    adv = col(d["adv"].astype(np.float32))                 # (the kernel reads the float64 pools as float32)
    tv = col(d["target_v"].astype(np.float32))
    ls = d["log_std"].astype(np.float64).reshape(1, -1)
    _, dmean, dv, _, parts = nets.gauss_ppo_loss_and_grads(mean, ls, value, action, old_logp, adv, old_v, tv, CLIP, ENT,
                                                           VF_CLIP, CRITIC)
    m = c.inv_b_mul                                        # (the oracle divides by B)
    logp = parts["logp"]
    ent = np.full_like(logp, (ls + 0.5 * (np.log(2.0 * np.pi) + 1.0)).sum())
    ratio = np.exp(logp - old_logp)
    surr1, surr2 = ratio * adv, np.clip(ratio, 1 - CLIP, 1 + CLIP) * adv
    vf1 = np.square(value - tv)
    vf2 = np.square(old_v + np.clip(value - old_v, -VF_CLIP, VF_CLIP) - tv)
    terms = np.concatenate([np.minimum(surr1, surr2), ent, np.maximum(vf1, vf2)], 1)
    in_rng = (ratio >= 1 - CLIP) & (ratio <= 1 + CLIP)
    in_v = np.abs(value - old_v) <= VF_CLIP
    dsurr_zero = ~((surr1 <= surr2) | in_rng)
    dv_zero = ~(vf1 >= vf2) & ~in_v
    near = np.minimum(np.abs(ratio - (1 - CLIP)), np.abs(ratio - (1 + CLIP))) < MARGIN
    near |= ~in_rng & (np.abs(surr1 - surr2) < MARGIN * np.maximum(np.abs(surr1), np.abs(surr2)))
    near |= np.abs(np.abs(value - old_v) - VF_CLIP) < MARGIN * VF_CLIP
    near |= ~in_v & (np.abs(vf1 - vf2) < MARGIN * np.maximum(vf1, vf2))
    pops = dict(dsurr_adv=float((~dsurr_zero).mean()), dsurr_zero=float(dsurr_zero.mean()),
                dv_live=float((~dv_zero).mean()), dv_zero=float(dv_zero.mean()))
    flags = (~in_rng).astype(np.float64) + 2.0 * (~in_v).astype(np.float64)
    return dict(feat=feat, mean=mean, value=value[:, 0], dmean=dmean * m, dvalue=dv[:, 0] * m, dls_rows=parts["dls_rows"] * m,
                terms=terms, keep=~near[:, 0], pops=pops, logp=logp[:, 0], flags=flags[:, 0])


def gauss_outputs(c):
    B, F, A = c.B, c.F, c.A
    return dict(mean=out_buf(B * A), value=out_buf(B), dmean=out_buf(B * A), dvalue=out_buf(B), terms=out_buf(B * 4),
                dls_rows=out_buf(B * align4(A)), df_pi=out_buf(B * F), df_v=out_buf(B * F), feat_pi=out_buf(B * F),
                feat_v=out_buf(B * F), rows=out_buf(B * 4))


def call_gauss(L, c, d, o):
    """one xt_ppo_gauss_heads_fused_ex call on the case's data and the output buffers `o` -> (rc, path)"""
    B, F, A = c.B, c.F, c.A
    cfg = L.PpoCfg()
    cfg.clip_ratio, cfg.ent_coef, cfg.vf_clip, cfg.critic_coef = CLIP, ENT, VF_CLIP, CRITIC
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
    rc = L.load().xt_ppo_gauss_heads_fused_ex(
        f_pi, f_v, part_pi, part_v, ks_pi, ks_v, stride, tb_pi, tb_v, L.ACT[d["act_feat"]], B, F, A, 1 if c.shared else 0,
        p(d["wpi"]), p(d["bpi"]), p(d["wv"]), p(d["bv"]), p(d["log_std"]), L.ptr(HB.dev(d["idx"])) if c.idx else None,
        p(d["action"]), p(d["old_logp"]), p(d["adv"]), p(d["old_v"]), p(d["target_v"]), ctypes.byref(cfg), c.inv_b_mul / B,
        L.ACT[c.act], L.ptr(o["mean"]), L.ptr(o["value"]), L.ptr(o["dmean"]), L.ptr(o["dvalue"]), L.ptr(o["dls_rows"]),
        align4(A), L.ptr(o["terms"]), L.ptr(o["df_pi"]), L.ptr(o["df_v"]) if sep else None,
        L.ptr(o["feat_pi"]) if c.ks else None, L.ptr(o["feat_v"]) if c.ks and sep else None,
        L.ptr(o["rows"]) if c.stats else None, None, ctypes.byref(path))
    torch.cuda.synchronize()
    return rc, path.value


@pytest.mark.parametrize("c", GAUSS_CASES, ids=[c.id for c in GAUSS_CASES])
def test_ppo_gauss_heads_fused_branch_vs_fp64(L, c):
    """Bars: mean, value and the finished features 2e-6, dmean / dvalue / the three terms columns 1e-5, d(features)
    against dfeat_reference of the kernel's own dmean / dvalue 3e-6 (test_gpu_heads_branch.py::check_ppo); dls_rows and
    their float64 column sum 1e-5 (test_gpu_kernels.py::test_ppo_loss_gauss_vs_oracle)."""
    B, F, A = c.B, c.F, c.A
    ld = align4(A)
    d = gauss_data(c)
    ref = gauss_reference(c, d)
    o = gauss_outputs(c)
    rc, path = call_gauss(L, c, d, o)
    L.check(rc, "xt_ppo_gauss_heads_fused_ex " + c.id)
    assert decode_head_path(path) == (gauss_family(), c.nq, 1 if c.ks else 0, 1 if c.shared else 0, 0), \
        (c.id, decode_head_path(path))
    sizes = dict(mean=B * A, value=B, dmean=B * A, dvalue=B, terms=B * 4, dls_rows=B * ld, df_pi=B * F, df_v=B * F,
                 feat_pi=B * F, feat_v=B * F, rows=B * 4)
    got = {k: split_out(o[k], n, k) for k, n in sizes.items()}
    sep = not c.shared
    written = ["mean", "value", "dmean", "dvalue", "terms", "df_pi"] + (["df_v"] if sep else []) + \
        ((["feat_pi"] + (["feat_v"] if sep else [])) if c.ks else []) + (["rows"] if c.stats else [])
    for k in got:        # everything the instance writes is written, the rest is untouched
        if k == "dls_rows":
            continue
        assert np.isfinite(got[k]).all() if k in written else np.isnan(got[k]).all(), (c.id, k)
    dls_full = got["dls_rows"].reshape(B, ld)
    assert np.isfinite(dls_full[:, :A]).all() and np.isnan(dls_full[:, A:]).all(), c.id      # (the padding columns stay)
    mean, dm, dls = got["mean"].reshape(B, A), got["dmean"].reshape(B, A), dls_full[:, :A]
    terms = got["terms"].reshape(B, 4)
    assert (terms[:, 3] == 0).all()
    kfeat = [got["feat_pi"].reshape(B, F), got["feat_v"].reshape(B, F)][:2 if sep else 1] if c.ks else d["feat"]
    ref_dpi, ref_dv = dfeat_reference(dm, got["dvalue"], d["wpi"], d["wv"], kfeat[0], kfeat[-1], c.act, c.shared)
    keep = ref["keep"]
    # (2 % of at most 40 rows is less than one row: in effect NO row of a case may sit within MARGIN of a branch boundary;
    # tests/test_cpu_gauss_heads_coverage.py checks this on the CPU.  A case that lands a row there gets another id.)
    assert keep.any() and (~keep).sum() <= 0.02 * B, (c.id, int((~keep).sum()))
    errs = {"mean": (rel_err(mean, ref["mean"]), 2e-6), "value": (rel_err(got["value"], ref["value"]), 2e-6),
            "dmean": (rel_err(dm[keep], ref["dmean"][keep]), 1e-5),
            "dvalue": (rel_err(got["dvalue"][keep], ref["dvalue"][keep]), 1e-5),
            "dls_rows": (rel_err(dls[keep], ref["dls_rows"][keep]), 1e-5),
            "dls_sum": (rel_err(dls[keep].astype(np.float64).sum(0), ref["dls_rows"][keep].sum(0)), 1e-5),
            "df_pi": (rel_err(got["df_pi"].reshape(B, F), ref_dpi), 3e-6)}
    if sep:
        errs["df_v"] = (rel_err(got["df_v"].reshape(B, F), ref_dv), 3e-6)
    if c.ks:
        errs["feat_pi"] = (rel_err(got["feat_pi"].reshape(B, F), ref["feat"][0]), 2e-6)
        if sep:
            errs["feat_v"] = (rel_err(got["feat_v"].reshape(B, F), ref["feat"][1]), 2e-6)
    for j, k in enumerate(("surr", "ent", "vf")):
        errs["terms." + k] = (rel_err(terms[:, j], ref["terms"][:, j]), 1e-5)
    check_bars("gauss_heads {} nq {} part {} shared {} stats {} excluded {}".format(
        c.id, c.nq, int(bool(c.ks)), int(c.shared), int(c.stats), int((~keep).sum())), errs)
    if c.stats:
        check_stats_rows(c, d, ref, got)


def check_stats_rows(c, d, ref, got):
    """the diagnostic row {old_logp - logp, (!in_rng) + 2 * (!in_v), tv, tv - v}.  Columns 1 to 3 are exact: the flags of the
    rows kept (none sits within MARGIN of a boundary), the float32 target, and ONE float32 subtraction of it and the kernel's
    own value.  Column 0 against float64 on the kernel's own mean: the float32 evaluation of the log-density takes, per
    action dimension, exp, a subtraction, a division and a product (<= 5 ulp of z^2), then A + 2 additions over terms no
    larger than |logp|, and the final subtraction of old_logp: 16 ulp of max(|logp|, |old_logp|) bounds it for A <= 8."""
    B, A = c.B, c.A
    r = got["rows"].reshape(B, 4)
    rows = d["rows"]
    tv32 = d["target_v"][rows].astype(np.float32)
    assert (r[:, 2].view(np.uint32) == tv32.view(np.uint32)).all(), c.id
    assert (r[:, 3].view(np.uint32) == (tv32 - got["value"]).astype(np.float32).view(np.uint32)).all(), c.id
    keep = ref["keep"]
    assert (r[keep, 1] == ref["flags"][keep]).all(), c.id
    ls = d["log_std"].astype(np.float64)
    zz = (d["action"][rows].astype(np.float64) - got["mean"].reshape(B, A).astype(np.float64)) / np.exp(ls)
    logp = -(0.5 * np.log(2.0 * np.pi) * A + 0.5 * np.square(zz).sum(-1) + ls.sum())
    olp = d["old_logp"][rows].astype(np.float64)
    tol = 16.0 * np.spacing(np.maximum(np.abs(logp), np.abs(olp)).astype(np.float32)).astype(np.float64)
    err = np.abs(r[:, 0].astype(np.float64) - (olp - logp))
    print("gauss_heads {} rows: old_logp - logp max err / tol {:.2e}".format(c.id, float((err / tol).max())))
    assert (err <= tol).all(), (c.id, float((err / tol).max()))
