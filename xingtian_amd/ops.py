"""Stand-alone hot-path ops on the GPU (thin host wrappers over the C ABI)."""
import numpy as np
import torch

from xingtian_amd import lib as L


def gae(value, reward, done, gamma=0.99, lam=0.95, device="cuda:0"):
    """GAE for n_traj trajectories at once, float64 on the GPU, bit-exact with the
    reference's numpy loop (xt/agent/ppo/ppo.py:87-104).

    value [n,T+1] f32, reward [n,T] f64, done [n,T] bool -> (adv [n,T] f64,
    old_value [n,T] f32, target_value [n,T] f64) as numpy arrays.
    """
    L.require_gpu()
    lib = L.load()
    value = np.ascontiguousarray(value, np.float32)
    reward = np.ascontiguousarray(reward, np.float64)
    done = np.ascontiguousarray(np.asarray(done, bool).astype(np.uint8))
    n, t = reward.shape
    if value.shape != (n, t + 1) or done.shape != (n, t):
        raise ValueError("gae: value must be [n,T+1], reward/done [n,T]")
    dev = torch.device(device)
    v = torch.from_numpy(value).to(dev)
    r = torch.from_numpy(reward).to(dev)
    d = torch.from_numpy(done).to(dev)
    adv = torch.empty((n, t), dtype=torch.float64, device=dev)
    tgt = torch.empty((n, t), dtype=torch.float64, device=dev)
    ov = torch.empty((n, t), dtype=torch.float32, device=dev)
    L.check(lib.xt_gae_f64(L.ptr(v), L.ptr(r), L.ptr(d), L.ptr(adv), L.ptr(tgt), L.ptr(ov), n, t,
                           float(gamma), float(lam), L.stream_ptr()), "xt_gae_f64")
    return adv.cpu().numpy(), ov.cpu().numpy(), tgt.cpu().numpy()


def impala_stats_from_sums(sums, loss=None):
    """The per-train IMPALA v-trace diagnostics from the XT_IMPALA_STATS_DOUBLES running sums one train leaves on the device
    (C ABI ``xt_net_set_impala_stats``; slots ``lib.IMPALA_STATS_SLOTS``).  Pure host arithmetic in float64, no GPU needed.

    -> None when no chunk was counted, else a dict of Python floats.  Per transition (every transition that carries loss
    counts once): ``behaviour_kl`` = mean(-log rho), an estimator of KL(behaviour || target) on behaviour samples;
    ``rho_mean``; ``rho_clip_fraction`` = share of rho > 1, the transitions the rho_bar = c_bar = 1 clip cuts; ``entropy``;
    ``vs_mean``; ``explained_variance`` = 1 - Var(vs - v) / Var(vs) (``nan`` when Var(vs) is zero to within the rounding of
    the sums: 1e-12 of the mean square).  ``rho_max`` is a maximum.  ``pg_loss`` / ``baseline_loss`` / ``entropy_loss`` are
    the three sum-form pieces as per-chunk means, so that ``pg_loss + 0.5 * baseline_loss + 0.01 * entropy_loss`` is the mean
    chunk loss (the kernel's constants).  ``grad_norm`` / ``grad_norm_max`` / ``grad_clip_fraction`` run over the chunks.
    ``loss`` is the mean chunk loss: ``loss`` when the caller has it (``Model.train`` returns it), else the recombination."""
    a = np.asarray(sums, np.float64).reshape(-1)
    if a.shape[0] != L.IMPALA_STATS_DOUBLES:
        raise ValueError("impala_stats_from_sums: {} sums expected, got {}".format(L.IMPALA_STATS_DOUBLES, a.shape[0]))
    s = L.IMPALA_STATS_SLOTS
    chunks, trans = float(a[s["CHUNKS"]]), float(a[s["TRANSITIONS"]])
    if chunks <= 0.0:
        return None
    per_t = (lambda k: float(a[s[k]]) / trans) if trans > 0.0 else (lambda k: float("nan"))
    pg_loss = float(a[s["PG"]]) / chunks
    baseline_loss = 0.5 * float(a[s["VERR_SQ"]]) / chunks
    entropy_loss = -float(a[s["ENT"]]) / chunks
    vs_sq, err_sq = per_t("VS_SQ"), per_t("VERR_SQ")
    var_vs, var_err = vs_sq - per_t("VS") ** 2, err_sq - per_t("VERR") ** 2
    explained = 1.0 - var_err / var_vs if var_vs > 1e-12 * vs_sq else float("nan")
    if loss is None:
        loss = pg_loss + 0.5 * baseline_loss + 0.01 * entropy_loss
    return dict(chunks=chunks, transitions=trans, behaviour_kl=per_t("NEG_LOG_RHO"), rho_mean=per_t("RHO"),
                rho_max=float(a[s["RHO_MAX"]]), rho_clip_fraction=per_t("RHO_CLIPPED"), entropy=per_t("ENT"),
                pg_loss=pg_loss, baseline_loss=baseline_loss, entropy_loss=entropy_loss, explained_variance=explained,
                vs_mean=per_t("VS"), grad_norm=float(a[s["GNORM_SUM"]]) / chunks, grad_norm_max=float(a[s["GNORM_MAX"]]),
                grad_clip_fraction=float(a[s["GNORM_CLIPPED"]]) / chunks, loss=float(loss))


def ppo_stats_from_sums(acc16, loss=None, ent_coef=0.0, critic_coef=1.0):
    """The per-update PPO diagnostics from the XT_TRAIN_STATS_DOUBLES running sums one train leaves on the device (C ABI
    ``xt_net_set_train_stats``; slots ``lib.TRAIN_STATS_SLOTS``).  Pure host arithmetic in float64, no GPU needed.

    -> None when no step was counted, else a dict of Python floats: ``policy_loss`` / ``entropy`` / ``value_loss`` are
    means of the minibatch means (as the reference's loss is), ``approx_kl`` / ``clip_fraction`` / ``vf_clip_fraction`` /
    ``explained_variance`` are row-weighted (every visited row counts once), ``grad_norm`` / ``grad_norm_max`` /
    ``grad_clip_fraction`` run over the steps.  ``explained_variance`` = 1 - Var(tv - v) / Var(tv), ``nan`` when Var(tv) is
    zero (to within the rounding of the sums: 1e-12 of the mean square).  ``loss`` is the mean minibatch loss: ``loss``
    when the caller has it (``Model.train`` returns it), else ``policy_loss - ent_coef * entropy + critic_coef *
    value_loss``."""
    a = np.asarray(acc16, np.float64).reshape(-1)
    if a.shape[0] != L.TRAIN_STATS_DOUBLES:
        raise ValueError("ppo_stats_from_sums: {} sums expected, got {}".format(L.TRAIN_STATS_DOUBLES, a.shape[0]))
    s = L.TRAIN_STATS_SLOTS
    steps, rows = float(a[s["STEPS"]]), float(a[s["ROWS"]])
    if steps <= 0.0:
        return None
    per_row = (lambda k: float(a[s[k]]) / rows) if rows > 0.0 else (lambda k: float("nan"))
    policy_loss, entropy, value_loss = -float(a[s["SURR"]]) / steps, float(a[s["ENT"]]) / steps, float(a[s["VF"]]) / steps
    tv_sq, err_sq = per_row("TV_SQ"), per_row("ERR_SQ")
    var_tv, var_err = tv_sq - per_row("TV") ** 2, err_sq - per_row("ERR") ** 2
    explained = 1.0 - var_err / var_tv if var_tv > 1e-12 * tv_sq else float("nan")
    if loss is None:
        loss = policy_loss - float(ent_coef) * entropy + float(critic_coef) * value_loss
    return dict(loss=float(loss), policy_loss=policy_loss, entropy=entropy, value_loss=value_loss,
                approx_kl=per_row("KL"), clip_fraction=per_row("CLIPPED"), vf_clip_fraction=per_row("VF_CLIPPED"),
                explained_variance=explained, grad_norm=float(a[s["GNORM_SUM"]]) / steps,
                grad_norm_max=float(a[s["GNORM_MAX"]]), grad_clip_fraction=float(a[s["GNORM_CLIPPED"]]) / steps,
                steps=steps, rows=rows)
