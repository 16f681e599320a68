"""Shared by tests/test_cpu_impala_stats.py and tests/test_gpu_impala_stats.py: the input recipe of the IMPALA v-trace
diagnostics tests and a float64 restatement of the per-transition quantities the STATS kernels reduce.

Recipe (``make_inputs``; everything stored as the float32 / int32 / bool the kernels read):
  logits = 1.5 N(0,1);  bp_logits = logits + 0.4 N(0,1);  a quarter of the transitions (flat index = 1 mod 4) is on-policy,
  bp_logits bit-identical to logits: both kernels and float64 then give rho = exp(0) = 1 exactly and the transition is
  NOT counted as clipped;  an off-policy transition with |log rho| < 0.02 gets +0.5 on the behaviour logit of its taken
  action;  rewards = 2 N(0,1) (the +-1 reward clip acts);  about 5 % of the transitions are done;  baseline = N(0,1).
``make_inputs`` asserts in float64 that every off-policy transition has |rho - 1| >= 1e-3: a condition on the INPUTS (no
transition is excluded anywhere), so that the count of rho > 1 is exact.  The seeds of CASES are chosen so that it holds.

``restate`` follows impala_loss_kernel statement for statement in float64; test_cpu_impala_stats.py ties the sum of its
loss terms to ``oracle.nets.impala_loss_and_grads`` (1e-12 relative)."""
import numpy as np

GAMMA = 0.99
MARGIN = 1e-3
K = 12          # XT_IMPALA_TRAJ_STATS_FLOATS
# column of a traj_stats row -> key of restate()'s per-transition arrays (column 9 is a maximum, 10 = T - 1, 11 = 0)
COLUMNS = ("ce_pg", "ent", "verr_sq", "verr", "vs", "vs_sq", "neg_log_rho", "rho", "clipped", "rho")
MAX_COL = 9
# (n_traj, T, A) of the kernel tests, by path
FUSED8 = [(1, 2, 2), (3, 64, 4), (2, 65, 6), (1, 128, 4), (20, 50, 6), (2, 129, 8), (1, 256, 3)]
FUSED32 = [(2, 5, 18), (3, 64, 9), (1, 255, 32)]
UNFUSED = [(2, 5, 18), (1, 64, 4), (2, 65, 6), (1, 128, 4), (1, 129, 3), (1, 256, 4), (1, 257, 4), (1, 1000, 6)]
CASES = sorted(set(FUSED8 + FUSED32 + UNFUSED))
SEEDS = {(1, 256, 3): 1}      # case -> seed where 0 misses the margin (a nudged transition whose behaviour policy is near one-hot)


def log_softmax64(x):
    x = np.asarray(x, np.float64)
    x = x - x.max(-1, keepdims=True)
    return x - np.log(np.exp(x).sum(-1, keepdims=True))


def taken_logp(logits, actions):
    return np.take_along_axis(log_softmax64(logits), np.asarray(actions).astype(np.int64)[..., None], -1)[..., 0]


def behaviour_logits(logits, actions, rng, n_traj, T, on_policy=True):
    """the recipe's bp_logits for given float32 logits [n_traj*T, A].  The tests through a net pass the oracle's logits and
    on_policy=False: the net's own fp32 logits differ from them in the last bits, so no transition can be on-policy to the
    bit there -- every transition is off-policy and the margin, which holds for the net's logits too, covers all of them"""
    logits = np.asarray(logits, np.float32)
    n = logits.shape[0]
    bp = (logits + 0.4 * rng.standard_normal(logits.shape)).astype(np.float32)
    on = (np.arange(n) % 4 == 1) & bool(on_policy)
    bp[on] = logits[on]
    log_rho = taken_logp(logits, actions) - taken_logp(bp, actions)
    near = ~on & (np.abs(log_rho) < 0.02)
    bp[near, np.asarray(actions)[near]] += np.float32(0.5)
    # the condition on the inputs: off-policy transitions (the bootstrap rows carry no loss) stay clear of rho = 1
    rho = np.exp(taken_logp(logits, actions) - taken_logp(bp, actions))
    carries = (np.arange(n) % T) != T - 1
    off = carries & ~on
    margin = float(np.abs(rho[off] - 1.0).min()) if off.any() else float("inf")
    assert margin >= MARGIN, ("an off-policy transition within {} of rho = 1".format(MARGIN), n_traj, T, margin)
    assert (rho[on] == 1.0).all()
    return bp, on, margin


def make_inputs(n_traj, T, A, seed=None):
    """-> dict of flat env-major arrays (index traj * T + t) + ``margin``, the smallest |rho - 1| off-policy"""
    if seed is None:
        seed = SEEDS.get((n_traj, T, A), 0)
    rng = np.random.default_rng(seed)
    n = n_traj * T
    logits = (1.5 * rng.standard_normal((n, A))).astype(np.float32)
    action = rng.integers(0, A, n).astype(np.int32)
    bp, on, margin = behaviour_logits(logits, action, rng, n_traj, T)
    reward = (2.0 * rng.standard_normal(n)).astype(np.float32)
    done = rng.random(n) < 0.05
    baseline = rng.standard_normal(n).astype(np.float32)
    return dict(logits=logits, bp=bp, action=action, reward=reward, done=done, baseline=baseline, on_policy=on,
                margin=margin, n_traj=n_traj, T=T, A=A)


def restate(logits, baseline, bp_logits, actions, dones, rewards, T, gamma=GAMMA):
    """float64, per transition [n_traj, T - 1]: the quantities the v-trace kernels hold (statement for statement
    impala_loss_kernel) -- rho, neg_log_rho = blp - tlp, clipped = rho > 1, ent, ce_pg = ce * pg_adv, vs, verr = vs - v,
    their squares, pg, and ``terms``, the transition's share of the sum-form loss"""
    lg = np.asarray(logits, np.float64)
    A = lg.shape[-1]
    n_traj = lg.shape[0] // T
    lg = lg.reshape(n_traj, T, A)[:, :-1]
    bl = np.asarray(bp_logits, np.float64).reshape(n_traj, T, A)[:, :-1]
    act = np.asarray(actions).reshape(n_traj, T)[:, :-1]
    v = np.asarray(baseline, np.float64).reshape(n_traj, T)
    val, nval = v[:, :-1], v[:, 1:]
    lsm = log_softmax64(lg)
    tlp, blp = taken_logp(lg, act), taken_logp(bl, act)
    rho = np.exp(tlp - blp)
    crho = np.minimum(1.0, rho)
    disc = np.where(np.asarray(dones, bool).reshape(n_traj, T)[:, :-1], 0.0, np.float64(gamma))
    rew = np.clip(np.asarray(rewards, np.float64).reshape(n_traj, T)[:, :-1], -1.0, 1.0)
    delta, dc = crho * (rew + disc * nval - val), disc * crho
    vs = np.zeros_like(val)
    acc = np.zeros(n_traj)
    for t in range(T - 2, -1, -1):
        acc = delta[:, t] + dc[:, t] * acc
        vs[:, t] = acc + val[:, t]
    vsn = np.concatenate([vs[:, 1:], v[:, -1:]], axis=1)
    pg = crho * (rew + disc * vsn - val)
    ent = -(np.exp(lsm) * lsm).sum(-1)
    ce = -tlp
    verr = vs - val
    terms = ce * pg + 0.5 * (0.5 * verr * verr) + 0.01 * (-ent)
    return dict(rho=rho, neg_log_rho=blp - tlp, clipped=(rho > 1.0).astype(np.float64), ent=ent, ce_pg=ce * pg, pg=pg, vs=vs,
                vs_sq=vs * vs, verr=verr, verr_sq=verr * verr, terms=terms)


def traj_rows(r):
    """the float64 value of every traj_stats column per trajectory [n_traj, 10], and sum |term| per column (the scale of a
    sum that can cancel)"""
    rows = np.stack([r[k].max(-1) if c == MAX_COL else r[k].sum(-1) for c, k in enumerate(COLUMNS)], axis=1)
    mags = np.stack([np.abs(r[k]).max(-1) if c == MAX_COL else np.abs(r[k]).sum(-1) for c, k in enumerate(COLUMNS)], axis=1)
    return rows, mags


def sums16(chunks):
    """the 16 running sums a train over `chunks` (list of restate() dicts) must leave, gradient-norm slots excluded (zero
    here), and the sum |term| of every slot"""
    want, mag = np.zeros(16), np.zeros(16)
    for r in chunks:
        rows, mags = traj_rows(r)
        want[0] += 1.0
        want[1] += r["rho"].size
        for c in range(10):
            if c == MAX_COL:
                want[2 + c] = max(want[2 + c], rows[:, c].max())
            else:
                want[2 + c] += rows[:, c].sum()
                mag[2 + c] += mags[:, c].sum()
    return want, mag
