"""Host restatements for the tests of the device acting path (``xt_net_act``): the Philox4x32-10 generator and the layout
that maps (seed, call, row, action) to uniforms (include/xt_mi355x.h), the float64 references of the log-probabilities and
the numpy expressions of the host ``predict`` path.  Not a test module."""
import numpy as np

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_MASK = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: four uint32 words (scalars or equal-shaped arrays), key: two -> uint32 array [..., 4]"""
    c = [np.asarray(x, dtype=np.uint64) & _MASK for x in np.broadcast_arrays(*counter)]
    k0, k1 = np.uint64(int(key[0]) & 0xFFFFFFFF), np.uint64(int(key[1]) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]          # 32 x 32 -> 64 bit: no overflow in uint64
        c = [(p1 >> _S32) ^ c[1] ^ k0, p1 & _MASK, (p0 >> _S32) ^ c[3] ^ k1, p0 & _MASK]
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return np.stack(c, axis=-1).astype(np.uint32)


def uniform(words):
    """u = (float(w >> 9) + 0.5) * 2^-23, exact in float32 and in float64; in [2^-24, 1 - 2^-24]"""
    return ((np.asarray(words, dtype=np.uint32) >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def _blocks(seed, call, rows, nblocks):
    """[len(rows), nblocks, 4] words: counter = (row, j, call low, call high), key = (seed low, seed high)"""
    rows = np.asarray(rows, dtype=np.uint64).reshape(-1, 1)
    j = np.arange(nblocks, dtype=np.uint64).reshape(1, -1)
    seed, call = int(seed) & (2 ** 64 - 1), int(call) & (2 ** 64 - 1)
    return philox4x32_10((rows, j, call & 0xFFFFFFFF, call >> 32), (seed & 0xFFFFFFFF, seed >> 32))


def categorical_uniforms(seed, call, rows, a):
    """[len(rows), a] float64: action k draws word k & 3 of block k >> 2"""
    w = _blocks(seed, call, rows, (a + 3) // 4)
    return uniform(w.reshape(len(w), -1)[:, :a])


def gumbel(seed, call, rows, a):
    return -np.log(-np.log(categorical_uniforms(seed, call, rows, a)))


def gauss_eps(seed, call, rows, a):
    """[len(rows), a] float64 Box-Muller: dimension k draws words 2(k & 1), 2(k & 1) + 1 of block k >> 1 as u1, u2"""
    w = _blocks(seed, call, rows, (a + 1) // 2)
    u = uniform(w.reshape(len(w), -1, 2)[:, :a])
    return np.sqrt(-2.0 * np.log(u[..., 0])) * np.cos(2.0 * np.pi * u[..., 1])


# ---- references
def log_softmax64(logits):
    x = np.asarray(logits, dtype=np.float64)
    x = x - x.max(axis=-1, keepdims=True)
    return x - np.log(np.exp(x).sum(axis=-1, keepdims=True))


def cat_logp_ref(logits, action):
    return np.take_along_axis(log_softmax64(logits), np.asarray(action, np.int64).reshape(-1, 1), axis=1)


def gauss_logp_ref(mean, log_std, action):
    m, ls, x = (np.asarray(v, dtype=np.float64) for v in (mean, log_std, action))
    ls = ls.reshape(1, -1)
    return -(0.5 * np.log(2.0 * np.pi) * m.shape[-1] + 0.5 * np.square((x - m) / np.exp(ls)).sum(-1, keepdims=True)
             + ls.sum(-1, keepdims=True))


def cat_logp_host(logits, action):
    """the numpy expressions of the host ``PPO.predict`` (float32 logits in, float32 out)"""
    m = logits.max(axis=-1, keepdims=True)
    lsm = logits - m - np.log(np.exp(logits - m).sum(axis=-1, keepdims=True))
    return np.take_along_axis(lsm, np.asarray(action)[:, None].astype(np.int64), axis=1).astype(np.float32)


def gauss_logp_host(mean, log_std, action):
    """the numpy expressions of the host ``PPO.predict``, DiagGaussian branch, for a given action"""
    log_std = np.asarray(log_std, np.float32).reshape(1, -1)
    std = np.exp(log_std)
    neglogp = np.float32(0.5 * np.log(2.0 * np.pi)) * np.float32(mean.shape[-1]) \
        + 0.5 * np.square((action - mean) / std).sum(-1, keepdims=True) + log_std.sum(-1, keepdims=True)
    return (-neglogp).astype(np.float32)


def logp_bound(e_host, ref):
    """G3: e_dev <= 4 e_host + 4 * 2^-24 * (1 + max |ref|)"""
    return 4.0 * e_host + 4.0 * 2.0 ** -24 * (1.0 + float(np.abs(ref).max()))


# ---- the sampling-law cases (B = 65 536 identical rows, seed 2026, call 7)
LAW_N, LAW_SEED, LAW_CALL = 65536, 2026, 7
LAW_LOGITS = [np.array([0.3, -1.2, 2.0, 0.0], np.float32), np.array([1.5, -3, 0, 0.25, -0.5, 4], np.float32),
              np.linspace(-2, 2, 18).astype(np.float32)]


def categorical_law_sigmas(action, logits):
    """per action |count - N p| / sqrt(N p (1 - p)) with p the float64 softmax"""
    n = len(action)
    p = np.exp(log_softmax64(logits))
    count = np.bincount(np.asarray(action).reshape(-1), minlength=len(p)).astype(np.float64)
    return np.abs(count - n * p) / np.sqrt(n * p * (1.0 - p))


def gauss_law_sigmas(eps):
    """(|mean| sqrt N, |var - 1| / sqrt(2 / N), |corr| sqrt N) maxima over the dimensions / pairs of eps [N, A]"""
    e = np.asarray(eps, dtype=np.float64)
    n = len(e)
    corr = np.corrcoef(e.T)
    off = np.abs(corr[~np.eye(e.shape[1], dtype=bool)]).max()
    return (np.abs(e.mean(0)).max() * np.sqrt(n), (np.abs(e.var(0) - 1.0) / np.sqrt(2.0 / n)).max(), off * np.sqrt(n))
