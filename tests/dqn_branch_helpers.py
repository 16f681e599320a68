"""Twins of the DQN head kernels and of the priority-tree semantics, shared by tests/test_gpu_dqn_branch.py and
tests/test_cpu_dqn_coverage.py.

``loss_twin32`` restates ``dqn_loss_kernel`` (csrc/xt_dqn.hip) operation by operation in numpy float32: the library is
built without contraction, so every product and sum rounds once and the twin can be compared with the device bit for
bit.  ``reduce_twin64`` restates ``dqn_loss_reduce_kernel`` in float64 in the kernel's order: the per-thread partial
over b = t, t + 256, ..., the halving tree from 128, the final casts.  ``sample_twin`` / ``apply_update`` restate the
sampling and the priority write-back on the host (tests/per_helpers.py holds the trees themselves).

Every twin takes ``bug``: a deliberately wrong variant of one detail.  The comparisons the GPU tests assert with must
reject each of them for at least one case of the tables (tests/test_cpu_dqn_coverage.py).
"""
import numpy as np

import dqn_helpers as H

F = np.float32
LOSS_BUGS = ("last_max", "gamma_f32", "w_f64", "w_by_slot", "no_clamp", "div_b")
REDUCE_BUGS = ("first_stride",)
SAMPLE_BUGS = ("left_nested", "with_last", "descent_ge", "no_floor")
UPDATE_BUGS = ("first_dup", "max_winners")


# ----------------------------------------------------------------------------------------------- xt_dqn_loss_w
def _mean32(l):
    s = np.zeros(l.shape[0], F)
    for a in range(l.shape[1]):                            # sequential, as the kernel's loop
        s = s + l[:, a]
    return s / F(l.shape[1])


def _q32(l, s, dueling):
    return s[:, None] + (l - _mean32(l)[:, None]) if dueling else l


def _argmax(q, last=False):
    return q.shape[1] - 1 - np.argmax(q[:, ::-1], axis=1) if last else np.argmax(q, axis=1)


def loss_twin32(d, dueling, double, gamma, weighted, slots=None, bug=None):
    """-> dict(astar, maxq, y, terms [2B], dlogits [B, A], dvalue [B], w32 [B] or None) of float32 / int arrays.  ``d``:
    float32 heads [B, ...], label arrays indexed by ``slots`` (None: by row), float64 ``w`` [B] indexed by row."""
    l, tl = d["logits"], d["t_logits"]
    b, a = l.shape
    rows = np.arange(b)
    lab = rows if slots is None else np.asarray(slots, np.int64)
    qt = _q32(tl, d["t_value"], dueling)
    pick = _q32(d["o_logits"], d["o_value"], dueling) if double else qt
    astar = _argmax(pick, last=bug == "last_max")
    maxq = qt[rows, astar]
    reward, done, action = d["reward"][lab], d["done"][lab], d["action"][lab].astype(np.int64)
    if bug == "gamma_f32":
        boot = (np.asarray(reward, np.float64) + (F(gamma) * maxq).astype(np.float64)).astype(F)
        y = np.where(done.astype(bool), np.asarray(reward, np.float64).astype(F), boot)
    else:
        y = H.y_numpy1(reward, maxq, done, gamma)
    act = np.clip(action, 0, a - 1)
    if bug == "no_clamp":                                  # what an unclamped index reads: the neighbouring row
        flat = np.concatenate([l.reshape(-1), np.zeros(a, F)])
        la = flat[rows * a + action]
        hot = (np.arange(a)[None, :] == action[:, None]).astype(F)
    else:
        la = l[rows, act]
        hot = (np.arange(a)[None, :] == act[:, None]).astype(F)
    qa = d["value"] + (la - _mean32(l)) if dueling else la
    delta = qa - y
    w32 = None
    if weighted:
        w32 = np.asarray(d["w"], np.float64).astype(F)
        if bug == "w_by_slot":
            w32 = w32[lab % b]
    if weighted and bug == "w_f64":
        x = (np.asarray(d["w"], np.float64) * delta.astype(np.float64)).astype(F)
    else:
        x = w32 * delta if weighted else delta
    den = F(b) if bug == "div_b" else F(b) * F(a)
    g = F(2.0) * x / den
    if dueling:
        dlogits, dvalue = g[:, None] * (hot - F(1.0) / F(a)), g.copy()
    else:
        dlogits, dvalue = g[:, None] * hot, np.zeros(b, F)
    terms = np.stack([delta, maxq], axis=1).reshape(-1)
    out = dict(astar=astar.astype(np.int32), maxq=maxq, y=y, terms=terms, dlogits=dlogits, dvalue=dvalue, w32=w32)
    assert all(v is None or v.dtype in (F, np.int32) for v in out.values())
    return out


def reduce_twin64(terms, b, a, w32=None, bug=None):
    """-> float32 [3]: (loss, mean |delta|, mean bootstrap Q) as ``dqn_loss_reduce_kernel`` forms them from the float32
    ``terms`` [2B] and the float32 weights"""
    delta, maxq = terms[0::2], terms[1::2]
    d2 = delta.astype(np.float64) * delta.astype(np.float64)
    cols = np.stack([w32.astype(np.float64) * d2 if w32 is not None else d2, np.abs(delta).astype(np.float64),
                     maxq.astype(np.float64)])
    strides = 1 if bug == "first_stride" else (b + 255) // 256
    padded = np.zeros((3, max(strides, (b + 255) // 256) * 256))          # (x + 0.0 is x: the rows no thread owns)
    padded[:, :b] = cols
    acc = np.zeros((3, 256))
    for k in range(strides):                               # thread t: b = t, t + 256, ...
        acc = acc + padded[:, 256 * k:256 * (k + 1)]
    o = 128
    while o > 0:
        acc[:, :o] = acc[:, :o] + acc[:, o:2 * o]
        o //= 2
    return np.array([acc[0, 0] / (float(b) * float(a)), acc[1, 0] / float(b), acc[2, 0] / float(b)]).astype(F)


def loss_ref64(d, dueling, double, gamma, weighted, slots=None):
    """-> (reference with the weights, reference without) in float64; an action outside [0, A) counts as the nearest
    valid one"""
    b, a = d["logits"].shape
    lab = np.arange(b) if slots is None else np.asarray(slots, np.int64)
    f64 = lambda x: np.asarray(x, np.float64)
    heads = [f64(d["logits"]), f64(d["value"]), f64(d["t_logits"]), f64(d["t_value"]),
             f64(d["o_logits"]) if double else None, f64(d["o_value"]) if double else None]
    labels = (np.clip(d["action"][lab], 0, a - 1), d["reward"][lab], d["done"][lab], gamma, dueling)
    plain = H.dqn_loss_ref(*heads, *labels)
    return (H.dqn_loss_ref(*heads, *labels, d["w"]) if weighted else plain), plain


BITWISE_KEYS = ("astar", "maxq", "y", "terms", "dlogits", "dvalue")


def bits_differ(got, want):
    """number of elements whose bit patterns differ (so -0.0 is not 0.0, and a NaN equals only itself)"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.size == want.size, (got.dtype, want.dtype, got.shape, want.shape)
    as_int = {4: np.int32, 8: np.int64}[got.dtype.itemsize]
    return int((got.reshape(-1).view(as_int) != want.reshape(-1).view(as_int)).sum())


def loss_bit_diffs(got, twin, out3):
    """-> {name: differing elements} of a kernel result (or a wrong twin) against the float32 twin and the ordered
    float64 reduction ``out3``"""
    diffs = {k: bits_differ(got[k], twin[k]) for k in BITWISE_KEYS}
    diffs["out3"] = bits_differ(got["out3"], out3)
    return diffs


BAR_LOSS, BAR_ELEM = 1e-4, 1e-5            # the bars of tests/test_gpu_dqn.py and tests/test_gpu_per.py


def loss_f64_errors(got, ref, plain, dueling):
    """-> {name: (error, bar)} against float64, as tests/test_gpu_dqn.py and tests/test_gpu_per.py measure them; an exact
    comparison reports 0.0 or inf"""
    o = np.asarray(got["out3"], np.float64)
    errs = {"astar": (0.0 if np.array_equal(got["astar"], ref["astar"]) else np.inf, 0.0),
            "loss": (abs(o[0] - ref["loss"]) / max(1.0, abs(ref["loss"])), BAR_LOSS),
            "abs_td": (abs(o[1] - plain["abs_td"]) / max(1.0, plain["abs_td"]), BAR_ELEM),
            "mean_maxq": (abs(o[2] - plain["mean_maxq"]) / max(1.0, abs(plain["mean_maxq"])), BAR_ELEM),
            "maxq": (H.rel_max(got["maxq"], ref["maxq"]), BAR_ELEM), "y": (H.rel_max(got["y"], ref["y"]), BAR_ELEM),
            "delta": (H.rel_max(got["terms"][0::2], ref["delta"]), BAR_ELEM),
            "dlogits": (H.rel_max(got["dlogits"], ref["dlogits"]), BAR_ELEM)}
    if dueling:
        errs["dvalue"] = (H.rel_max(got["dvalue"], ref["dvalue"]), BAR_ELEM)
    else:
        errs["dvalue"] = (np.inf if np.asarray(got["dvalue"]).any() else 0.0, 0.0)
    return errs


def within(errs):
    return all(e <= bar for e, bar in errs.values())


PAD = 3                                    # rows (and 2 * PAD + 1 floats of ``out``) behind what the launch owns (``pad``
                                           # of ``dqn_helpers.gpu_dqn_loss``)


# ----------------------------------------------------------------------------------------------- trees
def workgroup(b):
    """threads ``xt_per_update`` / ``xt_per_sample`` launch for a batch of ``b`` rows"""
    return (b + 63) // 64 * 64


def prefix_parts(sum_tree, n):
    """the maximal left subtrees' sums L1 .. Lk whose leaves are [0, n - 2], from the root downwards"""
    cap2 = len(sum_tree) // 2
    end, node, lo, hi, parts = n - 2, 1, 0, cap2 - 1, []
    while hi != end:
        mid = (lo + hi) // 2
        if end <= mid:
            node, hi = 2 * node, mid
        else:
            parts.append(float(sum_tree[2 * node]))
            node, lo = 2 * node + 1, mid + 1
    return parts + [float(sum_tree[node])]


def sample_twin(sum_tree, min_tree, n, u, beta, bug=None):
    """``per_helpers.sample`` (-> p_total, slots, weights) with a switch per detail"""
    cap2, b = len(sum_tree) // 2, len(u)
    parts = prefix_parts(sum_tree, n + 1 if bug == "with_last" else n)
    if bug == "left_nested":
        p_total = parts[0]
        for p in parts[1:]:
            p_total = p_total + p
    else:
        p_total = parts[-1]
        for p in reversed(parts[:-1]):
            p_total = p + p_total
    every = p_total / b
    slots = []
    for i in range(b):
        mass, node = float(u[i]) * every + i * every, 1
        while node < cap2:
            left = float(sum_tree[2 * node])
            if left >= mass if bug == "descent_ge" else left > mass:
                node = 2 * node
            else:
                mass -= left
                node = 2 * node + 1
        slots.append(min(node - cap2, n - 1))
    total = float(sum_tree[1])
    p_min = float(min_tree[1]) / total
    if bug != "no_floor":
        p_min = max(p_min, 1e-5)
    max_w = (p_min * n) ** (-beta)
    weights = [(float(sum_tree[cap2 + s]) / total * n) ** (-beta) / max_w for s in slots]
    return p_total, slots, weights


def apply_update(leaves, max_prio, slots, prios, alpha, bug=None):
    """one ``update_priorities`` batch on the host leaves (a float64 array of cap2 elements, changed in place) ->
    the new max_prio.  Of equal slots the last row wins, every row's priority counts for the maximum; a slot outside
    [0, cap2) is not stored."""
    cap2 = len(leaves)
    rows = [(int(s), float(p)) for s, p in zip(slots, prios)]
    for s, p in (reversed(rows) if bug == "first_dup" else rows):
        if 0 <= s < cap2:
            leaves[s] = p ** alpha
    if bug == "max_winners":
        last = {s: p for s, p in rows}
        return max([max_prio] + list(last.values()))
    return max([max_prio] + [p for _, p in rows])


def replay_case(case, priority=lambda p: p, bug=None):
    """``Case.host_leaves`` through ``apply_update`` -> (leaves [cap2] float64 array, max_prio)"""
    leaves, max_prio = np.zeros(case.cap2), 1.0
    for step in case.steps():
        if step[0] == "add":
            for first, count in step[1]:
                leaves[first:first + count] = max_prio ** case.alpha
        else:
            max_prio = apply_update(leaves, max_prio, step[1], [priority(p) for p in step[2]], case.alpha, bug)
    return leaves, max_prio
