"""Checker of the prioritised-replay path and small callers of its C entries, shared by tests/test_cpu_per.py and
tests/test_gpu_per.py.

The restatement below is written from the semantics alone ("Prioritised replay"), in Python
floats -- IEEE float64, one rounding per operation, so it can be compared with the device bit for bit: two trees of
``2 * cap2`` nodes built bottom-up from the leaves, the right-nested prefix sum over leaves [0, N - 2], the stratified
masses, the descent and the importance weights.  tests/golden/per_cases.npz holds what the executed reference computed
for the same inputs (tools/gen_golden_per.py), tests/golden/per_cases_wide.npz the same for update batches of up to 1024
rows.  ``build_trees_np`` is the same bottom-up construction level by level on numpy float64 arrays, for trees of
2^19 leaves and more.
"""
import ctypes
import os

import numpy as np

INF = float("inf")


# ----------------------------------------------------------------------------------------------- restatement
def cap2_of(capacity):
    c = 1
    while c < capacity:
        c *= 2
    return c


def build_tree(leaves, op):
    """[2 * cap2] Python floats: node i = op(node 2i, node 2i + 1), leaf cap2 + slot; node 0 is the neutral start value
    the reference leaves there and is never read"""
    cap2 = len(leaves)
    tree = [0.0] * cap2 + [float(x) for x in leaves]
    for i in range(cap2 - 1, 0, -1):
        tree[i] = op(tree[2 * i], tree[2 * i + 1])
    return tree


def min_leaves(leaves):
    """the min tree's leaves for the sum tree's: a slot never written holds the neutral element"""
    return [INF if x == 0.0 else x for x in leaves]


def build_trees(leaves_sum, leaves_min=None):
    s = build_tree(leaves_sum, lambda a, b: a + b)
    m = build_tree(min_leaves(leaves_sum) if leaves_min is None else leaves_min, min)
    m[0] = INF
    return s, m


def build_trees_np(leaves_sum, leaves_min=None):
    """``build_trees`` on numpy float64 arrays, one level per step: the same additions and the same ``min`` (the right
    operand only where it is strictly smaller), so the result equals the list builder's bit for bit"""
    ls = np.asarray(leaves_sum, np.float64)
    cap2 = len(ls)
    s, m = np.zeros(2 * cap2, np.float64), np.full(2 * cap2, INF, np.float64)
    s[cap2:] = ls
    m[cap2:] = np.where(ls == 0.0, INF, ls) if leaves_min is None else np.asarray(leaves_min, np.float64)
    lo = cap2 // 2
    while lo >= 1:
        s[lo:2 * lo] = s[2 * lo:4 * lo:2] + s[2 * lo + 1:4 * lo:2]
        left, right = m[2 * lo:4 * lo:2], m[2 * lo + 1:4 * lo:2]
        m[lo:2 * lo] = np.where(right < left, right, left)
        lo //= 2
    return s, m


def prefix_total(sum_tree, n):
    """sum over leaves [0, n - 2] as v[L1] + (v[L2] + (... + v[Lk])) over the maximal left subtrees on the way from the
    root down to leaf n - 2"""
    cap2 = len(sum_tree) // 2
    end, node, lo, hi, parts = n - 2, 1, 0, cap2 - 1, []
    while hi != end:                                       # (the range asked for always starts where the node's does)
        mid = (lo + hi) // 2
        if end <= mid:
            node, hi = 2 * node, mid
        else:
            parts.append(sum_tree[2 * node])
            node, lo = 2 * node + 1, mid + 1
    total = sum_tree[node]
    for p in reversed(parts):
        total = p + total
    return total


def find_idx(sum_tree, mass):
    cap2, i = len(sum_tree) // 2, 1
    while i < cap2:
        if sum_tree[2 * i] > mass:
            i = 2 * i
        else:
            mass -= sum_tree[2 * i]
            i = 2 * i + 1
    return i - cap2


def sample(sum_tree, min_tree, n, u, beta):
    """-> (p_total, slots [B], weights [B]) of ``sample(B, beta)`` with the uniform draws ``u`` on ``n`` stored
    transitions; a descent that ends at a leaf >= n is clamped to n - 1"""
    cap2, b = len(sum_tree) // 2, len(u)
    p_total = prefix_total(sum_tree, n)
    every = p_total / b
    slots = [min(find_idx(sum_tree, float(u[i]) * every + i * every), n - 1) for i in range(b)]
    p_min = max(min_tree[1] / sum_tree[1], 1e-5)
    max_w = (p_min * n) ** (-beta)
    weights = [(sum_tree[cap2 + s] / sum_tree[1] * n) ** (-beta) / max_w for s in slots]
    return p_total, slots, weights


def spans_of_message(capacity, head, size, n):
    """-> ([(first slot, count)] that a message of n transitions writes, new head, new size): at most two contiguous
    spans; of a message longer than the capacity the last ``capacity`` rows stay"""
    m = min(n, capacity)
    w = (head + size + n - m) % capacity
    first = min(m, capacity - w)
    spans = [(w, first)] + ([(0, m - first)] if m > first else [])
    total = size + n
    if total > capacity:
        return spans, (head + total - capacity) % capacity, capacity
    return spans, head, total


class Case(object):
    """one recorded case of tests/golden/per_cases.npz or per_cases_wide.npz"""

    def __init__(self, golden, name):
        g = lambda k: golden[name + "_" + k]
        self.name = name
        self.capacity, self.n, self.b = (int(x) for x in g("cfg")[:3])
        self.alpha, self.beta = float(g("cfg")[3]), float(g("cfg")[4])
        self.cap2 = cap2_of(self.capacity)
        self.msg_lens, self.script = g("msg_lens").tolist(), g("script").tolist()
        idx, prio, splits = g("upd_idx"), g("upd_prio"), [0] + g("upd_splits").tolist()
        self.batches = [(idx[a:z].tolist(), prio[a:z].tolist()) for a, z in zip(splits[:-1], splits[1:])]
        self.leaves, self.sum, self.min = g("leaves"), g("sum"), g("min")
        self.max_prio, self.u, self.p_total = float(g("max_prio")), g("u").tolist(), float(g("p_total"))
        self.idx, self.w = g("idx").tolist(), g("w")

    def steps(self):
        """the script as ("add", [(first, count), ...]) / ("update", slots, priorities) steps"""
        head = size = j = 0
        for s in self.script:
            if s >= 0:
                spans, head, size = spans_of_message(self.capacity, head, size, self.msg_lens[s])
                yield ("add", spans)
            else:
                yield ("update",) + self.batches[j]
                j += 1
        assert size == self.n and j == len(self.batches)

    def host_leaves(self, priority=lambda p: p):
        """-> (leaves [cap2] as Python floats, max_prio): the script replayed on the host, ``priority ** alpha``;
        ``priority`` maps a recorded priority to the one the device forms (|float32 delta| + eps)"""
        leaves, max_prio = [0.0] * self.cap2, 1.0
        for step in self.steps():
            if step[0] == "add":
                for first, count in step[1]:
                    for s in range(first, first + count):
                        leaves[s] = max_prio ** self.alpha
            else:
                for s, p in zip(step[1], map(priority, step[2])):
                    leaves[s] = p ** self.alpha
                    max_prio = max(max_prio, p)
        return leaves, max_prio


def load_cases(golden_dir, fname="per_cases.npz"):
    golden = np.load(os.path.join(golden_dir, fname))
    return {str(n): Case(golden, str(n)) for n in golden["names"]}


def rel_err(got, ref):
    """largest element-wise relative deviation"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float((np.abs(got - ref) / np.abs(ref)).max())


# ----------------------------------------------------------------------------------------------- C entries (GPU)
class GpuTrees(object):
    """sum / min trees and max_prio on cuda:0 with thin callers of xt_per_add / xt_per_update / xt_per_sample"""

    def __init__(self, capacity, alpha):
        import torch
        from xingtian_amd import lib as L
        self.L, self.lib, self.torch = L, L.load(), torch
        self.capacity, self.cap2, self.alpha = capacity, cap2_of(capacity), alpha
        dev = torch.device("cuda:0")
        self.sum = torch.zeros(2 * self.cap2, dtype=torch.float64, device=dev)
        self.min = torch.full((2 * self.cap2,), INF, dtype=torch.float64, device=dev)
        self.max_prio = torch.ones(1, dtype=torch.float64, device=dev)

    def add(self, first, count, cap2=None):
        L = self.L
        return self.lib.xt_per_add(L.ptr(self.sum), L.ptr(self.min), self.cap2 if cap2 is None else cap2,
                                   L.ptr(self.max_prio), first, count, ctypes.c_double(self.alpha), L.stream_ptr())

    def update(self, slots, delta, eps, stride=1, b=None):
        """``delta``: host float32 values, laid out on the device with ``stride`` elements between them"""
        L, torch = self.L, self.torch
        d_slots = torch.tensor(slots, dtype=torch.int32).cuda()
        buf = np.full(len(delta) * stride, np.nan, np.float32)
        buf[::stride] = delta
        d_delta = torch.from_numpy(buf).cuda()
        return self.lib.xt_per_update(L.ptr(self.sum), L.ptr(self.min), self.cap2, L.ptr(self.max_prio), L.ptr(d_slots),
                                      L.ptr(d_delta), stride, len(slots) if b is None else b, ctypes.c_double(eps),
                                      ctypes.c_double(self.alpha), L.stream_ptr())

    def sample(self, n, u, beta, b=None):
        """-> (rc, slots int32 [B], weights float64 [B]) as host arrays; the outputs start as -1 / NaN"""
        L, torch = self.L, self.torch
        d_u = torch.tensor(u, dtype=torch.float64).cuda()
        slots = torch.full((len(u),), -1, dtype=torch.int32, device="cuda")
        w = torch.full((len(u),), float("nan"), dtype=torch.float64, device="cuda")
        rc = self.lib.xt_per_sample(L.ptr(self.sum), L.ptr(self.min), self.cap2, n, L.ptr(d_u), len(u) if b is None else b,
                                    ctypes.c_double(beta), L.ptr(slots), L.ptr(w), L.stream_ptr())
        torch.cuda.synchronize()
        return rc, slots.cpu().numpy(), w.cpu().numpy()

    def read(self):
        """-> (sum tree, min tree as lists of Python floats, max_prio)"""
        self.torch.cuda.synchronize()
        return self.sum.cpu().tolist(), self.min.cpu().tolist(), float(self.max_prio.item())


    def read_np(self):
        """-> (sum tree, min tree as float64 arrays, max_prio)"""
        self.torch.cuda.synchronize()
        return self.sum.cpu().numpy(), self.min.cpu().numpy(), float(self.max_prio.item())


def assert_trees_follow_from_their_leaves_np(sum_tree, min_tree):
    """``assert_trees_follow_from_their_leaves`` for trees read back as float64 arrays"""
    cap2 = len(sum_tree) // 2
    ref_s, ref_m = build_trees_np(sum_tree[cap2:], min_tree[cap2:])
    assert np.array_equal(sum_tree[1:], ref_s[1:])
    assert np.array_equal(min_tree[1:], ref_m[1:])


def assert_trees_follow_from_their_leaves(sum_tree, min_tree):
    """every internal node of both trees equals the restatement built from the trees' own leaves, bit for bit"""
    cap2 = len(sum_tree) // 2
    ref_s, ref_m = build_trees(sum_tree[cap2:], min_tree[cap2:])
    assert sum_tree[1:] == ref_s[1:]
    assert min_tree[1:] == ref_m[1:]
