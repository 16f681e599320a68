"""Checker of the n-step path and small callers of its C entries, shared by tests/test_cpu_nstep.py and
tests/test_gpu_nstep.py.

The brute force below is written from the semantics alone ("n-step returns"): it never looks at a
ring.  Every message is kept as a Python list of its rows, a stored transition is the pair (message id, t), and the
target of (m, t) sums ``reward[m][t] + g reward[m][t + 1] + ...`` left to right in Python floats while rows of the same
message remain, none of them was terminal and fewer than n were taken.  ``BruteStore`` only records which pair a slot
holds (rows are written to consecutive slots modulo the capacity), so that a result can be compared with what
``nstep_targets`` and the kernel derive from the rings and the ``follow`` ring.
"""
import ctypes
import collections

import numpy as np

GAMMA = 0.99
CAUSES = ("full", "done_start", "done_mid", "message_end")


# ----------------------------------------------------------------------------------------------- brute force
def message_lengths(capacity):
    """lengths 1, 2, 6 and one longer than the capacity, in an order that wraps the ring and evicts"""
    return [6, 1, 2, 6, 2, capacity + 3, 6, 6, 1, 2, 6] if capacity < 20 else [6, 6, 1, 2, 6, 6, 6, 6, 6, 2, capacity + 7, 6, 1,
                                                                                 6, 2, 6, 6]


def make_messages(capacity, seed, a_dim=3, states=None, reward_shift=0.0):
    """-> list of messages (dicts of the five columns the reference's agents send, plus ``tag``: the global row index).
    ``states(tags, is_next)`` builds the state rows; by default [tag (+ 0.5 for the next state), tag * 2].  The rewards
    are standard normal draws plus ``reward_shift``."""
    rng = np.random.default_rng(seed)
    if states is None:
        states = lambda tags, nxt: np.stack([tags + (0.5 if nxt else 0.0), tags * 2.0], 1).astype(np.float32)
    msgs, tag = [], 0
    for i, n in enumerate(message_lengths(capacity)):
        tags = np.arange(tag, tag + n)
        tag += n
        done = rng.random(n) < 0.25
        if n == 6 and i % 2 == 0:
            done[:] = False                                  # some messages without a terminal row: full walks, message ends
        msgs.append({"tag": tags, "cur_state": states(tags, False), "next_state": states(tags, True),
                     "action": rng.integers(0, a_dim, n).astype(np.int32),
                     "reward": [float(x) + reward_shift for x in rng.standard_normal(n)], "done": [bool(x) for x in done]})
    return msgs


class BruteStore(object):
    """which (message id, t) every slot holds after the messages added so far"""

    def __init__(self, capacity):
        self.capacity, self.written, self.msgs = capacity, 0, []
        self.slot = [None] * capacity
        self.evicted = False

    def add(self, msg):
        mid = len(self.msgs)
        self.msgs.append(msg)
        for t in range(len(msg["done"])):                    # a row at a time: a long message overwrites its own head
            s = self.written % self.capacity
            self.evicted = self.evicted or self.slot[s] is not None
            self.slot[s] = (mid, t)
            self.written += 1

    def size(self):
        return min(self.written, self.capacity)

    def head(self):
        return (self.written - self.size()) % self.capacity

    def live_slots(self):
        return [s for s in range(self.capacity) if self.slot[s] is not None]

    def follow(self):
        """rows that come after the slot's row in its message (0 for a slot never written)"""
        return [0 if x is None else len(self.msgs[x[0]]["done"]) - 1 - x[1] for x in self.slot]

    def slot_of(self, mid, t):
        return self.slot.index((mid, t))

    def target(self, s, n, gamma=GAMMA):
        """-> dict(boot, action, reward, disc, done, cause, wraps, oldest) of the n-step target that starts at slot s"""
        mid, t = self.slot[s]
        m = self.msgs[mid]
        total, g, k = m["reward"][t], gamma, 0
        while k < n - 1 and t + k + 1 < len(m["done"]) and not m["done"][t + k]:
            k += 1
            total = total + g * m["reward"][t + k]
            g = g * gamma
        if m["done"][t + k]:
            cause = "done_start" if k == 0 else ("done_mid" if k < n - 1 else "full")
        else:
            cause = "full" if k == n - 1 else "message_end"
        boot = self.slot_of(mid, t + k)                      # (raises if a walked row is no longer stored)
        for i in range(k + 1):
            assert self.slot[(s + i) % self.capacity] == (mid, t + i)        # live rows only walk live rows
        return dict(boot=boot, action=int(m["action"][t]), reward=total, disc=g, done=int(m["done"][t + k]), cause=cause,
                    wraps=boot < s, oldest=self.evicted and s == self.head(), next_tag=float(m["tag"][t + k]) + 0.5,
                    tag=float(m["tag"][t]))

    def targets(self, slots, n, gamma=GAMMA):
        """the five label columns for ``slots`` as ``nstep_targets`` returns them, and the list of dicts"""
        rows = [self.target(s, n, gamma) for s in slots]
        cols = tuple(np.asarray([r[k] for r in rows], dt) for k, dt in (("boot", np.int32), ("action", np.int32),
                                                                        ("reward", np.float64), ("disc", np.float64),
                                                                        ("done", np.uint8)))
        return cols, rows


def fill(replay, capacity, seed, a_dim=3, states=None, reward_shift=0.0):
    """feed ``make_messages`` into a ``DeviceReplay`` and a ``BruteStore`` -> (store, messages)"""
    msgs = make_messages(capacity, seed, a_dim, states, reward_shift)
    store = BruteStore(capacity)
    for m in msgs:
        replay.add(m["cur_state"], m["next_state"], m["action"], m["reward"], m["done"])
        store.add(m)
    return store, msgs


def host_rings(replay):
    """-> (follow, action, reward, done) of a filled replay as host arrays"""
    h = lambda x: x.cpu().numpy()
    return h(replay.follow), h(replay.action), h(replay.reward), h(replay.done)


def cause_counts(capacities=(7, 50), steps=(2, 3, 5), seed=11):
    """how often every stop cause, a walk across the ring's end and a start at the oldest live row occur in the case
    table (all live slots after every message, every n), counted on the brute-force side"""
    c = collections.Counter()
    for cap in capacities:
        store = BruteStore(cap)
        for m in make_messages(cap, seed):
            store.add(m)
            for n in steps:
                for s in store.live_slots():
                    r = store.target(s, n)
                    c[r["cause"]] += 1
                    c["wraps"] += bool(r["wraps"] and r["boot"] != s)
                    c["oldest"] += bool(r["oldest"])
    return c


# ----------------------------------------------------------------------------------------------- C entries (GPU)
def gpu_gather_nstep(replay, slots, n, gamma=GAMMA, follow="ring", labels=True, b=None):
    """-> (rc, dst, dict of the five label tensors): xt_replay_gather_nstep on a filled ``DeviceReplay``; ``dst`` starts
    as 0xA5 bytes, the labels as -7 / NaN / 0xA5.  ``follow`` None / ``labels`` False pass null pointers."""
    import torch
    from xingtian_amd import lib as L
    ring = replay.next_state
    rb = ring[0].numel() * ring.element_size()
    d_slots = torch.tensor(list(slots), dtype=torch.int32, device=ring.device)
    nb = len(slots)
    dst = torch.full((nb, rb), 0xA5, dtype=torch.uint8, device=ring.device)
    lab = dict(boot=torch.full((nb,), -7, dtype=torch.int32, device=ring.device),
               action=torch.full((nb,), -7, dtype=torch.int32, device=ring.device),
               reward=torch.full((nb,), float("nan"), dtype=torch.float64, device=ring.device),
               disc=torch.full((nb,), float("nan"), dtype=torch.float64, device=ring.device),
               done=torch.full((nb,), 0xA5, dtype=torch.uint8, device=ring.device))
    lp = lambda k: L.ptr(lab[k]) if labels else None
    rc = L.load().xt_replay_gather_nstep(L.ptr(ring), rb, replay.capacity, L.ptr(d_slots), nb if b is None else b,
                                         L.ptr(replay.action), L.ptr(replay.reward), L.ptr(replay.done),
                                         L.ptr(replay.follow) if follow == "ring" else None, n, ctypes.c_double(gamma),
                                         L.ptr(dst), lp("boot"), lp("action"), lp("reward"), lp("disc"), lp("done"),
                                         L.stream_ptr())
    torch.cuda.synchronize()
    return rc, dst, lab


class CountingLib(object):
    """stands in for ``HipActorCritic.lib``: counts the calls of every entry by name"""

    def __init__(self, lib):
        self._lib, self.calls = lib, collections.Counter()

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def counted(*args):
            self.calls[name] += 1
            return fn(*args)
        return counted
