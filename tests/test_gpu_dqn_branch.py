"""GPU tests of every launch shape of csrc/xt_dqn.hip (TD / MSE head) and csrc/xt_per.hip (sum / min trees, sampling,
priority update) beyond the default batch of 32 and the toy rings of tests/test_gpu_dqn.py and tests/test_gpu_per.py.

One table per entry, the expected launch shape in every row:
  LOSS_CASES    ``xt_dqn_loss_w`` at 1, 2, 3 and 4 blocks of 256 rows (and as many strides of the reduction), dueling x
                double x weights x label gather through ``slots``; bit for bit against the float32 twin of
                tests/dqn_branch_helpers.py and the ordered float64 reduction, and against float64 at the bars of
                tests/test_gpu_dqn.py
  WIDE_NAMES    the recorded cases of tests/golden/per_cases_wide.npz: update workgroups of 64 .. 1024 threads
  DEEP_STEPS    adds and updates on a tree of 2^19 leaves (19 levels), every node checked after every step
  SAMPLE_CASES  ``xt_per_sample`` at 64, 320 and 1024 threads on that tree and on a freshly filled one, on both sides
                of the ``p_min`` floor, with draws on the edges and masses exactly on leaf boundaries
and ``xt_net_dqn_step`` / ``xt_net_dqn_step_per`` at B = 320 on the MLP pair.

tests/test_cpu_dqn_coverage.py checks without a GPU that these tables cover what they claim and that every comparison
used here rejects a deliberately wrong twin.  Measured figures: profiles/dqn_branch_parity.md."""
import collections
import math
import zlib

import numpy as np
import pytest
import torch

import dqn_branch_helpers as B
import dqn_helpers as H
import per_helpers as P

pytestmark = pytest.mark.gpu

GAMMA = 0.99
EPS = 1e-6


@pytest.fixture(scope="module")
def L():
    from xingtian_amd import lib
    lib.require_gpu()
    lib.load()
    return lib


def _seed(name):
    return zlib.crc32(name.encode())


# ------------------------------------------------------------------------------------------------ tables
LossCase = collections.namedtuple("LossCase", "id b a dueling double weighted via_slots blocks")
# (B, A, blocks of dqn_loss_kernel = strides of dqn_loss_reduce_kernel)
LOSS_SHAPES = ((255, 4, 1), (256, 4, 1), (257, 1, 2), (257, 18, 2), (513, 64, 3), (1000, 2, 4))
LOSS_CASES = [LossCase("b{}_a{}{}{}{}{}".format(b, a, "_duel" if du else "", "_double" if do else "", "_w" if w else "",
                                                "_slots" if sl else ""), b, a, du, do, w, sl, blocks)
              for b, a, blocks in LOSS_SHAPES for du in (False, True) for do in (False, True) for w in (False, True)
              for sl in (False, True)]

WIDE_NAMES = ("w1000_b1024", "w330_b320", "w140_b129", "w100_b65")
WIDE_WORKGROUPS = {64, 128, 192, 256, 320, 704, 960, 1024}

DEEP_CAP, DEEP_CAP2, DEEP_ALPHA, DEEP_BETA = 400000, 1 << 19, 0.6, 0.4
FRESH_SIZE = 250000
# kind "add": spans [(first, count)]; kind "update": rows, threads of the launch
DeepStep = collections.namedtuple("DeepStep", "id kind rows threads")
DEEP_STEPS = (DeepStep("fill", "add", ((0, DEEP_CAP),), 256),
              DeepStep("raise", "update", 3, 64),                          # max_prio leaves 1.0 before the next message
              DeepStep("wrap", "add", ((DEEP_CAP - 10, 10), (0, 15)), 256),
              DeepStep("u1024_a", "update", 1024, 1024), DeepStep("u1024_b", "update", 1024, 1024),
              DeepStep("u1024_c", "update", 1024, 1024),
              DeepStep("one_first", "update", 1, 64), DeepStep("one_last", "update", 1, 64),
              DeepStep("u320_outside", "update", 320, 320))
FAR_PAIRS = ((0, 600), (100, 1023), (423, 936))                            # equal slots more than 512 rows apart
LATE_ROW = 777                                                             # a row only the first halving step of the maximum reaches

# tree: "deep" after DEEP_STEPS | "fresh" one add of FRESH_SIZE leaves | "nest" eight leaves whose prefix sum depends
# on the nesting.  draws: "edges" random with 0.0 first and 1 - 2^-53 last | "zero" | "one" | "grid" 0.0 and 0.5 in turn
SampleCase = collections.namedtuple("SampleCase", "id tree size b threads draws")
SAMPLE_CASES = (SampleCase("deep_b1_zero", "deep", DEEP_CAP, 1, 64, "zero"),
                SampleCase("deep_b1_one", "deep", DEEP_CAP, 1, 64, "one"),
                SampleCase("deep_b320", "deep", DEEP_CAP, 320, 320, "edges"),
                SampleCase("deep_b1024", "deep", DEEP_CAP, 1024, 1024, "edges"),
                SampleCase("fresh_b1_one", "fresh", FRESH_SIZE, 1, 64, "one"),
                SampleCase("fresh_b320", "fresh", FRESH_SIZE, 320, 320, "edges"),
                SampleCase("fresh_b1024", "fresh", FRESH_SIZE, 1024, 1024, "edges"),
                # p_total = 2^17 over 1024 strata: every mass is a whole number, the boundary between two leaves
                SampleCase("fresh_b1024_grid", "fresh", (1 << 17) + 1, 1024, 1024, "grid"),
                SampleCase("nest_b1_one", "nest", 8, 1, 64, "one"))
NEST_ALPHA, NEST_EPS = 1.0, 2.0 ** -10
# |delta| + eps: 2^53, three times 2^-10, 0.5, 0.5, 1, 1 -> leaves [0, 6] sum to 2^53 + (1 + 1) = 2^53 + 2 from the right
# and to (2^53 + 1) + 1 = 2^53 from the left; the draw 1 - 2^-53 then ends in leaf 4 or in leaf 0
NEST_DELTA = (2.0 ** 53, 0.0, 0.0, 0.0, 0.5 - 2.0 ** -10, -(0.5 - 2.0 ** -10), 1.0 - 2.0 ** -10, 1.0 - 2.0 ** -10)

StepCase = collections.namedtuple("StepCase", "id per b cap dueling double threads")
STEP_CASES = tuple(StepCase("{}_b320{}".format("per" if per else "uniform", "_duel_double" if du else ""), per, 320, 600, du,
                            du, 320) for per in (True, False) for du in (True, False))


# ------------------------------------------------------------------------------------------------ data
def loss_rows(c):
    """the rows with a special role: (tie rows, row of action -1, row of action A): ties in the first and the last block,
    the two actions outside [0, A) in rows >= 256 wherever the batch has two such rows (else in its last two rows)"""
    return (3, c.b - 1), c.b - 1, 256 if c.b > 257 else c.b - 2


def tie_columns(a):
    """the two equal maxima of the first and of the last tie row: the first of each pair is the bootstrap action"""
    return (0, a - 1), (max(a // 2 - 1, 0), a - 1)


def loss_data(c):
    """-> (inputs of tests/dqn_branch_helpers.py's twins and caller, slots or None)"""
    rng = np.random.default_rng(_seed(c.id))
    b, a = c.b, c.a
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    d = dict(logits=f(b, a), value=f(b), t_logits=f(b, a) * 2, t_value=f(b), o_logits=f(b, a) * 2, o_value=f(b))
    ties, row_neg, row_big = loss_rows(c)
    if a >= 2:
        for k in ("t_logits", "o_logits"):
            for row, (j1, j2) in zip(ties, tie_columns(a)):
                d[k][row, j1] = d[k][row, j2] = d[k][row].max() + np.float32(1.0)
    n = 3 * b if c.via_slots else b
    slots = None
    if c.via_slots:
        slots = rng.permutation(n)[:b].astype(np.int32)
        slots[b - 7], slots[11] = slots[5], slots[10]                       # duplicates, far apart and adjacent
    lab = np.arange(b) if slots is None else slots
    d["action"] = rng.integers(0, a, n).astype(np.int32)
    d["reward"] = rng.standard_normal(n)
    d["done"] = np.where(np.arange(n) % 3 == 0, np.where(np.arange(n) % 2 == 0, 1, 255), 0).astype(np.uint8)
    d["action"][lab[row_neg]], d["action"][lab[row_big]] = -1, a
    if c.via_slots:                                                         # what no sampled slot points at is poison
        off = np.ones(n, bool)
        off[slots] = False
        d["action"][off], d["reward"][off], d["done"][off] = 1 << 30, np.nan, 1
    d["w"] = rng.uniform(0.05, 1.0, b)
    return d, slots


def deep_payload(step):
    """-> the (slots, float32 delta) of an update step of DEEP_STEPS"""
    rng = np.random.default_rng(_seed(step.id))
    if step.id == "raise":
        return [5, DEEP_CAP - 5, 200000], np.float32([7.5, -0.5, 2.0])
    if step.id in ("one_first", "one_last"):
        return [0 if step.id == "one_first" else DEEP_CAP - 1], np.float32([0.3 if step.id == "one_first" else -4.25])
    slots = rng.integers(0, DEEP_CAP, step.rows)
    delta = (rng.uniform(0.01, 3.0, step.rows) * rng.choice([-1.0, 1.0], step.rows)).astype(np.float32)
    if step.rows == 1024:
        for first, last in FAR_PAIRS:
            slots[last] = slots[first]
        slots[1], slots[1022] = 0, DEEP_CAP - 1                             # both ends of the ring
        if step.id == "u1024_a":
            delta[FAR_PAIRS[0][0]] = -9.5                                   # the batch's largest |delta| is a loser's
        if step.id == "u1024_b":
            delta[LATE_ROW] = 12.25                                         # ... and the next one's sits in a late row
    else:
        slots[7], slots[300] = -1, DEEP_CAP2                                # never stored; their |delta| is not the largest
    return slots.tolist(), delta


def draws(c):
    if c.draws in ("zero", "one"):
        return [0.0 if c.draws == "zero" else 1.0 - 2.0 ** -53] * c.b
    if c.draws == "grid":
        return [0.0 if i % 2 == 0 else 0.5 for i in range(c.b)]
    u = np.random.default_rng(_seed(c.id)).random(c.b)
    u[0], u[-1] = 0.0, 1.0 - 2.0 ** -53
    return u.tolist()


def step_data(c):
    """the ring of a STEP_CASES row: states, labels, and what picks the batch (uniform: ``slots``; prioritised: the float32
    TD errors ``prime`` that give every stored transition its own priority, and the draws ``u``)"""
    rng = np.random.default_rng(_seed(c.id))
    cap = c.cap
    d = dict(cur=rng.standard_normal((cap, 4)).astype(np.float32), nxt=rng.standard_normal((cap, 4)).astype(np.float32),
             action=rng.integers(0, 2, cap).astype(np.int32))
    # rewards around +2, so that the TD errors share a sign (tests/test_gpu_per.py: the 1-wide head's bias gradient is
    # the sum of the g_b, and where they cancel its relative error measures the cancellation, not the kernel)
    d["reward"] = rng.standard_normal(cap) + 2.0
    d["done"] = (rng.random(cap) < 0.3).astype(np.uint8)
    d["slots"] = rng.permutation(cap)[:c.b].astype(np.int32)
    d["prime"] = rng.uniform(0.01, 3.0, cap).astype(np.float32)
    d["u"] = rng.random(c.b)
    return d


def device_priority(delta, eps=EPS):
    """the priorities the device forms from float32 TD errors"""
    return [float(abs(np.float32(x))) + eps for x in delta]


def host_deep_leaves(steps=DEEP_STEPS, bug=None):
    """-> [(step, leaves [cap2] float64, max_prio)] after every step: DEEP_STEPS replayed on the host"""
    leaves, max_prio, out = np.zeros(DEEP_CAP2), 1.0, []
    for step in steps:
        if step.kind == "add":
            for first, count in step.rows:
                leaves[first:first + count] = max_prio ** DEEP_ALPHA
        else:
            slots, delta = deep_payload(step)
            max_prio = B.apply_update(leaves, max_prio, slots, device_priority(delta), DEEP_ALPHA, bug)
        out.append((step, leaves.copy(), max_prio))
    return out


def host_tree_leaves(tree):
    """-> (leaves [cap2], stored transitions, beta) of a tree SAMPLE_CASES names, replayed on the host"""
    if tree == "deep":
        return host_deep_leaves()[-1][1], DEEP_CAP, DEEP_BETA
    if tree == "fresh":
        leaves = np.zeros(DEEP_CAP2)
        leaves[:FRESH_SIZE] = 1.0
        return leaves, FRESH_SIZE, DEEP_BETA
    leaves = np.zeros(8)
    B.apply_update(leaves, 1.0, range(8), device_priority(NEST_DELTA, NEST_EPS), NEST_ALPHA)
    return leaves, 8, DEEP_BETA


# ------------------------------------------------------------------------------------------------ xt_dqn_loss_w
@pytest.mark.parametrize("c", LOSS_CASES, ids=[c.id for c in LOSS_CASES])
def test_dqn_loss_w_launch_shapes_against_the_float32_twin_and_float64(L, c):
    d, slots = loss_data(c)
    b, a = c.b, c.a
    assert c.blocks == (b + 255) // 256
    rc, got = H.gpu_dqn_loss(d["logits"], d["value"], d["t_logits"], d["t_value"], d["o_logits"] if c.double else None,
                             d["o_value"] if c.double else None, d["action"], d["reward"], d["done"], GAMMA, c.dueling,
                             entry="xt_dqn_loss_w", slots=slots, weights=d["w"] if c.weighted else None, pad=B.PAD)
    assert rc == 0
    # what the launch does not own keeps its sentinels: the rows behind B, out[3], out behind the terms
    for k in ("dlogits", "dvalue", "y", "maxq"):
        assert np.isnan(got[k][b:]).all() and not np.isnan(got[k][:b]).any(), k
    assert (got["astar"][b:] == -1).all() and np.isnan(got["out"][3]) and np.isnan(got["out"][4 + 2 * b:]).all()
    assert got["out"][4 + 2 * b:].size == 2 * B.PAD + 1
    dev = {k: got[k][:b] for k in ("astar", "maxq", "y", "dlogits", "dvalue")}
    dev["terms"], dev["out3"] = got["out"][4:4 + 2 * b], got["out"][:3]
    twin = B.loss_twin32(d, c.dueling, c.double, GAMMA, c.weighted, slots)
    out3 = B.reduce_twin64(twin["terms"], b, a, twin["w32"])
    diffs = B.loss_bit_diffs(dev, twin, out3)
    ref, plain = B.loss_ref64(d, c.dueling, c.double, GAMMA, c.weighted, slots)
    errs = B.loss_f64_errors(dev, ref, plain, c.dueling)
    print("dqn branch loss", c.id, "blocks", c.blocks, "| bits differing", diffs, "| vs float64",
          {k: "{:.3g}/{:g}".format(e, bar) for k, (e, bar) in errs.items()})
    assert not any(diffs.values()), diffs
    assert B.within(errs), errs
    # the special rows are what the table says
    ties, row_neg, row_big = loss_rows(c)
    lab = np.arange(b) if slots is None else slots
    assert d["action"][lab[row_neg]] == -1 and d["action"][lab[row_big]] == a
    if a >= 2:
        pick = d["o_logits"] if c.double else d["t_logits"]
        assert [int(dev["astar"][r]) for r in ties] == [j for j, _ in tie_columns(a)]
        assert all((pick[r] == pick[r].max()).sum() == 2 for r in ties)


# ------------------------------------------------------------------------------------------------ trees, recorded
@pytest.fixture(scope="module")
def wide(golden_dir):
    return P.load_cases(golden_dir, "per_cases_wide.npz")


@pytest.fixture(scope="module")
def replayed(L, wide):
    """name -> (GpuTrees after the case's whole script, its read-back): each script runs once for the module"""
    done = {}

    def get(name):
        if name not in done:
            c = wide[name]
            t = P.GpuTrees(c.capacity, c.alpha)
            for step in c.steps():
                if step[0] == "add":
                    for first, count in step[1]:
                        assert t.add(first, count) == 0
                else:
                    sign = [1.0 if i % 2 else -1.0 for i in range(len(step[1]))]        # |delta| is what counts
                    assert t.update(step[1], np.float32(step[2]) * np.float32(sign), EPS, stride=2) == 0
            done[name] = (t, t.read())
        return done[name]
    return get


@pytest.mark.parametrize("name", WIDE_NAMES)
def test_trees_after_the_recorded_wide_adds_and_updates(wide, replayed, name):
    c = wide[name]
    _, (s, m, max_prio) = replayed(name)
    leaves, host_max = c.host_leaves(lambda p: float(np.float32(p)) + EPS)
    assert max_prio == host_max                                            # exactly
    got = np.asarray(s[c.cap2:])
    written = np.asarray(leaves) != 0.0
    assert written.sum() == c.n and not got[~written].any() and all(math.isinf(x) for x in np.asarray(m[c.cap2:])[~written])
    err = P.rel_err(got[written], np.asarray(leaves)[written])
    print("dqn branch wide trees", name, "leaves rel", err, "| update threads",
          sorted({B.workgroup(len(b[0])) for b in c.batches}))
    assert err <= 1e-12
    assert s[c.cap2:] == [0.0 if math.isinf(x) else x for x in m[c.cap2:]]  # both trees hold the same leaves
    P.assert_trees_follow_from_their_leaves(s, m)


def test_the_recorded_wide_batches_launch_every_workgroup_size_of_the_table(wide):
    sizes = {len(b[0]) for c in wide.values() for b in c.batches}
    assert sizes == {3, 30, 35, 40, 65, 90, 129, 200, 320, 700, 952, 1024}
    assert {B.workgroup(n) for n in sizes} == WIDE_WORKGROUPS
    far = 0
    for c in wide.values():
        for slots, _ in c.batches:
            last = {s: i for i, s in enumerate(slots)}
            far = max(far, max(last[s] - i for i, s in enumerate(slots)))
    assert far > 512                                                       # equal slots more than 512 rows apart


@pytest.mark.parametrize("name", WIDE_NAMES)
def test_sample_on_the_wide_device_trees_equals_the_restatement(wide, replayed, name):
    c = wide[name]
    t, (s, m, _) = replayed(name)
    rc, slots, w = t.sample(c.n, c.u, c.beta)
    assert rc == 0
    _, ref_slots, ref_w = P.sample(s, m, c.n, c.u, c.beta)
    assert slots.tolist() == ref_slots                                     # exactly
    err = P.rel_err(w, ref_w)
    print("dqn branch wide sample", name, "threads", B.workgroup(c.b), "weights rel", err, "| min/total", m[1] / s[1],
          "| equal to the recorded indices:", slots.tolist() == c.idx)
    assert err <= 1e-12
    assert 0 <= slots.min() and slots.max() < c.n
    if name == "w330_b320":
        assert [c.u[i] for i in (0, 1, 2, -1)] == [0.0, 1.0 - 2.0 ** -53, 0.0, 1.0 - 2.0 ** -53] and slots[0] == 0


def test_the_recorded_cases_lie_above_the_p_min_floor(wide, replayed):
    above = []
    for name in WIDE_NAMES:
        _, (s, m, _) = replayed(name)
        above.append(m[1] / s[1] > 1e-5)
    assert any(above)                                                      # (the deep trees lie below it)


# ------------------------------------------------------------------------------------------------ trees, deep
@pytest.fixture(scope="module")
def deep(L):
    """DEEP_STEPS on the device -> ([(step, sum, min, max_prio) after every step], the GpuTrees)"""
    t = P.GpuTrees(DEEP_CAP, DEEP_ALPHA)
    assert t.cap2 == DEEP_CAP2
    snaps = []
    for step in DEEP_STEPS:
        if step.kind == "add":
            for first, count in step.rows:
                assert t.add(first, count) == 0
        else:
            slots, delta = deep_payload(step)
            assert len(slots) == step.rows and B.workgroup(step.rows) == step.threads
            assert t.update(slots, delta, EPS, stride=3) == 0
        snaps.append((step,) + t.read_np())
    return snaps, t


@pytest.mark.parametrize("k", range(len(DEEP_STEPS)), ids=[s.id for s in DEEP_STEPS])
def test_deep_trees_follow_from_their_leaves_after_every_step(deep, k):
    step, s, m, max_prio = deep[0][k]
    _, leaves, host_max = host_deep_leaves(DEEP_STEPS[:k + 1])[-1]
    assert max_prio == host_max                                            # the exact running maximum
    got, got_min = s[DEEP_CAP2:], m[DEEP_CAP2:]
    written = leaves != 0.0
    assert written.sum() == DEEP_CAP and not got[~written].any() and np.isinf(got_min[~written]).all()
    err = P.rel_err(got[written], leaves[written])
    print("dqn branch deep", step.id, "threads", step.threads, "leaves rel", err, "| max_prio", max_prio)
    assert err <= 1e-12
    assert np.array_equal(got[written], got_min[written])
    P.assert_trees_follow_from_their_leaves_np(s, m)
    if k:                                                                  # the step changed what it should, and only that
        before = deep[0][k - 1][1][DEEP_CAP2:]
        if step.kind == "add":
            touched = np.zeros(DEEP_CAP2, bool)
            for first, count in step.rows:
                touched[first:first + count] = True
        else:
            slots = np.asarray(deep_payload(step)[0])
            touched = np.zeros(DEEP_CAP2, bool)
            touched[slots[(slots >= 0) & (slots < DEEP_CAP2)]] = True
        assert np.array_equal(got[~touched], before[~touched]) and (got[touched] != before[touched]).any()


@pytest.fixture(scope="module")
def sample_trees(L, deep):
    """tree name -> (GpuTrees, sum and min as lists of Python floats, beta)"""
    snaps, t = deep
    out = {"deep": (t, snaps[-1][1].tolist(), snaps[-1][2].tolist(), DEEP_BETA)}
    fresh = P.GpuTrees(DEEP_CAP, DEEP_ALPHA)
    assert fresh.add(0, FRESH_SIZE) == 0
    nest = P.GpuTrees(8, NEST_ALPHA)
    assert nest.add(0, 8) == 0 and nest.update(list(range(8)), np.float32(NEST_DELTA), NEST_EPS) == 0
    for name, tr in (("fresh", fresh), ("nest", nest)):
        s, m, _ = tr.read_np()
        P.assert_trees_follow_from_their_leaves_np(s, m)
        out[name] = (tr, s.tolist(), m.tolist(), DEEP_BETA)
    return out


@pytest.mark.parametrize("c", SAMPLE_CASES, ids=[c.id for c in SAMPLE_CASES])
def test_sample_on_deep_trees_equals_the_restatement(sample_trees, c):
    t, s, m, beta = sample_trees[c.tree]
    u = draws(c)
    assert B.workgroup(c.b) == c.threads and len(u) == c.b
    rc, slots, w = t.sample(c.size, u, beta)
    assert rc == 0
    _, ref_slots, ref_w = P.sample(s, m, c.size, u, beta)
    assert slots.tolist() == ref_slots                                     # exactly
    err = P.rel_err(w, ref_w)
    ratio = m[1] / s[1]
    print("dqn branch sample", c.id, "threads", c.threads, "weights rel", err, "| min/total", ratio, "| slots",
          ref_slots[:3], "..", ref_slots[-1])
    assert err <= 1e-12
    assert 0 <= slots.min() and slots.max() < c.size
    if c.tree in ("deep", "fresh"):
        assert ratio < 1e-5                                                # the floor branch of p_min
    if c.draws == "grid":                                                  # a mass on a boundary belongs to the leaf after it
        assert ref_slots == [128 * i + (64 if i % 2 else 0) for i in range(c.b)]
    if c.draws in ("zero", "edges"):
        assert ref_slots[0] == 0


# ------------------------------------------------------------------------------------------------ steps at B = 320
def _spec_pair(a_dim, dueling):
    from xingtian_amd.model import netspec
    return netspec.dqn_mlp((4,), a_dim, 32, 1, dueling), H.oracle_spec("mlp", (4,), a_dim, 32, 1)


def _step_errors(got_loss, grads, ref, spec, ospec):
    """-> (relative loss error, {Keras name: relative 2-norm error of the gradient tensor})"""
    loss_err = abs(got_loss - ref["loss"]) / max(1.0, abs(ref["loss"]))
    errs = {}
    for h, o in H.name_map(spec, ospec).items():
        r = np.asarray(ref["grads"][o], np.float64)
        errs[h] = float(np.linalg.norm(np.asarray(grads[h], np.float64).reshape(r.shape) - r) / (np.linalg.norm(r) + 1e-30))
    return float(loss_err), errs


def _assert_step(c, got_loss, grads, ref, ref32, spec, ospec):
    """the bars of tests/test_gpu_dqn.py and tests/test_gpu_per.py: 1e-4 on the loss, 1e-5 on every gradient tensor;
    the float32 oracle's own figures are printed next to the device's"""
    loss_err, errs = _step_errors(got_loss, grads, ref, spec, ospec)
    loss32, errs32 = _step_errors(float(ref32["loss"]), {h: ref32["grads"][o] for h, o in H.name_map(spec, ospec).items()},
                                  ref, spec, ospec)
    print("dqn branch step", c.id, "loss", got_loss, float(ref["loss"]), "rel {:.3g} (oracle32 {:.3g})".format(loss_err, loss32),
          "| gradient tensors (device, oracle32):", {h: "{:.3g}, {:.3g}".format(errs[h], errs32[h]) for h in errs})
    assert loss_err <= 1e-4, (got_loss, ref["loss"])
    for h, e in errs.items():
        assert e <= 1e-5, (h, e)


@pytest.mark.parametrize("c", STEP_CASES, ids=[c.id for c in STEP_CASES])
def test_net_dqn_steps_at_320_rows_against_float64(L, c):
    from xingtian_amd.model.hip_net import HipActorCritic
    a_dim, alpha, beta, b, cap = 2, 0.6, 0.4, c.b, c.cap
    spec, ospec = _spec_pair(a_dim, c.dueling)
    d = step_data(c)
    cur, nxt, action, reward, done = (d[k] for k in ("cur", "nxt", "action", "reward", "done"))
    p_on, p_tg = H.seeded_params(ospec, 1, c.dueling), H.seeded_params(ospec, 2, c.dueling)
    net, target = HipActorCritic(spec, max_batch=b, seed=0), HipActorCritic(spec, max_batch=b, seed=0)
    net.set_weights(H.to_keras_names(spec, ospec, p_on))
    target.set_weights(H.to_keras_names(spec, ospec, p_tg))
    target_before = target.params.clone()
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    orc = H.DqnOracle(ospec, p_on, p_tg, c.dueling, c.double, GAMMA, lr=3e-4, dtype=np.float64)
    orc32 = H.DqnOracle(ospec, p_on, p_tg, c.dueling, c.double, GAMMA, lr=3e-4, dtype=np.float32)
    if not c.per:
        slots = d["slots"]
        out = net.dqn_step(target, net.to_device_obs(cur), net.to_device_obs(nxt), up(slots), up(action), up(reward),
                           up(done), GAMMA, c.dueling, c.double)
        torch.cuda.synchronize()
        batch = (cur[slots], nxt[slots], action[slots], reward[slots], done[slots])
        ref, ref32 = orc.step(*batch, apply=False), orc32.step(*batch, apply=False)
        _assert_step(c, float(out.cpu().numpy()[0]), net.grads_dict(), ref, ref32, spec, ospec)
        assert torch.equal(target.params, target_before) and not bool(target.grads.any())
        return
    t = P.GpuTrees(cap, alpha)                                             # a full ring of distinct priorities
    assert t.add(0, cap) == 0
    assert t.update(list(range(cap)), d["prime"], EPS) == 0
    s0, m0, max0 = t.read()
    u = d["u"]
    terms = torch.full((2 * b,), float("nan"), dtype=torch.float32, device="cuda")
    per = dict(size=cap, u=up(u), sum_tree=t.sum, min_tree=t.min, max_prio=t.max_prio, alpha=alpha, beta=beta, eps=EPS,
               terms_out=terms)
    out = net.dqn_step(target, net.to_device_obs(cur), net.to_device_obs(nxt), None, up(action), up(reward), up(done),
                       GAMMA, c.dueling, c.double, per=per)
    torch.cuda.synchronize()
    # the draw: the restatement on the tree as it was before the step
    _, ref_slots, ref_w = P.sample(s0, m0, cap, u.tolist(), beta)
    slots, w = net.per_slots[:b].cpu().numpy(), net.per_weights[:b].cpu().numpy()
    assert slots.tolist() == ref_slots and P.rel_err(w, ref_w) <= 1e-12
    assert len(set(ref_slots)) < b                                         # equal slots within the batch
    batch = (cur[slots], nxt[slots], action[slots], reward[slots], done[slots])
    ref, ref32 = orc.step(*batch, w, apply=False), orc32.step(*batch, w, apply=False)
    _assert_step(c, float(out.cpu().numpy()[0]), net.grads_dict(), ref, ref32, spec, ospec)
    delta = terms.cpu().numpy()[0::2]
    assert H.rel_max(delta, ref["delta"]) <= 1e-5
    # the write-back: the sampled leaves take (|delta| + eps) ** alpha of the device's own terms, the last occurrence of
    # a slot wins, every other leaf is untouched, the ancestors follow
    s1, m1, max1 = t.read()
    leaves = np.array(s0[t.cap2:])
    assert max1 == B.apply_update(leaves, max0, slots, device_priority(delta), alpha)
    got = np.array(s1[t.cap2:])
    sampled = np.zeros(t.cap2, bool)
    sampled[slots] = True
    assert P.rel_err(got[sampled], leaves[sampled]) <= 1e-12 and np.array_equal(got[~sampled], leaves[~sampled])
    assert s1[t.cap2:t.cap2 + cap] == m1[t.cap2:t.cap2 + cap]
    P.assert_trees_follow_from_their_leaves(s1, m1)
    assert torch.equal(target.params, target_before) and not bool(target.grads.any())     # the target net is forward only
