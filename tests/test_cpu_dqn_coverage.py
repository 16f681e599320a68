"""CPU checks of the case tables of tests/test_gpu_dqn_branch.py (the TD / MSE head of csrc/xt_dqn.hip and the priority
trees of csrc/xt_per.hip): tests/golden/per_cases_wide.npz holds the wide cases and the restatement reproduces them bit
for bit, ``build_trees_np`` is ``build_trees``, the tables cover every axis value, block count and workgroup size they
claim, and the comparisons the GPU tests assert with reject a deliberately wrong twin.  A launch shape dropped from a
table, or a comparison that stopped biting, fails here, on any box."""
import hashlib
import importlib.util
import os

import numpy as np
import pytest

import dqn_branch_helpers as B
import per_helpers as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE_NAMES = ("c5", "c37", "c707", "c1000", "c64", "c37_alpha1", "c37_beta1", "c64_edge")
WIDE = {"w1000_b1024": (1000, (700, 650), 1024, 0.6, 0.4, False), "w330_b320": (330, (200, 250), 320, 0.6, 0.4, True),
        "w140_b129": (140, (90, 40), 129, 1.0, 1.0, False), "w100_b65": (100, (100, 30), 65, 0.6, 0.4, False)}
BASE_SHA256 = "b2fbe109d6a3505479f5572f8bfb01c9d6d4be901fe514e4626a4cdc636e4974"


@pytest.fixture(scope="module")
def T():
    """the GPU module imported for its tables and data only (no test of it runs)"""
    spec = importlib.util.spec_from_file_location("_dqn_branch_cases", os.path.join(ROOT, "tests", "test_gpu_dqn_branch.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def wide(golden_dir):
    return P.load_cases(golden_dir, "per_cases_wide.npz")


@pytest.fixture(scope="module")
def recorded(golden_dir, wide):
    """all twelve recorded cases"""
    both = dict(P.load_cases(golden_dir))
    both.update(wide)
    assert sorted(both) == sorted(BASE_NAMES + tuple(WIDE))
    return both


# ------------------------------------------------------------------------------------------------ golden
def test_the_wide_golden_holds_the_four_cases_of_the_table_and_the_first_golden_is_untouched(golden_dir, wide, T):
    assert sorted(wide) == sorted(WIDE) == sorted(T.WIDE_NAMES)
    for name, (capacity, msg_lens, b, alpha, beta, edge) in WIDE.items():
        c = wide[name]
        assert (c.capacity, tuple(c.msg_lens), c.b, c.alpha, c.beta) == (capacity, msg_lens, b, alpha, beta), name
        assert c.n == min(capacity, sum(msg_lens)) and len(c.u) == b and max(c.idx) < c.n
        edges = [c.u[i] for i in (0, 1, 2, -1)] == [0.0, 1.0 - 2.0 ** -53, 0.0, 1.0 - 2.0 ** -53]
        assert edges == edge, name
    assert wide["w140_b129"].n < wide["w140_b129"].capacity                # N < capacity and N = capacity
    assert wide["w330_b320"].idx[-1] == 329                                # slot N - 1, by the 1 - 2^-53 draw
    sizes = sorted({len(b[0]) for c in wide.values() for b in c.batches})
    assert sizes == [3, 30, 35, 40, 65, 90, 129, 200, 320, 700, 952, 1024]
    assert {B.workgroup(n) for n in sizes} == {64, 128, 192, 256, 320, 704, 960, 1024} == T.WIDE_WORKGROUPS
    dup = max(len(b[0]) - len(set(b[0])) for c in wide.values() for b in c.batches)
    assert dup == 397                                                      # equal slots within one batch
    base, new = os.path.join(golden_dir, "per_cases.npz"), os.path.join(golden_dir, "per_cases_wide.npz")
    assert os.path.getsize(new) < os.path.getsize(base) == 165777
    with open(base, "rb") as f:
        assert hashlib.sha256(f.read()).hexdigest() == BASE_SHA256


@pytest.mark.parametrize("name", sorted(WIDE))
def test_restatement_reproduces_the_wide_cases_bit_for_bit(wide, name):
    c = wide[name]
    s, m = P.build_trees(c.leaves.tolist())
    assert s == c.sum.tolist() and m == c.min.tolist()                     # both full trees
    p_total, slots, weights = P.sample(s, m, c.n, c.u, c.beta)
    assert p_total == c.p_total and slots == c.idx
    assert P.rel_err(weights, c.w) == 0.0
    leaves, max_prio = c.host_leaves()
    assert max_prio == c.max_prio                                          # exact: a maximum of recorded values
    written = c.leaves != 0.0
    assert written.sum() == c.n and not np.asarray(leaves)[~written].any()
    assert P.rel_err(np.asarray(leaves)[written], c.leaves[written]) <= 1e-12
    again, again_max = B.replay_case(c)                                    # the twin the wrong variants derive from
    assert again.tolist() == leaves and again_max == max_prio


@pytest.mark.parametrize("name", sorted(BASE_NAMES + tuple(WIDE)))
def test_build_trees_np_is_build_trees_bit_for_bit(recorded, name):
    c = recorded[name]
    s, m = P.build_trees(c.leaves.tolist())
    s_np, m_np = P.build_trees_np(c.leaves)
    assert s_np.dtype == m_np.dtype == np.float64
    assert s_np.tolist() == s == c.sum.tolist() and m_np.tolist() == m == c.min.tolist()
    # given min leaves, and a tree of one leaf
    s2, m2 = P.build_trees_np(c.leaves, np.asarray(P.min_leaves(c.leaves.tolist())))
    assert s2.tolist() == s and m2.tolist() == m
    one = P.build_trees_np([2.5])
    assert one[0].tolist() == [0.0, 2.5] and one[1].tolist() == [P.INF, 2.5]


def test_build_trees_np_on_a_deep_tree_equals_the_list_builder(T):
    leaves = T.host_deep_leaves()[-1][1][:1 << 14]                         # 14 levels: the list builder stays quick
    assert (leaves != 0.0).all()
    s, m = P.build_trees(leaves.tolist())
    s_np, m_np = P.build_trees_np(leaves)
    assert s_np.tolist() == s and m_np.tolist() == m


# ------------------------------------------------------------------------------------------------ coverage
def test_loss_table_covers_every_axis_value_and_block_count(T):
    cases = T.LOSS_CASES
    assert len(cases) == len({c.id for c in cases}) == 6 * 16
    assert {(c.b, c.a) for c in cases} == {(255, 4), (256, 4), (257, 1), (257, 18), (513, 64), (1000, 2)}
    for shape in {(c.b, c.a) for c in cases}:                              # the full cross of the four switches per shape
        mine = {(c.dueling, c.double, c.weighted, c.via_slots) for c in cases if (c.b, c.a) == shape}
        assert len(mine) == 16, shape
    assert all(c.blocks == (c.b + 255) // 256 for c in cases)
    assert {c.blocks for c in cases} == {1, 2, 3, 4}                       # 1, 2 and 3+ blocks / reduction strides
    for c in cases:
        d, slots = T.loss_data(c)
        ties, row_neg, row_big = T.loss_rows(c)
        lab = np.arange(c.b) if slots is None else slots
        assert d["action"][lab[row_neg]] == -1 and d["action"][lab[row_big]] == c.a
        inside = np.delete(d["action"][lab], [row_neg, row_big])
        assert inside.min() >= 0 and inside.max() < c.a
        if c.b > 256:
            assert row_neg >= 256 and (row_big >= 256 or c.b == 257)       # (B = 257 has one row in its second block)
            assert ties[0] < 256 <= ties[1]
        done = d["done"][lab]
        assert {0, 1, 255} == set(done.tolist())                           # mixed, both truthy values
        if c.a >= 2:
            for k in ("t_logits", "o_logits"):
                assert all((d[k][r] == d[k][r].max()).sum() == 2 for r in ties), c.id
        assert (np.asarray(d["w"], np.float32).astype(np.float64) != d["w"]).all()         # float64 weights that round
        if c.via_slots:
            assert len(d["reward"]) == 3 * c.b and len(set(slots.tolist())) == c.b - 2 and slots[c.b - 7] == slots[5]
            off = np.ones(3 * c.b, bool)
            off[slots] = False
            assert off.sum() == 2 * c.b + 2 and np.isnan(d["reward"][off]).all() and (d["action"][off] == 1 << 30).all()
            assert not np.isnan(d["reward"][slots]).any() and (slots != np.arange(c.b)).any()
        else:
            assert slots is None and len(d["reward"]) == c.b


def test_tree_tables_cover_every_workgroup_size_depth_and_both_sides_of_the_floor(T, recorded):
    threads = {B.workgroup(len(b[0])) for name in T.WIDE_NAMES for b in recorded[name].batches}
    assert threads == {64, 128, 192, 256, 320, 704, 960, 1024}             # every multiple of 64 the wide batches give
    steps = T.DEEP_STEPS
    assert T.DEEP_CAP == 400000 and T.DEEP_CAP2 == P.cap2_of(T.DEEP_CAP) == 1 << 19
    assert [s.id for s in steps][0] == "fill" and steps[0].rows == ((0, 400000),)
    assert any(s.kind == "add" and s.rows == ((399990, 10), (0, 15)) for s in steps)       # the wrapping message
    assert [s.rows for s in steps if s.kind == "update"].count(1024) == 3
    for s in steps:
        if s.kind != "update":
            continue
        slots, delta = T.deep_payload(s)
        assert len(slots) == len(delta) == s.rows and B.workgroup(s.rows) == s.threads and delta.dtype == np.float32
        if s.rows == 1024:
            assert all(slots[i] == slots[j] and j - i > 512 for i, j in T.FAR_PAIRS)
            assert min(slots) == 0 and max(slots) == T.DEEP_CAP - 1
        if s.id == "u320_outside":
            assert -1 in slots and T.DEEP_CAP2 in slots
            inside = [x for x in slots if x not in (-1, T.DEEP_CAP2)]
            assert 0 <= min(inside) and max(inside) < T.DEEP_CAP
            assert max(abs(delta[slots.index(-1)]), abs(delta[slots.index(T.DEEP_CAP2)])) < np.abs(delta).max()
    assert [T.deep_payload(s)[0] for s in steps if s.rows == 1] == [[0], [T.DEEP_CAP - 1]]
    first = T.deep_payload(steps[3])
    assert steps[3].id == "u1024_a" and int(np.abs(first[1]).argmax()) == T.FAR_PAIRS[0][0]  # the largest |delta|: a loser's
    second = T.deep_payload(steps[4])                                      # ... and the running maximum rises in a row >= 512
    assert steps[4].id == "u1024_b" and int(np.abs(second[1]).argmax()) == T.LATE_ROW >= 512
    assert np.abs(second[1]).max() > np.abs(first[1]).max() > 7.5
    # sampling: B in {1, 320, 1024} on the deep tree at 400 000 and on the fresh one at 250 000, both edge draws
    S = T.SAMPLE_CASES
    for tree, size in (("deep", 400000), ("fresh", 250000)):
        assert {c.b for c in S if c.tree == tree and c.size == size} == {1, 320, 1024}, tree
        u = [x for c in S if c.tree == tree and c.size == size for x in T.draws(c)]
        assert 0.0 in u and 1.0 - 2.0 ** -53 in u
    assert all(B.workgroup(c.b) == c.threads for c in S) and {c.threads for c in S} == {64, 320, 1024}
    # both sides of the p_min floor
    ratios = {}
    for tree in ("deep", "fresh"):
        s, m = P.build_trees_np(T.host_tree_leaves(tree)[0])
        ratios[tree] = m[1] / s[1]
        assert ratios[tree] < 1e-5, tree
    above = [name for name in T.WIDE_NAMES if recorded[name].min[1] / recorded[name].sum[1] > 1e-5]
    assert above
    # the steps: B = 320 of a 600-row ring, prioritised and uniform, dueling + double and plain
    assert {(c.per, c.dueling, c.double) for c in T.STEP_CASES} == {(p, x, x) for p in (True, False) for x in (True, False)}
    assert all((c.b, c.cap, c.threads) == (320, 600, 320) for c in T.STEP_CASES)
    for c in T.STEP_CASES:
        d = T.step_data(c)
        if c.per:                                                          # distinct priorities; equal slots in the draw
            leaves = np.zeros(P.cap2_of(c.cap))
            B.apply_update(leaves, 1.0, range(c.cap), T.device_priority(d["prime"]), 0.6)
            assert len(set(leaves[:c.cap].tolist())) == c.cap
            s, m = P.build_trees_np(leaves)
            _, slots, _ = P.sample(s.tolist(), m.tolist(), c.cap, d["u"].tolist(), 0.4)
            assert len(set(slots)) < c.b
        else:
            assert len(set(d["slots"].tolist())) == c.b


# ------------------------------------------------------------------------------------------------ the comparisons bite
def test_loss_comparisons_reject_every_wrong_twin(T):
    """bit for bit: every wrong twin, at every case it applies to; against float64 at the bars: the ones that are wrong
    by more than a rounding"""
    applies = {"last_max": lambda c: c.a >= 2, "gamma_f32": lambda c: True, "w_f64": lambda c: c.weighted,
               "w_by_slot": lambda c: c.weighted and c.via_slots, "no_clamp": lambda c: True,
               "div_b": lambda c: c.a >= 2, "first_stride": lambda c: c.b > 256}
    rounding_only = ("gamma_f32", "w_f64")
    grads = ("dlogits", "dvalue")                  # (A = 1 with the dueling head: dlogits is g * (1 - 1), the gradient is dvalue's)
    where = {"last_max": ("astar",), "gamma_f32": ("y",), "w_f64": grads, "w_by_slot": grads, "no_clamp": ("terms",),
             "div_b": grads, "first_stride": ("out3",)}
    applied = dict.fromkeys(applies, 0)
    for c in T.LOSS_CASES:
        d, slots = T.loss_data(c)
        args = (d, c.dueling, c.double, T.GAMMA, c.weighted, slots)
        twin = B.loss_twin32(*args)
        out3 = B.reduce_twin64(twin["terms"], c.b, c.a, twin["w32"])
        ref, plain = B.loss_ref64(*args)
        good = dict(twin, out3=out3)
        assert not any(B.loss_bit_diffs(good, twin, out3).values())
        errs = B.loss_f64_errors(good, ref, plain, c.dueling)
        assert B.within(errs), (c.id, errs)
        # ... and the float32 twin itself lies well inside the bars (the ordered sum against float64 included)
        assert all(e <= 0.25 * bar for e, bar in errs.values()), (c.id, errs)
        for bug, ok in applies.items():
            if not ok(c):
                continue
            applied[bug] += 1
            if bug in B.REDUCE_BUGS:
                wrong = dict(twin, out3=B.reduce_twin64(twin["terms"], c.b, c.a, twin["w32"], bug))
            else:
                w = B.loss_twin32(*args, bug=bug)
                wrong = dict(w, out3=B.reduce_twin64(w["terms"], c.b, c.a, w["w32"]))
            diffs = B.loss_bit_diffs(wrong, twin, out3)
            assert any(diffs[k] > 0 for k in where[bug]), (c.id, bug, diffs)
            if bug not in rounding_only:
                assert not B.within(B.loss_f64_errors(wrong, ref, plain, c.dueling)), (c.id, bug)
    assert applied == {"last_max": 80, "gamma_f32": 96, "w_f64": 48, "w_by_slot": 24, "no_clamp": 96, "div_b": 80,
                       "first_stride": 64}
    assert set(applies) == set(B.LOSS_BUGS + B.REDUCE_BUGS)


def test_sample_comparisons_reject_every_wrong_twin(T, recorded):
    """slots exactly, weights to 1e-12: each wrong twin of the sampling is rejected by at least one case of the tables"""
    rejected = {bug: [] for bug in B.SAMPLE_BUGS}
    runs = [(name, c.sum.tolist(), c.min.tolist(), c.n, c.u, c.beta) for name, c in sorted(recorded.items())]
    built = {}
    for c in T.SAMPLE_CASES:
        if c.tree not in built:
            leaves, _, beta = T.host_tree_leaves(c.tree)
            s, m = P.build_trees_np(leaves)
            built[c.tree] = (s.tolist(), m.tolist(), beta)
        s, m, beta = built[c.tree]
        runs.append((c.id, s, m, c.size, T.draws(c), beta))
    for name, s, m, n, u, beta in runs:
        good = P.sample(s, m, n, u, beta)
        again = B.sample_twin(s, m, n, u, beta)
        assert again[0] == good[0] and again[1] == good[1] and again[2] == good[2], name   # the twin is the restatement
        for bug in B.SAMPLE_BUGS:
            _, slots, w = B.sample_twin(s, m, n, u, beta, bug)
            if slots != good[1] or P.rel_err(w, good[2]) > 1e-12:
                rejected[bug].append(name)
    new = {c.id for c in T.SAMPLE_CASES} | set(T.WIDE_NAMES)
    for bug, names in rejected.items():
        assert new & set(names), (bug, names)
    assert "nest_b1_one" in rejected["left_nested"] and "fresh_b1024_grid" in rejected["descent_ge"]
    assert {"deep_b1024", "fresh_b320"} <= set(rejected["no_floor"]) and not set(rejected["no_floor"]) & set(recorded)
    # the nesting case is what its comment says: 2^53 + 2 from the right, 2^53 from the left, leaf 4 or leaf 0
    s, m, beta = built["nest"]
    one = [1.0 - 2.0 ** -53]
    assert B.sample_twin(s, m, 8, one, beta)[:2] == (2.0 ** 53 + 2.0, [4])
    assert B.sample_twin(s, m, 8, one, beta, "left_nested")[:2] == (2.0 ** 53, [0])


def test_update_comparisons_reject_every_wrong_twin(T, wide):
    """leaves to 1e-12 and max_prio exactly: a first-occurrence-wins write-back and a maximum over the winners only"""
    rejected = {bug: [] for bug in B.UPDATE_BUGS}
    for name in T.WIDE_NAMES:
        c = wide[name]
        leaves, max_prio = B.replay_case(c)
        for bug in B.UPDATE_BUGS:
            wrong, wrong_max = B.replay_case(c, bug=bug)
            if wrong_max != max_prio or P.rel_err(wrong[leaves != 0.0], leaves[leaves != 0.0]) > 1e-12:
                rejected[bug].append(name)
    good = T.host_deep_leaves()
    for bug in B.UPDATE_BUGS:
        for (step, leaves, max_prio), (_, wrong, wrong_max) in zip(good, T.host_deep_leaves(bug=bug)):
            if wrong_max != max_prio or P.rel_err(wrong[leaves != 0.0], leaves[leaves != 0.0]) > 1e-12:
                rejected[bug].append(step.id)
    assert set(T.WIDE_NAMES) <= set(rejected["first_dup"]) and "u1024_a" in rejected["first_dup"]
    assert "u1024_a" in rejected["max_winners"]                            # the largest |delta| of the batch is a loser's
