"""The knob matrix: a pairwise covering array over every kernel-selection knob, shared by tests/test_cpu_knob_matrix.py
and tests/test_gpu_knob_matrix.py (a plain module, no fixtures).

FACTORS are the 34 words of ``xt_tuning`` (include/xt_mi355x.h) and the two later switches, ``xt_net_set_fwd_fuse12_flat``
(per net) and ``xt_bwd_dense_lean_set`` (process-wide): the default first, then the other values the knob's description
documents.  ``covering_array`` builds, by a seeded greedy construction, a set of rows in which every pair of
(factor, value) x (factor, value) occurs at least once; row 0 is all defaults.

BASES are the nets the matrix runs on, described with the machinery of tests/net_zoo_helpers.py (its rows, seeds, inputs,
float64 reference and bars).  ``expected_words`` restates, for a (base, row), the conditions under which the step takes
each of the forms its report has a word for (xingtian_amd/csrc/xt_net.hip and the launchers it leans on), with every knob
those conditions read; ``conv12_envelope_open`` restates ``conv12_valid_envelope`` (xt_conv1.hip), its eight knob
conditions included.  At the knobs of a zoo row both reduce to ``net_zoo_helpers.plan_from_conditions`` (``zoo_facts``;
the CPU test holds every zoo row's literals against it)."""
from collections import OrderedDict

import numpy as np

import net_zoo_helpers as Z

# ------------------------------------------------------------------------------------------------ factors
# (default first.  The block-count targets' second values change a split count at the matrix's shapes, see
# ``split_count_changes``: fwd_split_target 16 also stops the 33-frame PpoCnn's conv2 from splitting K, which opens the
# fused conv1 -> conv2 launch at that batch.)
FACTORS = OrderedDict([
    ("bf16x6", (1, 0)), ("dgrad_all_classes", (1, 0)), ("dgrad_tile64", (1, 0)), ("dgrad_halo", (1, 0)),
    ("bwd_own_instance", (1, 0)), ("bwd_fit_slots", (768, 0)), ("conv1_bf16x3", (1, 0)), ("conv1_flat", (1, 0)),
    ("conv1_waves", (8, 4)), ("fwd_two_groups", (1, 0)), ("direct", (1, 0)), ("direct_fwd", (1, 0)),
    ("direct_dgrad", (1, 0)), ("direct_all", (0, 1)), ("direct_waves", (1536, 256)), ("direct_max_waves", (8, 4)),
    ("direct_tile64_tiles", (3072, 64)), ("fwd_split_target", (256, 16)), ("wgrad_split_target", (512, 64)),
    ("reduce_z_lanes", (8, 16, 1)), ("defer_splitk", (1, 0)), ("finalize_ticket", (0, 1)), ("fwd_tiled_valid", (1, 0)),
    ("wgrad_rows", (4, 0, 1, 2)), ("fwd_prefetch_all", (0, 1)), ("bwd_deep_prefetch", (1, 0)), ("fwd_four_groups", (1, 0)),
    ("reduce_deep_lanes", (128, 0)), ("fwd_xcd_chunk", (1, 0)), ("tail_overlap", (0, 1, 2, 3)), ("tail_fused", (0, 1)),
    ("dense_wgrad_x6", (1, 0, 2)), ("fwd_fuse12", (0, 4096)), ("bwd_fuse21", (0, 1, 2)),
    ("fwd_fuse12_flat", (1, 0)), ("bwd_dense_lean", (1, 0)),
])
SWITCHES = ("fwd_fuse12_flat", "bwd_dense_lean")
TUNING_NAMES = [n for n in FACTORS if n not in SWITCHES]
DEFAULTS = OrderedDict((n, v[0]) for n, v in FACTORS.items())
ARRAY_SEED, ARRAY_CANDIDATES, MAX_ROWS = 7, 48, 32


class _Rng(object):
    """xorshift64: the array must not depend on the random streams of a library version"""

    def __init__(self, seed):
        self.s = ((seed + 1) * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF or 1

    def below(self, n):
        x = self.s
        x ^= (x << 13) & 0xFFFFFFFFFFFFFFFF
        x ^= x >> 7
        x ^= (x << 17) & 0xFFFFFFFFFFFFFFFF
        self.s = x
        return (x >> 11) % n

    def shuffle(self, a):
        for i in range(len(a) - 1, 0, -1):
            j = self.below(i + 1)
            a[i], a[j] = a[j], a[i]


def all_pairs(factors=FACTORS):
    names = list(factors)
    return {(i, a, j, b) for i in range(len(names)) for j in range(i + 1, len(names))
            for a in range(len(factors[names[i]])) for b in range(len(factors[names[j]]))}


def _row_pairs(row):
    return {(i, row[i], j, row[j]) for i in range(len(row)) for j in range(i + 1, len(row))}


def pinned_rows():
    """the partial rows the array starts with, behind row 0 (knob -> value; everything else is the greedy rule's).  A pairwise
    row sets half of the knobs of any conjunction to their other value, so a form that needs six or eight knobs at once is
    almost never one step from being taken, or taken, in it -- and that is where a dropped or a wrong condition shows:
      1 .. 8  the edge of the fused conv1 -> conv2 envelope: ONE of the eight knobs ``conv12_valid_envelope`` pins at its
              other value, the other seven at their defaults;
      9       bwd_fuse21 = 2 taken behind the fused conv1 -> conv2 launch (the third writer of the sign mask), which the
              split target 16 opens on 33 frames too;
      10      bwd_fuse21 = 1 (its threshold form, 255 frames) behind the flat first layer, the fused launch switched off;
      11, 12  both one-launch conv1 -> conv2 forwards (PpoCnn's, open on 33 frames through the split target 16, and
              ImpalaCnnOpt's, fwd_fuse12) together with tail_overlap 3 and 2 honoured (no finalize_ticket): these launches
              read the second layer's weights early, while the side stream may still hold the previous step's Adam share --
              the trains of check (f) cross steps with that share pending."""
    rows = [OrderedDict((e, FACTORS[e][int(e == x)]) for e in ENVELOPE_KNOBS) for x in ENVELOPE_KNOBS]
    inside = OrderedDict((e, FACTORS[e][0]) for e in ENVELOPE_KNOBS)
    taken = OrderedDict(inside, dgrad_all_classes=1, wgrad_rows=4)
    rows.append(OrderedDict(taken, bwd_fuse21=2, fwd_split_target=16, fwd_fuse12_flat=1))
    rows.append(OrderedDict(taken, bwd_fuse21=1, fwd_fuse12_flat=0))
    for tail in (3, 2):
        rows.append(OrderedDict(inside, fwd_split_target=16, fwd_fuse12_flat=1, fwd_fuse12=4096, tail_overlap=tail,
                                finalize_ticket=0))
    return rows


def covering_array(factors=FACTORS, seed=ARRAY_SEED, candidates=ARRAY_CANDIDATES, pinned=None):
    """-> list of OrderedDict(knob -> value).  Greedy, one row at a time: each candidate starts from a pair no row has yet,
    walks the other factors in a shuffled order and gives each the value that covers the most open pairs with the factors
    already set; the candidate that covers the most open pairs becomes the row.

    ``pinned`` (default ``pinned_rows()``): rows 1 .. len(pinned) hold the given values, every other factor of them is
    chosen by the same greedy rule."""
    names = list(factors)
    nv = [len(factors[n]) for n in names]
    k = len(names)
    pinned = pinned_rows() if pinned is None else pinned
    open_pairs = all_pairs(factors)
    rows = [[0] * k]
    open_pairs -= _row_pairs(rows[0])
    rng = _Rng(seed)

    def best_row(fixed):
        pool = sorted(open_pairs)
        best, best_gain = None, -1
        for _ in range(candidates):
            row = [None] * k
            if fixed:
                for f, v in fixed.items():
                    row[f] = v
            else:
                i, a, j, b = pool[rng.below(len(pool))]
                row[i], row[j] = a, b
            done = [f for f in range(k) if row[f] is not None]
            order = [f for f in range(k) if row[f] is None]
            rng.shuffle(order)
            for f in order:
                gains = [sum(1 for d in done if ((d, row[d], f, v) if d < f else (f, v, d, row[d])) in open_pairs)
                         for v in range(nv[f])]
                top = max(gains)
                choice = [v for v, g in enumerate(gains) if g == top]
                row[f] = choice[rng.below(len(choice))]
                done.append(f)
            gain = len(_row_pairs(row) & open_pairs)
            if gain > best_gain:
                best, best_gain = row, gain
        return best

    for fix in pinned:
        rows.append(best_row({names.index(n): factors[n].index(v) for n, v in fix.items()}))
        open_pairs -= _row_pairs(rows[-1])
    while open_pairs:
        rows.append(best_row(None))
        open_pairs -= _row_pairs(rows[-1])
    return [OrderedDict((n, factors[n][v]) for n, v in zip(names, row)) for row in rows]


def uncovered_pairs(array, factors=FACTORS):
    names = list(factors)
    left = all_pairs(factors)
    for r in array:
        left -= _row_pairs([factors[n].index(r[n]) for n in names])
    return left


_ARRAY = []


def array():
    """the matrix (generated once per process; callers must not change it)"""
    if not _ARRAY:
        _ARRAY.extend(covering_array())
    return _ARRAY


def non_default(knobs):
    return OrderedDict((n, v) for n, v in knobs.items() if v != DEFAULTS[n])


def tuning_of(knobs):
    return {n: knobs[n] for n in TUNING_NAMES}


# ------------------------------------------------------------------------------------------------ bases
# The fourth base is PpoCnn 84x84x4, hidden_sizes (256,), 4 actions, shared trunk at 255 frames: the smallest batch at
# which the flattened first-layer weight gradient, and with it bwd_fuse21 = 1, runs (>= 200 workgroups), and a batch at
# which the fused conv1 -> conv2 forward runs at the default knobs.  Its seed was to be the first of 1..64 at which the
# float32 oracle stays within ORACLE_F32_GRAD of the float64 one and min_relu_preact >= RELU_MARGIN (as ``SEEDS`` of the
# zoo were chosen).  NO seed of 1..64 passes either check, neither for this net nor for the (512,) one at 255 frames: the
# first layer's bias gradient is a float32 sum of 102 000 cancelling terms (2.6e-6 at the best seed, typically 3e-6 .. 8e-6)
# and the net has 4.8 million relu units, the closest 2e-10 .. 2.08e-7 from its kink (profiles/knob_matrix_parity.md).
# The base keeps check (a) at the zoo's own bars all the same -- a reference whose float32 rounding is 0.42 of the gradient
# bar still resolves a kernel error of the bar's size -- and the CPU test (tests/test_cpu_knob_matrix.py) holds its reference
# to what seed 9, the one of 1..64 with the largest relu margin, gives:
#   * relu margin 2.08e-7: four times the 5e-8 rounding of a first-layer sum that ``net_zoo_helpers.min_relu_preact``
#     derives (the zoo asks five times) -> B255_RELU_MARGIN = 2.0e-7;
#   * float32 oracle 4.15e-6 from float64 on the worst gradient tensor (the zoo asks 1e-6) -> B255_F32_GRAD = 4.2e-6, below
#     half the gradient bar: a kernel whose rounding is the float32 oracle's own stays inside the bar.
B255_RELU_MARGIN, B255_F32_GRAD = 2.0e-7, 4.2e-6
B255 = Z._row("cnn84_h256_a4_b255", "ppo_cnn", Z._cnn((84, 84, 4), 4, (256,)), "ppo_step", 255,
              Z._x("ppo_fused", 4, deferred=1, mask=1), seed=9)


def _zoo(rid):
    return Z.ROWS[Z.ROW_IDS.index(rid)]


# cnn84_h512_a4_b33 is the zoo's shape under a seed of its own.  The second consecutive step (e) needs a third margin: the
# reference of step 2, taken from the float64 oracle's own step-1 parameters, must keep RELU_MARGIN too.  The zoo's seed 7
# does not (7.8e-8), and no seed of 1..64 passes all three CPU checks (only 7, 21 and 54 pass the float32 one).  489 is the
# first seed from 1 up that does: float32 oracle 8.96e-7, margins 2.97e-7 and 7.74e-7 (tests/test_cpu_knob_matrix.py).
CNN33 = dict(_zoo("cnn84_h512_a4_b33"), id="cnn84_h512_a4_b33_s489", seed=489)


# bars: of check (a), the zoo's on every base;  f32_grad / relu_margin: what the CPU test holds the base's reference to;  second: the second consecutive step (e);  train: the entry whose train check (f) runs
def _base(row, second, train, f32_grad=None, relu_margin=None):
    return dict(row=row, second=second, train=train, bars=dict(Z.BARS),
                f32_grad=Z.ORACLE_F32_GRAD if f32_grad is None else f32_grad,
                relu_margin=Z.RELU_MARGIN if relu_margin is None else relu_margin)


BASES = OrderedDict([
    ("cnn84_h512_a4_b33", _base(CNN33, True, "ppo")),
    ("impala84_a4_t9x3", _base(_zoo("impala84_a4_t9x3"), False, "impala")),
    ("mlp376_h256x3_a8_b33", _base(_zoo("mlp376_h256x3_a8_b33"), True, None)),
    ("cnn84_h256_a4_b255", _base(B255, False, None, f32_grad=B255_F32_GRAD, relu_margin=B255_RELU_MARGIN)),
])
MAX_SECOND_SKIPS = 2      # cases of a base that may skip (e) because the read-back parameters' reference left the margin


# ------------------------------------------------------------------------------------------------ the step's conditions
def wgrad_split(lay, b, target=512):
    """xt_net.hip ``wgrad_split``: the split-M factor the step asks a layer's weight-gradient blocks for"""
    m, n = b * lay.OH * lay.OW, lay.N
    tiles = Z._cdiv(lay.K, 128) * Z._cdiv(n, 32) if n <= 32 else Z._cdiv(lay.K, 64) * Z._cdiv(n, 64)
    return max(1, min(target // tiles, Z._cdiv(m, 32) // 4))


def dgrad_direct_blocks(lay, b, t):
    """xt_direct.hip ``plan_dgrad_direct_fused``: the 32-row tiles of the register-direct input gradient inside a fused
    backward launch (0: the shape stays on another input gradient)"""
    if not t["direct"] or not t["direct_dgrad"] or lay.N % 32 or lay.C % 32 or lay.C % 64 == 0:
        return 0
    mc = b * Z._cdiv(lay.H, lay.S) * Z._cdiv(lay.W, lay.S)
    nsteps = Z._cdiv(lay.KH, lay.S) * Z._cdiv(lay.KW, lay.S) * (lay.N // 32)
    tiles = Z._cdiv(mc, 32) * (lay.C // 32) * lay.S * lay.S
    if not t["direct_all"] and (nsteps < 8 or tiles >= t["direct_tile64_tiles"]):
        return 0
    return tiles


def launch_ksplit(lay, b, t, u8=False, has_idx=False):
    """the split-K factor ``launch_fwd`` (xt_igemm.hip) cuts the deferred forward of ``lay`` into under the knobs ``t``:
    ``net_zoo_helpers.launch_ksplit`` with the knobs its constants stand for (``launch_fwd_direct``: direct, direct_fwd,
    direct_all, direct_waves, direct_max_waves; the LDS-tiled first choice: fwd_tiled_valid, bf16x6; the request:
    fwd_split_target)"""
    m, n, k = b * lay.OH * lay.OW, lay.N, lay.K
    split = max(Z.fwd_split(lay, b, t["fwd_split_target"]), 1)
    nsteps = Z._cdiv(k, 32)
    tiled_first = bool(t["fwd_tiled_valid"] and t["bf16x6"] and not u8 and n <= 32 and k >= 256 and not Z._padded(lay))
    tj = 2 if n % 64 == 0 else 1
    direct = (not tiled_first and t["direct"] and t["direct_fwd"] and not has_idx and not u8 and lay.C % 16 == 0 and
              k % 32 == 0 and n % 32 == 0 and (t["direct_all"] or (tj == 1 and k >= 256)))
    if direct:
        tiles = Z._cdiv(m, 32) * (n // (32 * tj))
        slices = max(1, min(Z._cdiv(t["direct_waves"], tiles), nsteps // 2))
        nw = min(slices, t["direct_max_waves"])
        ks = max(1, min(Z._cdiv(slices, nw), split))
        return Z._cdiv(nsteps, Z._cdiv(nsteps, ks))
    return Z._cdiv(nsteps, Z._cdiv(nsteps, split))


ENVELOPE_KNOBS = ("conv1_bf16x3", "conv1_flat", "conv1_waves", "bf16x6", "fwd_tiled_valid", "fwd_two_groups",
                  "fwd_four_groups", "fwd_prefetch_all")


def envelope_knobs_hold(t):
    """the eight knob conditions of ``conv12_valid_envelope``: the first layer takes the flat bf16x3 form (it writes the
    sign mask), the second the four-group bf16x6 form"""
    return bool(t["conv1_bf16x3"] and t["conv1_flat"] and t["conv1_waves"] != 4 and t["bf16x6"] and t["fwd_tiled_valid"] and
                t["fwd_two_groups"] and t["fwd_four_groups"] and not t["fwd_prefetch_all"])


def conv12_envelope_open(spec, b, t):
    """is the fused conv1 -> conv2 launch (xt_conv1.hip ``conv12_u8_valid_fwd_flat_kernel``) offered AND inside its
    envelope for this net, batch and knobs: the conditions of ``net_forward`` (two layers without pre-activation, the
    second layer's own forward not split over K) and of ``conv12_valid_envelope`` (knobs, geometry, rows per block)"""
    lays, xf = spec.layers, spec.input_xform
    n0 = sum(1 for l in lays if l.trunk == 0)
    if n0 < 2 or lays[0].act in Z.PREACT or lays[1].act in Z.PREACT:
        return False
    g, g2 = lays[0], lays[1]
    if Z.fwd_split(g2, b, t["fwd_split_target"]) != 1 or not envelope_knobs_hold(t):
        return False
    if not xf[0] or abs(xf[1]) >= 1e-4 or b < 1:
        return False
    if not (g.C == 4 and g.KW == 8 and g.KH == 8 and g.N == 32 and g.PT == 0 and g.PL == 0) or Z._padded(g):
        return False
    hwc = g.H * g.W * 4
    if hwc % 16 or hwc > 64 * 1024 or (g.W * 4) % 8 or (g.S * 4) % 8:
        return False
    if not (g2.C == 32 and g2.N == 32 and g2.KH == 4 and g2.KW == 4 and g2.S == 2 and g2.PT == 0 and g2.PL == 0):
        return False
    if g2.H != g.OH or g2.W != g.OW or g.OH != 2 * g2.OH + 2 or g.OW != 2 * g2.OW + 2:
        return False
    if b * g.OH * g.OW * 32 * 4 >= 1 << 31 or Z._cdiv(b * g2.OH * g2.OW, 128) > 256:
        return False
    rows = b * g2.OH
    nblk = max(min(rows, 256), Z._cdiv(rows, 12))
    r = Z._cdiv(rows, nblk)
    return r <= 12 and r * g2.OW <= 128 and (r + g2.OH - 2) // g2.OH + 1 <= 3


def expected_words(row, spec, knobs):
    """the report words of one step of zoo-style ``row`` under ``knobs`` (every factor), from the step's conditions ->
    dict(head, layers, trunks, preact, tail_overlap, finish_form (tuple of the values the conditions allow), fwd_fuse12,
    bwd_fuse21, ksplit / deferred / mask_valid (one per layer), conv12 (the fused conv1 -> conv2 launch runs))"""
    t = knobs
    base = Z.plan_from_conditions(dict(row, tuning={k: t[k] for k in Z.TUNING_DEFAULTS}), spec)
    lays, b, entry, xf = spec.layers, Z.frames(row), row["entry"], spec.input_xform
    nl = len(lays)
    begin = [min(i for i, l in enumerate(lays) if l.trunk == tr) for tr in range(spec.n_trunks)]
    end = [max(i for i, l in enumerate(lays) if l.trunk == tr) + 1 for tr in range(spec.n_trunks)]
    pre = [l.act in Z.PREACT for l in lays]
    fused_head = base["head"] in ("ppo_fused", "gauss_fused", "impala_fused")
    # (IMPALA's fused head always takes the partials; PPO's only with defer_splitk)
    offered = fused_head and (entry == "impala_step" or t["defer_splitk"] != 0)
    ksplit, deferred, mask_valid = [1] * nl, [0] * nl, [0] * nl
    for tr in range(spec.n_trunks):
        li = end[tr] - 1
        first = li == begin[tr]
        u8_first = bool(first and xf[0])
        if offered and not pre[li] and not u8_first:
            ksplit[li] = launch_ksplit(lays[li], b, t, u8=False, has_idx=first and entry == "ppo_step")
            deferred[li] = int(ksplit[li] > 1)
    # the sign mask: written by the flat bf16x3 first layer (and by the fused conv12 launch, whose envelope pins that form)
    mask_valid[0] = int(bool(lays[0].N == 32 and lays[0].act == "relu" and Z._conv1_flat_mask(lays[0], xf, b) and
                             t["conv1_bf16x3"] and t["conv1_flat"] and t["conv1_waves"] == 8))
    fuse12 = base["fuse12"]      # (the ImpalaCnnOpt pair's kernel reads no knob but its own threshold)
    conv12 = bool(t["fwd_fuse12_flat"] and not fuse12 and conv12_envelope_open(spec, b, t))
    # bwd_fuse21: plan_bwd_layer takes it inside the all-classes input gradient next to the four-stage weight gradient
    fuse21 = 0
    if t["bwd_fuse21"] != 0 and spec.n_trunks == 1 and nl >= 2 and mask_valid[0]:
        l0, l1 = lays[0], lays[1]
        n_dg = Z._cdiv(b * (l1.H // 2) * (l1.W // 2), 128)
        classes = (l1.S == 2 and l1.KH == 4 and l1.KW == 4 and l1.H % 2 == 0 and l1.W % 2 == 0 and l1.C == 32 and
                   l1.N == 32 and not Z._padded(l1))
        fuse21 = int(bool(classes and t["dgrad_all_classes"] and t["wgrad_rows"] == 4 and t["bf16x6"] and t["conv1_bf16x3"] and
                          l0.OH == l1.H and l0.OW == l1.W and (l0.S * 4) % 16 == 0 and
                          (t["bwd_fuse21"] == 2 or n_dg >= 200) and 512 - n_dg >= 8 * Z._cdiv(l1.K, 128)))
    # tail_overlap yields to finalize_ticket, to two trunks and to a layout it cannot split
    tail = 0
    off_a = lays[-1].param_off      # (the layout it splits: first layer first, the last layer and both heads behind it)
    if entry in ("ppo_step", "impala_step") and spec.n_trunks == 1 and nl >= 2 and lays[0].param_off == 0 and \
            not t["finalize_ticket"] and off_a > 0 and spec.pi_off > off_a and spec.v_off > off_a:
        tail = t["tail_overlap"] & 3
    # the gradient-reduction launch: PPO alone honours finalize_ticket (1: the last block finalises); tail_fused yields to
    # tail_overlap and to the ticket form, and runs fused (3) only where its whole grid can be resident at once -- a fact of
    # the device: at most 2048 workgroups of 256 threads (256 CUs x 2048 threads), so a grid beyond that is never fused
    if entry not in ("ppo_step", "impala_step"):
        form = (0,)
    elif entry == "ppo_step" and t["finalize_ticket"]:
        form = (1,)
    elif t["tail_fused"] and tail == 0:
        form = (2,) if fused_grid_lower_bound(spec) > 2048 else (2, 3)
    else:
        form = (2,)
    return dict(head=base["head"], layers=nl, trunks=spec.n_trunks, preact=base["preact"], tail_overlap=tail,
                finish_form=form, fwd_fuse12=fuse12, bwd_fuse21=fuse21, ksplit=ksplit, deferred=deferred,
                mask_valid=mask_valid, conv12=conv12)


def grad_counts(spec):
    """floats of every entry of the gradient table: trunk layers, pi head, v head"""
    return [(l.K + 1) * l.N for l in spec.layers] + [spec.feat * spec.action_dim + spec.action_dim, spec.feat + 1]


def fused_grid(counts, nslabs, t):
    """xt_optim.hip ``grads_finish_fused_grid``: the blocks of the fused tail for slab counts ``nslabs``"""
    grid = 1
    for c, ns in zip(counts, nslabs):
        cap = 32 if (t["reduce_deep_lanes"] > 0 and ns >= t["reduce_deep_lanes"]) else t["reduce_z_lanes"]
        zl = 1
        while zl < ns and zl < cap:
            zl <<= 1
        grid += Z._cdiv(Z._cdiv(c, 4), 256 // zl)
    return grid


def fused_grid_lower_bound(spec):
    return 1 + sum(Z._cdiv(Z._cdiv(c, 4), 256) for c in grad_counts(spec))


def zoo_facts(row, spec):
    """``expected_words`` at the knobs of a zoo row, as the dict ``net_zoo_helpers._x`` builds"""
    w = expected_words(row, spec, OrderedDict(DEFAULTS, **row["tuning"]))
    ends = [max(i for i, l in enumerate(spec.layers) if l.trunk == tr) for tr in range(spec.n_trunks)]
    d = {w["deferred"][e] for e in ends}
    assert len(d) == 1 and len(w["finish_form"]) == 1
    base = Z.plan_from_conditions(row, spec)
    return Z._x(w["head"], w["layers"], w["trunks"], d.pop(), w["mask_valid"][0], w["preact"], w["fwd_fuse12"], w["bwd_fuse21"],
                w["tail_overlap"], w["finish_form"][0], base["pad"], base["dense_conv"])


def report_words(rep):
    """``lib.step_report`` -> the words ``expected_words`` predicts (finish_form as reported)"""
    lay = rep["layer"]
    return dict(head=Z.head_class(rep["head_path"]), layers=rep["layers"], trunks=rep["trunks"],
                preact=int(any(l["preact"] for l in lay)), tail_overlap=rep["tail_overlap"], finish_form=rep["finish_form"],
                fwd_fuse12=rep["fwd_fuse12"], bwd_fuse21=rep["bwd_fuse21"], ksplit=[l["ksplit"] for l in lay],
                deferred=[l["deferred"] for l in lay], mask_valid=[l["mask_valid"] for l in lay])


def split_count_changes():
    """for each block-count target: (shape, count at the default, count at the factor's second value), the two differing.
    direct_waves / direct_max_waves cut the register-direct forward, which these nets' last layers (N a multiple of 64)
    take under direct_all only: a row of the array pairs them with it."""
    cnn = build(BASES["cnn84_h512_a4_b33"]["row"])[0]
    dense, conv2, conv3 = cnn.layers[3], cnn.layers[1], cnn.layers[2]
    d = OrderedDict(DEFAULTS)
    da = OrderedDict(d, direct_all=1)
    second = lambda k: FACTORS[k][1]
    return OrderedDict([
        ("fwd_split_target", ("fwd_split of the 33-frame Dense 3136 -> 512", Z.fwd_split(dense, 33, d["fwd_split_target"]),
                              Z.fwd_split(dense, 33, second("fwd_split_target")))),
        ("wgrad_split_target", ("wgrad_split of the 33-frame conv2", wgrad_split(conv2, 33, d["wgrad_split_target"]),
                                wgrad_split(conv2, 33, second("wgrad_split_target")))),
        ("direct_waves", ("launch_ksplit of that Dense layer under direct_all", launch_ksplit(dense, 33, da),
                          launch_ksplit(dense, 33, OrderedDict(da, direct_waves=second("direct_waves"))))),
        ("direct_max_waves", ("launch_ksplit of that Dense layer under direct_all", launch_ksplit(dense, 33, da),
                              launch_ksplit(dense, 33, OrderedDict(da, direct_max_waves=second("direct_max_waves"))))),
        ("direct_tile64_tiles", ("register-direct input-gradient blocks of the 33-frame conv3", dgrad_direct_blocks(conv3, 33, d),
                                 dgrad_direct_blocks(conv3, 33, OrderedDict(d, direct_tile64_tiles=second("direct_tile64_tiles"))))),
    ])


# ------------------------------------------------------------------------------------------------ references
_BUILT = {}


def build(row):
    """-> (netspec, oracle spec, initial parameters, inputs) of a base row, without any oracle step"""
    if row["id"] not in _BUILT:
        spec, ospec = Z.build_specs(row)
        params, _ = Z.seeded_params(row, ospec)
        _BUILT[row["id"]] = (spec, ospec, params, Z.make_inputs(row))
    return _BUILT[row["id"]]


def ppo_oracle_at(row, ospec, params, inp, steps_before=0, m=None, v=None, dtype=np.float64):
    """one PPO update in ``dtype`` from ``params`` with the optimiser state of ``steps_before`` earlier updates (``m`` /
    ``v``: their moments) -> (oracle, dict(loss, grads, params, gnorm, min_relu_z))"""
    cfg = dict(Z.PPO_CFG, BATCH_SIZE=Z.frames(row))
    orc = Z.nets.PpoLearnerOracle(ospec, OrderedDict((k, np.array(x, copy=True)) for k, x in params.items()), cfg, dtype)
    if steps_before:
        orc.opt.t = steps_before
        for k in orc.opt.m:
            orc.opt.m[k][...] = np.asarray(m[k], dtype).reshape(orc.opt.m[k].shape)
            orc.opt.v[k][...] = np.asarray(v[k], dtype).reshape(orc.opt.v[k].shape)
    i = inp["idx"]
    f32 = lambda x: x[i].astype(np.float32)
    out = orc.step(inp["obs"][i], inp["action"][i], f32(inp["logp"]), f32(inp["adv"]), f32(inp["old_v"]), f32(inp["target_v"]),
                   apply=True)
    return orc, dict(loss=out["loss"], grads=out["grads"], params=orc.net.params, gnorm=out["gnorm"], lr=cfg["LR"],
                     min_relu_z=Z.min_relu_preact(orc.net))


_FIRST = {}


def first_step_state(row):
    """the float64 oracle's own first update of a PPO base: parameters after it and the Adam moments (shared, unchanged)"""
    if row["id"] not in _FIRST:
        ref = Z.reference(row)
        orc, out = ppo_oracle_at(row, ref["ospec"], ref["params"], ref["inputs"])
        _FIRST[row["id"]] = dict(params=out["params"], m=orc.opt.m, v=orc.opt.v)
    return _FIRST[row["id"]]
