"""The envelope and the split of the fused conv1 -> conv2 -> conv3 forward (conv123_u8_valid_fwd_flat_kernel), read through
the host-only C entry xt_conv123_valid_plan, and the three new C-ABI symbols.  No GPU.

The split cuts the B * 7 conv3 rows into runs; the block of a run computes the conv2 rows oy .. oy + 2 of each of its conv3
rows oy and the conv1 rows 2 oy2 .. 2 oy2 + 3 of each of those conv2 rows oy2.  Who stores what: conv3 row oy owns conv2 row
oy and conv1 rows 2 oy, 2 oy + 1; the last conv3 row of a sample also owns the two conv2 and four conv1 rows past them.
"""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OH1, OH2, OH3, OW1, OW2, OW3 = 20, 9, 7, 20, 9, 7
PLAN_WORDS, BLOCK_WORDS = 9, 15
HEAD = ("inside", "in_net", "blocks", "group_rows", "group_blocks", "lds_bytes", "lds_limit", "max_conv1_pos", "max_conv2_pos")


def _geoms(L):
    g0, g1, g2 = L.ConvGeom(), L.ConvGeom(), L.ConvGeom()
    g0.H, g0.W, g0.C, g0.KH, g0.KW, g0.S, g0.PT, g0.PL, g0.OH, g0.OW, g0.N = 84, 84, 4, 8, 8, 4, 0, 0, 20, 20, 32
    g1.H, g1.W, g1.C, g1.KH, g1.KW, g1.S, g1.PT, g1.PL, g1.OH, g1.OW, g1.N = 20, 20, 32, 4, 4, 2, 0, 0, 9, 9, 32
    g2.H, g2.W, g2.C, g2.KH, g2.KW, g2.S, g2.PT, g2.PL, g2.OH, g2.OW, g2.N = 9, 9, 32, 3, 3, 1, 0, 0, 7, 7, 64
    g0.act = g1.act = g2.act = L.ACT["relu"]
    return g0, g1, g2, L.InputXform(1, 0.0, 255.0)


@functools.lru_cache(maxsize=None)
def _plan(b, rows=0, third_filters=64):
    from xingtian_amd import lib as L
    g0, g1, g2, xf = _geoms(L)
    g2.N = third_filters
    cap = PLAN_WORDS + BLOCK_WORDS * (b * OH3 + 8)
    out = (ctypes.c_int32 * cap)()
    assert L.load().xt_conv123_valid_plan(ctypes.byref(g0), ctypes.byref(xf), ctypes.byref(g1), ctypes.byref(g2), b, rows,
                                          out, cap) == 0
    words = np.array(out[:], dtype=np.int64)
    head = dict(zip(HEAD, (int(v) for v in words[:PLAN_WORDS])))
    blocks = words[PLAN_WORDS:PLAN_WORDS + BLOCK_WORDS * head["blocks"]].reshape(-1, BLOCK_WORDS)
    return head, blocks


@pytest.mark.parametrize("b,inside,in_net", [(200, 1, 0), (201, 1, 1), (320, 1, 1), (321, 1, 0), (341, 1, 0), (342, 1, 0),
                                             (404, 1, 0), (405, 0, 0)])
def test_envelope_answers(b, inside, in_net):
    """200: conv2's own forward would be split over K; 201 .. 320: fused; 321 .. 404: the split needs more than one block
    per CU, so the network keeps conv12 + conv3 (the stand-alone entry still launches); 405: outside conv12's envelope"""
    head, _ = _plan(b)
    assert (head["inside"], head["in_net"]) == (inside, in_net)
    assert head["lds_limit"] == 160 * 1024
    if inside:
        assert (head["blocks"] <= 256) == (b <= 320)
        assert 0 < head["lds_bytes"] <= head["lds_limit"]


def test_other_layers_and_oversized_runs_are_refused():
    assert _plan(320, 0, 32)[0]["inside"] == 0                             # another third layer
    assert _plan(8, 8)[0]["inside"] == 1
    assert _plan(8, 9)[0]["inside"] == 0                                   # some run of 9 rows touches three samples
    assert _plan(8, 10)[0]["inside"] == 0
    assert _plan(320, 8)[0]["in_net"] == 0                                 # the network takes the automatic split only


def test_headline_split():
    """B = 320: five samples (35 rows) over four blocks of 8, 9, 9, 9 rows, 256 blocks; the largest block computes 13 conv2
    rows and 30 conv1 rows"""
    head, blocks = _plan(320)
    assert (head["blocks"], head["group_rows"], head["group_blocks"]) == (256, 35, 4)
    assert [int(r1 - r0) for r0, r1 in blocks[:4, :2]] == [8, 9, 9, 9]
    assert head["max_conv2_pos"] == 13 * OW2 and head["max_conv1_pos"] == 30 * OW1


CASES = [(1, 0), (1, 1), (2, 7), (3, 8), (7, 8), (7, 1), (29, 0), (201, 0), (208, 0), (256, 0), (320, 0), (343, 0), (404, 0)]


@pytest.mark.parametrize("b,rows", CASES)
def test_every_row_has_one_owner_that_computes_what_it_needs(b, rows):
    head, blocks = _plan(b, rows)
    assert head["inside"] == 1 and len(blocks) == head["blocks"]
    r0, r1, c0, c1, s0, npos = (blocks[:, i] for i in range(6))
    # the conv3 runs tile [0, 7 B) in order: every conv3 row is owned by exactly one block
    assert r0[0] == 0 and r1[-1] == b * OH3 and np.array_equal(r0[1:], r1[:-1]) and (r1 > r0).all()
    if rows:
        assert (r1 - r0 <= rows).all() and ((r1 - r0)[:-1] == rows).all()
    assert ((r1 - r0) * OW3 <= 64).all() and ((c1 - c0) * OW2 <= 128).all() and (npos <= 768).all()
    owner = np.repeat(np.arange(len(blocks)), r1 - r0)                     # conv3 flat row -> block
    for k, blk in enumerate(blocks):
        pieces = blk[6:].reshape(3, 3)                                     # {conv2 rows, first conv1 row, ends its sample}
        assert int(blk[4]) == int(blk[2]) // OH2
        # the pieces are the block's conv2 run cut at the samples
        got = []
        for i, (n, clo, ends) in enumerate(pieces):
            if n > 0:
                assert clo % 2 == 0
                got += [(int(blk[4]) + i) * OH2 + clo // 2 + j for j in range(n)]
                assert bool(ends) == (clo // 2 + n == OH2)
        assert got == list(range(int(blk[2]), int(blk[3])))
        assert int(blk[5]) == sum((2 * n + 2) * OW1 for n, _, _ in pieces if n > 0)
        # every conv3 row reads three conv2 rows of ITS sample, all inside the run
        for f3 in range(int(blk[0]), int(blk[1])):
            s, oy = divmod(f3, OH3)
            assert oy + 2 < OH2
            assert int(blk[2]) <= s * OH2 + oy and s * OH2 + oy + 2 < int(blk[3])
        # every computed conv2 row reads four conv1 rows of its sample, all inside the piece of that sample
        for f2 in range(int(blk[2]), int(blk[3])):
            s, oy2 = divmod(f2, OH2)
            n, clo, _ = pieces[s - int(blk[4])]
            assert clo <= 2 * oy2 and 2 * oy2 + 3 < clo + 2 * n + 2 <= OH1
    # the owner of every conv2 and conv1 row computes it
    for s in (0, b // 2, b - 1):
        for oy2 in range(OH2):
            blk = blocks[owner[s * OH3 + min(oy2, OH3 - 1)]]
            assert int(blk[2]) <= s * OH2 + oy2 < int(blk[3])
        for r in range(OH1):
            blk = blocks[owner[s * OH3 + min(r // 2, OH3 - 1)]]
            n, clo, _ = blk[6:].reshape(3, 3)[s - int(blk[4])]
            assert n > 0 and clo <= r < clo + 2 * n + 2


def test_lds_footprint_is_the_largest_phase():
    """max(bf16 image + 48 KB of conv1 weight planes, act1 planes + 36 KB of transpose buffers, 72 KB combine buffer + act2
    planes) + 8 B per conv1 position; 600 positions at B = 320"""
    head, _ = _plan(320)
    nps = (head["max_conv1_pos"] + 7) // 8 * 8 + 4
    assert head["lds_bytes"] == 192 * nps + 8 * 32 * 36 * 4 + 8 * head["max_conv1_pos"] == 157632


def _want(header, name, structs):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
    assert m, name
    ctype_of = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float}
    want = []
    for arg in m.group(1).split(","):
        words = arg.replace("*", " * ").split()
        if "*" in words:
            pointee = [w for w in words if w not in ("const", "*")][0]
            want.append(structs.get(pointee, ctypes.c_void_p))
        else:
            want.append(ctype_of[[w for w in words if w != "const"][0]])
    return want


def test_header_ctypes_table_and_library_agree_on_the_new_symbols():
    from xingtian_amd import lib
    header = open(os.path.join(ROOT, "include", "xt_mi355x.h")).read()
    structs = {"xt_conv_geom": ctypes.POINTER(lib.ConvGeom), "xt_input_xform": ctypes.POINTER(lib.InputXform)}
    handle = lib.load()
    for name in ("xt_net_set_fwd_fuse123_flat", "xt_conv123_valid_fwd", "xt_conv123_valid_plan"):
        assert name in lib.SIGNATURES and hasattr(handle, name), name
        res, args = lib.SIGNATURES[name]
        want = _want(header, name, structs)
        assert res is ctypes.c_int32 and len(args) == len(want), (name, len(args), len(want))
        for i, (a, w) in enumerate(zip(args, want)):
            assert a is w, (name, i, a, w)
    for word, value in zip(HEAD + ("PLAN_WORDS",), range(PLAN_WORDS + 1)):
        name = {"inside": "INSIDE", "in_net": "IN_NET", "blocks": "BLOCKS", "group_rows": "GROUP_ROWS",
                "group_blocks": "GROUP_BLOCKS", "lds_bytes": "LDS_BYTES", "lds_limit": "LDS_LIMIT",
                "max_conv1_pos": "MAX_CONV1_POS", "max_conv2_pos": "MAX_CONV2_POS"}.get(word, "WORDS")
        assert re.search(r"\bXT_CONV123_PLAN_%s = %d\b" % (name, value), header), word
    assert re.search(r"\bXT_CONV123_BLOCK_WORDS = %d\b" % BLOCK_WORDS, header)


def test_the_switch_is_per_net_and_on_by_default():
    """no tuning knob was added; the report's word is a tail word behind the counted ones; the Python wrapper mirrors the
    library's default"""
    from xingtian_amd import lib
    from xingtian_amd.model.hip_net import HipActorCritic
    assert "fwd_fuse123_flat" not in [n for n, _ in lib.Tuning._fields_]
    assert lib.STEP_REPORT_TAIL == ("FWD_FUSE123",)
    header = open(os.path.join(ROOT, "include", "xt_mi355x.h")).read()
    assert re.search(r"\bXT_STEP_TAIL_FWD_FUSE123 = 0\b", header) and re.search(r"\bXT_STEP_TAIL_WORDS = 1\b", header)
    assert HipActorCritic.fwd_fuse123_flat_on is True and callable(HipActorCritic.set_fwd_fuse123_flat)
