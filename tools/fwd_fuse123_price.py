#!/usr/bin/env python
"""Price of the fused conv1 -> conv2 -> conv3 forward from the planner's arithmetic alone (host only, no GPU):
for every batch B the blocks, the conv3 / conv2 / conv1 rows of the largest block, the share of the conv1 and conv2 rows
that are computed twice (halo), the LDS bytes of the launch and whether the network takes it.

    python tools/fwd_fuse123_price.py [B_first B_last]        (default 201 404; equal rows are folded into ranges)
"""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from xingtian_amd import lib as L                                          # noqa: E402

PLAN_WORDS, BLOCK_WORDS = 9, 15


def price(b):
    g0, g1, g2 = L.ConvGeom(), L.ConvGeom(), L.ConvGeom()
    g0.H, g0.W, g0.C, g0.KH, g0.KW, g0.S, g0.PT, g0.PL, g0.OH, g0.OW, g0.N = 84, 84, 4, 8, 8, 4, 0, 0, 20, 20, 32
    g1.H, g1.W, g1.C, g1.KH, g1.KW, g1.S, g1.PT, g1.PL, g1.OH, g1.OW, g1.N = 20, 20, 32, 4, 4, 2, 0, 0, 9, 9, 32
    g2.H, g2.W, g2.C, g2.KH, g2.KW, g2.S, g2.PT, g2.PL, g2.OH, g2.OW, g2.N = 9, 9, 32, 3, 3, 1, 0, 0, 7, 7, 64
    g0.act = g1.act = g2.act = L.ACT["relu"]
    xf = L.InputXform(1, 0.0, 255.0)
    cap = PLAN_WORDS + BLOCK_WORDS * (7 * b + 8)
    out = (ctypes.c_int32 * cap)()
    L.check(L.load().xt_conv123_valid_plan(ctypes.byref(g0), ctypes.byref(xf), ctypes.byref(g1), ctypes.byref(g2), b, 0, out,
                                           cap), "xt_conv123_valid_plan")
    if not out[0]:
        return ("outside",)
    blocks = [out[PLAN_WORDS + BLOCK_WORDS * k:PLAN_WORDS + BLOCK_WORDS * (k + 1)] for k in range(out[2])]
    rows3 = [k[1] - k[0] for k in blocks]
    rows2 = [k[3] - k[2] for k in blocks]
    rows1 = [k[5] // 20 for k in blocks]
    halo2 = sum(rows2) / (9.0 * b) - 1.0
    halo1 = sum(rows1) / (20.0 * b) - 1.0
    return (out[2], "%d samples / %d" % (out[3] // 7, out[4]), max(rows3), max(rows2), max(rows1),
            "%.0f %%" % (100 * halo2), "%.0f %%" % (100 * halo1), out[5], "fused" if out[1] else "conv12 + conv3")


def main():
    lo, hi = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (201, 404)
    print("| B | blocks | group | max conv3 rows | max conv2 rows | max conv1 rows | conv2 halo | conv1 halo | LDS bytes | network |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    span = lambda a, b: str(a) if a == b else "%s-%s" % (a, b)
    first, prev, nb0 = lo, None, None
    for b in range(lo, hi + 2):
        row = price(b) if b <= hi else None
        if prev is not None and (row is None or row[1:] != prev[1:]):
            print("| %s | %s |" % (span(first, b - 1), " | ".join([span(nb0, prev[0])] + [str(v) for v in prev[1:]])))
            first, nb0 = b, None
        if nb0 is None and row is not None:
            nb0 = row[0]
        prev = row


if __name__ == "__main__":
    main()
