#!/usr/bin/env python
"""Time PpoCnn's conv1 -> conv2 -> conv3 forward as two launches (xt_conv12_valid_fwd + xt_layer_fwd) against the one
launch (xt_conv123_valid_fwd, automatic split) over a range of batches: eager launches back to back on one stream, HIP
events, best of 3 x 300, us per forward.  Needs a GPU.

    python tools/fwd_fuse123_envelope.py [B ...]
"""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from xingtian_amd import lib as L                                          # noqa: E402

PLAN_WORDS = 9


def main():
    sizes = [int(a) for a in sys.argv[1:]] or [201, 224, 256, 257, 288, 292, 293, 320, 321, 341, 360, 404]
    lib = L.load()
    g0, g1, g2 = L.ConvGeom(), L.ConvGeom(), L.ConvGeom()
    g0.H, g0.W, g0.C, g0.KH, g0.KW, g0.S, g0.PT, g0.PL, g0.OH, g0.OW, g0.N = 84, 84, 4, 8, 8, 4, 0, 0, 20, 20, 32
    g1.H, g1.W, g1.C, g1.KH, g1.KW, g1.S, g1.PT, g1.PL, g1.OH, g1.OW, g1.N = 20, 20, 32, 4, 4, 2, 0, 0, 9, 9, 32
    g2.H, g2.W, g2.C, g2.KH, g2.KW, g2.S, g2.PT, g2.PL, g2.OH, g2.OW, g2.N = 9, 9, 32, 3, 3, 1, 0, 0, 7, 7, 64
    g0.act = g1.act = g2.act = L.ACT["relu"]
    xf = L.InputXform(1, 0.0, 255.0)
    rng = np.random.default_rng(0)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    w = [dev((rng.standard_normal(s) * 0.05).astype(np.float32)) for s in ((256, 32), (32,), (512, 32), (32,), (288, 64), (64,))]
    st = L.stream_ptr()
    print("| B | blocks | network | two launches | fused | difference |")
    print("|---|---|---|---|---|---|")
    for b in sizes:
        frames = dev(rng.integers(0, 256, (b, 84, 84, 4)).astype(np.uint8))
        a1 = torch.zeros((b * 400, 32), device="cuda")
        m = torch.zeros((b * 400,), dtype=torch.int32, device="cuda")
        a2 = torch.zeros((b * 81, 32), device="cuda")
        a3 = torch.zeros((b * 49, 64), device="cuda")
        plan = (ctypes.c_int32 * PLAN_WORDS)()
        L.check(lib.xt_conv123_valid_plan(ctypes.byref(g0), ctypes.byref(xf), ctypes.byref(g1), ctypes.byref(g2), b, 0, plan,
                                          PLAN_WORDS), "xt_conv123_valid_plan")

        def two():
            L.check(lib.xt_conv12_valid_fwd(ctypes.byref(g0), ctypes.byref(xf), ctypes.byref(g1), b, L.ptr(frames), None,
                                            L.ptr(w[0]), L.ptr(w[1]), L.ptr(a1), L.ptr(m), L.ptr(w[2]), L.ptr(w[3]), L.ptr(a2),
                                            0, st), "xt_conv12_valid_fwd")
            L.check(lib.xt_layer_fwd(ctypes.byref(g2), None, b, L.ptr(a2), None, L.ptr(w[4]), L.ptr(w[5]), L.ptr(a3), None, 1,
                                     st), "xt_layer_fwd")

        def one():
            L.check(lib.xt_conv123_valid_fwd(ctypes.byref(g0), ctypes.byref(xf), ctypes.byref(g1), ctypes.byref(g2), b,
                                             L.ptr(frames), None, L.ptr(w[0]), L.ptr(w[1]), L.ptr(a1), L.ptr(m), L.ptr(w[2]),
                                             L.ptr(w[3]), L.ptr(a2), L.ptr(w[4]), L.ptr(w[5]), L.ptr(a3), 0, st),
                    "xt_conv123_valid_fwd")

        def best(fn):
            for _ in range(20):
                fn()
            out = []
            for _ in range(3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(300):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                out.append(e0.elapsed_time(e1) * 1000.0 / 300)
            return min(out)

        t2, t1 = best(two), best(one)
        print("| %d | %d | %s | %.2f | %.2f | %+.2f |" % (b, plan[2], "fused" if plan[1] else "conv12 + conv3", t2, t1, t1 - t2),
              flush=True)


if __name__ == "__main__":
    main()
