"""GPU parity tests (run with -m gpu on an MI355X) of the forward dispatcher (launch_fwd, about twenty kernel instances)
and of the first layer's weight gradient as the update runs it (launch_wgrad with slabs: the uint8 first-layer kernels,
which xt_layer_wgrad never reaches).  xt_layer_fwd_ex / xt_layer_wgrad_slabs report the branch taken; every row of
FWD_CASES / WG1_CASES names the branch and sub-fields it must take (XT_FWD_PATH_* / XT_WG1_PATH_* of
include/xt_mi355x.h), worked out from the dispatchers, so a case that drifts onto another kernel fails instead of passing
there.  Reference: float64 im2col products (oracle.nets), in chunks of samples for the large batches.

tests/test_cpu_fwd_coverage.py imports the tables on the CPU and checks that every branch and knob value has cases."""
import collections
import ctypes
import os
import re
import zlib

import numpy as np
import pytest
import torch

from oracle import nets

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

U8 = (1, 0.0, 255.0)          # xform = (uint8 flag, mean, std): the PPO / IMPALA state transform
F32 = (0, 0.0, 1.0)

FwdCase = collections.namedtuple(
    "FwdCase", "id kind hw cin cout k s padding act B path tile units nst ks xcd xform gather ksplit knobs probe kh")
Wg1Case = collections.namedtuple(
    "Wg1Case", "id kind hw cin cout k s padding act B path units slabs xform gather msplit slab_cap knobs probe")


def fwd(id, hw, cin, cout, k, s, padding, act, B, path, tile=0, units=1, nst=0, ks=1, xcd=0, xform=F32, gather=False,
        ksplit=1, knobs=None, probe=False, kh=None, kind="conv"):
    """path: the expected XT_FWD_PATH_* suffix; tile: the expected XT_FWD_TILE_* suffix (0: none); units / nst / ks / xcd:
    the expected sub-fields (see the header); ksplit: the split-K count ASKED for (ks: the effective one); kh: kernel rows
    when they differ from the kernel columns k; probe: the input is zero but for one entry, bias zero, no activation"""
    return FwdCase(id, kind, hw, cin, cout, k, s, padding, act, B, path, tile, units, nst, ks, xcd, xform, gather, ksplit,
                   knobs or {}, probe, kh)


def c1(id, hw, s, act, B, path, units, xform=U8, **kw):
    """a uint8 VALID first layer as PpoCnn's: 4 channels, 8-wide kernel, 32 filters"""
    return fwd(id, hw, 4, 32, 8, s, "valid", act, B, path, units=units, xform=xform, **kw)


def c1s(id, hw, k, act, B, path, units, xform=U8, **kw):
    """a uint8 SAME first layer as ImpalaCnnOpt's: 4 channels, 8x8/4 or 4x4/2, 16 filters"""
    return fwd(id, hw, 4, 16, k, k // 2, "same", act, B, path, units=units, xform=xform, **kw)


def fdense(id, cin, cout, act, B, path, tile, units, **kw):
    return fwd(id, (1, 1), cin, cout, 1, 1, "valid", act, B, path, tile, units, kind="dense", **kw)


S, Lg = "128X32", "64X64"
NOFLAT, W4, NOX3 = dict(conv1_flat=0), dict(conv1_waves=4), dict(conv1_bf16x3=0)
ALL, FP32 = dict(fwd_prefetch_all=1), dict(bf16x6=0)

# Where the expectations come from (xt_igemm.hip launch_fwd, xt_conv1.hip launch_conv1_*, xt_direct.hip launch_fwd_direct):
#  * first layer VALID: flattened when conv1_flat, 8 waves, KH = 8 and OH*OW >= 256 (a range of 256 / 512 positions must
#    touch at most 2 / 3 frame stacks); 512 positions from ceil(B*OH*OW / 512) >= 200 blocks, else 256.  84x84 /4 has 400
#    positions: 255 stacks are 199.2 -> 200 blocks, 254 are 198.4 -> 199.  68x68 /4 and 38x38 /2 have 256: 399 stacks
#    are 199.5 -> 200 blocks.  A mean makes the launcher refuse (generic uint8 kernel).
#  * first layer SAME: 512 positions for 8x8 kernels from 200 blocks (441 positions on 84x84: 232 stacks are 199.8 -> 200
#    blocks, 231 are 198.97 -> 199), 4x4 kernels always 256; odd W or a fractional mean is refused.
#  * register-direct: C % 16 = K % 32 = N % 32 = 0, no gather, fp32 input; by default only N % 64 != 0 with K >= 256, and
#    not the unpadded N <= 32, K >= 256 layers (fwd_tiled_valid with bf16x6).  units = waves per block:
#    slices = min(ceil(1536 / tiles), K/32 / 2), waves = min(slices, 8), split = min(ceil(slices / waves), ksplit asked).
#  * LDS-tiled: 128x32 tiles for N <= 32, else 64x64; nblk = tiles * ksplit; two wave groups when nblk <= 320 and the
#    k chunk per split is >= 256; four (bf16x6 only) when also nblk <= 256 and the chunk >= 512; fwd_prefetch_all takes the
#    unpadded two-group bf16x6 launches with (steps + 1) / 2 <= 8 steps per group; the XCD-chunked order is on when there
#    is more than one column tile or a split.
FWD_CASES = [
    # ---- first layer VALID, flattened over the batch (the relu rows also check the sign mask)
    c1("c1flat_84_b5", (84, 84), 4, "relu", 5, "C1_FLAT", 256),
    c1("c1flat_84_b1_none", (84, 84), 4, "none", 1, "C1_FLAT", 256),
    c1("c1flat_84_b255", (84, 84), 4, "relu", 255, "C1_FLAT", 512),
    c1("c1flat_84_b254_elu", (84, 84), 4, "elu", 254, "C1_FLAT", 256),
    c1("c1flat_68_b3", (68, 68), 4, "relu", 3, "C1_FLAT", 256),
    c1("c1flat_68_b399", (68, 68), 4, "relu", 399, "C1_FLAT", 512),
    c1("c1flat_38s2_b2", (38, 38), 2, "relu", 2, "C1_FLAT", 256),
    c1("c1flat_84x68_b3", (84, 68), 4, "relu", 3, "C1_FLAT", 256),
    c1("c1flat_84_b3_std1", (84, 84), 4, "relu", 3, "C1_FLAT", 256, xform=(1, 0.0, 1.0)),
    c1("c1flat_84_b6_gather", (84, 84), 4, "relu", 6, "C1_FLAT", 256, gather=True),
    c1("c1flat_84_probe", (84, 84), 4, "none", 2, "C1_FLAT", 256, probe=True),
    # ---- ... one frame stack per workgroup: fewer than 256 positions, a knob, or fewer than 8 kernel rows
    c1("c1stack_44_b3", (44, 44), 4, "relu", 3, "C1_STACK", 8),
    c1("c1stack_84_b1_noflat", (84, 84), 4, "relu", 1, "C1_STACK", 8, knobs=NOFLAT),
    c1("c1stack_84_b7_noflat_none", (84, 84), 4, "none", 7, "C1_STACK", 8, knobs=NOFLAT),
    c1("c1stack_84_b5_waves4", (84, 84), 4, "relu", 5, "C1_STACK", 4, knobs=W4),
    c1("c1stack_44_b3_waves4_elu", (44, 44), 4, "elu", 3, "C1_STACK", 4, knobs=W4),
    c1("c1stack_84_kh6_b3", (84, 84), 4, "relu", 3, "C1_STACK", 8, kh=6),
    c1("c1stack_84_b6_gather_noflat", (84, 84), 4, "relu", 6, "C1_STACK", 8, gather=True, knobs=NOFLAT),
    c1("c1stack_44_b4_std1", (44, 44), 4, "relu", 4, "C1_STACK", 8, xform=(1, 0.0, 1.0)),
    c1("c1stack_44_probe", (44, 44), 4, "none", 2, "C1_STACK", 8, probe=True),
    # ---- first layer SAME
    c1s("c1same_84_b3", (84, 84), 8, "relu", 3, "C1_SAME", 256),
    c1s("c1same_84_b232", (84, 84), 8, "relu", 232, "C1_SAME", 512),
    c1s("c1same_84_b231", (84, 84), 8, "relu", 231, "C1_SAME", 256),
    c1s("c1same_42_b4", (42, 42), 4, "relu", 4, "C1_SAME", 256),
    c1s("c1same_42_b1", (42, 42), 4, "relu", 1, "C1_SAME", 256),
    c1s("c1same_42_b232", (42, 42), 4, "relu", 232, "C1_SAME", 256),
    c1s("c1same_42_b6_m128", (42, 42), 4, "relu", 6, "C1_SAME", 256, xform=(1, 128.0, 128.0)),
    c1s("c1same_42_b6_m128_gather", (42, 42), 4, "relu", 6, "C1_SAME", 256, xform=(1, 128.0, 128.0), gather=True),
    c1s("c1same_84_b5_m128_gather_none", (84, 84), 8, "none", 5, "C1_SAME", 256, xform=(1, 128.0, 128.0), gather=True),
    c1s("c1same_84_probe", (84, 84), 8, "none", 2, "C1_SAME", 256, probe=True),
    c1s("c1same_42_probe_m128", (42, 42), 4, "none", 3, "C1_SAME", 256, xform=(1, 128.0, 128.0), probe=True),
    # ---- uint8 layers the first-layer launchers refuse, or conv1_bf16x3 = 0: the generic LDS-tiled fp32 kernel
    c1s("u8gen_43_oddw_b3", (43, 43), 4, "relu", 3, "TILED_FP32", 1, tile=S),                      # (K = 64: one group)
    c1s("u8gen_84_mean127p5_b3", (84, 84), 8, "relu", 3, "TILED_FP32", 2, tile=S, xform=(1, 127.5, 128.0)),
    c1("u8gen_84_mean128_b3", (84, 84), 4, "relu", 3, "TILED_FP32", 2, tile=S, xform=(1, 128.0, 128.0)),
    c1("u8gen_ppo_b5_nox3", (84, 84), 4, "relu", 5, "TILED_FP32", 2, tile=S, knobs=NOX3),
    c1s("u8gen_imp_b3_nox3", (84, 84), 8, "relu", 3, "TILED_FP32", 2, tile=S, knobs=NOX3),
    c1("u8gen_ppo_b4_nox3_gather", (84, 84), 4, "relu", 4, "TILED_FP32", 2, tile=S, knobs=NOX3, gather=True),
    c1("u8gen_ppo_probe_nox3", (84, 84), 4, "none", 2, "TILED_FP32", 2, tile=S, knobs=NOX3, probe=True),
    # ---- register-direct (units = waves per block)
    fwd("direct_imp_conv2_b6", (21, 21), 16, 32, 4, 2, "same", "relu", 6, "DIRECT", "DIRECT_TJ1", 4),
    fwd("direct_3x3_32_96_b5", (9, 9), 32, 96, 3, 1, "valid", "tanh", 5, "DIRECT", "DIRECT_TJ1", 4),
    fwd("direct_all_conv3_b9", (9, 9), 32, 64, 3, 1, "valid", "relu", 9, "DIRECT", "DIRECT_TJ2", 4,
        knobs=dict(direct_all=1)),
    fwd("direct_all_k64_b4", (6, 6), 16, 32, 2, 1, "valid", "relu", 4, "DIRECT", "DIRECT_TJ1", 1, knobs=dict(direct_all=1)),
    fdense("direct_splitk_1024_96_b37", 1024, 96, "relu", 37, "DIRECT", "DIRECT_TJ1", 8, ksplit=3, ks=2),
    fwd("direct_ppo_conv2_b7_notiledvalid", (20, 20), 32, 32, 4, 2, "valid", "relu", 7, "DIRECT", "DIRECT_TJ1", 8,
        knobs=dict(fwd_tiled_valid=0)),
    fwd("direct_ppo_conv2_b7_fp32", (20, 20), 32, 32, 4, 2, "valid", "relu", 7, "DIRECT", "DIRECT_TJ1", 8, knobs=FP32),
    fwd("direct_imp_conv2_probe", (21, 21), 16, 32, 4, 2, "same", "none", 2, "DIRECT", "DIRECT_TJ1", 4, probe=True),
    # ---- LDS-tiled bf16x6 (units = wave groups)
    fwd("x6_imp_conv2_b6_nodirectfwd", (21, 21), 16, 32, 4, 2, "same", "relu", 6, "TILED_X6", S, 2,
        knobs=dict(direct_fwd=0)),
    fwd("x6_imp_conv2_b6_nodirect", (21, 21), 16, 32, 4, 2, "same", "relu", 6, "TILED_X6", S, 2, knobs=dict(direct=0)),
    fwd("x6_ppo_conv2_b7", (20, 20), 32, 32, 4, 2, "valid", "relu", 7, "TILED_X6", S, 4),
    fwd("x6_ppo_conv3_b9", (9, 9), 32, 64, 3, 1, "valid", "relu", 9, "TILED_X6", Lg, 2),
    fdense("x6_ppo_dense_b37", 3136, 256, "relu", 37, "TILED_X6", Lg, 4, xcd=1),
    fdense("x6_ppo_dense_b1", 3136, 256, "tanh", 1, "TILED_X6", Lg, 4, xcd=1),
    # 4x4 32->32 (PpoCnn conv2's instance) at stride 1: 8 x 64x64 rows = 256 blocks, 8 x 50x82 = 257, 10 x ... = 320 / 321
    fwd("x6_4x4_32_256blk", (67, 67), 32, 32, 4, 1, "valid", "relu", 8, "TILED_X6", S, 4),
    fwd("x6_4x4_32_257blk", (53, 85), 32, 32, 4, 1, "valid", "relu", 8, "TILED_X6", S, 2),
    fwd("x6_4x4_32_320blk", (67, 67), 32, 32, 4, 1, "valid", "relu", 10, "TILED_X6", S, 2),
    fwd("x6_4x4_32_321blk", (53, 85), 32, 32, 4, 1, "valid", "relu", 10, "TILED_X6", S, 1),
    # 3x3 32->64 (PpoCnn conv3's instance): 20 x 32x32 rows = 320 blocks of 64, 22 x 19x49 = 20482 rows = 321
    fwd("x6_3x3_64_320blk", (34, 34), 32, 64, 3, 1, "valid", "relu", 20, "TILED_X6", Lg, 2),
    fwd("x6_3x3_64_321blk", (21, 51), 32, 64, 3, 1, "valid", "relu", 22, "TILED_X6", Lg, 1),
    fwd("x6_ppo_conv2_b7_nofour", (20, 20), 32, 32, 4, 2, "valid", "relu", 7, "TILED_X6", S, 2,
        knobs=dict(fwd_four_groups=0)),
    fwd("x6_ppo_conv2_b7_notwo", (20, 20), 32, 32, 4, 2, "valid", "relu", 7, "TILED_X6", S, 1,
        knobs=dict(fwd_two_groups=0)),
    fdense("x6_ppo_dense_b37_noxcd", 3136, 256, "relu", 37, "TILED_X6", Lg, 4, knobs=dict(fwd_xcd_chunk=0)),
    fwd("x6_5x5x4_b3", (15, 15), 4, 32, 5, 1, "valid", "none", 3, "TILED_X6", S, 1),                # (K = 100)
    # 98 steps: 16 splits asked -> 7 steps each -> 14 splits (224 < 256: one group); 3 asked -> 33 steps each -> 3
    fdense("x6_ppo_dense_b37_ks16", 3136, 256, "relu", 37, "TILED_X6", Lg, 1, ksplit=16, ks=14, xcd=1),
    fdense("x6_ppo_dense_b37_ks3", 3136, 256, "relu", 37, "TILED_X6", Lg, 4, ksplit=3, ks=3, xcd=1),
    fwd("x6_ppo_conv2_b7_ks2", (20, 20), 32, 32, 4, 2, "valid", "relu", 7, "TILED_X6", S, 2, ksplit=2, ks=2, xcd=1),
    fwd("x6_3x3_64_same_b9", (9, 9), 32, 64, 3, 1, "same", "relu", 9, "TILED_X6", Lg, 2),
    fwd("x6_3x3_8_32_same_b5", (10, 10), 8, 32, 3, 1, "same", "tanh", 5, "TILED_X6", S, 1),
    fwd("x6_ppo_conv2_probe", (20, 20), 32, 32, 4, 2, "valid", "none", 3, "TILED_X6", S, 4, probe=True),
    # ---- ... two groups with all loads up front: one row per instance (steps per group = (K/32 + 1) / 2)
    fwd("all_n4_128x32", (22, 22), 16, 32, 4, 2, "valid", "relu", 5, "TILED_X6_ALL", S, 2, nst=4, knobs=ALL),
    fwd("all_n4_64x64", (6, 6), 64, 64, 2, 1, "valid", "relu", 7, "TILED_X6_ALL", Lg, 2, nst=4, knobs=ALL),
    fwd("all_n5_64x64", (9, 9), 32, 64, 3, 1, "valid", "relu", 9, "TILED_X6_ALL", Lg, 2, nst=5, knobs=ALL),
    fwd("all_n8_128x32", (20, 20), 32, 32, 4, 2, "valid", "relu", 7, "TILED_X6_ALL", S, 2, nst=8, knobs=ALL),
    fwd("all_n8_64x64", (20, 20), 32, 64, 4, 2, "valid", "relu", 4, "TILED_X6_ALL", Lg, 2, nst=8, knobs=ALL),
    fwd("all_n8_64x64_6steps", (6, 6), 96, 64, 2, 1, "valid", "tanh", 5, "TILED_X6_ALL", Lg, 2, nst=8, knobs=ALL),
    fwd("all_n8_128x32_5steps", (9, 9), 32, 32, 3, 1, "valid", "relu", 6, "TILED_X6_ALL", S, 2, nst=8, knobs=ALL),
    fwd("all_n8_128x32_probe", (20, 20), 32, 32, 4, 2, "valid", "none", 3, "TILED_X6_ALL", S, 2, nst=8, knobs=ALL,
        probe=True),
    fdense("all_49steps_falls_through_b37", 3136, 256, "relu", 37, "TILED_X6", Lg, 4, xcd=1, knobs=ALL),
    fwd("all_padded_falls_through_b9", (9, 9), 32, 64, 3, 1, "same", "relu", 9, "TILED_X6", Lg, 2, knobs=ALL),
    # ---- LDS-tiled fp32 MFMA on fp32 input (bf16x6 = 0; shapes the register-direct kernel does not take)
    fwd("fp32_ppo_conv3_b9", (9, 9), 32, 64, 3, 1, "valid", "relu", 9, "TILED_FP32", Lg, 2, knobs=FP32),
    fwd("fp32_3x3_64_same_b9", (9, 9), 32, 64, 3, 1, "same", "relu", 9, "TILED_FP32", Lg, 2, knobs=FP32),
    fwd("fp32_5x5x4_b3", (15, 15), 4, 32, 5, 1, "valid", "none", 3, "TILED_FP32", S, 1, knobs=FP32),
    fwd("fp32_3x3_8_32_same_b5", (10, 10), 8, 32, 3, 1, "same", "tanh", 5, "TILED_FP32", S, 1, knobs=FP32),
    fwd("fp32_6x6s2_8_32_b3", (20, 20), 8, 32, 6, 2, "valid", "relu", 3, "TILED_FP32", S, 2, knobs=FP32),
    fwd("fp32_5x5x4_probe", (15, 15), 4, 32, 5, 1, "valid", "none", 2, "TILED_FP32", S, 1, knobs=FP32, probe=True),
]


def wg1(id, hw, cout, k, s, padding, B, path, units, slabs, slab_cap, xform=U8, gather=False, msplit=1, knobs=None,
        probe=False):
    """path: the expected XT_WG1_PATH_* suffix; units / slabs: the expected sub-fields; msplit: the split asked for (the
    generic kernel's; the first-layer kernels choose their own slab count); probe: dY is zero but for one entry"""
    return Wg1Case(id, "conv", hw, 4, cout, k, s, padding, "relu", B, path, units, slabs, xform, gather, msplit, slab_cap,
                   knobs or {}, probe)


def wv(id, hw, s, B, path, units, slabs, slab_cap, **kw):
    return wg1(id, hw, 32, 8, s, "valid", B, path, units, slabs, slab_cap, **kw)


def ws(id, hw, k, B, path, units, slabs, slab_cap, **kw):
    return wg1(id, hw, 16, k, k // 2, "same", B, path, units, slabs, slab_cap, **kw)


# Where the expectations come from (launch_wgrad, launch_conv1_wgrad_bf16x3, launch_conv1_same_wgrad):
#  * VALID 8x8 32 filters: needs slab_cap >= B.  nsteps = ceil(OH*OW / 16) must be in [16, 32] (the combine buffers alias
#    the dY staging; 16 float4 of dY per thread) and H*W*4 + nsteps * 2112 <= 81920 bytes of LDS: 84x84 /4 (25 steps,
#    81024 B), 68x68 /4 and 38x38 /2 (16 steps) pass; 44x44 /4 (7), 52x52 /4 (9) and 64x64 /4 (15) are too small and
#    88x88 /4 (28 steps, 90112 B) too large: generic.  One slab per frame stack (B = 1: straight into dwb), or, from 200
#    blocks of 512 positions with conv1_flat, 8 waves, OH*OW >= 256, S % 4 = 0 and B > 1, one slab per block.  A slab
#    capacity below the block count cannot send the flattened form back to the per-stack one: OH*OW <= 512 makes the
#    block count <= B, and slab_cap < B already keeps the whole launcher out (generic).
#  * SAME: 512 positions from 200 blocks (4x4 kernels too, unlike the forward), else 256; OH*OW >= 256; more blocks than
#    slab_cap: generic.  One block (OH*OW = 256 at B = 1: a 64x64 /4 or 32x32 /2 input) writes dwb.
#  * generic: the split asked for, lowered to ceil(steps / ceil(steps / msplit)) with steps = ceil(M / 32).
WG1_CASES = [
    # ---- VALID, one frame stack per workgroup
    wv("wg1stack_84_b1", (84, 84), 4, 1, "C1_STACK", 8, 1, 4),
    wv("wg1stack_84_b2", (84, 84), 4, 2, "C1_STACK", 8, 2, 4),
    wv("wg1stack_84_b7", (84, 84), 4, 7, "C1_STACK", 8, 7, 16),
    wv("wg1stack_84_b5_cap5", (84, 84), 4, 5, "C1_STACK", 8, 5, 5),
    wv("wg1gen_84_b6_cap5", (84, 84), 4, 6, "GENERIC", 0, 5, 5, msplit=5),             # (75 steps -> 15 each -> 5)
    wv("wg1stack_84_b5_waves4", (84, 84), 4, 5, "C1_STACK", 4, 5, 8, knobs=W4),
    wv("wg1stack_68_b3", (68, 68), 4, 3, "C1_STACK", 8, 3, 4),
    wv("wg1stack_38s2_b3_waves4", (38, 38), 2, 3, "C1_STACK", 4, 3, 4, knobs=W4),
    wv("wg1stack_38s2_b1", (38, 38), 2, 1, "C1_STACK", 8, 1, 4),
    wv("wg1gen_44_b3", (44, 44), 4, 3, "GENERIC", 0, 3, 4, msplit=3),                  # (10 steps -> 4 each -> 3)
    wv("wg1gen_52_b3", (52, 52), 4, 3, "GENERIC", 0, 3, 4, msplit=3),                  # (14 steps -> 5 each -> 3)
    wv("wg1gen_64_b3", (64, 64), 4, 3, "GENERIC", 0, 3, 4, msplit=3),                  # (22 steps -> 8 each -> 3)
    wv("wg1gen_88_b2", (88, 88), 4, 2, "GENERIC", 0, 4, 4, msplit=4),                  # (28 steps -> 7 each -> 4)
    wv("wg1stack_84_b4_std1", (84, 84), 4, 4, "C1_STACK", 8, 4, 4, xform=(1, 0.0, 1.0)),
    wv("wg1stack_84_b6_gather", (84, 84), 4, 6, "C1_STACK", 8, 6, 8, gather=True),
    wv("wg1stack_84_b254", (84, 84), 4, 254, "C1_STACK", 8, 254, 254),
    wv("wg1stack_84_b255_noflat", (84, 84), 4, 255, "C1_STACK", 8, 255, 255, knobs=NOFLAT),
    wv("wg1stack_84_probe", (84, 84), 4, 3, "C1_STACK", 8, 3, 4, probe=True),
    # ---- VALID, 512 flattened positions per workgroup
    wv("wg1flat_84_b255", (84, 84), 4, 255, "C1_FLAT", 512, 200, 255),
    wv("wg1flat_84_b255_gather", (84, 84), 4, 255, "C1_FLAT", 512, 200, 256, gather=True),
    wv("wg1flat_68_b399_probe", (68, 68), 4, 399, "C1_FLAT", 512, 200, 399, probe=True),
    # ---- SAME
    ws("wg1same_84_b1", (84, 84), 8, 1, "C1_SAME", 256, 2, 8),
    ws("wg1same_64_b1_one_block", (64, 64), 8, 1, "C1_SAME", 256, 1, 8),
    ws("wg1same_32_k4_b1_one_block", (32, 32), 4, 1, "C1_SAME", 256, 1, 8),
    ws("wg1same_42_b1", (42, 42), 4, 1, "C1_SAME", 256, 2, 8),
    ws("wg1same_84_b4", (84, 84), 8, 4, "C1_SAME", 256, 7, 8),
    ws("wg1same_42_b4", (42, 42), 4, 4, "C1_SAME", 256, 7, 7),
    ws("wg1same_84_b232", (84, 84), 8, 232, "C1_SAME", 512, 200, 232),
    ws("wg1same_84_b231", (84, 84), 8, 231, "C1_SAME", 256, 398, 400),
    ws("wg1same_42_b232", (42, 42), 4, 232, "C1_SAME", 512, 200, 232),
    ws("wg1same_42_b6_m128", (42, 42), 4, 6, "C1_SAME", 256, 11, 16, xform=(1, 128.0, 128.0)),
    ws("wg1same_84_b5_m128_gather", (84, 84), 8, 5, "C1_SAME", 256, 9, 16, xform=(1, 128.0, 128.0), gather=True),
    ws("wg1same_42_b6_gather", (42, 42), 4, 6, "C1_SAME", 256, 11, 16, gather=True),
    ws("wg1gen_same_84_b4_cap6", (84, 84), 8, 4, "GENERIC", 0, 6, 6, msplit=6),         # (56 steps -> 10 each -> 6)
    ws("wg1same_84_probe", (84, 84), 8, 2, "C1_SAME", 256, 4, 8, probe=True),
    ws("wg1same_42_probe", (42, 42), 4, 3, "C1_SAME", 256, 6, 8, probe=True),
    # ---- generic LDS-tiled fp32 kernel on uint8 input (conv1_bf16x3 = 0)
    wv("wg1gen_ppo_b5_nox3_m1", (84, 84), 4, 5, "GENERIC", 0, 1, 8, msplit=1, knobs=NOX3),
    wv("wg1gen_ppo_b5_nox3_m5", (84, 84), 4, 5, "GENERIC", 0, 5, 8, msplit=5, knobs=NOX3),      # (63 steps -> 13 -> 5)
    ws("wg1gen_imp_b3_nox3_m1", (84, 84), 8, 3, "GENERIC", 0, 1, 8, msplit=1, knobs=NOX3),
    ws("wg1gen_imp_b3_nox3_m5", (84, 84), 8, 3, "GENERIC", 0, 5, 8, msplit=5, knobs=NOX3),      # (42 steps -> 9 -> 5)
    wv("wg1gen_ppo_b4_nox3_gather", (84, 84), 4, 4, "GENERIC", 0, 3, 8, msplit=3, knobs=NOX3, gather=True),  # (50 -> 17 -> 3)
    wv("wg1gen_ppo_probe_nox3", (84, 84), 4, 2, "GENERIC", 0, 2, 8, msplit=2, knobs=NOX3, probe=True),     # (25 -> 13 -> 2)
]

# every non-default value of the knobs the two dispatchers read (the register-direct sizing knobs and the split targets,
# which xt_net applies, left out)
KNOBS = {"conv1_bf16x3": [0], "conv1_flat": [0], "conv1_waves": [4], "fwd_two_groups": [0], "fwd_four_groups": [0],
         "fwd_prefetch_all": [1], "fwd_xcd_chunk": [0], "fwd_tiled_valid": [0], "direct": [0], "direct_fwd": [0],
         "direct_all": [1], "bf16x6": [0]}

ARITH_OF = {"C1_FLAT": "BF16X3", "C1_STACK": "BF16X3", "C1_SAME": "BF16X3", "DIRECT": "FP32", "TILED_FP32": "FP32",
            "TILED_X6": "BF16X6", "TILED_X6_ALL": "BF16X6", "GENERIC": "FP32"}


def header_defines(prefix):
    """{name suffix: value} of the `#define <prefix><suffix> <number>` lines of include/xt_mi355x.h"""
    with open(os.path.join(ROOT, "include", "xt_mi355x.h")) as f:
        return {n: int(v) for n, v in re.findall(r"#define\s+{}(\w+)\s+(\d+)".format(prefix), f.read())}


def fwd_paths():
    return header_defines("XT_FWD_PATH_")


def wg1_paths():
    return header_defines("XT_WG1_PATH_")


def kernel_rows(c):
    return getattr(c, "kh", None) or c.k


def layer_of(c):
    """the oracle's layer; kernel rows != kernel columns (VALID only): the square kernel's layer on an input with k - kh
    more rows, whose first kh * k * C im2col columns are the short kernel's"""
    return nets.LayerSpec(c.id, c.kind, c.cin, c.cout, None, c.k, c.s, c.padding, (c.hw[0] + c.k - kernel_rows(c), c.hw[1]))


def geom_of(L, c, lay):
    g = L.ConvGeom()
    if c.kind == "conv":
        g.H, g.W, g.C, g.KH, g.KW, g.S = c.hw[0], c.hw[1], c.cin, kernel_rows(c), c.k, c.s
        g.PT, g.PL, g.OH, g.OW = lay.pt, lay.pl, lay.out_h, lay.out_w
    else:
        g.H = g.W = g.KH = g.KW = g.S = 1
        g.C = c.cin
        g.PT = g.PL = 0
        g.OH = g.OW = 1
    g.N = c.cout
    g.act = L.ACT[c.act]
    return g


def kdim(c):
    return kernel_rows(c) * c.k * c.cin if c.kind == "conv" else c.cin


# ---------------------------------------------------------------- GPU
FWD_RTOL, WG_RTOL = 2e-6, 3e-6
SENTINEL = np.float32(-1.2345e37)
NAN_BITS = 0x7FC00000
TAIL = 64
COLS_BYTES = 80e6           # im2col chunks stay below this
_KEEP = []


@pytest.fixture(scope="module")
def L():
    from xingtian_amd import lib
    lib.require_gpu()
    lib.load()
    return lib


@pytest.fixture(autouse=True)
def _keepalive():
    _KEEP.clear()
    yield
    torch.cuda.synchronize()
    _KEEP.clear()


def dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    _KEEP.append(t)
    return t


def out_buf(n):
    """n words holding the bits of a NaN, followed by TAIL sentinel floats"""
    a = np.full(n + TAIL, NAN_BITS, np.uint32)
    a[n:] = np.full(TAIL, SENTINEL).view(np.uint32)
    return dev(a.view(np.float32))


def split_out(t, n, what):
    a = t.cpu().numpy()
    assert (a[n:].view(np.uint32) == np.full(TAIL, SENTINEL).view(np.uint32)).all(), "store past the end of " + what
    return a[:n]


def untouched(a):
    return bool((a.view(np.uint32) == NAN_BITS).all())


def rel_err(got, ref):
    return np.linalg.norm((np.asarray(got, np.float64) - ref).ravel()) / (np.linalg.norm(ref.ravel()) + 1e-30)


def max_err_scaled(got, ref):
    return np.abs(np.asarray(got, np.float64) - ref).max() / (np.abs(ref).max() + 1e-30)


def assert_probe(got, ref, ulps, what):
    """every entry within `ulps` fp32 ulp of the float64 reference; entries whose reference is 0 exactly 0"""
    ref32 = np.abs(ref).astype(np.float32)
    tol = ulps * np.spacing(ref32).astype(np.float64)
    tol[ref == 0] = 0.0
    bad = np.abs(got.astype(np.float64) - ref) > tol
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    assert (ref != 0).any(), what        # (the probe reached something)


# Roundings on the single-term path, which bound a probe's error in ulp.  fp32 input: the operand is exact (in bf16 too),
# the three bf16 planes of the other operand add up in two roundings, the fp32 MFMA rounds its product once: 2 (the
# backward probes' bound).  uint8 input: the byte is exact in bf16 and its products with the three planes of the fp32
# operand add up in two roundings (generic kernel: the byte is scaled on load, one rounding, and the MFMA product is one
# more); 1 / std is rounded to fp32 once; the scaling product rounds once: 4.
PROBE_ULPS_F32, PROBE_ULPS_U8 = 2.0, 4.0


def make_input(c, rng):
    """-> (the host copy of the device input: fp32, or a uint8 pool of frame stacks; idx into the pool or None)"""
    shape = (c.B, c.hw[0], c.hw[1], c.cin) if c.kind == "conv" else (c.B, c.cin)
    if not c.xform[0]:
        assert not c.gather
        return rng.standard_normal(shape).astype(np.float32), None
    rows, idx = c.B, None
    if c.gather:      # a small pool; idx repeats rows and ends on the pool's last one
        rows = min(c.B, 37) + 3
        idx = rng.integers(0, rows, c.B).astype(np.int32)
        idx[1] = idx[0]
        idx[-1] = rows - 1
    return rng.integers(0, 256, (rows,) + shape[1:]).astype(np.uint8), idx


def transformed(c, pool, idx, b0, b1):
    """float64 input of samples [b0, b1) as the layer sees it"""
    u8, mean, std = c.xform
    sel = pool[idx[b0:b1]] if idx is not None else pool[b0:b1]
    x = sel.astype(np.float64)
    if u8:
        x = (x - (mean if abs(mean) >= 1e-4 else 0.0)) / std
    return x


def cols_chunks(c, lay, pool, idx):
    """yields (row0, row1, float64 im2col rows) over chunks of samples"""
    kk = kdim(c)
    ohow = lay.out_h * lay.out_w
    per = max(1, int(COLS_BYTES // (ohow * lay.k * lay.k * c.cin * 8))) if c.kind == "conv" else c.B
    for b0 in range(0, c.B, per):
        b1 = min(c.B, b0 + per)
        x = transformed(c, pool, idx, b0, b1)
        if c.kind == "conv":
            extra = c.k - kernel_rows(c)
            if extra:
                x = np.pad(x, ((0, 0), (0, extra), (0, 0), (0, 0)))
            cols = nets.im2col(x, lay)[:, :kk]
        else:
            cols = x.reshape(b1 - b0, -1)
        yield b0 * ohow, b1 * ohow, cols


def run_with_knobs(L, knobs, fn):
    old = L.set_tuning(**knobs) if knobs else {}
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        if old:
            L.set_tuning(**old)


@pytest.mark.parametrize("c", FWD_CASES, ids=[c.id for c in FWD_CASES])
def test_fwd_layer_branch_vs_fp64(L, c):
    lay = layer_of(c)
    rng = np.random.default_rng(zlib.crc32(c.id.encode()))
    pool, idx = make_input(c, rng)
    u8, mean, std = c.xform
    kk, n = kdim(c), c.cout
    m = c.B * lay.out_h * lay.out_w
    w = (rng.standard_normal((kk, n)) / np.sqrt(kk)).astype(np.float32)
    bias = (rng.standard_normal(n) * 0.1).astype(np.float32)
    if c.probe:       # zero input (uint8: the mean) but for the last channel of the bottom-right pixel of the last row read
        bias[:] = 0
        zero = int(mean) if u8 and abs(mean) >= 1e-4 else 0
        pool[:] = zero
        last = idx[-1] if idx is not None else c.B - 1
        pool[last].reshape(-1)[-1] = (zero + 100) if u8 else -1.5      # (both exact in bf16)
    g = geom_of(L, c, lay)
    xf = L.InputXform(u8, mean, std)
    y = out_buf(m * n)
    partial = out_buf(c.ksplit * m * n) if c.ksplit > 1 else None
    mask = out_buf(m)
    path, written = ctypes.c_int32(-1), ctypes.c_int32(-1)
    run_with_knobs(L, c.knobs, lambda: L.check(L.load().xt_layer_fwd_ex(
        ctypes.byref(g), ctypes.byref(xf), c.B, L.ptr(dev(pool)), L.ptr(dev(idx)) if idx is not None else None,
        L.ptr(dev(w)), L.ptr(dev(bias)), L.ptr(y), L.ptr(partial), c.ksplit, None, L.ptr(mask), ctypes.byref(written),
        ctypes.byref(path)), "fwd_layer " + c.id))
    # ---- the branch
    H = header_defines("XT_FWD_")
    v = path.value
    got_path = {"path": v & 0xF, "tile": (v >> H["TILE_SHIFT"]) & 7, "nst": (v >> H["NST_SHIFT"]) & 0xF,
                "xcd": (v >> H["XCD_SHIFT"]) & 1, "arith": (v >> H["ARITH_SHIFT"]) & 3,
                "units": (v >> H["UNITS_SHIFT"]) & 0x3FF, "ks": (v >> H["KSPLIT_SHIFT"]) & 0x7F}
    want = {"path": H["PATH_" + c.path], "tile": H["TILE_" + c.tile] if c.tile else 0, "nst": c.nst, "xcd": c.xcd,
            "arith": header_defines("XT_ARITH_")[ARITH_OF[c.path]], "units": c.units, "ks": c.ks}
    assert got_path == want, (c.id, got_path, want)
    # ---- stores stay inside the buffers; everything the launch owns was written
    got = split_out(y, m * n, "y").reshape(m, n)
    assert np.isfinite(got).all(), c.id
    if partial is not None:
        assert np.isfinite(split_out(partial, c.ksplit * m * n, "partial")[:c.ks * m * n]).all(), c.id
    got_mask = split_out(mask, m, "the relu mask").view(np.uint32)
    # ---- the sign mask: written by the flattened first-layer forward under relu only, from the kernel's own outputs
    if c.path == "C1_FLAT" and c.act == "relu":
        assert written.value == 1, c.id
        bits = ((got > 0).astype(np.uint64) << np.arange(n, dtype=np.uint64)).sum(1).astype(np.uint32)
        wrong = np.flatnonzero(got_mask != bits)
        assert wrong.size == 0, (c.id, "mask words differ", wrong[:4].tolist())
    else:
        assert written.value == 0 and untouched(got_mask), c.id
    # ---- values
    ref = np.empty((m, n))
    w64 = w.astype(np.float64)
    for r0, r1, cols in cols_chunks(c, lay, pool, idx):
        ref[r0:r1] = nets.act_fwd(cols @ w64 + bias, None if c.act == "none" else c.act)
    if c.probe:
        assert_probe(got, ref, PROBE_ULPS_U8 if u8 else PROBE_ULPS_F32, "y")
        return
    re_, me = rel_err(got, ref), max_err_scaled(got, ref)
    print("fwd_layer", c.id, c.path, got_path, "rel {:.2e} max {:.2e}".format(re_, me))
    assert re_ < FWD_RTOL, (c.id, re_)
    assert me < 1e-5, (c.id, me)


@pytest.mark.parametrize("c", WG1_CASES, ids=[c.id for c in WG1_CASES])
def test_first_layer_wgrad_branch_vs_fp64(L, c):
    lay = layer_of(c)
    rng = np.random.default_rng(zlib.crc32(c.id.encode()))
    pool, idx = make_input(c, rng)
    u8, mean, std = c.xform
    kk, n = kdim(c), c.cout
    m = c.B * lay.out_h * lay.out_w
    if c.probe:       # dY zero but for one channel of the last position of the last sample
        dy = np.zeros((m, n), np.float32)
        dy[m - 1, (2 * n) // 3 + 1] = -1.5      # (exact in bf16)
    else:
        dy = rng.standard_normal((m, n)).astype(np.float32)
    g = geom_of(L, c, lay)
    xf = L.InputXform(u8, mean, std)
    nw = (kk + 1) * n
    dwb = out_buf(nw)
    slabs = out_buf(c.slab_cap * nw)
    path = ctypes.c_int32(-1)
    run_with_knobs(L, c.knobs, lambda: L.check(L.load().xt_layer_wgrad_slabs(
        ctypes.byref(g), ctypes.byref(xf), c.B, L.ptr(dev(pool)), L.ptr(dev(idx)) if idx is not None else None,
        L.ptr(dev(dy)), L.ptr(dwb), L.ptr(slabs), c.slab_cap, c.msplit, None, ctypes.byref(path)), "wgrad_slabs " + c.id))
    H = header_defines("XT_WG1_")
    v = path.value
    got_path = {"path": v & 0xF, "arith": (v >> H["ARITH_SHIFT"]) & 3, "units": (v >> H["UNITS_SHIFT"]) & 0x3FF,
                "slabs": v >> H["SLABS_SHIFT"]}
    want = {"path": H["PATH_" + c.path], "arith": header_defines("XT_ARITH_")[ARITH_OF[c.path]], "units": c.units,
            "slabs": c.slabs}
    assert got_path == want, (c.id, got_path, want)
    got = split_out(dwb, nw, "dwb")
    got_slabs = split_out(slabs, c.slab_cap * nw, "the slab buffer")
    assert np.isfinite(got).all(), c.id
    # a single slab goes straight into dwb; more fill exactly their share of the slab buffer
    used = 0 if c.slabs == 1 else c.slabs * nw
    assert np.isfinite(got_slabs[:used]).all() and untouched(got_slabs[used:]), c.id
    got_w, got_b = got[:kk * n].reshape(kk, n), got[kk * n:]
    ref_w = np.zeros((kk, n))
    dy64 = dy.astype(np.float64)
    for r0, r1, cols in cols_chunks(c, lay, pool, idx):
        ref_w += cols.T @ dy64[r0:r1]
    ref_b = dy64.sum(0)
    if c.probe:
        assert_probe(got_w, ref_w, PROBE_ULPS_U8, "dW")
        assert_probe(got_b, ref_b, PROBE_ULPS_U8, "db")
        return
    ew, eb = rel_err(got_w, ref_w), rel_err(got_b, ref_b)
    print("wgrad_slabs", c.id, c.path, got_path, "dW {:.2e} db {:.2e}".format(ew, eb))
    assert ew < WG_RTOL, (c.id, "dW", ew)
    assert eb < WG_RTOL, (c.id, "db", eb)
