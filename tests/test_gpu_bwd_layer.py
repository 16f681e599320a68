"""GPU parity tests (run with -m gpu on an MI355X) of the fused backward launch (xt_layer_bwd): weight + bias gradient
and input gradient of one non-first trunk layer in ONE launch, the form every SGD step runs.  The launch picks one of
about a dozen kernel instances from the layer geometry and the tuning knobs; every row of BWD_CASES names the branch it
must take (XT_BWD_PATH_* of include/xt_mi355x.h, plus the input-gradient mode), so a case that drifts onto another
kernel fails instead of passing there.  Reference: float64 im2col / col2im products (oracle.nets).

tests/test_cpu_bwd_coverage.py imports BWD_CASES on the CPU and checks that every branch the header declares has cases."""
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

Case = collections.namedtuple("Case", "id kind hw cin cout k s padding act B path dg knobs slab_cap probe")


def case(id, kind, hw, cin, cout, k, s, padding, act, B, path, dg, knobs=None, slab_cap=None, probe=False):
    """act: the PRODUCER's activation ("relu_mask": relu with its sign mask handed to the launch); path: the expected
    XT_BWD_PATH_* suffix; dg: the expected input-gradient mode; slab_cap: None = sized as xt_net_create sizes it;
    probe: dY is zero but for one entry (the last position of the last sample, one channel)"""
    return Case(id, kind, hw, cin, cout, k, s, padding, act, B, path, dg, knobs or {}, slab_cap, probe)


def conv(id, hw, cin, cout, k, s, padding, act, B, path, dg, **kw):
    return case(id, "conv", hw, cin, cout, k, s, padding, act, B, path, dg, **kw)


def dense(id, cin, cout, act, B, path, dg, **kw):
    return case(id, "dense", (1, 1), cin, cout, 1, 1, "valid", act, B, path, dg, **kw)


# Network geometries: PpoCnn 84 / 42 conv2 = 4x4/2 32->32 on 20x20, conv3 = 3x3/1 32->64 on 9x9, Dense 3136->256;
# PpoCnn 30 (inferred filters) conv2 = 5x5/2 16->32 on 13x13, conv3 = 3x3/1 32->64 on 5x5, Dense 576->64;
# ImpalaCnnOpt 84 / 42 conv2 = 4x4/2 SAME 16->32 on 21x21, conv3 (collapses the 11x11 map) = Dense 3872->256;
# PpoMlp = Dense 64->64.
BWD_CASES = [
    # ---- 4x4/2 16->32, B >= 512 and 512 slabs: input + weight gradient per sample
    conv("s2fused_imp_b512", (21, 21), 16, 32, 4, 2, "same", "relu", 512, "S2FUSED", 5),
    conv("s2fused_imp_b600_tanh", (21, 21), 16, 32, 4, 2, "same", "tanh", 600, "S2FUSED", 5),
    conv("s2fused_22_valid_b513", (22, 22), 16, 32, 4, 2, "valid", "none", 513, "S2FUSED", 5),
    conv("s2fused_imp_probe", (21, 21), 16, 32, 4, 2, "same", "relu", 512, "S2FUSED", 5, probe=True),
    # ---- ... below 512 samples or slabs: sample-per-workgroup input gradient, tiled weight gradient
    conv("s2c16_imp_b40", (21, 21), 16, 32, 4, 2, "same", "relu", 40, "S2C16", 5),
    conv("s2c16_imp_b1", (21, 21), 16, 32, 4, 2, "same", "relu", 1, "S2C16", 5),
    conv("s2c16_imp_b511", (21, 21), 16, 32, 4, 2, "same", "relu", 511, "S2C16", 5),
    conv("s2c16_imp_b512_cap511", (21, 21), 16, 32, 4, 2, "same", "relu", 512, "S2C16", 5, slab_cap=511),
    conv("s2c16_22_valid_b7_swish", (22, 22), 16, 32, 4, 2, "valid", "swish", 7, "S2C16", 5),
    conv("s2c16_22_valid_b150_nodeep", (22, 22), 16, 32, 4, 2, "valid", "tanh", 150, "S2C16", 5,
         knobs=dict(bwd_deep_prefetch=0)),
    conv("s2c16_imp_probe", (21, 21), 16, 32, 4, 2, "same", "relu", 3, "S2C16", 5, probe=True),
    # ---- stride-1 halo input gradient in its own instance (more than 512 register-direct tiles)
    conv("halo_ppo_b320", (9, 9), 32, 64, 3, 1, "valid", "relu", 320, "HALO", 4),
    conv("halo_ppo_b261_tanh", (9, 9), 32, 64, 3, 1, "valid", "tanh", 261, "HALO", 4),
    conv("halo_ppo_b203", (9, 9), 32, 64, 3, 1, "valid", "relu", 203, "HALO", 4),
    conv("halo_ppo30_b700", (5, 5), 32, 64, 3, 1, "valid", "relu", 700, "HALO", 4),
    conv("halo_n128_b700", (5, 5), 32, 128, 3, 1, "valid", "none", 700, "HALO", 4),
    conv("halo_fp32_10x10_b200", (10, 10), 32, 64, 3, 1, "valid", "relu", 200, "HALO", 4),
    conv("halo_ppo_b320_nofit", (9, 9), 32, 64, 3, 1, "valid", "relu", 320, "HALO", 4, knobs=dict(bwd_fit_slots=0)),
    conv("halo_ppo_probe", (9, 9), 32, 64, 3, 1, "valid", "relu", 210, "HALO", 4, probe=True),
    # ---- all four stride-parity classes per block, four taps in flight, launch cut to 512 workgroups
    conv("pf4_ppo_b320_mask", (20, 20), 32, 32, 4, 2, "valid", "relu_mask", 320, "CLASSES_PF4", 2),
    conv("pf4_ppo_b320", (20, 20), 32, 32, 4, 2, "valid", "relu", 320, "CLASSES_PF4", 2),
    conv("pf4_ppo_b32_gelu", (20, 20), 32, 32, 4, 2, "valid", "gelu", 32, "CLASSES_PF4", 2),
    conv("pf4_ppo_b1", (20, 20), 32, 32, 4, 2, "valid", "relu_mask", 1, "CLASSES_PF4", 2),
    conv("pf4_ppo_b614", (20, 20), 32, 32, 4, 2, "valid", "tanh", 614, "CLASSES_PF4", 2),
    conv("pf4_22_b37_mask", (22, 22), 32, 32, 4, 2, "valid", "relu_mask", 37, "CLASSES_PF4", 2),
    conv("pf4_16_b90", (16, 16), 32, 32, 4, 2, "valid", "none", 90, "CLASSES_PF4", 2),
    conv("pf4_ppo_probe", (20, 20), 32, 32, 4, 2, "valid", "relu_mask", 5, "CLASSES_PF4", 2, probe=True),
    # ---- ... next to the staged-rows weight gradient (wgrad_rows = 1 / 2, not the default)
    conv("wrows1_ppo_b320", (20, 20), 32, 32, 4, 2, "valid", "relu_mask", 320, "CLASSES_WROWS", 2,
         knobs=dict(wgrad_rows=1)),
    conv("wrows1_ppo_b32", (20, 20), 32, 32, 4, 2, "valid", "relu", 32, "CLASSES_WROWS", 2, knobs=dict(wgrad_rows=1)),
    conv("wrows2_ppo_b100", (20, 20), 32, 32, 4, 2, "valid", "tanh", 100, "CLASSES_WROWS", 2, knobs=dict(wgrad_rows=2)),
    conv("wrows2_ppo_b1", (20, 20), 32, 32, 4, 2, "valid", "relu_mask", 1, "CLASSES_WROWS", 2, knobs=dict(wgrad_rows=2)),
    conv("wrows1_16_b65", (16, 16), 32, 32, 4, 2, "valid", "relu", 65, "CLASSES_WROWS", 2, knobs=dict(wgrad_rows=1)),
    conv("wrows1_ppo_probe", (20, 20), 32, 32, 4, 2, "valid", "relu_mask", 70, "CLASSES_WROWS", 2, probe=True,
         knobs=dict(wgrad_rows=1)),
    # ---- ... plain form: more than 480 class tiles, nine taps per class, or a knob
    conv("classes_ppo_b615_mask", (20, 20), 32, 32, 4, 2, "valid", "relu_mask", 615, "CLASSES", 2),
    conv("classes_6x6_b9", (20, 20), 32, 32, 6, 2, "valid", "relu", 9, "CLASSES", 2),
    conv("classes_6x6_b1_mask", (20, 20), 32, 32, 6, 2, "valid", "relu_mask", 1, "CLASSES", 2),
    conv("classes_ppo_b64_rows0", (20, 20), 32, 32, 4, 2, "valid", "tanh", 64, "CLASSES", 2, knobs=dict(wgrad_rows=0)),
    conv("classes_ppo_b50_fp32", (20, 20), 32, 32, 4, 2, "valid", "relu_mask", 50, "CLASSES", 2,
         knobs=dict(bf16x6=0)),
    conv("classes_6x6_probe", (20, 20), 32, 32, 6, 2, "valid", "relu", 3, "CLASSES", 2, probe=True),
    # ---- Dense deep-prefetch instance
    dense("pfg_ppo_dense_b320", 3136, 256, "relu", 320, "PF_GENERIC", 0),
    dense("pfg_ppo_dense_b1", 3136, 256, "relu", 1, "PF_GENERIC", 0),
    dense("pfg_ppo_dense_b384", 3136, 256, "tanh", 384, "PF_GENERIC", 0),
    dense("pfg_mlp_b200", 64, 64, "tanh", 200, "PF_GENERIC", 0),
    dense("pfg_mlp_b1024_swish", 64, 64, "swish", 1024, "PF_GENERIC", 0),
    dense("pfg_512_64_b1024", 512, 64, "relu", 1024, "PF_GENERIC", 0),
    dense("pfg_ppo30_dense_b50", 576, 64, "none", 50, "PF_GENERIC", 0),
    dense("pfg_ppo_dense_b320_wx6off", 3136, 256, "relu", 320, "PF_GENERIC", 0, knobs=dict(dense_wgrad_x6=0)),
    dense("pfg_512_64_probe", 512, 64, "relu", 77, "PF_GENERIC", 0, probe=True),
    # ---- generic tile pairs: 128x32 weight gradient + 128x32 input gradient
    conv("ss_ppo_b48_noclasses", (20, 20), 32, 32, 4, 2, "valid", "relu", 48, "PAIR_SS", 0,
         knobs=dict(dgrad_all_classes=0)),
    conv("ss_ppo30_conv2_b50", (13, 13), 16, 32, 5, 2, "valid", "relu", 50, "PAIR_SS", 0),
    conv("ss_3x3_32_b1", (9, 9), 32, 32, 3, 1, "valid", "tanh", 1, "PAIR_SS", 1),
    conv("ss_3x3_32_b33_same", (9, 9), 32, 32, 3, 1, "same", "relu", 33, "PAIR_SS", 1),
    conv("ss_ppo30_conv2_probe", (13, 13), 16, 32, 5, 2, "valid", "relu", 4, "PAIR_SS", 0, probe=True),
    # ---- 128x32 weight gradient + 64x64 input gradient
    conv("sl_3x3_64_32_b40", (9, 9), 64, 32, 3, 1, "valid", "relu", 40, "PAIR_SL", 0),
    conv("sl_3x3_64_32_b1_same", (7, 7), 64, 32, 3, 1, "same", "tanh", 1, "PAIR_SL", 0),
    conv("sl_3x3_64_32_probe", (9, 9), 64, 32, 3, 1, "valid", "relu", 3, "PAIR_SL", 0, probe=True),
    # ---- 64x64 weight gradient + 128x32 input gradient (register-direct input gradient modes 1 / 3 / 4)
    conv("ls_ppo_b48", (9, 9), 32, 64, 3, 1, "valid", "relu", 48, "PAIR_LS", 1),
    conv("ls_ppo30_conv3_b50", (5, 5), 32, 64, 3, 1, "valid", "relu", 50, "PAIR_LS", 1),
    conv("ls_ppo_b1", (9, 9), 32, 64, 3, 1, "valid", "gelu", 1, "PAIR_LS", 1),
    conv("ls_ppo_b320_tile32", (9, 9), 32, 64, 3, 1, "valid", "relu", 320, "PAIR_LS", 1,
         knobs=dict(dgrad_tile64=0)),
    conv("ls_ppo_b320_nohalo", (9, 9), 32, 64, 3, 1, "valid", "tanh", 320, "PAIR_LS", 3, knobs=dict(dgrad_halo=0)),
    conv("ls_ppo_b261_noown", (9, 9), 32, 64, 3, 1, "valid", "relu", 261, "PAIR_LS", 4,
         knobs=dict(bwd_own_instance=0)),
    conv("ls_same_b300", (9, 9), 32, 64, 3, 1, "same", "relu", 300, "PAIR_LS", 3),
    conv("ls_ppo_probe", (9, 9), 32, 64, 3, 1, "valid", "relu", 2, "PAIR_LS", 1, probe=True),
    # ---- 64x64 pair
    dense("ll_imp_dense_b40", 3872, 256, "relu", 40, "PAIR_LL", 1),
    dense("ll_imp_dense_b200", 3872, 256, "relu", 200, "PAIR_LL", 3),
    conv("ll_3x3_64_same_b20", (9, 9), 64, 64, 3, 1, "same", "tanh", 20, "PAIR_LL", 0),
    conv("ll_3x3_64_b1_fp32", (9, 9), 64, 64, 3, 1, "valid", "relu", 1, "PAIR_LL", 0, knobs=dict(bf16x6=0)),
    dense("ll_imp_dense_probe", 3872, 256, "relu", 3, "PAIR_LL", 1, probe=True),
    # ---- 64x64 pair with the bf16x6 weight gradient
    dense("llx6_ppo_dense_b385", 3136, 256, "relu", 385, "PAIR_LL_WX6", 0),
    dense("llx6_ppo_dense_b320_nodeep", 3136, 256, "tanh", 320, "PAIR_LL_WX6", 0, knobs=dict(bwd_deep_prefetch=0)),
    conv("llx6_3x3_64_b37", (9, 9), 64, 64, 3, 1, "valid", "relu", 37, "PAIR_LL_WX6", 0),
    conv("llx6_3x3_64_b1", (7, 7), 64, 64, 3, 1, "valid", "none", 1, "PAIR_LL_WX6", 0),
    conv("llx6_3x3_64_probe", (9, 9), 64, 64, 3, 1, "valid", "relu", 2, "PAIR_LL_WX6", 0, probe=True),
]

# the knobs the header documents, each with its non-default value(s) (EXPERIMENT values left out:
# dense_wgrad_x6 = 2, wgrad_rows = 3)
KNOBS = {"bf16x6": [0], "dgrad_all_classes": [0], "dgrad_tile64": [0], "dgrad_halo": [0], "bwd_own_instance": [0],
         "bwd_fit_slots": [0], "wgrad_rows": [0, 1, 2], "bwd_deep_prefetch": [0], "dense_wgrad_x6": [0]}


def header_paths():
    """{name suffix: value} of the XT_BWD_PATH_* branches include/xt_mi355x.h declares"""
    with open(os.path.join(ROOT, "include", "xt_mi355x.h")) as f:
        return {n: int(v) for n, v in re.findall(r"#define\s+XT_BWD_PATH_(\w+)\s+(\d+)", f.read())}


def header_int(name):
    with open(os.path.join(ROOT, "include", "xt_mi355x.h")) as f:
        return int(re.search(r"#define\s+{}\s+(\d+)".format(name), f.read()).group(1))


def layer_of(c):
    return nets.LayerSpec(c.id, c.kind, c.cin, c.cout, None, c.k, c.s, c.padding, c.hw)


def geom_of(L, lay):
    g = L.ConvGeom()
    if lay.kind == "conv":
        g.H, g.W, g.C, g.KH, g.KW, g.S = lay.in_h, lay.in_w, lay.cin, lay.k, lay.k, lay.s
        g.PT, g.PL, g.OH, g.OW = lay.pt, lay.pl, lay.out_h, lay.out_w
    else:
        g.H = g.W = g.KH = g.KW = g.S = 1
        g.C = lay.cin
        g.PT = g.PL = 0
        g.OH = g.OW = 1
    g.N = lay.cout
    g.act = L.ACT["relu"]
    return g


def net_split_and_cap(lay, B):
    """the weight-gradient split and the slab capacity xt_net_create / trunk_backward give a non-first layer
    (wgrad_split and the slab bound of xt_net.hip) at max_batch = B"""
    kk = lay.k * lay.k * lay.cin if lay.kind == "conv" else lay.cin
    n, m = lay.cout, B * lay.out_h * lay.out_w
    tiles = -(-kk // 128) * -(-n // 32) if n <= 32 else -(-kk // 64) * -(-n // 64)
    split = max(1, min(512 // tiles, -(-m // 32) // 4))
    cap_tiles = -(-kk // 128) if n <= 32 else -(-kk // 64) * -(-n // 64)
    cap = max(1, 512 // cap_tiles)
    if lay.kind == "conv" and lay.s == 2 and lay.k == 4 and lay.cin == 16 and n == 32 and B >= 512:
        cap = max(cap, 512)
    return split, cap


def decode_path(v):
    return v & 0xFF, (v >> header_int("XT_BWD_DG_SHIFT")) & 0xF, v >> header_int("XT_BWD_ARITH_SHIFT")


# ---------------------------------------------------------------- GPU
RTOL = 3e-6
SENTINEL = np.float32(-1.2345e37)
TAIL = 64
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


def out_buf(n, fill=float("nan")):
    """n floats prefilled with `fill`, followed by TAIL sentinel floats"""
    t = torch.full((n + TAIL,), fill, dtype=torch.float32, device="cuda")
    t[n:] = float(SENTINEL)
    _KEEP.append(t)
    return t


def split_out(t, n, what):
    a = t.cpu().numpy()
    assert (a[n:].view(np.uint32) == np.full(TAIL, SENTINEL).view(np.uint32)).all(), "store past the end of " + what
    return a[:n]


def rel_err(got, ref):
    return np.linalg.norm((np.asarray(got, np.float64) - ref).ravel()) / (np.linalg.norm(ref.ravel()) + 1e-30)


def max_err_scaled(got, ref):
    return np.abs(np.asarray(got, np.float64) - ref).max() / (np.abs(ref).max() + 1e-30)


def assert_probe(got, ref, what):
    """every entry within 2 fp32 ulp of the float64 reference; entries whose reference is 0 exactly 0"""
    ref32 = np.abs(ref).astype(np.float32)
    tol = 2.0 * np.spacing(ref32).astype(np.float64)
    tol[ref == 0] = 0.0
    bad = np.abs(got.astype(np.float64) - ref) > tol
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    assert (ref != 0).any(), what        # (the probe reached something)


def make_data(c, lay, rng):
    b = c.B
    act = "relu" if c.act == "relu_mask" else c.act
    z = rng.standard_normal((b, lay.in_h, lay.in_w, lay.cin)).astype(np.float32)
    if act in nets.NEEDS_PREACT:
        x = nets.act_fwd(z.astype(np.float64), act).astype(np.float32)
    elif act == "none":
        x = z
    else:
        x = nets.act_fwd(z.astype(np.float64), act).astype(np.float32)
    kk = lay.k * lay.k * lay.cin if lay.kind == "conv" else lay.cin
    w = (rng.standard_normal((kk, lay.cout)) / np.sqrt(kk)).astype(np.float32)
    m = b * lay.out_h * lay.out_w
    if c.probe:
        dy = np.zeros((m, lay.cout), np.float32)
        dy[m - 1, (2 * lay.cout) // 3 + 1] = -1.5      # (exact in bf16: the bf16x6 forms multiply it exactly)
    else:
        dy = rng.standard_normal((m, lay.cout)).astype(np.float32)
    return act, z, x, w, dy


def reference(lay, act, z, x, w, dy):
    b = x.shape[0]
    x64 = x.astype(np.float64)
    cols = nets.im2col(x64, lay) if lay.kind == "conv" else x64.reshape(b, -1)
    dy64 = dy.astype(np.float64)
    ref_w = cols.T @ dy64
    ref_b = dy64.sum(0)
    dcols = dy64 @ w.astype(np.float64).T
    dxs = nets.col2im(dcols, lay, b) if lay.kind == "conv" else dcols.reshape(x.shape)
    if act in nets.NEEDS_PREACT:
        ref_x = nets.act_bwd(dxs, None, act, z.astype(np.float64))
    else:
        ref_x = nets.act_bwd(dxs, x64, act)
    return ref_w, ref_b, ref_x


@pytest.mark.parametrize("c", BWD_CASES, ids=[c.id for c in BWD_CASES])
def test_bwd_layer_branch_vs_fp64(L, c):
    lay = layer_of(c)
    rng = np.random.default_rng(zlib.crc32(c.id.encode()))
    act, z, x, w, dy = make_data(c, lay, rng)
    g = geom_of(L, lay)
    msplit, cap = net_split_and_cap(lay, c.B)
    if c.slab_cap is not None:
        cap = c.slab_cap
    kk = w.shape[0]
    nw = (kk + 1) * lay.cout
    dx = out_buf(x.size)
    dwb = out_buf(nw)
    slabs = out_buf(cap * nw)
    mask = None
    if c.act == "relu_mask":
        bits = (x.reshape(-1, lay.cin) > 0).astype(np.uint64) << np.arange(lay.cin, dtype=np.uint64)
        mask = dev(bits.sum(1).astype(np.uint32).view(np.int32))
    path = ctypes.c_int32(-1)
    old = L.set_tuning(**c.knobs) if c.knobs else {}
    try:
        L.check(L.load().xt_layer_bwd(ctypes.byref(g), c.B, L.ptr(dev(x)),
                                      L.ptr(dev(z)) if act in nets.NEEDS_PREACT else None, L.ptr(dev(dy)), L.ptr(dev(w)),
                                      L.ACT[act], L.ptr(mask), L.ptr(dx), L.ptr(dwb), L.ptr(slabs), cap, msplit, None,
                                      ctypes.byref(path)), "bwd_layer " + c.id)
        torch.cuda.synchronize()
    finally:
        if old:
            L.set_tuning(**old)
    paths = header_paths()
    p, dg, arith = decode_path(path.value)
    assert (p, dg) == (paths[c.path], c.dg), (c.id, {v: k for k, v in paths.items()}.get(p, p), dg, arith)
    got_x = split_out(dx, x.size, "dx").reshape(x.shape)
    got_wb = split_out(dwb, nw, "dwb")
    split_out(slabs, cap * nw, "the slab buffer")
    assert np.isfinite(got_x).all() and np.isfinite(got_wb).all(), c.id
    got_w, got_b = got_wb[:kk * lay.cout].reshape(kk, lay.cout), got_wb[kk * lay.cout:]
    ref_w, ref_b, ref_x = reference(lay, act, z, x, w, dy)
    if c.probe:
        assert_probe(got_w, ref_w, "dW")
        assert_probe(got_b, ref_b, "db")
        assert_probe(got_x, ref_x, "dX")
        return
    errs = {"dW": (rel_err(got_w, ref_w), max_err_scaled(got_w, ref_w)),
            "db": (rel_err(got_b, ref_b), max_err_scaled(got_b, ref_b)),
            "dX": (rel_err(got_x, ref_x), max_err_scaled(got_x, ref_x))}
    print("bwd_layer", c.id, c.path, "dg", dg, "arith", arith, " ".join(
        "{} {:.2e}/{:.2e}".format(k, *v) for k, v in errs.items()))
    for k, (re_, me) in errs.items():
        assert re_ < RTOL, (c.id, k, re_)
        assert me < 1e-5, (c.id, k, me)
