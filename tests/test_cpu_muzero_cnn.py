"""CPU tests (no GPU) of the MuzeroCnn entries: ``xt_mz_create_conv`` and ``xt_mz_set_dyn_fused`` check their arguments on
the host, nothing is launched."""
import ctypes

from tests.test_cpu_muzero import PONG, _desc


def test_create_conv_and_dyn_fused_refusals():
    from xingtian_amd import lib as L
    from xingtian_amd.model.muzero.muzero_model import cnn_spec, mlp_spec
    lib = L.load()
    err = lambda: lib.xt_last_error().decode()      # noqa: E731
    xf = L.InputXform(1, 0.0, 255.0)
    spec = cnn_spec((36, 36, 4), 2, 256, 5, **PONG)

    def create(edit=None, xform=xf, **over):
        d, keep = _desc(L, spec, **over)
        if edit:
            edit(keep[0])
        h = ctypes.c_void_p()
        rc = lib.xt_mz_create_conv(ctypes.byref(d), ctypes.byref(xform) if xform else None, 4, ctypes.byref(h))
        return rc, h

    rc, h = create()
    assert rc == 0 and h.value and lib.xt_mz_workspace_bytes(h) > 0, err()
    assert lib.xt_mz_set_dyn_fused(h, 1) == 0 and lib.xt_mz_set_dyn_fused(h, 32) == 0 and lib.xt_mz_set_dyn_fused(h, 0) == 0
    assert lib.xt_mz_set_dyn_fused(h, 8) != 0 and "on = 8" in err()
    lib.xt_mz_destroy(h)
    d, keep = _desc(L, spec)
    assert lib.xt_mz_create(ctypes.byref(d), 4, ctypes.byref(h)) != 0 and "rep layer 0 is not a Dense layer" in err()

    def narrower(rep):          # conv2d_1 claims a 7x7 input, conv2d writes 8x8
        rep[1].g.H = rep[1].g.W = 7
        rep[1].g.OH = rep[1].g.OW = 2
    assert create(narrower)[0] != 0 and "rep layer 1 reads 7x7x32, its producer writes 8x8x32" in err()

    def overhang(rep):          # an output row whose window leaves the image
        rep[0].g.OH = 9
    assert create(overhang)[0] != 0 and "not a VALID convolution" in err()
    assert create(n_rep=3)[0] != 0 and "the rep chain ends in 1x1x64, hidden = 256" in err()
    assert create(xform=None)[0] != 0 and "null input transform" in err()
    assert create(unroll=0)[0] != 0 and "unroll" in err()           # xt_mz_create's own checks stand
    # the fused unroll names the width it cannot take
    d, keep = _desc(L, mlp_spec((4,), 2, 64, 4, 5, **PONG))
    assert lib.xt_mz_create(ctypes.byref(d), 4, ctypes.byref(h)) == 0
    assert lib.xt_mz_set_dyn_fused(h, 1) != 0 and "width of 4" in err()
    assert lib.xt_mz_set_dyn_fused(h, 0) == 0
    lib.xt_mz_destroy(h)
