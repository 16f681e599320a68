/* MuZero, appended under ABI 12: convolutional representation chains (MuzeroCnn) and the fused dynamics unroll.
 * The two entries are declared here, not in xt_mi355x.h: the MuZero section of that header and its ctypes table are
 * pinned entry for entry by tests/test_cpu_muzero.py; xingtian_amd/lib.py keeps these prototypes in MZ_CONV_SIGNATURES. */
#ifndef XT_MZ_CONV_H
#define XT_MZ_CONV_H

#include "xt_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

/* xt_mz_create with a representation chain that may begin with VALID convolution layers (PT == PL == 0, every output
 * pixel's window inside the image) and ends in a 1x1xhidden relu Dense layer; a Dense layer reads its producer's image
 * flattened in (H, W, C) order.  desc->obs_dim is the element count of the first layer's H x W x C image.  The first
 * layer reads the observations through `xf`: {1, 0, 255} uint8 frames as x / 255, {0, 0, 1} float32 as they are; the
 * layer-0 weight gradient reads them the same way.  Every other check, refusal and message is xt_mz_create's.  Refused:
 * a null transform, a convolution that is not VALID, a layer that does not read what its producer writes. */
int xt_mz_create_conv(const xt_mz_desc* desc, const xt_input_xform* xf, int32_t max_batch, xt_mz** out);

/* Switches xt_mz_step between the per-layer dynamics chain (on == 0, the default of every handle: 3 U forward and
 * 3 U + 1 backward launches for a two-layer trunk) and the two persistent kernels of xt_mz_dyn_dev.h (one forward and one
 * backward launch for the whole unroll, on fp32 matrix cores).  on == 1: the measured-best tile of 16 batch rows per
 * workgroup; on == 16 / 32: that many rows.  Refused with the width named unless hidden and every dynamics trunk width
 * are multiples of 16 up to 256.  The fused kernels sum four k at a time: their results differ from the per-layer
 * chain's in the last bits, and are the same bits from run to run.  xt_mz_initial / xt_mz_recurrent are not affected. */
int xt_mz_set_dyn_fused(xt_mz* mz, int32_t on);

#ifdef __cplusplus
}
#endif

#endif /* XT_MZ_CONV_H */
