"""ctypes binding of libdcvic_hip.so (include/dcvic.h, include/dcvic_loss.h, include/dcvic_rate.h, include/dcvic_train.h, include/dcvic_vq.h,
include/dcvic_sample_loss.h, include/dcvic_gumbel.h, include/dcvic_msssim_loss.h, include/dcvic_data.h, include/dcvic_bn.h, include/dcvic_tokens.h).  The library is REQUIRED: there is no
fallback path -- if it is missing or an entry point fails, the caller gets an exception."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DCVIC_LIB_PATH") or os.path.join(_HERE, "libdcvic_hip.so")   # DCVIC_LIB_PATH: diagnostic builds (tools/)

MAX_TAPS = 25
MAX_SRC = 3

ACT_NONE, ACT_RELU, ACT_LRELU02, ACT_SWISH, ACT_GELU, ACT_SIGMOID, ACT_HALF_TANH = range(7)


class ConvDesc(C.Structure):
    _fields_ = [
        ("Cin", C.c_int), ("Cout", C.c_int), ("T", C.c_int),
        ("tap_ky", C.c_int8 * MAX_TAPS), ("tap_kx", C.c_int8 * MAX_TAPS),
        ("tap_dy", C.c_int8 * MAX_TAPS), ("tap_dx", C.c_int8 * MAX_TAPS),
        ("KH", C.c_int), ("KW", C.c_int), ("stride", C.c_int), ("upsample", C.c_int),
        ("transposed_weight", C.c_int), ("cfg", C.c_int),
    ]


class Src(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("C", C.c_int), ("batch_stride", C.c_longlong)]


class ConvIO(C.Structure):
    _fields_ = [
        ("N", C.c_int), ("H", C.c_int), ("W", C.c_int),
        ("Hout", C.c_int), ("Wout", C.c_int), ("Hfull", C.c_int), ("Wfull", C.c_int),
        ("osy", C.c_int), ("osx", C.c_int), ("ooy", C.c_int), ("oox", C.c_int),
        ("n_src", C.c_int), ("src", Src * MAX_SRC),
        ("out", C.c_void_p), ("out_batch_stride", C.c_longlong),
        ("bias", C.c_void_p), ("act", C.c_int),
        ("res", C.c_void_p), ("res_batch_stride", C.c_longlong),
        ("aff_scale", C.c_void_p), ("aff_shift", C.c_void_p), ("aff_batch_stride", C.c_longlong),
        ("init", C.c_void_p), ("init_batch_stride", C.c_longlong),
    ]


class GemmArgs(C.Structure):
    _fields_ = [
        ("batch", C.c_int), ("M", C.c_int), ("N", C.c_int), ("K", C.c_int),
        ("A", C.c_void_p), ("a_bs", C.c_longlong), ("a_ms", C.c_longlong), ("a_ks", C.c_longlong),
        ("B", C.c_void_p), ("b_bs", C.c_longlong), ("b_ks", C.c_longlong), ("b_ns", C.c_longlong),
        ("C", C.c_void_p), ("c_bs", C.c_longlong), ("c_ms", C.c_longlong),
        ("alpha", C.c_float),
    ]


# The C ABI, stated once: every function include/dcvic.h declares as "return:parameters" type codes.  Every pointer parameter (structs
# and the `void* stream` included) is a c_void_p, which takes byref(struct), an int address or None; s = const char* and v = void are
# return types only.  lib() applies the table; tests/test_cabi.py holds it to the header's prototypes type for type.
_CTYPE = {"i": C.c_int, "q": C.c_longlong, "f": C.c_float, "d": C.c_double, "z": C.c_size_t, "p": C.c_void_p, "s": C.c_char_p, "v": None}
SIGNATURES = {
    "dcvic_last_error": "s:", "dcvic_version": "i:", "dcvic_device_info": "i:pp",
    "dcvic_conv_desc_init": "i:piiiiiiii", "dcvic_convT_phase_desc": "i:piiiii", "dcvic_conv_select_class": "i:piii", "dcvic_conv_last_variant": "i:",
    "dcvic_conv_set_tuning": "i:iii", "dcvic_conv_packed_bytes": "z:p", "dcvic_conv_pack_f32": "i:pppp", "dcvic_conv2d_f32": "i:pppp",
    "dcvic_wino_packed_bytes": "z:ii", "dcvic_wino_pack_f32": "i:ppiip", "dcvic_conv3x3_wino_f32": "i:iippp",
    "dcvic_wino_ups_packed_bytes": "z:ii", "dcvic_wino_ups_pack_f32": "i:ppiip", "dcvic_conv3x3_wino_ups_f32": "i:iippp",
    "dcvic_wino44_packed_bytes": "z:ii", "dcvic_wino44_pack_f32": "i:ppiip", "dcvic_conv3x3_wino44_f32": "i:iippp",
    "dcvic_conv3x3_thin_applies": "i:ii", "dcvic_conv3x3_thin_f32": "i:piipp",
    "dcvic_wino44_stats_tiles": "i:ii", "dcvic_conv3x3_wino44_stats_f32": "i:iipppp", "dcvic_groupnorm_part_f32": "i:pqpqppiiiifipip",
    "dcvic_wino44_ups_packed_bytes": "z:ii", "dcvic_wino44_ups_pack_f32": "i:ppiip", "dcvic_conv3x3_wino44_ups_f32": "i:iippp",
    "dcvic_conv3x3_wino44_ups_stats_f32": "i:iipppp",
    "dcvic_conv3x3_bf16_packed_bytes": "z:ii", "dcvic_conv3x3_bf16_mfma_shape": "i:", "dcvic_conv3x3_bf16_pack_f32": "i:ppiip",
    "dcvic_conv3x3_bf16_f32": "i:iiippp",
    "dcvic_bgemm_f32": "i:pp", "dcvic_attn_fused_f32": "i:pppqpqiiifip", "dcvic_groupnorm_f32": "i:pqpqppiiiifip",
    "dcvic_layernorm_c_f32": "i:ppppiiifp", "dcvic_softmax_c_f32": "i:piiip", "dcvic_swin_attn_f32": "i:pppiiiiiiip",
    "dcvic_ew_f32": "i:ipqpqpqpqiiifip", "dcvic_chan_affine_f32": "i:pqpqppqpqiiip", "dcvic_copy_planes_f32": "i:pqiipqiiiiiiip",
    "dcvic_copy_window_f32": "i:pqqqpqqqiiiip", "dcvic_absmax_f32": "i:pqpiqp", "dcvic_crop_clamp_f32": "i:pqiippiiiip",
    "dcvic_vq_argmin_f32": "i:pppppiiiip", "dcvic_argmax_lut_f32": "i:ppppppiiiip", "dcvic_gaussian_rate_f32": "i:pqpppqpipqppqpppiiip",
    "dcvic_rate_blocks": "i:q", "dcvic_neglog2_sum_f32": "i:pqppiqp", "dcvic_eb_rate_f32": "i:ppppppppppiiip",
    "dcvic_pmf_to_quantized_cdf_host": "i:pip", "dcvic_tables_create_host": "p:piipp", "dcvic_tables_destroy_host": "v:p",
    "dcvic_rans_encode_batch_host": "i:pppiqpqpi", "dcvic_rans_decoder_create_host": "p:pq", "dcvic_rans_decoder_destroy_host": "v:p",
    "dcvic_rans_decode_batch_host": "i:pppiqpi",
    # training step (csrc/train.hip)
    "dcvic_conv_wgrad_workspace_floats": "q:iiiiiip", "dcvic_conv_wgrad_f32": "i:pqiiipqiiiiiiiiipipp", "dcvic_chan_reduce_f32": "i:pqpqpiiip",
    "dcvic_sum_rows_f32": "i:ppiqip", "dcvic_ew_bwd_f32": "i:ippppqfiiiqp",
    "dcvic_groupnorm_bwd_f32": "i:pqpqpqppppiiiifip", "dcvic_layernorm_c_bwd_blocks": "i:ii", "dcvic_layernorm_c_bwd_f32": "i:pppppiiifp",
    "dcvic_softmax_c_bwd_f32": "i:pppiiifp",
    "dcvic_swin_attn_bwd_f32": "i:ppppppiiiiiiiip", "dcvic_reduce_loss_f32": "i:ippqidppp", "dcvic_cross_entropy_f32": "i:ppppiiifp",
    "dcvic_adam_step_f32": "i:ppppqffffipp", "dcvic_clip_scale_f32": "i:pfpp",
    "dcvic_resample2_f32": "i:ippqiip", "dcvic_s2d_f32": "i:ppqiiiiiiip", "dcvic_maxpool3s2_f32": "i:pppppqiip",
    "dcvic_lpips_tap_f32": "i:pppppiiifp",
    # OASIS GAN loss (csrc/chan_ce.hip)
    "dcvic_oasis_ce_workspace_doubles": "q:ii", "dcvic_oasis_ce_f32": "i:ppidppppiiip",
    # full-reference metrics (csrc/metrics.hip)
    "dcvic_l2pool_f32": "i:ppqiip", "dcvic_pair_moments_workspace_doubles": "q:qq", "dcvic_pair_moments_f64": "i:ppiiqpqpp",
    "dcvic_dists_score_f64": "i:pqppiipp", "dcvic_lpips_score_f64": "i:piipp",
    # HiFiC patch FID (csrc/fid.hip)
    "dcvic_fid_patch_resize_f32": "i:piipiiiipqp", "dcvic_fid_pool3_f32": "i:ipqiiiipqp", "dcvic_fid_mean_hw_f32": "i:pqiiipqp",
    "dcvic_fid_stats_accum_f64": "i:pqiippp",
    # MS-SSIM and PSNR (csrc/ssim.hip)
    "dcvic_msssim_workspace_bytes": "q:iiii", "dcvic_msssim_psnr_f64": "i:ppiiiippppqp",
}
SYMBOLS = list(SIGNATURES)
# include/dcvic_loss.h: the loss entry points declared outside dcvic.h's frozen table, in the same notation (csrc/chan_ce.hip)
LOSS_SIGNATURES = {
    "dcvic_focal_ce_workspace_doubles": "q:ii", "dcvic_focal_ce_f32": "i:ppddpppiiip",
}
# include/dcvic_rate.h: the differentiable rate term (csrc/rate_train.hip); dcvic_eb_params / dcvic_eb_grads are host structs of 14
# device pointers (matrix0..4, bias0..4, factor0..3), passed by address
RATE_SIGNATURES = {
    "dcvic_gaussian_rate_train_f32": "i:pqppqpqpdpqpqpppqppqpiiip", "dcvic_eb_rate_train_workspace_doubles": "q:iii",
    "dcvic_eb_rate_train_f32": "i:ppppipdpppppppiiip", "dcvic_eb_aux_loss_f32": "i:pppppiip",
}
# include/dcvic_train.h: training-step entry points added after dcvic.h's table was frozen (csrc/train.hip)
TRAIN_SIGNATURES = {
    "dcvic_conv_wgrad_src_f32": "i:pqiiipqiiiiiiiiipiiipp",
}
# include/dcvic_vq.h: which search kernel dcvic_vq_argmin_f32 launched (csrc/vq.hip), and its codes
VQ_SIGNATURES = {
    "dcvic_vq_last_variant": "i:",
}
# include/dcvic_sample_loss.h: the code losses with one weight per image (csrc/sample_loss.hip)
SAMPLE_LOSS_SIGNATURES = {
    "dcvic_focal_ce_sample_workspace_doubles": "q:ii", "dcvic_focal_ce_sample_f32": "i:pppdppppiiip",
    "dcvic_sq_err_sample_workspace_doubles": "q:iq", "dcvic_sq_err_sample_f32": "i:pqppppppiqp",
}
# include/dcvic_gumbel.h: the hard Gumbel-softmax VQ sample of training mode and its straight-through gradient (csrc/gumbel.hip)
GUMBEL_SIGNATURES = {
    "dcvic_gumbel_lut_f32": "i:pppppppdiiiip", "dcvic_gumbel_lut_bwd_f32": "i:pppppdpiiiip",
}
# include/dcvic_msssim_loss.h: the image distortions MSSSIMLoss and L1Loss of the rate-distortion trainer (csrc/msssim_loss.hip)
MSSSIM_LOSS_SIGNATURES = {
    "dcvic_msssim_loss_workspace_bytes": "q:iiii", "dcvic_msssim_loss_f32": "i:ppiiiidppppqp",
    "dcvic_abs_err_workspace_bytes": "q:iq", "dcvic_abs_err_f32": "i:ppqidpppqp",
}
# include/dcvic_data.h: the training data feed's resample / crop / flip / convert launch (csrc/data.hip); dcvic_crop_desc is a struct of
# 3 long long (src_off, tab_x, tab_y) and 6 int (src_h, src_w, src_stride, flip, kx, ky), passed by address (train/data.py DESC_DTYPE)
DATA_SIGNATURES = {
    "dcvic_u8_resample_crop_f32": "i:pqppiippp",
}
DATA_MAX_KSIZE = 17
# include/dcvic_bn.h: per-channel batch statistics and their backward, BatchNorm2d in training mode and ActNorm (csrc/bn_train.hip)
BN_SIGNATURES = {
    "dcvic_bn_workspace_bytes": "q:iii", "dcvic_bn_stats_f32": "i:pqpppqiiip", "dcvic_bn_train_fwd_f32": "i:pqpqppppddppipqiiip",
    "dcvic_bn_train_bwd_f32": "i:pqpqpqppppqppiipqiiip", "dcvic_actnorm_fwd_f32": "i:pqpqppiiiip", "dcvic_actnorm_bwd_f32": "i:pqpqpqpppqppiipqiiip",
}
# include/dcvic_tokens.h: a stored selection set's ingest, uint8 crops to fp32 NCHW and VQ tokens to idx / zq / feat (csrc/tokens.hip)
TOKEN_SIGNATURES = {
    "dcvic_u8_hwc_to_f32_nchw": "i:piiippp", "dcvic_vq_token_feat_f32": "i:pipiiiiipppp",
}
VQ_NONE, VQ_SHARD, VQ_PACKED2, VQ_PACKED1, VQ_LDS4, VQ_LDS8 = range(6)

_lib = None


class DcvicError(RuntimeError):
    pass


def lib() -> C.CDLL:
    """Load the HIP library; raise loudly if it has not been built (no CPU fallback exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise DcvicError(
            f"{LIB_PATH} is missing: build it with `python dc_vic_amd/csrc/build.py` "
            "(or __graft_entry__.build()). dc_vic_amd has no fallback path.")
    L = C.CDLL(LIB_PATH)
    for name, sig in (*SIGNATURES.items(), *LOSS_SIGNATURES.items(), *RATE_SIGNATURES.items(), *TRAIN_SIGNATURES.items(), *VQ_SIGNATURES.items(),
                      *SAMPLE_LOSS_SIGNATURES.items(), *GUMBEL_SIGNATURES.items(), *MSSSIM_LOSS_SIGNATURES.items(),
                      *DATA_SIGNATURES.items(), *BN_SIGNATURES.items(), *TOKEN_SIGNATURES.items()):     # the package's only restype / argtypes assignments; other symbols stay untyped
        fn = getattr(L, name)                # AttributeError names a symbol the library lacks
        ret, params = sig.split(":")
        fn.restype, fn.argtypes = _CTYPE[ret], [_CTYPE[c] for c in params]
    _lib = L
    return L


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = lib().dcvic_last_error()
        raise DcvicError(f"{what} failed (rc={rc}): {msg.decode() if msg else ''}")
