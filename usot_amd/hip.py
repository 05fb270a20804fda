"""ctypes binding of libusot_hip.so (the C ABI declared in include/usot_hip.h).

There is no fallback: if the shared library is missing or an entry point fails, the call
raises.  torch is used only for device memory and the current HIP stream.
"""
import ctypes as C
import os

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'csrc', 'libusot_hip.so')

ACT_NONE, ACT_RELU, ACT_EXP, ACT_CONF = 0, 1, 2, 3

EXPORTS = (
    'usot_abi_version', 'usot_device_guard', 'usot_device_slot', 'usot_strerror', 'usot_conv2d_f32', 'usot_conv_tile_count',
    'usot_conv_tile_info', 'usot_conv_tile_built', 'usot_experiments_built', 'usot_conv_bf16_tile_built', 'usot_conv_bf16_tile_info', 'usot_conv_tile_name', 'usot_conv_tile_launch', 'usot_conv_tile_wfrag', 'usot_conv_tile_xsplit', 'usot_conv_tile_kreq', 'usot_conv_tile_streamk', 'usot_conv_streamk_ws_floats', 'usot_conv_pack_wfrag_f32', 'usot_conv_ws_floats', 'usot_stem_conv_f32', 'usot_maxpool3x3s2_f32',
    'usot_xcorr_depthwise_f32', 'usot_groupdw_f32', 'usot_conf_fusion_reduce_f32',
    'usot_prroi_pool_forward_f32', 'usot_prroi_pool_backward_f32', 'usot_prroi_pool_coor_backward_f32', 'usot_permute4_f32', 'usot_decode_f32',
    'usot_plan_create', 'usot_plan_destroy', 'usot_plan_add_conv', 'usot_plan_add_stem',
    'usot_plan_add_maxpool', 'usot_plan_add_groupdw', 'usot_plan_add_conf_reduce',
    'usot_plan_add_prroi', 'usot_plan_add_permute', 'usot_plan_add_decode', 'usot_plan_run',
    'usot_plan_fork', 'usot_plan_join', 'usot_plan_capture', 'usot_plan_size',
    'usot_groupdw_multi_f32', 'usot_plan_add_groupdw_multi', 'usot_groupdw_multi_lp', 'usot_plan_add_groupdw_multi_lp', 'usot_conf_fusion_reduce_lp', 'usot_plan_add_conf_reduce_lp', 'usot_conv2d_batch_f32', 'usot_plan_add_conv_batch', 'usot_conv2d_bf16', 'usot_conv_bf16_tile_count', 'usot_cvt_f32_to_bf16', 'usot_maxpool3x3s2_bf16',
    'usot_plan_add_conv_bf16', 'usot_plan_add_cvt_bf16', 'usot_plan_add_maxpool_bf16',
    'usot_conv2d_lp', 'usot_cvt_f32_to_lp', 'usot_maxpool3x3s2_lp', 'usot_plan_add_conv_lp', 'usot_plan_add_cvt_lp',
    'usot_plan_add_maxpool_lp', 'usot_stem_pool_lp', 'usot_plan_add_stem_pool_lp',
    'usot_rows_copy_multi_f32', 'usot_plan_add_rows_copy_multi', 'usot_rows_append_gather_f32', 'usot_plan_add_rows_append_gather', 'usot_thin_conv3x3_f32', 'usot_plan_add_thin_conv', 'usot_stem_pool_f32', 'usot_plan_add_stem_pool',
    'usot_plan_profile', 'usot_plan_op_info', 'usot_rows_copy_f32', 'usot_plan_add_rows_copy', 'usot_crop_resize_u8_f32', 'usot_conv_resolve_tile', 'usot_decode_dev_f32',
    'PrRoIPoolingForwardGpu', 'usot_groupdw_auto_variant',
    'usot_stem_pool_ind_f32', 'usot_plan_add_stem_pool_ind', 'usot_bw_probe', 'usot_conv_kstream_lp', 'usot_conv_kstream_supported', 'usot_plan_add_conv_kstream', 'usot_pw_kstream_lp', 'usot_pw_kstream_supported', 'usot_plan_add_pw_kstream', 'usot_conv3x3_halo_lp', 'usot_conv3x3_halo_supported', 'usot_plan_add_conv3x3_halo', 'usot_bneck_first_lp', 'usot_bneck_first_supported', 'usot_plan_add_bneck_first', 'usot_bneck_tail_lp', 'usot_bneck_tail_supported', 'usot_plan_add_bneck_tail', 'usot_pw_panel_lp', 'usot_pw_panel_supported', 'usot_pw_panel_pixels', 'usot_pw_panel_min_pixels', 'usot_plan_add_pw_panel', 'usot_pw_panel_pair_lp', 'usot_pw_panel_pair_supported', 'usot_plan_add_pw_panel_pair', 'usot_conv_pw_lp', 'usot_conv_pw_supported', 'usot_conv_pw_pixels', 'usot_plan_add_conv_pw', 'usot_conv_pw_pair_lp', 'usot_conv_pw_pair_supported', 'usot_plan_add_conv_pw_pair', 'usot_conv_pw_ov_lp', 'usot_conv_pw_ov_supported', 'usot_conv_pw_ov_ws_bytes', 'usot_plan_add_conv_pw_ov', 'usot_conv_pw_ov_trace', 'usot_stem_conv_mu_f32', 'usot_stem_pool_mu_f32', 'usot_plan_add_stem_pool_mu', 'usot_plan_add_stem_mu', 'usot_pw_pair_lp', 'usot_pw_pair_layout', 'usot_pw_pair_supported', 'usot_plan_add_pw_pair', 'usot_pw_pair_f32', 'usot_pw_pair_f32s', 'usot_pw_pair_f32s_supported', 'usot_pw_pair_f32_supported', 'usot_pw_pair_f32_ws_floats', 'usot_pw_single_f32', 'usot_pw_single_f32_supported', 'usot_plan_add_pw_single', 'usot_stream_conv3x3_f32', 'usot_stream_conv3x3_f32_supported', 'usot_plan_add_stream_conv3x3', 'usot_pw_triple_f32', 'usot_pw_triple_f32_supported', 'usot_plan_add_pw_triple',
    'usot_decode_batch_f32', 'usot_plan_add_decode_batch', 'usot_rows_append_gather_batch_f32', 'usot_plan_add_rows_append_gather_batch',
    'usot_crop_resize_batch_u8_f32', 'usot_plan_add_crop_resize_batch',
    'usot_xcorr_depthwise_bwd_x_f32', 'usot_xcorr_depthwise_bwd_k_f32',
    'usot_rows_append_gather_dedupe_f32', 'usot_plan_add_rows_append_gather_dedupe', 'usot_groupdw_multi_dyn_f32',
    'usot_plan_add_groupdw_multi_dyn', 'usot_conf_fusion_reduce_map_f32', 'usot_plan_add_conf_reduce_map', 'usot_conv_tile_dyn',
    'usot_conv2d_wgrad_f32', 'usot_conv2d_dgrad_f32', 'usot_conv2d_wgrad_ws_floats', 'usot_conv2d_wgrad_psplit', 'usot_conv2d_wgrad_geometry',
    'usot_conv_pack_dgrad_f32', 'usot_conv2d_dgrad_route',
    'usot_batchnorm_fwd_f32', 'usot_batchnorm_bwd_f32', 'usot_batchnorm_ws_floats', 'usot_batchnorm_slices', 'usot_batchnorm_geometry',
    'usot_stem_pool_lp_strip',
)


class HipError(RuntimeError):
    pass


class ConvDesc(C.Structure):
    _fields_ = [('x', C.c_void_p), ('w', C.c_void_p), ('bias', C.c_void_p), ('res', C.c_void_p),
                ('y', C.c_void_p), ('ws', C.c_void_p),
                ('N', C.c_int32), ('H', C.c_int32), ('W', C.c_int32), ('Cin', C.c_int32),
                ('OH', C.c_int32), ('OW', C.c_int32), ('Cout', C.c_int32),
                ('KH', C.c_int32), ('KW', C.c_int32), ('stride', C.c_int32),
                ('pad_h', C.c_int32), ('pad_w', C.c_int32), ('dil_h', C.c_int32), ('dil_w', C.c_int32),
                ('y_cstride', C.c_int32), ('y_coff', C.c_int32), ('res_cstride', C.c_int32),
                ('res_coff', C.c_int32), ('y_nchw', C.c_int32),
                ('act', C.c_int32), ('act2', C.c_int32), ('act_split', C.c_int32),
                ('groups', C.c_int32),
                ('x_gs', C.c_int64), ('w_gs', C.c_int64), ('b_gs', C.c_int64), ('y_gs', C.c_int64),
                ('r_gs', C.c_int64),
                ('ksplit', C.c_int32), ('tile', C.c_int32), ('w_frag', C.c_int32), ('defer', C.c_int32),
                ('w_scale', C.c_void_p), ('x_split', C.c_int32), ('y_split', C.c_int32), ('ovf', C.c_void_p),
                ('n_dyn', C.c_void_p), ('n_first', C.c_int32)]


class GradDesc(C.Structure):
    """usot_conv_grad_desc"""
    _fields_ = [('x', C.c_void_p), ('w', C.c_void_p), ('wt', C.c_void_p), ('dy', C.c_void_p),
                ('dx', C.c_void_p), ('dw', C.c_void_p), ('db', C.c_void_p), ('ws', C.c_void_p),
                ('N', C.c_int32), ('H', C.c_int32), ('W', C.c_int32), ('Cin', C.c_int32),
                ('OH', C.c_int32), ('OW', C.c_int32), ('Cout', C.c_int32),
                ('KH', C.c_int32), ('KW', C.c_int32), ('stride', C.c_int32),
                ('pad_h', C.c_int32), ('pad_w', C.c_int32), ('dil_h', C.c_int32), ('dil_w', C.c_int32),
                ('psplit', C.c_int32), ('route', C.c_int32)]


class BnDesc(C.Structure):
    """usot_bn_desc"""
    _fields_ = [('x', C.c_void_p), ('gamma', C.c_void_p), ('beta', C.c_void_p), ('running_mean', C.c_void_p),
                ('running_var', C.c_void_p), ('y', C.c_void_p), ('save_mean', C.c_void_p), ('save_invstd', C.c_void_p),
                ('dy', C.c_void_p), ('dx', C.c_void_p), ('dgamma', C.c_void_p), ('dbeta', C.c_void_p), ('ws', C.c_void_p),
                ('M', C.c_int32), ('C', C.c_int32), ('eps', C.c_float), ('momentum', C.c_float),
                ('training', C.c_int32), ('act', C.c_int32), ('slices', C.c_int32)]


class BnAddDesc(C.Structure):
    """usot_bn_add_desc"""
    _fields_ = [('bn', BnDesc), ('res', C.c_void_p), ('dres', C.c_void_p)]


class ConfFusionDesc(C.Structure):
    """usot_conf_fusion_desc"""
    _fields_ = [('conf', C.c_void_p), ('value', C.c_void_p), ('out', C.c_void_p), ('dout', C.c_void_p), ('dconf', C.c_void_p),
                ('dvalue', C.c_void_p), ('B', C.c_int32), ('M', C.c_int32), ('P', C.c_int32), ('C', C.c_int32)]


class BoxExpDesc(C.Structure):
    """usot_box_exp_desc"""
    _fields_ = [('p', C.c_void_p), ('adjust', C.c_void_p), ('bias', C.c_void_p), ('y', C.c_void_p), ('dy', C.c_void_p),
                ('dp', C.c_void_p), ('dadjust', C.c_void_p), ('dbias', C.c_void_p), ('ws', C.c_void_p),
                ('R', C.c_int32), ('C', C.c_int32)]


SGD_FIRST, SGD_NESTEROV, SGD_MAXIMIZE = 1, 2, 4       # usot_sgd_tensor.flags


class SgdTensor(C.Structure):
    """usot_sgd_tensor"""
    _fields_ = [('p', C.c_void_p), ('g', C.c_void_p), ('buf', C.c_void_p), ('n', C.c_int64),
                ('lr', C.c_float), ('weight_decay', C.c_float), ('momentum', C.c_float), ('grad_scale', C.c_float),
                ('flags', C.c_int32), ('reserved', C.c_int32)]


class SgdLaunch(C.Structure):
    """usot_sgd_launch"""
    _fields_ = [('table', C.c_void_p), ('guard', C.c_void_p), ('counters', C.c_void_p), ('n_chunks', C.c_int64),
                ('T', C.c_int32), ('zero_grads', C.c_int32)]


class GroupDWDesc(C.Structure):
    _fields_ = [('x', C.c_void_p * 3), ('z', C.c_void_p * 3), ('out', C.c_void_p),
                ('hk', C.c_int32 * 3), ('wk', C.c_int32 * 3),
                ('x_cs', C.c_int32 * 3), ('x_co', C.c_int32 * 3),
                ('z_cs', C.c_int32 * 3), ('z_co', C.c_int32 * 3),
                ('wsm', C.c_float * 3),
                ('S', C.c_int32), ('x_rep', C.c_int32), ('OH', C.c_int32), ('OW', C.c_int32),
                ('C', C.c_int32), ('cols_per_thread', C.c_int32)]


class PwPairDesc(C.Structure):
    _fields_ = [('t2', C.c_void_p), ('w3p', C.c_void_p), ('res', C.c_void_p), ('w1', C.c_void_p),
                ('b3', C.c_void_p), ('b1', C.c_void_p), ('y', C.c_void_p), ('t', C.c_void_p),
                ('M', C.c_int32), ('CM', C.c_int32), ('CO', C.c_int32), ('CN', C.c_int32), ('act2', C.c_int32),
                ('ws', C.c_void_p), ('t2_parts', C.c_int32), ('res_parts', C.c_int32), ('t2_bias', C.c_void_p), ('res_bias', C.c_void_p),
                ('ovf', C.c_void_p)]


class BneckDesc(C.Structure):
    _fields_ = [('x', C.c_void_p), ('w1', C.c_void_p), ('w2', C.c_void_p), ('w3c', C.c_void_p), ('wn', C.c_void_p),
                ('b1', C.c_void_p), ('b2', C.c_void_p), ('b3c', C.c_void_p), ('bn', C.c_void_p),
                ('y', C.c_void_p), ('t', C.c_void_p), ('N', C.c_int32), ('H', C.c_int32), ('W', C.c_int32)]


# (immediate entry point, its plan adder, argtypes): the two take the same arguments after the first void * (the stream | the plan),
# so lib() sets each signature once for both names
PAIRS = (
    ('usot_conv2d_f32', 'usot_plan_add_conv', [C.c_void_p, C.c_void_p]),
    ('usot_conv2d_batch_f32', 'usot_plan_add_conv_batch', [C.c_void_p, C.c_void_p, C.c_int]),
    ('usot_thin_conv3x3_f32', 'usot_plan_add_thin_conv', [C.c_void_p, C.c_void_p, C.c_int]),
    ('usot_conv2d_bf16', 'usot_plan_add_conv_bf16', [C.c_void_p, C.c_void_p]),
    ('usot_conv2d_lp', 'usot_plan_add_conv_lp', [C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    ('usot_cvt_f32_to_bf16', 'usot_plan_add_cvt_bf16', [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]),
    ('usot_maxpool3x3s2_bf16', 'usot_plan_add_maxpool_bf16', [C.c_void_p] * 3 + [C.c_int] * 6),
    ('usot_stem_pool_lp', 'usot_plan_add_stem_pool_lp', [C.c_void_p] * 5 + [C.c_int] * 8 + [C.c_float] * 3),
    ('usot_pw_pair_lp', 'usot_plan_add_pw_pair', [C.c_void_p, C.c_void_p, C.c_int]),
    ('usot_pw_panel_lp', 'usot_plan_add_pw_panel', [C.c_void_p] * 6 + [C.c_int] * 5),
    ('usot_pw_panel_pair_lp', 'usot_plan_add_pw_panel_pair', [C.c_void_p, C.POINTER(PwPairDesc), C.c_int]),
    ('usot_conv_pw_lp', 'usot_plan_add_conv_pw', [C.c_void_p] * 6 + [C.c_int]),
    ('usot_conv_pw_pair_lp', 'usot_plan_add_conv_pw_pair', [C.c_void_p, C.c_void_p, C.POINTER(PwPairDesc), C.c_int]),
    ('usot_conv_pw_ov_lp', 'usot_plan_add_conv_pw_ov', [C.c_void_p, C.c_void_p, C.POINTER(PwPairDesc), C.c_int, C.c_void_p]),
    ('usot_conv3x3_halo_lp', 'usot_plan_add_conv3x3_halo', [C.c_void_p] * 5 + [C.c_int] * 7),
    ('usot_bneck_first_lp', 'usot_plan_add_bneck_first', [C.c_void_p, C.c_void_p, C.c_int]),
    ('usot_bneck_tail_lp', 'usot_plan_add_bneck_tail', [C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    ('usot_pw_kstream_lp', 'usot_plan_add_pw_kstream', [C.c_void_p] * 5 + [C.c_long] + [C.c_int] * 4),
    ('usot_conv_kstream_lp', 'usot_plan_add_conv_kstream', [C.c_void_p] * 5 + [C.c_int] * 10),
    ('usot_pw_single_f32', 'usot_plan_add_pw_single', [C.c_void_p] * 6 + [C.c_int] * 4),
    ('usot_pw_triple_f32', 'usot_plan_add_pw_triple', [C.c_void_p] * 5 + [C.c_int] * 10),
    ('usot_stream_conv3x3_f32', 'usot_plan_add_stream_conv3x3', [C.c_void_p] * 6 + [C.c_int] * 12),
    ('usot_stem_conv_f32', 'usot_plan_add_stem', [C.c_void_p] * 5 + [C.c_int] * 5),
    ('usot_stem_conv_mu_f32', 'usot_plan_add_stem_mu', [C.c_void_p] * 5 + [C.c_int] * 5 + [C.c_float] * 3),
    ('usot_stem_pool_f32', 'usot_plan_add_stem_pool', [C.c_void_p] * 5 + [C.c_int] * 7),
    ('usot_stem_pool_ind_f32', 'usot_plan_add_stem_pool_ind', [C.c_void_p] * 5 + [C.c_int] * 7 + [C.c_void_p]),
    ('usot_stem_pool_mu_f32', 'usot_plan_add_stem_pool_mu', [C.c_void_p] * 5 + [C.c_int] * 7 + [C.c_void_p] + [C.c_float] * 3),
    ('usot_maxpool3x3s2_f32', 'usot_plan_add_maxpool', [C.c_void_p] * 3 + [C.c_int] * 6),
    ('usot_groupdw_f32', 'usot_plan_add_groupdw', [C.c_void_p, C.c_void_p]),
    ('usot_groupdw_multi_f32', 'usot_plan_add_groupdw_multi', [C.c_void_p, C.c_void_p, C.c_int]),
    ('usot_groupdw_multi_lp', 'usot_plan_add_groupdw_multi_lp', [C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    ('usot_groupdw_multi_dyn_f32', 'usot_plan_add_groupdw_multi_dyn', [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    ('usot_conf_fusion_reduce_f32', 'usot_plan_add_conf_reduce', [C.c_void_p] * 3 + [C.c_int] * 4),
    ('usot_conf_fusion_reduce_lp', 'usot_plan_add_conf_reduce_lp', [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p] + [C.c_int] * 5),
    ('usot_conf_fusion_reduce_map_f32', 'usot_plan_add_conf_reduce_map', [C.c_void_p] * 3 + [C.c_int] * 4 + [C.c_void_p]),
    ('usot_prroi_pool_forward_f32', 'usot_plan_add_prroi', [C.c_void_p] * 4 + [C.c_int] * 6 + [C.c_float] + [C.c_int64] * 8),
    ('usot_permute4_f32', 'usot_plan_add_permute', [C.c_void_p] * 3 + [C.c_int] * 4 + [C.c_int64] * 4),
    ('usot_decode_dev_f32', 'usot_plan_add_decode',
     [C.c_void_p] * 6 + [C.c_int] * 3 + [C.c_float] + [C.c_double] * 2 + [C.c_void_p] * 2),
    ('usot_decode_batch_f32', 'usot_plan_add_decode_batch',
     [C.c_void_p] * 6 + [C.c_int] * 4 + [C.c_float] + [C.c_double] * 2 + [C.c_void_p] * 2),
    ('usot_rows_copy_f32', 'usot_plan_add_rows_copy', [C.c_void_p] * 4 + [C.c_int] * 3),
    ('usot_rows_copy_multi_f32', 'usot_plan_add_rows_copy_multi',
     [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    ('usot_rows_append_gather_f32', 'usot_plan_add_rows_append_gather', [C.c_void_p] * 6 + [C.c_int, C.c_int]),
    ('usot_rows_append_gather_dedupe_f32', 'usot_plan_add_rows_append_gather_dedupe', [C.c_void_p] * 6 + [C.c_int, C.c_int, C.c_void_p]),
    ('usot_rows_append_gather_batch_f32', 'usot_plan_add_rows_append_gather_batch', [C.c_void_p] * 6 + [C.c_int] * 3),
    ('usot_crop_resize_batch_u8_f32', 'usot_plan_add_crop_resize_batch', [C.c_void_p] * 3 + [C.c_int] * 2),
)

_lib = None


def lib():
    """The loaded library; raises HipError when it has not been built."""
    global _lib, LIB_PATH
    if _lib is None:
        LIB_PATH = os.environ.get('USOT_HIP_LIB', LIB_PATH)      # e.g. the -DUSOT_TRACE build of scripts/trace_kstep.py
        if not os.path.exists(LIB_PATH):
            raise HipError('%s is missing: run `python -m usot_amd.build` (hipcc, gfx950). '
                           'There is no CPU fallback for the tracking forward pass.' % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        L.usot_strerror.restype = C.c_char_p
        L.usot_strerror.argtypes = [C.c_int]
        L.usot_conv_ws_floats.restype = C.c_int64
        L.usot_plan_create.restype = C.c_void_p
        L.usot_plan_destroy.argtypes = [C.c_void_p]
        for immediate, plan_add, sig in PAIRS:
            getattr(L, immediate).argtypes = getattr(L, plan_add).argtypes = sig
        L.usot_conv3x3_halo_supported.argtypes = [C.c_int] * 2
        L.usot_bneck_first_supported.argtypes = [C.c_int] * 4
        L.usot_bneck_tail_supported.argtypes = [C.c_int] * 3
        L.usot_bw_probe.argtypes = [C.c_void_p] * 3 + [C.c_int64, C.c_int]
        L.usot_conv_kstream_supported.argtypes = [C.c_int] * 4
        L.usot_pw_kstream_supported.argtypes = [C.c_int] * 2
        L.usot_pw_panel_supported.argtypes = [C.c_int] * 2
        L.usot_pw_panel_pair_supported.argtypes = [C.c_int] * 3
        L.usot_pw_panel_pixels.argtypes = [C.c_int] * 3
        L.usot_pw_panel_min_pixels.argtypes = [C.c_int] * 2
        L.usot_conv_pw_supported.argtypes = [C.c_int] * 3
        L.usot_conv_pw_pixels.argtypes = [C.c_int64]
        L.usot_conv_pw_pair_supported.argtypes = [C.c_int] * 3
        L.usot_conv_pw_ov_supported.argtypes = [C.c_int] * 3
        L.usot_conv_pw_ov_ws_bytes.argtypes = [C.c_int64]
        L.usot_conv_pw_ov_ws_bytes.restype = C.c_int64
        L.usot_conv_pw_ov_trace.argtypes = [C.c_void_p]
        L.usot_crop_resize_u8_f32.argtypes = [C.c_void_p] * 3 + [C.c_int] * 9
        L.usot_conv_tile_dyn.argtypes = [C.c_int]
        L.usot_pw_pair_layout.argtypes = [C.c_int] * 4 + [C.POINTER(C.c_int32)] * 2
        L.usot_pw_pair_supported.argtypes = [C.c_int] * 3
        L.usot_pw_pair_f32.argtypes = [C.c_void_p, C.c_void_p]
        L.usot_pw_pair_f32_supported.argtypes = [C.c_int] * 3
        L.usot_pw_pair_f32s.argtypes = [C.c_void_p, C.c_void_p]
        L.usot_pw_pair_f32s_supported.argtypes = [C.c_int] * 3
        L.usot_pw_pair_f32_ws_floats.argtypes = [C.c_int] * 4
        L.usot_pw_pair_f32_ws_floats.restype = C.c_int64
        L.usot_pw_single_f32_supported.argtypes = [C.c_int] * 2
        L.usot_stream_conv3x3_f32_supported.argtypes = [C.c_int] * 2
        L.usot_pw_triple_f32_supported.argtypes = [C.c_int] * 4
        L.usot_stem_pool_lp_strip.argtypes = [C.c_int] * 3
        L.usot_plan_add_cvt_lp.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int]
        L.usot_plan_add_maxpool_lp.argtypes = [C.c_void_p] + [C.c_void_p] * 2 + [C.c_int] * 7
        L.usot_plan_fork.argtypes = [C.c_void_p, C.c_int]
        L.usot_plan_join.argtypes = [C.c_void_p, C.c_int]
        L.usot_plan_run.argtypes = [C.c_void_p, C.c_void_p]
        L.usot_plan_capture.argtypes = [C.c_void_p, C.c_void_p]
        L.usot_plan_size.argtypes = [C.c_void_p]
        L.usot_plan_profile.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float)]
        L.usot_plan_op_info.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        L.usot_xcorr_depthwise_f32.argtypes = [C.c_void_p] * 4 + [C.c_int] * 5
        L.usot_xcorr_depthwise_bwd_x_f32.argtypes = [C.c_void_p] * 4 + [C.c_int] * 5 + [C.c_float]
        L.usot_xcorr_depthwise_bwd_k_f32.argtypes = [C.c_void_p] * 4 + [C.c_int] * 5 + [C.c_float]
        for name in ('usot_conv2d_wgrad_f32', 'usot_conv2d_dgrad_f32'):
            getattr(L, name).argtypes = [C.c_void_p, C.c_void_p]
        for name in ('usot_conv2d_wgrad_ws_floats', 'usot_conv2d_wgrad_psplit', 'usot_conv2d_dgrad_route'):
            getattr(L, name).argtypes = [C.c_void_p]
        L.usot_conv2d_wgrad_ws_floats.restype = C.c_int64
        L.usot_conv2d_wgrad_geometry.argtypes = [C.POINTER(C.c_int)] * 3
        L.usot_conv_pack_dgrad_f32.argtypes = [C.c_void_p] * 3 + [C.c_int] * 4
        for name in ('usot_batchnorm_fwd_f32', 'usot_batchnorm_bwd_f32'):
            getattr(L, name).argtypes = [C.c_void_p, C.c_void_p]
        for name in ('usot_batchnorm_ws_floats', 'usot_batchnorm_slices'):
            getattr(L, name).argtypes = [C.c_void_p]
        L.usot_batchnorm_ws_floats.restype = C.c_int64
        L.usot_batchnorm_geometry.argtypes = [C.POINTER(C.c_int)] * 2
        # the head's gradient operators (csrc/head_grad.hip): bound here, not listed in EXPORTS (no plan adders, ABI 6 unchanged)
        for name in ('usot_conf_fusion_fwd_f32', 'usot_conf_fusion_bwd_f32', 'usot_box_exp_fwd_f32', 'usot_box_exp_bwd_f32'):
            getattr(L, name).argtypes = [C.c_void_p, C.c_void_p]
        L.usot_box_exp_ws_floats.argtypes = [C.c_void_p]
        # BatchNorm with a residual operand (csrc/batchnorm.hip): bound like the head's operators, not listed in EXPORTS
        for name in ('usot_batchnorm_add_fwd_f32', 'usot_batchnorm_add_bwd_f32'):
            getattr(L, name).argtypes = [C.c_void_p, C.c_void_p]
        L.usot_box_exp_ws_floats.restype = C.c_int64
        # the fused SGD step (csrc/sgd.hip): bound like the head's operators, not listed in EXPORTS
        L.usot_sgd_chunk_elems.argtypes = L.usot_sgd_grid_cap.argtypes = []
        L.usot_sgd_table_bytes.argtypes = [C.POINTER(C.c_int64), C.c_int, C.POINTER(C.c_int64)]
        L.usot_sgd_table_bytes.restype = C.c_int64
        L.usot_sgd_table_fill.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64]
        L.usot_sgd_step_f32.argtypes = [C.c_void_p, C.c_void_p]
        L.PrRoIPoolingForwardGpu.argtypes = [C.c_void_p] * 4 + [C.c_int] * 5 + [C.c_float, C.c_int]
        L.PrRoIPoolingForwardGpu.restype = None
        L.usot_prroi_pool_backward_f32.argtypes = [C.c_void_p] * 4 + [C.c_int] * 7 + [C.c_float]
        L.usot_prroi_pool_coor_backward_f32.argtypes = [C.c_void_p] * 6 + [C.c_int] * 7 + [C.c_float]
        for name in ('PrRoIPoolingBackwardGpu', 'PrRoIPoolingCoorBackwardGpu'):
            getattr(L, name).argtypes = [C.c_void_p] * 6 + [C.c_int] * 5 + [C.c_float, C.c_int, C.c_int]
            getattr(L, name).restype = None
        L.usot_decode_f32.argtypes = ([C.c_void_p] * 6 + [C.c_int] * 3 + [C.c_float]
                                      + [C.c_double] * 4)
        L.usot_conv_tile_info.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.usot_conv_bf16_tile_info.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.usot_conv_pack_wfrag_f32.argtypes = [C.c_void_p] * 3 + [C.c_int] * 2
        L.usot_conv_tile_kreq.argtypes = [C.c_int, C.POINTER(C.c_int)]
        L.usot_conv_streamk_ws_floats.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.usot_conv_streamk_ws_floats.restype = C.c_int64
        _lib = L
    return _lib


def check(code, what=''):
    if code != 0:
        raise HipError('%s failed: %s (%d)' % (what or 'usot call', lib().usot_strerror(code).decode(), code))


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(t, dtype=torch.float32):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise HipError('expected a device tensor (the HIP path has no CPU implementation)')
    if t.dtype != dtype:
        raise HipError('expected %s, got %s' % (dtype, t.dtype))
    return t


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def tile_name(tile):
    buf = C.create_string_buffer(96)
    check(lib().usot_conv_tile_name(int(tile), buf, 96), 'usot_conv_tile_name')
    return buf.value.decode()


def tile_launch(tile):
    """(threads per workgroup, dynamic LDS bytes) of conv tile id `tile`'s launch; (0, 0) for a tile that is not built."""
    th, lds = C.c_int(0), C.c_int(0)
    check(lib().usot_conv_tile_launch(int(tile), C.byref(th), C.byref(lds)), 'usot_conv_tile_launch')
    return th.value, lds.value


def tile_built(tile):
    """Whether conv tile id `tile` is compiled into the library: the ROUTED tiles always, the experimental ids (lab notebook:
    parity-green, measured slower, never selected by the engine) only when it was built with USOT_EXPERIMENTS=1."""
    return bool(lib().usot_conv_tile_built(int(tile)))


def lp_tile_built(tile):
    return bool(lib().usot_conv_bf16_tile_built(int(tile)))


def experiments_built():
    return bool(lib().usot_experiments_built())


def tile_wfrag(tile):
    """1 when conv tile id `tile` streams its filters in fragment order (descriptor field w_frag, pack_wfrag)."""
    return int(lib().usot_conv_tile_wfrag(int(tile))) if tile else 0


def tile_xsplit(tile):
    """1 when conv tile id `tile` reads its input map in the split-fp16 layout (descriptor field x_split, split_map)."""
    return int(lib().usot_conv_tile_xsplit(int(tile))) if tile else 0


def split_map(x):
    """NHWC fp32 map [..., C] (C % 64 == 0) -> the split-fp16 layout of usot_conv_desc.x_split / y_split as a float32-typed tensor of the
    same shape: per pixel and 64-channel block the 64 hi halves then the 64 lo halves of 8 x value."""
    c = x.shape[-1]
    assert c % 64 == 0
    v = x.float() * SPLIT16_X_SCALE
    hi = v.half()
    lo = (v - hi.float()).half()
    blocks = lambda t: t.reshape(tuple(x.shape[:-1]) + (c // 64, 64))
    return torch.cat([blocks(hi), blocks(lo)], -1).contiguous().view(torch.float32).reshape(x.shape)


def unsplit_map(y):
    """Inverse of split_map (hi + lo, / 8) - for tests and probes."""
    c = y.shape[-1]
    h = y.contiguous().view(torch.float16).reshape(tuple(y.shape[:-1]) + (c // 64, 2, 64)).float()
    return ((h[..., 0, :] + h[..., 1, :]) / SPLIT16_X_SCALE).reshape(y.shape)


def tile_kreq(tile):
    """(K, Cin multiple) a weight-stationary conv tile requires, or (0, 0) for the tiles that take any geometry."""
    if not tile:
        return 0, 0
    kp = C.c_int(0)
    k = int(lib().usot_conv_tile_kreq(int(tile), C.byref(kp)))
    return k, int(kp.value) if k else 0


def tile_supports(tile, cin, cout, k):
    """Whether conv tile id `tile` can run a convolution with these channel counts and reduction length."""
    kreq, kp = tile_kreq(tile)
    if not kreq:
        return True
    return k == kreq and cin % kp == 0 and cout % 32 == 0


def tile_streamk(tile):
    return int(lib().usot_conv_tile_streamk(int(tile))) if tile else 0


def streamk_ws(descs, tile, device):
    """Zeroed workspace of a persistent stream-K launch of `descs` (list of ConvDesc) on `tile`; sets every desc's ws."""
    arr = (ConvDesc * len(descs))(*descs)
    n = int(lib().usot_conv_streamk_ws_floats(arr, len(descs), int(tile)))
    if n < 0:
        raise HipError('usot_conv_streamk_ws_floats: %d' % n)
    ws = torch.zeros(max(n, 4), device=device, dtype=torch.float32)
    for d in descs:
        d.ws = ws.data_ptr()
    return ws


def pack_wfrag(w):
    """[Cout, K] row-major fp32 filter bank (K % 64 == 0) -> the same bank in MFMA fragment order, rows padded to a multiple
    of 16 (usot_conv_pack_wfrag_f32).  Returns a new device tensor [ceil(Cout/16)*16, K]."""
    _dev(w)
    cout, k = w.shape
    wf = torch.empty(((cout + 15) // 16) * 16, k, device=w.device, dtype=torch.float32)
    check(lib().usot_conv_pack_wfrag_f32(stream(), ptr(w.contiguous()), ptr(wf), cout, k), 'usot_conv_pack_wfrag_f32')
    return wf


def tile_table():
    L = lib()
    out = {}
    for i in range(1, L.usot_conv_tile_count() + 1):
        if not L.usot_conv_tile_built(i):
            continue
        bm, bn = C.c_int(), C.c_int()
        L.usot_conv_tile_info(i, C.byref(bm), C.byref(bn))
        out[i] = (bm.value, bn.value)
    return out


def tile_table_lp():
    """{low-precision tile id: (bm, bn)} of the tiles of usot_conv2d_lp this library holds (usot_conv_bf16_tile_info)."""
    L = lib()
    out = {}
    for i in range(1, L.usot_conv_bf16_tile_count() + 1):
        if not L.usot_conv_bf16_tile_built(i):
            continue
        bm, bn = C.c_int(), C.c_int()
        check(L.usot_conv_bf16_tile_info(i, C.byref(bm), C.byref(bn)), 'usot_conv_bf16_tile_info')
        out[i] = (bm.value, bn.value)
    return out


# ------------------------------------------------------------------ tensor-level wrappers

SPLIT16_X_SCALE = 8.0      # csrc/conv_f32_v3.h (PF = 4): the activations are split as hi + lo fp16 of 8 x


def split16_pack(w):
    """Filter bank [rows][K] fp32 (K % 64 == 0) -> (bank in the split-fp16 layout of usot_conv_desc.w_frag = 2 as a float32-typed
    tensor [rows][K]: per row and k-tile of 64, 64 hi halves then 64 lo halves of row x 2^e, e chosen per row so that the largest
    |value| lands in [512, 1024); the per-row factors 1 / (2^e x SPLIT16_X_SCALE) that undo both scales, float32 [rows])."""
    rows, k = w.shape
    assert k % 64 == 0
    w = w.float()
    amax = w.abs().amax(1)
    e = torch.where(amax > 0, torch.floor(torch.log2(1024.0 / amax.clamp_min(1e-30))), torch.zeros_like(amax))
    e = torch.where(amax * torch.exp2(e) >= 1024.0, e - 1, e).clamp(-100, 110)     # (guards the log2 rounding at exact powers of two)
    sw = torch.exp2(e)
    ws = w * sw[:, None]
    hi = ws.half()
    lo = (ws - hi.float()).half()
    packed = torch.cat([hi.view(rows, k // 64, 64), lo.view(rows, k // 64, 64)], 2).contiguous()      # [rows][KT][128] halves
    return packed.view(torch.float32).view(rows, k).contiguous(), (1.0 / (sw * SPLIT16_X_SCALE)).float().contiguous()


def conv_desc(x, w, bias, y, *, N, H, W, Cin, OH, OW, Cout, KH, KW, stride=1, pad=(0, 0), dil=(1, 1),
              res=None, act=ACT_NONE, act2=ACT_NONE, act_split=0, y_cstride=0, y_coff=0,
              res_cstride=0, res_coff=0, y_nchw=0, groups=1, x_gs=0, w_gs=0, b_gs=0, y_gs=0, r_gs=0,
              ksplit=1, tile=0, ws=None, w_frag=0, defer=0, w_scale=None, x_split=0, y_split=0, ovf=None, n_dyn=None, n_first=0):
    d = ConvDesc()
    d.x, d.w, d.bias, d.res, d.y, d.ws = (x, w, bias or None, res or None, y, ws or None)
    d.N, d.H, d.W, d.Cin, d.OH, d.OW, d.Cout = N, H, W, Cin, OH, OW, Cout
    d.KH, d.KW, d.stride = KH, KW, stride
    d.pad_h, d.pad_w, d.dil_h, d.dil_w = pad[0], pad[1], dil[0], dil[1]
    d.y_cstride, d.y_coff, d.res_cstride, d.res_coff, d.y_nchw = y_cstride, y_coff, res_cstride, res_coff, y_nchw
    d.act, d.act2, d.act_split = act, act2, act_split
    d.groups = groups
    d.x_gs, d.w_gs, d.b_gs, d.y_gs, d.r_gs = x_gs, w_gs, b_gs, y_gs, r_gs
    d.ksplit, d.tile, d.w_frag, d.defer = ksplit, tile, w_frag, defer
    d.w_scale = w_scale or None
    d.x_split, d.y_split = int(x_split), int(y_split)
    d.ovf = ovf or None          # split-fp16 tiles: the sticky "a finished sum was not finite" word (usot_conv_desc.ovf)
    d.n_dyn, d.n_first = n_dyn or None, int(n_first)      # run-time image count (usot_conv_desc.n_dyn): a device address, or off
    return d


def conv2d(x, w, bias, *, KH, KW, stride=1, pad=(0, 0), dil=(1, 1), res=None, act=ACT_NONE,
           tile=0, ksplit=1, y_nchw=False, y_split=False, ovf=None):
    """x NHWC [N,H,W,Cin] dense, w packed [Cout, KH*KW*Cin] -> y NHWC [N,OH,OW,Cout].
    ovf: int32 device tensor, the sticky range word of the split-fp16 tiles (usot_conv_desc.ovf)."""
    _dev(x), _dev(w)
    N, H, W_, Cin = x.shape
    Cout = w.shape[0]
    OH = (H + 2 * pad[0] - dil[0] * (KH - 1) - 1) // stride + 1
    OW = (W_ + 2 * pad[1] - dil[1] * (KW - 1) - 1) // stride + 1
    shape = (N, Cout, OH, OW) if y_nchw else (N, OH, OW, Cout)
    y = torch.empty(shape, device=x.device, dtype=torch.float32)
    ws = None
    if ksplit > 1:        # slabs + tile tickets (usot_conv_ws_floats); the tickets must start at zero
        ws = torch.zeros(ksplit * N * OH * OW * Cout + ((N * OH * OW + 15) // 16) * ((Cout + 31) // 32), device=x.device,
                         dtype=torch.float32)
    frag = tile_wfrag(tile)
    wsc = None
    xs = tile_xsplit(tile)
    if xs:                  # all-DMA split-fp16 tile: the input map in the split layout (here: converted for the caller)
        x = split_map(x)
    if frag == 2:           # split-fp16 tile: hi + lo fp16 of every scaled filter row, and the scales
        w, wsc = split16_pack(w)
    elif frag:              # weight-streaming tile: the filter bank in MFMA fragment order
        w = pack_wfrag(w)
    d = conv_desc(x.data_ptr(), w.data_ptr(), bias.data_ptr() if bias is not None else None, y.data_ptr(),
                  N=N, H=H, W=W_, Cin=Cin, OH=OH, OW=OW, Cout=Cout, KH=KH, KW=KW, stride=stride, pad=pad,
                  dil=dil, res=res.data_ptr() if res is not None else None, act=act, tile=tile,
                  ksplit=ksplit, ws=ws.data_ptr() if ws is not None else None, y_nchw=int(y_nchw), w_frag=frag,
                  w_scale=wsc.data_ptr() if wsc is not None else None, x_split=xs, y_split=int(y_split),
                  ovf=ovf.data_ptr() if ovf is not None else None)
    if tile_streamk(tile):
        keep = streamk_ws([d], tile, x.device)
    check(lib().usot_conv2d_f32(stream(), C.byref(d)), 'usot_conv2d_f32')
    return y


def stem_conv(x, w, bias, mu=(0.0, 0.0, 0.0)):
    """mu: per-input-channel offsets subtracted from the crop while it is staged (bias must carry + sum(w) * mu)."""
    _dev(x), _dev(w), _dev(bias)
    N, c, H, W_ = x.shape
    assert c == 3 and x.is_contiguous()
    OH, OW = (H - 7) // 2 + 1, (W_ - 7) // 2 + 1
    y = torch.empty((N, OH, OW, 64), device=x.device, dtype=torch.float32)
    check(lib().usot_stem_conv_mu_f32(stream(), ptr(x), ptr(w), ptr(bias), ptr(y), N, H, W_, OH, OW, *[float(v) for v in mu]),
          'usot_stem_conv_mu_f32')
    return y


def stem_pool(x, wfrag, bias, mu=(0.0, 0.0, 0.0)):
    """Fused fp32 stem + max-pool: x NCHW fp32 -> NHWC [N][PH][PW][64]; wfrag from engine.pack_stem_f32; mu as in stem_conv."""
    _dev(x), _dev(wfrag), _dev(bias)
    N, c, H, W_ = x.shape
    assert c == 3 and x.is_contiguous()
    OH, OW = (H - 7) // 2 + 1, (W_ - 7) // 2 + 1
    PH, PW = (OH - 1) // 2 + 1, (OW - 1) // 2 + 1
    y = torch.empty((N, PH, PW, 64), device=x.device, dtype=torch.float32)
    check(lib().usot_stem_pool_mu_f32(stream(), ptr(x), ptr(wfrag), ptr(bias), ptr(y), N, H, W_, OH, OW, PH, PW, None,
                                      *[float(v) for v in mu]), 'usot_stem_pool_mu_f32')
    return y


def stem_pool_lp(x, wfrag, bias, dtype=torch.bfloat16, mu=(0.0, 0.0, 0.0)):
    """Fused low-precision stem + max-pool: x NCHW fp32 -> NHWC [N][PH][PW][64] in `dtype`;
    wfrag from usot_amd.engine.pack_stem_lp; the kernel convolves x - mu[ci] (bias must hold the
    folded mu term).  bf16 output with fp16 fragments = the kernel's mode 2 (fp16 arithmetic, bf16 storage)."""
    _dev(x), _dev(wfrag, wfrag.dtype), _dev(bias)
    if wfrag.dtype not in (torch.float16, torch.bfloat16) or (dtype == torch.float16 and wfrag.dtype != dtype):
        raise HipError('stem_pool_lp: fragments %s for output %s' % (wfrag.dtype, dtype))
    N, c, H, W_ = x.shape
    assert c == 3 and x.is_contiguous()
    OH, OW = (H - 7) // 2 + 1, (W_ - 7) // 2 + 1
    PH, PW = (OH - 1) // 2 + 1, (OW - 1) // 2 + 1
    y = torch.empty((N, PH, PW, 64), device=x.device, dtype=dtype)
    check(lib().usot_stem_pool_lp(stream(), ptr(x), ptr(wfrag), ptr(bias), ptr(y), N, H, W_, OH, OW, PH, PW,
                                  1 if dtype == torch.float16 else (2 if wfrag.dtype == torch.float16 else 0), float(mu[0]), float(mu[1]), float(mu[2])),
          'usot_stem_pool_lp')
    return y


def maxpool3x3s2(x):
    _dev(x)
    N, H, W_, c = x.shape
    OH, OW = (H - 1) // 2 + 1, (W_ - 1) // 2 + 1
    y = torch.empty((N, OH, OW, c), device=x.device, dtype=torch.float32)
    check(lib().usot_maxpool3x3s2_f32(stream(), ptr(x), ptr(y), N, H, W_, c, OH, OW), 'usot_maxpool3x3s2_f32')
    return y


def xcorr_depthwise(x, kernel):
    """Drop-in for reference connect.py:147-157 on NCHW device tensors."""
    _dev(x), _dev(kernel)
    b, c, hk, wk = kernel.shape
    hx, wx = x.shape[2], x.shape[3]
    x = x.contiguous().view(-1, hx, wx)
    k = kernel.contiguous().view(-1, hk, wk)
    if x.shape[0] != k.shape[0]:
        raise HipError('xcorr_depthwise: plane counts differ (%d vs %d)' % (x.shape[0], k.shape[0]))
    out = torch.empty((b, c, hx - hk + 1, wx - wk + 1), device=x.device, dtype=torch.float32)
    check(lib().usot_xcorr_depthwise_f32(stream(), ptr(x), ptr(k), ptr(out), b * c, hx, wx, hk, wk),
          'usot_xcorr_depthwise_f32')
    return out


def _xcorr_grad_geometry(what, dout, hx, wx, hk, wk):
    if hk < 1 or wk < 1 or hx < hk or wx < wk or tuple(dout.shape[2:]) != (hx - hk + 1, wx - wk + 1):
        raise HipError('%s: grad_output %s does not belong to a %dx%d map and a %dx%d template'
                       % (what, tuple(dout.shape), hx, wx, hk, wk))


def xcorr_depthwise_backward_x(dout, kernel, x_shape, scale=1.0):
    """Gradient of `xcorr_depthwise` w.r.t. its search map, times `scale`: dout [B][C][OH][OW], kernel [B][C][Hk][Wk]
    -> dx of shape `x_shape` ([B][C][Hx][Wx]).  Every element of dx is written by the kernel."""
    _dev(dout), _dev(kernel)
    b, c, hx, wx = (int(v) for v in x_shape)
    hk, wk = kernel.shape[2], kernel.shape[3]
    _xcorr_grad_geometry('xcorr_depthwise_backward_x', dout, hx, wx, hk, wk)
    d = dout.contiguous().view(-1, dout.shape[2], dout.shape[3])
    k = kernel.contiguous().view(-1, hk, wk)
    if not d.shape[0] == k.shape[0] == b * c:
        raise HipError('xcorr_depthwise_backward_x: plane counts differ (%d, %d vs %d)' % (d.shape[0], k.shape[0], b * c))
    dx = torch.empty((b, c, hx, wx), device=dout.device, dtype=torch.float32)
    check(lib().usot_xcorr_depthwise_bwd_x_f32(stream(), ptr(d), ptr(k), ptr(dx), b * c, hx, wx, hk, wk, float(scale)),
          'usot_xcorr_depthwise_bwd_x_f32')
    return dx


def xcorr_depthwise_backward_k(dout, x, kernel_shape, scale=1.0):
    """Gradient of `xcorr_depthwise` w.r.t. its template, times `scale`: dout [B][C][OH][OW], x [B][C][Hx][Wx]
    -> dk of shape `kernel_shape` ([B][C][Hk][Wk]).  Every element of dk is written by the kernel."""
    _dev(dout), _dev(x)
    b, c, hk, wk = (int(v) for v in kernel_shape)
    hx, wx = x.shape[2], x.shape[3]
    _xcorr_grad_geometry('xcorr_depthwise_backward_k', dout, hx, wx, hk, wk)
    d = dout.contiguous().view(-1, dout.shape[2], dout.shape[3])
    xs = x.contiguous().view(-1, hx, wx)
    if not d.shape[0] == xs.shape[0] == b * c:
        raise HipError('xcorr_depthwise_backward_k: plane counts differ (%d, %d vs %d)' % (d.shape[0], xs.shape[0], b * c))
    dk = torch.empty((b, c, hk, wk), device=dout.device, dtype=torch.float32)
    check(lib().usot_xcorr_depthwise_bwd_k_f32(stream(), ptr(d), ptr(xs), ptr(dk), b * c, hx, wx, hk, wk, float(scale)),
          'usot_xcorr_depthwise_bwd_k_f32')
    return dk


def grad_desc(*, N, H, W, Cin, Cout, KH, KW, stride=1, pad=(0, 0), dil=(1, 1), x=None, w=None, wt=None, dy=None, dx=None,
              dw=None, db=None, ws=None, psplit=0, route=0):
    """usot_conv_grad_desc of a convolution's geometry; pointers are addresses (or None); OH / OW are the convolution's."""
    d = GradDesc()
    d.x, d.w, d.wt, d.dy, d.dx, d.dw, d.db, d.ws = (v or None for v in (x, w, wt, dy, dx, dw, db, ws))
    d.N, d.H, d.W, d.Cin, d.Cout, d.KH, d.KW, d.stride = N, H, W, Cin, Cout, KH, KW, stride
    d.pad_h, d.pad_w, d.dil_h, d.dil_w = pad[0], pad[1], dil[0], dil[1]
    d.OH = (H + 2 * pad[0] - dil[0] * (KH - 1) - 1) // max(stride, 1) + 1
    d.OW = (W + 2 * pad[1] - dil[1] * (KW - 1) - 1) // max(stride, 1) + 1
    d.psplit, d.route = psplit, route
    return d


def wgrad_geometry():
    """(Cout block, k block, pixels staged per step) of the weight-gradient kernel"""
    v = [C.c_int(0) for _ in range(3)]
    check(lib().usot_conv2d_wgrad_geometry(*[C.byref(i) for i in v]), 'usot_conv2d_wgrad_geometry')
    return tuple(i.value for i in v)


def conv2d_backward_w(x, dy, *, KH, KW, stride=1, pad=(0, 0), dil=(1, 1), bias=False, psplit=0):
    """Gradient of `conv2d` w.r.t. its packed filter bank (and its bias): x NHWC [N,H,W,Cin], dy NHWC [N,OH,OW,Cout] dense
    -> (dw [Cout, KH*KW*Cin], db [Cout] or None).  psplit: pixel slices (0 = the launcher's choice, usot_conv_grad_desc)."""
    _dev(x), _dev(dy)
    if x.dim() != 4 or dy.dim() != 4 or not x.is_contiguous() or not dy.is_contiguous():
        raise HipError('conv2d_backward_w: dense NHWC tensors expected')
    N, H, W_, Cin = x.shape
    Cout = dy.shape[3]
    d = grad_desc(N=N, H=H, W=W_, Cin=Cin, Cout=Cout, KH=KH, KW=KW, stride=stride, pad=pad, dil=dil, psplit=psplit)
    if tuple(dy.shape) != (N, d.OH, d.OW, Cout):
        raise HipError('conv2d_backward_w: grad_output %s does not belong to input %s (expected %s)'
                       % (tuple(dy.shape), tuple(x.shape), (N, d.OH, d.OW, Cout)))
    K = KH * KW * Cin
    dw = torch.empty((Cout, K), device=x.device, dtype=torch.float32)
    db = torch.empty((Cout,), device=x.device, dtype=torch.float32) if bias else None
    need = lib().usot_conv2d_wgrad_ws_floats(C.byref(d))
    if need < 0:
        check(int(need), 'usot_conv2d_wgrad_ws_floats')
    ws = torch.empty((need,), device=x.device, dtype=torch.float32) if need else None
    d.x, d.dy, d.dw, d.db, d.ws = x.data_ptr(), dy.data_ptr(), dw.data_ptr(), db.data_ptr() if bias else None, \
        ws.data_ptr() if ws is not None else None
    check(lib().usot_conv2d_wgrad_f32(stream(), C.byref(d)), 'usot_conv2d_wgrad_f32')
    return dw, db


def pack_dgrad(w, Cin, KH, KW):
    """Packed bank w [Cout, KH*KW*Cin] -> the rotated, transposed bank wt [Cin, KH*KW*Cout] of the data gradient's route A."""
    _dev(w)
    Cout = w.shape[0]
    if w.dim() != 2 or w.shape[1] != KH * KW * Cin or not w.is_contiguous():
        raise HipError('pack_dgrad: bank %s is not [Cout][%d*%d*%d]' % (tuple(w.shape), KH, KW, Cin))
    wt = torch.empty((Cin, KH * KW * Cout), device=w.device, dtype=torch.float32)
    check(lib().usot_conv_pack_dgrad_f32(stream(), ptr(w), ptr(wt), Cout, Cin, KH, KW), 'usot_conv_pack_dgrad_f32')
    return wt


def conv2d_backward_x(dy, w, x_shape, *, KH, KW, stride=1, pad=(0, 0), dil=(1, 1), route=0):
    """Gradient of `conv2d` w.r.t. its input: dy NHWC [N,OH,OW,Cout] dense, w packed [Cout, KH*KW*Cin] -> dx of shape
    `x_shape` ([N,H,W,Cin]).  route: 0 = auto, 1 = the forward kernels on the rotated bank, 2 = the direct kernel."""
    _dev(dy), _dev(w)
    N, H, W_, Cin = (int(v) for v in x_shape)
    if dy.dim() != 4 or w.dim() != 2 or not dy.is_contiguous() or not w.is_contiguous():
        raise HipError('conv2d_backward_x: dense tensors expected')
    Cout = w.shape[0]
    d = grad_desc(N=N, H=H, W=W_, Cin=Cin, Cout=Cout, KH=KH, KW=KW, stride=stride, pad=pad, dil=dil, route=route)
    if w.shape[1] != KH * KW * Cin or tuple(dy.shape) != (N, d.OH, d.OW, Cout):
        raise HipError('conv2d_backward_x: grad_output %s / bank %s do not belong to input %s'
                       % (tuple(dy.shape), tuple(w.shape), (N, H, W_, Cin)))
    d.dy, d.w, d.wt = dy.data_ptr(), w.data_ptr(), 16          # wt: any address, for the route query
    r = lib().usot_conv2d_dgrad_route(C.byref(d)) if route != 2 else 2
    if r < 0:
        check(r, 'usot_conv2d_dgrad_route')
    wt = pack_dgrad(w, Cin, KH, KW) if r == 1 else None
    dx = torch.empty((N, H, W_, Cin), device=dy.device, dtype=torch.float32)
    d.wt, d.dx = wt.data_ptr() if wt is not None else None, dx.data_ptr()
    check(lib().usot_conv2d_dgrad_f32(stream(), C.byref(d)), 'usot_conv2d_dgrad_f32')
    return dx


def bn_desc(*, M, C, eps=1e-5, momentum=0.1, training=True, act=ACT_NONE, slices=0, x=None, gamma=None, beta=None,
            running_mean=None, running_var=None, y=None, save_mean=None, save_invstd=None, dy=None, dx=None, dgamma=None,
            dbeta=None, ws=None):
    """usot_bn_desc of an [M][C] map; pointers are addresses (or None)"""
    d = BnDesc()
    d.x, d.gamma, d.beta, d.running_mean, d.running_var, d.y, d.save_mean, d.save_invstd, d.dy, d.dx, d.dgamma, d.dbeta, d.ws = (
        v or None for v in (x, gamma, beta, running_mean, running_var, y, save_mean, save_invstd, dy, dx, dgamma, dbeta, ws))
    d.M, d.C, d.eps, d.momentum, d.training, d.act, d.slices = M, C, eps, momentum, int(training), act, slices
    return d


def batchnorm_geometry():
    """(rows staged per step, channels per workgroup) of the batch-norm kernels"""
    v = [C.c_int(0) for _ in range(2)]
    check(lib().usot_batchnorm_geometry(*[C.byref(i) for i in v]), 'usot_batchnorm_geometry')
    return tuple(i.value for i in v)


def _bn_map(what, t, channels=None):
    """a dense [..., C] device map -> (M, C)"""
    _dev(t)
    if t.dim() < 2 or not t.is_contiguous() or (channels is not None and t.shape[-1] != channels):
        raise HipError('%s: a dense NHWC map%s expected, got shape %s strides %s'
                       % (what, '' if channels is None else ' of %d channels' % channels, tuple(t.shape), t.stride()))
    return t.numel() // t.shape[-1], t.shape[-1]


def _bn_vec(what, name, t, channels):
    _dev(t)
    if t.dim() != 1 or t.shape[0] != channels or not t.is_contiguous():
        raise HipError('%s: %s of shape %s does not hold %d channels' % (what, name, tuple(t.shape), channels))
    return t.data_ptr()


def _bn_ws(d, device):
    need = lib().usot_batchnorm_ws_floats(C.byref(d))
    if need < 0:
        check(int(need), 'usot_batchnorm_ws_floats')
    return torch.empty((need,), device=device, dtype=torch.float32)


def batch_norm_forward(x_nhwc, gamma, beta, running_mean, running_var, *, training, momentum=0.1, eps=1e-5, relu=False,
                       slices=0):
    """BatchNorm2d (and the ReLU behind it) of a dense NHWC map [..., C], C % 4 == 0 -> (y, save_mean, save_invstd).
    training: batch statistics; running_mean / running_var (each may be None) are updated in place on the device, and
    save_mean / save_invstd are what `batch_norm_backward` needs.  Eval: the running statistics normalise, and the two saved
    vectors are None."""
    what = 'batch_norm_forward'
    M, Cc = _bn_map(what, x_nhwc)
    d = bn_desc(M=M, C=Cc, eps=eps, momentum=momentum, training=training, act=ACT_RELU if relu else ACT_NONE, slices=slices,
                x=x_nhwc.data_ptr(), gamma=_bn_vec(what, 'gamma', gamma, Cc), beta=_bn_vec(what, 'beta', beta, Cc))
    if running_mean is not None or not training:
        d.running_mean = _bn_vec(what, 'running_mean', running_mean, Cc)
    if running_var is not None or not training:
        d.running_var = _bn_vec(what, 'running_var', running_var, Cc)
    y = torch.empty(x_nhwc.shape, device=x_nhwc.device, dtype=torch.float32)
    d.y = y.data_ptr()
    mean = invstd = ws = None
    if training:
        mean = torch.empty((Cc,), device=x_nhwc.device, dtype=torch.float32)
        invstd = torch.empty((Cc,), device=x_nhwc.device, dtype=torch.float32)
        ws = _bn_ws(d, x_nhwc.device)
        d.save_mean, d.save_invstd, d.ws = mean.data_ptr(), invstd.data_ptr(), ws.data_ptr()
    check(lib().usot_batchnorm_fwd_f32(stream(), C.byref(d)), 'usot_batchnorm_fwd_f32')
    return y, mean, invstd


def batch_norm_backward(dy, x_nhwc, gamma, beta, save_mean, save_invstd, running_mean, running_var, *, training, eps=1e-5,
                        relu=False, need=(True, True, True), slices=0):
    """Gradients of `batch_norm_forward` -> (dx | None, dgamma | None, dbeta | None), the ones `need` asks for.  dy and
    x_nhwc are dense NHWC maps of one shape.  training: save_mean / save_invstd of the forward call; eval: the running
    statistics it read.  beta is read with relu only: the mask is recomputed from x, not read from y."""
    what = 'batch_norm_backward'
    M, Cc = _bn_map(what, x_nhwc)
    _bn_map(what, dy, Cc)
    if dy.shape != x_nhwc.shape:
        raise HipError('%s: grad_output %s does not belong to input %s' % (what, tuple(dy.shape), tuple(x_nhwc.shape)))
    d = bn_desc(M=M, C=Cc, eps=eps, training=training, act=ACT_RELU if relu else ACT_NONE, slices=slices,
                x=x_nhwc.data_ptr(), dy=dy.data_ptr(), gamma=_bn_vec(what, 'gamma', gamma, Cc))
    if relu:
        d.beta = _bn_vec(what, 'beta', beta, Cc)
    if training:
        d.save_mean, d.save_invstd = _bn_vec(what, 'save_mean', save_mean, Cc), _bn_vec(what, 'save_invstd', save_invstd, Cc)
    else:
        d.running_mean = _bn_vec(what, 'running_mean', running_mean, Cc)
        d.running_var = _bn_vec(what, 'running_var', running_var, Cc)
    need_x, need_g, need_b = (bool(v) for v in need)
    dx = torch.empty(x_nhwc.shape, device=dy.device, dtype=torch.float32) if need_x else None
    dg = torch.empty((Cc,), device=dy.device, dtype=torch.float32) if need_g else None
    db = torch.empty((Cc,), device=dy.device, dtype=torch.float32) if need_b else None
    ws = _bn_ws(d, dy.device) if need_g or need_b or (training and need_x) else None
    d.dx, d.dgamma, d.dbeta, d.ws = ptr(dx), ptr(dg), ptr(db), ptr(ws)
    check(lib().usot_batchnorm_bwd_f32(stream(), C.byref(d)), 'usot_batchnorm_bwd_f32')
    return dx, dg, db


def bn_add_desc(*, res=None, dres=None, **bn):
    """usot_bn_add_desc: `bn_desc(**bn)` with the residual map and its gradient; pointers are addresses (or None)"""
    d = BnAddDesc()
    d.bn = bn_desc(**bn)
    d.res, d.dres = res or None, dres or None
    return d


def batch_norm_add_forward(x_nhwc, res_nhwc, gamma, beta, running_mean, running_var, *, training, momentum=0.1, eps=1e-5,
                           relu=True, slices=0):
    """BatchNorm2d of a dense NHWC map [..., C], C % 4 == 0, plus a residual map of the same shape, and the ReLU behind the sum
    (a bottleneck's tail) -> (y, save_mean, save_invstd).  Statistics and running statistics as in `batch_norm_forward`: the
    residual does not enter them."""
    what = 'batch_norm_add_forward'
    M, Cc = _bn_map(what, x_nhwc)
    _bn_map(what, res_nhwc, Cc)
    if res_nhwc.shape != x_nhwc.shape:
        raise HipError('%s: residual %s does not belong to input %s' % (what, tuple(res_nhwc.shape), tuple(x_nhwc.shape)))
    d = bn_add_desc(M=M, C=Cc, eps=eps, momentum=momentum, training=training, act=ACT_RELU if relu else ACT_NONE, slices=slices,
                    x=x_nhwc.data_ptr(), res=res_nhwc.data_ptr(), gamma=_bn_vec(what, 'gamma', gamma, Cc),
                    beta=_bn_vec(what, 'beta', beta, Cc))
    if running_mean is not None or not training:
        d.bn.running_mean = _bn_vec(what, 'running_mean', running_mean, Cc)
    if running_var is not None or not training:
        d.bn.running_var = _bn_vec(what, 'running_var', running_var, Cc)
    y = torch.empty(x_nhwc.shape, device=x_nhwc.device, dtype=torch.float32)
    d.bn.y = y.data_ptr()
    mean = invstd = ws = None
    if training:
        mean = torch.empty((Cc,), device=x_nhwc.device, dtype=torch.float32)
        invstd = torch.empty((Cc,), device=x_nhwc.device, dtype=torch.float32)
        ws = _bn_ws(d.bn, x_nhwc.device)
        d.bn.save_mean, d.bn.save_invstd, d.bn.ws = mean.data_ptr(), invstd.data_ptr(), ws.data_ptr()
    check(lib().usot_batchnorm_add_fwd_f32(stream(), C.byref(d)), 'usot_batchnorm_add_fwd_f32')
    return y, mean, invstd


def batch_norm_add_backward(dy, x_nhwc, res_nhwc, gamma, beta, save_mean, save_invstd, running_mean, running_var, *, training,
                            eps=1e-5, relu=True, need=(True, True, True, True), slices=0):
    """Gradients of `batch_norm_add_forward` -> (dx | None, dgamma | None, dbeta | None, dres | None), the ones `need` asks for
    (at least one).  dy, x_nhwc and res_nhwc are dense NHWC maps of one shape; the statistics as in `batch_norm_backward`.  The
    mask of the ReLU is recomputed from x and the residual, not read from y."""
    what = 'batch_norm_add_backward'
    M, Cc = _bn_map(what, x_nhwc)
    _bn_map(what, dy, Cc)
    _bn_map(what, res_nhwc, Cc)
    if dy.shape != x_nhwc.shape:
        raise HipError('%s: grad_output %s does not belong to input %s' % (what, tuple(dy.shape), tuple(x_nhwc.shape)))
    if res_nhwc.shape != x_nhwc.shape:
        raise HipError('%s: residual %s does not belong to input %s' % (what, tuple(res_nhwc.shape), tuple(x_nhwc.shape)))
    need_x, need_g, need_b, need_r = (bool(v) for v in need)
    if not (need_x or need_g or need_b or need_r):
        raise HipError('%s: no gradient is asked for' % what)
    d = bn_add_desc(M=M, C=Cc, eps=eps, training=training, act=ACT_RELU if relu else ACT_NONE, slices=slices,
                    x=x_nhwc.data_ptr(), res=res_nhwc.data_ptr(), dy=dy.data_ptr(), gamma=_bn_vec(what, 'gamma', gamma, Cc))
    if relu:
        d.bn.beta = _bn_vec(what, 'beta', beta, Cc)
    if training:
        d.bn.save_mean = _bn_vec(what, 'save_mean', save_mean, Cc)
        d.bn.save_invstd = _bn_vec(what, 'save_invstd', save_invstd, Cc)
    else:
        d.bn.running_mean = _bn_vec(what, 'running_mean', running_mean, Cc)
        d.bn.running_var = _bn_vec(what, 'running_var', running_var, Cc)
    dx = torch.empty(x_nhwc.shape, device=dy.device, dtype=torch.float32) if need_x else None
    dr = torch.empty(x_nhwc.shape, device=dy.device, dtype=torch.float32) if need_r else None
    dg = torch.empty((Cc,), device=dy.device, dtype=torch.float32) if need_g else None
    db = torch.empty((Cc,), device=dy.device, dtype=torch.float32) if need_b else None
    ws = _bn_ws(d.bn, dy.device) if need_g or need_b or (training and need_x) else None
    d.bn.dx, d.bn.dgamma, d.bn.dbeta, d.bn.ws, d.dres = ptr(dx), ptr(dg), ptr(db), ptr(ws), ptr(dr)
    check(lib().usot_batchnorm_add_bwd_f32(stream(), C.byref(d)), 'usot_batchnorm_add_bwd_f32')
    return dx, dg, db, dr


def conf_fusion_desc(*, B, M, P, C, conf=None, value=None, out=None, dout=None, dconf=None, dvalue=None):
    """usot_conf_fusion_desc of [B*M][P][C] maps; pointers are addresses (or None)"""
    d = ConfFusionDesc()
    d.conf, d.value, d.out, d.dout, d.dconf, d.dvalue = (v or None for v in (conf, value, out, dout, dconf, dvalue))
    d.B, d.M, d.P, d.C = B, M, P, C
    return d


def _cf_maps(what, conf, value, B, M):
    """the two dense [B*M, ..., C] device maps of a Conf_Fusion call -> (P, C)"""
    _bn_map(what, conf)
    if value is not None:
        _bn_map(what, value)
        if value.shape != conf.shape:
            raise HipError('%s: conf %s and value %s differ in shape' % (what, tuple(conf.shape), tuple(value.shape)))
    B, M = int(B), int(M)
    Cc = conf.shape[-1]
    if B < 1 or M < 1 or conf.dim() < 3 or conf.shape[0] != B * M or Cc < 4 or Cc % 4:
        raise HipError('%s: maps of shape %s are not [B*M = %d*%d, ..., C] with C %% 4 == 0' % (what, tuple(conf.shape), B, M))
    return conf.numel() // (B * M * Cc), Cc


def conf_fusion_forward(conf, value, B, M):
    """Conf_Fusion (connect.py:129-142) of the dense NHWC maps conf and value [B*M, H, W, C] (map b*M + m: slot m of batch
    element b), C % 4 == 0 -> out [B, H, W, C] = sum_m softmax-like weights exp(clamp(conf_m, -6, 4)) / S times value_m."""
    what = 'conf_fusion_forward'
    P, Cc = _cf_maps(what, conf, value, B, M)
    out = torch.empty((int(B),) + tuple(conf.shape[1:]), device=conf.device, dtype=torch.float32)
    d = conf_fusion_desc(B=int(B), M=int(M), P=P, C=Cc, conf=conf.data_ptr(), value=value.data_ptr(), out=out.data_ptr())
    check(lib().usot_conf_fusion_fwd_f32(stream(), C.byref(d)), 'usot_conf_fusion_fwd_f32')
    return out


def conf_fusion_backward(dout, conf, value, B, M, need=(True, True)):
    """Gradients of `conf_fusion_forward` -> (dconf | None, dvalue | None), the ones `need` asks for; dout is dense [B, H, W, C].
    The weights and `out` are recomputed from conf and value."""
    what = 'conf_fusion_backward'
    P, Cc = _cf_maps(what, conf, value, B, M)
    _bn_map(what, dout, Cc)
    if tuple(dout.shape) != (int(B),) + tuple(conf.shape[1:]):
        raise HipError('%s: grad_output %s does not belong to maps %s' % (what, tuple(dout.shape), tuple(conf.shape)))
    need_c, need_v = (bool(v) for v in need)
    dconf = torch.empty(conf.shape, device=conf.device, dtype=torch.float32) if need_c else None
    dvalue = torch.empty(conf.shape, device=conf.device, dtype=torch.float32) if need_v else None
    d = conf_fusion_desc(B=int(B), M=int(M), P=P, C=Cc, conf=conf.data_ptr(), value=value.data_ptr(), dout=dout.data_ptr())
    d.dconf, d.dvalue = ptr(dconf), ptr(dvalue)
    check(lib().usot_conf_fusion_bwd_f32(stream(), C.byref(d)), 'usot_conf_fusion_bwd_f32')
    return dconf, dvalue


def box_exp_desc(*, R, C=4, p=None, adjust=None, bias=None, y=None, dy=None, dp=None, dadjust=None, dbias=None, ws=None):
    """usot_box_exp_desc of an [R][4] map; pointers are addresses (or None)"""
    d = BoxExpDesc()
    d.p, d.adjust, d.bias, d.y, d.dy, d.dp, d.dadjust, d.dbias, d.ws = (
        v or None for v in (p, adjust, bias, y, dy, dp, dadjust, dbias, ws))
    d.R, d.C = R, C
    return d


def box_exp_ws_floats(R):
    """floats of workspace a box_exp_backward over R rows needs (host only)"""
    need = lib().usot_box_exp_ws_floats(C.byref(box_exp_desc(R=int(R))))
    if need < 0:
        check(int(need), 'usot_box_exp_ws_floats')
    return int(need)


def box_exp_row_step():
    """rows one workgroup of the box-exp reduction sums into one partial, read off the workspace query"""
    one, r = box_exp_ws_floats(1), 1
    while box_exp_ws_floats(r + 1) == one:
        r += 1
    return r


def _box_args(what, p, adjust, bias):
    _bn_map(what, p, 4)
    for name, t, n in (('adjust', adjust, 1), ('bias', bias, 4)):
        _dev(t)
        if t.numel() != n or not t.is_contiguous():
            raise HipError('%s: %s of shape %s does not hold %d float%s' % (what, name, tuple(t.shape), n, 's' * (n > 1)))
    return p.numel() // 4


def box_exp_forward(p, adjust, bias):
    """y = exp(adjust * p + bias[c]) of a dense NHWC map p [..., 4]; adjust (1 float) and bias (4 floats) are device tensors and
    are read on the device (connect.py:236-237)."""
    what = 'box_exp_forward'
    R = _box_args(what, p, adjust, bias)
    y = torch.empty(p.shape, device=p.device, dtype=torch.float32)
    d = box_exp_desc(R=R, p=p.data_ptr(), adjust=adjust.data_ptr(), bias=bias.data_ptr(), y=y.data_ptr())
    check(lib().usot_box_exp_fwd_f32(stream(), C.byref(d)), 'usot_box_exp_fwd_f32')
    return y


def box_exp_backward(dy, p, adjust, bias, need=(True, True, True)):
    """Gradients of `box_exp_forward` -> (dp | None, dadjust | None, dbias | None), the ones `need` asks for, dadjust and dbias
    in the shapes of adjust and bias.  y is recomputed from p; the two sums have an order fixed by the row count."""
    what = 'box_exp_backward'
    R = _box_args(what, p, adjust, bias)
    _bn_map(what, dy, 4)
    if dy.shape != p.shape:
        raise HipError('%s: grad_output %s does not belong to input %s' % (what, tuple(dy.shape), tuple(p.shape)))
    need_p, need_a, need_b = (bool(v) for v in need)
    dp = torch.empty(p.shape, device=p.device, dtype=torch.float32) if need_p else None
    da = torch.empty(adjust.shape, device=p.device, dtype=torch.float32) if need_a else None
    db = torch.empty(bias.shape, device=p.device, dtype=torch.float32) if need_b else None
    ws = torch.empty((box_exp_ws_floats(R),), device=p.device, dtype=torch.float32) if need_a or need_b else None
    d = box_exp_desc(R=R, p=p.data_ptr(), adjust=adjust.data_ptr(), bias=bias.data_ptr(), dy=dy.data_ptr())
    d.dp, d.dadjust, d.dbias, d.ws = ptr(dp), ptr(da), ptr(db), ptr(ws)
    check(lib().usot_box_exp_bwd_f32(stream(), C.byref(d)), 'usot_box_exp_bwd_f32')
    return dp, da, db


def sgd_chunk_elems():
    """elements of one chunk of the fused SGD step (host only)"""
    return int(lib().usot_sgd_chunk_elems())


def sgd_grid_cap():
    """most workgroups of one launch of the fused SGD step (host only)"""
    return int(lib().usot_sgd_grid_cap())


def sgd_table(records):
    """Table image of the fused SGD step for `records` (a ctypes array of SgdTensor, or a sequence of them): validated and laid out
    by usot_sgd_table_fill in HOST memory -> (image as a ctypes array of bytes, n_chunks).  Touches no device; the caller uploads
    the image and hands its device copy to sgd_step with the same T and n_chunks."""
    if not isinstance(records, C.Array):
        records = (SgdTensor * len(records))(*records)
    T = len(records)
    if T < 1 or records._type_ is not SgdTensor:
        raise HipError('sgd_table: at least one SgdTensor record expected')
    words = C.sizeof(SgdTensor) // 8                     # the records as int64 words: n is word 3 of each
    n = np.ascontiguousarray(np.frombuffer(records, dtype=np.int64)[SgdTensor.n.offset // 8::words])
    chunks = C.c_int64(0)
    nbytes = lib().usot_sgd_table_bytes(n.ctypes.data_as(C.POINTER(C.c_int64)), T, C.byref(chunks))
    if nbytes < 0:
        check(int(nbytes), 'usot_sgd_table_bytes')
    image = (C.c_ubyte * nbytes)()
    check(lib().usot_sgd_table_fill(records, T, image, nbytes), 'usot_sgd_table_fill')
    return image, int(chunks.value)


def sgd_step(table, T, n_chunks, guard=None, counters=None, zero_grads=False):
    """One launch of the fused SGD step over the uploaded table image `table` (uint8 device tensor; T records, n_chunks chunks -
    sgd_table).  guard: 1-element fp32 device tensor (the loss) or None; counters: int32 device tensor [2] (applied, skipped) or
    None; zero_grads: store 0 over every gradient the launch covers."""
    _dev(table, torch.uint8)
    if guard is not None and _dev(guard).numel() != 1:
        raise HipError('sgd_step: the guard holds %d values, not one' % guard.numel())
    if counters is not None and (_dev(counters, torch.int32).numel() != 2 or not counters.is_contiguous()):
        raise HipError('sgd_step: counters of shape %s are not two dense int32' % (tuple(counters.shape),))
    if not table.is_contiguous() or table.numel() < T * C.sizeof(SgdTensor) + 8 * n_chunks:
        raise HipError('sgd_step: a table of %d bytes does not hold %d records and %d chunks' % (table.numel(), T, n_chunks))
    d = SgdLaunch()
    d.table, d.guard, d.counters = table.data_ptr(), ptr(guard), ptr(counters)
    d.n_chunks, d.T, d.zero_grads = int(n_chunks), int(T), int(bool(zero_grads))
    check(lib().usot_sgd_step_f32(stream(), C.byref(d)), 'usot_sgd_step_f32')


def groupdw_desc(xs, zs, out, wsm, *, S, x_rep, OH, OW, Cc, x_cs, x_co, z_cs, z_co, cols=0):
    d = GroupDWDesc()
    geo = ((5, 5), (3, 5), (5, 3))
    for b in range(3):
        d.x[b], d.z[b] = xs[b], zs[b]
        d.hk[b], d.wk[b] = geo[b]
        d.x_cs[b], d.x_co[b], d.z_cs[b], d.z_co[b] = x_cs[b], x_co[b], z_cs[b], z_co[b]
        d.wsm[b] = float(wsm[b])
    d.out = out
    d.S, d.x_rep, d.OH, d.OW, d.C, d.cols_per_thread = S, x_rep, OH, OW, Cc, cols
    return d


def groupdw(xs, zs, wsm, x_rep=1, cols=0):
    """xs: 3 NHWC search maps [XS,h,w,C]; zs: 3 NHWC templates [S,hk,wk,C] -> [S,OH,OW,C]."""
    S, Cc = zs[0].shape[0], zs[0].shape[3]
    OH, OW = xs[0].shape[1] - 4, xs[0].shape[2] - 4
    for t in list(xs) + list(zs):
        _dev(t)
        assert t.is_contiguous()
    out = torch.empty((S, OH, OW, Cc), device=xs[0].device, dtype=torch.float32)
    d = groupdw_desc([t.data_ptr() for t in xs], [t.data_ptr() for t in zs], out.data_ptr(), wsm,
                     S=S, x_rep=x_rep, OH=OH, OW=OW, Cc=Cc, x_cs=[Cc] * 3, x_co=[0] * 3,
                     z_cs=[Cc] * 3, z_co=[0] * 3, cols=cols)
    check(lib().usot_groupdw_f32(stream(), C.byref(d)), 'usot_groupdw_f32')
    return out


GROUPDW_VARIANTS = {1: 'groupdw_nhwc_kernel<5,1> (strips)', 2: 'groupdw_nhwc_col_kernel', 3: 'groupdw_nhwc_stream_kernel',
                    4: 'groupdw_nhwc_ring_kernel', 5: 'groupdw_nhwc_kernel<5,5> (patches)', 6: 'groupdw_dma_kernel'}


def groupdw_variant_name(samples, ow=25):
    """Kernel the launcher's auto mode runs for `samples` samples (what a benchmark times)."""
    return GROUPDW_VARIANTS.get(int(lib().usot_groupdw_auto_variant(int(samples), int(ow))), 'groupdw')


def conf_fusion_reduce(cv, B, M):
    _dev(cv)
    P, C2 = cv.shape[1] * cv.shape[2], cv.shape[3]
    out = torch.empty((B, cv.shape[1], cv.shape[2], C2 // 2), device=cv.device, dtype=torch.float32)
    check(lib().usot_conf_fusion_reduce_f32(stream(), ptr(cv), ptr(out), B, M, P, C2 // 2),
          'usot_conf_fusion_reduce_f32')
    return out


def prroi_pool(features, rois, ph=7, pw=7, scale=1.0, out_nhwc=False):
    """features: NCHW-shaped tensor with ANY strides (dense NCHW or channels_last view);
    rois [R,5] device float32.  Returns NCHW-shaped [R,C,ph,pw] (channels_last strides when
    out_nhwc)."""
    _dev(features), _dev(rois)
    B, Cc, H, W_ = features.shape
    R = rois.shape[0]
    rois = rois.contiguous()
    if out_nhwc:
        buf = torch.zeros((R, ph, pw, Cc), device=features.device, dtype=torch.float32)
        out = buf.permute(0, 3, 1, 2)
    else:
        out = torch.zeros((R, Cc, ph, pw), device=features.device, dtype=torch.float32)
    fs, os_ = features.stride(), out.stride()
    check(lib().usot_prroi_pool_forward_f32(stream(), ptr(features), ptr(rois), ptr(out), R, Cc, H, W_, ph, pw,
                                            float(scale), fs[0], fs[1], fs[2], fs[3],
                                            os_[0], os_[1], os_[2], os_[3]), 'usot_prroi_pool_forward_f32')
    return out


def prroi_pool_backward(feature_shape, rois, top_diff, ph=7, pw=7, scale=1.0):
    """Feature gradient of Precise RoI Pooling (functional.py:71-73 -> prroi_pooling_gpu.c:46-77): dense NCHW
    [B,C,H,W] for top_diff [R,C,ph,pw]."""
    _dev(rois), _dev(top_diff)
    B, Cc, H, W_ = (int(v) for v in feature_shape)
    rois, top_diff = rois.contiguous(), top_diff.contiguous()
    out = torch.empty((B, Cc, H, W_), device=rois.device, dtype=torch.float32)        # zero-filled by the entry point
    check(lib().usot_prroi_pool_backward_f32(stream(), ptr(rois), ptr(top_diff), ptr(out), rois.shape[0], B, Cc, H, W_,
                                             ph, pw, float(scale)), 'usot_prroi_pool_backward_f32')
    return out


def prroi_pool_coor_backward(features, rois, top_data, top_diff, ph=7, pw=7, scale=1.0):
    """RoI gradient [R,5] (functional.py:74-76 -> prroi_pooling_gpu.c:79-113); column 0 (batch index) is zero."""
    _dev(features), _dev(rois)
    B, Cc, H, W_ = features.shape
    features, rois, top_data, top_diff = features.contiguous(), rois.contiguous(), top_data.contiguous(), top_diff.contiguous()
    out = torch.zeros((rois.shape[0], 5), device=rois.device, dtype=torch.float32)
    check(lib().usot_prroi_pool_coor_backward_f32(stream(), ptr(features), ptr(rois), ptr(top_data), ptr(top_diff), ptr(out),
                                                  rois.shape[0], B, Cc, H, W_, ph, pw, float(scale)),
          'usot_prroi_pool_coor_backward_f32')
    return out


def to_nhwc(t):
    """NCHW-shaped tensor (any strides) -> dense NHWC buffer [N,H,W,C] via the permute kernel."""
    _dev(t)
    N, Cc, H, W_ = t.shape
    s = t.stride()
    if s[1] == 1 and s[3] == Cc and s[2] == W_ * Cc and s[0] == H * W_ * Cc:
        return t.permute(0, 2, 3, 1)            # already channels-last in memory
    out = torch.empty((N, H, W_, Cc), device=t.device, dtype=torch.float32)
    check(lib().usot_permute4_f32(stream(), ptr(t), ptr(out), N, H, W_, Cc, s[0], s[2], s[3], s[1]),
          'usot_permute4_f32')
    return out


def to_nchw(t_nhwc):
    """Dense NHWC buffer -> dense NCHW tensor via the permute kernel."""
    _dev(t_nhwc)
    N, H, W_, Cc = t_nhwc.shape
    s = t_nhwc.stride()
    out = torch.empty((N, Cc, H, W_), device=t_nhwc.device, dtype=torch.float32)
    check(lib().usot_permute4_f32(stream(), ptr(t_nhwc), ptr(out), N, Cc, H, W_, s[0], s[3], s[1], s[2]),
          'usot_permute4_f32')
    return out


def decode(cls, cls_mem, bbox, window, S, instance_size, stride, ratio, penalty_k, window_influence, tw, th,
           out=None):
    _dev(cls), _dev(cls_mem), _dev(bbox), _dev(window, torch.float64)
    if out is None:
        out = torch.empty(8, device=cls.device, dtype=torch.float64)
    check(lib().usot_decode_f32(stream(), ptr(cls), ptr(cls_mem), ptr(bbox), ptr(window), ptr(out), S,
                                instance_size, stride, float(ratio), float(penalty_k),
                                float(window_influence), float(tw), float(th)), 'usot_decode_f32')
    return out


def conv2d_bf16(x, w, bias, *, KH, KW, stride=1, pad=(0, 0), dil=(1, 1), res=None, act=ACT_NONE, tile=0, out_f32=False,
                act2=ACT_NONE, act_split=0, groups=1):
    """x NHWC bf16|fp16 [N,H,W,Cin] (groups > 1: [G,N,H,W,Cin]), w packed same dtype [G*Cout, KH*KW*Cin],
    bias fp32 [G*Cout] -> y NHWC [N,OH,OW,Cout] ([G,N,OH,OW,Cout]) in the same dtype, or fp32 with out_f32."""
    lp = x.dtype
    if lp not in (torch.bfloat16, torch.float16):
        raise HipError('conv2d_bf16 takes bf16 or fp16 tensors')
    _dev(x, lp), _dev(w, lp)
    N, H, W_, Cin = x.shape[-4:]
    Cout = w.shape[0] // groups
    OH = (H + 2 * pad[0] - dil[0] * (KH - 1) - 1) // stride + 1
    OW = (W_ + 2 * pad[1] - dil[1] * (KW - 1) - 1) // stride + 1
    shape = (N, OH, OW, Cout) if groups == 1 else (groups, N, OH, OW, Cout)
    y = torch.empty(shape, device=x.device, dtype=torch.float32 if out_f32 else lp)
    d = conv_desc(x.data_ptr(), w.data_ptr(), bias.data_ptr() if bias is not None else None, y.data_ptr(),
                  N=N, H=H, W=W_, Cin=Cin, OH=OH, OW=OW, Cout=Cout, KH=KH, KW=KW, stride=stride, pad=pad, dil=dil,
                  res=res.data_ptr() if res is not None else None, act=act, act2=act2, act_split=act_split, tile=tile,
                  groups=groups, x_gs=N * H * W_ * Cin, w_gs=Cout * KH * KW * Cin, b_gs=Cout, y_gs=N * OH * OW * Cout)
    check(lib().usot_conv2d_lp(stream(), C.byref(d), 1 if lp == torch.float16 else 0, int(out_f32)), 'usot_conv2d_lp')
    return y


def pw_pair_pack(w, cm, co, cn, which):
    """Filter bank `w` ([CO,CM] for which = 0, [CN,CO] for which = 1) in the fragment order of the fused
    pointwise-pair kernel (usot_pw_pair_layout)."""
    n = w.numel() // 8
    row, k0 = (C.c_int32 * n)(), (C.c_int32 * n)()
    got = lib().usot_pw_pair_layout(int(cm), int(co), int(cn), int(which), row, k0)
    if got != n:
        raise HipError('usot_pw_pair_layout(%d, %d, %d, %d) = %d, expected %d chunks' % (cm, co, cn, which, got, n))
    r = torch.tensor(list(row), dtype=torch.long, device=w.device)
    k = torch.tensor(list(k0), dtype=torch.long, device=w.device)
    cols = k[:, None] + torch.arange(8, device=w.device)[None, :]
    return w[r[:, None], cols].contiguous().reshape(-1)


def pw_pair_f32_pack(w):
    """fp32 filter bank [rows, K] -> the fragment order of usot_pw_pair_f32: (column block, round, quad, row in block, 4 k)."""
    rows, k = w.shape
    return w.reshape(rows // 16, 16, k // 16, 4, 4).permute(0, 2, 3, 1, 4).contiguous().reshape(-1)


def pw_pair_s16_pack(w):
    """fp32 filter bank [rows, K] -> the split-fp16 bank of usot_pw_pair_f32s as one float32 tensor: rows x K floats of fragments
    (column block of 16 rows, 32-k step, hi | lo, quad, row in block, 8 halves) followed by the rows' factors 1 / (2^e x 8)."""
    rows, k = w.shape
    assert rows % 16 == 0 and k % 32 == 0
    w = w.float()
    amax = w.abs().amax(1)
    e = torch.where(amax > 0, torch.floor(torch.log2(1024.0 / amax.clamp_min(1e-30))), torch.zeros_like(amax))
    e = torch.where(amax * torch.exp2(e) >= 1024.0, e - 1, e).clamp(-100, 110)
    sw = torch.exp2(e)
    ws = w * sw[:, None]
    hi = ws.half()
    lo = (ws - hi.float()).half()
    frag = lambda t: t.reshape(rows // 16, 16, k // 32, 4, 8).permute(0, 2, 3, 1, 4)          # (cb, step, quad, row, 8)
    packed = torch.stack([frag(hi), frag(lo)], 2).contiguous().reshape(-1)                      # (cb, step, hi | lo, quad, row, 8)
    return torch.cat([packed.view(torch.float32), (1.0 / (sw * SPLIT16_X_SCALE)).float()]).contiguous()


def pw_pair_f32_supported(cm, co, cn):
    return bool(lib().usot_pw_pair_f32_supported(int(cm), int(co), int(cn)))


def pw_pair_f32(t2, w3, b3, res, w1, b1, act2=ACT_RELU, sliced=True, split16=False, ovf=None):
    """fp32 NHWC: Y = relu(t2 . w3^T + b3 + res), T = act2(Y . w1^T + b1); w3 [CO,CM], w1 [CN,CO] in natural order
    (packed here).  Returns (Y, T)."""
    for t in (t2, w3, b3, res, w1, b1):
        _dev(t)
    CM, (CO, CN) = t2.shape[-1], (w3.shape[0], w1.shape[0])
    M = t2.numel() // CM
    y = torch.empty(tuple(t2.shape[:-1]) + (CO,), device=t2.device, dtype=torch.float32)
    t = torch.empty(tuple(t2.shape[:-1]) + (CN,), device=t2.device, dtype=torch.float32)
    w3p, w1p = (pw_pair_s16_pack(w3), pw_pair_s16_pack(w1)) if split16 else (pw_pair_f32_pack(w3), pw_pair_f32_pack(w1))
    ws = pw_pair_f32_ws(M, CM, CO, CN, t2.device) if sliced else None
    d = pw_pair_desc(t2.data_ptr(), w3p.data_ptr(), b3.data_ptr(), res.data_ptr(), y.data_ptr(), w1p.data_ptr(), b1.data_ptr(),
                     t.data_ptr(), M, CM, CO, CN, act2, ws.data_ptr() if ws is not None else None,
                     ovf=ovf.data_ptr() if ovf is not None else None)
    fn = lib().usot_pw_pair_f32s if split16 else lib().usot_pw_pair_f32
    check(fn(stream(), C.byref(d)), 'usot_pw_pair_f32')
    if ws is not None:
        check(fn(stream(), C.byref(d)), 'usot_pw_pair_f32')      # a second launch finds the tickets reset
    return y, t


def pw_single_f32(x, w, b, res=None, act=ACT_NONE):
    """fp32 NHWC pointwise convolution on the small-M streaming kernel: y = act(x . w^T + b (+ res)); w [N,K] natural order."""
    _dev(x), _dev(w), _dev(b)
    K, N = x.shape[-1], w.shape[0]
    M = x.numel() // K
    y = torch.empty(tuple(x.shape[:-1]) + (N,), device=x.device, dtype=torch.float32)
    wp = pw_pair_f32_pack(w)
    check(lib().usot_pw_single_f32(stream(), ptr(x), ptr(wp), ptr(b), ptr(res) if res is not None else None, ptr(y), M, K, N, act),
          'usot_pw_single_f32')
    return y


def stream_conv3x3_f32(x, w, b, pad, dil, res=None, act=ACT_NONE):
    """fp32 NHWC 3x3 / stride-1 convolution on the small-M streaming kernel; w packed [N, 9*Cin] in (kh, kw, ci) order."""
    _dev(x), _dev(w), _dev(b)
    Nb, H, W_, Cin = x.shape
    N = w.shape[0]
    OH, OW = H + 2 * pad[0] - 2 * dil[0], W_ + 2 * pad[1] - 2 * dil[1]
    y = torch.empty((Nb, OH, OW, N), device=x.device, dtype=torch.float32)
    wp = pw_pair_f32_pack(w)
    check(lib().usot_stream_conv3x3_f32(stream(), ptr(x), ptr(wp), ptr(b), ptr(res) if res is not None else None, ptr(y),
                                        Nb, H, W_, Cin, OH, OW, N, pad[0], pad[1], dil[0], dil[1], act), 'usot_stream_conv3x3_f32')
    return y


def pw_triple_f32(x, w2, b2, w3, b3, res, w1, b1, pad=(1, 1), dil=(1, 1), act2=ACT_RELU):
    """fp32 NHWC: T2 = relu(conv3x3(x, w2) + b2); Y = relu(T2 . w3^T + b3 + res); T = act2(Y . w1^T + b1) in one launch.
    w2 packed [CM, 9*Cin] ((kh, kw, ci) order), w3 [CO, CM], w1 [CN, CO].  Returns (Y, T) as [Nb, OH, OW, C]."""
    for t in (x, w2, b2, w3, b3, res, w1, b1):
        _dev(t)
    Nb, H, W_, Cin = x.shape
    CM, CO, CN = w2.shape[0], w3.shape[0], w1.shape[0]
    OH, OW = H + 2 * pad[0] - 2 * dil[0], W_ + 2 * pad[1] - 2 * dil[1]
    y = torch.empty((Nb, OH, OW, CO), device=x.device, dtype=torch.float32)
    t = torch.empty((Nb, OH, OW, CN), device=x.device, dtype=torch.float32)
    w2p, w3p, w1p = pw_pair_f32_pack(w2), pw_pair_f32_pack(w3), pw_pair_f32_pack(w1)
    d = pw_pair_desc(None, w3p.data_ptr(), b3.data_ptr(), res.data_ptr(), y.data_ptr(), w1p.data_ptr(), b1.data_ptr(), t.data_ptr(),
                     Nb * OH * OW, CM, CO, CN, act2)
    check(lib().usot_pw_triple_f32(stream(), ptr(x), ptr(w2p), ptr(b2), C.byref(d), Nb, H, W_, Cin, OH, OW, pad[0], pad[1], dil[0], dil[1]),
          'usot_pw_triple_f32')
    return y, t


def pw_pair_supported(cm, co, cn):
    return bool(lib().usot_pw_pair_supported(int(cm), int(co), int(cn)))


def pw_pair_desc(t2, w3p, b3, res, y, w1, b1, t, M, CM, CO, CN, act2, ws=None, t2_parts=0, t2_bias=None, res_parts=0, res_bias=None,
                 ovf=None):
    d = PwPairDesc()
    d.t2, d.w3p, d.res, d.w1, d.b3, d.b1, d.y, d.t = t2, w3p, res, w1, b3, b1, y, t
    d.M, d.CM, d.CO, d.CN, d.act2 = M, CM, CO, CN, act2
    d.ws = ws
    d.t2_parts, d.t2_bias = t2_parts, t2_bias
    d.res_parts, d.res_bias = res_parts, res_bias
    d.ovf = ovf or None
    return d


def bneck_desc(x, w1, b1, w2, b2, w3c, b3c, wn, bn, y, t, N, H, W):
    d = BneckDesc()
    d.x, d.w1, d.w2, d.w3c, d.wn, d.b1, d.b2, d.b3c, d.bn, d.y, d.t = x, w1, w2, w3c, wn, b1, b2, b3c, bn, y, t
    d.N, d.H, d.W = N, H, W
    return d


def pw_pair_f32_ws(M, CM, CO, CN, device):
    """Zero-initialised workspace of the channel-sliced form of usot_pw_pair_f32, or None when the shape runs unsliced."""
    n = lib().usot_pw_pair_f32_ws_floats(int(M), int(CM), int(CO), int(CN))
    return torch.zeros(n, device=device, dtype=torch.float32) if n > 0 else None


def pw_pair(t2, w3, b3, res, w1, b1, act2=ACT_RELU):
    """Fused conv3 + residual + ReLU -> next 1x1 conv (+ act2) on low-precision [M, C] maps.
    t2 [M,CM], w3 [CO,CM] (natural rows), b3 fp32 [CO], res [M,CO], w1 [CN,CO], b1 fp32 [CN] -> (y [M,CO], t [M,CN])."""
    lp = t2.dtype
    if lp not in (torch.bfloat16, torch.float16):
        raise HipError('pw_pair takes bf16 or fp16 tensors')
    for a in (t2, w3, res, w1):
        _dev(a, lp)
    _dev(b3), _dev(b1)
    M, CM = t2.shape
    CO, CN = w3.shape[0], w1.shape[0]
    w3p, w1 = pw_pair_pack(w3, CM, CO, CN, 0), pw_pair_pack(w1, CM, CO, CN, 1)
    y = torch.empty((M, CO), device=t2.device, dtype=lp)
    t = torch.empty((M, CN), device=t2.device, dtype=lp)
    d = pw_pair_desc(t2.data_ptr(), w3p.data_ptr(), b3.data_ptr(), res.data_ptr(), y.data_ptr(), w1.data_ptr(), b1.data_ptr(),
                     t.data_ptr(), M, CM, CO, CN, act2)
    check(lib().usot_pw_pair_lp(stream(), C.byref(d), 1 if lp == torch.float16 else 0), 'usot_pw_pair_lp')
    return y, t


def crop_resize(frame_u8, out, x0, y0, win, fill):
    """frame_u8: device uint8 [H,W,3]; out: device float32 [3,S,S] (written in place)."""
    _dev(frame_u8, torch.uint8), _dev(out)
    if not frame_u8.is_contiguous() or not out.is_contiguous():
        raise HipError('crop_resize needs a dense HWC uint8 frame and a dense CHW output')
    H, W_, _ = frame_u8.shape
    S = out.shape[-1]
    check(lib().usot_crop_resize_u8_f32(stream(), ptr(frame_u8), ptr(out), H, W_, int(x0), int(y0), int(win), S,
                                        int(fill[0]), int(fill[1]), int(fill[2])), 'usot_crop_resize_u8_f32')
    return out


# ---- lock-step multi-video tracking (csrc/multitrack.hip; the control block is engine.STEP_CTL / SLOT_REC)
def decode_batch(cls, cls_mem, bbox, window, out, ctl, roi, S, instance_size, stride, ratio, penalty_k, window_influence):
    """cls / cls_mem [B,S,S] float32, bbox [B,4,S,S], window [S,S] float64 (device); out float64 [B,16] and roi float32 [B,5]
    (device or pinned); ctl: the step's control block (pinned or device uint8).  B = out.shape[0]."""
    for t in (cls, cls_mem, bbox, window, out, roi, ctl):
        if not t.is_contiguous():
            raise HipError('decode_batch needs dense tensors')
    B = out.shape[0]
    check(lib().usot_decode_batch_f32(stream(), ptr(cls), ptr(cls_mem), ptr(bbox), ptr(window), ptr(out), B, int(S),
                                      int(instance_size), int(stride), float(ratio), float(penalty_k), float(window_influence),
                                      ptr(ctl), ptr(roi)), 'usot_decode_batch_f32')
    return out


def rows_append_gather_batch(fresh, banks, picked, ctl, n_pick):
    """fresh: 4 tensors [B, ...]; banks: 4 tensors [B*cap, ...]; picked: 3 tensors [B*n_pick, ...] (float32, dense, device)."""
    B = fresh[0].shape[0]
    rl = [int(b[0].numel()) for b in banks]
    check(lib().usot_rows_append_gather_batch_f32(
        stream(), (C.c_void_p * 4)(*[t.data_ptr() for t in fresh]), (C.c_void_p * 4)(*[t.data_ptr() for t in banks]),
        (C.c_void_p * 3)(*[t.data_ptr() for t in picked]), (C.c_int32 * 4)(*rl), ptr(ctl), B, int(n_pick), int(banks[0].shape[0])),
        'usot_rows_append_gather_batch_f32')


def crop_resize_batch(ctl, out):
    """out: device float32 [B,3,S,S]; each slot's image address and window come from its control-block record."""
    _dev(out)
    if not out.is_contiguous():
        raise HipError('crop_resize_batch needs a dense [B,3,S,S] output')
    check(lib().usot_crop_resize_batch_u8_f32(stream(), ptr(ctl), ptr(out), out.shape[0], out.shape[-1]),
          'usot_crop_resize_batch_u8_f32')
    return out

