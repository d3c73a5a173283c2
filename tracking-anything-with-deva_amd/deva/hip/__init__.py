"""ctypes binding of libdeva_hip.so (C ABI declared in include/deva_hip.h).

The library is the only compute backend of this package: there is no PyTorch/CPU fallback.
`lib()` raises if the shared object has not been built (`python __graft_entry__.py`), and every
wrapper in `ops.py` raises if handed a tensor that is not a contiguous fp32 HIP tensor.
"""
import ctypes
import os
from ctypes import POINTER, Structure, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_uint32, c_void_p

from . import _native

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libdeva_hip.so')
ABI_VERSION = 11

ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_SQUARE_PLUS_ONE = 0, 1, 2, 3
KLAYOUT_TAP_MAJOR, KLAYOUT_CHUNK32 = 0, 1
KLAYOUT_Q4 = 16  # flag: k-quad interleaved storage


class ConvDesc(Structure):
    """mirror of `struct deva_conv_desc` (include/deva_hip.h)"""
    _fields_ = [
        ('in0', c_void_p), ('in1', c_void_p),
        ('in0_batch_stride', c_int64), ('in1_batch_stride', c_int64),
        ('c0', c_int32), ('c1', c_int32),
        ('batch', c_int32), ('height', c_int32), ('width', c_int32),
        ('weight', c_void_p), ('bias', c_void_p),
        ('cout', c_int32), ('cout_pad', c_int32),
        ('k_layout', c_int32),
        ('kh', c_int32), ('kw', c_int32), ('stride', c_int32), ('pad', c_int32),
        ('relu_in', c_int32),
        ('residual', c_void_p), ('residual_batch_stride', c_int64),
        ('act', c_int32),
        ('out', c_void_p),
        ('in_guard_elems', c_int32),
        ('workspace', c_void_p), ('workspace_elems', c_int64),
        ('weight_f16', c_void_p), ('amp', c_int32),
        ('split_scale_log2', c_int32), ('split_flag', c_void_p),
        ('weight_wino', c_void_p),
    ]


# kernel families of a convolution plan (include/deva_hip.h: DEVA_CONV_*), by value
CONV_FAMILIES = ('none', 'cout1_table', 'cout1_rows', 'wino', 'f16', 'split', 'q4', 'igemm')
CONV_IGEMM_VEC, CONV_IGEMM_ROW = 4, 8


class ConvLaunch(Structure):
    """mirror of `struct deva_conv_launch` (include/deva_hip.h)"""
    _fields_ = [
        ('family', c_int32), ('bm', c_int32), ('bn', c_int32), ('waves', c_int32), ('wk', c_int32), ('kind', c_int32),
        ('persistent', c_int32), ('tiles_m', c_int32), ('tiles_n', c_int32),
        ('splits', c_int32), ('per_split', c_int32), ('group_m', c_int32),
        ('grid_x', c_uint32), ('grid_y', c_uint32), ('block', c_uint32),
    ]


class ConvPlan(Structure):
    """mirror of `struct deva_conv_plan` (include/deva_hip.h)"""
    _fields_ = [('first', ConvLaunch), ('rerun', ConvLaunch), ('aliased', c_int32), ('sub_batch', c_int32)]


ENSEMBLE_MAX_VARIANTS = 8


class EnsembleVariant(Structure):
    """mirror of `struct deva_ensemble_variant` (include/deva_hip.h)"""
    _fields_ = [
        ('src', c_void_p),
        ('plane_stride', c_int64), ('row_stride', c_int64),
        ('channels', c_int32), ('height', c_int32), ('width', c_int32),
        ('flip', c_int32),
    ]


# name -> (restype, argtypes); must list every symbol of include/deva_hip.h
SIGNATURES = {
    'deva_hip_version': (c_int, []),
    'deva_hip_last_error': (c_char_p, []),
    'deva_conv2d': (c_int, [POINTER(ConvDesc), c_void_p]),
    'deva_conv2d_plan': (c_int, [POINTER(ConvDesc), POINTER(ConvPlan)]),
    'deva_conv_pack_f16': (c_int64, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, POINTER(c_int)]),
    'deva_conv_pack_split': (c_int64, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, POINTER(c_int), POINTER(c_int)]),
    'deva_conv_pack_wino': (c_int64, [c_void_p, c_void_p, c_int, c_int]),
    'deva_conv_pack': (c_int64, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, POINTER(c_int), POINTER(c_int)]),
    'deva_maxpool3x3s2': (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_void_p]),
    'deva_upsample2x_add': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    'deva_area_downsample': (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_void_p]),
    'deva_aggregate': (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_int64, c_void_p]),
    'deva_softmax_channels': (c_int, [c_void_p, c_void_p, c_int, c_int64, c_void_p]),
    'deva_upsample4x_softmax': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    'deva_global_avgmax': (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p]),
    'deva_cbam_mlp': (c_int, [c_void_p] * 7 + [c_int, c_int, c_int, c_void_p]),
    'deva_cbam_channel_pool': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    'deva_cbam_apply': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    'deva_stem7x7': (c_int, [c_void_p, c_int64, c_int, c_void_p, c_int64, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int,
                             c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    'deva_stem_pack': (c_int64, [c_void_p, c_int, c_void_p, c_void_p, POINTER(c_int)]),
    'deva_pad2d': (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    'deva_usage_init': (c_int, [c_void_p, c_void_p, c_int, c_void_p]),
    'deva_upsample2x_add_ds2': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    'deva_upsample2x_add_map': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    'deva_upsample2x_add_ds2_map': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                            c_void_p]),
    'deva_gather_s2': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    'deva_gru_update': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    'deva_affinity_topk': (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                   c_int, c_int, c_int, c_void_p, c_void_p]),
    'deva_affinity_finalize': (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    'deva_affinity_workspace': (c_int64, [c_int, c_int, c_int]),
    'deva_affinity_force_shape': (c_int, [c_int]),
    'deva_affinity_default_splits': (c_int, [c_int, c_int]),
    'deva_usage_update': (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int, c_void_p]),
    'deva_readout_sparse': (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_int,
                                    c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    'deva_affinity_select': (c_int, [c_void_p, c_int, c_int, c_int, c_int64, c_void_p, c_void_p, c_void_p]),
    'deva_affinity_read': (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int,
                                   c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    'deva_affinity_read_prepared': (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int,
                                            c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int,
                                            c_void_p]),
    'deva_affinity_bank_prep_bytes': (c_int64, [c_int]),
    'deva_affinity_read_scratch': (c_int64, [c_int, c_int, c_int]),
    'deva_affinity_dense': (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int,
                            c_void_p, c_void_p, c_void_p, c_void_p]),
    'deva_dense_read': (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int,
                                POINTER(c_void_p), POINTER(c_void_p), c_int, POINTER(c_void_p), c_void_p, c_void_p, c_int64,
                                c_void_p, c_void_p]),
    'deva_dense_read_scratch': (c_int64, [c_int, c_int]),
    'deva_affinity_prefilter_enabled': (c_int, [c_int, c_int, c_int]),
    'deva_affinity_force_prefilter': (c_int, [c_int]),
    'deva_probe_mfma_f32': (c_int64, [c_void_p, c_int64, c_void_p, c_int, c_void_p]),
    'deva_affinity_read_flag': (c_int, [c_void_p, c_void_p]),
    'deva_affinity_read_stats': (c_int, [c_void_p, c_int, c_int, c_int, POINTER(c_int64), c_void_p]),
    'deva_affinity_merge': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    'deva_bank_append': (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p]),
    'deva_bank_gather_rows': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p]),
    'deva_bank_export': (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p]),
    'deva_rank': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    'deva_rank_select': (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p]),
    'deva_evict_select': (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    'deva_similarity_dense': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p,
                                      c_void_p]),
    'deva_softmax_columns': (c_int, [c_void_p, c_int, c_int, c_int, c_void_p]),
    'deva_label_histogram': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int64, c_void_p, c_void_p]),
    'deva_lut_remap': (c_int, [c_void_p, c_void_p, c_int, c_int64, c_void_p, c_void_p]),
    'deva_input_head': (c_int, [c_void_p, c_int, c_int, POINTER(c_float), POINTER(c_float), c_int, c_void_p, c_int, c_int,
                                c_int, c_int, c_int, c_int, c_void_p]),
    'deva_index_mask': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p]),
    'deva_merge_paint': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_int, c_int64, c_void_p, c_void_p]),
    'deva_scores_u8': (c_int, [POINTER(EnsembleVariant), c_int, c_int, c_void_p, c_void_p]),
    'deva_ensemble_index_mask': (c_int, [POINTER(EnsembleVariant), c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p,
                                         c_void_p]),
    'deva_flip_w': (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p]),
    'deva_frame_result': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p,
                                  c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'deva_mask_rle_scratch': (c_int64, [c_int, c_int, c_int]),
    'deva_mask_rle_count': (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int64, c_void_p, c_void_p]),
    'deva_mask_rle_write': (c_int, [c_int, c_int, c_int, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p]),
    'deva_detection_scratch': (c_int64, [c_int, c_int, c_int, c_int, c_int]),
    'deva_detection_assemble': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_double, c_int, c_void_p,
                                        c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    'deva_proposal_scratch': (c_int64, [c_int]),
    'deva_proposal_begin': (c_int, [c_int, c_void_p, c_int64, c_void_p]),
    'deva_proposal_batch': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_double, c_double, c_double, c_double,
                                    c_void_p, c_int, c_void_p, c_int64, c_void_p]),
    'deva_proposal_finish': (c_int, [c_int, c_double, c_void_p, c_int64, c_void_p, c_void_p]),
    'deva_proposal_gather': (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int64, c_int, c_void_p, c_void_p]),
    'deva_box_nms': (c_int, [c_void_p, c_void_p, c_int, c_double, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    'deva_box_nms_xyxy': (c_int, [c_void_p, c_void_p, c_int, c_double, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    'deva_box_mask_select': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_double, c_void_p, c_void_p, c_void_p]),
    'deva_prompt_scratch': (c_int64, [c_int, c_int, c_int]),
    'deva_prompt_points': (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_double, c_void_p, c_int64, c_void_p, c_void_p,
                                   c_void_p, c_void_p]),
}

_LIB = None


class DevaHipError(RuntimeError):
    pass


def lib() -> ctypes.CDLL:
    """Load (once) and return the native library; raises if it has not been built."""
    return _LIB or _native.load(globals(), 'deva_hip_version', 'libdeva_hip.so', 'the HIP kernels')


def check(code: int, what: str) -> None:
    if code != 0:   # (tested here: the inference wrappers call this after every launch)
        _native.check(globals(), code, what, 'deva_hip_last_error')
