"""ctypes binding of ``libexabm4d.so`` (the C-ABI declared in ``include/exabm4d.h``).

There is no CPU fallback: if the shared library is missing, or no MI355X is visible when a
compute entry point is called, this module raises.  Contexts are per (process id, device) and are
created lazily, *after* any ``fork()`` -- the reference calls ``bm4d`` from forked
``ProcessPoolExecutor`` workers (reference ``scripts/precompute.py:215``).
"""
import ctypes
import importlib.util
import os
import sys
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_CANDIDATES = [
    os.environ.get("EXABM4D_LIB", ""),
    os.path.join(os.path.dirname(_HERE), "csrc", "libexabm4d.so"),
]

c_f32p = ctypes.POINTER(ctypes.c_float)
c_u16p = ctypes.POINTER(ctypes.c_uint16)
c_u32p = ctypes.POINTER(ctypes.c_uint32)
c_i32p = ctypes.POINTER(ctypes.c_int32)
c_i64p = ctypes.POINTER(ctypes.c_int64)
c_vp = ctypes.c_void_p

KEY_EMPTY = 0xFFFFFFFF
LABEL_SET_MAX = 1024        # exabm4d.h EXABM4D_LABEL_SET_MAX: distinct labels one patch's device set holds
RASTER_BOXES = 256          # exabm4d.h EXABM4D_RASTER_BOXES: box origins one rasteriser launch keeps in LDS
SEG_STATS_K = 23            # exabm4d.h EXABM4D_SEG_STATS_K
GAUSS_MAX_RADIUS = 64       # exabm4d.h EXABM4D_GAUSS_MAX_RADIUS
NOISE_LEVELS = 49           # exabm4d.h EXABM4D_NOISE_LEVELS
NOISE_BINS = 4096           # exabm4d.h EXABM4D_NOISE_BINS
FG_MAX_RADIUS = 8           # exabm4d.h EXABM4D_FG_MAX_RADIUS: iterations of Context.foreground_box_u16
DS_METHODS = {"mode": 0, "mean": 1, "max": 2}   # exabm4d.h EXABM4D_DS_MODE / _MEAN / _MAX: Context.downsample_box_u16
DS_EDGES = {"crop": 0, "partial": 1}            # exabm4d.h EXABM4D_DS_CROP / _PARTIAL
LABEL_ZEROS = {"count": 0, "ignore": 1}         # exabm4d.h EXABM4D_LABEL_ZEROS_COUNT / _IGNORE: Context.downsample_box_labels
CC_TILE = (8, 8, 64)        # exabm4d.h EXABM4D_CC_TILE_Z / _Y / _X: the tile Context.component_seeds_u16 labels in LDS
NOISE_WIDE_BINS = 16384     # exabm4d.h EXABM4D_NOISE_WIDE_BINS: wide bins per level of Context.measure_box_u16
COUNT_BINS = 65536          # exabm4d.h EXABM4D_COUNT_BINS: counters of a table of the uint16 counts
EVAL_K = 16                 # exabm4d.h EXABM4D_EVAL_K: doubles per patch of Context.evaluate_batch
# exabm4d.h EXABM4D_EVAL_*: the columns of such a row after those of masked_error_stats (0..5)
EVAL_MED, EVAL_MAD, EVAL_THR, EVAL_RAW_LO, EVAL_RAW_HI, EVAL_PRED_LO, EVAL_PRED_HI = 6, 7, 8, 9, 10, 11, 12
EVAL_PRED_NAN, EVAL_RAW_NAN, EVAL_TARGET_NAN = 13, 14, 15
# exabm4d.h label element types
LABEL_DTYPES = {np.dtype(np.uint8): 0, np.dtype(np.uint32): 1, np.dtype(np.uint64): 2,
                np.dtype(np.int32): 3, np.dtype(np.int64): 4}
DIFF_BINS = 131071          # exabm4d.h EXABM4D_DIFF_BINS: bins of a signed difference table (test - ref + 65535)
DATA_EXP_AUTO = -2 ** 31    # exabm4d.h EXABM4D_DATA_EXP_AUTO: E per volume from the data (fp32 entry points)
DATA_EXP_U16 = 17           # exabm4d.h EXABM4D_DATA_EXP_U16: the uint16 pipelines' fixed E
DTYPE_F32, DTYPE_F16, DTYPE_BF16 = 0, 1, 2   # exabm4d.h exabm4d_dtype: element types of the *_dt_dev entries


class Params(ctypes.Structure):
    """``exabm4d_params`` (include/exabm4d.h)."""

    _fields_ = [
        ("size", ctypes.c_uint32),
        ("block", ctypes.c_int32),
        ("step", ctypes.c_int32),
        ("search", ctypes.c_int32),
        ("max_group", ctypes.c_int32),
        ("lambda_ht", ctypes.c_float),
        ("c_match_ht", ctypes.c_float),
        ("c_match_wie", ctypes.c_float),
        ("kaiser_beta", ctypes.c_float),
    ]


class Transform(ctypes.Structure):
    """``exabm4d_transform`` (include/exabm4d.h)."""

    _fields_ = [
        ("size", ctypes.c_uint32),
        ("kind", ctypes.c_int32),
        ("wrapped", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
        ("wrap_offset", ctypes.c_double),
        ("max_count", ctypes.c_double),
        ("offset", ctypes.c_double),
        ("scale", ctypes.c_double),
        ("norm", ctypes.c_double),
        ("gain", ctypes.c_double),
        ("read_noise", ctypes.c_double),
        ("c_inv", ctypes.c_double),
        ("mn", ctypes.c_double),
        ("mx", ctypes.c_double),
        ("clip", ctypes.c_double),
    ]


class PgNoise(ctypes.Structure):
    """``exabm4d_pg_noise`` (include/exabm4d.h): the Poisson-Gaussian model and the inverse to use."""

    _fields_ = [
        ("size", ctypes.c_uint32),
        ("gain", ctypes.c_float),
        ("read_noise", ctypes.c_float),
        ("offset", ctypes.c_float),
        ("inverse", ctypes.c_int32),
    ]


class PatchGrid(ctypes.Structure):
    """``exabm4d_patch_grid`` (include/exabm4d.h): a brick's patches as a regular grid."""

    _fields_ = [
        ("first", ctypes.c_int32 * 3),
        ("count", ctypes.c_int32 * 3),
        ("stride", ctypes.c_int32),
        ("patch", ctypes.c_int32),
    ]


def patch_grid(first, count, stride, patch):
    """A filled ``PatchGrid``: per axis (z, y, x) the first patch index and the number of patches."""
    g = PatchGrid()
    g.first[:] = [int(v) for v in first]
    g.count[:] = [int(v) for v in count]
    g.stride, g.patch = int(stride), int(patch)
    return g


PG_INVERSES = {"algebraic": 0, "asymptotic": 1, "closed_form": 2}    # exabm4d.h EXABM4D_PG_INVERSE_*


def pg_noise(gain, read_noise, offset, inverse="closed_form"):
    """A filled ``PgNoise``; ``inverse`` by name (PG_INVERSES) or by its code.  The library validates the values."""
    if isinstance(inverse, str):
        if inverse not in PG_INVERSES:
            raise ValueError("inverse must be one of %s, not %r" % (sorted(PG_INVERSES), inverse))
        inverse = PG_INVERSES[inverse]
    return PgNoise(ctypes.sizeof(PgNoise), float(gain), float(read_noise), float(offset), int(inverse))


# name -> (restype, argtypes); every symbol include/exabm4d.h declares
_CTX = c_vp
_PP = ctypes.POINTER(Params)
_NP = ctypes.POINTER(PgNoise)
_TP = ctypes.POINTER(Transform)
_GP = ctypes.POINTER(PatchGrid)
_I, _F, _SZ = ctypes.c_int, ctypes.c_float, ctypes.c_size_t
SIGNATURES = {
    "exabm4d_version": (_I, []),
    "exabm4d_last_error": (ctypes.c_char_p, [_CTX]),
    "exabm4d_device_count": (_I, []),
    "exabm4d_create": (_I, [_I, ctypes.POINTER(_CTX)]),
    "exabm4d_destroy": (_I, [_CTX]),
    "exabm4d_set_stream": (_I, [_CTX, c_vp]),
    "exabm4d_reset_stream": (_I, [_CTX]),
    "exabm4d_sync": (_I, [_CTX]),
    "exabm4d_default_params": (_I, [_PP]),
    "exabm4d_set_option": (_I, [_CTX, ctypes.c_char_p, _I]),
    "exabm4d_profile_read": (_I, [_CTX, c_f32p, _I]),
    "exabm4d_malloc": (_I, [_CTX, _SZ, ctypes.POINTER(c_vp)]),
    "exabm4d_free": (_I, [_CTX, c_vp]),
    "exabm4d_memcpy_h2d": (_I, [_CTX, c_vp, c_vp, _SZ]),
    "exabm4d_memcpy_d2h": (_I, [_CTX, c_vp, c_vp, _SZ]),
    "exabm4d_memset": (_I, [_CTX, c_vp, _I, _SZ]),
    "exabm4d_event_create": (_I, [_CTX, ctypes.POINTER(c_vp)]),
    "exabm4d_event_destroy": (_I, [_CTX, c_vp]),
    "exabm4d_event_record": (_I, [_CTX, c_vp]),
    "exabm4d_event_elapsed_ms": (_I, [_CTX, c_vp, c_vp, c_f32p]),
    "exabm4d_grid_count": (_I, [_I]),
    "exabm4d_grid_positions": (_I, [_I, c_i32p]),
    "exabm4d_tables": (_I, [_PP, c_f32p, c_f32p]),
    "exabm4d_scratch_bytes": (_SZ, [_I, _I, _I, _I, _I]),
    "exabm4d_blockmatch_dev": (_I, [_CTX, c_vp, _I, _I, _I, _I, _F, _F, _PP, c_vp]),
    "exabm4d_blockmatch_u16_dev": (_I, [_CTX, c_vp, _I, _I, _I, _I, _F, _F, _PP, c_vp]),
    "exabm4d_match_decode": (_I, [c_u32p, _I, _I, _I, _I, _I, c_i64p, c_f32p,
                                  ctypes.POINTER(_I)]),
    "exabm4d_stage_dev": (_I, [_CTX, c_vp, c_vp, c_vp, _I, _I, _I, _I, _F, _PP, _I, c_vp, c_vp]),
    "exabm4d_normalize_dev": (_I, [_CTX, c_vp, c_vp, c_vp, _SZ, _F, _F]),
    "exabm4d_counts_from_u16_dev": (_I, [_CTX, c_vp, c_vp, _SZ, _F]),
    "exabm4d_round_counts_f32_dev": (_I, [_CTX, c_vp, c_vp, _SZ, _F]),
    "exabm4d_normalize_u16_dev": (_I, [_CTX, c_vp, c_vp, c_vp, _SZ, _F]),
    "exabm4d_denoise_f32_dev": (_I, [_CTX, c_vp, c_vp, _I, _I, _I, _I, _F, _PP, _I, _F, _F]),
    "exabm4d_denoise_u16_dev": (_I, [_CTX, c_vp, c_vp, _I, _I, _I, _I, _F, _F, _PP, _I]),
    "exabm4d_denoise_chunked_u16_dev": (_I, [_CTX, c_vp, c_vp, _I, _I, _I, _I, _I, _I, _I, _F, _F, _PP,
                                             _I]),
    "exabm4d_denoise_pg_u16_dev": (_I, [_CTX, c_vp, c_vp, _I, _I, _I, _I, _NP, _PP, _I]),
    "exabm4d_denoise_pg_chunked_u16_dev": (_I, [_CTX, c_vp, c_vp, _I, _I, _I, _I, _I, _I, _I, _NP, _PP, _I]),
    "exabm4d_denoise_pg_chunked_u16_host": (_I, [_CTX, c_vp, c_vp, _I, _I, _I, _I, _I, _NP, _PP, _I]),
    "exabm4d_gat_forward_u16_dev": (_I, [_CTX, _NP, c_vp, c_vp, _SZ]),
    "exabm4d_gat_inverse_u16_dev": (_I, [_CTX, _NP, c_vp, c_vp, _SZ]),
    "exabm4d_blockmatch_plan": (_I, [_CTX, _I, _I, _I, _I, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint64)]),
    "exabm4d_denoise_chunked_u16_host": (_I, [_CTX, c_vp, c_vp, _I, _I, _I, _I, _I, _F, _F, _PP, _I]),
    "exabm4d_denoise_f32_host": (_I, [_CTX, c_vp, c_vp, _I, _I, _I, _I, _F, _PP, _I, _F, _F]),
    "exabm4d_denoise_f32_host_v": (_I, [_CTX, c_vp, c_vp, _I, _I, _I, _I, _F, _PP, _I, _F, _F]),
    "exabm4d_groupnorm_workspace_bytes": (_SZ, [_I, _SZ, _I, _I]),
    "exabm4d_groupnorm_lrelu_ndhwc_dev": (_I, [_CTX, c_vp, c_vp, c_vp, _I, _SZ, _I, _I, c_vp, c_vp, _F, _F, c_vp, _SZ,
                                                c_vp]),
    "exabm4d_maxpool2_ndhwc_dev": (_I, [_CTX, c_vp, c_vp, c_vp, _I, _I, _I, _I, _I]),
    "exabm4d_upsample2_trilinear_ndhwc_dev": (_I, [_CTX, c_vp, c_vp, c_vp, _I, _I, _I, _I, _I]),
    "exabm4d_groupnorm_lrelu_ndhwc_dt_dev": (_I, [_CTX, c_vp, _I, c_vp, c_vp, _I, _SZ, _I, _I, c_vp, c_vp, _F, _F,
                                                   c_vp, _SZ, c_vp]),
    "exabm4d_maxpool2_ndhwc_dt_dev": (_I, [_CTX, c_vp, _I, c_vp, c_vp, _I, _I, _I, _I, _I]),
    "exabm4d_upsample2_trilinear_ndhwc_dt_dev": (_I, [_CTX, c_vp, _I, c_vp, c_vp, _I, _I, _I, _I, _I]),
    "exabm4d_groupnorm_lrelu_ndhwc_train_dev": (_I, [_CTX, c_vp, c_vp, c_vp, _I, _SZ, _I, _I, c_vp, c_vp, _F, _F, c_vp,
                                                      _SZ, c_vp]),
    "exabm4d_groupnorm_lrelu_bwd_workspace_bytes": (_SZ, [_I, _SZ, _I, _I]),
    "exabm4d_groupnorm_lrelu_bwd_ndhwc_dev": (_I, [_CTX, c_vp, c_vp, c_vp, c_vp, c_vp, _I, _SZ, _I, _I, c_vp, c_vp, _F,
                                                    c_vp, c_vp, c_vp, _SZ]),
    "exabm4d_maxpool2_bwd_ndhwc_dev": (_I, [_CTX, c_vp, c_vp, c_vp, c_vp, _I, _I, _I, _I, _I]),
    "exabm4d_upsample2_trilinear_bwd_ndhwc_dev": (_I, [_CTX, c_vp, c_vp, c_vp, _I, _I, _I, _I, _I]),
    "exabm4d_groupnorm_lrelu_ndhwc_train_dt_dev": (_I, [_CTX, c_vp, _I, c_vp, c_vp, _I, _SZ, _I, _I, c_vp, c_vp, _F, _F,
                                                         c_vp, _SZ, c_vp]),
    "exabm4d_groupnorm_lrelu_bwd_ndhwc_dt_dev": (_I, [_CTX, c_vp, _I, c_vp, c_vp, c_vp, c_vp, _I, _SZ, _I, _I, c_vp,
                                                       c_vp, _F, c_vp, c_vp, c_vp, _SZ]),
    "exabm4d_maxpool2_bwd_ndhwc_dt_dev": (_I, [_CTX, c_vp, _I, c_vp, c_vp, c_vp, _I, _I, _I, _I, _I]),
    "exabm4d_upsample2_trilinear_bwd_ndhwc_dt_dev": (_I, [_CTX, c_vp, _I, c_vp, c_vp, _I, _I, _I, _I, _I]),
    "exabm4d_charbonnier_workspace_bytes": (_SZ, []),
    "exabm4d_charbonnier_loss_dev": (_I, [_CTX, c_vp, c_vp, c_vp, c_vp, _I, _SZ, ctypes.c_double, ctypes.c_double,
                                           c_vp, _SZ, c_vp]),
    "exabm4d_charbonnier_loss_bwd_dev": (_I, [_CTX, c_vp, c_vp, c_vp, c_vp, _I, _SZ, ctypes.c_double,
                                               ctypes.c_double, c_vp, c_vp]),
    "exabm4d_host_register": (_I, [_CTX, c_vp, ctypes.c_size_t]),
    "exabm4d_host_unregister": (_I, [_CTX, c_vp]),
    "exabm4d_transform_forward_u16_dev": (_I, [_CTX, _TP, c_vp, c_vp, _SZ]),
    "exabm4d_transform_forward_f32_dev": (_I, [_CTX, _TP, c_vp, c_vp, _SZ]),
    "exabm4d_transform_inverse_u16_dev": (_I, [_CTX, _TP, c_vp, c_vp, _SZ]),
    "exabm4d_transform_inverse_f32_dev": (_I, [_CTX, _TP, c_vp, c_vp, _SZ]),
    "exabm4d_tile_gather_dev": (_I, [_CTX, c_vp, _I, _I, _I, c_i32p, _I, _I, c_vp]),
    "exabm4d_tile_accumulate_dev": (_I, [_CTX, c_vp, c_i32p, _I, _I, _I, c_vp, c_vp, _I, _I, _I]),
    "exabm4d_tile_finalize_u16_dev": (_I, [_CTX, _TP, c_vp, c_vp, c_vp, _SZ]),
    "exabm4d_tile_gather_u16_dev": (_I, [_CTX, c_vp, c_i32p, c_i32p, c_i32p, _TP, _GP, ctypes.c_longlong, _I, c_vp]),
    "exabm4d_tile_stitch_u16_dev": (_I, [_CTX, c_vp, ctypes.c_longlong, _GP, _I, c_i32p, c_i32p, c_i32p, _TP, c_vp]),
    "exabm4d_chunk_byte_histograms_dev": (_I, [_CTX, c_vp, _I, _I, _I, _I, _I, _I, c_vp]),
    "exabm4d_dctq_forward_dev": (_I, [_CTX, c_vp, _I, _I, _I, ctypes.c_float, c_vp]),
    "exabm4d_dctq_inverse_dev": (_I, [_CTX, c_vp, _I, _I, _I, ctypes.c_float, c_vp]),
    "exabm4d_i32_symbol_histogram_dev": (_I, [_CTX, c_vp, _SZ, c_vp]),
    "exabm4d_comm_unique_id": (_I, [c_vp]),
    "exabm4d_comm_create": (_I, [_CTX, _I, _I, c_vp, ctypes.POINTER(c_vp)]),
    "exabm4d_comm_destroy": (_I, [c_vp]),
    "exabm4d_halo_exchange_dev": (_I, [_CTX, c_vp, _I, c_vp, c_vp, _SZ, _I, c_vp, c_vp, _SZ]),
    "exabm4d_comm_max_f64_host": (_I, [_CTX, c_vp, ctypes.POINTER(ctypes.c_double)]),
    "exabm4d_codec_chunk_bound": (_SZ, [_SZ, _I]),
    "exabm4d_codec_volume_bound": (_SZ, [_I, _I, _I, _I, _I, _I, _I]),
    "exabm4d_codec_encode_dev": (_I, [_CTX, c_vp, _I, _I, _I, _I, _I, _I, _I, _I, c_vp, _SZ, c_vp, c_vp,
                                      c_vp]),
    "exabm4d_codec_decode_dev": (_I, [_CTX, c_vp, _SZ, c_vp, _I, _I, _I, _I, _I, _I, _I, c_vp]),
    "exabm4d_dctq_ladder_errors_dev": (_I, [_CTX, c_vp, _I, _I, _I, _I, _I, _I, c_vp]),
    "exabm4d_bounded_volume_bound": (_SZ, [_I, _I, _I, _I, _I, _I]),
    "exabm4d_bounded_encode_dev": (_I, [_CTX, c_vp, _I, _I, _I, _I, _I, _I, _I, c_vp, _SZ, c_vp, c_vp, c_vp]),
    "exabm4d_bounded_decode_dev": (_I, [_CTX, c_vp, _SZ, c_vp, _I, _I, _I, _I, _I, _I, c_vp]),
    "exabm4d_block_bounded_volume_bound": (_SZ, [_I, _I, _I, _I, _I, _I]),
    "exabm4d_block_bounded_steps_dev": (_I, [_CTX, c_vp, c_vp, _I, _I, _I, _I, _I, _I, _I, _I, c_vp]),
    "exabm4d_block_bounded_encode_dev": (_I, [_CTX, c_vp, c_vp, _I, _I, _I, _I, _I, _I, _I, _I, c_vp, _SZ, c_vp, c_vp,
                                              c_vp]),
    "exabm4d_block_bounded_steps_tab_dev": (_I, [_CTX, c_vp, c_vp, _I, _I, _I, _I, _I, _I, _I, _I, c_vp, c_vp]),
    "exabm4d_block_bounded_encode_tab_dev": (_I, [_CTX, c_vp, c_vp, _I, _I, _I, _I, _I, _I, _I, _I, c_vp, _SZ, c_vp,
                                                  c_vp, c_vp, c_vp]),
    "exabm4d_block_bounded_decode_dev": (_I, [_CTX, c_vp, _SZ, c_vp, _I, _I, _I, _I, _I, _I, c_vp]),
    "exabm4d_u16_histogram_dev": (_I, [_CTX, c_vp, _SZ, c_vp]),
    "exabm4d_key_histogram_dev": (_I, [_CTX, c_vp, _I, _SZ, _I, ctypes.c_double, _I,
                                       ctypes.c_uint64, c_vp]),
    "exabm4d_minmax_dev": (_I, [_CTX, c_vp, _I, _SZ, c_vp]),
    "exabm4d_masked_error_stats_dev": (_I, [_CTX, c_vp, _I, c_vp, _I, c_vp, _SZ,
                                            ctypes.c_double, c_vp]),
    "exabm4d_ssim3d_dev": (_I, [_CTX, c_vp, c_vp, _I, _I, _I, _I, _I, ctypes.c_double,
                                ctypes.c_double, c_vp]),
    "exabm4d_diff_histogram_u16_dev": (_I, [_CTX, c_vp, c_vp, c_vp, c_i32p, c_i32p, c_i32p, c_i32p, c_i32p, _I, c_vp]),
    "exabm4d_mip3_u16_dev": (_I, [_CTX, c_vp, c_vp, c_i32p, c_i32p, c_i32p, c_i32p, c_i32p, c_vp]),
    "exabm4d_ssim3d_box_dev": (_I, [_CTX, c_vp, c_vp, c_i32p, c_i32p, c_i32p, c_i32p, c_i32p, _I, ctypes.c_double,
                                    ctypes.c_double, c_vp]),
    "exabm4d_noise_table_dev": (_I, [_CTX, c_vp, _I, _I, _I, _I, _I, c_vp, c_vp, c_vp]),
    "exabm4d_measure_box_u16_dev": (_I, [_CTX, c_vp, c_vp, c_i32p, c_i32p, c_i32p, c_i32p, c_i32p, _I, c_vp, c_vp]),
    "exabm4d_foreground_box_u16_dev": (_I, [_CTX, c_vp, c_i32p, c_i32p, c_i32p, c_i32p, c_i32p, _I, _I, _I, c_vp, c_vp,
                                            c_vp, _I]),
    "exabm4d_components_scratch_bytes": (_SZ, [c_i32p, _I]),
    "exabm4d_component_seeds_u16_dev": (_I, [_CTX, c_vp, c_i32p, c_i32p, c_i32p, c_i32p, c_i32p, c_i32p, c_i32p, _I, _I,
                                             _I, c_vp, c_vp, c_vp, c_vp, _SZ, c_vp, _I]),
    "exabm4d_label_components_dev": (_I, [_CTX, c_vp, _I, c_i32p, _I, _I, _I, c_vp, c_vp, c_vp, c_vp, _SZ, c_vp]),
    "exabm4d_segment_collect_dev": (_I, [_CTX, c_vp, c_i32p, c_i32p, c_i32p, c_i32p, c_i32p, c_vp, c_vp, _SZ, c_vp, _SZ,
                                         c_vp, _SZ, c_vp]),
    "exabm4d_segment_relabel_dev": (_I, [_CTX, c_vp, c_i32p, c_i32p, c_i32p, c_i32p, c_i32p, c_vp, c_vp, _SZ, _I, c_vp,
                                         c_vp]),
    "exabm4d_nonzero_u8_dev": (_I, [_CTX, c_vp, _SZ, c_vp]),
    "exabm4d_downsample_box_u16_dev": (_I, [_CTX, c_vp, c_i32p, c_i32p, c_i32p, c_i32p, c_i32p, c_i32p, _I, _I, c_vp]),
    "exabm4d_downsample_box_labels_dev": (_I, [_CTX, c_vp, _I, c_i32p, c_i32p, c_i32p, c_i32p, c_i32p, c_i32p, _I, _I,
                                               c_vp]),
    "exabm4d_foreground_masks_dev": (_I, [_CTX, c_vp, _I, _I, _I, _I, _I, _F, _I, c_vp, c_vp]),
    "exabm4d_binary_dilate_dev": (_I, [_CTX, c_vp, _I, _I, _I, _I, _I, c_vp]),
    "exabm4d_gaussian_filter3d_dev": (_I, [_CTX, c_vp, _I, _I, _I, _I, _I, c_vp, _I, c_vp]),
    "exabm4d_label_set_dev": (_I, [_CTX, c_vp, _I, _I, _I, _I, _I, c_vp, c_vp, c_vp, c_vp]),
    "exabm4d_segment_stats_dev": (_I, [_CTX, c_vp, _I, c_vp, _I, c_vp, _I, _I, _I, _I, _I, c_vp, c_vp, _I,
                                       c_vp]),
    "exabm4d_foreground_counts_dev": (_I, [_CTX, c_vp, _I, _I, _I, _I, _I, _F, _I, c_vp, c_vp]),
    "exabm4d_annotation_masks_dev": (_I, [_CTX, c_vp, _I, _I, c_vp, _SZ, c_vp, _I, _I, _I, _I, _I, c_vp]),
    "exabm4d_evaluate_batch_dev": (_I, [_CTX, c_vp, _I, c_vp, _I, c_vp, _I, c_vp, _I, _SZ, ctypes.c_double, c_u32p,
                                        c_vp]),
    "exabm4d_gather_boxes_dev": (_I, [_CTX, c_vp, _SZ, c_vp, _I, c_vp, _I, c_vp, _I, _I, _I, _I, _I, _F,
                                      ctypes.c_double, c_vp]),
    "exabm4d_scatter_boxes_dev": (_I, [_CTX, c_vp, _SZ, _I, c_vp, _I, c_vp, _SZ, _I, c_vp, _I, c_vp, _I, _F]),
    "exabm4d_label_encode_bound": (_SZ, [_I, _I, _I, _I, _I, _I, _I]),
    "exabm4d_label_encode_dev": (_I, [_CTX, c_vp, _I, _I, _I, _I, _I, _I, _I, c_vp, _SZ, c_vp, c_vp, c_vp]),
    "exabm4d_label_decode_dev": (_I, [_CTX, c_vp, _SZ, c_vp, _I, _I, _I, _I, _I, _I, _I, c_vp]),
    "exabm4d_label_gather_boxes_dev": (_I, [_CTX, c_vp, _SZ, _I, c_vp, _I, c_vp, _I, c_vp, _I, _I, _I, _I, c_i32p,
                                            c_i32p, c_vp]),
}

# ``exabm4d_box_src`` (include/exabm4d.h): a decoded chunk in the pool ``Context.gather_boxes`` reads
BOX_SRC = np.dtype([("base", "<u8"), ("stride_y", "<u8"), ("stride_z", "<u8"), ("z0", "<i4"), ("y0", "<i4"),
                    ("x0", "<i4"), ("ez", "<i4"), ("ey", "<i4"), ("ex", "<i4")])

# ``exabm4d_label_src`` (include/exabm4d.h): a coded chunk in the container ``Context.label_gather_boxes`` reads
LABEL_SRC = np.dtype([("offset", "<u8"), ("bytes", "<u8"), ("z0", "<i4"), ("y0", "<i4"), ("x0", "<i4"),
                      ("ez", "<i4"), ("ey", "<i4"), ("ex", "<i4")])

_lib = None
_lib_lock = threading.Lock()


class NativeError(RuntimeError):
    """libexabm4d.so is missing, or a call into it failed."""


def library_path():
    for p in _LIB_CANDIDATES:
        if p and os.path.exists(p):
            return p
    raise NativeError(
        "libexabm4d.so not found (looked in %s). Build it with `make -C "
        "aind-exaspim-image-compression_amd/csrc` or __graft_entry__.build(); there is no "
        "CPU fallback for the HIP hot path." % [p for p in _LIB_CANDIDATES if p])


def _mapped_hip_runtimes():
    """Real paths of every libamdhip64 image mapped into this process (/proc/self/maps)."""
    seen = set()
    try:
        with open("/proc/self/maps") as f:
            for line in f:
                if "libamdhip64" in line:
                    seen.add(os.path.realpath(line.split(None, 5)[-1].strip()))
    except OSError:
        pass
    return seen


def _adopt_torch_hip_runtime():
    """PyTorch-ROCm wheels carry their own libamdhip64.so (same SONAME as /opt/rocm's).  Two copies
    in one process leave the one loaded second without devices, whichever side it belongs to: the
    reference's callers import ``bm4d`` first and torch later (data_handling.py:12, inference.py),
    so the order is not ours to choose.  Rule: when a torch with a bundled HIP runtime is
    installed, ITS runtime is the process's runtime -- it is mapped here (dlopen only: no HIP
    call, no device initialisation, torch itself is not imported) before libexabm4d.so, whose
    DT_NEEDED ``libamdhip64.so.7`` then binds to the image already loaded under that SONAME.
    ``EXABM4D_SYSTEM_HIP=1`` keeps /opt/rocm's runtime (for processes that never load torch)."""
    if os.environ.get("EXABM4D_SYSTEM_HIP") == "1":
        return None
    if _mapped_hip_runtimes():
        return None                       # somebody (torch, rocprofv3, the caller) already chose
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return None
    path = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if not os.path.exists(path):
        return None
    ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
    return path


def lib():
    """Load the shared library (no GPU needed for this) and bind every symbol."""
    global _lib
    with _lib_lock:
        if _lib is None:
            _adopt_torch_hip_runtime()
            L = ctypes.CDLL(library_path())
            mapped = _mapped_hip_runtimes()
            if len(mapped) > 1:
                raise NativeError(
                    "two HIP runtimes are mapped into this process (%s): the one loaded second has "
                    "no devices.  Load libexabm4d.so and torch against the same libamdhip64 "
                    "(see INTEGRATION.md 1d)." % ", ".join(sorted(mapped)))
            for name, (res, args) in SIGNATURES.items():
                fn = getattr(L, name)  # AttributeError if the .so lacks a declared symbol
                fn.restype = res
                fn.argtypes = args
            _lib = L
    return _lib


def components_scratch_bytes(win_dims, connectivity=26):
    """Bytes of scratch ``Context.component_seeds_u16`` takes for a window of ``win_dims`` (z, y, x); ValueError for
    bad arguments or 2^31 voxels and more.  No GPU needed."""
    dims = (ctypes.c_int32 * 3)(*(int(v) for v in win_dims))
    n = int(lib().exabm4d_components_scratch_bytes(dims, int(connectivity)))
    if n == 0:
        raise ValueError("components_scratch_bytes: dims >= 1 with fewer than 2^31 voxels, connectivity 6 or 26")
    return n


def components_region(vol_dims, box_origin, box_dims, min_voxels):
    """(origin, dims) of the region ``Context.component_seeds_u16`` labels: the box grown by ``min_voxels - 1`` voxels
    per axis and cut at the volume's faces (all z, y, x)."""
    grow = max(0, int(min_voxels) - 1)
    lo = tuple(max(0, int(b) - grow) for b in box_origin)
    hi = tuple(min(int(n), int(b) + int(d) + grow) for n, b, d in zip(vol_dims, box_origin, box_dims))
    return lo, tuple(h - l for h, l in zip(hi, lo))


def segment_record_capacities(win_dims, brick_origin, brick_dims):
    """(halo, face): the most halo and face records ``Context.segment_collect`` can write -- the voxels of the window
    outside the brick, and the voxels of the brick on a low face whose brick origin on that axis is > 0."""
    win = int(np.prod([int(v) for v in win_dims], dtype=np.int64))
    brick = int(np.prod([int(v) for v in brick_dims], dtype=np.int64))
    inner = int(np.prod([int(d) - (1 if int(o) > 0 else 0) for o, d in zip(brick_origin, brick_dims)], dtype=np.int64))
    return win - brick, brick - inner


def default_params(**overrides):
    p = Params()
    rc = lib().exabm4d_default_params(ctypes.byref(p))
    if rc:
        raise NativeError("exabm4d_default_params failed")
    for k, v in overrides.items():
        if not hasattr(p, k):
            raise ValueError(f"unknown BM4D parameter: {k}")
        setattr(p, k, v)
    return p


def _ptr(obj):
    """Device pointer of a DeviceBuffer, a torch tensor, an int, or None."""
    if obj is None:
        return None
    if isinstance(obj, DeviceBuffer):
        return obj.ptr
    if isinstance(obj, int):
        return obj
    if hasattr(obj, "data_ptr"):
        return int(obj.data_ptr())
    raise TypeError(f"cannot take a device pointer from {type(obj)!r}")


class DeviceBuffer:
    """A hipMalloc'd region owned through ``exabm4d_malloc`` (for hosts without torch)."""

    def __init__(self, ctx, nbytes):
        self.ctx = ctx
        self.nbytes = int(nbytes)
        p = c_vp()
        ctx._check(lib().exabm4d_malloc(ctx.handle, self.nbytes, ctypes.byref(p)))
        self.ptr = p.value

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        if arr.nbytes > self.nbytes:
            raise ValueError("host array larger than device buffer")
        self.ctx._check(lib().exabm4d_memcpy_h2d(self.ctx.handle, self.ptr, arr.ctypes.data,
                                                 arr.nbytes))
        return self

    def download(self, shape, dtype):
        out = np.empty(shape, dtype=dtype)
        if out.nbytes > self.nbytes:
            raise ValueError("requested more bytes than the device buffer holds")
        self.ctx._check(lib().exabm4d_memcpy_d2h(self.ctx.handle, out.ctypes.data, self.ptr,
                                                 out.nbytes))
        return out

    def zero(self):
        return self.fill(0)

    def fill(self, byte):
        self.ctx._check(lib().exabm4d_memset(self.ctx.handle, self.ptr, int(byte), self.nbytes))
        return self

    def free(self):
        if self.ptr:
            lib().exabm4d_free(self.ctx.handle, self.ptr)
            self.ptr = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Context:
    """One ``exabm4d_ctx`` -- bound to the process that created it and one device."""

    def __init__(self, device=0):
        self.pid = os.getpid()
        self.device = int(device)
        h = c_vp()
        rc = lib().exabm4d_create(self.device, ctypes.byref(h))
        if rc:
            raise NativeError("exabm4d_create(device=%d) failed: %s" % (
                self.device, lib().exabm4d_last_error(None).decode()))
        self.handle = h

    def _check(self, rc):
        if rc:
            msg = lib().exabm4d_last_error(self.handle).decode()
            if rc in (-1, -2):
                raise ValueError(msg)
            raise NativeError(msg)

    # -- memory ----------------------------------------------------------------------------
    def alloc(self, nbytes):
        return DeviceBuffer(self, nbytes)

    def to_device(self, arr):
        arr = np.ascontiguousarray(arr)
        return DeviceBuffer(self, arr.nbytes).upload(arr)

    def sync(self):
        self._check(lib().exabm4d_sync(self.handle))

    def set_option(self, name, value):
        self._check(lib().exabm4d_set_option(self.handle, name.encode(), int(value)))

    PHASES = ("counts_from_u16", "zero_acc_1", "blockmatch_ht", "stage_ht", "normalize_basic",
              "zero_acc_2", "blockmatch_wie", "stage_wie", "normalize_out")

    def profile_read(self):
        """Per-phase milliseconds of the last denoise call (needs set_option('profile', 1))."""
        ms = (ctypes.c_float * len(self.PHASES))()
        n = lib().exabm4d_profile_read(self.handle, ms, len(self.PHASES))
        if n < 0:
            self._check(n)
        return {name: float(ms[i]) for i, name in enumerate(self.PHASES[:n])}

    def set_stream(self, hip_stream):
        """Enqueue on an existing HIP stream handle; 0 / None is the HIP null stream (which is
        what torch's default stream is)."""
        self._check(lib().exabm4d_set_stream(self.handle, hip_stream or None))

    def reset_stream(self):
        """Back to the context's private non-blocking stream."""
        self._check(lib().exabm4d_reset_stream(self.handle))

    # -- HIP events on the context's stream -------------------------------------------------
    def event(self):
        e = c_vp()
        self._check(lib().exabm4d_event_create(self.handle, ctypes.byref(e)))
        return e

    def record(self, ev):
        self._check(lib().exabm4d_event_record(self.handle, ev))

    def elapsed_ms(self, a, b):
        ms = ctypes.c_float()
        self._check(lib().exabm4d_event_elapsed_ms(self.handle, a, b, ctypes.byref(ms)))
        return float(ms.value)

    # -- BM4D ---------------------------------------------------------------------------------
    def blockmatch(self, vol, shape, sigma, c_match, keys, params=None, batch=1):
        p = params or default_params()
        nz, ny, nx = shape
        self._check(lib().exabm4d_blockmatch_dev(self.handle, _ptr(vol), nz, ny, nx, batch,
                                                 float(sigma), float(c_match), ctypes.byref(p),
                                                 _ptr(keys)))

    def blockmatch_u16(self, vol, shape, sigma, c_match, keys, params=None, batch=1):
        p = params or default_params()
        nz, ny, nx = shape
        self._check(lib().exabm4d_blockmatch_u16_dev(self.handle, _ptr(vol), nz, ny, nx, batch,
                                                     float(sigma), float(c_match), ctypes.byref(p),
                                                     _ptr(keys)))

    def stage(self, noisy, basic, keys, shape, sigma, num, den, params=None, batch=1, data_exp=None):
        """One collaborative-filtering stage; ``num`` / ``den`` (fp32) are WRITTEN.  ``data_exp``: E of
        the numerator's fixed-point unit; None = per volume from ``noisy`` (the fp32
        pipelines' rule), DATA_EXP_U16 = what the uint16 pipelines use."""
        p = params or default_params()
        nz, ny, nx = shape
        self._check(lib().exabm4d_stage_dev(self.handle, _ptr(noisy), _ptr(basic), _ptr(keys), nz,
                                            ny, nx, batch, float(sigma), ctypes.byref(p),
                                            DATA_EXP_AUTO if data_exp is None else int(data_exp),
                                            _ptr(num), _ptr(den)))

    def normalize(self, num, den, out, n, clip=None):
        lo, hi = (1.0, 0.0) if clip is None else clip
        self._check(lib().exabm4d_normalize_dev(self.handle, _ptr(num), _ptr(den), _ptr(out), n,
                                                float(lo), float(hi)))

    def counts_from_u16(self, src, dst, n, offset):
        """dst (fp32) = (float)src - offset: read_counts, data_handling.py:337-354"""
        self._check(lib().exabm4d_counts_from_u16_dev(self.handle, _ptr(src), _ptr(dst), n, offset))

    def round_counts(self, src, dst, n, offset):
        """dst (fp32) = (float)rint(clamp(src + offset, 0, 65535)) - offset: what stage 2 of the uint16
        pipelines matches on"""
        self._check(lib().exabm4d_round_counts_f32_dev(self.handle, _ptr(src), _ptr(dst), n, offset))

    def normalize_u16(self, num, den, out, n, offset):
        """out (uint16) = rint(clamp(num / den + offset, 0, 65535))"""
        self._check(lib().exabm4d_normalize_u16_dev(self.handle, _ptr(num), _ptr(den), _ptr(out), n,
                                                    offset))

    def denoise_f32(self, src, dst, shape, sigma, params=None, stages=2, clip=None, batch=1):
        p = params or default_params()
        nz, ny, nx = shape
        lo, hi = (1.0, 0.0) if clip is None else clip
        self._check(lib().exabm4d_denoise_f32_dev(self.handle, _ptr(src), _ptr(dst), nz, ny, nx,
                                                  batch, float(sigma), ctypes.byref(p),
                                                  int(stages), float(lo), float(hi)))

    def denoise_u16(self, src, dst, shape, sigma, offset, params=None, stages=2, batch=1):
        p = params or default_params()
        nz, ny, nx = shape
        self._check(lib().exabm4d_denoise_u16_dev(self.handle, _ptr(src), _ptr(dst), nz, ny, nx,
                                                  batch, float(sigma), float(offset),
                                                  ctypes.byref(p), int(stages)))

    def denoise_chunked_u16(self, src, dst, shape, sigma, offset, chunk=256, halo=8, core=None,
                            params=None, stages=2):
        """Chunk-local mode: ``src`` [nz,ny,nx] uint16 on the device, ``dst`` receives the core
        planes ``core = (zc0, zc1)`` (default: all planes)."""
        p = params or default_params()
        nz, ny, nx = shape
        zc0, zc1 = (0, nz) if core is None else core
        self._check(lib().exabm4d_denoise_chunked_u16_dev(
            self.handle, _ptr(src), _ptr(dst), nz, ny, nx, int(zc0), int(zc1), int(chunk),
            int(halo), float(sigma), float(offset), ctypes.byref(p), int(stages)))

    def denoise_chunked_u16_host(self, src, dst, sigma, offset, chunk=256, halo=8, params=None, stages=2):
        """Host uint16 arrays (numpy / memmap, C-contiguous, same 3-D shape) streamed through the device
        one layer of chunks at a time; returns when ``dst`` is complete."""
        p = params or default_params()
        check_host_volume_pair(src, dst)
        nz, ny, nx = src.shape
        self._check(lib().exabm4d_denoise_chunked_u16_host(
            self.handle, src.ctypes.data, dst.ctypes.data, nz, ny, nx, int(chunk), int(halo), float(sigma),
            float(offset), ctypes.byref(p), int(stages)))

    # -- BM4D under Poisson-Gaussian noise; ``noise``: a PgNoise (pg_noise(...)) ---------------
    def denoise_pg_u16(self, src, dst, shape, noise, params=None, stages=2, batch=1):
        """uint16 counts -> stabilised -> BM4D at sigma 1 -> inverse -> uint16, device pointers."""
        p = params or default_params()
        nz, ny, nx = shape
        self._check(lib().exabm4d_denoise_pg_u16_dev(self.handle, _ptr(src), _ptr(dst), nz, ny, nx, int(batch),
                                                     ctypes.byref(noise), ctypes.byref(p), int(stages)))

    def denoise_pg_chunked_u16(self, src, dst, shape, noise, chunk=256, halo=8, core=None, params=None, stages=2):
        """``denoise_chunked_u16`` with the stabilised pipeline on every padded chunk."""
        p = params or default_params()
        nz, ny, nx = shape
        zc0, zc1 = (0, nz) if core is None else core
        self._check(lib().exabm4d_denoise_pg_chunked_u16_dev(
            self.handle, _ptr(src), _ptr(dst), nz, ny, nx, int(zc0), int(zc1), int(chunk), int(halo),
            ctypes.byref(noise), ctypes.byref(p), int(stages)))

    def denoise_pg_chunked_u16_host(self, src, dst, noise, chunk=256, halo=8, params=None, stages=2):
        """``denoise_chunked_u16_host`` with the stabilised pipeline on every padded chunk."""
        p = params or default_params()
        check_host_volume_pair(src, dst)
        nz, ny, nx = src.shape
        self._check(lib().exabm4d_denoise_pg_chunked_u16_host(
            self.handle, src.ctypes.data, dst.ctypes.data, nz, ny, nx, int(chunk), int(halo), ctypes.byref(noise),
            ctypes.byref(p), int(stages)))

    def gat_forward_u16(self, noise, src, dst, n):
        """dst (fp32) = the un-normalised generalised Anscombe transform of the uint16 counts src."""
        self._check(lib().exabm4d_gat_forward_u16_dev(self.handle, ctypes.byref(noise), _ptr(src), _ptr(dst), int(n)))

    def gat_inverse_u16(self, noise, src, dst, n):
        """dst (uint16) = rint(clamp(noise.inverse of the stabilised values src, 0, 65535))"""
        self._check(lib().exabm4d_gat_inverse_u16_dev(self.handle, ctypes.byref(noise), _ptr(src), _ptr(dst), int(n)))

    def denoise_f32_host(self, arr, sigma, params=None, stages=2, clip=None):
        """numpy fp32 [N,]Z,Y,X in -> new numpy array out (H2D, kernels, D2H, sync)."""
        p = params or default_params()
        arr = np.ascontiguousarray(arr, dtype=np.float32)
        if arr.ndim == 3:
            batch, (nz, ny, nx) = 1, arr.shape
        elif arr.ndim == 4:
            batch, (nz, ny, nx) = arr.shape[0], arr.shape[1:]
        else:
            raise ValueError("expected a 3-D volume or a 4-D batch of volumes")
        out = np.empty_like(arr)
        lo, hi = (1.0, 0.0) if clip is None else clip
        self._check(lib().exabm4d_denoise_f32_host(self.handle, arr.ctypes.data, out.ctypes.data,
                                                   nz, ny, nx, batch, float(sigma),
                                                   ctypes.byref(p), int(stages), float(lo),
                                                   float(hi)))
        return out

    # -- BM4DNet stage ---------------------------------------------------------------------------
    def groupnorm_lrelu_ndhwc(self, stream, x, y, batch, spatial, channels, groups, gamma, beta, eps, slope,
                              workspace, workspace_bytes, conv_bias=None, dtype=DTYPE_F32):
        """GroupNorm + LeakyReLU on an NDHWC tensor of ``dtype`` (a DTYPE_* code; x, y, gamma, beta, workspace:
        device pointers or objects with ``data_ptr()``; gamma, beta and conv_bias fp32 for every dtype;
        ``stream``: the HIP stream handle to run on).  ValueError where the fused kernels do not apply (see the
        header)."""
        self._check(lib().exabm4d_groupnorm_lrelu_ndhwc_dt_dev(
            self.handle, int(stream), int(dtype), _ptr(x), _ptr(y), int(batch), int(spatial), int(channels),
            int(groups), _ptr(gamma) if gamma is not None else None, _ptr(beta) if beta is not None else None,
            float(eps), float(slope), _ptr(workspace), int(workspace_bytes),
            _ptr(conv_bias) if conv_bias is not None else None))

    def maxpool2_ndhwc(self, stream, x, y, batch, d, h, w, channels, dtype=DTYPE_F32):
        self._check(lib().exabm4d_maxpool2_ndhwc_dt_dev(self.handle, int(stream), int(dtype), _ptr(x), _ptr(y),
                                                        int(batch), int(d), int(h), int(w), int(channels)))

    def upsample2_trilinear_ndhwc(self, stream, x, y, batch, d, h, w, channels, dtype=DTYPE_F32):
        self._check(lib().exabm4d_upsample2_trilinear_ndhwc_dt_dev(self.handle, int(stream), int(dtype), _ptr(x),
                                                                   _ptr(y), int(batch), int(d), int(h), int(w),
                                                                   int(channels)))

    # -- BM4DNet training (NDHWC tensors of ``dtype``, a DTYPE_* code, fp32 by default; see the header) --------
    def groupnorm_lrelu_ndhwc_train(self, stream, x, y, batch, spatial, channels, groups, gamma, beta, eps, slope,
                                    workspace, workspace_bytes, mean_rstd, dtype=DTYPE_F32):
        """The forward that also writes ``mean_rstd[batch][groups][2]`` (fp32 for every dtype) for the backward."""
        self._check(lib().exabm4d_groupnorm_lrelu_ndhwc_train_dt_dev(
            self.handle, int(stream), int(dtype), _ptr(x), _ptr(y), int(batch), int(spatial), int(channels),
            int(groups), _ptr(gamma), _ptr(beta), float(eps), float(slope), _ptr(workspace), int(workspace_bytes),
            _ptr(mean_rstd)))

    def groupnorm_lrelu_bwd_ndhwc(self, stream, x, y, dy, dx, batch, spatial, channels, groups, gamma, mean_rstd,
                                  slope, dgamma, dbeta, workspace, workspace_bytes, dtype=DTYPE_F32):
        """x, y, dy, dx in ``dtype``; gamma, mean_rstd, dgamma, dbeta fp32."""
        self._check(lib().exabm4d_groupnorm_lrelu_bwd_ndhwc_dt_dev(
            self.handle, int(stream), int(dtype), _ptr(x), _ptr(y), _ptr(dy), _ptr(dx), int(batch), int(spatial),
            int(channels), int(groups), _ptr(gamma), _ptr(mean_rstd), float(slope), _ptr(dgamma), _ptr(dbeta),
            _ptr(workspace), int(workspace_bytes)))

    def maxpool2_bwd_ndhwc(self, stream, x, dy, dx, batch, d, h, w, channels, dtype=DTYPE_F32):
        """``d, h, w``: the extents of the forward's input ``x`` (and of ``dx``)."""
        self._check(lib().exabm4d_maxpool2_bwd_ndhwc_dt_dev(self.handle, int(stream), int(dtype), _ptr(x), _ptr(dy),
                                                            _ptr(dx), int(batch), int(d), int(h), int(w),
                                                            int(channels)))

    def upsample2_trilinear_bwd_ndhwc(self, stream, dy, dx, batch, d, h, w, channels, dtype=DTYPE_F32):
        """``d, h, w``: the extents of the forward's input (of ``dx``); ``dy`` has twice each."""
        self._check(lib().exabm4d_upsample2_trilinear_bwd_ndhwc_dt_dev(self.handle, int(stream), int(dtype),
                                                                       _ptr(dy), _ptr(dx), int(batch), int(d), int(h),
                                                                       int(w), int(channels)))

    def charbonnier_loss(self, stream, pred, target, mask, mask_bytes, n, fg_weight, eps, workspace,
                         workspace_bytes, loss):
        self._check(lib().exabm4d_charbonnier_loss_dev(
            self.handle, int(stream), _ptr(pred), _ptr(target), _ptr(mask), int(mask_bytes), int(n),
            float(fg_weight), float(eps), _ptr(workspace), int(workspace_bytes), _ptr(loss)))

    def charbonnier_loss_bwd(self, stream, pred, target, mask, mask_bytes, n, fg_weight, eps, grad_loss, dpred):
        self._check(lib().exabm4d_charbonnier_loss_bwd_dev(
            self.handle, int(stream), _ptr(pred), _ptr(target), _ptr(mask), int(mask_bytes), int(n),
            float(fg_weight), float(eps), _ptr(grad_loss), _ptr(dpred)))

    def host_register(self, addr, nbytes):
        """Page-lock caller memory that host entry points copy from / to repeatedly (see the header)."""
        self._check(lib().exabm4d_host_register(self.handle, int(addr), int(nbytes)))

    def host_unregister(self, addr):
        self._check(lib().exabm4d_host_unregister(self.handle, int(addr)))

    def denoise_f32_host_v(self, in_addrs, out_addrs, shape, sigma, params=None, stages=2, clip=None):
        """A batch of fp32 volumes of ``shape`` that lie anywhere in host memory: ``in_addrs[i]`` /
        ``out_addrs[i]`` are the addresses of volume i (they may be equal: in place).  The caller keeps the
        memory alive and writable; nothing is allocated or copied on the host side."""
        if len(in_addrs) != len(out_addrs) or not len(in_addrs):
            raise ValueError("one input and one output address per volume")
        p = params or default_params()
        nz, ny, nx = (int(s) for s in shape)
        n = len(in_addrs)
        ins = (ctypes.c_void_p * n)(*[int(a) for a in in_addrs])
        outs = (ctypes.c_void_p * n)(*[int(a) for a in out_addrs])
        lo, hi = (1.0, 0.0) if clip is None else clip
        self._check(lib().exabm4d_denoise_f32_host_v(self.handle, ctypes.cast(ins, c_vp), ctypes.cast(outs, c_vp),
                                                     nz, ny, nx, n, float(sigma), ctypes.byref(p), int(stages),
                                                     float(lo), float(hi)))

    # -- transforms ---------------------------------------------------------------------------
    def transform_forward(self, tf, src, dst, n, src_is_u16):
        fn = (lib().exabm4d_transform_forward_u16_dev if src_is_u16
              else lib().exabm4d_transform_forward_f32_dev)
        self._check(fn(self.handle, ctypes.byref(tf), _ptr(src), _ptr(dst), n))

    def transform_inverse(self, tf, src, dst, n, quantise=True):
        fn = (lib().exabm4d_transform_inverse_u16_dev if quantise
              else lib().exabm4d_transform_inverse_f32_dev)
        self._check(fn(self.handle, ctypes.byref(tf), _ptr(src), _ptr(dst), n))

    # -- tiling -------------------------------------------------------------------------------
    def tile_gather(self, vol, shape, starts, patch, out):
        starts = np.ascontiguousarray(starts, dtype=np.int32).reshape(-1, 3)
        nz, ny, nx = shape
        self._check(lib().exabm4d_tile_gather_dev(
            self.handle, _ptr(vol), nz, ny, nx, starts.ctypes.data_as(c_i32p), len(starts),
            int(patch), _ptr(out)))

    def tile_accumulate(self, preds, starts, patch, trim, acc, wgt, shape):
        starts = np.ascontiguousarray(starts, dtype=np.int32).reshape(-1, 3)
        nz, ny, nx = shape
        self._check(lib().exabm4d_tile_accumulate_dev(
            self.handle, _ptr(preds), starts.ctypes.data_as(c_i32p), len(starts), int(patch),
            int(trim), _ptr(acc), _ptr(wgt), nz, ny, nx))

    def tile_finalize(self, tf, acc, wgt, out, n):
        self._check(lib().exabm4d_tile_finalize_u16_dev(self.handle, ctypes.byref(tf), _ptr(acc),
                                                        _ptr(wgt), _ptr(out), n))

    def tile_gather_u16(self, tf, win, win_origin, win_dims, vol_dims, grid, k0, nb, out):
        """Patches ``[k0, k0 + nb)`` of ``grid`` (a ``PatchGrid``) from the uint16 window ``win`` -> ``out``
        (nb, patch, patch, patch) fp32: transformed inside the volume, 0.0 beyond it.  ValueError for a window that
        does not hold the grid's patches or a batch past the grid."""
        tri = [(ctypes.c_int32 * 3)(*(int(v) for v in t)) for t in (win_origin, win_dims, vol_dims)]
        self._check(lib().exabm4d_tile_gather_u16_dev(self.handle, _ptr(win), tri[0], tri[1], tri[2],
                                                      ctypes.byref(tf), ctypes.byref(grid), int(k0), int(nb),
                                                      _ptr(out)))

    def tile_stitch_u16(self, tf, preds, n_patches, grid, trim, box_origin, box_dims, vol_dims, out):
        """All predictions of ``grid`` (``preds``: (n_patches, patch, patch, patch) fp32, raster order) -> the
        uint16 counts of the box, dense in ``out``."""
        tri = [(ctypes.c_int32 * 3)(*(int(v) for v in t)) for t in (box_origin, box_dims, vol_dims)]
        self._check(lib().exabm4d_tile_stitch_u16_dev(self.handle, _ptr(preds), int(n_patches), ctypes.byref(grid),
                                                      int(trim), tri[0], tri[1], tri[2], ctypes.byref(tf),
                                                      _ptr(out)))

    def chunk_byte_histograms(self, vol, shape, chunk, hist):
        nz, ny, nx = shape
        self._check(lib().exabm4d_chunk_byte_histograms_dev(self.handle, _ptr(vol), nz, ny, nx,
                                                            int(chunk[0]), int(chunk[1]),
                                                            int(chunk[2]), _ptr(hist)))

    # -- transform quantiser (row f-1) ---------------------------------------------------------
    def dctq_forward(self, vol, shape, q, idx):
        nz, ny, nx = shape
        self._check(lib().exabm4d_dctq_forward_dev(self.handle, _ptr(vol), nz, ny, nx, float(q),
                                                   _ptr(idx)))

    def dctq_inverse(self, idx, shape, q, vol):
        nz, ny, nx = shape
        self._check(lib().exabm4d_dctq_inverse_dev(self.handle, _ptr(idx), nz, ny, nx, float(q),
                                                   _ptr(vol)))

    # -- chunk entropy coder (row f-1) ------------------------------------------------------------
    def codec_encode(self, vol, typesize, shape, chunk, out=None, out_capacity=0, offsets=None,
                     sizes=None, totals=True, version=0):
        """Code every chunk of a device volume.  -> (sum of stream lengths, container bytes) when
        `totals` (synchronises), else None.  ``version``: EXAC format of THIS call (1 | 2; 0 = the
        context's "codec_version" option)."""
        nz, ny, nx = shape
        tot = np.zeros(2, dtype=np.uint64)
        self._check(lib().exabm4d_codec_encode_dev(
            self.handle, _ptr(vol), int(typesize), int(version), nz, ny, nx, int(chunk[0]), int(chunk[1]),
            int(chunk[2]), _ptr(out), int(out_capacity), _ptr(offsets), _ptr(sizes),
            tot.ctypes.data_as(c_vp) if totals else None))
        return (int(tot[0]), int(tot[1])) if totals else None

    def codec_decode(self, data, nbytes, offsets, typesize, shape, chunk, vol):
        """``data``: ``nbytes`` bytes of chunk streams on the device; the decoder never reads
        outside them, whatever ``offsets`` says (malformed containers raise ValueError)."""
        nz, ny, nx = shape
        self._check(lib().exabm4d_codec_decode_dev(
            self.handle, _ptr(data), int(nbytes), _ptr(offsets), int(typesize), nz, ny, nx,
            int(chunk[0]), int(chunk[1]), int(chunk[2]), _ptr(vol)))

    # -- error-bounded lossy chunk codec ----------------------------------------
    def dctq_ladder_errors(self, vol, shape, chunk, err):
        """err (device, uint32 [nchunks][29]) <- the largest reconstruction error of every chunk at every
        ladder step.  Asynchronous."""
        nz, ny, nx = shape
        self._check(lib().exabm4d_dctq_ladder_errors_dev(self.handle, _ptr(vol), nz, ny, nx, int(chunk[0]),
                                                         int(chunk[1]), int(chunk[2]), _ptr(err)))

    def bounded_encode(self, vol, shape, chunk, max_error, out=None, out_capacity=0, offsets=None, sizes=None,
                       totals=True):
        """Code every chunk of a device uint16 volume under the bound.  -> (sum of stream lengths, container
        bytes) when `totals` (synchronises), else None."""
        nz, ny, nx = shape
        tot = np.zeros(2, dtype=np.uint64)
        self._check(lib().exabm4d_bounded_encode_dev(
            self.handle, _ptr(vol), nz, ny, nx, int(chunk[0]), int(chunk[1]), int(chunk[2]), int(max_error),
            _ptr(out), int(out_capacity), _ptr(offsets), _ptr(sizes), tot.ctypes.data_as(c_vp) if totals else None))
        return (int(tot[0]), int(tot[1])) if totals else None

    def bounded_decode(self, data, nbytes, offsets, shape, chunk, vol):
        """``data``: ``nbytes`` bytes of bounded chunk streams on the device -> uint16 ``vol``; malformed
        containers raise ValueError without a read outside them."""
        nz, ny, nx = shape
        self._check(lib().exabm4d_bounded_decode_dev(
            self.handle, _ptr(data), int(nbytes), _ptr(offsets), nz, ny, nx, int(chunk[0]), int(chunk[1]),
            int(chunk[2]), _ptr(vol)))

    # -- error-bounded codec, a step per 8^3 block and a per-voxel bound ------------
    def block_bounded_steps(self, vol, shape, chunk, max_error, fg_max_error, plane, mask=None, table=None):
        """plane (device, uint8 [nchunks][nb rounded up to 16]) <- the step plane of every chunk (0xFE verbatim, 0xFF
        outside the volume), whatever mode the chunk would be stored in.  ``table`` (device, 65536 uint16, or None):
        the bound table of DESIGN.md 3.10d, through the ``_tab`` entry.  Asynchronous."""
        nz, ny, nx = shape
        args = (self.handle, _ptr(vol), _ptr(mask), nz, ny, nx, int(chunk[0]), int(chunk[1]), int(chunk[2]),
                int(max_error), int(fg_max_error), _ptr(plane))
        if table is None:
            self._check(lib().exabm4d_block_bounded_steps_dev(*args))
        else:
            self._check(lib().exabm4d_block_bounded_steps_tab_dev(*args, _ptr(table)))

    def block_bounded_encode(self, vol, shape, chunk, max_error, fg_max_error, mask=None, out=None, out_capacity=0,
                             offsets=None, sizes=None, totals=True, table=None):
        """``bounded_encode`` with a step per block; ``mask`` (device uint8 of the volume's shape, or None) marks
        the voxels whose bound is ``fg_max_error``, and ``table`` (device, 65536 uint16, or None) caps the bound of
        a voxel by ``table[its value]``, through the ``_tab`` entry."""
        nz, ny, nx = shape
        tot = np.zeros(2, dtype=np.uint64)
        args = (self.handle, _ptr(vol), _ptr(mask), nz, ny, nx, int(chunk[0]), int(chunk[1]), int(chunk[2]),
                int(max_error), int(fg_max_error), _ptr(out), int(out_capacity), _ptr(offsets), _ptr(sizes),
                tot.ctypes.data_as(c_vp) if totals else None)
        if table is None:
            self._check(lib().exabm4d_block_bounded_encode_dev(*args))
        else:
            self._check(lib().exabm4d_block_bounded_encode_tab_dev(*args, _ptr(table)))
        return (int(tot[0]), int(tot[1])) if totals else None

    def block_bounded_decode(self, data, nbytes, offsets, shape, chunk, vol):
        """``data``: ``nbytes`` bytes of block-bounded chunk streams on the device -> uint16 ``vol``; malformed
        containers raise ValueError without a read outside them."""
        nz, ny, nx = shape
        self._check(lib().exabm4d_block_bounded_decode_dev(
            self.handle, _ptr(data), int(nbytes), _ptr(offsets), nz, ny, nx, int(chunk[0]), int(chunk[1]),
            int(chunk[2]), _ptr(vol)))

    # -- background offset + quality metrics (row f-4); inputs on device, scalars to the host ----
    DTYPES = {np.dtype(np.uint16): 0, np.dtype(np.float32): 1, np.dtype(np.float64): 2}

    def i32_symbol_histogram(self, idx, n):
        hist = np.empty(65536, dtype=np.uint64)
        self._check(lib().exabm4d_i32_symbol_histogram_dev(self.handle, _ptr(idx), n,
                                                           hist.ctypes.data_as(c_vp)))
        return hist

    def u16_histogram(self, vol, n):
        hist = np.empty(65536, dtype=np.uint64)
        self._check(lib().exabm4d_u16_histogram_dev(self.handle, _ptr(vol), n,
                                                    hist.ctypes.data_as(c_vp)))
        return hist

    def key_histogram(self, vol, dtype, n, digit, prefix=0, center=None):
        hist = np.empty(65536, dtype=np.uint64)
        self._check(lib().exabm4d_key_histogram_dev(
            self.handle, _ptr(vol), self.DTYPES[np.dtype(dtype)], n, 0 if center is None else 1,
            0.0 if center is None else float(center), int(digit), int(prefix),
            hist.ctypes.data_as(c_vp)))
        return hist

    def minmax(self, vol, dtype, n):
        out = np.empty(2, dtype=np.float64)
        self._check(lib().exabm4d_minmax_dev(self.handle, _ptr(vol), self.DTYPES[np.dtype(dtype)], n,
                                             out.ctypes.data_as(c_vp)))
        return float(out[0]), float(out[1])

    def masked_error_stats(self, pred, pred_dtype, ref, ref_dtype, mask, n, thr=float("inf")):
        out = np.empty(7, dtype=np.float64)
        self._check(lib().exabm4d_masked_error_stats_dev(
            self.handle, _ptr(pred), self.DTYPES[np.dtype(pred_dtype)], _ptr(ref),
            self.DTYPES[np.dtype(ref_dtype)], _ptr(mask) if mask is not None else None, n,
            float(thr), out.ctypes.data_as(c_vp)))
        return out

    def ssim3d_sum(self, a, b, dtype, shape, window, c1, c2):
        out = np.empty(1, dtype=np.float64)
        nz, ny, nx = shape
        self._check(lib().exabm4d_ssim3d_dev(self.handle, _ptr(a), _ptr(b),
                                             self.DTYPES[np.dtype(dtype)], nz, ny, nx, int(window),
                                             float(c1), float(c2), out.ctypes.data_as(c_vp)))
        return float(out[0])

    # -- scoring a box inside a window -------------------------------------------
    @staticmethod
    def _box_geometry(vol_dims, win_origin, win_dims, box_origin, box_dims):
        return [(ctypes.c_int32 * 3)(*(int(v) for v in t))
                for t in (vol_dims, win_origin, win_dims, box_origin, box_dims)]

    def diff_histogram_u16(self, ref_win, test_win, mask_win, vol_dims, win_origin, win_dims, box_origin, box_dims,
                           hist, zero_first=False):
        """``hist[(test - ref) + 65535] += 1`` over the box ``box_origin + [0, box_dims)`` of two uint16 windows
        that hold ``win_origin + [0, win_dims)`` of a volume of ``vol_dims`` (all z, y, x).  ``hist``: ``DIFF_BINS``
        uint64 counters on the device, added to (``zero_first`` zeroes them before); with ``mask_win`` (uint16,
        non-zero = foreground) two tables, foreground then background.  Asynchronous."""
        tri = self._box_geometry(vol_dims, win_origin, win_dims, box_origin, box_dims)
        self._check(lib().exabm4d_diff_histogram_u16_dev(self.handle, _ptr(ref_win), _ptr(test_win), _ptr(mask_win),
                                                         *tri, 1 if zero_first else 0, _ptr(hist)))

    def mip3_u16(self, ref_win, test_win, vol_dims, win_origin, win_dims, box_origin, box_dims, planes):
        """Folds the box's maxima over z, y and x of ref, test and ``|test - ref|`` into ``planes``: 3 x
        ``mip_plane_words(vol_dims)`` uint32 words on the device, zeroed by the caller once (``split_mip_planes``
        names them).  Asynchronous."""
        tri = self._box_geometry(vol_dims, win_origin, win_dims, box_origin, box_dims)
        self._check(lib().exabm4d_mip3_u16_dev(self.handle, _ptr(ref_win), _ptr(test_win), *tri, _ptr(planes)))

    def ssim3d_box_sum(self, ref_win, test_win, vol_dims, win_origin, win_dims, box_origin, box_dims, window, c1, c2):
        """The sum of ``ssim3d_sum``'s map over the box only, read from two uint16 windows; ValueError when the
        windows do not cover the box and its halo."""
        out = np.empty(1, dtype=np.float64)
        tri = self._box_geometry(vol_dims, win_origin, win_dims, box_origin, box_dims)
        self._check(lib().exabm4d_ssim3d_box_dev(self.handle, _ptr(ref_win), _ptr(test_win), *tri, int(window),
                                                 float(c1), float(c2), out.ctypes.data_as(c_vp)))
        return float(out[0])

    # -- noise table -----------------------------------------------------------
    def noise_table(self, vol, dtype, shape, shift=0):
        """(hist[NOISE_LEVELS, NOISE_BINS], sum_s[NOISE_LEVELS], skipped) of a uint16 or float32 volume of
        ``shape`` (nz, ny, nx) resident in HBM."""
        dt = np.dtype(dtype)
        if dt not in (np.dtype(np.uint16), np.dtype(np.float32)):
            raise ValueError("noise_table: the volume must be uint16 or float32")
        hist = np.empty((NOISE_LEVELS, NOISE_BINS), dtype=np.uint64)
        sum_s = np.empty(NOISE_LEVELS, dtype=np.uint64)
        skipped = np.empty(1, dtype=np.uint64)
        nz, ny, nx = shape
        self._check(lib().exabm4d_noise_table_dev(
            self.handle, _ptr(vol), self.DTYPES[dt], int(nz), int(ny), int(nx), int(shift),
            hist.ctypes.data_as(c_vp), sum_s.ctypes.data_as(c_vp), skipped.ctypes.data_as(c_vp)))
        return hist, sum_s, int(skipped[0])

    # -- measuring a box inside a window ---------------------------------------
    def measure_box_u16(self, win, mask_win, vol_dims, win_origin, win_dims, box_origin, box_dims, counts, noise,
                        zero_first=False):
        """Adds the box ``box_origin + [0, box_dims)`` of a uint16 window that holds ``win_origin + [0, win_dims)`` of a
        volume of ``vol_dims`` (all z, y, x) to two tables on the device: ``counts`` (``COUNT_BINS`` uint64, one per
        value) and ``noise`` (``measure_noise_words()`` uint64: the wide noise table ``[NOISE_LEVELS,
        NOISE_WIDE_BINS]`` of the cells whose origins lie in the box, then ``sum_s``); ``zero_first`` zeroes them
        before.  With ``mask_win`` (uint16, non-zero = foreground) two tables each, foreground then background.
        ValueError when the window misses the far corner of a cell that begins in the box.  Asynchronous."""
        tri = self._box_geometry(vol_dims, win_origin, win_dims, box_origin, box_dims)
        self._check(lib().exabm4d_measure_box_u16_dev(self.handle, _ptr(win), _ptr(mask_win), *tri,
                                                      1 if zero_first else 0, _ptr(counts), _ptr(noise)))

    # -- the foreground mask of a box inside a window ----------------------------
    def foreground_box_u16(self, win, vol_dims, win_origin, win_dims, box_origin, box_dims, cut, radius, value=1,
                           out_u16=None, out_u8=None, counts=None, zero_first=False):
        """The mask of the box ``box_origin + [0, box_dims)`` of a uint16 window that holds ``win_origin + [0,
        win_dims)`` of a volume of ``vol_dims`` (all z, y, x): ``value`` where a voxel of the VOLUME with a count
        ``>= cut`` (0..65536) lies within the L1 distance ``radius`` (0..``FG_MAX_RADIUS``), else 0 -- ``radius``
        iterations of the 6-neighbour cross on ``vol >= cut``.  ``out_u16`` (``value`` / 0) and ``out_u8`` (1 / 0):
        dense device arrays of ``box_dims``, one at least.  ``counts``: two uint64 on the device, to which the seeds
        and the mask voxels of the box are added (``zero_first`` zeroes them before).  What the window holds past the
        volume's faces is never a seed.  ValueError when the window misses the box grown by ``radius`` (cut at the
        volume).  Asynchronous."""
        tri = self._box_geometry(vol_dims, win_origin, win_dims, box_origin, box_dims)
        self._check(lib().exabm4d_foreground_box_u16_dev(self.handle, _ptr(win), *tri, int(cut), int(radius),
                                                         int(value), _ptr(out_u16), _ptr(out_u8), _ptr(counts),
                                                         1 if zero_first else 0))

    # -- connected components of the seeds, and their filter by size -------------
    def component_seeds_u16(self, win, vol_dims, win_origin, win_dims, box_origin, box_dims, cut, min_voxels,
                            connectivity=26, count_origin=None, count_dims=None, seeds_u16=None, labels=None,
                            sizes=None, scratch=None, counts=None, zero_first=False, scratch_bytes=None):
        """The seeds (``>= cut``) of a uint16 window in the geometry of ``foreground_box_u16``, labelled by
        connected component (``connectivity`` 6 or 26) inside ``components_region(...)`` -- the box grown by
        ``min_voxels - 1`` and cut at the volume, which the window must hold -- and filtered: ``seeds_u16`` (dense
        uint16 of ``box_dims``) gets 1 where a seed's component has at least ``min_voxels`` voxels, else 0.
        ``labels`` / ``sizes``: uint32 per voxel of the region (label = 1 + region index of the component's first
        voxel; its size at index label - 1).  ``counts``: three uint64 on the device to which the seeds, the kept
        seeds and the dropped components (by first voxel) of ``count_origin + [0, count_dims)`` (default: the box)
        are added (``zero_first`` zeroes them before).  ``scratch``: a device buffer of at least
        ``components_scratch_bytes(win_dims)`` bytes (``scratch_bytes`` of them where it is a bare pointer); one
        is allocated and freed here when None.  Asynchronous when ``scratch`` is given."""
        tri = self._box_geometry(vol_dims, win_origin, win_dims, box_origin, box_dims)
        cnt = [(ctypes.c_int32 * 3)(*(int(v) for v in t))
               for t in (box_origin if count_origin is None else count_origin,
                         box_dims if count_dims is None else count_dims)]
        own = None
        if scratch is None:
            scratch = own = self.alloc(max(256, components_scratch_bytes(win_dims, connectivity)))
        try:
            self._check(lib().exabm4d_component_seeds_u16_dev(
                self.handle, _ptr(win), *tri, *cnt, int(cut), int(min_voxels), int(connectivity), _ptr(seeds_u16),
                _ptr(labels), _ptr(sizes), _ptr(scratch), int(scratch.nbytes if scratch_bytes is None else scratch_bytes),
                _ptr(counts), 1 if zero_first else 0))
        finally:
            if own is not None:
                own.free()                               # (freeing a buffer waits for the stream)

    def label_components(self, src, dtype, shape, cut=1, min_voxels=1, connectivity=26, labels=None, sizes=None,
                         kept_u8=None, scratch=None, counts=None, scratch_bytes=None):
        """``component_seeds_u16`` for a dense uint8 (seed where non-zero) or uint16 (seed where ``>= cut``) array
        of ``shape`` resident on the device, as box = window = volume: ``labels`` / ``sizes`` (uint32 per voxel),
        ``kept_u8`` (1 where the voxel's component has at least ``min_voxels`` voxels, any number >= 1) and
        ``counts`` (three uint64, zeroed first), each optional."""
        dt = np.dtype(dtype)
        if dt not in (np.dtype(np.uint8), np.dtype(np.bool_), np.dtype(np.uint16)):
            raise ValueError("label_components: the array must be uint8, bool or uint16")
        dims = (ctypes.c_int32 * 3)(*(int(v) for v in shape))
        own = None
        if scratch is None:
            scratch = own = self.alloc(max(256, components_scratch_bytes(shape, connectivity)))
        try:
            self._check(lib().exabm4d_label_components_dev(
                self.handle, _ptr(src), 1 if dt == np.dtype(np.uint16) else 0, dims, int(cut), int(min_voxels),
                int(connectivity), _ptr(labels), _ptr(sizes), _ptr(kept_u8), _ptr(scratch),
                int(scratch.nbytes if scratch_bytes is None else scratch_bytes), _ptr(counts)))
        finally:
            if own is not None:
                own.free()

    # -- the components of a volume from those of its bricks' windows -----------
    def segment_collect(self, labels, vol_dims, win_origin, win_dims, brick_origin, brick_dims, own, halo, halo_capacity,
                        face, face_capacity, size, size_capacity, counts):
        """What a merge over all bricks needs of one window's ``labels`` (uint32, ``component_seeds_u16`` with region
        = window): ``own`` (uint32 per voxel of the window, zeroed here) gets the voxels of each component inside the
        brick at index label - 1; ``halo`` / ``face`` / ``size`` (pairs of uint64, capacities in records) get the
        (volume index, provisional label) of the seeds outside the brick and of the brick's seeds on its low faces
        with a brick before them, and (provisional label, own count) per component with an own count; ``counts``
        (three uint64, zeroed here): the records there are of each kind.  ``segment_record_capacities`` states the
        least halo and face capacities; size records past ``size_capacity`` are counted and not stored.
        Asynchronous."""
        tri = self._box_geometry(vol_dims, win_origin, win_dims, brick_origin, brick_dims)
        self._check(lib().exabm4d_segment_collect_dev(
            self.handle, _ptr(labels), *tri, _ptr(own), _ptr(halo), int(halo_capacity), _ptr(face), int(face_capacity),
            _ptr(size), int(size_capacity), _ptr(counts)))

    def segment_relabel(self, labels, vol_dims, win_origin, win_dims, brick_origin, brick_dims, keys, vals, n_keys,
                        typesize, final, out):
        """The dense brick ``out`` (``typesize`` 4 or 8 bytes an element) of a window's ``labels``: ``vals[k]`` where
        ``keys[k]`` (uint64 on the device, ascending; None with ``n_keys`` 0) is the component's provisional label,
        else the provisional label, background 0.  ``final``: ``typesize`` bytes per voxel of the window, not kept.
        Asynchronous."""
        tri = self._box_geometry(vol_dims, win_origin, win_dims, brick_origin, brick_dims)
        self._check(lib().exabm4d_segment_relabel_dev(
            self.handle, _ptr(labels), *tri, _ptr(keys), _ptr(vals), int(n_keys), int(typesize), _ptr(final),
            _ptr(out)))

    def nonzero_u8(self, src, n, dst):
        """``dst[i] = src[i] != 0`` for ``n`` uint16 elements on the device, as bytes.  Asynchronous."""
        self._check(lib().exabm4d_nonzero_u8_dev(self.handle, _ptr(src), int(n), _ptr(dst)))

    # -- one pyramid level of a box inside a window -------------------------------
    def downsample_box_u16(self, win, vol_dims, win_origin, win_dims, box_origin, box_dims, factors, method="mode",
                           edge="crop", out_u16=None):
        """The box ``box_origin + [0, box_dims)`` of one pyramid level -- LEVEL coordinates -- of a SOURCE volume of
        ``vol_dims``, read from a uint16 window that holds ``win_origin + [0, win_dims)`` of the source (all z, y, x):
        every level voxel reduces its window of ``factors`` (1 or 2 each, one at least 2) source voxels, cut at the
        volume's faces, by ``method`` (``"mode"``: ties to the smallest value; ``"mean"``: half to even; ``"max"``).
        ``edge``: ``"crop"`` (the level has ``n // f`` voxels per axis) or ``"partial"`` (``ceil(n / f)``).
        ``out_u16``: a dense device array of ``box_dims``.  What the window holds past the volume's faces never enters
        a result.  ValueError when the box leaves the level or the window misses ``[box_origin f, min(vol,
        (box_origin + box_dims) f))``.  Asynchronous."""
        tri = self._box_geometry(vol_dims, win_origin, win_dims, box_origin, box_dims)
        fac = (ctypes.c_int32 * 3)(*(int(f) for f in factors))
        self._check(lib().exabm4d_downsample_box_u16_dev(
            self.handle, _ptr(win), *tri, fac, DS_METHODS.get(method, -1) if isinstance(method, str) else int(method),
            DS_EDGES.get(edge, -1) if isinstance(edge, str) else int(edge), _ptr(out_u16)))

    def downsample_box_labels(self, win, dtype, vol_dims, win_origin, win_dims, box_origin, box_dims, factors,
                              edge="crop", zeros="count", out=None):
        """``downsample_box_u16`` for a window of uint32 / uint64 ids (``dtype``), which compare as unsigned integers
        (DESIGN.md 5.24): every level voxel becomes the most frequent value of its window of source voxels, ties to the
        smallest value; with ``zeros="ignore"`` the most frequent non-zero value, 0 only where every voxel present is
        0 (``"count"``: 0 is a value like any other).  ``out``: a dense device array of ``box_dims`` of ``dtype``.
        ValueError as there, and for another dtype or a pointer not aligned to it.  Asynchronous."""
        tri = self._box_geometry(vol_dims, win_origin, win_dims, box_origin, box_dims)
        fac = (ctypes.c_int32 * 3)(*(int(f) for f in factors))
        self._check(lib().exabm4d_downsample_box_labels_dev(
            self.handle, _ptr(win), int(np.dtype(dtype).itemsize) if np.dtype(dtype).kind == "u" else -1, *tri, fac,
            DS_EDGES.get(edge, -1) if isinstance(edge, str) else int(edge),
            LABEL_ZEROS.get(zeros, -1) if isinstance(zeros, str) else int(zeros), _ptr(out)))

    # -- patch-cache masks and coherence gate; batches of (nz, ny, nx) patches --
    def foreground_masks(self, raw, dtype, batch, shape, k, dilate, mask):
        """Masks into the device bytes ``mask``; returns the per-patch fp32 thresholds."""
        thr = np.empty(batch, dtype=np.float32)
        nz, ny, nx = shape
        self._check(lib().exabm4d_foreground_masks_dev(
            self.handle, _ptr(raw), self.DTYPES[np.dtype(dtype)], int(batch), nz, ny, nx, float(k),
            int(dilate), _ptr(mask), thr.ctypes.data_as(c_vp)))
        return thr

    def binary_dilate(self, src, batch, shape, iterations, out):
        nz, ny, nx = shape
        self._check(lib().exabm4d_binary_dilate_dev(self.handle, _ptr(src), int(batch), nz, ny, nx,
                                                    int(iterations), _ptr(out)))

    def gaussian_filter3d(self, src, dtype, batch, shape, weights, out):
        """``weights``: the centre-and-right half (radius + 1 doubles) of the normalised kernel."""
        w = np.ascontiguousarray(weights, dtype=np.float64)
        nz, ny, nx = shape
        self._check(lib().exabm4d_gaussian_filter3d_dev(
            self.handle, _ptr(src), self.DTYPES[np.dtype(dtype)], int(batch), nz, ny, nx,
            w.ctypes.data_as(c_vp), len(w) - 1, _ptr(out)))

    def label_set(self, labels, dtype, batch, shape):
        """(keys, counts, held, status): keys / counts (batch, LABEL_SET_MAX), unordered."""
        keys = np.empty((batch, LABEL_SET_MAX), dtype=np.uint64)
        counts = np.empty((batch, LABEL_SET_MAX), dtype=np.uint32)
        held = np.empty(batch, dtype=np.uint32)
        status = np.empty(batch, dtype=np.uint32)
        nz, ny, nx = shape
        self._check(lib().exabm4d_label_set_dev(
            self.handle, _ptr(labels), LABEL_DTYPES[np.dtype(dtype)], int(batch), nz, ny, nx,
            keys.ctypes.data_as(c_vp), counts.ctypes.data_as(c_vp), held.ctypes.data_as(c_vp),
            status.ctypes.data_as(c_vp)))
        return keys, counts, held, status

    def segment_stats(self, labels, label_dtype, raw, raw_dtype, smooth, batch, shape, lag,
                      item_patch, item_key):
        """(n_items, SEG_STATS_K) float64 statistics of each (patch, label) item."""
        ip = np.ascontiguousarray(item_patch, dtype=np.int32)
        ik = np.ascontiguousarray(item_key, dtype=np.uint64)
        out = np.empty((len(ip), SEG_STATS_K), dtype=np.float64)
        nz, ny, nx = shape
        self._check(lib().exabm4d_segment_stats_dev(
            self.handle, _ptr(labels), LABEL_DTYPES[np.dtype(label_dtype)], _ptr(raw),
            self.DTYPES[np.dtype(raw_dtype)], _ptr(smooth), int(batch), nz, ny, nx, int(lag),
            ip.ctypes.data_as(c_vp), ik.ctypes.data_as(c_vp), len(ip), out.ctypes.data_as(c_vp)))
        return out

    # -- patch samplers ------------------------------------------------------------
    def foreground_counts(self, raw, dtype, batch, shape, k=6.0, dilate=1):
        """``int(make_foreground_mask(raw[b], k, dilate).sum())`` of ``batch`` uint16 or float32 patches on the
        device, as a (batch,) uint32 array; no mask is written for ``dilate`` 0 or 1."""
        counts = np.empty(int(batch), dtype=np.uint32)
        nz, ny, nx = shape
        self._check(lib().exabm4d_foreground_counts_dev(
            self.handle, _ptr(raw), self.DTYPES[np.dtype(dtype)], int(batch), int(nz), int(ny), int(nx), float(k),
            int(dilate), counts.ctypes.data_as(c_vp), None))
        return counts

    def annotation_masks(self, labels, label_dtype, seg_dilate, points, npoints, starts, skel_dilate, shape, mask):
        """``make_segmentation_mask(labels[b], seg_dilate) | make_skeleton_mask(points, starts[b], shape,
        skel_dilate)`` of every box into the device bytes ``mask``.  ``labels``: None or (batch, *shape) labels on
        the device; ``points``: None or ``npoints`` int32 zyx triples on the device; ``starts``: host (batch, 3)."""
        starts = np.ascontiguousarray(starts, dtype=np.int32).reshape(-1, 3)
        nz, ny, nx = shape
        self._check(lib().exabm4d_annotation_masks_dev(
            self.handle, _ptr(labels), LABEL_DTYPES[np.dtype(label_dtype)] if labels is not None else 0,
            int(seg_dilate), _ptr(points), int(npoints), starts.ctypes.data_as(c_vp), int(skel_dilate), len(starts),
            int(nz), int(ny), int(nx), _ptr(mask)))

    # -- validation scoring ------------------------------------------------------
    def evaluate_batch(self, pred, pred_dtype, raw, raw_dtype, target, target_dtype, mask, batch, n, k, ranks):
        """(batch, EVAL_K) float64 rows of ``exabm4d_evaluate_batch_dev``: the sums, counts, maxima, median, MAD,
        threshold and rank values ``evaluate_example`` is made of, for ``batch`` patches of ``n`` voxels on the
        device.  ``ranks``: the two median ranks, then the two percentile ranks (0-based)."""
        rk = (ctypes.c_uint32 * 4)(*[int(r) for r in ranks])
        out = np.empty((int(batch), EVAL_K), dtype=np.float64)
        self._check(lib().exabm4d_evaluate_batch_dev(
            self.handle, _ptr(pred), self.DTYPES[np.dtype(pred_dtype)], _ptr(raw),
            self.DTYPES[np.dtype(raw_dtype)], _ptr(target), self.DTYPES[np.dtype(target_dtype)], _ptr(mask),
            int(batch), int(n), float(k), rk, out.ctypes.data_as(c_vp)))
        return out

    # -- region reads of a chunk store --------------------------------------------
    def gather_boxes(self, pool, pool_elems, srcs, box_srcs, starts, box, out, dtype=np.uint16, offset=0.0, fill=0):
        """out[n][z][y][x] <- the voxel at starts[n] + (z, y, x) from the first source of ``box_srcs[n]`` that holds
        it, else ``fill``.  ``pool``: device uint16; ``srcs``: host array of ``BOX_SRC``; ``box_srcs``: host int32
        (nbox, per_box), -1 = unused; ``starts``: host int32 (nbox, 3); ``out``: device, nbox * prod(box) elements of
        ``dtype`` (uint16, or float32 = value - offset).  Checked on the host (ValueError, nothing written);
        asynchronous on the context's stream."""
        dt = np.dtype(dtype)
        if dt not in (np.dtype(np.uint16), np.dtype(np.float32)):
            raise ValueError("gather_boxes: out is uint16 or float32")
        srcs = np.ascontiguousarray(srcs, dtype=BOX_SRC).reshape(-1)
        starts = np.ascontiguousarray(starts, dtype=np.int32).reshape(-1, 3)
        box_srcs = np.ascontiguousarray(box_srcs, dtype=np.int32)
        if box_srcs.ndim != 2 or box_srcs.shape[0] != len(starts):
            raise ValueError("gather_boxes: box_srcs must be (nbox, per_box)")
        bz, by, bx = (int(b) for b in box)
        self._check(lib().exabm4d_gather_boxes_dev(
            self.handle, _ptr(pool), int(pool_elems), srcs.ctypes.data_as(c_vp), len(srcs),
            box_srcs.ctypes.data_as(c_vp), box_srcs.shape[1], starts.ctypes.data_as(c_vp), len(starts), bz, by, bx,
            self.DTYPES[dt], float(offset), float(fill), _ptr(out)))

    # -- region writes of a chunk store -------------------------------------------
    SCATTER_DTYPES = {np.dtype(np.uint16): 0, np.dtype(np.float32): 1, np.dtype(np.uint8): 3}

    def scatter_boxes(self, src, src_elems, src_dtype, boxes, pool, pool_elems, pool_dtype, dsts, dst_boxes,
                      offset=0.0):
        """The gather's mirror: every voxel of every destination ``dsts[d]`` (``BOX_SRC`` records: regions of the
        device buffer ``pool``) takes the value of the last box of ``dst_boxes[d]`` (host int32 (ndst, per_dst), -1 =
        unused) that holds it, read from the device buffer ``src`` where ``boxes[k]`` (``BOX_SRC``) says; a voxel no
        listed box holds stays as it is.  (``src_dtype``, ``pool_dtype``): (uint16, uint16), (uint8, uint8), or
        (float32, uint16) = ``rint(clip(v + offset, 0, 65535))``.  The destinations must not overlap.  Checked on
        the host (ValueError, nothing written); asynchronous on the context's stream."""
        sdt, pdt = np.dtype(src_dtype), np.dtype(pool_dtype)
        if sdt not in self.SCATTER_DTYPES or pdt not in self.SCATTER_DTYPES:
            raise ValueError("scatter_boxes: elements are uint16, float32 or uint8")
        boxes = np.ascontiguousarray(boxes, dtype=BOX_SRC).reshape(-1)
        dsts = np.ascontiguousarray(dsts, dtype=BOX_SRC).reshape(-1)
        dst_boxes = np.ascontiguousarray(dst_boxes, dtype=np.int32)
        if dst_boxes.ndim != 2 or dst_boxes.shape[0] != len(dsts):
            raise ValueError("scatter_boxes: dst_boxes must be (ndst, per_dst)")
        self._check(lib().exabm4d_scatter_boxes_dev(
            self.handle, _ptr(src), int(src_elems), self.SCATTER_DTYPES[sdt], boxes.ctypes.data_as(c_vp), len(boxes),
            _ptr(pool), int(pool_elems), self.SCATTER_DTYPES[pdt], dsts.ctypes.data_as(c_vp), len(dsts),
            dst_boxes.ctypes.data_as(c_vp), dst_boxes.shape[1], float(offset)))

    # -- label codec ---------------------------------------------------------
    def label_encode(self, vol, typesize, shape, chunk, out=None, out_capacity=0, offsets=None, sizes=None,
                     totals=True):
        """Code every chunk of a device uint32 / uint64 volume as ``exac-labels`` streams.  -> (sum of stream
        lengths, container bytes) when `totals` (synchronises), else None."""
        nz, ny, nx = shape
        tot = np.zeros(2, dtype=np.uint64)
        self._check(lib().exabm4d_label_encode_dev(
            self.handle, _ptr(vol), int(typesize), nz, ny, nx, int(chunk[0]), int(chunk[1]), int(chunk[2]),
            _ptr(out), int(out_capacity), _ptr(offsets), _ptr(sizes), tot.ctypes.data_as(c_vp) if totals else None))
        return (int(tot[0]), int(tot[1])) if totals else None

    def label_decode(self, data, nbytes, offsets, typesize, shape, chunk, vol):
        """``data``: ``nbytes`` bytes of ``exac-labels`` streams on the device -> ``vol``; a malformed stream or a
        palette index past its palette raises ValueError, without a read outside ``data`` or a write outside
        ``vol``."""
        nz, ny, nx = shape
        self._check(lib().exabm4d_label_decode_dev(
            self.handle, _ptr(data), int(nbytes), _ptr(offsets), int(typesize), nz, ny, nx, int(chunk[0]),
            int(chunk[1]), int(chunk[2]), _ptr(vol)))

    def label_gather_boxes(self, data, nbytes, typesize, srcs, box_srcs, starts, box, shape, chunk, out):
        """out[n][z][y][x] <- the label at starts[n] + (z, y, x) of the array ``shape`` in chunks ``chunk``, read
        from the coded chunks in the device container ``data``; 0 outside the array.  ``srcs``: host array of
        ``LABEL_SRC``; ``box_srcs``: host int32 (nbox, per_box), per box the rows of ``srcs`` of its chunk range in
        raster order; ``starts``: host int32 (nbox, 3); ``out``: device, nbox * prod(box) elements.  Checked on the
        host (ValueError, nothing written); synchronises."""
        srcs = np.ascontiguousarray(srcs, dtype=LABEL_SRC).reshape(-1)
        starts = np.ascontiguousarray(starts, dtype=np.int32).reshape(-1, 3)
        box_srcs = np.ascontiguousarray(box_srcs, dtype=np.int32)
        if box_srcs.ndim != 2 or box_srcs.shape[0] != len(starts):
            raise ValueError("label_gather_boxes: box_srcs must be (nbox, per_box)")
        bz, by, bx = (int(b) for b in box)
        shape3 = (ctypes.c_int32 * 3)(*[int(v) for v in shape])
        chunk3 = (ctypes.c_int32 * 3)(*[int(v) for v in chunk])
        self._check(lib().exabm4d_label_gather_boxes_dev(
            self.handle, _ptr(data), int(nbytes), int(typesize), srcs.ctypes.data_as(c_vp), len(srcs),
            box_srcs.ctypes.data_as(c_vp), box_srcs.shape[1], starts.ctypes.data_as(c_vp), len(starts), bz, by, bx,
            shape3, chunk3, _ptr(out)))

    def close(self):
        if self.handle and os.getpid() == self.pid:
            lib().exabm4d_destroy(self.handle)
        self.handle = None


COMM_ID_BYTES = 128


def comm_unique_id():
    """128 bytes from ncclGetUniqueId (rank 0 draws them; every rank passes them to ``Comm``)."""
    buf = (ctypes.c_uint8 * COMM_ID_BYTES)()
    rc = lib().exabm4d_comm_unique_id(buf)
    if rc:
        raise NativeError(lib().exabm4d_last_error(None).decode())
    return bytes(buf)


class Comm:
    """An RCCL communicator bound to a context's device (exabm4d_comm_*): the halo exchange of the sharded
    modes without torch.distributed.  Creation is collective over the ranks."""

    def __init__(self, ctx, nranks, rank, unique_id):
        if len(unique_id) != COMM_ID_BYTES:
            raise ValueError("unique_id must be %d bytes" % COMM_ID_BYTES)
        self.ctx, self.nranks, self.rank = ctx, int(nranks), int(rank)
        h = c_vp()
        buf = (ctypes.c_uint8 * COMM_ID_BYTES).from_buffer_copy(unique_id)
        ctx._check(lib().exabm4d_comm_create(ctx.handle, self.nranks, self.rank, buf, ctypes.byref(h)))
        self.handle = h

    def halo_exchange(self, lo_peer, send_lo, recv_lo, bytes_lo, hi_peer, send_hi, recv_hi, bytes_hi):
        """ncclGroupStart; send / recv with each neighbour; ncclGroupEnd -- on the context's stream, device
        pointers (ints, DeviceBuffers or tensors), a peer of -1 skips that side."""
        self.ctx._check(lib().exabm4d_halo_exchange_dev(
            self.ctx.handle, self.handle, int(lo_peer), _ptr(send_lo), _ptr(recv_lo), int(bytes_lo),
            int(hi_peer), _ptr(send_hi), _ptr(recv_hi), int(bytes_hi)))

    def max(self, value):
        """max over the ranks of ``value`` (a float); synchronises the context's stream: barrier + MAX."""
        v = ctypes.c_double(float(value))
        self.ctx._check(lib().exabm4d_comm_max_f64_host(self.ctx.handle, self.handle, ctypes.byref(v)))
        return float(v.value)

    def close(self):
        if self.handle:
            lib().exabm4d_comm_destroy(self.handle)
            self.handle = None


_contexts = {}
_ctx_lock = threading.Lock()
_hip_owner_pid = None        # pid of the process in which this module first created a context
_forked_from_hip_parent = False


def _after_fork_in_child():
    """HIP state does not survive fork(): a child of a process that had already initialised HIP
    (through this module or through torch) cannot use the GPU.  The reference's callers fork
    workers BEFORE any of them touches BM4D (scripts/precompute.py:215-222), which works; the
    other order must fail loudly instead of hanging in the driver."""
    global _forked_from_hip_parent
    torch_mod = __import__("sys").modules.get("torch")
    torch_up = False
    try:
        torch_up = bool(torch_mod is not None and torch_mod.cuda.is_initialized())
    except Exception:
        pass
    if _hip_owner_pid is not None or torch_up:
        _forked_from_hip_parent = True


os.register_at_fork(after_in_child=_after_fork_in_child)


def context(device=None):
    """The calling process's context for ``device`` (default: ``default_device()`` -- EXABM4D_DEVICE,
    LOCAL_RANK, or this pool worker's index mod the device count), created lazily.

    A context inherited through fork() is never reused: HIP state does not survive fork."""
    if device is None:
        device = default_device()
    global _hip_owner_pid
    if _forked_from_hip_parent:
        raise NativeError(
            "this process was fork()ed from a process that had already initialised HIP; the GPU "
            "cannot be used here.  Fork the workers before the parent touches the GPU (as "
            "scripts/precompute.py does), or start them with the 'spawn' method.")
    key = (os.getpid(), int(device))
    with _ctx_lock:
        ctx = _contexts.get(key)
        if ctx is None:
            ctx = Context(device)
            _contexts[key] = ctx
            if _hip_owner_pid is None:
                _hip_owner_pid = os.getpid()
    return ctx


def new_context(device=None):
    """One MORE context of the calling process on ``device`` (its own stream and scratch): for callers that keep
    several device calls in flight from several threads (the broker).  Not cached; the caller keeps it."""
    first = context(device)                 # the fork checks, and the process's cached context
    return Context(first.device)


def check_host_volume_pair(src, dst):
    """What exabm4d_denoise_chunked_u16_host needs of its two host arrays (raises ValueError)."""
    for a in (src, dst):
        if not isinstance(a, np.ndarray) or a.ndim != 3 or a.dtype != np.uint16 or not a.flags.c_contiguous:
            raise ValueError("3-D C-contiguous uint16 arrays expected")
    if src.shape != dst.shape:
        raise ValueError("source and destination differ in shape")
    if not dst.flags.writeable:
        raise ValueError("the destination is read-only")
    if np.shares_memory(src, dst):
        raise ValueError("source and destination may not overlap")


def slab_order_tile(position, columns, q):
    """Tile of launch position ``position`` (a workgroup's ticket, bm_kernels.hip ORDER) in slab order:
    XCD c = position mod 8 walks positions [c q, (c + 1) q) of every slab of ``columns`` tiles; returns
    (slab, column) or None for a padding position.  The host-side mirror of ``xcd_slab_sync``: the tile one
    slab below has position - 8 q, i.e. a smaller ticket."""
    c, j = position & 7, position >> 3
    slab, w = divmod(j, q)
    t = c * q + w
    return (slab, t) if t < columns else None


def blockmatch_plan(shape, batch=1, ctx=None):
    """The launch block matching chooses for this geometry (host logic of libexabm4d.so, no GPU needed):
    dict with the tile grid, the slab-order parameter, whether tiles carry their top cell layer upwards
     and the part of the context's scratch that takes.  ``ctx``: follow that context's
    options (None: the defaults)."""
    out = (ctypes.c_int32 * 6)()
    nbytes = ctypes.c_uint64()
    rc = lib().exabm4d_blockmatch_plan(ctx.handle if ctx is not None else None, int(shape[0]), int(shape[1]),
                                       int(shape[2]), int(batch), out, ctypes.byref(nbytes))
    if rc != 0:
        raise ValueError("blockmatch_plan: %s" % lib().exabm4d_last_error(None).decode())
    return {"tiles_z": out[0], "tiles_y": out[1], "tiles_x": out[2], "slab_order_q": out[3], "carry": bool(out[4]),
            "flat_tiles": bool(out[5]), "carry_bytes": int(nbytes.value)}


def device_count():
    """Number of visible devices.  hipGetDeviceCount initialises the HIP runtime, so the calling
    process counts as a HIP owner for the fork guard from here on."""
    global _hip_owner_pid
    n = int(lib().exabm4d_device_count())
    if _hip_owner_pid is None:
        _hip_owner_pid = os.getpid()
    return n


def device_count_no_init():
    """Number of GPUs this process would see, WITHOUT initialising the HIP runtime (a parent that is about to
    fork workers must not, see ``context``): the visibility lists HIP honours if one is set, else the KFD
    topology (nodes with SIMDs are GPUs).  0 when neither says anything."""
    for var in ("HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES"):
        v = os.environ.get(var)
        if v is not None:
            return len([t for t in v.split(",") if t.strip() != ""])
    root = "/sys/class/kfd/kfd/topology/nodes"
    n = 0
    try:
        for node in os.listdir(root):
            try:
                with open(os.path.join(root, node, "properties")) as f:
                    props = dict(line.split()[:2] for line in f if len(line.split()) >= 2)
                if int(props.get("simd_count", "0")) > 0:
                    n += 1
            except (OSError, ValueError):
                continue
    except OSError:
        return 0
    return n


def worker_index():
    """0-based index of this process among its parent's pool workers (``multiprocessing`` numbers the
    processes it starts: ``current_process()._identity`` -- what ``ProcessPoolExecutor`` workers carry), or
    None for a process nobody numbered (the main process, a plain ``os.fork``)."""
    try:
        import multiprocessing
        ident = multiprocessing.current_process()._identity
        return int(ident[-1]) - 1 if ident else None
    except Exception:
        return None


def default_device(count=None):
    """The device of a caller that named none: ``EXABM4D_DEVICE`` if set; else ``LOCAL_RANK`` (one process
    per GPU under torch.distributed.run); else -- the reference's worker pattern, a pool of forked workers
    that each call ``bm4d()`` (scripts/precompute.py:215-228) -- worker index mod device count, so that a
    pool spreads over the node's GPUs instead of piling onto device 0; a process without a worker index
    (the main process) gets 0.  ``count``: the device count to use (tests); default ``device_count_no_init()``."""
    v = os.environ.get("EXABM4D_DEVICE")
    if v not in (None, ""):
        return int(v)
    v = os.environ.get("LOCAL_RANK")
    if v not in (None, ""):
        return int(v)
    idx = worker_index()
    if idx is None:
        return 0
    n = device_count_no_init() if count is None else int(count)
    return idx % n if n > 0 else 0


# -- host-only helpers (no GPU) -----------------------------------------------------------------
def mip_plane_words(vol_dims):
    """32-bit words of the three projection planes (y, x), (z, x), (z, y) of one volume (``Context.mip3_u16``)."""
    nz, ny, nx = (int(v) for v in vol_dims)
    return ny * nx + nz * nx + nz * ny


def split_mip_planes(words, vol_dims):
    """The downloaded words of ``Context.mip3_u16`` -> ``{"ref" | "test" | "abs_diff": (yx, zx, zy)}`` as uint16."""
    nz, ny, nx = (int(v) for v in vol_dims)
    per = mip_plane_words(vol_dims)
    out = {}
    for i, name in enumerate(("ref", "test", "abs_diff")):
        w = np.asarray(words[i * per:(i + 1) * per])
        out[name] = (w[:ny * nx].reshape(ny, nx).astype(np.uint16),
                     w[ny * nx:ny * nx + nz * nx].reshape(nz, nx).astype(np.uint16),
                     w[ny * nx + nz * nx:].reshape(nz, ny).astype(np.uint16))
    return out


def measure_noise_words():
    """uint64 words of one noise block of ``Context.measure_box_u16``: the wide table, then ``sum_s``."""
    return NOISE_LEVELS * NOISE_WIDE_BINS + NOISE_LEVELS


def codec_chunk_bound(n, typesize):
    return int(lib().exabm4d_codec_chunk_bound(int(n), int(typesize)))


def codec_volume_bound(typesize, shape, chunk):
    b = int(lib().exabm4d_codec_volume_bound(int(typesize), int(shape[0]), int(shape[1]),
                                             int(shape[2]), int(chunk[0]), int(chunk[1]),
                                             int(chunk[2])))
    if b == 0:
        raise ValueError("codec: typesize must be 2 or 4 and every size >= 1")
    return b



def label_encode_bound(typesize, shape, chunk):
    """Bytes that hold the ``exac-labels`` container of any volume of this geometry."""
    b = lib().exabm4d_label_encode_bound(int(typesize), *[int(v) for v in shape], *[int(v) for v in chunk])
    if b == 0:
        raise ValueError("label codec: typesize must be 4 or 8, sizes >= 1, chunk <= 2^27 voxels, volume <= 2^40")
    return int(b)


def bounded_volume_bound(shape, chunk):
    b = int(lib().exabm4d_bounded_volume_bound(*(int(s) for s in shape), *(int(c) for c in chunk)))
    if b == 0:
        raise ValueError("bounded codec: sizes >= 1, chunk axes multiples of 8 in [8, 65528], chunk <= 2^28 voxels")
    return b


def block_bounded_volume_bound(shape, chunk):
    b = int(lib().exabm4d_block_bounded_volume_bound(*(int(s) for s in shape), *(int(c) for c in chunk)))
    if b == 0:
        raise ValueError("block-bounded codec: sizes >= 1, chunk axes multiples of 8 in [8, 65528], "
                         "chunk <= 2^28 voxels")
    return b


def grid_positions(n):
    c = lib().exabm4d_grid_count(int(n))
    pos = np.zeros(max(c, 0), dtype=np.int32)
    if c > 0:
        lib().exabm4d_grid_positions(int(n), pos.ctypes.data_as(c_i32p))
    return pos


def tables(params=None):
    p = params or default_params()
    dct = np.zeros(64, dtype=np.float32)
    win = np.zeros(512, dtype=np.float32)
    rc = lib().exabm4d_tables(ctypes.byref(p), dct.ctypes.data_as(c_f32p),
                              win.ctypes.data_as(c_f32p))
    if rc:
        raise ValueError(lib().exabm4d_last_error(None).decode())
    return dct.reshape(8, 8), win.reshape(8, 8, 8)


def match_decode(keys16, ref_pos, ny, nx):
    keys16 = np.ascontiguousarray(keys16, dtype=np.uint32)
    idx = np.zeros(16, dtype=np.int64)
    dist = np.zeros(16, dtype=np.float32)
    cnt = ctypes.c_int()
    rc = lib().exabm4d_match_decode(keys16.ctypes.data_as(c_u32p), int(ref_pos[0]),
                                    int(ref_pos[1]), int(ref_pos[2]), int(ny), int(nx),
                                    idx.ctypes.data_as(c_i64p), dist.ctypes.data_as(c_f32p),
                                    ctypes.byref(cnt))
    if rc:
        raise ValueError(lib().exabm4d_last_error(None).decode())
    return idx, dist, cnt.value
