"""ctypes binding of libparseq_hip.so (C ABI: include/parseq_hip.h).

This is the only way compute reaches the GPU in this package.  If the library is missing or fails to load the import
of this module's `lib()` raises — there is deliberately no fallback (a silent eager/CPU path would void every parity
and performance claim).  Device memory, streams and the caching allocator are torch's: tensors are passed as raw
device pointers + the current HIP stream.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

from . import build as _build

PARSEQ_F32, PARSEQ_BF16, PARSEQ_U8, PARSEQ_BF16X3 = 0, 1, 2, 3
ARCH_PARSEQ, ARCH_VITSTR = 0, 1
FLAG_DECODE_AR, FLAG_TESTING, FLAG_LATENCY = 1, 2, 4
ABI_VERSION = 15
ORIENT_MAX_VIEWS = 8                                  # PARSEQ_ORIENT_MAX_VIEWS
ORIENT_CRITERIA = {'mean': 0, 'sum': 1}               # enum parseq_orient_criterion
LINE_MAX_WINDOWS, LINE_MAX_OUT = 64, 2048             # PARSEQ_LINE_MAX_WINDOWS, PARSEQ_LINE_MAX_OUT
SCORE_MAX_CANDIDATES, SCORE_MAX_ORDERS = 16, 16       # PARSEQ_SCORE_MAX_CANDIDATES, PARSEQ_SCORE_MAX_ORDERS
SCORE_MIX, SCORE_MEAN, SCORE_LENGTH_NORM = 0, 1, 2    # enum parseq_score_flags


class ParseqConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        'img_h', 'img_w', 'patch_h', 'patch_w', 'embed_dim', 'enc_depth', 'enc_heads', 'enc_mlp_ratio',
        'dec_depth', 'dec_heads', 'dec_mlp_ratio', 'num_tokens', 'max_label_length', 'bos_id', 'eos_id', 'pad_id')]
    _fields_ += [('enc_ln_eps', C.c_float), ('dec_ln_eps', C.c_float), ('arch', C.c_int32)]


class ImageDesc(C.Structure):
    _fields_ = [('data', C.c_void_p), ('height', C.c_int32), ('width', C.c_int32), ('row_stride', C.c_int64)]


class RotatedImageDesc(C.Structure):
    """parseq_rotated_image_desc: an image and the map of its rotation (parseq_amd/preprocess.py rotation_map fills it)."""
    _fields_ = [('data', C.c_void_p), ('height', C.c_int32), ('width', C.c_int32), ('row_stride', C.c_int64), ('mode', C.c_int32),
                ('rot_height', C.c_int32), ('rot_width', C.c_int32), ('a', C.c_int32 * 6)]


class RegionDesc(C.Structure):
    """parseq_region_desc: a source image's index, the rectified size and Pillow's PERSPECTIVE data (parseq_amd/preprocess.py quad_coeffs)."""
    _fields_ = [('image', C.c_int32), ('height', C.c_int32), ('width', C.c_int32), ('coef', C.c_double * 8)]


MESH_MAX_STRIPS = 64      # PARSEQ_MESH_MAX_STRIPS


class MeshStrip(C.Structure):
    """parseq_mesh_strip: the output columns x0 .. x1 - 1 of a region and the QUAD data Pillow derives for them (parseq_amd/preprocess.py polygon_mesh)."""
    _fields_ = [('x0', C.c_int32), ('x1', C.c_int32), ('coef', C.c_double * 8)]


class MeshRegionDesc(C.Structure):
    """parseq_mesh_region_desc: a source image's index, the rectified size and the region's run of strips in the call's strips array."""
    _fields_ = [('image', C.c_int32), ('height', C.c_int32), ('width', C.c_int32), ('first_strip', C.c_int32), ('n_strips', C.c_int32)]


class AugmentBlur(C.Structure):
    """arg.blur of PARSEQ_AUG_GAUSSIAN_BLUR: one box pass (parseq_amd/augment.py gaussian_box)."""
    _fields_ = [('r', C.c_int32), ('ww', C.c_uint32), ('fw', C.c_uint32)]


class AugmentNoise(C.Structure):
    """arg.noise of PARSEQ_AUG_POISSON_NOISE: exp(-lam), the Philox key, lam."""
    _fields_ = [('p0', C.c_double), ('seed', C.c_uint64), ('lam', C.c_int32)]


class AugmentArg(C.Union):
    _fields_ = [('table', C.c_uint8 * 256), ('factor', C.c_float), ('coef', C.c_double * 6), ('blur', AugmentBlur), ('noise', AugmentNoise)]


class AugmentOp(C.Structure):
    """parseq_augment_op: one operator of a chain (parseq_amd/augment.py fills it)."""
    _fields_ = [('op', C.c_int32), ('mode', C.c_int32), ('out_height', C.c_int32), ('out_width', C.c_int32), ('arg', AugmentArg)]


class AugmentDesc(C.Structure):
    """parseq_augment_desc: an image and its chain of at most three operators."""
    _fields_ = [('data', C.c_void_p), ('height', C.c_int32), ('width', C.c_int32), ('row_stride', C.c_int64), ('num_ops', C.c_int32),
                ('reserved', C.c_int32), ('ops', AugmentOp * 3)]


class BeamTrace(C.Structure):
    """parseq_beam_trace: four nullable device pointers parseq_forward_beam fills per step."""
    _fields_ = [('logits', C.c_void_p), ('tokens_in', C.c_void_p), ('parent', C.c_void_p), ('score', C.c_void_p)]


class BeamRefineTrace(C.Structure):
    """parseq_beam_refine_trace: two nullable device pointers parseq_forward_beam_refine fills per refinement iteration."""
    _fields_ = [('tokens_in', C.c_void_p), ('logits', C.c_void_p)]


class LexiconMatchArgs(C.Structure):
    """parseq_lexicon_match_args: the word table of a match (parseq_amd/lexicon.py) and what the call is asked for."""
    _fields_ = [('table', C.c_void_p), ('table_own', C.c_void_p), ('row_ids', C.c_void_p), ('ranges', C.c_void_p), ('fold', C.c_void_p),
                ('n_rows', C.c_int32), ('n', C.c_int32), ('rescore', C.c_int32), ('keep_reading', C.c_int32)]


class GemmOperand(C.Structure):
    _fields_ = [('data', C.c_void_p), ('dtype', C.c_int32), ('outer_stride', C.c_int64), ('k_stride', C.c_int64)]


class TrainGemmDesc(C.Structure):
    """parseq_train_gemm_desc: one call of the training step's sgemm() (parseq_op_train_gemm)."""
    _fields_ = [('A', GemmOperand), ('B', GemmOperand), ('M', C.c_int32), ('N', C.c_int32), ('K', C.c_int32), ('C', C.c_void_p), ('c16', C.c_void_p),
                ('bias', C.c_void_p), ('R', C.c_void_p), ('ldr', C.c_int64), ('rper', C.c_int32), ('alpha', C.c_float), ('accumulate', C.c_int32),
                ('asum', C.c_void_p), ('gelu_pre', C.c_void_p), ('gelu_pre16', C.c_void_p), ('gelu_out', C.c_void_p), ('gelu_out16', C.c_void_p),
                ('bf16_ops', C.c_int32), ('scratch', C.c_void_p), ('scratch_floats', C.c_size_t)]


class GemmRoute(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ('kernel', 'whole', 'splits', 'k_chunk', 'folded_asum', 'folded_gelu_pre', 'folded_gelu_out')]


# enum parseq_gemm_kernel, by value
GEMM_KERNELS = ('valu', 'mfma_f32', 'bf16_kk', 'bf16_kn', 'bf16_nk', 'bf16_nn', 'b16_kk', 'b16_kn', 'b16_nk', 'b16_nn', 'a16_nn', 'both16_k', 'both16_t')
# the split-bf16 kernels of the bf16x3 training mode (ABI 15), by their value in the same enum
GEMM_KERNELS_X3 = {13: 'x3_kk', 14: 'x3_kn', 15: 'x3_nk', 16: 'x3_nn'}


class TrainAttnDesc(C.Structure):
    """parseq_train_attn_desc: one call of the training step's train_attn() (parseq_op_train_attention_desc)."""
    _fields_ = [('q', C.c_void_p), ('q_bstride', C.c_int64), ('ldq', C.c_int32), ('k', C.c_void_p), ('v', C.c_void_p), ('ldkv', C.c_int32),
                ('qmask', C.c_void_p), ('kmask', C.c_void_p), ('ldkm', C.c_int32), ('o', C.c_void_p), ('ldo', C.c_int32),
                ('o16', C.c_void_p), ('dq16', C.c_void_p), ('dk16', C.c_void_p), ('dv16', C.c_void_p), ('d_o', C.c_void_p),
                ('dq', C.c_void_p), ('lddq', C.c_int32), ('dk', C.c_void_p), ('dv', C.c_void_p), ('lddkv', C.c_int32),
                ('kv_accumulate', C.c_int32), ('Lq', C.c_int32), ('Lk', C.c_int32), ('H', C.c_int32), ('scale', C.c_float),
                ('drop_site', C.c_uint32), ('pass_B', C.c_int32), ('qmask_pstride', C.c_int64), ('site_pstride', C.c_uint32),
                ('kv_shared', C.c_int32), ('pass_loop', C.c_int32), ('lse', C.c_void_p), ('dsum', C.c_void_p), ('head_dim', C.c_int32),
                ('bf16_ops', C.c_int32), ('dropout_p', C.c_float), ('seed', C.c_uint64)]


# enum parseq_train_attn_route, by value
TRAIN_ATTN_ROUTES = ('dec_bf16', 'enc_bf16', 'mfma', 'wide', 'hd32', 'hd64', 'none')


class NativeError(RuntimeError):
    """A libparseq_hip entry point returned a non-zero status."""


_LIB: Optional[C.CDLL] = None

# name: (restype, argtypes) — must list every symbol include/parseq_hip.h declares (tests/test_abi.py checks)
SIGNATURES = {
    'parseq_abi_version': (C.c_int, []),
    'parseq_last_error': (C.c_char_p, []),
    'parseq_model_create': (C.c_int, [C.POINTER(ParseqConfig), C.POINTER(C.c_void_p)]),
    'parseq_model_destroy': (None, [C.c_void_p]),
    'parseq_model_set_param': (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64, C.c_void_p]),
    'parseq_model_num_params': (C.c_int, [C.c_void_p]),
    'parseq_model_param_info': (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int64)]),
    'parseq_plan_create': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]),
    'parseq_plan_refresh': (C.c_int, [C.c_void_p, C.c_void_p]),
    'parseq_plan_create_ex': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    'parseq_plan_destroy': (None, [C.c_void_p]),
    'parseq_plan_workspace_bytes': (C.c_size_t, [C.c_void_p]),
    'parseq_resize_workspace_bytes': (C.c_size_t, [C.c_int]),
    'parseq_resize_bicubic': (C.c_int, [C.POINTER(ImageDesc), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    'parseq_rotate_resize_workspace_bytes': (C.c_size_t, [C.c_int]),
    'parseq_rotate_resize_bicubic': (C.c_int, [C.POINTER(RotatedImageDesc), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    'parseq_op_rotate': (C.c_int, [C.POINTER(RotatedImageDesc), C.c_void_p, C.c_void_p]),
    'parseq_augment_workspace_bytes': (C.c_size_t, [C.POINTER(AugmentDesc), C.c_int]),
    'parseq_augment_resize_bicubic': (C.c_int, [C.POINTER(AugmentDesc), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'parseq_op_augment': (C.c_int, [C.POINTER(AugmentDesc), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'parseq_rectify_workspace_bytes': (C.c_size_t, [C.POINTER(RegionDesc), C.c_int, C.c_int]),
    'parseq_rectify': (C.c_int, [C.POINTER(ImageDesc), C.c_int, C.POINTER(RegionDesc), C.c_int, C.POINTER(C.c_void_p), C.c_void_p, C.c_size_t, C.c_void_p]),
    'parseq_rectify_resize_bicubic': (C.c_int, [C.POINTER(ImageDesc), C.c_int, C.POINTER(RegionDesc), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                C.c_size_t, C.c_void_p]),
    'parseq_mesh_rectify_workspace_bytes': (C.c_size_t, [C.POINTER(MeshRegionDesc), C.c_int, C.POINTER(MeshStrip), C.c_int, C.c_int]),
    'parseq_mesh_rectify': (C.c_int, [C.POINTER(ImageDesc), C.c_int, C.POINTER(MeshRegionDesc), C.c_int, C.POINTER(MeshStrip), C.c_int, C.POINTER(C.c_void_p),
                                      C.c_void_p, C.c_size_t, C.c_void_p]),
    'parseq_mesh_rectify_resize_bicubic': (C.c_int, [C.POINTER(ImageDesc), C.c_int, C.POINTER(MeshRegionDesc), C.c_int, C.POINTER(MeshStrip), C.c_int, C.c_int,
                                                     C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'parseq_cross_entropy': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'parseq_postprocess': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'parseq_eval_metrics': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'parseq_eval_beams': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'parseq_eval_errors_accum_bytes': (C.c_size_t, [C.c_int]),
    'parseq_eval_errors': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'parseq_plan_set_profiling': (C.c_int, [C.c_void_p, C.c_int]),
    'parseq_plan_get_profile': (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    'parseq_encode': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    'parseq_forward': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                 C.POINTER(C.c_int), C.c_void_p]),
    'parseq_decode_hidden': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'parseq_decode_query': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p]),
    'parseq_decode_ex': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'parseq_set_memory': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    'parseq_beam_workspace_bytes': (C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    'parseq_forward_beam': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.POINTER(BeamTrace), C.c_void_p, C.c_size_t, C.c_void_p]),
    'parseq_op_beam_step': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    'parseq_beam_lexicon_workspace_bytes': (C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    'parseq_forward_beam_lexicon': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.POINTER(BeamTrace), C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    'parseq_op_beam_step_lexicon': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    'parseq_beam_refine_workspace_bytes': (C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]),
    'parseq_forward_beam_refine': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.POINTER(BeamTrace), C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                             C.c_int, C.c_int, C.c_void_p, C.POINTER(BeamRefineTrace)]),
    'parseq_op_beam_refine_workspace_bytes': (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    'parseq_op_beam_refine': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    'parseq_decode_attention': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'parseq_op_attention_geometry': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p]),
    'parseq_localize_workspace_bytes': (C.c_size_t, [C.c_void_p, C.c_int]),
    'parseq_localize': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'parseq_op_lexicon_match_workspace_bytes': (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    'parseq_op_lexicon_match': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                          C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'parseq_forward_lexicon_match_workspace_bytes': (C.c_size_t, [C.c_void_p, C.c_int, C.POINTER(LexiconMatchArgs)]),
    'parseq_forward_lexicon_match': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(LexiconMatchArgs), C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'parseq_op_orient_select_workspace_bytes': (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    'parseq_op_orient_select': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'parseq_forward_oriented_workspace_bytes': (C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    'parseq_forward_oriented': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'parseq_score_workspace_bytes': (C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]),
    'parseq_score': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'parseq_op_score_rows': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                       C.c_void_p]),
    'parseq_op_score_rank': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    'parseq_op_stitch_lines': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                         C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p]),
    'parseq_read_lines_workspace_bytes': (C.c_size_t, [C.c_void_p, C.c_int]),
    'parseq_read_lines': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'parseq_beam_automaton_workspace_bytes': (C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    'parseq_forward_beam_automaton': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.POINTER(BeamTrace), C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                                C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    'parseq_op_beam_step_automaton': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                                C.c_float, C.c_float, C.c_void_p, C.c_void_p]),
    'parseq_vitstr_forward': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    'parseq_decode_logits': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p]),
    'parseq_model_param_offset': (C.c_int64, [C.c_void_p, C.c_int]),
    'parseq_model_grad_elems': (C.c_int64, [C.c_void_p]),
    'parseq_model_set_train_precision': (C.c_int, [C.c_void_p, C.c_int]),
    'parseq_train_decoder_workspace_bytes': (C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    'parseq_train_decoder_workspace_offset': (C.c_int64, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_char_p]),
    'parseq_train_decoder': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                       C.c_int, C.c_float, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'parseq_train_encoder_workspace_bytes': (C.c_size_t, [C.c_void_p, C.c_int]),
    'parseq_train_encoder_forward': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'parseq_train_encoder_forward_ex': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'parseq_train_encoder_backward': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'parseq_train_vitstr_head_workspace_bytes': (C.c_size_t, [C.c_void_p, C.c_int, C.c_int]),
    'parseq_train_vitstr_head': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_size_t, C.c_void_p]),
    'parseq_train_grad_segments': (C.c_int, [C.c_void_p]),
    'parseq_train_grad_segment': (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_void_p)]),
    'parseq_stream_wait_event': (C.c_int, [C.c_void_p, C.c_void_p]),
    'parseq_shard_bounds': (C.c_int, [C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    'parseq_grad_norm': (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    'parseq_adamw_step': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_float, C.c_float, C.c_float,
                                    C.c_float, C.c_float, C.c_int, C.c_void_p, C.c_float, C.c_void_p]),
    'parseq_model_get_param': (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64, C.c_void_p]),
    'parseq_model_get_params': (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_void_p]),
    'parseq_weights_average': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    'parseq_op_weights_average': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]),
    'parseq_model_set_params': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    'parseq_op_layernorm': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                      C.c_float, C.c_void_p]),
    'parseq_op_linear': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                   C.c_int, C.c_void_p]),
    'parseq_op_ln_linear': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                      C.c_float, C.c_void_p]),
    'parseq_op_split_pack': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    'parseq_op_linear_cfg': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                       C.c_int, C.c_int, C.c_void_p]),
    'parseq_op_ln_linear_pairs': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                            C.c_float, C.c_void_p]),
    'parseq_op_ln_linear_gelu': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                           C.c_int, C.c_void_p]),
    'parseq_op_mlp': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    'parseq_op_mlp_variant': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    'parseq_op_attn_fused': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    'parseq_op_enc_blocks': (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    'parseq_op_enc_head_tail': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    'parseq_op_enc_blocks_x3': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_uint32), C.c_int, C.c_int, C.c_void_p,
                                         C.c_void_p, C.POINTER(C.c_uint32), C.c_void_p, C.c_void_p, C.c_void_p]),
    'parseq_op_enc_blocks_x3w': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_uint32), C.c_int, C.c_int, C.c_void_p,
                                          C.c_void_p, C.POINTER(C.c_uint32), C.c_void_p, C.c_void_p, C.c_void_p]),
    'parseq_op_encoder_attention': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                              C.c_void_p]),
    'parseq_op_cross_attention_ar24': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    'parseq_op_train_attention': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                            C.c_int, C.POINTER(C.c_int), C.c_void_p]),
    'parseq_op_train_attention_desc': (C.c_int, [C.POINTER(TrainAttnDesc), C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_void_p]),
    'parseq_op_train_gemm': (C.c_int, [C.POINTER(TrainGemmDesc), C.POINTER(GemmRoute), C.c_void_p]),
    'parseq_op_train_linear': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    'parseq_op_train_layernorm': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
}


def lib_path() -> str:
    return os.environ.get('PARSEQ_HIP_LIB', _build.LIB_PATH)


def lib() -> C.CDLL:
    """Load (once) and return the shared library.  Raises if it is not there: build it with
    `python -m parseq_amd.build` / `__graft_entry__.build()`."""
    global _LIB
    if _LIB is None:
        path = lib_path()
        if not os.path.exists(path):
            raise RuntimeError(
                f'libparseq_hip.so not found at {path}. The PARSeq HIP backend has no CPU/eager fallback; '
                f'build it first: python -m parseq_amd.build')
        handle = C.CDLL(path)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)      # AttributeError here = header/library mismatch: fail loudly
            fn.restype, fn.argtypes = res, args
        if handle.parseq_abi_version() != ABI_VERSION:
            raise RuntimeError(f'libparseq_hip ABI {handle.parseq_abi_version()} != binding ABI {ABI_VERSION}')
        _LIB = handle
    return _LIB


def check(status: int) -> None:
    if status != 0:
        msg = lib().parseq_last_error()
        raise NativeError(f'libparseq_hip error {status}: {msg.decode() if msg else "?"}')


ALLOC_FN = C.CFUNCTYPE(C.c_void_p, C.c_size_t, C.c_void_p)
RELEASE_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p)


class TorchPlanAllocator:
    """parseq_plan_create_ex's (alloc, release) pair on top of torch's caching allocator: a plan's arena is one uint8 tensor, alive until the library
    hands the block back (reference: every intermediate of strhub/models/parseq/model.py:86-169 is a caching-allocator block).  One instance serves any
    number of plans; `blocks` = {pointer: tensor} is what is out.  release() synchronises the device first: the caching allocator may hand the block
    to anyone the moment the tensor dies, and a plan's work may still be running on side streams (slots)."""

    def __init__(self, device):
        import torch
        self.device = torch.device(device)
        self.blocks = {}
        self.bytes_out = 0
        self.calls = 0
        self._alloc = ALLOC_FN(self._do_alloc)
        self._release = RELEASE_FN(self._do_release)

    def _do_alloc(self, nbytes, _user):
        import torch
        try:
            t = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
        except Exception:
            return None
        self.blocks[t.data_ptr()] = t
        self.bytes_out += int(nbytes)
        self.calls += 1
        return t.data_ptr()

    def _do_release(self, ptr, _user):
        import torch
        t = self.blocks.pop(ptr, None)
        if t is not None:
            torch.cuda.synchronize(self.device)
            self.bytes_out -= t.numel()

    @property
    def alloc_ptr(self):
        return C.cast(self._alloc, C.c_void_p)

    @property
    def release_ptr(self):
        return C.cast(self._release, C.c_void_p)


def stream_ptr(device=None) -> C.c_void_p:
    """The current HIP stream of `device` (a torch.device, a tensor, or None = the current device).  Entry points that take
    a model or a plan run on that object's device whatever device is current (the library switches and restores), so the
    stream handed over must be that device's stream — pass the model's device / the tensors' device, never rely on the
    thread's current device."""
    import torch
    if device is not None and hasattr(device, 'device'):
        device = device.device
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def guard(device):
    """Context manager making `device` (torch.device or tensor) current: for the raw-pointer entry points (parseq_op_*,
    parseq_postprocess, parseq_eval_metrics, parseq_eval_beams, parseq_eval_errors, parseq_resize_bicubic, parseq_rotate_resize_bicubic, parseq_augment_resize_bicubic, parseq_rectify, parseq_rectify_resize_bicubic, parseq_mesh_rectify, parseq_mesh_rectify_resize_bicubic, parseq_cross_entropy, parseq_grad_norm, parseq_op_weights_average), which launch on the current device."""
    import torch
    if hasattr(device, 'device'):
        device = device.device
    return torch.cuda.device(device)


def dtype_code(t) -> int:
    import torch
    if t == torch.float32:
        return PARSEQ_F32
    if t == torch.bfloat16:
        return PARSEQ_BF16
    if t == torch.uint8:
        return PARSEQ_U8
    raise TypeError(f'unsupported dtype {t}: libparseq_hip takes float32, bfloat16 or (images only) uint8')


def ptr(t) -> C.c_void_p:
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
