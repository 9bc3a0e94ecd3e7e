"""ctypes binding of ``csrc/libm2fnet_hip.so`` (C ABI: ``include/m2fnet_hip.h``).

PyTorch is used for plumbing only: device memory (tensors), the current HIP stream and, in ``dp.py``,
``torch.distributed`` (RCCL).  All arithmetic of the hot path happens in the HIP kernels behind this
binding.  There is NO fallback: if the shared library is missing or the device is not gfx950 the import /
first use raises.
"""
from __future__ import annotations

import ctypes
import math
import os
import struct
import subprocess
from typing import Dict, Optional, Tuple

import torch

from .layout import M2FConfig, attention_sites, param_specs

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_PATH = os.environ.get("M2F_LIB", os.path.join(CSRC, "libm2fnet_hip.so"))   # M2F_LIB: experiment builds only
HEADER_PATH = os.path.abspath(os.path.join(_HERE, "..", "include", "m2fnet_hip.h"))

F32, BF16 = 0, 1
PRECISIONS = {"fp32": F32, "f32": F32, "float32": F32, "bf16": BF16, "bfloat16": BF16}
(BUF_TEXT, BUF_AUDIO, BUF_KEYPAD, BUF_LABELS, BUF_CLASSW, BUF_LOGITS, BUF_LOSS, BUF_DLOGITS,
 BUF_FAM0_OUT, BUF_CU_SEQLENS, BUF_DTEXT, BUF_DAUDIO, BUF_STREAM_LEN, BUF_STREAM_ACTIVE, BUF_STREAM_NEW, BUF_STREAM_TABLE,
 BUF_TEACHER, BUF_DISTILL, BUF_STREAM_ATTN, BUF_SPEAKERS, BUF_STREAM_SPEAKERS, BUF_FOCAL, BUF_PARTNER, BUF_RDROP, BUF_SUPCON,
 BUF_FEATURES, BUF_AUX, BUF_AUX_LABELS, BUF_AUX_LOGITS) = range(29)
BUF_ADV, BUF_ADV_SKIP, BUF_ADV_DELTA_TEXT, BUF_ADV_DELTA_AUDIO = range(29, 33)      # a plan's adversarial state (m2f_plan_adversarial)
ADV_SITE_TEXT, ADV_SITE_AUDIO = 0xAD510001, 0xAD510002                             # hash sites of the perturbation's uniform start
ADV_NORMS = {"utterance": 0, "batch": 1}                                           # norm_kind of m2f_adv_ascend
IN_TEXT, IN_AUDIO = 1, 2            # input_mask bits of m2f_plan_backward_outputs

c_void_p, c_int, c_float, c_int64, c_uint32 = (ctypes.c_void_p, ctypes.c_int, ctypes.c_float,
                                                ctypes.c_int64, ctypes.c_uint32)


class M2FConfigC(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in (
        "audio_enabled", "text_enabled", "fam_enabled", "d_audio", "d_text", "d_fam",
        "nhead_audio", "nhead_text", "nhead_fam", "nlayers_audio", "nlayers_text", "nlayers_fam",
        "ntrans_audio", "ntrans_text", "cls_hidden", "cls_out", "cls_layers", "dim_ff")] + [
        ("dropout", ctypes.c_float), ("ln_eps", ctypes.c_float)]


def config_to_c(c: M2FConfig) -> M2FConfigC:
    return M2FConfigC(int(c.audio_enabled), int(c.text_enabled), int(c.fam_enabled), c.d_audio, c.d_text, c.d_fam,
                      c.nhead_audio, c.nhead_text, c.nhead_fam, c.nlayers_audio, c.nlayers_text, c.nlayers_fam,
                      c.ntrans_audio, c.ntrans_text, c.cls_hidden, c.cls_out, c.cls_layers, c.dim_ff,
                      float(c.dropout), float(c.ln_eps))


class AttnOptsC(ctypes.Structure):
    """m2f_attn_opts: the options of m2f_attention_fwd / m2f_attention_varlen_fwd.  A zero-filled one is a band of width zero: always
    set past / future (-1 = unlimited)."""
    _fields_ = [("past", c_int), ("future", c_int), ("bias_gain", c_float), ("n_same", c_int), ("n_other", c_int), ("speakers", c_void_p)]


class AttnStreamOptsC(ctypes.Structure):
    """m2f_attn_stream_opts: the options of m2f_attention_stream / m2f_attention_stream_chunk (zero-filled = none)."""
    _fields_ = [("table", c_void_p), ("table_cols", c_int), ("n_pages", c_int), ("page_rows", c_int), ("weights", c_void_p),
                ("bias_gain", c_float), ("n_same", c_int), ("n_other", c_int), ("spk_cache", c_void_p), ("spk_new", c_void_p)]


class HipError(RuntimeError):
    pass


# name -> (restype, argtypes); every symbol include/m2fnet_hip.h declares
SIGNATURES = {
    "m2f_last_error": (ctypes.c_char_p, []),
    "m2f_device_check": (c_int, []),
    "m2f_param_layout": (c_int, [ctypes.POINTER(M2FConfigC), ctypes.POINTER(c_int64), ctypes.POINTER(c_int64), c_int,
                                 ctypes.POINTER(c_int64)]),
    "m2f_workspace_bytes": (c_int64, [ctypes.POINTER(M2FConfigC), c_int, c_int, c_int]),
    "m2f_workspace_bytes_packed": (c_int64, [ctypes.POINTER(M2FConfigC), c_int, c_int, c_int, c_int]),
    "m2f_plan_create": (c_void_p, [ctypes.POINTER(M2FConfigC), c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                                   c_void_p, c_int64, c_void_p]),
    "m2f_plan_create_packed": (c_void_p, [ctypes.POINTER(M2FConfigC), c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                                          c_void_p, c_int64, c_void_p]),
    "m2f_param_shadow_elems": (c_int64, [ctypes.POINTER(M2FConfigC)]),
    "m2f_param_shadow_init": (c_int, [ctypes.POINTER(M2FConfigC), c_void_p, c_void_p]),
    "m2f_workspace_bytes_shared": (c_int64, [ctypes.POINTER(M2FConfigC), c_int, c_int, c_int, c_int]),
    "m2f_plan_create_shared": (c_void_p, [ctypes.POINTER(M2FConfigC), c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                                          c_void_p, c_int64, c_void_p, c_void_p]),
    "m2f_plan_params_fresh": (c_int, [c_void_p, c_int]),
    "m2f_adam_step_shadowed": (c_int, [ctypes.POINTER(M2FConfigC), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float,
                                       c_float, c_float, c_float, c_float, c_int, c_void_p, c_void_p]),
    "m2f_adam_step_shadowed_range": (c_int, [ctypes.POINTER(M2FConfigC), c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int64,
                                             c_int64, c_float, c_float, c_float, c_float, c_float, c_int, c_void_p, c_void_p]),
    "m2f_grad_norm_scratch_bytes": (c_int64, [ctypes.POINTER(M2FConfigC)]),
    "m2f_grad_sumsq": (c_int, [ctypes.POINTER(M2FConfigC), c_void_p, c_int, c_int64, c_int64, c_void_p, c_int, c_int, c_void_p]),
    "m2f_grad_norm_finalize": (c_int, [ctypes.POINTER(M2FConfigC), c_void_p, c_void_p, ctypes.c_double, c_void_p, c_void_p]),
    "m2f_sam_perturb": (c_int, [ctypes.POINTER(M2FConfigC), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                ctypes.c_double, c_void_p, c_void_p]),
    "m2f_sam_restore": (c_int, [ctypes.POINTER(M2FConfigC), c_void_p, c_void_p, c_void_p]),
    "m2f_adv_scratch_bytes": (c_int64, [c_int]),
    "m2f_adv_ascend": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "m2f_adv_init": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_float, c_void_p, c_uint32, c_void_p]),
    "m2f_plan_adversarial_bytes": (c_int64, [c_void_p, c_int]),
    "m2f_plan_adversarial": (c_int, [c_void_p, c_int, c_void_p, c_int64]),
    "m2f_plan_adv_begin": (c_int, [c_void_p, c_float, c_int, c_void_p]),
    "m2f_plan_adv_ascend": (c_int, [c_void_p, c_int, c_void_p]),
    "m2f_tensor_stats_scratch_bytes": (c_int64, [ctypes.POINTER(M2FConfigC), c_int]),
    "m2f_tensor_stats_record_bytes": (c_int64, [ctypes.POINTER(M2FConfigC), c_int]),
    "m2f_tensor_stats": (c_int, [ctypes.POINTER(M2FConfigC), c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                 c_void_p]),
    "m2f_tensor_stats_passes": (c_int, [ctypes.POINTER(M2FConfigC), c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int,
                                        c_int, c_int, c_void_p]),
    "m2f_eval_scratch_bytes": (c_int64, [c_int, c_int]),
    "m2f_eval_record_bytes": (c_int64, [c_int]),
    "m2f_eval_scores": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_void_p]),
    "m2f_eval_step": (c_int, [c_void_p, c_float, c_int, c_void_p, c_int, c_void_p]),
    "m2f_eval_scores_focal": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p]),
    "m2f_plan_skipped_copies": (c_int, [c_void_p]),
    "m2f_plan_destroy": (None, [c_void_p]),
    "m2f_plan_buffer": (c_void_p, [c_void_p, c_int]),
    "m2f_plan_num_launches": (c_int, [c_void_p, c_int]),
    "m2f_gemm_ring_launches": (ctypes.c_longlong, []),
    "m2f_gemm_last_form": (c_int, []),
    "m2f_gemm_form": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_uint32, ctypes.POINTER(c_int)]),
    "m2f_forward": (c_int, [c_void_p, c_void_p]),
    "m2f_loss": (c_int, [c_void_p, c_float, c_int, c_int, c_void_p]),
    "m2f_backward": (c_int, [c_void_p, c_void_p]),
    "m2f_step": (c_int, [c_void_p, c_float, c_int, c_int, c_int, c_void_p]),
    "m2f_plan_split_offset": (c_int64, [c_void_p]),
    "m2f_step_part": (c_int, [c_void_p, c_int, c_float, c_int, c_int, c_int, c_void_p]),
    "m2f_step_timed": (c_int, [c_void_p, c_float, c_int, c_int, c_void_p, c_int, ctypes.POINTER(c_int),
                               ctypes.POINTER(c_float), ctypes.POINTER(ctypes.c_double)]),
    "m2f_event_overhead": (c_int, [c_void_p, c_int, ctypes.POINTER(c_float), ctypes.POINTER(c_float), c_void_p]),
    "m2f_gather_dialogues": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p,
                                     c_int, c_void_p, c_void_p, c_void_p]),
    "m2f_rng_advance": (c_int, [c_void_p, c_void_p]),
    "m2f_adam_step": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_float, c_float, c_float, c_float,
                              c_float, c_int, c_void_p, c_void_p]),
    "m2f_adam_step_g16": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_float, c_float, c_float, c_float,
                              c_float, c_int, c_void_p, c_void_p]),
    "m2f_gemm": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int,
                         c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_float,
                         c_void_p, c_int, c_int, c_int, c_int, c_uint32, c_float, c_void_p, c_int, c_void_p, c_void_p,
                         c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p]),
    "m2f_attention_fwd": (c_int, [c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int,
                                  c_void_p, c_void_p, c_int, c_void_p, c_uint32, c_float, c_void_p, c_void_p, ctypes.POINTER(AttnOptsC)]),
    "m2f_attention_bwd": (c_int, [c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int,
                                  c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p,
                                  c_int, c_void_p, c_int, c_uint32, c_float, c_void_p, c_void_p, c_int, c_int]),
    "m2f_attention_opts_layout": (c_int, [c_int, ctypes.POINTER(c_int), c_int]),
    "m2f_attention_probs_elems": (c_int64, [c_int, c_int, c_int]),
    "m2f_attention_weights": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "m2f_plan_attention_sites": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int]),
    "m2f_plan_attention_weights": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "m2f_plan_attention_band": (c_int, [c_void_p, c_int, c_int]),
    "m2f_plan_get_attention_band": (c_int, [c_void_p, ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    "m2f_plan_attention_bias": (c_int, [c_void_p, c_float]),
    "m2f_plan_get_attention_bias": (c_int, [c_void_p, ctypes.POINTER(c_float)]),
    "m2f_plan_attention_speakers": (c_int, [c_void_p, c_int, c_int]),
    "m2f_plan_get_attention_speakers": (c_int, [c_void_p, ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    "m2f_plan_stream_speakers": (c_int, [c_void_p, c_void_p]),
    "m2f_stream_advance_speakers": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "m2f_stream_advance_speakers_n": (c_int, [c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "m2f_attention_speaker_class": (c_int, [c_int, c_int, c_int]),
    "m2f_stream_workspace_bytes": (c_int64, [ctypes.POINTER(M2FConfigC), c_int, c_int, c_int, c_int, c_int]),
    "m2f_plan_create_stream": (c_void_p, [ctypes.POINTER(M2FConfigC), c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int64, c_void_p]),
    "m2f_stream_step": (c_int, [c_void_p, c_int, c_void_p]),
    "m2f_stream_reset": (c_int, [c_void_p, c_void_p, c_void_p]),
    "m2f_stream_cache_bytes": (c_int64, [c_void_p]),
    "m2f_attention_stream_cache_elems": (c_int64, [c_int, c_int, c_int, c_int, c_int]),
    "m2f_attention_stream": (c_int, [c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int,
                                     c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, ctypes.POINTER(AttnStreamOptsC)]),
    "m2f_stream_attention_elems": (c_int64, [c_void_p]),
    "m2f_plan_stream_attention": (c_int, [c_void_p, c_void_p, c_int64]),
    "m2f_stream_attention": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "m2f_stream_paged_workspace_bytes": (c_int64, [ctypes.POINTER(M2FConfigC), c_int, c_int, c_int, c_int, c_int, c_int, c_int]),
    "m2f_plan_create_stream_paged": (c_void_p, [ctypes.POINTER(M2FConfigC), c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int64,
                                                c_void_p]),
    "m2f_attention_stream_pool_elems": (c_int64, [c_int, c_int, c_int, c_int, c_int]),
    "m2f_stream_snapshot_row_elems": (c_int64, [c_void_p]),
    "m2f_stream_snapshot_sites": (c_int, [c_void_p, c_void_p, c_void_p, c_int]),
    "m2f_stream_gather": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "m2f_stream_scatter": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "m2f_attention_stream_cache_gather": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                                  c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "m2f_attention_stream_cache_scatter": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                                   c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "m2f_stream_chunk_workspace_bytes": (c_int64, [c_void_p, c_int, c_int]),
    "m2f_plan_create_stream_chunk": (c_void_p, [c_void_p, c_int, c_void_p, c_void_p, c_int64, c_void_p]),
    "m2f_stream_prefill": (c_int, [c_void_p, c_int, c_void_p]),
    "m2f_attention_stream_chunk": (c_int, [c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p,
                                           c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, ctypes.POINTER(AttnStreamOptsC)]),
    "m2f_attention_varlen_fwd": (c_int, [c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int,
                                         c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_uint32, c_float, c_void_p, c_void_p,
                                         ctypes.POINTER(AttnOptsC)]),
    "m2f_attention_varlen_bwd": (c_int, [c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int,
                                         c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int,
                                         c_void_p, c_int, c_void_p, c_int, c_uint32, c_float, c_void_p, c_void_p, c_int, c_int]),
    "m2f_set_shadow_map": (c_int, [c_void_p, c_void_p, c_int64]),
    "m2f_plan_grad_bf16": (c_int, [c_void_p, c_void_p]),
    "m2f_plan_accumulate_grads": (c_int, [c_void_p, c_int]),
    "m2f_plan_distill": (c_int, [c_void_p, c_int]),
    "m2f_plan_focal": (c_int, [c_void_p, c_int]),
    "m2f_plan_rdrop": (c_int, [c_void_p, c_int]),
    "m2f_plan_supcon": (c_int, [c_void_p, c_int]),
    "m2f_plan_crf": (c_int, [c_void_p, c_void_p, c_void_p]),
    "m2f_plan_aux_head": (c_int, [c_void_p, c_void_p, c_void_p, c_int]),
    "m2f_plan_stream_crf": (c_int, [c_void_p, c_void_p, c_void_p]),
    "m2f_plan_backward_outputs": (c_int, [c_void_p, c_int, c_int]),
    "m2f_plan_fused_adam_setup": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "m2f_plan_fused_adam": (c_int, [c_void_p, c_int]),
    "m2f_adam_hyper": (c_int, [c_void_p, c_float, c_float, c_float, c_float, c_float, c_int, c_void_p]),
    "m2f_adam_hyper_groups": (c_int, [c_void_p, c_void_p, c_int, c_void_p]),
    "m2f_adam_step_grouped": (c_int, [ctypes.POINTER(M2FConfigC), c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                      c_void_p, c_int64, c_int64, c_void_p, c_void_p]),
    "m2f_adam_step_ema": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_float, c_float, c_float, c_float,
                                  c_float, c_int, c_float, c_void_p, c_void_p]),
    "m2f_adam_step_g16_ema": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_float, c_float, c_float, c_float,
                                      c_float, c_int, c_float, c_void_p, c_void_p]),
    "m2f_adam_step_shadowed_range_ema": (c_int, [ctypes.POINTER(M2FConfigC), c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                                 c_float, c_int64, c_int64, c_float, c_float, c_float, c_float, c_float, c_int, c_void_p,
                                                 c_void_p]),
    "m2f_adam_step_grouped_ema": (c_int, [ctypes.POINTER(M2FConfigC), c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_float,
                                          c_void_p, c_int, c_void_p, c_int64, c_int64, c_void_p, c_void_p]),
    "m2f_ema_exchange": (c_int, [ctypes.POINTER(M2FConfigC), c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "m2f_plan_fused_adam_setup_grouped": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "m2f_gemm_p8": (c_int, [c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int,
                            c_int, c_int, c_int, c_void_p, c_void_p, c_int64, c_int, c_void_p]),
    "m2f_gemm_fp8": (c_int, [c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_float, c_void_p, c_int, c_void_p, c_void_p,
                             c_int, c_int, c_void_p, c_float, c_void_p]),
    "m2f_quantize_fp8": (c_int, [c_void_p, c_void_p, c_int64, c_float, c_void_p]),
    "m2f_embed_layernorm": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_float, c_void_p, c_int, c_void_p]),
    "m2f_attention_long_fwd_bf16": (c_int, [c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int,
                                            c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "m2f_attention_long_fwd_bf16_out8": (c_int, [c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int,
                                                 c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_int, c_void_p]),
    "m2f_layernorm_fwd_out8": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_float,
                                       c_void_p]),
    "m2f_layernorm_fwd_diag": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_int, c_void_p]),
    "m2f_set_shadow_only": (c_int, [c_int]),
    "m2f_attention_long_fwd": (c_int, [c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int,
                                       c_void_p, c_void_p, c_int, c_void_p]),
    "m2f_layernorm_fwd": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float,
                                  c_void_p]),
    "m2f_layernorm_bwd": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                  c_void_p, c_void_p, c_void_p]),
    "m2f_layernorm_fwd_drop": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_uint32,
                                       c_float, c_void_p, c_void_p]),
    "m2f_layernorm_bwd_masked": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                         c_void_p, c_void_p, c_void_p, c_uint32, c_float, c_void_p, c_void_p]),
    "m2f_dropout_rows": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_uint32, c_uint32, c_float, c_void_p, c_void_p]),
    "m2f_cross_entropy": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, c_float, c_int, c_void_p, c_void_p,
                                  c_void_p, c_void_p]),
    "m2f_cross_entropy_distill": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_int, c_void_p,
                                          c_void_p, c_void_p, c_void_p]),
    "m2f_cross_entropy_focal": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_int,
                                        c_void_p, c_void_p, c_void_p, c_void_p]),
    "m2f_crf_scratch_floats": (c_int64, [c_int, c_int, c_int]),
    "m2f_crf_nll": (c_int, [c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                            c_void_p, c_void_p, c_void_p]),
    "m2f_crf_viterbi": (c_int, [c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                c_void_p]),
    "m2f_crf_filter": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "m2f_cross_entropy_rdrop": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_int, c_void_p,
                                        c_void_p, c_void_p, c_void_p]),
    "m2f_supcon_scratch_floats": (c_int64, [c_int, c_int]),
    "m2f_supcon": (c_int, [c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                           c_void_p]),
    "m2f_aux_head_scratch_floats": (c_int64, [c_int, c_int, c_int]),
    "m2f_aux_head": (c_int, [c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                             c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "m2f_aux_head_forward": (c_int, [c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "m2f_aux_head_backward": (c_int, [c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                      c_void_p]),
    "m2f_aux_head_join": (c_int, [c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                  c_float, c_int, c_void_p, c_void_p]),
    "m2f_w2v_conv0": (c_int, [c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_float,
                              c_void_p, c_void_p, c_void_p, c_void_p]),
    "m2f_w2v_conv0_scratch_floats": (c_int64, [c_int, c_int, c_int]),
    "m2f_w2v_feat_layernorm": (c_int, [c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_void_p]),
    "m2f_w2v_pos_conv": (c_int, [c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "m2f_w2v_masked_mean": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "m2f_mel_frontend": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "m2f_mel_frontend_scratch_floats": (c_int64, [c_int]),
    "m2f_mel_stem": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "m2f_mel_conv": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                             c_int, c_int, c_int, c_void_p]),
    "m2f_mel_head": (c_int, [c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p,
                             c_void_p]),
}

_lib = None


def build_library(force: bool = False) -> str:
    """Compile the HIP sources for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    if force:
        subprocess.run(["make", "-C", CSRC, "clean"], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", CSRC, "-j4"], check=True, stdout=subprocess.DEVNULL)
    return LIB_PATH


def lib() -> ctypes.CDLL:
    """The loaded shared library; raises (never falls back) if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} not found: the HIP extension is required (no CPU/PyTorch fallback exists). "
                f"Build it with `make -C {CSRC}` or `python -c 'import __graft_entry__ as g; g.build()'`.")
        l = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(l, name)          # AttributeError if the library does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


def check(code: int, what: str = "") -> None:
    if code != 0:
        raise HipError(f"{what}: {lib().m2f_last_error().decode()} (code {code})")


def require_gpu() -> None:
    if not torch.cuda.is_available():
        raise HipError("the M2FNet HIP path needs an MI355X (gfx950) GPU; there is no CPU fallback")
    check(lib().m2f_device_check(), "m2f_device_check")


def stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def context_band(past, future) -> Tuple[int, int]:
    """The two integers of a context band as the C entries take them: each side None (unlimited, -1) or an integer >= 0 - how many
    utterances before (past) / after (future) its own an utterance attends to.  (None, 0) is causal attention."""
    out = []
    for name, v in (("past", past), ("future", future)):
        if v is None:
            out.append(-1)
            continue
        if isinstance(v, bool) or not isinstance(v, int) or v < 0:
            raise ValueError(f"context band: {name} must be None (unlimited) or an integer >= 0, got {v!r}")
        out.append(v)
    return out[0], out[1]


def position_bias(gain) -> float:
    """The gain of the distance-decay attention bias (ALiBi: a visible key's score gets ``-slope(h, H, gain) * |i - j|``,
    ``functional.position_bias_slopes``) as the kernels APPLY it: None -> 0.0 (off); a finite number >= 0 -> that number rounded to
    bf16, round to nearest even (the launch descriptors hold 16 bits of it; 1.0, 0.5, 2.0 are exact); anything else raises ValueError."""
    if gain is None:
        return 0.0
    if isinstance(gain, bool) or not isinstance(gain, (int, float)):
        raise ValueError(f"position bias: the gain must be None (off) or a finite number >= 0, got {gain!r}")
    g = float(gain)
    if not math.isfinite(g) or g < 0.0:
        raise ValueError(f"position bias: the gain must be None (off) or a finite number >= 0, got {gain!r}")
    try:
        u = struct.unpack("<I", struct.pack("<f", g))[0]
    except OverflowError:
        raise ValueError(f"position bias: the gain {gain!r} is out of range") from None
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    out = struct.unpack("<f", struct.pack("<I", u & 0xFFFFFFFF))[0]
    if not math.isfinite(out):
        raise ValueError(f"position bias: the gain {gain!r} is out of range")
    return out


def speaker_heads(setting, heads=None) -> Optional[Tuple[int, int]]:
    """The speaker-head setting ``(n_same, n_other)`` as the kernels take it: None -> None (off); a pair of integers >= 0, at least one
    of them positive -> the pair.  At a site with H heads, heads 0 .. n_same - 1 are SAME-speaker heads (query utterance i sees key j
    only if their speakers are equal - the utterance itself always qualifies), heads n_same .. n_same + n_other - 1 OTHER-speaker
    heads (only if they differ), the rest are untouched (`speaker_head_class`).  heads: optional ``{site name: H}`` - the sum must fit
    every site, else ValueError naming the site.  Anything else raises ValueError."""
    if setting is None:
        return None
    try:
        a, b = setting
    except (TypeError, ValueError):
        raise ValueError(f"speaker heads: the setting must be None (off) or a pair (n_same, n_other), got {setting!r}") from None
    for v in (a, b):
        if isinstance(v, bool) or not isinstance(v, int) or v < 0:
            raise ValueError(f"speaker heads: n_same and n_other must be integers >= 0, got {setting!r}")
    if a + b == 0:
        raise ValueError("speaker heads: at least one of n_same and n_other must be positive (None switches the heads off)")
    for name, H in (heads or {}).items():
        if a + b > H:
            raise ValueError(f"speaker heads: n_same + n_other = {a + b} exceeds the {H} heads of {name}")
    return int(a), int(b)


FOCAL_GAMMA_MAX = 8.0


def check_focal_gamma(gamma, name: str = "focal_gamma", who: str = "train_step") -> float:
    """gamma of the focal criterion as a float; ValueError naming the argument unless it is a finite number in [0, 8].  A host function:
    no GPU needed."""
    if isinstance(gamma, bool) or not isinstance(gamma, (int, float)):
        raise ValueError(f"{who}: {name} must be a number in [0, {FOCAL_GAMMA_MAX:g}], got {gamma!r}")
    if not (math.isfinite(gamma) and 0.0 <= gamma <= FOCAL_GAMMA_MAX):
        raise ValueError(f"{who}: {name} must be a finite number in [0, {FOCAL_GAMMA_MAX:g}], got {gamma!r}")
    return float(gamma)


def check_rdrop_alpha(alpha, name: str = "rdrop", who: str = "train_step") -> float:
    """alpha of the R-Drop criterion as a float; ValueError naming the argument unless it is a finite number >= 0.  A host function:
    no GPU needed."""
    if isinstance(alpha, bool) or not isinstance(alpha, (int, float)):
        raise ValueError(f"{who}: {name} must be a finite number >= 0, got {alpha!r}")
    if not (math.isfinite(alpha) and alpha >= 0.0):
        raise ValueError(f"{who}: {name} must be a finite number >= 0, got {alpha!r}")
    return float(alpha)


def check_supcon_pair(supcon, name: str = "supcon", who: str = "train_step") -> Tuple[float, float]:
    """(weight, temperature) of the supervised contrastive criterion as floats; ValueError naming the argument unless it is a pair of
    numbers with weight finite and >= 0 and temperature finite and > 0.  A host function: no GPU needed."""
    if not isinstance(supcon, (tuple, list)) or len(supcon) != 2:
        raise ValueError(f"{who}: {name} must be a pair (weight, temperature), got {supcon!r}")
    w, t = supcon
    for v in (w, t):
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise ValueError(f"{who}: {name} must be a pair of numbers (weight, temperature), got {supcon!r}")
    if not (math.isfinite(w) and w >= 0.0):
        raise ValueError(f"{who}: {name} weight must be a finite number >= 0, got {w!r}")
    if not (math.isfinite(t) and t > 0.0):
        raise ValueError(f"{who}: {name} temperature must be a finite number > 0, got {t!r}")
    return float(w), float(t)


def check_adv_hyper(epsilon, step_size=None, init_mag=0.0, who: str = "adversarial_step") -> Tuple[float, float, float]:
    """(epsilon, step_size, init_mag) of the adversarial ascent as floats: each a finite number >= 0 (bool, NaN, inf, negative or
    anything that is no number: ValueError naming it); step_size None = epsilon."""
    out = []
    for name, v in (("epsilon", epsilon), ("step_size", epsilon if step_size is None else step_size), ("init_mag", init_mag)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
            raise ValueError(f"{who}: {name} must be a finite number >= 0, got {v!r}")
        out.append(float(v))
    return tuple(out)


def adv_norm_kind(norm, who: str = "adversarial_step") -> int:
    """norm_kind of m2f_adv_ascend for "utterance" (the row's L2 norm) or "batch" (the L2 norm over all valid rows of the modality)."""
    if not isinstance(norm, str) or norm not in ADV_NORMS:
        raise ValueError(f"{who}: unknown norm {norm!r}; one of {sorted(ADV_NORMS)}")
    return ADV_NORMS[norm]


def input_modalities(names, text_enabled: bool, audio_enabled: bool, who: str, what: str = "input_grads") -> int:
    """The IN_TEXT | IN_AUDIO mask of a subset of ("text", "audio") (a name, or an iterable of names; None: every enabled modality).
    An unknown name, an empty subset and a modality the model has disabled are ValueErrors naming it."""
    enabled = {"text": text_enabled, "audio": audio_enabled}
    if names is None:
        names = [n for n, on in enabled.items() if on]
    if isinstance(names, str):
        names = (names,)
    try:
        names = list(names)
    except TypeError:
        raise ValueError(f"{who}: {what} must be a subset of ('text', 'audio'), got {names!r}") from None
    mask = 0
    for n in names:
        if n not in enabled:
            raise ValueError(f"{who}: {what} names {n!r}; a subset of ('text', 'audio') is expected")
        if not enabled[n]:
            raise ValueError(f"{who}: {what} names {n!r}, but the {n} modality of this model is disabled")
        mask |= IN_TEXT if n == "text" else IN_AUDIO
    if not mask:
        raise ValueError(f"{who}: {what} is empty; name 'text', 'audio' or both (None: no input gradient)")
    return mask


def rdrop_partner(pairs: int, l: int, T: int, L: Optional[int] = None, dst: Optional[torch.Tensor] = None,
                  valid: Optional[torch.Tensor] = None, device=None) -> torch.Tensor:
    """The twin map of the R-Drop criterion (M2F_BUF_PARTNER): int32 [T], for every token row of a plan the row of the same utterance
    in the other view, or -1.  The plan runs `2 * pairs` dialogues of `l` slots - view 0 and behind it view 1 -, so the twin of slot
    (b, i) is slot ((b + pairs) mod (2 * pairs), i).
    Padded and bucketed plans (`L`: the plan's row length, L >= l): slot (b, i) is token row b * L + i; the filler rows of a bucketed
    plan (dialogues past 2 * pairs, slots past l) get -1.
    Packed plans (`dst`, `valid` [2 * pairs, l]: the row map `Plan.set_inputs` placed the batch with, and which slots are real): the twin
    of row dst[b, i] is row dst[(b + pairs) mod (2 * pairs), i]; pad slots, filler dialogues' rows and the spare row get -1.
    Pure torch on `device` (or dst's), no host synchronisation: it runs on the CPU as it runs in the step."""
    n = 2 * int(pairs)
    if dst is not None:
        if dst.shape != (n, l) or valid is None or valid.shape != dst.shape:
            raise ValueError(f"rdrop_partner: dst and valid must be [{n}, {l}] (got {tuple(dst.shape)})")
        # (valid is the same in both views, so a real slot's twin is real; every pad slot writes -1 into the row it was sent to)
        twin = torch.where(valid, torch.roll(dst, int(pairs), 0), torch.full_like(dst, -1)).to(torch.int32)
        out = torch.full((T,), -1, dtype=torch.int32, device=dst.device)
        return out.index_copy_(0, dst.reshape(-1), twin.reshape(-1))
    if L is None or L < l or n * L > T:
        raise ValueError(f"rdrop_partner: a padded plan needs its row length L >= {l} and T >= {n} * L (got L = {L}, T = {T})")
    rows = torch.arange(n, device=device)[:, None] * L + torch.arange(l, device=device)[None, :]
    out = torch.full((T,), -1, dtype=torch.int32, device=device)
    out[rows.reshape(-1)] = torch.roll(rows, int(pairs), 0).reshape(-1).to(torch.int32)
    return out


def criterion_transition(held: dict, wanted: dict) -> list:
    """The single-switch calls that take a plan's criterion from `held` to `wanted`, as [(switch, value)]: both map the switches that
    are on - "distill", "focal", "rdrop", "supcon" to True, "crf" and "aux" to the key of their buffers - and a value of None switches
    off.  Every switch held and not wanted goes off FIRST, then every wanted switch that is not held (or held under another key) goes
    on: whatever the two states, no call meets a switch it is refused beside (csrc/plan.hip, exclusions[]), since `wanted` combines.
    Nothing for equal states.  A host function: no GPU needed."""
    return [(sw, None) for sw in held if sw not in wanted] + [(sw, v) for sw, v in wanted.items() if held.get(sw) != v]


SPK_NONE, SPK_SAME, SPK_OTHER = 0, 1, 2


def speaker_head_class(h: int, n_same: int, n_other: int) -> int:
    """The class of head h under (n_same, n_other): SPK_SAME, SPK_OTHER or SPK_NONE, as the LIBRARY states it (csrc/ops.h,
    m2f_attn_speaker_class - the one definition every kernel calls).  A host function: no GPU needed."""
    return int(lib().m2f_attention_speaker_class(int(h), int(n_same), int(n_other)))


def speaker_ids(speakers, who: str = "speakers") -> "torch.Tensor":
    """One speaker id per utterance as the kernels read it: a uint8 tensor of the same shape.  uint8 / int32 / int64 tensors are
    accepted; values are 0 .. 255 and only equality is used; a value outside that range raises ValueError (one host sync for the wider
    types).  Values in pad slots are ignored by every kernel."""
    if not isinstance(speakers, torch.Tensor) or speakers.dtype not in (torch.uint8, torch.int32, torch.int64):
        raise ValueError(f"{who}: a uint8 / int32 / int64 tensor of speaker ids is required, got "
                         f"{getattr(speakers, 'dtype', type(speakers).__name__)}")
    if speakers.dtype == torch.uint8:
        return speakers
    if speakers.numel():
        lo, hi = int(speakers.min()), int(speakers.max())
        if lo < 0 or hi > 255:
            raise ValueError(f"{who}: speaker ids must be 0 .. 255, got values in [{lo}, {hi}]")
    return speakers.to(torch.uint8)


def c_param_layout(c: M2FConfig) -> Tuple[list, list, int]:
    cc = config_to_c(c)
    n_max = 4096
    offs = (c_int64 * n_max)()
    nums = (c_int64 * n_max)()
    total = c_int64(0)
    n = lib().m2f_param_layout(ctypes.byref(cc), offs, nums, n_max, ctypes.byref(total))
    if n < 0:
        raise HipError(lib().m2f_last_error().decode())
    return list(offs[:n]), list(nums[:n]), int(total.value)


def verify_layout(c: M2FConfig) -> int:
    """Cross-check layout.py against the C side; returns the flat length in elements."""
    specs, total = param_specs(c)
    uniq = [s for s in specs if not s.alias_of]
    offs, nums, ctotal = c_param_layout(c)
    if ctotal != total or offs != [s.offset for s in uniq] or nums != [s.numel for s in uniq]:
        raise HipError("flat parameter layout mismatch between layout.py and csrc/plan.hip")
    return total


class Plan:
    """One bound launch list (config, B, L, precision, train/eval) + its workspace."""

    def __init__(self, cfg: M2FConfig, B: int, L: int, precision: int, train: bool, params: torch.Tensor,
                 grads: Optional[torch.Tensor], rng_state: Optional[torch.Tensor], T: Optional[int] = None,
                 param_shadow: Optional[torch.Tensor] = None):
        """T: PACKED plan (m2f_plan_create_packed) - T token rows shared by the B dialogues through cu_seqlens; `set_inputs`
        packs the padded batch it is given and `logits` unpacks, so callers see the padded [B, L, ...] surface either way.
        param_shadow: the model's shared bf16 parameter-shadow buffer (m2f_plan_create_shared); None = the plan keeps its own."""
        require_gpu()
        self.packed = T is not None
        self.cfg, self.B, self.L, self.T = cfg, B, L, (int(T) if self.packed else B * L)
        self.precision, self.train = precision, train
        self._cc = config_to_c(cfg)
        self.shared_shadow = param_shadow is not None
        self._fresh = False
        self._on_cast = None      # engine hook: a forward that re-cast the shared parameter shadows leaves them current
        if self.shared_shadow:
            nbytes = lib().m2f_workspace_bytes_shared(ctypes.byref(self._cc), B, L, self.T if self.packed else 0, int(train))
        else:
            nbytes = (lib().m2f_workspace_bytes_packed(ctypes.byref(self._cc), B, L, self.T, int(train)) if self.packed
                      else lib().m2f_workspace_bytes(ctypes.byref(self._cc), B, L, int(train)))
        if nbytes < 0:
            raise HipError(lib().m2f_last_error().decode())
        self.workspace = torch.zeros(nbytes + 256, dtype=torch.uint8, device=params.device)
        # the zero-fill runs on torch's current stream, m2f_plan_create uploads its tables with blocking copies on the
        # null stream: order the two whatever stream context the caller is in
        torch.cuda.current_stream(params.device).synchronize()
        base = self.workspace.data_ptr()
        self._ws_off = (-base) % 256
        self._keep = (params, grads, rng_state, param_shadow)
        if self.shared_shadow:
            self.handle = lib().m2f_plan_create_shared(ctypes.byref(self._cc), B, L, self.T if self.packed else 0, precision,
                                                       int(train), params.data_ptr(), ptr(grads), base + self._ws_off, nbytes,
                                                       ptr(rng_state), param_shadow.data_ptr())
        elif self.packed:
            self.handle = lib().m2f_plan_create_packed(ctypes.byref(self._cc), B, L, self.T, precision, int(train),
                                                       params.data_ptr(), ptr(grads), base + self._ws_off, nbytes, ptr(rng_state))
        else:
            self.handle = lib().m2f_plan_create(ctypes.byref(self._cc), B, L, precision, int(train), params.data_ptr(),
                                                ptr(grads), base + self._ws_off, nbytes, ptr(rng_state))
        if not self.handle:
            raise HipError("m2f_plan_create: " + lib().m2f_last_error().decode())
        C = cfg.cls_out
        pad8 = lambda w: (w + 7) // 8 * 8          # every activation row is padded to a multiple of 8 floats
        self.text_in = self._view(BUF_TEXT, (self.T, pad8(max(cfg.d_text, 1))), torch.float32)[:, : max(cfg.d_text, 1)]
        self.audio_in = self._view(BUF_AUDIO, (self.T, pad8(max(cfg.d_audio, 1))), torch.float32)[:, : max(cfg.d_audio, 1)]
        self.keypad_in = self._view(BUF_KEYPAD, (self.T,), torch.uint8)
        self.labels_in = self._view(BUF_LABELS, (self.T,), torch.int64)
        self.class_w = self._view(BUF_CLASSW, (16,), torch.float32)
        self._logits = self._view(BUF_LOGITS, (self.T, C) if self.packed else (B, L, C), torch.float32)
        self.cu_in = self._view(BUF_CU_SEQLENS, (B + 1,), torch.int32)
        self.speakers_in = self._view(BUF_SPEAKERS, (self.T,), torch.uint8)      # speaker heads: one id per token row, in the rows' order
        self._dst = self._valid = None        # packed plans: token row of every (dialogue, slot) of the last batch; its validity
        self._spare = None                    # packed plans of B * L rows: device flag "row T-1 is not owned by the last batch"
        # input gradients (train plans; m2f_plan_backward_outputs): d loss / d text, d loss / d audio in the token rows of text_in / audio_in
        self._dtext = (self._view(BUF_DTEXT, (self.T, pad8(cfg.d_text)), torch.float32)[:, : cfg.d_text]
                       if train and cfg.text_enabled else None)
        self._daudio = (self._view(BUF_DAUDIO, (self.T, pad8(cfg.d_audio)), torch.float32)[:, : cfg.d_audio]
                        if train and cfg.audio_enabled else None)
        self.input_mask, self.param_grads = 0, bool(train and grads is not None)
        if train and grads is not None:
            # (loss, den, num) live in the tail of the flat gradient buffer (see include/m2fnet_hip.h)
            assert grads.numel() >= params.numel() + 4, "gradient buffer needs a 64-float tail"
            self.loss = grads[params.numel(): params.numel() + 4]
            assert self.loss.data_ptr() == lib().m2f_plan_buffer(self.handle, BUF_LOSS)
        else:
            self.loss = self._view(BUF_LOSS, (4,), torch.float32)
        self._dlogits = self._view(BUF_DLOGITS, (self.T, C) if self.packed else (B, L, C), torch.float32)
        # The criterion (`set_criterion`).  held: the switches that are on - "distill", "focal", "rdrop", "supcon": True; "crf", "aux": the
        # key of their buffers - as the C side holds them; uploaded: per hyper-parameter buffer, what was last copied into it
        self.held, self.uploaded, self._block_refs = {}, {}, {}
        # inputs of the distillation criterion (train plans with a gradient buffer): the teacher's logits in the token rows of the plan's
        # own logits, and the (alpha, temperature) pair the criterion kernel reads on the device
        self._teacher = self._view(BUF_TEACHER, (self.T, C) if self.packed else (B, L, C), torch.float32) if train else None
        self.distill_hyper = self._view(BUF_DISTILL, (2,), torch.float32) if train else None
        # gamma of the focal criterion (train and eval plans): the float the criterion and eval-rows kernels read on the device
        self.focal_gamma = self._view(BUF_FOCAL, (1,), torch.float32)
        # inputs of the R-Drop criterion (train plans): the twin of every token row and the alpha the kernel reads on the device
        self.partner_in = self._view(BUF_PARTNER, (self.T,), torch.int32) if train else None
        self.rdrop_alpha = self._view(BUF_RDROP, (1,), torch.float32) if train else None
        self._partner_key = None              # what the padded twin map in partner_in was built for: (pairs, l); packed plans: never kept
        # the supervised contrastive criterion (train plans): the (weight, temperature) pair its kernels read on the device
        self.supcon_hyper = self._view(BUF_SUPCON, (2,), torch.float32) if train else None
        # the auxiliary label head (train plans): the (weight, label smoothing) pair its kernels read on the device, the second label of
        # every token row (placed as labels_in is) and the head's logits of the last step
        self.aux_hyper = self._view(BUF_AUX, (2,), torch.float32) if train else None
        self.aux_labels_in = self._view(BUF_AUX_LABELS, (self.T,), torch.int64) if train else None
        self._aux_logits = self._view(BUF_AUX_LOGITS, (self.T, 16) if self.packed else (B, L, 16), torch.float32) if train else None
        # the classifier's last hidden activation as stored, in the plan's token rows (what `supcon` contrasts; `features`)
        hid = cfg.cls_hidden
        self._features = self._view(BUF_FEATURES, (self.T, pad8(hid)) if self.packed else (B, L, pad8(hid)), torch.float32)[..., :hid]
        self._fam0_out = (self._view(BUF_FAM0_OUT, (self.T, pad8(cfg.d_fam)) if self.packed else (B, L, pad8(cfg.d_fam)),
                                     torch.float32)[..., : cfg.d_fam] if cfg.fam_enabled else None)
        # shape of the batch last handed to set_inputs: a plan may be larger than the batch it runs (shape buckets), the
        # result views below are cut to the batch
        self.in_B, self.in_L = B, L
        self.version = 0          # bumped by every forward; backward checks it still owns the activations
        self._pending = None      # weak reference to the autograd node whose backward still needs this plan's activations
        # the adversarial state (`adversarial`): the caller-side buffer the C side points into, the modalities it covers, its views
        self._adv_state, self.adv_mask = None, 0
        self.adv_hyper = self.adv_skip = None
        self.adv_delta = {}
        self._acc = False         # the accumulate form is on (accumulate_grads); it stays on across a rebuild, as the C side keeps it
        self._disarm()

    def _disarm(self) -> None:
        """What the optimizer and the engine armed on this plan, as the C side holds it after create and after a rebuild (backward_outputs):
        nothing.  The fused optimizer (optim.FusedAdam.prepare_fused) and the bf16 gradients (model._Engine._arm_grad_bf16) set up again."""
        self._fused_key = None        # the optimizer buffers the in-launch Adam form was set up with (None: not armed)
        self._fused_refs = None       # ... kept alive: the plan holds raw pointers
        self._fused_err = None        # ... the last refused setup's message,
        self._fused_bad = False       # ... for good (ungrouped optimizer: another table form, ...),
        self._fused_bad_key = None    # ... or for this key (grouped optimizer)
        self._g16_ref = None          # the bf16 gradient buffer the steps fill (None: fp32 gradients)
        self._g16_bad = False         # ... this plan cannot (fp32 mode, another table form)

    def _unpack(self, rows: torch.Tensor) -> torch.Tensor:
        """[T, C] rows of a packed plan -> the padded [b, l, C] surface of the last batch (pad slots = 0)."""
        return rows[self._dst] * self._valid[..., None].to(rows.dtype)

    @property
    def logits(self) -> torch.Tensor:
        if self.packed:
            return self._unpack(self._logits)
        return self._logits[: self.in_B, : self.in_L]

    @property
    def dlogits(self) -> torch.Tensor:
        if self.packed:
            return self._unpack(self._dlogits)
        return self._dlogits[: self.in_B, : self.in_L]

    def features(self, dst=None, valid=None, shape=None) -> torch.Tensor:
        """The classifier's last hidden activation of the plan's last forward as a fresh [b, l, cls_hidden] tensor in the caller's
        dialogue order (post-ReLU, and post-dropout in train mode: the operand the final Linear reads); pad slots are 0.  dst / valid /
        shape: the row map and batch shape of the forward meant (default: the last `set_inputs`)."""
        b, l = (self.in_B, self.in_L) if shape is None else shape
        if self.packed:
            dst, valid = (self._dst, self._valid) if dst is None else (dst, valid)
            return self._features[dst] * valid[..., None].to(self._features.dtype)
        pad = self.keypad_in.view(self.B, self.L)[:b, :l].bool()
        return self._features[:b, :l].masked_fill(pad[..., None], 0.0)

    def aux_logits(self, num_aux: int, dst=None, valid=None, shape=None) -> torch.Tensor:
        """The auxiliary head's logits of the plan's last step as a fresh [b, l, num_aux] tensor in the caller's dialogue order; pad
        slots are 0.  dst / valid / shape: as `features`."""
        b, l = (self.in_B, self.in_L) if shape is None else shape
        rows = self._aux_logits[..., :num_aux]
        if self.packed:
            dst, valid = (self._dst, self._valid) if dst is None else (dst, valid)
            return rows[dst] * valid[..., None].to(rows.dtype)
        pad = self.keypad_in.view(self.B, self.L)[:b, :l].bool()
        return rows[:b, :l].masked_fill(pad[..., None], 0.0)

    @property
    def fam0_out(self) -> Optional[torch.Tensor]:
        if self._fam0_out is None:
            return None
        return self._unpack(self._fam0_out) if self.packed else self._fam0_out[: self.in_B, : self.in_L]

    def _h(self) -> int:
        """The C handle; raises (instead of handing NULL to the library) once the plan was closed."""
        if not self.handle:
            raise HipError("this plan was closed (evicted from the engine's plan cache or destroyed): its workspace and launch "
                           "lists are gone")
        return self.handle

    def _view(self, which: int, shape, dtype) -> torch.Tensor:
        p = lib().m2f_plan_buffer(self.handle, which)
        if not p:
            raise HipError(f"plan buffer {which} missing")
        off = p - self.workspace.data_ptr()
        n = 1
        for s in shape:
            n *= s
        esize = torch.empty(0, dtype=dtype).element_size()
        return self.workspace[off: off + n * esize].view(dtype).view(*shape)

    def check_status(self) -> None:
        """Raises on a closed plan: no kernel of the launch lists can give up, so there is nothing else to check."""
        self._h()

    def num_launches(self) -> Dict[str, int]:
        return {k: lib().m2f_plan_num_launches(self._h(), i) for i, k in enumerate(("forward", "loss", "backward"))}

    def params_fresh(self, fresh: bool) -> None:
        """Declare the shared parameter shadows current (the optimizer wrote them) or stale (the forward re-casts them)."""
        fresh = bool(fresh) and self.shared_shadow
        if fresh != self._fresh:
            check(lib().m2f_plan_params_fresh(self._h(), int(fresh)), "m2f_plan_params_fresh")
            self._fresh = fresh

    def hold(self, node) -> None:
        """A forward ran under autograd: `node` (its grad_fn) will call backward() on these activations."""
        import weakref
        self._pending = weakref.ref(node) if node is not None else None

    def release(self) -> None:
        self._pending = None

    def busy(self) -> bool:
        """True while an autograd graph that has not run its backward yet (and is still alive) owns the activations."""
        return self._pending is not None and self._pending() is not None

    def set_inputs(self, text: Optional[torch.Tensor], audio: Optional[torch.Tensor], key_pad: torch.Tensor,
                   labels: Optional[torch.Tensor] = None, speakers: Optional[torch.Tensor] = None) -> None:
        """Device-to-device copies of one batch into the plan's staging buffers (async on the stream).
        speakers (uint8 [b, l], `speaker_ids`; a plan with speaker heads): one id per utterance - it travels as the mask does, through
        bucket padding (filler slots: 0) and packing (token row cu[b] + rank, as every other row of the batch).

        The batch may be SMALLER than the plan (b <= B dialogues of l <= L utterances: the engine rounds shapes up to a few
        buckets so that the variable dialogue lengths of real data do not create a plan per length).  The extra slots are
        padding in the reference's own sense - zero features, padding_mask = True, label -1 (src/utils.py:15-31) - and each
        extra DIALOGUE keeps one unmasked, unlabeled slot (a fully masked dialogue would produce NaN logits in the reference
        too): it flows through the forward, contributes exactly zero to the loss and to every gradient,
        and its logits are cut off by the `logits` view.  Valid logits do not depend on padding (SURVEY 8-a fact i)."""
        self._h()
        b, l = key_pad.shape if key_pad.dim() == 2 else (self.B, self.L)
        if b > self.B or l > self.L:
            raise HipError(f"batch {b} x {l} does not fit the plan {self.B} x {self.L}")
        self.in_B, self.in_L = b, l
        if self.packed:
            return self._set_inputs_packed(text, audio, key_pad.reshape(b, l), labels, speakers)
        if speakers is not None:
            if (b, l) == (self.B, self.L):
                self.speakers_in.copy_(speakers.reshape(self.T), non_blocking=True)
            else:
                self.speakers_in.zero_()
                self.speakers_in.view(self.B, self.L)[:b, :l].copy_(speakers.reshape(b, l), non_blocking=True)
        if (b, l) == (self.B, self.L):
            if text is not None and self.cfg.text_enabled:
                self.text_in.copy_(text.reshape(self.T, -1), non_blocking=True)
            if audio is not None and self.cfg.audio_enabled:
                self.audio_in.copy_(audio.reshape(self.T, -1), non_blocking=True)
            self.keypad_in.copy_(key_pad.reshape(self.T), non_blocking=True)
            if labels is not None:
                self.labels_in.copy_(labels.reshape(self.T), non_blocking=True)
            return
        B, L = self.B, self.L
        if text is not None and self.cfg.text_enabled:
            self.text_in.zero_()
            self.text_in.view(B, L, -1)[:b, :l].copy_(text, non_blocking=True)
        if audio is not None and self.cfg.audio_enabled:
            self.audio_in.zero_()
            self.audio_in.view(B, L, -1)[:b, :l].copy_(audio, non_blocking=True)
        kp = self.keypad_in.view(B, L)
        kp.fill_(1)
        kp[:b, :l].copy_(key_pad, non_blocking=True)
        if b < B:
            kp[b:, 0] = 0                           # one live (unlabeled) slot per filler dialogue
        self.labels_in.fill_(-1)
        if labels is not None:
            self.labels_in.view(B, L)[:b, :l].copy_(labels, non_blocking=True)

    def _set_inputs_packed(self, text, audio, key_pad, labels, speakers=None) -> None:
        """Packs a padded batch: the valid slots of dialogue b (in order) become token rows cu[b] .. cu[b+1]-1, no sync with
        the host.  Filler dialogues of a bucketed plan get one zero, unlabeled row each; row T-1 absorbs the scatter of the
        pad slots and is zeroed afterwards (the engine sizes T for valid + fillers + 1 rows).  Rows past the last dialogue are
        padding: zero features, label -1 - they contribute exact zeros to the loss and to every gradient."""
        b, l = key_pad.shape
        dev, T = key_pad.device, self.T
        valid = ~key_pad.bool()
        rank = torch.cumsum(valid, 1, dtype=torch.int64) - 1                     # position among the dialogue's valid slots
        lens = valid.sum(1, dtype=torch.int64)
        cu = torch.zeros(self.B + 1, dtype=torch.int64, device=dev)
        cu[1: b + 1] = torch.cumsum(lens, 0)
        if b < self.B:
            cu[b + 1:] = cu[b] + torch.arange(1, self.B - b + 1, device=dev)
        self.cu_in.copy_(cu.to(torch.int32), non_blocking=True)
        # row T-1 is a real row only in a plan of B * L rows that the batch fills (no pad slot is then scattered there)
        self._spare = None if T < self.B * self.L else cu[-1] < T
        dst = torch.where(valid, cu[:b, None] + rank, torch.full_like(rank, T - 1))
        self._dst, self._valid = dst, valid
        flat = dst.reshape(-1)
        for buf, src, on in ((self.text_in, text, self.cfg.text_enabled), (self.audio_in, audio, self.cfg.audio_enabled)):
            if src is not None and on:
                buf.zero_()
                buf.index_copy_(0, flat, src.reshape(b * l, -1).to(buf.dtype))
                self._clear_spare(buf, 0)
        self.keypad_in.zero_()
        self.labels_in.fill_(-1)
        if labels is not None:
            self.labels_in.index_copy_(0, flat, labels.reshape(-1).to(torch.int64))
            self._clear_spare(self.labels_in, -1)
        if speakers is not None:                          # (the same row map; the spare row and the fillers' rows: 0)
            self.speakers_in.zero_()
            self.speakers_in.index_copy_(0, flat, speakers.reshape(-1))
            self._clear_spare(self.speakers_in, 0)

    def _clear_spare(self, buf: torch.Tensor, value) -> None:
        """Row T-1 of a packed buffer := value, unless the batch owns it (see `_set_inputs_packed`)."""
        if self._spare is None:
            buf[self.T - 1] = value
        else:
            buf[self.T - 1] = torch.where(self._spare, torch.full_like(buf[self.T - 1], value), buf[self.T - 1])

    def set_dlogits(self, g: torch.Tensor) -> None:
        """d loss / d logits of the last batch ([b, l, C], padded surface) into the plan's buffer."""
        if self.packed:
            self._dlogits.zero_()
            self._dlogits.index_copy_(0, self._dst.reshape(-1), (g * self._valid[..., None].to(g.dtype)).reshape(-1, g.shape[-1]))
            self._clear_spare(self._dlogits, 0)
            return
        if self.in_B != self.B or self.in_L != self.L:
            self._dlogits.zero_()                 # filler slots of a bucketed plan carry no gradient
        self._dlogits[: self.in_B, : self.in_L].copy_(g.reshape(self.in_B, self.in_L, -1))

    @property
    def teacher(self) -> torch.Tensor:
        """The teacher rows of the last batch on its padded surface [b, l, C] (as `logits`)."""
        if self._teacher is None:
            raise HipError("this plan holds no teacher buffer (an eval plan)")
        if self.packed:
            return self._unpack(self._teacher)
        return self._teacher[: self.in_B, : self.in_L]

    def set_teacher(self, u: torch.Tensor) -> None:
        """The teacher's logits of the last batch ([b, l, C], padded surface) into the plan's buffer: they travel as `set_dlogits`
        moves a gradient - filler rows of a bucketed plan zero, packed plans through the batch's row map with the spare row cleared."""
        if self._teacher is None:
            raise HipError("this plan holds no teacher buffer (an eval plan)")
        if self.packed:
            self._teacher.zero_()
            self._teacher.index_copy_(0, self._dst.reshape(-1), (u * self._valid[..., None].to(u.dtype)).reshape(-1, u.shape[-1]))
            self._clear_spare(self._teacher, 0)
            return
        if self.in_B != self.B or self.in_L != self.L:
            self._teacher.zero_()                 # filler slots of a bucketed plan: label -1, the criterion selects zeros there
        self._teacher[: self.in_B, : self.in_L].copy_(u.reshape(self.in_B, self.in_L, -1))

    # -- the criterion ---------------------------------------------------------------------------------------------------------------
    def _switch(self, name: str, on: bool) -> None:
        """m2f_plan_<name>(plan, on), asked only when it differs from what the plan holds."""
        on = bool(on)
        if on == (name in self.held):
            return
        check(getattr(lib(), "m2f_plan_" + name)(self._h(), int(on)), "m2f_plan_" + name)
        if on:
            self.held[name] = True
        else:
            del self.held[name]

    def distill(self, on: bool) -> None:
        """m2f_plan_distill: the NEXT losses / steps run the distillation criterion on `teacher` and `distill_hyper` (on) / the plain
        criterion (off).  A change drops the captured steps.  Neither writes nor waits: `set_distill_hyper` and `set_teacher` fill the
        two buffers on the stream before the step.  Raises for a plan without a gradient buffer."""
        self._switch("distill", on)

    def focal(self, on: bool) -> None:
        """m2f_plan_focal: the NEXT losses / steps / eval steps run the focal form of the criterion with gamma = `focal_gamma` (on) / the
        form without it (off).  A change drops the captured steps; a change of gamma alone does not.  Neither writes nor waits:
        `set_focal_gamma` fills the buffer on the stream before the step."""
        self._switch("focal", on)

    def rdrop(self, on: bool) -> None:
        """m2f_plan_rdrop: the NEXT losses / steps run the R-Drop criterion on `partner_in` and `rdrop_alpha` (on) / the criterion
        without it (off).  A change drops the captured steps; a change of alpha or of the map does not.  Neither writes nor waits.
        The distillation, focal and CRF switches must be off (the C entry refuses by name)."""
        self._switch("rdrop", on)

    def supcon(self, on: bool) -> None:
        """m2f_plan_supcon: the NEXT losses / steps add the supervised contrastive term on the hidden features (on) / do not (off).
        A change drops the captured steps; a change of the pair does not.  Neither writes nor waits.  The distillation, focal, R-Drop
        and CRF switches must be off (the C entry refuses by name)."""
        self._switch("supcon", on)

    def _block(self, name: str, entry: str, params, grad, *extra) -> None:
        """The switch of a criterion that reads a parameter block: held under the key of its two tensors, which the plan keeps alive
        (params None: off)."""
        key = None if params is None else (params.data_ptr(), None if grad is None else grad.data_ptr(), *extra)
        if key != self.held.get(name):
            check(getattr(lib(), entry)(self._h(), ptr(params), ptr(grad), *extra), entry)
            self._block_refs[name] = (params, grad)
            if key is None:
                del self.held[name]
            else:
                self.held[name] = key

    def set_crf(self, params: Optional[torch.Tensor], grad: Optional[torch.Tensor] = None) -> None:
        """m2f_plan_crf: the criterion of the plan's NEXT losses / steps / eval steps is the linear-chain CRF over `params` (the module's
        flat block, read on the device at every step), its gradient written to `grad` (None: frozen) - or (params None) not.  The plan
        keeps the two tensors alive; a change of the pointers or of the switch drops the captured steps, a change of the values does
        not.  The focal and distillation switches must be off (the C entry refuses by name)."""
        self._block("crf", "m2f_plan_crf", params, grad)

    def set_aux(self, params: Optional[torch.Tensor], grad: Optional[torch.Tensor] = None, num_aux: int = 0,
                pair: Optional[Tuple[float, float]] = None) -> None:
        """m2f_plan_aux_head: the plan's NEXT losses / steps add the auxiliary label head over `params` (the module's flat block [W | b],
        read on the device at every step), its gradient written to `grad` (None: frozen) - or (params None) not.  The plan keeps the two
        tensors alive; a change of the pointers, of num_aux or of the switch drops the captured steps, a change of the values or of
        `pair` = (weight, label smoothing) - uploaded only when it differs from the last upload - does not.  The distillation, R-Drop,
        CRF and supervised contrastive switches must be off (the C entry refuses by name)."""
        self._block("aux", "m2f_plan_aux_head", params, grad, int(num_aux) if params is not None else 0)
        if params is not None and pair is not None:
            self._upload("aux_hyper", (float(pair[0]), float(pair[1])))

    def _upload(self, buf: str, value) -> None:
        """A hyper-parameter (a float, or a tuple of floats) into the plan's buffer of that name - only when it differs from what was
        last copied there: a schedule replays the captured step, and an unchanged value costs nothing."""
        if self.uploaded.get(buf) != value:
            getattr(self, buf).copy_(torch.tensor(value, dtype=torch.float32).reshape(-1), non_blocking=True)
            self.uploaded[buf] = value

    def set_distill_hyper(self, alpha: float, temperature: float) -> None:
        """(alpha, temperature) into `distill_hyper` (`_upload`)."""
        self._upload("distill_hyper", (float(alpha), float(temperature)))

    def set_focal_gamma(self, gamma: float) -> None:
        """gamma into `focal_gamma` (`_upload`)."""
        self._upload("focal_gamma", float(gamma))

    def set_focal(self, gamma: Optional[float]) -> None:
        """The criterion of the plan's next step or eval step: focal with this gamma (a number, checked by the caller), or (None) not."""
        self.focal(gamma is not None)
        if gamma is not None:
            self.set_focal_gamma(gamma)

    def _place_partner(self) -> None:
        """The twin map of the doubled batch `set_inputs` has just placed (view 0, then view 1), written from the row map that placed
        it - a packed plan's from `_dst`, on the device; a padded or bucketed plan's depends on the batch's shape alone and is written
        only when that changed."""
        if self.in_B % 2:
            raise HipError(f"the R-Drop criterion needs the batch twice (view 0, then view 1), got {self.in_B} dialogues")
        pairs = self.in_B // 2
        if self.packed:
            self.partner_in.copy_(rdrop_partner(pairs, self.in_L, self.T, dst=self._dst, valid=self._valid), non_blocking=True)
            self._partner_key = None
        elif self._partner_key != (pairs, self.in_L):
            self.partner_in.copy_(rdrop_partner(pairs, self.in_L, self.T, L=self.L, device=self.partner_in.device), non_blocking=True)
            self._partner_key = (pairs, self.in_L)

    def _place_aux_labels(self, labels: torch.Tensor) -> None:
        """The second labels of the last batch ([b, l] int64, padded surface) into the plan's buffer: they travel as `set_inputs` moves
        the emotion labels - filler slots of a bucketed plan -1, packed plans through the batch's row map with the spare row cleared."""
        if self.packed:
            self.aux_labels_in.fill_(-1)
            self.aux_labels_in.index_copy_(0, self._dst.reshape(-1), labels.reshape(-1).to(torch.int64))
            self._clear_spare(self.aux_labels_in, -1)
            return
        if (self.in_B, self.in_L) == (self.B, self.L):
            self.aux_labels_in.copy_(labels.reshape(self.T), non_blocking=True)
            return
        self.aux_labels_in.fill_(-1)
        self.aux_labels_in.view(self.B, self.L)[: self.in_B, : self.in_L].copy_(labels, non_blocking=True)

    def set_criterion(self, spec) -> None:
        """The criterion of the plan's NEXT step or eval step: `spec`, a ``criterion.Criterion`` (checked by ``criterion.resolve``).
        AFTER `set_inputs` (a packed plan maps teacher rows, auxiliary labels and twins as it mapped the batch).  The switches move
        by `criterion_transition` - whatever the plan held, in an order no C entry refuses -, the batch's criterion inputs are placed,
        and every hyper-parameter goes through `_upload`.  A step whose criterion is the plan's last one calls no m2f_plan_* entry and
        uploads nothing: captured steps replay across schedules, and are dropped exactly when a switch or a block's pointers change.
        A CRF's or an auxiliary head's block is an input of the step; trainable, its gradient goes to the module's buffer when the
        plan trains."""
        if not self.held and not spec.kinds:
            return
        dev, blocks, wanted = self.workspace.device, {}, {k: True for k in spec.kinds}
        if spec.crf is not None:
            blocks["crf"] = spec.crf.step_buffers(dev, want_grad=self.train)
        if spec.aux is not None:
            blocks["aux"] = (*spec.aux[0].step_buffers(dev, want_grad=self.train), spec.aux[0].num_classes)
        for name, (params, grad, *extra) in blocks.items():
            wanted[name] = (params.data_ptr(), None if grad is None else grad.data_ptr(), *extra)
        for switch, value in criterion_transition(self.held, wanted):
            if switch in ("crf", "aux"):
                (self.set_crf if switch == "crf" else self.set_aux)(*(blocks[switch] if value is not None else (None,)))
            else:
                self._switch(switch, value is not None)
        if spec.distill is not None:
            self.set_teacher(spec.teacher_logits)
            self.set_distill_hyper(*spec.distill)
        if spec.gamma is not None:
            self.set_focal_gamma(spec.gamma)
        if spec.rdrop is not None:
            self._place_partner()
            self._upload("rdrop_alpha", spec.rdrop)
        if spec.supcon is not None:
            self._upload("supcon_hyper", spec.supcon)
        if spec.aux is not None:
            self._place_aux_labels(spec.aux[1])
            self._upload("aux_hyper", spec.aux[2:])

    # (what the tests of the single criteria read the held switches and the uploads by)
    _supcon = property(lambda self: "supcon" in self.held)
    _crf_key = property(lambda self: self.held.get("crf", (None, None)))
    _aux_key = property(lambda self: self.held.get("aux", (None, None, 0)), lambda self, key: self.held.__setitem__("aux", key))
    gamma_host = property(lambda self: self.uploaded.get("focal_gamma"))
    alpha_host = property(lambda self: self.uploaded.get("rdrop_alpha"))
    supcon_host = property(lambda self: self.uploaded.get("supcon_hyper"))
    aux_host = property(lambda self: self.uploaded.get("aux_hyper"))

    def _casted(self) -> None:
        if self.shared_shadow and not self._fresh and self._on_cast is not None:
            self._on_cast()

    def forward(self) -> torch.Tensor:
        self.version += 1
        check(lib().m2f_forward(self._h(), stream_ptr()), "m2f_forward")
        self._casted()
        return self.logits

    def nbytes(self) -> int:
        return self.workspace.numel() + (self._adv_state.numel() if self._adv_state is not None else 0)

    def loss_fwd(self, label_smoothing: float = 0.1, use_class_weights: bool = False, normalise: bool = True):
        check(lib().m2f_loss(self._h(), label_smoothing, int(use_class_weights), int(normalise), stream_ptr()),
              "m2f_loss")
        return self.loss

    def backward(self) -> None:
        check(lib().m2f_backward(self._h(), stream_ptr()), "m2f_backward")

    def step(self, label_smoothing: float = 0.1, use_class_weights: bool = False, normalise: bool = True,
             use_graph: bool = True) -> torch.Tensor:
        self.version += 1
        check(lib().m2f_step(self._h(), label_smoothing, int(use_class_weights), int(normalise), int(use_graph),
                             stream_ptr()), "m2f_step")
        self._casted()
        return self.loss

    def eval_step(self, record: torch.Tensor, label_smoothing: float = 0.1, use_class_weights: bool = False,
                  use_graph: bool = True) -> None:
        """m2f_eval_step: the forward, then loss / accuracy / weighted F1 / confusion matrix of the plan's own logits against its
        labels buffer, ADDED to `record` (metrics.DeviceScores.record).  Nothing comes back to the host."""
        self.version += 1
        check(lib().m2f_eval_step(self._h(), label_smoothing, int(use_class_weights), record.data_ptr(), int(use_graph), stream_ptr()),
              "m2f_eval_step")
        self._casted()

    def fused_adam_setup(self, params, exp_avg, exp_avg_sq, param_shadow, hyper, grad_scale=None) -> None:
        """m2f_plan_fused_adam_setup: the optimizer's buffers for steps that apply Adam inside the weight-gradient launch (raises when
        the plan cannot: fp32 mode, another table form, per-plan shadows)."""
        check(lib().m2f_plan_fused_adam_setup(self._h(), params.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), param_shadow.data_ptr(),
                                              hyper.data_ptr(), ptr(grad_scale)), "m2f_plan_fused_adam_setup")
        self._fused_refs = (params, exp_avg, exp_avg_sq, param_shadow, hyper, grad_scale)

    def grad_bf16(self, buf16) -> None:
        """m2f_plan_grad_bf16: the NEXT steps leave every gradient, rounded once, in `buf16` (bf16 [n_params]; None: back to fp32)."""
        check(lib().m2f_plan_grad_bf16(self._h(), buf16.data_ptr() if buf16 is not None else None), "m2f_plan_grad_bf16")
        self._g16_ref = buf16

    def accumulate_grads(self, on: bool) -> None:
        """m2f_plan_accumulate_grads: the NEXT backwards / steps ADD every parameter gradient and the criterion tail's den and num into
        the gradient buffer (on) / overwrite them (off).  Raises for a plan without a gradient buffer, with fused Adam on or bf16
        gradients armed."""
        on = bool(on)
        if on == self._acc:
            return
        check(lib().m2f_plan_accumulate_grads(self._h(), int(on)), "m2f_plan_accumulate_grads")
        self._acc = on

    def attention_band(self, past: Optional[int], future: Optional[int]) -> None:
        """m2f_plan_attention_band: the context band of EVERY attention site of the plan (both encoders, every fusion layer, forward
        and backward) - utterance i attends to utterances i - past .. i + future of its dialogue, None = unlimited on that side.  A
        change drops the captured graphs; between steps only."""
        check(lib().m2f_plan_attention_band(self._h(), *context_band(past, future)), "m2f_plan_attention_band")

    @property
    def band(self) -> Tuple[Optional[int], Optional[int]]:
        """(past, future) as the plan's launches hold it, None = unlimited."""
        a, b = c_int(0), c_int(0)
        check(lib().m2f_plan_get_attention_band(self._h(), ctypes.byref(a), ctypes.byref(b)), "m2f_plan_get_attention_band")
        return (None if a.value < 0 else a.value, None if b.value < 0 else b.value)

    def attention_bias(self, gain) -> float:
        """m2f_plan_attention_bias: the distance-decay bias of EVERY attention site of the plan (`position_bias` has the rule and the
        rounding); None / 0 = off.  Returns the applied gain.  A change drops the captured graphs; between steps only."""
        check(lib().m2f_plan_attention_bias(self._h(), position_bias(gain)), "m2f_plan_attention_bias")
        return self.bias

    @property
    def bias(self) -> float:
        """The gain as the plan's launches apply it (0.0 = off)."""
        g = c_float(0.0)
        check(lib().m2f_plan_get_attention_bias(self._h(), ctypes.byref(g)), "m2f_plan_get_attention_bias")
        return float(g.value)

    def attention_speakers(self, setting) -> Optional[Tuple[int, int]]:
        """m2f_plan_attention_speakers: speaker heads of EVERY attention site of the plan (`speaker_heads` has the rule); None = off.
        The ids are the `speakers` argument of `set_inputs`.  A change drops the captured graphs; between steps only."""
        a, b = speaker_heads(setting) or (0, 0)
        try:
            check(lib().m2f_plan_attention_speakers(self._h(), a, b), "m2f_plan_attention_speakers")
        except HipError as e:
            if "exceeds the" in str(e):
                raise ValueError(str(e)) from None
            raise
        return self.speakers

    @property
    def speakers(self) -> Optional[Tuple[int, int]]:
        """(n_same, n_other) as the plan's launches apply them, or None."""
        a, b = c_int(0), c_int(0)
        check(lib().m2f_plan_get_attention_speakers(self._h(), ctypes.byref(a), ctypes.byref(b)), "m2f_plan_get_attention_speakers")
        return (int(a.value), int(b.value)) if (a.value or b.value) else None

    def backward_outputs(self, input_mask: int, param_grads: bool) -> None:
        """m2f_plan_backward_outputs: what the NEXT backward computes - input gradients of the modalities in `input_mask` (IN_TEXT |
        IN_AUDIO) and / or the parameter gradients.  A change rebuilds the launch lists and drops the captured graphs, the fused-optimizer
        setup and the bf16-gradient arming (the optimizer sets up again at its next step, the engine re-arms plans that compute parameter
        gradients); the accumulate form stays as it is."""
        check(lib().m2f_plan_backward_outputs(self._h(), int(input_mask), int(bool(param_grads))), "m2f_plan_backward_outputs")
        if (int(input_mask), bool(param_grads)) != (self.input_mask, self.param_grads):
            self._disarm()
        self.input_mask, self.param_grads = int(input_mask), bool(param_grads)

    # -- adversarial training on the input embeddings (csrc/adversarial.hip) ----------------------------------------------------------
    def adversarial(self, mask: int) -> None:
        """m2f_plan_adversarial: the plan holds a perturbation and a clean copy of the staged input of every modality in `mask`
        (IN_TEXT | IN_AUDIO), in a buffer of its own beside the workspace - allocated here, on first use or when the mask grows (a
        plan that never asks keeps the memory it always had).  0: off, the buffer is dropped."""
        mask = int(mask)
        if mask == self.adv_mask:
            return
        if not mask:
            check(lib().m2f_plan_adversarial(self._h(), 0, None, 0), "m2f_plan_adversarial")
            self._adv_state, self.adv_mask, self.adv_hyper, self.adv_skip, self.adv_delta = None, 0, None, None, {}
            self.uploaded.pop("adv_hyper", None)
            return
        nbytes = lib().m2f_plan_adversarial_bytes(self._h(), mask)
        if nbytes < 0:
            raise HipError("m2f_plan_adversarial_bytes: " + lib().m2f_last_error().decode())
        state = torch.zeros(nbytes + 256, dtype=torch.uint8, device=self.workspace.device)
        base = state.data_ptr() + (-state.data_ptr()) % 256
        check(lib().m2f_plan_adversarial(self._h(), mask, base, nbytes), "m2f_plan_adversarial")
        self._adv_state, self.adv_mask = state, mask
        self.uploaded.pop("adv_hyper", None)

        def view(which, shape, dtype):
            off = lib().m2f_plan_buffer(self.handle, which) - state.data_ptr()
            n = 1
            for v in shape:
                n *= v
            return state[off: off + n * torch.empty(0, dtype=dtype).element_size()].view(dtype).view(*shape)

        pad8 = lambda w: (w + 7) // 8 * 8
        self.adv_hyper = view(BUF_ADV, (2,), torch.float32)
        self.adv_skip = view(BUF_ADV_SKIP, (self.T,), torch.uint8)
        self.adv_delta = {}
        for bit, which, d in ((IN_TEXT, BUF_ADV_DELTA_TEXT, self.cfg.d_text), (IN_AUDIO, BUF_ADV_DELTA_AUDIO, self.cfg.d_audio)):
            if mask & bit:
                self.adv_delta[bit] = view(which, (self.T, pad8(d)), torch.float32)[:, :d]

    def adv_place_skip(self) -> None:
        """The skip flags of the batch `set_inputs` has just placed: 1 for every token row that holds no utterance of the batch - pad
        slots, the rows of filler dialogues (which a bucketed or packed plan keeps live but unlabeled), the rows behind the last
        dialogue of a packed plan.  On the device, no host wait."""
        if self.packed:
            self.adv_skip.fill_(1)
            self.adv_skip.index_copy_(0, self._dst.reshape(-1), (~self._valid).reshape(-1).to(torch.uint8))
            self._clear_spare(self.adv_skip, 1)              # (the pad slots' scatter target, unless the batch owns it)
            return
        if (self.in_B, self.in_L) == (self.B, self.L):
            self.adv_skip.copy_(self.keypad_in, non_blocking=True)
            return
        self.adv_skip.fill_(1)
        self.adv_skip.view(self.B, self.L)[: self.in_B, : self.in_L].copy_(self.keypad_in.view(self.B, self.L)[: self.in_B, : self.in_L])

    def adv_begin(self, epsilon: float, step_size: float, init_mag: float = 0.0, norm_kind: int = 0) -> None:
        """m2f_plan_adv_begin behind the skip flags and the (epsilon, step_size) pair (uploaded only when it changed): AFTER `set_inputs`."""
        self.adv_place_skip()
        self._upload("adv_hyper", (float(epsilon), float(step_size)))
        check(lib().m2f_plan_adv_begin(self._h(), float(init_mag), int(norm_kind), stream_ptr()), "m2f_plan_adv_begin")

    def adv_ascend(self, norm_kind: int = 0) -> None:
        """m2f_plan_adv_ascend: one ascent step on the input gradients the last backward left; the staged inputs become x_clean + delta."""
        check(lib().m2f_plan_adv_ascend(self._h(), int(norm_kind), stream_ptr()), "m2f_plan_adv_ascend")

    def perturbation(self, which: int, dst=None, valid=None, shape=None) -> torch.Tensor:
        """A FRESH [b, l, d] tensor of the perturbation of modality `which` in the caller's dialogue order; pad slots are exact zeros.
        The row map as `input_grad`."""
        rows = self.adv_delta.get(which)
        if rows is None:
            raise HipError("this plan holds no perturbation of that modality")
        return self._rows_out(rows, dst, valid, shape)

    def _rows_out(self, rows: torch.Tensor, dst=None, valid=None, shape=None) -> torch.Tensor:
        """[T, d] token rows -> a fresh [b, l, d] tensor in the caller's order with exact zeros at pad slots (`input_grad`'s mapping)."""
        b, l = (self.in_B, self.in_L) if shape is None else shape
        if self.packed:
            dst, valid = (self._dst, self._valid) if dst is None else (dst, valid)
            return rows[dst] * valid[..., None].to(rows.dtype)
        pad = self.keypad_in.view(self.B, self.L)[:b, :l].bool()
        return rows.view(self.B, self.L, -1)[:b, :l].masked_fill(pad[..., None], 0.0)

    def input_grad(self, which: int, dst=None, valid=None, shape=None) -> torch.Tensor:
        """A FRESH tensor (never a view of the plan's buffer, which the next backward overwrites) holding d loss / d text (which =
        IN_TEXT) or d loss / d audio (IN_AUDIO) of the last backward, on the padded surface [b, l, d] of the batch.  Packed plans map
        the token rows back through `dst` / `valid` (the forward's `_dst` / `_valid`) and leave exact zeros at pad slots: indexing and
        copies only."""
        rows = self._dtext if which == IN_TEXT else self._daudio
        if rows is None:
            raise HipError("this plan holds no input gradient of that modality (eval plan, or the modality is disabled)")
        b, l = (self.in_B, self.in_L) if shape is None else shape
        if self.packed:
            out = torch.zeros(b, l, rows.shape[1], dtype=rows.dtype, device=rows.device)
            out[valid] = rows.index_select(0, dst[valid])
            return out
        return rows.view(self.B, self.L, -1)[:b, :l].clone()

    def attention_sites(self):
        """[(name, H, hd)] of the plan's attention sites as the C side lists them (m2f_plan_attention_sites), cross-checked against
        ``layout.attention_sites``: the index of a site in this list is what `attention_maps` takes."""
        n_max = 4096
        kind, index, layer, H, hd = ((c_int * n_max)() for _ in range(5))
        n = lib().m2f_plan_attention_sites(self._h(), kind, index, layer, H, hd, n_max)
        if n < 0 or n > n_max:
            raise HipError("m2f_plan_attention_sites: " + lib().m2f_last_error().decode())
        fmt = ("audio_encoders.{}.layers.{}.self_attn", "text_encoders.{}.layers.{}.self_attn", "fusion_layers.{}.multihead_attention")
        got = [(fmt[kind[i]].format(index[i], layer[i]), H[i], hd[i]) for i in range(n)]
        if got != attention_sites(self.cfg):
            raise HipError("attention-site list mismatch between layout.py and csrc/plan_build.hip")
        return got

    def attention_maps(self, sites, per_head: bool, dst=None, valid=None, shape=None):
        """m2f_plan_attention_weights: FRESH tensors, one per listed site index, holding the attention maps of the plan's last forward
        on the padded surface of the batch - [b, l, l] (heads averaged) or [b, H, l, l] - one eager launch for all of them.  Packed
        plans map dialogue positions back to the batch's slots through `valid` (the forward's `_valid`), with exact zeros in the rows
        and columns of pad slots: indexing only."""
        heads = [h for (_, h, _) in self.attention_sites()]
        B, L = self.B, self.L
        dev = self.workspace.device
        outs = [torch.empty((B, heads[i], L, L) if per_head else (B, L, L), dtype=torch.float32, device=dev) for i in sites]
        if not outs:
            return outs
        idx = (c_int * len(outs))(*sites)
        ptrs = (c_void_p * len(outs))(*[o.data_ptr() for o in outs])
        check(lib().m2f_plan_attention_weights(self._h(), idx, len(outs), int(bool(per_head)), ptrs, stream_ptr()),
              "m2f_plan_attention_weights")
        b, l = (self.in_B, self.in_L) if shape is None else shape
        if not self.packed:
            return [o[:b, ..., :l, :l].clone() for o in outs]
        rank = (torch.cumsum(valid, 1, dtype=torch.int64) - 1).clamp_(min=0)          # a slot's position inside its dialogue
        pair = valid[:, :, None] & valid[:, None, :]
        res = []
        for o in outs:
            r = rank[:, None].expand(-1, o.shape[1], -1) if per_head else rank
            m = o[:b].gather(-2, r.unsqueeze(-1).expand(*r.shape, L))
            m = m.gather(-1, r.unsqueeze(-2).expand(*r.shape, l))
            res.append(m * (pair[:, None] if per_head else pair).to(m.dtype))
        return res

    def fused_adam_setup_grouped(self, params, exp_avg, exp_avg_sq, param_shadow, hyper_table, tensor_group, grad_scale=None) -> None:
        """m2f_plan_fused_adam_setup_grouped: ``fused_adam_setup`` for an optimizer with parameter groups / decoupled weight decay -
        `hyper_table` the rows of ``adam_hyper_groups``, `tensor_group` the group of every parameter tensor (-1: none)."""
        tg = (c_int * len(tensor_group))(*tensor_group)
        check(lib().m2f_plan_fused_adam_setup_grouped(self._h(), params.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(),
                                                      param_shadow.data_ptr(), hyper_table.data_ptr(), tg, len(tensor_group), ptr(grad_scale)),
              "m2f_plan_fused_adam_setup_grouped")

    def fused_adam(self, on: bool) -> None:
        """The NEXT step() also takes the optimizer step (on) / leaves the weight gradients in the gradient buffer (off)."""
        check(lib().m2f_plan_fused_adam(self._h(), int(bool(on))), "m2f_plan_fused_adam")

    def skipped_copies(self) -> int:
        """How many fp32 / bf16 copies of activations this plan does not write because nobody reads them (bf16 mode)."""
        return int(lib().m2f_plan_skipped_copies(self._h()))

    def split_offset(self) -> int:
        """First element of the flat gradient buffer that is final after `step_part(0)` (0: this plan cannot be split)."""
        return int(lib().m2f_plan_split_offset(self._h()))

    def step_part(self, part: int, label_smoothing: float = 0.1, use_class_weights: bool = False, normalise: bool = True,
                  use_graph: bool = True) -> torch.Tensor:
        """m2f_step_part: part 0 = forward + criterion + classifier / fusion backward (+ their weight gradients), part 1 = the rest."""
        if part == 0:
            self.version += 1
        check(lib().m2f_step_part(self._h(), int(part), label_smoothing, int(use_class_weights), int(normalise), int(use_graph),
                                  stream_ptr()), "m2f_step_part")
        if part == 0:
            self._casted()
        return self.loss

    def step_timed(self, label_smoothing: float = 0.1, use_class_weights: bool = False, normalise: bool = True):
        """One eager step with per-launch hipEvent timing -> list of (kind, ms, algorithmic flops)."""
        self.version += 1
        n_max = 4096
        kinds, ms, fl = (c_int * n_max)(), (c_float * n_max)(), (ctypes.c_double * n_max)()
        n = lib().m2f_step_timed(self._h(), label_smoothing, int(use_class_weights), int(normalise), stream_ptr(),
                                 n_max, kinds, ms, fl)
        if n < 0:
            raise HipError("m2f_step_timed: " + lib().m2f_last_error().decode())
        self._casted()
        return [(kinds[i], ms[i], fl[i]) for i in range(n)]

    def close(self) -> None:
        """Destroy the plan (captured graph, launch lists) and drop its workspace."""
        h = getattr(self, "handle", None)
        if h and _lib is not None:
            _lib.m2f_plan_destroy(h)
        self.handle = None
        self.workspace = None
        self._adv_state = None

    def __del__(self):
        self.close()


class StreamPlan:
    """One stream plan (m2f_plan_create_stream) + its workspace: `S` stream slots, K / V caches of `capacity` rows per slot at every
    attention site (a ring when `past` is an integer).  `streaming.DialogueStream` drives it.

    With `pages` (m2f_plan_create_stream_paged) every site holds pools of `pages` pages of `page_rows` (16 / 32 / 64) rows instead, and
    `table` (int32 [S, ceil(capacity / page_rows)], an input like `active`) names the page of each run of `page_rows` logical cache
    rows of a slot; the caller allocates (`streaming.PageAllocator`)."""

    def __init__(self, cfg: M2FConfig, S: int, capacity: int, past: Optional[int], precision: int, params: torch.Tensor,
                 param_shadow: Optional[torch.Tensor] = None, pages: Optional[int] = None, page_rows: int = 16):
        require_gpu()
        with torch.inference_mode(False):          # (a stream opened under inference_mode must stay writable outside it)
            self._create(cfg, S, capacity, past, precision, params, param_shadow, pages, page_rows)

    def _create(self, cfg, S, capacity, past, precision, params, param_shadow, pages=None, page_rows=16) -> None:
        self.cfg, self.S, self.capacity, self.past, self.precision = cfg, S, capacity, past, precision
        self.pages, self.page_rows = pages, page_rows
        self._cc = config_to_c(cfg)
        self.shared_shadow = param_shadow is not None
        self._fresh = False
        past_c = -1 if past is None else int(past)
        if pages is None:
            nbytes = lib().m2f_stream_workspace_bytes(ctypes.byref(self._cc), S, capacity, past_c, precision, int(self.shared_shadow))
        else:
            nbytes = lib().m2f_stream_paged_workspace_bytes(ctypes.byref(self._cc), S, capacity, past_c, precision, pages, page_rows,
                                                            int(self.shared_shadow))
        if nbytes < 0:
            raise HipError(("m2f_stream_workspace_bytes: " if pages is None else "m2f_stream_paged_workspace_bytes: ") + lib().m2f_last_error().decode())
        self.workspace = torch.zeros(nbytes + 256, dtype=torch.uint8, device=params.device)
        torch.cuda.current_stream(params.device).synchronize()       # (as Plan: the create call uses blocking copies on the null stream)
        base = self.workspace.data_ptr()
        off = (-base) % 256
        self._keep = (params, param_shadow)
        if pages is None:
            self.handle = lib().m2f_plan_create_stream(ctypes.byref(self._cc), S, capacity, past_c, precision, params.data_ptr(), base + off,
                                                       nbytes, ptr(param_shadow))
        else:
            self.handle = lib().m2f_plan_create_stream_paged(ctypes.byref(self._cc), S, capacity, past_c, precision, pages, page_rows,
                                                             params.data_ptr(), base + off, nbytes, ptr(param_shadow))
        if not self.handle:
            raise HipError(("m2f_plan_create_stream: " if pages is None else "m2f_plan_create_stream_paged: ") + lib().m2f_last_error().decode())
        pad8 = lambda w: (w + 7) // 8 * 8
        self.text_in = self._view(BUF_TEXT, (S, pad8(max(cfg.d_text, 1))), torch.float32)[:, : max(cfg.d_text, 1)]
        self.audio_in = self._view(BUF_AUDIO, (S, pad8(max(cfg.d_audio, 1))), torch.float32)[:, : max(cfg.d_audio, 1)]
        self.logits = self._view(BUF_LOGITS, (S, cfg.cls_out), torch.float32)
        self.len = self._view(BUF_STREAM_LEN, (S,), torch.int32)
        self.active = self._view(BUF_STREAM_ACTIVE, (S,), torch.uint8)
        self.table = None if pages is None else self._view(BUF_STREAM_TABLE, (S, (capacity + page_rows - 1) // page_rows), torch.int32)
        self.speakers_in = self._view(BUF_SPEAKERS, (S,), torch.uint8)       # speaker heads: the new utterances' ids, one per slot
        self.spk_cache = None                                                 # ... and the cached ones (`stream_speakers`)

    _h = Plan._h
    _view = Plan._view

    def params_fresh(self, fresh: bool) -> None:
        fresh = bool(fresh) and self.shared_shadow
        if fresh != self._fresh:
            check(lib().m2f_plan_params_fresh(self._h(), int(fresh)), "m2f_plan_params_fresh")
            self._fresh = fresh

    def step(self, use_graph: bool = True) -> None:
        check(lib().m2f_stream_step(self._h(), int(use_graph), stream_ptr()), "m2f_stream_step")

    def stream_crf(self, params: Optional[torch.Tensor], phi: Optional[torch.Tensor]) -> None:
        """m2f_plan_stream_crf: the step / prefill also runs the CRF's forward filter over `params` into the caller's `phi` [S, C] (both
        None: off).  The plan keeps the two tensors alive."""
        check(lib().m2f_plan_stream_crf(self._h(), ptr(params), ptr(phi)), "m2f_plan_stream_crf")
        self._crf_ref = (params, phi)

    def reset(self, mask: Optional[torch.Tensor] = None) -> None:
        """mask: device uint8 [S], non-zero = the slot starts a new dialogue; None = every slot."""
        check(lib().m2f_stream_reset(self._h(), ptr(mask), stream_ptr()), "m2f_stream_reset")

    def cache_bytes(self) -> int:
        return int(lib().m2f_stream_cache_bytes(self._h()))

    def snapshot_row_elems(self) -> int:
        """W: elements of one cached utterance over every site, K and V (m2f_stream_snapshot_row_elems)."""
        n = int(lib().m2f_stream_snapshot_row_elems(self._h()))
        if n < 0:
            raise HipError("m2f_stream_snapshot_row_elems: " + lib().m2f_last_error().decode())
        return n

    def snapshot_sites(self):
        """((H, hd), ...) of the attention sites in plan order: the order of a snapshot's segments."""
        n = lib().m2f_stream_snapshot_sites(self._h(), None, None, 0)
        if n < 0:
            raise HipError("m2f_stream_snapshot_sites: " + lib().m2f_last_error().decode())
        H, hd = (c_int * n)(), (c_int * n)()
        lib().m2f_stream_snapshot_sites(self._h(), H, hd, n)
        return tuple((int(a), int(b)) for a, b in zip(H, hd))

    def gather(self, slots: torch.Tensor, lengths: torch.Tensor, row_offsets: torch.Tensor, packed: torch.Tensor) -> None:
        """The live cache rows of the listed slots -> `packed` (m2f_stream_gather).  slots, lengths: device int32 [n]; row_offsets: device
        int64 [n]; packed: a contiguous 1-D tensor of the caches' element type."""
        check(lib().m2f_stream_gather(self._h(), slots.numel(), ptr(slots), ptr(lengths), ptr(row_offsets), ptr(packed), packed.numel(),
                                      stream_ptr()), "m2f_stream_gather")

    def scatter(self, slots: torch.Tensor, lengths: torch.Tensor, row_offsets: torch.Tensor, packed: torch.Tensor) -> None:
        """`packed` -> the cache rows of the listed slots, and len[slot] = lengths[e] (m2f_stream_scatter); a paged plan's table must
        already name the pages."""
        check(lib().m2f_stream_scatter(self._h(), slots.numel(), ptr(slots), ptr(lengths), ptr(row_offsets), ptr(packed), packed.numel(),
                                       stream_ptr()), "m2f_stream_scatter")

    attention_sites = Plan.attention_sites
    attention_bias = Plan.attention_bias         # (before the first step or between steps; a chunk plan takes it when it is created)
    bias = Plan.bias
    attention_speakers = Plan.attention_speakers     # (`stream_speakers` first)
    speakers = Plan.speakers

    def stream_speakers(self, on: bool) -> Optional[torch.Tensor]:
        """m2f_plan_stream_speakers: the cached speaker ids of the stream, uint8 [S, capacity] by LOGICAL cache row (row u % capacity of a
        ring; dense on a paged stream too) - made here (on) or dropped (off; refused while the plan has speaker heads).  The step
        stores the new ids in the launch that advances the counters."""
        if bool(on) == (self.spk_cache is not None):
            return self.spk_cache
        if not on:
            check(lib().m2f_plan_stream_speakers(self._h(), None), "m2f_plan_stream_speakers")
            self.spk_cache = None
            return None
        with torch.inference_mode(False):
            buf = torch.zeros(self.S, self.capacity, dtype=torch.uint8, device=self.workspace.device)
        torch.cuda.current_stream(buf.device).synchronize()
        check(lib().m2f_plan_stream_speakers(self._h(), buf.data_ptr()), "m2f_plan_stream_speakers")
        self.spk_cache = buf
        return buf

    def stream_attention(self, on: bool) -> None:
        """m2f_plan_stream_attention: from the next step on the attention launches also store each (slot, head)'s row of probabilities
        (on: into a buffer of m2f_stream_attention_elems floats made here - [site][S][H][C], 17.8 MB at C3, S = 64, C = 512) / run the
        kernels they always ran (off: the buffer is dropped).  A change drops the captured step once."""
        if bool(on) == (getattr(self, "attn_buf", None) is not None):
            return
        if not on:
            check(lib().m2f_plan_stream_attention(self._h(), None, 0), "m2f_plan_stream_attention")
            self.attn_buf = None
            return
        n = int(lib().m2f_stream_attention_elems(self._h()))
        if n < 0:
            raise HipError("m2f_stream_attention_elems: " + lib().m2f_last_error().decode())
        with torch.inference_mode(False):
            buf = torch.zeros(max(n, 4), dtype=torch.float32, device=self.workspace.device)
        torch.cuda.current_stream(buf.device).synchronize()          # (the switch waits for the device on the null stream)
        check(lib().m2f_plan_stream_attention(self._h(), buf.data_ptr(), buf.numel()), "m2f_plan_stream_attention")
        self.attn_buf = buf

    def attention_rows(self, sites, per_head: bool):
        """m2f_stream_attention: fresh tensors, one per listed site index, with the rows of the last step - [S, H, C] or, heads
        averaged on the device, [S, C]; one eager launch."""
        heads = [h for (_, h, _) in self.attention_sites()]
        dev = self.workspace.device
        outs = [torch.empty((self.S, heads[i], self.capacity) if per_head else (self.S, self.capacity), dtype=torch.float32, device=dev)
                for i in sites]
        if outs:
            idx = (c_int * len(outs))(*sites)
            ptrs = (c_void_p * len(outs))(*[o.data_ptr() for o in outs])
            check(lib().m2f_stream_attention(self._h(), idx, len(outs), int(bool(per_head)), ptrs, stream_ptr()), "m2f_stream_attention")
        return outs

    def num_launches(self) -> int:
        return lib().m2f_plan_num_launches(self._h(), 0) + 1

    def nbytes(self) -> int:
        return self.workspace.numel()

    def close(self) -> None:
        h = getattr(self, "handle", None)
        if h and _lib is not None:
            _lib.m2f_plan_destroy(h)
        self.handle = None
        self.workspace = None
        self.attn_buf = None
        self.spk_cache = None

    def __del__(self):
        self.close()


class StreamChunkPlan:
    """One chunk plan (m2f_plan_create_stream_chunk) + its workspace: up to `T` new utterances per slot and call over the caches and
    counts of `parent`, a StreamPlan (which must stay open while this plan lives).  Rows s*T + t of `text_in` / `audio_in` / `logits`
    ([S, T, .] views) belong to slot s; `new` (int32 [S]) holds how many of them the slot takes.  `streaming.DialogueStream.prefill`
    drives it."""

    def __init__(self, parent: "StreamPlan", T: int, params: torch.Tensor, param_shadow: Optional[torch.Tensor] = None):
        require_gpu()
        with torch.inference_mode(False):
            self._create(parent, T, params, param_shadow)

    def _create(self, parent, T, params, param_shadow) -> None:
        cfg, S = parent.cfg, parent.S
        self.cfg, self.S, self.T, self.parent, self.precision = cfg, S, T, parent, parent.precision
        self.shared_shadow = param_shadow is not None
        self._fresh = False
        nbytes = lib().m2f_stream_chunk_workspace_bytes(parent._h(), T, int(self.shared_shadow))
        if nbytes < 0:
            raise HipError("m2f_stream_chunk_workspace_bytes: " + lib().m2f_last_error().decode())
        self.workspace = torch.zeros(nbytes + 256, dtype=torch.uint8, device=params.device)
        torch.cuda.current_stream(params.device).synchronize()       # (as Plan: the create call uses blocking copies on the null stream)
        base = self.workspace.data_ptr()
        off = (-base) % 256
        self._keep = (params, param_shadow, parent)
        self.handle = lib().m2f_plan_create_stream_chunk(parent._h(), T, params.data_ptr(), base + off, nbytes, ptr(param_shadow))
        if not self.handle:
            raise HipError("m2f_plan_create_stream_chunk: " + lib().m2f_last_error().decode())
        pad8 = lambda w: (w + 7) // 8 * 8
        self.text_in = self._view(BUF_TEXT, (S, T, pad8(max(cfg.d_text, 1))), torch.float32)[:, :, : max(cfg.d_text, 1)]
        self.audio_in = self._view(BUF_AUDIO, (S, T, pad8(max(cfg.d_audio, 1))), torch.float32)[:, :, : max(cfg.d_audio, 1)]
        self.logits = self._view(BUF_LOGITS, (S, T, cfg.cls_out), torch.float32)
        self.new = self._view(BUF_STREAM_NEW, (S,), torch.int32)
        self.len = parent.len
        self.pages, self.page_rows, self.table = parent.pages, parent.page_rows, parent.table     # (a paged parent: its pools, its table)
        self.speakers_in = self._view(BUF_SPEAKERS, (S, T), torch.uint8)     # speaker heads: the chunk's ids, row s = slot s

    _h = Plan._h
    _view = Plan._view
    params_fresh = StreamPlan.params_fresh
    attention_bias = Plan.attention_bias         # (created with the parent's gain; a change drops the captured prefill)
    bias = Plan.bias
    attention_speakers = Plan.attention_speakers     # (created with the parent's setting and cached ids; `follow_speakers` after a change)
    speakers = Plan.speakers

    def follow_speakers(self) -> None:
        """Take the parent's cached-speaker array and speaker-head setting (after they changed on the parent)."""
        par = self.parent
        if par.spk_cache is None or par.speakers is None:      # (off: the chunk plan lets go of the array before the parent drops it)
            self.attention_speakers(None)
            check(lib().m2f_plan_stream_speakers(self._h(), None), "m2f_plan_stream_speakers")
        else:
            check(lib().m2f_plan_stream_speakers(self._h(), par.spk_cache.data_ptr()), "m2f_plan_stream_speakers")
            self.attention_speakers(par.speakers)
    nbytes = StreamPlan.nbytes
    close = StreamPlan.close
    stream_crf = StreamPlan.stream_crf

    def prefill(self, use_graph: bool = True) -> None:
        """forward over the chunk + len[s] += new[s]"""
        self.parent._h()
        check(lib().m2f_stream_prefill(self._h(), int(use_graph), stream_ptr()), "m2f_stream_prefill")

    def num_launches(self) -> int:
        return lib().m2f_plan_num_launches(self._h(), 0) + 1

    def __del__(self):
        self.close()


def event_overhead(pairs: int = 200):
    """-> (empty hipEvent pair, pair around a one-thread kernel) in ms: what a step_timed interval holds besides the kernel."""
    scratch = torch.zeros(4, dtype=torch.int32, device="cuda")
    a, b = c_float(0), c_float(0)
    check(lib().m2f_event_overhead(scratch.data_ptr(), pairs, ctypes.byref(a), ctypes.byref(b), stream_ptr()), "m2f_event_overhead")
    return a.value, b.value


def param_shadow_buffer(cfg: M2FConfig, device) -> torch.Tensor:
    """The shared bf16 parameter-shadow buffer of a model (+ the fused optimizer's tensor table behind it), initialised."""
    cc = config_to_c(cfg)
    n = lib().m2f_param_shadow_elems(ctypes.byref(cc))
    if n < 0:
        raise HipError(lib().m2f_last_error().decode())
    buf = torch.empty(n + 128, dtype=torch.int16, device=device)
    off = ((-buf.data_ptr()) % 256) // 2
    buf = buf[off: off + n]
    torch.cuda.current_stream(buf.device).synchronize()
    check(lib().m2f_param_shadow_init(ctypes.byref(cc), buf.data_ptr(), stream_ptr()), "m2f_param_shadow_init")
    return buf


def adam_step_shadowed(cfg: M2FConfig, params, grads, exp_avg, exp_avg_sq, param_shadow, step: int, lr: float,
                       betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                       grad_scale: Optional[torch.Tensor] = None, first: int = 0, end: int = -1,
                       ema: Optional[torch.Tensor] = None, ema_w: float = 0.0) -> None:
    """torch.optim.Adam's update over the flat buffers + the bf16 shadows of every 2-D parameter (m2f_adam_step_shadowed_range).
    The buffers are always passed WHOLE; `[first, end)` - offsets of parameter tensors, end < 0: to the last one - selects what is
    updated; `grads` fp32, or bf16 (the reduced buffer of the data-parallel bf16 exchange, same indexing).  `ema` (the WHOLE fp32
    average buffer) with `ema_w` = 1 - decay: the same launch also averages what it updates (m2f_adam_step_shadowed_range_ema)."""
    cc = config_to_c(cfg)
    if ema is not None:
        check(lib().m2f_adam_step_shadowed_range_ema(ctypes.byref(cc), params.data_ptr(), grads.data_ptr(), int(grads.dtype == torch.bfloat16),
                                                     exp_avg.data_ptr(), exp_avg_sq.data_ptr(), param_shadow.data_ptr(), ema.data_ptr(),
                                                     float(ema_w), int(first), int(end), lr, betas[0], betas[1], eps, weight_decay, step,
                                                     ptr(grad_scale), stream_ptr()), "m2f_adam_step_shadowed_range_ema")
        return
    check(lib().m2f_adam_step_shadowed_range(ctypes.byref(cc), params.data_ptr(), grads.data_ptr(), int(grads.dtype == torch.bfloat16),
                                             exp_avg.data_ptr(), exp_avg_sq.data_ptr(), param_shadow.data_ptr(), int(first), int(end),
                                             lr, betas[0], betas[1], eps, weight_decay, step, ptr(grad_scale), stream_ptr()),
          "m2f_adam_step_shadowed_range")


# Loads of the sum-of-squares kernel: nontemporal.  The optimizer reads the same gradients right behind it, but plain loads do not
# leave them where it would find them - measured inside the C3 bf16 step (tools/bench_grad_clip.py, rocprofv3 kernel times): fp32
# gradients 90 us plain / 70 us nontemporal, bf16 gradients 42 / 37 us, the Adam kernel behind it 597 / 596 us and 566 / 567 us.
GRAD_NORM_NONTEMPORAL = True


def grad_norm_scratch(cfg: M2FConfig, device) -> torch.Tensor:
    """float64 scratch of the gradient-norm launches: one partial sum of squares per 8192-element slice of a parameter tensor."""
    cc = config_to_c(cfg)
    n = lib().m2f_grad_norm_scratch_bytes(ctypes.byref(cc))
    if n < 0:
        raise HipError(lib().m2f_last_error().decode())
    return torch.zeros(n // 8, dtype=torch.float64, device=device)


def grad_sumsq(cfg: M2FConfig, grads: torch.Tensor, scratch: torch.Tensor, first: int = 0, end: int = -1, grid: int = 0,
               nontemporal: Optional[bool] = None) -> None:
    """m2f_grad_sumsq: the partial sums of squares of the parameter tensors at flat offsets [first, end) of `grads` (the WHOLE flat
    gradient buffer, fp32 or bf16) into `scratch`, on the current stream.  `grid` / `nontemporal` change speed only, never a bit."""
    cc = config_to_c(cfg)
    nt = GRAD_NORM_NONTEMPORAL if nontemporal is None else bool(nontemporal)
    check(lib().m2f_grad_sumsq(ctypes.byref(cc), grads.data_ptr(), int(grads.dtype == torch.bfloat16), int(first), int(end),
                               scratch.data_ptr(), int(grid), int(nt), stream_ptr()), "m2f_grad_sumsq")


def grad_norm_finalize(cfg: M2FConfig, scratch: torch.Tensor, record: torch.Tensor, max_norm: float,
                       den: Optional[torch.Tensor] = None) -> None:
    """m2f_grad_norm_finalize: record <- (norm, coef, divisor, sqrt(sum of squares)), four fp32 values, from every partial of `scratch`."""
    cc = config_to_c(cfg)
    check(lib().m2f_grad_norm_finalize(ctypes.byref(cc), scratch.data_ptr(), ptr(den), float(max_norm), record.data_ptr(), stream_ptr()),
          "m2f_grad_norm_finalize")


def check_sam_rho(rho, who: str = "FusedAdam") -> Optional[float]:
    """``sam_rho``: None, or a finite number > 0 (-> float); anything else is a ValueError."""
    if rho is None:
        return None
    if isinstance(rho, bool) or not isinstance(rho, (int, float)) or not math.isfinite(rho) or not rho > 0.0:
        raise ValueError(f"{who}.sam_rho must be None or a finite number > 0 (got {rho!r})")
    return float(rho)


def sam_perturb(cfg: M2FConfig, params: torch.Tensor, grads: torch.Tensor, saved: torch.Tensor, param_shadow: Optional[torch.Tensor],
                scratch: torch.Tensor, record: torch.Tensor, rho: float, grad_scale: Optional[torch.Tensor] = None) -> None:
    """m2f_sam_perturb on the current stream: `scratch` holds grad_sumsq's partials of `grads` (fp32 or bf16, the WHOLE flat buffer);
    record <- (||g / grad_scale||, c, grad_scale, sqrt(sum of squares)), saved <- params, params <- fma(c, grads, params) over parameter
    elements, and - with `param_shadow` - the bf16 shadows of the perturbed matrices."""
    cc = config_to_c(cfg)
    g16 = grads.dtype == torch.bfloat16
    check(lib().m2f_sam_perturb(ctypes.byref(cc), params.data_ptr(), None if g16 else grads.data_ptr(), grads.data_ptr() if g16 else None,
                                saved.data_ptr(), ptr(param_shadow), scratch.data_ptr(), ptr(grad_scale), float(rho), record.data_ptr(),
                                stream_ptr()), "m2f_sam_perturb")


def sam_restore(cfg: M2FConfig, params: torch.Tensor, saved: torch.Tensor) -> None:
    """m2f_sam_restore on the current stream: params <- saved over parameter elements (the pads keep what they hold)."""
    cc = config_to_c(cfg)
    check(lib().m2f_sam_restore(ctypes.byref(cc), params.data_ptr(), saved.data_ptr(), stream_ptr()), "m2f_sam_restore")


TSTATS_HEADER, TSTATS_FIELDS, TSTATS_MAX_BINS = 4, 9, 256      # csrc/ops.h M2F_TSTATS_*


def tensor_stats_buffers(cfg: M2FConfig, bins: int, device) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (scratch, record) of m2f_tensor_stats for `bins` bins: uint8 scratch of one partial per 8192-element slice of a parameter
    tensor, and the float64 record (TSTATS_HEADER values, then TSTATS_FIELDS + bins per parameter tensor; the counts are int64 bits)."""
    cc = config_to_c(cfg)
    ns, nr = lib().m2f_tensor_stats_scratch_bytes(ctypes.byref(cc), int(bins)), lib().m2f_tensor_stats_record_bytes(ctypes.byref(cc), int(bins))
    if ns < 0 or nr < 0:
        raise HipError(lib().m2f_last_error().decode())
    return torch.zeros(ns // 8, dtype=torch.float64, device=device), torch.zeros(nr // 8, dtype=torch.float64, device=device)


def tensor_stats(cfg: M2FConfig, a: torch.Tensor, scratch: torch.Tensor, record: torch.Tensor, bins: int,
                 b: Optional[torch.Tensor] = None, den: Optional[torch.Tensor] = None, grid: int = 0,
                 nontemporal: Optional[bool] = None, passes: int = 3) -> None:
    """m2f_tensor_stats: statistics and `bins`-bin histogram of every parameter tensor of the WHOLE flat buffer `a` (fp32 or bf16; with
    `b`, fp32: of a - b) into `record`, three launches on the current stream.  `grid` / `nontemporal` change speed only, never a byte;
    `passes` (1: statistics, 2: histogram alone, 3: both) is for timing."""
    cc = config_to_c(cfg)
    nt = GRAD_NORM_NONTEMPORAL if nontemporal is None else bool(nontemporal)
    if passes == 3:
        check(lib().m2f_tensor_stats(ctypes.byref(cc), a.data_ptr(), int(a.dtype == torch.bfloat16), ptr(b), int(bins), ptr(den),
                                     scratch.data_ptr(), record.data_ptr(), int(grid), int(nt), stream_ptr()), "m2f_tensor_stats")
        return
    check(lib().m2f_tensor_stats_passes(ctypes.byref(cc), a.data_ptr(), int(a.dtype == torch.bfloat16), ptr(b), int(bins), ptr(den),
                                        scratch.data_ptr(), record.data_ptr(), int(grid), int(nt), int(passes), stream_ptr()),
          "m2f_tensor_stats_passes")


def adam_hyper(hyper: torch.Tensor, step: int, lr: float, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0) -> None:
    """The step-dependent factors of Adam's update into 8 device floats (read by the fused step's kernels), on the current stream."""
    check(lib().m2f_adam_hyper(hyper.data_ptr(), lr, betas[0], betas[1], eps, weight_decay, int(step), stream_ptr()), "m2f_adam_hyper")


def adam_step(params: torch.Tensor, grads: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor, step: int,
              lr: float, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
              grad_scale: Optional[torch.Tensor] = None, ema: Optional[torch.Tensor] = None, ema_w: float = 0.0) -> None:
    """grads: fp32, or bf16 (the reduced buffer of the data-parallel bf16 exchange) - same update, fp32 state either way.
    `ema` (fp32, the elements of `params`) with `ema_w` = 1 - decay: the same launch also averages (m2f_adam_step_ema / _g16_ema)."""
    if ema is not None:
        g16 = grads.dtype == torch.bfloat16
        fn = lib().m2f_adam_step_g16_ema if g16 else lib().m2f_adam_step_ema
        check(fn(params.data_ptr(), grads.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), ema.data_ptr(), params.numel(), lr,
                 betas[0], betas[1], eps, weight_decay, step, float(ema_w), ptr(grad_scale), stream_ptr()),
              "m2f_adam_step_g16_ema" if g16 else "m2f_adam_step_ema")
        return
    if grads.dtype == torch.bfloat16:
        check(lib().m2f_adam_step_g16(params.data_ptr(), grads.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(),
                                      params.numel(), lr, betas[0], betas[1], eps, weight_decay, step, ptr(grad_scale),
                                      stream_ptr()), "m2f_adam_step_g16")
        return
    check(lib().m2f_adam_step(params.data_ptr(), grads.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(),
                              params.numel(), lr, betas[0], betas[1], eps, weight_decay, step, ptr(grad_scale),
                              stream_ptr()), "m2f_adam_step")


ADAM_MAX_GROUPS = 16


class AdamGroupC(ctypes.Structure):
    """m2f_adam_group (include/m2fnet_hip.h)."""
    _fields_ = [("lr", ctypes.c_double), ("beta1", c_float), ("beta2", c_float), ("eps", c_float), ("weight_decay", c_float),
                ("decoupled", c_int), ("step", c_int)]


def adam_hyper_groups(table: torch.Tensor, groups) -> None:
    """m2f_adam_hyper_groups: one row of 8 floats per group into `table` ([>= len(groups), 8] fp32 on the device), one launch on the
    current stream.  `groups`: (lr, (beta1, beta2), eps, weight_decay, decoupled, step) per group, step >= 1 the group's own count."""
    arr = (AdamGroupC * len(groups))(*[AdamGroupC(float(lr), float(b[0]), float(b[1]), float(eps), float(wd), int(bool(dec)), int(step))
                                       for (lr, b, eps, wd, dec, step) in groups])
    check(lib().m2f_adam_hyper_groups(table.data_ptr(), arr, len(groups), stream_ptr()), "m2f_adam_hyper_groups")


def adam_step_grouped(cfg: M2FConfig, params, grads, exp_avg, exp_avg_sq, param_shadow: Optional[torch.Tensor], tensor_group,
                      hyper_table: torch.Tensor, grad_scale: Optional[torch.Tensor] = None, first: int = 0, end: int = -1,
                      ema: Optional[torch.Tensor] = None, ema_w: float = 0.0) -> None:
    """torch.optim.Adam / AdamW with parameter groups over the flat buffers (m2f_adam_step_grouped): the tensors at offsets
    [first, end) that a group owns (`tensor_group`: a ctypes int array, one entry per parameter tensor, -1 = none) with their group's row
    of `hyper_table`; `param_shadow` (bf16 mode) or None (fp32 mode); `grads` fp32 or bf16.  `ema` with `ema_w` = 1 - decay: the same
    launch also averages the owned tensors (m2f_adam_step_grouped_ema)."""
    cc = config_to_c(cfg)
    if ema is not None:
        check(lib().m2f_adam_step_grouped_ema(ctypes.byref(cc), params.data_ptr(), grads.data_ptr(), int(grads.dtype == torch.bfloat16),
                                              exp_avg.data_ptr(), exp_avg_sq.data_ptr(), ptr(param_shadow), ema.data_ptr(), float(ema_w),
                                              tensor_group, len(tensor_group), hyper_table.data_ptr(), int(first), int(end),
                                              ptr(grad_scale), stream_ptr()), "m2f_adam_step_grouped_ema")
        return
    check(lib().m2f_adam_step_grouped(ctypes.byref(cc), params.data_ptr(), grads.data_ptr(), int(grads.dtype == torch.bfloat16),
                                      exp_avg.data_ptr(), exp_avg_sq.data_ptr(), ptr(param_shadow), tensor_group, len(tensor_group),
                                      hyper_table.data_ptr(), int(first), int(end), ptr(grad_scale), stream_ptr()), "m2f_adam_step_grouped")


def ema_exchange(cfg: M2FConfig, params: torch.Tensor, ema: torch.Tensor, tensor_group) -> None:
    """m2f_ema_exchange: params <-> ema in place over every tensor a group owns (`tensor_group` as in adam_step_grouped), on the current
    stream; pads and unowned tensors are not touched."""
    cc = config_to_c(cfg)
    check(lib().m2f_ema_exchange(ctypes.byref(cc), params.data_ptr(), ema.data_ptr(), tensor_group, len(tensor_group), stream_ptr()),
          "m2f_ema_exchange")
