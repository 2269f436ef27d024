"""ctypes binding of libmtn_hip.so (C ABI in include/mtn_hip.h).

The HIP library is the product path: if it is missing this module raises — there is no
CPU or PyTorch fallback behind these calls.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import gc
import os
import threading

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmtn_hip.so")

MTN_F32, MTN_BF16 = 0, 1
MTN_ACCUM_FIRST, MTN_ACCUM_ADD, MTN_ACCUM_LAST = 0, 1, 2      # mtn_grad_accum's modes (include/mtn_hip.h)
MTN_SCHED_ARGMAX, MTN_SCHED_SAMPLE = 0, 1                     # mtn_sched_mix's picks


class Dropout(C.Structure):
    _fields_ = [("p", C.c_float), ("salt", C.c_uint32), ("seed", C.c_void_p)]


class AdamFuse(C.Structure):
    _fields_ = [("p", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("p_lp", C.c_void_p), ("p_lpT", C.c_void_p),
                ("ldT", C.c_int), ("write_grad", C.c_int), ("state", C.c_void_p), ("grad_scale", C.c_void_p),
                ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float)]


class LnEpilogue(C.Structure):
    _fields_ = [("mode", C.c_int), ("fold", C.c_void_p), ("gate_inv_scale", C.c_float), ("part", C.c_void_p), ("np", C.c_int),
                ("x", C.c_void_p), ("a2", C.c_void_p), ("mean", C.c_void_p), ("rstd", C.c_void_p), ("dres", C.c_void_p),
                ("eps", C.c_float), ("dx", C.c_void_p), ("dx_lp", C.c_void_p), ("dx_lp_drop", Dropout), ("colpart", C.c_void_p)]


class LnFoldDesc(C.Structure):
    _fields_ = [("w", C.c_void_p), ("bias", C.c_void_p), ("a2", C.c_void_p), ("b2", C.c_void_p), ("out", C.c_void_p),
                ("K", C.c_int), ("block_start", C.c_int)]


class GemmProblem(C.Structure):
    _fields_ = [("A", C.c_void_p), ("B", C.c_void_p), ("lda", C.c_int), ("ldb", C.c_int),
                ("M", C.c_int), ("N", C.c_int), ("K", C.c_int), ("a_trans", C.c_int), ("b_trans", C.c_int),
                ("bias", C.c_void_p), ("relu", C.c_int), ("drop", Dropout),
                ("gate", C.c_void_p), ("gate_scale", C.c_float),
                ("residual", C.c_void_p), ("ldr", C.c_int),
                ("out_f32", C.c_void_p), ("out_lp", C.c_void_p), ("ldc", C.c_int), ("lp_drop_after_residual", C.c_int),
                ("rowsum_out", C.c_void_p),
                ("adam", C.POINTER(AdamFuse)), ("ln", C.POINTER(LnEpilogue))]


class AttnArgs(C.Structure):
    _fields_ = [("B", C.c_int), ("h", C.c_int), ("a", C.c_int), ("m", C.c_int), ("dk", C.c_int),
                ("q", C.c_void_p), ("k", C.c_void_p), ("v", C.c_void_p), ("ldq", C.c_int), ("ldkv", C.c_int),
                ("mask", C.c_void_p), ("mask_sb", C.c_long), ("mask_sq", C.c_long), ("drop", Dropout),
                ("o", C.c_void_p), ("ldo", C.c_int), ("lse", C.c_void_p),
                ("d_o", C.c_void_p), ("dq", C.c_void_p), ("dk_out", C.c_void_p), ("dv_out", C.c_void_p),
                ("q0", C.c_int), ("qn", C.c_int), ("kv_accum", C.c_int), ("kv_acc", C.c_void_p), ("kv_last", C.c_int)]


class MhaArgs(C.Structure):
    _fields_ = [("B", C.c_int), ("a", C.c_int), ("m", C.c_int), ("d", C.c_int), ("h", C.c_int),
                ("self_attn", C.c_int), ("ln_eps", C.c_float), ("drop_attn", Dropout), ("drop_out", Dropout),
                ("x", C.c_void_p), ("mem", C.c_void_p), ("mask", C.c_void_p), ("mask_sb", C.c_long), ("mask_sq", C.c_long),
                ("ln_a", C.c_void_p), ("ln_b", C.c_void_p), ("w_qkv", C.c_void_p), ("b_qkv", C.c_void_p),
                ("w_o", C.c_void_p), ("b_o", C.c_void_p), ("w_qkv_t", C.c_void_p), ("w_o_t", C.c_void_p),
                ("y", C.c_void_p), ("xn", C.c_void_p), ("mean", C.c_void_p), ("rstd", C.c_void_p),
                ("qkv", C.c_void_p), ("kv", C.c_void_p), ("o", C.c_void_p), ("lse", C.c_void_p),
                ("dy", C.c_void_p), ("dx", C.c_void_p), ("dmem", C.c_void_p), ("dmem_accumulate", C.c_int),
                ("d_ln_a", C.c_void_p), ("d_ln_b", C.c_void_p),
                ("d_w_qkv", C.c_void_p), ("d_b_qkv", C.c_void_p), ("d_w_o", C.c_void_p), ("d_b_o", C.c_void_p),
                ("ws_lp", C.c_void_p), ("ws_f32", C.c_void_p), ("defer_param_grads", C.c_int),
                ("dyl_ready", C.c_void_p), ("next_dyl", C.c_void_p), ("next_drop", Dropout), ("kv_ready", C.c_int),
                ("dmem_lp", C.c_void_p), ("dmem_lp_drop", Dropout), ("ln_fold", C.c_void_p)]


class FfnArgs(C.Structure):
    _fields_ = [("rows", C.c_int), ("d", C.c_int), ("d_ff", C.c_int), ("ln_eps", C.c_float),
                ("drop_hidden", Dropout), ("drop_out", Dropout),
                ("x", C.c_void_p), ("ln_a", C.c_void_p), ("ln_b", C.c_void_p),
                ("w1", C.c_void_p), ("b1", C.c_void_p), ("w2", C.c_void_p), ("b2", C.c_void_p),
                ("w1_t", C.c_void_p), ("w2_t", C.c_void_p),
                ("y", C.c_void_p), ("xn", C.c_void_p), ("mean", C.c_void_p), ("rstd", C.c_void_p), ("hid", C.c_void_p),
                ("dy", C.c_void_p), ("dx", C.c_void_p),
                ("d_ln_a", C.c_void_p), ("d_ln_b", C.c_void_p), ("d_w1", C.c_void_p), ("d_b1", C.c_void_p),
                ("d_w2", C.c_void_p), ("d_b2", C.c_void_p),
                ("ws_lp", C.c_void_p), ("ws_f32", C.c_void_p), ("defer_param_grads", C.c_int),
                ("dyl_ready", C.c_void_p), ("next_dyl", C.c_void_p), ("next_drop", Dropout), ("y_lp", C.c_void_p),
                ("ln_fold", C.c_void_p)]


class LossHeadArgs(C.Structure):
    _fields_ = [("n_seg", C.c_int), ("rows", C.c_int * 4), ("target", C.c_void_p * 4), ("norm", C.c_void_p * 4), ("coef", C.c_float * 4),
                ("V", C.c_int), ("ldz", C.c_int), ("pad", C.c_int), ("smoothing", C.c_float),
                ("logits", C.c_void_p), ("lse", C.c_void_p), ("rowloss", C.c_void_p),
                ("gloss", C.c_void_p), ("dlogits", C.c_void_p), ("ldd", C.c_int)]


class DistillHeadArgs(C.Structure):
    _fields_ = LossHeadArgs._fields_ + [("teacher", C.c_void_p * 4), ("ldq", C.c_long * 4), ("alpha", C.c_float), ("temperature", C.c_float),
                                        ("rowkd", C.c_void_p)]


class WLossHeadArgs(C.Structure):
    _fields_ = LossHeadArgs._fields_ + [("roww", C.c_void_p * 4), ("smoothing_seg", C.c_float * 4)]


class ULossHeadArgs(C.Structure):
    _fields_ = LossHeadArgs._fields_ + [("seq_len", C.c_int * 4), ("ul_alpha", C.c_float), ("rowul", C.c_void_p)]


class RLossHeadArgs(C.Structure):
    _fields_ = LossHeadArgs._fields_ + [("pair", C.c_int * 4), ("rd_alpha", C.c_float), ("rowrd", C.c_void_p), ("rowkl", C.c_void_p)]


class TransposeDesc(C.Structure):
    _fields_ = [("off", C.c_long), ("rows", C.c_int), ("cols", C.c_int), ("tile_start", C.c_int), ("reserved", C.c_int), ("dst_off", C.c_long)]


class LnFwdDesc(C.Structure):
    _fields_ = [("rows", C.c_int), ("d", C.c_int), ("eps", C.c_float), ("x", C.c_void_p), ("a2", C.c_void_p), ("b2", C.c_void_p),
                ("y_f32", C.c_void_p), ("y_lp", C.c_void_p), ("mean", C.c_void_p), ("rstd", C.c_void_p),
                ("tokens", C.c_void_p), ("lut", C.c_void_p), ("emb_scale", C.c_float), ("pe", C.c_void_p), ("seq_len", C.c_int),
                ("drop", Dropout), ("x_out", C.c_void_p), ("no_ln", C.c_int)]


class EmbedBwdDesc(C.Structure):
    _fields_ = [("rows", C.c_int), ("d", C.c_int), ("tokens", C.c_void_p), ("dx", C.c_void_p), ("emb_scale", C.c_float),
                ("drop", Dropout), ("dlut", C.c_void_p), ("lut_rows", C.c_int)]


class LnBwdDesc(C.Structure):
    _fields_ = [("rows", C.c_int), ("d", C.c_int), ("eps", C.c_float), ("x", C.c_void_p), ("a2", C.c_void_p), ("mean", C.c_void_p),
                ("rstd", C.c_void_p), ("g", C.c_void_p), ("dres", C.c_void_p), ("dx", C.c_void_p), ("partial", C.c_void_p),
                ("dx_lp", C.c_void_p), ("dx_lp_dtype", C.c_int), ("dx_lp_drop", Dropout)]


class CastDesc(C.Structure):
    _fields_ = [("n", C.c_long), ("src", C.c_void_p), ("dst", C.c_void_p), ("drop", Dropout), ("gate", C.c_void_p)]


class TtLnUnit(C.Structure):
    _fields_ = [("partial", C.c_void_p), ("nparts", C.c_int), ("d", C.c_int), ("a_off", C.c_long), ("b_off", C.c_long)]


class TtAux(C.Structure):
    _fields_ = [("p", C.c_void_p), ("g", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("lp", C.c_void_p), ("n_flat", C.c_long),
                ("n_ln", C.c_int), ("ln", C.POINTER(TtLnUnit)), ("n_chunks", C.c_int), ("chunk_off", C.POINTER(C.c_long)),
                ("chunk_len", C.POINTER(C.c_int)), ("bias_adam", C.c_int), ("state", C.c_void_p), ("grad_scale", C.c_void_p),
                ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float)]


class DecodeStage(C.Structure):
    _fields_ = [("kind", C.c_int), ("N", C.c_int), ("K", C.c_int), ("w", C.c_void_p), ("bias", C.c_void_p), ("ln_a", C.c_void_p),
                ("ln_b", C.c_void_p), ("ln_eps", C.c_float), ("kv", C.c_void_p), ("m", C.c_int), ("mask", C.c_void_p),
                ("mask_stride", C.c_long), ("cache", C.c_void_p)]


class DecodeArgs(C.Structure):
    _fields_ = [("W", C.c_int), ("d", C.c_int), ("h", C.c_int), ("L", C.c_int), ("n_stages", C.c_int), ("d_ff", C.c_int), ("xg", C.c_void_p), ("qg", C.c_void_p),
                ("og", C.c_void_p), ("hg", C.c_void_p), ("out_lp", C.c_void_p), ("tokens", C.c_void_p), ("lut", C.c_void_p),
                ("emb_scale", C.c_float), ("pe", C.c_void_p), ("pos", C.c_void_p), ("anc", C.c_void_p), ("sync", C.c_void_p), ("dbg", C.c_void_p), ("max_m", C.c_int)]


DEC_EMBED, DEC_SELF_QKV, DEC_SELF_ATT, DEC_OUT, DEC_CROSS, DEC_FFN1, DEC_FFN2, DEC_FINAL = range(8)


class BeamArgs(C.Structure):
    _fields_ = [("dialogues", C.c_int), ("width", C.c_int), ("L", C.c_int), ("k_top", C.c_int), ("k", C.c_int), ("beam", C.c_int), ("unk", C.c_int),
                ("eos", C.c_int), ("pad", C.c_int), ("min_len", C.c_int), ("penalty", C.c_double), ("top", C.c_void_p), ("tokens", C.c_void_p),
                ("pos", C.c_void_p), ("anc", C.c_void_p), ("lp", C.c_void_p), ("n_live", C.c_void_p), ("step", C.c_void_p), ("flags", C.c_void_p),
                ("log_parent", C.c_void_p), ("log_tok", C.c_void_p), ("log_score", C.c_void_p), ("log_done", C.c_void_p), ("log_n_old", C.c_void_p),
                ("log_n_new", C.c_void_p)]


class DiverseArgs(C.Structure):
    _fields_ = [("beam", BeamArgs), ("groups", C.c_int), ("diversity", C.c_float)]


class SampleArgs(C.Structure):
    _fields_ = [("rows", C.c_int), ("V", C.c_int), ("ldx", C.c_long), ("logp", C.c_void_p), ("temperature", C.c_float), ("top_k", C.c_int),
                ("top_p", C.c_float), ("n_banned", C.c_int), ("banned", C.c_int * 4), ("eos", C.c_int), ("min_len", C.c_int),
                ("seed", C.c_void_p), ("key", C.c_void_p), ("step", C.c_void_p), ("L", C.c_int), ("log_tok", C.c_void_p),
                ("log_logp", C.c_void_p), ("log_u", C.c_void_p), ("tokens", C.c_void_p), ("pos", C.c_void_p), ("anc", C.c_void_p)]


class ContrastiveArgs(C.Structure):
    _fields_ = [("dialogues", C.c_int), ("k", C.c_int), ("L", C.c_int), ("d", C.c_int), ("k_top", C.c_int), ("alpha", C.c_float),
                ("eos", C.c_int), ("min_len", C.c_int), ("n_banned", C.c_int), ("banned", C.c_int * 4), ("hidden", C.c_void_p),
                ("row_stride", C.c_long), ("pos_stride", C.c_long), ("top", C.c_void_p), ("tokens", C.c_void_p), ("pos", C.c_void_p),
                ("cand_logp", C.c_void_p), ("step", C.c_void_p), ("done", C.c_void_p), ("log_tok", C.c_void_p), ("log_logp", C.c_void_p),
                ("log_pen", C.c_void_p), ("log_rank", C.c_void_p)]


class ScoreArgs(C.Structure):
    _fields_ = [("n_seq", C.c_int), ("L", C.c_int), ("V", C.c_int), ("pad", C.c_int), ("ldz", C.c_long), ("logits", C.c_void_p),
                ("target", C.c_void_p), ("tok_logp", C.c_void_p), ("tok_rank", C.c_void_p), ("seq_logp", C.c_void_p), ("seq_len", C.c_void_p)]


class ConstrainArgs(C.Structure):
    _fields_ = [("rows", C.c_int), ("V", C.c_int), ("ldx", C.c_long), ("ldo", C.c_long), ("logp", C.c_void_p), ("out", C.c_void_p),
                ("ngram", C.c_int), ("theta", C.c_float), ("L", C.c_int), ("hist", C.c_void_p), ("ldh", C.c_long), ("hist_len", C.c_void_p),
                ("log_tok", C.c_void_p), ("log_parent", C.c_void_p), ("step", C.c_void_p), ("width", C.c_int), ("rows_per_step", C.c_int)]


class EnsembleArgs(C.Structure):
    _fields_ = [("rows", C.c_int), ("V", C.c_int), ("M", C.c_int), ("mode", C.c_int), ("x", C.c_void_p * 8), ("ld", C.c_long * 8),
                ("w", C.c_float * 8), ("out", C.c_void_p), ("ldo", C.c_long)]


class MbrArgs(C.Structure):
    _fields_ = [("sets", C.c_int), ("K", C.c_int), ("L", C.c_int), ("N", C.c_int), ("ldl", C.c_long), ("tok", C.c_void_p), ("len", C.c_void_p),
                ("n_hyp", C.c_void_p), ("w", C.c_void_p), ("log_tok", C.c_void_p), ("eos", C.c_int), ("expected", C.c_void_p),
                ("best", C.c_void_p), ("order", C.c_void_p), ("util", C.c_void_p)]


class EvalArgs(C.Structure):
    _fields_ = [("Q", C.c_int), ("R", C.c_int), ("L", C.c_int), ("ldl", C.c_long), ("hyp", C.c_void_p), ("hyp_len", C.c_void_p),
                ("ref", C.c_void_p), ("ref_len", C.c_void_p), ("n_ref", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_long),
                ("stats", C.c_void_p), ("rouge", C.c_void_p), ("cider", C.c_void_p), ("corpus", C.c_void_p), ("df_of_ref", C.c_void_p)]


class EvalRowsArgs(C.Structure):
    _fields_ = [("Qc", C.c_int), ("R", C.c_int), ("L", C.c_int), ("ldl", C.c_long), ("ref", C.c_void_p), ("ref_len", C.c_void_p),
                ("n_ref", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_long), ("N", C.c_int), ("hyp", C.c_void_p),
                ("hyp_len", C.c_void_p), ("item", C.c_void_p), ("stats", C.c_void_p), ("rouge", C.c_void_p), ("cider", C.c_void_p)]


class ScstAssembleArgs(C.Structure):
    _fields_ = [("rows", C.c_int), ("L", C.c_int), ("T", C.c_int), ("log_tok", C.c_void_p), ("sos", C.c_int), ("eos", C.c_int),
                ("pad", C.c_int), ("trg", C.c_void_p), ("trg_y", C.c_void_p), ("hyp", C.c_void_p), ("ldh", C.c_long), ("hyp_len", C.c_void_p)]


class ScstAdvantageArgs(C.Structure):
    _fields_ = [("D", C.c_int), ("S", C.c_int), ("T", C.c_int), ("reward", C.c_void_p), ("baseline", C.c_void_p), ("roww", C.c_void_p),
                ("adv", C.c_void_p), ("mean_reward", C.c_void_p), ("mean_baseline", C.c_void_p)]


class SchedArgs(C.Structure):
    _fields_ = [("B", C.c_int), ("T", C.c_int), ("V", C.c_int), ("ldx", C.c_long), ("logits", C.c_void_p), ("trg", C.c_void_p),
                ("key", C.c_void_p), ("state", C.c_void_p), ("pad", C.c_long), ("n_banned", C.c_int), ("banned", C.c_int * 4),
                ("p_max", C.c_float), ("start", C.c_int), ("ramp", C.c_int), ("pick", C.c_int), ("inv_temperature", C.c_float),
                ("seed", C.c_long), ("mixed", C.c_void_p), ("stats", C.c_void_p), ("pick_score", C.c_void_p)]


class LnFinalizeDesc(C.Structure):
    _fields_ = [("partial", C.c_void_p), ("nparts", C.c_int), ("d", C.c_int), ("da2", C.c_void_p), ("db2", C.c_void_p)]


GEMM_MAX_GROUP = 16


# every symbol include/mtn_hip.h declares: name -> (restype, argtypes)
_P = C.c_void_p
class AssembleTokensDesc(C.Structure):
    _fields_ = [("flat", C.c_void_p), ("start", C.c_void_p), ("len", C.c_void_p), ("ids", C.c_void_p), ("B", C.c_int), ("L", C.c_int),
                ("pad", C.c_int64), ("out", C.c_void_p), ("mask", C.c_void_p), ("std_mask", C.c_void_p), ("n_nonpad", C.c_void_p),
                ("row_len", C.c_void_p)]          # NULL (a zeroed struct): no row is cut


class AssembleFeaturesDesc(C.Structure):
    _fields_ = [("flat", C.c_void_p), ("start", C.c_void_p), ("len", C.c_void_p), ("ids", C.c_void_p), ("B", C.c_int), ("V", C.c_int),
                ("F", C.c_int), ("skip", C.c_int), ("out", C.c_void_p), ("mask", C.c_void_p)]


class CensusLaunch(C.Structure):
    _fields_ = [("dtype", C.c_int), ("count", C.c_int), ("variant", C.c_int), ("workgroups", C.c_int),
                ("flops", C.c_double), ("bytes", C.c_double), ("M", C.c_int * 4), ("N", C.c_int * 4), ("K", C.c_int * 4)]


SYMBOLS = {
    "mtn_assemble_tokens": (C.c_int, [C.c_int, C.POINTER(AssembleTokensDesc), _P]),
    "mtn_assemble_features": (C.c_int, [C.c_int, C.POINTER(AssembleFeaturesDesc), _P]),
    "mtn_topk_rows": (C.c_int, [_P, C.c_int, C.c_int, C.c_long, C.c_int, C.c_int, _P, _P]),
    "mtn_log_softmax_rows": (C.c_int, [_P, C.c_int, C.c_int, C.c_long, _P, C.c_long, _P]),
    "mtn_census_begin": (C.c_int, []),
    "mtn_census_end": (C.c_int, []),
    "mtn_census_info": (C.c_int, [C.c_int, C.POINTER(CensusLaunch)]),
    "mtn_census_replay": (C.c_int, [C.c_int, C.c_int, _P]),
    "mtn_census_variant_name": (C.c_char_p, [C.c_int]),
    "mtn_measure_mfma_peak": (C.c_int, [C.c_int, _P, _P, C.POINTER(C.c_double)]),
    "mtn_measure_mfma_peak_shapes": (C.c_int, [C.c_int, _P, _P, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "mtn_measure_hbm_peak": (C.c_int, [_P, _P, C.c_long, _P, C.POINTER(C.c_double)]),
    "mtn_reload_env": (C.c_int, []),
    "mtn_stream_create_cu_masked": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "mtn_stream_destroy": (C.c_int, [_P]),
    "mtn_last_error": (C.c_char_p, []),
    "mtn_version": (C.c_int, []),
    "mtn_gemm": (C.c_int, [C.c_int, C.c_int, C.POINTER(GemmProblem), _P]),
    "mtn_gemm_tt_table": (C.c_int, [C.c_int, C.c_int, C.POINTER(GemmProblem), _P]),
    "mtn_decode_step": (C.c_int, [C.POINTER(DecodeArgs), _P, C.c_int, _P]),
    "mtn_beam_advance": (C.c_int, [C.POINTER(BeamArgs), _P]),
    "mtn_diverse_advance": (C.c_int, [C.POINTER(DiverseArgs), _P]),
    "mtn_sample_rows": (C.c_int, [C.POINTER(SampleArgs), _P]),
    "mtn_contrastive_advance": (C.c_int, [C.POINTER(ContrastiveArgs), _P]),
    "mtn_score_rows": (C.c_int, [C.POINTER(ScoreArgs), _P]),
    "mtn_constrain_rows": (C.c_int, [C.POINTER(ConstrainArgs), _P]),
    "mtn_ensemble_rows": (C.c_int, [C.POINTER(EnsembleArgs), _P]),
    "mtn_mbr_select": (C.c_int, [C.POINTER(MbrArgs), _P]),
    "mtn_eval_metrics": (C.c_int, [C.POINTER(EvalArgs), _P]),
    "mtn_eval_workspace_bytes": (C.c_long, [C.c_int, C.c_int, C.c_int]),
    "mtn_debug_hold_cus": (C.c_int, [C.c_int, C.c_int, C.c_int, _P]),
    "mtn_gemm_tt_table_aux": (C.c_int, [C.c_int, C.c_int, C.POINTER(GemmProblem), C.POINTER(TtAux), _P]),
    "mtn_layernorm_fwd": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_float, _P, _P, _P, _P, _P, _P, _P, _P]),
    "mtn_layernorm_fwd_group": (C.c_int, [C.c_int, C.c_int, C.POINTER(LnFwdDesc), _P]),
    "mtn_embed_bwd_group": (C.c_int, [C.c_int, C.POINTER(EmbedBwdDesc), _P]),
    "mtn_layernorm_bwd_group": (C.c_int, [C.c_int, C.POINTER(LnBwdDesc), _P]),
    "mtn_attention_fwd_group": (C.c_int, [C.c_int, C.c_int, C.POINTER(AttnArgs), _P]),
    "mtn_attention_bwd_group": (C.c_int, [C.c_int, C.c_int, C.POINTER(AttnArgs), _P]),
    "mtn_cast_group": (C.c_int, [C.c_int, C.c_int, C.POINTER(CastDesc), _P]),
    "mtn_fused_enable": (C.c_int, [C.c_int]),
    "mtn_kv_project": (C.c_int, [C.c_int, C.c_int, C.POINTER(GemmProblem), C.c_int, _P]),
    "mtn_riders_flush": (C.c_int, [_P]),
    "mtn_riders_enabled": (C.c_int, []),
    "mtn_rider_counters": (C.c_int, [C.POINTER(C.c_long)]),
    "mtn_fused_counters": (C.c_int, [C.POINTER(C.c_long)]),
    "mtn_ln_epilogue_groups": (C.c_long, []),
    "mtn_ln_fold": (C.c_int, [C.c_int, _P, _P, C.c_int, C.c_int, _P]),
    "mtn_sublayer_group_fwd": (C.c_int, [C.c_int, C.c_int, C.POINTER(MhaArgs), C.c_int, C.POINTER(FfnArgs), _P]),
    "mtn_sublayer_group_bwd": (C.c_int, [C.c_int, C.c_int, C.POINTER(MhaArgs), C.c_int, C.POINTER(FfnArgs), _P]),
    "mtn_layernorm_bwd_partial_floats": (C.c_long, [C.c_int, C.c_int]),
    "mtn_layernorm_bwd_nparts": (C.c_int, [C.c_int]),
    "mtn_layernorm_bwd_finalize": (C.c_int, [C.c_int, C.POINTER(LnFinalizeDesc), _P]),
    "mtn_mha_param_grad_work": (C.c_int, [C.c_int, C.POINTER(MhaArgs), C.POINTER(GemmProblem), C.POINTER(LnFinalizeDesc)]),
    "mtn_ffn_param_grad_work": (C.c_int, [C.c_int, C.POINTER(FfnArgs), C.POINTER(GemmProblem), C.POINTER(LnFinalizeDesc)]),
    "mtn_layernorm_bwd": (C.c_int, [C.c_int, C.c_int, C.c_float, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "mtn_attention_fwd": (C.c_int, [C.c_int, C.POINTER(AttnArgs), _P]),
    "mtn_attention_bwd": (C.c_int, [C.c_int, C.POINTER(AttnArgs), _P]),
    "mtn_mha_sublayer_fwd": (C.c_int, [C.c_int, C.POINTER(MhaArgs), _P]),
    "mtn_mha_sublayer_bwd": (C.c_int, [C.c_int, C.POINTER(MhaArgs), _P]),
    "mtn_mha_bwd_ws_lp_elems": (C.c_long, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "mtn_mha_bwd_ws_f32_floats": (C.c_long, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "mtn_ffn_sublayer_fwd": (C.c_int, [C.c_int, C.POINTER(FfnArgs), _P]),
    "mtn_ffn_sublayer_bwd": (C.c_int, [C.c_int, C.POINTER(FfnArgs), _P]),
    "mtn_ffn_bwd_ws_f32_floats": (C.c_long, [C.c_int, C.c_int, C.c_int]),
    "mtn_cast_f32_to_lp": (C.c_int, [C.c_int, C.c_long, _P, _P, _P]),
    "mtn_dropout_bwd_to_lp": (C.c_int, [C.c_int, C.c_long, _P, Dropout, _P, _P]),
    "mtn_losshead_fwd": (C.c_int, [C.POINTER(LossHeadArgs), _P]),
    "mtn_losshead_bwd": (C.c_int, [C.c_int, C.POINTER(LossHeadArgs), _P]),
    "mtn_distill_fwd": (C.c_int, [C.POINTER(DistillHeadArgs), _P]),
    "mtn_distill_bwd": (C.c_int, [C.c_int, C.POINTER(DistillHeadArgs), _P]),
    "mtn_wlosshead_fwd": (C.c_int, [C.POINTER(WLossHeadArgs), _P]),
    "mtn_wlosshead_bwd": (C.c_int, [C.c_int, C.POINTER(WLossHeadArgs), _P]),
    "mtn_ulosshead_fwd": (C.c_int, [C.POINTER(ULossHeadArgs), _P]),
    "mtn_ulosshead_bwd": (C.c_int, [C.c_int, C.POINTER(ULossHeadArgs), _P]),
    "mtn_rlosshead_fwd": (C.c_int, [C.POINTER(RLossHeadArgs), _P]),
    "mtn_rlosshead_bwd": (C.c_int, [C.c_int, C.POINTER(RLossHeadArgs), _P]),
    "mtn_eval_table_build": (C.c_int, [C.POINTER(EvalRowsArgs), _P]),
    "mtn_eval_score_rows": (C.c_int, [C.POINTER(EvalRowsArgs), _P]),
    "mtn_scst_assemble": (C.c_int, [C.POINTER(ScstAssembleArgs), _P]),
    "mtn_scst_advantage": (C.c_int, [C.POINTER(ScstAdvantageArgs), _P]),
    "mtn_transpose_group": (C.c_int, [C.c_int, _P, _P, _P, C.c_int, C.c_int, _P]),
    "mtn_noam_tick": (C.c_int, [_P, C.c_float, C.c_int, C.c_int, C.c_float, C.c_float, _P]),
    "mtn_adam_step": (C.c_int, [C.c_int, C.c_long, _P, _P, _P, _P, _P, _P, _P, C.c_float, C.c_float, C.c_float, _P]),
    "mtn_adam_step_chunks": (C.c_int, [C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.c_float, C.c_float, C.c_float, _P]),
    "mtn_lerp_f32": (C.c_int, [C.c_long, _P, _P, C.c_float, _P]),
    "mtn_ema_step": (C.c_int, [C.c_long, _P, _P, _P, C.c_float, _P, _P]),
    "mtn_swap_f32": (C.c_int, [C.c_long, _P, _P, _P]),
    "mtn_grad_sumsq_partials": (C.c_int, [C.c_long]),
    "mtn_grad_sumsq": (C.c_int, [C.c_long, _P, _P, _P]),
    "mtn_clip_scale": (C.c_int, [C.c_int, _P, C.c_float, _P, _P, _P, _P, _P]),
    "mtn_grad_accum": (C.c_int, [C.c_int, C.c_long, _P, _P, _P, _P, _P, _P, _P]),
    "mtn_sched_mix": (C.c_int, [C.POINTER(SchedArgs), _P]),
}

_lib = None


class MtnHipError(RuntimeError):
    pass


def load():
    """Load the HIP library or raise.  No fallback."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("MTN_HIP_LIB", LIB_PATH)      # A/B builds of the kernels (same ABI) — development only
    if not os.path.exists(path):
        raise MtnHipError(f"{path} is missing: build it with `python -m mtn_amd.build` "
                          "(hipcc --offload-arch=gfx950).  mtn_amd has no CPU/PyTorch fallback.")
    lib = C.CDLL(path)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)             # AttributeError here = ABI drift: fail loudly
        fn.restype, fn.argtypes = res, args
    _lib = lib
    return lib


def fused_counters():
    """(forward fused, forward per-stage, backward fused, backward per-stage) group counts since the library was loaded."""
    out = (C.c_long * 4)()
    check(load().mtn_fused_counters(out))
    return tuple(int(v) for v in out)


def reload_env():
    """Make the library re-read its MTN_* environment switches (they are cached per call site): call after changing one."""
    if _lib is not None:
        _lib.mtn_reload_env()


def check(rc: int):
    if rc != 0:
        raise MtnHipError(f"libmtn_hip error {rc}: {load().mtn_last_error().decode()}")


def stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


_capture_lock = threading.Lock()
_captures = [0, False]          # captures open in any thread; whether the collector was on when the first of them began


@contextlib.contextmanager
def capturing(graph, **kw):
    """A ``torch.cuda.graph`` capture into ``graph`` (keywords passed on) with Python's cyclic garbage collector off while it lasts.
    A collection can start at any allocation, on any thread (the autograd worker that runs the deferred parameter-gradient flush
    included), and it runs the destructors of whatever dead cycles exist — among them captured graphs of trainers and sessions no
    longer in use.  The ROCm build's CUDAGraph destructor synchronises the device, which is forbidden while a stream is capturing: the
    error is raised inside a destructor and the process aborts.  Nothing is lost by waiting: the cycles are collected after the capture.
    The switch is process-wide, so captures are counted under a lock: the collector comes back when the LAST open capture ends, and
    only if it was on when the first began."""
    with _capture_lock:
        if _captures[0] == 0:
            _captures[1] = gc.isenabled()
            gc.disable()
        _captures[0] += 1
    try:
        with torch.cuda.graph(graph, **kw):
            yield
    finally:
        with _capture_lock:
            _captures[0] -= 1
            if _captures[0] == 0 and _captures[1]:
                gc.enable()


def ptr(t) -> int:
    return 0 if t is None else t.data_ptr()


def dtype_code(dt: torch.dtype) -> int:
    if dt == torch.float32:
        return MTN_F32
    if dt == torch.bfloat16:
        return MTN_BF16
    raise ValueError(f"unsupported compute dtype {dt}")
