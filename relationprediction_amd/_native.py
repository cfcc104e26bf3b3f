"""ctypes binding of librgcn.so (C ABI: include/rgcn.h).

This is the only place Python crosses into native code -- the analogue of
``session.run`` in the reference (code/optimization/optimize.py:81-88,
code/model.py:56,69,81).  There is NO fallback: if the HIP library is missing
or no GPU is visible, construction fails loudly.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "librgcn.so")

ABI_VERSION = 1
KIND_BLOCK, KIND_BASIS, KIND_BASIS_TDIAG, KIND_BASIS_PDIAG = 0, 1, 2, 3
KIND_EMBEDDING = 4           # Encoder.Name=embedding: no graph, no layers, the codes are W_emb (RGCN_KIND_EMBEDDING)
NORM_INTENDED, NORM_TF_AS_EXECUTED, NORM_NONE, NORM_LOCAL = 0, 1, 2, 3
BUF_EXCHANGE, BUF_SELF, BUF_DSELF_EXCHANGE, BUF_INDEG, BUF_OUTDEG, BUF_ROWPTR, BUF_NORM_EXCHANGE, \
    BUF_DBASIS_EXCHANGE, BUF_PERM_VERTEX, BUF_PERM_RELATION, BUF_RANK_ENERGIES, BUF_MSG_NORM, BUF_HIGHWAY_INNER, \
    BUF_HIGHWAY_GATE = range(14)
BUF_TDIAG_PRODUCTS = 14      # basis_tdiag contexts: [2, V, B*d], P_f then P_b of the layer run last
BUF_PDIAG_MIX = 15           # basis_pdiag contexts: [2, V, B], the mixing table a of the layer run last
BUF_PDIAG_AGG = 16           # basis_pdiag contexts: [V, d], the diagonal aggregate of the layer run last
BUF_RANK_MIXED_SCORES = 17   # [reserved queries, V], the mixed scores the last topk_mixed selected from
BUF_RELATION_ENERGIES = 18   # [reserved queries, R], the energies of the chunk a relation query scored last
BUF_OUT_DH = 19              # contexts with an output transform: [V, d], dL/dH_L of the last backward pass
BUF_NEGATIVE_UNRESOLVED = 20 # int64 [1]: negative rows every entity was a known positive for, since the reserve
BUF_NEGATIVE_RELATION_UNRESOLVED = 21  # int64 [1]: relation rows every other relation was a known positive for
BUF_RELATION_SOFTMAX_ENERGIES = 22  # [chunk, padded R]: the energies of the chunk the relation-softmax term walked last
BUF_RELATION_SOFTMAX_G = 23         # [chunk, padded R]: their gradients
BUF_RELATION_SOFTMAX_DQ = 24        # [chunk, code width]: the gradients of that chunk's query rows
BUF_ADVERSARIAL_WEIGHTS = 25        # [N]: the row weights of the last fused step under set_adversarial_negatives
BUF_ENTITY_SOFTMAX_G = 26           # [chunk, padded V]: the gradients of the chunk of rows the entity-softmax term walked last
BUF_ENTITY_SOFTMAX_DQ = 27          # [chunk, code width]: the gradients of that chunk's query rows
BUF_NEGATIVE_TYPED_OPEN = 28        # int64 [1]: negative rows the typed sampler drew over all entities, since the reserve
KINDS = {"block": KIND_BLOCK, "basis": KIND_BASIS, "basis_tdiag": KIND_BASIS_TDIAG,
         "basis_pdiag": KIND_BASIS_PDIAG, "embedding": KIND_EMBEDDING}
NORMS = {"intended": NORM_INTENDED, "tf_as_executed": NORM_TF_AS_EXECUTED, "none": NORM_NONE, "local": NORM_LOCAL}

INPUT_EMBEDDING, INPUT_ONEHOT = 0, 1
INPUT_MODES = {"embedding": INPUT_EMBEDDING, "onehot": INPUT_ONEHOT}

SKIP_NONE, SKIP_HIGHWAY = 0, 1
SKIP_MODES = {"none": SKIP_NONE, "highway": SKIP_HIGHWAY}


def norm_mode_value(norm_mode):
    """RGCN_NORM_* value of a name (the `IncidenceNormalization` settings key) or of a number"""
    if isinstance(norm_mode, str):
        if norm_mode not in NORMS:
            raise ValueError("IncidenceNormalization / norm_mode must be one of %s, not %r"
                             % (", ".join(sorted(NORMS, key=NORMS.get)), norm_mode))
        return NORMS[norm_mode]
    return int(norm_mode)


class RgcnError(RuntimeError):
    def __init__(self, status, message):
        super().__init__("librgcn status %d: %s" % (status, message))
        self.status = status


class RgcnConfig(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32), ("device", C.c_int32), ("num_entities", C.c_int32),
        ("num_relations", C.c_int32), ("dim", C.c_int32), ("num_layers", C.c_int32),
        ("kind", C.c_int32), ("num_bases", C.c_int32), ("keep_prob", C.c_float),
        ("norm_mode", C.c_int32), ("max_edges", C.c_int64), ("rank", C.c_int32),
        ("world", C.c_int32), ("input_mode", C.c_int32),
    ]


class RgcnConfigExt(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("skip_mode", C.c_int32), ("code_dim", C.c_int32)]


class RgcnOptimizerParams(C.Structure):
    """rgcn_optimizer_params of include/rgcn.h"""
    _fields_ = [("struct_size", C.c_int32), ("algorithm", C.c_int32), ("learning_rate", C.c_float), ("beta1", C.c_float),
                ("beta2", C.c_float), ("epsilon", C.c_float), ("max_grad_norm", C.c_float),
                ("initial_accumulator", C.c_float)]


# [Algorithm] Name= of the settings file -> RGCN_OPT_*
OPT_ADAM, OPT_GRADIENT_DESCENT, OPT_ADAGRAD = 0, 1, 2
ALGORITHMS = {"Adam": OPT_ADAM, "GradientDescent": OPT_GRADIENT_DESCENT, "AdaGrad": OPT_ADAGRAD}
STATUS_INVALID = 1

_lib = None

_P = C.c_void_p
_SIGS = {
    "rgcn_abi_version": (C.c_int32, []),
    "rgcn_create": (C.c_int32, [C.POINTER(RgcnConfig), C.POINTER(_P)]),
    "rgcn_create_ex": (C.c_int32, [C.POINTER(RgcnConfig), C.POINTER(RgcnConfigExt), C.POINTER(_P)]),
    "rgcn_destroy": (C.c_int32, [_P]),
    "rgcn_last_error": (C.c_char_p, [_P]),
    "rgcn_sync": (C.c_int32, [_P]),
    "rgcn_param_count": (C.c_int32, [_P]),
    "rgcn_param_info": (C.c_int32, [_P, C.c_int32, C.c_char_p, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    "rgcn_set_param": (C.c_int32, [_P, C.c_int32, _P, C.c_int64]),
    "rgcn_get_param": (C.c_int32, [_P, C.c_int32, _P, C.c_int64]),
    "rgcn_get_grad": (C.c_int32, [_P, C.c_int32, _P, C.c_int64]),
    "rgcn_set_graph": (C.c_int32, [_P, _P, C.c_int64]),
    "rgcn_set_graph_device": (C.c_int32, [_P, _P, C.c_int64]),
    "rgcn_forward": (C.c_int32, [_P, C.c_int32, C.c_uint64, _P]),
    "rgcn_get_codes": (C.c_int32, [_P, _P, C.c_int64]),
    "rgcn_get_activation": (C.c_int32, [_P, C.c_int32, _P, C.c_int64]),
    "rgcn_get_dropout_mask": (C.c_int32, [_P, C.c_int32, _P, C.c_int64]),
    "rgcn_codes_device": (_P, [_P]),
    "rgcn_backward": (C.c_int32, [_P, _P, C.c_int64]),
    "rgcn_backward_device": (C.c_int32, [_P, _P]),
    "rgcn_step_device": (C.c_int32, [_P, _P, C.c_int64, C.c_int32, C.c_uint64, _P]),
    "rgcn_decoder_reserve": (C.c_int32, [_P, C.c_int64]),
    "rgcn_decoder_loss_backward_device": (C.c_int32, [_P, _P, _P, C.c_int64, C.c_float]),
    "rgcn_dcodes_device": (_P, [_P]),
    "rgcn_get_loss": (C.c_int32, [_P, C.POINTER(C.c_double)]),
    "rgcn_optimizer_config": (C.c_int32, [_P, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float]),
    "rgcn_sampler_create": (C.c_int32, [_P, C.c_int64, C.c_int32, C.POINTER(_P)]),
    "rgcn_sampler_destroy": (None, [_P]),
    "rgcn_sampler_edge_neighborhood": (C.c_int32, [_P, C.c_int64, C.c_uint64, _P]),
    "rgcn_neighborhood_reserve": (C.c_int32, [_P, _P, C.c_int64]),
    "rgcn_sample_neighborhood_device": (C.c_int32, [_P, C.c_int64, C.c_uint64, _P, C.c_int32]),
    "rgcn_capture_begin": (C.c_int32, [_P]),
    "rgcn_capture_end": (C.c_int32, [_P, C.POINTER(C.c_int32)]),
    "rgcn_graph_launch": (C.c_int32, [_P, C.c_int32]),
    "rgcn_graph_destroy": (C.c_int32, [_P, C.c_int32]),
    "rgcn_negative_sample_device": (C.c_int32, [_P, _P, C.c_int64, C.c_int32, C.c_uint64, _P, _P]),
    "rgcn_known_positives_reserve": (C.c_int32, [_P, _P, C.c_int64]),
    "rgcn_negative_sample_exclusive_device": (C.c_int32, [_P, _P, C.c_int64, C.c_int32, C.c_uint64, _P, _P]),
    "rgcn_set_exclusive_negatives": (C.c_int32, [_P, C.c_int32]),
    "rgcn_negative_sample_relation_device": (C.c_int32, [_P, _P, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_uint64,
                                                         _P, _P]),
    "rgcn_set_relation_negatives": (C.c_int32, [_P, C.c_int32]),
    "rgcn_type_sets_reserve": (C.c_int32, [_P, _P, C.c_int64]),
    "rgcn_negative_sample_typed_device": (C.c_int32, [_P, _P, C.c_int64, C.c_int32, C.c_int32, C.c_uint64, _P, _P]),
    "rgcn_set_typed_negatives": (C.c_int32, [_P, C.c_int32]),
    "rgcn_reciprocal_rows_device": (C.c_int32, [_P, _P, C.c_int64, C.c_int32, C.c_int32, C.c_uint64, _P, _P]),
    "rgcn_set_reciprocal_relations": (C.c_int32, [_P, C.c_int32]),
    "rgcn_rank_typed_device": (C.c_int32, [_P, _P, C.c_int64, C.c_int32, _P, _P, _P, _P]),
    "rgcn_topk_typed_device": (C.c_int32, [_P, _P, C.c_int64, C.c_int32, C.c_int32, _P, _P, _P, _P]),
    "rgcn_relation_softmax_reserve": (C.c_int32, [_P, C.c_int64]),
    "rgcn_relation_softmax_device": (C.c_int32, [_P, _P, C.c_int64, C.c_float, C.c_int32]),
    "rgcn_set_relation_softmax": (C.c_int32, [_P, C.c_float, C.c_int64, C.c_int32]),
    "rgcn_relation_softmax_plan": (C.c_int32, [C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_int64)]),
    "rgcn_decoder_loss_backward_weighted_device": (C.c_int32, [_P, _P, _P, _P, C.c_int64, C.c_float]),
    "rgcn_adversarial_weights_device": (C.c_int32, [_P, _P, C.c_int64, C.c_int64, C.c_float, _P]),
    "rgcn_set_adversarial_negatives": (C.c_int32, [_P, C.c_float, C.c_int64]),
    "rgcn_entity_softmax_reserve": (C.c_int32, [_P, C.c_int64]),
    "rgcn_entity_softmax_device": (C.c_int32, [_P, _P, C.c_int64, C.c_float, C.c_int32]),
    "rgcn_set_entity_softmax": (C.c_int32, [_P, C.c_float, C.c_int64, C.c_int32]),
    "rgcn_entity_softmax_plan": (C.c_int32, [C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_int64)]),
    "rgcn_rank_reserve": (C.c_int32, [_P, C.c_int64]),
    "rgcn_rank_device": (C.c_int32, [_P, _P, C.c_int64, C.c_int32, _P, _P, _P, _P]),
    "rgcn_rank_energies_device": (_P, [_P]),
    "rgcn_rank_mixed_device": (C.c_int32, [_P, _P, C.c_int64, C.c_int32, _P, C.c_float, _P, _P, _P, _P]),
    "rgcn_topk_device": (C.c_int32, [_P, _P, C.c_int64, C.c_int32, C.c_int32, _P, _P, _P, _P]),
    "rgcn_score_queries_device": (C.c_int32, [_P, _P, C.c_int64, C.c_int32]),
    "rgcn_topk_mixed_device": (C.c_int32, [_P, _P, C.c_int64, C.c_int32, C.c_int32, _P, C.c_float, _P, _P, _P, _P]),
    "rgcn_score_relation_queries_device": (C.c_int32, [_P, _P, C.c_int64]),
    "rgcn_relation_energies_device": (_P, [_P]),
    "rgcn_rank_relation_device": (C.c_int32, [_P, _P, C.c_int64, _P, _P, _P, _P]),
    "rgcn_topk_relation_device": (C.c_int32, [_P, _P, C.c_int64, C.c_int32, _P, _P, _P, _P]),
    "rgcn_optimizer_config_ex": (C.c_int32, [_P, C.POINTER(RgcnOptimizerParams)]),
    "rgcn_optimizer_slot_count": (C.c_int32, [_P]),
    "rgcn_get_optimizer_slot": (C.c_int32, [_P, C.c_int32, C.c_int32, _P, C.c_int64]),
    "rgcn_set_optimizer_slot": (C.c_int32, [_P, C.c_int32, C.c_int32, _P, C.c_int64]),
    "rgcn_get_optimizer_step": (C.c_int32, [_P, C.POINTER(C.c_int64)]),
    "rgcn_set_optimizer_step": (C.c_int32, [_P, C.c_int64]),
    "rgcn_optimizer_step": (C.c_int32, [_P]),
    "rgcn_optimizer_norm_partial": (C.c_int32, [_P]),
    "rgcn_optimizer_apply": (C.c_int32, [_P]),
    "rgcn_train_step_device": (C.c_int32, [_P, _P, C.c_int64, _P, _P, C.c_int64, C.c_uint64, C.c_float]),
    "rgcn_prefetch_graph_device": (C.c_int32, [_P, _P, C.c_int64]),
    "rgcn_prefetch_graph_dropout_device": (C.c_int32, [_P, _P, C.c_int64, C.c_int64, C.c_uint64]),
    "rgcn_set_graph_dropout_device": (C.c_int32, [_P, _P, C.c_int64, C.c_int64, C.c_uint64, _P]),
    "rgcn_get_graph_edges": (C.c_int32, [_P, _P, C.c_int64]),
    "rgcn_train_step_minibatch_device": (C.c_int32, [_P, _P, C.c_int64, C.c_int64, C.c_uint64, C.c_int32, C.c_uint64,
                                                     _P, _P, C.c_uint64, C.c_float]),
    "rgcn_set_relation_owner": (C.c_int32, [_P, _P, C.c_int32]),
    "rgcn_comm_unique_id": (C.c_int32, [_P]),
    "rgcn_comm_init": (C.c_int32, [_P, _P]),
    "rgcn_comm_allreduce_sum": (C.c_int32, [_P, _P, C.c_int64]),
    "rgcn_forward_begin": (C.c_int32, [_P, C.c_int32, C.c_uint64, _P]),
    "rgcn_forward_layer_partial": (C.c_int32, [_P, C.c_int32]),
    "rgcn_forward_layer_finish": (C.c_int32, [_P, C.c_int32]),
    "rgcn_backward_begin": (C.c_int32, [_P, _P]),
    "rgcn_backward_layer_partial": (C.c_int32, [_P, C.c_int32]),
    "rgcn_backward_layer_finish": (C.c_int32, [_P, C.c_int32]),
    "rgcn_backward_end": (C.c_int32, [_P]),
    "rgcn_read_buffer": (C.c_int32, [_P, C.c_int32, _P, C.c_int64]),
    "rgcn_write_buffer": (C.c_int32, [_P, C.c_int32, _P, C.c_int64]),
    "rgcn_device_alloc": (C.c_int32, [_P, C.c_int64, C.POINTER(_P)]),
    "rgcn_device_free": (C.c_int32, [_P, _P]),
    "rgcn_copy_to_device": (C.c_int32, [_P, _P, _P, C.c_int64]),
    "rgcn_copy_to_device_async": (C.c_int32, [_P, _P, _P, C.c_int64, C.c_int32]),
    "rgcn_copy_to_host": (C.c_int32, [_P, _P, _P, C.c_int64]),
    "rgcn_timer_start": (C.c_int32, [_P]),
    "rgcn_timer_stop": (C.c_int32, [_P, C.POINTER(C.c_float)]),
    "rgcn_set_overlap": (C.c_int32, [_P, C.c_int32]),
    "rgcn_set_gemm_mode": (C.c_int32, [_P, C.c_int32]),
    "rgcn_set_fusion": (C.c_int32, [_P, C.c_int32]),
    "rgcn_comm_info": (C.c_int32, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "rgcn_device_info": (C.c_int32, [C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "rgcn_profile_enable": (C.c_int32, [_P, C.c_int32]),
    "rgcn_profile_reset": (C.c_int32, [_P]),
    "rgcn_profile_count": (C.c_int32, [_P]),
    "rgcn_profile_get_compulsory": (C.c_int32, [_P, C.c_int32, C.POINTER(C.c_double)]),
    "rgcn_profile_get": (C.c_int32, [_P, C.c_int32, C.c_char_p, C.c_int32, C.POINTER(C.c_int64),
                                    C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
}
# librgcn_devtools.so only (include/rgcn_devtools.h)
_DEVTOOLS_SIGS = {
    "rgcn_debug_gemm": (C.c_int32, [_P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P]),
    "rgcn_debug_xcd_map": (C.c_int32, [_P, C.c_int32, _P]),
    "rgcn_debug_device_memory": (C.c_int32, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "rgcn_debug_gemm_presplit": (C.c_int32, [_P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P,
                                             C.POINTER(C.c_float)]),
    "rgcn_debug_gemm_time": (C.c_int32, [_P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                         C.c_int32, _P, _P, C.POINTER(C.c_float)]),
    "rgcn_debug_gemm_prologue": (C.c_int32, [_P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                             C.c_int32, _P, _P, _P, _P, _P]),
    "rgcn_debug_gemm_call": (C.c_int32, [_P, _P, _P, _P, _P, _P]),
}


class DebugGemmDesc(C.Structure):
    """rgcn_debug_gemm_desc of include/rgcn_devtools.h"""
    _fields_ = [("a_kc", C.c_int32), ("b_kc", C.c_int32), ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32),
                ("lda", C.c_int32), ("ldb", C.c_int32), ("ldc", C.c_int32), ("split_k", C.c_int32), ("groups", C.c_int32),
                ("strideA", C.c_int64), ("strideB", C.c_int64), ("strideC", C.c_int64), ("limit", C.c_void_p),
                ("limit_stride", C.c_int32), ("limit_on_k", C.c_int32), ("presplit_b", C.c_int32), ("wide", C.c_int32),
                ("w8_knob", C.c_int32), ("a_offset", C.c_int32), ("b_offset", C.c_int32), ("c_offset", C.c_int32),
                ("a_floats", C.c_int64), ("b_floats", C.c_int64), ("c_floats", C.c_int64)]


GEMM_KERNEL_NAMES = ("none", "f32", "staged", "presplit", "w8")      # GemmKernel of csrc/gemm_plan.h


class DebugGemmPlan(C.Structure):
    """rgcn_debug_gemm_plan of include/rgcn_devtools.h: the plan a rgcn_debug_gemm_call obeyed"""
    _fields_ = [(n, C.c_int32) for n in ("kernel", "terms", "vec", "vecC", "table", "prologue", "swizzle", "splits",
                                         "k_per_split", "slabs", "ldc", "tiles_m", "tiles_n", "grid_x", "grid_y")]

    def as_dict(self):
        out = {n: int(getattr(self, n)) for n, _ in self._fields_}
        out["kernel"] = GEMM_KERNEL_NAMES[out["kernel"]]
        return out
_lib_devtools = None


def relation_softmax_plan(max_positives, num_relations, code_dim):
    """rgcn_relation_softmax_plan: how a context of these sizes cuts the relation-softmax term's work (context-free, no
    GPU): the chunk of positives, the padded relation count, the split of the relation gradient's product, the entity side's
    long-row cut and piece"""
    lib = load_library()
    out = (C.c_int64 * 5)()
    st = lib.rgcn_relation_softmax_plan(int(max_positives), int(num_relations), int(code_dim), out)
    if st != 0:
        raise RgcnError(st, "rgcn_relation_softmax_plan: arguments must be positive")
    return {"chunk": int(out[0]), "padded_r": int(out[1]), "split_k": int(out[2]), "long_row": int(out[3]),
            "piece": int(out[4])}


def entity_softmax_plan(max_positives, num_entities, code_dim):
    """rgcn_entity_softmax_plan: how a context of these sizes cuts the entity-softmax term's work (context-free, no GPU):
    the chunk of rows (two per positive), the padded entity count, the split of the candidate gradient's product, the
    query side's long-row cut and piece"""
    lib = load_library()
    out = (C.c_int64 * 5)()
    st = lib.rgcn_entity_softmax_plan(int(max_positives), int(num_entities), int(code_dim), out)
    if st != 0:
        raise RgcnError(st, "rgcn_entity_softmax_plan: arguments must be positive")
    return {"chunk": int(out[0]), "padded_v": int(out[1]), "split_k": int(out[2]), "long_row": int(out[3]),
            "piece": int(out[4])}


def exported_symbols():
    """Names this binding expects librgcn.so to export (checked against include/rgcn.h in tests)."""
    return sorted(_SIGS)


def exported_devtools_symbols():
    return sorted(_DEVTOOLS_SIGS)


def load_library(path=None, devtools=False):
    """dlopen librgcn.so and attach prototypes.  Raises ImportError (never falls back) if missing.
    devtools=True: librgcn_devtools.so, the same sources plus the stand-alone GEMM entry points."""
    global _lib, _lib_devtools
    if devtools:
        if _lib_devtools is None or path is not None:
            p = path or os.path.join(os.path.dirname(LIB_PATH), "librgcn_devtools.so")
            if not os.path.exists(p):
                raise ImportError("%s not found: python -m relationprediction_amd.build makes it" % p)
            lib = C.CDLL(p, mode=C.RTLD_LOCAL)
            for name, (res, args) in list(_SIGS.items()) + list(_DEVTOOLS_SIGS.items()):
                fn = getattr(lib, name)
                fn.restype = res
                fn.argtypes = args
            if path is not None:
                return lib
            _lib_devtools = lib
        return _lib_devtools
    if _lib is not None and path is None:
        return _lib
    if path is None and os.environ.get("RGCN_LIBRARY") == "devtools":
        # the multi-process tests run their ranks on the devtools build: only that one honours RGCN_RCCL_LIBRARY
        _lib = load_library(devtools=True)
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise ImportError(
            "%s not found: build the HIP library first (python -m relationprediction_amd.build, or "
            "__graft_entry__.build()).  There is no CPU fallback." % p)
    lib = C.CDLL(p, mode=C.RTLD_GLOBAL)
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)   # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if lib.rgcn_abi_version() != ABI_VERSION:
        raise ImportError("librgcn.so ABI version %d != binding %d" % (lib.rgcn_abi_version(), ABI_VERSION))
    if path is None:
        _lib = lib
    return lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class DeviceBuffer:
    """A raw device allocation owned through the engine (no torch needed)."""

    def __init__(self, engine, nbytes):
        self.engine = engine
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        engine._check(engine.lib.rgcn_device_alloc(engine.ctx, self.nbytes, C.byref(p)))
        self.ptr = p

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes == self.nbytes, (arr.nbytes, self.nbytes)
        self.engine._check(self.engine.lib.rgcn_copy_to_device(self.engine.ctx, self.ptr, _ptr(arr), arr.nbytes))
        return self

    def download(self, dtype, shape):
        out = np.empty(shape, dtype=dtype)
        assert out.nbytes <= self.nbytes
        self.engine._check(self.engine.lib.rgcn_copy_to_host(self.engine.ctx, _ptr(out), self.ptr, out.nbytes))
        return out

    def free(self):
        if self.ptr is not None and self.engine.ctx is not None:
            self.engine.lib.rgcn_device_free(self.engine.ctx, self.ptr)
        self.ptr = None


class NeighborhoodSampler:
    """sample_edge_neighborhood of the reference's train loop (code/train.py:161-198) in O(log V) per pick
    (include/rgcn.h rgcn_sampler_*).  Host only: needs the library, not a GPU."""

    def __init__(self, triples, num_entities):
        self.lib = load_library()
        t = np.ascontiguousarray(triples, dtype=np.int32).reshape(-1, 3)
        self.n = len(t)
        h = C.c_void_p()
        st = self.lib.rgcn_sampler_create(_ptr(t), self.n, int(num_entities), C.byref(h))
        if st != 0:
            raise RgcnError(st, "rgcn_sampler_create (ids out of range or empty graph)")
        self.handle = h

    def sample(self, sample_size, seed):
        out = np.empty(int(sample_size), dtype=np.int32)
        st = self.lib.rgcn_sampler_edge_neighborhood(self.handle, int(sample_size), C.c_uint64(int(seed)), _ptr(out))
        if st != 0:
            raise RgcnError(st, "rgcn_sampler_edge_neighborhood (sample_size %d of %d edges)" % (sample_size, self.n))
        return out

    def close(self):
        if getattr(self, "handle", None) is not None:
            self.lib.rgcn_sampler_destroy(self.handle)
            self.handle = None

    __del__ = close


class Engine:
    """One rgcn_ctx: the encoder (input layer + L relational graph-convolution layers) on one GPU.
    kind "embedding" with num_layers 0 and num_bases 1: the graph-less DistMult baseline (Encoder.Name=embedding), whose
    codes are W_emb itself -- no set_graph, train_step_device(None, 0, ...); RGCN_KIND_EMBEDDING in include/rgcn.h.
    input_mode "embedding": AffineTransform under the layers (UseInputTransform=Yes); "onehot": no input layer, the
    first basis layer reads per-entity tables (UseInputTransform=No; include/rgcn.h RGCN_INPUT_ONEHOT).
    skip "highway": every layer wrapped in a highway layer (SkipConnections=Highway; RGCN_SKIP_HIGHWAY), created through
    rgcn_create_ex; skip "none" goes through rgcn_create.  create_ex (tests): True = rgcn_create_ex with the extension
    struct whatever `skip` is, "null" = rgcn_create_ex with a NULL extension.
    code_dim c (UseOutputTransform=Yes; rgcn_config_ext::code_dim): a dense output layer codes = H_L . W_out + b_out on top
    of the last layer, also when c == dim; the code side -- codes(), backward(), dcodes(), W_relation, every ranking and
    top-k call -- is self.dc = c wide, the layer stack keeps self.d.  None or 0: no such layer, self.dc == self.d.
    ext_struct_size (tests): the struct_size the extension struct announces instead of its own size."""

    def __init__(self, num_entities, num_relations, dim, num_layers, kind, num_bases, keep_prob=0.8,
                 norm_mode="intended", max_edges=0, device=0, rank=0, world=1, devtools=False, input_mode="embedding",
                 skip="none", create_ex=None, code_dim=None, ext_struct_size=None):
        self.lib = load_library(devtools=devtools)
        self.ctx = None
        cfg = RgcnConfig()
        cfg.abi_version = ABI_VERSION
        cfg.device = int(device)
        cfg.num_entities = int(num_entities)
        cfg.num_relations = int(num_relations)
        cfg.dim = int(dim)
        cfg.num_layers = int(num_layers)
        cfg.kind = KINDS[kind] if isinstance(kind, str) else int(kind)
        cfg.num_bases = int(num_bases)
        cfg.keep_prob = float(keep_prob)
        cfg.norm_mode = norm_mode_value(norm_mode)
        cfg.max_edges = int(max_edges)
        cfg.rank = int(rank)
        cfg.world = int(world)
        cfg.input_mode = INPUT_MODES[input_mode] if isinstance(input_mode, str) else int(input_mode)
        self.cfg = cfg
        ctx = C.c_void_p()
        skip_mode = SKIP_MODES[skip] if isinstance(skip, str) else int(skip)
        if create_ex == "null":
            st = self.lib.rgcn_create_ex(C.byref(cfg), None, C.byref(ctx))
        elif skip_mode == SKIP_NONE and not create_ex and code_dim is None and ext_struct_size is None:
            st = self.lib.rgcn_create(C.byref(cfg), C.byref(ctx))
        else:
            ext = RgcnConfigExt(C.sizeof(RgcnConfigExt) if ext_struct_size is None else int(ext_struct_size), skip_mode,
                                int(code_dim or 0))
            st = self.lib.rgcn_create_ex(C.byref(cfg), C.byref(ext), C.byref(ctx))
        if st != 0:
            raise RgcnError(st, (self.lib.rgcn_last_error(None) or b"").decode())
        self.ctx = ctx
        self.V, self.R, self.d, self.L = cfg.num_entities, cfg.num_relations, cfg.dim, cfg.num_layers
        # the code width: the library read code_dim only from an extension struct of the current size
        self.dc = int(code_dim) if code_dim and create_ex != "null" and ext_struct_size in (None, C.sizeof(RgcnConfigExt)) \
            else self.d
        # what the methods below size their arrays by: callers hang attributes of their own on an engine (the sharded test
        # worker keeps its dcodes buffer in `e.dc`), which must not change what the binding hands the library
        self._code_width = self.dc
        self.max_edges = int(cfg.max_edges)
        self.param_names, self.param_shapes = [], []
        for i in range(self.lib.rgcn_param_count(self.ctx)):
            name = C.create_string_buffer(64)
            shape = (C.c_int64 * 4)()
            nd = C.c_int32()
            self._check(self.lib.rgcn_param_info(self.ctx, i, name, 64, shape, C.byref(nd)))
            self.param_names.append(name.value.decode())
            self.param_shapes.append(tuple(int(shape[k]) for k in range(nd.value)))

    # -- plumbing
    def _check(self, st):
        if st != 0:
            raise RgcnError(st, (self.lib.rgcn_last_error(self.ctx) or b"").decode())

    def close(self):
        if self.ctx is not None:
            if getattr(self, "_rank_buf", None) is not None:
                self._rank_buf.free()
                self._rank_buf = None
            self.lib.rgcn_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def sync(self):
        self._check(self.lib.rgcn_sync(self.ctx))

    def _index(self, key):
        return key if isinstance(key, int) else self.param_names.index(key)

    # -- parameters
    def set_param(self, key, value):
        i = self._index(key)
        a = np.ascontiguousarray(value, dtype=np.float32)
        if tuple(a.shape) != self.param_shapes[i]:
            raise ValueError("%s: shape %s != %s" % (self.param_names[i], a.shape, self.param_shapes[i]))
        self._check(self.lib.rgcn_set_param(self.ctx, i, _ptr(a), a.size))

    def set_params(self, params):
        for n in self.param_names:
            self.set_param(n, params[n])

    def get_param(self, key):
        i = self._index(key)
        out = np.empty(self.param_shapes[i], dtype=np.float32)
        self._check(self.lib.rgcn_get_param(self.ctx, i, _ptr(out), out.size))
        return out

    def get_grad(self, key):
        i = self._index(key)
        out = np.empty(self.param_shapes[i], dtype=np.float32)
        self._check(self.lib.rgcn_get_grad(self.ctx, i, _ptr(out), out.size))
        return out

    def get_grads(self):
        return {n: self.get_grad(n) for n in self.param_names}

    def get_params(self):
        return {n: self.get_param(n) for n in self.param_names}

    # -- graph
    def set_graph(self, triples):
        t = np.asarray(triples)
        if t.size == 0:
            t = np.zeros((0, 3), dtype=np.int32)
        if t.ndim != 2 or t.shape[1] != 3:
            raise ValueError("graph_edges must be [E,3]")
        if t.dtype != np.int32:
            # the reference feeds int64 numpy arrays into an int32 placeholder
            if t.size and (t.min() < -2 ** 31 or t.max() >= 2 ** 31):
                raise ValueError("ids do not fit int32")
            t = t.astype(np.int32)
        t = np.ascontiguousarray(t)
        self._check(self.lib.rgcn_set_graph(self.ctx, _ptr(t), t.shape[0]))
        self.num_edges = int(t.shape[0])

    def set_graph_device(self, dev_buffer, num_edges):
        self._check(self.lib.rgcn_set_graph_device(self.ctx, dev_buffer.ptr, int(num_edges)))
        self.num_edges = int(num_edges)

    def set_graph_dropout_device(self, batch_buffer, num_edges, keep, seed=0, keep_mask=None):
        """graph = exact-`keep` random subset of the batch's edges, drawn on the device (rgcn_set_graph_dropout_device);
        keep_mask: a DeviceBuffer with uint8 [num_edges] holding the caller's choice instead"""
        self._check(self.lib.rgcn_set_graph_dropout_device(self.ctx, batch_buffer.ptr, int(num_edges), int(keep),
                                                           C.c_uint64(seed), keep_mask.ptr if keep_mask else None))
        self.num_edges = int(keep)

    def graph_edges(self):
        """the [E,3] rows of the graph currently set (after edge dropout, if any)"""
        out = np.empty((self.num_edges, 3), dtype=np.int32)
        self._check(self.lib.rgcn_get_graph_edges(self.ctx, _ptr(out), self.num_edges))
        return out

    def prefetch_graph_dropout_device(self, batch_buffer, num_edges, keep, seed):
        self._check(self.lib.rgcn_prefetch_graph_dropout_device(self.ctx, batch_buffer.ptr, int(num_edges), int(keep),
                                                                C.c_uint64(seed)))

    def train_step_minibatch_device(self, batch_buffer, num_edges, keep, edge_seed, rate, negative_seed, x_dev, y_dev,
                                    seed=0, reg_param=0.01):
        self._check(self.lib.rgcn_train_step_minibatch_device(
            self.ctx, batch_buffer.ptr, int(num_edges), int(keep), C.c_uint64(edge_seed), int(rate),
            C.c_uint64(negative_seed), x_dev.ptr, y_dev.ptr, C.c_uint64(seed), C.c_float(reg_param)))
        self.num_edges = int(keep)
        self._decoder_rows = int(num_edges) * (int(rate) + 1 + getattr(self, "_relation_rate", 0) +
                                               (1 if getattr(self, "_reciprocal", False) else 0))

    def set_relation_owner(self, owner):
        o = np.ascontiguousarray(owner, dtype=np.int32)
        self._check(self.lib.rgcn_set_relation_owner(self.ctx, _ptr(o), o.size))

    # -- forward / backward
    def _masks(self, masks):
        if masks is None:
            return None, None
        m = np.ascontiguousarray(np.stack([np.asarray(x) for x in masks]).astype(np.uint8))
        if m.shape != (self.L, self.V, self.d):
            raise ValueError("dropout masks must be [L,V,d]")
        return m, _ptr(m)

    def forward(self, train=True, seed=0, masks=None):
        m, p = self._masks(masks)
        self._check(self.lib.rgcn_forward(self.ctx, 1 if train else 0, C.c_uint64(seed), p))

    def codes(self):
        out = np.empty((self.V, self._code_width), dtype=np.float32)
        self._check(self.lib.rgcn_get_codes(self.ctx, _ptr(out), out.size))
        return out

    def activation(self, layer):
        out = np.empty((self.V, self.d), dtype=np.float32)
        self._check(self.lib.rgcn_get_activation(self.ctx, int(layer), _ptr(out), out.size))
        return out

    def dropout_mask(self, layer):
        out = np.empty((self.V, self.d), dtype=np.uint8)
        self._check(self.lib.rgcn_get_dropout_mask(self.ctx, int(layer), _ptr(out), out.size))
        return out

    def backward(self, dcodes):
        g = np.ascontiguousarray(dcodes, dtype=np.float32)
        if g.shape != (self.V, self._code_width):
            raise ValueError("dcodes must be [V,d] ([V,code_dim] under an output transform)")
        self._check(self.lib.rgcn_backward(self.ctx, _ptr(g), g.size))

    def backward_device(self, dev_buffer):
        self._check(self.lib.rgcn_backward_device(self.ctx, dev_buffer.ptr))

    def step_device(self, triples_dev, num_edges, dcodes_dev, train=True, seed=0):
        self._check(self.lib.rgcn_step_device(self.ctx, triples_dev.ptr, int(num_edges), 1 if train else 0,
                                              C.c_uint64(seed), dcodes_dev.ptr))
        self.num_edges = int(num_edges)

    # -- decoder / optimizer / whole train step on the device
    def decoder_reserve(self, max_triples):
        self._check(self.lib.rgcn_decoder_reserve(self.ctx, int(max_triples)))

    def decoder_loss_backward_device(self, x_dev, y_dev, num_triples, reg_param):
        self._check(self.lib.rgcn_decoder_loss_backward_device(self.ctx, x_dev.ptr, y_dev.ptr, int(num_triples),
                                                               C.c_float(reg_param)))

    def backward_from_decoder(self):
        """encoder backward fed with the decoder's dL/dcodes (stays on the device)"""
        self._check(self.lib.rgcn_backward_device(self.ctx, self.lib.rgcn_dcodes_device(self.ctx)))

    def dcodes(self):
        out = np.empty((self.V, self._code_width), dtype=np.float32)
        self._check(self.lib.rgcn_copy_to_host(self.ctx, _ptr(out), self.lib.rgcn_dcodes_device(self.ctx), out.nbytes))
        return out

    def loss(self):
        v = C.c_double()
        self._check(self.lib.rgcn_get_loss(self.ctx, C.byref(v)))
        return float(v.value)

    def capture_begin(self):
        """Start recording device calls into a hipGraph (include/rgcn.h rgcn_capture_begin)."""
        self._check(self.lib.rgcn_capture_begin(self.ctx))

    def capture_end(self):
        gid = C.c_int32(-1)
        self._check(self.lib.rgcn_capture_end(self.ctx, C.byref(gid)))
        return int(gid.value)

    def graph_launch(self, graph_id):
        self._check(self.lib.rgcn_graph_launch(self.ctx, int(graph_id)))

    def graph_destroy(self, graph_id):
        self._check(self.lib.rgcn_graph_destroy(self.ctx, int(graph_id)))

    def neighborhood_reserve(self, train_triples):
        """the training graph to the device, once: what rgcn_sample_neighborhood_device draws graph batches from"""
        t = np.ascontiguousarray(train_triples, dtype=np.int32).reshape(-1, 3)
        self._check(self.lib.rgcn_neighborhood_reserve(self.ctx, _ptr(t), len(t)))
        self._nbr_edges = len(t)

    def sample_neighborhood_device(self, sample_size, seed, batch_dev, on_prefetch_stream=False):
        """sample_edge_neighborhood (code/train.py:161-198) on the device: [sample_size,3] rows into batch_dev"""
        self._check(self.lib.rgcn_sample_neighborhood_device(self.ctx, int(sample_size), C.c_uint64(int(seed)),
                                                             batch_dev.ptr, 1 if on_prefetch_stream else 0))

    def negative_sample_device(self, batch_dev, n, rate, seed, x_dev, y_dev, exclusive=False, relation_rate=0,
                               reciprocal=False):
        """X [n*(rate+1),3] and Y [n*(rate+1)] from the batch of n triples, all on the device.  exclusive: corruptions
        that are known positives (known_positives_reserve) are redrawn (rgcn_negative_sample_exclusive_device).
        relation_rate = m > 0: n*m rows (s, r', o) with a wrong relation follow, n*(rate+1+m) rows in all
        (rgcn_negative_sample_relation_device).  reciprocal: the reciprocal pass behind them (reciprocal_rows_device),
        n*(rate+2+m) rows in all."""
        if relation_rate:
            self._check(self.lib.rgcn_negative_sample_relation_device(
                self.ctx, batch_dev.ptr, int(n), int(rate), int(relation_rate), 1 if exclusive else 0,
                C.c_uint64(int(seed)), x_dev.ptr, y_dev.ptr))
        else:
            fn = self.lib.rgcn_negative_sample_exclusive_device if exclusive else self.lib.rgcn_negative_sample_device
            self._check(fn(self.ctx, batch_dev.ptr, int(n), int(rate), C.c_uint64(int(seed)), x_dev.ptr, y_dev.ptr))
        if reciprocal:
            self.reciprocal_rows_device(batch_dev, n, rate, relation_rate, seed, x_dev, y_dev)

    def reciprocal_rows_device(self, batch_dev, n, rate, relation_rate, seed, x_dev, y_dev):
        """the reciprocal pass over an X, Y one of the sampler calls filled with the same n, rate, relation_rate and seed
        (rgcn_reciprocal_rows_device): subject-replaced negatives take relation r + R, n inverse positives (s, r + R, o)
        follow the last row; the buffers hold n*(rate+2+relation_rate) rows"""
        self._check(self.lib.rgcn_reciprocal_rows_device(self.ctx, batch_dev.ptr, int(n), int(rate), int(relation_rate),
                                                         C.c_uint64(int(seed)), x_dev.ptr, y_dev.ptr))

    def set_reciprocal_relations(self, on):
        """reciprocal relations (rgcn_set_reciprocal_relations): (?, r, o) is asked of W_relation[R + r], the decoder takes
        relations in [0, 2R), the fused minibatch step trains on n*(rate+2+relation_rate) rows"""
        self._check(self.lib.rgcn_set_reciprocal_relations(self.ctx, 1 if on else 0))
        self._reciprocal = bool(on)

    def type_sets_reserve(self, triples):
        """the per-relation entity sets of `triples` (the training triples) to the device, once (rgcn_type_sets_reserve);
        an empty array releases them and switches the typed mode off"""
        t = np.ascontiguousarray(triples, dtype=np.int32).reshape(-1, 3)
        self._check(self.lib.rgcn_type_sets_reserve(self.ctx, _ptr(t) if len(t) else None, len(t)))

    def negative_sample_typed_device(self, batch_dev, n, rate, seed, x_dev, y_dev, exclusive=False):
        """negative_sample_device with every corruption drawn from the entities the type sets hold for that slot of the
        row's relation (rgcn_negative_sample_typed_device); exclusive: known positives are redrawn inside the list"""
        self._check(self.lib.rgcn_negative_sample_typed_device(self.ctx, batch_dev.ptr, int(n), int(rate),
                                                              1 if exclusive else 0, C.c_uint64(int(seed)), x_dev.ptr,
                                                              y_dev.ptr))

    def set_typed_negatives(self, on):
        """the negative sampling inside train_step_minibatch_device: the type-constrained one (True) or not"""
        self._check(self.lib.rgcn_set_typed_negatives(self.ctx, 1 if on else 0))

    def negative_typed_open(self):
        """negative rows, since the type sets were reserved, that the typed sampler drew over all entities"""
        out = np.zeros(1, dtype=np.int64)
        self._check(self.lib.rgcn_read_buffer(self.ctx, BUF_NEGATIVE_TYPED_OPEN, _ptr(out), out.nbytes))
        return int(out[0])

    def ranks_typed(self, triples, predict_object, filter_ptr, filter_idx):
        """ranks() among the members of the type set of (predict_object, relation) and the gold entity (include/rgcn.h
        rgcn_rank_typed_device)"""
        return self._ranks_staged(triples, filter_ptr, filter_idx,
                                  lambda n, x, ptr, idx, raw, filt: self.lib.rgcn_rank_typed_device(
                                      self.ctx, x, n, 1 if predict_object else 0, ptr, idx, raw, filt))

    def topk_typed(self, queries, predict_object, k, exclude_ptr=None, exclude_idx=None):
        """topk() among the members of the type set of (predict_object, relation) (include/rgcn.h
        rgcn_topk_typed_device)"""
        return self._topk_staged(queries, k, exclude_ptr, exclude_idx,
                                 lambda n, k, x, ptr, idx, ids, energies: self.lib.rgcn_topk_typed_device(
                                     self.ctx, x, n, 1 if predict_object else 0, k, ptr, idx, ids, energies))

    def set_relation_negatives(self, relation_rate):
        """relation rows per batch edge the negative sampling inside train_step_minibatch_device appends (0: none)"""
        self._check(self.lib.rgcn_set_relation_negatives(self.ctx, int(relation_rate)))
        self._relation_rate = int(relation_rate)

    def relation_softmax_reserve(self, max_positives):
        """size the relation-softmax term's buffers (rgcn_relation_softmax_reserve): one chunk of positives"""
        self._check(self.lib.rgcn_relation_softmax_reserve(self.ctx, int(max_positives)))
        # (a smaller request leaves the buffers as they are: the plan is that of the largest one)
        self._relsm_reserved = max(getattr(self, "_relsm_reserved", 0), int(max_positives))
        self._relsm_plan = relation_softmax_plan(self._relsm_reserved, self.R, self._code_width)

    def relation_softmax_device(self, positives_dev, num_positives, weight, exclusive=False):
        """add weight / P * sum_n [logsumexp over the relations of E[n, :] - E[n, r_n]] and its gradients to what the last
        decoder_loss_backward_device left (rgcn_relation_softmax_device); exclusive: relations known for the pair
        (known_positives_reserve) leave the candidate set"""
        self._check(self.lib.rgcn_relation_softmax_device(self.ctx, positives_dev.ptr, int(num_positives),
                                                         C.c_float(weight), 1 if exclusive else 0))

    def set_relation_softmax(self, weight, num_positives=0, exclusive=False):
        """the relation-softmax term inside the fused steps (rgcn_set_relation_softmax): train_step_minibatch_device takes
        its batch rows as the positives, train_step_device the first num_positives rows of X; weight 0 switches it off"""
        self._check(self.lib.rgcn_set_relation_softmax(self.ctx, C.c_float(weight), int(num_positives),
                                                      1 if exclusive else 0))

    def decoder_loss_backward_weighted_device(self, x_dev, y_dev, w_dev, num_triples, reg_param):
        """decoder_loss_backward_device with a weight per row (a float [N] device buffer) on the row's loss term and
        gradient (rgcn_decoder_loss_backward_weighted_device); w_dev None: that call itself"""
        self._check(self.lib.rgcn_decoder_loss_backward_weighted_device(
            self.ctx, x_dev.ptr, y_dev.ptr, w_dev.ptr if w_dev is not None else None, int(num_triples),
            C.c_float(reg_param)))

    def adversarial_weights(self, x_dev, num_triples, num_positives, temperature, w_out_dev):
        """the self-adversarial weights of a decoder batch whose first num_positives rows are the positives, for the codes
        of the last forward pass, into w_out_dev (rgcn_adversarial_weights_device): 1 for a positive, K softmax(temperature
        x energy) over its group for a negative"""
        self._check(self.lib.rgcn_adversarial_weights_device(self.ctx, x_dev.ptr if x_dev is not None else None,
                                                            int(num_triples), int(num_positives), C.c_float(temperature),
                                                            w_out_dev.ptr if w_out_dev is not None else None))

    def set_adversarial_negatives(self, temperature, num_positives=0):
        """self-adversarial weights inside the fused steps (rgcn_set_adversarial_negatives): train_step_minibatch_device
        takes its batch rows as the positives, train_step_device the first num_positives rows of X; temperature 0
        switches the mode off"""
        self._check(self.lib.rgcn_set_adversarial_negatives(self.ctx, C.c_float(temperature), int(num_positives)))

    def entity_softmax_reserve(self, max_positives):
        """size the entity-softmax term's buffers (rgcn_entity_softmax_reserve): one chunk of rows, two per positive"""
        self._check(self.lib.rgcn_entity_softmax_reserve(self.ctx, int(max_positives)))
        # (a smaller request leaves the buffers as they are: the plan is that of the largest one)
        self._entsm_reserved = max(getattr(self, "_entsm_reserved", 0), int(max_positives))
        self._entsm_plan = entity_softmax_plan(self._entsm_reserved, self.V, self._code_width)

    def entity_softmax_device(self, positives_dev, num_positives, weight, exclusive=False):
        """add weight / (2 P) * sum over the object and subject rows of [logsumexp over the entities of E[m, :] - E[m, g_m]]
        and its gradients to what the last decoder_loss_backward_device left (rgcn_entity_softmax_device); exclusive:
        entities known for the row's pair (known_positives_reserve) leave the candidate set"""
        self._check(self.lib.rgcn_entity_softmax_device(self.ctx, positives_dev.ptr, int(num_positives),
                                                       C.c_float(weight), 1 if exclusive else 0))

    def set_entity_softmax(self, weight, num_positives=0, exclusive=False):
        """the entity-softmax term inside the fused steps (rgcn_set_entity_softmax): train_step_minibatch_device takes its
        batch rows as the positives (the leading num_positives where that is smaller), train_step_device the first
        num_positives rows of X; weight 0 switches it off"""
        self._check(self.lib.rgcn_set_entity_softmax(self.ctx, C.c_float(weight), int(num_positives),
                                                    1 if exclusive else 0))

    def negative_relation_unresolved(self):
        """relation rows, since the reserve, for which every other relation was a known positive (they kept their first
        draw)"""
        out = np.zeros(1, dtype=np.int64)
        self._check(self.lib.rgcn_read_buffer(self.ctx, BUF_NEGATIVE_RELATION_UNRESOLVED, _ptr(out), out.nbytes))
        return int(out[0])

    def known_positives_reserve(self, triples):
        """the set of known positives to the device, once (NegativeSampler.set_known_positives); an empty set releases
        the index and switches the exclusive mode off"""
        t = np.ascontiguousarray(triples, dtype=np.int32).reshape(-1, 3)
        self._check(self.lib.rgcn_known_positives_reserve(self.ctx, _ptr(t) if len(t) else None, len(t)))

    def set_exclusive_negatives(self, on):
        """the negative sampling inside train_step_minibatch_device: the exclusive one (True) or the plain one"""
        self._check(self.lib.rgcn_set_exclusive_negatives(self.ctx, 1 if on else 0))

    def negative_unresolved(self):
        """negative rows, since the reserve, for which every entity was a known positive (they kept their first draw)"""
        out = np.zeros(1, dtype=np.int64)
        self._check(self.lib.rgcn_read_buffer(self.ctx, BUF_NEGATIVE_UNRESOLVED, _ptr(out), out.nbytes))
        return int(out[0])

    def rank_reserve(self, max_queries):
        self._check(self.lib.rgcn_rank_reserve(self.ctx, int(max_queries)))
        self._rank_reserved = max(getattr(self, "_rank_reserved", 0), int(max_queries))

    def ranks(self, triples, predict_object, filter_ptr, filter_idx):
        """Raw and filtered ranks (include/rgcn.h rgcn_rank_device) of the gold subject / object of every
        query triple on the codes of the last forward.  filter_ptr int64 [N+1], filter_idx int32 [nnz]."""
        return self._ranks_staged(triples, filter_ptr, filter_idx, lambda n, x, ptr, idx, raw, filt: self.lib.rgcn_rank_device(
            self.ctx, x, n, 1 if predict_object else 0, ptr, idx, raw, filt))

    def _stage_queries(self, x, list_ptr, list_idx, out_bytes):
        """ONE upload (list pointers | queries | list, packed) into a buffer the engine keeps, with room for out_bytes of
        answers behind it for ONE download: a call used to cost five device allocations, three blocking uploads and two
        downloads -- more host time than the scoring itself.  list_ptr int64 [N+1], list_idx int32 [nnz]: the filter or
        exclusion lists.  Returns the device addresses of (list pointers, queries, list, answers)."""
        n = len(x)
        fp = np.ascontiguousarray(list_ptr, dtype=np.int64)
        fi = np.ascontiguousarray(list_idx, dtype=np.int32)
        assert fp.shape == (n + 1,) and fp[-1] == len(fi)
        off_x, off_fi = 8 * (n + 1), 8 * (n + 1) + 12 * n
        off_out = (off_fi + 4 * max(len(fi), 1) + 7) // 8 * 8
        total = off_out + out_bytes
        if getattr(self, "_rank_buf", None) is None or self._rank_buf.nbytes < total:
            if getattr(self, "_rank_buf", None) is not None:
                self._rank_buf.free()
            self._rank_buf = DeviceBuffer(self, max(total, 1 << 20))
        base = self._rank_buf.ptr.value
        # staged through the library's pinned slots (<= 1 MB each), ordered on the main stream, no host wait: the list
        # (megabytes for the subject side of FB15k-237) travels while the queries are being scored
        head = np.concatenate([fp.view(np.uint8), x.reshape(-1).view(np.uint8)])
        for off, data in ((0, head), (off_fi, fi.view(np.uint8))):
            for lo in range(0, len(data), 1 << 20):
                part = data[lo:lo + (1 << 20)]
                self._check(self.lib.rgcn_copy_to_device_async(self.ctx, C.c_void_p(base + off + lo), _ptr(part), len(part), 0))
        return C.c_void_p(base), C.c_void_p(base + off_x), C.c_void_p(base + off_fi), base + off_out

    def _read_staged(self, address, count):
        out = np.empty(count, dtype=np.int32)
        self._check(self.lib.rgcn_copy_to_host(self.ctx, _ptr(out), C.c_void_p(address), out.nbytes))
        return out

    def _ranks_staged(self, triples, filter_ptr, filter_idx, call):
        """ranks and ranks_mixed: call(n, queries, filter pointers, filter list, raw out, filtered out) -> status"""
        x = np.ascontiguousarray(triples, dtype=np.int32).reshape(-1, 3)
        n = len(x)
        if n == 0:
            return np.zeros(0, np.int32), np.zeros(0, np.int32)
        ptr, xd, idx, out = self._stage_queries(x, filter_ptr, filter_idx, 8 * n)
        self._check(call(n, xd, ptr, idx, C.c_void_p(out), C.c_void_p(out + 4 * n)))
        r = self._read_staged(out, 2 * n)
        return r[:n].copy(), r[n:].copy()

    def _topk_staged(self, queries, k, exclude_ptr, exclude_idx, call):
        """topk and topk_mixed: call(n, k, queries, exclusion pointers, exclusion list, ids out, values out) -> status"""
        x = np.ascontiguousarray(queries, dtype=np.int32).reshape(-1, 3)
        n, k = len(x), int(k)
        if (exclude_ptr is None) != (exclude_idx is None):
            raise ValueError("exclude_ptr and exclude_idx come together")
        if n == 0:
            return np.zeros((0, max(k, 0)), np.int32), np.zeros((0, max(k, 0)), np.float32)
        has = exclude_ptr is not None
        room = min(max(k, 0), 1024)        # (a k outside [1, RGCN_MAX_TOPK] is the library's to refuse: it writes nothing)
        ptr, xd, idx, out = self._stage_queries(x, exclude_ptr if has else np.zeros(n + 1),
                                                exclude_idx if has else np.zeros(0), 8 * n * room)
        self._check(call(n, k, xd, ptr if has else None, idx if has else None, C.c_void_p(out),
                         C.c_void_p(out + 4 * n * room)))
        r = self._read_staged(out, 2 * n * k)
        return r[:n * k].reshape(n, k).copy(), r[n * k:].view(np.float32).reshape(n, k).copy()

    @contextlib.contextmanager
    def _partner_energies(self, partner, n):
        """the device address of `partner` -- a float32 [n, V] array (uploaded for the length of the `with`), a DeviceBuffer
        or a device address (n = 0: not looked at, the call returns its empty answer)"""
        if n == 0:
            yield None
        elif isinstance(partner, np.ndarray):
            e = np.ascontiguousarray(partner, dtype=np.float32)
            if e.shape != (n, self.V):
                raise ValueError("partner energies must be [%d, %d], not %s" % (n, self.V, e.shape))
            own = DeviceBuffer(self, e.nbytes).upload(e)
            try:
                yield own.ptr
            finally:
                own.free()
        else:
            yield partner.ptr if isinstance(partner, DeviceBuffer) else C.c_void_p(int(partner))

    def rank_energies_device(self):
        """device address of RGCN_BUF_RANK_ENERGIES (the [reserved queries, V] energies of the chunk scored last), or None
        before rank_reserve: what another engine's ranks_mixed takes as `partner` once this one has synchronised"""
        p = self.lib.rgcn_rank_energies_device(self.ctx)
        return int(p) if p else None

    def ranks_mixed(self, triples, predict_object, partner, weight, filter_ptr, filter_idx):
        """Raw and filtered ranks under weight * own score + (1 - weight) * partner score (include/rgcn.h
        rgcn_rank_mixed_device).  partner: the other model's energies for the same queries in the same order -- a
        float32 [N, V] numpy array (uploaded), a DeviceBuffer, or a device address (rank_energies_device() of another
        engine on the same GPU, complete and left alone until this call returns).  One chunk: N <= the reserve."""
        with self._partner_energies(partner, np.size(triples) // 3) as pp:
            return self._ranks_staged(triples, filter_ptr, filter_idx,
                                      lambda n, x, ptr, idx, raw, filt: self.lib.rgcn_rank_mixed_device(
                                          self.ctx, x, n, 1 if predict_object else 0, pp, C.c_float(float(weight)), ptr, idx,
                                          raw, filt))

    def topk(self, queries, predict_object, k, exclude_ptr=None, exclude_idx=None):
        """The k best completions of every query on the codes of the last forward, best first (include/rgcn.h
        rgcn_topk_device): (idx int32 [N,k], energy float32 [N,k]), rows short of k answers padded with (-1, -inf).
        queries [N,3] rows (s, r, o) of which the column being predicted is not read; exclude_ptr int64 [N+1] /
        exclude_idx int32 [nnz]: per-row ids that may not be answered (both None: none)."""
        return self._topk_staged(queries, k, exclude_ptr, exclude_idx,
                                 lambda n, k, x, ptr, idx, ids, energies: self.lib.rgcn_topk_device(
                                     self.ctx, x, n, 1 if predict_object else 0, k, ptr, idx, ids, energies))

    def score_queries(self, queries, predict_object):
        """Energies of every entity for each query into RGCN_BUF_RANK_ENERGIES and nothing else (include/rgcn.h
        rgcn_score_queries_device): what topk leaves there, for another engine's topk_mixed to read through
        rank_energies_device().  queries [N,3] rows (s, r, o) of which the predicted column is not read; one chunk: N <=
        the reserve.  Synchronises."""
        x = np.ascontiguousarray(queries, dtype=np.int32).reshape(-1, 3)
        if len(x) == 0:
            return
        xd = DeviceBuffer(self, x.nbytes).upload(x)
        try:
            self._check(self.lib.rgcn_score_queries_device(self.ctx, xd.ptr, len(x), 1 if predict_object else 0))
        finally:
            xd.free()

    def topk_mixed(self, queries, predict_object, k, partner, weight, exclude_ptr=None, exclude_idx=None):
        """topk() under weight * own score + (1 - weight) * partner score (include/rgcn.h rgcn_topk_mixed_device): (idx
        int32 [N,k], mixed score float32 [N,k]) ordered by (mixed score descending, entity id ascending), rows short of k
        answers padded with (-1, -inf).  partner as for ranks_mixed: the other model's energies for the same queries in the
        same order -- a float32 [N, V] numpy array (uploaded), a DeviceBuffer, or a device address
        (rank_energies_device() of another engine on the same GPU after its score_queries, left alone until this call
        returns).  One chunk: N <= the reserve."""
        with self._partner_energies(partner, np.size(queries) // 3) as pp:
            return self._topk_staged(queries, k, exclude_ptr, exclude_idx,
                                     lambda n, k, x, ptr, idx, ids, scores: self.lib.rgcn_topk_mixed_device(
                                         self.ctx, x, n, 1 if predict_object else 0, k, pp, C.c_float(float(weight)), ptr,
                                         idx, ids, scores))

    def score_relation_queries(self, queries):
        """Energies of every relation between s and o of each query into RGCN_BUF_RELATION_ENERGIES and nothing else
        (include/rgcn.h rgcn_score_relation_queries_device).  queries [N,3] rows (s, r, o) of which the r column is not
        read; one chunk: N <= the reserve.  Synchronises."""
        x = np.ascontiguousarray(queries, dtype=np.int32).reshape(-1, 3)
        if len(x) == 0:
            return
        xd = DeviceBuffer(self, x.nbytes).upload(x)
        try:
            self._check(self.lib.rgcn_score_relation_queries_device(self.ctx, xd.ptr, len(x)))
        finally:
            xd.free()

    def relation_energies_device(self):
        """device address of RGCN_BUF_RELATION_ENERGIES (the [reserved queries, R] energies of the chunk a relation query
        scored last), or None before the first relation query since rank_reserve"""
        p = self.lib.rgcn_relation_energies_device(self.ctx)
        return int(p) if p else None

    def ranks_relation(self, triples, filter_ptr, filter_idx):
        """Raw and filtered ranks (include/rgcn.h rgcn_rank_relation_device) of the gold relation of every query triple
        among all relations between its subject and object, on the codes of the last forward.  filter_ptr int64 [N+1],
        filter_idx int32 [nnz]: relation ids."""
        return self._ranks_staged(triples, filter_ptr, filter_idx,
                                  lambda n, x, ptr, idx, raw, filt: self.lib.rgcn_rank_relation_device(
                                      self.ctx, x, n, ptr, idx, raw, filt))

    def topk_relation(self, queries, k, exclude_ptr=None, exclude_idx=None):
        """The k best relations between s and o of every query, best first (include/rgcn.h rgcn_topk_relation_device):
        (idx int32 [N,k], energy float32 [N,k]), rows short of k answers padded with (-1, -inf).  queries [N,3] rows
        (s, r, o) of which r is not read; exclude_ptr int64 [N+1] / exclude_idx int32 [nnz]: per-row relation ids that
        may not be answered (both None: none)."""
        return self._topk_staged(queries, k, exclude_ptr, exclude_idx,
                                 lambda n, k, x, ptr, idx, ids, energies: self.lib.rgcn_topk_relation_device(
                                     self.ctx, x, n, k, ptr, idx, ids, energies))

    def optimizer_config(self, lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8, max_grad_norm=1.0, algorithm="Adam",
                         initial_accumulator=0.1, struct_size=None):
        """algorithm: "Adam", "GradientDescent" or "AdaGrad" (the settings' [Algorithm] Name=) or an RGCN_OPT_* number.
        Adam goes through rgcn_optimizer_config, the other two through rgcn_optimizer_config_ex.  struct_size (tests):
        rgcn_optimizer_config_ex whatever the algorithm, with a struct that announces this size."""
        if isinstance(algorithm, str):
            if algorithm not in ALGORITHMS:
                raise ValueError("Algorithm.Name must be one of %s, not %r" % (", ".join(ALGORITHMS), algorithm))
            algorithm = ALGORITHMS[algorithm]
        if algorithm == OPT_ADAM and struct_size is None:
            self._check(self.lib.rgcn_optimizer_config(self.ctx, lr, beta1, beta2, eps, max_grad_norm))
        else:
            p = RgcnOptimizerParams(C.sizeof(RgcnOptimizerParams) if struct_size is None else int(struct_size),
                                    int(algorithm), lr, beta1, beta2, eps, max_grad_norm, initial_accumulator)
            self._check(self.lib.rgcn_optimizer_config_ex(self.ctx, C.byref(p)))
        self._algorithm = int(algorithm)

    def optimizer_algorithm(self):
        """name of the configured algorithm"""
        number = getattr(self, "_algorithm", OPT_ADAM)
        return [k for k, v in ALGORITHMS.items() if v == number][0]

    def optimizer_slot_count(self):
        return int(self.lib.rgcn_optimizer_slot_count(self.ctx))

    def get_optimizer_slot(self, key, slot):
        i = self._index(key)
        out = np.empty(self.param_shapes[i], dtype=np.float32)
        self._check(self.lib.rgcn_get_optimizer_slot(self.ctx, i, int(slot), _ptr(out), out.size))
        return out

    def set_optimizer_slot(self, key, slot, value):
        i = self._index(key)
        a = np.ascontiguousarray(value, dtype=np.float32)
        if tuple(a.shape) != self.param_shapes[i]:
            raise ValueError("%s slot %d: shape %s != %s" % (self.param_names[i], slot, a.shape, self.param_shapes[i]))
        self._check(self.lib.rgcn_set_optimizer_slot(self.ctx, i, int(slot), _ptr(a), a.size))

    def optimizer_step_count(self):
        """steps taken, as the device counts them (replays of a captured graph included); synchronises"""
        t = C.c_int64()
        self._check(self.lib.rgcn_get_optimizer_step(self.ctx, C.byref(t)))
        return int(t.value)

    def set_optimizer_step_count(self, t):
        self._check(self.lib.rgcn_set_optimizer_step(self.ctx, int(t)))

    def optimizer_state(self):
        """{"algorithm": name, "step": count, "slots": {parameter name: [one array per slot, the parameter's shape]}} of
        every parameter the optimizer moves (a parameter without a gradient -- the unused layer bias -- has no entry);
        Adam: [m, v], AdaGrad: [accumulator], GradientDescent: []"""
        slots, count = {}, self.optimizer_slot_count()
        for name in self.param_names if count else ():
            try:
                slots[name] = [self.get_optimizer_slot(name, s) for s in range(count)]
            except RgcnError as e:
                if e.status != STATUS_INVALID:      # (RGCN_ERR_INVALID: the library's answer for a parameter without state)
                    raise
        return {"algorithm": self.optimizer_algorithm(), "step": self.optimizer_step_count(), "slots": slots}

    def set_optimizer_state(self, state):
        """Continue from an optimizer_state(): its algorithm must be the configured one (ValueError naming both)."""
        if state["algorithm"] != self.optimizer_algorithm():
            raise ValueError("optimizer state of %s, the configured algorithm is %s"
                             % (state["algorithm"], self.optimizer_algorithm()))
        for name, arrays in state["slots"].items():
            if len(arrays) != self.optimizer_slot_count():
                raise ValueError("%s: %d slots, %s has %d" % (name, len(arrays), state["algorithm"],
                                                              self.optimizer_slot_count()))
            for s, a in enumerate(arrays):
                self.set_optimizer_slot(name, s, a)
        self.set_optimizer_step_count(state["step"])

    def optimizer_step(self):
        self._check(self.lib.rgcn_optimizer_step(self.ctx))

    def optimizer_norm_partial(self):
        self._check(self.lib.rgcn_optimizer_norm_partial(self.ctx))

    def optimizer_apply(self):
        self._check(self.lib.rgcn_optimizer_apply(self.ctx))

    def train_step_device(self, triples_dev, num_edges, x_dev, y_dev, num_triples, seed=0, reg_param=0.01):
        """triples_dev None (with num_edges 0): the graph-less step of an "embedding" engine"""
        self._check(self.lib.rgcn_train_step_device(self.ctx, triples_dev.ptr if triples_dev is not None else None,
                                                    int(num_edges), x_dev.ptr, y_dev.ptr,
                                                    int(num_triples), C.c_uint64(seed), C.c_float(reg_param)))
        self.num_edges = int(num_edges)
        self._decoder_rows = int(num_triples)

    def prefetch_graph_device(self, triples_dev, num_edges):
        self._check(self.lib.rgcn_prefetch_graph_device(self.ctx, triples_dev.ptr, int(num_edges)))

    # -- phase API (sharding exchange points)
    def forward_begin(self, train=True, seed=0, masks=None):
        m, p = self._masks(masks)
        self._check(self.lib.rgcn_forward_begin(self.ctx, 1 if train else 0, C.c_uint64(seed), p))

    def forward_layer_partial(self, l):
        self._check(self.lib.rgcn_forward_layer_partial(self.ctx, l))

    def forward_layer_finish(self, l):
        self._check(self.lib.rgcn_forward_layer_finish(self.ctx, l))

    def backward_begin(self, dcodes_dev=None):
        """dcodes_dev None: the decoder's own dL/dcodes (rgcn_dcodes_device), which never leaves the device"""
        ptr = self.lib.rgcn_dcodes_device(self.ctx) if dcodes_dev is None else dcodes_dev.ptr
        self._check(self.lib.rgcn_backward_begin(self.ctx, ptr))

    def backward_layer_partial(self, l):
        self._check(self.lib.rgcn_backward_layer_partial(self.ctx, l))

    def backward_layer_finish(self, l):
        self._check(self.lib.rgcn_backward_layer_finish(self.ctx, l))

    def backward_end(self):
        self._check(self.lib.rgcn_backward_end(self.ctx))

    def read_buffer(self, which):
        if which in (BUF_INDEG, BUF_OUTDEG):
            out = np.empty(self.V, dtype=np.int32)
        elif which == BUF_ROWPTR:
            out = np.empty(self.V + 1, dtype=np.int32)
        elif which in (BUF_PERM_VERTEX, BUF_PERM_RELATION):
            out = np.empty(2 * self.num_edges, dtype=np.int32)
        elif which == BUF_MSG_NORM:
            out = np.empty(2 * self.num_edges, dtype=np.float32)
        elif which in (BUF_RANK_ENERGIES, BUF_RANK_MIXED_SCORES):
            out = np.empty((getattr(self, "_rank_reserved", 0), self.V), dtype=np.float32)
        elif which == BUF_RELATION_ENERGIES:
            out = np.empty((getattr(self, "_rank_reserved", 0), self.R), dtype=np.float32)
        elif which in (BUF_RELATION_SOFTMAX_ENERGIES, BUF_RELATION_SOFTMAX_G, BUF_RELATION_SOFTMAX_DQ):
            plan = getattr(self, "_relsm_plan", {"chunk": 0, "padded_r": 0})
            cols = self._code_width if which == BUF_RELATION_SOFTMAX_DQ else plan["padded_r"]
            out = np.empty((plan["chunk"], cols), dtype=np.float32)
        elif which == BUF_ADVERSARIAL_WEIGHTS:
            out = np.empty(getattr(self, "_decoder_rows", 0), dtype=np.float32)
        elif which in (BUF_ENTITY_SOFTMAX_G, BUF_ENTITY_SOFTMAX_DQ):
            plan = getattr(self, "_entsm_plan", {"chunk": 0, "padded_v": 0})
            cols = self._code_width if which == BUF_ENTITY_SOFTMAX_DQ else plan["padded_v"]
            out = np.empty((plan["chunk"], cols), dtype=np.float32)
        elif which == BUF_DSELF_EXCHANGE:
            out = np.empty((self.d, self.d), dtype=np.float32)
        elif which == BUF_NORM_EXCHANGE:
            out = np.empty(1, dtype=np.float32)
        elif which == BUF_DBASIS_EXCHANGE:
            out = np.empty((2, int(self.cfg.num_bases), self.d, self.d), dtype=np.float32)
        elif which == BUF_TDIAG_PRODUCTS:
            out = np.empty((2, self.V, int(self.cfg.num_bases) * self.d), dtype=np.float32)
        elif which == BUF_PDIAG_MIX:
            out = np.empty((2, self.V, int(self.cfg.num_bases)), dtype=np.float32)
        else:
            out = np.empty((self.V, self.d), dtype=np.float32)
        self._check(self.lib.rgcn_read_buffer(self.ctx, which, _ptr(out), out.nbytes))
        return out

    def write_buffer(self, which, arr):
        a = np.ascontiguousarray(arr, dtype=np.float32)
        self._check(self.lib.rgcn_write_buffer(self.ctx, which, _ptr(a), a.nbytes))

    # -- communicator
    @staticmethod
    def comm_unique_id():
        lib = load_library()
        buf = (C.c_uint8 * 128)()
        st = lib.rgcn_comm_unique_id(buf)
        if st != 0:
            raise RgcnError(st, (lib.rgcn_last_error(None) or b"").decode())
        return bytes(buf)

    @staticmethod
    def device_info(device=0):
        """(HIP devices this process sees, PCI address of `device` as domain << 16 | bus << 8 | device, or -1)"""
        lib = load_library()
        n, pci = C.c_int32(0), C.c_int64(-1)
        st = lib.rgcn_device_info(int(device), C.byref(n), C.byref(pci))
        if st != 0:
            raise RgcnError(st, (lib.rgcn_last_error(None) or b"").decode())
        return n.value, pci.value

    def comm_init(self, unique_id):
        buf = (C.c_uint8 * 128).from_buffer_copy(bytes(unique_id))
        self._check(self.lib.rgcn_comm_init(self.ctx, buf))

    def comm_info(self):
        """(ranks the collective library's communicator sees, this rank's index in it, its device); -1: unknown / none"""
        n, r, dev = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
        self._check(self.lib.rgcn_comm_info(self.ctx, C.byref(n), C.byref(r), C.byref(dev)))
        return n.value, r.value, dev.value

    def comm_allreduce_sum(self, dev_buffer, count):
        self._check(self.lib.rgcn_comm_allreduce_sum(self.ctx, dev_buffer.ptr, int(count)))

    # -- device memory / timing / profile
    def alloc(self, nbytes):
        return DeviceBuffer(self, nbytes)

    def copy_to_device(self, buf, arr):
        """Upload into the front of an existing (possibly larger) device buffer."""
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= buf.nbytes
        self._check(self.lib.rgcn_copy_to_device(self.ctx, buf.ptr, _ptr(arr), arr.nbytes))

    def copy_to_device_async(self, buf, arr, on_prefetch_stream=False):
        """As copy_to_device without waiting for the transfer (rgcn_copy_to_device_async): staged through pinned
        memory, ordered on the main stream or on the prefetch stream."""
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= buf.nbytes
        self._check(self.lib.rgcn_copy_to_device_async(self.ctx, buf.ptr, _ptr(arr), arr.nbytes,
                                                       1 if on_prefetch_stream else 0))

    def to_device(self, arr):
        arr = np.ascontiguousarray(arr)
        return DeviceBuffer(self, arr.nbytes).upload(arr)

    def timer_start(self):
        self._check(self.lib.rgcn_timer_start(self.ctx))

    def timer_stop(self):
        ms = C.c_float()
        self._check(self.lib.rgcn_timer_stop(self.ctx, C.byref(ms)))
        return float(ms.value)

    def set_overlap(self, on=True):
        self._check(self.lib.rgcn_set_overlap(self.ctx, 1 if on else 0))

    def set_fusion(self, mode):
        """form of the block layer: 0 two kernels + message buffer, 1 (default) destination-major banded single pass
        (block_rows.hip)"""
        self._check(self.lib.rgcn_set_fusion(self.ctx, int(mode)))

    def set_gemm_mode(self, mode):
        """0 = fp32 MFMA, 9 / 6 = exact bf16 operand split with 9 / 6 partial products (include/rgcn.h)."""
        self._check(self.lib.rgcn_set_gemm_mode(self.ctx, int(mode)))

    def profile_enable(self, on=True):
        self._check(self.lib.rgcn_profile_enable(self.ctx, 1 if on else 0))

    def profile_reset(self):
        self._check(self.lib.rgcn_profile_reset(self.ctx))

    def profile(self):
        """[{name, calls, total_ms, alg_bytes (design), alg_flops, compulsory_bytes}] aggregated per kernel name."""
        out = []
        n = self.lib.rgcn_profile_count(self.ctx)
        for i in range(n):
            name = C.create_string_buffer(64)
            calls = C.c_int64()
            ms, by, fl = C.c_double(), C.c_double(), C.c_double()
            self._check(self.lib.rgcn_profile_get(self.ctx, i, name, 64, C.byref(calls), C.byref(ms),
                                                  C.byref(by), C.byref(fl)))
            cb = C.c_double()
            self._check(self.lib.rgcn_profile_get_compulsory(self.ctx, i, C.byref(cb)))
            out.append({"name": name.value.decode(), "calls": calls.value, "total_ms": ms.value,
                        "alg_bytes": by.value, "alg_flops": fl.value, "compulsory_bytes": cb.value})
        return out

    def debug_gemm_presplit(self, a, b, trans_b=False, iters=0):
        """A . op(B) with B pre-split into MFMA fragments (devtools build); returns C, or (C, ms per product) if iters"""
        a = np.ascontiguousarray(a, dtype=np.float32)
        b = np.ascontiguousarray(b, dtype=np.float32)
        M, K = a.shape
        N = b.shape[0] if trans_b else b.shape[1]
        out = np.empty((M, N), dtype=np.float32)
        ms = C.c_float()
        self._check(self.lib.rgcn_debug_gemm_presplit(self.ctx, int(trans_b), M, N, K, int(iters), _ptr(a), _ptr(b),
                                                      _ptr(out), C.byref(ms)))
        return (out, float(ms.value)) if iters else out

    def debug_gemm_prologue(self, a, bias, b, a_out, wide=True, prologue=True, row_limit=-1):
        """relu(a + bias) . b through the A-operand prologue of a pre-split-weight kernel (devtools build; prologue=False:
        a . b on the same kernel).  a [M,lda] holds the operand in its first K = len(bias) columns; a_out [M,lda] is the
        write-back target's content before the launch.  Returns (C, a_out after the launch)."""
        a = np.ascontiguousarray(a, dtype=np.float32)
        b = np.ascontiguousarray(b, dtype=np.float32)
        bias = np.ascontiguousarray(bias, dtype=np.float32)
        out_a = np.array(a_out, dtype=np.float32, order="C", copy=True)
        M, lda = a.shape
        K, N = b.shape
        assert bias.shape == (K,) and out_a.shape == (M, lda)
        out = np.empty((M, N), dtype=np.float32)
        self._check(self.lib.rgcn_debug_gemm_prologue(self.ctx, int(bool(wide)), int(bool(prologue)), M, N, K, lda,
                                                      int(row_limit), _ptr(a), _ptr(bias), _ptr(b), _ptr(out_a), _ptr(out)))
        return out, out_a

    def debug_gemm_call(self, a, b, c, M, N, K, a_kc=True, b_kc=False, lda=None, ldb=None, ldc=None, split_k=1, groups=1,
                        strideA=0, strideB=0, strideC=0, limit=None, limit_stride=1, limit_on_k=False, presplit_b=False,
                        wide=0, w8_knob=1, a_offset=0, b_offset=0, c_offset=0):
        """One launch of the dense contractions as csrc/gemm_plan.h describes a call (devtools build; include/
        rgcn_devtools.h rgcn_debug_gemm_call).  a, b, c: flat float32 buffers holding the whole strided extent of the
        operands; c is what the device copy of C holds before the launch.  Returns (C after the launch, flat, and the plan
        the call obeyed as a dict).  Nothing is adjusted on the way: what does not fit or is refused raises RgcnError."""
        a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
        b = np.ascontiguousarray(b, dtype=np.float32).reshape(-1)
        out = np.array(c, dtype=np.float32, order="C", copy=True).reshape(-1)
        d = DebugGemmDesc()
        d.a_kc, d.b_kc, d.M, d.N, d.K = int(bool(a_kc)), int(bool(b_kc)), int(M), int(N), int(K)
        d.lda = int(lda if lda is not None else (K if a_kc else M))
        d.ldb = int(ldb if ldb is not None else (K if b_kc else N))
        d.ldc = int(ldc if ldc is not None else N)
        d.split_k, d.groups = int(split_k), int(groups)
        d.strideA, d.strideB, d.strideC = int(strideA), int(strideB), int(strideC)
        lim = None
        if limit is not None:
            lim = np.ascontiguousarray(limit, dtype=np.int32).reshape(-1)
            assert lim.size == (d.groups - 1) * int(limit_stride) + 1, (lim.size, d.groups, limit_stride)
            d.limit = lim.ctypes.data
        d.limit_stride, d.limit_on_k = int(limit_stride), int(bool(limit_on_k))
        d.presplit_b, d.wide, d.w8_knob = int(bool(presplit_b)), int(wide), int(w8_knob)
        d.a_offset, d.b_offset, d.c_offset = int(a_offset), int(b_offset), int(c_offset)
        d.a_floats, d.b_floats, d.c_floats = a.size, b.size, out.size
        plan = DebugGemmPlan()
        try:
            self._check(self.lib.rgcn_debug_gemm_call(self.ctx, C.byref(d), _ptr(a), _ptr(b), _ptr(out), C.byref(plan)))
        except RgcnError as e:
            e.plan = plan.as_dict()
            raise
        return out, plan.as_dict()

    def debug_xcd_map(self, n_blocks):
        """XCD of every workgroup of a plain 1-D launch (devtools build)"""
        out = np.zeros(int(n_blocks), dtype=np.int32)
        self._check(self.lib.rgcn_debug_xcd_map(self.ctx, int(n_blocks), _ptr(out)))
        return out

    def device_memory(self):
        """(blocks, bytes) of the device allocations the context owns right now, over all its owners (devtools build)"""
        blocks, nbytes = C.c_int64(0), C.c_int64(0)
        self._check(self.lib.rgcn_debug_device_memory(self.ctx, C.byref(blocks), C.byref(nbytes)))
        return int(blocks.value), int(nbytes.value)

    def debug_gemm_time(self, a, b, trans_a=False, trans_b=False, split_k=0, iters=20):
        a = np.ascontiguousarray(a, dtype=np.float32)
        b = np.ascontiguousarray(b, dtype=np.float32)
        K, M = (a.shape if trans_a else a.shape[::-1])
        N = b.shape[0] if trans_b else b.shape[1]
        ms = C.c_float()
        self._check(self.lib.rgcn_debug_gemm_time(self.ctx, int(trans_a), int(trans_b), M, N, K, int(split_k),
                                                  int(iters), _ptr(a), _ptr(b), C.byref(ms)))
        return float(ms.value)

    def debug_gemm(self, a, b, trans_a=False, trans_b=False, split_k=0):
        a = np.ascontiguousarray(a, dtype=np.float32)
        b = np.ascontiguousarray(b, dtype=np.float32)
        K, M = (a.shape if trans_a else a.shape[::-1])
        N = b.shape[0] if trans_b else b.shape[1]
        assert (b.shape[1] if trans_b else b.shape[0]) == K
        out = np.empty((M, N), dtype=np.float32)
        self._check(self.lib.rgcn_debug_gemm(self.ctx, int(trans_a), int(trans_b), M, N, K, int(split_k),
                                             _ptr(a), _ptr(b), _ptr(out)))
        return out
