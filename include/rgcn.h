/*
 * rgcn.h -- C ABI of librgcn.so: the MI355X-native R-GCN encoder hot path
 * (forward + backward of MichSchli/RelationPrediction's `gcn_basis` encoder
 * chain: AffineTransform -> L x {ConcatGcn | BasisGcn}).
 *
 * This is the drop-in boundary.  In the reference the
 * Python plugin chain (code/model.py, code/encoders, code/common/model_builder.py)
 * builds a TF-1.4 graph and crosses into native code at `session.run`
 * (code/optimization/optimize.py:81-88 for training, code/model.py:56,69,81 for
 * scoring).  Here the same plugin chain (package `relationprediction_amd`)
 * crosses into this library through ctypes.  Each entry point names the
 * reference interface it replaces (paths relative to the reference checkout).
 *
 * Conventions
 *   - plain C: `extern "C"`, no C++/torch types, no exceptions cross the boundary;
 *   - every call returns an rgcn_status (0 = ok); rgcn_last_error() has the text;
 *   - host pointers are BORROWED for the duration of the call only;
 *   - device memory is owned by the context; `*_device` variants take device
 *     pointers (HIP, same device) that the caller owns and keeps alive until
 *     the next rgcn_sync();
 *   - a process may hold several contexts, on one GPU or on several: a context owns its streams, its device memory and
 *     its error text, and the only state contexts share is the text of a failed rgcn_create and a pool of idle HIP
 *     streams that destroyed contexts leave for later ones (both behind a mutex).  Contexts do not order themselves
 *     against each other: a device pointer one context hands to another (rgcn_rank_energies_device into
 *     rgcn_rank_mixed_device or rgcn_topk_mixed_device) is valid once the call that filled it has synchronised or rgcn_sync() has returned on
 *     the owner.  A context itself is not thread-safe; its calls are stream-ordered on the context's own HIP stream
 *     and asynchronous unless they return host data;
 *   - all floating point is float32, all indices int32 (reference:
 *     code/extras/graph_representations.py:174, code/common/shared_functions.py:17).
 */
#ifndef RGCN_H_
#define RGCN_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: these declarations are its whole dynamic symbol table */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define RGCN_ABI_VERSION 1

typedef struct rgcn_ctx rgcn_ctx;
typedef int32_t rgcn_status;

enum {
  RGCN_OK = 0,
  RGCN_ERR_INVALID = 1,     /* bad argument / out-of-range index / wrong size */
  RGCN_ERR_HIP = 2,         /* a HIP runtime call failed */
  RGCN_ERR_RCCL = 3,        /* an RCCL call failed / librccl not loadable */
  RGCN_ERR_STATE = 4,       /* call order violated (e.g. backward before forward) */
  RGCN_ERR_UNSUPPORTED = 5, /* configuration outside what the kernels implement */
  RGCN_ERR_NOMEM = 6        /* the device is out of memory: any allocation the library makes, at create or later */
};

/* Encoder.Concatenation=Yes -> ConcatGcn (block-diagonal), else BasisGcn:
 * code/common/model_builder.py:291-294. */
enum { RGCN_KIND_BLOCK = 0, RGCN_KIND_BASIS = 1, RGCN_KIND_BASIS_TDIAG = 2, RGCN_KIND_BASIS_PDIAG = 3, RGCN_KIND_EMBEDDING = 4 };
/* RGCN_KIND_EMBEDDING = Encoder.Name=embedding (model_builder.py:27-41; settings/distmult.exp): the DistMult baseline,
 * RelationEmbedding(AffineTransform(onehot_input=True, use_bias=False, use_nonlinearity=False)).  No graph and no layer:
 *   - num_layers must be 0 and num_bases 1 (RGCN_ERR_INVALID otherwise); max_edges may be 0; keep_prob and norm_mode are
 *     checked as for every kind and not used; world > 1, RGCN_INPUT_ONEHOT and RGCN_SKIP_HIGHWAY: RGCN_ERR_UNSUPPORTED;
 *   - parameters: W_emb [V,d], b_emb [d], W_relation [V,d].  b_emb is created, stored and checkpointed but never read
 *     (use_bias=False; tf.gradients reports it unconnected): its gradient is all zeros and Adam leaves it alone;
 *   - the codes ARE W_emb, in train and test mode alike (no bias, no relu, no dropout).  rgcn_forward needs no graph and
 *     launches nothing; rgcn_codes_device returns the parameter's own storage, so after an optimizer step the codes are
 *     the updated table -- what a new forward pass would return; rgcn_get_activation(0) returns the codes, any other
 *     layer is RGCN_ERR_INVALID;
 *   - rgcn_backward / rgcn_backward_device set the gradient of W_emb to dcodes; rgcn_dcodes_device IS that gradient's
 *     storage, so the device decoder writes it in place;
 *   - rgcn_train_step_device(ctx, NULL, 0, x, y, N, ...) = decoder loss + gradients, then clip + Adam if configured; a
 *     non-NULL triple pointer or num_edges != 0 is RGCN_ERR_INVALID;
 *   - RGCN_ERR_UNSUPPORTED, the message naming the kind: rgcn_set_graph*, rgcn_prefetch_graph*, rgcn_step_device,
 *     rgcn_train_step_minibatch_device, rgcn_neighborhood_reserve, the phase API (rgcn_forward_begin ... rgcn_backward_end),
 *     rgcn_set_relation_owner, rgcn_capture_begin; rgcn_read_buffer knows RGCN_BUF_RANK_ENERGIES,
 *     RGCN_BUF_RANK_MIXED_SCORES, RGCN_BUF_RELATION_ENERGIES, RGCN_BUF_NEGATIVE_UNRESOLVED,
 *     RGCN_BUF_NEGATIVE_RELATION_UNRESOLVED and RGCN_BUF_NEGATIVE_TYPED_OPEN only (RGCN_ERR_STATE);
 *   - unchanged: rgcn_decoder_*, rgcn_negative_sample_device, rgcn_known_positives_reserve, rgcn_type_sets_reserve,
 *     rgcn_negative_sample_typed_device, rgcn_rank_typed_device, rgcn_topk_typed_device,
 *     rgcn_negative_sample_exclusive_device, rgcn_negative_sample_relation_device, rgcn_reciprocal_rows_device,
 *     rgcn_set_reciprocal_relations, rgcn_optimizer_*, rgcn_rank_device, rgcn_rank_mixed_device,
 *     rgcn_topk_device, rgcn_score_queries_device, rgcn_topk_mixed_device, rgcn_rank_relation_device,
 *     rgcn_topk_relation_device, rgcn_score_relation_queries_device, parameters, device memory, timer and profile. */
/* RGCN_KIND_BASIS_TDIAG = Encoder.DiagonalCoefficients=Yes -> BasisGcnTimesDiag
 * (code/encoders/message_gcns/gcn_basis_times_diag.py; model_builder.py:287-288, ahead of Concatenation): the
 * coefficient of a message is a VECTOR per (relation, basis) over the output channels,
 *     W_r = sum_b W_b . diag(sigmoid(C[r,b,:])),     pre = dropout(H . W_self) + sum of messages + b,
 * and, unlike the other two kinds, the layer's bias b IS added (:86): it has a gradient and the optimizer moves it.
 * num_bases = B.  Transform-first dataflow (csrc/basis_tdiag.hip): P = H . [W_f | W_b], then a destination-major
 * gather over the incidence CSR.  One GPU with embedding input and RGCN_SKIP_NONE only; rgcn_create / rgcn_create_ex
 * return RGCN_ERR_UNSUPPORTED for
 *   - world > 1 (P, dP and the coefficient table have no exchange points),
 *   - RGCN_INPUT_ONEHOT (the reference's one-hot branch of this layer exists, gcn_basis_times_diag.py:21,70,76; not built),
 *   - RGCN_SKIP_HIGHWAY,
 *   - num_bases > 64,
 *   - 2 * EntityCount * num_bases * dim >= 2^31 (the products are indexed with 32-bit ints per direction pair),
 * and rgcn_capture_begin returns RGCN_ERR_UNSUPPORTED on such a context (a captured step of this kind has never been
 * replayed against a reference).  Every RGCN_NORM_* mode and every rgcn_set_gemm_mode work; rgcn_set_fusion is ignored. */
/* RGCN_KIND_BASIS_PDIAG = Encoder.AddDiagonal=Yes -> BasisGcnWithDiag (code/encoders/message_gcns/gcn_basis_plus_diag.py;
 * model_builder.py:285-286, the flag the reference checks first): the basis layer plus a DistMult-like term per message,
 * H[src] * D[rho], with a trained vector D[rho] per directed relation; the layer's bias b IS added and trained.
 * AS EXECUTED by the reference (compute_messages unpacks the two basis products the other way round from how
 * compute_basis_functions returns them, :51 against :75-79) the basis term of a message is formed from the DESTINATION's
 * own features under the OTHER direction's basis tensor:
 *     a_dir[v,b] = sum_{m -> v, dir(m) = dir} n_m C_dir[r_m,b]
 *     pre[v]     = dropout(H . W_self)[v] + sum_dir sum_b a_dir[v,b] (H[v] . W_other(dir)[:,b,:])
 *                  + sum_{m -> v} n_m D[rho_m,:] * H[src_m,:] + b
 * num_bases = B (csrc/basis_pdiag.hip).  One GPU with embedding input and RGCN_SKIP_NONE only; rgcn_create /
 * rgcn_create_ex return RGCN_ERR_UNSUPPORTED for
 *   - world > 1 (the mixing table, the diagonal aggregate and dD have no exchange points),
 *   - RGCN_INPUT_ONEHOT (the one-hot branch of this layer is not built),
 *   - RGCN_SKIP_HIGHWAY,
 *   - num_bases > 64,
 *   - 2 * EntityCount * num_bases * dim >= 2^31 (the compacted unit rows are indexed with 32-bit ints per direction pair),
 * and rgcn_capture_begin returns RGCN_ERR_UNSUPPORTED on such a context.  Every RGCN_NORM_* mode and every
 * rgcn_set_gemm_mode work; rgcn_set_fusion is ignored. */

/* Neighbour normalisation of the incidence matrices, normalization=('global', ...)
 * (code/extras/graph_representations.py:82-93,122-133).  INTENDED = 1/deg(row of this edge);
 * TF_AS_EXECUTED = SURVEY.md section 9 H1 (tf.sparse_softmax on non-canonical indices returns the
 * values in sorted-row order); NONE = the 'none' branch (:70-81).
 * LOCAL = normalization=('local', ...) (code/extras/graph_representations.py:94-107,134-147: softmax of ones over the
 * entries that share (relation, row), summed over the relation axis), the paper's c_{i,r} = |N_i^r|: of a fed triple
 * (s, r, o) the forward message (directed relation r, destination o) gets 1 / |{fed (s', r, o)}| and the backward
 * message (directed relation R + r, destination s) gets 1 / |{fed (s, r, o')}|.  Counts run over the triples actually
 * fed (after edge dropout: the kept ones); duplicates count once each; a self-edge counts in both directions.  As
 * written only: there is no as-executed reading of 'local' (the H1 hazard would apply to the reference's 3-D softmax
 * as it does to the 2-D one).  Under relation sharding the counts need no exchange: a relation's owner holds every
 * message of it.  Any other value of the field: RGCN_ERR_INVALID. */
enum { RGCN_NORM_INTENDED = 0, RGCN_NORM_TF_AS_EXECUTED = 1, RGCN_NORM_NONE = 2, RGCN_NORM_LOCAL = 3 };

/* What lies under the first graph convolution (code/common/model_builder.py:140-165,277-283).
 * EMBEDDING = UseInputTransform=Yes: AffineTransform H_0 = relu(W_emb + b_emb), every layer dense.
 * ONEHOT    = UseInputTransform=No (RandomInput=No, PartiallyRandomInput=No): no input layer; the first BasisGcn has
 *             onehot_input=True and looks its messages up in per-entity tables (gcn_basis.py:16-24,60-71,
 *             message_gcn.py:28-79, shared_functions.py:5-9).  Basis kind on one GPU only: with RGCN_KIND_BLOCK (the
 *             reference's one-hot branch of ConcatGcn cannot execute, gcn_basis_concat.py:18-19,42-46), with world > 1
 *             or with EntityCount * NumberOfBasisFunctions * dim >= 2^31 rgcn_create returns RGCN_ERR_UNSUPPORTED.
 *             rgcn_capture_begin returns RGCN_ERR_UNSUPPORTED on such a context (a captured one-hot step has not
 *             been tested).  Any other value of the field: RGCN_ERR_INVALID. */
enum { RGCN_INPUT_EMBEDDING = 0, RGCN_INPUT_ONEHOT = 1 };

/* Skip connections around the graph-convolution layers (SkipConnections, code/common/model_builder.py:273-309).
 * NONE    = every layer's result is the next layer's input, what rgcn_create builds.
 * HIGHWAY = every layer l = 1..L is wrapped in a HighwayLayer (code/extras/highway_layer.py):
 *               T_l = sigmoid(H_{l-1} . W_highway_l + b_highway_l)
 *               H_l = T_l * N_l + (1 - T_l) * H_{l-1}        N_l = what layer l returns under RGCN_SKIP_NONE
 *           (N_l with the layer's relu for l < L, without for l = L; the self-loop dropout stays inside N_l, the highway
 *           layer applies none).  rgcn_get_codes / rgcn_get_activation(l) / rgcn_codes_device return the post-highway H_l.
 *           One GPU with embedding input only: with world > 1 or with RGCN_INPUT_ONEHOT rgcn_create_ex returns
 *           RGCN_ERR_UNSUPPORTED (the reference's one-hot first layer gets no highway layer while layers >= 2 do: not
 *           built), and rgcn_capture_begin returns RGCN_ERR_UNSUPPORTED on such a context.  Both block forms
 *           (rgcn_set_fusion), the basis kind, every RGCN_NORM_* and every rgcn_set_gemm_mode work.
 * Any other value: RGCN_ERR_INVALID. */
enum { RGCN_SKIP_NONE = 0, RGCN_SKIP_HIGHWAY = 1 };

/* Buffers readable through rgcn_read_buffer (tests / the sharding exchange). */
enum {
  RGCN_BUF_EXCHANGE = 0,   /* [V,d] buffer a multi-GPU run all-reduces (partial pre-activation / partial dH) */
  RGCN_BUF_SELF = 1,       /* [V,d] self-loop product H.W_self of the last layer run */
  RGCN_BUF_DSELF_EXCHANGE = 2, /* [d,d] partial dW_self a multi-GPU run all-reduces */
  RGCN_BUF_INDEG = 3,      /* int32 [V] in-degree inside the fed graph  */
  RGCN_BUF_OUTDEG = 4,     /* int32 [V] out-degree inside the fed graph */
  RGCN_BUF_ROWPTR = 5,     /* int32 [V+1] incidence CSR offsets (owned relations only) */
  RGCN_BUF_NORM_EXCHANGE = 6,   /* float [1] squared norm of this rank's relation-sharded gradients (optimizer phases) */
  RGCN_BUF_DBASIS_EXCHANGE = 7, /* basis kind: [2,B,d,d] partial gradient of the replicated basis tensors of the
                                   backward layer in flight, which a multi-GPU run all-reduces */
  /* the two orderings graph preparation produces (library's own stable sort, csr_sort.hip), for inspection:
   * incidence i < E = edge i seen from its object, i >= E = edge i-E seen from its subject; message m likewise with
   * directed relation r (m < E) or R + r */
  RGCN_BUF_PERM_VERTEX = 8,     /* int32 [2E] incidence ids in incidence-CSR order (by vertex, ties by id) */
  RGCN_BUF_PERM_RELATION = 9,   /* int32 [2E] message ids in message-list order (by directed relation, ties by id) */
  RGCN_BUF_RANK_ENERGIES = 10,  /* float [reserved queries, V] energies of the last chunk rgcn_rank_device,
                                   rgcn_topk_device or one of their mixed and score-only forms scored (the float half of the ranking; the counts and the selection
                                   are integer work on exactly these values) */
  RGCN_BUF_MSG_NORM = 11,       /* float [2E] normalisation of every message, in message-list order: entry j belongs to
                                   message RGCN_BUF_PERM_RELATION[j] (every RGCN_NORM_* mode).  Sharded context: only
                                   this rank's messages, which come first in the list; the rest is undefined */
  /* RGCN_SKIP_HIGHWAY contexts, of the layer the last rgcn_forward_layer_finish (or rgcn_forward: layer L) ran: */
  RGCN_BUF_HIGHWAY_INNER = 12,  /* float [V,d] N_l, the wrapped layer's result */
  RGCN_BUF_HIGHWAY_GATE = 13,   /* float [V,d] T_l, the transform gate */
  /* RGCN_KIND_BASIS_TDIAG contexts, of the layer the last rgcn_forward_layer_finish (or rgcn_forward: layer L) ran;
   * RGCN_ERR_STATE on every other context: */
  RGCN_BUF_TDIAG_PRODUCTS = 14, /* float [2][V][B*d]: P_f = H_{l-1} . W_f.reshape(d, B*d), then P_b likewise */
  /* RGCN_KIND_BASIS_PDIAG contexts, of the layer the last rgcn_forward_layer_finish (or rgcn_forward: layer L) ran;
   * RGCN_ERR_STATE before any layer has run and on every other context: */
  RGCN_BUF_PDIAG_MIX = 15,      /* float [2][V][B]: a_dir[v,b] = sum over the row's messages of direction dir of n C_dir[r,b] */
  RGCN_BUF_PDIAG_AGG = 16,      /* float [V,d]: the diagonal aggregate sum over the row's messages of n D[rho] * H_{l-1}[src] */
  RGCN_BUF_RANK_MIXED_SCORES = 17, /* float [reserved queries, V]: the mixed scores of the last rgcn_topk_mixed_device (what
                                   it selected from, bit for bit).  RGCN_ERR_STATE before the first such call, and again
                                   after a growing rgcn_rank_reserve until the next one */
  RGCN_BUF_RELATION_ENERGIES = 18, /* float [reserved queries, RelationCount]: energies of the last chunk
                                   rgcn_rank_relation_device, rgcn_topk_relation_device or
                                   rgcn_score_relation_queries_device scored (what the counts and the selection are integer
                                   work on).  RGCN_ERR_STATE before the first such call, and again after a growing
                                   rgcn_rank_reserve until the next one */
  RGCN_BUF_OUT_DH = 19,         /* float [V,d], contexts with an output transform (rgcn_config_ext::code_dim > 0): dL/dH_L of
                                   the last backward pass = dcodes . W_out^T, what the layer stack received as its dcodes.
                                   RGCN_ERR_STATE on every other context and before the first backward pass */
  RGCN_BUF_NEGATIVE_UNRESOLVED = 20,/* int64 [1]: negative rows, since the last rgcn_known_positives_reserve, for which EVERY
                                   entity was a known positive and which therefore kept their first draw (exclusive
                                   sampler, stand-alone and fused; replayed hipGraphs count too).  Every kind,
                                   RGCN_KIND_EMBEDDING included; RGCN_ERR_STATE without an index */
  RGCN_BUF_NEGATIVE_RELATION_UNRESOLVED = 21,/* int64 [1]: relation rows (rgcn_negative_sample_relation_device with
                                   exclusive != 0, stand-alone and fused), since the last rgcn_known_positives_reserve, for
                                   which EVERY other relation was a known positive for the pair and which therefore kept
                                   their first draw.  Every kind; RGCN_ERR_STATE without an index */
  /* the relation-softmax term (rgcn_relation_softmax_device and the fused steps under rgcn_set_relation_softmax), of
   * the LAST chunk it walked: every kind, RGCN_KIND_EMBEDDING included; RGCN_ERR_STATE before
   * rgcn_relation_softmax_reserve.  chunk and padded R: rgcn_relation_softmax_plan */
  RGCN_BUF_RELATION_SOFTMAX_ENERGIES = 22, /* float [chunk, padded R]: E[n, r'] = q_n . W_relation[r']; pad columns zero */
  RGCN_BUF_RELATION_SOFTMAX_G = 23,        /* float [chunk, padded R]: G[n, r'], the term's gradient w.r.t. E; pad columns zero */
  RGCN_BUF_RELATION_SOFTMAX_DQ = 24,       /* float [chunk, code width]: dq_n = sum over r' of G[n, r'] W_relation[r'] */
  RGCN_BUF_ADVERSARIAL_WEIGHTS = 25,       /* float [N]: the row weights of the last fused step that ran under
                                   rgcn_set_adversarial_negatives, N that step's decoder rows.  Every kind,
                                   RGCN_KIND_EMBEDDING included; RGCN_ERR_STATE before such a step */
  /* the entity-softmax term (rgcn_entity_softmax_device and the fused steps under rgcn_set_entity_softmax), of the LAST
   * chunk of rows it walked: every kind, RGCN_KIND_EMBEDDING included; RGCN_ERR_STATE before
   * rgcn_entity_softmax_reserve.  chunk and padded V: rgcn_entity_softmax_plan.  (The energies are not readable: G
   * overwrites them in place.) */
  RGCN_BUF_ENTITY_SOFTMAX_G = 26,          /* float [chunk, padded V]: G[m, e], the term's gradient w.r.t. E; pad columns zero */
  RGCN_BUF_ENTITY_SOFTMAX_DQ = 27,         /* float [chunk, code width]: dq_m = sum over e of G[m, e] c[e] */
  RGCN_BUF_NEGATIVE_TYPED_OPEN = 28        /* int64 [1]: negative rows, since the last rgcn_type_sets_reserve, that the
                                   type-constrained sampler (stand-alone and fused) drew over ALL entities: the list of
                                   the row's (side, relation) is open, the row's own entity is its only member, an id of
                                   the row is out of range, or (exclusive) every other member was a known positive.  Every
                                   kind, RGCN_KIND_EMBEDDING included; RGCN_ERR_STATE without type sets */
};

/*
 * Replaces the settings the reference components parse in their constructors:
 * Model.__init__ (code/model.py:17-25: EntityCount, RelationCount), ConcatGcn/BasisGcn.parse_settings
 * (gcn_basis_concat.py:10-15, gcn_basis.py:10-13: DropoutKeepProbability, NumberOfBasisFunctions),
 * build_encoder (model_builder.py:121-184: InternalEncoderDimension, NumberOfLayers).
 */
typedef struct rgcn_config {
  int32_t abi_version;    /* must be RGCN_ABI_VERSION */
  int32_t device;         /* HIP device ordinal */
  int32_t num_entities;   /* V = EntityCount */
  int32_t num_relations;  /* R = RelationCount */
  int32_t dim;            /* d = InternalEncoderDimension (the code width too, unless rgcn_config_ext::code_dim says otherwise) */
  int32_t num_layers;     /* L = NumberOfLayers (RGCN_KIND_EMBEDDING: 0) */
  int32_t kind;           /* RGCN_KIND_* */
  int32_t num_bases;      /* NumberOfBasisFunctions: block count nb (BLOCK, d % nb == 0) or B (BASIS, BASIS_TDIAG, BASIS_PDIAG) */
  float   keep_prob;      /* DropoutKeepProbability (self-loop dropout, train mode only) */
  int32_t norm_mode;      /* RGCN_NORM_* */
  int64_t max_edges;      /* capacity: largest E ever passed to rgcn_set_graph* */
  int32_t rank;           /* relation-sharding rank in [0, world) */
  int32_t world;          /* number of relation shards (1 = single GPU) */
  int32_t input_mode;     /* RGCN_INPUT_* (0 = embedding input, what every earlier caller passed here) */
} rgcn_config;

/* rgcn_config is full (64 bytes, pinned): what came later is passed beside it.  struct_size must be
 * sizeof(rgcn_config_ext), or 8 -- the layout before code_dim, read as code_dim = 0 -- else RGCN_ERR_INVALID.
 *
 * code_dim: the encoder's output transform (UseOutputTransform=Yes, code/common/model_builder.py:131-135,170-177,
 * code/encoders/affine_transform.py:63-83): a dense AffineTransform on top of the last graph convolution,
 *     codes = H_L . W_out + b_out        W_out [d, c], b_out [c], no relu, no dropout, train and test mode alike.
 *   0   no output layer: the codes are H_L, c = d, everything as rgcn_create builds it;
 *   c > 0   the layer exists (also when c == d: the reference applies it whenever the flag says Yes).  W_out and b_out sit
 *       between the last layer's parameters (its highway pair included) and W_relation, which becomes [EntityCount, c]
 *       (Model.get_weights() order).  Everything on the code side is c wide: rgcn_get_codes, rgcn_codes_device,
 *       rgcn_dcodes_device, the dcodes of rgcn_backward / _device / rgcn_step_device, the decoder, and the query rows of
 *       every rgcn_rank_*, rgcn_topk_* and rgcn_score_* call.  rgcn_get_activation(L) stays H_L [V,d].
 *       The layer sees H_L only: every kind but RGCN_KIND_EMBEDDING (the reference's embedding branch has no such layer),
 *       both rgcn_set_fusion forms, one-hot input, highway, every RGCN_NORM_* and every rgcn_set_gemm_mode work.  With
 *       world > 1 (W_out's gradient has no exchange point), with RGCN_KIND_EMBEDDING or with EntityCount x c >= 2^31
 *       rgcn_create_ex returns RGCN_ERR_UNSUPPORTED, and so does rgcn_capture_begin on such a context.
 *   c < 0   RGCN_ERR_INVALID. */
typedef struct rgcn_config_ext {
  int32_t struct_size;
  int32_t skip_mode;      /* RGCN_SKIP_* */
  int32_t code_dim;       /* c = CodeDimension of the output transform; 0: none (the codes are H_L) */
} rgcn_config_ext;

/* ---- lifecycle ------------------------------------------------------------------------------ */

int32_t rgcn_abi_version(void);

/* Replaces tf.Session() + Model.initialize_train() variable allocation
 * (code/train.py:258,278; code/model.py:93-94).  Weights start as zeros: the host plugin chain
 * draws the reference's numpy initialisers (shared_functions.py:16-29) and pushes them. */
rgcn_status rgcn_create(const rgcn_config* cfg, rgcn_ctx** out);
/* The same with the extended settings; ext == NULL: their defaults (RGCN_SKIP_NONE) -- rgcn_create(cfg, out) is
 * rgcn_create_ex(cfg, NULL, out).  A wrong struct_size, an unknown skip_mode or a negative code_dim: RGCN_ERR_INVALID;
 * RGCN_SKIP_HIGHWAY with world > 1 or with RGCN_INPUT_ONEHOT: RGCN_ERR_UNSUPPORTED; code_dim > 0: see rgcn_config_ext. */
rgcn_status rgcn_create_ex(const rgcn_config* cfg, const rgcn_config_ext* ext, rgcn_ctx** out);
rgcn_status rgcn_destroy(rgcn_ctx* ctx);

/* Text of the last error on this context (ctx == NULL: last error of a failed rgcn_create). */
const char* rgcn_last_error(const rgcn_ctx* ctx);

/* Wait for everything queued on the context's stream; also surfaces asynchronous device-side
 * validation failures (out-of-range vertex / relation ids in a device-resident graph). */
rgcn_status rgcn_sync(rgcn_ctx* ctx);

/* ---- parameters (the encoder part of Model.get_weights(), code/model.py:96-97) ----------------
 * Index order = reference order, innermost component first:
 *   W_emb [V,d], b_emb [d]                                  (affine_transform.py:30-31)
 *   per layer l=1..L:  BLOCK: W_f [R,nb,sd,sd], W_b [R,nb,sd,sd], W_self [d,d], b [d]
 *                                                           (gcn_basis_concat.py:30-33)
 *                      BASIS: W_f [d,B,d], W_b [d,B,d], C_f [R,B], C_b [R,B], W_self [d,d], b [d]
 *                                                           (gcn_basis.py:33-37)
 *                      BASIS_TDIAG: W_f [d,B,d], W_b [d,B,d], C_f [R,B,d], C_b [R,B,d], W_self [d,d], b [d]
 *                                                           (gcn_basis_times_diag.py:38-42); b is a LIVE parameter here
 *                      BASIS_PDIAG: W_f [d,B,d], W_b [d,B,d], C_f [R,B], C_b [R,B], D_b [R,d], D_f [R,d], W_self [d,d], b [d]
 *                                                           (gcn_basis_plus_diag.py:42-47: the BACKWARD diagonal table comes
 *                                                           first); b is a LIVE parameter here
 * RGCN_INPUT_ONEHOT (basis kind; model_builder.py:140-165,277-283, gcn_basis.py:16-24): no W_emb / b_emb, and layer 1 is
 *                      W_f [V,B,d], W_b [V,B,d], C_f [R,B], C_b [R,B], W_self [V,d], b [d]; layers 2..L as above.
 *                      rgcn_param_count / _info / rgcn_set_param / rgcn_get_param / rgcn_get_grad all follow that list.
 * RGCN_SKIP_HIGHWAY:   behind every layer's b come W_highway<l> [d,d] and b_highway<l> [d] (highway_layer.py; the
 *                      order Model.get_weights() returns).  The same calls, the optimizer's clip norm and Adam follow.
 * Host layouts are the reference's (row-major, shapes above); the device layout is private.
 * `b` is created but never used by the reference's BLOCK and BASIS layers: it is stored, never read,
 * and its gradient is all zeros (BASIS_TDIAG and BASIS_PDIAG add it: gradient, clip norm and Adam follow).  The LAST parameter is the decoder's W_relation [EntityCount, d]
 * (relation_embedding.py:15-18; only rows < RelationCount are ever used): the encoder path
 * does not touch it, the device decoder below does. */
int32_t     rgcn_param_count(const rgcn_ctx* ctx);
rgcn_status rgcn_param_info(const rgcn_ctx* ctx, int32_t index, char* name, int32_t name_cap,
                            int64_t shape[4], int32_t* ndim);
/* replaces tf.Variable(initializer) / Saver.restore: shared_functions.py:16-22, model.py:38 */
rgcn_status rgcn_set_param(rgcn_ctx* ctx, int32_t index, const float* host, int64_t count);
/* replaces Saver.save / session.run(variable): model.py:30-37 */
rgcn_status rgcn_get_param(rgcn_ctx* ctx, int32_t index, float* host, int64_t count);
/* replaces the tensors tf.gradients(loss, weights) returns: optimization/abstract.py:117-118 */
rgcn_status rgcn_get_grad(rgcn_ctx* ctx, int32_t index, float* host, int64_t count);

/* ---- graph (the `graph_edges` placeholder, graph_representations.py:173-177) -------------------
 * triples = int32 [E,3] rows (subject, relation, object) exactly as fed to the placeholder
 * (MessageGraph.process, :21-27).  The call builds, on the device, everything the reference derives
 * inside session.run: degrees, the 'global' normalisation values (:82-93,122-133), the
 * relation-sorted message list and the incidence CSR.  Edge dropout (GraphSplitSize, train.py:235-238)
 * is applied by the caller before the call: degrees are counted over the edges actually fed.
 * 0 <= E <= max_edges.  The host variant validates ids and returns RGCN_ERR_INVALID on a bad one. */
rgcn_status rgcn_set_graph(rgcn_ctx* ctx, const int32_t* triples_host, int64_t num_edges);
rgcn_status rgcn_set_graph_device(rgcn_ctx* ctx, const int32_t* triples_dev, int64_t num_edges);

/* Edge dropout of the reference's minibatch construction, on the device (code/train.py:233-238):
 *     graph_split_ids = np.random.choice(graph_batch_ids, size=int(GraphSplitSize * n), replace=False)
 * the message-passing graph is a uniformly random subset of EXACTLY `keep` of the n batch edges; only those are fed
 * to `graph_edges`, so degrees and normalisation are counted over the kept edges, while the decoder keeps
 * every batch edge as a positive (H9: pass the whole batch to the decoder / rgcn_train_step_minibatch_device).
 * batch_dev = int32 [n,3]; the draw is a function of (seed, n, keep) alone (counter-based keys, the `keep` smallest
 * win); keep_mask_dev (nullable) = uint8 [n] with exactly `keep` ones: the caller's set instead of the draw (how a
 * test injects the reference's choice).  The kept edges are compacted in batch order (the reference's come in the
 * random order of np.random.choice: same set distribution, other row order) and prepared like rgcn_set_graph_device;
 * rgcn_get_graph_edges returns the rows of the graph currently set ([keep,3]; synchronises). */
rgcn_status rgcn_set_graph_dropout_device(rgcn_ctx* ctx, const int32_t* batch_dev, int64_t num_edges, int64_t keep,
                                          uint64_t seed, const uint8_t* keep_mask_dev);
rgcn_status rgcn_get_graph_edges(rgcn_ctx* ctx, int32_t* host, int64_t count);

/* ---- forward: get_all_codes(mode) (message_gcn.py:44-79, affine_transform.py:63-83) ------------
 * train != 0 applies self-loop dropout (message_gcn.py:60-64).  The Bernoulli(keep_prob) draw is
 *   - dropout_masks_host != NULL: the caller's uint8 [L,V,d] 0/1 masks (parity testing), else
 *   - a counter-based generator keyed by (dropout_seed, layer, element) -- nothing is stored;
 *     rgcn_get_dropout_mask() re-materialises what the last forward used.
 * The result H_L [V,d] is the subject AND object code matrix (relation_embedding.py:23-25); on a context with an output
 * transform (rgcn_config_ext::code_dim = c > 0) the code matrix is H_L . W_out + b_out [V,c] and H_L stays readable
 * through rgcn_get_activation(L). */
rgcn_status rgcn_forward(rgcn_ctx* ctx, int32_t train, uint64_t dropout_seed,
                         const uint8_t* dropout_masks_host);
rgcn_status rgcn_get_codes(rgcn_ctx* ctx, float* host, int64_t count);              /* the codes: H_L [V,d], or [V,c] */
/* RGCN_INPUT_ONEHOT: there is no H_0 (message_gcn.py:28-36 hands the layer the vertex ids); layer 0 is RGCN_ERR_INVALID */
rgcn_status rgcn_get_activation(rgcn_ctx* ctx, int32_t layer, float* host, int64_t count); /* H_0..H_L */
rgcn_status rgcn_get_dropout_mask(rgcn_ctx* ctx, int32_t layer /*1..L*/, uint8_t* host, int64_t count);
const float* rgcn_codes_device(rgcn_ctx* ctx);                                      /* device codes (RGCN_KIND_EMBEDDING: W_emb's
                                                                                       own storage -- after an optimizer step the
                                                                                       updated table) */

/* ---- backward: tf.gradients(loss, weights) restricted to the encoder (abstract.py:117-118) -----
 * dcodes = dL/dcodes: dL/dH_L [V,d], or [V,c] under an output transform (the decoder's gradient w.r.t. subject+object
 * codes, already summed).
 * Needs a preceding rgcn_forward on the same graph.  Gradients are then readable by rgcn_get_grad. */
rgcn_status rgcn_backward(rgcn_ctx* ctx, const float* dcodes_host, int64_t count);
rgcn_status rgcn_backward_device(rgcn_ctx* ctx, const float* dcodes_dev);

/* One whole 'step' of the BASELINE metric, fully asynchronous: graph prep + forward(train) +
 * backward from device-resident inputs.  Replaces one session.run of the encoder part of
 * TensorflowOptimizer.update_from_batch (optimize.py:81-88). */
rgcn_status rgcn_step_device(rgcn_ctx* ctx, const int32_t* triples_dev, int64_t num_edges,
                             int32_t train, uint64_t dropout_seed, const float* dcodes_dev);

/* ---- "next" rows: DistMult decoder, clip + Adam, whole train step on the device ----
 * X = int32 [N,3] (subject, relation, object) positives + sampled negatives, Y = float32 [N] labels, as
 * NegativeSampler.transform emits them (code/common/auxilliaries.py:13-33).  Replaces the decoder part of
 * the train graph: BilinearDiag.get_loss + local_get_regularization (code/decoders/bilinear_diag.py:27-34,
 * 63-69) and their tf.gradients.  Needs rgcn_decoder_reserve(max N) once and a completed rgcn_forward.
 * Leaves dL/dcodes in rgcn_dcodes_device() (feed it to rgcn_backward_device) and dL/dW_relation in the
 * gradient of the last parameter; rgcn_get_loss returns loss + regulariser (synchronises).
 * max_triples (and a tiled batch's n * (rate + 1)) may not exceed RGCN_MAX_DECODER_TRIPLES: the decoder's kernels
 * index with 32-bit ints, whose largest expressions are 3 N + 2 and 2 N + 255. */
#define RGCN_MAX_DECODER_TRIPLES ((int64_t)1 << 29)
rgcn_status rgcn_decoder_reserve(rgcn_ctx* ctx, int64_t max_triples);
rgcn_status rgcn_decoder_loss_backward_device(rgcn_ctx* ctx, const int32_t* x_dev, const float* y_dev,
                                              int64_t num_triples, float regularization_parameter);
const float* rgcn_dcodes_device(rgcn_ctx* ctx);
rgcn_status rgcn_get_loss(rgcn_ctx* ctx, double* loss);
/* ---- minibatch construction on the host ---------------------------------------------
 * sample_edge_neighborhood of the reference's train loop (code/train.py:133-139 adjacency, :161-198 sampler):
 * the same random process (vertex ~ free edge ends x touched, then a free incident edge uniformly; uniform
 * restart over vertices with free edges when nothing touched has any) in O(log V) per pick instead of the
 * reference's O(V).  Host memory in, host memory out, no context, no GPU.  triples = int32 [n,3] rows
 * (subject, relation, object) of the training graph; out_edge_ids = int32 [sample_size] distinct row ids.
 * sample_size > n is an error (the reference crashes there). */
typedef struct rgcn_sampler rgcn_sampler;
rgcn_status rgcn_sampler_create(const int32_t* triples, int64_t num_triples, int32_t num_entities,
                                rgcn_sampler** out);
void rgcn_sampler_destroy(rgcn_sampler* sampler);
rgcn_status rgcn_sampler_edge_neighborhood(rgcn_sampler* sampler, int64_t sample_size, uint64_t seed,
                                           int32_t* out_edge_ids);

/* The same sampler ON THE DEVICE (csrc/neighborhood.hip): sample_edge_neighborhood's process has the distribution of
 * first-passage percolation with an Exp(1) clock on every edge end (a touched vertex's free edge ends are equally
 * likely to be picked next = they race with memoryless clocks), its restart rule that of a uniform random vertex order
 * over the connected components -- so the batch is every edge of the components visited in full plus the edges of
 * least pick time of the component the budget runs out in: parallel Bellman-Ford sweeps over the adjacency, a radix
 * select and a stable compaction on the device, the component order from V hashes on the host inside the call.  Same
 * distribution as code/train.py:161-198 (held to it by tests/test_gpu_sampler.py), another random stream, a function of
 * `seed` alone, no batch built on the host and no upload.  rgcn_neighborhood_reserve hands the training graph over once
 * (code/train.py:133-139 builds the adjacency lists once): ids are validated, components and adjacency are built on
 * the host and copied; rgcn_sample_neighborhood_device writes the drawn rows int32 [sample_size,3] (in edge order) to
 * batch_out_dev, asynchronously on the main stream or -- on_prefetch_stream != 0 -- on the stream
 * rgcn_prefetch_graph*_device works on, so that "draw the next batch, drop edges, prepare its graph" runs beside the
 * current step.  sample_size above the number of training triples is an error; a graph whose sweeps do not
 * settle within the budget (sized at rgcn_neighborhood_reserve from the graph's diameter; graphs several thousand hops
 * across exceed its ceiling) is refused at the next synchronising call, never answered wrongly. */
rgcn_status rgcn_neighborhood_reserve(rgcn_ctx* ctx, const int32_t* triples_host, int64_t num_triples);
rgcn_status rgcn_sample_neighborhood_device(rgcn_ctx* ctx, int64_t sample_size, uint64_t seed, int32_t* batch_out_dev,
                                            int32_t on_prefetch_stream);

/* NegativeSampler.transform (code/common/auxilliaries.py:13-33) on the device: x_out = int32 [n*(rate+1), 3], the batch
 * tiled rate+1 times with, in every row after the first n, the object (fair coin) or else the subject replaced by a
 * uniform entity id; y_out = float32 [n*(rate+1)], 1 for the first n rows, 0 after.  Same layout and distribution as
 * the reference's numpy code, other random stream (counter-based, a function of `seed`).  Ids of `batch` are NOT
 * validated here; the decoder rejects out-of-range ids when it consumes x_out.  Asynchronous, capturable. */
rgcn_status rgcn_negative_sample_device(rgcn_ctx* ctx, const int32_t* batch_dev, int64_t n, int32_t rate, uint64_t seed,
                                        int32_t* x_out_dev, float* y_out_dev);

/* NegativeSampler.transform_exclusive (code/common/auxilliaries.py:35-73) on the device: the corruptions above, redrawn
 * while they are known positives.
 *
 * rgcn_known_positives_reserve hands over the set K of known positives once (the reference registers the training
 * triples: set_known_positives, code/train.py), int32 [num_triples,3] rows (s, r, o) in host memory:
 *   - ids are checked on the host: an s or o outside [0, EntityCount) or an r outside [0, RelationCount) is
 *     RGCN_ERR_INVALID, and an index reserved earlier stays in place and keeps answering;
 *   - duplicates collapse.  The index is the sorted array of the unique packed keys (r V + s) V + o, built on the host,
 *     deterministically, and copied to device memory the context owns; a lookup is a branch-free binary search;
 *   - RelationCount x EntityCount^2 >= 2^63, or num_triples >= 2^31 (the bound of the key count, checked before
 *     duplicates collapse): RGCN_ERR_UNSUPPORTED;
 *   - num_triples == 0 releases the index and switches rgcn_set_exclusive_negatives off; a new K replaces the old one,
 *     keeps the mode and restarts RGCN_BUF_NEGATIVE_UNRESOLVED at 0;
 *   - RGCN_ERR_STATE between rgcn_capture_begin and rgcn_capture_end (it reads host memory and synchronises); a graph
 *     captured with one index must not be launched after that index was replaced or released;
 *   - every kind, RGCN_KIND_EMBEDDING included, and sharded contexts: the index is replicated, there is no collective,
 *     every rank draws the same rows.
 *
 * rgcn_negative_sample_exclusive_device: arguments, layout and labels of rgcn_negative_sample_device.  For negative row
 * i >= n let j = i - n, (s, r, o) = batch[i mod n] and T = RGCN_NEG_MAX_DRAWS; all draws are 24-bit counter draws
 * bits(tag, index) of `seed`:
 *   - the coin is the plain sampler's, bits(0x6e65, 2 j) & 1 (1: the object is replaced), and is never redrawn (the
 *     reference redraws only the value);
 *   - attempt 0 is the plain sampler's draw bit for bit: u = bits(0x6e66, 2 j) << 24 | bits(0x6e67, 2 j + 1), candidate
 *     (u V) >> 48;
 *   - a candidate e is KNOWN iff (s, r, e) (object side) or (e, r, o) (subject side) is in K; a known candidate is
 *     redrawn: attempt t = 1 .. T - 1 draws u from bits(0x6e68, 2 (j T + t)) << 24 | bits(0x6e69, 2 (j T + t) + 1);
 *   - if all T candidates are known the row takes the first entity that is not, scanning upward cyclically from the last
 *     candidate (at most V lookups; probability p^T for a pair with known fraction p);
 *   - if every entity is known the row keeps attempt 0's candidate and RGCN_BUF_NEGATIVE_UNRESOLVED grows by one;
 *   - a batch row with an id out of range is corrupted as the plain sampler corrupts it, without a lookup; nothing is read
 *     out of bounds and the decoder rejects the row when it consumes x_out.
 * The result is a function of (K, batch, seed) alone; it differs from rgcn_negative_sample_device's for the same seed only
 * in rows whose plain draw is known, and there only in the corrupted column; no negative row is in K unless the counter
 * counted it.  Asynchronous, capturable (replay k draws with seed + k, as the plain call).  RGCN_ERR_STATE without an index.
 *
 * rgcn_set_exclusive_negatives(ctx, 1): the negative sampling inside rgcn_train_step_minibatch_device is the exclusive one,
 * with that call's negative_seed.  RGCN_ERR_STATE without an index and during a capture.  Default 0: every call produces
 * the bytes it produced before these entry points existed. */
#define RGCN_NEG_MAX_DRAWS 32
rgcn_status rgcn_known_positives_reserve(rgcn_ctx* ctx, const int32_t* triples_host, int64_t num_triples);
rgcn_status rgcn_negative_sample_exclusive_device(rgcn_ctx* ctx, const int32_t* batch_dev, int64_t n, int32_t rate,
                                                  uint64_t seed, int32_t* x_out_dev, float* y_out_dev);
rgcn_status rgcn_set_exclusive_negatives(rgcn_ctx* ctx, int32_t on);

/* Relation corruptions: negative rows (s, r', o) with a wrong RELATION, behind the entity corruptions above.  Not in the
 * reference, whose sampler replaces entities only: W_relation is then trained to separate entities under a fixed
 * relation, never relations for a fixed pair -- the question rgcn_rank_relation_device asks.
 *
 * rgcn_negative_sample_relation_device: a batch with relation_rate = m > 0 has N = n (1 + rate + m) rows;
 * x_out_dev int32 [N,3], y_out_dev float [N].
 *   - rows [0, n (rate + 1)) are exactly what rgcn_negative_sample_device writes for the same (batch, n, rate, seed) --
 *     with exclusive != 0 what rgcn_negative_sample_exclusive_device writes -- bit for bit: the same kernels write them;
 *   - row i >= n (rate + 1), with j = i - n (rate + 1) and (s, r, o) = batch[j mod n], has label 0, s and o unchanged and
 *     the relation r'.  All draws are 24-bit counter draws bits(tag, index) of `seed`, T = RGCN_NEG_MAX_DRAWS:
 *       - attempt 0 draws u = bits(0x6e6a, 2 j) << 24 | bits(0x6e6b, 2 j + 1), c = (u (R - 1)) >> 48, and the candidate is
 *         r' = c + (c >= r): uniform over the R - 1 OTHER relations, the row's own relation is never drawn (at R = 18 a
 *         uniform draw over all R would label a positive as negative in 1 row of 18);
 *       - exclusive == 0: attempt 0 is the row;
 *       - exclusive != 0: a candidate is KNOWN iff (s, r', o) is in K; a known candidate is redrawn, attempt t = 1 .. T - 1
 *         from bits(0x6e6c, 2 (j T + t)) << 24 | bits(0x6e6d, 2 (j T + t) + 1);
 *       - if all T candidates are known the row takes the first relation that is not, scanning upward cyclically from the
 *         last candidate and passing over r (at most R - 1 lookups);
 *       - if every other relation is known the row keeps attempt 0's candidate and RGCN_BUF_NEGATIVE_RELATION_UNRESOLVED
 *         grows by one (RGCN_BUF_NEGATIVE_UNRESOLVED counts the entity rows only, as before);
 *       - a batch row with an id out of range takes r' = c of attempt 0, without the skip and without a lookup; nothing is
 *         read out of bounds and the decoder rejects the row when it consumes x_out.
 *   - the result is a function of (K, batch, seed) alone; the exclusive relation rows differ from the plain ones for the
 *     same seed only in rows whose attempt-0 candidate is known, and there only in column 1;
 *   - relation_rate in [0, 1024]; relation_rate == 0 is rgcn_negative_sample_device (exclusive != 0: its exclusive form);
 *     relation_rate > 0 with RelationCount < 2, and N above RGCN_MAX_DECODER_TRIPLES: RGCN_ERR_INVALID; exclusive != 0
 *     without an index: RGCN_ERR_STATE;
 *   - RGCN_ERR_STATE between rgcn_capture_begin and rgcn_capture_end: capture is not built for it;
 *   - asynchronous on the main stream; every kind, RGCN_KIND_EMBEDDING included;
 *   - a batch with relation rows is not the tiled batch of rgcn_negative_sample_device (copies of a triple no longer share
 *     a relation): the decoder prepares it as it prepares any caller's X.
 *
 * rgcn_set_relation_negatives(ctx, m): rgcn_train_step_minibatch_device appends m relation rows per batch edge, exclusive
 * iff rgcn_set_exclusive_negatives is on, with that call's negative_seed.  The step's N is n (1 + rate + m): the scratch
 * buffers and rgcn_decoder_reserve must cover it (RGCN_ERR_STATE).  RGCN_ERR_STATE during a capture, from this call and
 * from the step while m > 0; m > 0 on a context with world > 1: RGCN_ERR_UNSUPPORTED; RelationCount < 2: RGCN_ERR_INVALID.
 * Default 0: every call produces the bytes it produced before these entry points existed, the tiled path included. */
rgcn_status rgcn_negative_sample_relation_device(rgcn_ctx* ctx, const int32_t* batch_dev, int64_t n, int32_t rate,
                                                 int32_t relation_rate, int32_t exclusive, uint64_t seed,
                                                 int32_t* x_out_dev, float* y_out_dev);
rgcn_status rgcn_set_relation_negatives(rgcn_ctx* ctx, int32_t relation_rate);

/* Type-constrained negatives and queries: corruptions and candidates from the entities the training set has seen in that
 * slot of that relation (the local closed-world assumption of Krompass et al., 2015; PyKEEN's "pseudo-typed" sampler).
 * Not in the reference.
 *
 * rgcn_type_sets_reserve hands over the triples T once (the training triples, as for rgcn_known_positives_reserve), int32
 * [num_triples,3] rows (s, r, o) in host memory.  domain(r) = the sorted unique subjects of r in T, range(r) = the sorted
 * unique objects; list l = side R + r with side 0 = subjects, side 1 = objects (the sampler's coin, the queries'
 * predict_object).  A list with fewer than RGCN_TYPED_MIN_CANDIDATES members is OPEN and stands for all V entities
 * everywhere below: a relation T never saw, or a slot with a single filler, constrains nothing.
 *   - ids are checked on the host: an s or o outside [0, EntityCount) or an r outside [0, RelationCount) is
 *     RGCN_ERR_INVALID naming the row, and sets reserved earlier stay in place and keep answering;
 *   - the sets are built on the host, deterministically, and copied to device memory the context owns: ptr int64 [2R+1],
 *     idx int32 [ptr[2R]], and a bit mask uint32 [2R][W], W = ceil(V/32), bit e of row l set iff e is in list l (an open
 *     list: all V bits; the pad bits of the last word are clear);
 *   - 2 R W >= 2^31 or num_triples >= 2^31: RGCN_ERR_UNSUPPORTED (arithmetic, nothing is allocated);
 *   - num_triples == 0 releases the sets and switches rgcn_set_typed_negatives off; a new T replaces the old one, keeps
 *     the mode and restarts RGCN_BUF_NEGATIVE_TYPED_OPEN at 0;
 *   - RGCN_ERR_STATE between rgcn_capture_begin and rgcn_capture_end (it reads host memory and synchronises);
 *   - every kind, RGCN_KIND_EMBEDDING included, and sharded contexts: the sets are replicated.
 *
 * rgcn_negative_sample_typed_device: arguments, layout and labels of rgcn_negative_sample_device, and `exclusive`.  For
 * negative row i >= n let j = i - n, (s, r, o) = batch[i mod n], T = RGCN_NEG_MAX_DRAWS; draws are bits(tag, index) of `seed`:
 *   - the coin is the plain sampler's, bits(0x6e65, 2 j) & 1, never redrawn.  L = list (coin, r), m its length, own = the
 *     entity the coin replaces, p = the position of own in L (a branch-free binary search; -1: absent);
 *   - the row is TYPED iff its ids are in range, L is not open and n' = m - (p >= 0) >= 1.  Otherwise it is OPEN: drawn
 *     exactly as rgcn_negative_sample_device draws it -- exclusive != 0: as rgcn_negative_sample_exclusive_device, its
 *     unresolved count feeding RGCN_BUF_NEGATIVE_UNRESOLVED -- bit for bit, and RGCN_BUF_NEGATIVE_TYPED_OPEN grows by one;
 *   - a typed row's attempt 0 reads the plain sampler's 48 bits u = bits(0x6e66, 2 j) << 24 | bits(0x6e67, 2 j + 1):
 *     c = (u n') >> 48, c += (p >= 0 && c >= p), candidate L[c] -- uniform over the OTHER members of L, never own (with
 *     m = 2 a uniform draw over L would label the positive negative in half the rows; rgcn_negative_sample_relation_device
 *     skips r the same way);
 *   - exclusive != 0 on a typed row: a candidate is KNOWN as for the exclusive sampler and is redrawn, attempt
 *     t = 1 .. T - 1 from bits(0x6e68, 2 (j T + t)) << 24 | bits(0x6e69, 2 (j T + t) + 1) with the same skip; after T
 *     known candidates the row takes the first member of L that is not known, scanning positions upward cyclically from
 *     the last candidate and passing over p; if every other member is known the row becomes open (the open exclusive
 *     decision above, counted).  No typed row is ever left as a known positive;
 *   - a batch row with an id out of range is open and makes no lookup; nothing is read out of bounds.
 * The result is a function of (T, K, batch, seed) alone.  Asynchronous.  RGCN_ERR_STATE without sets, with exclusive != 0
 * and no index of known positives, and between rgcn_capture_begin and rgcn_capture_end (capture is not built for it).
 * The batch is the tiled one: copies of a triple still share their relation.
 *
 * rgcn_rank_typed_device: arguments, validation, comparison, tie rule and chunking of rgcn_rank_device.  Row i's
 * candidates are C = list (predict_object, r_i) + {gold_i}:
 *     raw      = #{e in C : score[e] >= score[gold]}
 *     filtered = raw - #{e in filter and in C : score[e] >= score[gold]} + 1
 * (a filter entry outside C is not subtracted).  With every list open: rgcn_rank_device's ranks bit for bit.
 *
 * rgcn_topk_typed_device: arguments, validation and selection of rgcn_topk_device; a row's exclusion mask starts from the
 * complement of its list instead of empty, so row i holds the min(k, |list \ excluded|) best members of the list, same
 * order, same fill values (-1 / -inf).  With every list open: rgcn_topk_device's bytes.
 * Both: RGCN_ERR_STATE without sets; no mixed form and no relation form; on a relation-sharded context every rank answers
 * its own queries, as rgcn_rank_device.
 *
 * rgcn_set_typed_negatives(ctx, 1): the negative sampling inside rgcn_train_step_minibatch_device is the typed one,
 * exclusive iff rgcn_set_exclusive_negatives is on, with that call's negative_seed; relation rows
 * (rgcn_set_relation_negatives) stay as they are, behind the typed entity rows.  RGCN_ERR_STATE without sets and during a
 * capture, and from the step itself during a capture while the mode is on; world > 1: RGCN_ERR_UNSUPPORTED.  Default 0:
 * every call produces the bytes and launches it produced before these entry points existed. */
#define RGCN_TYPED_MIN_CANDIDATES 2
rgcn_status rgcn_type_sets_reserve(rgcn_ctx* ctx, const int32_t* triples_host, int64_t num_triples);
rgcn_status rgcn_negative_sample_typed_device(rgcn_ctx* ctx, const int32_t* batch_dev, int64_t n, int32_t rate,
                                              int32_t exclusive, uint64_t seed, int32_t* x_out_dev, float* y_out_dev);
rgcn_status rgcn_set_typed_negatives(rgcn_ctx* ctx, int32_t on);
rgcn_status rgcn_rank_typed_device(rgcn_ctx* ctx, const int32_t* x_dev, int64_t num_queries, int32_t predict_object,
                                   const int64_t* filter_ptr_dev, const int32_t* filter_idx_dev, int32_t* raw_rank_dev,
                                   int32_t* filtered_rank_dev);
rgcn_status rgcn_topk_typed_device(rgcn_ctx* ctx, const int32_t* x_dev, int64_t num_queries, int32_t predict_object,
                                   int32_t k, const int64_t* exclude_ptr_dev, const int32_t* exclude_idx_dev,
                                   int32_t* topk_idx_dev, float* topk_energy_dev);

/* ---- reciprocal relations ([Decoder] ReciprocalRelations; Lacroix et al. 2018, Kazemi & Poole 2018) ------------------
 * DistMult's sum is symmetric in s and o.  Under the mode every relation has a second vector, used when the subject is
 * the unknown: (s, r, ?) is asked of W_relation[r], (?, r, o) of W_relation[RelationCount + r].  The storage is what it
 * always was: W_relation is [EntityCount, d], rows [R, 2 R) simply come into use.  No tensor or checkpoint shape changes.
 *
 * rgcn_reciprocal_rows_device: a pass over x_dev / y_dev that one of rgcn_negative_sample_device, its exclusive, relation
 * or typed form filled with the same n, rate, relation_rate and seed; the buffers hold n (rate + 2 + relation_rate) rows
 * (RGCN_ERR_STATE where the runtime can tell that they do not).  csrc/negative_reciprocal.h holds the decision, shared
 * with the host:
 *     rows [0, n)                      the positives: untouched
 *     rows [n, n (rate + 1))           the entity corruptions: a row whose SUBJECT was replaced -- the samplers' own coin,
 *                                      drop_bits(seed, 0x6e65, 2 (row - n)) & 1 == 0 -- has its relation r rewritten to
 *                                      r + R; no other word of these rows is written
 *     rows [n (rate + 1), n (rate + 1 + relation_rate))   the relation rows: untouched (forward relations)
 *     rows behind them, n of them      written: the inverse positives (s, r + R, o) of the batch, label 1
 * A relation outside [0, R) stays what it is.  The batch is no longer the tiled one: the decoder takes its general path.
 * Bad arguments and a batch above RGCN_MAX_DECODER_TRIPLES: RGCN_ERR_INVALID; 2 R > EntityCount: RGCN_ERR_UNSUPPORTED;
 * during a capture: RGCN_ERR_STATE.
 *
 * rgcn_set_reciprocal_relations(ctx, 1):
 *   - rgcn_train_step_minibatch_device runs the pass behind its sampler and trains on N = n (rate + 2 + relation_rate)
 *     rows, which its scratch buffers must hold (RGCN_ERR_STATE); the loss stays the mean over all N rows.
 *   - the decoder's relation bound is 2 R: rgcn_decoder_loss_backward_device, its weighted form and both fused steps take
 *     relations in [0, 2 R), W_relation's gradient has rows [0, 2 R) (the rows behind them stay zero), the optimizer
 *     updates and keeps state for them.  The buffers sized by the bound are rebuilt by the call: it may come before or
 *     after rgcn_decoder_reserve, and it waits for the work in flight.
 *   - the entity-side queries (rgcn_rank_device, rgcn_rank_typed_device, rgcn_rank_mixed_device, rgcn_topk_device,
 *     rgcn_topk_typed_device, rgcn_topk_mixed_device, rgcn_score_queries_device) with predict_object == 0 read
 *     W_relation[R + r]; r is validated against R first, as always, and a typed subject query still reads the list of
 *     (subject side, r).  predict_object != 0 and the relation queries do not change.
 *   - rgcn_adversarial_weights_device takes relations in [0, 2 R).  In a fused step under
 *     rgcn_set_adversarial_negatives the weights come from the rows in front of the inverse positives (num_positives
 *     groups, as ever) and the inverse positives, the last num_positives rows, take weight 1.
 *   - the relation-softmax term and the relation queries keep their R candidates.
 * RGCN_ERR_UNSUPPORTED: 2 R > EntityCount; world > 1; while rgcn_set_entity_softmax is on (and that call, and
 * rgcn_entity_softmax_device, while this mode is on: the term's subject rows and by-relation reduction are not built for
 * the 2 R rows); during a capture; rgcn_capture_begin while the mode is on.  Default 0: every call produces the bytes and
 * launches it produced before these entry points existed, and a relation >= R stays the error it was.  A model trained
 * without the mode and queried with it reads rows no step ever updated. */
rgcn_status rgcn_reciprocal_rows_device(rgcn_ctx* ctx, const int32_t* batch_dev, int64_t n, int32_t rate,
                                        int32_t relation_rate, uint64_t seed, int32_t* x_dev, float* y_dev);
rgcn_status rgcn_set_reciprocal_relations(rgcn_ctx* ctx, int32_t on);

/* The softmax-over-relations loss term: for every positive (s_n, r_n, o_n), n < P, the gold relation against ALL the
 * others at once -- the objective rgcn_rank_relation_device evaluates, which relation corruptions only sample.  Not in
 * the reference.  With c = the codes the decoder reads ([V, code width]; RGCN_KIND_EMBEDDING: W_emb) and W = rows
 * [0, RelationCount) of W_relation:
 *     q_n      = c[s_n] * c[o_n]                 elementwise, rounded once (the query row of rgcn_rank_relation_device)
 *     E[n,r']  = q_n . W[r']
 *     ell_n    = log sum_{r' in C_n} exp(E[n,r']) - E[n,r_n]            (the row maximum over C_n is subtracted)
 *     term     = weight / P * sum_n ell_n
 *     G[n,r']  = weight / P * (softmax over C_n of E[n,:] at r' - [r' = r_n]),  0 outside C_n
 *     dL/dW_relation[r'] += sum_n G[n,r'] q_n
 *     dq_n = sum_r' G[n,r'] W[r'];   dL/dcodes[s_n] += dq_n * c[o_n];   dL/dcodes[o_n] += dq_n * c[s_n]
 * (both on the same row when s_n = o_n).  C_n is every relation; with exclusive != 0 it is {r_n} and every r' for which
 * (s_n, r', o_n) is NOT in the set K of rgcn_known_positives_reserve: a relation that is a known fact for the pair is
 * neither a competitor nor a gradient target.  A row with C_n = {r_n} contributes exactly 0.  The regulariser does not
 * change.  Every sum has a fixed order (no atomics on floats): two calls return the same bytes.
 *
 * rgcn_relation_softmax_reserve(max_positives) sizes the term's buffers: query rows, their gradients and the energies of
 * ONE chunk of positives (rgcn_relation_softmax_plan: min(max_positives, 65536, what a 64 MB energy buffer holds)); longer
 * inputs are walked chunk by chunk, which is exact up to summation order.  max_positives <= 0 or above
 * RGCN_MAX_DECODER_TRIPLES, and RelationCount < 2: RGCN_ERR_INVALID; EntityCount >= 2^24: RGCN_ERR_UNSUPPORTED;
 * RGCN_ERR_STATE during a capture (it synchronises).
 *
 * rgcn_relation_softmax_device(positives_dev int32 [P,3], P, weight, exclusive): stand-alone.  Adds the term to the loss
 * (rgcn_get_loss) and to the gradients (rgcn_dcodes_device, W_relation's gradient) that the last
 * rgcn_decoder_loss_backward_device left; RGCN_ERR_STATE without one, before rgcn_relation_softmax_reserve, during a
 * capture, and with exclusive != 0 without an index.  weight negative or not finite, P <= 0, NULL positives,
 * RelationCount < 2: RGCN_ERR_INVALID; weight == 0: nothing is launched.  world > 1: RGCN_ERR_UNSUPPORTED.  Ids are
 * validated on the device: a positive with an id out of range fails the next synchronising call (rgcn_get_loss,
 * rgcn_sync) with RGCN_ERR_INVALID, nothing is read out of bounds, and the context stays usable.  Asynchronous on the
 * main stream.
 *
 * rgcn_set_relation_softmax(weight, num_positives, exclusive): the term inside the fused steps.  Under weight > 0
 *   - rgcn_train_step_minibatch_device takes its num_edges batch rows as the positives;
 *   - rgcn_train_step_device takes the first num_positives rows of its X, whose labels must be 1 (checked on the device:
 *     RGCN_ERR_INVALID at the next synchronising call); num_positives == 0 means "the minibatch step only" and such a
 *     step returns RGCN_ERR_STATE; num_positives above the step's N: RGCN_ERR_INVALID;
 *   - the steps need rgcn_relation_softmax_reserve (RGCN_ERR_STATE), return RGCN_ERR_UNSUPPORTED on a context with
 *     world > 1 and RGCN_ERR_STATE during a capture;
 *   - the top layer's dropout-scaled operand is formed by the backward pass from the complete dL/dcodes, not by the
 *     decoder's entity-gradient kernel.
 * weight == 0 (the default) restores every byte the steps produced before these entry points existed.  weight negative
 * or not finite, num_positives < 0, and weight > 0 with RelationCount < 2: RGCN_ERR_INVALID; weight > 0 during a capture,
 * and exclusive != 0 without an index: RGCN_ERR_STATE.
 *
 * rgcn_relation_softmax_plan: the term's host-side decisions as a context with these sizes runs them, context-free.
 * out[0] = chunk, out[1] = padded R (R up to a multiple of 4: the leading dimension of
 * RGCN_BUF_RELATION_SOFTMAX_ENERGIES / _G), out[2] = the split over the positives of the relation gradient's product at
 * a full chunk (its split-K slabs are the term's own, at most 2^23 floats), out[3] = the long-row cut of the entity side
 * (entity rows with more incidences in a chunk are summed in pieces), out[4] = the incidences per piece.  A non-positive
 * argument or NULL out: RGCN_ERR_INVALID. */
rgcn_status rgcn_relation_softmax_reserve(rgcn_ctx* ctx, int64_t max_positives);
rgcn_status rgcn_relation_softmax_device(rgcn_ctx* ctx, const int32_t* positives_dev, int64_t num_positives, float weight,
                                         int32_t exclusive);
rgcn_status rgcn_set_relation_softmax(rgcn_ctx* ctx, float weight, int64_t num_positives, int32_t exclusive);
rgcn_status rgcn_relation_softmax_plan(int64_t max_positives, int32_t num_relations, int32_t code_dim, int64_t out[5]);

/* The softmax-over-entities loss term ("1-N" scoring): for every positive (s_n, r_n, o_n), n < P, the gold object of
 * (s_n, r_n, ?) and the gold subject of (?, r_n, o_n) against ALL entities at once -- the objective rgcn_rank_device
 * evaluates, which the sampled corruptions only sample.  Not in the reference.  With c = the codes the decoder reads
 * ([V, code width]; RGCN_KIND_EMBEDDING: W_emb) and W = W_relation, every positive gives two rows, 2P in all: the object
 * row m = n (query entity a_m = s_n, gold g_m = o_n) and the subject row m = P + n (a_m = o_n, g_m = s_n):
 *     q_m      = c[a_m] * W[r_m]                 elementwise, rounded once (the query row of rgcn_rank_device)
 *     E[m,e]   = q_m . c[e]                      e in [0, V)
 *     ell_m    = log sum_{e in C_m} exp(E[m,e]) - E[m,g_m]               (the row maximum over C_m is subtracted)
 *     term     = weight / (2P) * sum_m ell_m
 *     G[m,e]   = weight / (2P) * (softmax over C_m of E[m,:] at e - [e = g_m]),  0 outside C_m
 *     dL/dcodes[e] += sum_m G[m,e] q_m           (the candidate side, all V rows)
 *     dq_m = sum_e G[m,e] c[e];   dL/dcodes[a_m] += dq_m * W[r_m];   dL/dW_relation[r_m] += dq_m * c[a_m]
 * The codes are a variable in both roles: there is no stop-gradient.  C_m is every entity; with exclusive != 0 it is
 * {g_m} and every e for which the completed triple -- (s_n, r_n, e) for an object row, (e, r_n, o_n) for a subject row --
 * is NOT in the set K of rgcn_known_positives_reserve.  A row with C_m = {g_m} contributes exactly 0.  The regulariser
 * does not change.  Every sum has a fixed order (no atomics on floats): two calls return the same bytes.
 *
 * rgcn_entity_softmax_reserve(max_positives) sizes the term's buffers: query rows, their gradients and the energies of
 * ONE chunk of rows (rgcn_entity_softmax_plan: min(2 max_positives, 65536, what a 256 MB energy buffer holds)); longer
 * inputs are walked chunk by chunk, which is exact up to summation order.  max_positives <= 0 or above
 * RGCN_MAX_DECODER_TRIPLES, and EntityCount < 2: RGCN_ERR_INVALID; EntityCount or RelationCount >= 2^24:
 * RGCN_ERR_UNSUPPORTED; RGCN_ERR_STATE during a capture (it synchronises).
 *
 * rgcn_entity_softmax_device(positives_dev int32 [P,3], P, weight, exclusive): stand-alone.  Adds the term to the loss
 * (rgcn_get_loss) and to the gradients (rgcn_dcodes_device, W_relation's gradient) that the last
 * rgcn_decoder_loss_backward_device left; RGCN_ERR_STATE without one, before rgcn_entity_softmax_reserve, during a
 * capture, and with exclusive != 0 without an index.  weight negative or not finite, P <= 0, NULL positives,
 * EntityCount < 2: RGCN_ERR_INVALID; weight == 0: nothing is launched.  world > 1: RGCN_ERR_UNSUPPORTED.  Ids are
 * validated on the device: a positive with an id out of range fails the next synchronising call (rgcn_get_loss,
 * rgcn_sync) with RGCN_ERR_INVALID, its rows of G are zero, nothing is read out of bounds, and the context stays usable.
 * Asynchronous on the main stream.
 *
 * rgcn_set_entity_softmax(weight, num_positives, exclusive): the term inside the fused steps.  Under weight > 0
 *   - rgcn_train_step_minibatch_device takes its num_edges batch rows as the positives (the leading num_positives of
 *     them where num_positives > 0 is smaller);
 *   - rgcn_train_step_device takes the first num_positives rows of its X, whose labels must be 1 (checked on the device:
 *     RGCN_ERR_INVALID at the next synchronising call); num_positives == 0 means "the minibatch step only" and such a
 *     step returns RGCN_ERR_STATE; num_positives above the step's N: RGCN_ERR_INVALID;
 *   - the steps need rgcn_entity_softmax_reserve (RGCN_ERR_STATE), return RGCN_ERR_UNSUPPORTED on a context with
 *     world > 1 and RGCN_ERR_STATE during a capture;
 *   - the term runs on the main stream behind the decoder (and behind the relation-softmax term where that is on), and
 *     the top layer's dropout-scaled operand is formed by the backward pass from the complete dL/dcodes.
 * weight == 0 (the default) restores every byte the steps produced before these entry points existed.  weight negative
 * or not finite, num_positives < 0, and weight > 0 with EntityCount < 2: RGCN_ERR_INVALID; weight > 0 during a capture,
 * and exclusive != 0 without an index: RGCN_ERR_STATE.  The term may be on together with rgcn_set_relation_softmax,
 * rgcn_set_relation_negatives and rgcn_set_adversarial_negatives: the terms add.
 *
 * rgcn_entity_softmax_plan: the term's host-side decisions as a context with these sizes runs them, context-free.
 * out[0] = chunk (ROWS, two per positive), out[1] = padded V (V up to a multiple of 4: the leading dimension of
 * RGCN_BUF_ENTITY_SOFTMAX_G), out[2] = the split over the rows of the candidate gradient's product at a full chunk (its
 * split-K slabs are the term's own, at most 2^24 floats), out[3] = the long-row cut of the query side (query entities
 * and relations with more rows in a chunk are summed in pieces), out[4] = the rows per piece.  A non-positive argument
 * or NULL out: RGCN_ERR_INVALID. */
rgcn_status rgcn_entity_softmax_reserve(rgcn_ctx* ctx, int64_t max_positives);
rgcn_status rgcn_entity_softmax_device(rgcn_ctx* ctx, const int32_t* positives_dev, int64_t num_positives, float weight,
                                       int32_t exclusive);
rgcn_status rgcn_set_entity_softmax(rgcn_ctx* ctx, float weight, int64_t num_positives, int32_t exclusive);
rgcn_status rgcn_entity_softmax_plan(int64_t max_positives, int32_t num_entities, int32_t code_dim, int64_t out[5]);

/* Self-adversarial negatives (Sun et al., RotatE, 2019) and the weighted decoder under them.  Not in the reference, which
 * weighs every row 1.  A decoder batch of N rows is laid out as every sampler here writes it: the first P rows are the
 * positives (label 1), every later row i (label 0) is a negative of positive i mod P; K = N / P - 1.  With temperature
 * alpha, energies x and G_b = {b + t P, t = 1..K}:
 *     p_i  = exp(alpha x_i - M_b) / sum_{j in G_b} exp(alpha x_j - M_b),   M_b = max_{j in G_b} alpha x_j
 *     w_i  = K p_i for a negative,   w_b = 1 for a positive
 *     loss = (1/N) sum_n w_n xent(x_n, y_n) + the regulariser (unweighted);   dx_n = w_n ((sigmoid(x_n) - y_n) / N)
 * The weights are constants: nothing differentiates through them.  A group's weights sum to K, so sum w = N and the
 * scale of the loss stays what it is; alpha -> 0 gives the unweighted loss.  The softmax is evaluated in double from the
 * float energies and rounded once, every sum has a fixed order (no atomics on floats): two calls return the same bytes.
 *
 * rgcn_decoder_loss_backward_weighted_device: rgcn_decoder_loss_backward_device with a caller's weight per row
 * (w_dev float [N]) on the row's loss term and gradient.  w_dev == NULL is that call; weights of 1.0f reproduce its bytes.
 * Weights must be finite and >= 0, checked on the device: RGCN_ERR_INVALID at the next synchronising call.
 *
 * rgcn_adversarial_weights_device: writes the weights above, for the codes of the last forward pass (RGCN_KIND_EMBEDDING:
 * W_emb), into w_out_dev (float [N]).  Asynchronous on the main stream; reads x_dev only, no rgcn_decoder_reserve needed.
 * num_triples % num_positives != 0, num_positives <= 0, a NULL pointer, a temperature that is negative or not finite:
 * RGCN_ERR_INVALID.  K = 0 or temperature == 0: all ones (a fill).  Before a forward pass: RGCN_ERR_STATE.  A row with
 * an id out of range reads nothing out of bounds, takes no part in its group and gets weight 0 (the decoder rejects
 * such a batch).
 *
 * rgcn_set_adversarial_negatives(temperature, num_positives): the weights inside the fused steps.  Under temperature > 0
 *   - rgcn_train_step_minibatch_device takes its num_edges batch rows as the positives;
 *   - rgcn_train_step_device takes num_positives; 0 means "the minibatch step only" and such a step returns
 *     RGCN_ERR_STATE; a value that does not divide the step's N: RGCN_ERR_INVALID (RGCN_KIND_EMBEDDING included);
 *   - the labels are checked on the device (1 for the positives, 0 behind them): RGCN_ERR_INVALID at the next
 *     synchronising call;
 *   - the steps return RGCN_ERR_UNSUPPORTED on a context with world > 1 (the sharded decoder cuts the batch by rows, and
 *     the groups with them) and RGCN_ERR_STATE during a capture;
 *   - the step's weights stay readable as RGCN_BUF_ADVERSARIAL_WEIGHTS.
 * The relation-softmax term is not weighted.  temperature == 0 (the default) restores every byte and launch the steps
 * produced before these entry points existed.  temperature negative or not finite, num_positives < 0: RGCN_ERR_INVALID;
 * temperature > 0 during a capture: RGCN_ERR_STATE. */
rgcn_status rgcn_decoder_loss_backward_weighted_device(rgcn_ctx* ctx, const int32_t* x_dev, const float* y_dev,
                                                       const float* w_dev, int64_t num_triples,
                                                       float regularization_parameter);
rgcn_status rgcn_adversarial_weights_device(rgcn_ctx* ctx, const int32_t* x_dev, int64_t num_triples, int64_t num_positives,
                                            float temperature, float* w_out_dev);
rgcn_status rgcn_set_adversarial_negatives(rgcn_ctx* ctx, float temperature, int64_t num_positives);

/* ---- evaluation: raw and filtered link-prediction ranks -------------------------------
 * Replaces Model.score_all_subjects / score_all_objects + Scorer.evaluate_mrr + MrrScore.append_line
 * (code/model.py:59-81, code/decoders/bilinear_diag.py:51-61, code/common/evaluation.py:148-153,349-389).
 * For every query triple x[i] = (s, r, o): score every entity e as sigmoid(sum_k codes[e,k] (W_relation[r] *
 * codes[o])[k]) (predict_object = 0: rank the subject) or sigmoid(sum_k (codes[s] * W_relation[r])[k] codes[e,k])
 * (predict_object = 1) on the codes of the last rgcn_forward, then
 *   raw_rank[i]      = #{e : score[e] >= score[gold]}
 *   filtered_rank[i] = raw_rank[i] - #{e in filter_idx[filter_ptr[i] : filter_ptr[i+1]] : score[e] >= score[gold]} + 1
 * (the filter list holds the known completions of the pair, the gold entity among them).  Comparisons are made
 * on fp32 sigmoid values as in the reference (saturated scores tie).  Everything is a device pointer;
 * rgcn_rank_reserve(max_queries) sizes the [max_queries, V] score buffer, longer inputs are chunked.
 * Relation-sharded contexts: the codes are replicated after the forward pass, so each rank ranks its own slice
 * of the queries (no collective) and the caller concatenates. */
rgcn_status rgcn_rank_reserve(rgcn_ctx* ctx, int64_t max_queries);
rgcn_status rgcn_rank_device(rgcn_ctx* ctx, const int32_t* x_dev, int64_t num_queries, int32_t predict_object,
                             const int64_t* filter_ptr_dev, const int32_t* filter_idx_dev, int32_t* raw_rank_dev,
                             int32_t* filtered_rank_dev);

/* ---- ensemble ranks: the rank of the gold entity under the weighted sum of TWO models' scores -----------------
 * The reference's R-GCN+ (code/tools/ensemble.py, WeightEnsemble.combine_prediction) on score matrices that never leave
 * the device.  rgcn_rank_energies_device = the device pointer of RGCN_BUF_RANK_ENERGIES (NULL before rgcn_rank_reserve).
 * partner_energies = float [num_queries, V], row-major: the OTHER model's energies for the same queries in the same
 * order -- another context's rgcn_rank_energies_device or any buffer on this context's device; the caller guarantees
 * that it is complete before the call and untouched until the call returns.
 * The call scores the queries exactly as rgcn_rank_device does (same query kernel, same GEMM, same buffer:
 * RGCN_BUF_RANK_ENERGIES holds the context's own energies afterwards, unmodified) and ranks on
 *     m[e] = (float)((double)weight * s_own[e] + (1.0 - (double)weight) * s_partner[e])
 * with s_* the fp32 sigmoid of each energy (evaluated in double, rounded once, as rgcn_rank_device's) and the mix
 * evaluated in double without fused multiply-add and rounded once:
 *     raw_rank[i]      = #{e : m[e] >= m[gold]}
 *     filtered_rank[i] = raw_rank[i] - #{e in the row's filter list : m[e] >= m[gold]} + 1.
 * weight = 1 returns rgcn_rank_device's ranks bit for bit (for finite partner energies); weight = 0 the partner's.
 * Saturated scores tie, as there.  ONE chunk only: num_queries above what rgcn_rank_reserve sized is RGCN_ERR_INVALID
 * (the partner's buffer has its own chunking).  weight outside [0, 1], or NaN: RGCN_ERR_INVALID.  Ids and filter lists
 * are validated as by rgcn_rank_device, through the same check kernel; RGCN_ERR_STATE before a forward pass or before
 * rgcn_rank_reserve.  Synchronises at the end, as rgcn_rank_device does. */
const float* rgcn_rank_energies_device(rgcn_ctx* ctx);
rgcn_status rgcn_rank_mixed_device(rgcn_ctx* ctx, const int32_t* x_dev, int64_t num_queries, int32_t predict_object,
                                   const float* partner_energies_dev, float weight, const int64_t* filter_ptr_dev,
                                   const int32_t* filter_idx_dev, int32_t* raw_rank_dev, int32_t* filtered_rank_dev);

/* ---- prediction: the k most plausible entities of a query, best first ------------------------------------
 * What a trained link predictor is asked: given (s, r, ?) or (?, r, o), which entities complete it.  Selects from the
 * scores of BilinearDiag.predict_all_object_scores / predict_all_subject_scores (code/decoders/bilinear_diag.py:51-61;
 * the reference has no top-k call: its users sort the [queries, V] score matrix on the host).
 * x = int32 [N,3] rows (s, r, o).  predict_object = 1: the candidates are objects, s and r are read, the o column is
 * NOT read and may hold anything (e.g. -1); predict_object = 0: candidates are subjects, r and o are read, s is not.
 * The two ids that are read are validated on the device as rgcn_rank_device does it (RGCN_ERR_INVALID, no result).
 * The energies are the ones rgcn_rank_device scores -- same query kernel, same GEMM, same buffers sized by
 * rgcn_rank_reserve, longer inputs chunked alike -- and RGCN_BUF_RANK_ENERGIES holds the last chunk's afterwards,
 * unmodified (exclusion is a bit mask beside them, never a write into them).
 * exclude_ptr int64 [N+1] / exclude_idx int32: CSR of the entity ids that may not appear in row i's answer (the known
 * completions of the pair); both NULL = exclude nothing.  Validated like the filter lists of rgcn_rank_device (ranges
 * monotone and within exclude_ptr[N], entries in [0, V), duplicates allowed).
 * Row i of the result holds the min(k, V - #distinct excluded) best remaining entities ordered by (energy descending,
 * entity id ascending), energies compared as floats in their numeric order with -0.0 below +0.0 -- a total order, so
 * the answer is a function of the energies alone, ties included, and two calls on the same energies return the same
 * bytes.  The sigmoid is monotone: this order refines the reference's order by score.  topk_idx int32 [N,k],
 * topk_energy float [N,k] (the buffer's values, bit for bit; sigmoid is left to the caller); slots a row cannot fill
 * hold id -1 and energy -INFINITY.
 * 1 <= k <= min(V, RGCN_MAX_TOPK), else RGCN_ERR_INVALID.  Needs a completed rgcn_forward and rgcn_rank_reserve
 * (RGCN_ERR_STATE).  EntityCount above RGCN_MAX_TOPK_ENTITIES is RGCN_ERR_UNSUPPORTED: a row's exclusion mask (one bit
 * per entity, 64 KB at the limit) lives in LDS.  Relation-sharded contexts: as rgcn_rank_device, every rank answers
 * its own queries, no collective.  Synchronises at the end (it reads the validation verdict): not capturable. */
#define RGCN_MAX_TOPK 1024
#define RGCN_MAX_TOPK_ENTITIES 524288
rgcn_status rgcn_topk_device(rgcn_ctx* ctx, const int32_t* x_dev, int64_t num_queries, int32_t predict_object,
                             int32_t k, const int64_t* exclude_ptr_dev, const int32_t* exclude_idx_dev,
                             int32_t* topk_idx_dev, float* topk_energy_dev);

/* ---- ensemble prediction: the k most plausible entities under the weighted sum of TWO models' scores -----------
 * rgcn_topk_device's question put to the mixture rgcn_rank_mixed_device ranks (the reference's R-GCN+).
 *
 * rgcn_score_queries_device is how the partner model produces its energies for queries that have no gold entity: it runs
 * rgcn_topk_device's validation (the two ids that are read, on the device; the predicted column is not read and may be
 * -1), query kernel and GEMM and nothing after them, so that RGCN_BUF_RANK_ENERGIES (rgcn_rank_energies_device) holds,
 * bit for bit, what rgcn_topk_device leaves there for the same queries.  ONE chunk only: num_queries above what
 * rgcn_rank_reserve sized is RGCN_ERR_INVALID (the buffer holds one chunk).  RGCN_ERR_STATE before a forward pass or
 * before rgcn_rank_reserve.  Synchronises at the end (it reads the validation verdict): not capturable.
 *
 * rgcn_topk_mixed_device: queries, their validation, the limits on k, the exclusion CSR, RGCN_MAX_TOPK and
 * RGCN_MAX_TOPK_ENTITIES are rgcn_topk_device's; partner_energies (float [num_queries, V], row-major, on this device,
 * complete before the call, untouched until it returns, only read) and weight (outside [0, 1] or NaN: RGCN_ERR_INVALID)
 * are rgcn_rank_mixed_device's.  The partner may be this context's own RGCN_BUF_RANK_ENERGIES of an earlier call only
 * through a copy: the call rewrites that buffer with its own energies.  ONE chunk only, as the mixed rank.
 * The call scores its queries as rgcn_topk_device does (RGCN_BUF_RANK_ENERGIES holds the context's own energies
 * afterwards, unmodified), then forms for every entity of every row
 *     m[e] = (float)((double)weight * s_own[e] + (1.0 - (double)weight) * s_partner[e])
 * exactly as rgcn_rank_mixed_device does (the same device function: fp32 sigmoids evaluated in double and rounded once,
 * the mix in double without fused multiply-add, rounded once) into a scratch of [reserved queries, V] floats,
 * RGCN_BUF_RANK_MIXED_SCORES, and selects from that scratch with rgcn_topk_device's selection: row i of the result holds
 * the min(k, V - #distinct excluded) best remaining entities ordered by (m descending, entity id ascending) -- a total
 * order on the stored floats, so two calls on the same inputs return the same bytes.  topk_idx int32 [N,k], topk_score
 * float [N,k] (the scratch's values, bit for bit); slots a row cannot fill hold id -1 and score -INFINITY.  NaN partner
 * energies leave that row's answer unspecified; nothing faults.
 * The scratch is allocated by the first call after rgcn_rank_reserve (RGCN_ERR_NOMEM if it does not fit) and released
 * with the other ranking buffers: a context that is never asked for the mixture never holds it.
 * Synchronising, capture (RGCN_ERR_STATE), relation-sharded contexts and RGCN_KIND_EMBEDDING: as rgcn_topk_device. */
rgcn_status rgcn_score_queries_device(rgcn_ctx* ctx, const int32_t* x_dev, int64_t num_queries,
                                      int32_t predict_object);
rgcn_status rgcn_topk_mixed_device(rgcn_ctx* ctx, const int32_t* x_dev, int64_t num_queries, int32_t predict_object,
                                   int32_t k, const float* partner_energies_dev, float weight,
                                   const int64_t* exclude_ptr_dev, const int32_t* exclude_idx_dev,
                                   int32_t* topk_idx_dev, float* topk_score_dev);

/* ---- relation queries: which relation holds between two given entities ------------------------------------
 * The decoder's third question: (s, ?, o).  The reference scores subjects and objects only; the energy is the same
 * DistMult sum with the relation as the free index,
 *     energy[r'] = sum_k (codes[s] * codes[o])[k] W_relation[r', k]      for r' in [0, RelationCount),
 * on the codes of the last rgcn_forward.  The pair row codes[s] * codes[o] is rounded to fp32 once, then the same NT GEMM
 * as rgcn_rank_device's runs against W_relation instead of the codes.  The energies go to a buffer of their own,
 * RGCN_BUF_RELATION_ENERGIES (float [reserved queries, RelationCount], row stride RelationCount, the last chunk's):
 * RGCN_BUF_RANK_ENERGIES is not touched by any of these calls, nor this buffer by an entity-side call.  The buffer is
 * allocated by the first relation call after rgcn_rank_reserve (RGCN_ERR_NOMEM if it does not fit) and released with the
 * other ranking buffers: a context that is never asked about relations never holds it.
 * rgcn_relation_energies_device = its device pointer, NULL before the first relation call.
 * x = int32 [N,3] rows (s, r, o).  rgcn_rank_relation_device reads all three columns, r being the gold relation;
 * rgcn_topk_relation_device and rgcn_score_relation_queries_device read s and o only, the r column may hold anything
 * (e.g. -1).  The ids that are read are validated on the device, s and o in [0, V), a gold r in [0, RelationCount)
 * (RGCN_ERR_INVALID, no usable result).
 * Ranks: comparison and tie rule of rgcn_rank_device (fp32 sigmoid evaluated in double and rounded once, so saturated
 * scores tie):
 *   raw_rank[i]      = #{r' : score[r'] >= score[gold]}
 *   filtered_rank[i] = raw_rank[i] - #{r' in filter_idx[filter_ptr[i] : filter_ptr[i+1]] : score[r'] >= score[gold]} + 1
 * (the filter list holds the relations known between the pair, the gold one among them); ranges validated as
 * rgcn_rank_device's, entries in [0, RelationCount).
 * Top-k: rgcn_topk_device's selection over the relations.  1 <= k <= min(RelationCount, RGCN_MAX_TOPK), else
 * RGCN_ERR_INVALID.  Row i holds the min(k, RelationCount - #distinct excluded) best remaining relation ids ordered by
 * (energy descending, id ascending), energies compared as floats in their numeric order with -0.0 below +0.0;
 * topk_energy holds the buffer's values bit for bit, slots a row cannot fill hold id -1 and energy -INFINITY.
 * exclude_ptr / exclude_idx: CSR of relation ids in [0, RelationCount), both NULL = exclude nothing (one NULL:
 * RGCN_ERR_INVALID).  RelationCount above RGCN_MAX_TOPK_ENTITIES is RGCN_ERR_UNSUPPORTED (the mask lives in LDS).
 * RelationCount above EntityCount is RGCN_ERR_UNSUPPORTED for all three calls: W_relation is stored [EntityCount, d] as
 * in the reference, and its first RelationCount rows are the candidates.
 * Rank and top-k chunk inputs longer than the reserve; score is ONE chunk only (num_queries above the reserve:
 * RGCN_ERR_INVALID).  num_queries = 0 is RGCN_OK.  RGCN_ERR_STATE before a forward pass, before rgcn_rank_reserve and
 * between rgcn_capture_begin and rgcn_capture_end: the calls synchronise at the end (they read the validation verdict).
 * RGCN_KIND_EMBEDDING and relation-sharded contexts: as rgcn_topk_device (codes and W_relation are replicated, every rank
 * answers its own queries, no collective).  The 2R directed relations of the encoder are not candidates, and there is no
 * mixed form. */
rgcn_status rgcn_score_relation_queries_device(rgcn_ctx* ctx, const int32_t* x_dev, int64_t num_queries);
const float* rgcn_relation_energies_device(rgcn_ctx* ctx);
rgcn_status rgcn_rank_relation_device(rgcn_ctx* ctx, const int32_t* x_dev, int64_t num_queries,
                                      const int64_t* filter_ptr_dev, const int32_t* filter_idx_dev,
                                      int32_t* raw_rank_dev, int32_t* filtered_rank_dev);
rgcn_status rgcn_topk_relation_device(rgcn_ctx* ctx, const int32_t* x_dev, int64_t num_queries, int32_t k,
                                      const int64_t* exclude_ptr_dev, const int32_t* exclude_idx_dev,
                                      int32_t* topk_idx_dev, float* topk_energy_dev);

/* GradientClipping(max_norm) + Adam(lr) of the Converge chain (optimization/tensorflow_backend/
 * algorithms.py:27-42,58-68).  max_grad_norm = 0 disables clipping. */
rgcn_status rgcn_optimizer_config(rgcn_ctx* ctx, float learning_rate, float beta1, float beta2, float epsilon,
                                  float max_grad_norm);
/* The reference's three [Algorithm] Name= values of the TensorFlow backend (algorithms.py:5-55) behind the same clip.
 * With scale = the clip's factor (1 when max_grad_norm = 0) and g = scale * gradient:
 *   RGCN_OPT_ADAM              as rgcn_optimizer_config; two state slots per parameter (0: m, 1: v), zeros at first;
 *   RGCN_OPT_GRADIENT_DESCENT  tf.train.GradientDescentOptimizer(lr): w -= lr g; no state;
 *   RGCN_OPT_ADAGRAD           tf.train.AdagradOptimizer(lr): a += g^2, w -= lr g / sqrt(a); one slot (the accumulator),
 *                              filled with initial_accumulator (TensorFlow's default: 0.1) at first; there is no epsilon.
 * An algorithm reads its own fields only (beta1, beta2, epsilon: Adam; initial_accumulator: AdaGrad).  struct_size must be
 * sizeof(rgcn_optimizer_params).  Configuring the algorithm a context already has keeps its state and step count (a new
 * initial_accumulator fills only slots created afterwards); another algorithm releases the state, restarts the count at 0
 * and is RGCN_ERR_STATE during a capture (a graph captured before it must not be launched again). */
enum { RGCN_OPT_ADAM = 0, RGCN_OPT_GRADIENT_DESCENT = 1, RGCN_OPT_ADAGRAD = 2 };
typedef struct rgcn_optimizer_params {
  int32_t struct_size, algorithm;
  float learning_rate, beta1, beta2, epsilon, max_grad_norm, initial_accumulator;
} rgcn_optimizer_params;
rgcn_status rgcn_optimizer_config_ex(rgcn_ctx* ctx, const rgcn_optimizer_params* params);
/* The optimizer's state, for inspection and for continuing a run.  A slot has its parameter's shape and travels in the
 * parameter's host layout (as rgcn_get_param / rgcn_set_param; count = the parameter's element count).  W_relation carries
 * state for its first RelationCount rows only: the other rows read as the slot's initial value and are ignored when
 * written.  A slot that no step has created yet is created by the call (zeros, or initial_accumulator).  The step count is
 * the DEVICE's (it advances inside the step, so a replayed hipGraph counts too): rgcn_get_optimizer_step synchronises.
 * RGCN_ERR_STATE before rgcn_optimizer_config(_ex) and during a capture; RGCN_ERR_INVALID for a parameter that has no
 * gradient (the unused layer bias) and for slot outside [0, rgcn_optimizer_slot_count); RGCN_ERR_UNSUPPORTED on a
 * world > 1 context (a relation's state is current on its owner only). */
int32_t     rgcn_optimizer_slot_count(const rgcn_ctx* ctx);      /* Adam 2 (m, v), AdaGrad 1, GradientDescent 0 */
rgcn_status rgcn_get_optimizer_slot(rgcn_ctx* ctx, int32_t param, int32_t slot, float* host, int64_t count);
rgcn_status rgcn_set_optimizer_slot(rgcn_ctx* ctx, int32_t param, int32_t slot, const float* host, int64_t count);
rgcn_status rgcn_get_optimizer_step(rgcn_ctx* ctx, int64_t* t);
rgcn_status rgcn_set_optimizer_step(rgcn_ctx* ctx, int64_t t);   /* 0 <= t < 2^24 */
rgcn_status rgcn_optimizer_step(rgcn_ctx* ctx);
/* The same step in two phases around its one exchange point on a relation-sharded context: the
 * squared norm of the relation-sharded gradients (block W_forward / W_backward, basis C_forward / C_backward:
 * owner-only, zero elsewhere) is a sum over ranks.  _norm_partial leaves this rank's share in
 * RGCN_BUF_NORM_EXCHANGE; the caller sum-all-reduces it (rgcn_optimizer_step does, with RCCL); _apply clips by
 * the global norm and runs the configured algorithm.  Replicated tensors receive identical updates on every rank; a relation's
 * weights are current on its owner only, so the owner map must stay fixed over a sharded training run.  The
 * stand-alone decoder pass (rgcn_decoder_loss_backward_device) is replicated: same batch, same result on every rank;
 * inside rgcn_train_step_device / rgcn_train_step_minibatch_device on a context with a communicator the decoder is
 * DIVIDED by triples: rank g scores the slice [g ceil(N / world), ...) of the batch, and the partial loss, dL/dcodes
 * and dL/dW_relation are summed over the ranks (three all-reduces: [V,d], [R,d], one float). */
rgcn_status rgcn_optimizer_norm_partial(rgcn_ctx* ctx);
rgcn_status rgcn_optimizer_apply(rgcn_ctx* ctx);
/* One TensorflowOptimizer.update_from_batch (optimize.py:81-88) entirely on the device, asynchronous:
 * graph prep (or adoption of a prefetched one), encoder forward (train), decoder loss + gradients,
 * encoder backward, and -- if rgcn_optimizer_config was called -- clip + Adam.  On a sharded context (after
 * rgcn_comm_init) the same sequence with its exchanges on RCCL; every rank passes the same graph and batch. */
rgcn_status rgcn_train_step_device(rgcn_ctx* ctx, const int32_t* triples_dev, int64_t num_edges,
                                   const int32_t* x_dev, const float* y_dev, int64_t num_triples,
                                   uint64_t dropout_seed, float regularization_parameter);

/* The reference's t_func after the neighbourhood sampling + update_from_batch (code/train.py:227-245,
 * optimize.py:81-88) in ONE asynchronous call on a graph batch that is resident in HBM: edge dropout (exact `keep`
 * of the n batch edges -> message graph, as rgcn_set_graph_dropout_device with edge_seed), negative sampling
 * (rgcn_negative_sample_device -- under rgcn_set_exclusive_negatives its exclusive form, under rgcn_set_typed_negatives
 * rgcn_negative_sample_typed_device -- on ALL n batch edges -> x_scratch_dev int32 [n*(rate+1),3], y_scratch_dev float
 * [n*(rate+1)]), under rgcn_set_relation_negatives(m) n*m relation rows behind them and n*(rate+1+m) rows in all), then the train step of rgcn_train_step_device.  Only the n batch triples cross PCIe per step. */
rgcn_status rgcn_train_step_minibatch_device(rgcn_ctx* ctx, const int32_t* batch_dev, int64_t num_edges, int64_t keep,
                                             uint64_t edge_seed, int32_t negative_rate, uint64_t negative_seed,
                                             int32_t* x_scratch_dev, float* y_scratch_dev, uint64_t dropout_seed,
                                             float regularization_parameter);

/* Software pipelining across steps: prepare the graph structures of the NEXT minibatch (same work as
 * rgcn_set_graph_device) on a side stream into a second buffer set while the step already queued
 * keeps running.  A later rgcn_step_device with the same (pointer, num_edges) adopts them instead of
 * rebuilding.  Call it AFTER queueing the current step.  The reference has no counterpart: its graph
 * arrives through feed_dict at session.run (optimize.py:81-88).
 * Contract: the triple buffer must not change between this call and the step that adopts the preparation.
 * Writing it through rgcn_copy_to_device* or freeing it through rgcn_device_free drops the preparation (the
 * step then rebuilds in line); writes the library cannot see (the caller's own kernels / copies) are the
 * caller's responsibility -- call rgcn_prefetch_graph_device again after them. */
rgcn_status rgcn_prefetch_graph_device(rgcn_ctx* ctx, const int32_t* triples_dev_next, int64_t num_edges);
/* the same for a step that draws its graph by edge dropout: adopted by rgcn_train_step_minibatch_device called with
 * the same (batch pointer, num_edges, keep, edge seed) */
rgcn_status rgcn_prefetch_graph_dropout_device(rgcn_ctx* ctx, const int32_t* batch_dev_next, int64_t num_edges,
                                               int64_t keep, uint64_t edge_seed);

/* ---- hipGraph capture of whole steps (BASELINE config 5: "hipGraph-captured train step") -------------
 * Between rgcn_capture_begin and rgcn_capture_end every asynchronous device call on the context
 * (rgcn_step_device, rgcn_train_step_device, rgcn_prefetch_graph_device, rgcn_set_graph_device + rgcn_forward +
 * rgcn_backward_device ...) is recorded into a hipGraph instead of being executed, side streams included;
 * rgcn_graph_launch replays it on the context's stream with one launch.  Shapes and device pointers are the
 * captured ones (static shapes: refresh the CONTENTS of the triple / batch buffers between launches); every random
 * draw differs from replay to replay -- a device counter offsets the captured seeds: replay k of a graph draws the
 * dropout masks, the edge-dropout subset and the negative samples of (captured seed + k) -- and Adam's step count
 * advances on the device.  Calls that synchronise or touch host memory return RGCN_ERR_STATE during a capture;
 * run one ordinary step first so that every lazily allocated buffer exists.  To keep the graph preparation of
 * the next minibatch overlapped inside a graph, capture an even number of steps, each followed by the prefetch
 * of the other triple buffer, with the first buffer prefetched (and finished) before the capture begins. */
rgcn_status rgcn_capture_begin(rgcn_ctx* ctx);
rgcn_status rgcn_capture_end(rgcn_ctx* ctx, int32_t* graph_id);
rgcn_status rgcn_graph_launch(rgcn_ctx* ctx, int32_t graph_id);
rgcn_status rgcn_graph_destroy(rgcn_ctx* ctx, int32_t graph_id);

/* ---- relation sharding across GPUs (new: the reference is single-device) ------------
 * owner[r] in [0, world) assigns relation r's edges and W_f[r]/W_b[r] (BLOCK) or C_f[r]/C_b[r]
 * (BASIS) to one rank.  Degrees stay global.  Must be identical on all ranks. */
rgcn_status rgcn_set_relation_owner(rgcn_ctx* ctx, const int32_t* owner, int32_t count);
/* RCCL bootstrap: rank 0 makes the id, the launcher broadcasts the 128 bytes, every rank inits.
 * librccl.so.1 is dlopen'ed on first use; a world==1 context never touches it. */
rgcn_status rgcn_comm_unique_id(uint8_t id[128]);
rgcn_status rgcn_comm_init(rgcn_ctx* ctx, const uint8_t id[128]);
/* sum-all-reduce of `count` floats at a device pointer on the context's stream (used by bench.py
 * for its barrier / max-over-ranks reduction so that no second RCCL client is needed). */
rgcn_status rgcn_comm_allreduce_sum(rgcn_ctx* ctx, float* dev, int64_t count);
/* What the collective library itself reports about the context's communicator (ncclCommCount / ncclCommUserRank /
 * ncclCommCuDevice): how many ranks it SEES, this rank's index, the device it is bound to -- the answer to "did RCCL
 * come up with N ranks" from inside a run (bench.py prints it as "rccl_ranks").  -1 where there is no communicator
 * (world == 1 / before rgcn_comm_init) or the bound library lacks the entry point. */
rgcn_status rgcn_comm_info(rgcn_ctx* ctx, int32_t* comm_ranks, int32_t* comm_rank, int32_t* comm_device);
/* Context-free: how many HIP devices this process sees (0 without a GPU) and, for 0 <= device < count, the PCI address
 * of that device as domain << 16 | bus << 8 | device (-1 otherwise).  A launcher that masks the visible devices per
 * rank (HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES) makes every rank's GPU "device 0": bench.py --gpus N picks its
 * device by this count and compares PCI addresses, not indices, when it checks that no two ranks share a GPU. */
rgcn_status rgcn_device_info(int32_t device, int32_t* count, int64_t* pci_address);

/* Phase API: the same forward/backward cut at the points where a sharded run exchanges data.
 * rgcn_forward == begin; for l: partial(l) [all-reduce EXCHANGE] finish(l).
 * rgcn_backward == begin; for l=L..1: partial(l) [all-reduce EXCHANGE, DSELF_EXCHANGE] finish(l); end.
 * With world > 1 and no communicator the caller performs the exchange itself through
 * rgcn_read_buffer / rgcn_write_buffer (single-GPU test double for the collective). */
rgcn_status rgcn_forward_begin(rgcn_ctx* ctx, int32_t train, uint64_t dropout_seed,
                               const uint8_t* dropout_masks_host);
rgcn_status rgcn_forward_layer_partial(rgcn_ctx* ctx, int32_t layer);
rgcn_status rgcn_forward_layer_finish(rgcn_ctx* ctx, int32_t layer);
rgcn_status rgcn_backward_begin(rgcn_ctx* ctx, const float* dcodes_dev);
rgcn_status rgcn_backward_layer_partial(rgcn_ctx* ctx, int32_t layer);
rgcn_status rgcn_backward_layer_finish(rgcn_ctx* ctx, int32_t layer);
rgcn_status rgcn_backward_end(rgcn_ctx* ctx);
rgcn_status rgcn_read_buffer(rgcn_ctx* ctx, int32_t which, void* host, int64_t bytes);
rgcn_status rgcn_write_buffer(rgcn_ctx* ctx, int32_t which, const void* host, int64_t bytes);

/* ---- device memory + timing helpers (so callers need no other GPU runtime) -------------------- */
rgcn_status rgcn_device_alloc(rgcn_ctx* ctx, int64_t bytes, void** dev);
rgcn_status rgcn_device_free(rgcn_ctx* ctx, void* dev);
rgcn_status rgcn_copy_to_device(rgcn_ctx* ctx, void* dev, const void* host, int64_t bytes);
/* As rgcn_copy_to_device, but the host does not wait for the transfer: the data is copied to a pinned staging
 * slot during the call (the caller's memory is free again on return) and the transfer is ordered on the
 * context's main stream, or -- on_prefetch_stream != 0 -- on the stream rgcn_prefetch_graph_device works on, so
 * that "upload the next minibatch's triples, then prepare its graph" runs beside the current step (the training
 * driver's double-buffered feed; the reference re-feeds numpy arrays through feed_dict on every session.run,
 * optimize.py:81-88).  Transfers above 1 MB fall back to waiting. */
rgcn_status rgcn_copy_to_device_async(rgcn_ctx* ctx, void* dev, const void* host, int64_t bytes,
                                      int32_t on_prefetch_stream);
rgcn_status rgcn_copy_to_host(rgcn_ctx* ctx, void* host, const void* dev, int64_t bytes);
/* HIP-event stopwatch on the context's stream (torch.cuda.Event cannot see this stream). */
rgcn_status rgcn_timer_start(rgcn_ctx* ctx);
rgcn_status rgcn_timer_stop(rgcn_ctx* ctx, float* elapsed_ms); /* synchronises */

/* Side-stream overlap on/off (default on).  With overlap off every kernel runs alone on the main stream: per-kernel
 * durations are exclusive.  (The product library reads NO tuning variable from the environment: its configuration is
 * what these setters say; experiment knobs exist in librgcn_devtools.so only, include/rgcn_devtools.h.) */
rgcn_status rgcn_set_overlap(rgcn_ctx* ctx, int32_t on);

/* Form of the block-diagonal layer (ConcatGcn.compute_messages + combine_messages, gcn_basis_concat.py:35-83, and
 * their gradient).  Both give bitwise the same activations and gradients -- with one exception, the embedding bias
 * gradient db_emb, which form 1 sums from the per-workgroup column partials of its row-gradient kernel (within 2e-6 of
 * scale of form 0's separate column-sum pass, bit-identical from engine to engine) --
 * tests/test_gpu_parity.py::test_single_pass_layer_equals_the_two_kernel_form.
 *   1 : (default) destination-major banded single pass (csrc/block_rows.hip): ONE kernel per layer and direction walks
 *       the incidence CSR -- a 16-lane group per (row, column band), one band per XCD, the relation's sd x sd blocks
 *       read through L2 from a band-tiled copy of the weights, rows taken by descending length, long rows by whole
 *       workgroups through LDS tiles -- and applies self-loop term, dropout and relu / relu'; no message buffer.
 *       39 / 46 us per layer forward / backward against 57 / 74 for form 0 at FB15k-237 minibatch size, half the time
 *       at the 272,115-edge training graph (profiles/r04_rowmajor_spmm_ab.md).  On relation-sharded contexts
 *       (world > 1) it walks the rank's own messages and writes the partial pre-activations for the exchange.
 *   0 : relation-major message kernel -> [2E,d] message buffer -> row-major reduce (k_combine): the reference form the
 *       other is held equal to, and what runs when the block count exceeds form 1's lane groups.
 * (Rounds 2-3 built two more forms -- the reduce as the self-loop GEMM's epilogue, per-block workgroups with an LDS
 * weight table --, measured them slower and removed them in round 5: profiles/r02_fused_layer_ab.log,
 * profiles/r03_block_spmm_ab.md.)  The basis kind runs its own kernels whatever the setting. */
rgcn_status rgcn_set_fusion(rgcn_ctx* ctx, int32_t mode);

/* Arithmetic of the dense contractions (self-loop and basis GEMMs); all of them take and return fp32.
 *   6 : (default) every fp32 operand is split exactly into three bf16 numbers hi + mid + lo (round to
 *       nearest + exact residual, twice) and the product is accumulated in fp32 from 6 of the 9 partial
 *       products on the bf16 matrix cores (v_mfma_f32_32x32x16_bf16); the three dropped ones (mid*lo,
 *       lo*mid, lo*lo) are below 2^-26 of |a||b| per product, a quarter of one fp32 rounding.  Measured
 *       error against float64 equals the fp32-MFMA path's (tests/test_gpu_parity.py::test_gemm_modes).
 *   9 : all 9 partial products - the products of exact fp32 arithmetic in another summation order
 *   0 : fp32 MFMA (v_mfma_f32_32x32x2_f32), 1/16 of the bf16 rate on gfx950
 *   3 : hi*hi, hi*mid, mid*hi only (about 2^-17; NOT fp32 - experiments only) */
rgcn_status rgcn_set_gemm_mode(rgcn_ctx* ctx, int32_t mode);

/* Per-kernel profile: when enabled every launch is bracketed by HIP events on the context's stream.
 * Records aggregate by kernel name, summed over calls.  alg_bytes = the DESIGN bytes of the launches (what the
 * kernel asks of the memory system by construction: a gathered row counts once per use, staging slabs count);
 * alg_flops = the algorithmic flops; rgcn_profile_get_compulsory = the COMPULSORY bytes (every distinct input byte
 * once + every output byte once) -- the figure roofline fractions are computed on.
 * The reference has no counterpart (TF's timeline is not used by code/train.py). */
rgcn_status rgcn_profile_enable(rgcn_ctx* ctx, int32_t on);
rgcn_status rgcn_profile_reset(rgcn_ctx* ctx);
int32_t     rgcn_profile_count(rgcn_ctx* ctx); /* synchronises, aggregates; number of kernel names */
rgcn_status rgcn_profile_get(rgcn_ctx* ctx, int32_t i, char* name, int32_t name_cap, int64_t* calls,
                             double* total_ms, double* alg_bytes, double* alg_flops);
rgcn_status rgcn_profile_get_compulsory(rgcn_ctx* ctx, int32_t i, double* compulsory_bytes);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* RGCN_H_ */
