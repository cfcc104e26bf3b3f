// check_config: every configuration rgcn_create refuses before it touches the device, in the order rgcn_create has always
// refused them -- where a configuration breaks several rules, the first rule below decides the status and the message.
// Pure host arithmetic on rgcn_config: depends on include/rgcn.h and the standard library only, no HIP and no rgcn_ctx
// (tests/sanitize/config_check_driver.cpp prints its answers, tests/test_config_check.py holds them as literals).
#pragma once

#include <cstdint>
#include <string>

#include "../../include/rgcn.h"

namespace rgcn {

struct ConfigVerdict {
  rgcn_status status;
  std::string message;      // empty when status is RGCN_OK
};

inline ConfigVerdict refuse(rgcn_status s, const std::string& m) { return ConfigVerdict{s, m}; }

// BasisGcnTimesDiag (basis_tdiag.hip) and BasisGcnWithDiag (basis_pdiag.hip): one GPU, embedding input, no highway layers
struct DiagKind {
  const char* name;           // the kind as the messages spell it
  const char* tag;            // ... and as the basis-count refusal does
  const char* why_one_gpu;    // what has no exchange points
  const char* why_no_onehot;  // the state of the kind's one-hot first layer
};
inline ConfigVerdict check_diag_kind(const rgcn_config& f, bool onehot, bool highway, const DiagKind& k) {
  const std::string name = k.name;
  if (f.world > 1) return refuse(RGCN_ERR_UNSUPPORTED, name + " on a sharded context (" + k.why_one_gpu + ")");
  if (onehot) return refuse(RGCN_ERR_UNSUPPORTED, name + " with RGCN_INPUT_ONEHOT (" + k.why_no_onehot + ")");
  if (highway) return refuse(RGCN_ERR_UNSUPPORTED, name + " with RGCN_SKIP_HIGHWAY (not built)");
  if (f.num_bases > 64) return refuse(RGCN_ERR_UNSUPPORTED, std::string("NumberOfBasisFunctions > 64 (") + k.tag + ")");
  if (2 * (int64_t)f.num_entities * f.num_bases * (int64_t)f.dim >= ((int64_t)1 << 31))
    return refuse(RGCN_ERR_UNSUPPORTED, name + ": 2 x EntityCount x NumberOfBasisFunctions x dimension must be below 2^31");
  return ConfigVerdict{RGCN_OK, ""};
}

// highway: rgcn_config_ext::skip_mode == RGCN_SKIP_HIGHWAY
inline ConfigVerdict check_config(const rgcn_config& f, bool highway) {
  if (f.abi_version != RGCN_ABI_VERSION) return refuse(RGCN_ERR_INVALID, "abi_version mismatch");
  const bool emb = f.kind == RGCN_KIND_EMBEDDING;
  if (f.num_entities <= 0 || f.num_relations <= 0 || f.dim <= 0 || (!emb && f.num_layers <= 0) || f.num_bases <= 0)
    return refuse(RGCN_ERR_INVALID, "EntityCount, RelationCount, dimension, NumberOfLayers and "
                                    "NumberOfBasisFunctions must be positive");
  if (emb && (f.num_layers != 0 || f.num_bases != 1))
    return refuse(RGCN_ERR_INVALID, "RGCN_KIND_EMBEDDING has no layers: num_layers must be 0 and num_bases 1");
  if (!(f.keep_prob > 0.0f && f.keep_prob <= 1.0f)) return refuse(RGCN_ERR_INVALID, "DropoutKeepProbability must be in (0,1]");
  if (f.kind != RGCN_KIND_BLOCK && f.kind != RGCN_KIND_BASIS && f.kind != RGCN_KIND_BASIS_TDIAG &&
      f.kind != RGCN_KIND_BASIS_PDIAG && !emb)
    return refuse(RGCN_ERR_INVALID, "unknown kind");
  if (f.norm_mode < 0 || f.norm_mode > RGCN_NORM_LOCAL) return refuse(RGCN_ERR_INVALID, "unknown norm_mode");
  if (f.world < 1 || f.rank < 0 || f.rank >= f.world) return refuse(RGCN_ERR_INVALID, "need 0 <= rank < world");
  if (f.max_edges < 0 || f.max_edges > (int64_t)500 * 1000 * 1000) return refuse(RGCN_ERR_INVALID, "max_edges out of range");
  if (f.input_mode != RGCN_INPUT_EMBEDDING && f.input_mode != RGCN_INPUT_ONEHOT)
    return refuse(RGCN_ERR_INVALID, "unknown input_mode (0: embedding input, 1: RGCN_INPUT_ONEHOT)");
  const bool onehot = f.input_mode == RGCN_INPUT_ONEHOT;
  if (emb) {
    // the Name=embedding encoder (model_builder.py:27-41): one GPU, no input-mode or skip variants
    if (f.world > 1) return refuse(RGCN_ERR_UNSUPPORTED, "RGCN_KIND_EMBEDDING on a sharded context (nothing to shard by relation)");
    if (onehot) return refuse(RGCN_ERR_UNSUPPORTED, "RGCN_KIND_EMBEDDING with RGCN_INPUT_ONEHOT (there is no first layer)");
    if (highway) return refuse(RGCN_ERR_UNSUPPORTED, "RGCN_KIND_EMBEDDING with RGCN_SKIP_HIGHWAY (there is no layer to skip)");
  }
  if (f.kind == RGCN_KIND_BASIS_TDIAG || f.kind == RGCN_KIND_BASIS_PDIAG) {
    static const DiagKind tdiag{
        "RGCN_KIND_BASIS_TDIAG", "basis_tdiag", "the products P, dP and the coefficient table have no exchange points",
        "the reference's one-hot branch of BasisGcnTimesDiag exists, gcn_basis_times_diag.py:21,70,76: not built"};
    static const DiagKind pdiag{
        "RGCN_KIND_BASIS_PDIAG", "basis_pdiag",
        "the mixing table, the diagonal aggregate and the diagonal tables' gradient have no exchange points",
        "the one-hot first layer of BasisGcnWithDiag is not built"};
    const ConfigVerdict v = check_diag_kind(f, onehot, highway, f.kind == RGCN_KIND_BASIS_TDIAG ? tdiag : pdiag);
    if (v.status != RGCN_OK) return v;
  }
  if (onehot) {
    // the featureless first layer (model_builder.py:277-283): BasisGcn only, per-entity tables on one GPU
    if (f.kind != RGCN_KIND_BASIS)
      return refuse(RGCN_ERR_UNSUPPORTED, "RGCN_INPUT_ONEHOT with the block kind: the reference's one-hot branch of ConcatGcn "
                                          "cannot execute (gcn_basis_concat.py:18-19,42-46)");
    if (f.world > 1)
      return refuse(RGCN_ERR_UNSUPPORTED, "RGCN_INPUT_ONEHOT on a sharded context (the [V,B,d] tables are not sharded)");
    if ((int64_t)f.num_entities * f.num_bases * (int64_t)f.dim >= ((int64_t)1 << 31))
      return refuse(RGCN_ERR_UNSUPPORTED, "RGCN_INPUT_ONEHOT: EntityCount x NumberOfBasisFunctions x dimension must be below 2^31");
  }
  if (highway) {
    if (f.world > 1)
      return refuse(RGCN_ERR_UNSUPPORTED, "RGCN_SKIP_HIGHWAY on a sharded context (the highway passes have no exchange points)");
    if (onehot)
      return refuse(RGCN_ERR_UNSUPPORTED, "RGCN_SKIP_HIGHWAY with RGCN_INPUT_ONEHOT (in the reference the one-hot first layer "
                                          "gets no highway layer while the layers above it do: not built)");
  }
  // the library's radix sort takes keys below 2^24 (csr_sort.hip): vertex ids and directed-relation ids
  if (f.num_entities >= (1 << 24) || 2 * (int64_t)f.num_relations >= (1 << 24))
    return refuse(RGCN_ERR_UNSUPPORTED, "EntityCount and 2 x RelationCount must be below 2^24 (sort key range of this build)");
  if ((int64_t)f.num_entities * f.dim > (int64_t)1 << 31 || 2 * f.max_edges * (int64_t)f.dim > ((int64_t)1 << 40))
    return refuse(RGCN_ERR_UNSUPPORTED, "problem too large for this build");
  if (f.kind == RGCN_KIND_BLOCK) {
    if (f.dim % f.num_bases != 0)
      return refuse(RGCN_ERR_INVALID, "InternalEncoderDimension must be divisible by NumberOfBasisFunctions "
                                      "(the reference silently mis-groups otherwise: gcn_basis_concat.py:15,42)");
    // what the block kernels are compiled for (block_msgs.hip, block_rows.hip)
    if (f.num_bases > 512) return refuse(RGCN_ERR_UNSUPPORTED, "NumberOfBasisFunctions (block count) > 512");
    const int sd = f.dim / f.num_bases;
    if (!(sd == 1 || sd == 2 || sd == 3 || sd == 4 || sd == 5 || sd == 8))
      return refuse(RGCN_ERR_UNSUPPORTED, "block size d/nb must be one of 1,2,3,4,5,8");
  } else if (f.num_bases > 64) {
    return refuse(RGCN_ERR_UNSUPPORTED, "NumberOfBasisFunctions > 64 (basis)");
  }
  return ConfigVerdict{RGCN_OK, ""};
}

// The output transform (rgcn_config_ext::code_dim; 0: no such layer): what rgcn_create_ex refuses of it, asked AFTER
// check_config has accepted the configuration -- whatever breaks a rule above is refused for that rule first
// (tests/sanitize/output_transform_config_driver.cpp prints the answers, tests/test_output_transform_config.py holds them).
inline ConfigVerdict check_output_transform(const rgcn_config& f, bool highway, int32_t code_dim) {
  (void)highway;      // (the layer sits above H_L whatever wraps the layers: a highway context takes it like any other)
  if (code_dim < 0) return refuse(RGCN_ERR_INVALID, "code_dim must be 0 (no output transform) or the positive CodeDimension");
  if (code_dim == 0) return ConfigVerdict{RGCN_OK, ""};
  if (f.kind == RGCN_KIND_EMBEDDING)
    return refuse(RGCN_ERR_UNSUPPORTED, "code_dim > 0 with RGCN_KIND_EMBEDDING (the reference's embedding encoder has no "
                                        "output transform, model_builder.py:27-41)");
  if (f.world > 1)
    return refuse(RGCN_ERR_UNSUPPORTED, "code_dim > 0 on a sharded context (the gradient of W_out has no exchange point)");
  if ((int64_t)f.num_entities * (int64_t)code_dim >= ((int64_t)1 << 31))
    return refuse(RGCN_ERR_UNSUPPORTED, "code_dim > 0: EntityCount x CodeDimension must be below 2^31");
  return ConfigVerdict{RGCN_OK, ""};
}

}  // namespace rgcn
