// Driver of the output transform's configuration rules (csrc/config_check.h check_output_transform: pure host C++, nothing
// from HIP) for tests/test_output_transform_config.py, built with AddressSanitizer / UndefinedBehaviorSanitizer like
// config_check_driver.cpp.  One line per named configuration: `name: status|message` as rgcn_create_ex answers -- check_config
// first, check_output_transform where that accepts; the test holds the expected lines as literals.
#include <cstdint>
#include <cstdio>

#include "../../relationprediction_amd/csrc/config_check.h"

using namespace rgcn;

// config_check_driver.cpp's small shape
static rgcn_config base(int kind, int num_bases, int num_layers = 2) {
  rgcn_config f{};
  f.abi_version = RGCN_ABI_VERSION;
  f.device = 0;
  f.num_entities = 150;
  f.num_relations = 9;
  f.dim = 20;
  f.num_layers = num_layers;
  f.kind = kind;
  f.num_bases = num_bases;
  f.keep_prob = 0.8f;
  f.norm_mode = RGCN_NORM_INTENDED;
  f.max_edges = 800;
  f.rank = 0;
  f.world = 1;
  f.input_mode = RGCN_INPUT_EMBEDDING;
  return f;
}
static rgcn_config entities(rgcn_config f, int32_t V) {
  f.num_entities = V;
  return f;
}
static rgcn_config sharded(rgcn_config f) {
  f.world = 2;
  f.rank = 1;
  return f;
}
static rgcn_config onehot(rgcn_config f) {
  f.input_mode = RGCN_INPUT_ONEHOT;
  return f;
}

static void show(const char* name, const rgcn_config& f, int32_t code_dim, bool highway = false) {
  ConfigVerdict v = check_config(f, highway);
  if (v.status == RGCN_OK) v = check_output_transform(f, highway, code_dim);
  std::printf("%s: %d|%s\n", name, (int)v.status, v.message.c_str());
}

int main() {
  const rgcn_config block = base(RGCN_KIND_BLOCK, 4), basis = base(RGCN_KIND_BASIS, 2);
  const rgcn_config tdiag = base(RGCN_KIND_BASIS_TDIAG, 2), pdiag = base(RGCN_KIND_BASIS_PDIAG, 2);
  const rgcn_config embedding = base(RGCN_KIND_EMBEDDING, 1, 0);
  // accepted: every kind that has layers, narrower, wider and as wide as the encoder
  show("ok_block", block, 8);
  show("ok_basis", basis, 8);
  show("ok_tdiag", tdiag, 8);
  show("ok_pdiag", pdiag, 8);
  show("ok_basis_onehot", onehot(basis), 8);
  show("ok_block_highway", block, 8, true);
  show("ok_basis_highway", basis, 8, true);
  show("ok_wider", basis, 33);
  show("ok_equal_dimensions", basis, 20);
  // no layer: whatever check_config accepts stays accepted
  show("none_block", block, 0);
  show("none_block_sharded", sharded(block), 0);
  show("none_embedding", embedding, 0);
  // refused
  show("negative", basis, -1);
  show("negative_on_embedding", embedding, -4);
  show("sharded_block", sharded(block), 8);
  show("sharded_basis", sharded(basis), 8);
  show("embedding_kind", embedding, 8);
  // EntityCount x CodeDimension against 2^31 (EntityCount itself stays below the sort-key limit 2^24)
  show("rows_times_code_dim_below_2_31", entities(basis, 1 << 23), 255);
  show("rows_times_code_dim_at_2_31", entities(basis, 1 << 23), 256);
  show("rows_times_code_dim_just_below_2_31", entities(basis, (1 << 23) - 1), 256);
  // two rules at once: check_config answers first; among the layer's own, the sign, then the kind, then the shard count
  show("both_unknown_kind_and_negative", base(7, 2), -1);
  show("both_highway_sharded_and_code_dim", sharded(block), 8, true);
  show("both_sharded_and_2_31", sharded(entities(basis, 1 << 23)), 256);
  std::printf("output_transform_config_driver: ok\n");
  return 0;
}
