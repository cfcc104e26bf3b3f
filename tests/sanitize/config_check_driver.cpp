// Driver of the configuration check (csrc/config_check.h: pure host C++, nothing from HIP) for tests/test_config_check.py,
// built with AddressSanitizer / UndefinedBehaviorSanitizer like gemm_plan_driver.cpp.  One line per named configuration:
// `name: status|message` as check_config() answers; the test holds the expected lines as literals.
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../../relationprediction_amd/csrc/config_check.h"

using namespace rgcn;

// the parity tests' small shape: accepted as it stands for every kind but the embedding one (base(RGCN_KIND_EMBEDDING, 1, 0))
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
static rgcn_config block() { return base(RGCN_KIND_BLOCK, 4); }
static rgcn_config basis() { return base(RGCN_KIND_BASIS, 2); }
static rgcn_config tdiag() { return base(RGCN_KIND_BASIS_TDIAG, 2); }
static rgcn_config pdiag() { return base(RGCN_KIND_BASIS_PDIAG, 2); }
static rgcn_config embedding() { return base(RGCN_KIND_EMBEDDING, 1, 0); }

static void show(const char* name, const rgcn_config& f, bool highway = false) {
  const ConfigVerdict v = check_config(f, highway);
  std::printf("%s: %d|%s\n", name, (int)v.status, v.message.c_str());
}

// one field changed
template <class T, class U>
static rgcn_config with(rgcn_config f, T rgcn_config::*field, U value) {
  f.*field = (T)value;
  return f;
}
static rgcn_config sharded(rgcn_config f, int world = 2, int rank = 1) {
  f.world = world;
  f.rank = rank;
  return f;
}
static rgcn_config onehot(rgcn_config f) { return with(f, &rgcn_config::input_mode, RGCN_INPUT_ONEHOT); }
static rgcn_config shape(rgcn_config f, int64_t V, int bases, int d) {
  f.num_entities = (int32_t)V;
  f.num_bases = bases;
  f.dim = d;
  return f;
}

int main() {
  // accepted: one per kind and option
  show("ok_block", block());
  show("ok_basis", basis());
  show("ok_basis_onehot", onehot(basis()));
  show("ok_block_highway", block(), true);
  show("ok_basis_highway", basis(), true);
  show("ok_tdiag", tdiag());
  show("ok_pdiag", pdiag());
  show("ok_embedding", embedding());
  show("ok_block_sharded", sharded(block()));
  show("ok_basis_local_norm", with(basis(), &rgcn_config::norm_mode, RGCN_NORM_LOCAL));

  // each refusal from a configuration that breaks that rule alone, in check_config's order
  show("abi", with(block(), &rgcn_config::abi_version, RGCN_ABI_VERSION + 1));
  show("zero_entities", with(block(), &rgcn_config::num_entities, 0));
  show("zero_relations", with(block(), &rgcn_config::num_relations, 0));
  show("zero_dim", with(block(), &rgcn_config::dim, 0));
  show("zero_layers", with(block(), &rgcn_config::num_layers, 0));
  show("zero_bases", with(basis(), &rgcn_config::num_bases, 0));
  show("embedding_with_a_layer", with(embedding(), &rgcn_config::num_layers, 1));
  show("embedding_two_bases", with(embedding(), &rgcn_config::num_bases, 2));
  show("keep_0", with(block(), &rgcn_config::keep_prob, 0.0f));
  show("keep_1", with(block(), &rgcn_config::keep_prob, 1.0f));
  show("keep_above_1", with(block(), &rgcn_config::keep_prob, std::nextafter(1.0f, 2.0f)));
  show("keep_negative", with(block(), &rgcn_config::keep_prob, -0.5f));
  show("kind_5", with(block(), &rgcn_config::kind, 5));
  show("kind_negative", with(block(), &rgcn_config::kind, -1));
  show("norm_negative", with(block(), &rgcn_config::norm_mode, -1));
  show("norm_4", with(block(), &rgcn_config::norm_mode, RGCN_NORM_LOCAL + 1));
  show("world_0", sharded(block(), 0, 0));
  show("rank_negative", sharded(block(), 2, -1));
  show("rank_is_world", sharded(block(), 2, 2));
  show("rank_0_of_2", sharded(block(), 2, 0));
  show("edges_negative", with(block(), &rgcn_config::max_edges, -1));
  show("edges_500m", with(block(), &rgcn_config::max_edges, (int64_t)500 * 1000 * 1000));
  show("edges_500m_and_1", with(block(), &rgcn_config::max_edges, (int64_t)500 * 1000 * 1000 + 1));
  show("input_mode_2", with(block(), &rgcn_config::input_mode, 2));
  show("embedding_sharded", sharded(embedding()));
  show("embedding_onehot", onehot(embedding()));
  show("embedding_highway", embedding(), true);
  show("tdiag_sharded", sharded(tdiag()));
  show("tdiag_onehot", onehot(tdiag()));
  show("tdiag_highway", tdiag(), true);
  show("tdiag_64_bases", with(tdiag(), &rgcn_config::num_bases, 64));
  show("tdiag_65_bases", with(tdiag(), &rgcn_config::num_bases, 65));
  show("tdiag_below_2_31", shape(tdiag(), ((int64_t)1 << 20) - 1, 32, 32));      // 2 V B d = 2^31 - 2048
  show("tdiag_at_2_31", shape(tdiag(), (int64_t)1 << 20, 32, 32));
  show("pdiag_sharded", sharded(pdiag()));
  show("pdiag_onehot", onehot(pdiag()));
  show("pdiag_highway", pdiag(), true);
  show("pdiag_64_bases", with(pdiag(), &rgcn_config::num_bases, 64));
  show("pdiag_65_bases", with(pdiag(), &rgcn_config::num_bases, 65));
  show("pdiag_below_2_31", shape(pdiag(), ((int64_t)1 << 20) - 1, 32, 32));
  show("pdiag_at_2_31", shape(pdiag(), (int64_t)1 << 20, 32, 32));
  show("onehot_block", onehot(block()));
  show("onehot_sharded", sharded(onehot(basis())));
  show("onehot_below_2_31", shape(onehot(basis()), ((int64_t)1 << 21) - 1, 32, 32));      // V B d = 2^31 - 1024
  show("onehot_at_2_31", shape(onehot(basis()), (int64_t)1 << 21, 32, 32));
  show("highway_sharded", sharded(block()), true);
  show("highway_onehot", onehot(basis()), true);
  show("entities_2_24_less_1", with(block(), &rgcn_config::num_entities, (1 << 24) - 1));
  show("entities_2_24", with(block(), &rgcn_config::num_entities, 1 << 24));
  show("relations_2_23_less_1", with(block(), &rgcn_config::num_relations, (1 << 23) - 1));
  show("relations_2_23", with(block(), &rgcn_config::num_relations, 1 << 23));
  show("rows_times_dim_2_31", shape(basis(), (int64_t)1 << 23, 2, 256));
  show("rows_times_dim_above_2_31", shape(basis(), (int64_t)1 << 23, 2, 257));
  show("messages_times_dim_below_2_40", with(with(basis(), &rgcn_config::max_edges, (int64_t)500 * 1000 * 1000), &rgcn_config::dim, 1099));
  show("messages_times_dim_above_2_40", with(with(basis(), &rgcn_config::max_edges, (int64_t)500 * 1000 * 1000), &rgcn_config::dim, 1100));
  show("block_3_of_20", with(block(), &rgcn_config::num_bases, 3));
  show("blocks_512", shape(block(), 150, 512, 512));
  show("blocks_513", shape(block(), 150, 513, 513));
  show("block_size_1", shape(block(), 150, 4, 4));
  show("block_size_2", shape(block(), 150, 4, 8));
  show("block_size_3", shape(block(), 150, 4, 12));
  show("block_size_4", shape(block(), 150, 4, 16));
  show("block_size_5", shape(block(), 150, 4, 20));
  show("block_size_6", shape(block(), 150, 4, 24));
  show("block_size_7", shape(block(), 150, 4, 28));
  show("block_size_8", shape(block(), 150, 4, 32));
  show("block_size_9", shape(block(), 150, 4, 36));
  show("basis_64_bases", with(basis(), &rgcn_config::num_bases, 64));
  show("basis_65_bases", with(basis(), &rgcn_config::num_bases, 65));
  show("basis_onehot_65_bases", with(onehot(basis()), &rgcn_config::num_bases, 65));

  // two rules broken at once: the earlier one answers
  show("both_abi_and_zero_entities", with(with(block(), &rgcn_config::abi_version, 0), &rgcn_config::num_entities, 0));
  show("both_embedding_layers_and_highway", with(embedding(), &rgcn_config::num_layers, 2), true);
  show("both_keep_0_and_entities_2_24", with(with(block(), &rgcn_config::keep_prob, 0.0f), &rgcn_config::num_entities, 1 << 24));
  show("both_unknown_kind_and_norm", with(with(block(), &rgcn_config::kind, 7), &rgcn_config::norm_mode, 9));
  show("both_tdiag_sharded_and_onehot", sharded(onehot(tdiag())));
  show("both_tdiag_65_bases_and_2_31", shape(tdiag(), (int64_t)1 << 20, 65, 32));
  show("both_pdiag_highway_and_65_bases", with(pdiag(), &rgcn_config::num_bases, 65), true);
  show("both_onehot_block_and_highway", onehot(block()), true);
  show("all_highway_onehot_sharded", sharded(onehot(basis())), true);
  show("both_blocks_513_and_indivisible", shape(block(), 150, 513, 514));
  show("both_blocks_513_and_block_size_6", shape(block(), 150, 513, 3078));
  std::printf("config_check_driver: ok\n");
  return 0;
}
