// Internal declarations shared by the translation units of librgcn.so.
// Nothing here is part of the C ABI (include/rgcn.h is).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rgcn.h"
#include "counter_rng.h"
#include "dev_pool.h"
#include "gemm_plan.h"
#include "negative_exclusive.h"
#include "entity_softmax_plan.h"
#include "relation_softmax_plan.h"

namespace rgcn {

// Experiment knobs exist in the devtools build only (librgcn_devtools.so, -DRGCN_DEVTOOLS: tools/ and a few tests); the
// product library reads no tuning variable from the environment and runs ONE configuration, the default.
#ifdef RGCN_DEVTOOLS
inline int knob(const char* name, int dflt) {
  const char* s = getenv(name);
  return s ? atoi(s) : dflt;
}
#else
constexpr int knob(const char*, int dflt) { return dflt; }
#endif

// ---------------------------------------------------------------- error plumbing
void set_global_error(const std::string& s);

#define RGCN_HIP(ctx, expr)                                                                      \
  do {                                                                                           \
    hipError_t _e = (expr);                                                                      \
    if (_e != hipSuccess) {                                                                      \
      (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(_e) + " (" __FILE__ ":" +       \
                   std::to_string(__LINE__) + ")";                                               \
      return RGCN_ERR_HIP;                                                                       \
    }                                                                                            \
  } while (0)

#define RGCN_TRY(expr)                       \
  do {                                       \
    rgcn_status _s = (expr);                 \
    if (_s != RGCN_OK) return _s;            \
  } while (0)

#define RGCN_FAIL(ctx, code, msg)            \
  do {                                       \
    (ctx)->err = (msg);                      \
    return (code);                           \
  } while (0)

// ---------------------------------------------------------------- dropout generator
// Counter-based Bernoulli(keep) draw: nothing is stored, forward and backward re-derive the same
// bit from (seed, layer, flat element index).  Statistically equivalent to tf.nn.dropout's floor(keep + U[0,1))
// (message_gcn.py:64); the exact TF Philox stream is not reproducible (parity tests inject masks).
// drop_bits (splitmix64 per draw, 24 bits out) serves the negative sampler; the dropout masks use the two-stage form
// below since round 4: a 64-bit key per (seed, layer) from splitmix64 -- uniform over a launch -- and a 32-bit
// two-multiply hash per element keyed at both rounds (9 VALU operations instead of ~40: the per-element 64-bit
// multiplies were a third of the VALU work of the single-pass layer kernels); keep iff the top 24 bits < keep * 2^24.
// (splitmix64_mix and drop_bits themselves: counter_rng.h, which a plain C++ compiler reads too)
struct DropKey {
  uint32_t k0, k1;
};
__host__ __device__ inline DropKey drop_key_of(uint64_t seed, uint32_t layer) {
  const uint64_t z = splitmix64_mix(seed + 0x9E3779B97F4A7C15ull * (((uint64_t)layer << 44) + 1ull));
  return DropKey{(uint32_t)z, (uint32_t)(z >> 32)};
}
__host__ __device__ inline uint32_t drop_bits24(const DropKey& k, uint64_t idx) {
  const uint32_t hi = (uint32_t)(idx >> 32);
  uint32_t x = (uint32_t)idx ^ k.k0 ^ ((hi << 16) | (hi >> 16));
  x ^= x >> 16;
  x *= 0x7feb352du;
  x += k.k1;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x >> 8;
}

enum DropMode { DROP_NONE = 0, DROP_RNG = 1, DROP_MASK = 2 };

// Rows of the incidence CSR with more slots than this are pre-reduced by a whole workgroup
// (k_long_row_reduce) so that the one-wave-group-per-row combine never walks a hub serially.
constexpr int kLongRow = 32;
// Full-graph scale only (more than 65536 messages, block kind): a row with more than kGiantRow slots is cut into
// kGiantRow-slot pieces that separate workgroups sum; a finishing pass adds a row's pieces in piece order.
constexpr int kGiantRow = 2048;
constexpr int kAuxStreams = 3;

struct DropSpec {
  int32_t mode;         // DropMode
  uint32_t layer;       // 1..L
  uint32_t thresh;      // keep iff drop_bits < thresh
  float inv_keep;       // 1 / keep_prob
  uint64_t seed;
  const uint8_t* mask;  // [V,d] 0/1 for this layer (DROP_MASK)
  const uint64_t* seed_offset;  // device counter added to `seed` (replayed hipGraphs draw fresh masks); may be null
};

#if defined(__HIPCC__)
// the (seed, layer) key of a launch's dropout spec; derive it ONCE per thread, outside the element loops
__device__ __forceinline__ DropKey drop_key(const DropSpec& ds) {
  if (ds.mode != DROP_RNG) return DropKey{0u, 0u};
  return drop_key_of(ds.seed + (ds.seed_offset ? *ds.seed_offset : 0ull), ds.layer);
}
// dropout factor of flat element idx: 1/keep or 0 (1 when the spec is inactive)
__device__ __forceinline__ float drop_factor(const DropSpec& ds, const DropKey& key, size_t idx) {
  if (ds.mode == DROP_NONE) return 1.0f;
  if (ds.mode == DROP_RNG) return drop_bits24(key, idx) < ds.thresh ? ds.inv_keep : 0.0f;
  return ds.mask[idx] ? ds.inv_keep : 0.0f;
}
__device__ __forceinline__ float drop_factor(const DropSpec& ds, size_t idx) { return drop_factor(ds, drop_key(ds), idx); }
#endif

// ---------------------------------------------------------------- profiling records
struct ProfRec {
  const char* name;
  hipEvent_t e0, e1;
  double bytes, flops, cbytes;
};
struct ProfAgg {
  std::string name;
  int64_t calls;
  double ms, bytes, flops, cbytes;
};

// ---------------------------------------------------------------- parameters
enum ParamLayout {
  LAYOUT_PLAIN = 0,        // device layout == host layout
  LAYOUT_BLOCK_T = 1,      // host [R][nb][sd*sd]  <-> device [R][sd*sd][nb]
  LAYOUT_BASIS_T = 2       // host [d][B][d]       <-> device [B][d][d]
};

struct Param {
  std::string name;
  int32_t ndim;
  int64_t shape[4];
  int64_t count;
  float* val;    // device (view into a layer allocation for W_f/W_b)
  float* grad;   // device
  int32_t layout;
  bool no_grad = false;   // created but never used by the forward pass (the per-layer bias)
};

struct LayerBufs {
  // BLOCK: wrel = [2R][sd*sd][nb] (first R = W_forward, last R = W_backward), same for grel.
  // BASIS: wrel = [2][B][d][d]  (GEMM operand [2B*d, d]); coef = [2R][B] (first R = C_forward).
  // BASIS, layer 1 of a one-hot context: wrel = [2][V][B][d] (the host layout), wself = [V][d], no fragment tables.
  float* wrel = nullptr;
  float* grel = nullptr;
  float* coef = nullptr;
  float* gcoef = nullptr;
  float* wself = nullptr;   // [d,d]
  float* gwself = nullptr;
  float* bias = nullptr;    // [d], unused by the math
  float* gbias = nullptr;
  // MFMA-fragment tables of the weights that are the B operand of a contraction (gemm_presplit_b: the three bf16 planes of
  // the exact split, in fragment order), rebuilt when the weights change: W_self for H.W_self (nn) and dS.W_self^T (nt);
  // basis kind: W'_dir for Zc.W' (nn) and Dc.W'^T (nt), two groups each.  Split arithmetic only (rgcn_set_gemm_mode 6 / 9).
  void *wself_nn = nullptr, *wself_nt = nullptr, *wrel_nn = nullptr, *wrel_nt = nullptr;
  // BLOCK, destination-major banded layer kernel (block_rows.hip): band-tiled copy of wrel,
  // [2R][8 bands][ceil(sd*sd/4)][GW lanes][4], allocated at create wherever block_rows_available() can hold
  float* wtile = nullptr;
  uint64_t wtile_version = ~0ull;
  // highway context (RGCN_SKIP_HIGHWAY): the gate's weight [d,d] and bias [d] (highway_layer.py) and their gradients
  float *whw = nullptr, *gwhw = nullptr, *bhw = nullptr, *gbhw = nullptr;
  // BASIS_TDIAG: wrel = [2][d][B*d] (W_forward, W_backward in the host layout: the B operand of P = H . W, N contiguous),
  // coef = [2R][B][d]; tdiag_g = sigmoid(coef), rebuilt when the weights change (basis_tdiag.hip)
  float* tdiag_g = nullptr;
  uint64_t tdiag_g_version = ~0ull;
  // BASIS_PDIAG: wrel / grel / coef / gcoef / the fragment tables as BASIS, except that the two direction groups of wrel
  // and grel are SWAPPED (group 0 = W_backward, group 1 = W_forward: the forward-direction units contract with W_backward,
  // basis_pdiag.hip); dtab = [2R][d] (first R = D_types_forward), gdtab its gradient
  float *dtab = nullptr, *gdtab = nullptr;
};

struct GraphBufs {
  DevPool pool;                 // owns every device buffer of the set (owner / errflag are the context's)
  int32_t* triples = nullptr;   // [maxE,3] (only when the host variant of set_graph is used)
  const int32_t* cur = nullptr; // triples of the current graph (ours or the caller's)
  int64_t E = 0;
  int32_t* indeg = nullptr;     // [V]
  int32_t* outdeg = nullptr;    // [V]
  int32_t* counters = nullptr;  // base of the zero-initialised block (indeg, outdeg, nlong)
  size_t counters_bytes = 0;
  int32_t* row_ptr = nullptr;   // [V+1]
  int32_t* long_rows = nullptr; // compacted list of rows with more than kLongRow slots (and at most the giant threshold)
  // giant rows: per row its first piece id and piece count; per piece its row and its index inside the row;
  // ngiant[0] = rows, ngiant[1] = pieces (device counters in the zero-initialised block)
  int32_t *giant_rows = nullptr, *giant_first = nullptr, *giant_cnt = nullptr, *piece_row = nullptr, *piece_k = nullptr;
  int32_t* ngiant = nullptr;
  int32_t giant_cap = 0, piece_cap = 0;
  bool giant_on = false;        // this graph was prepared with the giant-row cut enabled
  // rows ordered by DESCENDING number of slots, long / giant rows last (block kind, one GPU: the destination-major
  // layer kernel hands the four lane groups of a wavefront rows of equal length); row_key[v] = 32 - slots (33: long)
  uint32_t *row_key = nullptr, *row_key_s = nullptr;
  int32_t* row_order = nullptr;
  uint16_t* row_tab = nullptr;
  int32_t* nlong = nullptr;     // device counter (lives in the zero-initialised counter block)
  int32_t long_cap = 0;
  int32_t* rel_ptr = nullptr;   // [2R+1]
  int chunk = 48;               // messages per relation chunk of THIS graph (scales with its size)
  int32_t* chunk_ptr = nullptr; // [2R+1]
  int32_t* cum_in = nullptr;    // [V+1]  (tf_as_executed)
  int32_t* cum_out = nullptr;   // [V+1]
  uint32_t *keyv = nullptr, *keyv_s = nullptr, *keyr = nullptr, *keyr_s = nullptr;  // [2maxE]
  int32_t *valv = nullptr, *permv = nullptr, *valr = nullptr, *permr = nullptr;      // [2maxE]
  int32_t* pos = nullptr;       // [2maxE] incidence -> CSR slot
  // relation-sorted message list (SoA, [2maxE] each)
  int32_t *m_src = nullptr, *m_dst = nullptr, *m_dslot = nullptr, *m_sslot = nullptr;
  // slot-ordered copies for the row-major gathers of the basis path (destination order: d_*, source
  // order: s_*): partner vertex, directed relation, normalisation of the message in that slot
  int32_t *d_src = nullptr, *d_rel = nullptr, *s_dst = nullptr, *s_rel = nullptr;
  float *d_norm = nullptr, *s_norm = nullptr;
  float* m_norm = nullptr;
  // basis kind: the (row, direction) UNITS of the graph -- row v has a unit of direction dir (0: messages of W_forward,
  // arriving along an edge; 1: W_backward) iff one of this rank's messages of that direction lands on it.  The dense
  // contractions of the basis layer run over units, not over all V rows (basis.hip).  has_dir [2][V] 0/1;
  // unit_ptr [2][V+1] = its exclusive scan (unit index of (v, dir); entry V = number of units); unit_rows [2][V] = the
  // row of every unit, ascending
  int32_t *has_dir = nullptr, *unit_ptr = nullptr, *unit_rows = nullptr;
  int64_t units_host = -1;      // number of units, once somebody has read it back (profile accounting); -1: unknown
  uint32_t *keyv_t = nullptr, *keyr_t = nullptr;   // sort scratch (csr_sort.hip)
  uint16_t *tablev = nullptr, *tabler = nullptr;
  // RGCN_NORM_LOCAL where the vertex key cannot carry the relation: the relation-sorted message list stably sorted by
  // destination (keyd_s = destinations, permd = positions in the message list), and that sort's scratch
  uint32_t *keyd = nullptr, *keyd_s = nullptr, *keyd_t = nullptr;
  int32_t *vald = nullptr, *permd = nullptr;
  uint16_t* tabled = nullptr;
  // prefetch bookkeeping (rgcn_prefetch_graph_device): which graph this set was prepared for
  const int32_t* pf_tri = nullptr;
  int64_t pf_E = -1;
  int64_t pf_keep = -1;         // >= 0: prepared under edge dropout (keep of pf_E batch edges, seed pf_eseed)
  uint64_t pf_eseed = 0;
  bool pf_valid = false;
  hipEvent_t ev_ready = nullptr;   // recorded on the prefetch stream when the set is complete
  hipEvent_t ev_free = nullptr;    // recorded on the main stream when the last step using the set ended
  bool ready_in_capture = false, free_in_capture = false;   // those records belong to the running capture
  // both sets point at the context's one copy of these (rgcn_ctx::pool)
  int32_t* owner = nullptr;     // [R]
  int32_t* errflag = nullptr;   // device int: nonzero = bad id seen
  bool ready = false;
};

// decoder batch structures (csrc/decoder.hip)
struct DecoderBufs {
  DevPool pool;
  int64_t maxN = 0;
  int32_t relations = 0;       // the relation bound the buffers were sized for (decoder_relations at the reserve)
  int32_t N = 0;
  int64_t N_total = 0;         // triples of the whole batch when N is one rank's slice of it (denominator of the means)
  // the last batch rgcn_negative_sample_device (or the fused minibatch step) wrote: `tiled_period` rows tiled rate + 1
  // times into tiled_X -- rows p, p + period, p + 2 period, ... differ from row p in ONE entity.  decoder_prepare sorts
  // only the first copies by relation and puts the others directly behind them (k_dec_expand): a third of the sort work,
  // and the copies of a triple sit next to each other in a relation chunk, their shared rows fetched from HBM once
  // instead of rate + 1 times.  The expansion checks that every copy still has its first copy's relation (flag 16).
  const int32_t* tiled_X = nullptr;
  int64_t tiled_period = 0, tiled_N = 0;
  int32_t* perm_pos = nullptr; // first copies in relation order
  const int32_t* X = nullptr;
  uint32_t *keyv = nullptr, *keyv_s = nullptr, *keyr = nullptr, *keyr_s = nullptr;
  int32_t *valv = nullptr, *permv = nullptr, *valr = nullptr, *permr = nullptr;
  int32_t *row_ptr = nullptr, *rel_ptr = nullptr, *chunk_ptr = nullptr;
  int32_t *e_other = nullptr, *e_rel = nullptr, *e_trip = nullptr;
  int32_t *long_rows = nullptr, *nlong = nullptr;     // nlong[0] = long rows, nlong[1] = their pieces
  int32_t *long_first = nullptr, *long_cnt = nullptr;  // per long row: first piece id, number of pieces
  int32_t *piece_row = nullptr, *piece_k = nullptr;    // per piece: its row, its index inside the row
  float* piece_slab = nullptr;                         // [piece_cap][d] partial sums of the pieces
  int32_t long_cap = 0, piece_cap = 0, max_chunks = 0, energy_blocks = 0;
  float *dx = nullptr, *loss_part = nullptr, *slab = nullptr;
  // band-major, line-aligned copies of the codes and of W_relation for the line form of the entity gradient
  // (decoder.hip, k_dec_entity_lines): [bands][V][32] and [bands][R][32], bands = ceil(d / 32); rebuilt every call
  float *cb = nullptr, *rb = nullptr, *e_g = nullptr;   // e_g: the loss gradient of every incidence slot
  uint32_t *row_key = nullptr, *row_key_s = nullptr;    // rows by descending number of incidences (one radix pass)
  int32_t* row_order = nullptr;
  uint16_t* row_tab = nullptr;
  int32_t nbands = 0, cus = 0;     // cus: compute units of the device (persistent workgroups of the line kernel)
  double* loss = nullptr;
  uint32_t *keyv_t = nullptr, *keyr_t = nullptr;   // sort scratch (csr_sort.hip)
  uint16_t *tablev = nullptr, *tabler = nullptr;
  hipEvent_t ev_ready = nullptr;
  bool loss_valid = false;
};

// device neighbourhood sampler (csrc/neighborhood.hip): the training graph and the scratch of one draw
struct NeighborhoodBufs {
  DevPool pool;
  int64_t n = 0;                         // training triples
  int32_t* triples = nullptr;            // [n,3]
  // adjacency CSR by vertex, self loops left out: the other endpoint, and the id 2 e + side of the edge END AT THAT
  // OTHER endpoint (whose clock a relaxation adds)
  int32_t *adj_other = nullptr, *adj_end = nullptr;
  int32_t *seg_v = nullptr, *seg_beg = nullptr, *seg_end = nullptr;     // segments of <= 256 entries of one vertex's list
  int32_t nseg = 0;
  int32_t launches = 64;                 // sweep launches of one draw (from the graph's diameter, at reserve)
  int32_t* comp = nullptr;               // [V] connected component of the vertex (-1: no edges)
  uint8_t* comp_state = nullptr;         // [ncomp] 1: every edge of the component is in the batch (device copy)
  uint32_t* dist = nullptr;              // [V] touched-time (bits of a non-negative float)
  unsigned long long* tkey = nullptr;    // [n] (pick time | edge id) of the boundary component's edges, ~0 elsewhere
  uint32_t* hist = nullptr;              // [4096] digit histogram of the radix select
  unsigned long long* state = nullptr;   // select state (prefix, wanted rank)
  int32_t* changed = nullptr;            // per-launch "something moved" flags of the relaxation
  uint32_t* bcnt = nullptr;              // per-block counts / offsets of the compaction
  void* params = nullptr;                // the draw's parameters (seed, start vertex, ...: neighborhood.hip DrawParams)
  hipGraph_t draw_graph = nullptr;       // the kernels of one draw, recorded once, replayed per draw
  hipGraphExec_t draw_exec = nullptr;
  hipStream_t capture_stream = nullptr;
  // one set of per-draw state (params, distances, keys, select state, the graph) serves draws on the main AND the
  // prefetch stream: a draw on the other stream waits for the previous draw's end
  hipEvent_t ev_draw = nullptr;
  hipStream_t last_draw_stream = nullptr;
  // host side (components are a property of the graph: found once, at reserve)
  std::vector<int32_t> comp_h;           // [V]
  std::vector<int64_t> comp_edges_h;     // [ncomp] edges per component
  std::vector<uint8_t> comp_state_h;     // [ncomp] scratch of one draw
  int32_t ncomp = 0;
};

// index of known positives of the exclusive negative sampler (rgcn_known_positives_reserve; negative_exclusive.h)
struct KnownPositives {
  DevPool pool;                            // keys, unresolved
  uint64_t* keys = nullptr;                // [count] sorted unique packed keys (r V + s) V + o
  uint64_t* keys_by_object = nullptr;      // [count] the same set sorted by (r V + o) V + s (known_index_build_by_object):
                                           // the known subjects of a pair (r, o) are one range (the entity-softmax mask)
  int64_t count = 0;                       // 0: no index
  unsigned long long* unresolved = nullptr;  // rows every entity was known for, since the reserve (RGCN_BUF_NEGATIVE_UNRESOLVED)
  unsigned long long* relation_unresolved = nullptr;  // relation rows every other relation was known for
                                                      // (RGCN_BUF_NEGATIVE_RELATION_UNRESOLVED)
  bool exclusive = false;                  // rgcn_set_exclusive_negatives: the fused minibatch step draws exclusively
};

// per-relation entity sets of the type-constrained sampler and queries (rgcn_type_sets_reserve; type_sets.h builds them,
// negative_typed.h and ranking.hip read them)
struct TypeSetsDev {
  DevPool pool;                            // ptr, idx, mask, open
  int64_t* ptr = nullptr;                  // [2 R + 1]; list l = side R + r
  int32_t* idx = nullptr;                  // [ptr[2 R]] members, ascending inside a list
  uint32_t* mask = nullptr;                // [2 R][words]: bit e of row l (an open list: all V bits; pad bits clear)
  int64_t words = 0;                       // ceil(V / 32)
  bool ready = false;                      // false: no sets
  unsigned long long* open = nullptr;      // rows drawn over all entities, since the reserve (RGCN_BUF_NEGATIVE_TYPED_OPEN)
  bool typed = false;                      // rgcn_set_typed_negatives: the fused minibatch step draws from the lists
};

// the relation-softmax term (csrc/relation_softmax.hip; rgcn_relation_softmax_reserve): buffers of ONE chunk of positives
struct RelsmBufs {
  DevPool pool;
  int64_t maxP = 0;                       // what the reserve was asked for
  RelsmPlan plan;                         // chunk, padded R, split (relation_softmax_plan.h)
  float *Q = nullptr, *dQ = nullptr;      // [chunk, dc] query rows codes[s] * codes[o] and their gradients
  float *E = nullptr, *G = nullptr;       // [chunk, padded R] each: the energies, and their gradients (the row pass reads
                                          // one and writes the other, so both stay readable); pad columns stay zero
  float* Wp = nullptr;                    // [padded R, dc] rows [0, R) of W_relation, pad rows zero (copied every call)
  float* dW = nullptr;                    // [padded R, dc] G^T Q of the chunk
  float* loss_part = nullptr;             // one partial per workgroup of the row pass
  float* slab = nullptr;                  // split-K slabs of dW = G^T Q (GemmCall::slab), plan.split_k x [padded R, dc]
  size_t slab_floats = 0;
  // by-entity CSR of the chunk's 2n incidences (subject side first), built with the library's stable sort
  uint32_t *key = nullptr, *key_s = nullptr, *key_t = nullptr;
  int32_t *perm = nullptr, *val_t = nullptr;
  uint16_t* table = nullptr;
  int32_t *row_ptr = nullptr, *e_other = nullptr, *e_trip = nullptr;
  int32_t *long_rows = nullptr, *long_first = nullptr, *long_cnt = nullptr, *nlong = nullptr;   // nlong[0] rows, [1] pieces
  int32_t *piece_row = nullptr, *piece_k = nullptr;
  float* piece_slab = nullptr;            // [piece_cap][dc]
  int32_t long_cap = 0, piece_cap = 0;
  const int32_t* csr_X = nullptr;         // relation_softmax_prepare built the CSR of these positives' first csr_n rows
  int csr_n = 0;                          // (consumed, or rebuilt, by the next relation_softmax_compute)
  int64_t last_n = 0;                     // positives of the chunk the buffers hold (RGCN_BUF_RELATION_SOFTMAX_*); 0: none
  // rgcn_set_relation_softmax: the term inside the fused steps
  float weight = 0.f;
  int64_t step_positives = 0;             // leading rows of an X/Y step's batch; 0: the minibatch step only
  bool exclusive = false;
};

// self-adversarial negatives (csrc/adversarial.hip; rgcn_set_adversarial_negatives)
struct AdversarialState {
  DevPool pool;
  float* w = nullptr;                     // [cap] the weights of the last fused step under the mode (RGCN_BUF_ADVERSARIAL_WEIGHTS)
  int64_t cap = 0;
  int64_t last_N = 0;                     // rows of that step; 0: none yet
  float temperature = 0.f;                // 0: off
  int64_t step_positives = 0;             // leading rows of an X/Y step's batch; 0: the minibatch step only
};

// the entity-softmax term (csrc/entity_softmax.hip; rgcn_entity_softmax_reserve): buffers of ONE chunk of rows, two rows
// per positive (object row m = n, subject row m = P + n)
struct EntsmBufs {
  DevPool pool;
  int64_t maxP = 0;                       // what the reserve was asked for
  EntsmPlan plan;                         // chunk, padded V, split, form of the NN product (entity_softmax_plan.h)
  float *Q = nullptr, *dQ = nullptr;      // [chunk, dc] query rows codes[a] * W_relation[r] and their gradients
  float* E = nullptr;                     // [chunk, padded V]: the energies, overwritten in place by their gradients G;
                                          // pad columns stay zero
  float* Cp = nullptr;                    // plan.nn_padded: [padded V, dc] the codes, pad rows zero (copied every call)
  float* dC = nullptr;                    // [padded V, dc] G^T Q of the chunk
  float* loss_part = nullptr;             // one partial per workgroup of the row pass
  float* slab = nullptr;                  // split-K slabs of dC (GemmCall::slab), plan.split_k x [padded V, dc]
  size_t slab_floats = 0;
  int32_t* rows = nullptr;                // [chunk, 4] (query entity, relation, gold, side) of every row; gold -1: a bad row
  // CSR of the chunk's rows by query entity, then by relation (one after the other through the same buffers), built
  // with the library's stable sort
  uint32_t *key = nullptr, *key_s = nullptr, *key_t = nullptr;
  int32_t *perm = nullptr, *val_t = nullptr;
  uint16_t* table = nullptr;
  int32_t *row_ptr = nullptr, *e_other = nullptr;      // [max(V, R) + 1]; the other factor's row of every slot
  int32_t *long_rows = nullptr, *long_first = nullptr, *long_cnt = nullptr, *nlong = nullptr;   // nlong[0] rows, [1] pieces
  int32_t *piece_row = nullptr, *piece_k = nullptr;
  float* piece_slab = nullptr;            // [piece_cap][dc]
  int32_t long_cap = 0, piece_cap = 0;
  int64_t last_n = 0;                     // rows of the chunk the buffers hold (RGCN_BUF_ENTITY_SOFTMAX_*); 0: none
  // rgcn_set_entity_softmax: the term inside the fused steps
  float weight = 0.f;
  int64_t step_positives = 0;             // leading rows of an X/Y step's batch; 0: the minibatch step only
  bool exclusive = false;
};

struct OptimizerState {
  DevPool pool;              // moments, state, shard_sq
  DevPool part_pool;         // `part` alone: it is the one buffer that grows
  bool configured = false;
  int32_t algorithm = RGCN_OPT_ADAM;
  float lr = 0.01f, beta1 = 0.9f, beta2 = 0.999f, eps = 1e-8f, max_norm = 0.f;
  float init_acc = 0.1f;     // AdaGrad: what a new accumulator is filled with
  int64_t t = 0;
  std::vector<float*> m, v;  // per parameter: Adam's moments (slots 0, 1); AdaGrad's accumulator is m (slot 0), v stays null
  float* part = nullptr;
  size_t part_cap = 0;
  float* state = nullptr;    // [clip scale, global norm, step count t, bias-corrected rate]
  float* shard_sq = nullptr; // world > 1: squared norm of this rank's relation-sharded gradients (all-reduced)
  bool norm_pending = false; // optimizer_norm_partial ran, optimizer_apply has not
};

// ranking scratch (csrc/ranking.hip)
struct RankBufs {
  DevPool pool;
  float *q = nullptr, *s = nullptr;      // query rows [max,dc], energies [max,V]
  int32_t* bad = nullptr;
  float* thr = nullptr;                  // per query: the smallest energy whose fp32 sigmoid reaches the gold entity's
  float* mixed = nullptr;                // mixed scores [max,V]: null until the first rgcn_topk_mixed_device at this size
  float* rel = nullptr;                  // relation-side energies [max,R]: null until the first relation query at this size
  int64_t max = 0;
};

}  // namespace rgcn

struct rgcn_ctx {
  rgcn_config cfg;
  // Owns every device buffer that lives as long as the context: parameters, gradients, activations, slabs, the lazily
  // allocated masks / giant_slab / dcodes_own / replay_counter, the relation owner table and the error flag.  The graph
  // sets, the decoder batch, the sampler, the optimizer and the ranking scratch own theirs (their structs' pools).
  rgcn::DevPool pool;
  int V = 0, R = 0, d = 0, L = 0, nb = 0, sd = 0, kind = 0, B = 0;
  // The code width (CodeDimension): what the decoder, the ranking calls, W_relation and dcodes are wide.  dc == d and
  // codes == H[L] unless the context has an output transform (rgcn_config_ext::code_dim > 0; output_transform.hip):
  //   codes = H_L . W_out + b_out [V,dc]; the backward pass opens with out_dh = dcodes . W_out^T [V,d], which the layer
  //   stack takes for its dcodes (RGCN_BUF_OUT_DH), g_w_out = H_L^T . dcodes and g_b_out = the column sums of dcodes.
  // The layer stack keeps d.
  int dc = 0;
  bool out_layer = false;
  float *w_out = nullptr, *g_w_out = nullptr, *b_out = nullptr, *g_b_out = nullptr;
  void* wout_nn = nullptr;                // W_out's fragment table (the B operand of H_L . W_out; split arithmetic only)
  float* codes = nullptr;                 // [V,dc]; H[L] itself on a context without the layer
  float* out_dh = nullptr;                // [V,d]
  bool out_dh_valid = false;              // a backward pass has written out_dh
  int rank = 0, world = 1;
  // highway skip connections around every layer (rgcn_config_ext::skip_mode == RGCN_SKIP_HIGHWAY; highway.hip; one GPU,
  // embedding input): the layers write N_l, the highway pass T_l and H_l; all four buffers exist on such a context only
  bool highway = false;
  std::vector<float*> hw_N, hw_T;         // [1..L] N_l and T_l, [V,d] each, kept for the backward pass
  float* hw_dz[2] = {nullptr, nullptr};   // dZ_l, ping-pong like D / dS (layer 2's dW_hw GEMM may trail beside layer 1)
  float* hw_carry = nullptr;              // G_l * (1 - T_l)
  int hw_last = 0;                        // the layer the last fwd_layer_finish ran (RGCN_BUF_HIGHWAY_INNER / _GATE)
  // RGCN_KIND_BASIS_TDIAG (basis_tdiag.hip; one GPU, embedding input, no highway): P_l = H_{l-1} . [W_f | W_b] of every
  // layer ([2][V][B.d], kept for dC), ONE dP of that shape, the two directions' dP . W^T products [2][V][d]
  std::vector<float*> tdiag_P;            // [1..L]
  float* tdiag_dP = nullptr;
  float* tdiag_dh = nullptr;
  int tdiag_last = 0;                     // the layer the last fwd_layer_finish ran (RGCN_BUF_TDIAG_PRODUCTS)
  // RGCN_KIND_BASIS_PDIAG (basis_pdiag.hip; one GPU, embedding input, no highway): the mixing table a_l [2][V][B] of every
  // layer (the backward pass reads it), the diagonal aggregate [V,d] of the layer run last, da [2][V][B], the row-local
  // part of dH [V,d], the chunk slabs of dD ([chunks][d], inside slab_dw behind the [chunks][B] of dC)
  std::vector<float*> pdiag_a;            // [1..L]
  float* pdiag_agg = nullptr;
  float* pdiag_da = nullptr;
  float* pdiag_dh = nullptr;
  float* pdiag_slab_dd = nullptr;
  size_t pdiag_slab_chunks = 0;           // chunks either slab holds
  int pdiag_last = 0;                     // the layer the last fwd_layer_finish ran (RGCN_BUF_PDIAG_MIX / _AGG)
  // RGCN_KIND_EMBEDDING (the reference's Name=embedding encoder, the DistMult baseline): no graph and no layer.  The codes
  // ARE W_emb (H[0] = w_emb), their gradient is written where the optimizer reads it (dcodes_own = g_emb): of the buffers
  // below only the parameters, their gradients, the error flag, `zeros` and a one-tile slab exist on such a context
  bool embedding = false;
  bool onehot = false;          // featureless first layer (RGCN_INPUT_ONEHOT): no W_emb / b_emb / H_0, layer 1 is basis_onehot.hip
  int row_lo = 0, row_hi = 0;   // row shard of this rank: [rank * shard_rows, +shard_rows) cut at V
  int shard_rows = 0;           // ceil(V / world): equal chunks for the reduce-scatter / all-gather
  int V_pad = 0;                // world * shard_rows: rows every exchanged [V,d] buffer is allocated with
  float* repl_grads = nullptr;  // world > 1: W_self (and basis W') gradients of all layers, contiguous -> ONE all-reduce
  size_t repl_grads_floats = 0;
  hipEvent_t ev_gather = nullptr;   // the all-gather of the rows finished last (side stream 1) is complete
  bool gather_pending = false;      // ... and somebody still has to wait for it
  hipStream_t stream = nullptr;           // stream launches go to (main stream unless a StreamScope is active)
  hipStream_t main_stream = nullptr;
  hipStream_t aux[rgcn::kAuxStreams] = {nullptr, nullptr, nullptr};  // side streams: 0, 1 for independent kernels of one layer,
                                                               // 2 for the decoder's relation gradient (runs beside the backward pass)
  hipEvent_t ev_fork = nullptr, ev_join[rgcn::kAuxStreams] = {nullptr, nullptr, nullptr};
  bool use_aux = true;
  bool aux_dirty[rgcn::kAuxStreams] = {false, false, false};   // something was forked onto side stream k since its last join
  // block kind: 0 = message kernel + k_combine (two kernels, [2E,d] message buffer), 1 = the destination-major banded
  // single-pass layer (block_rows.hip; no message buffer, weights through L2)
  int fuse = 1;
  uint64_t weights_version = 1;           // bumped whenever a parameter value changes (set_param, Adam)
  bool dw_pending = false;                // a dW-only message-gradient kernel of the previous backward layer is still on side stream 0
  // Deferred end-of-step joins (rgcn_step_device at minibatch scale).  The backward pass of such a step
  // ends WITHOUT making the main stream wait for its side kernels: aux_dirty[0 / 1] stay set ("gradients pending") and
  //   SIDE_RECORDED: ev_join[0] (side stream 0, behind a wait for side stream 1) marks the end of every side kernel of the
  //                  backward layers -- all that reads activations, D / dS and the graph -- but not of the bias gradient's
  //                  column sums, which trail on side stream 1;
  //   SIDE_READS_JOINED: the main stream has waited for that event (the next forward pass may overwrite the activations);
  //                  the gradients themselves are still unjoined.
  // A full join (join_abandoned_side_work, sync_all) returns to SIDE_NONE.
  enum { SIDE_NONE = 0, SIDE_RECORDED = 1, SIDE_READS_JOINED = 2 };
  int side_state = SIDE_NONE;
  bool defer_end_joins = false;           // the backward pass in flight may end unjoined (set by rgcn_step_device)
  std::string err;

  std::vector<rgcn::Param> params;
  std::vector<rgcn::LayerBufs> layers;   // index 1..L (0 unused)
  float *w_emb = nullptr, *g_emb = nullptr, *b_emb = nullptr, *gb_emb = nullptr;
  float *w_rel = nullptr, *g_rel = nullptr;   // W_relation [EntityCount, dc] (decoder weight)
  rgcn::DecoderBufs dec;
  rgcn::NeighborhoodBufs nbr;
  rgcn::KnownPositives known;
  bool reciprocal = false;               // rgcn_set_reciprocal_relations: (?, r, o) is asked of W_relation[R + r]
  int32_t relation_negatives = 0;        // rgcn_set_relation_negatives: relation rows per positive in the fused minibatch step
  rgcn::TypeSetsDev types;
  rgcn::RelsmBufs relsm;
  rgcn::EntsmBufs entsm;
  rgcn::AdversarialState adv;
  rgcn::OptimizerState opt;

  std::vector<float*> H;                 // H[0..L], [V,d] each
  float* self_buf = nullptr;             // S / G : [V,d]
  float* exch = nullptr;                 // exchange buffer [V,d] (world > 1)
  float* dbuf[2] = {nullptr, nullptr};   // D_l ping-pong
  float* dsbuf[2] = {nullptr, nullptr};  // dS_l ping-pong
  float* msgbuf = nullptr;               // Y / Z : [2*maxE, d]  (BLOCK)   or Z [V, 2B*d] (BASIS)
  float* msgbuf2 = nullptr;              // BASIS: dZ [V, 2B*d]
  std::vector<float*> zsave;             // BASIS: Z of every layer, kept for dW' = Z^T.D
  float* aggbuf = nullptr;               // BASIS: Z.W' product [V,d]
  float* slab = nullptr;                 // split-K partial slabs of the GEMM
  size_t slab_floats = 0;
  float* slab_dw = nullptr;              // per-chunk dW slabs of the block-diagonal backward
  size_t slab_dw_floats = 0;
  float* stage = nullptr;                // host<->device staging for layout conversion
  size_t stage_floats = 0;
  uint8_t* masks = nullptr;              // [L,V,d] explicit dropout masks
  float* colsum_part = nullptr;           // two halves of colsum_part_floats each: a pass whose column sums finish on a side
  size_t colsum_part_floats = 0;          // stream (deferred joins) leaves its half to them and hands the next pass the other
  int colsum_half = 0;
  int32_t colsum_parts = 0;    // > 0: the last block_rows backward launch left that many [d] partial rows in colsum_part
  float* zeros = nullptr;                // 1024 zero floats (masked-lane load target of the GEMMs; 3 KB for a masked LDS-DMA)

  rgcn::GraphBufs g;                     // ACTIVE graph structures
  rgcn::GraphBufs g_alt;                 // second set: next graph is prepared here beside the running step
  hipStream_t pf_stream = nullptr;       // stream of rgcn_prefetch_graph_device
  int aux_priority = 0, pf_priority = 0;  // what the side / prefetch streams were created with (stream pool key)
  // pinned staging ring of rgcn_copy_to_device_async: the caller's memory is copied here during the call, the
  // transfer itself is stream-ordered and the host does not wait for it
  static constexpr int kStageSlots = 8;
  static constexpr size_t kStageBytes = (size_t)1 << 20;
  uint8_t* stage_host = nullptr;         // kStageSlots * kStageBytes, hipHostMalloc
  uint8_t* readback_host = nullptr;      // 32 pinned bytes: rgcn_get_loss fetches the loss and the error flag with one wait
  hipEvent_t stage_done[kStageSlots] = {};
  int stage_next = 0;
  int chunk = 48;                        // messages per relation chunk (capacity-scaled upper bound; GraphBufs::chunk is per graph)
  int gemm_mode = 0;                     // 0: fp32 MFMA; 3/6/9: bf16 split with that many partial products
  int msg_block = 0, msg_slots = 0;      // k_msg launch geometry

  // forward/backward state
  uint64_t frag_version = ~0ull;         // weights_version the weight fragment tables (LayerBufs::wself_nn ...) were built from
  bool frag_fresh = false;               // ... built since the last rgcn_forward_begin (captured steps rebuild once per step)
  bool wtile_fresh = false;              // the same for the band-tiled block weights (LayerBufs::wtile)
  bool fwd_done = false;
  bool h0_in_gemm = false;               // fwd_begin left H0 = relu(W_emb + b_emb) to layer 1's self-loop product (rgcn_schedule.hip)
  int fwd_train = 0;
  uint64_t seed = 0;
  bool explicit_masks = false;
  const float* bwd_D = nullptr;          // D_l of the backward layer in flight
  const float* bwd_dS = nullptr;         // dS_l = D_l * dropout_l
  int bwd_layer = 0;                     // next layer the backward pass will process (L..1, 0 = done)
  // hipGraph capture (rgcn_capture_begin / _end / rgcn_graph_launch)
  bool capturing = false;
  bool use_aux_before_capture = true;    // side-stream setting to restore when the capture ends
  bool cap_pf_forked = false;            // the prefetch stream has joined the capture and must be joined back
  uint64_t* replay_counter = nullptr;    // device counter bumped at the start of every captured graph
  hipEvent_t ev_step_begin = nullptr;    // recorded on the main stream where a step starts (capture: fork point of the prefetch)
  bool step_begin_in_capture = false;
  std::vector<hipGraphExec_t> graphs;
  std::vector<hipGraph_t> graph_defs;
  float* giant_slab = nullptr;           // [piece_cap][d] partial sums of giant-row pieces (scratch of one combine launch)
  rgcn::RankBufs ranking;
  float* dcodes_own = nullptr;           // [V,dc] staging for the host variant of backward

  // comm
  void* comm = nullptr;                  // ncclComm_t
  // profiling
  bool prof_on = false;
  bool dropout_lds_configured = false;   // k_edge_dropout's dynamic-LDS attribute set on this context's device
  std::vector<rgcn::ProfRec> prof;
  std::vector<hipEvent_t> event_pool;
  std::vector<rgcn::ProfAgg> prof_agg;
  hipEvent_t t0 = nullptr, t1 = nullptr;
};

namespace rgcn {

// Flags of the events that only ORDER this context's own streams on its own device (fork / join of the side streams, the
// prefetched graph structures, the decoder batch, the sampler's state).  A default hipEventRecord is a barrier packet with a
// system-scope release and acquire; what these events order is kernels of one device, each of which already carries its
// agent-scope fences, so on one GPU the event's own fence is dropped: 0.528-0.534 ms per headline step against 0.535-0.543,
// three interleaved runs each on one box (release-to-device scope: 0.538-0.540).  A sharded
// context, whose buffers other ranks' kernels read and write, keeps the default.
// kernel_only: the event orders kernels against kernels (fork, join).  Events that can also order copy-engine work -- a
// graph set's ready / free (host staging copies and memsets on the prefetch stream), the sampler's draw, the decoder batch's
// ready event, the step-begin marker -- keep the default fence: HIP documents no agent-scope release for SDMA operations.
inline unsigned order_event_flags(const rgcn_ctx* c, bool kernel_only = false) {
  return hipEventDisableTiming | (kernel_only && c->world == 1 ? hipEventDisableSystemFence : 0u);
}

// rows of W_relation the decoder, the adversarial weights and the optimizer work on: R, or 2 R under reciprocal relations
inline int decoder_relations(const rgcn_ctx* c) { return c->reciprocal ? 2 * c->R : c->R; }

// The one way the library allocates device memory: `pool` owns the block (n elements of T, or n bytes through a void**);
// zero queues a memset of it on the context's current stream.  Out of memory is RGCN_ERR_NOMEM.
template <class T>
inline rgcn_status dmalloc(rgcn_ctx* c, DevPool& pool, T** p, size_t n, bool zero) {
  return pool.alloc(p, n, zero, c->stream, &c->err);
}

// the partial sums of the giant-row pieces (rgcn_ctx::giant_slab), allocated when a graph with the cut on first meets a layer
inline rgcn_status giant_slab_ensure(rgcn_ctx* c) {
  if (c->giant_slab) return RGCN_OK;
  return dmalloc(c, c->pool, &c->giant_slab, (size_t)c->g.piece_cap * c->d, false);
}

// Runs the launches inside its scope on side stream k, ordered after everything already queued on
// the main stream (fork); join() makes the main stream wait for that side stream again.
struct StreamScope {
  rgcn_ctx* c;
  hipStream_t saved;
  bool active;
  // in_capture: the fork is also taken while a step is being captured (a captured step is otherwise one chain: the
  // side streams are switched off for the capture, rgcn_capture_begin)
  StreamScope(rgcn_ctx* ctx, int k, bool in_capture = false);
  ~StreamScope();
};
rgcn_status stream_join(rgcn_ctx* c, int k);
// the column-sum scratch of the pass in flight (rgcn_ctx::colsum_part, the current half)
inline float* colsum_scratch(const rgcn_ctx* c) { return c->colsum_part + (size_t)c->colsum_half * c->colsum_part_floats; }

// Brackets a launch with events when profiling is on.
struct ProfScope {
  rgcn_ctx* c;
  int idx;
  // bytes = DESIGN bytes (what the kernel requests from the memory system by construction: gathers counted per use,
  // staging slabs included); compulsory = every distinct input byte once + every output byte once, < 0:
  // the same figure.  Roofline fractions are computed on the compulsory bytes.
  ProfScope(rgcn_ctx* ctx, const char* name, double bytes, double flops, double compulsory = -1.0);
  ~ProfScope();
};

// ---- graph_prep.hip
rgcn_status graph_alloc(rgcn_ctx* c, GraphBufs& g);   // fills the set it is handed (owner / errflag: the caller)
void graph_free(rgcn_ctx* c);
rgcn_status graph_build(rgcn_ctx* c, const int32_t* triples_dev, int64_t E);
rgcn_status graph_build_dropout(rgcn_ctx* c, const int32_t* batch_dev, int64_t n, int64_t keep, uint64_t seed,
                                const uint8_t* keep_mask_dev);

// ---- csr_sort.hip: stable sort of (key, position) pairs by a small integer key, up to two sorts per call
struct SortSpec {
  const uint32_t* key_in;   // n keys, each <= max_key < 2^24
  uint32_t* key_out;        // sorted keys
  int32_t* val_out;         // original positions in key order (ties in position order)
  uint32_t* key_tmp;        // scratch, n elements each
  int32_t* val_tmp;
  int32_t* pos_out;         // optional: pos_out[position] = slot (inverse of val_out)
  uint16_t* table;          // scratch, sort_table_elems(n) elements
  int64_t n;
  uint32_t max_key;
};
size_t sort_table_elems(size_t n);
rgcn_status sort_pairs(rgcn_ctx* c, const char* tag, int njobs, const SortSpec* specs);

// ---- gemm_f32.hip (GemmBatch, GemmCall, GemmPlan and the decision itself: gemm_plan.h)
size_t gemm_bfrag_words(int K, int N);
struct PresplitJob {
  const float* B;      // the operand B (k, n): stored [n][k] (b_kc) or [k][n], leading dimension ldb
  void* F;             // its fragment table, gemm_bfrag_words(K, N) 16-byte words
  int ldb, K, N, b_kc;
};
rgcn_status gemm_presplit_b(rgcn_ctx* c, const PresplitJob* jobs, int n);

// C = A . B as GemmCall describes it: gemm_plan(call, c->gemm_mode, the RGCN_GEMM_W8 knob) followed by gemm_run
rgcn_status gemm_f32(rgcn_ctx* c, const char* tag, const GemmCall& call, double prof_scale = 1.0);
// the same, the call spelled out (GemmCall's fields; the slabs are the context's)
rgcn_status gemm_f32(rgcn_ctx* c, const char* tag, bool a_kc, bool b_kc, int M, int N, int K,
                     const float* A, int lda, const float* B, int ldb, float* C, int ldc,
                     int split_k, const GemmBatch* batch = nullptr, double prof_scale = 1.0);
// launches what the plan says (a refused plan: RGCN_ERR_UNSUPPORTED with the plan's reason), then the split-K reduce
rgcn_status gemm_run(rgcn_ctx* c, const char* tag, const GemmCall& call, const GemmPlan& plan, double prof_scale = 1.0);

// ---- block_msgs.hip
rgcn_status block_geometry(rgcn_ctx* c);
rgcn_status block_msg_forward(rgcn_ctx* c, int layer, const float* Hin, float* Ybuf);
// Zbuf == nullptr: the per-relation weight gradients only (the single-pass layer kernel computes the row gradients)
rgcn_status block_msg_backward(rgcn_ctx* c, int layer, const float* Hin, const float* D, float* Zbuf);
rgcn_status block_dw_reduce(rgcn_ctx* c, int layer);
rgcn_status block_to_device_layout(rgcn_ctx* c, const float* host_layout_dev, float* dst, int R);
rgcn_status block_from_device_layout(rgcn_ctx* c, const float* src, float* host_layout_dev, int R);

struct CombineArgs;
// ---- block_rows.hip: the block layer destination-major in ONE pass per direction, one column band per XCD, weights
// through L2 (no LDS table, no message buffer); bitwise equal to the two-kernel form
bool block_rows_available(const rgcn_ctx* c);
size_t block_rows_weight_floats(const rgcn_ctx* c);
rgcn_status block_rows(rgcn_ctx* c, const char* tag, int layer, bool backward, const float* X, const CombineArgs& ca);

// ---- basis.hip
rgcn_status basis_aggregate_forward(rgcn_ctx* c, int layer, const float* Hin, float* Z);
struct CombineArgs;
rgcn_status basis_backward_gather(rgcn_ctx* c, int layer, const float* dZ, const CombineArgs& ca,
                                  bool with_messages);
rgcn_status basis_dcoef(rgcn_ctx* c, int layer, const float* Hin, const float* dZ);
rgcn_status basis_dcoef_reduce(rgcn_ctx* c, int layer);   // the chunk partials in slab_dw -> gcoef of `layer`
double basis_units(rgcn_ctx* c);      // (row, direction) units of the current graph (profile accounting)
// Dc[dir][i][:] = D[row of unit i of direction dir][:]  (the compacted upstream rows, [2][V][d])
rgcn_status basis_gather_units(rgcn_ctx* c, const float* D, float* Dc);
rgcn_status basis_to_device_layout(rgcn_ctx* c, const float* host_layout_dev, float* dst);
rgcn_status basis_from_device_layout(rgcn_ctx* c, const float* src, float* host_layout_dev);

// ---- basis_tdiag.hip: the layer kernels of RGCN_KIND_BASIS_TDIAG (the GEMMs around them are the schedule's)
rgcn_status tdiag_refresh_gates(rgcn_ctx* c, int layer);                 // tdiag_g = sigmoid(coef) where the weights changed
// out = act(dropout(base) + sum over the row's messages of n sum_b G[rel,b,:] P_dir[src,b,:] + bias)
rgcn_status tdiag_rows_forward(rgcn_ctx* c, int layer, const float* P, const CombineArgs& ca);
// dP[dir][u][b][:] = sum over the messages u sends in direction dir of n G[rel,b,:] D[dst,:]; every row is written
rgcn_status tdiag_dp(rgcn_ctx* c, int layer, const float* D, float* dP);
// gcoef = G (1 - G) * sum over the relation's messages of n P_dir[src,b,:] D[dst,:]  (chunk slabs, chunk order)
rgcn_status tdiag_dcoef(rgcn_ctx* c, int layer, const float* P, const float* D);
// out = (base + dh[0] + dh[1]) * (gate > 0), out2 = out * dropout(drop2): the epilogue of the layer's backward pass
rgcn_status tdiag_dh_join(rgcn_ctx* c, const float* dh, const CombineArgs& ca);

// ---- basis_pdiag.hip: the layer kernels of RGCN_KIND_BASIS_PDIAG (the dense products are the basis kind's, the schedule's)
// one walk over every row's slots: a[dir][v][b] = sum n C[rel,b], agg[v] = sum n D[rel] * Hin[src], and the row's own
// compacted unit rows Zc[(v,dir),b,:] = a[dir][v][b] Hin[v,:] for the units that exist
rgcn_status pdiag_rows_forward(rgcn_ctx* c, int layer, const float* Hin, float* Zc, float* a, float* agg);
// out = act(((dropout(base) + the row's unit products of both directions) + agg) + bias)
rgcn_status pdiag_epilogue(rgcn_ctx* c, int layer, const float* prod, const float* agg, const CombineArgs& ca);
// row-local: da[dir][v][b] = <Hin[v], dZc[(v,dir),b,:]> (0 without a unit), dh[v] = sum_dir sum_b a[dir][v][b] dZc[(v,dir),b,:]
rgcn_status pdiag_row_backward(rgcn_ctx* c, const float* Hin, const float* dZc, const float* a, float* da, float* dh);
// gcoef[rel,b] = sum over the relation's messages of n da[dir][dst][b]  (chunk slabs, chunk order)
rgcn_status pdiag_dcoef(rgcn_ctx* c, int layer, const float* da);
// gdtab[rel,:] = sum over the relation's messages of n Hin[src,:] * D[dst,:]  (chunk slabs, compensated chunk reduce)
rgcn_status pdiag_ddiag(rgcn_ctx* c, int layer, const float* Hin, const float* D);
// out = ((base + dh) + sum over the messages row v sends of n dtab[rel] * D[dst]) * (gate > 0), out2 = out * dropout(drop2)
rgcn_status pdiag_dh_join(rgcn_ctx* c, int layer, const float* D, const float* dh, const CombineArgs& ca);

// ---- basis_onehot.hip: the featureless first layer (rgcn_config::input_mode == RGCN_INPUT_ONEHOT, basis kind): layer 1's
// weights are per-entity tables [2][V][B][d] (LayerBufs::wrel) and W_self [V,d], messages are table rows
rgcn_status onehot_forward(rgcn_ctx* c, float* out);                 // H_1 = act(dropout(W_self) + gathered table rows)
rgcn_status onehot_backward_tables(rgcn_ctx* c, const float* D);     // dW_forward, dW_backward from D = dL/dpre1
rgcn_status onehot_dcoef(rgcn_ctx* c, const float* D);               // dC_forward, dC_backward

// ---- elementwise.hip
struct CombineArgs {
  float* out;            // primary output [V,d]
  float* out2;           // optional: out * dropout(drop2)
  const float* base;     // optional [V,d] (valid for rows in [row_lo,row_hi)); dropout `drop` applies
  const float* add;      // optional [V,d] added as is
  // optional (basis kind): the compacted products [2][V][d] of the units of each direction; row v receives the rows
  // unit_ptr[dir][v] of both directions it has a unit in (GraphBufs::unit_ptr, [2][V+1])
  const float* add_units = nullptr;
  const int32_t* unit_ptr = nullptr;
  const float* msg;      // optional message rows [slots,d]; summed per CSR row
  const int32_t* row_ptr;
  const int32_t* long_rows; // rows with more than kLongRow slots (GraphBufs::long_rows / nlong)
  const int32_t* nlong;
  // giant rows (GraphBufs; all null when the cut is off)
  const int32_t* giant_rows = nullptr;
  const int32_t* giant_first = nullptr;
  const int32_t* giant_cnt = nullptr;
  const int32_t* piece_row = nullptr;
  const int32_t* piece_k = nullptr;
  const int32_t* ngiant = nullptr;
  float* giant_slab = nullptr;  // [pieces][d]
  const float* gate;     // optional: result *= (gate > 0)
  int32_t V, d;
  int32_t relu;
  int32_t row_lo, row_hi;
  int32_t v_begin = 0, v_count = -1;   // rows the launch walks: [v_begin, v_begin + v_count) (v_count < 0: all V)
  int32_t colsum = 0;    // block_rows backward: also leave the column sums of `out` as partials (rgcn_ctx::colsum_parts)
  DropSpec drop;         // applied to base
  DropSpec drop2;        // applied to out2
};
rgcn_status combine(rgcn_ctx* c, const char* tag, const CombineArgs& a, double alg_bytes);
// giant rows only: prologue + the pieces in GraphBufs' piece slab (written by the caller's own kernel) + epilogue
rgcn_status combine_giant_finish(rgcn_ctx* c, const CombineArgs& a);
// part[i][:] = out[giant_rows[i]][:] for the graph's giant rows, zeros up to giant_cap rows (column sums: block_rows.hip)
rgcn_status column_sum_giant_rows(rgcn_ctx* c, const float* out, float* part);
// out[col] = the sum of the nparts partial rows in rgcn_ctx::colsum_part (k_colsum_final's fixed order)
rgcn_status column_sum_finish(rgcn_ctx* c, float* out, int nparts, int cols);
rgcn_status input_forward(rgcn_ctx* c);                      // H0 = relu(W_emb + b_emb)
rgcn_status scale_dropout(rgcn_ctx* c, const float* in, float* out, const DropSpec& ds);
rgcn_status column_sum(rgcn_ctx* c, const float* in, float* out, int rows, int cols);
// ---- output_transform.hip: x[v][:] += b over the [rows, cols] array x, in place (the bias of the output transform)
rgcn_status add_row_bias(rgcn_ctx* c, float* x, const float* b, int rows, int cols);
rgcn_status relu_copy(rgcn_ctx* c, const float* in, float* out, int64_t n, int relu);
rgcn_status materialize_mask(rgcn_ctx* c, const DropSpec& ds, uint8_t* out_dev, int64_t n);

DropSpec make_drop(const rgcn_ctx* c, int layer, bool active);

// ---- highway.hip: the [V,d] passes of a highway context (the gate's three GEMMs are gemm_f32 calls of the schedule)
// T holds Z = H_in . W_hw on entry: T = sigmoid(Z + b), H = T * N + (1 - T) * H_in
rgcn_status highway_forward(rgcn_ctx* c, float* T, const float* b, const float* N, const float* Hin, float* H);
// D = G T relu'(N) (relu != 0), dS = D * dropout (dS != nullptr), dZ = G (N - H_in) T (1 - T), carry = G (1 - T); leaves
// *nparts column partials of dZ in colsum_scratch(c) (column_sum_finish adds them).  D may be G.
rgcn_status highway_backward(rgcn_ctx* c, const float* G, const float* T, const float* N, const float* Hin, float* D,
                             float* dS, float* dZ, float* carry, int relu, const DropSpec& drop, int* nparts);
// out += gz + carry; gate != nullptr: out *= (gate > 0) and *nparts column partials of out in colsum_scratch(c)
rgcn_status highway_join(rgcn_ctx* c, float* out, const float* gz, const float* carry, const float* gate, int* nparts);

// ---- decoder.hip / optimizer.hip
rgcn_status negative_sample(rgcn_ctx* c, const int32_t* batch_dev, int64_t n, int rate, uint64_t seed, int32_t* X,
                            float* Y);
// the same against the context's index of known positives (c->known.count > 0): negative_exclusive.h decides every row
rgcn_status negative_sample_exclusive(rgcn_ctx* c, const int32_t* batch_dev, int64_t n, int rate, uint64_t seed,
                                      int32_t* X, float* Y);
// the entity rows by one of the two calls above, then relation_rate relation corruptions of every batch row behind them
// (negative_relation.h decides every row); relation_rate > 0 clears DecoderBufs::tiled_X
rgcn_status negative_sample_relation(rgcn_ctx* c, const int32_t* batch_dev, int64_t n, int rate, int relation_rate,
                                     bool exclusive, uint64_t seed, int32_t* X, float* Y);
// the index: built on the host from validated limits (known_positives_index.h), swapped in only when complete;
// n == 0 releases it and switches the exclusive mode off
rgcn_status known_positives_reserve(rgcn_ctx* c, const int32_t* triples_host, int64_t n);
void known_positives_free(rgcn_ctx* c);
// the type sets: built on the host from validated limits (type_sets.h), swapped in only when complete; n == 0 releases
// them and switches the typed mode off
rgcn_status type_sets_reserve(rgcn_ctx* c, const int32_t* triples_host, int64_t n);
void type_sets_free(rgcn_ctx* c);
// the entity rows from the lists of the type sets (c->types.ready; negative_typed.h decides every row), exclusive against
// the index of known positives; relation_rate > 0: the relation rows of negative_sample_relation behind them
rgcn_status negative_sample_typed(rgcn_ctx* c, const int32_t* batch_dev, int64_t n, int rate, int relation_rate,
                                  bool exclusive, uint64_t seed, int32_t* X, float* Y);
// reciprocal relations (negative_reciprocal.h decides every row): the pass behind one of the sampler calls above that ran
// with the same n, rate, relation_rate and seed; X and Y hold n (rate + 2 + relation_rate) rows.  Clears tiled_X
rgcn_status reciprocal_rows(rgcn_ctx* c, const int32_t* batch_dev, int64_t n, int rate, int relation_rate, uint64_t seed,
                            int32_t* X, float* Y);
rgcn_status decoder_reserve(rgcn_ctx* c, int64_t max_triples);
void decoder_free(rgcn_ctx* c);
// N_total > N: X_dev is one rank's slice of a batch of N_total triples (relation-sharded train step); 0: N
rgcn_status decoder_prepare(rgcn_ctx* c, const int32_t* X_dev, int64_t N, int64_t N_total = 0);
// dcodes_drop / drop (optional): also write dL/dcodes * drop, the dropout-scaled copy the encoder's top layer consumes
// row_weights (optional, float [N]): a weight per row of the batch on its loss term and its dx (the weighted kernels)
rgcn_status decoder_compute(rgcn_ctx* c, const float* codes, const float* Y_dev, float reg_param,
                            float* dcodes_drop = nullptr, const DropSpec* drop = nullptr,
                            const float* row_weights = nullptr);
rgcn_status decoder_allreduce(rgcn_ctx* c);      // sharded run: sum the per-rank partial decoder results
// ---- adversarial.hip: self-adversarial weights of the decoder's negatives (adversarial_weights.h)
// w_out[i] = 1 for the P positives that lead the batch, K softmax_alpha(x) over its group for negative i of positive
// i mod P, K = N / P - 1 (N % P == 0, checked by the caller); the energies from `codes` and W_relation.  On the current
// stream; reads X only, so it needs no decoder_prepare.  Y_dev (optional): the labels, which must be 1 for the positives
// and 0 after them (error flag 128).  Ids out of range: weight 0, nothing read out of bounds.
rgcn_status adversarial_weights(rgcn_ctx* c, const float* codes, const int32_t* X_dev, const float* Y_dev, int64_t N,
                                int64_t P, float alpha, float* w_out);
rgcn_status adversarial_check_weights(rgcn_ctx* c, const float* w_dev, int64_t N);      // finite and >= 0, or error flag 256
rgcn_status adversarial_reserve(rgcn_ctx* c, int64_t rows);      // the fused steps' weight buffer (the caller has synchronised)
void adversarial_free(rgcn_ctx* c);
int adversarial_lds_cap();      // energies of one group the weight kernel keeps in LDS
rgcn_status optimizer_step(rgcn_ctx* c);
rgcn_status optimizer_norm_partial(rgcn_ctx* c);
rgcn_status optimizer_apply(rgcn_ctx* c);
// the state behind rgcn_get/set_optimizer_slot and _step: slots of the configured algorithm (Adam 2, AdaGrad 1, else 0);
// the device array of slot `slot` of parameter `param` and its element count (W_relation: RelationCount rows), created
// with its initial value if no step has yet; the [clip scale, norm, step count, rate] array, created zeroed likewise
int optimizer_slot_count(const rgcn_ctx* c);
float optimizer_slot_initial(const rgcn_ctx* c);
rgcn_status optimizer_slot(rgcn_ctx* c, int32_t param, int32_t slot, float** dev, int64_t* n);
rgcn_status optimizer_state_array(rgcn_ctx* c, float** state);
rgcn_status optimizer_fill(rgcn_ctx* c, float* dev, int64_t n, float value);
void optimizer_release_state(rgcn_ctx* c);      // another algorithm was configured: no slots, no count, the settings stay
// ---- neighborhood.hip: sample_edge_neighborhood on the device (parallel first-passage percolation)
rgcn_status neighborhood_reserve(rgcn_ctx* c, const int32_t* triples_host, int64_t n);
rgcn_status neighborhood_sample(rgcn_ctx* c, int64_t sample_size, uint64_t seed, int32_t* batch_out_dev,
                                bool on_prefetch_stream);
void neighborhood_free(rgcn_ctx* c);
// ---- ranking.hip
rgcn_status rank_reserve(rgcn_ctx* c, int64_t max_queries);
void rank_free(rgcn_ctx* c);
// the five entity-side query calls: one scoring path (run_queries) and the call's own tail; each synchronises and returns
// the verdict
rgcn_status rank_compute(rgcn_ctx* c, const int32_t* X_dev, int64_t N, int predict_object, const int64_t* filt_ptr,
                         const int32_t* filt_idx, int32_t* raw_out, int32_t* filt_out);
rgcn_status rank_mixed_compute(rgcn_ctx* c, const int32_t* X_dev, int64_t N, int predict_object, const float* partner_dev,
                               float weight, const int64_t* filt_ptr, const int32_t* filt_idx, int32_t* raw_out,
                               int32_t* filt_out);
rgcn_status topk_compute(rgcn_ctx* c, const int32_t* X_dev, int64_t N, int predict_object, int k,
                         const int64_t* excl_ptr, const int32_t* excl_idx, int32_t* idx_out, float* energy_out);
rgcn_status score_queries_compute(rgcn_ctx* c, const int32_t* X_dev, int64_t N, int predict_object);
rgcn_status topk_mixed_compute(rgcn_ctx* c, const int32_t* X_dev, int64_t N, int predict_object, int k,
                               const float* partner_dev, float weight, const int64_t* excl_ptr, const int32_t* excl_idx,
                               int32_t* idx_out, float* score_out);
// the relation forms of rank, top-k and score: the same path, the candidates are the R relations of the pair (s, o) and
// their energies land in ranking.rel (allocated by the first of these calls after a growing rank_reserve)
rgcn_status rank_relation_compute(rgcn_ctx* c, const int32_t* X_dev, int64_t N, const int64_t* filt_ptr,
                                  const int32_t* filt_idx, int32_t* raw_out, int32_t* filt_out);
rgcn_status topk_relation_compute(rgcn_ctx* c, const int32_t* X_dev, int64_t N, int k, const int64_t* excl_ptr,
                                  const int32_t* excl_idx, int32_t* idx_out, float* energy_out);
rgcn_status score_relation_queries_compute(rgcn_ctx* c, const int32_t* X_dev, int64_t N);
// the type-constrained forms of rank_compute and topk_compute (c->types.ready): the candidates of a row are the members
// of list (predict_object, r), and for the ranks the gold entity
rgcn_status rank_typed_compute(rgcn_ctx* c, const int32_t* X_dev, int64_t N, int predict_object, const int64_t* filt_ptr,
                               const int32_t* filt_idx, int32_t* raw_out, int32_t* filt_out);
rgcn_status topk_typed_compute(rgcn_ctx* c, const int32_t* X_dev, int64_t N, int predict_object, int k,
                               const int64_t* excl_ptr, const int32_t* excl_idx, int32_t* idx_out, float* energy_out);
void optimizer_free(rgcn_ctx* c);
// ---- relation_softmax.hip: the softmax-over-relations loss term of the positives (s, r, o) of a step
rgcn_status relation_softmax_reserve(rgcn_ctx* c, int64_t max_positives);
void relation_softmax_free(rgcn_ctx* c);
// adds weight / P * sum_n ell_n to dec.loss and its gradients to dcodes_own and to W_relation's gradient, on the current
// stream, which must be behind the decoder's kernels on every stream; the last chunk's relation gradient is left on side
// stream 2 (stream_join(c, 2) before anything reads W_relation's gradient or calls this again).  Y_dev (optional): the labels of the rows, which
// must all be 1 (error flag 64).  exclusive: relations known for the pair leave the candidate set (c->known)
// the by-entity CSR of the first chunk of these positives, on the current stream (depends on X only)
rgcn_status relation_softmax_prepare(rgcn_ctx* c, const int32_t* pos_dev, int64_t P);
rgcn_status relation_softmax_compute(rgcn_ctx* c, const float* codes, const int32_t* pos_dev, const float* Y_dev, int64_t P,
                                     float weight, bool exclusive);
// ---- entity_softmax.hip: the softmax-over-entities loss term of the positives (s, r, o) of a step
rgcn_status entity_softmax_reserve(rgcn_ctx* c, int64_t max_positives);
void entity_softmax_free(rgcn_ctx* c);
// adds weight / (2 P) * sum_m ell_m to dec.loss and its gradients to dcodes_own and to W_relation's gradient, all on the
// current stream, which must be behind the decoder's kernels (and the relation-softmax term's) on every stream.  Y_dev
// (optional): the labels of the rows, which must all be 1 (error flag 64).  exclusive: entities known for the row's
// pair leave its candidate set (c->known, both orders)
rgcn_status entity_softmax_compute(rgcn_ctx* c, const float* codes, const int32_t* pos_dev, const float* Y_dev, int64_t P,
                                   float weight, bool exclusive);

// ---- comm.cpp (RCCL via dlopen)
rgcn_status comm_unique_id(uint8_t id[128]);
rgcn_status comm_init(rgcn_ctx* c, const uint8_t id[128]);
rgcn_status comm_allreduce(rgcn_ctx* c, float* buf, int64_t count);
rgcn_status comm_reduce_scatter(rgcn_ctx* c, float* buf, int64_t count_per_rank);
rgcn_status comm_all_gather(rgcn_ctx* c, float* buf, int64_t count_per_rank);
rgcn_status comm_info(rgcn_ctx* c, int32_t* ranks, int32_t* rank, int32_t* device);
void comm_destroy(rgcn_ctx* c);

}  // namespace rgcn
