// The per-layer orchestration of the encoder: which kernel goes to which stream, in which order.
//   forward  (MessageGcn.compute_vertex_embeddings, code/encoders/message_gcns/message_gcn.py:49-79)
//   backward (tf.gradients(loss, weights), code/optimization/abstract.py:117-118; formulas SURVEY 8a a15)
// The forward pass of a block step is one chain on the main stream: [self-loop GEMM -> row kernel] x L.  H0 = relu(W_emb +
// b_emb) is formed by layer 1's self-loop GEMM on load and written back by it where that GEMM has the A-operand prologue
// (h0_by_self_loop_gemm below: the GEMM's plan says so); everywhere else k_input_fwd opens the chain.
// One schedule per situation: minibatch scale on one GPU with side streams, the chain a captured
// step records, full-graph scale / a relation-sharded run (the exchange points of DESIGN.md section 7).  The C ABI that
// drives these functions is rgcn_api.hip.
#include "rgcn_api_internal.h"

namespace rgcn {

// ---------------------------------------------------------------- forward
static bool h0_by_self_loop_gemm(const rgcn_ctx* c);

rgcn_status fwd_begin(rgcn_ctx* c, int train, uint64_t seed, const uint8_t* masks_host) {
  RGCN_NO_EMBEDDING(c, "rgcn_forward_begin");      // (rgcn_forward / rgcn_backward never come here on such a context)
  if (!c->g.ready) RGCN_FAIL(c, RGCN_ERR_STATE, "rgcn_forward before rgcn_set_graph");
  // (side kernels the main stream has not joined -- a step that ended unjoined, rgcn_step_device; a backward pass driven
  // layer by layer and abandoned between layers 2 and 1 -- read the activations this pass overwrites.  Nothing is queued
  // where the last pass ended joined, or where step_begin took this wait together with the prefetched graph's.)
  RGCN_TRY(join_side_reads(c));
  c->fwd_done = false;
  c->frag_fresh = false;
  c->wtile_fresh = false;
  c->fwd_train = train ? 1 : 0;
  c->seed = seed;
  c->explicit_masks = false;
  if (train && masks_host) {
    const size_t n = (size_t)c->L * c->V * c->d;
    if (!c->masks) RGCN_TRY(dmalloc(c, c->pool, &c->masks, n, false));
    RGCN_TRY(to_dev(c, c->masks, masks_host, n));
    c->explicit_masks = true;
  }
  if (c->onehot) return RGCN_OK;      // no AffineTransform under the layers: layer 1 reads entity ids (basis_onehot.hip)
  // H0 = relu(W_emb + b_emb): a pass of its own (k_input_fwd), or -- where layer 1's self-loop product runs on a kernel with
  // the A-operand prologue and nothing reads H0 before the row kernel behind that product -- formed by that product on load
  // and written back by it (fwd_layer_partial).  The wait above precedes either: both overwrite H0.
  c->h0_in_gemm = h0_by_self_loop_gemm(c);
  if (c->h0_in_gemm) return RGCN_OK;
  return input_forward(c);
}

// The all-gather of the rows finished last runs on side stream 1; whoever needs ALL rows (message kernels, the
// decoder, the column sums) makes its stream wait here, whoever needs the rank's own rows only (self-loop GEMMs) does not.
static rgcn_status wait_gather(rgcn_ctx* c) {
  if (c->gather_pending) {
    RGCN_HIP(c, hipStreamWaitEvent(c->stream, c->ev_gather, 0));
    if (c->stream == c->main_stream) c->gather_pending = false;
  }
  return RGCN_OK;
}
// all-gather the [V_pad,d] buffer whose own rows this rank just finished, beside whatever the main stream does next
static rgcn_status gather_rows(rgcn_ctx* c, float* buf) {
  StreamScope side(c, 1);
  RGCN_TRY(comm_all_gather(c, buf, (int64_t)c->shard_rows * c->d));
  if (side.active) {
    RGCN_HIP(c, hipEventRecord(c->ev_gather, c->aux[1]));
    c->gather_pending = true;
  }
  return RGCN_OK;
}

// The block layer destination-major in ONE pass over the incidence CSR, one column band per XCD, weights through L2
// (block_rows.hip): block kind, any world.  Otherwise (rgcn_set_fusion 0, or more blocks than the kernel's lane groups
// cover) the two-kernel form: relation-major message kernel + k_combine.
static bool rows_layer(const rgcn_ctx* c) { return c->fuse == 1 && block_rows_available(c); }

// Fragment tables of the weights that are the B operand of a contraction (W_self of every layer in both orientations, the
// basis tensors), rebuilt -- all of them, one launch -- when the weights changed (set_param, Adam) and once inside every
// captured step, whose replays follow weights the host does not see.  Nothing to do when the dense contractions run on
// the fp32 MFMA (no split, nothing to pre-split).
static rgcn_status refresh_weight_fragments(rgcn_ctx* c) {
  if (c->gemm_mode == 0) return RGCN_OK;
  if (c->capturing ? c->frag_fresh : c->frag_version == c->weights_version) return RGCN_OK;
  std::vector<PresplitJob> jobs;
  const int d = c->d, Bd = c->B * c->d;
  for (int l = 1; l <= c->L; ++l) {
    LayerBufs& lb = c->layers[l];
    if (!lb.wself_nn || !lb.wself_nt) continue;
    jobs.push_back(PresplitJob{lb.wself, lb.wself_nn, d, d, d, 0});      // H . W_self:      B (k, n) = W[k][n]
    jobs.push_back(PresplitJob{lb.wself, lb.wself_nt, d, d, d, 1});      // dS . W_self^T:   B (k, n) = W[n][k]
    if ((c->kind == RGCN_KIND_BASIS || c->kind == RGCN_KIND_BASIS_PDIAG) && lb.wrel_nn && lb.wrel_nt)
      for (int g = 0; g < 2; ++g) {
        const float* W = lb.wrel + (size_t)g * Bd * d;                   // W'_dir [B.d, d]
        jobs.push_back(PresplitJob{W, static_cast<char*>(lb.wrel_nn) + 16 * g * gemm_bfrag_words(Bd, d), d, Bd, d, 0});
        jobs.push_back(PresplitJob{W, static_cast<char*>(lb.wrel_nt) + 16 * g * gemm_bfrag_words(d, Bd), d, d, Bd, 1});
      }
  }
  if (c->out_layer) jobs.push_back(PresplitJob{c->w_out, c->wout_nn, c->dc, d, c->dc, 0});      // H_L . W_out: B (k, n) = W[k][n]
  if (!jobs.empty()) RGCN_TRY(gemm_presplit_b(c, jobs.data(), (int)jobs.size()));
  c->frag_fresh = true;
  c->frag_version = c->capturing ? ~0ull : c->weights_version;
  return RGCN_OK;
}
// the rows whose self-loop term and epilogue this rank owns: its shard of a sharded run, every row on one GPU
struct RowShard { int lo, hi; };
static RowShard row_shard(const rgcn_ctx* c) { return c->world > 1 ? RowShard{c->row_lo, c->row_hi} : RowShard{0, c->V}; }

// the self-loop products: one group, W_self as the pre-split B operand (forward: [k][n]; dH: used transposed, [n][k]);
// whoever launches one refreshes the fragment tables first
static GemmBatch self_loop_batch(const rgcn_ctx* c, int l, bool transposed) {
  GemmBatch b;
  if (c->gemm_mode != 0) b.bfrag = transposed ? c->layers[l].wself_nt : c->layers[l].wself_nn;
  b.wide = transposed ? 0 : 1;
  return b;
}
// S = H_{l-1} . W_self of layer l over this rank's row shard; form_h0 (layer 1): W_emb is the A operand and the product
// forms H0 = relu(W_emb + b_emb) on load and writes it back (GemmBatch::a_bias / a_out)
static GemmCall self_fwd_call(const rgcn_ctx* c, int l, bool form_h0) {
  const int d = c->d, lo = row_shard(c).lo, hi = row_shard(c).hi;
  GemmCall q{true, false, hi - lo, d, d, (form_h0 ? c->w_emb : c->H[l - 1]) + (size_t)lo * d, d, c->layers[l].wself, d,
             c->self_buf + (size_t)lo * d, d, 1, c->slab, self_loop_batch(c, l, false)};
  if (form_h0) {
    q.batch.a_bias = c->b_emb;
    q.batch.a_out = c->H[0];
  }
  return q;
}
// Layer 1's self-loop product takes W_emb as its A operand and forms H0 itself (GemmBatch::a_bias / a_out): the single-pass
// block layer on one GPU with the split arithmetic, where the GEMM is the first reader of H0 and the row kernel behind it
// the second.  Everywhere else -- the basis kind (the aggregation reads H0 beside the GEMM), the two-kernel block form (so
// does the message kernel), a sharded run, the fp32-MFMA mode, a shape the pre-split-weight kernels do not take -- H0 stays
// k_input_fwd's.  Devtools knob RGCN_H0_IN_GEMM = 0: the separate pass everywhere (the A/B, the bitwise tests).
constexpr int kH0InGemmDefault = 1;
static bool h0_by_self_loop_gemm(const rgcn_ctx* c) {
  if (knob("RGCN_H0_IN_GEMM", kH0InGemmDefault) == 0) return false;
  if (c->onehot || c->world != 1 || c->kind != RGCN_KIND_BLOCK || !rows_layer(c) || c->L < 1) return false;
  return gemm_plan(self_fwd_call(c, 1, true), c->gemm_mode, 1).prologue;      // (both pre-split kernels have it: any knob)
}

// Basis kind: the two direction groups of a batched GEMM over the (row, direction) units of the current graph; the
// group's extent (rows of A / C, or the depth of dW') is the direction's unit count, read on the device.
static GemmBatch basis_batch(const rgcn_ctx* c, size_t strideA, size_t strideB, size_t strideC, bool limit_on_k) {
  GemmBatch b;
  b.groups = 2;
  b.strideA = strideA; b.strideB = strideB; b.strideC = strideC;
  b.limit = c->g.unit_ptr + c->V;
  b.limit_stride = c->V + 1;
  b.limit_on_k = limit_on_k ? 1 : 0;
  return b;
}
static double basis_unit_share(rgcn_ctx* c) { return basis_units(c) / (2.0 * c->V); }

// BASIS_TDIAG: the two direction groups of a batched GEMM -- H (or its transpose) is the A operand of both, W_dir / dP_dir
// the B operand, P_dir / dW_dir the product
static GemmBatch tdiag_batch(size_t strideA, size_t strideB, size_t strideC) {
  GemmBatch b;
  b.groups = 2;
  b.strideA = strideA; b.strideB = strideB; b.strideC = strideC;
  return b;
}

// The three batched GEMMs over the (row, direction) units that the basis and the BASIS_PDIAG layer share (LayerBufs::wrel of
// the latter holds the two groups swapped: forward units x W_backward).  Whoever launches one has refreshed the fragment
// tables (fwd_layer_partial, bwd_layer_partial).
// forward: aggbuf[dir] = Zc_dir . W'_dir   ([units, B.d] x [B.d, d], two groups)
static rgcn_status units_product_fwd(rgcn_ctx* c, int l) {
  const int d = c->d, V = c->V, Bd = c->B * d;
  GemmBatch gb = basis_batch(c, (size_t)V * Bd, (size_t)Bd * d, (size_t)V * d, false);
  if (c->gemm_mode != 0) gb.bfrag = c->layers[l].wrel_nn;
  gb.strideBfrag = gemm_bfrag_words(Bd, d);
  gb.wide = 1;
  return gemm_f32(c, "gemm_basis_fwd", true, false, V, d, Bd, c->zsave[l], Bd, c->layers[l].wrel, d,
                  c->aggbuf, d, 1, &gb, basis_unit_share(c));
}
// dW'_dir = Zc_dir^T . Dc_dir   ([B.d, units] x [units, d], split over the units; two groups); Dc: the upstream rows of the
// units in aggbuf (basis_gather_units)
static rgcn_status units_product_dw(rgcn_ctx* c, int l) {
  const int d = c->d, V = c->V, Bd = c->B * d;
  const GemmBatch gk = basis_batch(c, (size_t)V * Bd, (size_t)V * d, (size_t)Bd * d, true);
  return gemm_f32(c, "gemm_basis_dw", false, false, Bd, d, V, c->zsave[l], Bd, c->aggbuf, d, c->layers[l].grel, d,
                  auto_split_k(2 * Bd, d, V), &gk, basis_unit_share(c));
}
// dZc_dir = Dc_dir . W'_dir^T   ([units, d] x [d, B.d], two groups), into msgbuf2
static rgcn_status units_product_dz(rgcn_ctx* c, int l) {
  const int d = c->d, V = c->V, Bd = c->B * d;
  GemmBatch gm = basis_batch(c, (size_t)V * d, (size_t)Bd * d, (size_t)V * Bd, false);
  if (c->gemm_mode != 0) gm.bfrag = c->layers[l].wrel_nt;
  gm.strideBfrag = gemm_bfrag_words(d, Bd);
  return gemm_f32(c, "gemm_basis_dz", true, true, V, Bd, d, c->aggbuf, d, c->layers[l].wrel, d, c->msgbuf2, Bd, 1, &gm,
                  basis_unit_share(c));
}

// The six forms a layer takes; fwd_layer_partial and bwd_layer_partial run one function each per form.
enum LayerForm { FORM_ONEHOT, FORM_BLOCK_ROWS, FORM_BLOCK_TWO_KERNEL, FORM_BASIS, FORM_TDIAG, FORM_PDIAG };
static LayerForm layer_form(const rgcn_ctx* c, int l) {
  if (c->onehot && l == 1) return FORM_ONEHOT;
  if (c->kind == RGCN_KIND_BLOCK) return rows_layer(c) ? FORM_BLOCK_ROWS : FORM_BLOCK_TWO_KERNEL;
  if (c->kind == RGCN_KIND_BASIS_TDIAG) return FORM_TDIAG;
  return c->kind == RGCN_KIND_BASIS_PDIAG ? FORM_PDIAG : FORM_BASIS;
}

// the forward epilogue every form but the one-hot first layer ends with: dst = relu?(dropout(S) + the form's own terms) over
// this rank's rows (a sharded run leaves the PARTIAL pre-activations, no relu, for the reduce-scatter that follows)
static CombineArgs fwd_epilogue_args(rgcn_ctx* c, int l, float* dst) {
  CombineArgs a;
  a.add = nullptr; a.msg = nullptr; a.row_ptr = nullptr; a.long_rows = nullptr; a.nlong = nullptr;
  a.out = dst; a.out2 = nullptr; a.base = c->self_buf; a.gate = nullptr; a.V = c->V; a.d = c->d;
  a.relu = (c->world == 1 && l < c->L) ? 1 : 0;
  a.row_lo = row_shard(c).lo; a.row_hi = row_shard(c).hi;
  a.drop = make_drop(c, l, true);
  a.drop2 = make_drop(c, l, false);
  return a;
}

// self: S = H . W_self over the rows of this rank's shard (self_fwd_call); dst: where the layer's result goes
static rgcn_status fwd_block_rows(rgcn_ctx* c, int l, const GemmCall& self, float* dst) {
  // S = H . W_self, then ONE kernel: H' = relu(dropout(S) + sum over the row's messages of n W_r H[src]) straight from
  // the incidence CSR (no message buffer)
  // (sharded run: the self-loop GEMM covers this rank's row shard, the kernel walks the rank's own messages and writes
  // the PARTIAL pre-activations -- the self-loop term inside the shard only, no relu -- for the reduce-scatter that
  // follows)
  RGCN_TRY(gemm_f32(c, "gemm_self_fwd", self));
  RGCN_TRY(wait_gather(c));
  return block_rows(c, "block_rows_fwd", l, false, c->H[l - 1], fwd_epilogue_args(c, l, dst));
}

static rgcn_status fwd_block_two_kernel(rgcn_ctx* c, int l, const GemmCall& self, float* dst) {
  const int d = c->d, V = c->V;
  const double Mmsg = 2.0 * c->g.E / c->world;
  // Two-kernel form.  The relational messages (HBM-bound) run beside the self-loop GEMM.  A stream that blocks on
  // another stream's event resumes ~10 us after the event fires, so the chain that continues (the combine) stays on
  // the stream of the kernel that finishes LAST: the messages on the main stream, the (shorter) GEMM forked.
  {
    StreamScope side(c, 0);
    RGCN_TRY(gemm_f32(c, "gemm_self_fwd", self));
  }
  RGCN_TRY(wait_gather(c));
  RGCN_TRY(block_msg_forward(c, l, c->H[l - 1], c->msgbuf));
  RGCN_TRY(stream_join(c, 0));
  CombineArgs a = fwd_epilogue_args(c, l, dst);
  a.msg = c->g.E > 0 ? c->msgbuf : nullptr;
  a.row_ptr = c->g.row_ptr; a.long_rows = c->g.long_rows; a.nlong = c->g.nlong;
  return combine(c, "combine_fwd", a, 4.0 * d * (2.0 * V + Mmsg) + 4.0 * V);
}

static rgcn_status fwd_tdiag(rgcn_ctx* c, int l, const GemmCall& self, float* dst) {
  // transform first (basis_tdiag.hip): P_dir = H . W_dir.reshape(d, B.d), two groups of one batched GEMM over the same
  // A operand, kept per layer for dC; the self-loop product beside it on side stream 1; then ONE destination-major
  // kernel: H' = relu(dropout(S) + sum over the row's messages of n sum_b G[rel,b,:] P_dir[src,b,:] + b)
  const int d = c->d, V = c->V, Bd = c->B * d;
  RGCN_TRY(tdiag_refresh_gates(c, l));
  {
    StreamScope side(c, 1);
    RGCN_TRY(gemm_f32(c, "gemm_self_fwd", self));
  }
  const GemmBatch gb = tdiag_batch(0, (size_t)d * Bd, (size_t)V * Bd);
  RGCN_TRY(gemm_f32(c, "gemm_tdiag_fwd", true, false, V, Bd, d, c->H[l - 1], d, c->layers[l].wrel, Bd, c->tdiag_P[l], Bd, 1, &gb));
  RGCN_TRY(stream_join(c, 1));
  return tdiag_rows_forward(c, l, c->tdiag_P[l], fwd_epilogue_args(c, l, dst));
}

static rgcn_status fwd_pdiag(rgcn_ctx* c, int l, const GemmCall& self, float* dst) {
  // basis_pdiag.hip: ONE destination-major walk forms the mixing table a_l, the diagonal aggregate and the rows' own unit
  // rows Zc[(v,dir),b,:] = a_dir[v,b] H[v,:]; Zc . W' is the basis kind's batched product over the units (LayerBufs::wrel
  // holds the two groups swapped: forward units x W_backward); the self-loop product beside both on side stream 1; then
  // H' = relu(dropout(S) + the two unit products + aggregate + b)
  {
    StreamScope side(c, 1);
    RGCN_TRY(gemm_f32(c, "gemm_self_fwd", self));
  }
  RGCN_TRY(pdiag_rows_forward(c, l, c->H[l - 1], c->zsave[l], c->pdiag_a[l], c->pdiag_agg));
  RGCN_TRY(units_product_fwd(c, l));
  RGCN_TRY(stream_join(c, 1));
  return pdiag_epilogue(c, l, c->aggbuf, c->pdiag_agg, fwd_epilogue_args(c, l, dst));
}

static rgcn_status fwd_basis(rgcn_ctx* c, int l, const GemmCall& self, float* dst) {
  // aggregate first, per (row, direction) unit: Zc[(v,dir),b,:] = sum n C[rel,b] H[src];
  // pre[v] = dropout(H.W_self)[v] + sum_dir Zc[(v,dir)] . W'_dir  -- two groups of one batched GEMM over the units
  const int d = c->d, V = c->V;
  // the self-loop GEMM needs the layer input only: it runs on side stream 1 beside the aggregation (HBM-bound) and
  // then beside the basis GEMM
  {
    StreamScope side(c, 1);
    RGCN_TRY(gemm_f32(c, "gemm_self_fwd", self));
  }
  RGCN_TRY(wait_gather(c));
  RGCN_TRY(basis_aggregate_forward(c, l, c->H[l - 1], c->zsave[l]));
  RGCN_TRY(units_product_fwd(c, l));
  RGCN_TRY(stream_join(c, 1));
  CombineArgs a = fwd_epilogue_args(c, l, dst);
  a.add_units = c->aggbuf; a.unit_ptr = c->g.unit_ptr;
  return combine(c, "combine_fwd", a, 4.0 * d * (2.0 * V + 2.0 * V * basis_unit_share(c)) + 8.0 * V);
}

rgcn_status fwd_layer_partial(rgcn_ctx* c, int l) {
  RGCN_NO_EMBEDDING(c, "rgcn_forward_layer_partial");
  if (l < 1 || l > c->L) RGCN_FAIL(c, RGCN_ERR_INVALID, "layer out of range");
  const LayerForm form = layer_form(c, l);
  // featureless first layer (world == 1): one destination-major kernel, messages looked up in the [V,B,d] tables, the
  // combine -- W_self row, dropout, relu -- as its epilogue; no GEMM
  if (form == FORM_ONEHOT) return onehot_forward(c, c->H[1]);
  // highway context: the layer's result is N_l; fwd_layer_finish forms H_l from it
  float* dst = c->world > 1 ? c->exch : c->highway ? c->hw_N[l] : c->H[l];
  RGCN_TRY(refresh_weight_fragments(c));
  bool form_h0 = false;
  if (l == 1 && c->h0_in_gemm) {
    // fwd_begin left H0 to this layer's self-loop product.  If the product can still form it (nothing switched the layer's
    // form or the arithmetic since), it reads W_emb and writes H0 = relu(W_emb + b_emb) on the way; otherwise the pass runs now.
    c->h0_in_gemm = false;
    form_h0 = h0_by_self_loop_gemm(c);
    if (!form_h0) RGCN_TRY(input_forward(c));
  }
  const GemmCall self = self_fwd_call(c, l, form_h0);      // S = H . W_self  (rows of this rank's shard)
  switch (form) {
    case FORM_BLOCK_ROWS: return fwd_block_rows(c, l, self, dst);
    case FORM_BLOCK_TWO_KERNEL: return fwd_block_two_kernel(c, l, self, dst);
    case FORM_TDIAG: return fwd_tdiag(c, l, self, dst);
    case FORM_PDIAG: return fwd_pdiag(c, l, self, dst);
    default: return fwd_basis(c, l, self, dst);
  }
}

// The output transform (output_transform.hip), the tail of the forward pass whatever the layer kind: codes = H_L . W_out +
// b_out -- the product with W_out as the pre-split B operand, wide like the other forward products, then the bias in place.
// No dropout: train and test mode run the same two launches.
static rgcn_status output_forward(rgcn_ctx* c) {
  const int d = c->d, dc = c->dc, V = c->V;
  RGCN_TRY(refresh_weight_fragments(c));      // (a one-hot single-layer stack launches no other product)
  GemmBatch b;
  if (c->gemm_mode != 0) b.bfrag = c->wout_nn;
  b.wide = 1;
  RGCN_TRY(gemm_f32(c, "gemm_out_fwd", true, false, V, dc, d, c->H[c->L], d, c->w_out, dc, c->codes, dc, 1, &b));
  return add_row_bias(c, c->codes, c->b_out, V, dc);
}

// The layer's backward pass, ahead of the stack's (bwd_begin): three launches on the main stream, in this order --
//   out_dh  = dcodes . W_out^T     (NT; what the layer stack takes for its dcodes)
//   g_W_out = H_L^T . dcodes       (TN, split-K)
//   g_b_out = the column sums of dcodes
static rgcn_status output_backward(rgcn_ctx* c, const float* dcodes) {
  const int d = c->d, dc = c->dc, V = c->V;
  RGCN_TRY(gemm_f32(c, "gemm_out_dh", true, true, V, d, dc, dcodes, dc, c->w_out, dc, c->out_dh, d, 1));
  RGCN_TRY(gemm_f32(c, "gemm_out_dw", false, false, d, dc, V, c->H[c->L], d, dcodes, dc, c->g_w_out, dc,
                    auto_split_k(d, dc, V)));
  RGCN_TRY(column_sum(c, dcodes, c->g_b_out, V, dc));
  c->out_dh_valid = true;
  return RGCN_OK;
}

rgcn_status fwd_layer_finish(rgcn_ctx* c, int l) {
  RGCN_NO_EMBEDDING(c, "rgcn_forward_layer_finish");
  if (l < 1 || l > c->L) RGCN_FAIL(c, RGCN_ERR_INVALID, "layer out of range");
  if (c->world > 1)
    RGCN_TRY(relu_copy(c, c->exch, c->H[l], (int64_t)c->V * c->d, l < c->L ? 1 : 0));
  if (c->highway) {
    // T_l = sigmoid(H_{l-1} . W_hw + b_hw), H_l = T_l N_l + (1 - T_l) H_{l-1}: the gate product lands in T_l's buffer and
    // the pass turns it into T_l in place.  W_hw has no fragment table: the plan picks a kernel that splits it per tile.
    const int d = c->d;
    RGCN_TRY(gemm_f32(c, "gemm_highway_fwd", true, false, c->V, d, d, c->H[l - 1], d, c->layers[l].whw, d, c->hw_T[l], d, 1));
    RGCN_TRY(highway_forward(c, c->hw_T[l], c->layers[l].bhw, c->hw_N[l], c->H[l - 1], c->H[l]));
    c->hw_last = l;
  }
  if (c->kind == RGCN_KIND_BASIS_TDIAG) c->tdiag_last = l;
  if (c->kind == RGCN_KIND_BASIS_PDIAG) c->pdiag_last = l;
  if (l == c->L && c->out_layer) RGCN_TRY(output_forward(c));
  if (l == c->L) c->fwd_done = true;
  return RGCN_OK;
}

// ---------------------------------------------------------------- backward
// The schedule whose end-of-pass joins may be deferred (rgcn_ctx::defer_end_joins): the single-pass block layer at
// minibatch scale on one GPU with the side streams on, outside a capture, two layers or more (bwd_block_rows' first
// branch).  In that schedule dW_self always runs on side stream 1 and the relation-weight kernels on side stream 0, so a
// pass that starts while the previous one's side kernels are unjoined queues its own behind them IN STREAM ORDER: the
// slabs and the gradients they share need no event.
static bool deferred_schedule(const rgcn_ctx* c) {
  return !c->highway && !c->out_layer && c->defer_end_joins && c->kind == RGCN_KIND_BLOCK && c->fuse == 1 && block_rows_available(c) && c->world == 1 &&
         c->g.E <= 65536 && c->use_aux && !c->capturing && c->L >= 2 && c->stream == c->main_stream;
}

// ds_ready: dcodes * dropout of the top layer, already written by the producer of dcodes (the device decoder does,
// inside a train step): the scale-and-copy pass over [V,d] is skipped
rgcn_status bwd_begin(rgcn_ctx* c, const float* dcodes_dev, const float* ds_ready) {
  RGCN_NO_EMBEDDING(c, "rgcn_backward_begin");
  if (!c->fwd_done) RGCN_FAIL(c, RGCN_ERR_STATE, "rgcn_backward needs a completed rgcn_forward on the current graph");
  if (!dcodes_dev) RGCN_FAIL(c, RGCN_ERR_INVALID, "dcodes is NULL");
  // Unjoined side kernels read the dS / D buffers this pass rewrites and write the gradients, slabs and column-sum partials
  // it writes: the full join -- except from one deferred step to the next.  There the forward pass has waited for every side
  // kernel that reads (SIDE_READS_JOINED), this pass's side kernels follow the pending ones in stream order, and its
  // column-sum partials go to the other half of the scratch (bwd_end): the main stream waits for nothing.
  if (!(c->side_state == rgcn_ctx::SIDE_READS_JOINED && deferred_schedule(c))) RGCN_TRY(join_abandoned_side_work(c));
  if (c->out_layer) {
    // the output transform first; the pass then continues with dL/dH_L in the place of dcodes (a ready-made dS would be a
    // dropout copy of the [V,dc] dcodes: of no use)
    RGCN_TRY(output_backward(c, dcodes_dev));
    dcodes_dev = c->out_dh;
    ds_ready = nullptr;
  }
  c->bwd_layer = c->L;
  c->bwd_D = dcodes_dev;
  if (c->highway) {      // dcodes is G_L; D_L and dS_L are the highway pass's (bwd_layer_partial), a ready-made dS is of no use
    c->bwd_dS = nullptr;
    return RGCN_OK;
  }
  DropSpec ds = make_drop(c, c->L, true);
  if (ds.mode != DROP_NONE && ds_ready != nullptr) {
    c->bwd_dS = ds_ready;
  } else if (ds.mode != DROP_NONE) {
    RGCN_TRY(scale_dropout(c, dcodes_dev, c->dsbuf[c->L & 1], ds));
    c->bwd_dS = c->dsbuf[c->L & 1];
  } else {
    c->bwd_dS = dcodes_dev;
  }
  return RGCN_OK;
}

// What the forms of a backward layer share (bwd_layer_partial fills it in): the layer and its input, this rank's row shard,
// the split rule of the weight gradients, and the epilogue
// (self-loop gradient + relational gradient) -> relu' -> next D / dS.
struct BwdLayer {
  int l;
  const float* Hin;
  LayerBufs* lb;
  int lo, rows;
  bool narrow_dw;      // (see auto_split_k)
  CombineArgs a;
};
// the dense pieces every form but the one-hot first layer is made of; whoever launches self_dh has refreshed the fragment tables
static rgcn_status self_dw(rgcn_ctx* c, const BwdLayer& s) {      // dW_self = H_in^T . dS   (split-K)
  const int d = c->d;
  return gemm_f32(c, "gemm_self_dw", false, false, d, d, s.rows, s.Hin + (size_t)s.lo * d, d, c->bwd_dS + (size_t)s.lo * d, d,
                  s.lb->gwself, d, auto_split_k(d, d, s.rows, s.narrow_dw));
}
static rgcn_status self_dh(rgcn_ctx* c, const BwdLayer& s) {      // G = dS . W_self^T
  const int d = c->d;
  const GemmBatch sbt = self_loop_batch(c, s.l, true);
  return gemm_f32(c, "gemm_self_dh", true, true, s.rows, d, d, c->bwd_dS + (size_t)s.lo * d, d, s.lb->wself, d,
                  c->self_buf + (size_t)s.lo * d, d, 1, &sbt);
}

static rgcn_status bwd_onehot(rgcn_ctx* c) {
  // Featureless first layer: D = dL/dpre1 (the layer above applied relu'(H_1); L = 1: the codes' gradient), dS = D *
  // dropout_1.  Nothing lies below, so there is no dH -- no self-loop GEMMs, no relu' of an H_0, no column sums:
  //   dW_self = dS (a copy), the tables' gradient source-major, the coefficients' per relation chunk.
  // The coefficient kernel reads the tables and D, the table kernel writes the tables' gradient: independent, the former
  // on side stream 0 beside the latter (which is bound by its 2 V B d writes).
  {
    StreamScope side(c, 0);
    RGCN_TRY(onehot_dcoef(c, c->bwd_D));
  }
  RGCN_TRY(relu_copy(c, c->bwd_dS, c->layers[1].gwself, (int64_t)c->V * c->d, 0));
  RGCN_TRY(onehot_backward_tables(c, c->bwd_D));
  return stream_join(c, 0);
}

// *defer_joins: the layer leaves its side kernels unjoined (bwd_layer_partial then skips its own join of side stream 1)
static rgcn_status bwd_block_rows(rgcn_ctx* c, const BwdLayer& s, bool* defer_joins) {
  // Row gradients: the single-pass kernel behind G = dS . W_self^T.  Relation-weight gradients (dW_r = sum n g (x) x,
  // relation-major, two row gathers per message): k_block_msg_bwd<dW only> + its slab reduce.  ONE schedule per
  // situation, each the measured best of round 4's A/Bs (profiles/r04_rowmajor_spmm_ab.md, r04_block_forms_ab.txt):
  //   minibatch scale, one GPU, side streams on:  dW_self forked BEFORE dH is launched (MFMA beside MFMA: the second
  //       GEMM fills the slots the first leaves idle, 456 workgroups on 512, and its tail), the relation-weight kernels
  //       forked BEHIND dH, beside the row-gradient kernel (two gather kernels share the chip better than either does
  //       with a GEMM), joined at the end of the layer: 0.553-0.556 ms per step against 0.597-0.599 as a chain (round 5,
  //       same box: dW_self forked BEHIND dH instead, beside the row-gradient kernel: 0.567-0.578 against 0.541-0.547);
  //   the same inside a capture (a captured step is a chain, rgcn_capture_begin) or with the side streams off: the
  //       chain, with the one fork a replayed graph gains from -- the slab reduce + dW_self beside dH;
  //   full-graph scale or a sharded run: the relation-weight kernels on side stream 0 from the start of the layer
  //       (at 272,115 edges they are five GEMMs long; a sharded run's all-gather rides on side stream 1), joined
  //       before the next layer overwrites D.
  const bool minibatch = c->world == 1 && c->g.E <= 65536;
  if (minibatch && c->use_aux) {
    {
      StreamScope side(c, 1);
      RGCN_TRY(self_dw(c, s));
    }
    RGCN_TRY(self_dh(c, s));
    {
      StreamScope side(c, 0);
      RGCN_TRY(block_msg_backward(c, s.l, s.Hin, c->bwd_D, nullptr));
      RGCN_TRY(block_dw_reduce(c, s.l));
    }
    RGCN_TRY(block_rows(c, "block_rows_bwd", s.l, true, c->bwd_D, s.a));
    // Layer 2's side kernels read H_1, D_2 and dS_2 and write their own slabs and gradients.  Layer 1, next, overwrites
    // none of those (its rows go to g_emb) and queues its side kernels behind them in stream order: its joins cover
    // both layers, and the main stream saves two waits between the layers.
    *defer_joins = s.l == 2;
    // Layer 1 of a step that may end unjoined (rgcn_step_device): nothing on the main stream behind this layer touches
    // what the side kernels read or write, so the main stream does not wait for them either.  One event marks their end
    // (record_side_done); the next forward pass, the prefetch stream and whoever wants the gradients wait for it --
    // DESIGN.md section 5.1 lists who.
    if (s.l == 1 && deferred_schedule(c)) {
      RGCN_TRY(record_side_done(c));
      *defer_joins = true;
    }
    return *defer_joins ? RGCN_OK : stream_join_both(c);
  } else if (minibatch) {
    RGCN_TRY(block_msg_backward(c, s.l, s.Hin, c->bwd_D, nullptr));
    {
      StreamScope side(c, 1, /*in_capture=*/true);
      RGCN_TRY(block_dw_reduce(c, s.l));
      RGCN_TRY(self_dw(c, s));
    }
    RGCN_TRY(self_dh(c, s));
    return block_rows(c, "block_rows_bwd", s.l, true, c->bwd_D, s.a);
  } else {
    {
      StreamScope side(c, 0);
      RGCN_TRY(wait_gather(c));          // D_l of every row (sharded run: gathered beside the self-loop GEMMs)
      RGCN_TRY(block_msg_backward(c, s.l, s.Hin, c->bwd_D, nullptr));
      RGCN_TRY(block_dw_reduce(c, s.l));
      c->dw_pending = side.active;
    }
    {
      StreamScope side(c, 1);
      RGCN_TRY(self_dw(c, s));
    }
    RGCN_TRY(self_dh(c, s));
    RGCN_TRY(wait_gather(c));
    return block_rows(c, "block_rows_bwd", s.l, true, c->bwd_D, s.a);
  }
}

static rgcn_status bwd_block_two_kernel(rgcn_ctx* c, const BwdLayer& s) {
  const int l = s.l, d = c->d, V = c->V;
  const double Mmsg = 2.0 * c->g.E / c->world;
  {   // two-kernel form: the relational gradient kernels (HBM-bound) on a side stream beside the self-loop GEMMs
    StreamScope side(c, 0);
    RGCN_TRY(wait_gather(c));          // D_l of every row (sharded run: gathered beside the self-loop GEMMs)
    RGCN_TRY(block_msg_backward(c, l, s.Hin, c->bwd_D, c->msgbuf));
    // the combine below needs only the message rows: mark the join point here, then let the
    // per-relation dW reduction trail behind on the side stream
    if (side.active) RGCN_HIP(c, hipEventRecord(c->ev_join[0], c->aux[0]));
    RGCN_TRY(block_dw_reduce(c, l));
  }
  RGCN_TRY(self_dh(c, s));
  {   // dW_self on side stream 1, queued behind the dH GEMM
    StreamScope side(c, 1);
    RGCN_TRY(self_dw(c, s));
  }
  if (c->use_aux) RGCN_HIP(c, hipStreamWaitEvent(c->main_stream, c->ev_join[0], 0));
  CombineArgs a = s.a;
  a.msg = c->g.E > 0 ? c->msgbuf : nullptr;
  a.row_ptr = c->g.row_ptr; a.long_rows = c->g.long_rows; a.nlong = c->g.nlong;
  return combine(c, "combine_bwd", a, 4.0 * d * ((a.out2 ? 4.0 : 3.0) * V + Mmsg) + 4.0 * V);
}

static rgcn_status bwd_tdiag(rgcn_ctx* c, const BwdLayer& s) {
  const int l = s.l, d = c->d, V = c->V, Bd = c->B * d;
  // db = the column sums of D (this layer's bias is added, gcn_basis_times_diag.py:86); dP source-major from D and G
  RGCN_TRY(tdiag_refresh_gates(c, l));
  RGCN_TRY(column_sum(c, c->bwd_D, s.lb->gbias, V, d));
  RGCN_TRY(tdiag_dp(c, l, c->bwd_D, c->tdiag_dP));
  {   // dC needs P_l and D only: per relation chunk on side stream 0, beside the dense products
    StreamScope side(c, 0);
    RGCN_TRY(tdiag_dcoef(c, l, c->tdiag_P[l], c->bwd_D));
  }
  {   // the two weight gradients on side stream 1 (they share the split-K slabs: one stream, in order)
    StreamScope side(c, 1);
    RGCN_TRY(self_dw(c, s));
    // dW_dir = H^T . dP_dir   ([d, V] x [V, B.d], split over the rows; two groups, the same A operand)
    const GemmBatch gk = tdiag_batch(0, (size_t)V * Bd, (size_t)d * Bd);
    int split = auto_split_k(d, 2 * Bd, V, true);
    if (split > 16) split = 16;      // (the slabs are sized for 16: rgcn_create)
    RGCN_TRY(gemm_f32(c, "gemm_tdiag_dw", false, false, d, Bd, V, s.Hin, d, c->tdiag_dP, Bd, s.lb->grel, Bd, split, &gk));
  }
  RGCN_TRY(self_dh(c, s));
  // dH's relational part: dP_dir . W_dir^T   ([V, B.d] x [B.d, d], two groups), added by the epilogue kernel
  const GemmBatch gm = tdiag_batch((size_t)V * Bd, (size_t)d * Bd, (size_t)V * d);
  RGCN_TRY(gemm_f32(c, "gemm_tdiag_dh", true, true, V, d, Bd, c->tdiag_dP, Bd, s.lb->wrel, Bd, c->tdiag_dh, d, 1, &gm));
  RGCN_TRY(tdiag_dh_join(c, c->tdiag_dh, s.a));
  return stream_join(c, 0);      // (the next layer rewrites D's buffer, dP and the chunk slabs)
}

static rgcn_status bwd_pdiag(rgcn_ctx* c, const BwdLayer& s) {
  const int l = s.l;
  // db = the column sums of G = dL/dpre (this layer's bias is added); dD needs H_{l-1} and G only: per relation chunk on
  // side stream 0, beside the dense products
  RGCN_TRY(column_sum(c, c->bwd_D, s.lb->gbias, c->V, c->d));
  {
    StreamScope side(c, 0);
    RGCN_TRY(pdiag_ddiag(c, l, s.Hin, c->bwd_D));
  }
  // the dense products are the basis kind's, over the compacted units: G[units], dW'_dir = Zc_dir^T . G[units] beside
  // dW_self on side stream 1, dZc_dir = G[units] . W'_dir^T on the main stream behind dS . W_self^T
  RGCN_TRY(basis_gather_units(c, c->bwd_D, c->aggbuf));
  {
    StreamScope side(c, 1);
    RGCN_TRY(self_dw(c, s));
    RGCN_TRY(units_product_dw(c, l));
  }
  RGCN_TRY(self_dh(c, s));
  RGCN_TRY(units_product_dz(c, l));
  // row-local: da and the a * dZc part of dH; dC from da per relation chunk; then the source-major diagonal gather joins
  // the three parts of dH, applies relu' and writes the dropout copy
  RGCN_TRY(pdiag_row_backward(c, s.Hin, c->msgbuf2, c->pdiag_a[l], c->pdiag_da, c->pdiag_dh));
  RGCN_TRY(pdiag_dcoef(c, l, c->pdiag_da));
  RGCN_TRY(pdiag_dh_join(c, l, c->bwd_D, c->pdiag_dh, s.a));
  return stream_join(c, 0);      // (the next layer rewrites G's buffer and the dD slabs)
}

static rgcn_status bwd_basis(rgcn_ctx* c, const BwdLayer& s) {
  const int l = s.l;
  // The upstream rows of the units, compacted like Zc (the row operand of dZ, the depth operand of dW')
  RGCN_TRY(wait_gather(c));            // D_l of every row
  RGCN_TRY(basis_gather_units(c, c->bwd_D, c->aggbuf));
  // The four dense contractions of the layer depend on D_l / dS_l only.  Two of them -- the weight gradients dW_self =
  // H^T.dS and dW'_dir = Zc_dir^T.D[units], needed at the end of the pass -- go to side stream 1, the two whose
  // products the gather kernels below consume (dH's self-loop part, dZ) stay on the main stream: the pairs fill each
  // other's idle CU slots and tails.
  {
    StreamScope side(c, 1);
    RGCN_TRY(self_dw(c, s));
    RGCN_TRY(units_product_dw(c, l));
  }
  RGCN_TRY(self_dh(c, s));
  RGCN_TRY(units_product_dz(c, l));
  RGCN_TRY(basis_dcoef(c, l, s.Hin, c->msgbuf2));
  return basis_backward_gather(c, l, c->msgbuf2, s.a, true);
}

// Highway context, ahead of the layer's own form: the highway pass of layer l and its weight gradient.
static rgcn_status bwd_highway_open(rgcn_ctx* c, const BwdLayer& s) {
  const int l = s.l, d = c->d, V = c->V;
  // G_l (bwd_D; l < L: in dbuf[l & 1], turned into D_l in place) -> D_l, dS_l, dZ_l, the carry, db_hw's partials
  const DropSpec dl = make_drop(c, l, true);
  float* dS = dl.mode != DROP_NONE ? c->dsbuf[l & 1] : nullptr;
  int nparts = 0;
  RGCN_TRY(highway_backward(c, c->bwd_D, c->hw_T[l], c->hw_N[l], s.Hin, c->dbuf[l & 1], dS, c->hw_dz[l & 1], c->hw_carry,
                            l < c->L ? 1 : 0, dl, &nparts));
  RGCN_TRY(column_sum_finish(c, s.lb->gbhw, nparts, d));
  c->bwd_D = c->dbuf[l & 1];
  c->bwd_dS = dS ? dS : c->dbuf[l & 1];
  {   // dW_hw = H_{l-1}^T . dZ (split-K): side stream 1, AHEAD of the layer's dW_self there -- the two share the slabs
    StreamScope side(c, 1);
    RGCN_TRY(gemm_f32(c, "gemm_highway_dw", false, false, d, d, V, s.Hin, d, c->hw_dz[l & 1], d, s.lb->gwhw, d,
                      auto_split_k(d, d, V, s.narrow_dw)));
  }
  return RGCN_OK;
}

rgcn_status bwd_layer_partial(rgcn_ctx* c, int l) {
  RGCN_NO_EMBEDDING(c, "rgcn_backward_layer_partial");
  if (l != c->bwd_layer || l < 1) RGCN_FAIL(c, RGCN_ERR_STATE, "backward layers must run L..1 in order");
  const LayerForm form = layer_form(c, l);
  if (form == FORM_ONEHOT) return bwd_onehot(c);
  const int d = c->d, V = c->V;
  const RowShard rs = row_shard(c);
  BwdLayer s;
  s.l = l; s.Hin = c->H[l - 1]; s.lb = &c->layers[l]; s.lo = rs.lo; s.rows = rs.hi - rs.lo;
  s.narrow_dw = c->kind == RGCN_KIND_BASIS || c->kind == RGCN_KIND_BASIS_PDIAG || s.rows >= 32768;       // (see auto_split_k)

  // epilogue shared by both kinds: (self-loop gradient + relational gradient) -> relu' -> next D / dS
  CombineArgs& a = s.a;
  a.add = nullptr;
  a.base = c->self_buf; a.msg = nullptr; a.row_ptr = nullptr; a.long_rows = nullptr; a.nlong = nullptr;
  a.V = c->V; a.d = c->d; a.relu = 0; a.row_lo = rs.lo; a.row_hi = rs.hi;
  a.drop = make_drop(c, l, false);
  if (c->highway) {
    // The epilogue leaves the RAW dH_{l-1}: relu' belongs to N_{l-1}, not to H_{l-1}, and applies to the sum with the
    // highway terms -- the gate, the dropout copy and (l = 1) relu'(H_0) with db_emb's column sums are highway.hip's.
    a.out = (l - 1 == 0) ? c->g_emb : c->dbuf[(l - 1) & 1];
    a.out2 = nullptr; a.gate = nullptr; a.drop2 = make_drop(c, l - 1, false);
    RGCN_TRY(bwd_highway_open(c, s));
  } else if (c->world == 1) {
    a.out = (l - 1 == 0) ? c->g_emb : c->dbuf[(l - 1) & 1];
    a.colsum = (l - 1 == 0) ? 1 : 0;       // db_emb = the column sums of dL/dH0 * relu'(H0): partials from the kernel that writes it
    a.drop2 = make_drop(c, l - 1, l - 1 >= 1);
    a.out2 = a.drop2.mode != DROP_NONE ? c->dsbuf[(l - 1) & 1] : nullptr;
    a.gate = s.Hin;
  } else {
    a.out = c->exch; a.out2 = nullptr; a.gate = nullptr; a.drop2 = make_drop(c, l, false);
  }

  if (c->dw_pending) {       // the previous layer's weight-gradient kernel reads the D buffer this layer may overwrite
    RGCN_TRY(stream_join(c, 0));
    c->dw_pending = false;
  }
  RGCN_TRY(refresh_weight_fragments(c));
  bool defer_joins = false;
  switch (form) {
    case FORM_BLOCK_ROWS: RGCN_TRY(bwd_block_rows(c, s, &defer_joins)); break;
    case FORM_BLOCK_TWO_KERNEL: RGCN_TRY(bwd_block_two_kernel(c, s)); break;
    case FORM_TDIAG: RGCN_TRY(bwd_tdiag(c, s)); break;
    case FORM_PDIAG: RGCN_TRY(bwd_pdiag(c, s)); break;
    default: RGCN_TRY(bwd_basis(c, s)); break;
  }
  if (c->highway) {
    // G_{l-1} = raw dH_{l-1} + dZ_l . W_hw^T + G_l (1 - T_l), in place over the raw rows; the product goes through the
    // self-loop buffer, free since the epilogue above read it
    RGCN_TRY(gemm_f32(c, "gemm_highway_dh", true, true, V, d, d, c->hw_dz[l & 1], d, s.lb->whw, d, c->self_buf, d, 1));
    int nparts = 0;
    RGCN_TRY(highway_join(c, a.out, c->self_buf, c->hw_carry, l == 1 ? s.Hin : nullptr, &nparts));
    if (l == 1) c->colsum_parts = nparts;      // db_emb: bwd_end adds them
  }
  // the dW_self GEMM must be done before the next layer overwrites its dS operand / the caller
  // all-reduces gwself
  if (!defer_joins) RGCN_TRY(stream_join(c, 1));
  return RGCN_OK;
}

// The finish of a sharded layer: D_{l-1} = (the reduced dH in exch) * relu'(H_{l-1}), dS_{l-1} its dropout copy, over the rows
// [row_lo, row_hi).  On one GPU the layer's own epilogue has written both; out / out2 say where.
static CombineArgs bwd_finish_args(rgcn_ctx* c, int l, int row_lo, int row_hi) {
  CombineArgs a;
  a.add = nullptr; a.msg = nullptr; a.row_ptr = nullptr; a.long_rows = nullptr; a.nlong = nullptr;
  a.drop = make_drop(c, l, false);
  a.drop2 = make_drop(c, l - 1, l - 1 >= 1);
  a.out = (l - 1 == 0) ? c->g_emb : c->dbuf[(l - 1) & 1];
  a.out2 = a.drop2.mode != DROP_NONE ? c->dsbuf[(l - 1) & 1] : nullptr;
  a.base = c->exch; a.gate = c->H[l - 1]; a.V = c->V; a.d = c->d; a.relu = 0; a.row_lo = row_lo; a.row_hi = row_hi;
  return a;
}

rgcn_status bwd_layer_finish(rgcn_ctx* c, int l) {
  RGCN_NO_EMBEDDING(c, "rgcn_backward_layer_finish");
  if (l != c->bwd_layer || l < 1) RGCN_FAIL(c, RGCN_ERR_STATE, "backward layers must run L..1 in order");
  const CombineArgs a = bwd_finish_args(c, l, 0, c->V);
  if (c->world > 1) RGCN_TRY(combine(c, "combine_bwd_finish", a, 4.0 * c->d * (a.out2 ? 4.0 : 3.0) * c->V));
  c->bwd_D = a.out;
  c->bwd_dS = a.out2 ? a.out2 : a.out;
  c->bwd_layer = l - 1;
  return RGCN_OK;
}

rgcn_status bwd_end(rgcn_ctx* c) {
  RGCN_NO_EMBEDDING(c, "rgcn_backward_end");
  if (c->bwd_layer != 0) RGCN_FAIL(c, RGCN_ERR_STATE, "rgcn_backward_end before all layers ran");
  if (c->onehot) {      // no W_emb / b_emb: nothing of the bottom-layer work exists (no relu' of H_0, no column sums)
    if (c->side_state != rgcn_ctx::SIDE_NONE) RGCN_TRY(join_abandoned_side_work(c));
    c->dw_pending = false;
    return stream_join(c, 0);
  }
  // AffineTransform: dW_emb = dH0 * (H0 > 0) is already in g_emb; db_emb = column sums
  // (single-pass block layer on one GPU: the bottom layer's row-gradient kernel left the column sums of its rows as partials)
  if (c->defer_end_joins && c->side_state == rgcn_ctx::SIDE_RECORDED && c->stream == c->main_stream && c->colsum_parts > 0) {
    // Deferred end (bwd_layer_partial, layer 1): the sum of the partials is 4 us of work nothing in the step waits for.  It
    // trails on side stream 1, behind the row kernel that left the partials; side stream 1 then waits for side stream 0, so
    // that its end is the end of everything the step launched (step_end records the graph set's ev_free there).  The next
    // pass writes its partials to the other half of the scratch: ordered behind this sum by the events of the pass between.
    {
      StreamScope side(c, 1);
      if (!side.active) RGCN_FAIL(c, RGCN_ERR_HIP, "internal: fork onto side stream 1 failed");
      RGCN_TRY(column_sum_finish(c, c->gb_emb, c->colsum_parts, c->d));
    }
    RGCN_HIP(c, hipStreamWaitEvent(c->aux[1], c->ev_join[0], 0));
    c->colsum_half ^= 1;
    c->colsum_parts = 0;
    c->dw_pending = false;
    return RGCN_OK;
  }
  if (c->side_state != rgcn_ctx::SIDE_NONE) RGCN_TRY(join_abandoned_side_work(c));      // (no partials were left, or a second rgcn_backward_end: gb_emb)
  if (c->colsum_parts > 0) RGCN_TRY(column_sum_finish(c, c->gb_emb, c->colsum_parts, c->d));
  else RGCN_TRY(column_sum(c, c->g_emb, c->gb_emb, c->V, c->d));
  c->colsum_parts = 0;
  c->dw_pending = false;
  return stream_join(c, 0);   // trailing per-relation dW reductions
}

// Sharded run with a communicator, forward exchange of layer l: the partial pre-activations are reduce-scattered,
// this rank applies the relu to ITS rows only, and the finished rows are all-gathered on side stream 1 while the main
// stream goes on (the next self-loop GEMM needs the rank's own rows, nothing else).
static rgcn_status fwd_exchange(rgcn_ctx* c, int l) {
  const int64_t chunk = (int64_t)c->shard_rows * c->d;
  RGCN_TRY(comm_reduce_scatter(c, c->exch, chunk));
  const size_t off = (size_t)c->rank * chunk;
  RGCN_TRY(relu_copy(c, c->exch + off, c->H[l] + off, chunk, l < c->L ? 1 : 0));
  RGCN_TRY(gather_rows(c, c->H[l]));
  if (l == c->L) {
    RGCN_TRY(wait_gather(c));          // the codes: every row, on the main stream
    c->fwd_done = true;
  }
  return RGCN_OK;
}

// Backward exchange of layer l: partial dH reduce-scattered, (relu', dropout) on the rank's rows, D_{l-1} gathered.
static rgcn_status bwd_exchange(rgcn_ctx* c, int l) {
  const int64_t chunk = (int64_t)c->shard_rows * c->d;
  RGCN_TRY(comm_reduce_scatter(c, c->exch, chunk));
  CombineArgs a = bwd_finish_args(c, l, c->row_lo, c->row_hi);
  a.v_begin = c->row_lo; a.v_count = c->row_hi - c->row_lo;      // (the launch walks the rank's own rows only)
  if (a.v_count > 0) RGCN_TRY(combine(c, "combine_bwd_finish", a, 4.0 * c->d * (a.out2 ? 4.0 : 3.0) * a.v_count));
  RGCN_TRY(gather_rows(c, a.out));
  c->bwd_D = a.out;
  c->bwd_dS = a.out2 ? a.out2 : a.out;      // own rows only: all the row-sharded self-loop GEMMs read
  c->bwd_layer = l - 1;
  return RGCN_OK;
}

rgcn_status forward_all(rgcn_ctx* c, int train, uint64_t seed, const uint8_t* masks) {
  if (c->embedding) {
    // RelationEmbedding(AffineTransform(onehot_input, no bias, no relu)), model_builder.py:27-41: the codes are the table
    // itself in either mode -- no graph, no dropout, no kernel.  H[0] is W_emb's own storage.
    c->fwd_train = train ? 1 : 0;
    c->seed = seed;
    c->fwd_done = true;
    return RGCN_OK;
  }
  if (c->world > 1 && !c->comm)
    RGCN_FAIL(c, RGCN_ERR_STATE, "world > 1: call rgcn_comm_init first (or drive the phase API yourself)");
  RGCN_TRY(fwd_begin(c, train, seed, masks));
  for (int l = 1; l <= c->L; ++l) {
    RGCN_TRY(fwd_layer_partial(c, l));
    if (c->world > 1) RGCN_TRY(fwd_exchange(c, l));
    else RGCN_TRY(fwd_layer_finish(c, l));
  }
  return RGCN_OK;
}

rgcn_status backward_all(rgcn_ctx* c, const float* dcodes_dev, const float* ds_ready) {
  if (c->embedding) {
    // dL/dW_emb = dL/dcodes.  The device decoder and rgcn_backward write it in place (dcodes_own IS g_emb); a caller's own
    // buffer is copied.  b_emb is never read: its gradient stays the zeros it was created with.
    if (!c->fwd_done) RGCN_FAIL(c, RGCN_ERR_STATE, "rgcn_backward needs a completed rgcn_forward");
    if (!dcodes_dev) RGCN_FAIL(c, RGCN_ERR_INVALID, "dcodes is NULL");
    if (dcodes_dev != c->g_emb)
      RGCN_HIP(c, hipMemcpyAsync(c->g_emb, dcodes_dev, sizeof(float) * (size_t)c->V * c->dc, hipMemcpyDeviceToDevice, c->stream));
    return RGCN_OK;
  }
  if (c->world > 1 && !c->comm)
    RGCN_FAIL(c, RGCN_ERR_STATE, "world > 1: call rgcn_comm_init first (or drive the phase API yourself)");
  RGCN_TRY(bwd_begin(c, dcodes_dev, ds_ready));
  for (int l = c->L; l >= 1; --l) {
    RGCN_TRY(bwd_layer_partial(c, l));
    if (c->world > 1) RGCN_TRY(bwd_exchange(c, l));
    else RGCN_TRY(bwd_layer_finish(c, l));
  }
  if (c->world > 1) {
    RGCN_TRY(wait_gather(c));          // dW_emb of every row (optimizer, column sums)
    // W_self (and basis W') gradients of all layers: partial sums over the row / relation shards, one collective
    RGCN_TRY(comm_allreduce(c, c->repl_grads, (int64_t)c->repl_grads_floats));
  }
  return bwd_end(c);
}

}  // namespace rgcn
