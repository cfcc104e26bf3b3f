// C ABI of librgcn.so (include/rgcn.h): contexts, parameters, graphs, steps, capture, profile.  The per-layer orchestration
// of the encoder (which kernel on which stream) lives in rgcn_schedule.hip, the stand-alone entry points of the devtools
// build in rgcn_devtools.hip; rgcn_api_internal.h is what the three share.
#include <cstdlib>
#include <mutex>
#include <utility>
#include <new>

#include "config_check.h"
#include "optimizer_check.h"
#include "rgcn_api_internal.h"

namespace rgcn {

static std::mutex g_err_mu;
static std::string g_err;
void set_global_error(const std::string& s) {
  std::lock_guard<std::mutex> lk(g_err_mu);
  g_err = s;
}

// ---------------------------------------------------------------- profiling
ProfScope::ProfScope(rgcn_ctx* ctx, const char* name, double bytes, double flops, double compulsory) : c(ctx), idx(-1) {
  if (!c->prof_on) return;
  ProfRec r;
  r.name = name;
  r.bytes = bytes;
  r.flops = flops;
  r.cbytes = compulsory < 0 ? bytes : compulsory;
  for (int k = 0; k < 2; ++k) {
    hipEvent_t e = nullptr;
    if (!c->event_pool.empty()) {
      e = c->event_pool.back();
      c->event_pool.pop_back();
    } else if (hipEventCreate(&e) != hipSuccess) {
      return;
    }
    (k == 0 ? r.e0 : r.e1) = e;
  }
  (void)hipEventRecord(r.e0, c->stream);
  c->prof.push_back(r);
  idx = (int)c->prof.size() - 1;
}
ProfScope::~ProfScope() {
  if (idx >= 0) (void)hipEventRecord(c->prof[idx].e1, c->stream);
}

StreamScope::StreamScope(rgcn_ctx* ctx, int k, bool in_capture) : c(ctx), saved(ctx->stream), active(false) {
  const bool on = c->use_aux || (in_capture && c->capturing && c->use_aux_before_capture && c->world == 1);
  if (k < 0 || !on || c->stream != c->main_stream) return;   // nested or disabled: stay on the current stream
  if (hipEventRecord(c->ev_fork, c->main_stream) != hipSuccess) return;
  if (hipStreamWaitEvent(c->aux[k], c->ev_fork, 0) != hipSuccess) return;
  c->stream = c->aux[k];
  c->aux_dirty[k] = true;
  active = true;
}
StreamScope::~StreamScope() { c->stream = saved; }

rgcn_status stream_join(rgcn_ctx* c, int k) {
  if (c->stream != c->main_stream) return RGCN_OK;
  // a join costs the main stream ~3.6 us even when the side stream is idle (profiles/r02_anyorder_probe.log): skip it when
  // nothing went to that stream since its last join (side streams switched off, or no fork taken)
  if (!c->aux_dirty[k]) return RGCN_OK;
  c->aux_dirty[k] = false;
  if (k < 2) c->side_state = rgcn_ctx::SIDE_NONE;      // (ev_join[k] is re-recorded: back to what the dirty flags say)
  RGCN_HIP(c, hipEventRecord(c->ev_join[k], c->aux[k]));
  RGCN_HIP(c, hipStreamWaitEvent(c->main_stream, c->ev_join[k], 0));
  return RGCN_OK;
}

// Side streams 0 and 1 behind ONE wait of the main stream (side 0 waits for side 1 first): where both were forked in the
// same layer, the second wait is a packet the main stream can do without.
rgcn_status stream_join_both(rgcn_ctx* c) {
  if (c->stream != c->main_stream) return RGCN_OK;
  if (c->aux_dirty[0] && c->aux_dirty[1]) {
    c->side_state = rgcn_ctx::SIDE_NONE;
    RGCN_HIP(c, hipEventRecord(c->ev_join[1], c->aux[1]));
    RGCN_HIP(c, hipStreamWaitEvent(c->aux[0], c->ev_join[1], 0));
    c->aux_dirty[1] = false;
  }
  RGCN_TRY(stream_join(c, 0));
  return stream_join(c, 1);
}

// Side kernels the main stream has not waited for.  Two ways to get there: a backward pass driven layer by layer (phase
// API) and abandoned between layers 2 and 1 (bwd_layer_partial defers layer 2's joins to layer 1), and the backward pass
// of rgcn_step_device, which ends unjoined on purpose (rgcn_ctx::side_state).  The side kernels read D / dS / the
// activations and the graph's message lists and write the weight gradients, their slabs and the bias gradient: whoever
// is about to rewrite what they read or to touch what they write -- a backward pass, a graph build on the main stream,
// the optimizer, a replayed graph, a copy into a caller's buffer -- joins them first (the calls that wait on the host
// synchronise the side streams themselves: sync_all, check_dev_flag).  Nothing is queued, and nothing is paid, where
// every pass ended joined.
rgcn_status join_abandoned_side_work(rgcn_ctx* c) {
  if (c->stream != c->main_stream) return RGCN_OK;
  RGCN_TRY(stream_join(c, 0));
  RGCN_TRY(stream_join(c, 1));
  c->side_state = rgcn_ctx::SIDE_NONE;
  return RGCN_OK;
}

// The end of a backward pass that leaves its side kernels unjoined: one event, on side stream 0, behind all of them.
rgcn_status record_side_done(rgcn_ctx* c) {
  RGCN_HIP(c, hipEventRecord(c->ev_join[1], c->aux[1]));
  RGCN_HIP(c, hipStreamWaitEvent(c->aux[0], c->ev_join[1], 0));
  RGCN_HIP(c, hipEventRecord(c->ev_join[0], c->aux[0]));
  c->aux_dirty[0] = c->aux_dirty[1] = true;
  c->side_state = rgcn_ctx::SIDE_RECORDED;
  return RGCN_OK;
}

// What a forward pass needs of unjoined side work: that it has finished READING (the pass overwrites the activations; it
// touches neither the gradients nor the slabs).  After a deferred end of step that is one wait for the event
// record_side_done left -- which fired before the main chain ended, the column sums behind it excluded -- and the gradients
// stay pending; in every other state, the full join.  also: an event of another stream (a prefetched graph's ev_ready) the
// main stream has to wait for at the same point; side stream 0, idle by then, takes that wait and the main stream still
// pays ONE wait packet.
rgcn_status join_side_reads(rgcn_ctx* c, hipEvent_t also) {
  if (c->stream != c->main_stream) return RGCN_OK;
  if (c->side_state == rgcn_ctx::SIDE_RECORDED) {
    if (also) {
      RGCN_HIP(c, hipStreamWaitEvent(c->aux[0], also, 0));
      RGCN_HIP(c, hipEventRecord(c->ev_join[0], c->aux[0]));
    }
    RGCN_HIP(c, hipStreamWaitEvent(c->main_stream, c->ev_join[0], 0));
    c->side_state = rgcn_ctx::SIDE_READS_JOINED;
    return RGCN_OK;
  }
  if (c->side_state != rgcn_ctx::SIDE_READS_JOINED) RGCN_TRY(join_abandoned_side_work(c));
  if (also) RGCN_HIP(c, hipStreamWaitEvent(c->main_stream, also, 0));
  return RGCN_OK;
}

static rgcn_status sync_all(rgcn_ctx* c) {
  if (c->capturing) RGCN_FAIL(c, RGCN_ERR_STATE, "this call synchronises with the device: not allowed between rgcn_capture_begin and rgcn_capture_end");
  if (c->pf_stream) RGCN_HIP(c, hipStreamSynchronize(c->pf_stream));
  for (int k = 0; k < kAuxStreams; ++k)
    if (c->aux[k]) RGCN_HIP(c, hipStreamSynchronize(c->aux[k]));
  RGCN_HIP(c, hipStreamSynchronize(c->main_stream));
  for (int k = 0; k < kAuxStreams; ++k) c->aux_dirty[k] = false;     // nothing left to join
  c->side_state = rgcn_ctx::SIDE_NONE;
  return RGCN_OK;
}

static rgcn_status profile_collect(rgcn_ctx* c) {
  RGCN_TRY(sync_all(c));
  for (ProfRec& r : c->prof) {
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, r.e0, r.e1);
    ProfAgg* a = nullptr;
    for (ProfAgg& x : c->prof_agg)
      if (x.name == r.name) { a = &x; break; }
    if (!a) {
      c->prof_agg.push_back({r.name, 0, 0.0, 0.0, 0.0, 0.0});
      a = &c->prof_agg.back();
    }
    a->calls += 1;
    a->ms += ms;
    a->bytes += r.bytes;
    a->flops += r.flops;
    a->cbytes += r.cbytes;
    c->event_pool.push_back(r.e0);
    c->event_pool.push_back(r.e1);
  }
  c->prof.clear();
  return RGCN_OK;
}

// ---------------------------------------------------------------- helpers

static void add_param(rgcn_ctx* c, const std::string& name, std::initializer_list<int64_t> shape,
                      float* val, float* grad, int layout) {
  Param p;
  p.name = name;
  p.ndim = (int)shape.size();
  p.count = 1;
  int i = 0;
  for (int64_t s : shape) { p.shape[i++] = s; p.count *= s; }
  for (; i < 4; ++i) p.shape[i] = 1;
  p.val = val;
  p.grad = grad;
  p.layout = layout;
  c->params.push_back(p);
}

// target: workgroups of a split-K launch.  Since the dW_self GEMM runs beside the dH GEMM (the backward layer's pairing)
// FEWER workgroups pay in the step -- headline 0.555-0.562 ms per step at 256, 0.558-0.568 at 384, 0.565-0.568 at 448,
// 0.567-0.575 at 512 -- but cost the GEMM itself (alone on the chip 54.6 us at 256, 51 at 448, 48.7 at 512: one workgroup
// per CU).  The headline shape keeps 512 (the step's gain is ~1 %, inside the box-to-box spread);
// `narrow` -- 256 -- where the step gains 3-5 %: K >= 32,768 rows (WN18 sizes: 1.128 ms against 1.166) and the
// basis kind (B = 2: 1.64 against 1.72).  profiles/r04_*: splitk A/B.  The rule reads the model's
// dimensions only, one figure for every form of the layer: the split decides the summation order of dW_self, and the forms
// are held bitwise equal to each other.
int auto_split_k(int M, int N, int K, bool narrow) {
  const int tiles = ((M + 127) / 128) * ((N + 127) / 128);
  if (tiles >= 192) return 1;
  const int target = narrow ? 256 : 512;
  int s = (target + tiles - 1) / tiles;
  const int max_by_k = (K + 127) / 128;   // at least 128 of K per slab
  if (s > max_by_k) s = max_by_k;
  if (s > 64) s = 64;
  if (s < 1) s = 1;
  return s;
}

// main_only: wait for the main stream alone (everything a finished step depends on was joined into it); the
// graph preparation of the NEXT minibatch, running on the prefetch stream, is left alone and its id check
// surfaces at the next synchronising call.
static rgcn_status check_dev_flag(rgcn_ctx* c, bool main_only = false) {
  if (c->capturing) RGCN_FAIL(c, RGCN_ERR_STATE, "this call synchronises with the device: not allowed between rgcn_capture_begin and rgcn_capture_end");
  int32_t flag = 0;
  if (!main_only) {
    if (c->pf_stream) RGCN_HIP(c, hipStreamSynchronize(c->pf_stream));
    for (int k = 0; k < kAuxStreams; ++k)
      if (c->aux[k]) RGCN_HIP(c, hipStreamSynchronize(c->aux[k]));
  }
  RGCN_HIP(c, hipMemcpyAsync(&flag, c->g.errflag, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  RGCN_HIP(c, hipStreamSynchronize(c->stream));
  if (flag) {
    RGCN_HIP(c, hipMemsetAsync(c->g.errflag, 0, sizeof(int32_t), c->stream));
    RGCN_FAIL(c, RGCN_ERR_INVALID, std::string(flag & 4 ? "edge dropout: the keep mask does not hold exactly `keep` ones; " : "") +
                                   (flag & 8 ? "device neighbourhood sampler: the relaxations did not settle within their iteration budget "
                                               "(a graph of very large diameter: use the host sampler); " : "") +
                                   (flag & 32 ? "device neighbourhood sampler: the compacted batch does not hold the requested number "
                                                "of edges (internal error: two draws sharing the sampler's state?); " : "") +
                                   (flag & 64 ? "relation softmax: a row taken as a positive does not carry the label 1; " : "") +
                                   (flag & 128 ? "adversarial negatives: the labels are not 1 for the leading positives and 0 for every "
                                                 "row behind them; " : "") +
                                   (flag & 256 ? "weighted decoder: a row weight is negative or not finite; " : "") +
                                   (flag & 16 ? "the decoder batch is no longer the tiled batch rgcn_negative_sample_device wrote into that "
                                                "buffer (rewritten by the caller's own kernels?): pass it in another buffer; " : "") +
                                   (flag & 3 ? "graph_edges / the decoder batch contains a vertex id outside [0,EntityCount) or a "
                                               "relation id outside [0,RelationCount)" : ""));
  }
  return RGCN_OK;
}

// A caller that rewrites (or frees) the triple buffer a prefetched graph was prepared from makes that
// preparation stale: drop it, the next step rebuilds in line.
static void invalidate_prefetch_of(rgcn_ctx* c, const void* dev, size_t bytes) {
  // a caller that rewrites the buffer the negative sampler tiled makes the decoder's knowledge of its layout stale
  if (c->dec.tiled_X) {
    const char* t = reinterpret_cast<const char*>(c->dec.tiled_X);
    const char* lo = reinterpret_cast<const char*>(dev);
    if (t + sizeof(int32_t) * 3 * (size_t)c->dec.tiled_N > lo && t < lo + (bytes ? bytes : 1)) c->dec.tiled_X = nullptr;
  }
  for (GraphBufs* g : {&c->g, &c->g_alt}) {
    if (!g->pf_valid || !g->pf_tri) continue;
    const char* t = reinterpret_cast<const char*>(g->pf_tri);
    const char* lo = reinterpret_cast<const char*>(dev);
    if (t + sizeof(int32_t) * 3 * (size_t)g->pf_E > lo && t < lo + (bytes ? bytes : 1)) g->pf_valid = false;
  }
}

rgcn_status to_host(rgcn_ctx* c, void* host, const void* dev, size_t bytes) {
  if (c->capturing) RGCN_FAIL(c, RGCN_ERR_STATE, "host transfers are not allowed while a hipGraph is being captured");
  RGCN_HIP(c, hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, c->stream));
  RGCN_HIP(c, hipStreamSynchronize(c->stream));
  return RGCN_OK;
}
rgcn_status to_dev(rgcn_ctx* c, void* dev, const void* host, size_t bytes) {
  if (c->capturing) RGCN_FAIL(c, RGCN_ERR_STATE, "host transfers are not allowed while a hipGraph is being captured");
  RGCN_HIP(c, hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, c->stream));
  RGCN_HIP(c, hipStreamSynchronize(c->stream));   // host memory is borrowed for the call only
  return RGCN_OK;
}

// Process-wide stream pool.  ROCm hands a new stream its hardware queue round-robin, and objects that outlive a
// context (an instantiated hipGraph with a forked branch keeps internal streams) shift that assignment: a context
// created LATER in the same process could find two of its four streams on one hardware queue, and its stream-launched
// step ran at half speed with the GPU idle between kernels (seen in bench.py: the second train-step workload at 2.7 ms
// against 1.3 ms in a fresh process, graph replay unaffected).  Streams are therefore kept when a context is destroyed
// and handed to the next one on that device: every context of a process runs on the streams -- and the queue
// assignment -- of the first.  Key: (device, priority).  Never destroyed (the runtime goes first at exit).
namespace {
struct PooledStream { int device; int priority; hipStream_t s; };
struct StreamPool {
  std::mutex mu;
  std::vector<PooledStream> free_streams;
};
StreamPool& stream_pool() {          // allocated once, never destroyed: usable from whatever runs at process exit
  static StreamPool* pool = new StreamPool();
  return *pool;
}
}  // namespace
static hipError_t acquire_stream(int device, int priority, hipStream_t* out) {
  {
    StreamPool& sp = stream_pool();
    std::lock_guard<std::mutex> lk(sp.mu);
    for (size_t i = 0; i < sp.free_streams.size(); ++i)
      if (sp.free_streams[i].device == device && sp.free_streams[i].priority == priority) {
        *out = sp.free_streams[i].s;
        sp.free_streams.erase(sp.free_streams.begin() + (long)i);
        return hipSuccess;
      }
  }
  return hipStreamCreateWithPriority(out, hipStreamNonBlocking, priority);
}
static void release_stream(int device, int priority, hipStream_t s) {
  if (!s) return;
  StreamPool& sp = stream_pool();
  std::lock_guard<std::mutex> lk(sp.mu);
  sp.free_streams.push_back(PooledStream{device, priority, s});
}

static void free_all(rgcn_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->cfg.device);
  if (c->capturing && c->main_stream) {      // destroyed in mid-capture: the streams go back to the pool in a usable state
    hipGraph_t dangling = nullptr;
    (void)hipStreamEndCapture(c->main_stream, &dangling);
    if (dangling) (void)hipGraphDestroy(dangling);
    (void)hipGetLastError();
    c->capturing = false;
  }
  if (c->pf_stream) (void)hipStreamSynchronize(c->pf_stream);
  for (int k = 0; k < kAuxStreams; ++k)
    if (c->aux[k]) (void)hipStreamSynchronize(c->aux[k]);
  if (c->main_stream) (void)hipStreamSynchronize(c->main_stream);
  comm_destroy(c);
  graph_free(c);
  decoder_free(c);
  neighborhood_free(c);
  known_positives_free(c);
  type_sets_free(c);
  optimizer_free(c);
  relation_softmax_free(c);
  entity_softmax_free(c);
  adversarial_free(c);
  rank_free(c);
  c->pool.release();
  for (ProfRec& r : c->prof) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
  for (hipEvent_t e : c->event_pool) (void)hipEventDestroy(e);
  if (c->t0) (void)hipEventDestroy(c->t0);
  if (c->t1) (void)hipEventDestroy(c->t1);
  for (int k = 0; k < kAuxStreams; ++k) {
    if (k < 2) release_stream(c->cfg.device, c->aux_priority, c->aux[k]);     // aux[2] is the prefetch stream, below
    if (c->ev_join[k]) (void)hipEventDestroy(c->ev_join[k]);
  }
  if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
  if (c->ev_gather) (void)hipEventDestroy(c->ev_gather);
  if (c->ev_step_begin) (void)hipEventDestroy(c->ev_step_begin);
  for (hipGraphExec_t g : c->graphs) if (g) (void)hipGraphExecDestroy(g);
  for (hipGraph_t g : c->graph_defs) if (g) (void)hipGraphDestroy(g);
  if (c->readback_host) (void)hipHostFree(c->readback_host);
  if (c->stage_host) {
    (void)hipHostFree(c->stage_host);
    for (hipEvent_t e : c->stage_done) if (e) (void)hipEventDestroy(e);
  }
  release_stream(c->cfg.device, c->pf_priority, c->pf_stream);
  release_stream(c->cfg.device, 0, c->main_stream);
  delete c;
}

// RGCN_KIND_EMBEDDING: the parameters in Model.get_weights() order (affine_transform.py:30-31, relation_embedding.py:15-18)
// and what the decoder, the optimizer and the ranking calls touch outside their own pools.  No graph set, no activations.
static rgcn_status create_embedding(rgcn_ctx* c) {
  const size_t V = c->V, d = c->d;
  RGCN_TRY(dmalloc(c, c->pool, &c->w_emb, V * d, true));
  RGCN_TRY(dmalloc(c, c->pool, &c->g_emb, V * d, true));
  RGCN_TRY(dmalloc(c, c->pool, &c->b_emb, d, true));
  RGCN_TRY(dmalloc(c, c->pool, &c->gb_emb, d, true));
  add_param(c, "W_emb", {(int64_t)V, (int64_t)d}, c->w_emb, c->g_emb, LAYOUT_PLAIN);
  add_param(c, "b_emb", {(int64_t)d}, c->b_emb, c->gb_emb, LAYOUT_PLAIN);
  c->params.back().no_grad = true;      // use_bias=False: created, checkpointed, never read (TF reports it unconnected)
  RGCN_TRY(dmalloc(c, c->pool, &c->w_rel, V * d, true));
  RGCN_TRY(dmalloc(c, c->pool, &c->g_rel, V * d, true));
  add_param(c, "W_relation", {(int64_t)V, (int64_t)d}, c->w_rel, c->g_rel, LAYOUT_PLAIN);
  c->layers.resize(1);
  c->H.assign(1, c->w_emb);             // the codes ARE the table
  c->codes = c->w_emb;
  c->dcodes_own = c->g_emb;             // the decoder's dL/dcodes lands where the optimizer reads dL/dW_emb
  // the ranking GEMM's launcher wants the zero page and a slab pointer (split_k = 1: no slab is ever written)
  c->slab_floats = 1024;
  RGCN_TRY(dmalloc(c, c->pool, &c->slab, c->slab_floats, true));
  RGCN_TRY(dmalloc(c, c->pool, &c->zeros, 1024, true));
  RGCN_TRY(dmalloc(c, c->pool, &c->g.errflag, 1, true));
  c->g_alt.errflag = c->g.errflag;
  RGCN_HIP(c, hipStreamSynchronize(c->stream));
  return RGCN_OK;
}

// ---- rgcn_create, piece by piece: streams and events; the parameter table, layer by layer (one function per layer form and
// the tail every form shares); the activations; the scratch of each kind; the tail every kind shares.  What a configuration
// is refused for is config_check.h's.
static rgcn_status create_streams(rgcn_ctx* c) {
  const rgcn_config& f = c->cfg;
  RGCN_HIP(c, hipSetDevice(f.device));
  RGCN_HIP(c, acquire_stream(f.device, 0, &c->stream));
  c->main_stream = c->stream;
  {
    // side streams get the highest priority: their short HBM-bound kernels should claim wave slots
    // ahead of the long MFMA-bound grid they run beside
    int prio_lo = 0, prio_hi = 0;
    RGCN_HIP(c, hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
    // Two high-priority side streams; "side stream 2" is the prefetch stream (created here, normal or low priority):
    // both of its jobs -- the next minibatch's graph prep and the decoder's relation gradient -- are fillers.  A
    // fifth HIP stream would share a hardware queue with one of the other four (ROCm maps streams onto 4 queues by
    // default) and serialise against it: measured, the pipelined encoder step went from 0.60 to 0.97 ms.
    c->aux_priority = prio_hi;
    for (int k = 0; k < 2; ++k) RGCN_HIP(c, acquire_stream(f.device, c->aux_priority, &c->aux[k]));
    c->pf_priority = prio_lo;
    RGCN_HIP(c, acquire_stream(f.device, c->pf_priority, &c->pf_stream));
    c->aux[2] = c->pf_stream;
    for (int k = 0; k < kAuxStreams; ++k)
      RGCN_HIP(c, hipEventCreateWithFlags(&c->ev_join[k], order_event_flags(c, true)));
  }
  RGCN_HIP(c, hipEventCreateWithFlags(&c->ev_fork, order_event_flags(c, true)));
  RGCN_HIP(c, hipEventCreateWithFlags(&c->ev_step_begin, order_event_flags(c)));
  // Block kind: the destination-major banded single pass (block_rows.hip; rgcn_set_fusion 1, the default) -- no message
  // buffer, weights through L2: 39-41 us forward / 46-48 backward per layer against 57 / 75 for the two-kernel form
  // (rgcn_set_fusion 0: k_block_msg_* + k_combine, the form every other is held bitwise equal to) at FB15k-237 minibatch
  // size, 0.39 ms against 0.77 per layer pass at the 272,115-edge training graph (profiles/r04_rowmajor_spmm_ab.md).
  // Two more forms were built, measured slower and removed in round 5: the combine as the self-loop GEMM's epilogue
  // (profiles/r02_fused_layer_ab.log) and per-block workgroups with an LDS weight table (profiles/r03_block_spmm_ab.md).
  c->use_aux = true;
  c->fuse = 1;
  c->gemm_mode = 6;
  RGCN_HIP(c, hipEventCreate(&c->t0));
  RGCN_HIP(c, hipEventCreate(&c->t1));
  return RGCN_OK;
}

// BasisGcn with onehot_input=True (gcn_basis.py:16-24): vertex_feature_dimension = EntityCount -- W_forward,
// W_backward [V,B,d] and W_self [V,d] are lookup tables, kept in the host layout; no GEMM, no fragment tables
static rgcn_status create_onehot_layer(rgcn_ctx* c, LayerBufs& lb) {
  const size_t V = c->V, d = c->d, R = c->R;
  const size_t per_dir = V * (size_t)c->B * d;
  RGCN_TRY(dmalloc(c, c->pool, &lb.wrel, 2 * per_dir, true));
  RGCN_TRY(dmalloc(c, c->pool, &lb.grel, 2 * per_dir, true));
  RGCN_TRY(dmalloc(c, c->pool, &lb.coef, 2 * R * c->B, true));
  RGCN_TRY(dmalloc(c, c->pool, &lb.gcoef, 2 * R * c->B, true));
  add_param(c, "W_f1", {(int64_t)V, c->B, (int64_t)d}, lb.wrel, lb.grel, LAYOUT_PLAIN);
  add_param(c, "W_b1", {(int64_t)V, c->B, (int64_t)d}, lb.wrel + per_dir, lb.grel + per_dir, LAYOUT_PLAIN);
  add_param(c, "C_f1", {(int64_t)R, c->B}, lb.coef, lb.gcoef, LAYOUT_PLAIN);
  add_param(c, "C_b1", {(int64_t)R, c->B}, lb.coef + R * c->B, lb.gcoef + R * c->B, LAYOUT_PLAIN);
  RGCN_TRY(dmalloc(c, c->pool, &lb.wself, V * d, true));
  RGCN_TRY(dmalloc(c, c->pool, &lb.gwself, V * d, true));
  RGCN_TRY(dmalloc(c, c->pool, &lb.bias, d, true));
  RGCN_TRY(dmalloc(c, c->pool, &lb.gbias, d, true));
  add_param(c, "W_self1", {(int64_t)V, (int64_t)d}, lb.wself, lb.gwself, LAYOUT_PLAIN);
  add_param(c, "b1", {(int64_t)d}, lb.bias, lb.gbias, LAYOUT_PLAIN);
  c->params.back().no_grad = true;
  return RGCN_OK;
}

static rgcn_status create_block_layer(rgcn_ctx* c, LayerBufs& lb, const std::string& sl) {
  const size_t R = c->R;
  const size_t per_dir = R * c->nb * c->sd * c->sd;
  RGCN_TRY(dmalloc(c, c->pool, &lb.wrel, 2 * per_dir, true));
  RGCN_TRY(dmalloc(c, c->pool, &lb.grel, 2 * per_dir, true));
  add_param(c, "W_f" + sl, {(int64_t)R, c->nb, c->sd, c->sd}, lb.wrel, lb.grel, LAYOUT_BLOCK_T);
  add_param(c, "W_b" + sl, {(int64_t)R, c->nb, c->sd, c->sd}, lb.wrel + per_dir, lb.grel + per_dir, LAYOUT_BLOCK_T);
  return dmalloc(c, c->pool, &lb.wtile, block_rows_weight_floats(c), true);
}

// gcn_basis_times_diag.py:38-42.  W_forward, W_backward stay in the host layout [d][B.d]: it is the B operand of
// P = H . W with N contiguous; the coefficients are [R,B,d] per direction, their sigmoid a table of the same shape
static rgcn_status create_tdiag_layer(rgcn_ctx* c, LayerBufs& lb, const std::string& sl) {
  const size_t d = c->d, R = c->R;
  const size_t per_dir = (size_t)c->B * d * d, per_c = R * c->B * d;
  RGCN_TRY(dmalloc(c, c->pool, &lb.wrel, 2 * per_dir, true));
  RGCN_TRY(dmalloc(c, c->pool, &lb.grel, 2 * per_dir, true));
  RGCN_TRY(dmalloc(c, c->pool, &lb.coef, 2 * per_c, true));
  RGCN_TRY(dmalloc(c, c->pool, &lb.gcoef, 2 * per_c, true));
  RGCN_TRY(dmalloc(c, c->pool, &lb.tdiag_g, 2 * per_c, true));
  add_param(c, "W_f" + sl, {(int64_t)d, c->B, (int64_t)d}, lb.wrel, lb.grel, LAYOUT_PLAIN);
  add_param(c, "W_b" + sl, {(int64_t)d, c->B, (int64_t)d}, lb.wrel + per_dir, lb.grel + per_dir, LAYOUT_PLAIN);
  add_param(c, "C_f" + sl, {(int64_t)R, c->B, (int64_t)d}, lb.coef, lb.gcoef, LAYOUT_PLAIN);
  add_param(c, "C_b" + sl, {(int64_t)R, c->B, (int64_t)d}, lb.coef + per_c, lb.gcoef + per_c, LAYOUT_PLAIN);
  return RGCN_OK;
}

// repl: the layer's slice of rgcn_ctx::repl_grads (sharded run), or null
static rgcn_status create_basis_layer(rgcn_ctx* c, LayerBufs& lb, const std::string& sl, float* repl) {
  const size_t d = c->d, R = c->R;
  const size_t per_dir = (size_t)c->B * d * d;
  RGCN_TRY(dmalloc(c, c->pool, &lb.wrel, 2 * per_dir, true));
  if (repl) lb.grel = repl + d * d;
  else RGCN_TRY(dmalloc(c, c->pool, &lb.grel, 2 * per_dir, true));
  RGCN_TRY(dmalloc(c, c->pool, &lb.coef, 2 * R * c->B, true));
  RGCN_TRY(dmalloc(c, c->pool, &lb.gcoef, 2 * R * c->B, true));
  // (BASIS_PDIAG: the two direction groups swapped -- the forward-direction units contract with W_backward)
  const bool pdiag = c->kind == RGCN_KIND_BASIS_PDIAG;
  const size_t off_f = pdiag ? per_dir : 0, off_b = pdiag ? 0 : per_dir;
  add_param(c, "W_f" + sl, {(int64_t)d, c->B, (int64_t)d}, lb.wrel + off_f, lb.grel + off_f, LAYOUT_BASIS_T);
  add_param(c, "W_b" + sl, {(int64_t)d, c->B, (int64_t)d}, lb.wrel + off_b, lb.grel + off_b, LAYOUT_BASIS_T);
  add_param(c, "C_f" + sl, {(int64_t)R, c->B}, lb.coef, lb.gcoef, LAYOUT_PLAIN);
  add_param(c, "C_b" + sl, {(int64_t)R, c->B}, lb.coef + R * c->B, lb.gcoef + R * c->B, LAYOUT_PLAIN);
  return RGCN_OK;
}

// the basis layer's tensors and, behind them, the diagonal tables
static rgcn_status create_pdiag_layer(rgcn_ctx* c, LayerBufs& lb, const std::string& sl) {
  const size_t d = c->d, R = c->R;
  RGCN_TRY(create_basis_layer(c, lb, sl, nullptr));
  // gcn_basis_plus_diag.py:42-47: the BACKWARD table comes first in get_weights(); device: [2R][d], forward first
  RGCN_TRY(dmalloc(c, c->pool, &lb.dtab, 2 * R * d, true));
  RGCN_TRY(dmalloc(c, c->pool, &lb.gdtab, 2 * R * d, true));
  add_param(c, "D_b" + sl, {(int64_t)R, (int64_t)d}, lb.dtab + R * d, lb.gdtab + R * d, LAYOUT_PLAIN);
  add_param(c, "D_f" + sl, {(int64_t)R, (int64_t)d}, lb.dtab, lb.gdtab, LAYOUT_PLAIN);
  return RGCN_OK;
}

// what every layer form but the one-hot first layer ends with: W_self and the fragment tables, the bias, the highway pair
static rgcn_status create_layer_tail(rgcn_ctx* c, LayerBufs& lb, const std::string& sl, float* repl) {
  const size_t d = c->d;
  const bool tdiag = c->kind == RGCN_KIND_BASIS_TDIAG, pdiag = c->kind == RGCN_KIND_BASIS_PDIAG;
  RGCN_TRY(dmalloc(c, c->pool, &lb.wself, d * d, true));
  {      // fragment tables (allocated here: a capture may be the first call that needs them)
    const size_t ws = 16 * gemm_bfrag_words((int)d, (int)d);
    RGCN_TRY(dmalloc(c, c->pool, &lb.wself_nn, ws, false));
    RGCN_TRY(dmalloc(c, c->pool, &lb.wself_nt, ws, false));
    if (c->kind == RGCN_KIND_BASIS || pdiag) {
      const int Bd = c->B * (int)d;
      RGCN_TRY(dmalloc(c, c->pool, &lb.wrel_nn, 2 * 16 * gemm_bfrag_words(Bd, (int)d), false));
      RGCN_TRY(dmalloc(c, c->pool, &lb.wrel_nt, 2 * 16 * gemm_bfrag_words((int)d, Bd), false));
    }
  }
  if (repl) lb.gwself = repl;
  else RGCN_TRY(dmalloc(c, c->pool, &lb.gwself, d * d, true));
  RGCN_TRY(dmalloc(c, c->pool, &lb.bias, d, true));
  RGCN_TRY(dmalloc(c, c->pool, &lb.gbias, d, true));
  add_param(c, "W_self" + sl, {(int64_t)d, (int64_t)d}, lb.wself, lb.gwself, LAYOUT_PLAIN);
  add_param(c, "b" + sl, {(int64_t)d}, lb.bias, lb.gbias, LAYOUT_PLAIN);
  c->params.back().no_grad = !(tdiag || pdiag);      // (BasisGcnTimesDiag and BasisGcnWithDiag add their bias)
  if (c->highway) {      // HighwayLayer.local_get_weights (highway_layer.py): [W, b], behind the layer it wraps
    RGCN_TRY(dmalloc(c, c->pool, &lb.whw, d * d, true));
    RGCN_TRY(dmalloc(c, c->pool, &lb.gwhw, d * d, true));
    RGCN_TRY(dmalloc(c, c->pool, &lb.bhw, d, true));
    RGCN_TRY(dmalloc(c, c->pool, &lb.gbhw, d, true));
    add_param(c, "W_highway" + sl, {(int64_t)d, (int64_t)d}, lb.whw, lb.gwhw, LAYOUT_PLAIN);
    add_param(c, "b_highway" + sl, {(int64_t)d}, lb.bhw, lb.gbhw, LAYOUT_PLAIN);
  }
  return RGCN_OK;
}

// the parameter table in Model.get_weights() order: the input layer, then layer after layer
static rgcn_status create_params(rgcn_ctx* c) {
  // every [V,d] buffer carries V_pad rows (== V on one GPU): the collectives work on world equal chunks, the
  // padding rows stay zero
  const size_t V = c->V, d = c->d, Vd = (size_t)c->V_pad * d;
  if (!c->onehot) {      // (one-hot input: no AffineTransform under the layers, model_builder.py:140-165)
    RGCN_TRY(dmalloc(c, c->pool, &c->w_emb, Vd, true));
    RGCN_TRY(dmalloc(c, c->pool, &c->g_emb, Vd, true));
    RGCN_TRY(dmalloc(c, c->pool, &c->b_emb, d, true));
    RGCN_TRY(dmalloc(c, c->pool, &c->gb_emb, d, true));
    add_param(c, "W_emb", {(int64_t)V, (int64_t)d}, c->w_emb, c->g_emb, LAYOUT_PLAIN);
    add_param(c, "b_emb", {(int64_t)d}, c->b_emb, c->gb_emb, LAYOUT_PLAIN);
  }
  c->layers.resize(c->L + 1);
  // world > 1: the gradients every rank holds a partial sum of -- W_self, and the basis tensors -- sit in ONE
  // allocation, layer after layer, so that the backward pass ends with one all-reduce instead of 2-3 per layer
  const size_t repl_per_layer = d * d + (c->kind == RGCN_KIND_BASIS ? 2 * (size_t)c->cfg.num_bases * d * d : 0);
  if (c->world > 1) {
    c->repl_grads_floats = repl_per_layer * c->L;
    RGCN_TRY(dmalloc(c, c->pool, &c->repl_grads, c->repl_grads_floats, true));
  }
  for (int l = 1; l <= c->L; ++l) {
    LayerBufs& lb = c->layers[l];
    const std::string sl = std::to_string(l);
    float* repl = c->repl_grads ? c->repl_grads + repl_per_layer * (l - 1) : nullptr;
    if (c->onehot && l == 1) {
      RGCN_TRY(create_onehot_layer(c, lb));
      continue;
    }
    switch (c->kind) {
      case RGCN_KIND_BLOCK: RGCN_TRY(create_block_layer(c, lb, sl)); break;
      case RGCN_KIND_BASIS_TDIAG: RGCN_TRY(create_tdiag_layer(c, lb, sl)); break;
      case RGCN_KIND_BASIS_PDIAG: RGCN_TRY(create_pdiag_layer(c, lb, sl)); break;
      default: RGCN_TRY(create_basis_layer(c, lb, sl, repl)); break;
    }
    RGCN_TRY(create_layer_tail(c, lb, sl, repl));
  }
  return RGCN_OK;
}

// W_relation (the decoder's, behind the layers in get_weights()) and what every kind keeps per layer and per pass
static rgcn_status create_activations(rgcn_ctx* c) {
  const size_t V = c->V, d = c->d, dc = c->dc, Vd = (size_t)c->V_pad * d, Vc = (size_t)c->V_pad * dc;
  if (c->out_layer) {      // the output transform (model_builder.py:170-177): [W, b] of the AffineTransform under RelationEmbedding
    RGCN_TRY(dmalloc(c, c->pool, &c->w_out, d * dc, true));
    RGCN_TRY(dmalloc(c, c->pool, &c->g_w_out, d * dc, true));
    RGCN_TRY(dmalloc(c, c->pool, &c->b_out, dc, true));
    RGCN_TRY(dmalloc(c, c->pool, &c->g_b_out, dc, true));
    RGCN_TRY(dmalloc(c, c->pool, &c->wout_nn, 16 * gemm_bfrag_words((int)d, (int)dc), false));
    add_param(c, "W_out", {(int64_t)d, (int64_t)dc}, c->w_out, c->g_w_out, LAYOUT_PLAIN);
    add_param(c, "b_out", {(int64_t)dc}, c->b_out, c->g_b_out, LAYOUT_PLAIN);
  }
  RGCN_TRY(dmalloc(c, c->pool, &c->w_rel, Vc, true));
  RGCN_TRY(dmalloc(c, c->pool, &c->g_rel, Vc, true));
  add_param(c, "W_relation", {(int64_t)V, (int64_t)dc}, c->w_rel, c->g_rel, LAYOUT_PLAIN);
  c->H.assign(c->L + 1, nullptr);
  for (int l = c->onehot ? 1 : 0; l <= c->L; ++l) RGCN_TRY(dmalloc(c, c->pool, &c->H[l], Vd, true));   // (one-hot input: no H_0)
  c->codes = c->H[c->L];
  if (c->out_layer) {
    RGCN_TRY(dmalloc(c, c->pool, &c->codes, Vc, true));
    RGCN_TRY(dmalloc(c, c->pool, &c->out_dh, Vd, true));
  }
  RGCN_TRY(dmalloc(c, c->pool, &c->self_buf, Vd, true));
  if (c->highway) {
    c->hw_N.assign(c->L + 1, nullptr);
    c->hw_T.assign(c->L + 1, nullptr);
    for (int l = 1; l <= c->L; ++l) {
      RGCN_TRY(dmalloc(c, c->pool, &c->hw_N[l], Vd, true));
      RGCN_TRY(dmalloc(c, c->pool, &c->hw_T[l], Vd, true));
    }
    for (int k = 0; k < 2; ++k) RGCN_TRY(dmalloc(c, c->pool, &c->hw_dz[k], Vd, true));
    RGCN_TRY(dmalloc(c, c->pool, &c->hw_carry, Vd, true));
  }
  if (c->world > 1) RGCN_TRY(dmalloc(c, c->pool, &c->exch, Vd, true));
  for (int k = 0; k < 2; ++k) {
    RGCN_TRY(dmalloc(c, c->pool, &c->dbuf[k], Vd, true));
    RGCN_TRY(dmalloc(c, c->pool, &c->dsbuf[k], Vd, true));
  }
  return RGCN_OK;
}

// The scratch of each kind.  M: message capacity; max_rel_chunks: most relation chunks a graph that fits can have; slab: the
// split-K slab floats the kind's own weight-gradient GEMM needs, where that is more than the dW_self GEMM's
static rgcn_status create_block_scratch(rgcn_ctx* c, size_t M, size_t max_rel_chunks) {
  RGCN_TRY(dmalloc(c, c->pool, &c->msgbuf, (M ? M : 1) * c->d, false));
  const size_t per_rel = (size_t)c->sd * c->sd * c->nb;
  c->slab_dw_floats = max_rel_chunks * per_rel;
  return dmalloc(c, c->pool, &c->slab_dw, c->slab_dw_floats, false);
}

static rgcn_status create_tdiag_scratch(rgcn_ctx* c, size_t max_rel_chunks, size_t& slab) {
  const size_t V = c->V, d = c->d;
  const size_t pd = 2 * V * (size_t)c->B * d;      // [2][V][B.d]
  c->tdiag_P.assign(c->L + 1, nullptr);
  for (int l = 1; l <= c->L; ++l) RGCN_TRY(dmalloc(c, c->pool, &c->tdiag_P[l], pd, true));
  RGCN_TRY(dmalloc(c, c->pool, &c->tdiag_dP, pd, true));
  RGCN_TRY(dmalloc(c, c->pool, &c->tdiag_dh, 2 * V * d, true));
  const size_t s2 = 16 * 2 * (size_t)c->B * d * d;      // dW_dir = H^T . dP_dir: two groups, at most 16 slabs each
  if (s2 > slab) slab = s2;
  c->slab_dw_floats = max_rel_chunks * (size_t)c->B * d;      // per-chunk partials of dG
  return dmalloc(c, c->pool, &c->slab_dw, c->slab_dw_floats, false);
}

// BASIS_PDIAG on top of the basis kind's: the chunk slabs of dC [chunks][B] and, behind them at a 16-byte boundary, of dD
// [chunks][d]; the mixing table of every layer, the diagonal aggregate, da and the row-local part of dH
static rgcn_status create_pdiag_extras(rgcn_ctx* c, size_t max_rel_chunks) {
  const size_t V = c->V, d = c->d;
  const size_t dc = (max_rel_chunks * (size_t)c->B + 3) / 4 * 4;
  c->slab_dw_floats = dc + max_rel_chunks * d;
  c->pdiag_slab_chunks = max_rel_chunks;
  RGCN_TRY(dmalloc(c, c->pool, &c->slab_dw, c->slab_dw_floats, false));
  c->pdiag_slab_dd = c->slab_dw + dc;
  c->pdiag_a.assign(c->L + 1, nullptr);
  for (int l = 1; l <= c->L; ++l) RGCN_TRY(dmalloc(c, c->pool, &c->pdiag_a[l], 2 * V * (size_t)c->B, true));
  RGCN_TRY(dmalloc(c, c->pool, &c->pdiag_da, 2 * V * (size_t)c->B, true));
  RGCN_TRY(dmalloc(c, c->pool, &c->pdiag_agg, V * d, true));
  return dmalloc(c, c->pool, &c->pdiag_dh, V * d, true);
}

static rgcn_status create_basis_scratch(rgcn_ctx* c, size_t max_rel_chunks, size_t& slab) {
  const size_t V = c->V, d = c->d;
  const size_t zc = 2 * (size_t)c->B * d;
  RGCN_TRY(dmalloc(c, c->pool, &c->msgbuf2, V * zc, true));
  // aggbuf [2][V][d]: unit products (forward), gathered upstream rows (backward)
  RGCN_TRY(dmalloc(c, c->pool, &c->aggbuf, 2 * V * d, true));
  c->zsave.assign(c->L + 1, nullptr);
  // (a one-hot layer 1 has no Z)
  for (int l = c->onehot ? 2 : 1; l <= c->L; ++l) RGCN_TRY(dmalloc(c, c->pool, &c->zsave[l], V * zc, true));
  // dW'_dir = Zc_dir^T . Dc_dir: two groups, split over V as units_product_dw asks (auto_split_k: past 16 slabs at few
  // tiles and many rows, e.g. 35 at B = 1, d = 260, V >= 4480), never fewer than 16
  const size_t s2 = (size_t)std::max(16, auto_split_k((int)zc, (int)d, (int)V)) * zc * d;
  if (s2 > slab) slab = s2;
  if (c->kind == RGCN_KIND_BASIS_PDIAG) return create_pdiag_extras(c, max_rel_chunks);
  c->slab_dw_floats = max_rel_chunks * (size_t)c->B;
  return dmalloc(c, c->pool, &c->slab_dw, c->slab_dw_floats, false);
}

// what every kind ends with: the split-K slabs, the staging buffer of the layout conversions, the column-sum scratch, the
// zero page, the two graph sets, the relation owner table
static rgcn_status create_shared_tail(rgcn_ctx* c, size_t slab) {
  const size_t V = c->V, d = std::max(c->d, c->dc), R = c->R, Vd = (size_t)c->V_pad * d;      // (d: the wider of the two widths)
  c->slab_floats = slab;
  RGCN_TRY(dmalloc(c, c->pool, &c->slab, slab, true));
  size_t stage = Vd;
  for (const Param& p : c->params)
    if ((size_t)p.count > stage) stage = (size_t)p.count;
  c->stage_floats = stage;
  RGCN_TRY(dmalloc(c, c->pool, &c->stage, stage, false));
  // one partial row per combine workgroup (4 rows each at worst) + the second-level partials of their sum
  c->colsum_part_floats = ((V + 3) / 4 + 1024 + 2 + ((V + 3) / 4 + 1024) / 32 + 2) * d;
  RGCN_TRY(dmalloc(c, c->pool, &c->colsum_part, 2 * c->colsum_part_floats, true));      // two halves: rgcn_ctx::colsum_half
  RGCN_TRY(dmalloc(c, c->pool, &c->zeros, 1024, true));
  for (GraphBufs* g : {&c->g, &c->g_alt}) RGCN_TRY(graph_alloc(c, *g));
  {      // the relation owner table and the error flag: one copy, both graph sets point at it
    RGCN_TRY(dmalloc(c, c->pool, &c->g.owner, R, true));
    RGCN_TRY(dmalloc(c, c->pool, &c->g.errflag, 1, true));
    c->g_alt.owner = c->g.owner;
    c->g_alt.errflag = c->g.errflag;
    std::vector<int32_t> owner(c->R);
    for (int r = 0; r < c->R; ++r) owner[r] = r % c->world;
    RGCN_TRY(to_dev(c, c->g.owner, owner.data(), sizeof(int32_t) * owner.size()));
  }
  RGCN_HIP(c, hipStreamSynchronize(c->stream));
  return RGCN_OK;
}

static rgcn_status create_impl(rgcn_ctx* c) {
  const rgcn_config& f = c->cfg;
  const ConfigVerdict verdict = check_config(f, c->highway);
  if (verdict.status != RGCN_OK) RGCN_FAIL(c, verdict.status, verdict.message);
  const ConfigVerdict out_verdict = check_output_transform(f, c->highway, c->dc);      // (dc: still the caller's code_dim)
  if (out_verdict.status != RGCN_OK) RGCN_FAIL(c, out_verdict.status, out_verdict.message);
  c->V = f.num_entities; c->R = f.num_relations; c->d = f.dim; c->L = f.num_layers; c->kind = f.kind;
  c->out_layer = c->dc > 0;
  if (!c->out_layer) c->dc = c->d;
  c->rank = f.rank; c->world = f.world;
  c->onehot = f.input_mode == RGCN_INPUT_ONEHOT;
  c->embedding = f.kind == RGCN_KIND_EMBEDDING;
  // messages per relation chunk: 48 at minibatch scale; grows with the capacity so that a full-graph
  // context does not cut a popular relation into thousands of chunks
  if (2 * f.max_edges > 65536) c->chunk = 48 * (int)((2 * f.max_edges + 65535) / 65536);
  if (c->kind == RGCN_KIND_BLOCK) {
    c->nb = f.num_bases;
    c->sd = c->d / c->nb;
    RGCN_TRY(block_geometry(c));
  } else {
    c->B = f.num_bases;
  }
  // equal row chunks (the reduce-scatter / all-gather want them equal): rank g finishes rows [g * shard_rows, +shard_rows)
  c->shard_rows = (c->V + c->world - 1) / c->world;
  c->V_pad = c->shard_rows * c->world;
  c->row_lo = std::min(c->V, c->rank * c->shard_rows);
  c->row_hi = std::min(c->V, c->row_lo + c->shard_rows);

  RGCN_TRY(create_streams(c));
  if (c->embedding) return create_embedding(c);
  RGCN_HIP(c, hipEventCreateWithFlags(&c->ev_gather, hipEventDisableTiming));
  RGCN_TRY(create_params(c));
  RGCN_TRY(create_activations(c));
  const size_t M = 2 * (size_t)f.max_edges;
  size_t slab = 64 * (size_t)c->d * c->d;   // split-K slabs of the dW_self GEMM
  if (c->out_layer) slab = std::max(slab, 64 * (size_t)c->d * c->dc);      // ... and of the dW_out GEMM ([d, dc], as many slabs at most)
  // most relation chunks any graph that fits the context can have: the chunk size follows the graph's own size
  // (graph_build), so a graph of 65536 messages cut at 48 can have more chunks than the largest graph cut coarser
  const size_t max_rel_chunks = std::max((M + c->chunk - 1) / c->chunk, (std::min<size_t>(M, 65536) + 47) / 48) + 2 * (size_t)c->R;
  switch (c->kind) {
    case RGCN_KIND_BLOCK: RGCN_TRY(create_block_scratch(c, M, max_rel_chunks)); break;
    case RGCN_KIND_BASIS_TDIAG: RGCN_TRY(create_tdiag_scratch(c, max_rel_chunks, slab)); break;
    default: RGCN_TRY(create_basis_scratch(c, max_rel_chunks, slab)); break;      // (BASIS_PDIAG: with its extras)
  }
  return create_shared_tail(c, slab);
}

// ---------------------------------------------------------------- layout conversion
static rgcn_status param_upload(rgcn_ctx* c, const Param& p, float* dst, const float* host) {
  c->weights_version += 1;       // derived copies (the block-major weight tables) are stale now
  if (p.layout == LAYOUT_PLAIN) return to_dev(c, dst, host, sizeof(float) * p.count);
  RGCN_TRY(to_dev(c, c->stage, host, sizeof(float) * p.count));
  if (p.layout == LAYOUT_BLOCK_T) RGCN_TRY(block_to_device_layout(c, c->stage, dst, c->R));
  else RGCN_TRY(basis_to_device_layout(c, c->stage, dst));
  RGCN_HIP(c, hipStreamSynchronize(c->stream));
  return RGCN_OK;
}
static rgcn_status param_download(rgcn_ctx* c, const Param& p, const float* src, float* host) {
  if (p.layout == LAYOUT_PLAIN) return to_host(c, host, src, sizeof(float) * p.count);
  if (p.layout == LAYOUT_BLOCK_T) RGCN_TRY(block_from_device_layout(c, src, c->stage, c->R));
  else RGCN_TRY(basis_from_device_layout(c, src, c->stage));
  return to_host(c, host, c->stage, sizeof(float) * p.count);
}

}  // namespace rgcn

using namespace rgcn;

// ================================================================= C ABI

extern "C" {

int32_t rgcn_abi_version(void) { return RGCN_ABI_VERSION; }

rgcn_status rgcn_create(const rgcn_config* cfg, rgcn_ctx** out) { return rgcn_create_ex(cfg, nullptr, out); }

rgcn_status rgcn_create_ex(const rgcn_config* cfg, const rgcn_config_ext* ext, rgcn_ctx** out) {
  if (!cfg || !out) { set_global_error("rgcn_create: NULL argument"); return RGCN_ERR_INVALID; }
  *out = nullptr;
  // 8: the layout before code_dim (struct_size, skip_mode), read as code_dim = 0
  if (ext && ext->struct_size != (int32_t)sizeof(rgcn_config_ext) && ext->struct_size != 8) {
    set_global_error("rgcn_create_ex: rgcn_config_ext::struct_size is neither sizeof(rgcn_config_ext) nor 8 (the layout "
                     "before code_dim)");
    return RGCN_ERR_INVALID;
  }
  if (ext && ext->skip_mode != RGCN_SKIP_NONE && ext->skip_mode != RGCN_SKIP_HIGHWAY) {
    set_global_error("rgcn_create_ex: unknown skip_mode (0: RGCN_SKIP_NONE, 1: RGCN_SKIP_HIGHWAY)");
    return RGCN_ERR_INVALID;
  }
  rgcn_ctx* c = new (std::nothrow) rgcn_ctx();
  if (!c) { set_global_error("out of host memory"); return RGCN_ERR_NOMEM; }
  c->cfg = *cfg;
  c->highway = ext && ext->skip_mode == RGCN_SKIP_HIGHWAY;
  c->dc = ext && ext->struct_size == (int32_t)sizeof(rgcn_config_ext) ? ext->code_dim : 0;      // (create_impl checks it)
  rgcn_status s = create_impl(c);
  if (s != RGCN_OK) {
    set_global_error(c->err);
    free_all(c);
    return s;
  }
  *out = c;
  return RGCN_OK;
}

rgcn_status rgcn_destroy(rgcn_ctx* ctx) {
  if (!ctx) return RGCN_OK;
  free_all(ctx);
  return RGCN_OK;
}

const char* rgcn_last_error(const rgcn_ctx* ctx) {
  if (ctx) return ctx->err.c_str();
  static thread_local std::string copy;
  std::lock_guard<std::mutex> lk(g_err_mu);
  copy = g_err;
  return copy.c_str();
}

rgcn_status rgcn_sync(rgcn_ctx* c) {
  RGCN_NEED(c);
  return check_dev_flag(c);
}

int32_t rgcn_param_count(const rgcn_ctx* c) { return c ? (int32_t)c->params.size() : 0; }

rgcn_status rgcn_param_info(const rgcn_ctx* c, int32_t index, char* name, int32_t name_cap,
                            int64_t shape[4], int32_t* ndim) {
  if (!c || index < 0 || index >= (int32_t)c->params.size()) return RGCN_ERR_INVALID;
  const Param& p = c->params[index];
  if (name && name_cap > 0) {
    strncpy(name, p.name.c_str(), (size_t)name_cap - 1);
    name[name_cap - 1] = 0;
  }
  if (shape) for (int i = 0; i < 4; ++i) shape[i] = p.shape[i];
  if (ndim) *ndim = p.ndim;
  return RGCN_OK;
}

static rgcn_status param_check(rgcn_ctx* c, int32_t index, const void* host, int64_t count) {
  if (index < 0 || index >= (int32_t)c->params.size()) RGCN_FAIL(c, RGCN_ERR_INVALID, "parameter index out of range");
  if (!host) RGCN_FAIL(c, RGCN_ERR_INVALID, "NULL host pointer");
  if (count != c->params[index].count)
    RGCN_FAIL(c, RGCN_ERR_INVALID, "element count does not match parameter " + c->params[index].name);
  return RGCN_OK;
}

rgcn_status rgcn_set_param(rgcn_ctx* c, int32_t index, const float* host, int64_t count) {
  RGCN_NEED(c);
  RGCN_TRY(param_check(c, index, host, count));
  return param_upload(c, c->params[index], c->params[index].val, host);
}
rgcn_status rgcn_get_param(rgcn_ctx* c, int32_t index, float* host, int64_t count) {
  RGCN_NEED(c);
  RGCN_TRY(param_check(c, index, host, count));
  return param_download(c, c->params[index], c->params[index].val, host);
}
rgcn_status rgcn_get_grad(rgcn_ctx* c, int32_t index, float* host, int64_t count) {
  RGCN_NEED(c);
  RGCN_TRY(param_check(c, index, host, count));
  RGCN_TRY(check_dev_flag(c));
  return param_download(c, c->params[index], c->params[index].grad, host);
}

rgcn_status rgcn_set_graph(rgcn_ctx* c, const int32_t* tri, int64_t E) {
  RGCN_NEED(c);
  RGCN_NO_EMBEDDING(c, "rgcn_set_graph");
  if (E < 0 || E > c->cfg.max_edges) RGCN_FAIL(c, RGCN_ERR_INVALID, "num_edges outside [0, max_edges]");
  if (E > 0 && !tri) RGCN_FAIL(c, RGCN_ERR_INVALID, "NULL triples");
  for (int64_t e = 0; e < E; ++e) {
    const int32_t s = tri[3 * e], r = tri[3 * e + 1], o = tri[3 * e + 2];
    if (s < 0 || s >= c->V || o < 0 || o >= c->V || r < 0 || r >= c->R)
      RGCN_FAIL(c, RGCN_ERR_INVALID, "graph_edges row " + std::to_string(e) + " has an id out of range");
  }
  RGCN_TRY(join_abandoned_side_work(c));      // (they read the message lists the build rewrites)
  if (E > 0) RGCN_TRY(to_dev(c, c->g.triples, tri, sizeof(int32_t) * 3 * (size_t)E));
  return graph_build(c, c->g.triples, E);
}

rgcn_status rgcn_set_graph_device(rgcn_ctx* c, const int32_t* tri_dev, int64_t E) {
  RGCN_NEED(c);
  RGCN_NO_EMBEDDING(c, "rgcn_set_graph_device");
  if (E < 0 || E > c->cfg.max_edges) RGCN_FAIL(c, RGCN_ERR_INVALID, "num_edges outside [0, max_edges]");
  if (E > 0 && !tri_dev) RGCN_FAIL(c, RGCN_ERR_INVALID, "NULL triples");
  RGCN_TRY(join_abandoned_side_work(c));
  return graph_build(c, tri_dev, E);
}

rgcn_status rgcn_forward(rgcn_ctx* c, int32_t train, uint64_t seed, const uint8_t* masks) {
  RGCN_NEED(c);
  return forward_all(c, train, seed, masks);
}

rgcn_status rgcn_get_activation(rgcn_ctx* c, int32_t layer, float* host, int64_t count) {
  RGCN_NEED(c);
  if (layer < 0 || layer > c->L) RGCN_FAIL(c, RGCN_ERR_INVALID, "layer out of range");
  if (c->onehot && layer == 0) RGCN_FAIL(c, RGCN_ERR_INVALID, "RGCN_INPUT_ONEHOT: there is no H_0 (the first layer reads entity ids)");
  if (!host || count != (int64_t)c->V * c->d) RGCN_FAIL(c, RGCN_ERR_INVALID, "need a [V,d] host buffer");
  if (!c->fwd_done) RGCN_FAIL(c, RGCN_ERR_STATE, "no completed forward pass");
  RGCN_TRY(check_dev_flag(c));
  return to_host(c, host, c->H[layer], sizeof(float) * (size_t)count);
}
rgcn_status rgcn_get_codes(rgcn_ctx* c, float* host, int64_t count) {
  if (!c) return RGCN_ERR_INVALID;
  if (!c->out_layer) return rgcn_get_activation(c, c->L, host, count);
  RGCN_NEED(c);
  if (!host || count != (int64_t)c->V * c->dc) RGCN_FAIL(c, RGCN_ERR_INVALID, "need a [V,CodeDimension] host buffer");
  if (!c->fwd_done) RGCN_FAIL(c, RGCN_ERR_STATE, "no completed forward pass");
  RGCN_TRY(check_dev_flag(c));
  return to_host(c, host, c->codes, sizeof(float) * (size_t)count);
}
const float* rgcn_codes_device(rgcn_ctx* c) { return c ? c->codes : nullptr; }

rgcn_status rgcn_get_dropout_mask(rgcn_ctx* c, int32_t layer, uint8_t* host, int64_t count) {
  RGCN_NEED(c);
  if (layer < 1 || layer > c->L) RGCN_FAIL(c, RGCN_ERR_INVALID, "layer out of range");
  if (!host || count != (int64_t)c->V * c->d) RGCN_FAIL(c, RGCN_ERR_INVALID, "need a [V,d] host buffer");
  DropSpec ds = make_drop(c, layer, true);
  uint8_t* tmp = reinterpret_cast<uint8_t*>(c->stage);
  RGCN_TRY(materialize_mask(c, ds, tmp, count));
  return to_host(c, host, tmp, (size_t)count);
}

rgcn_status rgcn_backward_device(rgcn_ctx* c, const float* dcodes_dev) {
  RGCN_NEED(c);
  return backward_all(c, dcodes_dev);
}
rgcn_status rgcn_backward(rgcn_ctx* c, const float* dcodes_host, int64_t count) {
  RGCN_NEED(c);
  if (!dcodes_host || count != (int64_t)c->V * c->dc) RGCN_FAIL(c, RGCN_ERR_INVALID, "dcodes must be [V,d] ([V,CodeDimension] under an output transform)");
  if (!c->dcodes_own) RGCN_TRY(dmalloc(c, c->pool, &c->dcodes_own, (size_t)count, false));
  RGCN_TRY(join_abandoned_side_work(c));      // (unjoined side kernels may read the previous dcodes)
  RGCN_TRY(to_dev(c, c->dcodes_own, dcodes_host, sizeof(float) * (size_t)count));
  return backward_all(c, c->dcodes_own);
}

// Start of a step: mark the point a prefetch may fork from, then adopt the prefetched structures of this
// graph or build them in line.  While a hipGraph is being captured, events recorded BEFORE the capture began
// must not be waited on (the replayed graph is ordered behind everything earlier on the stream anyway).
// keep >= 0: the graph is the edge-dropout subset (keep of the E batch edges, generator key eseed) of tri_dev.
// fork_point: something of this step forks from its start (the decoder's batch preparation; inside a capture, the prefetch):
// an encoder step outside a capture has no such fork and saves the main stream the packet.
// Ordering against the step before: every packet between two kernels of the main stream -- record or
// wait, fired or not -- costs the chain ~6 us (profiles/r07_deferred_joins.md), so an encoder step ends unjoined and this
// one starts with ONE wait: for the prefetched set's ev_ready and, through side stream 0, for the side kernels that read
// what the forward pass overwrites.  A graph built in line takes the full join first: the build rewrites the message lists.
static rgcn_status step_begin(rgcn_ctx* c, const int32_t* tri_dev, int64_t E, bool fork_point, int64_t keep = -1,
                              uint64_t eseed = 0) {
  const bool adopt = c->g_alt.pf_valid && c->g_alt.pf_tri == tri_dev && c->g_alt.pf_E == E && c->g_alt.pf_keep == keep &&
                     (keep < 0 || c->g_alt.pf_eseed == eseed);
  // a build in line rewrites the message lists unjoined side kernels may still read; a prefetched set was built behind
  // its own ev_free, which covers them (step_end), and the forward pass takes the join it needs (join_side_reads)
  if (!adopt) RGCN_TRY(join_abandoned_side_work(c));
  if (fork_point || c->capturing) RGCN_HIP(c, hipEventRecord(c->ev_step_begin, c->main_stream));
  c->step_begin_in_capture = c->capturing;
  if (adopt) {
    // the structures for this graph were prepared beside the previous step: swap them in
    std::swap(c->g, c->g_alt);
    c->g.pf_valid = false;
    c->fwd_done = false;
    if (c->capturing) {
      if (c->g.ready_in_capture) RGCN_HIP(c, hipStreamWaitEvent(c->main_stream, c->g.ev_ready, 0));
      return RGCN_OK;
    }
    return join_side_reads(c, c->g.ev_ready);
  }
  return keep < 0 ? graph_build(c, tri_dev, E) : graph_build_dropout(c, tri_dev, E, keep, eseed, nullptr);
}
// ev_free: the graph set may be rebuilt.  After a deferred end of step the side kernels still read it: side stream 1, which
// bwd_end put behind the main stream's last kernel and behind side stream 0, takes the record -- the prefetch stream waits
// for all three, the main stream for nothing.
static rgcn_status step_end(rgcn_ctx* c) {
  RGCN_HIP(c, hipEventRecord(c->g.ev_free, c->side_state == rgcn_ctx::SIDE_RECORDED ? c->aux[1] : c->main_stream));
  c->g.free_in_capture = c->capturing;
  return RGCN_OK;
}

rgcn_status rgcn_step_device(rgcn_ctx* c, const int32_t* tri_dev, int64_t E, int32_t train,
                             uint64_t seed, const float* dcodes_dev) {
  RGCN_NEED(c);
  RGCN_NO_EMBEDDING(c, "rgcn_step_device");
  if (E < 0 || E > c->cfg.max_edges) RGCN_FAIL(c, RGCN_ERR_INVALID, "num_edges outside [0, max_edges]");
  RGCN_TRY(step_begin(c, tri_dev, E, false));
  // (Round 5 tried forming the top layer's dS = dL/dcodes * dropout_L -- which depends on the caller's gradient and the seed
  // only -- on a side stream beside the forward pass: 0.567 ms per step against 0.559 on the same box.  A fork + join costs
  // the main stream more than the 13 us pass it hides.)
  RGCN_TRY(forward_all(c, train, seed, nullptr));
  // The step ends without a join (bwd_layer_partial, bwd_end): its caller gets the gradients through calls that join.
  c->defer_end_joins = true;
  const rgcn_status bs = backward_all(c, dcodes_dev);
  c->defer_end_joins = false;
  RGCN_TRY(bs);
  return step_end(c);
}

// ---- decoder / optimizer / whole train step ("next" rows f1, f2) ---------------------------------
rgcn_status rgcn_decoder_reserve(rgcn_ctx* c, int64_t max_triples) {
  RGCN_NEED(c);
  if (max_triples <= 0 || max_triples > RGCN_MAX_DECODER_TRIPLES) RGCN_FAIL(c, RGCN_ERR_INVALID, "max_triples out of range");
  RGCN_TRY(sync_all(c));
  return decoder_reserve(c, max_triples);
}

rgcn_status rgcn_decoder_loss_backward_device(rgcn_ctx* c, const int32_t* X_dev, const float* Y_dev, int64_t N,
                                              float reg_param) {
  RGCN_NEED(c);
  if (!c->fwd_done) RGCN_FAIL(c, RGCN_ERR_STATE, "the decoder needs a completed rgcn_forward");
  if (!X_dev || !Y_dev || N <= 0) RGCN_FAIL(c, RGCN_ERR_INVALID, "bad decoder batch");
  // world > 1: the codes are replicated after the last layer's exchange, so every rank runs the same decoder
  // pass on the same batch and holds identical dL/dcodes and dL/dW_relation (the kernels are deterministic)
  if (c->dec.maxN < N) RGCN_FAIL(c, RGCN_ERR_STATE, "call rgcn_decoder_reserve(ctx, max_triples) first");
  RGCN_TRY(decoder_prepare(c, X_dev, N));
  RGCN_TRY(decoder_compute(c, c->codes, Y_dev, reg_param));
  RGCN_TRY(stream_join(c, 2));      // the relation gradient ran on its own side stream
  c->dec.loss_valid = true;
  return RGCN_OK;
}

rgcn_status rgcn_decoder_loss_backward_weighted_device(rgcn_ctx* c, const int32_t* X_dev, const float* Y_dev,
                                                       const float* w_dev, int64_t N, float reg_param) {
  if (!w_dev) return rgcn_decoder_loss_backward_device(c, X_dev, Y_dev, N, reg_param);
  RGCN_NEED(c);
  if (!c->fwd_done) RGCN_FAIL(c, RGCN_ERR_STATE, "the decoder needs a completed rgcn_forward");
  if (!X_dev || !Y_dev || N <= 0) RGCN_FAIL(c, RGCN_ERR_INVALID, "bad decoder batch");
  if (c->dec.maxN < N) RGCN_FAIL(c, RGCN_ERR_STATE, "call rgcn_decoder_reserve(ctx, max_triples) first");
  RGCN_TRY(adversarial_check_weights(c, w_dev, N));
  RGCN_TRY(decoder_prepare(c, X_dev, N));
  RGCN_TRY(decoder_compute(c, c->codes, Y_dev, reg_param, nullptr, nullptr, w_dev));
  RGCN_TRY(stream_join(c, 2));      // the relation gradient ran on its own side stream
  c->dec.loss_valid = true;
  return RGCN_OK;
}

// ---- self-adversarial negatives: the stand-alone weights, the mode of the fused steps
static bool adv_temperature_ok(float t) { return t >= 0.f && t <= 3.0e38f; }      // (false for NaN and for infinity)

rgcn_status rgcn_adversarial_weights_device(rgcn_ctx* c, const int32_t* X_dev, int64_t N, int64_t P, float temperature,
                                            float* w_out_dev) {
  RGCN_NEED(c);
  if (!X_dev || !w_out_dev) RGCN_FAIL(c, RGCN_ERR_INVALID, "NULL batch or output");
  if (N <= 0 || N > RGCN_MAX_DECODER_TRIPLES || P <= 0 || N % P != 0)
    RGCN_FAIL(c, RGCN_ERR_INVALID, "num_triples must be a positive multiple of num_positives");
  if (!adv_temperature_ok(temperature)) RGCN_FAIL(c, RGCN_ERR_INVALID, "the temperature must be finite and not negative");
  if (!c->fwd_done) RGCN_FAIL(c, RGCN_ERR_STATE, "the weights are those of the last forward pass's codes: call rgcn_forward first");
  return adversarial_weights(c, c->embedding ? c->H[0] : c->codes, X_dev, nullptr, N, P, temperature, w_out_dev);
}

rgcn_status rgcn_set_adversarial_negatives(rgcn_ctx* c, float temperature, int64_t num_positives) {
  RGCN_NEED(c);
  if (!adv_temperature_ok(temperature)) RGCN_FAIL(c, RGCN_ERR_INVALID, "the temperature must be finite and not negative");
  if (num_positives < 0 || num_positives > RGCN_MAX_DECODER_TRIPLES) RGCN_FAIL(c, RGCN_ERR_INVALID, "num_positives out of range");
  if (temperature > 0.f && c->capturing) RGCN_FAIL(c, RGCN_ERR_STATE, "not while a hipGraph is being captured");
  c->adv.temperature = temperature;
  c->adv.step_positives = num_positives;
  return RGCN_OK;
}

// what a fused step checks before it queues anything while the mode is on (rgcn_set_adversarial_negatives, temperature
// > 0), P the step's positives; then the weight buffer follows the decoder's reserve
static rgcn_status adv_step_check(rgcn_ctx* c, int64_t N, int64_t P) {
  // (a sharded step cuts the batch by rows, and with them the groups)
  if (c->world > 1) RGCN_FAIL(c, RGCN_ERR_UNSUPPORTED, "adversarial negatives in the step of a relation-sharded context (world > 1)");
  if (c->capturing) RGCN_FAIL(c, RGCN_ERR_STATE, "adversarial negatives are not built for a hipGraph capture");
  if (P <= 0) RGCN_FAIL(c, RGCN_ERR_STATE, "rgcn_set_adversarial_negatives was given num_positives = 0: the minibatch step only");
  if (N % P != 0) RGCN_FAIL(c, RGCN_ERR_INVALID, "adversarial negatives: the batch's rows are no multiple of num_positives");
  return RGCN_OK;
}
static rgcn_status adv_step_buffer(rgcn_ctx* c) {
  if (c->adv.w && c->adv.cap >= c->dec.maxN) return RGCN_OK;
  RGCN_TRY(sync_all(c));      // (an earlier step may still read the buffer this replaces)
  return adversarial_reserve(c, c->dec.maxN);
}

const float* rgcn_dcodes_device(rgcn_ctx* c) { return c ? c->dcodes_own : nullptr; }

rgcn_status rgcn_get_loss(rgcn_ctx* c, double* loss) {
  RGCN_NEED(c);
  if (!loss) RGCN_FAIL(c, RGCN_ERR_INVALID, "NULL output");
  if (!c->dec.loss_valid) RGCN_FAIL(c, RGCN_ERR_STATE, "no decoder pass has run");
  if (c->capturing) RGCN_FAIL(c, RGCN_ERR_STATE, "host transfers are not allowed while a hipGraph is being captured");
  // the training loop reads the loss every iteration (optimize.py:81-88 returns it from session.run): the loss and the
  // device-side error flag come back through pinned memory with ONE wait for the main stream
  if (!c->readback_host) RGCN_HIP(c, hipHostMalloc((void**)&c->readback_host, 32, hipHostMallocDefault));
  double* h_loss = reinterpret_cast<double*>(c->readback_host);
  int32_t* h_flag = reinterpret_cast<int32_t*>(c->readback_host + 16);
  RGCN_HIP(c, hipMemcpyAsync(h_flag, c->g.errflag, sizeof(int32_t), hipMemcpyDeviceToHost, c->main_stream));
  RGCN_HIP(c, hipMemcpyAsync(h_loss, c->dec.loss, sizeof(double), hipMemcpyDeviceToHost, c->main_stream));
  RGCN_HIP(c, hipStreamSynchronize(c->main_stream));
  if (*h_flag) RGCN_TRY(check_dev_flag(c, /*main_only=*/true));      // reads it again, clears it, names the failure
  *loss = *h_loss;
  return RGCN_OK;
}

rgcn_status rgcn_negative_sample_device(rgcn_ctx* c, const int32_t* batch_dev, int64_t n, int32_t rate, uint64_t seed,
                                        int32_t* x_out_dev, float* y_out_dev) {
  RGCN_NEED(c);
  if (n < 0 || rate < 0 || rate > 1024 || (n > 0 && (!batch_dev || !x_out_dev || !y_out_dev)))
    RGCN_FAIL(c, RGCN_ERR_INVALID, "bad arguments");
  if (n * (int64_t)(rate + 1) > RGCN_MAX_DECODER_TRIPLES) RGCN_FAIL(c, RGCN_ERR_INVALID, "batch too large");
  return negative_sample(c, batch_dev, n, rate, seed, x_out_dev, y_out_dev);
}

// ---- exclusive negative sampling: the index of known positives, the stand-alone call, the mode of the fused step
rgcn_status rgcn_known_positives_reserve(rgcn_ctx* c, const int32_t* triples_host, int64_t n) {
  RGCN_NEED(c);
  if (n < 0 || (n > 0 && !triples_host)) RGCN_FAIL(c, RGCN_ERR_INVALID, "need the known positives (or num_triples = 0 to release them)");
  if (c->capturing) RGCN_FAIL(c, RGCN_ERR_STATE, "not while a hipGraph is being captured");
  RGCN_TRY(sync_all(c));      // (a sampling kernel in flight may still be reading the index this call replaces)
  return known_positives_reserve(c, triples_host, n);
}

rgcn_status rgcn_negative_sample_exclusive_device(rgcn_ctx* c, const int32_t* batch_dev, int64_t n, int32_t rate,
                                                  uint64_t seed, int32_t* x_out_dev, float* y_out_dev) {
  RGCN_NEED(c);
  if (n < 0 || rate < 0 || rate > 1024 || (n > 0 && (!batch_dev || !x_out_dev || !y_out_dev)))
    RGCN_FAIL(c, RGCN_ERR_INVALID, "bad arguments");
  if (n * (int64_t)(rate + 1) > RGCN_MAX_DECODER_TRIPLES) RGCN_FAIL(c, RGCN_ERR_INVALID, "batch too large");
  return negative_sample_exclusive(c, batch_dev, n, rate, seed, x_out_dev, y_out_dev);
}

rgcn_status rgcn_set_exclusive_negatives(rgcn_ctx* c, int32_t on) {
  RGCN_NEED(c);
  if (c->capturing) RGCN_FAIL(c, RGCN_ERR_STATE, "not while a hipGraph is being captured");
  if (on && c->known.count <= 0) RGCN_FAIL(c, RGCN_ERR_STATE, "call rgcn_known_positives_reserve first");
  c->known.exclusive = on != 0;
  return RGCN_OK;
}

// ---- relation corruptions: the stand-alone call and the mode of the fused step
// whether [dev, dev + bytes) lies inside one device allocation; a pointer the runtime cannot place is taken on trust
static bool allocation_covers(const void* dev, size_t bytes) {
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  if (hipMemGetAddressRange(&base, &size, const_cast<void*>(dev)) != hipSuccess) {
    (void)hipGetLastError();
    return true;
  }
  const char* lo = reinterpret_cast<const char*>(base);
  const char* p = reinterpret_cast<const char*>(dev);
  return p >= lo && p + bytes <= lo + size;
}

rgcn_status rgcn_negative_sample_relation_device(rgcn_ctx* c, const int32_t* batch_dev, int64_t n, int32_t rate,
                                                 int32_t relation_rate, int32_t exclusive, uint64_t seed,
                                                 int32_t* x_out_dev, float* y_out_dev) {
  RGCN_NEED(c);
  if (n < 0 || rate < 0 || rate > 1024 || relation_rate < 0 || relation_rate > 1024 ||
      (n > 0 && (!batch_dev || !x_out_dev || !y_out_dev)))
    RGCN_FAIL(c, RGCN_ERR_INVALID, "bad arguments");
  if (relation_rate > 0 && c->R < 2) RGCN_FAIL(c, RGCN_ERR_INVALID, "relation corruptions need at least two relations");
  if (n * (int64_t)(rate + 1 + relation_rate) > RGCN_MAX_DECODER_TRIPLES) RGCN_FAIL(c, RGCN_ERR_INVALID, "batch too large");
  if (c->capturing) RGCN_FAIL(c, RGCN_ERR_STATE, "not while a hipGraph is being captured");
  if (exclusive && c->known.count <= 0) RGCN_FAIL(c, RGCN_ERR_STATE, "call rgcn_known_positives_reserve first");
  return negative_sample_relation(c, batch_dev, n, rate, relation_rate, exclusive != 0, seed, x_out_dev, y_out_dev);
}

rgcn_status rgcn_set_relation_negatives(rgcn_ctx* c, int32_t relation_rate) {
  RGCN_NEED(c);
  if (relation_rate < 0 || relation_rate > 1024) RGCN_FAIL(c, RGCN_ERR_INVALID, "relation_rate outside [0, 1024]");
  if (c->capturing) RGCN_FAIL(c, RGCN_ERR_STATE, "not while a hipGraph is being captured");
  if (relation_rate > 0 && c->world > 1)
    RGCN_FAIL(c, RGCN_ERR_UNSUPPORTED, "relation corruptions in the fused step of a relation-sharded context (world > 1)");
  if (relation_rate > 0 && c->R < 2) RGCN_FAIL(c, RGCN_ERR_INVALID, "relation corruptions need at least two relations");
  c->relation_negatives = relation_rate;
  return RGCN_OK;
}

// ---- type-constrained negatives: the per-relation entity sets, the stand-alone call, the mode of the fused step
rgcn_status rgcn_type_sets_reserve(rgcn_ctx* c, const int32_t* triples_host, int64_t n) {
  RGCN_NEED(c);
  if (n < 0 || (n > 0 && !triples_host)) RGCN_FAIL(c, RGCN_ERR_INVALID, "need the triples (or num_triples = 0 to release the type sets)");
  if (c->capturing) RGCN_FAIL(c, RGCN_ERR_STATE, "not while a hipGraph is being captured");
  RGCN_TRY(sync_all(c));      // (a kernel in flight may still be reading the sets this call replaces)
  return type_sets_reserve(c, triples_host, n);
}

rgcn_status rgcn_negative_sample_typed_device(rgcn_ctx* c, const int32_t* batch_dev, int64_t n, int32_t rate,
                                              int32_t exclusive, uint64_t seed, int32_t* x_out_dev, float* y_out_dev) {
  RGCN_NEED(c);
  if (n < 0 || rate < 0 || rate > 1024 || (n > 0 && (!batch_dev || !x_out_dev || !y_out_dev)))
    RGCN_FAIL(c, RGCN_ERR_INVALID, "bad arguments");
  if (n * (int64_t)(rate + 1) > RGCN_MAX_DECODER_TRIPLES) RGCN_FAIL(c, RGCN_ERR_INVALID, "batch too large");
  if (c->capturing) RGCN_FAIL(c, RGCN_ERR_STATE, "not while a hipGraph is being captured");
  return negative_sample_typed(c, batch_dev, n, rate, 0, exclusive != 0, seed, x_out_dev, y_out_dev);
}

rgcn_status rgcn_set_typed_negatives(rgcn_ctx* c, int32_t on) {
  RGCN_NEED(c);
  if (c->capturing) RGCN_FAIL(c, RGCN_ERR_STATE, "not while a hipGraph is being captured");
  if (on && c->world > 1)
    RGCN_FAIL(c, RGCN_ERR_UNSUPPORTED, "type-constrained negatives in the fused step of a relation-sharded context (world > 1)");
  if (on && !c->types.ready) RGCN_FAIL(c, RGCN_ERR_STATE, "call rgcn_type_sets_reserve first");
  c->types.typed = on != 0;
  return RGCN_OK;
}

// ---- reciprocal relations: the stand-alone pass and the mode
rgcn_status rgcn_reciprocal_rows_device(rgcn_ctx* c, const int32_t* batch_dev, int64_t n, int32_t rate, int32_t relation_rate,
                                        uint64_t seed, int32_t* x_dev, float* y_dev) {
  RGCN_NEED(c);
  if (n < 0 || rate < 0 || rate > 1024 || relation_rate < 0 || relation_rate > 1024 ||
      (n > 0 && (!batch_dev || !x_dev || !y_dev)))
    RGCN_FAIL(c, RGCN_ERR_INVALID, "bad arguments");
  if (n * (int64_t)(rate + 2 + relation_rate) > RGCN_MAX_DECODER_TRIPLES) RGCN_FAIL(c, RGCN_ERR_INVALID, "batch too large");
  if (2 * (int64_t)c->R > c->V)
    RGCN_FAIL(c, RGCN_ERR_UNSUPPORTED, "reciprocal relations need 2 x num_relations <= num_entities rows of W_relation");
  if (c->capturing) RGCN_FAIL(c, RGCN_ERR_STATE, "not while a hipGraph is being captured");
  if (n > 0 && (!allocation_covers(x_dev, sizeof(int32_t) * 3 * (size_t)(n * (int64_t)(rate + 2 + relation_rate))) ||
                !allocation_covers(y_dev, sizeof(float) * (size_t)(n * (int64_t)(rate + 2 + relation_rate)))))
    RGCN_FAIL(c, RGCN_ERR_STATE, "the buffers must hold num_edges x (2 + negative_rate + relation_rate) rows");
  return reciprocal_rows(c, batch_dev, n, rate, relation_rate, seed, x_dev, y_dev);
}

rgcn_status rgcn_set_reciprocal_relations(rgcn_ctx* c, int32_t on) {
  RGCN_NEED(c);
  if (c->capturing)
    RGCN_FAIL(c, on ? RGCN_ERR_UNSUPPORTED : RGCN_ERR_STATE, "reciprocal relations: not while a hipGraph is being captured");
  if (on) {
    if (c->world > 1)
      RGCN_FAIL(c, RGCN_ERR_UNSUPPORTED, "reciprocal relations on a relation-sharded context (world > 1)");
    if (2 * (int64_t)c->R > c->V)
      RGCN_FAIL(c, RGCN_ERR_UNSUPPORTED, "reciprocal relations need 2 x num_relations <= num_entities rows of W_relation");
    if (c->entsm.weight > 0.f)
      RGCN_FAIL(c, RGCN_ERR_UNSUPPORTED, "reciprocal relations under the entity softmax (rgcn_set_entity_softmax): its subject rows "
                                         "and its by-relation reduction are not built for the 2 R relation rows");
  }
  if ((on != 0) == c->reciprocal) return RGCN_OK;
  RGCN_TRY(sync_all(c));      // (a step in flight still reads the decoder's buffers at their present size)
  c->reciprocal = on != 0;
  // off again: the gradient rows [R, 2 R) return to the zeros every row behind the relation bound holds
  if (!on)
    RGCN_HIP(c, hipMemsetAsync(c->g_rel + (size_t)c->R * c->dc, 0, sizeof(float) * (size_t)c->R * c->dc, c->main_stream));
  // everything sized by the relation bound follows it: rel_ptr, chunk_ptr, rb, the slab of the relation gradient
  const int64_t maxN = c->dec.maxN;
  if (maxN > 0) RGCN_TRY(decoder_reserve(c, maxN));
  return RGCN_OK;
}

// ---- the relation-softmax term: reserve, the stand-alone call, the mode of the fused steps, the host plan
rgcn_status rgcn_relation_softmax_reserve(rgcn_ctx* c, int64_t max_positives) {
  RGCN_NEED(c);
  if (max_positives <= 0 || max_positives > RGCN_MAX_DECODER_TRIPLES) RGCN_FAIL(c, RGCN_ERR_INVALID, "max_positives out of range");
  if (c->R < 2) RGCN_FAIL(c, RGCN_ERR_INVALID, "the relation softmax needs at least two relations");
  if (c->V >= (1 << 24)) RGCN_FAIL(c, RGCN_ERR_UNSUPPORTED, "relation softmax: 2^24 entities or more");
  RGCN_TRY(sync_all(c));
  return relation_softmax_reserve(c, max_positives);
}

static bool relsm_weight_ok(float w) { return w >= 0.f && w <= 3.0e38f; }      // (false for NaN and for infinity)

rgcn_status rgcn_relation_softmax_device(rgcn_ctx* c, const int32_t* pos_dev, int64_t P, float weight, int32_t exclusive) {
  RGCN_NEED(c);
  if (!pos_dev || P <= 0 || P > RGCN_MAX_DECODER_TRIPLES) RGCN_FAIL(c, RGCN_ERR_INVALID, "bad positives");
  if (!relsm_weight_ok(weight)) RGCN_FAIL(c, RGCN_ERR_INVALID, "the weight must be finite and not negative");
  if (c->R < 2) RGCN_FAIL(c, RGCN_ERR_INVALID, "the relation softmax needs at least two relations");
  if (c->world > 1) RGCN_FAIL(c, RGCN_ERR_UNSUPPORTED, "the relation softmax on a relation-sharded context (world > 1)");
  if (c->capturing) RGCN_FAIL(c, RGCN_ERR_STATE, "not while a hipGraph is being captured");
  if (!c->dec.loss_valid || !c->fwd_done)
    RGCN_FAIL(c, RGCN_ERR_STATE, "the term is added to a decoder pass: call rgcn_decoder_loss_backward_device first");
  if (c->relsm.maxP <= 0) RGCN_FAIL(c, RGCN_ERR_STATE, "call rgcn_relation_softmax_reserve first");
  if (exclusive && c->known.count <= 0) RGCN_FAIL(c, RGCN_ERR_STATE, "call rgcn_known_positives_reserve first");
  if (weight == 0.f) return RGCN_OK;
  RGCN_TRY(stream_join(c, 2));
  c->relsm.csr_X = nullptr;      // (a CSR a fused step prepared and never used is not this call's)
  RGCN_TRY(relation_softmax_compute(c, c->embedding ? c->H[0] : c->codes, pos_dev, nullptr, P, weight, exclusive != 0));
  return stream_join(c, 2);      // the last chunk's relation gradient ran on its own side stream
}

rgcn_status rgcn_set_relation_softmax(rgcn_ctx* c, float weight, int64_t num_positives, int32_t exclusive) {
  RGCN_NEED(c);
  if (!relsm_weight_ok(weight)) RGCN_FAIL(c, RGCN_ERR_INVALID, "the weight must be finite and not negative");
  if (num_positives < 0 || num_positives > RGCN_MAX_DECODER_TRIPLES) RGCN_FAIL(c, RGCN_ERR_INVALID, "num_positives out of range");
  if (weight > 0.f) {
    if (c->capturing) RGCN_FAIL(c, RGCN_ERR_STATE, "not while a hipGraph is being captured");
    if (c->R < 2) RGCN_FAIL(c, RGCN_ERR_INVALID, "the relation softmax needs at least two relations");
    if (exclusive && c->known.count <= 0) RGCN_FAIL(c, RGCN_ERR_STATE, "call rgcn_known_positives_reserve first");
  }
  c->relsm.weight = weight;
  c->relsm.step_positives = num_positives;
  c->relsm.exclusive = exclusive != 0;
  return RGCN_OK;
}

rgcn_status rgcn_relation_softmax_plan(int64_t max_positives, int32_t num_relations, int32_t code_dim, int64_t out[5]) {
  if (!out || max_positives <= 0 || num_relations <= 0 || code_dim <= 0) return RGCN_ERR_INVALID;
  const RelsmPlan p = relsm_plan(max_positives, num_relations, code_dim, kRelsmSlabFloats);      // what a context runs
  out[0] = p.chunk; out[1] = p.padded_r; out[2] = p.split_k; out[3] = kRelsmLongRow; out[4] = kRelsmPiece;
  return RGCN_OK;
}

// what a fused step checks before it queues anything while the term is on (rgcn_set_relation_softmax, weight > 0)
static rgcn_status relsm_step_check(rgcn_ctx* c) {
  if (c->world > 1) RGCN_FAIL(c, RGCN_ERR_UNSUPPORTED, "the relation softmax in the step of a relation-sharded context (world > 1)");
  if (c->capturing) RGCN_FAIL(c, RGCN_ERR_STATE, "the relation softmax is not built for a hipGraph capture");
  if (c->relsm.maxP <= 0) RGCN_FAIL(c, RGCN_ERR_STATE, "call rgcn_relation_softmax_reserve first");
  if (c->relsm.exclusive && c->known.count <= 0) RGCN_FAIL(c, RGCN_ERR_STATE, "call rgcn_known_positives_reserve first");
  return RGCN_OK;
}

// ---- the entity-softmax term: the relation term's four entry points and rules, over the entities
rgcn_status rgcn_entity_softmax_reserve(rgcn_ctx* c, int64_t max_positives) {
  RGCN_NEED(c);
  if (max_positives <= 0 || max_positives > RGCN_MAX_DECODER_TRIPLES) RGCN_FAIL(c, RGCN_ERR_INVALID, "max_positives out of range");
  if (c->V < 2) RGCN_FAIL(c, RGCN_ERR_INVALID, "the entity softmax needs at least two entities");
  if (c->V >= (1 << 24) || c->R >= (1 << 24)) RGCN_FAIL(c, RGCN_ERR_UNSUPPORTED, "entity softmax: 2^24 entities or relations, or more");
  if (c->capturing) RGCN_FAIL(c, RGCN_ERR_STATE, "not while a hipGraph is being captured");
  RGCN_TRY(sync_all(c));
  return entity_softmax_reserve(c, max_positives);
}

rgcn_status rgcn_entity_softmax_device(rgcn_ctx* c, const int32_t* pos_dev, int64_t P, float weight, int32_t exclusive) {
  RGCN_NEED(c);
  if (!pos_dev || P <= 0 || P > RGCN_MAX_DECODER_TRIPLES) RGCN_FAIL(c, RGCN_ERR_INVALID, "bad positives");
  if (!relsm_weight_ok(weight)) RGCN_FAIL(c, RGCN_ERR_INVALID, "the weight must be finite and not negative");
  if (c->V < 2) RGCN_FAIL(c, RGCN_ERR_INVALID, "the entity softmax needs at least two entities");
  if (c->world > 1) RGCN_FAIL(c, RGCN_ERR_UNSUPPORTED, "the entity softmax on a relation-sharded context (world > 1)");
  if (c->reciprocal) RGCN_FAIL(c, RGCN_ERR_UNSUPPORTED, "the entity softmax under reciprocal relations (rgcn_set_reciprocal_relations)");
  if (c->capturing) RGCN_FAIL(c, RGCN_ERR_STATE, "not while a hipGraph is being captured");
  if (!c->dec.loss_valid || !c->fwd_done)
    RGCN_FAIL(c, RGCN_ERR_STATE, "the term is added to a decoder pass: call rgcn_decoder_loss_backward_device first");
  if (c->entsm.maxP <= 0) RGCN_FAIL(c, RGCN_ERR_STATE, "call rgcn_entity_softmax_reserve first");
  if (exclusive && c->known.count <= 0) RGCN_FAIL(c, RGCN_ERR_STATE, "call rgcn_known_positives_reserve first");
  if (weight == 0.f) return RGCN_OK;
  RGCN_TRY(stream_join(c, 2));      // W_relation's gradient may still be on its side stream: the term adds to it
  return entity_softmax_compute(c, c->embedding ? c->H[0] : c->codes, pos_dev, nullptr, P, weight, exclusive != 0);
}

rgcn_status rgcn_set_entity_softmax(rgcn_ctx* c, float weight, int64_t num_positives, int32_t exclusive) {
  RGCN_NEED(c);
  if (!relsm_weight_ok(weight)) RGCN_FAIL(c, RGCN_ERR_INVALID, "the weight must be finite and not negative");
  if (num_positives < 0 || num_positives > RGCN_MAX_DECODER_TRIPLES) RGCN_FAIL(c, RGCN_ERR_INVALID, "num_positives out of range");
  if (weight > 0.f) {
    if (c->capturing) RGCN_FAIL(c, RGCN_ERR_STATE, "not while a hipGraph is being captured");
    if (c->V < 2) RGCN_FAIL(c, RGCN_ERR_INVALID, "the entity softmax needs at least two entities");
    if (c->reciprocal)
      RGCN_FAIL(c, RGCN_ERR_UNSUPPORTED, "the entity softmax under reciprocal relations (rgcn_set_reciprocal_relations): its subject "
                                         "rows and its by-relation reduction are not built for the 2 R relation rows");
    if (exclusive && c->known.count <= 0) RGCN_FAIL(c, RGCN_ERR_STATE, "call rgcn_known_positives_reserve first");
  }
  c->entsm.weight = weight;
  c->entsm.step_positives = num_positives;
  c->entsm.exclusive = exclusive != 0;
  return RGCN_OK;
}

rgcn_status rgcn_entity_softmax_plan(int64_t max_positives, int32_t num_entities, int32_t code_dim, int64_t out[5]) {
  if (!out || max_positives <= 0 || num_entities <= 0 || code_dim <= 0) return RGCN_ERR_INVALID;
  const EntsmPlan p = entsm_plan(max_positives, num_entities, code_dim, kEntsmSlabFloats);      // what a context runs
  out[0] = p.chunk; out[1] = p.padded_v; out[2] = p.split_k; out[3] = kEntsmLongRow; out[4] = kEntsmPiece;
  return RGCN_OK;
}

// what a fused step checks before it queues anything while the term is on (rgcn_set_entity_softmax, weight > 0)
static rgcn_status entsm_step_check(rgcn_ctx* c) {
  if (c->world > 1) RGCN_FAIL(c, RGCN_ERR_UNSUPPORTED, "the entity softmax in the step of a relation-sharded context (world > 1)");
  if (c->capturing) RGCN_FAIL(c, RGCN_ERR_STATE, "the entity softmax is not built for a hipGraph capture");
  if (c->entsm.maxP <= 0) RGCN_FAIL(c, RGCN_ERR_STATE, "call rgcn_entity_softmax_reserve first");
  if (c->entsm.exclusive && c->known.count <= 0) RGCN_FAIL(c, RGCN_ERR_STATE, "call rgcn_known_positives_reserve first");
  return RGCN_OK;
}

rgcn_status rgcn_rank_reserve(rgcn_ctx* c, int64_t max_queries) {
  RGCN_NEED(c);
  if (max_queries <= 0) RGCN_FAIL(c, RGCN_ERR_INVALID, "max_queries must be positive");
  RGCN_TRY(sync_all(c));
  return rank_reserve(c, max_queries);
}

// What the query entries below require before any device work, in this order; `checks` names the ones that apply to
// `entry` beside those that apply to all (arguments, no capture, a forward, a reserve).  world > 1: the codes are
// replicated after the last exchange, so the queries need no collective -- each rank passes its own slice of them and the
// caller concatenates.
// QUERY_RELATION: the candidates of the top-k limits are the relations, not the entities.
enum : unsigned { QUERY_WEIGHT = 1, QUERY_TOPK = 2, QUERY_ONE_CHUNK = 4, QUERY_RELATION = 8 };
static rgcn_status query_preconditions(rgcn_ctx* c, const char* entry, unsigned checks, bool args_ok, int64_t n,
                                       float weight = 0.f, int32_t k = 0) {
  const std::string name(entry);
  const int candidates = (checks & QUERY_RELATION) ? c->R : c->V;
  const std::string count_name = (checks & QUERY_RELATION) ? "RelationCount" : "EntityCount";
  if (!args_ok) RGCN_FAIL(c, RGCN_ERR_INVALID, "bad arguments");
  if ((checks & QUERY_WEIGHT) && !(weight >= 0.0f && weight <= 1.0f))
    RGCN_FAIL(c, RGCN_ERR_INVALID, name + ": weight must be in [0, 1]");
  if ((checks & QUERY_TOPK) && (k < 1 || k > candidates || k > RGCN_MAX_TOPK))
    RGCN_FAIL(c, RGCN_ERR_INVALID, name + ": k must be in [1, min(" + count_name + ", " + std::to_string(RGCN_MAX_TOPK) + ")]");
  if ((checks & QUERY_TOPK) && candidates > RGCN_MAX_TOPK_ENTITIES)
    RGCN_FAIL(c, RGCN_ERR_UNSUPPORTED, name + ": " + count_name + " above " + std::to_string(RGCN_MAX_TOPK_ENTITIES) +
                                           " (a row's exclusion mask must fit in LDS)");
  // (W_relation is stored [EntityCount, d] as in the reference: the relation GEMM reads its first RelationCount rows)
  if ((checks & QUERY_RELATION) && c->R > c->V)
    RGCN_FAIL(c, RGCN_ERR_UNSUPPORTED, name + ": RelationCount above EntityCount (W_relation holds EntityCount rows)");
  if (c->capturing) RGCN_FAIL(c, RGCN_ERR_STATE, "this call synchronises with the device: not allowed between rgcn_capture_begin and rgcn_capture_end");
  if (!c->fwd_done) RGCN_FAIL(c, RGCN_ERR_STATE, name + " needs a completed rgcn_forward (test mode on the full graph)");
  if (c->ranking.max <= 0) RGCN_FAIL(c, RGCN_ERR_STATE, "call rgcn_rank_reserve first");
  if ((checks & QUERY_ONE_CHUNK) && n > c->ranking.max)
    RGCN_FAIL(c, RGCN_ERR_INVALID, name + ": one chunk only -- num_queries above what rgcn_rank_reserve sized (the score "
                                          "buffers, this context's and a partner's, hold one chunk)");
  return RGCN_OK;
}

rgcn_status rgcn_rank_device(rgcn_ctx* c, const int32_t* x_dev, int64_t n, int32_t predict_object,
                             const int64_t* filter_ptr_dev, const int32_t* filter_idx_dev, int32_t* raw_rank_dev,
                             int32_t* filtered_rank_dev) {
  RGCN_NEED(c);
  RGCN_TRY(query_preconditions(c, "rgcn_rank_device", 0,
                               n >= 0 && (n == 0 || (x_dev && filter_ptr_dev && raw_rank_dev && filtered_rank_dev)), n));
  if (n == 0) return RGCN_OK;
  return rank_compute(c, x_dev, n, predict_object ? 1 : 0, filter_ptr_dev, filter_idx_dev, raw_rank_dev, filtered_rank_dev);
}

rgcn_status rgcn_rank_typed_device(rgcn_ctx* c, const int32_t* x_dev, int64_t n, int32_t predict_object,
                                   const int64_t* filter_ptr_dev, const int32_t* filter_idx_dev, int32_t* raw_rank_dev,
                                   int32_t* filtered_rank_dev) {
  RGCN_NEED(c);
  RGCN_TRY(query_preconditions(c, "rgcn_rank_typed_device", 0,
                               n >= 0 && (n == 0 || (x_dev && filter_ptr_dev && raw_rank_dev && filtered_rank_dev)), n));
  if (!c->types.ready) RGCN_FAIL(c, RGCN_ERR_STATE, "call rgcn_type_sets_reserve first");
  if (n == 0) return RGCN_OK;
  return rank_typed_compute(c, x_dev, n, predict_object ? 1 : 0, filter_ptr_dev, filter_idx_dev, raw_rank_dev,
                            filtered_rank_dev);
}

rgcn_status rgcn_topk_typed_device(rgcn_ctx* c, const int32_t* x_dev, int64_t n, int32_t predict_object, int32_t k,
                                   const int64_t* exclude_ptr_dev, const int32_t* exclude_idx_dev, int32_t* topk_idx_dev,
                                   float* topk_energy_dev) {
  RGCN_NEED(c);
  RGCN_TRY(query_preconditions(c, "rgcn_topk_typed_device", QUERY_TOPK,
                               n >= 0 && (n == 0 || (x_dev && topk_idx_dev && topk_energy_dev)) &&
                                   !exclude_ptr_dev == !exclude_idx_dev,
                               n, 0.f, k));
  if (!c->types.ready) RGCN_FAIL(c, RGCN_ERR_STATE, "call rgcn_type_sets_reserve first");
  if (n == 0) return RGCN_OK;
  return topk_typed_compute(c, x_dev, n, predict_object ? 1 : 0, k, exclude_ptr_dev, exclude_idx_dev, topk_idx_dev,
                            topk_energy_dev);
}

const float* rgcn_rank_energies_device(rgcn_ctx* c) { return c ? c->ranking.s : nullptr; }

rgcn_status rgcn_rank_mixed_device(rgcn_ctx* c, const int32_t* x_dev, int64_t n, int32_t predict_object,
                                   const float* partner_energies_dev, float weight, const int64_t* filter_ptr_dev,
                                   const int32_t* filter_idx_dev, int32_t* raw_rank_dev, int32_t* filtered_rank_dev) {
  RGCN_NEED(c);
  RGCN_TRY(query_preconditions(c, "rgcn_rank_mixed_device", QUERY_WEIGHT | QUERY_ONE_CHUNK,
                               n >= 0 && (n == 0 || (x_dev && partner_energies_dev && filter_ptr_dev && raw_rank_dev &&
                                                     filtered_rank_dev)),
                               n, weight));
  if (n == 0) return RGCN_OK;
  return rank_mixed_compute(c, x_dev, n, predict_object ? 1 : 0, partner_energies_dev, weight, filter_ptr_dev, filter_idx_dev,
                            raw_rank_dev, filtered_rank_dev);
}

rgcn_status rgcn_topk_device(rgcn_ctx* c, const int32_t* x_dev, int64_t n, int32_t predict_object, int32_t k,
                             const int64_t* exclude_ptr_dev, const int32_t* exclude_idx_dev, int32_t* topk_idx_dev,
                             float* topk_energy_dev) {
  RGCN_NEED(c);
  RGCN_TRY(query_preconditions(c, "rgcn_topk_device", QUERY_TOPK,
                               n >= 0 && (n == 0 || (x_dev && topk_idx_dev && topk_energy_dev)) &&
                                   !exclude_ptr_dev == !exclude_idx_dev,
                               n, 0.f, k));
  if (n == 0) return RGCN_OK;
  return topk_compute(c, x_dev, n, predict_object ? 1 : 0, k, exclude_ptr_dev, exclude_idx_dev, topk_idx_dev, topk_energy_dev);
}

rgcn_status rgcn_score_queries_device(rgcn_ctx* c, const int32_t* x_dev, int64_t n, int32_t predict_object) {
  RGCN_NEED(c);
  RGCN_TRY(query_preconditions(c, "rgcn_score_queries_device", QUERY_ONE_CHUNK, n >= 0 && (n == 0 || x_dev), n));
  if (n == 0) return RGCN_OK;
  return score_queries_compute(c, x_dev, n, predict_object ? 1 : 0);
}

rgcn_status rgcn_topk_mixed_device(rgcn_ctx* c, const int32_t* x_dev, int64_t n, int32_t predict_object, int32_t k,
                                   const float* partner_energies_dev, float weight, const int64_t* exclude_ptr_dev,
                                   const int32_t* exclude_idx_dev, int32_t* topk_idx_dev, float* topk_score_dev) {
  RGCN_NEED(c);
  RGCN_TRY(query_preconditions(c, "rgcn_topk_mixed_device", QUERY_WEIGHT | QUERY_TOPK | QUERY_ONE_CHUNK,
                               n >= 0 && (n == 0 || (x_dev && partner_energies_dev && topk_idx_dev && topk_score_dev)) &&
                                   !exclude_ptr_dev == !exclude_idx_dev,
                               n, weight, k));
  if (n == 0) return RGCN_OK;
  return topk_mixed_compute(c, x_dev, n, predict_object ? 1 : 0, k, partner_energies_dev, weight, exclude_ptr_dev,
                            exclude_idx_dev, topk_idx_dev, topk_score_dev);
}

rgcn_status rgcn_score_relation_queries_device(rgcn_ctx* c, const int32_t* x_dev, int64_t n) {
  RGCN_NEED(c);
  RGCN_TRY(query_preconditions(c, "rgcn_score_relation_queries_device", QUERY_RELATION | QUERY_ONE_CHUNK,
                               n >= 0 && (n == 0 || x_dev), n));
  if (n == 0) return RGCN_OK;
  return score_relation_queries_compute(c, x_dev, n);
}

const float* rgcn_relation_energies_device(rgcn_ctx* c) { return c ? c->ranking.rel : nullptr; }

rgcn_status rgcn_rank_relation_device(rgcn_ctx* c, const int32_t* x_dev, int64_t n, const int64_t* filter_ptr_dev,
                                      const int32_t* filter_idx_dev, int32_t* raw_rank_dev, int32_t* filtered_rank_dev) {
  RGCN_NEED(c);
  RGCN_TRY(query_preconditions(c, "rgcn_rank_relation_device", QUERY_RELATION,
                               n >= 0 && (n == 0 || (x_dev && filter_ptr_dev && raw_rank_dev && filtered_rank_dev)), n));
  if (n == 0) return RGCN_OK;
  return rank_relation_compute(c, x_dev, n, filter_ptr_dev, filter_idx_dev, raw_rank_dev, filtered_rank_dev);
}

rgcn_status rgcn_topk_relation_device(rgcn_ctx* c, const int32_t* x_dev, int64_t n, int32_t k,
                                      const int64_t* exclude_ptr_dev, const int32_t* exclude_idx_dev, int32_t* topk_idx_dev,
                                      float* topk_energy_dev) {
  RGCN_NEED(c);
  RGCN_TRY(query_preconditions(c, "rgcn_topk_relation_device", QUERY_RELATION | QUERY_TOPK,
                               n >= 0 && (n == 0 || (x_dev && topk_idx_dev && topk_energy_dev)) &&
                                   !exclude_ptr_dev == !exclude_idx_dev,
                               n, 0.f, k));
  if (n == 0) return RGCN_OK;
  return topk_relation_compute(c, x_dev, n, k, exclude_ptr_dev, exclude_idx_dev, topk_idx_dev, topk_energy_dev);
}

rgcn_status rgcn_optimizer_config_ex(rgcn_ctx* c, const rgcn_optimizer_params* p) {
  RGCN_NEED(c);
  const OptimizerVerdict verdict = check_optimizer_params(p);
  if (verdict.status != RGCN_OK) RGCN_FAIL(c, verdict.status, verdict.message);
  OptimizerState& o = c->opt;
  if (p->algorithm != o.algorithm) {
    // the state of one algorithm means nothing to another: released, and the count starts over
    if (c->capturing) RGCN_FAIL(c, RGCN_ERR_STATE, "the optimizer's algorithm cannot change while a hipGraph is being captured");
    RGCN_HIP(c, hipStreamSynchronize(c->stream));
    optimizer_release_state(c);
    o.algorithm = p->algorithm;
  }
  o.lr = p->learning_rate;
  o.max_norm = p->max_grad_norm;
  if (p->algorithm == RGCN_OPT_ADAM) { o.beta1 = p->beta1; o.beta2 = p->beta2; o.eps = p->epsilon; }
  if (p->algorithm == RGCN_OPT_ADAGRAD) o.init_acc = p->initial_accumulator;
  o.configured = true;
  return RGCN_OK;
}

rgcn_status rgcn_optimizer_config(rgcn_ctx* c, float lr, float beta1, float beta2, float eps, float max_grad_norm) {
  const rgcn_optimizer_params p = {(int32_t)sizeof(rgcn_optimizer_params), RGCN_OPT_ADAM, lr, beta1, beta2, eps,
                                   max_grad_norm, 0.1f};
  return rgcn_optimizer_config_ex(c, &p);
}

int32_t rgcn_optimizer_slot_count(const rgcn_ctx* c) { return c ? optimizer_slot_count(c) : 0; }

// what every call on the optimizer's state refuses; param < 0: a call on the step count, which has no parameter
static rgcn_status optimizer_state_check(rgcn_ctx* c, int32_t param, int32_t slot, const void* host, int64_t count) {
  if (!c->opt.configured) RGCN_FAIL(c, RGCN_ERR_STATE, "rgcn_optimizer_config was not called");
  if (c->world > 1)
    RGCN_FAIL(c, RGCN_ERR_UNSUPPORTED, "optimizer state on a sharded context (a relation's state is current on its owner only)");
  if (c->capturing) RGCN_FAIL(c, RGCN_ERR_STATE, "this call synchronises with the device: not allowed between rgcn_capture_begin and rgcn_capture_end");
  if (param < 0) return RGCN_OK;
  RGCN_TRY(param_check(c, param, host, count));
  if (c->params[param].no_grad)
    RGCN_FAIL(c, RGCN_ERR_INVALID, "parameter " + c->params[param].name + " has no gradient and no optimizer state");
  if (slot < 0 || slot >= optimizer_slot_count(c)) RGCN_FAIL(c, RGCN_ERR_INVALID, "optimizer slot out of range");
  return RGCN_OK;
}

// A slot in its parameter's clothes: the same layout and, but for W_relation, the same element count -- W_relation's slot
// holds the first RelationCount rows, which are the head of its (plain) host layout.
static Param slot_as_param(const rgcn_ctx* c, int32_t param, int64_t n) {
  Param q = c->params[param];
  q.count = n;
  return q;
}

rgcn_status rgcn_get_optimizer_slot(rgcn_ctx* c, int32_t param, int32_t slot, float* host, int64_t count) {
  RGCN_NEED(c);
  RGCN_TRY(optimizer_state_check(c, param, slot, host, count));
  RGCN_TRY(check_dev_flag(c));
  float* dev = nullptr;
  int64_t n = 0;
  RGCN_TRY(optimizer_slot(c, param, slot, &dev, &n));
  RGCN_TRY(param_download(c, slot_as_param(c, param, n), dev, host));
  const float initial = optimizer_slot_initial(c);
  for (int64_t i = n; i < count; ++i) host[i] = initial;      // (W_relation's rows without state)
  return RGCN_OK;
}

rgcn_status rgcn_set_optimizer_slot(rgcn_ctx* c, int32_t param, int32_t slot, const float* host, int64_t count) {
  RGCN_NEED(c);
  RGCN_TRY(optimizer_state_check(c, param, slot, host, count));
  float* dev = nullptr;
  int64_t n = 0;
  RGCN_TRY(optimizer_slot(c, param, slot, &dev, &n));
  const uint64_t version = c->weights_version;
  RGCN_TRY(param_upload(c, slot_as_param(c, param, n), dev, host));
  c->weights_version = version;      // (no weight changed: the tables derived from the weights are still right)
  return RGCN_OK;
}

rgcn_status rgcn_get_optimizer_step(rgcn_ctx* c, int64_t* t) {
  RGCN_NEED(c);
  if (!t) RGCN_FAIL(c, RGCN_ERR_INVALID, "NULL pointer");
  RGCN_TRY(optimizer_state_check(c, -1, 0, nullptr, 0));
  RGCN_TRY(check_dev_flag(c));
  float* state = nullptr;
  RGCN_TRY(optimizer_state_array(c, &state));
  float count = 0.f;
  RGCN_TRY(to_host(c, &count, state + 2, sizeof(float)));
  *t = (int64_t)count;
  c->opt.t = *t;
  return RGCN_OK;
}

rgcn_status rgcn_set_optimizer_step(rgcn_ctx* c, int64_t t) {
  RGCN_NEED(c);
  RGCN_TRY(optimizer_state_check(c, -1, 0, nullptr, 0));
  // the device keeps the count as a float (state[2], beside the clip scale and the rate): exact below 2^24
  if (t < 0 || t >= ((int64_t)1 << 24)) RGCN_FAIL(c, RGCN_ERR_INVALID, "optimizer step count outside [0, 2^24)");
  float* state = nullptr;
  RGCN_TRY(optimizer_state_array(c, &state));
  const float count = (float)t;
  RGCN_TRY(to_dev(c, state + 2, &count, sizeof(float)));
  c->opt.t = t;
  return RGCN_OK;
}

rgcn_status rgcn_optimizer_step(rgcn_ctx* c) {
  RGCN_NEED(c);
  if (c->world > 1 && !c->comm)
    RGCN_FAIL(c, RGCN_ERR_STATE, "world > 1: call rgcn_comm_init first (or drive rgcn_optimizer_norm_partial / _apply yourself)");
  RGCN_TRY(join_abandoned_side_work(c));      // (the gradients of a step that ended unjoined)
  return optimizer_step(c);
}
rgcn_status rgcn_optimizer_norm_partial(rgcn_ctx* c) {
  RGCN_NEED(c);
  RGCN_TRY(join_abandoned_side_work(c));
  return optimizer_norm_partial(c);
}
rgcn_status rgcn_optimizer_apply(rgcn_ctx* c) { RGCN_NEED(c); return optimizer_apply(c); }

// everything of a train step behind the graph preparation: encoder forward, decoder loss + gradients, encoder
// backward, clip + Adam
// n_pos > 0: the leading n_pos rows of X are the positives of the relation-softmax term (one GPU; relsm_step_check)
// n_ent > 0: the leading n_ent rows of X are the positives of the entity-softmax term (one GPU; entsm_step_check)
static rgcn_status train_step_tail(rgcn_ctx* c, const int32_t* X_dev, const float* Y_dev, int64_t N, uint64_t seed,
                                   float reg_param, int64_t n_pos = 0, int64_t adv_pos = 0, int64_t n_ent = 0,
                                   int64_t recip_tail = 0) {
  RGCN_TRY(forward_all(c, 1, seed, nullptr));
  // adv_pos > 0: self-adversarial weights of the negatives (one GPU; adv_step_check), from the codes the forward pass just
  // left.  On the main stream: the pass reads X alone, so it runs beside the decoder's preparation on side stream 1.
  const float* row_w = nullptr;
  if (adv_pos > 0) {
    // recip_tail > 0 (reciprocal relations): the inverse positives behind the groups take weight 1
    RGCN_TRY(adversarial_weights(c, c->codes, X_dev, Y_dev, N - recip_tail, adv_pos, c->adv.temperature, c->adv.w));
    RGCN_TRY(optimizer_fill(c, c->adv.w + (N - recip_tail), recip_tail, 1.0f));
    c->adv.last_N = N;
    row_w = c->adv.w;
  }
  // Relation-sharded run: the decoder is divided by TRIPLES -- rank g takes the slice [g ceil(N / world), ...) of the
  // batch (the codes are replicated after the last forward exchange), its loss terms and gradients are normalised by
  // the whole batch's N, and the partial dL/dcodes [V,d], dL/dW_relation [R,d] and loss are summed over the ranks
  // (decoder_allreduce) before the backward pass starts.
  const int64_t per = (N + c->world - 1) / c->world;
  const int64_t lo = c->world > 1 ? std::min<int64_t>(N, (int64_t)c->rank * per) : 0;
  const int64_t n_loc = c->world > 1 ? std::min<int64_t>(N, lo + per) - lo : N;
  const int32_t* X_loc = X_dev + 3 * lo;
  const float* Y_loc = Y_dev + lo;
  // The decoder batch's CSRs depend on X only.  They are built on side stream 1, forked at the START of the step,
  // but enqueued AFTER the encoder's prep and forward: their two sorts are ~45 launches of a few microseconds, and
  // queued first they kept the host from feeding the main stream for the first 0.3 ms of every step.
  // A captured step is a single chain (rgcn_capture_begin) with ONE exception, this fork: the preparation is ~0.15 ms
  // of small launches that nothing in the encoder's forward pass depends on, worth far more than the two cross-stream
  // edges it puts into the graph.
  const bool fork_in_capture = c->capturing && c->use_aux_before_capture && c->step_begin_in_capture && c->world == 1;
  if (c->use_aux || fork_in_capture) {
    RGCN_HIP(c, hipStreamWaitEvent(c->aux[1], c->ev_step_begin, 0));
    c->stream = c->aux[1];
    c->aux_dirty[1] = true;
    rgcn_status ps = decoder_prepare(c, X_loc, n_loc, N);
    // (the relation-softmax term's CSR depends on X only too: beside the decoder's)
    if (ps == RGCN_OK && n_pos > 0) ps = relation_softmax_prepare(c, X_dev, n_pos);
    c->stream = c->main_stream;
    RGCN_TRY(ps);
  } else {
    RGCN_TRY(decoder_prepare(c, X_loc, n_loc, N));
    if (n_pos > 0) RGCN_TRY(relation_softmax_prepare(c, X_dev, n_pos));
  }
  RGCN_TRY(stream_join(c, 1));
  // one GPU: the decoder's entity-gradient kernel also writes dL/dcodes * dropout_L, the operand of the top layer's
  // self-loop GEMMs (a sharded run scales after the all-reduce of the partial dL/dcodes, in bwd_begin)
  const DropSpec top_drop = make_drop(c, c->L, true);
  // (a highway context forms dS_L itself, from G_L T_L: bwd_layer_partial; under an output transform the top layer's D is
  // dcodes . W_out^T, which bwd_begin forms and scales: a dropout copy of the [V,dc] dcodes is of no use)
  // (with the relation-softmax term on, dL/dcodes is complete only behind the term: bwd_begin scales it)
  // (and likewise with the entity-softmax term on)
  float* ds_ready = (c->world == 1 && !c->highway && !c->out_layer && top_drop.mode != DROP_NONE && n_pos <= 0 && n_ent <= 0)
                        ? c->dsbuf[c->L & 1] : nullptr;
  RGCN_TRY(decoder_compute(c, c->codes, Y_loc, reg_param, ds_ready, &top_drop, row_w));
  if (n_pos > 0) {
    // the term adds to what the decoder left, W_relation's gradient on side stream 2 included: join it first
    RGCN_TRY(stream_join(c, 2));
    RGCN_TRY(relation_softmax_compute(c, c->codes, X_dev, Y_dev, n_pos, c->relsm.weight, c->relsm.exclusive));
  }
  if (n_ent > 0) {
    // on the main stream behind the decoder and the relation term; it adds to W_relation's gradient, whose last writers
    // (the decoder's reduce, the relation term's last chunk) are on side stream 2: join it first
    RGCN_TRY(stream_join(c, 2));
    RGCN_TRY(entity_softmax_compute(c, c->codes, X_dev, Y_dev, n_ent, c->entsm.weight, c->entsm.exclusive));
  }
  if (c->world > 1) {
    RGCN_TRY(stream_join(c, 2));    // the relation gradient's reduce ran on its own side stream: it is all-reduced too
    RGCN_TRY(decoder_allreduce(c));
  }
  c->dec.loss_valid = true;
  RGCN_TRY(backward_all(c, c->dcodes_own, ds_ready));
  RGCN_TRY(stream_join(c, 2));      // dL/dW_relation, computed beside the backward pass
  RGCN_TRY(step_end(c));
  if (c->opt.configured) RGCN_TRY(optimizer_step(c));
  return RGCN_OK;
}

static rgcn_status prefetch_impl(rgcn_ctx* c, const int32_t* tri_dev, int64_t E, int64_t keep, uint64_t eseed) {
  if (E < 0 || E > c->cfg.max_edges) RGCN_FAIL(c, RGCN_ERR_INVALID, "num_edges outside [0, max_edges]");
  if (keep > E) RGCN_FAIL(c, RGCN_ERR_INVALID, "edge dropout: keep outside [0, num_edges]");
  if (keep >= 0 && E >= ((int64_t)1 << 24)) RGCN_FAIL(c, RGCN_ERR_UNSUPPORTED, "edge dropout: more than 2^24 batch edges");
  if (E > 0 && !tri_dev) RGCN_FAIL(c, RGCN_ERR_INVALID, "NULL triples");
  // build into the INACTIVE set on the prefetch stream; it only has to wait for the last step that
  // used that set (not for the step currently queued on the main stream)
  std::swap(c->g, c->g_alt);
  rgcn_status s = RGCN_OK;
  do {
    if (c->capturing) {
      // join the capture at the start of the step queued last (so that the preparation overlaps it), and
      // behind the last captured step that used this buffer set
      if (!c->step_begin_in_capture) { s = RGCN_ERR_STATE; c->err = "capture: queue a step before its prefetch"; break; }
      if (hipStreamWaitEvent(c->pf_stream, c->ev_step_begin, 0) != hipSuccess) { s = RGCN_ERR_HIP; c->err = "hipStreamWaitEvent"; break; }
      if (c->g.free_in_capture && hipStreamWaitEvent(c->pf_stream, c->g.ev_free, 0) != hipSuccess) { s = RGCN_ERR_HIP; c->err = "hipStreamWaitEvent"; break; }
      c->cap_pf_forked = true;
    } else if (hipStreamWaitEvent(c->pf_stream, c->g.ev_free, 0) != hipSuccess) { s = RGCN_ERR_HIP; c->err = "hipStreamWaitEvent"; break; }
    c->stream = c->pf_stream;
    const bool was_done = c->fwd_done;
    s = keep < 0 ? graph_build(c, tri_dev, E) : graph_build_dropout(c, tri_dev, E, keep, eseed, nullptr);
    c->fwd_done = was_done;          // the ACTIVE set's forward state is untouched
    c->stream = c->main_stream;
    if (s != RGCN_OK) break;
    if (hipEventRecord(c->g.ev_ready, c->pf_stream) != hipSuccess) { s = RGCN_ERR_HIP; c->err = "hipEventRecord"; break; }
    c->g.ready_in_capture = c->capturing;
    c->g.pf_tri = tri_dev;
    c->g.pf_E = E;
    c->g.pf_keep = keep;
    c->g.pf_eseed = eseed;
    c->g.pf_valid = true;
  } while (0);
  c->stream = c->main_stream;
  std::swap(c->g, c->g_alt);
  return s;
}

rgcn_status rgcn_train_step_device(rgcn_ctx* c, const int32_t* tri_dev, int64_t E, const int32_t* X_dev,
                                   const float* Y_dev, int64_t N, uint64_t seed, float reg_param) {
  RGCN_NEED(c);
  if (c->embedding && (tri_dev || E != 0))
    RGCN_FAIL(c, RGCN_ERR_INVALID, "an RGCN_KIND_EMBEDDING context takes no graph: pass NULL triples and num_edges 0");
  if (E < 0 || E > c->cfg.max_edges) RGCN_FAIL(c, RGCN_ERR_INVALID, "num_edges outside [0, max_edges]");
  if (!X_dev || !Y_dev || N <= 0) RGCN_FAIL(c, RGCN_ERR_INVALID, "bad decoder batch");
  // (the term's refusals first: a sharded context is refused whether or not it has its communicator yet)
  if (c->relsm.weight > 0.f) RGCN_TRY(relsm_step_check(c));
  if (c->adv.temperature > 0.f) RGCN_TRY(adv_step_check(c, N, c->adv.step_positives));
  if (c->entsm.weight > 0.f) RGCN_TRY(entsm_step_check(c));
  if (c->world > 1 && !c->comm)
    RGCN_FAIL(c, RGCN_ERR_STATE, "world > 1: call rgcn_comm_init first (or drive the phase API yourself)");
  if (c->dec.maxN < N) RGCN_FAIL(c, RGCN_ERR_STATE, "call rgcn_decoder_reserve(ctx, max_triples) first");
  int64_t n_pos = 0;
  if (c->relsm.weight > 0.f) {
    if (c->relsm.step_positives <= 0)
      RGCN_FAIL(c, RGCN_ERR_STATE, "rgcn_set_relation_softmax was given num_positives = 0: the minibatch step only");
    if (c->relsm.step_positives > N) RGCN_FAIL(c, RGCN_ERR_INVALID, "rgcn_set_relation_softmax: num_positives above the batch's rows");
    n_pos = c->relsm.step_positives;
  }
  int64_t n_ent = 0;
  if (c->entsm.weight > 0.f) {
    if (c->entsm.step_positives <= 0)
      RGCN_FAIL(c, RGCN_ERR_STATE, "rgcn_set_entity_softmax was given num_positives = 0: the minibatch step only");
    if (c->entsm.step_positives > N) RGCN_FAIL(c, RGCN_ERR_INVALID, "rgcn_set_entity_softmax: num_positives above the batch's rows");
    n_ent = c->entsm.step_positives;
  }
  const int64_t adv_pos = c->adv.temperature > 0.f ? c->adv.step_positives : 0;
  if (c->adv.temperature > 0.f) RGCN_TRY(adv_step_buffer(c));
  // reciprocal relations: the batch ends in its inverse positives, one per positive, which stand outside the groups
  const int64_t recip_tail = c->reciprocal && adv_pos > 0 ? adv_pos : 0;
  if (recip_tail > 0 && N < 2 * recip_tail)
    RGCN_FAIL(c, RGCN_ERR_INVALID, "adversarial negatives under reciprocal relations: the batch has no inverse positives behind its groups");
  if (c->embedding) {
    // the DistMult baseline's step: decoder loss + gradients on the table itself (dL/dcodes is written into W_emb's
    // gradient), then clip + Adam.  One chain on the main stream but for the relation gradient's side stream.
    RGCN_TRY(forward_all(c, 1, seed, nullptr));
    const float* row_w = nullptr;
    if (adv_pos > 0) {
      RGCN_TRY(adversarial_weights(c, c->H[0], X_dev, Y_dev, N - recip_tail, adv_pos, c->adv.temperature, c->adv.w));
      RGCN_TRY(optimizer_fill(c, c->adv.w + (N - recip_tail), recip_tail, 1.0f));
      c->adv.last_N = N;
      row_w = c->adv.w;
    }
    RGCN_TRY(decoder_prepare(c, X_dev, N));
    RGCN_TRY(decoder_compute(c, c->H[0], Y_dev, reg_param, nullptr, nullptr, row_w));
    RGCN_TRY(stream_join(c, 2));
    if (n_pos > 0) {
      c->relsm.csr_X = nullptr;
      RGCN_TRY(relation_softmax_compute(c, c->H[0], X_dev, Y_dev, n_pos, c->relsm.weight, c->relsm.exclusive));
    }
    RGCN_TRY(stream_join(c, 2));
    if (n_ent > 0) RGCN_TRY(entity_softmax_compute(c, c->H[0], X_dev, Y_dev, n_ent, c->entsm.weight, c->entsm.exclusive));
    c->dec.loss_valid = true;
    if (c->opt.configured) RGCN_TRY(optimizer_step(c));
    return RGCN_OK;
  }
  RGCN_TRY(step_begin(c, tri_dev, E, true));
  return train_step_tail(c, X_dev, Y_dev, N, seed, reg_param, n_pos, adv_pos, n_ent, recip_tail);
}

rgcn_status rgcn_prefetch_graph_device(rgcn_ctx* c, const int32_t* tri_dev, int64_t E) {
  RGCN_NEED(c);
  RGCN_NO_EMBEDDING(c, "rgcn_prefetch_graph_device");
  return prefetch_impl(c, tri_dev, E, -1, 0);
}
rgcn_status rgcn_prefetch_graph_dropout_device(rgcn_ctx* c, const int32_t* batch_dev, int64_t n, int64_t keep,
                                               uint64_t seed) {
  RGCN_NEED(c);
  RGCN_NO_EMBEDDING(c, "rgcn_prefetch_graph_dropout_device");
  if (keep < 0) RGCN_FAIL(c, RGCN_ERR_INVALID, "edge dropout: keep outside [0, num_edges]");
  return prefetch_impl(c, batch_dev, n, keep, seed);
}

rgcn_status rgcn_set_graph_dropout_device(rgcn_ctx* c, const int32_t* batch_dev, int64_t n, int64_t keep, uint64_t seed,
                                          const uint8_t* keep_mask_dev) {
  RGCN_NEED(c);
  RGCN_NO_EMBEDDING(c, "rgcn_set_graph_dropout_device");
  if (n < 0 || n > c->cfg.max_edges) RGCN_FAIL(c, RGCN_ERR_INVALID, "num_edges outside [0, max_edges]");
  if (keep < 0 || keep > n) RGCN_FAIL(c, RGCN_ERR_INVALID, "edge dropout: keep outside [0, num_edges]");
  if (n >= ((int64_t)1 << 24)) RGCN_FAIL(c, RGCN_ERR_UNSUPPORTED, "edge dropout: more than 2^24 batch edges");
  if (n > 0 && !batch_dev) RGCN_FAIL(c, RGCN_ERR_INVALID, "NULL triples");
  RGCN_TRY(join_abandoned_side_work(c));
  return graph_build_dropout(c, batch_dev, n, keep, seed, keep_mask_dev);
}

rgcn_status rgcn_get_graph_edges(rgcn_ctx* c, int32_t* host, int64_t count) {
  RGCN_NEED(c);
  if (!c->g.ready) RGCN_FAIL(c, RGCN_ERR_STATE, "no graph has been set");      // (always, on an RGCN_KIND_EMBEDDING context)
  if (count != c->g.E || (count > 0 && !host)) RGCN_FAIL(c, RGCN_ERR_INVALID, "need an [E,3] host buffer of the current graph's size");
  if (count == 0) return RGCN_OK;
  RGCN_TRY(check_dev_flag(c));
  return to_host(c, host, c->g.cur, sizeof(int32_t) * 3 * (size_t)count);
}

rgcn_status rgcn_train_step_minibatch_device(rgcn_ctx* c, const int32_t* batch_dev, int64_t n, int64_t keep,
                                             uint64_t edge_seed, int32_t negative_rate, uint64_t negative_seed,
                                             int32_t* x_scratch_dev, float* y_scratch_dev, uint64_t dropout_seed,
                                             float reg_param) {
  RGCN_NEED(c);
  RGCN_NO_EMBEDDING(c, "rgcn_train_step_minibatch_device");
  if (n <= 0 || n > c->cfg.max_edges) RGCN_FAIL(c, RGCN_ERR_INVALID, "num_edges outside [1, max_edges]");
  if (keep < 0 || keep > n) RGCN_FAIL(c, RGCN_ERR_INVALID, "edge dropout: keep outside [0, num_edges]");
  if (n >= ((int64_t)1 << 24)) RGCN_FAIL(c, RGCN_ERR_UNSUPPORTED, "edge dropout: more than 2^24 batch edges");
  if (negative_rate < 0 || negative_rate > 1024 || !batch_dev || !x_scratch_dev || !y_scratch_dev)
    RGCN_FAIL(c, RGCN_ERR_INVALID, "bad arguments");
  const int32_t relation_rate = c->relation_negatives;      // rgcn_set_relation_negatives; 0: the step as it always was
  const bool reciprocal = c->reciprocal;            // rgcn_set_reciprocal_relations; off: the step as it always was
  const int64_t N = n * (int64_t)(negative_rate + 1 + relation_rate) + (reciprocal ? n : 0);
  const bool relsm_on = c->relsm.weight > 0.f;      // rgcn_set_relation_softmax; off: the step as it always was
  if (relsm_on) RGCN_TRY(relsm_step_check(c));      // (ahead of the communicator's check, as in rgcn_train_step_device)
  const bool adv_on = c->adv.temperature > 0.f;     // rgcn_set_adversarial_negatives; off: the step as it always was
  if (adv_on) RGCN_TRY(adv_step_check(c, N, n));
  const bool entsm_on = c->entsm.weight > 0.f;      // rgcn_set_entity_softmax; off: the step as it always was
  if (entsm_on) RGCN_TRY(entsm_step_check(c));
  if (c->world > 1 && !c->comm)
    RGCN_FAIL(c, RGCN_ERR_STATE, "world > 1: call rgcn_comm_init first (or drive the phase API yourself)");
  if (c->dec.maxN < N) RGCN_FAIL(c, RGCN_ERR_STATE, "call rgcn_decoder_reserve(ctx, max_triples) first");
  if (adv_on) RGCN_TRY(adv_step_buffer(c));
  const bool typed = c->types.typed;                 // rgcn_set_typed_negatives; off: the step as it always was
  if (typed && c->capturing) RGCN_FAIL(c, RGCN_ERR_STATE, "type-constrained negatives are not built for a hipGraph capture");
  if (reciprocal && c->capturing) RGCN_FAIL(c, RGCN_ERR_UNSUPPORTED, "reciprocal relations are not built for a hipGraph capture");
  if (relation_rate > 0 || reciprocal) {
    if (relation_rate > 0 && c->capturing) RGCN_FAIL(c, RGCN_ERR_STATE, "relation corruptions are not built for a hipGraph capture");
    if (N > RGCN_MAX_DECODER_TRIPLES) RGCN_FAIL(c, RGCN_ERR_INVALID, "batch too large");
    // the relation rows lie behind the n (rate + 1) rows a caller sized its scratch for before the mode existed
    if (!allocation_covers(x_scratch_dev, sizeof(int32_t) * 3 * (size_t)N) ||
        !allocation_covers(y_scratch_dev, sizeof(float) * (size_t)N))
      RGCN_FAIL(c, RGCN_ERR_STATE, reciprocal ? "the scratch buffers must hold num_edges x (2 + negative_rate + relation_rate) rows"
                                              : "the scratch buffers must hold num_edges x (1 + negative_rate + relation_rate) rows");
  }
  // the message graph: adopted from the prefetch of this very (batch, keep, seed), or drawn and prepared in line
  RGCN_TRY(step_begin(c, batch_dev, n, false, keep, edge_seed));   // (the fork point is recorded below)
  // the decoder batch: all n batch edges as positives (the dropped ones included) + their corruptions
  if (typed)
    RGCN_TRY(negative_sample_typed(c, batch_dev, n, negative_rate, relation_rate, c->known.exclusive, negative_seed,
                                   x_scratch_dev, y_scratch_dev));
  else if (relation_rate > 0)
    RGCN_TRY(negative_sample_relation(c, batch_dev, n, negative_rate, relation_rate, c->known.exclusive, negative_seed,
                                      x_scratch_dev, y_scratch_dev));
  else if (c->known.exclusive)
    RGCN_TRY(negative_sample_exclusive(c, batch_dev, n, negative_rate, negative_seed, x_scratch_dev, y_scratch_dev));
  else
    RGCN_TRY(negative_sample(c, batch_dev, n, negative_rate, negative_seed, x_scratch_dev, y_scratch_dev));
  if (reciprocal)
    RGCN_TRY(reciprocal_rows(c, batch_dev, n, negative_rate, relation_rate, negative_seed, x_scratch_dev, y_scratch_dev));
  // the decoder's batch preparation forks from ev_step_begin onto a side stream: it must see the sampled batch
  RGCN_HIP(c, hipEventRecord(c->ev_step_begin, c->main_stream));
  return train_step_tail(c, x_scratch_dev, y_scratch_dev, N, dropout_seed, reg_param, relsm_on ? n : 0, adv_on ? n : 0,
                         // (the batch rows, or the leading num_positives of them where rgcn_set_entity_softmax named a count)
                         entsm_on ? (c->entsm.step_positives > 0 ? std::min<int64_t>(c->entsm.step_positives, n) : n) : 0,
                         reciprocal && adv_on ? n : 0);
}

// ---- neighbourhood edge sampler on the device ------------------------------------------
rgcn_status rgcn_neighborhood_reserve(rgcn_ctx* c, const int32_t* triples_host, int64_t n) {
  RGCN_NEED(c);
  RGCN_NO_EMBEDDING(c, "rgcn_neighborhood_reserve");
  if (n <= 0 || n >= ((int64_t)1 << 31) / 3 || !triples_host) RGCN_FAIL(c, RGCN_ERR_INVALID, "need the training triples");
  if (c->capturing) RGCN_FAIL(c, RGCN_ERR_STATE, "not while a hipGraph is being captured");
  for (int64_t e = 0; e < n; ++e) {
    const int32_t s = triples_host[3 * e], r = triples_host[3 * e + 1], o = triples_host[3 * e + 2];
    if (s < 0 || s >= c->V || o < 0 || o >= c->V || r < 0 || r >= c->R)
      RGCN_FAIL(c, RGCN_ERR_INVALID, "training triple " + std::to_string(e) + " has an id out of range");
  }
  RGCN_TRY(sync_all(c));
  return neighborhood_reserve(c, triples_host, n);
}

rgcn_status rgcn_sample_neighborhood_device(rgcn_ctx* c, int64_t sample_size, uint64_t seed, int32_t* batch_out_dev,
                                            int32_t on_prefetch_stream) {
  RGCN_NEED(c);
  if (c->nbr.n <= 0) RGCN_FAIL(c, RGCN_ERR_STATE, "call rgcn_neighborhood_reserve first");
  // the reference's loop dies on NaN probabilities when asked for more edges than the graph has
  if (sample_size < 0 || sample_size > c->nbr.n) RGCN_FAIL(c, RGCN_ERR_INVALID, "sample_size outside [0, number of training triples]");
  if (sample_size > 0 && !batch_out_dev) RGCN_FAIL(c, RGCN_ERR_INVALID, "NULL output");
  if (c->capturing) RGCN_FAIL(c, RGCN_ERR_STATE, "not while a hipGraph is being captured");
  invalidate_prefetch_of(c, batch_out_dev, sizeof(int32_t) * 3 * (size_t)sample_size);
  if (on_prefetch_stream) c->stream = c->pf_stream;
  const rgcn_status s = neighborhood_sample(c, sample_size, seed, batch_out_dev, on_prefetch_stream != 0);
  c->stream = c->main_stream;
  return s;
}

// ---- hipGraph capture of whole steps --------------------------------------------------------------
namespace {
__global__ void k_bump_counter(uint64_t* counter) { counter[0] += 1; }
}

rgcn_status rgcn_capture_begin(rgcn_ctx* c) {
  RGCN_NEED(c);
  RGCN_NO_EMBEDDING(c, "rgcn_capture_begin");
  if (c->capturing) RGCN_FAIL(c, RGCN_ERR_STATE, "a capture is already running");
  if (c->prof_on) RGCN_FAIL(c, RGCN_ERR_STATE, "switch the per-kernel profile off before capturing");
  if (c->onehot)
    RGCN_FAIL(c, RGCN_ERR_UNSUPPORTED, "rgcn_capture_begin: capture on an RGCN_INPUT_ONEHOT context is not supported (a captured "
                                       "one-hot step has never been replayed against a reference)");
  // Sharded contexts: the step contains RCCL collectives, which a stream capture records like any other launch.  That
  // path is exercised with device-side stand-in collectives of several ranks on ONE GPU only
  // (tests/test_gpu_multiprocess.py::test_captured_sharded_train_step); real librccl kernels inside a capture have never
  // run here (no multi-GPU box), so it stays EXPERIMENTAL and opt-in: RGCN_CAPTURE_SHARDED=1.
  if (c->highway)
    RGCN_FAIL(c, RGCN_ERR_UNSUPPORTED, "rgcn_capture_begin: capture on an RGCN_SKIP_HIGHWAY context is not supported (a captured "
                                       "highway step has never been replayed against a reference)");
  if (c->out_layer)
    RGCN_FAIL(c, RGCN_ERR_UNSUPPORTED, "rgcn_capture_begin: capture on a context with an output transform (code_dim > 0) is not "
                                       "supported (a captured step with the layer has never been replayed against a reference)");
  if (c->kind == RGCN_KIND_BASIS_TDIAG)
    RGCN_FAIL(c, RGCN_ERR_UNSUPPORTED, "rgcn_capture_begin: capture on an RGCN_KIND_BASIS_TDIAG context is not supported (a "
                                       "captured step of this kind has never been replayed against a reference)");
  if (c->kind == RGCN_KIND_BASIS_PDIAG)
    RGCN_FAIL(c, RGCN_ERR_UNSUPPORTED, "rgcn_capture_begin: capture on an RGCN_KIND_BASIS_PDIAG context is not supported (a "
                                       "captured step of this kind has never been replayed against a reference)");
  if (c->reciprocal)
    RGCN_FAIL(c, RGCN_ERR_UNSUPPORTED, "rgcn_capture_begin: reciprocal relations (rgcn_set_reciprocal_relations) are not built "
                                       "for a hipGraph capture");
  if (c->world > 1 && knob("RGCN_CAPTURE_SHARDED", 0) != 1)
    RGCN_FAIL(c, RGCN_ERR_UNSUPPORTED, "capture on a sharded context is experimental (never run against real RCCL on "
                                       "several GPUs): the devtools build enables it with RGCN_CAPTURE_SHARDED=1");
  RGCN_TRY(sync_all(c));
  if (!c->replay_counter) {
    RGCN_TRY(dmalloc(c, c->pool, &c->replay_counter, 1, false));
    RGCN_HIP(c, hipMemset(c->replay_counter, 0, sizeof(uint64_t)));
  }
  c->g.ready_in_capture = c->g.free_in_capture = false;
  c->g_alt.ready_in_capture = c->g_alt.free_in_capture = false;
  c->step_begin_in_capture = false;
  c->cap_pf_forked = false;
  RGCN_HIP(c, hipStreamBeginCapture(c->main_stream, hipStreamCaptureModeRelaxed));
  c->capturing = true;
  // whatever the capture does first, the weights' derived tables (MFMA fragments, band tiles) are rebuilt INSIDE it: a
  // replay follows weights the host does not see, tables built before the capture would be baked in stale
  c->frag_fresh = false;
  c->wtile_fresh = false;
  // A captured step is recorded as ONE chain on the main stream (only the prefetch of the next graph forks off):
  // the replayed graph pays more than streams do for every cross-stream edge (measured, profiles/r02_hipgraph_ab.log:
  // 0.687 ms per step with the side streams captured, 0.634-0.640 as a chain, 0.614-0.631 stream-launched), and
  // the side streams buy the stream-launched step under 3 % (the last A/B of the two captures: profiles/r06_hipgraph_ab.md).
  c->use_aux_before_capture = c->use_aux;
  c->use_aux = false;
  hipLaunchKernelGGL(k_bump_counter, dim3(1), dim3(1), 0, c->main_stream, c->replay_counter);
  return RGCN_OK;
}

rgcn_status rgcn_capture_end(rgcn_ctx* c, int32_t* graph_id) {
  RGCN_NEED(c);
  if (!c->capturing) RGCN_FAIL(c, RGCN_ERR_STATE, "no capture is running");
  if (!graph_id) RGCN_FAIL(c, RGCN_ERR_INVALID, "NULL graph_id");
  hipError_t e = hipSuccess;
  for (int k = 0; k < kAuxStreams; ++k)        // (side streams forked inside the capture rejoin the origin stream)
    if (c->use_aux && c->aux[k] && c->aux_dirty[k]) {
      c->aux_dirty[k] = false;
      if (e == hipSuccess) e = hipEventRecord(c->ev_join[k], c->aux[k]);
      if (e == hipSuccess) e = hipStreamWaitEvent(c->main_stream, c->ev_join[k], 0);
    }
  if (c->cap_pf_forked) {                      // the prefetch stream must rejoin the origin stream
    e = hipEventRecord(c->ev_join[0], c->pf_stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(c->main_stream, c->ev_join[0], 0);
  }
  hipGraph_t graph = nullptr;
  const hipError_t e2 = hipStreamEndCapture(c->main_stream, &graph);
  c->capturing = false;
  c->frag_fresh = false;
  c->wtile_fresh = false;
  c->use_aux = c->use_aux_before_capture;
  // events last recorded inside the capture are unusable outside it: give them a fresh, ordinary record
  (void)hipEventRecord(c->ev_fork, c->main_stream);
  (void)hipEventRecord(c->ev_step_begin, c->main_stream);
  for (int k = 0; k < kAuxStreams; ++k) if (c->aux[k]) (void)hipEventRecord(c->ev_join[k], c->aux[k]);
  for (rgcn::GraphBufs* g : {&c->g, &c->g_alt}) {
    if (g->ev_ready) (void)hipEventRecord(g->ev_ready, c->pf_stream);
    if (g->ev_free) (void)hipEventRecord(g->ev_free, c->main_stream);
    g->ready_in_capture = g->free_in_capture = false;
  }
  if (c->dec.ev_ready) (void)hipEventRecord(c->dec.ev_ready, c->main_stream);
  c->step_begin_in_capture = false;
  if (e != hipSuccess || e2 != hipSuccess || !graph) {
    if (graph) (void)hipGraphDestroy(graph);
    c->err = std::string("stream capture failed: ") + hipGetErrorString(e2 != hipSuccess ? e2 : e);
    return RGCN_ERR_HIP;
  }
  hipGraphExec_t exec = nullptr;
  e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
  if (e != hipSuccess) {
    (void)hipGraphDestroy(graph);
    c->err = std::string("hipGraphInstantiate: ") + hipGetErrorString(e);
    return RGCN_ERR_HIP;
  }
  c->graph_defs.push_back(graph);
  c->graphs.push_back(exec);
  *graph_id = (int32_t)c->graphs.size() - 1;
  return RGCN_OK;
}

rgcn_status rgcn_graph_launch(rgcn_ctx* c, int32_t graph_id) {
  RGCN_NEED(c);
  if (c->capturing) RGCN_FAIL(c, RGCN_ERR_STATE, "a capture is running");
  if (graph_id < 0 || graph_id >= (int32_t)c->graphs.size() || !c->graphs[graph_id])
    RGCN_FAIL(c, RGCN_ERR_INVALID, "unknown graph id");
  RGCN_TRY(join_abandoned_side_work(c));      // (the replayed steps rewrite everything unjoined side kernels touch)
  RGCN_HIP(c, hipGraphLaunch(c->graphs[graph_id], c->main_stream));
  c->fwd_done = true;       // the replayed steps leave activations / gradients of their last step behind
  c->weights_version += 1;  // a replayed train step moved the weights behind the host's back: derived weight tables
                            // (block_rows) built before the replay are stale for uncaptured passes
  return RGCN_OK;
}

rgcn_status rgcn_graph_destroy(rgcn_ctx* c, int32_t graph_id) {
  RGCN_NEED(c);
  if (graph_id < 0 || graph_id >= (int32_t)c->graphs.size() || !c->graphs[graph_id])
    RGCN_FAIL(c, RGCN_ERR_INVALID, "unknown graph id");
  RGCN_TRY(sync_all(c));
  (void)hipGraphExecDestroy(c->graphs[graph_id]);
  (void)hipGraphDestroy(c->graph_defs[graph_id]);
  c->graphs[graph_id] = nullptr;
  c->graph_defs[graph_id] = nullptr;
  return RGCN_OK;
}

rgcn_status rgcn_set_relation_owner(rgcn_ctx* c, const int32_t* owner, int32_t count) {
  RGCN_NEED(c);
  RGCN_NO_EMBEDDING(c, "rgcn_set_relation_owner");
  if (!owner || count != c->R) RGCN_FAIL(c, RGCN_ERR_INVALID, "owner must have RelationCount entries");
  for (int r = 0; r < count; ++r)
    if (owner[r] < 0 || owner[r] >= c->world) RGCN_FAIL(c, RGCN_ERR_INVALID, "owner[r] outside [0, world)");
  c->g.ready = false;
  c->g.pf_valid = false;
  c->g_alt.pf_valid = false;
  c->fwd_done = false;
  RGCN_TRY(sync_all(c));
  return to_dev(c, c->g.owner, owner, sizeof(int32_t) * (size_t)count);
}

rgcn_status rgcn_comm_unique_id(uint8_t id[128]) {
  if (!id) return RGCN_ERR_INVALID;
  return comm_unique_id(id);
}
rgcn_status rgcn_comm_init(rgcn_ctx* c, const uint8_t id[128]) {
  RGCN_NEED(c);
  if (!id) RGCN_FAIL(c, RGCN_ERR_INVALID, "NULL id");
  return comm_init(c, id);
}
rgcn_status rgcn_comm_info(rgcn_ctx* c, int32_t* comm_ranks, int32_t* comm_rank, int32_t* comm_device) {
  RGCN_NEED(c);
  return comm_info(c, comm_ranks, comm_rank, comm_device);
}

rgcn_status rgcn_device_info(int32_t device, int32_t* count, int64_t* pci_address) {
  if (!count || !pci_address) return RGCN_ERR_INVALID;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); n = 0; }
  *count = n;
  *pci_address = -1;
  if (device < 0 || device >= n) return RGCN_OK;
  int dom = 0, bus = 0, dev = 0;
  if (hipDeviceGetAttribute(&dom, hipDeviceAttributePciDomainID, device) != hipSuccess ||
      hipDeviceGetAttribute(&bus, hipDeviceAttributePciBusId, device) != hipSuccess ||
      hipDeviceGetAttribute(&dev, hipDeviceAttributePciDeviceId, device) != hipSuccess) {
    (void)hipGetLastError();
    return RGCN_ERR_HIP;
  }
  *pci_address = ((int64_t)dom << 16) | ((int64_t)(bus & 0xff) << 8) | (int64_t)(dev & 0xff);
  return RGCN_OK;
}

rgcn_status rgcn_comm_allreduce_sum(rgcn_ctx* c, float* dev, int64_t count) {
  RGCN_NEED(c);
  return comm_allreduce(c, dev, count);
}

rgcn_status rgcn_forward_begin(rgcn_ctx* c, int32_t train, uint64_t seed, const uint8_t* masks) {
  RGCN_NEED(c);
  return fwd_begin(c, train, seed, masks);
}
rgcn_status rgcn_forward_layer_partial(rgcn_ctx* c, int32_t l) { RGCN_NEED(c); return fwd_layer_partial(c, l); }
rgcn_status rgcn_forward_layer_finish(rgcn_ctx* c, int32_t l) { RGCN_NEED(c); return fwd_layer_finish(c, l); }
rgcn_status rgcn_backward_begin(rgcn_ctx* c, const float* dcodes_dev) { RGCN_NEED(c); return bwd_begin(c, dcodes_dev); }
rgcn_status rgcn_backward_layer_partial(rgcn_ctx* c, int32_t l) { RGCN_NEED(c); return bwd_layer_partial(c, l); }
rgcn_status rgcn_backward_layer_finish(rgcn_ctx* c, int32_t l) { RGCN_NEED(c); return bwd_layer_finish(c, l); }
rgcn_status rgcn_backward_end(rgcn_ctx* c) { RGCN_NEED(c); return bwd_end(c); }

static rgcn_status buffer_of(rgcn_ctx* c, int32_t which, void** p, int64_t* bytes) {
  const int64_t Vd = (int64_t)c->V * c->d * 4;
  if (c->embedding && which != RGCN_BUF_RANK_ENERGIES && which != RGCN_BUF_RANK_MIXED_SCORES &&
      which != RGCN_BUF_RELATION_ENERGIES && which != RGCN_BUF_NEGATIVE_TYPED_OPEN && which != RGCN_BUF_NEGATIVE_UNRESOLVED &&
      which != RGCN_BUF_NEGATIVE_RELATION_UNRESOLVED && which != RGCN_BUF_RELATION_SOFTMAX_ENERGIES &&
      which != RGCN_BUF_RELATION_SOFTMAX_G && which != RGCN_BUF_RELATION_SOFTMAX_DQ &&
      which != RGCN_BUF_ADVERSARIAL_WEIGHTS && which != RGCN_BUF_ENTITY_SOFTMAX_G && which != RGCN_BUF_ENTITY_SOFTMAX_DQ)
    RGCN_FAIL(c, RGCN_ERR_STATE, "an RGCN_KIND_EMBEDDING context has the ranking buffers only (no graph, no layer buffers)");
  switch (which) {
    case RGCN_BUF_NEGATIVE_TYPED_OPEN:
      if (!c->types.ready) RGCN_FAIL(c, RGCN_ERR_STATE, "no type sets (rgcn_type_sets_reserve first)");
      *p = c->types.open; *bytes = 8; return RGCN_OK;
    case RGCN_BUF_NEGATIVE_UNRESOLVED:
      if (c->known.count <= 0) RGCN_FAIL(c, RGCN_ERR_STATE, "no known positives (rgcn_known_positives_reserve first)");
      *p = c->known.unresolved; *bytes = 8; return RGCN_OK;
    case RGCN_BUF_NEGATIVE_RELATION_UNRESOLVED:
      if (c->known.count <= 0) RGCN_FAIL(c, RGCN_ERR_STATE, "no known positives (rgcn_known_positives_reserve first)");
      *p = c->known.relation_unresolved; *bytes = 8; return RGCN_OK;
    case RGCN_BUF_RELATION_SOFTMAX_ENERGIES:
    case RGCN_BUF_RELATION_SOFTMAX_G:
    case RGCN_BUF_RELATION_SOFTMAX_DQ:
      if (c->relsm.maxP <= 0) RGCN_FAIL(c, RGCN_ERR_STATE, "no relation-softmax buffers (rgcn_relation_softmax_reserve first)");
      if (which == RGCN_BUF_RELATION_SOFTMAX_DQ) { *p = c->relsm.dQ; *bytes = c->relsm.plan.chunk * c->dc * 4; }
      else {
        *p = which == RGCN_BUF_RELATION_SOFTMAX_G ? c->relsm.G : c->relsm.E;
        *bytes = c->relsm.plan.chunk * c->relsm.plan.padded_r * 4;
      }
      return RGCN_OK;
    case RGCN_BUF_ADVERSARIAL_WEIGHTS:
      if (!c->adv.w || c->adv.last_N <= 0)
        RGCN_FAIL(c, RGCN_ERR_STATE, "no fused step has run under rgcn_set_adversarial_negatives");
      *p = c->adv.w; *bytes = c->adv.last_N * 4; return RGCN_OK;
    case RGCN_BUF_ENTITY_SOFTMAX_G:
    case RGCN_BUF_ENTITY_SOFTMAX_DQ:
      if (c->entsm.maxP <= 0) RGCN_FAIL(c, RGCN_ERR_STATE, "no entity-softmax buffers (rgcn_entity_softmax_reserve first)");
      if (which == RGCN_BUF_ENTITY_SOFTMAX_DQ) { *p = c->entsm.dQ; *bytes = c->entsm.plan.chunk * c->dc * 4; }
      else { *p = c->entsm.E; *bytes = c->entsm.plan.chunk * c->entsm.plan.padded_v * 4; }
      return RGCN_OK;
    case RGCN_BUF_EXCHANGE:
      if (!c->exch) RGCN_FAIL(c, RGCN_ERR_STATE, "no exchange buffer on a world == 1 context");
      *p = c->exch; *bytes = Vd; return RGCN_OK;
    case RGCN_BUF_SELF: *p = c->self_buf; *bytes = Vd; return RGCN_OK;
    case RGCN_BUF_DSELF_EXCHANGE: {
      int l = c->bwd_layer;
      if (l < 1 || l > c->L) RGCN_FAIL(c, RGCN_ERR_STATE, "no backward layer in flight");
      *p = c->layers[l].gwself; *bytes = (int64_t)c->d * c->d * 4; return RGCN_OK;
    }
    case RGCN_BUF_DBASIS_EXCHANGE: {
      int l = c->bwd_layer;
      if (c->kind != RGCN_KIND_BASIS) RGCN_FAIL(c, RGCN_ERR_STATE, "basis kind only");
      if (l < 1 || l > c->L) RGCN_FAIL(c, RGCN_ERR_STATE, "no backward layer in flight");
      *p = c->layers[l].grel; *bytes = (int64_t)2 * c->B * c->d * c->d * 4; return RGCN_OK;
    }
    case RGCN_BUF_NORM_EXCHANGE:
      if (!c->opt.shard_sq) RGCN_FAIL(c, RGCN_ERR_STATE, "no sharded-norm buffer (world == 1, or no rgcn_optimizer_norm_partial yet)");
      *p = c->opt.shard_sq; *bytes = 4; return RGCN_OK;
    case RGCN_BUF_INDEG: *p = c->g.indeg; *bytes = (int64_t)c->V * 4; return RGCN_OK;
    case RGCN_BUF_OUTDEG: *p = c->g.outdeg; *bytes = (int64_t)c->V * 4; return RGCN_OK;
    case RGCN_BUF_ROWPTR: *p = c->g.row_ptr; *bytes = (int64_t)(c->V + 1) * 4; return RGCN_OK;
    case RGCN_BUF_PERM_VERTEX: *p = c->g.permv; *bytes = (int64_t)2 * c->g.E * 4; return RGCN_OK;
    case RGCN_BUF_PERM_RELATION: *p = c->g.permr; *bytes = (int64_t)2 * c->g.E * 4; return RGCN_OK;
    case RGCN_BUF_MSG_NORM: *p = c->g.m_norm; *bytes = (int64_t)2 * c->g.E * 4; return RGCN_OK;
    case RGCN_BUF_RANK_ENERGIES:
      if (!c->ranking.s) RGCN_FAIL(c, RGCN_ERR_STATE, "no score buffer (rgcn_rank_reserve first)");
      *p = c->ranking.s; *bytes = (int64_t)c->ranking.max * c->V * 4; return RGCN_OK;
    case RGCN_BUF_RANK_MIXED_SCORES:
      if (!c->ranking.mixed) RGCN_FAIL(c, RGCN_ERR_STATE, "no mixed scores (no rgcn_topk_mixed_device since the last rgcn_rank_reserve)");
      *p = c->ranking.mixed; *bytes = (int64_t)c->ranking.max * c->V * 4; return RGCN_OK;
    case RGCN_BUF_RELATION_ENERGIES:
      if (!c->ranking.rel) RGCN_FAIL(c, RGCN_ERR_STATE, "no relation energies (no relation query since the last rgcn_rank_reserve)");
      *p = c->ranking.rel; *bytes = (int64_t)c->ranking.max * c->R * 4; return RGCN_OK;
    case RGCN_BUF_HIGHWAY_INNER:
    case RGCN_BUF_HIGHWAY_GATE:
      if (!c->highway) RGCN_FAIL(c, RGCN_ERR_STATE, "not an RGCN_SKIP_HIGHWAY context");
      if (c->hw_last < 1) RGCN_FAIL(c, RGCN_ERR_STATE, "no rgcn_forward_layer_finish has run");
      *p = which == RGCN_BUF_HIGHWAY_INNER ? c->hw_N[c->hw_last] : c->hw_T[c->hw_last]; *bytes = Vd; return RGCN_OK;
    case RGCN_BUF_TDIAG_PRODUCTS:
      if (c->kind != RGCN_KIND_BASIS_TDIAG) RGCN_FAIL(c, RGCN_ERR_STATE, "not an RGCN_KIND_BASIS_TDIAG context");
      if (c->tdiag_last < 1) RGCN_FAIL(c, RGCN_ERR_STATE, "no rgcn_forward_layer_finish has run");
      *p = c->tdiag_P[c->tdiag_last]; *bytes = (int64_t)2 * c->V * c->B * c->d * 4; return RGCN_OK;
    case RGCN_BUF_PDIAG_MIX:
    case RGCN_BUF_PDIAG_AGG:
      if (c->kind != RGCN_KIND_BASIS_PDIAG) RGCN_FAIL(c, RGCN_ERR_STATE, "not an RGCN_KIND_BASIS_PDIAG context");
      if (c->pdiag_last < 1) RGCN_FAIL(c, RGCN_ERR_STATE, "no rgcn_forward_layer_finish has run");
      if (which == RGCN_BUF_PDIAG_MIX) { *p = c->pdiag_a[c->pdiag_last]; *bytes = (int64_t)2 * c->V * c->B * 4; }
      else { *p = c->pdiag_agg; *bytes = Vd; }
      return RGCN_OK;
    case RGCN_BUF_OUT_DH:
      if (!c->out_layer) RGCN_FAIL(c, RGCN_ERR_STATE, "not a context with an output transform (rgcn_config_ext::code_dim > 0)");
      if (!c->out_dh_valid) RGCN_FAIL(c, RGCN_ERR_STATE, "no backward pass has run");
      *p = c->out_dh; *bytes = Vd; return RGCN_OK;
    default: RGCN_FAIL(c, RGCN_ERR_INVALID, "unknown buffer id");
  }
}
rgcn_status rgcn_read_buffer(rgcn_ctx* c, int32_t which, void* host, int64_t bytes) {
  RGCN_NEED(c);
  void* p; int64_t n;
  RGCN_TRY(buffer_of(c, which, &p, &n));
  if (!host || bytes != n) RGCN_FAIL(c, RGCN_ERR_INVALID, "buffer size mismatch");
  return to_host(c, host, p, (size_t)n);
}
rgcn_status rgcn_write_buffer(rgcn_ctx* c, int32_t which, const void* host, int64_t bytes) {
  RGCN_NEED(c);
  void* p; int64_t n;
  RGCN_TRY(buffer_of(c, which, &p, &n));
  if (!host || bytes != n) RGCN_FAIL(c, RGCN_ERR_INVALID, "buffer size mismatch");
  if (which != RGCN_BUF_EXCHANGE && which != RGCN_BUF_DSELF_EXCHANGE && which != RGCN_BUF_NORM_EXCHANGE &&
      which != RGCN_BUF_DBASIS_EXCHANGE)
    RGCN_FAIL(c, RGCN_ERR_INVALID, "only the exchange buffers are writable");
  return to_dev(c, p, host, (size_t)n);
}

rgcn_status rgcn_device_alloc(rgcn_ctx* c, int64_t bytes, void** dev) {
  RGCN_NEED(c);
  if (!dev || bytes < 0) RGCN_FAIL(c, RGCN_ERR_INVALID, "bad arguments");
  RGCN_HIP(c, hipMalloc(dev, (size_t)(bytes ? bytes : 1)));
  return RGCN_OK;
}
rgcn_status rgcn_device_free(rgcn_ctx* c, void* dev) {
  RGCN_NEED(c);
  if (c->capturing) RGCN_FAIL(c, RGCN_ERR_STATE, "this call synchronises with the device: not allowed between rgcn_capture_begin and rgcn_capture_end");
  RGCN_HIP(c, hipStreamSynchronize(c->stream));
  if (dev) {
    for (int k = 0; k < 2; ++k)      // unjoined side kernels may still be reading it (the dcodes of rgcn_step_device)
      if (c->aux_dirty[k] && c->aux[k]) RGCN_HIP(c, hipStreamSynchronize(c->aux[k]));
    invalidate_prefetch_of(c, dev, 1);
    if (c->pf_stream) RGCN_HIP(c, hipStreamSynchronize(c->pf_stream));   // a prefetch may still be reading it
    RGCN_HIP(c, hipFree(dev));
  }
  return RGCN_OK;
}
rgcn_status rgcn_copy_to_device(rgcn_ctx* c, void* dev, const void* host, int64_t bytes) {
  RGCN_NEED(c);
  if (!dev || !host || bytes < 0) RGCN_FAIL(c, RGCN_ERR_INVALID, "bad arguments");
  invalidate_prefetch_of(c, dev, (size_t)bytes);
  RGCN_TRY(join_abandoned_side_work(c));      // (dev may be the dcodes unjoined side kernels still read)
  return to_dev(c, dev, host, (size_t)bytes);
}
rgcn_status rgcn_copy_to_device_async(rgcn_ctx* c, void* dev, const void* host, int64_t bytes,
                                      int32_t on_prefetch_stream) {
  RGCN_NEED(c);
  if (!dev || !host || bytes < 0) RGCN_FAIL(c, RGCN_ERR_INVALID, "bad arguments");
  if (c->capturing) RGCN_FAIL(c, RGCN_ERR_STATE, "host transfers are not allowed while a hipGraph is being captured");
  if (bytes == 0) return RGCN_OK;
  invalidate_prefetch_of(c, dev, (size_t)bytes);
  hipStream_t st = on_prefetch_stream ? c->pf_stream : c->main_stream;
  if (!on_prefetch_stream) {
    RGCN_TRY(join_abandoned_side_work(c));    // as rgcn_copy_to_device
  } else if (c->side_state != rgcn_ctx::SIDE_NONE) {
    RGCN_HIP(c, hipStreamWaitEvent(st, c->ev_join[0], 0));      // (behind every side kernel that reads; the main stream pays nothing)
  } else {
    for (int k = 0; k < 2; ++k)
      if (c->aux_dirty[k] && c->aux[k]) RGCN_HIP(c, hipStreamSynchronize(c->aux[k]));
  }
  if ((size_t)bytes > rgcn_ctx::kStageBytes) {      // too large for a staging slot: ordered on `st`, host waits
    RGCN_HIP(c, hipMemcpyAsync(dev, host, (size_t)bytes, hipMemcpyHostToDevice, st));
    RGCN_HIP(c, hipStreamSynchronize(st));
    return RGCN_OK;
  }
  if (!c->stage_host) {
    RGCN_HIP(c, hipHostMalloc((void**)&c->stage_host, rgcn_ctx::kStageSlots * rgcn_ctx::kStageBytes, hipHostMallocDefault));
    for (int k = 0; k < rgcn_ctx::kStageSlots; ++k)
      RGCN_HIP(c, hipEventCreateWithFlags(&c->stage_done[k], hipEventDisableTiming));
  }
  const int slot = c->stage_next;
  c->stage_next = (slot + 1) % rgcn_ctx::kStageSlots;
  RGCN_HIP(c, hipEventSynchronize(c->stage_done[slot]));      // the transfer that last used this slot has run
  uint8_t* stage = c->stage_host + (size_t)slot * rgcn_ctx::kStageBytes;
  memcpy(stage, host, (size_t)bytes);
  RGCN_HIP(c, hipMemcpyAsync(dev, stage, (size_t)bytes, hipMemcpyHostToDevice, st));
  RGCN_HIP(c, hipEventRecord(c->stage_done[slot], st));
  return RGCN_OK;
}
rgcn_status rgcn_copy_to_host(rgcn_ctx* c, void* host, const void* dev, int64_t bytes) {
  RGCN_NEED(c);
  if (!dev || !host || bytes < 0) RGCN_FAIL(c, RGCN_ERR_INVALID, "bad arguments");
  return to_host(c, host, dev, (size_t)bytes);
}

rgcn_status rgcn_timer_start(rgcn_ctx* c) {
  RGCN_NEED(c);
  if (c->capturing) RGCN_FAIL(c, RGCN_ERR_STATE, "not allowed between rgcn_capture_begin and rgcn_capture_end");
  RGCN_HIP(c, hipEventRecord(c->t0, c->stream));
  return RGCN_OK;
}
rgcn_status rgcn_timer_stop(rgcn_ctx* c, float* ms) {
  RGCN_NEED(c);
  if (c->capturing) RGCN_FAIL(c, RGCN_ERR_STATE, "not allowed between rgcn_capture_begin and rgcn_capture_end");
  if (!ms) RGCN_FAIL(c, RGCN_ERR_INVALID, "NULL output");
  RGCN_HIP(c, hipEventRecord(c->t1, c->stream));
  RGCN_HIP(c, hipEventSynchronize(c->t1));
  RGCN_HIP(c, hipEventElapsedTime(ms, c->t0, c->t1));
  return RGCN_OK;
}

rgcn_status rgcn_set_overlap(rgcn_ctx* c, int32_t on) {
  RGCN_NEED(c);
  RGCN_TRY(sync_all(c));
  c->use_aux = on != 0;
  return RGCN_OK;
}

rgcn_status rgcn_set_fusion(rgcn_ctx* c, int32_t mode) {
  RGCN_NEED(c);
  if (mode != 0 && mode != 1) RGCN_FAIL(c, RGCN_ERR_INVALID, "fusion mode must be 0 (two kernels) or 1 (single pass)");
  c->fuse = mode;
  return RGCN_OK;
}

rgcn_status rgcn_set_gemm_mode(rgcn_ctx* c, int32_t mode) {
  RGCN_NEED(c);
  if (mode != 0 && mode != 3 && mode != 6 && mode != 9) RGCN_FAIL(c, RGCN_ERR_INVALID, "gemm mode must be 0, 3, 6 or 9");
  c->gemm_mode = mode;
  return RGCN_OK;
}

rgcn_status rgcn_profile_enable(rgcn_ctx* c, int32_t on) {
  RGCN_NEED(c);
  if (!on && c->prof_on) RGCN_TRY(profile_collect(c));
  c->prof_on = on != 0;
  return RGCN_OK;
}
rgcn_status rgcn_profile_reset(rgcn_ctx* c) {
  RGCN_NEED(c);
  RGCN_TRY(profile_collect(c));
  c->prof_agg.clear();
  return RGCN_OK;
}
int32_t rgcn_profile_count(rgcn_ctx* c) {
  if (!c) return 0;
  (void)hipSetDevice(c->cfg.device);
  if (profile_collect(c) != RGCN_OK) return 0;
  return (int32_t)c->prof_agg.size();
}
rgcn_status rgcn_profile_get(rgcn_ctx* c, int32_t i, char* name, int32_t name_cap, int64_t* calls,
                             double* total_ms, double* alg_bytes, double* alg_flops) {
  RGCN_NEED(c);
  if (i < 0 || i >= (int32_t)c->prof_agg.size()) RGCN_FAIL(c, RGCN_ERR_INVALID, "profile index out of range");
  const ProfAgg& a = c->prof_agg[i];
  if (name && name_cap > 0) {
    strncpy(name, a.name.c_str(), (size_t)name_cap - 1);
    name[name_cap - 1] = 0;
  }
  if (calls) *calls = a.calls;
  if (total_ms) *total_ms = a.ms;
  if (alg_bytes) *alg_bytes = a.bytes;
  if (alg_flops) *alg_flops = a.flops;
  return RGCN_OK;
}
rgcn_status rgcn_profile_get_compulsory(rgcn_ctx* c, int32_t i, double* compulsory_bytes) {
  RGCN_NEED(c);
  if (i < 0 || i >= (int32_t)c->prof_agg.size()) RGCN_FAIL(c, RGCN_ERR_INVALID, "profile index out of range");
  if (compulsory_bytes) *compulsory_bytes = c->prof_agg[i].cbytes;
  return RGCN_OK;
}


}  // extern "C"
