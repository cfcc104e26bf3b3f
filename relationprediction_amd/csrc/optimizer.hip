// Optimizer step on the device: global-norm gradient clipping + one of the reference's three update rules over every
// trainable tensor ("next" row f2 of SURVEY.md 8f).  Reference chain (Appendix B): GradientClipping(max_norm) =
// tf.clip_by_global_norm (code/optimization/tensorflow_backend/algorithms.py:58-68) wrapped around the [Algorithm] the
// settings name (:5-55, optimizer_parameter_parser.py:55-64):
//
//   scale = max_norm / max(||g||_2, max_norm),  g = scale * gradient           (clip_by_global_norm; 1 when off)
//   Adam(lr) = tf.train.AdamOptimizer(lr, beta1=0.9, beta2=0.999), epsilon 1e-8 (:27-42)                     k_adam
//     lr_t = lr * sqrt(1 - beta2^t) / (1 - beta1^t);  m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2
//     w   -= lr_t * m / (sqrt(v) + eps)
//   GradientDescent(lr) = tf.train.GradientDescentOptimizer(lr) (:5-16): w -= lr g; no state                  k_sgd
//   AdaGrad(lr) = tf.train.AdagradOptimizer(lr) (:44-55): a += g^2;  w -= lr g / sqrt(a)                      k_adagrad
//     one accumulator per element, CREATED FILLED with initial_accumulator_value (TF's default 0.1) and no epsilon: the
//     fill is what keeps an element that never saw a gradient from 0 / 0, so it is part of the semantics.
//   The two constants of AdaGrad (0.1, no epsilon) and GradientDescent's plain form are TF 1.x's DOCUMENTED behaviour; no
//   TensorFlow was at hand to confirm them against an execution.
// One table-driven launch covers all tensors (device layouts: all three rules are elementwise, so the private
// block / basis weight layouts need no conversion); the norm is a two-stage fixed-order reduction whose
// result stays on the device -- no host synchronisation, the whole train step is one stream of launches.
// The unused per-layer bias `b` gets no gradient in TF (None) and is skipped; W_relation is updated on
// its first RelationCount rows only (the other rows never receive a gradient).
// Deviation kept on purpose: TF computes the global norm over UN-aggregated IndexedSlices for gathered
// weights; here gradients are already aggregated (trajectory parity with TF is unpinned either way).
// No such deviation in the two stateless-per-row rules: for a gathered tensor TF applies GradientDescent and AdaGrad
// SPARSELY, after summing duplicate indices (_apply_sparse_duplicate_indices), so a row nobody gathered keeps its weights
// and its accumulator -- and the dense formulas above do exactly that to a row whose aggregated gradient is zero
// (a += 0, w -= 0).  The dense elementwise pass over the aggregated gradient IS what the reference executes.
#include "rgcn_internal.h"

namespace rgcn {

namespace {

constexpr int kOptThreads = 256;
constexpr int kOptItems = 8;          // elements per thread
constexpr int kOptMaxTensors = 40;

struct OptTensor {
  float* w;
  const float* g;
  float* m;
  float* v;
  int64_t n;
  int32_t block0;     // first block of this tensor
};
struct OptTable {
  OptTensor t[kOptMaxTensors];
  int32_t count;
  int32_t nblocks;
};

__device__ __forceinline__ int find_tensor(const OptTable& tab, int b) {
  int lo = 0, hi = tab.count;
  while (hi - lo > 1) {
    int mid = (lo + hi) >> 1;
    if (tab.t[mid].block0 <= b) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ void __launch_bounds__(kOptThreads) k_sqnorm_part(OptTable tab, float* __restrict__ part) {
  __shared__ float red[kOptThreads / 64];
  const int ti = find_tensor(tab, blockIdx.x);
  const OptTensor t = tab.t[ti];
  const int64_t base = (int64_t)(blockIdx.x - t.block0) * kOptThreads * kOptItems;
  // 16 B per lane and load where the tensor starts on a 16-byte boundary (every hipMalloc'ed gradient does; a slice of
  // the contiguous replicated-gradient buffer of a sharded run need not); a tensor's last few elements one by one
  const bool aligned = (reinterpret_cast<uintptr_t>(t.g) & 15) == 0;
  float acc = 0.f;
  float4 q[kOptItems / 4];
#pragma unroll
  for (int k = 0; k < kOptItems / 4; ++k) {
    const int64_t i = base + ((int64_t)k * kOptThreads + threadIdx.x) * 4;
    q[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (aligned && i + 3 < t.n) {
      q[k] = *reinterpret_cast<const float4*>(t.g + i);
    } else if (i < t.n) {
      q[k].x = t.g[i];
      if (i + 1 < t.n) q[k].y = t.g[i + 1];
      if (i + 2 < t.n) q[k].z = t.g[i + 2];
      if (i + 3 < t.n) q[k].w = t.g[i + 3];
    }
  }
#pragma unroll
  for (int k = 0; k < kOptItems / 4; ++k) {
    acc = fmaf(q[k].x, q[k].x, acc);
    acc = fmaf(q[k].y, q[k].y, acc);
    acc = fmaf(q[k].z, q[k].z, acc);
    acc = fmaf(q[k].w, q[k].w, acc);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// state[0] = clip scale, state[1] = global norm (for inspection), state[2] = step count t, state[3] = the
// bias-corrected rate lr * sqrt(1 - beta2^t) / (1 - beta1^t).  t advances HERE, on the device, so that a
// captured hipGraph of the train step (rgcn_capture_*) keeps counting when it is replayed.
// Sum of a range of block partials, as one float: the squared norm of this rank's relation-sharded gradients,
// which a multi-GPU run sum-all-reduces before k_clip_scale adds it to the replicated tensors' partials.
__global__ void __launch_bounds__(256) k_sum_range(const float* __restrict__ part, int nparts, float* __restrict__ out) {
  __shared__ double red[256];
  double a = 0.0;
  for (int i = threadIdx.x; i < nparts; i += 256) a += part[i];
  red[threadIdx.x] = a;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = (float)red[0];
}

__global__ void __launch_bounds__(256) k_clip_scale(const float* __restrict__ part, int nparts,
                                                    const float* __restrict__ exchanged, float max_norm,
                                                    float lr, float b1, float b2, float* __restrict__ state) {
  __shared__ double red[256];
  double a = (exchanged && threadIdx.x == 0) ? (double)exchanged[0] : 0.0;
  // a thread's partials part[tid], part[tid + 256], ... added in that order -- but fetched eight at a time: one after the
  // other they are twenty dependent trips to the L2 (5,000 partials at FB15k-237 size), most of this kernel's time
  for (int i0 = threadIdx.x; i0 < nparts; i0 += 8 * 256) {
    float p[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) p[k] = i0 + k * 256 < nparts ? part[i0 + k * 256] : 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) if (i0 + k * 256 < nparts) a += p[k];
  }
  red[threadIdx.x] = a;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float norm = (float)sqrt(red[0]);
    state[1] = norm;
    state[0] = max_norm > 0.f ? max_norm / fmaxf(norm, max_norm) : 1.0f;
    const double t = (double)state[2] + 1.0;
    state[2] = (float)t;
    state[3] = (float)((double)lr * sqrt(1.0 - pow((double)b2, t)) / (1.0 - pow((double)b1, t)));
  }
}

__global__ void __launch_bounds__(kOptThreads) k_adam(OptTable tab, const float* __restrict__ state,
                                                      float b1, float b2, float eps) {
  const int ti = find_tensor(tab, blockIdx.x);
  const OptTensor t = tab.t[ti];
  const float scale = state[0], lr_t = state[3];
  const int64_t base = (int64_t)(blockIdx.x - t.block0) * kOptThreads * kOptItems;
#pragma unroll
  for (int k = 0; k < kOptItems; ++k) {
    const int64_t i = base + (int64_t)k * kOptThreads + threadIdx.x;
    if (i < t.n) {
      const float g = t.g[i] * scale;
      const float m = fmaf(b1, t.m[i], (1.0f - b1) * g);
      const float v = fmaf(b2, t.v[i], (1.0f - b2) * g * g);
      t.m[i] = m;
      t.v[i] = v;
      t.w[i] -= lr_t * m / (sqrtf(v) + eps);
    }
  }
}

// GradientDescent and AdaGrad: pure streaming passes, 12 B (read g, read + write w) and 20 B (+ read + write a) per
// element against Adam's 28 B.  The tensor table, the block -> tensor search and the 256 x 8 elements per workgroup are
// k_adam's; the element order inside a workgroup is k_sqnorm_part's: a lane moves 16 bytes per array where w, g and (AdaGrad)
// the accumulator of the tensor all start on a 16-byte boundary -- every hipMalloc'ed one does, a slice of the contiguous
// replicated-gradient buffer of a sharded run need not -- and the tensor's last few elements, or a whole unaligned
// tensor, go one by one.  Both quads of a lane are loaded before the first is stored: w, g and a come out of a table, the
// compiler cannot know they do not overlap and would not move a load over a store by itself.
template <bool kAdagrad>
__device__ __forceinline__ void update_element(float& w, float graw, float& a, float scale, float lr) {
  const float g = graw * scale;
  if (kAdagrad) {
    a = fmaf(g, g, a);
    w -= lr * g / sqrtf(a);
  } else {
    w -= lr * g;
  }
}

template <bool kAdagrad>
__device__ __forceinline__ void stream_update(const OptTable& tab, const float* __restrict__ state, float lr) {
  const int ti = find_tensor(tab, blockIdx.x);
  const OptTensor t = tab.t[ti];
  const float scale = state[0];
  const int64_t base = (int64_t)(blockIdx.x - t.block0) * kOptThreads * kOptItems;
  const uintptr_t starts = reinterpret_cast<uintptr_t>(t.w) | reinterpret_cast<uintptr_t>(t.g) |
                           (kAdagrad ? reinterpret_cast<uintptr_t>(t.m) : (uintptr_t)0);
  const bool aligned = (starts & 15) == 0;
  float4 gq[kOptItems / 4], wq[kOptItems / 4], aq[kOptItems / 4];
  bool vec[kOptItems / 4];
#pragma unroll
  for (int k = 0; k < kOptItems / 4; ++k) {
    const int64_t i = base + ((int64_t)k * kOptThreads + threadIdx.x) * 4;
    vec[k] = aligned && i + 3 < t.n;
    gq[k] = wq[k] = aq[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (vec[k]) {
      gq[k] = *reinterpret_cast<const float4*>(t.g + i);
      wq[k] = *reinterpret_cast<const float4*>(t.w + i);
      if (kAdagrad) aq[k] = *reinterpret_cast<const float4*>(t.m + i);
    }
  }
#pragma unroll
  for (int k = 0; k < kOptItems / 4; ++k) {
    const int64_t i = base + ((int64_t)k * kOptThreads + threadIdx.x) * 4;
    if (vec[k]) {
      update_element<kAdagrad>(wq[k].x, gq[k].x, aq[k].x, scale, lr);
      update_element<kAdagrad>(wq[k].y, gq[k].y, aq[k].y, scale, lr);
      update_element<kAdagrad>(wq[k].z, gq[k].z, aq[k].z, scale, lr);
      update_element<kAdagrad>(wq[k].w, gq[k].w, aq[k].w, scale, lr);
      *reinterpret_cast<float4*>(t.w + i) = wq[k];
      if (kAdagrad) *reinterpret_cast<float4*>(t.m + i) = aq[k];
    } else {
      for (int e = 0; e < 4; ++e) {
        if (i + e < t.n) {
          float w = t.w[i + e], a = kAdagrad ? t.m[i + e] : 0.f;
          update_element<kAdagrad>(w, t.g[i + e], a, scale, lr);
          t.w[i + e] = w;
          if (kAdagrad) t.m[i + e] = a;
        }
      }
    }
  }
}

__global__ void __launch_bounds__(kOptThreads) k_sgd(OptTable tab, const float* __restrict__ state, float lr) {
  stream_update<false>(tab, state, lr);
}
__global__ void __launch_bounds__(kOptThreads) k_adagrad(OptTable tab, const float* __restrict__ state, float lr) {
  stream_update<true>(tab, state, lr);
}

// a new AdaGrad accumulator's initial value (and the rows of W_relation's slot that carry no state, on the way to the host)
__global__ void __launch_bounds__(256) k_fill(float* __restrict__ p, int64_t n, float value) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) p[i] = value;
}

}  // namespace

namespace {

// Relation-sharded tensors: block W_forward / W_backward, basis C_forward / C_backward.  On a
// world > 1 context each rank holds the gradient of the relations it owns (zeros elsewhere), so their squared
// norm is a sum over ranks; everything else is replicated and identical on every rank.
bool is_sharded_param(const rgcn_ctx* c, const Param& p) {
  if (c->world <= 1) return false;
  const char* pre = c->kind == RGCN_KIND_BLOCK ? "W_" : "C_";
  return p.name.compare(0, 2, pre) == 0 && (p.name[2] == 'f' || p.name[2] == 'b') && p.name != "W_relation";
}

int slot_count_of(int32_t algorithm) {
  return algorithm == RGCN_OPT_ADAM ? 2 : algorithm == RGCN_OPT_ADAGRAD ? 1 : 0;
}

// elements of parameter i that the optimizer touches, and that carry state
int64_t updated_count(const rgcn_ctx* c, size_t i) {
  const Param& p = c->params[i];
  // rows >= RelationCount never get a gradient; under reciprocal relations rows >= 2 RelationCount
  return p.name == "W_relation" ? (int64_t)decoder_relations(c) * c->dc : p.count;
}

// elements the state slots of parameter i are allocated with: W_relation's hold the reciprocal rows whether or not the
// mode is on, so that rgcn_set_reciprocal_relations may come before or after the first step
int64_t slot_elements(const rgcn_ctx* c, size_t i) {
  const Param& p = c->params[i];
  if (p.name != "W_relation") return p.count;
  return (int64_t)(2 * (int64_t)c->R <= c->V ? 2 * c->R : c->R) * c->dc;
}

// the state slots of parameter i, created at their initial value (Adam: zeros; AdaGrad: init_acc) if they are not there
rgcn_status ensure_slots(rgcn_ctx* c, size_t i) {
  OptimizerState& o = c->opt;
  if (o.m.empty()) {
    o.m.assign(c->params.size(), nullptr);
    o.v.assign(c->params.size(), nullptr);
  }
  if (slot_count_of(o.algorithm) == 0 || o.m[i]) return RGCN_OK;
  const int64_t n = slot_elements(c, i);
  if (o.algorithm == RGCN_OPT_ADAM) {
    RGCN_TRY(dmalloc(c, o.pool, &o.m[i], (size_t)n, true));
    return dmalloc(c, o.pool, &o.v[i], (size_t)n, true);
  }
  RGCN_TRY(dmalloc(c, o.pool, &o.m[i], (size_t)n, false));
  return optimizer_fill(c, o.m[i], n, o.init_acc);
}

// the launch table: replicated tensors first (blocks [0, *nrep)), sharded ones behind them
rgcn_status build_table(rgcn_ctx* c, OptTable& tab, int* nrep, double* total) {
  OptimizerState& o = c->opt;
  tab.count = 0;
  int nblocks = 0;
  *total = 0;
  for (int pass = 0; pass < 2; ++pass) {
    for (size_t i = 0; i < c->params.size(); ++i) {
      const Param& p = c->params[i];
      if (p.no_grad) continue;                       // the never-used layer bias: TF returns None for it
      if ((int)is_sharded_param(c, p) != pass) continue;
      const int64_t n = updated_count(c, i);
      RGCN_TRY(ensure_slots(c, i));
      if (tab.count >= kOptMaxTensors) RGCN_FAIL(c, RGCN_ERR_UNSUPPORTED, "too many tensors for one optimizer launch");
      OptTensor& t = tab.t[tab.count++];
      t.w = p.val; t.g = p.grad; t.m = o.m[i]; t.v = o.v[i]; t.n = n; t.block0 = nblocks;
      nblocks += (int)((n + kOptThreads * kOptItems - 1) / (kOptThreads * kOptItems));
      *total += (double)n;
    }
    if (pass == 0) *nrep = nblocks;
  }
  tab.nblocks = nblocks;
  if ((size_t)nblocks > o.part_cap) {
    o.part_pool.release();
    o.part_cap = 0;
    RGCN_TRY(dmalloc(c, o.part_pool, &o.part, (size_t)nblocks, false));
    o.part_cap = (size_t)nblocks;
  }
  if (!o.state) RGCN_TRY(dmalloc(c, o.pool, &o.state, 4, true));
  if (c->world > 1 && !o.shard_sq) RGCN_TRY(dmalloc(c, o.pool, &o.shard_sq, 1, true));
  return RGCN_OK;
}

}  // namespace

// Phase 1: squared-norm partials of every gradient; on a sharded context the relation-sharded tensors' share
// ends in opt.shard_sq (RGCN_BUF_NORM_EXCHANGE), which the caller sum-all-reduces before phase 2.
rgcn_status optimizer_norm_partial(rgcn_ctx* c) {
  OptimizerState& o = c->opt;
  if (!o.configured) RGCN_FAIL(c, RGCN_ERR_STATE, "rgcn_optimizer_config was not called");
  OptTable tab;
  int nrep = 0;
  double total = 0;
  RGCN_TRY(build_table(c, tab, &nrep, &total));
  {
    ProfScope ps(c, "opt_grad_norm", 4.0 * total, 2.0 * total);
    hipLaunchKernelGGL(k_sqnorm_part, dim3(tab.nblocks), dim3(kOptThreads), 0, c->stream, tab, o.part);
    if (c->world > 1)
      hipLaunchKernelGGL(k_sum_range, dim3(1), dim3(256), 0, c->stream, o.part + nrep, tab.nblocks - nrep, o.shard_sq);
  }
  RGCN_HIP(c, hipGetLastError());
  o.norm_pending = true;
  return RGCN_OK;
}

// Phase 2: clip scale from the (exchanged) norm, then the configured algorithm's update on every tensor.
rgcn_status optimizer_apply(rgcn_ctx* c) {
  OptimizerState& o = c->opt;
  if (!o.norm_pending) RGCN_FAIL(c, RGCN_ERR_STATE, "rgcn_optimizer_apply without rgcn_optimizer_norm_partial");
  o.norm_pending = false;
  OptTable tab;
  int nrep = 0;
  double total = 0;
  RGCN_TRY(build_table(c, tab, &nrep, &total));
  o.t += 1;        // host-side mirror (exact only while no captured graph is replayed)
  c->weights_version += 1;   // derived copies of the weights (block-major tables) are stale after this step
  {
    ProfScope ps(c, "opt_clip_scale", 4.0 * tab.nblocks, 0);
    hipLaunchKernelGGL(k_clip_scale, dim3(1), dim3(256), 0, c->stream, o.part, nrep,
                       c->world > 1 ? (const float*)o.shard_sq : (const float*)nullptr, o.max_norm, o.lr, o.beta1,
                       o.beta2, o.state);
  }
  if (o.algorithm == RGCN_OPT_ADAM) {
    ProfScope ps(c, "opt_adam", 28.0 * total, 10.0 * total);
    hipLaunchKernelGGL(k_adam, dim3(tab.nblocks), dim3(kOptThreads), 0, c->stream, tab, o.state, o.beta1, o.beta2,
                       o.eps);
  } else if (o.algorithm == RGCN_OPT_ADAGRAD) {
    ProfScope ps(c, "opt_adagrad", 20.0 * total, 6.0 * total);
    hipLaunchKernelGGL(k_adagrad, dim3(tab.nblocks), dim3(kOptThreads), 0, c->stream, tab, o.state, o.lr);
  } else {
    ProfScope ps(c, "opt_sgd", 12.0 * total, 3.0 * total);
    hipLaunchKernelGGL(k_sgd, dim3(tab.nblocks), dim3(kOptThreads), 0, c->stream, tab, o.state, o.lr);
  }
  RGCN_HIP(c, hipGetLastError());
  return RGCN_OK;
}

int optimizer_slot_count(const rgcn_ctx* c) { return slot_count_of(c->opt.algorithm); }

float optimizer_slot_initial(const rgcn_ctx* c) { return c->opt.algorithm == RGCN_OPT_ADAGRAD ? c->opt.init_acc : 0.f; }

rgcn_status optimizer_fill(rgcn_ctx* c, float* dev, int64_t n, float value) {
  if (n <= 0) return RGCN_OK;
  const int64_t blocks = (n + 256 * 8 - 1) / (256 * 8);
  hipLaunchKernelGGL(k_fill, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, c->stream, dev, n, value);
  RGCN_HIP(c, hipGetLastError());
  return RGCN_OK;
}

rgcn_status optimizer_slot(rgcn_ctx* c, int32_t param, int32_t slot, float** dev, int64_t* n) {
  OptimizerState& o = c->opt;
  RGCN_TRY(ensure_slots(c, (size_t)param));
  *dev = slot == 0 ? o.m[param] : o.v[param];
  *n = updated_count(c, (size_t)param);
  return RGCN_OK;
}

rgcn_status optimizer_state_array(rgcn_ctx* c, float** state) {
  OptimizerState& o = c->opt;
  if (!o.state) RGCN_TRY(dmalloc(c, o.pool, &o.state, 4, true));
  *state = o.state;
  return RGCN_OK;
}

void optimizer_release_state(rgcn_ctx* c) {
  OptimizerState& o = c->opt;
  o.pool.release();      // moments / accumulators, state, shard_sq (`part` is scratch of a step: it stays)
  o.m.clear();
  o.v.clear();
  o.state = nullptr;
  o.shard_sq = nullptr;
  o.t = 0;
  o.norm_pending = false;
}

rgcn_status optimizer_step(rgcn_ctx* c) {
  RGCN_TRY(optimizer_norm_partial(c));
  if (c->world > 1) RGCN_TRY(comm_allreduce(c, c->opt.shard_sq, 1));
  return optimizer_apply(c);
}

void optimizer_free(rgcn_ctx* c) {
  c->opt.pool.release();
  c->opt.part_pool.release();
  c->opt = OptimizerState();
}

}  // namespace rgcn
