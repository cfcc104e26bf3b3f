// Highway skip connections around the graph-convolution layers (SkipConnections=Highway: code/extras/highway_layer.py,
// code/common/model_builder.py:273-309):
//   T_l = sigmoid(H_{l-1} . W_hw_l + b_hw_l)
//   H_l = T_l * N_l + (1 - T_l) * H_{l-1}             N_l = what layer l returns without the skip connection
// The three d x d contractions of a layer (the gate product, dZ . W_hw^T, H_{l-1}^T . dZ) are gemm_f32 calls made by the
// schedule (rgcn_schedule.hip); here are the HBM-bound [V,d] passes between them:
//   k_highway_fwd   Z, b_hw, N_l, H_{l-1}                 -> T_l (over Z, in place), H_l
//   k_highway_bwd   G_l = dL/dH_l, T_l, N_l, H_{l-1}      -> D_l = G T relu'(N), dS_l = D_l * dropout_l,
//                                                            dZ_l = G (N - H) T (1 - T), carry = G (1 - T),
//                                                            per-workgroup column partials of dZ_l (db_hw_l)
//   k_highway_join  raw dH_{l-1} of the layer's own backward, dZ_l . W_hw^T, carry -> G_{l-1}; at l = 1 also relu'(H_0)
//                   and the column partials of the result (db_emb)
// fp32, 16-byte accesses where d % 4 == 0 and the pointers allow, scalar otherwise.  No atomics: the column partials are
// one [d] row per workgroup, summed over a workgroup's row lanes in lane order and over the workgroups by k_colsum_final
// (column_sum_finish) in its fixed order -- bitwise repeatable.
#include "rgcn_internal.h"

namespace rgcn {

namespace {

constexpr int kHwThreads = 256;
constexpr int kHwMaxBlocks = 1024;      // grid cap of the row-lane kernels (= column-partial rows at most)

template <int VEC>
__device__ __forceinline__ void hw_load(const float* p, float (&v)[VEC]) {
  if constexpr (VEC == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
    v[0] = *p;
  }
}
template <int VEC>
__device__ __forceinline__ void hw_store(float* p, const float (&v)[VEC]) {
  if constexpr (VEC == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  else *p = v[0];
}

// sigmoid without special cases: z = +inf -> 1 / (1 + 0) = 1, z = -inf -> 1 / (1 + inf) = 0
__device__ __forceinline__ float hw_sigmoid(float z) { return 1.0f / (1.0f + __expf(-z)); }

template <int VEC>
__global__ void __launch_bounds__(kHwThreads) k_highway_fwd(float* T, const float* __restrict__ b,
                                                            const float* __restrict__ N, const float* __restrict__ Hin,
                                                            float* __restrict__ H, int64_t nvec_total, int d) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < nvec_total; i += stride) {
    const int64_t off = i * VEC;
    const int col = (int)(off % d);
    float z[VEC], bb[VEC], n[VEC], h[VEC], t[VEC], o[VEC];
    hw_load<VEC>(T + off, z);
    hw_load<VEC>(b + col, bb);
    hw_load<VEC>(N + off, n);
    hw_load<VEC>(Hin + off, h);
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      t[k] = hw_sigmoid(z[k] + bb[k]);
      o[k] = t[k] * n[k] + (1.0f - t[k]) * h[k];
    }
    hw_store<VEC>(T + off, t);
    hw_store<VEC>(H + off, o);
  }
}

// The row-lane layout of the two backward kernels: a workgroup is CL column lanes (VEC columns each) x 256 / CL row lanes;
// row lane rl of workgroup b walks the rows b * RL + rl, + gridDim.x * RL, ...  A thread's column sum over its rows stays
// in registers; the row lanes of a column meet in LDS and are added in lane order -> part[b][col].
template <int VEC>
__device__ __forceinline__ void hw_column_partial(const float (&acc)[VEC], float* red, int cl, int rl, int CL, int RL,
                                                  int cidx, int nvec, float* __restrict__ part, int d) {
  __syncthreads();       // (the previous column chunk's sums have been read)
#pragma unroll
  for (int k = 0; k < VEC; ++k) red[((size_t)rl * CL + cl) * VEC + k] = acc[k];
  __syncthreads();
  if (rl == 0 && cidx < nvec) {
    float tot[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      float t = 0.0f;
      for (int q = 0; q < RL; ++q) t += red[((size_t)q * CL + cl) * VEC + k];
      tot[k] = t;
    }
    hw_store<VEC>(part + (size_t)blockIdx.x * d + (size_t)cidx * VEC, tot);
  }
}

struct HighwayBwdArgs {
  const float* G;        // dL/dH_l (may be D: in place)
  const float* T;
  const float* N;
  const float* Hin;
  float* D;              // G T relu'(N)
  float* dS;             // optional: D * dropout_l
  float* dZ;
  float* carry;
  float* part;           // [gridDim.x][d] column partials of dZ
  int32_t V, d, relu, CL;
  DropSpec drop;
};

template <int VEC>
__global__ void __launch_bounds__(kHwThreads) k_highway_bwd(HighwayBwdArgs a) {
  __shared__ float red[kHwThreads * VEC];
  const int CL = a.CL, RL = kHwThreads / CL;
  const int cl = threadIdx.x % CL, rl = threadIdx.x / CL;
  const int nvec = a.d / VEC;
  const DropKey key = drop_key(a.drop);
  for (int c0 = 0; c0 < nvec; c0 += CL) {
    const int cidx = c0 + cl;
    float acc[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = 0.0f;
    if (cidx < nvec) {
      for (int64_t r = (int64_t)blockIdx.x * RL + rl; r < a.V; r += (int64_t)gridDim.x * RL) {
        const size_t off = (size_t)r * a.d + (size_t)cidx * VEC;
        float g[VEC], t[VEC], n[VEC], h[VEC], D[VEC], dz[VEC], cy[VEC];
        hw_load<VEC>(a.G + off, g);
        hw_load<VEC>(a.T + off, t);
        hw_load<VEC>(a.N + off, n);
        hw_load<VEC>(a.Hin + off, h);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
          const float gt = g[k] * t[k];
          D[k] = (a.relu && !(n[k] > 0.0f)) ? 0.0f : gt;
          dz[k] = gt * (n[k] - h[k]) * (1.0f - t[k]);
          cy[k] = g[k] * (1.0f - t[k]);
          acc[k] += dz[k];
        }
        hw_store<VEC>(a.D + off, D);
        hw_store<VEC>(a.dZ + off, dz);
        hw_store<VEC>(a.carry + off, cy);
        if (a.dS != nullptr) {
          float s[VEC];
#pragma unroll
          for (int k = 0; k < VEC; ++k) s[k] = D[k] * drop_factor(a.drop, key, off + k);
          hw_store<VEC>(a.dS + off, s);
        }
      }
    }
    hw_column_partial<VEC>(acc, red, cl, rl, CL, RL, cidx, nvec, a.part, a.d);
  }
}

// out = out + gz + carry (in place over the layer's raw dH); gate != nullptr (l = 1): *= relu'(H_0), column partials
template <int VEC>
__global__ void __launch_bounds__(kHwThreads) k_highway_join(float* out, const float* __restrict__ gz,
                                                             const float* __restrict__ carry,
                                                             const float* __restrict__ gate, float* __restrict__ part,
                                                             int V, int d, int CL) {
  __shared__ float red[kHwThreads * VEC];
  const int RL = kHwThreads / CL;
  const int cl = threadIdx.x % CL, rl = threadIdx.x / CL;
  const int nvec = d / VEC;
  for (int c0 = 0; c0 < nvec; c0 += CL) {
    const int cidx = c0 + cl;
    float acc[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = 0.0f;
    if (cidx < nvec) {
      for (int64_t r = (int64_t)blockIdx.x * RL + rl; r < V; r += (int64_t)gridDim.x * RL) {
        const size_t off = (size_t)r * d + (size_t)cidx * VEC;
        float x[VEC], z[VEC], cy[VEC];
        hw_load<VEC>(out + off, x);
        hw_load<VEC>(gz + off, z);
        hw_load<VEC>(carry + off, cy);
#pragma unroll
        for (int k = 0; k < VEC; ++k) x[k] = (x[k] + z[k]) + cy[k];
        if (gate != nullptr) {
          float gt[VEC];
          hw_load<VEC>(gate + off, gt);
#pragma unroll
          for (int k = 0; k < VEC; ++k) x[k] = gt[k] > 0.0f ? x[k] : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[k] += x[k];
        hw_store<VEC>(out + off, x);
      }
    }
    if (part != nullptr) hw_column_partial<VEC>(acc, red, cl, rl, CL, RL, cidx, nvec, part, d);      // (uniform branch)
  }
}

bool hw_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// column lanes of the row-lane kernels: the power of two that covers nvec, at most the workgroup
int hw_column_lanes(int nvec) {
  int cl = 1;
  while (cl < nvec && cl < kHwThreads) cl *= 2;
  return cl;
}
// workgroups: every row lane of the grid gets a row, capped; the partial rows must fit the context's column-sum scratch
int hw_row_grid(const rgcn_ctx* c, int CL) {
  const int RL = kHwThreads / CL;
  int64_t g = ((int64_t)c->V + RL - 1) / RL;
  if (g > kHwMaxBlocks) g = kHwMaxBlocks;
  if (g < 1) g = 1;
  return (int)g;
}

}  // namespace

rgcn_status highway_forward(rgcn_ctx* c, float* T, const float* b, const float* N, const float* Hin, float* H) {
  const int64_t n = (int64_t)c->V * c->d;
  ProfScope ps(c, "highway_fwd", 20.0 * n, 8.0 * n);
  const bool vec4 = c->d % 4 == 0 && hw_aligned16(T) && hw_aligned16(b) && hw_aligned16(N) && hw_aligned16(Hin) &&
                    hw_aligned16(H);
  const int64_t nvec = vec4 ? n / 4 : n;
  int64_t grid = (nvec + kHwThreads - 1) / kHwThreads;
  if (grid > 8192) grid = 8192;
  if (grid < 1) grid = 1;
  if (vec4)
    hipLaunchKernelGGL((k_highway_fwd<4>), dim3((unsigned)grid), dim3(kHwThreads), 0, c->stream, T, b, N, Hin, H, nvec, c->d);
  else
    hipLaunchKernelGGL((k_highway_fwd<1>), dim3((unsigned)grid), dim3(kHwThreads), 0, c->stream, T, b, N, Hin, H, nvec, c->d);
  RGCN_HIP(c, hipGetLastError());
  return RGCN_OK;
}

rgcn_status highway_backward(rgcn_ctx* c, const float* G, const float* T, const float* N, const float* Hin, float* D,
                             float* dS, float* dZ, float* carry, int relu, const DropSpec& drop, int* nparts) {
  HighwayBwdArgs a;
  a.G = G; a.T = T; a.N = N; a.Hin = Hin; a.D = D; a.dS = dS; a.dZ = dZ; a.carry = carry;
  a.part = colsum_scratch(c);
  a.V = c->V; a.d = c->d; a.relu = relu; a.drop = drop;
  const bool vec4 = c->d % 4 == 0 && hw_aligned16(G) && hw_aligned16(T) && hw_aligned16(N) && hw_aligned16(Hin) &&
                    hw_aligned16(D) && hw_aligned16(dS) && hw_aligned16(dZ) && hw_aligned16(carry) && hw_aligned16(a.part);
  a.CL = hw_column_lanes(vec4 ? c->d / 4 : c->d);
  const int grid = hw_row_grid(c, a.CL);
  if ((size_t)grid * c->d > c->colsum_part_floats) RGCN_FAIL(c, RGCN_ERR_STATE, "internal: column-sum scratch too small");
  const double n = (double)c->V * c->d;
  ProfScope ps(c, "highway_bwd", 4.0 * n * (dS ? 8.0 : 7.0), 10.0 * n);
  if (vec4) hipLaunchKernelGGL((k_highway_bwd<4>), dim3(grid), dim3(kHwThreads), 0, c->stream, a);
  else hipLaunchKernelGGL((k_highway_bwd<1>), dim3(grid), dim3(kHwThreads), 0, c->stream, a);
  RGCN_HIP(c, hipGetLastError());
  *nparts = grid;
  return RGCN_OK;
}

rgcn_status highway_join(rgcn_ctx* c, float* out, const float* gz, const float* carry, const float* gate, int* nparts) {
  float* part = gate != nullptr ? colsum_scratch(c) : nullptr;
  const bool vec4 = c->d % 4 == 0 && hw_aligned16(out) && hw_aligned16(gz) && hw_aligned16(carry) && hw_aligned16(gate) &&
                    hw_aligned16(part);
  const int CL = hw_column_lanes(vec4 ? c->d / 4 : c->d);
  const int grid = hw_row_grid(c, CL);
  if (part && (size_t)grid * c->d > c->colsum_part_floats) RGCN_FAIL(c, RGCN_ERR_STATE, "internal: column-sum scratch too small");
  const double n = (double)c->V * c->d;
  ProfScope ps(c, "highway_join", 4.0 * n * (gate ? 5.0 : 4.0), 3.0 * n);
  if (vec4)
    hipLaunchKernelGGL((k_highway_join<4>), dim3(grid), dim3(kHwThreads), 0, c->stream, out, gz, carry, gate, part, c->V, c->d, CL);
  else
    hipLaunchKernelGGL((k_highway_join<1>), dim3(grid), dim3(kHwThreads), 0, c->stream, out, gz, carry, gate, part, c->V, c->d, CL);
  RGCN_HIP(c, hipGetLastError());
  *nparts = part ? grid : 0;
  return RGCN_OK;
}

}  // namespace rgcn
