// Self-adversarial weights of the decoder's negatives on the device ([General] AdversarialTemperature;
// rgcn_adversarial_weights_device and the fused steps under rgcn_set_adversarial_negatives).  Not in the reference, which
// weighs every row 1 (code/decoders/bilinear_diag.py:32-34).
//
// A decoder batch of N rows is laid out as every sampler here writes it: the first P rows are the positives, and every
// later row i is a negative of positive i mod P, so positive b owns the K = N / P - 1 rows b + P, b + 2 P, ...  Their
// weights are K times the softmax of alpha x over the group (adversarial_weights.h, shared with the host); a positive's
// weight is 1.  The weights are constants of the loss: k_dec_energy / k_dec_energy_rel read them (decoder.hip), nothing
// differentiates through them.
//
// k_adv_weights: one wavefront per positive.  The positive's three rows sit in registers in k_dec_energy_rel's lane
// mapping (column vector c in lane c mod 64, T <= 4 vectors per lane), so an energy is that kernel's fmaf chain and
// shuffle reduction, bit for bit.  The negatives are reached by arithmetic on the row index -- no CSR, so the kernel can
// run right behind the forward pass, beside decoder_prepare.  For every negative the three ids are compared with the
// positive's and only the rows that differ are gathered: one row for an entity corruption or a relation row, up to
// three for a caller's own batch.  Two negatives' gathers are in flight together and the next two negatives' ids are
// requested before these rows are waited for.  The group's energies stay in LDS (kAdvCap per wavefront); a longer group
// keeps the rest in its own rows of the OUTPUT, which hold an energy until the weight replaces it.  Energy j of a group
// is written and read back by lane j mod 64 alone, so no store has to become visible to another lane.  The maximum
// and the sum are per-lane partials in index order, then a butterfly over the wavefront: a fixed order, no atomics.
// Rows wider than the register form (d / VEC > 256: decoder_compute's unfused case) walk all three rows per negative.
#include <algorithm>

#include "adversarial_weights.h"
#include "rgcn_internal.h"
#include "row_walk.h"

namespace rgcn {

namespace {

constexpr int kAdvCap = 512;        // energies of one group held in LDS (per wavefront; 8 KB per workgroup)
constexpr int kAdvMaxBlocks = 8192; // workgroups of four wavefronts; more positives than that are taken in turns

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
  return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

struct AdvRow {
  int s, r, o;
  bool ok;
};

// row i of the batch; past_end: a row that does not exist (the odd one of the last pair)
__device__ __forceinline__ AdvRow adv_row(const int32_t* __restrict__ X, const float* __restrict__ Y, int64_t i, bool exists,
                                          int V, int R, int lane, int32_t* errflag) {
  AdvRow q{0, 0, 0, false};
  if (!exists) return q;
  q.s = X[3 * i]; q.r = X[3 * i + 1]; q.o = X[3 * i + 2];
  q.ok = (unsigned)q.s < (unsigned)V && (unsigned)q.o < (unsigned)V && (unsigned)q.r < (unsigned)R;
  if (Y != nullptr && lane == 0 && Y[i] != 0.0f) atomicOr(errflag, 128);
  return q;
}

// T > 0: the register form, T vectors per lane; T == 0: the looped form
template <int VEC, int T>
__global__ void __launch_bounds__(256) k_adv_weights(const float* __restrict__ codes, const float* __restrict__ Wr,
                                                     const int32_t* __restrict__ X, const float* __restrict__ Y, int P,
                                                     int K, int V, int R, int d, float alpha, float* __restrict__ w,
                                                     int32_t* errflag) {
  constexpr int TR = T > 0 ? T : 1;
  __shared__ float en[4][kAdvCap];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nvec = d / VEC;
  for (int p = blockIdx.x * 4 + wave; p < P; p += gridDim.x * 4) {
    int s = X[3 * (int64_t)p], r = X[3 * (int64_t)p + 1], o = X[3 * (int64_t)p + 2];
    const bool pok = (unsigned)s < (unsigned)V && (unsigned)o < (unsigned)V && (unsigned)r < (unsigned)R;
    if (Y != nullptr && lane == 0 && Y[p] != 1.0f) atomicOr(errflag, 128);
    float ps[TR][VEC], pr[TR][VEC], po[TR][VEC];
#pragma unroll
    for (int t = 0; t < TR; ++t) {
#pragma unroll
      for (int k = 0; k < VEC; ++k) { ps[t][k] = 0.f; pr[t][k] = 0.f; po[t][k] = 0.f; }
      if constexpr (T > 0) {
        const int c = lane + 64 * t;
        if (pok && c < nvec) {
          vload<VEC>(codes + (size_t)s * d + (size_t)c * VEC, ps[t]);
          vload<VEC>(Wr + (size_t)r * d + (size_t)c * VEC, pr[t]);
          vload<VEC>(codes + (size_t)o * d + (size_t)c * VEC, po[t]);
        }
      }
    }
    if (!pok) { s = -1; r = -1; o = -1; }      // an id out of range: no row of a negative counts as shared with it
    if (lane == 0) w[p] = 1.0f;
    AdvRow nx[2];
    nx[0] = adv_row(X, Y, (int64_t)p + P, K > 0, V, R, lane, errflag);
    nx[1] = adv_row(X, Y, (int64_t)p + 2 * (int64_t)P, K > 1, V, R, lane, errflag);
    for (int t = 0; t < K; t += 2) {
      const AdvRow cu[2] = {nx[0], nx[1]};
      float x[2] = {0.f, 0.f};
      if constexpr (T > 0) {
        float a[2][TR][VEC], b[2][TR][VEC], e[2][TR][VEC];
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
          for (int tt = 0; tt < TR; ++tt) {
            const int c = lane + 64 * tt;
#pragma unroll
            for (int k = 0; k < VEC; ++k) { a[u][tt][k] = ps[tt][k]; b[u][tt][k] = pr[tt][k]; e[u][tt][k] = po[tt][k]; }
            if (cu[u].ok && c < nvec) {
              if (cu[u].s != s) vload<VEC>(codes + (size_t)cu[u].s * d + (size_t)c * VEC, a[u][tt]);
              if (cu[u].r != r) vload<VEC>(Wr + (size_t)cu[u].r * d + (size_t)c * VEC, b[u][tt]);
              if (cu[u].o != o) vload<VEC>(codes + (size_t)cu[u].o * d + (size_t)c * VEC, e[u][tt]);
            }
          }
        nx[0] = adv_row(X, Y, (int64_t)p + (int64_t)(t + 3) * P, t + 2 < K, V, R, lane, errflag);
        nx[1] = adv_row(X, Y, (int64_t)p + (int64_t)(t + 4) * P, t + 3 < K, V, R, lane, errflag);
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
          for (int tt = 0; tt < TR; ++tt) {
            const int c = lane + 64 * tt;
            if (c < nvec) {
#pragma unroll
              for (int k = 0; k < VEC; ++k) x[u] = fmaf(a[u][tt][k] * b[u][tt][k], e[u][tt][k], x[u]);
            }
          }
      } else {
        nx[0] = adv_row(X, Y, (int64_t)p + (int64_t)(t + 3) * P, t + 2 < K, V, R, lane, errflag);
        nx[1] = adv_row(X, Y, (int64_t)p + (int64_t)(t + 4) * P, t + 3 < K, V, R, lane, errflag);
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          if (!cu[u].ok) continue;
          const float* p1 = codes + (size_t)cu[u].s * d;
          const float* pb = Wr + (size_t)cu[u].r * d;
          const float* p2 = codes + (size_t)cu[u].o * d;
          for (int c = lane; c < nvec; c += 64) {
            float a[VEC], b[VEC], e[VEC];
            vload<VEC>(p1 + (size_t)c * VEC, a);
            vload<VEC>(pb + (size_t)c * VEC, b);
            vload<VEC>(p2 + (size_t)c * VEC, e);
#pragma unroll
            for (int k = 0; k < VEC; ++k) x[u] = fmaf(a[k] * b[k], e[k], x[u]);
          }
        }
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        x[0] += __shfl_down(x[0], off, 64);
        x[1] += __shfl_down(x[1], off, 64);
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int j = t + u;
        float xb = __shfl(x[u], 0, 64);
        if (!cu[u].ok) xb = -INFINITY;           // takes no part: weight 0 (adversarial_weights.h)
        if (j < K && lane == (j & 63)) {
          if (j < kAdvCap) en[wave][j] = xb;
          else w[(int64_t)p + (int64_t)(j + 1) * P] = xb;
        }
      }
    }
    // lane l holds (wrote, and now reads) the energies l, l + 64, ... of the group
    double M = -INFINITY;
    for (int j = lane; j < K; j += 64) {
      const float xj = j < kAdvCap ? en[wave][j] : w[(int64_t)p + (int64_t)(j + 1) * P];
      M = fmax(M, adv_scaled(xj, alpha));
    }
    M = wave_max(M);
    double sum = 0.0;
    for (int j = lane; j < K; j += 64) {
      const float xj = j < kAdvCap ? en[wave][j] : w[(int64_t)p + (int64_t)(j + 1) * P];
      sum += adv_term(adv_scaled(xj, alpha), M);
    }
    sum = wave_sum(sum);
    for (int j = lane; j < K; j += 64) {
      const int64_t i = (int64_t)p + (int64_t)(j + 1) * P;
      const float xj = j < kAdvCap ? en[wave][j] : w[i];
      w[i] = adv_weight(adv_term(adv_scaled(xj, alpha), M), sum, K);
    }
  }
}

// a caller's weights (rgcn_decoder_loss_backward_weighted_device): finite and not negative, or flag 256
__global__ void __launch_bounds__(256) k_adv_check_weights(const float* __restrict__ w, int64_t N, int32_t* errflag) {
  bool bad = false;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (int64_t)gridDim.x * 256) {
    const float v = w[i];
    bad = bad || !(v >= 0.f && v <= 3.0e38f);      // (false for NaN and for infinity)
  }
  if (bad) atomicOr(errflag, 256);
}

}  // namespace

int adversarial_lds_cap() { return kAdvCap; }

rgcn_status adversarial_check_weights(rgcn_ctx* c, const float* w_dev, int64_t N) {
  if (N <= 0) return RGCN_OK;
  const int64_t blocks = (N + 256 * 8 - 1) / (256 * 8);
  hipLaunchKernelGGL(k_adv_check_weights, dim3((unsigned)std::min<int64_t>(blocks, 4096)), dim3(256), 0, c->stream, w_dev,
                     N, c->g.errflag);
  RGCN_HIP(c, hipGetLastError());
  return RGCN_OK;
}

rgcn_status adversarial_weights(rgcn_ctx* c, const float* codes, const int32_t* X, const float* Y, int64_t N, int64_t P,
                                float alpha, float* w_out) {
  const int64_t K = N / P - 1;
  if (K == 0 || alpha == 0.f) return optimizer_fill(c, w_out, N, 1.0f);
  const int V = c->V, R = decoder_relations(c), d = c->dc;      // (2 R under reciprocal relations)
  const float* Wr = c->w_rel;
  const bool vec4 = (d % 4 == 0) && aligned16(codes) && aligned16(Wr);
  const int nvec = vec4 ? d / 4 : d;
  const int T = nvec <= 64 ? 1 : (nvec <= 128 ? 2 : (nvec <= 256 ? 4 : 0));
  const int blocks = (int)std::min<int64_t>((P + 3) / 4, kAdvMaxBlocks);
  // design: the positive's three rows and one row per negative (an entity corruption or a relation row; a caller's own
  // batch and the looped form gather up to three), the batch and the labels once, the weights once
  ProfScope ps(c, "adv_weights", 4.0 * d * (3.0 * P + (T > 0 ? 1.0 : 3.0) * (double)K * P) + 20.0 * N, 6.0 * N * d,
               4.0 * d * ((double)V + R) + 20.0 * N);
#define RGCN_LAUNCH_ADV(VEC, TT)                                                                                        \
  hipLaunchKernelGGL((k_adv_weights<VEC, TT>), dim3(blocks), dim3(256), 0, c->stream, codes, Wr, X, Y, (int)P, (int)K, V, \
                     R, d, alpha, w_out, c->g.errflag)
  if (vec4) {
    if (T == 1) RGCN_LAUNCH_ADV(4, 1); else if (T == 2) RGCN_LAUNCH_ADV(4, 2); else if (T == 4) RGCN_LAUNCH_ADV(4, 4);
    else RGCN_LAUNCH_ADV(4, 0);
  } else {
    if (T == 1) RGCN_LAUNCH_ADV(1, 1); else if (T == 2) RGCN_LAUNCH_ADV(1, 2); else if (T == 4) RGCN_LAUNCH_ADV(1, 4);
    else RGCN_LAUNCH_ADV(1, 0);
  }
#undef RGCN_LAUNCH_ADV
  RGCN_HIP(c, hipGetLastError());
  return RGCN_OK;
}

void adversarial_free(rgcn_ctx* c) {
  c->adv.pool.release();
  const float t = c->adv.temperature;
  const int64_t sp = c->adv.step_positives;
  c->adv = AdversarialState();
  c->adv.temperature = t;
  c->adv.step_positives = sp;
}

// the fused steps' weight buffer: as many rows as the decoder is reserved for
rgcn_status adversarial_reserve(rgcn_ctx* c, int64_t rows) {
  if (c->adv.cap >= rows && c->adv.w) return RGCN_OK;
  adversarial_free(c);
  RGCN_TRY(dmalloc(c, c->adv.pool, &c->adv.w, (size_t)rows, false));
  c->adv.cap = rows;
  return RGCN_OK;
}

}  // namespace rgcn
