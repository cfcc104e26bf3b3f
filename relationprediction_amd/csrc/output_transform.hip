// The encoder's output transform (UseOutputTransform=Yes: code/common/model_builder.py:131-135,170-177, the dense
// AffineTransform of code/encoders/affine_transform.py:63-83 with use_bias=True, use_nonlinearity=False) on top of H_L:
//   codes = H_L . W_out + b_out            W_out [d, c], b_out [c]; no relu, no dropout, train and test mode alike
// The three contractions of the layer (H_L . W_out, dcodes . W_out^T, H_L^T . dcodes) are gemm_f32 calls made by the
// schedule (rgcn_schedule.hip) and db_out is column_sum's; here is the one HBM-bound pass between them:
//   k_row_bias   x [rows, cols], b [cols]  -> x[v][:] += b, in place
// fp32, 16-byte accesses where cols % 4 == 0 and both pointers allow, scalar otherwise.
#include "rgcn_internal.h"

namespace rgcn {

namespace {

template <int VEC>
__global__ void k_row_bias(float* __restrict__ x, const float* __restrict__ b, int64_t nvec, int cols) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < nvec; i += stride) {
    const int64_t off = i * VEC;
    const int col = (int)(off % cols);      // (VEC == 4: cols % 4 == 0, a vector never straddles two rows)
    if constexpr (VEC == 4) {
      float4 v = *reinterpret_cast<const float4*>(x + off);
      const float4 bb = *reinterpret_cast<const float4*>(b + col);
      v.x += bb.x; v.y += bb.y; v.z += bb.z; v.w += bb.w;
      *reinterpret_cast<float4*>(x + off) = v;
    } else {
      x[off] += b[col];
    }
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

rgcn_status add_row_bias(rgcn_ctx* c, float* x, const float* b, int rows, int cols) {
  const int64_t n = (int64_t)rows * cols;
  if (n <= 0) return RGCN_OK;
  ProfScope ps(c, "out_bias", 8.0 * n + 4.0 * cols, 1.0 * n);
  const bool vec4 = cols % 4 == 0 && aligned16(x) && aligned16(b);
  const int64_t nvec = vec4 ? n / 4 : n;
  int64_t blocks = (nvec + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  if (vec4) hipLaunchKernelGGL((k_row_bias<4>), dim3((unsigned)blocks), dim3(256), 0, c->stream, x, b, nvec, cols);
  else hipLaunchKernelGGL((k_row_bias<1>), dim3((unsigned)blocks), dim3(256), 0, c->stream, x, b, nvec, cols);
  RGCN_HIP(c, hipGetLastError());
  return RGCN_OK;
}

}  // namespace rgcn
