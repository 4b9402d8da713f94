// Elementwise exact (erf) GELU and its derivative: the transformer's `transformer_act: gelu`
// (transformers.py:265-273 returns F.gelu) wherever the feed-forward does not run as the fused
// launch of ffn.hip -- post-norm, d_model 512, the bf16 mode, training.
//
//   forward   y  = 0.5 z (1 + erf(z / sqrt 2))
//   backward  dz = dy (Phi(z) + z phi(z)),  Phi(z) = 0.5 (1 + erf(z / sqrt 2)),
//                                           phi(z) = exp(-z^2 / 2) / sqrt(2 pi)
//
// the formulas torch's fp32 F.gelu and its gradient evaluate. Memory-bound: one 16-B load and
// store per lane and iteration of a grid-stride loop, a scalar tail for n % 4. The tails are
// safe: for z <= -6 erff returns -1 and the product is 0 (0.5 z * 0, no 0 * inf: z is finite
// or the result is NaN as torch's is); for z >= 6 it returns 1 and y = z; in the backward
// z^2 may overflow to inf, exp(-inf) = 0 and z * 0 = 0 for every finite z.
#include "common.h"

namespace fgr {
namespace {

constexpr float kRsqrt2 = 0.70710678118654752440f;      // 1 / sqrt 2
constexpr float kRsqrt2Pi = 0.39894228040143267794f;    // 1 / sqrt(2 pi)

__device__ __forceinline__ float gelu_f(float z) { return 0.5f * z * (1.f + erff(z * kRsqrt2)); }
__device__ __forceinline__ float gelu_grad_f(float z, float dy) {
    const float cdf = 0.5f * (1.f + erff(z * kRsqrt2));
    const float pdf = expf(-0.5f * z * z) * kRsqrt2Pi;
    return dy * fmaf(z, pdf, cdf);
}

constexpr int kGeluBlock = 256;
constexpr int kGeluMaxBlocks = 256 * 8;                 // 8 blocks per CU: enough loads in flight

__global__ void __launch_bounds__(kGeluBlock)
gelu_fwd_kernel(const float* z, float* y, int64_t n) {
    const int64_t n4 = n / 4, stride = (int64_t)gridDim.x * kGeluBlock;
    const int64_t tid = (int64_t)blockIdx.x * kGeluBlock + threadIdx.x;
    for (int64_t i = tid; i < n4; i += stride) {
        const float4 v = reinterpret_cast<const float4*>(z)[i];
        reinterpret_cast<float4*>(y)[i] = make_float4(gelu_f(v.x), gelu_f(v.y), gelu_f(v.z), gelu_f(v.w));
    }
    const int64_t i = 4 * n4 + tid;                       // the n % 4 tail
    if (i < n) y[i] = gelu_f(z[i]);
}

__global__ void __launch_bounds__(kGeluBlock)
gelu_bwd_kernel(const float* z, const float* dy, float* dz, int64_t n) {
    const int64_t n4 = n / 4, stride = (int64_t)gridDim.x * kGeluBlock;
    const int64_t tid = (int64_t)blockIdx.x * kGeluBlock + threadIdx.x;
    for (int64_t i = tid; i < n4; i += stride) {
        const float4 v = reinterpret_cast<const float4*>(z)[i];
        const float4 g = reinterpret_cast<const float4*>(dy)[i];
        reinterpret_cast<float4*>(dz)[i] =
            make_float4(gelu_grad_f(v.x, g.x), gelu_grad_f(v.y, g.y), gelu_grad_f(v.z, g.z),
                        gelu_grad_f(v.w, g.w));
    }
    const int64_t i = 4 * n4 + tid;
    if (i < n) dz[i] = gelu_grad_f(z[i], dy[i]);
}

inline unsigned gelu_blocks(int64_t n) {
    return (unsigned)std::min<int64_t>(kGeluMaxBlocks, ceil_div(std::max<int64_t>(n / 4, 1), kGeluBlock));
}
// [a, a + n) and [b, b + n) are the same range or disjoint
inline bool same_or_disjoint(const float* a, const float* b, int64_t n) {
    return a == b || a + n <= b || b + n <= a;
}
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace
}  // namespace fgr

using namespace fgr;

extern "C" int fgr_gelu_fwd(const float* z, float* y, int64_t n, void* stream) {
    FGR_REQUIRE(n >= 0, "fgr_gelu_fwd: n %lld < 0", (long long)n);
    if (n == 0) return FGR_OK;
    FGR_REQUIRE(z && y, "fgr_gelu_fwd: null pointer");
    FGR_REQUIRE(aligned16(z) && aligned16(y), "fgr_gelu_fwd: z and y must be 16-B aligned");
    FGR_REQUIRE(same_or_disjoint(z, y, n), "fgr_gelu_fwd: y overlaps z partially");
    hipLaunchKernelGGL(gelu_fwd_kernel, dim3(gelu_blocks(n)), dim3(kGeluBlock), 0, as_stream(stream),
                       z, y, n);
    FGR_CHECK_LAUNCH("gelu_fwd_kernel");
    return FGR_OK;
}

extern "C" int fgr_gelu_bwd(const float* z, const float* dy, float* dz, int64_t n, void* stream) {
    FGR_REQUIRE(n >= 0, "fgr_gelu_bwd: n %lld < 0", (long long)n);
    if (n == 0) return FGR_OK;
    FGR_REQUIRE(z && dy && dz, "fgr_gelu_bwd: null pointer");
    FGR_REQUIRE(aligned16(z) && aligned16(dy) && aligned16(dz),
                "fgr_gelu_bwd: z, dy and dz must be 16-B aligned");
    FGR_REQUIRE(same_or_disjoint(dy, dz, n) && same_or_disjoint(z, dz, n),
                "fgr_gelu_bwd: dz overlaps dy or z partially");
    hipLaunchKernelGGL(gelu_bwd_kernel, dim3(gelu_blocks(n)), dim3(kGeluBlock), 0, as_stream(stream),
                       z, dy, dz, n);
    FGR_CHECK_LAUNCH("gelu_bwd_kernel");
    return FGR_OK;
}
