// Weighted Procrustes (Kabsch) with a 3x3 Jacobi SVD, one block per problem.
//
// Restates fast_compute_rigid_transform (utils/se3_torch.py:226-273):
//   w <- w if w > threshold else 0                         (:240-242)
//   wn = w / max(sum w, 1e-6); ca = sum a wn; cb = sum b wn (:248-251)
//   H  = (a - ca)^T ((b - cb) wn)                          (:252-254)
//   U S V^T = svd(H); R = V U^T, or V diag(1,1,-1) U^T if det(V U^T) <= 0  (:264-269)
//   t  = -R ca + cb                                        (:272)
// Reductions and the SVD run in fp64 (one-sided Jacobi), results rounded to fp32.
// A zero covariance (all weights under the threshold) gives U = V = I -> R = I,
// which is what torch.svd returns for the zero matrix.
#include "common.h"
#include "procrustes.h"

namespace fgr {
namespace {

// Generic accessor-driven solver: point i of problem p -> (a, b, w).
template <class Get>
__device__ void solve(int64_t n, float threshold, Get get, float* out) {
    __shared__ double sh[(kPoseThreads / 64) * 16];
    double s[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int64_t i = threadIdx.x; i < n; i += kPoseThreads) {
        float a[3], b[3], w;
        get(i, a, b, w);
        if (threshold >= 0.f && !(w > threshold)) w = 0.f;
        s[0] += w;
        for (int d = 0; d < 3; ++d) { s[1 + d] += (double)w * a[d]; s[4 + d] += (double)w * b[d]; }
    }
    block_reduce(s, 7, sh);
    const double W = fmax(s[0], 1e-6);
    double ca[3], cb[3];
    for (int d = 0; d < 3; ++d) { ca[d] = s[1 + d] / W; cb[d] = s[4 + d] / W; }
    double h[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int64_t i = threadIdx.x; i < n; i += kPoseThreads) {
        float a[3], b[3], w;
        get(i, a, b, w);
        if (threshold >= 0.f && !(w > threshold)) w = 0.f;
        const double wn = (double)w / W;
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) h[3 * r + c] += (a[r] - ca[r]) * ((b[c] - cb[c]) * wn);
    }
    block_reduce(h, 9, sh);
    if (threadIdx.x == 0) {
        double H[3][3], R[3][3];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) H[r][c] = h[3 * r + c];
        svd3_rotation(H, R);
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) out[4 * r + c] = (float)R[r][c];
            out[4 * r + 3] = (float)(-(R[r][0] * ca[0] + R[r][1] * ca[1] + R[r][2] * ca[2]) + cb[r]);
        }
    }
}

__global__ void __launch_bounds__(kPoseThreads)
procrustes_kernel(const float* __restrict__ a, const float* __restrict__ b,
                  const float* __restrict__ w, int64_t n_pts, float threshold,
                  float* __restrict__ out) {
    const int64_t p = blockIdx.x;
    const float* ap = a + p * n_pts * 3;
    const float* bp = b + p * n_pts * 3;
    const float* wp = w + p * n_pts;
    solve(n_pts, threshold,
          [&](int64_t i, float* av, float* bv, float& wv) {
              for (int d = 0; d < 3; ++d) { av[d] = ap[3 * i + d]; bv[d] = bp[3 * i + d]; }
              wv = wp[i];
          },
          out + p * 12);
}

__device__ __forceinline__ float sigmoidf(float x) { return 1.0f / (1.0f + expf(-x)); }

// grid = (n_pairs, n_layers)
__global__ void __launch_bounds__(kPoseThreads)
pair_pose_kernel(const float* __restrict__ xyz, const float* __restrict__ corr,
                 const float* __restrict__ logits, int64_t n_tot,
                 const int64_t* __restrict__ seg_off, int n_pairs, float threshold,
                 float* __restrict__ out) {
    const int pr = blockIdx.x, l = blockIdx.y;
    const int64_t sb = seg_off[pr], se = seg_off[pr + 1];
    const int64_t tb = seg_off[n_pairs + pr], te = seg_off[n_pairs + pr + 1];
    const int64_t ns = se - sb, nt = te - tb;
    const float* cl = corr + (int64_t)l * n_tot * 3;
    const float* lg = logits + (int64_t)l * n_tot;
    solve(ns + nt, threshold,
          [&](int64_t i, float* av, float* bv, float& wv) {
              if (i < ns) {            // [src_xyz | src_corr]
                  const int64_t r = sb + i;
                  for (int d = 0; d < 3; ++d) { av[d] = xyz[3 * r + d]; bv[d] = cl[3 * r + d]; }
                  wv = sigmoidf(lg[r]);
              } else {                 // [tgt_corr | tgt_xyz]
                  const int64_t r = tb + (i - ns);
                  for (int d = 0; d < 3; ++d) { av[d] = cl[3 * r + d]; bv[d] = xyz[3 * r + d]; }
                  wv = sigmoidf(lg[r]);
              }
          },
          out + ((int64_t)l * n_pairs + pr) * 12);
}

}  // namespace
}  // namespace fgr

using namespace fgr;

extern "C" int fgr_procrustes(const float* a, const float* b, const float* w, int64_t n_batch,
                              int64_t n_pts, float threshold, float* out, void* stream) {
    FGR_REQUIRE(n_batch >= 0 && n_pts >= 0, "fgr_procrustes: bad arguments");
    FGR_REQUIRE(n_batch == 0 || (a && b && w && out), "fgr_procrustes: null pointer");
    if (n_batch == 0) return FGR_OK;
    hipLaunchKernelGGL(procrustes_kernel, dim3((unsigned)n_batch), dim3(kPoseThreads), 0,
                       as_stream(stream), a, b, w, n_pts, threshold, out);
    FGR_CHECK_LAUNCH("procrustes_kernel");
    return FGR_OK;
}

extern "C" int fgr_pair_pose(const float* xyz, const float* corr, const float* logits,
                             int64_t n_tot, const int64_t* seg_off, int32_t n_pairs,
                             int32_t n_layers, float threshold, float* out, void* stream) {
    FGR_REQUIRE(n_pairs > 0 && n_layers > 0 && n_tot >= 0 && seg_off && xyz && corr && logits &&
                    out,
                "fgr_pair_pose: bad arguments");
    TimedCall timed_(as_stream(stream));
    hipLaunchKernelGGL(pair_pose_kernel, dim3((unsigned)n_pairs, (unsigned)n_layers),
                       dim3(kPoseThreads), 0, as_stream(stream), xyz, corr, logits, n_tot,
                       seg_off, n_pairs, threshold, out);
    FGR_CHECK_LAUNCH("pair_pose_kernel");
    return FGR_OK;
}
