// RANSAC pose estimation from putative correspondences, resident on the device: the robust
// estimator between the forward's correspondences and fgr_icp. include/fgreg.h states the
// semantics; tests/_ransac_ref.py restates them in numpy.
//
// * ransac_prep_kernel (robust_parts.h), one block per pair: compacts the eligible rows into
//   the workspace and counts them into n_eligible, which the later launches read.
// * ransac_score_kernel, grid (hypothesis chunk, pair): ONE LANE OWNS ONE HYPOTHESIS. It draws
//   its three ranks from the counter-based hash of common.h (nothing stored, any geometry
//   draws the same), solves the 3-point Kabsch in fp64 (procrustes.h's Jacobi SVD), rounds the
//   pose once to fp32 and keeps those 12 floats in registers. The pair's compacted rows are
//   staged through LDS kRsTile at a time; in the counting loop every lane reads the same LDS
//   address (a broadcast, no bank conflict) and tests d2 < r2 under its own pose. The block's
//   best (count, lowest h) and that lane's pose go to the block's slot of the workspace.
// * ransac_select_kernel (robust_parts.h), one block per pair: reduces the slots, runs the
//   refit loop and writes the outputs under the final pose from the caller's rows.
// Nothing is read back and every launch is unconditional: a call can be captured into a graph.
// Built with -ffp-contract=off (see geom.hip): the transform and d2 round as written.
#include <cfloat>

#include "robust_parts.h"

namespace fgr {
namespace {

constexpr int kRsTile = 256;                       // compacted rows per LDS tile
constexpr int kMaxHyp = 1 << 20;
static_assert(kRsTile == kRsThreads, "a thread stages one row of a tile; hypotheses per block");

int rs_blocks(int32_t n_hyp) { return (n_hyp + kRsThreads - 1) / kRsThreads; }

__global__ void __launch_bounds__(kRsThreads)
ransac_score_kernel(const float4* __restrict__ rows, const int64_t* __restrict__ off,
                    const int32_t* __restrict__ n_eligible, int n_hyp, uint32_t seed, float r2,
                    RsSlot* __restrict__ slots, float* __restrict__ hyp_pose,
                    int32_t* __restrict__ hyp_count) {
    __shared__ float4 tile[2 * kRsTile];
    __shared__ long long wbest[kRsThreads / 64];
    const int p = blockIdx.y;
    const int h = blockIdx.x * kRsThreads + threadIdx.x;
    const int m = n_eligible[p];
    const float4* R0 = rows + 2 * off[p];
    float T[12];
    rs_identity(T);
    bool valid = false;
    if (h < n_hyp && m >= 3) {
        uint32_t rk[3];
#pragma unroll
        for (int k = 0; k < 3; ++k)
            rk[k] = (uint32_t)(((uint64_t)attn_drop_hash(seed, k, p, h) * (uint64_t)m) >> 32);
        valid = rk[0] != rk[1] && rk[0] != rk[2] && rk[1] != rk[2];
        if (valid) {
            double A[3][3], B[3][3], am[3], bm[3], H[3][3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float4 u = R0[2 * (int64_t)rk[k]], v = R0[2 * (int64_t)rk[k] + 1];
                A[k][0] = u.x; A[k][1] = u.y; A[k][2] = u.z;
                B[k][0] = u.w; B[k][1] = v.x; B[k][2] = v.y;
            }
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                am[r] = ((A[0][r] + A[1][r]) + A[2][r]) / 3.0;
                bm[r] = ((B[0][r] + B[1][r]) + B[2][r]) / 3.0;
            }
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    H[r][c] = ((A[0][r] - am[r]) * (B[0][c] - bm[c]) +
                               (A[1][r] - am[r]) * (B[1][c] - bm[c])) +
                              (A[2][r] - am[r]) * (B[2][c] - bm[c]);
            rs_pose(H, am, bm, T);
        }
    }
    int cnt = 0;
    if (m >= 3) {                                          // block-uniform
        for (int64_t t0 = 0; t0 < m; t0 += kRsTile) {          // 64-bit: m may be near 2^31
            const int n = (int)min((int64_t)kRsTile, m - t0);
            __syncthreads();                               // the previous tile has been read
            if ((int)threadIdx.x < n) {
                tile[2 * threadIdx.x] = R0[2 * (t0 + threadIdx.x)];
                tile[2 * threadIdx.x + 1] = R0[2 * (t0 + threadIdx.x) + 1];
            }
            __syncthreads();
#pragma unroll 4
            for (int j = 0; j < n; ++j) {
                const float4 u = tile[2 * j], v = tile[2 * j + 1];   // one address: a broadcast
                cnt += rs_d2(T, u.x, u.y, u.z, u.w, v.x, v.y) < r2 ? 1 : 0;
            }
        }
    }
    if (!valid) cnt = -1;
    if (h < n_hyp) {
        const int64_t o = (int64_t)p * n_hyp + h;
        if (hyp_count) hyp_count[o] = cnt;
        if (hyp_pose) {
#pragma unroll
            for (int k = 0; k < 12; ++k) hyp_pose[12 * o + k] = T[k];
        }
    }
    const long long key = valid ? rs_key(cnt, h) : -1ll;
    long long best = key;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const long long other = __shfl_xor(best, o, 64);
        best = other > best ? other : best;
    }
    if (threadIdx.x % 64 == 0) wbest[threadIdx.x / 64] = best;
    __syncthreads();
    best = wbest[0];
#pragma unroll
    for (int k = 1; k < kRsThreads / 64; ++k) best = wbest[k] > best ? wbest[k] : best;
    RsSlot* s = slots + (int64_t)p * gridDim.x + blockIdx.x;
    if (best < 0) {
        if (threadIdx.x == 0) { s->count = -1; s->h = -1; }
    } else if (key == best) {                              // one lane: h is part of the key
        s->count = cnt;
        s->h = h;
#pragma unroll
        for (int k = 0; k < 12; ++k) s->T[k] = T[k];
    }
}

struct RsWs {
    float4* rows;
    RsSlot* slots;
    size_t total;
};

void carve_ransac(void* ws, int64_t n_tot, int32_t n_pairs, int32_t n_hyp, RsWs* w) {
    char* p = static_cast<char*>(ws);
    size_t o = 0;
    auto take = [&](size_t bytes) { void* r = p ? p + o : nullptr; o += rs_align(bytes); return r; };
    w->rows = (float4*)take(sizeof(float4) * 2 * (size_t)n_tot);
    w->slots = (RsSlot*)take(sizeof(RsSlot) * (size_t)n_pairs * rs_blocks(n_hyp));
    w->total = o;
}

bool ransac_sizes_ok(int64_t n_tot, int32_t n_pairs, int32_t n_hyp) {
    return n_pairs >= 1 && n_pairs <= 65535 && n_hyp >= 1 && n_hyp <= kMaxHyp && n_tot >= 0 &&
           n_tot < (1ll << 31);
}

}  // namespace
}  // namespace fgr

using namespace fgr;

extern "C" int fgr_ransac_workspace(int64_t n_tot, int32_t n_pairs, int32_t n_hyp, size_t* bytes) {
    FGR_REQUIRE(bytes && ransac_sizes_ok(n_tot, n_pairs, n_hyp),
                "fgr_ransac_workspace: bad arguments (n_tot %lld n_pairs %d n_hyp %d)",
                (long long)n_tot, n_pairs, n_hyp);
    RsWs w;
    carve_ransac(nullptr, n_tot, n_pairs, n_hyp, &w);
    *bytes = w.total;
    return FGR_OK;
}

extern "C" int fgr_ransac_pose(const float* a, const float* b, const float* w, int64_t n_tot,
                               const int64_t* off, int32_t n_pairs, float w_min, float inlier_dist,
                               int32_t n_hyp, uint32_t seed, int32_t n_refits, void* ws,
                               size_t ws_bytes, float* pose, int32_t* n_inliers,
                               float* inlier_rmse, int32_t* n_eligible, int32_t* best_hyp,
                               int32_t* n_updates, uint8_t* inlier_mask, float* hyp_pose,
                               int32_t* hyp_count, void* stream) {
    FGR_REQUIRE(ransac_sizes_ok(n_tot, n_pairs, n_hyp) && n_refits >= 0 && inlier_dist > 0.f &&
                    inlier_dist <= FLT_MAX && off && ws &&
                    (reinterpret_cast<uintptr_t>(ws) & 15) == 0 && pose && n_inliers && inlier_rmse &&
                    n_eligible && best_hyp && n_updates && ((a && b) || n_tot == 0),
                "fgr_ransac_pose: bad arguments (n_tot %lld n_pairs %d n_hyp %d n_refits %d "
                "inlier_dist %g)",
                (long long)n_tot, n_pairs, n_hyp, n_refits, (double)inlier_dist);
    RsWs s;
    carve_ransac(ws, n_tot, n_pairs, n_hyp, &s);
    FGR_REQUIRE(s.total <= ws_bytes, "fgr_ransac_pose: workspace %zu < %zu bytes", ws_bytes,
                s.total);
    hipStream_t st = as_stream(stream);
    TimedCall timed_(st);
    const int n_blk = rs_blocks(n_hyp);
    const float r2 = inlier_dist * inlier_dist;
    hipLaunchKernelGGL(ransac_prep_kernel, dim3((unsigned)n_pairs), dim3(kRsThreads), 0, st, a, b,
                       w, off, w_min, s.rows, n_eligible, (int32_t*)nullptr);
    FGR_CHECK_LAUNCH("ransac_prep_kernel");
    hipLaunchKernelGGL(ransac_score_kernel, dim3((unsigned)n_blk, (unsigned)n_pairs),
                       dim3(kRsThreads), 0, st, s.rows, off, n_eligible, n_hyp, seed, r2, s.slots,
                       hyp_pose, hyp_count);
    FGR_CHECK_LAUNCH("ransac_score_kernel");
    hipLaunchKernelGGL(ransac_select_kernel, dim3((unsigned)n_pairs), dim3(kRsThreads), 0, st, a,
                       b, w, off, s.rows, n_eligible, s.slots, n_blk, w_min, r2, n_refits, pose,
                       n_inliers, inlier_rmse, best_hyp, n_updates, inlier_mask);
    FGR_CHECK_LAUNCH("ransac_select_kernel");
    return FGR_OK;
}
