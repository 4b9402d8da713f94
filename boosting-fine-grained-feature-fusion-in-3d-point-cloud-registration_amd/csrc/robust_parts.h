// The parts the two robust pose estimators share: ransac.hip (fgr_ransac_pose, uniform 3-point
// samples) and compat.hip (fgr_compat_pose, seeds from spatial compatibility) differ only in
// where their hypotheses come from. Both compact the eligible rows the same way, score a pose by
// the same fp32 count, leave one RsSlot per group of hypotheses, and hand the slots to the same
// select + refit kernel. Internal linkage, as procrustes.h: each translation unit that includes
// this header compiles its own copy, and both are built with -ffp-contract=off (the transform
// and d2 round as written). The two kernels below therefore exist twice in the library under one
// name: in a profiler trace a ransac_prep_kernel / ransac_select_kernel that follows
// ransac_score_kernel is fgr_ransac_pose's, one around the compat_* kernels is fgr_compat_pose's
// (its prep also takes the idx pointer).
//
// * ransac_prep_kernel, one block per pair: the eligible rows (w > w_min, strict) are compacted
//   in row order into the workspace by a ballot / prefix scan, eight floats a row
//   (ax ay az bx | by bz 0 0), and their number m goes to n_eligible, which the later launches
//   read. With `idx` it also records each rank's row index within its pair.
// * ransac_select_kernel, one block per pair: reduces the slots (largest count, then lowest h),
//   runs the refit loop -- fp64 moments of the inliers, per-thread in row order then
//   block_reduce's fixed tree, no floating-point atomics; the solve on thread 0 -- and writes
//   the outputs under the final pose from the caller's rows.
#pragma once
#include "common.h"
#include "procrustes.h"

namespace fgr {
namespace {

constexpr int kRsThreads = kPoseThreads;           // block_reduce's block

struct RsSlot {                                    // the best hypothesis of a group, 64 bytes
    int32_t count, h;                              // -1, -1: no valid hypothesis in the group
    float T[12];
    int32_t pad[2];
};

size_t rs_align(size_t x) { return (x + 255) & ~size_t(255); }

// (count, h) -> a key whose maximum is the largest count, then the lowest h (h < 2^20)
__device__ __forceinline__ long long rs_key(int count, int h) {
    return ((long long)count << 32) | (long long)(0x7fffffff - h);
}

// d2 of row (a, b) under T: ((R0 x + R1 y) + R2 z) + t, then ((dx dx) + dy dy) + dz dz
__device__ __forceinline__ float rs_d2(const float* T, float ax, float ay, float az, float bx,
                                       float by, float bz) {
    const float dx = (((T[0] * ax + T[1] * ay) + T[2] * az) + T[3]) - bx;
    const float dy = (((T[4] * ax + T[5] * ay) + T[6] * az) + T[7]) - by;
    const float dz = (((T[8] * ax + T[9] * ay) + T[10] * az) + T[11]) - bz;
    return (dx * dx + dy * dy) + dz * dz;
}

// T <- [R | bm - R am] rounded to fp32, R the rotation of the covariance H = sum (a - am)(b - bm)^T
__device__ void rs_pose(const double H[3][3], const double* am, const double* bm, float* T) {
    double R[3][3];
    svd3_rotation(H, R);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) T[4 * r + c] = (float)R[r][c];
        T[4 * r + 3] = (float)(bm[r] - (R[r][0] * am[0] + R[r][1] * am[1] + R[r][2] * am[2]));
    }
}

__device__ __forceinline__ void rs_identity(float* T) {
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = (k % 5 == 0) ? 1.f : 0.f;
}

// The fp64 Kabsch moments of a set of rows, 16 doubles: n, sum a, sum b, sum a b^T
__device__ __forceinline__ void rs_moments_add(double* v, const float4 u, const float4 q) {
    const double pa[3] = {u.x, u.y, u.z}, pb[3] = {u.w, q.x, q.y};
    v[0] += 1.0;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        v[1 + r] += pa[r];
        v[4 + r] += pb[r];
#pragma unroll
        for (int cc = 0; cc < 3; ++cc) v[7 + 3 * r + cc] += pa[r] * pb[cc];
    }
}

// the pose of reduced moments: H = sum a b^T - (sum a)(sum b)^T / n
__device__ void rs_moments_pose(const double* v, float* T) {
    const double n = v[0];
    double H[3][3], am[3], bm[3];
    for (int r = 0; r < 3; ++r) {
        am[r] = v[1 + r] / n;
        bm[r] = v[4 + r] / n;
    }
    for (int r = 0; r < 3; ++r)
        for (int cc = 0; cc < 3; ++cc) H[r][cc] = v[7 + 3 * r + cc] - v[1 + r] * v[4 + cc] / n;
    rs_pose(H, am, bm, T);
}

__global__ void __launch_bounds__(kRsThreads)
ransac_prep_kernel(const float* __restrict__ a, const float* __restrict__ b,
                   const float* __restrict__ w, const int64_t* __restrict__ off, float w_min,
                   float4* __restrict__ rows, int32_t* __restrict__ n_eligible,
                   int32_t* __restrict__ idx) {
    __shared__ int wave_cnt[kRsThreads / 64];
    const int p = blockIdx.x;
    const int64_t beg = off[p], end = off[p + 1];
    const int lane = threadIdx.x % 64, wv = threadIdx.x / 64;
    int64_t base = 0;                                      // eligible rows before this chunk
    for (int64_t c0 = beg; c0 < end; c0 += kRsThreads) {   // block-uniform
        const int64_t i = c0 + threadIdx.x;
        const bool el = i < end && (!w || w[i] > w_min);   // a NaN weight is not eligible
        const unsigned long long bal = __ballot(el);
        const int before = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wave_cnt[wv] = __popcll(bal);
        __syncthreads();
        int wbase = 0, tot = 0;
#pragma unroll
        for (int k = 0; k < kRsThreads / 64; ++k) {
            const int c = wave_cnt[k];
            if (k < wv) wbase += c;
            tot += c;
        }
        if (el) {
            const int64_t r = beg + base + wbase + before;   // <= i: inside the pair's rows
            rows[2 * r] = make_float4(a[3 * i], a[3 * i + 1], a[3 * i + 2], b[3 * i]);
            rows[2 * r + 1] = make_float4(b[3 * i + 1], b[3 * i + 2], 0.f, 0.f);
            if (idx) idx[r] = (int32_t)(i - beg);
        }
        base += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) n_eligible[p] = (int32_t)base;
}

// the number of compacted rows with d2 < r2 under T, in every thread
__device__ int rs_count(const float* T, const float4* __restrict__ R0, int m, float r2,
                        double* sh) {
    double c = 0.0;
    for (int64_t i = threadIdx.x; i < m; i += kRsThreads) {
        const float4 u = R0[2 * i], v = R0[2 * i + 1];
        if (rs_d2(T, u.x, u.y, u.z, u.w, v.x, v.y) < r2) c += 1.0;
    }
    block_reduce(&c, 1, sh);
    return (int)c;
}

__global__ void __launch_bounds__(kRsThreads)
ransac_select_kernel(const float* __restrict__ a, const float* __restrict__ b,
                     const float* __restrict__ w, const int64_t* __restrict__ off,
                     const float4* __restrict__ rows, const int32_t* __restrict__ n_eligible,
                     const RsSlot* __restrict__ slots, int n_blk, float w_min, float r2,
                     int n_refits, float* __restrict__ pose, int32_t* __restrict__ n_inliers,
                     float* __restrict__ inlier_rmse, int32_t* __restrict__ best_hyp,
                     int32_t* __restrict__ n_updates, uint8_t* __restrict__ inlier_mask) {
    __shared__ double sh[(kRsThreads / 64) * 16];
    __shared__ long long wbest[kRsThreads / 64];
    __shared__ int win;
    __shared__ float Ts[12], Tn[12];
    const int p = blockIdx.x;
    const int64_t beg = off[p], end = off[p + 1];
    const int m = n_eligible[p];
    const float4* R0 = rows + 2 * beg;
    const RsSlot* S = slots + (int64_t)p * n_blk;
    // the best slot: largest count, then lowest h
    long long mine = -1;
    int mine_s = -1;
    for (int s = threadIdx.x; s < n_blk; s += kRsThreads) {
        const int c = S[s].count;
        const long long k = c >= 0 ? rs_key(c, S[s].h) : -1ll;
        if (k > mine) { mine = k; mine_s = s; }
    }
    long long best = mine;
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
    if (best < 0) {                                        // block-uniform: no valid hypothesis
        if (threadIdx.x < 12) pose[12 * p + threadIdx.x] = (threadIdx.x % 5 == 0) ? 1.f : 0.f;
        if (threadIdx.x == 0) {
            n_inliers[p] = 0;
            inlier_rmse[p] = 0.f;
            best_hyp[p] = -1;
            n_updates[p] = 0;
        }
        if (inlier_mask)
            for (int64_t i = beg + threadIdx.x; i < end; i += kRsThreads) inlier_mask[i] = 0;
        return;
    }
    if (mine == best) win = mine_s;                        // one thread: h is part of the key
    __syncthreads();
    if (threadIdx.x < 12) Ts[threadIdx.x] = S[win].T[threadIdx.x];
    int c = S[win].count, upd = 0;
    __syncthreads();
    for (int it = 0; it < n_refits; ++it) {                // every exit is block-uniform
        double v[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) v[k] = 0.0;
        for (int64_t i = threadIdx.x; i < m; i += kRsThreads) {
            const float4 u = R0[2 * i], q = R0[2 * i + 1];
            if (rs_d2(Ts, u.x, u.y, u.z, u.w, q.x, q.y) < r2) rs_moments_add(v, u, q);
        }
        block_reduce(v, 16, sh);
        if (v[0] < 3.0) break;
        if (threadIdx.x == 0) {
            float T[12];
            rs_moments_pose(v, T);
#pragma unroll
            for (int k = 0; k < 12; ++k) Tn[k] = T[k];
        }
        __syncthreads();
        const int c2 = rs_count(Tn, R0, m, r2, sh);        // ends with a barrier
        if (c2 < c) break;
        if (threadIdx.x < 12) Ts[threadIdx.x] = Tn[threadIdx.x];
        __syncthreads();
        ++upd;
        if (c2 == c) break;
        c = c2;
    }
    // the outputs under the final pose, from the caller's rows
    double v[2] = {0.0, 0.0};
    for (int64_t i = beg + threadIdx.x; i < end; i += kRsThreads) {
        bool inl = false;
        if (!w || w[i] > w_min) {
            const float d2 = rs_d2(Ts, a[3 * i], a[3 * i + 1], a[3 * i + 2], b[3 * i],
                                   b[3 * i + 1], b[3 * i + 2]);
            inl = d2 < r2;
            if (inl) { v[0] += 1.0; v[1] += (double)d2; }
        }
        if (inlier_mask) inlier_mask[i] = inl ? 1 : 0;
    }
    block_reduce(v, 2, sh);
    if (threadIdx.x < 12) pose[12 * p + threadIdx.x] = Ts[threadIdx.x];
    if (threadIdx.x == 0) {
        n_inliers[p] = (int32_t)v[0];
        inlier_rmse[p] = v[0] > 0.0 ? (float)sqrt(v[1] / v[0]) : 0.f;
        best_hyp[p] = S[win].h;
        n_updates[p] = upd;
    }
}

}  // namespace
}  // namespace fgr
