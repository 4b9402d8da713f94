// GPU-resident 3DMatch / MCD training augmentations: data_loaders/transforms.py as
// data_loaders/__init__.py:16-57 chains them in front of every training sample,
//   RigidPerturb :15-72 -> Jitter :75-92 -> ShufflePoints :95-131 -> RandomSwap :134-151.
// The random draws stay on the host in the reference's three global streams
// (fgreg/augment.py); the kernels do the geometry and the index bookkeeping. Where the
// reference rounds to float32 after every step, these evaluate each output once in float64
// and round once (fgreg.augment.train_augment_host is the same chain in NumPy float64; the
// two differ by the centroid's summation order only, i.e. by a final rounding at most).
// Three launches, no host sync between them:
//   augment_pose_kernel     one block per pair: centroid of the perturbed cloud (float64,
//                           fixed tree order, no atomics), C^-1 P C, the new pose, the swap's
//                           inverse; the two per-cloud 3x4 transforms go to the workspace;
//                           the pair's part of the inverse map is set to -1
//   augment_gather_kernel   grid over 256-row output tiles of every cloud: T raw[perm[i]] +
//                           noise[perm[i]], the overlap byte, inverse map raw row -> output row
//   augment_corr_kernel     one block per pair: order-preserving compaction of the columns
//                           whose two points both survived ShufflePoints' truncation
// There is no per-cloud point cap: nothing is tiled by the cloud, sizes only fit int32.
#include "common.h"

#pragma clang fp contract(off)

namespace fgr {
namespace {

constexpr int kPoseThreads = 1024;
constexpr int kTileRows = 256;        // gather: output rows per tile = threads per block
constexpr int kCorrThreads = 1024;    // correspondence columns per scan chunk

// flags[b] bits
constexpr int kPerturb = FGR_AUG_PERTURB, kSource = FGR_AUG_SOURCE, kCentre = FGR_AUG_CENTRE,
              kSwap = FGR_AUG_SWAP;

struct Se3 {
    double r[9], t[3];
};

__device__ __forceinline__ Se3 se3_identity() {
    Se3 o;
#pragma unroll
    for (int i = 0; i < 9; ++i) o.r[i] = (i % 4 == 0) ? 1.0 : 0.0;
    o.t[0] = o.t[1] = o.t[2] = 0.0;
    return o;
}

__device__ __forceinline__ Se3 se3_load(const float* p) {
    Se3 o;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) o.r[i * 3 + j] = (double)p[i * 4 + j];
        o.t[i] = (double)p[i * 4 + 3];
    }
    return o;
}

// a . b (se3_cat, utils/se3_torch.py:32-40)
__device__ __forceinline__ Se3 se3_cat(const Se3& a, const Se3& b) {
    Se3 o;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j)
            o.r[i * 3 + j] = (a.r[i * 3] * b.r[j] + a.r[i * 3 + 1] * b.r[3 + j]) +
                             a.r[i * 3 + 2] * b.r[6 + j];
        o.t[i] = ((a.r[i * 3] * b.t[0] + a.r[i * 3 + 1] * b.t[1]) + a.r[i * 3 + 2] * b.t[2]) +
                 a.t[i];
    }
    return o;
}

// (R^T | -R^T t) (se3_inv, :43-48): the transpose, as the reference inverts
__device__ __forceinline__ Se3 se3_inv(const Se3& a) {
    Se3 o;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) o.r[i * 3 + j] = a.r[j * 3 + i];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
        o.t[i] = -((o.r[i * 3] * a.t[0] + o.r[i * 3 + 1] * a.t[1]) + o.r[i * 3 + 2] * a.t[2]);
    return o;
}

__device__ __forceinline__ void se3_store(const Se3& a, double* p) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) p[i * 4 + j] = a.r[i * 3 + j];
        p[i * 4 + 3] = a.t[i];
    }
}

// One block per pair. in_off: (2B + 1) row offsets of the packed input clouds (source of
// pair b, then its target).
__global__ void __launch_bounds__(kPoseThreads)
augment_pose_kernel(const float* __restrict__ xyz, int ld, const int64_t* __restrict__ in_off,
                    const float* __restrict__ pose, const float* __restrict__ perturb,
                    const int32_t* __restrict__ flags, float* __restrict__ pose_out,
                    double* __restrict__ tf, int32_t* __restrict__ inv) {
    __shared__ double red[3][kPoseThreads];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int fl = flags[b];
    const int64_t o0 = in_off[2 * b], o2 = in_off[2 * b + 2];
    for (int64_t i = o0 + tid; i < o2; i += kPoseThreads) inv[i] = -1;

    double cen[3] = {0.0, 0.0, 0.0};
    if ((fl & kPerturb) && (fl & kCentre)) {        // uniform over the block
        const int c = (fl & kSource) ? 0 : 1;
        const int64_t o = in_off[2 * b + c], n = in_off[2 * b + c + 1] - o;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;        // rows tid, tid + 1024, ... in order
        for (int64_t i = tid; i < n; i += kPoseThreads) {
            const float* p = xyz + (o + i) * ld;
            s0 += (double)p[0];
            s1 += (double)p[1];
            s2 += (double)p[2];
        }
        red[0][tid] = s0;
        red[1][tid] = s1;
        red[2][tid] = s2;
        __syncthreads();
        for (int h = kPoseThreads / 2; h > 0; h >>= 1) {    // fixed tree: run-to-run identical
            if (tid < h) {
                red[0][tid] += red[0][tid + h];
                red[1][tid] += red[1][tid + h];
                red[2][tid] += red[2][tid + h];
            }
            __syncthreads();
        }
        const double dn = (double)(n > 0 ? n : 1);
        cen[0] = red[0][0] / dn;
        cen[1] = red[1][0] / dn;
        cen[2] = red[2][0] / dn;
    }
    if (tid != 0) return;

    Se3 ps = se3_load(pose + b * 12);
    Se3 ts = se3_identity(), tt = se3_identity();
    if (fl & kPerturb) {
        Se3 p = se3_load(perturb + b * 12);
        if (fl & kCentre) {
            // C^-1 . P . C with C = (I | -centroid): the rotation stays, t' = (R (-c) + t) + c
            Se3 cm = se3_identity(), ci = se3_identity();
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                cm.t[i] = -cen[i];
                ci.t[i] = cen[i];
            }
            p = se3_cat(se3_cat(ci, p), cm);
        }
        if (fl & kSource) {
            ps = se3_cat(ps, se3_inv(p));
            ts = p;
        } else {
            ps = se3_cat(p, ps);
            tt = p;
        }
    }
    if (fl & kSwap) ps = se3_inv(ps);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) pose_out[b * 12 + i * 4 + j] = (float)ps.r[i * 3 + j];
        pose_out[b * 12 + i * 4 + 3] = (float)ps.t[i];
    }
    se3_store(ts, tf + (int64_t)(2 * b) * 12);
    se3_store(tt, tf + (int64_t)(2 * b + 1) * 12);
}

// blockIdx.y = input cloud c (2b: source, 2b + 1: target), blockIdx.x strides over its
// 256-row output tiles. perm / out_off are in input-cloud order; the cloud's rows land at the
// other cloud's place when the pair is swapped (outputs are post-swap).
__global__ void __launch_bounds__(kTileRows)
augment_gather_kernel(const float* __restrict__ xyz, int ld, const int64_t* __restrict__ in_off,
                      const uint8_t* __restrict__ overlap, const int32_t* __restrict__ perm,
                      const int64_t* __restrict__ out_off, const float* __restrict__ noise,
                      const int32_t* __restrict__ flags, const double* __restrict__ tf,
                      float* __restrict__ xyz_out, uint8_t* __restrict__ overlap_out,
                      int32_t* __restrict__ inv) {
    __shared__ float tile[kTileRows * 3];
    const int c = blockIdx.y, b = c >> 1, tid = threadIdx.x;
    const int64_t io = in_off[c], n = in_off[c + 1] - io;
    const int64_t po = out_off[c], m = out_off[c + 1] - po;
    int64_t dst = po;
    if (flags[b] & kSwap) {
        const int64_t base = out_off[2 * b];     // the target's rows first, then the source's
        dst = (c & 1) ? base : base + (out_off[2 * b + 2] - out_off[2 * b + 1]);
    }
    double t[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) t[e] = tf[(int64_t)c * 12 + e];

    for (int64_t r0 = (int64_t)blockIdx.x * kTileRows; r0 < m; r0 += (int64_t)gridDim.x * kTileRows) {
        const int64_t i = r0 + tid;
        if (i < m) {
            const int64_t p = (int64_t)perm[po + i];
            float v[3] = {0.f, 0.f, 0.f};
            uint8_t ovb = 0;
            if ((uint64_t)p < (uint64_t)n) {        // the host validates; never index past the cloud
                const float* q = xyz + (io + p) * ld;
                const double x = (double)q[0], y = (double)q[1], z = (double)q[2];
                double nz[3] = {0.0, 0.0, 0.0};
                if (noise) {
                    const float* nq = noise + (io + p) * 3;
                    nz[0] = (double)nq[0], nz[1] = (double)nq[1], nz[2] = (double)nq[2];
                }
#pragma unroll
                for (int e = 0; e < 3; ++e)
                    v[e] = (float)(((((t[e * 4] * x + t[e * 4 + 1] * y) + t[e * 4 + 2] * z)) +
                                    t[e * 4 + 3]) + nz[e]);
                ovb = overlap[io + p];
                inv[io + p] = (int32_t)i;
            }
            tile[tid * 3] = v[0];
            tile[tid * 3 + 1] = v[1];
            tile[tid * 3 + 2] = v[2];
            overlap_out[dst + i] = ovb;
        }
        __syncthreads();
        // the tile's rows are contiguous in the output: dword-coalesced stores
        const int64_t rows = m - r0 < kTileRows ? m - r0 : kTileRows;
        float* o = xyz_out + (dst + r0) * 3;
        for (int j = tid; j < rows * 3; j += kTileRows) o[j] = tile[j];
        __syncthreads();
    }
}

// Exclusive block scan of one flag per thread (crop.hip's block_scan at this block size).
__device__ __forceinline__ int corr_scan(int flag, int* sh, int* total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint64_t bal = __ballot(flag);
    const int pre = __popcll(bal & ((lane ? (~0ull >> (64 - lane)) : 0ull)));
    if (lane == 0) sh[wv] = __popcll(bal);
    __syncthreads();
    int base = 0, tot = 0;
    for (int w = 0; w < kCorrThreads / 64; ++w) {
        const int cnt = sh[w];
        base += w < wv ? cnt : 0;
        tot += cnt;
    }
    __syncthreads();
    *total = tot;
    return base + pre;
}

// One block per pair; corr / corr_out are (2, corr_ld) with pair b's columns at
// [corr_off[b], corr_off[b + 1]).
__global__ void __launch_bounds__(kCorrThreads)
augment_corr_kernel(const int64_t* __restrict__ corr, int64_t corr_ld,
                    const int64_t* __restrict__ corr_off, const int64_t* __restrict__ in_off,
                    const int32_t* __restrict__ flags, const int32_t* __restrict__ inv,
                    int64_t* __restrict__ corr_out, int32_t* __restrict__ n_corr) {
    __shared__ int sh[kCorrThreads / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int64_t co = corr_off[b], nc = corr_off[b + 1] - co;
    const int64_t so = in_off[2 * b], to = in_off[2 * b + 1];
    const int64_t ns = to - so, nt = in_off[2 * b + 2] - to;
    const bool swap = flags[b] & kSwap;
    int base = 0, bad = 0;
    for (int64_t j0 = 0; j0 < nc; j0 += kCorrThreads) {
        const int64_t j = j0 + tid;
        int a = -1, q = -1;
        if (j < nc) {
            const int64_t s = corr[co + j], r = corr[corr_ld + co + j];
            if ((uint64_t)s < (uint64_t)ns && (uint64_t)r < (uint64_t)nt) {
                a = inv[so + s];
                q = inv[to + r];
            } else {
                bad = 1;                    // never dereferenced: the pair is reported instead
            }
        }
        const int f = a >= 0 && q >= 0;
        int tot;
        const int pos = corr_scan(f, sh, &tot);
        if (f) {
            corr_out[co + base + pos] = swap ? q : a;
            corr_out[corr_ld + co + base + pos] = swap ? a : q;
        }
        base += tot;
    }
    bad = __syncthreads_or(bad);
    if (tid == 0) n_corr[b] = bad ? -1 : base;
}

inline size_t tf_bytes(int32_t n_pairs) { return (size_t)n_pairs * 2 * 12 * sizeof(double); }

}  // namespace
}  // namespace fgr

using namespace fgr;

extern "C" int fgr_augment_workspace_bytes(int64_t n_points, int32_t n_pairs, size_t* bytes) {
    FGR_REQUIRE(bytes && n_points >= 0 && n_pairs > 0, "fgr_augment_workspace_bytes: bad arguments");
    *bytes = tf_bytes(n_pairs) + (size_t)n_points * sizeof(int32_t);
    return FGR_OK;
}

extern "C" int fgr_augment_pairs(const float* xyz, int32_t ld, const int64_t* in_off,
                                 int64_t n_points, const uint8_t* overlap,
                                 const int64_t* corr, int64_t corr_ld, const int64_t* corr_off,
                                 const float* pose, const float* perturb, const int32_t* flags,
                                 const int32_t* perm, const int64_t* out_off, int32_t max_out,
                                 const float* noise, int32_t n_pairs, float* xyz_out,
                                 uint8_t* overlap_out, int64_t* corr_out, int32_t* n_corr,
                                 float* pose_out, void* ws, size_t ws_bytes, void* stream) {
    FGR_REQUIRE(n_pairs > 0 && ld >= 3 && n_points > 0 && max_out > 0 &&
                    corr_ld >= 0,
                "fgr_augment_pairs: bad arguments");
    FGR_REQUIRE(xyz && in_off && overlap && corr_off && pose && perturb && flags && perm &&
                    out_off && xyz_out && overlap_out && n_corr && pose_out && ws,
                "fgr_augment_pairs: null pointer");
    FGR_REQUIRE(corr_ld == 0 || (corr && corr_out), "fgr_augment_pairs: null pointer (corr)");
    FGR_REQUIRE(reinterpret_cast<uintptr_t>(ws) % 8 == 0, "fgr_augment_pairs: ws not 8-B aligned");
    const size_t need = tf_bytes(n_pairs) + (size_t)n_points * sizeof(int32_t);
    FGR_REQUIRE(ws_bytes >= need, "fgr_augment_pairs: workspace of %zu bytes, need %zu", ws_bytes,
                need);
    double* tf = static_cast<double*>(ws);
    int32_t* inv = reinterpret_cast<int32_t*>(static_cast<char*>(ws) + tf_bytes(n_pairs));
    hipStream_t st = as_stream(stream);
    TimedCall tc(st);
    hipLaunchKernelGGL(augment_pose_kernel, dim3((unsigned)n_pairs), dim3(kPoseThreads), 0, st, xyz,
                       ld, in_off, pose, perturb, flags, pose_out, tf, inv);
    FGR_CHECK_LAUNCH("augment_pose_kernel");
    const unsigned tiles = (unsigned)ceil_div(max_out, kTileRows);
    hipLaunchKernelGGL(augment_gather_kernel, dim3(tiles, (unsigned)n_pairs * 2), dim3(kTileRows),
                       0, st, xyz, ld, in_off, overlap, perm, out_off, noise, flags, tf, xyz_out,
                       overlap_out, inv);
    FGR_CHECK_LAUNCH("augment_gather_kernel");
    hipLaunchKernelGGL(augment_corr_kernel, dim3((unsigned)n_pairs), dim3(kCorrThreads), 0, st,
                       corr, corr_ld, corr_off, in_off, flags, inv, corr_out, n_corr);
    FGR_CHECK_LAUNCH("augment_corr_kernel");
    return FGR_OK;
}
