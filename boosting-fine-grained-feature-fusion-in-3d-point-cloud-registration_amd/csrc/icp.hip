// Point-to-point and point-to-plane ICP on the full clouds, resident on the device: refine a
// predicted pose, then say how good it is (fitness, inlier RMSE, the 6x6 information matrix).
// include/fgreg.h states the semantics; tests/_icp_ref.py and tests/_icp_plane_ref.py restate
// them in numpy.
//
// * The targets never move: they are binned once per call into the radius search's cell grid
//   (grid_common.h, edge >= 1.0625 max_dist) and the source is the side that is transformed.
// * icp_assoc_kernel, one launch per pass: each source point reads its pair's current pose from
//   device memory, transforms itself in fp32 as written, scans the 27 cells around the result
//   and keeps the nearest target (lowest row on an exact d2 tie; the members of a cell are in
//   arrival order, so the tie rule is applied to every candidate). The inliers' moments -- the
//   count, sum p, sum s, sum p s^T, sum d2 and, for the information matrix, sum s s^T -- are
//   reduced per block in fp64 (shuffle tree, fixed order) and stored in the block's own slot of
//   the workspace: no floating-point atomics, the same bits every run.
//   kLpp lanes share one source point (FGR_ICP_LPP, a power of two <= 32: lane j takes cells
//   j, j + kLpp, ... of the 27 and a shuffle picks the group's best). 1 = a thread per point;
//   8 is the fastest of 1, 4, 8, 16, 32 at 717-, 20k- and 60k-point clouds (DESIGN.md "Pose
//   refinement": a pass takes 25 / 33 / 85 us against 44 / 77 / 278 us with a thread per point).
// * icp_step_kernel, one block per pair after each pass: sums the pair's slots in a fixed
//   order, writes fitness and rmse, applies the stopping rule and, if the pair goes on, solves
//   the Procrustes update (procrustes.h's Jacobi SVD, fp64) and stores the next pose as fp32.
//   A done pair sets a flag in the workspace; the later passes' blocks of that pair return at
//   once, so its outputs are frozen. max_iters + 1 passes are enqueued unconditionally: the
//   host never reads anything back.
// * icp_score_kernel finishes a single pass for fgr_registration_score, the information matrix
//   included: sum J^T J with J = [I | -[s]x] is a function of n, sum s and sum s s^T alone.
// * fgr_icp_plane (normals from normals.hip or the caller): icp_plane_assoc_kernel shares the
//   scan (nearest_target) and reduces the 6 x 6 normal equations -- count, sum d2, sum rho^2,
//   the 21 upper terms of sum a a^T and the 6 of sum a rho, a = [n | q x n], rho = n . (q - s)
//   -- into 30-double slots of its own; icp_plane_step_kernel applies the same stopping rule,
//   stops a singular system (a Cholesky pivot <= 1e-12 trace), solves, and composes the pose
//   with exp([w]x) in fp64. 8 lanes per point stay the fastest of 4, 8, 16.
// Built with -ffp-contract=off (see geom.hip): the transform and d2 round as written.
#include "common.h"
#include "grid_common.h"
#include "procrustes.h"

#ifndef FGR_ICP_LPP
#define FGR_ICP_LPP 8
#endif

namespace fgr {
namespace {

constexpr int kIcpThreads = kPoseThreads;          // block_reduce's block
constexpr int kLpp = FGR_ICP_LPP;                  // lanes per source point
constexpr int kIcpPts = kIcpThreads / kLpp;        // source points per block
constexpr int kPart = 24;                          // doubles per partial slot (23 used)
static_assert(kLpp >= 1 && kLpp <= 32 && (kLpp & (kLpp - 1)) == 0, "FGR_ICP_LPP: 1, 2, .. 32");

// slot layout: 0 count | 1..3 sum p | 4..6 sum s | 7..15 sum p s^T (row p) | 16 sum d2 |
//              17..22 sum s s^T (xx xy xz yy yz zz)
constexpr int kNMoments = 17, kNInfo = 23;

struct IcpState {
    double f_prev, e_prev;
    int done, pad;
};

// first slot of pair b: its blocks never reach the next pair's first slot, since
// ceil(len / P) <= floor(end / P) - floor(begin / P) + 1
__device__ __forceinline__ int64_t pair_slot0(int64_t begin, int b) { return begin / kIcpPts + b; }
int64_t icp_slots(int64_t n_src_tot, int32_t n_pairs) { return n_src_tot / kIcpPts + n_pairs; }

__device__ __forceinline__ bool nearer(float d2, int m, float best, int bm) {
    return d2 < best || (d2 == best && m < bm);
}

// the nearest target of q = (qx, qy, qz) in the 27 cells around it, lowest row on an exact d2
// tie; lane `sub` of the point's kLpp lanes takes cells sub, sub + kLpp, ... and a shuffle
// gives every lane of the group the group's best
__device__ __forceinline__ void nearest_target(float qx, float qy, float qz, const RGrid& g,
                                               const int* __restrict__ start,
                                               const int* __restrict__ members,
                                               const float* __restrict__ tgt, int sub,
                                               float* best_out, int* bm_out) {
    // a query far outside the grid: the conversion saturates, the clamp keeps cx + 1 in range
    const int cx = min(max(cell_coord(qx, g.org[0], g.cell), -2), g.nx + 1);
    const int cy = min(max(cell_coord(qy, g.org[1], g.cell), -2), g.ny + 1);
    const int cz = min(max(cell_coord(qz, g.org[2], g.cell), -2), g.nz + 1);
    float best = INFINITY;
    int bm = 0x7fffffff;
    for (int c = sub; c < 27; c += kLpp) {
        const int x = cx + c % 3 - 1, y = cy + (c / 3) % 3 - 1, z = cz + c / 9 - 1;
        if (x < 0 || x >= g.nx || y < 0 || y >= g.ny || z < 0 || z >= g.nz) continue;
        const long long cell = g.base + ((long long)z * g.ny + y) * g.nx + x;
        const int e = start[cell + 1];
        for (int j = start[cell]; j < e; ++j) {
            const int m = members[j];
            const float d2 = dist2g(qx, qy, qz, tgt[3 * (int64_t)m], tgt[3 * (int64_t)m + 1],
                                    tgt[3 * (int64_t)m + 2]);
            if (nearer(d2, m, best, bm)) { best = d2; bm = m; }
        }
    }
#pragma unroll
    for (int o = kLpp / 2; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o, 64);
        const int om = __shfl_xor(bm, o, 64);
        if (nearer(ob, om, best, bm)) { best = ob; bm = om; }
    }
    *best_out = best;
    *bm_out = bm;
}

// term k of a slot for one inlier (p, s in fp64, d2): every k is a compile-time constant
__device__ __forceinline__ double moment_term(int k, bool on, const double* p, const double* s,
                                              double d2) {
    if (k == 0) return on ? 1.0 : 0.0;
    if (k < 4) return p[k - 1];
    if (k < 7) return s[k - 4];
    if (k < 16) return p[(k - 7) / 3] * s[(k - 7) % 3];
    if (k == 16) return d2;
    const int r = k < 20 ? 0 : (k < 22 ? 1 : 2), c = k < 20 ? k - 17 : (k < 22 ? k - 19 : 2);
    return s[r] * s[c];
}

template <bool OUT, bool INFO>
__global__ void __launch_bounds__(kIcpThreads)
icp_assoc_kernel(const float* __restrict__ src, const int64_t* __restrict__ src_off,
                 const float* __restrict__ tgt, const int64_t* __restrict__ tgt_off,
                 const RGrid* __restrict__ grids, const int* __restrict__ start,
                 const int* __restrict__ members, const float* __restrict__ pose,
                 const IcpState* __restrict__ state, float r2, double* __restrict__ part,
                 int* __restrict__ idx_out, float* __restrict__ d2_out) {
    __shared__ double sh[(kIcpThreads / 64) * kPart];
    const int b = blockIdx.y;
    if (state && state[b].done) return;                    // block-uniform: a frozen pair
    const int64_t sb = src_off[b], se = src_off[b + 1];
    const int64_t p0 = (int64_t)blockIdx.x * kIcpPts;
    if (p0 >= se - sb) return;                             // block-uniform
    const int64_t tb = tgt_off[b];
    const int grp = threadIdx.x / kLpp, sub = threadIdx.x % kLpp;
    const int64_t i = sb + p0 + grp;
    const bool valid = i < se;
    const int64_t ic = valid ? i : sb + p0;                // always a row of this pair
    const float* T = pose + 12 * b;
    const float px = src[3 * ic], py = src[3 * ic + 1], pz = src[3 * ic + 2];
    const float qx = ((T[0] * px + T[1] * py) + T[2] * pz) + T[3];
    const float qy = ((T[4] * px + T[5] * py) + T[6] * pz) + T[7];
    const float qz = ((T[8] * px + T[9] * py) + T[10] * pz) + T[11];
    const RGrid g = grids[b];
    float best;
    int bm;
    nearest_target(qx, qy, qz, g, start, members, tgt, sub, &best, &bm);
    const bool inl = valid && best < r2;                   // NaN and +inf are no inliers
    // this lane's terms (zero unless it carries an inlier), reduced one at a time so that the
    // search loop above keeps its registers: shuffle tree per wave, then the waves in order
    const bool on = inl && sub == 0;
    const int64_t bc = on ? bm : tb;                       // never dereferenced when !on
    double p[3] = {0.0, 0.0, 0.0}, s[3] = {0.0, 0.0, 0.0};
    if (on) {
        p[0] = px; p[1] = py; p[2] = pz;
        s[0] = tgt[3 * bc]; s[1] = tgt[3 * bc + 1]; s[2] = tgt[3 * bc + 2];
    }
    const double d2v = on ? (double)best : 0.0;
    constexpr int N = INFO ? kNInfo : kNMoments;
    const int wv = threadIdx.x / 64, lane = threadIdx.x % 64;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        double x = moment_term(k, on, p, s, d2v);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
        if (lane == 0) sh[wv * kPart + k] = x;
    }
    __syncthreads();
    if (threadIdx.x < N) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < kIcpThreads / 64; ++w) t += sh[w * kPart + threadIdx.x];
        part[(pair_slot0(sb, b) + blockIdx.x) * kPart + threadIdx.x] = t;
    }
    if (OUT && valid && sub == 0) {
        if (idx_out) idx_out[i] = inl ? (int)(bm - tb) : -1;
        if (d2_out) d2_out[i] = inl ? best : INFINITY;
    }
}

// v[0..n) <- the sums over the pair's slots: thread t adds slots t, t + 256, ... in ascending
// order, then the block's shuffle tree -- the same order every run. All threads hold the sums.
__device__ void sum_slots(const double* __restrict__ part, int64_t slot0, int64_t n_slots, int n,
                          double* v, double* sh) {
    for (int k = 0; k < kPart; ++k) v[k] = 0.0;
    for (int64_t s = threadIdx.x; s < n_slots; s += kIcpThreads)
        for (int k = 0; k < n; ++k) v[k] += part[(slot0 + s) * kPart + k];
    block_reduce(v, 16, sh);
    block_reduce(v + 16, n - 16, sh);
}

__device__ __forceinline__ void fitness_rmse(const double* v, int64_t n_src, double* f, double* e) {
    *f = n_src > 0 ? v[0] / (double)n_src : 0.0;
    *e = v[0] > 0.0 ? sqrt(v[16] / v[0]) : 0.0;
}

__global__ void icp_init_kernel(const float* __restrict__ pose_in, int n_pairs,
                                IcpState* __restrict__ state, float* __restrict__ pose_out,
                                float* __restrict__ fitness, float* __restrict__ rmse,
                                int* __restrict__ n_iters) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < 12 * n_pairs) pose_out[t] = pose_in[t];
    if (t < n_pairs) {
        IcpState s;
        s.f_prev = s.e_prev = 0.0;
        s.done = s.pad = 0;
        state[t] = s;
        fitness[t] = 0.f;
        rmse[t] = 0.f;
        n_iters[t] = 0;
    }
}

// pass k of pair blockIdx.x, after its association
__global__ void __launch_bounds__(kIcpThreads)
icp_step_kernel(const double* __restrict__ part, const int64_t* __restrict__ src_off,
                IcpState* __restrict__ state, float* __restrict__ pose,
                float* __restrict__ fitness, float* __restrict__ rmse, int* __restrict__ n_iters,
                int k, int max_iters, double rel_fitness, double rel_rmse) {
    __shared__ double sh[(kIcpThreads / 64) * 16];
    const int b = blockIdx.x;
    // read by every thread before the barriers of sum_slots, written by thread 0 after them
    if (state[b].done) return;
    const int64_t sb = src_off[b], n_src = src_off[b + 1] - sb;
    double v[kPart];
    sum_slots(part, pair_slot0(sb, b), (n_src + kIcpPts - 1) / kIcpPts, kNMoments, v, sh);
    if (threadIdx.x != 0) return;
    double f, e;
    fitness_rmse(v, n_src, &f, &e);
    fitness[b] = (float)f;
    rmse[b] = (float)e;
    const IcpState prev = state[b];
    const bool converged = k >= 1 && fabs(f - prev.f_prev) < rel_fitness &&
                           fabs(e - prev.e_prev) < rel_rmse;
    state[b].f_prev = f;
    state[b].e_prev = e;
    if (converged || v[0] < 3.0 || k == max_iters) {
        state[b].done = 1;
        return;
    }
    const double n = v[0];
    double H[3][3], R[3][3], pm[3], sm[3];
    for (int r = 0; r < 3; ++r) {
        pm[r] = v[1 + r] / n;
        sm[r] = v[4 + r] / n;
    }
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) H[r][c] = v[7 + 3 * r + c] - v[1 + r] * v[4 + c] / n;
    svd3_rotation(H, R);
    float* T = pose + 12 * b;
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) T[4 * r + c] = (float)R[r][c];
        T[4 * r + 3] = (float)(sm[r] - (R[r][0] * pm[0] + R[r][1] * pm[1] + R[r][2] * pm[2]));
    }
    n_iters[b] = k + 1;
}

__global__ void __launch_bounds__(kIcpThreads)
icp_score_kernel(const double* __restrict__ part, const int64_t* __restrict__ src_off,
                 float* __restrict__ fitness, float* __restrict__ rmse, double* __restrict__ info) {
    __shared__ double sh[(kIcpThreads / 64) * 16];
    const int b = blockIdx.x;
    const int64_t sb = src_off[b], n_src = src_off[b + 1] - sb;
    double v[kPart];
    sum_slots(part, pair_slot0(sb, b), (n_src + kIcpPts - 1) / kIcpPts, kNInfo, v, sh);
    if (threadIdx.x != 0) return;
    double f, e;
    fitness_rmse(v, n_src, &f, &e);
    fitness[b] = (float)f;
    rmse[b] = (float)e;
    if (!info) return;
    // J = [I | A], A = -[s]x: J^T J = [I, A; A^T, A^T A], A^T A = |s|^2 I - s s^T
    const double sx = v[4], sy = v[5], sz = v[6];
    const double xx = v[17], xy = v[18], xz = v[19], yy = v[20], yz = v[21], zz = v[22];
    const double A[3][3] = {{0.0, sz, -sy}, {-sz, 0.0, sx}, {sy, -sx, 0.0}};
    const double Q[3][3] = {{yy + zz, -xy, -xz}, {-xy, xx + zz, -yz}, {-xz, -yz, xx + yy}};
    double* G = info + 36 * b;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            G[6 * r + c] = r == c ? v[0] : 0.0;
            G[6 * r + 3 + c] = A[r][c];
            G[6 * (3 + r) + c] = A[c][r];
            G[6 * (3 + r) + 3 + c] = Q[r][c];
        }
}

// ------------------------------------------------------------------------------------------
// point-to-plane: the same association, the 6 x 6 normal equations as the moments
// ------------------------------------------------------------------------------------------
// slot layout: 0 count | 1 sum d2 | 2 sum rho^2 | 3..23 sum a a^T, upper triangle by rows |
//              24..29 sum a rho, with a = [n | q x n] (translation first) and rho = n . (q - s)
constexpr int kPlanePart = 30;                     // doubles per partial slot, all used
constexpr int kPlaneMinInl = 6;
enum { kPlaneConverged = 0, kPlaneMaxIters = 1, kPlaneFewInliers = 2, kPlaneSingular = 3 };

// term k of a plane slot for one inlier: every k is a compile-time constant
__device__ __forceinline__ double plane_term(int k, bool on, const double* a, double rho,
                                             double d2) {
    if (k == 0) return on ? 1.0 : 0.0;
    if (k == 1) return d2;
    if (k == 2) return rho * rho;
    if (k >= 24) return a[k - 24] * rho;
    int t = k - 3, r = 0;
    while (t >= 6 - r) { t -= 6 - r; ++r; }
    return a[r] * a[r + t];
}

__global__ void __launch_bounds__(kIcpThreads)
icp_plane_assoc_kernel(const float* __restrict__ src, const int64_t* __restrict__ src_off,
                       const float* __restrict__ tgt, const int64_t* __restrict__ tgt_off,
                       const float* __restrict__ nrm, const RGrid* __restrict__ grids,
                       const int* __restrict__ start, const int* __restrict__ members,
                       const float* __restrict__ pose, const IcpState* __restrict__ state,
                       float r2, double* __restrict__ part) {
    __shared__ double sh[(kIcpThreads / 64) * kPlanePart];
    const int b = blockIdx.y;
    if (state[b].done) return;                             // block-uniform: a frozen pair
    const int64_t sb = src_off[b], se = src_off[b + 1];
    const int64_t p0 = (int64_t)blockIdx.x * kIcpPts;
    if (p0 >= se - sb) return;                             // block-uniform
    const int64_t tb = tgt_off[b];
    const int grp = threadIdx.x / kLpp, sub = threadIdx.x % kLpp;
    const int64_t i = sb + p0 + grp;
    const bool valid = i < se;
    const int64_t ic = valid ? i : sb + p0;                // always a row of this pair
    const float* T = pose + 12 * b;
    const float px = src[3 * ic], py = src[3 * ic + 1], pz = src[3 * ic + 2];
    const float qx = ((T[0] * px + T[1] * py) + T[2] * pz) + T[3];
    const float qy = ((T[4] * px + T[5] * py) + T[6] * pz) + T[7];
    const float qz = ((T[8] * px + T[9] * py) + T[10] * pz) + T[11];
    const RGrid g = grids[b];
    float best;
    int bm;
    nearest_target(qx, qy, qz, g, start, members, tgt, sub, &best, &bm);
    const bool cand = valid && best < r2 && sub == 0;      // NaN and +inf are no inliers
    const int64_t bc = cand ? bm : tb;                     // never dereferenced when !cand
    double a[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, rho = 0.0;
    bool on = false;
    if (cand) {
        const float nx = nrm[3 * bc], ny = nrm[3 * bc + 1], nz = nrm[3 * bc + 2];
        on = !(nx == 0.f && ny == 0.f && nz == 0.f);       // the zero normal: no inlier
        if (on) {
            const double q[3] = {qx, qy, qz};
            const double d[3] = {q[0] - (double)tgt[3 * bc], q[1] - (double)tgt[3 * bc + 1],
                                 q[2] - (double)tgt[3 * bc + 2]};
            a[0] = nx; a[1] = ny; a[2] = nz;
            a[3] = q[1] * a[2] - q[2] * a[1];
            a[4] = q[2] * a[0] - q[0] * a[2];
            a[5] = q[0] * a[1] - q[1] * a[0];
            rho = (a[0] * d[0] + a[1] * d[1]) + a[2] * d[2];
        }
    }
    const double d2v = on ? (double)best : 0.0;
    const int wv = threadIdx.x / 64, lane = threadIdx.x % 64;
#pragma unroll
    for (int k = 0; k < kPlanePart; ++k) {
        double x = plane_term(k, on, a, rho, d2v);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
        if (lane == 0) sh[wv * kPlanePart + k] = x;
    }
    __syncthreads();
    if (threadIdx.x < kPlanePart) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < kIcpThreads / 64; ++w) t += sh[w * kPlanePart + threadIdx.x];
        part[(pair_slot0(sb, b) + blockIdx.x) * kPlanePart + threadIdx.x] = t;
    }
}

// Cholesky A = L L^T of the symmetric 6 x 6 A, then L L^T x = rhs. false, with x untouched, at a
// pivot <= 1e-12 trace(A)
__device__ bool chol6_solve(const double A[6][6], const double* rhs, double* x) {
    double L[6][6], tr = 0.0;
    for (int i = 0; i < 6; ++i) tr += A[i][i];
    for (int j = 0; j < 6; ++j) {
        double d = A[j][j];
        for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
        if (!(d > 1e-12 * tr)) return false;
        L[j][j] = sqrt(d);
        for (int i = j + 1; i < 6; ++i) {
            double v = A[i][j];
            for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k];
            L[i][j] = v / L[j][j];
        }
    }
    double y[6];
    for (int i = 0; i < 6; ++i) {
        double v = rhs[i];
        for (int k = 0; k < i; ++k) v -= L[i][k] * y[k];
        y[i] = v / L[i][i];
    }
    for (int i = 5; i >= 0; --i) {
        double v = y[i];
        for (int k = i + 1; k < 6; ++k) v -= L[k][i] * x[k];
        x[i] = v / L[i][i];
    }
    return true;
}

// pass k of pair blockIdx.x, after its association
__global__ void __launch_bounds__(kIcpThreads)
icp_plane_step_kernel(const double* __restrict__ part, const int64_t* __restrict__ src_off,
                      IcpState* __restrict__ state, float* __restrict__ pose,
                      float* __restrict__ fitness, float* __restrict__ rmse,
                      float* __restrict__ plane_rmse, int* __restrict__ n_iters,
                      int* __restrict__ status, double* __restrict__ info, int k, int max_iters,
                      double rel_fitness, double rel_rmse) {
    __shared__ double sh[(kIcpThreads / 64) * 16];
    const int b = blockIdx.x;
    // read by every thread before the barriers of the reduction, written by thread 0 after them
    if (state[b].done) return;
    const int64_t sb = src_off[b], n_src = src_off[b + 1] - sb;
    const int64_t slot0 = pair_slot0(sb, b), n_slots = (n_src + kIcpPts - 1) / kIcpPts;
    // thread t adds slots t, t + 256, ... in ascending order, then the block's shuffle tree
    double v[32];
    for (int j = 0; j < 32; ++j) v[j] = 0.0;
    for (int64_t s = threadIdx.x; s < n_slots; s += kIcpThreads)
        for (int j = 0; j < kPlanePart; ++j) v[j] += part[(slot0 + s) * kPlanePart + j];
    block_reduce(v, 16, sh);
    block_reduce(v + 16, kPlanePart - 16, sh);
    if (threadIdx.x != 0) return;
    const double n = v[0];
    const double f = n_src > 0 ? n / (double)n_src : 0.0;
    const double e = n > 0.0 ? sqrt(v[1] / n) : 0.0;
    fitness[b] = (float)f;
    rmse[b] = (float)e;
    plane_rmse[b] = (float)(n > 0.0 ? sqrt(v[2] / n) : 0.0);
    const IcpState prev = state[b];
    const bool converged = k >= 1 && fabs(f - prev.f_prev) < rel_fitness &&
                           fabs(e - prev.e_prev) < rel_rmse;
    state[b].f_prev = f;
    state[b].e_prev = e;
    double A[6][6], rhs[6], x[6];
    for (int r = 0, t = 3; r < 6; ++r)
        for (int c = r; c < 6; ++c, ++t) A[r][c] = A[c][r] = v[t];
    for (int r = 0; r < 6; ++r) rhs[r] = -v[24 + r];
    int stop = -1;
    if (converged) stop = kPlaneConverged;
    else if (n < (double)kPlaneMinInl) stop = kPlaneFewInliers;
    else if (!chol6_solve(A, rhs, x)) stop = kPlaneSingular;
    else if (k == max_iters) stop = kPlaneMaxIters;
    if (stop >= 0) {
        state[b].done = 1;
        if (status) status[b] = stop;
        if (info)
            for (int r = 0; r < 6; ++r)
                for (int c = 0; c < 6; ++c) info[36 * b + 6 * r + c] = A[r][c];
        return;
    }
    // x = (t, w): dR = exp([w]x) by Rodrigues, T <- [dR R | dR t_old + t]
    const double wx = x[3], wy = x[4], wz = x[5];
    const double th = sqrt((wx * wx + wy * wy) + wz * wz);
    const double ca = th < 1e-12 ? 1.0 : sin(th) / th;
    const double cb = th < 1e-12 ? 0.5 : (1.0 - cos(th)) / (th * th);
    const double K[3][3] = {{0.0, -wz, wy}, {wz, 0.0, -wx}, {-wy, wx, 0.0}};
    double dR[3][3], Tn[3][4];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c)
            dR[r][c] = (r == c ? 1.0 : 0.0) + ca * K[r][c] +
                       cb * ((K[r][0] * K[0][c] + K[r][1] * K[1][c]) + K[r][2] * K[2][c]);
    float* T = pose + 12 * b;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c)
            Tn[r][c] = ((dR[r][0] * (double)T[c] + dR[r][1] * (double)T[4 + c]) +
                        dR[r][2] * (double)T[8 + c]) + (c == 3 ? x[r] : 0.0);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) T[4 * r + c] = (float)Tn[r][c];
    n_iters[b] = k + 1;
}

struct IcpWs {
    RGridWs grid;
    double* part;
    IcpState* state;
    size_t total;
};

void carve_icp(void* ws, int64_t n_src_tot, int64_t n_tgt_tot, int32_t n_pairs, IcpWs* w) {
    carve_rgrid(ws, n_tgt_tot, n_pairs, &w->grid);
    char* p = static_cast<char*>(ws);
    size_t o = w->grid.total;
    auto take = [&](size_t bytes) { void* r = p ? p + o : nullptr; o += align_up(bytes); return r; };
    w->part = (double*)take(sizeof(double) * kPart * icp_slots(n_src_tot, n_pairs));
    w->state = (IcpState*)take(sizeof(IcpState) * n_pairs);
    w->total = o;
}

void carve_icp_plane(void* ws, int64_t n_src_tot, int64_t n_tgt_tot, int32_t n_pairs, IcpWs* w) {
    carve_rgrid(ws, n_tgt_tot, n_pairs, &w->grid);
    char* p = static_cast<char*>(ws);
    size_t o = w->grid.total;
    auto take = [&](size_t bytes) { void* r = p ? p + o : nullptr; o += align_up(bytes); return r; };
    w->part = (double*)take(sizeof(double) * kPlanePart * icp_slots(n_src_tot, n_pairs));
    w->state = (IcpState*)take(sizeof(IcpState) * n_pairs);
    w->total = o;
}

bool icp_sizes_ok(int64_t n_src_tot, int64_t n_tgt_tot, int32_t n_pairs) {
    return n_pairs > 0 && n_pairs <= 65535 && n_src_tot >= 0 && n_tgt_tot >= 0 &&
           n_src_tot < (1ll << 31) &&
           4 * n_tgt_tot + 1024ll * n_pairs < (1ll << 31) - 1;
}

}  // namespace
}  // namespace fgr

using namespace fgr;

extern "C" int fgr_icp_workspace(int64_t n_src_tot, int64_t n_tgt_tot, int32_t n_pairs,
                                 size_t* bytes) {
    FGR_REQUIRE(bytes && icp_sizes_ok(n_src_tot, n_tgt_tot, n_pairs),
                "fgr_icp_workspace: bad arguments");
    IcpWs w;
    carve_icp(nullptr, n_src_tot, n_tgt_tot, n_pairs, &w);
    *bytes = w.total;
    return FGR_OK;
}

extern "C" int fgr_icp(const float* src, const int64_t* src_off, int64_t n_src_tot,
                       const float* tgt, const int64_t* tgt_off, int64_t n_tgt_tot,
                       int32_t n_pairs, int32_t max_src_len, const float* pose_in, float max_dist,
                       int32_t max_iters, float rel_fitness, float rel_rmse, void* ws,
                       size_t ws_bytes, float* pose_out, float* fitness, float* rmse,
                       int32_t* n_iters, void* stream) {
    FGR_REQUIRE(icp_sizes_ok(n_src_tot, n_tgt_tot, n_pairs) && src_off && tgt_off && pose_in &&
                    ws && pose_out && fitness && rmse && n_iters && (src || n_src_tot == 0) &&
                    (tgt || n_tgt_tot == 0) && max_src_len >= 0 && max_src_len <= n_src_tot &&
                    max_dist > 0.f && max_iters >= 0 && rel_fitness >= 0.f && rel_rmse >= 0.f &&
                    pose_out != pose_in,
                "fgr_icp: bad arguments (n_pairs %d max_src_len %d max_dist %g max_iters %d)",
                n_pairs, max_src_len, (double)max_dist, max_iters);
    IcpWs w;
    carve_icp(ws, n_src_tot, n_tgt_tot, n_pairs, &w);
    if (w.total > ws_bytes) {
        set_error("fgr_icp: workspace %zu < %zu bytes", ws_bytes, w.total);
        return FGR_E_WORKSPACE;
    }
    hipStream_t st = as_stream(stream);
    TimedCall timed_(st);
    hipLaunchKernelGGL(icp_init_kernel, dim3((unsigned)ceil_div(12 * (int64_t)n_pairs, 256)),
                       dim3(256), 0, st, pose_in, n_pairs, w.state, pose_out, fitness, rmse,
                       n_iters);
    FGR_CHECK_LAUNCH("icp_init_kernel");
    int rc = launch_rgrid_build(tgt, tgt_off, n_pairs, n_tgt_tot, max_dist, w.grid, st);
    if (rc != FGR_OK) return rc;
    const float r2 = max_dist * max_dist;
    const dim3 grd((unsigned)ceil_div(max_src_len, kIcpPts), (unsigned)n_pairs);
    for (int k = 0; k <= max_iters; ++k) {
        if (grd.x > 0) {
            hipLaunchKernelGGL((icp_assoc_kernel<false, false>), grd, dim3(kIcpThreads), 0, st, src,
                               src_off, tgt, tgt_off, w.grid.grids, w.grid.start, w.grid.members,
                               pose_out, w.state, r2, w.part, (int*)nullptr, (float*)nullptr);
            FGR_CHECK_LAUNCH("icp_assoc_kernel");
        }
        hipLaunchKernelGGL(icp_step_kernel, dim3((unsigned)n_pairs), dim3(kIcpThreads), 0, st,
                           w.part, src_off, w.state, pose_out, fitness, rmse, n_iters, k, max_iters,
                           (double)rel_fitness, (double)rel_rmse);
        FGR_CHECK_LAUNCH("icp_step_kernel");
    }
    return FGR_OK;
}

extern "C" int fgr_registration_score(const float* src, const int64_t* src_off, int64_t n_src_tot,
                                      const float* tgt, const int64_t* tgt_off, int64_t n_tgt_tot,
                                      int32_t n_pairs, int32_t max_src_len, const float* pose,
                                      float max_dist, void* ws, size_t ws_bytes, float* fitness,
                                      float* rmse, int32_t* idx, float* d2, double* info,
                                      void* stream) {
    FGR_REQUIRE(icp_sizes_ok(n_src_tot, n_tgt_tot, n_pairs) && src_off && tgt_off && pose && ws &&
                    fitness && rmse && (src || n_src_tot == 0) && (tgt || n_tgt_tot == 0) &&
                    max_src_len >= 0 && max_src_len <= n_src_tot && max_dist > 0.f,
                "fgr_registration_score: bad arguments (n_pairs %d max_src_len %d max_dist %g)",
                n_pairs, max_src_len, (double)max_dist);
    IcpWs w;
    carve_icp(ws, n_src_tot, n_tgt_tot, n_pairs, &w);
    if (w.total > ws_bytes) {
        set_error("fgr_registration_score: workspace %zu < %zu bytes", ws_bytes, w.total);
        return FGR_E_WORKSPACE;
    }
    hipStream_t st = as_stream(stream);
    TimedCall timed_(st);
    int rc = launch_rgrid_build(tgt, tgt_off, n_pairs, n_tgt_tot, max_dist, w.grid, st);
    if (rc != FGR_OK) return rc;
    const float r2 = max_dist * max_dist;
    const dim3 grd((unsigned)ceil_div(max_src_len, kIcpPts), (unsigned)n_pairs);
    if (grd.x > 0) {
        hipLaunchKernelGGL((icp_assoc_kernel<true, true>), grd, dim3(kIcpThreads), 0, st, src,
                           src_off, tgt, tgt_off, w.grid.grids, w.grid.start, w.grid.members, pose,
                           (const IcpState*)nullptr, r2, w.part, idx, d2);
        FGR_CHECK_LAUNCH("icp_assoc_kernel");
    }
    hipLaunchKernelGGL(icp_score_kernel, dim3((unsigned)n_pairs), dim3(kIcpThreads), 0, st, w.part,
                       src_off, fitness, rmse, info);
    FGR_CHECK_LAUNCH("icp_score_kernel");
    return FGR_OK;
}

extern "C" int fgr_icp_plane_workspace(int64_t n_src_tot, int64_t n_tgt_tot, int32_t n_pairs,
                                       size_t* bytes) {
    FGR_REQUIRE(bytes && icp_sizes_ok(n_src_tot, n_tgt_tot, n_pairs),
                "fgr_icp_plane_workspace: bad arguments");
    IcpWs w;
    carve_icp_plane(nullptr, n_src_tot, n_tgt_tot, n_pairs, &w);
    *bytes = w.total;
    return FGR_OK;
}

extern "C" int fgr_icp_plane(const float* src, const int64_t* src_off, int64_t n_src_tot,
                             const float* tgt, const int64_t* tgt_off, int64_t n_tgt_tot,
                             const float* tgt_normals, int32_t n_pairs, int32_t max_src_len,
                             const float* pose_in, float max_dist, int32_t max_iters,
                             float rel_fitness, float rel_rmse, void* ws, size_t ws_bytes,
                             float* pose_out, float* fitness, float* rmse, float* plane_rmse,
                             int32_t* n_iters, int32_t* status, double* info, void* stream) {
    FGR_REQUIRE(icp_sizes_ok(n_src_tot, n_tgt_tot, n_pairs) && src_off && tgt_off && pose_in &&
                    ws && pose_out && fitness && rmse && plane_rmse && n_iters &&
                    (src || n_src_tot == 0) && ((tgt && tgt_normals) || n_tgt_tot == 0) &&
                    max_src_len >= 0 && max_src_len <= n_src_tot && max_dist > 0.f &&
                    max_iters >= 0 && rel_fitness >= 0.f && rel_rmse >= 0.f && pose_out != pose_in,
                "fgr_icp_plane: bad arguments (n_pairs %d max_src_len %d max_dist %g max_iters %d)",
                n_pairs, max_src_len, (double)max_dist, max_iters);
    IcpWs w;
    carve_icp_plane(ws, n_src_tot, n_tgt_tot, n_pairs, &w);
    if (w.total > ws_bytes) {
        set_error("fgr_icp_plane: workspace %zu < %zu bytes", ws_bytes, w.total);
        return FGR_E_WORKSPACE;
    }
    hipStream_t st = as_stream(stream);
    TimedCall timed_(st);
    hipLaunchKernelGGL(icp_init_kernel, dim3((unsigned)ceil_div(12 * (int64_t)n_pairs, 256)),
                       dim3(256), 0, st, pose_in, n_pairs, w.state, pose_out, fitness, rmse,
                       n_iters);
    FGR_CHECK_LAUNCH("icp_init_kernel");
    int rc = launch_rgrid_build(tgt, tgt_off, n_pairs, n_tgt_tot, max_dist, w.grid, st);
    if (rc != FGR_OK) return rc;
    const float r2 = max_dist * max_dist;
    const dim3 grd((unsigned)ceil_div(max_src_len, kIcpPts), (unsigned)n_pairs);
    for (int k = 0; k <= max_iters; ++k) {
        if (grd.x > 0) {
            hipLaunchKernelGGL(icp_plane_assoc_kernel, grd, dim3(kIcpThreads), 0, st, src, src_off,
                               tgt, tgt_off, tgt_normals, w.grid.grids, w.grid.start,
                               w.grid.members, pose_out, w.state, r2, w.part);
            FGR_CHECK_LAUNCH("icp_plane_assoc_kernel");
        }
        hipLaunchKernelGGL(icp_plane_step_kernel, dim3((unsigned)n_pairs), dim3(kIcpThreads), 0, st,
                           w.part, src_off, w.state, pose_out, fitness, rmse, plane_rmse, n_iters,
                           status, info, k, max_iters, (double)rel_fitness, (double)rel_rmse);
        FGR_CHECK_LAUNCH("icp_plane_step_kernel");
    }
    return FGR_OK;
}
