// Surface normals of packed clouds, resident on the device: what point-to-plane ICP (icp.hip,
// fgr_icp_plane) is given. include/fgreg.h states the semantics; tests/_icp_plane_ref.py
// restates them in numpy.
//
// * The cloud is binned into the radius search's cell grid (grid_common.h) at `radius`; the
//   neighbourhood of p is every point s of its cloud with dist2g(p, s) < r2, p itself included.
// * Reproducibility: the grid build fills a cell in atomic (arrival) order, and an fp64 sum
//   taken in that order would change from run to run. cell_rank_kernel therefore puts each
//   cell's members into ascending row order: a member's place inside its cell is the number of
//   members of that cell with a lower row (rows are distinct, so the places are). The shared
//   build is left as it is; the sorted copy lives in this file's part of the workspace.
// * normals_kernel: kLpp lanes share one point (lane j takes cells j, j + kLpp, ... of the 27,
//   as icp_assoc_kernel). Each lane sums its cells' members in the sorted order -- the count,
//   sum d and the six sum d d^T terms, d = s - p formed in fp32, products and sums in fp64 --
//   and a shuffle tree adds the lanes in a fixed order. Lane 0 of the group forms the
//   covariance, takes the eigenvector of its smallest eigenvalue (sym3_eigen: fp64 cyclic
//   Jacobi), orients it towards the viewpoint and stores it as fp32.
// * The per-cloud count of valid normals is an integer: one int32 atomicAdd per wave and cloud.
// Built with -ffp-contract=off: d and d2 round as written.
#include "common.h"
#include "grid_common.h"

#ifndef FGR_NORMALS_LPP
#define FGR_NORMALS_LPP 8
#endif

namespace fgr {
namespace {

constexpr int kNrmThreads = 256;
constexpr int kLpp = FGR_NORMALS_LPP;               // lanes per point
constexpr int kNrmPts = kNrmThreads / kLpp;         // points per block
constexpr int kNrmTerms = 10;                       // count | sum d | xx xy xz yy yz zz
static_assert(kLpp >= 1 && kLpp <= 32 && (kLpp & (kLpp - 1)) == 0, "FGR_NORMALS_LPP: 1, 2, .. 32");

// Eigen-decomposition of the symmetric 3x3 A (upper triangle read) by cyclic Jacobi in fp64:
// w[j] and the unit column V[.][j] are an eigenpair; the pairs are not sorted.
__device__ void sym3_eigen(const double A[3][3], double w[3], double V[3][3]) {
    double a[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            a[i][j] = i <= j ? A[i][j] : A[j][i];
            V[i][j] = i == j ? 1.0 : 0.0;
        }
    for (int sweep = 0; sweep < 30; ++sweep) {
        double off = 0.0;
        for (int p = 0; p < 2; ++p) {
            for (int q = p + 1; q < 3; ++q) {
                const double apq = a[p][q];
                if (fabs(apq) <= 1e-300 || fabs(apq) <= 1e-17 * sqrt(fabs(a[p][p] * a[q][q])))
                    continue;                               // negligible beside both diagonals
                off = fmax(off, fabs(apq));
                const double zeta = (a[q][q] - a[p][p]) / (2.0 * apq);
                const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
                const int r = 3 - p - q;                    // the third index
                const double arp = a[r][p], arq = a[r][q];
                a[p][p] -= t * apq;
                a[q][q] += t * apq;
                a[p][q] = a[q][p] = 0.0;
                a[r][p] = a[p][r] = cs * arp - sn * arq;
                a[r][q] = a[q][r] = sn * arp + cs * arq;
                for (int i = 0; i < 3; ++i) {
                    const double vp = V[i][p], vq = V[i][q];
                    V[i][p] = cs * vp - sn * vq;
                    V[i][q] = sn * vp + cs * vq;
                }
            }
        }
        if (off == 0.0) break;
    }
    for (int j = 0; j < 3; ++j) w[j] = a[j][j];
}

__global__ void normals_init_kernel(int* __restrict__ n_valid, int n_clouds) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n_clouds) n_valid[t] = 0;
}

// sorted[start[c] + #{members of cell c with a lower row than i}] = i
__global__ void cell_rank_kernel(int64_t ns, const int* __restrict__ cellof,
                                 const int* __restrict__ start, const int* __restrict__ members,
                                 int* __restrict__ sorted) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ns) return;
    const int c = cellof[i], b = start[c], e = start[c + 1];
    int rank = 0;
    for (int j = b; j < e; ++j) rank += members[j] < (int)i ? 1 : 0;
    sorted[b + rank] = (int)i;
}

__global__ void __launch_bounds__(kNrmThreads)
normals_kernel(const float* __restrict__ pts, const int64_t* __restrict__ off, int n_clouds,
               int64_t ns, const RGrid* __restrict__ grids, const int* __restrict__ start,
               const int* __restrict__ sorted, const float* __restrict__ view, float r2,
               float* __restrict__ normals, int* __restrict__ n_valid) {
    const int grp = threadIdx.x / kLpp, sub = threadIdx.x % kLpp;
    const int64_t i = (int64_t)blockIdx.x * kNrmPts + grp;
    const bool live = i < ns;
    const int64_t ic = live ? i : ns - 1;                  // ns > 0: always a row
    const int c = find_segment(off, n_clouds, ic);
    const RGrid g = grids[c];
    const float px = pts[3 * ic], py = pts[3 * ic + 1], pz = pts[3 * ic + 2];
    // the point's own cell, as rgrid_key_kernel placed it
    const int cx = min(max(cell_coord(px, g.org[0], g.cell), 0), g.nx - 1);
    const int cy = min(max(cell_coord(py, g.org[1], g.cell), 0), g.ny - 1);
    const int cz = min(max(cell_coord(pz, g.org[2], g.cell), 0), g.nz - 1);
    double m[kNrmTerms];
#pragma unroll
    for (int k = 0; k < kNrmTerms; ++k) m[k] = 0.0;
    for (int q = sub; q < 27; q += kLpp) {
        const int x = cx + q % 3 - 1, y = cy + (q / 3) % 3 - 1, z = cz + q / 9 - 1;
        if (x < 0 || x >= g.nx || y < 0 || y >= g.ny || z < 0 || z >= g.nz) continue;
        const long long cell = g.base + ((long long)z * g.ny + y) * g.nx + x;
        const int e = start[cell + 1];
        for (int j = start[cell]; j < e; ++j) {
            const int64_t s = sorted[j];
            const float sx = pts[3 * s], sy = pts[3 * s + 1], sz = pts[3 * s + 2];
            if (!(dist2g(px, py, pz, sx, sy, sz) < r2)) continue;
            const float fx = sx - px, fy = sy - py, fz = sz - pz;
            const double dx = fx, dy = fy, dz = fz;
            m[0] += 1.0;
            m[1] += dx; m[2] += dy; m[3] += dz;
            m[4] += dx * dx; m[5] += dx * dy; m[6] += dx * dz;
            m[7] += dy * dy; m[8] += dy * dz; m[9] += dz * dz;
        }
    }
#pragma unroll
    for (int k = 0; k < kNrmTerms; ++k)
#pragma unroll
        for (int o = kLpp / 2; o > 0; o >>= 1) m[k] += __shfl_xor(m[k], o, 64);
    const bool lead = live && sub == 0;
    bool ok = false;
    if (lead) {
        double n[3] = {0.0, 0.0, 0.0};
        if (m[0] >= 3.0) {
            ok = true;
            const double inv = 1.0 / m[0];
            const double mx = m[1] * inv, my = m[2] * inv, mz = m[3] * inv;
            double C[3][3], w[3], V[3][3];
            C[0][0] = m[4] * inv - mx * mx; C[0][1] = m[5] * inv - mx * my;
            C[0][2] = m[6] * inv - mx * mz; C[1][1] = m[7] * inv - my * my;
            C[1][2] = m[8] * inv - my * mz; C[2][2] = m[9] * inv - mz * mz;
            C[1][0] = C[0][1]; C[2][0] = C[0][2]; C[2][1] = C[1][2];
            sym3_eigen(C, w, V);
            int lo = 0;                                    // the lowest index on a tie
            if (w[1] < w[lo]) lo = 1;
            if (w[2] < w[lo]) lo = 2;
            const double len = sqrt(V[0][lo] * V[0][lo] + V[1][lo] * V[1][lo] + V[2][lo] * V[2][lo]);
            for (int d = 0; d < 3; ++d) n[d] = V[d][lo] / len;
            const double vx = view ? (double)view[3 * c] : 0.0, vy = view ? (double)view[3 * c + 1] : 0.0,
                         vz = view ? (double)view[3 * c + 2] : 0.0;
            const double dot = (n[0] * (vx - (double)px) + n[1] * (vy - (double)py)) + n[2] * (vz - (double)pz);
            bool flip = dot < 0.0;
            if (dot == 0.0) {
                const double first = n[0] != 0.0 ? n[0] : (n[1] != 0.0 ? n[1] : n[2]);
                flip = first < 0.0;
            }
            if (flip)
                for (int d = 0; d < 3; ++d) n[d] = -n[d];
        }
        for (int d = 0; d < 3; ++d) normals[3 * i + d] = (float)n[d];
    }
    // the count of valid normals: the lanes of a wave that share a cloud add once
    unsigned long long todo = __ballot(ok);
    const int lane = threadIdx.x % 64;
    while (todo) {
        const int first = __ffsll((long long)todo) - 1;
        const int cf = __shfl(c, first, 64);
        const unsigned long long same = __ballot(ok && c == cf) & todo;
        if (lane == first) atomicAdd(&n_valid[cf], __popcll(same));
        todo &= ~same;
    }
}

struct NormalsWs {
    RGridWs grid;
    int* sorted;
    size_t total;
};

void carve_normals(void* ws, int64_t n_tot, int32_t n_clouds, NormalsWs* w) {
    carve_rgrid(ws, n_tot, n_clouds, &w->grid);
    char* p = static_cast<char*>(ws);
    size_t o = w->grid.total;
    auto take = [&](size_t bytes) { void* r = p ? p + o : nullptr; o += align_up(bytes); return r; };
    w->sorted = (int*)take(4 * n_tot);
    w->total = o;
}

// the limits of icp.hip's icp_sizes_ok, for one packed cloud set
bool normals_sizes_ok(int64_t n_tot, int32_t n_clouds) {
    return n_clouds > 0 && n_clouds <= 65535 && n_tot >= 0 &&
           4 * n_tot + 1024ll * n_clouds < (1ll << 31) - 1;
}

}  // namespace
}  // namespace fgr

using namespace fgr;

extern "C" int fgr_estimate_normals_workspace(int64_t n_tot, int32_t n_clouds, size_t* bytes) {
    FGR_REQUIRE(bytes && normals_sizes_ok(n_tot, n_clouds),
                "fgr_estimate_normals_workspace: bad arguments");
    NormalsWs w;
    carve_normals(nullptr, n_tot, n_clouds, &w);
    *bytes = w.total;
    return FGR_OK;
}

extern "C" int fgr_estimate_normals(const float* pts, const int64_t* off, int64_t n_tot,
                                    int32_t n_clouds, float radius, const float* view, void* ws,
                                    size_t ws_bytes, float* normals, int32_t* n_valid,
                                    void* stream) {
    FGR_REQUIRE(normals_sizes_ok(n_tot, n_clouds) && off && ws && n_valid &&
                    ((pts && normals) || n_tot == 0) && radius > 0.f && radius < INFINITY,
                "fgr_estimate_normals: bad arguments (n_clouds %d radius %g)", n_clouds,
                (double)radius);
    NormalsWs w;
    carve_normals(ws, n_tot, n_clouds, &w);
    if (w.total > ws_bytes) {
        set_error("fgr_estimate_normals: workspace %zu < %zu bytes", ws_bytes, w.total);
        return FGR_E_WORKSPACE;
    }
    hipStream_t st = as_stream(stream);
    TimedCall timed_(st);
    hipLaunchKernelGGL(normals_init_kernel, dim3((unsigned)ceil_div(n_clouds, 256)), dim3(256), 0,
                       st, n_valid, n_clouds);
    FGR_CHECK_LAUNCH("normals_init_kernel");
    if (n_tot == 0) return FGR_OK;
    int rc = launch_rgrid_build(pts, off, n_clouds, n_tot, radius, w.grid, st);
    if (rc != FGR_OK) return rc;
    hipLaunchKernelGGL(cell_rank_kernel, dim3((unsigned)ceil_div(n_tot, 256)), dim3(256), 0, st,
                       n_tot, w.grid.cellof, w.grid.start, w.grid.members, w.sorted);
    FGR_CHECK_LAUNCH("cell_rank_kernel");
    hipLaunchKernelGGL(normals_kernel, dim3((unsigned)ceil_div(n_tot, kNrmPts)), dim3(kNrmThreads),
                       0, st, pts, off, (int)n_clouds, n_tot, w.grid.grids, w.grid.start, w.sorted,
                       view, radius * radius, normals, n_valid);
    FGR_CHECK_LAUNCH("normals_kernel");
    return FGR_OK;
}
