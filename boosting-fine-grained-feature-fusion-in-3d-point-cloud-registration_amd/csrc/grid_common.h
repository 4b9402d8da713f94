// Helpers shared by the geometry kernels of grid.hip (dense counting sorts),
// grid_sparse.hip (radix-sorted voxel keys) and icp.hip (nearest-neighbour association): the
// device-wide exclusive scan, the per-cloud bounding box, the voxel grid descriptor and the
// cell-binned support grid of the radius search with its build. Everything has internal
// linkage: each translation unit that includes this header compiles its own copy.
#pragma once
#include "common.h"

namespace fgr {

namespace {

typedef unsigned long long u64;

// ------------------------------------------------------------------------------------------
// device-wide exclusive scan of int32 counters (3 launches), optionally dual: the second
// component counts the non-zero counters (the voxel ordinal)
// ------------------------------------------------------------------------------------------
constexpr int kSB = 256, kSI = 16, kST = kSB * kSI;

__device__ __forceinline__ int2 add2(int2 a, int2 b) { return make_int2(a.x + b.x, a.y + b.y); }

__device__ __forceinline__ int2 wave_incl_scan2(int2 v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int tx = __shfl_up(v.x, o, 64), ty = __shfl_up(v.y, o, 64);
        if (lane >= o) { v.x += tx; v.y += ty; }
    }
    return v;
}

// 256-thread block exclusive scan of int2; *tot = the block total (all threads)
__device__ __forceinline__ int2 block_excl_scan2(int2 v, int2* tot) {
    __shared__ int2 wsum[kSB / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int2 inc = wave_incl_scan2(v, lane);
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    int2 pre = make_int2(0, 0), all = make_int2(0, 0);
#pragma unroll
    for (int i = 0; i < kSB / 64; ++i) {
        if (i < w) pre = add2(pre, wsum[i]);
        all = add2(all, wsum[i]);
    }
    __syncthreads();
    *tot = all;
    return make_int2(pre.x + inc.x - v.x, pre.y + inc.y - v.y);
}

// n = *n_dev (device-side element count) when n_dev, else n_static; element n itself reads as
// 0, so the exclusive scan's entry n is the total.
__device__ __forceinline__ int64_t scan_n(const int64_t* n_dev, int64_t n_static) {
    return n_dev ? *n_dev : n_static;
}

template <bool DUAL>
__global__ void __launch_bounds__(kSB) scan_tile_kernel(const int* __restrict__ in,
                                                        const int64_t* __restrict__ n_dev,
                                                        int64_t n_static, int2* __restrict__ tiles) {
    const int64_t n = scan_n(n_dev, n_static);
    const int64_t base = (int64_t)blockIdx.x * kST;
    int2 s = make_int2(0, 0);
    if (base <= n) {
#pragma unroll 4
        for (int k = 0; k < kSI; ++k) {
            const int64_t i = base + k * kSB + threadIdx.x;
            const int v = i < n ? in[i] : 0;
            s.x += v;
            if (DUAL) s.y += v > 0 ? 1 : 0;
        }
    }
    int2 tot;
    block_excl_scan2(s, &tot);
    if (threadIdx.x == 0) tiles[blockIdx.x] = tot;
}

// one block: tile totals -> exclusive tile offsets, in place
__global__ void __launch_bounds__(kSB) scan_offsets_kernel(int2* __restrict__ tiles, int ntiles) {
    int2 carry = make_int2(0, 0);
    for (int b0 = 0; b0 < ntiles; b0 += kSB) {
        const int i = b0 + threadIdx.x;
        const int2 v = i < ntiles ? tiles[i] : make_int2(0, 0);
        int2 tot;
        const int2 ex = block_excl_scan2(v, &tot);
        if (i < ntiles) tiles[i] = add2(ex, carry);
        carry = add2(carry, tot);
    }
}

// io[i] <- exclusive prefix (in place) for i in [0, n]; ord[i] <- exclusive count of non-zero.
// RAW: `tiles` holds the raw tile totals (at most kSB tiles) and each block sums those before
// its own (one load per thread and a block reduction) -- the scan without its one-block
// offsets launch; else `tiles` holds the exclusive tile offsets (scan_offsets_kernel)
template <bool DUAL, bool RAW = false>
__global__ void __launch_bounds__(kSB) scan_final_kernel(int* __restrict__ io, int* __restrict__ ord,
                                                         const int64_t* __restrict__ n_dev,
                                                         int64_t n_static,
                                                         const int2* __restrict__ tiles) {
    const int64_t n = scan_n(n_dev, n_static);
    const int64_t base = (int64_t)blockIdx.x * kST;
    if (base > n) return;                                   // block-uniform
    int2 carry;
    if constexpr (RAW) {
        const int2 v = (int)threadIdx.x < (int)blockIdx.x ? tiles[threadIdx.x] : make_int2(0, 0);
        block_excl_scan2(v, &carry);                        // carry = the sum over earlier tiles
    } else {
        carry = tiles[blockIdx.x];
    }
    for (int k = 0; k < kSI; ++k) {
        const int64_t i = base + k * kSB + threadIdx.x;
        const int v = i < n ? io[i] : 0;
        int2 tot;
        const int2 ex = block_excl_scan2(make_int2(v, DUAL ? (v > 0 ? 1 : 0) : 0), &tot);
        if (i <= n) {
            io[i] = carry.x + ex.x;
            if (DUAL) ord[i] = carry.y + ex.y;
        }
        carry = add2(carry, tot);
    }
}

int scan_tiles(int64_t n_max) { return (int)ceil_div(n_max + 1, kST); }

template <bool DUAL>
int launch_scan(int* io, int* ord, const int64_t* n_dev, int64_t n_max, int2* tiles,
                hipStream_t st) {
    const int nt = scan_tiles(n_max);
    hipLaunchKernelGGL(scan_tile_kernel<DUAL>, dim3(nt), dim3(kSB), 0, st, io, n_dev, n_max, tiles);
    FGR_CHECK_LAUNCH("scan_tile_kernel");
    if (nt <= kSB) {                                 // <= 1M counters: two launches
        hipLaunchKernelGGL((scan_final_kernel<DUAL, true>), dim3(nt), dim3(kSB), 0, st, io, ord, n_dev,
                           n_max, tiles);
        FGR_CHECK_LAUNCH("scan_final_kernel");
        return FGR_OK;
    }
    hipLaunchKernelGGL(scan_offsets_kernel, dim3(1), dim3(kSB), 0, st, tiles, nt);
    FGR_CHECK_LAUNCH("scan_offsets_kernel");
    hipLaunchKernelGGL(scan_final_kernel<DUAL>, dim3(nt), dim3(kSB), 0, st, io, ord, n_dev, n_max,
                       tiles);
    FGR_CHECK_LAUNCH("scan_final_kernel");
    return FGR_OK;
}

// per-cloud min / max of xyz (256 threads, one block per cloud); valid in thread 0
// bounding box of pts[b, e) over the whole block (<= 1024 threads); every thread keeps 4
// points' loads in flight per round (the loop is latency-bound: one block per cloud)
__device__ __forceinline__ void block_bbox(const float* __restrict__ pts, int64_t b, int64_t e,
                                           float mn[3], float mx[3]) {
    mn[0] = mn[1] = mn[2] = INFINITY;
    mx[0] = mx[1] = mx[2] = -INFINITY;
    const int64_t bs = blockDim.x;
    for (int64_t i0 = b + threadIdx.x; i0 < e; i0 += 4 * bs) {
        float v[4][3];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t i = i0 + u * bs;
            const int64_t ic = i < e ? i : i0;              // i0 < e: always a valid point
#pragma unroll
            for (int d = 0; d < 3; ++d) v[u][d] = pts[3 * ic + d];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                mn[d] = fminf(mn[d], v[u][d]);
                mx[d] = fmaxf(mx[d], v[u][d]);
            }
    }
    __shared__ float red[2][3][16];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        for (int o = 32; o > 0; o >>= 1) {
            mn[d] = fminf(mn[d], __shfl_xor(mn[d], o, kWave));
            mx[d] = fmaxf(mx[d], __shfl_xor(mx[d], o, kWave));
        }
    }
    const int w = threadIdx.x / kWave, l = threadIdx.x % kWave, nw = (int)(bs / kWave);
    if (l == 0)
        for (int d = 0; d < 3; ++d) { red[0][d][w] = mn[d]; red[1][d][w] = mx[d]; }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int d = 0; d < 3; ++d) {
            mn[d] = red[0][d][0];
            mx[d] = red[1][d][0];
            for (int k = 1; k < nw; ++k) {
                mn[d] = fminf(mn[d], red[0][d][k]);
                mx[d] = fmaxf(mx[d], red[1][d][k]);
            }
        }
}

struct DGrid {
    float org[3];
    int pad;
    u64 nx, ny;
    long long base, cells;          // first counter of the cloud, its key-space size
};

constexpr long long kHuge = 1ll << 62;

size_t align_up(size_t x) { return (x + 255) & ~size_t(255); }

// ------------------------------------------------------------------------------------------
// the cell-binned support grid of the radius search (grid.hip) and of the ICP association
// (icp.hip): descriptor, counting-sort build and the distance both rank by
// ------------------------------------------------------------------------------------------
struct RGrid {
    float org[3];
    float cell;
    int nx, ny, nz;
    float radius;                   // the radius the grid was built for (queries use <= it)
    long long base;                 // first cell counter of the cloud (= 4 s_off[c] + 1024 c)
};

__host__ __device__ inline long long rgrid_cap(int64_t n_c) { return 4 * n_c + 1024; }

// blocks >= n_clouds zero the cell starts (4096 each), as dgrid_bbox_kernel
__global__ void __launch_bounds__(1024) rgrid_bbox_kernel(const float* __restrict__ s,
                                                         const int64_t* __restrict__ s_off,
                                                         float radius, RGrid* __restrict__ grids,
                                                         int n_clouds, int* __restrict__ zero,
                                                         int64_t n_zero) {
    const int c = blockIdx.x;
    if (c >= n_clouds) {                                   // block-uniform
        const int64_t z0 = (int64_t)(c - n_clouds) * 4096;
        for (int64_t i = z0 + threadIdx.x; i < min(z0 + 4096, n_zero); i += 1024) zero[i] = 0;
        return;
    }
    const int64_t b = s_off[c], e = s_off[c + 1];
    float mn[3], mx[3];
    block_bbox(s, b, e, mn, mx);
    if (threadIdx.x != 0) return;
    RGrid g;
    g.radius = radius;
    g.base = 4 * b + 1024ll * c;
    if (e <= b) {
        g.org[0] = g.org[1] = g.org[2] = 0.f;
        g.cell = radius;
        g.nx = g.ny = g.nz = 1;
    } else {
        const long long cap = rgrid_cap(e - b);
        float cell = radius * 1.0625f;
        long long d[3];
        for (int it = 0; it < 200; ++it) {
            for (int k = 0; k < 3; ++k) d[k] = (long long)floorf((mx[k] - mn[k]) / cell) + 1;
            if (d[0] * d[1] * d[2] <= cap && d[0] <= 65536 && d[1] <= 65536 && d[2] <= 65536) break;
            cell *= 1.25f;
        }
        for (int k = 0; k < 3; ++k) g.org[k] = mn[k];
        g.cell = cell;
        g.nx = (int)d[0];
        g.ny = (int)d[1];
        g.nz = (int)d[2];
    }
    grids[c] = g;
}

__device__ __forceinline__ int cell_coord(float x, float org, float cell) {
    return (int)floorf((x - org) / cell);
}

__global__ void rgrid_key_kernel(const float* __restrict__ s, const int64_t* __restrict__ s_off,
                                 int n_clouds, int64_t ns, const RGrid* __restrict__ grids,
                                 int* __restrict__ hist, int* __restrict__ cellof,
                                 int* __restrict__ slot) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ns) return;
    const int c = find_segment(s_off, n_clouds, i);
    const RGrid g = grids[c];
    const int x = min(max(cell_coord(s[3 * i], g.org[0], g.cell), 0), g.nx - 1);
    const int y = min(max(cell_coord(s[3 * i + 1], g.org[1], g.cell), 0), g.ny - 1);
    const int z = min(max(cell_coord(s[3 * i + 2], g.org[2], g.cell), 0), g.nz - 1);
    const int cell = (int)(g.base + ((long long)z * g.ny + y) * g.nx + x);
    cellof[i] = cell;
    slot[i] = atomicAdd(&hist[cell], 1);
}

__global__ void rgrid_scatter_kernel(int64_t ns, const int* __restrict__ cellof,
                                     const int* __restrict__ slot, const int* __restrict__ start,
                                     int* __restrict__ members) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ns) return;
    members[start[cellof[i]] + slot[i]] = (int)i;
}

// d2 exactly as nanoflann's L2_Simple_Adaptor::evalMetric (and geom.hip's dist2)
__device__ __forceinline__ float dist2g(float qx, float qy, float qz, float sx, float sy, float sz) {
    float dx = qx - sx, dy = qy - sy, dz = qz - sz;
    float d2 = dx * dx;
    d2 = d2 + dy * dy;
    d2 = d2 + dz * dz;
    return d2;
}

struct RGridWs {
    RGrid* grids;
    int* start;
    int2* tiles;
    int *cellof, *slot, *members;
    size_t total;
};

void carve_rgrid(void* ws, int64_t ns, int32_t nc, RGridWs* g) {
    char* p = static_cast<char*>(ws);
    size_t o = 0;
    auto take = [&](size_t bytes) { void* r = p ? p + o : nullptr; o += align_up(bytes); return r; };
    const int64_t cap = 4 * ns + 1024ll * nc;
    g->grids = (RGrid*)take(sizeof(RGrid) * nc);
    g->start = (int*)take(4 * (cap + 1));
    g->tiles = (int2*)take(sizeof(int2) * scan_tiles(cap));
    g->cellof = (int*)take(4 * ns);
    g->slot = (int*)take(4 * ns);
    g->members = (int*)take(4 * ns);
    g->total = o;
}

// bins the supports s (ns rows, n_clouds segments) into the carved grid g at `radius`
int launch_rgrid_build(const float* s, const int64_t* s_off, int32_t n_clouds, int64_t ns,
                       float radius, const RGridWs& g, hipStream_t st) {
    const int64_t cap = 4 * ns + 1024ll * n_clouds;
    hipLaunchKernelGGL(rgrid_bbox_kernel, dim3((unsigned)(n_clouds + ceil_div(cap + 1, 4096))),
                       dim3(1024), 0, st, s, s_off, radius, g.grids, n_clouds, g.start,
                       (int64_t)(cap + 1));
    FGR_CHECK_LAUNCH("rgrid_bbox_kernel");
    if (ns > 0) {
        hipLaunchKernelGGL(rgrid_key_kernel, dim3((unsigned)ceil_div(ns, 256)), dim3(256), 0, st, s,
                           s_off, n_clouds, ns, g.grids, g.start, g.cellof, g.slot);
        FGR_CHECK_LAUNCH("rgrid_key_kernel");
    }
    int rc = launch_scan<false>(g.start, nullptr, nullptr, cap, g.tiles, st);
    if (rc != FGR_OK) return rc;
    if (ns > 0) {
        hipLaunchKernelGGL(rgrid_scatter_kernel, dim3((unsigned)ceil_div(ns, 256)), dim3(256), 0,
                           st, ns, g.cellof, g.slot, g.start, g.members);
        FGR_CHECK_LAUNCH("rgrid_scatter_kernel");
    }
    return FGR_OK;
}

}  // namespace
}  // namespace fgr
