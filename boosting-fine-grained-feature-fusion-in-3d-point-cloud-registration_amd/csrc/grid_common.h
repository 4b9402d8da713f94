// Helpers shared by the geometry kernels of grid.hip (dense counting sorts) and
// grid_sparse.hip (radix-sorted voxel keys): the device-wide exclusive scan, the per-cloud
// bounding box and the voxel grid descriptor. Everything has internal linkage: each
// translation unit that includes this header compiles its own copy.
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

}  // namespace
}  // namespace fgr
