// Grid subsampling of large-extent clouds on gfx950: voxel keys sorted by a stable radix sort
// instead of counted in a dense histogram (grid.hip), so memory and time follow the number of
// points and not the bounding box.
//
// Same semantics as the dense path and oracle/geom_oracle.c, bit for bit (grid_subsampling.cpp:
// 5-106): per cloud the origin is floor(min/dl)*dl, the voxel key ix + nx iy + nx ny iz is
// formed with the fp32 expressions of dgrid_key_kernel, voxels come out in ascending key order
// per cloud with the clouds end to end, and each barycentre sums its members in ascending point
// index and multiplies by (float)(1.0/(double)cnt).
//
//   1. sgrid_bbox_kernel / sgrid_base_kernel: per-cloud grid (DGrid) and base[c], the running
//      sum of the earlier clouds' key spaces; the GLOBAL key of a point is base[c] + key, so one
//      sort orders all clouds at once and cloud c's points land at sorted positions
//      [off[c], off[c + 1]).
//   2. One least-significant-digit radix sort of (global key, point index) over all points:
//      8-bit digits, and only as many passes as the summed key space has bytes. A pass is a
//      per-block digit histogram (kRT items per block, stored digit-major), the device-wide
//      exclusive scan of grid_common.h over it, and a scatter that ranks an item among the
//      block's earlier items of the same digit by wave ballots (a 64-bit match mask per lane,
//      popcount of the lanes below) plus per-wave digit counts in LDS. Every pass is stable and
//      the first one starts from ascending point index, so after the last pass a voxel's
//      members are contiguous AND in ascending point index: the barycentre kernel sums them
//      sequentially, with no insertion sort or min-selection. No result depends on the
//      arrival order of an atomic (the LDS histogram's atomic adds only count).
//   3. Voxel heads: sorted key != its left neighbour; an exclusive scan of the head flags gives
//      every voxel's ordinal, the per-cloud counts (differences at off[c]) and the total.
//
// Limits are reported through counts[n_clouds] < 0, never truncated (fgreg.h lists the codes):
//   -1  a cloud has more than 2^20 voxels along an axis (the `big` test of dgrid_bbox_kernel),
//   -2  the clouds' summed key space reaches 2^62,
//   -3  the caller's key_bits hint is smaller than the summed key space needs.
// n_points >= 2^31 is an argument error (point indices and scan offsets are int32).
// The host launches the passes its key_bits hint allows (0 = all eight); the device computes
// the pass count from the summed key space (ctl[2]) and passes beyond it return at once, so
// the sorted arrays end in buffer A when that count is even and in B when it is odd.
// Built with -ffp-contract=off like grid.hip: keys and barycentres round as written.
#include "common.h"
#include "grid_common.h"

namespace fgr {

namespace {

constexpr int kRB = 256;             // threads per sort block
constexpr int kRI = 4;               // items per thread
constexpr int kRT = kRB * kRI;       // items per sort block (fgreg.ops.GRID_SPARSE_TILE)
constexpr int kMaxPass = 8;

enum { kErrAxis = -1, kErrSpace = -2, kErrBits = -3 };

// one block per cloud: the cloud's grid, exactly as dgrid_bbox_kernel (cells = kHuge marks a
// cloud with more than 2^20 voxels along an axis)
__global__ void __launch_bounds__(1024) sgrid_bbox_kernel(const float* __restrict__ pts,
                                                         const int64_t* __restrict__ off, float dl,
                                                         DGrid* __restrict__ grids) {
    const int c = blockIdx.x;
    const int64_t b = off[c], e = off[c + 1];
    float mn[3], mx[3];
    block_bbox(pts, b, e, mn, mx);
    if (threadIdx.x != 0) return;
    DGrid g;
    g.pad = 0;
    g.base = 0;
    if (e <= b) {
        g.org[0] = g.org[1] = g.org[2] = 0.f;
        g.nx = g.ny = 1;
        g.cells = 0;
    } else {
        // origin and dims exactly as grid_subsampling.cpp:25-31
        const float inv = 1.0f / dl;
        long long dims[3];
        for (int d = 0; d < 3; ++d) {
            g.org[d] = floorf(mn[d] * inv) * dl;
            dims[d] = (long long)floorf((mx[d] - g.org[d]) / dl) + 1;
        }
        g.nx = (u64)dims[0];
        g.ny = (u64)dims[1];
        const bool big = dims[0] > (1 << 20) || dims[1] > (1 << 20) || dims[2] > (1 << 20);
        g.cells = big ? kHuge : dims[0] * dims[1] * dims[2];
    }
    grids[c] = g;
}

// ctl[0] = status (0, or the negative code counts[n_clouds] reports), ctl[1] = the summed key
// space, ctl[2] = radix passes that key space needs (the bytes of its largest key)
__global__ void sgrid_base_kernel(DGrid* __restrict__ grids, int n_clouds, int host_passes,
                                  int64_t* __restrict__ ctl) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    long long b = 0, status = 0;
    for (int c = 0; c < n_clouds; ++c) {
        const long long cells = grids[c].cells;
        grids[c].base = b;
        if (cells >= kHuge) {                       // dims <= 2^20 each: a product is <= 2^60
            if (status == 0) status = kErrAxis;
        } else if (b >= kHuge - cells) {
            if (status == 0) status = kErrSpace;
            b = kHuge;
        } else {
            b += cells;
        }
    }
    int bits = 0;
    if (status == 0 && b > 1) bits = 64 - __clzll(b - 1);
    const int passes = (bits + 7) / 8;
    if (status == 0 && passes > host_passes) status = kErrBits;
    ctl[0] = status;
    ctl[1] = b;
    ctl[2] = status == 0 ? passes : 0;
}

__global__ void sgrid_key_kernel(const float* __restrict__ pts, const int64_t* __restrict__ off,
                                 int n_clouds, int64_t n, float dl, const DGrid* __restrict__ grids,
                                 const int64_t* __restrict__ ctl, u64* __restrict__ keys,
                                 int* __restrict__ vals) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || ctl[0] != 0) return;
    const int c = find_segment(off, n_clouds, i);
    const DGrid g = grids[c];
    // key exactly as grid_subsampling.cpp:53-56 (grid.hip dgrid_key_kernel)
    const u64 ix = (u64)(long long)floorf((pts[3 * i] - g.org[0]) / dl);
    const u64 iy = (u64)(long long)floorf((pts[3 * i + 1] - g.org[1]) / dl);
    const u64 iz = (u64)(long long)floorf((pts[3 * i + 2] - g.org[2]) / dl);
    const u64 key = ix + g.nx * iy + g.nx * g.ny * iz;
    keys[i] = (u64)g.base + key;
    vals[i] = (int)i;
}

// pass `pass` reads buffer A when it is even and B when it is odd
__device__ __forceinline__ bool pass_active(const int64_t* ctl, int pass) {
    return ctl[0] == 0 && (int64_t)pass < ctl[2];
}

// hist[d * n_blocks + b] = items of block b whose digit is d; every entry is written
__global__ void __launch_bounds__(kRB) ssort_hist_kernel(const int64_t* __restrict__ ctl, int pass,
                                                        int64_t n, int n_blocks,
                                                        const u64* __restrict__ ka,
                                                        const u64* __restrict__ kb,
                                                        int* __restrict__ hist) {
    if (!pass_active(ctl, pass)) return;                     // grid-uniform
    const u64* __restrict__ src = (pass & 1) ? kb : ka;
    __shared__ int h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * kRT;
    const int sh = 8 * pass;
#pragma unroll
    for (int k = 0; k < kRI; ++k) {
        const int64_t j = base + k * kRB + threadIdx.x;
        if (j < n) atomicAdd(&h[(int)((src[j] >> sh) & 255)], 1);
    }
    __syncthreads();
    hist[(int64_t)threadIdx.x * n_blocks + blockIdx.x] = h[threadIdx.x];
}

// Stable scatter of one pass. Items of a block are taken in index order: round k, wave w, lane.
// dbase[d]: where the block's next item of digit d goes (the scanned histogram, advanced after
// every round); wc[w][d]: items of digit d in wave w of the current round.
__global__ void __launch_bounds__(kRB) ssort_scatter_kernel(const int64_t* __restrict__ ctl, int pass,
                                                           int64_t n, int n_blocks,
                                                           u64* __restrict__ ka, u64* __restrict__ kb,
                                                           int* __restrict__ va, int* __restrict__ vb,
                                                           const int* __restrict__ hist) {
    if (!pass_active(ctl, pass)) return;                     // grid-uniform
    const u64* __restrict__ sk = (pass & 1) ? kb : ka;
    const int* __restrict__ sv = (pass & 1) ? vb : va;
    u64* __restrict__ dk = (pass & 1) ? ka : kb;
    int* __restrict__ dv = (pass & 1) ? va : vb;
    __shared__ int dbase[256];
    __shared__ int wc[kRB / 64][256];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    dbase[tid] = hist[(int64_t)tid * n_blocks + blockIdx.x];
#pragma unroll
    for (int i = 0; i < kRB / 64; ++i) wc[i][tid] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * kRT;
    const int sh = 8 * pass;
    const u64 lt_mask = (1ull << lane) - 1ull;
    for (int k = 0; k < kRI; ++k) {
        const int64_t j = base + k * kRB + tid;
        const bool valid = j < n;
        const u64 key = valid ? sk[j] : 0ull;
        const int val = valid ? sv[j] : 0;
        const int d = (int)((key >> sh) & 255);
        // lanes of this wave that hold a valid item of the same digit (every lane votes)
        u64 mask = __ballot(valid);
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            const bool set = (d >> bit) & 1;
            const u64 bal = __ballot(set);
            mask &= set ? bal : ~bal;
        }
        const int rank = __popcll(mask & lt_mask);
        if (valid && rank == 0) wc[w][d] = __popcll(mask);
        __syncthreads();
        if (valid) {
            int pos = dbase[d] + rank;
            for (int i = 0; i < w; ++i) pos += wc[i][d];
            dk[pos] = key;
            dv[pos] = val;
        }
        __syncthreads();
        int s = 0;
#pragma unroll
        for (int i = 0; i < kRB / 64; ++i) {
            s += wc[i][tid];
            wc[i][tid] = 0;
        }
        dbase[tid] += s;
        __syncthreads();
    }
}

__device__ __forceinline__ bool sorted_in_b(const int64_t* ctl) { return (ctl[2] & 1) != 0; }

// head[i] = 1 where sorted position i starts a voxel (then scanned in place)
__global__ void sgrid_head_kernel(const int64_t* __restrict__ ctl, int64_t n,
                                  const u64* __restrict__ ka, const u64* __restrict__ kb,
                                  int* __restrict__ head) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (ctl[0] != 0) { head[i] = 0; return; }
    const u64* __restrict__ k = sorted_in_b(ctl) ? kb : ka;
    head[i] = (i == 0 || k[i] != k[i - 1]) ? 1 : 0;
}

// ord = the exclusive scan of the head flags, entries [0, n]. Thread i < n: a head writes its
// voxel's start and per-cloud key; thread c <= n_clouds: the counts.
__global__ void sgrid_count_kernel(const DGrid* __restrict__ grids, const int64_t* __restrict__ off,
                                   int n_clouds, int64_t n, const int64_t* __restrict__ ctl,
                                   const u64* __restrict__ ka, const u64* __restrict__ kb,
                                   const int* __restrict__ ord, int64_t* __restrict__ counts,
                                   int* __restrict__ vstart, u64* __restrict__ vkey) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t status = ctl[0];
    if (i <= n_clouds) {
        if (status != 0) counts[i] = i < n_clouds ? 0 : status;
        else if (i < n_clouds) counts[i] = (int64_t)ord[off[i + 1]] - ord[off[i]];
        else {
            const int m = ord[n];
            counts[n_clouds] = m;
            vstart[m] = (int)n;
        }
    }
    if (i >= n || status != 0) return;
    const int v = ord[i];
    if (ord[i + 1] == v) return;                            // not a head
    const u64* __restrict__ k = sorted_in_b(ctl) ? kb : ka;
    const int c = find_segment(off, n_clouds, i);           // cloud c sorts into [off[c], off[c+1])
    vstart[v] = (int)i;
    vkey[v] = k[i] - (u64)grids[c].base;
}

// Barycentre per voxel: its members are contiguous and in ascending point index (the
// reference's input order, grid_subsampling.cpp:70, 87)
__global__ void sgrid_fill_kernel(const float* __restrict__ pts, const int64_t* __restrict__ ctl,
                                  const int* __restrict__ va, const int* __restrict__ vb,
                                  const int* __restrict__ vstart, const u64* __restrict__ vkey,
                                  int64_t n_out, float* __restrict__ out,
                                  int64_t* __restrict__ out_keys) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n_out || ctl[0] != 0) return;
    const int* __restrict__ vals = sorted_in_b(ctl) ? vb : va;
    const int b = vstart[v], e = vstart[v + 1], cnt = e - b;
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (int j = b; j < e; ++j) {
        const int p = vals[j];
        sx += pts[3 * p];
        sy += pts[3 * p + 1];
        sz += pts[3 * p + 2];
    }
    const float s = (float)(1.0 / (double)cnt);
    out[3 * v] = sx * s;
    out[3 * v + 1] = sy * s;
    out[3 * v + 2] = sz * s;
    if (out_keys) out_keys[v] = (int64_t)vkey[v];
}

struct SGridWs {
    DGrid* grids;
    int64_t* ctl;
    u64 *ka, *kb, *vkey;
    int *va, *vb, *hist, *ord, *vstart;
    int2* tiles;
    size_t total;
};

int64_t sort_blocks(int64_t n) { return ceil_div(n, kRT); }

// depends on n and nc only, never on the clouds' extent
void carve_sparse(void* ws, int64_t n, int32_t nc, SGridWs* g) {
    char* p = static_cast<char*>(ws);
    size_t o = 0;
    auto take = [&](size_t bytes) { void* r = p ? p + o : nullptr; o += align_up(bytes); return r; };
    const int64_t nh = 256 * sort_blocks(n);
    g->grids = (DGrid*)take(sizeof(DGrid) * nc);
    g->ctl = (int64_t*)take(4 * sizeof(int64_t));
    g->ka = (u64*)take(8 * n);
    g->kb = (u64*)take(8 * n);
    g->vkey = (u64*)take(8 * n);
    g->va = (int*)take(4 * n);
    g->vb = (int*)take(4 * n);
    g->hist = (int*)take(4 * (nh + 1));
    g->ord = (int*)take(4 * (n + 1));
    g->vstart = (int*)take(4 * (n + 1));
    g->tiles = (int2*)take(sizeof(int2) * scan_tiles(nh > n ? nh : n));
    g->total = o;
}

}  // namespace
}  // namespace fgr

using namespace fgr;

extern "C" int fgr_grid_subsample_sparse_workspace(int64_t n_points, int32_t n_clouds,
                                                   size_t* bytes) {
    FGR_REQUIRE(bytes && n_points >= 0 && n_clouds > 0 && n_points < (1ll << 31),
                "fgr_grid_subsample_sparse_workspace: bad arguments");
    SGridWs g;
    carve_sparse(nullptr, n_points, n_clouds, &g);
    *bytes = g.total;
    return FGR_OK;
}

extern "C" int fgr_grid_subsample_sparse_count(const float* points, const int64_t* off,
                                               int32_t n_clouds, int64_t n_points, float dl,
                                               int32_t key_bits, void* ws, size_t ws_bytes,
                                               int64_t* counts, void* stream) {
    FGR_REQUIRE(off && counts && ws && n_clouds > 0 && n_points >= 0 && dl > 0.f &&
                    (points || n_points == 0) && n_points < (1ll << 31) && key_bits >= 0 &&
                    key_bits <= 62,
                "fgr_grid_subsample_sparse_count: bad arguments");
    SGridWs g;
    carve_sparse(ws, n_points, n_clouds, &g);
    if (g.total > ws_bytes) {
        set_error("fgr_grid_subsample_sparse_count: workspace %zu < %zu bytes", ws_bytes, g.total);
        return FGR_E_WORKSPACE;
    }
    hipStream_t st = as_stream(stream);
    TimedCall timed_(st);
    const int64_t n = n_points;
    if (n == 0) {
        FGR_CHECK_HIP(hipMemsetAsync(counts, 0, sizeof(int64_t) * (n_clouds + 1), st));
        return FGR_OK;
    }
    const int passes = key_bits == 0 ? kMaxPass : (key_bits + 7) / 8;
    hipLaunchKernelGGL(sgrid_bbox_kernel, dim3((unsigned)n_clouds), dim3(1024), 0, st, points, off,
                       dl, g.grids);
    FGR_CHECK_LAUNCH("sgrid_bbox_kernel");
    hipLaunchKernelGGL(sgrid_base_kernel, dim3(1), dim3(64), 0, st, g.grids, n_clouds, passes,
                       g.ctl);
    FGR_CHECK_LAUNCH("sgrid_base_kernel");
    const unsigned nb = (unsigned)ceil_div(n, 256);
    hipLaunchKernelGGL(sgrid_key_kernel, dim3(nb), dim3(256), 0, st, points, off, n_clouds, n, dl,
                       g.grids, g.ctl, g.ka, g.va);
    FGR_CHECK_LAUNCH("sgrid_key_kernel");
    const int sb = (int)sort_blocks(n);
    for (int p = 0; p < passes; ++p) {
        hipLaunchKernelGGL(ssort_hist_kernel, dim3((unsigned)sb), dim3(kRB), 0, st, g.ctl, p, n, sb,
                           g.ka, g.kb, g.hist);
        FGR_CHECK_LAUNCH("ssort_hist_kernel");
        int rc = launch_scan<false>(g.hist, nullptr, nullptr, 256ll * sb, g.tiles, st);
        if (rc != FGR_OK) return rc;
        hipLaunchKernelGGL(ssort_scatter_kernel, dim3((unsigned)sb), dim3(kRB), 0, st, g.ctl, p, n,
                           sb, g.ka, g.kb, g.va, g.vb, g.hist);
        FGR_CHECK_LAUNCH("ssort_scatter_kernel");
    }
    hipLaunchKernelGGL(sgrid_head_kernel, dim3(nb), dim3(256), 0, st, g.ctl, n, g.ka, g.kb, g.ord);
    FGR_CHECK_LAUNCH("sgrid_head_kernel");
    int rc = launch_scan<false>(g.ord, nullptr, nullptr, n, g.tiles, st);
    if (rc != FGR_OK) return rc;
    const int64_t nt = n > n_clouds + 1 ? n : n_clouds + 1;
    hipLaunchKernelGGL(sgrid_count_kernel, dim3((unsigned)ceil_div(nt, 256)), dim3(256), 0, st,
                       g.grids, off, n_clouds, n, g.ctl, g.ka, g.kb, g.ord, counts, g.vstart,
                       g.vkey);
    FGR_CHECK_LAUNCH("sgrid_count_kernel");
    return FGR_OK;
}

extern "C" int fgr_grid_subsample_sparse_fill(int64_t n_points, int32_t n_clouds, int64_t n_out,
                                              void* ws, size_t ws_bytes, const float* points,
                                              float* out_points, int64_t* out_keys, void* stream) {
    FGR_REQUIRE(ws && n_clouds > 0 && n_points >= 0 && n_points < (1ll << 31) && n_out >= 0 &&
                    n_out <= n_points && ((out_points && points) || n_out == 0),
                "fgr_grid_subsample_sparse_fill: bad arguments");
    SGridWs g;
    carve_sparse(ws, n_points, n_clouds, &g);
    if (g.total > ws_bytes) {
        set_error("fgr_grid_subsample_sparse_fill: workspace %zu < %zu bytes", ws_bytes, g.total);
        return FGR_E_WORKSPACE;
    }
    hipStream_t st = as_stream(stream);
    TimedCall timed_(st);
    if (n_out == 0) return FGR_OK;
    hipLaunchKernelGGL(sgrid_fill_kernel, dim3((unsigned)ceil_div(n_out, 256)), dim3(256), 0, st,
                       points, g.ctl, g.va, g.vb, g.vstart, g.vkey, n_out, out_points, out_keys);
    FGR_CHECK_LAUNCH("sgrid_fill_kernel");
    return FGR_OK;
}
