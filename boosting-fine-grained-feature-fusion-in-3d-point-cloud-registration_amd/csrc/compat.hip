// Pose estimation from spatial compatibility, resident on the device: the estimator for
// correspondence sets with few inliers, where fgr_ransac_pose's uniform 3-point samples are
// almost never all-inlier. Two correct correspondences preserve the distance between their
// points, so the inliers form a dense clique of the compatibility graph; a seed from that
// clique and its most compatible neighbours give an all-inlier sample without a draw (the
// first- and second-order measure of SC2-PCR, reduced to its integer core). include/fgreg.h
// states the semantics; tests/_compat_ref.py restates them in numpy.
//
// Six launches, whatever the data:
// * ransac_prep_kernel (robust_parts.h): compacts the eligible rows, counts them into
//   n_eligible and records each rank's row index.
// * compat_bits_kernel, grid (64-row tile, pair): the first-order matrix SC as bits. The tile's
//   rows lie in LDS; a wave takes a word of 64 columns, ONE LANE PER COLUMN j, reads row i from
//   LDS (one address: a broadcast), and the wave ballot of |la - lb| < compat_dist IS the
//   64-bit word of row i. Lane i keeps it, so a wave stores 64 words at once. Also zeroes s.
// * compat_second_kernel, grid (column tile, row tile, pair): s_i = sum_j SC_ij c_ij with
//   c_ij = popcount(row_i & row_j), tiled like a GEMM over (64 rows i) x (64 rows j) x (16
//   words): both row tiles are staged in LDS at a stride of 17 words, a thread accumulates a
//   4 x 4 register block of c, masks it by the SC bits of its rows and adds the sums of its
//   rows -- reduced over 16 lanes -- to s_i with an integer atomic (order-independent).
//   LDS banking (ds_read_b64: bank (a / 4) % 64 within a 32-lane half): the 16 lanes of a
//   group read 16 consecutive j rows, 34 dwords apart -> banks {34 l, 34 l + 1} mod 64, all
//   distinct; rows of 16 words (32 dwords) would put them on two banks, 16-way. The i rows
//   are two addresses a half-wave, eight banks apart.
// * compat_top_kernel, one block per pair: the min(n_seeds, m) ranks with the largest
//   (s, lowest rank) by a bit-wise search for the threshold key, then each selected key's
//   position by counting the larger ones; seed_row and row_score.
// * compat_seed_kernel, grid (seed, pair): lists the seed's neighbours from its row of bits,
//   recomputes their c_ij (one lane per neighbour, the seed's row broadcast from LDS), finds
//   the top k - 1 packed (c, -j) keys by the same threshold search, sums the members' fp64
//   moments in a fixed order (the seed on thread 0, the chosen neighbours as per-thread
//   partials over the neighbour list, block_reduce's tree: reproducible, not rank order, which
//   only the fp64 rounding could see), solves on thread 0 and counts
//   d2 < r2 over all rows (rs_count). One RsSlot per seed.
// * ransac_select_kernel (robust_parts.h): selection, refits and outputs, as fgr_ransac_pose.
// Built with -ffp-contract=off: the distances, the transform and d2 round as written.
#include <cfloat>

#include "robust_parts.h"

namespace fgr {
namespace {

typedef unsigned long long u64;

constexpr int kCpMaxLen = 8192;                    // rows of a pair: s <= m^2 stays in int32
constexpr int kCpMaxSeeds = 1024;
constexpr int kCpMaxK = 256;
constexpr int kCpTile = 64;                        // rows of a tile = bits of a word
constexpr int kCpKW = 16;                          // words of a row per LDS stage
constexpr int kCpLd = kCpKW + 1;                   // padded LDS row stride, in words
constexpr int kCpRankBits = 14;                    // a rank < 8192 in a key's low bits
constexpr int kCpRankMask = (1 << kCpRankBits) - 1;
static_assert(kCpMaxLen <= (1 << (kCpRankBits - 1)), "ranks fit the key");
static_assert(kRsThreads == 256, "4 waves: 16 x 16 threads of 4 x 4 register blocks");

// words of a row of bits in the workspace: even (16-B loads), a function of max_len only
int cp_stride(int32_t max_len) {
    const int w = (max_len + 63) / 64;
    return w < 2 ? 2 : (w + 1) & ~1;
}

// the eligible rows of pair p as the later kernels see them: a pair above the caller's bound
// has no rows (nothing of it would fit the workspace), so it gets no seed
__device__ __forceinline__ int cp_m(const int32_t* n_eligible, int p, int max_len) {
    const int m = n_eligible[p];
    return m <= max_len ? m : 0;
}

// sum of an int over the block, in every thread; sh: kRsThreads / 64 ints; ends with a barrier
__device__ __forceinline__ int block_sum_int(int v, int* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (threadIdx.x % 64 == 0) sh[threadIdx.x / 64] = v;
    __syncthreads();
    int t = 0;
#pragma unroll
    for (int k = 0; k < kRsThreads / 64; ++k) t += sh[k];
    __syncthreads();
    return t;
}

__device__ __forceinline__ float cp_len(float dx, float dy, float dz) {
    return sqrtf((dx * dx + dy * dy) + dz * dz);
}

__global__ void __launch_bounds__(kRsThreads)
compat_bits_kernel(const float4* __restrict__ rows, const int64_t* __restrict__ off,
                   const int32_t* __restrict__ n_eligible, int max_len, int ld, float cdist,
                   u64* __restrict__ bits, int32_t* __restrict__ s) {
    __shared__ float4 tile[2 * kCpTile];
    const int p = blockIdx.y;
    const int m = cp_m(n_eligible, p, max_len);
    const int i0 = blockIdx.x * kCpTile;
    if (i0 >= m) return;                                   // block-uniform
    const int64_t beg = off[p];
    const float4* R0 = rows + 2 * beg;
    u64* B0 = bits + beg * ld;
    if (threadIdx.x < 2 * kCpTile) {
        const int r = threadIdx.x / 2;
        tile[threadIdx.x] = i0 + r < m ? R0[2 * (int64_t)i0 + threadIdx.x]
                                       : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (threadIdx.x < kCpTile && i0 + (int)threadIdx.x < m) s[beg + i0 + threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x % 64, wv = threadIdx.x / 64;
    const int W = (m + 63) / 64;
    for (int jw = wv; jw < W; jw += kRsThreads / 64) {     // wave-uniform
        const int j = jw * 64 + lane;
        float4 u = make_float4(0.f, 0.f, 0.f, 0.f), v = u;
        if (j < m) { u = R0[2 * (int64_t)j]; v = R0[2 * (int64_t)j + 1]; }
        u64 mine = 0;
#pragma unroll 4
        for (int ii = 0; ii < kCpTile; ++ii) {
            const float4 x = tile[2 * ii], y = tile[2 * ii + 1];       // a broadcast
            const float la = cp_len(x.x - u.x, x.y - u.y, x.z - u.z);
            const float lb = cp_len(x.w - u.w, y.x - v.x, y.y - v.y);
            const bool sc = j < m && j != i0 + ii && fabsf(la - lb) < cdist;   // a NaN: false
            const u64 bal = __ballot(sc);
            if (lane == ii) mine = bal;
        }
        if (i0 + lane < m) B0[(int64_t)(i0 + lane) * ld + jw] = mine;
    }
}

__global__ void __launch_bounds__(kRsThreads)
compat_second_kernel(const int64_t* __restrict__ off, const int32_t* __restrict__ n_eligible,
                     int max_len, int ld, const u64* __restrict__ bits,
                     int32_t* __restrict__ s) {
    __shared__ u64 tI[kCpTile * kCpLd], tJ[kCpTile * kCpLd];
    const int p = blockIdx.z;
    const int m = cp_m(n_eligible, p, max_len);
    const int i0 = blockIdx.y * kCpTile, j0 = blockIdx.x * kCpTile;
    if (i0 >= m || j0 >= m) return;                        // block-uniform
    const int64_t beg = off[p];
    const u64* B0 = bits + beg * ld;
    const int W = (m + 63) / 64;
    const int ti = threadIdx.x / 16, tj = threadIdx.x % 16;
    // the SC bits of this thread's four rows i against the tile's 64 columns
    u64 scw[4];
    bool any = false;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = i0 + 4 * ti + r;
        scw[r] = i < m ? B0[(int64_t)i * ld + blockIdx.x] : 0ull;
        any = any || scw[r] != 0;
    }
    if (!__syncthreads_or(any)) return;                    // no compatible pair in the tile
    int acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = 0;
    for (int k0 = 0; k0 < W; k0 += kCpKW) {
        __syncthreads();                                   // the previous stage has been read
#pragma unroll
        for (int e = threadIdx.x; e < kCpTile * kCpKW; e += kRsThreads) {
            const int r = e / kCpKW, k = e % kCpKW;
            const bool kin = k0 + k < W;
            tI[r * kCpLd + k] = (kin && i0 + r < m) ? B0[(int64_t)(i0 + r) * ld + k0 + k] : 0ull;
            tJ[r * kCpLd + k] = (kin && j0 + r < m) ? B0[(int64_t)(j0 + r) * ld + k0 + k] : 0ull;
        }
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < kCpKW; ++k) {
            u64 wi[4], wj[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) wi[r] = tI[(4 * ti + r) * kCpLd + k];
#pragma unroll
            for (int c = 0; c < 4; ++c) wj[c] = tJ[(tj + 16 * c) * kCpLd + k];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[r][c] += __popcll(wi[r] & wj[c]);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        int v = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) v += ((scw[r] >> (tj + 16 * c)) & 1ull) ? acc[r][c] : 0;
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);     // the 16 lanes of a ti
        const int i = i0 + 4 * ti + r;
        if (tj == 0 && i < m && v != 0) atomicAdd(&s[beg + i], v);
    }
}

// The largest threshold T with at least `want` keys >= T among key(0 .. n): keys are distinct,
// so exactly `want` keys pass (want <= n). Every thread returns T; block-uniform control flow.
template <class Key, class F>
__device__ Key cp_threshold(int n, int want, int n_bits, F key, int* sh) {
    Key T = 0;
    for (int bit = n_bits - 1; bit >= 0; --bit) {
        const Key cand = T | ((Key)1 << bit);
        int c = 0;
        for (int t = threadIdx.x; t < n; t += kRsThreads) c += key(t) >= cand ? 1 : 0;
        if (block_sum_int(c, sh) >= want) T = cand;
    }
    return T;
}

__global__ void __launch_bounds__(kRsThreads)
compat_top_kernel(const float* __restrict__ w, const int64_t* __restrict__ off,
                  const int32_t* __restrict__ n_eligible, const int32_t* __restrict__ idx,
                  const int32_t* __restrict__ s, int max_len, float w_min, int n_seeds,
                  int32_t* __restrict__ seed_rank, int32_t* __restrict__ seed_row,
                  int32_t* __restrict__ row_score) {
    __shared__ long long sel[kCpMaxSeeds];
    __shared__ int shi[kRsThreads / 64];
    __shared__ int n_sel;
    const int p = blockIdx.x;
    const int64_t beg = off[p], end = off[p + 1];
    const int m = cp_m(n_eligible, p, max_len);
    const int32_t* S0 = s + beg;
    const int32_t* I0 = idx + beg;
    if (row_score) {
        for (int64_t i = beg + threadIdx.x; i < end; i += kRsThreads)
            if (!(!w || w[i] > w_min) || m == 0) row_score[i] = -1;
        for (int r = threadIdx.x; r < m; r += kRsThreads) row_score[beg + I0[r]] = S0[r];
    }
    const int ns = n_seeds < m ? n_seeds : m;
    for (int k = threadIdx.x; k < n_seeds; k += kRsThreads) {
        if (k >= ns) {
            seed_rank[(int64_t)p * n_seeds + k] = -1;
            if (seed_row) seed_row[(int64_t)p * n_seeds + k] = -1;
        }
    }
    if (ns == 0) return;                                   // block-uniform
    if (threadIdx.x == 0) n_sel = 0;
    auto key = [&](int r) {
        return ((long long)S0[r] << kCpRankBits) | (long long)(kCpRankMask - r);
    };
    const long long T = cp_threshold<long long>(m, ns, 31 + kCpRankBits, key, shi);
    for (int r = threadIdx.x; r < m; r += kRsThreads) {
        const long long k = key(r);
        if (k >= T) {                                      // any order: positions come next
            const int e = atomicAdd(&n_sel, 1);
            if (e < kCpMaxSeeds) sel[e] = k;               // exactly ns pass: keys are distinct
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < ns; e += kRsThreads) {
        const long long k = sel[e];
        int pos = 0;
        for (int f = 0; f < ns; ++f) pos += sel[f] > k ? 1 : 0;
        const int r = kCpRankMask - (int)(k & kCpRankMask);
        seed_rank[(int64_t)p * n_seeds + pos] = r;
        if (seed_row) seed_row[(int64_t)p * n_seeds + pos] = I0[r];
    }
}

__global__ void __launch_bounds__(kRsThreads)
compat_seed_kernel(const float4* __restrict__ rows, const int64_t* __restrict__ off,
                   const int32_t* __restrict__ n_eligible, int max_len, int ld,
                   const u64* __restrict__ bits, const int32_t* __restrict__ seed_rank,
                   int n_seeds, int k_set, float r2, RsSlot* __restrict__ slots,
                   float* __restrict__ seed_pose, int32_t* __restrict__ seed_count) {
    __shared__ uint32_t keys[kCpMaxLen];                   // neighbour t: first j, then (c, -j)
    __shared__ u64 rowi[kCpMaxLen / 64];
    __shared__ int degree;
    __shared__ double sh[(kRsThreads / 64) * 16];
    __shared__ int shi[kRsThreads / 64];
    __shared__ float Ts[12];
    const int q = blockIdx.x, p = blockIdx.y;
    const int64_t o = (int64_t)p * n_seeds + q;
    const int m = cp_m(n_eligible, p, max_len);
    const int i = seed_rank[o];                            // -1: an unused position
    const int64_t beg = off[p];
    const float4* R0 = rows + 2 * beg;
    const u64* B0 = bits + beg * ld;
    const int W = (m + 63) / 64;
    int deg = 0;
    if (i >= 0) {                                          // block-uniform
        // the neighbour list, ascending: the thread of word t counts the bits of the words
        // before it (W <= 128) and writes its own bits' columns from there
        if ((int)threadIdx.x < W) rowi[threadIdx.x] = B0[(int64_t)i * ld + threadIdx.x];
        __syncthreads();
        if ((int)threadIdx.x < W) {
            int before = 0;
            for (int t = 0; t < (int)threadIdx.x; ++t) before += __popcll(rowi[t]);
            u64 x = rowi[threadIdx.x];
            while (x) {
                keys[before++] = threadIdx.x * 64 + __ffsll(x) - 1;
                x &= x - 1;
            }
            if ((int)threadIdx.x == W - 1) degree = before;
        }
        __syncthreads();
        deg = degree;
        // c_ij of every neighbour, one lane per neighbour; the seed's row is a broadcast
        for (int t = threadIdx.x; t < deg; t += kRsThreads) {
            const int j = (int)keys[t];
            const ulonglong2* Bj = reinterpret_cast<const ulonglong2*>(B0 + (int64_t)j * ld);
            int c = 0;
#pragma unroll 4
            for (int k = 0; 2 * k < W; ++k) {
                const ulonglong2 x = Bj[k];
                c += __popcll(x.x & rowi[2 * k]);
                if (2 * k + 1 < W) c += __popcll(x.y & rowi[2 * k + 1]);
            }
            keys[t] = ((uint32_t)c << kCpRankBits) | (uint32_t)(kCpRankMask - j);
        }
        __syncthreads();
    }
    const int take = deg < k_set - 1 ? deg : k_set - 1;
    const bool valid = i >= 0 && take >= 2;                // block-uniform
    int cnt = -1;
    if (valid) {
        auto key = [&](int t) { return keys[t]; };
        const uint32_t T = cp_threshold<uint32_t>(deg, take, 14 + kCpRankBits, key, shi);
        double v[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) v[k] = 0.0;
        if (threadIdx.x == 0) rs_moments_add(v, R0[2 * (int64_t)i], R0[2 * (int64_t)i + 1]);
        for (int t = threadIdx.x; t < deg; t += kRsThreads) {
            if (keys[t] >= T) {
                const int64_t j = kCpRankMask - (int)(keys[t] & kCpRankMask);
                rs_moments_add(v, R0[2 * j], R0[2 * j + 1]);
            }
        }
        block_reduce(v, 16, sh);
        if (threadIdx.x == 0) {
            float T12[12];
            rs_moments_pose(v, T12);
#pragma unroll
            for (int k = 0; k < 12; ++k) Ts[k] = T12[k];
        }
        __syncthreads();
        cnt = rs_count(Ts, R0, m, r2, sh);
    } else {
        if (threadIdx.x < 12) Ts[threadIdx.x] = (threadIdx.x % 5 == 0) ? 1.f : 0.f;
        __syncthreads();
    }
    if (threadIdx.x < 12) {
        slots[o].T[threadIdx.x] = Ts[threadIdx.x];
        if (seed_pose) seed_pose[12 * o + threadIdx.x] = Ts[threadIdx.x];
    }
    if (threadIdx.x == 0) {
        slots[o].count = cnt;
        slots[o].h = valid ? q : -1;
        if (seed_count) seed_count[o] = cnt;
    }
}

struct CpWs {
    float4* rows;
    int32_t* idx;
    int32_t* s;
    u64* bits;
    int32_t* seed_rank;
    RsSlot* slots;
    size_t total;
};

void carve_compat(void* ws, int64_t n_tot, int32_t n_pairs, int32_t max_len, int32_t n_seeds,
                  CpWs* w) {
    char* p = static_cast<char*>(ws);
    size_t o = 0;
    auto take = [&](size_t bytes) { void* r = p ? p + o : nullptr; o += rs_align(bytes); return r; };
    w->rows = (float4*)take(sizeof(float4) * 2 * (size_t)n_tot);
    w->idx = (int32_t*)take(sizeof(int32_t) * (size_t)n_tot);
    w->s = (int32_t*)take(sizeof(int32_t) * (size_t)n_tot);
    w->bits = (u64*)take(sizeof(u64) * (size_t)n_tot * cp_stride(max_len));
    w->seed_rank = (int32_t*)take(sizeof(int32_t) * (size_t)n_pairs * n_seeds);
    w->slots = (RsSlot*)take(sizeof(RsSlot) * (size_t)n_pairs * n_seeds);
    w->total = o;
}

bool compat_sizes_ok(int64_t n_tot, int32_t n_pairs, int32_t max_len, int32_t n_seeds) {
    return n_pairs >= 1 && n_pairs <= 65535 && n_tot >= 0 && n_tot < (1ll << 31) &&
           max_len >= 0 && max_len <= kCpMaxLen && n_seeds >= 1 && n_seeds <= kCpMaxSeeds;
}

bool cp_dist_ok(float d) { return d > 0.f && d <= FLT_MAX; }

}  // namespace
}  // namespace fgr

using namespace fgr;

extern "C" int fgr_compat_workspace(int64_t n_tot, int32_t n_pairs, int32_t max_len,
                                    int32_t n_seeds, size_t* bytes) {
    FGR_REQUIRE(bytes && compat_sizes_ok(n_tot, n_pairs, max_len, n_seeds),
                "fgr_compat_workspace: bad arguments (n_tot %lld n_pairs %d max_len %d n_seeds %d)",
                (long long)n_tot, n_pairs, max_len, n_seeds);
    CpWs w;
    carve_compat(nullptr, n_tot, n_pairs, max_len, n_seeds, &w);
    *bytes = w.total;
    return FGR_OK;
}

extern "C" int fgr_compat_pose(const float* a, const float* b, const float* w, int64_t n_tot,
                               const int64_t* off, int32_t n_pairs, int32_t max_len, float w_min,
                               float compat_dist, float inlier_dist, int32_t n_seeds, int32_t k,
                               int32_t n_refits, void* ws, size_t ws_bytes, float* pose,
                               int32_t* n_inliers, float* inlier_rmse, int32_t* n_eligible,
                               int32_t* best_seed, int32_t* n_updates, uint8_t* inlier_mask,
                               int32_t* row_score, int32_t* seed_row, float* seed_pose,
                               int32_t* seed_count, void* stream) {
    FGR_REQUIRE(compat_sizes_ok(n_tot, n_pairs, max_len, n_seeds) && k >= 3 && k <= kCpMaxK &&
                    n_refits >= 0 && cp_dist_ok(compat_dist) && cp_dist_ok(inlier_dist) && off &&
                    ws && (reinterpret_cast<uintptr_t>(ws) & 15) == 0 && pose && n_inliers &&
                    inlier_rmse && n_eligible && best_seed && n_updates &&
                    ((a && b) || n_tot == 0),
                "fgr_compat_pose: bad arguments (n_tot %lld n_pairs %d max_len %d n_seeds %d k %d "
                "n_refits %d compat_dist %g inlier_dist %g)",
                (long long)n_tot, n_pairs, max_len, n_seeds, k, n_refits, (double)compat_dist,
                (double)inlier_dist);
    CpWs s;
    carve_compat(ws, n_tot, n_pairs, max_len, n_seeds, &s);
    FGR_REQUIRE(s.total <= ws_bytes, "fgr_compat_pose: workspace %zu < %zu bytes", ws_bytes,
                s.total);
    hipStream_t st = as_stream(stream);
    TimedCall timed_(st);
    const int ld = cp_stride(max_len);
    const unsigned tiles = (unsigned)((max_len + kCpTile - 1) / kCpTile > 0
                                          ? (max_len + kCpTile - 1) / kCpTile : 1);
    const float r2 = inlier_dist * inlier_dist;
    hipLaunchKernelGGL(ransac_prep_kernel, dim3((unsigned)n_pairs), dim3(kRsThreads), 0, st, a, b,
                       w, off, w_min, s.rows, n_eligible, s.idx);
    FGR_CHECK_LAUNCH("ransac_prep_kernel");
    hipLaunchKernelGGL(compat_bits_kernel, dim3(tiles, (unsigned)n_pairs), dim3(kRsThreads), 0, st,
                       s.rows, off, n_eligible, max_len, ld, compat_dist, s.bits, s.s);
    FGR_CHECK_LAUNCH("compat_bits_kernel");
    hipLaunchKernelGGL(compat_second_kernel, dim3(tiles, tiles, (unsigned)n_pairs),
                       dim3(kRsThreads), 0, st, off, n_eligible, max_len, ld, s.bits, s.s);
    FGR_CHECK_LAUNCH("compat_second_kernel");
    hipLaunchKernelGGL(compat_top_kernel, dim3((unsigned)n_pairs), dim3(kRsThreads), 0, st, w, off,
                       n_eligible, s.idx, s.s, max_len, w_min, n_seeds, s.seed_rank, seed_row,
                       row_score);
    FGR_CHECK_LAUNCH("compat_top_kernel");
    hipLaunchKernelGGL(compat_seed_kernel, dim3((unsigned)n_seeds, (unsigned)n_pairs),
                       dim3(kRsThreads), 0, st, s.rows, off, n_eligible, max_len, ld, s.bits,
                       s.seed_rank, n_seeds, k, r2, s.slots, seed_pose, seed_count);
    FGR_CHECK_LAUNCH("compat_seed_kernel");
    hipLaunchKernelGGL(ransac_select_kernel, dim3((unsigned)n_pairs), dim3(kRsThreads), 0, st, a,
                       b, w, off, s.rows, n_eligible, s.slots, n_seeds, w_min, r2, n_refits, pose,
                       n_inliers, inlier_rmse, best_seed, n_updates, inlier_mask);
    FGR_CHECK_LAUNCH("ransac_select_kernel");
    return FGR_OK;
}
