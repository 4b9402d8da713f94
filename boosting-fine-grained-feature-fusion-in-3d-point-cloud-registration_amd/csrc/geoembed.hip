// GeometricStructureEmbedding (position_embedding.py:129-196, `pos_emb_type: geometric`): the
// rotation-invariant embedding of each point's distances and angles to its k nearest neighbours
// of the same cloud,
//
//   out[i] = max_{j in nn(i)} [ proj_d(E(d_ij)) + red_{r in nn(i)} proj_a(E(a_ijr)) ]
//
//   d_ij  = |p_j - p_i| / sigma_d
//   a_ijr = atan2(|(p_r - p_i) x (p_j - p_i)|, (p_r - p_i) . (p_j - p_i)) * 180 / (sigma_a pi)
//   E(t)  = [sin(t w_0), cos(t w_0), sin(t w_1), cos(t w_1), ...]      (D values, interleaved)
//
// with red = max or mean and both maxima per channel. The reference forms the embedding of every
// pair and triplet of a cloud ((1, N, N, k, D) tensors) and gathers k columns of each row; what
// it uses is k (1 + k) embedding rows per point. Two launches build only those:
//
//   * geo_indices_kernel: brute force over the point's own cloud. A block owns 16 points, 16
//     threads each (a serial scan is bound by its own latency, not by arithmetic): the
//     candidates of the block's clouds pass through LDS 256 at a time, thread (point, part) scans
//     a sixteenth of every tile with its k best kept sorted in registers, and part 0 merges the
//     16 lists. "Better" is (squared distance from coordinate differences,
//     index) in lexicographic order -- ties to the lower index whatever the scan order -- and the
//     point itself is excluded by index. Then d and a with precise sqrtf / atan2f. No atomics,
//     no candidate outside the point's cloud.
//   * geo_embed_kernel: a block owns G groups of 4 points. A group is five 16-column MFMA tiles:
//     tile t < 4 holds the angle rows of point t (lane column 4 j + r), tile 4 the distance rows
//     of all four points (lane column 4 t + j); lanes with j >= k or r >= k are padding. Only
//     the 4 k^2 + 4 k real columns of a group exist in memory: the block builds their E rows
//     once, with precise sincosf, as two-fp16-term B fragments in LDS ([group][k32 step][term]
//     [g][column] x 16 B = 1 KB per column; |E| <= 1, so the scale is the constant 2^14), and a
//     padding lane reads a real column's fragment (its results are masked). The eight waves
//     split the projections' 16-column output panels (wave w: panels 2 w, 2 w + 1 of both); a
//     panel's weight fragments of both projections (A operand; plain fgr_split_weights_h3 images
//     from global / L2) stay in registers while the wave runs the f16x3 products of all G
//     groups, so a block reads each weight byte once for 4 G points. A panel's epilogue is in
//     registers: lane (g, c) holds outputs 16 q + 4 g .. + 3 of column c; bias, the reduction
//     over r across the four lanes of a quad (DPP), the distance term fetched from tile 4's lane
//     4 t + j, padding to -inf, the maximum over the 16 lanes of the row (DPP), and lane c = 0
//     stores 16 B.
//
// A point's arithmetic is a fixed sequence that involves no other point (MFMA B columns are
// independent, the scale is a constant), so its bits do not depend on the call's other points.
#include <climits>
#include <cmath>

#include "mfma.h"

namespace fgr {
namespace {

constexpr int kGeoMaxK = 4;
constexpr int kGeoThreads = 512;           // 8 waves: two output panels of each projection per wave
constexpr int kIdxPts = 16;                // points per block of the indices kernel
constexpr int kIdxParts = 16;              // threads per point
constexpr int kIdxTile = kIdxPts * kIdxParts;      // candidates staged in LDS at a time

// (d2, id) into the K best, sorted by (d2, id) ascending
template <int K>
__device__ __forceinline__ void knn_insert(float (&bd)[K], int (&bi)[K], float d2, int id) {
    if (!(d2 < bd[K - 1] || (d2 == bd[K - 1] && id < bi[K - 1]))) return;
    bool shift = false;
#pragma unroll
    for (int s = 0; s < K; ++s) {
        // in front of the first entry that is worse; from there on every entry moves down a slot
        if (shift || d2 < bd[s] || (d2 == bd[s] && id < bi[s])) {
            shift = true;
            const float td = bd[s]; bd[s] = d2; d2 = td;
            const int ti = bi[s]; bi[s] = id; id = ti;
        }
    }
}

template <int K>
__global__ void __launch_bounds__(kIdxTile) geo_indices_kernel(
        const float* __restrict__ xyz, int64_t n, const int64_t* __restrict__ cloud_off,
        int n_clouds, float sigma_d, float factor_a, int32_t* __restrict__ nn,
        float* __restrict__ d, float* __restrict__ a) {
    __shared__ float4 pts[kIdxTile];
    __shared__ float md[kIdxParts - 1][K][kIdxPts];
    __shared__ int mi[kIdxParts - 1][K][kIdxPts];
    const int tid = threadIdx.x, pl = tid % kIdxPts, part = tid / kIdxPts;
    const int64_t i0 = (int64_t)blockIdx.x * kIdxPts;
    const bool live = i0 + pl < n;
    const int64_t i = min(i0 + pl, n - 1);      // threads past n scan as the last point, write nothing
    // a table entry is clamped into the call's rows, whatever it holds
    auto row = [&](int c) { return max((int64_t)0, min(cloud_off[c], n)); };
    const int cl = find_segment(cloud_off, n_clouds, i);
    const int64_t lo = row(cl), hi = max(lo, row(cl + 1));
    // the block's candidates: from the first point's cloud to the last point's cloud
    const int64_t b_lo = row(find_segment(cloud_off, n_clouds, i0));
    const int64_t b_hi = max(b_lo, row(find_segment(cloud_off, n_clouds, min(i0 + kIdxPts, n) - 1) + 1));
    const float px = xyz[3 * i], py = xyz[3 * i + 1], pz = xyz[3 * i + 2];
    float bd[K];
    int bi[K];
#pragma unroll
    for (int s = 0; s < K; ++s) { bd[s] = INFINITY; bi[s] = INT_MAX; }
    for (int64_t base = b_lo; base < b_hi; base += kIdxTile) {
        __syncthreads();                             // the previous tile has been read
        if (base + tid < b_hi) {
            const float* q = xyz + 3 * (base + tid);
            pts[tid] = make_float4(q[0], q[1], q[2], 0.f);
        }
        __syncthreads();
        const int cnt = (int)min((int64_t)kIdxTile, b_hi - base);
        const int j1 = min((part + 1) * kIdxPts, cnt);
        for (int jj = part * kIdxPts; jj < j1; ++jj) {
            const int64_t j = base + jj;
            if (j < lo || j >= hi || j == i) continue;
            const float4 q = pts[jj];
            const float dx = q.x - px, dy = q.y - py, dz = q.z - pz;
            knn_insert<K>(bd, bi, dx * dx + dy * dy + dz * dz, (int)j);
        }
    }
    if (part > 0) {
#pragma unroll
        for (int s = 0; s < K; ++s) { md[part - 1][s][pl] = bd[s]; mi[part - 1][s][pl] = bi[s]; }
    }
    __syncthreads();
    if (part > 0 || !live) return;
#pragma unroll
    for (int h = 0; h < kIdxParts - 1; ++h) {
#pragma unroll
        for (int s = 0; s < K; ++s) knn_insert<K>(bd, bi, md[h][s][pl], mi[h][s][pl]);
    }
    float vx[K], vy[K], vz[K];
#pragma unroll
    for (int s = 0; s < K; ++s) {
        // a cloud of fewer than K + 1 points (the host wrappers refuse it): the point itself
        if (bi[s] == INT_MAX) { bi[s] = (int)i; bd[s] = 0.f; }
        const float* q = xyz + 3 * (int64_t)bi[s];
        vx[s] = q[0] - px; vy[s] = q[1] - py; vz[s] = q[2] - pz;
        nn[i * K + s] = bi[s];
        d[i * K + s] = sqrtf(bd[s]) / sigma_d;
    }
#pragma unroll
    for (int j = 0; j < K; ++j) {
#pragma unroll
        for (int r = 0; r < K; ++r) {
            // ref = p_r - p_i, anc = p_j - p_i: |ref x anc|, ref . anc
            const float cx = vy[r] * vz[j] - vz[r] * vy[j];
            const float cy = vz[r] * vx[j] - vx[r] * vz[j];
            const float cz = vx[r] * vy[j] - vy[r] * vx[j];
            const float sn = sqrtf(cx * cx + cy * cy + cz * cz);
            const float cs = vx[r] * vx[j] + vy[r] * vy[j] + vz[r] * vz[j];
            a[(i * K + j) * K + r] = atan2f(sn, cs) * factor_a;
        }
    }
}

struct GeoEmbedArgs {
    const float* d; const float* a; int64_t n;
    const float* div_term;                       // w_m, D / 2 values
    const u32x4* wd; const float* wd_sc; const float* bd;
    const u32x4* wa; const float* wa_sc; const float* ba;
    float* out; int64_t ldo;
};

// real columns of a 4-point group: the points' k^2 angle rows, then their k distance rows
__host__ __device__ constexpr int geo_cols(int k) { return 4 * k * k + 4 * k; }
// groups per block: what fits the 160 KB of LDS at 1 KB per column (k = 3: 3 x 48 KB)
__host__ __device__ constexpr int geo_groups(int k) { return k <= 2 ? 4 : (k == 3 ? 3 : 1); }

template <int K, bool MEAN>
__global__ void __launch_bounds__(kGeoThreads, 1) geo_embed_kernel(GeoEmbedArgs p) {
    constexpr int D = 256, KS = D / 32;                   // k32 steps
    constexpr int NC = geo_cols(K), G = geo_groups(K), KK = K * K;
    __shared__ u32x4 img[G * KS * 2 * 4 * NC];            // [group][k32 step][term][g][column]
    __shared__ float tv[G][NC];                           // the columns' a / d values

    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    const int g = lane >> 4, c = lane & 15;
    const int64_t p0 = (int64_t)blockIdx.x * (4 * G);

    // points past n take the last point's (finite) values and are never stored
    for (int idx = tid; idx < G * NC; idx += kGeoThreads) {
        const int gi = idx / NC, col = idx % NC;
        float v;
        if (col < 4 * KK) {
            const int64_t pt = min(p0 + 4 * gi + col / KK, p.n - 1);
            v = p.a[pt * KK + col % KK];
        } else {
            const int c2 = col - 4 * KK;
            const int64_t pt = min(p0 + 4 * gi + c2 / K, p.n - 1);
            v = p.d[pt * K + c2 % K];
        }
        tv[gi][col] = v;
    }
    __syncthreads();

    // E rows as B fragments: slot (g, column) of k32 step s holds k = 32 s + 8 g + e, i.e. (sin,
    // cos) of w_m, m = 16 s + 4 g + 0..3
    for (int idx = tid; idx < G * KS * 4 * NC; idx += kGeoThreads) {
        const int col = idx % NC, gg = (idx / NC) & 3, s = (idx / (4 * NC)) % KS;
        const int gi = idx / (4 * NC * KS);
        if (p0 + 4 * gi >= p.n) break;                    // a whole group past n (idx ascends in gi)
        const float x = tv[gi][col];
        const float4 w4 = ld4(p.div_term + 16 * s + 4 * gg);
        const float om[4] = {x * w4.x, x * w4.y, x * w4.z, x * w4.w};
        float e[8];
#pragma unroll
        for (int m = 0; m < 4; ++m) sincosf(om[m], &e[2 * m], &e[2 * m + 1]);
        u32x4 hi, lo;
        split8_f16(e, 16384.f, hi, lo);
        u32x4* dst = img + ((gi * KS + s) * 2) * (4 * NC) + gg * NC + col;
        dst[0] = hi;
        dst[4 * NC] = lo;
    }
    __syncthreads();

    constexpr float kInvScale = 1.f / 16384.f;
    // lane column c of an angle tile is (j, r) = (c >> 2, c & 3), of the distance tile (point,
    // j) = (c >> 2, c & 3); a padding lane reads a real column
    const int jc = c >> 2, rc = c & 3;
    const int col_a = (jc < K && rc < K) ? jc * K + rc : 0;
    const int col_d = 4 * KK + (rc < K ? jc * K + rc : 0);
#pragma unroll 1
    for (int pq = 0; pq < 2; ++pq) {
        const int q = 2 * wv + pq;                         // output panel: n = 16 q + 4 g + r
        u32x4 wa[KS][2], wd[KS][2];
#pragma unroll
        for (int s = 0; s < KS; ++s) {
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                wa[s][t] = p.wa[((q * KS + s) * 2 + t) * 64 + lane];
                wd[s][t] = p.wd[((q * KS + s) * 2 + t) * 64 + lane];
            }
        }
        const int n0 = 16 * q + 4 * g;
        const float4 sa = ld4(p.wa_sc + n0), ba = ld4(p.ba + n0);
        const float4 sd = ld4(p.wd_sc + n0), bd = ld4(p.bd + n0);
        const float sav[4] = {sa.x, sa.y, sa.z, sa.w}, bav[4] = {ba.x, ba.y, ba.z, ba.w};
        const float sdv[4] = {sd.x, sd.y, sd.z, sd.w}, bdv[4] = {bd.x, bd.y, bd.z, bd.w};
#pragma unroll 1
        for (int gi = 0; gi < G; ++gi) {
            if (p0 + 4 * gi >= p.n) break;
            f32x4 acc[5];
#pragma unroll
            for (int t = 0; t < 5; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const u32x4* src = img + ((gi * KS + s) * 2) * (4 * NC) + g * NC;
                f16x8 eh[5], el[5];
#pragma unroll
                for (int t = 0; t < 5; ++t) {
                    const int col = t < 4 ? t * KK + col_a : col_d;
                    eh[t] = __builtin_bit_cast(f16x8, src[col]);
                    el[t] = __builtin_bit_cast(f16x8, src[4 * NC + col]);
                }
                // term by term over the five tiles: no MFMA waits for the one before it
#pragma unroll
                for (int term = 0; term < 3; ++term) {
#pragma unroll
                    for (int t = 0; t < 5; ++t) {
                        const f16x8 wh = __builtin_bit_cast(f16x8, t < 4 ? wa[s][0] : wd[s][0]);
                        const f16x8 wl = __builtin_bit_cast(f16x8, t < 4 ? wa[s][1] : wd[s][1]);
                        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
                            term == 0 ? wl : wh, term == 1 ? el[t] : eh[t], acc[t], 0, 0, 0);
                    }
                }
            }
            float yd[4];                                   // proj_d of (point c >> 2, j = c & 3)
#pragma unroll
            for (int r = 0; r < 4; ++r) yd[r] = fmaf(acc[4][r], sdv[r] * kInvScale, bdv[r]);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                float y[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float v = fmaf(acc[t][r], sav[r] * kInvScale, bav[r]);
                    // the reduction over r: the four lanes of a quad, every lane gets the result
                    if constexpr (MEAN) {
                        v = rc < K ? v : 0.f;
                        v += dpp<0xB1>(v);
                        v += dpp<0x4E>(v);
                        v = v / (float)K;
                    } else {
                        v = rc < K ? v : -INFINITY;
                        v = fmaxf(v, dpp<0xB1>(v));
                        v = fmaxf(v, dpp<0x4E>(v));
                    }
                    // + the distance term of (point t, j): tile 4's lane column 4 t + j, same g
                    v += __shfl(yd[r], (lane & 48) | (4 * t + jc), kWave);
                    y[r] = row16_max(jc < K ? v : -INFINITY);  // the maximum over j
                }
                const int64_t pt = p0 + 4 * gi + t;
                if (c == 0 && pt < p.n)
                    *reinterpret_cast<float4*>(p.out + pt * p.ldo + n0) =
                        make_float4(y[0], y[1], y[2], y[3]);
            }
        }
    }
}

template <int K>
void geo_embed_launch(const GeoEmbedArgs& a, int reduction, hipStream_t st) {
    const dim3 grid((unsigned)ceil_div(a.n, 4 * geo_groups(K)));
    if (reduction == FGR_GEO_MEAN)
        hipLaunchKernelGGL((geo_embed_kernel<K, true>), grid, dim3(kGeoThreads), 0, st, a);
    else
        hipLaunchKernelGGL((geo_embed_kernel<K, false>), grid, dim3(kGeoThreads), 0, st, a);
}

}  // namespace
}  // namespace fgr

using namespace fgr;

extern "C" int fgr_geo_embed_indices(const float* xyz, int64_t n, const int64_t* cloud_off,
                                     int32_t n_clouds, int32_t k, float sigma_d, float factor_a,
                                     int32_t* nn, float* d, float* a, void* stream) {
    FGR_REQUIRE(n >= 0 && n <= 0x7fffffff && n_clouds >= 0,
                "fgr_geo_embed_indices: bad arguments (n %lld, n_clouds %d)", (long long)n, n_clouds);
    FGR_REQUIRE(k >= 1 && k <= kGeoMaxK, "fgr_geo_embed_indices: k %d not supported (1..%d)", k,
                kGeoMaxK);
    FGR_REQUIRE(sigma_d > 0.f && std::isfinite(sigma_d) && std::isfinite(factor_a),
                "fgr_geo_embed_indices: sigma_d must be positive and finite, factor_a finite");
    if (n == 0) return FGR_OK;
    FGR_REQUIRE(n_clouds >= 1, "fgr_geo_embed_indices: %lld points in no cloud", (long long)n);
    FGR_REQUIRE(xyz && cloud_off && nn && d && a, "fgr_geo_embed_indices: null pointer");
    hipStream_t st = as_stream(stream);
    TimedCall timed_(st);
    const dim3 grid((unsigned)ceil_div(n, kIdxPts));
#define FGR_GEO_IDX(K_)                                                                        \
    hipLaunchKernelGGL((geo_indices_kernel<K_>), grid, dim3(kIdxTile), 0, st, xyz, n, cloud_off, \
                       n_clouds, sigma_d, factor_a, nn, d, a)
    switch (k) {
        case 1: FGR_GEO_IDX(1); break;
        case 2: FGR_GEO_IDX(2); break;
        case 3: FGR_GEO_IDX(3); break;
        default: FGR_GEO_IDX(4); break;
    }
#undef FGR_GEO_IDX
    FGR_CHECK_LAUNCH("geo_indices_kernel");
    return FGR_OK;
}

extern "C" int fgr_geo_embed_f16x3_supported(int64_t n, int32_t d_model, int32_t k) {
    return (n >= 1 && n <= 0x7fffffff && d_model == 256 && k >= 1 && k <= kGeoMaxK) ? 1 : 0;
}

extern "C" int fgr_geo_embed_f16x3(const float* d, const float* a, int64_t n, int32_t k,
                                   const float* div_term, const void* wd_img, const float* bd,
                                   const void* wa_img, const float* ba, int32_t d_model,
                                   int32_t reduction, float* out, int64_t ldo, void* stream) {
    FGR_REQUIRE(n >= 0 && ldo >= d_model, "fgr_geo_embed_f16x3: bad arguments (n %lld, ldo %lld)",
                (long long)n, (long long)ldo);
    FGR_REQUIRE(d_model == 256 && k >= 1 && k <= kGeoMaxK,
                "fgr_geo_embed_f16x3: d_model %d, k %d not supported (256, 1..%d: "
                "fgr_geo_embed_f16x3_supported)", d_model, k, kGeoMaxK);
    FGR_REQUIRE(reduction == FGR_GEO_MAX || reduction == FGR_GEO_MEAN,
                "fgr_geo_embed_f16x3: reduction %d (FGR_GEO_MAX or FGR_GEO_MEAN)", reduction);
    FGR_REQUIRE(div_term && wd_img && bd && wa_img && ba, "fgr_geo_embed_f16x3: null weight pointer");
    FGR_REQUIRE(n == 0 || (d && a && out), "fgr_geo_embed_f16x3: null pointer");
    FGR_REQUIRE(n == 0 || fgr_geo_embed_f16x3_supported(n, d_model, k),
                "fgr_geo_embed_f16x3: n %lld not supported", (long long)n);
    const uintptr_t al = reinterpret_cast<uintptr_t>(wd_img) | reinterpret_cast<uintptr_t>(bd) |
                         reinterpret_cast<uintptr_t>(wa_img) | reinterpret_cast<uintptr_t>(ba) |
                         reinterpret_cast<uintptr_t>(div_term) | reinterpret_cast<uintptr_t>(out);
    FGR_REQUIRE((al & 15) == 0 && ldo % 4 == 0,
                "fgr_geo_embed_f16x3: images, biases, div_term and out must be 16-B aligned, "
                "ldo %% 4 == 0");
    if (n == 0) return FGR_OK;
    hipStream_t st = as_stream(stream);
    TimedCall timed_(st);
    // fgr_split_weights_h3 of (256, 256): 16 panels x 8 k32 steps x 128 units, then the scales
    const size_t units = (size_t)(d_model / 16) * (d_model / 32) * 128 * 16;
    GeoEmbedArgs g;
    g.d = d; g.a = a; g.n = n; g.div_term = div_term; g.out = out; g.ldo = ldo;
    g.wd = static_cast<const u32x4*>(wd_img);
    g.wd_sc = reinterpret_cast<const float*>(static_cast<const char*>(wd_img) + units);
    g.bd = bd;
    g.wa = static_cast<const u32x4*>(wa_img);
    g.wa_sc = reinterpret_cast<const float*>(static_cast<const char*>(wa_img) + units);
    g.ba = ba;
    switch (k) {
        case 1: geo_embed_launch<1>(g, reduction, st); break;
        case 2: geo_embed_launch<2>(g, reduction, st); break;
        case 3: geo_embed_launch<3>(g, reduction, st); break;
        default: geo_embed_launch<4>(g, reduction, st); break;
    }
    FGR_CHECK_LAUNCH("geo_embed_kernel");
    return FGR_OK;
}
