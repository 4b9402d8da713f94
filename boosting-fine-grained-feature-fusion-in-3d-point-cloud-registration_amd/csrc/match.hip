// Feature matching (fgr_feature_nn, fgr_match_pairs; semantics in include/fgreg.h, restated in
// tests/_match_ref.py). Built -ffp-contract=off: the fp32 score dot - |k|^2 / 2, the distance
// |q|^2 - 2 s and the inlier residual round as written.
//
// fgr_feature_nn is the first half of the flash-attention tile loop: S^T = K Q^T on the fp16
// matrix cores in the f16x3 split (mma_h3), 64 keys at a time, with a running (best, second,
// index) per lane instead of the softmax and PV. One launch covers every segment; a block of 4
// waves takes 64 query rows of one segment (block_split's XCD order), wave w rows 16 w .. + 15.
//   * Queries are the MFMA's B operand and stay in registers for the whole block: lane (g, c)
//     holds dims 32 kd + 8 g .. + 7 of query c, scaled by the row's exact power of two
//     (row_scale_exp) and split in two fp16 terms.
//   * Keys are the A operand. Thread (key = tid / 4, g = tid % 4) first reads its key row's
//     dims 32 kd + 8 g .. + 7 of every kd for the row's max |x| and |k|^2 (no workspace), then
//     stages the tile through LDS one 32-wide k step at a time, scaled and split, in two
//     buffers with one barrier per step; the next step's global load is in flight over the
//     MFMAs. LDS unit (term, g, key) x 16 B with the g stride padded to 68 units, so that the
//     four g writers of a key and the 16 readers of a fragment hit distinct banks.
//   * C[i = key 4 g + r][j = query c]: every lane owns one query and sees its keys in
//     ascending order, so `>` keeps the lowest index; the four g lanes of a query merge once,
//     after the last tile, with the explicit lowest-index rule.
// The score is acc * 2^-e_k * 2^-e_q (exact) - |k|^2 / 2. No atomics, every output element is
// stored once.
#include "attn_tile.h"

namespace fgr {
namespace {

constexpr int kNnThreads = 256;
constexpr int kNnGStride = 68;                    // units between the g planes of a term
constexpr int kNnTerm = 4 * kNnGStride;           // units of one term of a k step
constexpr int kNoKey = 0x7fffffff;

struct NnBest {
    float b, s;
    int i;
};
// keys arrive in ascending order: a strictly larger score takes over, an equal one is second
__device__ __forceinline__ void nn_take(NnBest& r, float v, int key) {
    if (v > r.b) {
        r.s = r.b;
        r.b = v;
        r.i = key;
    } else if (v > r.s) {
        r.s = v;
    }
}
// two disjoint key sets: the larger best wins, the lower index on equal scores
__device__ __forceinline__ void nn_merge(NnBest& r, float b2, float s2, int i2) {
    const bool take = b2 > r.b || (b2 == r.b && i2 < r.i);
    const float loser = take ? r.b : b2;
    r.s = fmaxf(loser, fmaxf(r.s, s2));
    if (take) {
        r.b = b2;
        r.i = i2;
    }
}

template <int KD>
__global__ __launch_bounds__(kNnThreads) void feature_nn_kernel(
    const float* __restrict__ q, const float* __restrict__ k, int d, int kd_n,
    const int64_t* __restrict__ q_off, const int64_t* __restrict__ kv_off,
    const int32_t* __restrict__ kv_seg, int n_seg, int n_blk, int metric,
    int32_t* __restrict__ nn_idx, float* __restrict__ best, float* __restrict__ second) {
    __shared__ uint4 kb[2][2 * kNnTerm];
    __shared__ __attribute__((aligned(16))) float kst[2][2][64];     // [tile & 1][2^-e_k, |k|^2 / 2][key]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, c = lane & 15;
    int seg, head, blk;
    if (!block_split(n_blk, n_seg, 1, seg, head, blk)) return;
    const int64_t q0 = q_off[seg];
    const int qlen = (int)(q_off[seg + 1] - q0);
    if (blk * 64 >= qlen) return;
    const int ks = kv_seg[seg];
    const int64_t k0 = kv_off[ks];
    const int klen = (int)(kv_off[ks + 1] - k0);

    // ---- this lane's part of its query row (a row past the segment repeats the last one)
    const int qi = blk * 64 + wave * 16 + c;
    const float* qp = q + (q0 + min(qi, qlen - 1)) * (int64_t)d + 8 * g;
    f16x8 qh[KD], ql[KD];
    float q2, q_unscale;
    {
        float x[KD][8];
        float mx = 0.f, ss = 0.f;
#pragma unroll
        for (int kd = 0; kd < KD; ++kd) {
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
            if (kd < kd_n) {
                a = ld4(qp + 32 * kd);
                b = ld4(qp + 32 * kd + 4);
            }
            x[kd][0] = a.x; x[kd][1] = a.y; x[kd][2] = a.z; x[kd][3] = a.w;
            x[kd][4] = b.x; x[kd][5] = b.y; x[kd][6] = b.z; x[kd][7] = b.w;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                mx = fmaxf(mx, fabsf(x[kd][e]));
                ss += x[kd][e] * x[kd][e];
            }
        }
        q2 = xg_sum(ss);
        const int eq = row_scale_exp(xg_max(mx));
        const float sq = __builtin_ldexpf(1.f, eq);
        q_unscale = __builtin_ldexpf(1.f, -eq);
#pragma unroll
        for (int kd = 0; kd < KD; ++kd)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                _Float16 h, m;
                split2(x[kd][e] * sq, h, m);
                qh[kd][e] = h;
                ql[kd][e] = m;
            }
    }

    NnBest r{-INFINITY, -INFINITY, kNoKey};
    const int skey = tid >> 2, sg = tid & 3;
    const int ntile = (klen + 63) / 64;
    int p = 0;
    for (int t = 0; t < ntile; ++t) {
        // ---- this thread's key row of the tile (past the segment: the last row again; its
        // scores are never taken): max |x| and |k|^2 over the whole row, shared by its 4 threads
        const float* kp = k + (k0 + min(t * 64 + skey, klen - 1)) * (int64_t)d + 8 * sg;
        float mx = 0.f, ss = 0.f;
        for (int kd = 0; kd < kd_n; ++kd) {
            const float4 a = ld4(kp + 32 * kd), b = ld4(kp + 32 * kd + 4);
            mx = fmaxf(mx, fmaxf(fmaxf(fmaxf(fabsf(a.x), fabsf(a.y)), fmaxf(fabsf(a.z), fabsf(a.w))),
                                 fmaxf(fmaxf(fabsf(b.x), fabsf(b.y)), fmaxf(fabsf(b.z), fabsf(b.w)))));
            ss += a.x * a.x; ss += a.y * a.y; ss += a.z * a.z; ss += a.w * a.w;
            ss += b.x * b.x; ss += b.y * b.y; ss += b.z * b.z; ss += b.w * b.w;
        }
        mx = fmaxf(mx, __shfl_xor(mx, 1, kWave));
        mx = fmaxf(mx, __shfl_xor(mx, 2, kWave));
        ss += __shfl_xor(ss, 1, kWave);
        ss += __shfl_xor(ss, 2, kWave);
        const int ek = row_scale_exp(mx);
        const float sk = __builtin_ldexpf(1.f, ek);
        if (sg == 0) {
            kst[t & 1][0][skey] = __builtin_ldexpf(1.f, -ek);
            kst[t & 1][1][skey] = metric == FGR_MATCH_EUCLID ? 0.5f * ss : 0.f;
        }

        // ---- the k steps: split and stage step kd, start the load of kd + 1, barrier, MFMAs
        f32x4 acc[4];
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
        float4 xa = ld4(kp), xb = ld4(kp + 4);
#pragma unroll
        for (int kd = 0; kd < KD; ++kd) {
            if (kd >= kd_n) continue;       // uniform over the block
            const float x[8] = {xa.x, xa.y, xa.z, xa.w, xb.x, xb.y, xb.z, xb.w};
            f16x8 h8, m8;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                _Float16 h, m;
                split2(x[e] * sk, h, m);
                h8[e] = h;
                m8[e] = m;
            }
            kb[p][sg * kNnGStride + skey] = __builtin_bit_cast(uint4, h8);
            kb[p][kNnTerm + sg * kNnGStride + skey] = __builtin_bit_cast(uint4, m8);
            if (kd + 1 < kd_n) {
                xa = ld4(kp + 32 * (kd + 1));
                xb = ld4(kp + 32 * (kd + 1) + 4);
            }
            __syncthreads();
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                const f16x8 kh = __builtin_bit_cast(f16x8, kb[p][g * kNnGStride + 16 * n + c]);
                const f16x8 kl = __builtin_bit_cast(f16x8, kb[p][kNnTerm + g * kNnGStride + 16 * n + c]);
                mma_h3(kh, kl, qh[kd], ql[kd], acc[n]);
            }
            p ^= 1;
        }

        // ---- scores of this lane's 16 keys of the tile, in ascending key order
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const float4 us = *reinterpret_cast<const float4*>(&kst[t & 1][0][16 * n + 4 * g]);
            const float4 hk = *reinterpret_cast<const float4*>(&kst[t & 1][1][16 * n + 4 * g]);
            const float u[4] = {us.x, us.y, us.z, us.w}, hh[4] = {hk.x, hk.y, hk.z, hk.w};
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int key = t * 64 + 16 * n + 4 * g + rr;
                const float v = (acc[n][rr] * u[rr]) * q_unscale - hh[rr];
                if (key < klen) nn_take(r, v, key);
            }
        }
    }

    // ---- the four g lanes of a query hold disjoint key sets
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {
        const float b2 = __shfl_xor(r.b, o, kWave), s2 = __shfl_xor(r.s, o, kWave);
        const int i2 = __shfl_xor(r.i, o, kWave);
        nn_merge(r, b2, s2, i2);
    }
    if (g == 0 && qi < qlen) {
        const int64_t row = q0 + qi;
        nn_idx[row] = r.i == kNoKey ? -1 : r.i;
        float ob = r.b, os = r.s;
        if (metric == FGR_MATCH_EUCLID) {       // -inf (no key) -> +inf
            ob = fmaxf(0.f, q2 - 2.f * ob);
            os = fmaxf(0.f, q2 - 2.f * os);
        }
        best[row] = ob;
        if (second) second[row] = os;
    }
}

// One block per pair, no atomics: rows strided over the block, the two counts reduced in
// integers (wave shuffles, then the 4 wave totals through LDS).
__global__ __launch_bounds__(256) void match_pairs_kernel(
    const int32_t* __restrict__ nn, const float* __restrict__ best, const float* __restrict__ second,
    const float* __restrict__ xyz, const int64_t* __restrict__ off, const int64_t* __restrict__ out_off,
    int n_pairs, int mode, float ratio2, const float* __restrict__ gt_pose, float r2,
    float* __restrict__ a, float* __restrict__ b, float* __restrict__ w,
    int32_t* __restrict__ n_match, int32_t* __restrict__ n_inlier) {
    __shared__ int red[2][4];
    const int p = blockIdx.x;
    const int64_t s0 = off[p], ns = off[p + 1] - s0;
    const int64_t t0 = off[n_pairs + p], nt = off[n_pairs + p + 1] - t0;
    const int64_t o0 = out_off[p];
    float P[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) P[e] = gt_pose ? gt_pose[12 * p + e] : 0.f;
    int cm = 0, ci = 0;
    for (int64_t i = threadIdx.x; i < ns + nt; i += blockDim.x) {
        const bool is_src = i < ns;
        const int64_t row = is_src ? s0 + i : t0 + (i - ns);
        const int64_t other0 = is_src ? t0 : s0, other_n = is_src ? nt : ns;
        int n = nn[row];
        if (n < 0 || n >= other_n) n = -1;
        bool on = n >= 0 && (is_src || mode == FGR_MATCH_BILATERAL);
        if (on && mode == FGR_MATCH_MUTUAL) on = (int64_t)nn[t0 + n] == i;
        if (on && ratio2 > 0.f) on = best[row] < ratio2 * second[row];
        const float ox = xyz[3 * row], oy = xyz[3 * row + 1], oz = xyz[3 * row + 2];
        float mx = 0.f, my = 0.f, mz = 0.f;
        if (n >= 0) {
            const float* m = xyz + 3 * (other0 + n);
            mx = m[0]; my = m[1]; mz = m[2];
        }
        const float ax = is_src ? ox : mx, ay = is_src ? oy : my, az = is_src ? oz : mz;
        const float bx = is_src ? mx : ox, by = is_src ? my : oy, bz = is_src ? mz : oz;
        const int64_t o = o0 + i;
        a[3 * o] = ax; a[3 * o + 1] = ay; a[3 * o + 2] = az;
        b[3 * o] = bx; b[3 * o + 1] = by; b[3 * o + 2] = bz;
        w[o] = on ? 1.f : 0.f;
        cm += on;
        if (gt_pose && on) {
            const float dx = (((P[0] * ax + P[1] * ay) + P[2] * az) + P[3]) - bx;
            const float dy = (((P[4] * ax + P[5] * ay) + P[6] * az) + P[7]) - by;
            const float dz = (((P[8] * ax + P[9] * ay) + P[10] * az) + P[11]) - bz;
            const float d2 = ((dx * dx) + dy * dy) + dz * dz;
            ci += d2 < r2;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        cm += __shfl_xor(cm, o, kWave);
        ci += __shfl_xor(ci, o, kWave);
    }
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = cm;
        red[1][threadIdx.x >> 6] = ci;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        n_match[p] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
        if (n_inlier) n_inlier[p] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    }
}

template <int KD>
void launch_nn(dim3 grid, hipStream_t st, const float* q, const float* k, int d,
               const int64_t* q_off, const int64_t* kv_off, const int32_t* kv_seg, int n_seg,
               int n_blk, int metric, int32_t* nn_idx, float* best, float* second) {
    hipLaunchKernelGGL(feature_nn_kernel<KD>, grid, dim3(kNnThreads), 0, st, q, k, d, d / 32, q_off,
                       kv_off, kv_seg, n_seg, n_blk, metric, nn_idx, best, second);
}

}  // namespace
}  // namespace fgr

using namespace fgr;

extern "C" int fgr_feature_nn_supported(int32_t d) { return d % 32 == 0 && d >= 32 && d <= 512; }

extern "C" int fgr_feature_nn(const float* q, const float* k, int32_t d, int64_t n_q_rows,
                              int64_t n_k_rows, const int64_t* q_off, const int64_t* kv_off,
                              const int32_t* kv_seg, int32_t n_seg, int32_t max_q_len,
                              int32_t metric, int32_t* nn_idx, float* best, float* second,
                              void* stream) {
    FGR_REQUIRE(fgr_feature_nn_supported(d), "fgr_feature_nn: d = %d (needs d %% 32 == 0, 32 <= d <= 512)", d);
    FGR_REQUIRE(metric == FGR_MATCH_DOT || metric == FGR_MATCH_EUCLID, "fgr_feature_nn: metric %d", metric);
    FGR_REQUIRE(n_seg >= 1 && n_seg <= 65535, "fgr_feature_nn: n_seg = %d", n_seg);
    FGR_REQUIRE(n_q_rows >= 0 && n_q_rows < (int64_t)1 << 31 && n_k_rows >= 0 && n_k_rows < (int64_t)1 << 31,
                "fgr_feature_nn: n_q_rows = %lld, n_k_rows = %lld", (long long)n_q_rows, (long long)n_k_rows);
    FGR_REQUIRE(max_q_len >= 0 && max_q_len <= n_q_rows, "fgr_feature_nn: max_q_len = %d", max_q_len);
    FGR_REQUIRE(q_off && kv_off && kv_seg, "fgr_feature_nn: null segment table");
    if (n_q_rows == 0 || max_q_len == 0) return FGR_OK;
    FGR_REQUIRE(q && nn_idx && best && (k || n_k_rows == 0), "fgr_feature_nn: null operand");
    FGR_REQUIRE(((uintptr_t)q | (uintptr_t)k) % 16 == 0, "fgr_feature_nn: q and k must be 16-B aligned");
    hipStream_t st = as_stream(stream);
    const int n_blk = (max_q_len + 63) / 64;
    const dim3 grid((unsigned)((n_seg + 7) / 8 * 8 * n_blk));
    TimedCall timed(st);
    auto go = [&](auto kd) {
        launch_nn<decltype(kd)::value>(grid, st, q, k, d, q_off, kv_off, kv_seg, n_seg, n_blk, metric,
                                       nn_idx, best, second);
    };
    using std::integral_constant;
    const int kd_n = d / 32;       // the smallest register image that holds the row
    if (kd_n <= 1) go(integral_constant<int, 1>{});
    else if (kd_n <= 2) go(integral_constant<int, 2>{});
    else if (kd_n <= 4) go(integral_constant<int, 4>{});
    else if (kd_n <= 8) go(integral_constant<int, 8>{});
    else go(integral_constant<int, 16>{});
    FGR_CHECK_LAUNCH("fgr_feature_nn");
    return FGR_OK;
}

extern "C" int fgr_match_pairs(const int32_t* nn_idx, const float* best, const float* second,
                               const float* xyz, int64_t n_rows, const int64_t* off,
                               const int64_t* out_off, int32_t n_pairs, int32_t mode,
                               float max_ratio, const float* gt_pose, float inlier_dist, float* a,
                               float* b, float* w, int32_t* n_match, int32_t* n_inlier,
                               void* stream) {
    FGR_REQUIRE(n_pairs >= 1 && n_pairs <= 65535, "fgr_match_pairs: n_pairs = %d", n_pairs);
    FGR_REQUIRE(mode >= FGR_MATCH_SRC && mode <= FGR_MATCH_BILATERAL, "fgr_match_pairs: mode %d", mode);
    FGR_REQUIRE(n_rows >= 0 && n_rows < (int64_t)1 << 31, "fgr_match_pairs: n_rows = %lld", (long long)n_rows);
    FGR_REQUIRE(off && out_off && n_match, "fgr_match_pairs: null table or n_match");
    FGR_REQUIRE(n_rows == 0 || (nn_idx && xyz && a && b && w), "fgr_match_pairs: null operand");
    const bool ratio = max_ratio > 0.f;      // a NaN ratio is off
    FGR_REQUIRE(!ratio || n_rows == 0 || (best && second), "fgr_match_pairs: max_ratio needs best and second");
    FGR_REQUIRE((gt_pose != nullptr) == (n_inlier != nullptr), "fgr_match_pairs: gt_pose and n_inlier go together");
    FGR_REQUIRE(!gt_pose || (inlier_dist > 0.f && inlier_dist < INFINITY),
                "fgr_match_pairs: inlier_dist = %g", (double)inlier_dist);
    hipStream_t st = as_stream(stream);
    TimedCall timed(st);
    hipLaunchKernelGGL(match_pairs_kernel, dim3(n_pairs), dim3(256), 0, st, nn_idx, best, second, xyz,
                       off, out_off, n_pairs, mode, ratio ? max_ratio * max_ratio : 0.f, gt_pose,
                       gt_pose ? inlier_dist * inlier_dist : 0.f, a, b, w, n_match, n_inlier);
    FGR_CHECK_LAUNCH("fgr_match_pairs");
    return FGR_OK;
}
