// PositionEmbeddingLearned (position_embedding.py:52-71) in ONE launch: the five-layer per-point
// MLP with ReLU between layers,
//
//   out[r] = L4(ReLU(L3(ReLU(L2(ReLU(L1(ReLU(L0(xyz[r])))))))))     3 -> 32 -> 64 -> 128 -> 256 -> d
//
// Built from the existing parts it is five GEMM launches with four activation round trips to
// memory; here a block owns 16 RT whole rows (RT row tiles of 16) end to end and the hidden
// activations live in registers and LDS only.
//
//   * layer 0 (K = 3) is three fp32 FMAs per hidden unit: wave w < RT computes row tile w, lane
//     (g, c) the units 8 g + e (e = 0..7) of row c -- which is layer 1's B fragment;
//   * layers 1-4 are the fp32-accurate f16x3 products of gemm_rs.hip / ffn.hip (two fp16 terms
//     per operand, three v_mfma_f32_16x16x32_f16 term products) in the swapped orientation of
//     ffn.hip (weight fragment = MFMA A operand, activations = B operand). The waves split the
//     WEIGHTS, as ffn.hip's default version does: wave w owns a quarter of a layer's 16-column
//     output panels for all the block's rows, its weight fragments read straight from global
//     memory (L2) into registers -- each byte by one wave of the block only -- through a register
//     ring of kPmRing load groups (a group = one k32 step of a panel pair, both terms) that runs
//     across the layer boundaries (weights do not depend on activations);
//   * between layers the block's rows go through an LDS row image [row tile][k32 step][term]
//     [lane] x 16 B (at most 4 x 8 x 2 x 64 x 16 B = 64 KB): after a layer's MFMAs lane (g, c)
//     holds outputs 16 p + 4 g .. + 3 of row c for each of its panels p; bias + ReLU in
//     registers, then the row's maximum (the lane's, its three g partners', and the other
//     waves' through 1 KB of LDS), ONE power-of-two scale per row from that actual maximum
//     (max in [2^14, 2^15): no host-supplied bound), the split into the two fp16 terms, and an
//     8-B store of the lane's four k values into the image in natural k order: k = 16 p + 4 g + r
//     is element 4 (g & 1) + r of lane group 2 (p & 1) + (g >> 1) of k32 step p / 2. Two
//     barriers per layer (maxima; image), eight per launch;
//   * the last layer's panels are scaled, biased and stored as they finish (16-B stores).
//
// Every row's arithmetic is a fixed sequence that involves no other row (MFMA B columns are
// independent; the scales are per row), so a row's bits do not depend on the call's other rows,
// on its position, or on RT.
//
// Weight images: layers 1-4 take the plain fgr_split_weights_h3 images ([panel][k32 step]
// [term][g][16] x 16 B in natural k order, k32 steps padded to an even count -- layer 1's K = 32
// image carries one zero step that is skipped -- then the per-row inverse scales). Layer 0's
// weight and all biases are raw fp32.
#include "mfma.h"

namespace fgr {
namespace {


constexpr int kPmRing = 4;                       // register ring of load groups (3 in flight)

struct PosMlpArgs {
    const float* xyz; int64_t n;
    const float* w0; const float* b0;
    const u32x4* w[4]; const float* wsc[4]; const float* b[4];
    float* out; int64_t ldo;
};

// layer 1..4 -> index l = 0..3 (K = 32 << l): k32 steps used, k32 steps of the image (padded even)
__host__ __device__ constexpr int pm_ks(int l) { return 1 << l; }
__host__ __device__ constexpr int pm_ks_img(int l) { return l == 0 ? 2 : (1 << l); }
// output width, panels per wave, panels per load group, load groups of the layer (per wave)
__host__ __device__ constexpr int pm_n(int l, int d) { return l == 3 ? d : (64 << l); }
__host__ __device__ constexpr int pm_pw(int l, int d) { return pm_n(l, d) / 64; }
__host__ __device__ constexpr int pm_ppg(int l) { return l == 0 ? 1 : 2; }
__host__ __device__ constexpr int pm_groups(int l, int d) { return pm_pw(l, d) / pm_ppg(l) * pm_ks(l); }
__host__ __device__ constexpr int pm_base(int l, int d) {
    int b = 0;
    for (int i = 0; i < l; ++i) b += pm_groups(i, d);
    return b;
}

template <int D, int RT>
__global__ void __launch_bounds__(256, 1) pos_mlp_kernel(PosMlpArgs p) {
    static_assert(D == 256 || D == 512, "d_model");
    static_assert(RT == 1 || RT == 2 || RT == 4, "row tiles");
    __shared__ u32x4 act[RT * 8 * 2 * 64];                // [row tile][k32 step][term][lane]
    __shared__ float wmax[4][16 * RT];                    // [wave][row]: the waves' row maxima
    uint2* act2 = reinterpret_cast<uint2*>(act);

    constexpr int BR = 16 * RT;
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    const int g = lane >> 4, c = lane & 15;
    const int64_t r0 = (int64_t)blockIdx.x * BR;

    // load group f (flat over the layers, compile-time after unrolling) into a ring slot:
    // layer l, panel group pg, k32 step s: panels wv PW + pg PPG + pp, both terms
    auto issue = [&](int f, u32x4 (&slot)[4]) {
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            if (f >= pm_base(l, D) && f < pm_base(l, D) + pm_groups(l, D)) {
                const int j = f - pm_base(l, D), pg = j / pm_ks(l), s = j % pm_ks(l);
#pragma unroll
                for (int e = 0; e < 2 * pm_ppg(l); ++e) {
                    const int q = wv * pm_pw(l, D) + pg * pm_ppg(l) + (e >> 1);
                    slot[e] = p.w[l][((q * pm_ks_img(l) + s) * 2 + (e & 1)) * 64 + lane];
                }
            }
        }
    };
    u32x4 ring[kPmRing][4];
#pragma unroll
    for (int f = 0; f < kPmRing - 1; ++f) issue(f, ring[f]);

    // layer 0 in fp32: wave wv < RT, lane (g, c): units 8 g + e of row r0 + 16 wv + c
    if (wv < RT) {
        const int64_t row = min(r0 + 16 * wv + c, p.n - 1);
        const float x = p.xyz[3 * row], y = p.xyz[3 * row + 1], z = p.xyz[3 * row + 2];
        float h[8];
        float mx = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int j = 8 * g + e;
            const float v = fmaf(p.w0[3 * j + 2], z, fmaf(p.w0[3 * j + 1], y, fmaf(p.w0[3 * j], x, p.b0[j])));
            h[e] = fmaxf(v, 0.f);
            mx = fmaxf(mx, h[e]);
        }
        const int ea = row_scale_exp(xg_max(mx));
        u32x4 hi, lo;
        split8_f16(h, __builtin_ldexpf(1.f, ea), hi, lo);
        act[((wv * 8 + 0) * 2 + 0) * 64 + lane] = hi;
        act[((wv * 8 + 0) * 2 + 1) * 64 + lane] = lo;
        if (g == 0) wmax[0][16 * wv + c] = __builtin_ldexpf(1.f, -ea);   // the row's 1 / scale
    }
    __syncthreads();
    float inv_sc[RT];                                     // 1 / scale of the image's rows (row c)
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) inv_sc[rt] = wmax[0][16 * rt + c];
    __syncthreads();                                      // wmax is rewritten below

    // layers 1..4
#pragma unroll
    for (int l = 0; l < 4; ++l) {
        const int PW = pm_pw(l, D), PPG = pm_ppg(l), KS = pm_ks(l), base = pm_base(l, D);
        const bool last = l == 3;
        f32x4 hid[RT][4];                                 // a hidden layer's outputs (PW <= 4)
#pragma unroll
        for (int pg = 0; pg < PW / PPG; ++pg) {
            f32x4 acc[RT][2];
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) acc[rt][0] = acc[rt][1] = f32x4{0.f, 0.f, 0.f, 0.f};
            float4 cw[2], cb[2];                          // the panels' column scales and bias
#pragma unroll
            for (int pp = 0; pp < PPG; ++pp) {
                const int n = 16 * (wv * PW + pg * PPG + pp) + 4 * g;
                cw[pp] = *reinterpret_cast<const float4*>(p.wsc[l] + n);
                cb[pp] = *reinterpret_cast<const float4*>(p.b[l] + n);
            }
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const int f = base + pg * KS + s;
                issue(f + kPmRing - 1, ring[(f + kPmRing - 1) % kPmRing]);
                u32x4 (&wf)[4] = ring[f % kPmRing];
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) {
                    const f16x8 ah = __builtin_bit_cast(f16x8, act[((rt * 8 + s) * 2 + 0) * 64 + lane]);
                    const f16x8 al = __builtin_bit_cast(f16x8, act[((rt * 8 + s) * 2 + 1) * 64 + lane]);
#pragma unroll
                    for (int pp = 0; pp < PPG; ++pp) {
                        const f16x8 wh = __builtin_bit_cast(f16x8, wf[2 * pp]);
                        const f16x8 wl = __builtin_bit_cast(f16x8, wf[2 * pp + 1]);
                        acc[rt][pp] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl, ah, acc[rt][pp], 0, 0, 0);
                        acc[rt][pp] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, al, acc[rt][pp], 0, 0, 0);
                        acc[rt][pp] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, ah, acc[rt][pp], 0, 0, 0);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);        // nothing crosses groups
            }
            // the group's panels: y = acc wsc[n] / scale_row + b[n], lane (g, c): n = 16 q + 4 g + r
#pragma unroll
            for (int pp = 0; pp < PPG; ++pp) {
                const int n = 16 * (wv * PW + pg * PPG + pp) + 4 * g;
                const float4 w4 = cw[pp], b4 = cb[pp];
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) {
                    const f32x4 a = acc[rt][pp];
                    const float is = inv_sc[rt];
                    f32x4 y = f32x4{fmaf(a[0], w4.x * is, b4.x), fmaf(a[1], w4.y * is, b4.y),
                                    fmaf(a[2], w4.z * is, b4.z), fmaf(a[3], w4.w * is, b4.w)};
                    if (last) {
                        const int64_t rr = r0 + 16 * rt + c;
                        if (rr < p.n)
                            *reinterpret_cast<float4*>(p.out + rr * p.ldo + n) =
                                make_float4(y[0], y[1], y[2], y[3]);
                    } else {
                        hid[rt][(pg * PPG + pp) & 3] = f32x4{fmaxf(y[0], 0.f), fmaxf(y[1], 0.f),
                                                             fmaxf(y[2], 0.f), fmaxf(y[3], 0.f)};
                    }
                }
            }
        }
        if (!last) {
            // the rows' maxima over this wave's panels, then over the waves
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                float mx = 0.f;
#pragma unroll
                for (int q = 0; q < PW; ++q)
                    mx = fmaxf(mx, fmaxf(fmaxf(hid[rt][q & 3][0], hid[rt][q & 3][1]),
                                         fmaxf(hid[rt][q & 3][2], hid[rt][q & 3][3])));
                mx = xg_max(mx);
                if (g == 0) wmax[wv][16 * rt + c] = mx;
            }
            __syncthreads();            // maxima visible; every wave is done reading the image
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                const int rc = 16 * rt + c;
                const float mx = fmaxf(fmaxf(wmax[0][rc], wmax[1][rc]), fmaxf(wmax[2][rc], wmax[3][rc]));
                const int ea = row_scale_exp(mx);
                inv_sc[rt] = __builtin_ldexpf(1.f, -ea);
                const float sc = __builtin_ldexpf(1.f, ea);
#pragma unroll
                for (int q2 = 0; q2 < PW; q2 += 2) {
                    // two panels' values (8) per split; PW = 1 (layer 1): the second half is unused
                    const bool two = q2 + 1 < PW;
                    const f32x4 v0 = hid[rt][q2 & 3], v1 = two ? hid[rt][(q2 + 1) & 3] : f32x4{0.f, 0.f, 0.f, 0.f};
                    const float hv[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
                    u32x4 hi, lo;
                    split8_f16(hv, sc, hi, lo);
#pragma unroll
                    for (int pp = 0; pp < (two ? 2 : 1); ++pp) {
                        const int q = wv * PW + q2 + pp;          // k = 16 q + 4 g + r
                        const int s = q >> 1, gl = 2 * (q & 1) + (g >> 1);
                        const int u = ((rt * 8 + s) * 2 + 0) * 64 + gl * 16 + c;   // 16-B unit, term 0
                        act2[2 * u + (g & 1)] = make_uint2(hi[2 * pp], hi[2 * pp + 1]);
                        act2[2 * (u + 64) + (g & 1)] = make_uint2(lo[2 * pp], lo[2 * pp + 1]);
                    }
                }
            }
            __syncthreads();            // the next layer's image complete; wmax free again
        }
    }
}

template <int D>
void pos_mlp_launch(const PosMlpArgs& a, hipStream_t st) {
    // rows per block: the fewest row tiles (most blocks) that still fit one round of the CUs
    constexpr int64_t kCus = 256;
    const int64_t n = a.n;
    if ((n + 15) / 16 <= kCus)
        hipLaunchKernelGGL((pos_mlp_kernel<D, 1>), dim3((unsigned)((n + 15) / 16)), dim3(256), 0, st, a);
    else if ((n + 31) / 32 <= kCus)
        hipLaunchKernelGGL((pos_mlp_kernel<D, 2>), dim3((unsigned)((n + 31) / 32)), dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL((pos_mlp_kernel<D, 4>), dim3((unsigned)((n + 63) / 64)), dim3(256), 0, st, a);
}

}  // namespace
}  // namespace fgr

using namespace fgr;

extern "C" int fgr_pos_mlp_f16x3_supported(int64_t n, int32_t d_model) {
    return (n >= 1 && n <= (int64_t)0x7fffffff * 16 && (d_model == 256 || d_model == 512)) ? 1 : 0;
}

extern "C" int fgr_pos_mlp_f16x3(const float* xyz, int64_t n, const float* w0, const float* b0,
                                 const void* w1_img, const float* b1, const void* w2_img,
                                 const float* b2, const void* w3_img, const float* b3,
                                 const void* w4_img, const float* b4, int32_t d_model, float* out,
                                 int64_t ldo, void* stream) {
    FGR_REQUIRE(n >= 0 && ldo >= d_model, "fgr_pos_mlp_f16x3: bad arguments (n %lld, ldo %lld)",
                (long long)n, (long long)ldo);
    FGR_REQUIRE(d_model == 256 || d_model == 512,
                "fgr_pos_mlp_f16x3: d_model %d not supported (256 or 512: fgr_pos_mlp_f16x3_supported)",
                d_model);
    FGR_REQUIRE(w0 && b0 && w1_img && b1 && w2_img && b2 && w3_img && b3 && w4_img && b4,
                "fgr_pos_mlp_f16x3: null weight pointer");
    FGR_REQUIRE(n == 0 || (xyz && out), "fgr_pos_mlp_f16x3: null pointer");
    FGR_REQUIRE(n == 0 || fgr_pos_mlp_f16x3_supported(n, d_model),
                "fgr_pos_mlp_f16x3: n %lld not supported", (long long)n);
    const uintptr_t al = reinterpret_cast<uintptr_t>(w1_img) | reinterpret_cast<uintptr_t>(b1) |
                         reinterpret_cast<uintptr_t>(w2_img) | reinterpret_cast<uintptr_t>(b2) |
                         reinterpret_cast<uintptr_t>(w3_img) | reinterpret_cast<uintptr_t>(b3) |
                         reinterpret_cast<uintptr_t>(w4_img) | reinterpret_cast<uintptr_t>(b4) |
                         reinterpret_cast<uintptr_t>(out);
    FGR_REQUIRE((al & 15) == 0 && ldo % 4 == 0,
                "fgr_pos_mlp_f16x3: images, b1..b4 and out must be 16-B aligned, ldo %% 4 == 0");
    if (n == 0) return FGR_OK;
    hipStream_t st = as_stream(stream);
    TimedCall timed_(st);
    PosMlpArgs a;
    a.xyz = xyz; a.n = n; a.w0 = w0; a.b0 = b0; a.out = out; a.ldo = ldo;
    const void* imgs[4] = {w1_img, w2_img, w3_img, w4_img};
    const float* bs[4] = {b1, b2, b3, b4};
    for (int l = 0; l < 4; ++l) {
        // fgr_split_weights_h3 of (N, K): N / 16 panels x (padded) k32 steps x 128 units, then scales
        const char* im = static_cast<const char*>(imgs[l]);
        a.w[l] = reinterpret_cast<const u32x4*>(im);
        a.wsc[l] = reinterpret_cast<const float*>(
            im + (size_t)(pm_n(l, d_model) / 16) * pm_ks_img(l) * 128 * 16);
        a.b[l] = bs[l];
    }
    if (d_model == 256) pos_mlp_launch<256>(a, st);
    else pos_mlp_launch<512>(a, st);
    FGR_CHECK_LAUNCH("pos_mlp_kernel");
    return FGR_OK;
}
