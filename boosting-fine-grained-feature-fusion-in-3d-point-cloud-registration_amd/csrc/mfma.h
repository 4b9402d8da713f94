// Device helpers shared by the matrix-core kernels (gfx950 / CDNA4, wave64): vector types,
// reductions across the four 16-lane rows, the f16x3 scale exponents and MFMA trio, the XCD block order,
// the register-staged GEMMs' A unit load, s_waitcnt encodings and the GEMM epilogue of one
// output. One definition each; all force-inlined.
#pragma once
#include "common.h"

namespace fgr {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// ---- reductions over lanes c, c^16, c^32, c^48 (the four g rows of an MFMA lane map) on
// v_permlane16_swap / v_permlane32_swap (no LDS crossbar); every lane gets the result
__device__ __forceinline__ float x16_sum(float v) {       // v[l] + v[l^16]
    auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return __uint_as_float(a[0]) + __uint_as_float(a[1]);
}
__device__ __forceinline__ float x32_sum(float v) {       // v[l] + v[l^32]
    auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return __uint_as_float(b[0]) + __uint_as_float(b[1]);
}
__device__ __forceinline__ float xg_sum(float v) { return x32_sum(x16_sum(v)); }
__device__ __forceinline__ float xg_max(float v) {
    auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
    auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return fmaxf(__uint_as_float(b[0]), __uint_as_float(b[1]));
}
// Sum over all 64 lanes without the LDS crossbar: DPP within each 16-lane row, then across
// the four rows; every lane gets the total.
__device__ __forceinline__ float wave_sum_dpp(float v) { return xg_sum(row16_sum(v)); }

// maxima of MFMA results: plain fmaxf (their users are built -fno-honor-nans, so no NaN
// canonicalisation of the inputs; inline asm cannot be used here: the compiler's hazard
// recognizer does not see an asm block's reads of MFMA results)
__device__ __forceinline__ float vmax3(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }
__device__ __forceinline__ float vmax2(float a, float b) { return fmaxf(a, b); }

// ---- f16x3 scale exponents (the precision argument at the top of gemm16.hip rests on them)
// Row scale: the power-of-two exponent e that puts an operand row's (tile's) max |x| = mx
// into [2^14, 2^15), i.e. mx * 2^e in [2^14, 2^15); 0 for an all-zero row. Capped at 127 so
// 2^e stays a finite fp32.
__device__ __forceinline__ int row_scale_exp(float mx) {
    return mx > 0.f ? min(15 - __builtin_amdgcn_frexp_expf(mx), 127) : 0;
}
// Chunk rule of the k-looped kernels: for a 32-wide k chunk whose max |x| is cm > 0,
// cm * 2^sh in [2^7, 2^8)
__device__ __forceinline__ int chunk_shift(float cm) {
    return min(8 - __builtin_amdgcn_frexp_expf(cm), 127);
}
// a row's in-flight scale exponent before its first non-zero chunk (its partial sums are 0)
constexpr int SH_UNSET = 0x3fff;

// ---- the three significant products of an f16x3 16x16x32 step (A-operand terms wh + wl,
// B-operand terms ah + am), the small ones first
__device__ __forceinline__ void mma_h3(const f16x8& wh, const f16x8& wl, const f16x8& ah,
                                       const f16x8& am, f32x4& acc) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl, ah, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, am, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, ah, acc, 0, 0, 0);
}

// ---- XCD-aware block order: hardware dispatches block t to XCD t % 8; the bijective remap
// of 0..n-1 that gives each XCD a contiguous range of tiles (its L2 keeps what neighbouring
// tiles share)
__device__ __forceinline__ int xcd_tile(int t, int n) {
    const int q = n / 8, r = n % 8, x = t % 8, lo = t / 8;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + lo;
}

// ---- one A unit of the register-staged GEMMs: the 8 floats arow[k .. k+7] of an activation
// row of length K, zeros past K. KVEC (K % 8 == 0, 16-B aligned rows): two 16-B loads,
// address clamped into the row; else scalar loads, each clamped.
template <bool KVEC>
__device__ __forceinline__ void load_a8(const float* arow, int k, int K, float4 (&ar)[2]) {
    if constexpr (KVEC) {
        const float* src = arow + min(k, K - 8);
        const float4 x0 = *reinterpret_cast<const float4*>(src);
        const float4 x1 = *reinterpret_cast<const float4*>(src + 4);
        const bool ok = k < K;
        ar[0] = ok ? x0 : make_float4(0.f, 0.f, 0.f, 0.f);
        ar[1] = ok ? x1 : make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
        float tt[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float xv = arow[min(k + e, K - 1)];
            tt[e] = k + e < K ? xv : 0.f;
        }
        ar[0] = make_float4(tt[0], tt[1], tt[2], tt[3]);
        ar[1] = make_float4(tt[4], tt[5], tt[6], tt[7]);
    }
}

// ---- s_waitcnt immediates, gfx9 encoding: vmcnt = bits 3:0 and 15:14, expcnt = bits 6:4
// (7: no wait), lgkmcnt = bits 11:8 (15: no wait)
// s_waitcnt vmcnt(N) only
template <int N>
__device__ __forceinline__ void wait_vm() {
    static_assert(N >= 0 && N < 64, "vmcnt");
    __builtin_amdgcn_s_waitcnt((N & 15) | ((N >> 4) << 14) | (7 << 4) | (15 << 8));
}
// s_waitcnt vmcnt(N) lgkmcnt(0)
template <int N>
__device__ __forceinline__ void wait_vm_lgkm0() {
    static_assert(N >= 0 && N < 64, "vmcnt");
    __builtin_amdgcn_s_waitcnt((N & 15) | ((N >> 4) << 14) | (7 << 4));
}
// s_waitcnt lgkmcnt(0) only
__device__ __forceinline__ void wait_lgkm0() {
    __builtin_amdgcn_s_waitcnt((15) | (7 << 4) | (0 << 8) | (3 << 14));
}

// ---- GEMM epilogue of one output: act(y + b + r), or LeakyReLU_0.1(ReLU(y + b) + r) for
// FGR_ACT_RELU_RES_LEAKY (absent bias / residual come in as 0)
__device__ __forceinline__ float finish_out(float y, float b, float r, int act) {
    if (act == FGR_ACT_RELU_RES_LEAKY) {
        const float t = fmaxf(y + b, 0.f) + r;
        return t > 0.f ? t : 0.1f * t;
    }
    const float t = y + b + r;
    return act == FGR_ACT_RELU ? fmaxf(t, 0.f) : t;
}
// the same with the activation and the presence of a residual fixed at compile time
template <int ACT, bool RES>
__device__ __forceinline__ float finish_ct(float y, float b, float r) {
    if constexpr (ACT == FGR_ACT_RELU_RES_LEAKY) {
        float t = fmaxf(y + b, 0.f);
        if constexpr (RES) t += r;
        return t > 0.f ? t : 0.1f * t;
    } else {
        float t = y + b;
        if constexpr (RES) t += r;
        if constexpr (ACT == FGR_ACT_RELU) t = fmaxf(t, 0.f);
        return t;
    }
}

}  // namespace fgr
