// Fused Res2Net hierarchy (the "fine-grained feature fusion" of my_Bottle2neck,
// res2net.py:126-148) on the split matrix cores.
//
// Given h = ReLU(BN1(conv1(x))) split into `scale` chunks of width w, computes in one
// launch, for i < nums (= scale - 1):
//   sp_i = ReLU(BN_i(conv_i(sp_{i-1} + h_i)))      (sp_{-1} = 0)
// with BN folded into (W_i, b_i) on the host, and writes the concatenation input of
// conv3 + downsample: cat = [sp_0 .. sp_{nums-1} | h_{nums..scale-1} | x].
// The reference runs this as 7 dependent (Linear, BN, ReLU) triples plus adds and a
// cat (21+ launches over HBM); here sp never leaves the chip between steps.
// Two fp32-accurate variants: fgr_res2net_chain6 (three exact bf16 terms, six products;
// w = 112, 224 -- dispatched at w = 224, where it measured faster) and fgr_res2net_chain_h3
// (scaled split fp16, three products; w % 4 == 0 up to 224).
#include "mfma.h"

namespace fgr {
namespace {

// dst[r0 + row][0..cols) = src[r0 + row][0..cols) for row < rows (rows past n skipped): the
// concatenation tail of the chain kernels. 16-B accesses when every row start is 16-B aligned,
// kCpU of them in flight per thread: every load unconditional (element index and row clamped
// to valid ones, the store masked) -- round 5: guarded loads had put the staging array in
// scratch with a vmcnt(0) wait after each load, one memory round trip per float4
constexpr int kCpU = 8;
__device__ __forceinline__ void copy_rows(float* __restrict__ dst, int64_t ldd,
                                          const float* __restrict__ src, int64_t lds, int64_t r0,
                                          int rows, int64_t n, int cols, int tid, int nth) {
    const bool v4 = ((cols | (int)(ldd & 3) | (int)(lds & 3)) & 3) == 0 &&
                    ((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src)) & 15) == 0;
    if (v4) {
        const int c4 = cols / 4;
        const int nr = (int)min<int64_t>(rows, n - r0);   // rows of this block below n
        if (nr <= 0 || c4 == 0) return;
        const int tot = nr * c4;
        for (int e0 = tid; e0 < tot; e0 += kCpU * nth) {
            float4 v[kCpU];
#pragma unroll
            for (int u = 0; u < kCpU; ++u) {
                const int e = min(e0 + u * nth, tot - 1);
                const int row = e / c4, cc = (e - row * c4) * 4;
                v[u] = *reinterpret_cast<const float4*>(src + (r0 + row) * lds + cc);
            }
#pragma unroll
            for (int u = 0; u < kCpU; ++u) {
                const int e = e0 + u * nth;
                if (e < tot) {
                    const int row = e / c4, cc = (e - row * c4) * 4;
                    *reinterpret_cast<float4*>(dst + (r0 + row) * ldd + cc) = v[u];
                }
            }
        }
        return;
    }
    for (int e = tid; e < rows * cols; e += nth) {
        const int row = e / cols, cc = e - row * cols;
        if (r0 + row < n) dst[(r0 + row) * ldd + cc] = src[(r0 + row) * lds + cc];
    }
}

constexpr int kRows = 32;

// ------------------------------------------------------------------------------------
// bf16x6 variant (fp32-accurate): the hierarchy on the bf16 matrix cores, every fp32 value
// split exactly into three bf16 terms h + m + l (residual <= 2^-27 |x|), the six products
// hh + hm + mh + hl + lh + mm accumulated in fp32. Per step the A operand
// a = sp_{i-1} + h_i is formed in fp32, split and stored as fragment-ordered LDS images
//   img[t][ks][g][row] (16-B units: row, k = 32 ks + 8 g .. + 7),
// read with conflict-free ds_read_b128; sp_i stays in an fp32 LDS tile between steps.
// W_i comes pre-split from the host in fragment order [i][jt][ks][t][g][c][8] (1 KB per
// wave-load), streamed two k-steps ahead. K is padded to a multiple of 32 (w = 112 -> 128)
// with zero weights and zero A columns. 2 barriers per step (build | MFMA + epilogue).
// ------------------------------------------------------------------------------------

__device__ __forceinline__ void split3(float x, __bf16& h, __bf16& m, __bf16& l) {
    h = (__bf16)x;
    const float r = x - (float)h;
    m = (__bf16)r;
    l = (__bf16)(r - (float)m);
}

// R rows per block (16, 32 or 48: R / 16 row fragments per wave; 48 puts ModelNet's 9544
// rows in 199 blocks -- one round of one 14-wave block per CU -- instead of 256 + 43, 16
// spreads 3DMatch's ~2k rows over twice the CUs)
template <int KT, int R = kRows>   // KT = w / 16 column tiles (= waves); KS = ceil(w / 32) k-steps
__global__ void __launch_bounds__(64 * KT)
res2net_chain6_kernel(const float* __restrict__ h, int64_t n, int scale, int nums,
                      const u32x4* __restrict__ wf, const float* __restrict__ bias,
                      const float* __restrict__ x, int cin, float* __restrict__ cat, int64_t ld) {
    constexpr int W = 16 * KT, KS = (W + 31) / 32, NU = R * KS * 4;   // A units per term
    // sp rows padded to W + 4 floats: at a stride of W (a multiple of 32 floats here) the
    // build's reads -- consecutive lanes on consecutive rows -- hit 2-4 of the 64 LDS banks
    // (16-32-way conflicts); at W + 4 the 16-B reads of a wave spread over all of them
    constexpr int SPW = W + 4;
    __shared__ u32x4 img[3 * NU];
    __shared__ float sp[R * SPW];
    const int tid = threadIdx.x, nth = 64 * KT;
    const int wv = tid / 64, lane = tid % 64, g = lane >> 4, c = lane & 15;
    const int64_t r0 = (int64_t)blockIdx.x * R;
    const int64_t hw = (int64_t)scale * W;
    const int col = wv * 16 + c;

    for (int i = 0; i < nums; ++i) {
        const u32x4* wb = wf + (((int64_t)i * KT + wv) * KS) * 192 + lane;
        u32x4 bq[3][3];                                // ring: k-steps ks, ks+1, ks+2
#pragma unroll
        for (int q = 0; q < 2; ++q)
            if (q < KS) {
#pragma unroll
                for (int t = 0; t < 3; ++t) bq[q][t] = wb[(q * 3 + t) * 64];
            }
        const float bc = bias[i * W + col];
        // build the split A images: unit u -> (row = u % 32, kg = u / 32), 8 k each
        for (int u = tid; u < NU; u += nth) {
            const int row = u % R, kg = u / R;       // kg = 4 ks + g'
            const int k0 = 8 * kg;
            float a[8];
            const int64_t gr = r0 + row;
#pragma unroll
            for (int e = 0; e < 8; e += 4) {
                float4 hv = make_float4(0.f, 0.f, 0.f, 0.f);
                if (gr < n && k0 + e < W)
                    hv = *reinterpret_cast<const float4*>(h + gr * hw + (int64_t)i * W + k0 + e);
                a[e] = hv.x; a[e + 1] = hv.y; a[e + 2] = hv.z; a[e + 3] = hv.w;
            }
            if (i > 0 && k0 < W) {                      // k0 + 8 <= W: W % 16 == 0
                const float4 s0 = *reinterpret_cast<const float4*>(sp + row * SPW + k0);
                const float4 s1 = *reinterpret_cast<const float4*>(sp + row * SPW + k0 + 4);
                a[0] += s0.x; a[1] += s0.y; a[2] += s0.z; a[3] += s0.w;
                a[4] += s1.x; a[5] += s1.y; a[6] += s1.z; a[7] += s1.w;
            }
            bf16x8 th, tm, tl;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                __bf16 hh, mm, ll;
                split3(a[e], hh, mm, ll);
                th[e] = hh; tm[e] = mm; tl[e] = ll;
            }
            img[0 * NU + kg * R + row] = __builtin_bit_cast(u32x4, th);
            img[1 * NU + kg * R + row] = __builtin_bit_cast(u32x4, tm);
            img[2 * NU + kg * R + row] = __builtin_bit_cast(u32x4, tl);
        }
        __syncthreads();
        constexpr int RF = R / 16;
        f32x4 acc[RF];
#pragma unroll
        for (int f = 0; f < RF; ++f) acc[f] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            if (ks + 2 < KS) {
#pragma unroll
                for (int t = 0; t < 3; ++t) bq[(ks + 2) % 3][t] = wb[((ks + 2) * 3 + t) * 64];
            }
            const bf16x8 bh = __builtin_bit_cast(bf16x8, bq[ks % 3][0]);
            const bf16x8 bm = __builtin_bit_cast(bf16x8, bq[ks % 3][1]);
            const bf16x8 bl = __builtin_bit_cast(bf16x8, bq[ks % 3][2]);
            const int base = (ks * 4 + g) * R;
            bf16x8 ah[RF], am[RF], al[RF];
#pragma unroll
            for (int f = 0; f < RF; ++f) {
                ah[f] = __builtin_bit_cast(bf16x8, img[0 * NU + base + 16 * f + c]);
                am[f] = __builtin_bit_cast(bf16x8, img[1 * NU + base + 16 * f + c]);
                al[f] = __builtin_bit_cast(bf16x8, img[2 * NU + base + 16 * f + c]);
            }
            // the six products of three-term bf16 splits, smallest first
#pragma unroll
            for (int f = 0; f < RF; ++f) acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(am[f], bm, acc[f], 0, 0, 0);
#pragma unroll
            for (int f = 0; f < RF; ++f) acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[f], bh, acc[f], 0, 0, 0);
#pragma unroll
            for (int f = 0; f < RF; ++f) acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[f], bl, acc[f], 0, 0, 0);
#pragma unroll
            for (int f = 0; f < RF; ++f) acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(am[f], bh, acc[f], 0, 0, 0);
#pragma unroll
            for (int f = 0; f < RF; ++f) acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[f], bm, acc[f], 0, 0, 0);
#pragma unroll
            for (int f = 0; f < RF; ++f) acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[f], bh, acc[f], 0, 0, 0);
        }
        // epilogue: sp_i -> cat and the fp32 LDS tile (read by the next step's build,
        // which starts after the barrier below)
#pragma unroll
        for (int rg = 0; rg < RF; ++rg) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = rg * 16 + 4 * g + r;
                const float y = fmaxf(acc[rg][r] + bc, 0.f);
                if (r0 + row < n) cat[(r0 + row) * ld + (int64_t)i * W + col] = y;
                sp[row * SPW + col] = y;
            }
        }
        __syncthreads();
    }
    copy_rows(cat + (int64_t)nums * W, ld, h + (int64_t)nums * W, hw, r0, R, n,
              (scale - nums) * W, tid, nth);
    if (x) copy_rows(cat + hw, ld, x, cin, r0, R, n, cin, tid, nth);
}

// ------------------------------------------------------------------------------------
// f16x3 variant (scaled two-term fp16 splits, see gemm16.hip): the same hierarchy at half
// the matrix-core work of bf16x6. Swapped products (C^T = W a^T: W_i fragments as the A
// operand, activation rows as the B operand) so each lane owns ONE activation row and
// four output columns. Each step forms a = sp_{i-1} + h_i for the block's 32 rows, takes
// the row max (LDS atomics: the whole row is on chip, so the scale is exact per row, no
// online rescaling), scales the row by 2^e (max in [2^14, 2^15)) and splits it into fp16
// (h, m) images img[t][ks][g][row]; W_i rows come pre-scaled per output column with their
// inverse scales wsc[i][col] (fgreg.ops.res2net_fragments_h3).
// ------------------------------------------------------------------------------------

// R rows per block (32, or 48 at w = 224 when that saves a round of blocks, as in chain6).
// Each step issues the whole step's W_i fragments (KS x 2 per lane) before the build, so the
// matrix-core loop never waits on L2; rmax is double-buffered (reset in the previous step's
// epilogue): 3 barriers per step.
template <int KT, int R = kRows>
__global__ void __launch_bounds__(64 * KT)
res2net_chain_h3_kernel(const float* __restrict__ h, int64_t n, int w, int scale, int nums,
                        const u32x4* __restrict__ wf, const float* __restrict__ wsc,
                        const float* __restrict__ bias, const float* __restrict__ x, int cin,
                        float* __restrict__ cat, int64_t ld) {
    // W = the width padded to whole 16-column tiles (one wave each); w <= W the real width
    // (w % 4 == 0): columns past w carry zero weights and are never stored
    constexpr int W = 16 * KT, KS = (W + 31) / 32, NU = R * KS * 4;       // A units per term
    constexpr int IT = (NU + 64 * KT - 1) / (64 * KT);                    // build units / thread
    constexpr int RF = R / 16;                                            // row fragments
    constexpr int SPW = W + 4;                 // padded sp rows (bank spread, as in chain6)
    __shared__ u32x4 img[2 * NU];
    __shared__ float sp[R * SPW];
    __shared__ int rmax[2][R];
    const int tid = threadIdx.x, nth = 64 * KT;
    const int wv = tid / 64, lane = tid % 64, g = lane >> 4, c = lane & 15;
    const int64_t r0 = (int64_t)blockIdx.x * R;
    const int64_t hw = (int64_t)scale * w;
    const int col0 = wv * 16 + 4 * g;                  // this lane's 4 output columns
    const bool col_ok = col0 < w;
    if (tid < R) rmax[0][tid] = 0;
    __syncthreads();

    for (int i = 0; i < nums; ++i) {
        int* rm = rmax[i & 1];
        const u32x4* wb = wf + (((int64_t)i * KT + wv) * KS) * 128 + lane;
        u32x4 bq[KS][2];
#pragma unroll
        for (int q = 0; q < KS; ++q)
#pragma unroll
            for (int t = 0; t < 2; ++t) bq[q][t] = wb[(q * 2 + t) * 64];
        const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 wsv = col_ok ? *reinterpret_cast<const float4*>(wsc + i * w + col0) : z4;
        const float4 bc = col_ok ? *reinterpret_cast<const float4*>(bias + i * w + col0) : z4;
        // a = sp_{i-1} + h_i: unit u -> (row = u % R, kg = u / R), 8 k each
        float a[IT][8];
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int u = tid + nth * it;
            const int row = u % R, kg = u / R, k0 = 8 * kg;
            const int64_t gr = r0 + row;
#pragma unroll
            for (int e = 0; e < 8; e += 4) {
                float4 hv = make_float4(0.f, 0.f, 0.f, 0.f);
                if (u < NU && gr < n && k0 + e < w)
                    hv = *reinterpret_cast<const float4*>(h + gr * hw + (int64_t)i * w + k0 + e);
                a[it][e] = hv.x; a[it][e + 1] = hv.y; a[it][e + 2] = hv.z; a[it][e + 3] = hv.w;
            }
        }
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int u = tid + nth * it;
            const int row = u % R, kg = u / R, k0 = 8 * kg;
            float cm = 0.f;
            if (i > 0 && u < NU && k0 < W) {            // k0 < W => k0 + 8 <= W (W % 16 == 0)
                // sp columns in [w, W) hold 0 (zero weights and bias there); units at k0 >= W
                // are the k32 steps' padding past W (no sp columns)
                const float4 s0 = *reinterpret_cast<const float4*>(sp + row * SPW + k0);
                const float4 s1 = *reinterpret_cast<const float4*>(sp + row * SPW + k0 + 4);
                a[it][0] += s0.x; a[it][1] += s0.y; a[it][2] += s0.z; a[it][3] += s0.w;
                a[it][4] += s1.x; a[it][5] += s1.y; a[it][6] += s1.z; a[it][7] += s1.w;
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) cm = fmaxf(cm, fabsf(a[it][e]));
            if (u < NU && cm > 0.f) atomicMax(&rm[row], __float_as_int(cm));
        }
        __syncthreads();
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int u = tid + nth * it;
            if (u >= NU) break;
            const int row = u % R, kg = u / R;
            const float mx = __int_as_float(rm[row]);
            const float s = __builtin_ldexpf(1.f, row_scale_exp(mx));
            f16x8 th, tm;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float xs = a[it][e] * s;
                const _Float16 hh = (_Float16)xs;
                th[e] = hh;
                tm[e] = (_Float16)(xs - (float)hh);
            }
            img[0 * NU + kg * R + row] = __builtin_bit_cast(u32x4, th);
            img[1 * NU + kg * R + row] = __builtin_bit_cast(u32x4, tm);
        }
        __syncthreads();
        f32x4 acc[RF];
#pragma unroll
        for (int f = 0; f < RF; ++f) acc[f] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const f16x8 wh = __builtin_bit_cast(f16x8, bq[ks][0]);
            const f16x8 wl = __builtin_bit_cast(f16x8, bq[ks][1]);
            const int base = (ks * 4 + g) * R;
            f16x8 ah[RF], am[RF];
#pragma unroll
            for (int f = 0; f < RF; ++f) {
                ah[f] = __builtin_bit_cast(f16x8, img[0 * NU + base + 16 * f + c]);
                am[f] = __builtin_bit_cast(f16x8, img[1 * NU + base + 16 * f + c]);
            }
#pragma unroll
            for (int f = 0; f < RF; ++f) acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl, ah[f], acc[f], 0, 0, 0);
#pragma unroll
            for (int f = 0; f < RF; ++f) acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, am[f], acc[f], 0, 0, 0);
#pragma unroll
            for (int f = 0; f < RF; ++f) acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, ah[f], acc[f], 0, 0, 0);
        }
        // epilogue: lane (g, c) holds sp_i[row rg * 16 + c][cols col0 .. col0 + 3]
#pragma unroll
        for (int rg = 0; rg < RF; ++rg) {
            const int row = rg * 16 + c;
            const float mx = __int_as_float(rm[row]);
            // (the outer test repeats row_scale_exp's own: the negation stays inside the select)
            const float rs = __builtin_ldexpf(1.f, mx > 0.f ? -row_scale_exp(mx) : 0);
            const f32x4 av = acc[rg];
            float4 y;
            y.x = fmaxf(av[0] * rs * wsv.x + bc.x, 0.f);
            y.y = fmaxf(av[1] * rs * wsv.y + bc.y, 0.f);
            y.z = fmaxf(av[2] * rs * wsv.z + bc.z, 0.f);
            y.w = fmaxf(av[3] * rs * wsv.w + bc.w, 0.f);
            if (r0 + row < n && col_ok)
                *reinterpret_cast<float4*>(cat + (r0 + row) * ld + (int64_t)i * w + col0) = y;
            *reinterpret_cast<float4*>(sp + row * SPW + col0) = y;
        }
        if (tid < R) rmax[(i + 1) & 1][tid] = 0;       // next step's row maxima
        __syncthreads();
    }
    copy_rows(cat + (int64_t)nums * w, ld, h + (int64_t)nums * w, hw, r0, R, n,
              (scale - nums) * w, tid, nth);
    if (x) copy_rows(cat + hw, ld, x, cin, r0, R, n, cin, tid, nth);
}

// ------------------------------------------------------------------------------------
// Whole bottleneck front (conv1 + hierarchy + concat) in one launch, f16x3: the chain above
// with h = ReLU(x W1^T + b1) computed on chip instead of read from memory. The block's x
// tile (R rows x CIN) is loaded ONCE: its exact row maxima give one power-of-two scale per
// row, the scaled rows are split into two fp16 terms (the recipe of gemm_rs.hip: products
// lo.hi, hi.lo, hi.hi, fp32 accumulation, scales in the epilogue) and kept as a second LDS
// image ximg[t][ks][g][row], and the same registers write the x columns of cat. conv1 has
// the chain's orientation (W1 fragments as the A operand), so chunk i + 1 lands in the lane
// layout of the chain's accumulator: step i issues its MFMAs right after the wave's share of
// the split, before the barrier (they need neither the sp tile nor the images, and the matrix
// pipe is otherwise idle in that phase: 37.6 us per launch at 11472 rows against 38.9 with
// them inside the chain's k-loop), and the epilogue writes a_{i+1} = sp_i + h_{i+1} into the
// fp32 sp tile and folds its row maximum with the same LDS atomicMax. The build of step i + 1 then reads only
// LDS: no dependent memory load per step, 2 barriers per step, and h never exists in memory
// (its last chunk goes straight to cat). W1 comes as the image of
// fgreg.ops.res2net_conv1_fragments: [jt = chunk * KT + tile][ks][term][g][c][8], 1 KB per
// wave-load, read a whole chunk ahead. The chain's accumulators see the MFMA sequence of
// res2net_chain_h3_kernel.
// ------------------------------------------------------------------------------------
// (7 waves: 4 waves per SIMD, i.e. <= 128 registers, keeps two blocks per CU as the chain has)
template <int KT, int KSX, int R = kRows>     // CIN = 32 KSX
__global__ void __launch_bounds__(64 * KT, KT == 7 ? 4 : 1)
res2net_block_h3_kernel(const float* __restrict__ x, int64_t n, int w, int scale,
                        const u32x4* __restrict__ w1f, const float* __restrict__ w1sc,
                        const float* __restrict__ b1, const u32x4* __restrict__ wf,
                        const float* __restrict__ wsc, const float* __restrict__ bias,
                        float* __restrict__ cat, int64_t ld) {
    constexpr int W = 16 * KT, KS = (W + 31) / 32, NU = R * KS * 4, NTH = 64 * KT;
    constexpr int CIN = 32 * KSX, NUX = R * KSX * 4;                      // x units per term
    constexpr int IT = (NU + NTH - 1) / NTH, ITX = (NUX + NTH - 1) / NTH;
    constexpr int RF = R / 16, SPW = W + 4;
    __shared__ u32x4 img[2 * NU];
    __shared__ u32x4 ximg[2 * NUX];
    __shared__ float sp[R * SPW];              // a_i = sp_{i-1} + h_i between steps
    __shared__ int rmax[2][R];
    __shared__ int xmax[R];
    const int tid = threadIdx.x;
    const int wv = tid / 64, lane = tid % 64, g = lane >> 4, c = lane & 15;
    const int64_t r0 = (int64_t)blockIdx.x * R;
    const int64_t hw = (int64_t)scale * w;
    const int nums = scale - 1;
    const int col0 = wv * 16 + 4 * g;                  // this lane's 4 output columns
    const bool col_ok = col0 < w;
    if (tid < R) { rmax[0][tid] = 0; rmax[1][tid] = 0; xmax[tid] = 0; }

    // conv1 operands of chunk j: W1 fragments (every k-step), inverse scales, bias
    u32x4 w1q[KSX][2];
    float4 w1sv, b1v;
    auto load_w1 = [&](int j) {
        const u32x4* wb = w1f + (((int64_t)j * KT + wv) * KSX) * 128 + lane;
#pragma unroll
        for (int q = 0; q < KSX; ++q)
#pragma unroll
            for (int t = 0; t < 2; ++t) w1q[q][t] = wb[(q * 2 + t) * 64];
        w1sv = b1v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (col_ok) {
            w1sv = ld4(w1sc + (int64_t)j * w + col0);
            b1v = ld4(b1 + (int64_t)j * w + col0);
        }
    };
    load_w1(0);
    __syncthreads();

    // ---- the x tile: unit u -> (row = u % R, kg = u / R), 8 k each
    {
        float xa[ITX][8];
#pragma unroll
        for (int it = 0; it < ITX; ++it) {
            const int u = tid + NTH * it;
            const int row = u % R, kg = u / R;
            const int64_t gr = r0 + row;
#pragma unroll
            for (int e = 0; e < 8; e += 4) {
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (u < NUX && gr < n) v = ld4(x + gr * CIN + 8 * kg + e);
                xa[it][e] = v.x; xa[it][e + 1] = v.y; xa[it][e + 2] = v.z; xa[it][e + 3] = v.w;
            }
        }
#pragma unroll
        for (int it = 0; it < ITX; ++it) {
            const int u = tid + NTH * it;
            const int row = u % R, kg = u / R;
            const int64_t gr = r0 + row;
            if (u < NUX && gr < n) {                    // the x columns of cat
                float* d = cat + gr * ld + hw + 8 * kg;
                *reinterpret_cast<float4*>(d) = make_float4(xa[it][0], xa[it][1], xa[it][2], xa[it][3]);
                *reinterpret_cast<float4*>(d + 4) = make_float4(xa[it][4], xa[it][5], xa[it][6], xa[it][7]);
            }
            float cm = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) cm = fmaxf(cm, fabsf(xa[it][e]));
            if (u < NUX && cm > 0.f) atomicMax(&xmax[row], __float_as_int(cm));
        }
        __syncthreads();
#pragma unroll
        for (int it = 0; it < ITX; ++it) {
            const int u = tid + NTH * it;
            if (u >= NUX) break;
            const int row = u % R, kg = u / R;
            const float s = __builtin_ldexpf(1.f, row_scale_exp(__int_as_float(xmax[row])));
            f16x8 th, tm;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float xs = xa[it][e] * s;
                const _Float16 hh = (_Float16)xs;
                th[e] = hh;
                tm[e] = (_Float16)(xs - (float)hh);
            }
            ximg[0 * NUX + kg * R + row] = __builtin_bit_cast(u32x4, th);
            ximg[1 * NUX + kg * R + row] = __builtin_bit_cast(u32x4, tm);
        }
    }
    __syncthreads();
    float rsx[RF];                                     // 2^-e of x rows rg * 16 + c
#pragma unroll
    for (int rg = 0; rg < RF; ++rg) {
        const float mx = __int_as_float(xmax[rg * 16 + c]);
        rsx[rg] = __builtin_ldexpf(1.f, mx > 0.f ? -row_scale_exp(mx) : 0);
    }
    // one k-step of conv1: the three products of gemm_rs.hip, in its order
    f32x4 acc1[RF];                                    // conv1's accumulators (one chunk)
    auto conv1_step = [&](int ks) {
        const f16x8 wh = __builtin_bit_cast(f16x8, w1q[ks][0]);
        const f16x8 wl = __builtin_bit_cast(f16x8, w1q[ks][1]);
        const int base = (ks * 4 + g) * R;
        f16x8 xh[RF], xl[RF];
#pragma unroll
        for (int f = 0; f < RF; ++f) {
            xh[f] = __builtin_bit_cast(f16x8, ximg[0 * NUX + base + 16 * f + c]);
            xl[f] = __builtin_bit_cast(f16x8, ximg[1 * NUX + base + 16 * f + c]);
        }
#pragma unroll
        for (int f = 0; f < RF; ++f) acc1[f] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl, xh[f], acc1[f], 0, 0, 0);
#pragma unroll
        for (int f = 0; f < RF; ++f) acc1[f] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, xl[f], acc1[f], 0, 0, 0);
#pragma unroll
        for (int f = 0; f < RF; ++f) acc1[f] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, xh[f], acc1[f], 0, 0, 0);
    };
    // h_j[row rg * 16 + c][cols col0 .. col0 + 3] of the chunk whose operands are loaded
    auto conv1_out = [&](const f32x4 av, const int rg) {
        float4 hv;
        hv.x = fmaxf(av[0] * (rsx[rg] * w1sv.x) + b1v.x, 0.f);
        hv.y = fmaxf(av[1] * (rsx[rg] * w1sv.y) + b1v.y, 0.f);
        hv.z = fmaxf(av[2] * (rsx[rg] * w1sv.z) + b1v.z, 0.f);
        hv.w = fmaxf(av[3] * (rsx[rg] * w1sv.w) + b1v.w, 0.f);
        return hv;
    };
    // a (>= 0) into the sp tile and its maximum into the row's slot
    auto put_a = [&](const float4& a, int row, int* rm) {
        *reinterpret_cast<float4*>(sp + row * SPW + col0) = a;
        const float cm = fmaxf(fmaxf(a.x, a.y), fmaxf(a.z, a.w));
        if (cm > 0.f) atomicMax(&rm[row], __float_as_int(cm));
    };

    // ---- chunk 0: a_0 = h_0 (columns in [w, W) get 0: zero weights, scales and bias)
    {
#pragma unroll
        for (int f = 0; f < RF; ++f) acc1[f] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KSX; ++ks) conv1_step(ks);
#pragma unroll
        for (int rg = 0; rg < RF; ++rg) put_a(conv1_out(acc1[rg], rg), rg * 16 + c, rmax[0]);
    }
    __syncthreads();

    for (int i = 0; i < nums; ++i) {
        int* rm = rmax[i & 1];
        int* rmn = rmax[(i + 1) & 1];
        const u32x4* wb = wf + (((int64_t)i * KT + wv) * KS) * 128 + lane;
        u32x4 bq[KS][2];
#pragma unroll
        for (int q = 0; q < KS; ++q)
#pragma unroll
            for (int t = 0; t < 2; ++t) bq[q][t] = wb[(q * 2 + t) * 64];
        float4 wsv = make_float4(0.f, 0.f, 0.f, 0.f), bc = wsv;
        if (col_ok) {
            wsv = ld4(wsc + i * w + col0);
            bc = ld4(bias + i * w + col0);
        }
        load_w1(i + 1);
        // the next step's row maxima: last read in the previous step's epilogue, written by
        // this step's epilogue (after the barrier below)
        if (tid < R) rmn[tid] = 0;
        // split a_i (the sp tile; its row maxima are complete): units at k0 >= W are the k32
        // steps' padding past W
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int u = tid + NTH * it;
            if (u >= NU) break;
            const int row = u % R, kg = u / R, k0 = 8 * kg;
            float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            if (k0 < W) {                               // k0 + 8 <= W: W % 16 == 0
                const float4 s0 = *reinterpret_cast<const float4*>(sp + row * SPW + k0);
                const float4 s1 = *reinterpret_cast<const float4*>(sp + row * SPW + k0 + 4);
                a[0] = s0.x; a[1] = s0.y; a[2] = s0.z; a[3] = s0.w;
                a[4] = s1.x; a[5] = s1.y; a[6] = s1.z; a[7] = s1.w;
            }
            const float s = __builtin_ldexpf(1.f, row_scale_exp(__int_as_float(rm[row])));
            f16x8 th, tm;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float xs = a[e] * s;
                const _Float16 hh = (_Float16)xs;
                th[e] = hh;
                tm[e] = (_Float16)(xs - (float)hh);
            }
            img[0 * NU + kg * R + row] = __builtin_bit_cast(u32x4, th);
            img[1 * NU + kg * R + row] = __builtin_bit_cast(u32x4, tm);
        }
#pragma unroll
        for (int f = 0; f < RF; ++f) acc1[f] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KSX; ++ks) conv1_step(ks);    // chunk i + 1, independent of the chain
        __syncthreads();
        f32x4 acc[RF];
#pragma unroll
        for (int f = 0; f < RF; ++f) acc[f] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const f16x8 wh = __builtin_bit_cast(f16x8, bq[ks][0]);
            const f16x8 wl = __builtin_bit_cast(f16x8, bq[ks][1]);
            const int base = (ks * 4 + g) * R;
            f16x8 ah[RF], am[RF];
#pragma unroll
            for (int f = 0; f < RF; ++f) {
                ah[f] = __builtin_bit_cast(f16x8, img[0 * NU + base + 16 * f + c]);
                am[f] = __builtin_bit_cast(f16x8, img[1 * NU + base + 16 * f + c]);
            }
#pragma unroll
            for (int f = 0; f < RF; ++f) acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl, ah[f], acc[f], 0, 0, 0);
#pragma unroll
            for (int f = 0; f < RF; ++f) acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, am[f], acc[f], 0, 0, 0);
#pragma unroll
            for (int f = 0; f < RF; ++f) acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, ah[f], acc[f], 0, 0, 0);
        }
        // epilogue: lane (g, c) holds sp_i and h_{i+1} at [row rg * 16 + c][col0 .. col0 + 3]
#pragma unroll
        for (int rg = 0; rg < RF; ++rg) {
            const int row = rg * 16 + c;
            const float mx = __int_as_float(rm[row]);
            const float rs = __builtin_ldexpf(1.f, mx > 0.f ? -row_scale_exp(mx) : 0);
            const f32x4 av = acc[rg];
            float4 y;
            y.x = fmaxf(av[0] * rs * wsv.x + bc.x, 0.f);
            y.y = fmaxf(av[1] * rs * wsv.y + bc.y, 0.f);
            y.z = fmaxf(av[2] * rs * wsv.z + bc.z, 0.f);
            y.w = fmaxf(av[3] * rs * wsv.w + bc.w, 0.f);
            const float4 hv = conv1_out(acc1[rg], rg);
            const bool st = r0 + row < n && col_ok;
            float* crow = cat + (r0 + row) * ld + col0;
            if (st) *reinterpret_cast<float4*>(crow + (int64_t)i * w) = y;
            if (i + 1 < nums)
                put_a(make_float4(y.x + hv.x, y.y + hv.y, y.z + hv.z, y.w + hv.w), row, rmn);
            else if (st)                                // h_{scale-1}: the pass-through chunk
                *reinterpret_cast<float4*>(crow + (int64_t)(i + 1) * w) = hv;
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------
// The same front on the bf16x6 hierarchy (w = 224, cin = 256): conv1 stays f16x3 (the recipe
// above; h is fp32 either way) in chain6's orientation -- the x image is the A operand, the
// W1 fragments (the same image as block_h3's) the B operand -- so h_{i+1} lands in chain6's
// accumulator layout (rows 4 g + r, column c) and the epilogue writes sp_i + h_{i+1} into
// the sp tile. conv1 of chunk i + 1 needs neither the sp tile nor the bf16 images, so a wave
// issues its MFMAs right after its share of the split, before the barrier: the matrix pipe is
// otherwise idle in that phase (measured at 9544 rows: 93 us, against 98 us with conv1 after
// the chain's k-loop and 95 us with every other wave of a SIMD running conv1 before its
// split). Its W1 fragments come through a two-deep ring beside the chain's three-deep one;
// keeping the two k-loops apart keeps both within the 128 registers of a 14-wave block.
// LDS at R = 48: img 64512 + sp 43776 + ximg 49152 + row scales 192 B: one block per CU.
// ------------------------------------------------------------------------------------
template <int KT, int KSX, int R = kRows>
__global__ void __launch_bounds__(64 * KT)
res2net_block6_kernel(const float* __restrict__ x, int64_t n, int scale,
                      const u32x4* __restrict__ w1f, const float* __restrict__ w1sc,
                      const float* __restrict__ b1, const u32x4* __restrict__ wf,
                      const float* __restrict__ bias, float* __restrict__ cat, int64_t ld) {
    constexpr int W = 16 * KT, KS = (W + 31) / 32, NU = R * KS * 4, NTH = 64 * KT;
    constexpr int CIN = 32 * KSX, NUX = R * KSX * 4;
    constexpr int ITX = (NUX + NTH - 1) / NTH;
    constexpr int RF = R / 16, SPW = W + 4;
    __shared__ u32x4 img[3 * NU];
    __shared__ u32x4 ximg[2 * NUX];
    __shared__ float sp[R * SPW];              // a_i = sp_{i-1} + h_i between steps
    __shared__ int xmax[R];
    __shared__ float xrs[R];                   // 2^-e of the x rows
    const int tid = threadIdx.x;
    const int wv = tid / 64, lane = tid % 64, g = lane >> 4, c = lane & 15;
    const int64_t r0 = (int64_t)blockIdx.x * R;
    const int64_t hw = (int64_t)scale * W;
    const int nums = scale - 1;
    const int col = wv * 16 + c;
    if (tid < R) xmax[tid] = 0;
    __syncthreads();

    // ---- the x tile (as res2net_block_h3_kernel)
    {
        float xa[ITX][8];
#pragma unroll
        for (int it = 0; it < ITX; ++it) {
            const int u = tid + NTH * it;
            const int row = u % R, kg = u / R;
            const int64_t gr = r0 + row;
#pragma unroll
            for (int e = 0; e < 8; e += 4) {
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (u < NUX && gr < n) v = ld4(x + gr * CIN + 8 * kg + e);
                xa[it][e] = v.x; xa[it][e + 1] = v.y; xa[it][e + 2] = v.z; xa[it][e + 3] = v.w;
            }
        }
#pragma unroll
        for (int it = 0; it < ITX; ++it) {
            const int u = tid + NTH * it;
            const int row = u % R, kg = u / R;
            const int64_t gr = r0 + row;
            if (u < NUX && gr < n) {                    // the x columns of cat
                float* d = cat + gr * ld + hw + 8 * kg;
                *reinterpret_cast<float4*>(d) = make_float4(xa[it][0], xa[it][1], xa[it][2], xa[it][3]);
                *reinterpret_cast<float4*>(d + 4) = make_float4(xa[it][4], xa[it][5], xa[it][6], xa[it][7]);
            }
            float cm = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) cm = fmaxf(cm, fabsf(xa[it][e]));
            if (u < NUX && cm > 0.f) atomicMax(&xmax[row], __float_as_int(cm));
        }
        __syncthreads();
        if (tid < R) xrs[tid] = __builtin_ldexpf(1.f, -row_scale_exp(__int_as_float(xmax[tid])));
#pragma unroll
        for (int it = 0; it < ITX; ++it) {
            const int u = tid + NTH * it;
            if (u >= NUX) break;
            const int row = u % R, kg = u / R;
            const float s = __builtin_ldexpf(1.f, row_scale_exp(__int_as_float(xmax[row])));
            f16x8 th, tm;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float xs = xa[it][e] * s;
                const _Float16 hh = (_Float16)xs;
                th[e] = hh;
                tm[e] = (_Float16)(xs - (float)hh);
            }
            ximg[0 * NUX + kg * R + row] = __builtin_bit_cast(u32x4, th);
            ximg[1 * NUX + kg * R + row] = __builtin_bit_cast(u32x4, tm);
        }
    }
    __syncthreads();

    // conv1 of chunk j (its first two k-steps' W1 fragments in w1q[0], w1q[1]): h_j of this
    // lane's column and rows rg * 16 + 4 g + r, the three products in gemm_rs.hip's order
    u32x4 w1q[2][2];
    auto w1_base = [&](int j) { return w1f + (((int64_t)j * KT + wv) * KSX) * 128 + lane; };
    auto w1_head = [&](const u32x4* wb) {
#pragma unroll
        for (int q = 0; q < 2; ++q)
            if (q < KSX) {
#pragma unroll
                for (int t = 0; t < 2; ++t) w1q[q][t] = wb[(q * 2 + t) * 64];
            }
    };
    f32x4 acc1[RF];
    auto conv1 = [&](const u32x4* wb) {
#pragma unroll
        for (int f = 0; f < RF; ++f) acc1[f] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KSX; ++ks) {
            const f16x8 wh = __builtin_bit_cast(f16x8, w1q[ks % 2][0]);
            const f16x8 wl = __builtin_bit_cast(f16x8, w1q[ks % 2][1]);
            const int base = (ks * 4 + g) * R;
            f16x8 xh[RF], xl[RF];
#pragma unroll
            for (int f = 0; f < RF; ++f) {
                xh[f] = __builtin_bit_cast(f16x8, ximg[0 * NUX + base + 16 * f + c]);
                xl[f] = __builtin_bit_cast(f16x8, ximg[1 * NUX + base + 16 * f + c]);
            }
#pragma unroll
            for (int f = 0; f < RF; ++f) acc1[f] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xh[f], wl, acc1[f], 0, 0, 0);
#pragma unroll
            for (int f = 0; f < RF; ++f) acc1[f] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xl[f], wh, acc1[f], 0, 0, 0);
#pragma unroll
            for (int f = 0; f < RF; ++f) acc1[f] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xh[f], wh, acc1[f], 0, 0, 0);
            if (ks + 2 < KSX) {                         // the slot just consumed
#pragma unroll
                for (int t = 0; t < 2; ++t) w1q[ks % 2][t] = wb[((ks + 2) * 2 + t) * 64];
            }
        }
    };
    auto conv1_out = [&](const float a, const int row, const float ws, const float bb) {
        return fmaxf(a * (xrs[row] * ws) + bb, 0.f);
    };

    // ---- chunk 0: a_0 = h_0
    {
        const u32x4* wb = w1_base(0);
        w1_head(wb);
        const float ws = w1sc[col], bb = b1[col];
        conv1(wb);
#pragma unroll
        for (int rg = 0; rg < RF; ++rg)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = rg * 16 + 4 * g + r;
                sp[row * SPW + col] = conv1_out(acc1[rg][r], row, ws, bb);
            }
    }
    __syncthreads();

    for (int i = 0; i < nums; ++i) {
        const u32x4* wb = wf + (((int64_t)i * KT + wv) * KS) * 192 + lane;
        u32x4 bq[3][3];                                // ring: k-steps ks, ks+1, ks+2
#pragma unroll
        for (int q = 0; q < 2; ++q)
            if (q < KS) {
#pragma unroll
                for (int t = 0; t < 3; ++t) bq[q][t] = wb[(q * 3 + t) * 64];
            }
        const float bc = bias[i * W + col];
        const u32x4* wb1 = w1_base(i + 1);
        w1_head(wb1);
        const float ws = w1sc[(i + 1) * W + col], bb = b1[(i + 1) * W + col];
        // split a_i (the sp tile) into the three bf16 images; conv1 of chunk i + 1 needs
        // neither the tile nor the images, so its MFMAs go here, beside the split's VALU /
        // LDS work (the matrix pipe is idle in this phase), not after the chain's
        auto build = [&](const int u) {
            const int row = u % R, kg = u / R;
            const int k0 = 8 * kg;
            float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            if (W % 32 == 0 || k0 < W) {                // k0 + 8 <= W: W % 16 == 0
                const float4 s0 = *reinterpret_cast<const float4*>(sp + row * SPW + k0);
                const float4 s1 = *reinterpret_cast<const float4*>(sp + row * SPW + k0 + 4);
                a[0] = s0.x; a[1] = s0.y; a[2] = s0.z; a[3] = s0.w;
                a[4] = s1.x; a[5] = s1.y; a[6] = s1.z; a[7] = s1.w;
            }
            bf16x8 th, tm, tl;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                __bf16 hh, mm, ll;
                split3(a[e], hh, mm, ll);
                th[e] = hh; tm[e] = mm; tl[e] = ll;
            }
            img[0 * NU + kg * R + row] = __builtin_bit_cast(u32x4, th);
            img[1 * NU + kg * R + row] = __builtin_bit_cast(u32x4, tm);
            img[2 * NU + kg * R + row] = __builtin_bit_cast(u32x4, tl);
        };
        constexpr int IT = (NU + NTH - 1) / NTH;
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int u = tid + NTH * it;
            if ((it + 1) * NTH <= NU || u < NU) build(u);
        }
        conv1(wb1);                                     // chunk i + 1
        __syncthreads();
        f32x4 acc[RF];
#pragma unroll
        for (int f = 0; f < RF; ++f) acc[f] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            if (ks + 2 < KS) {
#pragma unroll
                for (int t = 0; t < 3; ++t) bq[(ks + 2) % 3][t] = wb[((ks + 2) * 3 + t) * 64];
            }
            const bf16x8 bh = __builtin_bit_cast(bf16x8, bq[ks % 3][0]);
            const bf16x8 bm = __builtin_bit_cast(bf16x8, bq[ks % 3][1]);
            const bf16x8 bl = __builtin_bit_cast(bf16x8, bq[ks % 3][2]);
            const int base = (ks * 4 + g) * R;
            bf16x8 ah[RF], am[RF], al[RF];
#pragma unroll
            for (int f = 0; f < RF; ++f) {
                ah[f] = __builtin_bit_cast(bf16x8, img[0 * NU + base + 16 * f + c]);
                am[f] = __builtin_bit_cast(bf16x8, img[1 * NU + base + 16 * f + c]);
                al[f] = __builtin_bit_cast(bf16x8, img[2 * NU + base + 16 * f + c]);
            }
            // the six products of three-term bf16 splits, smallest first (as chain6)
#pragma unroll
            for (int f = 0; f < RF; ++f) acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(am[f], bm, acc[f], 0, 0, 0);
#pragma unroll
            for (int f = 0; f < RF; ++f) acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[f], bh, acc[f], 0, 0, 0);
#pragma unroll
            for (int f = 0; f < RF; ++f) acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[f], bl, acc[f], 0, 0, 0);
#pragma unroll
            for (int f = 0; f < RF; ++f) acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(am[f], bh, acc[f], 0, 0, 0);
#pragma unroll
            for (int f = 0; f < RF; ++f) acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[f], bm, acc[f], 0, 0, 0);
#pragma unroll
            for (int f = 0; f < RF; ++f) acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[f], bh, acc[f], 0, 0, 0);
        }
        // epilogue: sp_i -> cat; a_{i+1} = sp_i + h_{i+1} -> the sp tile (read by the next
        // step's build after the barrier below), the last chunk straight to cat
#pragma unroll
        for (int rg = 0; rg < RF; ++rg) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = rg * 16 + 4 * g + r;
                const float y = fmaxf(acc[rg][r] + bc, 0.f);
                const float hv = conv1_out(acc1[rg][r], row, ws, bb);
                float* crow = cat + (r0 + row) * ld + col;
                if (r0 + row < n) crow[(int64_t)i * W] = y;
                if (i + 1 < nums) sp[row * SPW + col] = y + hv;
                else if (r0 + row < n) crow[(int64_t)(i + 1) * W] = hv;
            }
        }
        __syncthreads();
    }
}

}  // namespace
}  // namespace fgr

using namespace fgr;

// (w, cin) pairs with a fused instance: every w : cin = 7 : 8 pair of the reference whose
// block fits the register file without a W1 ring (224 / 256 stays on the two launches)
static int block_h3_kt(int w, int cin) {
    const int kt = (w + 15) / 16;
    if (w <= 0 || w % 4 != 0) return 0;
    if ((kt == 2 && cin == 32) || (kt == 4 && cin == 64) || (kt == 7 && cin == 128)) return kt;
    return 0;
}

extern "C" int fgr_res2net_block_h3(const float* x, int64_t n, int32_t w, int32_t cin,
                                    int32_t scale, const void* w1_img, const float* w1_scale,
                                    const float* b1, const void* w_img, const float* w_scale,
                                    const float* bias, float* cat, int64_t ld_cat, void* stream) {
    FGR_REQUIRE(n >= 0 && scale >= 2, "fgr_res2net_block_h3: bad n %lld / scale %d", (long long)n,
                scale);
    const int kt = block_h3_kt(w, cin);
    FGR_REQUIRE(kt != 0,
                "fgr_res2net_block_h3: no instance for width %d with cin %d ((28, 32), (56, 64), "
                "(112, 128) up to tile padding)", w, cin);
    FGR_REQUIRE(ld_cat >= (int64_t)scale * w + cin && ld_cat % 4 == 0,
                "fgr_res2net_block_h3: ld_cat %lld too small (needs %lld) or not a multiple of 4",
                (long long)ld_cat, (long long)scale * w + cin);
    FGR_REQUIRE(n == 0 || (x && w1_img && w1_scale && b1 && w_img && w_scale && bias && cat),
                "fgr_res2net_block_h3: null pointer");
    const uintptr_t al = reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(cat) |
                         reinterpret_cast<uintptr_t>(w1_scale) | reinterpret_cast<uintptr_t>(b1) |
                         reinterpret_cast<uintptr_t>(w_scale) | reinterpret_cast<uintptr_t>(bias) |
                         reinterpret_cast<uintptr_t>(w1_img) | reinterpret_cast<uintptr_t>(w_img);
    FGR_REQUIRE((al & 15) == 0,
                "fgr_res2net_block_h3: x %p / cat %p / images / scales / biases must be 16-B aligned",
                (const void*)x, (const void*)cat);
    if (n == 0) return FGR_OK;
    hipStream_t st = as_stream(stream);
    TimedCall timed_(st);
#define FGR_BH3_CASE(KT, KSX)                                                                    \
    case KT:                                                                                     \
        hipLaunchKernelGGL((res2net_block_h3_kernel<KT, KSX>), dim3((unsigned)ceil_div(n, kRows)), \
                           dim3(64 * KT), 0, st, x, n, w, scale, (const u32x4*)w1_img, w1_scale, \
                           b1, (const u32x4*)w_img, w_scale, bias, cat, ld_cat);                 \
        break;
    switch (kt) {
        FGR_BH3_CASE(2, 1)
        FGR_BH3_CASE(4, 2)
        FGR_BH3_CASE(7, 4)
    }
#undef FGR_BH3_CASE
    FGR_CHECK_LAUNCH("res2net_block_h3_kernel");
    return FGR_OK;
}

extern "C" int fgr_res2net_chain_h3(const float* h, int64_t n, int32_t w, int32_t scale,
                                    const void* w_img, const float* w_scale, const float* bias,
                                    const float* x, int32_t cin, float* cat, int64_t ld_cat,
                                    void* stream) {
    FGR_REQUIRE(n >= 0 && scale >= 2 && w > 0 && w <= 224 && w % 4 == 0 && cin >= 0,
                "fgr_res2net_chain_h3: unsupported width %d / scale %d (w %% 4 == 0, <= 224)", w,
                scale);
    FGR_REQUIRE(ld_cat >= (int64_t)scale * w + (x ? cin : 0) && ld_cat % 4 == 0,
                "fgr_res2net_chain_h3: ld_cat too small or not a multiple of 4");
    FGR_REQUIRE(n == 0 || (h && w_img && w_scale && bias && cat), "fgr_res2net_chain_h3: null pointer");
    FGR_REQUIRE(((reinterpret_cast<uintptr_t>(h) | reinterpret_cast<uintptr_t>(cat) |
                  reinterpret_cast<uintptr_t>(w_scale) | reinterpret_cast<uintptr_t>(bias)) & 15) == 0 &&
                    (scale * w) % 4 == 0,
                "fgr_res2net_chain_h3: h / cat / w_scale / bias must be 16-B aligned");
    if (n == 0) return FGR_OK;
    hipStream_t st = as_stream(stream);
    TimedCall timed_(st);
    const int kt = (w + 15) / 16;
    // w > 112 (one 14-wave block per CU): 48-row blocks when that saves a round of blocks
    // (rounds x rows per block over 256 CUs, as fgr_res2net_chain6); FGR_R2N_ROWS=32 forces 32
    const char* rr = getenv("FGR_R2N_ROWS");
    const bool r48 = kt == 14 && !(rr && rr[0] == '3') &&
                     ceil_div(ceil_div(n, 48), 256) * 48 < ceil_div(ceil_div(n, 32), 256) * 32;
#define FGR_H3_CASE(KT)                                                                         \
    case KT:                                                                                    \
        hipLaunchKernelGGL(res2net_chain_h3_kernel<KT>, dim3((unsigned)ceil_div(n, kRows)),     \
                           dim3(64 * KT), 0, st, h, n, w, scale, scale - 1, (const u32x4*)w_img, \
                           w_scale, bias, x, cin, cat, ld_cat);                                 \
        break;
    if (r48) {
        hipLaunchKernelGGL((res2net_chain_h3_kernel<14, 48>), dim3((unsigned)ceil_div(n, 48)),
                           dim3(64 * 14), 0, st, h, n, w, scale, scale - 1, (const u32x4*)w_img,
                           w_scale, bias, x, cin, cat, ld_cat);
        FGR_CHECK_LAUNCH("res2net_chain_h3_kernel");
        return FGR_OK;
    }
    switch (kt) {
        FGR_H3_CASE(2)
        FGR_H3_CASE(4)
        FGR_H3_CASE(7)
        FGR_H3_CASE(14)
        default:
            set_error("fgr_res2net_chain_h3: width %d has no kernel instance (28, 56, 112, 224)", w);
            return FGR_E_ARG;
    }
#undef FGR_H3_CASE
    FGR_CHECK_LAUNCH("res2net_chain_h3_kernel");
    return FGR_OK;
}

extern "C" int fgr_res2net_chain6(const float* h, int64_t n, int32_t w, int32_t scale,
                                  const void* w_img, const float* bias, const float* x,
                                  int32_t cin, float* cat, int64_t ld_cat, void* stream) {
    FGR_REQUIRE(n >= 0 && scale >= 2 && (w == 112 || w == 224) && cin >= 0,
                "fgr_res2net_chain6: unsupported width %d / scale %d (needs 112 or 224)", w, scale);
    FGR_REQUIRE(ld_cat >= (int64_t)scale * w + (x ? cin : 0), "fgr_res2net_chain6: ld_cat too small");
    FGR_REQUIRE(n == 0 || (h && w_img && bias && cat), "fgr_res2net_chain6: null pointer");
    FGR_REQUIRE(((reinterpret_cast<uintptr_t>(h) & 15) == 0) && (scale * w) % 4 == 0,
                "fgr_res2net_chain6: h must be 16-B aligned");
    if (n == 0) return FGR_OK;
    hipStream_t st = as_stream(stream);
    TimedCall timed_(st);
    // w = 224 (one 14-wave block per CU): 48-row blocks when that saves a round of blocks
    // over 32-row ones (rounds x rows per block; 256 CUs); FGR_R2N_ROWS=32 forces 32 (A/B)
    const char* rr = getenv("FGR_R2N_ROWS");
    int rows = 32;
    if (w == 224 && !(rr && rr[0] == '3')) {       // min over R of rounds(R) x R, larger R on ties
        int64_t best = ceil_div(ceil_div(n, 32), 256) * 32;
        for (int r : {48, 16}) {
            const int64_t cost = ceil_div(ceil_div(n, r), 256) * r;
            if (cost < best) { best = cost; rows = r; }
        }
    }
    const int64_t b32 = ceil_div(n, 32);
    if (w == 112)
        hipLaunchKernelGGL(res2net_chain6_kernel<7>, dim3((unsigned)b32), dim3(64 * 7), 0, st, h, n,
                           scale, scale - 1, (const u32x4*)w_img, bias, x, cin, cat, ld_cat);
    else if (rows == 48)
        hipLaunchKernelGGL((res2net_chain6_kernel<14, 48>), dim3((unsigned)ceil_div(n, 48)), dim3(64 * 14),
                           0, st, h, n, scale, scale - 1, (const u32x4*)w_img, bias, x, cin, cat, ld_cat);
    else if (rows == 16)
        hipLaunchKernelGGL((res2net_chain6_kernel<14, 16>), dim3((unsigned)ceil_div(n, 16)), dim3(64 * 14),
                           0, st, h, n, scale, scale - 1, (const u32x4*)w_img, bias, x, cin, cat, ld_cat);
    else
        hipLaunchKernelGGL(res2net_chain6_kernel<14>, dim3((unsigned)b32), dim3(64 * 14), 0, st, h, n,
                           scale, scale - 1, (const u32x4*)w_img, bias, x, cin, cat, ld_cat);
    FGR_CHECK_LAUNCH("res2net_chain6_kernel");
    return FGR_OK;
}

extern "C" int fgr_res2net_block6(const float* x, int64_t n, int32_t w, int32_t cin, int32_t scale,
                                  const void* w1_img, const float* w1_scale, const float* b1,
                                  const void* w_img, const float* bias, float* cat,
                                  int64_t ld_cat, void* stream) {
    FGR_REQUIRE(n >= 0 && scale >= 2, "fgr_res2net_block6: bad n %lld / scale %d", (long long)n,
                scale);
    FGR_REQUIRE(w == 224 && cin == 256,
                "fgr_res2net_block6: no instance for width %d with cin %d (needs 224, 256)", w, cin);
    FGR_REQUIRE(ld_cat >= (int64_t)scale * w + cin && ld_cat % 4 == 0,
                "fgr_res2net_block6: ld_cat %lld too small (needs %lld) or not a multiple of 4",
                (long long)ld_cat, (long long)scale * w + cin);
    FGR_REQUIRE(n == 0 || (x && w1_img && w1_scale && b1 && w_img && bias && cat),
                "fgr_res2net_block6: null pointer");
    const uintptr_t al = reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(cat) |
                         reinterpret_cast<uintptr_t>(w1_img) | reinterpret_cast<uintptr_t>(w_img);
    FGR_REQUIRE((al & 15) == 0, "fgr_res2net_block6: x %p / cat %p / images must be 16-B aligned",
                (const void*)x, (const void*)cat);
    if (n == 0) return FGR_OK;
    hipStream_t st = as_stream(stream);
    TimedCall timed_(st);
    // rows per block as fgr_res2net_chain6: min over R of rounds(R) x R over 256 CUs, larger R
    // on ties; FGR_R2N_ROWS=32 forces 32
    const char* rr = getenv("FGR_R2N_ROWS");
    int rows = 32;
    if (!(rr && rr[0] == '3')) {
        int64_t best = ceil_div(ceil_div(n, 32), 256) * 32;
        for (int r : {48, 16}) {
            const int64_t cost = ceil_div(ceil_div(n, r), 256) * r;
            if (cost < best) { best = cost; rows = r; }
        }
    }
#define FGR_B6_LAUNCH(R)                                                                        \
    hipLaunchKernelGGL((res2net_block6_kernel<14, 8, R>), dim3((unsigned)ceil_div(n, R)),       \
                       dim3(64 * 14), 0, st, x, n, scale, (const u32x4*)w1_img, w1_scale, b1,   \
                       (const u32x4*)w_img, bias, cat, ld_cat)
    if (rows == 48) FGR_B6_LAUNCH(48);
    else if (rows == 16) FGR_B6_LAUNCH(16);
    else FGR_B6_LAUNCH(32);
#undef FGR_B6_LAUNCH
    FGR_CHECK_LAUNCH("res2net_block6_kernel");
    return FGR_OK;
}
