// Head-averaged attention weights on packed, unpadded segments: what nn.MultiheadAttention
// returns beside its output with the default need_weights = True (the reference's
// layer.satt_weights / xatt_weights, transformers.py:177-179, 240-242),
//   w[r][j] = (1 / H) sum_h softmax_j(scale q_h[r] . k_h[j])      j < n (the key segment)
//   w[r][j] = 0                                                   n <= j < max_kv_len.
// An inspection path, so exact fp32 in both precision modes: scores on the fp32-input MFMA
// (v_mfma_f32_16x16x4_f32, one rounding per product, as attention.hip), expf, no split.
//
// The flash kernels never form this matrix, so it has a kernel of its own. Block = 4 waves = 16
// query rows of one segment. The work of a block is a long chain of small steps ((head, key
// tile) -> 64 scores per row), so the waves share rows and split the chain, each staging its
// own operands in LDS of its own (no block barrier inside a sweep):
//   sweep 1  wave w takes heads w, w + 4, ...: over the 64-key tiles, the running max m and
//            sum l of every (row, head); m and 1 / l go to LDS. One block barrier.
//   sweep 2  wave w takes key tiles w, w + 4, ...: over the heads in ascending order, the
//            scores again (the same MFMA chain, so the same bits), acc += exp(s - m_h) *
//            (1 / l_h) in registers; then acc / H crosses the wave's LDS so that every store
//            instruction writes whole 64-column runs of 4 rows (16-B stores where w allows).
//            Every element is stored once, no atomics: two runs give the same bits.
// Q and K of one (head, key tile) are staged in slices of at most 32 of the head's columns, so
// the LDS footprint does not grow with head_dim.
//
// MFMA 16x16x4 f32 lane maps (lane l, g = l >> 4, c = l & 15):
//   A[i = c][k = g], B[k = g][j = c], C/D[row = 4g + r][col = c], r = 0..3.
#include "mfma.h"

namespace fgr {
namespace {

constexpr int kWQ = 16;          // query rows per block (one MFMA tile, shared by the 4 waves)
constexpr int kWK = 64;          // keys per tile
constexpr int kWD = 32;          // head columns per staged slice
constexpr int kWOut = kWK + 4;   // row of a wave's output tile (floats; 16-B aligned rows)
constexpr size_t kWLdsMax = 64 << 10;

// LDS floats: [m (H x 16) | 1 / l (H x 16) | per wave: Q slice 16 x LD, then K slice 64 x LD,
// which the wave's 16 x kWOut output tile reuses]
__host__ __device__ inline int aw_ld(int dh) { return (dh < kWD ? dh : kWD) + 1; }
__host__ __device__ inline int aw_wave_floats(int dh) {
    const int kt = kWK * aw_ld(dh), ot = 16 * kWOut;
    return (kWQ * aw_ld(dh) + (kt > ot ? kt : ot) + 3) & ~3;
}
inline size_t aw_lds_bytes(int n_head, int dh) {
    return sizeof(float) * (2 * (size_t)n_head * kWQ + 4 * (size_t)aw_wave_floats(dh));
}

// orders this wave's LDS writes before its later LDS reads (and the reverse)
__device__ __forceinline__ void aw_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// by one wave: rows row0 .. row0 + rows - 1 (zeros from row `live` on), columns col0 .. col0 +
// dc of src, times mult, into dst[row][LD]
__device__ __forceinline__ void aw_stage(float* dst, int LD, const float* __restrict__ src,
                                         int64_t ld, int64_t row0, int rows, int live, int col0,
                                         int dc, float mult, bool vec, int lane) {
    if (vec) {
        // 8 loads per lane in flight before the first LDS write (a 64 x 32 slice is 8 per lane)
        constexpr int U = 8;
        const int n4 = dc >> 2, total = rows * n4;
        const unsigned inv = 65536u / (unsigned)n4 + 1u;   // e / n4 for e < 512, n4 <= 8
        for (int e0 = lane; e0 < total; e0 += 64 * U) {
            float4 x[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int e = e0 + 64 * u;
                const int r = (int)(((unsigned)e * inv) >> 16), c4 = (e - r * n4) * 4;
                x[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (e < total && r < live) x[u] = ld4(src + (row0 + r) * ld + col0 + c4);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int e = e0 + 64 * u;
                const int r = (int)(((unsigned)e * inv) >> 16), c4 = (e - r * n4) * 4;
                if (e >= total) break;
                float* p = dst + r * LD + c4;
                p[0] = x[u].x * mult; p[1] = x[u].y * mult;
                p[2] = x[u].z * mult; p[3] = x[u].w * mult;
            }
        }
    } else {
        for (int e = lane; e < rows * dc; e += 64) {
            const int r = e / dc, cc = e - r * dc;
            dst[r * LD + cc] = r < live ? src[(row0 + r) * ld + col0 + cc] * mult : 0.f;
        }
    }
}

__global__ void __launch_bounds__(256)
attn_weights_kernel(const float* __restrict__ q, int64_t ld_q, const float* __restrict__ k,
                    int64_t ld_k, float* __restrict__ w, int64_t ld_w,
                    const int64_t* __restrict__ q_off, const int64_t* __restrict__ kv_off,
                    const int32_t* __restrict__ kv_seg, int max_kv_len, int n_head, int dh,
                    float scale, int vec_in, int vec_out) {
    extern __shared__ __align__(16) float aw_lds[];
    const int seg = blockIdx.y;
    const int64_t qe = q_off[seg + 1];
    const int64_t q0 = q_off[seg] + (int64_t)blockIdx.x * kWQ;
    if (q0 >= qe) return;                                  // block-uniform
    const int nq = (int)min((int64_t)kWQ, qe - q0);        // live rows of this tile
    const int ks = kv_seg[seg];
    const int64_t kb = kv_off[ks];
    const int nk = (int)(kv_off[ks + 1] - kb);

    const int tid = threadIdx.x, wv = tid / 64, lane = tid % 64;
    const int g = lane >> 4, c = lane & 15;
    const int LD = aw_ld(dh);
    float* m_s = aw_lds;
    float* il_s = m_s + n_head * kWQ;
    float* q_s = il_s + n_head * kWQ + wv * aw_wave_floats(dh);    // this wave's own
    float* k_s = q_s + kWQ * LD;
    float* ow = k_s;                                       // the output tile, after the scores
    const bool one_slice = dh <= kWD;

    // s = (scale q_h) k_h^T of the 16 rows x the 64 keys from k0, keys past the segment at
    // -inf; stage_q: the head's Q slice is not in this wave's LDS yet
    auto scores = [&](int h, int k0, bool stage_q, f32x4 (&s)[4]) {
        const int nt = min(kWK, nk - k0);
#pragma unroll
        for (int n = 0; n < 4; ++n) s[n] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int d0 = 0; d0 < dh; d0 += kWD) {
            const int dc = min(kWD, dh - d0);
            aw_wave_sync();                                // the previous slice is consumed
            if (stage_q || !one_slice)
                aw_stage(q_s, LD, q, ld_q, q0, kWQ, nq, h * dh + d0, dc, scale, vec_in, lane);
            aw_stage(k_s, LD, k, ld_k, kb + k0, kWK, nt, h * dh + d0, dc, 1.0f, vec_in, lane);
            aw_wave_sync();
            for (int kk = 0; kk < dc; kk += 4) {
                const float a = q_s[c * LD + kk + g];
#pragma unroll
                for (int n = 0; n < 4; ++n) {              // 4 independent accumulators
                    const float b = k_s[(n * 16 + c) * LD + kk + g];
                    s[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, s[n], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int n = 0; n < 4; ++n)
            if (n * 16 + c >= nt) s[n] = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    };

    // ---- sweep 1: m and 1 / l of every (row, head); this wave's heads
    for (int h = wv; h < n_head; h += 4) {
        float m_run[4], l_run[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) { m_run[r] = -INFINITY; l_run[r] = 0.f; }
        for (int k0 = 0; k0 < nk; k0 += kWK) {
            f32x4 s[4];
            scores(h, k0, k0 == 0, s);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float mx = fmaxf(fmaxf(s[0][r], s[1][r]), fmaxf(s[2][r], s[3][r]));
                mx = row16_max(mx);                        // key 0 of a tile is live: finite
                const float m_new = fmaxf(m_run[r], mx);
                float rs = 0.f;
#pragma unroll
                for (int n = 0; n < 4; ++n) rs += expf(s[n][r] - m_new);
                rs = row16_sum(rs);
                l_run[r] = l_run[r] * expf(m_run[r] - m_new) + rs;
                m_run[r] = m_new;
            }
        }
        if (c == 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                m_s[h * kWQ + 4 * g + r] = m_run[r];
                il_s[h * kWQ + 4 * g + r] = 1.0f / l_run[r];
            }
        }
    }
    __syncthreads();                                       // every head's statistics are in LDS

    // ---- sweep 2: the weights of this wave's 64-column tiles (zeros past the key segment)
    const float inv_h = 1.0f / (float)n_head;
    for (int k0 = wv * kWK; k0 < max_kv_len; k0 += 4 * kWK) {
        f32x4 acc[4];
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (k0 < nk) {                                     // wave-uniform
            for (int h = 0; h < n_head; ++h) {
                f32x4 s[4];
                scores(h, k0, true, s);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float mh = m_s[h * kWQ + 4 * g + r];
                    const float il = il_s[h * kWQ + 4 * g + r];
#pragma unroll
                    for (int n = 0; n < 4; ++n) acc[n][r] += expf(s[n][r] - mh) * il;
                }
            }
        }
        // C layout -> the wave's LDS tile (over its K slice) -> row-major stores
        aw_wave_sync();
#pragma unroll
        for (int n = 0; n < 4; ++n)
#pragma unroll
            for (int r = 0; r < 4; ++r) ow[(4 * g + r) * kWOut + n * 16 + c] = acc[n][r] * inv_h;
        aw_wave_sync();
        if (vec_out) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int rl = i * 4 + g, col = k0 + c * 4;
                if (rl >= nq || col >= max_kv_len) continue;
                const float4 x = ld4(ow + rl * kWOut + c * 4);
                float* dst = w + (q0 + rl) * ld_w + col;
                if (col + 4 <= max_kv_len) {
                    *reinterpret_cast<float4*>(dst) = x;
                } else {
                    dst[0] = x.x;
                    if (col + 1 < max_kv_len) dst[1] = x.y;
                    if (col + 2 < max_kv_len) dst[2] = x.z;
                }
            }
        } else {
            for (int rl = 0; rl < nq; ++rl)
                if (k0 + lane < max_kv_len) w[(q0 + rl) * ld_w + k0 + lane] = ow[rl * kWOut + lane];
        }
    }
}

}  // namespace
}  // namespace fgr

using namespace fgr;

extern "C" int fgr_attention_weights(const float* q, int64_t ld_q, const float* k, int64_t ld_k,
                                     float* w, int64_t ld_w, const int64_t* q_off,
                                     const int64_t* kv_off, const int32_t* kv_seg, int32_t n_seg,
                                     int32_t max_q_len, int32_t max_kv_len, int32_t n_head,
                                     int32_t head_dim, float scale, void* stream) {
    FGR_REQUIRE(q && k && w && q_off && kv_off && kv_seg && n_seg > 0 && n_head > 0 &&
                    max_q_len >= 0 && max_kv_len >= 0,
                "fgr_attention_weights: bad arguments");
    FGR_REQUIRE(head_dim > 0 && head_dim % 4 == 0 && head_dim <= 256,
                "fgr_attention_weights: head_dim %d unsupported (a multiple of 4, at most 256)",
                head_dim);
    FGR_REQUIRE(ld_q >= (int64_t)n_head * head_dim && ld_k >= (int64_t)n_head * head_dim,
                "fgr_attention_weights: row stride smaller than n_head * head_dim");
    FGR_REQUIRE(ld_w >= max_kv_len, "fgr_attention_weights: ld_w %lld < max_kv_len %d",
                (long long)ld_w, max_kv_len);
    const size_t lds = aw_lds_bytes(n_head, head_dim);
    FGR_REQUIRE(lds <= kWLdsMax,
                "fgr_attention_weights: n_head %d at head_dim %d needs %zu bytes of LDS (at most %zu)",
                n_head, head_dim, lds, kWLdsMax);
    if (max_q_len == 0 || max_kv_len == 0) return FGR_OK;
    const auto al16 = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
    const int vec_in = al16(q) && al16(k) && ld_q % 4 == 0 && ld_k % 4 == 0;
    const int vec_out = al16(w) && ld_w % 4 == 0;
    hipStream_t st = as_stream(stream);
    TimedCall timed_(st);
    const dim3 grid((unsigned)ceil_div(max_q_len, kWQ), (unsigned)n_seg);
    hipLaunchKernelGGL(attn_weights_kernel, grid, dim3(256), lds, st, q, ld_q, k, ld_k, w, ld_w,
                       q_off, kv_off, kv_seg, max_kv_len, n_head, head_dim, scale, vec_in, vec_out);
    FGR_CHECK_LAUNCH("attn_weights_kernel");
    return FGR_OK;
}
