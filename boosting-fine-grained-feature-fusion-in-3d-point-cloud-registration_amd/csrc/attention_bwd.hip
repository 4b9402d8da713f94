// Training backward of the multi-head attention core on gfx950: fgr_attention_bwd and its
// _train / _drop forms (transformers.py:197-226) over packed segments, as scalar kernels (head
// dim 4 / 8) and on the fp32 matrix cores (head dim 16 / 32 / 64); the training form runs on the
// f16 matrix cores of attention16.hip (attn_bwd_f16x3) where that applies.
//
// Every reduction is deterministic: fixed-order sums, no floating-point atomics, so two backward
// passes give bit-identical gradients.
#include "mfma.h"

#include <algorithm>
#include <cstdlib>

namespace fgr {
namespace {

// ---- attention backward ------------------------------------------------------------------
// Softmax attention per (query segment i -> key segment kv_seg[i], head h), s = scale q.k:
//   P = softmax(S), O = P V;  dV = P^T dO, dP = dO V^T, dS = P (dP - rowsum(dO o O)), dQ =
//   scale dS K, dK = scale dS^T Q.
// Kernel 1: one thread per query row (64-query blocks, K / V tiles of 64 keys in LDS): the
// row's max and sum (pass 1), then dQ (pass 2); writes the row's log-sum-exp and D = dO.O.
// Kernel 2: one thread per key row: over every query segment attending its segment, Q / dO
// tiles in LDS, accumulates dK and dV.
struct AttnBwd {
    const float* q; int64_t ldq;
    const float* k; int64_t ldk;
    const float* v; int64_t ldv;
    const float* o; int64_t ldo;
    const float* dout; int64_t lddo;
    float* dq; int64_t lddq;
    float* dk; int64_t lddk;
    float* dv; int64_t lddv;
    const int64_t* q_off;
    const int64_t* kv_off;
    const int32_t* kv_seg;
    int n_seg, n_kv_seg, nhead;
    int q_blocks, kv_blocks;
    float scale;
    float* lse;      // (Nq, nhead)
    float* dsum;     // (Nq, nhead)
    // attention-weight dropout (MFMA kernels, DROP): entries with attn_drop_hash < drop_thresh
    // are dropped, kept ones scaled by inv_keep (the forward's mask: fgr_attention_f16x3_drop)
    uint32_t drop_seed, drop_thresh;
    float inv_keep;
    // training: the forward's log2-sum-exp per (row, head) (fgr_attention_f16x3_train); the
    // MFMA dQ kernel then skips its max / sum pass
    const float* lse_in;
};

template <int DH>
__global__ void __launch_bounds__(64)
attn_bwd_dq_kernel(AttnBwd a) {
    __shared__ float kt[64][DH + 1];
    __shared__ float vt[64][DH + 1];
    const int seg = blockIdx.x / a.q_blocks, qb = blockIdx.x % a.q_blocks, h = blockIdx.y;
    const int lane = threadIdx.x;
    const int64_t qb0 = a.q_off[seg], qe = a.q_off[seg + 1];
    const int64_t r = qb0 + (int64_t)qb * 64 + lane;
    if (qb0 + (int64_t)qb * 64 >= qe) return;                 // whole block past the segment
    const bool ok = r < qe;
    const int ks = a.kv_seg[seg];
    const int64_t kb = a.kv_off[ks], ke = a.kv_off[ks + 1];
    float qv[DH], dov[DH], dqv[DH];
    float dsum = 0.f;
#pragma unroll
    for (int j = 0; j < DH; ++j) {
        qv[j] = ok ? a.q[r * a.ldq + h * DH + j] * a.scale : 0.f;
        dov[j] = ok ? a.dout[r * a.lddo + h * DH + j] : 0.f;
        dsum += ok ? dov[j] * a.o[r * a.ldo + h * DH + j] : 0.f;
        dqv[j] = 0.f;
    }
    float m = -INFINITY, l = 0.f;
    for (int64_t t0 = kb; t0 < ke; t0 += 64) {
        const int nt = (int)min((int64_t)64, ke - t0);
        __syncthreads();
        for (int e = lane; e < nt * DH; e += 64) {
            const int kk = e / DH, j = e % DH;
            kt[kk][j] = a.k[(t0 + kk) * a.ldk + h * DH + j];
        }
        __syncthreads();
        for (int kk = 0; kk < nt; ++kk) {
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < DH; ++j) s = fmaf(qv[j], kt[kk][j], s);
            if (s > m) {
                l = l * expf(m - s) + 1.f;
                m = s;
            } else {
                l += expf(s - m);
            }
        }
    }
    const float inv_l = 1.f / l;
    for (int64_t t0 = kb; t0 < ke; t0 += 64) {
        const int nt = (int)min((int64_t)64, ke - t0);
        __syncthreads();
        for (int e = lane; e < nt * DH; e += 64) {
            const int kk = e / DH, j = e % DH;
            kt[kk][j] = a.k[(t0 + kk) * a.ldk + h * DH + j];
            vt[kk][j] = a.v[(t0 + kk) * a.ldv + h * DH + j];
        }
        __syncthreads();
        for (int kk = 0; kk < nt; ++kk) {
            float s = 0.f, dp = 0.f;
#pragma unroll
            for (int j = 0; j < DH; ++j) {
                s = fmaf(qv[j], kt[kk][j], s);
                dp = fmaf(dov[j], vt[kk][j], dp);
            }
            const float p = expf(s - m) * inv_l;
            const float ds = p * (dp - dsum);
#pragma unroll
            for (int j = 0; j < DH; ++j) dqv[j] = fmaf(ds, kt[kk][j], dqv[j]);
        }
    }
    if (!ok) return;
#pragma unroll
    for (int j = 0; j < DH; ++j) a.dq[r * a.lddq + h * DH + j] = dqv[j] * a.scale;
    a.lse[r * a.nhead + h] = m + logf(l);
    a.dsum[r * a.nhead + h] = dsum;
}

template <int DH>
__global__ void __launch_bounds__(64)
attn_bwd_dkdv_kernel(AttnBwd a) {
    __shared__ float qt[64][DH + 1];
    __shared__ float dot_[64][DH + 1];
    __shared__ float lt[64], dt[64];
    const int ks = blockIdx.x / a.kv_blocks, kbk = blockIdx.x % a.kv_blocks, h = blockIdx.y;
    const int lane = threadIdx.x;
    const int64_t kb0 = a.kv_off[ks], ke = a.kv_off[ks + 1];
    const int64_t r = kb0 + (int64_t)kbk * 64 + lane;
    if (kb0 + (int64_t)kbk * 64 >= ke) return;
    const bool ok = r < ke;
    float kv[DH], vv[DH], dkv[DH], dvv[DH];
#pragma unroll
    for (int j = 0; j < DH; ++j) {
        kv[j] = ok ? a.k[r * a.ldk + h * DH + j] : 0.f;
        vv[j] = ok ? a.v[r * a.ldv + h * DH + j] : 0.f;
        dkv[j] = dvv[j] = 0.f;
    }
    for (int seg = 0; seg < a.n_seg; ++seg) {
        if (a.kv_seg[seg] != ks) continue;
        const int64_t qb = a.q_off[seg], qe = a.q_off[seg + 1];
        for (int64_t t0 = qb; t0 < qe; t0 += 64) {
            const int nt = (int)min((int64_t)64, qe - t0);
            __syncthreads();
            for (int e = lane; e < nt * DH; e += 64) {
                const int qq = e / DH, j = e % DH;
                qt[qq][j] = a.q[(t0 + qq) * a.ldq + h * DH + j] * a.scale;
                dot_[qq][j] = a.dout[(t0 + qq) * a.lddo + h * DH + j];
            }
            if (lane < nt) {
                lt[lane] = a.lse[(t0 + lane) * a.nhead + h];
                dt[lane] = a.dsum[(t0 + lane) * a.nhead + h];
            }
            __syncthreads();
            for (int qq = 0; qq < nt; ++qq) {
                float s = 0.f, dp = 0.f;
#pragma unroll
                for (int j = 0; j < DH; ++j) {
                    s = fmaf(qt[qq][j], kv[j], s);
                    dp = fmaf(dot_[qq][j], vv[j], dp);
                }
                const float p = expf(s - lt[qq]);
                const float ds = p * (dp - dt[qq]);
#pragma unroll
                for (int j = 0; j < DH; ++j) {
                    dvv[j] = fmaf(p, dot_[qq][j], dvv[j]);
                    dkv[j] = fmaf(ds, qt[qq][j], dkv[j]);      // qt holds scale * q
                }
            }
        }
    }
    if (!ok) return;
#pragma unroll
    for (int j = 0; j < DH; ++j) {
        a.dk[r * a.lddk + h * DH + j] = dkv[j];
        a.dv[r * a.lddv + h * DH + j] = dvv[j];
    }
}

// ---- attention backward on the fp32 matrix cores (head dim 16 / 32 / 64; round 5) -----------
// The same two-kernel split as above, as tiled v_mfma_f32_16x16x4_f32 products (exact fp32
// products, fp32 accumulation: the precision of the scalar kernels, ~6-10x their speed on the
// forward's shapes). A wave owns 16 rows of its side (kernel 1: queries; kernel 2: keys), a
// 256-thread block 64; the other side streams through LDS in tiles of 64 rows.
// Lane maps of the 16x16x4 product (lane l, g = l >> 4, c = l & 15): A[i = c][k = g],
// B[k = g][j = c], D[i = 4g + r][j = c]. The head-dim contraction pairs lane g with dims
// g * KS + s at k-step s (KS = DH / 4), so a lane holds KS CONSECUTIVE dims of its row (vector
// loads); the key / query contraction (dV, dK, dQ) pairs lane g with row 16n + 4g + r at k-step
// (n, r) -- exactly the rows whose scores the lane holds after the score product, so P and dS
// feed the next product from registers. Scores run in the log2 domain (q pre-scaled by
// scale * log2 e, P = exp2(s - lse2)); the workspace keeps lse2 and D = dO . O per (row, head).
constexpr float kLog2e = 1.4426950408889634f;

// KS consecutive floats of a row (16-B aligned when KS % 4 == 0)
template <int KS>
__device__ __forceinline__ void load_ks(const float* p, float (&v)[KS], bool ok, float mul) {
    if constexpr (KS % 4 == 0) {
#pragma unroll
        for (int s = 0; s < KS; s += 4) {
            const float4 x = ok ? *reinterpret_cast<const float4*>(p + s) : make_float4(0.f, 0.f, 0.f, 0.f);
            v[s] = x.x * mul; v[s + 1] = x.y * mul; v[s + 2] = x.z * mul; v[s + 3] = x.w * mul;
        }
    } else {
#pragma unroll
        for (int s = 0; s < KS; ++s) v[s] = ok ? p[s] * mul : 0.f;
    }
}

// stage 64 rows x DH of `src` (row stride ld, head offset applied) into LDS rows of pitch LD,
// rows >= n zero, each row scaled by mul
template <int DH, int LD>
__device__ __forceinline__ void stage_rows(float* dst, const float* src, int64_t ld, int n, float mul) {
    constexpr int R4 = DH / 4;
    for (int e = threadIdx.x; e < 64 * R4; e += 256) {
        const int row = e / R4, d4 = (e % R4) * 4;
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row < n) x = *reinterpret_cast<const float4*>(src + row * ld + d4);
        float* o = dst + row * LD + d4;
        o[0] = x.x * mul; o[1] = x.y * mul; o[2] = x.z * mul; o[3] = x.w * mul;
    }
}

// DROP: with M the forward's scaled mask (0 or 1 / (1 - p)), O = (P o M) V, so dV = (P o M)^T dO,
// dP = M o (dO V^T) and dS = P o (dP - D) with D = rowsum(dO o O) unchanged.
template <int DH, bool DROP = false>
__global__ void __launch_bounds__(256)
attn_bwd_dq_mfma_kernel(AttnBwd a) {
    constexpr int KS = DH / 4, DT = DH / 16, LD = DH + 4;
    __shared__ float kt[64 * LD];
    __shared__ float vt[64 * LD];
    const int seg = blockIdx.x / a.q_blocks, qb = blockIdx.x % a.q_blocks, h = blockIdx.y;
    const int64_t qb0 = a.q_off[seg], qe = a.q_off[seg + 1];
    if (qb0 + (int64_t)qb * 64 >= qe) return;                 // block-uniform
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, g = lane >> 4, c = lane & 15;
    const int64_t r = qb0 + (int64_t)qb * 64 + wv * 16 + c;  // this lane's query row
    const bool ok = r < qe;
    const int ks = a.kv_seg[seg];
    const int64_t kb = a.kv_off[ks], ke = a.kv_off[ks + 1];
    float qv[KS], dov[KS], ov[KS];
    load_ks<KS>(a.q + r * a.ldq + h * DH + g * KS, qv, ok, a.scale * kLog2e);
    load_ks<KS>(a.dout + r * a.lddo + h * DH + g * KS, dov, ok, 1.f);
    load_ks<KS>(a.o + r * a.ldo + h * DH + g * KS, ov, ok, 1.f);
    float dsum = 0.f;
#pragma unroll
    for (int s = 0; s < KS; ++s) dsum = fmaf(dov[s], ov[s], dsum);
    dsum = xg_sum(dsum);
    // S^T tile n of the staged keys: lane (g, c) -> keys 16n + 4g + r of query c
    auto scores = [&](const float* tile, const float (&rv)[KS], int n) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        const float* kr = tile + (16 * n + c) * LD + g * KS;
#pragma unroll
        for (int s = 0; s < KS; ++s)
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(kr[s], rv[s], acc, 0, 0, 0);
        return acc;
    };
    // pass 1: the row's max and sum (per lane over its keys, then over the 4 lanes of the row)
    // -- or the forward's log-sum-exp
    float m = -INFINITY, l = 0.f;
    for (int64_t t0 = a.lse_in ? ke : kb; t0 < ke; t0 += 64) {
        const int nt = (int)min((int64_t)64, ke - t0);
        __syncthreads();
        stage_rows<DH, LD>(kt, a.k + t0 * a.ldk + h * DH, a.ldk, nt, 1.f);
        __syncthreads();
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const f32x4 s4 = scores(kt, qv, n);
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                if (16 * n + 4 * g + rr >= nt) continue;
                const float sv = s4[rr];
                if (sv > m) { l = l * __builtin_amdgcn_exp2f(m - sv) + 1.f; m = sv; }
                else l += __builtin_amdgcn_exp2f(sv - m);
            }
        }
    }
    const float M = xg_max(m);
    const float lse2 = a.lse_in ? (ok ? a.lse_in[r * a.nhead + h] : 0.f)
                                : M + __builtin_amdgcn_logf(xg_sum(m == -INFINITY ? 0.f : l * __builtin_amdgcn_exp2f(m - M)));
    // pass 2: P, dP, dS and dQ^T += K^T dS^T
    f32x4 dq[DT];
#pragma unroll
    for (int t = 0; t < DT; ++t) dq[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int64_t t0 = kb; t0 < ke; t0 += 64) {
        const int nt = (int)min((int64_t)64, ke - t0);
        __syncthreads();
        stage_rows<DH, LD>(kt, a.k + t0 * a.ldk + h * DH, a.ldk, nt, 1.f);
        stage_rows<DH, LD>(vt, a.v + t0 * a.ldv + h * DH, a.ldv, nt, 1.f);
        __syncthreads();
        float ds[4][4];
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const f32x4 s4 = scores(kt, qv, n);
            const f32x4 p4 = scores(vt, dov, n);                // dP^T = V dO^T
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const bool in = 16 * n + 4 * g + rr < nt;
                const float p = in ? __builtin_amdgcn_exp2f(s4[rr] - lse2) : 0.f;
                float dp = p4[rr];
                if constexpr (DROP)
                    dp = attn_drop_hash(a.drop_seed, h, r, t0 + 16 * n + 4 * g + rr) < a.drop_thresh
                             ? 0.f : dp * a.inv_keep;
                ds[n][rr] = p * (dp - dsum);
            }
        }
#pragma unroll
        for (int t = 0; t < DT; ++t)
#pragma unroll
            for (int n = 0; n < 4; ++n)
#pragma unroll
                for (int rr = 0; rr < 4; ++rr)
                    dq[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                        kt[(16 * n + 4 * g + rr) * LD + 16 * t + c], ds[n][rr], dq[t], 0, 0, 0);
    }
    // dQ = scale * sum dS K; lane (g, c) holds dims 16t + 4g .. + 3 of query c
    const int64_t rq = qb0 + (int64_t)qb * 64 + wv * 16 + c;
    if (rq < qe) {
#pragma unroll
        for (int t = 0; t < DT; ++t)
            *reinterpret_cast<float4*>(a.dq + rq * a.lddq + h * DH + 16 * t + 4 * g) =
                make_float4(dq[t][0] * a.scale, dq[t][1] * a.scale, dq[t][2] * a.scale, dq[t][3] * a.scale);
        if (g == 0) {
            a.lse[rq * a.nhead + h] = lse2;
            a.dsum[rq * a.nhead + h] = dsum;
        }
    }
}

template <int DH, bool DROP = false>
__global__ void __launch_bounds__(256)
attn_bwd_dkdv_mfma_kernel(AttnBwd a) {
    constexpr int KS = DH / 4, DT = DH / 16, LD = DH + 4;
    __shared__ float qt[64 * LD];
    __shared__ float dt[64 * LD];
    __shared__ float lt[64], st[64];
    const int ks = blockIdx.x / a.kv_blocks, kbk = blockIdx.x % a.kv_blocks, h = blockIdx.y;
    const int64_t kb0 = a.kv_off[ks], ke = a.kv_off[ks + 1];
    if (kb0 + (int64_t)kbk * 64 >= ke) return;
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, g = lane >> 4, c = lane & 15;
    const int64_t rk = kb0 + (int64_t)kbk * 64 + wv * 16 + c;   // this lane's key row
    const bool ok = rk < ke;
    float kv[KS], vv[KS];
    load_ks<KS>(a.k + rk * a.ldk + h * DH + g * KS, kv, ok, 1.f);
    load_ks<KS>(a.v + rk * a.ldv + h * DH + g * KS, vv, ok, 1.f);
    f32x4 dk[DT], dv[DT];
#pragma unroll
    for (int t = 0; t < DT; ++t) dk[t] = dv[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int seg = 0; seg < a.n_seg; ++seg) {
        if (a.kv_seg[seg] != ks) continue;
        const int64_t qb = a.q_off[seg], qe = a.q_off[seg + 1];
        for (int64_t t0 = qb; t0 < qe; t0 += 64) {
            const int nt = (int)min((int64_t)64, qe - t0);
            __syncthreads();
            stage_rows<DH, LD>(qt, a.q + t0 * a.ldq + h * DH, a.ldq, nt, a.scale * kLog2e);
            stage_rows<DH, LD>(dt, a.dout + t0 * a.lddo + h * DH, a.lddo, nt, 1.f);
            if (tid < 64) {
                lt[tid] = tid < nt ? a.lse[(t0 + tid) * a.nhead + h] : INFINITY;   // P = 0 past the end
                st[tid] = tid < nt ? a.dsum[(t0 + tid) * a.nhead + h] : 0.f;
            }
            __syncthreads();
            float p[4][4], ds[4][4];
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                // S[query 16n + 4g + r][key c] = Q K^T, dP = dO V^T
                f32x4 s4 = {0.f, 0.f, 0.f, 0.f}, d4 = s4;
                const float* qr = qt + (16 * n + c) * LD + g * KS;
                const float* dr = dt + (16 * n + c) * LD + g * KS;
#pragma unroll
                for (int s = 0; s < KS; ++s) {
                    s4 = __builtin_amdgcn_mfma_f32_16x16x4f32(qr[s], kv[s], s4, 0, 0, 0);
                    d4 = __builtin_amdgcn_mfma_f32_16x16x4f32(dr[s], vv[s], d4, 0, 0, 0);
                }
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    const int qi = 16 * n + 4 * g + rr;
                    const float pv = __builtin_amdgcn_exp2f(s4[rr] - lt[qi]);
                    if constexpr (DROP) {
                        const float mk = attn_drop_hash(a.drop_seed, h, t0 + qi, rk) < a.drop_thresh
                                             ? 0.f : a.inv_keep;
                        p[n][rr] = pv * mk;                    // dV uses the dropped weights
                        ds[n][rr] = pv * (d4[rr] * mk - st[qi]);
                    } else {
                        p[n][rr] = pv;
                        ds[n][rr] = pv * (d4[rr] - st[qi]);
                    }
                }
            }
            // dV^T += dO^T P, dK^T += Q^T dS (k-step (n, r): query 16n + 4g + r)
#pragma unroll
            for (int t = 0; t < DT; ++t)
#pragma unroll
                for (int n = 0; n < 4; ++n)
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr) {
                        const int qi = 16 * n + 4 * g + rr;
                        dv[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(dt[qi * LD + 16 * t + c], p[n][rr], dv[t], 0, 0, 0);
                        dk[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(qt[qi * LD + 16 * t + c], ds[n][rr], dk[t], 0, 0, 0);
                    }
        }
    }
    if (!ok) return;
    // the staged q carried scale * log2 e: dK = scale * sum dS q = (sum dS qt) / log2 e
    constexpr float il2 = 1.0f / kLog2e;
#pragma unroll
    for (int t = 0; t < DT; ++t) {
        *reinterpret_cast<float4*>(a.dk + rk * a.lddk + h * DH + 16 * t + 4 * g) =
            make_float4(dk[t][0] * il2, dk[t][1] * il2, dk[t][2] * il2, dk[t][3] * il2);
        *reinterpret_cast<float4*>(a.dv + rk * a.lddv + h * DH + 16 * t + 4 * g) =
            make_float4(dv[t][0], dv[t][1], dv[t][2], dv[t][3]);
    }
}

}  // namespace
}  // namespace fgr

using namespace fgr;

extern "C" int fgr_attention_bwd_workspace(int64_t nq, int32_t nhead, size_t* bytes) {
    FGR_REQUIRE(bytes && nq >= 0 && nhead > 0, "fgr_attention_bwd_workspace: bad arguments");
    *bytes = (size_t)std::max<int64_t>(nq, 1) * nhead * 2 * sizeof(float);
    return FGR_OK;
}

static int attention_bwd_impl(const float* q, int64_t ldq, const float* k, int64_t ldk,
                              const float* v, int64_t ldv, const float* o, int64_t ldo,
                              const float* dout, int64_t lddo, float* dq, int64_t lddq, float* dk,
                              int64_t lddk, float* dv, int64_t lddv, const int64_t* q_off,
                              const int64_t* kv_off, const int32_t* kv_seg, int32_t n_seg,
                              int32_t n_kv_seg, int64_t nq, int64_t max_q_len, int64_t max_kv_len,
                              int32_t nhead, int32_t dh, float scale, void* ws, size_t ws_bytes,
                              uint32_t drop_seed, float drop_p, void* stream,
                              const float* lse_in = nullptr, int64_t n_kv_rows = -1) {
    FGR_REQUIRE(n_seg > 0 && n_kv_seg > 0 && nhead > 0 && nq >= 0 &&
                    (dh == 4 || dh == 8 || dh == 16 || dh == 32 || dh == 64),
                "fgr_attention_bwd: bad arguments (head dim 4 / 8 / 16 / 32 / 64)");
    FGR_REQUIRE(q && k && v && o && dout && dq && dk && dv && q_off && kv_off && kv_seg && ws,
                "fgr_attention_bwd: null pointer");
    size_t need = 0;
    fgr_attention_bwd_workspace(nq, nhead, &need);
    FGR_REQUIRE(ws_bytes >= need, "fgr_attention_bwd: workspace too small");
    AttnBwd a{q, ldq, k, ldk, v, ldv, o, ldo, dout, lddo, dq, lddq, dk, lddk, dv, lddv, q_off, kv_off,
              kv_seg, n_seg, n_kv_seg, nhead, (int)std::max<int64_t>(1, ceil_div(max_q_len, 64)),
              (int)std::max<int64_t>(1, ceil_div(max_kv_len, 64)), scale, (float*)ws,
              (float*)ws + std::max<int64_t>(nq, 1) * nhead, drop_seed,
              (uint32_t)std::min(4294967295.0, (double)drop_p * 4294967296.0),
              drop_p > 0.f ? 1.0f / (1.0f - drop_p) : 1.f, lse_in};
    const bool drop = drop_p > 0.f;
    hipStream_t st = as_stream(stream);
    dim3 g1((unsigned)(n_seg * a.q_blocks), nhead), g2((unsigned)(n_kv_seg * a.kv_blocks), nhead);
    // head dim 16 / 32 / 64 with 16-B aligned rows: the fp32-MFMA kernels
    const bool al = ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k) |
                      reinterpret_cast<uintptr_t>(v) | reinterpret_cast<uintptr_t>(o) |
                      reinterpret_cast<uintptr_t>(dout) | reinterpret_cast<uintptr_t>(dq) |
                      reinterpret_cast<uintptr_t>(dk) | reinterpret_cast<uintptr_t>(dv)) & 15) == 0 &&
                    (ldq | ldk | ldv | ldo | lddo | lddq | lddk | lddv) % 4 == 0;
    const bool mfma = al && (dh == 16 || dh == 32 || dh == 64);
    FGR_REQUIRE(!drop || (al && (dh == 16 || dh == 32 || dh == 64)),
                "fgr_attention_bwd_drop: dropout needs head dim 16 / 32 / 64 and 16-B aligned rows");
    // training with the forward's lse (head dim 32 / 64): the f16x3 kernels (attention16.hip
    // attn_bwd_f16x3), their K / V / Q / dO images after lse / D in ws
    // (fgr_attention_bwd_train_workspace)
    const size_t lse_bytes = (need + 255) & ~(size_t)255;
    const int64_t n_rows = std::max(nq, n_kv_rows);
    if (lse_in && n_kv_rows >= 0 && al && (dh == 32 || dh == 64) &&
        ws_bytes >= lse_bytes + attn_bwd_f16x3_bytes(n_rows, std::max(n_seg, n_kv_seg), nhead, dh)) {
        FGR_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15) == 0, "fgr_attention_bwd_train: ws alignment");
        return attn_bwd_f16x3(q, ldq, k, ldk, v, ldv, o, ldo, dout, lddo, dq, lddq, dk, lddk, dv,
                              lddv, q_off, kv_off, kv_seg, n_seg, n_kv_seg, n_rows, max_q_len,
                              max_kv_len, nhead, dh, scale, lse_in, a.dsum,
                              static_cast<char*>(ws) + lse_bytes, a.drop_seed, a.drop_thresh,
                              a.inv_keep, st);
    }
    if (drop) {
        switch (dh) {
#define ATD(D) case D: \
            hipLaunchKernelGGL((attn_bwd_dq_mfma_kernel<D, true>), g1, dim3(256), 0, st, a); \
            FGR_CHECK_LAUNCH("attn_bwd_dq_mfma_kernel"); \
            hipLaunchKernelGGL((attn_bwd_dkdv_mfma_kernel<D, true>), g2, dim3(256), 0, st, a); \
            break;
            ATD(16) ATD(32) ATD(64)
#undef ATD
        }
        FGR_CHECK_LAUNCH("attn_bwd_dkdv_mfma_kernel");
        return FGR_OK;
    }
    if (mfma) {
        switch (dh) {
#define ATM(D) case D: \
            hipLaunchKernelGGL(attn_bwd_dq_mfma_kernel<D>, g1, dim3(256), 0, st, a); \
            FGR_CHECK_LAUNCH("attn_bwd_dq_mfma_kernel"); \
            hipLaunchKernelGGL(attn_bwd_dkdv_mfma_kernel<D>, g2, dim3(256), 0, st, a); \
            break;
            ATM(16) ATM(32) ATM(64)
#undef ATM
        }
        FGR_CHECK_LAUNCH("attn_bwd_dkdv_mfma_kernel");
        return FGR_OK;
    }
    switch (dh) {
#define ATB(D) case D: \
        hipLaunchKernelGGL(attn_bwd_dq_kernel<D>, g1, dim3(64), 0, st, a); \
        FGR_CHECK_LAUNCH("attn_bwd_dq_kernel"); \
        hipLaunchKernelGGL(attn_bwd_dkdv_kernel<D>, g2, dim3(64), 0, st, a); \
        break;
        ATB(4) ATB(8) ATB(16) ATB(32) ATB(64)
#undef ATB
    }
    FGR_CHECK_LAUNCH("attn_bwd_dkdv_kernel");
    return FGR_OK;
}

extern "C" int fgr_attention_bwd(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v,
                                 int64_t ldv, const float* o, int64_t ldo, const float* dout,
                                 int64_t lddo, float* dq, int64_t lddq, float* dk, int64_t lddk,
                                 float* dv, int64_t lddv, const int64_t* q_off, const int64_t* kv_off,
                                 const int32_t* kv_seg, int32_t n_seg, int32_t n_kv_seg, int64_t nq,
                                 int64_t max_q_len, int64_t max_kv_len, int32_t nhead, int32_t dh,
                                 float scale, void* ws, size_t ws_bytes, void* stream) {
    return attention_bwd_impl(q, ldq, k, ldk, v, ldv, o, ldo, dout, lddo, dq, lddq, dk, lddk, dv,
                              lddv, q_off, kv_off, kv_seg, n_seg, n_kv_seg, nq, max_q_len,
                              max_kv_len, nhead, dh, scale, ws, ws_bytes, 0u, 0.f, stream);
}

extern "C" int fgr_attention_bwd_train(const float* q, int64_t ldq, const float* k, int64_t ldk,
                                       const float* v, int64_t ldv, const float* o, int64_t ldo,
                                       const float* dout, int64_t lddo, float* dq, int64_t lddq,
                                       float* dk, int64_t lddk, float* dv, int64_t lddv,
                                       const int64_t* q_off, const int64_t* kv_off,
                                       const int32_t* kv_seg, int32_t n_seg, int32_t n_kv_seg,
                                       int64_t nq, int64_t max_q_len, int64_t max_kv_len,
                                       int32_t nhead, int32_t dh, float scale, void* ws,
                                       size_t ws_bytes, uint32_t seed, float p, const float* lse,
                                       int64_t n_kv_rows, void* stream) {
    FGR_REQUIRE(p >= 0.f && p < 1.f, "fgr_attention_bwd_train: dropout p %f not in [0, 1)", p);
    FGR_REQUIRE(lse, "fgr_attention_bwd_train: null lse");
    return attention_bwd_impl(q, ldq, k, ldk, v, ldv, o, ldo, dout, lddo, dq, lddq, dk, lddk, dv,
                              lddv, q_off, kv_off, kv_seg, n_seg, n_kv_seg, nq, max_q_len,
                              max_kv_len, nhead, dh, scale, ws, ws_bytes, seed, p, stream, lse,
                              n_kv_rows);
}

// fgr_attention_bwd_train's workspace: lse / D per (query row, head), then (head dim 32 / 64)
// the f16x3 kernels' K / V / Q / dO tile images (nq query rows in n_seg segments, n_kv_rows key
// rows in n_kv_seg segments, one packed row space)
extern "C" int fgr_attention_bwd_train_workspace(int64_t nq, int32_t n_seg, int64_t n_kv_rows,
                                                 int32_t n_kv_seg, int32_t nhead, int32_t dh,
                                                 size_t* bytes) {
    FGR_REQUIRE(bytes && nq >= 0 && n_seg > 0 && n_kv_rows >= 0 && n_kv_seg > 0 && nhead > 0,
                "fgr_attention_bwd_train_workspace: bad arguments");
    size_t need = 0;
    fgr_attention_bwd_workspace(nq, nhead, &need);
    *bytes = need;
    if (dh == 32 || dh == 64)
        *bytes = ((need + 255) & ~(size_t)255) +
                 attn_bwd_f16x3_bytes(std::max(nq, n_kv_rows), std::max(n_seg, n_kv_seg), nhead, dh);
    return FGR_OK;
}

extern "C" int fgr_attention_bwd_drop(const float* q, int64_t ldq, const float* k, int64_t ldk,
                                      const float* v, int64_t ldv, const float* o, int64_t ldo,
                                      const float* dout, int64_t lddo, float* dq, int64_t lddq,
                                      float* dk, int64_t lddk, float* dv, int64_t lddv,
                                      const int64_t* q_off, const int64_t* kv_off,
                                      const int32_t* kv_seg, int32_t n_seg, int32_t n_kv_seg,
                                      int64_t nq, int64_t max_q_len, int64_t max_kv_len,
                                      int32_t nhead, int32_t dh, float scale, void* ws,
                                      size_t ws_bytes, uint32_t seed, float p, void* stream) {
    FGR_REQUIRE(p >= 0.f && p < 1.f, "fgr_attention_bwd_drop: dropout p %f not in [0, 1)", p);
    return attention_bwd_impl(q, ldq, k, ldk, v, ldv, o, ldo, dout, lddo, dq, lddq, dk, lddk, dv,
                              lddv, q_off, kv_off, kv_seg, n_seg, n_kv_seg, nq, max_q_len,
                              max_kv_len, nhead, dh, scale, ws, ws_bytes, seed, p, stream);
}
