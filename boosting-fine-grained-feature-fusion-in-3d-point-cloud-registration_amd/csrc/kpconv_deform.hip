// Deformable (and modulated) KPConv on gfx950: the `deformable` branch of KPConv.forward
// (finegrained_kpconv_blocks.py:270-345, :384-385), forward and backward.
//
// A rigid "offset" KPConv (fgr_kpconv_gather_mode + the weight GEMM) gives 3K (4K when modulated)
// offset features per query. From them
//   fgr_kpconv_deform_points   kp_q[q, k, :] = kp[k] + extent * f[q, 3k : 3k + 3],
//                              mod[q, k] = 2 sigmoid(f[q, 3K + k]),  f = raw / nnorm + bias
//   fgr_kpconv_gather_deform   wf[q, k, c] = mod[q, k] sum_{in-range h} w(d2[q, h, k]) x[idx[q, h], c]
//                              nnorm[q] = max(1, #{in-range h : sum_c x[idx[q, h], c] > 0})
//   fgr_kpconv_scatter_deform  dx of that gather over the table's CSR inverse (fgr_nbr_inverse)
//   fgr_kpconv_deform_grad     d_kp[q, k, :] and d_mod[q, k] of that gather
// with d2[q, h, k] = |(s[idx[q, h]] - q) - kp_q[q, k]|^2 and w the influence of common.h.
//
// In-range rule: a valid neighbour is in range iff d2 < extent^2 for some k; one that is not is
// a shadow (zero feature row, not counted by nnorm). The reference re-indexes its tables with a
// topk whose width it reads back to the host (:319-343); here a lane that holds a valid
// neighbour walks its K distances first and the ballot that compacts the chunk takes the
// in-range lanes only, so nothing leaves the device and the forward stays graph-capturable.
// The in-range mask and the closest one-hot are constants of the backward.
//
// load_vec / store_wf / the closest stage restate kpconv.hip's (file-local there; the rigid
// kernels are not touched by this file).
#include "mfma.h"

#include <algorithm>

namespace fgr {
namespace {

constexpr int kMaxKpD = 32;        // kernel points supported (configs use 15)
constexpr int kWavesD = 4;         // waves (= queries) per block
constexpr int kUD = 4;             // neighbour rows in flight per wave

template <int VEC>
__device__ __forceinline__ void load_vec(const float* p, float (&v)[VEC]) {
    if constexpr (VEC == 1) {
        v[0] = p[0];
    } else if constexpr (VEC == 2) {
        float2 t = *reinterpret_cast<const float2*>(p);
        v[0] = t.x; v[1] = t.y;
    } else {
        float4 t = *reinterpret_cast<const float4*>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    }
}

typedef float wf4 __attribute__((ext_vector_type(4)));
typedef float wf2 __attribute__((ext_vector_type(2)));

// wf rows are written once and read once, by the weight GEMM: non-temporal stores
template <int VEC>
__device__ __forceinline__ void store_wf(float* p, const float (&v)[VEC]) {
    if constexpr (VEC == 1) {
        __builtin_nontemporal_store(v[0], p);
    } else if constexpr (VEC == 2) {
        __builtin_nontemporal_store(wf2{v[0], v[1]}, reinterpret_cast<wf2*>(p));
    } else {
        __builtin_nontemporal_store(wf4{v[0], v[1], v[2], v[3]}, reinterpret_cast<wf4*>(p));
    }
}

// min_k d2 of a centred neighbour under the query's own kernel points (LDS, every lane reads
// the same address: a broadcast) and its argmin (the lowest k on a tie, as torch.argmin)
__device__ __forceinline__ float nearest_kp(float nx, float ny, float nz, const float* kp, int n_kp,
                                            int* best_k) {
    float best = kp_d2(nx, ny, nz, kp, 0);
    int bk = 0;
#pragma unroll 4
    for (int k = 1; k < n_kp; ++k) {
        const float d2 = kp_d2(nx, ny, nz, kp, k);
        if (d2 < best) { best = d2; bk = k; }
    }
    *best_k = bk;
    return best;
}

// One wave per query. WIDE: cin = 64 * VEC with channels on lanes, VEC contiguous floats per
// lane (16-B row loads at cin 256). Narrow (!WIDE, VEC 1): cin <= 64 at run time, lane c owns
// channel c and the lanes past cin idle. The query's K deformed kernel points (and its K
// modulations) sit in the wave's LDS slice. Per 64-wide chunk of the row: every lane that
// holds a valid neighbour takes its K distances, the in-range ones are compacted by ballot,
// their influences go to LDS once and their feature rows are streamed kUD at a time into K
// accumulators; the normaliser's "row sum > 0" is a DPP wave sum of the rows as they stream by.
// Pad rows and columns k >= n_kp get weight 0 in every mode (a constant influence taken from
// the function would add feature row 0).
template <int VEC, int KU, bool WIDE, int INF, int AGG>
__global__ void __launch_bounds__(64 * kWavesD)
kpconv_gather_deform_kernel(const float* __restrict__ q, const float* __restrict__ s, int64_t nq,
                            int64_t ns, const int64_t* __restrict__ idx, int width,
                            const float* __restrict__ x, int cin, const float* __restrict__ kp_q,
                            const float* __restrict__ mod, int n_kp, float wscale, float e2,
                            float* __restrict__ wf, float* __restrict__ nnorm) {
    constexpr int U = kUD;
    static_assert(KU % 4 == 0 && (WIDE || VEC == 1), "instances");
    __shared__ __attribute__((aligned(16))) float w_lds[kWavesD][64 + U][KU];
    __shared__ int nb_lds[kWavesD][64 + U];
    __shared__ float3 p_lds[kWavesD][64];
    __shared__ float kp_lds[kWavesD][3 * kMaxKpD];
    __shared__ float mod_lds[kWavesD][kMaxKpD];
    const int wv = threadIdx.x / 64, lane = threadIdx.x % 64;
    const int64_t qi = (int64_t)blockIdx.x * kWavesD + wv;
    if (qi >= nq) return;                               // no block-wide barrier below
    float* kp = kp_lds[wv];
    for (int i = lane; i < 3 * n_kp; i += 64) kp[i] = kp_q[qi * 3 * n_kp + i];
    // the modulations are fetched with the kernel points: loads issued between the wf stores of
    // the epilogue would each wait for the stores before them (measured: + 4 to 10 us a launch)
    if (lane < n_kp) mod_lds[wv][lane] = mod ? mod[qi * n_kp + lane] : 1.0f;
    __builtin_amdgcn_wave_barrier();
    const float qx = q[3 * qi], qy = q[3 * qi + 1], qz = q[3 * qi + 2];
    const bool chan = WIDE || lane < cin;               // this lane owns channels
    const int64_t coff = WIDE ? lane * VEC : (chan ? lane : 0);

    float acc[KU][VEC];
#pragma unroll
    for (int k = 0; k < KU; ++k)
#pragma unroll
        for (int j = 0; j < VEC; ++j) acc[k][j] = 0.f;
    int n_pos = 0;
    const int64_t* row = idx + qi * width;

    for (int h0 = 0; h0 < width; h0 += 64) {
        const int h = h0 + lane;
        const int64_t id = h < width ? row[h] : ns;
        bool live = id >= 0 && id < ns;
        float3 d = make_float3(0.f, 0.f, 0.f);
        if (live) {
            // neighbours are centred first, then compared with the kernel points (:302, :313)
            d = make_float3(s[3 * id] - qx, s[3 * id + 1] - qy, s[3 * id + 2] - qz);
            int bk;
            live = nearest_kp(d.x, d.y, d.z, kp, n_kp, &bk) < e2;       // :325
        }
        const unsigned long long m = __ballot(live);
        const int v = __popcll(m);
        if (v == 0) continue;
        if (live) {
            const int p = __popcll(m & ((1ull << lane) - 1ull));
            nb_lds[wv][p] = (int)id;
            p_lds[wv][p] = d;
        }
        if (lane < U) nb_lds[wv][v + lane] = 0;         // pad rows: weight 0, row 0
        __builtin_amdgcn_wave_barrier();
        if constexpr (AGG == FGR_AGG_CLOSEST) {
            for (int t = lane; t < U * KU; t += 64) w_lds[wv][v + t / KU][t % KU] = 0.f;
            for (int hh = lane; hh < v; hh += 64) {
                const float3 c = p_lds[wv][hh];
                int bk;
                const float wb = kp_influence<INF>(nearest_kp(c.x, c.y, c.z, kp, n_kp, &bk), wscale);
#pragma unroll
                for (int k = 0; k < KU; k += 4)
                    *reinterpret_cast<float4*>(&w_lds[wv][hh][k]) =
                        make_float4(k == bk ? wb : 0.f, k + 1 == bk ? wb : 0.f,
                                    k + 2 == bk ? wb : 0.f, k + 3 == bk ? wb : 0.f);
            }
        } else {
            for (int t = lane; t < (v + U) * KU; t += 64) {
                const int hh = t / KU, k = t - hh * KU;
                float w = 0.f;
                if (hh < v && k < n_kp) {
                    const float3 c = p_lds[wv][hh];
                    w = kp_weight<INF>(c.x, c.y, c.z, kp, k, wscale);
                }
                w_lds[wv][hh][k] = w;
            }
        }
        __builtin_amdgcn_wave_barrier();
        for (int hh = 0; hh < v; hh += U) {
            float xv[U][VEC];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if constexpr (WIDE) {
                    load_vec<VEC>(x + (int64_t)nb_lds[wv][hh + u] * (64 * VEC) + coff, xv[u]);
                } else {
                    const float t = x[(int64_t)nb_lds[wv][hh + u] * cin + coff];
                    xv[u][0] = chan ? t : 0.f;
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                float t = 0.f;
#pragma unroll
                for (int j = 0; j < VEC; ++j) t += xv[u][j];
                t = wave_sum_dpp(t);
                n_pos += (hh + u < v && t > 0.f) ? 1 : 0;
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int k = 0; k < KU; ++k) {
                    const float w = w_lds[wv][hh + u][k];
#pragma unroll
                    for (int j = 0; j < VEC; ++j) acc[k][j] = fmaf(w, xv[u][j], acc[k][j]);
                }
        }
        __builtin_amdgcn_wave_barrier();
    }
    const int64_t cw = WIDE ? 64 * VEC : cin;
    float* out = wf + qi * (int64_t)n_kp * cw + coff;
#pragma unroll
    for (int k = 0; k < KU; ++k)
        if (k < n_kp && chan) {
            if (mod) {                                  // :384-385
                const float mk = mod_lds[wv][k];
#pragma unroll
                for (int j = 0; j < VEC; ++j) acc[k][j] *= mk;
            }
            store_wf<VEC>(out + (int64_t)k * cw, acc[k]);
        }
    if (lane == 0) nnorm[qi] = (float)(n_pos > 1 ? n_pos : 1);
}

// Thread per (query, kernel point): the offset features f = raw / nnorm + bias (:272, the
// offset conv's own division :395-399), the deformed kernel point kp + extent * f[3k : 3k + 3]
// (two roundings, as :286 and :306) and the modulation 2 sigmoid(f[3K + k]) (:279).
__global__ void __launch_bounds__(256)
deform_points_kernel(const float* __restrict__ raw, const float* __restrict__ rn,
                     const float* __restrict__ bias, const float* __restrict__ kp, int64_t nq,
                     int n_kp, float extent, float* __restrict__ kp_q, float* __restrict__ mod) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= nq * n_kp) return;
    const int64_t qi = t / n_kp;
    const int k = (int)(t - qi * n_kp);
    const int dim = (mod ? 4 : 3) * n_kp;
    const float* r = raw + qi * dim;
    const float n = rn[qi];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float f = __fadd_rn(__fdiv_rn(r[3 * k + i], n), bias[3 * k + i]);
        kp_q[3 * t + i] = __fadd_rn(__fmul_rn(f, extent), kp[3 * k + i]);
    }
    if (mod) {
        const float f = __fadd_rn(__fdiv_rn(r[3 * n_kp + k], n), bias[3 * n_kp + k]);
        mod[t] = 2.0f / (1.0f + expf(-f));
    }
}

// fgr_kpconv_scatter's recipe (train.hip) under the query's own kernel points: one wave per
// query, the valid neighbours of a chunk compacted by ballot with their K masked, modulated
// influences in LDS (a valid neighbour out of range keeps its CSR slot and writes zeros to it);
// per 64-channel slice the query's dwf rows are held in registers and every neighbour's
// sum_k mod_k w_hk dwf[q, k, c] goes to its slot g[pos[q * width + h], c].
template <int INF, int AGG>
__global__ void __launch_bounds__(256)
kpconv_scatter_deform_kernel(const float* __restrict__ q, const float* __restrict__ s, int64_t nq,
                             int64_t ns, const int64_t* __restrict__ idx, int width,
                             const float* __restrict__ dwf, int cin, const float* __restrict__ kp_q,
                             const float* __restrict__ mod, int n_kp, float wscale, float e2,
                             const int* __restrict__ pos, float* __restrict__ g) {
    __shared__ float w_lds[4][64][kMaxKpD + 1];
    __shared__ int slot_lds[4][64];
    __shared__ float kp_lds[4][3 * kMaxKpD];
    __shared__ float mod_lds[4][kMaxKpD];
    const int wv = threadIdx.x / 64, lane = threadIdx.x % 64;
    const int64_t qi = (int64_t)blockIdx.x * 4 + wv;
    if (qi >= nq) return;
    float* kp = kp_lds[wv];
    for (int i = lane; i < 3 * n_kp; i += 64) kp[i] = kp_q[qi * 3 * n_kp + i];
    if (lane < n_kp) mod_lds[wv][lane] = mod ? mod[qi * n_kp + lane] : 1.0f;
    __builtin_amdgcn_wave_barrier();
    const float qx = q[3 * qi], qy = q[3 * qi + 1], qz = q[3 * qi + 2];
    const int64_t* row = idx + qi * width;
    const float* dq = dwf + qi * (int64_t)n_kp * cin;
    for (int h0 = 0; h0 < width; h0 += 64) {
        const int h = h0 + lane;
        const int64_t id = h < width ? row[h] : ns;
        const bool valid = id >= 0 && id < ns;
        const unsigned long long m = __ballot(valid);
        const int v = __popcll(m);
        if (v == 0) continue;
        if (valid) {
            const int p = __popcll(m & ((1ull << lane) - 1ull));
            slot_lds[wv][p] = pos[qi * width + h];
            const float nx = s[3 * id] - qx, ny = s[3 * id + 1] - qy, nz = s[3 * id + 2] - qz;
            int bk;
            const float best = nearest_kp(nx, ny, nz, kp, n_kp, &bk);
            const bool in_range = best < e2;
            for (int k = 0; k < n_kp; ++k) {
                float w;
                if constexpr (AGG == FGR_AGG_CLOSEST) w = k == bk ? kp_influence<INF>(best, wscale) : 0.f;
                else w = kp_weight<INF>(nx, ny, nz, kp, k, wscale);
                w_lds[wv][p][k] = in_range ? w * mod_lds[wv][k] : 0.f;
            }
        }
        __builtin_amdgcn_wave_barrier();
        for (int c0 = 0; c0 < cin; c0 += 64) {
            const int c = c0 + lane;
            const bool act = c < cin;
            float dw[kMaxKpD];
#pragma unroll
            for (int k = 0; k < kMaxKpD; ++k)
                dw[k] = (act && k < n_kp) ? dq[(int64_t)k * cin + c] : 0.f;
            for (int hh = 0; hh < v; ++hh) {
                float acc = 0.f;
#pragma unroll
                for (int k = 0; k < kMaxKpD; ++k)
                    if (k < n_kp) acc = fmaf(w_lds[wv][hh][k], dw[k], acc);
                if (act) g[(int64_t)slot_lds[wv][hh] * cin + c] = acc;
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// dx[s, c] = the sum of support row s's CSR slots in slot (= ascending entry) order
__global__ void __launch_bounds__(256)
deform_rowsum_kernel(const int* __restrict__ start, int64_t ns, const float* __restrict__ g, int cin,
                     float* __restrict__ dx) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= ns * cin) return;
    const int64_t sr = t / cin;
    const int c = (int)(t - sr * cin);
    const int b = start[sr], e = start[sr + 1];
    float acc = 0.f;
    for (int j = b; j < e; ++j) acc += g[(int64_t)j * cin + c];
    dx[t] = acc;
}

// d_kp, d_mod of the gather: with A[q, k, c] = sum_h w_hk x_h,c (wf = mod A) and
// G[h, k] = sum_c dwf[q, k, c] x[idx[q, h], c],
//   d_mod[q, k]   = sum_{in-range h} G[h, k] w_hk
//   d_kp[q, k, :] = mod[q, k] sum_{in-range h} G[h, k] dw_hk/dkp,
//   dw/dkp = (n_h - kp_k) / (extent |n_h - kp_k|) where w > 0 (linear; 0 at d2 = 0, where the
//   reference's sqrt gives NaN), 2 wscale w (n_h - kp_k) (gaussian), 0 (constant),
// times the closest one-hot. One wave per query, so every (q, k) has one owner: a lane takes one
// in-range neighbour, walks its feature row against the query's dwf rows (the same address in
// every lane) for the K dot products, and the lanes are summed in the fixed order of the DPP /
// permlane tree; chunks add in order. No atomics: two runs are bit-equal.
template <int INF, int AGG>
__global__ void __launch_bounds__(256)
kpconv_deform_grad_kernel(const float* __restrict__ q, const float* __restrict__ s, int64_t nq,
                          int64_t ns, const int64_t* __restrict__ idx, int width,
                          const float* __restrict__ x, int cin, const float* __restrict__ dwf,
                          const float* __restrict__ kp_q, const float* __restrict__ mod, int n_kp,
                          float wscale, float e2, float* __restrict__ d_kp,
                          float* __restrict__ d_mod) {
    __shared__ float kp_lds[4][3 * kMaxKpD];
    const int wv = threadIdx.x / 64, lane = threadIdx.x % 64;
    const int64_t qi = (int64_t)blockIdx.x * 4 + wv;
    if (qi >= nq) return;
    float* kp = kp_lds[wv];
    for (int i = lane; i < 3 * n_kp; i += 64) kp[i] = kp_q[qi * 3 * n_kp + i];
    __builtin_amdgcn_wave_barrier();
    const float qx = q[3 * qi], qy = q[3 * qi + 1], qz = q[3 * qi + 2];
    const int64_t* row = idx + qi * width;
    const float* dq = dwf + qi * (int64_t)n_kp * cin;
    float gx = 0.f, gy = 0.f, gz = 0.f, gm = 0.f;      // lane k: the sums of kernel point k
    for (int h0 = 0; h0 < width; h0 += 64) {
        const int h = h0 + lane;
        const int64_t id = h < width ? row[h] : ns;
        bool live = id >= 0 && id < ns;
        float nx = 0.f, ny = 0.f, nz = 0.f;
        int bk = 0;
        if (live) {
            nx = s[3 * id] - qx; ny = s[3 * id + 1] - qy; nz = s[3 * id + 2] - qz;
            live = nearest_kp(nx, ny, nz, kp, n_kp, &bk) < e2;
        }
        if (__ballot(live) == 0ull) continue;
        float G[kMaxKpD];
#pragma unroll
        for (int k = 0; k < kMaxKpD; ++k) G[k] = 0.f;
        if (live) {
            const float* xr = x + id * cin;
            for (int c = 0; c < cin; ++c) {
                const float xv = xr[c];
#pragma unroll
                for (int k = 0; k < kMaxKpD; ++k)
                    if (k < n_kp) G[k] = fmaf(dq[(int64_t)k * cin + c], xv, G[k]);
            }
        }
#pragma unroll
        for (int k = 0; k < kMaxKpD; ++k) {
            if (k >= n_kp) continue;                    // wave-uniform
            float tm = 0.f, tx = 0.f, ty = 0.f, tz = 0.f;
            if (live && (AGG != FGR_AGG_CLOSEST || k == bk)) {
                const float ex = nx - kp[3 * k], ey = ny - kp[3 * k + 1], ez = nz - kp[3 * k + 2];
                const float d2 = ex * ex + ey * ey + ez * ez;
                const float w = kp_influence<INF>(d2, wscale);
                float cf = 0.f;
                if constexpr (INF == FGR_KP_LINEAR) cf = (w > 0.f && d2 > 0.f) ? wscale / sqrtf(d2) : 0.f;
                else if constexpr (INF == FGR_KP_GAUSSIAN) cf = 2.0f * wscale * w;
                tm = G[k] * w;
                const float gc = G[k] * cf;
                tx = gc * ex; ty = gc * ey; tz = gc * ez;
            }
            tm = wave_sum_dpp(tm);
            if constexpr (INF != FGR_KP_CONSTANT) {
                tx = wave_sum_dpp(tx); ty = wave_sum_dpp(ty); tz = wave_sum_dpp(tz);
            }
            if (lane == k) { gm += tm; gx += tx; gy += ty; gz += tz; }
        }
    }
    if (lane < n_kp) {
        const float mk = mod ? mod[qi * n_kp + lane] : 1.0f;
        float* o = d_kp + (qi * n_kp + lane) * 3;
        o[0] = mk * gx; o[1] = mk * gy; o[2] = mk * gz;
        if (d_mod) d_mod[qi * n_kp + lane] = gm;
    }
}

struct DeformArgs {
    const float* q; const float* s; int64_t nq, ns; const int64_t* idx; int width;
    const float* x; int cin; const float* kp_q; const float* mod; int n_kp; float wscale, e2;
    float* wf; float* nnorm; hipStream_t st;
};

template <int VEC, bool WIDE, int INF, int AGG>
void launch_gather_deform(const DeformArgs& a) {
    const dim3 grid((unsigned)ceil_div(a.nq, kWavesD)), block(64 * kWavesD);
    if (a.n_kp <= 16)
        hipLaunchKernelGGL((kpconv_gather_deform_kernel<VEC, 16, WIDE, INF, AGG>), grid, block, 0,
                           a.st, a.q, a.s, a.nq, a.ns, a.idx, a.width, a.x, a.cin, a.kp_q, a.mod,
                           a.n_kp, a.wscale, a.e2, a.wf, a.nnorm);
    else
        hipLaunchKernelGGL((kpconv_gather_deform_kernel<VEC, kMaxKpD, WIDE, INF, AGG>), grid, block,
                           0, a.st, a.q, a.s, a.nq, a.ns, a.idx, a.width, a.x, a.cin, a.kp_q, a.mod,
                           a.n_kp, a.wscale, a.e2, a.wf, a.nnorm);
}

// the in-range threshold: extent^2 taken in double, rounded once (:325 compares fp32 distances
// with the Python float KP_extent ** 2)
inline float extent2(float extent) { return (float)((double)extent * (double)extent); }

inline bool deform_cin_ok(int cin) { return (cin >= 1 && cin <= 64) || cin == 128 || cin == 256; }

}  // namespace
}  // namespace fgr

using namespace fgr;

// the checks every entry point with a table shares; `name` is the entry point's own
#define FGR_DEFORM_CHECKS(name)                                                                   \
    FGR_REQUIRE(nq >= 0 && ns >= 0 && width >= 0, name ": bad sizes (nq %lld, ns %lld, width %d)", \
                (long long)nq, (long long)ns, width);                                             \
    FGR_REQUIRE(n_kp > 0 && n_kp <= kMaxKpD, name ": n_kp %d unsupported (need 1..32)", n_kp);    \
    FGR_REQUIRE(extent > 0.f, name ": extent %g is not positive", (double)extent);                \
    FGR_REQUIRE(kp_modes_ok(influence, aggregation),                                              \
                name ": unknown mode (influence %d, aggregation %d; need FGR_KP_* 0..2 and "      \
                     "FGR_AGG_* 0..1)", influence, aggregation);                                  \
    FGR_REQUIRE(deform_cin_ok(cin), name ": cin %d unsupported (need 1..64, 128 or 256)", cin)

extern "C" int fgr_kpconv_deform_points(const float* offset_raw, const float* offset_nnorm,
                                        const float* offset_bias, const float* kp, int64_t nq,
                                        int32_t n_kp, float extent, float* kp_q, float* mod,
                                        void* stream) {
    FGR_REQUIRE(nq >= 0 && nq * (int64_t)kMaxKpD < (1ll << 31),
                "fgr_kpconv_deform_points: bad sizes (nq %lld)", (long long)nq);
    FGR_REQUIRE(n_kp > 0 && n_kp <= kMaxKpD,
                "fgr_kpconv_deform_points: n_kp %d unsupported (need 1..32)", n_kp);
    FGR_REQUIRE(extent > 0.f, "fgr_kpconv_deform_points: extent %g is not positive", (double)extent);
    FGR_REQUIRE(nq == 0 || (offset_raw && offset_nnorm && offset_bias && kp && kp_q),
                "fgr_kpconv_deform_points: null pointer");
    if (nq == 0) return FGR_OK;
    hipStream_t st = as_stream(stream);
    TimedCall timed_(st);
    hipLaunchKernelGGL(deform_points_kernel, dim3((unsigned)ceil_div(nq * n_kp, 256)), dim3(256), 0,
                       st, offset_raw, offset_nnorm, offset_bias, kp, nq, n_kp, extent, kp_q, mod);
    FGR_CHECK_LAUNCH("deform_points_kernel");
    return FGR_OK;
}

extern "C" int fgr_kpconv_gather_deform_workspace(int64_t ns, int32_t cin, size_t* bytes) {
    FGR_REQUIRE(bytes && ns >= 0 && cin > 0, "fgr_kpconv_gather_deform_workspace: bad arguments");
    *bytes = 0;       // the in-range mask and the normaliser's positivity are taken inline
    return FGR_OK;
}

extern "C" int fgr_kpconv_gather_deform(const float* q, const float* s, int64_t nq, int64_t ns,
                                        const int64_t* idx, int32_t width, const float* x,
                                        int32_t cin, const float* kp_q, const float* mod,
                                        int32_t n_kp, float extent, int32_t influence,
                                        int32_t aggregation, float* wf, float* nnorm,
                                        void* workspace, size_t ws_bytes, void* stream) {
    (void)workspace; (void)ws_bytes;
    FGR_DEFORM_CHECKS("fgr_kpconv_gather_deform");
    FGR_REQUIRE(nq == 0 || (q && s && x && kp_q && wf && nnorm && (idx || width == 0)),
                "fgr_kpconv_gather_deform: null pointer");
    if (nq == 0) return FGR_OK;
    // 16-B row loads / stores at cin 256, 8-B at 128: torch allocations are 256-B aligned
    FGR_REQUIRE(cin < 128 || (((uintptr_t)x | (uintptr_t)wf) & 15) == 0,
                "fgr_kpconv_gather_deform: x / wf must be 16-B aligned at cin %d", cin);
    hipStream_t st = as_stream(stream);
    TimedCall timed_(st);
    const DeformArgs a{q, s, nq, ns, idx, width, x, cin, kp_q, mod, n_kp,
                       kp_wscale(influence, extent), extent2(extent), wf, nnorm, st};
    kp_with_modes(influence, aggregation, [&](auto inf, auto agg) {
        constexpr int INF = decltype(inf)::value, AGG = decltype(agg)::value;
        if (cin == 256) launch_gather_deform<4, true, INF, AGG>(a);
        else if (cin == 128) launch_gather_deform<2, true, INF, AGG>(a);
        else if (cin == 64) launch_gather_deform<1, true, INF, AGG>(a);
        else launch_gather_deform<1, false, INF, AGG>(a);
    });
    FGR_CHECK_LAUNCH("kpconv_gather_deform_kernel");
    return FGR_OK;
}

extern "C" int fgr_kpconv_scatter_deform_workspace(int64_t nq, int32_t width, int32_t cin,
                                                   size_t* bytes) {
    FGR_REQUIRE(bytes && nq >= 0 && width >= 0 && cin > 0,
                "fgr_kpconv_scatter_deform_workspace: bad arguments");
    *bytes = std::max<size_t>(1, (size_t)nq * width * cin * sizeof(float));
    return FGR_OK;
}

extern "C" int fgr_kpconv_scatter_deform(const float* q, const float* s, int64_t nq, int64_t ns,
                                         const int64_t* idx, int32_t width, const float* dwf,
                                         int32_t cin, const float* kp_q, const float* mod,
                                         int32_t n_kp, float extent, int32_t influence,
                                         int32_t aggregation, const int32_t* start,
                                         const int32_t* pos, float* dx, void* ws, size_t ws_bytes,
                                         void* stream) {
    FGR_DEFORM_CHECKS("fgr_kpconv_scatter_deform");
    if (ns == 0) return FGR_OK;
    FGR_REQUIRE(start && dx && ws, "fgr_kpconv_scatter_deform: null pointer");
    size_t need = 0;
    fgr_kpconv_scatter_deform_workspace(nq, width, cin, &need);
    FGR_REQUIRE(ws_bytes >= need, "fgr_kpconv_scatter_deform: workspace %zu < %zu bytes", ws_bytes, need);
    FGR_REQUIRE(nq == 0 || width == 0 || (q && s && idx && dwf && kp_q && pos),
                "fgr_kpconv_scatter_deform: null pointer");
    hipStream_t st = as_stream(stream);
    TimedCall timed_(st);
    float* g = (float*)ws;
    if (nq > 0 && width > 0) {
        const float wscale = kp_wscale(influence, extent), e2 = extent2(extent);
        kp_with_modes(influence, aggregation, [&](auto inf, auto agg) {
            hipLaunchKernelGGL((kpconv_scatter_deform_kernel<decltype(inf)::value, decltype(agg)::value>),
                               dim3((unsigned)ceil_div(nq, 4)), dim3(256), 0, st, q, s, nq, ns, idx,
                               width, dwf, cin, kp_q, mod, n_kp, wscale, e2, (const int*)pos, g);
        });
        FGR_CHECK_LAUNCH("kpconv_scatter_deform_kernel");
    }
    hipLaunchKernelGGL(deform_rowsum_kernel, dim3((unsigned)ceil_div(ns * cin, 256)), dim3(256), 0, st,
                       (const int*)start, ns, (const float*)g, cin, dx);
    FGR_CHECK_LAUNCH("deform_rowsum_kernel");
    return FGR_OK;
}

extern "C" int fgr_kpconv_deform_grad(const float* q, const float* s, int64_t nq, int64_t ns,
                                      const int64_t* idx, int32_t width, const float* x, int32_t cin,
                                      const float* dwf, const float* kp_q, const float* mod,
                                      int32_t n_kp, float extent, int32_t influence,
                                      int32_t aggregation, float* d_kp, float* d_mod, void* stream) {
    FGR_DEFORM_CHECKS("fgr_kpconv_deform_grad");
    FGR_REQUIRE(nq == 0 || (q && s && x && dwf && kp_q && d_kp && (idx || width == 0)),
                "fgr_kpconv_deform_grad: null pointer");
    if (nq == 0) return FGR_OK;
    hipStream_t st = as_stream(stream);
    TimedCall timed_(st);
    const float wscale = kp_wscale(influence, extent), e2 = extent2(extent);
    kp_with_modes(influence, aggregation, [&](auto inf, auto agg) {
        hipLaunchKernelGGL((kpconv_deform_grad_kernel<decltype(inf)::value, decltype(agg)::value>),
                           dim3((unsigned)ceil_div(nq, 4)), dim3(256), 0, st, q, s, nq, ns, idx, width,
                           x, cin, dwf, kp_q, mod, n_kp, wscale, e2, d_kp, d_mod);
    });
    FGR_CHECK_LAUNCH("kpconv_deform_grad_kernel");
    return FGR_OK;
}
