// Training backward of the forward's non-GEMM ops on gfx950 (train.py's
// `loss.backward()`, trainer.py:110-125). The dense products' backward (dX = dY W, dW = dY^T X)
// runs on the f16x3 / bf16 GEMMs with transposed weight images (fgreg/autograd.py); this file
// holds the rest:
//
//   fgr_nbr_inverse         the inverse (CSR) of a neighbour table: for every support row the
//                           (query, slot) entries naming it, in ascending entry order -- built
//                           once per table, shared by every scatter over that table
//   fgr_kpconv_scatter      KPConv gather-weight backward: dx[idx[q,h], c] += sum_k w(q,h,k)
//                           dwf[q,k,c] -- the scatter-add that the reference's
//                           `gather(method=2)` exists for (finegrained_kpconv_blocks.py:66-97)
//   fgr_max_pool_bwd        max_pool (:125-141): the gradient goes to the row's first max entry
//   fgr_corr_attention_bwd  CorrespondenceDecoder.simple_attention (finegrained_regtr.py:328-363)
//                           backward: dq, dk of softmax(q.k scale) xyz
//   fgr_layernorm_bwd       nn.LayerNorm backward (transformers.py:105-107) + gamma / beta grads
//   fgr_colsum              deterministic column sums (bias gradients)
// (the MHA core backward, fgr_attention_bwd, is attention_bwd.hip; the training segment norm
// has its own file too)
//
// Every reduction is deterministic: fixed-order partials (fp64 where they are long), merged in
// order, and no floating-point atomics anywhere. The two scatters (KPConv, max-pool) run as
// gathers over the table's inverse: each support row sums its own contributions in ascending
// (query, slot) order, so two backward passes give bit-identical gradients.
#include "mfma.h"

#include <algorithm>

namespace fgr {
namespace {

constexpr int kMaxKpT = 32;

// ---- inverse neighbour table ----------------------------------------------------------------
// Entry e = q * width + h of an (nq, width) table names support row idx[e] when 0 <= idx[e] < ns
// (the shadow index ns and negatives name none). The inverse lists, per support row s, the
// entries naming s in ascending e: start[s] .. start[s + 1] - 1 index ent[], and pos[e] is the
// CSR slot of entry e (-1 for a non-entry). count (int atomics: an exact count) -> one-block
// exclusive scan -> fill through per-row cursors (arbitrary order) -> per-row rank sort.
__global__ void __launch_bounds__(256)
nbr_count_kernel(const int64_t* __restrict__ idx, int64_t n_ent, int64_t ns, int* __restrict__ cnt) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_ent) return;
    const int64_t id = idx[e];
    if (id >= 0 && id < ns) atomicAdd(cnt + id, 1);
}

// One 1024-thread block: thread t scans a contiguous run of rows; cnt becomes the fill cursors.
__global__ void __launch_bounds__(1024)
nbr_scan_kernel(int* __restrict__ cnt, int64_t ns, int* __restrict__ start) {
    __shared__ int wtot[16];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int64_t per = (ns + 1023) / 1024;
    const int64_t b = min(ns, (int64_t)t * per), e = min(ns, b + per);
    int sum = 0;
    for (int64_t i = b; i < e; ++i) sum += cnt[i];
    int inc = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(inc, o, 64);
        if (lane >= o) inc += v;
    }
    if (lane == 63) wtot[w] = inc;
    __syncthreads();
    int base = inc - sum;
    for (int i = 0; i < w; ++i) base += wtot[i];
    for (int64_t i = b; i < e; ++i) {
        const int c = cnt[i];
        start[i] = base;
        cnt[i] = base;
        base += c;
    }
    if (t == 1023) start[ns] = base;
}

__global__ void __launch_bounds__(256)
nbr_fill_kernel(const int64_t* __restrict__ idx, int64_t n_ent, int64_t ns, int* __restrict__ cursor,
                int* __restrict__ tmp) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_ent) return;
    const int64_t id = idx[e];
    if (id >= 0 && id < ns) tmp[atomicAdd(cursor + id, 1)] = (int)e;
}

// One wave per support row: entry keys are unique, so each one's rank in the row is the count
// of smaller keys.
__global__ void __launch_bounds__(256)
nbr_sort_kernel(const int* __restrict__ start, int64_t ns, const int* __restrict__ tmp,
                int* __restrict__ ent, int* __restrict__ pos) {
    const int64_t s = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= ns) return;
    const int lane = threadIdx.x & 63;
    const int b = start[s], n = start[s + 1] - b;
    for (int j = lane; j < n; j += 64) {
        const int key = tmp[b + j];
        int rank = 0;
        for (int i = 0; i < n; ++i) rank += tmp[b + i] < key ? 1 : 0;
        ent[b + rank] = key;
        pos[key] = b + rank;
    }
}

// Segmented row sums over the inverse: dx[s, c] = sum_{j = start[s]}^{start[s+1]-1} g[j, c], in
// slot (= ascending entry) order; rows nobody names get 0.
__global__ void __launch_bounds__(256)
csr_rowsum_kernel(const int* __restrict__ start, int64_t ns, const float* __restrict__ g, int cin,
                  float* __restrict__ dx) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= ns * cin) return;
    const int64_t s = t / cin;
    const int c = (int)(t - s * cin);
    const int b = start[s], e = start[s + 1];
    float acc = 0.f;
    for (int j = b; j < e; ++j) acc += g[(int64_t)j * cin + c];
    dx[t] = acc;
}

// One wave per query: the valid neighbours of each 64-wide chunk are compacted by ballot and
// their K influences computed once into LDS (the forward gather's recipe, kpconv.hip); then for
// every 64-channel slice the query's dwf rows (K x 64) are held in registers and each valid
// neighbour's contribution sum_k w_hk dwf[q, k, c] is written to its CSR slot of the inverse
// (g[pos[q * width + h], c]); csr_rowsum_kernel then adds each support row's slots in order.
// INF / AGG: the forward's influence function and aggregation mode (FGR_KP_*, FGR_AGG_*).
template <int INF, int AGG>
__global__ void __launch_bounds__(256)
kpconv_scatter_rows_kernel(const float* __restrict__ q, const float* __restrict__ s, int64_t nq,
                           int64_t ns, const int64_t* __restrict__ idx, int width,
                           const float* __restrict__ dwf, int cin, const float* __restrict__ kp_g,
                           int n_kp, float wscale, const int* __restrict__ pos,
                           float* __restrict__ g) {
    __shared__ float w_lds[4][64][kMaxKpT + 1];
    __shared__ int slot_lds[4][64];
    __shared__ float kp[3 * kMaxKpT];
    const int wv = threadIdx.x / 64, lane = threadIdx.x % 64;
    for (int i = threadIdx.x; i < 3 * n_kp; i += blockDim.x) kp[i] = kp_g[i];
    __syncthreads();
    const int64_t qi = (int64_t)blockIdx.x * 4 + wv;
    if (qi >= nq) return;
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
            if constexpr (AGG == FGR_AGG_CLOSEST) {
                int bk;
                const float wb = kp_closest<INF>(nx, ny, nz, kp, n_kp, wscale, &bk);
                for (int k = 0; k < n_kp; ++k) w_lds[wv][p][k] = k == bk ? wb : 0.f;
            } else {
                for (int k = 0; k < n_kp; ++k)
                    w_lds[wv][p][k] = kp_weight<INF>(nx, ny, nz, kp, k, wscale);
            }
        }
        __builtin_amdgcn_wave_barrier();
        for (int c0 = 0; c0 < cin; c0 += 64) {
            const int c = c0 + lane;
            const bool act = c < cin;
            float dw[kMaxKpT];
#pragma unroll
            for (int k = 0; k < kMaxKpT; ++k)
                dw[k] = (act && k < n_kp) ? dq[(int64_t)k * cin + c] : 0.f;
            for (int hh = 0; hh < v; ++hh) {
                float acc = 0.f;
#pragma unroll
                for (int k = 0; k < kMaxKpT; ++k)
                    if (k < n_kp) acc = fmaf(w_lds[wv][hh][k], dw[k], acc);
                if (act) g[(int64_t)slot_lds[wv][hh] * cin + c] = acc;
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// Thread per (query, channel): the slot of the row's first maximum over x[idx[q, h], c] with
// shadow entries reading 0 (the appended zero row, finegrained_kpconv_blocks.py:134-140); -1
// when a shadow entry wins (its gradient goes nowhere).
__global__ void __launch_bounds__(256)
max_pool_argmax_kernel(const float* __restrict__ x, int64_t ns, int c, const int64_t* __restrict__ idx,
                       int64_t nq, int width, int* __restrict__ am) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= nq * c) return;
    const int64_t qi = t / c;
    const int ch = (int)(t - qi * c);
    const int64_t* row = idx + qi * width;
    int arg = -1;
    float best = 0.f;
    for (int h = 0; h < width; ++h) {
        const int64_t id = row[h];
        const bool real = id >= 0 && id < ns;
        const float v = real ? x[id * c + ch] : 0.f;
        if (h == 0 || v > best) {
            best = v;
            arg = real ? h : -1;
        }
    }
    am[t] = arg;
}

// Thread per (support row, channel): the gradients of every (query, slot) entry naming the row
// whose channel arg-max is that slot, in ascending entry order.
__global__ void __launch_bounds__(256)
max_pool_bwd_csr_kernel(const int* __restrict__ start, const int* __restrict__ ent, int64_t ns, int c,
                        int width, const int* __restrict__ am, const float* __restrict__ dy,
                        float* __restrict__ dx) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= ns * c) return;
    const int64_t s = t / c;
    const int ch = (int)(t - s * c);
    float acc = 0.f;
    for (int j = start[s]; j < start[s + 1]; ++j) {
        const int e = ent[j];
        const int64_t qi = e / width;
        const int h = e - (int)(qi * width);
        const int64_t qc = qi * c + ch;
        if (am[qc] == h) acc += dy[qc];
    }
    dx[t] = acc;
}

// ---- LayerNorm backward ------------------------------------------------------------------
// One wave per row (PER = d / 64 columns per lane), rows r = block * 64 + wave + 4 i; the
// wave's lanes keep the column partials of dy * xhat and dy over its rows, merged per block
// in LDS and written as the block's partial row (2 d floats) for fgr_colsum.
constexpr int kLnRowsWave = 4;                 // rows per wave, loaded together
constexpr int kLnRows = 4 * kLnRowsWave;       // rows per block (16: ~600 blocks at 9.5k rows)

template <int PER>
__global__ void __launch_bounds__(256)
layernorm_bwd_kernel(const float* __restrict__ x, int64_t n, int d, const float* __restrict__ g,
                     float eps, const float* __restrict__ dy, float* __restrict__ dx,
                     float* __restrict__ part) {
    const int wv = threadIdx.x / 64, lane = threadIdx.x % 64;
    float pg[PER], pb[PER], gm[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        pg[j] = pb[j] = 0.f;
        const int col = lane + 64 * j;
        gm[j] = col < d ? g[col] : 0.f;
    }
    // every load of the wave's rows first (one memory round trip), then the rows in turn
    float v[kLnRowsWave][PER], gy[kLnRowsWave][PER];
    const int64_t rb = (int64_t)blockIdx.x * kLnRows + wv * kLnRowsWave;
#pragma unroll
    for (int i = 0; i < kLnRowsWave; ++i) {
        const int64_t r = min(rb + i, n - 1);
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int col = min(lane + 64 * j, d - 1);
            v[i][j] = x[r * d + col];
            gy[i][j] = dy[r * d + col];
        }
    }
#pragma unroll
    for (int i = 0; i < kLnRowsWave; ++i) {
        const int64_t r = rb + i;
        if (r >= n) break;                         // wave-uniform
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < PER; ++j) s += (lane + 64 * j) < d ? v[i][j] : 0.f;
        const float mean = wave_sum(s) / (float)d;
        float sq = 0.f;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const float a = (lane + 64 * j) < d ? v[i][j] - mean : 0.f;
            sq += a * a;
        }
        const float rstd = 1.0f / sqrtf(wave_sum(sq) / (float)d + eps);
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int col = lane + 64 * j;
            if (col < d) {
                const float xh = (v[i][j] - mean) * rstd;
                const float dxh = gy[i][j] * gm[j];
                s1 += dxh;
                s2 += dxh * xh;
                pg[j] += gy[i][j] * xh;
                pb[j] += gy[i][j];
                v[i][j] = xh;
                gy[i][j] = dxh;
            }
        }
        const float m1 = wave_sum(s1) / (float)d, m2 = wave_sum(s2) / (float)d;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int col = lane + 64 * j;
            if (col < d) dx[r * d + col] = rstd * (gy[i][j] - m1 - v[i][j] * m2);
        }
    }
    __shared__ float lg[4][64 * PER], lb[4][64 * PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        lg[wv][lane + 64 * j] = pg[j];
        lb[wv][lane + 64 * j] = pb[j];
    }
    __syncthreads();
    for (int col = threadIdx.x; col < d; col += 256) {
        float* p = part + (int64_t)blockIdx.x * 2 * d;
        p[col] = ((lg[0][col] + lg[1][col]) + lg[2][col]) + lg[3][col];
        p[d + col] = ((lb[0][col] + lb[1][col]) + lb[2][col]) + lb[3][col];
    }
}

// ---- column sums -----------------------------------------------------------------------
constexpr int kColRows = 256;     // rows per partial: >= 4 blocks per CU on the tall inputs

__global__ void __launch_bounds__(256)
colsum_part_kernel(const float* __restrict__ x, int64_t n, int c, int64_t ldx, double* __restrict__ part) {
    const int ch = blockIdx.x * 64 + threadIdx.x % 64, rg = threadIdx.x / 64;
    const int64_t r0 = (int64_t)blockIdx.y * kColRows;
    double s = 0.0;
    if (ch < c) {
        const int64_t r1 = min(n, r0 + kColRows);
        double s1 = 0.0, s2 = 0.0, s3 = 0.0;       // four chains: the loads stay in flight
        int64_t r = r0 + rg;
        for (; r + 12 < r1; r += 16) {
            s += (double)x[r * ldx + ch];
            s1 += (double)x[(r + 4) * ldx + ch];
            s2 += (double)x[(r + 8) * ldx + ch];
            s3 += (double)x[(r + 12) * ldx + ch];
        }
        for (; r < r1; r += 4) s += (double)x[r * ldx + ch];
        s = (s + s1) + (s2 + s3);
    }
    __shared__ double l[4][64];
    l[rg][threadIdx.x % 64] = s;
    __syncthreads();
    if (rg == 0 && ch < c)
        part[(int64_t)blockIdx.y * c + ch] =
            ((l[0][threadIdx.x] + l[1][threadIdx.x]) + l[2][threadIdx.x]) + l[3][threadIdx.x];
}

__global__ void __launch_bounds__(256)
colsum_final_kernel(const double* __restrict__ part, int nparts, int c, float* __restrict__ out) {
    const int ch = blockIdx.x * 256 + threadIdx.x;
    if (ch >= c) return;
    double s = 0.0;
    for (int k = 0; k < nparts; ++k) s += part[(int64_t)k * c + ch];
    out[ch] = (float)s;
}

// ---- CorrespondenceDecoder.simple_attention backward ----------------------------------------
// corr[i] = sum_j P_ij v_j, P = softmax_j(s_ij), s_ij = scale q_i.k_j, v_j = the partner cloud's
// xyz (3 columns, no gradient). With D_i = dO_i . corr_i and dS_ij = P_ij (dO_i . v_j - D_i):
//   dq_i = scale sum_j dS_ij k_j,   dk_j = scale sum_i dS_ij q_i.
// The forward kernel's layout (attention.hip corr_attention_kernel): 32 rows x 8 lanes per
// block, each lane a D/8 slice of the dot products reduced over its 8 lanes with DPP, the other
// side's rows staged 32 at a time through LDS; fp32, no atomics (kernel 2 owns its key rows).
constexpr int kCbQ = 32;

__device__ __forceinline__ float sum8(float s) {
    s += dpp<0xB1>(s);
    s += dpp<0x4E>(s);
    s += dpp<0x141>(s);
    return s;
}

struct CorrBwd {
    const float* q; int64_t ld_q;
    const float* k; int64_t ld_k;
    const float* xyz;
    const float* dout;
    float* dq; int64_t ld_dq;
    float* dk; int64_t ld_dk;
    const int64_t* q_off;
    const int64_t* kv_off;
    const int32_t* kv_seg;
    const int64_t* v_off;
    int n_seg;
    float scale;
    float* lse;
    float* dsum;
};

template <int D>
__global__ void __launch_bounds__(256)
corr_attn_bwd_dq_kernel(CorrBwd a) {
    constexpr int DL = D / 8;
    __shared__ float kt[kCbQ][D + 4];
    __shared__ float vt[kCbQ][3];
    const int seg = blockIdx.y;
    const int64_t qb = a.q_off[seg], qe = a.q_off[seg + 1];
    const int64_t q0 = qb + (int64_t)blockIdx.x * kCbQ;
    if (q0 >= qe) return;                                  // block-uniform
    const int ks = a.kv_seg[seg];
    const int64_t kb = a.kv_off[ks], ke = a.kv_off[ks + 1];
    const int64_t vb = a.v_off[ks];
    const int tid = threadIdx.x, qi = tid >> 3, sl = tid & 7;
    const int64_t row = q0 + qi;
    const bool active = row < qe;
    float qv[DL], dqv[DL];
#pragma unroll
    for (int e = 0; e < DL; ++e) {
        qv[e] = active ? a.q[row * a.ld_q + sl * DL + e] * a.scale : 0.f;
        dqv[e] = 0.f;
    }
    const float d0 = active ? a.dout[row * 3] : 0.f, d1 = active ? a.dout[row * 3 + 1] : 0.f,
                d2 = active ? a.dout[row * 3 + 2] : 0.f;
    float m = -INFINITY, l = 0.f, a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int pass = 0; pass < 2; ++pass) {
        float inv_l = 0.f, dsum = 0.f;
        if (pass == 1) {
            inv_l = 1.0f / l;
            dsum = d0 * (a0 * inv_l) + d1 * (a1 * inv_l) + d2 * (a2 * inv_l);   // dO . corr
        }
        for (int64_t j0 = kb; j0 < ke; j0 += kCbQ) {
            const int nk = (int)min((int64_t)kCbQ, ke - j0);
            __syncthreads();
            for (int e = tid; e < kCbQ * D; e += 256) {
                const int r = e / D, cc = e - r * D;
                kt[r][cc] = r < nk ? a.k[(j0 + r) * a.ld_k + cc] : 0.f;
            }
            if (tid < kCbQ * 3) {
                const int r = tid / 3, cc = tid - r * 3;
                vt[r][cc] = r < nk ? a.xyz[(vb + (j0 - kb) + r) * 3 + cc] : 0.f;
            }
            __syncthreads();
            for (int r = 0; r < nk; ++r) {
                float s = 0.f;
#pragma unroll
                for (int e = 0; e < DL; ++e) s = fmaf(qv[e], kt[r][sl * DL + e], s);
                s = sum8(s);
                if (pass == 0) {                           // the forward's online softmax
                    if (s > m) {
                        const float f = __expf(m - s);
                        l *= f; a0 *= f; a1 *= f; a2 *= f;
                        m = s;
                    }
                    const float p = __expf(s - m);
                    l += p;
                    a0 = fmaf(p, vt[r][0], a0);
                    a1 = fmaf(p, vt[r][1], a1);
                    a2 = fmaf(p, vt[r][2], a2);
                } else {
                    const float p = __expf(s - m) * inv_l;
                    const float dp = d0 * vt[r][0] + d1 * vt[r][1] + d2 * vt[r][2];
                    const float ds = p * (dp - dsum);
#pragma unroll
                    for (int e = 0; e < DL; ++e) dqv[e] = fmaf(ds, kt[r][sl * DL + e], dqv[e]);
                }
            }
        }
        if (pass == 1 && active) {
#pragma unroll
            for (int e = 0; e < DL; ++e) a.dq[row * a.ld_dq + sl * DL + e] = dqv[e] * a.scale;
            if (sl == 0) {
                a.lse[row] = m + logf(l);
                a.dsum[row] = dsum;
            }
        }
    }
}

template <int D>
__global__ void __launch_bounds__(256)
corr_attn_bwd_dk_kernel(CorrBwd a) {
    constexpr int DL = D / 8;
    __shared__ float qt[kCbQ][D + 4];
    __shared__ float dt[kCbQ][5];                          // dO (3), lse, D of each staged query
    const int ks = blockIdx.y;
    const int64_t kb = a.kv_off[ks], ke = a.kv_off[ks + 1];
    const int64_t k0 = kb + (int64_t)blockIdx.x * kCbQ;
    if (k0 >= ke) return;                                  // block-uniform
    const int tid = threadIdx.x, ki = tid >> 3, sl = tid & 7;
    const int64_t row = k0 + ki;
    const bool active = row < ke;
    float kv[DL], dkv[DL];
#pragma unroll
    for (int e = 0; e < DL; ++e) {
        kv[e] = active ? a.k[row * a.ld_k + sl * DL + e] : 0.f;
        dkv[e] = 0.f;
    }
    for (int seg = 0; seg < a.n_seg; ++seg) {
        if (a.kv_seg[seg] != ks) continue;
        const int64_t vb = a.v_off[ks] + (row - kb);
        const float v0 = active ? a.xyz[vb * 3] : 0.f, v1 = active ? a.xyz[vb * 3 + 1] : 0.f,
                    v2 = active ? a.xyz[vb * 3 + 2] : 0.f;
        const int64_t qb = a.q_off[seg], qe = a.q_off[seg + 1];
        for (int64_t i0 = qb; i0 < qe; i0 += kCbQ) {
            const int nq = (int)min((int64_t)kCbQ, qe - i0);
            __syncthreads();
            for (int e = tid; e < kCbQ * D; e += 256) {
                const int r = e / D, cc = e - r * D;
                qt[r][cc] = r < nq ? a.q[(i0 + r) * a.ld_q + cc] * a.scale : 0.f;
            }
            if (tid < kCbQ) {
                const bool ok = tid < nq;
                const int64_t r = i0 + tid;
                dt[tid][0] = ok ? a.dout[r * 3] : 0.f;
                dt[tid][1] = ok ? a.dout[r * 3 + 1] : 0.f;
                dt[tid][2] = ok ? a.dout[r * 3 + 2] : 0.f;
                dt[tid][3] = ok ? a.lse[r] : 0.f;
                dt[tid][4] = ok ? a.dsum[r] : 0.f;
            }
            __syncthreads();
            for (int r = 0; r < nq; ++r) {
                float s = 0.f;
#pragma unroll
                for (int e = 0; e < DL; ++e) s = fmaf(qt[r][sl * DL + e], kv[e], s);
                s = sum8(s);
                const float p = __expf(s - dt[r][3]);
                const float dp = dt[r][0] * v0 + dt[r][1] * v1 + dt[r][2] * v2;
                const float ds = p * (dp - dt[r][4]);
#pragma unroll
                for (int e = 0; e < DL; ++e) dkv[e] = fmaf(ds, qt[r][sl * DL + e], dkv[e]);   // qt = scale q
            }
        }
    }
    if (!active) return;
#pragma unroll
    for (int e = 0; e < DL; ++e) a.dk[row * a.ld_dk + sl * DL + e] = dkv[e];
}

}  // namespace
}  // namespace fgr

using namespace fgr;

extern "C" int fgr_nbr_inverse_workspace(int64_t nq, int32_t width, int64_t ns, size_t* bytes) {
    FGR_REQUIRE(bytes && nq >= 0 && width >= 0 && ns >= 0 && nq * (int64_t)width < (1ll << 31),
                "fgr_nbr_inverse_workspace: bad arguments");
    *bytes = (size_t)(ns + 1) * sizeof(int) + (size_t)nq * width * sizeof(int);
    return FGR_OK;
}

extern "C" int fgr_nbr_inverse(const int64_t* idx, int64_t nq, int32_t width, int64_t ns, int32_t* start,
                               int32_t* pos, int32_t* ent, void* ws, size_t ws_bytes, void* stream) {
    FGR_REQUIRE(nq >= 0 && width >= 0 && ns >= 0 && nq * (int64_t)width < (1ll << 31),
                "fgr_nbr_inverse: bad arguments");
    FGR_REQUIRE(start && pos && ent && ws && (nq * width == 0 || idx), "fgr_nbr_inverse: null pointer");
    size_t need = 0;
    fgr_nbr_inverse_workspace(nq, width, ns, &need);
    FGR_REQUIRE(ws_bytes >= need, "fgr_nbr_inverse: workspace %zu < %zu bytes", ws_bytes, need);
    hipStream_t st = as_stream(stream);
    const int64_t n_ent = nq * (int64_t)width;
    int* cnt = (int*)ws;
    int* tmp = cnt + (ns + 1);
    FGR_CHECK_HIP(hipMemsetAsync(cnt, 0, (size_t)(ns + 1) * sizeof(int), st));
    if (n_ent > 0)
        FGR_CHECK_HIP(hipMemsetAsync(pos, 0xFF, (size_t)n_ent * sizeof(int), st));
    const unsigned eb = (unsigned)std::max<int64_t>(1, ceil_div(n_ent, 256));
    if (n_ent > 0) {
        hipLaunchKernelGGL(nbr_count_kernel, dim3(eb), dim3(256), 0, st, idx, n_ent, ns, cnt);
        FGR_CHECK_LAUNCH("nbr_count_kernel");
    }
    hipLaunchKernelGGL(nbr_scan_kernel, dim3(1), dim3(1024), 0, st, cnt, ns, start);
    FGR_CHECK_LAUNCH("nbr_scan_kernel");
    if (n_ent == 0 || ns == 0) return FGR_OK;
    hipLaunchKernelGGL(nbr_fill_kernel, dim3(eb), dim3(256), 0, st, idx, n_ent, ns, cnt, tmp);
    FGR_CHECK_LAUNCH("nbr_fill_kernel");
    hipLaunchKernelGGL(nbr_sort_kernel, dim3((unsigned)ceil_div(ns, 4)), dim3(256), 0, st, start, ns,
                       (const int*)tmp, ent, pos);
    FGR_CHECK_LAUNCH("nbr_sort_kernel");
    return FGR_OK;
}

extern "C" int fgr_kpconv_scatter_workspace(int64_t nq, int32_t width, int32_t cin, size_t* bytes) {
    FGR_REQUIRE(bytes && nq >= 0 && width >= 0 && cin > 0, "fgr_kpconv_scatter_workspace: bad arguments");
    *bytes = std::max<size_t>(1, (size_t)nq * width * cin * sizeof(float));
    return FGR_OK;
}

extern "C" int fgr_kpconv_scatter_mode(const float* q, const float* s, int64_t nq, int64_t ns,
                                       const int64_t* idx, int32_t width, const float* dwf,
                                       int32_t cin, const float* kernel_points, int32_t n_kp,
                                       float extent, int32_t influence, int32_t aggregation,
                                       const int32_t* start, const int32_t* pos, float* dx,
                                       void* ws, size_t ws_bytes, void* stream) {
    FGR_REQUIRE(nq >= 0 && ns >= 0 && width >= 0 && cin > 0 && n_kp > 0 && n_kp <= kMaxKpT &&
                    extent > 0.f, "fgr_kpconv_scatter: bad arguments");
    FGR_REQUIRE(kp_modes_ok(influence, aggregation),
                "fgr_kpconv_scatter_mode: unknown mode (influence %d, aggregation %d; need "
                "FGR_KP_* 0..2 and FGR_AGG_* 0..1)", influence, aggregation);
    if (ns == 0) return FGR_OK;
    FGR_REQUIRE(start && dx && ws, "fgr_kpconv_scatter: null pointer");
    size_t need = 0;
    fgr_kpconv_scatter_workspace(nq, width, cin, &need);
    FGR_REQUIRE(ws_bytes >= need, "fgr_kpconv_scatter: workspace %zu < %zu bytes", ws_bytes, need);
    hipStream_t st = as_stream(stream);
    float* g = (float*)ws;
    if (nq > 0 && width > 0) {
        FGR_REQUIRE(q && s && idx && dwf && kernel_points && pos, "fgr_kpconv_scatter: null pointer");
        const float wscale = kp_wscale(influence, extent);
        kp_with_modes(influence, aggregation, [&](auto inf, auto agg) {
            hipLaunchKernelGGL((kpconv_scatter_rows_kernel<decltype(inf)::value, decltype(agg)::value>),
                               dim3((unsigned)ceil_div(nq, 4)), dim3(256), 0, st, q, s, nq, ns, idx,
                               width, dwf, cin, kernel_points, n_kp, wscale, (const int*)pos, g);
        });
        FGR_CHECK_LAUNCH("kpconv_scatter_rows_kernel");
    }
    hipLaunchKernelGGL(csr_rowsum_kernel, dim3((unsigned)ceil_div(ns * cin, 256)), dim3(256), 0, st,
                       (const int*)start, ns, (const float*)g, cin, dx);
    FGR_CHECK_LAUNCH("csr_rowsum_kernel");
    return FGR_OK;
}

extern "C" int fgr_kpconv_scatter(const float* q, const float* s, int64_t nq, int64_t ns,
                                  const int64_t* idx, int32_t width, const float* dwf, int32_t cin,
                                  const float* kernel_points, int32_t n_kp, float extent,
                                  const int32_t* start, const int32_t* pos, float* dx, void* ws,
                                  size_t ws_bytes, void* stream) {
    return fgr_kpconv_scatter_mode(q, s, nq, ns, idx, width, dwf, cin, kernel_points, n_kp, extent,
                                   FGR_KP_LINEAR, FGR_AGG_SUM, start, pos, dx, ws, ws_bytes, stream);
}

extern "C" int fgr_max_pool_bwd_workspace(int64_t nq, int32_t c, size_t* bytes) {
    FGR_REQUIRE(bytes && nq >= 0 && c > 0, "fgr_max_pool_bwd_workspace: bad arguments");
    *bytes = std::max<size_t>(1, (size_t)nq * c * sizeof(int));
    return FGR_OK;
}

extern "C" int fgr_max_pool_bwd(const float* x, int64_t ns, int32_t c, const int64_t* idx, int64_t nq,
                                int32_t width, const float* dy, const int32_t* start,
                                const int32_t* ent, float* dx, void* ws, size_t ws_bytes,
                                void* stream) {
    FGR_REQUIRE(ns >= 0 && nq >= 0 && c > 0 && width > 0, "fgr_max_pool_bwd: bad arguments");
    if (ns == 0) return FGR_OK;
    FGR_REQUIRE(start && ent && dx && ws && (nq == 0 || (x && idx && dy)), "fgr_max_pool_bwd: null pointer");
    size_t need = 0;
    fgr_max_pool_bwd_workspace(nq, c, &need);
    FGR_REQUIRE(ws_bytes >= need, "fgr_max_pool_bwd: workspace %zu < %zu bytes", ws_bytes, need);
    hipStream_t st = as_stream(stream);
    int* am = (int*)ws;
    if (nq > 0) {
        hipLaunchKernelGGL(max_pool_argmax_kernel, dim3((unsigned)ceil_div(nq * c, 256)), dim3(256), 0, st,
                           x, ns, c, idx, nq, width, am);
        FGR_CHECK_LAUNCH("max_pool_argmax_kernel");
    }
    hipLaunchKernelGGL(max_pool_bwd_csr_kernel, dim3((unsigned)ceil_div(ns * c, 256)), dim3(256), 0, st,
                       (const int*)start, (const int*)ent, ns, c, width, (const int*)am, dy, dx);
    FGR_CHECK_LAUNCH("max_pool_bwd_csr_kernel");
    return FGR_OK;
}

extern "C" int fgr_corr_attention_bwd_workspace(int64_t n_rows, size_t* bytes) {
    FGR_REQUIRE(bytes && n_rows >= 0, "fgr_corr_attention_bwd_workspace: bad arguments");
    *bytes = (size_t)std::max<int64_t>(n_rows, 1) * 2 * sizeof(float);
    return FGR_OK;
}

extern "C" int fgr_corr_attention_bwd(const float* q, int64_t ld_q, const float* k, int64_t ld_k,
                                      const float* xyz, const float* dout, float* dq, int64_t ld_dq,
                                      float* dk, int64_t ld_dk, const int64_t* q_off,
                                      const int64_t* kv_off, const int32_t* kv_seg,
                                      const int64_t* v_off, int32_t n_seg, int32_t n_kv_seg,
                                      int64_t n_rows, int32_t max_q_len, int32_t max_kv_len, int32_t d,
                                      float scale, void* ws, size_t ws_bytes, void* stream) {
    FGR_REQUIRE(n_seg > 0 && n_kv_seg > 0 && n_rows >= 0 && max_q_len >= 0 && max_kv_len >= 0 &&
                    ld_q >= d && ld_k >= d && ld_dq >= d && ld_dk >= d,
                "fgr_corr_attention_bwd: bad arguments");
    FGR_REQUIRE(d == 32 || d == 64 || d == 128 || d == 256 || d == 512,
                "fgr_corr_attention_bwd: d %d unsupported (32, 64, 128, 256, 512)", d);
    FGR_REQUIRE(q && k && xyz && dout && dq && dk && q_off && kv_off && kv_seg && v_off && ws,
                "fgr_corr_attention_bwd: null pointer");
    size_t need = 0;
    fgr_corr_attention_bwd_workspace(n_rows, &need);
    FGR_REQUIRE(ws_bytes >= need, "fgr_corr_attention_bwd: workspace %zu < %zu bytes", ws_bytes, need);
    const int64_t nr = std::max<int64_t>(n_rows, 1);
    CorrBwd a{q, ld_q, k, ld_k, xyz, dout, dq, ld_dq, dk, ld_dk, q_off, kv_off, kv_seg, v_off, n_seg,
              scale, (float*)ws, (float*)ws + nr};
    hipStream_t st = as_stream(stream);
    const dim3 g1((unsigned)std::max<int64_t>(1, ceil_div(max_q_len, kCbQ)), (unsigned)n_seg);
    const dim3 g2((unsigned)std::max<int64_t>(1, ceil_div(max_kv_len, kCbQ)), (unsigned)n_kv_seg);
    switch (d) {
#define CAB(DD) case DD: \
        hipLaunchKernelGGL(corr_attn_bwd_dq_kernel<DD>, g1, dim3(256), 0, st, a); \
        FGR_CHECK_LAUNCH("corr_attn_bwd_dq_kernel"); \
        hipLaunchKernelGGL(corr_attn_bwd_dk_kernel<DD>, g2, dim3(256), 0, st, a); \
        break;
        CAB(32) CAB(64) CAB(128) CAB(256) CAB(512)
#undef CAB
    }
    FGR_CHECK_LAUNCH("corr_attn_bwd_dk_kernel");
    return FGR_OK;
}

extern "C" int fgr_colsum_workspace(int64_t n, int32_t c, size_t* bytes) {
    FGR_REQUIRE(bytes && n >= 0 && c > 0, "fgr_colsum_workspace: bad arguments");
    *bytes = (size_t)std::max<int64_t>(1, ceil_div(n, kColRows)) * c * sizeof(double);
    return FGR_OK;
}

extern "C" int fgr_colsum(const float* x, int64_t n, int32_t c, int64_t ldx, float* out, void* ws,
                          size_t ws_bytes, void* stream) {
    FGR_REQUIRE(n >= 0 && c > 0 && ldx >= c, "fgr_colsum: bad arguments");
    FGR_REQUIRE(out && ws && (n == 0 || x), "fgr_colsum: null pointer");
    size_t need = 0;
    fgr_colsum_workspace(n, c, &need);
    FGR_REQUIRE(ws_bytes >= need, "fgr_colsum: workspace too small");
    const int nparts = (int)std::max<int64_t>(1, ceil_div(n, kColRows));
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(colsum_part_kernel, dim3((unsigned)ceil_div(c, 64), nparts), dim3(256), 0, st, x, n,
                       c, ldx, (double*)ws);
    FGR_CHECK_LAUNCH("colsum_part_kernel");
    hipLaunchKernelGGL(colsum_final_kernel, dim3((unsigned)ceil_div(c, 256)), dim3(256), 0, st,
                       (const double*)ws, nparts, c, out);
    FGR_CHECK_LAUNCH("colsum_final_kernel");
    return FGR_OK;
}

extern "C" int fgr_layernorm_bwd_workspace(int64_t n, int32_t d, size_t* bytes) {
    FGR_REQUIRE(bytes && n >= 0 && d > 0, "fgr_layernorm_bwd_workspace: bad arguments");
    const int64_t nb = std::max<int64_t>(1, ceil_div(n, kLnRows));
    size_t cs = 0;
    fgr_colsum_workspace(nb, 2 * d, &cs);
    *bytes = (size_t)nb * 2 * d * sizeof(float) + cs;
    return FGR_OK;
}

extern "C" int fgr_layernorm_bwd(const float* x, int64_t n, int32_t d, const float* gamma, float eps,
                                 const float* dy, float* dx, float* dgamma_dbeta, void* ws,
                                 size_t ws_bytes, void* stream) {
    FGR_REQUIRE(n >= 0 && d > 0 && d <= 1024, "fgr_layernorm_bwd: bad arguments (0 < d <= 1024)");
    FGR_REQUIRE(gamma && dgamma_dbeta && ws && (n == 0 || (x && dy && dx)), "fgr_layernorm_bwd: null pointer");
    size_t need = 0;
    fgr_layernorm_bwd_workspace(n, d, &need);
    FGR_REQUIRE(ws_bytes >= need, "fgr_layernorm_bwd: workspace too small");
    const int64_t nb = std::max<int64_t>(1, ceil_div(n, kLnRows));
    float* part = (float*)ws;
    void* cws = (char*)ws + (size_t)nb * 2 * d * sizeof(float);
    size_t cs = 0;
    fgr_colsum_workspace(nb, 2 * d, &cs);
    hipStream_t st = as_stream(stream);
    if (n == 0) {
        FGR_CHECK_HIP(hipMemsetAsync(part, 0, (size_t)2 * d * sizeof(float), st));
    } else {
        int per = 1;
        while (64 * per < d) per *= 2;
        switch (per) {
#define LNB(P) case P: hipLaunchKernelGGL(layernorm_bwd_kernel<P>, dim3((unsigned)nb), dim3(256), 0, st, x, n, d, gamma, eps, dy, dx, part); break;
            LNB(1) LNB(2) LNB(4) LNB(8) LNB(16)
#undef LNB
            default: FGR_REQUIRE(false, "fgr_layernorm_bwd: unsupported d");
        }
        FGR_CHECK_LAUNCH("layernorm_bwd_kernel");
    }
    return fgr_colsum(part, nb, 2 * d, 2 * d, dgamma_dbeta, cws, cs, stream);
}
