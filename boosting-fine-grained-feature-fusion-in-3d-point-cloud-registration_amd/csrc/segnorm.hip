// Training segment norm on gfx950: per-(segment, channel) normalisation
// with batch statistics, forward and backward -- the InstanceNorm of BatchNormBlock
// (finegrained_kpconv_blocks.py:462-518, segment = cloud) and the Res2Net BatchNorm1d in train()
// (res2net.py:126-159, one segment, affine):
//
//   z = (v - mean) * rstd (* gamma + beta), v = x / row_div;  a = act(z);  y = post(a + residual)
//
//   fgr_segnorm_stats   mean / rstd / biased var: partial sums per (segment, chunk of kRowsChunk
//                       rows, channel), then their merge
//   fgr_segnorm_apply   y from x and the statistics
//   fgr_segnorm_fwd     both; where it can, with the merge inside the apply pass
//   fgr_segnorm_bwd     dx, dres, dgamma / dbeta from (y, dy): the same two passes
//
// Each formula stands once: the element functions (seg_fwd_elem, seg_bwd_elem), the merges of the
// chunk partials (seg_merge_fwd, seg_merge_bwd, seg_merge_affine_grads), the four-rows-in-flight
// row loop (seg_rows4) and the channel loads (ldc). The kernels are templated on the channel
// vector width V: 1, or 4 (one float4 per thread) for c % 4 == 0 and 16-B aligned pointers.
// Every reduction is deterministic: fp64 partials in a fixed layout, merged in a fixed order.
#include "mfma.h"

#include <algorithm>
#include <cstdlib>
#include <initializer_list>

namespace fgr {
namespace {

// Partial sums per (segment, chunk of kRowsChunk rows, channel), in fp64 and shifted by the
// segment's first row (no cancellation for |mean| >> std), merged in chunk order.
constexpr int kRowsChunk = 256;
constexpr int kSegLds = 64;        // segment tables up to this many segments cached in LDS
// The merges folded into the apply passes (segments of at most kSegFuseChunksMax chunks, e.g.
// ModelNet's per-cloud InstanceNorms): one launch per norm and direction instead of two.
constexpr int kSegFuseChunks = 16;          // up to here the merge order of the merge kernels
constexpr int kSegFuseChunksMax = 64;       // beyond: the separate merge kernels

// The value of norm.hip's act_fn, tested in the other order. The two stay apart: the compiler
// emits different (equivalent) code for the two orders, in either file's kernels.
__device__ __forceinline__ float act_fwd(float z, int act) {
    if (act == FGR_ACT_RELU) return fmaxf(z, 0.f);
    if (act == FGR_ACT_LEAKY) return z > 0.f ? z : 0.1f * z;
    return z;
}
// derivative factor from the activation's INPUT sign (torch: relu' = (out > 0), leaky' =
// (in > 0 ? 1 : slope); out and in share their sign for both)
__device__ __forceinline__ float act_grad(float zin, int act) {
    if (act == FGR_ACT_RELU) return zin > 0.f ? 1.f : 0.f;
    if (act == FGR_ACT_LEAKY) return zin > 0.f ? 1.f : 0.1f;
    return 1.f;
}

struct SegArgs {
    const float* x;
    const float* row_div;
    const int64_t* seg_off;
    int n_seg;
    int c;
    int n_chunks;
};

// In the backward, residual is y where the forward had a residual (NULL where not): the
// backward needs post'(y), never the residual's values.
struct SegApply {
    SegArgs a;
    int64_t n;
    const float* mean;
    const float* rstd;
    const float* gamma;
    const float* beta;
    int act;
    const float* residual;
    int post_act;
};

// ---- channel vectors: V consecutive channels of one row, a float (V = 1) or a float4 (V = 4)
template <int V>
struct Chan {
    float v[V];
};

template <int V>
__device__ __forceinline__ Chan<V> ldc(const float* p) {
    if constexpr (V == 4) {
        const float4 q = ld4(p);
        return {{q.x, q.y, q.z, q.w}};
    } else {
        return {{*p}};
    }
}

template <int V>
__device__ __forceinline__ void stc(float* p, const Chan<V>& c) {
    if constexpr (V == 4)
        *reinterpret_cast<float4*>(p) = make_float4(c.v[0], c.v[1], c.v[2], c.v[3]);
    else
        *p = c.v[0];
}

template <int V>
__device__ __forceinline__ Chan<V> fillc(float f) {
    Chan<V> c;
#pragma unroll
    for (int j = 0; j < V; ++j) c.v[j] = f;
    return c;
}

// gamma, beta of channels ch .. ch + V - 1; (1, 0) without affine
template <int V>
__device__ __forceinline__ void ld_affine(const SegApply& p, int ch, Chan<V>& g, Chan<V>& b) {
    g = fillc<V>(1.f);
    b = fillc<V>(0.f);
    if (p.gamma) {
        g = ldc<V>(p.gamma + ch);
        b = ldc<V>(p.beta + ch);
    }
}

// ---- the element formulas ---------------------------------------------------------------
// y = post(act((x / rd - mean) * rstd * gamma + beta) + residual); rd, g, b, res are read only
// where p has the row divisor, the affine, the residual.
__device__ __forceinline__ float seg_fwd_elem(const SegApply& p, float x, float rd, float mu, float rs,
                                              float g, float b, float res) {
    const float v = p.a.row_div ? x / rd : x;
    float z = (v - mu) * rs;
    if (p.gamma) z = z * g + b;
    float y = act_fwd(z, p.act);
    if (p.residual) y = act_fwd(y + res, p.post_act);
    return y;
}

// gr * ag - m1 - xh * m2 (gr * ag = dz), its roundings pinned: left to itself the compiler
// contracts this expression differently from kernel to kernel. V = 4 fuses both products into
// the subtractions (dz is not rounded first), V = 1 rounds each product: what the float4 and
// the scalar kernels have computed from the start. The two differ in dx's last bit.
template <int V>
__device__ __forceinline__ float seg_dz_centred(float gr, float ag, float m1, float xh, float m2) {
    if constexpr (V == 4) {
        return fmaf(-xh, m2, fmaf(gr, ag, -m1));
    } else {
#pragma clang fp contract(off)
        return gr * ag - m1 - xh * m2;
    }
}

// gr = dy * post'(y) (= dres), dz = gr * act'(z), xh = xhat; with DX also
// dx = rstd * gamma * (dz - mean(dz) - xhat * mean(dz xhat)) / rd, from the segment's sums
// s1 = sum dz, s2 = sum dz xhat and inv_n = 1 / rows. The statistics pass (DX = false) divides
// by rd only where there is a row divisor, the apply pass by rd = 1 without one: x / 1.0f is
// exact, so the two agree in every bit.
struct SegGrad {
    float gr, dz, xh, dx;
};

template <bool DX, int V = 4>
__device__ __forceinline__ SegGrad seg_bwd_elem(const SegApply& p, float x, float rd, float mu, float rs,
                                                float g, float b, float dy, float y, float s1 = 0.f,
                                                float s2 = 0.f, float inv_n = 0.f) {
    SegGrad e;
    const float v = DX || p.a.row_div ? x / rd : x;
    e.xh = (v - mu) * rs;
    e.gr = dy;
    if (p.residual) e.gr *= act_grad(y, p.post_act);
    const float ag = act_grad(e.xh * g + b, p.act);
    e.dz = e.gr * ag;
    e.dx = 0.f;
    if constexpr (DX) e.dx = rs * g * seg_dz_centred<V>(e.gr, ag, s1 * inv_n, e.xh, s2 * inv_n) / rd;
    return e;
}

// ---- the row loop of the chunk-grid kernels -------------------------------------------------
// One row's V channels of x, of the arrays pa and pb (dy and y, or the residual) and its divisor.
template <int V>
struct SegRow {
    Chan<V> x, a, b;
    float rd;
};

// Rows r, r + G, r + 2 G, ... below r1 (G = 4 V row groups per block), channels ch .. ch + V - 1,
// four rows in flight per thread: every load of the four rows first (clamped to the chunk's
// last row, so that they need no branch), then use(row, its values) for those inside the chunk,
// in row order. (One dependent load per row and channel cost 22 / 38 us per ModelNet call in the
// statistics passes.) HAS_A: pa is read; has_b: pb is read (zeros otherwise).
template <int V, bool HAS_A, class F>
__device__ __forceinline__ void seg_rows4(const SegArgs& s, const float* __restrict__ pa,
                                          const float* __restrict__ pb, bool has_b, int ch, int64_t r,
                                          int64_t r1, F&& use) {
    constexpr int G = 4 * V;
    for (; r < r1; r += 4 * G) {
        SegRow<V> w[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t rr = min(r + G * u, r1 - 1);
            const int64_t o = rr * s.c + ch;
            w[u].x = ldc<V>(s.x + o);
            w[u].a = fillc<V>(0.f);
            if constexpr (HAS_A) w[u].a = ldc<V>(pa + o);
            w[u].b = has_b ? ldc<V>(pb + o) : fillc<V>(0.f);
            w[u].rd = s.row_div ? s.row_div[rr] : 1.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (r + G * u >= r1) break;
            use(r + G * u, w[u]);
        }
    }
}

// ---- statistics: partial sums per (segment, chunk, channel) --------------------------------
// One block per (chunk, segment, 64 channels): 64 / V channel lanes x 4 V row groups; row group
// rg takes the chunk's rows rg, rg + 4 V, ... and the block adds its row groups' sums in LDS.
//
// V = 1 is bit-identical to a plain scalar loop "for (r = r0 + rg; r < r1; r += 4)": each
// thread visits rows rg, rg + 4, rg + 8, ... in that order (seg_rows4 loads four of them ahead
// and uses them in order), and the four row groups are added in index order starting from +0.0
// (a running sum that started at +0.0 is never -0.0, so 0.0 + l[0] = l[0]).
template <int V>
__global__ void __launch_bounds__(256)
segnorm_stats_kernel(SegArgs a, double* __restrict__ part) {
    constexpr int L = 64 / V, G = 4 * V;
    const int seg = blockIdx.y, chunk = blockIdx.x;
    const int cl = threadIdx.x % L, rg = threadIdx.x / L;
    const int ch = blockIdx.z * 64 + V * cl;
    const int C = a.c;
    const int64_t b = a.seg_off[seg], e = a.seg_off[seg + 1];
    const int64_t r0 = b + (int64_t)chunk * kRowsChunk;
    double s1[V], s2[V];
#pragma unroll
    for (int j = 0; j < V; ++j) s1[j] = s2[j] = 0.0;
    int cnt = 0;
    if (ch < C && r0 < e) {
        const Chan<V> pv = ldc<V>(a.x + b * C + ch);
        const float pd = a.row_div ? a.row_div[b] : 1.f;
        double piv[V];
#pragma unroll
        for (int j = 0; j < V; ++j) piv[j] = (double)(a.row_div ? pv.v[j] / pd : pv.v[j]);
        seg_rows4<V, false>(a, nullptr, nullptr, false, ch, r0 + rg, min(e, r0 + kRowsChunk),
                            [&](int64_t, const SegRow<V>& w) {
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float f = a.row_div ? w.x.v[j] / w.rd : w.x.v[j];
                const double d = (double)f - piv[j];
                s1[j] += d;
                s2[j] += d * d;
            }
            ++cnt;
        });
    }
    __shared__ double l1[G][64], l2[G][64];
    __shared__ int lc[G][L];
#pragma unroll
    for (int j = 0; j < V; ++j) {
        l1[rg][V * cl + j] = s1[j];
        l2[rg][V * cl + j] = s2[j];
    }
    lc[rg][cl] = cnt;
    __syncthreads();
    const int l = threadIdx.x;
    if (l < 64 && blockIdx.z * 64 + l < C) {
        double t1 = 0.0, t2 = 0.0;
        int tc = 0;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            t1 += l1[g][l];
            t2 += l2[g][l];
            tc += lc[g][(unsigned)l / V];
        }
        double* p = part + (((int64_t)seg * a.n_chunks + chunk) * C + blockIdx.z * 64 + l) * 3;
        p[0] = t1;
        p[1] = t2;
        p[2] = (double)tc;
    }
}

// dz = dy * post'(y) * act'(z); partial sums of dz and dz * xhat per (segment, chunk, channel).
// The layout of segnorm_stats_kernel, and for V = 1 its argument.
template <int V>
__global__ void __launch_bounds__(256)
segnorm_bwd_stats_kernel(SegApply p, const float* __restrict__ dy, const float* __restrict__ y,
                         double* __restrict__ part) {
    constexpr int L = 64 / V, G = 4 * V;
    const int seg = blockIdx.y, chunk = blockIdx.x;
    const int cl = threadIdx.x % L, rg = threadIdx.x / L;
    const int ch = blockIdx.z * 64 + V * cl;
    const int C = p.a.c;
    const int64_t b = p.a.seg_off[seg], e = p.a.seg_off[seg + 1];
    const int64_t r0 = b + (int64_t)chunk * kRowsChunk;
    double s1[V], s2[V];
#pragma unroll
    for (int j = 0; j < V; ++j) s1[j] = s2[j] = 0.0;
    if (ch < C && r0 < e) {
        const int64_t sc = (int64_t)seg * C + ch;
        const Chan<V> mu = ldc<V>(p.mean + sc), rs = ldc<V>(p.rstd + sc);
        Chan<V> gm, bt;
        ld_affine<V>(p, ch, gm, bt);
        seg_rows4<V, true>(p.a, dy, y, p.residual != nullptr, ch, r0 + rg, min(e, r0 + kRowsChunk),
                           [&](int64_t, const SegRow<V>& w) {
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const SegGrad g = seg_bwd_elem<false>(p, w.x.v[j], w.rd, mu.v[j], rs.v[j], gm.v[j], bt.v[j],
                                                      w.a.v[j], w.b.v[j]);
                s1[j] += (double)g.dz;
                s2[j] += (double)g.dz * (double)g.xh;
            }
        });
    }
    __shared__ double l1[G][64], l2[G][64];
#pragma unroll
    for (int j = 0; j < V; ++j) {
        l1[rg][V * cl + j] = s1[j];
        l2[rg][V * cl + j] = s2[j];
    }
    __syncthreads();
    const int l = threadIdx.x;
    if (l < 64 && blockIdx.z * 64 + l < C) {
        double t1 = 0.0, t2 = 0.0;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            t1 += l1[g][l];
            t2 += l2[g][l];
        }
        double* q = part + (((int64_t)seg * p.a.n_chunks + chunk) * C + blockIdx.z * 64 + l) * 2;
        q[0] = t1;
        q[1] = t2;
    }
}

// ---- the merges of the chunk partials ----------------------------------------------------
// Chunks k0, k0 + step, ... of (seg, ch), NP doubles each, added to s in that order with U
// chunk loads in flight.
template <int NP, int U>
__device__ __forceinline__ void seg_add_chunks(const double* __restrict__ part, int seg, int n_chunks,
                                               int c, int ch, int k0, int step, double (&s)[NP]) {
#pragma unroll U
    for (int k = k0; k < n_chunks; k += step) {
        const double* q = part + (((int64_t)seg * n_chunks + k) * c + ch) * NP;
#pragma unroll
        for (int j = 0; j < NP; ++j) s[j] += q[j];
    }
}

// The sums of one (segment, channel) over its chunks. This is the one definition of their
// order, for the merge kernels and the fused kernels alike: chunks 0, 1, 2, ... by one thread;
// or, in a fused block with more than kSegFuseChunks chunks (split4: the BatchNorms over every
// row), the four waves sum the chunks congruent to their index mod 4 -- waves 1..3 into sred
// (seg_merge_side, then a barrier) -- and wave 0 adds them in wave order. lane: the channel's
// index within the block's 64.
template <int NP>
__device__ __forceinline__ void seg_merge_side(const double* __restrict__ part, int seg, int n_chunks,
                                               int c, double (*sred)[NP][64]) {
    const int tid = threadIdx.x, ch = blockIdx.z * 64 + (tid & 63), w = tid >> 6;
    if (tid < 64 || ch >= c) return;
    double s[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) s[j] = 0.0;
    seg_add_chunks<NP, 4>(part, seg, n_chunks, c, ch, w, 4, s);
#pragma unroll
    for (int j = 0; j < NP; ++j) sred[w - 1][j][tid & 63] = s[j];
}

template <int NP>
__device__ __forceinline__ void seg_merge(const double* __restrict__ part, int seg, int n_chunks, int c,
                                          int ch, bool split4, double (*sred)[NP][64], int lane,
                                          double (&s)[NP]) {
#pragma unroll
    for (int j = 0; j < NP; ++j) s[j] = 0.0;
    seg_add_chunks<NP, 8>(part, seg, n_chunks, c, ch, 0, split4 ? 4 : 1, s);
    if (split4)
        for (int w = 0; w < 3; ++w)
#pragma unroll
            for (int j = 0; j < NP; ++j) s[j] += sred[w][j][lane];
}

// Forward: (sum d, sum d^2, rows) with d = v - pivot -> mean, rstd, biased var; zeros for an
// empty segment.
struct SegMoments {
    float mean, rstd, var;
};

__device__ __forceinline__ SegMoments seg_merge_fwd(const SegArgs& a, const double* __restrict__ part,
                                                    float eps, int seg, int ch, bool split4,
                                                    double (*sred)[3][64], int lane) {
    SegMoments m = {0.f, 0.f, 0.f};
    const int64_t b = a.seg_off[seg], e = a.seg_off[seg + 1];
    if (e <= b) return m;
    double s[3];
    seg_merge<3>(part, seg, a.n_chunks, a.c, ch, split4, sred, lane, s);
    const double piv = (double)(a.row_div ? a.x[b * a.c + ch] / a.row_div[b] : a.x[b * a.c + ch]);
    const double m1 = s[0] / s[2];
    const double vv = fmax(s[1] / s[2] - m1 * m1, 0.0);
    m.mean = (float)(piv + m1);
    m.var = (float)vv;
    m.rstd = (float)(1.0 / sqrt(vv + (double)eps));
    return m;
}

// Backward: s1 = sum dz, s2 = sum dz xhat of the segment.
__device__ __forceinline__ void seg_merge_bwd(const SegArgs& a, const double* __restrict__ part, int seg,
                                              int ch, bool split4, double (*sred)[2][64], int lane,
                                              float& s1, float& s2) {
    double s[2];
    seg_merge<2>(part, seg, a.n_chunks, a.c, ch, split4, sred, lane, s);
    s1 = (float)s[0];
    s2 = (float)s[1];
}

// dgamma = sum dz xhat, dbeta = sum dz over every segment's chunks, in (segment, chunk) order
__device__ __forceinline__ void seg_merge_affine_grads(const SegArgs& a, const double* __restrict__ part,
                                                       int ch, float* __restrict__ dgamma,
                                                       float* __restrict__ dbeta) {
    double g[2] = {0.0, 0.0};
    for (int sg = 0; sg < a.n_seg; ++sg) seg_add_chunks<2, 8>(part, sg, a.n_chunks, a.c, ch, 0, 1, g);
    dbeta[ch] = (float)g[0];
    dgamma[ch] = (float)g[1];
}

// Thread per (segment, channel): merge the chunk partials in order -> mean, rstd, biased var.
__global__ void __launch_bounds__(256)
segnorm_merge_kernel(SegArgs a, const double* __restrict__ part, float eps, float* __restrict__ mean,
                     float* __restrict__ rstd, float* __restrict__ var) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)a.n_seg * a.c) return;
    const SegMoments m = seg_merge_fwd(a, part, eps, (int)(t / a.c), (int)(t % a.c), false, nullptr, 0);
    mean[t] = m.mean;
    rstd[t] = m.rstd;
    var[t] = m.var;
}

// Thread per (segment, channel): the chunk sums in order -> sdz, sdzx (per segment); with
// gamma, thread per channel also sums over segments -> dgamma, dbeta.
__global__ void __launch_bounds__(256)
segnorm_bwd_merge_kernel(SegArgs a, const double* __restrict__ part, float* __restrict__ sums,
                         float* __restrict__ dgamma, float* __restrict__ dbeta) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)a.n_seg * a.c) return;
    const int seg = (int)(t / a.c), ch = (int)(t % a.c);
    seg_merge_bwd(a, part, seg, ch, false, nullptr, 0, sums[2 * t], sums[2 * t + 1]);
    if (dgamma && seg == 0) seg_merge_affine_grads(a, part, ch, dgamma, dbeta);
}

// ---- the elementwise passes, one thread per V channels of a row -----------------------------
// V = 4: 32-bit element indices (float4 indices stay below 2^31, seg_vec_ok) and the segment
// table in LDS; V = 1: 64-bit indices and the table in global memory.
template <int V>
struct SegFlat {
    using idx_t = std::conditional_t<V == 4, int, int64_t>;
    idx_t t, r;      // the thread's V-channel vector and its row
    int ch, seg;
    bool live;
};

template <int V>
__device__ __forceinline__ SegFlat<V> seg_flat(const SegApply& p) {
    using idx_t = typename SegFlat<V>::idx_t;
    __shared__ int64_t so[kSegLds + 1];
    if constexpr (V == 4) {
        if (p.a.n_seg <= kSegLds)
            for (int i = threadIdx.x; i <= p.a.n_seg; i += 256) so[i] = p.a.seg_off[i];
        __syncthreads();
    }
    SegFlat<V> f;
    const int cv = p.a.c / V;
    f.t = (idx_t)blockIdx.x * 256 + threadIdx.x;
    f.live = f.t < (idx_t)(p.n * cv);
    if (!f.live) return f;
    f.r = f.t / cv;
    f.ch = V * (int)(f.t - f.r * cv);
    if constexpr (V == 4)
        f.seg = p.a.n_seg <= kSegLds ? find_segment(so, p.a.n_seg, f.r) : find_segment(p.a.seg_off, p.a.n_seg, f.r);
    else
        f.seg = find_segment(p.a.seg_off, p.a.n_seg, f.r);
    return f;
}

template <int V>
__global__ void __launch_bounds__(256)
segnorm_apply_kernel(SegApply p, float* __restrict__ out) {
    const SegFlat<V> f = seg_flat<V>(p);
    if (!f.live) return;
    const int64_t sc = (int64_t)f.seg * p.a.c + f.ch, o = (int64_t)V * f.t;
    const Chan<V> xv = ldc<V>(p.a.x + o);
    const float rd = p.a.row_div ? p.a.row_div[f.r] : 1.f;
    const Chan<V> mu = ldc<V>(p.mean + sc), rs = ldc<V>(p.rstd + sc);
    Chan<V> gm, bt;
    ld_affine<V>(p, f.ch, gm, bt);
    const Chan<V> rv = p.residual ? ldc<V>(p.residual + o) : fillc<V>(0.f);
    Chan<V> y;
#pragma unroll
    for (int j = 0; j < V; ++j)
        y.v[j] = seg_fwd_elem(p, xv.v[j], rd, mu.v[j], rs.v[j], gm.v[j], bt.v[j], rv.v[j]);
    stc<V>(out + o, y);
}

// dx and dres = dy * post'(y) from the merged sums (s1, s2 interleaved per (segment, channel))
template <int V>
__global__ void __launch_bounds__(256)
segnorm_bwd_apply_kernel(SegApply p, const float* __restrict__ dy, const float* __restrict__ y,
                         const float* __restrict__ sums, float* __restrict__ dx,
                         float* __restrict__ dres) {
    const SegFlat<V> f = seg_flat<V>(p);
    if (!f.live) return;
    const int64_t sc = (int64_t)f.seg * p.a.c + f.ch, o = (int64_t)V * f.t;
    const float inv_n = 1.0f / (float)(p.a.seg_off[f.seg + 1] - p.a.seg_off[f.seg]);
    const Chan<V> mu = ldc<V>(p.mean + sc), rs = ldc<V>(p.rstd + sc);
    Chan<V> gm, bt;
    ld_affine<V>(p, f.ch, gm, bt);
    const float rd = p.a.row_div ? p.a.row_div[f.r] : 1.f;
    const Chan<V> xv = ldc<V>(p.a.x + o), dv = ldc<V>(dy + o);
    const Chan<V> yv = p.residual ? ldc<V>(y + o) : fillc<V>(0.f);
    const Chan<V> sa = ldc<V>(sums + 2 * sc), sb = ldc<V>(sums + 2 * sc + V);
    float s[2 * V];                                               // (s1, s2) per channel
#pragma unroll
    for (int j = 0; j < V; ++j) {
        s[j] = sa.v[j];
        s[V + j] = sb.v[j];
    }
    Chan<V> gx, gres;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const SegGrad g = seg_bwd_elem<true, V>(p, xv.v[j], rd, mu.v[j], rs.v[j], gm.v[j], bt.v[j], dv.v[j],
                                                yv.v[j], s[2 * j], s[2 * j + 1], inv_n);
        gres.v[j] = g.gr;
        gx.v[j] = g.dx;
    }
    if (dres) stc<V>(dres + o, gres);
    stc<V>(dx + o, gx);
}

// ---- the merges folded into the apply passes: one block per (chunk, segment, 64 channels) as
// the statistics pass, whose first 64 threads merge the 64 channels' chunk partials into LDS
// with the merge kernels' own functions (seg_merge_fwd / seg_merge_bwd: up to kSegFuseChunks
// chunks the same order and roundings, so bit-identical results), then the block applies them
// to its chunk's rows. The chunk-0 block writes mean / rstd / var (forward) or dgamma / dbeta
// (backward, segment 0).
__global__ void __launch_bounds__(256)
segnorm_merge_apply4_kernel(SegApply p, const double* __restrict__ part, float eps, float* __restrict__ mean,
                            float* __restrict__ rstd, float* __restrict__ var, float* __restrict__ out) {
    __shared__ float smu[64], srs[64];
    __shared__ double sred[3][3][64];
    const int seg = blockIdx.y, chunk = blockIdx.x;
    const int C = p.a.c;
    const int64_t b = p.a.seg_off[seg], e = p.a.seg_off[seg + 1];
    const int64_t r0 = b + (int64_t)chunk * kRowsChunk;
    if (r0 >= e && chunk != 0) return;                         // block-uniform
    const int tid = threadIdx.x;
    const bool split4 = p.a.n_chunks > kSegFuseChunks;
    if (split4) {
        seg_merge_side<3>(part, seg, p.a.n_chunks, C, sred);
        __syncthreads();
    }
    if (tid < 64 && blockIdx.z * 64 + tid < C) {
        const int ch = blockIdx.z * 64 + tid;
        const int64_t t = (int64_t)seg * C + ch;
        const SegMoments m = seg_merge_fwd(p.a, part, eps, seg, ch, split4, sred, tid);
        smu[tid] = m.mean;
        srs[tid] = m.rstd;
        if (chunk == 0) {
            mean[t] = m.mean;
            rstd[t] = m.rstd;
            var[t] = m.var;
        }
    }
    __syncthreads();
    if (r0 >= e) return;
    const int cl = tid & 15, rg = tid >> 4;
    const int ch = blockIdx.z * 64 + 4 * cl;
    if (ch >= C) return;
    const Chan<4> mu = {{smu[4 * cl], smu[4 * cl + 1], smu[4 * cl + 2], smu[4 * cl + 3]}};
    const Chan<4> rs = {{srs[4 * cl], srs[4 * cl + 1], srs[4 * cl + 2], srs[4 * cl + 3]}};
    Chan<4> gm, bt;
    ld_affine<4>(p, ch, gm, bt);
    seg_rows4<4, false>(p.a, nullptr, p.residual, p.residual != nullptr, ch, r0 + rg, min(e, r0 + kRowsChunk),
                        [&](int64_t r, const SegRow<4>& w) {
        Chan<4> y;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            y.v[j] = seg_fwd_elem(p, w.x.v[j], w.rd, mu.v[j], rs.v[j], gm.v[j], bt.v[j], w.b.v[j]);
        stc<4>(out + r * C + ch, y);
    });
}

__global__ void __launch_bounds__(256)
segnorm_bwd_merge_apply4_kernel(SegApply p, const float* __restrict__ dy, const float* __restrict__ y,
                                const double* __restrict__ part, float* __restrict__ dgamma,
                                float* __restrict__ dbeta, float* __restrict__ dx, float* __restrict__ dres) {
    __shared__ float sm1[64], sm2[64];
    __shared__ double sred[3][2][64];
    const int seg = blockIdx.y, chunk = blockIdx.x;
    const int C = p.a.c;
    const int64_t b = p.a.seg_off[seg], e = p.a.seg_off[seg + 1];
    const int64_t r0 = b + (int64_t)chunk * kRowsChunk;
    const bool gblock = dgamma && seg == 0 && chunk == 0;
    if (r0 >= e && !gblock) return;                            // block-uniform
    const int tid = threadIdx.x;
    const bool split4 = p.a.n_chunks > kSegFuseChunks;         // as the forward
    if (split4) {
        seg_merge_side<2>(part, seg, p.a.n_chunks, C, sred);
        __syncthreads();
    }
    if (tid < 64 && blockIdx.z * 64 + tid < C) {
        const int ch = blockIdx.z * 64 + tid;
        seg_merge_bwd(p.a, part, seg, ch, split4, sred, tid, sm1[tid], sm2[tid]);
        if (gblock) seg_merge_affine_grads(p.a, part, ch, dgamma, dbeta);
    }
    __syncthreads();
    if (r0 >= e) return;
    const int cl = tid & 15, rg = tid >> 4;
    const int ch = blockIdx.z * 64 + 4 * cl;
    if (ch >= C) return;
    const int64_t sc = (int64_t)seg * C + ch;
    const float inv_n = 1.0f / (float)(e - b);
    const Chan<4> mu = ldc<4>(p.mean + sc), rs = ldc<4>(p.rstd + sc);
    Chan<4> gm, bt;
    ld_affine<4>(p, ch, gm, bt);
    const Chan<4> m1 = {{sm1[4 * cl], sm1[4 * cl + 1], sm1[4 * cl + 2], sm1[4 * cl + 3]}};
    const Chan<4> m2 = {{sm2[4 * cl], sm2[4 * cl + 1], sm2[4 * cl + 2], sm2[4 * cl + 3]}};
    seg_rows4<4, true>(p.a, dy, y, p.residual != nullptr, ch, r0 + rg, min(e, r0 + kRowsChunk),
                       [&](int64_t r, const SegRow<4>& w) {
        Chan<4> gx, gres;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const SegGrad g = seg_bwd_elem<true>(p, w.x.v[j], w.rd, mu.v[j], rs.v[j], gm.v[j], bt.v[j],
                                                 w.a.v[j], w.b.v[j], m1.v[j], m2.v[j], inv_n);
            gres.v[j] = g.gr;
            gx.v[j] = g.dx;
        }
        if (dres) stc<4>(dres + r * C + ch, gres);
        stc<4>(dx + r * C + ch, gx);
    });
}

}  // namespace
}  // namespace fgr

using namespace fgr;

// ---- dispatch ----------------------------------------------------------------------------
// the float4 kernels: c % 4 == 0, every given pointer 16-B aligned (NULL allowed), float4
// indices below 2^31
static bool seg_vec_ok(int64_t n, int c, std::initializer_list<const void*> ptrs) {
    if (c % 4 != 0 || n * c / 4 >= (int64_t)1 << 31) return false;
    for (const void* q : ptrs)
        if (reinterpret_cast<uintptr_t>(q) & 15) return false;
    return true;
}

static int seg_chunks(int64_t max_seg_len) { return (int)std::max<int64_t>(1, ceil_div(max_seg_len, kRowsChunk)); }

// The kernels of one call, from its shape and the pointers its float4 kernels would touch:
// scalar (V = 1), float4 (V = 4), or float4 with the merge inside the apply pass.
enum SegPath { kSegScalar, kSegVec, kSegVecFused };

static SegPath seg_path(int64_t n, int c, int n_chunks, std::initializer_list<const void*> ptrs) {
    static const bool fuse = [] { const char* e = getenv("FGR_SEG_FUSED"); return !(e && e[0] == '0'); }();
    if (!seg_vec_ok(n, c, ptrs)) return kSegScalar;
    return fuse && n > 0 && n_chunks <= kSegFuseChunksMax ? kSegVecFused : kSegVec;
}

// The argument checks of every entry point (who, for the error text), all before its first
// launch: the sizes, gamma / beta (/ dgamma / dbeta) given together or not at all (paired),
// the pointers it needs (need_rows: only where there are rows), and the workspace:
// fgr_segnorm_workspace + ws_extra bytes.
static int seg_check(const char* who, int64_t n, int c, int n_seg, int64_t max_seg_len, bool paired,
                     std::initializer_list<const void*> need, std::initializer_list<const void*> need_rows,
                     size_t ws_bytes, size_t ws_extra) {
    FGR_REQUIRE(n >= 0 && c > 0 && n_seg > 0 && max_seg_len >= 0 && paired, "%s: bad arguments", who);
    for (const void* q : need) FGR_REQUIRE(q, "%s: null pointer", who);
    if (n > 0)
        for (const void* q : need_rows) FGR_REQUIRE(q, "%s: null pointer", who);
    size_t part_bytes = 0;
    fgr_segnorm_workspace(max_seg_len, c, n_seg, &part_bytes);
    FGR_REQUIRE(ws_bytes >= part_bytes + ws_extra,
                "%s: workspace too small (fgr_segnorm_workspace + %zu bytes)", who, ws_extra);
    return FGR_OK;
}

static dim3 seg_chunk_grid(const SegArgs& a) { return dim3(a.n_chunks, a.n_seg, (unsigned)ceil_div(a.c, 64)); }
static dim3 seg_flat_grid(int64_t elems) { return dim3((unsigned)ceil_div(elems, 256)); }

// the statistics pass reads x alone through float4s
static int seg_launch_stats(const SegArgs& a, int64_t n, double* part, hipStream_t st) {
    if (seg_path(n, a.c, a.n_chunks, {a.x}) != kSegScalar)
        hipLaunchKernelGGL(segnorm_stats_kernel<4>, seg_chunk_grid(a), dim3(256), 0, st, a, part);
    else
        hipLaunchKernelGGL(segnorm_stats_kernel<1>, seg_chunk_grid(a), dim3(256), 0, st, a, part);
    FGR_CHECK_LAUNCH("segnorm_stats_kernel");
    return FGR_OK;
}

static int seg_launch_merge(const SegArgs& a, const double* part, float eps, float* mean, float* rstd,
                            float* var, hipStream_t st) {
    hipLaunchKernelGGL(segnorm_merge_kernel, seg_flat_grid((int64_t)a.n_seg * a.c), dim3(256), 0, st, a, part,
                       eps, mean, rstd, var);
    FGR_CHECK_LAUNCH("segnorm_merge_kernel");
    return FGR_OK;
}

static int seg_launch_apply(const SegApply& p, bool vec, float* out, hipStream_t st) {
    if (vec)
        hipLaunchKernelGGL(segnorm_apply_kernel<4>, seg_flat_grid(p.n * p.a.c / 4), dim3(256), 0, st, p, out);
    else
        hipLaunchKernelGGL(segnorm_apply_kernel<1>, seg_flat_grid(p.n * p.a.c), dim3(256), 0, st, p, out);
    FGR_CHECK_LAUNCH("segnorm_apply_kernel");
    return FGR_OK;
}

extern "C" int fgr_segnorm_workspace(int64_t max_seg_len, int32_t c, int32_t n_seg, size_t* bytes) {
    FGR_REQUIRE(bytes && max_seg_len >= 0 && c > 0 && n_seg >= 0, "fgr_segnorm_workspace: bad arguments");
    *bytes = (size_t)n_seg * seg_chunks(max_seg_len) * c * 3 * sizeof(double);
    return FGR_OK;
}

extern "C" int fgr_segnorm_stats(const float* x, int64_t n, int32_t c, const int64_t* seg_off,
                                 int32_t n_seg, int64_t max_seg_len, const float* row_div, float eps,
                                 float* mean, float* rstd, float* var, void* ws, size_t ws_bytes,
                                 void* stream) {
    if (int rc = seg_check("fgr_segnorm_stats", n, c, n_seg, max_seg_len, true,
                           {x, seg_off, mean, rstd, var, ws}, {}, ws_bytes, 0))
        return rc;
    const SegArgs a{x, row_div, seg_off, n_seg, c, seg_chunks(max_seg_len)};
    hipStream_t st = as_stream(stream);
    if (int rc = seg_launch_stats(a, n, (double*)ws, st)) return rc;
    return seg_launch_merge(a, (const double*)ws, eps, mean, rstd, var, st);
}

extern "C" int fgr_segnorm_apply(const float* x, int64_t n, int32_t c, const int64_t* seg_off,
                                 int32_t n_seg, const float* row_div, const float* mean,
                                 const float* rstd, const float* gamma, const float* beta, int32_t act,
                                 const float* residual, int32_t post_act, float* out, void* stream) {
    if (int rc = seg_check("fgr_segnorm_apply", n, c, n_seg, 0, !gamma == !beta, {},
                           {x, seg_off, mean, rstd, out}, SIZE_MAX, 0))              // no workspace
        return rc;
    if (n == 0) return FGR_OK;
    const SegApply p{{x, row_div, seg_off, n_seg, c, 1}, n, mean, rstd, gamma, beta, act, residual, post_act};
    const bool vec = seg_path(n, c, 1, {x, out, residual, mean, rstd, gamma, beta}) != kSegScalar;
    return seg_launch_apply(p, vec, out, as_stream(stream));
}

// validate, the statistics pass, then merge + apply in one launch (fused) or two
extern "C" int fgr_segnorm_fwd(const float* x, int64_t n, int32_t c, const int64_t* seg_off,
                               int32_t n_seg, int64_t max_seg_len, const float* row_div, float eps,
                               float* mean, float* rstd, float* var, const float* gamma,
                               const float* beta, int32_t act, const float* residual,
                               int32_t post_act, float* out, void* ws, size_t ws_bytes,
                               void* stream) {
    if (int rc = seg_check("fgr_segnorm_fwd", n, c, n_seg, max_seg_len, !gamma == !beta,
                           {x, seg_off, mean, rstd, var, ws}, {out}, ws_bytes, 0))
        return rc;
    const SegApply p{{x, row_div, seg_off, n_seg, c, seg_chunks(max_seg_len)}, n, mean, rstd, gamma, beta, act,
                     residual, post_act};
    const SegPath path = seg_path(n, c, p.a.n_chunks, {x, out, residual, mean, rstd, gamma, beta});
    hipStream_t st = as_stream(stream);
    if (int rc = seg_launch_stats(p.a, n, (double*)ws, st)) return rc;
    if (path == kSegVecFused) {
        hipLaunchKernelGGL(segnorm_merge_apply4_kernel, seg_chunk_grid(p.a), dim3(256), 0, st, p,
                           (const double*)ws, eps, mean, rstd, var, out);
        FGR_CHECK_LAUNCH("segnorm_merge_apply4_kernel");
        return FGR_OK;
    }
    if (int rc = seg_launch_merge(p.a, (const double*)ws, eps, mean, rstd, var, st)) return rc;
    if (n == 0) return FGR_OK;
    return seg_launch_apply(p, path == kSegVec, out, st);
}

// validate, the statistics pass, then merge + apply in one launch (fused) or two
extern "C" int fgr_segnorm_bwd(const float* x, int64_t n, int32_t c, const int64_t* seg_off,
                               int32_t n_seg, int64_t max_seg_len, const float* row_div,
                               const float* mean, const float* rstd, const float* gamma,
                               const float* beta, int32_t act, int32_t has_residual, int32_t post_act,
                               const float* y, const float* dy, float* dx, float* dres,
                               float* dgamma, float* dbeta, void* ws, size_t ws_bytes, void* stream) {
    if (!has_residual) y = dres = nullptr;                     // y is read for post'(y) alone
    if (int rc = seg_check("fgr_segnorm_bwd", n, c, n_seg, max_seg_len,
                           (!gamma == !beta) && (!gamma == !dgamma) && (!dgamma == !dbeta),
                           {x, seg_off, mean, rstd, dy, dx, ws, has_residual ? (const void*)y : ws}, {}, ws_bytes,
                           (size_t)std::max(n_seg, 0) * std::max(c, 0) * 2 * sizeof(float)))
        return rc;
    // workspace: the chunk partials (2 doubles per entry, inside the stats' 3-double region of
    // fgr_segnorm_workspace bytes) followed by the merged sums (2 floats per (segment, channel))
    size_t part_bytes = 0;
    fgr_segnorm_workspace(max_seg_len, c, n_seg, &part_bytes);
    double* part = (double*)ws;
    float* sums = (float*)((char*)ws + part_bytes);
    const SegApply p{{x, row_div, seg_off, n_seg, c, seg_chunks(max_seg_len)}, n, mean, rstd, gamma, beta, act,
                     y, post_act};
    const SegPath path = seg_path(n, c, p.a.n_chunks, {x, dy, y, dx, dres, mean, rstd, gamma, beta, sums});
    hipStream_t st = as_stream(stream);
    if (path != kSegScalar)
        hipLaunchKernelGGL(segnorm_bwd_stats_kernel<4>, seg_chunk_grid(p.a), dim3(256), 0, st, p, dy, y, part);
    else
        hipLaunchKernelGGL(segnorm_bwd_stats_kernel<1>, seg_chunk_grid(p.a), dim3(256), 0, st, p, dy, y, part);
    FGR_CHECK_LAUNCH("segnorm_bwd_stats_kernel");
    if (path == kSegVecFused) {
        hipLaunchKernelGGL(segnorm_bwd_merge_apply4_kernel, seg_chunk_grid(p.a), dim3(256), 0, st, p, dy, y,
                           (const double*)part, dgamma, dbeta, dx, dres);
        FGR_CHECK_LAUNCH("segnorm_bwd_merge_apply4_kernel");
        return FGR_OK;
    }
    hipLaunchKernelGGL(segnorm_bwd_merge_kernel, seg_flat_grid((int64_t)n_seg * c), dim3(256), 0, st, p.a,
                       (const double*)part, sums, dgamma, dbeta);
    FGR_CHECK_LAUNCH("segnorm_bwd_merge_kernel");
    if (n == 0) return FGR_OK;
    if (path == kSegVec)
        hipLaunchKernelGGL(segnorm_bwd_apply_kernel<4>, seg_flat_grid(n * c / 4), dim3(256), 0, st, p, dy, y,
                           (const float*)sums, dx, dres);
    else
        hipLaunchKernelGGL(segnorm_bwd_apply_kernel<1>, seg_flat_grid(n * c), dim3(256), 0, st, p, dy, y,
                           (const float*)sums, dx, dres);
    FGR_CHECK_LAUNCH("segnorm_bwd_apply_kernel");
    return FGR_OK;
}
