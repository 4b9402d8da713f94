// The matrix-core attention kernels' shared parts (attention16.hip: f16x3 forward, dQ, dK/dV;
// bf16.hip: bf16 forward): the per-(tile, head) K / V image layout, which the image kernels and
// the in_proj GEMM epilogues (gemm_rs.hip, gemm_ws.hip, gemm5.hip, bf16.hip) write and the
// attention kernels read, and the pieces of the key-tile loop. One definition each; device
// parts force-inlined, sizes constexpr (host and device).
// A kernel uses a loop part only where its generated tile loop stays what it was with the code
// written out (same opcodes and s_waitcnt between its first and last barrier, DESIGN.md "The
// matrix-core attention kernels from one set of parts"); load_row8, split_row8 and tile_loop
// did not pass that in every kernel and say below who uses them. Substituting them in the
// other kernels changes those kernels' loops or speed: compile and compare before doing so.
#pragma once
#include <type_traits>

#include "mfma.h"

namespace fgr {

// ---- image layout. One image holds a 64-key tile of one head, in 16-B units (8 halves):
//   K: [k-step DH/32][term][g 4][key 64] x 16 B (dims 32 ks + 8 g .. + 7)   ds_read_b128
//   V: [term][key 64][DH] halves, 16-B chunk index XOR v_swz<DH>(key)      ds_read_b64_tr_b16
// TERMS = 2 for the f16x3 split (hi, lo), 1 for bf16.
constexpr int kv_unit_v(int dh, int terms) { return terms * (dh / 32) * 256; }       // first V unit
constexpr int kv_units(int dh, int terms) { return kv_unit_v(dh, terms) + terms * 8 * dh; }
static_assert(kv_units(32, 2) == 1024 && kv_unit_v(32, 2) == 512, "f16x3 image, head dim 32");
static_assert(kv_units(64, 2) == 2048 && kv_unit_v(64, 2) == 1024, "f16x3 image, head dim 64");
static_assert(kv_units(32, 1) == 512 && kv_unit_v(32, 1) == 256, "bf16 image, head dim 32");
static_assert(kv_units(64, 1) == 1024 && kv_unit_v(64, 1) == 512, "bf16 image, head dim 64");

// V image row swizzle: XOR applied to the 16-B chunk index of key row `key`, so that the
// ds_read_b64_tr_b16 of a 32-lane group (8 key rows x 32 B) hits 64 distinct banks. DH 32
// (64-B rows, 4 per 256-B bank period): rows r, r + 4 separated by 32 B (row bit 2); DH 64
// (128-B rows, 2 per period): rows r, r + 2, r + 4, r + 6 share banks and take four distinct
// 32-B chunk pairs (row bits 1-2) -- without it they read 2-way conflicted (round-3 PMC:
// 1.2 M conflict cycles per 0.9 M LDS instructions at DH 64, none at DH 32).
template <int DH>
__host__ __device__ __forceinline__ constexpr int v_swz(int key) {
    static_assert(DH == 32 || DH == 64, "head dim");
    if constexpr (DH == 64) return ((key >> 1) & 3) << 1;
    else return ((key >> 2) & 1) << 1;
}

template <int DH, int TERMS>
struct KvImage {
    static constexpr int units = kv_units(DH, TERMS), unit_v = kv_unit_v(DH, TERMS);
    // byte offset of the K unit of (k-step, term, 8-dim group g, key)
    static __host__ __device__ __forceinline__ constexpr int k_unit(int ks, int term, int g, int key) {
        return (((ks * TERMS + term) * 4 + g) * 64 + key) * 16;
    }
    // 16-B chunk `chunk` (dims 8 chunk .. + 7) of V row (term, key) of the image at `base`
    template <class P>
    static __host__ __device__ __forceinline__ P v_chunk_at(P base, int term, int key, int chunk) {
        return base + unit_v * 16 + term * (128 * DH) + key * (2 * DH) + (chunk ^ v_swz<DH>(key)) * 16;
    }
};

// Tile numbering, times n_head plus the head for the image index. Per segment (the image
// kernels): tile t of segment s, whose rows start at packed row row0, is row0 / 64 + s + t, so
// every segment starts a tile of its own; global (the GEMM epilogues): packed row r lies in
// tile r / 64 whatever its segment, and a segment starts row0 & 63 rows into its first tile.
__host__ __device__ __forceinline__ constexpr int64_t seg_tile(int64_t row0, int s) { return row0 / 64 + s; }
__host__ __device__ __forceinline__ constexpr int64_t global_tile(int64_t row) { return row / 64; }
// tiles that the per-segment numbering of n_seg segments over n_rows rows can reach
constexpr int64_t n_tiles16(int64_t n_rows, int32_t n_seg) { return n_rows / 64 + n_seg + 1; }

// ---- host side: bytes of nt images; an f16x3 image set is nt images followed by their nt
// (e_k, e_v) exponents (bf16 images carry none)
inline int64_t kv_image_bytes(int64_t nt, int dh, int terms) { return nt * kv_units(dh, terms) * 16; }
inline int64_t kv_space_bytes(int64_t nt, int dh) { return kv_image_bytes(nt, dh, 2) + nt * 8; }
template <class U4, class I2>
struct KvSpaceOf {
    U4* img;
    I2* sc;
};
using KvSpace = KvSpaceOf<uint4, int2>;
using KvSpaceConst = KvSpaceOf<const uint4, const int2>;
inline KvSpace kv_space(void* base, int64_t nt, int dh) {
    return {static_cast<uint4*>(base),
            reinterpret_cast<int2*>(static_cast<char*>(base) + kv_image_bytes(nt, dh, 2))};
}
inline KvSpaceConst kv_space(const void* base, int64_t nt, int dh) {
    return {static_cast<const uint4*>(base),
            reinterpret_cast<const int2*>(static_cast<const char*>(base) + kv_image_bytes(nt, dh, 2))};
}

// Calls f(integral_constant<int, DH>) for the run-time head dim (32 or 64, checked by the
// callers), attn_with_modes f(.., bool_constant<DROP>) for the dropout switch too, so kernels
// take them as template parameters
template <class F>
void attn_with_dh(int head_dim, F&& f) {
    if (head_dim == 64) f(std::integral_constant<int, 64>{});
    else f(std::integral_constant<int, 32>{});
}
template <class F>
void attn_with_modes(int head_dim, bool drop, F&& f) {
    attn_with_dh(head_dim, [&](auto dh_tag) {
        if (drop) f(dh_tag, std::true_type{});
        else f(dh_tag, std::false_type{});
    });
}

// ---- tile-loop parts. Lane maps of the 16x16x32 MFMA (lane l, g = l >> 4, c = l & 15):
// A[i = c][k = 8g + e], B[k = 8g + e][j = c], C[i = 4g + r][j = c].
typedef __attribute__((address_space(3))) char lds_c;
typedef __attribute__((address_space(3))) u32x4 lds_u4;
typedef __attribute__((address_space(3))) s16x4 lds_s4;
using B0 = std::integral_constant<int, 0>;       // LDS buffer tags
using B1 = std::integral_constant<int, 1>;

__device__ __forceinline__ void split2(float x, _Float16& h, _Float16& m) {
    h = (_Float16)x;
    m = (_Float16)(x - (float)h);
}

// Block -> ((segment, head) pair, 64-row block): blocks L, L + 1, .. of one XCD (L & 7) take
// consecutive row blocks of one pair. False for the padding past n_seg * n_head pairs.
// Used by the dQ and dK/dV kernels; the two forward kernels keep it written out (speed)
__device__ __forceinline__ bool block_split(int n_blk, int n_seg, int n_head, int& seg, int& head,
                                            int& blk) {
    const int L = blockIdx.x, xcd = L & 7, j0 = L >> 3;
    const int pair = (j0 / n_blk) * 8 + xcd;
    blk = j0 % n_blk;
    if (pair >= n_seg * n_head) return false;
    seg = pair / n_head;
    head = pair % n_head;
    return true;
}

// this lane's B-operand part of a row: dims 32 kd + 8 g .. + 7 from p = row + head * DH + 8 g
// (zeros if !ok). Used by the dQ kernel; the two forward kernels and dK/dV keep the load
// written out (f16x3 forward: kept the parent's stream; bf16 forward: speed; dK/dV: its load,
// scale and row maxima are one loop)
template <int KD>
__device__ __forceinline__ void load_row8(const float* p, bool ok, float (&x)[KD][8]) {
#pragma unroll
    for (int kd = 0; kd < KD; ++kd) {
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
        if (ok) {
            a = ld4(p + 32 * kd);
            b = ld4(p + 32 * kd + 4);
        }
        x[kd][0] = a.x; x[kd][1] = a.y; x[kd][2] = a.z; x[kd][3] = a.w;
        x[kd][4] = b.x; x[kd][5] = b.y; x[kd][6] = b.z; x[kd][7] = b.w;
    }
}

// x *= pre; -> the row's scale exponent e (row_scale_exp of max |x| over the row's four g
// lanes) and the two-term split of x 2^e. Used by the dQ kernel; in the f16x3 forward and in
// dK/dV it changed s_nop / s_waitcnt counts inside the tile loop, so they keep it written out
template <int KD>
__device__ __forceinline__ int split_row8(float (&x)[KD][8], float pre, f16x8 (&t)[KD][2]) {
    float mx = 0.f;
#pragma unroll
    for (int kd = 0; kd < KD; ++kd)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            x[kd][e] *= pre;
            mx = fmaxf(mx, fabsf(x[kd][e]));
        }
    const int ex = row_scale_exp(xg_max(mx));
    const float s = __builtin_ldexpf(1.f, ex);
#pragma unroll
    for (int kd = 0; kd < KD; ++kd)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            _Float16 h, m;
            split2(x[kd][e] * s, h, m);
            t[kd][0][e] = h; t[kd][1][e] = m;
        }
    return ex;
}

// per-lane LDS byte addresses within an image; everything else is an instruction offset.
// K fragment reads: key c of 8-dim group g
__device__ __forceinline__ uint32_t k_frag_addr(int g, int c) { return (uint32_t)(g * 64 + c) * 16; }
// V transposed reads: lane c = 4qq + p reads rows 4g + qq (+16 k, +32 j), columns
// 16t + 4p .. +3: chunk 2t + (p >> 1) XOR the image's row swizzle
template <int DH, int TERMS>
__device__ __forceinline__ uint32_t v_tr_addr(int g, int c, int t) {
    const int qq = c >> 2, pp = c & 3;
    return KvImage<DH, TERMS>::unit_v * 16 + (4 * g + qq) * (2 * DH) +
           (((2 * t + (pp >> 1)) ^ v_swz<DH>(4 * g + qq)) * 16) + (pp & 1) * 8;
}

// A fragment of keys 16 n .. + 15, k-step kd, one term, from the K part of the image at bp
template <class T8, int DH, int TERMS>
__device__ __forceinline__ T8 read_k_frag(lds_c* bp, uint32_t kaddr, int kd, int term, int n) {
    return __builtin_bit_cast(T8, *(lds_u4*)(bp + kaddr + KvImage<DH, TERMS>::k_unit(kd, term, 0, 16 * n)));
}
// transposed A fragment (dims x keys) of one term and 32-key step from the V part: vb =
// image + vaddr[t] + term * 128 DH + j * 32 * 2 DH
template <int DH>
__device__ __forceinline__ s16x8 read_v_tr(lds_c* vb) {
    const s16x4 a0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4*)vb);
    const s16x4 a1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4*)(vb + 16 * (2 * DH)));
    return __builtin_shufflevector(a0, a1, 0, 1, 2, 3, 4, 5, 6, 7);
}
template <int DH>
__device__ __forceinline__ void read_v_tr2(lds_c* vb, f16x8 (&vf)[2]) {     // both f16x3 terms
#pragma unroll
    for (int tm = 0; tm < 2; ++tm) vf[tm] = __builtin_bit_cast(f16x8, read_v_tr<DH>(vb + tm * (128 * DH)));
}

// one 1-KiB piece (64 lanes x 16 B) global -> LDS by LDS-DMA; src is this lane's unit
__device__ __forceinline__ void dma_piece(const u32x4* src, lds_c* dst) {
    __builtin_amdgcn_global_load_lds((const void*)src, (__attribute__((address_space(3))) void*)dst,
                                     16, 0, 0);
}
template <int N>
__device__ __forceinline__ void dma_pieces(const u32x4* src, lds_c* dst) {
#pragma unroll
    for (int j = 0; j < N; ++j) dma_piece(src + j * 64, dst + j * 1024);
}

// ---- the two-buffer tile loop: tile t + 1 in flight (dma(t + 1, other buffer)) while
// body(t, buffer ..) computes tile t; one barrier per tile. The buffers are two LDS objects
// of the kernel and dma / body address them by pointers derived from those objects (the
// compiler then knows that the DMA into one cannot alias reads of the other; one array made it
// wait vmcnt(0) for the next tile's DMA before the first V read of every tile). Unrolled by
// two, so that both buffers' addresses are per-lane constants + instruction offsets.
// a tile body's first step: tile tt has landed in buffer BUF, tile tt + 1 starts into the other
template <int BUF, class Dma>
__device__ __forceinline__ void tile_enter(int tt, int ntile, Dma& dma) {
    wait_vm_lgkm0<0>();             // this wave's pieces of tile tt landed
    __builtin_amdgcn_s_barrier();   // everyone's landed; buffer 1 - BUF no longer read
    if (tt + 1 < ntile) dma(tt + 1, std::integral_constant<int, 1 - BUF>{});
}
// ntile tiles, tile tt in buffer tt & 1 (the caller has started tile 0 into buffer 0). Used
// by the dQ kernel; dK/dV keeps the same loop written out (as a function it cost an s_nop and
// an s_waitcnt in two of its loops), the forwards have the lead / shift form:
// body(tt, buf), which begins with tile_enter
template <class Body>
__device__ __forceinline__ void tile_loop(int ntile, Body&& body) {
    int tt = 0;
    for (; tt + 2 <= ntile; tt += 2) {
        body(tt, B0{});
        body(tt + 1, B1{});
    }
    if (tt < ntile) body(tt, B0{});
}

}  // namespace fgr
