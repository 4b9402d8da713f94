/* fgreg.h -- C ABI of libfgreg.so, the MI355X (gfx950) kernels of the per-pair
 * registration forward of "Boosting Fine-grained Feature Fusion in 3D Point
 * Cloud Registration" (a REGTR fork: KPConv + Res2Net backbone, cross-attention
 * transformer, weighted-Procrustes pose).
 *
 * Conventions (every entry point):
 *  - all array arguments are DEVICE pointers allocated by the caller; nothing
 *    is allocated inside (data-dependent sizes use a count call + a fill call,
 *    scratch comes from a caller-provided workspace sized by *_workspace());
 *  - `stream` is a hipStream_t passed as void*; all work is stream-ordered,
 *    no call synchronises the device or the host;
 *  - return 0 on success, a negative FGR_E* code on error; the message of the
 *    last error on the calling thread is returned by fgr_last_error();
 *  - no C++ exception crosses the ABI; no mutable global state besides a
 *    per-thread error string.
 *
 * Packed layout: clouds are stacked along rows in the reference's order
 * src_0..src_{B-1}, tgt_0..tgt_{B-1} (models/finegrained_regtr.py:121), with
 * int64 row offsets `off[n_clouds + 1]`. A neighbour table is (Nq, width)
 * int64 whose missing entries hold the "shadow" index Ns_total
 * (finegrained_kpconv.py:288-291).
 */
#ifndef FGREG_H
#define FGREG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FGR_ABI_VERSION 2

enum {
    FGR_OK = 0,
    FGR_E_ARG = -1,      /* invalid argument / shape            */
    FGR_E_LAUNCH = -2,   /* HIP launch or runtime error          */
    FGR_E_WORKSPACE = -3 /* workspace too small                  */
};

/* radius-search row semantics */
enum {
    FGR_NB_INDEX = 0, /* PyTorch3D ball_query: first `width` supports in index order
                         (finegrained_kpconv.py:266-293, PreprocessorGPU)          */
    FGR_NB_DIST = 1   /* nanoflann radiusSearch(sorted) + [:, :K]: the `width`
                         nearest, ties by index (neighbors.cpp:211-332, :260-261)  */
};

/* activation codes; FGR_ACT_RELU_RES_LEAKY (the f16x3 GEMMs only) applies the residual AFTER
 * the ReLU: C = LeakyReLU_0.1(ReLU(A.W + bias) + R) -- a Res2Net block output plus its
 * identity shortcut (finegrained_kpconv_blocks.py:715-725) in one epilogue. */
enum { FGR_ACT_NONE = 0, FGR_ACT_LEAKY = 1, FGR_ACT_RELU = 2, FGR_ACT_RELU_RES_LEAKY = 3,
       /* the exact (erf) GELU: fgr_ffn_f16x3_act only. NO GEMM entry point takes it (their
        * epilogues have no GELU; callers run the GEMM with FGR_ACT_NONE, then fgr_gelu_fwd) */
       FGR_ACT_GELU = 4 };

int fgr_abi_version(void);
const char* fgr_last_error(void);

/* Opt-in instrumentation (bench.py's per-kernel rooflines; not part of the reference's
 * interface): arms two caller-created hipEvent_t for the NEXT timed entry point called on
 * this thread (fgr_kpconv_gather, fgr_attention*, fgr_gemm_f16x3, fgr_gemm_bf16,
 * fgr_grid_subsample_count / _fill, fgr_grid_subsample_sparse_count / _fill, fgr_radius_search,
 * fgr_radius_grid_build, fgr_radius_search_grid, fgr_instnorm, fgr_layernorm,
 * fgr_pair_pose). That call records `start_event` on its stream right before its
 * first kernel launch and `end_event` after its last one, then disarms; (NULL, NULL)
 * disarms explicitly. Thread-local like the error string. */
int fgr_time_next_call(void* start_event, void* end_event);

/* ---- grid subsampling ------------------------------------------------------------
 * Replaces batch_grid_subsampling_kpconv_gpu (finegrained_kpconv.py:218-245; ME
 * UNWEIGHTED_AVERAGE) and its CPU twin subsample_batch
 * (cpp_subsampling/wrapper.cpp:62-333 -> grid_subsampling.cpp:5-211).
 * Voxel key and barycentre follow grid_subsampling.cpp bit for bit; voxels are
 * emitted in ascending key order per cloud, members summed in ascending point index.
 * `max_cells`: a counting sort over a dense voxel-key histogram of that many counters (the
 * clouds' key spaces nx*ny*nz laid end to end; 0 = the default 8 n_points + 2^20; < 0 is
 * rejected: the round-1 radix-sort path was removed in round 5; key spaces too large for a
 * histogram go through fgr_grid_subsample_sparse_* below). The same max_cells must be
 * passed to all three calls.
 * 1) fgr_grid_subsample_count: writes counts[c] (voxels of cloud c) and
 *    counts[n_clouds] (total) as int64; keeps the sorted state in `ws`. Dense path only:
 *    if the key space exceeds max_cells, counts[n_clouds] = -(cells needed) and nothing else
 *    is valid -- call again with a larger max_cells.
 * 2) fgr_grid_subsample_fill: writes out_points (total, 3) and optionally the
 *    voxel keys (total) from the same `ws` (must follow the count call). */
int fgr_grid_subsample_workspace(int64_t n_points, int32_t n_clouds, int64_t max_cells,
                                 size_t* bytes);
int fgr_grid_subsample_count(const float* points, const int64_t* off, int32_t n_clouds,
                             int64_t n_points, float dl, int64_t max_cells, void* ws,
                             size_t ws_bytes, int64_t* counts, void* stream);
int fgr_grid_subsample_fill(int64_t n_points, int32_t n_clouds, int64_t max_cells, int64_t n_out,
                            void* ws, size_t ws_bytes, const float* points, float* out_points,
                            int64_t* out_keys, void* stream);

/* Sparse path for large-extent clouds (outdoor lidar at a 5 cm voxel): the same outputs as
 * the dense trio above, bit for bit, from one stable 8-bit radix sort of (voxel key, point
 * index) over all points. The workspace (fgr_grid_subsample_sparse_workspace() bytes) and the
 * time depend on n_points and n_clouds only, never on the clouds' extent; it needs no
 * pre-clearing. `key_bits`: 0, or an upper bound on the bits of the clouds' summed key space
 * (e.g. from the -(cells needed) a dense count reported) -- only ceil(key_bits / 8) sort passes
 * are then launched (0: all eight; passes the key space does not need return at once).
 * fgr_grid_subsample_sparse_count writes counts as fgr_grid_subsample_count does; a limit is
 * reported, never truncated, as counts[n_clouds] < 0 with every counts[c] = 0:
 *   -1  a cloud has more than 2^20 voxels along an axis,
 *   -2  the clouds' summed key space nx*ny*nz reaches 2^62,
 *   -3  key_bits is smaller than the summed key space needs.
 * n_points >= 2^31 is an argument error. fgr_grid_subsample_sparse_fill must follow the count
 * call on the same `ws`. */
int fgr_grid_subsample_sparse_workspace(int64_t n_points, int32_t n_clouds, size_t* bytes);
int fgr_grid_subsample_sparse_count(const float* points, const int64_t* off, int32_t n_clouds,
                                    int64_t n_points, float dl, int32_t key_bits, void* ws,
                                    size_t ws_bytes, int64_t* counts, void* stream);
int fgr_grid_subsample_sparse_fill(int64_t n_points, int32_t n_clouds, int64_t n_out, void* ws,
                                   size_t ws_bytes, const float* points, float* out_points,
                                   int64_t* out_keys, void* stream);

/* ---- radius neighbour search -----------------------------------------------------
 * Replaces batch_neighbors_kpconv_gpu (ball_query, finegrained_kpconv.py:266-293)
 * and batch_neighbors_kpconv (cpp_neighbors.batch_query, :248-263).
 * d2 = ((qx-sx)^2 + (qy-sy)^2) + (qz-sz)^2 in fp32 without FMA, kept iff d2 < r*r.
 * fgr_radius_count: uncapped neighbour count per query + the max (int32 scalar);
 * fgr_radius_search: fills out (nq, width) int64 (mode FGR_NB_*; DIST needs width <= 64). */
int fgr_radius_count(const float* q, const int64_t* q_off, const float* s, const int64_t* s_off,
                     int32_t n_clouds, int64_t nq, int32_t max_q_len, float radius,
                     int32_t* counts, int32_t* max_count, void* stream);
int fgr_radius_search(const float* q, const int64_t* q_off, const float* s, const int64_t* s_off,
                      int32_t n_clouds, int64_t nq, int64_t ns, int32_t max_q_len, float radius,
                      int32_t mode, int32_t width, int64_t* out, void* stream);

/* Cell-binned radius search for large clouds (same rows as fgr_radius_search, both modes):
 * fgr_radius_grid_build bins the supports of every cloud into cubic cells of edge
 * >= 1.0625 * radius (a counting sort; the grid workspace, fgr_radius_grid_workspace() bytes,
 * depends on ns and n_clouds only); fgr_radius_search_grid then scans the 27 cells around
 * each query. One grid serves every query set searched with a radius <= the build radius
 * over the same supports (the conv and pool tables of a pyramid level). width <= 256.
 * With counts != NULL it writes the uncapped counts + their max instead (fgr_radius_count). */
int fgr_radius_grid_workspace(int64_t ns, int32_t n_clouds, size_t* bytes);
int fgr_radius_grid_build(const float* s, const int64_t* s_off, int32_t n_clouds, int64_t ns,
                          float radius, void* grid, size_t grid_bytes, void* stream);
int fgr_radius_search_grid(const float* q, const int64_t* q_off, int32_t n_clouds, int64_t nq,
                           int32_t max_q_len, const float* s, const int64_t* s_off, int64_t ns,
                           const void* grid, size_t grid_bytes, float radius, int32_t mode,
                           int32_t width, int64_t* out, int32_t* counts, int32_t* max_count,
                           void* stream);

/* ---- KPConv ------------------------------------------------------------------------
 * The gather-weight stage of KPConv.forward (finegrained_kpconv_blocks.py:296-381,
 * rigid, linear influence, sum aggregation):
 *   wf[q, k, c] = sum_{valid h} max(0, 1 - |(s[idx[q,h]] - q) - kp[k]| / extent) * x[idx[q,h], c]
 * and the normaliser of :395-399: nnorm[q] = max(1, #{valid h : sum_c x[idx[q,h], c] > 0}).
 * The caller finishes with (wf.view(nq, K*cin) @ W.view(K*cin, cout)) / nnorm.
 * cin: 1..64, 128 or 256; n_kp <= 32. Any other cin (96, 192, ...) returns FGR_E_ARG
 * before anything is launched or written.
 * workspace: fgr_kpconv_gather_workspace() bytes (per-source-row flags of the normaliser). */
int fgr_kpconv_gather_workspace(int64_t ns, int32_t cin, size_t* bytes);
int fgr_kpconv_gather(const float* q, const float* s, int64_t nq, int64_t ns, const int64_t* idx,
                      int32_t width, const float* x, int32_t cin, const float* kp, int32_t n_kp,
                      float extent, float* wf, float* nnorm, void* workspace, size_t ws_bytes,
                      void* stream);

/* The other influence functions and aggregation modes of KPConv.forward (:347-372). With
 * d2 = |(s[idx[q,h]] - q) - kp[k]|^2 the weight of neighbour h at kernel point k is
 *   FGR_KP_LINEAR    max(0, 1 - sqrt(d2) / extent)                      (fgr_kpconv_gather)
 *   FGR_KP_GAUSSIAN  exp(-d2 / (2 (0.3 extent)^2 + 1e-9))               (radius_gaussian, :100-107)
 *   FGR_KP_CONSTANT  1
 * and FGR_AGG_CLOSEST multiplies it by [k == argmin_k d2] (the lowest k on an exact tie).
 * Shadow entries are skipped in every mode (their feature row is zero in the reference) and
 * nnorm does not depend on the mode. fgr_kpconv_gather_mode takes the arguments, widths,
 * workspace and refusals of fgr_kpconv_gather, which is its (FGR_KP_LINEAR, FGR_AGG_SUM)
 * case; any other mode value returns FGR_E_ARG before anything is launched or written. */
#define FGR_KP_LINEAR 0
#define FGR_KP_GAUSSIAN 1
#define FGR_KP_CONSTANT 2
#define FGR_AGG_SUM 0
#define FGR_AGG_CLOSEST 1
int fgr_kpconv_gather_mode(const float* q, const float* s, int64_t nq, int64_t ns,
                           const int64_t* idx, int32_t width, const float* x, int32_t cin,
                           const float* kp, int32_t n_kp, float extent, int32_t influence,
                           int32_t aggregation, float* wf, float* nnorm, void* workspace,
                           size_t ws_bytes, void* stream);

/* Deformable (and modulated) KPConv, the `deformable` branch of KPConv.forward (:270-345,
 * :384-385). A rigid offset KPConv (fgr_kpconv_gather_mode + the weight GEMM) gives the raw
 * offset product (nq, 3K; 4K when modulated) and its normaliser.
 *  fgr_kpconv_deform_points  with f = offset_raw / offset_nnorm + offset_bias:
 *      kp_q[q, k, :] = kp[k] + extent * f[q, 3k : 3k + 3]            (nq, K, 3)
 *      mod[q, k]     = 2 sigmoid(f[q, 3K + k])                       (nq, K)
 *    mod == NULL: not modulated (offset_raw has 3K columns, else 4K).
 *  fgr_kpconv_gather_deform  fgr_kpconv_gather_mode under every query's own kernel points, with
 *    d2[q, h, k] = |(s[idx[q,h]] - q) - kp_q[q, k]|^2. A valid neighbour is IN RANGE iff
 *    d2 < extent^2 for some k; one that is not is a shadow (the reference's topk re-indexing,
 *    :319-343, without its host readback):
 *      wf[q, k, c] = mod[q, k] * sum_{in-range h} w(d2[q, h, k]) x[idx[q,h], c]   (mod NULL: 1)
 *      nnorm[q]    = max(1, #{in-range h : sum_c x[idx[q,h], c] > 0})
 *    The widths, n_kp, modes and refusals of fgr_kpconv_gather_mode; x and wf 16-B aligned at
 *    cin 128 / 256. workspace: fgr_kpconv_gather_deform_workspace() bytes.
 *  fgr_kpconv_scatter_deform  dx (ns, cin) of that gather from dwf (nq, K * cin) over the CSR
 *    inverse of fgr_nbr_inverse, as fgr_kpconv_scatter_mode; the in-range mask is a constant.
 *  fgr_kpconv_deform_grad    d_kp (nq, K, 3) and d_mod (nq, K; NULL: skipped) of that gather from
 *    dwf: through w into kp_q (none under FGR_KP_CONSTANT: exact zeros; 0 at d2 = 0, where the
 *    reference's sqrt has no derivative) and through mod. The in-range mask and the closest
 *    one-hot are constants. One wave owns each (q, k): no atomics, bit-reproducible.
 * Every entry point checks its arguments before anything is launched or written: a bad mode,
 * cin, n_kp or extent returns FGR_E_ARG and fgr_last_error names the entry point and the value. */
int fgr_kpconv_deform_points(const float* offset_raw, const float* offset_nnorm,
                             const float* offset_bias, const float* kp, int64_t nq, int32_t n_kp,
                             float extent, float* kp_q, float* mod, void* stream);
int fgr_kpconv_gather_deform_workspace(int64_t ns, int32_t cin, size_t* bytes);
int fgr_kpconv_gather_deform(const float* q, const float* s, int64_t nq, int64_t ns,
                             const int64_t* idx, int32_t width, const float* x, int32_t cin,
                             const float* kp_q, const float* mod, int32_t n_kp, float extent,
                             int32_t influence, int32_t aggregation, float* wf, float* nnorm,
                             void* workspace, size_t ws_bytes, void* stream);
int fgr_kpconv_scatter_deform_workspace(int64_t nq, int32_t width, int32_t cin, size_t* bytes);
int fgr_kpconv_scatter_deform(const float* q, const float* s, int64_t nq, int64_t ns,
                              const int64_t* idx, int32_t width, const float* dwf, int32_t cin,
                              const float* kp_q, const float* mod, int32_t n_kp, float extent,
                              int32_t influence, int32_t aggregation, const int32_t* start,
                              const int32_t* pos, float* dx, void* ws, size_t ws_bytes,
                              void* stream);
int fgr_kpconv_deform_grad(const float* q, const float* s, int64_t nq, int64_t ns,
                           const int64_t* idx, int32_t width, const float* x, int32_t cin,
                           const float* dwf, const float* kp_q, const float* mod, int32_t n_kp,
                           float extent, int32_t influence, int32_t aggregation, float* d_kp,
                           float* d_mod, void* stream);

/* max_pool (finegrained_kpconv_blocks.py:125-141): out[q, c] = max over the row of
 * x[idx[q, h], c], shadow entries contributing 0 (the appended zero row). */
int fgr_max_pool(const float* x, int64_t ns, int32_t c, const int64_t* idx, int64_t nq,
                 int32_t width, float* out, void* stream);

/* ---- normalisation -----------------------------------------------------------------
 * Segmented instance norm, nn.InstanceNorm1d(affine=False) applied per cloud
 * (BatchNormBlock, finegrained_kpconv_blocks.py:498-507), fused with:
 *   v   = row_div ? x[r, c] / row_div[r] : x[r, c]       (KPConv normaliser, :399)
 *   y   = act((v - mean_seg,c) / sqrt(var_seg,c + eps))   (biased variance)
 *   out = residual ? post_act(y + residual[r, c]) : y     (bottleneck sum, :725)
 * Segments of up to 1024 rows are normalised from registers in one launch; longer
 * ones need a workspace of fgr_instnorm_workspace() bytes (two launches). */
int fgr_instnorm_workspace(int64_t max_seg_len, int32_t c, int32_t n_seg, size_t* bytes);
int fgr_instnorm(const float* x, int64_t n, int32_t c, const int64_t* seg_off, int32_t n_seg,
                 int64_t max_seg_len, const float* row_div, float eps, int32_t act,
                 const float* residual, int32_t post_act, float* out, void* ws, size_t ws_bytes,
                 void* stream);

/* Row LayerNorm (nn.LayerNorm, transformers.py:105-107) with an optional added
 * tensor (the positional embedding, transformers.py:194-195): out = LN(x)*g + b (+ add).
 * If pre_bias is given, x += pre_bias is applied first and written back to x (the
 * deferred bias of the Linear that produced the residual stream). */
int fgr_layernorm(float* x, int64_t n, int32_t d, const float* gamma, const float* beta,
                  float eps, const float* add, const float* pre_bias, float* out, void* stream);
/* Two LayerNorms of the same rows in one pass (same eps, shared statistics):
 * out = LN(x)*gamma + beta (+ add), out2 = LN(x)*gamma2 + beta2 (+ add2). The cross encoder's
 * per-layer output norm (transformers.py:43-44, return_intermediate) of layer l and norm1 +
 * with_pos_embed of layer l + 1 (:193-195) read the same residual stream. x is not written. */
int fgr_layernorm_dual(const float* x, int64_t n, int32_t d, const float* gamma,
                       const float* beta, const float* add, float* out, const float* gamma2,
                       const float* beta2, const float* add2, float* out2, float eps,
                       void* stream);

/* out = a + b over n floats: the post-norm layer's with_pos_embed (transformers.py:121-124,
 * pre_norm: False; the pre-norm path fuses this add into fgr_layernorm). */
int fgr_add(const float* a, const float* b, int64_t n, float* out, void* stream);

/* Elementwise exact GELU over n floats (`transformer_act: gelu`, transformers.py:265-273 =
 * F.gelu) and its derivative, the formulas torch's fp32 F.gelu and its gradient evaluate:
 *   fgr_gelu_fwd:  y[i]  = 0.5 z[i] (1 + erf(z[i] / sqrt 2))
 *   fgr_gelu_bwd:  dz[i] = dy[i] (Phi(z[i]) + z[i] phi(z[i])),  Phi(z) = 0.5 (1 + erf(z / sqrt 2)),
 *                                                                phi(z) = exp(-z^2 / 2) / sqrt(2 pi)
 * The tails are exact: z <= -6 gives (-)0, z >= 6 gives z (and dz = dy), no NaN for any finite
 * z. All pointers 16-B aligned (FGR_E_ARG otherwise; n need not be a multiple of 4). In place
 * is allowed (y == z; dz == dy or dz == z); an output that overlaps an input partially is
 * FGR_E_ARG. n = 0 returns FGR_OK and touches nothing (pointers may be NULL); n < 0 or a null
 * pointer with n > 0 is FGR_E_ARG. Writes exactly n floats. */
int fgr_gelu_fwd(const float* z, float* y, int64_t n, void* stream);
int fgr_gelu_bwd(const float* z, const float* dy, float* dz, int64_t n, void* stream);

/* PositionEmbeddingCoordsSine (position_embedding.py:29-49) for 3-D input. */
int fgr_sine_pos_embed(const float* xyz, int64_t n, int32_t d_model, float temperature,
                       float scale, float* out, void* stream);

/* ---- Res2Net hierarchy ----------------------------------------------------------------
 * The fine-grained fusion core of my_Bottle2neck (res2net.py:126-148), eval BatchNorm
 * folded into the Linears: for i < scale - 1,
 *   sp_i = ReLU(W_i (sp_{i-1} + h_i) + b_i)          (sp_{-1} = 0)
 * writing cat = [sp_0 .. sp_{scale-2} | h_{scale-1} | x] (the conv3 / downsample operand).
 * h (n, scale*w), x (n, cin) or NULL, cat (n, ld_cat); bias (scale-1, w).
 * fgr_res2net_chain6 (fp32-accurate split bf16: three exact bf16 terms, six products; w = 112
 * or 224, dispatched at w = 224 where it measured faster): w_img = the (scale-1, w, w) folded
 * weights K-padded to a multiple of 32, split into three bf16 terms and laid out in 16x16x32
 * fragment order [i][jt][ks][term][g][c][8] (fgreg.ops.res2net_fragments3); h 16-B aligned. */
int fgr_res2net_chain6(const float* h, int64_t n, int32_t w, int32_t scale, const void* w_img,
                       const float* bias, const float* x, int32_t cin, float* cat,
                       int64_t ld_cat, void* stream);

/* fp32-accurate f16x3 variant (scaled two-term fp16 splits, see fgr_gemm_f16x3): rows of
 * a = sp_{i-1} + h_i scaled exactly per row, W_i rows pre-scaled per output column.
 * w_img = fgreg.ops.res2net_fragments_h3 image [i][jt][ks][term 2][g][c][8] (fp16), w_scale
 * (scale-1, w) the inverse column scales; h, cat, w_scale, bias 16-B aligned, ld_cat % 4 == 0. */
int fgr_res2net_chain_h3(const float* h, int64_t n, int32_t w, int32_t scale, const void* w_img,
                         const float* w_scale, const float* bias, const float* x, int32_t cin,
                         float* cat, int64_t ld_cat, void* stream);

/* The bottleneck front in one launch (f16x3): conv1 + the hierarchy + the concat, from x:
 *   h_j  = ReLU(W1_j x + b1_j)                        j < scale   (never stored, except the
 *   sp_i = ReLU(W_i (sp_{i-1} + h_i) + b_i)           i < scale-1  pass-through h_{scale-1})
 *   cat  = [sp_0 .. sp_{scale-2} | h_{scale-1} | x]
 * x (n, cin) contiguous, cat (n, ld_cat), ld_cat >= scale*w + cin and ld_cat % 4 == 0.
 * conv1 follows fgr_gemm_f16x3's row-stationary recipe: one exact power-of-two scale per row
 * of x, two fp16 terms, W1 pre-scaled per output row. w1_img = fgreg.ops.res2net_conv1_fragments
 * image [jt = j*KT + tile][ks][term 2][g][c][8] (fp16; KT = ceil(w / 16) tiles per chunk, each
 * chunk zero-padded to whole tiles; ks < cin / 32) with value
 * W1[j*w + 16 tile + c][32 ks + 8 g + e] * 2^e_row; w1_scale (scale*w) its inverse scales,
 * b1 (scale*w); w_img / w_scale / bias as fgr_res2net_chain_h3. Instances (w, cin): (28, 32),
 * (56, 64), (112, 128) -- w % 4 == 0 within the same tile counts; any other pair is refused
 * (224, 256) has fgr_res2net_block6 below.
 * Every pointer 16-B aligned. */
int fgr_res2net_block_h3(const float* x, int64_t n, int32_t w, int32_t cin, int32_t scale,
                         const void* w1_img, const float* w1_scale, const float* b1,
                         const void* w_img, const float* w_scale, const float* bias, float* cat,
                         int64_t ld_cat, void* stream);

/* The same front on the bf16x6 hierarchy (fgr_res2net_chain6's arithmetic for the chain,
 * conv1 in f16x3 as in fgr_res2net_block_h3, from the same w1_img / w1_scale / b1): the one
 * instance is (w, cin) = (224, 256), any other pair is refused. w_img / bias as
 * fgr_res2net_chain6. x, cat and both images 16-B aligned, ld_cat % 4 == 0. Rows per block
 * (16 / 32 / 48) by row count as fgr_res2net_chain6; the result does not depend on it. */
int fgr_res2net_block6(const float* x, int64_t n, int32_t w, int32_t cin, int32_t scale,
                       const void* w1_img, const float* w1_scale, const float* b1,
                       const void* w_img, const float* bias, float* cat, int64_t ld_cat,
                       void* stream);

/* ---- dense layers ----------------------------------------------------------------------
 * Every Linear / KPConv-weight product of the forward:
 *   C[m, n] = act(A[m, :] . W[n, :] + bias[n] (+ R[m, n]))
 * W is given as an image built once per weight (element (i, j) read from
 * w[i * stride_n + j * stride_k], so a (K, Cin, Cout) KPConv weight needs no transpose copy);
 * A fp32 row-major, 16-B aligned with lda % 4 == 0 when k % 8 == 0.
 *
 * fp32-accurate scaled split-fp16 GEMM ("f16x3", the default mode):
 * W rows are scaled by powers of two (row max in [2^14, 2^15)) and A rows on the fly (per
 * row, lowered only when a later k chunk would overflow fp16, with an exact rescale of the
 * partial sums); each operand is then split into two fp16 terms (2^-22 relative) and the
 * three significant term products accumulate in fp32 on v_mfma_f32_16x16x32_f16: <= ~3 *
 * 2^-22 relative per product (fp32's own rounding is 2^-24). The image (built once by
 * fgr_split_weights_h3, fgr_split_weights_h3_bytes() bytes, 16-B aligned) holds the split W
 * in tile order followed by the per-row inverse scales. */
int fgr_split_weights_h3_bytes(int32_t n, int32_t k, size_t* bytes);
int fgr_split_weights_h3(const float* w, int32_t n, int32_t k, int64_t stride_n,
                         int64_t stride_k, void* img, void* stream);
/* Many fgr_split_weights_h3 images in one launch (training re-splits every weight after each
 * optimizer step): descs = a DEVICE array of count descriptors, panel0 = the running sum of
 * the earlier descriptors' (n + 15) / 16, total_panels = the sum over all; every image
 * bit-equal to fgr_split_weights_h3's. */
typedef struct {
    const float* w;       /* element (i, j) at w[i * stride_n + j * stride_k] */
    void* img;            /* fgr_split_weights_h3_bytes(n, k) bytes, 16-B aligned */
    int64_t stride_n;
    int64_t stride_k;
    int64_t panel0;
    int32_t n;
    int32_t k;
} fgr_split_desc;
int fgr_split_weights_h3_batch(const void* descs, int32_t count, int64_t total_panels,
                               void* stream);
int fgr_gemm_f16x3(const float* a, int64_t lda, const void* w_img, float* c, int64_t ldc,
                   const float* bias, const float* r, int64_t ldr, int32_t m, int32_t n,
                   int32_t k, int32_t act, void* stream);

/* bf16 GEMM (the bf16 compute mode, BASELINE configs[4] -- 3DLoMatch with bf16 features),
 * same contract as fgr_gemm_f16x3 (act includes FGR_ACT_RELU_RES_LEAKY):
 *   C[m, n] = act(bf16(A[m, :]) . bf16(W[n, :]) + bias[n] (+ R[m, n]))
 * One v_mfma_f32_16x16x32_bf16 product per product: operands rounded to bf16 (RNE, ~2^-9
 * relative), fp32 accumulation, fp32 epilogue and output. Replaces the same nn.Linear /
 * KPConv-weight products as fgr_gemm_f16x3 (finegrained_regtr.py:47-105 via its layers) at a
 * third of the matrix-core work. W image built once by fgr_split_weights_bf16
 * (fgr_split_weights_bf16_bytes() bytes, 16-B aligned; element (i, j) read from
 * w[i * stride_n + j * stride_k]); A 16-B aligned with lda % 4 == 0 when k % 8 == 0. */
/* Split-K forms of fgr_gemm_f16x3 / fgr_gemm_bf16 (same contract plus a caller workspace):
 * where the tile grid alone cannot fill the chip (few activation rows, long K) the g5 kernel
 * runs ksplit parts over disjoint k ranges into the workspace and one launch sums them in a
 * fixed order and applies the epilogue (deterministic). fgr_gemm_workspace (mode 0 = f16x3,
 * 1 = bf16) returns the bytes the dispatcher wants for a shape (0: no split); a smaller or
 * NULL workspace runs unsplit. */
int fgr_gemm_workspace(int32_t m, int32_t n, int32_t k, int32_t mode, size_t* bytes);
int fgr_gemm_f16x3_ws(const float* a, int64_t lda, const void* w_img, float* c, int64_t ldc,
                      const float* bias, const float* r, int64_t ldr, int32_t m, int32_t n,
                      int32_t k, int32_t act, void* ws, size_t ws_bytes, void* stream);
int fgr_gemm_bf16_ws(const float* a, int64_t lda, const void* w_img, float* c, int64_t ldc,
                     const float* bias, const float* r, int64_t ldr, int32_t m, int32_t n,
                     int32_t k, int32_t act, void* ws, size_t ws_bytes, void* stream);

/* Pre-norm transformer sub-layer input, fused (transformers.py:193-196 norm1 ->
 * with_pos_embed -> self_attn in_proj; :213-221 norm2 -> multihead_attn in_proj; :231-232
 * norm3 -> linear1):
 *   C[m, n] = act(A[m, :] . W[n, :] + bias[n]),  A = LayerNorm_eps(X) * gamma + beta (+ add)
 * with the LayerNorm over the k features of each row (biased variance, as nn.LayerNorm) and
 * the f16x3 product of fgr_gemm_f16x3 (w_img from fgr_split_weights_h3). act: FGR_ACT_NONE or
 * FGR_ACT_RELU; add (optional, e.g. the positional embedding) has row stride ld_add. All
 * pointers 16-B aligned, row strides multiples of 4. Only for shapes where
 * fgr_gemm_f16x3_ln_supported(m, n, k) returns 1 (the row-stationary kernel: k <= 256,
 * k % 8 == 0, n % 16 == 0, many rows); FGR_E_ARG otherwise. */
int fgr_gemm_f16x3_ln_supported(int32_t m, int32_t n, int32_t k);
int fgr_gemm_f16x3_ln(const float* x, int64_t ldx, const float* gamma, const float* beta,
                      float eps, const float* add, int64_t ld_add, const void* w_img, float* c,
                      int64_t ldc, const float* bias, int32_t m, int32_t n, int32_t k,
                      int32_t act, void* stream);
/* fgr_gemm_f16x3_ln plus a second LayerNorm output of the same rows, written once:
 *   out2 = LayerNorm_eps(X) * gamma2 + beta2   (row stride ld_out2, 16-B aligned)
 * -- the cross encoder's per-layer output norm of layer l (transformers.py:43-44) computed in
 * the prologue of layer l + 1's in_proj, which normalises the same rows. Requires `add`. */
int fgr_gemm_f16x3_ln_out2(const float* x, int64_t ldx, const float* gamma, const float* beta,
                           float eps, const float* add, int64_t ld_add, const void* w_img,
                           float* c, int64_t ldc, const float* bias, int32_t m, int32_t n,
                           int32_t k, int32_t act, const float* gamma2, const float* beta2,
                           float* out2, int64_t ld_out2, void* stream);

/* Pre-norm position-wise feed-forward sub-layer in one launch (transformers.py:231-238):
 *   out = x + linear2(ReLU(linear1(LayerNorm_eps(x) * gamma + beta)))
 * x, out (m, d) (out may be x itself), linear1 (f, d) + b1, linear2 (d, f) + b2, the f16x3
 * products of fgr_gemm_f16x3; the (m, f) hidden activations never leave the chip.
 * w1_img: fgr_split_weights_h3 of linear1.weight; w2_img: fgr_split_weights_ffn2 of
 * linear2.weight (the chunk-major image in the k order the fused kernel consumes; bytes from
 * fgr_split_weights_ffn2_bytes(d, f), f % 32 == 0); bound (device, 2 floats) = {max_j
 * ||linear1.weight[j]||_2, max_j |b1[j]|} (sets the hidden values' fp16 scale). All pointers
 * 16-B aligned, row strides multiples of 4. fgr_ffn_f16x3_supported(m, d, f): d = 256,
 * 64 <= f <= 2048, f % 64 == 0 (the ModelNet transformer). Replaces the two-launch
 * linear1 (fgr_gemm_f16x3_ln) -> linear2 (fgr_gemm_f16x3_ws, residual) sequence.
 * fgr_ffn_f16x3_act: the same with the activation as an argument, FGR_ACT_RELU (exactly
 * fgr_ffn_f16x3, which calls it) or FGR_ACT_GELU (the exact erf GELU, 0.5 z (1 + erf(z / sqrt
 * 2)), formed on the fp32 hidden value before its fp16 split); any other code is FGR_E_ARG.
 * fgr_ffn_f16x3_act_supported(m, d, f, act): for FGR_ACT_RELU what fgr_ffn_f16x3_supported
 * returns; for FGR_ACT_GELU that and f % 128 == 0 (GELU exists in the weight-split kernel
 * only); 0 for any other code.
 * Unsupported GELU shapes run as fgr_gemm_f16x3_ln (FGR_ACT_NONE), fgr_gelu_fwd in place, then
 * fgr_gemm_f16x3_ws (residual). */
int fgr_split_weights_ffn2_bytes(int32_t n, int32_t k, size_t* bytes);
int fgr_split_weights_ffn2(const float* w, int32_t n, int32_t k, int64_t stride_n,
                           int64_t stride_k, void* img, void* stream);
int fgr_ffn_f16x3_supported(int32_t m, int32_t d, int32_t f);
int fgr_ffn_f16x3(const float* x, int64_t ldx, const float* gamma, const float* beta, float eps,
                  const void* w1_img, const float* b1, const void* w2_img, const float* b2,
                  const float* bound, float* out, int64_t ldo, int32_t m, int32_t d, int32_t f,
                  void* stream);
int fgr_ffn_f16x3_act_supported(int32_t m, int32_t d, int32_t f, int32_t act);
int fgr_ffn_f16x3_act(const float* x, int64_t ldx, const float* gamma, const float* beta,
                      float eps, const void* w1_img, const float* b1, const void* w2_img,
                      const float* b2, const float* bound, float* out, int64_t ldo, int32_t m,
                      int32_t d, int32_t f, int32_t act, void* stream);

/* PositionEmbeddingLearned (position_embedding.py:52-71) in one launch: the per-point MLP
 *   out[r] = L4(ReLU(L3(ReLU(L2(ReLU(L1(ReLU(L0(xyz[r])))))))))
 * with Linear widths 3 -> 32 -> 64 -> 128 -> 256 -> d_model (the hidden widths are the
 * reference's and fixed). xyz (n, 3) contiguous fp32; out (n, d_model) with row stride ldo.
 * Layer 0 (K = 3) runs in fp32 FMAs on the raw weight w0 (32, 3) row-major and bias b0 (32);
 * layers 1-4 are the f16x3 products of fgr_gemm_f16x3: wL_img = fgr_split_weights_h3 of
 * LinearL.weight ((64, 32), (128, 64), (256, 128), (d_model, 256); fgr_split_weights_h3_bytes
 * bytes each), bL the raw fp32 bias. Each hidden row is scaled for its fp16 split by one power
 * of two taken from that row's actual maximum (no host-supplied bound); the hidden activations
 * never leave the chip. A row's result depends on that row's coordinates alone -- bit for bit,
 * whatever the other rows of the call and wherever it stands in it. No workspace. Images, b1..b4
 * and out 16-B aligned, ldo >= d_model, ldo % 4 == 0; out[r][d_model .. ldo) is not written.
 * fgr_pos_mlp_f16x3_supported(n, d_model): n >= 1 and d_model 256 or 512; another d_model is
 * FGR_E_ARG with a message; n = 0 returns FGR_OK and touches nothing (as fgr_sine_pos_embed).
 * Replaces five fgr_gemm_f16x3 launches (FGR_ACT_RELU on the first four). */
int fgr_pos_mlp_f16x3_supported(int64_t n, int32_t d_model);
int fgr_pos_mlp_f16x3(const float* xyz, int64_t n, const float* w0, const float* b0,
                      const void* w1_img, const float* b1, const void* w2_img, const float* b2,
                      const void* w3_img, const float* b3, const void* w4_img, const float* b4,
                      int32_t d_model, float* out, int64_t ldo, void* stream);

/* GeometricStructureEmbedding (position_embedding.py:129-196) in two launches. For point i of a
 * cloud, nn(i) = its k nearest OTHER points of the same cloud (squared distance from coordinate
 * differences in fp32; i excluded by index; ties to the lower index),
 *   d_ij  = |p_j - p_i| / sigma_d                                              j in nn(i)
 *   a_ijr = atan2(|(p_r - p_i) x (p_j - p_i)|, (p_r - p_i) . (p_j - p_i)) * factor_a,  j, r in nn(i)
 *   E(t)  = [sin(t w_0), cos(t w_0), sin(t w_1), cos(t w_1), ...]   (d_model values)
 *   out_i = max_j [ proj_d(E(d_ij)) + red_r proj_a(E(a_ijr)) ],  red = max | mean, per channel.
 *
 * fgr_geo_embed_indices: xyz (n, 3) contiguous fp32, the clouds packed end to end; cloud_off
 * (n_clouds + 1) int64 DEVICE row offsets, cloud_off[0] = 0, cloud_off[n_clouds] = n. Writes nn
 * (n, k) int32 (packed row indices, nearest first), d (n, k), a (n, k, k) [i][j][r] fp32, exactly
 * those elements. k 1..4. A cloud must have more than k points; that is the CALLER's check (the
 * table is on the device): in a shorter cloud the missing neighbours are the point itself (d 0,
 * a 0), never a row of another cloud or out of bounds. factor_a = 180 / (sigma_a pi). Precise
 * sqrtf / atan2f, no atomics, deterministic. No workspace.
 *
 * fgr_geo_embed_f16x3: d, a as written above; div_term (d_model / 2) fp32 = w_m; wd_img / wa_img
 * = fgr_split_weights_h3 of proj_d.weight / proj_a.weight (d_model, d_model); bd / ba the raw
 * fp32 biases; reduction FGR_GEO_MAX / FGR_GEO_MEAN; out (n, d_model) with row stride ldo. The
 * k (1 + k) embedding rows of a point are built on chip (precise sinf / cosf) and never reach
 * memory; the projections are the f16x3 products of fgr_gemm_f16x3. A point's result depends on
 * its own d / a values alone, bit for bit. Images, biases, div_term and out 16-B aligned, ldo >=
 * d_model, ldo % 4 == 0; out[i][d_model .. ldo) is not written. No workspace.
 * fgr_geo_embed_f16x3_supported(n, d_model, k): n >= 1, d_model 256, k 1..4; anything else is
 * FGR_E_ARG with a message; n = 0 returns FGR_OK and touches nothing. */
#define FGR_GEO_MAX 0
#define FGR_GEO_MEAN 1
int fgr_geo_embed_indices(const float* xyz, int64_t n, const int64_t* cloud_off, int32_t n_clouds,
                          int32_t k, float sigma_d, float factor_a, int32_t* nn, float* d,
                          float* a, void* stream);
int fgr_geo_embed_f16x3_supported(int64_t n, int32_t d_model, int32_t k);
int fgr_geo_embed_f16x3(const float* d, const float* a, int64_t n, int32_t k,
                        const float* div_term, const void* wd_img, const float* bd,
                        const void* wa_img, const float* ba, int32_t d_model, int32_t reduction,
                        float* out, int64_t ldo, void* stream);

int fgr_split_weights_bf16_bytes(int32_t n, int32_t k, size_t* bytes);
int fgr_split_weights_bf16(const float* w, int32_t n, int32_t k, int64_t stride_n,
                           int64_t stride_k, void* img, void* stream);
int fgr_gemm_bf16(const float* a, int64_t lda, const void* w_img, float* c, int64_t ldc,
                  const float* bias, const float* r, int64_t ldr, int32_t m, int32_t n, int32_t k,
                  int32_t act, void* stream);

/* ---- attention ---------------------------------------------------------------------
 * Multi-head scaled-dot-product attention core of nn.MultiheadAttention
 * (transformers.py:95-96, 197-226) on packed, unpadded segments: query segment
 * i (rows q_off[i]..q_off[i+1]) attends to key segment kv_seg[i] (rows
 * kv_off[j]..kv_off[j+1]); the reference's key padding mask is the segment end.
 * Head h reads columns [h*dh, (h+1)*dh) of q/k/v rows (row strides ld_*).
 * o = softmax((q * scale) k^T) v, fp32 in/out, fp32 MFMA (v_mfma_f32_16x16x4_f32); any
 * head_dim in {4, 8, 16, 32, 64, 128, 256} (the forward dispatches head_dim 32 / 64 -- every
 * reference config -- to fgr_attention_f16x3 / _bf16 below). */
int fgr_attention(const float* q, int64_t ld_q, const float* k, int64_t ld_k, const float* v,
                  int64_t ld_v, float* o, int64_t ld_o, const int64_t* q_off,
                  const int64_t* kv_off, const int32_t* kv_seg, int32_t n_seg,
                  int32_t max_q_len, int32_t n_head, int32_t head_dim, float scale, void* stream);

/* The attention maps nn.MultiheadAttention returns beside its output (need_weights = True, the
 * default): the post-softmax weights averaged over the heads, which the reference's layers keep
 * as satt_weights / xatt_weights (transformers.py:177-179, 240-242) for
 * TransformerCrossEncoder.get_attentions (:61-81). Segments and heads as fgr_attention. For
 * packed query row r of segment i, n = the length of key segment kv_seg[i]:
 *   w[r * ld_w + j] = (1 / n_head) sum_h softmax_j(scale q_h[r] . k_h[j])     0 <= j < n
 *   w[r * ld_w + j] = 0                                                       n <= j < max_kv_len
 * and columns max_kv_len .. ld_w of a row are not written; an empty query segment writes
 * nothing (a non-empty one on an empty key segment is outside the contract). An inspection
 * path, not part of the forward: exact fp32 whatever the precision mode (v_mfma_f32_16x16x4_f32
 * scores, expf; no f16x3 split, no bf16), every element stored once and no atomics, so two runs
 * give the same bits. FGR_E_ARG with a message: head_dim not a multiple of 4 or above 256,
 * ld_w < max_kv_len, ld_q / ld_k < n_head * head_dim, or more heads than the kernel's 64 KiB
 * of LDS hold the (row, head) softmax statistics of (n_head <= 182 at head_dim >= 32). 16-B
 * loads / stores where the operand is 16-B aligned with a row stride that is a multiple of 4,
 * 4-B ones otherwise. No workspace. */
int fgr_attention_weights(const float* q, int64_t ld_q, const float* k, int64_t ld_k, float* w,
                          int64_t ld_w, const int64_t* q_off, const int64_t* kv_off,
                          const int32_t* kv_seg, int32_t n_seg, int32_t max_q_len,
                          int32_t max_kv_len, int32_t n_head, int32_t head_dim, float scale,
                          void* stream);

/* fp32-accurate attention on the fp16 matrix cores (head_dim 32 -- ModelNet's d 256 / 8 heads --
 * or 64 -- 3DMatch's d 512 / 8 heads), same semantics and arguments as fgr_attention plus
 * the key segment count / row count / longest key segment and a caller workspace: K/V are
 * scaled per (64-key tile, head), Q per query and P by 2^14 into fp16's normal range (exact
 * powers of two), split into two fp16 terms and the three significant term products
 * accumulate in fp32 (<= ~3 * 2^-22 per product); q/k/v/o 16-B aligned, row strides
 * multiples of 4. Workspace: fgr_attention_f16x3_workspace() bytes (split
 * K/V images + per-tile scale exponents), 16-B aligned. */
int fgr_attention_f16x3_workspace(int64_t n_kv_rows, int32_t n_kv_seg, int32_t n_head,
                                  size_t* bytes);
int fgr_attention_f16x3(const float* q, int64_t ld_q, const float* k, int64_t ld_k,
                        const float* v, int64_t ld_v, float* o, int64_t ld_o,
                        const int64_t* q_off, const int64_t* kv_off, const int32_t* kv_seg,
                        int32_t n_seg, int32_t n_kv_seg, int64_t n_kv_rows, int32_t max_q_len,
                        int32_t max_kv_len, int32_t n_head, int32_t head_dim, float scale,
                        void* workspace, int64_t ws_bytes, void* stream);

/* bf16 attention (the bf16 compute mode; head_dim 32 or 64), same semantics and arguments as
 * fgr_attention_f16x3: q * scale * log2(e), K, V and the softmax numerators P rounded to bf16
 * (RNE) where they enter v_mfma_f32_16x16x32_bf16; scores, the online softmax, accumulation
 * and the output stay fp32. Workspace: fgr_attention_bf16_workspace() bytes (bf16 K/V
 * images), 16-B aligned. */
int fgr_attention_bf16_workspace(int64_t n_kv_rows, int32_t n_kv_seg, int32_t n_head,
                                 size_t* bytes);
int fgr_attention_bf16(const float* q, int64_t ld_q, const float* k, int64_t ld_k,
                       const float* v, int64_t ld_v, float* o, int64_t ld_o,
                       const int64_t* q_off, const int64_t* kv_off, const int32_t* kv_seg,
                       int32_t n_seg, int32_t n_kv_seg, int64_t n_kv_rows, int32_t max_q_len,
                       int32_t max_kv_len, int32_t n_head, int32_t head_dim, float scale,
                       void* workspace, int64_t ws_bytes, void* stream);

/* CorrespondenceDecoder.simple_attention (finegrained_regtr.py:328-363; the soft
 * correspondence head of direct_regress_coor: False): single-head attention of width d whose
 * values are the partner cloud's coordinates, for all (layer, cloud) segments in one launch:
 *   out[r] = sum_j softmax_j(scale * q[r] . k[j]) * xyz[v_off[s'] + (j - kv_off[s'])]
 * for query row r of segment s (rows q_off[s]..q_off[s+1]), s' = kv_seg[s], keys j in
 * kv_off[s']..kv_off[s'+1]. fp32; d in {32, 64, 128, 256, 512}; out (rows, 3). */
int fgr_corr_attention(const float* q, int64_t ld_q, const float* k, int64_t ld_k,
                       const float* xyz, float* out, const int64_t* q_off, const int64_t* kv_off,
                       const int32_t* kv_seg, const int64_t* v_off, int32_t n_seg,
                       int32_t max_q_len, int32_t d, float scale, void* stream);

/* CorrespondenceDecoder with num_neighbors > 0 (finegrained_regtr.py:353-357), applied to the
 * output of fgr_corr_attention (same q, k, segments and scale). The reference's
 * `neighbor_mask[:, :, topk(attn, k).indices] = 0` indexes the QUERY dimension with top-k KEY
 * indices, so a query row j keeps its unmasked softmax iff j is in the union U_dir of the
 * top-k key indices of every (layer, pair, query) row of its direction (src->tgt, tgt->src);
 * every other row is NaN (softmax of an all -inf row). Segments i with (i % n_clouds) <
 * n_clouds / 2 are the src direction. flags (2 * max_kv_len bytes, device) receive U as
 * bytes, direction-major, for the caller's index-range check (an index >= Q raises in the
 * reference). Ties rank the lower key index first. Workspace: fgr_corr_topk_workspace. */
int fgr_corr_topk_workspace(int64_t n_rows, int32_t max_kv_len, size_t* bytes);
int fgr_corr_topk_mask(const float* q, int64_t ld_q, const float* k, int64_t ld_k, float* out,
                       const int64_t* q_off, const int64_t* kv_off, const int32_t* kv_seg,
                       int32_t n_seg, int32_t n_clouds, int64_t n_rows, int32_t max_q_len,
                       int32_t max_kv_len, int32_t d, float scale, int32_t n_top, uint8_t* flags,
                       void* ws, size_t ws_bytes, void* stream);

/* Batched device-to-device copies: n (src[i] -> dst[i], bytes[i]) triples (host arrays of device
 * pointers) in one launch per 32 copies; 16-B accesses where both ends are 16-B aligned. Not a
 * reference interface: the HIP-graph replay of the forward refreshes its static inputs and
 * clones its outputs with it (one dispatch instead of one blit per tensor). */
int fgr_copy_batch(int32_t n, const void* const* src, void* const* dst, const int64_t* bytes,
                   void* stream);

/* Device-side row offsets from device-side lengths (int64, n entries -> n + 1 offsets,
 * offsets[0] = 0), so a pyramid level's segment table is built without a host round trip
 * (replaces the host-list -> device copy of fgreg.ops.offsets after grid subsampling;
 * reference: the stack_lengths / batch offsets of PreprocessorGPU,
 * finegrained_kpconv.py:422-542). One launch, asynchronous. */
int fgr_lengths_to_offsets(const int64_t* lengths, int32_t n, int64_t* offsets, void* stream);

/* ---- pose ----------------------------------------------------------------------------
 * fast_compute_rigid_transform (utils/se3_torch.py:226-273; threshold < 0 gives the
 * unthresholded compute_rigid_transform, :131-173) on n_batch independent problems
 * a, b (n_batch, n_pts, 3), w (n_batch, n_pts) -> out (n_batch, 3, 4). A problem without a
 * weight over the threshold gives R = I, t = 0 exactly (torch.svd of the zero covariance); a rank-1 covariance (collinear points) gives one of the optimal rotations. */
int fgr_procrustes(const float* a, const float* b, const float* w, int64_t n_batch, int64_t n_pts,
                   float threshold, float* out, void* stream);

/* The forward's pose stage (models/finegrained_regtr.py:198-218) straight from the
 * packed tensors: for pair p and layer l, a = [src_kp ; tgt_corr_l], b = [src_corr_l ;
 * tgt_kp], w = sigmoid([src_logit_l ; tgt_logit_l]) thresholded at `threshold`.
 * xyz (n_tot, 3) coarse points, corr (n_layers, n_tot, 3), logits (n_layers, n_tot),
 * seg_off (2*n_pairs + 1) -> out (n_layers, n_pairs, 3, 4). */
int fgr_pair_pose(const float* xyz, const float* corr, const float* logits, int64_t n_tot,
                  const int64_t* seg_off, int32_t n_pairs, int32_t n_layers, float threshold,
                  float* out, void* stream);

/* ---- test-step tail --------------------------------------------
 * What GenericRegModel.test_step runs after the forward (generic_reg_model.py:128-132),
 * on packed tensors (clouds src_0..src_{B-1}, tgt_0..tgt_{B-1}):
 *  fgr_overlap_pool     compute_overlaps, one level (finegrained_kpconv.py:560-569):
 *                       out[q] = clamp(mean_{h: idx[q,h] < n_prev} prev[idx[q,h]], 0, 1),
 *                       NaN for a row without valid entries (as the reference); a negative
 *                       index counts from the end (torch indexing), one below -n_prev is
 *                       skipped;
 *  fgr_bce_logits_mean  nn.BCEWithLogitsLoss() on x[i * stride_x] vs y[i] (:264-267);
 *  fgr_transform_points se3_transform_list (se3_torch.py:70-90): rows of segment s get
 *                       pose[s] (3 x 4), or se3_inv(pose[s]) when inverse != 0;
 *  fgr_infonce_rows     InfoNCELossFull.compute_infonce (feature_loss.py:268-296) per anchor
 *                       row, given the match logits (n_anchor, ld) over ALL positive rows
 *                       (columns of pair b: p_off[b]..p_off[b+1]): nearest positive by
 *                       torch.cdist's matrix-multiply distance (lowest index on ties),
 *                       row_mask = (its distance < r_p), points closer than r_n ignored,
 *                       row_loss = logsumexp - positive logit; a pair with no positive row
 *                       gives row_loss NaN, row_mask 0;
 *  fgr_infonce_reduce   sum(loss[mask]) / sum(mask) per pair, mean over pairs (:295, 314);
 *  fgr_circle_loss      CircleLossFull.forward (feature_loss.py:160-243) with Euclidean feature
 *                       distances (feature_loss_type: circle, finegrained_regtr.py:86-88) over
 *                       n_pairs pairs packed along rows (anchor rows a_off[b]..a_off[b+1] of
 *                       anchor_feat (n_anchor, d) / axyz, positive rows p_off[b]..p_off[b+1]);
 *                       fd_off[b] = sum_{b' < b} n_a(b') n_p(b') (int64, device), fd_elems its
 *                       total; max_anchor / max_pos the largest per-pair counts; the workspace
 *                       holds the per-pair distance matrices and per-line losses
 *                       (fgr_circle_loss_workspace bytes); out = the 0-d loss (NaN for a pair
 *                       with no row or no column holding both a positive and a negative, as
 *                       the reference's mean over an empty selection);
 *  fgr_pair_cdist       the circle loss's first stage alone: fd (packed per pair at fd_off[b],
 *                       row-major n_a(b) x n_p(b)) = sqrt(sum_k (a_ik - p_jk)^2 + 1e-12), the
 *                       reference's cdist 'euclidean' by direct differences
 *                       (feature_loss.py:11-36): the training CircleLoss forward;
 *  fgr_corr_loss        CorrCriterion('mae') for src (pose) + tgt (se3_inv(pose)) directions
 *                       with overlap weights w (corr_loss.py:18-38, finegrained_regtr.py:283-296);
 *  fgr_se3_compare      se3_compare(pred[l, b], gt[b]) (se3_torch.py:117-129) -> rotation
 *                       error in degrees and translation error, (n_layers, n_pairs) each.
 * The single-block reductions are deterministic. */
int fgr_overlap_pool(const float* prev, int64_t n_prev, const int64_t* idx, int64_t nq,
                     int32_t width, float* out, void* stream);
int fgr_bce_logits_mean(const float* x, int64_t stride_x, const float* y, int64_t n, float* out,
                        void* stream);
int fgr_transform_points(const float* xyz, int64_t n, const int64_t* seg_off, int32_t n_seg,
                         const float* pose, int32_t inverse, float* out, void* stream);
int fgr_infonce_rows(const float* logits, int64_t ld, const float* axyz, const float* pxyz,
                     const int64_t* a_off, const int64_t* p_off, int32_t n_pairs, int64_t n_anchor,
                     float r_p, float r_n, float* row_loss, float* row_mask, void* stream);
/* Training (loss.backward() through the InfoNCE above): dlogits (n_anchor, n_cols over all
 * pairs' positive rows) = grad[0] * row_weight[i] * (softmax_ij - [j == positive]) over the
 * row's pair block, ignored columns and other pairs' columns 0; row_weight[i] =
 * row_mask[i] / (kept rows of the pair * n_pairs) makes it the gradient of
 * fgr_infonce_reduce's output. The positive / ignore mask / log-sum-exp are recomputed as
 * fgr_infonce_rows does. */
int fgr_infonce_rows_bwd(const float* logits, int64_t ld, const float* axyz, const float* pxyz,
                         const int64_t* a_off, const int64_t* p_off, int32_t n_pairs,
                         int64_t n_anchor, int64_t n_cols, float r_n, const float* row_weight,
                         const float* grad, float* dlogits, int64_t ld_d, void* stream);
int fgr_infonce_reduce(const float* row_loss, const float* row_mask, const int64_t* a_off,
                       int32_t n_pairs, float* out, void* stream);
int fgr_circle_loss_workspace(int64_t fd_elems, int64_t n_anchor, int64_t n_pos, size_t* bytes);
int fgr_circle_loss(const float* anchor_feat, const float* pos_feat, int32_t d, const float* axyz,
                    const float* pxyz, const int64_t* a_off, const int64_t* p_off,
                    const int64_t* fd_off, int32_t n_pairs, int64_t n_anchor, int64_t n_pos,
                    int32_t max_anchor, int32_t max_pos, int64_t fd_elems, float r_p, float r_n,
                    void* ws, size_t ws_bytes, float* out, void* stream);
int fgr_pair_cdist(const float* anchor_feat, const float* pos_feat, int32_t d, const int64_t* a_off,
                   const int64_t* p_off, const int64_t* fd_off, int32_t n_pairs, int32_t max_anchor,
                   int32_t max_pos, float* fd, void* stream);
int fgr_corr_loss(const float* xyz, const float* corr, const float* w, const int64_t* seg_off,
                  int32_t n_pairs, const float* pose, float* out, void* stream);
int fgr_se3_compare(const float* pred, const float* gt, int32_t n_layers, int32_t n_pairs,
                    float* rot_deg, float* trans, void* stream);

/* ---- ModelNet evaluation metrics (benchmark/benchmark_modelnet.py:33-82 compute_metrics, the
 * ModelNet branch of GenericRegModel.test_step, generic_reg_model.py:138-147) -------------------
 * pred, gt (n_pairs, 3, 4) fp32 poses; src, ref (n_pairs, n_pts, 3) the input clouds; raw
 * (n_pairs, n_raw, 3) the clean reference clouds (points_raw); all contiguous.
 * out (n_pairs, 7) fp64 = r_mse, r_mae (the 'xyz' Euler angles in degrees, scipy's from_matrix
 * orthogonalisation restated), t_mse, t_mae, err_r_deg, err_t (isotropic), chamfer_dist (the
 * modified Chamfer distance over the raw cloud). Workspace: fgr_modelnet_metrics_workspace
 * bytes (the per-point squared minima). Two launches, deterministic. */
int fgr_modelnet_metrics_workspace(int32_t n_pairs, int32_t n_pts, size_t* bytes);
int fgr_modelnet_metrics(const float* pred, const float* gt, const float* src, const float* ref,
                         const float* raw, int32_t n_pairs, int32_t n_pts, int32_t n_raw, void* ws,
                         size_t ws_bytes, double* out, void* stream);

/* ---- Input side: the ModelNet crop test pipeline on the GPU ----------
 * Replaces, for a batch of samples, the geometry of data_loaders/modelnet_transforms.py
 * RandomCrop (:176-246), RandomTransformSE3_euler (:300-355), Resampler (:92-148),
 * RandomJitter (:151-173) and ShufflePoints (:374-397) as chained by
 * data_loaders/modelnet.py:111-117; the random draws stay in NumPy's stream on the host
 * (fgreg/transforms_gpu.py). Pair b's raw cloud is rows [offsets[b], offsets[b+1]) of `raw`
 * (ld floats per row, xyz first; at most fgr_crop_max_points rows); cloud 0 = source,
 * 1 = reference.
 *  fgr_crop_pairs_mask      per (pair, cloud): d = (p - mean(p)) . dirs[b, c] and the
 *                           percentile threshold (order statistics crop_k[b], crop_k[b]+1 of d,
 *                           NumPy's lerp with gamma[b]; crop_k[b] < 0: threshold 0, the
 *                           p_keep = 0.5 rule) -> mask (2, Ntot) u8, keep (2, Ntot) i32 (kept
 *                           raw indices, in order, at the pair's offset) and count (n_pairs, 2).
 *  fgr_crop_pairs_assemble  per pair: output row i of cloud c is raw row keep[c][sel[b, c, i]]
 *                           (Resampler's choice composed with ShufflePoints' permutation by
 *                           the host), the source moved by rt[b] (3x4 float32), plus
 *                           noise[b, c, i] (float64, clipped); overlap[b, c, i] = the other
 *                           cloud's mask at that raw index; corr (2, Ntot) i64 gets the
 *                           correspondence pairs (raw-index order) at the pair's offset and
 *                           n_corr[b] their count. sel must hold distinct values < count.
 * Outputs equal fgreg.transforms.modelnet_crop_test bit for bit (tests/test_gpu_transforms.py). */
int fgr_crop_max_points(int32_t* n_max);
int fgr_crop_pairs_mask(const float* raw, int32_t ld, const int64_t* offsets, int32_t n_pairs,
                        const double* dirs, const int32_t* crop_k, const double* gamma,
                        uint8_t* mask, int32_t* keep, int32_t* count, void* stream);
int fgr_crop_pairs_assemble(const float* raw, int32_t ld, const int64_t* offsets, int32_t n_pairs,
                            const uint8_t* mask, const int32_t* keep, const int32_t* sel,
                            const double* noise, const float* rt, int32_t m, float* xyz,
                            uint8_t* overlap, int64_t* corr, int32_t* n_corr, void* stream);

/* ---- Input side: the 3DMatch / MCD training augmentations on the GPU -----------------------
 * data_loaders/transforms.py RigidPerturb (:15-72), Jitter (:75-92), ShufflePoints (:95-131)
 * and RandomSwap (:134-151) as data_loaders/__init__.py:16-57 chains them, for a batch of
 * n_pairs samples; the random draws stay in the reference's streams on the host
 * (fgreg/augment.py). Every output is evaluated in float64 and rounded once.
 * Layout: the clouds are 2 n_pairs packed segments, the source of pair b (segment 2b), then
 * its target (2b + 1). in_off (2 n_pairs + 1) are their row offsets in xyz (ld floats per row,
 * xyz first), overlap (one byte per row) and noise (nullable; 3 float32 per row, already
 * scaled); n_points = in_off[2 n_pairs]. perm holds, per INPUT segment at out_off
 * (2 n_pairs + 1), the kept raw rows in output order (distinct, < the cloud's size: the caller
 * validates them); max_out >= the longest of them. corr / corr_out are (2, corr_ld) int64 with
 * pair b's columns at [corr_off[b], corr_off[b + 1]) (n_pairs + 1 offsets; corr may be NULL
 * when corr_ld is 0). pose / perturb / pose_out are (n_pairs, 3, 4) float32. flags[b] is a sum
 * of FGR_AUG_*: PERTURB (perturb[b] applies), SOURCE (to the source; else to the target),
 * CENTRE (about the perturbed cloud's centroid, C^-1 P C: the 'small' mode), SWAP.
 *   pose_out[b]    pose . P^-1 (source perturbed) or P . pose, inverted under SWAP
 *   xyz_out        row out_off[s] + i of the cloud that ends as segment s:
 *                  T raw[perm[i]] + noise[perm[i]] (T = P of the perturbed cloud, else I)
 *   overlap_out    overlap[perm[i]], same rows
 *   corr_out       the columns of corr whose two points were both kept, as output rows, in
 *                  their original order (rows exchanged under SWAP), n_corr[b] of them
 * Outputs are in post-swap order: under SWAP the target's rows come first in pair b's span
 * (and are the new source). A correspondence index outside its cloud is never dereferenced:
 * n_corr[b] = -1 for that pair. ws: fgr_augment_workspace_bytes(n_points, n_pairs) bytes,
 * 8-B aligned. Three launches on `stream`, no host sync; results are run-to-run identical. */
#define FGR_AUG_PERTURB 1
#define FGR_AUG_SOURCE 2
#define FGR_AUG_CENTRE 4
#define FGR_AUG_SWAP 8
int fgr_augment_workspace_bytes(int64_t n_points, int32_t n_pairs, size_t* bytes);
int fgr_augment_pairs(const float* xyz, int32_t ld, const int64_t* in_off, int64_t n_points,
                      const uint8_t* overlap, const int64_t* corr, int64_t corr_ld,
                      const int64_t* corr_off, const float* pose, const float* perturb,
                      const int32_t* flags, const int32_t* perm, const int64_t* out_off,
                      int32_t max_out, const float* noise, int32_t n_pairs, float* xyz_out,
                      uint8_t* overlap_out, int64_t* corr_out, int32_t* n_corr, float* pose_out,
                      void* ws, size_t ws_bytes, void* stream);

/* The pre-norm layer's in_proj with the attention's K / V images written in its epilogue
 * (transformers.py:193-196 / :213-221 + the image building of fgr_attention_f16x3, head dim 32):
 * qkv = (LayerNorm(x) * gamma + beta + add) W^T + bias as fgr_gemm_f16x3_ln, but only the q
 * columns [0, d) go to q (m, d; ld_q) as fp32 -- the k and v columns go straight into kv_img:
 * the f16x3 K / V images of every GLOBAL 64-row tile and head, then their int2 scale exponents
 * (fgr_kv_image_bytes(m, n_head, 32) bytes). Optional side output out2 = LayerNorm(x) * gamma2 +
 * beta2 as fgr_gemm_f16x3_ln_out2. fgr_gemm_f16x3_ln_qkv_supported(m, d, n_head): d = 32 n_head =
 * 256 and the row-stationary kernel for (m, 3d, d).
 * fgr_attention_f16x3_img: fgr_attention_f16x3 (head dim 32) reading those images (kv rows = the
 * same packed rows, n_kv_rows = m) instead of building its own. */
int fgr_kv_image_bytes(int64_t n_rows, int32_t n_head, int32_t head_dim, size_t* bytes);
int fgr_gemm_f16x3_ln_qkv_supported(int32_t m, int32_t d, int32_t n_head);
int fgr_gemm_f16x3_ln_qkv(const float* x, int64_t ldx, const float* gamma, const float* beta,
                          float eps, const float* add, int64_t ld_add, const void* w_img, float* q,
                          int64_t ld_q, const float* bias, int32_t m, int32_t d, int32_t n_head,
                          void* kv_img, const float* gamma2, const float* beta2, float* out2,
                          int64_t ld_out2, void* stream);
/* fgr_gemm_f16x3_qkv: the same for an in_proj without the LayerNorm prologue, head dim 64
 * (qkv = a W^T + bias, a (m, d); the staged 64 x 128-tile g5 epilogue writes the images):
 * fgr_gemm_f16x3_qkv_supported(m, d, n_head): d = 64 n_head, d % 128 == 0. fgr_kv_image_bytes
 * takes head_dim 32 or 64, fgr_attention_f16x3_img reads either. */
int fgr_gemm_f16x3_qkv_supported(int32_t m, int32_t d, int32_t n_head);
int fgr_gemm_f16x3_qkv(const float* a, int64_t lda, const void* w_img, float* q, int64_t ld_q,
                       const float* bias, int32_t m, int32_t d, int32_t n_head, void* kv_img,
                       void* stream);
/* bf16 mode: fgr_gemm_bf16_qkv writes q (fp32) and the bf16 K / V images (head dim 64, no
 * scales; fgr_kv_image_bf16_bytes) of every global 64-row tile from the register-staged 64 x
 * 128 bf16 kernel's epilogue, fgr_attention_bf16_img reads them. */
int fgr_kv_image_bf16_bytes(int64_t n_rows, int32_t n_head, int32_t head_dim, size_t* bytes);
int fgr_gemm_bf16_qkv_supported(int32_t m, int32_t d, int32_t n_head);
int fgr_gemm_bf16_qkv(const float* a, int64_t lda, const void* w_img, float* q, int64_t ld_q,
                      const float* bias, int32_t m, int32_t d, int32_t n_head, void* kv_img,
                      void* stream);
int fgr_attention_bf16_img(const float* q, int64_t ld_q, const void* kv_img, int64_t n_kv_rows,
                           float* o, int64_t ld_o, const int64_t* q_off, const int64_t* kv_off,
                           const int32_t* kv_seg, int32_t n_seg, int32_t max_q_len,
                           int32_t n_head, int32_t head_dim, float scale, void* stream);
int fgr_attention_f16x3_img(const float* q, int64_t ld_q, const void* kv_img, int64_t n_kv_rows,
                            float* o, int64_t ld_o, const int64_t* q_off, const int64_t* kv_off,
                            const int32_t* kv_seg, int32_t n_seg, int32_t max_q_len,
                            int32_t n_head, int32_t head_dim, float scale, void* stream);

/* The CorrespondenceRegressor head (finegrained_regtr.py:411-455, direct_regress_coor: True) on
 * the (m, d) stacked layer outputs f in two row-stationary f16x3 launches:
 *   hidden = ReLU(f W0^T + b0), logits = f Wc^T + bc   -- ONE product over the image of the
 *            stacked (d + 16, d) weight [W0; Wc; 0] (fgr_split_weights_h3) with bias
 *            b0c = [b0; bc; 0] (d + 16 floats); hidden (m, d) is caller scratch;
 *   corr   = ReLU(hidden W2^T + b2) W4^T + b4           -- the 3-wide coor_mlp[4] formed in the
 *            second product's epilogue from its fp32 outputs (w4 (3, d) and b4 (3) fp32).
 * corr (m, 3), logits (m) contiguous. fgr_corr_head_supported(m, d): d % 16 == 0, d <= 256;
 * other widths use fgr_gemm_f16x3 per layer. */
int fgr_corr_head_supported(int32_t m, int32_t d);
int fgr_corr_head_f16x3(const float* f, int64_t ldf, int32_t m, int32_t d, const void* w0c_img,
                        const float* b0c, const void* w2_img, const float* b2, const float* w4,
                        const float* b4, float* hidden, float* corr, float* logits, void* stream);

/* ---- Training backward (train.py -> trainer.py:110-125 backward) -------
 * The dense products' gradients run on the GEMM entry points above with transposed weight
 * images (fgreg/autograd.py); these cover the rest. Every entry point is deterministic: no
 * floating-point atomics, every reduction in a fixed order (ABI 2; ABI 1's two scatters added
 * with fp32 atomics).
 *  fgr_nbr_inverse      the inverse (CSR) of an (nq, width) neighbour table over ns support rows:
 *                       start[ns + 1], and for support row s the entries e = q * width + h with
 *                       idx[e] == s in ascending e at ent[start[s] .. start[s + 1]); pos[e] = the
 *                       CSR slot of entry e, -1 where idx[e] names no support row (shadow index
 *                       / negative). ent and pos hold nq * width ints; workspace
 *                       fgr_nbr_inverse_workspace bytes. Built once per table, read by both
 *                       scatters below (the reference's gather(method=2) transpose,
 *                       finegrained_kpconv_blocks.py:66-97, as a gather over the inverse).
 *  fgr_kpconv_scatter   KPConv gather-weight backward: dx[s, c] = sum over the entries (q, h)
 *                       naming s, in CSR order, of sum_k w(q,h,k) dwf[q,k,c] with the forward's
 *                       influences (finegrained_kpconv_blocks.py:296-381). dx (ns, cin) is
 *                       WRITTEN (rows nobody names get 0); start / pos from fgr_nbr_inverse of
 *                       idx; workspace fgr_kpconv_scatter_workspace bytes (one cin-row per
 *                       table entry).
 *  fgr_max_pool_bwd     max_pool (:125-141): dx[s, c] = sum of dy[q, c] over the entries (q, h)
 *                       naming s whose slot h is the row's first maximum of channel c (shadow
 *                       entries read 0 and pass nothing on). dx (ns, c) is WRITTEN; start / ent
 *                       from fgr_nbr_inverse of idx; workspace fgr_max_pool_bwd_workspace.
 *  fgr_segnorm_stats    per-(segment, channel) mean / rstd / biased var of v = x / row_div:
 *                       InstanceNorm1d per cloud (:498-507) or BatchNorm1d batch statistics
 *                       (one segment, res2net.py:126-159 in train()); workspace
 *                       fgr_segnorm_workspace bytes.
 *  fgr_segnorm_apply    out = post(act((v - mean) rstd (* gamma + beta)) + residual).
 *  fgr_segnorm_bwd      its backward from (y = out, dy): dx, dres (= d residual), dgamma / dbeta
 *                       (NULL without gamma); workspace fgr_segnorm_workspace + 8 n_seg c bytes.
 *  fgr_layernorm_bwd    nn.LayerNorm backward (transformers.py:105-107): dx, and
 *                       dgamma_dbeta[0..d) = sum dy xhat, [d..2d) = sum dy; d <= 1024.
 *  fgr_colsum           out[c] = sum_r x[r, c] (fp64 partials; bias gradients).
 *  fgr_attention_bwd    softmax attention backward over packed segments (the layout of
 *                       fgr_attention*): dq, dk, dv (each may alias column slices of one
 *                       tensor), head dim 4 / 8 / 16 / 32 / 64, fp32; key segments may be attended by any
 *                       number of query segments; the rows of a key segment that no query
 *                       segment attends get dk = dv = 0. A non-empty query segment whose key
 *                       segment is empty (a softmax over nothing) is undefined, here and in
 *                       every attention entry point.
 *  fgr_corr_attention_bwd  backward of fgr_corr_attention (CorrespondenceDecoder.simple_attention,
 *                       finegrained_regtr.py:328-363): from dout (n_rows, 3) = d corr, writes
 *                       dq = scale dS K and dk = scale dS^T Q (dS = P (dout . xyz_j - dout .
 *                       corr_i)) over the same segment tables; xyz gets no gradient (the
 *                       reference's values are coordinates). Key rows no query segment attends
 *                       get dk = 0; d 32 / 64 / 128 / 256 / 512, fp32; workspace
 *                       fgr_corr_attention_bwd_workspace(n_rows) bytes. */
int fgr_nbr_inverse_workspace(int64_t nq, int32_t width, int64_t ns, size_t* bytes);
int fgr_nbr_inverse(const int64_t* idx, int64_t nq, int32_t width, int64_t ns, int32_t* start,
                    int32_t* pos, int32_t* ent, void* ws, size_t ws_bytes, void* stream);
int fgr_kpconv_scatter_workspace(int64_t nq, int32_t width, int32_t cin, size_t* bytes);
int fgr_kpconv_scatter(const float* q, const float* s, int64_t nq, int64_t ns, const int64_t* idx,
                       int32_t width, const float* dwf, int32_t cin, const float* kernel_points,
                       int32_t n_kp, float extent, const int32_t* start, const int32_t* pos,
                       float* dx, void* ws, size_t ws_bytes, void* stream);
/* fgr_kpconv_scatter with the influences of fgr_kpconv_gather_mode (FGR_KP_*, FGR_AGG_*): the
 * same arguments, workspace and refusals; fgr_kpconv_scatter is its (0, 0) case */
int fgr_kpconv_scatter_mode(const float* q, const float* s, int64_t nq, int64_t ns,
                            const int64_t* idx, int32_t width, const float* dwf, int32_t cin,
                            const float* kernel_points, int32_t n_kp, float extent,
                            int32_t influence, int32_t aggregation, const int32_t* start,
                            const int32_t* pos, float* dx, void* ws, size_t ws_bytes,
                            void* stream);
int fgr_max_pool_bwd_workspace(int64_t nq, int32_t c, size_t* bytes);
int fgr_max_pool_bwd(const float* x, int64_t ns, int32_t c, const int64_t* idx, int64_t nq,
                     int32_t width, const float* dy, const int32_t* start, const int32_t* ent,
                     float* dx, void* ws, size_t ws_bytes, void* stream);
int fgr_corr_attention_bwd_workspace(int64_t n_rows, size_t* bytes);
int fgr_corr_attention_bwd(const float* q, int64_t ld_q, const float* k, int64_t ld_k,
                           const float* xyz, const float* dout, float* dq, int64_t ld_dq, float* dk,
                           int64_t ld_dk, const int64_t* q_off, const int64_t* kv_off,
                           const int32_t* kv_seg, const int64_t* v_off, int32_t n_seg,
                           int32_t n_kv_seg, int64_t n_rows, int32_t max_q_len, int32_t max_kv_len,
                           int32_t d, float scale, void* ws, size_t ws_bytes, void* stream);
int fgr_segnorm_workspace(int64_t max_seg_len, int32_t c, int32_t n_seg, size_t* bytes);
int fgr_segnorm_stats(const float* x, int64_t n, int32_t c, const int64_t* seg_off, int32_t n_seg,
                      int64_t max_seg_len, const float* row_div, float eps, float* mean, float* rstd,
                      float* var, void* ws, size_t ws_bytes, void* stream);
int fgr_segnorm_apply(const float* x, int64_t n, int32_t c, const int64_t* seg_off, int32_t n_seg,
                      const float* row_div, const float* mean, const float* rstd, const float* gamma,
                      const float* beta, int32_t act, const float* residual, int32_t post_act,
                      float* out, void* stream);
/* fgr_segnorm_stats then fgr_segnorm_apply in one call (the training forward). */
int fgr_segnorm_fwd(const float* x, int64_t n, int32_t c, const int64_t* seg_off, int32_t n_seg,
                    int64_t max_seg_len, const float* row_div, float eps, float* mean, float* rstd,
                    float* var, const float* gamma, const float* beta, int32_t act,
                    const float* residual, int32_t post_act, float* out, void* ws, size_t ws_bytes,
                    void* stream);
int fgr_segnorm_bwd(const float* x, int64_t n, int32_t c, const int64_t* seg_off, int32_t n_seg,
                    int64_t max_seg_len, const float* row_div, const float* mean, const float* rstd,
                    const float* gamma, const float* beta, int32_t act, int32_t has_residual,
                    int32_t post_act, const float* y, const float* dy, float* dx, float* dres,
                    float* dgamma, float* dbeta, void* ws, size_t ws_bytes, void* stream);
int fgr_colsum_workspace(int64_t n, int32_t c, size_t* bytes);
int fgr_colsum(const float* x, int64_t n, int32_t c, int64_t ldx, float* out, void* ws,
               size_t ws_bytes, void* stream);
int fgr_layernorm_bwd_workspace(int64_t n, int32_t d, size_t* bytes);
int fgr_layernorm_bwd(const float* x, int64_t n, int32_t d, const float* gamma, float eps,
                      const float* dy, float* dx, float* dgamma_dbeta, void* ws, size_t ws_bytes,
                      void* stream);
int fgr_attention_bwd_workspace(int64_t nq, int32_t nhead, size_t* bytes);
int fgr_attention_bwd(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v,
                      int64_t ldv, const float* o, int64_t ldo, const float* dout, int64_t lddo,
                      float* dq, int64_t lddq, float* dk, int64_t lddk, float* dv, int64_t lddv,
                      const int64_t* q_off, const int64_t* kv_off, const int32_t* kv_seg,
                      int32_t n_seg, int32_t n_kv_seg, int64_t nq, int64_t max_q_len,
                      int64_t max_kv_len, int32_t nhead, int32_t dh, float scale, void* ws,
                      size_t ws_bytes, void* stream);
/* Training with nn.MultiheadAttention(dropout = p > 0): the same forward / backward with the
 * attention weights of the PV product dropped by a counter-based hash of (seed, head, query
 * row, key row) -- kept with probability 1 - p and scaled by 1 / (1 - p), the softmax sum
 * over every weight (transformers.py:95-96; common.h attn_drop_hash). The backward with the
 * same seed / p reproduces the forward's mask; head dim 16 / 32 / 64 (the forward: 32 / 64),
 * 16-B aligned rows; the backward refuses p > 0 on any other shape (FGR_E_ARG, nothing
 * written). Masks are not torch's Philox draws (same distribution). A (row, head) whose every
 * weight is dropped gives o = 0 and contributes exactly 0 to dq, dk and dv. */
int fgr_attention_f16x3_drop(const float* q, int64_t ld_q, const float* k, int64_t ld_k,
                             const float* v, int64_t ld_v, float* o, int64_t ld_o,
                             const int64_t* q_off, const int64_t* kv_off, const int32_t* kv_seg,
                             int32_t n_seg, int32_t n_kv_seg, int64_t n_kv_rows, int32_t max_q_len,
                             int32_t max_kv_len, int32_t n_head, int32_t head_dim, float scale,
                             void* workspace, int64_t ws_bytes, uint32_t seed, float p,
                             void* stream);
/* Training pair (dropout p >= 0 as the _drop pair): the forward also writes, per (row, head),
 * the log2-sum-exp of the scaled scores to lse (n_rows * n_head floats); the backward reads it
 * back and skips its own max / sum pass over the keys (head dim 16 / 32 / 64, 16-B aligned
 * rows; other shapes recompute it and ignore lse). With p > 0 the lse is still that of the
 * undropped softmax. */
int fgr_attention_f16x3_train(const float* q, int64_t ld_q, const float* k, int64_t ld_k,
                              const float* v, int64_t ld_v, float* o, int64_t ld_o,
                              const int64_t* q_off, const int64_t* kv_off, const int32_t* kv_seg,
                              int32_t n_seg, int32_t n_kv_seg, int64_t n_kv_rows, int32_t max_q_len,
                              int32_t max_kv_len, int32_t n_head, int32_t head_dim, float scale,
                              void* workspace, int64_t ws_bytes, uint32_t seed, float p, float* lse,
                              void* stream);
int fgr_attention_bwd_train(const float* q, int64_t ldq, const float* k, int64_t ldk,
                            const float* v, int64_t ldv, const float* o, int64_t ldo,
                            const float* dout, int64_t lddo, float* dq, int64_t lddq, float* dk,
                            int64_t lddk, float* dv, int64_t lddv, const int64_t* q_off,
                            const int64_t* kv_off, const int32_t* kv_seg, int32_t n_seg,
                            int32_t n_kv_seg, int64_t nq, int64_t max_q_len, int64_t max_kv_len,
                            int32_t nhead, int32_t dh, float scale, void* ws, size_t ws_bytes,
                            uint32_t seed, float p, const float* lse, int64_t n_kv_rows,
                            void* stream);
/* fgr_attention_bwd_train's workspace over nq query rows in n_seg segments and n_kv_rows packed
 * key rows in n_kv_seg segments: lse / D per (row, head) and, at head dim 32 / 64, the K / V /
 * Q / dO tile images of the dQ and dK / dV kernels on the f16 matrix cores (split-fp16 x3
 * products, as fgr_attention_f16x3). A workspace of fgr_attention_bwd_workspace's size runs the
 * fp32-MFMA kernels instead. */
int fgr_attention_bwd_train_workspace(int64_t nq, int32_t n_seg, int64_t n_kv_rows,
                                      int32_t n_kv_seg, int32_t nhead, int32_t dh, size_t* bytes);
int fgr_attention_bwd_drop(const float* q, int64_t ldq, const float* k, int64_t ldk,
                           const float* v, int64_t ldv, const float* o, int64_t ldo,
                           const float* dout, int64_t lddo, float* dq, int64_t lddq, float* dk,
                           int64_t lddk, float* dv, int64_t lddv, const int64_t* q_off,
                           const int64_t* kv_off, const int32_t* kv_seg, int32_t n_seg,
                           int32_t n_kv_seg, int64_t nq, int64_t max_q_len, int64_t max_kv_len,
                           int32_t nhead, int32_t dh, float scale, void* ws, size_t ws_bytes,
                           uint32_t seed, float p, void* stream);

/* Weight gradient of a dense product, dW = dY^T X (every nn.Linear / KPConv weight of the
 * backward, trainer.py:110-125), read straight from the two row-major activations:
 *   dw[i][j] = sum_{r < rows} dy[r * ld_dy + i] * x[r * ld_x + j]      (i < m, j < n)
 * and, when db is not NULL, the bias gradient db[i] = sum_r dy[r * ld_dy + i] (fp64 sums).
 * fp32-accurate (f16x3: per-chunk column scales, three fp16 products, fp32 accumulation);
 * m, n, the row strides and ld_dw multiples of 4, dy / x / dw 16-B aligned. Rows are split
 * into chunks whose partials are summed in chunk order (deterministic); the workspace
 * fgr_gemm_wgrad_workspace(rows, m, n, db != NULL) bytes holds them (0 when one chunk
 * suffices). rows == 0 writes zeros. */
int fgr_gemm_wgrad_workspace(int64_t rows, int32_t m, int32_t n, int32_t with_bias, size_t* bytes);
int fgr_gemm_f16x3_wgrad(const float* dy, int64_t ld_dy, const float* x, int64_t ld_x,
                         int64_t rows, int32_t m, int32_t n, float* dw, int64_t ld_dw, float* db,
                         void* ws, size_t ws_bytes, void* stream);

/* ---- pose refinement on the full clouds: point-to-point ICP, fitness, information -------
 * Not part of the reference: the step its consumers run after the forward (a pose graph over
 * fragments, RRE / RTE on dense points). Pair b matches source segment b, rows
 * [src_off[b], src_off[b + 1]) of src (n_src_tot, 3), against target segment b of tgt
 * (n_tgt_tot, 3); poses are (n_pairs, 3, 4) fp32, source -> target.
 *
 * One association pass under a pose T = [R | t]: for every source point p,
 *   qx = ((R00 px + R01 py) + R02 pz) + tx   (fp32, no FMA; qy, qz likewise),
 * the nearest target s by d2 = ((qx-sx)^2 + (qy-sy)^2) + (qz-sz)^2 (as fgr_radius_search; the
 * lowest target row on an exact tie) is its correspondence iff d2 < max_dist * max_dist
 * (fp32, strict). The targets are binned once per call into the cell grid of
 * fgr_radius_grid_build at radius max_dist and each query scans the 27 cells around it.
 * Over the inliers, in fp64 and in a fixed order (no floating-point atomics):
 *   fitness = n_inl / n_src, rmse = sqrt(sum d2 / n_inl)   (stored as fp32; 0 when n_inl = 0).
 *
 * fgr_icp iterates on the device, per pair: pass k = 0, 1, ... associates under T_k and gives
 * (f_k, e_k). The pair is done when k >= 1 and |f_k - f_(k-1)| < rel_fitness and
 * |e_k - e_(k-1)| < rel_rmse (fp64), or n_inl < 3, or k == max_iters. Otherwise
 *   H = sum p s^T - (sum p)(sum s)^T / n_inl, R = V U^T of H's SVD (det +1), t = mean s - R mean p
 * (p the untransformed source point) becomes T_(k+1), rounded to fp32, and n_iters = k + 1. A
 * done pair is frozen: pose_out, fitness, rmse (both of pose_out) and n_iters (int32) no longer
 * change. max_iters + 1 passes are enqueued whatever the data: no readback, allocation or
 * synchronisation, so a call can be captured into a graph. An empty source or target returns
 * pose_in, fitness 0, rmse 0, n_iters 0. pose_out must not overlap pose_in.
 *
 * fgr_registration_score is one pass under `pose`: fitness, rmse and, each where not NULL,
 * idx (n_src_tot) int32 = the correspondence's row inside its target segment or -1,
 * d2 (n_src_tot) fp32 = its d2 or +inf, and info (n_pairs, 6, 6) fp64 =
 *   sum over the inliers of J^T J, J = [I3 | -[s]x], s the matched target point,
 * translation first (info[0][0] = n_inl), exactly symmetric.
 *
 * Both take fgr_icp_workspace() bytes (the target grid, per-block fp64 partial sums, per-pair
 * state) and refuse a shorter workspace before anything is launched or written.
 * 4 n_tgt_tot + 1024 n_pairs and n_src_tot stay below 2^31, n_pairs <= 65535; max_src_len >=
 * the longest source segment. */
int fgr_icp_workspace(int64_t n_src_tot, int64_t n_tgt_tot, int32_t n_pairs, size_t* bytes);
int fgr_icp(const float* src, const int64_t* src_off, int64_t n_src_tot, const float* tgt,
            const int64_t* tgt_off, int64_t n_tgt_tot, int32_t n_pairs, int32_t max_src_len,
            const float* pose_in, float max_dist, int32_t max_iters, float rel_fitness,
            float rel_rmse, void* ws, size_t ws_bytes, float* pose_out, float* fitness,
            float* rmse, int32_t* n_iters, void* stream);
int fgr_registration_score(const float* src, const int64_t* src_off, int64_t n_src_tot,
                           const float* tgt, const int64_t* tgt_off, int64_t n_tgt_tot,
                           int32_t n_pairs, int32_t max_src_len, const float* pose,
                           float max_dist, void* ws, size_t ws_bytes, float* fitness, float* rmse,
                           int32_t* idx, float* d2, double* info, void* stream);

/* ---- surface normals and point-to-plane ICP ----------------------------------------------
 * fgr_estimate_normals: pts (n_tot, 3) fp32 packed, off (n_clouds + 1) device row offsets,
 * view (n_clouds, 3) fp32 per-cloud viewpoints or NULL = the origin. The cloud is binned with
 * the grid of fgr_radius_grid_build at `radius`. For every point p:
 *   neighbourhood = the points s of p's cloud with ((sx-px)^2 + (sy-py)^2) + (sz-pz)^2 < r2,
 *     r2 = radius * radius (fp32, strict; p itself is one of them);
 *   d = s - p in fp32; n = the count, sum d and sum d d^T in fp64 (a product of two fp32 values
 *     is exact in fp64, only the sums round); C = sum d d^T / n - (sum d / n)(sum d / n)^T;
 *   n < 3: the normal is (0, 0, 0) and is not counted. Otherwise it is the unit eigenvector of
 *     C's smallest eigenvalue (fp64 cyclic Jacobi; the lowest index among equal eigenvalues),
 *     flipped so that normal . (view - p) >= 0 in fp64 and, where that product is exactly 0,
 *     so that its first non-zero component is positive; stored as fp32.
 * normals (n_tot, 3) fp32; n_valid (n_clouds) int32 = the points of the cloud with a non-zero
 * normal. The members of each grid cell are put into ascending row order first, so the sums
 * are taken in one order: the same bits every run. No floating-point atomics, no readback,
 * allocation or synchronisation: a call can be captured into a graph. It takes exactly
 * fgr_estimate_normals_workspace() bytes and refuses a shorter workspace before anything is
 * launched or written. 4 n_tot + 1024 n_clouds stays below 2^31, n_clouds <= 65535.
 *
 * fgr_icp_plane: the arguments, association, fitness, rmse, stopping rule and freezing of
 * fgr_icp, with tgt_normals (n_tgt_tot, 3) fp32 (of fgr_estimate_normals, or the caller's own
 * unit normals) and the point-to-plane update. Per pass under T_k, for every source point:
 *   q = T_k p and its nearest target s exactly as fgr_icp (d2 < max_dist^2 a candidate); a
 *   candidate whose target has the normal (0, 0, 0) is no inlier (no other target is tried);
 *   in fp64 from the fp32 q, s, n: rho = n . (q - s), a = [n | q x n] (translation first).
 * Over the inliers, in fp64 and in fgr_icp's fixed order: n_inl, sum d2, sum rho^2,
 *   A = sum a a^T (6 x 6), g = sum a rho.
 *   fitness = n_inl / n_src, rmse = sqrt(sum d2 / n_inl) (the point-to-point distance, so the
 *   two methods' outputs compare), plane_rmse = sqrt(sum rho^2 / n_inl), all stored as fp32.
 * The pair is done, in this order of precedence, with status
 *   0 converged: k >= 1 and |f_k - f_(k-1)| < rel_fitness and |e_k - e_(k-1)| < rel_rmse;
 *   2 n_inl < 6;
 *   3 singular: the fp64 Cholesky of A meets a pivot <= 1e-12 trace(A) (one plane, or two
 *     parallel ones);
 *   1 k == max_iters.
 * Otherwise A x = -g, x = (t, w); dR = exp([w]x) by Rodrigues in fp64 (I + [w]x + [w]x^2 / 2
 * for |w| < 1e-12); T_(k+1) = [dR R_k | dR t_k + t], computed in fp64 from the stored fp32 T_k
 * and rounded to fp32; n_iters = k + 1. A done pair is frozen at the pose of its last
 * completed update. status (n_pairs) int32 and info (n_pairs, 6, 6) fp64 are written where
 * not NULL: info = A of the last pass run, the returned pose's, full and exactly symmetric. It
 * is the point-to-plane information, not the Redwood gt.info matrix of
 * fgr_registration_score. max_iters + 1 passes are enqueued whatever the data: no readback,
 * allocation or synchronisation. It takes exactly fgr_icp_plane_workspace() bytes; the size
 * limits are fgr_icp's. */
int fgr_estimate_normals_workspace(int64_t n_tot, int32_t n_clouds, size_t* bytes);
int fgr_estimate_normals(const float* pts, const int64_t* off, int64_t n_tot, int32_t n_clouds,
                         float radius, const float* view, void* ws, size_t ws_bytes,
                         float* normals, int32_t* n_valid, void* stream);
int fgr_icp_plane_workspace(int64_t n_src_tot, int64_t n_tgt_tot, int32_t n_pairs,
                            size_t* bytes);
int fgr_icp_plane(const float* src, const int64_t* src_off, int64_t n_src_tot, const float* tgt,
                  const int64_t* tgt_off, int64_t n_tgt_tot, const float* tgt_normals,
                  int32_t n_pairs, int32_t max_src_len, const float* pose_in, float max_dist,
                  int32_t max_iters, float rel_fitness, float rel_rmse, void* ws,
                  size_t ws_bytes, float* pose_out, float* fitness, float* rmse,
                  float* plane_rmse, int32_t* n_iters, int32_t* status, double* info,
                  void* stream);

/* ---- robust pose: RANSAC over putative correspondences -----------------------------------
 * The estimator between the forward's correspondences and fgr_icp (the reference ships an
 * unreachable one, models/ransaclib; this is not a port of it). a, b are (n_tot, 3) packed
 * correspondences with b ~ R a + t, w (n_tot) their weights or NULL, off (n_pairs + 1) device
 * row offsets; pair p owns rows [off[p], off[p + 1]).
 *
 * Eligibility: row i is eligible iff w == NULL or w[i] > w_min (strict; a NaN weight is not).
 *   m = n_eligible[p]; the eligible rows keep their order, a rank is a position in that order.
 * Sampling: hypothesis h of pair p draws the ranks
 *   r_k = ((uint64) hash(seed, k, p, h) * m) >> 32,  k = 0, 1, 2,
 *   hash = the counter-based hash of the attention dropout (csrc/common.h attn_drop_hash with
 *   head = k, q = p, k = h; restated by fgreg.autograd). Two equal ranks, or m < 3, make the
 *   hypothesis invalid: hyp_count = -1, hyp_pose = identity, it never wins.
 * Minimal solve, fp64: centroids am = ((a0 + a1) + a2) / 3 and bm, H = sum (a - am)(b - bm)^T,
 *   R = V U^T of H's SVD with the reflection fix (det +1), t = bm - R am, rounded once to an
 *   fp32 (3, 4) pose. A collinear sample is valid and gets one of the optimal rotations, as
 *   fgr_procrustes.
 * Score: the number of eligible rows with d2 < r2, all fp32 without FMA,
 *   qx = ((R00 x + R01 y) + R02 z) + tx (qy, qz likewise), d = q - b,
 *   d2 = ((dx dx) + dy dy) + dz dz, r2 = inlier_dist * inlier_dist (as fgr_icp's pass).
 * Selection: the largest count wins, ties go to the lowest h -> best_hyp. Without a valid
 *   hypothesis: best_hyp = -1, pose = identity, n_inliers = 0, inlier_rmse = 0, n_updates = 0,
 *   mask all 0.
 * Refits, at most n_refits, from the winner (T, c): K = {eligible i : d2_T(i) < r2}; stop if
 *   |K| < 3; T' = the fp64 unweighted Kabsch over K (sums in a fixed order, no floating-point
 *   atomics) rounded to fp32; c' = the count under T'; if c' < c stop and keep T; otherwise
 *   adopt T' and ++n_updates; if c' == c stop, else c = c' and repeat.
 * Outputs, under the final T: pose (n_pairs, 3, 4), n_inliers, inlier_rmse =
 *   fp32(sqrt(sum d2 / n_inliers)) with the sum in fp64 (0 without inliers), n_eligible,
 *   best_hyp, n_updates (all (n_pairs), int32 but the rmse); each where not NULL: inlier_mask
 *   (n_tot) in the caller's row order, 1 = inlier, 0 otherwise and for ineligible rows;
 *   hyp_pose (n_pairs, n_hyp, 3, 4) and hyp_count (n_pairs, n_hyp), every hypothesis's pose
 *   and score.
 * FGR_E_ARG, with nothing launched or written: n_pairs outside 1..65535, n_hyp outside
 * 1..2^20, n_refits < 0, inlier_dist not finite or <= 0, n_tot outside 0..2^31 - 1, a NULL
 * required pointer (a, b may be NULL when n_tot == 0), ws not 16-B aligned, ws_bytes below
 * fgr_ransac_workspace() (the compacted rows and one 64-B slot per 256 hypotheses and pair;
 * exactly the bytes used). Three launches on `stream`, whatever the data: no readback,
 * allocation or synchronisation, so a call can be captured into a graph. */
int fgr_ransac_workspace(int64_t n_tot, int32_t n_pairs, int32_t n_hyp, size_t* bytes);
int fgr_ransac_pose(const float* a, const float* b, const float* w, int64_t n_tot,
                    const int64_t* off, int32_t n_pairs, float w_min, float inlier_dist,
                    int32_t n_hyp, uint32_t seed, int32_t n_refits, void* ws, size_t ws_bytes,
                    float* pose, int32_t* n_inliers, float* inlier_rmse, int32_t* n_eligible,
                    int32_t* best_hyp, int32_t* n_updates, uint8_t* inlier_mask, float* hyp_pose,
                    int32_t* hyp_count, void* stream);

/* ---- robust pose: seeds from spatial compatibility ----------------------------------------
 * The estimator for few inliers (3-5 %: descriptor matches of low-overlap pairs), where a
 * uniform 3-point sample is all-inlier with probability p^3 and fgr_ransac_pose would need
 * hundreds of thousands of hypotheses. Two correct correspondences preserve the distance
 * between their points, so the inliers form a dense clique of the compatibility graph, and a
 * seed from it yields an all-inlier sample without a draw (the first- and second-order measure
 * of SC2-PCR, reduced to its integer core). a, b, w, off and the eligibility are
 * fgr_ransac_pose's: row i is eligible iff w == NULL or w[i] > w_min, m = n_eligible[p], the
 * eligible rows keep their order and a rank is a position in that order. max_len is the
 * caller's bound on a pair's row count; it sizes the workspace and the launches. A pair with
 * more than max_len eligible rows gets no seed (best_seed = -1, row_score = -1).
 *
 * First order, for ranks i != j, all fp32 without FMA:
 *   dx = ax_i - ax_j (dy, dz likewise), l2 = ((dx dx) + dy dy) + dz dz, la = sqrt(l2)
 *   correctly rounded; lb the same from b; SC_ij = |la - lb| < compat_dist (a NaN makes it 0),
 *   SC_ii = 0. Symmetric by construction ((x - y)^2 == (y - x)^2 exactly). Stored as bits, one
 *   row per rank in 64-bit words; bits past m are 0.
 * Second order: c_ij = popcount(row_i & row_j), s_i = sum_j SC_ij c_ij in int32 (<= m^2).
 *   row_score (n_tot, may be NULL), in the caller's row order: s_i, and -1 on ineligible rows.
 * Seeds: the min(n_seeds, m) ranks with the largest s, ties to the lowest rank, in that order:
 *   seed position q = 0, 1, .. seed_row (n_pairs, n_seeds; may be NULL): the seed's row index
 *   within its pair in the caller's numbering, -1 in unused positions.
 * Consensus set of seed i: i and the at most k - 1 ranks j with SC_ij = 1 and the largest c_ij,
 *   ties to the lowest j. Fewer than 3 members (or an unused position) make the seed invalid:
 *   seed_count = -1, seed_pose = identity, it never wins.
 * Solve: the unweighted fp64 Kabsch over the members with the moments of fgr_ransac_pose's
 *   refit -- n, sum a, sum b, sum a b^T, H = sum a b^T - (sum a)(sum b)^T / n, summed in a
 *   fixed order without floating-point atomics -- R = V U^T of H's SVD with the reflection fix,
 *   t = bm - R am, rounded once to an fp32 (3, 4) pose.
 * Score, selection, refits and outputs are fgr_ransac_pose's with the seed position in the
 *   place of h: the count of eligible rows with d2 < r2 (fp32 without FMA, r2 = inlier_dist *
 *   inlier_dist); the largest count wins, ties go to the earliest position -> best_seed;
 *   without a valid seed best_seed = -1, pose = identity, n_inliers = 0, inlier_rmse = 0,
 *   n_updates = 0, mask all 0; at most n_refits refits with the same adopt / stop rules; pose,
 *   n_inliers, inlier_rmse, n_eligible, n_updates, inlier_mask as there. Each where not NULL:
 *   seed_pose (n_pairs, n_seeds, 3, 4) and seed_count (n_pairs, n_seeds), every position's
 *   pose and score.
 * FGR_E_ARG, with nothing launched or written: n_pairs outside 1..65535, n_tot outside
 * 0..2^31 - 1, max_len outside 0..8192, n_seeds outside 1..1024, k outside 3..256,
 * n_refits < 0, compat_dist or inlier_dist not finite or <= 0, a NULL required pointer (a, b
 * may be NULL when n_tot == 0), ws not 16-B aligned, ws_bytes below fgr_compat_workspace() (a
 * function of (n_tot, n_pairs, max_len, n_seeds) only: the compacted rows, their row indices
 * and scores, n_tot rows of bits at max_len's stride, one rank and one 64-B slot per seed;
 * exactly the bytes used). Six launches on `stream`, whatever the data: no readback,
 * allocation, synchronisation or floating-point atomic (s_i is summed by integer atomics,
 * which no order changes), so two runs give the same bits and a call can be captured into a
 * graph. */
int fgr_compat_workspace(int64_t n_tot, int32_t n_pairs, int32_t max_len, int32_t n_seeds,
                         size_t* bytes);
int fgr_compat_pose(const float* a, const float* b, const float* w, int64_t n_tot,
                    const int64_t* off, int32_t n_pairs, int32_t max_len, float w_min,
                    float compat_dist, float inlier_dist, int32_t n_seeds, int32_t k,
                    int32_t n_refits, void* ws, size_t ws_bytes, float* pose,
                    int32_t* n_inliers, float* inlier_rmse, int32_t* n_eligible,
                    int32_t* best_seed, int32_t* n_updates, uint8_t* inlier_mask,
                    int32_t* row_score, int32_t* seed_row, float* seed_pose, int32_t* seed_count,
                    void* stream);

/* ---- feature matching: nearest neighbours in descriptor space, then correspondences --------
 * The second source of correspondences beside the regressed coordinates (the reference ships
 * the GeoTransformer utilities for it, models/ransaclib/registration_utils.py; this is not a
 * port of them). Both entry points are one launch on `stream`, whatever the data, without
 * workspace, atomics, readback, allocation or synchronisation: two runs give the same bits and
 * a call can be captured into a graph.
 *
 * fgr_feature_nn: q (n_q_rows, d) and k (n_k_rows, d) are dense fp32 rows, 16-B aligned;
 * q_off, kv_off (n_seg + 1 each) and kv_seg (n_seg) are the segment tables of the
 * cross-attention. Query row r lies in segment s (q_off[s] <= r < q_off[s + 1]); its keys are
 * the rows kv_off[kv_seg[s]] .. kv_off[kv_seg[s] + 1) of k, numbered j = 0, 1, .. from the
 * start of that key segment. max_q_len bounds the query segments' lengths.
 * Score of key j:  s_j = q_r . k_j                  (FGR_MATCH_DOT)
 *                  s_j = q_r . k_j - |k_j|^2 / 2    (FGR_MATCH_EUCLID: the arg-max of the score
 *                  is the arg-min of |q_r - k_j|^2; |q_r|^2 never enters a comparison).
 * Precision: always the fp32-accurate f16x3 split product, whatever the GEMM mode (as
 *   fgr_pos_mlp_f16x3): every query and key row is scaled by an exact power of two of its own
 *   (its max |x| into [2^14, 2^15)), split in two fp16 terms, multiplied on the fp16 matrix
 *   cores with fp32 accumulation, and the fp32 product is unscaled exactly; |k_j|^2 and |q_r|^2
 *   are fp32 sums over the fp32 rows. Multiplying every row by a power of two therefore changes
 *   no index and scales best / second exactly.
 * nn_idx[r]: the arg-max j. On bit-equal scores the LOWEST index wins, in every merge (within
 *   a lane, across lanes, across key tiles). -1 when the key segment is empty.
 * best[r], second[r] (second may be NULL): DOT: the best and the second-best score (a
 *   duplicate of the best counts as second); EUCLID: the squared distances
 *   max(0, |q_r|^2 - 2 s) of the two. With fewer than two keys second is -inf (DOT) or +inf
 *   (EUCLID); with none so is best.
 * FGR_E_ARG, with nothing launched or written: d refused by fgr_feature_nn_supported (1 iff
 * d % 32 == 0 and 32 <= d <= 512), a metric other than the two, n_seg outside 1..65535, row
 * counts outside 0..2^31 - 1, max_q_len outside 0..n_q_rows, a NULL table or required operand,
 * q or k not 16-B aligned. n_q_rows == 0 or max_q_len == 0 returns FGR_OK and touches nothing.
 * Writes exactly the n_q_rows elements of each output.
 *
 * fgr_match_pairs: nn_idx, best, second (n_rows each) are fgr_feature_nn's results on a packed
 * batch laid out as the forward packs it -- off (2 n_pairs + 1): segments 0 .. n_pairs - 1 are
 * the source clouds, n_pairs .. 2 n_pairs - 1 the targets, kv_seg[c] = (c + n_pairs) %
 * (2 n_pairs) -- and xyz (n_rows, 3) the packed coordinates. Pair p owns the output rows
 * out_off[p] .. out_off[p] + ns + nt (out_off: n_pairs + 1 offsets) of a, b (n_tot, 3) and w
 * (n_tot), in the row layout of fgreg.robust.correspondences:
 *   source rows first:  row i       a = src_xyz[i],       b = tgt_xyz[nn(i)]
 *   then target rows:   row ns + j  a = src_xyz[nn(j)],   b = tgt_xyz[j].
 * A row without a neighbour (nn = -1 or outside the opposite cloud) gets zeros for the missing
 * point and w = 0. Weights are 0 / 1:
 *   FGR_MATCH_SRC        1 on the source rows, 0 on the target rows;
 *   FGR_MATCH_MUTUAL     1 on source row i iff nn_tgt[nn_src[i]] == i, 0 on every target row
 *                        (each mutual pair appears once);
 *   FGR_MATCH_BILATERAL  1 on every row.
 * With max_ratio > 0 a row also needs best < (max_ratio * max_ratio) * second in fp32 (Lowe's
 * test on the EUCLID squared distances; best and second are then required). No compaction:
 * rows that do not take part carry weight 0, which fgr_ransac_pose skips.
 * n_match[p] = the number of w = 1 rows. With gt_pose ((n_pairs, 3, 4), together with
 * n_inlier) n_inlier[p] counts the w = 1 rows with d2 < r2, all fp32 without FMA as
 * fgr_ransac_pose's score: qx = ((R00 x + R01 y) + R02 z) + tx, d = q - b,
 * d2 = ((dx dx) + dy dy) + dz dz, r2 = inlier_dist * inlier_dist. Counts are integer block
 * reductions, every element is stored once.
 * FGR_E_ARG, with nothing launched or written: n_pairs outside 1..65535, an unknown mode,
 * n_rows outside 0..2^31 - 1, a NULL table, n_match or (n_rows > 0) operand, max_ratio > 0
 * without best / second, gt_pose without n_inlier or the reverse, gt_pose with inlier_dist not
 * finite or <= 0. */
enum { FGR_MATCH_DOT = 0, FGR_MATCH_EUCLID = 1 };
enum { FGR_MATCH_SRC = 0, FGR_MATCH_MUTUAL = 1, FGR_MATCH_BILATERAL = 2 };
int fgr_feature_nn_supported(int32_t d);
int fgr_feature_nn(const float* q, const float* k, int32_t d, int64_t n_q_rows, int64_t n_k_rows,
                   const int64_t* q_off, const int64_t* kv_off, const int32_t* kv_seg,
                   int32_t n_seg, int32_t max_q_len, int32_t metric, int32_t* nn_idx, float* best,
                   float* second, void* stream);
int fgr_match_pairs(const int32_t* nn_idx, const float* best, const float* second,
                    const float* xyz, int64_t n_rows, const int64_t* off, const int64_t* out_off,
                    int32_t n_pairs, int32_t mode, float max_ratio, const float* gt_pose,
                    float inlier_dist, float* a, float* b, float* w, int32_t* n_match,
                    int32_t* n_inlier, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FGREG_H */
