"""Loader of libfgreg.so (the C ABI declared in include/fgreg.h).

The library is built in-tree (csrc/Makefile -> fgreg/libfgreg.so) and loaded with
ctypes; torch tensors cross the boundary only as raw device pointers. There is no
fallback: if the library is missing, or no GPU is visible, every op raises.
"""
import ctypes
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('FGREG_LIB_PATH') or os.path.join(HERE, 'libfgreg.so')  # override: A/B builds (tools/)
CSRC = os.path.join(os.path.dirname(HERE), 'csrc')

_vp = ctypes.c_void_p
_i32 = ctypes.c_int32
_i64 = ctypes.c_int64
_f32 = ctypes.c_float
_sz = ctypes.c_size_t

ABI_VERSION = 2     # FGR_ABI_VERSION of include/fgreg.h (INTEGRATION.md "ABI history")

# name -> argtypes (all return int status)
SIGNATURES = {
    'fgr_grid_subsample_workspace': [_i64, _i32, _i64, ctypes.POINTER(_sz)],
    'fgr_grid_subsample_count': [_vp, _vp, _i32, _i64, _f32, _i64, _vp, _sz, _vp, _vp],
    'fgr_grid_subsample_fill': [_i64, _i32, _i64, _i64, _vp, _sz, _vp, _vp, _vp, _vp],
    'fgr_grid_subsample_sparse_workspace': [_i64, _i32, ctypes.POINTER(_sz)],
    'fgr_grid_subsample_sparse_count': [_vp, _vp, _i32, _i64, _f32, _i32, _vp, _sz, _vp, _vp],
    'fgr_grid_subsample_sparse_fill': [_i64, _i32, _i64, _vp, _sz, _vp, _vp, _vp, _vp],
    'fgr_radius_grid_workspace': [_i64, _i32, ctypes.POINTER(_sz)],
    'fgr_radius_grid_build': [_vp, _vp, _i32, _i64, _f32, _vp, _sz, _vp],
    'fgr_radius_search_grid': [_vp, _vp, _i32, _i64, _i32, _vp, _vp, _i64, _vp, _sz, _f32, _i32,
                               _i32, _vp, _vp, _vp, _vp],
    'fgr_radius_count': [_vp, _vp, _vp, _vp, _i32, _i64, _i32, _f32, _vp, _vp, _vp],
    'fgr_radius_search': [_vp, _vp, _vp, _vp, _i32, _i64, _i64, _i32, _f32, _i32, _i32, _vp, _vp],
    'fgr_kpconv_gather_workspace': [_i64, _i32, ctypes.POINTER(_sz)],
    'fgr_kpconv_gather': [_vp, _vp, _i64, _i64, _vp, _i32, _vp, _i32, _vp, _i32, _f32, _vp, _vp,
                          _vp, _sz, _vp],
    'fgr_kpconv_gather_mode': [_vp, _vp, _i64, _i64, _vp, _i32, _vp, _i32, _vp, _i32, _f32, _i32,
                               _i32, _vp, _vp, _vp, _sz, _vp],
    'fgr_kpconv_deform_points': [_vp, _vp, _vp, _vp, _i64, _i32, _f32, _vp, _vp, _vp],
    'fgr_kpconv_gather_deform_workspace': [_i64, _i32, ctypes.POINTER(_sz)],
    'fgr_kpconv_gather_deform': [_vp, _vp, _i64, _i64, _vp, _i32, _vp, _i32, _vp, _vp, _i32, _f32,
                                 _i32, _i32, _vp, _vp, _vp, _sz, _vp],
    'fgr_kpconv_scatter_deform_workspace': [_i64, _i32, _i32, ctypes.POINTER(_sz)],
    'fgr_kpconv_scatter_deform': [_vp, _vp, _i64, _i64, _vp, _i32, _vp, _i32, _vp, _vp, _i32, _f32,
                                  _i32, _i32, _vp, _vp, _vp, _vp, _sz, _vp],
    'fgr_kpconv_deform_grad': [_vp, _vp, _i64, _i64, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _i32,
                               _f32, _i32, _i32, _vp, _vp, _vp],
    'fgr_max_pool': [_vp, _i64, _i32, _vp, _i64, _i32, _vp, _vp],
    'fgr_instnorm_workspace': [_i64, _i32, _i32, ctypes.POINTER(_sz)],
    'fgr_instnorm': [_vp, _i64, _i32, _vp, _i32, _i64, _vp, _f32, _i32, _vp, _i32, _vp, _vp, _sz,
                     _vp],
    'fgr_layernorm': [_vp, _i64, _i32, _vp, _vp, _f32, _vp, _vp, _vp, _vp],
    'fgr_sine_pos_embed': [_vp, _i64, _i32, _f32, _f32, _vp, _vp],
    'fgr_add': [_vp, _vp, _i64, _vp, _vp],
    'fgr_layernorm_dual': [_vp, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f32, _vp],
    'fgr_attention': [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _i32, _i32, _i32,
                      _i32, _f32, _vp],
    'fgr_attention_weights': [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _i32, _i32, _i32, _i32,
                              _i32, _f32, _vp],
    'fgr_attention_f16x3_workspace': [_i64, _i32, _i32, ctypes.POINTER(_sz)],
    'fgr_attention_f16x3': [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _i32, _i32,
                            _i64, _i32, _i32, _i32, _i32, _f32, _vp, _i64, _vp],
    'fgr_attention_f16x3_drop': [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _i32,
                                 _i32, _i64, _i32, _i32, _i32, _i32, _f32, _vp, _i64,
                                 ctypes.c_uint32, _f32, _vp],
    'fgr_attention_f16x3_train': [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _i32,
                                  _i32, _i64, _i32, _i32, _i32, _i32, _f32, _vp, _i64,
                                  ctypes.c_uint32, _f32, _vp, _vp],
    'fgr_attention_bf16_workspace': [_i64, _i32, _i32, ctypes.POINTER(_sz)],
    'fgr_attention_bf16': [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _i32, _i32,
                           _i64, _i32, _i32, _i32, _i32, _f32, _vp, _i64, _vp],
    'fgr_res2net_chain6': [_vp, _i64, _i32, _i32, _vp, _vp, _vp, _i32, _vp, _i64, _vp],
    'fgr_res2net_chain_h3': [_vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _i64, _vp],
    'fgr_res2net_block_h3': [_vp, _i64, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64,
                             _vp],
    'fgr_res2net_block6': [_vp, _i64, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp],
    'fgr_split_weights_h3_bytes': [_i32, _i32, ctypes.POINTER(_sz)],
    'fgr_split_weights_h3_batch': [_vp, _i32, _i64, _vp],
    'fgr_split_weights_h3': [_vp, _i32, _i32, _i64, _i64, _vp, _vp],
    'fgr_gemm_f16x3': [_vp, _i64, _vp, _vp, _i64, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _vp],
    'fgr_gemm_f16x3_ln_supported': [_i32, _i32, _i32],
    'fgr_gemm_f16x3_ln': [_vp, _i64, _vp, _vp, _f32, _vp, _i64, _vp, _vp, _i64, _vp, _i32, _i32,
                          _i32, _i32, _vp],
    'fgr_gemm_f16x3_ln_out2': [_vp, _i64, _vp, _vp, _f32, _vp, _i64, _vp, _vp, _i64, _vp, _i32,
                               _i32, _i32, _i32, _vp, _vp, _vp, _i64, _vp],
    'fgr_split_weights_ffn2_bytes': [_i32, _i32, ctypes.POINTER(_sz)],
    'fgr_split_weights_ffn2': [_vp, _i32, _i32, _i64, _i64, _vp, _vp],
    'fgr_ffn_f16x3_supported': [_i32, _i32, _i32],
    'fgr_ffn_f16x3': [_vp, _i64, _vp, _vp, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32,
                      _i32, _vp],
    'fgr_ffn_f16x3_act_supported': [_i32, _i32, _i32, _i32],
    'fgr_ffn_f16x3_act': [_vp, _i64, _vp, _vp, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32,
                          _i32, _i32, _i32, _vp],
    'fgr_gelu_fwd': [_vp, _vp, _i64, _vp],
    'fgr_gelu_bwd': [_vp, _vp, _vp, _i64, _vp],
    'fgr_pos_mlp_f16x3_supported': [_i64, _i32],
    'fgr_pos_mlp_f16x3': [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp,
                          _i64, _vp],
    'fgr_geo_embed_indices': [_vp, _i64, _vp, _i32, _i32, _f32, _f32, _vp, _vp, _vp, _vp],
    'fgr_geo_embed_f16x3_supported': [_i64, _i32, _i32],
    'fgr_geo_embed_f16x3': [_vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _i64,
                            _vp],
    'fgr_split_weights_bf16_bytes': [_i32, _i32, ctypes.POINTER(_sz)],
    'fgr_split_weights_bf16': [_vp, _i32, _i32, _i64, _i64, _vp, _vp],
    'fgr_gemm_bf16': [_vp, _i64, _vp, _vp, _i64, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _vp],
    'fgr_gemm_workspace': [_i32, _i32, _i32, _i32, ctypes.POINTER(_sz)],
    'fgr_gemm_f16x3_ws': [_vp, _i64, _vp, _vp, _i64, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _vp,
                          _sz, _vp],
    'fgr_gemm_bf16_ws': [_vp, _i64, _vp, _vp, _i64, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _vp,
                         _sz, _vp],
    'fgr_kv_image_bytes': [_i64, _i32, _i32, ctypes.POINTER(_sz)],
    'fgr_gemm_f16x3_ln_qkv_supported': [_i32, _i32, _i32],
    'fgr_gemm_f16x3_ln_qkv': [_vp, _i64, _vp, _vp, _f32, _vp, _i64, _vp, _vp, _i64, _vp, _i32, _i32,
                              _i32, _vp, _vp, _vp, _vp, _i64, _vp],
    'fgr_gemm_f16x3_qkv_supported': [_i32, _i32, _i32],
    'fgr_gemm_f16x3_qkv': [_vp, _i64, _vp, _vp, _i64, _vp, _i32, _i32, _i32, _vp, _vp],
    'fgr_kv_image_bf16_bytes': [_i64, _i32, _i32, ctypes.POINTER(_sz)],
    'fgr_gemm_bf16_qkv_supported': [_i32, _i32, _i32],
    'fgr_gemm_bf16_qkv': [_vp, _i64, _vp, _vp, _i64, _vp, _i32, _i32, _i32, _vp, _vp],
    'fgr_attention_bf16_img': [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _i32, _i32, _i32,
                               _i32, _f32, _vp],
    'fgr_attention_f16x3_img': [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _i32, _i32, _i32,
                                _i32, _f32, _vp],
    'fgr_corr_head_supported': [_i32, _i32],
    'fgr_corr_head_f16x3': [_vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    'fgr_copy_batch': [_i32, _vp, _vp, _vp, _vp],
    'fgr_lengths_to_offsets': [_vp, _i32, _vp, _vp],
    'fgr_overlap_pool': [_vp, _i64, _vp, _i64, _i32, _vp, _vp],
    'fgr_bce_logits_mean': [_vp, _i64, _vp, _i64, _vp, _vp],
    'fgr_transform_points': [_vp, _i64, _vp, _i32, _vp, _i32, _vp, _vp],
    'fgr_infonce_rows': [_vp, _i64, _vp, _vp, _vp, _vp, _i32, _i64, _f32, _f32, _vp, _vp, _vp],
    'fgr_infonce_reduce': [_vp, _vp, _vp, _i32, _vp, _vp],
    'fgr_infonce_rows_bwd': [_vp, _i64, _vp, _vp, _vp, _vp, _i32, _i64, _i64, _f32, _vp, _vp, _vp, _i64,
                             _vp],
    'fgr_circle_loss_workspace': [_i64, _i64, _i64, ctypes.POINTER(_sz)],
    'fgr_circle_loss': [_vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _i64, _i64, _i32, _i32,
                        _i64, _f32, _f32, _vp, _sz, _vp, _vp],
    'fgr_pair_cdist': [_vp, _vp, _i32, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp],
    'fgr_corr_loss': [_vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp],
    'fgr_se3_compare': [_vp, _vp, _i32, _i32, _vp, _vp, _vp],
    'fgr_corr_attention': [_vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32,
                           _f32, _vp],
    'fgr_corr_topk_workspace': [_i64, _i32, ctypes.POINTER(_sz)],
    'fgr_corr_topk_mask': [_vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _i32, _i32, _i64, _i32, _i32,
                           _i32, _f32, _i32, _vp, _vp, _sz, _vp],
    'fgr_procrustes': [_vp, _vp, _vp, _i64, _i64, _f32, _vp, _vp],
    'fgr_time_next_call': [_vp, _vp],
    'fgr_pair_pose': [_vp, _vp, _vp, _i64, _vp, _i32, _i32, _f32, _vp, _vp],
    'fgr_nbr_inverse_workspace': [_i64, _i32, _i64, ctypes.POINTER(_sz)],
    'fgr_nbr_inverse': [_vp, _i64, _i32, _i64, _vp, _vp, _vp, _vp, _sz, _vp],
    'fgr_kpconv_scatter_workspace': [_i64, _i32, _i32, ctypes.POINTER(_sz)],
    'fgr_kpconv_scatter': [_vp, _vp, _i64, _i64, _vp, _i32, _vp, _i32, _vp, _i32, _f32, _vp, _vp,
                           _vp, _vp, _sz, _vp],
    'fgr_kpconv_scatter_mode': [_vp, _vp, _i64, _i64, _vp, _i32, _vp, _i32, _vp, _i32, _f32, _i32,
                                _i32, _vp, _vp, _vp, _vp, _sz, _vp],
    'fgr_max_pool_bwd_workspace': [_i64, _i32, ctypes.POINTER(_sz)],
    'fgr_max_pool_bwd': [_vp, _i64, _i32, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _sz, _vp],
    'fgr_corr_attention_bwd_workspace': [_i64, ctypes.POINTER(_sz)],
    'fgr_corr_attention_bwd': [_vp, _i64, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp,
                               _vp, _i32, _i32, _i64, _i32, _i32, _i32, _f32, _vp, _sz, _vp],
    'fgr_segnorm_workspace': [_i64, _i32, _i32, ctypes.POINTER(_sz)],
    'fgr_segnorm_stats': [_vp, _i64, _i32, _vp, _i32, _i64, _vp, _f32, _vp, _vp, _vp, _vp, _sz, _vp],
    'fgr_segnorm_apply': [_vp, _i64, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _vp,
                          _vp],
    'fgr_segnorm_fwd': [_vp, _i64, _i32, _vp, _i32, _i64, _vp, _f32, _vp, _vp, _vp, _vp, _vp, _i32, _vp,
                        _i32, _vp, _vp, _sz, _vp],
    'fgr_segnorm_bwd': [_vp, _i64, _i32, _vp, _i32, _i64, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32,
                        _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp],
    'fgr_colsum_workspace': [_i64, _i32, ctypes.POINTER(_sz)],
    'fgr_colsum': [_vp, _i64, _i32, _i64, _vp, _vp, _sz, _vp],
    'fgr_gemm_wgrad_workspace': [_i64, _i32, _i32, _i32, ctypes.POINTER(_sz)],
    'fgr_gemm_f16x3_wgrad': [_vp, _i64, _vp, _i64, _i64, _i32, _i32, _vp, _i64, _vp, _vp, _sz, _vp],
    'fgr_layernorm_bwd_workspace': [_i64, _i32, ctypes.POINTER(_sz)],
    'fgr_layernorm_bwd': [_vp, _i64, _i32, _vp, _f32, _vp, _vp, _vp, _vp, _sz, _vp],
    'fgr_attention_bwd_workspace': [_i64, _i32, ctypes.POINTER(_sz)],
    'fgr_attention_bwd': [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64,
                          _vp, _i64, _vp, _vp, _vp, _i32, _i32, _i64, _i64, _i64, _i32, _i32, _f32,
                          _vp, _sz, _vp],
    'fgr_attention_bwd_drop': [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64,
                               _vp, _i64, _vp, _i64, _vp, _vp, _vp, _i32, _i32, _i64, _i64, _i64,
                               _i32, _i32, _f32, _vp, _sz, ctypes.c_uint32, _f32, _vp],
    'fgr_attention_bwd_train': [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64,
                                _vp, _i64, _vp, _i64, _vp, _vp, _vp, _i32, _i32, _i64, _i64, _i64,
                                _i32, _i32, _f32, _vp, _sz, ctypes.c_uint32, _f32, _vp, _i64, _vp],
    'fgr_attention_bwd_train_workspace': [_i64, _i32, _i64, _i32, _i32, _i32, ctypes.POINTER(_sz)],
    'fgr_modelnet_metrics_workspace': [_i32, _i32, ctypes.POINTER(_sz)],
    'fgr_modelnet_metrics': [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _sz, _vp, _vp],
    'fgr_crop_max_points': [ctypes.POINTER(_i32)],
    'fgr_crop_pairs_mask': [_vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    'fgr_crop_pairs_assemble': [_vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp,
                                _vp, _vp],
    'fgr_augment_workspace_bytes': [_i64, _i32, ctypes.POINTER(_sz)],
    'fgr_augment_pairs': [_vp, _i32, _vp, _i64, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i32,
                          _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp],
    'fgr_icp_workspace': [_i64, _i64, _i32, ctypes.POINTER(_sz)],
    'fgr_icp': [_vp, _vp, _i64, _vp, _vp, _i64, _i32, _i32, _vp, _f32, _i32, _f32, _f32, _vp, _sz,
                _vp, _vp, _vp, _vp, _vp],
    'fgr_registration_score': [_vp, _vp, _i64, _vp, _vp, _i64, _i32, _i32, _vp, _f32, _vp, _sz,
                               _vp, _vp, _vp, _vp, _vp, _vp],
    'fgr_estimate_normals_workspace': [_i64, _i32, ctypes.POINTER(_sz)],
    'fgr_estimate_normals': [_vp, _vp, _i64, _i32, _f32, _vp, _vp, _sz, _vp, _vp, _vp],
    'fgr_icp_plane_workspace': [_i64, _i64, _i32, ctypes.POINTER(_sz)],
    'fgr_icp_plane': [_vp, _vp, _i64, _vp, _vp, _i64, _vp, _i32, _i32, _vp, _f32, _i32, _f32, _f32,
                      _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    'fgr_ransac_workspace': [_i64, _i32, _i32, ctypes.POINTER(_sz)],
    'fgr_ransac_pose': [_vp, _vp, _vp, _i64, _vp, _i32, _f32, _f32, _i32, ctypes.c_uint32, _i32,
                        _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    'fgr_compat_workspace': [_i64, _i32, _i32, _i32, ctypes.POINTER(_sz)],
    'fgr_compat_pose': [_vp, _vp, _vp, _i64, _vp, _i32, _i32, _f32, _f32, _f32, _i32, _i32, _i32,
                        _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    'fgr_feature_nn_supported': [_i32],
    'fgr_feature_nn': [_vp, _vp, _i32, _i64, _i64, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp,
                       _vp],
    'fgr_match_pairs': [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _i32, _i32, _f32, _vp, _f32, _vp, _vp,
                        _vp, _vp, _vp, _vp],
}

NB_INDEX, NB_DIST = 0, 1
ACT_NONE, ACT_LEAKY, ACT_RELU, ACT_RELU_RES_LEAKY = 0, 1, 2, 3
ACT_GELU = 4        # ops.ffn / autograd.linear_t only: no GEMM entry point takes it

_lib = None


class FgrError(RuntimeError):
    pass


def build(jobs=8):
    """Compile csrc/ into fgreg/libfgreg.so for gfx950 (hipcc cross-compiles without a GPU)."""
    subprocess.check_call(['make', '-s', '-C', CSRC, f'-j{jobs}'])


def load():
    """Returns the ctypes handle, raising FgrError if the library cannot be loaded."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FgrError(f'{LIB_PATH} not built: run `make -C {CSRC}` (or __graft_entry__.build())')
    L = ctypes.CDLL(LIB_PATH)
    L.fgr_abi_version.restype = ctypes.c_int
    L.fgr_last_error.restype = ctypes.c_char_p
    # version first: a stale library fails here, not on a missing symbol below
    if L.fgr_abi_version() != ABI_VERSION:
        raise FgrError(f'libfgreg ABI version mismatch: {LIB_PATH} has {L.fgr_abi_version()}, '
                       f'fgreg expects {ABI_VERSION} (rebuild: make -C {CSRC})')
    for name, argtypes in SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype = ctypes.c_int
        fn.argtypes = argtypes
    _lib = L
    return L


def check(rc, name):
    if rc != 0:
        msg = load().fgr_last_error().decode(errors='replace')
        raise FgrError(f'{name} failed ({rc}): {msg}')


_WS_SIZES = {}


def ws_size(name, *args):
    """Bytes a `*_workspace(args..., size_t* bytes)` entry point reports, memoised per
    (name, args): the queries are pure functions of the shape, and training issues hundreds
    per step."""
    key = (name,) + args
    v = _WS_SIZES.get(key)
    if v is None:
        nb = _sz(0)
        check(getattr(load(), name)(*args, nb), name)
        v = nb.value
        if len(_WS_SIZES) > 65536:
            _WS_SIZES.clear()
        _WS_SIZES[key] = v
    return v
