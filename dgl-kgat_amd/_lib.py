"""Loader for libkgat_hip.so - the C-ABI library (include/kgat_hip.h) that holds every HIP
kernel of the path.  There is no fallback: if the library is missing, does not load, or
lacks a declared symbol, importing the op layer fails loudly."""
import ctypes as C
import hashlib
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
SO_PATH = os.path.join(_HERE, "libkgat_hip.so")
# source -> extra hipcc flags.  -amdgpu-mfma-vgpr-form puts MFMA results in VGPRs so the VALU
# epilogue reads them without v_accvgpr_read copies (f32 MFMA and VALU share the SIMD's issue
# port - measured with scripts/micro/mfma_rate.hip - so fewer instructions is the lever); the
# LDS-staged chunk kernels lose occupancy with it and are built without.
SOURCES = {
    "kgat_graph.hip": [],
    "kgat_permute.hip": [],
    "kgat_spmm.hip": [],
    "kgat_spmm_max.hip": [],
    "kgat_spmm_kmax.hip": [],
    "kgat_spmm_bi.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form=1"],
    "kgat_softmax.hip": [],
    "kgat_att.hip": [],
    "kgat_att_persistent.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form=1"],
    "kgat_dense.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form=1"],
    "kgat_transr.hip": [],
    "kgat_transr_rank.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form=1"],
    "kgat_eval.hip": [],
    "kgat_eval_topk.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form=1"],
    "kgat_eval_rank.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form=1"],
    "kgat_optim.hip": [],
    "kgat_bpr.hip": [],
    "kgat_sage.hip": [],
    "kgat_edge_weights.hip": [],
    "kgat_att_bwd.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form=1"],
    "kgat_gat.hip": [],
    "kgat_rgcn.hip": [],
    "kgat_transe.hip": [],
    "kgat_bi_pool.hip": [],
    "kgat_ripple.hip": [],
    "kgat_nfm_eval.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form=1"],
    "kgat_ripple_eval.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form=1"],
}
HEADER = os.path.join(os.path.dirname(_HERE), "include", "kgat_hip.h")

_i64, _i32, _u32, _sz, _p = C.c_int64, C.c_int, C.c_uint, C.c_size_t, C.c_void_p

# name -> (restype, argtypes); must list every function include/kgat_hip.h declares
SIGNATURES = {
    "kgat_version": (_i32, []),
    "kgat_last_error": (C.c_char_p, []),
    "kgat_build_hash": (C.c_char_p, []),
    "kgat_csr_from_coo_workspace_bytes": (_sz, [_i64, _i64]),
    "kgat_csr_from_coo": (_i32, [_i64, _i64, _p, _p, _p, _p, _p, _p, _p, _sz, _p]),
    "kgat_group_by_relation_workspace_bytes": (_sz, [_i64, _i32]),
    "kgat_group_by_relation": (_i32, [_i64, _i32, _p, _p, _p, _p, _sz, _p]),
    "kgat_invert_permutation": (_i32, [_i64, _p, _p, _p]),
    "kgat_row_order_workspace_bytes": (_sz, [_i64]),
    "kgat_row_order_by_degree": (_i32, [_i64, _p, _p, _p, _sz, _p]),
    "kgat_att_score_f32": (_i32, [_i64, _i64, _i32, _i32, _i32, _p, _p, _p, _p, _p, _p, _p, _p, _p,
                                  _p, _i32, _p]),
    "kgat_head_groups_workspace_bytes": (_sz, [_i64]),
    "kgat_head_groups": (_i32, [_i64, _i32, _p, _p, _p, _p, _p, _p, _sz, _p]),
    "kgat_att_score_split_supported": (_i32, [_i64, _i32, _i32, _i32]),
    "kgat_att_score_split_f32": (_i32, [_i64, _i64, _i32, _i32, _i32, _p, _p, _p, _p, _p, _p, _p, _i64, _p, _p,
                                        _p, _p, _p, _p, _p]),
    "kgat_att_score_folded_supported": (_i32, [_i64, _i32, _i32, _i32]),
    "kgat_att_score_folded_f32": (_i32, [_i64, _i64, _i32, _i32, _i32, _p, _p, _p, _p, _p, _p, _p, _i64, _p, _p,
                                         _p, _p, _p, _p, _i32, _p]),
    "kgat_fold_tiles_max": (_i64, [_i64, _i64, _i32, _i32]),
    "kgat_fold_tiles_workspace_bytes": (_sz, [_i64, _i32]),
    "kgat_fold_tiles": (_i32, [_i64, _i32, _i64, _p, _p, _p, _i32, _p, _p, _p, _sz, _p]),
    "kgat_att_score_fused_supported": (_i32, [_i64, _i32, _i32, _i32]),
    "kgat_fold_tile_parts_workspace_bytes": (_sz, [_i64]),
    "kgat_fold_tile_parts": (_i32, [_i64, _i32, _p, _p, _i32, _i32, _i32, _i32, _p, _p, _sz, _p]),
    "kgat_att_pack_records": (_i32, [_i64, _i32, _p, _p, _p, _p, _p, _p]),
    "kgat_att_score_fused_f32": (_i32, [_i64, _i64, _i32, _i32, _i32, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i32,
                                        _p, _p, _p, _p, _p, _p, _i32, _p]),
    "kgat_att_score_fused_timed_f32": (_i32, [_i64, _i64, _i32, _i32, _i32, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i32,
                                              _p, _p, _p, _p, _p, _p, _i32, _p, _p]),
    # backward of the attention logits: reference models.py:135-154 under autograd (ABI 15, additive)
    "kgat_att_score_bwd_supported": (_i32, [_i64, _i32, _i32, _i32]),
    "kgat_att_score_bwd_workspace_bytes": (_sz, [_i64, _i64, _i64, _i32, _i32, _i32]),
    "kgat_att_score_bwd_f32": (_i32, [_i64, _i64, _i64, _i32, _i32, _i32, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p,
                                      _p, _p, _p, _p, _p, _p, _sz, _p]),
    "kgat_edge_softmax_workspace_bytes": (_sz, [_i64, _i64]),
    "kgat_edge_softmax_f32": (_i32, [_i64, _i64, _i64, _p, _p, _p, _p, _i32, _p, _p, _p, _sz, _p]),
    "kgat_edge_softmax_3pass_workspace_bytes": (_sz, [_i64]),
    "kgat_edge_softmax_3pass_f32": (_i32, [_i64, _i64, _i64, _p, _p, _p, _i32, _p, _p, _p, _sz, _p]),
    "kgat_edge_softmax_bwd_f32": (_i32, [_i64, _i64, _p, _p, _p, _p, _p, _p]),
    "kgat_spmm_workspace_bytes": (_sz, [_i64, _i32]),
    "kgat_spmm_umule_sum_f32": (_i32, [_i64, _i64, _i64, _i64, _i32, _p, _p, _p, _p, _p, _p, _p, _p,
                                       _p, _sz, _u32, _i32, _p, _i64, _p]),
    # DGL's fn.max reducer with argmax; the max-times product of explain.attention_paths (ABI 16, additive)
    "kgat_spmm_max_workspace_bytes": (_sz, [_i64, _i32]),
    "kgat_spmm_umule_max_f32": (_i32, [_i64, _i64, _i64, _i64, _i32, _p, _p, _p, _p, _p, _p, _p, _p, _p, _sz, _p]),
    # the top-4 reducer with (edge, slot) back-pointers: explain.attention_paths(top=2..4) (ABI 16, additive)
    "kgat_spmm_max4_workspace_bytes": (_sz, [_i64, _i32]),
    "kgat_spmm_umule_max4_f32": (_i32, [_i64, _i64, _i64, _i64, _i32, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _sz, _p]),
    "kgat_bi_interaction_supported": (_i32, [_i32, _i32]),
    "kgat_spmm_bi_fused_supported": (_i32, [_i32, _i32]),
    "kgat_spmm_bi_fused_f32": (_i32, [_i64, _i64, _i64, _i64, _i32, _i32, _p, _p, _p, _p, _p, _p, C.c_float, _p, _p,
                                      _i64, _p, _p, _sz, _p, _i64, _p]),
    "kgat_add3_rows_f32": (_i32, [_i64, _i32, _p, _i64, _p, _p, _p, _p]),
    "kgat_sum_partials_f32": (_i32, [_i32, _p, _p, _p, _p, _p]),
    "kgat_bi_interaction_bwd_pre_f32": (_i32, [_i64, _i32, _p, _p, _p, _p, _i64, C.c_float, C.c_float, C.c_uint64, _i64,
                                               _p, _p]),
    "kgat_mul2_f32": (_i32, [_i64, _p, _p, _p, _p, _p, _p]),
    "kgat_bi_interaction_bwd_input_supported": (_i32, [_i32, _i32]),
    "kgat_bi_interaction_bwd_weight_partials": (_i64, [_i64]),
    "kgat_transr_supported": (_i32, [_i64, _i32, _i32, _i32, _i64]),
    "kgat_transr_workspace_bytes": (_sz, [_i64, _i32, _i32, _i32]),
    "kgat_transr_loss_grad_f32": (_i32, [_i64, _i32, _i32, _i32, _i64, _p, _p, _p, _p, _p, _p, _p, C.c_float, _p, _p,
                                         _p, _p, _p, _sz, _p]),
    "kgat_transr_forward_f32": (_i32, [_i64, _i32, _i32, _i32, _i64, _p, _p, _p, _p, _p, _p, _p, C.c_float, _p, _p, _sz, _p]),
    "kgat_transr_backward_f32": (_i32, [_i64, _i32, _i32, _i32, _i64, _p, _p, _p, _p, _p, _p, _p, _p, _p, _sz, _p]),
    "kgat_bi_interaction_f32": (_i32, [_i64, _i32, _i32, _p, _p, C.c_float, _p, _p, _i64, _p]),
    "kgat_spmm_tile_edges": (_i32, [_i64, _i32]),
    "kgat_l2_normalize_rows_f32": (_i32, [_i64, _i32, _p, _p, _i64, _p]),
    "kgat_readout_concat_f32": (_i32, [_i64, _i32, _p, _p, _p, _p, _i64, _p]),
    "kgat_sddmm_dot_f32": (_i32, [_i64, _i32, _p, _p, _p, _p, _p, _p]),
    "kgat_gather_probe_f32": (_i32, [_i64, _i32, _p, _p, _p, _p]),
    "kgat_gather_f32": (_i32, [_i64, _p, _p, _p, _p]),
    "kgat_gather_i32": (_i32, [_i64, _p, _p, _p, _p]),
    # a graph-static permutation as two streaming passes over a plan (ABI 16, additive)
    "kgat_permute_tile": (_i32, []),
    "kgat_permute_supported": (_i32, [_i64]),
    "kgat_permute_f32": (_i32, [_i64, _p, _p, _p, _p, _p, _p, _p]),
    # edge softmax + edge-id-ordered copy, the cut-row rescale folded into the bin pass (ABI 16, additive)
    "kgat_edge_softmax_permuted_supported": (_i32, [_i64, _i64]),
    "kgat_edge_softmax_permuted_f32": (_i32, [_i64, _i64, _i64, _p, _p, _p, _p, _i32, _p, _p, _p, _p, _p, _p, _p, _sz, _p]),
    "kgat_eval_supported": (_i32, [_i32, _i32]),
    "kgat_eval_items_elems": (_i64, [_i64, _i32]),
    "kgat_eval_items_kmajor_f32": (_i32, [_i64, _i32, _p, _i64, _p, _p, _p]),
    "kgat_eval_workspace_bytes": (_sz, [_i64, _i64, _i32, _i32]),
    "kgat_bpr_workspace_bytes": (_sz, [_i64, _i32]),
    "kgat_bpr_loss_f32": (_i32, [_i64, _i32, _p, _i64, _i64, _p, _p, _p, C.c_float, _p, _p, _p, _sz, _p]),
    "kgat_bpr_grad_f32": (_i32, [_i64, _i32, _p, _i64, _i64, _p, _p, _p, _p, C.c_float, _p, _p, _p, _sz, _p]),
    "kgat_transr_sorted_bytes": (_sz, [_i64, _i32]),
    "kgat_transr_presort_f32": (_i32, [_i64, _i32, _i64, _i64, _p, _p, _p, _p, _p, _sz, _p]),
    "kgat_transr_step_workspace_bytes": (_sz, [_i64, _i32, _i32, _i32]),
    "kgat_transr_adam_step_f32": (_i32, [_i64, _i32, _i32, _i32, _i64, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p,
                                         C.c_double, C.c_double, C.c_double, C.c_double, C.c_float, _p, _p, C.c_uint64,
                                         _p, _sz, _p]),
    # BPR-MF pretraining as three-launch iterations: reference models.py:170-178, kgat.py:150-168 (ABI 16, additive)
    "kgat_mf_supported": (_i32, [_i64, _i32, _i64]),
    "kgat_mf_sorted_bytes": (_sz, [_i64]),
    "kgat_mf_presort_f32": (_i32, [_i64, _i64, _i64, _p, _p, _p, _p, _sz, _p]),
    "kgat_mf_step_workspace_bytes": (_sz, [_i64, _i32]),
    "kgat_mf_adam_step_f32": (_i32, [_i64, _i32, _i64, _p, _p, _p, _p, _p, _p, _p, _i64, C.c_double, C.c_double,
                                     C.c_double, C.c_double, C.c_float, _p, _p, C.c_uint64, _p, _sz, _p]),
    "kgat_adam_max_tensors": (_i32, []),
    "kgat_adam_step_f32": (_i32, [_i32, _p, _p, _p, _p, _p, _p, C.c_double, C.c_double, C.c_double, C.c_double, _i32, _p]),
    # global-norm gradient clipping: reference kgat.py:32,162 (ABI 16, additive)
    "kgat_grad_norm_chain": (_i32, []),
    "kgat_grad_sumsq_partials": (_i64, [_i32, _p]),
    "kgat_grad_sumsq_f32": (_i32, [_i32, _p, _p, _p, _i64, _p]),
    "kgat_grad_norm_finish_f32": (_i32, [_i64, _p, C.c_double, _p, _p, _p]),
    "kgat_adam_step_clipped_f32": (_i32, [_i32, _p, _p, _p, _p, _p, _p, C.c_double, C.c_double, C.c_double, C.c_double,
                                          _i32, _p, _p]),
    "kgat_scale_grads_f32": (_i32, [_i32, _p, _p, _p, _p]),
    "kgat_copy_reduce_f32": (_i32, [_i64, _i64, _i64, _i64, _i32, _p, _p, _p, _p, _p, _i32, _p, _sz, _p]),
    "kgat_sage_dense_supported": (_i32, [_i32, _i32]),
    "kgat_sage_dense_f32": (_i32, [_i64, _i32, _i32, _p, _p, _p, _p, _p, _p, _i32, _p, _p, _i64, _p, _i64, _p]),
    "kgat_dropout_rows_f32": (_i32, [_i64, _i32, _p, _p, C.c_float, C.c_uint64, _p, _p]),
    "kgat_sage_bwd_input_f32": (_i32, [_i64, _i32, _i32, _p, _p, _p, _p, _p, _p, _p]),
    "kgat_sage_bwd_weight_f32": (_i32, [_i64, _i32, _i32, _p, _p, _p, _p, _p, _p, _i64, _p]),
    "kgat_aggregator_supported": (_i32, [_i32, _i32, _i32]),
    "kgat_aggregator_f32": (_i32, [_i32, _i64, _i32, _i32, _p, _p, _p, C.c_float, _p, _p, _i64, _p, _i64, _p]),
    "kgat_aggregator_deferred_f32": (_i32, [_i32, _i64, _i32, _i32, _p, _p, _p, C.c_float, _p, _p, _i64, _p, _i64, _p,
                                            _i64, _i64, _p, _i32, _p]),
    "kgat_aggregator_train_f32": (_i32, [_i32, _i64, _i32, _i32, _p, _p, _p, C.c_float, C.c_float, C.c_uint64, _i64, _p,
                                         _p, _i64, _p, _i64, _p]),
    "kgat_aggregator_bwd_supported": (_i32, [_i32, _i32, _i32]),
    "kgat_aggregator_bwd_input_f32": (_i32, [_i32, _i64, _i32, _i32, _p, _p, _p, _p, _p, _p, _p]),
    "kgat_aggregator_bwd_weight_f32": (_i32, [_i32, _i64, _i32, _i32, _p, _p, _p, _p, _i64, _p]),
    "kgat_bi2_supported": (_i32, [_i32, _i32]),
    "kgat_bi2_bwd_supported": (_i32, [_i32, _i32]),
    "kgat_bi2_f32": (_i32, [_i64, _i32, _i32, _p, _p, _p, _p, C.c_float, _p, _p, _i64, _p, _i64, _p]),
    "kgat_bi2_deferred_f32": (_i32, [_i64, _i32, _i32, _p, _p, _p, _p, C.c_float, _p, _p, _i64, _p, _i64, _p, _i64, _i64,
                                     _p, _i32, _p]),
    "kgat_bi2_train_f32": (_i32, [_i64, _i32, _i32, _p, _p, _p, _p, C.c_float, C.c_float, C.c_uint64, _i64, _p, _p, _p,
                                  _i64, _p, _i64, _p]),
    "kgat_bi2_bwd_pre_f32": (_i32, [_i64, _i32, _p, _p, _p, _p, _p, _i64, C.c_float, C.c_float, C.c_uint64, _i64, _p, _p,
                                    _p]),
    "kgat_bi2_bwd_input_f32": (_i32, [_i64, _i32, _i32, _p, _p, _p, _p, _p, _p, _p, _p, _p]),
    "kgat_bi2_bwd_weight_f32": (_i32, [_i64, _i32, _i32, _p, _p, _p, _p, _p, _p, _i64, _p]),
    "kgat_eval_recall_ndcg_f32": (_i32, [_i64, _p, _i64, _i32, _p, _i64, _p, _p, _p, _p, _p, _i32, _p, _p, _sz, _p,
                                         _p, _p, _p]),
    "kgat_eval_topk_supported": (_i32, [_i32, _i32]),
    "kgat_eval_topk_workspace_bytes": (_sz, [_i64, _i64, _i32, _i32]),
    "kgat_eval_topk_f32": (_i32, [_i64, _p, _i64, _i32, _p, _i64, _p, _p, _p, _i32, _i32, _p, _sz, _p, _p, _p]),
    "kgat_eval_metrics_at_ks": (_i32, [_i64, _i32, _p, _p, _p, _i32, _p, _p, _p, _p]),
    # exact ranks of the held-out items at any depth and their metrics (ABI 16, additive)
    "kgat_eval_rank_supported": (_i32, [_i32]),
    "kgat_eval_rank_workspace_bytes": (_sz, [_i64, _i64, _i32, _i64, _i64]),
    "kgat_eval_rank_f32": (_i32, [_i64, _p, _i64, _i32, _p, _i64, _p, _p, _p, _i64, _p, _p, _i64, _i32, _p, _sz, _p, _p,
                                  _p]),
    "kgat_eval_rank_metrics_workspace_bytes": (_sz, [_i64]),
    "kgat_eval_rank_metrics": (_i32, [_i64, _i64, _p, _p, _p, _i64, _p, _i32, _p, _p, _p, _sz, _p, _p, _p]),
    "kgat_edge_norm_f32": (_i32, [_i64, _i64, _p, _p, _p, _p, _p, _i32, _p, _p, _p]),
    "kgat_edge_dropout_f32": (_i32, [_i64, _p, _p, C.c_float, C.c_uint64, _p, _p]),
    # TransR link prediction: projection + filtered rank counts (ABI 16, additive)
    "kgat_transr_project_supported": (_i32, [_i32, _i32]),
    "kgat_transr_project_f32": (_i32, [_i64, _i64, _i32, _i32, _p, _p, _i64, _p, _p, C.c_float, _p, _p, _p]),
    "kgat_transr_rank_supported": (_i32, [_i32]),
    "kgat_transr_rank_f32": (_i32, [_i64, _i64, _i64, _i32, _p, _p, _p, _p, _p, _p, _i64, _p, _p, _p]),
    # dgl.nn.pytorch.conv.GATConv's aggregation (u_add_v, leaky_relu, edge_softmax, u_mul_e -> sum) in one walk, and
    # its backward (ABI 16, additive)
    "kgat_gat_supported": (_i32, [_i32, _i32]),
    "kgat_gat_workspace_bytes": (_sz, [_i64, _i64, _i32, _i32, _i32]),
    "kgat_gat_fwd_f32": (_i32, [_i64, _i64, _i32, _i32, _p, _p, _p, _p, _p, _p, _p, C.c_float, C.c_float, C.c_uint64,
                                _p, _p, _p, _p, _sz, _p]),
    "kgat_gat_bwd_f32": (_i32, [_i64, _i64, _i32, _i32, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p,
                                C.c_float, C.c_float, C.c_uint64, _p, _p, _p, _p, _sz, _p]),
    # dgl.nn.pytorch.conv.RelGraphConv (regularizer "basis"), the sparse part aggregate-first: one gather of a source
    # row feeds B accumulators; backward towards x and towards the coefficients (ABI 16, additive)
    "kgat_rgcn_supported": (_i32, [_i32, _i32, _i32]),
    "kgat_rgcn_scratch_bytes": (_sz, [_i64, _i64, _i32, _i32, _i32, _i32]),
    "kgat_rgcn_fwd_f32": (_i32, [_i64, _i64, _i32, _i32, _i32, _p, _p, _p, _p, _p, _p, _p, _p, _p, _sz, _p]),
    "kgat_rgcn_bwd_x_f32": (_i32, [_i64, _i64, _i32, _i32, _i32, _p, _p, _p, _p, _p, _p, _p, _p, _p, _sz, _p]),
    "kgat_rgcn_bwd_coef_f32": (_i32, [_i64, _i64, _i32, _i32, _i32, _p, _p, _p, _p, _p, _p, _p, _p, _p, _sz, _p]),
    # TransE KG embedding (the CFKG baseline): reference models.py:114-133 without the projection, kgat.py:116-136
    # (ABI 16, additive)
    "kgat_transe_supported": (_i32, [_i64, _i32, _i32, _i64]),
    "kgat_transe_scratch_bytes": (_sz, [_i64, _i32, _i32]),
    "kgat_transe_sorted_bytes": (_sz, [_i64, _i32]),
    "kgat_transe_forward_f32": (_i32, [_i64, _i32, _i32, _i64, _p, _p, _p, _p, _p, _p, C.c_float, _p, _p, _sz, _p]),
    "kgat_transe_backward_f32": (_i32, [_i64, _i32, _i32, _i64, _p, _p, _p, _p, _p, _p, _p, _p, _sz, _p]),
    "kgat_transe_loss_grad_f32": (_i32, [_i64, _i32, _i32, _i64, _p, _p, _p, _p, _p, _p, C.c_float, _p, _p, _p, _p, _sz, _p]),
    "kgat_transe_presort_f32": (_i32, [_i64, _i32, _i64, _i64, _p, _p, _p, _p, _p, _sz, _p]),
    "kgat_transe_adam_step_f32": (_i32, [_i64, _i32, _i32, _i64, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, C.c_double,
                                         C.c_double, C.c_double, C.c_double, C.c_float, _p, _p, C.c_uint64, _p, _sz, _p]),
    # Bi-Interaction pooling over sparse feature sets (the FM / NFM baselines) and its dense backward (ABI 16, additive)
    "kgat_bi_pool_supported": (_i32, [_i32, _i64]),
    "kgat_bi_pool_scratch_bytes": (_sz, [_i64, _i64, _i64, _i64]),
    "kgat_bi_pool_fwd_f32": (_i32, [_i64, _i32, _i64, _i64, _i64, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p]),
    "kgat_bi_pool_bwd_f32": (_i32, [_i64, _i32, _i64, _i64, _i64, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _sz, _p]),
    # ripple-set attention of one hop (the RippleNet baseline): logits, softmax and the weighted sum of the tail rows in
    # one walk; backward towards the query table (ABI 16, additive)
    "kgat_ripple_supported": (_i32, [_i32, _i32, _i32, _i64]),
    "kgat_ripple_hop_fwd_f32": (_i32, [_i64, _i32, _i32, _i32, _i32, _i32, _i64, _i64, _p, _p, _p, _p, _p, _p, _p, _p, _p]),
    "kgat_ripple_hop_bwd_f32": (_i32, [_i64, _i32, _i32, _i32, _i32, _i32, _i64, _i64, _p, _p, _p, _p, _p, _p, _p, _p, _p,
                                       _p, _p]),
    # all-pairs evaluation of a one-hidden-layer NFM: MLP scores into the K best unseen items (ABI 16, additive)
    "kgat_nfm_eval_supported": (_i32, [_i32, _i32, _i32]),
    "kgat_nfm_eval_scratch_bytes": (_sz, [_i64, _i64, _i32, _i32, _i32]),
    "kgat_nfm_eval_topk_f32": (_i32, [_i64, _p, _i64, _i32, _i32, _p, _i64, _p, _p, _p, _p, _p, _p, _p, _p, _i32, _p, _sz,
                                      _p, _p, _p]),
    # all-pairs evaluation of RippleNet: per-user key table, then attention scores into the K best unseen items (ABI 16,
    # additive)
    "kgat_eval_ripple_supported": (_i32, [_i32, _i32, _i32, _i32, _i32]),
    "kgat_eval_ripple_keys_f32": (_i32, [_i64, _p, _i32, _i32, _i32, _i32, _i64, _i64, _p, _p, _p, _p, _p, _p]),
    "kgat_eval_ripple_scratch_bytes": (_sz, [_i64, _i64, _i32, _i32, _i32, _i32]),
    "kgat_eval_ripple_topk_f32": (_i32, [_i64, _p, _i64, _i32, _i32, _i32, _i32, _i32, _i64, _i64, _p, _p, _p, _p, _p, _p,
                                         _p, _i32, _p, _sz, _p, _p, _p]),
}

_lib = None


class KGATLibraryError(RuntimeError):
    pass


def _hipcc():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    return hipcc if os.path.exists(hipcc) else "hipcc"


BASE_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"]
OBJ_DIR = os.path.join(_HERE, "build")


ABI_VERSION = 16


def source_hash():
    """sha256[:16] over everything the library is built from: csrc/*, the public header, the
    compiler flags.  Embedded in the library at build time (kgat_build_hash) and compared at load
    time - file times do not survive a copy to another machine, content does."""
    h = hashlib.sha256()
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".hip", ".h")):
            with open(os.path.join(CSRC, f), "rb") as fh:
                h.update(f.encode() + b"\0" + fh.read())
    with open(HEADER, "rb") as fh:
        h.update(fh.read())
    h.update(repr((BASE_FLAGS, sorted(SOURCES.items()))).encode())
    return h.hexdigest()[:16]


def built_hash():
    """The hash embedded in the library on disk (read from the file, no dlopen), or None."""
    try:
        with open(SO_PATH, "rb") as fh:
            blob = fh.read()
    except OSError:
        return None
    tag = b"kgat-src-hash:"
    i = blob.find(tag)
    return blob[i + len(tag):i + len(tag) + 16].decode("ascii", "replace") if i >= 0 else None


def needs_build():
    return built_hash() != source_hash()


def _unit_hash(src, flags):
    """Key of one object file: its source, every header it may include, its flags."""
    h = hashlib.sha256()
    for f in [src] + sorted(f for f in os.listdir(CSRC) if f.endswith(".h")):
        with open(os.path.join(CSRC, f), "rb") as fh:
            h.update(f.encode() + b"\0" + fh.read())
    with open(HEADER, "rb") as fh:
        h.update(fh.read())
    h.update(repr(flags).encode())
    return h.hexdigest()


def build(force=False):
    """Compile the HIP sources for gfx950 in-tree (hipcc cross-compiles without a GPU): one
    object per source (per-file flags; an object whose inputs did not change is kept), then one
    shared library.  The source hash is compiled into kgat_graph.hip (kgat_build_hash).

    Safe under a multi-rank launch after a source edit: the build holds an exclusive lock on a
    file in the object directory (the other ranks wait, then find the library fresh), and objects
    and the library are written under temporary names and moved into place atomically, so no
    process can dlopen a half-written file."""
    if not (force or needs_build()):
        return SO_PATH
    import fcntl
    os.makedirs(OBJ_DIR, exist_ok=True)
    with open(os.path.join(OBJ_DIR, ".build.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            if not (force or needs_build()):  # another process built it while this one waited
                return SO_PATH
            return _build_locked(force)
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)


def _build_locked(force):
    procs, objs = [], []
    tag = '-DKGAT_BUILD_HASH="kgat-src-hash:%s"' % source_hash()
    for src, extra in SOURCES.items():
        obj = os.path.join(OBJ_DIR, src.replace(".hip", ".o"))
        objs.append(obj)
        flags = BASE_FLAGS + extra + ([tag] if src == "kgat_graph.hip" else [])
        key = _unit_hash(src, flags)
        try:
            with open(obj + ".key") as fh:
                fresh = os.path.exists(obj) and fh.read() == key
        except OSError:
            fresh = False
        if fresh and not force:
            continue
        tmp = "%s.%d.tmp" % (obj, os.getpid())
        procs.append((subprocess.Popen([_hipcc()] + flags + ["-c", os.path.join(CSRC, src), "-o", tmp]), obj, tmp, key))
    failed = None
    for p, obj, tmp, key in procs:
        if p.wait() != 0:
            failed = failed or subprocess.CalledProcessError(p.returncode, p.args)
            continue
        os.replace(tmp, obj)
        with open(obj + ".key.tmp", "w") as fh:
            fh.write(key)
        os.replace(obj + ".key.tmp", obj + ".key")
    if failed is not None:
        raise failed
    so_tmp = "%s.%d.tmp" % (SO_PATH, os.getpid())
    subprocess.check_call([_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", so_tmp] + objs)
    os.replace(so_tmp, SO_PATH)
    return SO_PATH


def _under_profiler():
    """rocprofv3 / rocprof run their target with a tool library preloaded (and ROCPROF* / ROCP_* variables set)."""
    pre = os.environ.get("LD_PRELOAD", "")
    return "rocprof" in pre.lower() or any(k.startswith(("ROCPROF", "ROCP_TOOL", "ROCPROFILER")) for k in os.environ)


def load():
    """dlopen libkgat_hip.so and bind every declared symbol.  `import torch` must have
    happened first so that libamdhip64 resolves to the runtime torch already loaded (one HIP
    runtime per process - streams and pointers are shared with torch).  A library that is
    missing or was built from other sources than the ones beside it is rebuilt (hipcc
    cross-compiles); if that fails, loading fails - there is no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    import torch  # noqa: F401  (loads torch's libamdhip64.so first)
    if needs_build():
        if _under_profiler():
            # a rebuild would spawn hipcc from inside the profiled process: its children inherit the profiler's
            # preload, which initialises the GPU before hipcc execs clang - the launcher hop this pool forbids
            raise KGATLibraryError(
                "libkgat_hip.so (%s) is missing or stale and this process runs under a profiler preload: build first "
                "(`python -c 'import __graft_entry__ as g; g.build()'`), then profile" % SO_PATH)
        try:
            build()
        except (OSError, subprocess.CalledProcessError) as e:
            raise KGATLibraryError(
                "libkgat_hip.so (%s) is %s and rebuilding it failed (%s). Run `python -c 'import "
                "__graft_entry__ as g; g.build()'`; there is no CPU or PyTorch fallback for this path."
                % (SO_PATH, "missing" if not os.path.exists(SO_PATH) else "stale (built from other sources)", e)) from e
    try:
        lib = C.CDLL(SO_PATH, mode=C.RTLD_GLOBAL)
    except OSError as e:
        raise KGATLibraryError("cannot load %s: %s" % (SO_PATH, e)) from e
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise KGATLibraryError("libkgat_hip.so lacks symbol %s" % name) from e
        fn.restype, fn.argtypes = res, args
    if lib.kgat_version() != ABI_VERSION:
        raise KGATLibraryError("libkgat_hip.so ABI version %d != %d" % (lib.kgat_version(), ABI_VERSION))
    got = lib.kgat_build_hash().decode()
    if got != "kgat-src-hash:" + source_hash():
        raise KGATLibraryError("libkgat_hip.so was built from other sources (%s) than the ones beside it (%s)"
                               % (got, source_hash()))
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().kgat_last_error()
        raise KGATLibraryError("%s failed (%d): %s" % (what, rc, msg.decode() if msg else ""))
