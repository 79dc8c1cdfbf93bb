// Every `int t3d_*(...)` that include/t3d.h declares, once.
//
// A new entry point:  declare it in include/t3d.h, add ONE line here -- S(name) when a recorded step may contain it (an
// enqueue call of the train / inference step), Q(name) otherwise (size and flag queries, the loaders' calls, t3d_plan_*) --
// and that is all.  From this list and the header's declaration the compiler makes
//   - the plan's replay thunk and arity (csrc/plan.hip: kEntries, the S group),
//   - the argument-type string the Python binding sets `argtypes` from (csrc/abi.hip -> t3d_abi_entry -> torchdet3d/_native.py).
// A name that the header does not declare does not compile; one that the header declares and this list lacks fails
// tests/test_abi.py, as does an exported symbol that neither has.
#ifndef T3D_ABI_ENTRIES_H_
#define T3D_ABI_ENTRIES_H_

#define T3D_ABI_ENTRIES(S, Q) \
  /* the calls a step may contain */ \
  S(t3d_dwconv_fwd) S(t3d_bn_finalize) S(t3d_bn_eval_affine) S(t3d_bn_eval_affine_batched) \
  S(t3d_pwconv_fwd) S(t3d_pwconv_dgrad) S(t3d_pack_weight) \
  S(t3d_set_dw_slots) S(t3d_set_exact_pool) S(t3d_sum_slots_batched) S(t3d_dwconv_bwd) \
  S(t3d_pwconv_wgrad) S(t3d_pwconv_yfree_prep) S(t3d_pwconv_dgrad_yfree) S(t3d_pwconv_wgrad_yfree) \
  S(t3d_pwconv_yfree_prep2) S(t3d_pwconv_bwd_yfree) S(t3d_pwconv_bwd_yfree_w) S(t3d_pwconv_wgrad_yfree_finish) \
  S(t3d_bn_bwd_finalize) S(t3d_stem_im2col) S(t3d_stem_im2col_u8) S(t3d_crop_resize_u8) \
  S(t3d_pwconv_fwd_mat) S(t3d_im2col) S(t3d_im2col_nchw) S(t3d_col2im_bwd) S(t3d_pack_conv_weight) \
  S(t3d_unpack_conv_grad) S(t3d_maxpool_fwd) S(t3d_maxpool_bwd) S(t3d_res_relu_fwd) \
  S(t3d_res_relu_bwd) S(t3d_subsample) S(t3d_ir_block_eval) S(t3d_bn_apply) S(t3d_bn_act_bwd) \
  S(t3d_gap_fwd) S(t3d_pool_fwd) S(t3d_pool_bwd) S(t3d_head_fwd) \
  S(t3d_linear_fwd) S(t3d_head_fwd_all) S(t3d_head_bwd) S(t3d_head_bwd_weights) \
  S(t3d_se_fwd_fused) S(t3d_se_bwd_data) S(t3d_se_bwd_weights) S(t3d_se_after_sums) \
  S(t3d_se_after_apply) S(t3d_se_after_bwd) S(t3d_set_reduction_replicas) S(t3d_set_workspace) S(t3d_set_main_workspace) \
  S(t3d_fold_request) S(t3d_pack_weights_batched) S(t3d_pwconv_pack_frag) S(t3d_adamw_step) S(t3d_set_grad_watch) \
  S(t3d_sgd_step) S(t3d_rmsprop_step) S(t3d_adadelta_step) \
  S(t3d_zero_batched) S(t3d_copy_cols) S(t3d_bn_bias_grad) S(t3d_se_bwd_affine) S(t3d_dropout_mask) \
  S(t3d_loss_fwd_bwd) S(t3d_metrics_per_sample) S(t3d_iou3d) S(t3d_box_iou3d) S(t3d_ssd_decode_nms) \
  S(t3d_expdw_fwd) S(t3d_track_step) S(t3d_ssd_select_rects) S(t3d_head_select) S(t3d_track_kp_to_frame) \
  S(t3d_objectron_pairs) S(t3d_objectron_hitmiss) S(t3d_draw_overlays_u8) S(t3d_ssd_multibox_loss) \
  S(t3d_ssd_head_bwd) S(t3d_ssd_cap_per_image) S(t3d_coco_match) \
  /* the rest: queries that return sizes / flags / routes, process-wide aids, the loaders' calls, the plan's own interface */ \
  Q(t3d_version) Q(t3d_pwconv_frag_bytes) Q(t3d_pwconv_wants_frag) Q(t3d_pwconv_route) Q(t3d_pwconv_force_route) \
  Q(t3d_pwconv_bwd_yfree_scratch) Q(t3d_dwconv_route) Q(t3d_dwconv_plan) Q(t3d_dwconv_force_route) \
  Q(t3d_augment_crops_u8) Q(t3d_augment_resized_u8) Q(t3d_augment_chain_crops_u8) Q(t3d_augment_chain_resized_u8) \
  Q(t3d_detect_augment_u8) Q(t3d_detect_draw) Q(t3d_detect_draw_host) Q(t3d_jpeg_index) Q(t3d_jpeg_decode_work_bytes) Q(t3d_jpeg_decode_u8) Q(t3d_jpeg_decode_roi_u8) \
  Q(t3d_detect_roi_plan) \
  Q(t3d_detect_roi_plan_host) \
  Q(t3d_jpeg_header) Q(t3d_jpeg_index_work_bytes) Q(t3d_jpeg_index_device) \
  Q(t3d_jpeg_encode_setup)Q(t3d_jpeg_encode_work_bytes) Q(t3d_jpeg_encode_u8) \
  Q(t3d_ssd_multibox_work_bytes) Q(t3d_ssd_head_bwd_work_bytes) Q(t3d_track_state_bytes) Q(t3d_track_lds_bytes) \
  Q(t3d_draw_glyphs) Q(t3d_set_launch_events) Q(t3d_fold_pending) Q(t3d_expdw_supported) \
  Q(t3d_plan_create) Q(t3d_plan_destroy) Q(t3d_plan_add_call) Q(t3d_plan_add_fork) Q(t3d_plan_add_fork_after) \
  Q(t3d_launch_count) Q(t3d_plan_add_copy_d2h) Q(t3d_plan_add_event_record) Q(t3d_plan_end_segment) \
  Q(t3d_plan_num_ops) Q(t3d_plan_time_entry) Q(t3d_plan_failed_op) Q(t3d_plan_run) \
  Q(t3d_abi_entry) Q(t3d_abi_struct)

#endif /* T3D_ABI_ENTRIES_H_ */
