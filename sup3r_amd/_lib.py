"""ctypes binding of ``libsup3r_hip.so`` (include/sup3r_hip.h).

This is the only compute back-end of the package: there is no CPU fallback.
If the shared library is missing or a call fails, a ``RuntimeError`` naming the
problem is raised — nothing is silently routed elsewhere.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# SUP3R_AMD_LIB: alternative build of the same library (A/B kernel probes)
LIB_PATH = os.environ.get('SUP3R_AMD_LIB') or os.path.join(
    HERE, 'lib', 'libsup3r_hip.so')

# enums (include/sup3r_hip.h)
PREC_F32, PREC_BF16, PREC_BF16X3 = 0, 1, 2
LOSS_MAE, LOSS_MSE, LOSS_EXP = 0, 1, 2
BUF_W, BUF_G, BUF_M, BUF_V = 0, 1, 2, 3
OPT_ADAM = 0
SURF_OTHER, SURF_TEMP, SURF_PRES, SURF_RH = 0, 1, 2, 3
E_TIMEOUT = -6
PRECISIONS = {'f32': PREC_F32, 'bf16': PREC_BF16, 'bf16x3': PREC_BF16X3}

EXPORTS = [
    's3_ctx_create', 's3_ctx_destroy', 's3_last_error', 's3_ctx_sync',
    's3_ctx_stream', 's3_ctx_stat', 's3_params_create', 's3_params_destroy',
    's3_params_total', 's3_params_set', 's3_params_get', 's3_params_dptr',
    's3_params_zero_grad', 's3_params_version', 's3_params_mean_abs',
    's3_adam_step', 's3_optimizer_step', 's3_optimizer_stage',
    's3_optimizer_step_staged', 's3_params_touch', 's3_capture_begin',
    's3_capture_end', 's3_capture_abort', 's3_graph_launch', 's3_graph_nodes',
    's3_graph_destroy',
    's3_ctx_set_option', 's3_ctx_get_option', 's3_option_name_at',
    's3_plan_create', 's3_plan_create_opt', 's3_plan_destroy', 's3_plan_forward',
    's3_plan_supports_window', 's3_plan_forward_window',
    's3_plan_backward', 's3_plan_tensor', 's3_plan_workspace_bytes',
    's3_plan_profile_begin', 's3_plan_profile_end',
    's3_plan_op_is_mfma', 's3_plan_op_info', 's3_plan_tensor_dtype', 's3_plan_tensor_read',
    's3_loss_content', 's3_loss_content_masked', 's3_loss_rel_bce',
    's3_lossmap_fwd', 's3_lossmap_bwd', 's3_loss_mmd',
    's3_loss_sliced_wasserstein', 's3_sw_directions', 's3_time_window',
    's3_time_mean', 's3_dft_axis',
    's3_specmap',
    's3_copy_channels', 's3_affine_channels', 's3_fill', 's3_copy_block',
    's3_coarsen', 's3_gaussian_smooth', 's3_condmom_target', 's3_bias_correct', 's3_chunk_stats',
    's3_bc_base_series', 's3_bc_moments', 's3_bc_window_quantiles',
    's3_bc_match_zero_rate', 's3_bc_presrat', 's3_bc_skill',
    's3_sample_gather', 's3_cc_night_mask', 's3_cc_window_gather',
    's3_nn_fill', 's3_channel_moments', 's3_normalize_channels',
    's3_st_interp', 's3_resize2d', 's3_surface_downscale',
    's3_chunk_epilogue', 's3_chunk_time_last', 's3_chunk_time_first',
    's3_step_handover', 's3_broadcast_axis', 's3_branch_join',
    's3_time_pad_reflect',
    's3_host_register', 's3_host_unregister', 's3_d2h_window',
    's3_d2h_stream', 's3_host_alloc', 's3_host_free', 's3_d2h_async',
    's3_dma_d2h_begin', 's3_dma_wait',
    's3_invert_uv', 's3_clip_channels', 's3_range_mask', 's3_fill_indexed',
    's3_level_interp', 's3_derive_pointwise', 's3_time_flags',
    's3_stack_features', 's3_level_stats',
    's3_exo_nearest_work_bytes', 's3_exo_nearest',
    's3_exo_group_mean_work_bytes', 's3_exo_group_mean',
    's3_qa_recoarsen', 's3_qa_select', 's3_qa_hist', 's3_qa_power_sum',
    's3_raster_gather', 's3_daily_reduce', 's3_site_day_mean',
    's3_scale_to_time_max',
    's3_regrid_knn_work_bytes', 's3_regrid_knn', 's3_regrid_apply',
    's3_comm_unique_id', 's3_comm_init', 's3_params_allreduce_grads',
    's3_params_arm_allreduce',
    's3_allreduce_sum', 's3_params_broadcast', 's3_broadcast',
    's3_comm_destroy', 's3_comm_wait', 's3_comm_info', 's3_version',
]


OPTION_UNSET = -2 ** 31


class PlanOptions(C.Structure):
    _fields_ = [('n', C.c_int32), ('names', C.POINTER(C.c_char_p)),
                ('values', C.POINTER(C.c_int32))]


class TensorDesc(C.Structure):
    _fields_ = [('dims', C.c_int64 * 5)]


class BiasChannel(C.Structure):
    """``s3_bias_channel``: the per-channel descriptor of s3_bias_correct"""
    _fields_ = [
        ('kind', C.c_int32), ('flags', C.c_uint32), ('n_t', C.c_int32),
        ('n_q', C.c_int32), ('scalar', C.c_void_p), ('adder', C.c_void_p),
        ('oh', C.c_void_p), ('mh', C.c_void_p), ('mf', C.c_void_p),
        ('tau', C.c_void_p), ('kfac', C.c_void_p),
        ('scalar_lo', C.c_float), ('scalar_hi', C.c_float),
        ('adder_lo', C.c_float), ('adder_hi', C.c_float),
        ('out_lo', C.c_float), ('out_hi', C.c_float),
        ('delta_lo', C.c_float), ('delta_hi', C.c_float),
        ('denom_min', C.c_float), ('denom_zero', C.c_float),
    ]


class OpDesc(C.Structure):
    _fields_ = [
        ('kind', C.c_int32), ('in0', C.c_int32), ('in1', C.c_int32),
        ('res', C.c_int32), ('out', C.c_int32), ('w', C.c_int32),
        ('b', C.c_int32), ('k', C.c_int32 * 3), ('stride', C.c_int32 * 3),
        ('lo', C.c_int32 * 3), ('hi', C.c_int32 * 3), ('pad_mode', C.c_int32),
        ('act', C.c_int32), ('alpha', C.c_float), ('d2s', C.c_int32),
        ('rep', C.c_int32), ('bcast_c', C.c_int32),
        ('reserved', C.c_int32 * 4),
    ]


_lib = None


def build_hint():
    return ('build it with `python -c "import __graft_entry__ as g; '
            'g.build()"` or `make -C sup3r_amd/csrc` (needs hipcc)')


def lib():
    """Load (once) and return the ctypes handle of libsup3r_hip.so."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f'sup3r_amd: HIP library {LIB_PATH} not found; {build_hint()}. '
            'There is no CPU fallback.')
    # torch first: its wheel bundles its own libamdhip64 / libhsa-runtime64.
    # Loading ours (linked against /opt/rocm) before torch's leaves two HIP
    # runtimes in the process and hipSetDevice then reports "no ROCm-capable
    # device"; after torch, the already-loaded runtime is shared.
    import torch  # noqa: F401
    L = C.CDLL(LIB_PATH)
    vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    u64 = C.c_uint64
    pf = C.POINTER(C.c_float)
    sig = {
        's3_ctx_create': (i32, [i32, vp, i32, C.POINTER(vp)]),
        's3_ctx_destroy': (None, [vp]),
        's3_last_error': (C.c_char_p, [vp]),
        's3_ctx_sync': (i32, [vp]),
        's3_ctx_stream': (vp, [vp]),
        's3_ctx_stat': (i64, [vp, i32]),
        's3_params_create': (i32, [vp, i32, C.POINTER(i64), C.POINTER(vp)]),
        's3_params_destroy': (None, [vp]),
        's3_params_total': (i64, [vp]),
        's3_params_set': (i32, [vp, i32, i32, pf]),
        's3_params_get': (i32, [vp, i32, i32, pf]),
        's3_params_dptr': (vp, [vp, i32, i32]),
        's3_params_zero_grad': (i32, [vp]),
        's3_params_version': (u64, [vp]),
        's3_params_mean_abs': (i32, [vp, i32, i32, pf]),
        's3_adam_step': (i32, [vp, f32, f32, f32, f32, i64]),
        's3_optimizer_step': (i32, [vp, i32, C.POINTER(C.c_double), i32, i64]),
        's3_optimizer_stage': (i32, [vp, i32, C.POINTER(C.c_double), i32, i64]),
        's3_optimizer_step_staged': (i32, [vp, i32]),
        's3_params_touch': (i32, [vp]),
        's3_capture_begin': (i32, [vp]),
        's3_capture_end': (i32, [vp, C.POINTER(vp)]),
        's3_capture_abort': (i32, [vp]),
        's3_graph_launch': (i32, [vp]),
        's3_graph_nodes': (i64, [vp]),
        's3_graph_destroy': (None, [vp]),
        's3_plan_create': (i32, [vp, vp, C.POINTER(TensorDesc), i32,
                                 C.POINTER(OpDesc), i32, C.POINTER(i32), i32,
                                 i32, i32, i32, C.POINTER(vp)]),
        's3_plan_create_opt': (i32, [vp, vp, C.POINTER(TensorDesc), i32,
                                     C.POINTER(OpDesc), i32, C.POINTER(i32),
                                     i32, i32, i32, i32,
                                     C.POINTER(PlanOptions), C.POINTER(vp)]),
        's3_ctx_set_option': (i32, [vp, C.c_char_p, i32]),
        's3_ctx_get_option': (i32, [vp, C.c_char_p, C.POINTER(i32)]),
        's3_option_name_at': (C.c_char_p, [i32]),
        's3_plan_destroy': (None, [vp]),
        's3_plan_forward': (i32, [vp, C.POINTER(vp), vp]),
        's3_plan_supports_window': (i32, [vp]),
        's3_plan_forward_window': (i32, [vp, C.POINTER(vp), vp,
                                         C.POINTER(i64), C.POINTER(i64), vp,
                                         i32]),
        's3_plan_backward': (i32, [vp, vp, vp, i32, i32]),
        's3_plan_tensor': (vp, [vp, i32]),
        's3_plan_workspace_bytes': (i64, [vp]),
        's3_plan_profile_begin': (i32, [vp, i32]),
        's3_plan_profile_end': (i32, [vp, pf, i32]),
        's3_plan_op_is_mfma': (i32, [vp, i32]),
        's3_plan_op_info': (i32, [vp, i32, C.POINTER(i32), i32]),
        's3_plan_tensor_dtype': (i32, [vp, i32]),
        's3_plan_tensor_read': (i64, [vp, i32, vp, C.c_size_t]),
        's3_loss_content': (i32, [vp, i32, vp, i32, vp, i32, i32, i64, f32,
                                  vp, vp, i32]),
        's3_loss_content_masked': (i32, [vp, i32, vp, i32, vp, i32, vp, i32,
                                         i32, i64, f32, vp, vp, i32]),
        's3_loss_rel_bce': (i32, [vp, vp, vp, i32, f32, vp, vp, vp]),
        's3_lossmap_fwd': (i32, [vp, i32, vp, i32, i32, i32, i32, i32, i32,
                                 i32, i32, i32, vp, vp]),
        's3_lossmap_bwd': (i32, [vp, i32, vp, vp, vp, i32, i32, i32, i32, i32,
                                 i32, i32, i32, i32, vp, vp]),
        's3_loss_mmd': (i32, [vp, vp, i32, vp, i32, i32, i64, i32, f32, f32,
                              vp, vp]),
        's3_loss_sliced_wasserstein': (i32, [vp, vp, i32, vp, i32, i32, i64,
                                             i32, i32, u64, f32, vp, vp]),
        's3_sw_directions': (i32, [vp, u64, i32, i64, vp]),
        's3_time_window': (i32, [vp, vp, i64, i32, i32, i32, i32, vp, i32,
                                 f32]),
        's3_time_mean': (i32, [vp, vp, i64, i32, i32, i32, i32, vp, i32, f32]),
        's3_dft_axis': (i32, [vp, vp, vp, vp, vp, i64, i32, i64, i32]),
        's3_specmap': (i32, [vp, i32, vp, vp, vp, i32, i32, i32, i32, i32,
                             i32, vp, vp]),
        's3_copy_channels': (i32, [vp, vp, i32, i32, vp, i32, i32, i32, i64,
                                   i32]),
        's3_affine_channels': (i32, [vp, vp, vp, i32, i64, pf, pf]),
        's3_fill': (i32, [vp, vp, i64, f32]),
        's3_copy_block': (i32, [vp, vp, vp, i64, i64, i64, i64, i64, i64, i64]),
        's3_chunk_stats': (i32, [vp, vp, i32, i64, i32, vp]),
        's3_chunk_epilogue': (i32, [vp, vp, i32, C.POINTER(i64),
                                    C.POINTER(i64), C.POINTER(i64), i32, pf,
                                    pf, vp, vp]),
        's3_chunk_time_first': (i32, [vp, vp, i32, C.POINTER(i64), i32,
                                      C.POINTER(C.c_double),
                                      C.POINTER(C.c_double), i32, vp]),
        's3_broadcast_axis': (i32, [vp, vp, i64, i64, i64, i64, vp]),
        's3_step_handover': (i32, [vp, vp, i64, i32, C.POINTER(i32), i32, pf,
                                   pf, vp, i32, pf, pf, vp]),
        's3_branch_join': (i32, [vp, vp, i32, C.POINTER(i32), i32, pf, pf,
                                 vp, i32, C.POINTER(i32), i32, pf, pf, i64,
                                 i64, i64, pf, pf, vp]),
        's3_time_pad_reflect': (i32, [vp, vp, i64, i64, i32, i64, pf, pf,
                                      vp]),
        's3_chunk_time_last': (i32, [vp, vp, i32, C.POINTER(i64),
                                     C.POINTER(i64), C.POINTER(i64), i32, pf,
                                     pf, vp]),
        's3_invert_uv': (i32, [vp, vp, i64, i64, i32, i32, i32, vp, vp]),
        's3_clip_channels': (i32, [vp, vp, i32, i64, pf, pf]),
        's3_range_mask': (i32, [vp, vp, i32, i32, i64, f32, f32, vp]),
        's3_fill_indexed': (i32, [vp, vp, i32, i32, i64, vp, vp]),
        's3_level_interp': (i32, [vp, i64, i64, i32, i32, i32, vp, pf, vp, i32,
                                  pf, i32, C.POINTER(vp), C.POINTER(vp), i32,
                                  pf, i32, C.POINTER(vp)]),
        's3_derive_pointwise': (i32, [vp, i32, i64, i64, vp, vp, vp, vp, vp,
                                      f32, vp, vp]),
        's3_time_flags': (i32, [vp, i32, vp, i64, i64, i32, f32, vp]),
        's3_stack_features': (i32, [vp, C.POINTER(vp), i32, i64, i64, i64,
                                    vp]),
        's3_level_stats': (i32, [vp, vp, i64, i64, i32, vp, i32, f32, f32, vp]),
        's3_exo_nearest_work_bytes': (i64, [i64]),
        's3_exo_nearest': (i32, [vp, vp, i64, vp, i64, C.c_double, vp, i64,
                                 vp, vp]),
        's3_exo_group_mean_work_bytes': (i64, [i64, i64]),
        's3_exo_group_mean': (i32, [vp, vp, vp, i64, i64, i64, i64,
                                    C.POINTER(i32), C.c_double, vp, i64, vp,
                                    vp]),
        's3_qa_recoarsen': (i32, [vp, vp, i32, i64, i64, i64, i32,
                                  C.POINTER(i32), C.POINTER(i32), i32, i32,
                                  i32, C.POINTER(vp), C.POINTER(vp),
                                  C.POINTER(vp), vp]),
        's3_qa_select': (i32, [vp, vp, i32, i64, i64, i64, i64, i32, f32, f32,
                               f32, i64, i64, vp]),
        's3_qa_hist': (i32, [vp, vp, i32, i64, i64, i64, i64, i32, f32, f32,
                             f32, i32, f32, f32, f32, C.c_double, i32, i32,
                             vp, vp, vp]),
        's3_qa_power_sum': (i32, [vp, vp, vp, vp, vp, i64, i32, i64, vp]),
        's3_raster_gather': (i32, [vp, i32, i32, C.POINTER(vp), C.POINTER(vp),
                                   i64, i64, i64, i64, i64, i64, i64, i64,
                                   i64, i64, i64, vp]),
        's3_daily_reduce': (i32, [vp, i32, C.POINTER(vp), i64, i64, i32, i32,
                                  C.POINTER(i32), C.POINTER(i32),
                                  C.POINTER(i32), C.POINTER(vp)]),
        's3_site_day_mean': (i32, [vp, vp, i64, i64, vp, i64, i32, i64, i32,
                                   vp, i64, vp]),
        's3_scale_to_time_max': (i32, [vp, vp, vp, i64, i64, vp]),
        's3_regrid_knn_work_bytes': (i64, [i64]),
        's3_regrid_knn': (i32, [vp, vp, i64, vp, i64, i32, vp, i64, vp, vp,
                                vp]),
        's3_regrid_apply': (i32, [vp, i32, C.POINTER(vp), C.POINTER(vp), i64,
                                  i64, i64, i64, i32, vp, vp, vp]),
        's3_host_register': (i32, [vp, vp, C.c_size_t]),
        's3_host_unregister': (i32, [vp, vp]),
        's3_d2h_window': (i32, [vp, vp, vp, i64, i64, i64, i64, i64, vp]),
        's3_d2h_stream': (i32, [vp, vp, vp, C.c_size_t, vp, i32]),
        's3_host_alloc': (i32, [vp, C.c_size_t, i32, C.POINTER(vp)]),
        's3_host_free': (i32, [vp, vp]),
        's3_d2h_async': (i32, [vp, vp, vp, C.c_size_t, vp]),
        's3_dma_d2h_begin': (i32, [vp, vp, vp, C.c_size_t,
                                   C.POINTER(C.c_uint64)]),
        's3_dma_wait': (i32, [vp, C.c_uint64, i32]),
        's3_coarsen': (i32, [vp, vp, i32, i32, i32, i32, i32, i32, i32, i32,
                             vp]),
        's3_gaussian_smooth': (i32, [vp, vp, i32, i32, i32, i32, i32, pf, i32,
                                     C.c_uint32, vp, vp]),
        's3_condmom_target': (i32, [vp, vp, vp, vp, i32, i32, i32, i32, i32,
                                    i32, i32, C.POINTER(i32), i32, i32,
                                    C.c_uint32, i32, i32, i32, vp, vp]),
        's3_sample_gather': (i32, [vp, vp, i64, i64, i64, i32, C.POINTER(i32),
                                   i32, i32, i32, i32, C.POINTER(i32), i32,
                                   vp]),
        's3_cc_night_mask': (i32, [vp, vp, i64, i64, i64, i32, C.POINTER(i32),
                                   i32, i32, i32, i32, vp]),
        's3_cc_window_gather': (i32, [vp, vp, i64, i64, i64, i32,
                                      C.POINTER(i32), i32, i32, i32, i32,
                                      C.POINTER(i32), i32, vp, vp]),
        's3_nn_fill': (i32, [vp, vp, i32, i32, i32, i32, i32, i32, vp, vp]),
        's3_channel_moments': (i32, [vp, vp, i64, i32, vp]),
        's3_normalize_channels': (i32, [vp, vp, i64, i32, pf, pf,
                                        C.POINTER(C.c_ubyte)]),
        's3_bias_correct': (i32, [vp, vp, i32, i32, i32, i32, i32,
                                  C.POINTER(BiasChannel), i32, i32,
                                  C.POINTER(i32), vp, vp, vp,
                                  C.POINTER(C.c_double),
                                  C.POINTER(C.c_double), i32, vp, vp]),
        's3_bc_base_series': (i32, [vp, vp, vp, i64, i64, i32, vp, vp, vp, vp,
                                    i32, vp, vp, vp, vp, i32, C.c_uint32, i32,
                                    i64, i64, vp]),
        's3_bc_moments': (i32, [vp, vp, i32, i64, vp, vp, i32, vp, vp, vp]),
        's3_bc_window_quantiles': (i32, [vp, vp, i32, i64, i32, vp, vp, vp,
                                         vp, i32, vp]),
        's3_bc_match_zero_rate': (i32, [vp, vp, i64, vp, i32, i64, vp, vp]),
        's3_bc_presrat': (i32, [vp, vp, i64, vp, i64, vp, i64, i32, i32, i32,
                                vp, vp, vp, i32, C.c_double, vp, vp,
                                C.POINTER(vp), C.POINTER(vp), C.POINTER(vp),
                                C.POINTER(vp), vp, vp, vp, vp, vp, vp, vp]),
        's3_bc_skill': (i32, [vp, vp, i64, vp, i64, i32, i32, vp, vp, vp,
                              vp]),
        's3_st_interp': (i32, [vp, vp, i32, i32, i32, i32, i32, i32, i32, vp,
                               vp]),
        's3_resize2d': (i32, [vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp,
                              i32, vp, vp]),
        's3_surface_downscale': (i32, [vp, vp, i32, i32, i32, i32, i32, vp, vp,
                                       vp, vp, i32, vp, vp, vp, i32, vp, u64,
                                       C.c_uint32, vp, vp, vp, vp, vp, vp]),
        's3_comm_unique_id': (i32, [vp]),
        's3_comm_init': (i32, [vp, i32, i32, vp]),
        's3_params_allreduce_grads': (i32, [vp]),
        's3_params_arm_allreduce': (i32, [vp, i64]),
        's3_allreduce_sum': (i32, [vp, vp, i64]),
        's3_comm_info': (i32, [vp, C.POINTER(i32), C.POINTER(i32)]),
        's3_params_broadcast': (i32, [vp, i32, i32]),
        's3_broadcast': (i32, [vp, vp, i64, i32]),
        's3_comm_destroy': (None, [vp]),
        's3_comm_wait': (i32, [vp, i64]),
        's3_version': (C.c_char_p, []),
    }
    for name in EXPORTS:
        fn = getattr(L, name)   # AttributeError if the .so lacks a symbol
        fn.restype, fn.argtypes = sig[name]
    _lib = L
    return L


STATS = {'persist_dgrad': 0, 'gconv_splitk': 1, 'bucket_elems': 2,
         'dgrad_c2_slide': 3, 'buckets': 4, 'allreduces': 5,
         # support passes of the training step, one per kernel launched
         'bias_stage1': 6, 'bias_stage1_v4': 7, 'bias_cols': 8,
         'bias_cols_split': 9, 'bias_partial': 10, 'bias_partial_ride': 11,
         'bias_partial_flush': 12, 'epi_generic': 13, 'epi_c4': 14,
         'epi_d2s4': 15, 'epi_c4_bsum': 16, 'epi_d2s4_bsum': 17,
         'fold_gather': 18, 'fold_pad4': 19, 'fold_pad4_fr16': 20,
         'fold16x8': 21, 'fold_plain': 22, 'fold_masked': 23, 'fold_add': 24,
         'axpy': 25, 'axpy4': 26,
         # persistent trunk convs launched on the skip-prefetch variant
         'persist_skippre': 27,
         # in-family variants of the discriminator's conv kernels
         'halo_s2_k64': 28, 'fewch_halo': 29, 'fewch_halo_signs': 30,
         'dgrad_s2_o16': 31, 'dgrad_s2_mb': 32,
         # variants of the hi-res tail conv, forward and weight gradient
         'tail_tile': 33, 'tail_band': 34, 'tail_slide': 35, 'tail_sweep': 36,
         'tail_x3': 37, 'wgrad_tail_tile': 38, 'wgrad_tail_tile_in16': 39,
         'wgrad_tail_sweep': 40}


def option_names():
    """names of the context / plan options (include/sup3r_hip.h)"""
    L, out, i = lib(), [], 0
    while True:
        name = L.s3_option_name_at(i)
        if not name:
            return out
        out.append(name.decode())
        i += 1


def plan_options(options):
    """dict name -> int | None (None = unset) as an ``s3_plan_options``
    (+ the ctypes arrays it points into, to be kept alive by the caller)"""
    items = sorted((options or {}).items())
    n = len(items)
    names = (C.c_char_p * max(n, 1))(*[k.encode() for k, _ in items])
    values = (C.c_int32 * max(n, 1))(*[
        OPTION_UNSET if v is None else int(v) for _, v in items])
    return PlanOptions(n, names, values), (names, values)

# s3_plan_op_info fields / codes (include/sup3r_hip.h)
OPINFO_FIELDS = ('kind', 'fwd', 'in16', 'out16', 'res16', 'fwd_bf16_ops',
                 'wgrad', 'dgrad', 'mask_fused_from', 'in_rep', 'res_rep',
                 'dgrad_frame16', 'fewpos_mfma')
FWD_KERNELS = ('direct', 'mfma_tile', 'mfma_persist', 'gconv', 'gconv_fewch',
               'halo32', 'fewpos', 'tail_mfma', 'small', 'fused2d', 'halo_s2',
               'mfma_gen', 'conv2d_ws', 'conv2d_head')
WGRAD_KERNELS = ('direct', 'f32_trunk', 'bf16_trunk', 'f32_gen', 'bf16_gen',
                 'bf16_2d', 'c2', 'tail', 'fewpos')
DGRAD_KERNELS = ('direct', 'mfma_frame', 'mfma_valid', 'mfma_chunked',
                 'fewch_frame', 's2', 'c2', 'gconv', 'fewpos')

TC_METHODS = {'subsample': 0, 'average': 1, 'total': 2, 'max': 3, 'min': 4}
CM_SUBFILTER, CM_LINEAR, CM_MOM1, CM_SQUARE = 1, 2, 4, 8
# s3_sample_gather: samples per launch, channels kept (include/sup3r_hip.h)
SAMPLE_MAX_ORIGINS, SAMPLE_MAX_CHANNELS = 64, 32
# s3_channel_moments / s3_normalize_channels: channels of a cube
STATS_MAX_CHANNELS = 64
# DualSamplerCC's status words and the fill's largest extent (include/sup3r_hip.h)
CC_STATUS_WORDS = 4
CC_NIGHT_MASK, CC_START_RAW, CC_START, CC_FILLED = 0, 1, 2, 3
NN_FILL_MAX_AXIS = 2048
# s3_bias_correct: limits, channel kinds, flags (include/sup3r_hip.h)
BC_MAX_CHANNELS, BC_MAX_CHUNKS = 16, 32
BC_NONE, BC_LINEAR, BC_QDM = 0, 1, 2
(BC_MONTH, BC_WEIGHTS, BC_SCALAR_RANGE, BC_ADDER_RANGE, BC_OUT_RANGE,
 BC_PER_CHUNK, BC_RELATIVE, BC_NO_TREND, BC_DENOM_ZERO, BC_DENOM_MIN,
 BC_DELTA_RANGE, BC_PRESRAT, BC_GLOBAL) = (1 << i for i in range(13))
# s3_bc_*: sort limit, daily reductions, flags (include/sup3r_hip.h)
BCC_MAX_SORT, BCC_MAX_GROUPS = 32768, 12
BCC_AVG, BCC_MAX, BCC_MIN, BCC_SUM, BCC_NONE = range(5)
BCC_NANSKIP, BCC_CS_RATIO, BCC_ROUND = 1, 2, 4
BCC_PR_BIAS_NONFINITE, BCC_PR_FUT_NONFINITE, BCC_PR_INDEX = 0, 1, 2
BCC_SK_PERCENTILES, BCC_SK_STATS = 7, 13
(BCC_SK_MEAN, BCC_SK_STD, BCC_SK_SKEW, BCC_SK_KURTOSIS, BCC_SK_ZERO_RATE,
 BCC_SK_PCT0) = range(6)
BCC_SK_BIAS = 12
BCC_SK_KS_WORDS, BCC_SK_STATUS_WORDS, BCC_SK_NO_KS = 4, 4, -1
# s3_level_interp / s3_derive_pointwise / s3_time_flags / s3_stack_features:
# limits, methods, level sources, ops, modes (include/sup3r_hip.h)
LI_MAX_LEVELS, LI_MAX_SINGLE, LI_MAX_VARS, LI_MAX_TARGETS = 64, 8, 8, 16
LI_LINEAR, LI_LOG = 0, 1
LI_LEV_COLUMN, LI_LEV_VECTOR = 0, 1
(DP_UV_FROM_WSWD, DP_WSWD_FROM_UV, DP_SURFACE_RH, DP_RATIO_MASKED,
 DP_CLOUD_MASK, DP_RATIO_CLIP01, DP_ADD, DP_SCALE, DP_OFFSET, DP_BCAST_PIXEL,
 DP_BCAST_TIME) = range(11)
TF_LE, TF_NAN = 0, 1
STACK_MAX_PLANES = 32
LS_WORDS = 8
(LS_NAN, LS_BAD_MIN, LS_BAD_MAX, LS_ALL_NAN, LS_FIRST_MAX, LS_FIRST_MIN,
 LS_LAST_MAX, LS_LAST_MIN) = range(8)
# s3_exo_group_mean: most columns of one slab (include/sup3r_hip.h)
EXO_MAX_SLAB = 32
# s3_qa_*: layouts, limits, the summary's words, flags (include/sup3r_hip.h)
QA_CUBE, QA_TIME_FIRST = 0, 1
QA_MAX_FEATURES, QA_SUMMARY_WORDS, QA_MAX_BINS = 16, 5, 4096
QA_HIST_STATS, QA_HIST_COUNTS, QA_HIST_KEEP_ALL = 1, 2, 4
# s3_raster_gather / s3_daily_reduce: layouts, limits, ops (include/sup3r_hip.h)
RG_GRID, RG_FLAT, RG_FLAT_1D = 0, 1, 2
DAILY_MAX_SRC, DAILY_MAX_OUT = 8, 16
DAILY_MEAN, DAILY_MAX, DAILY_MIN, DAILY_SUM, DAILY_RATIO = range(5)
# s3_regrid_knn / s3_regrid_apply: most neighbours (include/sup3r_hip.h)
REGRID_MAX_K = 8


def last_error(ctx):
    """text of the context's last error ('' if none)"""
    raw = lib().s3_last_error(ctx) if ctx else None
    return raw.decode() if raw else ''


def check(rc, ctx=None, what=''):
    if rc == 0:
        return
    msg = ''
    if ctx:
        raw = lib().s3_last_error(ctx)
        msg = raw.decode() if raw else ''
    if rc == E_TIMEOUT:
        raise TimeoutError(f'sup3r_amd: {msg or what}')
    raise RuntimeError(f'sup3r_amd HIP call failed ({what}, code {rc}): {msg}')
