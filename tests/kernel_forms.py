"""Every option of gpsig_set_option (csrc/api.hip; documented in include/gpsig_hip.h) and what tests the kernel forms it selects.

A plain module, no tests in it: tests/test_kernel_forms_registry.py checks on the CPU that the option names parsed from the C ABI's
strcmp chain are exactly the keys below, that every named test function exists in its file, and that every recorded default is the
initialiser of the option's field in csrc/ctx.hpp.  A new option therefore fails the CPU suite until it is entered here with the tests
that run each of its values, or with a one-line reason why it selects no kernel form of its own.

Each entry is either
    {"default": <ctx.hpp initialiser>, "values": [<values the tests set>], "tests": ["<file>::<test function>", ...]}
or
    {"default": <ctx.hpp initialiser>, "exempt": "<one-line reason>"}.
"""

_P = "test_gpu_parity.py::"
_G = "test_gpu_grad.py::"
_W = "test_gpu_wide.py::"
_F = "test_gpu_kernel_forms.py::"
_L = "test_gpu_lowrank_spectral.py::"
_I = "test_gpu_grad_instances.py::"

OPTIONS = {
    "glds": {"default": 1, "values": [0, 1], "tests": [_P + "test_lds_dma_staging_and_generic_kernels_agree_bitwise"]},
    "exact": {"default": 1, "values": [0, 1], "tests": [_P + "test_lds_dma_staging_and_generic_kernels_agree_bitwise", _P + "test_exact_higher_order_rbf_instances"]},
    "max_run": {"default": 0, "values": [0, 1, 3], "tests": [_P + "test_lds_dma_staging_and_generic_kernels_agree_bitwise", _P + "test_shards_partition_the_gram"]},
    "tensor_lanes": {"default": -1, "values": [-1, 0, 1], "tests": [_P + "test_tensor_vs_sequence_lane_mappings_agree"]},
    "grad_scratch_mb": {"default": 4096, "exempt": "a memory budget, not a kernel form: chunked launches are covered by test_gpu_grad.py (test_seq_level_gradients_are_chunk_invariant)"},
    "grad_impl": {"default": 0, "values": [0, 1, 2, 3, 4], "tests": [_G + "test_wave_and_storage_gradient_kernels_agree", _G + "test_tensor_level_gradients",
                                                                     _G + "test_stationary_kernels_reverse_pass_in_one_launch", _G + "test_higher_order_reverse_pass_in_two_sweeps",
                                                                     _F + "test_fused_reverse_kernel_edges", _I + "test_every_compiled_sweep_instance_against_the_oracle"]},
    "grad_stash_mb": {"default": 4096, "values": [0, 4096], "tests": [_G + "test_forward_pass_keeps_what_its_reverse_pass_needs"]},
    "matern_fast": {"default": 1, "values": [0, 1], "tests": [_P + "test_matern_families_at_compile_time_in_the_sequence_gram", _F + "test_keep_reset_in_the_float64_pair_kernel"]},
    "grad_fused_piece": {"default": 0, "values": [0, 1, 3, 16, 17, 64], "tests": [_F + "test_grad_fused_piece"]},
    "tvs_zreg": {"default": -1, "values": [-1, 0, 1], "tests": [_F + "test_tvs_zreg_in_the_tensor_lane_gradient"]},
    "tvs_grad_tile": {"default": 1, "values": [0, 1], "tests": [_G + "test_tensor_vs_sequence_tile_gradient_kernel", _F + "test_tvs_zreg_in_the_tensor_lane_gradient"]},
    "pinned_staging": {"default": 1, "values": [0, 1], "tests": [_F + "test_pinned_staging_in_host_pointer_mode"]},
    "lr_jacobi": {"default": 1, "values": [0, 1], "tests": [_P + "test_low_rank_objects_drawn_on_the_device", "test_gpu_draw_edges.py::test_eigendecomposition_backward_error"]},
    "sig_features": {"default": -1, "values": [-1, 0, 1], "tests": [_P + "test_linear_gram_as_feature_contraction", _F + "test_keep_reset_in_the_float64_pair_kernel"]},
    "sig_gemm_dma": {"default": 1, "values": [0, 1], "tests": [_P + "test_linear_gram_as_feature_contraction"]},
    "sig_graded": {"default": 1, "values": [0, 1], "tests": [_F + "test_sig_graded_pieces"]},
    "lr_grad_threads": {"default": 1024, "values": [512, 1024], "tests": [_F + "test_lr_grad_threads"]},
    "sig_features_grad": {"default": -1, "values": [-1, 0, 1], "tests": [_G + "test_linear_level_gradients_through_the_feature_contraction", _G + "test_level_sum_gradient_as_one_op"]},
    "sig_features_keep": {"default": 0, "values": [0, 1], "tests": [_P + "test_compact_row_blocks_reassemble_the_symmetric_gram"]},
    "keep_reset": {"default": 1, "values": [0, 1], "tests": [_F + "test_keep_reset_in_the_float64_pair_kernel", _F + "test_keep_reset_in_the_float32_packed_kernel"]},
    "pk2": {"default": 1, "values": [0, 1, 2], "tests": [_P + "test_float32_packed_kernels", _F + "test_keep_reset_in_the_float32_packed_kernel"]},
    "f32_pack": {"default": 2, "values": [1, 2], "tests": [_F + "test_keep_reset_in_the_float32_packed_kernel"]},
    "f32_waves": {"default": 0, "values": [0, 1, 4], "tests": [_P + "test_float32_packed_kernels", _F + "test_keep_reset_in_the_float32_packed_kernel"]},
    "tvs_tile": {"default": -1, "values": [-1, 0, 1], "tests": [_G + "test_weighted_tensor_vs_sequence_sum", _P + "test_tile_kernel_for_many_tensors",
                                                                _F + "test_threshold_tvs_tile_from_32_tensors"]},
    "wide": {"default": -1, "values": [-1, 0, 1], "tests": [_W + "test_wide_sequence_lattices_and_gradient", _G + "test_higher_order_reverse_pass_in_two_sweeps",
                                                            _F + "test_threshold_wide_kzx_beyond_8_columns", _F + "test_threshold_wide_kzz_beyond_12_columns",
                                                            _I + "test_every_compiled_sweep_instance_against_the_oracle"]},
    "wide_chunk_mb": {"default": 0, "values": [0, 1], "tests": [_W + "test_wide_tensor_vs_sequence_levels_and_gradient", _F + "test_wide_contract_forms_in_the_kzx_reverse_pass"]},
    "wide_contract": {"default": 1, "values": [0, 1, 2, 3], "tests": [_F + "test_wide_contract_forms_in_the_kzx_reverse_pass", _F + "test_wide_contract_forms_in_the_lattice_reverse_pass",
                                                                      _F + "test_wide_contract_strip_grid_stride"]},
    "wide_lat_waves": {"default": -1, "values": [-1, 0, 1], "tests": [_W + "test_wide_sequence_lattices_and_gradient", _F + "test_threshold_lat_waves_at_128_lattices"]},
    "wide_sym_fold": {"default": 1, "values": [0, 1], "tests": [_W + "test_wide_sequence_lattices_and_gradient"]},
    "ho_g32": {"default": -1, "values": [-1, 0, 1], "tests": [_F + "test_ho_g32", _I + "test_every_compiled_sweep_instance_against_the_oracle"]},
    "wide_few_cols": {"default": 0, "values": [0, 6], "tests": [_F + "test_threshold_few_rule"]},
    "tvs_grad_matern": {"default": 1, "values": [0, 1], "tests": [_F + "test_tvs_grad_matern"]},
    "wide_o1_sweeps": {"default": 1, "values": [0, 1, 2], "tests": [_W + "test_wide_sequence_lattices_and_gradient", _F + "test_threshold_wide_o1_sweeps_at_1024_lattices"]},
    "tvs_features": {"default": -1, "values": [-1, 0, 1], "tests": [_P + "test_tensor_vs_sequence_through_level_features"]},
    "tvs_tile_nw": {"default": 0, "values": [0, 1, 2, 4], "tests": [_P + "test_tile_kernel_for_many_tensors"]},
    "capture_routes": {"default": 0, "values": [0, 1], "tests": ["test_gpu_graph_routes.py::test_option_skips_only_the_wide_route_at_nine_columns",
                                                                 "test_gpu_graph_routes.py::test_fresh_context_warm_up_sizes_the_recorded_route",
                                                                 "test_gpu_graph_routes.py::test_option_is_restored_when_graphed_raises"]},
    "diag_own": {"default": 1, "values": [0, 1], "tests": [_P + "test_diagonal_pass_with_one_sequence_per_pair_group"]},
    "spectral_wave": {"default": 1, "values": [0, 1], "tests": [_P + "test_spectral_wavefront_kernels"]},
    "tens_tile": {"default": 1, "values": [0, 1], "tests": [_P + "test_tensor_gram_tiles"]},
    "lr_gemm": {"default": 1, "values": [0, 1], "tests": [_P + "test_low_rank_gram_products_in_lds_tiles"]},
    "lr_fused": {"default": 1, "values": [0, 1, 2], "tests": [_P + "test_low_rank_fused_feature_kernel", _L + "test_sequence_feature_routes", _F + "test_lr_fused_variants_and_pads"]},
    "lr_fused_variant": {"default": 0, "values": [0, 1, 2, 3], "tests": [_F + "test_lr_fused_variants_and_pads"]},
    "lr_fused_pad": {"default": 1, "values": [0, 1, 3], "tests": [_F + "test_lr_fused_variants_and_pads"]},
}
