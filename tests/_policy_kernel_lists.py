"""Every kernel csrc/policy.hip defines is in exactly one of these lists, with the test whose cases reach it.  Two route tests
import them, so the lists cannot drift apart: tests/test_policy_routes.py (the inference cases reach FORWARD) and
tests/test_learn_routes.py (the learn-pass cases reach BACKWARD and gru_step_fwd512_kernel).  An instance the library registers
outside the lists fails both, so a new kernel cannot arrive without a case."""

FORWARD = ["c1_act_kernel<1, 8>", "c1_act_kernel<2, 4>", "c1_act_kernel<4, 4>", "frag_pack_f32_kernel", "frag_pack_planes_kernel",
           "gi_act_kernel<7>", "gi_act_kernel<8>", "goal_to_i32_kernel", "goal_vec_fwd_kernel", "gru_gates_fwd_kernel",
           "gru_step_fwd_kernel", "heads_fwd_kernel<8>", "permute_row_kernel", "tail_fwd_kernel<false>", "tail_fwd_kernel<true>",
           "to_cmajor_kernel"]
FORWARD_ELSEWHERE = {   # forward kernels no inference case can reach -> what runs them (as EXEMPT does in tests/_conv_tile_ref.py)
    "gru_step_fwd512_kernel": "the learn pass at H = 512 (Step::fused16 needs !infer): tests/test_learn_routes.py pins the cases that "
                              "launch it, tests/test_gpu_learn_routes.py checks their numbers",
    "fuse_goal_kernel<false>": "fusion = 1, the zero-shot policy (no compressor, no combiner): tests/test_gpu_zeroshot.py",
    "fuse_goal_kernel<true>": "fusion = 1 with bf16 embeddings: tests/test_gpu_zeroshot.py",
}
BACKWARD = ["colsum4_kernel", "colsum_fold_kernel", "colsum_kernel", "frame_sum_kernel", "from_cmajor_kernel", "goal_vec_bwd_kernel",
            "group_sum_scatter_kernel", "gru_gates_bwd_kernel", "gru_step_bwd512_kernel", "gru_step_bwd_kernel", "seg_fold_kernel",
            "splitk_fold_kernel", "tail_bwd_fold_kernel", "tail_bwd_kernel<false>", "tail_bwd_kernel<true>", "tail_bwd_reduce_kernel",
            "tn_small_part_kernel", "transpose_f32_kernel"]
LEARN_FORWARD = ["gru_step_fwd512_kernel"]      # the entries of FORWARD_ELSEWHERE that the learn-pass table must reach
