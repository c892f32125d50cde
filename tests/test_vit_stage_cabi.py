"""The transformer stage entry points on a box without a GPU: exported, bound, and every refusal comes before any HIP call."""
import ctypes


NEW = ("ec_mha_bf16", "ec_layernorm_bf16", "ec_vit_assemble_bf16", "ec_row_stats_bf16", "ec_ln_fold_bf16", "ec_gemm_bf16_ln")
ARG, SHAPE, UNSUPPORTED = -1, -2, -6


def test_new_symbols_are_exported_and_bound():
    from embodied_clip_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name


def test_mha_refusals():
    from embodied_clip_amd import _lib
    lib = _lib.load()
    assert lib.ec_mha_bf16(None, 1, 1, 50, 128, 2, 0, None) == ARG
    assert lib.ec_mha_bf16(1, None, 1, 50, 128, 2, 0, None) == ARG
    assert lib.ec_mha_bf16(1, 1, 1, 50, 128, 4, 0, None) == SHAPE      # D / heads = 32
    assert lib.ec_mha_bf16(1, 1, 1, 50, 128, 1, 0, None) == SHAPE      # D / heads = 128
    assert lib.ec_mha_bf16(1, 1, 1, 50, 96, 1, 0, None) == SHAPE       # D / heads = 96
    assert lib.ec_mha_bf16(1, 1, 1, 50, 128, 0, 0, None) == SHAPE      # no heads
    assert lib.ec_mha_bf16(1, 1, 1, 0, 128, 2, 0, None) == SHAPE       # L < 1
    assert lib.ec_mha_bf16(1, 1, 1, 513, 128, 2, 0, None) == SHAPE     # L > 512
    assert lib.ec_mha_bf16(1, 1, 1, 513, 128, 2, 1, None) == SHAPE
    assert lib.ec_mha_bf16(1, 1, 0, 50, 128, 2, 0, None) == SHAPE      # no sequences


def test_layernorm_family_refusals():
    from embodied_clip_amd import _lib
    lib = _lib.load()
    assert lib.ec_layernorm_bf16(None, 1, 1, 1, 4, 128, None) == ARG
    assert lib.ec_layernorm_bf16(1, None, 1, 1, 4, 128, None) == ARG
    assert lib.ec_layernorm_bf16(1, 1, None, 1, 4, 128, None) == ARG
    assert lib.ec_layernorm_bf16(1, 1, 1, None, 4, 128, None) == ARG
    assert lib.ec_row_stats_bf16(None, 1, 4, 128, None) == ARG
    assert lib.ec_row_stats_bf16(1, None, 4, 128, None) == ARG
    for D in (0, 32, 96, 1000, 1088, 2048):                            # D % 64, D > 1024
        assert lib.ec_layernorm_bf16(1, 1, 1, 1, 4, D, None) == SHAPE, D
        assert lib.ec_row_stats_bf16(1, 1, 4, D, None) == SHAPE, D
        assert lib.ec_vit_assemble_bf16(1, 1, 1, 1, 1, 1, None, 2, 5, D, None) == SHAPE, D
    assert lib.ec_layernorm_bf16(1, 1, 1, 1, 0, 128, None) == SHAPE
    assert lib.ec_row_stats_bf16(1, 1, 0, 128, None) == SHAPE
    for missing in range(6):                                           # stats may be NULL, nothing else
        a = [1] * 6
        a[missing] = None
        assert lib.ec_vit_assemble_bf16(*a, None, 2, 5, 128, None) == ARG, missing
    assert lib.ec_vit_assemble_bf16(1, 1, 1, 1, 1, 1, None, 2, 1, 128, None) == SHAPE     # L < 2
    assert lib.ec_vit_assemble_bf16(1, 1, 1, 1, 1, 1, None, 0, 5, 128, None) == SHAPE     # no frames


def test_fold_and_folded_gemm_refusals():
    from embodied_clip_amd import _lib
    lib = _lib.load()
    for missing in range(7):
        a = [1] * 7
        a[missing] = None
        assert lib.ec_ln_fold_bf16(*a, 128, 128, None) == ARG, missing
    assert lib.ec_ln_fold_bf16(1, 1, 1, 1, 1, 1, 1, 0, 128, None) == SHAPE
    assert lib.ec_ln_fold_bf16(1, 1, 1, 1, 1, 1, 1, 128, 0, None) == SHAPE
    g = lambda A=1, Wt=1, bias=1, res=None, out=1, M=4, N=128, K=128, act=0, ln_s=None, ln_stats=None, ln_np=0, stats_out=None: \
        lib.ec_gemm_bf16_ln(A, Wt, bias, res, out, M, N, K, act, ln_s, ln_stats, ln_np, stats_out, None, None)
    assert g(A=None) == ARG and g(Wt=None) == ARG and g(out=None) == ARG
    assert g(M=0) == SHAPE and g(N=192) == SHAPE and g(K=96) == SHAPE and g(K=0) == SHAPE
    assert g(res=1, act=2) == UNSUPPORTED                              # QuickGELU after a residual
    assert g(ln_s=1, ln_stats=1, ln_np=1, res=1) == ARG                # a folded launch carries no residual
    assert g(ln_s=1, ln_stats=1, ln_np=1, bias=None) == ARG
    assert g(ln_s=1, ln_stats=None, ln_np=1) == ARG
    assert g(ln_s=1, ln_stats=1, ln_np=0) == ARG and g(ln_s=1, ln_stats=1, ln_np=9) == ARG
    assert g(N=1152, K=64, stats_out=1) == SHAPE                       # nine 128-wide records per row do not fit the consumer
