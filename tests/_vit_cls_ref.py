"""Float64 references, element-wise error bounds, fp32/bf16 emulations and named wrong versions of the CLS-only last block's
kernels (vit_cls.hip: rows_gemm_bf16_kernel, cls_rows_ln_kernel, cls_attn_kernel).  CPU only.  tests/test_vit_cls_ref.py checks
here, without a GPU, that every bound bites: the emulation of the kernel's arithmetic stays under it and each wrong version exceeds
it at least 4 x somewhere.  tests/test_gpu_vit_cls.py then holds the kernels to the same bounds on the same inputs.

Every reference takes the SAME bf16 (and fp32) operands the kernel gets and works in float64.  UB = 2^-8 (bf16), U = 2^-24 (fp32).

ec_gemm_rows_bf16:  z = sum_k a_k w_k + bias (+ res), out = act(z).  tests/_conv_tile_ref.py's bound with one more term for the
K-split: a wave keeps ONE fp32 accumulator per element over its K-tiles (c(K) = 64 ceil(K / 64) additions charged for the whole
walk, whatever the split), the W = 4 waves' partials are added in wave order (W additions charged), then bias and residual:
    fp = (c(K) + W + 2) U (sum_k |a_k w_k| + |bias| + |res|)
    QuickGELU: fp -> 1.1 fp + g,  g = U |ref| ((1 - s) (3.404 |z| + 2) + 4)      (that file's derivation: v_exp, v_rcp)
    bound = 1.05 (R (|ref| + fp) + fp)
R is the ONE rounding of the result: UB when it is rounded to bf16 -- store 0 (bf16) and store 1 (the bf16 value written as fp32:
the embedding at the API edge) -- and U for the fp32 store (store 2).

ec_vit_cls_attn: _vit_stage_ref.attention_ref's bound on the query's row (fewer roundings than the cores: P stays fp32).
ec_vit_cls_rows_ln: _vit_stage_ref.layernorm_ref's bound (the strided path's summation depth D / 64 + 6).
"""
import torch

from _conv_tile_ref import quickgelu
from _vit_stage_ref import (F64, U, UB, _randn, attention_inputs, attention_probs, attention_ref, bf16, layernorm_emulate,  # noqa: F401
                            layernorm_inputs, layernorm_ref, worst_ratio, _split_qkv)

ACT_NONE, ACT_QUICKGELU = 0, 2
STORE_BF16, STORE_BF16_AS_F32, STORE_F32 = 0, 1, 2
NWAVES = 4                 # per-wave partials added


# ------------------------------------------------------------------------------------------------------------------
# ec_gemm_rows_bf16
# ------------------------------------------------------------------------------------------------------------------
GEMM_M = (1, 3, 31, 33, 128, 130)          # one row, ragged MFMA tile, exactly full, second row block
GEMM_NK = ((32, 64), (96, 192), (128, 3072))
GEMM_PITCH = (1, 3)                         # A pitch = K, 3 K
# every epilogue variant: (act, residual with its own pitch, store, bias)
GEMM_VARIANTS = (
    dict(act=ACT_NONE, res=False, store=STORE_BF16, bias=True),
    dict(act=ACT_QUICKGELU, res=False, store=STORE_BF16, bias=True),
    dict(act=ACT_NONE, res=True, store=STORE_BF16, bias=True),
    dict(act=ACT_NONE, res=True, store=STORE_BF16_AS_F32, bias=True),
    dict(act=ACT_NONE, res=False, store=STORE_F32, bias=True),
    dict(act=ACT_NONE, res=False, store=STORE_BF16, bias=False),
    dict(act=ACT_QUICKGELU, res=False, store=STORE_F32, bias=True),
)


def gemm_cases():
    """Every M with every (N, K) and both pitches; the variant cycles (7 variants against 36 shapes: each meets every M, every
    (N, K) and both pitches somewhere)."""
    out = []
    for mi, M in enumerate(GEMM_M):
        for ni, (N, K) in enumerate(GEMM_NK):
            for pi, pm in enumerate(GEMM_PITCH):
                i = (mi * len(GEMM_NK) + ni) * len(GEMM_PITCH) + pi
                out.append(dict(M=M, N=N, K=K, lda=pm * K, **GEMM_VARIANTS[i % len(GEMM_VARIANTS)]))
    return out


def gemm_id(c):
    return "M%d-N%d-K%d-lda%d-act%d-res%d-store%d-bias%d" % (c["M"], c["N"], c["K"], c["lda"], c["act"], c["res"], c["store"], c["bias"])


def gemm_inputs(c, seed=0):
    """-> dict: A bf16 [M, lda] (the columns past K hold other data: a wrong pitch shows), W bf16 [N, K], bias fp32 [N] | None,
    res bf16 [M, ldr] | None with ldr = N + 16"""
    M, N, K, lda = c["M"], c["N"], c["K"], c["lda"]
    s = 7 * M + 131 * N + 17 * K + lda + seed
    A = _randn(s, M, lda).to(torch.bfloat16).contiguous()
    W = (_randn(s + 1, N, K) * K ** -0.5).to(torch.bfloat16).contiguous()
    bias = (0.3 * _randn(s + 2, N)).contiguous() if c["bias"] else None
    res = _randn(s + 3, M, N + 16).to(torch.bfloat16).contiguous() if c["res"] else None
    return dict(A=A, W=W, bias=bias, res=res)


def c_of_k(K):
    return 64 * -(-K // 64)


def _gelu_g(ref, pre):
    sg = torch.sigmoid(1.702 * pre)
    return U * ref.abs() * ((1 - sg) * (3.404 * pre.abs() + 2) + 4)


def gemm_ref(c, op):
    """-> ref, bound: float64 [M, N]"""
    N, K = c["N"], c["K"]
    a, w = op["A"][:, :K].to(F64), op["W"].to(F64)
    b = op["bias"].to(F64)[None, :] if op["bias"] is not None else torch.zeros(1, N, dtype=F64)
    r = op["res"][:, :N].to(F64) if op["res"] is not None else torch.zeros(1, N, dtype=F64)
    pre = a @ w.T + b + r
    fp = (c_of_k(K) + NWAVES + 2) * U * (a.abs() @ w.abs().T + b.abs() + r.abs())
    ref = pre
    if c["act"] == ACT_QUICKGELU:
        ref = quickgelu(pre)
        fp = 1.1 * fp + _gelu_g(ref, pre)
    rnd = U if c["store"] == STORE_F32 else UB
    return ref, 1.05 * (rnd * (ref.abs() + fp) + fp)


def wave_of_ktile(K):
    """wave that walks each 64-wide K-tile: w, w + 4, ..."""
    return torch.arange(K // 64) % NWAVES


def gemm_emulate(c, op, wrong=None):
    """The kernel's arithmetic in fp32: per-wave partials over the K-tiles w, w + 4, ..., added in wave order, + bias, + residual,
    activation, one rounding (none for the fp32 store).  wrong: None | 'drop_wave_partial' (the last wave that has a K-tile adds
    nothing) | 'pitch_K' (row m read at m K instead of m lda) | 'bias_by_row' | 'no_bias' | 'res_normalised' (the residual row
    LayerNorm-ed, gamma 1 beta 0, instead of raw)."""
    f = torch.float32
    M, N, K = c["M"], c["N"], c["K"]
    if wrong == "pitch_K":
        a = op["A"].reshape(-1)[:M * K].reshape(M, K).to(f)
    else:
        a = op["A"][:, :K].to(f)
    w = op["W"].to(f)
    wv = wave_of_ktile(K).repeat_interleave(64)
    last = int(wv.max())
    z = torch.zeros(M, N, dtype=f)
    for i in range(NWAVES):
        if wrong == "drop_wave_partial" and i == last:
            continue
        sel = wv == i
        if bool(sel.any()):
            z = z + a[:, sel] @ w[:, sel].T
    if op["bias"] is not None and wrong != "no_bias":
        b = op["bias"]
        z = z + (b[torch.arange(M) % N][:, None] if wrong == "bias_by_row" else b[None, :])
    if op["res"] is not None:
        r = op["res"][:, :N].to(f)
        if wrong == "res_normalised":
            r = bf16((r - r.mean(-1, keepdim=True)) * torch.rsqrt(r.var(-1, unbiased=False, keepdim=True) + 1e-5))
        z = z + r
    if c["act"] == ACT_QUICKGELU:
        z = quickgelu(z)
    return z if c["store"] == STORE_F32 else bf16(z)


GEMM_WRONG = ("drop_wave_partial", "pitch_K", "bias_by_row", "no_bias", "res_normalised")


def gemm_wrong_applies(c, kind):
    """the cases on which a wrong version differs from the right one at all"""
    if kind == "pitch_K":
        return c["lda"] != c["K"] and c["M"] > 1
    if kind in ("bias_by_row", "no_bias"):
        return c["bias"] and (kind == "no_bias" or c["M"] > 1)
    if kind == "res_normalised":
        return c["res"]
    return True


# ------------------------------------------------------------------------------------------------------------------
# ec_vit_cls_attn: one query per (frame, head).  The inputs are _vit_stage_ref's 'reverse' family (q_i = c k_{L-1-i}, the dominant
# key of query i is L - 1 - i).  The kernel sees ONE query per frame: row 0 -- and, so that EVERY key dominates somewhere, each
# other row i in turn plays the class row (L calls on the same kv; the reference's row i is the expected output).
# ------------------------------------------------------------------------------------------------------------------
ATTN_CASES = ((3, 1, 2), (3, 37, 2), (2, 50, 3), (2, 82, 2), (1, 257, 2))     # (B, L, heads)


def attn_inputs(B, L, heads):
    """-> qkv bf16 [B*L, 3D]; q_rows bf16 [L, B, D] (row i of every frame as the query), kv bf16 [B*L, 2D]"""
    D = heads * 64
    qkv = attention_inputs("reverse", B, L, D, heads)
    q_rows = qkv[:, :D].reshape(B, L, D).permute(1, 0, 2).contiguous()
    kv = qkv[:, D:].contiguous()
    return qkv, q_rows, kv


def attn_ref(qkv, B, L, heads):
    """-> ref, bound float64 [L, B, D] (index 0: the class row), dominant p per (row, frame, head)"""
    D = heads * 64
    ref, bound, dom = attention_ref(qkv, B, L, D, heads, False)
    sh = lambda t: t.reshape(B, L, D).permute(1, 0, 2)      # noqa: E731
    return sh(ref), sh(bound), dom.permute(2, 0, 1)


def attn_emulate(qkv, B, L, heads, wrong=None):
    """cls_attn_kernel's arithmetic for the class row (row 0) of every frame: q scaled in fp32, fp32 scores / softmax / PV, O rounded to
    bf16 -> [B, D].  wrong (float64, no rounding): 'query_row_1' | 'frame_b_minus_1' (the class row of the frame before) |
    'kv_swapped'"""
    D = heads * 64
    dt = torch.float32 if wrong is None else F64
    q, k, v = (t.to(dt) for t in _split_qkv(qkv, B, L, D, heads))      # [B, heads, L, 64]
    row = 1 if wrong == "query_row_1" else 0
    q0 = q[:, :, row:row + 1] * 0.125
    if wrong == "frame_b_minus_1":
        q0 = torch.roll(q0, 1, dims=0)
    if wrong == "kv_swapped":
        k, v = v, k
    p = torch.softmax(q0 @ k.transpose(-1, -2), dim=-1)
    o = (p @ v).reshape(B, D)
    return bf16(o) if wrong is None else o


ATTN_WRONG = ("query_row_1", "frame_b_minus_1", "kv_swapped")


def attn_wrong_applies(B, L, kind):
    """(with one key the softmax is 1 whatever the query: a wrong query shows from two keys on)"""
    return {"query_row_1": L > 1, "frame_b_minus_1": B > 1 and L > 1, "kv_swapped": True}[kind]


# ------------------------------------------------------------------------------------------------------------------
# ec_vit_cls_rows_ln: `rows` rows read at a pitch out of a wider buffer
# ------------------------------------------------------------------------------------------------------------------
LN_DIMS = (64, 128, 192, 768)
LN_PITCH = (1, 5)
LN_ROWS = (1, 3, 5)
LN_FAMILIES = ("plain", "mean_dominated", "near_constant", "gamma_spread")


def ln_inputs(family, rows, D, pitch_mul, seed=0):
    """-> buf bf16 [rows, pitch_mul D] whose leading D columns are the rows (the rest: rows of the same family), gamma, beta"""
    x, gamma, beta = layernorm_inputs(family, rows * pitch_mul, D, seed)
    return x.reshape(rows, pitch_mul * D).contiguous(), gamma, beta


def ln_wrong_pitch(buf, rows, D, gamma, beta):
    """rows read at pitch D instead of the buffer's: row r starts at r D"""
    v = buf.reshape(-1)[:rows * D].reshape(rows, D).to(F64)
    return layernorm_ref(v, gamma, beta)[0]
