"""Float64 references, element-wise error bounds, fp32/bf16 emulations and named wrong versions of the transformer tower
stages (vit.hip: attention cores, LayerNorm, token assembly, row records, LayerNorm fold; conv_igemm.hip: the
LayerNorm-folded GEMM).  CPU only.  tests/test_vit_stage_ref.py checks here, without a GPU, that every bound bites on the
inputs below: the emulation of the kernel's arithmetic stays under it and each wrong version exceeds it at least 4 x
somewhere.  tests/test_gpu_vit_stages.py then holds the kernels to the same bounds on the same inputs.

Every reference takes the SAME bf16 (and fp32) inputs the kernel gets and works in float64.

Number formats: bf16 keeps 8 significant bits, so round-to-nearest has unit roundoff UB = 2^-8 (|bf16(x) - x| <= 2^-8 |x|);
fp32 has U = 2^-24.  A sum of fp32 terms added along a tree of depth t has error <= t U sum|terms| (first order).
"""
import math

import torch

import _bounds
from _bounds import F64, U, UB, bf16, randn as _randn  # noqa: F401

EPS = 1e-5
worst_ratio = lambda got, ref, bound: _bounds.worst_ratio(got, ref, bound)[0]      # noqa: E731  (these stages report no index)


# ------------------------------------------------------------------------------------------------------------------
# attention: out[b, i, h] = sum_j p_ij v_j,  p_i = softmax_j(q_i . k_j / 8  [j <= i when causal]),  head dim 64
#
# Rounding points of both cores (mha_kernel, mha_general_kernel) and of attnpool_core_kernel: scores, softmax and both sums in
# fp32; P rounded to bf16 before the PV product (attnpool: kept in fp32 -- fewer roundings, same bound); O rounded to bf16.
#   |sum_j (bf16(p_j) - p_j) v_j| <= 2^-8 sum_j p_j |v_j|                 (P rounding)
#   |bf16(o) - o|                 <= 2^-8 |o| <= 2^-8 (1 + 2^-8) sum_j p_j |v_j|      (O rounding)
# together 2^-7 sum_j p_j |v_j| to first order; the fp32 terms (64-term dot products, L-term sums, the fast exponential) are
# O(L 2^-24) relative, far inside the 5 % on top:   bound = 1.05 * 2^-7 * sum_j p_j |v_j|.
# ------------------------------------------------------------------------------------------------------------------
ATT_SCALE = 0.125


def _split_qkv(qkv, B, L, D, heads):
    """bf16 [B*L, 3D] -> q, k, v float64 [B, heads, L, 64]"""
    t = qkv.to(F64).reshape(B, L, 3, heads, 64).permute(2, 0, 3, 1, 4)
    return t[0], t[1], t[2]


def _merge_heads(o):
    B, H, L, _ = o.shape
    return o.permute(0, 2, 1, 3).reshape(B * L, H * 64)


def _mask(L, causal, shift=0):
    """allowed[i, j]; causal: j < i + 1 + shift (shift 0 is the true mask)"""
    if not causal:
        return torch.ones(L, L, dtype=torch.bool)
    i = torch.arange(L)
    return i[None, :] < (i[:, None] + 1 + shift)


def attention_probs(q, k, causal, scale=ATT_SCALE, shift=0):
    s = (q @ k.transpose(-1, -2)) * scale
    m = _mask(q.shape[-2], causal, shift)
    s = s.masked_fill(~m, float("-inf"))
    p = torch.softmax(s, dim=-1)
    return torch.nan_to_num(p, nan=0.0)        # (a wrong mask may leave a query without keys: it then gets zeros)


def attention_ref(qkv, B, L, D, heads, causal):
    """-> ref [B*L, D], bound [B*L, D], dominant p per query [B, heads, L]   (all float64)"""
    q, k, v = _split_qkv(qkv, B, L, D, heads)
    p = attention_probs(q, k, causal)
    ref = _merge_heads(p @ v)
    bound = 1.05 * 2.0 ** -7 * _merge_heads(p @ v.abs())
    return ref, bound, p.max(dim=-1).values


def attention_emulate(qkv, B, L, D, heads, causal):
    """The kernels' arithmetic: fp32 scores / softmax, P rounded to bf16, fp32 PV, O rounded to bf16."""
    q, k, v = (t.to(torch.float32) for t in _split_qkv(qkv, B, L, D, heads))
    s = (q @ k.transpose(-1, -2)) * ATT_SCALE
    s = s.masked_fill(~_mask(L, causal), float("-inf"))
    p = bf16(torch.softmax(s, dim=-1))
    return bf16(_merge_heads(p @ v))


def attention_wrong(qkv, B, L, D, heads, causal, kind):
    """Named wrong versions, in float64 (no rounding: the deviation is the mistake alone)."""
    q, k, v = _split_qkv(qkv, B, L, D, heads)
    if kind == "causal_nk_qi":
        return _merge_heads(attention_probs(q, k, True, shift=-1) @ v)
    if kind == "causal_nk_qi_plus_2":
        return _merge_heads(attention_probs(q, k, True, shift=1) @ v)
    if kind == "scale_rsqrt_D":
        return _merge_heads(attention_probs(q, k, causal, scale=D ** -0.5) @ v)
    if kind == "kv_swapped":
        return _merge_heads(attention_probs(q, v, causal) @ k)
    raise KeyError(kind)


def attention_drop_key_ratios(qkv, B, L, D, heads, causal, ref, bound):
    """For EVERY key j (of every sequence and head): the worst |wrong - ref| / bound over the channels of the query that key
    dominates, the wrong version being the softmax without key j.  Without key j query i gets (o_i - p_ij v_j) / (1 - p_ij);
    only the query with the largest p_ij is evaluated (one place is enough to expose the drop).  -> [B, heads, L]"""
    q, k, v = _split_qkv(qkv, B, L, D, heads)
    p = attention_probs(q, k, causal)
    o = p @ v
    pj, qi = p.max(dim=-2)                                   # per key j: its largest weight and the query that gives it
    oi = torch.gather(o, 2, qi[..., None].expand(-1, -1, -1, 64))
    wrong = (oi - pj[..., None] * v) / (1 - pj[..., None]).clamp_min(1e-300)
    only = pj >= 1 - 1e-12                                   # the query's only key: nothing is left, the row comes out as zeros
    wrong = torch.where(only[..., None], torch.zeros_like(wrong), wrong)
    bnd = bound.reshape(B, L, heads, 64).permute(0, 2, 1, 3)
    bi = torch.gather(bnd, 2, qi[..., None].expand(-1, -1, -1, 64))
    return ((wrong - oi).abs() / bi).max(dim=-1).values


def attention_inputs(family, B, L, D, heads, seed=0):
    """bf16 qkv [B*L, 3D] with different data in every sequence and head.
      'reverse'  (non-causal)  q_i = c k_{L-1-i}: every key is the dominant key of one query, and the reversal exposes
                               transposed indexing
      'diag'     (causal)      q_i = c k_i: the diagonal dominates (a mask one short, nk = qi, loses it)
      'next'     (causal)      q_i = c k_{i+1}: the query asks for the first forbidden key (any leak forward shows)
    c starts at 1 and is raised until the dominant p of every query is >= 0.5 ('reverse', 'diag'), respectively until the
    forbidden key WOULD take >= 0.5 of every query that has one ('next')."""
    k = _randn(1000 * L + seed, B, heads, L, 64)
    v = _randn(1000 * L + seed + 1, B, heads, L, 64)
    c = 1.0
    while True:
        if family == "reverse":
            q = c * k.flip(2)
        elif family == "diag":
            q = c * k
        elif family == "next":
            q = c * torch.cat([k[:, :, 1:], k[:, :, :1]], dim=2)
        else:
            raise KeyError(family)
        qb, kb = bf16(q).to(F64), bf16(k).to(F64)
        if family == "next":
            if L == 1:
                break
            p = attention_probs(qb, kb, True, shift=1)
            dom = torch.diagonal(p, offset=1, dim1=-2, dim2=-1).min()
        else:
            dom = attention_probs(qb, kb, family != "reverse").max(dim=-1).values.min()
        if float(dom) >= 0.5:
            break
        c *= 1.25
    t = torch.stack([q, k, v], 0)                            # [3, B, heads, L, 64]
    return t.permute(1, 3, 0, 2, 4).reshape(B * L, 3 * D).to(torch.bfloat16).contiguous()


# (L, causal, family) of every ec_mha_bf16 case at B = 3, heads = 2, D = 128: the MFMA core (non-causal, L <= 64), the general
# core non-causal at the 64-key chunk edges and the limit, and causal with both inputs
MHA_CASES = ([(L, False, "reverse") for L in (1, 2, 31, 32, 33, 50, 63, 64, 65, 128, 129, 197, 257, 512)]
             + [(L, True, f) for L in (1, 2, 20, 64, 65, 77, 129, 512) for f in ("diag", "next")])
MHA_WIDE_CASE = dict(B=2, L=50, D=768, heads=12, causal=False, family="reverse")


# ------------------------------------------------------------------------------------------------------------------
# LayerNorm stages.  y = (v - mean) rstd gamma + beta over the D values v of a row, rstd = 1 / sqrt(var + eps), var over D.
#
# Kernel (layernorm_kernel, one wave per row): a lane adds its D / 64 values in sequence (the D % 256 path: in groups of four,
# pairwise), then a 6-step butterfly: summation depth t <= D / 64 + 6 for both paths.  First order, U = 2^-24:
#   mean:   |dmean| <= (t + 1) U mean|v|                        (t for the sum, 1 for the division)
#   var:    sum (v - mean^)^2 = sum d^2 + D dmean^2, each d and d^2 rounded, the sum at depth t, one division and the + eps:
#           relative (t + 5) U  +  dmean^2 / (var + eps)
#   rstd:   half of that, + 2 U for the rsqrt
#   d rstd gamma + beta: |gamma| rstd |dmean| from the mean, 3 U |d rstd gamma| for the three products, U |y| for the add
#   fp = |gamma| rstd (|dmean| + |d| (rel_rstd + 4 U)) + U (|y| + |beta|)
# and one rounding of the result to bf16:   bound = 2^-8 (|y| + fp) + fp.
# Token assembly (layernorm_kernel<1>) first forms v = base + pos in fp32: |dv| <= U |v|, which moves y by at most
# |gamma| rstd (|dv| + mean|dv|) -- added to fp through `v_err`.
# ------------------------------------------------------------------------------------------------------------------
def ln_depth(D):
    return D // 64 + 6


def layernorm_ref(v, gamma, beta, v_err=None):
    """v float64 [rows, D] (the exact row values), gamma / beta fp32 [D] -> ref, bound (float64)"""
    D = v.shape[-1]
    g, b = gamma.to(F64), beta.to(F64)
    t = ln_depth(D)
    mean = v.mean(-1, keepdim=True)
    d = v - mean
    var = (d * d).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + EPS)
    y = d * rstd * g + b
    dmean = (t + 1) * U * v.abs().mean(-1, keepdim=True)
    rel_rstd = 0.5 * ((t + 5) * U + dmean ** 2 / (var + EPS)) + 2 * U
    fp = g.abs() * rstd * (dmean + d.abs() * (rel_rstd + 4 * U)) + U * (y.abs() + b.abs())
    if v_err is not None:
        fp = fp + g.abs() * rstd * (v_err + v_err.mean(-1, keepdim=True))
    return y, UB * (y.abs() + fp) + fp


def layernorm_emulate(v32, gamma, beta):
    """fp32 statistics and arithmetic on fp32 row values, result rounded to bf16 (returned as fp32)."""
    D = v32.shape[-1]
    mean = v32.sum(-1, keepdim=True) / D
    d = v32 - mean
    rstd = torch.rsqrt((d * d).sum(-1, keepdim=True) / D + torch.tensor(EPS, dtype=torch.float32))
    return bf16(d * rstd * gamma + beta)


def layernorm_wrong(v, gamma, beta, kind, vector_path=False):
    """Named wrong versions in float64.  `lane_missing`: lane 5 of the wave adds nothing to the two sums (its channels are
    d % 64 == 5, or the D / 64 consecutive channels from 5 D / 64 on the D % 256 path)."""
    D = v.shape[-1]
    g, b = gamma.to(F64), beta.to(F64)
    keep = torch.ones(D, dtype=F64)
    nvar, eps = D, EPS
    if kind == "var_over_D_minus_1":
        nvar = D - 1
    elif kind == "no_eps":
        eps = 0.0
    elif kind == "lane_missing":
        per = D // 64
        if vector_path:
            keep[5 * per:6 * per] = 0
        else:
            keep[5::64] = 0
    elif kind == "gamma_beta_shifted":
        g, b = torch.roll(g, -1), torch.roll(b, -1)
    else:
        raise KeyError(kind)
    mean = (v * keep).sum(-1, keepdim=True) / D
    d = v - mean
    var = (d * d * keep).sum(-1, keepdim=True) / nvar
    return d / torch.sqrt(var + eps) * g + b


LN_WRONG = ("var_over_D_minus_1", "no_eps", "lane_missing", "gamma_beta_shifted")
LN_FAMILIES = ("plain", "mean_dominated", "near_constant", "gamma_spread")
LN_DIMS = (64, 192, 256, 768, 1024)
LN_ROWS = (1, 3, 4, 5, 197)
# the family whose rows expose each wrong version (the others need not: eps is invisible at unit variance and hides the divisor
# of a variance of 1e-6; a lost lane moves a zero-mean row by little).  D - 1 for D changes gamma z by 1 / (2 D), under 2^-8 of it:
# it shows where beta cancels most of gamma z, which the random beta of the plain rows does somewhere in every case below.
LN_CAUGHT_BY = {"var_over_D_minus_1": "plain", "no_eps": "near_constant", "lane_missing": "mean_dominated",
                "gamma_beta_shifted": "gamma_spread"}


def layernorm_inputs(family, rows, D, seed=0):
    """-> x bf16 [rows, D], gamma fp32 [D], beta fp32 [D]
      plain            unit normal rows, gamma ~ 1, beta ~ 0.5 N
      mean_dominated   |mean| ~ 6 sigma (alternating sign by row)
      near_constant    2^-7 + 1e-3 N: var ~ 1e-6 against eps 1e-5, and beta = 0 so that the output is the normalised row alone
      gamma_spread     gamma = 2^(-2 .. 2), beta ~ N"""
    s = 7919 * D + 31 * rows + seed
    x = _randn(s, rows, D)
    gamma = 1.0 + 0.1 * _randn(s + 1, D)
    beta = 0.5 * _randn(s + 2, D)
    if family == "mean_dominated":
        sign = torch.where(torch.arange(rows) % 2 == 0, 1.0, -1.0)[:, None]
        x = x + 6.0 * sign
    elif family == "near_constant":
        x = 2.0 ** -7 + 1e-3 * x
        beta = torch.zeros(D)
    elif family == "gamma_spread":
        gamma = torch.exp2(4 * torch.rand(D, generator=torch.Generator().manual_seed(s + 3)) - 2)
        beta = _randn(s + 2, D)
    elif family != "plain":
        raise KeyError(family)
    return x.to(torch.bfloat16).contiguous(), gamma.contiguous(), beta.contiguous()


# token assembly + ln_pre: (B, L, D)
ASSEMBLE_SHAPES = ((1, 2, 64), (3, 5, 192), (2, 50, 768))


def assemble_inputs(B, L, D, seed=0):
    s = 104729 * D + 17 * L + seed
    pemb = _randn(s, B * (L - 1), D).to(torch.bfloat16).contiguous()
    cls = _randn(s + 1, D) * 0.5
    pos = _randn(s + 2, L, D) * 0.3 + 0.7                   # (a common offset: the rows are not zero-mean)
    gamma = 1.0 + 0.2 * _randn(s + 3, D)
    beta = 0.3 * _randn(s + 4, D)
    return pemb, cls.contiguous(), pos.contiguous(), gamma.contiguous(), beta.contiguous()


def assemble_rows(pemb, cls, pos, B, L, D):
    """-> the exact row values v float64 [B*L, D], the fp32 rows the kernel forms, and U |v| (the rounding of that sum)"""
    base = torch.cat([cls[None, None, :].expand(B, 1, D), pemb.to(torch.float32).reshape(B, L - 1, D)], dim=1)
    v64 = (base.to(F64) + pos.to(F64)[None]).reshape(B * L, D)
    v32 = (base + pos[None]).reshape(B * L, D)
    return v64, v32, U * v64.abs()


# ------------------------------------------------------------------------------------------------------------------
# LayerNorm records {sum, M2, count, 0} of a bf16 row (or of BN columns of it): count and the fourth field are exact; sum and M2
# are compared with float64 of the bf16 values that were STORED, within the fp32 summation bound at depth t:
#   |dsum| <= t U sum|y|;   the kernel's mean m^ = sum^ / n is off by dm <= (t + 1) U mean|y|, so its
#   M2^ = sum (y - m^)^2 = M2 + n dm^2, plus (t + 4) U M2 for rounding d, d^2 and the sum.
# ------------------------------------------------------------------------------------------------------------------
def record_ref(y, t):
    """y float64 [rows, n] -> (sum, M2, n), (bound_sum, bound_M2)"""
    n = y.shape[-1]
    s = y.sum(-1)
    m2 = ((y - s[:, None] / n) ** 2).sum(-1)
    a = y.abs().sum(-1)
    dm = (t + 1) * U * a / n
    return (s, m2, float(n)), (t * U * a + 1e-300, (t + 4) * U * m2 + n * dm ** 2 + 1e-300)


def record_emulate(y32):
    n = y32.shape[-1]
    s = y32.sum(-1)
    m2 = ((y32 - s[:, None] / n) ** 2).sum(-1)
    return s, m2


def tile_records_ref(y, width, t):
    """Records of every `width`-column tile of y float64 [rows, D]: refs and bounds as [rows, D / width] tensors."""
    rows, D = y.shape
    (s, m2, n), (bs, bm) = record_ref(y.reshape(rows * (D // width), width), t)
    sh = (rows, D // width)
    return (s.reshape(sh), m2.reshape(sh), n), (bs.reshape(sh), bm.reshape(sh))


# depth of the record sums: row_stats / layernorm kernels as ln_depth(D); the GEMM epilogue adds a lane's 8 values (the sum
# pairwise, M2 as a chain of 8 fused multiply-adds: the deeper one counts) and then a butterfly over width / 8 lanes
def epilogue_record_depth(width):
    return 8 + int(math.log2(width // 8))


# ------------------------------------------------------------------------------------------------------------------
# ec_ln_fold_bf16:  Wg = bf16(fp32(W) gamma) bit for bit (one fp32 product, one rounding);  s[n] = sum_k Wg[n, k] over the ROUNDED
# values;  c[n] = sum_k beta[k] W[n, k] + b[n].  A thread adds ceil(K / 256) terms in sequence (c: fused multiply-adds), then 6
# butterfly steps and 2 more across the four waves: depth t = ceil(K / 256) + 8, and one more rounding for + b.
# ------------------------------------------------------------------------------------------------------------------
FOLD_SHAPES = ((64, 64), (192, 192), (768, 768), (256, 1024))     # (N, K): the assemble widths, and K = 1024


def fold_inputs(N, K, seed=0):
    s = 613 * K + N + seed
    W = (_randn(s, N, K) * K ** -0.5).to(torch.bfloat16).contiguous()
    gamma = torch.exp2(4 * torch.rand(K, generator=torch.Generator().manual_seed(s + 1)) - 2).contiguous()
    beta = _randn(s + 2, K).contiguous()
    b = (0.1 * _randn(s + 3, N)).contiguous()
    return W, gamma, beta, b


def fold_ref(W, gamma, beta, b):
    """-> Wg (bf16 tensor, exact), (s, bound_s), (c, bound_c)"""
    N, K = W.shape
    t = -(-K // 256) + 8
    Wg = (W.to(torch.float32) * gamma[None, :]).to(torch.bfloat16)
    s = Wg.to(F64).sum(-1)
    bs = t * U * Wg.to(F64).abs().sum(-1) + 1e-300
    prod = beta.to(F64)[None, :] * W.to(F64)
    c = prod.sum(-1) + b.to(F64)
    bc = (t + 1) * U * (prod.abs().sum(-1) + b.to(F64).abs()) + 1e-300
    return Wg, (s, bs), (c, bc)


def fold_emulate(W, gamma, beta, b):
    Wg = (W.to(torch.float32) * gamma[None, :]).to(torch.bfloat16)
    return Wg, Wg.to(torch.float32).sum(-1), (beta[None, :] * W.to(torch.float32)).sum(-1) + b


# ------------------------------------------------------------------------------------------------------------------
# ec_gemm_bf16_ln (consumer):  out = act(rstd (x Wg^T - mean s) + c), with the stored bf16 x, the Wg / s / c the fold wrote and
# the exact mean / rstd (eps 1e-5) of x.  The kernel accumulates x Wg^T in fp32 over K terms, combines the row's records in
# fp32 (Chan), forms rstd acc - mean rstd s + c with fused multiply-adds and rounds once to bf16:
#   pre-activation error  e <= K U rstd (sum_k |x_k Wg_nk| + |mean s_n|) + U |c_n|
#   bound = 2^-8 |ref| + e            (EC_ACT_NONE)
#   bound = 2^-8 |ref| + 1.1 e        (QuickGELU z sigmoid(1.702 z): |derivative| <= 1.1)
# ------------------------------------------------------------------------------------------------------------------
ACT_NONE, ACT_QUICKGELU = 0, 2


def quickgelu(z):
    return z * torch.sigmoid(1.702 * z)


def gemm_ln_ref(x, Wg, s, c, act):
    """x bf16 [M, K], Wg bf16 [N, K], s / c fp32 [N] -> ref, bound (float64 [M, N])"""
    K = x.shape[-1]
    xd, wd, sd, cd = x.to(F64), Wg.to(F64), s.to(F64), c.to(F64)
    mean = xd.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((xd - mean) ** 2).mean(-1, keepdim=True) + EPS)
    z = rstd * (xd @ wd.T - mean * sd[None, :]) + cd[None, :]
    e = K * U * rstd * (xd.abs() @ wd.abs().T + (mean * sd[None, :]).abs()) + U * cd.abs()[None, :]
    if act == ACT_QUICKGELU:
        ref = quickgelu(z)
        return ref, UB * ref.abs() + 1.1 * e
    return z, UB * z.abs() + e


def combine_records(sums, m2s, counts, wrong=None):
    """The consumer's combination of a row's np records -> mean, rstd.  sums / m2s [M, np], counts [np] or scalar; any float dtype.
    wrong: None | ('ignore', q) -- record q left out | 'equal_weight' -- the between-tile term not weighted by the count"""
    cnt = torch.as_tensor(counts, dtype=sums.dtype).expand(sums.shape[-1]).clone()
    if isinstance(wrong, tuple):
        keep = [i for i in range(sums.shape[-1]) if i != wrong[1]]
        sums, m2s, cnt = sums[:, keep], m2s[:, keep], cnt[keep]
    n = cnt.sum()
    mean = sums.sum(-1, keepdim=True) / n
    d = sums / cnt - mean
    w = torch.ones_like(cnt) if wrong == "equal_weight" else cnt
    m2 = (m2s + w * d * d).sum(-1, keepdim=True)
    return mean, torch.rsqrt(m2 / n + EPS)


def gemm_ln_emulate(x, Wg, s, c, act, width, wrong=None):
    """Producer records of `width`-column tiles and the consumer's arithmetic, all in fp32, result rounded to bf16.
    wrong: as combine_records, or 'no_mean_s' -- the - mean s term left out."""
    f = torch.float32
    xf, wf = x.to(f), Wg.to(f)
    M, K = xf.shape
    tiles = xf.reshape(M, K // width, width)
    sums = tiles.sum(-1)
    m2s = ((tiles - sums[..., None] / width) ** 2).sum(-1)
    mean, rstd = combine_records(sums, m2s, float(width), None if wrong == "no_mean_s" else wrong)
    acc = xf @ wf.T
    ms = 0.0 if wrong == "no_mean_s" else mean * s.to(f)[None, :]
    z = rstd * (acc - ms) + c.to(f)[None, :]
    return bf16(quickgelu(z) if act == ACT_QUICKGELU else z)


def residual_stream(kind, M, D, seed=0):
    """bf16 [M, D] residual rows.  'plain': unit normal.  'mean_dominated': + 6 overall, +-2 alternating by 128-column block and +-1.5 by 256-column block, so
    that |mean| ~ 6 sigma within a block AND the blocks' means differ (what the records' combination has to get right)."""
    x = _randn(15485863 + 977 * D + M + seed, M, D)
    if kind == "mean_dominated":
        col = torch.arange(D)
        blk = torch.where((col // 128) % 2 == 0, 2.0, -2.0) + torch.where((col // 256) % 2 == 0, 1.5, -1.5)
        if D // 128 > 1:
            blk[-128:] *= 1.5                                # (unequal blocks: leaving any ONE record out moves the mean)
        x = x + 6.0 + blk[None, :]
    elif kind != "plain":
        raise KeyError(kind)
    return x.to(torch.bfloat16).contiguous()


def consumer_weights(N, K, seed=0):
    """The folded GEMM's operands through the fold's own reference arithmetic (CPU stand-in for ec_ln_fold_bf16's output)."""
    W, gamma, beta, b = fold_inputs(N, K, seed + 5)
    Wg, s, c = fold_emulate(W, gamma, beta, b)
    return (W, gamma, beta, b), (Wg, s, c)


GEMM_M = (1, 191, 192, 193, 256, 257, 449)
GEMM_N = (128, 384, 512)
GEMM_SETTINGS = {"default": {}, "bm192_off": {"EC_VIT_BM192": "0"}, "wide": {"EC_VIT_WIDE": "2"}}


def gemm_widths(setting):
    return (256, 768, 1024) if setting == "wide" else (128, 384, 768, 1024)


def gemm_expected_np(setting, D):
    return D // 256 if (setting == "wide" and D % 256 == 0) else D // 128


def gemm_cases(setting):
    """Every M with every D once; N, the activation and the residual family cycle so that each value of each meets every D and
    every M somewhere.  -> list of dicts"""
    out = []
    for di, D in enumerate(gemm_widths(setting)):
        for mi, M in enumerate(GEMM_M):
            i = di * len(GEMM_M) + mi
            out.append(dict(M=M, D=D, N=GEMM_N[(mi + di) % 3], act=(ACT_NONE, ACT_QUICKGELU)[(mi // 3 + di + mi) % 2],
                            stream=("plain", "mean_dominated")[i % 2]))
    return out
