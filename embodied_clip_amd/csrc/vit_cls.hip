// The CLS-only form of a ResidualAttentionBlock ([U] openai/CLIP clip/model.py), for the class embedding that [U] allenact
// ClipViTEmbedder returns with class_emb_only (`x[:, 0, :]` after resblocks[:-1]): of the last block that runs only row 0 of every
// frame is read, so K / V are needed for all L tokens but q, the attention row, out_proj, ln_2, c_fc and c_proj for B rows instead
// of B * L.  vit.hip's run_cls_block issues the block; this file holds the three kernels that work on the B class rows:
//   rows_gemm_bf16_kernel   out[M, N] = act(A W^T + bias (+ res)) for 1..128 rows per row block
//   cls_rows_ln_kernel      LayerNorm of B rows read at a pitch (the class rows of x [B*L, D] in place)
//   cls_attn_kernel         one query per (frame, head) against kv [B*L, 2D]
// and their stage entry points (ec_gemm_rows_bf16, ec_vit_cls_rows_ln, ec_vit_cls_attn).
#include "common.h"

namespace {

__device__ __forceinline__ float wave_sum_f(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max_f(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// Few-row GEMM.  The tile kernels of conv_igemm.hip put a [128, 768] output on six workgroups; here a workgroup owns a strip of
// 32 columns of ALL rows of its row block (up to RT * 32 = 128 rows; blockIdx.y walks row blocks of 128) and its four waves split
// K: wave w walks the 64-wide K-tiles w, w + 4, ... -- N / 32 workgroups (24 for N = 768, 96 for N = 3072), each streaming its 32
// rows of W exactly once.  Operand fragments come straight from global memory in MFMA layout (lane = row fr / column fr, 8
// consecutive k: one 16-byte load), the loads of two K-tiles are issued before the first MFMA of the pair.  One fp32 accumulator per
// element per wave; the four partials are added through LDS in wave order (no float atomics), then bias, residual, activation and
// ONE rounding.  Rows past M are computed on a clamped row and never stored.
//   store: 0 bf16 | 1 rounded to bf16, written as fp32 (the embedding at the API edge) | 2 fp32
template <int RT>
__global__ __launch_bounds__(256) void rows_gemm_bf16_kernel(const uint16_t* __restrict__ A, long lda, const uint16_t* __restrict__ W,
                                                            const float* __restrict__ bias, const uint16_t* __restrict__ res, long ldr,
                                                            void* __restrict__ out, long ldo, int M, int N, int K, int act, int store) {
    __shared__ float part[4][RT * 32][32];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 31, fh = lane >> 5;
    const int n0 = blockIdx.x * 32, m0 = blockIdx.y * 128;
    const int nkt = K / 64;
    f32x16_t acc[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[rt][r] = 0.f;
    if (wave < nkt) {
        const uint16_t* wp = W + (long)(n0 + fr) * K + fh * 8;
        const uint16_t* ap[RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) ap[rt] = A + (long)min(m0 + rt * 32 + fr, M - 1) * lda + fh * 8;
        uint4 wf[4], af[RT][4];
        auto load = [&](uint4 (&w_)[4], uint4 (&a_)[RT][4], int kt) {
            const int k0 = kt * 64;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) w_[ks] = *reinterpret_cast<const uint4*>(wp + k0 + ks * 16);
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) a_[rt][ks] = *reinterpret_cast<const uint4*>(ap[rt] + k0 + ks * 16);
        };
        auto mma = [&](const uint4 (&w_)[4], const uint4 (&a_)[RT][4]) {
#pragma unroll
            for (int ks = 0; ks < 4; ++ks)
#pragma unroll
                for (int rt = 0; rt < RT; ++rt)
                    acc[rt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, a_[rt][ks]),
                                                                     __builtin_bit_cast(bf16x8_t, w_[ks]), acc[rt], 0, 0, 0);
        };
        // Two K-tiles per pass, all 2 (4 + 4 RT) loads in flight before the first MFMA: the scheduling barrier keeps them together
        // (left alone the compiler interleaves load / s_waitcnt / MFMA one fragment at a time -- ten serial memory round trips per
        // K-tile).  The loop body has no branch: a second tile past the end re-reads the first and multiplies a zeroed W fragment
        // (acc + 0 is exact).
        uint4 wn[4], an[RT][4];
        for (int kt = wave; kt < nkt; kt += 8) {
            const bool two = kt + 4 < nkt;
            load(wf, af, kt);
            load(wn, an, two ? kt + 4 : kt);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) wn[ks] = make_uint4(two ? wn[ks].x : 0u, two ? wn[ks].y : 0u, two ? wn[ks].z : 0u, two ? wn[ks].w : 0u);
            mma(wf, af);
            mma(wn, an);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    // C/D layout: column = lane & 31, rows (r & 3) + 8 (r >> 2) + 4 fh
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int r = 0; r < 16; ++r) part[wave][rt * 32 + (r & 3) + 8 * (r >> 2) + 4 * fh][fr] = acc[rt][r];
    __syncthreads();
    for (int e = tid; e < RT * 32 * 32; e += 256) {
        const int row = e >> 5, col = e & 31;
        const long gm = (long)m0 + row;
        if (gm >= M) break;                                     // (rows ascend with e)
        float v = ((part[0][row][col] + part[1][row][col]) + part[2][row][col]) + part[3][row][col];
        const int n = n0 + col;
        if (bias) v += bias[n];
        if (res) v += ec_bf2f(res[gm * ldr + n]);
        if (act == EC_ACT_QUICKGELU) v *= __builtin_amdgcn_rcpf(1.f + __expf(-1.702f * v));   // as conv_igemm.hip's epilogue
        if (store == 2) {
            reinterpret_cast<float*>(out)[gm * ldo + n] = v;
        } else {
            const uint16_t o = (uint16_t)(ec_pack2(v, 0.f) & 0xffffu);
            if (store == 1) reinterpret_cast<float*>(out)[gm * ldo + n] = ec_bf2f(o);
            else reinterpret_cast<uint16_t*>(out)[gm * ldo + n] = o;
        }
    }
}

// LayerNorm over D (fp32 statistics) of `rows` bf16 rows read at a pitch, one wave per row: layernorm_kernel<0>'s arithmetic
// (vit.hip; lane owns channels lane, lane + 64, ...).  pitch = L * D reads the class rows of x [B*L, D] in place.
__global__ __launch_bounds__(256) void cls_rows_ln_kernel(const uint16_t* __restrict__ x, long pitch, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, uint16_t* __restrict__ out, int rows, int D,
                                                         float eps) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    constexpr int MAXV = 16;               // D <= 1024
    const int per = D / 64;
    const uint16_t* p = x + (long)row * pitch;
    float v[MAXV];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < MAXV; ++i)
        if (i < per) { v[i] = ec_bf2f(p[i * 64 + lane]); s += v[i]; }
    const float mean = wave_sum_f(s) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < MAXV; ++i)
        if (i < per) { const float d0 = v[i] - mean; q += d0 * d0; }
    const float rstd = rsqrtf(wave_sum_f(q) / (float)D + eps);
    uint16_t* o = out + (long)row * D;
#pragma unroll
    for (int i = 0; i < MAXV; ++i)
        if (i < per) {
            const int d = i * 64 + lane;
            o[d] = (uint16_t)(ec_pack2((v[i] - mean) * rstd * gamma[d] + beta[d], 0.f) & 0xffffu);
        }
}

// One query per (frame, head), head dim 64, up to EC_CLS_ATTN_MAX_TOKENS keys: one wave per (frame, head).  Rounding points of
// attnpool_core_kernel (vit.hip): q scaled in fp32 before the dot product, scores / softmax / both sums in fp32, P kept in fp32, O
// rounded to bf16.  Unlike that kernel a LANE owns keys lane, lane + 64, ...: it reads its key rows as 16-byte pieces and forms the
// 64-term dot product alone (no butterfly per key); then lane d adds up output channel d over the keys.
__global__ __launch_bounds__(64) void cls_attn_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ kv,
                                                     uint16_t* __restrict__ out, int L, int C, int heads, float scale) {
    __shared__ float sq[64];
    __shared__ float sp[EC_CLS_ATTN_MAX_TOKENS];
    const int lane = threadIdx.x;
    const int b = blockIdx.x / heads, h = blockIdx.x % heads;
    sq[lane] = ec_bf2f(q[(long)b * C + h * 64 + lane]) * scale;
    const uint16_t* kb = kv + (long)b * L * 2 * C + h * 64;
    __syncthreads();
    constexpr int MAXJ = EC_CLS_ATTN_MAX_TOKENS / 64;
    float sc[MAXJ];
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < MAXJ; ++i) {
        const int j = i * 64 + lane;
        sc[i] = -INFINITY;
        if (i * 64 < L && j < L) {
            const uint4* kr = reinterpret_cast<const uint4*>(kb + (long)j * 2 * C);
            float a = 0.f;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const uint4 u = kr[c];
                const float* qq = sq + c * 8;
                a += qq[0] * ec_lo(u.x); a += qq[1] * ec_hi(u.x); a += qq[2] * ec_lo(u.y); a += qq[3] * ec_hi(u.y);
                a += qq[4] * ec_lo(u.z); a += qq[5] * ec_hi(u.z); a += qq[6] * ec_lo(u.w); a += qq[7] * ec_hi(u.w);
            }
            sc[i] = a;
            mx = fmaxf(mx, a);
        }
    }
    mx = wave_max_f(mx);
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < MAXJ; ++i) {
        const int j = i * 64 + lane;
        if (i * 64 < L) {
            const float e = (j < L) ? __expf(sc[i] - mx) : 0.f;
            sc[i] = e;
            sum += e;
        }
    }
    const float inv = 1.f / wave_sum_f(sum);
#pragma unroll
    for (int i = 0; i < MAXJ; ++i) {
        const int j = i * 64 + lane;
        if (i * 64 < L && j < L) sp[j] = sc[i] * inv;
    }
    __syncthreads();
    float o = 0.f;
    const uint16_t* vb = kb + C + lane;
#pragma unroll 4
    for (int t = 0; t < L; ++t) o += sp[t] * ec_bf2f(vb[(long)t * 2 * C]);
    out[(long)b * C + h * 64 + lane] = (uint16_t)(ec_pack2(o, 0.f) & 0xffffu);
}

inline bool aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
inline bool ln_width_ok(int D) { return D >= 64 && D % 64 == 0 && D <= 1024; }

}  // namespace

extern "C" int ec_gemm_rows_bf16(const void* A, long lda, const void* W, const float* bias, const void* res, long ldr, void* out,
                                 long ldo, int M, int N, int K, int act, int store, ec_stream_t stream) {
    if (!A || !W || !out) return EC_ERR_ARG;
    if (store < 0 || store > 2 || (act != EC_ACT_NONE && act != EC_ACT_QUICKGELU)) return EC_ERR_ARG;
    if (!aligned(A, 16) || !aligned(W, 16) || !aligned(bias, 4) || !aligned(res, 2) || !aligned(out, store ? 4 : 2)) return EC_ERR_ARG;
    if (M < 1 || M > (1 << 20) || N < 32 || N % 32 != 0 || K < 64 || K % 64 != 0 || N > (1 << 20) || K > (1 << 20)) return EC_ERR_SHAPE;
    if (lda < K || lda % 8 != 0 || ldo < N || (res && ldr < N)) return EC_ERR_SHAPE;
    if (lda > (1L << 40) / M || ldo > (1L << 40) / M || (res && ldr > (1L << 40) / M)) return EC_ERR_SHAPE;
    const int rt = (min(M, 128) + 31) / 32;
    const dim3 grid((unsigned)(N / 32), (unsigned)((M + 127) / 128)), block(256);
    hipStream_t s = (hipStream_t)stream;
#define EC_ROWS_GO(RT_)                                                                                                            \
    hipLaunchKernelGGL(rows_gemm_bf16_kernel<RT_>, grid, block, 0, s, (const uint16_t*)A, lda, (const uint16_t*)W, bias,            \
                       (const uint16_t*)res, ldr, out, ldo, M, N, K, act, store)
    switch (rt) {
        case 1: EC_ROWS_GO(1); break;
        case 2: EC_ROWS_GO(2); break;
        case 3: EC_ROWS_GO(3); break;
        default: EC_ROWS_GO(4); break;
    }
#undef EC_ROWS_GO
    EC_CHECK_LAUNCH();
    return EC_OK;
}

extern "C" int ec_vit_cls_rows_ln(const void* x, long pitch, const float* gamma, const float* beta, void* out, int rows, int D,
                                  ec_stream_t stream) {
    if (!x || !gamma || !beta || !out) return EC_ERR_ARG;
    if (!aligned(x, 2) || !aligned(out, 2) || !aligned(gamma, 4) || !aligned(beta, 4)) return EC_ERR_ARG;
    if (rows < 1 || rows > (1 << 24) || !ln_width_ok(D) || pitch < D || pitch > (1L << 40) / rows) return EC_ERR_SHAPE;
    hipLaunchKernelGGL(cls_rows_ln_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)x,
                       pitch, gamma, beta, (uint16_t*)out, rows, D, 1e-5f);
    EC_CHECK_LAUNCH();
    return EC_OK;
}

extern "C" int ec_vit_cls_attn(const void* q, const void* kv, void* out, int B, int L, int D, int heads, ec_stream_t stream) {
    if (!q || !kv || !out) return EC_ERR_ARG;
    if (!aligned(q, 2) || !aligned(kv, 16) || !aligned(out, 2)) return EC_ERR_ARG;
    if (B <= 0 || heads <= 0 || D <= 0 || D % heads != 0 || D / heads != 64 || L < 1 || L > EC_CLS_ATTN_MAX_TOKENS) return EC_ERR_SHAPE;
    if ((long)B * heads >= (1L << 31) || (long)B * L * 2 * D * 2 >= (1L << 31)) return EC_ERR_SHAPE;
    hipLaunchKernelGGL(cls_attn_kernel, dim3((unsigned)(B * heads)), dim3(64), 0, (hipStream_t)stream, (const uint16_t*)q,
                       (const uint16_t*)kv, (uint16_t*)out, L, D, heads, 0.125f);
    EC_CHECK_LAUNCH();
    return EC_OK;
}
