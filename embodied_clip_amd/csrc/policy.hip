// GRU actor-critic policy: forward and hand-written backward.
//
// Replaces ``ActorCriticModel.forward`` as ``ResnetTensorObjectNavActorCritic``
// and the autograd graph torch builds behind ``total_loss.backward()``
// ([U] allenai/allenact ~v0.5.0: projects/objectnav_baselines/models/
// object_nav_models.py ResnetTensorGoalEncoder; allenact/embodiedai/models/
// basic_models.py RNNStateEncoder, LinearActorHead, LinearCriticHead;
// launched by the reference at readme_files/baselines_robothor_objectnav.md:48-51;
// SURVEY.md §8a a11-a14).
//
// Data layout (all fp32 except the frozen features):
//   feat  [T*N, S, C]      NHWC rows of the rollout feature buffer (bf16 or fp32)
//   params one flat fp32 buffer in AllenAct parameter order (ec_policy_param_offset)
//   grads  one flat fp32 buffer, same offsets (one all-reduce bucket)
// The goal embedding is folded into a [num_goals, 128] row-group bias table
// E1 = embed_class @ W3[:, 32:]^T + b3, so the 64-channel concat is never built.
#include <stdlib.h>

#include <mutex>
#include <new>
#include <unordered_map>

#include "common.h"

// C++-linkage internal of the library (ec_gemm_bf16a_xp and every extern "C" entry this file calls are declared in common.h)
int ec_dw_tn_xp(const void* dYplanes, const void* X, float* part, float* dW, long M, int NX, int planes, ec_stream_t stream);   // dw_tn.hip

namespace {

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + __expf(-x)); }

__global__ void goal_to_i32_kernel(const long long* g, int* o, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) o[i] = (int)g[i];
}

// x[b, c*S + p] = x4[(b*S + p)*Cc + c]   (channel-major flatten of the combiner output)
// (ldx / xcol: row pitch and first column of this stream's block inside x -- the dual RGB + depth encoder concatenates
//  its two streams' channel-major blocks, [U] ResnetDualTensorGoalEncoder: torch.cat([rgb_x, depth_x], dim=1) then flatten)
__global__ void to_cmajor_kernel(const float* __restrict__ x4, float* __restrict__ x, int S, int Cc, long total, int ldx,
                                 int xcol) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int per = S * Cc;
    const long b = i / per;
    const int r = (int)(i - b * per);
    const int c = r / S, p = r - c * S;
    x[b * ldx + xcol + r] = x4[(b * S + p) * Cc + c];
}
__global__ void from_cmajor_kernel(const float* __restrict__ dx, float* __restrict__ dx4, int S, int Cc, long total, int ldx,
                                   int xcol) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int per = S * Cc;
    const long b = i / per;
    const int r = (int)(i - b * per);
    const int p = r / Cc, c = r - p * Cc;
    dx4[i] = dx[b * ldx + xcol + c * S + p];
}

// EC_WIH_PERM (learn pass): instead of re-ordering the [T*N x 1568] activations between the combiner's pixel-major rows and
// nn.Flatten's channel-major order (to_cmajor / from_cmajor: 2 x 206 MB of strided traffic per optimiser step, 0.5 ms),
// the 9.6-MB weight_ih is re-ordered once per step: mode 0  out[r, p*Cc + c] = in[r, c*S + p];  mode 1 (its gradient,
// back to the parameter's order)  out[r, c*S + p] += in[r, p*Cc + c].  One row per workgroup, staged through LDS.
// ld: the row stride of the PARAMETER and of its gradient (mode 0's `in`, mode 1's `out`) -- flat, or flat + E on a handle with a
// previous-action embedding, whose columns flat.. are not touched; the re-ordered copy is dense.
__global__ __launch_bounds__(256) void permute_row_kernel(const float* __restrict__ in, float* __restrict__ out, int S, int Cc,
                                                         int mode, int ld) {
    extern __shared__ float prow[];
    const int flat = S * Cc;
    const long base = (long)blockIdx.x * flat, pbase = (long)blockIdx.x * ld;
    for (int i = threadIdx.x; i < flat; i += 256) prow[i] = in[(mode == 0 ? pbase : base) + i];
    __syncthreads();
    if (mode == 0) {
        for (int i = threadIdx.x; i < flat; i += 256) out[base + i] = prow[(i % Cc) * S + i / Cc];
    } else {
        for (int i = threadIdx.x; i < flat; i += 256) out[pbase + i] += prow[(i % S) * Cc + i / S];
    }
}
// torch.nn.GRU cell with the RNNStateEncoder episode mask:
//   hp = m*h_prev;  r = s(gi_r + m*gh_r + b_hr);  z = s(gi_z + m*gh_z + b_hz)
//   hn = m*gh_n + b_hn;  n = tanh(gi_n + r*hn);  h = (1-z)*n + z*hp
// (gh = h_prev W_hh^T without bias; the mask commutes with the row-wise GEMM).
__global__ void gru_gates_fwd_kernel(const float* __restrict__ gi, const float* __restrict__ gh,
                                     const float* __restrict__ bhh, const float* __restrict__ hprev,
                                     const float* __restrict__ mask, float* __restrict__ hout,
                                     float* __restrict__ gates, float* __restrict__ hn_s, float* __restrict__ hp_s,
                                     int N, int H) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N * H) return;
    const int n = i / H, j = i - n * H;
    const float m = mask[n];
    const float* gir = gi + (long)n * 3 * H;
    const float* ghr = gh + (long)n * 3 * H;
    const float hp = m * hprev[i];
    const float r = sigmoidf_(gir[j] + m * ghr[j] + bhh[j]);
    const float z = sigmoidf_(gir[H + j] + m * ghr[H + j] + bhh[H + j]);
    const float hn = m * ghr[2 * H + j] + bhh[2 * H + j];
    const float nn = tanhf(gir[2 * H + j] + r * hn);
    hout[i] = (1.f - z) * nn + z * hp;
    if (gates) {
        float* g = gates + (long)n * 3 * H;
        g[j] = r; g[H + j] = z; g[2 * H + j] = nn;
        hn_s[i] = hn;
        hp_s[i] = hp;
    }
}

// Fused GRU forward step (round 2): recurrent projection + gate math in ONE launch per time step, replacing the
// [N x 3H x H] GEMM launch + gru_gates_fwd_kernel pair (17 + 7 us per step at N = 128, 128 steps per direction).
// Workgroup (blockIdx.x, blockIdx.y) owns hidden units j0..j0+7 (24 gate columns of W_hh) of actors n0..n0+31:
//   * hp = m * h_prev tile [32 x H] and the 24 W_hh rows [24 x H] are staged in LDS (row pitch H + 4 floats: the
//     16-lane groups of a ds_read_b128 hit 16 different 16-byte slots);
//   * wave w contracts its quarter of K with the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32 == an fmaf chain, so the
//     result stays within fp32 rounding of the reference GRU): lane (i = l & 31, hh = l >> 5) feeds k = kb + 4 hh + q
//     to the q-th MFMA of a k-block of 8, one ds_read_b128 per operand per 4 MFMAs;
//   * the four partial 32 x 32 tiles are summed through LDS in a fixed order (actor-local, batch-invariant: act steps
//     stay bit-reproducible whatever the slicing), then thread (a, u) applies the gate math of unit j0 + u of actor a.
__global__ __launch_bounds__(256) void gru_step_fwd_kernel(const float* __restrict__ gi, const float* __restrict__ Whh,
                                                          const float* __restrict__ bhh, const float* __restrict__ hprev,
                                                          const float* __restrict__ mask, float* __restrict__ hout,
                                                          float* __restrict__ gates, float* __restrict__ hn_s,
                                                          float* __restrict__ hp_s, int N, int H, int gi_parts,
                                                          long gi_pstride) {
    extern __shared__ __attribute__((aligned(16))) float gsm[];
    // K is walked in chunks of KC = 256 (whole K when H is not a multiple of 256): the two tiles then take 66.5 KB, so two
    // workgroups fit a CU and the recurrences of the two actor slices (two HIP streams) overlap instead of queueing
    const int KC = ((H & 255) == 0) ? 256 : H;
    const int P = KC + 4;
    float* sA = gsm;
    float* sB = gsm + 32 * P;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j0 = blockIdx.x * 8, n0 = blockIdx.y * 32;
    const int i = lane & 31, hh = lane >> 5;
    f32x16_t acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    if (KC == 256) {                                                    // W rows 24..31 of the B tile: zeros, once
        for (int idx = tid; idx < 8 * 64; idx += 256) {
            const int r = 24 + (idx >> 6), c4 = idx & 63;
            *reinterpret_cast<float4*>(sB + r * P + c4 * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    // the episode mask is applied to the contraction result (m (h W^T) == (m h) W^T exactly for m in {0, 1})
    for (int k0 = 0; k0 < H; k0 += KC) {
        if (k0) __syncthreads();                                        // every wave is done reading the previous chunk
        if (KC == 256) {
            // LDS-DMA staging: one 1-KiB piece per tile row (256 floats); 56 rows round-robin over the 4 waves
            typedef __attribute__((address_space(3))) void lds_v;
            typedef const __attribute__((address_space(1))) void gbl_v;
            const int uwave = __builtin_amdgcn_readfirstlane(wave);
            for (int r = uwave; r < 56; r += 4) {
                const float* src;
                float* dst;
                if (r < 32) {
                    const int n = min(n0 + r, N - 1);                   // rows past N are never read back
                    src = hprev + (long)n * H + k0 + lane * 4;
                    dst = sA + r * P;
                } else {
                    const int c = r - 32;
                    src = Whh + ((long)(c >> 3) * H + j0 + (c & 7)) * H + k0 + lane * 4;
                    dst = sB + c * P;
                }
                __builtin_amdgcn_global_load_lds((gbl_v*)src, (lds_v*)dst, 16, 0, 0);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        } else {
            const int q4 = H >> 2;
            for (int idx = tid; idx < 32 * q4; idx += 256) {
                const int r = idx / q4, c4 = idx - r * q4;
                float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
                const int n = n0 + r;
                if (n < N) a = *reinterpret_cast<const float4*>(hprev + (long)n * H + c4 * 4);
                if (r < 24) b = *reinterpret_cast<const float4*>(Whh + ((long)(r >> 3) * H + j0 + (r & 7)) * H + c4 * 4);
                *reinterpret_cast<float4*>(sA + r * P + c4 * 4) = a;
                *reinterpret_cast<float4*>(sB + r * P + c4 * 4) = b;
            }
        }
        __syncthreads();
        const int kq = KC >> 2;
        const float* pa = sA + i * P + wave * kq + 4 * hh;
        const float* pb = sB + i * P + wave * kq + 4 * hh;
        for (int kb = 0; kb < kq; kb += 8) {
            const float4 a = *reinterpret_cast<const float4*>(pa + kb);
            const float4 b = *reinterpret_cast<const float4*>(pb + kb);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
        }
    }
    __syncthreads();                       // the operand tiles are dead: LDS becomes the 4 partial [32 x 32] tiles
    float* part = gsm;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * hh;     // actor (C/D layout of the 32x32 MFMA), column = lane & 31
        part[(wave * 32 + row) * 32 + i] = acc[r];
    }
    __syncthreads();
    const int a_ = tid >> 3, u = tid & 7;
    const int n = n0 + a_, j = j0 + u;
    if (n >= N) return;
    float gh[3];
#pragma unroll
    for (int g = 0; g < 3; ++g) {
        const int c = g * 8 + u;
        gh[g] = ((part[(0 * 32 + a_) * 32 + c] + part[(1 * 32 + a_) * 32 + c]) + part[(2 * 32 + a_) * 32 + c]) +
                part[(3 * 32 + a_) * 32 + c];
    }
    const float* gir = gi + (long)n * 3 * H;
    float gi_r = gir[j], gi_z = gir[H + j], gi_n = gir[2 * H + j];
    for (int p2 = 1; p2 < gi_parts; ++p2) {        // act step: the input projection arrives as split-K parts (fixed order)
        const float* gp2 = gir + p2 * gi_pstride;
        gi_r += gp2[j]; gi_z += gp2[H + j]; gi_n += gp2[2 * H + j];
    }
    const float m = mask[n];
    const float hp = m * hprev[(long)n * H + j];
    const float r = sigmoidf_(gi_r + m * gh[0] + bhh[j]);
    const float z = sigmoidf_(gi_z + m * gh[1] + bhh[H + j]);
    const float hn = m * gh[2] + bhh[2 * H + j];
    const float nn = tanhf(gi_n + r * hn);
    const long o = (long)n * H + j;
    hout[o] = (1.f - z) * nn + z * hp;
    if (gates) {
        float* gp = gates + (long)n * 3 * H;
        gp[j] = r; gp[H + j] = z; gp[2 * H + j] = nn;
        hn_s[o] = hn;
        hp_s[o] = hp;
    }
}

// reverse step: dh = dhs + dh_carry;  outputs dgi (wrt gi), dghb (wrt m*gh + b_hh),
// dh_carry <- m * dh * z   (the GEMM m*(dghb W_hh) is accumulated on top afterwards)
__global__ void gru_gates_bwd_kernel(const float* __restrict__ dhs, float* __restrict__ dh_carry,
                                     const float* __restrict__ gates, const float* __restrict__ hn_s,
                                     const float* __restrict__ hp_s, const float* __restrict__ mask,
                                     float* __restrict__ dgi, float* __restrict__ dghb, int N, int H) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N * H) return;
    const int n = i / H, j = i - n * H;
    const float* g = gates + (long)n * 3 * H;
    const float r = g[j], z = g[H + j], nn = g[2 * H + j];
    const float hn = hn_s[i], hp = hp_s[i];
    const float dh = dhs[i] + dh_carry[i];
    const float dn_pre = dh * (1.f - z) * (1.f - nn * nn);
    const float dz_pre = dh * (hp - nn) * z * (1.f - z);
    const float dr_pre = dn_pre * hn * r * (1.f - r);
    float* a = dgi + (long)n * 3 * H;
    float* b = dghb + (long)n * 3 * H;
    a[j] = dr_pre; a[H + j] = dz_pre; a[2 * H + j] = dn_pre;
    b[j] = dr_pre; b[H + j] = dz_pre; b[2 * H + j] = dn_pre * r;
    dh_carry[i] = mask[n] * dh * z;
}

// out[c][r] = in[r][c] (fp32, R x C -> C x R): W_hh^T for the fused backward step, once per ec_policy_backward
__global__ __launch_bounds__(256) void transpose_f32_kernel(const float* __restrict__ in, float* __restrict__ out, int R, int C) {
    __shared__ float t[32][33];
    const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = r0 + ty + 8 * i, c = c0 + tx;
        t[ty + 8 * i][tx] = (r < R && c < C) ? in[(long)r * C + c] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = c0 + ty + 8 * i, r = r0 + tx;
        if (r < R && c < C) out[(long)c * R + r] = t[tx][ty + 8 * i];
    }
}

// Fused GRU BACKWARD step (round 3): the recurrent back-projection of step t+1 and the gate math of step t in ONE launch,
// replacing the [N x H x 3H] split-K GEMM (fp32 atomics: 17 us) + gru_gates_bwd_kernel (5 us) pair of every step:
//   dh[n, j] = dhs_t[n, j] + carry[n, j] + m_{t+1}[n] * sum_k dghb_{t+1}[n, k] W_hh[k, j]
// (carry = the element-wise part m_{t+1} dh_{t+1} z_{t+1} the previous launch left), then the cell's gate gradients.
// Workgroup (blockIdx.x, blockIdx.y) owns hidden units j0..j0+31 of actors n0..n0+31; K = 3H is walked in 256-wide chunks
// through LDS-DMA exactly as gru_step_fwd_kernel does (A tile = dghb rows, B tile = rows j0.. of W_hh^T), the four waves
// contract a quarter of each chunk on the exact-fp32 MFMA and their partial tiles are summed through LDS in a fixed
// order: no atomics, so the policy gradients are now bit-reproducible run to run.
__global__ __launch_bounds__(256) void gru_step_bwd_kernel(const float* __restrict__ dghb_next, const float* __restrict__ WhhT,
                                                          const float* __restrict__ mask_next, const float* __restrict__ dhs,
                                                          float* __restrict__ carry, const float* __restrict__ gates,
                                                          const float* __restrict__ hn_s, const float* __restrict__ hp_s,
                                                          const float* __restrict__ mask, float* __restrict__ dgi,
                                                          float* __restrict__ dghb, int N, int H) {
    extern __shared__ __attribute__((aligned(16))) float gsm[];
    constexpr int KC = 256, P = KC + 4;
    const int K = 3 * H;
    float* sA = gsm;
    float* sB = gsm + 32 * P;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j0 = blockIdx.x * 32, n0 = blockIdx.y * 32;
    const int i = lane & 31, hh = lane >> 5;
    f32x16_t acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int k0 = 0; k0 < K; k0 += KC) {
        if (k0) __syncthreads();
        typedef __attribute__((address_space(3))) void lds_v;
        typedef const __attribute__((address_space(1))) void gbl_v;
        const int uwave = __builtin_amdgcn_readfirstlane(wave);
        for (int r = uwave; r < 64; r += 4) {                      // one 1-KiB LDS-DMA piece per tile row
            const float* src;
            float* dst;
            if (r < 32) {
                const int n = min(n0 + r, N - 1);                  // rows past N are never read back
                src = dghb_next + (long)n * K + k0 + lane * 4;
                dst = sA + r * P;
            } else {
                src = WhhT + (long)(j0 + r - 32) * K + k0 + lane * 4;
                dst = sB + (r - 32) * P;
            }
            __builtin_amdgcn_global_load_lds((gbl_v*)src, (lds_v*)dst, 16, 0, 0);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        const float* pa = sA + i * P + wave * (KC >> 2) + 4 * hh;
        const float* pb = sB + i * P + wave * (KC >> 2) + 4 * hh;
#pragma unroll
        for (int kb = 0; kb < (KC >> 2); kb += 8) {
            const float4 a = *reinterpret_cast<const float4*>(pa + kb);
            const float4 b = *reinterpret_cast<const float4*>(pb + kb);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
        }
    }
    __syncthreads();                       // the operand tiles are dead: LDS becomes the 4 partial [32 x 32] tiles
    float* part = gsm;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * hh;     // actor (C/D layout of the 32x32 MFMA), column = lane & 31
        part[(wave * 32 + row) * 32 + i] = acc[r];
    }
    __syncthreads();
    const int a_ = tid >> 3, u0 = tid & 7;
    const int n = n0 + a_;
    if (n >= N) return;
    const float mn = mask_next[n], m = mask[n];
    const float* g = gates + (long)n * 3 * H;
    float* ga = dgi + (long)n * 3 * H;
    float* gb = dghb + (long)n * 3 * H;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int c = u0 + 8 * q, j = j0 + c;
        const float proj = ((part[(0 * 32 + a_) * 32 + c] + part[(1 * 32 + a_) * 32 + c]) + part[(2 * 32 + a_) * 32 + c]) +
                           part[(3 * 32 + a_) * 32 + c];
        const long o = (long)n * H + j;
        const float r = g[j], z = g[H + j], nn = g[2 * H + j];
        const float hn = hn_s[o], hp = hp_s[o];
        const float dh = dhs[o] + (carry[o] + mn * proj);
        const float dn_pre = dh * (1.f - z) * (1.f - nn * nn);
        const float dz_pre = dh * (hp - nn) * z * (1.f - z);
        const float dr_pre = dn_pre * hn * r * (1.f - r);
        ga[j] = dr_pre; ga[H + j] = dz_pre; ga[2 * H + j] = dn_pre;
        gb[j] = dr_pre; gb[H + j] = dz_pre; gb[2 * H + j] = dn_pre * r;
        carry[o] = m * dh * z;
    }
}

// ---- 16 x 16-tile GRU step kernels for the UPDATE's recurrences (H == 512, EC_GRU_FUSED >= 2, round 3) ----
// The 32 x 32-tile kernels above put 256 (forward) / 64 (backward) workgroups on the chip and wait for every K chunk with
// nothing else in flight: 15 us a step, 2 x 1024 dependent steps per update.  These two use the 16x16x4 fp32 MFMA so that
// 16 actors x 16 hidden units make a workgroup (256 of them for 128 actors, forward AND backward), and give every wave a
// PRIVATE quarter of K: a wave's LDS-DMA pieces land in its own LDS slice (no workgroup barrier between load and MFMA; the
// wave waits with counted s_waitcnt vmcnt while later pieces are still in flight).  Rows are stored unpadded, 512 B per
// row and wave, with the 16-B units XOR-swizzled by (row & 15) on the GLOBAL side of the DMA (LDS side is contiguous by
// construction), which makes the ds_read_b128 operand reads conflict-free.  The epilogue's operands are fetched before the
// first piece is issued.  Same fp32 arithmetic as above, K summed in a different (fixed) order.
typedef __attribute__((address_space(3))) void gru_lds_v;
typedef const __attribute__((address_space(1))) void gru_gbl_v;

__device__ __forceinline__ f32x4_t mfma16f(float a, float b, f32x4_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
// Loads the compiler must neither sink to their first use (the epilogue operands: fetched under the pieces) nor fence with a
// vmcnt(0) of its own (it puts one in front of every ds_read that follows an LDS-DMA): issued as asm, waited for by the
// kernels' counted s_waitcnt, and tied to their consumers through gru_tie().
__device__ __forceinline__ float gru_gload(const float* p) {
    float v;
    asm volatile("global_load_dword %0, %1, off" : "=&v"(v) : "v"(p) : "memory");
    return v;
}
__device__ __forceinline__ f32x4_t gru_lread(unsigned lds_addr) {
    f32x4_t v;
    asm volatile("ds_read_b128 %0, %1" : "=&v"(v) : "v"(lds_addr) : "memory");
    return v;
}
__device__ __forceinline__ unsigned gru_lds_addr(const float* p) {
    return (unsigned)(unsigned long)(__attribute__((address_space(3))) const float*)p;
}
template <int CNT> __device__ __forceinline__ void gru_lwait(f32x4_t& a, f32x4_t& b) {   // ds_reads up to here have returned
    asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(a), "+v"(b) : "n"(CNT));
}

__global__ __launch_bounds__(256) void gru_step_fwd512_kernel(const float* __restrict__ gi, const float* __restrict__ Whh,
                                                             const float* __restrict__ bhh, const float* __restrict__ hprev,
                                                             const float* __restrict__ mask, float* __restrict__ hout,
                                                             float* __restrict__ gates, float* __restrict__ hn_s,
                                                             float* __restrict__ hp_s, int N) {
    constexpr int H = 512, KW = 128;                       // KW: the k range of one wave (512 B of every row)
    extern __shared__ __attribute__((aligned(16))) float gsm[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j0 = blockIdx.x * 16, n0 = blockIdx.y * 16;
    float* wl = gsm + wave * (64 * KW);                    // 64 rows (16 actors + 3 x 16 W rows) x 128 floats = 32 KB / wave
    float* part = gsm + 4 * 64 * KW;                       // [wave][gate][16 actors][16 units]
    // epilogue operands first (oldest in the vmcnt order: complete before any piece that is waited for)
    const int a_ = tid >> 4, u_ = tid & 15;
    const int n = min(n0 + a_, N - 1), j = j0 + u_;
    // 32 pieces of 1 KiB: two rows each (lanes 0..31 / 32..63), 8 for the actors' h rows, then 8 per gate
    const int half = lane >> 5, unit = lane & 31;
    const int kw0 = wave * KW;
#pragma unroll
    for (int p = 0; p < 32; ++p) {
        const int r = 2 * p + half;                        // row of this lane
        const float* row;
        if (p < 8) row = hprev + (long)min(n0 + r, N - 1) * H;
        else {
            const int c = r - 16;
            row = Whh + ((long)(c >> 4) * H + j0 + (c & 15)) * H;
        }
        const float* src = row + kw0 + 4 * (unit ^ (r & 15));
        __builtin_amdgcn_global_load_lds((gru_gbl_v*)src, (gru_lds_v*)(wl + 2 * p * KW), 16, 0, 0);
    }
    // the epilogue's operands go LAST (gi is an HBM miss; vmcnt retires in order, so in front they would hold every piece back)
    const float* gir = gi + (long)n * 3 * H;
    float gi_r = gru_gload(gir + j), gi_z = gru_gload(gir + H + j), gi_n = gru_gload(gir + 2 * H + j);
    float m = gru_gload(mask + n);
    float hp_raw = gru_gload(hprev + (long)n * H + j);
    float b_r = gru_gload(bhh + j), b_z = gru_gload(bhh + H + j), b_n = gru_gload(bhh + 2 * H + j);
    const int i = lane & 15, q = lane >> 4;
    const unsigned la = gru_lds_addr(wl + i * KW);
    unsigned sw[8];
#pragma unroll
    for (int s2 = 0; s2 < 8; ++s2) sw[s2] = 16u * (unsigned)((4 * s2 + q) ^ i);
    f32x4_t av[8], bv[8];
    asm volatile("s_waitcnt vmcnt(32)" ::: "memory");      // 8 scalar loads + 24 pieces may still be in flight
#pragma unroll
    for (int s2 = 0; s2 < 8; ++s2) av[s2] = gru_lread(la + sw[s2]);
    f32x4_t acc[3], acd[3];                                 // two chains per tile: the 16x16x4 MFMA issues every 32 cycles, depends at 40
#pragma unroll
    for (int g = 0; g < 3; ++g) {
        acc[g] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        acd[g] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        if (g == 0) asm volatile("s_waitcnt vmcnt(24)" ::: "memory");
        else if (g == 1) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        const unsigned lb = la + (unsigned)((16 + 16 * g) * KW * 4);
#pragma unroll
        for (int s2 = 0; s2 < 8; ++s2) bv[s2] = gru_lread(lb + sw[s2]);
#pragma unroll
        for (int s2 = 0; s2 < 8; ++s2) {
            switch (s2) {                                   // (8 reads in flight; the s2-th has returned when 7 - s2 remain)
                case 0: gru_lwait<7>(av[0], bv[0]); break;
                case 1: gru_lwait<6>(av[1], bv[1]); break;
                case 2: gru_lwait<5>(av[2], bv[2]); break;
                case 3: gru_lwait<4>(av[3], bv[3]); break;
                case 4: gru_lwait<3>(av[4], bv[4]); break;
                case 5: gru_lwait<2>(av[5], bv[5]); break;
                case 6: gru_lwait<1>(av[6], bv[6]); break;
                default: gru_lwait<0>(av[7], bv[7]); break;
            }
            acc[g] = mfma16f(av[s2][0], bv[s2][0], acc[g]);
            acd[g] = mfma16f(av[s2][1], bv[s2][1], acd[g]);
            acc[g] = mfma16f(av[s2][2], bv[s2][2], acc[g]);
            acd[g] = mfma16f(av[s2][3], bv[s2][3], acd[g]);
        }
        __builtin_amdgcn_sched_barrier(0);                  // (keep this tile's MFMAs in front of the next tile's piece wait)
    }
    // the scalar loads: landed after this wait; hand the epilogue operands to the compiler
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("" : "+v"(gi_r), "+v"(gi_z), "+v"(gi_n), "+v"(m), "+v"(hp_raw), "+v"(b_r), "+v"(b_z), "+v"(b_n));
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
        for (int r = 0; r < 4; ++r) part[((wave * 3 + g) * 16 + 4 * q + r) * 16 + i] = acc[g][r] + acd[g][r];   // (actor 4q + r, unit i)
    __syncthreads();
    if (n0 + a_ >= N) return;
    float gh[3];
#pragma unroll
    for (int g = 0; g < 3; ++g) {
        const int o = (g * 16 + a_) * 16 + u_;
        gh[g] = ((part[o] + part[3 * 256 + o]) + part[6 * 256 + o]) + part[9 * 256 + o];
    }
    const float hp = m * hp_raw;
    const float r = sigmoidf_(gi_r + m * gh[0] + b_r);
    const float z = sigmoidf_(gi_z + m * gh[1] + b_z);
    const float hn = m * gh[2] + b_n;
    const float nn = tanhf(gi_n + r * hn);
    const long o = (long)n * H + j;
    hout[o] = (1.f - z) * nn + z * hp;
    float* gp = gates + (long)n * 3 * H;
    gp[j] = r; gp[H + j] = z; gp[2 * H + j] = nn;
    hn_s[o] = hn;
    hp_s[o] = hp;
}

// Backward step, same scheme: dh[n, j] = dhs + carry + m_{t+1} sum_k dghb_{t+1}[n, k] W_hh^T[j, k] with K = 3H = 1536; a
// wave owns 384 k, walked as three 128-k sub-chunks through two private 16-KB buffers (the third sub-chunk's pieces are
// issued into buffer 0 as soon as the wave has read sub-chunk 0 out of it).  Two accumulators alternate so that the
// dependent-issue latency of the 16x16x4 MFMA (40 vs 32 cycles) stays hidden.
__global__ __launch_bounds__(256) void gru_step_bwd512_kernel(const float* __restrict__ dghb_next, const float* __restrict__ WhhT,
                                                             const float* __restrict__ mask_next, const float* __restrict__ dhs,
                                                             float* __restrict__ carry, const float* __restrict__ gates,
                                                             const float* __restrict__ hn_s, const float* __restrict__ hp_s,
                                                             const float* __restrict__ mask, float* __restrict__ dgi,
                                                             float* __restrict__ dghb, int N) {
    constexpr int H = 512, K = 3 * H, KS = 128;
    extern __shared__ __attribute__((aligned(16))) float gsm[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j0 = blockIdx.x * 16, n0 = blockIdx.y * 16;
    float* wl = gsm + wave * (2 * 32 * KS);                // two buffers of 32 rows x 128 floats
    float* part = gsm + 4 * 2 * 32 * KS;
    const int a_ = tid >> 4, u_ = tid & 15;
    const int n = min(n0 + a_, N - 1), j = j0 + u_;
    const long o = (long)n * H + j;
    const int half = lane >> 5, unit = lane & 31;
    const int kw0 = wave * (3 * KS);
    auto issue = [&](int sc, int buf) {
#pragma unroll
        for (int p = 0; p < 16; ++p) {
            const int rr = 2 * p + half;
            const float* row = (p < 8) ? dghb_next + (long)min(n0 + rr, N - 1) * K : WhhT + (long)(j0 + rr - 16) * K;
            const float* src = row + kw0 + sc * KS + 4 * (unit ^ (rr & 15));
            __builtin_amdgcn_global_load_lds((gru_gbl_v*)src, (gru_lds_v*)(wl + buf * (32 * KS) + 2 * p * KS), 16, 0, 0);
        }
    };
    const int i = lane & 15, q = lane >> 4;
    const unsigned la = gru_lds_addr(wl + i * KS);
    unsigned sw[8];
#pragma unroll
    for (int s2 = 0; s2 < 8; ++s2) sw[s2] = 16u * (unsigned)((4 * s2 + q) ^ i);
    f32x4_t acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    auto contract = [&](int buf) {
        const unsigned pa = la + (unsigned)(buf * 32 * KS * 4), pb = pa + 16u * KS * 4;
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {                    // 2 x (4 A + 4 B reads in flight, then 16 MFMAs)
            f32x4_t av[4], bv[4];
#pragma unroll
            for (int s2 = 0; s2 < 4; ++s2) {
                av[s2] = gru_lread(pa + sw[4 * hf + s2]);
                bv[s2] = gru_lread(pb + sw[4 * hf + s2]);
            }
#pragma unroll
            for (int s2 = 0; s2 < 4; ++s2) {
                switch (s2) {
                    case 0: gru_lwait<6>(av[0], bv[0]); break;
                    case 1: gru_lwait<4>(av[1], bv[1]); break;
                    case 2: gru_lwait<2>(av[2], bv[2]); break;
                    default: gru_lwait<0>(av[3], bv[3]); break;
                }
                acc0 = mfma16f(av[s2][0], bv[s2][0], acc0);
                acc1 = mfma16f(av[s2][1], bv[s2][1], acc1);
                acc0 = mfma16f(av[s2][2], bv[s2][2], acc0);
                acc1 = mfma16f(av[s2][3], bv[s2][3], acc1);
            }
        }
    };
    issue(0, 0);
    issue(1, 1);
    // the epilogue's operands (HBM misses) behind the first two sub-chunks in the in-order vmcnt queue
    const float* g = gates + (long)n * 3 * H;
    float r = gru_gload(g + j), z = gru_gload(g + H + j), nn = gru_gload(g + 2 * H + j);
    float hn = gru_gload(hn_s + o), hp = gru_gload(hp_s + o);
    float dhs_v = gru_gload(dhs + o), carry_v = gru_gload(carry + o);
    float mn = gru_gload(mask_next + n), m = gru_gload(mask + n);
    asm volatile("s_waitcnt vmcnt(25)" ::: "memory");      // sub-chunk 1 (16 pieces) + 9 scalar loads may be in flight
    contract(0);                                           // (ends on lgkmcnt(0): this wave's reads of buffer 0 have returned)
    __builtin_amdgcn_sched_barrier(0);
    issue(2, 0);
    asm volatile("s_waitcnt vmcnt(25)" ::: "memory");      // 9 scalar loads + sub-chunk 2
    contract(1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    contract(0);
    asm volatile("" : "+v"(r), "+v"(z), "+v"(nn), "+v"(hn), "+v"(hp), "+v"(dhs_v), "+v"(carry_v), "+v"(mn), "+v"(m));
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) part[(wave * 16 + 4 * q + rr) * 16 + i] = acc0[rr] + acc1[rr];
    __syncthreads();
    if (n0 + a_ >= N) return;
    const int po = a_ * 16 + u_;
    const float proj = ((part[po] + part[256 + po]) + part[512 + po]) + part[768 + po];
    const float dh = dhs_v + (carry_v + mn * proj);
    const float dn_pre = dh * (1.f - z) * (1.f - nn * nn);
    const float dz_pre = dh * (hp - nn) * z * (1.f - z);
    const float dr_pre = dn_pre * hn * r * (1.f - r);
    float* ga = dgi + (long)n * 3 * H;
    float* gb = dghb + (long)n * 3 * H;
    ga[j] = dr_pre; ga[H + j] = dz_pre; ga[2 * H + j] = dn_pre;
    gb[j] = dr_pre; gb[H + j] = dz_pre; gb[2 * H + j] = dn_pre * r;
    carry[o] = m * dh * z;
}

// part[blockIdx.y][n] = sum over the block's rows of Y[m*ld + n]   (no atomics: colsum_fold_kernel adds the row blocks in order)
__global__ void colsum_kernel(const float* __restrict__ Y, float* __restrict__ out, long M, int N, int ld,
                              int rows_per_block) {
    const int n = blockIdx.x * 64 + (threadIdx.x & 63);
    const int sub = threadIdx.x >> 6;   // 4 row lanes
    const long r0 = (long)blockIdx.y * rows_per_block;
    const long r1 = min(M, r0 + rows_per_block);
    float s = 0.f;
    if (n < N)
        for (long r = r0 + sub; r < r1; r += 4) s += Y[r * ld + n];
    __shared__ float red[4][64];
    red[sub][threadIdx.x & 63] = s;
    __syncthreads();
    if (sub == 0 && n < N) out[(long)blockIdx.y * N + n] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// The same for wide matrices (N % 4 == 0, ld % 4 == 0: the GRU's [T*N x 3H] gate gradients, 100 MB each per optimiser step):
// 16-B loads, 8 of them in flight per lane, 64 x 4 columns per wave and rows_per_block / 4 rows per wave -- HBM-bound
// instead of latency-bound (280 -> ~30 us per call).
__global__ __launch_bounds__(256) void colsum4_kernel(const float* __restrict__ Y, float* __restrict__ out, long M, int N, int ld,
                                                     int rows_per_block) {
    const int lane = threadIdx.x & 63, sub = threadIdx.x >> 6;
    const int c = (blockIdx.x * 64 + lane) * 4;
    const long r0 = (long)blockIdx.y * rows_per_block;
    const long r1 = min(M, r0 + rows_per_block);
    f32x4_t s = {0.f, 0.f, 0.f, 0.f};
    if (c < N) {
        const float* base = Y + c;
        long r = r0 + sub;
        for (; r + 28 < r1; r += 32) {
            f32x4_t v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = *reinterpret_cast<const f32x4_t*>(base + (r + 4 * k) * ld);
#pragma unroll
            for (int k = 0; k < 8; ++k) s += v[k];
        }
        for (; r < r1; r += 4) s += *reinterpret_cast<const f32x4_t*>(base + r * ld);
    }
    __shared__ f32x4_t red[4][64];
    red[sub][lane] = s;
    __syncthreads();
    if (c < N) out[(long)blockIdx.y * N + c + sub] = ((red[0][lane][sub] + red[1][lane][sub]) + red[2][lane][sub]) + red[3][lane][sub];
}

// dE1[goal[b], n] += sum_p dm1[(b*S + p)*N + n]
__global__ void group_sum_scatter_kernel(const float* __restrict__ dm1, const int* __restrict__ goal,
                                         float* __restrict__ dE1, int S, int N, long B) {
    const long b = blockIdx.x;
    if (b >= B) return;
    for (int n = threadIdx.x; n < N; n += blockDim.x) {
        const float* p = dm1 + b * S * N + n;
        float s = 0.f;
        for (int q = 0; q < S; ++q) s += p[(long)q * N];
        atomicAdd(dE1 + (long)goal[b] * N + n, s);
    }
}

// ---- coordinate goals (ec_policy_cfg.goal_in > 0; [U] ResnetTensorPointNavActorCritic: embed_goal = nn.Linear(goal_in, goal_dims)) ----
// A goal that is a vector per frame cannot be tabulated: the goal half of target_obs_combiner.0 becomes a PER-FRAME bias row
//     Eg[b, :]  = goal_vec[b, :] Wc^T + bc                 [B, goal_dims]
//     E1f[b, :] = Eg[b, :] W3[:, co:]^T + b3               [B, comb_hid]
// that the combiner's first stage adds to the rows of frame b.  One launch per forward call, every mode: both products are
// fmaf chains over a frame's own values in a fixed order, so a frame's row does not depend on the batch it arrives in, and
// nothing goal-derived is ever cached.  FR frames per pass of a workgroup; W3[:, co:], Wc and the biases sit in LDS.
constexpr int GV_FR = 8;
__global__ __launch_bounds__(256) void goal_vec_fwd_kernel(const float* __restrict__ gv, const float* __restrict__ Wc,
                                                          const float* __restrict__ bc, const float* __restrict__ W3b, int w3_ld,
                                                          const float* __restrict__ b3, float* __restrict__ Eg,
                                                          float* __restrict__ E1f, long B, int gin, int gd, int ch) {
    extern __shared__ float gsm_[];
    float* sW3 = gsm_;                       // [ch][gd + 1]
    float* sWc = sW3 + ch * (gd + 1);        // [gd][gin]
    float* sbc = sWc + gd * gin;             // [gd]
    float* sb3 = sbc + gd;                   // [ch]
    float* sEg = sb3 + ch;                   // [GV_FR][gd]
    const int tid = threadIdx.x;
    for (int i = tid; i < ch * gd; i += 256) sW3[(i / gd) * (gd + 1) + i % gd] = W3b[(long)(i / gd) * w3_ld + i % gd];
    for (int i = tid; i < gd * gin; i += 256) sWc[i] = Wc[i];
    for (int i = tid; i < gd; i += 256) sbc[i] = bc[i];
    for (int i = tid; i < ch; i += 256) sb3[i] = b3[i];
    for (long b0 = (long)blockIdx.x * GV_FR; b0 < B; b0 += (long)gridDim.x * GV_FR) {
        const int nf = (int)min((long)GV_FR, B - b0);
        __syncthreads();                     // the tables are staged / the previous pass has read sEg
        for (int e = tid; e < nf * gd; e += 256) {
            const int f = e / gd, j = e - f * gd;
            const float* g = gv + (b0 + f) * gin;
            float v = sbc[j];
            for (int q = 0; q < gin; ++q) v = fmaf(g[q], sWc[j * gin + q], v);
            sEg[e] = v;
            Eg[(b0 + f) * gd + j] = v;
        }
        __syncthreads();
        for (int e = tid; e < nf * ch; e += 256) {
            const int f = e / ch, n = e - f * ch;
            float v = sb3[n];
            for (int j = 0; j < gd; ++j) v = fmaf(sEg[f * gd + j], sW3[n * (gd + 1) + j], v);
            E1f[(b0 + f) * ch + n] = v;
        }
    }
}
// dEg[b, j] = sum_n dE1f[b, n] W3[n, co + j]   (n ascending: one thread per output, no atomics)
__global__ __launch_bounds__(256) void goal_vec_bwd_kernel(const float* __restrict__ dE1f, const float* __restrict__ W3b, int w3_ld,
                                                          float* __restrict__ dEg, long B, int gd, int ch) {
    extern __shared__ float gsm_[];
    float* sW3 = gsm_;                       // [ch][gd + 1]
    float* sD = sW3 + ch * (gd + 1);         // [GV_FR][ch]
    const int tid = threadIdx.x;
    for (int i = tid; i < ch * gd; i += 256) sW3[(i / gd) * (gd + 1) + i % gd] = W3b[(long)(i / gd) * w3_ld + i % gd];
    for (long b0 = (long)blockIdx.x * GV_FR; b0 < B; b0 += (long)gridDim.x * GV_FR) {
        const int nf = (int)min((long)GV_FR, B - b0);
        __syncthreads();
        for (int e = tid; e < nf * ch; e += 256) sD[e] = dE1f[b0 * ch + e];
        __syncthreads();
        for (int e = tid; e < nf * gd; e += 256) {
            const int f = e / gd, j = e - f * gd;
            float v = 0.f;
            for (int n = 0; n < ch; ++n) v = fmaf(sD[f * ch + n], sW3[n * (gd + 1) + j], v);
            dEg[(b0 + f) * gd + j] = v;
        }
    }
}
// dE1f[b, n] = sum over the tiles that hold rows of frame b, in tile order, of the segment sums tail_bwd_kernel<true> left:
// seg[t][0] = column sums of dm1 over the rows of tile t that belong to the frame its first row is in, seg[t][1] = over the
// rest (the next frame: S >= 32, so a 32-row tile touches at most two frames)
__global__ __launch_bounds__(128) void seg_fold_kernel(const float* __restrict__ seg, float* __restrict__ dE1f, int S, long B) {
    const long b = blockIdx.x;
    const int n = threadIdx.x;
    const long t0 = b * S / 32, t1 = ((b + 1) * S - 1) / 32;
    float s = 0.f;
    for (long t = t0; t <= t1; ++t) s += seg[(t * 2 + ((t * 32) / S == b ? 0 : 1)) * 128 + n];
    dE1f[b * 128 + n] = s;
}
// the same off a materialised dm1 (the unfused tail): dE1f[b, n] = sum_p dm1[(b*S + p)*N + n]
__global__ void frame_sum_kernel(const float* __restrict__ dm1, float* __restrict__ dE1f, int S, int N) {
    const long b = blockIdx.x;
    for (int n = threadIdx.x; n < N; n += blockDim.x) {
        const float* p = dm1 + b * S * N + n;
        float s = 0.f;
        for (int q = 0; q < S; ++q) s += p[(long)q * N];
        dE1f[b * N + n] = s;
    }
}
// part[y][m*No + n] = sum over row block y (rows ascending) of A[r*lda + m] X[r*ldx + n]: the small weight gradients of the
// goal half (dW3[:, co:] = dE1f^T Eg, dWc = dEg^T goal_vec) over all T*N frames; splitk_fold_kernel adds the row blocks in
// order onto the gradient.  32 rows at a time through LDS, 16 outputs per thread and sweep.
__global__ __launch_bounds__(256) void tn_small_part_kernel(const float* __restrict__ A, int lda, const float* __restrict__ X, int ldx,
                                                           float* __restrict__ part, int Mo, int No, long K, int rows_per_block) {
    extern __shared__ float gsm_[];
    float* sA = gsm_;                        // [32][Mo]
    float* sX = sA + 32 * Mo;                // [32][No]
    const int tid = threadIdx.x, ne = Mo * No;
    const long r0 = (long)blockIdx.x * rows_per_block, r1 = min(K, r0 + rows_per_block);
    for (int e0 = 0; e0 < ne; e0 += 4096) {
        float acc[16];
        int am[16], an[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int e = min(e0 + tid + 256 * q, ne - 1);
            acc[q] = 0.f; am[q] = e / No; an[q] = e - am[q] * No;
        }
        for (long c0 = r0; c0 < r1; c0 += 32) {
            const int nr = (int)min((long)32, r1 - c0);
            __syncthreads();
            for (int i = tid; i < nr * Mo; i += 256) sA[i] = A[(c0 + i / Mo) * lda + i % Mo];
            for (int i = tid; i < nr * No; i += 256) sX[i] = X[(c0 + i / No) * ldx + i % No];
            __syncthreads();
            for (int r = 0; r < nr; ++r)
#pragma unroll
                for (int q = 0; q < 16; ++q) acc[q] = fmaf(sA[r * Mo + am[q]], sX[r * No + an[q]], acc[q]);
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int e = e0 + tid + 256 * q;
            if (e < ne && e < e0 + 4096) part[(long)blockIdx.x * ne + e] = acc[q];
        }
    }
}

// zero-shot fusion: x[b, :] = feat[b, :] / |feat[b, :]| * table[goal[b], :]   (one wave per row; fp32 statistics)
template <bool BF16>
__global__ __launch_bounds__(256) void fuse_goal_kernel(const void* __restrict__ feat, const float* __restrict__ table,
                                                       const int* __restrict__ goal, float* __restrict__ x, long B, int E,
                                                       int num_goals) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= B) return;
    float ss = 0.f;
    for (int k = lane; k < E; k += 64) {
        const float v = BF16 ? ec_bf2f(((const uint16_t*)feat)[row * E + k]) : ((const float*)feat)[row * E + k];
        ss += v * v;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor(ss, off, 64);
    const float inv = 1.f / fmaxf(sqrtf(ss), 1e-12f);
    int g = goal[row];
    g = g < 0 ? 0 : (g >= num_goals ? num_goals - 1 : g);
    const float* t = table + (long)g * E;
    for (int k = lane; k < E; k += 64) {
        const float v = BF16 ? ec_bf2f(((const uint16_t*)feat)[row * E + k]) : ((const float*)feat)[row * E + k];
        x[row * E + k] = v * inv * t[k];
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Fused forward "tail" of ResnetTensorGoalEncoder (round 2): for every feature-map pixel (row)
//     c2 = relu(W2 c1 + b2)            128 -> 32    (resnet_compressor.2)
//     m1 = relu(W3[:, :32] c2 + E1[goal])  32 -> 128   (target_obs_combiner.0; the goal half is the row-group bias E1)
//     x4 = W4 m1 + b4                  128 -> 32    (target_obs_combiner.2)
// in ONE pass over c1 instead of three GEMM launches that each stream a [T*N*49, 128] fp32 tensor through HBM with
// 32- or 128-long contractions (0.5-0.9 ms each per slice and epoch against ~0.2 ms of traffic for all three together).
// A wave owns 32-row tiles: the c1 tile is staged in a wave-private LDS image, each stage runs on the exact-fp32 MFMA
// (v_mfma_f32_32x32x2_f32, an fmaf chain) with the weights resident in LDS as B operands, and a stage's output tile goes
// back to the wave's LDS image (bias + ReLU applied) as the next stage's A operand -- and to HBM, because the backward
// needs c2 and m1.  No workgroup barrier after the weights are staged.  Geometry fixed to the reference's
// (128, 32, 128, 32); other widths keep the GEMM path.
// Fragment-order copies of the act step's two weight operands (built with the other weight-derived tables, once per
// parameter update): a fragment = what one MFMA operand load of a wave fetches = 64 lanes x 16 B = ONE contiguous 1-KB unit.
// Out of the row-major tables a fragment load touched 32 rows x 32 B -- 64 quarter-used sectors per instruction -- and the
// act kernels ran at the resulting L2 -> L1 rate (gi 16-19 us, c1 19 us at 32 actors).
//   fp32 [N][K]  (gi):  unit (cb * K/8 + g) * 64 + l  =  row 32 cb + (l & 31), k = 8 g + 4 (l >> 5) .. + 3
//   bf16 planes [N][3][K] (c1):  unit ((cb * K/16 + ks) * 3 + pl) * 64 + l  =  row 32 cb + (l & 31), plane pl, k = 16 ks + 8 (l >> 5) .. + 7
__global__ void frag_pack_f32_kernel(const float4* __restrict__ W, float4* __restrict__ F, int N, int K) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long)N * K / 4) return;
    const int l = (int)(t & 63);
    const long f = t >> 6;
    const int G = K / 8, g = (int)(f % G), cb = (int)(f / G);
    F[t] = W[((long)(cb * 32 + (l & 31)) * K + g * 8 + 4 * (l >> 5)) >> 2];
}
__global__ void frag_pack_planes_kernel(const uint4* __restrict__ P, uint4* __restrict__ F, int N, int K) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long)N * 3 * K / 8) return;
    const int l = (int)(t & 63);
    const long f = t >> 6;
    const int pl = (int)(f % 3);
    const long f2 = f / 3;
    const int KS = K / 16, ks = (int)(f2 % KS), cb = (int)(f2 / KS);
    F[t] = P[(((long)(cb * 32 + (l & 31)) * 3 + pl) * K + ks * 16 + 8 * (l >> 5)) >> 3];
}

// Act step (T = 1): the GRU's input projection gi[N][3H] = x[N][K] W[3H][K]^T + b for a handful of actor rows (N = 32..128),
// K = 1568.  As a tiled GEMM this is 24-96 workgroups walking K in series behind a split-K fold (18 us at 32 actors);
// here a workgroup owns a 32 x 32 output tile and its NW waves SPLIT K (224 each for K = 1568 = 7 x 224), fragments straight
// from global memory as float4 (exact-fp32 MFMA 32x32x2: an operand is one element per lane, so a float4 feeds four MFMAs),
// the NW partial tiles folded through LDS in wave order + bias: deterministic, no atomics, no partial matrices in HBM.
template <int NW>
__global__ __launch_bounds__(NW * 64) void gi_act_kernel(const float* __restrict__ x, const float* __restrict__ W,
                                                         const float* __restrict__ bias, float* __restrict__ gi, int N, int K,
                                                         int NO) {
    ec_gi_act_body<NW, false>(x, W, bias, gi, N, K, NO, ec_gi_act_pa{});      // (the body: common.h, shared with prev_action.hip's instance)
}

// Act step: the compressor's first 1x1 conv over the slice's bf16 feature rows, c1[M][NO] = relu(feat[M][K] W1[NO][K]^T + b1)
// (M = 49 n rows, K = 2048, NO = 128), exact-fp32 as everywhere in the policy: W1 arrives as three bf16 planes
// ([NO][3][K], ec_split3_bf16, cached in the act workspace with the other weight-derived tables) and each k-step runs the
// three plane products, lowest plane first, into one accumulator.  A workgroup owns a 32 x 32 output tile and its eight
// waves split K (fragments straight from global memory); the partial tiles are folded through LDS in wave order.  Replaces
// a split-K GEMM whose four partial matrices tail_fwd_kernel had to fold.
template <int MBLK, int U>
__global__ __launch_bounds__(512) void c1_act_kernel(const uint16_t* __restrict__ feat, const uint16_t* __restrict__ Wp,
                                                     const float* __restrict__ bias, float* __restrict__ c1, long M, int K, int NO) {
    // MBLK 32-row blocks per workgroup (the W slice is fetched once per workgroup: taller tiles for larger M), U k-steps of
    // fragment loads in flight per wave (the loop is L2-latency-bound: few, deep rounds)
    constexpr int NW = 8;
    __shared__ float part[NW][32][33];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 31, hh = lane >> 5;
    const int j0 = blockIdx.x * 32;
    const long m0 = (long)blockIdx.y * (32 * MBLK);
    const int kw = K / NW, k0 = wave * kw;
    const uint16_t* pa[MBLK];
#pragma unroll
    for (int mb = 0; mb < MBLK; ++mb) pa[mb] = feat + min(m0 + mb * 32 + i, M - 1) * K + k0 + 8 * hh;
    // W1's planes in fragment order (frag_pack_planes_kernel): (k-step ks, plane pl) of column block cb is one 1-KB unit
    const s16x8_t* pbf = reinterpret_cast<const s16x8_t*>(Wp) + ((long)blockIdx.x * (K / 16) + k0 / 16) * 3 * 64 + lane;
    f32x16_t acc[MBLK];
#pragma unroll
    for (int mb = 0; mb < MBLK; ++mb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mb][r] = 0.f;
    for (int kb = 0; kb < kw; kb += 16 * U) {
        s16x8_t a[U][MBLK], b[U][3];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int kk = min(kb + 16 * u, kw - 16);
#pragma unroll
            for (int mb = 0; mb < MBLK; ++mb) a[u][mb] = *reinterpret_cast<const s16x8_t*>(pa[mb] + kk);
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) b[u][pl] = pbf[((kk >> 4) * 3 + pl) * 64];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (kb + 16 * u < kw) {
#pragma unroll
                for (int pl = 2; pl >= 0; --pl)
#pragma unroll
                    for (int mb = 0; mb < MBLK; ++mb)
                        acc[mb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, a[u][mb]),
                                                                          __builtin_bit_cast(bf16x8_t, b[u][pl]), acc[mb], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int mb = 0; mb < MBLK; ++mb) {
        if (mb) __syncthreads();                                  // the previous block's fold is done reading `part`
#pragma unroll
        for (int r = 0; r < 16; ++r) part[wave][(r & 3) + 8 * (r >> 2) + 4 * hh][i] = acc[mb][r];
        __syncthreads();
        for (int e = tid; e < 32 * 32; e += NW * 64) {
            const int row = e >> 5, col = e & 31;
            float v = part[0][row][col];
#pragma unroll
            for (int w2 = 1; w2 < NW; ++w2) v += part[w2][row][col];
            const long m = m0 + mb * 32 + row;
            if (m < M) c1[m * NO + j0 + col] = fmaxf(v + bias[j0 + col], 0.f);
        }
    }
}

constexpr int ACT_PARTS = 4, ACT_MAX_ROWS = 16384;   // act step: split-K factor of the two long-K GEMMs / row limit of that path
constexpr int TL_P128 = 132, TL_P32 = 36;     // LDS row pitches (floats): 16-byte slots of 16 consecutive rows differ

// VEC (coordinate goals, goal_in > 0): E1 is the per-frame bias E1f [M / S][128] and stays in global memory (16.8 MB at
// 32,768 frames: L2-resident next to the c1 stream); no table is staged (num_goals == 0) and `goal` is not read.  A 32-row
// tile touches at most two frames (S >= 32 on this variant): their two bias rows are fetched with the next c1 tile, ahead of
// the contractions, and the epilogue picks one by row.
template <bool VEC>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void tail_fwd_kernel(const float* __restrict__ c1, const float* __restrict__ W2,
                                                         const float* __restrict__ b2, const float* __restrict__ W3,
                                                         int w3_ld, const float* __restrict__ E1,
                                                         const int* __restrict__ goal, int S, int num_goals,
                                                         const float* __restrict__ W4, const float* __restrict__ b4,
                                                         float* __restrict__ c2, float* __restrict__ m1,
                                                         float* __restrict__ x4, long M, int c1_parts, long c1_pstride,
                                                         const float* __restrict__ b1, int gstride) {
    extern __shared__ __attribute__((aligned(16))) float tsm[];
    float* sW2 = tsm;                            // [32][132]
    float* sW3 = sW2 + 32 * TL_P128;             // [128][36]
    float* sW4 = sW3 + 128 * TL_P32;             // [32][132]
    float* sE1 = sW4 + 32 * TL_P128;             // [num_goals][128]
    float* sB = sE1 + num_goals * 128;           // b2[32], b4[32]
    float* wave_base = sB + 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float* T1 = wave_base + wave * (32 * TL_P128 + 32 * TL_P32);   // c1 tile, later the m1 tile
    float* T2 = T1 + 32 * TL_P128;                                 // c2 tile
    // (all of a thread's weight loads in flight before its first LDS store: ec_stage_all, common.h -- the act step's
    //  instance of this kernel is 13-25 workgroups whose prologue is on the rollout's critical chain)
    ec_stage_all<32 * 32, 256, float4>(tid,                        // W2: [32][128]
        [&](int idx) { return *reinterpret_cast<const float4*>(W2 + (idx >> 5) * 128 + (idx & 31) * 4); },
        [&](int idx, const float4& v) { *reinterpret_cast<float4*>(sW2 + (idx >> 5) * TL_P128 + (idx & 31) * 4) = v; });
    ec_stage_all<32 * 32, 256, float4>(tid,                        // W4: [32][128]
        [&](int idx) { return *reinterpret_cast<const float4*>(W4 + (idx >> 5) * 128 + (idx & 31) * 4); },
        [&](int idx, const float4& v) { *reinterpret_cast<float4*>(sW4 + (idx >> 5) * TL_P128 + (idx & 31) * 4) = v; });
    ec_stage_all<128 * 8, 256, float4>(tid,                        // W3[:, :32]: [128][32] out of rows of w3_ld floats
        [&](int idx) { return *reinterpret_cast<const float4*>(W3 + (long)(idx >> 3) * w3_ld + (idx & 7) * 4); },
        [&](int idx, const float4& v) { *reinterpret_cast<float4*>(sW3 + (idx >> 3) * TL_P32 + (idx & 7) * 4) = v; });
    for (int idx = tid; idx < num_goals * 32; idx += 256)
        *reinterpret_cast<float4*>(sE1 + idx * 4) = *reinterpret_cast<const float4*>(E1 + idx * 4);
    if (tid < 32) { sB[tid] = b2[tid]; sB[32 + tid] = b4[tid]; }
    __syncthreads();

    const int i = lane & 31, hh = lane >> 5;
    const long ntiles = (M + 31) / 32;
    const long tstep = (long)gridDim.x * 4;
    // c1 tiles are fetched one tile ahead into registers (16 float4 per lane: rows past M clamp to the last row)
    // (plain unrolled loops, no lambda: an array captured by a lambda lands in scratch memory)
    f32x4_t st[16];                                                // native vector type: HIP's float4 struct would be memcpy'd through scratch
    long tile = (long)blockIdx.x * 4 + wave;
#pragma unroll
    for (int q = 0; q < 16; ++q) {                                 // (unconditional, clamped: keeps st[] in registers)
        const int idx = lane + 64 * q, r = idx >> 5, c4 = idx & 31;
        st[q] = *reinterpret_cast<const f32x4_t*>(c1 + min(tile * 32 + r, M - 1) * 128 + c4 * 4);
    }
    // act step (c1_parts > 1): c1 arrives as split-K partial sums WITHOUT bias / ReLU -- folded here in a fixed order
    // (unconditional code on both paths: with one part the loop below does nothing and b1v stays 0 / relu off)
    const bool fold = c1_parts > 1;
    f32x4_t b1v = {0.f, 0.f, 0.f, 0.f};
    if (fold) b1v = *reinterpret_cast<const f32x4_t*>(b1 + (lane & 31) * 4);
    auto fold_parts = [&](f32x4_t v, long row, int c4) {
        for (int p2 = 1; p2 < c1_parts; ++p2) v += *reinterpret_cast<const f32x4_t*>(c1 + p2 * c1_pstride + row * 128 + c4 * 4);
        v += b1v;
        v[0] = fmaxf(v[0], 0.f); v[1] = fmaxf(v[1], 0.f); v[2] = fmaxf(v[2], 0.f); v[3] = fmaxf(v[3], 0.f);
        return v;
    };
    if (fold) {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int idx = lane + 64 * q, r = idx >> 5, c4 = idx & 31;
            st[q] = fold_parts(st[q], min(tile * 32 + r, M - 1), c4);
        }
    }
    for (; tile < ntiles; tile += tstep) {
        const long m0 = tile * 32;
        const long grp_base = m0 / S;                               // wave-uniform
        const int grp_rem = (int)(m0 - grp_base * S);
        const int last_row = (int)min((long)31, M - 1 - m0);
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int idx = lane + 64 * q, r = idx >> 5, c4 = idx & 31;
            *reinterpret_cast<f32x4_t*>(T1 + r * TL_P128 + c4 * 4) = st[q];
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) {                             // next tile: in flight under this tile's three contractions
            const int idx = lane + 64 * q, r = idx >> 5, c4 = idx & 31;
            st[q] = *reinterpret_cast<const f32x4_t*>(c1 + min((tile + tstep) * 32 + r, M - 1) * 128 + c4 * 4);
        }
        float ef0[4], ef1[4];                                      // VEC: this tile's two bias rows (columns jt * 32 + i)
        (void)ef0; (void)ef1; (void)last_row;
        if constexpr (VEC) {
            const long nframes = M / S;
            const float* e0 = E1 + min(grp_base, nframes - 1) * 128 + i;
            const float* e1 = E1 + min(grp_base + 1, nframes - 1) * 128 + i;
#pragma unroll
            for (int jt = 0; jt < 4; ++jt) { ef0[jt] = e0[jt * 32]; ef1[jt] = e1[jt * 32]; }
        }
        if (fold) {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int idx = lane + 64 * q, r = idx >> 5, c4 = idx & 31;
                st[q] = fold_parts(st[q], min((tile + tstep) * 32 + r, M - 1), c4);
            }
        }
        // ---- c2 = relu(c1 W2^T + b2) ----
        f32x16_t acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        for (int kb = 0; kb < 128; kb += 8) {
            const float4 a = *reinterpret_cast<const float4*>(T1 + i * TL_P128 + kb + 4 * hh);
            const float4 b = *reinterpret_cast<const float4*>(sW2 + i * TL_P128 + kb + 4 * hh);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
        }
        {
            const float bj = sB[i];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * hh;     // C/D layout: column = lane & 31
                T2[row * TL_P32 + i] = fmaxf(acc[r] + bj, 0.f);
            }
        }
        // the tile leaves through the wave's LDS image as 16-byte row chunks (a lane of the C/D layout holds single floats)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int idx = lane + 64 * q, r = idx >> 3, c4 = idx & 7;
            if (m0 + r < M)
                *reinterpret_cast<float4*>(c2 + (m0 + r) * 32 + c4 * 4) = *reinterpret_cast<const float4*>(T2 + r * TL_P32 + c4 * 4);
        }
        // ---- m1 = relu(c2 W3a^T + E1[goal]) : four 32-column tiles, K = 32 ----
        f32x16_t am[4];
#pragma unroll
        for (int jt = 0; jt < 4; ++jt)
#pragma unroll
            for (int r = 0; r < 16; ++r) am[jt][r] = 0.f;
#pragma unroll
        for (int kb = 0; kb < 32; kb += 8) {
            const float4 a = *reinterpret_cast<const float4*>(T2 + i * TL_P32 + kb + 4 * hh);
#pragma unroll
            for (int jt = 0; jt < 4; ++jt) {
                const float4 b = *reinterpret_cast<const float4*>(sW3 + (jt * 32 + i) * TL_P32 + kb + 4 * hh);
                am[jt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, am[jt], 0, 0, 0);
                am[jt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, am[jt], 0, 0, 0);
                am[jt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, am[jt], 0, 0, 0);
                am[jt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, am[jt], 0, 0, 0);
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * hh;
            if constexpr (VEC) {
                const bool first = grp_rem + row < S;                // rows of the frame the tile starts in
#pragma unroll
                for (int jt = 0; jt < 4; ++jt)
                    T1[row * TL_P128 + jt * 32 + i] = fmaxf(am[jt][r] + (first ? ef0[jt] : ef1[jt]), 0.f);
            } else {
            // row group (actor-step) of this row in 32-bit arithmetic: a 64-bit division per element would cost more than the MFMAs
            const unsigned trow = min((unsigned)(grp_rem + row), (unsigned)(grp_rem + last_row));
            int g = goal[(grp_base + (long)(trow / (unsigned)S)) * gstride];   // (gstride 2: the low words of the caller's int64 ids)
            g = g < 0 ? 0 : (g >= num_goals ? num_goals - 1 : g);
            const float* e = sE1 + g * 128 + i;
#pragma unroll
            for (int jt = 0; jt < 4; ++jt)
                T1[row * TL_P128 + jt * 32 + i] = fmaxf(am[jt][r] + e[jt * 32], 0.f);   // (the c1 tile is dead by now)
            }
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int idx = lane + 64 * q, r = idx >> 5, c4 = idx & 31;
            if (m0 + r < M)
                *reinterpret_cast<float4*>(m1 + (m0 + r) * 128 + c4 * 4) = *reinterpret_cast<const float4*>(T1 + r * TL_P128 + c4 * 4);
        }
        // ---- x4 = m1 W4^T + b4 ----
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        for (int kb = 0; kb < 128; kb += 8) {
            const float4 a = *reinterpret_cast<const float4*>(T1 + i * TL_P128 + kb + 4 * hh);
            const float4 b = *reinterpret_cast<const float4*>(sW4 + i * TL_P128 + kb + 4 * hh);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
        }
        {
            const float bj = sB[32 + i];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * hh;
                T2[row * TL_P32 + i] = acc[r] + bj;                   // (the c2 tile is dead: m1's MFMAs have read it)
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int idx = lane + 64 * q, r = idx >> 3, c4 = idx & 7;
            if (m0 + r < M)
                *reinterpret_cast<float4*>(x4 + (m0 + r) * 32 + c4 * 4) = *reinterpret_cast<const float4*>(T2 + r * TL_P32 + c4 * 4);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Fused backward "tail" (round 2): the reverse of tail_fwd_kernel in ONE pass, for every 32-row tile
//     dm1 = (dx4 W4) * [m1 > 0]        32 -> 128      dW4 += dx4^T m1      db4 += colsum dx4     dE1[goal] += rowgroup-sum dm1
//     dc2 = (dm1 W3a) * [c2 > 0]       128 -> 32      dW3a += dm1^T c2
//     dc1 = (dc2 W2) * [c1 > 0]        32 -> 128      dW2 += dc2^T c1      db2 += colsum dc2     db1 += colsum dc1
// The GEMM path did this with three NN GEMMs, three TN GEMMs, three column sums and a row-group scatter, each streaming
// [T*N*49, 128|32] fp32 tensors through HBM (~9 ms per slice and epoch); this kernel reads dx4, m1, c2, c1 once and writes
// dc1 once (~1.4 GB, the floor).  A wave owns 32-row tiles; everything runs on the exact-fp32 MFMA (32x32x2): the data
// GEMMs read A rows as float4 from the wave's LDS image and B from transposed weight copies in LDS; the weight-gradient
// GEMMs contract over the tile's ROWS, so their operands are single floats of the same LDS images (lane = channel,
// k = row: the fp32 MFMA takes one element per lane, no transposed copy needed).  The weight gradients stay in the wave's
// accumulators for all of its tiles and leave as one partial set per wave; tail_bwd_reduce_kernel folds the sets into the
// gradient tensors.  dE1 is accumulated in an LDS table per workgroup (a 32-row tile touches at most two row groups: S >= 32).
constexpr int TB_MAX_WG = 256;
constexpr int TB_MAXG = 16;                       // goal rows of the per-wave dE1 register tables (num_goals <= 16 on the fused path)
constexpr int TB_W = 3 * 4096;                    // dW4 [32][128], dW3a [128][32], dW2 [32][128]
constexpr int TB_PART = TB_W + 64 + 64 + 256;     // + db4, db2 (two lane halves each), db1 (two halves)

// VEC (coordinate goals): there is no goal table to accumulate into -- the gradient of the per-frame bias is dE1f[b] = the sum of
// dm1 over the 49 rows of frame b, which span up to three tiles owned by different waves.  The tile's two row-group sums (the
// same two 128-float lines the table variant forms) leave as they are, partE[tile][2][128]; seg_fold_kernel adds a frame's
// segments in tile order.  8 floats of extra traffic per row against the ~1,300 B the tile already moves, no atomics, and no
// second pass over m1 / dx4 as a per-frame kernel would need.
template <bool VEC>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void tail_bwd_kernel(
    const float* __restrict__ dx4, const float* __restrict__ m1, const float* __restrict__ c2, const float* __restrict__ c1,
    const float* __restrict__ W2, const float* __restrict__ W3, int w3_ld, const float* __restrict__ W4,
    const int* __restrict__ goal, int S, int num_goals, float* __restrict__ dc1, uint16_t* __restrict__ dc1p,
    float* __restrict__ part, float* __restrict__ partE, long M) {
    extern __shared__ __attribute__((aligned(16))) float tsm[];
    float* sW4T = tsm;                            // [128 n][36]:  sW4T[n][k] = W4[k][n]
    float* sW3T = sW4T + 128 * TL_P32;            // [32 n][132]:  sW3T[n][k] = W3[k][n], n < 32
    float* sW2T = sW3T + 32 * TL_P128;            // [128 n][36]:  sW2T[n][k] = W2[k][n]
    float* sE = sW2T + 128 * TL_P32;              // [num_goals][128]
    float* wave_base = sE + (num_goals * 128 > 1024 ? num_goals * 128 : 1024);   // (== the host's tb_lds formula)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float* Tm = wave_base + wave * (32 * TL_P128 + 32 * TL_P32);   // m1 tile -> dm1 -> c1 tile -> dc1
    float* Tx = Tm + 32 * TL_P128;                                 // dx4 tile -> c2 tile -> dc2
    for (int idx = tid; idx < 4096; idx += 256) {
        const int k = idx >> 7, n = idx & 127;
        sW4T[n * TL_P32 + k] = W4[idx];
        sW2T[n * TL_P32 + k] = W2[idx];
        const int k3 = idx >> 5, n3 = idx & 31;
        sW3T[n3 * TL_P128 + k3] = W3[(long)k3 * w3_ld + n3];
    }
    __syncthreads();
    // dE1 (round 6: no float atomics): the tile's two row-group sums go through a wave-private 256-float line of the sE area
    // into PER-WAVE register tables regE[goal][2] (lane owns columns lane, lane + 64; the goal ids are wave-uniform, the
    // table update is 16 predicated adds) -- a wave folds its tiles in a fixed order, one table per wave leaves the kernel.
    float* sEw = sE + wave * 256;
    float regE[VEC ? 1 : TB_MAXG][2];
    if constexpr (!VEC) {
#pragma unroll
    for (int g = 0; g < TB_MAXG; ++g) { regE[g][0] = 0.f; regE[g][1] = 0.f; }
    }

    const int i = lane & 31, hh = lane >> 5;
    const long ntiles = (M + 31) / 32;
    const long tstep = (long)gridDim.x * 4;
    const long ngroups = (M + S - 1) / S;
    f32x16_t gW4[4], gW3[4], gW2[4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) { gW4[t][r] = 0.f; gW3[t][r] = 0.f; gW2[t][r] = 0.f; }
    float db4p = 0.f, db2p = 0.f, db1p[4] = {0.f, 0.f, 0.f, 0.f};
    f32x4_t sm[16], sx[4];                          // register prefetch (native vectors; see tail_fwd_kernel)
    long tile = (long)blockIdx.x * 4 + wave;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int idx = lane + 64 * q, r = idx >> 3, c4 = idx & 7;
        sx[q] = *reinterpret_cast<const f32x4_t*>(dx4 + min(tile * 32 + r, M - 1) * 32 + c4 * 4);
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int idx = lane + 64 * q, r = idx >> 5, c4 = idx & 31;
        sm[q] = *reinterpret_cast<const f32x4_t*>(m1 + min(tile * 32 + r, M - 1) * 128 + c4 * 4);
    }
    for (; tile < ntiles; tile += tstep) {
        const long m0 = tile * 32;
        const long grp_base = m0 / S;                                // wave-uniform
        const int nb = (int)((grp_base + 1) * S - m0);               // rows [0, nb) belong to group grp_base, the rest to the next
        // ---- stage dx4 (rows past M as zeros: they then contribute nothing anywhere) and m1 ----
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int idx = lane + 64 * q, r = idx >> 3, c4 = idx & 7;
            f32x4_t v = sx[q];
            if (m0 + r >= M) v = f32x4_t{0.f, 0.f, 0.f, 0.f};
            *reinterpret_cast<f32x4_t*>(Tx + r * TL_P32 + c4 * 4) = v;
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int idx = lane + 64 * q, r = idx >> 5, c4 = idx & 31;
            *reinterpret_cast<f32x4_t*>(Tm + r * TL_P128 + c4 * 4) = sm[q];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {                                // c2 and c1 of this tile: in flight under dW4 / dm1
            const int idx = lane + 64 * q, r = idx >> 3, c4 = idx & 7;
            sx[q] = *reinterpret_cast<const f32x4_t*>(c2 + min(m0 + r, M - 1) * 32 + c4 * 4);
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int idx = lane + 64 * q, r = idx >> 5, c4 = idx & 31;
            sm[q] = *reinterpret_cast<const f32x4_t*>(c1 + min(m0 + r, M - 1) * 128 + c4 * 4);
        }
        // ---- dW4[k][n] += sum_rows dx4[row][k] m1[row][n];  db4 ----
#pragma unroll 1
        for (int st = 0; st < 16; ++st) {
            const int row = 2 * st + hh;
            const float a = Tx[row * TL_P32 + i];
            db4p += a;
#pragma unroll
            for (int jt = 0; jt < 4; ++jt)
                gW4[jt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, Tm[row * TL_P128 + jt * 32 + i], gW4[jt], 0, 0, 0);
        }
        // ---- dm1 = (dx4 W4) * [m1 > 0] -> Tm;  dE1 row-group sums (one 32-column tile at a time: 16 live accumulators) ----
        {
            int g0 = 0, g1 = 0;
            if constexpr (!VEC) {
            g0 = goal[min(grp_base, ngroups - 1)]; g1 = goal[min(grp_base + 1, ngroups - 1)];
            g0 = g0 < 0 ? 0 : (g0 >= num_goals ? num_goals - 1 : g0);
            g1 = g1 < 0 ? 0 : (g1 >= num_goals ? num_goals - 1 : g1);
            }
#pragma unroll 1
            for (int jt = 0; jt < 4; ++jt) {
                f32x16_t acc;
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
                for (int kb = 0; kb < 32; kb += 8) {
                    const float4 a = *reinterpret_cast<const float4*>(Tx + i * TL_P32 + kb + 4 * hh);
                    const float4 b = *reinterpret_cast<const float4*>(sW4T + (jt * 32 + i) * TL_P32 + kb + 4 * hh);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
                }
                float e0 = 0.f, e1 = 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = (r & 3) + 8 * (r >> 2) + 4 * hh;     // C/D layout: column = lane & 31
                    float* pm = Tm + row * TL_P128 + jt * 32 + i;
                    const float v = (*pm > 0.f) ? acc[r] : 0.f;
                    *pm = v;
                    if (row < nb) e0 += v; else e1 += v;
                }
                e0 += __shfl_xor(e0, 32, 64);                        // the two lane halves hold the column's rows 4 hh .. : add them
                e1 += __shfl_xor(e1, 32, 64);
                if constexpr (VEC) {                                 // the two segment sums of this tile, straight to partE[tile][2][128]
                    if (hh == 0) { partE[tile * 256 + jt * 32 + i] = e0; partE[tile * 256 + 128 + jt * 32 + i] = e1; }
                } else {
                if (hh == 0) { sEw[jt * 32 + i] = e0; sEw[128 + jt * 32 + i] = e1; }
                }
            }
            (void)g0; (void)g1; (void)ngroups; (void)sEw;
            if constexpr (!VEC) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_wave_barrier();
            const float c0a = sEw[lane], c0b = sEw[64 + lane], c1a = sEw[128 + lane], c1b = sEw[192 + lane];
            const bool two = nb < 32;
#pragma unroll
            for (int g = 0; g < TB_MAXG; ++g) {
                regE[g][0] += (g == g0 ? c0a : 0.f) + ((two && g == g1) ? c1a : 0.f);
                regE[g][1] += (g == g0 ? c0b : 0.f) + ((two && g == g1) ? c1b : 0.f);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");       // (the line is rewritten by the next tile)
            __builtin_amdgcn_wave_barrier();
            }
        }
        // ---- stage c2 (dx4 is dead); fetch the next tile's dx4 ----
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int idx = lane + 64 * q, r = idx >> 3, c4 = idx & 7;
            *reinterpret_cast<f32x4_t*>(Tx + r * TL_P32 + c4 * 4) = sx[q];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int idx = lane + 64 * q, r = idx >> 3, c4 = idx & 7;
            sx[q] = *reinterpret_cast<const f32x4_t*>(dx4 + min((tile + tstep) * 32 + r, M - 1) * 32 + c4 * 4);
        }
        // ---- dW3a[m][c] += sum_rows dm1[row][m] c2[row][c] ----
#pragma unroll 1
        for (int st = 0; st < 16; ++st) {
            const int row = 2 * st + hh;
            const float b = Tx[row * TL_P32 + i];
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
                gW3[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(Tm[row * TL_P128 + mt * 32 + i], b, gW3[mt], 0, 0, 0);
        }
        // ---- dc2 = (dm1 W3a) * [c2 > 0] -> Tx;  db2 ----
        {
            f32x16_t acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
            for (int kb = 0; kb < 128; kb += 8) {
                const float4 a = *reinterpret_cast<const float4*>(Tm + i * TL_P128 + kb + 4 * hh);
                const float4 b = *reinterpret_cast<const float4*>(sW3T + i * TL_P128 + kb + 4 * hh);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * hh;
                float* px = Tx + row * TL_P32 + i;
                const float v = (*px > 0.f) ? acc[r] : 0.f;
                *px = v;
                db2p += v;
            }
        }
        // ---- stage c1 (dm1 is dead); fetch the next tile's m1 ----
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int idx = lane + 64 * q, r = idx >> 5, c4 = idx & 31;
            *reinterpret_cast<f32x4_t*>(Tm + r * TL_P128 + c4 * 4) = sm[q];
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int idx = lane + 64 * q, r = idx >> 5, c4 = idx & 31;
            sm[q] = *reinterpret_cast<const f32x4_t*>(m1 + min((tile + tstep) * 32 + r, M - 1) * 128 + c4 * 4);
        }
        // ---- dW2[k][n] += sum_rows dc2[row][k] c1[row][n] ----
#pragma unroll 1
        for (int st = 0; st < 16; ++st) {
            const int row = 2 * st + hh;
            const float a = Tx[row * TL_P32 + i];
#pragma unroll
            for (int jt = 0; jt < 4; ++jt)
                gW2[jt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, Tm[row * TL_P128 + jt * 32 + i], gW2[jt], 0, 0, 0);
        }
        // ---- dc1 = (dc2 W2) * [c1 > 0] -> Tm -> HBM;  db1 ----
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) {
            f32x16_t acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
            for (int kb = 0; kb < 32; kb += 8) {
                const float4 a = *reinterpret_cast<const float4*>(Tx + i * TL_P32 + kb + 4 * hh);
                const float4 b = *reinterpret_cast<const float4*>(sW2T + (jt * 32 + i) * TL_P32 + kb + 4 * hh);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
            }
            float d = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * hh;
                float* pm = Tm + row * TL_P128 + jt * 32 + i;
                const float v = (*pm > 0.f) ? acc[r] : 0.f;
                *pm = v;
                d += v;
            }
            db1p[jt] += d;
        }
        if (dc1p) {                                       // dc1 leaves as three bf16 planes [row][3][128]: the operand of ec_dw_tn_x3
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int idx = lane + 64 * q, r = idx >> 5, c4 = idx & 31;
                const float4 v = *reinterpret_cast<const float4*>(Tm + r * TL_P128 + c4 * 4);
                const float x[4] = {v.x, v.y, v.z, v.w};
                uint2 p0, p1, p2;
                ec_split3x4(x, p0, p1, p2);
                if (m0 + r < M) {
                    uint16_t* d = dc1p + (m0 + r) * 384 + c4 * 4;
                    *reinterpret_cast<uint2*>(d) = p0;
                    *reinterpret_cast<uint2*>(d + 128) = p1;
                    *reinterpret_cast<uint2*>(d + 256) = p2;
                }
            }
        } else {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int idx = lane + 64 * q, r = idx >> 5, c4 = idx & 31;
            if (m0 + r < M)
                *reinterpret_cast<float4*>(dc1 + (m0 + r) * 128 + c4 * 4) = *reinterpret_cast<const float4*>(Tm + r * TL_P128 + c4 * 4);
        }
        }
    }
    // ---- one partial set per wave; the dE1 table per workgroup ----
    float* pp = part + ((long)blockIdx.x * 4 + wave) * TB_PART;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * hh;
            pp[row * 128 + t * 32 + i] = gW4[t][r];                  // dW4[k = row][n = t*32 + i]
            pp[4096 + (t * 32 + row) * 32 + i] = gW3[t][r];          // dW3a[m = t*32 + row][c = i]
            pp[8192 + row * 128 + t * 32 + i] = gW2[t][r];           // dW2[k = row][n = t*32 + i]
        }
    pp[TB_W + hh * 32 + i] = db4p;
    pp[TB_W + 64 + hh * 32 + i] = db2p;
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) pp[TB_W + 128 + hh * 128 + jt * 32 + i] = db1p[jt];
    if constexpr (!VEC) {
    float* pe = partE + ((long)blockIdx.x * 4 + wave) * num_goals * 128;
#pragma unroll
    for (int g = 0; g < TB_MAXG; ++g)
        if (g < num_goals) { pe[g * 128 + lane] = regE[g][0]; pe[g * 128 + 64 + lane] = regE[g][1]; }
    }
}

// folds the per-wave partial sets of tail_bwd_kernel into the gradient tensors (grads +=, dE1 +=).  Two stages, no atomics:
// y-slice blockIdx.y adds the sets p = y, y + ny, ... in increasing order into red[y][e]; tail_bwd_fold_kernel adds the ny
// slices in slice order onto the gradient.
__device__ __forceinline__ float* tail_dst(int e, float* gW4, float* gW3, int w3_ld, float* gW2, float* gb4, float* gb2, float* gb1,
                                           float* dE1) {
    if (e < 4096) return gW4 + e;
    if (e < 8192) { const int q = e - 4096; return gW3 + (long)(q >> 5) * w3_ld + (q & 31); }
    if (e < TB_W) return gW2 + (e - 8192);
    if (e < TB_W + 64) return gb4 + ((e - TB_W) & 31);
    if (e < TB_W + 128) return gb2 + ((e - TB_W - 64) & 31);
    if (e < TB_PART) return gb1 + ((e - TB_W - 128) & 127);
    return dE1 + (e - TB_PART);
}
__global__ __launch_bounds__(256) void tail_bwd_reduce_kernel(const float* __restrict__ part, int nsets,
                                                               const float* __restrict__ partE, int num_goals,
                                                               float* __restrict__ red) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    const int ne = TB_PART + num_goals * 128;
    if (e >= ne) return;
    float s = 0.f;
    if (e < TB_PART) {
        for (int p = blockIdx.y; p < nsets; p += gridDim.y) s += part[(long)p * TB_PART + e];
    } else {
        const int q = e - TB_PART;
        for (int p = blockIdx.y; p < nsets; p += gridDim.y) s += partE[(long)p * num_goals * 128 + q];
    }
    red[(long)blockIdx.y * ne + e] = s;
}
// red[ny][ne] -> gradient; a bias element, whose two lane halves sit in 2 slots of a set, is summed by ONE thread
__global__ __launch_bounds__(256) void tail_bwd_fold_kernel(const float* __restrict__ red, int ny, int num_goals,
                                                             float* __restrict__ gW4, float* __restrict__ gW3, int w3_ld,
                                                             float* __restrict__ gW2, float* __restrict__ gb4, float* __restrict__ gb2,
                                                             float* __restrict__ gb1, float* __restrict__ dE1) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    const int ne = TB_PART + num_goals * 128;
    if (e >= ne) return;
    auto slot = [&](int q) { float t = 0.f; for (int y = 0; y < ny; ++y) t += red[(long)y * ne + q]; return t; };
    if (e >= TB_W && e < TB_PART) {                        // bias slots: [db4 h0 | db4 h1 | db2 h0 | db2 h1 | db1 h0 (128) | db1 h1 (128)]
        const int q = e - TB_W;
        if (q < 32) gb4[q] += slot(e) + slot(e + 32);
        else if (q >= 64 && q < 96) gb2[q - 64] += slot(e) + slot(e + 32);
        else if (q >= 128 && q < 256) gb1[q - 128] += slot(e) + slot(e + 128);
        return;
    }
    *tail_dst(e, gW4, gW3, w3_ld, gW2, gb4, gb2, gb1, dE1) += slot(e);
}

// out[n] += sum_m Y[m*ld + n] WITHOUT atomics: row block blockIdx.y leaves its column sums in part[y][n] (colsum_part* below),
// colsum_fold_kernel adds the row blocks in order
__global__ __launch_bounds__(256) void colsum_fold_kernel(const float* __restrict__ part, int nby, int N, float* __restrict__ out) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    float s = 0.f;
    for (int y = 0; y < nby; ++y) s += part[(long)y * N + n];
    out[n] += s;
}
// dW[m*ldc + n] += sum_k parts[k][m][n]: the ordered fold of a split-K weight-gradient GEMM's partial matrices (EC_GEMM_SPLIT_PARTS)
__global__ __launch_bounds__(256) void splitk_fold_kernel(const float* __restrict__ parts, int sk, int Mo, int No, int ldc,
                                                         float* __restrict__ dW) {
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    if (q >= (long)Mo * No) return;
    float s = 0.f;
    for (int k = 0; k < sk; ++k) s += parts[(long)k * Mo * No + q];
    const long m = q / No, n = q - m * No;
    dW[m * ldc + n] += s;
}

inline size_t al(size_t v) { return (v + 255) / 256 * 256; }

enum { P_EMB, P_W1, P_B1, P_W2, P_B2, P_W3, P_B3, P_W4, P_B4, P_WIH, P_WHH, P_BIH, P_BHH, P_WA, P_BA, P_WC, P_BC,
       // dual (RGB + depth) encoder: the depth stream's compressor / combiner, same shapes as P_W1 .. P_B4
       P_W1D, P_B1D, P_W2D, P_B2D, P_W3D, P_B3D, P_W4D, P_B4D,
       // coordinate goals (goal_in > 0): P_EMB is embed_goal.weight [goal_dims, goal_in], P_GB is embed_goal.bias, second in the flat order
       P_GB,
       // previous-action embedding (prev_action_dims > 0): prev_action_embedder.fc.weight [num_actions + null, E], last in the flat order
       P_PAE, P_COUNT };
constexpr int P_COUNT_SINGLE = P_BC + 1, P_COUNT_DUAL = P_B4D + 1, P_COUNT_VEC = P_COUNT_SINGLE + 1;

}  // namespace

struct ec_policy {
    ec_policy_cfg c;
    size_t off[P_COUNT] = {}, total = 0;
    // The flat buffer's tensors in flat order -- what ec_policy_param_offset's idx counts -- written by put() alone, which every
    // constructor calls tensor by tensor in that order.  count: ec_policy_num_param_tensors; slots >= count: the indices the lookup
    // answers (ec_policy_create_rnn_layers says which handle has more of them than tensors)
    struct Tensor { size_t off, num; };
    Tensor table[P_COUNT + 4 * (EC_RNN_MAX_LAYERS - 1)] = {};
    int count = 0, slots = 0;
    // `n` floats behind everything put so far, 16-byte aligned; -> their offset.  listed = false: a part this handle does not
    // have (n = 0) -- it gets the offset, and no index
    size_t put(size_t n, bool listed = true) {
        const size_t at = total;
        if (listed) table[slots++] = Tensor{at, n};
        total += (n + 3) / 4 * 4;
        return at;
    }
    const float* goal_table = nullptr;   // fusion == 1: borrowed f32 [num_goals, in_channels]
    int rnn = EC_RNN_GRU;                // the recurrent cell (ec_policy_create_rnn)
    // recurrent layers (ec_policy_create_rnn_layers).  Layer l >= 1 owns weight_ih_l{l} [G, H], weight_hh_l{l} [G, H], bias_ih_l{l},
    // bias_hh_l{l}: uoff [l - 1][0..3], behind every other tensor of the flat order
    int layers = 1;
    size_t uoff[EC_RNN_MAX_LAYERS - 1][4] = {};
    // The part of the flat order that every handle shares (c, rnn and layers are set): weight_ih_l0 [G, in0], weight_hh_l0,
    // bias_ih_l0, bias_hh_l0, the actor's weight and bias, the critic's; the previous-action table of a handle that has one;
    // then layer 1, 2, ...: weight_ih, weight_hh, bias_ih, bias_hh each
    void put_core(size_t in0) {
        const size_t H = c.hidden, A = c.num_actions, E = c.prev_action_dims, GW = (rnn == EC_RNN_LSTM ? 4 : 3) * H;
        const size_t n8[8] = {GW * in0, GW * H, GW, GW, A * H, A, H, 1}, un[4] = {GW * H, GW * H, GW, GW};
        for (int k = 0; k < 8; ++k) off[P_WIH + k] = put(n8[k]);
        off[P_PAE] = put((A + c.prev_action_null) * E, E != 0);
        for (int l = 1; l < layers; ++l)
            for (int k = 0; k < 4; ++k) uoff[l - 1][k] = put(un[k]);
    }
    // The pooled-embedding net (ec_policy_create_pooled).  Its plan is the fusion handle's -- no compressor, no combiner, the
    // recurrent core reads a [T*N, in_channels] matrix -- with in_channels = hidden: that matrix is v = ReLU(visual_fc(e)).
    // Tensors in front of weight_ih_l0, index into off: visual_fc weight, bias; the goal-id embedding; sensor i's weight, bias
    struct Pooled {
        bool on = false;
        int D = 0, ed = 0, ids = 0, ns = 0, k[3] = {0, 0, 0}, K = 0;   // ids: 1 with a goal-id embedding; K = sum k
        size_t off[9] = {};
        int side() const { return ed * (ids + ns); }                   // columns of weight_ih_l0 between v's and the previous action's
        // The two-view rearrangement net (ec_policy_create_two_view): the pooled plan from v onwards, with two_view.hip's trainable
        // front in place of visual_fc.  off [TV_WE .. TV_B2]: its six tensors; no goal-id embedding, no sensors, D unused
        bool tv = false;
        int tvC = 0, tvS2 = 0, tvA1 = 0;
    } pl;
    // EC_POLICY_INFER_REUSE bookkeeping: the key of the launch plan (make_plan) that built the weight-derived tables in a given
    // act workspace.  Which tables exist and where (E1, W1's planes in fragment order, the re-ordered weight_ih and its
    // fragment-order copy) are plan fields, and an inference plan is a function of exactly (handle, T, N, feature dtype): a
    // REUSE call whose plan has another key (fp32 features first, bf16 next; another N) rebuilds instead of reading
    // uninitialised tables.
    struct Built { int T, N, bf16; bool operator==(const Built&) const = default; };
    mutable std::mutex tables_mu;
    mutable std::unordered_map<const void*, Built> tables;
};

namespace {

int pick_splitk(long M, long N, long K) {
    const long tiles = ((M + 127) / 128) * ((N + 127) / 128);
    long s = 1024 / (tiles > 0 ? tiles : 1);
    const long nk = (K + 31) / 32;
    if (s > nk / 4) s = nk / 4;
    if (s < 1) s = 1;
    if (s > 256) s = 256;
    return (int)s;
}

// LinearActorHead + LinearCriticHead ([U] allenact basic_models.py): hv[b, :A] = hs[b] . Wa^T + ba, hv[b, A] = hs[b] . wc + bc.
// A+1 <= 8 outputs of a 512-long dot product per row: one wave per row (the tiled GEMM would run this as ONE
// workgroup -- 44 us for 128 rows).  Lane l owns elements l, l+64, ... of the row; fixed-order wave reduction.
// smp.actions != nullptr (ec_policy_act): the wave that owns a row also samples its action from the logits it has just reduced
// (CategoricalDistr.sample + log_prob, ec_sample_row: the arithmetic of sample_kernel) -- the act step's sixth launch folded into its fifth.
struct SampleArgs {
    long long* actions = nullptr;
    float* logp = nullptr;
    float* values = nullptr;
    uint64_t seed = 0, step = 0;
    int first_actor = 0;
    int greedy = 0;               // 1: CategoricalDistr.mode() (ec_mode_row: first maximal logit) instead of a draw; seed / step / first_actor unused
};
// ec_policy_act_ex: teacher forcing behind the selection (expert == nullptr: none)
struct ForceArgs {
    const long long* expert = nullptr;
    const float* mask = nullptr;
    float p = 0.f;
};
template <int MAXO>
__global__ __launch_bounds__(256) void heads_fwd_kernel(const float* __restrict__ hs, const float* __restrict__ Wa,
                                                       const float* __restrict__ ba, const float* __restrict__ Wc,
                                                       const float* __restrict__ bc, float* __restrict__ hv, long B,
                                                       int H, int A, SampleArgs smp) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= B) return;
    float acc[MAXO];
#pragma unroll
    for (int o = 0; o < MAXO; ++o) acc[o] = 0.f;
    const float* x = hs + row * H;
    if ((H & 255) == 0) {
        // lane l owns the 4 elements [4 l, 4 l + 4) of every 256-wide chunk: one float4 of the row and one of each output's
        // weight row per chunk, all MAXO + 1 loads of a chunk in flight together (the scalar-per-lane loop waited for
        // 8 dependent rounds of 8 loads: 17 us for a 9-us GRU step in front of it); outputs past A read Wc (discarded)
        for (int k0 = 0; k0 < H; k0 += 256) {
            const float4 v = *reinterpret_cast<const float4*>(x + k0 + 4 * lane);
            float4 wv[MAXO];
#pragma unroll
            for (int o = 0; o < MAXO; ++o)
                wv[o] = *reinterpret_cast<const float4*>((o < A ? Wa + (long)o * H : Wc) + k0 + 4 * lane);
#pragma unroll
            for (int o = 0; o < MAXO; ++o)
                acc[o] = fmaf(v.w, wv[o].w, fmaf(v.z, wv[o].z, fmaf(v.y, wv[o].y, fmaf(v.x, wv[o].x, acc[o]))));
        }
    } else {
        for (int k = lane; k < H; k += 64) {
            const float v = x[k];
#pragma unroll
            for (int o = 0; o < MAXO; ++o)
                if (o <= A) acc[o] = fmaf(v, (o < A ? Wa[(long)o * H + k] : Wc[k]), acc[o]);
        }
    }
#pragma unroll
    for (int o = 0; o < MAXO; ++o) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc[o] += __shfl_xor(acc[o], off, 64);
    }
    if (lane <= A) {
        float r = 0.f;
#pragma unroll
        for (int o = 0; o < MAXO; ++o)
            if (o == lane) r = acc[o];
        hv[row * (A + 1) + lane] = r + (lane < A ? ba[lane] : bc[0]);
    }
    if (smp.actions) {   // (wave-uniform) every lane holds every reduced output: lane 0 samples from the final logits
        float lg[MAXO];
#pragma unroll
        for (int o = 0; o < MAXO; ++o) lg[o] = acc[o] + (o < A ? ba[o] : (o == A ? bc[0] : 0.f));
        if (lane == 0) {
            int a;
            float lp;
            const auto logit = [&](int k) { float v = 0.f;
#pragma unroll
                                            for (int o = 0; o < MAXO; ++o) if (o == k) v = lg[o];
                                            return v; };
            if (smp.greedy) ec_mode_row(logit, A, a, lp);          // (a runtime field: the same kernel instance serves evaluation)
            else ec_sample_row(logit, A, smp.seed, smp.step, (uint64_t)(row + smp.first_actor), a, lp);
            smp.actions[row] = a;
            smp.logp[row] = lp;
            float vv = 0.f;
#pragma unroll
            for (int o = 0; o < MAXO; ++o) if (o == A) vv = lg[o];
            if (smp.values) smp.values[row] = vv;
        }
    }
}

// split-K for the small per-step GEMMs that only ever ACCUMULATE (atomics are fine): aim at ~1 workgroup
// per CU on 64x64 tiles while keeping >= 4 K-tiles per slice.
int step_splitk(long M, long N, long K) {
    const long blocks = ((M + 63) / 64) * ((N + 63) / 64);
    long s = 256 / (blocks > 0 ? blocks : 1);
    const long nk = (K + 31) / 32;
    if (s > nk / 4) s = nk / 4;
    return (int)(s < 1 ? 1 : s);
}

#define RC(x) do { int rc__ = (x); if (rc__ != EC_OK) return rc__; } while (0)

// ---- the launch plan --------------------------------------------------------------------------------------------------------
// Every size and every path decision of one entry-point call, made ONCE (make_plan) from the handle, (T, N), the mode and the
// feature dtype.  The workspace layout, the forward and the backward all read this one value, so they cannot disagree about how
// large an area is or which kernel wrote it.  A stack value: building it allocates nothing and takes no lock (it sits on the
// act step's serial launch chain).
constexpr size_t LDS_LIMIT = 160 * 1024;      // dynamic LDS a workgroup may ask for

struct Geo {
    int T, N, B;                  // B = T * N rows through the GRU and the heads
    int S, M49;                   // pixels per frame; B * S rows through compressor and combiner (0 in fusion mode)
    int H, A, A1, C, cat;         // hidden size; actions, actions + critic; feature channels; compress_out + goal_dims
    int nstream, flat1, flat;     // encoder streams (2: dual RGB + depth); one stream's / the whole GRU input width
    int E, R, ldw;                // previous-action embedding: width (0: none), table rows, weight_ih's row stride flat + X + E
    int X, pcol;                  // pooled-embedding net: the goal-id / sensor columns of weight_ih (0 elsewhere); the previous action's first column flat + X
    bool pooled; int D, PK, PG;   // pooled-embedding net: embedding width, sensor floats per frame, goal-table rows
    bool tv; int tvC, tvS2, tvA1; // two-view net (a pooled plan with another front): feature channels, pixels per frame, attention width
    int G, SW;                    // gate width 3H (GRU) | 4H (LSTM); state width H | 2H (an LSTM state row is [h | c])
    int L;                        // recurrent layers; a state row is [N, L * SW], layer l's state the slice at l * SW
};

struct Ws {   // float offsets into the workspace
    struct Stream { size_t E1, c1, c2, m1, x4; } st[2];   // per encoder stream ([1]: the dual encoder's depth stream)
    size_t x, gi, gh, gates, hn, hp, hs, goal32, w1p;
    // act step: weight_ih in pixel-major column order (valid while E1 is); the same / W1's planes in MFMA-FRAGMENT order (gi_act_kernel / c1_act_kernel)
    size_t wihA, wihF, w1pF;
    size_t dhs, dhc, dgi, dghb, dx, dx4, dm1, dc2, dc1, dE1, tpart, tpartE, whhT, wihP, gwihP, tA, tB, end;
    // coordinate goals (all empty with goal_in == 0): the per-frame bias rows and the goal embeddings of this call; the learn
    // pass's copy of the goal vectors; the backward's dE1f / dEg, the tail's per-tile segment sums, the row-block partials of
    // the two small weight gradients
    size_t E1f, Eg, gvec, dE1f, dEg, tseg, gpart;
    // learn pass of a wide handle (A + 1 > 8; all empty otherwise): both heads as one table [Wa; wc | ba; bc] ((A + 1) * H
    // weights, then A + 1 biases), the table's gradient in the same layout, the row-block partials of its column sum
    size_t hW, hG, hP;
    // previous-action embedding (all empty with prev_action_dims == 0): the table PT [R, 3H] (weight-derived: kept with E1 under
    // EC_POLICY_INFER_REUSE); the learn pass's copy of the int64 indices; ec_pa_grad_launch's scratch
    size_t pt, paidx, pas;
    // LSTM handles (all empty on a GRU handle): the cell-state history [B, H]; the backward's dL/dc carry [N, H].  On such a handle
    // `hn` holds the masked previous cell states, `dgi` the one gate gradient da, and `dghb` is empty.
    size_t cs, dcc;
    // layers l >= 1 of a multi-layer core (all empty with one layer), index l - 1: the layer's input projection gi [B, G], what its
    // step kernels keep (gates [B, G]; hn, hp [B, H]), its state history hs [B, H] (the top layer's feeds the heads) and, on an
    // LSTM handle, its cell-state history; uh0: a GRU stack's initial states as dense [L][N, H] blocks (its step kernels take no pitch)
    size_t ugi[EC_RNN_MAX_LAYERS - 1], ugates[EC_RNN_MAX_LAYERS - 1], uhn[EC_RNN_MAX_LAYERS - 1], uhp[EC_RNN_MAX_LAYERS - 1],
           uhs[EC_RNN_MAX_LAYERS - 1], ucs[EC_RNN_MAX_LAYERS - 1], uh0;
    // pooled-embedding net (all empty on every other handle).  Weight-derived, kept under EC_POLICY_INFER_REUSE: the goal-id table
    // GT [PG, G], SV [G, K], sb [G], visual_fc's weight in fragment order (act route); the learn pass's copies of the goal ids and
    // the sensor floats; the backward's dSV / dsb and the goal table's binned-sum scratch.  v [B, H] is the `x` area, dv `dx`, the
    // dense copy of weight_ih[:, :H] `wihA` (inference) / `wihP` (learn pass), as on a handle with a previous-action embedding.
    size_t gt, sv, sb, fcF, pgoal, psens, dsv, dsb, gts;
    // two-view net (all empty on every other handle): the combined conv weight as bf16 planes in fragment order (weight-derived,
    // kept under EC_POLICY_INFER_REUSE); the learn pass's attention probabilities [B, S2] and post-ReLU activations [B S2, A1 + H];
    // the backward's scratch (ec_tv_bwd_scratch_floats)
    size_t tvw, tva, tvact, tvs;
};
constexpr int GP_MAXY = 64;                   // row blocks of tn_small_part_kernel
constexpr int HP_MAXY = 128;                  // row blocks of the wide heads' column sum

enum class C1 { pingpong, act_kernel, split_parts, plain };      // compressor conv 1
enum class Gi { act7, act8, split_parts, plain };                // GRU input projection (act7 / act8: gi_act_kernel<7 | 8>)
enum class Wih { plain, perm_learn, perm_act };                  // weight_ih as stored / re-ordered per learn pass / per act-table build
enum class Step { gemm_gates, fused32, fused16 };                // a recurrence step: GEMM + gate kernel / 32-tile / 16-tile fused kernel
enum class Cell { gru, lstm };                                   // the recurrent cell (lstm.hip's kernels: always the 32-tile ones)
enum { PL_FCW, PL_FCB, PL_GEMB, PL_SW0, PL_SB0 };                // ec_policy::Pooled::off (sensor i: PL_SW0 + 2 i, PL_SB0 + 2 i)
enum { TV_WE, TV_BE, TV_WA, TV_BA, TV_W2, TV_B2, TV_NPRE };      // ... of a two-view handle
constexpr int PA_TABLE_MAX_E = 64;                               // widest previous-action embedding of prev_action.hip's table / chain kernels

struct Plan {
    Geo g;
    Cell cell;
    bool vec;                     // coordinate goals (goal_in > 0): per-frame bias rows instead of the goal-id table
    bool wide;                    // learn pass with A + 1 > 8: the heads through one packed table, and no float atomics on any route
    bool ordered;                 // no float atomics on any route of the backward: coordinate goals, wide handles, LSTM handles
    bool infer, feat_bf16;        // infer: EC_POLICY_INFER or _REUSE (stated by the caller, never inferred from the workspace size)
    ec_policy::Built key;         // what a REUSE call must match
    int act_parts;                // partial matrices the c1 / gi areas hold: ACT_PARTS for the act step's few rows, else 1
    C1 c1; int c1_mblk, c1_fold;  // c1_act_kernel's <MBLK, U> variant; partial matrices of c1 the fused tail folds
    int planes;                   // bf16 planes of the fp32 operand in the compressor conv and its weight gradient (EC_POLICY_FAST: 2 of 3)
    bool tail_fwd, tail_bwd;      // EC_TAIL_FUSED: c2 / m1 / x4 in one pass over c1, and its backward
    size_t tail_fwd_lds, tail_bwd_lds;
    Wih wih; bool goal_direct;    // the fused tail reads the low words of the int64 goal ids itself: no conversion launch
    Gi gi; int gi_fold;           // partial matrices of gi the step kernel folds
    Step step_fwd, step_bwd; size_t gru_lds;   // (gru_step_fwd_kernel's tiles)
    bool hs_direct;               // T == 1 inference: the new state goes straight to h_final, the heads read it there
    bool stack;                   // EC_RNN_STACK: act step of a multi-layer core, one launch per layer (rnn_stack.hip)
    bool pact;                    // EC_POOLED_ACT: act step of a pooled-embedding handle on pooled_net.hip's two kernels (given h_final != h0)
    bool dw_t, dw1_planes;        // EC_DW_TRANSPOSED; EC_DW1_TR (dc1 then only exists as bf16 planes)
    int bwd3;                     // EC_GEMM_3PRODUCTS or 0 for the backward's large gradient GEMMs
    Ws w;
};

Ws layout(const ec_policy_cfg& c, const Geo& g, Cell cell, int parts, bool bwd, bool pact) {
    const size_t B = g.B, M49 = g.M49, H = g.H, N = g.N, flat = g.flat, E1 = (size_t)c.num_goals * c.comb_hid, G = g.G;
    const bool lstm = cell == Cell::lstm;
    const size_t w1planes = c.fusion ? 0 : ((size_t)c.compress_hid * 3 * c.in_channels + 1) / 2;   // W1 as three bf16 planes
    const size_t wih = (c.fusion && !g.pooled) ? 0 : G * flat;                                   // a re-ordered / dense copy of weight_ih
    Ws w; size_t o = 0;
    auto take = [&](size_t n) { size_t r = o; o += al(n * 4) / 4; return r; };
    auto take_if = [&](bool on, size_t n) { return take(on ? n : 0); };   // an area that is not needed: empty, at the running offset
    for (int i = 0; i < 2; ++i) {
        const bool on = i < g.nstream;
        w.st[i].E1 = take_if(on, E1);
        w.st[i].c1 = take_if(on, M49 * c.compress_hid * parts);   // the act step: room for the split-K partial matrices of c1 (and of gi below)
        w.st[i].c2 = take_if(on, M49 * c.compress_out);
        w.st[i].m1 = take_if(on, M49 * c.comb_hid);
        w.st[i].x4 = take_if(on, M49 * c.comb_out);
    }
    w.x = take(B * flat);
    w.gi = take(B * G * parts);
    w.gh = take(N * G);
    w.gates = take(B * G);
    w.hn = take(B * H); w.hp = take(B * H); w.hs = take(B * H);
    w.goal32 = take(B);
    w.w1p = take(w1planes);
    w.wihA = take_if(!c.dual, wih); w.wihF = take_if(!c.dual && !g.pooled, wih);
    w.w1pF = take(w1planes);
    // what only the learn pass and its backward need
    w.dhs = take_if(bwd, B * H);
    w.dhc = take_if(bwd, N * H);
    w.dgi = take_if(bwd, B * G); w.dghb = take_if(bwd && !lstm, B * G);
    w.dx = take_if(bwd, B * flat);
    w.dx4 = take_if(bwd, M49 * c.comb_out);
    w.dm1 = take_if(bwd, M49 * c.comb_hid);
    w.dc2 = take_if(bwd, M49 * c.compress_out);
    w.dc1 = take_if(bwd, M49 * c.compress_hid * 3 / 2 + 4);   // fp32 [M49][hid], or its three bf16 planes [M49][3][hid]
    w.dE1 = take_if(bwd, E1);
    w.tpart = take_if(bwd && !c.fusion, (size_t)TB_MAX_WG * 4 * TB_PART);              // tail_bwd_kernel's partial sets
    w.tpartE = take_if(bwd && !c.fusion, (size_t)TB_MAX_WG * 4 * c.num_goals * 128);   // ... and its per-wave dE1 tables
    w.whhT = take_if(bwd, H * G);                                                     // W_hh^T (fused backward step)
    w.wihP = take_if(bwd, wih); w.gwihP = take_if(bwd, wih);                              // weight_ih in pixel-major column order (EC_WIH_PERM) and its gradient
    w.tA = take_if(bwd, B * G);                                                       // transposed operands of the GRU's weight-gradient GEMMs
    w.tB = take_if(bwd, B * (flat > H ? flat : H));
    const bool vec = c.goal_in > 0;
    w.E1f = take_if(vec, B * c.comb_hid); w.Eg = take_if(vec, B * c.goal_dims);
    w.gvec = take_if(vec && bwd, B * c.goal_in);
    w.dE1f = take_if(vec && bwd, B * c.comb_hid); w.dEg = take_if(vec && bwd, B * c.goal_dims);
    w.tseg = take_if(vec && bwd, (M49 + 31) / 32 * 256);
    w.gpart = take_if(vec && bwd, (size_t)GP_MAXY * c.comb_hid * c.goal_dims);
    const bool wide = bwd && g.A1 > 8;
    w.hW = take_if(wide, (size_t)g.A1 * H + g.A1); w.hG = take_if(wide, (size_t)g.A1 * H + g.A1);
    w.hP = take_if(wide, (size_t)HP_MAXY * g.A1);
    const bool pa = g.E > 0;
    w.pt = take_if(pa, (size_t)g.R * G);
    w.paidx = take_if(pa && bwd, 2 * B);
    w.pas = take_if(pa && bwd, pa ? ec_pa_grad_scratch_floats((long)B, g.G, g.R) : 0);
    w.cs = take_if(lstm, B * H);
    w.dcc = take_if(lstm && bwd, N * H);
    for (int l = 1; l < EC_RNN_MAX_LAYERS; ++l) {
        const bool on = l < g.L;
        w.ugi[l - 1] = take_if(on, B * G); w.ugates[l - 1] = take_if(on, B * G);
        w.uhn[l - 1] = take_if(on, B * H); w.uhp[l - 1] = take_if(on, B * H); w.uhs[l - 1] = take_if(on, B * H);
        w.ucs[l - 1] = take_if(on && lstm, B * H);
    }
    w.uh0 = take_if(g.L > 1 && !lstm, (size_t)g.L * N * H);
    const bool pl = g.pooled, pids = pl && g.PG > 0, psn = pl && g.PK > 0;
    w.gt = take_if(pids, (size_t)g.PG * G);
    w.sv = take_if(psn, G * (size_t)g.PK); w.sb = take_if(psn, G);
    w.fcF = take_if(pact && !bwd, H * (size_t)g.D);   // (at every T of an inference workspace: its size stays monotone in T)
    w.pgoal = take_if(pids && bwd, 2 * B); w.psens = take_if(psn && bwd, B * (size_t)g.PK);
    w.dsv = take_if(psn && bwd, G * (size_t)g.PK); w.dsb = take_if(psn && bwd, G);
    w.gts = take_if(pids && bwd, pids ? ec_pa_grad_scratch_floats((long)B, g.G, g.PG) : 0);
    const ec_tv_shape tvs{(long)B, g.tvS2, g.tvC, g.H, g.tvA1};
    w.tvw = take_if(g.tv, g.tv ? ec_tv_planes_floats(tvs) : 0);
    w.tva = take_if(g.tv && bwd, B * (size_t)g.tvS2);
    w.tvact = take_if(g.tv && bwd, B * (size_t)g.tvS2 * (H + (size_t)g.tvA1));
    w.tvs = take_if(g.tv && bwd, g.tv ? ec_tv_bwd_scratch_floats(tvs) : 0);
    w.end = o;
    return w;
}

// The one reader of ec_config() in this file, and the one place a path predicate is written.  `mode`: EC_POLICY_LEARN / _INFER /
// _INFER_REUSE; the backward builds the plan of the learn-pass forward whose workspace it reads.
Plan make_plan(const ec_policy* h, int T, int N, int mode, bool feat_bf16) {
    const ec_policy_cfg& c = h->c;
    const EcConfig& cfg = ec_config();
    Plan p;
    Geo& g = p.g;
    g.T = T; g.N = N; g.B = T * N;
    g.S = c.spatial * c.spatial; g.M49 = c.fusion ? 0 : g.B * g.S;
    g.H = c.hidden; g.A = c.num_actions; g.A1 = g.A + 1; g.C = c.in_channels; g.cat = c.compress_out + c.goal_dims;
    g.nstream = (c.dual && !c.fusion) ? 2 : 1; g.flat1 = c.comb_out * g.S; g.flat = c.fusion ? c.in_channels : g.nstream * g.flat1;
    g.pooled = h->pl.on; g.X = h->pl.side(); g.D = h->pl.D; g.PK = h->pl.K; g.PG = h->pl.ids ? c.num_goals : 0;
    g.tv = h->pl.tv; g.tvC = h->pl.tvC; g.tvS2 = h->pl.tvS2; g.tvA1 = h->pl.tvA1;
    g.E = c.prev_action_dims; g.R = c.num_actions + c.prev_action_null; g.pcol = g.flat + g.X; g.ldw = g.pcol + g.E;   // (no route below depends on E)
    p.cell = h->rnn == EC_RNN_LSTM ? Cell::lstm : Cell::gru;
    g.G = (p.cell == Cell::lstm ? 4 : 3) * c.hidden; g.SW = (p.cell == Cell::lstm ? 2 : 1) * c.hidden;
    g.L = h->layers;
    const int B = g.B, S = g.S, M49 = g.M49, H = g.H, C = g.C, flat = g.flat;
    p.infer = mode != EC_POLICY_LEARN; p.feat_bf16 = feat_bf16; p.vec = c.goal_in > 0;
    p.wide = !p.infer && g.A1 > 8;
    p.ordered = p.vec || p.wide || p.cell == Cell::lstm || g.L > 1 || g.pooled;
    p.key = ec_policy::Built{T, N, feat_bf16 ? 1 : 0};
    // Act step: so few rows that the two long-K, small-M GEMMs (compressor conv 1, GRU input projection) run as ACT_PARTS K
    // slices whose partial matrices the consuming kernels fold in a fixed order (no float atomics: rollouts stay bit-reproducible)
    const bool small = M49 > 0 && M49 <= ACT_MAX_ROWS;
    p.act_parts = small ? ACT_PARTS : 1;
    const bool act_on = cfg.act_split && p.infer && small;
    // EC_TAIL_FUSED (default 1): the fused tail kernels are written for the reference's widths
    const bool tail_widths = cfg.tail_fused && !c.fusion && c.compress_hid == 128 && c.compress_out == 32 && c.comb_hid == 128 && c.comb_out == 32;
    p.tail_fwd_lds = ((size_t)2 * 32 * TL_P128 + 128 * TL_P32 + (size_t)c.num_goals * 128 + 64 + 4 * (size_t)(32 * TL_P128 + 32 * TL_P32)) * sizeof(float);
    p.tail_fwd = tail_widths && p.tail_fwd_lds <= LDS_LIMIT && (!p.vec || S >= 32);   // (vec: a tile spans at most two frames; else the GEMM route)
    p.tail_bwd_lds = ((size_t)2 * 128 * TL_P32 + 32 * TL_P128 + std::max<size_t>((size_t)c.num_goals * 128, 4 * 256) +
                      4 * (size_t)(32 * TL_P128 + 32 * TL_P32)) * sizeof(float);   // (the sE area: four wave-private 256-float lines)
    p.tail_bwd = tail_widths && S >= 32 && p.tail_bwd_lds <= LDS_LIMIT && c.num_goals <= TB_MAXG;
    p.goal_direct = p.infer && p.tail_fwd && !p.vec; p.hs_direct = p.infer && T == 1;
    // EC_WIH_PERM: the GRU's input projection reads the combiner output where it lies (pixel-major rows) against a re-ordered weight_ih
    // (permute_row_kernel, one row in LDS), no activation transposes.  Learn pass: per call; act step: by the first call after a parameter
    // update, kept in the workspace like E1
    const bool wih_ok = cfg.wih_perm && !c.fusion && !c.dual && (size_t)c.comb_out * S * 4 <= 64 * 1024;
    p.wih = !wih_ok ? Wih::plain : !p.infer ? Wih::perm_learn : p.tail_fwd ? Wih::perm_act : Wih::plain;
    // Compressor conv 1.  EC_C1_PINGPONG (default 1): bf16 features x fp32 W1 as bf16 planes on the 8-wave ping-pong kernel
    // (conv_igemm8, X3 mode) once there are enough 256-row tiles to fill the chip.  EC_POLICY_FAST: its two leading planes (16
    // mantissa bits) instead of all three, a third fewer MFMAs in a launch that is MFMA-bound; learn pass only (the conv and
    // its weight gradient), the act step stays exact
    const bool c1_split = act_on && p.tail_fwd && (C % 32) == 0 && C / 32 >= ACT_PARTS;
    if (cfg.c1_pingpong && feat_bf16 && c.compress_hid % 128 == 0 && C % 64 == 0 && M49 >= 256 * 128) p.c1 = C1::pingpong;
    else if (c1_split && feat_bf16 && !c.dual && (C % 128) == 0 && (c.compress_hid % 32) == 0) p.c1 = C1::act_kernel;
    else p.c1 = c1_split ? C1::split_parts : C1::plain;
    p.c1_mblk = M49 <= 2048 ? 1 : (M49 <= 4096 ? 2 : 4); p.c1_fold = p.c1 == C1::split_parts ? ACT_PARTS : 1;
    p.planes = (cfg.policy_fast && !p.infer) ? 2 : 3;
    // EC_GRU_FUSED (default 2): one fused launch per step where the geometry allows (forward: H % 32 == 0 and the tiles fit
    // the LDS; backward: H % 256 == 0, T > 1).  The update's recurrences at H == 512 run the 16 x 16-tile kernels, one workgroup
    // per CU with 140 KB of LDS; the act step keeps the 66-KB kernel, which co-resides with the other actor slice's encoder
    p.gru_lds = std::max((size_t)2 * 32 * (((H & 255) == 0 ? 256 : H) + 4) * sizeof(float),      // operand tiles (K chunk) ...
                         (size_t)4 * 32 * 32 * sizeof(float));                                   // ... reused for the 4 partial tiles
    const bool step_ok = cfg.gru_fused && (H % 32) == 0 && p.gru_lds <= LDS_LIMIT;
    const Step fused = (cfg.gru_fused >= 2 && H == 512 && !p.infer) ? Step::fused16 : Step::fused32;
    p.step_fwd = step_ok ? fused : Step::gemm_gates;
    p.step_bwd = (cfg.gru_fused && (H % 256) == 0 && T > 1) ? fused : Step::gemm_gates;
    // an LSTM handle: the 32-tile kernels of lstm.hip at every H (ec_policy_create_rnn admits only widths whose forward tiles fit);
    // EC_GRU_FUSED=0 still selects the gate-plus-GEMM pair for its backward
    if (p.cell == Cell::lstm) {
        p.gru_lds = ec_lstm_fwd_lds(H);
        p.step_fwd = Step::fused32;
        if (p.step_bwd == Step::fused16) p.step_bwd = Step::fused32;
    }
    const bool step_ok_any = step_ok || p.cell == Cell::lstm;
    // a multi-layer core's act step: every layer one launch of the 32-tile geometry (a GRU whose fused step is off: the general route)
    p.stack = g.L > 1 && cfg.rnn_stack && p.infer && T == 1 && p.step_fwd == Step::fused32 && ec_lstm_hidden_ok(H);
    // a pooled-embedding handle's act step: visual_fc on the gi_act geometry (K = D over 7 or 8 waves), then layer 0 in one launch
    // (a two-view handle: its front's launch stands where visual_fc's does)
    const bool pact_any = g.pooled && cfg.pooled_act && ec_lstm_hidden_ok(H) && (g.tv || g.D % 56 == 0 || g.D % 64 == 0);   // (a handle that can take it)
    p.pact = pact_any && p.infer && T == 1;
    // GRU input projection.  Act step with a handful of rows: one launch, K split over the waves of a workgroup and folded
    // in-kernel (gi_act_kernel); else split-K only as separate partial matrices folded by the step kernel
    const int gi_nw = (flat % 56 == 0) ? 7 : ((flat % 64 == 0) ? 8 : 0);
    if (cfg.act_split && p.wih == Wih::perm_act && T == 1 && B <= 256 && gi_nw != 0 && g.G % 32 == 0) p.gi = gi_nw == 7 ? Gi::act7 : Gi::act8;
    else p.gi = (act_on && step_ok_any && (flat + 31) / 32 >= ACT_PARTS) ? Gi::split_parts : Gi::plain;
    p.gi_fold = p.gi == Gi::split_parts ? ACT_PARTS : 1;
    // EC_GEMM_BWD3 / EC_POLICY_FAST: the large gradient GEMMs (weight gradients over all T*N rows, dx = dgi @ W_ih) on the three
    // leading products of the bf16x3 split (relative product error 2^-16; gradients agree with the fp32 oracle to ~1e-5, not ~1e-6)
    p.bwd3 = (cfg.gemm_bwd3 || cfg.policy_fast) ? EC_GEMM_3PRODUCTS : 0;
    // EC_DW_TRANSPOSED (default 1): the GRU's two weight-gradient GEMMs contract over the T*N rows, i.e. BOTH operands are strided in K, the
    // slowest staging of gemm_x3 (1.02 ms for dW_ih at 128 actors, 0.49 ms for the same-size input projection); transposed first (~0.1 ms)
    p.dw_t = cfg.dw_transposed && B >= 1024;
    // EC_DW1_TR (default 1): dW1 through the transpose-read kernel (dw_tn.hip), its partial tiles in the tail's partial sets
    p.dw1_planes = p.tail_bwd && cfg.dw1_tr && feat_bf16 && C % 256 == 0 && M49 >= 2048 &&
                   (size_t)ec_dw_tn_x3_splits(M49, C) * 128 * C <= (size_t)TB_MAX_WG * 4 * TB_PART;
    p.w = layout(c, g, p.cell, p.act_parts, mode == EC_POLICY_LEARN, pact_any);
    return p;
}

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) for a kernel that asks for more than 64 KB: once per device (ec_attr_needed)
template <auto Kernel>
void allow_big_lds() {
    static std::atomic<uint64_t> done{0};
    if (auto guard = ec_attr_needed(done))
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_LIMIT);
}

// One entry-point call: the plan and the caller's buffers.  The stages of the forward (Fwd) and of the backward (Bwd) are
// members: each a linear list of launches that switches on plan fields only.
struct Ctx {
    const ec_policy* h; const ec_policy_cfg& c;
    const Plan& p; const Geo& g; const Ws& w;      // (g, w: the plan's)
    const float* params;
    float* ws;
    ec_stream_t stream; hipStream_t s;             // (one stream, under both of its types)
    Ctx(const ec_policy* h_, const Plan& p_, const float* params_, void* workspace, ec_stream_t stream_)
        : h(h_), c(h_->c), p(p_), g(p_.g), w(p_.w), params(params_), ws((float*)workspace), stream(stream_), s((hipStream_t)stream_) {}
    // stream 1 (the dual encoder's depth stream) has its own compressor / combiner tensors
    size_t off(int i, int sidx = 0) const { return h->off[(sidx && i >= P_W1 && i <= P_B4) ? i + (P_W1D - P_W1) : i]; }
    const float* W(int i, int sidx = 0) const { return params + off(i, sidx); }
    // layer l >= 1's tensor k (0 weight_ih, 1 weight_hh, 2 bias_ih, 3 bias_hh)
    const float* UW(int l, int k) const { return params + h->uoff[l - 1][k]; }
    // what a recurrence (forward or reverse) of ONE layer reads and writes; layer 0's is the single-layer handle's
    struct Layer { const float *whh, *bhh; float *gi, *gates, *hn, *hp, *hs, *cs; int gi_fold; };
    Layer layer(int l) const {
        if (l == 0) return Layer{W(P_WHH), W(P_BHH), ws + w.gi, ws + w.gates, ws + w.hn, ws + w.hp, ws + w.hs, ws + w.cs, p.gi_fold};
        return Layer{UW(l, 1), UW(l, 3), ws + w.ugi[l - 1], ws + w.ugates[l - 1], ws + w.uhn[l - 1], ws + w.uhp[l - 1], ws + w.uhs[l - 1],
                     ws + w.ucs[l - 1], 1};
    }
    float* hs_top() const { return ws + (g.L > 1 ? w.uhs[g.L - 2] : w.hs); }   // the history the heads read
    // the pooled-embedding net: tensor i in front of weight_ih_l0; the sensors' nn.Linear tensors (and, for a backward, their gradients)
    const float* PW(int i) const { return params + h->pl.off[i]; }
    ec_pooled_sensors pooled_sensors(float* grads) const {
        const ec_policy::Pooled& q = h->pl;
        ec_pooled_sensors sn{};
        sn.ns = q.ns; sn.K = q.K; sn.ed = q.ed;
        for (int i = 0; i < q.ns; ++i) {
            sn.k[i] = q.k[i]; sn.w[i] = PW(PL_SW0 + 2 * i); sn.b[i] = PW(PL_SB0 + 2 * i);
            if (grads) { sn.dw[i] = grads + q.off[PL_SW0 + 2 * i]; sn.db[i] = grads + q.off[PL_SB0 + 2 * i]; }
        }
        return sn;
    }
    // ec_gemm_f32 without its extras (row-group bias, ReLU mask, row scale, split-K)
    int gemm(const void* A, const void* B, float* Cp, int M, int N, int K, long sam, long sak, long sbk, long sbn, int ldc, int flags = 0,
             const float* bias = nullptr) const {
        return ec_gemm_f32(A, B, Cp, M, N, K, sam, sak, sbk, sbn, ldc, flags, bias, nullptr, nullptr, 0, nullptr, nullptr, 1, stream);
    }
};

struct Fwd : Ctx {
    using Ctx::Ctx;
    const int* goal_ids = nullptr;   // int32 ids in the workspace, or (goal_direct) the caller's int64 ids
    bool reuse = false;              // EC_POLICY_INFER_REUSE, and this workspace holds the tables of this plan
    const long long* prev = nullptr; // previous actions [B] (handles with a previous-action embedding)
    const float* masks_all = nullptr;

    // weight_ih[:, :flat] where the GEMMs of the routes that keep the parameter's column order read it: the parameter itself, or on a
    // handle with a previous-action embedding (row stride flat + E) its dense copy -- in the learn pass's / the act tables' area
    // of the re-ordered weight, which those routes leave unused
    const float* wih_plain() const { return g.ldw != g.flat ? ws + (p.infer ? w.wihA : w.wihP) : W(P_WIH); }
    // previous-action embedding: the table (with the other weight-derived tables) and, for a backward, the indices
    // (E above PA_TABLE_MAX_E, a two-view handle alone: PT = Emb . W_ih[:, pcol:]^T as one ec_gemm_f32)
    int prev_action_tables() {
        if (!reuse) {
            if (g.E > PA_TABLE_MAX_E) RC(gemm(W(P_PAE), W(P_WIH) + g.pcol, ws + w.pt, g.R, g.G, g.E, g.E, 1, 1, g.ldw, g.G));
            else ec_pa_table_launch(W(P_PAE), W(P_WIH), g.ldw, g.pcol, ws + w.pt, g.R, g.G, g.E, s);
        }
        if (!p.infer) (void)hipMemcpyAsync(ws + w.paidx, prev, (size_t)g.B * 8, hipMemcpyDeviceToDevice, s);
        return EC_OK;
    }

    // ---- the pooled-embedding net (pooled_net.hip's kernels; the tables of prev_action.hip) ----
    ec_pooled_side side{};           // what layer 0's input projection adds per frame (pooled_front fills it)
    bool pact = false;               // this call runs the act route (p.pact and a state row of its own to write)
    float* wih_dense() const { return ws + (p.infer ? w.wihA : w.wihP); }
    // The weight-derived tables (unless reused), the learn pass's copies of the side inputs, v = ReLU(visual_fc(e)) into the `x`
    // area and -- on the general route -- the input projection with the table rows added.  The act route leaves the projection to
    // pooled_step0_kernel.
    int pooled_front(const float* embed, const long long* goal, const float* sens) {
        const ec_policy::Pooled& q = h->pl;
        const int B = g.B, H = g.H, GW = g.G;
        if (!reuse) {
            ec_pa_rows_copy_launch(W(P_WIH), g.ldw, wih_dense(), H, GW, H, 0, s);
            if (q.ids) ec_pa_table_launch(PW(PL_GEMB), W(P_WIH), g.ldw, H, ws + w.gt, g.PG, GW, q.ed, s);
            if (q.ns) ec_pooled_tables_launch(W(P_WIH), g.ldw, H + q.ids * q.ed, pooled_sensors(nullptr), ws + w.sv, ws + w.sb, GW, s);
            if (p.pact) ec_pooled_frag_pack_launch(PW(PL_FCW), ws + w.fcF, H, q.D, s);
        }
        if (g.E) RC(prev_action_tables());
        if (!p.infer) {
            if (q.ids) (void)hipMemcpyAsync(ws + w.pgoal, goal, (size_t)B * 8, hipMemcpyDeviceToDevice, s);
            if (q.ns) (void)hipMemcpyAsync(ws + w.psens, sens, (size_t)B * q.K * 4, hipMemcpyDeviceToDevice, s);
        }
        side = ec_pooled_side{q.ns ? ws + w.sb : nullptr, q.ids ? ws + w.gt : nullptr, goal, g.PG, g.E ? ws + w.pt : nullptr, prev, masks_all,
                              c.prev_action_null, c.num_actions, q.ns ? ws + w.sv : nullptr, sens, q.K};
        if (pact) {
            ec_pooled_fc_act_launch(embed, ws + w.fcF, PW(PL_FCB), ws + w.x, B, q.D, H, s);
            return EC_OK;
        }
        RC(gemm(embed, PW(PL_FCW), ws + w.x, B, H, q.D, q.D, 1, 1, q.D, H, EC_GEMM_RELU, PW(PL_FCB)));
        RC(gemm(ws + w.x, wih_dense(), ws + w.gi, B, GW, H, H, 1, 1, H, GW, 0, W(P_BIH)));
        ec_pooled_rows_add_launch(ws + w.gi, side, (long)B, GW, s);
        return EC_OK;
    }

    // The two-view net's front: the weight-derived tables (unless reused), then v = the attention-pooled encoder of (u, w) into
    // the `x` area -- a learn pass also keeps the probabilities and the post-ReLU activations -- and, on the general route, the
    // input projection with the previous action's table row added
    ec_tv_shape tv_shape() const { return ec_tv_shape{(long)g.B, g.tvS2, g.tvC, g.H, g.tvA1}; }
    int two_view_front(const void* u, const void* v2) {
        const int B = g.B, H = g.H, GW = g.G;
        if (!reuse) {
            ec_pa_rows_copy_launch(W(P_WIH), g.ldw, wih_dense(), H, GW, H, 0, s);
            ec_tv_pack_launch(PW(TV_WE), PW(TV_WA), ws + w.tvw, tv_shape(), s);
        }
        if (g.E) RC(prev_action_tables());
        side = ec_pooled_side{nullptr, nullptr, nullptr, 0, g.E ? ws + w.pt : nullptr, prev, masks_all, c.prev_action_null, c.num_actions,
                              nullptr, nullptr, 0};
        const ec_tv_fwd_args a{(const uint16_t*)u, (const uint16_t*)v2, ws + w.tvw, PW(TV_BE), PW(TV_BA), PW(TV_W2), PW(TV_B2), ws + w.x,
                               p.infer ? nullptr : ws + w.tva, p.infer ? nullptr : ws + w.tvact, (long)B, g.tvS2, g.tvC, H, g.tvA1};
        ec_tv_fwd_launch(a, s);
        if (pact) return EC_OK;
        RC(gemm(ws + w.x, wih_dense(), ws + w.gi, B, GW, H, H, 1, 1, H, GW, 0, W(P_BIH)));
        if (g.E) ec_pooled_rows_add_launch(ws + w.gi, side, (long)B, GW, s);
        return EC_OK;
    }

    // coordinate goals: this call's per-frame bias rows (and, for a backward, the goal vectors and embeddings it will need)
    static size_t goal_vec_lds(const ec_policy_cfg& c, bool bwd) {
        const size_t w3 = (size_t)c.comb_hid * (c.goal_dims + 1);
        return (bwd ? w3 + (size_t)GV_FR * c.comb_hid
                    : w3 + (size_t)c.goal_dims * c.goal_in + c.goal_dims + c.comb_hid + (size_t)GV_FR * c.goal_dims) * sizeof(float);
    }
    int goal_rows(const float* goal_vec) {
        const long nwg = std::min<long>(1024, ((long)g.B + GV_FR - 1) / GV_FR);
        hipLaunchKernelGGL(goal_vec_fwd_kernel, dim3((unsigned)nwg), dim3(256), goal_vec_lds(c, false), s, goal_vec, W(P_EMB), W(P_GB),
                           W(P_W3) + c.compress_out, g.cat, W(P_B3), ws + w.Eg, ws + w.E1f, (long)g.B, c.goal_in, c.goal_dims, c.comb_hid);
        if (!p.infer)
            (void)hipMemcpyAsync(ws + w.gvec, goal_vec, (size_t)g.B * c.goal_in * 4, hipMemcpyDeviceToDevice, s);
        return EC_OK;
    }

    int goal_and_fusion(const void* feat, const int64_t* goal) {
        int* goal32 = (int*)(ws + w.goal32);
        goal_ids = p.goal_direct ? (const int*)goal : goal32;
        if (!p.goal_direct)
            hipLaunchKernelGGL(goal_to_i32_kernel, dim3((g.B + 255) / 256), dim3(256), 0, s, (const long long*)goal, goal32, g.B);
        if (!c.fusion) return EC_OK;
        if (!h->goal_table) return EC_ERR_ARG;
        hipLaunchKernelGGL(p.feat_bf16 ? fuse_goal_kernel<true> : fuse_goal_kernel<false>, dim3((unsigned)((g.B + 3) / 4)), dim3(256), 0, s, feat,
                           h->goal_table, goal32, ws + w.x, (long)g.B, g.flat, c.num_goals);
        return EC_OK;
    }

    template <int MBLK, int U>
    void c1_act(const void* featS, const float* b1, float* c1) {
        hipLaunchKernelGGL((c1_act_kernel<MBLK, U>), dim3((unsigned)(c.compress_hid / 32), (unsigned)((g.M49 + 32 * MBLK - 1) / (32 * MBLK))),
                           dim3(512), 0, s, (const uint16_t*)featS, (const uint16_t*)(ws + w.w1pF), b1, c1, (long)g.M49, g.C, c.compress_hid);
    }

    // resnet_compressor + target_obs_combiner of one encoder stream, up to this stream's block of the GRU input
    int encoder_stream(int sidx, const void* featS) {
        const Ws::Stream& o = w.st[sidx];
        const int M49 = g.M49, C = g.C, cat = g.cat;
        auto WS = [&](int i) { return W(i, sidx); };
        // E1 = embed_class @ W3[:, co:]^T + b3   (coordinate goals: goal_rows() has built E1f, per call)
        if (!reuse && !p.vec)
            RC(gemm(WS(P_EMB), WS(P_W3) + c.compress_out, ws + o.E1, c.num_goals, c.comb_hid, c.goal_dims, c.goal_dims, 1, 1, cat, c.comb_hid, 0, WS(P_B3)));
        if (p.c1 == C1::pingpong) {
            RC(ec_split3_bf16(WS(P_W1), ws + w.w1p, c.compress_hid, C, stream));
            RC(ec_gemm_bf16a_xp(featS, ws + w.w1p, WS(P_B1), ws + o.c1, M49, c.compress_hid, C, 1 /* EC_ACT_RELU */, p.planes, stream));
        } else if (p.c1 == C1::act_kernel) {
            // act step: one launch, K split over the waves of a workgroup, W1's three bf16 planes cached in the workspace with
            // E1; c1 leaves with bias + ReLU (no partial matrices to fold)
            if (!reuse) {
                RC(ec_split3_bf16(WS(P_W1), ws + w.w1p, c.compress_hid, C, stream));
                const long nu = (long)c.compress_hid * 3 * C / 8;
                hipLaunchKernelGGL(frag_pack_planes_kernel, dim3((unsigned)((nu + 255) / 256)), dim3(256), 0, s, (const uint4*)(ws + w.w1p),
                                   (uint4*)(ws + w.w1pF), c.compress_hid, C);
            }
            if (p.c1_mblk == 1) c1_act<1, 8>(featS, WS(P_B1), ws + o.c1);
            else if (p.c1_mblk == 2) c1_act<2, 4>(featS, WS(P_B1), ws + o.c1);
            else c1_act<4, 4>(featS, WS(P_B1), ws + o.c1);
        } else if (p.c1 == C1::split_parts) {
            // act step: K = C is long and M small (196 workgroups walking 64 K-steps each): four K slices write four
            // partial matrices, tail_fwd_kernel folds them (+ b1, ReLU) in a fixed order -- no atomics, bit-reproducible,
            // and independent of how the actors are sliced
            RC(ec_gemm_f32(featS, WS(P_W1), ws + o.c1, M49, c.compress_hid, C, C, 1, 1, C, c.compress_hid,
                           EC_GEMM_SPLIT_PARTS | (p.feat_bf16 ? EC_GEMM_A_BF16 : 0), nullptr, nullptr, nullptr, 0, nullptr, nullptr, ACT_PARTS, stream));
        } else {
            RC(gemm(featS, WS(P_W1), ws + o.c1, M49, c.compress_hid, C, C, 1, 1, C, c.compress_hid, EC_GEMM_RELU | (p.feat_bf16 ? EC_GEMM_A_BF16 : 0), WS(P_B1)));
        }
        if (p.tail_fwd) {
            const long nwg = std::min<long>(512, (((long)M49 + 31) / 32 + 3) / 4);   // 4 tiles of 32 rows per workgroup
            if (p.vec) {
                allow_big_lds<tail_fwd_kernel<true>>();
                hipLaunchKernelGGL(tail_fwd_kernel<true>, dim3((unsigned)nwg), dim3(256), p.tail_fwd_lds, s, ws + o.c1, WS(P_W2), WS(P_B2), WS(P_W3), cat,
                                   ws + w.E1f, (const int*)nullptr, g.S, 0, WS(P_W4), WS(P_B4), ws + o.c2, ws + o.m1, ws + o.x4, (long)M49,
                                   p.c1_fold, (long)M49 * c.compress_hid, WS(P_B1), 1);
            } else {
            allow_big_lds<tail_fwd_kernel<false>>();
            hipLaunchKernelGGL(tail_fwd_kernel<false>, dim3((unsigned)nwg), dim3(256), p.tail_fwd_lds, s, ws + o.c1, WS(P_W2), WS(P_B2), WS(P_W3), cat,
                               ws + o.E1, goal_ids, g.S, c.num_goals, WS(P_W4), WS(P_B4), ws + o.c2, ws + o.m1, ws + o.x4, (long)M49,
                               p.c1_fold, (long)M49 * c.compress_hid, WS(P_B1), p.goal_direct ? 2 : 1);
            }
        } else {
            RC(gemm(ws + o.c1, WS(P_W2), ws + o.c2, M49, c.compress_out, c.compress_hid, c.compress_hid, 1, 1, c.compress_hid, c.compress_out, EC_GEMM_RELU, WS(P_B2)));
            // target_obs_combiner (goal half folded into the row-group bias E1[goal])
            // (coordinate goals: the row group IS the frame -- gidx null selects bias row m / S)
            RC(ec_gemm_f32(ws + o.c2, WS(P_W3), ws + o.m1, M49, c.comb_hid, c.compress_out, c.compress_out, 1, 1, cat,
                           c.comb_hid, EC_GEMM_RELU, nullptr, p.vec ? ws + w.E1f : ws + o.E1, p.vec ? nullptr : goal_ids, g.S, nullptr, nullptr, 1, stream));
            RC(gemm(ws + o.m1, WS(P_W4), ws + o.x4, M49, c.comb_out, c.comb_hid, c.comb_hid, 1, 1, c.comb_hid, c.comb_out, 0, WS(P_B4)));
        }
        if (p.wih == Wih::plain) {
            const long total = (long)g.B * g.flat1;
            hipLaunchKernelGGL(to_cmajor_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, ws + o.x4, ws + w.x,
                               g.S, c.comb_out, total, g.flat, sidx * g.flat1);
            if (g.E && (!p.infer || !reuse))
                ec_pa_rows_copy_launch(W(P_WIH), g.ldw, ws + (p.infer ? w.wihA : w.wihP), g.flat, g.G, g.flat, 0, s);
        } else if (p.wih == Wih::perm_learn || !reuse) {
            hipLaunchKernelGGL(permute_row_kernel, dim3((unsigned)g.G), dim3(256), g.flat * sizeof(float), s, W(P_WIH),
                               ws + (p.wih == Wih::perm_learn ? w.wihP : w.wihA), g.S, c.comb_out, 0, g.ldw);
        }
        return EC_OK;
    }

    // GRU input projection for all T at once
    int input_projection() {
        const int B = g.B, G = g.G, flat = g.flat;
        if (p.gi == Gi::act7 || p.gi == Gi::act8) {
            const float* xin = ws + w.st[0].x4;
            const float* win = ws + w.wihF;                              // the re-ordered weight_ih in fragment order
            if (!reuse) {
                const long nu = (long)G * flat / 4;
                hipLaunchKernelGGL(frag_pack_f32_kernel, dim3((unsigned)((nu + 255) / 256)), dim3(256), 0, s, (const float4*)(ws + w.wihA),
                                   (float4*)(ws + w.wihF), G, flat);
            }
            const int nw = p.gi == Gi::act7 ? 7 : 8;                     // waves of a workgroup
            const dim3 grid((unsigned)(G / 32), (unsigned)((B + 31) / 32));
            if (g.E)      // the previous action's table row rides in the fold (prev_action.hip's instance of the same body): as many launches
                ec_pa_gi_act_launch(nw, xin, win, W(P_BIH), ws + w.gi, B, flat, G,
                                    ec_gi_act_pa{ws + w.pt, prev, masks_all, c.prev_action_null, c.num_actions}, s);
            else
            hipLaunchKernelGGL(nw == 7 ? gi_act_kernel<7> : gi_act_kernel<8>, grid, dim3(64 * nw), 0, s,
                               xin, win, W(P_BIH), ws + w.gi, B, flat, G);
            return EC_OK;
        }
        const float* xin = p.wih == Wih::plain ? ws + w.x : ws + w.st[0].x4;
        const float* win = p.wih == Wih::perm_learn ? ws + w.wihP : (p.wih == Wih::perm_act ? ws + w.wihA : wih_plain());
        RC(ec_gemm_f32(xin, win, ws + w.gi, B, G, flat, flat, 1, 1, flat, G, p.gi == Gi::split_parts ? EC_GEMM_SPLIT_PARTS : 0,
                       W(P_BIH), nullptr, nullptr, 0, nullptr, nullptr, p.gi_fold, stream));
        // the previous action's table row, onto part 0 of a split-K projection (the step kernel folds the parts in order)
        if (g.E) ec_pa_add_launch(ws + w.gi, ws + w.pt, prev, masks_all, c.prev_action_null, c.num_actions, (long)B, G, s);
        return EC_OK;
    }

    // LSTM handle: one lstm.hip launch per step.  h0 and state_out are [N, 2H] rows [h | c]; the histories hs / cs are dense, so
    // step 0 reads pitch 2H and every later step pitch H.  T == 1 inference with a state row of its own: the step stores h
    // densely for the heads AND into the row, c into the row -- the GRU act step's launch count, no copy on the serial chain.
    float* state_out = nullptr;      // the caller's h_final on an LSTM handle (or null)
    Layer lay{};                     // the layer the recurrence() members run (set by the caller)
    // h0 / so: this layer's slice of the state rows (pitch ld_s = L * 2H; one layer: the rows themselves)
    int recurrence_lstm(const float* h0, const float* masks, float* hs, float* so, long ld_s) {
        const int N = g.N, H = g.H, T = g.T;
        float* cs = lay.cs;
        const bool direct = p.hs_direct && so && so != h0;
        const bool keep = !p.infer;      // learn pass: gates and the masked previous states for the backward
        for (int t = 0; t < T; ++t) {
            const size_t o4 = (size_t)t * N * g.G, o1 = (size_t)t * N * H;
            const float* hprev = t == 0 ? h0 : hs + o1 - (size_t)N * H;
            const float* cprev = t == 0 ? h0 + H : cs + o1 - (size_t)N * H;
            ec_lstm_fwd_launch(lay.gi + o4, lay.whh, lay.bhh, hprev, cprev, t == 0 ? ld_s : (long)H, masks + (size_t)t * N, hs + o1, H,
                               direct ? so + H : cs + o1, direct ? ld_s : (long)H, direct ? so : nullptr, ld_s,
                               keep ? lay.gates + o4 : nullptr, keep ? lay.hp + o1 : nullptr, keep ? lay.hn + o1 : nullptr, N, H,
                               lay.gi_fold, (long)g.B * g.G, s);
        }
        if (so && !direct) {
            if (g.L == 1) ec_lstm_state_rows_launch(so, hs + (size_t)(T - 1) * N * H, cs + (size_t)(T - 1) * N * H, N, H, 0, s);
            else {
                ec_pa_rows_copy_launch(hs + (size_t)(T - 1) * N * H, H, so, (int)ld_s, N, H, 0, s);
                ec_pa_rows_copy_launch(cs + (size_t)(T - 1) * N * H, H, so + H, (int)ld_s, N, H, 0, s);
            }
        }
        return EC_OK;
    }

    // the sequential recurrence of layer `lay`; step t's new state goes to hs + t * N * H
    int recurrence(const float* h0, const float* masks, float* hs) {
        const int N = g.N, H = g.H;
        if (p.cell == Cell::lstm) return recurrence_lstm(h0, masks, hs, state_out, 2L * H);
        const size_t gru16_lds = (size_t)(4 * 64 * 128 + 4 * 3 * 256) * sizeof(float);
        if (p.step_fwd == Step::fused32) allow_big_lds<gru_step_fwd_kernel>();
        if (p.step_fwd == Step::fused16) allow_big_lds<gru_step_fwd512_kernel>();
        for (int t = 0; t < g.T; ++t) {
            const float* hprev = (t == 0) ? h0 : hs + (size_t)(t - 1) * N * H;
            const float* m = masks + (size_t)t * N;
            const size_t o3 = (size_t)t * N * 3 * H, o1 = (size_t)t * N * H;
            if (p.step_fwd == Step::fused16) {
                hipLaunchKernelGGL(gru_step_fwd512_kernel, dim3(32u, (unsigned)((N + 15) / 16)), dim3(256), gru16_lds, s,
                                   lay.gi + o3, lay.whh, lay.bhh, hprev, m, hs + o1, lay.gates + o3, lay.hn + o1, lay.hp + o1, N);
            } else if (p.step_fwd == Step::fused32) {
                hipLaunchKernelGGL(gru_step_fwd_kernel, dim3((unsigned)(H / 8), (unsigned)((N + 31) / 32)), dim3(256), p.gru_lds, s,
                                   lay.gi + o3, lay.whh, lay.bhh, hprev, m, hs + o1, lay.gates + o3, lay.hn + o1, lay.hp + o1,
                                   N, H, lay.gi_fold, (long)g.B * 3 * H);
            } else {
                RC(gemm(hprev, lay.whh, ws + w.gh, N, 3 * H, H, H, 1, 1, H, 3 * H));
                hipLaunchKernelGGL(gru_gates_fwd_kernel, dim3((N * H + 255) / 256), dim3(256), 0, s, lay.gi + o3, ws + w.gh,
                                   lay.bhh, hprev, m, hs + o1, lay.gates + o3, lay.hn + o1, lay.hp + o1, N, H);
            }
        }
        return EC_OK;
    }

    // the act step's upper layers, one rnn_stack.hip launch each: layer l reads layer l - 1 out of the new state rows
    void stack_upper_layers(const float* h0, const float* masks, float* h_final) {
        const int L = g.L, N = g.N, H = g.H, SW = g.SW;
        const long ld_s = (long)L * SW;
        const bool lstm = p.cell == Cell::lstm;
        for (int l = 1; l < L; ++l) {
            ec_rnn_stack_args a{};
            a.x = h_final + (size_t)(l - 1) * SW; a.ld_x = ld_s;
            a.wih = UW(l, 0); a.whh = UW(l, 1); a.bih = UW(l, 2); a.bhh = UW(l, 3);
            a.hprev = h0 + (size_t)l * SW; a.cprev = lstm ? a.hprev + H : nullptr; a.ld_prev = ld_s; a.mask = masks;
            a.hout = h_final + (size_t)l * SW; a.ld_h = ld_s; a.cout = lstm ? a.hout + H : nullptr; a.ld_c = ld_s;
            a.hout2 = l == L - 1 ? hs_top() : nullptr; a.ld_h2 = H;
            a.gi_parts = 1; a.N = N; a.H = H;
            ec_rnn_stack_launch(lstm ? 1 : 0, a, s);
        }
    }
    // A pooled-embedding handle's act route: layer 0 in one launch (both projections, the table rows, the cell; states at the row
    // pitch, with one layer also a dense h for the heads), then the upper layers as above
    void pooled_act_recurrence(const float* h0, const float* masks, float* h_final) {
        const int L = g.L, H = g.H;
        const long ld_s = (long)L * g.SW;
        const bool lstm = p.cell == Cell::lstm;
        ec_rnn_stack_args a{};
        a.x = ws + w.x; a.ld_x = H; a.wih = wih_dense(); a.whh = W(P_WHH); a.bih = W(P_BIH); a.bhh = W(P_BHH);
        a.hprev = h0; a.cprev = lstm ? h0 + H : nullptr; a.ld_prev = ld_s; a.mask = masks;
        a.hout = h_final; a.ld_h = ld_s; a.cout = lstm ? h_final + H : nullptr; a.ld_c = ld_s;
        a.hout2 = L == 1 ? ws + w.hs : nullptr; a.ld_h2 = H;
        a.gi_parts = 1; a.N = g.N; a.H = H;
        ec_pooled_step0_launch(lstm ? 1 : 0, a, side, s);
        stack_upper_layers(h0, masks, h_final);
    }

    // A multi-layer core (g.L > 1).  h0 / h_final: [N, L * SW] rows, layer l's state the slice at l * SW.
    //   * act step (p.stack, a state row of its own to write): layer 0's step with both states at the row pitch (an LSTM: lstm.hip's
    //     kernel; a GRU: rnn_stack.hip's with the projection as given), then ONE rnn_stack.hip launch per upper layer, which reads
    //     the layer below out of the new state row; the top layer also stores h densely for the heads.  No copy launch.
    //   * otherwise layer by layer: layer l's whole recurrence with the single-layer step kernels, then one GEMM over all T * N rows
    //     with the bias fused gives layer l + 1's input projection.
    int recurrence_layers(const float* h0, const float* masks, float* h_final) {
        const int L = g.L, N = g.N, H = g.H, T = g.T, B = g.B, SW = g.SW;
        const long ld_s = (long)L * SW;
        const bool lstm = p.cell == Cell::lstm;
        if (p.stack && h_final && h_final != h0) {
            lay = layer(0);
            if (lstm) {
                ec_lstm_fwd_launch(lay.gi, lay.whh, lay.bhh, h0, h0 + H, ld_s, masks, h_final, ld_s, h_final + H, ld_s, nullptr, 0, nullptr,
                                   nullptr, nullptr, N, H, lay.gi_fold, (long)B * g.G, s);
            } else {
                ec_rnn_stack_args a{};
                a.whh = lay.whh; a.bhh = lay.bhh; a.hprev = h0; a.ld_prev = ld_s; a.mask = masks; a.hout = h_final; a.ld_h = ld_s;
                a.gi = lay.gi; a.gi_parts = lay.gi_fold; a.gi_pstride = (long)B * g.G; a.N = N; a.H = H;
                ec_rnn_stack_launch(0, a, s);
            }
            stack_upper_layers(h0, masks, h_final);
            return EC_OK;
        }
        const float* below = nullptr;
        for (int l = 0; l < L; ++l) {
            lay = layer(l);
            if (l) RC(gemm(below, UW(l, 0), lay.gi, B, g.G, H, H, 1, 1, H, g.G, 0, UW(l, 2)));
            if (lstm) {
                RC(recurrence_lstm(h0 + (size_t)l * SW, masks, lay.hs, h_final ? h_final + (size_t)l * SW : nullptr, ld_s));
            } else {
                float* d0 = ws + w.uh0 + (size_t)l * N * H;
                ec_pa_rows_copy_launch(h0 + (size_t)l * H, (int)ld_s, d0, H, N, H, 0, s);
                RC(recurrence(d0, masks, lay.hs));
            }
            below = lay.hs;
        }
        if (!lstm && h_final)
            for (int l = 0; l < L; ++l)
                ec_pa_rows_copy_launch(layer(l).hs + (size_t)(T - 1) * N * H, H, h_final + (size_t)l * H, (int)ld_s, N, H, 0, s);
        return EC_OK;
    }

    // heads: hv[:, :A] = actor logits, hv[:, A] = critic value; then the final state, unless the recurrence left it there
    int heads(const float* hs, float* hv, float* h_final, const SampleArgs& smp, const ForceArgs* wide) {
        const int B = g.B, H = g.H, A = g.A, A1 = g.A1;
        if (A1 <= 8) {
            hipLaunchKernelGGL(heads_fwd_kernel<8>, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, s, hs, W(P_WA), W(P_BA), W(P_WC), W(P_BC), hv, (long)B, H, A, smp);
        } else if (p.wide) {    // learn pass: both heads as one [A + 1, H] table (kept for the backward), one GEMM with the bias fused
            ec_heads_pack_launch(W(P_WA), W(P_BA), W(P_WC), W(P_BC), ws + w.hW, A, H, s);
            RC(gemm(hs, ws + w.hW, hv, B, A1, H, H, 1, 1, H, A1, 0, ws + w.hW + (size_t)A1 * H));
        } else if (wide || g.pooled) {
            // ec_policy_act_ex: heads and selection in one launch (wide_actions.hip), no workspace of its own.  A pooled-embedding
            // handle's inference forward takes the same launch without a selection: a row's logits then do not depend on how the
            // actors are sliced, and the act step equals the forward bit for bit
            const ForceArgs none{};
            const ForceArgs* fa = wide ? wide : &none;
            RC(ec_heads_wide_launch(hs, W(P_WA), W(P_BA), W(P_WC), W(P_BC), hv, (long)B, H, A, smp.actions, smp.logp, smp.values, smp.greedy,
                                    smp.seed, smp.step, smp.first_actor, fa->expert, fa->mask, fa->p, s));
        } else {
            RC(gemm(hs, W(P_WA), hv, B, A, H, H, 1, 1, H, A1, 0, W(P_BA)));
            RC(gemm(hs, W(P_WC), hv + A, B, 1, H, H, 1, 1, H, A1, 0, W(P_BC)));
        }
        if (h_final && hs != h_final)
            (void)hipMemcpyAsync(h_final, ws + w.hs + (size_t)(g.T - 1) * g.N * H, (size_t)g.N * H * 4, hipMemcpyDeviceToDevice, s);
        return EC_OK;
    }
};

// EC_POLICY_INFER_REUSE bookkeeping (ec_policy::Built): is what an earlier EC_POLICY_INFER call left in this workspace valid
// for plan `p`?  Records `p` as the builder when it is not; a learn pass overwrites the workspace and drops the record.
bool tables_reusable(const ec_policy* h, const void* workspace, const Plan& p, int mode) {
    std::lock_guard<std::mutex> lk(h->tables_mu);
    if (!p.infer) { h->tables.erase(workspace); return false; }
    const auto it = h->tables.find(workspace);
    if (mode == EC_POLICY_INFER_REUSE && it != h->tables.end() && it->second == p.key) return true;
    // bounded: a caller that allocates a fresh act workspace per call would otherwise add an entry per allocator address for
    // the life of the handle.  Dropping every record is always safe -- a REUSE call that finds none rebuilds its tables.
    if (h->tables.size() >= 64 && it == h->tables.end()) h->tables.clear();
    h->tables[workspace] = p.key;
    return false;
}

// What one forward or act call is given.  Every exported forward / act function fills one record and hands it on; nothing
// between the C ABI and the stages of Fwd takes these one by one.  A plain aggregate on the caller's stack: no allocation, no lock.
enum class Face { tensor, tensor_pa, pooled, two_view };     // the group of entry points; a handle answers exactly one (face_of)
struct Call {
    Face face = Face::tensor;
    const float* params = nullptr;
    const void *feat = nullptr, *feat2 = nullptr;             // pooled: feat = the embedding rows; two_view: the views u, w
    int feat_bf16 = 0;
    const int64_t* goal = nullptr;
    const float* goal_vec = nullptr;
    const int64_t* prev_actions = nullptr;
    const float *sensors = nullptr, *h0 = nullptr, *masks = nullptr;
    int T = 1, N = 0;
    void* workspace = nullptr;
    size_t ws_bytes = 0;
    int mode = EC_POLICY_INFER;
    float *hv = nullptr, *h_final = nullptr;
    SampleArgs smp{};                   // an act call: the selection; seed / step / first_actor as the caller gave them
    const ForceArgs* force = nullptr;   // the one-call act step of every handle (ec_policy_act_ex and after); nullptr: the narrow entry points
    ec_stream_t stream = nullptr;
};
inline int act_mode(int reuse_tables) { return reuse_tables ? EC_POLICY_INFER_REUSE : EC_POLICY_INFER; }

Face face_of(const ec_policy* h) {
    return h->pl.tv ? Face::two_view : h->pl.on ? Face::pooled : h->c.prev_action_dims > 0 ? Face::tensor_pa : Face::tensor;
}
// more than 7 actions: heads and selection (and forcing) are wide_actions.hip's one launch
bool wide_heads(const ec_policy* h) { return h->c.num_actions + 1 > 8; }

// Every rule by which a forward (and the forward of an act call) is accepted, but the workspace size, which takes the plan.
// One rule per line; the order is the precedence of the codes.
int check_call(const ec_policy* h, const Call& c) {
    if (!h || !c.params || !c.feat || !c.h0 || !c.masks || !c.workspace || !c.hv) return EC_ERR_ARG;
    if (c.face != face_of(h)) return EC_ERR_ARG;              // each kind of handle has entry points of its own
    const bool tensor = c.face == Face::tensor || c.face == Face::tensor_pa, pooled = c.face == Face::pooled, tv = c.face == Face::two_view;
    // a NULL argument matches a part the handle does not have, and the reverse
    if ((c.prev_actions != nullptr) != (h->c.prev_action_dims > 0)) return EC_ERR_ARG;
    if (tensor && (h->c.goal_in > 0 ? (!c.goal_vec || c.goal) : (!c.goal || c.goal_vec))) return EC_ERR_ARG;   // the handle's goal type
    if (tensor && h->c.dual && !c.feat2) return EC_ERR_ARG;
    if (pooled && ((c.goal != nullptr) != (h->pl.ids != 0) || (c.sensors != nullptr) != (h->pl.ns > 0))) return EC_ERR_ARG;
    if (pooled && (c.goal_vec || c.feat2 || c.feat_bf16)) return EC_ERR_ARG;
    if (tv && (!c.feat2 || c.goal || c.goal_vec || c.sensors)) return EC_ERR_ARG;
    if (!tensor && ((uintptr_t)c.feat & 15) != 0) return EC_ERR_ARG;                                           // (read as 16-byte vectors)
    if (tv && ((uintptr_t)c.feat2 & 15) != 0) return EC_ERR_ARG;
    if (c.T <= 0 || c.N <= 0) return EC_ERR_SHAPE;
    if (c.mode < 0 || c.mode > EC_POLICY_INFER_REUSE) return EC_ERR_ARG;
    return EC_OK;
}

// The rules of an act call that come in front of check_call's.  Pinned as they are: without a handle the narrow entry points
// answer EC_ERR_UNSUPPORTED and the others EC_ERR_ARG, and only the others look at first_actor.
int check_act(const ec_policy* h, const Call& c) {
    const SampleArgs& s = c.smp;
    if (!c.force) {      // ec_policy_act, _vec, _greedy, _vec_greedy: plain tensor handles, the one-wave-per-row heads launch
        if (!s.actions || !s.logp || (h && face_of(h) != Face::tensor)) return EC_ERR_ARG;
        if (!h || wide_heads(h)) return EC_ERR_UNSUPPORTED;
        return EC_OK;
    }
    const ForceArgs& f = *c.force;
    if (!h || !s.actions || !s.logp) return EC_ERR_ARG;
    if (c.face != face_of(h)) return EC_ERR_ARG;
    if (c.face == Face::tensor_pa && !c.prev_actions) return EC_ERR_ARG;
    if ((f.expert != nullptr) != (f.mask != nullptr)) return EC_ERR_ARG;
    if (!(f.p >= 0.f && f.p <= 1.f)) return EC_ERR_ARG;       // (NaN included)
    if (!f.expert && f.p != 0.f) return EC_ERR_ARG;
    if (f.expert && s.greedy) return EC_ERR_ARG;              // forcing belongs to the sampling act step
    if (h->c.num_actions > 256) return EC_ERR_UNSUPPORTED;
    if (s.first_actor < 0) return EC_ERR_SHAPE;
    return EC_OK;
}

int policy_forward_impl(const ec_policy_t* h, const Call& c) {
    RC(check_call(h, c));
    const Plan p = make_plan(h, c.T, c.N, c.mode, c.feat_bf16 != 0);
    if (c.ws_bytes < p.w.end * 4) return EC_ERR_WORKSPACE;
    const ForceArgs* wide = (c.force && wide_heads(h)) ? c.force : nullptr;
    const float *h0 = c.h0, *masks = c.masks;
    float *hv = c.hv, *h_final = c.h_final;
    Fwd f(h, p, c.params, c.workspace, c.stream);
    f.reuse = tables_reusable(h, c.workspace, p, c.mode);
    f.prev = (const long long*)c.prev_actions; f.masks_all = masks;
    if (h->pl.on) {
        f.pact = p.pact && h_final && h_final != h0;
        if (h->pl.tv) RC(f.two_view_front(c.feat, c.feat2));
        else RC(f.pooled_front((const float*)c.feat, (const long long*)c.goal, c.sensors));
        if (f.pact) {
            f.pooled_act_recurrence(h0, masks, h_final);
            RC(f.heads(f.hs_top(), hv, nullptr, c.smp, wide));
            EC_CHECK_LAUNCH();
            return EC_OK;
        }
    } else {
        if (p.vec) RC(f.goal_rows(c.goal_vec));
        else RC(f.goal_and_fusion(c.feat, c.goal));
        if (!h->c.fusion)
            for (int sidx = 0; sidx < p.g.nstream; ++sidx)   // dual encoder: the RGB stream, then the depth stream (own weights, own activations)
                RC(f.encoder_stream(sidx, sidx ? c.feat2 : c.feat));
        if (p.g.E) RC(f.prev_action_tables());
        RC(f.input_projection());
    }
    const bool lstm = p.cell == Cell::lstm;   // (the heads read the dense history; recurrence_lstm leaves the [h | c] rows in h_final)
    float* hs = (!lstm && p.hs_direct && h_final && h_final != h0) ? h_final : f.ws + p.w.hs;
    if (p.g.L > 1) {       // a multi-layer core leaves every layer's state in h_final itself; the heads read the top layer's history
        hs = f.hs_top();
        RC(f.recurrence_layers(h0, masks, h_final));
        RC(f.heads(hs, hv, nullptr, c.smp, wide));
        EC_CHECK_LAUNCH();
        return EC_OK;
    }
    if (lstm) f.state_out = h_final;
    f.lay = f.layer(0);
    RC(f.recurrence(h0, masks, hs));
    RC(f.heads(hs, hv, lstm ? nullptr : h_final, c.smp, wide));
    EC_CHECK_LAUNCH();
    return EC_OK;
}

// An act call: the T = 1 inference forward whose heads launch selects.  More than 7 actions: the stages in front as they are,
// then the wide heads launch with the selection (and the forcing) in it; up to 7: the one-wave-per-row heads launch, then
// ec_teacher_force's.
int policy_act(const ec_policy_t* h, Call c) {
    RC(check_act(h, c));
    if (c.smp.greedy) { c.smp.seed = 0; c.smp.step = 0; c.smp.first_actor = 0; }     // (the mode does not read them)
    RC(policy_forward_impl(h, c));
    if (!c.force || !c.force->expert || wide_heads(h)) return EC_OK;
    return ec_teacher_force(c.hv, (const int64_t*)c.force->expert, c.force->mask, c.force->p, (int64_t*)c.smp.actions, c.smp.logp, c.N,
                            h->c.num_actions, c.smp.seed, c.smp.step, c.smp.first_actor, c.stream);
}

struct Bwd : Ctx {
    using Ctx::Ctx;
    float* grads = nullptr;
    const float* masks_all = nullptr;   // (previous-action embedding: the null token's selector)
    bool parts_ok = true;         // the dx area is free for partial matrices (cleared once dx occupies it)
    float* G(int i, int sidx = 0) const { return grads + off(i, sidx); }

    // column sums (bias gradients) without atomics: row block y leaves its sums in cpart[y][Ncol] (the forward's per-step `gh`
    // scratch: N x 3H floats, idle in the backward), colsum_fold_kernel adds the row blocks in order onto the gradient
    void colsum(const float* Y, float* out, long M, int Ncol, int ld, float* cpart = nullptr, size_t cpart_cap = 0) {
        if (!cpart) { cpart = ws + w.gh; cpart_cap = (size_t)g.N * g.G; }
        const bool wide = (Ncol & 3) == 0 && (ld & 3) == 0 && Ncol >= 256 && M >= 1024;
        long nby = (M + (wide ? 255 : 2047)) / (wide ? 256 : 2048);
        const long fit = (long)(cpart_cap / (size_t)Ncol);
        nby = std::max<long>(1, std::min(nby, fit));            // (Ncol <= 3H always: at least one row block fits)
        const int rpb = (int)(((M + nby - 1) / nby + 3) / 4 * 4);
        nby = (M + rpb - 1) / rpb;
        if (wide) hipLaunchKernelGGL(colsum4_kernel, dim3((unsigned)((Ncol + 255) / 256), (unsigned)nby), dim3(256), 0, s, Y, cpart, M, Ncol, ld, rpb);
        else hipLaunchKernelGGL(colsum_kernel, dim3((unsigned)((Ncol + 63) / 64), (unsigned)nby), dim3(256), 0, s, Y, cpart, M, Ncol, ld, rpb);
        hipLaunchKernelGGL(colsum_fold_kernel, dim3((unsigned)((Ncol + 255) / 256)), dim3(256), 0, s, cpart, (int)nby, Ncol, out);
    }
    // weight-gradient GEMMs that split K: every K slice writes its own partial matrix (EC_GEMM_SPLIT_PARTS) into `sparts` and
    // splitk_fold_kernel adds the slices in order onto the gradient -- the fp32 atomics this replaces made two runs from one
    // seed differ in the last bits.  sparts: the dx area (free until dx / dx4 is computed, behind the weight gradients; with
    // the re-ordered weight_ih and in fusion mode it is never used at all).
    int gemm_acc_split(const void* A_, const void* B_, float* dW, int Mo, int No, long K, long sam, long sak, long sbk, long sbn,
                       int ldc, int flags, int sk) {
        float* sparts = ws + w.dx;
        const size_t sparts_cap = (size_t)g.B * g.flat;
        // every K slice costs a partial matrix written and read back: no more slices than fill the chip twice with 128 x 128 tiles
        const long tiles_ = (long)((Mo + 127) / 128) * ((No + 127) / 128);
        const int sk_cap = (int)std::max<long>(2, 512 / (tiles_ > 0 ? tiles_ : 1));
        if (sk > sk_cap) sk = sk_cap;
        while (sk > 1 && (size_t)sk * Mo * No > sparts_cap) --sk;
        if (sk <= 1) return gemm(A_, B_, dW, Mo, No, (int)K, sam, sak, sbk, sbn, ldc, EC_GEMM_ACCUMULATE | flags);
        RC(ec_gemm_f32(A_, B_, sparts, Mo, No, (int)K, sam, sak, sbk, sbn, No, EC_GEMM_SPLIT_PARTS | flags, nullptr, nullptr, nullptr, 0, nullptr, nullptr, sk, stream));
        const long nq = (long)Mo * No;
        hipLaunchKernelGGL(splitk_fold_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, s, sparts, sk, Mo, No, ldc, dW);
        return EC_OK;
    }
    // dW += dY^T X over K rows: K slices into partial matrices folded in order while the dx area is free (`parts_ok`); the
    // tail's unfused fallback GEMMs (EC_TAIL_FUSED=0, the dual encoder) run after dx exists and keep the atomic split
    int tn(const float* dY, int ldy, const void* X, int ldx, int x_bf16, float* dW, int Mo, int No, long K, int ldc) {
        // (coordinate goals, wide handles: no float atomics on any route -- without the partial-matrix area the GEMM walks K in one piece)
        const int sk = (p.ordered && !parts_ok) ? 1 : pick_splitk(Mo, No, K), flags = (x_bf16 ? EC_GEMM_B_BF16 : 0) | p.bwd3;
        if (parts_ok) return gemm_acc_split(dY, X, dW, Mo, No, K, 1, ldy, ldx, 1, ldc, flags, sk);
        return ec_gemm_f32(dY, X, dW, Mo, No, (int)K, 1, ldy, ldx, 1, ldc, EC_GEMM_ACCUMULATE | flags, nullptr, nullptr, nullptr, 0, nullptr,
                           nullptr, sk, stream);
    }
    // the same for the GRU's two weight gradients (ld(dY) == Mo, ld(X) == ld(dW) == No): on transposed operands if the plan says so
    int tn_gru(const float* dY, const float* X, float* dW, int Mo, int No, long K) {
        if (!p.dw_t) return tn(dY, Mo, X, No, 0, dW, Mo, No, K, No);
        hipLaunchKernelGGL(transpose_f32_kernel, dim3((unsigned)((Mo + 31) / 32), (unsigned)((K + 31) / 32)), dim3(256), 0, s, dY,
                           ws + w.tA, (int)K, Mo);
        hipLaunchKernelGGL(transpose_f32_kernel, dim3((unsigned)((No + 31) / 32), (unsigned)((K + 31) / 32)), dim3(256), 0, s, X,
                           ws + w.tB, (int)K, No);
        return gemm_acc_split(ws + w.tA, ws + w.tB, dW, Mo, No, K, K, 1, 1, K, No, p.bwd3, pick_splitk(Mo, No, K));
    }

    int heads(const float* dhv) {
        const int B = g.B, H = g.H, A = g.A, A1 = g.A1;
        if (p.wide) {
            // on the forward's packed table: dhs = dhv [B, A+1] x tab [A+1, H]; the table's gradient dhv^T hs by K slices folded
            // in order and its bias row by ordered column sums, both onto a zeroed copy; one launch adds that to the four tensors
            float* gt = ws + w.hG;
            RC(gemm(dhv, ws + w.hW, ws + w.dhs, B, H, A1, A1, 1, H, 1, H));
            (void)hipMemsetAsync(gt, 0, ((size_t)A1 * H + A1) * 4, s);
            RC(gemm_acc_split(dhv, hs_top(), gt, A1, H, B, 1, A1, H, 1, H, 0, pick_splitk(A1, H, B)));
            colsum(dhv, gt + (size_t)A1 * H, B, A1, A1, ws + w.hP, (size_t)HP_MAXY * A1);
            ec_heads_unpack_add_launch(gt, G(P_WA), G(P_BA), G(P_WC), G(P_BC), A, H, s);
            return EC_OK;
        }
        RC(gemm(dhv, W(P_WA), ws + w.dhs, B, H, A, A1, 1, H, 1, H));
        RC(gemm(dhv + A, W(P_WC), ws + w.dhs, B, H, 1, A1, 1, H, 1, H, EC_GEMM_ACCUMULATE));
        RC(gemm_acc_split(dhv, hs_top(), G(P_WA), A, H, B, 1, A1, H, 1, H, 0, pick_splitk(A, H, B)));
        RC(gemm_acc_split(dhv + A, hs_top(), G(P_WC), 1, H, B, 1, A1, H, 1, H, 0, pick_splitk(1, H, B)));
        colsum(dhv, G(P_BA), B, A, A1);
        colsum(dhv + A, G(P_BC), B, 1, A1);
        return EC_OK;
    }

    Layer lay{};                  // the layer the recurrence() members run (set by the caller)
    int lidx = 0;                 // ... and its index: dh_final's slice at lidx * SW starts its carries
    // LSTM, reverse time (lstm.hip).  dh_final is [N, 2H] rows [dh | dc]: its halves start the two carries.  Fused: step T-1 is
    // the plain gate kernel, every earlier step ONE launch (back-projection of step t+1 + gates of step t, against a W_hh
    // transposed once); else gate kernel + GEMM per step with split-K 1.  No float atomics on either route.
    int recurrence_lstm(const float* masks, const float* dh_final) {
        const int T = g.T, N = g.N, H = g.H, GW = g.G;
        float* da = ws + w.dgi;
        if (dh_final && g.L > 1) {
            const float* row = dh_final + (size_t)lidx * g.SW;
            ec_pa_rows_copy_launch(row, g.L * g.SW, ws + w.dhc, H, N, H, 0, s);
            ec_pa_rows_copy_launch(row + H, g.L * g.SW, ws + w.dcc, H, N, H, 0, s);
        } else if (dh_final) ec_lstm_state_rows_launch(const_cast<float*>(dh_final), ws + w.dhc, ws + w.dcc, N, H, 1, s);
        else {
            (void)hipMemsetAsync(ws + w.dhc, 0, (size_t)N * H * 4, s);
            (void)hipMemsetAsync(ws + w.dcc, 0, (size_t)N * H * 4, s);
        }
        const bool fused = p.step_bwd != Step::gemm_gates;
        if (fused)
            hipLaunchKernelGGL(transpose_f32_kernel, dim3((unsigned)(H / 32), (unsigned)(GW / 32)), dim3(256), 0, s, lay.whh, ws + w.whhT, GW, H);
        for (int t = T - 1; t >= 0; --t) {
            const size_t o4 = (size_t)t * N * GW, o1 = (size_t)t * N * H;
            const float* m = masks + (size_t)t * N;
            if (!fused || t == T - 1) {
                ec_lstm_bwd_gates_launch(ws + w.dhs + o1, ws + w.dhc, ws + w.dcc, lay.gates + o4, lay.cs + o1, lay.hn + o1, m, da + o4,
                                         N, H, s);
                // dh_carry (left zero by the gate kernel) += m * (da @ W_hh)   (fused: inside the next launch)
                if (!fused)
                    RC(ec_gemm_f32(da + o4, lay.whh, ws + w.dhc, N, H, GW, GW, 1, H, 1, H, EC_GEMM_ACCUMULATE, nullptr, nullptr, nullptr, 0,
                                   nullptr, m, 1, stream));
            } else {
                ec_lstm_bwd_fused_launch(da + o4 + (size_t)N * GW, ws + w.whhT, m + N, ws + w.dhs + o1, ws + w.dcc, lay.gates + o4,
                                         lay.cs + o1, lay.hn + o1, m, da + o4, N, H, s);
            }
        }
        return EC_OK;
    }

    // GRU, reverse time.  Fused: step T-1 is the plain gate kernel (its carry is dh_final), every earlier step ONE fused launch
    // (back-projection of step t+1 + gates of step t); else gate kernel + GEMM per step
    int recurrence(const float* masks, const float* dh_final) {
        const int T = g.T, N = g.N, H = g.H;
        if (p.cell == Cell::lstm) return recurrence_lstm(masks, dh_final);
        const size_t gb_lds = (size_t)2 * 32 * (256 + 4) * sizeof(float), gb16_lds = (size_t)(4 * 2 * 32 * 128 + 4 * 256) * sizeof(float);
        if (dh_final && g.L > 1) ec_pa_rows_copy_launch(dh_final + (size_t)lidx * H, g.L * H, ws + w.dhc, H, N, H, 0, s);
        else if (dh_final) (void)hipMemcpyAsync(ws + w.dhc, dh_final, (size_t)N * H * 4, hipMemcpyDeviceToDevice, s);
        else (void)hipMemsetAsync(ws + w.dhc, 0, (size_t)N * H * 4, s);
        if (p.step_bwd != Step::gemm_gates)
            hipLaunchKernelGGL(transpose_f32_kernel, dim3((unsigned)(H / 32), (unsigned)(3 * H / 32)), dim3(256), 0, s, lay.whh, ws + w.whhT, 3 * H, H);
        if (p.step_bwd == Step::fused32) allow_big_lds<gru_step_bwd_kernel>();
        if (p.step_bwd == Step::fused16) allow_big_lds<gru_step_bwd512_kernel>();
        for (int t = T - 1; t >= 0; --t) {
            const size_t o3 = (size_t)t * N * 3 * H, o1 = (size_t)t * N * H;
            const float* m = masks + (size_t)t * N;
            if (p.step_bwd == Step::gemm_gates || t == T - 1) {
                hipLaunchKernelGGL(gru_gates_bwd_kernel, dim3((N * H + 255) / 256), dim3(256), 0, s, ws + w.dhs + o1, ws + w.dhc,
                                   lay.gates + o3, lay.hn + o1, lay.hp + o1, m, ws + w.dgi + o3, ws + w.dghb + o3, N, H);
                // dh_carry += m * (dghb @ W_hh)   (fused: step T-1's back-projection runs inside the next launch)
                if (p.step_bwd == Step::gemm_gates)
                    RC(ec_gemm_f32(ws + w.dghb + o3, lay.whh, ws + w.dhc, N, H, 3 * H, 3 * H, 1, H, 1, H, EC_GEMM_ACCUMULATE, nullptr,
                                   nullptr, nullptr, 0, nullptr, m, p.ordered ? 1 : step_splitk(N, H, 3 * H), stream));
            } else if (p.step_bwd == Step::fused16) {
                hipLaunchKernelGGL(gru_step_bwd512_kernel, dim3(32u, (unsigned)((N + 15) / 16)), dim3(256), gb16_lds, s,
                                   ws + w.dghb + o3 + (size_t)N * 3 * H, ws + w.whhT, m + N, ws + w.dhs + o1, ws + w.dhc,
                                   lay.gates + o3, lay.hn + o1, lay.hp + o1, m, ws + w.dgi + o3, ws + w.dghb + o3, N);
            } else {
                hipLaunchKernelGGL(gru_step_bwd_kernel, dim3((unsigned)(H / 32), (unsigned)((N + 31) / 32)), dim3(256), gb_lds, s,
                                   ws + w.dghb + o3 + (size_t)N * 3 * H, ws + w.whhT, m + N, ws + w.dhs + o1, ws + w.dhc,
                                   lay.gates + o3, lay.hn + o1, lay.hp + o1, m, ws + w.dgi + o3, ws + w.dghb + o3, N, H);
            }
        }
        return EC_OK;
    }

    // Layer l >= 1 of a multi-layer core, behind its reverse recurrence: its four gradients (the input history is the layer below's
    // state history), then dx = da W_ih over all T * N rows INTO the dhs area -- the reverse recurrence of layer l - 1 reads it as
    // the heads' dhs was read at the top.  GEMMs in one K piece or K slices folded in order, ordered column sums: no float atomics.
    int upper_layer_grads(int l) {
        const int B = g.B, H = g.H, GW = g.G;
        const float* dghb = ws + (p.cell == Cell::lstm ? w.dgi : w.dghb);
        float* gu = grads;
        RC(tn_gru(dghb, lay.hp, gu + h->uoff[l - 1][1], GW, H, B));
        colsum(dghb, gu + h->uoff[l - 1][3], B, GW, GW);
        RC(tn_gru(ws + w.dgi, layer(l - 1).hs, gu + h->uoff[l - 1][0], GW, H, B));
        colsum(ws + w.dgi, gu + h->uoff[l - 1][2], B, GW, GW);
        return gemm(ws + w.dgi, UW(l, 0), ws + w.dhs, B, H, GW, GW, 1, H, 1, H);
    }

    // weight and bias gradients of the recurrence and of the input projection (TN over all T*N rows)
    // (an LSTM handle's one gate gradient da lies in the dgi area and serves as both)
    int gru_grads() {
        const int B = g.B, H = g.H, flat = g.flat, GW = g.G;
        const float* dghb = ws + (p.cell == Cell::lstm ? w.dgi : w.dghb);
        RC(tn_gru(dghb, ws + w.hp, G(P_WHH), GW, H, B));
        colsum(dghb, G(P_BHH), B, GW, GW);
        if (p.wih == Wih::perm_learn) {   // gradient in the re-ordered weight's column order, then added back in the parameter's order
            (void)hipMemsetAsync(ws + w.gwihP, 0, (size_t)GW * flat * 4, s);
            RC(tn_gru(ws + w.dgi, ws + w.st[0].x4, ws + w.gwihP, GW, flat, B));
            hipLaunchKernelGGL(permute_row_kernel, dim3((unsigned)(GW)), dim3(256), flat * sizeof(float), s, ws + w.gwihP,
                               G(P_WIH), g.S, c.comb_out, 1, g.ldw);
        } else if (g.ldw != flat) {       // the dense gradient, then added back onto the parameter's rows (stride flat + E; the pooled net's: flat + X + E)
            (void)hipMemsetAsync(ws + w.gwihP, 0, (size_t)GW * flat * 4, s);
            RC(tn_gru(ws + w.dgi, ws + w.x, ws + w.gwihP, GW, flat, B));
            ec_pa_rows_copy_launch(ws + w.gwihP, flat, G(P_WIH), g.ldw, GW, flat, 1, s);
        } else {
            RC(tn_gru(ws + w.dgi, ws + w.x, G(P_WIH), GW, flat, B));
        }
        colsum(ws + w.dgi, G(P_BIH), B, GW, GW);
        // previous-action embedding: its gradient and columns flat.. of weight_ih's (inside the recurrent section: before the event)
        if (g.E > PA_TABLE_MAX_E) {
            // (a two-view handle alone) the same binned ordered sum over frames -- it does not depend on E -- leaves dPT [R, G] in front
            // of the scratch; dEmb += dPT Wa and dWa += dPT^T Emb on ec_gemm_f32, the second through the transpose-read routine
            ec_pa_bins_launch(ws + w.dgi, (const long long*)(ws + w.paidx), masks_all, c.prev_action_null, c.num_actions, ws + w.pas, (long)B,
                              GW, s);
            RC(gemm(ws + w.pas, W(P_WIH) + g.pcol, G(P_PAE), g.R, g.E, GW, GW, 1, g.ldw, 1, g.E, EC_GEMM_ACCUMULATE | p.bwd3));
            RC(tn(ws + w.pas, GW, W(P_PAE), g.E, 0, G(P_WIH) + g.pcol, GW, g.E, g.R, g.ldw));
        } else if (g.E) {
            ec_pa_grad_launch(ws + w.dgi, (const long long*)(ws + w.paidx), masks_all, c.prev_action_null, c.num_actions, W(P_PAE), W(P_WIH),
                              g.ldw, g.pcol, G(P_PAE), G(P_WIH), ws + w.pas, (long)B, GW, g.E, s);
        }
        return EC_OK;
    }

    // ---- the pooled-embedding net ----
    // From layer 0's dgi: the goal-id table's gradient as prev_action.hip's binned ordered sum (the same problem with no null row and
    // no mask), chained to the embedding and to its columns of weight_ih; dSV = dgi^T s by K slices folded in order and dsb = the
    // ordered column sum, chained by pooled_net.hip's two launches to the sensors' columns of weight_ih and to W_i, b_i.  Everything
    // that lands inside weight_ih's gradient is done here, before the recurrent section is declared final.
    int pooled_side_grads() {
        const ec_policy::Pooled& q = h->pl;
        const int B = g.B, GW = g.G;
        if (q.ids)
            ec_pa_grad_launch(ws + w.dgi, (const long long*)(ws + w.pgoal), nullptr, 0, g.PG, PW(PL_GEMB), W(P_WIH), g.ldw, g.flat,
                              grads + q.off[PL_GEMB], G(P_WIH), ws + w.gts, (long)B, GW, q.ed, s);
        if (q.ns) {
            (void)hipMemsetAsync(ws + w.dsv, 0, (size_t)GW * q.K * 4, s);
            (void)hipMemsetAsync(ws + w.dsb, 0, (size_t)GW * 4, s);
            RC(tn(ws + w.dgi, GW, ws + w.psens, q.K, 0, ws + w.dsv, GW, q.K, B, q.K));
            colsum(ws + w.dgi, ws + w.dsb, B, GW, GW);
            ec_pooled_sensor_grads_launch(W(P_WIH), G(P_WIH), g.ldw, g.flat + q.ids * q.ed, pooled_sensors(grads), ws + w.dsv, ws + w.dsb, GW, s);
        }
        return EC_OK;
    }
    // dv = (dgi W_ih[:, :H]) where v > 0 (the forward's dense copy; v is the `x` area), then visual_fc's two gradients over the
    // embedding rows.  dv occupies the partial-matrix area: the weight gradient walks K in one piece (no float atomics).
    int pooled_fc_grads(const float* embed) {
        const ec_policy::Pooled& q = h->pl;
        const int B = g.B, H = g.H, GW = g.G;
        RC(ec_gemm_f32(ws + w.dgi, ws + w.wihP, ws + w.dx, B, H, GW, GW, 1, H, 1, H, p.bwd3, nullptr, nullptr, nullptr, 0, ws + w.x, nullptr, 1,
                       stream));
        parts_ok = false;
        RC(tn(ws + w.dx, H, embed, q.D, 0, grads + q.off[PL_FCW], H, q.D, B, q.D));
        colsum(ws + w.dx, grads + q.off[PL_FCB], B, H, H);
        return EC_OK;
    }

    // The two-view net: dv = dgi W_ih[:, :H] with no mask (v is not rectified after pooling), then the front's six gradients from the
    // probabilities and activations the forward kept (two_view.hip: ordered sums only)
    int two_view_grads(const void* u, const void* v2) {
        const ec_policy::Pooled& q = h->pl;
        const int B = g.B, H = g.H, GW = g.G;
        RC(ec_gemm_f32(ws + w.dgi, ws + w.wihP, ws + w.dx, B, H, GW, GW, 1, H, 1, H, p.bwd3, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 1,
                       stream));
        parts_ok = false;
        ec_tv_bwd_launch(u, v2, PW(TV_W2), ws + w.dx, ws + w.tva, ws + w.tvact, ws + w.tvs, grads + q.off[TV_WE], grads + q.off[TV_BE],
                         grads + q.off[TV_WA], grads + q.off[TV_BA], grads + q.off[TV_W2], grads + q.off[TV_B2],
                         ec_tv_shape{(long)B, g.tvS2, g.tvC, H, g.tvA1}, s);
        return EC_OK;
    }

    // dx = dgi @ W_ih (channel-major), or dx4 = dgi @ (re-ordered weight_ih): already pixel-major
    int input_grad() {
        const int B = g.B, flat = g.flat, GW = g.G;
        if (p.wih != Wih::perm_learn)
            return gemm(ws + w.dgi, g.E ? ws + w.wihP : W(P_WIH), ws + w.dx, B, flat, GW, GW, 1, flat, 1, flat, p.bwd3);   // (E: the forward's dense copy)
        // The weight is transposed first (9.6 MB, into the gradient staging buffer, free again by now) so that BOTH operands are
        // K-contiguous: the GEMM's strided-B staging runs at half the rate (263 vs ~130 us at 32 actors, 770 vs ~540 at 128)
        // (both grid dimensions rounded up: 3H is no multiple of 32 where H is none, the gate + GEMM route; the kernel guards the edges)
        hipLaunchKernelGGL(transpose_f32_kernel, dim3((unsigned)((flat + 31) / 32), (unsigned)((GW + 31) / 32)), dim3(256), 0, s,
                           ws + w.wihP, ws + w.gwihP, GW, flat);
        return gemm(ws + w.dgi, ws + w.gwihP, ws + w.dx4, B, flat, GW, GW, 1, 1, GW, flat, p.bwd3);
    }

    // goal half of target_obs_combiner.0 (dE1 = row-group sums of dm1 scattered by goal id)
    int goal_half(int sidx) {
        float* dE1 = ws + w.dE1;
        colsum(dE1, G(P_B3, sidx), c.num_goals, c.comb_hid, c.comb_hid);
        RC(tn(dE1, c.comb_hid, W(P_EMB, sidx), c.goal_dims, 0, G(P_W3, sidx) + c.compress_out, c.comb_hid, c.goal_dims, c.num_goals, g.cat));
        return gemm(dE1, W(P_W3, sidx) + c.compress_out, G(P_EMB, sidx), c.num_goals, c.goal_dims, c.comb_hid, c.comb_hid, 1, g.cat, 1, c.goal_dims,
                    EC_GEMM_ACCUMULATE);
    }

    // dW[m*ldc + n] += sum_b A[b][m] X[b][n] for the goal half's small weight gradients: row blocks, folded in order
    void tn_small(const float* A_, int Mo, const float* X, int No, float* dW, int ldc) {
        const long K = g.B;
        const int rpb = (int)std::max<long>(32, ((K + GP_MAXY - 1) / GP_MAXY + 31) / 32 * 32);
        const int ny = (int)((K + rpb - 1) / rpb);
        hipLaunchKernelGGL(tn_small_part_kernel, dim3((unsigned)ny), dim3(256), (size_t)32 * (Mo + No) * sizeof(float), s, A_, Mo, X, No,
                           ws + w.gpart, Mo, No, K, rpb);
        const long nq = (long)Mo * No;
        hipLaunchKernelGGL(splitk_fold_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, s, ws + w.gpart, ny, Mo, No, ldc, dW);
    }
    // goal half with coordinate goals, from dE1f [B, comb_hid] (the per-frame sums of dm1):
    //   db3 += colsum dE1f;  dW3[:, co:] += dE1f^T Eg;  dEg = dE1f W3[:, co:];  dWc += dEg^T goal_vec;  dbc += colsum dEg
    int goal_half_vec() {
        const float* dE1f = ws + w.dE1f;
        colsum(dE1f, G(P_B3), g.B, c.comb_hid, c.comb_hid);
        tn_small(dE1f, c.comb_hid, ws + w.Eg, c.goal_dims, G(P_W3) + c.compress_out, g.cat);
        const long nwg = std::min<long>(1024, ((long)g.B + GV_FR - 1) / GV_FR);
        hipLaunchKernelGGL(goal_vec_bwd_kernel, dim3((unsigned)nwg), dim3(256), Fwd::goal_vec_lds(c, true), s, dE1f, W(P_W3) + c.compress_out,
                           g.cat, ws + w.dEg, (long)g.B, c.goal_dims, c.comb_hid);
        tn_small(ws + w.dEg, c.goal_dims, ws + w.gvec, c.goal_in, G(P_EMB), c.goal_in);
        colsum(ws + w.dEg, G(P_GB), g.B, c.goal_dims, c.goal_dims);
        return EC_OK;
    }

    // combiner and compressor of one encoder stream (the depth stream re-uses the gradient temporaries: one HIP stream)
    int encoder_stream(int sidx, const void* featS) {
        const Ws::Stream& o = w.st[sidx];
        const int B = g.B, S = g.S, M49 = g.M49, C = g.C, cat = g.cat;
        const int* goal32 = (const int*)(ws + w.goal32);
        auto WS = [&](int i) { return W(i, sidx); };
        auto GS = [&](int i) { return G(i, sidx); };
        if (p.wih != Wih::perm_learn) {
            const long total = (long)B * g.flat1;
            hipLaunchKernelGGL(from_cmajor_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, ws + w.dx,
                               ws + w.dx4, S, c.comb_out, total, g.flat, sidx * g.flat1);
        }
        if (!p.vec) (void)hipMemsetAsync(ws + w.dE1, 0, (size_t)c.num_goals * c.comb_hid * 4, s);
        if (p.tail_bwd) {
            // dm1 / dc2 / dc1 and all small weight gradients of the tail in one pass
            const long nwg = std::min<long>(TB_MAX_WG, (((long)M49 + 31) / 32 + 3) / 4);
            if (p.vec) {
                allow_big_lds<tail_bwd_kernel<true>>();
                hipLaunchKernelGGL(tail_bwd_kernel<true>, dim3((unsigned)nwg), dim3(256), p.tail_bwd_lds, s, ws + w.dx4, ws + o.m1, ws + o.c2, ws + o.c1,
                                   WS(P_W2), WS(P_W3), cat, WS(P_W4), (const int*)nullptr, S, 0, ws + w.dc1,
                                   p.dw1_planes ? (uint16_t*)(ws + w.dc1) : nullptr, ws + w.tpart, ws + w.tseg, (long)M49);
                hipLaunchKernelGGL(seg_fold_kernel, dim3((unsigned)B), dim3(128), 0, s, ws + w.tseg, ws + w.dE1f, S, (long)B);
            } else {
            allow_big_lds<tail_bwd_kernel<false>>();
            hipLaunchKernelGGL(tail_bwd_kernel<false>, dim3((unsigned)nwg), dim3(256), p.tail_bwd_lds, s, ws + w.dx4, ws + o.m1, ws + o.c2, ws + o.c1,
                               WS(P_W2), WS(P_W3), cat, WS(P_W4), goal32, S, c.num_goals, ws + w.dc1,
                               p.dw1_planes ? (uint16_t*)(ws + w.dc1) : nullptr, ws + w.tpart, ws + w.tpartE, (long)M49);
            }
            const int ne = TB_PART + c.num_goals * 128;
            // the y-slices' sums: behind the used partial sets when there is room (nwg < TB_MAX_WG), else in the dm1 area, which
            // the fused path never materialises (nwg == TB_MAX_WG means M49 >= 32,768 rows: 4 M floats)
            float* red = (nwg < TB_MAX_WG) ? ws + w.tpart + (size_t)nwg * 4 * TB_PART : ws + w.dm1;
            const size_t red_cap = (nwg < TB_MAX_WG) ? (size_t)(TB_MAX_WG - nwg) * 4 * TB_PART : (size_t)M49 * c.comb_hid;
            int ny = (int)std::min<size_t>(8, red_cap / (size_t)ne);
            if (ny < 1) return EC_ERR_WORKSPACE;
            hipLaunchKernelGGL(tail_bwd_reduce_kernel, dim3((unsigned)((ne + 255) / 256), (unsigned)ny), dim3(256), 0, s, ws + w.tpart,
                               (int)nwg * 4, ws + w.tpartE, c.num_goals, red);
            hipLaunchKernelGGL(tail_bwd_fold_kernel, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, s, red, ny, c.num_goals, GS(P_W4),
                               GS(P_W3), cat, GS(P_W2), GS(P_B4), GS(P_B2), GS(P_B1), ws + w.dE1);
        } else {
            // ---- target_obs_combiner ----
            RC(tn(ws + w.dx4, c.comb_out, ws + o.m1, c.comb_hid, 0, GS(P_W4), c.comb_out, c.comb_hid, M49, c.comb_hid));
            colsum(ws + w.dx4, GS(P_B4), M49, c.comb_out, c.comb_out);
            RC(ec_gemm_f32(ws + w.dx4, WS(P_W4), ws + w.dm1, M49, c.comb_hid, c.comb_out, c.comb_out, 1, c.comb_hid, 1, c.comb_hid,
                           0, nullptr, nullptr, nullptr, 0, ws + o.m1, nullptr, 1, stream));
            RC(tn(ws + w.dm1, c.comb_hid, ws + o.c2, c.compress_out, 0, GS(P_W3), c.comb_hid, c.compress_out, M49, cat));
            if (p.vec) hipLaunchKernelGGL(frame_sum_kernel, dim3((unsigned)B), dim3(128), 0, s, ws + w.dm1, ws + w.dE1f, S, c.comb_hid);
            else if (p.ordered) ec_goal_group_sum_launch(ws + w.dm1, goal32, ws + w.dE1, S, c.comb_hid, (long)B, c.num_goals, s);
            else
            hipLaunchKernelGGL(group_sum_scatter_kernel, dim3((unsigned)B), dim3(128), 0, s, ws + w.dm1, goal32, ws + w.dE1, S,
                               c.comb_hid, (long)B);
            // ---- resnet_compressor ----
            RC(ec_gemm_f32(ws + w.dm1, WS(P_W3), ws + w.dc2, M49, c.compress_out, c.comb_hid, c.comb_hid, 1, cat, 1,
                           c.compress_out, 0, nullptr, nullptr, nullptr, 0, ws + o.c2, nullptr, 1, stream));
            RC(tn(ws + w.dc2, c.compress_out, ws + o.c1, c.compress_hid, 0, GS(P_W2), c.compress_out, c.compress_hid, M49, c.compress_hid));
            colsum(ws + w.dc2, GS(P_B2), M49, c.compress_out, c.compress_out);
            RC(ec_gemm_f32(ws + w.dc2, WS(P_W2), ws + w.dc1, M49, c.compress_hid, c.compress_out, c.compress_out, 1,
                           c.compress_hid, 1, c.compress_hid, 0, nullptr, nullptr, nullptr, 0, ws + o.c1, nullptr, 1, stream));
            colsum(ws + w.dc1, GS(P_B1), M49, c.compress_hid, c.compress_hid);
        }
        if (p.vec) RC(goal_half_vec());
        else RC(goal_half(sidx));
        if (p.dw1_planes) return ec_dw_tn_xp(ws + w.dc1, featS, ws + w.tpart, GS(P_W1), M49, C, p.planes, stream);   // (tpart: free again after the reducer)
        return tn(ws + w.dc1, c.compress_hid, featS, C, p.feat_bf16, GS(P_W1), c.compress_hid, C, M49, C);
    }
};

}  // namespace

extern "C" int ec_policy_create(ec_policy_t** out, const ec_policy_cfg* cfg) { return ec_policy_create_rnn(out, cfg, EC_RNN_GRU); }
extern "C" int ec_policy_rnn_type(const ec_policy_t* h) { return h ? h->rnn : -1; }
extern "C" int ec_policy_state_width(const ec_policy_t* h) { return h ? h->layers * (h->rnn == EC_RNN_LSTM ? 2 : 1) * h->c.hidden : 0; }
extern "C" int ec_policy_rnn_layers(const ec_policy_t* h) { return h ? h->layers : 0; }
extern "C" int ec_policy_create_rnn(ec_policy_t** out, const ec_policy_cfg* cfg, int rnn_type) {
    return ec_policy_create_rnn_layers(out, cfg, rnn_type, 1);
}

extern "C" int ec_policy_create_rnn_layers(ec_policy_t** out, const ec_policy_cfg* cfg, int rnn_type, int num_layers) {
    if (!out || !cfg) return EC_ERR_ARG;
    if (rnn_type != EC_RNN_GRU && rnn_type != EC_RNN_LSTM) return EC_ERR_ARG;
    if (num_layers < 1 || num_layers > EC_RNN_MAX_LAYERS) return EC_ERR_ARG;
    const ec_policy_cfg& c = *cfg;
    if (c.fusion != 0 && c.fusion != 1) return EC_ERR_ARG;
    if (c.dual != 0 && c.dual != 1) return EC_ERR_ARG;
    if (c.dual && c.fusion) return EC_ERR_ARG;
    if (c.goal_in < 0 || c.goal_in > 8 || (c.goal_in && c.fusion)) return EC_ERR_ARG;
    if (c.goal_in && c.dual) return EC_ERR_UNSUPPORTED;
    if (c.prev_action_dims < 0 || c.prev_action_dims > 64 || (c.prev_action_null != 0 && c.prev_action_null != 1)) return EC_ERR_ARG;
    if (c.prev_action_null && !c.prev_action_dims) return EC_ERR_ARG;
    if (c.prev_action_dims && (c.dual || c.fusion)) return EC_ERR_UNSUPPORTED;   // (the two-tower and zero-shot agents: not built)
    if (c.in_channels <= 0 || c.spatial <= 0 || c.hidden <= 0 || (c.num_goals <= 0 && !c.goal_in) || c.num_actions <= 0) return EC_ERR_SHAPE;
    if ((c.in_channels & 3) || (c.hidden & 3)) return EC_ERR_SHAPE;
    if (c.fusion) {
        if (c.spatial != 1) return EC_ERR_SHAPE;
    } else {
        if (c.goal_dims <= 0 || c.compress_hid <= 0 || c.compress_out <= 0 || c.comb_hid <= 0 || c.comb_out <= 0)
            return EC_ERR_SHAPE;
        if ((c.compress_hid & 3) || (c.compress_out & 3) || (c.comb_hid & 3) || (c.comb_out & 3) || (c.goal_dims & 3))
            return EC_ERR_SHAPE;
    }
    // (coordinate goals: W3[:, co:] and one pass of frames sit in the LDS of the two goal_vec kernels)
    if (c.goal_in && std::max(Fwd::goal_vec_lds(c, false), Fwd::goal_vec_lds(c, true)) > 64 * 1024) return EC_ERR_SHAPE;
    if (num_layers > 1 && (c.dual || c.fusion)) return EC_ERR_UNSUPPORTED;   // (the two-tower and zero-shot agents keep one layer)
    if (rnn_type == EC_RNN_LSTM) {
        if (c.dual || c.fusion) return EC_ERR_UNSUPPORTED;   // (the two-tower and zero-shot agents keep the GRU)
        if (!ec_lstm_hidden_ok(c.hidden)) return EC_ERR_SHAPE; // (8 units x 4 gates per tile: hidden % 32 == 0, tiles within the LDS)
    }
    ec_policy* h = new (std::nothrow) ec_policy();
    if (!h) return EC_ERR_ALLOC;
    h->c = c;
    h->rnn = rnn_type; h->layers = num_layers;
    if (c.goal_in) h->c.num_goals = 0;   // ignored: no goal table anywhere (the table areas of the workspace are empty)
    const size_t S = (size_t)c.spatial * c.spatial;
    const size_t flat = c.fusion ? (size_t)c.in_channels : (size_t)(c.dual ? 2 : 1) * c.comb_out * S;
    // the goal embedding (coordinate goals: embed_goal.weight, then its bias), compressor and combiner: no elements on a fusion handle
    const size_t enc = c.fusion ? 0 : 1;
    const size_t n[1 + 8] = {c.goal_in ? (size_t)c.goal_dims * c.goal_in : (size_t)c.num_goals * c.goal_dims,
                             (size_t)c.compress_hid * c.in_channels, (size_t)c.compress_hid,
                             (size_t)c.compress_out * c.compress_hid, (size_t)c.compress_out,
                             (size_t)c.comb_hid * (c.compress_out + c.goal_dims), (size_t)c.comb_hid,
                             (size_t)c.comb_out * c.comb_hid, (size_t)c.comb_out};
    h->off[P_EMB] = h->put(enc * n[0]);
    h->off[P_GB] = h->put(c.goal_in ? (size_t)c.goal_dims : 0, c.goal_in != 0);
    for (int i = P_W1; i <= P_B4; ++i) h->off[i] = h->put(enc * n[i]);
    h->put_core(flat + c.prev_action_dims);
    // the dual encoder's depth stream: the compressor's and combiner's shapes again
    if (c.dual)
        for (int i = P_W1; i <= P_B4; ++i) h->off[i + (P_W1D - P_W1)] = h->put(n[i]);
    h->count = h->slots;
    // (kept as it was: a one-layer handle without the depth stream answers the indices up to the dual handle's count too, with
    // no elements at the end of the buffer)
    static_assert(P_COUNT_VEC + 1 <= P_COUNT_DUAL);   // (the most tensors such a handle has: coordinate goals and previous actions)
    while (num_layers == 1 && h->slots < P_COUNT_DUAL) h->put(0);
    *out = h;
    return EC_OK;
}
extern "C" void ec_policy_destroy(ec_policy_t* h) { delete h; }
extern "C" int ec_policy_set_goal_table(ec_policy_t* h, const float* table) {
    if (!h || !table || !h->c.fusion || h->pl.on) return EC_ERR_ARG;
    h->goal_table = table;
    return EC_OK;
}
extern "C" int ec_policy_num_param_tensors(const ec_policy_t* h) { return h ? h->count : P_COUNT_SINGLE; }   // (NULL: kept as it was)
extern "C" size_t ec_policy_flat_size(const ec_policy_t* h) { return h ? h->total : 0; }
extern "C" int ec_policy_param_offset(const ec_policy_t* h, int idx, size_t* off, size_t* numel) {
    if (!h || idx < 0 || !off || !numel) return EC_ERR_ARG;
    if (idx >= h->slots) return EC_ERR_ARG;
    *off = h->table[idx].off; *numel = h->table[idx].num;
    return EC_OK;
}
extern "C" size_t ec_policy_workspace_bytes(const ec_policy_t* h, int T, int N, int for_backward) {
    if (!h || T <= 0 || N <= 0) return 0;
    return make_plan(h, T, N, for_backward != 0 ? EC_POLICY_LEARN : EC_POLICY_INFER, false).w.end * 4;
}

// ---- the forward and act entry points: each fills a Call and hands it on ----
extern "C" int ec_policy_forward(const ec_policy_t* h, const float* params, const void* feat, int feat_bf16, const int64_t* goal,
                                 const float* h0, const float* masks, int T, int N, void* workspace, size_t ws_bytes, int for_backward,
                                 float* hv, float* h_final, ec_stream_t stream) {
    return ec_policy_forward2(h, params, feat, nullptr, feat_bf16, goal, h0, masks, T, N, workspace, ws_bytes, for_backward, hv, h_final, stream);
}
extern "C" int ec_policy_forward2(const ec_policy_t* h, const float* params, const void* feat, const void* feat2, int feat_bf16,
                                  const int64_t* goal, const float* h0, const float* masks, int T, int N, void* workspace,
                                  size_t ws_bytes, int for_backward, float* hv, float* h_final, ec_stream_t stream) {
    return policy_forward_impl(h, {.face = Face::tensor, .params = params, .feat = feat, .feat2 = feat2, .feat_bf16 = feat_bf16, .goal = goal,
                                   .h0 = h0, .masks = masks, .T = T, .N = N, .workspace = workspace, .ws_bytes = ws_bytes, .mode = for_backward,
                                   .hv = hv, .h_final = h_final, .stream = stream});
}
extern "C" int ec_policy_forward_vec(const ec_policy_t* h, const float* params, const void* feat, const void* feat2, int feat_bf16,
                                     const float* goal_vec, const float* h0, const float* masks, int T, int N, void* workspace,
                                     size_t ws_bytes, int for_backward, float* hv, float* h_final, ec_stream_t stream) {
    return policy_forward_impl(h, {.face = Face::tensor, .params = params, .feat = feat, .feat2 = feat2, .feat_bf16 = feat_bf16, .goal_vec = goal_vec,
                                   .h0 = h0, .masks = masks, .T = T, .N = N, .workspace = workspace, .ws_bytes = ws_bytes, .mode = for_backward,
                                   .hv = hv, .h_final = h_final, .stream = stream});
}

// The act step in ONE call ([U] allenact OnPolicyRLEngine.act: actor_critic(...) then distributions.sample() / log_probs()):
// ec_policy_forward2(T = 1, EC_POLICY_INFER | EC_POLICY_INFER_REUSE) whose heads launch also samples -- exactly the results of
// ec_policy_forward2 followed by ec_sample_actions, one launch less on the act step's serial chain.
extern "C" int ec_policy_act(const ec_policy_t* h, const float* params, const void* feat, const void* feat2, int feat_bf16,
                             const int64_t* goal, const float* h0, const float* masks, int N, void* workspace, size_t ws_bytes,
                             int reuse_tables, float* hv, float* h_final, int64_t* actions, float* logp, float* values,
                             uint64_t seed, uint64_t step, int first_actor, ec_stream_t stream) {
    return policy_act(h, {.face = Face::tensor, .params = params, .feat = feat, .feat2 = feat2, .feat_bf16 = feat_bf16, .goal = goal, .h0 = h0,
                          .masks = masks, .N = N, .workspace = workspace, .ws_bytes = ws_bytes, .mode = act_mode(reuse_tables), .hv = hv,
                          .h_final = h_final, .smp = {(long long*)actions, logp, values, seed, step, first_actor, 0}, .stream = stream});
}
extern "C" int ec_policy_act_vec(const ec_policy_t* h, const float* params, const void* feat, const void* feat2, int feat_bf16,
                                 const float* goal_vec, const float* h0, const float* masks, int N, void* workspace, size_t ws_bytes,
                                 int reuse_tables, float* hv, float* h_final, int64_t* actions, float* logp, float* values,
                                 uint64_t seed, uint64_t step, int first_actor, ec_stream_t stream) {
    return policy_act(h, {.face = Face::tensor, .params = params, .feat = feat, .feat2 = feat2, .feat_bf16 = feat_bf16, .goal_vec = goal_vec,
                          .h0 = h0, .masks = masks, .N = N, .workspace = workspace, .ws_bytes = ws_bytes, .mode = act_mode(reuse_tables), .hv = hv,
                          .h_final = h_final, .smp = {(long long*)actions, logp, values, seed, step, first_actor, 0}, .stream = stream});
}

// The evaluation act step (readme_files/baselines_robothor_objectnav.md:66-68 `--eval`, baselines_habitat.md:89-97
// `--run-type eval`, zeroshot_objectnav.md:20-27): ec_policy_act / ec_policy_act_vec whose heads launch takes
// CategoricalDistr.mode() instead of a draw (SampleArgs::greedy; the same kernel instances and launch geometry).
extern "C" int ec_policy_act_greedy(const ec_policy_t* h, const float* params, const void* feat, const void* feat2, int feat_bf16,
                                    const int64_t* goal, const float* h0, const float* masks, int N, void* workspace, size_t ws_bytes,
                                    int reuse_tables, float* hv, float* h_final, int64_t* actions, float* logp, float* values,
                                    ec_stream_t stream) {
    return policy_act(h, {.face = Face::tensor, .params = params, .feat = feat, .feat2 = feat2, .feat_bf16 = feat_bf16, .goal = goal, .h0 = h0,
                          .masks = masks, .N = N, .workspace = workspace, .ws_bytes = ws_bytes, .mode = act_mode(reuse_tables), .hv = hv,
                          .h_final = h_final, .smp = {(long long*)actions, logp, values, 0, 0, 0, 1}, .stream = stream});
}
extern "C" int ec_policy_act_vec_greedy(const ec_policy_t* h, const float* params, const void* feat, const void* feat2, int feat_bf16,
                                        const float* goal_vec, const float* h0, const float* masks, int N, void* workspace,
                                        size_t ws_bytes, int reuse_tables, float* hv, float* h_final, int64_t* actions, float* logp,
                                        float* values, ec_stream_t stream) {
    return policy_act(h, {.face = Face::tensor, .params = params, .feat = feat, .feat2 = feat2, .feat_bf16 = feat_bf16, .goal_vec = goal_vec,
                          .h0 = h0, .masks = masks, .N = N, .workspace = workspace, .ws_bytes = ws_bytes, .mode = act_mode(reuse_tables), .hv = hv,
                          .h_final = h_final, .smp = {(long long*)actions, logp, values, 0, 0, 0, 1}, .stream = stream});
}

// The act step in one call for every handle (include/ec_amd.h): selection by flag, and teacher forcing behind it
extern "C" int ec_policy_act_ex(const ec_policy_t* h, const float* params, const void* feat, const void* feat2, int feat_bf16,
                                const int64_t* goal, const float* goal_vec, const float* h0, const float* masks, int N, void* workspace,
                                size_t ws_bytes, int reuse_tables, float* hv, float* h_final, int64_t* actions, float* logp,
                                float* values, int greedy, uint64_t seed, uint64_t step, int first_actor,
                                const int64_t* expert_actions, const float* expert_mask, float force_p, ec_stream_t stream) {
    const ForceArgs force{(const long long*)expert_actions, expert_mask, force_p};
    return policy_act(h, {.face = Face::tensor, .params = params, .feat = feat, .feat2 = feat2, .feat_bf16 = feat_bf16, .goal = goal,
                          .goal_vec = goal_vec, .h0 = h0, .masks = masks, .N = N, .workspace = workspace, .ws_bytes = ws_bytes,
                          .mode = act_mode(reuse_tables), .hv = hv, .h_final = h_final,
                          .smp = {(long long*)actions, logp, values, seed, step, first_actor, greedy ? 1 : 0}, .force = &force, .stream = stream});
}

// Handles with a previous-action embedding (include/ec_amd.h): ec_policy_forward_vec / ec_policy_act_ex with both goal arguments
// and the previous actions
extern "C" int ec_policy_forward_pa(const ec_policy_t* h, const float* params, const void* feat, const void* feat2, int feat_bf16,
                                    const int64_t* goal, const float* goal_vec, const int64_t* prev_actions, const float* h0,
                                    const float* masks, int T, int N, void* workspace, size_t ws_bytes, int for_backward, float* hv,
                                    float* h_final, ec_stream_t stream) {
    return policy_forward_impl(h, {.face = Face::tensor_pa, .params = params, .feat = feat, .feat2 = feat2, .feat_bf16 = feat_bf16, .goal = goal,
                                   .goal_vec = goal_vec, .prev_actions = prev_actions, .h0 = h0, .masks = masks, .T = T, .N = N,
                                   .workspace = workspace, .ws_bytes = ws_bytes, .mode = for_backward, .hv = hv, .h_final = h_final, .stream = stream});
}
extern "C" int ec_policy_act_pa(const ec_policy_t* h, const float* params, const void* feat, const void* feat2, int feat_bf16,
                                const int64_t* goal, const float* goal_vec, const int64_t* prev_actions, const float* h0,
                                const float* masks, int N, void* workspace, size_t ws_bytes, int reuse_tables, float* hv, float* h_final,
                                int64_t* actions, float* logp, float* values, int greedy, uint64_t seed, uint64_t step, int first_actor,
                                const int64_t* expert_actions, const float* expert_mask, float force_p, ec_stream_t stream) {
    const ForceArgs force{(const long long*)expert_actions, expert_mask, force_p};
    return policy_act(h, {.face = Face::tensor_pa, .params = params, .feat = feat, .feat2 = feat2, .feat_bf16 = feat_bf16, .goal = goal,
                          .goal_vec = goal_vec, .prev_actions = prev_actions, .h0 = h0, .masks = masks, .N = N, .workspace = workspace,
                          .ws_bytes = ws_bytes, .mode = act_mode(reuse_tables), .hv = hv, .h_final = h_final,
                          .smp = {(long long*)actions, logp, values, seed, step, first_actor, greedy ? 1 : 0}, .force = &force, .stream = stream});
}

// The pooled-embedding net (include/ec_amd.h): a handle whose plan is the fusion handle's with in_channels = hidden, its own
// tensors in front of weight_ih_l0, and the two entry points below
extern "C" int ec_policy_is_pooled(const ec_policy_t* h) { return (h && h->pl.on && !h->pl.tv) ? 1 : 0; }
extern "C" int ec_policy_create_pooled(ec_policy_t** out, const ec_pooled_cfg* cfg) {
    if (!out || !cfg) return EC_ERR_ARG;
    const ec_pooled_cfg& q = *cfg;
    if (q.rnn_type != EC_RNN_GRU && q.rnn_type != EC_RNN_LSTM) return EC_ERR_ARG;
    if (q.num_layers < 1 || q.num_layers > EC_RNN_MAX_LAYERS) return EC_ERR_ARG;
    if (q.num_sensors < 0 || q.num_sensors > 3 || q.num_goals < 0 || q.num_goals > 256) return EC_ERR_ARG;
    if (q.num_goals == 0 && q.num_sensors == 0) return EC_ERR_ARG;            // the net needs a goal
    int K = 0;
    for (int i = 0; i < q.num_sensors; ++i) {
        if (q.sensor_in[i] < 1 || q.sensor_in[i] > 8) return EC_ERR_ARG;
        K += q.sensor_in[i];
    }
    if (K > 8) return EC_ERR_ARG;
    if (q.embed_dims < 1 || q.embed_dims > 64) return EC_ERR_ARG;
    if (q.num_actions < 2 || q.num_actions > 256) return EC_ERR_ARG;
    if (q.prev_action_dims < 0 || q.prev_action_dims > 64 || (q.prev_action_null != 0 && q.prev_action_null != 1)) return EC_ERR_ARG;
    if (q.prev_action_null && !q.prev_action_dims) return EC_ERR_ARG;
    if (q.embed_in < 64 || q.embed_in > 4096 || (q.embed_in & 3)) return EC_ERR_SHAPE;
    if (q.hidden <= 0 || (q.hidden & 3)) return EC_ERR_SHAPE;
    if (q.rnn_type == EC_RNN_LSTM && !ec_lstm_hidden_ok(q.hidden)) return EC_ERR_SHAPE;
    ec_policy* h = new (std::nothrow) ec_policy();
    if (!h) return EC_ERR_ALLOC;
    ec_policy_cfg& c = h->c;
    c = ec_policy_cfg{};
    c.in_channels = q.hidden; c.spatial = 1; c.hidden = q.hidden; c.num_goals = q.num_goals; c.num_actions = q.num_actions;
    c.fusion = 1;                        // (the plan's: M49 = 0, flat = in_channels; no goal table is ever read)
    c.prev_action_dims = q.prev_action_dims; c.prev_action_null = q.prev_action_null;
    h->rnn = q.rnn_type; h->layers = q.num_layers;
    ec_policy::Pooled& pl = h->pl;
    pl.on = true; pl.D = q.embed_in; pl.ed = q.embed_dims; pl.ids = q.num_goals > 0 ? 1 : 0; pl.ns = q.num_sensors; pl.K = K;
    for (int i = 0; i < q.num_sensors; ++i) pl.k[i] = q.sensor_in[i];
    const size_t H = q.hidden;
    pl.off[PL_FCW] = h->put(H * pl.D);
    pl.off[PL_FCB] = h->put(H);
    pl.off[PL_GEMB] = h->put((size_t)q.num_goals * pl.ed, pl.ids != 0);
    for (int i = 0; i < pl.ns; ++i) {
        pl.off[PL_SW0 + 2 * i] = h->put((size_t)pl.ed * pl.k[i]);
        pl.off[PL_SB0 + 2 * i] = h->put((size_t)pl.ed);
    }
    h->put_core(H + pl.side() + q.prev_action_dims);
    h->count = h->slots;
    *out = h;
    return EC_OK;
}
extern "C" int ec_policy_forward_pooled(const ec_policy_t* h, const float* params, const float* embed, const int64_t* goal,
                                        const float* sensors, const int64_t* prev_actions, const float* h0, const float* masks, int T,
                                        int N, void* workspace, size_t ws_bytes, int for_backward, float* hv, float* h_final,
                                        ec_stream_t stream) {
    return policy_forward_impl(h, {.face = Face::pooled, .params = params, .feat = embed, .goal = goal, .prev_actions = prev_actions,
                                   .sensors = sensors, .h0 = h0, .masks = masks, .T = T, .N = N, .workspace = workspace, .ws_bytes = ws_bytes,
                                   .mode = for_backward, .hv = hv, .h_final = h_final, .stream = stream});
}
extern "C" int ec_policy_act_pooled(const ec_policy_t* h, const float* params, const float* embed, const int64_t* goal,
                                    const float* sensors, const int64_t* prev_actions, const float* h0, const float* masks, int N,
                                    void* workspace, size_t ws_bytes, int reuse_tables, float* hv, float* h_final, int64_t* actions,
                                    float* logp, float* values, int greedy, uint64_t seed, uint64_t step, int first_actor,
                                    const int64_t* expert_actions, const float* expert_mask, float force_p, ec_stream_t stream) {
    const ForceArgs force{(const long long*)expert_actions, expert_mask, force_p};
    return policy_act(h, {.face = Face::pooled, .params = params, .feat = embed, .goal = goal, .prev_actions = prev_actions, .sensors = sensors,
                          .h0 = h0, .masks = masks, .N = N, .workspace = workspace, .ws_bytes = ws_bytes, .mode = act_mode(reuse_tables), .hv = hv,
                          .h_final = h_final, .smp = {(long long*)actions, logp, values, seed, step, first_actor, greedy ? 1 : 0}, .force = &force,
                          .stream = stream});
}

// The two-view rearrangement net (include/ec_amd.h): the pooled-embedding handle's plan from v onwards, two_view.hip's front
extern "C" int ec_policy_is_two_view(const ec_policy_t* h) { return (h && h->pl.tv) ? 1 : 0; }
extern "C" int ec_policy_create_two_view(ec_policy_t** out, const ec_two_view_cfg* cfg) {
    if (!out || !cfg) return EC_ERR_ARG;
    const ec_two_view_cfg& q = *cfg;
    if (q.rnn_type != EC_RNN_GRU && q.rnn_type != EC_RNN_LSTM) return EC_ERR_ARG;
    if (q.num_layers < 1 || q.num_layers > EC_RNN_MAX_LAYERS) return EC_ERR_ARG;
    if (q.num_actions < 2 || q.num_actions > 256) return EC_ERR_ARG;
    if (q.prev_action_dims < 0 || q.prev_action_dims > 512 || (q.prev_action_null != 0 && q.prev_action_null != 1)) return EC_ERR_ARG;
    if (q.prev_action_null && !q.prev_action_dims) return EC_ERR_ARG;
    if (q.spatial < 1 || q.spatial > 8) return EC_ERR_SHAPE;
    if (!ec_tv_shape_ok(ec_tv_shape{1, q.spatial * q.spatial, q.in_channels, q.hidden, q.attn_hidden})) return EC_ERR_SHAPE;
    ec_policy* h = new (std::nothrow) ec_policy();
    if (!h) return EC_ERR_ALLOC;
    ec_policy_cfg& c = h->c;
    c = ec_policy_cfg{};
    c.in_channels = q.hidden; c.spatial = 1; c.hidden = q.hidden; c.num_goals = 0; c.num_actions = q.num_actions;
    c.fusion = 1;                        // (the plan's: M49 = 0, flat = in_channels = hidden; no goal table is ever read)
    c.prev_action_dims = q.prev_action_dims; c.prev_action_null = q.prev_action_null;
    h->rnn = q.rnn_type; h->layers = q.num_layers;
    ec_policy::Pooled& pl = h->pl;
    pl.on = true; pl.tv = true; pl.tvC = q.in_channels; pl.tvS2 = q.spatial * q.spatial; pl.tvA1 = q.attn_hidden;
    const size_t H = q.hidden, A1 = q.attn_hidden, K3 = 3 * (size_t)q.in_channels;
    pl.off[TV_WE] = h->put(H * K3);
    pl.off[TV_BE] = h->put(H);
    pl.off[TV_WA] = h->put(A1 * K3);
    pl.off[TV_BA] = h->put(A1);
    pl.off[TV_W2] = h->put(A1);
    pl.off[TV_B2] = h->put(1);
    h->put_core(H + q.prev_action_dims);
    h->count = h->slots;
    *out = h;
    return EC_OK;
}
extern "C" int ec_policy_forward_two_view(const ec_policy_t* h, const float* params, const void* feat, const void* feat2,
                                          const int64_t* prev_actions, const float* h0, const float* masks, int T, int N,
                                          void* workspace, size_t ws_bytes, int for_backward, float* hv, float* h_final,
                                          ec_stream_t stream) {
    return policy_forward_impl(h, {.face = Face::two_view, .params = params, .feat = feat, .feat2 = feat2, .prev_actions = prev_actions, .h0 = h0,
                                   .masks = masks, .T = T, .N = N, .workspace = workspace, .ws_bytes = ws_bytes, .mode = for_backward, .hv = hv,
                                   .h_final = h_final, .stream = stream});
}
extern "C" int ec_policy_act_two_view(const ec_policy_t* h, const float* params, const void* feat, const void* feat2,
                                      const int64_t* prev_actions, const float* h0, const float* masks, int N, void* workspace,
                                      size_t ws_bytes, int reuse_tables, float* hv, float* h_final, int64_t* actions, float* logp,
                                      float* values, int greedy, uint64_t seed, uint64_t step, int first_actor,
                                      const int64_t* expert_actions, const float* expert_mask, float force_p, ec_stream_t stream) {
    const ForceArgs force{(const long long*)expert_actions, expert_mask, force_p};
    return policy_act(h, {.face = Face::two_view, .params = params, .feat = feat, .feat2 = feat2, .prev_actions = prev_actions, .h0 = h0,
                          .masks = masks, .N = N, .workspace = workspace, .ws_bytes = ws_bytes, .mode = act_mode(reuse_tables), .hv = hv,
                          .h_final = h_final, .smp = {(long long*)actions, logp, values, seed, step, first_actor, greedy ? 1 : 0}, .force = &force,
                          .stream = stream});
}

extern "C" int ec_policy_backward(const ec_policy_t* h, const float* params, const void* feat, int feat_bf16,
                                  const float* masks, int T, int N, void* workspace, size_t ws_bytes, const float* dhv,
                                  const float* dh_final, float* grads, ec_stream_t stream) {
    return ec_policy_backward2(h, params, feat, nullptr, feat_bf16, masks, T, N, workspace, ws_bytes, dhv, dh_final, grads, stream);
}

extern "C" int ec_policy_backward2(const ec_policy_t* h, const float* params, const void* feat, const void* feat2, int feat_bf16,
                                   const float* masks, int T, int N, void* workspace, size_t ws_bytes, const float* dhv,
                                   const float* dh_final, float* grads, ec_stream_t stream) {
    return ec_policy_backward3(h, params, feat, feat2, feat_bf16, masks, T, N, workspace, ws_bytes, dhv, dh_final, grads, nullptr, stream);
}

// Reads what ec_policy_forward2(.., EC_POLICY_LEARN) left in `workspace`: built from the same (handle, T, N, dtype), the plan
// here IS that forward's plan -- in particular which of ws.x / ws.x4 holds the GRU input.
extern "C" int ec_policy_backward3(const ec_policy_t* h, const float* params, const void* feat, const void* feat2, int feat_bf16,
                                   const float* masks, int T, int N, void* workspace, size_t ws_bytes, const float* dhv,
                                   const float* dh_final, float* grads, ec_event_t recurrent_grads_ready, ec_stream_t stream) {
    if (!h || !params || !feat || !masks || !workspace || !dhv || !grads) return EC_ERR_ARG;
    if (h->c.dual && !feat2) return EC_ERR_ARG;
    if (h->pl.on && ((uintptr_t)feat & 15) != 0) return EC_ERR_ARG;      // (the embedding rows are read as float4)
    if (h->pl.tv && (!feat2 || !feat_bf16 || ((uintptr_t)feat2 & 15) != 0)) return EC_ERR_ARG;   // (two views, both bf16)
    if (T <= 0 || N <= 0) return EC_ERR_SHAPE;
    const Plan p = make_plan(h, T, N, EC_POLICY_LEARN, feat_bf16 != 0 && !h->pl.on);
    if (ws_bytes < p.w.end * 4) return EC_ERR_WORKSPACE;
    Bwd b(h, p, params, workspace, stream);
    b.grads = grads;
    b.masks_all = masks;
    RC(b.heads(dhv));
    for (int l = p.g.L - 1; l >= 0; --l) {       // top layer down; layer l - 1's dhs is layer l's dx
        b.lay = b.layer(l); b.lidx = l;
        RC(b.recurrence(masks, dh_final));
        if (l) RC(b.upper_layer_grads(l));
    }
    RC(b.gru_grads());
    if (h->pl.on) RC(b.pooled_side_grads());
    // the gradients of the GRU and of both heads (tensors rnn.weight_ih_l0 .. critic.fc.bias: 92 % of the bucket) are final
    // here; what follows only writes the goal encoder's.  A caller that sums the bucket over ranks starts that section's
    // all-reduce behind this event, under the rest of this backward
    if (recurrent_grads_ready && hipEventRecord((hipEvent_t)recurrent_grads_ready, b.s) != hipSuccess) return EC_ERR_LAUNCH;
    if (h->pl.tv) {
        RC(b.two_view_grads(feat, feat2));
    } else if (h->pl.on) {
        RC(b.pooled_fc_grads((const float*)feat));
    } else if (!h->c.fusion) {   // (fusion: the image embedding and the goal table are frozen, nothing trainable upstream of the GRU)
        b.parts_ok = p.wih == Wih::perm_learn;   // the plain path writes dx into the partial-matrix area now
        RC(b.input_grad());
        for (int sidx = 0; sidx < p.g.nstream; ++sidx) RC(b.encoder_stream(sidx, sidx ? feat2 : feat));
    }
    EC_CHECK_LAUNCH();
    return EC_OK;
}
