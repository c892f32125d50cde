// LSTM recurrent core of the single-tower actor-critic policy: the fused forward step, the fused reverse step, the plain gate
// kernel of the gate-plus-GEMM route, and their launches for policy.hip's two recurrence() members.
//
// Restates torch.nn.LSTM's cell under the RNNStateEncoder episode mask ([U] allenact basic_models.py RNNStateEncoder with
// rnn_type="LSTM"; neither source is under the reference tree: parity unpinned, as for the rest of the policy):
//   hp = m*h_prev;  cp = m*c_prev                       (the mask resets BOTH states)
//   a  = (W_ih x + b_ih) + m*(h_prev W_hh^T) + b_hh     gate order i, f, g, o  (rows 0..H-1, H..2H-1, ...)
//   i = s(a_i); f = s(a_f); g = tanh(a_g); o = s(a_o);  c = f*cp + i*g;  h = o*tanh(c)
// Reverse step (dh = dL/dh_t with every later step's contribution in it, carry_c = dL/dc_t from step t+1):
//   tc = tanh(c);  do = dh*tc*o(1-o);  dc = carry_c + dh*o*(1-tc^2)
//   di = dc*g*i(1-i);  df = dc*cp*f(1-f);  dg = dc*i*(1-g^2);  carry_c <- m*dc*f;  dh_{t-1} += m*(da W_hh)
// da is the gradient wrt the input projection AND wrt the recurrent projection (the cell has no gate between them), so one
// [N, 4H] area serves where the GRU keeps dgi and dghb.  No floating-point atomics anywhere in this file.
#include "common.h"

namespace {

constexpr size_t LSTM_LDS_LIMIT = 160 * 1024;

// (expf, not the GRU's __expf: the step kernels alone are held to 10 x the fp32 closed form's own distance from float64)
__device__ __forceinline__ float lstm_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// Fused forward step: recurrent projection + gate math in ONE launch per time step; the geometry of policy.hip's
// gru_step_fwd_kernel.  Workgroup (blockIdx.x, blockIdx.y) owns hidden units j0..j0+7 of actors n0..n0+31: 8 units x 4 gates
// are exactly the 32 columns of a v_mfma_f32_32x32x2_f32 tile (the GRU zero-fills 8 of them).
//   * the h_prev tile [32 x KC] and the 32 W_hh rows [32 x KC] are staged in LDS (row pitch KC + 4 floats), K walked in
//     chunks of KC = 256 through LDS-DMA when H % 256 == 0 and as one plain-staged chunk otherwise: 66.5 KB at most when
//     chunked, so the recurrences of two actor slices share a CU;
//   * wave w contracts its quarter of every chunk on the exact-fp32 MFMA; the four partial tiles are summed through LDS in
//     a fixed order (actor-local: an actor's result does not depend on how the actors are sliced);
//   * thread (a, u) applies the cell of unit j0 + u of actor a.  The mask multiplies the contraction result
//     (m (h W^T) == (m h) W^T exactly for m in {0, 1}).
// hprev / cprev: rows of pitch ld_prev ([h | c] rows of pitch 2H at step 0, the dense histories afterwards); hout / cout:
// pitches ld_h / ld_c; hout2 (pitch ld_h2, or null): a second copy of h -- the act step stores h densely for the heads AND
// into the caller's [h | c] state row, so no copy launch follows.  gates (learn pass, or null): i, f, g, o [N, 4H] with
// hp_s / cp_s [N, H] (or null) = the masked previous states the backward needs.
__global__ __launch_bounds__(256) void lstm_step_fwd_kernel(const float* __restrict__ gi, const float* __restrict__ Whh,
                                                           const float* __restrict__ bhh, const float* __restrict__ hprev,
                                                           const float* __restrict__ cprev, long ld_prev,
                                                           const float* __restrict__ mask, float* __restrict__ hout, long ld_h,
                                                           float* __restrict__ cout, long ld_c, float* __restrict__ hout2, long ld_h2,
                                                           float* __restrict__ gates, float* __restrict__ hp_s,
                                                           float* __restrict__ cp_s, int N, int H, int gi_parts, long gi_pstride) {
    extern __shared__ __attribute__((aligned(16))) float lsm[];
    const int KC = ((H & 255) == 0) ? 256 : H;
    const int P = KC + 4;
    float* sA = lsm;
    float* sB = lsm + 32 * P;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j0 = blockIdx.x * 8, n0 = blockIdx.y * 32;
    const int i = lane & 31, hh = lane >> 5;
    f32x16_t acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int k0 = 0; k0 < H; k0 += KC) {
        if (k0) __syncthreads();                                        // every wave is done reading the previous chunk
        if (KC == 256) {
            // LDS-DMA staging: one 1-KiB piece per tile row (256 floats); 64 rows round-robin over the 4 waves
            typedef __attribute__((address_space(3))) void lds_v;
            typedef const __attribute__((address_space(1))) void gbl_v;
            const int uwave = __builtin_amdgcn_readfirstlane(wave);
            for (int r = uwave; r < 64; r += 4) {
                const float* src;
                float* dst;
                if (r < 32) {
                    const int n = min(n0 + r, N - 1);                   // rows past N are never read back
                    src = hprev + (long)n * ld_prev + k0 + lane * 4;
                    dst = sA + r * P;
                } else {
                    const int c = r - 32;                               // tile column c = gate (c >> 3), unit j0 + (c & 7)
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
                float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
                const int n = n0 + r;
                if (n < N) a = *reinterpret_cast<const float4*>(hprev + (long)n * ld_prev + c4 * 4);
                const float4 b = *reinterpret_cast<const float4*>(Whh + ((long)(r >> 3) * H + j0 + (r & 7)) * H + c4 * 4);
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
    float* part = lsm;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * hh;     // actor (C/D layout of the 32x32 MFMA), column = lane & 31
        part[(wave * 32 + row) * 32 + i] = acc[r];
    }
    __syncthreads();
    const int a_ = tid >> 3, u = tid & 7;
    const int n = n0 + a_, j = j0 + u;
    if (n >= N) return;
    const float* gir = gi + (long)n * 4 * H;
    const float m = mask[n];
    float a[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int c = g * 8 + u;
        const float gh = ((part[(0 * 32 + a_) * 32 + c] + part[(1 * 32 + a_) * 32 + c]) + part[(2 * 32 + a_) * 32 + c]) +
                         part[(3 * 32 + a_) * 32 + c];
        float x = gir[g * H + j];
        for (int p2 = 1; p2 < gi_parts; ++p2) x += gir[p2 * gi_pstride + g * H + j];   // split-K parts of the input projection, in order
        a[g] = x + m * gh + bhh[g * H + j];
    }
    const float hp = m * hprev[(long)n * ld_prev + j];
    const float cp = m * cprev[(long)n * ld_prev + j];
    const float ig = lstm_sigmoid(a[0]), fg = lstm_sigmoid(a[1]), gg = tanhf(a[2]), og = lstm_sigmoid(a[3]);
    const float cn = fg * cp + ig * gg;
    const float hn = og * tanhf(cn);
    hout[(long)n * ld_h + j] = hn;
    cout[(long)n * ld_c + j] = cn;
    if (hout2) hout2[(long)n * ld_h2 + j] = hn;
    if (gates) {
        float* gp = gates + (long)n * 4 * H;
        gp[j] = ig; gp[H + j] = fg; gp[2 * H + j] = gg; gp[3 * H + j] = og;
        if (hp_s) {
            const long o = (long)n * H + j;
            hp_s[o] = hp;
            cp_s[o] = cp;
        }
    }
}

// the cell's gate gradients of one (actor, unit); returns what carry_c becomes
__device__ __forceinline__ float lstm_cell_bwd(float dh, float dc_in, float ig, float fg, float gg, float og, float c, float cp, float m,
                                               float* __restrict__ da_row, int H, int j) {
    const float tc = tanhf(c);
    const float d_o = dh * tc * og * (1.f - og);
    const float dc = dc_in + dh * og * (1.f - tc * tc);
    da_row[j] = dc * gg * ig * (1.f - ig);
    da_row[H + j] = dc * cp * fg * (1.f - fg);
    da_row[2 * H + j] = dc * ig * (1.f - gg * gg);
    da_row[3 * H + j] = d_o;
    return m * dc * fg;
}

// Reverse step of the gate-plus-GEMM route (and step T-1 of the fused one): dh = dhs + carry_h.  carry_h is left ZERO: the
// GEMM that follows accumulates m * (da W_hh) onto it (the LSTM has no element-wise path from h_t to h_{t-1}).
__global__ void lstm_gates_bwd_kernel(const float* __restrict__ dhs, float* __restrict__ carry_h, float* __restrict__ carry_c,
                                      const float* __restrict__ gates, const float* __restrict__ cs, const float* __restrict__ cp_s,
                                      const float* __restrict__ mask, float* __restrict__ da, int N, int H) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N * H) return;
    const int n = i / H, j = i - n * H;
    const float* g = gates + (long)n * 4 * H;
    const float dh = dhs[i] + carry_h[i];
    carry_c[i] = lstm_cell_bwd(dh, carry_c[i], g[j], g[H + j], g[2 * H + j], g[3 * H + j], cs[i], cp_s[i], mask[n],
                               da + (long)n * 4 * H, H, j);
    carry_h[i] = 0.f;
}

// Fused reverse step (H % 256 == 0): the recurrent back-projection of step t+1 and the gate math of step t in ONE launch,
//   dh[n, j] = dhs_t[n, j] + m_{t+1}[n] * sum_k da_{t+1}[n, k] W_hh[k, j]
// the geometry of policy.hip's gru_step_bwd_kernel with K = 4H: workgroup (blockIdx.x, blockIdx.y) owns hidden units
// j0..j0+31 of actors n0..n0+31, K walked in 256-float chunks through LDS-DMA (A tile = da rows, B tile = rows j0.. of
// W_hh^T [H, 4H]), the four waves' partial tiles summed through LDS in a fixed order.  carry_h is neither read nor written.
__global__ __launch_bounds__(256) void lstm_step_bwd_kernel(const float* __restrict__ da_next, const float* __restrict__ WhhT,
                                                           const float* __restrict__ mask_next, const float* __restrict__ dhs,
                                                           float* __restrict__ carry_c, const float* __restrict__ gates,
                                                           const float* __restrict__ cs, const float* __restrict__ cp_s,
                                                           const float* __restrict__ mask, float* __restrict__ da, int N, int H) {
    extern __shared__ __attribute__((aligned(16))) float lsm[];
    constexpr int KC = 256, P = KC + 4;
    const int K = 4 * H;
    float* sA = lsm;
    float* sB = lsm + 32 * P;
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
                src = da_next + (long)n * K + k0 + lane * 4;
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
    float* part = lsm;
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
    const float* g = gates + (long)n * 4 * H;
    float* ga = da + (long)n * 4 * H;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int c = u0 + 8 * q, j = j0 + c;
        const float proj = ((part[(0 * 32 + a_) * 32 + c] + part[(1 * 32 + a_) * 32 + c]) + part[(2 * 32 + a_) * 32 + c]) +
                           part[(3 * 32 + a_) * 32 + c];
        const long o = (long)n * H + j;
        const float dh = dhs[o] + mn * proj;
        carry_c[o] = lstm_cell_bwd(dh, carry_c[o], g[j], g[H + j], g[2 * H + j], g[3 * H + j], cs[o], cp_s[o], m, ga, H, j);
    }
}

// [N, 2H] rows [h | c] <-> two dense [N, H] halves (split == 1: state -> halves; 0: halves -> state)
__global__ void lstm_state_rows_kernel(float* __restrict__ state, float* __restrict__ hpart, float* __restrict__ cpart, int N, int H,
                                       int split) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N * H) return;
    const int n = i / H, j = i - n * H;
    float* row = state + (long)n * 2 * H;
    if (split) { hpart[i] = row[j]; cpart[i] = row[H + j]; }
    else { row[j] = hpart[i]; row[H + j] = cpart[i]; }
}

template <auto Kernel>
void lstm_allow_big_lds() {
    static std::atomic<uint64_t> done{0};
    if (auto guard = ec_attr_needed(done))
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LSTM_LDS_LIMIT);
}

}  // namespace

// policy.hip's hooks (declared in common.h): the launches without the argument checks of the C-ABI faces below
size_t ec_lstm_fwd_lds(int H) {
    return std::max((size_t)2 * 32 * (((H & 255) == 0 ? 256 : H) + 4) * sizeof(float), (size_t)4 * 32 * 32 * sizeof(float));
}
bool ec_lstm_hidden_ok(int H) { return H > 0 && (H % 32) == 0 && ec_lstm_fwd_lds(H) <= LSTM_LDS_LIMIT; }

void ec_lstm_fwd_launch(const float* gi, const float* whh, const float* bhh, const float* hprev, const float* cprev, long ld_prev,
                        const float* mask, float* hout, long ld_h, float* cout, long ld_c, float* hout2, long ld_h2, float* gates,
                        float* hp_s, float* cp_s, int N, int H, int gi_parts, long gi_pstride, hipStream_t s) {
    lstm_allow_big_lds<lstm_step_fwd_kernel>();
    hipLaunchKernelGGL(lstm_step_fwd_kernel, dim3((unsigned)(H / 8), (unsigned)((N + 31) / 32)), dim3(256), ec_lstm_fwd_lds(H), s, gi, whh, bhh,
                       hprev, cprev, ld_prev, mask, hout, ld_h, cout, ld_c, hout2, ld_h2, gates, hp_s, cp_s, N, H, gi_parts, gi_pstride);
}
void ec_lstm_bwd_gates_launch(const float* dhs, float* carry_h, float* carry_c, const float* gates, const float* cs, const float* cp_s,
                              const float* mask, float* da, int N, int H, hipStream_t s) {
    hipLaunchKernelGGL(lstm_gates_bwd_kernel, dim3((unsigned)((N * H + 255) / 256)), dim3(256), 0, s, dhs, carry_h, carry_c, gates, cs, cp_s,
                       mask, da, N, H);
}
void ec_lstm_bwd_fused_launch(const float* da_next, const float* whhT, const float* mask_next, const float* dhs, float* carry_c,
                              const float* gates, const float* cs, const float* cp_s, const float* mask, float* da, int N, int H,
                              hipStream_t s) {
    lstm_allow_big_lds<lstm_step_bwd_kernel>();
    hipLaunchKernelGGL(lstm_step_bwd_kernel, dim3((unsigned)(H / 32), (unsigned)((N + 31) / 32)), dim3(256),
                       (size_t)2 * 32 * (256 + 4) * sizeof(float), s, da_next, whhT, mask_next, dhs, carry_c, gates, cs, cp_s, mask, da, N, H);
}
void ec_lstm_state_rows_launch(float* state, float* hpart, float* cpart, int N, int H, int split, hipStream_t s) {
    hipLaunchKernelGGL(lstm_state_rows_kernel, dim3((unsigned)((N * H + 255) / 256)), dim3(256), 0, s, state, hpart, cpart, N, H, split);
}

extern "C" int ec_lstm_step_fwd(const float* a_in, const float* whh, const float* bhh, const float* state_prev, long ld_prev,
                                const float* mask, float* h_out, long ld_h, float* c_out, long ld_c, float* gates, int N, int H,
                                ec_stream_t stream) {
    if (!a_in || !whh || !bhh || !state_prev || !mask || !h_out || !c_out) return EC_ERR_ARG;
    if (N <= 0 || !ec_lstm_hidden_ok(H)) return EC_ERR_SHAPE;
    if ((ld_prev != H && ld_prev < 2L * H) || (ld_prev & 3) || ld_h < H || ld_c < H) return EC_ERR_SHAPE;
    if ((((uintptr_t)a_in | (uintptr_t)whh | (uintptr_t)state_prev) & 15) != 0) return EC_ERR_ARG;
    // pitch H: the two states as stacked dense blocks [2, N, H]; otherwise [h | c] rows
    const float* cprev = ld_prev == H ? state_prev + (size_t)N * H : state_prev + H;
    // (the masked previous states a learn pass keeps beside the gates are the policy's own: not written here)
    ec_lstm_fwd_launch(a_in, whh, bhh, state_prev, cprev, ld_prev, mask, h_out, ld_h, c_out, ld_c, nullptr, 0, gates, nullptr, nullptr, N, H,
                       1, 0, (hipStream_t)stream);
    EC_CHECK_LAUNCH();
    return EC_OK;
}

extern "C" int ec_lstm_step_bwd(const float* dhs, const float* gates, const float* c, const float* c_prev, const float* mask,
                                const float* whh, const float* whhT, const float* da_next, const float* mask_next, float* carry_h,
                                float* carry_c, float* da, int N, int H, ec_stream_t stream) {
    if (!dhs || !gates || !c || !c_prev || !mask || !carry_c || !da) return EC_ERR_ARG;
    if (N <= 0 || !ec_lstm_hidden_ok(H)) return EC_ERR_SHAPE;
    if (whhT) {                                   // fused: back-projection of step t+1 + gates of step t
        if (!da_next || !mask_next) return EC_ERR_ARG;
        if ((H % 256) != 0) return EC_ERR_SHAPE;
        if ((((uintptr_t)da_next | (uintptr_t)whhT) & 15) != 0) return EC_ERR_ARG;
        ec_lstm_bwd_fused_launch(da_next, whhT, mask_next, dhs, carry_c, gates, c, c_prev, mask, da, N, H, (hipStream_t)stream);
        EC_CHECK_LAUNCH();
        return EC_OK;
    }
    if (!whh || !carry_h) return EC_ERR_ARG;
    ec_lstm_bwd_gates_launch(dhs, carry_h, carry_c, gates, c, c_prev, mask, da, N, H, (hipStream_t)stream);
    EC_CHECK_LAUNCH();
    return ec_gemm_f32(da, whh, carry_h, N, H, 4 * H, 4L * H, 1, H, 1, H, EC_GEMM_ACCUMULATE, nullptr, nullptr, nullptr, 0, nullptr, mask, 1,
                       stream);
}
