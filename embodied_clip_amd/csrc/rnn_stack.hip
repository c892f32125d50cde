// Upper layers of a multi-layer recurrent core (torch.nn.GRU / torch.nn.LSTM with num_layers = L, dropout = 0, under the
// RNNStateEncoder episode mask): ONE launch per layer per act step -- the input projection W_ih x, the recurrent projection
// W_hh h_prev and the cell together -- instead of a GEMM launch and a step launch that depend on each other.
//
// Layer l >= 1 at step t takes x = h^{l-1}_t.  The mask multiplies the previous state of the layer, never its input:
//   GRU   r = s((x W_ir^T + b_ir) + m (h W_hr^T) + b_hr);  z likewise;  hn = m (h W_hn^T) + b_hn
//         n = tanh((x W_in^T + b_in) + r hn);  h' = (1 - z) n + z (m h)
//   LSTM  a = (x W_ih^T + b_ih) + m (h W_hh^T) + b_hh   (gate order i, f, g, o);  c' = f (m c) + i g;  h' = o tanh(c')
// The geometry is that of lstm_step_fwd_kernel / gru_step_fwd_kernel: workgroup (blockIdx.x, blockIdx.y) owns hidden units
// j0..j0+7 of actors n0..n0+31, the 8 units x 3 | 4 gates are columns of a v_mfma_f32_32x32x2_f32 tile (the GRU zero-fills 8).
//   * TWO accumulators per wave: one for the x half (against W_ih rows), one for the h_prev half (against W_hh rows).  The GRU
//     needs them apart (its n gate), and apart the mask multiplies the recurrent contraction only (exact for m in {0, 1});
//   * the halves are walked as separate K chunks through the SAME two LDS tiles (row pitch KC + 4 floats): KC = 256 through
//     LDS-DMA when H % 256 == 0, one plain-staged chunk per half otherwise -- the single-layer kernels' footprint (66.5 KB at
//     most when chunked);
//   * the four waves' partial tiles are summed through LDS in a fixed order, the x part before the h part, each through the
//     same 16-KB area: an actor's result does not depend on how the actors are sliced.  No atomics;
//   * h (and c) go to the caller's state row by pitch, and optionally a second, dense copy of h for the heads.  The next layer
//     reads the state row through its x pitch: no copy launch follows.  Rows past N are never written.
// `gi` non-null (layer 0 of a GRU stack on the act step): the x half is not contracted; gi [N, G] (+ split-K parts, folded in
// order) already holds W_ih x + b_ih -- the single-layer GRU step with row pitches on both states.
#include "common.h"

namespace {

constexpr size_t STACK_LDS_LIMIT = 160 * 1024;

__device__ __forceinline__ float stack_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

template <bool LSTM>
__global__ __launch_bounds__(256) void rnn_stack_step_kernel(const ec_rnn_stack_args a) {
    extern __shared__ __attribute__((aligned(16))) float ssm[];
    constexpr int NG = LSTM ? 4 : 3;                 // gates; tile columns NG * 8 .. 31 are zero on the GRU
    const int N = a.N, H = a.H;
    const int KC = ((H & 255) == 0) ? 256 : H;
    const int P = KC + 4;
    float* sA = ssm;
    float* sB = ssm + 32 * P;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j0 = blockIdx.x * 8, n0 = blockIdx.y * 32;
    const int i = lane & 31, hh = lane >> 5;
    f32x16_t accx, acch;
#pragma unroll
    for (int r = 0; r < 16; ++r) { accx[r] = 0.f; acch[r] = 0.f; }
    if (!LSTM && KC == 256) {                                           // W rows 24..31 of the B tile: zeros, once
        for (int idx = tid; idx < 8 * 64; idx += 256) {
            const int r = 24 + (idx >> 6), c4 = idx & 63;
            *reinterpret_cast<float4*>(sB + r * P + c4 * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    bool first = true;
    for (int half = a.gi ? 1 : 0; half < 2; ++half) {
        const float* A = half ? a.hprev : a.x;                          // the operand rows of this half and their pitch
        const long lda = half ? a.ld_prev : a.ld_x;
        const float* Wm = half ? a.whh : a.wih;
        f32x16_t acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        for (int k0 = 0; k0 < H; k0 += KC) {
            if (!first) __syncthreads();                                // every wave is done reading the previous chunk
            first = false;
            if (KC == 256) {
                // LDS-DMA staging: one 1-KiB piece per tile row (256 floats); the rows round-robin over the 4 waves
                typedef __attribute__((address_space(3))) void lds_v;
                typedef const __attribute__((address_space(1))) void gbl_v;
                const int uwave = __builtin_amdgcn_readfirstlane(wave);
                for (int r = uwave; r < 32 + NG * 8; r += 4) {
                    const float* src;
                    float* dst;
                    if (r < 32) {
                        const int n = min(n0 + r, N - 1);               // rows past N are never read back
                        src = A + (long)n * lda + k0 + lane * 4;
                        dst = sA + r * P;
                    } else {
                        const int c = r - 32;                           // tile column c = gate (c >> 3), unit j0 + (c & 7)
                        src = Wm + ((long)(c >> 3) * H + j0 + (c & 7)) * H + k0 + lane * 4;
                        dst = sB + c * P;
                    }
                    __builtin_amdgcn_global_load_lds((gbl_v*)src, (lds_v*)dst, 16, 0, 0);
                }
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            } else {
                const int q4 = H >> 2;
                for (int idx = tid; idx < 32 * q4; idx += 256) {
                    const int r = idx / q4, c4 = idx - r * q4;
                    float4 av = make_float4(0.f, 0.f, 0.f, 0.f), bv = av;
                    const int n = n0 + r;
                    if (n < N) av = *reinterpret_cast<const float4*>(A + (long)n * lda + c4 * 4);
                    if (r < NG * 8) bv = *reinterpret_cast<const float4*>(Wm + ((long)(r >> 3) * H + j0 + (r & 7)) * H + c4 * 4);
                    *reinterpret_cast<float4*>(sA + r * P + c4 * 4) = av;
                    *reinterpret_cast<float4*>(sB + r * P + c4 * 4) = bv;
                }
            }
            __syncthreads();
            const int kq = KC >> 2;
            const float* pa = sA + i * P + wave * kq + 4 * hh;
            const float* pb = sB + i * P + wave * kq + 4 * hh;
            for (int kb = 0; kb < kq; kb += 8) {
                const float4 av = *reinterpret_cast<const float4*>(pa + kb);
                const float4 bv = *reinterpret_cast<const float4*>(pb + kb);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv.x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv.y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bv.z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bv.w, acc, 0, 0, 0);
            }
        }
        if (half) acch = acc; else accx = acc;
    }
    // the operand tiles are dead: LDS becomes the 4 partial [32 x 32] tiles, of the x half first, then of the h half
    float* part = ssm;
    const int a_ = tid >> 3, u = tid & 7;
    const int n = n0 + a_, j = j0 + u;
    float xs[NG], hsum[NG];
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * hh;     // actor (C/D layout of the 32x32 MFMA), column = lane & 31
            part[(wave * 32 + row) * 32 + i] = half ? acch[r] : accx[r];
        }
        __syncthreads();
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const int c = g * 8 + u;
            const float v = ((part[(0 * 32 + a_) * 32 + c] + part[(1 * 32 + a_) * 32 + c]) + part[(2 * 32 + a_) * 32 + c]) +
                            part[(3 * 32 + a_) * 32 + c];
            if (half) hsum[g] = v; else xs[g] = v;
        }
    }
    if (n >= N) return;
    if (a.gi) {                                                          // the input projection as given: split-K parts in order
        const float* gir = a.gi + (long)n * NG * H;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            float v = gir[g * H + j];
            for (int p2 = 1; p2 < a.gi_parts; ++p2) v += gir[p2 * a.gi_pstride + g * H + j];
            xs[g] = v;
        }
    } else {
#pragma unroll
        for (int g = 0; g < NG; ++g) xs[g] += a.bih[g * H + j];
    }
    const float m = a.mask[n];
    const float hp = m * a.hprev[(long)n * a.ld_prev + j];
    float hn;
    if constexpr (LSTM) {
        float act[NG];
#pragma unroll
        for (int g = 0; g < NG; ++g) act[g] = xs[g] + m * hsum[g] + a.bhh[g * H + j];
        const float cp = m * a.cprev[(long)n * a.ld_prev + j];
        const float ig = stack_sigmoid(act[0]), fg = stack_sigmoid(act[1]), gg = tanhf(act[2]), og = stack_sigmoid(act[NG - 1]);
        const float cn = fg * cp + ig * gg;
        hn = og * tanhf(cn);
        a.cout[(long)n * a.ld_c + j] = cn;
    } else {
        const float r = stack_sigmoid(xs[0] + m * hsum[0] + a.bhh[j]);
        const float z = stack_sigmoid(xs[1] + m * hsum[1] + a.bhh[H + j]);
        const float hnn = m * hsum[2] + a.bhh[2 * H + j];
        const float nn = tanhf(xs[2] + r * hnn);
        hn = (1.f - z) * nn + z * hp;
    }
    a.hout[(long)n * a.ld_h + j] = hn;
    if (a.hout2) a.hout2[(long)n * a.ld_h2 + j] = hn;
}

template <auto Kernel>
void stack_allow_big_lds() {
    static std::atomic<uint64_t> done{0};
    if (auto guard = ec_attr_needed(done))
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)STACK_LDS_LIMIT);
}

}  // namespace

// policy.hip's hook (declared in common.h): the launch without the argument checks of the C-ABI face below
void ec_rnn_stack_launch(int lstm, const ec_rnn_stack_args& a, hipStream_t s) {
    const dim3 grid((unsigned)(a.H / 8), (unsigned)((a.N + 31) / 32));
    const size_t lds = ec_lstm_fwd_lds(a.H);          // the two operand tiles / the 4 partial tiles: the single-layer step's
    if (lstm) {
        stack_allow_big_lds<rnn_stack_step_kernel<true>>();
        hipLaunchKernelGGL(rnn_stack_step_kernel<true>, grid, dim3(256), lds, s, a);
    } else {
        stack_allow_big_lds<rnn_stack_step_kernel<false>>();
        hipLaunchKernelGGL(rnn_stack_step_kernel<false>, grid, dim3(256), lds, s, a);
    }
}

extern "C" int ec_rnn_stack_step_fwd(int rnn_type, const float* x, long ld_x, const float* wih, const float* whh, const float* bih,
                                     const float* bhh, const float* state_prev, long ld_prev, const float* mask, float* h_out, long ld_h,
                                     float* c_out, long ld_c, float* h_out2, long ld_h2, int N, int H, ec_stream_t stream) {
    if (rnn_type != EC_RNN_GRU && rnn_type != EC_RNN_LSTM) return EC_ERR_ARG;
    const bool lstm = rnn_type == EC_RNN_LSTM;
    if (!x || !wih || !whh || !bih || !bhh || !state_prev || !mask || !h_out || (lstm && !c_out)) return EC_ERR_ARG;
    if (N <= 0 || !ec_lstm_hidden_ok(H)) return EC_ERR_SHAPE;
    const long SW = (lstm ? 2L : 1L) * H;
    if (ld_x < H || (ld_x & 3) || ld_prev < SW || (ld_prev & 3) || ld_h < H || (lstm && ld_c < H) || (h_out2 && ld_h2 < H)) return EC_ERR_SHAPE;
    if ((((uintptr_t)x | (uintptr_t)wih | (uintptr_t)whh | (uintptr_t)state_prev) & 15) != 0) return EC_ERR_ARG;
    ec_rnn_stack_args a{};
    a.x = x; a.ld_x = ld_x; a.wih = wih; a.whh = whh; a.bih = bih; a.bhh = bhh;
    a.hprev = state_prev; a.cprev = lstm ? state_prev + H : nullptr; a.ld_prev = ld_prev; a.mask = mask;
    a.hout = h_out; a.ld_h = ld_h; a.cout = lstm ? c_out : nullptr; a.ld_c = ld_c; a.hout2 = h_out2; a.ld_h2 = ld_h2;
    a.gi = nullptr; a.gi_parts = 1; a.gi_pstride = 0; a.N = N; a.H = H;
    ec_rnn_stack_launch(lstm ? 1 : 0, a, (hipStream_t)stream);
    EC_CHECK_LAUNCH();
    return EC_OK;
}
