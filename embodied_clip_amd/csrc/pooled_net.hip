// The pooled-embedding net (habitat-lab's PointNavResNetNet over one pooled CLIP vector per frame; include/ec_amd.h
// ec_policy_create_pooled): the kernels that net has of its own.  policy.hip owns the handle, the plan and the launch order.
//
// Restates (published sources, not under the reference tree: parity unpinned, as for the PointNav goal encoder):
//   [U] habitat_baselines PointNavResNetNet: visual_fc = Sequential(Flatten, Linear(D, hidden), ReLU); tgt_embeding / gps_embedding /
//       compass_embedding = nn.Linear(k, 32); obj_categories_embedding = nn.Embedding(num_goals, 32); prev_action_embedding;
//       x = cat([visual, goal embeddings..., prev action]) -> RNNStateEncoder.
// Every side input reaches the recurrent core through gi = x . weight_ih_l0^T alone, so with W_i' the sensor's column block of
// weight_ih_l0 (ed columns), W_i / b_i the sensor's nn.Linear:
//   SV[:, cols_i] = W_i' W_i [G, k_i]     sb = sum_i W_i' b_i [G]     gi[b] += sb + SV s[b]
// and nothing [B, ed]-shaped exists.  The goal-id table GT and the previous-action table PT are prev_action.hip's.
// No floating-point atomics: every sum below has a fixed order that depends on the shapes alone.
#include "common.h"

namespace {

constexpr size_t POOLED_LDS_LIMIT = 160 * 1024;
constexpr int POOLED_MAX_K = 8;

__device__ __forceinline__ float pooled_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// SV[r, c] (c < K) and sb[r] (c == K): one thread per output, fp32 FMA in ascending j (the embedding's index)
__global__ __launch_bounds__(256) void pooled_tables_kernel(const float* __restrict__ wih, long ld, int col0, const ec_pooled_sensors sn,
                                                            float* __restrict__ sv, float* __restrict__ sb, int G) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const int K1 = sn.K + 1;
    if (t >= (long)G * K1) return;
    const int r = (int)(t / K1), c = (int)(t - (long)r * K1);
    const float* wrow = wih + (long)r * ld + col0;
    if (c == sn.K) {
        float acc = 0.f;
        for (int i = 0; i < sn.ns; ++i)
            for (int j = 0; j < sn.ed; ++j) acc = fmaf(wrow[i * sn.ed + j], sn.b[i][j], acc);
        sb[r] = acc;
        return;
    }
    int i = 0, c0 = 0;
    while (c >= c0 + sn.k[i]) { c0 += sn.k[i]; ++i; }
    const int q = c - c0, ki = sn.k[i];
    float acc = 0.f;
    for (int j = 0; j < sn.ed; ++j) acc = fmaf(wrow[i * sn.ed + j], sn.w[i][j * ki + q], acc);
    sv[(long)r * sn.K + c] = acc;
}

// gi[b, r] = (((gi[b, r] + sb[r]) + gt[goal[b], r]) + pt[row(b), r]) + sum_k sv[r, k] s[b, k]  (k ascending; absent parts skipped;
// an index outside its table adds nothing)
__global__ __launch_bounds__(256) void pooled_rows_add_kernel(float* __restrict__ gi, const ec_pooled_side sd, long B, int G) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= B * G) return;
    const long b = t / G;
    const int r = (int)(t - b * G);
    float v = gi[t];
    if (sd.sb) v += sd.sb[r];
    if (sd.gt) {
        const long long g = sd.goal[b];
        if (g >= 0 && g < sd.num_goals) v += sd.gt[(long)g * G + r];
    }
    if (sd.pt) {
        const int p = ec_pa_index(sd.prev, sd.masks, b, sd.null_token, sd.A);
        if (p >= 0) v += sd.pt[(long)p * G + r];
    }
    if (sd.sv) {
        const float* s = sd.sens + b * sd.K;
        const float* svr = sd.sv + (long)r * sd.K;
        for (int k = 0; k < sd.K; ++k) v = fmaf(svr[k], s[k], v);
    }
    gi[t] = v;
}

// dW_ih[r, blk_i + j] += sum_q dSV[r, c_i + q] W_i[j, q] + dsb[r] b_i[j]: one thread per element of the sensor blocks
__global__ __launch_bounds__(256) void pooled_sensor_dwih_kernel(float* __restrict__ dwih, long ld, int col0, const ec_pooled_sensors sn,
                                                                 const float* __restrict__ dsv, const float* __restrict__ dsb, int G) {
    const int X = sn.ns * sn.ed;
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long)G * X) return;
    const int r = (int)(t / X), x = (int)(t - (long)r * X);
    const int i = x / sn.ed, j = x - i * sn.ed;
    int c0 = 0;
    for (int u = 0; u < i; ++u) c0 += sn.k[u];
    const int ki = sn.k[i];
    float acc = 0.f;
    for (int q = 0; q < ki; ++q) acc = fmaf(dsv[(long)r * sn.K + c0 + q], sn.w[i][j * ki + q], acc);
    acc = fmaf(dsb[r], sn.b[i][j], acc);
    dwih[(long)r * ld + col0 + x] += acc;
}

// dW_i[j, q] += sum_r W_ih[r, blk_i + j] dSV[r, c_i + q] (lane q < k_i) and db_i[j] += sum_r W_ih[r, blk_i + j] dsb[r] (lane k_i):
// one workgroup per (sensor, j); wave w sums the w-th contiguous quarter of r in ascending order, the quarters fold in order
__global__ __launch_bounds__(256) void pooled_sensor_dw_kernel(const float* __restrict__ wih, long ld, int col0, const ec_pooled_sensors sn,
                                                               const float* __restrict__ dsv, const float* __restrict__ dsb, int G) {
    __shared__ float red[4][POOLED_MAX_K + 1];
    const int i = blockIdx.x / sn.ed, j = blockIdx.x - i * sn.ed;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int c0 = 0;
    for (int u = 0; u < i; ++u) c0 += sn.k[u];
    const int ki = sn.k[i];
    const int per = (G + 3) / 4, r0 = w * per, r1 = (r0 + per < G) ? r0 + per : G;
    if (lane <= ki) {
        const float* wcol = wih + col0 + i * sn.ed + j;
        float acc = 0.f;
#pragma unroll 8
        for (int r = r0; r < r1; ++r) acc = fmaf(wcol[(long)r * ld], lane < ki ? dsv[(long)r * sn.K + c0 + lane] : dsb[r], acc);
        red[w][lane] = acc;
    }
    __syncthreads();
    if (w == 0 && lane <= ki) {
        const float v = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
        if (lane < ki) sn.dw[i][j * ki + lane] += v;
        else sn.db[i][j] += v;
    }
}

// (policy.hip's frag_pack_f32_kernel, which that file keeps private; here for the stand-alone entry point too)
// W [N, K] (dense rows) in the fragment order ec_gi_act_body reads: group g of column block cb is the contiguous 1-KB unit
// (cb K/8 + g), lane l's float4 = W[cb 32 + (l & 31)][8 g + 4 (l >> 5) ..]
__global__ __launch_bounds__(256) void pooled_frag_pack_kernel(const float4* __restrict__ W, float4* __restrict__ F, int N, int K) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long)N * K / 4) return;
    const int l = (int)(t & 63);
    const long f = t >> 6;
    const int Gk = K / 8, g = (int)(f % Gk), cb = (int)(f / Gk);
    F[t] = W[((long)(cb * 32 + (l & 31)) * K + g * 8 + 4 * (l >> 5)) >> 2];
}

// visual_fc on the act step: v [N, H] = ReLU(e [N, D] W_fc^T + b).  policy.hip's gi_act_kernel<NW> geometry (the shared body,
// common.h) with the ReLU in the fold: a workgroup owns a 32 x 32 output tile, its NW waves split K = D, operands arrive as
// float4 (W_fc in fragment order) into v_mfma_f32_32x32x2_f32, the partial tiles fold through LDS in wave order.
template <int NW>
__global__ __launch_bounds__(NW * 64) void pooled_fc_act_kernel(const float* __restrict__ e, const float* __restrict__ W,
                                                                const float* __restrict__ bias, float* __restrict__ v, int N, int K,
                                                                int NO) {
    ec_gi_act_body<NW, false, true>(e, W, bias, v, N, K, NO, ec_gi_act_pa{});
}

// Layer 0 of the act step in ONE launch: input projection (v against the dense copy of weight_ih_l0[:, :H]), recurrent
// projection, the side inputs' table rows and the cell.  rnn_stack.hip's rnn_stack_step_kernel -- its geometry (8 units x 3 | 4
// gates per tile, actors n0..n0+31), LDS footprint, two accumulators, x half before h half, states by pitch -- with the x-half
// epilogue  xs = ((((x W_ih^T + b_ih) + sb) + GT[goal]) + PT[row]) + SV s  (k ascending).  Rows past N are never written.
template <bool LSTM>
__global__ __launch_bounds__(256) void pooled_step0_kernel(const ec_rnn_stack_args a, const ec_pooled_side sd) {
    extern __shared__ __attribute__((aligned(16))) float psm[];
    constexpr int NG = LSTM ? 4 : 3;                 // gates; tile columns NG * 8 .. 31 are zero on the GRU
    const int N = a.N, H = a.H;
    const int KC = ((H & 255) == 0) ? 256 : H;
    const int P = KC + 4;
    float* sA = psm;
    float* sB = psm + 32 * P;
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
    for (int half = 0; half < 2; ++half) {
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
    float* part = psm;
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
    const int G = NG * H;
    // the x half's epilogue: bias, then the side inputs' rows in the order of the recurrent input's columns
    const float* gtr = nullptr;
    if (sd.gt) {
        const long long gidx = sd.goal[n];
        if (gidx >= 0 && gidx < sd.num_goals) gtr = sd.gt + (long)gidx * G;
    }
    const float* ptr = nullptr;
    if (sd.pt) {
        const int pr = ec_pa_index(sd.prev, sd.masks, n, sd.null_token, sd.A);
        if (pr >= 0) ptr = sd.pt + (long)pr * G;
    }
    float sv_[POOLED_MAX_K];
#pragma unroll
    for (int k = 0; k < POOLED_MAX_K; ++k) sv_[k] = (sd.sv && k < sd.K) ? sd.sens[(long)n * sd.K + k] : 0.f;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const int col = g * H + j;
        float v = xs[g] + a.bih[col];
        if (sd.sb) v += sd.sb[col];
        if (gtr) v += gtr[col];
        if (ptr) v += ptr[col];
        if (sd.sv) {
            const float* svr = sd.sv + (long)col * sd.K;
#pragma unroll
            for (int k = 0; k < POOLED_MAX_K; ++k)
                if (k < sd.K) v = fmaf(svr[k], sv_[k], v);
        }
        xs[g] = v;
    }
    const float m = a.mask[n];
    const float hp = m * a.hprev[(long)n * a.ld_prev + j];
    float hn;
    if constexpr (LSTM) {
        float act[NG];
#pragma unroll
        for (int g = 0; g < NG; ++g) act[g] = xs[g] + m * hsum[g] + a.bhh[g * H + j];
        const float cp = m * a.cprev[(long)n * a.ld_prev + j];
        const float ig = pooled_sigmoid(act[0]), fg = pooled_sigmoid(act[1]), gg = tanhf(act[2]), og = pooled_sigmoid(act[NG - 1]);
        const float cn = fg * cp + ig * gg;
        hn = og * tanhf(cn);
        a.cout[(long)n * a.ld_c + j] = cn;
    } else {
        const float r = pooled_sigmoid(xs[0] + m * hsum[0] + a.bhh[j]);
        const float z = pooled_sigmoid(xs[1] + m * hsum[1] + a.bhh[H + j]);
        const float hnn = m * hsum[2] + a.bhh[2 * H + j];
        const float nn = tanhf(xs[2] + r * hnn);
        hn = (1.f - z) * nn + z * hp;
    }
    a.hout[(long)n * a.ld_h + j] = hn;
    if (a.hout2) a.hout2[(long)n * a.ld_h2 + j] = hn;
}

template <auto Kernel>
void pooled_allow_big_lds() {
    static std::atomic<uint64_t> done{0};
    if (auto guard = ec_attr_needed(done))
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)POOLED_LDS_LIMIT);
}

}  // namespace

// policy.hip's hooks (declared in common.h): the launches without the argument checks of the C-ABI faces below
void ec_pooled_tables_launch(const float* wih, long ld, int col0, const ec_pooled_sensors& sn, float* sv, float* sb, int G, hipStream_t s) {
    const long total = (long)G * (sn.K + 1);
    hipLaunchKernelGGL(pooled_tables_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, wih, ld, col0, sn, sv, sb, G);
}
void ec_pooled_rows_add_launch(float* gi, const ec_pooled_side& sd, long B, int G, hipStream_t s) {
    const long total = B * G;
    hipLaunchKernelGGL(pooled_rows_add_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, gi, sd, B, G);
}
void ec_pooled_sensor_grads_launch(const float* wih, float* dwih, long ld, int col0, const ec_pooled_sensors& sn, const float* dsv,
                                   const float* dsb, int G, hipStream_t s) {
    const long total = (long)G * sn.ns * sn.ed;
    hipLaunchKernelGGL(pooled_sensor_dwih_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, dwih, ld, col0, sn, dsv, dsb, G);
    hipLaunchKernelGGL(pooled_sensor_dw_kernel, dim3((unsigned)(sn.ns * sn.ed)), dim3(256), 0, s, wih, ld, col0, sn, dsv, dsb, G);
}
void ec_pooled_frag_pack_launch(const float* w, float* wfrag, int N, int K, hipStream_t s) {
    const long nu = (long)N * K / 4;
    hipLaunchKernelGGL(pooled_frag_pack_kernel, dim3((unsigned)((nu + 255) / 256)), dim3(256), 0, s, (const float4*)w, (float4*)wfrag, N, K);
}
void ec_pooled_fc_act_launch(const float* e, const float* wfrag, const float* b, float* v, int N, int D, int H, hipStream_t s) {
    const dim3 grid((unsigned)(H / 32), (unsigned)((N + 31) / 32));
    if (D % 56 == 0) hipLaunchKernelGGL(pooled_fc_act_kernel<7>, grid, dim3(64 * 7), 0, s, e, wfrag, b, v, N, D, H);
    else hipLaunchKernelGGL(pooled_fc_act_kernel<8>, grid, dim3(64 * 8), 0, s, e, wfrag, b, v, N, D, H);
}
void ec_pooled_step0_launch(int lstm, const ec_rnn_stack_args& a, const ec_pooled_side& sd, hipStream_t s) {
    const dim3 grid((unsigned)(a.H / 8), (unsigned)((a.N + 31) / 32));
    const size_t lds = ec_lstm_fwd_lds(a.H);          // the two operand tiles / the 4 partial tiles: the single-layer step's
    if (lstm) {
        pooled_allow_big_lds<pooled_step0_kernel<true>>();
        hipLaunchKernelGGL(pooled_step0_kernel<true>, grid, dim3(256), lds, s, a, sd);
    } else {
        pooled_allow_big_lds<pooled_step0_kernel<false>>();
        hipLaunchKernelGGL(pooled_step0_kernel<false>, grid, dim3(256), lds, s, a, sd);
    }
}

extern "C" int ec_pooled_fc_act(const float* e, const float* w, const float* b, float* wfrag, float* v, int N, int D, int H,
                                ec_stream_t stream) {
    if (!e || !w || !wfrag || !v) return EC_ERR_ARG;
    if (N <= 0 || D <= 0 || H <= 0 || (D % 56 != 0 && D % 64 != 0) || (H % 32) != 0) return EC_ERR_SHAPE;
    if ((((uintptr_t)e | (uintptr_t)w | (uintptr_t)wfrag) & 15) != 0) return EC_ERR_ARG;
    ec_pooled_frag_pack_launch(w, wfrag, H, D, (hipStream_t)stream);
    ec_pooled_fc_act_launch(e, wfrag, b, v, N, D, H, (hipStream_t)stream);
    EC_CHECK_LAUNCH();
    return EC_OK;
}

extern "C" int ec_pooled_step0_fwd(int rnn_type, const float* x, long ld_x, const float* wih, const float* whh, const float* bih,
                                   const float* bhh, const float* sb, const float* gt, const int64_t* goal, int num_goals,
                                   const float* pt, const int64_t* prev_actions, int null_token, int A, const float* sv,
                                   const float* sensors, int K, const float* state_prev, long ld_prev, const float* mask, float* h_out,
                                   long ld_h, float* c_out, long ld_c, float* h_out2, long ld_h2, int N, int H, ec_stream_t stream) {
    if (rnn_type != EC_RNN_GRU && rnn_type != EC_RNN_LSTM) return EC_ERR_ARG;
    const bool lstm = rnn_type == EC_RNN_LSTM;
    if (!x || !wih || !whh || !bih || !bhh || !state_prev || !mask || !h_out || (lstm && !c_out)) return EC_ERR_ARG;
    if ((gt != nullptr) != (goal != nullptr) || (pt != nullptr) != (prev_actions != nullptr) || (sv != nullptr) != (sensors != nullptr))
        return EC_ERR_ARG;
    if (h_out == state_prev) return EC_ERR_ARG;       // in place: a workgroup reads rows of state_prev that another one writes
    if (gt && (num_goals < 1 || num_goals > 256)) return EC_ERR_ARG;
    if (pt && (A < 1 || A > 256 || (null_token != 0 && null_token != 1))) return EC_ERR_ARG;
    if (sv && (K < 1 || K > POOLED_MAX_K)) return EC_ERR_ARG;
    if (N <= 0 || !ec_lstm_hidden_ok(H)) return EC_ERR_SHAPE;
    const long SW = (lstm ? 2L : 1L) * H;
    if (ld_x < H || (ld_x & 3) || ld_prev < SW || (ld_prev & 3) || ld_h < H || (lstm && ld_c < H) || (h_out2 && ld_h2 < H)) return EC_ERR_SHAPE;
    if ((((uintptr_t)x | (uintptr_t)wih | (uintptr_t)whh | (uintptr_t)state_prev) & 15) != 0) return EC_ERR_ARG;
    ec_rnn_stack_args a{};
    a.x = x; a.ld_x = ld_x; a.wih = wih; a.whh = whh; a.bih = bih; a.bhh = bhh;
    a.hprev = state_prev; a.cprev = lstm ? state_prev + H : nullptr; a.ld_prev = ld_prev; a.mask = mask;
    a.hout = h_out; a.ld_h = ld_h; a.cout = lstm ? c_out : nullptr; a.ld_c = ld_c; a.hout2 = h_out2; a.ld_h2 = ld_h2;
    a.gi = nullptr; a.gi_parts = 1; a.gi_pstride = 0; a.N = N; a.H = H;
    const ec_pooled_side sd{sb, gt, (const long long*)goal, num_goals, pt, (const long long*)prev_actions, mask, null_token, A, sv,
                            sensors, sv ? K : 0};
    ec_pooled_step0_launch(lstm ? 1 : 0, a, sd, (hipStream_t)stream);
    EC_CHECK_LAUNCH();
    return EC_OK;
}
