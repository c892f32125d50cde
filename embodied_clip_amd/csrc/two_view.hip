// The two-view rearrangement net's front (include/ec_amd.h ec_policy_create_two_view): an attention-pooled, TRAINABLE encoder over
// two frozen CLIP maps per frame -- the current view u and the goal-state view w from the same pose.  policy.hip owns the handle,
// the plan and the launch order; everything behind the pooled vector v is the pooled-embedding net's.
//
// Restates (published sources, not under the reference tree: parity unpinned):
//   [U] ai2thor-rearrangement ResNetRearrangeActorCriticRNN: concat_img = cat([u, w, u * w], channel);
//       visual_encoder = Sequential(Conv2d(3C, H, 1), ReLU); visual_attention = Sequential(Conv2d(3C, 32, 1), ReLU, Conv2d(32, 1, 1));
//       probs = softmax(attention.view(B, -1)); x = (encoder * probs).mean(-1).mean(-1)   (a MEAN over the S2 pixels, not a sum)
// Per frame, with c_p = [u_p | w_p | u_p * w_p] (K = 3C):
//   e_p = ReLU(W_e c_p + b_e)   m_p = ReLU(W_a c_p + b_a)   l_p = <w_2, m_p> + b_2   a = softmax_p(l)   v = (1 / S2) sum_p a_p e_p
//
// Forward (tv_fwd_kernel).  Both convs read the same operand, so K is walked ONCE against the combined [A1 + H, 3C] weight
// (attention rows first), kept as three bf16 planes in MFMA-fragment order (tv_pack_kernel).  [u | w | u*w] never exists in
// memory: a workgroup stages 64 channels of u and w, forms the product while staging -- the fp32 product of two bf16 values has 16
// significant bits and splits EXACTLY into two bf16 planes -- and the operand is 4C bf16 columns (u, w, hi, lo) against the weight
// planes; lo x plane 2 (2^-24 of the product) is not multiplied.  A workgroup owns whole frames: FG = 32 RT / S2 frames in RT
// 32-row tiles (RT = 5: 3 frames of 49 rows in 160, 91.9 % useful rows; RT = 2 for launches of few frames: 1 frame in 64, 76.6 %),
// and up to 8 column tiles (4 waves x 2): the attention tiles, which every column chunk of a frame group recomputes, and its share
// of the encoder tiles.  The epilogue goes through LDS: bias + ReLU, the w_2 dot in ascending column order, one thread per frame
// for the softmax (maximum subtracted), then (frame, column) threads for the weighted mean in ascending pixel order.  Nothing
// depends on which frames share a workgroup: a frame's v has the same bits however the frames are sliced.
//
// Backward (tv_bwd_rows_kernel, tv_dw_kernel, folds).  From dv, the stored probabilities a and the stored post-ReLU activations:
//   s_p = <e_p, dv> / S2   dl_p = a_p (s_p - sum_q a_q s_q)   de_p = (a_p / S2) dv [e_p > 0]   dm_p = dl_p w_2 [m_p > 0]
// The rows kernel (one workgroup per frame) leaves the two row scalars (a_p / S2, dl_p) and the frame's share of the bias gradients,
// of dw_2 and of db_2; two ordered folds add the frames up.  The weight gradient contracts over all B S2 pixels, the SLOW index of
// both operands: tv_dw_kernel rebuilds dY from the row scalars and the sign of the stored activations (it is rank one per frame and
// never stored), splits it into three bf16 planes, and turns both operands in registers -- a thread loads eight consecutive pixel
// rows of one column and writes them as one 16-byte K-contiguous fragment piece.  The product columns are built on the fly as in
// the forward.  The pixel range is cut into splits whose partial tiles a last launch folds in order.
// No floating-point atomics: every sum has a fixed order that depends on the shapes alone.
#include <algorithm>

#include "common.h"

namespace {

constexpr int TV_KC = 64;                       // channels of u / w per staged chunk
constexpr int TV_PITCH = TV_KC + 8;             // bf16 elements per LDS row: 144 B, an odd number of 16-byte slots
constexpr int TV_EP = 33;                       // floats per row of an epilogue tile
constexpr size_t TV_LDS_LIMIT = 160 * 1024;

template <int RT>
constexpr size_t tv_fwd_lds() {
    constexpr size_t stage = (size_t)4 * 32 * RT * TV_PITCH * 2, epi = ((size_t)4 * 32 * RT * TV_EP + 2 * 32 * RT) * 4;
    return stage > epi ? stage : epi;
}

__device__ __forceinline__ bf16x8_t tv_frag(const uint4 v) { return __builtin_bit_cast(bf16x8_t, v); }

// hi + lo == x * y exactly for bf16-valued x, y (pairs packed as ec_pack2 packs them)
__device__ __forceinline__ void tv_prod2(uint32_t x, uint32_t y, uint32_t& hi, uint32_t& lo) {
    const float p0 = ec_lo(x) * ec_lo(y), p1 = ec_hi(x) * ec_hi(y);
    hi = ec_pack2(p0, p1);
    lo = ec_pack2(p0 - ec_lo(hi), p1 - ec_hi(hi));
}

// [W_a; W_e] (row n < A1: W_a[n], else W_e[n - A1]; K = 3C) as three bf16 planes in the order tv_fwd_kernel reads: the 1-KB unit
// ((ct KB + kb) 3 + plane) holds, for lane l, W[ct 32 + (l & 31)][kb 16 + 8 (l >> 5) ..+8]
__global__ __launch_bounds__(256) void tv_pack_kernel(const float* __restrict__ We, const float* __restrict__ Wa, uint4* __restrict__ wp,
                                                      int H, int A1, int C) {
    const int K3 = 3 * C, KB = K3 / 16;
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long)((H + A1) / 32) * KB * 64) return;
    const int lane = (int)(t & 63);
    const long f = t >> 6;
    const int kb = (int)(f % KB), ct = (int)(f / KB);
    const int n = ct * 32 + (lane & 31);
    const float* src = (n < A1 ? Wa + (long)n * K3 : We + (long)(n - A1) * K3) + kb * 16 + (lane >> 5) * 8;
    const float4 q0 = *reinterpret_cast<const float4*>(src), q1 = *reinterpret_cast<const float4*>(src + 4);
    const float x0[4] = {q0.x, q0.y, q0.z, q0.w}, x1[4] = {q1.x, q1.y, q1.z, q1.w};
    uint2 a0, a1, a2, b0, b1, b2;
    ec_split3x4(x0, a0, a1, a2);
    ec_split3x4(x1, b0, b1, b2);
    uint4* dst = wp + f * 3 * 64 + lane;
    dst[0] = make_uint4(a0.x, a0.y, b0.x, b0.y);
    dst[64] = make_uint4(a1.x, a1.y, b1.x, b1.y);
    dst[128] = make_uint4(a2.x, a2.y, b2.x, b2.y);
}

// grid (frame groups of FG frames, column chunks of TEC encoder tiles); 4 waves; see the header
template <int RT>
__global__ __launch_bounds__(256) void tv_fwd_kernel(const ec_tv_fwd_args p, int FG, int TEC) {
    extern __shared__ __attribute__((aligned(16))) unsigned char tsm[];
    constexpr int M = 32 * RT, PL = M * TV_PITCH * 2, NP = (M * 8 + 255) / 256;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i32 = lane & 31, hh = lane >> 5;
    const int S2 = p.S2, C = p.C, A1 = p.A1, H = p.H, NT = H + A1, TA = A1 / 32, KB = 3 * C / 16;
    const long f0 = (long)blockIdx.x * FG;
    const int nf = (int)(p.B - f0 < FG ? p.B - f0 : FG), nrows = nf * S2;
    const int e0 = blockIdx.y * TEC, te = (H / 32 - e0 < TEC) ? H / 32 - e0 : TEC, ntl = TA + te;
    bool on[2];
    int ct[2];
#pragma unroll
    for (int sl = 0; sl < 2; ++sl) {
        const int t = sl * 4 + wave;
        on[sl] = t < ntl;
        ct[sl] = !on[sl] ? 0 : (t < TA ? t : e0 + t);          // (encoder tile e0 + (t - TA) is combined tile TA + e0 + t - TA)
    }
    f32x16_t acc[2][RT];
#pragma unroll
    for (int sl = 0; sl < 2; ++sl)
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[sl][rt][r] = 0.f;

    // staging: piece idx = (row, 8 channels); rows past the group's frames are zeros
    const uint16_t* ug = p.u + f0 * S2 * C;
    const uint16_t* wg = p.w + f0 * S2 * C;
    uint4 ru[NP], rw[NP];
    auto fetch = [&](int kc) {
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int idx = tid + i * 256, r = idx >> 3, c8 = idx & 7;
            ru[i] = make_uint4(0u, 0u, 0u, 0u);
            rw[i] = ru[i];
            if (r < nrows) {
                const long o = (long)r * C + kc + c8 * 8;
                ru[i] = *reinterpret_cast<const uint4*>(ug + o);
                rw[i] = *reinterpret_cast<const uint4*>(wg + o);
            }
        }
    };
    fetch(0);
    for (int kc = 0; kc < C; kc += TV_KC) {
        __syncthreads();                                        // every wave is done reading the previous chunk
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int idx = tid + i * 256, r = idx >> 3, c8 = idx & 7;
            if (idx < M * 8) {
                uint4 hi, lo;
                tv_prod2(ru[i].x, rw[i].x, hi.x, lo.x);
                tv_prod2(ru[i].y, rw[i].y, hi.y, lo.y);
                tv_prod2(ru[i].z, rw[i].z, hi.z, lo.z);
                tv_prod2(ru[i].w, rw[i].w, hi.w, lo.w);
                unsigned char* d = tsm + (r * TV_PITCH + c8 * 8) * 2;
                *reinterpret_cast<uint4*>(d) = ru[i];
                *reinterpret_cast<uint4*>(d + PL) = rw[i];
                *reinterpret_cast<uint4*>(d + 2 * PL) = hi;
                *reinterpret_cast<uint4*>(d + 3 * PL) = lo;
            }
        }
        __syncthreads();
        if (kc + TV_KC < C) fetch(kc + TV_KC);                  // the next chunk's rows travel under this chunk's MFMAs
#pragma unroll
        for (int ks = 0; ks < TV_KC / 16; ++ks) {
            const int kbu = (kc >> 4) + ks;
            uint4 bu[2][3], bw[2][3], bp[2][3];
#pragma unroll
            for (int sl = 0; sl < 2; ++sl) {
                if (on[sl]) {
                    const uint4* base = reinterpret_cast<const uint4*>(p.wp) + (long)ct[sl] * KB * 3 * 64 + lane;
#pragma unroll
                    for (int pl = 0; pl < 3; ++pl) {
                        bu[sl][pl] = base[((long)kbu * 3 + pl) * 64];
                        bw[sl][pl] = base[((long)(kbu + C / 16) * 3 + pl) * 64];
                        bp[sl][pl] = base[((long)(kbu + 2 * (C / 16)) * 3 + pl) * 64];
                    }
                }
            }
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                const unsigned char* a = tsm + ((rt * 32 + i32) * TV_PITCH + ks * 16 + hh * 8) * 2;
                const bf16x8_t aU = tv_frag(*reinterpret_cast<const uint4*>(a)), aW = tv_frag(*reinterpret_cast<const uint4*>(a + PL));
                const bf16x8_t aH = tv_frag(*reinterpret_cast<const uint4*>(a + 2 * PL)), aL = tv_frag(*reinterpret_cast<const uint4*>(a + 3 * PL));
#pragma unroll
                for (int sl = 0; sl < 2; ++sl) {
                    if (on[sl]) {                               // (wave-uniform) smallest terms first
                        f32x16_t c = acc[sl][rt];
                        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(aL, tv_frag(bp[sl][1]), c, 0, 0, 0);
                        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(aL, tv_frag(bp[sl][0]), c, 0, 0, 0);
#pragma unroll
                        for (int pl = 2; pl >= 0; --pl) {
                            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(aH, tv_frag(bp[sl][pl]), c, 0, 0, 0);
                            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(aW, tv_frag(bw[sl][pl]), c, 0, 0, 0);
                            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(aU, tv_frag(bu[sl][pl]), c, 0, 0, 0);
                        }
                        acc[sl][rt] = c;
                    }
                }
            }
        }
    }

    // ---- epilogue: the operand planes are dead, LDS becomes the 4 waves' [M x 32] tiles, the logits and the probabilities ----
    float* sE = reinterpret_cast<float*>(tsm);
    float* sLg = sE + 4 * M * TV_EP;
    float* sA = sLg + M;
    const bool first = blockIdx.y == 0;                         // the column chunk that stores what every chunk computes
    const float inv = 1.f / (float)S2;
#pragma unroll
    for (int sl = 0; sl < 2; ++sl) {
        __syncthreads();
        if (on[sl]) {
            const int n = ct[sl] * 32 + i32;
            const float bias = n < A1 ? p.ba[n] : p.be[n - A1];
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = rt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;   // C/D layout of the 32x32 MFMA, column = lane & 31
                    sE[(wave * M + row) * TV_EP + i32] = fmaxf(acc[sl][rt][r] + bias, 0.f);
                }
        }
        __syncthreads();
        if (p.act) {                                            // the post-ReLU activations, for the backward
            for (int wv = 0; wv < 4; ++wv) {
                const int t = sl * 4 + wv;
                if (t >= ntl || (t < TA && !first)) continue;
                const int n0 = (t < TA ? t : e0 + t) * 32;
                for (int idx = tid; idx < nrows * 32; idx += 256) {
                    const int row = idx >> 5, c = idx & 31;
                    p.act[(f0 * S2 + row) * NT + n0 + c] = sE[(wv * M + row) * TV_EP + c];
                }
            }
        }
        if (sl == 0) {
            // l_p = <w_2, m_p> + b_2 in ascending column order (attention tile t is wave t's tile of this pass)
            for (int r = tid; r < nrows; r += 256) {
                float l = 0.f;
                for (int t = 0; t < TA; ++t)
                    for (int c = 0; c < 32; ++c) l = fmaf(sE[(t * M + r) * TV_EP + c], p.w2[t * 32 + c], l);
                sLg[r] = l + p.b2[0];
            }
            __syncthreads();
            for (int f = tid; f < nf; f += 256) {               // one thread per frame: softmax over its S2 pixels
                const float* l = sLg + f * S2;
                float mx = l[0];
                for (int q = 1; q < S2; ++q) mx = fmaxf(mx, l[q]);
                float se = 0.f;
                for (int q = 0; q < S2; ++q) se += expf(l[q] - mx);
                for (int q = 0; q < S2; ++q) {
                    const float a = expf(l[q] - mx) / se;
                    sA[f * S2 + q] = a;
                    if (p.a && first) p.a[(f0 + f) * S2 + q] = a;
                }
            }
            __syncthreads();
        }
        for (int wv = 0; wv < 4; ++wv) {                        // v = (1 / S2) sum_p a_p e_p, ascending p
            const int t = sl * 4 + wv;
            if (t < TA || t >= ntl) continue;
            const int c0 = (e0 + t - TA) * 32;
            for (int idx = tid; idx < nf * 32; idx += 256) {
                const int f = idx >> 5, c = idx & 31;
                const float* e = sE + (wv * M + f * S2) * TV_EP + c;
                const float* a = sA + f * S2;
                float s = 0.f;
                for (int q = 0; q < S2; ++q) s = fmaf(a[q], e[q * TV_EP], s);
                p.v[(f0 + f) * H + c0 + c] = s * inv;
            }
        }
    }
}

// ---- backward ----
// per-frame vector fp[b]: [ db (A1 + H: attention bias, then encoder bias) | dw_2 (A1) | db_2 (1) ]
__host__ __device__ inline int tv_fcols(int H, int A1) { return H + 2 * A1 + 1; }

// one workgroup per frame: the row scalars rowc[row] = (a_p / S2, dl_p) and the frame's vector fp[b]
__global__ __launch_bounds__(256) void tv_bwd_rows_kernel(const float* __restrict__ act, const float* __restrict__ a,
                                                          const float* __restrict__ dv, const float* __restrict__ w2,
                                                          float* __restrict__ rowc, float* __restrict__ fp, int S2, int H, int A1) {
    __shared__ float ss[64], sdl[64], sac[64], st;
    const long b = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, NT = H + A1;
    const float* actb = act + b * S2 * NT;
    const float* dvb = dv + b * H;
    const float inv = 1.f / (float)S2;
    for (int q = wave; q < S2; q += 4) {                        // s_q: lane l sums columns l, l + 64, ... ascending, then a fixed butterfly
        const float* e = actb + (long)q * NT + A1;
        float s = 0.f;
        for (int n = lane; n < H; n += 64) s = fmaf(e[n], dvb[n], s);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (lane == 0) ss[q] = s * inv;
    }
    __syncthreads();
    if (tid == 0) {
        float t = 0.f;
        for (int q = 0; q < S2; ++q) t = fmaf(a[b * S2 + q], ss[q], t);
        st = t;
    }
    __syncthreads();
    if (tid < S2) {
        const float aq = a[b * S2 + tid], dl = aq * (ss[tid] - st), ac = aq * inv;
        sdl[tid] = dl;
        sac[tid] = ac;
        rowc[(b * S2 + tid) * 2] = ac;
        rowc[(b * S2 + tid) * 2 + 1] = dl;
    }
    __syncthreads();
    const int F = tv_fcols(H, A1);
    for (int n = tid; n < F; n += 256) {                        // column sums over the frame's pixels, ascending
        float s = 0.f;
        if (n < A1) {
            const float wn = w2[n];
            for (int q = 0; q < S2; ++q) s += actb[(long)q * NT + n] > 0.f ? sdl[q] * wn : 0.f;
        } else if (n < NT) {
            const float dn = dvb[n - A1];
            for (int q = 0; q < S2; ++q) s += actb[(long)q * NT + n] > 0.f ? sac[q] * dn : 0.f;
        } else if (n < NT + A1) {
            for (int q = 0; q < S2; ++q) s = fmaf(sdl[q], actb[(long)q * NT + n - NT], s);
        } else {
            for (int q = 0; q < S2; ++q) s += sdl[q];
        }
        fp[b * F + n] = s;
    }
}

// out[blk][n] = sum over the block's rows of in[row][n], ascending
__global__ __launch_bounds__(256) void tv_fold_rows_kernel(const float* __restrict__ in, float* __restrict__ out, long rows, int F, int per) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= F) return;
    const long r0 = (long)blockIdx.y * per, r1 = r0 + per < rows ? r0 + per : rows;
    float s = 0.f;
    for (long r = r0; r < r1; ++r) s += in[r * F + n];
    out[(long)blockIdx.y * F + n] = s;
}
// ... and the blocks, ascending, onto the four small gradients
__global__ __launch_bounds__(256) void tv_fold_out_kernel(const float* __restrict__ part, int nblk, float* __restrict__ dbe,
                                                          float* __restrict__ dba, float* __restrict__ dw2, float* __restrict__ db2, int H,
                                                          int A1) {
    const int n = blockIdx.x * 256 + threadIdx.x, F = tv_fcols(H, A1), NT = H + A1;
    if (n >= F) return;
    float s = 0.f;
    for (int k = 0; k < nblk; ++k) s += part[(long)k * F + n];
    if (n < A1) dba[n] += s;
    else if (n < NT) dbe[n - A1] += s;
    else if (n < NT + A1) dw2[n - NT] += s;
    else db2[0] += s;
}

struct TvDwArgs {
    const uint16_t *u, *w;
    const float *act, *rowc, *dv, *w2;
    float* part;              // [nsplit][A1 + H][3C]
    long M, rows_per_split;   // pixels; a multiple of 32
    int S2, C, H, A1;
};
constexpr int TV_DP = 40;     // bf16 elements per LDS row of the transposed tiles: 80 B, an odd number of 16-byte slots

// grid (C / 64 channel blocks, groups of four 32-row tiles of [A1 + H], pixel splits); wave w owns row tile 4 y + w and the six
// 32-column tiles (u, w, u*w: two each) of its channel block; see the header
__global__ __launch_bounds__(256) void tv_dw_kernel(const TvDwArgs p) {
    __shared__ __attribute__((aligned(16))) uint16_t sY[3][128][TV_DP];
    __shared__ __attribute__((aligned(16))) uint16_t sX[4][64][TV_DP];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i32 = lane & 31, hh = lane >> 5;
    const int S2 = p.S2, C = p.C, H = p.H, A1 = p.A1, NT = H + A1;
    const int cb = blockIdx.x, n0 = blockIdx.y * 128, sp = blockIdx.z;
    const bool active = n0 + wave * 32 < NT;
    const long row0 = (long)sp * p.rows_per_split, row1 = (row0 + p.rows_per_split < p.M) ? row0 + p.rows_per_split : p.M;
    f32x16_t acc[6];
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
    const int xch = tid & 63, xo = tid >> 6;
    for (long kt = row0; kt < row1; kt += 32) {
        __syncthreads();                                        // every wave is done reading the previous tile
        {   // X: channel xch, pixel rows kt + 8 xo ..+8 as one K-contiguous piece of each of the four planes
            uint32_t pu[4], pw[4], ph[4], plo[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                uint32_t xu[2], xw[2];
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const long row = kt + xo * 8 + 2 * j + e;
                    xu[e] = 0u; xw[e] = 0u;
                    if (row < row1) {
                        const long o = row * C + cb * 64 + xch;
                        xu[e] = p.u[o];
                        xw[e] = p.w[o];
                    }
                }
                pu[j] = xu[0] | (xu[1] << 16);
                pw[j] = xw[0] | (xw[1] << 16);
                tv_prod2(pu[j], pw[j], ph[j], plo[j]);
            }
            *reinterpret_cast<uint4*>(&sX[0][xch][xo * 8]) = make_uint4(pu[0], pu[1], pu[2], pu[3]);
            *reinterpret_cast<uint4*>(&sX[1][xch][xo * 8]) = make_uint4(pw[0], pw[1], pw[2], pw[3]);
            *reinterpret_cast<uint4*>(&sX[2][xch][xo * 8]) = make_uint4(ph[0], ph[1], ph[2], ph[3]);
            *reinterpret_cast<uint4*>(&sX[3][xch][xo * 8]) = make_uint4(plo[0], plo[1], plo[2], plo[3]);
        }
#pragma unroll
        for (int it = 0; it < 2; ++it) {   // dY: column n, pixel rows kt + 8 o ..+8, rebuilt from the row scalars and the activation's sign
            const int item = tid + it * 256, nl = item & 127, o = item >> 7, n = n0 + nl;
            if (n < NT) {
                float y[8];
                const float wn = n < A1 ? p.w2[n] : 0.f;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const long row = kt + o * 8 + j;
                    y[j] = 0.f;
                    if (row < row1 && p.act[row * NT + n] > 0.f)
                        y[j] = n < A1 ? p.rowc[row * 2 + 1] * wn : p.rowc[row * 2] * p.dv[(row / S2) * H + n - A1];
                }
                const float y0[4] = {y[0], y[1], y[2], y[3]}, y1[4] = {y[4], y[5], y[6], y[7]};
                uint2 a0, a1, a2, b0, b1, b2;
                ec_split3x4(y0, a0, a1, a2);
                ec_split3x4(y1, b0, b1, b2);
                *reinterpret_cast<uint4*>(&sY[0][nl][o * 8]) = make_uint4(a0.x, a0.y, b0.x, b0.y);
                *reinterpret_cast<uint4*>(&sY[1][nl][o * 8]) = make_uint4(a1.x, a1.y, b1.x, b1.y);
                *reinterpret_cast<uint4*>(&sY[2][nl][o * 8]) = make_uint4(a2.x, a2.y, b2.x, b2.y);
            }
        }
        __syncthreads();
        if (active) {
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const int ko = ks * 16 + hh * 8;
                bf16x8_t ya[3];
#pragma unroll
                for (int pl = 0; pl < 3; ++pl) ya[pl] = tv_frag(*reinterpret_cast<const uint4*>(&sY[pl][wave * 32 + i32][ko]));
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const bf16x8_t bU = tv_frag(*reinterpret_cast<const uint4*>(&sX[0][j * 32 + i32][ko]));
                    const bf16x8_t bW = tv_frag(*reinterpret_cast<const uint4*>(&sX[1][j * 32 + i32][ko]));
                    const bf16x8_t bH = tv_frag(*reinterpret_cast<const uint4*>(&sX[2][j * 32 + i32][ko]));
                    const bf16x8_t bL = tv_frag(*reinterpret_cast<const uint4*>(&sX[3][j * 32 + i32][ko]));
                    acc[4 + j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ya[1], bL, acc[4 + j], 0, 0, 0);
                    acc[4 + j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ya[0], bL, acc[4 + j], 0, 0, 0);
#pragma unroll
                    for (int pl = 2; pl >= 0; --pl) {           // smallest plane first
                        acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ya[pl], bU, acc[j], 0, 0, 0);
                        acc[2 + j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ya[pl], bW, acc[2 + j], 0, 0, 0);
                        acc[4 + j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ya[pl], bH, acc[4 + j], 0, 0, 0);
                    }
                }
            }
        }
    }
    if (!active) return;
    float* out = p.part + (long)sp * NT * 3 * C;
#pragma unroll
    for (int s = 0; s < 3; ++s)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int n = n0 + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
                out[(long)n * 3 * C + (long)s * C + cb * 64 + j * 32 + i32] = acc[2 * s + j][r];
            }
}

// dW_a / dW_e += the splits' partial tiles, in split order
__global__ __launch_bounds__(256) void tv_dw_fold_kernel(const float* __restrict__ part, int nsplit, long n4, long a4, float* __restrict__ dWa,
                                                         float* __restrict__ dWe) {
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    if (q >= n4) return;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k = 0; k < nsplit; ++k) {
        const float4 v = *reinterpret_cast<const float4*>(part + ((long)k * n4 + q) * 4);
        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    float* dst = q < a4 ? dWa + q * 4 : dWe + (q - a4) * 4;
    float4 d = *reinterpret_cast<float4*>(dst);
    d.x += s.x; d.y += s.y; d.z += s.z; d.w += s.w;
    *reinterpret_cast<float4*>(dst) = d;
}

constexpr int TV_FOLD_ROWS = 128;   // frames per block of the first fold

int tv_dw_splits(long M, int C, int NT) {
    const long base = (long)(C / 64) * ((NT / 32 + 3) / 4), ktiles = (M + 31) / 32;
    long ns = (512 + base - 1) / base;
    if (ns > 16) ns = 16;
    if (ns > ktiles) ns = ktiles;
    return (int)(ns < 1 ? 1 : ns);
}
long tv_fold_blocks(long B) { return (B + TV_FOLD_ROWS - 1) / TV_FOLD_ROWS; }
size_t tv_al(size_t floats) { return (floats + 63) / 64 * 64; }

template <auto Kernel>
void tv_allow_big_lds() {
    static std::atomic<uint64_t> done{0};
    if (auto guard = ec_attr_needed(done))
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)TV_LDS_LIMIT);
}

template <int RT>
void tv_fwd_launch_rt(const ec_tv_fwd_args& a, hipStream_t s) {
    const int FG = std::max(1, 32 * RT / a.S2), TA = a.A1 / 32, TE = a.H / 32;
    const int ny = (TE + (8 - TA) - 1) / (8 - TA), TEC = (TE + ny - 1) / ny;
    tv_allow_big_lds<tv_fwd_kernel<RT>>();
    hipLaunchKernelGGL(tv_fwd_kernel<RT>, dim3((unsigned)((a.B + FG - 1) / FG), (unsigned)ny), dim3(256), tv_fwd_lds<RT>(), s, a, FG, TEC);
}

}  // namespace

// policy.hip's hooks (declared in common.h): the launches without the argument checks of the C-ABI faces below
bool ec_tv_shape_ok(const ec_tv_shape& q) {
    return q.B > 0 && q.C >= 64 && q.C <= 4096 && q.C % 64 == 0 && q.S2 >= 1 && q.S2 <= 64 && ec_lstm_hidden_ok(q.H) && q.A1 >= 32 &&
           q.A1 <= 128 && q.A1 % 32 == 0 && q.B <= 0x7fffffffL / 64;       // (row counts and grids stay within 32 bits)
}
size_t ec_tv_planes_floats(const ec_tv_shape& q) { return tv_al((size_t)(q.H + q.A1) * 3 * q.C * 3 / 2); }
size_t ec_tv_bwd_scratch_floats(const ec_tv_shape& q) {
    const size_t F = (size_t)tv_fcols(q.H, q.A1), NT = (size_t)q.H + q.A1;
    return tv_al((size_t)q.B * q.S2 * 2) + tv_al((size_t)q.B * F) + tv_al((size_t)tv_fold_blocks(q.B) * F) +
           tv_al((size_t)tv_dw_splits(q.B * q.S2, q.C, (int)NT) * NT * 3 * q.C);
}
void ec_tv_pack_launch(const float* We, const float* Wa, void* planes, const ec_tv_shape& q, hipStream_t s) {
    const long n = (long)((q.H + q.A1) / 32) * (3 * q.C / 16) * 64;
    hipLaunchKernelGGL(tv_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, We, Wa, (uint4*)planes, q.H, q.A1, q.C);
}
void ec_tv_fwd_launch(const ec_tv_fwd_args& a, hipStream_t s) {
    // five-tile groups once they give every CU a workgroup; below that one frame group per 64 rows, for the act step's few frames
    const int FG5 = std::max(1, 160 / a.S2), TA = a.A1 / 32, TE = a.H / 32, ny = (TE + (8 - TA) - 1) / (8 - TA);
    if (((a.B + FG5 - 1) / FG5) * ny >= 256) tv_fwd_launch_rt<5>(a, s);
    else tv_fwd_launch_rt<2>(a, s);
}
void ec_tv_bwd_launch(const void* u, const void* w, const float* w2, const float* dv, const float* a, const float* act, float* scratch,
                      float* dWe, float* dbe, float* dWa, float* dba, float* dw2, float* db2, const ec_tv_shape& q, hipStream_t s) {
    const int H = q.H, A1 = q.A1, NT = H + A1, F = tv_fcols(H, A1);
    const long M = q.B * q.S2;
    float* rowc = scratch;
    float* fp = rowc + tv_al((size_t)M * 2);
    float* part1 = fp + tv_al((size_t)q.B * F);
    float* dwp = part1 + tv_al((size_t)tv_fold_blocks(q.B) * F);
    hipLaunchKernelGGL(tv_bwd_rows_kernel, dim3((unsigned)q.B), dim3(256), 0, s, act, a, dv, w2, rowc, fp, q.S2, H, A1);
    const int nblk = (int)tv_fold_blocks(q.B);
    hipLaunchKernelGGL(tv_fold_rows_kernel, dim3((unsigned)((F + 255) / 256), (unsigned)nblk), dim3(256), 0, s, fp, part1, q.B, F, TV_FOLD_ROWS);
    hipLaunchKernelGGL(tv_fold_out_kernel, dim3((unsigned)((F + 255) / 256)), dim3(256), 0, s, part1, nblk, dbe, dba, dw2, db2, H, A1);
    TvDwArgs d;
    d.u = (const uint16_t*)u; d.w = (const uint16_t*)w; d.act = act; d.rowc = rowc; d.dv = dv; d.w2 = w2; d.part = dwp;
    d.M = M; d.S2 = q.S2; d.C = q.C; d.H = H; d.A1 = A1;
    const int ns = tv_dw_splits(M, q.C, NT);
    d.rows_per_split = (((M + ns - 1) / ns) + 31) / 32 * 32;
    hipLaunchKernelGGL(tv_dw_kernel, dim3((unsigned)(q.C / 64), (unsigned)((NT / 32 + 3) / 4), (unsigned)ns), dim3(256), 0, s, d);
    const long n4 = (long)NT * 3 * q.C / 4, a4 = (long)A1 * 3 * q.C / 4;
    hipLaunchKernelGGL(tv_dw_fold_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, dwp, ns, n4, a4, dWa, dWe);
}

// ---- C-ABI: the two kernels alone (tests/test_gpu_two_view_kernels.py, tools/bench_two_view.py) ----
namespace {
struct TvWs { size_t wp, a, act, scr, end; };
TvWs tv_ws(const ec_tv_shape& q, bool bwd) {
    TvWs w; size_t o = 0;
    auto take = [&](size_t n) { size_t r = o; o += tv_al(n); return r; };
    w.wp = take(ec_tv_planes_floats(q));
    w.a = take((size_t)q.B * q.S2);
    w.act = take(bwd ? (size_t)q.B * q.S2 * (q.H + q.A1) : 0);
    w.scr = take(bwd ? ec_tv_bwd_scratch_floats(q) : 0);
    w.end = o;
    return w;
}
}  // namespace

extern "C" size_t ec_two_view_workspace_bytes(long B, int S2, int C, int H, int A1, int for_backward) {
    const ec_tv_shape q{B, S2, C, H, A1};
    if (!ec_tv_shape_ok(q)) return 0;
    return tv_ws(q, for_backward != 0).end * 4;
}

extern "C" int ec_two_view_fwd(const void* u, const void* w, const float* We, const float* be, const float* Wa, const float* ba,
                               const float* w2, const float* b2, float* v, long B, int S2, int C, int H, int A1, void* workspace,
                               size_t ws_bytes, int save, ec_stream_t stream) {
    if (!u || !w || !We || !be || !Wa || !ba || !w2 || !b2 || !v || !workspace) return EC_ERR_ARG;
    const ec_tv_shape q{B, S2, C, H, A1};
    if (!ec_tv_shape_ok(q)) return EC_ERR_SHAPE;
    if ((((uintptr_t)u | (uintptr_t)w | (uintptr_t)We | (uintptr_t)Wa | (uintptr_t)workspace) & 15) != 0) return EC_ERR_ARG;
    const TvWs l = tv_ws(q, save != 0);
    if (ws_bytes < l.end * 4) return EC_ERR_WORKSPACE;
    float* ws = (float*)workspace;
    ec_tv_pack_launch(We, Wa, ws + l.wp, q, (hipStream_t)stream);
    const ec_tv_fwd_args a{(const uint16_t*)u, (const uint16_t*)w, ws + l.wp, be, ba, w2, b2, v, ws + l.a, save ? ws + l.act : nullptr,
                           B, S2, C, H, A1};
    ec_tv_fwd_launch(a, (hipStream_t)stream);
    EC_CHECK_LAUNCH();
    return EC_OK;
}

extern "C" int ec_two_view_bwd(const void* u, const void* w, const float* w2, const float* dv, float* dWe, float* dbe, float* dWa,
                               float* dba, float* dw2, float* db2, long B, int S2, int C, int H, int A1, void* workspace,
                               size_t ws_bytes, ec_stream_t stream) {
    if (!u || !w || !w2 || !dv || !dWe || !dbe || !dWa || !dba || !dw2 || !db2 || !workspace) return EC_ERR_ARG;
    const ec_tv_shape q{B, S2, C, H, A1};
    if (!ec_tv_shape_ok(q)) return EC_ERR_SHAPE;
    if ((((uintptr_t)u | (uintptr_t)w | (uintptr_t)dWe | (uintptr_t)dWa | (uintptr_t)workspace) & 15) != 0) return EC_ERR_ARG;
    const TvWs l = tv_ws(q, true);
    if (ws_bytes < l.end * 4) return EC_ERR_WORKSPACE;
    float* ws = (float*)workspace;
    ec_tv_bwd_launch(u, w, w2, dv, ws + l.a, ws + l.act, ws + l.scr, dWe, dbe, dWa, dba, dw2, db2, q, (hipStream_t)stream);
    EC_CHECK_LAUNCH();
    return EC_OK;
}

// ---- the plugin class's bridge: both views' fp32 NCHW maps -> bf16 pixel-major rows -------------------------------------------------
// AllenAct hands ResNetRearrangeActorCriticRNN two fp32 [B, C, HW] tensors per call; the kernels above read bf16 [B, HW, C].  This is
// nchw_to_nhwc_bf16_kernel (stem_elementwise.hip: one workgroup per frame and 64-channel slab, a [HW][65] float tile, 4-byte loads,
// 2-byte stores, atomicOr on the flag) for TWO tensors in ONE launch (blockIdx.y = the view), run on every act step: the values
// are rounded to nearest even, and *changed is SET (never cleared: the caller reads it when it can afford to) when one of them
// was not a bf16 value already.  Both sides move 16 bytes per lane:
//   in   the slab's [64][HW] floats are one contiguous 16-byte aligned run: float4 loads, lane after lane;
//   LDS  float tile [64][P], P = HW | 1.  Odd HW (7 x 7, 3 x 3, 1 x 1 maps): P == HW, the tile IS the run, and a float4 goes in as
//        one 16-byte store.  Even HW: one pad column and four ds_write_b32 per lane (addresses 4 words apart across lanes: 4-way
//        on the 32 store banks, which costs a store 2 x -- the price of the odd pitch the reads need, paid by the even maps only);
//   out  lane l -> (pixel hw, 8-channel piece j) with j = (l & 3) + 4 * (l >> 5) and hw = 8 * group + ((l >> 2) & 7): its eight
//        ds_read_b32 hit word (8 j + k) P + hw.  Within a 32-lane half j takes four values, 8 j P mod 32 is {0, 8, 16, 24} in
//        some order because P is odd, and hw eight consecutive ones: 32 distinct banks for every k.  The wave then stores eight
//        pixels' 128-byte runs of the row-major output, each as 8 x 16 bytes.
// The flag is a plain store of the constant 1 by lane 0 of a wave that saw such a value: every writer stores the same word.
namespace {

constexpr int PR_TC = 64;     // channels per slab

__global__ __launch_bounds__(256) void nchw_pair_to_nhwc_bf16_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                    uint16_t* __restrict__ out_a, uint16_t* __restrict__ out_b,
                                                                    int HW, int C, int P, int* changed) {
    extern __shared__ __attribute__((aligned(16))) float ptile[];   // [PR_TC][P]
    const int slabs = C / PR_TC;
    const long frame = blockIdx.x / slabs;
    const int c0 = (int)(blockIdx.x % slabs) * PR_TC;
    const float* src = (blockIdx.y ? b : a) + (frame * C + c0) * HW;
    uint16_t* dst = (blockIdx.y ? out_b : out_a) + frame * HW * C + c0;
    const float4* src4 = reinterpret_cast<const float4*>(src);
    const int n4 = (PR_TC / 4) * HW;
    int bad = 0;
    auto off_grid = [](float v) -> int { return ((__float_as_uint(v) & 0xffffu) != 0u) && (v == v); };   // (NaNs are left to the consumer)
    for (int i = threadIdx.x; i < n4; i += 256) {
        const float4 v = src4[i];
        bad |= off_grid(v.x) | off_grid(v.y) | off_grid(v.z) | off_grid(v.w);
        if (P == HW) {
            reinterpret_cast<float4*>(ptile)[i] = v;
        } else {
            const float x[4] = {v.x, v.y, v.z, v.w};
            int c = (4 * i) / HW, hw = 4 * i - c * HW;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                ptile[c * P + hw] = x[k];
                if (++hw == HW) { hw = 0; ++c; }
            }
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, j = (lane & 3) + 4 * (lane >> 5);
    for (int hw = 8 * (threadIdx.x >> 6) + ((lane >> 2) & 7); hw < HW; hw += 32) {
        const float* t = ptile + 8 * j * P + hw;
        uint4 o;
        o.x = ec_pack2(t[0], t[P]);
        o.y = ec_pack2(t[2 * P], t[3 * P]);
        o.z = ec_pack2(t[4 * P], t[5 * P]);
        o.w = ec_pack2(t[6 * P], t[7 * P]);
        *reinterpret_cast<uint4*>(dst + (long)hw * C + 8 * j) = o;
    }
    if (__builtin_amdgcn_ballot_w64(bad != 0) != 0 && lane == 0) *changed = 1;
}

}  // namespace

extern "C" int ec_nchw_f32_pair_to_nhwc_bf16(const float* a, const float* b, void* out_a, void* out_b, long B, int HW, int C,
                                             int* changed, ec_stream_t stream) {
    if (!a || !b || !out_a || !out_b || !changed) return EC_ERR_ARG;
    if ((((uintptr_t)a | (uintptr_t)b | (uintptr_t)out_a | (uintptr_t)out_b | (uintptr_t)changed) & 15) != 0) return EC_ERR_ARG;
    if (B <= 0 || HW < 1 || HW > 64 || C <= 0 || C % PR_TC != 0) return EC_ERR_SHAPE;
    if (B > 0x7fffffffL) return EC_ERR_SHAPE;
    const long blocks = B * (long)(C / PR_TC);
    if (blocks > 0x7fffffffL) return EC_ERR_SHAPE;      // (one workgroup per frame and slab in grid.x)
    const int P = HW | 1;
    hipLaunchKernelGGL(nchw_pair_to_nhwc_bf16_kernel, dim3((unsigned)blocks, 2), dim3(256), (size_t)PR_TC * P * sizeof(float),
                       (hipStream_t)stream, a, b, (uint16_t*)out_a, (uint16_t*)out_b, HW, C, P, changed);
    EC_CHECK_LAUNCH();
    return EC_OK;
}
