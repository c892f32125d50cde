// Stem conv1 on a ONE-channel frame (fp32 [B,H,W] depth -> bf16 NHWC): the depth tower of the RGB-D agent.
//
// Replaces: [U] ClipResNetPreprocessor.process on the depth sensor (readme_files/baselines_habitat.md:75 "replace `rgb`
// with `rgbd`"), which repeats the one-channel frame three times and runs CLIP's first conv-bn-relu on the copy.  Repeating a
// channel is a sum over the input-channel axis of the weights (w9[k][co] = sum_ci w[(k*3+ci)][co], encoder.fold_stem_depth), so
// the kernel reads the 200 KB frame itself: no 602 KB expansion is written or read back.  The sensor's normalisation
// (value = depth * scale + shift) is applied while the patch is staged, so the padding is exactly zero in the NORMALISED
// domain, as in ec_stem_conv1_u8.
#include "common.h"

namespace {

typedef unsigned int u32x4_dep __attribute__((ext_vector_type(4)));

// Same 16 x 16 output tile per workgroup as stem_conv1_kernel; every extent below is the ONE-channel geometry.
constexpr int DT = 16;                 // output tile edge
constexpr int DP = 2 * DT + 1;         // input patch edge (33)
constexpr int DOFF = 3;                // patch rows start three floats early: column 2*ox0 - 4 is a multiple of 4
constexpr int DVEC = 9;                // 16-byte vectors per patch row: columns [2*ox0 - 4, 2*ox0 + 32)
constexpr int DROW = 4 * DVEC;         // floats per patch row (36)
constexpr int DSTG = 32 * 80;          // bytes of one wave's output staging image (32 pixels x 64 B, 80-B pitch)
constexpr int DSMEM = (4 * DSTG > DP * DROW * 4 ? 4 * DSTG : DP * DROW * 4) / 4;   // floats: the patch, then 4 staging images

template <int COUT>
__global__ __launch_bounds__(256) void stem_conv1_depth_kernel(const float* __restrict__ depth, const float* __restrict__ w9,
                                                               const float* __restrict__ bias, uint16_t* __restrict__ out,
                                                               int H, int W, int Ho, int Wo, int tiles_x, int tiles_y,
                                                               float scale, float shift) {
    __shared__ __attribute__((aligned(16))) float patch[DSMEM];
    int bid = blockIdx.x;
    const int tx = bid % tiles_x; bid /= tiles_x;
    const int ty = bid % tiles_y;
    const int b = bid / tiles_y;
    const int oy0 = ty * DT, ox0 = tx * DT;
    const int iy0 = 2 * oy0 - 1, ix0 = 2 * ox0 - 1;
    const long img_off = (long)b * H * W;          // one float per pixel
    const int c0 = ix0 - DOFF;                     // first staged column of a row (multiple of 4)
    // W % 4 == 0 (and a 16-byte aligned frame pointer): a vector is entirely inside or outside the row
    const bool vec = (W & 3) == 0 && (reinterpret_cast<size_t>(depth) & 15) == 0;
    const long frames = (long)gridDim.x / (tiles_x * tiles_y);
    if (vec && frames * H * W * 4 < (1L << 32) - 16) {
        // all of a thread's patch loads in flight before its first LDS store; through a buffer descriptor over the launch's
        // frames ([0, frames*H*W*4) bytes), a vector outside the frame being an out-of-range offset that reads as zeros
#if defined(__HIP_DEVICE_COMPILE__)
        const unsigned nbytes = (unsigned)(frames * H * W * 4);
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)depth, 0, nbytes, 0x00020000);
        constexpr int NV = DP * DVEC, IT = (NV + 255) / 256;
        u32x4_dep raw[IT];
        bool ok_[IT];
#pragma unroll
        for (int i = 0; i < IT; ++i) {
            const int e = min((int)threadIdx.x + 256 * i, NV - 1);
            const int r = e / DVEC, q = e - r * DVEC;
            const int iy = iy0 + r, col = c0 + 4 * q;
            const bool ok = iy >= 0 && iy < H && col >= 0 && col < W;
            ok_[i] = ok;
            // (the last vector of the last row of the last frame ends at byte frames*H*W*4 == nbytes: in range)
            const unsigned off = ok ? (unsigned)((img_off + (long)iy * W + col) * 4) : 0xFFFFFFF0u;
            raw[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)off, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < IT; ++i) {
            const int e = threadIdx.x + 256 * i;
            if (e < NV) {
                const int r = e / DVEC, q = e - r * DVEC;
                const float4 d = __builtin_bit_cast(float4, raw[i]);
                float4 v;   // the affine applies inside the frame only: padding is zero AFTER scale / shift
                v.x = ok_[i] ? d.x * scale + shift : 0.f;
                v.y = ok_[i] ? d.y * scale + shift : 0.f;
                v.z = ok_[i] ? d.z * scale + shift : 0.f;
                v.w = ok_[i] ? d.w * scale + shift : 0.f;
                *reinterpret_cast<float4*>(patch + r * DROW + 4 * q) = v;
            }
        }
#endif
    } else if (vec) {
        for (int e = threadIdx.x; e < DP * DVEC; e += 256) {
            const int r = e / DVEC, q = e - r * DVEC;
            const int iy = iy0 + r, col = c0 + 4 * q;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (iy >= 0 && iy < H && col >= 0 && col < W) {
                const float4 d = *reinterpret_cast<const float4*>(depth + img_off + (long)iy * W + col);
                v = make_float4(d.x * scale + shift, d.y * scale + shift, d.z * scale + shift, d.w * scale + shift);
            }
            *reinterpret_cast<float4*>(patch + r * DROW + 4 * q) = v;
        }
    } else {
        for (int e = threadIdx.x; e < DP * DP; e += 256) {
            const int r = e / DP, c = e - r * DP;
            const int iy = iy0 + r, ix = ix0 + c;
            float v = 0.f;
            if (iy >= 0 && iy < H && ix >= 0 && ix < W) v = depth[img_off + (long)iy * W + ix] * scale + shift;
            patch[r * DROW + c + DOFF] = v;   // same image as the vector path: column ix0 + c sits at c + DOFF
        }
    }
    __syncthreads();
    if constexpr (COUT % 32 == 0) {
        // ---- MFMA route: the 3x3 window is a K = 9 (-> 16) contraction, ONE v_mfma_f32_32x32x16_bf16 per 32 pixels x 32
        // channels (the RGB kernel's K = 27 -> 32 takes two).  Lane (px, h) holds k = 8 h + e: taps 0..7 in the h = 0 half,
        // tap 8 and seven zeros in the other.  Window values and weights are rounded to bf16 where stem_conv1_kernel rounds
        // them; swapped operands (D[channel][pixel]) and the wave-private output image as there.
        constexpr int FN = COUT / 32;
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, px = lane & 31, h = lane >> 5;
        int koff[8];
        bool kval[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int k = 8 * h + e;
            kval[e] = k < 9;
            koff[e] = kval[e] ? (k / 3) * DROW + (k % 3) : 0;
        }
        s16x8_t wf[FN];
#pragma unroll
        for (int j = 0; j < FN; ++j) {
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = kval[e] ? w9[(8 * h + e) * COUT + 32 * j + px] : 0.f;
            const u32x4_dep pk = {ec_pack2(v[0], v[1]), ec_pack2(v[2], v[3]), ec_pack2(v[4], v[5]), ec_pack2(v[6], v[7])};
            wf[j] = __builtin_bit_cast(s16x8_t, pk);
        }
        s16x8_t af[2];
#pragma unroll
        for (int b2 = 0; b2 < 2; ++b2) {
            const int p_ = (wave * 2 + b2) * 32 + px;              // pixel of the 16 x 16 tile this lane gathers for
            const int ly = p_ >> 4, lx = p_ & 15;
            const float* win = patch + (2 * ly) * DROW + 2 * lx + DOFF;
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = kval[e] ? win[koff[e]] : 0.f;
            const u32x4_dep pk = {ec_pack2(v[0], v[1]), ec_pack2(v[2], v[3]), ec_pack2(v[4], v[5]), ec_pack2(v[6], v[7])};
            af[b2] = __builtin_bit_cast(s16x8_t, pk);
        }
        __syncthreads();                                           // every wave has gathered: the LDS becomes 4 staging images
        unsigned char* stg = reinterpret_cast<unsigned char*>(patch) + wave * DSTG;
#pragma unroll
        for (int b2 = 0; b2 < 2; ++b2) {
#pragma unroll
            for (int j = 0; j < FN; ++j) {
                f32x16_t acc;
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = 0.f;
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, wf[j]), __builtin_bit_cast(bf16x8_t, af[b2]), acc, 0, 0, 0);
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const float4 bv = *reinterpret_cast<const float4*>(bias + 32 * j + 8 * g + 4 * h);
                    uint2 o;
                    o.x = ec_pack2(fmaxf(acc[4 * g + 0] + bv.x, 0.f), fmaxf(acc[4 * g + 1] + bv.y, 0.f));
                    o.y = ec_pack2(fmaxf(acc[4 * g + 2] + bv.z, 0.f), fmaxf(acc[4 * g + 3] + bv.w, 0.f));
                    *reinterpret_cast<uint2*>(stg + px * 80 + (8 * g + 4 * h) * 2) = o;
                }
#pragma unroll
                for (int i = 0; i < 2; ++i) {                      // (same wave wrote it: LDS is in order per wave)
                    const int c = lane + 64 * i, q = c >> 2, part = c & 3;
                    const int p2 = (wave * 2 + b2) * 32 + q;
                    const int oy = oy0 + (p2 >> 4), ox = ox0 + (p2 & 15);
                    const u32x4_dep v = *reinterpret_cast<const u32x4_dep*>(stg + q * 80 + part * 16);
                    if (oy < Ho && ox < Wo)
                        *reinterpret_cast<u32x4_dep*>(out + ((long)(b * Ho + oy) * Wo + ox) * COUT + 32 * j + part * 8) = v;
                }
            }
        }
        return;
    }
    // ---- fp32 route (COUT = 48): packed fp32 FMAs, one output pixel and all channels per lane, wave-uniform weights
    const int ly = threadIdx.x / DT, lx = threadIdx.x % DT;
    const int oy = oy0 + ly, ox = ox0 + lx;
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    f32x2 acc2[COUT / 2];
#pragma unroll
    for (int c = 0; c < COUT / 2; ++c) acc2[c] = *reinterpret_cast<const f32x2*>(bias + 2 * c);
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const float v = patch[(2 * ly + ky) * DROW + 2 * lx + kx + DOFF];
            const f32x2 v2 = {v, v};
            const f32x2* wr = reinterpret_cast<const f32x2*>(w9 + (ky * 3 + kx) * COUT);
#pragma unroll
            for (int c = 0; c < COUT / 2; ++c) acc2[c] = __builtin_elementwise_fma(v2, wr[c], acc2[c]);
        }
    if (oy < Ho && ox < Wo) {
        uint4* dst = reinterpret_cast<uint4*>(out + ((long)(b * Ho + oy) * Wo + ox) * COUT);
#pragma unroll
        for (int c = 0; c < COUT / 2; c += 4) {
            uint4 v;
            v.x = ec_pack2(fmaxf(acc2[c + 0][0], 0.f), fmaxf(acc2[c + 0][1], 0.f));
            v.y = ec_pack2(fmaxf(acc2[c + 1][0], 0.f), fmaxf(acc2[c + 1][1], 0.f));
            v.z = ec_pack2(fmaxf(acc2[c + 2][0], 0.f), fmaxf(acc2[c + 2][1], 0.f));
            v.w = ec_pack2(fmaxf(acc2[c + 3][0], 0.f), fmaxf(acc2[c + 3][1], 0.f));
            dst[c / 4] = v;
        }
    }
}

}  // namespace

extern "C" int ec_stem_conv1_depth(const float* depth, float scale, float shift, const float* w9, const float* bias, void* out,
                                   int B, int H, int W, int Cout, ec_stream_t stream) {
    if (!depth || !w9 || !bias || !out) return EC_ERR_ARG;
    if (B <= 0 || H < 2 || W < 2) return EC_ERR_SHAPE;
    if (Cout != 32 && Cout != 48 && Cout != 64) return EC_ERR_SHAPE;
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const int tx = (Wo + DT - 1) / DT, ty = (Ho + DT - 1) / DT;
    if ((long)B * tx * ty > 0x7fffffffL) return EC_ERR_SHAPE;
    dim3 grid((unsigned)(B * tx * ty));
    hipStream_t s = (hipStream_t)stream;
    uint16_t* o = (uint16_t*)out;
    if (Cout == 32)
        hipLaunchKernelGGL((stem_conv1_depth_kernel<32>), grid, dim3(256), 0, s, depth, w9, bias, o, H, W, Ho, Wo, tx, ty, scale, shift);
    else if (Cout == 48)
        hipLaunchKernelGGL((stem_conv1_depth_kernel<48>), grid, dim3(256), 0, s, depth, w9, bias, o, H, W, Ho, Wo, tx, ty, scale, shift);
    else   // RN50x16: 48 real channels zero-padded to the 32-channel granule of the conv kernels
        hipLaunchKernelGGL((stem_conv1_depth_kernel<64>), grid, dim3(256), 0, s, depth, w9, bias, o, H, W, Ho, Wo, tx, ty, scale, shift);
    EC_CHECK_LAUNCH();
    return EC_OK;
}
