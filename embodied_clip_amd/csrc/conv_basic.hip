// torchvision BasicBlock transition tail (ResNet-18 / 34, first block of layers 2-4) as ONE implicit GEMM:
//
//   out = relu( conv3x3(c1) + conv1x1_stride2(x) + (b2 + bd) )
//
// c1 [B,Ho,Wo,planes] is the block's conv1 output, x [B,2Ho,2Wo,inplanes] its input.  BN is folded into both convs; the two
// weight matrices are laid side by side as W_cat [Cout][9 planes + inplanes] and the two biases summed once, at create time
// (rn50.hip), so the K axis is the concatenation of the nine taps of c1 and the one stride-2 tap of x at (2 yo, 2 xo).  The
// downsample output is never written, there is one launch less per transition block, and the sum is rounded to bf16 once.
//
// Replaces `out = self.bn2(self.conv2(out)); identity = self.downsample(x); out += identity; out = self.relu(out)` of
// [U] torchvision models/resnet.py BasicBlock.forward.
//
// Structure: conv_igemm.hip's 4-wave tile kernel reduced to what this launch needs -- operands global -> LDS directly
// (LDS-DMA, the same 128-B row XOR swizzle), two LDS stages, swapped v_mfma_f32_32x32x16_bf16 operands (a lane owns one
// pixel and 4 consecutive channels per 4 accumulators), bias + ReLU + one bf16 rounding staged through LDS and stored as
// 16-B row chunks.  planes and inplanes are multiples of 64, so a 64-wide K-tile lies either in c1's nine taps or in x: the
// operand source is chosen once per K-tile.
#include "common.h"

namespace {

constexpr int BK = 64;              // K-tile (bf16 elements) = 128-B rows in LDS
constexpr int ROW_BYTES = BK * 2;

struct TailArgs {
    const uint16_t* c1;
    const uint16_t* x;
    const uint16_t* w;
    const float* bias;
    uint16_t* out;
    int Ho, Wo, planes, inplanes, Cout, K1, K, M;
    int ntn;
    unsigned c1_bytes, x_bytes, w_bytes;
};

typedef __attribute__((address_space(3))) void lds_void_t;

__device__ __forceinline__ int lds_off(int row, int chunk) { return row * ROW_BYTES + ((chunk ^ ((row >> 1) & 7)) << 4); }
__device__ __forceinline__ float relu_f(float v) { return __builtin_amdgcn_fmed3f(v, 0.f, __builtin_inff()); }

template <int BM, int BN>
__global__ __launch_bounds__(256, 2) void basic_tail_s2_kernel(TailArgs p) {
    constexpr int WM = 2, WN = 2;
    constexpr int TM = BM / WM, TN = BN / WN, FM = TM / 32, FN = TN / 32;
    constexpr int NT = 256, LR = NT / 8;
    constexpr int A_IT = BM / LR, B_IT = BN / LR;
    constexpr int A_BYTES = BM * ROW_BYTES, B_BYTES = BN * ROW_BYTES;
    static_assert(BM % LR == 0 && BN % LR == 0 && FM >= 1 && FN >= 1, "tile geometry");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int tile = (int)blockIdx.x;
    const int m0 = (tile / p.ntn) * BM, n0 = (tile % p.ntn) * BN;

    // loader geometry: row lrow + LR * i of the tile, source 16-B chunk `chunk` of the 128-B K row (swizzled as conv_igemm)
    const int chunk = (tid & 7) ^ ((tid >> 4) & 7);
    const int lrow = tid >> 3;
    unsigned a_off[A_IT];   // c1: byte offset of the row's output pixel, channel 0
    unsigned x_off[A_IT];   // x: byte offset of input pixel (2 yo, 2 xo), channel 0
    unsigned a_msk[A_IT];   // bit ky*3+kx: that tap of c1 lies inside the frame (0 for rows past M)
    unsigned b_off[B_IT];
    const int HWo = p.Ho * p.Wo;
#pragma unroll
    for (int i = 0; i < A_IT; ++i) {
        const int m = m0 + lrow + LR * i;
        const int b = m / HWo, r = m - b * HWo;
        const int yo = r / p.Wo, xo = r - yo * p.Wo;
        const unsigned xm = (xo > 0 ? 1u : 0u) | 2u | (xo < p.Wo - 1 ? 4u : 0u);
        const unsigned msk = (yo > 0 ? xm : 0u) | (xm << 3) | (yo < p.Ho - 1 ? (xm << 6) : 0u);
        a_msk[i] = m < p.M ? msk : 0u;
        a_off[i] = (unsigned)m * (unsigned)p.planes * 2u;
        x_off[i] = (unsigned)(((long)b * 2 * p.Ho + 2 * yo) * (2 * p.Wo) + 2 * xo) * (unsigned)p.inplanes * 2u;
    }
#pragma unroll
    for (int i = 0; i < B_IT; ++i) b_off[i] = ((unsigned)(n0 + lrow + LR * i) * (unsigned)p.K + chunk * 8) * 2u;

#if defined(__HIP_DEVICE_COMPILE__)
    const __amdgpu_buffer_rsrc_t rs_c1 = __builtin_amdgcn_make_buffer_rsrc((void*)p.c1, 0, p.c1_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc((void*)p.x, 0, p.x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc((void*)p.w, 0, p.w_bytes, 0x00020000);
#endif
    const int wave_lds = wave * 1024;   // 64 lanes x 16 B: LDS-DMA writes are lane-linear from a wave-uniform base
    const int nk = p.K / BK;
    auto load_tile = [&](int kt, int buf) {
        unsigned char* sa = smem + buf * (A_BYTES + B_BYTES) + wave_lds;
        unsigned char* sb = sa + A_BYTES;
        const int k = kt * BK + chunk * 8;
#if defined(__HIP_DEVICE_COMPILE__)
        if (kt * BK < p.K1) {   // one of the nine taps of c1 (stride 1, pad 1)
            const int tap = k / p.planes, ci = k - tap * p.planes;
            const int ky = (tap * 11) >> 5, kx = tap - ky * 3;   // tap / 3, tap % 3 for tap in 0..8
            const int toff = (((ky - 1) * p.Wo + (kx - 1)) * p.planes + ci) * 2;
            const unsigned bit = 1u << tap;
#pragma unroll
            for (int q = 0; q < A_IT; ++q) {
                const unsigned off = (a_msk[q] & bit) ? a_off[q] + (unsigned)toff : 0xFFFFFFF0u;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_c1, (lds_void_t*)(sa + q * (LR * ROW_BYTES)), 16, off, 0, 0, 0);
            }
        } else {                // the stride-2 centre tap of x
            const unsigned ci2 = (unsigned)(k - p.K1) * 2u;
#pragma unroll
            for (int q = 0; q < A_IT; ++q) {
                const unsigned off = (a_msk[q] & 16u) ? x_off[q] + ci2 : 0xFFFFFFF0u;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_x, (lds_void_t*)(sa + q * (LR * ROW_BYTES)), 16, off, 0, 0, 0);
            }
        }
#pragma unroll
        for (int q = 0; q < B_IT; ++q) {
            const unsigned off = b_off[q] + (unsigned)(kt * (BK * 2));
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w, (lds_void_t*)(sb + q * (LR * ROW_BYTES)), 16, off, 0, 0, 0);
        }
#endif
    };

    f32x16_t acc[FM][FN];
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int frow = lane & 31, fhalf = lane >> 5;
    auto compute = [&](int buf) {
        const unsigned char* sa = smem + buf * (A_BYTES + B_BYTES);
        const unsigned char* sb = sa + A_BYTES;
#pragma unroll
        for (int ks = 0; ks < BK / 16; ++ks) {
            s16x8_t af[FM], bfr[FN];
            const int c = ks * 2 + fhalf;
#pragma unroll
            for (int i = 0; i < FM; ++i) af[i] = *reinterpret_cast<const s16x8_t*>(sa + lds_off(wm * TM + i * 32 + frow, c));
#pragma unroll
            for (int j = 0; j < FN; ++j) bfr[j] = *reinterpret_cast<const s16x8_t*>(sb + lds_off(wn * TN + j * 32 + frow, c));
            // swapped operands: D[n][m] -> a lane owns one pixel, 4 consecutive channels per 4 accumulator registers
#pragma unroll
            for (int i = 0; i < FM; ++i)
#pragma unroll
                for (int j = 0; j < FN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, bfr[j]),
                                                                        __builtin_bit_cast(bf16x8_t, af[i]), acc[i][j], 0, 0, 0);
        }
    };

    // two LDS stages: the LDS-DMA of K-tile kt+1 is in flight while kt computes; one barrier per K-tile
    load_tile(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        if (kt + 1 < nk) load_tile(kt + 1, cur ^ 1);
        compute(cur);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }

    // epilogue: + summed bias, ReLU, ONE rounding to bf16 -> LDS image -> 16-B row chunks
    constexpr int PITCH = BN * 2 + 16;
    static_assert(BM * PITCH <= 2 * (A_BYTES + B_BYTES), "epilogue image fits the stages");
#pragma unroll
    for (int j = 0; j < FN; ++j) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int lcol = wn * TN + j * 32 + 8 * g + 4 * fhalf;
            const float4 bv = *reinterpret_cast<const float4*>(p.bias + n0 + lcol);
#pragma unroll
            for (int i = 0; i < FM; ++i) {
                const int lrow_px = wm * TM + i * 32 + frow;
                uint2 o;
                o.x = ec_pack2(relu_f(acc[i][j][4 * g + 0] + bv.x), relu_f(acc[i][j][4 * g + 1] + bv.y));
                o.y = ec_pack2(relu_f(acc[i][j][4 * g + 2] + bv.z), relu_f(acc[i][j][4 * g + 3] + bv.w));
                *reinterpret_cast<uint2*>(smem + lrow_px * PITCH + lcol * 2) = o;
            }
        }
    }
    __syncthreads();
    constexpr int CH = BN / 8, RPP = NT / CH;
    const int srow = tid / CH, schunk = tid % CH;
#pragma unroll
    for (int r0 = 0; r0 < BM; r0 += RPP) {
        const int row = r0 + srow;
        if (m0 + row < p.M)
            *reinterpret_cast<uint4*>(p.out + (long)(m0 + row) * p.Cout + n0 + schunk * 8) =
                *reinterpret_cast<const uint4*>(smem + row * PITCH + schunk * 16);
    }
}

template <int BM, int BN>
int launch_tail(TailArgs p, hipStream_t s) {
    p.ntn = p.Cout / BN;
    const long ntiles = (long)((p.M + BM - 1) / BM) * p.ntn;
    const size_t lds = 2 * (size_t)(BM + BN) * ROW_BYTES;
    auto kern = basic_tail_s2_kernel<BM, BN>;
    static std::atomic<uint64_t> attr_done{0};
    if (auto g = ec_attr_needed(attr_done))
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kern, dim3((unsigned)ntiles), dim3(256), lds, s, p);
    EC_CHECK_LAUNCH();
    return EC_OK;
}

}  // namespace

extern "C" int ec_basic_tail_s2_bf16(const void* c1, const void* x, const void* w_cat, const float* bias_cat, void* out, int B,
                                     int Ho, int Wo, int planes, int inplanes, int Cout, ec_stream_t stream) {
    if (!c1 || !x || !w_cat || !bias_cat || !out) return EC_ERR_ARG;
    if (B <= 0 || Ho <= 0 || Wo <= 0 || Ho >= 2048 || Wo >= 32768) return EC_ERR_SHAPE;
    if (planes < 64 || planes % 64 != 0 || inplanes < 64 || inplanes % 64 != 0 || Cout < 64 || Cout % 64 != 0) return EC_ERR_SHAPE;
    const long M = (long)B * Ho * Wo;
    // 32-bit buffer-descriptor offsets: every operand below 2 GiB
    if (M * planes * 2 >= (1L << 31) || 4 * M * inplanes * 2 >= (1L << 31) || M * Cout * 2 >= (1L << 31)) return EC_ERR_SHAPE;
    TailArgs a;
    a.c1 = (const uint16_t*)c1; a.x = (const uint16_t*)x; a.w = (const uint16_t*)w_cat; a.bias = bias_cat; a.out = (uint16_t*)out;
    a.Ho = Ho; a.Wo = Wo; a.planes = planes; a.inplanes = inplanes; a.Cout = Cout;
    a.K1 = 9 * planes; a.K = a.K1 + inplanes; a.M = (int)M; a.ntn = 0;
    if ((long)Cout * a.K * 2 >= (1L << 31)) return EC_ERR_SHAPE;
    a.c1_bytes = (unsigned)(M * planes * 2);
    a.x_bytes = (unsigned)(4 * M * inplanes * 2);
    a.w_bytes = (unsigned)((long)Cout * a.K * 2);
    hipStream_t s = (hipStream_t)stream;
    // 128 x 128 tiles while they give every CU two; 64 x 64 tiles for the small launches (the 7 x 7 and 14 x 14 maps)
    if (Cout % 128 == 0 && ((M + 127) / 128) * (Cout / 128) >= 512) return launch_tail<128, 128>(a, s);
    return launch_tail<64, 64>(a, s);
}
