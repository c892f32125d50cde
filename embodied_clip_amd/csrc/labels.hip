// Probe labels from the simulator's semantic-segmentation frame: object presence and 3 x 3 localisation.
//
// Replaces the numpy labelling of primitive_probing/generate_data/thor_image_features.py:71-88,115-127
// (`class_mask` per target class = all three channels equal the class colour, `obj_presence` = any pixel of the mask,
// over the whole frame and over the nine `grid_bboxes` cells).  The reference builds C full-frame boolean masks per
// frame on the host; here every semantic frame is read ONCE and nothing but the labels is written.
//
// Shape of the launch:
//   * a frame is cut into its three cell rows (rows [floor(i*H/3), floor((i+1)*H/3)), a contiguous byte range) and
//     each of those into up to 8 slices of whole image rows; one workgroup of 256 threads per (frame, slice).  A
//     slice lies inside one cell row, so a workgroup owns three cells and keeps three class sets;
//   * a class set is a 64-bit mask (C <= 64 == the wave size).  Lane c of every wave holds class c's packed 24-bit
//     colour, so "which classes have colour k" is ONE `__ballot(table == k)`: the ballot's bit c is class c.  Two
//     classes with one colour both fire, a class without a colour holds a key no pixel can have;
//   * a lane takes 4 pixels = 12 bytes = 3 dwords per pass from a pixel index that is a multiple of 4 counted from the
//     frame's first pixel (the next pass's loads are issued before this pass's work).  The wave then resolves each
//     DISTINCT colour among its 256 pixels once: first unresolved key -> v_readlane -> ballot -> every lane takes the
//     set for each of its pixels with that key.  Semantic frames are flat regions: one turn for a wave inside a
//     region, a handful where a row of the image crosses object borders.  No per-class loop anywhere;
//   * the three sets are OR-reduced over the wave with shuffles, over the workgroup's waves through LDS, and unpacked:
//     thread c stores a 1 for each of the three cells class c was seen in, and a 1 in `presence` (the nine cells tile
//     the frame, so presence == OR over cells, thor_image_features.py:122).  The outputs are zeroed on the stream
//     before the launch; several slices may store the same 1, which needs no atomic and has one possible result.
// Frames whose bytes are not 4-byte aligned (odd H*W, e.g. 301 x 299) and the ragged ends of a slice are read bytewise.
#include "common.h"

namespace {

constexpr int NT = 256;                 // threads per workgroup
constexpr int MAX_SLICES = 8;           // slices per cell row
constexpr int SLICE_PIXELS = 4 * NT * 4;   // aim: four passes per workgroup
constexpr uint32_t KEY_NONE = 0xFFFFFFFFu;   // class without a colour / lane >= C: equals no 24-bit key
constexpr uint32_t KEY_OUTSIDE = 0xFFFFFFFEu;   // pixel outside the slice

__device__ __forceinline__ uint32_t key_at(const unsigned char* p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
}

__device__ __forceinline__ uint64_t wave_or(uint64_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v |= __shfl_xor(v, off, EC_WAVE);
    return v;
}

// Class sets of a lane's four keys.  Each turn takes the first unresolved key of the first lane that has one, asks
// every lane's table entry about it (the ballot IS the class set) and resolves that key in all four slots of all lanes:
// one turn per DISTINCT colour among the wave's 256 pixels (one for a flat region).  Wave-uniform control flow: the
// ballots need every lane.
__device__ __forceinline__ void classes_of(const uint32_t (&k)[4], uint32_t table, uint64_t (&set)[4]) {
    uint32_t pend = 0xFu;
    set[0] = set[1] = set[2] = set[3] = 0;
    for (;;) {
        const uint64_t lanes = __ballot(pend != 0);
        if (!lanes) break;
        const int l = __ffsll((unsigned long long)lanes) - 1;
        const uint32_t cur = (pend & 1u) ? k[0] : (pend & 2u) ? k[1] : (pend & 4u) ? k[2] : k[3];
        const uint32_t key = (uint32_t)__builtin_amdgcn_readlane((int)cur, l);
        const uint64_t classes = __ballot(table == key);
        for (int q = 0; q < 4; ++q)
            if (k[q] == key) {
                set[q] = classes;
                pend &= ~(1u << q);
            }
    }
}

__global__ __launch_bounds__(NT) void semantic_labels_kernel(const unsigned char* __restrict__ sem,
                                                             const unsigned char* __restrict__ colors,
                                                             long long* __restrict__ presence,
                                                             long long* __restrict__ localization, int H, int W, int C,
                                                             int slices) {
    __shared__ unsigned long long sets[3];
    const int b = blockIdx.y;
    const int i = blockIdx.x / slices, s = blockIdx.x - i * slices;
    const int ya = (i * H) / 3, yb = ((i + 1) * H) / 3;
    const int rows = (yb - ya + slices - 1) / slices;
    const int r0 = ya + s * rows, r1 = min(r0 + rows, yb);
    if (r0 >= r1) return;                                            // whole workgroup: this slice holds no row
    const int x1 = W / 3, x2 = (2 * W) / 3;
    const int tid = threadIdx.x, lane = tid & (EC_WAVE - 1);
    if (tid < 3) sets[tid] = 0;

    uint32_t table = KEY_NONE;
    if (lane < C) {
        const unsigned char* e = colors + ((size_t)b * C + lane) * 4;
        if (e[3]) table = key_at(e);
    }

    const unsigned char* src = sem + (size_t)b * H * W * 3;
    const bool aligned = ((uintptr_t)src & 3) == 0;
    const int P0 = r0 * W, P1 = r1 * W;                              // pixels [P0, P1) of the frame
    const int g0 = P0 >> 2, g1 = (P1 + 3) >> 2;                      // groups of 4 pixels, counted from the frame's start
    const int passes = (g1 - g0 + NT - 1) / NT;
    int p = (g0 + tid) << 2;
    int x = p % W;
    const int dx = (NT * 4) % W;
    uint64_t m0 = 0, m1 = 0, m2 = 0;
    auto load = [&](int p, uint32_t (&k)[4]) {                      // 4 pixels from pixel index p; KEY_OUTSIDE beyond the slice
        if (aligned && p >= P0 && p + 4 <= P1) {
            const uint32_t* q = reinterpret_cast<const uint32_t*>(src + (size_t)p * 3);
            const uint32_t w0 = q[0], w1 = q[1], w2 = q[2];
            k[0] = w0 & 0xFFFFFFu;
            k[1] = (w0 >> 24) | ((w1 & 0xFFFFu) << 8);
            k[2] = (w1 >> 16) | ((w2 & 0xFFu) << 16);
            k[3] = w2 >> 8;
        } else {
            for (int q = 0; q < 4; ++q) k[q] = (p + q >= P0 && p + q < P1) ? key_at(src + (size_t)(p + q) * 3) : KEY_OUTSIDE;
        }
    };
    uint32_t k[4], kn[4] = {KEY_OUTSIDE, KEY_OUTSIDE, KEY_OUTSIDE, KEY_OUTSIDE};
    load(p, k);
    for (int it = 0; it < passes; ++it) {
        p += NT * 4;
        if (it + 1 < passes) load(p, kn);                            // the next pass's loads fly during this pass's turns
        uint64_t set[4];
        classes_of(k, table, set);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            int xq = x + q;
            if (xq >= W) xq -= W;
            m0 |= xq < x1 ? set[q] : 0ull;
            m1 |= (xq >= x1 && xq < x2) ? set[q] : 0ull;
            m2 |= xq >= x2 ? set[q] : 0ull;
            k[q] = kn[q];
        }
        x += dx;
        if (x >= W) x -= W;
    }
    m0 = wave_or(m0);
    m1 = wave_or(m1);
    m2 = wave_or(m2);
    __syncthreads();                                                 // sets[] zeroed
    if (lane == 0) {
        if (m0) atomicOr(&sets[0], (unsigned long long)m0);
        if (m1) atomicOr(&sets[1], (unsigned long long)m1);
        if (m2) atomicOr(&sets[2], (unsigned long long)m2);
    }
    __syncthreads();
    if (tid < C) {
        bool any = false;
#pragma unroll
        for (int j = 0; j < 3; ++j)
            if ((sets[j] >> tid) & 1ull) {
                localization[((size_t)b * 9 + i * 3 + j) * C + tid] = 1;
                any = true;
            }
        if (any) presence[(size_t)b * C + tid] = 1;
    }
}

}  // namespace

extern "C" int ec_semantic_labels_u8(const uint8_t* sem_u8, const uint8_t* colors_u8, int64_t* presence, int64_t* localization,
                                     int B, int H, int W, int C, ec_stream_t stream) {
    if (!sem_u8 || !colors_u8 || !presence || !localization) return EC_ERR_ARG;
    if (B <= 0 || B > 65535 || H < 3 || W < 3 || C <= 0 || C > 64) return EC_ERR_SHAPE;
    if ((long long)H * W > (1ll << 28)) return EC_ERR_SHAPE;         // pixel indices are ints
    if (hipMemsetAsync(presence, 0, (size_t)B * C * sizeof(int64_t), (hipStream_t)stream) != hipSuccess) return EC_ERR_LAUNCH;
    if (hipMemsetAsync(localization, 0, (size_t)B * 9 * C * sizeof(int64_t), (hipStream_t)stream) != hipSuccess) return EC_ERR_LAUNCH;
    const long long cell_row_pixels = (long long)((H + 2) / 3) * W;
    long long slices = (cell_row_pixels + SLICE_PIXELS - 1) / SLICE_PIXELS;
    if (slices > MAX_SLICES) slices = MAX_SLICES;
    dim3 grid((unsigned)(3 * slices), (unsigned)B);
    hipLaunchKernelGGL(semantic_labels_kernel, grid, dim3(NT), 0, (hipStream_t)stream, sem_u8, colors_u8,
                       reinterpret_cast<long long*>(presence), reinterpret_cast<long long*>(localization), H, W, C, (int)slices);
    EC_CHECK_LAUNCH();
    return EC_OK;
}
