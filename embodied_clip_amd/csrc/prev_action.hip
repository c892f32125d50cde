// Previous-action embedding of the recurrent input: the weight-derived table, its gather-add onto the GRU's input projection
// and its gradient as a binned ordered sum.
//
// Restates (published sources, not under the reference tree: parity unpinned, as for the PointNav goal encoder):
//   [U] habitat_baselines PointNavResNetPolicy: prev_action_embedding = nn.Embedding(num_actions + 1, 32), indexed by
//       ((prev_actions.float() + 1) * masks).long(), concatenated to the recurrent input;
//   [U] allenact VisualNavActorCritic: prev_action_embedder = FeatureEmbedding(action_space.n [+ 1], action_embed_size)
//       (add_prev_actions, add_prev_action_null_token), concatenated to the observation embedding before state_encoder.
// The embedding reaches the network through gi = x' . weight_ih^T alone, so with Wa = weight_ih[:, flat : flat + E]
//   PT = Emb . Wa^T [R, G]    gi[b] += PT[idx[b]]    dPT[r] = sum over {b : idx[b] == r} of dgi[b]
//   dEmb += dPT . Wa          dWa += dPT^T . Emb
// (R = A + null rows, G = 3 * hidden columns) and nothing [B, E]-shaped exists.  idx[b] is formed here from prev_actions, masks
// and the null flag (ec_pa_index, common.h); an index outside [0, R) is never dereferenced: that frame adds nothing and receives nothing.
// No floating-point atomics: every sum below has a fixed order that depends on the shapes alone.
#include "common.h"

namespace {

constexpr int PA_MAX_A = 256;
constexpr int PA_MAX_E = 64;
constexpr int PA_COLS = 64;               // columns of one workgroup (one wave): a lane owns a column
constexpr int PA_CHUNK_MIN = 128;         // fewest frames of one partition of the binned sum
constexpr long PA_MAX_PARTS = 4096;       // most partitions (gridDim.y)

// PT[r, g] = sum_e Emb[r, e] * W[g * ld + col0 + e], fp32 FMA in ascending e.  A workgroup stages 64 rows of Wa (E contiguous
// floats each, whatever ld is) in LDS at an odd pitch, then wave w forms table rows w, w + 4, ...: Emb[r, e] is wave-uniform.
__global__ __launch_bounds__(256) void pa_table_kernel(const float* __restrict__ emb, const float* __restrict__ w, long ld, int col0,
                                                       float* __restrict__ pt, int R, int G, int E) {
    __shared__ float wt[PA_COLS * (PA_MAX_E + 1)];
    const int pitch = E | 1;
    const int g0 = blockIdx.x * PA_COLS;
    for (int i = threadIdx.x; i < PA_COLS * E; i += 256) {
        const int g = i / E, e = i - g * E;
        wt[g * pitch + e] = (g0 + g < G) ? w[(long)(g0 + g) * ld + col0 + e] : 0.f;
    }
    __syncthreads();
    const int gl = threadIdx.x & 63, g = g0 + gl;
    const float* wrow = wt + gl * pitch;
    for (int r = threadIdx.x >> 6; r < R; r += 4) {
        const float* erow = emb + (long)r * E;
        float acc = 0.f;
        for (int e = 0; e < E; ++e) acc = fmaf(erow[e], wrow[e], acc);
        if (g < G) pt[(long)r * G + g] = acc;
    }
}

// gi[b, :] += PT[idx[b], :]; VEC = 4: one float4 per thread (G a multiple of 4, both bases 16-byte aligned)
template <int VEC>
__global__ __launch_bounds__(256) void pa_add_kernel(float* __restrict__ gi, const float* __restrict__ pt,
                                                     const long long* __restrict__ prev, const float* __restrict__ masks,
                                                     int null_token, int A, long B, int G) {
    const int per = G / VEC;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= B * per) return;
    const long b = i / per;
    const int c = (int)(i - b * per) * VEC;
    const int r = ec_pa_index(prev, masks, b, null_token, A);
    if (r < 0) return;
    if (VEC == 4) {
        float4 v = *reinterpret_cast<float4*>(gi + b * G + c);
        const float4 t = *reinterpret_cast<const float4*>(pt + (long)r * G + c);
        v.x += t.x; v.y += t.y; v.z += t.z; v.w += t.w;
        *reinterpret_cast<float4*>(gi + b * G + c) = v;
    } else {
        gi[b * G + c] += pt[(long)r * G + c];
    }
}

// Binned sum of one partition: workgroup (x, p) = one wave owns columns 64 x .. 64 x + 63 of frames [p * chunk, (p + 1) * chunk)
// and keeps R x 64 bins in LDS (lane = column = bank: conflict-free, and no lane reads another lane's bins, so no barrier).
// Frames are walked in ascending b, eight loads in flight; the frame's row is wave-uniform.  The bins of every row are stored,
// zeros included, so the fold below reads nothing that was not written by this call.
__global__ __launch_bounds__(64) void pa_bin_kernel(const float* __restrict__ dgi, const long long* __restrict__ prev,
                                                    const float* __restrict__ masks, int null_token, int A, float* __restrict__ part,
                                                    long B, int G, long chunk) {
    extern __shared__ float bins[];                                   // [R][PA_COLS]
    const int R = A + null_token;
    const int lane = threadIdx.x;
    const int col = blockIdx.x * PA_COLS + lane;
    const bool on = col < G;
    const int c = on ? col : G - 1;                                    // (columns past G read the last one; never stored)
    const long b0 = (long)blockIdx.y * chunk;
    const long b1 = (b0 + chunk < B) ? b0 + chunk : B;
    for (int r = 0; r < R; ++r) bins[r * PA_COLS + lane] = 0.f;
    for (long b = b0; b < b1; b += 8) {
        float v[8];
        int ix[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const bool live = b + u < b1;
            const long bb = live ? b + u : b1 - 1;
            ix[u] = live ? ec_pa_index(prev, masks, bb, null_token, A) : -1;
            v[u] = dgi[bb * G + c];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (ix[u] >= 0) bins[ix[u] * PA_COLS + lane] += v[u];
    }
    if (!on) return;
    float* dst = part + (long)blockIdx.y * R * G + col;
    for (int r = 0; r < R; ++r) dst[(long)r * G] = bins[r * PA_COLS + lane];
}

// dPT[e] = the partitions' bins of element e, folded in partition order
__global__ __launch_bounds__(256) void pa_fold_kernel(const float* __restrict__ part, float* __restrict__ dpt, long RG, int P) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= RG) return;
    float acc = 0.f;
    for (int p = 0; p < P; ++p) acc += part[(long)p * RG + e];
    dpt[e] = acc;
}

// dEmb[r, e] += sum_g dPT[r, g] * W[g * ld + col0 + e]: one workgroup per table row, lane = e, wave q sums the q-th contiguous
// quarter of g in ascending order (one wave walking all 1536 columns was a serial chain of loads: 7 such waves took longer than
// the pass over dgi), the four quarters are folded in order
__global__ __launch_bounds__(256) void pa_demb_kernel(const float* __restrict__ dpt, const float* __restrict__ w, long ld, int col0,
                                                      float* __restrict__ demb, int G, int E) {
    __shared__ float red[4][64];
    const int r = blockIdx.x, e = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int per = (G + 3) / 4, g0 = q * per, g1 = (g0 + per < G) ? g0 + per : G;
    const float* drow = dpt + (long)r * G;
    const float* wcol = w + col0 + (e < E ? e : 0);                  // (lanes past E read column 0; never stored)
    float acc = 0.f;
#pragma unroll 8
    for (int g = g0; g < g1; ++g) acc = fmaf(drow[g], wcol[(long)g * ld], acc);
    red[q][e] = acc;
    __syncthreads();
    if (q == 0 && e < E) demb[(long)r * E + e] += ((red[0][e] + red[1][e]) + red[2][e]) + red[3][e];
}

// dW[g * ld + col0 + e] += sum_r dPT[r, g] * Emb[r, e], ascending r: one wave per row of weight_ih, lane = e
__global__ __launch_bounds__(64) void pa_dw_kernel(const float* __restrict__ dpt, const float* __restrict__ emb, float* __restrict__ dw,
                                                   long ld, int col0, int R, int G, int E) {
    const int g = blockIdx.x, e = threadIdx.x;
    if (e >= E) return;
    float acc = 0.f;
    for (int r = 0; r < R; ++r) acc = fmaf(dpt[(long)r * G + g], emb[(long)r * E + e], acc);
    dw[(long)g * ld + col0 + e] += acc;
}

// weight_ih[:, :flat] of a handle with a previous-action embedding as a dense [rows, flat] copy (add == 0), and the dense
// gradient added back onto the parameter's rows (add == 1): policy.hip's routes that read weight_ih in its own column order
__global__ __launch_bounds__(256) void pa_rows_copy_kernel(const float* __restrict__ in, int ld_in, float* __restrict__ out, int ld_out,
                                                       int cols, long total, int add) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long r = i / cols;
    const int c = (int)(i - r * cols);
    if (add) out[r * ld_out + c] += in[r * ld_in + c];
    else out[r * ld_out + c] = in[r * ld_in + c];
}

// policy.hip's gi_act_kernel<NW> with the previous action's table row added in the fold (the shared body: common.h)
template <int NW>
__global__ __launch_bounds__(NW * 64) void pa_gi_act_kernel(const float* __restrict__ x, const float* __restrict__ W,
                                                            const float* __restrict__ bias, float* __restrict__ gi, int N, int K, int NO,
                                                            ec_gi_act_pa pa) {
    ec_gi_act_body<NW, true>(x, W, bias, gi, N, K, NO, pa);
}

// frames of one partition: at least R (the partitions' bins then take no more room than dgi itself) and at least PA_CHUNK_MIN
long pa_chunk(long B, int R) {
    long chunk = R > PA_CHUNK_MIN ? R : PA_CHUNK_MIN;
    const long cap = (B + PA_MAX_PARTS - 1) / PA_MAX_PARTS;
    return chunk > cap ? chunk : cap;
}

bool pa_shape_ok(long B, int G, int A, int null_token, int E) {
    return B > 0 && G > 0 && A >= 1 && A <= PA_MAX_A && (null_token == 0 || null_token == 1) && E >= 1 && E <= PA_MAX_E;
}

}  // namespace

// policy.hip's hooks (declared in common.h): the launches without the argument checks of the C-ABI faces below
void ec_pa_table_launch(const float* emb, const float* w, long ld, int col0, float* pt, int R, int G, int E, hipStream_t s) {
    hipLaunchKernelGGL(pa_table_kernel, dim3((unsigned)((G + PA_COLS - 1) / PA_COLS)), dim3(256), 0, s, emb, w, ld, col0, pt, R, G, E);
}
void ec_pa_add_launch(float* gi, const float* pt, const long long* prev, const float* masks, int null_token, int A, long B, int G,
                      hipStream_t s) {
    const bool vec = (G & 3) == 0 && (((uintptr_t)gi | (uintptr_t)pt) & 15) == 0;
    const long n = vec ? B * (G / 4) : B * G;
    const dim3 grid((unsigned)((n + 255) / 256));
    if (vec)
        hipLaunchKernelGGL(pa_add_kernel<4>, grid, dim3(256), 0, s, gi, pt, prev, masks,
                           null_token, A, B, G);
    else
        hipLaunchKernelGGL(pa_add_kernel<1>, grid, dim3(256), 0, s, gi, pt, prev, masks,
                           null_token, A, B, G);
}
void ec_pa_gi_act_launch(int nw, const float* x, const float* W, const float* bias, float* gi, int N, int K, int NO, ec_gi_act_pa pa,
                         hipStream_t s) {
    const dim3 grid((unsigned)(NO / 32), (unsigned)((N + 31) / 32));
    if (nw == 7) hipLaunchKernelGGL(pa_gi_act_kernel<7>, grid, dim3(64 * 7), 0, s, x, W, bias, gi, N, K, NO, pa);
    else hipLaunchKernelGGL(pa_gi_act_kernel<8>, grid, dim3(64 * 8), 0, s, x, W, bias, gi, N, K, NO, pa);
}
void ec_pa_rows_copy_launch(const float* in, int ld_in, float* out, int ld_out, int rows, int cols, int add, hipStream_t s) {
    const long total = (long)rows * cols;
    hipLaunchKernelGGL(pa_rows_copy_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, in, ld_in, out, ld_out, cols, total, add);
}
size_t ec_pa_grad_scratch_floats(long B, int G, int R) {
    const long chunk = pa_chunk(B, R);
    return (size_t)((B + chunk - 1) / chunk + 1) * R * G;
}
// the binned ordered sum alone: dPT [R, G] into the first R * G floats of the scratch (the partitions' bins behind it)
void ec_pa_bins_launch(const float* dgi, const long long* prev, const float* masks, int null_token, int A, float* scratch, long B, int G,
                       hipStream_t s) {
    const int R = A + null_token;
    const long chunk = pa_chunk(B, R);
    const int P = (int)((B + chunk - 1) / chunk);
    const long RG = (long)R * G;
    float* dpt = scratch;                                             // [R, G]; what the caller may read afterwards
    float* part = scratch + RG;                                       // [P, R, G]
    const size_t lds = (size_t)R * PA_COLS * sizeof(float);           // at most 257 x 64 x 4 = 65,792 B
    static std::atomic<uint64_t> attr_done{0};
    if (auto g = ec_attr_needed(attr_done))
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(pa_bin_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)((PA_MAX_A + 1) * PA_COLS * sizeof(float)));
    hipLaunchKernelGGL(pa_bin_kernel, dim3((unsigned)((G + PA_COLS - 1) / PA_COLS), (unsigned)P), dim3(64), lds, s, dgi,
                       prev, masks, null_token, A, part, B, G, chunk);
    hipLaunchKernelGGL(pa_fold_kernel, dim3((unsigned)((RG + 255) / 256)), dim3(256), 0, s, part, dpt, RG, P);
}
void ec_pa_grad_launch(const float* dgi, const long long* prev, const float* masks, int null_token, int A, const float* emb,
                       const float* w, long ld, int col0, float* demb, float* dw, float* scratch, long B, int G, int E, hipStream_t s) {
    const int R = A + null_token;
    const float* dpt = scratch;
    ec_pa_bins_launch(dgi, prev, masks, null_token, A, scratch, B, G, s);
    hipLaunchKernelGGL(pa_demb_kernel, dim3((unsigned)R), dim3(256), 0, s, dpt, w, ld, col0, demb, G, E);
    hipLaunchKernelGGL(pa_dw_kernel, dim3((unsigned)G), dim3(64), 0, s, dpt, emb, dw, ld, col0, R, G, E);
}

extern "C" int ec_prev_action_table(const float* emb, const float* w, long ld, int col0, float* pt, int A, int null_token, int G,
                                    int E, ec_stream_t stream) {
    if (!emb || !w || !pt) return EC_ERR_ARG;
    if (!pa_shape_ok(1, G, A, null_token, E) || col0 < 0 || ld < (long)col0 + E) return EC_ERR_SHAPE;
    ec_pa_table_launch(emb, w, ld, col0, pt, A + null_token, G, E, (hipStream_t)stream);
    EC_CHECK_LAUNCH();
    return EC_OK;
}

extern "C" int ec_prev_action_add(float* gi, const float* pt, const int64_t* prev_actions, const float* masks, int null_token, int A,
                                  long B, int G, ec_stream_t stream) {
    if (!gi || !pt || !prev_actions) return EC_ERR_ARG;
    if (!pa_shape_ok(B, G, A, null_token, 1)) return EC_ERR_SHAPE;
    if (null_token && !masks) return EC_ERR_ARG;
    if ((B * G + 255) / 256 > 0x7fffffffL) return EC_ERR_SHAPE;
    ec_pa_add_launch(gi, pt, (const long long*)prev_actions, masks, null_token, A, B, G, (hipStream_t)stream);
    EC_CHECK_LAUNCH();
    return EC_OK;
}

extern "C" size_t ec_prev_action_grad_scratch_floats(long B, int G, int A, int null_token) {
    if (!pa_shape_ok(B, G, A, null_token, 1)) return 0;
    return ec_pa_grad_scratch_floats(B, G, A + null_token);
}

extern "C" int ec_prev_action_grad(const float* dgi, const int64_t* prev_actions, const float* masks, int null_token, int A,
                                   const float* emb, const float* w, long ld, int col0, float* demb, float* dw, float* scratch, long B,
                                   int G, int E, ec_stream_t stream) {
    if (!dgi || !prev_actions || !emb || !w || !demb || !dw || !scratch) return EC_ERR_ARG;
    if (!pa_shape_ok(B, G, A, null_token, E) || col0 < 0 || ld < (long)col0 + E) return EC_ERR_SHAPE;
    if (null_token && !masks) return EC_ERR_ARG;
    ec_pa_grad_launch(dgi, (const long long*)prev_actions, masks, null_token, A, emb, w, ld, col0, demb, dw, scratch, B, G, E, (hipStream_t)stream);
    EC_CHECK_LAUNCH();
    return EC_OK;
}
