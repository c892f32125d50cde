// Imitation learning: expert cross-entropy (forward + analytic backward), its normaliser, and the teacher-forcing draw.
//
// Restates ([U] allenai/allenact ~v0.5.0; parity unpinned like the rest of the policy side):
//   Imitation.loss for a CategoricalDistr            (onpolicy_sync/losses/imitation.py: the `expert_action` branch)
//   TeacherForcingDistr.sample / log_prob            (base_abstractions/distributions.py)
// Launched by the reference's rearrangement baselines (readme_files/baselines_ithor_rearrangement.md: DAgger) and by
// AllenAct's behaviour-cloning / DAgger configurations of the ObjectNav and PointNav agents.
// All fp32 per row; every sum that crosses rows accumulates in fp64 in a FIXED order (no floating-point atomics), so two
// runs give the same bits and a row's gradient does not depend on which call or block it fell into.
#include <math.h>

#include "common.h"

namespace {

constexpr int IL_THREADS = 256;           // four waves per workgroup
// rows of one workgroup's contiguous chunk (more once B exceeds IL_MAX_BLOCKS chunks): one row per thread, or four rows per wave
// (a wave's rows are a serial load -> butterfly -> exp -> store chain each: at 64 rows per wave the launch was latency-bound)
constexpr int IL_ROWS = 256, IL_ROWS_WAVE = 16;
constexpr int IL_MAX_BLOCKS = 1024;
constexpr int IL_MAX_A = 256;             // the wave path keeps IL_MAX_A / 64 logits per lane
// scratch: [3 * block + i] the blocks' partial sums, [3 * IL_MAX_BLOCKS] the ticket counter
constexpr int IL_TICKET = 3 * IL_MAX_BLOCKS;

__device__ __forceinline__ float il_wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float il_wave_sum(float v) {   // xor butterfly: a fixed order, the same total on every lane
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// D of this call when the caller gives none: EVERY block sums the whole mask in the same order, so all blocks hold the same
// value without a grid-wide synchronisation.  Returned to every thread.
__device__ __forceinline__ double il_own_denominator(const float* __restrict__ mask, long B, double (*red)[1], double* bcast) {
    double m[1] = {0.0};
    for (long i = threadIdx.x; i < B; i += IL_THREADS) m[0] += (double)mask[i];
    ec_block_sum<1, IL_THREADS / 64>(m, red);
    if (threadIdx.x == 0) *bcast = m[0];
    __syncthreads();
    return *bcast;
}

// Partials -> scratch; the block that draws the last (integer) ticket folds them in block order (sumsq_kernel's pattern, ppo.hip)
__device__ __forceinline__ void il_fold(double (&acc)[3], double* __restrict__ scratch, double* __restrict__ sums3,
                                        double (*red)[3], unsigned* last) {
    ec_block_sum<3, IL_THREADS / 64>(acc, red);
    unsigned* ticket = reinterpret_cast<unsigned*>(scratch + IL_TICKET);
    if (threadIdx.x == 0) {
        scratch[3 * blockIdx.x + 0] = acc[0];
        scratch[3 * blockIdx.x + 1] = acc[1];
        scratch[3 * blockIdx.x + 2] = acc[2];
        __threadfence();                                             // the partials are visible device-wide before the ticket is
        *last = (atomicAdd(ticket, 1u) == gridDim.x - 1) ? 1u : 0u;
    }
    __syncthreads();
    if (!*last) return;
    __threadfence();                                                 // acquire: the other blocks' partials
    double f[3] = {0.0, 0.0, 0.0};
    for (unsigned b = threadIdx.x; b < gridDim.x; b += IL_THREADS)
#pragma unroll
        for (int i = 0; i < 3; ++i) f[i] += __hip_atomic_load(scratch + 3 * b + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();                                                 // (red is reused)
    ec_block_sum<3, IL_THREADS / 64>(f, red);
    if (threadIdx.x == 0) {
        sums3[0] = f[0]; sums3[1] = f[1]; sums3[2] = f[2];
        *ticket = 0u;
    }
}

// A <= 16: one thread per row, the row in registers (ppo_loss_kernel's shape).
template <int MAXA>
__global__ __launch_bounds__(IL_THREADS) void il_loss_row_kernel(const float* __restrict__ hv, const long long* __restrict__ expert,
                                                                 const float* __restrict__ mask, const double* __restrict__ denom,
                                                                 float* __restrict__ dhv, double* __restrict__ sums3,
                                                                 double* __restrict__ scratch, long B, int A, long chunk, float gw,
                                                                 int accumulate) {
    __shared__ double red1[IL_THREADS / 64][1];
    __shared__ double red3[IL_THREADS / 64][3];
    __shared__ double dshare;
    __shared__ unsigned last;
    const double D = denom ? denom[0] : il_own_denominator(mask, B, red1, &dshare);
    const float sc = gw * (float)(1.0 / (D > 1.0 ? D : 1.0));
    const long r0 = (long)blockIdx.x * chunk, r1 = (r0 + chunk < B) ? r0 + chunk : B;
    double acc[3] = {0.0, 0.0, 0.0};
    for (long i = r0 + threadIdx.x; i < r1; i += IL_THREADS) {
        const float m = mask[i];
        float* drow = dhv + i * (A + 1);
        if (m == 0.f) {                                              // the expert id of such a row is never read
            if (!accumulate)
                for (int k = 0; k <= A; ++k) drow[k] = 0.f;
            continue;
        }
        const float* row = hv + i * (A + 1);
        float lg[MAXA];
        float mx = -INFINITY;
        int best = 0;
#pragma unroll
        for (int k = 0; k < MAXA; ++k) {
            lg[k] = (k < A) ? row[k] : -INFINITY;
            if (lg[k] > mx) { mx = lg[k]; best = k; }                // strict: the FIRST maximal logit
        }
        const long long e = expert[i];
        const bool ok = e >= 0 && e < A;
        // softmax_k = ex_k / se; at k == e the gradient softmax_e - 1 is formed as -(sum of the OTHER ex) / se: no cancellation
        // when the row is near one-hot on the expert's action.  log_prob = (lg - mx) - log(se): the large common offset leaves first
        float se = 0.f, others = 0.f, d_e = 0.f;
#pragma unroll
        for (int k = 0; k < MAXA; ++k) {
            lg[k] = (k < A) ? expf(lg[k] - mx) : 0.f;                // (lg now holds ex_k)
            if (k < A && k == e) d_e = row[k] - mx;
            se += lg[k];
            others += (k == e) ? 0.f : lg[k];
        }
        const float inv = 1.f / se;
        const float lp_e = d_e - logf(se);
#pragma unroll
        for (int k = 0; k < MAXA; ++k) {
            if (k < A) {
                const float g = sc * m * ((k == e) ? -(others * inv) : lg[k] * inv);
                drow[k] = accumulate ? drow[k] + g : g;
            }
        }
        if (!accumulate) drow[A] = 0.f;
        acc[0] += (double)(m * -lp_e);
        acc[1] += (double)m;
        acc[2] += (double)((ok && best == (int)e) ? m : 0.f);
        if (!ok) acc[0] = (double)NAN;                               // ec_ppo_loss_ex's rule: an id outside [0, A) poisons the loss
    }
    il_fold(acc, scratch, sums3, red3, &last);
}

// A > 16: one 64-lane wave per row, lane-strided logits (lane, lane + 64, ...), max and sum by wave butterflies.
__global__ __launch_bounds__(IL_THREADS) void il_loss_wave_kernel(const float* __restrict__ hv, const long long* __restrict__ expert,
                                                                  const float* __restrict__ mask, const double* __restrict__ denom,
                                                                  float* __restrict__ dhv, double* __restrict__ sums3,
                                                                  double* __restrict__ scratch, long B, int A, long chunk, float gw,
                                                                  int accumulate) {
    __shared__ double red1[IL_THREADS / 64][1];
    __shared__ double red3[IL_THREADS / 64][3];
    __shared__ double dshare;
    __shared__ unsigned last;
    const double D = denom ? denom[0] : il_own_denominator(mask, B, red1, &dshare);
    const float sc = gw * (float)(1.0 / (D > 1.0 ? D : 1.0));
    const long r0 = (long)blockIdx.x * chunk, r1 = (r0 + chunk < B) ? r0 + chunk : B;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int PER = IL_MAX_A / 64;
    double acc[3] = {0.0, 0.0, 0.0};                                 // (lane 0 of every wave accumulates its rows)
    for (long i = r0 + wave; i < r1; i += IL_THREADS / 64) {
        const float m = mask[i];                                     // wave-uniform
        float* drow = dhv + i * (A + 1);
        if (m == 0.f) {
            if (!accumulate)
                for (int k = lane; k <= A; k += 64) drow[k] = 0.f;
            continue;
        }
        const float* row = hv + i * (A + 1);
        float lg[PER];
        float mx = -INFINITY;
        int best = 0x7fffffff;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int k = lane + 64 * j;
            lg[j] = (k < A) ? row[k] : -INFINITY;
            if (lg[j] > mx) { mx = lg[j]; best = k; }
        }
        const float lane_mx = mx;
        mx = il_wave_max(mx);
        // the first index of the row's maximum: the smallest index among the lanes that hold it
        int cand = (lane_mx == mx) ? best : 0x7fffffff;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { const int other = __shfl_xor(cand, o, 64); cand = other < cand ? other : cand; }
        const long long e = expert[i];
        const bool ok = e >= 0 && e < A;
        // (the row kernel's arithmetic: softmax_e - 1 as -(sum of the other ex) / se, log_prob = (lg - mx) - log(se))
        float se = 0.f, others = 0.f;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int k = lane + 64 * j;
            lg[j] = (k < A) ? expf(lg[j] - mx) : 0.f;                // (lg now holds ex_k)
            se += lg[j];
            others += (k == e) ? 0.f : lg[j];
        }
        se = il_wave_sum(se);
        others = il_wave_sum(others);
        const float inv = 1.f / se;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int k = lane + 64 * j;
            if (k < A) {
                const float g = sc * m * ((k == e) ? -(others * inv) : lg[j] * inv);
                drow[k] = accumulate ? drow[k] + g : g;
            }
        }
        if (lane == 0) {
            if (!accumulate) drow[A] = 0.f;
            const float lp_e = ok ? (row[e] - mx) - logf(se) : 0.f;
            acc[0] += (double)(m * -lp_e);
            acc[1] += (double)m;
            acc[2] += (double)((ok && cand == (int)e) ? m : 0.f);
            if (!ok) acc[0] = (double)NAN;
        }
    }
    il_fold(acc, scratch, sums3, red3, &last);
}

// out = sum over t < T, n0 <= n < n1 of mask[t, n]: one workgroup, a fixed order
__global__ __launch_bounds__(IL_THREADS) void il_count_kernel(const float* __restrict__ mask, int T, int N, int n0, int n1,
                                                              double* __restrict__ out) {
    __shared__ double red[IL_THREADS / 64][1];
    const int w = n1 - n0;
    double acc[1] = {0.0};
    for (long i = threadIdx.x; i < (long)T * w; i += IL_THREADS) acc[0] += (double)mask[(i / w) * N + n0 + (i % w)];
    ec_block_sum<1, IL_THREADS / 64>(acc, red);
    if (threadIdx.x == 0) out[0] = acc[0];
}

// TeacherForcingDistr: with probability p (and an expert action present) the step takes the expert's action and its log-prob
__global__ void il_teacher_force_kernel(const float* __restrict__ hv, const long long* __restrict__ expert,
                                        const float* __restrict__ mask, float p, long long* __restrict__ actions,
                                        float* __restrict__ logp, int N, int A, uint64_t seed, uint64_t step, int first_actor) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    if (mask[n] == 0.f) return;
    const uint64_t h = ec_mix64(ec_mix64(ec_mix64(seed) ^ IL_TF_STREAM) ^ (step * 0x100000001B3ull + (uint64_t)(n + first_actor)));
    const float u = (float)((h >> 40) * (1.0 / 16777216.0));   // [0,1) with 24 bits, as ec_sample_row's
    if (!(u < p)) return;
    const long long e = expert[n];
    actions[n] = e;
    if (e < 0 || e >= A) { logp[n] = NAN; return; }             // a present expert action outside [0, A): loud, and never an index
    const float* row = hv + (long)n * (A + 1);
    logp[n] = row[e] - ec_lse_row([&](int k) { return row[k]; }, A);
}

}  // namespace

extern "C" int ec_imitation_scratch_doubles(void) { return 3 * IL_MAX_BLOCKS + 1; }

extern "C" int ec_imitation_loss(const float* hv, const int64_t* expert_actions, const float* expert_mask, const double* denom,
                                 float* dhv, double* sums3, double* scratch, long B, int A, float weight, float grad_scale,
                                 int accumulate, ec_stream_t stream) {
    if (!hv || !expert_actions || !expert_mask || !dhv || !sums3 || !scratch) return EC_ERR_ARG;
    if (B <= 0 || A < 1 || A > IL_MAX_A) return EC_ERR_SHAPE;
    hipStream_t s = (hipStream_t)stream;
    const long per = (B + IL_MAX_BLOCKS - 1) / IL_MAX_BLOCKS;
    const long rows = A <= 16 ? IL_ROWS : IL_ROWS_WAVE;
    const long chunk = per > rows ? per : rows;                    // contiguous rows of one block
    const unsigned blocks = (unsigned)((B + chunk - 1) / chunk);
    (void)hipMemsetAsync(scratch + IL_TICKET, 0, sizeof(double), s);      // the ticket counter
    const float gw = grad_scale * weight;
    const long long* e = (const long long*)expert_actions;
    if (A <= 8)
        hipLaunchKernelGGL(il_loss_row_kernel<8>, dim3(blocks), dim3(IL_THREADS), 0, s, hv, e, expert_mask, denom, dhv, sums3,
                           scratch, B, A, chunk, gw, accumulate);
    else if (A <= 16)
        hipLaunchKernelGGL(il_loss_row_kernel<16>, dim3(blocks), dim3(IL_THREADS), 0, s, hv, e, expert_mask, denom, dhv, sums3,
                           scratch, B, A, chunk, gw, accumulate);
    else
        hipLaunchKernelGGL(il_loss_wave_kernel, dim3(blocks), dim3(IL_THREADS), 0, s, hv, e, expert_mask, denom, dhv, sums3,
                           scratch, B, A, chunk, gw, accumulate);
    EC_CHECK_LAUNCH();
    return EC_OK;
}

extern "C" int ec_expert_count(const float* expert_mask, int T, int N, int n0, int n1, double* out, ec_stream_t stream) {
    if (!expert_mask || !out) return EC_ERR_ARG;
    if (T <= 0 || N <= 0 || n0 < 0 || n1 <= n0 || n1 > N) return EC_ERR_SHAPE;
    hipLaunchKernelGGL(il_count_kernel, dim3(1), dim3(IL_THREADS), 0, (hipStream_t)stream, expert_mask, T, N, n0, n1, out);
    EC_CHECK_LAUNCH();
    return EC_OK;
}

extern "C" int ec_teacher_force(const float* hv, const int64_t* expert_actions, const float* expert_mask, float p,
                                int64_t* actions, float* logp, int N, int A, uint64_t seed, uint64_t step, int first_actor,
                                ec_stream_t stream) {
    if (!hv || !expert_actions || !expert_mask || !actions || !logp) return EC_ERR_ARG;
    if (!(p >= 0.f && p <= 1.f)) return EC_ERR_ARG;                // (NaN included)
    if (N <= 0 || A <= 0 || first_actor < 0) return EC_ERR_SHAPE;
    if (p == 0.f) return EC_OK;                                    // nothing is forced: no launch
    hipLaunchKernelGGL(il_teacher_force_kernel, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, hv,
                       (const long long*)expert_actions, expert_mask, p, (long long*)actions, logp, N, A, seed, step, first_actor);
    EC_CHECK_LAUNCH();
    return EC_OK;
}
