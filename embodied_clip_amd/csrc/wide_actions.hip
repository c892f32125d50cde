// Wide action spaces (up to 256 actions; the reference's fifth experiment, iTHOR rearrangement, has 84:
// readme_files/baselines_ithor_rearrangement.md): the actor / critic heads with the action selection in the same launch, and
// the PPO loss with one wave per row; for the learn pass of such a handle, both heads packed into one [A + 1, H] table (one GEMM
// each way in policy.hip) and the goal-embedding scatter of the unfused encoder tail in a fixed order.
//
// Restates ([U] allenai/allenact ~v0.5.0, as policy.hip / ppo.hip / imitation.hip do for the narrow agents):
//   LinearActorHead + LinearCriticHead                 (embodiedai/models/basic_models.py)
//   CategoricalDistr.sample / mode / log_prob          (base_abstractions/distributions.py)
//   TeacherForcingDistr.sample / log_prob              (the same file)
//   PPO.loss_per_step                                  (onpolicy_sync/losses/ppo.py)
// The narrow kernels keep a row's A + 1 outputs in one thread's registers (heads_fwd_kernel<8>, ppo_loss_kernel<16>); here a
// row is spread over lanes.  Every sum that the shared selection functions (common.h) form serially is formed serially here
// too, so the selection equals ec_sample_actions / ec_mode_actions / ec_teacher_force on the logits this launch wrote, bit for
// bit.  A row's outputs depend on that row alone (not on B, not on the rows that share its workgroup); reductions that cross
// rows accumulate in fp64 in a fixed order (no floating-point atomics).
#include <math.h>

#include "common.h"

namespace {

constexpr int WA_MAX_A = 256;
constexpr int WA_THREADS = 256;           // four waves per workgroup
constexpr int WA_ROWS = 4;                // heads: rows of one workgroup -- one selection wave per row
constexpr int WA_LD = WA_MAX_A + 4;       // LDS row pitch of the outputs (A + 1 <= 257)

__device__ __forceinline__ float wa_wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float wa_wave_sum(float v) {   // xor butterfly: a fixed order, the same total on every lane
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

struct WaSelect {
    long long* actions;               // nullptr: logits and values only
    float* logp;
    float* values;                    // or nullptr
    uint64_t seed, step;
    int first_actor;
    int greedy;
    const long long* expert;          // teacher forcing: all three or none
    const float* mask;
    float force_p;
};

// hv[b, :A] = hs[b] . Wa^T + ba, hv[b, A] = hs[b] . wc + bc for WA_ROWS rows per workgroup, then one wave per row selects.
// Dot products: 16 lanes share one output -- lane j of the group owns elements [64 i + 4 j, 64 i + 4 j + 4) of the row, one
// float4 of the weight row per step (a wave reads 4 weight rows x 256 contiguous bytes) against the rows' float4s from LDS --
// then a 16-lane xor butterfly: the order depends on H alone.
__global__ __launch_bounds__(WA_THREADS) void wa_heads_kernel(const float* __restrict__ hs, const float* __restrict__ Wa,
                                                              const float* __restrict__ ba, const float* __restrict__ Wc,
                                                              const float* __restrict__ bc, float* __restrict__ hv, long B, int H,
                                                              int A, WaSelect sel) {
    extern __shared__ float wa_lds[];
    float* xs = wa_lds;                                   // [WA_ROWS][H]
    float* outs = wa_lds + (size_t)WA_ROWS * H;           // [WA_ROWS][WA_LD]: the rows' logits and value
    float* exs = outs + WA_ROWS * WA_LD;                  // [WA_ROWS][WA_LD]: exp terms of the selection
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long row0 = (long)blockIdx.x * WA_ROWS;
    const int A1 = A + 1;
    const int H4 = H >> 2;
    // rows past B read row B - 1 (their results are never stored)
    for (int i = tid; i < WA_ROWS * H4; i += WA_THREADS) {
        const int r = i / H4, c = i - r * H4;
        long row = row0 + r;
        row = row < B ? row : B - 1;
        reinterpret_cast<float4*>(xs)[r * H4 + c] = reinterpret_cast<const float4*>(hs + row * H)[c];
    }
    __syncthreads();
    const int sub = tid & 15, og = tid >> 4;
    for (int o0 = 0; o0 < A1; o0 += WA_THREADS / 16) {
        const int o = o0 + og;
        const bool live = o < A1;
        const float* wrow = (live && o < A) ? Wa + (long)o * H : Wc;      // (outputs past A read wc; discarded)
        float acc[WA_ROWS];
#pragma unroll
        for (int r = 0; r < WA_ROWS; ++r) acc[r] = 0.f;
#pragma unroll 4
        for (int c = sub; c < H4; c += 16) {
            const float4 wv = reinterpret_cast<const float4*>(wrow)[c];
#pragma unroll
            for (int r = 0; r < WA_ROWS; ++r) {
                const float4 v = reinterpret_cast<const float4*>(xs)[r * H4 + c];
                acc[r] = fmaf(v.w, wv.w, fmaf(v.z, wv.z, fmaf(v.y, wv.y, fmaf(v.x, wv.x, acc[r]))));
            }
        }
#pragma unroll
        for (int r = 0; r < WA_ROWS; ++r) {
#pragma unroll
            for (int off = 8; off > 0; off >>= 1) acc[r] += __shfl_xor(acc[r], off, 64);
        }
        if (live && sub == 0) {
            const float bias = o < A ? ba[o] : bc[0];
#pragma unroll
            for (int r = 0; r < WA_ROWS; ++r) outs[r * WA_LD + o] = acc[r] + bias;
        }
    }
    __syncthreads();
    for (int i = tid; i < WA_ROWS * A1; i += WA_THREADS) {
        const int r = i / A1, o = i - r * A1;
        if (row0 + r < B) hv[(row0 + r) * A1 + o] = outs[r * WA_LD + o];
    }
    if (!sel.actions) return;                             // (uniform over the grid)

    // ---- selection: wave w owns row w of the workgroup.  Every wave runs every barrier below; `on` masks the stores.
    const long row = row0 + wave;
    const bool on = row < B;
    const float* lg = outs + wave * WA_LD;
    float* ex = exs + wave * WA_LD;
    // ec_lse_row: the maximum (order-free), then the exp terms (lanes), then their sum in index order (lane 0)
    float mx = -INFINITY, top = -INFINITY;
    int best = 0x7fffffff;
    for (int k = lane; k < A; k += 64) {
        const float v = lg[k];
        mx = fmaxf(mx, v);
        if (v > top) { top = v; best = k; }               // strict: the lane's FIRST maximal logit
    }
    mx = wa_wave_max(mx);
    for (int k = lane; k < A; k += 64) ex[k] = expf(lg[k] - mx);
    __syncthreads();
    float lse = 0.f;
    if (lane == 0) {
        float se = 0.f;
        for (int k = 0; k < A; ++k) se += ex[k];
        lse = mx + logf(se);
    }
    lse = __shfl(lse, 0, 64);
    __syncthreads();                                      // (ex is rewritten below)
    int a = 0;
    if (sel.greedy) {
        // ec_mode_row: the first index of the maximal logit = the smallest index among the lanes that hold the maximum
        int cand = (best != 0x7fffffff && top == mx) ? best : 0x7fffffff;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { const int other = __shfl_xor(cand, o, 64); cand = other < cand ? other : cand; }
        a = cand == 0x7fffffff ? 0 : cand;
    } else {
        // ec_sample_row: the CDF terms (lanes), then the running sum and its first crossing in index order (lane 0)
        for (int k = lane; k < A; k += 64) ex[k] = expf(lg[k] - lse);
        __syncthreads();
        if (lane == 0) {
            const uint64_t h = ec_mix64(ec_mix64(sel.seed) ^ (sel.step * 0x100000001B3ull + (uint64_t)((int)row + sel.first_actor)));
            const float u = (float)((h >> 40) * (1.0 / 16777216.0));   // [0,1) with 24 bits
            float cdf = 0.f;
            a = A - 1;
            for (int k = 0; k < A; ++k) {
                cdf += ex[k];
                if (u < cdf) { a = k; break; }
            }
        }
    }
    if (lane == 0 && on) {
        long long act = a;
        float lp = lg[a] - lse;
        if (sel.expert && sel.mask[row] != 0.f) {         // il_teacher_force_kernel's rule and uniform stream
            const uint64_t h = ec_mix64(ec_mix64(ec_mix64(sel.seed) ^ IL_TF_STREAM) ^
                                        (sel.step * 0x100000001B3ull + (uint64_t)((int)row + sel.first_actor)));
            const float u = (float)((h >> 40) * (1.0 / 16777216.0));
            if (u < sel.force_p) {
                const long long e = sel.expert[row];
                act = e;
                lp = (e < 0 || e >= A) ? NAN : lg[e] - lse;   // a present expert action outside [0, A): loud, never an index
            }
        }
        sel.actions[row] = act;
        sel.logp[row] = lp;
        if (sel.values) sel.values[row] = lg[A];
    }
}

// ---- PPO loss -----------------------------------------------------------------------------------------------------------
constexpr int WP_ROWS_WAVE = 16;          // rows of one workgroup's contiguous chunk (more once B exceeds WP_MAX_BLOCKS chunks)
constexpr int WP_MAX_BLOCKS = 1024;
// scratch: [4 * block + i] the blocks' partial sums, [4 * WP_MAX_BLOCKS] the ticket counter
constexpr int WP_TICKET = 4 * WP_MAX_BLOCKS;

// ppo_loss_kernel's per-row arithmetic (ppo.hip) with the row spread over a 64-lane wave: lane-strided logits (lane,
// lane + 64, ...), max and sums by xor butterflies (il_loss_wave_kernel's layout, imitation.hip).
__global__ __launch_bounds__(WA_THREADS) void wa_ppo_loss_kernel(const float* __restrict__ hv, const long long* __restrict__ actions,
                                                                 const float* __restrict__ old_logp, const float* __restrict__ old_val,
                                                                 const float* __restrict__ returns, const float* __restrict__ nadv,
                                                                 float* __restrict__ dhv, double* __restrict__ sums,
                                                                 double* __restrict__ scratch, long B, int A, long chunk, float clip,
                                                                 float vclip, float vcoef, float ecoef, float grad_scale) {
    __shared__ double red[WA_THREADS / 64][4];
    __shared__ unsigned last;
    const long r0 = (long)blockIdx.x * chunk, r1 = (r0 + chunk < B) ? r0 + chunk : B;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int PER = WA_MAX_A / 64;
    const float invB = grad_scale / (float)B;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};                            // (lane 0 of every wave accumulates its rows)
    for (long i = r0 + wave; i < r1; i += WA_THREADS / 64) {
        const float* row = hv + i * (A + 1);
        float lg[PER];
        float mx = -INFINITY;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int k = lane + 64 * j;
            lg[j] = (k < A) ? row[k] : -INFINITY;
            mx = fmaxf(mx, lg[j]);
        }
        mx = wa_wave_max(mx);
        float se = 0.f;
#pragma unroll
        for (int j = 0; j < PER; ++j) se += (lane + 64 * j < A) ? expf(lg[j] - mx) : 0.f;
        se = wa_wave_sum(se);
        // log p_k = (lg - mx) - log(se): the large common offset leaves first (il_loss_wave_kernel's form) -- mx + log(se) rounds at
        // the magnitude of the logits, and at logit scale 30 that rounding (2^-18) shows in the ratio and in every p_k
        const float lse = logf(se);
        const long long a64 = actions[i];                            // range-checked as 64 bits: 1 << 32 is no action 0
        const int a = (a64 >= 0 && a64 < A) ? (int)a64 : -1;
        float ent = 0.f, lp_a = 0.f;
        float pr[PER];
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int k = lane + 64 * j;
            lg[j] = (k < A) ? (lg[j] - mx) - lse : 0.f;              // (lg now holds log p_k)
            pr[j] = (k < A) ? expf(lg[j]) : 0.f;
            ent -= pr[j] * lg[j];
            if (k < A && k == a) lp_a = lg[j];
        }
        ent = wa_wave_sum(ent);
        lp_a = wa_wave_sum(lp_a);                                    // (one lane holds it, the others 0: exact)
        // from here every lane holds the row's scalars
        const float adv = nadv[i];
        const float ratio = expf(lp_a - old_logp[i]);
        const float surr1 = ratio * adv;
        const float rc = fminf(fmaxf(ratio, 1.f - clip), 1.f + clip);
        const float surr2 = rc * adv;
        const bool use2 = surr2 < surr1;
        const float la = -(use2 ? surr2 : surr1);
        // d(-min)/d(ratio): surr1 branch -> -adv; surr2 branch -> -adv inside the clamp range, 0 outside
        const bool in_rng = (ratio >= 1.f - clip) && (ratio <= 1.f + clip);
        const float dla_dratio = use2 ? (in_rng ? -adv : 0.f) : -adv;
        const float dla_dlp = dla_dratio * ratio;
        const float v = row[A], vo = old_val[i], R = returns[i];
        const float dv = v - vo;
        // vclip < 0: use_clipped_value_loss=False -> 0.5 * (R - V)^2
        const bool vc_on = vclip >= 0.f;
        const float vcl = vc_on ? vo + fminf(fmaxf(dv, -vclip), vclip) : v;
        const float l1 = (v - R) * (v - R), l2 = (vcl - R) * (vcl - R);
        const float lv = 0.5f * fmaxf(l1, l2);
        const bool v_in = !vc_on || ((dv >= -vclip) && (dv <= vclip));
        const float g1 = (v - R), g2 = v_in ? (vcl - R) : 0.f;
        const float dlv_dv = (l1 > l2) ? g1 : ((l2 > l1) ? g2 : 0.5f * (g1 + g2));   // torch.max splits ties evenly
        float* drow = dhv + i * (A + 1);
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int k = lane + 64 * j;
            if (k < A) {
                const float dlp = ((k == a) ? 1.f : 0.f) - pr[j];
                const float dent = pr[j] * (lg[j] + ent);            // d(-H)/dlogit_k
                drow[k] = invB * (dla_dlp * dlp + ecoef * dent);
            }
        }
        if (lane == 0) {
            drow[A] = invB * vcoef * dlv_dv;
            acc[0] += la; acc[1] += lv; acc[2] += -ent; acc[3] += ratio;
            if (a < 0) acc[0] = (double)NAN;                           // ec_ppo_loss_ex's rule: an id outside [0, A) poisons the loss
        }
    }
    // partials -> scratch; the block that draws the last (integer) ticket folds them in block order (sumsq_kernel's pattern)
    ec_block_sum<4, WA_THREADS / 64>(acc, red);
    unsigned* ticket = reinterpret_cast<unsigned*>(scratch + WP_TICKET);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) scratch[4 * blockIdx.x + q] = acc[q];
        __threadfence();                                             // the partials are visible device-wide before the ticket is
        last = (atomicAdd(ticket, 1u) == gridDim.x - 1) ? 1u : 0u;
    }
    __syncthreads();
    if (!last) return;
    __threadfence();                                                 // acquire: the other blocks' partials
    double f[4] = {0.0, 0.0, 0.0, 0.0};
    for (unsigned b = threadIdx.x; b < gridDim.x; b += WA_THREADS)
#pragma unroll
        for (int q = 0; q < 4; ++q) f[q] += __hip_atomic_load(scratch + 4 * b + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();                                                 // (red is reused)
    ec_block_sum<4, WA_THREADS / 64>(f, red);
    if (threadIdx.x == 0) {
        sums[0] = f[0]; sums[1] = f[1]; sums[2] = f[2]; sums[3] = f[3];
        *ticket = 0u;
    }
}

// ---- learn pass: both heads as one [A + 1, H] table -----------------------------------------------------------------------
// tab = [Wa; wc | ba; bc]: (A + 1) * H weights, then A + 1 biases.  The learn pass runs its heads as ONE GEMM each way on it
// (no product with an M, N or K of 1); wa_heads_unpack_add_kernel adds the table's gradient onto the four gradient tensors.
__global__ __launch_bounds__(WA_THREADS) void wa_heads_pack_kernel(const float* __restrict__ Wa, const float* __restrict__ ba,
                                                                   const float* __restrict__ wc, const float* __restrict__ bc,
                                                                   float* __restrict__ tab, int A, int H) {
    const long nw = (long)(A + 1) * H, ne = nw + A + 1;
    const long e = (long)blockIdx.x * WA_THREADS + threadIdx.x;
    if (e >= ne) return;
    if (e < nw) tab[e] = e < (long)A * H ? Wa[e] : wc[e - (long)A * H];
    else tab[e] = (e - nw) < A ? ba[e - nw] : bc[0];
}
__global__ __launch_bounds__(WA_THREADS) void wa_heads_unpack_add_kernel(const float* __restrict__ gtab, float* __restrict__ gWa,
                                                                         float* __restrict__ gba, float* __restrict__ gwc,
                                                                         float* __restrict__ gbc, int A, int H) {
    const long nw = (long)(A + 1) * H, ne = nw + A + 1;
    const long e = (long)blockIdx.x * WA_THREADS + threadIdx.x;
    if (e >= ne) return;
    float* dst = e < nw ? (e < (long)A * H ? gWa + e : gwc + (e - (long)A * H)) : ((e - nw) < A ? gba + (e - nw) : gbc);
    *dst += gtab[e];
}

// dE1[q, n] += sum over the frames b with goal[b] == q, b ascending, of sum_p dm1[(b*S + p)*N + n]: the goal-embedding scatter
// of the unfused encoder tail in a fixed order (one workgroup per goal id, one thread per column; ids outside the table are
// skipped).  The float-atomic scatter it stands in for made two learn passes differ in the last bits.
__global__ __launch_bounds__(128) void wa_group_sum_kernel(const float* __restrict__ dm1, const int* __restrict__ goal,
                                                           float* __restrict__ dE1, int S, int N, long B) {
    const int q = blockIdx.x;
    for (int n = threadIdx.x; n < N; n += blockDim.x) {
        float acc = 0.f;
        for (long b = 0; b < B; ++b) {
            if (goal[b] != q) continue;                              // (uniform over the workgroup)
            const float* p = dm1 + b * S * N + n;
            float s = 0.f;
            for (int k = 0; k < S; ++k) s += p[(long)k * N];
            acc += s;
        }
        dE1[(long)q * N + n] += acc;
    }
}

}  // namespace

// policy.hip's learn pass of a handle with more than 7 actions: the packed heads table, its gradient, the ordered goal scatter
void ec_heads_pack_launch(const float* Wa, const float* ba, const float* wc, const float* bc, float* tab, int A, int H, hipStream_t s) {
    const long ne = (long)(A + 1) * H + A + 1;
    hipLaunchKernelGGL(wa_heads_pack_kernel, dim3((unsigned)((ne + WA_THREADS - 1) / WA_THREADS)), dim3(WA_THREADS), 0, s, Wa, ba, wc, bc,
                       tab, A, H);
}
void ec_heads_unpack_add_launch(const float* gtab, float* gWa, float* gba, float* gwc, float* gbc, int A, int H, hipStream_t s) {
    const long ne = (long)(A + 1) * H + A + 1;
    hipLaunchKernelGGL(wa_heads_unpack_add_kernel, dim3((unsigned)((ne + WA_THREADS - 1) / WA_THREADS)), dim3(WA_THREADS), 0, s, gtab,
                       gWa, gba, gwc, gbc, A, H);
}
void ec_goal_group_sum_launch(const float* dm1, const int* goal, float* dE1, int S, int N, long B, int num_goals, hipStream_t s) {
    hipLaunchKernelGGL(wa_group_sum_kernel, dim3((unsigned)num_goals), dim3(128), 0, s, dm1, goal, dE1, S, N, B);
}

// policy.hip's act step calls this for handles with more than 7 actions (ec_policy_act_ex); ec_heads_wide is its C-ABI face.
int ec_heads_wide_launch(const float* hs, const float* Wa, const float* ba, const float* wc, const float* bc, float* hv, long B, int H,
                         int A, long long* actions, float* logp, float* values, int greedy, uint64_t seed, uint64_t step,
                         int first_actor, const long long* expert_actions, const float* expert_mask, float force_p, hipStream_t s) {
    const size_t lds = ((size_t)WA_ROWS * H + 2 * WA_ROWS * WA_LD) * sizeof(float);
    if (lds > 64 * 1024) return EC_ERR_UNSUPPORTED;               // (the default dynamic-LDS limit: H up to 3576)
    const bool force = actions && expert_actions && force_p > 0.f;
    const WaSelect sel{actions, logp, values, seed, step, first_actor, greedy, force ? expert_actions : nullptr,
                       force ? expert_mask : nullptr, force_p};
    hipLaunchKernelGGL(wa_heads_kernel, dim3((unsigned)((B + WA_ROWS - 1) / WA_ROWS)), dim3(WA_THREADS), lds, s, hs, Wa, ba, wc, bc, hv,
                       B, H, A, sel);
    return EC_OK;
}

extern "C" int ec_heads_wide(const float* hs, const float* Wa, const float* ba, const float* wc, const float* bc, float* hv, long B,
                             int H, int A, int64_t* actions, float* logp, float* values, int greedy, uint64_t seed, uint64_t step,
                             int first_actor, const int64_t* expert_actions, const float* expert_mask, float force_p,
                             ec_stream_t stream) {
    if (!hs || !Wa || !ba || !wc || !bc || !hv) return EC_ERR_ARG;
    if (actions && !logp) return EC_ERR_ARG;
    if ((expert_actions != nullptr) != (expert_mask != nullptr)) return EC_ERR_ARG;
    if (!(force_p >= 0.f && force_p <= 1.f)) return EC_ERR_ARG;    // (NaN included)
    if (!expert_actions && force_p != 0.f) return EC_ERR_ARG;
    if (expert_actions && (greedy || !actions)) return EC_ERR_ARG;   // forcing belongs to the sampling act step
    if (B <= 0 || H <= 0 || (H & 3) || A < 1 || A > WA_MAX_A || first_actor < 0) return EC_ERR_SHAPE;
    const int rc = ec_heads_wide_launch(hs, Wa, ba, wc, bc, hv, B, H, A, (long long*)actions, logp, values, greedy, seed, step,
                                        first_actor, (const long long*)expert_actions, expert_mask, force_p, (hipStream_t)stream);
    if (rc != EC_OK) return rc;
    EC_CHECK_LAUNCH();
    return EC_OK;
}

extern "C" int ec_ppo_loss_wide_scratch_doubles(void) { return 4 * WP_MAX_BLOCKS + 1; }

extern "C" int ec_ppo_loss_wide(const float* hv, const int64_t* actions, const float* old_logp, const float* old_values,
                                const float* returns, const float* norm_adv, float* dhv, double* sums4, double* scratch, long B,
                                int A, float clip, float value_clip, float vcoef, float ecoef, float grad_scale,
                                ec_stream_t stream) {
    if (!hv || !actions || !old_logp || !old_values || !returns || !norm_adv || !dhv || !sums4 || !scratch) return EC_ERR_ARG;
    if (B <= 0 || A < 1 || A > WA_MAX_A) return EC_ERR_SHAPE;
    hipStream_t s = (hipStream_t)stream;
    const long per = (B + WP_MAX_BLOCKS - 1) / WP_MAX_BLOCKS;
    const long chunk = per > WP_ROWS_WAVE ? per : WP_ROWS_WAVE;      // contiguous rows of one block
    const unsigned blocks = (unsigned)((B + chunk - 1) / chunk);
    (void)hipMemsetAsync(scratch + WP_TICKET, 0, sizeof(double), s);   // the ticket counter
    hipLaunchKernelGGL(wa_ppo_loss_kernel, dim3(blocks), dim3(WA_THREADS), 0, s, hv, (const long long*)actions, old_logp, old_values,
                       returns, norm_adv, dhv, sums4, scratch, B, A, chunk, clip, value_clip, vcoef, ecoef, grad_scale);
    EC_CHECK_LAUNCH();
    return EC_OK;
}
