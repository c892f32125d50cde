// Episode bookkeeping of a rollout on the device: completed episodes, their returns, lengths and success flags.
//
// Restates what [U] allenai/allenact ~v0.5.0 keeps on the host -- a task's cumulative reward / num_steps_taken() / metrics()
// ["success"], folded by utils/tensor_utils.py ScalarMeanTracker into the `reward`, `ep_length`, `success` scalars of every log
// line -- for the rollout tensors the engine already holds in HBM.  It is what an evaluation run reports (the reference's
// readme_files/baselines_robothor_objectnav.md:66-68 `--eval`, baselines_habitat.md:89-97 `--run-type eval`,
// zeroshot_objectnav.md:20-27).  Conventions of ec_gae (ppo.hip): rewards [T,N], masks [T+1,N], masks[t+1,n] == 0 ends the
// episode that step t belongs to.
#include "common.h"

namespace {

constexpr int EP_BLOCK = 1024, EP_WAVES = EP_BLOCK / 64;

// ONE workgroup, one lane per actor (lanes on adjacent n: every row of [T,N] is read coalesced), chunks of EP_BLOCK actors
// when N exceeds the block.  Per chunk: a count pass (episodes each actor completes in this call), an exclusive scan of the
// counts over the block -- integers, wave scans then the waves' totals in wave order -- and the write pass, which walks the T
// steps in order (the fp32 return is the sequential sum a host loop forms), appends the actor's records at its scanned offset
// and gathers the totals in double.  Records come out actor-ascending, then t-ascending, whatever the scheduling.
__global__ __launch_bounds__(EP_BLOCK) void episode_stats_kernel(const float* __restrict__ rew, const float* __restrict__ msk,
                                                                 const float* __restrict__ succ, float* __restrict__ carry_ret,
                                                                 int* __restrict__ carry_len, double* __restrict__ totals,
                                                                 float* __restrict__ rec_f, int* __restrict__ rec_i, int cap,
                                                                 int* __restrict__ n_records, int T, int N) {
    __shared__ int wave_tot[EP_WAVES];
    __shared__ double red[EP_WAVES][5];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nr_in = *n_records;            // (read by every thread before the first barrier; written by thread 0 after the last)
    const long rec0 = nr_in > 0 ? nr_in : 0; // a negative count never becomes a negative record index
    long chunk_base = 0;                     // records of the chunks before this one (block-uniform)
    double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int n0 = 0; n0 < N; n0 += EP_BLOCK) {
        const int n = n0 + tid;
        const bool live = n < N;
        int cnt = 0;
        if (live)
            for (int t = 0; t < T; ++t) cnt += (msk[(long)(t + 1) * N + n] == 0.f) ? 1 : 0;
        // exclusive scan of cnt over the block
        int inc = cnt;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(inc, o, 64);
            if (lane >= o) inc += up;
        }
        if (lane == 63) wave_tot[wave] = inc;
        __syncthreads();
        int before = 0, chunk_total = 0;
        for (int w = 0; w < EP_WAVES; ++w) {
            const int v = wave_tot[w];
            if (w < wave) before += v;
            chunk_total += v;
        }
        long slot = rec0 + chunk_base + before + (inc - cnt);
        if (live) {
            float ret = carry_ret[n];
            int len = carry_len[n];
            for (int t = 0; t < T; ++t) {
                ret += rew[(long)t * N + n];
                len += 1;
                if (msk[(long)(t + 1) * N + n] == 0.f) {
                    const float sc = succ ? succ[(long)t * N + n] : 0.f;
                    acc[0] += 1.0;
                    acc[1] += (double)ret;
                    acc[2] += (double)ret * (double)ret;
                    acc[3] += (double)len;
                    acc[4] += (double)sc;
                    if (rec_f && slot < cap) {
                        rec_f[slot * 2 + 0] = ret;
                        rec_f[slot * 2 + 1] = sc;
                        rec_i[slot * 3 + 0] = n;
                        rec_i[slot * 3 + 1] = t;
                        rec_i[slot * 3 + 2] = len;
                    }
                    ++slot;
                    ret = 0.f;
                    len = 0;
                }
            }
            carry_ret[n] = ret;
            carry_len[n] = len;
        }
        chunk_base += chunk_total;
        __syncthreads();                     // wave_tot is rewritten by the next chunk
    }
    ec_block_sum<5, EP_WAVES>(acc, red);     // the fixed-order block reduction of ppo.hip's sums (common.h); thread 0 holds the totals
    if (tid == 0) {
#pragma unroll
        for (int i = 0; i < 5; ++i) totals[i] += acc[i];
        const long nr = rec0 + chunk_base;
        *n_records = (int)(nr > 0x7fffffffL ? 0x7fffffffL : nr);
    }
}

}  // namespace

extern "C" int ec_episode_stats(const float* rewards, const float* masks, const float* success, float* carry_ret,
                                int32_t* carry_len, double* totals5, float* rec_f, int32_t* rec_i, int cap, int32_t* n_records,
                                int T, int N, ec_stream_t stream) {
    if (!rewards || !masks || !carry_ret || !carry_len || !totals5 || !n_records) return EC_ERR_ARG;
    if ((rec_f == nullptr) != (rec_i == nullptr)) return EC_ERR_ARG;      // the two record buffers go together
    if (T <= 0 || N <= 0 || cap < 0) return EC_ERR_SHAPE;
    hipLaunchKernelGGL(episode_stats_kernel, dim3(1), dim3(EP_BLOCK), 0, (hipStream_t)stream, rewards, masks, success, carry_ret,
                       carry_len, totals5, rec_f, rec_i, rec_f ? cap : 0, n_records, T, N);
    EC_CHECK_LAUNCH();
    return EC_OK;
}
