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


// ---- navigation metrics ----------------------------------------------------------------------------------------------
// SPL, SoftSPL, the distance to the goal and the per-category rows of the result tables the reference points to (success and
// SPL on RoboTHOR ObjectNav; SPL, SoftSPL, distance to goal on Habitat; success and SPL per object type, 8 seen and 4 unseen,
// on readme_files/zeroshot_objectnav.md:20-48).  Restates [U] allenact's `spl_metric` (RoboTHOR ObjectNav task) and [U]
// habitat-lab's `SPL` / `SoftSPL` measures from their published descriptions -- neither source is pinned, so the operation
// order below (include/ec_amd.h spells it out) is this library's own and tests/_nav_episode_ref.py is its reference.
constexpr int NAV_COLS = 10, NAV_MAX_C = 64;
constexpr int NAV_LDS_MAX = EP_WAVES * NAV_MAX_C * NAV_COLS * (int)sizeof(double);   // 81920 B of the CU's 160 KB

// The shape of episode_stats_kernel (one workgroup, a lane per actor, count pass / scan / write pass per chunk of EP_BLOCK
// actors).  Row 0 of the totals is gathered as there: a lane's ten doubles, then ec_block_sum -- it does not depend on the
// categories, so a call with C = 0 gives the bits of row 0 of a call with them.  The category rows: every WAVE owns a [C][10]
// double table in LDS; at a step where lanes of the wave end an episode with an id in [0, C) the wave serves them one at a
// time, in lane order (ballot loop), the episode's fp32 values are read across to lane 0 and lane 0 alone adds them to the
// table -- one thread does every load and store of a table, so the order of the additions is the program's (t ascending, then
// lane, then chunk).  The waves' tables are folded in wave order at the end.  No atomics; ends are rare (1 step in 100).
__global__ __launch_bounds__(EP_BLOCK) void nav_episode_stats_kernel(
    const float* __restrict__ rew, const float* __restrict__ msk, const float* __restrict__ succ, const float* __restrict__ sdist,
    const float* __restrict__ d0s, const float* __restrict__ d1s, const int64_t* __restrict__ cat, int C,
    float* __restrict__ carry_ret, int* __restrict__ carry_len, float* __restrict__ carry_path, double* __restrict__ totals,
    float* __restrict__ rec_f, int* __restrict__ rec_i, int cap, int* __restrict__ n_records, int T, int N) {
    extern __shared__ double nav_tab[];      // [EP_WAVES][C][NAV_COLS]
    __shared__ int wave_tot[EP_WAVES];
    __shared__ double red[EP_WAVES][NAV_COLS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nr_in = *n_records;
    const long rec0 = nr_in > 0 ? nr_in : 0;
    double* tab = nav_tab + (long)wave * C * NAV_COLS;
    for (int i = lane; i < C * NAV_COLS; i += 64) tab[i] = 0.0;
    __syncthreads();
    long chunk_base = 0;
    double acc[NAV_COLS];
#pragma unroll
    for (int i = 0; i < NAV_COLS; ++i) acc[i] = 0.0;
    for (int n0 = 0; n0 < N; n0 += EP_BLOCK) {
        const int n = n0 + tid;
        const bool live = n < N;
        int cnt = 0;
        if (live)
            for (int t = 0; t < T; ++t) cnt += (msk[(long)(t + 1) * N + n] == 0.f) ? 1 : 0;
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
        float ret = live ? carry_ret[n] : 0.f, path = live ? carry_path[n] : 0.f;
        int len = live ? carry_len[n] : 0;
        for (int t = 0; t < T; ++t) {            // (every lane of a wave walks the steps together: the ballot below is wave-wide)
            bool end = false;
            if (live) {
                ret += rew[(long)t * N + n];
                path += sdist[(long)t * N + n];
                len += 1;
                end = msk[(long)(t + 1) * N + n] == 0.f;
            }
            float sc = 0.f, spl = 0.f, soft = 0.f, d0 = 0.f, d1 = 0.f;
            long c = -1;
            if (end) {
                sc = succ ? succ[(long)t * N + n] : 0.f;
                d0 = d0s[(long)t * N + n];
                if (d1s) d1 = d1s[(long)t * N + n];
                if (cat) c = cat[(long)t * N + n];
                if (d0 > 0.f) {
                    const float ratio = d0 / fmaxf(d0, path);
                    spl = sc > 0.f ? ratio : 0.f;
                    if (d1s) soft = fmaxf(0.f, 1.f - d1 / d0) * ratio;
                } else if (d0 == 0.f) {
                    spl = (sc > 0.f && path == 0.f) ? 1.f : 0.f;
                    if (d1s) soft = spl;
                }
                acc[0] += 1.0;
                acc[1] += (double)ret;
                acc[2] += (double)ret * (double)ret;
                acc[3] += (double)len;
                acc[4] += (double)sc;
                acc[5] += (double)spl;
                acc[6] += (double)soft;
                acc[7] += (double)d1;
                acc[8] += (double)path;
                acc[9] += d0 < 0.f ? 1.0 : 0.0;
                if (rec_f && slot < cap) {
                    float* rf = rec_f + slot * 7;
                    rf[0] = ret; rf[1] = sc; rf[2] = spl; rf[3] = soft; rf[4] = path; rf[5] = d1; rf[6] = d0;
                    int* ri = rec_i + slot * 4;
                    ri[0] = n; ri[1] = t; ri[2] = len; ri[3] = cat ? (int)c : -1;
                }
                ++slot;
            }
            if (C > 0) {
                const int ci = (end && c >= 0 && c < C) ? (int)c : -1;
                unsigned long long pending = __ballot(ci >= 0);
                while (pending) {                // wave-uniform
                    const int src = __ffsll((long long)pending) - 1;
                    pending &= pending - 1;
                    const int c_s = __shfl(ci, src, 64), len_s = __shfl(len, src, 64);
                    const float ret_s = __shfl(ret, src, 64), sc_s = __shfl(sc, src, 64), spl_s = __shfl(spl, src, 64),
                                soft_s = __shfl(soft, src, 64), d1_s = __shfl(d1, src, 64), path_s = __shfl(path, src, 64),
                                d0_s = __shfl(d0, src, 64);
                    if (lane == 0) {
                        double* row = tab + c_s * NAV_COLS;
                        row[0] += 1.0;
                        row[1] += (double)ret_s;
                        row[2] += (double)ret_s * (double)ret_s;
                        row[3] += (double)len_s;
                        row[4] += (double)sc_s;
                        row[5] += (double)spl_s;
                        row[6] += (double)soft_s;
                        row[7] += (double)d1_s;
                        row[8] += (double)path_s;
                        row[9] += d0_s < 0.f ? 1.0 : 0.0;
                    }
                }
            }
            if (end) {
                ret = 0.f;
                path = 0.f;
                len = 0;
            }
        }
        if (live) {
            carry_ret[n] = ret;
            carry_path[n] = path;
            carry_len[n] = len;
        }
        chunk_base += chunk_total;
        __syncthreads();                     // wave_tot is rewritten by the next chunk
    }
    ec_block_sum<NAV_COLS, EP_WAVES>(acc, red);      // (the waves' tables are complete and visible since the barrier that ended the last chunk)
    if (tid == 0) {
#pragma unroll
        for (int i = 0; i < NAV_COLS; ++i) totals[i] += acc[i];
        const long nr = rec0 + chunk_base;
        *n_records = (int)(nr > 0x7fffffffL ? 0x7fffffffL : nr);
    }
    for (int j = tid; j < C * NAV_COLS; j += EP_BLOCK) {
        double s = 0.0;
        for (int w = 0; w < EP_WAVES; ++w) s += nav_tab[(long)w * C * NAV_COLS + j];
        totals[NAV_COLS + j] += s;
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

extern "C" int ec_nav_episode_stats(const float* rewards, const float* masks, const float* success, const float* step_dist,
                                    const float* start_dist, const float* goal_dist, const int64_t* category, int C,
                                    float* carry_ret, int32_t* carry_len, float* carry_path, double* totals, float* rec_f,
                                    int32_t* rec_i, int cap, int32_t* n_records, int T, int N, ec_stream_t stream) {
    if (!rewards || !masks || !step_dist || !start_dist || !carry_ret || !carry_len || !carry_path || !totals || !n_records)
        return EC_ERR_ARG;
    if ((rec_f == nullptr) != (rec_i == nullptr)) return EC_ERR_ARG;      // the two record buffers go together
    if (T <= 0 || N <= 0 || cap < 0 || C < 0 || C > NAV_MAX_C) return EC_ERR_SHAPE;
    if ((category != nullptr) != (C > 0)) return EC_ERR_ARG;              // ids without rows to count them in, or rows without ids
    const size_t lds = (size_t)EP_WAVES * C * NAV_COLS * sizeof(double);
    static std::atomic<uint64_t> attr_done{0};
    if (auto g = ec_attr_needed(attr_done))
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(nav_episode_stats_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  NAV_LDS_MAX);
    hipLaunchKernelGGL(nav_episode_stats_kernel, dim3(1), dim3(EP_BLOCK), lds, (hipStream_t)stream, rewards, masks, success,
                       step_dist, start_dist, goal_dist, category, C, carry_ret, carry_len, carry_path, totals, rec_f, rec_i,
                       rec_f ? cap : 0, n_records, T, N);
    EC_CHECK_LAUNCH();
    return EC_OK;
}
