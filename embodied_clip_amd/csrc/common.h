// Shared device helpers for the gfx950 (CDNA4, wave64) kernels of the
// embodied-clip hot path.  HIP only -- no CUDA compatibility layer.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "../../include/ec_amd.h"

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef short s16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x16_t __attribute__((ext_vector_type(16)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));

#define EC_WAVE 64

__device__ __forceinline__ uint16_t ec_f2bf(float f) {
    // round-to-nearest-even fp32 -> bf16 (finite inputs)
    uint32_t u = __float_as_uint(f);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
__device__ __forceinline__ float ec_bf2f(uint16_t h) { return __uint_as_float(((uint32_t)h) << 16); }
typedef __bf16 ec_bf16x2_t __attribute__((ext_vector_type(2)));
typedef float ec_f32x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t ec_pack2(float lo, float hi) {
    // native conversion: one v_cvt_pk_bf16_f32 (round-to-nearest-even) for the pair
    ec_f32x2_t v = {lo, hi};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, ec_bf16x2_t));
}
__device__ __forceinline__ float ec_lo(uint32_t p) { return __uint_as_float(p << 16); }
__device__ __forceinline__ float ec_hi(uint32_t p) { return __uint_as_float(p & 0xffff0000u); }

// fp32 -> three bf16 planes (leading bits, then two residuals): x == p0 + p1 + p2 to ~2^-24; four values at a time
__device__ __forceinline__ void ec_split3x4(const float (&x)[4], uint2& p0, uint2& p1, uint2& p2) {
    p0.x = ec_pack2(x[0], x[1]); p0.y = ec_pack2(x[2], x[3]);
    const float r0 = x[0] - ec_lo(p0.x), r1 = x[1] - ec_hi(p0.x), r2 = x[2] - ec_lo(p0.y), r3 = x[3] - ec_hi(p0.y);
    p1.x = ec_pack2(r0, r1); p1.y = ec_pack2(r2, r3);
    p2.x = ec_pack2(r0 - ec_lo(p1.x), r1 - ec_hi(p1.x)); p2.y = ec_pack2(r2 - ec_lo(p1.y), r3 - ec_hi(p1.y));
}

// CategoricalDistr.sample() + log_prob() of one row of logits ([U] allenact base_abstractions/distributions.py): inverse CDF on a
// counter-based uniform keyed by (seed, step, GLOBAL actor id).  Shared by sample_kernel (ppo.hip) and the act step's heads
// launch (policy.hip: ec_policy_act) -- the same arithmetic, so the two routes sample identical actions.
__device__ __forceinline__ uint64_t ec_mix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// log-sum-exp of one row of logits: the normaliser of log_prob(), shared by the sampling and the greedy selection below
template <class RowFn>
__device__ __forceinline__ float ec_lse_row(RowFn row, int A) {
    float mx = -INFINITY;
    for (int k = 0; k < A; ++k) mx = fmaxf(mx, row(k));
    float se = 0.f;
    for (int k = 0; k < A; ++k) se += expf(row(k) - mx);
    return mx + logf(se);
}
// CategoricalDistr.mode() + log_prob() of one row ([U] the same distributions.py: `self._param.argmax(dim=-1)`): the FIRST index
// of the maximal logit (the tie rule numpy.argmax documents), evaluation's deterministic action.  Shared by mode_kernel (ppo.hip)
// and the act step's heads launch (ec_policy_act_greedy).
template <class RowFn>
__device__ __forceinline__ void ec_mode_row(RowFn row, int A, int& a_out, float& logp_out) {
    const float lse = ec_lse_row(row, A);
    int a = 0;
    float best = row(0);
    for (int k = 1; k < A; ++k) {
        const float v = row(k);
        if (v > best) { best = v; a = k; }
    }
    a_out = a;
    logp_out = best - lse;
}
template <class RowFn>
__device__ __forceinline__ void ec_sample_row(RowFn row, int A, uint64_t seed, uint64_t step, uint64_t global_actor, int& a_out,
                                              float& logp_out) {
    const float lse = ec_lse_row(row, A);
    const uint64_t h = ec_mix64(ec_mix64(seed) ^ (step * 0x100000001B3ull + global_actor));
    const float u = (float)((h >> 40) * (1.0 / 16777216.0));   // [0,1) with 24 bits
    float cdf = 0.f;
    int a = A - 1;
    for (int k = 0; k < A; ++k) {
        cdf += expf(row(k) - lse);
        if (u < cdf) { a = k; break; }
    }
    a_out = a;
    logp_out = row(a) - lse;
}

// the stream constant of the teacher-forcing uniform ("teachFor"): another draw than ec_sample_row makes for the same key.
// Shared by il_teacher_force_kernel (imitation.hip) and the wide heads launch (wide_actions.hip).
constexpr uint64_t IL_TF_STREAM = 0x7465616368466f72ull;

// Block reduction of up to NV doubles in a FIXED order (wave butterflies, then the waves' sums in wave order): thread 0 returns
// the totals.  No atomics in the reductions that use it (round 6): a floating-point atomicAdd per block made the advantage
// statistics, the loss sums and the gradient norm depend on the order the blocks happened to retire in -- two runs from one
// seed differed in the last bits, and Adam's sign-like steps amplify that.  Shared by ppo.hip and episode.hip.
__device__ __forceinline__ double ec_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}
template <int NV, int NWAVES>
__device__ __forceinline__ void ec_block_sum(double (&v)[NV], double (*red)[NV]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const double s = ec_wave_sum(v[i]);
        if (lane == 0) red[wave][i] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            double t = 0.0;
            for (int w = 0; w < NWAVES; ++w) t += red[w][i];
            v[i] = t;
        }
    }
}

// Bijective XCD-aware remap of a linear block id (cdna guide T1): the
// dispatcher places block b on XCD b % 8; give each XCD a contiguous chunk of
// the logical tile space so neighbouring tiles share an L2.
__device__ __forceinline__ unsigned ec_xcd_remap(unsigned bid, unsigned nwg) {
    const unsigned nx = 8;
    if (nwg < nx * 2) return bid;
    unsigned xcd = bid % nx, q = nwg / nx, r = nwg % nx;
    unsigned base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + bid / nx;
}

static inline int ec_ilog2(int v) {
    int l = 0;
    while ((1 << l) < v) ++l;
    return l;
}

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is PER DEVICE: one flag bit per device ordinal.  Usage:
//     if (auto g = ec_attr_needed(done)) { hipFuncSetAttribute(...); }
// The guard publishes the device's bit when it goes out of scope, i.e. AFTER the attribute call has returned: a second
// thread on the same device either sees the bit (the attribute is in force) or sets the attribute itself (idempotent) --
// it can never skip the call and launch with the old LDS limit.
struct ec_attr_guard {
    std::atomic<uint64_t>* a;
    uint64_t bit;
    explicit operator bool() const { return a != nullptr; }
    ec_attr_guard(std::atomic<uint64_t>* a_, uint64_t b_) : a(a_), bit(b_) {}
    ec_attr_guard(const ec_attr_guard&) = delete;
    ec_attr_guard& operator=(const ec_attr_guard&) = delete;
    ~ec_attr_guard() { if (a) a->fetch_or(bit, std::memory_order_release); }
};
static inline ec_attr_guard ec_attr_needed(std::atomic<uint64_t>& done) {
    int d = 0;
    (void)hipGetDevice(&d);
    const uint64_t bit = 1ull << (d & 63);
    if (done.load(std::memory_order_acquire) & bit) return ec_attr_guard(nullptr, 0);
    return ec_attr_guard(&done, bit);
}

// Fewest 256-row output tiles for which the conv / GEMM dispatch takes the 8-wave kernel (conv_igemm.hip conv_route).
// A property of the encoder HANDLE (ec_rn50_set_conv8_min_tiles / ec_vit_set_conv8_min_tiles), in force for the calling
// thread while that handle's forward issues its launches; everything else sees the default.
constexpr int EC_CONV8_MIN_TILES_DEFAULT = 150;
extern thread_local int ec_tls_conv8_min_tiles;
struct ec_min_tiles_scope {
    int prev;
    explicit ec_min_tiles_scope(int n) : prev(ec_tls_conv8_min_tiles) { ec_tls_conv8_min_tiles = n > 0 ? n : EC_CONV8_MIN_TILES_DEFAULT; }
    ec_min_tiles_scope(const ec_min_tiles_scope&) = delete;
    ~ec_min_tiles_scope() { ec_tls_conv8_min_tiles = prev; }
};

// Once-per-workgroup staging loops (weights -> LDS).  Written as `for (idx = tid; ...) lds[f(idx)] = global[g(idx)]` hipcc
// emits load -> s_waitcnt vmcnt(0) -> ds_write per iteration: TOTAL / NT serial L2 round trips at the head of EVERY
// launch (18 of them, ~15 us, in the narrow 3x3 kernels -- round-3 EC_ROWS_DBG ablation).  Here all of a thread's loads
// are issued before its first store (compile-time trip count, fully unrolled; the ragged last pass re-reads the last
// valid element and only its STORE is predicated, so no load sits behind an exec-masked branch).
template <int TOTAL, int NT, class T, class LoadFn, class StoreFn>
__device__ __forceinline__ void ec_stage_all(int tid, LoadFn load, StoreFn store) {
    constexpr int IT = (TOTAL + NT - 1) / NT;
    T v[IT];
#pragma unroll
    for (int i = 0; i < IT; ++i) {
        int idx = tid + i * NT;
        if (TOTAL % NT != 0) idx = idx < TOTAL ? idx : TOTAL - 1;
        v[i] = load(idx);
    }
#pragma unroll
    for (int i = 0; i < IT; ++i) {
        const int idx = tid + i * NT;
        if (TOTAL % NT == 0 || idx < TOTAL) store(idx, v[i]);
    }
}

// ---- library configuration -------------------------------------------------------------------------------------------
// Every tuning / experiment switch of the library, read from the environment ONCE (first use) into one immutable
// struct; the dispatch functions read fields of ec_config() instead of keeping getenv-initialised statics each.
// ec_config_hash() goes into ec_rn50_plan_hash / ec_vit_plan_hash, so a profile under profiles/ names the switch
// settings it was measured with.  DESIGN.md section 5.1 documents each variable.
struct EcConfig {
    // --- encoder: selection between ADOPTED kernel paths (each one is exercised by a parity test) ---
    int conv_narrow;      // EC_CONV_NARROW   (3)   narrow 3x3 kernels: 0 off, 1 gather (32 ch), 2 gather (also 64 ch), 3 row tiles
    int conv_rowsn;       // EC_CONV_ROWSN    (1)   multi-row tiles for the un-pooled narrow 3x3 layers (0: single-row tiles)
    int conv_big;         // EC_CONV_BIG      (1)   0 no conv_igemm8, 1 where measured faster, 4 wherever it applies (tests)
    long conv8_min_tiles; // EC_CONV8_MIN_TILES (0) overrides the handles' dispatch threshold when > 0
    int conv8_bn128;      // EC_CONV8_BN128   (0)   1 with EC_CONV_BIG=4: force 128-wide tiles; -1: layer-2 3x3 convs stay on the 4-wave kernel
    int conv8_longseg;    // EC_CONV8_LONGSEG (1)   conv_igemm8, 128-wide tiles: two segments per K-tile, three LDS stages (0: four segments)
    int conv_t224;        // EC_CONV_T224     (2)   196-of-224-row tiles: 0 off, 1 everywhere, 2 rule, 3 also 256-tile launches
    int conv_t64;         // EC_CONV_T64      (150) launches with fewer 128x128 tiles use 64x64 tiles
    int conv_ring;        // EC_CONV_RING     (1)   ring pipeline for launches with <= 1-2 workgroups per CU (0: single-stage loop)
    int conv_regw;        // EC_CONV_REGW     (1)   register-weight 1x1 kernel
    int rn50_fuse;        // EC_RN50_FUSE     (1)   fused layer-1 / layer-2 block boundaries in the trunk plan
    int rn50_bneck;       // EC_RN50_BNECK    (128) launches of at least this many frames run layer3.1-5 as fused bottleneck launches (conv_bneck.hip); 0: never
    int rn50_bneck3;      // EC_RN50_BNECK3   (1)   the fused bottleneck launches include conv1 (the whole block in one launch)
    int rn50_img3;        // EC_RN50_IMG3     (1)   small launches run the 14x14x256 (<= 32 frames) / 7x7x512 (<= 64 frames) 3x3 convs on the image-resident K-split kernel
    int rn50_dscat;       // EC_RN50_DSCAT    (1)   stride-2 Bottlenecks of layers 3-4: conv3 and the downsample conv as ONE GEMM over the concatenated K axis (pooled conv2 output | pooled block input)
    int rn50_poolout;     // EC_RN50_POOLOUT  (1)   layer 2's last conv3 also emits AvgPool2d(2) of its output (the pooled block input of layer3.0's K-concatenated GEMM): no pooling pass
    // --- policy / update ---
    int gemm_no_x3;       // EC_GEMM_NO_X3    (0)   policy GEMMs on the fp32 MFMA instead of bf16x3
    int gemm_bwd3;        // EC_GEMM_BWD3     (0)   ec_policy_backward's large gradient GEMMs on three of the six bf16x3 products (also on under EC_POLICY_FAST)
    int policy_fast;      // EC_POLICY_FAST   (1)   learn pass: the backward's large gradient GEMMs on the three leading bf16x3 products, the compressor conv over the
                          //                        stored features and its weight gradient on the two leading planes of the fp32 operand (16 mantissa bits; products
                          //                        accurate to 2^-16 .. 2^-17 -- finer than the TF32 the reference's torch 1.7 uses for fp32 matmuls on Ampere);
                          //                        0: every policy GEMM fp32-exact (six products / three planes)
    int act_split;        // EC_ACT_SPLIT     (1)   act step: K-split kernels for its two long-K GEMMs
    int tail_fused;       // EC_TAIL_FUSED    (1)   compressor tail / combiner fused kernels
    int gru_fused;        // EC_GRU_FUSED     (2)   0 GEMM + gate kernels, 1 fused 32x32-tile step kernels, 2 + 16x16-tile kernels in the update
    int c1_pingpong;      // EC_C1_PINGPONG   (1)   compressor conv 1 over stored features on the 8-wave kernel
    int dw1_tr;           // EC_DW1_TR        (1)   dW1 on the transpose-read kernel
    int wih_perm;         // EC_WIH_PERM      (1)   learn pass: re-ordered weight_ih instead of activation transposes
    int dw_transposed;    // EC_DW_TRANSPOSED (1)   GRU weight-gradient GEMMs on transposed (K-contiguous) operands
    int rnn_stack;        // EC_RNN_STACK     (1)   act step of a multi-layer recurrent core: one launch per upper layer (rnn_stack.hip); 0: the general
                          //                        layer-by-layer route.  NOT part of ec_config_hash(): no single-layer plan reads it
    int pooled_act;       // EC_POOLED_ACT    (1)   act step of a pooled-embedding handle: pooled_fc_act_kernel + pooled_step0_kernel (pooled_net.hip);
                          //                        0: the general route.  NOT part of ec_config_hash(): no other handle's plan reads it
    int rgbd_joint;       // EC_RGBD_JOINT    (1)   ec_rn50_embed_rgbd: the RGB and the depth frames of a chunk in ONE pass of the plan at twice the frames;
                          //                        0: two passes, RGB then depth.  NOT part of ec_config_hash(): no plan reads it, only the pass count
    // --- ViT / text GEMMs (ec_gemm_bf16_ln8).  NOT part of ec_config_hash(): the profile summaries under profiles/ are keyed by the hash as it was ---
    int vit_wide;         // EC_VIT_WIDE      (1)   0: 128-wide tiles only, 2: 256-wide wherever N allows
    int vit_bm192;        // EC_VIT_BM192     (1)   0: no 192-row tiles
    int vit_cls_tail;     // EC_VIT_CLS_TAIL  (-1)  ec_vit_embed_cls: -1 the route the library's rule picks per (tokens, frames), 0 the general route
                          //                        (whole last block, then row 0), 1 the CLS-only last block (vit_cls.hip).  NOT part of
                          //                        ec_config_hash(); ec_vit_plan_hash mixes it in when it is set
};
// Fixed since round 5 (measured winners; the A/B numbers live in docs/experiments.md): 768 persistent workgroups, residual 1x1
// launches of K 512..2047 with < 100 256-wide tiles on 128-wide 8-wave tiles, low-fill limits 100 tiles / K >= 1024, ring-mode
// LDS-DMA pieces interleaved with the MFMAs, 128 x 128 ring tiles on 8 waves.
constexpr int EC_CONV8_LOWFILL = 100, EC_CONV8_LOWFILL_K = 1024;
const EcConfig& ec_config();          // api.hip
uint64_t ec_config_hash();            // FNV-1a over the fields above (all but vit_wide / vit_bm192)

// Library-internal entry points (C++ linkage, not part of include/ec_amd.h); EC_ERR_SHAPE from the first three = not handled
int ec_conv3x3_narrow(const void* in, const void* w, const float* bias, void* out, int B, int H, int W, int Cin, int Cout,
                      int pool, hipStream_t s);   // conv3x3_narrow.hip: resident-weight kernel for the narrow early 3x3 layers
int ec_conv1x1_regw(const void* a, const void* w, const float* bias, const void* res, void* y, long M, int K, int N, int act,
                    hipStream_t s);               // conv_pair.hip: register-weight kernel for a few bandwidth-bound 1x1 shapes
int ec_conv1x1_regw_pool(const void* a, const void* w, const float* bias, const void* res, void* y, void* y_pooled, int B, int H,
                         int W, int K, int N, int act, int ld_pooled, hipStream_t s);   // conv_pair.hip: ... also emitting AvgPool2d(2) of y
int ec_gemm_bf16a_xp(const void* A, const void* Wplanes, const float* bias, float* out, long M, int N, int K, int act, int planes,
                     ec_stream_t stream);         // conv_igemm.hip: ec_gemm_bf16a_x3 over the 2 or 3 leading weight planes
int ec_gemm_bf16_ln8(const void* A, const void* Wt, const float* bias, const void* res, void* out, int M, int N, int K, int act,
                     const float* ln_s, const float* ln_stats, int ln_np, float* stats_out, int* np_out,
                     ec_stream_t stream);         // conv_igemm.hip: the 8-wave GEMM with LayerNorm folded in / emitting its row records

int ec_heads_wide_launch(const float* hs, const float* Wa, const float* ba, const float* wc, const float* bc, float* hv, long B, int H,
                         int A, long long* actions, float* logp, float* values, int greedy, uint64_t seed, uint64_t step,
                         int first_actor, const long long* expert_actions, const float* expert_mask, float force_p,
                         hipStream_t s);           // wide_actions.hip: the heads of a wide action space + selection, one launch
// wide_actions.hip, the learn pass of a wide handle: [Wa; wc | ba; bc] as one table ((A + 1) * H + A + 1 floats), the table's
// gradient added onto the four gradient tensors, and the goal-embedding scatter of the unfused tail in a fixed order
void ec_heads_pack_launch(const float* Wa, const float* ba, const float* wc, const float* bc, float* tab, int A, int H, hipStream_t s);
void ec_heads_unpack_add_launch(const float* gtab, float* gWa, float* gba, float* gwc, float* gbc, int A, int H, hipStream_t s);
void ec_goal_group_sum_launch(const float* dm1, const int* goal, float* dE1, int S, int N, long B, int num_goals, hipStream_t s);

// prev_action.hip: the previous-action embedding.  Row of the table that frame b selects, or -1.  null: row 0 is the null token
// (an episode's first step, masks == 0) and action a
// is row a + 1 -- ((prev + 1) * masks).long() for masks in {0, 1}; otherwise the action itself.  Compared as 64 bits: 1 << 32
// is no action 0.
__device__ __forceinline__ int ec_pa_index(const long long* __restrict__ prev, const float* __restrict__ masks, long b, int null_token,
                                        int A) {
    const long long a = prev[b];
    if (null_token) {
        if (masks[b] == 0.f) return 0;
        return (a >= -1 && a < A) ? (int)a + 1 : -1;
    }
    return (a >= 0 && a < A) ? (int)a : -1;
}

// The act step's input projection (policy.hip gi_act_kernel<NW>: its header comment describes the tiling) as a body shared with
// prev_action.hip's instance, which adds the previous action's row of the table PT in the fold, behind the bias (PA).  The PA = false
// instantiation is gi_act_kernel's arithmetic as it was.
struct ec_gi_act_pa { const float* pt; const long long* prev; const float* masks; int null_token, A; };
// RELU (pooled_net.hip's instance, PA = false only): max(. + bias, 0) is stored -- visual_fc of the pooled-embedding net.
template <int NW, bool PA, bool RELU = false>
__device__ __forceinline__ void ec_gi_act_body(const float* __restrict__ x, const float* __restrict__ W, const float* __restrict__ bias,
                                               float* __restrict__ gi, int N, int K, int NO, const ec_gi_act_pa pax) {
    __shared__ float part[NW][32][33];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 31, hh = lane >> 5;
    const int j0 = blockIdx.x * 32, n0 = blockIdx.y * 32;
    const int kw = K / NW, k0 = wave * kw;
    const float* pa = x + (long)min(n0 + i, N - 1) * K + k0 + 4 * hh;        // (rows past N are computed on a clamped row, never stored)
    // W in fragment order (frag_pack_f32_kernel): group g of column block cb is the contiguous 1-KB unit (cb K/8 + g)
    const f32x4_t* pbf = reinterpret_cast<const f32x4_t*>(W) + ((long)blockIdx.x * (K / 8) + k0 / 8) * 64 + lane;
    f32x16_t acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    constexpr int U = 7;                                          // groups of 8 k in flight
    for (int kb = 0; kb < kw; kb += 8 * U) {
        f32x4_t a[U], b[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int kk = min(kb + 8 * u, kw - 8);                // (kw is a multiple of 8; a clamped group is skipped below)
            a[u] = *reinterpret_cast<const f32x4_t*>(pa + kk);
            b[u] = pbf[(kk >> 3) * 64];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (kb + 8 * u < kw) {
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u][0], b[u][0], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u][1], b[u][1], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u][2], b[u][2], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u][3], b[u][3], acc, 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) part[wave][(r & 3) + 8 * (r >> 2) + 4 * hh][i] = acc[r];     // C/D layout: row = actor, column = lane & 31
    __syncthreads();
    for (int e = tid; e < 32 * 32; e += NW * 64) {
        const int row = e >> 5, col = e & 31;
        float v = part[0][row][col];
#pragma unroll
        for (int w2 = 1; w2 < NW; ++w2) v += part[w2][row][col];
        if (!PA) {
            if (n0 + row < N) {
                const float o = v + (bias ? bias[j0 + col] : 0.f);
                gi[(long)(n0 + row) * NO + j0 + col] = RELU ? fmaxf(o, 0.f) : o;
            }
        } else if (n0 + row < N) {
            float o = v + (bias ? bias[j0 + col] : 0.f);
            const int r = ec_pa_index(pax.prev, pax.masks, n0 + row, pax.null_token, pax.A);
            if (r >= 0) o += pax.pt[(long)r * NO + j0 + col];
            gi[(long)(n0 + row) * NO + j0 + col] = o;
        }
    }
}

// ... and its launches for policy.hip: the table PT = Emb . Wa^T, gi[b] += PT[idx[b]], and the binned ordered gradient (scratch:
// ec_pa_grad_scratch_floats floats; its first R * G hold dPT afterwards)
void ec_pa_table_launch(const float* emb, const float* w, long ld, int col0, float* pt, int R, int G, int E, hipStream_t s);
void ec_pa_add_launch(float* gi, const float* pt, const long long* prev, const float* masks, int null_token, int A, long B, int G,
                      hipStream_t s);
size_t ec_pa_grad_scratch_floats(long B, int G, int R);
// gi_act_kernel<nw>'s launch (nw = 7 | 8) with the table row added in the fold; rows [rows, cols] copied between two row strides
// (add == 0) or added (add == 1): weight_ih[:, :flat] as a dense copy, the dense gradient back onto the parameter's rows
void ec_pa_gi_act_launch(int nw, const float* x, const float* W, const float* bias, float* gi, int N, int K, int NO, ec_gi_act_pa pa,
                         hipStream_t s);
void ec_pa_rows_copy_launch(const float* in, int ld_in, float* out, int ld_out, int rows, int cols, int add, hipStream_t s);
void ec_pa_bins_launch(const float* dgi, const long long* prev, const float* masks, int null_token, int A, float* scratch, long B, int G,
                       hipStream_t s);      // the binned ordered sum alone: dPT [R, G] in front of the scratch
void ec_pa_grad_launch(const float* dgi, const long long* prev, const float* masks, int null_token, int A, const float* emb,
                       const float* w, long ld, int col0, float* demb, float* dw, float* scratch, long B, int G, int E, hipStream_t s);

// lstm.hip: the LSTM cell's step kernels for policy.hip's two recurrence() members (argument meanings: the kernels' headers).
// ec_lstm_hidden_ok: H % 32 == 0 and the forward step's two operand tiles fit the LDS (every H % 256 == 0; else H <= 608).
size_t ec_lstm_fwd_lds(int H);
bool ec_lstm_hidden_ok(int H);
void ec_lstm_fwd_launch(const float* gi, const float* whh, const float* bhh, const float* hprev, const float* cprev, long ld_prev,
                        const float* mask, float* hout, long ld_h, float* cout, long ld_c, float* hout2, long ld_h2, float* gates,
                        float* hp_s, float* cp_s, int N, int H, int gi_parts, long gi_pstride, hipStream_t s);
void ec_lstm_bwd_gates_launch(const float* dhs, float* carry_h, float* carry_c, const float* gates, const float* cs, const float* cp_s,
                              const float* mask, float* da, int N, int H, hipStream_t s);
void ec_lstm_bwd_fused_launch(const float* da_next, const float* whhT, const float* mask_next, const float* dhs, float* carry_c,
                              const float* gates, const float* cs, const float* cp_s, const float* mask, float* da, int N, int H,
                              hipStream_t s);
void ec_lstm_state_rows_launch(float* state, float* hpart, float* cpart, int N, int H, int split, hipStream_t s);

// rnn_stack.hip: one launch for an upper layer's act step -- input projection, recurrent projection and cell (argument meanings:
// the kernel's header).  gi != null: no x half, the projection as given (layer 0 of a GRU stack, states at a row pitch).
struct ec_rnn_stack_args {
    const float *x; long ld_x;
    const float *wih, *whh, *bih, *bhh;
    const float *hprev, *cprev; long ld_prev;
    const float* mask;
    float* hout; long ld_h;
    float* cout; long ld_c;
    float* hout2; long ld_h2;
    const float* gi; int gi_parts; long gi_pstride;
    int N, H;
};
void ec_rnn_stack_launch(int lstm, const ec_rnn_stack_args& a, hipStream_t s);

// pooled_net.hip: the pooled-embedding net's own launches for policy.hip (argument meanings: the kernels' headers).
//   tables: SV [G, K] and sb [G] from the sensor blocks of weight_ih_l0 (row stride ld, sensor i's block at column col0 + i * ed)
//   rows_add: gi[b] = (((gi[b] + sb) + gt[goal[b]]) + pt[row(b)]) + sum_k sv[:, k] sensors[b, k]; every part optional
//   sensor_grads: from dSV [G, K] and dsb [G], dW_ih[:, blk_i] += dSV_i W_i^T + dsb b_i^T, dW_i += W_ih[:, blk_i]^T dSV_i,
//   db_i += W_ih[:, blk_i]^T dsb -- one thread per output, ascending inner index
struct ec_pooled_sensors { int ns, k[3], K, ed; const float* w[3]; const float* b[3]; float* dw[3]; float* db[3]; };
struct ec_pooled_side {
    const float* sb; const float* gt; const long long* goal; int num_goals;
    const float* pt; const long long* prev; const float* masks; int null_token, A;
    const float* sv; const float* sens; int K;
};
void ec_pooled_tables_launch(const float* wih, long ld, int col0, const ec_pooled_sensors& sn, float* sv, float* sb, int G, hipStream_t s);
void ec_pooled_rows_add_launch(float* gi, const ec_pooled_side& sd, long B, int G, hipStream_t s);
void ec_pooled_sensor_grads_launch(const float* wih, float* dwih, long ld, int col0, const ec_pooled_sensors& sn, const float* dsv,
                                   const float* dsb, int G, hipStream_t s);
void ec_pooled_frag_pack_launch(const float* w, float* wfrag, int N, int K, hipStream_t s);
void ec_pooled_fc_act_launch(const float* e, const float* wfrag, const float* b, float* v, int N, int D, int H, hipStream_t s);
void ec_pooled_step0_launch(int lstm, const ec_rnn_stack_args& a, const ec_pooled_side& sd, hipStream_t s);

// two_view.hip: the two-view rearrangement net's front for policy.hip (argument meanings: the kernels' headers).
//   planes: [W_a; W_e] as three bf16 planes in fragment order (ec_tv_planes_floats floats; weight-derived)
//   fwd: v [B, H]; a [B, S2] the probabilities and act [B S2, A1 + H] the post-ReLU activations (attention columns first), each
//   stored if non-null -- what bwd reads, with ec_tv_bwd_scratch_floats floats of scratch; bwd ADDS onto the six gradients
struct ec_tv_shape { long B; int S2, C, H, A1; };
struct ec_tv_fwd_args {
    const uint16_t *u, *w; const void* wp;
    const float *be, *ba, *w2, *b2;
    float *v, *a, *act;
    long B; int S2, C, H, A1;
};
bool ec_tv_shape_ok(const ec_tv_shape& q);
size_t ec_tv_planes_floats(const ec_tv_shape& q);
size_t ec_tv_bwd_scratch_floats(const ec_tv_shape& q);
void ec_tv_pack_launch(const float* We, const float* Wa, void* planes, const ec_tv_shape& q, hipStream_t s);
void ec_tv_fwd_launch(const ec_tv_fwd_args& a, hipStream_t s);
void ec_tv_bwd_launch(const void* u, const void* w, const float* w2, const float* dv, const float* a, const float* act, float* scratch,
                      float* dWe, float* dbe, float* dWa, float* dba, float* dw2, float* db2, const ec_tv_shape& q, hipStream_t s);

// vit_cls.hip: the most keys cls_attn_kernel takes (vit.hip holds it equal to the general attention core's limit)
constexpr int EC_CLS_ATTN_MAX_TOKENS = 512;

#define EC_CHECK_LAUNCH()                             \
    do {                                                    \
        hipError_t e__ = hipGetLastError();                 \
        if (e__ != hipSuccess) return EC_ERR_LAUNCH;        \
    } while (0)
