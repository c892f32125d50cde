// Shared by the layer-1 boundary kernels (conv_pair.hip, conv_pair_rebuild.hip): tile geometry, the swizzled LDS weight image and
// the software-pipelined LDS fragment stream.
#pragma once

#include <type_traits>
#include <utility>

#include "common.h"

namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));   // native vector: plain loads/stores, SROA-friendly
constexpr int PX = 32;         // pixels per wave tile
constexpr int NY = 256;        // channels of y
constexpr int KA = 64;         // channels of a0 / a1

__device__ __forceinline__ int pw_off(int row, int chunk) {   // 128-B rows, XOR swizzle on the 16-B chunk
    return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4);
}

// Software-pipelined LDS fragment stream for kernels that run ONE wave per SIMD: left to the compiler every MFMA gets its
// own `ds_read_b128 -> s_waitcnt lgkmcnt(0)` in front (it sinks operand reads to their use), i.e. the full LDS latency per
// MFMA with nothing to hide it.  Here the reads are inline asm, LEAD steps ahead of the MFMA that consumes them, and the
// waits carry the fragment register so the MFMA cannot be scheduled above its wait (LDS returns data in order:
// "lgkmcnt(n)" = all but the newest n have arrived; compiler-generated LDS traffic in between only makes the waits
// conservative).  addr(i): LDS byte address (VGPR) and immediate offset of step i; mma(i, frag) consumes it.
template <int I, int LEAD, class AddrFn>
__device__ __forceinline__ void lsm_issue(u32x4 (&ring)[LEAD], AddrFn& addr) {
    const auto a = addr(std::integral_constant<int, I>{});
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(ring[I % LEAD]) : "v"(a.first), "n"(decltype(a.second)::value));
}
template <int I, int NSTEP, int LEAD, class AddrFn, class MmaFn>
__device__ __forceinline__ void lsm_step(u32x4 (&ring)[LEAD], AddrFn& addr, MmaFn& mma) {
    if constexpr (I < NSTEP) {
        constexpr int after = (LEAD - 1 < NSTEP - 1 - I) ? LEAD - 1 : NSTEP - 1 - I;   // reads issued after read I
        asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(ring[I % LEAD]) : "n"(after));
        mma(std::integral_constant<int, I>{}, ring[I % LEAD]);
        if constexpr (I + LEAD < NSTEP) lsm_issue<I + LEAD, LEAD>(ring, addr);
        lsm_step<I + 1, NSTEP, LEAD>(ring, addr, mma);
    }
}
template <int I, int N, int LEAD, class AddrFn>
__device__ __forceinline__ void lsm_prologue(u32x4 (&ring)[LEAD], AddrFn& addr) {
    if constexpr (I < N) {
        lsm_issue<I, LEAD>(ring, addr);
        lsm_prologue<I + 1, N, LEAD>(ring, addr);
    }
}
template <int NSTEP, int LEAD, class AddrFn, class MmaFn>
__device__ __forceinline__ void lds_stream_mfma(AddrFn addr, MmaFn mma) {
    u32x4 ring[LEAD];
    lsm_prologue<0, (LEAD < NSTEP ? LEAD : NSTEP), LEAD>(ring, addr);
    lsm_step<0, NSTEP, LEAD>(ring, addr, mma);
}

}  // namespace
