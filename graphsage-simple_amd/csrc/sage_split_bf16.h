// The exact three-term bf16 split of an fp32 value and what goes with it, shared by the kernels that contract on the bf16 matrix pipe
// with fp32 accuracy (sage_dense.hip: dense_bf16x3_kernel; sage_layer1_phase.hip: the phase-sliced layer 1).
#pragma once
#include "sage_internal.h"

#ifdef __HIPCC__
namespace sage_split_detail {

using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using bf16x4 = __attribute__((ext_vector_type(4))) __bf16;

// |x| >= 2^127, +-Inf or NaN (exponent field 254 or 255): the three-term split is not exact there -- RNE to bf16 can
// round the first term up to Inf, and Inf - Inf poisons the remainders -- so a tile (or a weight slice) that holds such a
// value is recomputed by a plain fp32 fma chain with torch.mm's Inf / NaN behaviour.
__device__ inline bool huge4(const f32x4 x) {
    bool h = false;
#pragma unroll
    for (int e = 0; e < 4; ++e) h |= (__float_as_uint(x[e]) & 0x7F800000u) >= 0x7F000000u;
    return h;
}

__device__ inline void split3(const f32x4 x, bf16x4& hi, bf16x4& mid, bf16x4& lo) {
    hi = __builtin_convertvector(x, bf16x4);
    const f32x4 r1 = x - __builtin_convertvector(hi, f32x4);
    mid = __builtin_convertvector(r1, bf16x4);
    const f32x4 r2 = r1 - __builtin_convertvector(mid, f32x4);
    lo = __builtin_convertvector(r2, bf16x4);
}

// Block barrier for data exchanged through LDS only.  __syncthreads() carries a workgroup-scope fence, and on gfx9 a release
// fence is `s_waitcnt vmcnt(0)`: it DRAINS every global load in flight -- the W slice (24 KiB per wave) requested in the
// prologue, the next tile's rows requested before the MFMA loop -- at each of the two barriers per tile.  Here only the LDS
// queue is waited for; the compiler still waits for a load where its value is used.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// One 16-k step of the split contraction: the six products whose terms reach 2^-24 |x||w|, smallest first.  a* = planes of the rows
// (lo, mid, hi), b[0..2] = planes of W (hi, mid, lo) in the register order of sage_prepare_weights.
__device__ __forceinline__ f32x16 mfma_bf16x3_step(const bf16x8 ah, const bf16x8 am, const bf16x8 al, const bf16x8 (&b)[3], f32x16 acc) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, b[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, b[2], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, b[1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, b[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, b[1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, b[0], acc, 0, 0, 0);
    return acc;
}

}  // namespace sage_split_detail
#endif
