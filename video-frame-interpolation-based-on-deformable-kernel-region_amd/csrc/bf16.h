// bf16.h -- bfloat16 storage as the kernels handle it: 16-bit patterns widened exactly on load, float32 arithmetic, one
// rounding to nearest even on store (correlation_bf16.hip, pwc_warp_bf16.hip, gradacc.hip).
#pragma once
#include "vfi_common.h"

namespace vfi {

typedef unsigned short bf16_t;                                  // the storage bits
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float bf16_widen(bf16_t v) { return __uint_as_float((unsigned)v << 16); }
// two floats to two bfloat16, round to nearest even, NaN stays NaN: one v_cvt_pk_bf16_f32
__device__ __forceinline__ unsigned bf16_pack_rne(float lo, float hi) {
    return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{lo, hi}, bf16x2));
}
__device__ __forceinline__ bf16_t bf16_rne(float v) { return (bf16_t)(bf16_pack_rne(v, 0.0f) & 0xffffu); }

// Two horizontally adjacent elements of a row, p[0] in the low half and p[1] in the high half: one 4-byte access where p is
// 4-byte aligned and the pair is inside the row (`pair`), 2-byte accesses otherwise (a lone element: the high half is 0 on
// load and dropped on store).  The branch is around the whole access, so a caller's batch of loads stays a batch.
__device__ __forceinline__ bool bf16_pair_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }
__device__ __forceinline__ void bf16_store_pair(bf16_t* p, unsigned two, bool pair) {
    if (pair && bf16_pair_aligned(p)) {
        *reinterpret_cast<unsigned*>(p) = two;
    } else {
        p[0] = (bf16_t)(two & 0xffffu);
        if (pair) p[1] = (bf16_t)(two >> 16);
    }
}

}  // namespace vfi
