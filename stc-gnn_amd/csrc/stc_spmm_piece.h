// Internal: the 16-byte piece of a feature row that one lane of an aggregation kernel moves and sums (stc_spmm_gather.h with stc_spmm.hip and
// stc_spmm_bf16.hip; stc_spmm_patch.hip), and the bf16 widen / pack of every bf16-storage kernel file (also stc_node_bf16.hip, stc_gates.hip,
// stc_x3_frag.h).
//
// A piece is four floats, or eight bf16 (bf16 storage, BASELINE configuration 5): bf16 values widen to fp32 exactly (a 16-bit shift), every
// product and the whole sum are fp32, one fmaf per entry from zero, and a result is rounded to bf16 ONCE at its store (round to nearest even,
// v_cvt_pk_bf16_f32).  Every aggregation kernel sums a row by this fmaf chain in the order of its entries: they agree bit for bit.
// Pieces travel as Raw whatever they hold; those read or written once go through stc_ld_once / stc_st_once (stc_common.h).
#pragma once
#include "stc_common.h"

namespace {

using Raw = __attribute__((ext_vector_type(4))) float;      // 16 bytes as they lie in memory
using u32x4 = __attribute__((ext_vector_type(4))) unsigned;
using bf16x2 = __attribute__((ext_vector_type(2))) __bf16;

// ---- bf16 pairs in a 32-bit word: element 2 i in the low half
__device__ __forceinline__ float lo_f(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float hi_f(unsigned u) { return __uint_as_float(u & 0xffff0000u); }
__device__ __forceinline__ unsigned pk_bf16(float a, float b) {     // v_cvt_pk_bf16_f32 (RNE): a in the low half
    const bf16x2 v = {(__bf16)a, (__bf16)b};
    return __builtin_bit_cast(unsigned, v);
}
__device__ __forceinline__ void unpack8(const u32x4 v, float (&r)[8]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) { r[2 * i] = lo_f(v[i]); r[2 * i + 1] = hi_f(v[i]); }
}
__device__ __forceinline__ void unpack8(const Raw v, float (&r)[8]) { unpack8(__builtin_bit_cast(u32x4, v), r); }
__device__ __forceinline__ u32x4 pack8(const float (&r)[8]) {
    return u32x4{pk_bf16(r[0], r[1]), pk_bf16(r[2], r[3]), pk_bf16(r[4], r[5]), pk_bf16(r[6], r[7])};
}
__device__ __forceinline__ Raw pack8_raw(const float (&r)[8]) { return __builtin_bit_cast(Raw, pack8(r)); }

// ---- the fp32 sums of one piece
template <bool BF16>
struct Piece;

template <>
struct Piece<false> {                                     // four floats (kept as ONE vector value: element arrays cost the patch kernel 16 registers and more)
    Raw v;
    __device__ __forceinline__ void zero() { v = Raw{0.f, 0.f, 0.f, 0.f}; }
    __device__ __forceinline__ void fma(float s, const Raw x) {
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = fmaf(s, x[c], v[c]);
    }
};

template <>
struct Piece<true> {                                      // eight bf16 columns, summed in fp32
    float v[8];
    __device__ __forceinline__ void zero() {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = 0.f;
    }
    __device__ __forceinline__ void fma(float s, const Raw x) {
        const u32x4 u = __builtin_bit_cast(u32x4, x);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v[2 * i] = fmaf(s, lo_f(u[i]), v[2 * i]);
            v[2 * i + 1] = fmaf(s, hi_f(u[i]), v[2 * i + 1]);
        }
    }
};

}  // namespace
