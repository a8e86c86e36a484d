// The two 16-bit element formats of the MFMA path: bf16 (DT_BF16) and fp16 (DT_F16).  They share every layout,
// LDS image, tile shape and counted wait -- an element is two bytes either way -- and differ only in the MFMA opcode and the
// conversions to and from fp32.  The bf16 forms are the expressions the kernels used before fp16 existed, so that the bf16
// instantiations compile to the same code; the fp16 forms round to nearest even (v_cvt_pk_f16_f32 / v_cvt_f16_f32 under the
// default MODE; never v_cvt_pkrtz_f16_f32) and overflow to +-inf, as torch's .to(torch.float16) does.
#pragma once
#include "kernels.h"

namespace hrn {

template <int DT>
struct H16;

template <>
struct H16<DT_BF16> {
    typedef __attribute__((ext_vector_type(8))) __bf16 x8;
    static constexpr unsigned short NEG_INF = 0xff80;
    static __device__ __forceinline__ float ld(unsigned short h) { return __uint_as_float(((unsigned)h) << 16); }
    // the low / high element of a packed dword
    static __device__ __forceinline__ float lo(unsigned r) { return __uint_as_float(r << 16); }
    static __device__ __forceinline__ float hi(unsigned r) { return __uint_as_float(r & 0xffff0000u); }
    static __device__ __forceinline__ unsigned short st(float f) {  // round to nearest even
        unsigned u = __float_as_uint(f);
        u += 0x7fffu + ((u >> 16) & 1u);
        return (unsigned short)(u >> 16);
    }
    // two values -> one packed dword (a in the low half): the compiler's conversion (v_cvt_pk_bf16_f32) ...
    static __device__ __forceinline__ unsigned pk(float a, float b) {
        typedef __attribute__((ext_vector_type(2))) __bf16 x2;
        const x2 v = {(__bf16)a, (__bf16)b};
        return __builtin_bit_cast(unsigned, v);
    }
    // ... and the same instruction from inline asm (kernels that keep the compiler from reordering it)
    static __device__ __forceinline__ unsigned pk_asm(float a, float b) {
        unsigned r;
        asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
        return r;
    }
    template <class V>
    static __device__ __forceinline__ __attribute__((ext_vector_type(4))) float mma(V w, V x, __attribute__((ext_vector_type(4))) float acc) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(x8, w), __builtin_bit_cast(x8, x), acc, 0, 0, 0);
    }
};

template <>
struct H16<DT_F16> {
    typedef __attribute__((ext_vector_type(8))) _Float16 x8;
    static constexpr unsigned short NEG_INF = 0xfc00;
    static __device__ __forceinline__ float ld(unsigned short h) { return (float)__builtin_bit_cast(_Float16, h); }
    // (lo / hi as inline asm, one instruction each like bf16's shift / mask: as compiler-visible conversions they tip hipcc's
    // code-size heuristics into a second copy of part of the 96-cout kernel's loop)
    static __device__ __forceinline__ float lo(unsigned r) {
        float f;
        asm("v_cvt_f32_f16 %0, %1" : "=v"(f) : "v"(r));
        return f;
    }
    static __device__ __forceinline__ float hi(unsigned r) {
        float f;
        asm("v_cvt_f32_f16_sdwa %0, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1" : "=v"(f) : "v"(r));
        return f;
    }
    static __device__ __forceinline__ unsigned short st(float f) { return __builtin_bit_cast(unsigned short, (_Float16)f); }
    static __device__ __forceinline__ unsigned pk_asm(float a, float b) {
        unsigned r;
        asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
        return r;
    }
    static __device__ __forceinline__ unsigned pk(float a, float b) {   // (gfx950 selects v_cvt_pk_f16_f32 for it)
        typedef __attribute__((ext_vector_type(2))) _Float16 x2;
        const x2 v = {(_Float16)a, (_Float16)b};
        return __builtin_bit_cast(unsigned, v);
    }
    template <class V>
    static __device__ __forceinline__ __attribute__((ext_vector_type(4))) float mma(V w, V x, __attribute__((ext_vector_type(4))) float acc) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(x8, w), __builtin_bit_cast(x8, x), acc, 0, 0, 0);
    }
};

}  // namespace hrn
