// The element format of a handle's activations and MFMA operands: fp32 (DT_F32), bf16 (DT_BF16) or fp16 (DT_F16),
// decided once, at hrn_create.  This header is the one place that decision is written down: the device-side traits Tr<DT> / mma<DT>
// every pass kernel is templated on, and the host-side with_elem() that turns a handle's dtype into that template argument.
//
// The two 16-bit formats share every layout, LDS image, tile shape and counted wait -- an element is two bytes either way -- and
// differ only in the MFMA opcode and the conversions to and from fp32.  The fp16 forms round to nearest even (v_cvt_pk_f16_f32 /
// v_cvt_f16_f32 under the default MODE; never v_cvt_pkrtz_f16_f32) and overflow to +-inf, as torch's .to(torch.float16) does.
#pragma once
#include "kernels.h"

#include <type_traits>

namespace hrn {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
// Pointers that come out of a descriptor in memory are generic; name the address space, or every access through them is a FLAT
// one, which counts on lgkmcnt as well and forces lgkmcnt(0) drains in front of the MFMAs (measured in conv3x3_lds.inc: every
// wait in the chunk loop was a full drain)
#define GLOBAL_AS __attribute__((address_space(1)))

// the 16-bit MFMA path (bf16 or fp16 elements: same layouts, tiles and kernels) versus the fp32 one
constexpr bool is16(int dt) { return dt != DT_F32; }

template <int DT>
struct Tr;

struct Tr16 {   // what the two 16-bit formats share
    using elem = unsigned short;
    using vec = s16x8;   // 8 elements = 16 B = one MFMA operand
    using out4 = s16x4;  // 4 output channels
    static constexpr int KC = 32, VEC = 8;
};

template <>
struct Tr<DT_BF16> : Tr16 {
    typedef bf16x8 x8;
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
    static __device__ __forceinline__ f32x4 mma(V w, V x, f32x4 acc) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(x8, w), __builtin_bit_cast(x8, x), acc, 0, 0, 0);
    }
};

template <>
struct Tr<DT_F16> : Tr16 {
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
    static __device__ __forceinline__ f32x4 mma(V w, V x, f32x4 acc) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(x8, w), __builtin_bit_cast(x8, x), acc, 0, 0, 0);
    }
};

template <>
struct Tr<DT_F32> {
    using elem = float;
    using vec = f32x4;  // 4 fp32 = 16 B = four 16x16x4 MFMA steps
    using out4 = f32x4;
    static constexpr int KC = 16, VEC = 4;
    static __device__ __forceinline__ float ld(elem e) { return e; }
    static __device__ __forceinline__ elem st(float f) { return f; }
};

// one K chunk (Tr<DT>::KC deep) of a 16 x 16 tile: one 16x16x32 MFMA, or four 16x16x4 ones in k order (the exact fp32 fma chain)
template <int DT>
__device__ __forceinline__ f32x4 mma(typename Tr<DT>::vec w, typename Tr<DT>::vec x, f32x4 acc) {
    if constexpr (is16(DT)) {
        return Tr<DT>::mma(w, x, acc);
    } else {
#pragma unroll
        for (int t = 0; t < 4; ++t) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w[t], x[t], acc, 0, 0, 0);
        return acc;
    }
}

// ---- host side: f(std::integral_constant<int, DT>) with the handle's dtype as a compile-time constant; an unknown dtype is an error
template <int DT>
using elem_c = std::integral_constant<int, DT>;

template <class F>
inline hipError_t with_elem16(int dtype, F &&f) {   // the kernels that exist for the 16-bit formats only
    if (dtype == DT_BF16) return f(elem_c<DT_BF16>{});
    if (dtype == DT_F16) return f(elem_c<DT_F16>{});
    return hipErrorInvalidValue;
}
template <class F>
inline hipError_t with_elem(int dtype, F &&f) {
    return dtype == DT_F32 ? f(elem_c<DT_F32>{}) : with_elem16(dtype, f);
}
// ... and f(format, std::integral_constant<int, NR>) for the generic kernel's cout width nr (16 * nr channels per wave): the 16-bit
// formats have 6 / 4 / 3 / 2, fp32 has 4 / 3 / 2
template <class F>
inline hipError_t with_elem_nr(int dtype, int nr, F &&f) {
    return with_elem(dtype, [&](auto dt) {
        if constexpr (is16(decltype(dt)::value))
            if (nr == 6) return f(dt, std::integral_constant<int, 6>{});
        if (nr == 4) return f(dt, std::integral_constant<int, 4>{});
        if (nr == 3) return f(dt, std::integral_constant<int, 3>{});
        if (nr == 2) return f(dt, std::integral_constant<int, 2>{});
        return hipErrorInvalidValue;
    });
}

}  // namespace hrn
