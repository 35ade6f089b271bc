// fp32 on the bf16 matrix pipe: the one place that knows how an fp32 value becomes three bf16 planes and in which order the
// partial products are summed (conv_bf3.hip, wgrad_bf3.hip).
#pragma once
#include "dip_common.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// exact three-way split by truncation: a == h + m + l, each with <= 8 significand bits (a bf16 number), returned in the
// HIGH halves of h, m, l
__device__ __forceinline__ void dip_bf3_split(float a, unsigned& h, unsigned& m, unsigned& l) {
    const unsigned uh = __float_as_uint(a) & 0xFFFF0000u;
    const float r1 = a - __uint_as_float(uh);
    const unsigned um = __float_as_uint(r1) & 0xFFFF0000u;
    const float r2 = r1 - __uint_as_float(um);
    h = uh;
    m = um;
    l = __float_as_uint(r2) & 0xFFFF0000u;        // (<= 8 significand bits are left: the mask only drops zeros)
}

// two split values -> one dword of a plane (x0 the first bf16 in memory); four -> the 8 bytes of a 4-channel group
__device__ __forceinline__ unsigned dip_bf3_pack2(unsigned x0, unsigned x1) { return (x0 >> 16) | x1; }
__device__ __forceinline__ u32x2 dip_bf3_pack4(const unsigned (&x)[4]) {
    return u32x2{dip_bf3_pack2(x[0], x[1]), dip_bf3_pack2(x[2], x[3])};
}

// the producer's BatchNorm + activation on four channels: a4 / b4 point at their coefficients.  TR = 1: LeakyReLU(slope),
// TR = 2: the activation codes of dip_act (Swish, ELU, ReLU), TR = 0: nothing
template <int TR>
__device__ __forceinline__ f32x4 dip_bf3_transform(f32x4 v, const float* a4p, const float* b4p, float slope) {
    if constexpr (TR != 0) {
        const f32x4 a4 = *reinterpret_cast<const f32x4*>(a4p), b4 = *reinterpret_cast<const f32x4*>(b4p);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float tv = fmaf(a4[e], v[e], b4[e]);
            v[e] = TR == 1 ? dip_act_leaky(tv, slope) : dip_act(tv, slope);
        }
    }
    return v;
}

// f(pa, pb) (integral constants: plane of A, plane of B) for every partial product of the NT-term form, smallest products
// first.  NT = 9: all cross products (exact); NT = 8: without lo*lo (< 2^-32 of the product: 2^-8 of the rounding error of ONE
// fp32 accumulation step); NT = 6: also without lo*mid, mid*lo (each < 2^-24 of the product)
template <int NT, class F>
__device__ __forceinline__ void dip_bf3_products(F&& f) {
    dip_static_for<0, 5>([&](auto S) {
        constexpr int sm = 4 - decltype(S)::value;
        if constexpr (!((NT == 6 && sm > 2) || (NT == 8 && sm > 3))) {
            dip_static_for<0, 3>([&](auto PA) {
                constexpr int pa = decltype(PA)::value, pb = sm - pa;
                if constexpr (pb >= 0 && pb <= 2) f(PA, std::integral_constant<int, pb>{});
            });
        }
    });
}

// host: (number of products 6 / 8 / 9, transform of the descriptor) -> f(integral constant NT, integral constant TR)
static inline int dip_bf3_tr(const DipTransform& tr) { return tr.a == nullptr ? 0 : (tr.slope > 0.f ? 1 : 2); }
template <class F>
int dip_bf3_dispatch(int nt, int tr, F&& f) {
    auto with_nt = [&](auto NT) {
        if (tr == 0) return f(NT, std::integral_constant<int, 0>{});
        if (tr == 1) return f(NT, std::integral_constant<int, 1>{});
        return f(NT, std::integral_constant<int, 2>{});
    };
    if (nt == 6) return with_nt(std::integral_constant<int, 6>{});
    if (nt == 8) return with_nt(std::integral_constant<int, 8>{});
    return with_nt(std::integral_constant<int, 9>{});
}
