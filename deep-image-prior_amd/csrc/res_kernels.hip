// Residual join of the ResNet backbone (models/resnet.py:13-24 of the reference: `return out + x_` at the end of every
// ResidualSequential) and its adjoint, as streaming NHWC kernels: a lane owns a float4 of four channels, four such groups per
// thread, plain vector loads and stores.  Bandwidth kernels: one read of every input, one write.
//
//   forward   out = act_a(a_a[c] * xa + b_a[c]) + act_b(a_b[c] * xb + b_b[c])
//             side a = the block's input (identity, or for the first block the activation behind the first conv, which has no
//             BatchNorm: ones / zeros coefficients with the activation's slope code), side b = the block's second BatchNorm
//             (no activation), both evaluated here from the raw conv outputs -- neither operand is materialised.
//   backward  gout = (g + src) [* act'(a[c] * y + b[c])]
//             g = gradient wrt the block's output, src = data gradient of the block's first conv where the conv launch left it
//             (DipGradSrc); the optional factor is the activation behind the first conv (the bottom of the chain), so that the
//             launch writes dy of that conv directly.
#include "dip_common.h"
#include "dip_gradsrc.h"
#include "dip_group.h"

namespace {

constexpr int RES_IPT = 4;              // float4 groups per thread
constexpr int RES_IPB = 256 * RES_IPT;  // ... per workgroup

// one side of the forward join for channels [ch, ch + 4): t.a == NULL is the identity
__device__ __forceinline__ f32x4 res_side(f32x4 v, const DipTransform& t, int ch) {
    if (t.a == nullptr) return v;
    const f32x4 a = ld4(t.a + ch), b = ld4(t.b + ch);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = dip_act(fmaf(a[e], v[e], b[e]), t.slope);
    return v;
}

__global__ __launch_bounds__(256) void res_join_fwd_kernel(const float* __restrict__ xa, int Cxa, const DipTransform ta,
                                                           const float* __restrict__ xb, int Cxb, const DipTransform tb,
                                                           float* __restrict__ out, int Co, long long n4, int nc4) {
    const int bid = dip_xcd_remap(blockIdx.x, gridDim.x);
    const long long i0 = (long long)bid * RES_IPB + threadIdx.x;
    f32x4 va[RES_IPT], vb[RES_IPT];
#pragma unroll
    for (int k = 0; k < RES_IPT; ++k) {          // all loads first
        const long long i = i0 + k * 256;
        if (i < n4) {
            const long long p = i / nc4;
            const int ch = (int)(i - p * nc4) * 4;
            va[k] = ld4(xa + (size_t)p * Cxa + ch);
            vb[k] = ld4(xb + (size_t)p * Cxb + ch);
        }
    }
#pragma unroll
    for (int k = 0; k < RES_IPT; ++k) {
        const long long i = i0 + k * 256;
        if (i < n4) {
            const long long p = i / nc4;
            const int ch = (int)(i - p * nc4) * 4;
            st4(out + (size_t)p * Co + ch, res_side(va[k], ta, ch) + res_side(vb[k], tb, ch));
        }
    }
}

__global__ __launch_bounds__(256) void res_join_bwd_kernel(const float* __restrict__ g, int Cg, const DipGradSrc src,
                                                           const float* __restrict__ y, int Cy, const DipTransform ty,
                                                           float* __restrict__ gout, int Cgo, int H, int W, long long n4,
                                                           int nc4) {
    const int bid = dip_xcd_remap(blockIdx.x, gridDim.x);
    const long long i0 = (long long)bid * RES_IPB + threadIdx.x;
#pragma unroll
    for (int k = 0; k < RES_IPT; ++k) {
        const long long i = i0 + k * 256;
        if (i >= n4) continue;
        const long long p = i / nc4;
        const int ch = (int)(i - p * nc4) * 4;
        const int r = (int)(p / W), c = (int)(p - (long long)r * W);
        f32x4 v = grad_src4(src, r, c, H, W, ch);
        if (g != nullptr) v += ld4(g + (size_t)p * Cg + ch);
        if (y != nullptr) {
            f32x4 t = ld4(y + (size_t)p * Cy + ch);
            if (ty.a != nullptr) {
                const f32x4 a = ld4(ty.a + ch), b = ld4(ty.b + ch);
#pragma unroll
                for (int e = 0; e < 4; ++e) t[e] = fmaf(a[e], t[e], b[e]);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] *= dip_act_grad(t[e], ty.slope);
        }
        st4(gout + (size_t)p * Cgo + ch, v);
    }
}

}  // namespace

extern "C" int dip_res_join_fwd(const float* xa, int Cxa, const DipTransform* ta, const float* xb, int Cxb,
                                const DipTransform* tb, float* out, int Co, int npix, int C, void* stream) {
    if (xa == nullptr || xb == nullptr || out == nullptr || ta == nullptr || tb == nullptr) DIP_FAIL("res_join_fwd: NULL argument");
    if (npix < 1 || C < 4 || (C & 3) || (Cxa & 3) || (Cxb & 3) || (Co & 3) || Cxa < C || Cxb < C || Co < C)
        DIP_FAIL("res_join_fwd: C and the channel strides must be multiples of 4, strides >= C");
    if ((ta->a == nullptr) != (ta->b == nullptr) || (tb->a == nullptr) != (tb->b == nullptr))
        DIP_FAIL("res_join_fwd: a transform needs both coefficient rows");
    const int nc4 = C / 4;
    const long long n4 = (long long)npix * nc4;
    dip_launch(res_join_fwd_kernel, dim3((unsigned)((n4 + RES_IPB - 1) / RES_IPB)), dim3(256), 0, (hipStream_t)stream, xa, Cxa, *ta,
               xb, Cxb, *tb, out, Co, n4, nc4);
    DIP_CHECK_LAUNCH();
    return 0;
}

extern "C" int dip_res_join_bwd(const float* g, int Cg, const DipGradSrc* src, const float* y, int Cy, const DipTransform* ty,
                                float* gout, int Cgo, int H, int W, int C, void* stream) {
    if (src == nullptr || src->g == nullptr || gout == nullptr) DIP_FAIL("res_join_bwd: NULL argument");
    if (H < 1 || W < 1 || C < 4 || (C & 3) || (Cgo & 3) || Cgo < C || (src->Cg & 3) || (src->choff & 3) ||
        src->choff < 0 || src->Cg < src->choff + C || src->pad < 0)
        DIP_FAIL("res_join_bwd: C and the channel strides must be multiples of 4, strides >= C");
    if (g != nullptr && ((Cg & 3) || Cg < C)) DIP_FAIL("res_join_bwd: stride of g");
    if (src->tw != nullptr || src->win_h > 0) DIP_FAIL("res_join_bwd: a thin-conv or cropped gradient source is not served");
    DipTransform t = {nullptr, nullptr, 1.0f};
    if (y != nullptr) {
        if (ty == nullptr || (Cy & 3) || Cy < C || (ty->a == nullptr) != (ty->b == nullptr)) DIP_FAIL("res_join_bwd: transform / stride of y");
        t = *ty;
    }
    const int nc4 = C / 4;
    const long long n4 = (long long)H * W * nc4;
    dip_launch(res_join_bwd_kernel, dim3((unsigned)((n4 + RES_IPB - 1) / RES_IPB)), dim3(256), 0, (hipStream_t)stream, g, Cg, *src,
               y, Cy, t, gout, Cgo, H, W, n4, nc4);
    DIP_CHECK_LAUNCH();
    return 0;
}
