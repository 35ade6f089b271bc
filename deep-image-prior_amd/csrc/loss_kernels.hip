// Loss head and device-side iteration state.
//
//  * dip_loss_head_fwd / dip_loss_head_bwd: the tail of the closure fused into two launches --
//    output conv (1x1, <= 4 channels) + nn.Sigmoid (models/skip.py:96-98 of the reference) +
//    optional mask multiply + torch.nn.MSELoss (denoising.ipynb:177,219; inpainting.ipynb:310:
//    mse(out * mask, img * mask), mean over ALL elements).  HBM-bound: the 128-channel activation
//    is read once (conv on the 4x4x1 MFMA, one lane per pixel); the scalar loss is reduced per lane
//    -> LDS tree -> one partial per block, and the last-arriving block sums the partials in a fixed
//    order (deterministic, no float atomics).
//  * DipIterState + dip_adam_tick / dip_adam_step_dev / dip_noise_axpy_dev: Adam's step count and
//    the Philox offset live in device memory, so one optimisation iteration is a STATIC launch list
//    and can be replayed as a hipGraph (nothing changes on the host between iterations).
#include "dip_common.h"
#include "dip_group.h"
#include <stdlib.h>

namespace {

__device__ __forceinline__ float sigmoidf_(float v) { return 1.f / (1.f + expf(-v)); }

// One lane = one pixel.  The 1x1 conv towards <= 4 channels runs on v_mfma_f32_4x4x1_16b_f32 (16
// independent 4x4 outer products per instruction, A of block 0 broadcast with CBSZ = 4):
//   A[i][k] = w[o = i][c = k]  (lanes 0..3),   B[k][j] = act(u[pixel(lane)][c = k]),   D[i][lane] = y[o = i][pixel]
// so after Cin K steps every lane holds the 4 outputs of its own pixel: no cross-lane reduction for the
// conv, NCHW stores / target / mask loads are coalesced across the lanes, and the only reduction left
// is the scalar loss: per-lane sums -> LDS tree -> one partial per block -> loss_reduce_kernel.
template <bool GRP = false>
__global__ __launch_bounds__(256) void loss_head_fwd_kernel(const DipLossHeadDesc d_, const int ppb, const DipGrpArg<GRP> grp) {
    DIP_GRP_DESC(DipLossHeadDesc, d);
    __shared__ float red[256];
    const int tid = threadIdx.x;
    const int oi = tid & 3;                                    // A row of this lane (only lanes 0..3 of a wave are read)
    const int cin4 = (d.Cin + 3) >> 2;
    const bool has_tr = d.tr.a != nullptr;
    const float slope = d.tr.slope;
    float bias[4];
#pragma unroll
    for (int o = 0; o < 4; ++o) bias[o] = (d.bias != nullptr && o < d.Cout) ? d.bias[o] : 0.f;
    const float* wrow = d.w + (size_t)(oi < d.Cout ? oi : 0) * d.Cin;
    const bool wvalid = oi < d.Cout;

    const int p0 = blockIdx.x * ppb, p1 = min(p0 + ppb, d.HW);
    float lsum = 0.f;
    for (int pb = p0; pb < p1; pb += 256) {
        const int p = pb + tid;
        const bool pv = p < p1;
        const float* up = d.u + (size_t)(pv ? p : p0) * d.Cu;
        f32x4 ac4[4];                                          // independent accumulator chains
#pragma unroll
        for (int e = 0; e < 4; ++e) ac4[e] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
        for (int k4 = 0; k4 < cin4; ++k4) {
            f32x4 b = *reinterpret_cast<const f32x4*>(up + k4 * 4);
            f32x4 a;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int c = k4 * 4 + e;
                a[e] = (wvalid && c < d.Cin) ? wrow[c] : 0.f;
                if (has_tr) {
                    const float ta = c < d.Cin ? d.tr.a[c] : 0.f, tb = c < d.Cin ? d.tr.b[c] : 0.f;   // wave-uniform
                    b[e] = dip_act(fmaf(ta, b[e], tb), slope);
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) ac4[e] = __builtin_amdgcn_mfma_f32_4x4x1f32(a[e], b[e], ac4[e], 4, 0, 0);
        }
        const f32x4 acc = (ac4[0] + ac4[1]) + (ac4[2] + ac4[3]);
        if (pv) {
#pragma unroll
            for (int o = 0; o < 4; ++o) {
                if (o < d.Cout) {
                    float y = acc[o] + bias[o];
                    if (d.sigmoid) y = sigmoidf_(y);
                    d.out[(size_t)o * d.HW + p] = y;
                    const float t = d.target[(size_t)o * d.HW + p];
                    float a = y, b = t;
                    if (d.mask != nullptr) {
                        const float m = d.mask[(size_t)(d.mask_c == 1 ? 0 : o) * d.HW + p];
                        a = y * m;                                 // mse(out * mask, img * mask)
                        b = t * m;
                    }
                    const float df = a - b;
                    lsum = fmaf(df, df, lsum);
                }
            }
        }
    }
    // block tree (fixed order) -> one partial per block; loss_reduce_kernel sums the partials
    red[tid] = lsum;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    if (tid == 0) d.partials[blockIdx.x] = red[0];
}

// Coalesced variant for Cin/4 = NC4 a power of two <= 32 (every net of the notebooks: 128, 16 or 8 channels in front
// of the output conv): NC4 consecutive lanes share a pixel, each owns 4 channels -- a wave reads 64/NC4 whole pixels
// = one contiguous run per load instruction (the lane-per-pixel kernel above strides 4*Cu bytes between lanes and
// ran at 1.8 TB/s) -- computes its 4 x Cout partial products, and an xor-butterfly over the NC4 lanes (fixed order)
// leaves the sums in every lane; lane o of the group finishes output channel o.
template <int NC4, bool GRP = false>
__global__ __launch_bounds__(256) void loss_head_fwd_coal_kernel(const DipLossHeadDesc d_, const int ppb, const DipGrpArg<GRP> grp) {
    DIP_GRP_DESC(DipLossHeadDesc, d);
    __shared__ float red[256];
    constexpr int PW = 64 / NC4;                 // pixels per wave and step
    constexpr int PB = 4 * PW;                   // ... per block and step
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cg = lane % NC4, psub = lane / NC4;
    const bool has_tr = d.tr.a != nullptr;
    const float slope = has_tr ? d.tr.slope : 1.f;
    const bool leaky = slope > 0.f;
    f32x4 ta = f32x4{1.f, 1.f, 1.f, 1.f}, tb = f32x4{0.f, 0.f, 0.f, 0.f};
    float w[4][4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int c = cg * 4 + e;
        if (has_tr && c < d.Cin) { ta[e] = d.tr.a[c]; tb[e] = d.tr.b[c]; }
#pragma unroll
        for (int o = 0; o < 4; ++o) w[o][e] = (o < d.Cout && c < d.Cin) ? d.w[(size_t)o * d.Cin + c] : 0.f;
    }
    // the lane group's sums are formed by a PACKED butterfly: the first two exchanges (distances NC4 / 2, NC4 / 4) also halve
    // the number of values a lane carries (4 -> 2 -> 1: a lane sends the half it will not finish), the others add one value:
    // log2(NC4) + 1 cross-lane moves per pixel step instead of 4 log2(NC4) -- with 32 lanes per pixel 6 instead of 20, which
    // had the LDS crossbar (ds_bpermute), not HBM, pace this kernel (48 us for 134 MB).  Output channel of a lane: 2 bA + bB.
    const bool bA = (cg & (NC4 / 2)) != 0, bB = (cg & (NC4 / 4)) != 0;
    const int myo = 2 * (bA ? 1 : 0) + (bB ? 1 : 0);
    const bool writer = (cg & (NC4 / 4 - 1)) == 0 && myo < d.Cout;
    const float mybias = (d.bias != nullptr && myo < d.Cout) ? d.bias[myo] : 0.f;
    const int p0 = blockIdx.x * ppb, p1 = min(p0 + ppb, d.HW);
    float lsum = 0.f;
    constexpr int UN = 4;                        // independent loads in flight per thread
    for (int base = p0 + wave * PW; base < p1; base += UN * PB) {      // (wave-uniform trip count: the shuffles below)
        const int pb = base + psub;
        f32x4 u[UN];
#pragma unroll
        for (int q = 0; q < UN; ++q) {
            const int p = pb + q * PB;
            u[q] = *reinterpret_cast<const f32x4*>(d.u + (size_t)(p < p1 ? p : p0) * d.Cu + cg * 4);
        }
#pragma unroll
        for (int q = 0; q < UN; ++q) {
            const int p = pb + q * PB;
            f32x4 v = u[q];
            if (leaky) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = dip_act_leaky(fmaf(ta[e], v[e], tb[e]), slope);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = dip_act(fmaf(ta[e], v[e], tb[e]), slope);
            }
            float part[4];
#pragma unroll
            for (int o = 0; o < 4; ++o) part[o] = (w[o][0] * v[0] + w[o][1] * v[1]) + (w[o][2] * v[2] + w[o][3] * v[3]);
            const float k0 = (bA ? part[2] : part[0]) + __shfl_xor(bA ? part[0] : part[2], NC4 / 2);
            const float k1 = (bA ? part[3] : part[1]) + __shfl_xor(bA ? part[1] : part[3], NC4 / 2);
            float mine = (bB ? k1 : k0) + __shfl_xor(bB ? k0 : k1, NC4 / 4);
#pragma unroll
            for (int sft = NC4 / 8; sft >= 1; sft >>= 1) mine += __shfl_xor(mine, sft);
            if (p < p1 && writer) {
                float y = mine + mybias;
                if (d.sigmoid) y = sigmoidf_(y);
                d.out[(size_t)myo * d.HW + p] = y;
                const float t = d.target[(size_t)myo * d.HW + p];
                float a = y, b = t;
                if (d.mask != nullptr) {
                    const float m = d.mask[(size_t)(d.mask_c == 1 ? 0 : myo) * d.HW + p];
                    a = y * m;                                     // mse(out * mask, img * mask)
                    b = t * m;
                }
                const float df = a - b;
                lsum = fmaf(df, df, lsum);
            }
        }
    }
    red[tid] = lsum;
    __syncthreads();
    for (int s2 = 128; s2 >= 1; s2 >>= 1) {
        if (tid < s2) red[tid] += red[tid + s2];
        __syncthreads();
    }
    if (tid == 0) d.partials[blockIdx.x] = red[0];
}

// Fixed-order fp64 sum of the per-block partials -> the scalar loss.  A launch of its own on purpose: a
// "last-arriving block" ticket needs an agent-scope release fence in EVERY block, which on the multi-XCD
// MI355X writes back / invalidates L2 each time (the ticketed version of this head took 110 us instead
// of ~35: DESIGN.md, dead ends).
template <bool GRP = false>
__global__ __launch_bounds__(256) void loss_reduce_kernel(const float* __restrict__ partials_, int n, double scale,
                                                          float* __restrict__ loss_, const DipGrpArg<GRP> grp) {
    DIP_GRP_PTR(const float*, partials);
    DIP_GRP_PTR(float*, loss);
    __shared__ double dred[256];
    const int tid = threadIdx.x;
    double s = 0.0;
    for (int i = tid; i < n; i += 256) s += (double)partials[i];
    dred[tid] = s;
    __syncthreads();
    for (int st = 128; st >= 1; st >>= 1) {
        if (tid < st) dred[tid] += dred[tid + st];
        __syncthreads();
    }
    if (tid == 0) *loss = (float)(dred[0] * scale);
}

// dy[p][o] = gscale * 2/N * (out*m - t*m) * m * out*(1-out)       (NHWC, channel stride Cy; pad channels zero)
template <bool GRP = false>
__global__ __launch_bounds__(256) void loss_head_bwd_kernel(const DipLossHeadDesc d_, const float* __restrict__ gscale_,
                                                            float* __restrict__ dy_, const int Cy, const DipGrpArg<GRP> grp) {
    DIP_GRP_DESC(DipLossHeadDesc, d);
    DIP_GRP_PTR(const float*, gscale);
    DIP_GRP_PTR(float*, dy);
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= d.HW) return;
    const float gs = gscale != nullptr ? *gscale : 1.f;
    const float k = 2.f / ((float)d.Cout * (float)d.HW);
    for (int c0 = 0; c0 < Cy; c0 += 4) {
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int o = c0 + e;
            if (o < d.Cout) {
                const float y = d.out[(size_t)o * d.HW + p];
                const float t = d.target[(size_t)o * d.HW + p];
                float a = y, b = t, m = 1.f;
                if (d.mask != nullptr) {
                    m = d.mask[(size_t)(d.mask_c == 1 ? 0 : o) * d.HW + p];
                    a = y * m;
                    b = t * m;
                }
                float g = (a - b) * k * gs;                        // aten mse_loss_backward: 2/N * (x - t) * grad
                if (d.mask != nullptr) g = g * m;                  // MulBackward
                if (d.sigmoid) g = g * ((1.f - y) * y);            // aten sigmoid_backward
                v[e] = g;
            }
        }
        *reinterpret_cast<f32x4*>(dy + (size_t)p * Cy + c0) = v;
    }
}

// ---------------------------------------------------------------- device-side iteration state
// t <- t + 1 and the two step-dependent scalars: what adam_tick_kernel (lr by value) and adam_tick_dev_kernel (lr in device
// memory) both run, so the two cannot drift apart
__device__ __forceinline__ void adam_tick_body(DipIterState* st, double lr, double beta1, double beta2) {
    const unsigned long long step = st->step + 1ull;
    st->step = step;
    // scalar prep as torch/optim/adam.py (_single_tensor_adam), in double
    const double bc1 = 1.0 - pow(beta1, (double)step);
    const double bc2 = 1.0 - pow(beta2, (double)step);
    st->step_size = (float)(lr / bc1);
    st->bc2_sqrt = (float)sqrt(bc2);
}

template <bool GRP = false>
__global__  void adam_tick_kernel(DipIterState* st_, double lr, double beta1, double beta2, const DipGrpArg<GRP> grp) {
    DIP_GRP_PTR(DipIterState*, st);
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    adam_tick_body(st, lr, beta1, beta2);
}

// lr read from device memory: a grouped pointer like st, so every instance of a group steps with the lr of its own slab row,
// and a setter rewrites it in stream order under a captured graph
template <bool GRP = false>
__global__  void adam_tick_dev_kernel(DipIterState* st_, const double* __restrict__ lr_dev_, double beta1, double beta2,
                                      const DipGrpArg<GRP> grp) {
    DIP_GRP_PTR(DipIterState*, st);
    DIP_GRP_PTR(const double*, lr_dev);
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    adam_tick_body(st, *lr_dev, beta1, beta2);
}

template <bool GRP = false>
__global__  void counter_add_kernel(unsigned long long* c_, unsigned long long inc, const DipGrpArg<GRP> grp) {
    DIP_GRP_PTR(unsigned long long*, c);
    if (threadIdx.x == 0 && blockIdx.x == 0) *c += inc;
}

template <bool GRP = false>
__global__  void counter_add_n_kernel(unsigned long long* c_, int n, unsigned long long inc, const DipGrpArg<GRP> grp) {
    DIP_GRP_PTR(unsigned long long*, c);
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i < n) c[i] += inc;
}

}  // namespace

// the coalesced head needs a lane per output channel inside a pixel's lane group
#define NC4_MIN_CHECK(cout, nc4) ((nc4) < 4 || (cout) > (nc4))
static int head_ppb(int HW) {
    int ppb = dip_round_up(dip_cdiv(HW, 1024), 256);      // ~1024 blocks, whole 256-pixel strips
    return ppb < 256 ? 256 : ppb;
}

extern "C" int dip_loss_head_nblk(int HW, int Cin) {
    (void)Cin;
    return dip_cdiv(HW, head_ppb(HW));
}

extern "C" int dip_loss_head_fwd(const DipLossHeadDesc* dp, void* stream) {
    const DipLossHeadDesc& d = *dp;
    if (d.Cout < 1 || d.Cout > 4) DIP_FAIL("loss_head: 1..4 output channels");
    if (d.Cin < 1 || (d.Cu & 3) || dip_round_up(d.Cin, 4) > d.Cu) DIP_FAIL("loss_head: channel stride must be a multiple of 4 covering Cin");
    if (d.mask != nullptr && d.mask_c != 1 && d.mask_c != d.Cout) DIP_FAIL("loss_head: mask must have 1 or Cout channels");
    const int ppb = head_ppb(d.HW);
    const int nblk = dip_cdiv(d.HW, ppb);
    if (nblk != d.nblk) DIP_FAIL("loss_head: nblk must come from dip_loss_head_nblk");
    const int nc4 = (d.Cin + 3) / 4;
    static const bool no_coal = getenv("DIP_LOSS_HEAD_NO_COAL") != nullptr;
    hipStream_t st = (hipStream_t)stream;
    if (no_coal || nc4 > 32 || (nc4 & (nc4 - 1)) != 0 || (NC4_MIN_CHECK(d.Cout, nc4))) {
        dip_launch_pair<DIP_FAM_LOSS>(loss_head_fwd_kernel<false>, loss_head_fwd_kernel<true>, dim3(nblk), dim3(256), 0, st, d, ppb);
    } else {
        switch (nc4) {
            case 32: dip_launch_pair<DIP_FAM_LOSS>(loss_head_fwd_coal_kernel<32>, loss_head_fwd_coal_kernel<32, true>, dim3(nblk), dim3(256), 0, st, d, ppb); break;
            case 16: dip_launch_pair<DIP_FAM_LOSS>(loss_head_fwd_coal_kernel<16>, loss_head_fwd_coal_kernel<16, true>, dim3(nblk), dim3(256), 0, st, d, ppb); break;
            case 8: dip_launch_pair<DIP_FAM_LOSS>(loss_head_fwd_coal_kernel<8>, loss_head_fwd_coal_kernel<8, true>, dim3(nblk), dim3(256), 0, st, d, ppb); break;
            default: dip_launch_pair<DIP_FAM_LOSS>(loss_head_fwd_coal_kernel<4>, loss_head_fwd_coal_kernel<4, true>, dim3(nblk), dim3(256), 0, st, d, ppb); break;
        }
    }
    DIP_CHECK_LAUNCH();
    dip_launch_pair<DIP_FAM_LOSS>(loss_reduce_kernel<false>, loss_reduce_kernel<true>, dim3(1), dim3(256), 0, (hipStream_t)stream,
                                  (const float*)d.partials, nblk, 1.0 / ((double)d.Cout * (double)d.HW), d.loss);
    DIP_CHECK_LAUNCH();
    return 0;
}

extern "C" int dip_loss_head_bwd(const DipLossHeadDesc* dp, const float* gscale, float* dy, int Cy, void* stream) {
    const DipLossHeadDesc& d = *dp;
    if (d.Cout < 1 || d.Cout > 4 || (Cy & 3) || Cy < d.Cout) DIP_FAIL("loss_head_bwd: bad channel counts");
    dip_launch_pair<DIP_FAM_LOSS>(loss_head_bwd_kernel<false>, loss_head_bwd_kernel<true>, dim3(dip_cdiv(d.HW, 256)), dim3(256), 0, (hipStream_t)stream,
                                  d, gscale, dy, Cy);
    DIP_CHECK_LAUNCH();
    return 0;
}

extern "C" int dip_adam_tick(DipIterState* st, double lr, double beta1, double beta2, void* stream) {
    dip_launch_pair<DIP_FAM_LOSS>(adam_tick_kernel<false>, adam_tick_kernel<true>, dim3(1), dim3(1), 0, (hipStream_t)stream, st, lr, beta1, beta2);
    DIP_CHECK_LAUNCH();
    return 0;
}

extern "C" int dip_adam_tick_dev(DipIterState* st, const double* lr_dev, double beta1, double beta2, void* stream) {
    if (st == nullptr) DIP_FAIL("adam_tick_dev: iteration state is NULL");
    if (lr_dev == nullptr) DIP_FAIL("adam_tick_dev: lr pointer is NULL");
    dip_launch_pair<DIP_FAM_LOSS>(adam_tick_dev_kernel<false>, adam_tick_dev_kernel<true>, dim3(1), dim3(1), 0, (hipStream_t)stream, st,
                                  lr_dev, beta1, beta2);
    DIP_CHECK_LAUNCH();
    return 0;
}

extern "C" int dip_counter_add(uint64_t* counter, uint64_t inc, void* stream) {
    dip_launch_pair<DIP_FAM_LOSS>(counter_add_kernel<false>, counter_add_kernel<true>, dim3(1), dim3(1), 0, (hipStream_t)stream,
                                  reinterpret_cast<unsigned long long*>(counter), (unsigned long long)inc);
    DIP_CHECK_LAUNCH();
    return 0;
}

extern "C" int dip_counter_add_n(uint64_t* counters, int n, uint64_t inc, void* stream) {
    if (counters == nullptr || n < 1) DIP_FAIL("counter_add_n: needs n >= 1 counters");
    dip_launch_pair<DIP_FAM_LOSS>(counter_add_n_kernel<false>, counter_add_n_kernel<true>, dim3(dip_cdiv(n, 64)), dim3(64), 0,
                                  (hipStream_t)stream, reinterpret_cast<unsigned long long*>(counters), n, (unsigned long long)inc);
    DIP_CHECK_LAUNCH();
    return 0;
}

// ---------------------------------------------------------------- fused super-resolution tail
// The tail of the super-resolution closure (super-resolution.ipynb:169-186 of the reference: out_LR = downsampler(out_HR);
// mse(out_LR, img_LR)) in two launches.  The arithmetic of every element is that of the kernels it replaces
// (lanczos_fwd_kernel / lanczos_bwd_kernel / head_bwd_kernel, misc_kernels.hip): same fmaf chains in the same order, so y and
// dy are bit-identical to the unfused chain; what differs is how the operands reach the lanes.
namespace {

constexpr int SR_T = 16;                       // one block = one channel's 16 x 16 tile of LR outputs
constexpr int SR_LDS_BYTES = 48 * 1024;        // budget of the staged source window
constexpr int SR_UN = 8;                       // independent global loads per lane while the window is staged

// Forward.  Neighbouring outputs read source windows shifted by f, so the block stages the (15 f + k) columns x ((rp - 1) f + k)
// rows its outputs read in LDS: row by row, coalesced, clamped once (ReplicationPad2d).  The window is stored PHASE-SPLIT --
// column x = q f + p lives at p * qn + q -- so the 16 lanes of an output row, which read columns f apart, hit consecutive
// banks; `pitch` is padded on the host so that the second output row of a 32-lane half lands 16 banks further (ds_read_b32
// banks modulo 32 per half wave): conflict-free for f = 2, 4, 8.  Taps are wave-uniform: scalar loads (no global store happens
// before the last of them).  rp < 16 (a window beyond the LDS budget: k = 32, 33 at f = 8) walks the tile in bands of rp rows.
// K, F: compile-time k, f (0: read from the descriptor).
template <int K, int F, bool GRP = false>
__global__ __launch_bounds__(256) void sr_loss_fwd_kernel(const DipSRLossDesc d_, const int qn, const int pitch, const int rp,
                                                          const DipGrpArg<GRP> grp) {
    DIP_GRP_DESC(DipSRLossDesc, d);
    extern __shared__ float sr_win[];
    __shared__ float red[256];
    const int k = K ? K : d.k, f = F ? F : d.f;
    const int tid = threadIdx.x, lx = tid & 15, ly = tid >> 4;
    const int ntx = (d.Wo + SR_T - 1) / SR_T, nty = (d.Ho + SR_T - 1) / SR_T;
    const int b = blockIdx.x;
    const int ox0 = (b % ntx) * SR_T, oy0 = ((b / ntx) % nty) * SR_T, c = b / (ntx * nty);
    const float* xc = d.out + (size_t)c * d.H * d.W;
    const int wc = (SR_T - 1) * f + k, wr = (rp - 1) * f + k, nwin = wr * wc;
    const int ox = ox0 + lx, oy = oy0 + ly;
    const bool inside = ox < d.Wo && oy < d.Ho;
    const int gx0 = ox0 * f - d.pad;
    float acc = 0.f;
    for (int ob = 0; ob < SR_T && oy0 + ob < d.Ho; ob += rp) {        // (block-uniform trip count)
        const int gy0 = (oy0 + ob) * f - d.pad;
        if (ob) __syncthreads();
        for (int i0 = tid; i0 < nwin; i0 += 256 * SR_UN) {             // SR_UN loads in flight per lane, then their LDS writes
            float v[SR_UN];
#pragma unroll
            for (int u = 0; u < SR_UN; ++u) {
                const int idx = i0 + u * 256, wy = idx / wc, wx = idx - wy * wc;
                v[u] = idx < nwin ? xc[(size_t)min(max(gy0 + wy, 0), d.H - 1) * d.W + min(max(gx0 + wx, 0), d.W - 1)] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < SR_UN; ++u) {
                const int idx = i0 + u * 256, wy = idx / wc, wx = idx - wy * wc;
                if (idx < nwin) sr_win[wy * pitch + (wx % f) * qn + wx / f] = v[u];
            }
        }
        __syncthreads();
        if (inside && ly >= ob && ly < ob + rp) {
            const float* base = sr_win + (ly - ob) * f * pitch + lx;
            for (int i = 0; i < k; ++i) {
                const float* row = base + i * pitch;
                const float* tp = d.taps + i * k;
                if constexpr (K > 0) {
#pragma unroll
                    for (int j = 0; j < K; ++j) acc = fmaf(tp[j], row[(j % F) * qn + j / F], acc);
                } else {
                    for (int jq = 0; jq * f < k; ++jq)
                        for (int p = 0; p < f && jq * f + p < k; ++p)               // j = jq f + p ascending
                            acc = fmaf(tp[jq * f + p], row[p * qn + jq], acc);
                }
            }
        }
    }
    float sq = 0.f;
    if (inside) {
        const size_t o = ((size_t)c * d.Ho + oy) * d.Wo + ox;
        const float r = acc - d.target[o];
        d.y[o] = acc;
        sq = r * r;
    }
    red[tid] = sq;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    if (tid == 0) d.partials[b] = red[0];
}

// ---- the TV term of the closure (total_loss = mse(out_LR, img_LR) + tv_weight * tv_loss(out_HR); utils/sr_utils.py:54-59)
constexpr int TV_P = SR_T + 1;                 // a 16 x 16 tile of pixels reads the terms of 17 x 17
constexpr int TV_BW = 64, TV_BH = 16;          // tile of the forward pass: one wave per 64 columns x 4 rows
enum : int { TV_POW = 0, TV_SQRT = 1, TV_ONE = 2, TV_TWO = 3 };      // exact forms of s^beta, as ATen's pow has them

template <bool TV> using SrBwdDesc = std::conditional_t<TV, DipSRTVDesc, DipSRLossDesc>;
__device__ __forceinline__ const DipSRLossDesc& sr_part(const DipSRLossDesc& d) { return d; }
__device__ __forceinline__ const DipSRLossDesc& sr_part(const DipSRTVDesc& d) { return d.sr; }

// s of the term at a pixel: dhd = right - own, dwd = below - own, s = dhd^2 + dwd^2 (one fma; no epsilon: the reference has none)
__device__ __forceinline__ float tv_s(float dhd, float dwd) { return fmaf(dhd, dhd, __fmul_rn(dwd, dwd)); }
__device__ __forceinline__ float tv_pow(float s, float beta, int mode) {
    return mode == TV_SQRT ? sqrtf(s) : mode == TV_ONE ? s : mode == TV_TWO ? __fmul_rn(s, s) : powf(s, beta);
}
// g(s) = beta s^(beta - 1); beta < 1 at s == 0 is +inf, and a = inf * 0 = NaN, as autograd over the spelled closure yields
__device__ __forceinline__ float tv_dpow(float s, float beta, int mode) {
    return mode == TV_SQRT ? 0.5f / sqrtf(s) : mode == TV_ONE ? 1.f : mode == TV_TWO ? __fmul_rn(2.f, s)
                                                                                  : __fmul_rn(beta, powf(s, beta - 1.f));
}
// a = g(s) dhd, b = g(s) dwd of the term at (y, x) of one channel; zero where the term does not exist (outside the image, the
// last row, the last column): nothing outside the image is read
__device__ __forceinline__ void tv_ab(const float* __restrict__ oc, int y, int x, int H, int W, float beta, int mode, float& a,
                                      float& b) {
    a = 0.f;
    b = 0.f;
    if (y < 0 || x < 0 || y >= H - 1 || x >= W - 1) return;
    const float o = oc[y * W + x];
    const float dhd = oc[y * W + x + 1] - o, dwd = oc[(y + 1) * W + x] - o;
    const float g = tv_dpow(tv_s(dhd, dwd), beta, mode);
    a = __fmul_rn(g, dhd);
    b = __fmul_rn(g, dwd);
}

// Forward of the TV term: a pure stream over out.  A block is one channel's 16 rows x 64 columns; a wave walks 4 rows of its 64
// columns keeping the row below in registers (the row it loads for `dwd` is the next step's own row), so an element comes from
// HBM once (the right neighbour is the same cache line; the row under a wave's strip is read twice, by neighbouring waves of
// one block).  Per lane a chain of adds in row order, then the 256-wide LDS tree -> one partial per block.
template <bool GRP = false>
__global__ __launch_bounds__(256) void sr_tv_fwd_kernel(const DipSRTVDesc d_, const int mode, const DipGrpArg<GRP> grp) {
    DIP_GRP_DESC(DipSRTVDesc, d);
    __shared__ float red[256];
    const int H = d.sr.H, W = d.sr.W;
    const int tid = threadIdx.x;
    const int ntx = (W + TV_BW - 1) / TV_BW, nty = (H + TV_BH - 1) / TV_BH;
    const int b = blockIdx.x;
    const int x = (b % ntx) * TV_BW + (tid & 63), y0 = ((b / ntx) % nty) * TV_BH + (tid >> 6) * 4, c = b / (ntx * nty);
    const float* oc = d.sr.out + (size_t)c * H * W;
    const float beta = d.beta;
    float lsum = 0.f;
    if (x < W - 1 && y0 < H - 1) {
        float cur = oc[y0 * W + x], right = oc[y0 * W + x + 1];
        for (int r = 0; r < 4 && y0 + r < H - 1; ++r) {
            const float dn = oc[(y0 + r + 1) * W + x], dnr = oc[(y0 + r + 1) * W + x + 1];
            lsum = __fadd_rn(lsum, tv_pow(tv_s(right - cur, dn - cur), beta, mode));
            cur = dn;
            right = dnr;
        }
    }
    red[tid] = lsum;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    if (tid == 0) d.tv_partials[b] = red[0];
}

// *loss = (float)(sum_mse / (C Ho Wo) + (double)*tv_weight * sum_tv): both partial ranges in fixed order in fp64, one launch
template <bool GRP = false>
__global__ __launch_bounds__(256) void sr_tv_reduce_kernel(const DipSRTVDesc d_, const DipGrpArg<GRP> grp) {
    DIP_GRP_DESC(DipSRTVDesc, d);
    __shared__ double dred[2][256];
    const int tid = threadIdx.x;
    double s0 = 0.0, s1 = 0.0;
    for (int i = tid; i < d.sr.nblk; i += 256) s0 += (double)d.sr.partials[i];
    for (int i = tid; i < d.tv_nblk; i += 256) s1 += (double)d.tv_partials[i];
    dred[0][tid] = s0;
    dred[1][tid] = s1;
    __syncthreads();
    for (int st = 128; st >= 1; st >>= 1) {
        if (tid < st) {
            dred[0][tid] += dred[0][tid + st];
            dred[1][tid] += dred[1][tid + st];
        }
        __syncthreads();
    }
    if (tid == 0)
        *d.sr.loss = (float)(dred[0][0] / ((double)d.sr.C * (double)d.sr.Ho * (double)d.sr.Wo) + (double)*d.tv_weight * dred[1][0]);
}

// Backward: one lane per HR pixel, every channel (four per float4 store); a block is a 16 x 16 tile of HR pixels.  g is
// lanczos_bwd_kernel's gather over v = ((y - target) * kk) * gs (at most ceil(k / f)^2 terms off the frame; a frame pixel also
// takes the padded rows / columns that clamp onto it), then head_bwd_kernel's sigmoid factor and NHWC store with zero pad
// channels.  STAGE: the few LR pixels the tile's gathers touch -- rows oyb .. oyb + nr - 1, columns oxb .. oxb + ncol - 1 of every
// channel -- and the taps are formed ONCE per block into LDS (the lanes of a tile read each of them ~ (16 / f + k / f)^2 / 4 times, and
// y, target would be two loads each time); STAGE = false (a filter whose footprint exceeds the LDS budget) forms v where it
// is read.
//
// TV (dip_sr_tv_loss_bwd): the same kernel over a DipSRTVDesc adds the gradient of tv_weight * tv_loss(out) (utils/sr_utils.py:54-59
// through autograd) to g before the sigmoid factor.  With a = g(s) dhd, b = g(s) dwd of the term at a pixel (tv_ab; zero where the
// term does not exist) pixel p takes -(a + b) of its own term, a of the term to its left and b of the term above it:
//   t = ((-(a[p] + b[p])) + a[left]) + b[above];   coef = (2.f * tvw) * gs;   g = acc + coef * t      (every op rounded on its own)
// STAGE forms a and b of the tile and its one-pixel halo to the left and above (TV_P x TV_P per channel) ONCE per block in LDS,
// so every s and every sqrt / pow is formed once and not three times per pixel; STAGE = false forms them where they are read, by
// the same function: the same bits.
template <bool STAGE, int K, int F, bool TV = false, bool GRP = false>
__global__ __launch_bounds__(256) void sr_loss_bwd_kernel(const SrBwdDesc<TV> dd_, const float* __restrict__ gscale_,
                                                          float* __restrict__ dy_, const int Cy, const int tv_mode,
                                                          const DipGrpArg<GRP> grp) {
    DIP_GRP_DESC(SrBwdDesc<TV>, dd);
    const DipSRLossDesc& d = sr_part(dd);
    DIP_GRP_PTR(const float*, gscale);
    DIP_GRP_PTR(float*, dy);
    extern __shared__ float sr_lds[];
    const int HW = d.H * d.W;
    const int tid = threadIdx.x;
    const int tx0 = blockIdx.x * SR_T, ty0 = blockIdx.y * SR_T;
    const int sx = tx0 + (tid & 15), sy = ty0 + (tid >> 4);
    const int k = K ? K : d.k, f = F ? F : d.f, pad = d.pad, Ho = d.Ho, Wo = d.Wo;
    const int ntv = (TV && STAGE) ? d.C * TV_P * TV_P : 0;
    float* const tv_a = sr_lds;                    // [C][TV_P][TV_P], origin (ty0 - 1, tx0 - 1); tv_b behind it
    float* const tv_b = sr_lds + ntv;
    float* const sr_tap = sr_lds + 2 * ntv;        // [k * k]: a lane's taps depend on its pixel's phase, so not scalar loads
    float* const sr_v = sr_tap + k * k;
    float tv_beta = 0.f, tv_coef = 0.f;
    if constexpr (TV) {
        tv_beta = dd.beta;
        tv_coef = __fmul_rn(__fmul_rn(2.f, *dd.tv_weight), gscale != nullptr ? *gscale : 1.f);
        if constexpr (STAGE) {
            for (int idx = tid; idx < ntv; idx += 256) {
                const int c = idx / (TV_P * TV_P), li = idx - c * (TV_P * TV_P), r = li / TV_P, q = li - r * TV_P;
                tv_ab(d.out + (size_t)c * HW, ty0 - 1 + r, tx0 - 1 + q, d.H, d.W, tv_beta, tv_mode, tv_a[idx], tv_b[idx]);
            }
        }
    }
    const size_t HWo = (size_t)Ho * Wo;
    const float gs = gscale != nullptr ? *gscale : 1.f;
    const float kk = 2.f / ((float)d.C * (float)(Ho * Wo));
    int oyb = 0, oxb = 0, nr = 0, ncol = 0;
    if constexpr (STAGE) {
        // padded-domain rows / columns of the whole tile (as ylo .. yhi below, + pad) -> the LR rows / columns they reach
        const int ty1 = min(ty0 + SR_T - 1, d.H - 1), tx1 = min(tx0 + SR_T - 1, d.W - 1);
        const int tmin = ty0 == 0 ? 0 : ty0 + pad, tmax = ty1 == d.H - 1 ? d.H - 1 + 2 * pad : ty1 + pad;
        const int umin = tx0 == 0 ? 0 : tx0 + pad, umax = tx1 == d.W - 1 ? d.W - 1 + 2 * pad : tx1 + pad;
        oyb = max((tmin - k + 1 + f - 1) / f, 0);
        oxb = max((umin - k + 1 + f - 1) / f, 0);
        nr = max(min(tmax / f, Ho - 1) - oyb + 1, 0);
        ncol = max(min(umax / f, Wo - 1) - oxb + 1, 0);
        const int per = nr * ncol, n = d.C * per;
        for (int idx = tid; idx < k * k; idx += 256) sr_tap[idx] = d.taps[idx];
        for (int idx = tid; idx < n; idx += 256) {
            const int c = idx / per, rem = idx - c * per, r = rem / ncol, q = rem - r * ncol;
            const size_t o = (size_t)c * HWo + (size_t)(oyb + r) * Wo + (oxb + q);
            sr_v[idx] = ((d.y[o] - d.target[o]) * kk) * gs;
        }
        __syncthreads();
    }
    if (sx >= d.W || sy >= d.H) return;
    const int p = sy * d.W + sx;
    const int ylo = (sy == 0) ? -pad : sy, yhi = (sy == d.H - 1) ? d.H - 1 + pad : sy;
    const int xlo = (sx == 0) ? -pad : sx, xhi = (sx == d.W - 1) ? d.W - 1 + pad : sx;
    for (int c0 = 0; c0 < Cy; c0 += 4) {
        const int nc = min(d.C - c0, 4);
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        if (nc > 0) {
            const float* yc = d.y + (size_t)c0 * HWo;
            const float* tc = d.target + (size_t)c0 * HWo;
            const int per = nr * ncol;
            for (int py = ylo; py <= yhi; ++py) {
                const int t = py + pad;
                const int oy_hi = min(t / f, Ho - 1);
                const int oy_lo = max((t - k + 1 + f - 1) / f, 0);
                for (int oy = oy_lo; oy <= oy_hi; ++oy) {
                    const int i = t - oy * f;
                    if (i < 0 || i >= k) continue;
                    for (int px = xlo; px <= xhi; ++px) {
                        const int u = px + pad;
                        const int ox_hi = min(u / f, Wo - 1);
                        const int ox_lo = max((u - k + 1 + f - 1) / f, 0);
                        for (int ox = ox_lo; ox <= ox_hi; ++ox) {
                            const int j = u - ox * f;
                            if (j < 0 || j >= k) continue;
                            const float tap = STAGE ? sr_tap[i * k + j] : d.taps[i * k + j];
#pragma unroll
                            for (int e = 0; e < 4; ++e)
                                if (e < nc) {
                                    float v;
                                    if constexpr (STAGE) {
                                        v = sr_v[(c0 + e) * per + (oy - oyb) * ncol + (ox - oxb)];
                                    } else {
                                        const size_t q = e * HWo + (size_t)oy * Wo + ox;
                                        v = ((yc[q] - tc[q]) * kk) * gs;
                                    }
                                    acc[e] = fmaf(tap, v, acc[e]);
                                }
                        }
                    }
                }
            }
        }
        f32x4 v4;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float g = 0.f;
            if (e < nc) {
                g = acc[e];
                if constexpr (TV) {
                    float a, b, al, bu, unused;
                    if constexpr (STAGE) {
                        const int li = (c0 + e) * (TV_P * TV_P) + (sy - ty0 + 1) * TV_P + (sx - tx0 + 1);
                        a = tv_a[li];
                        b = tv_b[li];
                        al = tv_a[li - 1];
                        bu = tv_b[li - TV_P];
                    } else {
                        const float* oc = d.out + (size_t)(c0 + e) * HW;
                        tv_ab(oc, sy, sx, d.H, d.W, tv_beta, tv_mode, a, b);
                        tv_ab(oc, sy, sx - 1, d.H, d.W, tv_beta, tv_mode, al, unused);
                        tv_ab(oc, sy - 1, sx, d.H, d.W, tv_beta, tv_mode, unused, bu);
                    }
                    const float t = __fadd_rn(__fadd_rn(-__fadd_rn(a, b), al), bu);
                    g = __fadd_rn(g, __fmul_rn(tv_coef, t));
                }
                if (d.sigmoid) {
                    const float o = d.out[(size_t)(c0 + e) * HW + p];
                    g = g * ((1.f - o) * o);     // aten sigmoid_backward: grad * (1 - y) * y
                }
            }
            v4[e] = g;
        }
        *reinterpret_cast<f32x4*>(dy + (size_t)p * Cy + c0) = v4;
    }
}

// everything the two entry points refuse before a launch
const char* sr_loss_refusal(const DipSRLossDesc* dp) {
    if (dp == nullptr) return "sr_loss: NULL descriptor";
    const DipSRLossDesc& d = *dp;
    if (d.out == nullptr || d.taps == nullptr || d.target == nullptr || d.y == nullptr || d.partials == nullptr || d.loss == nullptr)
        return "sr_loss: NULL field";
    if (d.C < 1 || d.k < 1 || d.f < 1) return "sr_loss: C, k, f must be >= 1";
    if (d.H < 1 || d.W < 1 || d.pad < 0 || d.H + 2 * d.pad < d.k || d.W + 2 * d.pad < d.k)
        return "sr_loss: the padded image is smaller than the filter";
    if (d.Ho != (d.H + 2 * d.pad - d.k) / d.f + 1 || d.Wo != (d.W + 2 * d.pad - d.k) / d.f + 1)
        return "sr_loss: Ho / Wo must be (H + 2 pad - k) / f + 1";
    if ((long long)d.C * d.H * d.W > 0x7fffffffLL) return "sr_loss: image too large";
    if (d.nblk != dip_sr_loss_nblk(d.C, d.Ho, d.Wo)) return "sr_loss: nblk must come from dip_sr_loss_nblk";
    return nullptr;
}

}  // namespace

extern "C" int dip_sr_loss_nblk(int C, int Ho, int Wo) {
    if (C < 1 || Ho < 1 || Wo < 1) return 0;
    return C * dip_cdiv(Ho, SR_T) * dip_cdiv(Wo, SR_T);
}

// the down-sampler + MSE partials of both forwards: the same instantiations, so y is the same bits with and without TV
static int sr_fwd_launch(const DipSRLossDesc& d, hipStream_t st) {
    // the phase-split window: qn columns per phase; pitch >= f qn with f * pitch = 16 (mod 32) where one exists (see the kernel)
    const int wc = (SR_T - 1) * d.f + d.k;
    const int qn = dip_cdiv(wc, d.f);
    int pitch = d.f * qn;
    for (int e = 0; e < 32; ++e)
        if ((d.f * (pitch + e)) % 32 == 16) { pitch += e; break; }
    int rp = SR_T;
    while (rp > 1 && (size_t)((rp - 1) * d.f + d.k) * pitch * 4 > (size_t)SR_LDS_BYTES) rp >>= 1;
    const size_t lds = (size_t)((rp - 1) * d.f + d.k) * pitch * 4;
    if (lds > (size_t)SR_LDS_BYTES) DIP_FAIL("sr_loss: the filter's source window does not fit the LDS budget");
    const dim3 grid(d.nblk), blk(256);
    if (d.k == 16 && d.f == 4)
        dip_launch_pair<DIP_FAM_LOSS>(sr_loss_fwd_kernel<16, 4>, sr_loss_fwd_kernel<16, 4, true>, grid, blk, lds, st, d, qn, pitch, rp);
    else
        dip_launch_pair<DIP_FAM_LOSS>(sr_loss_fwd_kernel<0, 0>, sr_loss_fwd_kernel<0, 0, true>, grid, blk, lds, st, d, qn, pitch, rp);
    DIP_CHECK_LAUNCH();
    return 0;
}

extern "C" int dip_sr_loss_fwd(const DipSRLossDesc* dp, void* stream) {
    if (const char* why = sr_loss_refusal(dp)) DIP_FAIL(why);
    const DipSRLossDesc& d = *dp;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = sr_fwd_launch(d, st)) return rc;
    // (through the pair as well: launched bare it would reduce instance 0 only)
    dip_launch_pair<DIP_FAM_LOSS>(loss_reduce_kernel<false>, loss_reduce_kernel<true>, dim3(1), dim3(256), 0, st, (const float*)d.partials,
                                  d.nblk, 1.0 / ((double)d.C * (double)d.Ho * (double)d.Wo), d.loss);
    DIP_CHECK_LAUNCH();
    return 0;
}

// TV: whether a and b of the tile fit the budget beside the staged LR pixels (DipSRLossDesc: tvb = 0)
template <bool TV, class D>
static int sr_bwd_launch(const D& dd, const DipSRLossDesc& d, const float* gscale, float* dy, int Cy, int tv_mode, hipStream_t st) {
    // LR rows (columns) a 16-row tile of HR pixels can reach: its padded-domain span is at most 15 + 2 pad (a tile that
    // touches both edges), and floor(tmax / f) - ceil((tmin - k + 1) / f) + 1 <= (tmax - tmin + k - 1) / f + 1 (+ 1 to spare)
    const long long nl = (SR_T - 1 + 2 * d.pad + d.k - 1) / d.f + 2;
    const long long tvb = TV ? 2LL * d.C * TV_P * TV_P * 4 : 0;
    const long long lds = ((long long)d.C * nl * nl + (long long)d.k * d.k) * 4 + tvb;
    const dim3 grid(dip_cdiv(d.W, SR_T), dip_cdiv(d.H, SR_T));
    const dim3 blk(256);
    if (lds > SR_LDS_BYTES)
        dip_launch_pair<DIP_FAM_LOSS>(sr_loss_bwd_kernel<false, 0, 0, TV>, sr_loss_bwd_kernel<false, 0, 0, TV, true>, grid, blk, 0, st,
                                      dd, gscale, dy, Cy, tv_mode);
    else if (d.k == 16 && d.f == 4)
        dip_launch_pair<DIP_FAM_LOSS>(sr_loss_bwd_kernel<true, 16, 4, TV>, sr_loss_bwd_kernel<true, 16, 4, TV, true>, grid, blk,
                                      (size_t)lds, st, dd, gscale, dy, Cy, tv_mode);
    else
        dip_launch_pair<DIP_FAM_LOSS>(sr_loss_bwd_kernel<true, 0, 0, TV>, sr_loss_bwd_kernel<true, 0, 0, TV, true>, grid, blk,
                                      (size_t)lds, st, dd, gscale, dy, Cy, tv_mode);
    DIP_CHECK_LAUNCH();
    return 0;
}

static const char* sr_bwd_refusal(const DipSRLossDesc& d, const float* dy, int Cy) {
    if (dy == nullptr) return "sr_loss_bwd: NULL dy";
    if (Cy < d.C || (Cy & 3)) return "sr_loss_bwd: Cy must be a multiple of 4 covering C";
    if ((long long)d.H * d.W * Cy > 0x7fffffffLL) return "sr_loss_bwd: image too large";
    return nullptr;
}

extern "C" int dip_sr_loss_bwd(const DipSRLossDesc* dp, const float* gscale, float* dy, int Cy, void* stream) {
    if (const char* why = sr_loss_refusal(dp)) DIP_FAIL(why);
    if (const char* why = sr_bwd_refusal(*dp, dy, Cy)) DIP_FAIL(why);
    return sr_bwd_launch<false>(*dp, *dp, gscale, dy, Cy, 0, (hipStream_t)stream);
}

// ---------------------------------------------------------------- ... with the TV term
extern "C" int dip_sr_tv_nblk(int C, int H, int W) {
    if (C < 1 || H < 1 || W < 1) return 0;
    return C * dip_cdiv(H, TV_BH) * dip_cdiv(W, TV_BW);
}

// everything the two TV entry points refuse before a launch; *mode: the exact form of s^beta
static const char* sr_tv_refusal(const DipSRTVDesc* dp, int* mode) {
    if (dp == nullptr) return "sr_tv_loss: NULL descriptor";
    if (const char* why = sr_loss_refusal(&dp->sr)) return why;
    const DipSRTVDesc& d = *dp;
    if (d.tv_weight == nullptr || d.tv_partials == nullptr) return "sr_tv_loss: NULL tv_weight / tv_partials";
    if (d.tv_nblk != dip_sr_tv_nblk(d.sr.C, d.sr.H, d.sr.W)) return "sr_tv_loss: tv_nblk must come from dip_sr_tv_nblk";
    if (!(d.beta > 0.f) || !(d.beta <= 3.402823466e38f)) return "sr_tv_loss: beta must be finite and > 0";
    *mode = d.beta == 0.5f ? TV_SQRT : d.beta == 1.f ? TV_ONE : d.beta == 2.f ? TV_TWO : TV_POW;
    return nullptr;
}

extern "C" int dip_sr_tv_loss_fwd(const DipSRTVDesc* dp, void* stream) {
    int mode = 0;
    if (const char* why = sr_tv_refusal(dp, &mode)) DIP_FAIL(why);
    const DipSRTVDesc& d = *dp;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = sr_fwd_launch(d.sr, st)) return rc;
    dip_launch_pair<DIP_FAM_LOSS>(sr_tv_fwd_kernel<false>, sr_tv_fwd_kernel<true>, dim3(d.tv_nblk), dim3(256), 0, st, d, mode);
    DIP_CHECK_LAUNCH();
    dip_launch_pair<DIP_FAM_LOSS>(sr_tv_reduce_kernel<false>, sr_tv_reduce_kernel<true>, dim3(1), dim3(256), 0, st, d);
    DIP_CHECK_LAUNCH();
    return 0;
}

extern "C" int dip_sr_tv_loss_bwd(const DipSRTVDesc* dp, const float* gscale, float* dy, int Cy, void* stream) {
    int mode = 0;
    if (const char* why = sr_tv_refusal(dp, &mode)) DIP_FAIL(why);
    if (const char* why = sr_bwd_refusal(dp->sr, dy, Cy)) DIP_FAIL(why);
    return sr_bwd_launch<true>(*dp, dp->sr, gscale, dy, Cy, mode, (hipStream_t)stream);
}
