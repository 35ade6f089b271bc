// Device-side bookkeeping of the super-resolution closure (super-resolution.ipynb:169-191, sr_prior_effect.ipynb cell 6).
//
// After backward() the reference closure does, every iteration, on the host:
//   psnr_LR = compare_psnr(imgs['LR_np'], torch_to_np(out_LR))      -> D2H + sync
//   psnr_HR = compare_psnr(imgs['HR_np'], torch_to_np(out_HR))      -> D2H + sync
//   psnr_history.append([psnr_LR, psnr_HR])
// Here the two squared-error sums stay on the GPU: one streaming pass over both sizes leaves one fp32 partial per block, a
// one-block kernel turns them into the record {loss, mse_LR, mse_HR, psnr_LR, psnr_HR}.  Nothing synchronises; the host reads
// the records when it wants the curve.  No EMA and no back-tracking: this closure has neither (monitor_kernels.hip has both).
#include "dip_common.h"
#include "dip_group.h"
#include "monitor_common.h"

namespace {

// The phases and their instantiations are those of fit_monitor_*_kernel (monitor_kernels.hip):
// DEV = false (dip_sr_monitor): the record row comes from the host, by value; no counter is read or written.
// DEV = true (dip_sr_monitor_dev): the iteration index i is counter[0], the row is records + 5 * i and the finalize kernel's
// last store is counter[0] = i + 1.  i outside [0, capacity) is the overflow guard: nothing is written at all.
// GRP (csrc/dip_group.h; DIP_FAM_LOSS): one dispatch for the B monitors of a group; every pointer is shifted to the
// workgroup's instance (blockIdx.z) before the same body runs, and the guard stays workgroup-uniform.
//
// One grid for both sizes: blocks [0, nblk_hr) walk out_HR against img_HR, blocks [nblk_hr, gridDim.x) walk out_LR against
// img_LR, each range with its own grid stride; block b leaves its sum in partial[b].  Without ground truth nblk_hr is 0.
template <bool DEV, bool GRP = false>
__global__ __launch_bounds__(256) void sr_monitor_partials_kernel(const float* __restrict__ out_hr_,
                                                                  const float* __restrict__ img_hr_, int64_t n_hr, int nblk_hr,
                                                                  const float* __restrict__ out_lr_,
                                                                  const float* __restrict__ img_lr_, int64_t n_lr,
                                                                  const int* __restrict__ counter_, int capacity,
                                                                  float* __restrict__ partial_, const DipGrpArg<GRP> grp) {
    DIP_GRP_PTR(const float*, out_hr);
    DIP_GRP_PTR(const float*, img_hr);
    DIP_GRP_PTR(const float*, out_lr);
    DIP_GRP_PTR(const float*, img_lr);
    DIP_GRP_PTR(const int*, counter);
    DIP_GRP_PTR(float*, partial);
    if constexpr (DEV) {
        const int it = counter[0];                // uniform; the finalize launch behind this one advances it
        if (!mon_in_range(it, capacity)) return;
    }
    const bool hr = (int)blockIdx.x < nblk_hr;    // workgroup-uniform
    const float* __restrict__ a = hr ? out_hr : out_lr;
    const float* __restrict__ b = hr ? img_hr : img_lr;
    const int64_t n = hr ? n_hr : n_lr;
    const int blk = hr ? (int)blockIdx.x : (int)blockIdx.x - nblk_hr;
    const int nblk = hr ? nblk_hr : (int)gridDim.x - nblk_hr;
    float s = 0.f;
    for (int64_t i = (int64_t)blk * 256 + threadIdx.x; i < n; i += (int64_t)nblk * 256) {
        const float d = a[i] - b[i];
        s = fmaf(d, d, s);
    }
    mon_block_sum(s, partial + blockIdx.x);
}

// record: [loss, mse_LR, mse_HR, psnr_LR, psnr_HR]
// Lane t sums the partials t, t + 64, ... of each range in double, thread 0 the 64 lane sums in lane order: a fixed order.
// DEV = false: `record` is the row; DEV = true: `record` is row 0 of the table.
template <bool DEV, bool GRP = false>
__global__ __launch_bounds__(64) void sr_monitor_finalize_kernel(const float* __restrict__ partial_, int nblk_hr, int nblk_lr,
                                                                 int64_t n_hr, int64_t n_lr, const float* __restrict__ loss_,
                                                                 float* __restrict__ record_, int* __restrict__ counter_,
                                                                 int capacity, const DipGrpArg<GRP> grp) {
    DIP_GRP_PTR(const float* __restrict__, partial);
    DIP_GRP_PTR(const float* __restrict__, loss);
    DIP_GRP_PTR(float* __restrict__, record);
    DIP_GRP_PTR(int* __restrict__, counter);
    __shared__ double sh[2][64];
    int it = 0;
    if constexpr (DEV) {
        it = counter[0];
        if (!mon_in_range(it, capacity)) return;  // guard: the host refuses first (SRFitMonitor / NativeIteration / GroupedFits)
        record += 5 * (int64_t)it;
    }
    double h = 0.0, l = 0.0;
    for (int b = threadIdx.x; b < nblk_hr; b += 64) h += (double)partial[b];
    for (int b = threadIdx.x; b < nblk_lr; b += 64) l += (double)partial[nblk_hr + b];
    sh[0][threadIdx.x] = h;
    sh[1][threadIdx.x] = l;
    __syncthreads();
    if (threadIdx.x != 0) return;
    h = 0.0; l = 0.0;
    for (int t = 0; t < 64; ++t) {
        h += sh[0][t];
        l += sh[1][t];
    }
    const bool have_hr = nblk_hr > 0;
    record[0] = loss != nullptr ? loss[0] : 0.f;
    record[1] = (float)(l / (double)n_lr);
    record[2] = have_hr ? (float)(h / (double)n_hr) : 0.f;
    record[3] = mon_psnr(l, n_lr);
    record[4] = have_hr ? mon_psnr(h, n_hr) : 0.f;
    if constexpr (DEV) counter[0] = it + 1;
}

template <bool DEV>
int sr_monitor_launch(const float* out_hr, const float* out_lr, const float* img_hr, const float* img_lr, int64_t n_hr,
                      int64_t n_lr, const float* loss, float* partial, float* record, int* counter, int capacity,
                      hipStream_t st) {
    const int nh = img_hr != nullptr ? dip_fit_monitor_nblk(n_hr) : 0;
    const int nl = dip_fit_monitor_nblk(n_lr);
    dip_launch_pair<DIP_FAM_LOSS>(sr_monitor_partials_kernel<DEV>, sr_monitor_partials_kernel<DEV, true>, dim3(nh + nl),
                                  dim3(256), 0, st, out_hr, img_hr, n_hr, nh, out_lr, img_lr, n_lr, (const int*)counter,
                                  capacity, partial);
    DIP_CHECK_LAUNCH();
    dip_launch_pair<DIP_FAM_LOSS>(sr_monitor_finalize_kernel<DEV>, sr_monitor_finalize_kernel<DEV, true>, dim3(1), dim3(64), 0,
                                  st, (const float*)partial, nh, nl, n_hr, n_lr, loss, record, counter, capacity);
    DIP_CHECK_LAUNCH();
    return 0;
}

}  // namespace

extern "C" int dip_sr_monitor(const float* out_HR, const float* out_LR, const float* img_HR, const float* img_LR,
                              int64_t n_hr, int64_t n_lr, const float* loss, float* partial, float* record, void* stream) {
    if (n_hr <= 0 || n_lr <= 0 || out_HR == nullptr || out_LR == nullptr || img_LR == nullptr || partial == nullptr ||
        record == nullptr)
        DIP_FAIL("sr_monitor: bad arguments");
    return sr_monitor_launch<false>(out_HR, out_LR, img_HR, img_LR, n_hr, n_lr, loss, partial, record, nullptr, 0,
                                    reinterpret_cast<hipStream_t>(stream));
}

extern "C" int dip_sr_monitor_dev(const DipSRMonitorDesc* d, void* stream) {
    if (d == nullptr) DIP_FAIL("sr_monitor_dev: NULL descriptor");
    if (d->out_HR == nullptr || d->out_LR == nullptr || d->img_LR == nullptr || d->partial == nullptr ||
        d->records == nullptr || d->counter == nullptr)
        DIP_FAIL("sr_monitor_dev: a required pointer is NULL");
    if (d->n_hr <= 0 || d->n_lr <= 0 || d->capacity <= 0) DIP_FAIL("sr_monitor_dev: n_hr, n_lr and capacity must be > 0");
    return sr_monitor_launch<true>(d->out_HR, d->out_LR, d->img_HR, d->img_LR, d->n_hr, d->n_lr, d->loss, d->partial,
                                   d->records, d->counter, d->capacity, reinterpret_cast<hipStream_t>(stream));
}
