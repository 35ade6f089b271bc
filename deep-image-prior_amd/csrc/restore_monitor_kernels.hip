// Device-side bookkeeping of the restoration / inpainting closure (restoration.ipynb:180-219).
//
// After backward() the reference closure does, every iteration, on the host:
//   psrn_masked = compare_psnr(img_masked, out.detach().cpu().numpy()[0] * img_mask_np)   (:192)  -> D2H + sync
//   psrn        = compare_psnr(img_np,     out.detach().cpu().numpy()[0])                 (:193)  -> D2H + sync
//   if PLOT and i % show_every == 0:                                                      (:198)
//       fall back to the last checkpoint when psrn_masked dropped by > 5 dB               (:202-208)
//       else checkpoint all parameters on the CPU, psrn_masked_last = psrn_masked         (:209-211)
// Here the two squared-error sums stay on the GPU: one streaming pass leaves two fp32 partials per block, a one-block kernel
// turns them into the record {loss, mse_masked, mse, psnr_masked, psnr, fell_back} and takes the back-tracking decision, and
// dip_arena_backtrack (monitor_kernels.hip, unchanged: `state` has FitMonitor's float[4] layout) applies it to the flat
// parameter arena.  img_masked = img * mask, so (out*mask - img*mask) is computed as (out - img) * mask.  No EMA: this closure
// has none.  Nothing synchronises; the host reads the records when it wants the curve.
//
// The notebook starts psrn_masked_last at 0 and keeps no have_last flag; here the first check always snapshots (have_last).
// For images and outputs in [0, 1] every squared error is <= 1, so psrn_masked >= 0 and `psrn_masked - 0 < -5` is never true:
// the two rules take the same decisions.  The iteration index counts closure evaluations, one record row each: a fall-back is
// written into its row and the index moves on (the notebook returns before its `i += 1` and tests again at its next call).
#include "dip_common.h"
#include "dip_group.h"
#include "monitor_common.h"

namespace {

// The phases and their instantiations are those of fit_monitor_*_kernel (monitor_kernels.hip):
// DEV = false (dip_restore_monitor): `check` and the record row come from the host, by value; no counter is read or written.
// DEV = true (dip_restore_monitor_dev): the iteration index i is counter[0], check = backtracking && i % show_every == 0 (the
// restoration notebook checks ON the show_every-th iterations, the denoising one between them), the row is records + 6 * i and
// the finalize kernel's last store is counter[0] = i + 1.  i outside [0, capacity) is the overflow guard: nothing is written to
// records / counter and the decision flags are cleared, so the arena_backtrack launch that follows does nothing.
// GRP (csrc/dip_group.h; DIP_FAM_LOSS): one dispatch for the B monitors of a group; every pointer is shifted to the
// workgroup's instance (blockIdx.z) before the same body runs.  A workgroup belongs to exactly one instance, so the guard
// stays workgroup-uniform and each instance takes its own decision.
//
// mask is [mask_c][hw] with mask_c 1 (one plane for all channels: element i reads mask[i % hw]) or n / hw (element i reads
// mask[i]).  i % hw is carried along the grid-stride walk (one 64-bit remainder per thread, then add-and-wrap).
template <bool DEV, bool GRP = false>
__global__ __launch_bounds__(256) void restore_monitor_partials_kernel(const float* __restrict__ out_,
                                                                       const float* __restrict__ img_,
                                                                       const float* __restrict__ mask_, int mask_c, int64_t n,
                                                                       int64_t hw, const int* __restrict__ counter_,
                                                                       int capacity, float* __restrict__ partial_,
                                                                       const DipGrpArg<GRP> grp) {
    DIP_GRP_PTR(const float*, out);
    DIP_GRP_PTR(const float*, img);
    DIP_GRP_PTR(const float*, mask);
    DIP_GRP_PTR(const int*, counter);
    DIP_GRP_PTR(float*, partial);
    __shared__ float sh[2][256];
    if constexpr (DEV) {
        const int it = counter[0];                // uniform; the finalize launch behind this one advances it
        if (!mon_in_range(it, capacity)) return;
    }
    const bool plane = mask_c == 1;               // uniform
    const int64_t stride = (int64_t)gridDim.x * 256;
    const int64_t pstep = stride % hw;            // uniform
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int64_t p = i % hw;                           // i % hw, kept current below
    float s0 = 0.f, s1 = 0.f;
    for (; i < n; i += stride) {
        const float d = out[i] - img[i];
        const float dm = d * mask[plane ? p : i];
        s0 = fmaf(dm, dm, s0);
        s1 = fmaf(d, d, s1);
        p += pstep;
        if (p >= hw) p -= hw;
    }
    sh[0][threadIdx.x] = s0; sh[1][threadIdx.x] = s1;
    for (int s = 128; s >= 1; s >>= 1) {          // (not mon_block_sum: a two-sum form of it compiles to other code)
        __syncthreads();
        if ((int)threadIdx.x < s) {
            sh[0][threadIdx.x] += sh[0][threadIdx.x + s];
            sh[1][threadIdx.x] += sh[1][threadIdx.x + s];
        }
    }
    if (threadIdx.x == 0) {
        partial[blockIdx.x * 2 + 0] = sh[0][0];
        partial[blockIdx.x * 2 + 1] = sh[1][0];
    }
}

// record: [loss, mse_masked, mse, psnr_masked, psnr, fell_back]
// state:  [psnr_masked_last, restore_flag, have_last, snapshot_flag]        (the layout dip_arena_backtrack reads)
// DEV = false: `record` is the row and `check` the host's decision; DEV = true: `record` is row 0 of the table and `check`
// says whether the monitor back-tracks at all.
template <bool DEV, bool GRP = false>
__global__ __launch_bounds__(64) void restore_monitor_finalize_kernel(const float* __restrict__ partial_, int nblk, int64_t n,
                                                                      const float* __restrict__ loss_,
                                                                      float* __restrict__ record_, float* __restrict__ state_,
                                                                      int check, float thresh_db, int* __restrict__ counter_,
                                                                      int capacity, int show_every, const DipGrpArg<GRP> grp) {
    DIP_GRP_PTR(const float* __restrict__, partial);
    DIP_GRP_PTR(const float* __restrict__, loss);
    DIP_GRP_PTR(float* __restrict__, record);
    DIP_GRP_PTR(float* __restrict__, state);
    DIP_GRP_PTR(int* __restrict__, counter);
    if (threadIdx.x != 0) return;
    int it = 0;
    if constexpr (DEV) {
        it = counter[0];
        if (!mon_in_range(it, capacity)) {        // guard: the host refuses first
            state[1] = 0.f;
            state[3] = 0.f;
            return;
        }
        record += 6 * (int64_t)it;
        check = check && (it % show_every == 0);  // restoration.ipynb:198 `i % show_every == 0`
    }
    double s[2] = {0.0, 0.0};
    for (int b = 0; b < nblk; ++b)
        for (int k = 0; k < 2; ++k) s[k] += (double)partial[b * 2 + k];
    float mse[2], psnr[2];
    for (int k = 0; k < 2; ++k) {
        mse[k] = (float)(s[k] / (double)n);                      // compare_psnr over the whole array (:192-193)
        psnr[k] = mon_psnr(s[k], n);
    }
    record[0] = loss != nullptr ? loss[0] : 0.f;
    record[1] = mse[0]; record[2] = mse[1];
    record[3] = psnr[0]; record[4] = psnr[1];
    record[5] = mon_backtrack_decision(state, check, psnr[0], thresh_db);       // restoration.ipynb:202-211
    if constexpr (DEV) counter[0] = it + 1;
}

template <bool DEV>
int restore_monitor_launch(const float* out, const float* img, const float* mask, int mask_c, int64_t n, int64_t hw,
                           const float* loss, float* partial, float* record, float* state, int check, float backtrack_db,
                           int* counter, int capacity, int show_every, hipStream_t st) {
    const int nblk = dip_fit_monitor_nblk(n);
    dip_launch_pair<DIP_FAM_LOSS>(restore_monitor_partials_kernel<DEV>, restore_monitor_partials_kernel<DEV, true>, dim3(nblk),
                                  dim3(256), 0, st, out, img, mask, mask_c, n, hw, (const int*)counter, capacity, partial);
    DIP_CHECK_LAUNCH();
    dip_launch_pair<DIP_FAM_LOSS>(restore_monitor_finalize_kernel<DEV>, restore_monitor_finalize_kernel<DEV, true>, dim3(1),
                                  dim3(64), 0, st, (const float*)partial, nblk, n, loss, record, state, check, backtrack_db,
                                  counter, capacity, show_every);
    DIP_CHECK_LAUNCH();
    return 0;
}

// mask_c is 1 or the number of planes n / hw
inline bool restore_mask_ok(int mask_c, int64_t n, int64_t hw) {
    return n > 0 && hw > 0 && n % hw == 0 && (mask_c == 1 || (int64_t)mask_c == n / hw);
}

}  // namespace

extern "C" int dip_restore_monitor(const float* out, const float* img, const float* mask, int mask_c, int64_t n, int64_t hw,
                                   const float* loss, float* partial, float* record, float* state, int check_backtrack,
                                   float backtrack_db, void* stream) {
    if (out == nullptr || img == nullptr || mask == nullptr || partial == nullptr || record == nullptr || state == nullptr)
        DIP_FAIL("restore_monitor: a required pointer is NULL");
    if (n <= 0 || hw <= 0) DIP_FAIL("restore_monitor: n and hw must be > 0");
    if (!restore_mask_ok(mask_c, n, hw)) DIP_FAIL("restore_monitor: n must be a multiple of hw and mask_c 1 or n / hw");
    return restore_monitor_launch<false>(out, img, mask, mask_c, n, hw, loss, partial, record, state,
                                         check_backtrack != 0 ? 1 : 0, backtrack_db, nullptr, 0, 0,
                                         reinterpret_cast<hipStream_t>(stream));
}

extern "C" int dip_restore_monitor_dev(const DipRestoreMonitorDesc* d, void* stream) {
    if (d == nullptr) DIP_FAIL("restore_monitor_dev: NULL descriptor");
    if (d->out == nullptr || d->img == nullptr || d->mask == nullptr || d->partial == nullptr || d->records == nullptr ||
        d->counter == nullptr || d->state == nullptr)
        DIP_FAIL("restore_monitor_dev: a required pointer is NULL");
    if (d->n <= 0 || d->hw <= 0 || d->capacity <= 0 || d->show_every <= 0)
        DIP_FAIL("restore_monitor_dev: n, hw, capacity and show_every must be > 0");
    if (!restore_mask_ok(d->mask_c, d->n, d->hw))
        DIP_FAIL("restore_monitor_dev: n must be a multiple of hw and mask_c 1 or n / hw");
    return restore_monitor_launch<true>(d->out, d->img, d->mask, d->mask_c, d->n, d->hw, d->loss, d->partial, d->records,
                                        d->state, d->backtracking != 0 ? 1 : 0, d->backtrack_db, d->counter, d->capacity,
                                        d->show_every, reinterpret_cast<hipStream_t>(stream));
}
