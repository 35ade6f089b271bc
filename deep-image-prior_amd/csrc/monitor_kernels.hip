// Device-side bookkeeping of the notebooks' closures.
//
// The reference closure (denoising.ipynb:214-248) does, every iteration, on the host:
//   out_avg = out_avg * exp_weight + out * (1 - exp_weight)                  (:214-217)
//   psrn_noisy / psrn_gt / psrn_gt_sm = compare_psnr(...) on .cpu().numpy()  (:223-225)  -> 3 D2H + sync
//   if i % show_every: fall back to the last checkpoint when psrn_noisy dropped by > 5 dB,
//                      else checkpoint all parameters on the CPU               (:238-248) -> 8.9 MB D2H
// Here the same arithmetic stays on the GPU: one streaming pass updates the EMA and the three
// squared-error sums, a one-block kernel turns them into a record {loss, 3 MSEs, 3 PSNRs, fell_back}
// and takes the back-tracking decision, and dip_arena_backtrack applies it to the flat parameter
// arena against a device-resident snapshot.  Nothing synchronises; the host reads the records when
// it wants to print.
#include "dip_common.h"
#include "dip_group.h"
#include "monitor_common.h"

namespace {

// One body per phase, in two instantiations (as adam_kernel<DEV> in misc_kernels.hip).
// DEV = false (dip_fit_monitor): `first`, `check` and the record row come from the host, by value; no counter is read or written.
// DEV = true (dip_fit_monitor_dev): the iteration index i is counter[0], so the launch arguments are the same in every
// iteration (a slot of NativeIteration's command arrays must be iteration-invariant): first = (i == 0), check = backtracking &&
// i % show_every != 0, the row is records + 8 * i, and the finalize kernel's last store is counter[0] = i + 1.  i outside
// [0, capacity) is the overflow guard: nothing is written to records / out_avg / counter and the decision flags are cleared,
// so the arena_backtrack launch that follows does nothing.
// GRP (csrc/dip_group.h; DIP_FAM_LOSS): one dispatch for the B monitors of a group.  The monitor's buffers are per-instance
// data of the slab, so every pointer -- counter, state, partial, records, out_avg, snapshot, params -- is shifted to the
// workgroup's instance (blockIdx.z) before the same body runs.  A workgroup belongs to exactly one instance: the overflow
// guard and arena_backtrack's early return stay workgroup-uniform, and each instance takes its own decision.
// (The partials phase keeps its body in a function of its own: local copies of the pointers in front of the guard's early
// return reshape the solo kernel's control flow; behind a call it stays, instruction for instruction, what it was.)
template <bool DEV>
__device__ __forceinline__ void fit_monitor_partials_body(const float* __restrict__ out, const float* __restrict__ noisy,
                                                          const float* __restrict__ gt, float* __restrict__ avg, int64_t n,
                                                          float w, int first, const int* __restrict__ counter, int capacity,
                                                          float* __restrict__ partial) {
    __shared__ float sh[3][256];
    if constexpr (DEV) {
        const int it = counter[0];                // uniform; the finalize launch behind this one advances it
        if (it < 0 || it >= capacity) return;     // (not mon_in_range: in front of `first` it compiles to other code)
        first = it == 0;
    }
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float o = out[i];
        const float a = first ? o : fmaf(avg[i], w, o * (1.f - w));
        avg[i] = a;
        const float dn = o - noisy[i];
        s0 = fmaf(dn, dn, s0);
        if (gt != nullptr) {
            const float g = gt[i];
            s1 = fmaf(o - g, o - g, s1);
            s2 = fmaf(a - g, a - g, s2);
        }
    }
    sh[0][threadIdx.x] = s0; sh[1][threadIdx.x] = s1; sh[2][threadIdx.x] = s2;
    for (int s = 128; s >= 1; s >>= 1) {          // (not mon_block_sum: a three-sum form of it compiles to other code)
        __syncthreads();
        if ((int)threadIdx.x < s) {
#pragma unroll
            for (int k = 0; k < 3; ++k) sh[k][threadIdx.x] += sh[k][threadIdx.x + s];
        }
    }
    if (threadIdx.x == 0) {
        partial[blockIdx.x * 4 + 0] = sh[0][0];
        partial[blockIdx.x * 4 + 1] = sh[1][0];
        partial[blockIdx.x * 4 + 2] = sh[2][0];
    }
}

template <bool DEV, bool GRP = false>
__global__ __launch_bounds__(256) void fit_monitor_partials_kernel(const float* __restrict__ out_,
                                                                   const float* __restrict__ noisy_,
                                                                   const float* __restrict__ gt_, float* __restrict__ avg_,
                                                                   int64_t n, float w, int first,
                                                                   const int* __restrict__ counter_, int capacity,
                                                                   float* __restrict__ partial_, const DipGrpArg<GRP> grp) {
    DIP_GRP_PTR(const float*, out);
    DIP_GRP_PTR(const float*, noisy);
    DIP_GRP_PTR(const float*, gt);
    DIP_GRP_PTR(float*, avg);
    DIP_GRP_PTR(const int*, counter);
    DIP_GRP_PTR(float*, partial);
    fit_monitor_partials_body<DEV>(out, noisy, gt, avg, n, w, first, counter, capacity, partial);
}

// record: [loss, mse_noisy, mse_gt, mse_gt_sm, psnr_noisy, psnr_gt, psnr_gt_sm, fell_back]
// state:  [psnr_noisy_last, restore_flag, have_last, snapshot_flag]
// DEV = false: `record` is the row and `check` the host's decision; DEV = true: `record` is row 0 of the table and `check`
// says whether the monitor back-tracks at all.
template <bool DEV, bool GRP = false>
__global__ __launch_bounds__(64) void fit_monitor_finalize_kernel(const float* __restrict__ partial_, int nblk, int64_t n,
                                                                  int have_gt, const float* __restrict__ loss_,
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
        record += 8 * (int64_t)it;
        check = check && (it % show_every != 0);
    }
    double s[3] = {0.0, 0.0, 0.0};
    for (int b = 0; b < nblk; ++b)
        for (int k = 0; k < 3; ++k) s[k] += (double)partial[b * 4 + k];
    float mse[3], psnr[3];
    for (int k = 0; k < 3; ++k) {
        mse[k] = (float)(s[k] / (double)n);
        psnr[k] = mon_psnr(s[k], n);
    }
    record[0] = loss != nullptr ? loss[0] : 0.f;
    record[1] = mse[0]; record[2] = have_gt ? mse[1] : 0.f; record[3] = have_gt ? mse[2] : 0.f;
    record[4] = psnr[0]; record[5] = have_gt ? psnr[1] : 0.f; record[6] = have_gt ? psnr[2] : 0.f;
    record[7] = mon_backtrack_decision(state, check, psnr[0], thresh_db);
    if constexpr (DEV) counter[0] = it + 1;
}

template <bool GRP = false>
__global__ __launch_bounds__(256) void arena_backtrack_kernel(float* __restrict__ params_, float* __restrict__ snapshot_,
                                                              int64_t n, const float* __restrict__ state_,
                                                              const DipGrpArg<GRP> grp) {
    DIP_GRP_PTR(float* __restrict__, params);
    DIP_GRP_PTR(float* __restrict__, snapshot);
    DIP_GRP_PTR(const float* __restrict__, state);
    const float restore = state[1], snap = state[3];
    if (restore == 0.f && snap == 0.f) return;
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    if (i + 3 < n) {
        if (restore != 0.f) *reinterpret_cast<f32x4*>(params + i) = *reinterpret_cast<const f32x4*>(snapshot + i);
        else *reinterpret_cast<f32x4*>(snapshot + i) = *reinterpret_cast<const f32x4*>(params + i);
    } else {
        for (int64_t j = i; j < n; ++j) {
            if (restore != 0.f) params[j] = snapshot[j];
            else snapshot[j] = params[j];
        }
    }
}

// ---------------------------------------------------------------- posterior mean / variance of the outputs (Welford)
// Iteration i = counter[0] is a sample iff i >= burn_in and (i - burn_in) % every == 0 (and count < 2^24: k stays exact as a
// float; the host refuses first).  Every block reads counter and count, none writes them: the one-thread kernel behind the
// element pass advances both, ordered by the stream.
#define DIP_POSTERIOR_MAX_SAMPLES (1 << 24)
__device__ __forceinline__ bool posterior_is_sample(int it, int count, int burn_in, int every) {
    return it >= burn_in && (it - burn_in) % every == 0 && count >= 0 && count < DIP_POSTERIOR_MAX_SAMPLES;
}

// REC (dip_posterior_rec_dev): the same pass also leaves the block's fp64 sum of (double(mean') - double(gt))^2 over the
// just-updated mean in partial[blockIdx.x]; mean and m2 come from the very statements of REC = false.
template <bool REC>
__device__ __forceinline__ void posterior_update_body(const float* __restrict__ out, float* __restrict__ mean,
                                                      float* __restrict__ m2, int64_t n, int burn_in, int every,
                                                      const int* __restrict__ counter, const int* __restrict__ count,
                                                      const float* __restrict__ gt, double* __restrict__ partial) {
    // Every operation rounds on its own: without the pragma m2 + d * (x - mean') becomes one FMA.  It is lexical, and
    // __fmul_rn / __fadd_rn are plain * and + in a header, outside its reach: the operators themselves are written here.
#pragma clang fp contract(off)
    const int it = counter[0], cnt = count[0];    // uniform
    if (it < 0 || !posterior_is_sample(it, cnt, burn_in, every)) return;
    const float k = (float)(cnt + 1);
    double s = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float x = out[i], mu = mean[i];
        const float d = x - mu;
        const float mu2 = mu + __fdiv_rn(d, k);
        mean[i] = mu2;
        m2[i] = m2[i] + d * (x - mu2);
        if constexpr (REC) {
            const double e = (double)mu2 - (double)gt[i];
            s = s + e * e;
        }
    }
    if constexpr (REC) mon_block_sum<double>(s, partial + blockIdx.x);
}

template <bool GRP = false>
__global__ __launch_bounds__(256) void posterior_update_kernel(const float* __restrict__ out_, float* __restrict__ mean_,
                                                               float* __restrict__ m2_, int64_t n, int burn_in, int every,
                                                               const int* __restrict__ counter_, const int* __restrict__ count_,
                                                               const DipGrpArg<GRP> grp) {
    DIP_GRP_PTR(const float*, out);
    DIP_GRP_PTR(float*, mean);
    DIP_GRP_PTR(float*, m2);
    DIP_GRP_PTR(const int*, counter);
    DIP_GRP_PTR(const int*, count);
    posterior_update_body<false>(out, mean, m2, n, burn_in, every, counter, count, nullptr, nullptr);
}

template <bool GRP = false>
__global__ __launch_bounds__(256) void posterior_update_rec_kernel(const float* __restrict__ out_, float* __restrict__ mean_,
                                                                   float* __restrict__ m2_, int64_t n, int burn_in, int every,
                                                                   const int* __restrict__ counter_,
                                                                   const int* __restrict__ count_, const float* __restrict__ gt_,
                                                                   double* __restrict__ partial_, const DipGrpArg<GRP> grp) {
    DIP_GRP_PTR(const float*, out);
    DIP_GRP_PTR(float*, mean);
    DIP_GRP_PTR(float*, m2);
    DIP_GRP_PTR(const int*, counter);
    DIP_GRP_PTR(const int*, count);
    DIP_GRP_PTR(const float*, gt);
    DIP_GRP_PTR(double*, partial);
    posterior_update_body<true>(out, mean, m2, n, burn_in, every, counter, count, gt, partial);
}

__device__ __forceinline__ void posterior_advance(int burn_in, int every, int* __restrict__ counter, int* __restrict__ count) {
    const int it = counter[0], cnt = count[0];
    if (it < 0 || it == 0x7fffffff) return;       // (a counter the host did not initialise)
    if (posterior_is_sample(it, cnt, burn_in, every)) count[0] = cnt + 1;
    counter[0] = it + 1;
}

template <bool GRP = false>
__global__ __launch_bounds__(64) void posterior_advance_kernel(int burn_in, int every, int* __restrict__ counter_,
                                                               int* __restrict__ count_, const DipGrpArg<GRP> grp) {
    DIP_GRP_PTR(int*, counter);
    DIP_GRP_PTR(int*, count);
    if (threadIdx.x != 0) return;
    posterior_advance(burn_in, every, counter, count);
}

// The one-thread kernel of dip_posterior_rec_dev: on a sample iteration it adds the nblk fp64 partials in block order and writes
// row `count` of records -- {iteration, mse_mean, psnr_mean} -- before count and counter advance as above.  A row outside
// [0, capacity) is not written (the host refuses first); the sample itself has been taken.
template <bool GRP = false>
__global__ __launch_bounds__(64) void posterior_record_kernel(int burn_in, int every, int* __restrict__ counter_,
                                                              int* __restrict__ count_, const double* __restrict__ partial_,
                                                              int nblk, int64_t n, float* __restrict__ records_, int capacity,
                                                              const DipGrpArg<GRP> grp) {
    DIP_GRP_PTR(int*, counter);
    DIP_GRP_PTR(int*, count);
    DIP_GRP_PTR(const double*, partial);
    DIP_GRP_PTR(float*, records);
    if (threadIdx.x != 0) return;
    const int it = counter[0], cnt = count[0];
    if (it >= 0 && it != 0x7fffffff && posterior_is_sample(it, cnt, burn_in, every) && mon_in_range(cnt, capacity)) {
        double s = 0.0;
        for (int b = 0; b < nblk; ++b) s += partial[b];
        float* row = records + 3 * (int64_t)cnt;
        row[0] = (float)it;
        row[1] = (float)(s / (double)n);
        row[2] = mon_psnr(s, n);
    }
    posterior_advance(burn_in, every, counter, count);
}

// ---------------------------------------------------------------- pooling the chains of a grouped posterior (Gelman-Rubin)
// Row c of `mean` / `m2` lies chains[c] * stride bytes behind row 0.  Per element, L lanes at a time (L = 4: 16-byte accesses),
// in individually rounded fp32 operations, walking the chains in list order (include/dip_hip.h states the arithmetic).
template <int L> struct PoolVec { using T = float; };
template <> struct PoolVec<4> { using T = f32x4; };

template <int L>
__device__ __forceinline__ void pool_elements(const char* __restrict__ mean0, const char* __restrict__ m20, long long stride,
                                              const int* __restrict__ chains, int nchains, int64_t i, float fc, float fck,
                                              float fc1, float f, float* __restrict__ mean, float* __restrict__ var,
                                              float* __restrict__ within, float* __restrict__ rhat, double& rsum, double& rmax,
                                              double& ndeg) {
#pragma clang fp contract(off)
    using V = typename PoolVec<L>::T;
    union U { V v; float f[L]; };
    float s[L], w[L], q[L], mu[L];
#pragma unroll
    for (int j = 0; j < L; ++j) s[j] = w[j] = q[j] = 0.f;
    for (int c = 0; c < nchains; ++c) {
        const long long off = (long long)chains[c] * stride;
        U a, b;
        a.v = *reinterpret_cast<const V*>(mean0 + off + 4 * i);
        b.v = *reinterpret_cast<const V*>(m20 + off + 4 * i);
#pragma unroll
        for (int j = 0; j < L; ++j) {
            s[j] = s[j] + a.f[j];
            w[j] = w[j] + b.f[j];
        }
    }
#pragma unroll
    for (int j = 0; j < L; ++j) mu[j] = __fdiv_rn(s[j], fc);
    for (int c = 0; c < nchains; ++c) {
        U a;
        a.v = *reinterpret_cast<const V*>(mean0 + (long long)chains[c] * stride + 4 * i);
#pragma unroll
        for (int j = 0; j < L; ++j) {
            const float d = a.f[j] - mu[j];
            q[j] = q[j] + d * d;
        }
    }
    U om, ov, ow, orh;
#pragma unroll
    for (int j = 0; j < L; ++j) {
        const float W = __fdiv_rn(w[j], fck);
        const float Bk = __fdiv_rn(q[j], fc1);
        const float Vv = f * W + Bk;
        float R;
        if (W > 0.f) {
            R = sqrtf(__fdiv_rn(Vv, W));          // (correctly rounded; __fsqrt_rn is the native, 1-ulp square root here)
            rsum += (double)R;
            rmax = fmax(rmax, (double)R);
        } else {                                  // degenerate (no within-chain variance, or a NaN): left out of the summary
            R = __builtin_nanf("");
            ndeg += 1.0;
        }
        om.f[j] = mu[j]; ov.f[j] = Vv; ow.f[j] = W; orh.f[j] = R;
    }
    *reinterpret_cast<V*>(mean + i) = om.v;
    *reinterpret_cast<V*>(var + i) = ov.v;
    *reinterpret_cast<V*>(within + i) = ow.v;
    if (rhat != nullptr) *reinterpret_cast<V*>(rhat + i) = orh.v;
}

// VEC: every row and every output is 16-byte aligned -- quads, then the n % 4 elements behind them one by one.
// partial[3 * blockIdx.x + {0, 1, 2}] = the block's {sum of R, max of R, number of degenerate elements} in fp64.
template <bool VEC>
__global__ __launch_bounds__(256) void posterior_pool_kernel(const char* __restrict__ mean0, const char* __restrict__ m20,
                                                             long long stride, const int* __restrict__ chains, int nchains,
                                                             int64_t n, float fc, float fck, float fc1, float f,
                                                             float* __restrict__ mean, float* __restrict__ var,
                                                             float* __restrict__ within, float* __restrict__ rhat,
                                                             double* __restrict__ partial) {
    __shared__ double sh[3][256];
    double rsum = 0.0, rmax = -1.0, ndeg = 0.0;   // (R >= 0: -1 says "no element yet")
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
    if constexpr (VEC) {
        const int64_t nq = n / 4;
        for (int64_t qd = t; qd < nq; qd += step)
            pool_elements<4>(mean0, m20, stride, chains, nchains, 4 * qd, fc, fck, fc1, f, mean, var, within, rhat, rsum, rmax,
                             ndeg);
        for (int64_t i = 4 * nq + t; i < n; i += step)
            pool_elements<1>(mean0, m20, stride, chains, nchains, i, fc, fck, fc1, f, mean, var, within, rhat, rsum, rmax, ndeg);
    } else {
        for (int64_t i = t; i < n; i += step)
            pool_elements<1>(mean0, m20, stride, chains, nchains, i, fc, fck, fc1, f, mean, var, within, rhat, rsum, rmax, ndeg);
    }
    sh[0][threadIdx.x] = rsum; sh[1][threadIdx.x] = rmax; sh[2][threadIdx.x] = ndeg;
    for (int s = 128; s >= 1; s >>= 1) {
        __syncthreads();
        if ((int)threadIdx.x < s) {
            sh[0][threadIdx.x] += sh[0][threadIdx.x + s];
            sh[1][threadIdx.x] = fmax(sh[1][threadIdx.x], sh[1][threadIdx.x + s]);
            sh[2][threadIdx.x] += sh[2][threadIdx.x + s];
        }
    }
    if (threadIdx.x == 0) {
        partial[3 * blockIdx.x + 0] = sh[0][0];
        partial[3 * blockIdx.x + 1] = sh[1][0];
        partial[3 * blockIdx.x + 2] = sh[2][0];
    }
}

// summary = {mean of R over the non-degenerate elements, their max, the number of degenerate ones}; NaN, NaN, n when all are.
__global__ __launch_bounds__(64) void posterior_pool_finalize_kernel(const double* __restrict__ partial, int nblk, int64_t n,
                                                                     double* __restrict__ summary) {
    if (threadIdx.x != 0) return;
    double rsum = 0.0, rmax = -1.0, ndeg = 0.0;
    for (int b = 0; b < nblk; ++b) {
        rsum += partial[3 * b + 0];
        rmax = fmax(rmax, partial[3 * b + 1]);
        ndeg += partial[3 * b + 2];
    }
    const double good = (double)n - ndeg;
    summary[0] = good > 0.0 ? rsum / good : __builtin_nan("");
    summary[1] = good > 0.0 ? rmax : __builtin_nan("");
    summary[2] = ndeg;
}

}  // namespace

extern "C" int dip_posterior_dev(const DipPosteriorDesc* d, void* stream) {
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (d == nullptr) DIP_FAIL("posterior_dev: NULL descriptor");
    if (d->out == nullptr || d->mean == nullptr || d->m2 == nullptr || d->count == nullptr || d->counter == nullptr)
        DIP_FAIL("posterior_dev: a required pointer is NULL");
    if (d->n <= 0 || d->burn_in < 0 || d->every < 1) DIP_FAIL("posterior_dev: n > 0, burn_in >= 0 and every >= 1 are required");
    if (d->n > ((int64_t)1 << 33)) DIP_FAIL("posterior_dev: n must be <= 2^33");
    const int nblk = dip_fit_monitor_nblk(d->n);
    dip_launch_pair<DIP_FAM_LOSS>(posterior_update_kernel<false>, posterior_update_kernel<true>, dim3(nblk), dim3(256), 0, st,
                                  d->out, d->mean, d->m2, d->n, d->burn_in, d->every, (const int*)d->counter,
                                  (const int*)d->count);
    DIP_CHECK_LAUNCH();
    dip_launch_pair<DIP_FAM_LOSS>(posterior_advance_kernel<false>, posterior_advance_kernel<true>, dim3(1), dim3(64), 0, st,
                                  d->burn_in, d->every, d->counter, d->count);
    DIP_CHECK_LAUNCH();
    return 0;
}

extern "C" int dip_posterior_rec_dev(const DipPosteriorRecDesc* d, void* stream) {
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (d == nullptr) DIP_FAIL("posterior_rec_dev: NULL descriptor");
    if (d->out == nullptr || d->mean == nullptr || d->m2 == nullptr || d->count == nullptr || d->counter == nullptr ||
        d->gt == nullptr || d->partial == nullptr || d->records == nullptr)
        DIP_FAIL("posterior_rec_dev: a required pointer is NULL");
    if (d->n <= 0 || d->burn_in < 0 || d->every < 1 || d->capacity < 1)
        DIP_FAIL("posterior_rec_dev: n > 0, burn_in >= 0, every >= 1 and capacity >= 1 are required");
    if (d->n > ((int64_t)1 << 33)) DIP_FAIL("posterior_rec_dev: n must be <= 2^33");
    const int nblk = dip_fit_monitor_nblk(d->n);
    dip_launch_pair<DIP_FAM_LOSS>(posterior_update_rec_kernel<false>, posterior_update_rec_kernel<true>, dim3(nblk), dim3(256), 0,
                                  st, d->out, d->mean, d->m2, d->n, d->burn_in, d->every, (const int*)d->counter,
                                  (const int*)d->count, d->gt, d->partial);
    DIP_CHECK_LAUNCH();
    dip_launch_pair<DIP_FAM_LOSS>(posterior_record_kernel<false>, posterior_record_kernel<true>, dim3(1), dim3(64), 0, st,
                                  d->burn_in, d->every, d->counter, d->count, (const double*)d->partial, nblk, d->n, d->records,
                                  d->capacity);
    DIP_CHECK_LAUNCH();
    return 0;
}

extern "C" int dip_posterior_pool(const float* mean0, const float* m20, long long stride, const int* chains, int nchains, int k,
                                  int64_t n, float* mean, float* var, float* within, float* rhat, double* partial,
                                  double* summary, void* stream) {
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (dip_group_ctx()->ninst > 1) DIP_FAIL("posterior_pool: a group bracket is open (the launch pools rows, it is not one of them)");
    if (mean0 == nullptr || m20 == nullptr || chains == nullptr || mean == nullptr || var == nullptr || within == nullptr ||
        partial == nullptr || summary == nullptr)
        DIP_FAIL("posterior_pool: a required pointer is NULL");
    if (n <= 0 || n > ((int64_t)1 << 33)) DIP_FAIL("posterior_pool: n must be in (0, 2^33]");
    if (k < 2 || k > DIP_POSTERIOR_MAX_SAMPLES) DIP_FAIL("posterior_pool: k (samples per chain) must be in [2, 2^24]");
    if (nchains < 2 || nchains > (1 << 16)) DIP_FAIL("posterior_pool: at least 2 chains (and at most 65536) are pooled");
    uintptr_t bits = reinterpret_cast<uintptr_t>(mean0) | reinterpret_cast<uintptr_t>(m20) | (uintptr_t)stride |
                     reinterpret_cast<uintptr_t>(mean) | reinterpret_cast<uintptr_t>(var) |
                     reinterpret_cast<uintptr_t>(within) | reinterpret_cast<uintptr_t>(rhat);
    if (bits & 3) DIP_FAIL("posterior_pool: rows, stride and outputs must be 4-byte aligned");
    const float fc = (float)nchains, fck = (float)((int64_t)nchains * (k - 1)), fc1 = (float)(nchains - 1);
    const float f = (float)(k - 1) / (float)k;
    const int nblk = dip_fit_monitor_nblk(n);
    const char* a = reinterpret_cast<const char*>(mean0);
    const char* b = reinterpret_cast<const char*>(m20);
    if (bits & 15)
        posterior_pool_kernel<false><<<dim3(nblk), dim3(256), 0, st>>>(a, b, stride, chains, nchains, n, fc, fck, fc1, f, mean, var,
                                                                      within, rhat, partial);
    else
        posterior_pool_kernel<true><<<dim3(nblk), dim3(256), 0, st>>>(a, b, stride, chains, nchains, n, fc, fck, fc1, f, mean, var,
                                                                     within, rhat, partial);
    DIP_CHECK_LAUNCH();
    posterior_pool_finalize_kernel<<<dim3(1), dim3(64), 0, st>>>((const double*)partial, nblk, n, summary);
    DIP_CHECK_LAUNCH();
    return 0;
}

extern "C" int dip_fit_monitor_nblk(int64_t n) {
    int64_t b = (n + 1023) / 1024;
    if (b > 1024) b = 1024;
    if (b < 1) b = 1;
    return (int)b;
}

extern "C" int dip_fit_monitor(const float* out, const float* noisy, const float* gt, float* out_avg, int64_t n,
                               float exp_weight, int first, const float* loss, float* partial, float* record,
                               float* state, int check_backtrack, float backtrack_db, void* stream) {
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (n <= 0 || out == nullptr || noisy == nullptr || out_avg == nullptr) DIP_FAIL("fit_monitor: bad arguments");
    const int nblk = dip_fit_monitor_nblk(n);
    dip_launch_pair<DIP_FAM_LOSS>(fit_monitor_partials_kernel<false>, fit_monitor_partials_kernel<false, true>, dim3(nblk),
                                  dim3(256), 0, st, out, noisy, gt, out_avg, n, exp_weight, first, (const int*)nullptr, 0,
                                  partial);
    DIP_CHECK_LAUNCH();
    dip_launch_pair<DIP_FAM_LOSS>(fit_monitor_finalize_kernel<false>, fit_monitor_finalize_kernel<false, true>, dim3(1),
                                  dim3(64), 0, st, (const float*)partial, nblk, n, gt != nullptr ? 1 : 0, loss, record, state,
                                  check_backtrack, backtrack_db, (int*)nullptr, 0, 0);
    DIP_CHECK_LAUNCH();
    return 0;
}

extern "C" int dip_fit_monitor_dev(const DipFitMonitorDesc* d, void* stream) {
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (d == nullptr) DIP_FAIL("fit_monitor_dev: NULL descriptor");
    if (d->out == nullptr || d->noisy == nullptr || d->out_avg == nullptr || d->partial == nullptr || d->records == nullptr ||
        d->counter == nullptr || d->state == nullptr)
        DIP_FAIL("fit_monitor_dev: a required pointer is NULL");
    if (d->n <= 0 || d->capacity <= 0 || d->show_every <= 0) DIP_FAIL("fit_monitor_dev: n, capacity and show_every must be > 0");
    const int nblk = dip_fit_monitor_nblk(d->n);
    dip_launch_pair<DIP_FAM_LOSS>(fit_monitor_partials_kernel<true>, fit_monitor_partials_kernel<true, true>, dim3(nblk),
                                  dim3(256), 0, st, d->out, d->noisy, d->gt, d->out_avg, d->n, d->exp_weight, 0,
                                  (const int*)d->counter, d->capacity, d->partial);
    DIP_CHECK_LAUNCH();
    dip_launch_pair<DIP_FAM_LOSS>(fit_monitor_finalize_kernel<true>, fit_monitor_finalize_kernel<true, true>, dim3(1),
                                  dim3(64), 0, st, (const float*)d->partial, nblk, d->n, d->gt != nullptr ? 1 : 0, d->loss,
                                  d->records, d->state, d->backtracking != 0 ? 1 : 0, d->backtrack_db, d->counter,
                                  d->capacity, d->show_every);
    DIP_CHECK_LAUNCH();
    return 0;
}

extern "C" int dip_arena_backtrack(float* params, float* snapshot, int64_t n, const float* state, void* stream) {
    if (n <= 0) return 0;
    if ((reinterpret_cast<uintptr_t>(params) | reinterpret_cast<uintptr_t>(snapshot)) & 15)
        DIP_FAIL("arena_backtrack: arenas must be 16-byte aligned");
    const int64_t quads = (n + 3) / 4;
    dip_launch_pair<DIP_FAM_LOSS>(arena_backtrack_kernel<false>, arena_backtrack_kernel<true>,
                                  dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                                  params, snapshot, n, state);
    DIP_CHECK_LAUNCH();
    return 0;
}
