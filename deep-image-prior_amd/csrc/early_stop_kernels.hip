// Ground-truth-free early stopping on the device: the windowed moving variance of the net output (ES-WMV; Wang et al.,
// "Early Stopping for Deep Image Prior").
//
// The reference's notebooks stop a fit by a hand-picked num_iter and a person looking at the plot every show_every iterations
// (`optimize(OPTIMIZER, p, closure, LR, num_iter)`, utils/common_utils.py:223-230).  The host form of the criterion keeps the last W
// outputs, so every iteration pays
//   out_np = out.detach().cpu().numpy()            -> one device-to-host copy of the output and one synchronisation
//   var_t  = np.var(window)                        -> W * n floats read again on the host
// Here the window is a ring [W][n] in device memory and the variance is maintained incrementally: one streaming pass over the
// output replaces the oldest ring slot, updates the per-element fp64 mean and leaves one fp64 partial of the M2 increment per
// block; a one-block kernel sums the partials in a fixed order, updates the scalar M2, takes the decision (new minimum /
// wait / stop), writes the record row and advances the counter; a conditional copy keeps the output (and, through
// dip_early_stop_keep, the flat parameter arena) of the minimum.  Nothing synchronises; the host polls the 4-byte `stopped`
// word when it wants to know (dip_optim.NativeIteration.run_until).
//
// Arithmetic, per element p with x_new = out[p], x_old = the ring slot it replaces, W = window:
//   warm-up (fill < W), k = fill + 1:   d = x_new - mu;  mu' = mu + d / k;  M2 += d * (x_new - mu')            (Welford)
//   window full:                        d = x_new - x_old;  mu' = mu + d / W;  M2 += d * ((x_new - mu') + (x_old - mu))
// all in fp64; var = M2 / (W n) is rounded to fp32 only for the record, the comparison uses the fp64 value.
//
// The ring is 4 W n bytes (315 MB for W = 100 at 3 x 512 x 512), too much for every row of a group.  The same paper's
// exponential-moving-variance form (ES-EMV) needs no ring: per element only the fp64 mean, and one scalar v --
//   first output:   mu = x, v = 0
//   afterwards:     d = x - mu;  mu' = mu + alpha d;  v' = (1 - alpha) (v + alpha sum(d^2) / n)
// -- one load of out, one load and one store of the mean (20 n bytes against 28 n), the same partial sums, the same decision
// and record from iteration `warmup` on (v ramps up from zero for about 1 / alpha iterations: without a warm-up the second
// iteration is a false minimum).  dip_early_stop_emv_dev; state double[0] holds v, `fill` is 0 before the first output and 1
// afterwards, `head` is unused.
#include "dip_common.h"
#include "dip_group.h"
#include "monitor_common.h"

namespace {

// state (DipEarlyStopDesc.state, 64 bytes): two views of one buffer
//   double[0] M2        double[1] var_min (+inf at the start)        double[2] var of the latest decision (+inf at the start)
//   int32[6] head   int32[7] fill   int32[8] wait   int32[9] best_iter (-1 at the start)   int32[10] stopped   int32[11] improved
enum { ES_HEAD = 6, ES_FILL = 7, ES_WAIT = 8, ES_BEST = 9, ES_STOPPED = 10, ES_IMPROVED = 11 };

// GRP (csrc/dip_group.h; DIP_FAM_LOSS): the pointers are shifted to the workgroup's instance before the same body runs; a
// workgroup belongs to exactly one instance, so the guards stay workgroup-uniform.
template <bool GRP = false>
__global__ __launch_bounds__(256) void early_stop_stream_kernel(const float* __restrict__ out_, float* __restrict__ ring_,
                                                                double* __restrict__ mean_, int64_t n, int window,
                                                                const int* __restrict__ counter_, int capacity,
                                                                const int* __restrict__ state_, double* __restrict__ partial_,
                                                                const DipGrpArg<GRP> grp) {
    DIP_GRP_PTR(const float*, out);
    DIP_GRP_PTR(float*, ring);
    DIP_GRP_PTR(double*, mean);
    DIP_GRP_PTR(const int*, counter);
    DIP_GRP_PTR(const int*, state);
    DIP_GRP_PTR(double*, partial);
    const int it = counter[0];                    // uniform; the finalize launch behind this one advances it
    if (!mon_in_range(it, capacity)) return;
    if (state[ES_STOPPED] != 0) return;           // frozen: ring, mean and M2 stay what they were at the stopping iteration
    const int head = state[ES_HEAD], fill = state[ES_FILL];
    if (head < 0 || head >= window || fill < 0 || fill > window) return;          // (a state the host did not initialise)
    float* __restrict__ slot = ring + (int64_t)head * n;
    const bool warm = fill < window;              // uniform
    const double inv = 1.0 / (double)(warm ? fill + 1 : window);
    double s = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float x = out[i];
        const double xn = (double)x;
        const double mu = fill == 0 ? 0.0 : mean[i];
        double d, mu2, t;
        if (warm) {
            d = xn - mu;
            mu2 = mu + d * inv;
            t = xn - mu2;
        } else {
            const double xo = (double)slot[i];
            d = xn - xo;
            mu2 = mu + d * inv;
            t = (xn - mu2) + (xo - mu);
        }
        s = fma(d, t, s);
        slot[i] = x;
        mean[i] = mu2;
    }
    mon_block_sum(s, partial + blockIdx.x);
}

// One wave sums the per-block partials in a fixed order: lane l sums blocks [l c, (l + 1) c) in block order into sh[l] ...
__device__ __forceinline__ void es_lane_sums(const double* __restrict__ partial, int nblk, double* sh) {
    const int c = (nblk + 63) / 64;
    const int b0 = (int)threadIdx.x * c, b1 = b0 + c < nblk ? b0 + c : nblk;
    double s = 0.0;
    for (int b = b0; b < b1; ++b) s += partial[b];
    sh[threadIdx.x] = s;
}
// ... and lane 0 adds the 64 lane sums in lane order
__device__ __forceinline__ double es_total(const double* sh) {
    double s = 0.0;
    for (int l = 0; l < 64; ++l) s += sh[l];
    return s;
}
// the decision on the fp64 variance of iteration `it` (lane 0)
__device__ __forceinline__ void es_decide(double var, int it, int patience, int* __restrict__ state, double* __restrict__ fs) {
    fs[2] = var;
    if (var < fs[1]) {                            // strict; a NaN variance compares false and `wait` advances
        fs[1] = var;
        state[ES_BEST] = it;
        state[ES_WAIT] = 0;
        state[ES_IMPROVED] = 1;
    } else {
        const int w = state[ES_WAIT] + 1;
        state[ES_WAIT] = w;
        if (w >= patience) state[ES_STOPPED] = 1;
    }
}
// record: [var, var_min, best_iter, wait, stopped]      (once stopped: the stopping iteration's row again)
__device__ __forceinline__ void es_record(float* __restrict__ records, int it, const int* __restrict__ state,
                                          const double* __restrict__ fs, int* __restrict__ counter) {
    float* __restrict__ r = records + 5 * (int64_t)it;
    r[0] = (float)fs[2];
    r[1] = (float)fs[1];
    r[2] = (float)state[ES_BEST];
    r[3] = (float)state[ES_WAIT];
    r[4] = (float)state[ES_STOPPED];
    counter[0] = it + 1;
}

template <bool GRP = false>
__global__ __launch_bounds__(64) void early_stop_finalize_kernel(const double* __restrict__ partial_, int nblk, int64_t n,
                                                                 int window, int patience, float* __restrict__ records_,
                                                                 int* __restrict__ state_, int* __restrict__ counter_,
                                                                 int capacity, const DipGrpArg<GRP> grp) {
    DIP_GRP_PTR(const double* __restrict__, partial);
    DIP_GRP_PTR(float* __restrict__, records);
    DIP_GRP_PTR(int* __restrict__, state);
    DIP_GRP_PTR(int* __restrict__, counter);
    __shared__ double sh[64];
    const int it = counter[0];
    const bool inside = mon_in_range(it, capacity);
    const int head = state[ES_HEAD], fill = state[ES_FILL];
    const bool live = inside && state[ES_STOPPED] == 0 && head >= 0 && head < window && fill >= 0 && fill <= window;
    if (live) es_lane_sums(partial, nblk, sh);    // uniform
    __syncthreads();                              // (every lane has read `state` and `counter` before lane 0 writes them)
    if (threadIdx.x != 0) return;
    double* __restrict__ fs = reinterpret_cast<double*>(state);
    state[ES_IMPROVED] = 0;
    if (!inside) return;                          // guard: the host refuses first (EarlyStopMonitor / NativeIteration)
    if (live) {
        const double m2 = fs[0] + es_total(sh);
        fs[0] = m2;
        const int f2 = fill < window ? fill + 1 : window;
        state[ES_FILL] = f2;
        state[ES_HEAD] = head + 1 == window ? 0 : head + 1;
        if (f2 == window) es_decide(m2 / ((double)window * (double)n), it, patience, state, fs);
    }
    es_record(records, it, state, fs, counter);
}

// ---------------------------------------------------------------- ES-EMV: the ring-free criterion
// One load of out, one load and one store of the fp64 mean per element; the block's partial of sum d^2.
template <bool GRP = false>
__global__ __launch_bounds__(256) void early_stop_emv_stream_kernel(const float* __restrict__ out_, double* __restrict__ mean_,
                                                                    int64_t n, double alpha, const int* __restrict__ counter_,
                                                                    int capacity, const int* __restrict__ state_,
                                                                    double* __restrict__ partial_, const DipGrpArg<GRP> grp) {
    DIP_GRP_PTR(const float*, out);
    DIP_GRP_PTR(double*, mean);
    DIP_GRP_PTR(const int*, counter);
    DIP_GRP_PTR(const int*, state);
    DIP_GRP_PTR(double*, partial);
    const int it = counter[0];                    // uniform; the finalize launch behind this one advances it
    if (!mon_in_range(it, capacity)) return;
    if (state[ES_STOPPED] != 0) return;           // frozen: mean and v stay what they were at the stopping iteration
    const bool first = state[ES_FILL] == 0;       // uniform
    double s = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double xn = (double)out[i];
        if (first) {
            mean[i] = xn;
        } else {
            const double mu = mean[i];
            const double d = xn - mu;
            s = fma(d, d, s);
            mean[i] = mu + alpha * d;
        }
    }
    mon_block_sum(s, partial + blockIdx.x);
}

template <bool GRP = false>
__global__ __launch_bounds__(64) void early_stop_emv_finalize_kernel(const double* __restrict__ partial_, int nblk, int64_t n,
                                                                     double alpha, int warmup, int patience,
                                                                     float* __restrict__ records_, int* __restrict__ state_,
                                                                     int* __restrict__ counter_, int capacity,
                                                                     const DipGrpArg<GRP> grp) {
    DIP_GRP_PTR(const double* __restrict__, partial);
    DIP_GRP_PTR(float* __restrict__, records);
    DIP_GRP_PTR(int* __restrict__, state);
    DIP_GRP_PTR(int* __restrict__, counter);
    __shared__ double sh[64];
    const int it = counter[0];
    const bool inside = mon_in_range(it, capacity);
    const bool live = inside && state[ES_STOPPED] == 0;
    const bool first = state[ES_FILL] == 0;
    if (live) es_lane_sums(partial, nblk, sh);    // uniform
    __syncthreads();                              // (every lane has read `state` and `counter` before lane 0 writes them)
    if (threadIdx.x != 0) return;
    double* __restrict__ fs = reinterpret_cast<double*>(state);
    state[ES_IMPROVED] = 0;
    if (!inside) return;                          // guard: the host refuses first
    if (live) {
        const double v = first ? 0.0 : (1.0 - alpha) * (fs[0] + alpha * es_total(sh) / (double)n);
        fs[0] = v;
        state[ES_FILL] = 1;
        if (it >= warmup) es_decide(v, it, patience, state, fs);
    }
    es_record(records, it, state, fs, counter);
}

// dst <- src when the finalize kernel in front of it recorded a new minimum.  Whole quads where both buffers are 16-byte
// aligned, element by element otherwise and in the tail: n is any positive count and nothing behind dst[n - 1] is written.
template <bool GRP = false>
__global__ __launch_bounds__(256) void early_stop_keep_kernel(const float* __restrict__ src_, float* __restrict__ dst_, int64_t n,
                                                              const int* __restrict__ state_, const DipGrpArg<GRP> grp) {
    DIP_GRP_PTR(const float* __restrict__, src);
    DIP_GRP_PTR(float* __restrict__, dst);
    DIP_GRP_PTR(const int* __restrict__, state);
    if (state[ES_IMPROVED] == 0) return;
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    const bool quads = ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0;
    if (quads && i + 3 < n) {
        *reinterpret_cast<f32x4*>(dst + i) = *reinterpret_cast<const f32x4*>(src + i);
    } else {
        const int64_t e = i + 4 < n ? i + 4 : n;
        for (int64_t j = i; j < e; ++j) dst[j] = src[j];
    }
}

int early_stop_keep_launch(const float* src, float* dst, int64_t n, const int* state, hipStream_t st) {
    const int64_t quads = (n + 3) / 4;
    dip_launch_pair<DIP_FAM_LOSS>(early_stop_keep_kernel<false>, early_stop_keep_kernel<true>,
                                  dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, st, src, dst, n, state);
    DIP_CHECK_LAUNCH();
    return 0;
}

}  // namespace

extern "C" int dip_early_stop_dev(const DipEarlyStopDesc* d, void* stream) {
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (d == nullptr) DIP_FAIL("early_stop_dev: NULL descriptor");
    if (d->out == nullptr || d->ring == nullptr || d->mean == nullptr || d->partial == nullptr || d->records == nullptr ||
        d->state == nullptr || d->counter == nullptr || d->best_out == nullptr)
        DIP_FAIL("early_stop_dev: a required pointer is NULL");
    if (d->n <= 0 || d->window <= 0 || d->patience <= 0 || d->capacity <= 0)
        DIP_FAIL("early_stop_dev: n, window, patience and capacity must be > 0");
    if (d->window < 2) DIP_FAIL("early_stop_dev: window must be >= 2");
    if (d->n > ((int64_t)1 << 33)) DIP_FAIL("early_stop_dev: n must be <= 2^33");
    const int nblk = dip_fit_monitor_nblk(d->n);
    dip_launch_pair<DIP_FAM_LOSS>(early_stop_stream_kernel<false>, early_stop_stream_kernel<true>, dim3(nblk), dim3(256), 0, st,
                                  d->out, d->ring, d->mean, d->n, d->window, (const int*)d->counter, d->capacity,
                                  (const int*)d->state, d->partial);
    DIP_CHECK_LAUNCH();
    dip_launch_pair<DIP_FAM_LOSS>(early_stop_finalize_kernel<false>, early_stop_finalize_kernel<true>, dim3(1), dim3(64), 0, st,
                                  (const double*)d->partial, nblk, d->n, d->window, d->patience, d->records,
                                  reinterpret_cast<int*>(d->state), d->counter, d->capacity);
    DIP_CHECK_LAUNCH();
    return early_stop_keep_launch(d->out, d->best_out, d->n, reinterpret_cast<const int*>(d->state), st);
}

extern "C" int dip_early_stop_emv_dev(const DipEarlyStopEmvDesc* d, void* stream) {
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (d == nullptr) DIP_FAIL("early_stop_emv_dev: NULL descriptor");
    if (d->out == nullptr || d->mean == nullptr || d->partial == nullptr || d->records == nullptr || d->state == nullptr ||
        d->counter == nullptr || d->best_out == nullptr)
        DIP_FAIL("early_stop_emv_dev: a required pointer is NULL");
    if (d->n <= 0 || d->patience <= 0 || d->capacity <= 0 || d->warmup <= 0)
        DIP_FAIL("early_stop_emv_dev: n, patience, capacity and warmup must be > 0");
    if (!(d->alpha > 0.0 && d->alpha < 1.0)) DIP_FAIL("early_stop_emv_dev: alpha must be in (0, 1)");
    if (d->n > ((int64_t)1 << 33)) DIP_FAIL("early_stop_emv_dev: n must be <= 2^33");
    const int nblk = dip_fit_monitor_nblk(d->n);
    dip_launch_pair<DIP_FAM_LOSS>(early_stop_emv_stream_kernel<false>, early_stop_emv_stream_kernel<true>, dim3(nblk), dim3(256), 0,
                                  st, d->out, d->mean, d->n, d->alpha, (const int*)d->counter, d->capacity,
                                  (const int*)d->state, d->partial);
    DIP_CHECK_LAUNCH();
    dip_launch_pair<DIP_FAM_LOSS>(early_stop_emv_finalize_kernel<false>, early_stop_emv_finalize_kernel<true>, dim3(1), dim3(64), 0,
                                  st, (const double*)d->partial, nblk, d->n, d->alpha, d->warmup, d->patience, d->records,
                                  reinterpret_cast<int*>(d->state), d->counter, d->capacity);
    DIP_CHECK_LAUNCH();
    return early_stop_keep_launch(d->out, d->best_out, d->n, reinterpret_cast<const int*>(d->state), st);
}

extern "C" int dip_early_stop_keep(const float* src, float* dst, int64_t n, const void* state, void* stream) {
    if (src == nullptr || dst == nullptr || state == nullptr) DIP_FAIL("early_stop_keep: a required pointer is NULL");
    if (n <= 0 || n > ((int64_t)1 << 33)) DIP_FAIL("early_stop_keep: n must be in (0, 2^33]");
    return early_stop_keep_launch(src, dst, n, reinterpret_cast<const int*>(state), reinterpret_cast<hipStream_t>(stream));
}
