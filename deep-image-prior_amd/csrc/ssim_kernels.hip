// Mean structural similarity (SSIM; Wang, Bovik, Sheikh, Simoncelli 2004) of the net output against a ground truth, on the
// device.  The reference computes none: who wants the number next to the PSNRs copies `out` to the host every iteration and
// filters there (skimage.metrics.structural_similarity), which is the copy and the synchronisation per iteration the other
// monitors (monitor_kernels.hip, sr_monitor_kernels.hip, restore_monitor_kernels.hip) removed, and cannot be part of a launch
// list or a hipGraph.  include/dip_hip.h states the definition and the arithmetic (dip_ssim_dev).
//
// Unlike every other record this is no point-wise stream over `out`: S needs five Gaussian-filtered moment maps.  One
// workgroup (256 threads) owns one channel's tile of SSIM_TH x SSIM_TW = 16 x 64 VALID outputs:
//   * it stages the (16 + 10) x (64 + 10) windows of x - p and y - p (p the pivot) in LDS once -- 2 x 26 x 74 floats, 15392
//     bytes; consecutive threads load consecutive columns of a row, positions outside the image are 0 and reach no valid output;
//   * thread t owns column t % 64 of the row strip t / 64 (4 output rows, 14 window rows).  It walks its 14 window rows top
//     down; per row the horizontal 11-tap fma chain (tap order) gives the five row moments h[5] from 22 LDS reads -- a wave
//     reads 64 consecutive floats per instruction: no bank conflict -- and h enters the vertical chains of the up to four
//     outputs it belongs to, which therefore also accumulate in tap order.  The vertical pass never leaves the registers
//     (20 accumulators); there is no LDS image of the row moments and one barrier in all.  The price is that a strip's 14
//     rows are filtered for 4 outputs where a 26-row LDS image would serve 16: 2.2x the horizontal fmas, for a third of the LDS;
//   * S from individually rounded factors, the optional store to `map`, the thread's four S added in row order, then the
//     256-wide LDS tree of mon_block_sum: one fp32 partial per block, invalid lanes contribute 0.
// A one-block kernel adds the partials in fp64 in a fixed order, divides by C (H-10) (W-10), writes the record row and advances
// the counter.  No float atomics, no last-block ticket: two runs give the same bits.
#include "dip_common.h"
#include "dip_group.h"
#include "monitor_common.h"

namespace {

constexpr int SSIM_WIN = 11, SSIM_HALO = SSIM_WIN - 1;
constexpr int SSIM_TH = 16, SSIM_TW = 64;                 // valid outputs per workgroup
constexpr int SSIM_ROWS = 4;                              // output rows per thread: 256 threads = 4 strips x 64 columns
constexpr int SSIM_LH = SSIM_TH + SSIM_HALO, SSIM_LW = SSIM_TW + SSIM_HALO;
static_assert(SSIM_TW * (SSIM_TH / SSIM_ROWS) == 256, "one thread per column of a row strip");
static_assert(2 * SSIM_LH * SSIM_LW * sizeof(float) + 256 * sizeof(float) <= 48 * 1024, "LDS budget");

// The grid is (tiles across, tiles down x nsrc, C): source 0 is `out`, source 1 (avg != NULL) the smoothed output; block
// (bx, by, c) of source s leaves its sum in partial[s * nblk + (c * tiles_y + by) * tiles_x + bx].  `map` is of `out` only.
// counter == NULL: the functional form, no guard.  GRP (csrc/dip_group.h; DIP_FAM_LOSS): one dispatch for the B monitors of a
// group; every pointer is shifted to the workgroup's instance before the same body runs, the guard stays workgroup-uniform.
template <bool GRP = false>
__global__ __launch_bounds__(256) void ssim_map_kernel(const float* __restrict__ out_, const float* __restrict__ avg_,
                                                       const float* __restrict__ gt_, float* __restrict__ map_,
                                                       float* __restrict__ partial_, const int* __restrict__ counter_,
                                                       int capacity, int C, int H, int W, int tiles_y, float c1, float c2,
                                                       float pivot, const DipGrpArg<GRP> grp) {
    // The four factors of S round operation by operation (with out == gt numerator and denominator are then the same bits).
    // The pragma is lexical, and __fmul_rn / __fadd_rn are plain * and + in a header, outside its reach: the operators
    // themselves are written here; the filter chains ask for their fma by name.
#pragma clang fp contract(off)
    DIP_GRP_PTR(const float*, out);
    DIP_GRP_PTR(const float*, avg);
    DIP_GRP_PTR(const float*, gt);
    DIP_GRP_PTR(float*, map);
    DIP_GRP_PTR(float*, partial);
    DIP_GRP_PTR(const int*, counter);
    if (counter != nullptr && !mon_in_range(counter[0], capacity)) return;        // uniform; the finalize launch advances it
    // g[k] = exp(-(k - 5)^2 / (2 * 1.5^2)), normalised to sum 1 in fp64, rounded to fp32 (tests/ssim_ref.py: taps32); the
    // loops below are unrolled, so every tap is an immediate
    constexpr float g[SSIM_WIN] = {0.00102838012f, 0.00759875821f, 0.0360007733f, 0.109360687f, 0.213005543f, 0.266011715f,
                                   0.213005543f, 0.109360687f, 0.0360007733f, 0.00759875821f, 0.00102838012f};
    __shared__ float sx[SSIM_LH][SSIM_LW], sy[SSIM_LH][SSIM_LW];
    const int c = (int)dip_grp_z<GRP>(grp);
    const int src = (int)blockIdx.y / tiles_y, ty = (int)blockIdx.y % tiles_y;     // workgroup-uniform
    const int y0 = ty * SSIM_TH, x0 = (int)blockIdx.x * SSIM_TW;
    const int Hv = H - SSIM_HALO, Wv = W - SSIM_HALO;
    const float* __restrict__ xs = (src == 0 ? out : avg) + (int64_t)c * H * W;
    const float* __restrict__ ys = gt + (int64_t)c * H * W;
    for (int i = threadIdx.x; i < SSIM_LH * SSIM_LW; i += 256) {
        const int r = i / SSIM_LW, q = i % SSIM_LW;
        const bool in = y0 + r < H && x0 + q < W;
        const int64_t at = (int64_t)(y0 + r) * W + (x0 + q);
        sx[r][q] = in ? xs[at] - pivot : 0.f;
        sy[r][q] = in ? ys[at] - pivot : 0.f;
    }
    __syncthreads();
    const int col = threadIdx.x % SSIM_TW, strip = threadIdx.x / SSIM_TW;
    float acc[SSIM_ROWS][5];
#pragma unroll
    for (int j = 0; j < SSIM_ROWS; ++j)
#pragma unroll
        for (int m = 0; m < 5; ++m) acc[j][m] = 0.f;
#pragma unroll
    for (int r = 0; r < SSIM_ROWS + SSIM_HALO; ++r) {
        const int row = strip * SSIM_ROWS + r;
        float h[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < SSIM_WIN; ++k) {
            const float a = sx[row][col + k], b = sy[row][col + k];
            h[0] = fmaf(g[k], a, h[0]);
            h[1] = fmaf(g[k], b, h[1]);
            h[2] = fmaf(g[k], a * a, h[2]);
            h[3] = fmaf(g[k], b * b, h[3]);
            h[4] = fmaf(g[k], a * b, h[4]);
        }
#pragma unroll
        for (int j = 0; j < SSIM_ROWS; ++j)
            if (r - j >= 0 && r - j < SSIM_WIN) {                                 // (resolved when unrolled)
#pragma unroll
                for (int m = 0; m < 5; ++m) acc[j][m] = fmaf(g[r - j], h[m], acc[j][m]);
            }
    }
    const int ox = x0 + col;
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < SSIM_ROWS; ++j) {
        const int oy = y0 + strip * SSIM_ROWS + j;
        if (oy < Hv && ox < Wv) {
            const float ma = acc[j][0], mb = acc[j][1];                           // the means about the pivot
            const float sxx = acc[j][2] - ma * ma, syy = acc[j][3] - mb * mb, sxy = acc[j][4] - ma * mb;
            const float mx = ma + pivot, my = mb + pivot;
            const float n1 = 2.f * (mx * my) + c1, n2 = 2.f * sxy + c2;
            const float d1 = (mx * mx + my * my) + c1, d2 = (sxx + syy) + c2;
            const float S = __fdiv_rn(n1 * n2, d1 * d2);
            if (src == 0 && map != nullptr) map[((int64_t)c * Hv + oy) * Wv + ox] = S;
            s = s + S;
        }
    }
    const int tiles_x = (int)gridDim.x, nblk = C * tiles_y * tiles_x;
    mon_block_sum(s, partial + (int64_t)src * nblk + ((int64_t)c * tiles_y + ty) * tiles_x + blockIdx.x);
}

// record: [ssim, ssim_sm].  Lane t adds the partials t, t + 64, ... of each source in double, thread 0 the 64 lane sums in
// lane order: a fixed order.  counter == NULL: `records` is the row and nothing advances; otherwise the row is records +
// 2 * counter[0], the last store is counter[0] + 1, and an index outside [0, capacity) writes nothing at all.
template <bool GRP = false>
__global__ __launch_bounds__(64) void ssim_finalize_kernel(const float* __restrict__ partial_, int nblk, int nsrc, double count,
                                                           float* __restrict__ records_, int* __restrict__ counter_,
                                                           int capacity, const DipGrpArg<GRP> grp) {
    DIP_GRP_PTR(const float* __restrict__, partial);
    DIP_GRP_PTR(float* __restrict__, records);
    DIP_GRP_PTR(int* __restrict__, counter);
    __shared__ double sh[2][64];
    int it = 0;
    if (counter != nullptr) {
        it = counter[0];
        if (!mon_in_range(it, capacity)) return;  // guard: the host refuses first (SSIMMonitor / NativeIteration / GroupedFits)
    }
    float* __restrict__ record = records + 2 * (int64_t)it;
    double a = 0.0, b = 0.0;
    for (int i = threadIdx.x; i < nblk; i += 64) a += (double)partial[i];
    if (nsrc > 1)
        for (int i = threadIdx.x; i < nblk; i += 64) b += (double)partial[nblk + i];
    sh[0][threadIdx.x] = a;
    sh[1][threadIdx.x] = b;
    __syncthreads();
    if (threadIdx.x != 0) return;
    a = 0.0; b = 0.0;
    for (int t = 0; t < 64; ++t) {
        a += sh[0][t];
        b += sh[1][t];
    }
    record[0] = (float)(a / count);
    record[1] = nsrc > 1 ? (float)(b / count) : 0.f;
    if (counter != nullptr) counter[0] = it + 1;
}

inline int ssim_tiles(int n, int t) { return (n - SSIM_HALO + t - 1) / t; }

}  // namespace

extern "C" int dip_ssim_nblk(int C, int H, int W) {
    if (C < 1 || H < SSIM_WIN || W < SSIM_WIN) return -1;
    const int64_t n = (int64_t)C * ssim_tiles(H, SSIM_TH) * ssim_tiles(W, SSIM_TW);
    return n > 0x7fffffff ? -1 : (int)n;
}

extern "C" int dip_ssim_dev(const DipSsimDesc* d, void* stream) {
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (d == nullptr) DIP_FAIL("ssim_dev: NULL descriptor");
    if (d->out == nullptr || d->gt == nullptr || d->partial == nullptr || d->records == nullptr)
        DIP_FAIL("ssim_dev: a required pointer is NULL (out, gt, partial, records)");
    if (d->C < 1 || d->H < SSIM_WIN || d->W < SSIM_WIN) DIP_FAIL("ssim_dev: C >= 1 and H, W >= 11 are required");
    if (d->counter != nullptr && d->capacity <= 0) DIP_FAIL("ssim_dev: capacity must be > 0");
    const int nsrc = d->avg != nullptr ? 2 : 1;
    const int tx = ssim_tiles(d->W, SSIM_TW), ty = ssim_tiles(d->H, SSIM_TH);
    if ((int64_t)ty * nsrc > 65535 || d->C > 65535 || (int64_t)d->C * dip_group_ctx()->ninst > 65535)
        DIP_FAIL("ssim_dev: the image is too large for one grid (tiles down x sources, channels x instances <= 65535)");
    const int nblk = dip_ssim_nblk(d->C, d->H, d->W);
    if (nblk < 1 || d->nblk != nblk) DIP_FAIL("ssim_dev: nblk is not dip_ssim_nblk(C, H, W)");
    dip_launch_pair<DIP_FAM_LOSS>(ssim_map_kernel<false>, ssim_map_kernel<true>, dim3(tx, ty * nsrc, d->C), dim3(256), 0, st,
                                  d->out, d->avg, d->gt, d->map, d->partial, (const int*)d->counter, d->capacity, d->C, d->H,
                                  d->W, ty, d->c1, d->c2, d->pivot);
    DIP_CHECK_LAUNCH();
    const double count = (double)d->C * (double)(d->H - SSIM_HALO) * (double)(d->W - SSIM_HALO);
    dip_launch_pair<DIP_FAM_LOSS>(ssim_finalize_kernel<false>, ssim_finalize_kernel<true>, dim3(1), dim3(64), 0, st,
                                  (const float*)d->partial, nblk, nsrc, count, d->records, d->counter, d->capacity);
    DIP_CHECK_LAUNCH();
    return 0;
}
