// Device code the monitor kernels share (monitor_kernels.hip, sr_monitor_kernels.hip, restore_monitor_kernels.hip,
// early_stop_kernels.hip).  Inline helpers only: every kernel compiles to the instruction stream it had with the code written
// out (profiles/monitor_refactor_isa.txt).
#pragma once
#include <cstdint>

// The overflow guard of a device-indexed launch: is the iteration index it = counter[0] in [0, capacity)?  (The host refuses
// first.)  Workgroup-uniform.
__device__ __forceinline__ bool mon_in_range(int it, int capacity) { return it >= 0 && it < capacity; }

// The block's total of one running sum per thread (256 threads), added in a fixed pairing order (deterministic); thread 0
// stores it to *dst.  The LDS array lives here, not in the caller: handed in by reference it is addressed through a generic
// pointer until late in the compilation, and the kernels come out different.  (So do the two- and three-sum kernels of
// restore_monitor_kernels.hip and monitor_kernels.hip from a K-sum form of this helper: they keep their loops.)
template <typename T>
__device__ __forceinline__ void mon_block_sum(T v, T* __restrict__ dst) {
    __shared__ T sh[256];
    sh[threadIdx.x] = v;
    for (int s = 128; s >= 1; s >>= 1) {
        __syncthreads();
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    }
    if (threadIdx.x == 0) dst[0] = sh[0];
}

// compare_psnr with data_range = 1 from a sum of n squared errors
__device__ __forceinline__ float mon_psnr(double s, int64_t n) { return (float)(-10.0 * log10(s / (double)n)); }

// The back-tracking decision of the denoising and restoration closures on state = [psnr_last, restore_flag, have_last,
// snapshot_flag] (the layout dip_arena_backtrack reads): when `check`, fall back to the last checkpoint if psnr dropped by
// more than thresh_db since it was taken, or else take a new one.  Returns the restore flag (the record's fell_back).
__device__ __forceinline__ float mon_backtrack_decision(float* state, bool check, float psnr, float thresh_db) {
    float restore = 0.f, snap = 0.f;
    if (check) {
        if (state[2] != 0.f && psnr - state[0] < -thresh_db) {
            restore = 1.f;                        // "Falling back to previous checkpoint."
        } else {
            snap = 1.f;
            state[0] = psnr;
            state[2] = 1.f;
        }
    }
    state[1] = restore;
    state[3] = snap;
    return restore;
}
