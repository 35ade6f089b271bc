/*
 * dip_hip.h -- C ABI of libdip_hip.so: the MI355X (gfx950) kernels behind the
 * deep-image-prior optimisation loop (skip-net forward + backward + Adam).
 *
 * The reference (DmitryUlyanov/deep-image-prior) has NO native code and no FFI: its arithmetic
 * is PyTorch `nn` modules.  Each entry point below therefore cites the reference *call site* of
 * the PyTorch op(s) it replaces.  INTEGRATION.md shows the ctypes binding a maintainer adds.
 *
 * Conventions
 *   - every tensor is fp32, device memory, NHWC ("pixel-major": [H][W][Cs]) unless stated;
 *     Cs (channel stride) is a multiple of 4, channels [C, Cs) are zero;
 *   - the library allocates nothing and never synchronises: all buffers are caller-owned
 *     (PyTorch caching allocator), every launch goes to the `stream` argument (a hipStream_t),
 *     so the launch sequence is hipGraph-capturable;
 *   - return value: 0 on success, otherwise a hipError_t (or -1 for an unsupported
 *     configuration); dip_last_error() returns a description of the CALLING THREAD's last failure (thread-local).
 *   - one process per GPU, calls come from the thread that owns the stream; the error slot, the open group
 *     (dip_group_begin) and the native-family mask (dip_group_native) are per thread.
 */
#ifndef DIP_HIP_H
#define DIP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DIP_ABI_VERSION 9

#define DIP_PAD_ZERO 0
#define DIP_PAD_REFLECT 1
#define DIP_PAD_REPLICATE 2   /* nn.ReplicationPad2d: the Downsampler inside conv(), models/downsampler.py:56-61 */

/* DipTransform.slope codes for activations other than LeakyReLU (act_fun='Swish' | 'ELU') */
#define DIP_ACT_SWISH (-1.0f)
#define DIP_ACT_ELU (-2.0f)
#define DIP_ACT_RELU (-3.0f)  /* act_fun given as the module CLASS nn.ReLU (models/common.py:90-91: `return act_fun()`) */

#define DIP_UP_NEAREST 0
#define DIP_UP_BILINEAR 1

int dip_abi_version(void);
/* First 16 hex digits of the sha256 over the sources this binary was built from (csrc/*.hip, csrc/*.h, this header; see
 * __graft_entry__.source_id()); "unknown" for a build outside the recipe.  No reference counterpart: provenance of a
 * measured binary (VERDICT r04 next #9c). */
const char* dip_build_id(void);
const char* dip_last_error(void);
/* PCI address ("0000:d9:00.0", lower case hex) of HIP device `device`, for locating its sysfs directory
 * (/sys/bus/pci/devices/<address>: hwmon power / clock sensors, numa_node).  No reference counterpart: bench.py's
 * `device` / power blocks and its rank -> NUMA-node pinning use it.  buf: >= 13 bytes. */
int dip_device_pci_bus_id(int device, char* buf, int len);


/* ---------------------------------------------------------------- command lists ------------- */
/* The static launch list of one direction of the skip-net issued by ONE call (csrc/dip_list.hip) instead of one foreign
 * call per launch -- the host half of "an iteration is a static launch list".  No reference counterpart: the reference's
 * launches are issued op by op by PyTorch's dispatcher from nn.Module.forward / autograd (utils/common_utils.py:223-230).
 * A command is LAUNCH (fn = dip_list_fn_id("dip_conv_igemm") ..., the call's arguments in `slots`: one 8-byte slot per
 * parameter in declaration order -- ints sign-extended to 64 bits, floats in the low 4 bytes, pointers as addresses --
 * INCLUDING a last slot for the trailing `stream` parameter, which dip_list_run fills with streams[stream]), RECORD
 * (hipEventRecord(events[event], streams[stream])) or WAIT (hipStreamWaitEvent(streams[stream], events[event])).
 * The caller owns slots, streams and events; dip_list_run allocates nothing and never synchronises (hipGraph-capturable).
 * Returns 0, or the rc of the first failing command with its index in *failed_at (dip_last_error() describes it). */
#define DIP_CMD_LAUNCH 0
#define DIP_CMD_RECORD 1
#define DIP_CMD_WAIT 2
typedef struct DipCmd {
    int32_t kind, fn, stream, event;
    uint64_t* slots;
    int32_t nslots, reserved;
} DipCmd;
int dip_list_fn_id(const char* name);          /* -1: not a stream-launching entry point */
int dip_list_fn_nargs(int fn);                 /* parameters of that entry point, the trailing stream included */
int dip_list_run(const DipCmd* cmds, int n, void* const* streams, int nstreams, void* const* events, int nevents,
                 int* failed_at);
/* n HIP events without timing (hipEventDisableTiming) for RECORD / WAIT commands */
int dip_events_create(void** events, int n);
int dip_events_destroy(void** events, int n);

/* One optimisation iteration as ONE call -- the body of the reference's loop, `optimizer.zero_grad(); closure();
 * optimizer.step()` (utils/common_utils.py:223-230) around the closure of inpainting.ipynb:300-315 / denoising.ipynb:204-221
 * (reg-noise, net(net_input), masked MSE, backward()) -- once the head, the noise and the optimiser are known statically:
 * the command lists of its phases (reg-noise + weight repack + input layout | forward list | dip_loss_head_fwd, BatchNorm
 * batch counters, dip_loss_head_bwd | backward list | dip_adam_tick + dip_adam_step_dev) issued back to back on ONE stream
 * table.  No autograd graph, no per-phase foreign call.  A phase is a command array as dip_list_run takes it plus the event
 * table ITS records / waits index (phases do not share events), so the forward / backward phases are the arrays the
 * engine issues through dip_list_run: same launches, same order, same fork / join events.  Allocates nothing, never
 * synchronises.  Returns 0, or the rc of the first failing command with failed_at[0] = its phase, failed_at[1] = its index
 * in that phase (failed_at: int[2] or NULL).  Python wrapper: dip_native.IterList, used by dip_optim.NativeIteration. */
typedef struct DipPhase {
    const DipCmd* cmds;
    void* const* events;
    int32_t n, nevents;
} DipPhase;
int dip_iter_run(const DipPhase* phases, int nphases, void* const* streams, int nstreams, int* failed_at);

/* ---------------------------------------------------------------- grouped execution --------- */
/* B independent fits in ONE launch list: B copies of the skip-net of models/skip.py:45-100 --
 * own weights, own BatchNorm statistics, own Adam state, own input and target -- with identical architecture and sizes.
 * The caller carves EVERY buffer of a fit (arenas, activations, scratch, the DipPackRec tables, input, target, loss)
 * from one slab per instance; the slabs are the rows of one [ninst][stride_bytes] allocation, laid out identically.  It
 * builds the descriptors of instance 0 and issues the launch list once between dip_group_begin and dip_group_end: every
 * launch of this library then serves all instances, instance b with each non-NULL pointer argument and descriptor field
 * advanced by b * stride_bytes (base / row_bytes = slab of instance 0: a pointer outside it fails the call, rc -1).  Plans,
 * tile walks and summation orders are those of a solo launch, so each instance's results are bit-identical to the same fit
 * run on its own.  Kernels with a grouped form run B instances in one dispatch (gridDim.z x B); the others are dispatched B
 * times by the library (csrc/dip_group.h).  Host-side state, thread-local: a group replicates the launches of the thread
 * that opened it only; hipGraph-capturable like a solo list.
 * dip_group_native: bit mask of the kernel families whose one-dispatch form is in use (default all; DIP_GROUP_NATIVE);
 * mask < 0 only queries.  Returns the previous mask.  dip_group_size: instances of the open group (1: none). */
int dip_group_begin(int ninst, long long stride_bytes, const void* base, long long row_bytes);
int dip_group_end(void);
int dip_group_size(void);
int dip_group_native(int mask);

/* Per-channel input transform fused into a consumer's loader:
 *   u = act(t),  t = a[c]*x + b[c];  act = max(t, slope*t) for slope in (0, 1] (slope = 1 -> affine
 *   only), t*sigmoid(t) for slope == DIP_ACT_SWISH, ELU(alpha=1) for slope == DIP_ACT_ELU, max(t, 0) for DIP_ACT_RELU
 * This is BatchNorm2d(train)-apply (models/common.py:95-96) + act() (models/common.py:76-92:
 * LeakyReLU(0.2), Swish, ELU, none) with a = gamma*rstd, b = beta - mean*a.  a == NULL -> identity. */
typedef struct DipTransform {
    const float* a;
    const float* b;
    float slope;
} DipTransform;

/* ---------------------------------------------------------------- layout / head ------------ */
/* NCHW [C][H*W] -> NHWC [H*W][Cs] (pad channels zeroed).  Boundary of `net(net_input)`:
 * get_noise() makes [1,C,H,W] NCHW (utils/common_utils.py:140). */
int dip_nchw_to_nhwc(const float* src, float* dst, int C, int HW, int Cs, void* stream);
/* NHWC [H*W][Cs] -> NCHW [C][H*W], optionally adding into dst (grad wrt net_input). */
int dip_nhwc_to_nchw(const float* src, float* dst, int C, int HW, int Cs, int accumulate, void* stream);
/* out[c][p] = sigmoid(y[p][c]) (or copy): nn.Sigmoid, models/skip.py:97-98; NHWC -> NCHW. */
int dip_head_fwd(const float* y, float* out, int C, int HW, int Cs, int sigmoid, void* stream);
/* dy[p][c] = gout[c][p] * out[c][p]*(1-out[c][p]) (sigmoid backward); NCHW -> NHWC. */
int dip_head_bwd(const float* gout, const float* out, float* dy, int C, int HW, int Cs, int sigmoid,
                 void* stream);

/* ---------------------------------------------------------------- weights ----------------- */
/* One record per Conv2d: repacks OIHW weights (nn.Conv2d, models/common.py:120) from the flat
 * parameter arena into the MFMA B-operand layouts used by dip_conv_igemm:
 *   forward : Wf[tap][c/4][o (CoutP32)][c%4]          = W[o][c][tap]
 *   dgrad   : Wd[tap][o/4][c (CinP32)][o%4]           = W[o][c][KS*KS-1-tap]
 * offsets are in floats; dgrad_off < 0 skips the dgrad pack. */
typedef struct DipPackRec {
    int64_t w_off;      /* into `params` */
    int64_t fwd_off;    /* into `packed` */
    int64_t dgrad_off;  /* into `packed`, or -1 */
    int32_t Cout, Cin, KS;
    int32_t CinP4, CoutP32, CoutP4, CinP32;
} DipPackRec;
int dip_pack_weights(const float* params, float* packed, const DipPackRec* recs_dev, int nrec,
                     int max_elems, void* stream);
/* The same weights as THREE bf16 planes for the bf16-pipe convolution (conv_bf3.hip: w == w1 + w2 + w3 exactly, 8 + 8 + 8
 * significand bits), [tap][k / 16][plane][n][16 k] bf16:  forward: k = input channel, n = output channel (CoutP32 of them);
 * data gradient: k = output channel, n = input channel (CinP32), taps flipped.  Offsets in bf16 elements, -1 = skip. */
typedef struct DipPackRec3 {
    int64_t w_off;      /* into `params` (floats) */
    int64_t fwd_off;    /* into `packed3` (bf16 elements), or -1 */
    int64_t dgrad_off;  /* into `packed3`, or -1 */
    int32_t Cout, Cin, KS;
    int32_t nchF, CoutP32, nchD, CinP32;   /* nchF = ceil(CinP4 / 16), nchD = ceil(CoutP4 / 16) */
} DipPackRec3;
int dip_pack_weights_bf3(const float* params, void* packed3, const DipPackRec3* recs_dev, int nrec, long long max_elems,
                         void* stream);

/* ---------------------------------------------------------------- convolution ------------- */
/* In-launch finalisation of the BatchNorm2d that follows a launch (dip_upcat_fwd_fin; opt-in, DIP_TICKET_FIN=1): the last
 * workgroup to arrive (fence-free ticket, one counter per 32-channel block) reduces the partial rows in fp64 and
 * writes the state block + running statistics -- exactly what dip_bn_finalize computes in a launch of its own
 * (nn.BatchNorm2d training forward, models/common.py:95-96).  state == NULL: off (the caller runs dip_bn_finalize).
 * `ticket` points at zero-initialised counters (ceil(Cout / 32) of them) that the launch leaves at zero. */
typedef struct DipBnFin {
    const float* gamma;
    const float* beta;
    float eps, momentum;
    float* state;                /* [4][Cs]: mean, rstd, a, b */
    int32_t Cs, C;
    float* running_mean;         /* or NULL */
    float* running_var;
    uint32_t* ticket;
} DipBnFin;
/* The same for phase 2 of a BatchNorm backward (dip_bn_bwd_stats_fin, dip_upsample_bwd_stats_crop_fin): dgamma, dbeta (may be NULL) and coef [2][bnb_Cs] = {k1 = S1 / npix, k2 = S2 / npix}, what
 * dip_bn_bwd_finalize computes.  coef == NULL: off. */
typedef struct DipBnbFin {
    float* dgamma;
    float* dbeta;
    float* coef;
    int32_t C, npix;
    uint32_t* ticket;
} DipBnbFin;

/* Implicit-GEMM convolution on the fp32 MFMA (v_mfma_f32_32x32x2_f32):
 *   y[q][o] (+)= bias[o] + sum_{tap,c} u[src(q,tap)][c] * Wp[tap][c][o],  u = transform(x)
 * per spatial dim  v = q*stride + k - off ; pad_mode reflect mirrors v into [0,Hv), zero drops
 * it;  Hv = (Hin-1)*dil + 1 ; dil == 2 reads x[v/2] for even v and 0 for odd v.
 * Replaces ReflectionPad2d + Conv2d (models/common.py:114-124) for the forward
 * (off = pad, dil = 1) and autograd's ConvolutionBackward data-gradient (transposed conv for
 * the stride-2 layers, models/skip.py:64) with flipped weights (off = KS-1-zero_pad, stride 1,
 * dil = forward stride; with reflection padding the result is the gradient on the PADDED
 * domain, folded back by dip_bn_bwd_stats / dip_fold_add).
 * stats != NULL: per-workgroup BatchNorm partials {count, mean, M2}[CoutP32] per tile
 * (Chan/Welford form) for the BatchNorm2d that follows the conv (models/common.py:95-96). */
typedef struct DipConvDesc {
    const float* x;
    int32_t Hin, Win, Cx, Cin;   /* Cx = channel stride of x, Cin = channels convolved (mult of 4) */
    DipTransform tr;
    const float* wp;             /* packed weights (see DipPackRec) */
    const float* bias;           /* [Cout] or NULL */
    float* y;
    int32_t Hout, Wout, Cy, Cout; /* Cy = channel stride of y */
    int32_t y_pitch;             /* pixels per output row in memory (0 -> Wout); lets a 1x1 dgrad
                                    accumulate into the interior of a padded gradient buffer */
    int32_t ks, stride, pad_mode, off, dil, accumulate;
    float* stats;                /* [stats_rows][3][CoutP32] or NULL (rows: dip_conv_plan) */
    int32_t ksplit;              /* <= 1: one pass.  > 1: split-K over (channel chunk, tap) units into
                                    `ws`, then a fixed-order reduction (small images: too few tiles
                                    to fill 256 CUs otherwise); take the value from dip_conv_plan */
    float* ws;                   /* split-K workspace, ksplit*Hout*Wout*Cy floats, or NULL */
    /* Optional (data-gradient launches): phase 1 of the backward of the BatchNorm(+activation) that PRODUCED this
     * convolution's input in the forward pass, fused into the epilogue.  The launch's output is the gradient g wrt
     * that BatchNorm's activated output on a domain padded by bnb_pad (reflection padding: the fold of the ring is
     * linear, so every padded position contributes with the activation of its mirror pixel):
     *   {sum g*act'(z), sum g*act'(z)*xhat},  z = a*y + b,  per output tile and channel
     *   -> bnb_partials [dip_conv_ntiles(Hout, Wout)][2][bnb_Cs]   (8x16-pixel tiles; columns >= 128 of a
     *      129..132-column gradient come from conv_thin4: bnb_partials_thin [dip_conv_thin4_ntiles()][2][bnb_Cs])
     * i.e. what dip_bn_bwd_stats(dz = NULL) computes in a pass of its own over g and y (autograd
     * NativeBatchNormBackward + LeakyReluBackward of models/common.py:82,96); dip_bn_bwd_finalize2 reduces the
     * rows.  bnb_y == NULL: off.  Only one-pass launches (dip_conv_bnb_fusable). */
    const float* bnb_y;          /* raw output y of the conv in front of that BatchNorm, [H][W][bnb_Cy], H = Hout - 2*bnb_pad */
    const float* bnb_state;      /* its state block [4][bnb_Cs]: mean, rstd, a, b */
    float* bnb_partials;
    float* bnb_partials_thin;
    int32_t bnb_Cy, bnb_Cs, bnb_pad;
    float bnb_slope;
    /* Optional: the same weights as three bf16 planes (DipPackRec3).  When set, dip_conv_igemm runs the 3x3 stride-1 layers
     * with >= 256 tiles on the bf16 matrix pipe: every fp32 operand split EXACTLY into three bf16 terms (8 + 8 + 8
     * significand bits), the cross products -- each exact in fp32 -- accumulated in fp32 by v_mfma_f32_32x32x16_bf16: the
     * same roundings as an fp32 fmaf chain (measured error vs fp64 below the fp32 MFMA's).  Default: eight of the nine
     * (lo x lo, < 2^-32 of a*b, is left out; half the fp32 matrix-pipe time, conv_bf3.hip); DIP_CONV_BF3=9: all nine;
     * =0: fp32 MFMA everywhere; =6: without the three smallest products (each < 2^-24 of a*b).  NULL: fp32 MFMA. */
    const void* wp3;
} DipConvDesc;
int dip_conv_igemm(const DipConvDesc* d, void* stream);
/* number of 8x16 output tiles */
int dip_conv_ntiles(int Hout, int Wout);
/* number of 16x16 output tiles of dip_conv_thin4 (rows of bnb_partials_thin) */
int dip_conv_thin4_ntiles(int Hout, int Wout);
/* 1 when dip_conv_igemm runs `d` in one pass through a kernel whose epilogue can emit the fused BatchNorm-backward
 * partials (bnb_* fields; evaluated with bnb_y ignored): no split-K, not the phase mode, not the N = 160 variant */
int dip_conv_bnb_fusable(const DipConvDesc* d);
/* launch plan of one convolution: split-K factor, rows of the statistics partial buffer and the
 * split-K workspace size in floats (0 when *ksplit == 1) */
int dip_conv_plan(int Hout, int Wout, int Cin, int Cout, int ks, int stride, int* ksplit, int* stats_rows,
                  int64_t* ws_floats);
/* the same for a layer that is NOT taken by the bf16-pipe kernel although its shape is (no DipConvDesc.wp3, a transform over
 * more than 512 input channels, fused bnb_* partials): without the "96..255 tiles run the 64-column bf16 form in one pass"
 * rule, i.e. split-K as the fp32 kernels want it.  The engine re-plans with it when dip_conv_bf3_eligible(d) == 0. */
int dip_conv_plan_fp32(int Hout, int Wout, int Cin, int Cout, int ks, int stride, int* ksplit, int* stats_rows,
                       int64_t* ws_floats);
/* launch plan of the data gradient of a stride-2 3x3 convolution (a dil == 2 descriptor; Hout x Wout is
 * the gradient's domain, Cin/Cout the descriptor's): the LDS-DMA kernel's phase mode evaluates it as 4
 * dense sub-filter convolutions, one per output-pixel parity (9 taps per 4 pixels instead of 36), with its
 * own split-K bound.  Other filter sizes / column counts get dip_conv_plan's answer. */
int dip_conv_plan_dil2(int Hout, int Wout, int Cin, int Cout, int ks, int* ksplit, int* stats_rows,
                       int64_t* ws_floats);
/* which kernel dip_conv_igemm launches for `d` (diagnostic; bench.py attributes its HIP-event times
 * with it): 0 = conv_igemm_kernel (operands staged through registers: stride 2, 5x5),
 * 1 = conv_igemm_dma_kernel (LDS-DMA staging: stride-1 1x1 / 3x3), 2 = conv_igemm_kernel N=160 variant
 * (3x3, 129..160 output channels, split-K), 3 = conv_thin4_mfma_kernel (columns 0..Cout-129: the tap sum pulled out of the
 * contraction, v_mfma_f32_16x16x4_f32 fed straight from global memory; the vector-ALU conv_thin4_kernel above 128 input channels
 * and with fused BatchNorm-backward partials) + conv_igemm_dma_kernel (the other 128 columns): 3x3 data gradients towards a
 * 132-channel tensor,
 * 4 = conv_igemm_dma_kernel in phase mode (dil == 2: data gradient of a stride-2 3x3 convolution),
 * 5 = conv_igemm_dma_kernel in strided-forward mode (3x3, stride 2: the input split by pixel parity),
 * 6 = conv1x1_res_kernel (1x1, 128 -> 97..128 channels, >= 256x256 pixels: persistent workgroups, weights in registers),
 * 7 = conv_bf3_kernel (3x3 stride 1 on the bf16 matrix pipe), 8 = conv_thin_kernel (<= 64 channels in and out, 3x3 / 5x5,
 * 16x16x4 MFMA tiles, all taps' weights LDS-resident: the high-resolution layers of the narrow nets) */
int dip_conv_variant(const DipConvDesc* d);
/* The two launches behind variant 3, exported so that a caller can put them on DIFFERENT streams (they
 * write disjoint columns of the same output): columns [0, ncols) (ncols = Cout - 128 <= 4) of a 3x3
 * stride-1 transform-free convolution (matrix-pipe form up to 128 input channels, vector ALU beyond), and one 128-column block starting at column
 * n_base on the LDS-DMA kernel.  Same descriptor as dip_conv_igemm. */
int dip_conv_thin4(const DipConvDesc* d, int ncols, void* stream);
int dip_conv_igemm_dma_cols(const DipConvDesc* d, int n_base, void* stream);
/* Thin layers (round 6, csrc/conv_thin.hip): 3x3 / 5x5, stride 1 / 2 (forward) or the stride-1 data gradient, <= 64 input
 * and output channels, at least 4625 output pixels -- the 16 / 32 / 64-channel layers of the
 * 'library' inpainting net (inpainting.ipynb:222-232) and the snail net (denoising.ipynb:143-150) at their high
 * resolutions; same contract as dip_conv_igemm (which dispatches to it: dip_conv_variant == 8), one pass, stats rows =
 * dip_conv_ntiles.  dip_conv_thin_shape_ok: the shape part of the eligibility (what dip_conv_plan knows). */
int dip_conv_thin(const DipConvDesc* d, void* stream);
int dip_conv_thin_eligible(const DipConvDesc* d);
int dip_conv_thin_shape_ok(int Hout, int Wout, int Cin, int Cout, int ks, int stride);
/* Low-resolution layers (models/skip.py:57-91 at depth >= 2: <= 64x64 outputs in the notebooks' nets): ONE launch per
 * convolution instead of conv + split-K finish.  A workgroup computes one 32-pixel x 32-channel tile; its 4 / 8 / 16 waves
 * split K, each with its whole slice of operand loads in flight at once, straight from L2 into the MFMA registers (no LDS
 * staging: such a layer is latency-bound, not bandwidth-bound), and are summed through LDS in a fixed order; the epilogue
 * emits the BatchNorm partials (`stats`: [rows][3][CoutP32], for dip_bn_finalize) or -- data gradients -- the d->bnb_*
 * partials ([rows][2][bnb_Cs], for dip_bn_bwd_finalize2 with nblk_lo = 0); any 1..160 output columns (no conv_thin4 side
 * launch).  1x1 / 3x3, stride 1 / 2, dil 1 / 2 (dil == 2: per output-parity class, only the taps that hit non-zero
 * positions), every padding mode and activation; d->ksplit / d->ws are ignored.
 * dip_conv_small_eligible: the shape is served AND Hout * Wout <= 4624 (= 68 x 68);
 * dip_conv_small_rows: rows of the partial buffers (0: shape not served). */
int dip_conv_small(const DipConvDesc* d, void* stream);
int dip_conv_small_eligible(const DipConvDesc* d);
int dip_conv_small_rows(const DipConvDesc* d);
/* Data gradient of a reflection-padded 3x3 stride-1 convolution WITHOUT the padded domain (models/common.py:116-121 +
 * autograd's ReflectionPad2dBackward): the caller computes the interior H x W positions as a plain zero-padded correlation
 * (dip_conv_igemm with off = 1: 512 tiles at 256^2 instead of the 561 of the (H+2) x (W+2) domain) and this launch adds
 * what the ring of the padded domain folds onto the frame rows 1, H-2 / columns 1, W-2 -- per frame pixel the gradient of
 * the <= 3 ring positions that mirror onto it, accumulated into y.  `d` = the interior descriptor (x = dy [H][W],
 * y = gradient [H][W][Cy], ks 3, stride 1, dil 1, off 1, DIP_PAD_ZERO, no transform / bias / stats).  The gradient buffer
 * then needs no fold (DipGradSrc.pad = 0).  dip_conv_dgrad_ring_ok: shape served and H * W <= 300000
 * (up to 512 x 512). */
int dip_conv_dgrad_ring(const DipConvDesc* d, void* stream);
int dip_conv_dgrad_ring_ok(const DipConvDesc* d);
/* bf16-pipe convolution (see DipConvDesc.wp3): eligibility of `d`, the launch of columns [n_base, n_base + ncols) and the
 * number of cross products in use (0 = off, 9, 6) */
int dip_conv_bf3_eligible(const DipConvDesc* d);
int dip_conv_bf3_cols(const DipConvDesc* d, int n_base, int ncols, void* stream);
int dip_conv_bf3_terms(void);
/* overrides DIP_CONV_BF3 for this process: 0 (off), 6, 8 (without lo x lo: < 2^-32 of a product), 9; -1 = back to the environment */
int dip_conv_bf3_set_terms(int terms);
/* second half of a split-K dispatch (d->ksplit > 1): fixed-order sum of the workspace slices, bias,
 * store, BatchNorm partials.  dip_conv_igemm calls it itself; exported for per-kernel timing. */
int dip_conv_splitk_finish(const DipConvDesc* d, void* stream);

/* Weight gradient (autograd ConvolutionBackward, weight + bias part):
 *   dW[o][c][tap] = sum_q dy[q][o] * u[src(q,tap)][c],  db[o] = sum_q dy[q][o]
 * Two stages, deterministic: dip_conv_wgrad writes `nsplit` partial slabs
 * [nsplit][tap][CinP32][CoutP32] (+ [nsplit][CoutP32] bias partials), dip_wgrad_reduce sums the
 * slabs in a fixed order and writes OIHW gradients into the grad arena. */
typedef struct DipWgradDesc {
    const float* x;
    int32_t Hin, Win, Cx, Cin;
    DipTransform tr;
    const float* dy;
    int32_t Hout, Wout, Cdy, Cout;
    int32_t ks, stride, pad_mode, off;
    float* partial;
    float* bias_partial;          /* or NULL */
    int32_t nsplit;
    int32_t tap_groups;           /* 3x3 MFMA kernel: the 9 taps are spread over 1, 3 or 9 workgroups (more, lighter
                                     workgroups for low-resolution layers); 0 = 1.  From dip_wgrad_plan2. */
    int32_t chan_block;           /* 1x1 MFMA kernel: input channels per workgroup / 32: 4 (default, 0) or 1 */
} DipWgradDesc;
int dip_conv_wgrad(const DipWgradDesc* d, void* stream);
/* dip_conv_wgrad routes the 3x3 stride-1 layers with >= 32 input channels and >= 256 x 256 outputs to the bf16 matrix pipe
 * (wgrad_bf3.hip: the exact three-way operand split of DipConvDesc.wp3's kernel, here applied to BOTH activations while
 * they are staged transposed in LDS; same slabs, same dip_wgrad_reduce): eligibility, the launch, and the
 * (tap, channel)-packed <= 4-channel tail of a 132-channel layer that stays on the fp32 MFMA (phase 2 of the fp32 kernel on
 * its own).  DIP_WGRAD_NO_BF3=1 / DIP_CONV_BF3=0 switch it off. */
int dip_wgrad_bf3_eligible(const DipWgradDesc* d);
int dip_wgrad_bf3(const DipWgradDesc* d, void* stream);
int dip_conv_wgrad_tail(const DipWgradDesc* d, void* stream);
/* The same rows as a streaming kernel (round 6, wgrad_tail.hip; dip_conv_wgrad_tail dispatches to it): (tap, channel) packed
 * into the rows of the fp32 MFMA, K = pairs of output pixels straight from global memory, one pass over dy, the slabs of
 * `d->nsplit` walkers written like the bf16-pipe kernel's.  _ok: 3x3, stride 1, 1..4 channels behind whole 32-channel chunks. */
int dip_wgrad_tail_stream_ok(const DipWgradDesc* d);
int dip_wgrad_tail_stream(const DipWgradDesc* d, void* stream);
/* Thin layers (round 6, csrc/wgrad_thin.hip): 3x3 / 5x5, stride 1 / 2, 8..64 input channels, <= 64 output channels, >= 4096
 * output pixels -- the 16 / 32 / 64-channel convs of the 'library' and snail nets (inpainting.ipynb:222-232,
 * denoising.ipynb:143-150): 16-channel x 16-column x 4-pixel MFMA tiles, the taps spread over the workgroup's waves; same
 * slabs, same dip_wgrad_reduce.  dip_conv_wgrad dispatches to it; nsplit from dip_wgrad_plan / dip_wgrad_plan2
 * (= dip_wgrad_thin_nsplit for these shapes). */
int dip_wgrad_thin(const DipWgradDesc* d, void* stream);
int dip_wgrad_thin_eligible(const DipWgradDesc* d);
int dip_wgrad_thin_shape_ok(int Hout, int Wout, int Cin, int Cout, int ks, int stride);
int dip_wgrad_thin_nsplit(int Hout, int Wout, int Cin, int Cout, int ks, int stride);
/* number of 4x16 output tiles walked by the wgrad workgroups (upper bound for nsplit) */
int dip_conv_wgrad_ntiles(int Hout, int Wout);
/* nsplit (number of partial slabs) to run dip_conv_wgrad with; mandatory for 1x1 convs with
 * Cout <= 8 and for 3x3 / 5x5 / 7x7 convs with <= 4 INPUT channels (the first conv of a net), which take thin
 * vector-ALU streaming kernels with one slab per block */
int dip_wgrad_plan(int Hout, int Wout, int Cin, int Cout, int ks, int stride, int* nsplit);
/* the full launch plan: nsplit plus the tap_groups / chan_block fields of DipWgradDesc.  Large layers
 * get (nsplit as dip_wgrad_plan, 1, 4); layers with <= 256 pixel tiles (<= 128x128 outputs) trade
 * taps-per-workgroup and slabs against workgroup count with a small cost model so that a 16x16 layer
 * runs ~150 light workgroups instead of 4 heavy ones. */
int dip_wgrad_plan2(int Hout, int Wout, int Cin, int Cout, int ks, int stride, int* nsplit, int* tap_groups,
                    int* chan_block);
int dip_wgrad_reduce(const float* partial, const float* bias_partial, int nsplit, int ks, int Cin,
                     int Cout, float* dw /*OIHW*/, float* dbias /*or NULL*/, void* stream);

/* ---------------------------------------------------------------- BatchNorm (train mode) -- */
/* state block per BatchNorm: 4 rows of Cs floats: mean, rstd, a, b  (a = gamma*rstd, b = beta - mean*a) */
/* Combine per-tile partials -> batch statistics, update running stats (momentum 0.1, unbiased
 * var), nn.BatchNorm2d training forward (models/common.py:95-96). */
int dip_bn_finalize(const float* partials, int ntiles, int Cstride, int C, const float* gamma,
                    const float* beta, float eps, float momentum, float* state, int Cs,
                    float* running_mean, float* running_var, void* stream);

/* Source of an incoming activation gradient `du` for pixel (r,c), channel ch:
 *   du = sum over folded positions of  g[((r+pad)*Wg + (c+pad)) * Cg + choff + ch]
 * fold == 1 adds the mirror images of the reflection-padded border (adjoint of
 * nn.ReflectionPad2d, models/common.py:116-118), fold == 2 the ring positions that nn.ReplicationPad2d clamps onto a
 * border pixel (models/downsampler.py:56-61); Hg = H + 2*pad, Wg = W + 2*pad. */
typedef struct DipGradSrc {
    const float* g;
    int32_t pad, fold, Cg, choff;
    /* Optional crop window (win_h > 0, then pad == 0): g is a [win_h][win_w] tensor that covers rows win_y..win_y+win_h-1,
     * columns win_x..win_x+win_w-1 of the [H][W] activation; du = 0 outside (adjoint of Concat's centre crop,
     * models/common.py:29-37, for the branch that was cropped). */
    int32_t win_y, win_x, win_h, win_w;
    /* Optional thin 1x1 convolution in front of the activation (tw != NULL; then pad == 0, no window, choff == 0): g is the
     * gradient [H][W][Cg] of the OUTPUT of a bias + 1x1 conv with tn <= 4 output channels (the net's last nn.Conv2d,
     * models/skip.py:98: num_channels_up[0] -> num_output_channels) and
     *   du[ch] = sum_{j < tn} g[(r*W + c) * Cg + j] * tw[j * tcw + ch]          (tw = that conv's OIHW weight, tcw = its Cin)
     * is evaluated where it is consumed -- the conv's data gradient (autograd ConvolutionBackward, input part) is never
     * written to memory: one launch and three passes over an activation-sized tensor less per iteration. */
    const float* tw;
    int32_t tn, tcw;
} DipGradSrc;

/* BatchNorm+LeakyReLU backward, phase 1:  dz = du * (a*y+b > 0 ? 1 : slope); writes dz (unless
 * dz == NULL: then phase 3 is dip_bn_bwd_apply_src, which recomputes it) and the per-block partial
 * sums {sum dz, sum dz*xhat}.  (autograd NativeBatchNormBackward + LeakyReluBackward of
 * models/common.py:82,96.) */
int dip_bn_bwd_stats(const DipGradSrc* src, const float* y, int H, int W, int Cy, int C,
                     const float* state, int Cs, float slope, float* dz, int Cdz,
                     float* partials /*[nblk][2][Cs]*/, int nblk, void* stream);
int dip_bn_bwd_nblk(int H, int W, int C);
/* phase 1 + in-launch phase 2 (fin->coef != NULL; needs dip_fin_rows_ok(nblk, C)): the last block to arrive writes
 * dgamma, dbeta and coef, no dip_bn_bwd_finalize launch */
int dip_bn_bwd_stats_fin(const DipGradSrc* src, const float* y, int H, int W, int Cy, int C,
                         const float* state, int Cs, float slope, float* dz, int Cdz,
                         float* partials /*[nblk][2][Cs]*/, int nblk, const DipBnbFin* fin, void* stream);
/* phase 2: reduce partials -> dgamma, dbeta (grad arena) and k1 = S1/N, k2 = S2/N in `coef` [2][Cs] */
int dip_bn_bwd_finalize(const float* partials, int nblk, int Cs, int C, int npix, float* dgamma,
                        float* dbeta, float* coef, void* stream);
/* phase 2 over two partial buffers: channels < c_lo from partials_lo [nblk_lo][2][Cs] (the conv_thin4 columns of a
 * 129..132-column data gradient with fused statistics), the others from partials [nblk][2][Cs]; c_lo % 4 == 0 */
int dip_bn_bwd_finalize2(const float* partials, int nblk, const float* partials_lo, int nblk_lo, int c_lo, int Cs,
                         int C, int npix, float* dgamma, float* dbeta, float* coef, void* stream);
/* phase 3 (in place): dy = a * (dz - k1 - xhat*k2) */
int dip_bn_bwd_apply(float* dz, int Cdz, const float* y, int Cy, int npix, int C, const float* state,
                     int Cs, const float* coef, void* stream);
/* phase 3 straight from the gradient source (one tensor pass less than stats-with-dz + apply):
 *   dy = a * (du * lrelu'(a*y+b) - k1 - xhat*k2) */
int dip_bn_bwd_apply_src(const DipGradSrc* src, const float* y, int H, int W, int Cy, int C,
                         const float* state, int Cs, float slope, const float* coef, float* dy, int Cdy,
                         void* stream);
/* The three phases in ONE launch for low-resolution activations (round 6; csrc/bn_bwd_one.hip): a workgroup owns four
 * channels of the whole H x W plane, so S1 = sum dz and S2 = sum dz * xhat are workgroup-local (per-thread fp32 sums, a
 * fixed-order fp64 reduction) and dy = a * (du * act'(a*y+b) - S1/N - xhat * S2/N) follows in the same launch; dgamma,
 * dbeta and coef [2][Cs] are written as dip_bn_bwd_finalize writes them (each may be NULL).  Same reference ops as
 * dip_bn_bwd_stats / _finalize / _apply_src (autograd NativeBatchNormBackward + LeakyReluBackward of
 * models/common.py:82,96).  dip_bn_bwd_one_ok: 1 when the engine should use this form (npix <= 1024
 * = 32 x 32: above that a 4-channel slice of the plane costs 8x its bytes in L1 fills). */
int dip_bn_bwd_one_ok(int npix, int C);
int dip_bn_bwd_one(const DipGradSrc* src, const float* y, int H, int W, int Cy, int C, const float* state, int Cs,
                   float slope, float* dy, int Cdy, float* dgamma, float* dbeta, float* coef, void* stream);
/* Fold a (reflection-)padded gradient back onto the image and emit it NCHW: gradient wrt
 * `net_input` for get_params('net,input') (utils/common_utils.py:47-49). */
int dip_fold_to_nchw(const DipGradSrc* src, int H, int W, int C, float* dst, void* stream);
/* The same, NHWC out ([H][W][Cd]): dy of a conv whose output feeds a padded consumer directly, without a BatchNorm in
 * between (the stride-1 conv in front of the Lanczos Downsampler of conv(..., downsample_mode='lanczos2')). */
int dip_fold_to_nhwc(const DipGradSrc* src, int H, int W, int C, float* dst, int Cd, void* stream);

/* Residual join of the ResNet backbone (models/resnet.py:13-24 of the reference: ResidualSequential.forward ends in
 * `return out + x_`; the crop branch in front of it cannot trigger with the 3x3 / padding-1 convs of get_block):
 *   out[p][c] = act_a(ta.a[c] * xa[p][c] + ta.b[c]) + act_b(tb.a[c] * xb[p][c] + tb.b[c]),   p < npix, c < C
 * Both operands are read as raw NHWC conv outputs (channel strides Cxa, Cxb) and transformed on the fly; a transform with
 * a == NULL is the identity.  C and the strides are multiples of 4.  One read of each input, one write. */
int dip_res_join_fwd(const float* xa, int Cxa, const DipTransform* ta, const float* xb, int Cxb, const DipTransform* tb,
                     float* out, int Co, int npix, int C, void* stream);
/* Its adjoint (autograd AddBackward of the same `out + x_`, models/resnet.py:24) joined with the data gradient of the block's
 * first conv:  gout = (g + src) [* act'(ty.a[c] * y + ty.b[c])]
 * g = gradient wrt the block's output ([H][W][Cg], NULL = 0), src = the conv's data gradient where the conv launch left it
 * (padded / folded: DipGradSrc; no thin-conv source, no crop window).  y != NULL multiplies by the derivative of the
 * activation behind the net's first conv (models/resnet.py:60-61: conv + act, no BatchNorm in between) at its raw output
 * y, so the launch at the bottom of the chain writes dy of that conv. */
int dip_res_join_bwd(const float* g, int Cg, const DipGradSrc* src, const float* y, int Cy, const DipTransform* ty,
                     float* gout, int Cgo, int H, int W, int C, void* stream);

/* ---------------------------------------------------------------- upsample + concat ------- */
/* cat[p][0:ns]      = T_s(s[p])                      (skip branch, Concat child "0")
 * cat[p][ns:ns+nd]  = upsample2x(T_d(d))[p]          (deeper branch, nn.Upsample models/skip.py:81)
 * and the {count, mean, M2} partials of the BatchNorm2d(ns+nd) that follows (models/skip.py:55).
 * Concat: models/common.py:11-42.  Default geometry (Hs == 0): s is [H][W], d is [(H+1)/2][(W+1)/2] (an odd size drops
 * the last up-sampled row / column: the centre crop with offset 0).  General centre crop (models/common.py:29-37; pooling
 * nets or skip-less scales at sizes that 2^scales does not divide): Hs, Ws = size of s, (os_y, os_x) = its crop offset;
 * Hd, Wd = size of d, (od_y, od_x) = crop offset inside its [2*Hd][2*Wd] up-sampled image; H, W = the common (min) size. */
typedef struct DipUpcatDesc {
    const float* s; int32_t Cs_s, ns; DipTransform ts;      /* ns may be 0 (s == NULL) */
    const float* d; int32_t Cs_d, nd; DipTransform td;      /* low-res [H/2][W/2][Cs_d] */
    int32_t H, W, mode;                                      /* output (high-res) size */
    float* cat; int32_t Cs_cat;
    float* stats; int32_t nblk;                              /* [nblk][3][Cs_cat] */
    int32_t Hs, Ws, os_y, os_x;                              /* 0: default geometry */
    int32_t Hd, Wd, od_y, od_x;
} DipUpcatDesc;
int dip_upcat_fwd(const DipUpcatDesc* d, void* stream);
/* the same launch + in-launch finalisation of the concat BatchNorm (fin->state != NULL; needs dip_fin_rows_ok(d->nblk, ns + nd)) */
int dip_upcat_fwd_fin(const DipUpcatDesc* d, const DipBnFin* fin, void* stream);
/* 1 when a launch that writes `rows` partial rows of C channels may finalise them itself (<= 256 rows, <= 256 channels;
 * DIP_NO_TICKET_FIN=1 switches every in-launch finalisation off) */
int dip_fin_rows_ok(int rows, int C);
int dip_upcat_nblk(int H, int W, int C);

/* nn.AvgPool2d(2,2) behind a stride-1 conv (conv(..., downsample_mode='avg'), models/common.py:101-104):
 * x [H][W][Cx] -> y [H/2][W/2][Cy] (H, W even or floored) + the {count, mean, M2} partials
 * [nblk][3][Cy] of the BatchNorm that follows (nblk = dip_upcat_nblk(H/2, W/2, C); stats may be
 * NULL); the adjoint writes dx[r][c] = dy[r/2][c/2] / 4 (0 on a floored odd border). */
int dip_avgpool2_fwd(const float* x, int H, int W, int Cx, int C, float* y, int Cy, float* stats, int nblk,
                     void* stream);
int dip_avgpool2_bwd(const float* dy, int H, int W, int Cdy, int C, float* dx, int Cdx, void* stream);
/* nn.MaxPool2d(2,2) behind a stride-1 conv (conv(..., downsample_mode='max'), models/common.py:105-106):
 * same contract as dip_avgpool2_fwd; the adjoint routes dy to the first maximal element of each 2x2
 * window of x (ATen's tie rule), recomputing the arg-max from x, zeros elsewhere. */
int dip_maxpool2_fwd(const float* x, int H, int W, int Cx, int C, float* y, int Cy, float* stats, int nblk,
                     void* stream);
int dip_maxpool2_bwd(const float* dy, const float* x, int H, int W, int Cdy, int Cx, int C, float* dx, int Cdx,
                     void* stream);

/* Adjoint of the 2x upsample fused with the LeakyReLU/BatchNorm backward phase 1 of the
 * deeper branch: du_d = upsample2x^T(dcat[:, choff:choff+nd]); dz = du_d * lrelu'(a*y+b);
 * partial sums as in dip_bn_bwd_stats.  (autograd UpsampleBilinear2DBackward / Nearest.) */
int dip_upsample_bwd_stats(const float* dcat, int Cs_cat, int choff, int H, int W, int mode,
                           const float* y, int Cy, int C, const float* state, int Cs, float slope,
                           float* dz, int Cdz, float* partials, int nblk, void* stream);
/* the same with the general crop geometry of DipUpcatDesc: dcat is [H][W], the deeper branch [Hd][Wd] (y, dz), cropped at
 * (od_y, od_x) of its up-sampled image; nblk = dip_bn_bwd_nblk(Hd, Wd, C) */
int dip_upsample_bwd_stats_crop(const float* dcat, int Cs_cat, int choff, int H, int W, int Hd, int Wd, int od_y,
                                int od_x, int mode, const float* y, int Cy, int C, const float* state, int Cs,
                                float slope, float* dz, int Cdz, float* partials, int nblk, void* stream);

/* dip_upsample_bwd_stats_crop + in-launch phase 2 of the deeper branch's BatchNorm backward (fin as in dip_bn_bwd_stats_fin) */
int dip_upsample_bwd_stats_crop_fin(const float* dcat, int Cs_cat, int choff, int H, int W, int Hd, int Wd, int od_y,
                                    int od_x, int mode, const float* y, int Cy, int C, const float* state, int Cs,
                                    float slope, float* dz, int Cdz, float* partials, int nblk, const DipBnbFin* fin,
                                    void* stream);

/* Adjoint of the up-sampling + all three BatchNorm-backward phases of the deeper branch in ONE launch (the form of
 * dip_bn_bwd_one with dip_upsample_bwd_stats_crop's gradient source; autograd UpsampleBilinear2DBackward / Nearest +
 * NativeBatchNormBackward + LeakyReluBackward, models/skip.py:81, models/common.py:82,96): dy [Hd][Wd][Cdy] = gradient wrt
 * the raw output y of the deeper branch's last conv.  Use when dip_bn_bwd_one_ok(Hd * Wd, C). */
int dip_upsample_bwd_one(const float* dcat, int Cs_cat, int choff, int H, int W, int Hd, int Wd, int od_y, int od_x,
                         int mode, const float* y, int Cy, int C, const float* state, int Cs, float slope, float* dy,
                         int Cdy, float* dgamma, float* dbeta, float* coef, void* stream);

/* ---------------------------------------------------------------- optimiser --------------- */
/* torch.optim.Adam(lr) defaults, one fused launch over a flat arena
 * (utils/common_utils.py:225-230):  m += (1-b1)(g-m); v = b2 v + (1-b2) g^2;
 * p -= (lr/bc1) * m / (sqrt(v)/sqrt(bc2) + eps),  bc = 1 - beta^step. */
int dip_adam_step(float* p, const float* g, float* m, float* v, int64_t n, double lr, double beta1,
                  double beta2, double eps, int step, void* stream);

/* net_input = z + sigma * N(0,1): the closure's reg-noise line (denoising.ipynb:208-209),
 * counter-based Philox4x32-10 + Box-Muller, NCHW in / NCHW out (elementwise).  The stream is specified in DESIGN.md
 * ("The reg-noise stream").  All three entry points: n <= 0 returns 0 and launches nothing; a NULL z or out (or counter /
 * state pointer) with n > 0 returns -1 before anything is launched. */
int dip_noise_axpy(const float* z, float* out, int64_t n, float sigma, uint64_t seed, uint64_t offset,
                   void* stream);

/* ---------------------------------------------------------------- device-side iteration state */
/* Everything that changes from one optimisation iteration to the next on the HOST side of the
 * reference loop (utils/common_utils.py:226-230: the step count inside torch.optim.Adam; the
 * device RNG position behind `noise.normal_()`, denoising.ipynb:209) kept in DEVICE memory, so the
 * launch list of one iteration is static and can be captured once and replayed as a hipGraph. */
typedef struct DipIterState {
    uint64_t step;        /* Adam step count t (0 before the first step) */
    float step_size;      /* lr / (1 - beta1^t), written by dip_adam_tick */
    float bc2_sqrt;       /* sqrt(1 - beta2^t) */
} DipIterState;
/* t <- t + 1 and the two bias-correction scalars of torch.optim.Adam, computed in double. */
int dip_adam_tick(DipIterState* st, double lr, double beta1, double beta2, void* stream);
/* dip_adam_step with step_size / bc2_sqrt read from `st` (call dip_adam_tick first). */
int dip_adam_step_dev(float* p, const float* g, float* m, float* v, int64_t n, double beta1, double beta2,
                      double eps, const DipIterState* st, void* stream);
/* dip_noise_axpy whose Philox offset lives at *offset_dev and is advanced by ceil(n/4) afterwards. */
int dip_noise_axpy_dev(const float* z, float* out, int64_t n, float sigma, uint64_t seed, uint64_t* offset_dev,
                       void* stream);
/* dip_noise_axpy_dev with the seed in device memory too: state_dev = {offset, seed} (two uint64).  In a group every
 * instance reads its own pair, i.e. draws its own stream. */
int dip_noise_axpy_dev2(const float* z, float* out, int64_t n, float sigma, uint64_t* state_dev, void* stream);
/* The hyper-parameters of a sweep or a schedule in DEVICE memory, next to the state above: the launch reads the scalar where it
 * lives, a setter rewrites it in stream order (one fill on the stream), and neither a command array nor a captured hipGraph
 * holds its value.  Inside dip_group_begin / dip_group_end lr_dev / sigma_dev are grouped pointers like st / state_dev: every
 * instance reads the scalar of its own slab row.
 *
 * dip_adam_tick_dev: dip_adam_tick with lr = *lr_dev (one fp64).  The same double arithmetic in the same order:
 *     t <- t + 1;  step_size = (float)(lr / (1 - beta1^t));  bc2_sqrt = (float)sqrt(1 - beta2^t)
 * so the 16 bytes of *st are those dip_adam_tick writes for the same lr.
 * dip_noise_axpy_dev3: dip_noise_axpy_dev2 with sigma = *sigma_dev (one fp32): out[i] = fmaf(sigma, N_i, z[i]), N_i normal
 * i % 4 of Philox quad offset + i / 4 under key seed, {offset, seed} = state_dev[0..1]; state_dev[0] += ceil(n / 4) behind the
 * launch.  sigma == 0 still draws and advances: out = z + 0 * N (a -0.0 of z comes out as +0.0).
 * dip_noise_axpy_dev1s: the solo counterpart, dip_noise_axpy_dev with sigma = *sigma_dev: the seed by value, the offset at
 * *offset_dev, advanced the same way.  All three run the body of the kernel they are named after.
 * A NULL st / lr_dev / z / out / sigma_dev / state_dev / offset_dev, or n <= 0, returns -1 before anything is launched. */
int dip_adam_tick_dev(DipIterState* st, const double* lr_dev, double beta1, double beta2, void* stream);
int dip_noise_axpy_dev3(const float* z, float* out, int64_t n, const float* sigma_dev, uint64_t* state_dev, void* stream);
int dip_noise_axpy_dev1s(const float* z, float* out, int64_t n, const float* sigma_dev, uint64_t seed, uint64_t* offset_dev,
                         void* stream);
/* *counter += inc (one thread; ordering by the stream). */
int dip_counter_add(uint64_t* counter, uint64_t inc, void* stream);
/* counters[i] += inc for i < n in one launch: `num_batches_tracked += 1` of every nn.BatchNorm2d of the net in train mode
 * (models/common.py:82,95 through torch.nn.BatchNorm2d.forward), whose counters the engine keeps in one int64 arena. */
int dip_counter_add_n(uint64_t* counters, int n, uint64_t inc, void* stream);

/* ---------------------------------------------------------------- SGLD: Adam + weight decay + parameter noise ---- */
/* Langevin sampling of the weights (Cheng et al., "A Bayesian Perspective on the Deep Image Prior", CVPR 2019): after the
 * optimiser step Gaussian noise is added to the convolution weights, with a small weight decay as the Gaussian prior.  ONE
 * launch over a flat arena does the Adam update with optional weight decay and adds Philox noise to the elements inside a
 * table of noised ranges.  Per element i of p, with wd = (float)weight_decay:
 *   g'  = wd != 0 ? fmaf(wd, p[i], g[i]) : g[i]     one rounding, what ATen's CPU grad.add(param, alpha=wd) computes; with
 *                                                   weight_decay == 0 the fma is skipped: g' = g bit for bit, -0.0 included
 *   m', v', p1 = the sequence of dip_adam_step on g', rounding for rounding
 *   p[i] = i inside a noised range ? fmaf(std, nrm(i), p1) : p1
 * nrm(i) is normal number i % 4 of Philox quad offset + i / 4 of the reg-noise stream (DESIGN.md "The reg-noise stream")
 * under key seed ^ 0x53474C4453474C44 ("SGLDSGLD"): without the XOR a RegNoise(seed=0) and an SGLD stream of seed 0 would add
 * the SAME normals to the input and to the first weights.  Quads are indexed from p, not from a range start, so the stream
 * does not depend on the table; the normals of elements outside the ranges are dropped.
 * ranges: nranges x {begin, end} int64 in DEVICE memory, in elements of p, sorted and disjoint, at most 512 of them; what lies
 * beyond n is ignored.  _dev reads step_size / bc2_sqrt from `st` (dip_adam_tick first) and offset / seed / std from *noise, and
 * advances noise->offset by ceil(n / 4) behind the launch, the way dip_noise_axpy_dev2 advances its counter: a static launch.
 * n <= 0 returns 0 and launches nothing.  noise == NULL or nranges == 0: no noise, weight decay only (a non-NULL noise still
 * advances).  NULL p / g / m / v / st with n > 0, ranges == NULL with nranges > 0 (and a noise state), nranges < 0 or > 512:
 * -1 before anything is launched.  Kernel: one thread per quad per trip of a grid-stride loop (one Philox block serves four
 * elements), 16-byte loads and stores when all four pointers are 16-byte aligned and the quad is whole, element by element
 * otherwise; the table is staged into LDS once per block, binary search per quad.  Grouped instantiation: DIP_FAM_LOSS. */
typedef struct DipSgldState {
    uint64_t offset;      /* Philox quad of element 0 of the next launch */
    uint64_t seed;
    float std;            /* standard deviation of the noise added to a noised element */
    float pad_;
} DipSgldState;           /* 24 bytes, device memory */
int dip_adam_sgld_step_dev(float* p, const float* g, float* m, float* v, int64_t n, double beta1, double beta2, double eps,
                           double weight_decay, const DipIterState* st, DipSgldState* noise, const int64_t* ranges,
                           int nranges, void* stream);
/* The same with host scalars (the relation dip_adam_step has to dip_adam_step_dev): nothing is advanced. */
int dip_adam_sgld_step(float* p, const float* g, float* m, float* v, int64_t n, double lr, double beta1, double beta2,
                       double eps, double weight_decay, int step, float std, uint64_t seed, uint64_t offset,
                       const int64_t* ranges, int nranges, void* stream);

/* ---------------------------------------------------------------- fused loss head ------------ */
/* The tail of the closure in two launches: output conv (1x1, Cout <= 4, weights straight from the
 * OIHW parameter arena) + nn.Sigmoid (models/skip.py:96-98) + optional mask + torch.nn.MSELoss
 * (denoising.ipynb:177,219: mse(out, img_noisy); inpainting.ipynb:310: mse(out * mask, img * mask),
 * the mean runs over ALL Cout*HW elements in both cases).
 *   forward : out[o][p] = sigmoid(sum_c w[o][c] * tr(u[p][c]) + bias[o])            (NCHW)
 *             *loss = 1/(Cout*HW) * sum (out*m - target*m)^2
 *             one lane per pixel (conv on the 4x4x1 MFMA), LDS tree per block, one partial per block,
 *             then a one-block fp64 sum of the partials in a fixed order (second launch inside the
 *             call): deterministic, no float atomics.
 *   backward: dy[p][o] = *gscale * 2/(Cout*HW) * (out*m - target*m) * m * out*(1-out)  (NHWC, stride Cy)
 *             = grad wrt the output conv's result, consumed by dip_conv_wgrad / dip_conv_igemm. */
typedef struct DipLossHeadDesc {
    const float* u;       /* [HW][Cu] input activation of the output conv (raw conv output of the producer) */
    int Cu, Cin;
    DipTransform tr;      /* the producer's BatchNorm + LeakyReLU */
    const float* w;       /* [Cout][Cin] 1x1 weights (OIHW) */
    const float* bias;    /* [Cout] or NULL */
    int Cout, HW, sigmoid;
    const float* target;  /* [Cout][HW] NCHW */
    const float* mask;    /* [mask_c][HW] NCHW or NULL; mask_c in {1, Cout} */
    int mask_c;
    float* out;           /* [Cout][HW] NCHW: the network output */
    float* partials;      /* nblk floats */
    int nblk;             /* dip_loss_head_nblk(HW, Cin) */
    float* loss;          /* 1 float */
} DipLossHeadDesc;
int dip_loss_head_nblk(int HW, int Cin);
int dip_loss_head_fwd(const DipLossHeadDesc* d, void* stream);
int dip_loss_head_bwd(const DipLossHeadDesc* d, const float* gscale, float* dy, int Cy, void* stream);

/* ---------------------------------------------------------------- fused super-resolution tail ---- */
/* The tail of the super-resolution closure (super-resolution.ipynb:169-186: out_LR = downsampler(out_HR);
 * total_loss = mse(out_LR, img_LR_var)) behind dip_head_fwd, in two launches: the fixed-taps Downsampler
 * (models/downsampler.py:65-71: ReplicationPad2d(pad) + depth-wise k x k stride-f correlation) + torch.nn.MSELoss.
 *   forward : y[c][oy][ox] = the fmaf chain of dip_lanczos_down_fwd (taps row-major, source index clamped, from 0.f), so y is
 *             bit-identical to dip_lanczos_down_fwd(out);  r = y - target;  one fp32 partial of sum r^2 per block, then the
 *             fixed-order fp64 sum of dip_loss_head_fwd with scale 1/(C*Ho*Wo) in a launch of its own: no float atomics.
 *   backward: v = ((y - target) * kk) * gs with kk = 2.f / ((float)C * (float)(Ho*Wo)), gs = gscale ? *gscale : 1.f;
 *             g = the fmaf chain of dip_lanczos_down_bwd over v;  dy[p][c] = sigmoid ? g * ((1.f - out) * out) : g
 *             (NHWC, channel stride Cy, pad channels zero, as dip_head_bwd): bit-identical to that chain of three.
 * The descriptor is read when the call launches (`loss` may be rewritten by the host between calls).  Refused with -1 before
 * any launch: a NULL descriptor or field, C, k, f < 1, Ho / Wo != (H + 2 pad - k) / f + 1, nblk != dip_sr_loss_nblk(C, Ho, Wo),
 * Cy < C or Cy % 4 != 0.  Inside dip_group_begin / dip_group_end both calls (and dip_head_fwd in front of them) serve every
 * instance with ONE dispatch per kernel: all six pointer fields, gscale and dy must lie in instance 0's slab -- the taps too,
 * so the instances of a group may carry different taps of the same (k, f, pad).  sizeof(DipSRLossDesc) == 96 (LP64). */
typedef struct DipSRLossDesc {
    const float* out;      /* [C][H*W] NCHW: the network output (input here) */
    const float* taps;     /* [k*k] */
    const float* target;   /* [C][Ho*Wo] */
    float* y;              /* [C][Ho*Wo]: the LR output, written by the forward, read by the backward */
    float* partials;       /* nblk floats */
    int nblk;              /* dip_sr_loss_nblk(C, Ho, Wo) */
    float* loss;           /* 1 float */
    int C, H, W, k, f, pad, Ho, Wo, sigmoid;
} DipSRLossDesc;
int dip_sr_loss_nblk(int C, int Ho, int Wo);
int dip_sr_loss_fwd(const DipSRLossDesc* d, void* stream);
int dip_sr_loss_bwd(const DipSRLossDesc* d, const float* gscale, float* dy, int Cy, void* stream);

/* ... with the TV term of the closure (super-resolution.ipynb:180-181, sr_prior_effect.ipynb:109):
 *   total_loss = mse(out_LR, img_LR_var) + tv_weight * tv_loss(out_HR, beta)
 * tv_loss (utils/sr_utils.py:84-94 of the reference) has, per channel, one term per pixel with y < H-1 and x < W-1:
 *   dhd = out[y][x+1] - out[y][x];  dwd = out[y+1][x] - out[y][x];  s = fmaf(dhd, dhd, dwd * dwd);  term = s^beta
 * s^beta is sqrtf(s), s, s * s for beta 0.5, 1, 2 (the exact forms ATen's pow has) and powf(s, beta) otherwise.
 *   forward : y and the MSE partials come from the kernel dip_sr_loss_fwd launches (y stays bit-identical to
 *             dip_lanczos_down_fwd(out)); one more kernel streams over out (one channel's 16 rows x 64 columns per block: a
 *             chain of fp32 adds in row order per lane, an LDS tree per block, one fp32 partial per block, no float atomics);
 *             one reduce launch sums both partial ranges in fixed order in fp64 and writes
 *             *loss = (float)(sum_mse / (C*Ho*Wo) + (double)*tv_weight * sum_tv).   H == 1 or W == 1: sum_tv = 0.
 *   backward: ONE kernel: acc = the gather of dip_sr_loss_bwd (same fmaf chain), plus the TV gradient of the same pixel.  With
 *             g(s) = beta * s^(beta-1) (0.5f / sqrtf(s), 1.f, 2.f * s for beta 0.5, 1, 2; beta * powf(s, beta - 1.f) otherwise),
 *             a = g(s) * dhd, b = g(s) * dwd of the term at a pixel -- both 0.f where the term does not exist (the last row, the
 *             last column) -- the evaluation order, every operation rounded on its own (no contraction), is
 *               t    = ((-(a[p] + b[p])) + a[left of p]) + b[above p]
 *               coef = (2.f * *tv_weight) * gs                         (gs = gscale ? *gscale : 1.f)
 *               g    = acc + coef * t;      dy[p][c] = sigmoid ? g * ((1.f - out) * out) : g
 *             the same order whether a and b are staged in LDS (17 x 17 per channel per 16 x 16 tile) or formed where they are
 *             read (a filter whose staged form would pass the 48 KB LDS budget), solo or grouped.
 * There is NO epsilon and no guard at s == 0, as in the reference: for beta < 1 g(0) = +inf and a = inf * 0 = NaN, which is what
 * autograd over the spelled closure yields at a pixel whose right and lower neighbours equal it; beta >= 1 stays finite.
 * tv_weight is ONE float in device memory: the instances of a group may differ in it and it may be rewritten between calls
 * without re-planning.  Refused with -1 before any launch: everything dip_sr_loss_fwd / _bwd refuse (on `sr`), NULL tv_weight
 * or tv_partials, tv_nblk != dip_sr_tv_nblk(C, H, W), beta <= 0 or not finite.  Inside dip_group_begin / dip_group_end:
 * as DipSRLossDesc, with tv_weight and tv_partials in instance 0's slab too.  sizeof(DipSRTVDesc) == 120 (LP64). */
typedef struct DipSRTVDesc {
    DipSRLossDesc sr;        /* everything dip_sr_loss_fwd / _bwd read and write */
    const float* tv_weight;  /* 1 float, device memory */
    float* tv_partials;      /* tv_nblk floats */
    int tv_nblk;             /* dip_sr_tv_nblk(C, H, W) */
    float beta;              /* > 0; the notebooks' 0.5 */
} DipSRTVDesc;
int dip_sr_tv_nblk(int C, int H, int W);
int dip_sr_tv_loss_fwd(const DipSRTVDesc* d, void* stream);
int dip_sr_tv_loss_bwd(const DipSRTVDesc* d, const float* gscale, float* dy, int Cy, void* stream);

/* ---------------------------------------------------------------- closure bookkeeping ---- */
/* The per-iteration bookkeeping of the notebooks' closures without host round trips
 * (denoising.ipynb:214-248): EMA of the output, PSNR against the noisy / clean image, and the
 * "fall back to the last checkpoint if psrn_noisy dropped by more than 5 dB" rule.
 *   out_avg <- first ? out : out_avg*exp_weight + out*(1-exp_weight)
 *   record  <- {loss, mse_noisy, mse_gt, mse_gt_sm, psnr_noisy, psnr_gt, psnr_gt_sm, fell_back}
 *              (psnr = -10 log10(mse), data range 1; the gt entries are 0 when gt == NULL;
 *               `loss` is a device scalar or NULL)
 *   state   =  {psnr_noisy_last, restore, have_last, snapshot}; zero it before the first call.
 *              With check_backtrack != 0 (the notebook's `if i % show_every:`): restore = 1 when
 *              psnr_noisy - psnr_noisy_last < -backtrack_db, otherwise snapshot = 1 and
 *              psnr_noisy_last <- psnr_noisy.
 * `partial` is scratch of 4*dip_fit_monitor_nblk(n) floats.  All tensors NCHW / flat, n elements. */
int dip_fit_monitor_nblk(int64_t n);
int dip_fit_monitor(const float* out, const float* noisy, const float* gt, float* out_avg, int64_t n,
                    float exp_weight, int first, const float* loss, float* partial, float* record,
                    float* state, int check_backtrack, float backtrack_db, void* stream);
/* dip_fit_monitor with the iteration index in DEVICE memory: the same bookkeeping of the reference closure
 * (denoising.ipynb:214-248; restoration.ipynb:192-211 is dip_restore_monitor / dip_restore_monitor_dev below) in a form whose
 * launch arguments do not change from one iteration to the next, so it can be a command of dip_iter_run's lists (a descriptor
 * pointer plus the stream, like dip_loss_head_fwd).  With i = counter[0]:
 *   first           = (i == 0)                                 (:214 `if out_avg is None`)
 *   check_backtrack = backtracking && (i % show_every != 0)    (:238 `if i % show_every:`)
 *   record          = records + 8*i
 * and, after the record and `state` are written exactly as dip_fit_monitor writes them, counter[0] <- i + 1.
 * i outside [0, capacity): records, out_avg and counter are left alone and state[1] = state[3] = 0, so the
 * dip_arena_backtrack behind it does nothing (a guard against out-of-bounds writes; callers check the capacity first).
 * The descriptor is read when the call launches: `loss` (this iteration's loss scalar, or NULL) may be rewritten by the
 * host between calls.  gt may be NULL; every other pointer is required; n, capacity, show_every > 0, otherwise -1 before
 * anything is launched.  sizeof(DipFitMonitorDesc) == 104 (LP64).
 * Inside dip_group_begin / dip_group_end the call serves the B monitors of the group: every non-NULL pointer of the
 * descriptor (out, noisy, gt, out_avg, loss, partial, records, counter, state) must lie in instance 0's slab, and instance
 * b works on the same fields advanced by b * stride -- its own counter (so the instances may stand at different iterations;
 * the overflow guard is per instance), its own record row, out_avg, state and decision.  Two dispatches for all B (family
 * DIP_FAM_LOSS), or 2 B when that family runs as a host loop. */
typedef struct DipFitMonitorDesc {
    const float* out;       /* [n] the network output of this iteration */
    const float* noisy;     /* [n] */
    const float* gt;        /* [n] or NULL */
    float* out_avg;         /* [n] */
    int64_t n;
    float exp_weight, backtrack_db;
    const float* loss;      /* 1 float or NULL: column 0 of the record */
    float* partial;         /* 4*dip_fit_monitor_nblk(n) floats of scratch */
    float* records;         /* [capacity][8] */
    int capacity, show_every;
    int backtracking;       /* 0 / 1 */
    int reserved;
    int* counter;           /* int32[1]: the iteration index, advanced by the call */
    float* state;           /* float[4], as for dip_fit_monitor */
} DipFitMonitorDesc;
int dip_fit_monitor_dev(const DipFitMonitorDesc* d, void* stream);
/* applies the decision in `state` to the flat parameter arena: restore -> params = snapshot,
 * snapshot -> snapshot = params, neither -> nothing (the notebook's net_param.data.copy_(...) /
 * last_net = [x.detach().cpu() ...], :242-247).  Inside dip_group_begin / dip_group_end: params, snapshot and state lie
 * in instance 0's slab and instance b applies ITS state to ITS params / snapshot (advanced by b * stride), so in one
 * dispatch some instances restore, some snapshot and some do nothing. */
int dip_arena_backtrack(float* params, float* snapshot, int64_t n, const float* state, void* stream);

/* The bookkeeping of the super-resolution closure (super-resolution.ipynb:169-191, sr_prior_effect.ipynb cell 6) without
 * host round trips: after backward() the notebook does, in every iteration,
 *   psnr_LR = compare_psnr(imgs['LR_np'], torch_to_np(out_LR));  psnr_HR = compare_psnr(imgs['HR_np'], torch_to_np(out_HR))
 *   psnr_history.append([psnr_LR, psnr_HR])
 * -- two device-to-host copies and two synchronisations.  Here one streaming pass leaves per-block fp32 partial sums of
 * (out_HR - img_HR)^2 (n_hr elements) and (out_LR - img_LR)^2 (n_lr elements) -- one grid, the HR blocks in front of the LR
 * blocks; per thread an fmaf chain over a grid-stride walk, per block a 256-wide LDS tree in a fixed pairing order -- and a
 * one-block kernel sums them in double, in block order, and writes the row
 *   record <- {loss, mse_LR, mse_HR, psnr_LR, psnr_HR}       (psnr = -10 log10(mse), data range 1; 5 floats per row)
 * Deterministic, no float atomics.  img_HR may be NULL (no ground truth: the HR blocks are not launched, mse_HR = psnr_HR = 0);
 * `loss` is a device scalar or NULL (0).  `partial` is scratch of dip_fit_monitor_nblk(n_hr) + dip_fit_monitor_nblk(n_lr)
 * floats.  There is no EMA and no back-tracking: the reference closure has neither.
 * dip_sr_monitor: `record` is the row, by value from the host (the eager closure's update()).
 * dip_sr_monitor_dev: the iteration index i = counter[0] lives in DEVICE memory, so the arguments do not change between
 * iterations and the call can be a command of dip_iter_run's lists; the row is records + 5*i and the last store is
 * counter[0] <- i + 1.  i outside [0, capacity): nothing is written (the guard of dip_fit_monitor_dev; callers check the
 * capacity first).  The descriptor is read when the call launches: `loss` may be rewritten by the host between calls.
 * img_HR and loss may be NULL; every other pointer is required; n_hr, n_lr, capacity > 0, otherwise -1 before anything is
 * launched.  sizeof(DipSRMonitorDesc) == 88 (LP64).
 * Inside dip_group_begin / dip_group_end both calls serve the B monitors of the group with two dispatches (family
 * DIP_FAM_LOSS; a workgroup belongs to one instance): every non-NULL pointer must lie in instance 0's slab, and instance b
 * works on the same fields advanced by b * stride -- its own counter, partial sums and record row. */
typedef struct DipSRMonitorDesc {
    const float* out_HR;    /* [n_hr] the network output of this iteration */
    const float* out_LR;    /* [n_lr] its down-sampled version (DipSRLossDesc.y) */
    const float* img_HR;    /* [n_hr] or NULL */
    const float* img_LR;    /* [n_lr] */
    int64_t n_hr, n_lr;
    const float* loss;      /* 1 float or NULL: column 0 of the record */
    float* partial;         /* dip_fit_monitor_nblk(n_hr) + dip_fit_monitor_nblk(n_lr) floats of scratch */
    float* records;         /* [capacity][5] */
    int capacity;
    int reserved;
    int* counter;           /* int32[1]: the iteration index, advanced by the call */
} DipSRMonitorDesc;
int dip_sr_monitor(const float* out_HR, const float* out_LR, const float* img_HR, const float* img_LR, int64_t n_hr,
                   int64_t n_lr, const float* loss, float* partial, float* record, void* stream);
int dip_sr_monitor_dev(const DipSRMonitorDesc* d, void* stream);

/* The bookkeeping of the restoration / inpainting closure (restoration.ipynb:180-219) without host round trips: after
 * backward() the notebook does, in every iteration,
 *   psrn_masked = compare_psnr(img_masked, out.detach().cpu().numpy()[0] * img_mask_np)            (restoration.ipynb:192)
 *   psrn        = compare_psnr(img_np,     out.detach().cpu().numpy()[0])                          (restoration.ipynb:193)
 * -- two device-to-host copies and two synchronisations -- and, when i % show_every == 0 (restoration.ipynb:198), falls back
 * to the last parameter checkpoint when psrn_masked dropped by more than 5 dB (restoration.ipynb:202-208) or else copies
 * every parameter to the CPU and remembers psrn_masked (restoration.ipynb:209-211).  Here one streaming pass over the NCHW
 * output (n elements, planes of hw) leaves per block the fp32 sums of ((out - img) * m)^2 and (out - img)^2, with
 * m = mask[mask_c == 1 ? i % hw : i] (img_masked = img * mask) -- per thread two fmaf chains over a grid-stride walk, per
 * block a 256-wide LDS tree in a fixed pairing order -- and a one-block kernel sums them in double, in block order:
 *   record <- {loss, mse_masked, mse, psnr_masked, psnr, fell_back}     (6 floats; mse = sum / n, psnr = -10 log10(mse), data
 *              range 1: compare_psnr over the whole array, as the notebook calls it; `loss` is a device scalar or NULL (0))
 *   state   =  {psnr_masked_last, restore, have_last, snapshot}: the float[4] of dip_fit_monitor, so dip_arena_backtrack
 *              applies the decision unchanged; zero it before the first call.  With check_backtrack != 0: restore = 1 when
 *              have_last is set and psnr_masked - psnr_masked_last < -backtrack_db, otherwise snapshot = 1,
 *              psnr_masked_last <- psnr_masked and have_last <- 1.  (The notebook starts psrn_masked_last at 0 and has no
 *              have_last; for images and outputs in [0, 1] psnr_masked >= 0, so the two rules decide identically.)
 * Deterministic, no float atomics, no EMA (this closure has none).  `partial` is scratch of 2*dip_fit_monitor_nblk(n) floats.
 * dip_restore_monitor: `record` is the row and check_backtrack the host's `i % show_every == 0`, by value (the eager
 * closure's update()).
 * dip_restore_monitor_dev: the iteration index i = counter[0] lives in DEVICE memory, so the arguments do not change between
 * iterations and the call can be a command of dip_iter_run's lists: check_backtrack = backtracking && (i % show_every == 0),
 * the row is records + 6*i, and the last store is counter[0] <- i + 1.  i outside [0, capacity): records and counter are left
 * alone and state[1] = state[3] = 0, so the dip_arena_backtrack behind it does nothing (the guard of dip_fit_monitor_dev;
 * callers check the capacity first).  The descriptor is read when the call launches: `loss` may be rewritten by the host
 * between calls.
 * loss may be NULL; every other pointer is required; n, hw, capacity, show_every > 0, n % hw == 0 and mask_c is 1 or n / hw,
 * otherwise -1 before anything is launched.  sizeof(DipRestoreMonitorDesc) == 104 (LP64).
 * Inside dip_group_begin / dip_group_end both calls serve the B monitors of the group with two dispatches (family
 * DIP_FAM_LOSS; a workgroup belongs to one instance): every non-NULL pointer must lie in instance 0's slab, and instance b
 * works on the same fields advanced by b * stride -- its own counter, partial sums, record row, state and decision. */
typedef struct DipRestoreMonitorDesc {
    const float* out;       /* [n] the network output of this iteration, NCHW */
    const float* img;       /* [n] the image the loss fits (restoration.ipynb: img_var) */
    const float* mask;      /* [mask_c][hw] */
    int64_t n, hw;
    int mask_c;             /* 1 or n / hw */
    float backtrack_db;
    const float* loss;      /* 1 float or NULL: column 0 of the record */
    float* partial;         /* 2*dip_fit_monitor_nblk(n) floats of scratch */
    float* records;         /* [capacity][6] */
    int capacity, show_every;
    int backtracking;       /* 0 / 1 */
    int reserved;
    int* counter;           /* int32[1]: the iteration index, advanced by the call */
    float* state;           /* float[4], as for dip_fit_monitor */
} DipRestoreMonitorDesc;
int dip_restore_monitor(const float* out, const float* img, const float* mask, int mask_c, int64_t n, int64_t hw,
                        const float* loss, float* partial, float* record, float* state, int check_backtrack,
                        float backtrack_db, void* stream);
int dip_restore_monitor_dev(const DipRestoreMonitorDesc* d, void* stream);

/* Ground-truth-free early stopping: the windowed moving variance of the net output (ES-WMV; Wang et al., "Early Stopping for
 * Deep Image Prior").  What it replaces is the host loop's per-iteration `out.detach().cpu()` -- one device-to-host copy of
 * the output and one synchronisation per iteration, then a variance over the last W outputs on the host; the reference itself
 * stops by a hand-picked num_iter (utils/common_utils.py:223-230 runs exactly num_iter iterations).
 * With outputs x_0, x_1, ... of n floats, window W >= 2 and patience P >= 1, for iteration t = counter[0], while not stopped:
 *   t <  W-1: x_t enters the window, no decision;
 *   t >= W-1: mu_t = mean of x_{t-W+1..t};  var_t = sum_w |x_{t-w} - mu_t|^2 / (W n);
 *             var_t < var_min (strict): var_min <- var_t, best_iter <- t, wait <- 0, best_out <- x_t, improved <- 1
 *             otherwise:                wait <- wait + 1;  wait >= P: stopped <- 1
 * Once stopped, ring, mean, M2, var_min, best_iter and best_out are frozen; later calls only write their record row (the
 * stopping iteration's row again) and advance the counter.  A NaN output makes var_t NaN: the comparison is false and wait
 * advances (no special case; the fp64 mean keeps the NaN, so the fit then stops after P iterations).
 *   record <- {var, var_min, best_iter, wait, stopped}     (5 floats per row; warm-up rows are {inf, inf, -1, 0, 0};
 *              best_iter is exact in fp32 up to 2^24)
 * Arithmetic: a ring [W][n] of fp32 outputs, a per-element fp64 mean and a scalar fp64 M2, updated in ONE streaming pass
 * (256 threads, grid-stride, dip_fit_monitor_nblk(n) blocks; 28 n bytes of traffic) --
 *   warm-up, k-th sample:   d = x_new - mu;  mu' = mu + d/k;  M2 += d (x_new - mu')                      (Welford)
 *   window full:            d = x_new - x_old;  mu' = mu + d/W;  M2 += d ((x_new - mu') + (x_old - mu))
 * -- with one fp64 partial per block from a 256-wide LDS tree in a fixed pairing order; a one-block kernel sums the partials
 * in a fixed order (64 lanes, each a contiguous run of blocks in block order, then the lane sums in lane order), takes the decision on the fp64 var = M2 / (W n), rounds it once to fp32 for the record and advances
 * counter[0]; a conditional copy then keeps out in best_out.  Deterministic, no float atomics, nothing synchronises.
 * state (64 bytes, 8-byte aligned), two views of one buffer:
 *   double[0] M2, double[1] var_min, double[2] the latest var;
 *   int32[6] ring head, [7] fill count, [8] wait, [9] best_iter, [10] stopped, [11] improved (this call found a new minimum).
 *   Before the first call: all zero except var_min = var = +inf and best_iter = -1.
 * t outside [0, capacity): nothing but improved <- 0 is written (the guard of dip_restore_monitor_dev; callers check the
 * capacity first).  `loss` is not part of the record and is not read; the field keeps the descriptor in the shape of the other
 * monitors' (dip_optim.NativeIteration rewrites it per iteration).  Every other pointer is required; n, window, patience,
 * capacity > 0 and window >= 2, otherwise -1 before anything is launched.  sizeof(DipEarlyStopDesc) == 96 (LP64).
 * The kernels have grouped instantiations (family DIP_FAM_LOSS: every non-NULL pointer in instance 0's slab, instance b works
 * on the same fields advanced by b * stride); dip_group.GroupedFits(early_stop=) issues them inside its group bracket.
 * dip_early_stop_keep: dst <- src (n floats, any n, any 4-byte alignment; whole quads only where both are 16-byte aligned)
 * when state's `improved` is set, else nothing: issued behind dip_early_stop_dev over the flat parameter arena, it keeps the
 * parameters that produced best_out. */
typedef struct DipEarlyStopDesc {
    const float* out;       /* [n] the network output of this iteration */
    float* ring;            /* [window][n] the last `window` outputs */
    double* mean;           /* [n] fp64 mean over the window */
    double* partial;        /* dip_fit_monitor_nblk(n) doubles of scratch */
    float* records;         /* [capacity][5] */
    void* state;            /* 64 bytes, see above */
    int* counter;           /* int32[1]: the iteration index, advanced by the call */
    float* best_out;        /* [n] the output at the minimum */
    int64_t n;
    int window, patience, capacity;
    const float* loss;      /* not read */
} DipEarlyStopDesc;
int dip_early_stop_dev(const DipEarlyStopDesc* d, void* stream);
int dip_early_stop_keep(const float* src, float* dst, int64_t n, const void* state, void* stream);

/* The ring-free form of the same criterion: the exponential moving variance of the output (ES-EMV, the same paper).  Per fit
 * only the fp64 mean [n] and one scalar v are carried -- no [window][n] ring -- so a group can afford it in every row.
 * Outputs x_0, x_1, ..., alpha in (0, 1), warmup >= 1, patience P >= 1, all arithmetic fp64:
 *   t = 0:                        mu <- x_0, v <- 0
 *   t >= 1, while not stopped:    d = x_t - mu;  mu <- mu + alpha d;  v <- (1 - alpha) (v + alpha sum(d^2) / n)
 *   t >= warmup, while not stopped: var_t = v and the decision of dip_early_stop_dev --
 *             var_t < var_min (strict): var_min <- var_t, best_iter <- t, wait <- 0, best_out <- x_t, improved <- 1
 *             otherwise:                wait <- wait + 1;  wait >= P: stopped <- 1
 *   record <- {var, var_min, best_iter, wait, stopped}; rows before `warmup` are {inf, inf, -1, 0, 0}, rows after the stopping
 *             iteration repeat its row.  Once stopped, mu, v, var_min, best_iter and best_out are frozen.
 * v starts at zero and ramps up for about 1 / alpha iterations: with warmup = 1 the second iteration is a false minimum
 * (utils.fit_monitor defaults to ceil(2 / alpha)).  A NaN output makes v NaN: no minimum is taken and wait advances.
 * ONE streaming pass (256 threads, grid-stride, dip_fit_monitor_nblk(n) blocks): one load of out, one load and one store of
 * the mean -- 20 n bytes of traffic against the 28 n of the windowed form -- one fp64 fma into the thread's partial of sum d^2,
 * the 256-wide LDS tree in the fixed pairing order, one fp64 partial per block; then the one-wave finalize in the fixed lane
 * order of dip_early_stop_dev and the same conditional copy into best_out.  Deterministic, no float atomics, nothing synchronises.
 * state: the 64-byte layout of dip_early_stop_dev with double[0] = v; the int words keep their meaning (fill: 0 before the
 * first output, 1 afterwards); `head` is unused.  t is counter[0]; t outside [0, capacity): nothing but improved <- 0 is written.
 * Every pointer is required; n, patience, capacity, warmup > 0, alpha in (0, 1), n <= 2^33, otherwise -1 before anything is
 * launched.  The loss is no part of the record, so the descriptor has no `loss` field (DipEarlyStopDesc carries one that is not
 * read).  sizeof(DipEarlyStopEmvDesc) == 88 (LP64).  Grouped instantiations: family DIP_FAM_LOSS.
 * dip_early_stop_keep keeps the parameter arena of the minimum, as behind dip_early_stop_dev. */
typedef struct DipEarlyStopEmvDesc {
    const float* out;       /* [n] the network output of this iteration */
    double* mean;           /* [n] fp64 exponential moving mean */
    double* partial;        /* dip_fit_monitor_nblk(n) doubles of scratch */
    float* records;         /* [capacity][5] */
    void* state;            /* 64 bytes, see above */
    int* counter;           /* int32[1]: the iteration index, advanced by the call */
    float* best_out;        /* [n] the output at the minimum */
    int64_t n;
    double alpha;
    int warmup, patience, capacity, reserved;
} DipEarlyStopEmvDesc;
int dip_early_stop_emv_dev(const DipEarlyStopEmvDesc* d, void* stream);

/* Sample mean and variance of the network outputs of an SGLD fit (Welford).  Iteration i = counter[0] is a sample iff
 * i >= burn_in and (i - burn_in) % every == 0.  Then, per element, with k = (float)(count + 1), every operation individually
 * rounded in fp32 and nothing contracted:
 *   d = x - mean;  mean' = mean + d / k;  m2' = m2 + d * (x - mean')
 * (mean and m2 start at zero; the first sample needs no special case: mean' == x and m2' == 0 exactly).  The sample variance is
 * m2 / (count - 1).  Two launches: the element pass (256 threads, grid-stride, dip_fit_monitor_nblk(n) blocks) only READS
 * counter and count; one thread behind it, ordered by the stream, does count += 1 (on a sample) and counter += 1.
 * Deterministic, no float atomics, nothing synchronises.  count >= 2^24 takes no more samples (k would no longer be exact;
 * the host refuses first).  Every pointer is required; n in (0, 2^33], burn_in >= 0, every >= 1, otherwise -1 before anything
 * is launched.  sizeof(DipPosteriorDesc) == 56 (LP64).  Grouped instantiations: family DIP_FAM_LOSS. */
typedef struct DipPosteriorDesc {
    const float* out;       /* [n] the network output of this iteration */
    float* mean;            /* [n] */
    float* m2;              /* [n] sum of squared deviations */
    int* count;             /* int32[1]: samples taken */
    int* counter;           /* int32[1]: the iteration index, advanced by the call */
    int64_t n;
    int burn_in, every;
} DipPosteriorDesc;
int dip_posterior_dev(const DipPosteriorDesc* d, void* stream);

/* dip_posterior_dev with the PSNR of the posterior mean against a ground truth (the curve of the SGLD paper).  mean and m2 are
 * dip_posterior_dev's, bit for bit: the same kernel body under a template flag.  On a sample iteration -- and only then -- the
 * element pass also forms, per block, the fp64 sum of (double(mean') - double(gt))^2 over the just-updated mean (threads in
 * grid-stride order, then a 256-wide LDS tree in a fixed pairing order), and the one thread behind it adds the
 * dip_fit_monitor_nblk(n) partials in block order and writes, BEFORE count advances, fp32 row number `count` of records:
 *   record <- {iteration (= counter[0], exact below 2^24), mse_mean = sum / n, psnr_mean = 10 log10(1 / mse_mean)}
 * (data range 1, as dip_fit_monitor's psnr_gt; 3 floats per row).  A row outside [0, capacity) is not written (the host refuses
 * first).  Deterministic, no float atomics, nothing synchronises.  Every pointer is required; n, burn_in, every as above,
 * capacity >= 1, otherwise -1 before anything is launched.  sizeof(DipPosteriorRecDesc) == 88 (LP64).  Grouped instantiations:
 * family DIP_FAM_LOSS. */
typedef struct DipPosteriorRecDesc {
    const float* out;       /* [n] the network output of this iteration */
    float* mean;            /* [n] */
    float* m2;              /* [n] sum of squared deviations */
    int* count;             /* int32[1]: samples taken = the next record row */
    int* counter;           /* int32[1]: the iteration index, advanced by the call */
    int64_t n;
    int burn_in, every;
    const float* gt;        /* [n] the ground truth */
    double* partial;        /* dip_fit_monitor_nblk(n) doubles of scratch */
    float* records;         /* [capacity][3] */
    int capacity, reserved;
} DipPosteriorRecDesc;
int dip_posterior_rec_dev(const DipPosteriorRecDesc* d, void* stream);

/* Pools C chains of one posterior -- rows of `mean` / `m2` at a fixed byte stride (the slab rows of a grouped fit), each holding
 * k samples -- into the pooled mean, the Gelman-Rubin variance estimate and R-hat (Gelman & Rubin 1992; BDA3 section 11.4).
 * Row c lies chains[c] * stride bytes behind mean0 / m20; `chains` is a device int32[nchains] list, walked in list order.  Per
 * element, every operation individually rounded in fp32 and nothing contracted (divisions and the square root correctly
 * rounded):
 *   s = 0;  for c: s = s + mean_c          mu = s / (float)C
 *   w = 0;  for c: w = w + m2_c            W  = w / (float)(C * (k - 1))
 *   q = 0;  for c: d = mean_c - mu; q = q + d * d        Bk = q / (float)(C - 1)
 *   f = (float)(k - 1) / (float)k          V  = f * W + Bk          (two roundings)
 *   R = sqrt(V / W)
 * mean <- mu, within <- W, var <- V, rhat <- R (rhat may be NULL: no map).  An element with !(W > 0) is degenerate: its R is
 * NaN and it is left out of the summary.  summary (fp64[3]) <- {mean of R over the other elements, their max, the number of
 * degenerate elements}; NaN, NaN, n when every element is degenerate.  The summary comes from per-block fp64 partials (a 256-wide
 * LDS tree in a fixed pairing order) added by one thread in block order: deterministic, no float atomics.  `partial` is scratch
 * of 3 * dip_fit_monitor_nblk(n) doubles.  256 threads, grid-stride over dip_fit_monitor_nblk(n) blocks; 16-byte accesses when
 * mean0, m20, stride and the outputs are all 16-byte aligned, 4-byte accesses otherwise (4-byte alignment is required).  The
 * caller vouches for the chain indices (rows that exist).  One launch pair outside a group bracket: with a bracket open, NULL
 * pointers, n outside (0, 2^33], k outside [2, 2^24] or nchains < 2 it returns -1 before anything is launched. */
int dip_posterior_pool(const float* mean0, const float* m20, long long stride, const int* chains, int nchains, int k, int64_t n,
                       float* mean, float* var, float* within, float* rhat, double* partial, double* summary, void* stream);

/* Mean structural similarity (SSIM; Wang, Bovik, Sheikh, Simoncelli 2004) of the network output -- and, optionally, of its
 * moving average -- against a ground truth.  What it replaces is a host filter behind an `out.detach().cpu()` per iteration;
 * the reference computes no SSIM.  Per channel of [C][H][W] images x (out, or avg) and y (gt):
 *   window       Gaussian 11 x 11, separable, g[k] = exp(-(k - 5)^2 / (2 * 1.5^2)) normalised to sum 1 in fp64, then rounded
 *                to fp32;
 *   moments      mu_x, mu_y, E[xx], E[yy], E[xy] by that filter over VALID positions only, (H - 10) x (W - 10) per channel
 *                (no padding: what cropping a 5-pixel border after filtering amounts to);
 *   covariances  biased: s_xx = E[xx] - mu_x^2, s_yy, s_xy alike;
 *   map          S = ((2 mu_x mu_y + c1)(2 s_xy + c2)) / ((mu_x^2 + mu_y^2 + c1)(s_xx + s_yy + c2)), with
 *                c1 = (0.01 data_range)^2 and c2 = (0.03 data_range)^2 from the caller;
 *   ssim         the mean of S over all channels and valid positions.
 * Arithmetic (fp32): the moments are formed about `pivot` (data_range / 2): a = x - pivot, b = y - pivot and the products
 * a a, b b, a b, each rounded once, go through the horizontal and then the vertical 11-tap chain h <- fma(g[k], v[k], h) in tap
 * order from zero; s_xx = E[aa] - mu_a mu_a (variances do not see the shift, and most of the cancellation of E[xx] - mu_x^2
 * is gone), mu_x = mu_a + pivot.  The four factors are formed from individually rounded operations, never contracted:
 *   n1 = 2 (mu_x mu_y) + c1;  n2 = 2 s_xy + c2;  d1 = (mu_x mu_x + mu_y mu_y) + c1;  d2 = (s_xx + s_yy) + c2;
 *   S = (n1 n2) / (d1 d2), a correctly rounded division.
 * With x == y bit for bit, n1 == d1 and n2 == d2 bit for bit: every S is exactly 1.0f, and so is the mean.
 * One workgroup owns a tile of 16 x 64 valid outputs of one channel and leaves ONE fp32 partial: every thread adds its four S
 * in row order, then a 256-wide LDS tree in a fixed pairing order (invalid positions contribute 0).  A one-block kernel adds
 * the dip_ssim_nblk(C, H, W) partials of a source in fp64 in a fixed order (64 lanes, lane t the partials t, t + 64, ...,
 * then the lane sums in lane order), divides by C (H-10) (W-10) and rounds once to fp32.  Deterministic: no float atomics, no
 * last-block ticket, nothing synchronises.
 *   record <- {ssim, ssim_sm}    (2 floats per row; ssim_sm is the SSIM of `avg` against gt, 0 when avg is NULL)
 * counter != NULL: the iteration index i = counter[0] lives in DEVICE memory, the row is records + 2*i and the last store is
 * counter[0] <- i + 1; i outside [0, capacity) writes nothing at all -- map, partial, records and counter are left alone
 * (callers check the capacity first).  counter == NULL is the functional form: row 0, nothing advanced, capacity not read.
 * `map` (NULL: not stored) receives S of `out`, [C][H-10][W-10].  `partial` is scratch of nblk floats, 2*nblk with avg.
 * out, gt, partial and records are required; C >= 1, H >= 11, W >= 11, nblk == dip_ssim_nblk(C, H, W) (which is -1 for
 * sizes it refuses), capacity > 0 with a counter; otherwise -1 before anything is launched.  sizeof(DipSsimDesc) == 88 (LP64).
 * Grouped instantiations: family DIP_FAM_LOSS (every non-NULL pointer in instance 0's slab, instance b works on the same
 * fields advanced by b * stride). */
typedef struct DipSsimDesc {
    const float* out;       /* [C][H][W] the network output of this iteration */
    const float* avg;       /* [C][H][W] a second source (the smoothed output) or NULL */
    const float* gt;        /* [C][H][W] the ground truth */
    float* map;             /* [C][H-10][W-10] S of `out`, or NULL */
    float* partial;         /* nblk floats of scratch (2*nblk with avg) */
    float* records;         /* [capacity][2] */
    int* counter;           /* int32[1]: the iteration index, advanced by the call; NULL: row 0, nothing advanced */
    int capacity;
    int C, H, W;
    float c1, c2, pivot;
    int nblk;               /* dip_ssim_nblk(C, H, W) */
} DipSsimDesc;
int dip_ssim_nblk(int C, int H, int W);
int dip_ssim_dev(const DipSsimDesc* d, void* stream);

/* ---------------------------------------------------------------- Lanczos down-sampler ---- */
/* Downsampler.forward (models/downsampler.py:65-71): ReplicationPad2d(pad) + depth-wise
 * k x k stride-`factor` correlation with the fixed taps; NCHW [C][H][W] -> [C][H/f][W/f]. */
int dip_lanczos_down_fwd(const float* x, const float* taps, float* y, int C, int H, int W, int k,
                         int factor, int pad, void* stream);
int dip_lanczos_down_bwd(const float* gy, const float* taps, float* gx, int C, int H, int W, int k,
                         int factor, int pad, void* stream);
/* The same module with its dense weight being optimised -- get_params('down', ...), utils/common_utils.py:44-46:
 * ReplicationPad2d(pad) + Conv2d(C, C, k, stride=factor) with weight w [C][C][k][k] (OIHW) and bias [C] (may be NULL),
 * models/downsampler.py:88-101; NCHW.  _bwd_data: autograd's gradient wrt the input, _bwd_weight: wrt weight (dw, same
 * layout as w) and bias (db, may be NULL); x is the UNPADDED input of the forward. */
int dip_down_dense_fwd(const float* x, const float* w, const float* bias, float* y, int C, int H, int W, int k,
                       int factor, int pad, void* stream);
int dip_down_dense_bwd_data(const float* gy, const float* w, float* gx, int C, int H, int W, int k, int factor,
                            int pad, void* stream);
int dip_down_dense_bwd_weight(const float* gy, const float* x, float* dw, float* db, int C, int H, int W, int k,
                              int factor, int pad, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DIP_HIP_H */
