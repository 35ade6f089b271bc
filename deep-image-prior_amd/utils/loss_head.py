"""Fused loss head for the notebooks' closures (no counterpart file in the reference, which spells
the same arithmetic out as separate PyTorch ops in every closure):

    denoising.ipynb:212,219      out = net(net_input);            total_loss = mse(out, img_noisy_torch)
    inpainting.ipynb:308-310     out = net(net_input);            total_loss = mse(out * mask_var, img_var * mask_var)

    head = MSEHead(net, img_noisy_torch)                      # or MSEHead(net, img_var, mask=mask_var)
    def closure():
        total_loss, out = head(net_input)                     # out: the network output, detached
        total_loss.backward()
        return total_loss

`head(net_input)` runs the skip-net up to the input of its last conv and then ONE launch
(dip_loss_head_fwd) for the 1x1 output conv + Sigmoid + mask + MSE, with the scalar reduced by an
LDS tree per block and a fixed-order fp64 sum of the per-block partials; `backward()` starts from
dip_loss_head_bwd.  The plain `out = net(x); mse(out, t)` spelling keeps working (the head,
the mask product and the MSE then run as separate kernels); this class is the opt-in fused path.

Super-resolution (super-resolution.ipynb:169-186 of the reference):

    out_HR = net(net_input); out_LR = downsampler(out_HR); total_loss = mse(out_LR, img_LR_var)

    head = SRHead(net, img_LR_var, downsampler)
    def closure():
        total_loss, out_HR = head(net_input)                  # head.out_LR: the down-sampled output, for psnr_LR
        total_loss.backward()
        return total_loss

`SRHead` runs the whole net (out_HR is bit-identical to net(net_input)) and then ONE launch for the Lanczos down-sampler +
MSE (dip_sr_loss_fwd); `backward()` starts from dip_sr_loss_bwd (MSE backward + the down-sampler's adjoint + the sigmoid
factor) instead of three autograd nodes.

With the TV prior (super-resolution.ipynb:180-181, sr_prior_effect.ipynb:109):

    total_loss = mse(out_LR, img_LR_var) + tv_weight * tv_loss(out_HR)

    head = SRHead(net, img_LR_var, downsampler, tv_weight=tv_weight)          # tv_beta=0.5 as utils.sr_utils.tv_loss

the same two calls become dip_sr_tv_loss_fwd (one more streaming kernel over out_HR; both sums reduced in one launch) and
dip_sr_tv_loss_bwd (ONE kernel: the gather above + the TV gradient of the same pixel).  No epsilon, as in the reference: for
tv_beta < 1 a pixel whose right and lower neighbours equal it gives NaN gradients in both spellings.

Both heads describe their launches ONCE, as the (fn, args, name) triples SkipEngine.forward / backward issue one by one and
dip_optim.NativeIteration compiles into its command arrays: `with_out_conv`, `_descriptor`, `fwd_launches`, `bwd_launches`.
The descriptors and the triples themselves are module-level functions (mse_* / sr_*), which dip_group.GroupedFits calls with
the buffers of its slab.
"""
import ctypes as C

import torch

import dip_native as N


# ---------------------------------------------------------------- the two tails, said once
# MSEHead / SRHead (one fit) and dip_group.GroupedFits (B fits through one launch list) fill the descriptors and list the
# launches HERE; they differ only in where the buffers live.
def mse_descriptor(eng, target_ptr, mask_ptr, mask_c, out_ptr, partials_ptr, nblk, loss_ptr):
    """(DipLossHeadDesc for the engine's current plan, the DipTransform it points into: the caller keeps that alive)."""
    a, oc = eng.last_act, eng.out_conv
    tr = a.transform()
    p = eng.params.data_ptr()
    return N.DipLossHeadDesc(a.buf.data_ptr(), a.Cs, oc.Cin, tr, p + 4 * oc.w_off, p + 4 * oc.b_off if oc.b_off >= 0 else None,
                             oc.Cout, eng.Hout * eng.Wout, 1 if eng.need_sigmoid else 0, target_ptr, mask_ptr, mask_c,
                             out_ptr, partials_ptr, nblk, loss_ptr), tr


def mse_fwd_launches(eng, desc):
    """The head's forward as (fn, args, name) triples; args without the trailing stream."""
    return [(eng.lib.dip_loss_head_fwd, (C.byref(desc),), "loss_head_fwd")]


def mse_bwd_launches(eng, desc, gscale_ptr):
    """What writes eng.dy_out (the gradient wrt the output conv's result) from d loss at gscale_ptr."""
    return [(eng.lib.dip_loss_head_bwd, (C.byref(desc), gscale_ptr, eng.dy_out.data_ptr(), N.round_up(eng.n_out, 4)),
             "loss_head_bwd")]


def sr_check_fixed_taps(d, who="SRHead"):
    """The fused tail applies the FIXED taps: a down-sampler that is (or may be) trained is refused."""
    if getattr(d, "_dense", False) or getattr(d, "_nondiag", False) or d.downsampler_.weight.requires_grad \
            or d.downsampler_.bias.requires_grad:
        raise NotImplementedError(f"dip-amd: {who} covers the fixed-taps Downsampler; a trainable one (opt_over='down', a "
                                  "loaded non-diagonal weight, or the down-sampler of a skip() net) goes through the "
                                  "spelled closure: out_LR = downsampler(net(x)); mse(out_LR, img_LR)")


def sr_support(d):
    """(k, factor, pad) of a Downsampler."""
    return int(d.kernel.shape[0]), int(d.factor), int(d._pad)


def sr_geometry(d, H, W, who="SRHead"):
    """(k, f, pad, Ho, Wo) of down-sampler d behind an H x W network output."""
    k, f, pad = sr_support(d)
    if H + 2 * pad < k or W + 2 * pad < k:
        raise ValueError(f"{who}: the net output {(H, W)} is smaller than the {k}x{k} filter")
    return k, f, pad, (H + 2 * pad - k) // f + 1, (W + 2 * pad - k) // f + 1


def sr_descriptor(eng, geom, out_ptr, taps_ptr, target_ptr, y_ptr, partials_ptr, nblk, loss_ptr):
    k, f, pad, Ho, Wo = geom
    return N.DipSRLossDesc(out_ptr, taps_ptr, target_ptr, y_ptr, partials_ptr, nblk, loss_ptr, eng.n_out, eng.Hout, eng.Wout,
                           k, f, pad, Ho, Wo, 1 if eng.need_sigmoid else 0)


def sr_check_tv(tv_weight, tv_beta, who="SRHead"):
    """(tv_weight, tv_beta) as floats; a negative or non-finite weight and tv_beta <= 0 (or non-finite) are refused."""
    import math
    try:
        w, beta = float(tv_weight), float(tv_beta)
    except (TypeError, ValueError):
        raise TypeError(f"dip-amd: {who}: tv_weight / tv_beta must be numbers, got {tv_weight!r} / {tv_beta!r}") from None
    if not math.isfinite(w) or w < 0:
        raise ValueError(f"dip-amd: {who}: tv_weight must be finite and >= 0, got {tv_weight!r}")
    if not math.isfinite(beta) or beta <= 0:
        raise ValueError(f"dip-amd: {who}: tv_beta must be finite and > 0, got {tv_beta!r}")
    return w, beta


def sr_tv_descriptor(sr_desc, tv_weight_ptr, tv_partials_ptr, tv_nblk, beta):
    """DipSRTVDesc: the DipSRLossDesc of the same fit + the TV term's device scalar, partials and beta."""
    return N.DipSRTVDesc(sr_desc, tv_weight_ptr, tv_partials_ptr, tv_nblk, beta)


def sr_fwd_launches(eng, desc):
    """dip_head_fwd (NHWC -> NCHW + sigmoid: out_HR as net(x) writes it) + dip_sr_loss_fwd, as (fn, args, name) triples; for
    a DipSRTVDesc dip_sr_tv_loss_fwd: total_loss = mse(out_LR, img_LR) + tv_weight * tv_loss(out_HR, beta)."""
    fn, name = (eng.lib.dip_sr_tv_loss_fwd, "sr_tv_loss_fwd") if isinstance(desc, N.DipSRTVDesc) else \
        (eng.lib.dip_sr_loss_fwd, "sr_loss_fwd")
    return [(eng.lib.dip_head_fwd, (eng.y_out.data_ptr(), desc.out, eng.n_out, eng.Hout * eng.Wout, N.round_up(eng.n_out, 4),
                                    1 if eng.need_sigmoid else 0), "head_fwd"),
            (fn, (C.byref(desc),), name)]


def sr_bwd_launches(eng, desc, gscale_ptr):
    fn, name = (eng.lib.dip_sr_tv_loss_bwd, "sr_tv_loss_bwd") if isinstance(desc, N.DipSRTVDesc) else \
        (eng.lib.dip_sr_loss_bwd, "sr_loss_bwd")
    return [(fn, (C.byref(desc), gscale_ptr, eng.dy_out.data_ptr(), N.round_up(eng.n_out, 4)), name)]


class MSEHead:
    kind = "mse"
    with_out_conv = False       # dip_loss_head_fwd runs the output conv itself: the forward list stops in front of it
    fwd_launches, bwd_launches = staticmethod(mse_fwd_launches), staticmethod(mse_bwd_launches)

    def __init__(self, net, target, mask=None):
        eng = getattr(net, "__dict__", {}).get("_dip_engine")
        if eng is None or isinstance(eng, Exception):
            raise RuntimeError("dip-amd: MSEHead needs a net built by models.skip.skip()")
        if not target.is_cuda:
            raise RuntimeError("dip-amd: MSEHead works on MI355X tensors only (no CPU fallback)")
        self.net, self.engine = net, eng
        oc = eng.out_conv
        if oc.ks != 1 or oc.Cout > 4:
            raise NotImplementedError("dip-amd: the fused loss head covers a 1x1 output conv with <= 4 channels "
                                      "(n_channels 1 or 3 in every reference notebook)")
        if target.dim() != 4 or target.shape[0] != 1 or target.shape[1] != oc.Cout:
            raise ValueError(f"MSEHead: target must be [1,{oc.Cout},H,W], got {tuple(target.shape)}")
        self.target = target.detach().contiguous().float()
        self.mask = None
        self.mask_c = 0
        if mask is not None:
            m = mask.detach().to(target.device).float()
            while m.dim() < 4:
                m = m[None]
            if m.shape[0] != 1 or m.shape[1] not in (1, oc.Cout) or m.shape[2:] != target.shape[2:]:
                raise ValueError(f"MSEHead: mask must be [1,1|{oc.Cout},H,W], got {tuple(m.shape)}")
            self.mask, self.mask_c = m.contiguous(), int(m.shape[1])
        self._scratch = None

    def _descriptor(self, eng, out, loss):
        """DipLossHeadDesc for the engine's current plan (called by SkipEngine.forward)."""
        H, W = eng.Hout, eng.Wout
        if tuple(self.target.shape[2:]) != (H, W):
            raise ValueError(f"MSEHead: target is {tuple(self.target.shape[2:])}, the net output is {(H, W)}")
        nblk = eng.lib.dip_loss_head_nblk(H * W, eng.out_conv.Cin)
        dev = out.device
        if self._scratch is None or self._scratch.numel() != nblk or self._scratch.device != dev:
            self._scratch = torch.empty(nblk, dtype=torch.float32, device=dev)
        desc, tr = mse_descriptor(eng, self.target.data_ptr(), None if self.mask is None else self.mask.data_ptr(), self.mask_c,
                                  out.data_ptr(), self._scratch.data_ptr(), nblk, loss.data_ptr())
        self._keep = (out.detach(), tr)     # (not `loss`: it becomes the autograd output and would pin the graph)
        return desc

    def _check_state(self):
        pass

    def _plan_key(self):
        """What a compiled command array (dip_optim.NativeIteration) was built from, objects by identity."""
        return (self.kind, id(self.target), self.target.data_ptr(), id(self.mask), self.mask_c)

    def _plan_keep(self):
        """The objects behind _plan_key and every buffer the descriptor points to: alive as long as the plan."""
        return (self.target, self.mask, self._keep, self._scratch)

    def __call__(self, net_input):
        import dip_engine
        if not self.net.training:
            raise NotImplementedError("dip-amd: eval-mode BatchNorm is not implemented")
        loss, out = dip_engine.run_net_loss(self.engine, self, net_input)
        return loss, out


class SRHead:
    """net + fixed-taps Downsampler + MSE (see the module docstring).  `target` (img_LR) may be replaced and the
    down-sampler's state reloaded between calls; `out_LR` is a buffer this object owns and overwrites.
    tv_weight > 0: total_loss = mse(out_LR, img_LR) + tv_weight * tv_loss(out_HR, tv_beta) (dip_sr_tv_loss_fwd / _bwd); the
    weight lives in a device scalar, rewritten by set_tv_weight() without a re-plan."""
    kind = "sr"
    with_out_conv = True        # the forward list runs to its end; dip_head_fwd writes out_HR as net(x) does
    fwd_launches, bwd_launches = staticmethod(sr_fwd_launches), staticmethod(sr_bwd_launches)

    def __init__(self, net, img_LR, downsampler, tv_weight=0.0, tv_beta=0.5):
        self.tv_weight, self.tv_beta = sr_check_tv(tv_weight, tv_beta)
        self._tv = self.tv_weight > 0
        self._tvw = None            # the device scalar; a new one when the weight is first needed on another device
        self._tv_scratch = None
        from models.downsampler import Downsampler
        eng = getattr(net, "__dict__", {}).get("_dip_engine")
        if eng is None or isinstance(eng, Exception):
            raise RuntimeError("dip-amd: SRHead needs a net built by models.skip.skip()")
        if eng.kind != "skip":
            raise NotImplementedError("dip-amd: SRHead covers skip() nets; the ResNet backbone has no fused loss head")
        if not isinstance(downsampler, Downsampler):
            raise TypeError(f"dip-amd: SRHead needs a models.downsampler.Downsampler, got {type(downsampler).__name__}")
        self.net, self.engine, self.downsampler = net, eng, downsampler
        self._check_state()
        n_out = eng.out_conv.Cout
        if downsampler.downsampler_.weight.shape[0] != n_out:
            raise ValueError(f"SRHead: the Downsampler has {downsampler.downsampler_.weight.shape[0]} planes, the net output "
                             f"has {n_out}")
        if not isinstance(img_LR, torch.Tensor) or img_LR.dim() != 4 or img_LR.shape[0] != 1 or img_LR.shape[1] != n_out:
            raise ValueError(f"SRHead: img_LR must be [1,{n_out},Ho,Wo], got {tuple(getattr(img_LR, 'shape', ()))}")
        if not img_LR.is_cuda:
            raise RuntimeError("dip-amd: SRHead works on MI355X tensors only (no CPU fallback)")
        self.target = img_LR.detach().contiguous().float()
        self._scratch = None
        self._y = None
        self._keep = None

    def _check_state(self):
        """The fused tail applies the FIXED taps: a down-sampler that is (or may be) trained is refused at every call."""
        sr_check_fixed_taps(self.downsampler)

    @property
    def out_LR(self):
        """downsampler(out_HR) of the last call, [1,C,Ho,Wo] (overwritten by the next one)."""
        return self._y

    def _geometry(self, eng):
        return sr_geometry(self.downsampler, eng.Hout, eng.Wout)

    def _descriptor(self, eng, out, loss):
        """DipSRLossDesc for the engine's current plan (called by SkipEngine.forward and NativeIteration)."""
        self._check_state()
        k, f, pad, Ho, Wo = self._geometry(eng)
        if tuple(self.target.shape[2:]) != (Ho, Wo):
            raise ValueError(f"SRHead: img_LR is {tuple(self.target.shape[2:])}, the down-sampled net output is {(Ho, Wo)}")
        dev = out.device
        taps = self.downsampler._taps
        if taps.device != dev or self.target.device != dev:
            raise RuntimeError(f"dip-amd: SRHead: the Downsampler is on {taps.device}, img_LR on {self.target.device}, the net "
                               f"runs on {dev}")
        Cn = eng.n_out
        nblk = eng.lib.dip_sr_loss_nblk(Cn, Ho, Wo)
        if self._scratch is None or self._scratch.numel() != nblk or self._scratch.device != dev:
            self._scratch = torch.empty(nblk, dtype=torch.float32, device=dev)
        if self._y is None or tuple(self._y.shape) != (1, Cn, Ho, Wo) or self._y.device != dev:
            self._y = torch.empty((1, Cn, Ho, Wo), dtype=torch.float32, device=dev)
        self._keep = (out.detach(), taps)
        sr = sr_descriptor(eng, (k, f, pad, Ho, Wo), out.data_ptr(), taps.data_ptr(), self.target.data_ptr(), self._y.data_ptr(),
                           self._scratch.data_ptr(), nblk, loss.data_ptr())
        if not self._tv:
            return sr
        tv_nblk = eng.lib.dip_sr_tv_nblk(Cn, eng.Hout, eng.Wout)
        if self._tv_scratch is None or self._tv_scratch.numel() != tv_nblk or self._tv_scratch.device != dev:
            self._tv_scratch = torch.empty(tv_nblk, dtype=torch.float32, device=dev)
        if self._tvw is None or self._tvw.device != dev:
            self._tvw = torch.full((1,), self.tv_weight, dtype=torch.float32, device=dev)
        return sr_tv_descriptor(sr, self._tvw.data_ptr(), self._tv_scratch.data_ptr(), tv_nblk, self.tv_beta)

    def set_tv_weight(self, w):
        """Another tv_weight > 0 for the calls that follow: the device scalar is rewritten in stream order, nothing is
        re-planned (a NativeIteration keeps its command arrays).  To or from 0 the launch list would change: build a new head."""
        w, _ = sr_check_tv(w, self.tv_beta)
        if (w > 0) != self._tv:
            raise ValueError(f"dip-amd: SRHead.set_tv_weight({w!r}) on a head built with tv_weight={self.tv_weight!r}: switching "
                             "the TV term on or off changes the launch list; construct a new SRHead")
        self.tv_weight = w
        if self._tvw is not None:
            self._tvw.fill_(w)

    def _plan_key(self):
        d = self.downsampler
        key = (self.kind, id(self.target), self.target.data_ptr(), id(d), id(d._taps), int(d.kernel.shape[0]), int(d.factor),
               int(d._pad), id(self._y))
        # (the weight's VALUE is not part of the key: it is read from the device scalar when the kernels run)
        return key + (("tv", self.tv_beta, id(self._tvw), id(self._tv_scratch)) if self._tv else ())

    def _plan_keep(self):
        return (self.target, self.downsampler, self._keep, self._scratch, self._y) + \
            ((self._tvw, self._tv_scratch) if self._tv else ())

    def __call__(self, net_input):
        import dip_engine
        if not self.net.training:
            raise NotImplementedError("dip-amd: eval-mode BatchNorm is not implemented")
        loss, out = dip_engine.run_net_loss(self.engine, self, net_input)
        return loss, out
