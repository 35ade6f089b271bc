"""Input-noise regularisation of the closures on the device RNG of libdip_hip.so (no counterpart
file in the reference, which writes it inline):

    denoising.ipynb:198,208-209      noise = net_input.detach().clone()
                                     net_input = net_input_saved + (noise.normal_() * reg_noise_std)

    reg = RegNoise(net_input_saved, reg_noise_std, seed=0)
    def closure():
        net_input = reg()                 # net_input_saved + N(0,1) * reg_noise_std, ONE launch

Counter-based Philox4x32-10 + Box-Muller (dip_noise_axpy_dev); the stream position lives in device
memory and advances with every call, so the call is a static launch (hipGraph-replayable) and no
normal_() + mul + add temporaries are made.  RegNoise(..., device_std=True) keeps the level in device memory as well
(dip_noise_axpy_dev1s; reg.set_std(x) anneals it under a captured graph).  The stream is NOT torch's device generator stream (the
reference's device stream cannot be reproduced on a CPU oracle either, SURVEY.md section 8c "RNG").
"""
import torch

import dip_native as N


def check_level(x, who, what="reg_noise_std"):
    """The noise level as a float, or the ValueError that says what is wrong with it (non-numbers, NaN, inf, negatives)."""
    import math
    import numbers
    if isinstance(x, bool) or not isinstance(x, numbers.Real) or not math.isfinite(x) or x < 0:
        raise ValueError(f"dip-amd: {who}: {what} must be a finite number >= 0, got {x!r}")
    return float(x)


class RegNoise:
    """device_std=True: the level lives in device memory (one float next to the stream position) and the launch reads it there
    (dip_noise_axpy_dev1s): set_std(x) rewrites it in stream order, so a captured GraphedIteration and a NativeIteration plan
    follow an annealed level without a re-capture / re-plan.  The noise path is then taken at level 0 too (out = saved + 0 * N,
    the stream keeps advancing), so the level can go to 0 and back.  `std` is the host mirror."""

    def __init__(self, net_input_saved, reg_noise_std, seed=0, device_std=False):
        self.device_std = bool(device_std)
        if self.device_std:                      # (refused before anything needs a GPU)
            reg_noise_std = check_level(reg_noise_std, "RegNoise")
        if not net_input_saved.is_cuda:
            raise RuntimeError("dip-amd: RegNoise works on MI355X tensors only (no CPU fallback)")
        self.saved = net_input_saved.detach().contiguous().float()
        self.std = float(reg_noise_std)
        self.seed = int(seed)
        self.offset = torch.zeros(1, dtype=torch.int64, device=self.saved.device)
        self.out = torch.empty_like(self.saved)
        self.std_dev = torch.full((1,), self.std, dtype=torch.float32, device=self.saved.device) if self.device_std else None

    @property
    def noisy(self):
        """Whether __call__ / NativeIteration's prologue issue the noise launch (and feed `out`, not `saved`)."""
        return self.device_std or self.std > 0

    def set_std(self, std):
        """The level from the next call on: one 4-byte fill on the current stream, no synchronisation."""
        if not self.device_std:
            raise RuntimeError("dip-amd: RegNoise.set_std: this RegNoise holds its level as a launch argument; construct it with "
                               "device_std=True")
        self.std = check_level(std, "RegNoise.set_std")
        self.std_dev.fill_(self.std)

    def _launch(self, lib):
        """(fn, args without the stream, name) of the noise launch: what __call__ issues and NativeIteration's prologue holds."""
        if self.device_std:
            return (lib.dip_noise_axpy_dev1s, (self.saved.data_ptr(), self.out.data_ptr(), self.saved.numel(),
                                               self.std_dev.data_ptr(), self.seed, self.offset.data_ptr()), "noise_axpy_dev1s")
        return (lib.dip_noise_axpy_dev, (self.saved.data_ptr(), self.out.data_ptr(), self.saved.numel(), self.std, self.seed,
                                         self.offset.data_ptr()), "noise_axpy_dev")

    def _plan_key(self):
        """What NativeIteration's prologue was built from: the level's value, or -- in device memory -- the scalar's identity."""
        return (id(self.std_dev) if self.device_std else self.std, self.seed, id(self.saved), id(self.out), id(self.offset))

    def __call__(self):
        """Returns net_input_saved + N(0,1)*std in a buffer owned by this object (overwritten by the
        next call, like the reference's `noise` tensor)."""
        if not self.noisy:
            return self.saved
        dev = self.saved.device
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            fn, args, name = self._launch(N.lib())
            N.check(fn(*args, st), name)
        return self.out
