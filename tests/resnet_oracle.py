"""CPU truth of the ResNet backbone: the forward of models.resnet.ResNet restated in plain torch ops on a
state_dict, dtype-generic (fp64 = the truth, fp32 = the reference path's own roundoff), with the two test hooks
tests/parity.py relies on for skip nets (oracle/dip_oracle.py: _bn_act):

  masks  {key: bool [1,C,H,W]} imposes the LeakyReLU branch pattern another implementation realised,
  zrec   dict that receives the pre-activations (for parity.mask_report).

Mask / pre-activation keys: "model.0" for the activation behind the first conv (no BatchNorm in between), the
BatchNorm's state_dict prefix ("model.2.1", ...) for the one inside each block.

The op sequence is torch's own (F.pad, F.conv2d, F.batch_norm, F.leaky_relu, +, sigmoid) in the order the reference's
module tree calls them, so in fp32 and without masks the result is bitwise what the nn.Module tree computes.
"""
import torch
import torch.nn.functional as F


class ResNetSpec:
    def __init__(self, num_input_channels, num_output_channels, num_blocks, num_channels, need_residual=True,
                 act_fun="LeakyReLU", pad="reflection"):
        self.cin, self.cout, self.num_blocks, self.C = num_input_channels, num_output_channels, num_blocks, num_channels
        self.need_residual, self.act_fun, self.pad = need_residual, act_fun, pad
        # conv() puts a ReflectionPad2d in front of the Conv2d: the Conv2d is child "1" then, "0" otherwise
        self.cidx = "1" if pad == "reflection" else "0"

    @property
    def first(self):
        return f"model.0.{self.cidx}"

    def block(self, k):
        p = f"model.{2 + k}"
        return p + ".0", p + ".1", p + ".3", p + ".4"          # conv1, bn1, conv2, bn2

    @property
    def tail(self):
        return f"model.{2 + self.num_blocks}", f"model.{3 + self.num_blocks}"

    @property
    def out(self):
        return f"model.{4 + self.num_blocks}.{self.cidx}"

    def param_names(self):
        names = [self.first + ".weight", self.first + ".bias"]
        for k in range(self.num_blocks):
            c1, b1, c2, b2 = self.block(k)
            names += [c1 + ".weight", b1 + ".weight", b1 + ".bias", c2 + ".weight", b2 + ".weight", b2 + ".bias"]
        tc, tb = self.tail
        names += [tc + ".weight", tc + ".bias", tb + ".weight", tb + ".bias", self.out + ".weight", self.out + ".bias"]
        return names

    def zero_grad_keys(self):
        """The only analytically-zero gradient: the bias of the conv that feeds the last BatchNorm.  (The block convs have
        no bias; beta of the block BatchNorms and the first / last conv biases are NOT zero: zero padding behind them.)"""
        return {self.tail[0] + ".bias"}


def _act(x, act_fun, key, masks, zrec):
    if zrec is not None:
        zrec[key] = x.detach().float()
    if act_fun == "none":
        return x
    if act_fun is torch.nn.ReLU and masks is not None and key in masks:
        return x * masks[key].contiguous().to(x.dtype)          # the imposed branch pattern, as for LeakyReLU below
    if not isinstance(act_fun, str):
        return act_fun()(x)
    if act_fun == "Swish":
        return x * torch.sigmoid(x)
    if act_fun == "ELU":
        return F.elu(x)
    assert act_fun == "LeakyReLU", act_fun
    if masks is not None and key in masks:
        return x * (masks[key].contiguous().to(x.dtype) * 0.8 + 0.2)
    return F.leaky_relu(x, 0.2)


def _bn(x, sd, key, eps=1e-5):
    return F.batch_norm(x, None, None, sd[key + ".weight"], sd[key + ".bias"], True, 0.1, eps)


def _padded_conv(x, sd, key, pad):
    if pad == "reflection":
        return F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), sd[key + ".weight"], sd[key + ".bias"])
    return F.conv2d(x, sd[key + ".weight"], sd[key + ".bias"], padding=1)


def forward(spec: ResNetSpec, sd, x, masks=None, zrec=None):
    h = _act(_padded_conv(x, sd, spec.first, spec.pad), spec.act_fun, "model.0", masks, zrec)
    for k in range(spec.num_blocks):
        c1, b1, c2, b2 = spec.block(k)
        t = F.conv2d(h, sd[c1 + ".weight"], None, padding=1)
        t = _act(_bn(t, sd, b1), spec.act_fun, b1, masks, zrec)
        t = _bn(F.conv2d(t, sd[c2 + ".weight"], None, padding=1), sd, b2)
        h = t + h if spec.need_residual else t
    tc, tb = spec.tail
    h = _bn(F.conv2d(h, sd[tc + ".weight"], sd[tc + ".bias"], padding=1), sd, tb)
    return torch.sigmoid(_padded_conv(h, sd, spec.out, spec.pad))


def grads(spec: ResNetSpec, sd, z, loss_fn, dtype, masks=None, z_requires_grad=False, zrec=None):
    """(out, loss, {name: grad}) in `dtype` -- the counterpart of parity.oracle_grads; loss_fn(out, dtype) -> scalar."""
    names = spec.param_names()
    params = {k: sd[k].detach().to(dtype).clone().requires_grad_(True) for k in names}
    zz = z.to(dtype)
    if z_requires_grad:
        zz = zz.clone().requires_grad_(True)
    out = forward(spec, params, zz, masks, zrec)
    loss = loss_fn(out, dtype)
    loss.backward()
    g = {k: params[k].grad.detach() for k in names}
    if z_requires_grad:
        g["__input__"] = zz.grad.detach()
    return out.detach(), loss.item(), g


def hip_masks(net, spec: ResNetSpec):
    """LeakyReLU branch pattern the HIP forward realised, from the engine's raw conv outputs (as hipops.lrelu_masks does
    for skip nets): z = fma(a, y, b) > 0 per BatchNorm, y > 0 behind the first conv."""
    eng = net.__dict__["_dip_engine"]
    masks = {}

    def put(key, z, a):
        masks[key] = (z[:, :, :a.C] > 0).permute(2, 0, 1)[None].contiguous().cpu()

    R0 = eng.R0
    put("model.0", R0.buf.view(R0.H, R0.W, R0.Cs), R0)
    for k, b in enumerate(eng.blocks):
        A1 = b.st[1]
        state = A1.bn.state.view(4, A1.Cs)
        put(spec.block(k)[1], torch.addcmul(state[3], state[2], A1.buf.view(A1.H, A1.W, A1.Cs)), A1)
    return masks
