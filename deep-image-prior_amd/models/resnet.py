"""`ResNet` -- the plain residual chain at full resolution, API- and state_dict-compatible with the
reference's models/resnet.py:9-96, executed by hand-written gfx950 kernels.

The constructor assembles the SAME torch.nn module tree as the reference class (same child names,
same construction order -> same parameter RNG stream under torch.manual_seed, same state_dict keys
such as `model.0.1.weight`, `model.2.0.weight`, `model.2.1.running_mean`), but `forward()` hands the
tree to the HIP engine (dip_engine.ResNetEngine) instead of calling the children.  There is no
CPU / eager fallback.

What the tree really is (and the engine keeps):
  * the first and the last conv are built by `conv(..., pad=pad)`; the block convs and the conv in
    front of the last BatchNorm are nn.Conv2d(C, C, 3, 1, 1), i.e. ALWAYS zero-padded; the block
    convs have no bias;
  * the tree always ends in nn.Sigmoid(), whatever `need_sigmoid` says.
"""
import torch.nn as nn

from .common import act, conv
from .skip import _act_code_of_module_class


class ResidualSequential(nn.Sequential):
    """nn.Sequential whose output is added to its input.  A parameter holder on the MI355X path: the
    engine runs the children and the addition (dip_res_join_fwd); the module's own forward is the
    eager definition of the same thing."""

    def forward(self, x):
        out = super().forward(x)
        # the reference centre-crops x when the sizes differ; 3x3 convs with padding 1 never get there
        assert out.shape[2:] == x.shape[2:], "ResidualSequential: the block changed the spatial size"
        return out + x

    def eval(self):
        raise NotImplementedError("dip-amd: eval-mode BatchNorm is not implemented (the reference's "
                                  "ResidualSequential.eval() ends the process)")


def get_block(num_channels, norm_layer, act_fun):
    """conv -> norm -> act -> conv -> norm, the body of one residual block."""
    def conv3():
        return nn.Conv2d(num_channels, num_channels, 3, 1, 1, bias=False)

    first = [conv3(), norm_layer(num_channels, affine=True), act(act_fun)]
    return first + [conv3(), norm_layer(num_channels, affine=True)]


class ResNet(nn.Module):
    def __init__(self, num_input_channels, num_output_channels, num_blocks, num_channels, need_residual=True,
                 act_fun='LeakyReLU', need_sigmoid=True, norm_layer=nn.BatchNorm2d, pad='reflection'):
        """pad: 'reflection|zero' for the first and the last conv (the others are zero-padded)."""
        super().__init__()
        block_type = ResidualSequential if need_residual else nn.Sequential
        mods = [conv(num_input_channels, num_channels, 3, stride=1, bias=True, pad=pad), act(act_fun)]
        for _ in range(num_blocks):
            mods.append(block_type(*get_block(num_channels, norm_layer, act_fun)))
        mods.append(nn.Conv2d(num_channels, num_channels, 3, 1, 1))
        mods.append(norm_layer(num_channels, affine=True))
        mods.append(conv(num_channels, num_output_channels, 3, 1, bias=True, pad=pad))
        mods.append(nn.Sigmoid())           # appended unconditionally, as the reference does
        self.model = nn.Sequential(*mods)
        _attach_engine(self, num_blocks, bool(need_residual), pad, act_fun, norm_layer)

    def forward(self, input):
        eng = self.__dict__.get('_dip_engine')
        if eng is None:
            raise RuntimeError("dip-amd: this ResNet has no engine attached")
        if isinstance(eng, Exception):
            raise eng
        import dip_engine
        return dip_engine.run_net(eng, input)

    def eval(self):
        raise NotImplementedError("dip-amd: eval-mode BatchNorm is not implemented (ResNet.eval())")

    def __deepcopy__(self, memo):
        import copy
        cls = self.__class__
        new = cls.__new__(cls)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            if k in ('_dip_engine',):
                continue
            new.__dict__[k] = copy.deepcopy(v, memo)
        spec = self.__dict__.get('_dip_spec')
        if spec is not None:
            _attach_engine(new, *spec)
        return new


def _attach_engine(net, num_blocks, need_residual, pad, act_fun, norm_layer):
    """(Re)creates the HIP engine for `net` from its module tree (so deepcopy works).  An unsupported
    option is kept and raised at the first forward(): construction stays cheap."""
    import dip_engine
    net.__dict__['_dip_spec'] = (num_blocks, need_residual, pad, act_fun, norm_layer)
    act_codes = {'LeakyReLU': 0.2, 'none': 1.0, 'Swish': -1.0, 'ELU': -2.0}
    try:
        if norm_layer is not nn.BatchNorm2d:
            raise NotImplementedError(f"dip-amd: norm_layer={norm_layer!r} has no gfx950 path (nn.BatchNorm2d only)")
        if pad not in ('reflection', 'zero'):
            raise NotImplementedError(f"dip-amd: pad={pad!r} has no gfx950 path ('reflection' and 'zero' do)")
        if isinstance(act_fun, str):
            if act_fun not in act_codes:
                raise NotImplementedError(f"dip-amd: act_fun={act_fun!r} has no gfx950 kernel")
            act_code = act_codes[act_fun]
        else:
            act_code = _act_code_of_module_class(act_fun)
        seq = list(net.model._modules.values())

        def conv_of(block):
            return next(m for m in block._modules.values() if isinstance(m, nn.Conv2d))

        blocks = []
        for blk in seq[2:2 + num_blocks]:
            c1, b1, _, c2, b2 = blk._modules.values()
            blocks.append((c1, b1, c2, b2))
        tail_conv, tail_bn, out_block = seq[2 + num_blocks:5 + num_blocks]
        net.__dict__['_dip_engine'] = dip_engine.ResNetEngine(net, conv_of(seq[0]), blocks, tail_conv, tail_bn,
                                                              conv_of(out_block), need_residual, pad, act_slope=act_code)
    except NotImplementedError as e:
        net.__dict__['_dip_engine'] = e
