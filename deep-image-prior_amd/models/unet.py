"""`UNet` -- importable, not executable.

The reference's notebooks (inpainting, restoration) begin with `from models.unet import UNet`, so
the name has to exist for their import cell to run.  The backbone itself (ConvTranspose2d 4x4,
InstanceNorm2d, MaxPool2d chains; models/unet.py:32-128 of the reference) has no gfx950 path in this
backend and there is no eager fallback: constructing one raises.
"""
import torch.nn as nn


class UNet(nn.Module):
    def __init__(self, num_input_channels=3, num_output_channels=3, feature_scale=4, more_layers=0, concat_x=False,
                 upsample_mode='deconv', pad='zero', norm_layer=nn.InstanceNorm2d, need_sigmoid=True, need_bias=True):
        raise NotImplementedError("dip-amd: UNet is outside the MI355X-native path (ConvTranspose2d / InstanceNorm2d / "
                                  "MaxPool2d chains): no gfx950 path; use models.skip.skip() or models.resnet.ResNet")
