"""LDM AutoencoderKL decoder for 3-D volumes (reference: diffsci/models/nets/autoencoderldm3d.py): ``ddconfig``, ``ResnetBlock``,
``AttnBlock``, ``Upsample``, ``Decoder``, ``AutoencoderKL`` with the reference's constructors and state_dict keys, on the HIP
kernels.  The implementation is shared with the 2-D module: see autoencoderldm.py."""
from . import autoencoderldm as _impl


class ddconfig(object):
    """autoencoderldm3d.py: same arguments and defaults."""

    def __init__(self, double_z: bool = True, z_channels: int = 4, resolution: int = 64, in_channels: int = 1, out_ch: int = 1,
                 ch: int = 32, ch_mult: list = [1, 2, 4, 4], num_res_blocks: int = 2, attn_resolutions: list = [],
                 dropout: float = 0.0, has_mid_attn: bool = True):
        _impl.set_ddconfig(self, locals())


class ResnetBlock(_impl.ResnetBlock):
    __doc__ = _impl.ResnetBlock.__doc__
    _dim = 3


class AttnBlock(_impl.AttnBlock):
    __doc__ = _impl.AttnBlock.__doc__
    _dim = 3


class Upsample(_impl.Upsample):
    __doc__ = _impl.Upsample.__doc__
    _dim = 3


class Decoder(_impl.Decoder):
    __doc__ = _impl.Decoder.__doc__
    _dim = 3
    _ResnetBlock, _AttnBlock, _Upsample = ResnetBlock, AttnBlock, Upsample


class AutoencoderKL(_impl.AutoencoderKL):
    __doc__ = _impl.AutoencoderKL.__doc__
    _dim, _Decoder = 3, Decoder

    def __init__(self, ddconfig, lossconfig=None, distillconfig=None, embed_dim=4, ckpt_path=None, ignore_keys=[], image_key="image",
                 colorize_nlabels=None, monitor=None):
        super().__init__()
        self._setup(ddconfig, embed_dim, ckpt_path, ignore_keys, image_key, colorize_nlabels, monitor)
