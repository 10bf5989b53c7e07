"""CircularConv2d / CircularConv3d (commonlayers.py:918-1034): 'same' convolutions whose spatial axes are padded periodically or
with zeros, axis by axis.  Constructor, attributes and state_dict keys are the reference's (the weights live in .conv);
forward runs the fp16x3 HIP kernels through ops.  The networks use them as parameter containers and launch the kernels from
their own walks, with the axes taken from the net (circular_axes)."""
import torch

from ... import ops


def normalize_circular_dims(circular_dims, dim):
    """circular_dims of the reference (None = every axis, [] = zero padding everywhere, indices 0..dim-1 in tensor-axis order)
    as a set; an index outside the range is a ValueError (the reference would ignore it silently)."""
    if circular_dims is None:
        return set(range(dim))
    dims = set(int(d) for d in circular_dims)
    bad = sorted(d for d in dims if not 0 <= d < dim)
    if bad:
        raise ValueError(f"circular_dims {bad} outside 0..{dim - 1} ({'[0]=D, [1]=H, [2]=W' if dim == 3 else '[0]=H, [1]=W'})")
    return dims


class PeriodicAxes:
    """The one place a network (or a public block) keeps its periodic axes: `circular_axes`, one bool per spatial axis in
    tensor-axis order.  Everything else is read from it."""
    circular_axes = ()

    @property
    def circular(self):
        """Some axis wraps: the network takes the periodic routes (no pre-split images, no pooled epilogue, no exact input layer)."""
        return any(self.circular_axes)

    @property
    def circular_arg(self):
        """What the walk's launches pass as circular=: the axes, or False where none wraps."""
        return self.circular_axes if any(self.circular_axes) else False

    def drop_caches(self):
        """Forget packed weights, workspaces and whatever else was derived from the parameters or the axes: the next call packs
        and plans again.  Networks with caches of their own extend this."""
        for name in ("_packed", "_packed_sig"):
            if name in self.__dict__:
                setattr(self, name, None)


class _CircularConv(torch.nn.Module):
    dim = 2

    def __init__(self, in_channels, out_channels, kernel_size, circular_dims=None, *args, **kwargs):
        super().__init__()
        if not isinstance(kernel_size, int) or kernel_size % 2 != 1:
            raise ValueError(f"CircularConv requires odd kernel size, got {kernel_size}.")
        self.kernel_size = kernel_size
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.padding = kernel_size // 2
        self.circular_dims = normalize_circular_dims(circular_dims, self.dim)
        kwargs["padding"] = 0
        self.conv = (torch.nn.Conv3d if self.dim == 3 else torch.nn.Conv2d)(in_channels, out_channels, kernel_size, *args, **kwargs)
        one = (1,) * self.dim
        if self.conv.stride != one or self.conv.dilation != one or self.conv.groups != 1:
            raise NotImplementedError(f"{type(self).__name__}: stride, dilation and groups other than 1 have no HIP kernel")
        self._pack = None

    @property
    def weight(self):
        return self.conv.weight

    @property
    def bias(self):
        return self.conv.bias

    @property
    def axes(self):
        """One bool per spatial axis, tensor-axis order: what ops' circular= takes."""
        return tuple(d in self.circular_dims for d in range(self.dim))

    def forward(self, x):
        if self.kernel_size > 7:
            raise NotImplementedError(f"{type(self).__name__}.forward: kernel sizes up to 7; got {self.kernel_size}")
        w = self.conv.weight
        key = (w.data_ptr(), w._version, w.device)
        if self._pack is None or self._pack[0] != key:
            pack = ops.pack_conv3d(w.detach()) if self.dim == 3 else ops.pack_conv(w.detach(), "fp16x3")
            self._pack = (key, pack)
        bias = None if self.conv.bias is None else self.conv.bias.detach()
        if self.dim == 3:
            return ops.conv3d_mfma(x, self._pack[1], bias=bias, circular=self.axes)
        return ops.conv(x, self._pack[1], bias=bias, circular=self.axes)


class CircularConv2d(_CircularConv):
    """(in_channels, out_channels, kernel_size, circular_dims=None, *args, **kwargs); [B, C, H, W]: [0] = H, [1] = W."""
    dim = 2


class CircularConv3d(_CircularConv):
    """(in_channels, out_channels, kernel_size, circular_dims=None, *args, **kwargs); [B, C, D, H, W]: [0] = D, [1] = H, [2] = W."""
    dim = 3
