"""Post-training periodization (reference: diffsci/extra/punetg_converters.py): turn a trained zero-padded network into one
that is periodic along chosen spatial axes, by replacing its torch.nn.Conv2d / Conv3d containers with CircularConv2d /
CircularConv3d that hold the same values (state_dict keys gain '.conv') and pointing the network's walk at those axes.

Axis order is the tensor's: [B, C, H, W]: [0] = H, [1] = W;  [B, C, D, H, W]: [0] = D, [1] = H, [2] = W.  None = every axis.

Acts on PUNetG / PUNetGCond (fields and volumes), ADM and the public ADM blocks, and on plain torch modules made of
convolutions.  Magnitude-preserving containers are no torch.nn.Conv* (here as in the reference) and stay as they are.  The
networks whose walks have no periodic route are refused by name.  Everything is validated before anything is altered.

Differences from the reference.  A kernel that is not square / cubic raises ValueError (the reference asserts).  A plain
convolution with stride, dilation or groups other than 1 raises NotImplementedError: the reference would build the circular
layer, this package has no periodic kernel for it.  Converting a module again does not wrap the inner .conv of a layer that
is already circular a second time; it gives the layer (and the network) the new axes."""
import copy

import torch

from ..models.nets.commonlayers import CircularConv2d, CircularConv3d, PeriodicAxes, _CircularConv, normalize_circular_dims

_CONV = {torch.nn.Conv2d: (CircularConv2d, 2), torch.nn.Conv3d: (CircularConv3d, 3)}


def _no_periodic_route():
    from ..models.nets import autoencoderldm, convit, dit, vaenet
    return (autoencoderldm._Launcher, vaenet.VAENet, vaenet.PatchedConv, convit.ConVit, convit.ConVitBlock, dit.DiffusionTransformer)


def _conv_kind(m):
    """(circular class, dimension) of a plain torch convolution container, else None."""
    for cls, kind in _CONV.items():
        if isinstance(m, cls):
            return kind
    return None


def _sites(module):
    """(parent, child name, child) of every plain convolution container outside a circular layer, and the circular layers."""
    plain, circ = [], []

    def walk(parent):
        for name, child in parent.named_children():
            if isinstance(child, _CircularConv):
                circ.append(child)
            elif _conv_kind(child) is not None:
                plain.append((parent, name, child))
            else:
                walk(child)
    walk(module)
    return plain, circ


def _validate(module, circular_dims):
    """Every refusal, with nothing altered: networks without a periodic route, axes outside the layers' and the networks' range,
    kernels a circular layer cannot have."""
    refused = _no_periodic_route()
    for m in module.modules():
        if isinstance(m, refused):
            raise NotImplementedError(f"convert_conv_to_circular: {type(m).__name__} has no periodic route on the HIP path")
    plain, circ = _sites(module)
    for m in module.modules():
        if isinstance(m, PeriodicAxes):
            normalize_circular_dims(circular_dims, len(m.circular_axes))
    for layer in circ:
        normalize_circular_dims(circular_dims, layer.dim)
    for _, _, conv in plain:
        dim = _conv_kind(conv)[1]
        normalize_circular_dims(circular_dims, dim)
        k = conv.kernel_size
        if any(s != k[0] for s in k):
            raise ValueError(f"Non-{'cubic' if dim == 3 else 'square'} kernels not supported; got {tuple(k)}")
        if k[0] % 2 == 0:
            raise ValueError(f"CircularConv requires odd kernel size, got {k[0]}. This layer cannot be converted.")
        one = (1,) * dim
        if conv.stride != one or conv.dilation != one or conv.groups != 1:
            raise NotImplementedError(f"convert_conv_to_circular: {type(conv).__name__} with stride {conv.stride}, dilation "
                                      f"{conv.dilation}, groups {conv.groups} has no periodic HIP kernel")


def _detached_copy(module):
    """deepcopy without the captured plans (hipGraphs cannot be copied, and the copy must re-plan anyway)."""
    holders = [(m, m._plans.plans) for m in module.modules() if hasattr(getattr(m, "_plans", None), "plans")]
    for m, _ in holders:
        m._plans.plans = {}
    try:
        return copy.deepcopy(module)
    finally:
        for m, plans in holders:
            m._plans.plans = plans


def _drop_caches(m):
    """Captured plans of a sampler module, and whatever a network says are its caches (PeriodicAxes.drop_caches)."""
    if hasattr(getattr(m, "_plans", None), "clear"):
        m._plans.clear()
    if isinstance(m, PeriodicAxes):
        m.drop_caches()


def convert_conv_to_circular(module, circular_dims=None, inplace=False):
    """Replace every Conv2d / Conv3d of `module` by a CircularConv2d / CircularConv3d with the same weights and make the
    network(s) in it periodic along circular_dims.  inplace=False: a deep copy is converted and returned, the argument stays as
    it is.  Returns the converted module."""
    _validate(module, circular_dims)
    if not inplace:
        module = _detached_copy(module)
    plain, circ = _sites(module)
    with torch.no_grad():
        for parent, name, conv in plain:
            cls, _ = _conv_kind(conv)
            new = cls(conv.in_channels, conv.out_channels, conv.kernel_size[0], circular_dims, bias=conv.bias is not None)
            new.conv.to(device=conv.weight.device, dtype=conv.weight.dtype)
            new.conv.weight.copy_(conv.weight)
            if conv.bias is not None:
                new.conv.bias.copy_(conv.bias)
            new.train(conv.training)
            setattr(parent, name, new)
    for layer in circ:
        layer.circular_dims = normalize_circular_dims(circular_dims, layer.dim)
    for m in module.modules():
        # (a magnitude-preserving network has no circular layer: it stays zero-padded)
        if isinstance(m, PeriodicAxes) and any(isinstance(c, _CircularConv) for c in m.modules()):
            dims = normalize_circular_dims(circular_dims, len(m.circular_axes))
            m.circular_axes = tuple(d in dims for d in range(len(m.circular_axes)))
        _drop_caches(m)
    return module


def count_conv_layers(module):
    """{'Conv2d', 'Conv3d', 'CircularConv2d', 'CircularConv3d'} -> how many modules of each kind `module` holds.  As in the
    reference, the torch convolution inside a circular layer counts as a Conv2d / Conv3d of its own."""
    counts = dict.fromkeys(("Conv2d", "Conv3d", "CircularConv2d", "CircularConv3d"), 0)
    for m in module.modules():
        for cls in (CircularConv2d, CircularConv3d, torch.nn.Conv2d, torch.nn.Conv3d):
            if isinstance(m, cls):
                counts[cls.__name__] += 1
                break
    return counts
