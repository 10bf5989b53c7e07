"""DiffusionPeriodizer on a real MI355X: ds_crop_blend and the expansion against the restatement tests/periodizer_ref.py (pinned to
the reference's own results by tests/test_periodizer.py), the module around a real network against the reference-equivalent fp32
and fp64 evaluation, the three sampler families with the periodizer as a planned source, and the range guard through the wrapper.

Bounds.  The kernel keeps the reference's operations and their order and multiplies by the same weight table, so every kernel
case is bit equality (torch.equal) with the restatement evaluated in this process in fp32 on the CPU with that table; expansion
and crop are copies.  Around a network: rel-L2 < 1e-5 against the fp32 reference and, against fp64, within max(4 x the reference's
own fp32-fp64 distance, 2e-6) -- the referee rule of tests/test_gpu_ldm_decoder.py; and bit equality with the hand composition
ops.periodic_expand -> net -> ops.crop_blend.  Sampler runs: captured, step-by-step and evaluated-as-given runs are the same
launches on the same inputs -- bit equality."""
import math
import os
import re
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import punetg_ref  # noqa: E402
from tests import periodizer_ref as R  # noqa: E402
from tests.test_gpu_ldm_decoder import referee  # noqa: E402

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "diffsci_amd", "csrc")

# Fields (B, C, H, W), pad, blend_width:
#   2x3x6x7    both axes active, corners take 4 inputs, widths no multiple of 4
#   1x2x4x16   2 bw == H: that axis is skipped; W and its pad multiples of 4: the aligned 16-byte path
#   1x1x8x16   width 0 on one axis; an odd pad on a width that is a multiple of 4: source rows misaligned for the vector path
#   1x2x3x5    a pad longer than the axis (the expansion spans several periods); the other axis pad 0
#   2x1x5x9    pad 0; 2 bw = 8 < 9: the strips meet around a single untouched centre column (2 bw > 5 skips H)
# Volumes (B, C, D, H, W):
#   1x2x5x6x7  three active axes: 8-input corners
#   2x1x4x4x8  two axes skipped
#   1x3x8x8x8  a pure crop
CASES = R.FIELDS + R.VOLUMES
IDS = [R.case_name(*c) for c in CASES]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from diffsci_amd import ops
    return ops


@pytest.fixture(scope="module")
def M():
    import diffsci_amd.models as M
    return M


def tables(ops, bw, n, dev):
    """(the device tables the kernel reads, the same values on the host for the restatement)."""
    w = ops.blend_weights(R.per_axis(bw, n), dev)
    return w, [None if t is None else t.cpu() for t in w]


# ---------------------------------------------------------------- 1. the kernel and the expansion
@pytest.mark.parametrize("k", range(len(CASES)), ids=IDS)
def test_crop_blend_and_expand_bit_for_bit(ops, dev, k):
    from diffsci_amd.extra import DiffusionPeriodizer
    shape, pad, bw = CASES[k]
    n = len(shape) - 2
    x = R.case_input(shape, k) + torch.randn(shape, generator=torch.Generator().manual_seed(k)) * 0.37    # not dyadic: the roundings show
    per = DiffusionPeriodizer(torch.nn.Identity(), pad, bw, dimension=n)
    xd = x.to(dev)
    xe = per.expand_periodic(xd)
    want_e = R.expand(x, pad)
    assert torch.equal(xe.cpu(), want_e) and torch.equal(per.forward_expand_only(xd).cpu(), want_e)
    y = R.analytic_net(want_e)
    yd = y.to(dev)
    assert torch.equal(per.crop_center(yd, shape[2:]).cpu(), R.crop(y, pad, shape[2:]))
    w, wh = tables(ops, bw, n, dev)
    for t in w:
        assert t is None or torch.equal(t.cpu(), R.weights(t.numel()))               # the reference's expression, on the host
    # crop and blend in one pass
    got = ops.crop_blend(yd, pad, bw)
    want = R.blend(R.crop(y, pad, shape[2:]), bw, wh)
    assert got.shape == want.shape and torch.equal(got.cpu(), want), IDS[k]
    assert torch.equal(yd.cpu(), y)
    # the same into a given buffer one float off a 16-byte boundary, and from one
    out = torch.empty(want.numel() + 1, device=dev)[1:].view(want.shape)
    assert ops.crop_blend(yd, pad, bw, out=out) is out and torch.equal(out.cpu(), want)
    ys = torch.empty(y.numel() + 1, device=dev)[1:].view(y.shape)
    ys.copy_(yd)
    assert torch.equal(ops.crop_blend(ys, pad, bw).cpu(), want)
    # cosine_blend_boundaries: a new tensor, the input unchanged; the kernel with zero pads
    before = xd.clone()
    b = per.cosine_blend_boundaries(xd)
    assert b.data_ptr() != xd.data_ptr() and torch.equal(xd, before)
    assert torch.equal(b.cpu(), R.blend(x, bw, wh))
    # forward and forward_no_blend around an analytic network evaluated by torch on the device
    per.net = Analytic()
    on_device = R.analytic_net(xe).cpu()
    assert torch.equal(per.forward_no_blend(xd).cpu(), R.crop(on_device, pad, shape[2:]))
    assert torch.equal(per(xd).cpu(), R.blend(R.crop(on_device, pad, shape[2:]), bw, wh))


class Analytic(torch.nn.Module):
    def forward(self, x, *args, **kwargs):
        return R.analytic_net(x)


def launch_shape(planes, A):
    """ds_crop_blend's launch: (rows, quads, lanes per row, rows per block, grid.x, grid.y), the caps read off the source."""
    with open(os.path.join(CSRC, "ds_periodize.hip")) as f:
        src = f.read()
    threads = int(re.search(r"constexpr int NT = (\d+);", src).group(1))
    blocks = int(re.search(r"constexpr unsigned MAX_BLOCKS = (\d+);", src).group(1))
    m = re.search(r"\(unsigned\)planes < (\d+)u \? \(unsigned\)planes : (\d+)u;", src)
    assert m.group(1) == m.group(2)
    most_planes = int(m.group(1))
    rows, quads = A[0] * A[1], (A[2] + 3) // 4
    sh = 0
    while sh < 6 and (1 << sh) < quads:
        sh += 1
    rpb = threads >> sh
    gy = min(planes, most_planes)
    gx = min(-(-rows // rpb), max(blocks // gy, 1))
    return rows, quads, 1 << sh, rpb, gx, gy, most_planes


def test_crop_blend_past_the_grid_caps(ops, dev):
    """The launch caps its grid (1024 planes in grid.y, 2048 workgroups in all) and loops.  103 x 10 = 1030 planes of a
    (20, 20, 5) box: planes 1024 .. 1029 are a second trip of the plane loop and, with grid.x capped at 2, rows 256 and above a
    second trip of the row loop.  Then one field row of 300 floats: 75 quads on 64 lanes, a second trip of the quad loop."""
    shape, pad, bw = (103, 10, 20, 20, 5), (1, 0, 2), (2, 3, 1)
    rows, quads, lpr, rpb, gx, gy, most = launch_shape(shape[0] * shape[1], shape[2:])
    assert shape[0] * shape[1] > most == gy and gx == 2 and rows > gx * rpb
    g = torch.Generator().manual_seed(77)
    y = torch.randn(shape[:2] + tuple(s + 2 * p for s, p in zip(shape[2:], pad)), generator=g)
    w, wh = tables(ops, bw, 3, dev)
    assert torch.equal(ops.crop_blend(y.to(dev), pad, bw).cpu(), R.blend(R.crop(y, pad, shape[2:]), bw, wh))
    shape, pad, bw = (1, 2, 3, 300), (0, 2), (1, 5)
    rows, quads, lpr, rpb, gx, gy, _ = launch_shape(2, (1,) + shape[2:])
    assert quads == 75 > lpr == 64
    y = torch.randn(1, 2, 3, 304, generator=g)
    w, wh = tables(ops, bw, 2, dev)
    assert torch.equal(ops.crop_blend(y.to(dev), pad, bw).cpu(), R.blend(R.crop(y, pad, shape[2:]), bw, wh))


# ---------------------------------------------------------------- 2. around a real network
def small_net(M, dim, seed):
    torch.manual_seed(seed)
    over = dict(model_channels=16, channel_expansion=[2], dimension=dim)
    net = M.PUNetG(M.PUNetGConfig(**over))
    with torch.no_grad():
        for k, w in net.state_dict().items():
            if "gnorm" in k or k.endswith("bias"):
                w.add_(0.2 * torch.randn_like(w))
    sd = {k: w.clone() for k, w in net.state_dict().items()}
    return net, sd, punetg_ref.default_config(**over)


@pytest.mark.parametrize("dim,shape,pad,bw", [(2, (2, 1, 16, 16), 8, 3), (3, (1, 1, 8, 8, 8), 4, 2)], ids=["2d", "3d"])
def test_module_around_punetg_against_the_reference(M, ops, dev, dim, shape, pad, bw):
    from diffsci_amd.extra import DiffusionPeriodizer
    net, sd, cfg = small_net(M, dim, 300 + dim)
    g = torch.Generator().manual_seed(310 + dim)
    x, t = torch.randn(shape, generator=g) * 1.5 + 0.3, torch.tensor([0.3, 2.5][:shape[0]])
    sd64 = {k: w.double() for k, w in sd.items()}
    with torch.inference_mode():
        want32 = R.forward(lambda xe: punetg_ref.punetg_forward(sd, cfg, xe, t), x, pad, bw)
        want64 = R.forward(lambda xe: punetg_ref.punetg_forward(sd64, cfg, xe, t.double()), x.double(), pad, bw)
    per = DiffusionPeriodizer(net, pad, bw, dimension=dim).to(dev).eval()
    xd, td = x.to(dev), t.to(dev)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        with torch.no_grad():
            got = per(xd, td)
            by_hand = ops.crop_blend(net(ops.periodic_expand(xd, pad), td), pad, bw)
            keyword = per(xd, t=td)
    assert tuple(got.shape) == shape
    referee(got.cpu(), want32, want64, f"periodizer around PUNetG {dim}-D")
    assert torch.equal(got, by_hand) and torch.equal(got, keyword)
    assert net.conv_precision == "fp16x3"


# ---------------------------------------------------------------- 3. inside the samplers
def hidden(per):
    """The same periodizer with its planned protocol hidden: the run is evaluated as given."""
    per.__dict__["forward_with_shifts"] = None
    return per


def three_ways(module, per, sample):
    """(captured, step by step, evaluated as given), each from the same seed."""
    out = []
    for use_graph, hide in ((True, False), (False, False), (True, True)):
        module.use_graph = use_graph
        if hide:
            hidden(per)
        torch.manual_seed(1234)
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)
            out.append(sample())
        per.__dict__.pop("forward_with_shifts", None)
    module.use_graph = True
    return out


def test_karras_module_runs_the_periodizer_as_a_planned_source(M, dev):
    from diffsci_amd.extra import DiffusionPeriodizer
    from diffsci_amd.models.karras.engine import ModuleSource
    net, _, _ = small_net(M, 2, 320)
    per = DiffusionPeriodizer(net, 8, 3, dimension=2)
    module = M.KarrasModule(per, M.KarrasModuleConfig.from_edm()).to(dev).eval()
    like = torch.empty(2, 1, 16, 16, device=dev)
    assert ModuleSource(module, None, 1.0, 2, like).planned and not ModuleSource(module, None, 1.0, 2, like).batched_cfg
    sample = lambda: module.sample(2, [1, 16, 16], nsteps=3, integrator="heun")          # noqa: E731
    captured, stepped, as_given = three_ways(module, per, sample)
    assert tuple(captured.shape) == (2, 1, 16, 16) and bool(torch.isfinite(captured).all())
    assert torch.equal(captured, stepped) and torch.equal(captured, as_given)
    assert len(module._plans.plans) == 1                       # the as-given run is not captured (capture_eager is off)
    torch.manual_seed(1234)
    assert torch.equal(sample(), captured) and len(module._plans.plans) == 1            # the replay
    hidden(per)
    assert not ModuleSource(module, None, 1.0, 2, like).planned
    per.__dict__.pop("forward_with_shifts")
    assert ModuleSource(module, None, 1.0, 2, like).planned
    per.blend_width = (2, 2)
    torch.manual_seed(1234)
    other = sample()
    assert len(module._plans.plans) == 2 and not torch.equal(other, captured)


def test_ddpm_module_runs_the_periodizer_as_a_planned_source(M, dev):
    from diffsci_amd.extra import DiffusionPeriodizer
    V = M.ddpmv2
    net, _, _ = small_net(M, 2, 330)
    per = DiffusionPeriodizer(net, 8, 3, dimension=2)
    # (the "exp" schedule: the classical one's 3-step table is degenerate -- its alpha-bar reaches 0 and the coefficients are NaN)
    module = V.DDPMModule(per, V.DDPMModuleConfig.from_ddim("exp")).to(dev).eval()
    captured, stepped, as_given = three_ways(module, per, lambda: module.sample(2, [1, 16, 16], nsteps=3))
    assert bool(torch.isfinite(captured).all()) and torch.equal(captured, stepped) and torch.equal(captured, as_given)
    assert len(module._plans.plans) == 1


def test_si_module_runs_the_periodizer_as_a_planned_source(M, dev):
    from diffsci_amd.extra import DiffusionPeriodizer
    net, _, _ = small_net(M, 2, 340)
    per = DiffusionPeriodizer(net, 8, 3, dimension=2)
    module = M.SIModule(M.SIModuleConfig(scheduler="linear"), per).to(dev).eval()
    captured, stepped, as_given = three_ways(module, per, lambda: module.sample(2, [1, 16, 16], nsteps=3))
    assert bool(torch.isfinite(captured).all()) and torch.equal(captured, stepped) and torch.equal(captured, as_given)
    assert len(module._plans.plans) == 1


def test_range_guard_escalates_the_inner_network_through_the_wrapper(M, dev):
    """One weight of the first block's first convolution set to 2^57.  The fp16x3 packing scales a layer by a power of two
    clamped at 2^-40 (ops.pack_conv), so that weight becomes 2^17 > 65504 = inf in fp16 and the expanded run's result is not
    finite although its inputs are; in fp32 the network is finite (one channel of about 1e17 that the block's second norm
    divides away).  The run's last step kernel raises the result word -- the inner network's, asked through the wrapper -- the
    run escalates the INNER network to bf16x6 once, with the warning, and runs again: a finite result, a second plan."""
    from diffsci_amd.extra import DiffusionPeriodizer
    from diffsci_amd.models.nets import precision
    net, _, _ = small_net(M, 2, 350)
    with torch.no_grad():
        next(iter(net._resblocks())).conv1.weight[0, 0, 1, 1] = 2.0 ** 57
    per = DiffusionPeriodizer(net, 8, 3, dimension=2)
    module = M.KarrasModule(per, M.KarrasModuleConfig.from_edm()).to(dev).eval()
    wn = torch.randn(2, 1, 16, 16, generator=torch.Generator().manual_seed(7)).to(dev)
    with pytest.warns(RuntimeWarning, match="fp16x3 convolution range") as seen:
        out = module.propagate_white_noise(wn, nsteps=3)
    assert len([w for w in seen if "fp16x3 convolution range" in str(w.message)]) == 1
    assert net.conv_precision == "bf16x6" and per.conv_precision == "bf16x6" and "conv_precision" not in per.__dict__
    assert bool(torch.isfinite(out).all())
    assert precision.guard_words(per, dev).tolist() == [0, 0] and precision.guard_words(net, dev) is precision.guard_words(per, dev)
    assert len(module._plans.plans) == 2                       # the fp16x3 capture and the bf16x6 one
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        assert torch.equal(module.propagate_white_noise(wn, nsteps=3), out)
    assert math.isfinite(float(out.abs().max()))
