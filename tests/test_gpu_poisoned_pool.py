"""Whole networks on a pool that is never clean.  runtime.Workspace hands the same torch.empty memory to one layer after another
and, after capture, to every replay; nothing clears it.  Here every buffer the pool hands out outside stream capture -- fresh or
reused -- is first filled with a poison (tests/guarded.py: the NaN pattern, then 3.0e38), and so is every fresh float32 / int32
device tensor the package asks torch.empty for (the op wrappers' own outputs and scratch, and the networks that keep no pool:
VAENet and the LDM decoder).  One eager forward of the smallest configuration of each family that reaches every route must
equal, bit for bit, the forward on an untouched pool.  Four runs per case on one network:

    baseline   untouched pool (fresh device memory)
    A          every take poisoned
    B          nothing poisoned: the pool now holds what A left -- real, finite, plausible data, and A's poison wherever no
               launch wrote -- the state of a long-lived process
    C          every take poisoned again

Forwards are the unguarded ones (forward_unguarded): the domain guards of nets/precision.py would answer a NaN by recomputing on
another arithmetic, and hide it; RuntimeWarnings are errors for the same reason.

Captured runs: capture, replay, poison every tensor in every free list of the network's pool (dead by the pool's own contract;
what a plan took and kept is not touched), replay: the two replays must be bit-equal -- a replay is a function of its inputs, not
of the previous replay."""
import warnings

import pytest
import torch

from tests import convit_ref, dit_ref, ldm_ref, net_trace, vaenet_ref
from tests.golden_util import load
from tests.guarded import POISONS

pytestmark = pytest.mark.gpu
B = 2


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def M():
    import diffsci_amd.models as M
    return M


def _fill(t, bits):
    if t.is_cuda and t.numel() and t.dtype in (torch.float32, torch.int32) and t.is_contiguous():
        t.view(torch.int32).fill_(bits)
    return t


def _poison_takes(mp, bits):
    """Inside the monkeypatch context mp: Workspace.take and torch.empty fill what they return, except under stream capture."""
    from diffsci_amd.models.nets import runtime
    take, empty, count = runtime.Workspace.take, torch.empty, [0]

    def poisoned_take(self, shape, device):
        t = take(self, shape, device)
        if torch.cuda.is_current_stream_capturing():
            return t
        count[0] += 1
        return _fill(t, bits)

    def poisoned_empty(*args, **kw):
        t = empty(*args, **kw)
        if not t.is_cuda or torch.cuda.is_current_stream_capturing():
            return t
        count[0] += 1
        return _fill(t, bits)

    mp.setattr(runtime.Workspace, "take", poisoned_take)
    mp.setattr(torch, "empty", poisoned_empty)
    return count


def _outputs(run):
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        with torch.inference_mode():
            out = run()
    outs = out if isinstance(out, (list, tuple)) else [out]
    torch.cuda.synchronize()
    return [o.clone() for o in outs]


def _same(a, b):
    return all(x.shape == y.shape and torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))
               for x, y in zip(a, b)) and len(a) == len(b)


def check_on_poisoned_pool(run, monkeypatch, bits):
    base = _outputs(run)
    assert all(bool(torch.isfinite(o).all()) and bool(o.abs().max() > 0) for o in base), "the baseline is blind"
    with monkeypatch.context() as mp:
        poisoned = _poison_takes(mp, bits)
        a = _outputs(run)
    assert poisoned[0] > 0, "no buffer was poisoned: the case is blind"
    b = _outputs(run)
    with monkeypatch.context() as mp:
        _poison_takes(mp, bits)
        c = _outputs(run)
    bad = [name for name, got in (("A: poisoned takes", a), ("B: the pool A left", b), ("C: poisoned takes again", c))
           if not _same(got, base)]
    assert not bad, bad


def _randomise(net, seed):
    """Default initialisations zero some layers (a zero output layer would make the case blind): every parameter moves."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in net.parameters():
            p.add_(0.05 * torch.randn(p.shape, generator=g))
    return net


def _x(seed, *shape):
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(seed))
    x[0] *= 2.0 ** -6                                       # per-sample activation exponents differ
    return x


def _punetg(dev, dim=2, side=16, batch=B, switches=(), cls="PUNetG", cls_args=(), sides=None, **cfg):
    torch.manual_seed(5)
    net, _ = net_trace.punetg(dim, cls=cls, cls_args=cls_args, **cfg)
    net = _randomise(net, 6).to(dev).eval()
    for k, v in switches:
        assert hasattr(net, k)
        setattr(net, k, v)
    sides = sides or (side,) * dim
    x = _x(7, batch, net.config.input_channels if cls == "PUNetG" else 1, *sides).to(dev)
    t = torch.linspace(0.2, 1.1, batch).to(dev)
    return net, x, t


# name -> (keyword arguments of _punetg); net_trace.BASE: 16 -> 32 channels, one transition, attention at the bottom
PUNETG = {
    "fused_loader_2d": dict(),                                                     # norms folded into the loaders (the default)
    "fused_loader_ragged_2d": dict(side=24),                                       # 24 x 24: ragged pixel tiles on both geometries
    "images_2d": dict(model_channels=32, switches=(("fuse_max_cot", 0),)),         # standalone norms write pre-split images
    "table_images_2d": dict(model_channels=32, side=72, batch=1, switches=(("fuse_max_cot", 0),)),    # planes the image kernel refuses
    "standalone_norms_2d": dict(model_channels=32, switches=(("fuse_max_cot", 0), ("norm_images", False))),
    "unfused_2d": dict(switches=(("fuse_norm", False),)),
    "pool_loader_2d": dict(switches=(("pool_route", "loader"),)),
    "pool_pass_2d": dict(switches=(("pool_route", "pass"),)),
    "pool_epilogue_2d": dict(switches=(("pool_route", "epilogue"),)),
    # 64 channels at 32 x 32, batch 64: 4 pixel tiles x 64 samples = 256 items, the persistent kernel and its pooled epilogue
    "persistent_2d": dict(model_channels=64, side=32, batch=64),
    "circular_2d": dict(convolution_type="circular"),
    "k5_2d": dict(kernel_size=5),
    # L = 32 x 64 = 2048 at the bottom: the image form of the attention, its workspace from the pool; folded K / V and not
    "attention_folded_2d": dict(batch=1, sides=(64, 128), switches=(("attn_fold", True),)),
    "attention_unfolded_2d": dict(batch=1, sides=(64, 128), switches=(("attn_fold", False),)),
    "volumes_3d": dict(dim=3, side=8),
    "volumes_circular_3d": dict(dim=3, side=8, convolution_type="circular"),
    "volumes_unfused_3d": dict(dim=3, side=8, switches=(("fuse_norm", False),)),
}


@pytest.mark.parametrize("poison", list(POISONS))
@pytest.mark.parametrize("name", list(PUNETG))
def test_punetg(dev, monkeypatch, name, poison):
    net, x, t = _punetg(dev, **PUNETG[name])
    check_on_poisoned_pool(lambda: net.forward_unguarded(x, t), monkeypatch, POISONS[poison])


@pytest.mark.parametrize("poison", list(POISONS))
@pytest.mark.parametrize("dim", [2, 3])
def test_punetg_cond_with_a_field(dev, monkeypatch, dim, poison):
    side = 16 if dim == 2 else 8
    net, x, t = _punetg(dev, dim=dim, side=side, cls="PUNetGCond", cls_args=(None, ["c"]))
    y = {"c": _x(9, 1, 1, *(side,) * dim).to(dev)}
    check_on_poisoned_pool(lambda: net.forward_unguarded(x, t, y), monkeypatch, POISONS[poison])


@pytest.mark.parametrize("poison", list(POISONS))
@pytest.mark.parametrize("dim,side,batch,shared", [(2, 16, 2, False), (2, 16, 2, True), (2, 16, 1, False),
                                                   (3, 8, 2, False), (3, 8, 2, True), (3, 8, 1, False), (3, 16, 1, False)])
def test_punetg_with_a_field_valued_embedding(dev, monkeypatch, dim, side, batch, shared, poison):
    """A field of embeddings ye [1 or B, model_channels, *sides] (no embedding module: y is ye): per-pixel time MLPs from the
    corner-pooled field (_FieldShifts, ops.cornerpool_f, the 1x1 convolutions with their arena rows), at batch 2 and 1."""
    net, x, t = _punetg(dev, dim=dim, side=side, batch=batch)
    ye = _x(11, 1 if shared else batch, net.config.model_channels, *(side,) * dim).to(dev)
    check_on_poisoned_pool(lambda: net.forward_unguarded(x, t, ye), monkeypatch, POISONS[poison])


ADM = {
    "default": dict(),
    "images": dict(model_channels=32, switches=(("fuse_max_cot", 0),)),
    "images_off": dict(model_channels=32, switches=(("fuse_max_cot", 0), ("norm_images", False))),
    "unfused": dict(switches=(("fuse_norm", False),)),
    "side64_images": dict(model_channels=32, side=64, batch=1, switches=(("fuse_max_cot", 0),)),      # the parity kernel on images
}


@pytest.mark.parametrize("poison", list(POISONS))
@pytest.mark.parametrize("name", list(ADM))
def test_adm(dev, monkeypatch, name, poison):
    kw = dict(ADM[name])
    side, batch, switches = kw.pop("side", 16), kw.pop("batch", B), kw.pop("switches", ())
    torch.manual_seed(5)
    net, _ = net_trace.adm(2, **kw)
    net = _randomise(net, 8).to(dev).eval()
    for k, v in switches:
        assert hasattr(net, k)
        setattr(net, k, v)
    x = _x(7, batch, 2, side, side).to(dev)
    t = torch.linspace(0.2, 1.1, batch).to(dev)
    check_on_poisoned_pool(lambda: net.forward_unguarded(x, t), monkeypatch, POISONS[poison])


@pytest.mark.parametrize("poison", list(POISONS))
def test_adm_block_with_two_heads(dev, monkeypatch, M, poison):
    """ADMEncoderBlock(attn_heads=2) at 64 channels: the head-axis kernel at d = 32 (L = 64), buffers from torch.empty."""
    torch.manual_seed(5)
    blk = M.nets.ADMEncoderBlock(16, 64, 24, has_residual=True, has_attn=True, attn_heads=2)
    blk = _randomise(blk, 3).to(dev).eval()
    x, te = _x(1, B, 16, 8, 8).to(dev), _x(2, B, 24).to(dev)
    check_on_poisoned_pool(lambda: blk(x, te), monkeypatch, POISONS[poison])


@pytest.mark.parametrize("poison", list(POISONS))
def test_dit(dev, monkeypatch, M, poison):
    v, sd, kw = dit_ref.load_golden("a")
    net = M.DiffusionTransformer(**kw)
    net.load_state_dict(sd, strict=True)
    net = net.to(dev).eval()
    x, t = v["x"].to(dev), v["t"].to(dev)
    check_on_poisoned_pool(lambda: net.forward_unguarded(x, t), monkeypatch, POISONS[poison])


@pytest.mark.parametrize("poison", list(POISONS))
def test_convit(dev, monkeypatch, M, poison):
    v, sd, kw = convit_ref.load_golden("a")
    net = M.nets.ConVit(M.nets.ConVitConfig(**kw), conditional_embedding=torch.nn.Linear(1, kw.get("embed_dim", 64)))
    net.load_state_dict(sd, strict=True)
    net = net.to(dev).eval()
    x, t, y = v["x"].to(dev), v["t"].to(dev), v["y"].to(dev)
    check_on_poisoned_pool(lambda: net.forward_unguarded(x, t, y), monkeypatch, POISONS[poison])


@pytest.mark.parametrize("poison", list(POISONS))
@pytest.mark.parametrize("fuse", [True, False])
def test_vaenet_encode_and_decode(dev, monkeypatch, fuse, poison):
    v, sd, info = vaenet_ref.load_golden("a")
    net = vaenet_ref.build(info)
    net.load_state_dict(sd, strict=True)
    net = net.to(dev).eval()
    net.fuse_norm = fuse
    x, eps, zin = v["x"].to(dev), v["eps"].to(dev), v["zin"].to(dev)
    check_on_poisoned_pool(lambda: [net.encode(x, sample=False), net.encode(x, eps=eps), net.decode(zin)], monkeypatch, POISONS[poison])


@pytest.mark.parametrize("poison", list(POISONS))
@pytest.mark.parametrize("fuse", [True, False])
def test_ldm_decoder(dev, monkeypatch, fuse, poison):
    v, sd, info = ldm_ref.load_golden("a")
    net = ldm_ref.build(info)
    net.load_state_dict(sd, strict=True)
    net = net.to(dev).eval()
    net.fuse_norm = fuse
    z = v["z"].to(dev)
    check_on_poisoned_pool(lambda: net(z), monkeypatch, POISONS[poison])


# ---------------------------------------------------------------------------------------------------------------- captured runs
def _net8(M, dev):
    _, sd = load("punetg8_forward")
    net = M.PUNetG(M.PUNetGConfig(model_channels=8))
    net.load_state_dict(sd)
    return net.to(dev).eval()


def _poison_free_lists(net, bits):
    n = 0
    for lst in net._ws.free.values():
        for t in lst:
            _fill(t, bits)
            n += 1
    torch.cuda.synchronize()
    return n


def check_replays(module, net, run, bits):
    module.use_graph = True
    module._plans.clear()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        first = run().clone()                               # the capture
        assert len(module._plans.plans) == 1
        second = run().clone()                              # a replay
        assert _poison_free_lists(net, bits) > 0
        third = run().clone()                               # a replay over a dead pool full of poison
    assert len(module._plans.plans) == 1
    assert bool(torch.isfinite(second).all()) and bool(second.abs().max() > 0)
    assert torch.equal(first, second), "the first replay differs from the capturing run"
    assert torch.equal(second, third), "a replay depends on what the pool's free buffers held"


@pytest.mark.parametrize("poison", list(POISONS))
def test_captured_karras_heun(dev, M, poison):
    net = _net8(M, dev)
    module = M.KarrasModule(net, M.KarrasModuleConfig.from_edm()).to(dev).eval()
    wn = _x(3, B, 1, 32, 32).to(dev)
    check_replays(module, net, lambda: module.propagate_white_noise(wn, nsteps=4), POISONS[poison])


@pytest.mark.parametrize("poison", list(POISONS))
def test_captured_si_inpainting(dev, M, poison):
    net = _net8(M, dev)
    module = M.SIModule(M.SIModuleConfig(scheduler="cosine", precondition_fn="edm", initial_norm=2.0), net).to(dev).eval()
    g = torch.Generator().manual_seed(4)
    x_orig, mask = torch.randn(1, 32, 32, generator=g), (torch.rand(1, 32, 32, generator=g) < 0.4).float()

    def run():
        torch.manual_seed(5)
        return module.inpaint_fused(x_orig, mask, nsamples=2, nsteps=5, mask_falloff=2, resample_steps=1, mask_start_t=0.8)
    check_replays(module, net, run, POISONS[poison])


@pytest.mark.parametrize("poison", list(POISONS))
def test_captured_ddpm(dev, M, poison):
    V = M.ddpmv2
    net = _net8(M, dev)
    module = V.DDPMModule(net, V.DDPMModuleConfig.from_ddpm("exp")).to(dev)
    x = _x(3, B, 1, 32, 32).to(dev)

    def run():
        torch.manual_seed(21)
        return module.propagate_toward_sample(x, nsteps=6)
    check_replays(module, net, run, POISONS[poison])
