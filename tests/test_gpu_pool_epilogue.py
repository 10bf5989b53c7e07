"""The DownSampler's MaxPool2d(2) from the store phase of the persistent 3x3 kernel (ds_conv3p.hip, POOL; ds_conv2d_h3_pc).

Max pooling is exact and the pooled launch stores what the plain one stores, so every comparison here is bit for bit: the pooled
output against torch's max_pool2d of the launch's own output, the launch's other outputs against the same launch without pool_out,
and the network on the "pass" and "epilogue" routes against the "loader" route (PUNetG.pool_route).  Shapes: the smallest that give
a 256-CU part at least one (channel tile, pixel tile, sample) item per workgroup -- 272 items of one channel tile (some workgroups
walk two items, most one) and 256 items of two channel tiles."""
import math

import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and bool((_bits(a) == _bits(b)).all())


_CASES = {}


def _case(dev, B, C, H, W):
    """Inputs of a residual block's second convolution, made once per shape and left unchanged."""
    key = (B, C, H, W)
    if key not in _CASES:
        from diffsci_amd import ops
        g = torch.Generator().manual_seed(1000 + C)
        x = torch.randn(B, C, H, W, generator=g).to(dev)
        w = (torch.randn(C, C, 3, 3, generator=g) / math.sqrt(C * 9)).to(dev)
        tab = torch.zeros(B, ops.table_channels(C), 4)
        tab[:, :C, 0] = torch.randn(B, C, generator=g) * 0.3
        tab[:, :C, 1] = torch.rand(B, C, generator=g) + 0.5
        tab[:, :C, 2] = torch.randn(B, C, generator=g) * 0.3
        tab[:, :, 3] = 2.0 ** -3
        gw, gb = (torch.randn(C, generator=g) * 0.2 + 1.0).to(dev), (torch.randn(C, generator=g) * 0.2).to(dev)
        _CASES[key] = dict(x=x, pw=ops.pack_conv(w, "fp16x3"), bias=torch.randn(C, generator=g).to(dev),
                           res1=torch.randn(B, C, H, W, generator=g).to(dev), res2=torch.randn(B, C, H, W, generator=g).to(dev),
                           tab=tab.to(dev), img=ops.inorm_silu_images(x, gw, gb, 0, eps=1e-5))
    return _CASES[key]


def _launch(dev, c, shape, nres, image, extras, pooled):
    from diffsci_amd import ops
    B, C, H, W = shape
    ts = torch.full((B, C, ops.conv_tile_count(H, W), 4), float("nan"), device=dev) if extras else None
    oa = torch.zeros(B, dtype=torch.int32, device=dev) if extras else None
    pool = ops.PoolOut(torch.full((B, C, H // 2, W // 2), float("nan"), device=dev)) if pooled else None
    kw = dict(bias=c["bias"], res1=c["res1"], res2=c["res2"] if nres == 2 else None, tile_stats=ts, out_amax=oa)
    if pooled:
        kw["pool"] = pool
    if image:
        out = ops.conv_img(c["img"], c["pw"], B, C, H, W, **kw)
    else:
        out = ops.conv(c["x"], c["pw"], prenorm=c["tab"], **kw)
    torch.cuda.synchronize()
    return out, ts, oa, pool


@gpu
@pytest.mark.parametrize("shape", [(17, 64, 32, 128), (32, 128, 16, 64)], ids=["c64-272items", "c128-256items"])
@pytest.mark.parametrize("extras", [True, False], ids=["stats+amax", "bare"])
@pytest.mark.parametrize("image", [False, True], ids=["fused", "image"])
@pytest.mark.parametrize("nres", [1, 2])
def test_store_phase_pools(dev, shape, nres, image, extras):
    if torch.cuda.get_device_properties(dev).multi_processor_count > 256:
        pytest.fail("the shapes of this test assume at most 256 compute units")
    c = _case(dev, *shape)
    out, ts, oa, pool = _launch(dev, c, shape, nres, image, extras, True)
    want, ts0, oa0, _ = _launch(dev, c, shape, nres, image, extras, False)
    assert pool.written, "a qualifying launch must pool"
    assert _same(pool.tensor, F.max_pool2d(out, 2))
    assert _same(out, want)
    if extras:
        assert _same(ts, ts0) and bool((oa == oa0).all()) and bool((oa != 0).all())


@gpu
def test_launches_that_do_not_qualify_say_so(dev):
    """No residual, periodic padding, a raw input, too few items: out is complete, pool_out untouched, the answer is False."""
    from diffsci_amd import ops
    shape = (17, 64, 32, 128)
    B, C, H, W = shape
    c = _case(dev, *shape)
    want = ops.conv(c["x"], c["pw"], prenorm=c["tab"], bias=c["bias"])
    for kw in (dict(prenorm=c["tab"]), dict(prenorm=c["tab"], res1=c["res1"], circular=True), dict(res1=c["res1"])):
        pool = ops.PoolOut(torch.full((B, C, H // 2, W // 2), 7.0, device=dev))
        out = ops.conv(c["x"], c["pw"], bias=c["bias"], pool=pool, **kw)
        assert not pool.written and bool((pool.tensor == 7.0).all())
        assert _same(out, ops.conv(c["x"], c["pw"], bias=c["bias"], **kw))
    assert _same(ops.conv(c["x"], c["pw"], prenorm=c["tab"], bias=c["bias"], pool=ops.PoolOut(torch.empty(B, C, H // 2, W // 2, device=dev))), want)
    few = ops.PoolOut(torch.full((2, C, H // 2, W // 2), 7.0, device=dev))
    ops.conv(c["x"][:2], c["pw"], prenorm=c["tab"][:2].contiguous(), res1=c["res1"][:2], pool=few)
    assert not few.written and bool((few.tensor == 7.0).all())
    with pytest.raises(ValueError):
        ops.conv(c["x"], c["pw"], prenorm=c["tab"], res1=c["res1"], pool=ops.PoolOut(torch.empty(B, C, H // 2, W, device=dev)))


@gpu
def test_raw_launch_on_the_persistent_kernel_equals_the_one_shot_kernel(dev):
    """pc_raw: the plain raw-input convolution (the DownSampler after a pooling pass) on the persistent kernel."""
    from diffsci_amd import ops
    shape = (17, 64, 32, 128)
    c = _case(dev, *shape)
    ia = ops.absmax_rows(c["x"])
    ts = [torch.empty(17, 64, ops.conv_tile_count(32, 128), 4, device=dev) for _ in range(2)]
    a = ops.conv(c["x"], c["pw"], bias=c["bias"], in_amax=ia, tile_stats=ts[0])
    b = ops.conv(c["x"], c["pw"], bias=c["bias"], in_amax=ia, tile_stats=ts[1], pc_raw=True)
    assert _same(a, b) and _same(ts[0], ts[1])


def _net_outputs(M, dev, cfg_kw, shape, routes, seed):
    """{route: (eager output, captured output)} of one network on one input."""
    torch.manual_seed(seed)
    net = M.PUNetG(M.PUNetGConfig(**cfg_kw)).to(dev).eval()
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(*shape, generator=g).to(dev)
    t = (torch.rand(shape[0], generator=g) + 0.1).to(dev)
    got = {}
    with torch.inference_mode():
        shifts = net.time_shifts(net.embed_time(t))
        for route in routes:
            net.pool_route = route
            eager = net.forward_with_shifts(x, shifts).clone()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                y = net.forward_with_shifts(x, shifts)
            graph.replay()
            torch.cuda.synchronize()
            got[route] = (eager, y.clone())
    return got


@gpu
def test_network_routes_agree(dev):
    """PUNetG at 64 channels on [17, 1, 32, 128]: two DownSamplers; the first level's last block pools in its store phase (272
    items), the second level's has too few items and keeps the loader."""
    import diffsci_amd.models as M
    got = _net_outputs(M, dev, dict(model_channels=64), (17, 1, 32, 128), ("loader", "pass", "epilogue"), 5)
    want = got["loader"][0]
    assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0
    for route in ("loader", "pass", "epilogue"):
        for kind, y in zip(("eager", "captured"), got[route]):
            assert _same(y, want), f"{route} ({kind}) differs from the loader route"


@gpu
@pytest.mark.parametrize("cfg_kw,shape", [(dict(model_channels=64), (2, 1, 24, 40)),
                                           (dict(model_channels=64, convolution_type="circular"), (17, 1, 32, 128))],
                         ids=["24x40-plane", "circular"])
def test_network_whose_last_block_does_not_qualify(dev, cfg_kw, shape):
    import diffsci_amd.models as M
    got = _net_outputs(M, dev, cfg_kw, shape, ("loader", "epilogue"), 6)
    want = got["loader"][0]
    assert bool(torch.isfinite(want).all())
    for y in got["epilogue"]:
        assert _same(y, want)


# ------------------------------------------------------------------ host side: no GPU
def test_unknown_route_is_refused():
    import diffsci_amd.models as M
    net = M.PUNetG(M.PUNetGConfig(model_channels=8)).eval()
    net.pool_route = "epilog"
    with pytest.raises(ValueError, match="pool_route"):
        net.forward_with_shifts(torch.zeros(1, 1, 16, 16), [])


def test_entry_point_in_header_exports_and_ctypes():
    import ctypes
    import json
    import os

    import build
    from diffsci_amd import _native as N
    from tests import abi_trace
    from tests.test_native_abi import header_functions
    assert "ds_conv2d_h3_pc" in header_functions()
    assert hasattr(ctypes.CDLL(build.build(force=False, verbose=False)), "ds_conv2d_h3_pc")
    res, args = N._PROTOS["ds_conv2d_h3_pc"]
    h3 = N._PROTOS["ds_conv2d_h3"][1]
    assert res is ctypes.c_int and args[:len(h3)] == h3 and len(args) == len(h3) + 3 and args[-1] is ctypes.c_int
    assert N.ABI_VERSION == 4 and len(h3) == 20
    # ds_conv2d_h3 itself is what it was: the pinned trace still holds its calls, argument for argument
    with open(os.path.join(os.path.dirname(__file__), "golden", "abi_trace.json")) as f:
        calls = [c for t in json.load(f)["cases"].values() for c in t["calls"] if c[0] == "ds_conv2d_h3"]
    assert calls and all(len(c) == 21 for c in calls)
    assert "ds_conv2d_h3_pc" not in abi_trace.LAUNCHES          # its stream is not the last argument: the trace table is the parent's


def test_wrapper_routes_to_the_new_entry_only_when_asked(monkeypatch):
    """conv2d without pool / pc_raw launches ds_conv2d_h3 with the arguments it always had; with either, ds_conv2d_h3_pc with the
    same leading arguments, the pooled buffer and the flags word."""
    from diffsci_amd import _native as N
    from diffsci_amd import ops
    real, seen = N.lib(), []

    class Stub:
        def __getattr__(self, name):
            if name not in ("ds_conv2d_h3", "ds_conv2d_h3_pc"):
                return getattr(real, name)

            def launch(*a):
                seen.append((name, a))
                return 0
            return launch

    monkeypatch.setattr(ops, "_off_device", lambda t: None)
    monkeypatch.setattr(N, "lib", lambda: Stub())
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    B, C, H, W = 2, 64, 8, 32
    x, res = torch.zeros(B, C, H, W), torch.zeros(B, C, H, W)
    pw = ops.PackedConv(torch.zeros(real.ds_conv2d_h3_packed_bytes(C, C) // 4), C, C, 3, "fp16x3")
    tab = torch.zeros(B, ops.table_channels(C), 4)
    out = torch.zeros(B, C, H, W)
    ops.conv(x, pw, prenorm=tab, res1=res, out=out)
    pool = ops.PoolOut(torch.zeros(B, C, H // 2, W // 2))
    ops.conv(x, pw, prenorm=tab, res1=res, out=out, pool=pool)
    ia = torch.zeros(B, dtype=torch.int32)
    ops.conv(x, pw, in_amax=ia, out=out, pc_raw=True)
    assert [n for n, _ in seen] == ["ds_conv2d_h3", "ds_conv2d_h3_pc", "ds_conv2d_h3_pc"]
    plain, pooled, raw = (a for _, a in seen)
    assert len(plain) == 20 and pooled[:20] == plain and pooled[20] == pool.tensor.data_ptr() and pooled[22] == 0
    assert not pool.written                                       # the stub wrote no answer
    assert raw[20] is None and raw[22] == N.DS_PC_RAW and raw[15] is None and raw[17] == ia.data_ptr()
