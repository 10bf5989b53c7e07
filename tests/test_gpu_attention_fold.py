"""The folded single-head attention block on the GPU: ds_attention_h3_xkv against ds_attention_h3_ws bit for
bit, its three exponent rows against fp64, runtime.attention folded against unfolded against the fp64 module, and PUNetG-64 with
attn_fold on against off.

Bounds.  (1) equality of bits.  (2) check_rows of tests/test_gpu_attention_edges.py, the bound of the image form at the same E.
(3) err(folded) <= 2 x max(err(unfolded), err(torch fp32 on the CPU)), max-abs over the output against the fp64 module: the two
routes round at the same level through different summation trees.  (4) max |folded - unfolded| <= 2 x max |fp16x3 - fp32
convolutions| of the unfolded network on the same input."""
import pytest
import torch

from tests.test_gpu_attention_edges import check_rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _xkv(N, q, x, rows, out_amax):
    """ds_attention_h3_xkv on a NaN-filled output; rows = (q_amax, k_amax, v_amax)."""
    B, E, L = q.shape
    out = torch.full((B, E, L), float("nan"), device=q.device)
    work = torch.empty(N.lib().ds_attention_h3_workspace_bytes(B, E, L) // 4, device=q.device)
    N.check(N.lib().ds_attention_h3_xkv(out.data_ptr(), q.data_ptr(), x.data_ptr(), work.data_ptr(), B, E, L, _ptr(rows[0]),
                                        _ptr(rows[1]), _ptr(rows[2]), _ptr(out_amax), _stream(), 0), "ds_attention_h3_xkv")
    return out


def _ws(N, qkv, E, in_amax, out_amax):
    B, _, L = qkv.shape
    out = torch.full((B, E, L), float("nan"), device=qkv.device)
    work = torch.empty(N.lib().ds_attention_h3_workspace_bytes(B, E, L) // 4, device=qkv.device)
    N.check(N.lib().ds_attention_h3_ws(out.data_ptr(), qkv.data_ptr(), work.data_ptr(), B, E, L, _ptr(in_amax), _ptr(out_amax),
                                       _stream()), "ds_attention_h3_ws")
    return out


def _same(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---------------------------------------------------------------- 1. the old entry's bits
@pytest.mark.parametrize("L", [32, 160])
@pytest.mark.parametrize("E", [32, 256])
def test_same_bits_as_the_qkv_entry(dev, E, L):
    """E = 256 is the 512-register, 128 KiB instance; L = 32 one key tile, L = 160 two query blocks, the second a single wave
    that stores and three that recompute."""
    from diffsci_amd import _native as N
    from diffsci_amd import ops
    B = 2
    q, x = _randn(E + L, B, E, L).to(dev), (3.0 * _randn(E + L + 1, B, E, L)).to(dev)
    qkv = torch.cat([q, x, x], dim=1).contiguous()
    r = ops.absmax_rows(qkv)                                   # one row for everything: what the old entry can express
    for rows, in_amax in (((r, r, r), torch.cat([r, r])), ((None, None, None), None)):
        a_new, a_old = ops.amax_new(B, dev), ops.amax_new(B, dev)
        got, want = _xkv(N, q, x, rows, a_new), _ws(N, qkv, E, in_amax, a_old)
        assert bool(torch.isfinite(want).all()) and _same(got, want), f"E={E} L={L} rows={'given' if in_amax is not None else 'NULL'}"
        assert torch.equal(a_new, a_old)
        assert torch.equal(a_new.view(torch.float32), got.abs().flatten(1).amax(dim=1))


def test_flags_must_be_zero(dev):
    from diffsci_amd import _native as N
    q = torch.zeros(1, 32, 32, device=dev)
    work = torch.empty(N.lib().ds_attention_h3_workspace_bytes(1, 32, 32) // 4, device=dev)
    rc = N.lib().ds_attention_h3_xkv(q.data_ptr(), q.data_ptr(), q.data_ptr(), work.data_ptr(), 1, 32, 32, None, None, None, None,
                                     _stream(), 1)
    assert rc != 0


# ---------------------------------------------------------------- 2. separate exponents
@pytest.mark.parametrize("L", [32, 160])
@pytest.mark.parametrize("E", [32, 256])
def test_separate_exponents_vs_fp64(dev, E, L):
    """q times 2^12, x times 2^-9, sample 1 another 2^6 apart on each side: one shared exponent would push one of the two out of
    fp16's range; the rows are the samples' own, measured."""
    from diffsci_amd import _native as N
    from diffsci_amd import ops
    B = 2
    q, x = _randn(2 * E + L, B, E, L) * 2.0 ** 12, _randn(2 * E + L + 1, B, E, L) * 2.0 ** -9
    q[1] *= 2.0 ** 6
    x[1] *= 2.0 ** -6
    qd, xd = q.to(dev), x.to(dev)
    rq, rx = ops.absmax_rows(qd), ops.absmax_rows(xd)
    slots = ops.amax_new(B, dev)
    got = _xkv(N, qd, xd, (rq, rx, rx), slots)
    assert torch.equal(slots.view(torch.float32), got.abs().flatten(1).amax(dim=1))
    check_rows(f"xkv E={E} L={L}, q x 2^12, x x 2^-9", got, torch.cat([q, x, x], dim=1), E, 1)


# ---------------------------------------------------------------- 3. the block
_BLOCK = {}


def _block_reference():
    """Inputs, the fp64 module and torch fp32 on the CPU for x4 [2, 256, 32, 32], once."""
    if not _BLOCK:
        E, B, H, W = 256, 2, 32, 32
        torch.manual_seed(11)
        m = torch.nn.MultiheadAttention(E, 1, batch_first=True)
        g = torch.Generator().manual_seed(12)
        with torch.no_grad():
            m.in_proj_bias.copy_(0.5 * torch.randn(3 * E, generator=g))
            m.out_proj.bias.copy_(0.5 * torch.randn(E, generator=g))
        t = {"m": m, "x": torch.randn(B, E, H, W, generator=g), "res2": torch.randn(B, E, H, W, generator=g)}
        for dtype, key in ((torch.float64, "f64"), (torch.float32, "f32")):
            md = torch.nn.MultiheadAttention(E, 1, batch_first=True).to(dtype)
            md.load_state_dict({k: v.to(dtype) for k, v in m.state_dict().items()})
            tok = t["x"].to(dtype).flatten(2).transpose(1, 2)
            with torch.no_grad():
                y = md(tok, tok, tok, need_weights=False)[0].transpose(1, 2).reshape(B, E, H, W)
            t[key] = (y + t["x"].to(dtype)) + t["res2"].to(dtype)
        _BLOCK.update(t)
    return _BLOCK


def test_block_folded_vs_unfolded_vs_fp64(dev):
    from diffsci_amd import ops
    from diffsci_amd.models.nets import runtime
    t = _block_reference()
    m, E = t["m"], 256
    x, res2 = t["x"].to(dev), t["res2"].to(dev)
    B, _, H, W = x.shape
    L = H * W
    w_in, w_out = m.in_proj_weight.detach(), m.out_proj.weight.detach()
    b_in, b_out = m.in_proj_bias.detach(), m.out_proj.bias.detach()
    p_in = ops.pack_conv(w_in.reshape(3 * E, E, 1, 1).to(dev), "fp16x3")
    p_out = ops.pack_conv(w_out.reshape(E, E, 1, 1).to(dev), "fp16x3")
    M, c, Wp, bp = runtime.fold_attention_weights(w_in, b_in, w_out, b_out)
    folded = runtime.FoldedAttention(ops.pack_conv(M.float().reshape(E, E, 1, 1).to(dev), "fp16x3"), c.float().to(dev),
                                     ops.pack_conv(Wp.float().reshape(E, E, 1, 1).to(dev), "fp16x3"), bp.float().to(dev))
    assert runtime.attention_folds(folded, E, L, 1, "fp16x3", False)

    def run(bundle):
        ws = runtime.Workspace()
        am = runtime.AmaxArena(ws, B, dev)
        stats = torch.full((B, E, ops.conv_tile_count(H, W), 4), float("nan"), device=dev)
        amax = ops.amax_new(B, dev)
        y = runtime.attention(x, p_in, b_in.to(dev), p_out, b_out.to(dev), E=E, heads=1, precision="fp16x3", ws=ws, am=am,
                              res1=x, res2=res2, tile_stats=stats, out_amax=amax, folded=bundle)
        am.release()
        return y, stats, amax, ws

    y_f, stats, amax, ws = run(folded)
    y_u, _, _, ws_u = run(None)
    assert ((B, E, H, W), str(dev)) in ws.free and ((B, 3 * E, H, W), str(dev)) not in ws.free      # qkv shrank to E channels
    assert ((B, 3 * E, H, W), str(dev)) in ws_u.free
    err = lambda y: float((y.double().cpu() - t["f64"]).abs().max())
    e_f, e_u, e_t = err(y_f), err(y_u), float((t["f32"].double() - t["f64"]).abs().max())
    print(f"[fold block] max-abs vs the fp64 module on values up to {float(t['f64'].abs().max()):.2f}: folded {e_f:.3e}, "
          f"unfolded {e_u:.3e}, torch fp32 on the CPU {e_t:.3e}")
    assert e_f <= 2 * max(e_u, e_t)
    # what the out-projection's epilogue left describes the folded output itself
    assert torch.equal(amax, ops.absmax_rows(y_f))
    K, S, Q, n = stats.cpu().double().unbind(-1)                   # per (channel, tile): shift, sum (y - K), sum (y - K)^2, count
    assert torch.equal(n.sum(-1), torch.full((B, E), float(L), dtype=torch.float64))
    yd = y_f.double().cpu()
    # fp32 accumulation of L terms: |error| <= L * 2^-24 * sum |terms|
    assert ((n * K + S).sum(-1) - yd.sum(dim=(2, 3))).abs().le(L * 2.0 ** -24 * yd.abs().sum(dim=(2, 3))).all()


# ---------------------------------------------------------------- 4. the network
def test_network_folded_vs_unfolded(dev):
    """PUNetG-64 on [2, 1, 128, 128]: the bottleneck is [2, 256, 32, 32], the smallest shape on the folded route."""
    import diffsci_amd.models as M
    torch.manual_seed(21)
    net = M.PUNetG(M.PUNetGConfig(model_channels=64)).to(dev).eval()
    g = torch.Generator().manual_seed(22)
    with torch.no_grad():
        for a in net.attn_block:                                   # torch initialises these biases to zero
            a.mhattn.in_proj_bias.copy_(0.5 * torch.randn(a.mhattn.in_proj_bias.shape, generator=g))
            a.mhattn.out_proj.bias.copy_(0.5 * torch.randn(a.mhattn.out_proj.bias.shape, generator=g))
    assert len(net.attn_block) > 0 and net.attn_fold is True
    x = torch.randn(2, 1, 128, 128, generator=g).to(dev)
    tt = (torch.rand(2, generator=g) + 0.1).to(dev)
    with torch.inference_mode():
        shifts = net.time_shifts(net.embed_time(tt))
        eager = net.forward_with_shifts(x, shifts).clone()
        assert "_attn_folded" in net.__dict__                      # the route was taken
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            y = net.forward_with_shifts(x, shifts)
        graph.replay()
        torch.cuda.synchronize()
        captured = y.clone()
        graph.replay()
        torch.cuda.synchronize()
        replayed = y.clone()
        net.attn_fold = False
        off = net.forward_with_shifts(x, shifts).clone()
        net.conv_precision = "fp32"
        exact = net.forward_with_shifts(x, shifts).clone()
    assert bool(torch.isfinite(eager).all()) and float(eager.abs().max()) > 0
    assert _same(captured, eager) and _same(replayed, eager)
    d_fold, d_prec = float((eager - off).abs().max()), float((off - exact).abs().max())
    print(f"[fold net] max |folded - unfolded| {d_fold:.3e}; max |fp16x3 - fp32 convolutions| of the unfolded network {d_prec:.3e}; "
          f"max |y| {float(off.abs().max()):.3f}")
    assert not _same(eager, off)                                   # two routes, not one
    assert d_fold <= 2 * d_prec
