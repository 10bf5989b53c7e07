"""A recording stand-in for libdiffsci_hip.so and the table of valid ops.py calls whose launch sequences are pinned
(tests/golden/abi_trace.json, written by tools/make_abi_trace_golden.py from the PARENT commit's ops.py).

Every `_native._PROTOS` entry that returns c_int and takes the stream last (the ds_graph_* entries aside) is a launch: the
stand-in records (name, arguments) and returns 0.  Size and support queries go to the real library, which loads without a GPU.
A pointer is recorded as [label of the named tensor or pool buffer it falls in, byte offset], or "fresh" for memory the wrapper
allocated itself -- so `film + 4C`, the chunks of `mod`, `s_in[1 + kz]` and `am + 4 (1 + kz)` are pinned too.  All tensors live
on the host: nothing here may run a kernel, which is the point -- the gap tests hand the wrappers buffers a kernel would overrun.
"""
import ctypes

import torch

from diffsci_amd import _native as N


def is_launch(name):
    res, args = N._PROTOS[name]
    return res is ctypes.c_int and bool(args) and args[-1] is ctypes.c_void_p and not name.startswith("ds_graph_")


LAUNCHES = sorted(n for n in N._PROTOS if is_launch(n))


class Recorder:
    """Stands where N.lib() stood."""

    def __init__(self, real):
        self._real, self.calls, self._regions, self._keep = real, [], [], []

    def name(self, label, t):
        """Label the storage of tensor t (kept alive, so no later allocation can land in it)."""
        self._keep.append(t)
        self._regions.append((t.data_ptr(), t.data_ptr() + max(t.numel() * t.element_size(), 1), label))
        return t

    def _pointer(self, p):
        if p is None:
            return None
        for lo, hi, label in self._regions:
            if lo <= p < hi:
                return [label, p - lo]
        return "fresh"

    def _arg(self, v, ctype):
        if ctype is ctypes.c_void_p:
            return self._pointer(v)
        if ctype is ctypes.POINTER(N.EvalCoef):
            k = v._obj
            return [getattr(k, f) for f, _ in N.EvalCoef._fields_]
        return float(v) if ctype is ctypes.c_float else int(v)

    def __getattr__(self, name):
        if name.startswith("_") or name not in N._PROTOS:
            raise AttributeError(name)
        if not is_launch(name):
            return getattr(self._real, name)
        types = N._PROTOS[name][1]

        def launch(*args):
            assert len(args) == len(types), (name, len(args), len(types))
            self.calls.append([name] + [self._arg(v, t) for v, t in zip(args, types)])
            return 0
        return launch


class Pool:
    """The buffer pool of the traced calls: every take is a new buffer labelled by take order."""

    def __init__(self, rec):
        self.rec, self.n, self.out = rec, 0, []

    def take(self, shape, device):
        t = self.rec.name(f"pool{self.n}", torch.empty(tuple(shape), dtype=torch.float32, device=device))
        self.n += 1
        self.out.append(t.data_ptr())
        return t

    def give(self, t):
        self.out.remove(t.data_ptr())


class Ctx:
    """What a case builds its arguments from: named tensors with fixed contents, a pool, the ops module under trace."""

    def __init__(self, ops, rec):
        self.ops, self.rec = ops, rec
        self.pools = []

    def f(self, label, *shape):
        n = 1
        for s in shape:
            n *= s
        t = ((torch.arange(n, dtype=torch.float32) * 37 % 101) - 50) / 64
        return self.rec.name(label, t.reshape(shape).contiguous())

    def i(self, label, n):
        return self.rec.name(label, torch.zeros(n, dtype=torch.int32))

    def pool(self):
        self.pools.append(Pool(self.rec))
        return self.pools[-1]

    def pack(self, label, w, *args, **kw):
        """ops.pack_conv with the packed streams labelled (label, label.up, label.sub<i>)."""
        pw = self.ops.pack_conv(w, *args, **kw)
        for tag, p in [("", pw)] + [(f".sub{i}", s[2]) for i, s in enumerate(pw.subs or [])]:
            if p.data is not None:
                self.rec.name(label + tag, p.data)
            if p.up is not None:
                self.rec.name(label + tag + ".up", p.up)
        return pw

    def pack3d(self, label, w, upsampled=False):
        return [self.pack(f"{label}.z{kz}", w[:, :, kz].contiguous(), "fp16x3", upsampled=upsampled and w.shape[2] == 3)
                for kz in range(w.shape[2])]


B = 2


def _steps(c):
    o = c.ops
    x, f, fu, out, eps = (c.f(n, B, 3, 8, 8) for n in ("x", "f", "fu", "out", "eps"))
    xin2 = c.f("xin2", 2 * B, 3, 8, 8)
    state = c.rec.name("state", torch.zeros(2, dtype=torch.int64))
    k, k2 = o.EvalCoef(), o.EvalCoef()
    k.c_out, k.guidance, k.xin_copies, k2.xin_copies = 0.5, 2.0, 1, 2
    o.scale(x, 0.5)
    o.scale(x, 0.5, out=c.f("flat", x.numel()))                                    # a flat buffer of the same size
    o.add(x, f, out=out)
    o.mask_blend(x, f, c.f("mask", 3, 8, 8), out=out)
    o.axpby(x, 2.0)
    o.axpby(x, 2.0, f, 0.5, out=out)
    o.div_scalar(x, 3.0, out=out)
    o.batchnorm_eval(x, c.f("mean", 3), c.f("var", 3), c.f("bw", 3), c.f("bb", 3), inverse=True, out=out)
    o.batchnorm_eval(x, c.f("mean1", 1), c.f("var1", 1))
    o.lerp_stack(x, f, 3)
    o.drift(x, f, k)
    o.drift(x, f, k, fu, out=out)
    o.score(x, f, k, fu, out=out)
    o.philox_normal(state, 8, (B, 3, 8, 8), out=out)
    o.euler(x, f, k, 0.1, x_out=out)
    o.euler(x, f, k, 0.1, fu=fu, x_out=out, xin_out=c.f("xin", B, 3, 8, 8), c_in_next=0.7, noise_coef=0.3, sqrt_abs_dt=0.2,
            philox=(state, 16))
    o.euler(x, f, k, 0.1, x_out=out, eps=eps, noise_coef=0.3, sqrt_abs_dt=0.2)
    o.heun(x, f, k, fu, k2, 0.1, x_out=out)
    o.heun(x, f, k, fu, k2, 0.1, f1u=eps, f2u=eps, x_out=out, xin_out=xin2, c_in_next=0.7)
    o.churn(x, eps, 0.4, out)
    o.churn(x, None, 0.4, out, xin_out=xin2, c_in=0.9, philox=(state, 4), ratio=0.8, scale=1.5, xin_copies=2)
    o.denoiser(x, f, c.f("c_out", B), c.f("c_skip", B), fu=fu, guidance=1.5, out=out)
    o.inorm_silu(x, c.f("nw", 3), c.f("nb", 3), 1, out=out)
    o.tanh(x, out=out)


def _amax(c):
    o = c.ops
    x = c.f("x", B, 4, 8, 8)
    am = c.i("am", B)
    o.amax_zero(am)
    o.absmax_rows(x)
    o.absmax_rows(x[:, 1:3], out=am)
    o.absmax_rows(x, 4, out=c.i("am4", 4))
    o.absmax_channels(x, am, c.i("scratch", B * 4), c.i("flag", 1), c.f("wmax", 4))
    arena = c.rec.name("arena", torch.zeros(3, B, dtype=torch.int32))
    o.input_amax(arena, 1, x, c.i("flag2", 1), None)
    o.amax_merge(am, c.i("a", B), c.i("b", B))
    o.amax_merge(am, c.i("a2", B))


def _conv2d(c):
    o, M = c.ops, N
    C = 8
    x = c.f("x", B, C, 8, 8)
    w3, w1, w5 = c.f("w3", C, C, 3, 3), c.f("w1", 64, C, 1, 1), c.f("w5", C, C, 5, 5)
    bias, res1, res2 = c.f("bias", C), c.f("res1", B, C, 8, 8), c.f("res2", B, C, 8, 8)
    out = c.f("out", B, C, 8, 8)
    ts = c.f("ts", B, C, o.conv_tile_count(8, 8), 4)
    h3 = c.pack("h3", w3, "fp16x3")
    am, om = c.i("in_amax", B), c.i("out_amax", B)
    o.conv(x, h3, bias=bias, shift=c.f("shift1", 1, C), res1=res1, res2=res2, tile_stats=ts, out=out)          # in_amax None
    o.conv(x, h3, shift=c.f("shiftB", B, C), in_amax=am, out_amax=om, out=out, circular=True)
    o.conv(x, h3, prenorm=c.f("prenorm", B, o.table_channels(C), 4), out=out)
    o.conv(x, h3, in_amax=o.NORMALISED)
    half = c.f("half", B, C, 4, 4)
    o.conv(x, h3, load_mode=M.DS_LOAD_MAXPOOL2, in_amax=am, out=half)
    o.conv(half, h3, load_mode=M.DS_LOAD_UPSAMPLE2, in_amax=am, out=out)                    # no parity kernels: ds_conv2d_h3
    o.conv(x, h3, res1=half, res1_upsampled=True, in_amax=am, out=out)
    x16, out32 = c.f("x16", B, C, 16, 16), c.f("out32", B, C, 32, 32)
    h3u = c.pack("h3u", w3, "fp16x3", upsampled=True)
    assert N.lib().ds_conv2d_h3_up_supported(16, 16)
    o.conv(x16, h3u, bias=bias, load_mode=M.DS_LOAD_UPSAMPLE2, in_amax=c.i("am16", B), out=out32,
           tile_stats=c.f("ts32", B, C, o.conv_tile_count(32, 32), 4), res1=x16, res1_upsampled=True, circular=True)
    o.conv(x, c.pack("h5", w5, "fp16x3"), bias=bias, shift=c.f("shift5", B, C), res1=res1, tile_stats=ts, out=out, out_amax=om)
    o.conv(x, c.pack("h5b", w5, "fp16x3"), in_amax=am, out=out)
    p1 = c.pack("p1", w1, "fp16x3")
    o.conv(x, p1, bias=c.f("bias64", 64), load_mode=M.DS_LOAD_AVGPOOL2, in_amax=am, out=c.f("out1", B, 64, 4, 4))
    w1b = c.f("w1b", 128, C, 1, 1)
    o.conv(x, c.pack("p1b", w1b, "fp16x3"), in_amax=am, out_amax=c.i("om2", 2 * B), amax_split=64)
    o.conv(x, c.pack("x6", w3, "bf16x6"), bias=bias, shift=c.f("shift6", B, C), res1=res1, out=out)
    o.conv(x, c.pack("f32", w3, "fp32"), bias=bias, load_mode=M.DS_LOAD_MAXPOOL2, out=half)
    o.conv(x, c.pack("f32_1", c.f("w1c", C, C, 1, 1), "fp32"), res2=res2, out=out)
    o.conv_direct(x, c.f("wd", 2, C, 3, 3), c.f("bd", 2), circular=True)
    o.conv_direct(x, c.f("wd2", 2, C, 3, 3), out=c.f("outd", B, 2, 8, 8))


def _conv_s2(c):
    o = c.ops
    x, x3 = c.f("x", B, 8, 8, 8), c.f("x3", B, 8, 4, 8, 8)
    w, wt = c.f("w", 8, 8, 3, 3), c.f("wt", 2, 8, 3, 3)
    pw = o.pack_conv_s2(w)
    c.rec.name("pw", pw.data)
    o.conv_s2(x, pw, bias=c.f("bias", 8), res1=c.f("res", B, 8, 4, 4), out_amax=c.i("om", B))
    o.conv_s2(x, pw, in_amax=c.i("am", B), out=c.f("out", B, 8, 4, 4))
    pd = o.pack_conv_s2(wt)
    c.rec.name("pd", pd.data)
    o.conv_s2(x, pd, bias=c.f("bias2", 2), out_amax=c.i("om2", B))
    w3, w3t = c.f("w3", 8, 8, 3, 3, 3), c.f("w3t", 2, 8, 3, 3, 3)
    pk = o.pack_conv3d_s2(w3)
    for kz, p in enumerate(pk):
        c.rec.name(f"pk{kz}", p.data)
    o.conv3d_s2(x3, pk, bias=c.f("b3", 8), res1=c.f("r3", B, 8, 2, 4, 4), out=c.f("o3", B, 8, 2, 4, 4), ws=c.pool())
    o.conv3d_s2(x3, pk)
    pt = o.pack_conv3d_s2(w3t)
    c.rec.name("pt", pt.data)
    o.conv3d_s2(x3, pt, bias=c.f("b3t", 2))


def _volumes(c):
    o, M = c.ops, N
    C = 8
    x = c.f("x", B, C, 4, 8, 8)
    w = c.f("w", C, C, 3, 3, 3)
    bias, shiftB, shift1 = c.f("bias", C), c.f("shiftB", B, C), c.f("shift1", 1, C)
    res1, res2, out = c.f("res1", B, C, 4, 8, 8), c.f("res2", B, C, 4, 8, 8), c.f("out", B, C, 4, 8, 8)
    half, dbl = c.f("half", B, C, 2, 4, 4), c.f("dbl", B, C, 8, 16, 16)
    o.conv3d(x, w, bias, shiftB, res1, res2, out=out)
    o.conv3d(x, w, shift=shift1, load_mode=M.DS_LOAD_MAXPOOL2, out=half)
    o.conv3d(x, w, load_mode=M.DS_LOAD_UPSAMPLE2, circular=True, out=dbl)
    pk = c.pack3d("pk", w)
    st = c.f("st", B, C, o.volume_stat_tiles(4, 64), 4)
    o.conv3d_mfma(x, pk, bias, shiftB, res1, res2, out=out, ws=c.pool(), out_stats=st)
    o.conv3d_mfma(x, pk, bias, shiftB)
    o.conv3d_mfma(x, pk, shift=shift1, in_amax=o.NORMALISED, out=out, ws=c.pool())
    o.conv3d_mfma(x, pk, load_mode=M.DS_LOAD_MAXPOOL2, out=half, ws=c.pool())
    o.conv3d_mfma(x, c.pack3d("pku", w, upsampled=True), shift=shiftB, load_mode=M.DS_LOAD_UPSAMPLE2, out=dbl, ws=c.pool())
    o.conv3d_mfma(x, pk, circular=True, out=out, ws=c.pool())
    o.conv3d_mfma(x, c.pack3d("pk5", c.f("w5", C, C, 5, 5, 5)), bias, shiftB, circular=True, out=out, ws=c.pool())
    o.conv3d_mfma(x, c.pack3d("pk1", c.f("w1", C, C, 1, 1, 1)), out=out)
    tab1 = c.f("tab1", B, o.table_channels(C), 4)
    pk2 = c.pack3d("pk2", c.f("wb", C, C, 3, 3, 3))
    nw, nb = c.f("nw", C), c.f("nb", C)
    for circ in (False, True):
        o.resblock3d_fused(x, tab1, pk, bias, shiftB, pk2, bias, nw, nb, 0, res2=res2, out=out, out_stats=st, ws=c.pool(),
                           circular=circ)
        o.resblock3d_fused(x, tab1, pk, bias, shift1 if circ else shiftB, pk2, None, nw, nb, 1, circular=circ)
    o.avgpool3d(x)
    o.upsample3d(x)
    f4 = c.f("f4", B, C, 8, 8)
    for t in (f4, x):
        o.avgpool_f(t, 2)
        o.upsample_f(t, 3)
        o.maxpool_f(t, 2)
        o.cornerpool_f(t, 2)
    o.cornerpool_f(f4[:1].contiguous(), 4, te=c.f("te", B, C), out_amax=c.i("om", B))
    o.cornerpool_f(x, 2, te=c.f("te1", 1, C), out=c.f("outc", B, C, 2, 4, 4))
    o.box_copy3d(x, (-1, 2, 3), c.f("dst", B, C, 6, 8, 8), (1, 0, 2), (5, 8, 6))
    m = c.f("moments", B, 4, 8, 8)
    o.posterior_sample(m, eps=c.f("eps", B, 2, 8, 8), clamp=(-30.0, 20.0))
    o.posterior_sample(m, eps=c.f("eps2", B, 2, 8, 8), out=c.f("z", B, 2, 8, 8))


def _norms(c):
    o = c.ops
    C = 8
    x = c.f("x", B, C, 8, 8)
    w, b = c.f("w", C), c.f("b", C)
    film1, filmB = c.f("film1", 1, 2 * C), c.f("filmB", B, 2 * C)
    st = o.gnorm1_stats(x, 0)
    stats = c.f("stats", B, 2)
    o.gnorm1_stats(x, 1, stats=stats, workspace=c.f("gws", N.lib().ds_gnorm1_workspace_bytes(B) // 4))
    o.gnorm1_apply(x, st, w, b, 0)
    o.gnorm1_apply(x, stats, w, b, 0, film=film1, out=c.f("out", B, C, 8, 8))
    o.gnorm1_apply(x, stats, w, b, 1, pool=True, film=filmB, out=c.f("outp", B, C, 4, 4))
    o.gnorm1_apply(x, None, None, None, 2, pool=True)
    o.gnorm1_apply_poolf(x, stats, w, b, 0, 4, film=filmB)
    o.gnorm1_apply_poolf(x, stats, w, b, 1, 2, film=film1, out=c.f("outf", B, C, 4, 4))
    ta = c.f("ta", B, C, o.conv_tile_count(8, 8), 4)
    tb = c.f("tb", B, 4, o.conv_tile_count(8, 8), 4)
    o.inorm_table(ta, w, b, 0, 64)
    o.inorm_table(ta, None, None, 1, 64, out=c.f("tab", B, o.table_channels(C), 4))
    o.gnorm1_table(ta, w, b, 0, 64, film=filmB)
    o.gnorm1_table(ta, c.f("w12", 12), c.f("b12", 12), 1, 64, stats_b=tb, film=c.f("film12", 1, 24),
                   out=c.f("tab12", B, o.table_channels(12), 4))
    o.gnorm1_stats_tiles(ta, 0, 64)
    o.gnorm1_stats_tiles(ta, 1, 64, stats_b=tb, stats=stats)
    o.gnorm1_apply_images(x, stats, w, b, 0, film=film1)
    o.gnorm1_apply_images(x, stats, w, b, 1, pool=True, film=filmB, out=c.f("imgp", o.conv_images_floats(B, C, 4, 4)))
    img = o.inorm_silu_images(x, w, b, 0, out=c.f("img", o.conv_images_floats(B, C, 8, 8)))
    o.inorm_silu_images(x, None, None, 1)
    o.table_apply_images(x, c.f("table", B, o.table_channels(C), 4))
    o.table_apply_images(x, c.f("table2", B, o.table_channels(C), 4), out=img)
    pw = c.pack("pw", c.f("cw", C, C, 3, 3), "fp16x3", upsampled=True)
    bias, om = c.f("bias", C), c.i("om", B)
    o.conv_img(img, pw, B, C, 8, 8, bias=bias, shift=filmB[:, :C].contiguous(), res1=x, res2=x, tile_stats=ta, out_amax=om)
    o.conv_img(img, pw, B, C, 8, 8, shift=c.f("shift1", 1, C), res1=c.f("r4", B, C, 4, 4), res1_upsampled=True,
               out=c.f("outi", B, C, 8, 8))
    img16 = c.f("img16", o.conv_images_floats(B, C, 16, 16))
    assert o.conv_up_img_supported(pw, 16, 16)
    o.conv_up_img(img16, pw, B, C, 16, 16, bias=bias, shift=c.f("shiftB", B, C), res1=c.f("r32", B, C, 32, 32),
                  tile_stats=c.f("ts32", B, C, o.conv_tile_count(32, 32), 4), out_amax=om)
    o.conv_up_img(img16, pw, B, C, 16, 16, out=c.f("out32", B, C, 32, 32))
    v = c.f("v", B, C, 2, 4, 4)
    gs = o.groupnorm_stats(v, 4)
    o.groupnorm_stats(v, 2, stats=c.f("gs2", B, 2, 2), workspace=c.f("gws2", N.lib().ds_gnorm1_workspace_bytes(B * 2) // 4))
    o.groupnorm_apply(v, gs, w, b, 4)
    o.groupnorm_apply(v, gs, None, None, 4, act=True, out=c.f("gout", B, C, 2, 4, 4), out_amax=om)
    o.groupnorm_stats_tiles(ta, 4, 64)
    o.groupnorm_stats_tiles(ta, 2, 64, stats=c.f("gs3", B, 2, 2))
    o.groupnorm_table(w, b, 4, 64, tile_stats=ta)
    o.groupnorm_table(w, b, 2, 64, stats=c.f("gs4", B, 2, 2), out=c.f("gtab", B, o.table_channels(C), 4))


def _small(c):
    o = c.ops
    a, b4 = c.f("a", B, 3, 8, 8), c.f("b4", B, 5, 8, 8)
    o.concat2(a, b4)
    o.concat2(c.f("a5", B, 3, 2, 4, 4), c.f("b5", B, 1, 2, 4, 4), out=c.f("cat5", B, 4, 2, 4, 4))
    h = c.f("h", B, 16)
    o.add_act(h, act=1)
    o.add_act(h, c.f("add1", 16), act=2, out=c.f("hout", B, 16))
    o.add_act(h, c.f("addB", B, 16))
    o.linear(h, c.f("lw", 24, 16), c.f("lb", 24), act=1)
    o.linear(h, c.f("lw2", 24, 16), out=c.f("lout", B, 24))
    t, W = c.f("t", B), c.f("W", 8)
    o.fourier_features(t, W)
    o.fourier_features(t, W, add=c.f("ye", B, 16), out=c.f("ff", B, 16))
    o.fourier_features(t, W, add=c.f("ye1", 16))
    o.fourier_channels(a, c.f("Wc", 3, 4))
    o.fourier_channels(c.f("a5b", B, 3, 2, 4, 4), c.f("Wc2", 3, 4), out=c.f("fc", B, 8, 2, 4, 4))


def _attention(c):
    o = c.ops
    for name, E, L, prec, heads, kw in (
            ("mfma", 32, 32, "fp32", 1, {}),                                   # ds_attention
            ("generic", 32, 33, "fp16x3", 1, {"out_amax": True}),              # ds_attention_generic
            ("h3", 32, 64, "fp16x3", 1, {}),                                   # ds_attention_h3, in_amax reduced here
            ("h3_rows", 32, 64, "fp16x3", 1, {"in_amax": True, "out_amax": True, "out": True}),
            ("h3_norm", 32, 64, "fp16x3", 1, {"in_amax": o.NORMALISED}),
            ("h3_ws", 32, 2048, "fp16x3", 1, {"in_amax": True}),               # ds_attention_h3_ws, workspace allocated
            ("h3_ws_given", 32, 2048, "fp16x3", 1, {"in_amax": True, "workspace": True, "out": True}),
            ("heads", 64, 64, "fp16x3", 2, {"out_amax": True}),                # ds_attention_h3_heads without images
            ("heads_ws", 64, 2048, "fp16x3", 2, {"in_amax": True, "workspace": True, "out": True}),
            ("heads_ws_fresh", 64, 2048, "fp16x3", 2, {"in_amax": o.NORMALISED}),
            ("heads_generic", 48, 64, "fp16x3", 2, {"out_amax": True}),        # ds_attention_heads_generic (width 24)
            ("heads_fp32", 64, 64, "fp32", 2, {})):
        qkv = c.f(f"{name}.qkv", B, 3 * E, L)
        if kw.get("in_amax") is True:
            kw["in_amax"] = c.i(f"{name}.in_amax", 2 * B)
        if kw.get("out_amax"):
            kw["out_amax"] = c.i(f"{name}.out_amax", B)
        if kw.get("out"):
            kw["out"] = c.f(f"{name}.out", B, E, L)
        if kw.get("workspace"):
            kw["workspace"] = c.f(f"{name}.ws", o.attention_workspace_floats(B, E, L, prec, heads) + 3)
        o.attention(qkv, E, precision=prec, heads=heads, **kw)


def _tokens(c):
    o = c.ops
    E, L = 16, 12
    x, y = c.f("x", B, E, L), c.f("y", B, E, L)
    w, b = c.f("w", E), c.f("b", E)
    mod1, modB, modT = c.f("mod1", 1, 6 * E), c.f("modB", B, 6 * E), c.f("modT", 5, 6 * E)
    o.token_l2_normalize(c.f("q", B, 3 * E, L), E, E, gain=4.0)
    o.token_layernorm(x, w, b)
    o.token_layernorm(x, None, None, mod=mod1, out=c.f("out", B, E, L), out_amax=c.i("om", B))
    o.token_layernorm(x, w, b, mod=modB, shift_chunk=3, scale_chunk=4)
    o.token_layernorm(x, w, b, mod=modT, shift_chunk=0, scale_chunk=1, row=3)
    o.token_gate(x, y, modB, chunk=2)
    o.token_gate(x, y, modT, chunk=5, row=4, out=x)
    o.token_gate(x, y, mod1, chunk=0)
    o.silu_amax(x)
    o.silu_amax(x, out=x, out_amax=c.i("om2", B))
    img = c.f("img", B, 3, 8, 12)
    o.patch_embed(img, c.f("pe", E, 3 * 4), c.f("peb", E), 2)
    o.patch_embed(img, c.f("pe4", E, 3 * 16), None, 4, out=c.f("tok", B, E, 6))
    tok = c.f("tok24", B, E, 24)
    o.patch_unembed(tok, c.f("pu", 12, E), c.f("pub", 12), 2, (B, 3, 8, 12))
    o.patch_unembed(tok, c.f("pu2", 12, E), None, 2, (B, 3, 8, 12), out=c.f("img_out", B, 3, 8, 12))
    o.pack_conv_weight(c.f("pcw", 8, 8, 3, 3))


CASES = {"steps": _steps, "amax": _amax, "conv2d": _conv2d, "conv_s2": _conv_s2, "volumes": _volumes, "norms": _norms,
         "small": _small, "attention": _attention, "tokens": _tokens}


def traced(ops, monkeypatch_setattr, fn):
    """Run fn(ctx) with `ops` launching into a Recorder -> (recorder, ctx).  monkeypatch_setattr(target, name, value) patches;
    the caller patches the device test(s) of `ops` itself (they differ between the parent and the branch)."""
    rec = Recorder(N.lib())
    monkeypatch_setattr(N, "lib", lambda: rec)
    monkeypatch_setattr(ops, "_stream", lambda: 0)
    ctx = Ctx(ops, rec)
    fn(ctx)
    return rec, ctx


def trace_of(ops, monkeypatch_setattr, fn):
    """The pinned record of one case: its launches, and per pool how many buffers were taken and how many never given back."""
    rec, ctx = traced(ops, monkeypatch_setattr, fn)
    return {"calls": rec.calls, "pools": [[p.n, len(p.out)] for p in ctx.pools]}
