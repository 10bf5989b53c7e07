"""Pin the CPU oracle (oracle/) against golden vectors produced by the real reference.

These tests are the oracle's licence: bit-for-bit agreement (fp32 and fp64) with
outputs of /root/reference generated in the build container.  They run on CPU.
"""
import pytest
import torch

from oracle import karras_ref as K
from oracle import mlp_ref, punetg_ref
from tests.golden_util import load, rel_l2, same_cpu_arithmetic

torch.set_num_threads(8)

SAME_ISA = None


def _same_isa():
    return same_cpu_arithmetic()


def assert_exact_or_ulp(got, want, what):
    """Bit-exact on the ISA the fixtures were made on; <= 2 ulp elsewhere (torch's CPU
    pow/log/sin kernels are ISA-dependent in the last place)."""
    if _same_isa():
        assert torch.equal(got, want), f"{what}: not bit-exact (max abs {float((got-want).abs().max())})"
    else:
        torch.testing.assert_close(got, want, rtol=3e-7, atol=0)


def assert_exact_or_rel(got, want, what, rel):
    """Network-sized tensors: bit-exact on the fixtures' ISA, rel-L2 bound elsewhere."""
    if _same_isa() and got.dtype == torch.float32:
        assert torch.equal(got, want), f"{what}: not bit-exact (rel-L2 {rel_l2(got, want):.3e})"
    else:
        assert rel_l2(got, want) < rel, what


@pytest.mark.parametrize("n", [2, 5, 10, 18, 50, 100, 256])
def test_sigma_grid(n):
    v, _ = load("schedule")
    assert_exact_or_ulp(K.edm_sigma_grid(n + 1), v[f"steps_{n}"], f"sigma grid n={n}")


def test_sigma_grid_shape_and_ends():
    g = K.edm_sigma_grid(51)
    assert g.shape == (51,) and g.dtype == torch.float32
    # (80**(1/7))**7 is NOT 80 in fp32 -- the reference's grid starts 1 ulp-ish above it
    assert abs(g[0].item() - 80.0) < 1e-4 and g[-1].item() == 0.0
    assert abs(g[-2].item() - 0.002) < 1e-8
    assert (torch.diff(g) < 0).all()


@pytest.mark.parametrize("n", [19, 51])
def test_step_from_time_integer_path(n):
    v, _ = load("schedule")
    got = K.edm_step_from_time(v["step_from_time_t"], n)
    assert got.dtype == torch.int32
    assert torch.equal(got, v[f"step_from_time_{n}"])


@pytest.mark.parametrize("B", [1, 4, 64])
@pytest.mark.parametrize("n", [18, 50])
def test_precond_scalars(B, n):
    v, _ = load("schedule")
    grid = v[f"steps_{n}"][:-1]
    want = v[f"precond_B{B}_N{n}"]
    for i, ti in enumerate(grid):
        sig = ti * torch.ones(B)
        cs, co, ci, cn = K.edm_precond(sig)
        got = torch.stack([cs[0], co[0], ci[0], cn[0], cs[-1], co[-1], ci[-1], cn[-1]])
        assert_exact_or_ulp(got, want[i], f"precond row {i}")


@pytest.mark.parametrize("target", ["zero", "gauss"])
@pytest.mark.parametrize("integ", ["heun", "euler"])
def test_analytic_trajectories(target, integ):
    v, _ = load("toy_analytic")
    fn = K.point_target_score(0.0) if target == "zero" else K.gaussian_target_score(0.7)
    hist = K.propagate_backward(v["x"] * 80.0, fn, 18, integrator=integ, record_history=True)
    assert_exact_or_ulp(hist, v[f"{target}_{integ}_N18"], f"{target}/{integ}")


def test_reference_own_known_answer():
    """tests/test_karras_on_toy_dataset.py:18-27 of the reference: point mass at 0 -> samples ~ 0."""
    torch.manual_seed(0)
    x = torch.randn(100, 1)
    hist = K.propagate_backward(x, K.point_target_score(0.0), 100, record_history=True)
    assert hist.shape == (101, 100, 1)
    assert torch.isclose(hist[0], x).all()
    assert torch.isclose(hist[-1], torch.tensor(0.0), rtol=1e-2, atol=1e-2).all()


def test_heun_closed_form_gain():
    """N(0,s^2) target => x_N = x_0 * prod g_i."""
    grid = K.edm_sigma_grid(19)
    x = torch.tensor([[1.0], [-2.5]], dtype=torch.float64) * 80.0
    out = K.propagate_backward(x, K.gaussian_target_score(0.7), 18, sigma_grid=grid)
    g = K.heun_gain_product(grid, 0.7)
    torch.testing.assert_close(out, x * g, rtol=1e-12, atol=0)


def test_mlp_cfg1_trajectories():
    v, sd = load("mlp_cfg1")
    net = mlp_ref.make_net(sd)
    for integ in ("heun", "euler"):
        hist = K.propagate_white_noise(net, v["white_noise"], 18, integrator=integ, record_history=True)
        assert_exact_or_ulp(hist, v[f"hist_{integ}_N18_f32"], f"mlp {integ}")
    hist = K.propagate_white_noise(net, v["white_noise"], 18, integrator="karras",
                                   record_history=True, eps=v["eps_karras_N18"])
    assert_exact_or_ulp(hist, v["hist_karras_N18_f32"], "mlp karras")
    hist = K.propagate_white_noise(net, v["white_noise"], 18, integrator="euler-maruyama",
                                   record_history=True, eps=v["eps_em_N18"],
                                   langevin_const=float(v["em_langevin_const"]))
    assert_exact_or_ulp(hist, v["hist_em_N18_f32"], "mlp euler-maruyama")
    sd64 = {k: t.double() for k, t in sd.items()}
    hist = K.propagate_white_noise(mlp_ref.make_net(sd64), v["white_noise"].double(), 18,
                                   record_history=True)
    assert_exact_or_ulp(hist, v["hist_heun_N18_f64"], "mlp heun fp64")


def test_punetg_layers_and_forward():
    v, sd = load("punetg8_forward")
    cfg = punetg_ref.default_config(model_channels=8)
    import torch.nn.functional as F
    with torch.inference_mode():
        x, t = v["x"], v["t"]
        h = F.conv2d(x, sd["convin.weight"], sd["convin.bias"], padding="same")
        assert_exact_or_ulp(h, v["convin"], "convin")
        te = punetg_ref.fourier_features(t, sd["time_projection.W"])
        assert_exact_or_ulp(te, v["te"], "fourier")
        p = "downward_blocks.0.0."
        g1 = F.silu(F.group_norm(h, 8, sd[p + "gnorm1.weight"], sd[p + "gnorm1.bias"], 1e-5))
        assert_exact_or_ulp(g1, v["gn1_silu"], "gn1+silu")
        assert_exact_or_ulp(punetg_ref.time_shift(sd, p + "timeblock.", te), v["timeshift"], "timeshift")
        r = punetg_ref.resnet_block(sd, p, h, te)
        assert_exact_or_ulp(r, v["resblock"], "resblock")
        rs = F.silu(punetg_ref.group_rms_norm(v["conv1_shift"], sd[p + "gnorm2.weight"], sd[p + "gnorm2.bias"]))
        assert_exact_or_ulp(rs, v["rms_silu"], "rms+silu")
        a = punetg_ref.attention_2d(sd, "attn_block.0.", v["attn_in"])
        assert_exact_or_rel(a, v["attn_out"], "attn_out", 2e-6)
        out = punetg_ref.punetg_forward(sd, cfg, x, t)
        assert_exact_or_rel(out, v["out_f32"], "out_f32", 2e-6)
        sd64 = {k: w.double() for k, w in sd.items()}
        out64 = punetg_ref.punetg_forward(sd64, cfg, x.double(), t.double())
        assert_exact_or_rel(out64, v["out_f64"], "out_f64", 1e-14)


def test_punetg_trajectories():
    v, _ = load("punetg8_traj")
    _, sd = load("punetg8_forward")
    cfg = punetg_ref.default_config(model_channels=8)
    net = punetg_ref.make_net(sd, cfg)
    wn = v["white_noise"]
    h = K.propagate_white_noise(net, wn, 6, record_history=True)
    assert_exact_or_rel(h, v["hist_heun_N6_f32"], "hist_heun_N6_f32", 2e-6)
    h = K.propagate_white_noise(net, wn, 6, integrator="euler", record_history=True)
    assert_exact_or_rel(h, v["hist_euler_N6_f32"], "hist_euler_N6_f32", 2e-6)
    h = K.propagate_white_noise(net, wn, 6, integrator="karras", record_history=True, eps=v["eps_karras_N6"])
    assert_exact_or_rel(h, v["hist_karras_N6_f32"], "hist_karras_N6_f32", 2e-6)
    h = K.propagate_white_noise(net, wn, 6, integrator="euler-maruyama", record_history=True, eps=v["eps_em_N6"])
    assert_exact_or_rel(h, v["hist_em_N6_f32"], "hist_em_N6_f32", 2e-6)
    o = K.propagate_white_noise(net, wn, 18)
    assert_exact_or_rel(o, v["out_heun_N18_f32"], "out_heun_N18_f32", 5e-6)
    sd64 = {k: w.double() for k, w in sd.items()}
    net64 = punetg_ref.make_net(sd64, cfg)
    h = K.propagate_white_noise(net64, wn.double(), 6, record_history=True)
    assert_exact_or_rel(h, v["hist_heun_N6_f64"], "hist_heun_N6_f64", 1e-13)
    o = K.propagate_white_noise(net64, wn.double(), 18)
    assert_exact_or_rel(o, v["out_heun_N18_f64"], "out_heun_N18_f64", 1e-13)


def test_punetg_cfg_guidance():
    v, _ = load("punetg8_cfg")
    _, sd = load("punetg8_forward")
    cfg = punetg_ref.default_config(model_channels=8)
    W = v["emb_weight"]
    net = punetg_ref.make_net(sd, cfg, embed=lambda y: W[y])
    wn, y = v["white_noise"], v["y"]
    h = K.propagate_white_noise(net, wn, 4, y=y, guidance=2.0, conditional=True, record_history=True)
    assert_exact_or_rel(h, v["hist_cfg_g2_N4_f32"], "hist_cfg_g2_N4_f32", 2e-6)
    o = K.propagate_white_noise(net, wn, 4, y=y, guidance=1.0, conditional=True)
    assert_exact_or_rel(o, v["out_cond_g1_N4_f32"], "out_cond_g1_N4_f32", 2e-6)
    o = K.propagate_white_noise(net, wn, 4, y=y, guidance=0.0, conditional=True)
    assert_exact_or_rel(o, v["out_cond_g0_N4_f32"], "out_cond_g0_N4_f32", 2e-6)


@pytest.mark.parametrize("skip", ["concat", "add"])
def test_adm_forward_and_trajectories(skip):
    from oracle import adm_ref
    v, sd = load(f"adm8_{skip}")
    cfg = adm_ref.default_config(model_channels=8, time_embed_dim=8, output_embed_dim=16,
                                 skip_integration_type=skip)
    with torch.inference_mode():
        x, t = v["x"], v["t"]
        te = adm_ref.time_embedding(sd, t)
        assert_exact_or_ulp(te, v["te"], "ADMTimeEmbedding")
        b0 = adm_ref.block(sd, "encoder.layers.0.input_blocks.0.", v["stem"], te)
        assert_exact_or_rel(b0, v["enc00"], "encoder block", 2e-6)
        b1 = adm_ref.block(sd, "encoder.layers.0.input_blocks.1.", v["enc00"], te, sample="down")
        assert_exact_or_rel(b1, v["enc01_down"], "encoder block + avg-pool", 2e-6)
        out = adm_ref.adm_forward(sd, cfg, x, t)
        assert_exact_or_rel(out, v["out_f32"], "out_f32", 2e-6)
        sd64 = {k: w.double() for k, w in sd.items()}
        out64 = adm_ref.adm_forward(sd64, cfg, x.double(), t.double())
        assert_exact_or_rel(out64, v["out_f64"], "out_f64", 1e-13)
        net = adm_ref.make_net(sd, cfg)
        o = K.propagate_white_noise(net, v["white_noise"], 6)
        assert_exact_or_rel(o, v["out_heun_N6_f32"], "heun N6", 2e-6)
        h = K.propagate_white_noise(net, v["white_noise"], 4, integrator="karras", record_history=True,
                                    eps=v["eps_karras_N4"])
        assert_exact_or_rel(h, v["hist_karras_N4_f32"], "karras N4", 2e-6)


def test_porosity_conditional_cfg():
    """Config-5 shape of the path: 4-channel PUNetG + dict-style PorosityEmbedder + CFG."""
    from oracle import embedder_ref
    v, sd = load("punetg8_porosity")
    cfg = punetg_ref.default_config(model_channels=8, input_channels=4, output_channels=4)
    embed = lambda y: embedder_ref.porosity_embed(sd, "conditional_embedding.", y)   # noqa: E731
    with torch.inference_mode():
        assert_exact_or_ulp(embed({"porosity": v["porosity"].unsqueeze(0)}), v["ye"], "porosity embedding")
        assert_exact_or_ulp(embed({"porosity": v["porosity_batch"]}), v["ye_batch"], "batched porosity embedding")
    net = punetg_ref.make_net(sd, cfg, embed=embed)
    y = {"porosity": v["porosity"]}                      # un-batched, as the caller passes it
    h = K.propagate_white_noise(net, v["white_noise"], 4, y=y, guidance=2.0, conditional=True, record_history=True)
    assert_exact_or_rel(h, v["hist_cfg_g2_N4_f32"], "hist_cfg_g2_N4_f32", 2e-6)
    o = K.propagate_white_noise(net, v["white_noise"], 4, y=y, guidance=1.0, conditional=True)
    assert_exact_or_rel(o, v["out_cond_g1_N4_f32"], "out_cond_g1_N4_f32", 2e-6)


def test_inpaint_repaint_forward_and_interpolation():
    """SURVEY 8f-1 rows against the reference: Scheduler.inpaint / repaint / propagate_forward with an
    analytic score, and the module-level forward propagation, inpainting and image interpolation."""
    v, _ = load("inpaint8")
    _, sd = load("punetg8_forward")
    fn = K.gaussian_target_score(0.7)
    x, yh, mask = v["x"], v["y_hist"], v["mask"]
    assert_exact_or_ulp(K.inpaint(x, yh, mask, fn, 6, record_history=True), v["sched_inpaint_hist"], "inpaint history")
    assert_exact_or_ulp(K.inpaint(x, yh, mask, fn, 6), v["sched_inpaint_out"], "inpaint")
    h = K.repaint(x, yh, mask, fn, 6, 2, 2, v["sched_repaint_eps"], record_history=True)
    assert_exact_or_ulp(h, v["sched_repaint_hist"], "repaint history")
    assert_exact_or_ulp(K.propagate_forward(x / 80.0, fn, 6, record_history=True), v["sched_forward_heun_hist"], "forward Heun")
    net = punetg_ref.make_net(sd, punetg_ref.default_config(model_channels=8))

    def score_fn(xx, sigma):
        return K.score(net, xx, sigma)
    with torch.inference_mode():
        fh = K.propagate_forward(v["x0"], score_fn, 4, record_history=True)
        assert_exact_or_rel(fh, v["toward_noise_heun_N4"], "toward noise (Heun)", 2e-6)
        fe = K.propagate_forward(v["x0"], score_fn, 4, integrator="euler-maruyama", record_history=True,
                                 eps=v["toward_noise_em_eps"])
        assert_exact_or_rel(fe, v["toward_noise_em_N4"], "toward noise (EM)", 2e-6)
        ih = K.inpaint(v["inpaint_noise"], v["toward_noise_em_N4"], v["mask2"], score_fn, 4, record_history=True)
        assert_exact_or_rel(ih, v["module_inpaint_hist"], "module inpaint", 2e-6)
        xn = K.propagate_forward(v["x0"], score_fn, 4)
        xi = K.linear_interpolation(xn[0], xn[1], 3)
        out = K.propagate_backward(xi, score_fn, 4)
        assert_exact_or_rel(out, v["interp_N4_n3"], "interpolate_images", 2e-6)


@pytest.mark.parametrize("tag", ["vp", "ve"])
def test_vp_ve_parameterisations(tag):
    """VP / VE time grids, preconditioners, both branches of Scheduler.rhs, all integrators."""
    from oracle import vpve_ref as V
    v, _ = load("vpve8")
    _, sd = load("punetg8_forward")
    fns = V.VP() if tag == "vp" else V.VE()
    steps = V.vp_steps if tag == "vp" else V.ve_steps
    precond = V.vp_precond(fns, M=2) if tag == "vp" else V.ve_precond
    for n in (4, 6, 18):
        assert_exact_or_ulp(steps(n + 1), v[f"{tag}_steps_{n}"], f"{tag} grid {n}")
    scale = float(v[f"{tag}_maximum_scale"])
    sig = torch.tensor([0.05, 0.7, 3.0, 40.0])
    assert_exact_or_ulp(torch.stack(precond(sig)), v[f"{tag}_precond"], "preconditioner")
    fn = K.gaussian_target_score(0.7)
    x = v["x"]
    for integ in ("heun", "euler"):
        h = V.propagate(fns, steps(19), x * scale, fn, integ, record_history=True)
        assert_exact_or_ulp(h, v[f"{tag}_toy_{integ}_N18"], f"{tag} toy {integ}")
    h = V.propagate(fns, steps(7), x * scale, fn, "euler-maruyama", record_history=True, eps=v[f"{tag}_toy_em_eps"])
    assert_exact_or_ulp(h, v[f"{tag}_toy_em_N6"], f"{tag} toy EM")
    h = V.propagate(fns, steps(7), x * 0.3, fn, "heun", backward=False, record_history=True)
    assert_exact_or_ulp(h, v[f"{tag}_toy_forward_N6"], f"{tag} toy forward")
    net = punetg_ref.make_net(sd, punetg_ref.default_config(model_channels=8))

    def score_fn(xx, sigma):
        return K.score(net, xx, sigma, precond=precond)
    with torch.inference_mode():
        assert_exact_or_rel(score_fn(v[f"{tag}_xs"], torch.tensor([0.3, 5.0])), v[f"{tag}_score"], "get_score", 2e-6)
        h = V.propagate(fns, steps(7), v["white_noise"] * scale, score_fn, "heun", record_history=True)
        assert_exact_or_rel(h, v[f"{tag}_punetg_heun_N6"], f"{tag} PUNetG Heun", 2e-6)
        o = V.propagate(fns, steps(7), v["white_noise"] * scale, score_fn, "euler")
        assert_exact_or_rel(o, v[f"{tag}_punetg_euler_N6"], f"{tag} PUNetG Euler", 2e-6)
        if tag == "ve":
            h = V.propagate(fns, steps(5), v["white_noise"] * scale, score_fn, "karras", record_history=True,
                            eps=v["ve_punetg_karras_eps"])
            assert_exact_or_rel(h, v["ve_punetg_karras_N4"], "VE PUNetG sigma-churn", 2e-6)


def test_vp_sigma_churn():
    """The Karras integrator on the VP parameterisation: the churn rescales x by s(t_hat)/s(t) (integrators.py:103)."""
    from oracle import vpve_ref as V
    v, _ = load("vp_karras")
    fns = V.VP()
    assert_exact_or_ulp(V.vp_steps(7), v["steps_6"], "vp grid")
    scale = float(fns.scaling_fn(v["steps_6"][0]) * fns.noise_fn(v["steps_6"][0]))
    h = V.propagate(fns, v["steps_6"], v["x"] * scale, K.gaussian_target_score(0.7), "karras", record_history=True, eps=v["eps"])
    assert_exact_or_rel(h, v["hist_N6"], "VP sigma-churn", 2e-6)


def test_punetg_circular_convolutions():
    """convolution_type='circular' -- periodic padding, parameters under `.conv`."""
    v, sd = load("punetg8_circular")
    cfg = punetg_ref.default_config(model_channels=8, convolution_type="circular")
    with torch.inference_mode():
        h = punetg_ref.conv3x3(sd, "convin", v["x"], True)
        assert_exact_or_ulp(h, v["convin"], "circular convin")
        import torch.nn.functional as F
        d = punetg_ref.conv3x3(sd, "downsamplers.0.conv", F.max_pool2d(h, 2), True)
        assert_exact_or_ulp(d, v["down0"], "circular DownSampler")
        u = punetg_ref.conv3x3(sd, "upsamplers.1.conv", F.interpolate(d, scale_factor=2.0, mode="nearest"), True)
        assert_exact_or_ulp(u, v["up1"], "circular UpSampler")
        assert_exact_or_rel(punetg_ref.punetg_forward(sd, cfg, v["x"], v["t"]), v["out_f32"], "out_f32", 2e-6)
        hist = K.propagate_white_noise(punetg_ref.make_net(sd, cfg), v["white_noise"], 6, record_history=True)
        assert_exact_or_rel(hist, v["hist_heun_N6_f32"], "hist_heun_N6_f32", 2e-6)


VARIANTS = {
    "mp": dict(convolution_type="mp"),
    "pix_ln": dict(first_resblock_norm="GroupPix", second_resblock_norm="GroupLN"),
    "none_rms_noaffine": dict(first_resblock_norm="none", second_resblock_norm="GroupRMS", affine_norm=False),
    "cosine": dict(attn_type="cosine"),
    "fourier_in": dict(in_embedding=True, bias=False),      # ConvolutionalFourierProjection as convin (punetg.py:194-202)
    "extra_res": dict(),                                    # extra_residual = AvgPool2d(3, 1, 1) shared by every block
    "k5": dict(kernel_size=5, in_out_kernel_size=1, transition_kernel_size=5),
    "k7": dict(kernel_size=1, in_out_kernel_size=7, transition_kernel_size=7),
    "k5_circular": dict(kernel_size=5, in_out_kernel_size=5, transition_kernel_size=7, convolution_type="circular"),   # round 3
}
EXTRA_RES = torch.nn.AvgPool2d(3, stride=1, padding=1)


@pytest.mark.parametrize("tag", sorted(VARIANTS))
def test_punetg_layer_variants(tag):
    """magnitude-preserving layers (normedlayers.py, the in-house attention) and the other
    norm choices of ResnetBlockC (GroupPix, none, affine_norm=False) against the reference's outputs."""
    v, sd = load("punetg8_" + tag)
    over = VARIANTS[tag]
    cfg = punetg_ref.default_config(model_channels=8, **over)
    er = EXTRA_RES if tag == "extra_res" else None
    cfg["extra_residual"] = er
    kind = "mp" if tag == "mp" else (over.get("convolution_type") == "circular")
    norms = (over.get("first_resblock_norm", "GroupLN"), over.get("second_resblock_norm", "GroupRMS"))
    if not over.get("affine_norm", True):
        assert not any("gnorm" in k for k in sd)
    with torch.inference_mode():
        if tag == "fourier_in":
            assert "convin.W" in sd and "convin.weight" not in sd
            # the fixture's layer output is net.convin(x) on the bare 1-channel x: einsum broadcasts it over both rows of W
            h = punetg_ref.fourier_input(sd, v["x"])
        else:
            h = punetg_ref.conv3x3(sd, "convin", v["x"], kind)
        assert_exact_or_ulp(h, v["convin"], tag + " convin")
        te = punetg_ref.fourier_features(v["t"], sd["time_projection.W"])
        r = punetg_ref.resnet_block(sd, "downward_blocks.0.0.", v["convin"], te, kind, norms, er)
        assert_exact_or_rel(r, v["resblock"], tag + " resblock", 1e-6)
        if tag in ("mp", "cosine"):
            a = punetg_ref.mp_attention_2d(sd, "attn_block.0.", v["attn_in"], False, tag == "mp", tag == "cosine")
        else:
            a = punetg_ref.attention_2d(sd, "attn_block.0.", v["attn_in"])
        assert_exact_or_rel(a, v["attn_out"], tag + " attention", 2e-6)
        assert_exact_or_rel(punetg_ref.punetg_forward(sd, cfg, v["x"], v["t"]), v["out_f32"], tag + " out_f32", 2e-6)
        hist = K.propagate_white_noise(punetg_ref.make_net(sd, cfg), v["white_noise"], 6, record_history=True)
        assert_exact_or_rel(hist, v["hist_heun_N6_f32"], tag + " hist_heun_N6_f32", 2e-6)


def _spatial_embed(sd):
    w, b = sd["conditional_embedding.weight"], sd["conditional_embedding.bias"]
    return lambda y: torch.nn.functional.conv2d(y if y.dim() == 4 else y[None], w, b)


def test_punetg_spatial_conditional_embedding():
    """punetg.py:405-407, commonlayers.py:537-546, 838-869: a conditional embedding that is a field makes the time shift of
    every block a field (time MLP per pixel, CornerPool to the block's resolution)."""
    v, sd = load("punetg8_spatial_cond")
    cfg = punetg_ref.default_config(model_channels=8)
    embed = _spatial_embed(sd)
    with torch.inference_mode():
        r = punetg_ref.resnet_block(sd, "downward_blocks.1.0.", v["resblock_in"], v["resblock_te"])
        assert_exact_or_rel(r, v["resblock_l1"], "level-1 block with a CornerPooled shift", 1e-6)
        net = punetg_ref.make_net(sd, cfg, embed)
        assert_exact_or_rel(net(v["x"], v["t"], v["y"]), v["out_f32"], "out_f32", 2e-6)
        assert_exact_or_rel(net(v["x"], v["t"]), v["out_uncond_f32"], "out_uncond_f32", 2e-6)
        sd64 = {k: t.double() for k, t in sd.items()}
        out64 = punetg_ref.make_net(sd64, cfg, _spatial_embed(sd64))(v["x"].double(), v["t"].double(), v["y"].double())
        assert rel_l2(out64, v["out_f64"]) < 1e-13
        for g in (1.0, 2.0):
            hist = K.propagate_white_noise(net, v["white_noise"], 4, y=v["y"][0], guidance=g, conditional=True, record_history=True)
            assert_exact_or_rel(hist, v[f"hist_heun_N4_g{int(g)}_f32"], f"history g={g}", 2e-6)


def test_si_latent_boundary_and_single_step():
    """SIModule with an autoencoder and the batch-norm initial_norm (flowfield.py:300-345, 742-747), and its
    single-step entry point integration_step (:749-781)."""
    from oracle import si_ref as S
    v, _ = load("si8_latent")
    _, sd = load("latent8")
    cfg = punetg_ref.default_config(model_channels=8, input_channels=4, output_channels=4)
    base = punetg_ref.make_net(sd, cfg)
    model = lambda x, t, y=None: base(x, t, y)                                  # noqa: E731
    sch = S.scheduler("linear")
    bn = dict(mean=torch.tensor([0.3, -0.2, 0.05, 1.1]), var=torch.tensor([2.5, 0.4, 1.0, 0.09]), sigma=1.0)
    ae = ToyAutoencoder()
    noise = v["noise"]
    ts = torch.linspace(1, 0, 5)
    with torch.inference_mode():
        lat = K.batchnorm_eval(S.sample(sch, "identity", model, noise, 5), inverse=True, **bn)
        assert_exact_or_rel(lat, v["latents_N5"], "latents", 2e-6)
        assert_exact_or_rel(ae.decode(lat), v["sample_N5"], "decoded sample", 2e-6)
        h = S.integrate(sch, "identity", model, noise * sch["sigma"](ts[0]), ts, return_history=True)
        hu = torch.stack([K.batchnorm_eval(x, inverse=True, **bn) for x in h])
        assert_exact_or_rel(hu, v["hist_N5"], "unnormalised history", 2e-6)
        t0, t1 = torch.full((2,), 0.7), torch.full((2,), 0.45)
        for m in ("euler", "heun"):
            assert_exact_or_rel(S.integration_step(sch, "identity", model, noise, t0, t1, m), v["step_" + m], m + " step", 2e-6)
    assert str(v["sd_keys"]) == "['initial_norm.running_mean' 'initial_norm.running_var']"


def si_custom_precondition(model, x, t, y=None):
    """The user precondition callable of the si8_generic fixture (oracle/tools/make_golden.py)."""
    return 0.5 * model(x, t, y=y) - 0.1 * x


def test_si_generic_preconditioners_and_per_sample_times():
    """Autonomous flows, a user precondition callable (flowfield.py:127-165), per-sample times in the field getters."""
    from oracle import si_ref as S
    v, _ = load("si8_generic")
    _, sd = load("punetg8_forward")
    cfg = punetg_ref.default_config(model_channels=8)

    def model(x, t=None, y=None):                                   # PUNetG.forward: t = None -> zero time embedding
        return punetg_ref.punetg_forward(sd, cfg, x, t)
    noise = v["noise"]
    ts = torch.linspace(1, 0, 5)
    with torch.inference_mode():
        for tag, sname, kind in (("auto_identity", "linear", "auto_identity"), ("auto_edm", "cosine", "auto_edm"),
                                 ("callable", "linear", si_custom_precondition)):
            sch = S.scheduler(sname)
            assert_exact_or_rel(S.sample(sch, kind, model, noise, 5), v[tag + "_sample_N5"], tag, 2e-6)
            h = S.integrate(sch, kind, model, noise * sch["sigma"](ts[0]), ts, return_history=True)
            assert_exact_or_rel(h, v[tag + "_hist_N5"], tag + " history", 2e-6)
        sch = S.scheduler("cosine")
        assert_exact_or_rel(S.flow_field(sch, "edm", model, noise, v["persample_t"]), v["persample_flow"], "per-sample flow", 2e-6)
        assert_exact_or_rel(S.score_field(sch, "edm", model, noise, v["persample_t"]), v["persample_score"], "per-sample score", 2e-6)


def _inpaint_draws(v, tag):
    return [v[f"{tag}_eps{i:02d}"] for i in range(int(v[tag + "_ndraws"]))]


SI_INPAINT = (("hard", "linear", "identity", None, dict(nsteps=5)),
              ("soft_jump", "cosine", "edm", 2.0, dict(nsteps=5, mask_falloff=2, resample_steps=1, mask_start_t=0.8)))


def test_si_inpaint():
    """SIModule.inpaint (flowfield.py:546-702) with the reference's recorded noise draws."""
    from oracle import si_ref as S
    v, _ = load("si8_inpaint")
    _, sd = load("punetg8_forward")
    base = punetg_ref.make_net(sd, punetg_ref.default_config(model_channels=8))
    model = lambda x, t, y=None: base(x, t, y)                                  # noqa: E731
    with torch.inference_mode():
        assert_exact_or_ulp(S.soft_mask(v["mask"], 2), v["soft_jump_soft_mask"], "soft mask")
        for tag, sname, kind, ns, kw in SI_INPAINT:
            out = S.inpaint(S.scheduler(sname), kind, model, v["x_orig"], v["mask"], v["orig_noise"],
                            draws=_inpaint_draws(v, tag), norm_sigma=ns, **kw)
            assert_exact_or_rel(out, v[tag + "_out"], "inpaint " + tag, 2e-6)


class TinyCondNet(torch.nn.Module):
    """The stand-in network of the autoreg8 fixture's cond_time = 3 case (oracle/tools/make_golden.py)."""

    def __init__(self):
        super().__init__()
        self.gain = torch.nn.Parameter(torch.tensor(0.3))

    def forward(self, x, t, y=None):
        f = y["y"].reshape(y["y"].shape[0], 3, 2, *y["y"].shape[2:])
        wts = torch.tensor([0.2, -0.5, 0.9]).view(1, 3, 1, 1, 1).to(x)
        return self.gain * x + (f * wts).sum(dim=1) + 0.1 * t.view(-1, 1, 1, 1)


def test_autoregressive_forecast_loop():
    """KarrasModule.autoregressive_sample (autoregressivesample.py:27-203) -- window assembly,
    sample-0 conditioning, minibatching -- with the white noise drawn from the CPU generator as sample() does."""
    v, _ = load("autoreg8")
    _, sd = load("punetg8_cond")
    cfg = punetg_ref.default_config(model_channels=8, input_channels=3, output_channels=1)

    def cond_net(x, t, y=None):                                   # PUNetGCond.forward, punetg.py:719-735
        f = y["y"].expand(x.shape[0], *y["y"].shape[1:])
        return punetg_ref.punetg_forward(sd, cfg, torch.cat([x, f], dim=1), t)

    def sampler(net, shape, nsteps):
        def fn(n, y):
            wn = torch.randn(n, *shape)
            return K.propagate_white_noise(net, wn, nsteps, y=dict(y), conditional=True)
        return fn

    with torch.inference_mode():
        torch.manual_seed(121)
        f = K.autoregressive_forecast(sampler(cond_net, (1, 16, 16), 3), v["y0"].clone(), 2, (1, 16, 16), 5, 2)
        assert_exact_or_rel(f, v["plain_forecasts"], "autoregressive forecasts", 2e-6)
        assert_exact_or_rel(f, v["plain_intermediate_latent"], "latent == pixel without an autoencoder", 2e-6)
        assert_exact_or_rel(f[-1], v["plain_final_forecast"], "final forecast", 2e-6)
        torch.manual_seed(121)                                     # maximum_batch_size = 2 on 3 samples: runs of 2 and 1
        parts = [K.autoregressive_forecast(sampler(cond_net, (1, 16, 16), 3), v["y0"].clone(), b, (1, 16, 16), 5, 2)
                 for b in (2, 1)]
        assert_exact_or_rel(parts[0], v["batched_forecasts"][:, :2], "minibatched forecasts, first run", 2e-6)
        # the single-sample run takes other convolution code paths in torch's CPU backend than the fixture's run did
        # (thread count / blocking), and five forecasts fed back into the condition amplify that last-ulp difference
        assert rel_l2(parts[1], v["batched_forecasts"][:, 2:]) < 1e-4
        tiny = TinyCondNet()
        torch.manual_seed(122)
        f3 = K.autoregressive_forecast(sampler(lambda x, t, y=None: tiny(x, t, y), (2, 8, 8), 3), v["tiny_y0"].clone(),
                                       2, (2, 8, 8), 6, 3)
        assert_exact_or_rel(f3, v["tiny_forecasts"], "cond_time = 3 window assembly", 2e-6)


class ToyAutoencoder(torch.nn.Module):
    """The parameter-free autoencoder the latent8 fixture was generated with (oracle/tools/make_golden.py)."""

    def encode(self, x):
        return torch.nn.functional.pixel_unshuffle(x, 2) * 0.5

    def decode(self, z):
        return torch.nn.functional.pixel_shuffle(z * 2.0, 2)


def test_latent_boundary_and_edm_batch_norm():
    """autoencoder + DimensionAgnosticBatchNorm around the loop (karrasmodule.py:1192-1241)."""
    v, sd = load("latent8")
    cfg = punetg_ref.default_config(model_channels=8, input_channels=4, output_channels=4)
    net = punetg_ref.make_net(sd, cfg)
    ae = ToyAutoencoder()
    with torch.inference_mode():
        stats = dict(mean=torch.tensor([0.3, -0.2, 0.05, 1.1]), var=torch.tensor([2.5, 0.4, 1.0, 0.09]), sigma=0.5,
                     weight=torch.tensor([1.5, 0.7, -1.2, 0.9]), bias=torch.tensor([0.1, -0.3, 0.0, 0.4]))
        assert_exact_or_ulp(K.batchnorm_eval(v["bnC_in"], **stats), v["bnC_normalize"], "per-channel normalize")
        assert_exact_or_ulp(K.batchnorm_eval(v["bnC_in"], inverse=True, **stats), v["bnC_unnormalize"], "per-channel unnorm")
        bn = dict(mean=v["bn1_mean"], var=v["bn1_var"], sigma=0.5)
        z = K.encode(v["x"], ae, bn)
        assert_exact_or_ulp(z, v["bn1_encode"], "encode")
        assert_exact_or_ulp(K.decode(z, ae, bn), v["bn1_decode_encode"], "decode(encode)")
        lat = K.propagate_white_noise(net, v["white_noise"], 4)
        assert_exact_or_rel(lat, v["bn1_latent_N4"], "latent sample", 2e-6)
        assert_exact_or_rel(K.decode(lat, ae, bn), v["bn1_sample_N4"], "decoded sample", 2e-6)
        hist = K.propagate_white_noise(net, v["white_noise"], 3, record_history=True)
        assert_exact_or_rel(K.decode(hist, ae, bn, record_history=True), v["bn1_hist_N3"], "decoded history", 2e-6)
        plain = dict(mean=torch.tensor([-0.4]), var=torch.tensor([0.6]), sigma=0.5)
        assert_exact_or_rel(K.decode(lat, None, plain), v["plain_sample_N4"], "batch-norm only", 2e-6)
    assert str(v["plain_sd_keys"]) == "['edm_batch_norm.running_mean' 'edm_batch_norm.running_var']"


@pytest.mark.parametrize("tag,over", [
    ("rms_ln", dict(first_resblock_norm="GroupRMS", second_resblock_norm="GroupLN")),
    ("ln_ln_noaffine", dict(first_resblock_norm="GroupLN", second_resblock_norm="GroupLN", affine_norm=False)),
    ("dec2", dict(decoder_type=2))])
def test_adm_norm_choices(tag, over):
    """make_norm_layers (adm.py:385-406): either norm in either slot; ADM ignores affine_norm=False (keys stay)."""
    from oracle import adm_ref
    v, sd = load("adm8_" + tag)
    cfg = adm_ref.default_config(model_channels=8, time_embed_dim=8, output_embed_dim=16, **over)
    norms = (over.get("first_resblock_norm", "GroupLN"), over.get("second_resblock_norm", "GroupRMS"))
    with torch.inference_mode():
        te = adm_ref.time_embedding(sd, v["t"])
        b0 = adm_ref.block(sd, "encoder.layers.0.input_blocks.0.", v["stem"], te, norms=norms)
        assert_exact_or_rel(b0, v["enc00"], tag + " block", 1e-6)
        assert_exact_or_rel(adm_ref.adm_forward(sd, cfg, v["x"], v["t"]), v["out_f32"], tag + " out", 2e-6)


@pytest.mark.parametrize("tag", ["3d", "3d_circular"])
def test_punetg_volumes(tag):
    """PUNetG(dimension=3) -- Conv3d / CircularConv3d, MaxPool3d, nearest upsampling, attention over
    the flattened voxels."""
    import torch.nn.functional as F
    v, sd = load("punetg8_" + tag)
    circ = tag.endswith("circular")
    cfg = punetg_ref.default_config(model_channels=8, convolution_type="circular" if circ else "default")
    with torch.inference_mode():
        h = punetg_ref.conv3x3(sd, "convin", v["x"], circ)
        assert_exact_or_ulp(h, v["convin"], "Conv3d convin")
        d = punetg_ref.conv3x3(sd, "downsamplers.0.conv", F.max_pool3d(h, 2), circ)
        assert_exact_or_ulp(d, v["down0"], "3-D DownSampler")
        u = punetg_ref.conv3x3(sd, "upsamplers.1.conv", F.interpolate(d, scale_factor=2.0, mode="nearest"), circ)
        assert_exact_or_ulp(u, v["up1"], "3-D UpSampler")
        te = punetg_ref.fourier_features(v["t"], sd["time_projection.W"])
        r = punetg_ref.resnet_block(sd, "downward_blocks.0.0.", v["convin"], te, circ)
        assert_exact_or_rel(r, v["resblock"], "3-D resblock", 1e-6)
        assert_exact_or_rel(punetg_ref.punetg_forward(sd, cfg, v["x"], v["t"]), v["out_f32"], "3-D forward", 2e-6)
        if not circ:
            hist = K.propagate_white_noise(punetg_ref.make_net(sd, cfg), v["white_noise"], 4, record_history=True)
            assert_exact_or_rel(hist, v["hist_heun_N4_f32"], "3-D trajectory", 2e-6)


SMALL_VOLUME_NET = dict(channel_expansion=[2], number_resnet_downward_block=1, number_resnet_upward_block=1,
                        number_resnet_attn_block=1, number_resnet_before_attn_block=1, number_resnet_after_attn_block=1)
VOLUME_K5 = {"3d_k5": dict(kernel_size=5, in_out_kernel_size=1, transition_kernel_size=5),
             "3d_k5_circular": dict(kernel_size=5, in_out_kernel_size=5, transition_kernel_size=5, convolution_type="circular")}


@pytest.mark.parametrize("tag", sorted(VOLUME_K5))
def test_punetg_volumes_with_other_kernel_sizes(tag):
    """Round 3 (SURVEY 8f-4 residue): 1^3 and 5^3 kernels on volumes (punetg_config.py:19-25; Conv3d(padding='same') /
    CircularConv3d with padding k//2, commonlayers.py:973-1034), on a two-level network with one block per stage."""
    v, sd = load("punetg8_" + tag)
    circ = tag.endswith("circular")
    cfg = punetg_ref.default_config(model_channels=8, **VOLUME_K5[tag], **SMALL_VOLUME_NET)
    with torch.inference_mode():
        assert_exact_or_ulp(punetg_ref.conv3x3(sd, "convin", v["x"], circ), v["convin"], "k^3 convin")
        te = punetg_ref.fourier_features(v["t"], sd["time_projection.W"])
        r = punetg_ref.resnet_block(sd, "downward_blocks.0.0.", v["convin"], te, circ)
        assert_exact_or_rel(r, v["resblock"], "5^3 resblock", 1e-6)
        assert_exact_or_rel(punetg_ref.punetg_forward(sd, cfg, v["x"], v["t"]), v["out_f32"], "k^3 forward", 2e-6)


def test_adm_circular_convolutions():
    from oracle import adm_ref
    v, sd = load("adm8_circular")
    cfg = adm_ref.default_config(model_channels=8, time_embed_dim=8, output_embed_dim=16, convolution_type="circular")
    with torch.inference_mode():
        assert_exact_or_rel(adm_ref.adm_forward(sd, cfg, v["x"], v["t"]), v["out_f32"], "ADM circular", 2e-6)


def _si_cases():
    return (("linear_identity", "linear", "identity", None), ("edm_edm", "edm", "edm", None),
            ("cosine_edm_norm2", "cosine", "edm", 2.0))


def test_si_flow_matching_sampler():
    """SIModule sampling (three interpolants, identity / EDM parameterisation, CFG)."""
    from oracle import si_ref as S
    v, _ = load("si8")
    _, sd = load("punetg8_forward")
    vc, _ = load("punetg8_cfg")
    cfg = punetg_ref.default_config(model_channels=8)
    base = punetg_ref.make_net(sd, cfg)
    model = lambda x, t, y=None: base(x, t, y)                                  # noqa: E731
    W = vc["emb_weight"]
    cbase = punetg_ref.make_net(sd, cfg, embed=lambda y: W[y])
    cmodel = lambda x, t, y=None: cbase(x, t, y)                                # noqa: E731
    noise = v["noise"]
    ts = torch.linspace(1, 0, 6)
    with torch.inference_mode():
        for tag, sname, kind, ns in _si_cases():
            sch = S.scheduler(sname)
            assert_exact_or_rel(S.sample(sch, kind, model, noise, 6, norm_sigma=ns), v[f"{tag}_sample_N6"], tag, 2e-6)
            h = S.integrate(sch, kind, model, noise * sch["sigma"](ts[0]), ts, return_history=True)
            assert_exact_or_rel(h if ns is None else h * ns, v[f"{tag}_hist_N6"], tag + " history", 2e-6)
            tt = torch.tensor([0.4, 0.4])
            assert_exact_or_rel(S.flow_field(sch, kind, model, noise, tt), v[f"{tag}_flow"], tag + " flow", 2e-6)
            assert_exact_or_rel(S.score_field(sch, kind, model, noise, tt), v[f"{tag}_score"], tag + " score", 2e-6)
        y = v["cfg_y"].unsqueeze(0)
        lin, edm = S.scheduler("linear"), S.scheduler("edm")
        assert_exact_or_rel(S.sample(lin, "identity", cmodel, noise, 6, y=y, guidance=2.0), v["cfg_g2_sample_N6"], "cfg g2", 2e-6)
        assert_exact_or_rel(S.sample(lin, "identity", cmodel, noise, 6, y=y, guidance=1.0), v["cfg_g1_sample_N6"], "cfg g1", 2e-6)
        assert_exact_or_rel(S.sample(edm, "edm", cmodel, noise, 6, y=y, guidance=2.0), v["cfg_edm_g2_sample_N6"], "cfg edm", 2e-6)


def test_punetg_without_biases():
    v, sd = load("punetg8_nobias")
    assert not any(k.endswith("conv1.bias") or k.startswith("convin.bias") for k in sd)
    cfg = punetg_ref.default_config(model_channels=8, bias=False)
    with torch.inference_mode():
        assert_exact_or_rel(punetg_ref.punetg_forward(sd, cfg, v["x"], v["t"]), v["out_f32"], "bias=False", 2e-6)


def test_punetgcond_channel_conditioning():
    """PUNetGCond (punetg.py:706-735): y['field'] concatenated to x as input channels."""
    v, sd = load("punetg8_cond")
    cfg = punetg_ref.default_config(model_channels=8, input_channels=3, output_channels=1)
    base = punetg_ref.make_net(sd, cfg)

    def net(x, t, y=None):
        ycat = y["field"]
        if ycat.shape[0] == 1 and x.shape[0] > 1:
            ycat = torch.cat([ycat] * x.shape[0], dim=0)
        return base(torch.cat([x, ycat], dim=1), t)
    with torch.inference_mode():
        assert_exact_or_rel(net(v["x"], v["t"], {"field": v["field"]}), v["out_f32"], "PUNetGCond forward", 2e-6)
        h = K.propagate_white_noise(net, v["white_noise"], 4, y={"field": v["field"][0]}, guidance=1.0, conditional=True,
                                    record_history=True)
        assert_exact_or_rel(h, v["hist_heun_N4_f32"], "PUNetGCond trajectory", 2e-6)


def test_euler_maruyama_langevin_interval():
    v, _ = load("em_interval")
    h = K.propagate_backward(v["x"], K.gaussian_target_score(0.7), 12, integrator="euler-maruyama", record_history=True,
                             eps=v["eps"], langevin_const=float(v["langevin_const"]),
                             langevin_interval=tuple(float(t) for t in v["langevin_interval"]))
    assert_exact_or_ulp(h, v["hist"], "EM with a Langevin interval")


def test_philox_known_answers():
    """The in-kernel noise generator is Philox4x32-10: its oracle (oracle/philox_ref.py) reproduces the published
    Random123 known-answer vectors (kat_vectors: zero, all-ones and the pi-digits inputs)."""
    import numpy as np
    from oracle import philox_ref as P

    def kat(c, k):
        return [int(v) for v in P.philox4x32_10(np.array([c], dtype=np.uint64), np.array([k], dtype=np.uint64))[0]]
    assert kat([0, 0, 0, 0], [0, 0]) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert kat([0xffffffff] * 4, [0xffffffff] * 2) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert kat([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0]) == \
        [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]
    z = P.normal(1234, 0, 1 << 18)
    assert abs(z.mean()) < 0.01 and abs(z.std() - 1) < 0.01 and np.isfinite(z).all()
    assert np.array_equal(P.normal(1234, 16, 64), P.normal(1234, 0, 128)[64:])          # offset = counter shift


ADM_BLOCK_CASES = {
    # tag: (sample, has_attn, has_residual, norms, skip_integration_type, circular)
    "enc2d": (None, False, False, ("GroupLN", "GroupRMS"), "concat", False),
    "enc2d_down": ("down", False, False, ("GroupLN", "GroupRMS"), "concat", False),
    "enc3d": (None, False, False, ("GroupLN", "GroupRMS"), "concat", False),
    "enc3d_full": ("down", True, True, ("GroupLN", "GroupRMS"), "concat", False),
    "dec2d_skip": ("up", True, True, ("GroupLN", "GroupRMS"), "concat", False),
    "dec3d_skip_add": ("up", False, True, ("GroupRMS", "GroupLN"), "add", False),
    "enc3d_circ": ("down", False, True, ("GroupLN", "GroupRMS"), "concat", True),
}


@pytest.mark.parametrize("tag", sorted(ADM_BLOCK_CASES))
def test_adm_blocks_on_fields_and_volumes(tag):
    """ADM residual blocks called on their own as the reference's tests/test_adm.py does (14^2 fields, 14^3 volumes;
    AvgPool3d, attention over 343 voxels, skip concat / add): the oracle's block against the reference's outputs."""
    from oracle import adm_ref
    v, sd_all = load("adm_blocks")
    sd = {k[len(tag) + 1:]: w for k, w in sd_all.items() if k.startswith(tag + "/")}
    sample, has_attn, has_res, norms, skip_type, circ = ADM_BLOCK_CASES[tag]
    with torch.inference_mode():
        got = adm_ref.block(sd, "", v[tag + "/x"], v[tag + "/te"], sample=sample, has_attn=has_attn, attn_residual=True,
                            circular=circ, norms=norms, skip=v.get(tag + "/skip"), skip_integration_type=skip_type,
                            has_residual=has_res)
    if tag == "dec2d_skip":
        # 784 tokens: nn.MultiheadAttention's eval-mode fast path (the reference module) and the functional form the
        # oracle calls differ in the last bit at this length (5e-8 relative); every other case is bit-identical
        assert rel_l2(got, v[tag + "/out_f32"]) < 2e-7
    else:
        assert_exact_or_rel(got, v[tag + "/out_f32"], tag, 2e-6)
