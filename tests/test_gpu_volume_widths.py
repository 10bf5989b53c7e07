"""The volume path at production width on a real MI355X: PUNetGConfig(dimension=3) defaults to model_channels=64, so its levels run at
64, 128 and 256 channels -- on multi-chunk 16x16x32 kernels, 16-byte patch loads, the persistent producer / consumer kernel and the
parity kernel, none of which the 8-channel volume tests reach.  Kernel cases against fp64 (tools/volume_check.py), the 64-channel
network against the CPU oracle, and a kernel trace that proves the cases take the routes they are there for."""
import csv
import glob
import os
import re
import shutil
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.golden_util import rel_l2  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "volume_check.py")
N_CASES = 13                                   # 8 conv3d_mfma cases + 5 resblock3d_fused cases
TRACED = "f64,f128,f64_circ,c256_128_up,c64_128"


def _env():
    return {k: v for k, v in os.environ.items() if not k.startswith("DS_CONV_")}


def test_volume_kernels_at_production_width_vs_fp64():
    """tools/volume_check.py: ops.conv3d_mfma (plain, pooled, upsampled on both kernels, periodic, ragged channels, 5x5x5, per-slice
    magnitudes held to the bound on every output slice) and ops.resblock3d_fused (persistent kernel plain and periodic, two channel
    tiles, below the persistent minimum, ragged planes; GroupNorm and GroupRMSNorm as norm2) at 64-256 channels: within
    max(3 x torch fp32's own rel-L2, the 8-channel tests' floor) and max(4 x torch fp32's max-abs, 1e-5) of fp64; out_stats and the
    table built from them against the fp64 moments of the output; outputs, statistics and tables bit-identical between the default
    routes and the round-3 routes (one-shot kernels, one-pixel staging; child process)."""
    p = subprocess.run([sys.executable, TOOL], cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=900)
    assert p.returncode == 0 and "ALL OK" in p.stdout, p.stdout[-6000:] + p.stderr[-2000:]
    assert p.stdout.count("  ok") == N_CASES and p.stdout.count("A/B out == stats ==") == N_CASES, p.stdout[-6000:]


@pytest.mark.parametrize("conv_type,shape", [("default", (2, 1, 64, 32, 64)), ("circular", (2, 1, 16, 32, 64))])
def test_punetg64_volume_forward_vs_oracle(conv_type, shape):
    """PUNetG(model_channels=64, dimension=3), levels of 64 / 128 / 256 channels, against the CPU oracle in fp32 and fp64 and against
    its own standalone-norm route.  On [2, 1, 64, 32, 64] the folded blocks of level 0 (130 slices x 8 tiles) and level 1 (66 slices x
    2 tiles x 2 channel tiles) reach the persistent kernel; level 2 (256 channels: fuse_max_cot = 2) runs the standalone norms.  The
    periodic network on [2, 1, 16, 32, 64] puts level 0 (34 slices x 8 tiles = 272 items) on the periodic persistent variant."""
    import diffsci_amd.models as M
    from diffsci_amd import ops
    from oracle import punetg_ref
    dev = torch.device("cuda:0")
    torch.manual_seed(64 + len(conv_type))
    over = dict(model_channels=64, dimension=3, convolution_type=conv_type)
    net = M.PUNetG(M.PUNetGConfig(**over))
    assert list(net.config.channel_expansion) == [2, 4]
    with torch.no_grad():
        for k, w in net.state_dict().items():
            if "gnorm" in k or k.endswith("bias"):
                w.add_(0.2 * torch.randn_like(w))
    sd = {k: w.clone() for k, w in net.state_dict().items()}
    x, t = torch.randn(*shape) * 1.5 + 0.3, torch.tensor([0.3, 2.5])
    cfg = punetg_ref.default_config(**over)
    with torch.inference_mode():
        want32 = punetg_ref.punetg_forward(sd, cfg, x, t)
        want64 = punetg_ref.punetg_forward({k: w.double() for k, w in sd.items()}, cfg, x.double(), t.double())
    net = net.to(dev).eval()
    assert net.fuse_norm and net.fuse_max_cot == 2
    widths, circ = [], []
    orig = ops.resblock3d_fused

    def counted(h, *a, **k):
        widths.append(h.shape[1])
        circ.append(bool(k.get("circular")))
        return orig(h, *a, **k)
    ops.resblock3d_fused = counted
    try:
        with torch.no_grad():
            folded = net(x.to(dev), t.to(dev)).cpu()
    finally:
        ops.resblock3d_fused = orig
    assert len(widths) >= 4 and set(widths) == {64, 128}, f"the folded blocks did not run at 64 and 128 channels: {widths}"
    assert all(c == (conv_type == "circular") for c in circ)
    net.fuse_norm = False
    with torch.no_grad():
        plain = net(x.to(dev), t.to(dev)).cpu()
    net.fuse_norm = True
    ref_err = rel_l2(want32, want64)
    print(f"{conv_type}: vs oracle fp32 {rel_l2(folded, want32):.2e}, vs fp64 {rel_l2(folded, want64):.2e} (oracle fp32 vs fp64 "
          f"{ref_err:.2e}), folded vs standalone norms {rel_l2(folded, plain):.2e}, {len(widths)} folded blocks")
    assert torch.isfinite(folded).all()
    assert rel_l2(folded, want32) < 1e-5
    assert rel_l2(folded, want64) < max(4 * ref_err, 2e-6)
    assert rel_l2(folded, plain) < 3e-6


def _template_args(names, kernel):
    """Template argument lists of every instantiation of `kernel` among demangled kernel names."""
    out = []
    for n in names:
        m = re.search(r"\b" + kernel + r"<([^>]*)>", n)
        if m:
            out.append([a.strip() for a in m.group(1).split(",")])
    return out


def test_volume_cases_reach_the_intended_kernels(tmp_path):
    """A numerical test of a route that was silently not taken proves nothing, and the library has no 'which kernel ran' query: the
    driver's default arm under the profiler's kernel trace.  k_conv3p<PRE, CIRC, NRES, VEC, IMG> must appear with the fused loader
    (f64, f128) and in its periodic variant (f64_circ), both with 16-byte patch loads; k_conv3h<MODE, W16, PRE, CIRC, NW, S16, IMGIN,
    TWO, VEC> in its 16x16x32 form with 16-byte loads (conv1 of the fused blocks, c64_128); k_convup (c256_128_up)."""
    prof = shutil.which("rocprofv3")
    if prof is None:
        pytest.skip("rocprofv3 is not on PATH")
    p = subprocess.run([prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", str(tmp_path), "-o", "v", "--",
                        sys.executable, TOOL, "--no-ab", "--only", TRACED], cwd=ROOT, env=_env(), capture_output=True, text=True,
                       timeout=900)
    assert p.returncode == 0 and "ALL OK" in p.stdout, p.stdout[-4000:] + p.stderr[-3000:]
    files = glob.glob(os.path.join(str(tmp_path), "**", "*kernel_stats.csv"), recursive=True)
    assert files, "no kernel statistics written: " + p.stderr[-2000:]
    names = set()
    for f in files:
        with open(f, newline="") as fh:
            for row in csv.DictReader(fh):
                names.add(row["Name"])
    listing = "\n".join(sorted(n for n in names if "k_conv" in n))
    p3 = _template_args(names, "k_conv3p")
    assert any(a[0] == "true" and a[1] == "false" for a in p3), "k_conv3p with the fused loader did not run:\n" + listing
    assert any(a[0] == "true" and a[1] == "true" for a in p3), "the periodic k_conv3p did not run:\n" + listing
    assert all(a[3] == "true" and a[4] == "false" for a in p3), "k_conv3p without 16-byte loads, or on image input:\n" + listing
    h3 = _template_args(names, "k_conv3h")
    assert h3, "k_conv3h did not run:\n" + listing
    assert any(a[0] == "0" and a[2] == "false" and a[5] == "true" and a[8] == "true" for a in h3), \
        "the 16x16x32 k_conv3h with 16-byte loads (raw / activated input) did not run:\n" + listing
    assert _template_args(names, "k_convup"), "k_convup did not run:\n" + listing
