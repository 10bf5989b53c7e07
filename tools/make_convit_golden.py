"""Generate tests/golden/convit_{a,b,c}.npz and their weight files (`_w1`, `_w2`, ...): the reference's ConVit (convit.py:639-735)
run on the CPU in fp32 and as an fp64 copy (imported through oracle/tools/refshim.py; needs the reference checkout that shim
points at).  The fixtures are data only: the state_dict, the inputs, the recorded white noise, the reference's outputs, and -- as
JSON strings -- its constructor signatures and state_dict key -> shape list.

Every case has a time embedding and, because the reference cannot be built otherwise (convit.py:715), a conditional embedding:
a torch.nn.Linear(1, embed_dim) whose weights are state_dict entries (`conditional_embedding.*`).  Outputs are recorded with the
condition y [B, 1] and with y=None.

    a  embed_dim=64, 8 heads (head width 8), 2 layers, default kernels on [2,1,32,32]     + 4-step Heun histories of a conditional
                                                                                           KarrasModule at guidance 1 and 2
    b  embed_dim=128, 4 heads (head width 32), 1 layer, ffn_expansion_factor=2, kernel_size_conv=3, kernel_size_in_out=3,
       in_channels=3 on [2,3,32,32]                                                       L = 256
    c  embed_dim=64, 2 heads, 1 layer, relative_positioning, attn_compression_factor=4, kernel_size_depthwise=5 on [2,1,24,40]
                                                                                          L = 60, not a multiple of 32

Norm weights, every bias and fusion_weight are perturbed (+ 0.25 randn) so that no term is exercised at its initial value only.

    python tools/make_convit_golden.py"""
import inspect
import json
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle", "tools"))
sys.path.insert(0, ROOT)
import refshim  # noqa: E402

refshim.install()
import diffsci.models as M  # noqa: E402

torch.set_num_threads(8)
PART_BYTES = 900 << 10
COMMON = dict(has_time_embedding=True, has_conditional_embedding=True, condition_dropout=0.1)
CASES = {
    "a": (dict(embed_dim=64, num_heads=8, num_layers=2, **COMMON), (2, 1, 32, 32), 480),
    "b": (dict(embed_dim=128, num_heads=4, num_layers=1, ffn_expansion_factor=2, kernel_size_conv=3, kernel_size_in_out=3, in_channels=3,
               **COMMON), (2, 3, 32, 32), 482),
    "c": (dict(embed_dim=64, num_heads=2, num_layers=1, relative_positioning=True, attn_compression_factor=4, kernel_size_depthwise=5,
               **COMMON), (2, 1, 24, 40), 484),
}


def signature(fn):
    out = []
    for name, p in inspect.signature(fn).parameters.items():
        if name != "self":
            d = p.default
            out.append([name, p.kind.name, "<required>" if d is inspect.Parameter.empty else d])
    return out


def save(name, arrs):
    """No committed file above 1 MiB: the state_dict goes to `<name>_w<i>.npz` (keys "sd/..."), the rest stays in `<name>.npz`.
    A tensor too large for one file is cut along its first axis into pieces `sd/<key>#<j>` (tests/convit_ref.load_golden joins them)."""
    gold = os.path.join(ROOT, "tests", "golden")
    arrs = dict(arrs)
    for k in [k for k in arrs if k.startswith("sd/") and arrs[k].numel() * 4 > PART_BYTES]:
        v = arrs.pop(k)
        for j, piece in enumerate(torch.chunk(v, -(-v.numel() * 4 // PART_BYTES), dim=0)):
            arrs[f"{k}#{j}"] = piece.contiguous()
    parts, room = [{k: v for k, v in arrs.items() if not k.startswith("sd/")}], [0]
    for k in sorted((k for k in arrs if k.startswith("sd/")), key=lambda k: (-arrs[k].numel(), k)):
        n = arrs[k].numel() * 4
        i = next((i for i in range(1, len(parts)) if room[i] + n <= PART_BYTES), None)
        if i is None:
            parts.append({})
            room.append(0)
            i = len(parts) - 1
        parts[i][k] = arrs[k]
        room[i] += n
    size = 0
    for i, part in enumerate(parts):
        path = os.path.join(gold, name + (f"_w{i}" if i else "") + ".npz")
        np.savez_compressed(path, **{k: (np.asarray(v.detach().cpu().numpy()) if torch.is_tensor(v) else np.asarray(v))
                                     for k, v in part.items()})
        assert os.path.getsize(path) < 1 << 20, path
        size += os.path.getsize(path)
    return len(parts), size


def build(kw, dtype=torch.float32):
    net = M.nets.ConVit(M.nets.ConVitConfig(**kw), conditional_embedding=torch.nn.Linear(1, kw["embed_dim"]))
    return net.to(dtype).eval()


def main():
    total = 0
    for tag, (kw, shape, seed) in CASES.items():
        torch.manual_seed(seed)
        net = build(kw)
        with torch.no_grad():
            for k, v in net.state_dict().items():
                if "norm" in k or ".rms." in k or k.endswith("bias") or k.endswith("fusion_weight"):
                    v.add_(0.25 * torch.randn_like(v))
        sd = net.state_dict()
        torch.manual_seed(seed + 1)
        x = torch.randn(*shape)
        t = torch.tensor([0.3, -1.1])
        y = torch.tensor([[0.7], [-0.4]])
        arrs = {"sd/" + k: v for k, v in sd.items()}
        arrs.update(x=x, t=t, y=y)
        arrs["kwargs"] = json.dumps(kw)
        arrs["signature"] = json.dumps({"ConVit": signature(M.nets.ConVit.__init__), "ConVitBlock": signature(M.nets.ConVitBlock.__init__),
                                        "ConVitConfig": signature(M.nets.ConVitConfig.__init__)})
        arrs["keys"] = json.dumps([[k, list(v.shape)] for k, v in sd.items()])
        net64 = build(kw, torch.float64)
        net64.load_state_dict({k: v.double() for k, v in sd.items()})
        with torch.inference_mode():
            arrs["out_f32"] = net(x, t, y)
            arrs["out_f64"] = net64(x.double(), t.double(), y.double())
            arrs["out_nocond_f32"] = net(x, t)
            arrs["out_nocond_f64"] = net64(x.double(), t.double())
        assert arrs["out_f64"].dtype == torch.float64
        if tag == "a":
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                module = M.KarrasModule(net, M.KarrasModuleConfig.from_edm(), conditional=True).eval()
                module64 = M.KarrasModule(net64, M.KarrasModuleConfig.from_edm(), conditional=True).eval()
            wn = torch.randn(*shape)
            arrs["white_noise"] = wn
            ys = arrs["y_hist"] = torch.tensor([0.7])                   # the sampler takes ONE condition for the batch (karrasmodule.py:916-917)
            arrs["steps_4"] = module.config.noisescheduler.create_steps(5)
            with torch.inference_mode():
                for name, g in (("heun", 1.0), ("cfg2", 2.0)):
                    arrs[f"hist_{name}_N4_f32"] = module.propagate_white_noise(wn, ys, guidance=g, nsteps=4, record_history=True)
                    arrs[f"hist_{name}_N4_f64"] = module64.propagate_white_noise(wn.double(), ys.double(), guidance=g, nsteps=4,
                                                                                 record_history=True)
            assert arrs["hist_cfg2_N4_f64"].dtype == torch.float64
        nparts, size = save("convit_" + tag, arrs)
        total += size

        def rel(a, b):
            return float((arrs[a].double() - arrs[b]).norm() / arrs[b].norm())
        print(f"convit_{tag}: {nparts} files, {size / 1024:.1f} KiB; {len(sd)} state_dict entries; fp32 vs fp64 {rel('out_f32', 'out_f64'):.3e}"
              f" (y=None: {rel('out_nocond_f32', 'out_nocond_f64'):.3e})", flush=True)
        if tag == "a":
            for name in ("heun", "cfg2"):
                h32, h64 = arrs[f"hist_{name}_N4_f32"].double(), arrs[f"hist_{name}_N4_f64"]
                print(f"  {name} history fp32 vs fp64, per state:", [f"{float((a - b).norm() / b.norm()):.2e}" for a, b in zip(h32, h64)])
    print(f"total {total / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
