"""Generate tests/golden/dit_{a,b,c}.npz and their weight files (`_w1`, `_w2`, ...): the reference's DiffusionTransformer
(difftransformer.py:200-236) run on the CPU in fp32 and as an fp64 copy (imported through oracle/tools/refshim.py; needs the
reference checkout that shim points at).  The fixtures are data only: the state_dict, the inputs, the recorded white noise, the
reference's outputs, and -- as JSON strings -- its constructor signature and state_dict key -> shape list.

    a  defaults with nblocks=2 on [2,1,32,32]                    head width 16, L = 64; + a 4-step Heun history of KarrasModule
    b  nembed=128, nheads=4, nblocks=2, patch_size=2, nchannels=3 on [2,3,16,16]       head width 32, L = 64
    c  nembed=64, nheads=2, nblocks=1 on [2,1,24,40]             L = 60, not a multiple of 32

Norm affines and every bias are perturbed (+ 0.25 randn) so that no term is exercised at its initial value only.

    python tools/make_dit_golden.py"""
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
CASES = {
    "a": (dict(nblocks=2), (2, 1, 32, 32), 380),
    "b": (dict(nembed=128, nheads=4, nblocks=2, patch_size=2, nchannels=3), (2, 3, 16, 16), 382),
    "c": (dict(nembed=64, nheads=2, nblocks=1), (2, 1, 24, 40), 384),
}


def signature():
    out = []
    for name, p in inspect.signature(M.nets.DiffusionTransformer.__init__).parameters.items():
        if name != "self":
            out.append([name, p.kind.name, p.default])
    return out


def save(name, arrs):
    """No committed file above 1 MiB: the state_dict goes to `<name>_w<i>.npz` (keys "sd/..."), the rest stays in `<name>.npz`."""
    gold = os.path.join(ROOT, "tests", "golden")
    parts, room = [{k: v for k, v in arrs.items() if not k.startswith("sd/")}], [0]
    for k in sorted((k for k in arrs if k.startswith("sd/")), key=lambda k: -arrs[k].numel()):
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


def main():
    for tag, (kw, shape, seed) in CASES.items():
        torch.manual_seed(seed)
        net = M.nets.DiffusionTransformer(**kw).eval()
        with torch.no_grad():
            for k, v in net.state_dict().items():
                if ".norm" in k or k.endswith("bias"):
                    v.add_(0.25 * torch.randn_like(v))
        sd = net.state_dict()
        torch.manual_seed(seed + 1)
        x = torch.randn(*shape)
        t = torch.tensor([0.3, -1.1])
        arrs = {"sd/" + k: v for k, v in sd.items()}
        arrs.update(x=x, t=t)
        arrs["kwargs"] = json.dumps(kw)
        arrs["signature"] = json.dumps(signature())
        arrs["keys"] = json.dumps([[k, list(v.shape)] for k, v in sd.items()])
        net64 = M.nets.DiffusionTransformer(**kw).double().eval()
        net64.load_state_dict({k: v.double() for k, v in sd.items()})
        with torch.inference_mode():
            arrs["out_f32"] = net(x, t)
            arrs["out_f64"] = net64(x.double(), t.double())
        if tag == "a":
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                module = M.KarrasModule(net, M.KarrasModuleConfig.from_edm()).eval()
                module64 = M.KarrasModule(net64, M.KarrasModuleConfig.from_edm()).eval()
            wn = torch.randn(*shape)
            arrs["white_noise"] = wn
            arrs["steps_4"] = module.config.noisescheduler.create_steps(5)
            with torch.inference_mode():
                arrs["hist_heun_N4_f32"] = module.propagate_white_noise(wn, nsteps=4, record_history=True)
                arrs["hist_heun_N4_f64"] = module64.propagate_white_noise(wn.double(), nsteps=4, record_history=True)
            assert arrs["hist_heun_N4_f64"].dtype == torch.float64
        nparts, size = save("dit_" + tag, arrs)
        rel = float((arrs["out_f32"].double() - arrs["out_f64"]).norm() / arrs["out_f64"].norm())
        print(f"dit_{tag}: {nparts} files, {size / 1024:.1f} KiB; {len(sd)} state_dict entries; fp32 vs fp64 {rel:.3e}", flush=True)
        if tag == "a":
            h32, h64 = arrs["hist_heun_N4_f32"].double(), arrs["hist_heun_N4_f64"]
            print("  history fp32 vs fp64, per state:", [f"{float((a - b).norm() / b.norm()):.2e}" for a, b in zip(h32, h64)])


if __name__ == "__main__":
    main()
