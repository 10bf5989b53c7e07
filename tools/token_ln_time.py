"""Time ds_token_layernorm per launch, and one eager DiffusionTransformer evaluation, at the shapes of tools/dit_time.py
  nembed=256, nheads=4, nblocks=6, patch_size=4 on [16,1,128,128]   (tokens [16,256,1024])
  the defaults (nembed=64) on [64,1,128,128]                         (tokens [64,64,1024])
and the LayerNorm alone at the wider register counts ([16,384,1024]: 16 rows per thread, [16,1024,1024]: 32).
Device events around ROUNDS windows after a warm-up (the LayerNorm: 20 replays of a captured chain of 100 launches; the evaluation:
40 eager calls); the median window is printed with the fastest and the slowest.
Run it once per library to compare two builds (DIFFSCI_HIP_LIB names the other one), alternating the runs.

    python tools/token_ln_time.py [label]"""
import os
import sys
sys.path.insert(0, os.getcwd())
import torch
from diffsci_amd import ops
import diffsci_amd.models as M

dev = torch.device("cuda:0")
LABEL = sys.argv[1] if len(sys.argv) > 1 else "tree"
ROUNDS = 7


def timed(f, n):
    for _ in range(max(n // 10, 3)):
        f()
    torch.cuda.synchronize()
    rounds = []
    for _ in range(ROUNDS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            f()
        e1.record()
        torch.cuda.synchronize()
        rounds.append(e0.elapsed_time(e1) / n * 1e3)
    rounds.sort()
    return rounds[ROUNDS // 2], rounds[0], rounds[-1]


def layernorm(B, E, L):
    torch.manual_seed(0)
    x, a = torch.randn(B, E, L, device=dev), torch.empty(B, E, L, device=dev)
    w, b = torch.randn(E, device=dev), torch.randn(E, device=dev)
    tab = torch.randn(40, 6 * E, device=dev)
    am = torch.zeros(B, dtype=torch.int32, device=dev)
    def launch():
        ops.token_layernorm(x, w, b, tab, 0, 1, 7, out=a, out_amax=am)

    launch()
    torch.cuda.synchronize()
    graph, per = torch.cuda.CUDAGraph(), 100              # a chain of launches replayed: the host's time per call stays out
    with torch.cuda.graph(graph):
        for _ in range(per):
            launch()
    med, lo, hi = (v / per for v in timed(graph.replay, 20))
    print(f"{LABEL:8s} token_layernorm + adaLN (+ amax) [{B},{E},{L}]: {med:8.2f} us per launch ({lo:.2f} - {hi:.2f}), "
          f"{8 * x.numel() / med / 1e3:6.0f} GB/s", flush=True)


def evaluation(kw, shape):
    torch.manual_seed(0)
    net = M.DiffusionTransformer(**kw).to(dev).eval()
    img, t = torch.randn(shape, device=dev), torch.rand(shape[0], device=dev)
    with torch.no_grad():
        med, lo, hi = timed(lambda: net.forward_unguarded(img, t), 40)
    print(f"{LABEL:8s} DiffusionTransformer({', '.join(f'{k}={v}' for k, v in kw.items()) or 'defaults'}) on {list(shape)}, one eager "
          f"evaluation: {med / 1e3:8.4f} ms ({lo / 1e3:.4f} - {hi / 1e3:.4f})", flush=True)


for B, E, L in ((16, 256, 1024), (64, 64, 1024), (16, 384, 1024), (16, 1024, 1024)):
    layernorm(B, E, L)
evaluation(dict(nembed=256, nheads=4, nblocks=6, patch_size=4), (16, 1, 128, 128))
evaluation(dict(), (64, 1, 128, 128))
