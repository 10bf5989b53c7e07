"""The attention core on the inputs of tests/test_gpu_attention_core.py, with the library of the tree it is run in (the working
directory, which needs a copy of that test file): rel-L2 and max-abs of the whole output against fp64, per case and exponent-row
variant.  Run inside a build of the parent commit it writes the fixture the test compares with.

    python <this tree>/tools/attn_core_errors.py [--write tests/golden/attn_core_parent_errors.json]"""
import json
import os
import sys
sys.path.insert(0, os.getcwd())
import torch
from diffsci_amd import _native as N
from diffsci_amd import ops
from tests import test_gpu_attention_core as T
from tests.test_gpu_attention_edges import _sdpa

dev = torch.device("cuda:0")
out = {}
for E, H, L in T.SHAPES:
    for B in (1, 3):
        for data in ("gauss", "staircase"):
            qkv = T.make_input(E, H, L, B, data)
            want = _sdpa(qkv, E, H, torch.float64)
            t32 = T.errors(_sdpa(qkv, E, H, torch.float32), want)
            for key, got in T.run_case(ops, N, qkv, E, H, dev).items():
                e = T.errors(got, want)
                out[f"{T.case_id(E, H, L, B, data)}-{key}"] = e
                print(f"{T.case_id(E, H, L, B, data):32s} {key}: rel-L2 {e[0]:.3e} max-abs {e[1]:.3e}   torch fp32 {t32[0]:.3e} {t32[1]:.3e}",
                      flush=True)
if "--write" in sys.argv:
    f = sys.argv[sys.argv.index("--write") + 1]
    json.dump({"what": "k_attn3h before the tile loop was restructured: [rel-L2, max-abs] against fp64 on the inputs of "
                       "tests/test_gpu_attention_core.py, one MI355X (tools/attn_core_errors.py)", "errors": out},
              open(f, "w"), indent=1)
    print("wrote", f)
