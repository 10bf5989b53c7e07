"""Generate the fixtures of DiffusionPeriodizer (tests/test_periodizer.py) from the reference implementation on the CPU (imported
through oracle/tools/refshim.py; needs the reference checkout that shim points at).  Data only:

    tests/golden/periodizer_cases.npz          per case of tests/periodizer_ref.py (FIELDS, VOLUMES) the input and what the reference's
                                               DiffusionPeriodizer returns: <case>/x, /expand (expand_periodic), /crop (crop_center of
                                               the analytic network's output on the expansion), /blend (cosine_blend_boundaries of x),
                                               /forward (forward around tests.periodizer_ref.analytic_net)
    tests/golden/api_surface_periodizer.json   inspect.signature of the three public names and of the class's methods

    python tools/make_periodizer_golden.py"""
import inspect
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle", "tools"))
sys.path.insert(0, ROOT)
import refshim  # noqa: E402

refshim.install()
from diffsci.extra import periodizer as P  # noqa: E402

import importlib.util  # noqa: E402

# by path: the reference checkout has a `tests` package of its own
_spec = importlib.util.spec_from_file_location("periodizer_ref", os.path.join(ROOT, "tests", "periodizer_ref.py"))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)

GOLD = os.path.join(ROOT, "tests", "golden")
METHODS = ("__init__", "expand_periodic", "crop_center", "cosine_blend_boundaries", "forward", "forward_no_blend",
           "forward_expand_only")


class Analytic(torch.nn.Module):
    def forward(self, x, *args, **kwargs):
        return R.analytic_net(x, *args, **kwargs)


def main():
    out = {}
    for k, (shape, pad, bw) in enumerate(R.FIELDS + R.VOLUMES):
        name = R.case_name(shape, pad, bw)
        x = R.case_input(shape, k)
        per = P.DiffusionPeriodizer(Analytic(), pad, bw, dimension=len(shape) - 2)
        with torch.no_grad():
            expanded = per.expand_periodic(x)
            out[name + "/x"] = x.numpy()
            out[name + "/expand"] = expanded.numpy()
            out[name + "/crop"] = per.crop_center(per.net(expanded), shape[2:]).contiguous().numpy()
            out[name + "/blend"] = per.cosine_blend_boundaries(x).numpy()
            out[name + "/forward"] = per(x).numpy()
    out["cpu_capability"] = np.array(torch.backends.cpu.get_cpu_capability())
    path = os.path.join(GOLD, "periodizer_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    surface = {"DiffusionPeriodizer": {m: str(inspect.signature(getattr(P.DiffusionPeriodizer, m))) for m in METHODS},
               "PeriodicSamplerWrapper": {m: str(inspect.signature(getattr(P.PeriodicSamplerWrapper, m)))
                                          for m in ("__init__", "step", "reset")},
               "measure_periodicity_error": str(inspect.signature(P.measure_periodicity_error))}
    path = os.path.join(GOLD, "api_surface_periodizer.json")
    with open(path, "w") as f:
        json.dump(surface, f, indent=1, sort_keys=True)
        f.write("\n")
    print(path)


if __name__ == "__main__":
    main()
