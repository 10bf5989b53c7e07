"""The attention core's tile loop (k_attn3h, ds_attn3h.hip) against fp64 at the smallest shapes that reach every
path of the loop: E = 256 at L = 32 (one key tile), 64 (two tiles: the first pair whose S^T product runs under the other's
softmax) and 160 (a second query block with one wave that stores and three that recompute); E = 32 at L = 96; (E, H) = (512, 2)
at L = 32 for the form with a head axis.  B = 1 and 3, the image form and the form that stages in the workgroup, with the
exponent rows and without (NULL).  At B = 3 sample 1 has q and k scaled by 2^-6.

Data: Gaussian, and the staircase logits of tests/test_gpu_attention_edges.py (c = 5: the deferred rescale moves on some tiles).
Reference: fp64 softmax(q^T k / sqrt(d)) v per sample and head, computed once per case.
Bounds.  (1) check_rows of tests/test_gpu_attention_edges.py on every (sample, head) row: rel-L2 <= max(4 x torch fp32's, 1e-7),
max-abs <= max(4 x torch fp32's, one ulp of max |ref|).  (2) Over the whole output, rel-L2 and max-abs against fp64 at most 1.5 x
what the kernel measured before the loop was restructured, on these inputs (tests/golden/attn_core_parent_errors.json, written by
tools/attn_core_errors.py; profiles/attn_core.log): the margin is for fp32 sums in another order, and a lost lo-piece product
costs a factor of 2^11.  (3) The two forms agree bit for bit, as everywhere else in the suite."""
import json
import os

import pytest
import torch

from tests.golden_util import rel_l2
from tests.test_gpu_attention_edges import _heads_form, _in_amax, _sdpa, _staircase, check_rows

pytestmark = pytest.mark.gpu

SHAPES = [(256, 1, 32), (256, 1, 64), (256, 1, 160), (32, 1, 96), (512, 2, 32)]        # (E, H, L)
PARENT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attn_core_parent_errors.json")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def case_id(E, H, L, B, data):
    return f"E{E}-H{H}-L{L}-B{B}-{data}"


def make_input(E, H, L, B, data):
    """qkv [B, 3E, L] on the CPU, from a seed of its own; at B > 1 sample 1 has q and k times 2^-6."""
    seed = 7 * E + 5 * H + 3 * L + B
    if data == "gauss":
        qkv = torch.randn(B, 3 * E, L, generator=torch.Generator().manual_seed(seed))
    else:
        qkv = _staircase(E, H, L, B, 5, seed)
    if B > 1:
        qkv[1, :2 * E] *= 2.0 ** -6
    return qkv.contiguous()


def run_case(ops, N, qkv, E, H, dev):
    """{rows | null: output} of both forms, which must agree bit for bit."""
    x = qkv.to(dev)
    outs = {}
    for key, rows in (("rows", _in_amax(ops, x, E)), ("null", None)):
        staged = _heads_form(N, x, E, H, False, rows, None)
        image = _heads_form(N, x, E, H, True, rows, None)
        assert torch.isfinite(staged).all() and torch.isfinite(image).all(), f"{key}: a query was not stored"
        assert torch.equal(staged, image), f"{key}: staged and image forms differ"
        outs[key] = image.cpu()
    return outs


def errors(got, want):
    """(rel-L2, max-abs) of the whole output against fp64."""
    return rel_l2(got, want), float((got.double() - want).abs().max())


@pytest.mark.parametrize("data", ["gauss", "staircase"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("E,H,L", SHAPES)
def test_tile_loop_vs_fp64(dev, E, H, L, B, data):
    from diffsci_amd import _native as N
    from diffsci_amd import ops
    parent = json.load(open(PARENT))["errors"]
    qkv = make_input(E, H, L, B, data)
    want = _sdpa(qkv, E, H, torch.float64)
    for key, got in run_case(ops, N, qkv, E, H, dev).items():
        what = f"{case_id(E, H, L, B, data)} {key}"
        check_rows(what, got, qkv, E, H)
        e_rel, e_abs = errors(got, want)
        p_rel, p_abs = parent[f"{case_id(E, H, L, B, data)}-{key}"]
        print(f"[core] {what}: rel-L2 {e_rel:.3e} (before {p_rel:.3e}, x{e_rel / p_rel:.2f}); max-abs {e_abs:.3e} "
              f"(before {p_abs:.3e}, x{e_abs / p_abs:.2f})")
        assert e_rel <= 1.5 * p_rel and e_abs <= 1.5 * p_abs, what
