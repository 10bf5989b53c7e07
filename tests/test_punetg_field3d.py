"""Field-valued conditional embeddings on volumes (dimension=3 PUNetG): the corner-pool binding, the wrapper's refusals and the
N-D compatibility rule of _FieldShifts.level -- host-side only, no GPU needed (every check runs before any device use)."""
import os

import pytest
import torch

import diffsci_amd.models as M
from diffsci_amd import _native as N
from diffsci_amd import ops
from diffsci_amd.models.nets.punetg import _FieldShifts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_binding_exports_the_corner_pool():
    assert "ds_cornerpool_f" in N.exported_symbols()
    assert "ds_cornerpool_f" in N._PROTOS
    header = open(os.path.join(ROOT, "include", "diffsci_hip.h")).read()
    assert "int ds_cornerpool_f(float* out, const float* x, const float* te, unsigned* out_amax," in header


def test_kernel_source_is_in_the_resampling_file():
    src = open(os.path.join(ROOT, "diffsci_amd", "csrc", "ds_resample.hip")).read()
    assert 'extern "C" int ds_cornerpool_f(' in src and "k_cornerpool_f" in src


@pytest.mark.parametrize("shape", [(1, 4, 8), (4, 8), (1, 1, 2, 2, 2, 2)])
def test_wrapper_refuses_other_ranks(shape):
    with pytest.raises(ValueError, match="fields"):
        ops.cornerpool_f(torch.zeros(shape), 2)


@pytest.mark.parametrize("shape,f", [((1, 2, 8, 6), 4), ((1, 2, 9, 8), 2), ((1, 2, 8, 8, 6), 4), ((2, 1, 6, 6, 6), 4)])
def test_wrapper_refuses_sides_that_do_not_divide(shape, f):
    with pytest.raises(ValueError, match="divide"):
        ops.cornerpool_f(torch.zeros(shape), f)


@pytest.mark.parametrize("bad", [0, -2, True, False, 1.5, "2", None])
def test_wrapper_refuses_bad_factors(bad):
    with pytest.raises(ValueError, match="factor"):
        ops.cornerpool_f(torch.zeros(1, 1, 4, 4, 4), bad)


@pytest.mark.parametrize("te", [(3,), (1, 2), (1, 3, 1), (3, 3)])
def test_wrapper_refuses_a_te_of_the_wrong_shape(te):
    with pytest.raises(ValueError, match="te|batch"):
        ops.cornerpool_f(torch.zeros(2, 3, 4, 4, 4), 2, te=torch.zeros(te))


def test_wrapper_refuses_a_wrong_out_before_any_launch(monkeypatch):
    calls = []
    monkeypatch.setattr(N, "lib", lambda: calls.append(1))
    with pytest.raises(ValueError, match="out has shape"):
        ops.cornerpool_f(torch.zeros(2, 3, 4, 4, 4), 2, out=torch.zeros(2, 3, 2, 2, 4))
    with pytest.raises(ValueError, match="batch"):
        ops.cornerpool_f(torch.zeros(2, 3, 4, 4, 4), 2, out=torch.zeros(3, 3, 2, 2, 2))
    assert not calls


def test_cpu_tensors_are_refused_after_the_shape_checks():
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.cornerpool_f(torch.zeros(1, 1, 4, 4, 4), 2)


def test_level_takes_three_sizes_and_keeps_the_reference_rule():
    """rescale_yt: the factor comes from the first side, every side must satisfy block * f == field; a coarser field is the
    reference's broken upscaling branch."""
    fs = _FieldShifts(torch.zeros(1, 8, 16, 16, 16), None, False, rows=None, batch=2)
    with pytest.raises(ValueError, match=r"yt_dims \(16, 16, 16\) and y_dims \(8, 8, 4\)"):
        fs.level(8, 8, 4)
    with pytest.raises(ValueError, match=r"yt_dims \(16, 16, 16\) and y_dims \(5, 5, 5\)"):
        fs.level(5, 5, 5)
    with pytest.raises(ValueError, match="not compatible"):
        fs.level(8, 8)                                               # a field's sizes against a volume
    with pytest.raises(NotImplementedError, match="coarser"):
        fs.level(32, 32, 32)
    with pytest.raises(NotImplementedError, match="coarser"):
        fs.level(16, 32, 16)
    fs2 = _FieldShifts(torch.zeros(1, 8, 8, 8), None, False)         # the 2-D form keeps its signature and its refusals
    with pytest.raises(NotImplementedError, match="coarser"):
        fs2.level(16, 16)
    with pytest.raises(ValueError, match=r"yt_dims \(8, 8\) and y_dims \(4, 2\)"):
        fs2.level(4, 2)


def _net3(**over):
    return M.PUNetG(M.PUNetGConfig(model_channels=8, dimension=3, **over), conditional_embedding=torch.nn.Identity())


def test_embed_condition_checks_rank_and_channels_on_the_host():
    net3, net2 = _net3(), M.PUNetG(M.PUNetGConfig(model_channels=8), conditional_embedding=torch.nn.Identity())
    with pytest.raises(ValueError, match="rank 5"):
        net3.embed_condition(torch.zeros(1, 8, 16, 16))              # a 2-D field on a volume network
    with pytest.raises(ValueError, match="rank 4"):
        net2.embed_condition(torch.zeros(1, 8, 16, 16, 16))
    with pytest.raises(ValueError, match="rank 5"):
        net3.embed_condition(torch.zeros(1, 8, 16))
    for net, shape in ((net3, (1, 4, 8, 8, 8)), (net2, (1, 4, 8, 8))):
        with pytest.raises(ValueError, match="model_channels channels"):
            net.embed_condition(torch.zeros(shape))
    with pytest.raises(RuntimeError, match="no CPU path"):           # a well-formed volume field gets as far as the device check
        net3.embed_condition(torch.zeros(1, 8, 8, 8, 8))
    assert net3.embed_condition(torch.zeros(2, 8)).shape == (2, 8)   # vectors as before
