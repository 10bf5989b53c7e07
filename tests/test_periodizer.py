"""DiffusionPeriodizer on the host: the restatement tests/periodizer_ref.py against what the reference itself produced
(tests/golden/periodizer_cases.npz, tools/make_periodizer_golden.py), the public surface against the reference's signatures, the
plain-Python parts, every refusal of the three ops wrappers through the recording stand-in of tests/abi_trace.py, and the launch
sequence of a planned evaluation through tests/net_trace.py's recorder.  Nothing here runs a kernel.

Bounds: expand and crop are copies -- torch.equal.  The blended outputs are the same fp32 operations in the same order on a cosine
table evaluated here, and a different CPU may round that table by a unit in the last place: rel-L2 < 2e-6, the project's bound for
two routes of one arithmetic (tests/test_gpu_vaenet.py); whether they were equal is printed."""
import ctypes
import inspect
import json
import os

import pytest
import torch

from diffsci_amd import _native as N
from diffsci_amd import ops
from tests import abi_trace, golden_util, net_trace
from tests import periodizer_ref as R
from tests.golden_util import rel_l2

CASES = R.FIELDS + R.VOLUMES
IDS = [R.case_name(*c) for c in CASES]
CROP_BLEND = "ds_crop_blend"


@pytest.fixture(scope="module")
def golden():
    return golden_util.load("periodizer_cases")[0]


# ---------------------------------------------------------------- 1. the restatement against the reference's own results
@pytest.mark.parametrize("k", range(len(CASES)), ids=IDS)
def test_restatement_against_the_reference(golden, k):
    shape, pad, bw = CASES[k]
    name = IDS[k]
    x = golden[name + "/x"]
    assert tuple(x.shape) == shape
    expanded = R.expand(x, pad)
    assert torch.equal(expanded, golden[name + "/expand"])
    assert torch.equal(R.crop(R.analytic_net(expanded), pad, shape[2:]), golden[name + "/crop"])
    for what, got in (("blend", R.blend(x, bw)), ("forward", R.forward(R.analytic_net, x, pad, bw))):
        want = golden[name + "/" + what]
        err = rel_l2(got, want)
        print(f"{name} {what}: rel-L2 {err:.2e}, equal {torch.equal(got, want)}")
        assert got.shape == want.shape and err < 2e-6, (name, what, err)
    if all(b <= 0 or 2 * b >= s for b, s in zip(R.per_axis(bw, len(shape) - 2), shape[2:])):
        assert torch.equal(R.blend(x, bw), x)                                       # every axis skipped: the identity


def test_restated_blend_reads_the_values_before_the_axis_was_blended():
    """A pin of the restatement itself (tests/periodizer_ref.py), which the GPU tests take as the reference; it runs no code of
    the package.  Both strips from the pre-blend values; a later axis blends what the earlier one blended: checked element by element in
    fp64 on a corner, an edge and the interior of a volume."""
    x = R.case_input((1, 1, 5, 6, 7), 3).double()
    got = R.blend(x, (2, 1, 3))
    w = [R.weights(b, torch.float64) for b in (2, 1, 3)]

    def a0(i, j, k):
        m = min(i, 4 - i)
        return float(x[0, 0, i, j, k]) if m >= 2 else float(w[0][m] * x[0, 0, i, j, k] + (1 - w[0][m]) * x[0, 0, 4 - i, j, k])

    def a1(i, j, k):
        m = min(j, 5 - j)
        return a0(i, j, k) if m >= 1 else float(w[1][m] * a0(i, j, k) + (1 - w[1][m]) * a0(i, 5 - j, k))

    def a2(i, j, k):
        m = min(k, 6 - k)
        return a1(i, j, k) if m >= 3 else float(w[2][m] * a1(i, j, k) + (1 - w[2][m]) * a1(i, j, 6 - k))

    for i, j, k in ((0, 0, 0), (4, 5, 6), (1, 0, 2), (2, 3, 3), (3, 2, 5), (0, 3, 3), (2, 5, 3)):
        assert abs(float(got[0, 0, i, j, k]) - a2(i, j, k)) < 1e-14, (i, j, k)
    assert float(got[0, 0, 2, 3, 3]) == float(x[0, 0, 2, 3, 3])


# ---------------------------------------------------------------- 2. the public surface and the plain-Python parts
def test_signatures_are_the_reference_s():
    from diffsci_amd import extra
    with open(os.path.join(golden_util.GOLDEN_DIR, "api_surface_periodizer.json")) as f:
        want = json.load(f)
    sig = lambda fn: str(inspect.signature(fn)).replace("diffsci_amd.", "diffsci.")            # noqa: E731
    for cls in ("DiffusionPeriodizer", "PeriodicSamplerWrapper"):
        for method, s in want[cls].items():
            assert sig(getattr(getattr(extra, cls), method)) == s, (cls, method)
    assert sig(extra.measure_periodicity_error) == want["measure_periodicity_error"]


def test_constructor_normalises_and_refuses_as_the_reference():
    from diffsci_amd.extra import DiffusionPeriodizer
    net = torch.nn.Linear(2, 2)
    p = DiffusionPeriodizer(net, 3)
    assert (p.net, p.pad, p.blend_width, p.dimension) == (net, (3, 3, 3), (8, 8, 8), 3)
    p = DiffusionPeriodizer(net, [1, 2], blend_width=(0, 5), dimension=2)
    assert (p.pad, p.blend_width, p.dimension) == ((1, 2), (0, 5), 2)
    with pytest.raises(AssertionError, match="pad must have 3 elements"):
        DiffusionPeriodizer(net, (1, 2))
    with pytest.raises(AssertionError, match="blend_width must have 2 elements"):
        DiffusionPeriodizer(net, 1, blend_width=(1, 2, 3), dimension=2)
    assert sorted(p.state_dict()) == ["net.bias", "net.weight"]
    with pytest.raises(AssertionError, match="Expected 2D spatial input, got 3D"):
        p.expand_periodic(torch.zeros(1, 1, 2, 2, 2))
    # the crop is the reference's view
    y = torch.arange(2 * 5 * 8.).reshape(1, 2, 5, 8)
    assert torch.equal(p.crop_center(y, (3, 4)), y[:, :, 1:4, 2:6])


def test_sampler_wrapper_counts_steps():
    from diffsci_amd.extra import PeriodicSamplerWrapper

    class Sampler:
        def step(self, x, t, **kw):
            return ("sampler", x, t, kw)

    def periodizer(x, t=None, **kw):
        return ("periodizer", x, t, kw)

    w = PeriodicSamplerWrapper(Sampler(), periodizer, apply_every_n_steps=3)
    assert (w.sampler.__class__, w.periodizer, w.apply_every_n_steps, w._step_count) == (Sampler, periodizer, 3, 0)
    who = [w.step(i, -i, y=7)[0] for i in range(7)]
    assert who == ["sampler", "sampler", "periodizer"] * 2 + ["sampler"] and w._step_count == 7
    assert w.step(1, 2, y=7) == ("sampler", 1, 2, {"y": 7})
    w.reset()
    assert w._step_count == 0 and [w.step(0, 0)[0] for _ in range(3)][-1] == "periodizer"
    assert PeriodicSamplerWrapper(Sampler(), periodizer).step(5, 6, y=1) == ("periodizer", 5, 6, {"y": 1})


def test_measure_periodicity_error():
    from diffsci_amd.extra import measure_periodicity_error
    x = R.case_input((2, 3, 5, 6, 7), 9)
    got, want = measure_periodicity_error(x), R.periodicity_error(x)
    assert sorted(got) == sorted(["mse_H", "mse_W", "mse_D", "max_diff_H", "max_diff_W", "max_diff_D", "total_mse", "mse_per_dim",
                                  "max_diff_per_dim"])
    for k, v in want.items():
        for a, b in zip(got[k] if isinstance(v, list) else [got[k]], v if isinstance(v, list) else [v]):
            assert isinstance(a, float) and abs(a - b) <= 1e-6 * abs(b), k
    assert got["max_diff_per_dim"] == [got["max_diff_H"], got["max_diff_W"], got["max_diff_D"]]
    two = measure_periodicity_error(x[:, :, 0], dimension=2)
    assert "mse_D" not in two and len(two["mse_per_dim"]) == 2 and two["total_mse"] == sum(two["mse_per_dim"])
    per = R.blend(x, 2)                                      # what the blend is for: opposite faces move towards each other
    assert measure_periodicity_error(per)["total_mse"] < got["total_mse"]


# ---------------------------------------------------------------- 3. the ops wrappers: one launch, or none
class Recorder(net_trace.Recorder):
    """ds_crop_blend is no launch by abi_trace.is_launch -- the flags word closes its list, the stream is second to last -- and
    the real entry would launch.  Recorded like one."""

    def __getattr__(self, name):
        if name != CROP_BLEND:
            return super().__getattr__(name)
        types = N._PROTOS[CROP_BLEND][1]

        def launch(*args):
            assert len(args) == len(types), (CROP_BLEND, len(args), len(types))
            self.calls.append([CROP_BLEND] + [self._arg(v, t) for v, t in zip(args, types)])
            return 0
        return launch


def test_crop_blend_closes_its_list_with_the_flags_word():
    res, args = N._PROTOS[CROP_BLEND]
    assert res is ctypes.c_int and args[-1] is ctypes.c_int and args[-2] is ctypes.c_void_p and len(args) == 17
    assert not abi_trace.is_launch(CROP_BLEND)


@pytest.fixture
def rec(monkeypatch):
    r = Recorder(N.lib(), True)
    monkeypatch.setattr(ops, "_off_device", lambda t: None)
    monkeypatch.setattr(N, "lib", lambda: r)
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    return r


def test_periodic_expand_is_one_box_copy(rec):
    x = rec.name("x", R.case_input((2, 3, 6, 7)))
    out = ops.periodic_expand(x, (1, 2))
    assert tuple(out.shape) == (2, 3, 8, 11)
    assert rec.calls == [["ds_box_copy3d", "fresh", ["x", 0], 6, 1, 6, 7, 0, -1, -2, 1, 8, 11, 0, 0, 0, 1, 8, 11, "fresh"]]
    rec.calls.clear()
    v = rec.name("v", R.case_input((1, 2, 3, 4, 5)))
    given = rec.name("out", torch.empty(1, 2, 13, 4, 7))
    assert ops.periodic_expand(v, (5, 0, 1), out=given) is given
    assert rec.calls == [["ds_box_copy3d", ["out", 0], ["v", 0], 2, 3, 4, 5, -5, 0, -1, 13, 4, 7, 0, 0, 0, 13, 4, 7, "fresh"]]
    rec.calls.clear()
    assert tuple(ops.periodic_expand(torch.empty(0, 2, 3, 4), 1).shape) == (0, 2, 5, 6) and rec.calls == []


def test_crop_blend_is_one_launch(rec):
    y = rec.name("y", R.case_input((2, 3, 8, 11)))
    w = ops.blend_weights((2, 3), "cpu")
    assert [tuple(t.shape) for t in w] == [(2,), (3,)] and ops.blend_weights((2, 3), "cpu")[1] is w[1]      # cached
    assert torch.equal(w[1], R.weights(3)) and ops.blend_weights((0, 3, -1), "cpu")[::2] == (None, None)
    rec.name("w1", w[0]), rec.name("w2", w[1])
    out = ops.crop_blend(y, (1, 2), (2, 3))
    assert tuple(out.shape) == (2, 3, 6, 7)
    assert rec.calls == [[CROP_BLEND, "fresh", ["y", 0], 6, 1, 6, 7, 0, 1, 2, 0, 2, 3, None, ["w1", 0], ["w2", 0], "fresh", 0]]
    rec.calls.clear()
    v = rec.name("v", R.case_input((1, 2, 9, 6, 13)))
    given = rec.name("out", torch.empty(1, 2, 5, 6, 7))
    mine = tuple(rec.name(f"t{a}", R.weights(b)) for a, b in enumerate((2, 1, 3)))
    assert ops.crop_blend(v, (2, 0, 3), (2, 1, 3), out=given, weights=mine) is given
    assert rec.calls == [[CROP_BLEND, ["out", 0], ["v", 0], 2, 5, 6, 7, 2, 0, 3, 2, 1, 3, ["t0", 0], ["t1", 0], ["t2", 0], "fresh", 0]]
    rec.calls.clear()
    # widths the kernel skips need no table: 2 bw >= size, and 0
    ops.crop_blend(y, 0, (4, 0), weights=(None, None))
    assert rec.calls == [[CROP_BLEND, "fresh", ["y", 0], 6, 1, 8, 11, 0, 0, 0, 0, 4, 0, None, None, None, "fresh", 0]]


def _bad_expand():
    x, buf = R.case_input((2, 3, 6, 7)), torch.zeros(64)
    return [
        ("no tensor", TypeError, lambda: ops.periodic_expand([1.0], 1)),
        ("fp64", TypeError, lambda: ops.periodic_expand(x.double(), 1)),
        ("rank 3", ValueError, lambda: ops.periodic_expand(x[0], 1)),
        ("rank 6", ValueError, lambda: ops.periodic_expand(x[None, None], 1)),
        ("empty axis", ValueError, lambda: ops.periodic_expand(x[:, :, :0], 1)),
        ("negative pad", ValueError, lambda: ops.periodic_expand(x, (1, -1))),
        ("three pads for a field", ValueError, lambda: ops.periodic_expand(x, (1, 1, 1))),
        ("a float pad", TypeError, lambda: ops.periodic_expand(x, 1.0)),
        ("float pads", ValueError, lambda: ops.periodic_expand(x, (1.0, 2))),
        ("not contiguous", ValueError, lambda: ops.periodic_expand(x.transpose(2, 3), 1)),
        ("out too small", ValueError, lambda: ops.periodic_expand(x, 1, out=torch.empty(2, 3, 8, 8))),
        ("out of another rank", ValueError, lambda: ops.periodic_expand(x, 1, out=torch.empty(6, 8, 9))),
        ("out no tensor", TypeError, lambda: ops.periodic_expand(x, 1, out=[0.0])),
        ("out fp16", TypeError, lambda: ops.periodic_expand(x, 1, out=torch.empty(2, 3, 8, 9, dtype=torch.float16))),
        ("out strided", ValueError, lambda: ops.periodic_expand(x, 1, out=torch.empty(2, 3, 9, 8).transpose(2, 3))),
        ("out shares bytes", ValueError, lambda: ops.periodic_expand(buf[:24].view(1, 1, 4, 6), 1, out=buf[10:58].view(1, 1, 6, 8))),
    ]


def _bad_crop():
    y = R.case_input((2, 3, 8, 11))
    w = (R.weights(2), R.weights(3))
    return [
        ("no tensor", TypeError, lambda: ops.crop_blend(None, 1, 1)),
        ("fp64", TypeError, lambda: ops.crop_blend(y.double(), 1, 1)),
        ("rank 3", ValueError, lambda: ops.crop_blend(y[0], 1, 1)),
        ("negative pad", ValueError, lambda: ops.crop_blend(y, (-1, 1), 1)),
        ("negative width", ValueError, lambda: ops.crop_blend(y, 1, (1, -2))),
        ("three widths for a field", ValueError, lambda: ops.crop_blend(y, 1, (1, 1, 1))),
        ("a float width", TypeError, lambda: ops.crop_blend(y, 1, 2.0)),
        ("pad takes the whole axis", ValueError, lambda: ops.crop_blend(y, (4, 1), 1)),
        ("not contiguous", ValueError, lambda: ops.crop_blend(y.transpose(2, 3), 1, 1)),
        ("out of the uncropped shape", ValueError, lambda: ops.crop_blend(y, (1, 2), (2, 3), out=torch.empty(2, 3, 8, 11))),
        ("out no tensor", TypeError, lambda: ops.crop_blend(y, (1, 2), (2, 3), out=(1,))),
        ("out fp64", TypeError, lambda: ops.crop_blend(y, (1, 2), (2, 3), out=torch.empty(2, 3, 6, 7, dtype=torch.float64))),
        ("out strided", ValueError, lambda: ops.crop_blend(y, (1, 2), (2, 3), out=torch.empty(2, 3, 7, 6).transpose(2, 3))),
        ("out shares bytes", ValueError, lambda: ops.crop_blend(y, (1, 2), (2, 3), out=y.flatten()[:252].view(2, 3, 6, 7))),
        ("no table on a blended axis", ValueError, lambda: ops.crop_blend(y, (1, 2), (2, 3), weights=(w[0], None))),
        ("a short table", ValueError, lambda: ops.crop_blend(y, (1, 2), (2, 3), weights=(w[0], w[1][:2]))),
        ("one table for two axes", ValueError, lambda: ops.crop_blend(y, (1, 2), (2, 3), weights=(w[0],))),
        ("a table of another dtype", TypeError, lambda: ops.crop_blend(y, (1, 2), (2, 3), weights=(w[0], w[1].double()))),
        ("a 2-D table", ValueError, lambda: ops.crop_blend(y, (1, 2), (2, 3), weights=(w[0], w[1][None]))),
    ]


@pytest.mark.parametrize("k", range(len(_bad_expand())))
def test_periodic_expand_refuses_before_any_launch(rec, k):
    what, error, call = _bad_expand()[k]
    with pytest.raises(error):
        call()
    assert rec.calls == [], what


@pytest.mark.parametrize("k", range(len(_bad_crop())))
def test_crop_blend_refuses_before_any_launch(rec, k):
    what, error, call = _bad_crop()[k]
    with pytest.raises(error):
        call()
    assert rec.calls == [], what


@pytest.mark.parametrize("width", [2.0, (2, 3.0), True, (1, False), "3", None])
def test_blend_weights_refuses_widths_that_are_no_ints(rec, width):
    with pytest.raises(TypeError):
        ops.blend_weights(width, "cpu")
    assert rec.calls == []


def test_c_entry_point_refuses_without_launching():
    """ds_crop_blend's own refusals, which the wrapper never lets through: every one returns before the launch, so the real
    entry is called here with host addresses (the manner of tests/test_tiled_sampling.py for ds_box_scatter3d)."""
    import build
    build.build(force=False, verbose=False)
    L = N.lib()
    buf = (ctypes.c_float * 4096)()
    y = ctypes.addressof(buf)
    out, w = y + 4 * 2048, y + 4 * 4000                        # y: 2 planes of 1 x 10 x 12, out: 2 planes of 1 x 6 x 8
    OK, SHAPE, NULL, UNSUPPORTED = 0, -1, -2, -4

    def call(out=out, y=y, planes=2, A=(1, 6, 8), p=(0, 2, 2), bw=(0, 2, 3), tables=(None, w, w), flags=0):
        return L.ds_crop_blend(out, y, planes, *A, *p, *bw, *tables, None, flags)

    assert call(flags=1) == UNSUPPORTED and b"flags" in L.ds_last_error()
    assert call(out=None) == NULL and call(y=None) == NULL
    assert call(p=(0, -1, 2)) == SHAPE and b"negative pad" in L.ds_last_error()
    assert call(bw=(0, 2, -3)) == SHAPE and b"negative blend width" in L.ds_last_error()
    assert call(tables=(None, w, None)) == SHAPE and b"no weight table" in L.ds_last_error()
    assert call(tables=(None, None, w)) == SHAPE
    assert call(A=(1, 0, 8)) == SHAPE and call(planes=-1) == SHAPE
    assert call(out=y + 4 * 100) == SHAPE and b"overlap" in L.ds_last_error()            # out inside y
    assert call(y=out + 4 * 10) == SHAPE and b"overlap" in L.ds_last_error()             # y begins inside out
    assert call(A=(1, 2 ** 30, 8), p=(0, 2 ** 29, 2)) == SHAPE and b"31 bits" in L.ds_last_error()
    # a table is needed on an ACTIVE axis only: width 3 of 6 (2 bw == A) and width 0 are skipped; no planes: nothing is launched
    assert call(planes=0, bw=(0, 3, 0), tables=(None, None, None)) == OK
    assert call(planes=0) == OK


def test_host_tensors_are_refused(monkeypatch):
    r = Recorder(N.lib(), True)
    monkeypatch.setattr(N, "lib", lambda: r)
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    x = R.case_input((1, 1, 4, 4))
    for call in (lambda: ops.periodic_expand(x, 1), lambda: ops.crop_blend(x, 1, 0)):
        with pytest.raises(RuntimeError, match="there is no CPU path"):
            call()
    assert r.calls == []


# ---------------------------------------------------------------- 4. the wrapper and what a plan reads through it
def _wrapped(dim=2, **kw):
    from diffsci_amd.extra import DiffusionPeriodizer
    net, _ = net_trace.punetg(dim, **kw)
    return net, DiffusionPeriodizer(net, 4, 2, dimension=dim)


def test_switches_and_guard_words_are_the_inner_network_s():
    from diffsci_amd.models.karras import engine
    from diffsci_amd.models.nets import precision
    net, per = _wrapped()
    for name in engine.MODEL_SWITCHES:
        assert getattr(per, name, None) == getattr(net, name, None), name
    assert per.dim == net.dim and per.auto_precision is net.auto_precision and per.config is net.config
    per.conv_precision = "bf16x6"                              # what precision.escalate assigns
    assert net.conv_precision == "bf16x6" and "conv_precision" not in per.__dict__
    per.exact_input_layer = True
    assert net.exact_input_layer is True
    net.conv_precision, net.exact_input_layer = "fp16x3", False
    words = precision.guard_words(per, "cpu")
    assert precision.guard_words(net, "cpu") is words and precision.input_layer_flag(net, "cpu").data_ptr() == words.data_ptr()
    assert precision.result_word(per, "cpu").data_ptr() == words[1:2].data_ptr()
    words[1] = 1
    assert precision._read_guard_words(per) == (False, True) and precision._read_guard_words(net) == (False, False)
    # the words first asked of the inner network are found through a wrapper made later
    from diffsci_amd.extra import DiffusionPeriodizer
    net2, _ = net_trace.punetg(2)
    first = precision.guard_words(net2, "cpu")
    assert precision.guard_words(DiffusionPeriodizer(net2, 1, 1, dimension=2), "cpu") is first


def test_plan_key_holds_pad_width_and_dimension():
    from diffsci_amd.extra import DiffusionPeriodizer
    from diffsci_amd.models.karras import engine
    net, per = _wrapped()
    base = engine.model_signature(per)
    assert base[:2] == engine.model_signature(net) and len(engine.model_signature(net)) == 2
    others = [DiffusionPeriodizer(net, 4, 3, dimension=2), DiffusionPeriodizer(net, (4, 2), 2, dimension=2),
              DiffusionPeriodizer(net, 4, (2, 0), dimension=2)]
    sigs = [engine.model_signature(p) for p in others]
    assert len({base, *sigs}) == 4 and all(s[:2] == base[:2] for s in sigs)
    assert engine.model_signature(DiffusionPeriodizer(net, 4, 2, dimension=2)) == base
    net.fuse_norm = not net.fuse_norm
    assert engine.model_signature(per) != base                 # a switch of the inner network, read through the wrapper


def test_protocol_is_offered_only_when_the_inner_network_offers_it():
    from diffsci_amd.extra import DiffusionPeriodizer
    net, per = _wrapped()
    for name in ("forward_with_shifts", "forward_unguarded", "embed_time", "time_shifts", "embed_condition", "condition_is_field"):
        assert callable(getattr(per, name)), name
    assert per.embed_time.__self__ is net and per.capturable is True
    assert not hasattr(per, "field_shifts") and not hasattr(per, "_split_condition")
    plain = DiffusionPeriodizer(torch.nn.Conv2d(1, 1, 3, padding=1), 2, 1, dimension=2)
    for name in ("forward_with_shifts", "forward_unguarded", "embed_time", "dim", "conv_precision"):
        assert getattr(plain, name, None) is None, name
    cond, _ = net_trace.punetg(2, cls="PUNetGCond", cls_args=(None, ["c"]))
    wrapped = DiffusionPeriodizer(cond, 2, 1, dimension=2)
    assert hasattr(cond, "forward_with_shifts") and getattr(wrapped, "forward_with_shifts", None) is None   # evaluated as given
    assert callable(wrapped.forward_unguarded)
    extra, _ = net_trace.punetg(2, cls_args=(None, net_trace.Half()))
    assert DiffusionPeriodizer(extra, 2, 1, dimension=2).capturable is False


class _Planned(torch.nn.Module):
    """An inner network that offers the planned protocol and records the buffers it is handed."""
    conv_precision = "fp32"

    def __init__(self):
        super().__init__()
        self.seen = []

    def forward_with_shifts(self, x, shifts, row=None, out=None):
        self.seen.append((x.data_ptr(), out.data_ptr(), tuple(x.shape), tuple(out.shape)))
        return out


def test_expanded_buffers_are_never_evicted(rec):
    """A captured plan has the addresses of the expanded input and output baked in, and a module keeps several plans: every
    state shape keeps its buffers for the wrapper's life, however many shapes it has seen."""
    import weakref
    from diffsci_amd.extra import DiffusionPeriodizer
    net = _Planned()
    per = DiffusionPeriodizer(net, 2, 1, dimension=2)
    shapes = [(b, 1, 4, 4 + k) for k, b in enumerate((1, 2, 3, 4, 5, 6, 7, 8, 9, 10))]          # more than a PlanCache holds
    for s in shapes:
        out = torch.empty(s[0], 3, *s[2:])
        assert per.forward_with_shifts(torch.zeros(s), None, row=0, out=out) is out
    first = net.seen[:len(shapes)]
    assert [f[2:] for f in first] == [((s[0], 1, 8, s[3] + 4), (s[0], 3, 8, s[3] + 4)) for s in shapes]
    alive = [weakref.ref(t) for t in per._expanded.values()]
    assert len(alive) == 2 * len(shapes) and len({f[0] for f in first} | {f[1] for f in first}) == 2 * len(shapes)
    for s in shapes:                                                  # the second visit: the first visit's addresses
        per.forward_with_shifts(torch.zeros(s), None, row=0, out=torch.empty(s[0], 3, *s[2:]))
    assert net.seen[len(shapes):] == first and all(r() is not None for r in alive)
    # input and output of the same shape are two buffers
    net.seen.clear()
    per.forward_with_shifts(torch.zeros(2, 3, 4, 4), None, out=torch.empty(2, 3, 4, 4))
    assert net.seen[0][0] != net.seen[0][1] and net.seen[0][2] == net.seen[0][3]
    assert [c[0] for c in rec.calls].count("ds_box_copy3d") == 2 * len(shapes) + 1


def test_pad_and_net_assigned_after_construction(rec):
    """pad is part of the plan key because it may be assigned later: the buffers follow the EXPANDED shape.  A new inner network
    brings its own guard words, and only attributes the inner network has are written to it."""
    from diffsci_amd.extra import DiffusionPeriodizer
    from diffsci_amd.models.nets import precision
    net = _Planned()
    per = DiffusionPeriodizer(net, 2, 1, dimension=2)
    x, out = torch.zeros(1, 1, 4, 4), torch.empty(1, 1, 4, 4)
    per.forward_with_shifts(x, None, out=out)
    per.pad = (1, 1)
    per.forward_with_shifts(x, None, out=out)
    per.pad = (2, 2)
    per.forward_with_shifts(x, None, out=out)
    assert [s[2] for s in net.seen] == [(1, 1, 8, 8), (1, 1, 6, 6), (1, 1, 8, 8)] and net.seen[0][:2] == net.seen[2][:2]
    assert rec.calls[-1][:13] == [CROP_BLEND, "fresh", "fresh", 1, 1, 4, 4, 0, 2, 2, 0, 1, 1]
    assert rec.calls[-3][:13] == [CROP_BLEND, "fresh", "fresh", 1, 1, 4, 4, 0, 1, 1, 0, 1, 1]
    words = precision.guard_words(per, "cpu")
    other = _Planned()
    per.net = other
    assert per.net is other and precision.guard_words(per, "cpu") is precision.guard_words(other, "cpu")
    assert precision.guard_words(per, "cpu") is not words and precision.guard_words(net, "cpu") is words
    per.conv_precision = "bf16x6"                                      # the inner network's own attribute
    assert other.__dict__["conv_precision"] == "bf16x6" and "conv_precision" not in per.__dict__
    # what the inner network never had stays on the wrapper
    plain = torch.nn.Conv2d(1, 1, 3, padding=1)
    wrapped = DiffusionPeriodizer(plain, 2, 1, dimension=2)
    wrapped.config, wrapped.conv_precision, wrapped.dim = "mine", "fp32", 2
    assert not any(hasattr(plain, n) for n in ("config", "conv_precision", "dim"))
    assert (wrapped.config, wrapped.conv_precision, wrapped.dim) == ("mine", "fp32", 2)
    assert sorted(wrapped.state_dict()) == ["net.bias", "net.weight"]


# ---------------------------------------------------------------- 5. the launch sequence of a planned evaluation
def _trace(dim, side, run):
    rec = Recorder(N.lib(), True)
    pool = net_trace.Pool(rec)
    saved = [(N, "lib", N.lib), (ops, "_stream", ops._stream), (ops, "_off_device", ops._off_device)]
    try:
        N.lib, ops._stream, ops._off_device = (lambda: rec), (lambda: 0), (lambda t: None)
        c = net_trace.Net(rec, pool, dim=dim, side=side)
        del rec.calls[:]                                      # the weight packing of the construction is not the evaluation's
        run(c)
    finally:
        for mod, attr, v in saved:
            setattr(mod, attr, v)
    return rec.calls


@pytest.mark.parametrize("dim,side,pad", [(2, 8, 4), (3, 4, 2)], ids=["2d", "3d"])
def test_planned_evaluation_is_expand_network_crop(dim, side, pad):
    """One ds_box_copy3d, the inner network's own launches at the expanded shape, one ds_crop_blend; the middle equals the trace
    of the bare network at that shape (its input and output buffers are unnamed in both)."""
    from diffsci_amd.extra import DiffusionPeriodizer
    big = side + 2 * pad

    def wrapped(c):
        per = DiffusionPeriodizer(c.net, pad, 1, dimension=dim)
        shifts = [c.f(f"shift{k}", 5, C) for k, C in enumerate(c.widths())]
        out = c.x(c.net.config.output_channels, "out")
        assert per.forward_with_shifts(c.x(), shifts, row=3, out=out) is out

    def bare(c):
        shifts = [c.f(f"shift{k}", 5, C) for k, C in enumerate(c.widths())]
        cin, cout = c.net.config.input_channels, c.net.config.output_channels
        c.net.forward_with_shifts(torch.empty(net_trace.B, cin, *[big] * dim), shifts, row=3,
                                  out=torch.empty(net_trace.B, cout, *[big] * dim))

    got, want = _trace(dim, side, wrapped), _trace(dim, big, bare)
    assert got[0][0] == "ds_box_copy3d" and got[-1][0] == CROP_BLEND
    assert [c[0] for c in got].count("ds_box_copy3d") == 1 + [c[0] for c in want].count("ds_box_copy3d")
    assert [c[0] for c in got].count(CROP_BLEND) == 1
    assert len(want) > 20 and got[1:-1] == want
    lead = 3 - dim
    S, E, p = [1] * lead + [side] * dim, [1] * lead + [big] * dim, [0] * lead + [pad] * dim
    planes_in, planes_out = net_trace.B * 2, net_trace.B * 1
    assert got[0] == ["ds_box_copy3d", "fresh", ["x", 0], planes_in, *S, *[-v for v in p], *E, 0, 0, 0, *E, "fresh"]
    assert got[-1][:13] == [CROP_BLEND, ["out", 0], "fresh", planes_out, *S, *p, *([0] * lead + [1] * dim)]
    assert got[-1][-2:] == ["fresh", 0]                       # the stream, then the flags word
