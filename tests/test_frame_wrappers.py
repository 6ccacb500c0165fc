"""The plane checks of the six frame-pass wrappers of RayTracer (denoise, denoise_variance, luminance_moments,
temporal_accumulate, adaptive_plan, adaptive_merge): each refuses, with a ValueError and before any library call, a mix of
tensors and arrays, a tensor off the handle's device, and a tensor of the wrong shape, dtype or layout; and color=None with
numpy planes.  No device: a tensor "on cuda:0" is a CPU tensor that says so, and the handle has no library."""
import numpy as np
import pytest
import torch

W, H = 4, 3
BUDGET = 2 * W * H


class OnDevice(torch.Tensor):
    """A CPU tensor that reports cuda:0 as its device: what the wrappers' checks read, and nothing gets past them here."""
    device = property(lambda self: torch.device("cuda", 0))


def on_device(a):
    return (a if isinstance(a, torch.Tensor) else torch.from_numpy(a)).as_subclass(OnDevice)


def _frame():
    rng = np.random.default_rng(11)
    f = lambda *s: rng.random(s, np.float32)  # noqa: E731
    i = lambda *s: rng.integers(0, 3, s).astype(np.int32)  # noqa: E731
    return {"color": f(H, W, 4), "normal": f(H, W, 3), "point": f(H, W, 3), "albedo": f(H, W, 4), "emission": f(H, W, 4),
            "object": i(H, W), "moments": f(H, W, 4), "history": f(H, W), "prev_color": f(H, W, 4), "prev_history": f(H, W),
            "variance": f(H, W), "dir": f(H, W, 3), "counts": i(H, W), "offsets": i(H, W), "radiance": f(BUDGET, 4)}


def _camera():
    from ray_tracer_2_amd import _abi as A
    return A.CameraUniform()


def _guides(p):
    return {k: p[k] for k in ("normal", "point", "albedo", "emission")}


def _temporal_guides(p):
    return {k: p[k] for k in ("point", "normal", "object")}


# wrapper -> (the call on a dict of planes, the plane the cases spoil: not the one the frame's size is read from)
WRAPPERS = {
    "denoise": (lambda t, p: t.denoise(_guides(p), p["color"]), "point"),
    "denoise_variance": (lambda t, p: t.denoise_variance(_guides(p), p["color"], moments=p["moments"], history=p["history"]), "history"),
    "luminance_moments": (lambda t, p: t.luminance_moments(_guides(p), p["color"]), "albedo"),
    "temporal_accumulate": (lambda t, p: t.temporal_accumulate(_temporal_guides(p), _temporal_guides(p), _camera(), p["prev_color"],
                                                               p["prev_history"], p["color"]), "prev_history"),
    "adaptive_plan": (lambda t, p: t.adaptive_plan(p["variance"], p["dir"], (0.0, 0.0, 1.0), BUDGET), "dir"),
    "adaptive_merge": (lambda t, p: t.adaptive_merge(p["radiance"], p["counts"], p["offsets"], p["color"], p["history"]), "history"),
}


def _wider(a):
    return np.concatenate([a, a[:, :1]], axis=1)


def _strided(a):
    """The same shape and values, every second element of a buffer twice as long in the last axis."""
    return on_device(torch.from_numpy(np.repeat(a, 2, axis=-1).copy()))[..., ::2]


CASES = {
    "a mix of a tensor and arrays": (None, False, "mix of device tensors and host arrays"),
    "a tensor on the CPU": (lambda a: torch.from_numpy(a), True, "must be on cuda:0"),
    "a wrong shape": (lambda a: on_device(_wider(a)), True, "shape"),
    "a wrong dtype": (lambda a: on_device(a.astype(np.float64)), True, "tensor of shape"),
    "a non-contiguous tensor": (_strided, True, "contiguous"),
}


@pytest.fixture
def tracer(rt):
    t = rt.RayTracer.__new__(rt.RayTracer)   # (no handle: the checks come before any library call)
    t._L, t._h, t.device = None, None, 0
    return t


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("wrapper", list(WRAPPERS))
def test_device_planes_are_checked_before_any_library_call(tracer, wrapper, case):
    call, victim = WRAPPERS[wrapper]
    spoil, others_on_device, text = CASES[case]
    p = _frame()
    assert not _strided(p[victim]).is_contiguous() and tuple(_strided(p[victim]).shape) == p[victim].shape
    if others_on_device:
        planes = dict({k: on_device(v) for k, v in p.items()}, **{victim: spoil(p[victim])})
    else:   # the mix: one tensor among arrays
        planes = dict(p, **{victim: on_device(p[victim])})
    with pytest.raises(ValueError, match=text):
        call(tracer, planes)


@pytest.mark.parametrize("wrapper", [w for w in WRAPPERS if w != "adaptive_plan"])   # (the plan has no colour plane)
def test_color_none_needs_device_planes(tracer, wrapper):
    call, _ = WRAPPERS[wrapper]
    with pytest.raises(ValueError, match="color is required with numpy planes"):
        call(tracer, dict(_frame(), color=None))


@pytest.mark.parametrize("wrapper", list(WRAPPERS))
def test_good_device_planes_reach_the_library(tracer, wrapper):
    """The cases above fail for the reason they name: with every plane in order nothing is refused, and the call goes on to
    what this test cannot give it (a device for the outputs, then the library)."""
    call, _ = WRAPPERS[wrapper]
    with pytest.raises(Exception) as e:
        call(tracer, {k: on_device(v) for k, v in _frame().items()})
    assert not isinstance(e.value, ValueError), e.value
