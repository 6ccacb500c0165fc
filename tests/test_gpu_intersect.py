"""The kernels' ray-scene intersection, one ray at a time (rt_test_intersect: intersect_scene of the product sources in the
test library), against the oracle (oracle.intersect: calculate_ray_collions, wgsl:353-396) bit for bit, on the ray
families of tests/_ray_families.py, under every configuration of the walk the options reach.

What images cannot tell apart and this can:
  * rays no camera aims: signed-zero axis directions from the scene's own box planes, shared edges and vertices, the
    determinant at the cull threshold, origins around EPSILON, sphere tangents and insides, equal-distance ties across
    meshes (isect_offer's index clause), mirrored / sheared transforms, every item kind and stack / BVH-height boundary;
  * the lane layout: the same rays permuted, with all lanes active, a random half, or one lane per wave give the same
    bits per ray (the wave-cooperative loops: the vote's ballots, the readfirstlane item streams);
  * the instantiation: the probe reports the kernel it ran, and it is the one a render of that configuration takes.
With option cross_prune = 1 (opt-in, not exact) the differences from the oracle are reported, not asserted."""
import numpy as np
import pytest

import _ray_families as RF
from oracle import independent_f64 as F

pytestmark = pytest.mark.gpu

N_RANDOM = 100000
N_F64 = 4000   # random rays per scene also checked against the float64 reference, straight from the kernel

# option sets (each applied before a fresh upload of the scene; the defaults restored afterwards)
CONFIGS = [{}, {"lds_scene": 0}, {"stack_wide": 0}, {"stack_wide": 1}, {"lds_scene": 0, "stack_wide": 1},
           {"lds_scene": 0, "stack_wide": 0}, {"forest": 0}, {"flat2": 0}, {"forest": 0, "flat2": 0, "lds_scene": 0},
           {"tlas": 0}, {"tlas": 0, "lds_scene": 0}, {"tlas_min": 2}, {"cull_roots": 0}, {"cull_roots": 1},
           {"cull_roots": 1, "lds_scene": 0, "tlas": 0}]
DEFAULTS = {"lds_scene": 1, "stack_wide": -1, "forest": 1, "flat2": 1, "tlas": 1, "tlas_min": 8, "cull_roots": -1,
            "cross_prune": 0}
# the instantiation word of a record (include/rt_test_abi.h)
ISECT_TLAS, ISECT_SIMPLE, ISECT_STATS, ISECT_LDS = 1, 2, 32, 64


def same_bits(got, want, what):
    """Records equal word for word; a NaN float equals any NaN (test_gpu_device_units.same_bits: NaN sign and payload
    are outside the arithmetic contract).  Word 14 (which kernel ran) is checked apart."""
    g, w = got.copy(), want.copy()
    g[:, 14:] = 0
    w[:, 14:] = 0
    is_float = np.zeros(g.shape[1], bool)
    is_float[1:10] = True
    nan = ((g & 0x7fffffff) > 0x7f800000) & ((w & 0x7fffffff) > 0x7f800000) & is_float[None, :]
    bad = np.flatnonzero(((g != w) & ~nan).any(1))
    assert bad.size == 0, (f"{what}: {bad.size} of {len(g)} rays differ, first {bad[0]}: kernel {got[bad[0]].tolist()} "
                           f"oracle {want[bad[0]].tolist()}")


@pytest.fixture(scope="module")
def probe(rt):
    t = rt.RayTracer(device=0, max_width=64, max_height=64, lib=rt.load_test())
    yield t
    t.close()


def _set(t, opts):
    for k, v in {**DEFAULTS, **opts}.items():
        t.set_option(k, v)


def _launch_kind(rt, t):
    """What a render of the loaded scene under the current options launches (rt_last_launch)."""
    t.render(rt.make_params(16, 16, 1, 1, skybox=1, frames=0))
    t.synchronize()
    return t.last_launch()


def _plain(arrays):
    return len(arrays.spheres) == 0 and all(int(m["material"]["flag"]) == 0 for m in arrays.meshes)


def _all_rays(fams):
    return np.concatenate([v[0] for v in fams.values()]), np.concatenate([v[1] for v in fams.values()])


@pytest.mark.parametrize("name", RF.LIBRARY + RF.BUILT)
def test_probe_equals_the_oracle_bit_for_bit_in_every_configuration(rt, oracle, probe, name):
    arrays = RF.scene(rt, name)
    fams = RF.families(arrays, name, n_random=N_RANDOM)
    ro, rd = _all_rays(fams)
    want = oracle.intersect(arrays, ro, RF.normalized(rd))   # (the probe normalizes rd the same way)
    variants = [dict(), dict(general=True), dict(stats=True), dict(stats=True, general=True)]
    if _plain(arrays):
        variants += [dict(simple=True), dict(simple=True, stats=True)]
    seen = set()
    try:
        for cfg in CONFIGS:
            _set(probe, cfg)
            probe.load_scene(arrays)
            kind = _launch_kind(rt, probe)
            for var in variants:
                if var.get("simple") and kind["many_mesh"]:
                    with pytest.raises(rt.RtError):   # (the many-mesh kernels have no SIMPLE instantiation)
                        probe.intersect(ro[:1], rd[:1], **var)
                    continue
                got = probe.intersect(ro, rd, **var)
                if var.get("stats"):
                    same_bits(got, want, f"{name} {cfg} {var}")
                else:   # (the product instantiations do not count tests)
                    same_bits(got[:, :12], want[:, :12], f"{name} {cfg} {var}")
                b = int(got[0, 14])
                assert np.all(got[:, 14] == b), (name, cfg, var)
                assert bool(b & ISECT_TLAS) == kind["many_mesh"], (name, cfg, var, b, kind)
                assert bool(b & ISECT_LDS) == kind["scene_in_lds"], (name, cfg, var, b, kind)
                assert bool(b & ISECT_STATS) == bool(var.get("stats")), (name, cfg, var, b)
                if var.get("simple"):
                    assert b & ISECT_SIMPLE, (name, cfg, var, b)
                elif var.get("general") or var.get("stats"):
                    assert not b & ISECT_SIMPLE, (name, cfg, var, b)
                else:   # the instantiation the render took
                    assert bool(b & ISECT_SIMPLE) == kind["specialised"], (name, cfg, b, kind)
                seen.add(b)
    finally:
        _set(probe, {})
    counts = ", ".join(f"{k} {len(v[0])}" for k, v in fams.items())
    print(f"\n{name}: {len(ro)} rays ({counts}); instantiations run: {sorted(seen)}")


@pytest.mark.parametrize("name", ["cornell", "dragon", "sponza", "room", "items", "ties", "ties_tlas", "cull17", "leaf128",
                                  "height33"])
@pytest.mark.parametrize("cfg", [{}, {"lds_scene": 0}], ids=["default", "global"])
def test_records_do_not_depend_on_the_lane_layout(rt, probe, name, cfg):
    """The same rays in a random order, with every lane active, a random half, or one lane per wave (64 rays): every
    ray's record is the one it gets in order with all lanes active."""
    arrays = RF.scene(rt, name)
    ro, rd = _all_rays(RF.families(arrays, name, n_random=20000))
    rng = np.random.default_rng(sum(map(ord, name)))
    try:
        _set(probe, cfg)
        probe.load_scene(arrays)
        for var in (dict(), dict(stats=True)):
            base = probe.intersect(ro, rd, **var)
            perm = rng.permutation(len(ro))
            for layout in ("all", "half", "one_per_wave"):
                if layout == "all":
                    a = np.ones(len(ro), np.uint8)
                elif layout == "half":
                    a = (rng.uniform(size=len(ro)) < 0.5).astype(np.uint8)
                else:
                    a = np.zeros(len(ro), np.uint8)
                    a[int(rng.integers(0, 64))::64] = 1
                got = probe.intersect(ro[perm], rd[perm], active=a, **var)
                on = a == 1
                same_bits(got[on], base[perm][on], f"{name} {cfg} {var} {layout}")
                assert not got[~on].any(), "an inactive lane wrote its record"
    finally:
        _set(probe, {})


@pytest.mark.parametrize("name", RF.LIBRARY + ["items", "xforms", "glass", "cull16", "leaf128", "height32"])
def test_kernel_agrees_with_the_f64_reference_off_the_ambiguous_rays(rt, probe, name):
    """Every family (random rays: a sample) straight from the kernel against the float64 brute force -- the comparison
    of tests/test_intersect_oracle_f64.py without the oracle in between."""
    import test_intersect_oracle_f64 as T
    arrays = RF.scene(rt, name)
    ro, rd = _all_rays(RF.families(arrays, name, n_random=N_F64))
    try:
        _set(probe, {})
        probe.load_scene(arrays)
        got = probe.intersect(ro, rd)
    finally:
        _set(probe, {})
    c = T.compare(arrays, got, ro, RF.normalized(rd), F.Scene(arrays))
    assert c["bad"].size == 0, (name, c["bad"][:5])
    print(f"\n{name}: {c['rays']} rays, {c['ambiguous']} ambiguous, {c['deep_misses']} lost to the clamped stack")


@pytest.mark.parametrize("name", ["sponza", "cull17", "ties_tlas", "tlas9"])
def test_cross_prune_differences_are_reported(rt, oracle, probe, name):
    """Option cross_prune = 1 is opt-in and not exact: its differences from the oracle are printed."""
    arrays = RF.scene(rt, name)
    fams = RF.families(arrays, name, n_random=N_RANDOM)
    out = []
    try:
        _set(probe, {"cross_prune": 1})
        probe.load_scene(arrays)
        for fam, (ro, rd) in fams.items():
            want = oracle.intersect(arrays, ro, RF.normalized(rd))
            got = probe.intersect(ro, rd)
            out.append(f"{fam} {int((got[:, :12] != want[:, :12]).any(1).sum())}/{len(ro)}")
    finally:
        _set(probe, {})
    print(f"\n{name} cross_prune = 1, rays differing from the oracle: " + ", ".join(out))


def test_the_probe_refuses_what_a_render_cannot_trace(rt, probe, cornell):
    probe.load_scene(cornell)
    with pytest.raises(ValueError):
        probe.intersect([[0, 1, 3]], [[0, 0, 0]])
    with pytest.raises(ValueError):
        probe.intersect([[np.inf, 1, 3]], [[0, 0, -1]])
    L, h = probe._L, probe._h
    ro = np.array([[0, 1, 3]], np.float32)
    rd = np.array([[0, 0, 0]], np.float32)
    out = np.zeros((1, 16), np.uint32)
    assert L.rt_test_intersect(h, ro.ctypes.data, rd.ctypes.data, None, 1, 0, out.ctypes.data) == -1   # zero direction
    rd[0, 2] = np.nan
    assert L.rt_test_intersect(h, ro.ctypes.data, rd.ctypes.data, None, 1, 0, out.ctypes.data) == -1   # NaN
    rd[0, 2] = -1.0
    assert L.rt_test_intersect(h, ro.ctypes.data, rd.ctypes.data, None, 1, 8, out.ctypes.data) == -1   # unknown flag
    assert L.rt_test_intersect(h, ro.ctypes.data, rd.ctypes.data, None, 1, 5, out.ctypes.data) == -1   # general + SIMPLE
    assert L.rt_test_intersect(h, ro.ctypes.data, rd.ctypes.data, None, 1 << 25, 0, out.ctypes.data) == -2   # too many
    assert not out.any()
    probe.load_scene(RF.scene(rt, "room"))
    with pytest.raises(rt.RtError):   # spheres: no SIMPLE instantiation for this scene
        probe.intersect([[0, 1, 3]], [[0, 0, -1]], simple=True)
