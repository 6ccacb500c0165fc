"""The kernels' shading step, one hit at a time (rt_test_shade: path_end and roulette_skip of the product sources in the test
library), against the oracle (oracle.shade: the body of trace's loop, wgsl:405-468, with path_end's bookkeeping) bit for
bit, on the case families of tests/_shade_cases.py, in every instantiation of path_end the options and the probe's flags
reach -- and straight against the float64 restatement (independent_f64.scatter).

What images and radiance queries cannot tell apart and this can: WHICH hit went wrong.  The families sit on the inputs a
random image almost never reaches -- the critical angle from both of its tests, a cosine rounding past +-1, draws of
exactly 0.0 and 1.0 at every decision, roulette probabilities of 0, 1, subnormal and 2^120, NaN and negative channels,
glass of ior 1, < 1, 0, inf and NaN, texture coordinates far outside [0, 1) and non-finite, every bookkeeping boundary.
Outside the probe: the vote, the memo (FAST_MISS's shortcut reads it), park / resume and the refill.
"""
import time

import numpy as np
import pytest

import _shade_cases as SC
from oracle import independent_f64 as F

pytestmark = pytest.mark.gpu

DEFAULTS = {"lds_scene": 1, "tlas": 1}
FLOAT_WORDS = np.zeros(32, bool)
FLOAT_WORDS[0:18] = True


def same_bits(got, want, what, words=slice(0, 25)):
    """Records equal word for word; a NaN float equals any NaN (test_gpu_device_units.same_bits: NaN sign and payload are
    outside the arithmetic contract).  Word 25 (which kernel ran) is checked apart; the words behind it are zero."""
    g, w = got[:, words], want[:, words]
    nan = ((g & 0x7fffffff) > 0x7f800000) & ((w & 0x7fffffff) > 0x7f800000) & FLOAT_WORDS[words][None, :]
    bad = np.flatnonzero(((g != w) & ~nan).any(1))
    assert bad.size == 0, (f"{what}: {bad.size} of {len(g)} cases differ, first {bad[0]}: kernel {got[bad[0]].tolist()} "
                           f"oracle {want[bad[0]].tolist()}")


@pytest.fixture(scope="module")
def probe(rt):
    t = rt.RayTracer(device=0, max_width=64, max_height=64, lib=rt.load_test())
    yield t
    t.close()


_WANT = {}


def expected(oracle, which):
    """(arrays, names, families, the oracle's records per family and batch) of a palette: computed once, shared, not changed."""
    if which not in _WANT:
        arrays, names = SC.palette(which)
        fams = SC.families(which)
        want = {f: [oracle.shade(arrays, b["cases"], b["nb"], b["rpp"], b["skybox"]) for b in bs] for f, bs in fams.items()}
        for v in want.values():
            for r in v:
                r.setflags(write=False)
        _WANT[which] = (arrays, names, fams, want)
    return _WANT[which]


def _set(t, opts):
    for k, v in {**DEFAULTS, **opts}.items():
        t.set_option(k, v)


def _launch_kind(rt, t):
    """What a render of the loaded scene under the current options launches (rt_last_launch)."""
    t.render(rt.make_params(16, 16, 1, 1, skybox=1, frames=0))
    t.synchronize()
    return t.last_launch()


@pytest.mark.parametrize("which", ["plain", "general"])
def test_probe_equals_the_oracle_bit_for_bit_in_every_instantiation(rt, oracle, probe, which):
    arrays, names, fams, want = expected(oracle, which)
    configs = [{}, {"lds_scene": 0}] + ([{"tlas": 0}] if which == "general" else [])
    variants = [dict(), dict(general=True), dict(fast_miss=False), dict(total_regs=True), dict(general=True, fast_miss=False, total_regs=True)]
    if which == "plain":
        variants += [dict(simple=True), dict(simple=True, fast_miss=False), dict(simple=True, total_regs=True)]
    seen = set()
    t0 = time.perf_counter()
    try:
        for cfg in configs:
            _set(probe, cfg)
            probe.load_scene(arrays)
            kind = _launch_kind(rt, probe)
            for var in variants:
                for fam, batches in fams.items():
                    for b, w in zip(batches, want[fam]):
                        got = probe.shade(b["cases"], b["nb"], b["rpp"], b["skybox"], **var)
                        what = f"{which} {fam} {cfg} {var} nb {b['nb']} rpp {b['rpp']} skybox {b['skybox']}"
                        same_bits(got, w, what)
                        assert not got[:, 26:].any(), what
                        i = int(got[0, SC.R_INST])
                        assert np.all(got[:, SC.R_INST] == i), what
                        assert bool(i & SC.INST_TLAS) == kind["many_mesh"], (what, i, kind)
                        assert bool(i & SC.INST_LDS) == kind["scene_in_lds"], (what, i, kind)
                        assert bool(i & SC.INST_NO_FAST_MISS) == (var.get("fast_miss") is False), (what, i)
                        assert bool(i & SC.INST_TOTAL_LDS) == (not var.get("total_regs")), (what, i)
                        if var.get("simple"):
                            assert i & SC.INST_SIMPLE, (what, i)
                        elif var.get("general"):
                            assert not i & SC.INST_SIMPLE, (what, i)
                        else:   # the instantiation the render took
                            assert bool(i & SC.INST_SIMPLE) == kind["specialised"], (what, i, kind)
                        seen.add(i)
    finally:
        _set(probe, {})
    print(f"\n{which}: " + ", ".join(f"{f} {sum(len(b['cases']) for b in bs)}" for f, bs in fams.items()) +
          f"; instantiations run: {sorted(seen)}; {time.perf_counter() - t0:.2f} s")
    for bit in (SC.INST_LDS, SC.INST_TOTAL_LDS) + ((SC.INST_SIMPLE,) if which == "plain" else ()):
        assert {bool(i & bit) for i in seen} == {False, True}, (bit, sorted(seen))
    if which == "general":   # (the top-level tree's kernels, and the few-mesh ones with option tlas = 0)
        assert {bool(i & SC.INST_TLAS) for i in seen} == {False, True}, sorted(seen)


@pytest.mark.parametrize("cfg", [{}, {"lds_scene": 0}], ids=["default", "global"])
@pytest.mark.parametrize("which", ["plain", "general"])
def test_records_do_not_depend_on_the_lane_layout(oracle, probe, which, cfg):
    """The same cases in a random order, with every lane active, a random half, or one lane per wave: every active case's
    record is the one it gets in order with all lanes active; an inactive lane writes nothing."""
    arrays, names, fams, want = expected(oracle, which)
    cases = np.concatenate([b["cases"] for bs in fams.values() for b in bs if (b["nb"], b["rpp"], b["skybox"]) == (SC.NB, SC.RPP, 1)])
    rng = np.random.default_rng(len(cases))
    try:
        _set(probe, cfg)
        probe.load_scene(arrays)
        for var in (dict(), dict(fast_miss=False, total_regs=True)):
            base = probe.shade(cases, SC.NB, SC.RPP, 1, **var)
            perm = rng.permutation(len(cases))
            for layout in ("all", "half", "one_per_wave"):
                if layout == "all":
                    a = np.ones(len(cases), np.uint8)
                elif layout == "half":
                    a = (rng.uniform(size=len(cases)) < 0.5).astype(np.uint8)
                else:
                    a = np.zeros(len(cases), np.uint8)
                    a[int(rng.integers(0, 64))::64] = 1
                got = probe.shade(cases[perm], SC.NB, SC.RPP, 1, active=a, **var)
                on = a == 1
                same_bits(got[on], base[perm][on], f"{which} {cfg} {var} {layout}", words=slice(0, 32))
                assert not got[~on].any(), "an inactive lane wrote its record"
    finally:
        _set(probe, {})


@pytest.mark.parametrize("which", ["plain", "general"])
def test_kernel_agrees_with_the_f64_scatter_off_the_ambiguous_cases(oracle, probe, which):
    """A sample of every family straight from the kernel against the float64 restatement -- the comparison of
    tests/test_shade_oracle_f64.py without the oracle in between."""
    arrays, names, fams, _want = expected(oracle, which)
    fscene = F.Scene(arrays)
    out = []
    try:
        _set(probe, {})
        probe.load_scene(arrays)
        for fam, batches in fams.items():
            n = n_amb = 0
            for b in batches:
                c = b["cases"][::max(1, len(b["cases"]) // 4000)]
                got = probe.shade(c, b["nb"], b["rpp"], b["skybox"])
                bad, amb = SC.compare(fscene, got, c, b["nb"], b["rpp"], b["skybox"])
                assert not bad, (which, fam, {k: (v.size, v[:3].tolist()) for k, v in bad.items()})
                n += len(c)
                n_amb += int(amb.sum())
            out.append(f"{fam} {n} ({n_amb} ambiguous)")
    finally:
        _set(probe, {})
    print(f"\n{which}: " + ", ".join(out))


@pytest.mark.parametrize("which", ["plain", "general"])
def test_roulette_skip_equals_the_oracle_stepped_sample_by_sample(oracle, probe, which):
    """roulette_skip from a given state against oracle.shade stepped until the first survivor: dead count, RNG state, total,
    j, the counters and the return value, bit for bit; glass and textured materials are refused (nothing moves)."""
    arrays, names = SC.palette(which)
    mats = SC.materials_of(arrays)
    refused = np.array([int(m["flag"]) == 1 or (int(m["flag"]) == 2 and int(m["diffuse_index"]) != -1) for m in mats])
    n_dead = 0
    try:
        for cfg in ({}, {"lds_scene": 0}):
            _set(probe, cfg)
            probe.load_scene(arrays)
            for rpp in (1, 2, 8):
                cases = SC.roulette_cases(arrays, names, rpp)
                want = SC.roulette_expected(oracle, arrays, cases, rpp)
                variants = [dict(), dict(general=True, total_regs=True)] + ([dict(simple=True)] if which == "plain" else [])
                for var in variants:
                    got = probe.shade(cases, 4, rpp, 1, roulette_skip=True, **var)
                    g = got[:, SC.ROULETTE_WORDS]
                    nan = ((g & 0x7fffffff) > 0x7f800000) & ((want & 0x7fffffff) > 0x7f800000)
                    nan[:, 4:] = False
                    bad = np.flatnonzero(((g != want) & ~nan).any(1))
                    assert bad.size == 0, (which, cfg, rpp, var, bad.size, int(bad[0]), names[int(cases[bad[0], SC.C_OBJ])],
                                           g[bad[0]].tolist(), want[bad[0]].tolist())
                    # what the skip does not own stays: the ray, the throughput, the light, seg
                    assert np.array_equal(got[:, SC.R_RD:SC.R_LIGHT + 4], cases[:, SC.C_RD:SC.C_LIGHT + 4]) and np.array_equal(got[:, SC.R_SEG], cases[:, SC.C_SEG])
                    assert not got[refused[cases[:, SC.C_OBJ]]][:, SC.R_DEAD].any(), "a glass or textured material was skipped"
                n_dead += int(want[:, 9].sum())
                assert want[:, 9].max() == rpp and (want[:, 9] == 0).any()   # (both ends of the dead count occur)
    finally:
        _set(probe, {})
    print(f"\n{which}: {n_dead} samples skipped in the expected results")


def test_the_probe_refuses_what_it_cannot_run(rt, probe):
    arrays, names = SC.palette("plain")
    _set(probe, {})
    probe.load_scene(arrays)
    L, h = probe._L, probe._h
    good = SC.make(1)
    out = np.zeros((1, 32), np.uint32)

    def call(c, which=0, flags=0, n=1):
        c = np.ascontiguousarray(c, np.uint32)
        return L.rt_test_shade(h, which, c.ctypes.data, None, n, 4, 4, 1, flags, out.ctypes.data)
    assert call(SC.make(1, obj=len(names))) == -1                     # object index outside the scene
    assert call(SC.make(1, obj=0xffffffff)) == -1
    for mode in (1, 2, 4, 0x80000003):                                # STEP_WAIT, STEP_REUSE, STEP_RESUME, garbage
        assert call(SC.make(1, mode=mode)) == -1
    assert call(good, which=2) == -1 and call(good, which=-1) == -1   # unknown function
    assert call(good, flags=16) == -1                                 # unknown flag
    assert call(good, flags=5) == -1                                  # general + SIMPLE
    assert call(good, n=(1 << 20) + 1) == -1                          # too many
    assert not out.any()
    assert call(good) == 0 and out.any()
    g_arrays, _ = SC.palette("general")
    probe.load_scene(g_arrays)
    out[:] = 0
    assert call(good, flags=4) == -1                                  # spheres, glass, textures: no SIMPLE instantiation
    assert not out.any()
    with pytest.raises(rt.RtError):
        probe.shade(good, 4, 4, simple=True)
