"""The rule that lets a launch skip forest walks (csrc/host/launch_options.h: terminal_skip_scene, terminal_skip_for), on the
CPU, through the test library: the host packer lays a scene out (rt_test_pack_scene) and the rule reads that head.

The rule as the header states it.  A mesh is DARK when the four products emission_color * emission_strength are +0 bitwise.
The lane-sparse items of the mesh loop are the forest items and the single meshes with an internal root that is not a
two-leaf one.  terminal_skip_ok = 1 iff the scene has such an item, every mesh of the first one and of every item behind it
is dark, every dark material's color and specular_color components are finite -- and the launch takes the SIMPLE few-mesh
kernels on a scene staged in LDS without counters.  terminal_c is the componentwise maximum of color.xyz and
specular_color.xyz over the dark meshes.  Every expectation below follows from those sentences and the scenes' own numbers;
nothing is computed with the code under test."""
import ctypes as C

import numpy as np
import pytest

from _terminal_skip_scenes import ITEM_FOREST, copy_of, cornell_with_the_light_behind, emissive, items_of

TERMINAL_SKIP = 9   # RT_TEST_RULE_TERMINAL_SKIP


def rule(rt, arrays, lds=1, simple=None, counters=0, **pack):
    """(terminal_skip_ok, dark mask, terminal_c as three floats) for `arrays` packed under the options `pack`; simple = None:
    a launch takes SIMPLE when the packer found plain materials only (no sphere, no glass, no texture)"""
    blob, lay, facts = rt.RayTracer.pack_scene(arrays, **pack)
    lay = np.ascontiguousarray(lay, np.uint32)
    if simple is None:
        simple = int(facts[6])   # plain_materials
    c = (C.c_float * 3)(-1.0, -1.0, -1.0)
    inp = (C.c_int64 * 8)(blob.ctypes.data, lay.ctypes.data, int(facts[0]), arrays.meshes.shape[0], lds, simple, counters, C.addressof(c))
    out = (C.c_int64 * 2)()
    L = rt.load_test()
    rc = L.rt_test_launch_rule(TERMINAL_SKIP, C.byref(inp), C.byref(out))
    assert rc == 0, (rc, L.rt_last_error(None))
    return int(out[0]), int(out[1]), np.array(list(c), np.float32)


@pytest.fixture(scope="module")
def light_behind(rt):
    return cornell_with_the_light_behind(rt)


def test_cornell_is_eligible_and_its_bound_is_the_white_walls(rt, cornell):
    lit = emissive(cornell)
    assert len(lit) == 1
    n = cornell.meshes.shape[0]
    items = items_of(rt, cornell)
    # what the issue says of the layout: the forest of the two boxes is the last item, the light a single mesh before it
    assert items[-1][0] & ITEM_FOREST and len(items[-1][1]) == 2 and lit[0] not in items[-1][1]
    ok, dark, c = rule(rt, cornell)
    assert ok == 1
    assert dark == ((1 << n) - 1) & ~(1 << lit[0])
    m = cornell.meshes["material"]
    both = np.concatenate([m["color"][[i for i in range(n) if i != lit[0]], :3], m["specular_color"][[i for i in range(n) if i != lit[0]], :3]])
    assert np.array_equal(c, both.max(axis=0))
    assert np.array_equal(c, np.array([0.725, 0.71, 0.68], np.float32))   # CornellBox-Original.mtl: Kd of the white walls


def test_the_launch_has_to_take_the_simple_lds_kernels_without_counters(rt, cornell):
    assert rule(rt, cornell)[0] == 1
    for kw in (dict(simple=0), dict(lds=0), dict(counters=1)):
        ok, dark, c = rule(rt, cornell, **kw)
        assert ok == 0 and not c.any(), kw
        assert dark == rule(rt, cornell)[1]   # (the mask of the dark meshes is a fact of the scene)


def test_a_scene_with_glass_takes_no_simple_kernels_and_refuses(rt, cornell):
    a = copy_of(rt, cornell)
    a.meshes["material"]["flag"][0] = 1   # RT_MATERIAL_GLASS
    ok, _dark, c = rule(rt, a)
    assert ok == 0 and not c.any()
    assert rule(rt, a, simple=1)[0] == 1   # (the scene's items and emission alone would allow it: the launch decides)


def test_an_emissive_forest_member_refuses(rt, cornell):
    box = items_of(rt, cornell)[-1][1][1]
    for field, value in (("emission_strength", 1.0), ("emission_strength", -0.0)):
        a = copy_of(rt, cornell)
        a.meshes["material"]["emission_color"][box] = (1, 1, 1, 1)
        a.meshes["material"][field][box] = value
        ok, dark, c = rule(rt, a)
        assert ok == 0 and not (dark >> box) & 1 and not c.any(), (field, value)   # (1 * -0 = -0: not +0 bitwise)
    a = copy_of(rt, cornell)
    a.meshes["material"]["emission_color"][box] = (1, 1, 1, 1)   # strength +0: every product is +0, the box stays dark
    assert rule(rt, a)[0] == 1


def test_an_emissive_item_behind_the_forest_refuses(rt, light_behind):
    lit = emissive(light_behind)
    items = items_of(rt, light_behind)
    forest_at = [k for k, (kind, _m) in enumerate(items) if kind & ITEM_FOREST]
    light_at = [k for k, (_kind, m) in enumerate(items) if m == lit]
    assert len(forest_at) == 1 and len(light_at) == 1 and light_at[0] > forest_at[0]
    ok, dark, c = rule(rt, light_behind)
    assert ok == 0 and not c.any() and not (dark >> lit[0]) & 1
    # ... and with the light switched off the same layout is eligible
    a = copy_of(rt, light_behind)
    a.meshes["material"]["emission_strength"][lit[0]] = 0.0
    assert rule(rt, a)[0] == 1


def test_a_single_mesh_with_an_internal_root_is_a_sparse_item(rt, cornell):
    """forest = 0: the two boxes are single items in mesh order; what follows the first of them has to be dark, the light included"""
    items = items_of(rt, cornell, forest=0)
    assert not any(kind & ITEM_FOREST for kind, _m in items)
    lit, boxes = emissive(cornell)[0], items_of(rt, cornell)[-1][1]
    order = [m[0] for _kind, m in items]
    ok, _dark, _c = rule(rt, cornell, forest=0)
    assert ok == (1 if order.index(lit) < min(order.index(b) for b in boxes) else 0)
    a = copy_of(rt, cornell)
    a.meshes["material"]["emission_strength"][lit] = 0.0
    assert rule(rt, a, forest=0)[0] == 1


@pytest.mark.parametrize("value", [np.inf, -np.inf, np.nan])
@pytest.mark.parametrize("field", ["color", "specular_color"])
def test_a_non_finite_colour_of_a_dark_material_refuses(rt, cornell, field, value):
    a = copy_of(rt, cornell)
    dark_mesh = [i for i in range(a.meshes.shape[0]) if i not in emissive(a)][0]
    a.meshes["material"][field][dark_mesh, 1] = value
    ok, _dark, c = rule(rt, a)
    assert ok == 0 and not c.any()
    # ... but the light's own colours are not part of the bound
    b = copy_of(rt, cornell)
    b.meshes["material"][field][emissive(b)[0], 1] = value
    assert rule(rt, b)[0] == 1


def test_the_bound_takes_both_colours_and_keeps_signs(rt, cornell):
    a = copy_of(rt, cornell)
    n, lit = a.meshes.shape[0], emissive(a)[0]
    dark = [i for i in range(n) if i != lit]
    m = a.meshes["material"]
    m["color"][dark] = (-0.5, 0.25, 0.125, 1.0)
    m["specular_color"][dark] = (-0.75, 0.0, 0.0, 0.0)
    m["specular_color"][dark[2]] = (-0.625, 0.0, 1.5, 0.0)
    m["color"][lit] = (9.0, 9.0, 9.0, 1.0)   # (not dark: not counted)
    ok, _dark, c = rule(rt, a)
    assert ok == 1 and np.array_equal(c, np.array([-0.5, 0.25, 1.5], np.float32))
