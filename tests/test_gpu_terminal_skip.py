"""The terminal skip (RenderArgs::terminal_dark; rt_kernel.hip: intersect_scene's TERM).

A path segment whose path is certain to end at its hit -- the last allowed bounce, or a roulette value no dark material's
throughput can reach -- and whose closest hit so far is a mesh that emits nothing leaves the forest walk out, on scenes
where everything from the forest on emits nothing.  Nothing about the result may change: every image here is equal bit
for bit (alpha included) to the oracle's and to the same frames with the skip switched off through the test library, and
the segment and reuse counters are equal too.  The frames are 44 x 28 (6 x 4 tiles, the right and top ones partly outside),
8 samples per pixel, three frames.  The rule's own cases (which scenes it accepts, its bound) are checked on the CPU in
tests/test_terminal_skip_rule_host.py; here its answer is read back from the launch."""
import ctypes as C

import numpy as np
import pytest

from _terminal_skip_scenes import copy_of, cornell_with_the_light_behind, dark_mask, emissive, items_of
from conftest import bits

pytestmark = pytest.mark.gpu

W, H, SPP, FRAMES = 44, 28, 8, 3


@pytest.fixture(scope="module")
def light_behind(rt):
    return cornell_with_the_light_behind(rt)


@pytest.fixture(scope="module")
def skipper(rt, cornell):
    t = rt.RayTracer(device=0, max_width=64, max_height=64, lib=rt.load_test())
    t.set_option("pipeline", 0)
    t.set_option("frame_ahead", 0)
    t.set_option("batch_frames", 64)
    t.load_scene(cornell)
    yield t
    t.close()


def switch(t, on):
    t._check(t._L.rt_test_terminal_skip(t._h, int(on), None))


def last_mask(t):
    """(dark mask, terminal_c) the handle's last render launch ran with; (0, zeros): it skipped nothing"""
    out = (C.c_uint32 * 4)()
    t._check(t._L.rt_test_terminal_skip(t._h, -1, out))
    return int(out[0]), np.array(list(out)[1:], np.uint32).view(np.float32)


def params(rt, bounces, f, w=W, h=H, spp=SPP):
    return rt.make_params(w, h, bounces, spp, skybox=1, frames=f)


@pytest.fixture(scope="module")
def references(rt, oracle):
    """(name, bounces) -> the oracle's image after each of the frames 0 .. 2, and its segment, node-test and triangle-test
    counts summed over them; computed once per scene, never modified"""
    cache = {}

    def get(name, arrays, bounces):
        if (name, bounces) not in cache:
            img, images, seg, nt, tt = np.zeros((H, W, 4), np.float32), [], 0, 0, 0
            for f in range(FRAMES):
                img, st = oracle.render(params(rt, bounces, f), arrays, image=img)
                images.append(img.copy())
                images[-1].setflags(write=False)
                seg, nt, tt = seg + int(st.segments), nt + int(st.node_tests), tt + int(st.triangle_tests)
            cache[(name, bounces)] = (images, seg, nt, tt)
        return cache[(name, bounces)]
    return get


def render_each(rt, t, bounces):
    """frames 0 .. 2, one launch per frame: the image after every frame, (segments, segments_reused), the masks of the launches"""
    t.write_image(np.zeros((H, W, 4), np.float32))
    t.reset_timing()
    images, masks = [], []
    for f in range(FRAMES):
        t.render(params(rt, bounces, f))
        images.append(t.read_image(W, H).copy())
        masks.append(last_mask(t)[0])
    s = t.stats()
    return images, (int(s.segments), int(s.segments_reused)), masks


def render_batch(rt, t, bounces, group=0):
    t._check(t._L.rt_test_frame_group(t._h, group, None))
    try:
        t.write_image(np.zeros((H, W, 4), np.float32))
        t.reset_timing()
        t.render_frames(params(rt, bounces, 0), FRAMES)
        s = t.stats()
        return t.read_image(W, H).copy(), (int(s.segments), int(s.segments_reused)), last_mask(t)[0]
    finally:
        t._check(t._L.rt_test_frame_group(t._h, 0, None))


def on_and_off_equal_the_oracle(rt, t, ref, bounces, want_mask, where):
    """the three frames launch by launch and as one batch, skip on and off, against `ref` and against each other"""
    images_ref, seg_ref = ref[0], ref[1]
    got = {}
    for on in (1, 0):
        switch(t, on)
        images, counts, masks = render_each(rt, t, bounces)
        for f in range(FRAMES):
            assert np.array_equal(bits(images[f]), bits(images_ref[f])), (where, on, f)
        assert counts[0] == seg_ref, (where, on)
        assert masks == [want_mask if on else 0] * FRAMES, (where, on, masks)
        batch, bcounts, bmask = render_batch(rt, t, bounces)
        assert np.array_equal(bits(batch), bits(images_ref[-1])), (where, on, "batch")
        assert bcounts[0] == seg_ref and bmask == (want_mask if on else 0), (where, on, "batch")
        got[on] = (counts, bcounts)
    switch(t, 1)
    assert got[1] == got[0], where   # segments and segments_reused, launch by launch and batched


def settle(rt, t):
    # (a single frame right behind a new scene renders without the primary table: one frame first, so that what is counted
    # below does not depend on which call came first)
    t.render(params(rt, 1, 0, spp=1))


@pytest.mark.parametrize("variant", [0, 1], ids=["persistent", "wave_per_tile"])
@pytest.mark.parametrize("bounces", [4, 1, 0])
def test_cornell_at_four_one_and_no_bounces(rt, skipper, cornell, references, bounces, variant):
    """4: the bench's paths.  1: every secondary segment is at the last bounce, so every one that holds a wall hit skips.
    0: nothing behind the primary segment is traversed, and a primary segment never skips."""
    t = skipper
    t.load_scene(cornell)
    settle(rt, t)
    t.set_option("kernel_variant", variant)
    try:
        ref = references("cornell", cornell, bounces)
        if bounces == 0:
            assert ref[1] == W * H * SPP * FRAMES
        on_and_off_equal_the_oracle(rt, t, ref, bounces, dark_mask(cornell), (bounces, variant))
    finally:
        t.set_option("kernel_variant", -1)


def test_a_light_behind_the_forest_makes_the_rule_refuse(rt, skipper, cornell, references, light_behind):
    """The light is the item behind the forest, the boxes stand between it and the floor: a lane that left the boxes out
    would light their shadows.  The launch must run with no mask, and the image is the oracle's."""
    t = skipper
    t.load_scene(light_behind)
    settle(rt, t)
    try:
        on_and_off_equal_the_oracle(rt, t, references("light_behind", light_behind, 4), 4, 0, "light behind")
        # ... and the same layout with the light switched off skips (its paths then end in the dark: every mesh is dark)
        dark = copy_of(rt, light_behind)
        dark.meshes["material"]["emission_strength"][emissive(light_behind)[0]] = 0.0
        t.update_instances(dark)
        settle(rt, t)
        on_and_off_equal_the_oracle(rt, t, references("light_behind_off", dark, 4), 4, dark_mask(dark), "light behind, off")
    finally:
        t.load_scene(cornell)


def test_an_emissive_forest_member_at_upload_and_through_an_update(rt, skipper, cornell, references):
    t = skipper
    box = items_of(rt, cornell)[-1][1][0]
    lit = copy_of(rt, cornell)
    lit.meshes["material"]["emission_color"][box] = (0.3, 0.9, 0.4, 1.0)
    lit.meshes["material"]["emission_strength"][box] = 2.0
    try:
        t.load_scene(lit)   # at upload
        settle(rt, t)
        on_and_off_equal_the_oracle(rt, t, references("lit_box", lit, 4), 4, 0, "lit box, uploaded")
        t.load_scene(cornell)   # eligible ...
        settle(rt, t)
        on_and_off_equal_the_oracle(rt, t, references("cornell", cornell, 4), 4, dark_mask(cornell), "before the update")
        t.update_instances(lit)   # ... until the material changes in place: the flag must drop
        settle(rt, t)
        on_and_off_equal_the_oracle(rt, t, references("lit_box", lit, 4), 4, 0, "lit box, updated")
        t.update_instances(cornell)   # ... and come back
        settle(rt, t)
        on_and_off_equal_the_oracle(rt, t, references("cornell", cornell, 4), 4, dark_mask(cornell), "after the update back")
    finally:
        t.load_scene(cornell)


def _albedo_scenes(rt, cornell):
    lit = emissive(cornell)[0]
    dark = [i for i in range(cornell.meshes.shape[0]) if i != lit]
    bright = copy_of(rt, cornell)      # a colour component above 1: the bound exceeds every roulette value, nothing dies for certain
    bright.meshes["material"]["color"][dark, 0] = 1.5
    spec = copy_of(rt, cornell)        # is_spec always, and the specular colour is the brighter one: it sets the bound
    spec.meshes["material"]["specular"][dark] = 1.0
    spec.meshes["material"]["specular_color"][dark] = (0.9, 0.8, 0.85, 1.0)
    spec.meshes["material"]["color"][dark] = (0.2, 0.1, 0.15, 1.0)
    negative = copy_of(rt, cornell)    # a negative component: the throughput turns negative and the T >= 0 guard has to hold
    negative.meshes["material"]["color"][dark, 1] = -0.6
    return {"bright": bright, "specular": spec, "negative": negative}


@pytest.mark.parametrize("name", ["bright", "specular", "negative"])
def test_unusual_albedos(rt, skipper, cornell, references, name):
    t = skipper
    arrays = _albedo_scenes(rt, cornell)[name]
    try:
        t.load_scene(arrays)
        settle(rt, t)
        on_and_off_equal_the_oracle(rt, t, references(name, arrays, 4), 4, dark_mask(arrays), name)
        m = arrays.meshes["material"]
        dark = [i for i in range(arrays.meshes.shape[0]) if i not in emissive(arrays)]
        want_c = np.maximum(m["color"][dark, :3].max(axis=0), m["specular_color"][dark, :3].max(axis=0))
        t.render(params(rt, 4, 0))   # (the switch is on again: the bound this launch ran with)
        assert np.array_equal(last_mask(t)[1], want_c)
    finally:
        t.load_scene(cornell)


@pytest.mark.parametrize("option", [None, ("primary_hits", 0, 1), ("primary_table", 0, 1)], ids=lambda o: "first_frame" if o is None else o[0])
def test_without_a_primary_table_the_memo_still_gets_the_true_hit(rt, skipper, cornell, references, option):
    """Right behind an upload a frame has no primary table, and with primary_hits = 0 never one with hits: the lanes traverse
    their primary segments and memoise what they find.  A primary segment never skips, so every later sample of the pixel
    reuses the true hit: the images are the oracle's and the reuse counters those of the skip switched off."""
    t = skipper
    ref = references("cornell", cornell, 4)
    got = {}
    try:
        if option:
            t.set_option(option[0], option[1])
        for on in (1, 0):
            t.load_scene(cornell)   # (no settling frame: the first launch below is the first frame of the scene)
            switch(t, on)
            images, counts, masks = render_each(rt, t, 4)
            for f in range(FRAMES):
                assert np.array_equal(bits(images[f]), bits(ref[0][f])), (option, on, f)
            assert counts[0] == ref[1] and masks == [dark_mask(cornell) if on else 0] * FRAMES, (option, on)
            got[on] = counts
        assert got[1] == got[0] and got[1][1] > 0, option
    finally:
        switch(t, 1)
        if option:
            t.set_option(option[0], option[2])
        t.load_scene(cornell)


def test_forced_groups_and_strip_shares(rt, skipper, cornell, references):
    t = skipper
    t.load_scene(cornell)
    settle(rt, t)
    ref = references("cornell", cornell, 4)
    t.set_option("kernel_variant", 0)
    try:
        # batches in forced frame groups against one launch per frame
        switch(t, 1)
        _images, each_counts, _masks = render_each(rt, t, 4)
        for g in (2, 3):
            for on in (1, 0):
                switch(t, on)
                img, counts, mask = render_batch(rt, t, 4, group=g)
                assert np.array_equal(bits(img), bits(ref[0][-1])), (g, on)
                assert counts == each_counts and mask == (dark_mask(cornell) if on else 0), (g, on)
        # a strip share: ranks 0 .. 2 of three render their 8-row strips of the three frames, skip on and off
        world = 3
        pad = t.strip_texels(W, H, 0, world)
        gathered = {on: np.zeros((world, pad, 4), np.float32) for on in (1, 0)}
        for on in (1, 0):
            switch(t, on)
            for r in range(world):
                t.write_image(np.zeros((H, W, 4), np.float32))
                t.render_strips_frames(params(rt, 4, 0), FRAMES, r, world)
                assert last_mask(t)[0] == (dark_mask(cornell) if on else 0)
                n = t.strip_texels(W, H, r, world)
                gathered[on][r, :n] = t.read_texels(n)
        assert np.array_equal(bits(gathered[1]), bits(gathered[0]))
        stage = rt.RayTracer(0, world * pad, 1)
        try:
            stage.write_image(gathered[1].reshape(1, world * pad, 4))
            t.assemble_strips(stage.device_image_ptr, W, H, world)
            assert np.array_equal(bits(t.read_image(W, H)), bits(ref[0][-1]))
        finally:
            stage.close()
    finally:
        switch(t, 1)
        t.set_option("kernel_variant", -1)


def test_a_counter_launch_counts_the_shader_s_tests(rt, skipper, cornell, references):
    """count_tests: the counter instantiations walk everything (the rule refuses them), so with the switch on the node and
    triangle test counts are the oracle's."""
    t = skipper
    t.load_scene(cornell)
    settle(rt, t)
    images_ref, seg, nt, tt = references("cornell", cornell, 4)
    switch(t, 1)
    t.set_counters(True)
    try:
        t.write_image(np.zeros((H, W, 4), np.float32))
        t.reset_timing()
        for f in range(FRAMES):
            t.render(params(rt, 4, f))
            assert last_mask(t)[0] == 0
        s = t.stats()
        assert np.array_equal(bits(t.read_image(W, H)), bits(images_ref[-1]))
        assert (int(s.segments), int(s.node_tests), int(s.triangle_tests)) == (seg, nt, tt)
    finally:
        t.set_counters(False)
