"""The roulette skip of path_step's pre-step (option "roulette_skip").

A sample whose memoised primary ray hits a plain material dies or survives its russian roulette as a function of the RNG
state at its start; the samples that die are applied -- light, sample count, RNG, ray counters -- without being shaded.
Nothing about the result may change: every image here is bit-identical to the oracle's (alpha included) and to the same
frames with the option off, and the ray counters are the oracle's.  The scenes put the death rate everywhere between
never and always, make the dead samples carry light, let the is_spec draw choose the threshold, and mix eligible pixels
with sky, glass and textured ones inside one 8 x 8 tile.
"""
import os

import numpy as np
import pytest

from conftest import GOLDEN, bits

pytestmark = pytest.mark.gpu

W = H = 16   # four 8 x 8 tiles
FRAMES = 3
QUAD = [[-1, 0, -1, 0, 1, 0, 0, 0], [1, 0, -1, 0, 1, 0, 1, 0], [1, 0, 1, 0, 1, 0, 1, 1], [-1, 0, 1, 0, 1, 0, 0, 1]]
QUAD_IDX = [2, 1, 0, 3, 2, 0]


def _floor_scene(rt, mat):
    """One quad that fills the view: the camera looks steeply down at a 100 x 100 floor."""
    sc = rt.Scene()
    sc.set_camera((0.3, 2.0, 1.0), (0.2, 0.0, 0.1), fov=40.0)
    sc.add_mesh_from_data(QUAD, QUAD_IDX, xform=rt.transform(scale=(50, 1, 50)), mat=mat)
    sc.build()
    return rt.SceneArrays.from_scene(sc)


def _mixed_scene(rt):
    """Sky above the horizon, a diffuse quad and a textured quad side by side below it, a glass sphere in the middle of
    the view, where the four tiles meet."""
    earth = rt.SceneArrays.load(os.path.join(GOLDEN, "texture_test_scene.npz")).textures[0]   # (earthmap.png, decoded)
    sc = rt.Scene()
    sc.set_camera((0.3, 1.0, 3.0), (0.2, 0.4, 0.1), fov=50.0)
    ti = sc.add_texture_rgba8(earth)
    sc.add_mesh_from_data(QUAD, QUAD_IDX, xform=rt.transform(pos=(-2.4, 0, 0), scale=(3, 1, 4)),
                          mat=rt.material(color=(0.6, 0.5, 0.4, 1), smoothness=0.0))
    sc.add_mesh_from_data(QUAD, QUAD_IDX, xform=rt.transform(pos=(3.6, 0, 0), scale=(3, 1, 4)),
                          mat=rt.material(flag=2, diffuse_index=ti, smoothness=0.0))
    sc.add_sphere((0.2, 0.5, 0.6), 0.5, rt.material(color=(0.9, 0.9, 1, 1), flag=1, ior=1.45, smoothness=0.9, specular=0.8,
                                                     absorption=(0.2, 0.1, 0.05, 0), absorption_strength=1.5))
    sc.build()
    return rt.SceneArrays.from_scene(sc)


def _grey(c):
    return (c, c, c, 1.0)


SCENES = {
    "colour_0.05": lambda rt: _floor_scene(rt, rt.material(color=_grey(0.05), smoothness=0.0)),     # 95 % die: whole pixels
    "colour_0.0": lambda rt: _floor_scene(rt, rt.material(color=_grey(0.0), smoothness=0.0)),       # every sample dies
    "colour_1.0": lambda rt: _floor_scene(rt, rt.material(color=_grey(1.0), smoothness=0.0)),       # only a draw of 1.0 kills
    "colour_1.5": lambda rt: _floor_scene(rt, rt.material(color=_grey(1.5), smoothness=0.0)),       # nothing dies
    "emissive": lambda rt: _floor_scene(rt, rt.material(color=_grey(0.5), emission_color=(1, 0.9, 0.8, 1),
                                                        emission_strength=2.0, smoothness=0.0)),   # the dead add light
    "specular": lambda rt: _floor_scene(rt, rt.material(color=(0.2, 0.1, 0.05, 1), specular=0.5,
                                                        specular_color=(0.9, 0.6, 0.3, 1), smoothness=0.7)),   # is_spec picks the threshold
    "mixed_tile": _mixed_scene,
}


@pytest.fixture(scope="module")
def small(rt):
    t = rt.RayTracer(device=0, max_width=W, max_height=H)
    yield t
    t.close()


@pytest.fixture(scope="module")
def references(rt, oracle):
    """(scene, spp, bounces) -> the oracle's image after each of the frames 0 .. 2 and its segment count per frame;
    computed once, never modified."""
    cache = {}

    def get(name, arrays, spp, bounces):
        key = (name, spp, bounces)
        if key not in cache:
            img, images, segs = np.zeros((H, W, 4), np.float32), [], []
            for f in range(FRAMES):
                img, st = oracle.render(rt.make_params(W, H, bounces, spp, skybox=1, frames=f), arrays, image=img)
                images.append(img.copy())
                segs.append(int(st.segments))
            for im in images:
                im.setflags(write=False)
            cache[key] = (images, segs)
        return cache[key]
    return get


def _render_each(rt, t, spp, bounces):
    """frames 0 .. 2, one render per frame, each frame read: the image after every frame, the counters of the three"""
    t.write_image(np.zeros((H, W, 4), np.float32))
    t.reset_timing()
    images = []
    for f in range(FRAMES):
        t.render(rt.make_params(W, H, bounces, spp, skybox=1, frames=f))
        images.append(t.read_image(W, H))
    s = t.stats()
    return images, int(s.segments), int(s.segments_reused)


def _render_batch(rt, t, spp, bounces):
    t.write_image(np.zeros((H, W, 4), np.float32))
    t.reset_timing()
    t.render_frames(rt.make_params(W, H, bounces, spp, skybox=1, frames=0), FRAMES)
    img = t.read_image(W, H)
    s = t.stats()
    return img, int(s.segments), int(s.segments_reused)


@pytest.mark.parametrize("name", list(SCENES))
def test_skipped_samples_leave_every_bit_and_counter_as_the_oracle_has_them(rt, oracle, small, references, name):
    arrays = SCENES[name](rt)
    small.load_scene(arrays)
    # (the first single frame after a camera change is rendered without the primary table -- the camera may be moving -- and
    # so serves its first samples by traversal; one frame settles the new scene's camera before anything is counted)
    small.render(rt.make_params(W, H, 0, 1, skybox=1, frames=0))
    try:
        for lds in (1, 0):
            for variant in (0, 1):
                small.set_option("lds_scene", lds)
                small.set_option("kernel_variant", variant)
                for spp in (1, 8, 17):
                    for bounces in (0, 4):
                        ref_images, ref_segs = references(name, arrays, spp, bounces)
                        if name == "colour_0.0":
                            # the input provably takes the all-dead path: every sample is its primary segment and nothing else
                            assert ref_segs == [W * H * spp] * FRAMES
                        got = {}
                        for skip in (1, 0):
                            small.set_option("roulette_skip", skip)
                            where = (name, lds, variant, spp, bounces, skip)
                            images, segments, reused = _render_each(rt, small, spp, bounces)
                            for f in range(FRAMES):
                                assert np.array_equal(bits(images[f]), bits(ref_images[f])), (where, f)
                            assert segments == sum(ref_segs), where
                            assert reused == W * H * spp * FRAMES, where
                            batch, segments, reused = _render_batch(rt, small, spp, bounces)
                            assert np.array_equal(bits(batch), bits(ref_images[-1])), (where, "batch")
                            assert segments == sum(ref_segs), (where, "batch")
                            assert reused == W * H * spp * FRAMES, (where, "batch")
                            got[skip] = images + [batch]
                        for on, off in zip(got[1], got[0]):
                            assert np.array_equal(bits(on), bits(off)), (name, lds, variant, spp, bounces)
    finally:
        small.set_option("roulette_skip", 1)
        small.set_option("kernel_variant", -1)
        small.set_option("lds_scene", 1)


def test_the_scenes_reach_both_sides_of_the_roulette(rt, oracle, references):
    """What the scenes are for, read off the oracle's segment counts at 4 bounces: colour 0.05 kills nearly every sample at
    its primary hit (so whole pixels end inside the skip), colour 1.5 kills none (every sample goes on to a second
    segment), the mixed view has both."""
    n = W * H * 8
    segs = {name: references(name, SCENES[name](rt), 8, 4)[1][0] for name in ("colour_0.05", "colour_1.5", "mixed_tile")}
    assert n <= segs["colour_0.05"] < 1.15 * n
    assert segs["colour_1.5"] >= 2 * n
    assert n < segs["mixed_tile"]
