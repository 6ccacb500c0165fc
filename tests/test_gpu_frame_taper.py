"""The taper of a grouped launch (RenderArgs::frame_taper): the tile order is cut into segments and the tiles of a segment
are cut into groups of the segment's own size.  Only the schedule may change: with segment tables forced through the test
library, the image, the segment and reuse counters and the tile costs of the batch's first frame must equal, bit for bit
and count for count, the same frames rendered one rt_render per frame -- at the 20 x 12 frame of
tests/test_gpu_frame_groups.py (3 x 2 tiles).  The last part feeds synthetic tile costs to the kernel that writes the
table on the device and to the host's evaluation of the same rule: the two tables must be equal word for word."""
import ctypes as C

import numpy as np
import pytest

from conftest import bits
from test_gpu_frame_groups import (BOUNCES, H, OPTIONS, SPP, TILES, W, counts, force, last_group, reference, settle, start_image,
                                   tile_costs)

pytestmark = pytest.mark.gpu

BIG = 1 << 30
WORDS, HEAD = 28, 4          # RT_TEST_TAPER_WORDS; {segments, items, frames, G}
FRAME_TAPER = 7              # RT_TEST_RULE_FRAME_TAPER

# name: (first ranks, group sizes, frames of the batch, the forced head group)
TABLES = {
    "one segment": ((0,), (3,), 7, 3),                       # = today's grouped launch: 7 frames as 3 + 3 + 1
    "4 2 1": ((0, 2, 4), (4, 2, 1), 7, 4),                   # ragged groups at every level: 4 + 3, 2 + 2 + 2 + 1, 1 x 7
    "4 1 4": ((0, 2, 4), (4, 1, 4), 7, 4),                   # not monotone
    "a group beyond the batch": ((0, 3), (2, 64), 5, 2),     # g >= n: one group per tile
    "empty segments": ((0, 2, 2, 6), (3, 1, 2, 4), 7, 3),    # ranks 2..1 hold nothing; the last one starts at n_tiles
    "two frames": ((0, 2, 4), (2, 1, 2), 2, 2),
}


@pytest.fixture(scope="module")
def tapered(rt, cornell):
    t = rt.RayTracer(device=0, max_width=64, max_height=64, lib=rt.load_test())
    t.set_option("kernel_variant", 0)
    t.set_option("pipeline", 0)
    t.set_option("frame_ahead", 0)
    t.set_option("batch_frames", 64)
    t.load_scene(cornell)
    yield t
    t.close()


def force_table(t, ranks, sizes):
    n = len(ranks)
    t._check(t._L.rt_test_frame_taper(t._h, n, (C.c_uint32 * max(n, 1))(*ranks), (C.c_uint32 * max(n, 1))(*sizes), None))


def last_table(t):
    out = (C.c_uint32 * WORDS)()
    t._check(t._L.rt_test_frame_taper(t._h, -1, None, None, out))
    return list(out)


def expected_table(ranks, sizes, n, head, n_tiles):
    """The table of forced segments, by hand: a segment's tiles x ceil(n / g) items each, in rank order."""
    table, item = [len(ranks), 0, n, head], 0
    for k, (r, g) in enumerate(zip(ranks, sizes)):
        r, nxt = min(r, n_tiles), min(ranks[k + 1], n_tiles) if k + 1 < len(ranks) else n_tiles
        table += [r, g, item]
        item += (nxt - r) * -(-n // g)
    table[1] = item
    return table + [0] * (WORDS - len(table))


def tapered_batch(rt, t, f0, n, head, ranks, sizes, w=W, h=H, bounces=BOUNCES, spp=SPP, n_tiles=TILES):
    t.set_option("tile_feedback_period", BIG)
    force(t, head)
    force_table(t, ranks, sizes)
    try:
        t.write_image(start_image(f0, w, h))
        t.reset_timing()
        t.render_frames(rt.make_params(w, h, bounces, spp, skybox=1, frames=f0), n)
        return t.read_image(w, h).copy(), counts(t), tile_costs(t, n_tiles), last_group(t), last_table(t)
    finally:
        force(t, 0)
        force_table(t, (), ())


_references = {}


def shared_reference(rt, t, f0):
    """The single-frame launches of the default options, rendered once per first frame for every test that compares with them."""
    if f0 not in _references:
        _references[f0] = reference(rt, t, f0, [2, 5, 7])
    return _references[f0]


@pytest.mark.parametrize("f0", [0, 5])   # the plain store of frame 0, and an accumulation that goes on
@pytest.mark.parametrize("name", list(TABLES))
def test_forced_tables_equal_single_frames(rt, tapered, name, f0):
    ranks, sizes, n, head = TABLES[name]
    want, want_costs = shared_reference(rt, tapered, f0)
    assert sum(want_costs) > 0
    img, cnt, costs, used, table = tapered_batch(rt, tapered, f0, n, head, ranks, sizes)
    assert used == head
    assert table == expected_table(ranks, sizes, n, head, TILES)
    assert np.array_equal(bits(img), bits(want[n][0]))
    assert cnt == want[n][1]
    assert costs == want_costs


def test_one_segment_is_the_grouped_launch(rt, tapered):
    """... and the same batch without a table (no tile order yet: the rule has nothing to cut) gives the same again."""
    ranks, sizes, n, head = TABLES["one segment"]
    with_table = tapered_batch(rt, tapered, 0, n, head, ranks, sizes)
    without = tapered_batch(rt, tapered, 0, n, head, (), ())
    assert without[4] == [0] * WORDS and with_table[4][0] == 1
    assert np.array_equal(bits(with_table[0]), bits(without[0])) and with_table[1:4] == without[1:4]


@pytest.mark.parametrize("option", OPTIONS[1:], ids=lambda o: f"{o[0]}={o[1]}")
def test_every_memo_home_under_a_tapered_batch(rt, tapered, option):
    """Where the memo lives and what it holds (a complete table, no table, a table without hits, the memo in global memory):
    the lane that restarts a pixel for its next frame (memo_next_frame) does so inside items of 4, 2 and 1 frames."""
    t = tapered
    t.set_option(option[0], option[1])
    try:
        want, want_costs = reference(rt, t, 5, [7])
        plain = option[0] in ("batch_tile_major", "lds_scene")   # (launches that take no groups, hence no table)
        for name in ("4 2 1", "4 1 4"):
            ranks, sizes, n, head = TABLES[name]
            img, cnt, costs, used, table = tapered_batch(rt, t, 5, n, head, ranks, sizes)
            assert used == (1 if plain else head), (option, name)
            assert table == ([0] * WORDS if plain else expected_table(ranks, sizes, n, head, TILES)), (option, name)
            assert np.array_equal(bits(img), bits(want[n][0])), (option, name)
            assert cnt == want[n][1] and costs == want_costs, (option, name)
    finally:
        t.set_option(option[0], option[2])


def test_tapered_counter_launch_against_the_oracle(rt, oracle, tapered, cornell):
    ranks, sizes, n, head = TABLES["4 2 1"]
    ref, seg, nt, tt = np.zeros((H, W, 4), np.float32), 0, 0, 0
    for f in range(n):
        ref, st = oracle.render(rt.make_params(W, H, BOUNCES, SPP, skybox=1, frames=f), cornell, image=ref)
        seg, nt, tt = seg + st.segments, nt + st.node_tests, tt + st.triangle_tests
    tapered.set_counters(True)
    try:
        img, cnt, _, used, table = tapered_batch(rt, tapered, 0, n, head, ranks, sizes)
    finally:
        tapered.set_counters(False)
    assert used == head and table[0] == 3
    assert np.array_equal(bits(img), bits(ref)) and cnt == (seg, 0, nt, tt)


def test_tapered_strip_shares_assemble_to_the_full_frames(rt, tapered):
    w, h, world, n = 20, 28, 2, 5   # four strips, the last one ragged: both ranks own two, 6 tiles each
    t = tapered
    want, _ = reference(rt, t, 0, [n], w, h, n_tiles=3 * 4)
    pad = t.strip_texels(w, h, 0, world)
    gathered = np.zeros((world, pad, 4), np.float32)
    force(t, 4)
    force_table(t, (0, 2, 4), (4, 2, 1))
    try:
        for r in range(world):
            t.write_image(np.zeros((h, w, 4), np.float32))
            t.render_strips_frames(rt.make_params(w, h, BOUNCES, SPP, skybox=1, frames=0), n, r, world)
            assert last_group(t) == 4 and last_table(t) == expected_table((0, 2, 4), (4, 2, 1), n, 4, 6)
            cnt = t.strip_texels(w, h, r, world)
            gathered[r, :cnt] = t.read_texels(cnt)
    finally:
        force(t, 0)
        force_table(t, (), ())
    stage = rt.RayTracer(0, world * pad, 1)
    try:
        stage.write_image(gathered.reshape(1, world * pad, 4))
        t.assemble_strips(stage.device_image_ptr, w, h, world)
        assert np.array_equal(bits(t.read_image(w, h)), bits(want[n][0]))
    finally:
        stage.close()


def test_many_mesh_scene_ignores_the_forced_table(rt, tapered, cornell):
    from ray_tracer_2_amd import scenes
    w, h, n, t = 28, 20, 7, tapered
    t.load_scene(rt.SceneArrays.from_scene(scenes.sponza_standin(200)))
    settle(rt, t, w, h)
    try:
        want, want_costs = reference(rt, t, 0, [n], w, h, 3, 2, n_tiles=4 * 3)
        img, cnt, costs, used, table = tapered_batch(rt, t, 0, n, 4, (0, 2, 4), (4, 2, 1), w, h, 3, 2, n_tiles=4 * 3)
        assert used == 1 and table == [0] * WORDS
        assert np.array_equal(bits(img), bits(want[n][0])) and cnt == want[n][1] and costs == want_costs
    finally:
        t.load_scene(cornell)
        settle(rt, t)


def test_deferred_walk_rounds_ignore_the_forced_table(rt, tapered, cornell):
    from test_gpu_scenes import _random_scene
    t, n, w, h = tapered, 5, 28, 20
    try:
        t.set_option("lds_scene", 0)
        t.set_option("defer_min_nodes", 1)
        t.set_option("sort_rounds", 0)
        t.load_scene(_random_scene(rt, 2000))
        settle(rt, t, w, h)
        want, _ = reference(rt, t, 0, [n], w, h, 5, 3, n_tiles=4 * 3)
        t.set_option("sort_rounds", 2)
        img, cnt, _, used, table = tapered_batch(rt, t, 0, n, 4, (0, 2, 4), (4, 2, 1), w, h, 5, 3, n_tiles=4 * 3)
        assert t.last_launch()["deferred_walks"], "the rounds did not run"
        assert used == 1 and table == [0] * WORDS
        assert np.array_equal(bits(img), bits(want[n][0])) and cnt == want[n][1]
    finally:
        t.set_option("sort_rounds", -1)
        t.set_option("defer_min_nodes", 1024)
        t.set_option("lds_scene", 1)
        t.load_scene(cornell)
        settle(rt, t)


def test_the_rule_tapers_a_batch_behind_a_tile_order(rt, tapered):
    """Unforced: the second batch of a sequence has a tile order and, with groups, the rule's own table, written on the
    device -- whatever it holds, the two batches equal fourteen single frames."""
    t, n = tapered, 7
    t.set_option("tile_feedback_period", BIG)
    t.write_image(start_image(0))
    t.reset_timing()
    for k in range(2 * n):
        t.render(rt.make_params(W, H, BOUNCES, SPP, skybox=1, frames=k))
    want, want_counts = t.read_image(W, H).copy(), counts(t)
    t.set_option("tile_feedback_period", 4)   # (resets the history; every batch of 7 refreshes the order)
    force(t, 4)
    try:
        t.write_image(start_image(0))
        t.reset_timing()
        t.render_frames(rt.make_params(W, H, BOUNCES, SPP, skybox=1, frames=0), n)
        first = last_table(t)
        t.render_frames(rt.make_params(W, H, BOUNCES, SPP, skybox=1, frames=n), n)
        table = last_table(t)
        assert first == [0] * WORDS                       # no order yet: untapered
        assert 1 <= table[0] <= 8 and table[2:4] == [n, 4] and table[HEAD:HEAD + 3] == [0, table[HEAD + 1], 0]
        assert np.array_equal(bits(t.read_image(W, H)), bits(want)) and counts(t) == want_counts
    finally:
        force(t, 0)
        t.set_option("tile_feedback_period", 8)


# ---- the rule on the device = the rule on the host --------------------------------------------------------------------

def host_table(rt, costs, n, head, waves, max_cost, floor, alpha):
    L = rt.load_test()
    words = (C.c_uint32 * (len(costs) + WORDS))(*costs)
    inp = (C.c_int64 * 8)(n, head, waves, max_cost, floor, len(costs), C.addressof(words), alpha)
    out = (C.c_int64 * 2)()
    rc = L.rt_test_launch_rule(FRAME_TAPER, C.byref(inp), C.byref(out))
    assert rc == 0, (rc, L.rt_last_error(None))
    return list(words[len(costs):])


def device_table(t, costs, n, head, waves, max_cost, floor, alpha):
    arr = (C.c_uint32 * max(len(costs), 1))(*costs)
    out = (C.c_uint32 * WORDS)()
    t._check(t._L.rt_test_frame_taper_rule(t._h, arr, len(costs), max_cost, floor, n, head, waves, alpha, out))
    return list(out)


def two_level(n_tiles, seed):
    """Cornell's profile at 8 spp and 4 bounces: a share of tiles at the floor (sky served by the table), the rest spread
    between the floor and the most a tile can take."""
    r = np.random.RandomState(seed)
    c = np.where(r.rand(n_tiles) < 0.4, 512, r.randint(513, 2561, n_tiles))
    return [int(x) for x in c]


MAX_COST, FLOOR = 64 * 8 * 5, 64 * 8
COSTS = {
    "no tiles": [],
    "one tile": [1500],
    "all equal": [1500] * 300,
    "all at or below the floor": [512, 100, 0, 512] * 50,
    "one heavy tile among cheap ones": [520] * 99 + [2560],
    "fewer tiles than bins": [2560, 2000, 1500, 1500, 900, 600, 513, 512, 511, 0],
    "4080 tiles": two_level(4080, 1),
    "32400 tiles": two_level(32400, 2),
    "beyond the most a tile can take": [5000, 2561, 2560] * 7,
}


@pytest.mark.parametrize("name", list(COSTS))
def test_the_device_rule_is_the_host_rule(rt, tapered, name):
    costs = COSTS[name]
    seen = set()
    for n, head in ((20, 5), (64, 8), (64, 16), (7, 4), (2, 2), (33, 1)):
        for waves in (5120, 100, 0):
            for alpha in (1, 2, 8):
                for floor in (FLOOR, 0):
                    args = (costs, n, head, waves, MAX_COST, floor, alpha)
                    dev, host = device_table(tapered, *args), host_table(rt, *args)
                    assert dev == host, (name, args[1:])
                    seen.add(tuple(dev[HEAD + 1:HEAD + 3 * dev[0]:3]))
    if name in ("4080 tiles", "32400 tiles", "fewer tiles than bins"):
        assert any(len(s) > 1 for s in seen), "no case of this profile tapered at all"
