"""The rule that gives a batch its frame groups (csrc/host/launch_options.h: frame_group_for), on the CPU.

The rule as the header states it: G frames of a pixel are rendered back to back by the lane that took the pixel, and the
work items of the launch are tiles x ceil(n / G) (tile, group) pairs.  G = 1 for a batch of fewer than two frames, for
the frame-major order, for a launch with deferred-walk rounds planned and for a scene read from global memory or walked
by the many-mesh kernels.  Else take the LARGEST g that is at most the compile-time cap (RT_FRAME_GROUP, 8), at most n, and leaves tiles x ceil(n / g) >= 24 x resident waves (g = 1 if no
g >= 2 does); G is the smallest group size that needs no more groups than g: ceil(n / ceil(n / g)).  Every expected
value below was worked out by hand from that sentence; nothing here is computed with the code under test."""
import ctypes as C

import pytest

FRAME_GROUP = 6              # RT_TEST_RULE_FRAME_GROUP
CAP, FLOOR = 8, 24           # the default RT_FRAME_GROUP; items per resident wave
WAVES = 256 * 5 * 4          # an MI355X: 1280 workgroups of four waves = 5120 resident waves
TILES_1080P = 240 * 135      # 32400: 6.3 per resident wave
TILES_SHARE8 = 240 * 17      # 4080: the strip share of rank 0 of eight, 0.8 per resident wave


def group(rt, n, tiles, waves, tile_major=1, rounds=0, costly=0):
    L, inp, out = rt.load_test(), (C.c_int64 * 8)(n, tiles, waves, tile_major, rounds, costly), (C.c_int64 * 2)()
    rc = L.rt_test_launch_rule(FRAME_GROUP, C.byref(inp), C.byref(out))
    assert rc == 0, (rc, L.rt_last_error(None))
    assert out[1] == CAP, "these expectations are written for the default cap"
    return out[0]


def test_the_headline_shapes(rt):
    # the whole 1920 x 1080 frame: 122880 items wanted, 32400 tiles -> at least 4 groups
    assert group(rt, 64, TILES_1080P, WAVES) == 8     # 8 groups of 8
    assert group(rt, 32, TILES_1080P, WAVES) == 8     # 4 groups of 8
    assert group(rt, 33, TILES_1080P, WAVES) == 7     # g = 8 -> 5 groups, which 7 frames each cover (7 7 7 7 5)
    assert group(rt, 31, TILES_1080P, WAVES) == 8     # 4 groups: ceil(31 / 4)
    assert group(rt, 28, TILES_1080P, WAVES) == 7     # g = 8 -> 4 groups of 7
    assert group(rt, 24, TILES_1080P, WAVES) == 6     # g = 8 -> 3 groups: too few; g = 7 -> 4 groups of 6
    assert group(rt, 20, TILES_1080P, WAVES) == 5     # g = 8, 7 -> 3 groups; g = 6 -> 4 groups of 5
    assert group(rt, 10, TILES_1080P, WAVES) == 3     # g = 3 -> 4 groups (3 3 3 1)
    assert group(rt, 9, TILES_1080P, WAVES) == 2      # g = 3 -> 3 groups; g = 2 -> 5 groups
    assert group(rt, 8, TILES_1080P, WAVES) == 2 and group(rt, 7, TILES_1080P, WAVES) == 2


def test_one_for_what_takes_no_groups(rt):
    assert group(rt, 1, TILES_1080P, WAVES) == 1 and group(rt, 0, TILES_1080P, WAVES) == 1      # a batch of one, a single frame
    assert group(rt, 64, TILES_1080P, WAVES, tile_major=0) == 1                                 # frame-major order
    assert group(rt, 64, TILES_1080P, WAVES, rounds=1) == 1                                     # deferred-walk rounds planned
    assert group(rt, 64, TILES_1080P, WAVES, tile_major=0, rounds=1) == 1
    assert group(rt, 64, TILES_1080P, WAVES, costly=1) == 1       # a scene in global memory, the many-mesh kernels
    # the item floor: batches too small for four groups of two
    for n in (2, 3, 4, 5, 6):
        assert group(rt, n, TILES_1080P, WAVES) == 1, n
    assert group(rt, 64, 1, WAVES) == 1 and group(rt, 64, 0, WAVES) == 1


def test_the_strip_share_of_eight_ranks(rt):
    # 4080 tiles want 31 groups for 122880 items (30 x 4080 = 122400 falls short)
    assert group(rt, 28, TILES_SHARE8, WAVES) == 1    # (its frames rendered ahead: no groups)
    assert group(rt, 60, TILES_SHARE8, WAVES) == 1    # g = 2 -> 30 groups
    assert group(rt, 61, TILES_SHARE8, WAVES) == 2    # 31 groups
    assert group(rt, 62, TILES_SHARE8, WAVES) == 2 and group(rt, 64, TILES_SHARE8, WAVES) == 2


def test_both_sides_of_the_item_floor(rt):
    # 100 resident waves want 2400 items; 16 frames: g = 8 -> 2 groups (of 8), 7 and 6 -> 3 (of 6), 5 and 4 -> 4 (of 4),
    # 3 -> 6 (of 3), 2 -> 8 (of 2)
    for tiles, g in ((1200, 8), (1199, 6), (800, 6), (799, 4), (600, 4), (599, 3), (400, 3), (399, 2), (300, 2), (299, 1), (150, 1), (149, 1)):
        assert group(rt, 16, tiles, 100) == g, tiles
    # ... and in the waves: 1000 tiles, 16 frames (2000 / 24 = 83.3, 3000 / 24 = 125, 4000 / 24 = 166.7, 6000 / 24 = 250, 8000 / 24 = 333.3)
    for waves, g in ((83, 8), (84, 6), (125, 6), (126, 4), (166, 4), (167, 3), (250, 3), (251, 2), (333, 2), (334, 1)):
        assert group(rt, 16, 1000, waves) == g, waves
    assert group(rt, 16, 1000, 0) == 8    # (no resident waves known: nothing to starve)


@pytest.mark.parametrize("tiles,waves", [(TILES_1080P, WAVES), (TILES_SHARE8, WAVES), (6, WAVES), (1000, 100), (1, 1)])
def test_never_more_than_the_batch_or_the_cap_and_the_groups_cover_the_batch(rt, tiles, waves):
    for n in range(1, 65):
        g = group(rt, n, tiles, waves)
        assert 1 <= g <= min(n, CAP), (n, g)
        n_groups = -(-n // g)
        assert n_groups * g >= n and (n_groups - 1) * g < n, (n, g)    # the last group is not empty
        assert g == -(-n // n_groups), (n, g)                          # ... and no smaller size covers the batch with as many
        if g > 1:
            assert tiles * n_groups >= FLOOR * waves, (n, g)
