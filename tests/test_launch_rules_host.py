"""The rules that turn options into a launch (csrc/host/launch_options.h), on the CPU, at the figures include/rt_abi.h
quotes and at both sides of every threshold.  The thresholds below were read off the source of commit d11ad3b
(csrc/rt_api.hip: automatic_pipeline_depth, plan_rounds, vote_thresholds, choose_kernel_shape, render_frames_impl,
blocks_per_cu_for / persistent_blocks_for), where these rules lived among the HIP calls; nothing here is computed with
the code under test."""
import ctypes as C

import pytest

VOTES, ROUNDS, VARIANT, DEPTH, BATCH, GRID = range(6)
FRAME = 1920 * 1080          # the rounds' unit of work: one such frame at 16 samples per pixel
CUS = 256                    # an MI355X: persistent_blocks = CUs x 5 = 1280 workgroups of four waves


# which of a rule's inputs are option values: they go through the setter first, as in a handle
OPTIONS = {VOTES: ("vote_eighths", "vote_patience"), VARIANT: ("kernel_variant", "persistent_blocks"), DEPTH: ("pipeline",),
           GRID: (None, "persistent_blocks")}


def stored(rt, name, value):
    L, out = rt.load_test(), (C.c_int32 * 2)()
    rc = L.rt_test_set_option(name.encode(), value, C.byref(out))
    assert rc == 0, (name, value, L.rt_last_error(None))
    return out[0]


def rule(rt, which, *values):
    values = [stored(rt, name, v) if name else v for name, v in zip(OPTIONS.get(which, ()), values)] + list(values[len(OPTIONS.get(which, ())):])
    L, inp, out = rt.load_test(), (C.c_int64 * 8)(*values), (C.c_int64 * 2)()
    rc = L.rt_test_launch_rule(which, C.byref(inp), C.byref(out))
    assert rc == 0, (rc, L.rt_last_error(None))
    return out[0], out[1]


def test_vote_thresholds(rt):
    # -1 / -1: 6 and 3 for a scene in LDS on the few-mesh kernels, 7 and 16 for the others, 8 and 16 inside a deferred-walk sequence
    assert rule(rt, VOTES, -1, -1, 0, 0) == (6, 3)
    assert rule(rt, VOTES, -1, -1, 0, 1) == (7, 16)
    assert rule(rt, VOTES, -1, -1, 1, 0) == (8, 16) and rule(rt, VOTES, -1, -1, 1, 1) == (8, 16)
    # explicit values pass through, each on its own
    for rounds, costly in ((0, 0), (0, 1), (1, 0), (1, 1)):
        assert rule(rt, VOTES, 0, 0, rounds, costly) == (0, 0)
        assert rule(rt, VOTES, 8, 1000, rounds, costly) == (8, 1000)
    assert rule(rt, VOTES, 5, -1, 0, 0) == (5, 3) and rule(rt, VOTES, -1, 7, 0, 1) == (7, 7)


# (units of work from which on, rounds): a deferred mesh of >= 400 000 internal nodes / a smaller one
BIG_LADDER = [(2, 2), (4, 3), (12, 4), (24, 8), (48, 12), (96, 16), (384, 24)]
SMALL_LADDER = [(8, 3), (12, 4), (24, 6)]


@pytest.mark.parametrize("internal,ladder", [(400000, BIG_LADDER), (399999, SMALL_LADDER), (1 << 21, BIG_LADDER), (1, SMALL_LADDER)])
def test_automatic_rounds_at_both_sides_of_every_step(rt, internal, ladder):
    below = 0
    for units, rounds in ladder:
        # `units` frames' worth of pixels at 16 spp, and one pixel less; the same work as one frame at 16 x units spp
        assert rule(rt, ROUNDS, FRAME * units, 16, internal)[0] == rounds
        assert rule(rt, ROUNDS, FRAME * units - 1, 16, internal)[0] == below
        assert rule(rt, ROUNDS, FRAME, 16 * units, internal)[0] == rounds
        assert rule(rt, ROUNDS, FRAME, 16 * units - 1, internal)[0] == below
        below = rounds
    assert rule(rt, ROUNDS, FRAME * 100000, 16, internal)[0] == ladder[-1][1]
    assert rule(rt, ROUNDS, 0, 16, internal)[0] == 0 and rule(rt, ROUNDS, FRAME * 1000, 0, internal)[0] == 0
    assert rule(rt, ROUNDS, FRAME * 1000, -3, internal)[0] == 0   # (no samples: no work)


def test_kernel_variant(rt):
    # automatic: one wave per tile at <= 1.25 tiles per resident wave (tiles * 4 <= waves * 5)
    waves = CUS * 5 * 4
    assert waves * 5 % 4 == 0
    assert rule(rt, VARIANT, -1, CUS * 5, waves * 5 // 4, 0, 0)[0] == 1
    assert rule(rt, VARIANT, -1, CUS * 5, waves * 5 // 4 + 1, 0, 0)[0] == 0
    assert rule(rt, VARIANT, -1, 1, 5, 0, 0)[0] == 1 and rule(rt, VARIANT, -1, 1, 6, 0, 0)[0] == 0
    assert rule(rt, VARIANT, -1, CUS * 5, 240 * 135, 0, 0)[0] == 0   # a 1920 x 1080 frame
    # explicit values pass through
    assert rule(rt, VARIANT, 0, CUS * 5, 1, 0, 0)[0] == 0 and rule(rt, VARIANT, 1, CUS * 5, 1 << 20, 0, 0)[0] == 1
    # a batch's (frame, tile) work items and the counters are the persistent kernel's, whatever the option says
    for option in (-1, 1):
        assert rule(rt, VARIANT, option, CUS * 5, 1, 2, 0)[0] == 0
        assert rule(rt, VARIANT, option, CUS * 5, 1, 0, 1)[0] == 0


def test_pipeline_depth(rt):
    for world in (1, 2, 4, 8):
        assert rule(rt, DEPTH, -1, 4, world)[0] == 3    # four queues (the runtime's default): three frames in flight
    assert rule(rt, DEPTH, -1, 5, 1)[0] == 4            # five and more: four
    assert rule(rt, DEPTH, -1, 12, 4)[0] == 7           # twelve, and a strip share of four ranks and more: seven
    assert rule(rt, DEPTH, -1, 12, 8)[0] == 7
    assert rule(rt, DEPTH, -1, 12, 2)[0] == 4 and rule(rt, DEPTH, -1, 12, 3)[0] == 4
    assert rule(rt, DEPTH, -1, 11, 4)[0] == 4 and rule(rt, DEPTH, -1, 1, 4)[0] == 3
    for explicit in (0, 2, 3, 4, 8):                    # an explicit option passes through, whatever the queues
        assert rule(rt, DEPTH, explicit, 4, 1)[0] == explicit and rule(rt, DEPTH, explicit, 12, 4)[0] == explicit
    assert rule(rt, DEPTH, 1, 4, 1)[0] == 3 and rule(rt, DEPTH, 1, 5, 1)[0] == 4 and rule(rt, DEPTH, 1, 12, 4)[0] == 7   # 1 = automatic


def test_equal_batches(rt):
    assert rule(rt, BATCH, 20, 16)[0] == 10             # 10 + 10, not 16 + 4
    assert rule(rt, BATCH, 16, 16)[0] == 16 and rule(rt, BATCH, 17, 16)[0] == 9 and rule(rt, BATCH, 33, 16)[0] == 11
    assert rule(rt, BATCH, 5, 16)[0] == 5 and rule(rt, BATCH, 2, 64)[0] == 2   # a cap above n: one batch of n
    assert rule(rt, BATCH, 7, 1)[0] == 1
    assert rule(rt, BATCH, 0, 16)[0] == 0


def test_persistent_grid(rt):
    KIB = 1024
    # (LDS bytes per workgroup, workgroups per CU): 160 KiB of LDS per CU, at most the five of the register budget, at least one
    for lds, per_cu in ((0, 5), (29888, 5), (32 * KIB, 5), (32 * KIB + 1, 4), (40 * KIB, 4), (40 * KIB + 1, 3), (73728, 2),
                        (80 * KIB, 2), (80 * KIB + 1, 1), (160 * KIB, 1), (160 * KIB + 1, 1), (1 << 20, 1)):
        assert rule(rt, GRID, lds, CUS * 5) == (per_cu, CUS * per_cu), lds
    # an explicit grid smaller than a CU's worth is kept; a larger one is scaled by the occupancy
    assert rule(rt, GRID, 73728, 4) == (2, 4) and rule(rt, GRID, 73728, 5) == (2, 2) and rule(rt, GRID, 73728, 12) == (2, 4)
    assert rule(rt, GRID, 0, 12) == (5, 10)   # (whole CUs' worth: 12 / 5 x 5)
