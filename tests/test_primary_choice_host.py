"""The primary table of a launch (csrc/host/launch_state.h: choose_primary) on the CPU: none, the shared one or the
pipeline slot's own; rebuilt or not; and what a rebuild owes first.  The full truth table over its inputs is checked against
a restatement of the condition as it stood in commit e4b795b (csrc/rt_api.hip: bind_primary_table), written out below;
nothing here is computed with the code under test."""
import ctypes as C
import itertools

import numpy as np

FACTS = ("primary_table", "primary_hits", "primary_per_slot", "camera_moved", "n_batch", "pipelined", "pixel_cache", "debug_flag",
         "rays_per_pixel", "count_tests", "shared_serves", "shared_large", "shared_may_grow", "own_serves", "own_large", "own_may_grow")
NONE, SHARED, OWN = 0, 1, 2
NO_SYNC, SLOT_STREAM, DRAIN_STREAMS = 0, 1, 2
# a launch that takes the shared table as it stands: every option at its default, a single frame, nothing pipelined
DEFAULT = dict(primary_table=1, primary_hits=1, primary_per_slot=1, camera_moved=0, n_batch=0, pipelined=0, pixel_cache=1, debug_flag=0,
               rays_per_pixel=8, count_tests=0, shared_serves=1, shared_large=1, shared_may_grow=1, own_serves=0, own_large=0, own_may_grow=1)


def choose(rt, rows):
    rows = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1, len(FACTS))
    out = np.zeros((len(rows), 5), dtype=np.uint32)
    assert rt.load_test().rt_test_primary_choice(rows.ctypes.data_as(C.c_void_p), len(rows), out.ctypes.data_as(C.c_void_p)) == 0
    return out


def one(rt, **facts):
    table, want_hits, rebuild, sync, barrier = (int(v) for v in choose(rt, [[{**DEFAULT, **facts}[k] for k in FACTS]])[0])
    return dict(table=table, want_hits=want_hits, rebuild=rebuild, sync=sync, barrier=barrier)


def test_full_truth_table(rt):
    values = {"n_batch": (0, 2), "rays_per_pixel": (0, 8)}  # (every other input: 0 and 1)
    rows = np.array(list(itertools.product(*[values.get(k, (0, 1)) for k in FACTS])), dtype=np.int32)
    assert len(rows) == 1 << 16
    f = {k: rows[:, i] for i, k in enumerate(FACTS)}
    true = {k: v != 0 for k, v in f.items()}
    # bind_primary_table as it stood
    usable = (true["primary_table"] & (true["shared_large"] | true["shared_may_grow"]) & true["pixel_cache"] & ~true["debug_flag"] &
              (f["rays_per_pixel"] > 0) & ~(true["camera_moved"] & (f["n_batch"] == 0)))
    want_hits = true["primary_hits"] & ~true["count_tests"]
    use_own = true["pipelined"] & ~true["shared_serves"] & true["primary_per_slot"] & (true["own_large"] | true["own_may_grow"])
    serves = np.where(use_own, true["own_serves"], true["shared_serves"])
    large = np.where(use_own, true["own_large"], true["shared_large"])
    rebuild = usable & ~serves
    expect = np.stack([np.where(usable, np.where(use_own, OWN, SHARED), NONE), usable & want_hits, rebuild,
                       np.where(rebuild & ~large, np.where(use_own, SLOT_STREAM, DRAIN_STREAMS), NO_SYNC), rebuild & ~use_own], axis=1)
    got = choose(rt, rows)
    bad = np.nonzero((got != expect.astype(np.uint32)).any(axis=1))[0]
    assert len(bad) == 0, (dict(zip(FACTS, rows[bad[0]])), got[bad[0]], expect[bad[0]])


def test_a_moved_camera_takes_no_table_on_a_single_frame_but_a_batch_keeps_it(rt):
    assert one(rt)["table"] == SHARED and one(rt, camera_moved=1)["table"] == NONE
    assert one(rt, camera_moved=1, n_batch=2)["table"] == SHARED
    # ... rebuilt for the new camera behind the other streams' frames; nobody waits for a table that is large enough
    assert one(rt, camera_moved=1, n_batch=2, shared_serves=0) == dict(table=SHARED, want_hits=1, rebuild=1, sync=NO_SYNC, barrier=1)


def test_a_pipelined_frame_takes_its_own_table_only_with_primary_per_slot_and_room(rt):
    stale = dict(pipelined=1, shared_serves=0)
    assert one(rt, pipelined=1)["table"] == SHARED  # (the shared table serves: no reason for another)
    assert one(rt, **stale) == dict(table=OWN, want_hits=1, rebuild=1, sync=SLOT_STREAM, barrier=0)
    assert one(rt, **stale, own_large=1) == dict(table=OWN, want_hits=1, rebuild=1, sync=NO_SYNC, barrier=0)
    assert one(rt, **stale, own_large=1, own_serves=1) == dict(table=OWN, want_hits=1, rebuild=0, sync=NO_SYNC, barrier=0)
    for without in (dict(primary_per_slot=0), dict(own_may_grow=0)):
        assert one(rt, **stale, **without) == dict(table=SHARED, want_hits=1, rebuild=1, sync=NO_SYNC, barrier=1), without
    assert one(rt, shared_serves=0)["table"] == SHARED  # (not pipelined: there is no slot)


def test_a_table_that_has_to_grow(rt):
    small = dict(shared_serves=0, shared_large=0)
    assert one(rt, **small) == dict(table=SHARED, want_hits=1, rebuild=1, sync=DRAIN_STREAMS, barrier=1)
    assert one(rt, **small, shared_may_grow=0)["table"] == NONE  # (beyond the cap on device memory: done without)
    assert one(rt, **small, shared_may_grow=0, pipelined=1)["table"] == NONE  # (... a slot table does not stand in for it)


def test_counters_never_want_hits(rt):
    for facts in itertools.product((0, 1), repeat=4):
        facts = dict(zip(("primary_hits", "pipelined", "shared_serves", "n_batch"), facts))
        assert one(rt, count_tests=1, **facts)["want_hits"] == 0, facts
    assert one(rt)["want_hits"] == 1 and one(rt, primary_hits=0)["want_hits"] == 0


def test_launches_without_samples_or_a_memo_take_no_table(rt):
    for facts in (dict(debug_flag=1), dict(rays_per_pixel=0), dict(pixel_cache=0), dict(primary_table=0)):
        assert one(rt, **facts) == dict(table=NONE, want_hits=0, rebuild=0, sync=NO_SYNC, barrier=0), facts
