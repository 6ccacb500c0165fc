"""The sequence of frames rendered ahead (csrc/host/launch_state.h: AheadSequence), whole sequences of calls on the CPU:
which one-frame call starts a batch, which calls are served from it, what drops it, how the automatic depth ramps up, and
the frames asked for / speculative that rt_get_stats reports.  tests/test_frame_ahead_policy.py pins the depth rule; this
pins the sequence that uses it.  The expected values were worked out by hand from the source of commit e4b795b
(csrc/rt_api.hip: render_single, render_impl, account_launch), where the sequence lived among the HIP calls; nothing here
is computed with the code under test."""
import ctypes as C

from ray_tracer_2_amd import _abi as A

u32, i32 = C.c_uint32, C.c_int32
FRAME, BATCHED, BUMP, SET_OPTION = range(4)
W, H = 1920, 1080
SHARE8 = (((H + 7) // 8) // 8 + 1) * 8 * W  # rank 0's share of eight: the rule's depth is 28 (tests/test_frame_ahead_policy.py)


class Call(C.Structure):
    _fields_ = [("kind", u32), ("params", A.Params), ("rank", u32), ("world", u32), ("frame_ahead", i32), ("scene_in_lds", u32),
                ("host_waits", u32), ("batch_fails", u32), ("n_frames", u32), ("texels", C.c_uint64)]


class Decision(C.Structure):
    _fields_ = [("slot", i32)] + [(n, u32) for n in ("continues", "began", "plain", "in_flight", "ramp", "failed_once", "frames",
                                                     "frames_speculative")]


def frame(f, depth=4, rank=0, world=1, spp=8, waits=0, fails=0, texels=SHARE8):
    p = A.Params(width=W, height=H, number_of_bounces=4, rays_per_pixel=spp, skybox=1, frames=f, accumulate=1)
    return Call(FRAME, p, rank, world, depth, 1, waits, fails, 0, texels)


def other(kind, n_frames=0):
    return Call(kind, A.Params(), 0, 1, 0, 0, 0, 0, n_frames, 0)


def run(rt, calls):
    arr, out = (Call * len(calls))(*calls), (Decision * len(calls))()
    assert rt.load_test().rt_test_ahead_sequence(arr, len(calls), out) == 0
    return list(out)


def what(d):  # ("plain",) | ("batch", frames) | ("slot", k)
    assert (d.slot >= 0) + (d.began != 0) + d.plain == 1
    return ("slot", d.slot) if d.slot >= 0 else ("batch", d.began) if d.began else ("plain",)


def test_explicit_depth_of_four(rt):
    d = run(rt, [frame(f) for f in range(1, 11)])
    # (the call that starts a batch blends slot 0 of it)
    assert [what(x) for x in d] == [("plain",), ("batch", 4), ("slot", 1), ("slot", 2), ("slot", 3),
                                    ("batch", 4), ("slot", 1), ("slot", 2), ("slot", 3), ("batch", 4)]
    assert [x.frames for x in d] == list(range(1, 11))
    assert [x.frames_speculative for x in d] == [0, 3, 2, 1, 0, 3, 2, 1, 0, 3]
    assert [x.in_flight for x in d] == [0, 1, 1, 1, 0, 1, 1, 1, 0, 1]


def test_a_call_that_is_not_the_next_frame_drops_the_batch(rt):
    breaks = {"a changed parameter": [frame(4, spp=16)], "another rank": [frame(4, rank=1, world=2)], "another world": [frame(4, world=2)],
              "a bumped generation": [other(BUMP), frame(4)], "a frame number that skips": [frame(5)],
              "a frame number again": [frame(3)]}
    for why, tail in breaks.items():
        d = run(rt, [frame(1), frame(2), frame(3)] + tail + [frame(tail[-1].params.frames + 1, spp=tail[-1].params.rays_per_pixel,
                                                                   rank=tail[-1].rank, world=tail[-1].world)])
        assert [what(x) for x in d[:3]] == [("plain",), ("batch", 4), ("slot", 1)], why
        assert what(d[-2]) == ("plain",) and (d[-2].continues, d[-2].in_flight, d[-2].ramp) == (0, 0, 2), why
        # its frame counts as asked for; the two frames left of the batch stay speculative: nobody asked for them
        assert (d[-2].frames, d[-2].frames_speculative) == (4, 2), why
        # ... and the call behind it continues it: the next batch
        assert what(d[-1]) == ("batch", 4) and (d[-1].frames, d[-1].frames_speculative) == (5, 5), why


def test_a_launch_through_the_batched_path_ends_the_batch(rt):
    d = run(rt, [frame(1), frame(2), frame(3), other(BATCHED, 3), frame(4)])
    assert (d[3].in_flight, d[3].frames, d[3].frames_speculative) == (0, 6, 2)
    # (frame 4 follows the one-frame call for frame 3: not served from the dropped batch, it starts the next one)
    assert d[4].slot == -1 and what(d[4]) == ("batch", 4) and (d[4].frames, d[4].frames_speculative) == (7, 5)


def test_automatic_depth_ramps_up_to_the_rule(rt):
    d = run(rt, [frame(f, depth=-1) for f in range(1, 88)])
    assert what(d[0]) == ("plain",)
    assert [x.began for x in d if x.began] == [2, 4, 8, 16, 28, 28]
    assert [f for f, x in zip(range(1, 88), d) if x.began] == [2, 4, 8, 16, 32, 60]
    assert all(x.slot >= 0 for x in d[1:] if not x.began) and [x.frames for x in d] == list(range(1, 88))
    assert d[1].ramp == 4 and d[15].ramp == 32 and d[31].ramp == 64 and d[86].ramp == 64
    # a sequence that breaks starts from 2 again
    d = run(rt, [frame(f, depth=-1) for f in range(1, 10)] + [frame(20, depth=-1), frame(21, depth=-1), frame(22, depth=-1), frame(23, depth=-1)])
    assert [x.began for x in d[:9] if x.began] == [2, 4, 8] and d[8].ramp == 16
    assert what(d[9]) == ("plain",) and d[9].ramp == 2
    assert [what(x) for x in d[10:]] == [("batch", 2), ("slot", 1), ("batch", 4)]


def test_a_host_that_waits_and_a_scene_without_a_depth_render_frame_by_frame(rt):
    assert all(what(x) == ("plain",) for x in run(rt, [frame(f, depth=-1, waits=1) for f in range(1, 8)]))
    assert all(what(x) == ("plain",) for x in run(rt, [frame(f, depth=-1, texels=W * H) for f in range(1, 8)]))
    assert all(what(x) == ("plain",) for x in run(rt, [frame(f, depth=0) for f in range(1, 8)]))


def test_after_a_failed_batch_automatic_stays_off_until_the_option_is_set(rt):
    d = run(rt, [frame(1, depth=-1), frame(2, depth=-1, fails=1)] + [frame(f, depth=-1) for f in range(3, 8)] +
            [other(SET_OPTION), frame(8, depth=-1), frame(9, depth=-1), frame(10, depth=-1)])
    assert [what(x) for x in d[:7]] == [("plain",)] * 7 and [x.failed_once for x in d[:7]] == [0, 1, 1, 1, 1, 1, 1]
    assert [x.frames for x in d[:7]] == list(range(1, 8)) and all(x.frames_speculative == 0 for x in d[:7])
    assert d[7].failed_once == 0
    # (the option bumped the generation: frame 8 continues nothing, frame 9 continues frame 8)
    assert [what(x) for x in d[8:]] == [("plain",), ("batch", 2), ("slot", 1)]
    # an explicit depth is not switched off by a failure
    d = run(rt, [frame(1), frame(2, fails=1), frame(3)])
    assert [what(x) for x in d] == [("plain",), ("plain",), ("batch", 4)] and d[2].failed_once == 0
