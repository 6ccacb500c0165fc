"""The tile-feedback schedule (csrc/host/launch_state.h: TileSchedule), whole sequences of launches on the CPU: when the
tile order and the taper table are rewritten, when costs are recorded and into which of the two tables, whether a launch
uses the order and takes the tapered head.  The expected values were worked out by hand from the source of commit e4b795b
(csrc/rt_api.hip: tile_feedback), where the schedule lived among the HIP calls; nothing here is computed with the code
under test."""
import ctypes as C

u32 = C.c_uint32
BUFFER, COMPILED, APPLIES, RESET = 1, 2, 4, 8
TAPER = BUFFER | COMPILED | APPLIES
SHAPE = (1920, 1080, 0, 1)


class Call(C.Structure):
    _fields_ = [("width", u32), ("height", u32), ("rank", u32), ("world", u32), ("n_batch", u32), ("tapered_head", u32),
                ("period", C.c_int32), ("flags", u32)]


class Decision(C.Structure):
    _fields_ = [(n, u32) for n in ("rewrite_order", "order_from", "write_taper", "use_order", "take_head", "record_costs",
                                   "record_into", "have_order", "costs_ready", "order_age", "cost_slot", "taper_head",
                                   "taper_batch")]

    def state(self):
        return (self.have_order, self.costs_ready, self.order_age, self.cost_slot, self.taper_head, self.taper_batch)


def launch(n_batch=0, head=0, period=8, flags=TAPER, shape=SHAPE):
    return Call(*shape, n_batch, head, period, flags)


def run(rt, calls):
    arr, out = (Call * len(calls))(*calls), (Decision * len(calls))()
    assert rt.load_test().rt_test_tile_schedule(arr, len(calls), out) == 0
    return list(out)


def test_single_frames_refresh_every_period(rt):
    d = run(rt, [launch() for _ in range(20)])
    launches = range(1, 21)
    assert [n for n, x in zip(launches, d) if x.record_costs] == [1, 9, 17]
    assert [n for n, x in zip(launches, d) if x.rewrite_order] == [2, 10, 18]
    assert [n for n, x in zip(launches, d) if x.use_order] == list(range(2, 21))
    # the two cost tables take turns, and an order is rewritten from the table of the recording before it
    assert [x.record_into for x in d if x.record_costs] == [1, 0, 1]
    assert [x.order_from for x in d if x.rewrite_order] == [1, 0, 1]
    assert not any(x.write_taper or x.take_head for x in d)  # (single frames have no head)


def test_batches_longer_than_the_period_refresh_every_launch(rt):
    d = run(rt, [launch(20, 20) for _ in range(5)])
    assert [(x.rewrite_order, x.use_order, x.record_costs) for x in d] == [(0, 0, 1)] + [(1, 1, 1)] * 4
    assert [x.record_into for x in d] == [1, 0, 1, 0, 1]
    assert [x.order_from for x in d[1:]] == [1, 0, 1, 0]  # never the table the launch records into
    assert [x.order_age for x in d] == [20] * 5


def test_a_new_shape_and_the_options_reset_start_over(rt):
    other = (1920, 1080, 1, 2)
    d = run(rt, [launch(), launch(), launch(), launch(shape=other), launch(shape=other), launch(flags=TAPER | RESET, shape=other),
                 launch(shape=other)])
    assert [x.use_order for x in d] == [0, 1, 1, 0, 1, 0, 1]
    assert [x.rewrite_order for x in d] == [0, 1, 0, 0, 1, 0, 1]
    assert [x.record_costs for x in d] == [1, 0, 0, 1, 0, 1, 0]


def test_the_tapered_head_needs_the_table_of_this_batch_and_head(rt):
    far = 1000  # (no refresh by age)
    d = run(rt, [launch(20, 20, far), launch(20, 20, far), launch(20, 20, far), launch(10, 20, far), launch(20, 7, far),
                 launch(20, 1, far), launch(20, 20, far)])
    assert [x.rewrite_order for x in d] == [0, 1, 0, 0, 0, 0, 0] and [x.write_taper for x in d] == [0, 1, 0, 0, 0, 0, 0]
    # no order yet; a table written in this very launch; the held table; another batch size; another head; no head; held still
    assert [x.take_head for x in d] == [0, 1, 1, 0, 0, 0, 1]
    assert [x.use_order for x in d] == [0, 1, 1, 1, 1, 1, 1]
    assert (d[-1].taper_head, d[-1].taper_batch) == (20, 20)


def test_no_taper_buffer_or_no_taper_compiled_in_means_no_head(rt):
    for flags in (APPLIES | COMPILED, APPLIES | BUFFER):
        d = run(rt, [launch(20, 20, flags=flags) for _ in range(3)])
        assert [x.rewrite_order for x in d] == [0, 1, 1]
        assert not any(x.write_taper or x.take_head for x in d) and all(x.taper_head == 0 for x in d)


def test_a_rewrite_without_a_head_drops_the_held_table(rt):
    # 20 frames at period 8: the single frame behind the batches rewrites the order -- the table cut the old one
    d = run(rt, [launch(20, 20), launch(20, 20), launch(), launch(20, 20, 1000)])
    assert [x.take_head for x in d] == [0, 1, 0, 0]
    assert [x.rewrite_order for x in d] == [0, 1, 1, 0] and d[2].taper_head == 0 and d[3].use_order == 1


def test_a_launch_the_step_does_not_apply_to_leaves_the_state_untouched(rt):
    off = BUFFER | COMPILED
    d = run(rt, [launch(), launch(), launch(20, 20, flags=off), launch(flags=off, shape=(64, 64, 0, 1)), launch(period=1, flags=off),
                 launch()])
    for x in d[2:5]:
        assert x.state() == d[1].state()
        assert not any((x.rewrite_order, x.write_taper, x.use_order, x.take_head, x.record_costs))
    assert (d[5].use_order, d[5].rewrite_order, d[5].order_age) == (1, 0, 2)  # (the third launch of its shape)
