// launch_state_entries.cpp -- TEST LIBRARY ONLY (-DRT_TEST_ENTRIES=1; the product build compiles nothing here): the entry
// points of include/rt_test_abi.h that run whole sequences of calls through the rules of launch_state.h, from a fresh state.
// Plain C++ like the rules themselves: no device, no handle (tests/test_tile_schedule_host.py,
// tests/test_ahead_sequence_host.py, tests/test_primary_choice_host.py).
#ifndef RT_TEST_ENTRIES
#define RT_TEST_ENTRIES 0
#endif
#if RT_TEST_ENTRIES
#include "launch_state.h"
#include "rt_test_abi.h"

using rt2::FrameShape;

extern "C" {

int rt_test_tile_schedule(const rt_test_tile_call* calls, uint32_t n, rt_test_tile_decision* out) {
    if (!calls || !out) return RT_ERR_INVALID_ARGUMENT;
    rt2::TileSchedule s;
    for (uint32_t i = 0; i < n; ++i) {
        const rt_test_tile_call& c = calls[i];
        if (c.flags & RT_TEST_TILE_RESET) s.reset();
        rt2::TileLaunch l;
        l.shape = FrameShape{c.width, c.height, c.rank, c.world};
        l.n_batch = c.n_batch, l.tapered_head = c.tapered_head, l.period = c.period;
        l.taper_buffer = (c.flags & RT_TEST_TILE_TAPER_BUFFER) != 0, l.taper_compiled = (c.flags & RT_TEST_TILE_TAPER_COMPILED) != 0;
        l.applies = (c.flags & RT_TEST_TILE_APPLIES) != 0;
        const rt2::TileDecision d = s.step(l);
        out[i] = rt_test_tile_decision{d.rewrite_order, (uint32_t)d.order_from, d.write_taper, d.use_order, d.take_head, d.record_costs,
                                       (uint32_t)d.record_into, s.have_order, s.costs_ready, s.order_age, (uint32_t)s.cost_slot,
                                       s.taper_head, s.taper_batch};
    }
    return RT_OK;
}
// (the calls into the sequence are render_single's, render_impl's, account_launch's and rt_set_option's, in their order)
int rt_test_ahead_sequence(const rt_test_ahead_call* calls, uint32_t n, rt_test_ahead_decision* out) {
    if (!calls || !out) return RT_ERR_INVALID_ARGUMENT;
    rt2::AheadSequence s;
    uint64_t generation = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const rt_test_ahead_call& c = calls[i];
        rt_test_ahead_decision d{};
        d.slot = -1;
        const auto launch = [&](uint32_t frames, bool blend_later) {  // render_impl, and whether it succeeds
            s.broken();
            if (blend_later && c.batch_fails) return false;
            if (!blend_later) s.launched(frames);
            return true;
        };
        if (c.kind == RT_TEST_AHEAD_BUMP) generation += 1;
        if (c.kind == RT_TEST_AHEAD_SET_OPTION) generation += 1, s.try_again();
        if (c.kind == RT_TEST_AHEAD_BATCHED) launch(c.n_frames, false);
        if (c.kind == RT_TEST_AHEAD_FRAME) {
            const rt2::FrameCall call{c.params, c.rank, c.world, generation};
            const rt2::AheadStep step = s.one_frame_call(call);
            d.slot = step.slot;
            d.continues = step.continues;
            if (step.slot >= 0) {
                s.served(call);
            } else {
                rt2::Options opt;
                opt.frame_ahead = c.frame_ahead;
                const bool automatic = opt.frame_ahead < 0;
                uint32_t depth = 0;
                if (step.continues)
                    depth = s.start_depth(rt2::ahead_depth(opt, c.params, false, s.failed_once, c.scene_in_lds != 0, c.texels, automatic && c.host_waits), automatic);
                if (depth >= 2 && launch(depth, true)) {
                    s.began(call, depth, c.texels);
                    s.remember(call);
                    d.began = depth;
                } else {
                    if (depth >= 2) s.failed(automatic);
                    launch(1u, false);
                    s.remember(call);
                    d.plain = 1;
                }
            }
        }
        d.in_flight = s.in_flight, d.ramp = s.ramp, d.failed_once = s.failed_once;
        d.frames = (uint32_t)s.frames_asked, d.frames_speculative = (uint32_t)s.frames_speculative;
        out[i] = d;
    }
    return RT_OK;
}
int rt_test_primary_choice(const int32_t* facts, uint32_t n, uint32_t* out) {
    if (!facts || !out) return RT_ERR_INVALID_ARGUMENT;
    static_assert(RT_TEST_PRIMARY_FACTS == 16 && RT_TEST_PRIMARY_CHOICE == 5, "");
    for (uint32_t i = 0; i < n; ++i) {
        const int32_t* in = facts + (size_t)i * RT_TEST_PRIMARY_FACTS;
        rt2::PrimaryFacts f;
        f.primary_table = in[0], f.primary_hits = in[1], f.primary_per_slot = in[2];
        f.camera_moved = in[3] != 0, f.n_batch = (uint32_t)in[4], f.pipelined = in[5] != 0, f.pixel_cache = (uint32_t)in[6];
        f.debug_flag = in[7], f.rays_per_pixel = in[8], f.count_tests = (uint32_t)in[9];
        f.shared = rt2::TableFacts{in[10] != 0, in[11] != 0, in[12] != 0};
        f.own = rt2::TableFacts{in[13] != 0, in[14] != 0, in[15] != 0};
        const rt2::PrimaryChoice c = rt2::choose_primary(f);
        const uint32_t words[RT_TEST_PRIMARY_CHOICE] = {c.table, c.want_hits, c.rebuild, c.sync, c.barrier};
        memcpy(out + (size_t)i * RT_TEST_PRIMARY_CHOICE, words, sizeof(words));
    }
    return RT_OK;
}

}  // extern "C"
#endif  // RT_TEST_ENTRIES
