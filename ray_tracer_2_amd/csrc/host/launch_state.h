// launch_state.h -- the rules of a handle that keep state from one call to the next: when the tile order is rewritten
// (TileSchedule), which one-frame call is served from a batch rendered ahead (AheadSequence), which primary table a launch
// reads (choose_primary).  Plain C++ without HIP, like launch_options.h: each rule takes its state and this call's facts
// and returns a decision; rt_api.hip performs the HIP calls the decision names.  Whole sequences of calls are checked on a
// machine without a GPU (tests/test_tile_schedule_host.py, tests/test_ahead_sequence_host.py,
// tests/test_primary_choice_host.py).
#ifndef RT_LAUNCH_STATE_H
#define RT_LAUNCH_STATE_H

#include "launch_options.h"  // MAX_BATCH_FRAMES, RT_FRAME_TAPER (and include/rt_abi.h: rt_params, rt_strip_texels)

namespace rt2 {

// The frame layout a buffer, a table or a history was made for: the image size and the strip split.  The default (zero)
// shape is "nothing made yet": it equals no shape a launch can have (render_impl refuses world == 0).
struct FrameShape {
    uint32_t width = 0, height = 0, rank = 0, world = 0;
    bool operator==(const FrameShape& o) const { return width == o.width && height == o.height && rank == o.rank && world == o.world; }
    bool operator!=(const FrameShape& o) const { return !(*this == o); }
    // texels of this rank's share (world == 1: the frame itself, without the padding of a ragged last strip)
    uint64_t texels() const { return world == 1 ? (uint64_t)width * height : rt_strip_texels(width, height, rank, world); }
};

// ---- the tile-feedback schedule ------------------------------------------------------------------------------------------
// Tile-cost feedback (persistent kernel, path-trace frames only): the tiles are handed out in the order of the rays each
// took in an earlier frame of the same shape, heaviest first.  Progressive accumulation re-renders the same view, so an
// order stays good: it is refreshed every `period` frames (costs are recorded in the frame before a refresh), not every
// frame.  The costs go to two tables in turn: the one a launch records into is never the one the order is rewritten from.
struct TileLaunch {
    FrameShape shape;
    uint32_t n_batch = 0;       // frames of the batch (0: a single frame)
    uint32_t tapered_head = 0;  // the frame group the launch takes if it carries a taper table (0, 1: none)
    int period = 8;             // option "tile_feedback_period"
    bool taper_buffer = false, taper_compiled = RT_FRAME_TAPER != 0;  // the handle has a taper table; the kernels read one
    // option "tile_feedback" on, no debug view, the tiles fit the tables, the persistent kernel (else: nothing happens)
    bool applies = true;
};
struct TileDecision {
    bool rewrite_order = false;  // before the launch: the order from the costs in table `order_from` ...
    int order_from = 0;
    bool write_taper = false;    // ... and the taper table of that order, for this batch size and head
    bool use_order = false;      // the launch hands its tiles out in the order
    bool take_head = false;      // ... and takes the tapered head, with the taper table
    bool record_costs = false;   // the launch records its tiles' costs into table `record_into`, zeroed first
    int record_into = 0;
};
struct TileSchedule {
    FrameShape shape;  // the frame layout the tile costs and the tile order were recorded for
    bool have_order = false, costs_ready = false;
    uint32_t order_age = 0;                    // frames rendered with the order
    int cost_slot = 0;                         // the table of the last recording
    uint32_t taper_batch = 0, taper_head = 0;  // the held taper table: for batches of taper_batch frames in groups of taper_head (0: none)

    void reset() { shape = FrameShape{}; }  // (the history starts again: no launch has the zero shape)
    TileDecision step(const TileLaunch& l) {
        TileDecision d;
        if (!l.applies) return d;
        if (shape != l.shape) have_order = costs_ready = false;
        if (!have_order) taper_head = 0;  // (a table cuts the order it was written behind)
        if (costs_ready && (!have_order || order_age >= (uint32_t)l.period)) {
            d.rewrite_order = true;
            d.order_from = cost_slot;
            // ... and, for a grouped launch, the taper of that order from the same costs (frame_taper_table)
            d.write_taper = l.taper_compiled && l.tapered_head > 1u && l.taper_buffer;
            taper_head = d.write_taper ? l.tapered_head : 0u;
            if (d.write_taper) taper_batch = l.n_batch;
            have_order = true;
            order_age = 0;
            costs_ready = false;
        }
        const uint32_t frames_now = l.n_batch ? l.n_batch : 1u;
        d.use_order = have_order;
        // The launch takes the tapered head exactly when it carries the table written for this batch size and that head --
        // held from an earlier refresh, or written just above.  (The table of another batch size or head, or no order yet:
        // the launch runs untapered, in the groups frame_group_for gave it.)
        d.take_head = have_order && l.tapered_head > 1u && taper_head == l.tapered_head && taper_batch == l.n_batch;
        if (!have_order || order_age + frames_now >= (uint32_t)l.period) {
            cost_slot ^= 1;
            d.record_costs = costs_ready = true;
            d.record_into = cost_slot;
        }
        order_age += frames_now;
        shape = l.shape;
        return d;
    }
};

// ---- frames rendered ahead (option "frame_ahead", include/rt_abi.h; the depth: ahead_depth) ----------------------------
// The one-frame call for frame f that continues the call before it renders frames f .. f + d - 1 in one batched launch
// into the batch scratch images; the next d - 1 calls only blend theirs.  A call that is not the batch's next frame -- a
// changed parameter, another rank or world, anything that bumped the handle's generation, a frame number that skips --
// drops what is left of the batch (it was never blended) and renders its own frame.
inline bool same_frame_params(const rt_params& a, const rt_params& b, int32_t b_frames) {  // (the padding is not compared)
    return a.width == b.width && a.height == b.height && a.number_of_bounces == b.number_of_bounces &&
           a.rays_per_pixel == b.rays_per_pixel && a.skybox == b.skybox && a.frames == b_frames && a.accumulate == b.accumulate &&
           a.debug_flag == b.debug_flag && a.debug_scale == b.debug_scale;
}
struct FrameCall {  // a one-frame call; `generation`: the handle's, bumped by everything that changes what a frame looks like
    rt_params params{};
    uint32_t rank = 0, world = 1;
    uint64_t generation = 0;
    // is `c` the call for the frame `step` frames behind this one, everything else equal?
    bool followed_by(const FrameCall& c, uint32_t step) const {
        return generation == c.generation && rank == c.rank && world == c.world &&
               same_frame_params(c.params, params, (int32_t)((uint32_t)params.frames + step));
    }
};
struct AheadStep {
    int32_t slot = -1;       // >= 0: the call is served from this slot of the batch in flight, nothing is launched
    bool continues = false;  // (slot < 0) the call continues the one-frame call before it: it may start a batch
};
struct AheadSequence {
    bool in_flight = false;  // a batch with slots left
    FrameCall base;          // the call that started it: slot 0
    uint32_t n = 0, next = 0;  // slots rendered / the next one to hand out
    uint64_t texels = 0;       // slot stride
    bool have_last = false;
    FrameCall last;  // the last one-frame call that succeeded
    // automatic: batches of 2, 4, 8, ... frames up to the depth while the sequence goes on, so that a host that stops after
    // n frames has had at most n rendered in vain; back to 2 when the sequence breaks
    uint32_t ramp = 2;
    bool failed_once = false;  // the batch could not be set up once (memory): automatic stays off
    // since rt_reset_timing: frames the host asked for, and frames rendered ahead that no call has asked for (yet)
    unsigned long long frames_asked = 0, frames_speculative = 0;

    // What a one-frame call does.  A batch whose next frame it is not is dropped here.
    AheadStep one_frame_call(const FrameCall& c) {
        AheadStep s;
        if (in_flight) {
            if (base.followed_by(c, next)) {
                s.slot = (int32_t)next;
                return s;
            }
            in_flight = false;  // the host went another way
            ramp = 2;
        }
        s.continues = have_last && last.followed_by(c, 1u);
        if (!s.continues) ramp = 2;
        return s;
    }
    // The frames the batch that starts now renders, from the rule's depth: an automatic depth climbs the ramp.
    uint32_t start_depth(uint32_t rule_depth, bool automatic) {
        if (!automatic || rule_depth < 2u) return rule_depth;
        const uint32_t d = std::min(rule_depth, ramp);
        ramp = ramp >= MAX_BATCH_FRAMES / 2 ? MAX_BATCH_FRAMES : ramp * 2;
        return d;
    }
    // ---- what the caller then did ----
    void launched(uint32_t frames) { frames_asked += frames; }  // a launch that blends what it renders (not a batch rendered ahead)
    void began(const FrameCall& c, uint32_t d, uint64_t slot_texels) {  // a batch of d frames was launched for `c`: slot 0 is c's
        in_flight = true;
        base = c;
        n = d;
        next = 1;
        texels = slot_texels;
        frames_asked += 1u;  // (the others count as asked for when their calls come)
        frames_speculative += d - 1u;
    }
    void served(const FrameCall& c) {  // the slot one_frame_call named was blended
        next += 1;
        frames_asked += 1;
        if (frames_speculative > 0) frames_speculative -= 1;
        if (next == n) in_flight = false;
        remember(c);
    }
    void remember(const FrameCall& c) { have_last = true, last = c; }  // c's frame is in the image
    void forget() { have_last = false; }                                // a one-frame call failed
    void failed(bool automatic) { if (automatic) failed_once = true; }  // no room for the batch: frames one by one from now on
    void try_again() { failed_once = false; }                           // (the option was set again)
    void broken() { in_flight = false; }  // whatever launches breaks the sequence; what is left of a batch is dropped
    void reset_counts() { frames_asked = frames_speculative = 0; }
};

// ---- the primary table of a launch --------------------------------------------------------------------------------------
// Which table of primary rays (and, option "primary_hits", their hits) a launch reads: none -- every pixel computes its
// own memo --, the shared one, or the pipeline slot's own.  A frame whose camera is not the last sampled frame's (the
// camera is MOVING) renders without a table: building one that the next frame throws away costs more than it saves
// (config 2: 1.32 ms per frame of a moving camera with a table per frame, 1.24 without); a batch keeps the table whatever
// the camera did, its frames share it.  A pipelined frame whose camera (or shape) is not the shared table's builds a
// table of its OWN pipeline slot on its own stream -- ordered behind that slot's previous frame and read by nobody else,
// so no frame in flight has to finish first (option "primary_per_slot").  A table that would have to be allocated beyond
// option "max_device_mb" is done without; a slot table likewise falls back to the shared one.
struct SampledCamera {  // the camera of the last frame that took samples (the comparison is the caller's: a memcmp)
    rt_camera_uniform camera{};
    bool valid = false;
    void sampled(const rt_camera_uniform& c) { camera = c, valid = true; }
};
struct TableFacts {
    bool serves = false;        // as it stands: this camera, shape, with hits if wanted
    bool large_enough = false;  // holds the launch's texels
    bool may_grow = false;      // the cap on device memory leaves room for one that does
    bool fits() const { return large_enough || may_grow; }
};
struct PrimaryFacts {
    int primary_table = 1, primary_hits = 1, primary_per_slot = 1;  // the options
    bool camera_moved = false;  // the camera differs from the last sampled frame's
    uint32_t n_batch = 0;
    bool pipelined = false;
    uint32_t pixel_cache = 1;
    int32_t debug_flag = 0, rays_per_pixel = 1;
    uint32_t count_tests = 0;
    TableFacts shared, own;
};
// (the counter kernels re-intersect every segment, so a launch with counters neither needs nor fills the hits)
inline bool primary_wants_hits(int primary_hits, uint32_t count_tests) { return primary_hits != 0 && count_tests == 0u; }
struct PrimaryChoice {
    enum Table : uint32_t { NONE = 0, SHARED = 1, OWN = 2 };
    // Whoever may still read a table that has to grow finishes first: the slot's previous frame read its own (SLOT_STREAM),
    // pipelined frames read the shared one on their own streams (DRAIN_STREAMS).
    enum Sync : uint32_t { NO_SYNC = 0, SLOT_STREAM = 1, DRAIN_STREAMS = 2 };
    Table table = NONE;
    bool want_hits = false;
    bool rebuild = false;  // the table does not serve as it stands: make it (grown if it is too small)
    Sync sync = NO_SYNC;   // ... after this
    bool barrier = false;  // ... and after the other streams' sampling launches: they read the shared table (barrier_other)
};
inline PrimaryChoice choose_primary(const PrimaryFacts& f) {
    PrimaryChoice c;
    if (!(f.primary_table && f.shared.fits() && f.pixel_cache != 0 && f.debug_flag == 0 && f.rays_per_pixel > 0 &&
          !(f.camera_moved && f.n_batch == 0)))
        return c;
    c.want_hits = primary_wants_hits(f.primary_hits, f.count_tests);
    const bool use_own = f.pipelined && !f.shared.serves && f.primary_per_slot != 0 && f.own.fits();
    const TableFacts& t = use_own ? f.own : f.shared;
    c.table = use_own ? PrimaryChoice::OWN : PrimaryChoice::SHARED;
    if (!t.serves) {
        c.rebuild = true;
        if (!t.large_enough) c.sync = use_own ? PrimaryChoice::SLOT_STREAM : PrimaryChoice::DRAIN_STREAMS;
        c.barrier = !use_own;
    }
    return c;
}

}  // namespace rt2

#endif
