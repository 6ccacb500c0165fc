"""Writes tests/golden/option_behaviour.json: what rt_set_option does with every option name at a grid of values, and with
names it must refuse -- per case the return code, the error text, the value then in force and the three side effects on
the handle (primary tables invalidated, tile history reset, frame_ahead_failed cleared).

PROVENANCE: the committed fixture was recorded ONCE, from commit d11ad3b -- the last one whose rt_set_option was an
if / else-if ladder over some forty fields of rt_handle -- through a throw-away shim that is not committed: a test entry

    int rt_shim_set_option(const char* name, int value, long long out[5], char* err, int err_bytes)

that built an rt_handle on the stack with primary.valid and every slot's primary.valid set, a non-empty `history` and
frame_ahead_failed = true, called that commit's rt_set_option on it, checked that `generation` went up by one, and
returned the code, the handle's error text and out = {name known to the shim, the field read back by a hand-written
map (max_device_bytes >> 20, !force_global, use_primary, pixel_cache_opt, force_stack_wide, batch_frames_opt, ...),
all tables invalid, history == FrameShape{}, !frame_ahead_failed}.  Usage then: python make_option_behaviour.py <shim .so>.
The fixture pins the option table (csrc/host/launch_options.cpp) to that behaviour: do not regenerate it from later code
(a changed record is a changed option, which tests/test_options_host.py has to report, not absorb).  The script refuses
to run while the fixture exists."""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
INT_MIN, INT_MAX = -2**31, 2**31 - 1
VALUES = [INT_MIN, -2, -1, 0, 1, 2, 3, 7, 8, 9, 63, 64, 65, 2048, 2049, INT_MAX]
NAMES = ["kernel_variant", "persistent_blocks", "specialise", "lds_scene", "pixel_cache", "primary_table", "primary_hits",
         "max_device_mb", "memo_in_table", "vote_eighths", "vote_patience", "tile_feedback", "tile_feedback_period", "pipeline",
         "pipeline_when_idle", "primary_per_slot", "frame_ahead", "cross_prune", "batch_frames", "batch_tile_major", "forest",
         "flat2", "stack_wide", "tlas", "tlas_min", "cull_roots", "sort_rounds", "defer_min_nodes", "fast_miss", "roulette_skip",
         "park_levels", "multi_rccl", "lds_top", "lds_tlas", "hybrid", "wavefront"]
REFUSED_NAMES = ["", "Pipeline", "pipeline ", "no_such_option"]

if __name__ == "__main__":
    FIXTURE = os.path.join(HERE, "option_behaviour.json")
    if os.path.exists(FIXTURE):
        raise SystemExit(f"{FIXTURE} exists: it pins the options to commit d11ad3b and is not refreshed from later code")
    shim = C.CDLL(sys.argv[1]).rt_shim_set_option
    shim.restype, shim.argtypes = C.c_int, [C.c_char_p, C.c_int, C.POINTER(C.c_longlong * 5), C.c_char_p, C.c_int]
    assert len(NAMES) == 36 and len(set(NAMES)) == 36
    cases = []
    for name in NAMES + REFUSED_NAMES:
        for value in VALUES:
            out, err = (C.c_longlong * 5)(), C.create_string_buffer(1024)
            rc = shim(name.encode(), value, C.byref(out), err, 1024)
            assert rc != -1000, "generation was not bumped exactly once"
            assert bool(out[0]) == (name in NAMES), name
            cases.append(dict(name=name, value=value, code=rc, error=err.value.decode(), stored=int(out[1]) if out[0] else None,
                              drops_primary=bool(out[2]), resets_tiles=bool(out[3]), clears_ahead_failed=bool(out[4])))
    with open(FIXTURE, "w") as f:
        f.write('{"values": %s,\n "names": %s,\n "refused_names": %s,\n "cases": [\n' %
                (json.dumps(VALUES), json.dumps(NAMES), json.dumps(REFUSED_NAMES)))
        f.write(",\n".join("  " + json.dumps(c) for c in cases))
        f.write("\n ]}\n")
