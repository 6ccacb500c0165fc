"""The option table (csrc/host/launch_options.cpp) on the CPU: every name at a grid of values against what rt_set_option
did before the options had a table (tests/golden/option_behaviour.json, recorded from commit d11ad3b: see
tests/golden/make_option_behaviour.py), and the table against the one include/rt_abi.h documents."""
import ctypes as C
import json
import os
import re

from conftest import ROOT

BOOLEAN, UPLOAD, EXPERIMENT, DROPS_PRIMARY, RESETS_TILES, CLEARS_AHEAD_FAILED, ONE_IS_AUTO, NOT_ONE = 1, 2, 4, 8, 16, 32, 64, 128
INT_MIN, INT_MAX = -2**31, 2**31 - 1
# the documented table's rows (include/rt_abi.h, the comment above rt_set_option)
HEADER_ROW = re.compile(r"^ \*   ([a-z_0-9]+)\s{2,}(.+?)\s\((-?\d+|CUs x 5)\)\s+(\(upload\))?", re.M)
EXPERIMENTS_HEADING = "Only in a library built with -DRT_EXPERIMENTS=1"


def table(rt):
    L, rows = rt.load_test(), {}
    for index in range(1000):
        name, info = C.create_string_buffer(32), (C.c_int32 * 4)()
        if L.rt_test_option_table(index, name, C.byref(info)) != 0:
            break
        assert name.value.decode() not in rows
        rows[name.value.decode()] = dict(lo=info[0], hi=info[1], default=info[2], flags=info[3])
    return rows


def set_option(rt, name, value):
    L, out = rt.load_test(), (C.c_int32 * 2)()
    rc = L.rt_test_set_option(name.encode(), value, C.byref(out))
    return rc, out[0], out[1], (L.rt_last_error(None).decode() if rc != 0 else "")


def test_every_name_and_value_does_what_the_ladder_did(rt):
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "option_behaviour.json")))
    rows = table(rt)
    assert sorted(golden["names"]) == sorted(rows) and len(rows) == 36
    assert golden["values"] == [INT_MIN, -2, -1, 0, 1, 2, 3, 7, 8, 9, 63, 64, 65, 2048, 2049, INT_MAX]
    assert golden["refused_names"] == ["", "Pipeline", "pipeline ", "no_such_option"]
    assert len(golden["cases"]) == (36 + 4) * 16
    assert {(c["name"], c["value"]) for c in golden["cases"]} == {(n, v) for n in golden["names"] + golden["refused_names"] for v in golden["values"]}
    bad = []
    for c in golden["cases"]:
        rc, stored, effects, error = set_option(rt, c["name"], c["value"])
        got = dict(name=c["name"], value=c["value"], code=rc, error=error, stored=stored if c["name"] in rows else None,
                   drops_primary=bool(effects & DROPS_PRIMARY), resets_tiles=bool(effects & RESETS_TILES),
                   clears_ahead_failed=bool(effects & CLEARS_AHEAD_FAILED))
        if got != c or effects & ~(DROPS_PRIMARY | RESETS_TILES | CLEARS_AHEAD_FAILED):
            bad.append((c, got, effects))
    assert not bad, bad[:5]
    for name in golden["refused_names"]:
        assert all(c["code"] == -1 and c["error"] == "unknown option " + name for c in golden["cases"] if c["name"] == name)


def test_the_table_is_the_one_the_header_documents(rt):
    text = open(os.path.join(ROOT, "include", "rt_abi.h")).read()
    documented = {m.group(1): m for m in HEADER_ROW.finditer(text)}
    rows = table(rt)
    assert len(documented) == 36 and set(documented) == set(rows)
    for name, m in documented.items():
        row = rows[name]
        if m.group(3) == "CUs x 5":   # (asked of the device by rt_create: nothing to store before)
            assert name == "persistent_blocks" and row["default"] == 0
        else:
            assert row["default"] == int(m.group(3)), name
        assert bool(row["flags"] & UPLOAD) == (m.group(4) is not None), name
    experiments = {n for n, m in documented.items() if m.start() > text.index(EXPERIMENTS_HEADING)}
    assert experiments == {"lds_top", "lds_tlas", "hybrid", "wavefront"}
    assert {n for n, r in rows.items() if r["flags"] & EXPERIMENT} == experiments
    # what a library built with RT_EXPERIMENTS accepts for them (commit d11ad3b's rt_set_option; this library: 0 only, above)
    assert [(rows[n]["lo"], rows[n]["hi"], bool(rows[n]["flags"] & BOOLEAN)) for n in ("lds_top", "lds_tlas", "hybrid", "wavefront")] == \
        [(-1, 2048, False), (0, 2, False), (0, 1, True), (0, 1, False)]
    # the two irregular rules are data of their rows
    assert {n for n, r in rows.items() if r["flags"] & ONE_IS_AUTO} == {"pipeline"}
    assert {n for n, r in rows.items() if r["flags"] & NOT_ONE} == {"frame_ahead"}


def test_the_python_packer_defaults_are_the_pack_rows(rt):
    rows = table(rt)
    assert rt.RayTracer.PACK_OPTIONS == {n: rows[n]["default"] for n in ("tlas", "forest", "flat2", "tlas_min", "defer_min_nodes")}
    assert {n for n, r in rows.items() if r["flags"] & UPLOAD} == set(rt.RayTracer.PACK_OPTIONS)
