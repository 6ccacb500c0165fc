"""Writes tests/golden/scene_pack_digests.json: per case of tests/_scene_pack_cases.py the sha256 of the packed blob, its
12 layout words and the fact words of rt_test_pack_scene; per malformed input the return code and the error text.

PROVENANCE: the committed fixture was recorded ONCE, from commit d75b674 -- the last one whose packer was
build_geometry / build_instances inside csrc/rt_api.hip -- with rt_test_pack_scene as a thin shim over those two
functions.  It pins the refactored packer (csrc/host/scene_pack.cpp) to that behaviour: do not regenerate it from later
code (a changed digest is a changed blob, which tests/test_scene_pack_host.py has to report, not absorb).  The script
refuses to run while the fixture exists."""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import ray_tracer_2_amd as rt  # noqa: E402
import _scene_pack_cases as P  # noqa: E402

if __name__ == "__main__":
    FIXTURE = os.path.join(HERE, "scene_pack_digests.json")
    if os.path.exists(FIXTURE):
        raise SystemExit(f"{FIXTURE} exists: it pins the packer to commit d75b674 and is not refreshed from later code")
    out, decoded = {"cases": {}, "malformed": {}}, []
    for name, arrays, options in P.cases(rt):
        blob, lay, facts = rt.RayTracer.pack_scene(arrays, **options)
        out["cases"][name] = dict(sha256=hashlib.sha256(blob.tobytes()).hexdigest(), layout=[int(x) for x in lay],
                                  facts=[int(x) for x in facts])
        decoded.append(P.decode(blob, lay, facts))
    for name, arrays in P.malformed(rt):
        try:
            rt.RayTracer.pack_scene(arrays)
            raise SystemExit(f"{name}: packed")
        except rt.RtError as e:
            out["malformed"][name] = dict(rc=e.code, error=str(e).split(": ", 1)[1])
    missing = [k for k, v in P.coverage(decoded).items() if not v]
    if missing:
        raise SystemExit(f"coverage condition not met: {missing}")
    with open(FIXTURE, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
