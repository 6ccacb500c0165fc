"""The host packer (csrc/host/scene_pack.cpp) without a GPU: rt_test_pack_scene on the cases of _scene_pack_cases.py against
tests/golden/scene_pack_digests.json -- blob digests, layouts, facts, return codes and error texts recorded from the
packer as it was inside rt_api.hip (tests/golden/make_scene_pack_digests.py says from which commit).  The fixture is a
pin, not an expectation to refresh: a case that no longer reproduces it packs another blob."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import _scene_pack_cases as P
from conftest import GOLDEN

FIXTURE = json.load(open(os.path.join(GOLDEN, "scene_pack_digests.json")))


@pytest.fixture(scope="module")
def packed(rt):
    """name -> (blob, layout, facts) of every case, packed once."""
    return {name: rt.RayTracer.pack_scene(arrays, **options) for name, arrays, options in P.cases(rt)}


def test_the_cases_are_the_fixtures(packed):
    assert sorted(packed) == sorted(FIXTURE["cases"])


@pytest.mark.parametrize("name", sorted(FIXTURE["cases"]))
def test_case_reproduces_its_recorded_blob_layout_and_facts(packed, name):
    blob, lay, facts = packed[name]
    want = FIXTURE["cases"][name]
    assert [int(x) for x in lay] == want["layout"]
    assert [int(x) for x in facts] == want["facts"]
    assert blob.size == want["layout"][9]
    assert hashlib.sha256(blob.tobytes()).hexdigest() == want["sha256"]


def test_empty_scene_is_sixteen_zero_bytes(packed):
    blob, lay, _ = packed["empty"]
    assert blob.size == 16 and not blob.any() and int(lay[1]) == 0


def test_instance_phase_rerun_on_the_stored_geometry_gives_the_same_head(rt, packed):
    import ray_tracer_2_amd._abi as A
    k = A.PACK_FACT_FIELDS.index("rerun_same")
    assert all(int(facts[k]) == 1 for _, _, facts in packed.values())


def test_malformed_bvhs_are_refused_with_the_recorded_code_and_text(rt):
    for name, arrays in P.malformed(rt):
        with pytest.raises(rt.RtError) as e:
            rt.RayTracer.pack_scene(arrays)
        want = FIXTURE["malformed"][name]
        assert e.value.code == want["rc"] == P.INDEX_RANGE
        assert str(e.value) == f"rt error {want['rc']}: {want['error']}"


def test_coverage_condition(packed):
    """Every item kind, flag and decision named by the coverage condition occurs in some case (decoded from the item
    words, mesh records, forest entries and tree records of the packed blobs)."""
    seen = P.coverage([P.decode(*packed[name]) for name in sorted(packed)])
    assert all(seen.values()), [k for k, v in seen.items() if not v]


def test_pack_scene_is_exported_by_the_test_library_only(rt):
    from ray_tracer_2_amd import lib

    def exported(path):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    rt.load(), lib.load_test()
    assert "rt_test_pack_scene" in lib.TEST_EXPORTS and "rt_test_pack_scene" not in lib.EXPORTS
    assert "rt_test_pack_scene" in exported(lib.TEST_LIB_PATH)
    assert "rt_test_pack_scene" not in exported(lib.LIB_PATH)


def test_unknown_packer_option_is_refused(rt, packed):
    with pytest.raises(ValueError):
        rt.RayTracer.pack_scene(P.empty_scene(rt), tlas_minimum=3)
