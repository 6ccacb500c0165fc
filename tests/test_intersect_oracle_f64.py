"""The oracle's ray-scene intersection (oracle/shader_oracle.cpp calculate_ray_collions, which the kernels equal bit for
bit: tests/test_gpu_intersect.py) against the float64 brute force of oracle/independent_f64.py, one ray at a time, on the
ray families of tests/_ray_families.py -- the geometry images never reach.

The oracle walks the same BVH through the same binary32 slab test as the kernels, so a ray both mishandle alike (a leaf box
that misses its triangle after rounding, a builder bug) is invisible to every parity test.  The float64 reference tests
every triangle and has no BVH.  On every ray it does not flag as ambiguous (independent_f64.ambiguity: binary32 may
legitimately decide otherwise) the two must agree on hit / miss, the winner and the back face, and on distance, point,
normal and uv within 1e-5 of the scene's scale (north_star's tolerance), widened where binary32's own error bound for
the winner is wider (ambiguity's dst_tol / uv_tol / normal_tol: grazing hits, small triangles far from the origin,
spheres away from it).  The one exception the shader itself makes is
asserted, not skipped: its 32-entry stack clamps (wgsl:297) in meshes of BVH height >= 32, where the oracle may miss what
the float64 walk hits."""
import numpy as np
import pytest

import _ray_families as RF
from oracle import independent_f64 as F

# Largest fraction of ambiguous rays a random family may have (measured: <= 0.02 % on every scene below but the tie
# scenes, whose duplicated geometry -- and in "glass" the face the opaque and the glass box share -- makes equal distances
# on purpose).  A larger fraction means the margins have grown so wide that the comparison stops saying anything.
RANDOM_AMBIGUOUS_MAX = 0.005
TIE_SCENES = ("ties", "ties_tlas", "glass")
N_RANDOM = 100000


def mesh_bvh_height(arrays, mi):
    """The upload's mesh_bvh_height (csrc/rt_api.hip): the depth of the deepest leaf, the root at depth 0."""
    nodes, off = arrays.nodes, int(arrays.meshes[mi]["node_offset"])
    st, h = [(0, 0)], 0
    while st:
        i, d = st.pop()
        h = max(h, d)
        if nodes[off + i]["count"] == 0:
            st += [(int(nodes[off + i]["left"]), d + 1), (int(nodes[off + i]["right"]), d + 1)]
    return h


def scene_scale(arrays):
    lo, hi = RF._bounds(arrays)
    return max(1.0, float(np.abs(np.concatenate([lo, hi])).max()))


def compare(arrays, rec, ro, rd, fscene=None):
    """Per-ray comparison of probe records (oracle or kernel) for rays (ro, rd), rd normalized, with the float64
    reference.  Returns a dict of counts and the indices of the disagreements outside the ambiguous rays."""
    fscene = fscene or F.Scene(arrays)
    ro64, rd64 = ro.astype(np.float64), rd.astype(np.float64)
    hit, dst, point, normal, uv, which, backface = F.closest_hit(fscene, ro64, rd64)
    am = F.ambiguity(fscene, ro64, rd64)
    amb = am["ambiguous"]
    f = rec.view(np.float32)
    r_hit = rec[:, 0] == 1
    tol = 1e-5 * scene_scale(arrays)
    win = np.where(hit, which, -1)
    r_win = np.where(r_hit, rec[:, 11].astype(np.int64), -1)
    both = hit & r_hit
    with np.errstate(invalid="ignore"):
        close = (np.abs(f[:, 1] - dst) <= tol + am["dst_tol"]) & (np.abs(f[:, 2:5] - point).max(1) <= tol + am["dst_tol"]) & \
                (np.abs(f[:, 5:8] - normal).max(1) <= 1e-5 + am["normal_tol"]) & \
                (np.abs(f[:, 8:10] - uv).max(1) <= 1e-5 + am["uv_tol"])
    same = (hit == r_hit) & (win == r_win) & (~both | ((rec[:, 10] == 1) == backface)) & (~both | close)
    deep = {mi for mi in range(len(arrays.meshes)) if mesh_bvh_height(arrays, mi) >= 32}
    # the shader's clamped stack may lose the float64 winner in a deep mesh: the oracle then reports a farther hit or none
    lost = ~same & hit & np.isin(win, list(deep)) & (~r_hit | (f[:, 1] > dst))
    bad = np.flatnonzero(~same & ~amb & ~lost)
    return dict(rays=len(ro), ambiguous=int(amb.sum()), deep_misses=int((lost & ~amb).sum()), bad=bad, hit=hit, amb=amb,
                win=win, r_win=r_win, dst=dst)


SCENES = RF.LIBRARY + RF.BUILT


@pytest.mark.parametrize("name", SCENES)
def test_oracle_equals_the_f64_reference_on_every_family(rt, oracle, name):
    arrays = RF.scene(rt, name)
    fscene = F.Scene(arrays)
    lines = []
    for fam, (ro, rd) in RF.families(arrays, name, n_random=N_RANDOM).items():
        rd = RF.normalized(rd)
        rec = oracle.intersect(arrays, ro, rd)
        c = compare(arrays, rec, ro, rd, fscene)
        lines.append(f"{fam} {c['rays']} rays, {c['ambiguous']} ambiguous, {c['deep_misses']} lost to the clamped stack")
        b = c["bad"]
        assert b.size == 0, (f"{name}/{fam}: {b.size} rays disagree, first ray {ro[b[0]].tolist()} {rd[b[0]].tolist()}: "
                             f"f64 winner {c['win'][b[0]]} at {c['dst'][b[0]]}, oracle {c['r_win'][b[0]]} at "
                             f"{rec[b[0], 1:2].view(np.float32)[0]}")
        if fam == "random" and name not in TIE_SCENES:
            assert c["ambiguous"] <= RANDOM_AMBIGUOUS_MAX * c["rays"], (name, c["ambiguous"])
        if c["deep_misses"]:
            assert any(mesh_bvh_height(arrays, mi) >= 32 for mi in range(len(arrays.meshes))), name
    print(f"\n{name}: " + "; ".join(lines))


@pytest.mark.parametrize("name", ["height30", "height31", "height32", "height33"])
def test_chain_scenes_have_the_heights_they_name(rt, name):
    """The boundary of the shader's stack: heights 30 and 31 are walked with the kernels' own stack, 32 and up with the
    literal, clamped one (DMESH_DEEP: height + 1 > RT_BVH_STACK)."""
    arrays = RF.scene(rt, name)
    assert mesh_bvh_height(arrays, 0) == int(name[6:])


@pytest.mark.parametrize("name,leaf", [("leaf127", 127), ("leaf128", 128)])
def test_leaf_scenes_put_a_leaf_of_that_size_on_the_stack(rt, name, leaf):
    arrays = RF.scene(rt, name)
    n = arrays.nodes[int(arrays.meshes[1]["node_offset"]):]
    assert n[0]["count"] == 0 and n[n[0]["left"]]["count"] == 0   # (below an internal child of the root: stacked)
    assert max(int(c) for c in n["count"]) == leaf


def test_ambiguity_flags_the_edges_of_a_triangle_and_not_its_inside():
    """ambiguity's margins on one triangle: a ray through the middle is certain, one through a vertex, an edge, along the
    plane or from EPSILON off it is not."""
    arrays = RF.make_arrays([dict(tris=RF.quad((0, 0, 0), (1, 0, 0), (0, 1, 0))[:1], bvh=("rootleaf",))])
    fs = F.Scene(arrays)
    # (|cross(e_ab, e_ac)| = 4: a direction 2.5e-9 off the plane has det = 1e-8, the cull threshold)
    ro = np.array([[-0.3, -0.6, 1], [-1, -1, 1], [0, -1, 1], [-2, -0.6, 4e-9], [-0.3, -0.6, 1e-5], [-0.3, -0.6, 3]])
    rd = np.array([[0, 0, -1], [0, 0, -1], [0, 0, -1], [1, 0, -2.5e-9], [0, 0, -1], [0, 0, 1]], np.float64)
    a = F.ambiguity(fs, ro, F.normalize(rd))
    assert a["ambiguous"].tolist() == [False, True, True, True, True, False]
    assert a["bary"][1] < 1 and a["bary"][2] < 1 and a["det"][3] < 1 and a["eps"][4] < 1
