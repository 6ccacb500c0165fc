"""The families of nodes that tests/test_bvh_search_host.py (host search) and tests/test_gpu_bvh_search.py (device search)
put through rt_test_sah_search (include/rt_test_abi.h) and compare with tests/_sah_reference.py.  Seeded and
deterministic.  A case is (tri9 [n, 9] f32, order [n] u32, levels): `levels` is a list of QUERY arrays, which go through
one search object in turn.  No query of a case is left out of a comparison."""
import numpy as np

import _sah_reference as ref

F32 = np.float32
QUERY = np.dtype([("start", "<u4"), ("count", "<u4"), ("aabb_min", "<f4", 3), ("aabb_max", "<f4", 3)])
RESULT = np.dtype([("axis", "<i4"), ("pos", "<f4"), ("cost", "<f4")])
SIZES = (2, 3, 63, 64, 65, 191, 192, 193, 511, 512, 513, 1023, 1024, 1025, 1537, 5000)


# ---- the entry point ---------------------------------------------------------------------------------------------------
def search(rt, device, tri9, order, levels):
    """rt_test_sah_search: one RESULT per query, level after level.  Raises RtError with the library's text."""
    from ray_tracer_2_amd.lib import RtError
    L = rt.load_test()
    tri9 = np.ascontiguousarray(tri9, F32).reshape(-1, 9)
    order = np.ascontiguousarray(order, np.uint32)
    q = np.ascontiguousarray(np.concatenate([np.asarray(l, QUERY).reshape(-1) for l in levels]) if levels else np.zeros(0, QUERY))
    counts = np.array([len(l) for l in levels], np.uint32)
    out = np.zeros(len(q), RESULT)
    out["axis"] = -7   # (every record must be written)
    rc = L.rt_test_sah_search(int(device), tri9.ctypes.data, len(tri9), order.ctypes.data, q.ctypes.data,
                              counts.ctypes.data, len(counts), out.ctypes.data)
    if rc < 0:
        raise RtError(rc, L.rt_last_error(None).decode())
    return out


def reference(tri9, order, levels):
    """The same results from tests/_sah_reference.py (nodes of equal size are priced together)."""
    q = np.concatenate([np.asarray(l, QUERY).reshape(-1) for l in levels])
    out = np.zeros(len(q), RESULT)
    for count in np.unique(q["count"]):
        k = np.flatnonzero(q["count"] == count)
        a, p, c = ref.find_best_split(tri9, order, q["start"][k], count, q["aabb_min"][k], q["aabb_max"][k])
        out["axis"][k], out["pos"][k], out["cost"][k] = a, p, c
    return out


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def assert_same(got, want, what):
    """The issue's rule: the axis exactly, the position bit for bit, the cost by value (== or both NaN).  Returns how
    many zero costs differ in sign (compared by value like every other: outside the contract, counted for the record)."""
    assert len(got) == len(want)
    bad = np.flatnonzero(got["axis"] != want["axis"])
    assert bad.size == 0, (what, "axis", bad[:8], got[bad[:8]], want[bad[:8]])
    bad = np.flatnonzero(bits(got["pos"]) != bits(want["pos"]))
    assert bad.size == 0, (what, "pos", bad[:8], got[bad[:8]], want[bad[:8]])
    same = (got["cost"] == want["cost"]) | (np.isnan(got["cost"]) & np.isnan(want["cost"]))
    bad = np.flatnonzero(~same)
    assert bad.size == 0, (what, "cost", bad[:8], got[bad[:8]], want[bad[:8]])
    return int(np.count_nonzero(bits(got["cost"]) != bits(want["cost"])))


# ---- building blocks ---------------------------------------------------------------------------------------------------
def tri9_of(P):
    """Centroid, min, max of triangles P [n, 3, 3] with the builder's f32 operations (bvh.rs:233-238)."""
    P = np.asarray(P, F32)
    c = (((P[:, 0] + P[:, 1]).astype(F32) + P[:, 2]).astype(F32) * F32(1.0 / 3.0)).astype(F32)
    return np.concatenate([c, P.min(1), P.max(1)], 1).astype(F32)


def soup(rng, n, spread=1.0, size=0.1):
    return tri9_of(rng.uniform(-spread, spread, (n, 1, 3)) + rng.uniform(-size, size, (n, 3, 3)))


def tight(tri9, order, start, count):
    t = tri9[order[start:start + count]]
    with np.errstate(all="ignore"):
        return np.fmin.reduce(t[:, 3:6], 0), np.fmax.reduce(t[:, 6:9], 0)


def queries(tri9, order, nodes, boxes=None):
    """QUERY records of nodes [(start, count)]: the tight box of each node's triangles unless `boxes` gives (min, max)."""
    q = np.zeros(len(nodes), QUERY)
    for k, (s, c) in enumerate(nodes):
        q[k]["start"], q[k]["count"] = s, c
        q[k]["aabb_min"], q[k]["aabb_max"] = boxes[k] if boxes is not None else tight(tri9, order, s, c)
    return q


# ---- sizes -------------------------------------------------------------------------------------------------------------
def case_sizes():
    """~6,000 triangles; the counts around the 64-lane, 192-thread and 512-triangle seams, at start 0 and at odd offsets
    (chunks straddle)."""
    rng = np.random.default_rng(101)
    t = soup(rng, 6001)
    order = rng.permutation(6001).astype(np.uint32)
    nodes = [(s, c) for c in SIZES for s in (0, 1, 333, 777, 6001 - c) if s + c <= 6001]
    return t, order, [queries(t, order, nodes)]


def case_big(n):
    """One node of n triangles (n / 512 partials for the combine kernel) at an odd start."""
    rng = np.random.default_rng(n)
    t = soup(rng, n + 11, spread=4.0, size=0.05)
    order = rng.permutation(n + 11).astype(np.uint32)
    return t, order, [queries(t, order, [(7, n)])]


# ---- many nodes --------------------------------------------------------------------------------------------------------
def case_many_nodes():
    """One level of 70,000 nodes of 2 or 3 triangles (more workgroups than 65,535) shuffled with nodes of 513 .. 2,000, so
    that one-chunk and multi-chunk nodes, and the partial indices handed out in between, interleave."""
    rng = np.random.default_rng(202)
    counts = np.concatenate([rng.integers(2, 4, 70000), [513, 700, 1024, 1025, 1500, 2000]])
    counts = counts[rng.permutation(len(counts))]
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    n = int(counts.sum())
    # neighbouring triangles lie close together, as the nodes deep in a tree do
    t = tri9_of(np.repeat(rng.uniform(-5, 5, (n // 2 + 1, 1, 3)), 2, 0)[:n] + rng.uniform(-0.05, 0.05, (n, 3, 3)))
    order = np.arange(n, dtype=np.uint32)
    q = np.zeros(len(counts), QUERY)
    q["start"], q["count"] = starts, counts
    with np.errstate(all="ignore"):
        q["aabb_min"] = np.fmin.reduceat(t[:, 3:6], starts, 0)
        q["aabb_max"] = np.fmax.reduceat(t[:, 6:9], starts, 0)
    return t, order, [q]


# ---- successive levels -------------------------------------------------------------------------------------------------
def case_levels():
    """Several levels through one search object, the numbers of queries, workgroups, multi-chunk nodes and partials growing
    and shrinking in turn (every device buffer is reallocated at least once, and reused below its capacity after)."""
    rng = np.random.default_rng(303)
    n = 6000
    t = soup(rng, n)
    order = rng.permutation(n).astype(np.uint32)
    shapes = [(1, 6000), (8, 750), (300, 20), (0, 0), (3000, 2), (40, 150), (2, 3000), (10, 600), (1, 2), (5, 1100), (900, 5)]
    levels = []
    for k, c in shapes:
        levels.append(queries(t, order, [(i * c + (n - k * c) // 2, c) for i in range(k)]))
    return t, order, levels


# ---- boxes -------------------------------------------------------------------------------------------------------------
def _ulps(x, d):
    x = F32(x)
    for _ in range(abs(d)):
        x = np.nextafter(x, F32(np.inf if d > 0 else -np.inf), dtype=F32)
    return x


def integer_ratio_sizes(M):
    """{k: (s-, s, s+)} for k = 1 .. 50: an axis size s with f32(f32(s / M) * 50) == k exactly, and its neighbours one ulp
    either side.  Where binary32 has no such s (the products step over 15, 27 and 30: their quotients' ulp times 50 exceeds
    the product's ulp), s is the last size whose product is below k, so that the three still straddle the boundary."""
    out = {}
    for k in range(1, 51):
        near = F32(F32(k) * F32(M) / F32(50))
        around = [_ulps(near, d) for d in range(-8, 9)]
        value = [F32(F32(x / F32(M)) * F32(50)) for x in around]
        hits = [x for x, v in zip(around, value) if v == F32(k)] or [[x for x, v in zip(around, value) if v < F32(k)][-1]]
        out[k] = (_ulps(hits[0], -1), hits[0], _ulps(hits[0], 1))
    return out


def case_box_ratios():
    """Boxes whose short axes make axis_size / max_axis * 50 an exact integer, and one ulp either side of one: every
    n_split_tests from 1 to 50, with each axis in turn the longest; and very short axes.  The boxes are given, not
    the tight ones: triangles stick out of them."""
    rng = np.random.default_rng(404)
    t = tri9_of(rng.uniform(0, 48, (200, 1, 3)) + rng.uniform(-1, 1, (200, 3, 3)))
    order = rng.permutation(200).astype(np.uint32)
    boxes = []
    corner = np.array([1.0, 0.5, 0.25], F32)
    for M in (F32(50.0), F32(64.0), F32(3.7)):
        sizes = integer_ratio_sizes(M)
        for k, three in sizes.items():
            other = sizes.get(51 - k, three)[1]
            for size in three:
                for long_axis in range(3):
                    e = np.roll(np.array([M, size, other], F32), long_axis)
                    boxes.append((np.zeros(3, F32), e))                       # extents exactly e
                    boxes.append((corner, (corner + e).astype(F32)))          # extents as they round
    for tiny in (1e-6, 1e-30, 1e-44):
        for long_axis in range(3):
            boxes.append((np.zeros(3, F32), np.roll(np.array([40.0, tiny, 7.0], F32), long_axis)))
    n = ref.n_split_tests(np.array([b[0] for b in boxes]), np.array([b[1] for b in boxes]))
    assert set(range(1, 51)) <= set(n.reshape(-1).tolist())
    return t, order, [queries(t, order, [(0, 200)] * len(boxes), boxes)]


def case_flat():
    """Zero extent on one, two and three axes (200 and 700 triangles: one chunk and two)."""
    rng = np.random.default_rng(505)
    parts, nodes = [], []
    for n in (200, 700):
        for flat in ((0,), (1,), (2,), (0, 1), (0, 2), (1, 2), (0, 1, 2)):
            P = rng.uniform(-1, 1, (n, 1, 3)) + rng.uniform(-0.1, 0.1, (n, 3, 3))
            P = np.round(P, 2)   # (ties as well)
            for a in flat:
                P[:, :, a] = 0.375
            nodes.append((sum(len(p) for p in parts), n))
            parts.append(tri9_of(P))
    t = np.concatenate(parts)
    order = np.arange(len(t), dtype=np.uint32)
    return t, order, [queries(t, order, nodes)]


def case_loose_boxes():
    """Query boxes larger than the tight box of the triangles, up to planes that leave one side empty (0 * inf = NaN: must
    lose)."""
    rng = np.random.default_rng(606)
    t = soup(rng, 3000)
    order = rng.permutation(3000).astype(np.uint32)
    nodes, boxes = [], []
    for c in (2, 40, 512, 513, 1400):
        for s in (0, 101, 3000 - c):
            lo, hi = tight(t, order, s, c)
            for grow in (0.01, 0.5, 3.0, 40.0):
                g = rng.uniform(0, grow, 6).astype(F32)
                nodes.append((s, c))
                boxes.append(((lo - g[:3]).astype(F32), (hi + g[3:]).astype(F32)))
    return t, order, [queries(t, order, nodes, boxes)]


# ---- values ------------------------------------------------------------------------------------------------------------
def case_on_the_plane():
    """Centroids with the exact bits of candidate positions (`<` is strict: they go right), and one ulp either side."""
    rng = np.random.default_rng(707)
    parts, nodes, boxes = [], [], []
    for n in (2, 3, 150, 600) * 6:
        mn = rng.uniform(-4, 4, 3).astype(F32)
        mx = (mn + np.roll(np.array([2.0, 1.4, 0.62], F32) * rng.uniform(0.2, 1, 3).astype(F32), rng.integers(0, 3))).astype(F32)
        pos, valid = ref.candidates(mn, mx)
        pos = pos.reshape(3, 50)
        valid = valid.reshape(3, 50)
        c = np.zeros((n, 3), F32)
        for a in range(3):
            planes = pos[a][valid[a]]
            pick = planes[rng.integers(0, len(planes), n)]
            step = rng.integers(-1, 2, n)
            c[:, a] = np.where(step == 0, pick, np.where(step < 0, np.nextafter(pick, F32(-np.inf)), np.nextafter(pick, F32(np.inf))))
        half = rng.uniform(0.0, 0.05, (n, 3)).astype(F32)
        nodes.append((sum(len(p) for p in parts), n))
        boxes.append((mn, mx))
        parts.append(np.concatenate([c, (c - half).astype(F32), (c + half).astype(F32)], 1))
    t = np.concatenate(parts)
    order = np.arange(len(t), dtype=np.uint32)
    return t, order, [queries(t, order, nodes, boxes)]


def case_ties():
    """Lattices of equal triangles, mirror-symmetric about their centre and the same along every axis: many candidates,
    on all three axes, cost the same, and the first in axis-major order must win.  All triangles identical: no plane
    separates anything."""
    rng = np.random.default_rng(808)
    parts, nodes = [], []

    def add(P):
        nodes.append((sum(len(p) for p in parts), len(P)))
        parts.append(tri9_of(P))

    shape = np.array([[0, 0, 0], [0.5, 0.25, 0], [0.25, 0.5, 0.5]], F32)
    sym = np.array([[-0.25, -0.25, -0.25], [0.25, 0.25, 0.25], [0, 0, 0]], F32)   # (its box is a cube about its centroid)
    for side in (2, 4, 8, 9, 12):
        g = np.stack(np.meshgrid(*[np.arange(side, dtype=F32)] * 3, indexing="ij"), -1).reshape(-1, 1, 3)
        add(g + shape[None])
        add(g - F32((side - 1) / 2) + sym[None])                      # mirror-symmetric about the origin, cubic
        add((g - F32((side - 1) / 2))[rng.permutation(len(g))] + sym[None])
    for sides in ((3, 8, 8), (8, 3, 8), (8, 8, 3), (2, 12, 12), (12, 12, 2), (5, 5, 20), (20, 4, 20)):   # two axes tie
        g = np.stack(np.meshgrid(*[np.arange(k, dtype=F32) for k in sides], indexing="ij"), -1).reshape(-1, 1, 3)
        add(g + sym[None])
        add(g[rng.permutation(len(g))] + shape[None])
    g2 = np.stack(np.meshgrid(np.arange(40, dtype=F32), np.arange(30, dtype=F32), indexing="ij"), -1).reshape(-1, 1, 2)
    add(np.concatenate([g2, np.zeros_like(g2[..., :1])], -1) + shape[None])   # a regular grid in a plane
    for n in (2, 513, 1000):
        add(np.repeat(shape[None], n, 0))
    t = np.concatenate(parts)
    order = np.arange(len(t), dtype=np.uint32)
    return t, order, [queries(t, order, nodes)]


def case_signed_zeros():
    """Signed zeros in min, max and centroid: flat sides at +-0, boxes whose corners are zeros of either sign."""
    rng = np.random.default_rng(909)
    parts, nodes = [], []
    z = np.array([0.0, -0.0], F32)
    for n in (2, 64, 513, 900):
        for flat in ((0,), (1, 2), ()):
            t = soup(rng, n, spread=1.0, size=0.2)
            t[rng.random(t.shape) < 0.15] = 0.0
            neg = rng.random(t.shape) < 0.5
            t = np.where((t == 0) & neg, F32(-0.0), t).astype(F32)
            for a in flat:   # a side that is a zero of random sign in every field
                for f in (a, 3 + a, 6 + a):
                    t[:, f] = z[rng.integers(0, 2, n)]
            nodes.append((sum(len(p) for p in parts), n))
            parts.append(t)
    t = np.concatenate(parts)
    order = np.arange(len(t), dtype=np.uint32)
    q = queries(t, order, nodes)
    q2 = q.copy()   # the same nodes with the zeros of the boxes flipped
    for f in ("aabb_min", "aabb_max"):
        q2[f] = np.where(q2[f] == 0, -q2[f], q2[f])
    return t, order, [np.concatenate([q, q2])]


def case_overflow():
    """Coordinates near 1e19: half areas, and counts times half areas, overflow to +inf on the big sides and stay finite
    on small ones (a cluster of random size and share at one end of the x axis)."""
    rng = np.random.default_rng(1010)
    parts, nodes = [], []
    for n in (3, 100, 513, 1200):
        for spread in (1e19, 5e18, 2e19):
            for _ in range(6):
                nodes.append((sum(len(p) for p in parts), n))
                t = soup(rng, n, spread=spread, size=spread * 1e-3)
                t *= np.tile(np.roll([1.0, 10.0 ** rng.uniform(-5, 0), 10.0 ** rng.uniform(-5, 0)], rng.integers(0, 3)), 3).astype(F32)
                k = max(1, int(n * rng.uniform(0.2, 0.9)))
                t[:k] *= F32(10.0 ** rng.uniform(-4, -0.5))   # a cluster whose own box may not overflow
                parts.append(t[rng.permutation(n)])
    t = np.concatenate(parts)
    order = np.arange(len(t), dtype=np.uint32)
    return t, order, [queries(t, order, nodes)]


def case_denormal():
    """Extents near 1e-20 (the products of the half area are denormal) and near 1e-38 (the extents are, the products are
    zero): the host keeps denormals."""
    rng = np.random.default_rng(1111)
    parts, nodes = [], []
    for n in (3, 100, 513, 1200):
        for spread, at in ((1e-20, 0.0), (1e-20, 1e-16), (3e-19, 0.0), (1e-38, 0.0), (3e-38, 1e-36), (1e-41, 0.0)):
            nodes.append((sum(len(p) for p in parts), n))
            P = (F32(at) + rng.uniform(-spread, spread, (n, 1, 3)) + rng.uniform(-spread / 8, spread / 8, (n, 3, 3)))
            parts.append(tri9_of(P))
    t = np.concatenate(parts)
    order = np.arange(len(t), dtype=np.uint32)
    return t, order, [queries(t, order, nodes)]


def case_non_finite():
    """+inf, -inf and NaN among the triangles' fields, with the box a builder would hold (the NaN-ignoring fold: non-finite
    where an infinity took part), with the box of the finite fields only, and with non-finite boxes given outright."""
    rng = np.random.default_rng(1212)
    parts, nodes, boxes = [], [], []
    special = np.array([np.inf, -np.inf, np.nan], F32)
    for n in (2, 3, 100, 513, 1200):
        for share in (0.002, 0.01, 0.05, 0.6):
            t = soup(rng, n)
            hit = rng.random(t.shape) < share
            hit[0, 0] = True
            fin = np.where(hit, np.nan, t)
            t = np.where(hit, special[rng.integers(0, 3, t.shape)], t).astype(F32)
            s = sum(len(p) for p in parts)
            parts.append(t)
            with np.errstate(all="ignore"):
                lo, hi = np.fmin.reduce(t[:, 3:6], 0), np.fmax.reduce(t[:, 6:9], 0)
                flo, fhi = np.fmin.reduce(fin[:, 3:6], 0).astype(F32), np.fmax.reduce(fin[:, 6:9], 0).astype(F32)
            flo, fhi = np.where(np.isnan(flo), F32(-1), flo), np.where(np.isnan(fhi), F32(1), fhi)
            for b in ((lo, hi), (flo, fhi)):
                nodes.append((s, n))
                boxes.append(b)
            for k in range(4):
                b = np.stack([flo, fhi]).astype(F32)
                b[rng.integers(0, 2), rng.integers(0, 3)] = special[(k + n) % 3]
                nodes.append((s, n))
                boxes.append((b[0], b[1]))
    t = np.concatenate(parts)
    order = np.arange(len(t), dtype=np.uint32)
    return t, order, [queries(t, order, nodes, boxes)]


CASES = {
    "sizes": case_sizes,
    "node_100k": lambda: case_big(100_000),
    "node_1m": lambda: case_big(1_048_576 + 300),
    "many_nodes": case_many_nodes,
    "levels": case_levels,
    "box_ratios": case_box_ratios,
    "flat": case_flat,
    "loose_boxes": case_loose_boxes,
    "on_the_plane": case_on_the_plane,
    "ties": case_ties,
    "signed_zeros": case_signed_zeros,
    "overflow": case_overflow,
    "denormal": case_denormal,
    "non_finite": case_non_finite,
}


# ---- whole builds ------------------------------------------------------------------------------------------------------
def mesh8(P):
    """(vertices8, indices) of triangles P [n, 3, 3], no vertex shared."""
    P = np.asarray(P, F32)
    v = np.concatenate([P.reshape(-1, 3), np.tile(np.array([0, 1, 0, 0, 0], F32), (3 * len(P), 1))], 1)
    return v, np.arange(3 * len(P), dtype=np.uint32)


def _soup_mesh(rng, n):
    return mesh8(rng.uniform(-1, 1, (n, 1, 3)) + rng.uniform(-0.2, 0.2, (n, 3, 3)))


def _grid_mesh(k):
    """k x k unit quads in the plane z = 1, two triangles each, shared vertices: rows and columns of equal centroids."""
    x, y = np.meshgrid(np.arange(k + 1, dtype=F32), np.arange(k + 1, dtype=F32), indexing="ij")
    v = np.concatenate([np.stack([x, y, np.ones_like(x)], -1).reshape(-1, 3),
                        np.tile(np.array([0, 0, 1, 0, 0], F32), ((k + 1) ** 2, 1))], 1)
    i, j = np.meshgrid(np.arange(k), np.arange(k), indexing="ij")
    a = (i * (k + 1) + j).reshape(-1)
    idx = np.stack([a, a + k + 1, a + 1, a + 1, a + k + 1, a + k + 2], -1).reshape(-1)
    return v, idx.astype(np.uint32)


def build_scenes():
    """{name: (meshes [(vertices8, indices, position)], min_triangles)} -- the whole builds of the issue."""
    rng = np.random.default_rng(77)
    one = _soup_mesh(rng, 700)
    nf = _soup_mesh(rng, 800)
    hit = rng.choice(nf[0].shape[0], 12, replace=False)
    nf[0][hit, rng.integers(0, 3, 12)] = np.array([np.inf, -np.inf, np.nan], F32)[np.arange(12) % 3]
    return {
        "exact_sizes": ([(*_soup_mesh(rng, n), (0, 0, 0)) for n in (2, 511, 512, 513, 1024, 1025)], 1),
        "grid": ([(*_grid_mesh(32), (0, 0, 0))], 1),
        "instanced_twice": ([(*one, (0, 0, 0)), (*one, (3, 1, -2))], 1),
        "threshold": ([(*_soup_mesh(rng, n), (0, 0, 0)) for n in (599, 600, 601, 598, 602)], 600),
        "non_finite_vertices": ([(*nf, (0, 0, 0))], 1),
    }


def make_scene(rt, meshes):
    from ray_tracer_2_amd.scene import transform
    sc = rt.Scene()
    for v, idx, pos in meshes:
        sc.add_mesh_from_data(v, idx, xform=transform(pos=pos))
    return sc


def built_bytes(rt, sc, **kw):
    sc.build(**kw)
    a = rt.SceneArrays.from_scene(sc)
    return a.nodes.tobytes(), a.triangles.tobytes(), a.meshes.tobytes()


def _same_values(a, b):
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def check_tree(arrays, i, order, P):
    """Validity of mesh i's tree, by rules that depend on no builder: `order` is a permutation and the packed triangles
    are P[order]; every interior node's children split its range in two, left part first, and the root holds all; every
    node box is the fold of the triangles under it (min / max that ignore NaN, from +-FLT_MAX; by value).  Level by
    level in numpy, so that the million-triangle tree passes through the same lines as a two-triangle one."""
    m = arrays.meshes[i]
    n, t0, n0 = int(m["triangles"]), int(m["triangle_offset"]), int(m["node_offset"])
    tris = arrays.triangles[t0:t0 + n]
    assert np.array_equal(np.sort(order), np.arange(n))
    for k, f in enumerate(("v1", "v2", "v3")):
        assert np.array_equal(bits(tris[f]), bits(P[order, k]))
    nodes = arrays.nodes[n0:]
    levels, seen = [np.array([0])], 1
    while True:
        cur = levels[-1]
        inner = cur[nodes["count"][cur] == 0]
        if inner.size == 0:
            break
        levels.append(np.concatenate([nodes["left"][inner], nodes["right"][inner]]).astype(np.int64))
        seen += levels[-1].size
        assert seen <= 2 * n
    reach = np.concatenate(levels)
    assert np.unique(reach).size == reach.size                      # a tree: no node reached twice
    N = int(reach.max()) + 1
    first, end = np.zeros(N, np.int64), np.zeros(N, np.int64)
    lo, hi = np.zeros((N, 3), F32), np.zeros((N, 3), F32)
    fmax = np.finfo(F32).max
    tmin = np.fmin(np.fmin(tris["v1"], tris["v2"]), tris["v3"])
    tmax = np.fmax(np.fmax(tris["v1"], tris["v2"]), tris["v3"])
    leaves = reach[nodes["count"][reach] > 0]
    leaves = leaves[np.argsort(nodes["first"][leaves], kind="stable")]
    first[leaves] = nodes["first"][leaves]
    end[leaves] = first[leaves] + nodes["count"][leaves]
    assert first[leaves[0]] == 0 and end[leaves[-1]] == n and np.array_equal(end[leaves[:-1]], first[leaves[1:]])
    lo[leaves] = np.fmin(np.fmin.reduceat(tmin, first[leaves], 0), F32(fmax))
    hi[leaves] = np.fmax(np.fmax.reduceat(tmax, first[leaves], 0), F32(-fmax))
    for cur in levels[::-1]:
        inner = cur[nodes["count"][cur] == 0]
        l, r = nodes["left"][inner].astype(np.int64), nodes["right"][inner].astype(np.int64)
        assert np.array_equal(end[l], first[r]) and np.all(first[l] < end[l]) and np.all(first[r] < end[r])
        first[inner], end[inner] = first[l], end[r]
        lo[inner], hi[inner] = np.fmin(lo[l], lo[r]), np.fmax(hi[l], hi[r])
    assert first[0] == 0 and end[0] == n
    assert _same_values(nodes["aabb_min"][reach], lo[reach]) and _same_values(nodes["aabb_max"][reach], hi[reach])
    return reach.size
