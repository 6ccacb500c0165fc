"""A plain numpy restatement of the reference builder's SAH plane search for one BVH node: `find_best_split` with
Quality::High (src/core/bvh.rs:299-351), its `evaluate_sah` (:352-370) and `Aabb::half_area` (:87-90).

It shares nothing with ray_tracer_2_amd/csrc/host/bvh.cpp, csrc/rt_bvh_search.hip or oracle/host_oracle.py; the tests
compare those with it.  Every binary32 operation is one numpy float32 operation, in the reference's order:

* bounds = aabb_max - aabb_min; max_axis = bounds[0].max(bounds[1].max(bounds[2])) (:312, :325; f32::max ignores NaN);
* an axis of size == 0.0 is skipped (:329-331);
* n_split_tests = ceil(axis_size / max_axis * 50) `as u32` -- the cast saturates and sends NaN to 0 --, clamped to
  1..50 (:332-334); counts are integers;
* plane i: split_t = (i + 1) as f32 / (n as f32 + 1.0); pos = axis_min + axis_size * split_t (:337-338);
* a triangle is on the left when centroid[axis] < pos, strictly (:360);
* the side boxes are min / max folds from +inf / -inf (:92-99, :83-86).  f32::min / f32::max ignore a NaN operand, so
  the folds are np.fmin / np.fmax reductions: exact in any order, apart from the sign of a zero;
* half_area = (ex * ey + ey * ez) + ex * ez (:88-89); cost = nl * lha + nr * rha (:368) -- an empty side gives
  0 * inf = NaN, which never wins;
* the candidates are taken axis by axis, plane by plane, and `cost < best_cost` is strict (:340-344): of equal costs the
  first wins; with no winner the result is (+inf, axis 0, position 0.0) (:308-310 initial values in subdivide :382-383).

`find_best_split` prices the nodes of one call together when they have the same triangle count (the arrays are
[node, candidate, triangle]), in slices of at most ELEMENTS elements, so that a level of 70,000 tiny nodes and one node
of a million triangles both go through the same lines.
"""
import numpy as np

F32 = np.float32
TEST_SPLITS = 50   # BVH::TEST_SPLITS
ELEMENTS = 1 << 22


def n_split_tests(aabb_min, aabb_max):
    """[Q, 3] integer plane counts (0 for a skipped axis) of boxes [Q, 3]."""
    with np.errstate(all="ignore"):
        mn, mx = np.asarray(aabb_min, F32).reshape(-1, 3), np.asarray(aabb_max, F32).reshape(-1, 3)
        bounds = (mx - mn).astype(F32)
        max_axis = np.fmax(bounds[:, 0], np.fmax(bounds[:, 1], bounds[:, 2])).astype(F32)
        ratio = ((bounds / max_axis[:, None]).astype(F32) * F32(TEST_SPLITS)).astype(F32)
        c = np.ceil(ratio).astype(np.float64)
        as_u32 = np.where(np.isnan(c) | (c <= 0), 0.0, np.where(c >= 4294967296.0, 4294967295.0, c)).astype(np.int64)
        n = np.clip(as_u32, 1, TEST_SPLITS)
        return np.where(bounds == 0, 0, n)


def candidates(aabb_min, aabb_max):
    """(pos [Q, 150] f32, valid [Q, 150] bool): candidate t = axis * 50 + plane, the reference's order."""
    with np.errstate(all="ignore"):
        mn, mx = np.asarray(aabb_min, F32).reshape(-1, 3), np.asarray(aabb_max, F32).reshape(-1, 3)
        bounds = (mx - mn).astype(F32)
        n = n_split_tests(mn, mx)                                        # [Q, 3]
        i = np.arange(TEST_SPLITS)
        valid = i[None, None, :] < n[:, :, None]                         # [Q, 3, 50]
        num = (i + 1).astype(F32)[None, None, :]
        den = (n.astype(F32) + F32(1.0)).astype(F32)[:, :, None]
        split_t = (num / den).astype(F32)
        pos = (mn[:, :, None] + (bounds[:, :, None] * split_t).astype(F32)).astype(F32)
        return pos.reshape(-1, 3 * TEST_SPLITS), valid.reshape(-1, 3 * TEST_SPLITS)


def _half_area(mn, mx):
    e = (mx - mn).astype(F32)
    ex, ey, ez = e[..., 0], e[..., 1], e[..., 2]
    return (((ex * ey).astype(F32) + (ey * ez).astype(F32)).astype(F32) + (ex * ez).astype(F32)).astype(F32)


def _costs(tri, pos, axes):
    """evaluate_sah: tri [Q, n, 9], pos [Q, T], axes [T] -> cost [Q, T] f32."""
    cent = tri[:, :, :3][:, :, axes].transpose(0, 2, 1)                  # [Q, T, n]
    left = cent < pos[:, :, None]
    nl = left.sum(-1)
    nr = tri.shape[1] - nl
    box = {}
    for side, mask in (("l", left), ("r", ~left)):
        mn = np.stack([np.fmin.reduce(np.where(mask, tri[:, None, :, 3 + d], F32(np.inf)), axis=-1, initial=F32(np.inf))
                       for d in range(3)], -1)
        mx = np.stack([np.fmax.reduce(np.where(mask, tri[:, None, :, 6 + d], F32(-np.inf)), axis=-1, initial=F32(-np.inf))
                       for d in range(3)], -1)
        box[side] = _half_area(mn.astype(F32), mx.astype(F32))
    return ((nl.astype(F32) * box["l"]).astype(F32) + (nr.astype(F32) * box["r"]).astype(F32)).astype(F32)


def find_best_split(tri9, order, starts, count, aabb_min, aabb_max):
    """The nodes [starts[q], starts[q] + count) of `order` with boxes aabb_min/max [Q, 3]:
    (axis [Q] int32, pos [Q] f32, cost [Q] f32)."""
    tri9 = np.asarray(tri9, F32).reshape(-1, 9)
    order = np.asarray(order).astype(np.int64)
    starts = np.asarray(starts, np.int64).reshape(-1)
    count = int(count)
    assert count >= 2
    Q = len(starts)
    pos, valid = candidates(aabb_min, aabb_max)
    T = 3 * TEST_SPLITS
    cost = np.full((Q, T), np.inf, F32)
    t_step = max(1, min(T, ELEMENTS // count))
    q_step = max(1, ELEMENTS // (count * t_step))
    axes_all = np.arange(T) // TEST_SPLITS
    with np.errstate(all="ignore"):
        for q0 in range(0, Q, q_step):
            q1 = min(Q, q0 + q_step)
            tri = tri9[order[starts[q0:q1, None] + np.arange(count)[None, :]]]          # [q, n, 9]
            for t0 in range(0, T, t_step):
                t1 = min(T, t0 + t_step)
                if valid[q0:q1, t0:t1].any():
                    cost[q0:q1, t0:t1] = _costs(tri, pos[q0:q1, t0:t1], axes_all[t0:t1])
    # the reference's loop over the candidates, all nodes at once
    best = np.full(Q, np.inf, F32)
    axis = np.zeros(Q, np.int32)
    split = np.zeros(Q, F32)
    for t in range(T):
        take = valid[:, t] & (cost[:, t] < best)
        best = np.where(take, cost[:, t], best)
        axis = np.where(take, np.int32(t // TEST_SPLITS), axis)
        split = np.where(take, pos[:, t], split)
    return axis.astype(np.int32), split.astype(F32), best.astype(F32)
