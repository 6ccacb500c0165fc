"""The oracle's shading step (oracle.shade: shade_segment of shader_oracle.cpp, the body of trace's loop, with path_end's
bookkeeping) against the float64 restatement (independent_f64.scatter), one hit at a time, on the case families of
tests/_shade_cases.py.  No GPU.

Off the cases scatter calls ambiguous (a decision within binary32's rounding of its threshold, or an ill-conditioned
output), the integer outputs are equal -- RNG state, seg, j, fresh ("the path ended"), the return value ("the pixel is
done"), the segment count and meta -- and the float outputs agree within the pin of tests/test_f64_pin.py,
|a - b| <= 1e-5 max(|b|, 1e-3), per value; an output that is not finite on one side is not finite on the other.  The one
exception is the new direction rd, where |b| is the vector's largest component (tests/_shade_cases.py: compare says why).

The share of ambiguous cases is capped at 2 % of the random family and of each of its materials; the families built to sit
on a threshold (critical, edge_draws, incidence) are exempt and their counts printed.
"""
import numpy as np
import pytest

import _shade_cases as SC
from oracle import independent_f64 as F

CAP = 0.02
EXEMPT = ("critical", "edge_draws", "incidence")


@pytest.fixture(scope="module", params=["plain", "general"])
def pal(request):
    arrays, names = SC.palette(request.param)
    return request.param, arrays, names, F.Scene(arrays), SC.families(request.param)


def test_oracle_shade_agrees_with_the_f64_scatter_off_the_ambiguous_cases(oracle, pal):
    which, arrays, names, fscene, fams = pal
    lines = []
    for fam, batches in fams.items():
        n = n_amb = 0
        for b in batches:
            got = oracle.shade(arrays, b["cases"], b["nb"], b["rpp"], b["skybox"])
            bad, amb = SC.compare(fscene, got, b["cases"], b["nb"], b["rpp"], b["skybox"])
            assert not bad, (which, fam, {k: (v.size, v[:3].tolist(), [names[int(o)] for o in b["cases"][v[:3], SC.C_OBJ]]) for k, v in bad.items()})
            n += len(amb)
            n_amb += int(amb.sum())
            if fam == "random":
                assert amb.mean() <= CAP, (which, amb.mean())
                obj = b["cases"][:, SC.C_OBJ]
                share = np.array([amb[obj == o].mean() for o in range(len(names))])
                lines.append(f"  worst material {names[int(share.argmax())]} {share.max():.4f}")
                assert share.max() <= CAP, (which, dict(zip(names, share.round(4))))
        lines.append(f"{which} {fam}: {n} cases, {n_amb} ambiguous" + ("" if fam not in EXEMPT else " (exempt from the cap)"))
    print("\n" + "\n".join(lines))


def test_the_references_glue_is_the_oracles_on_plain_numbers(oracle):
    """A directed handful where nothing is close to anything: a survivor, a death, a miss and STEP_END give the bookkeeping
    words by hand."""
    arrays, names = SC.palette("plain")
    one, zero = names.index("one"), names.index("zero")
    c = np.concatenate([SC.make(1, obj=one, seg=1, j=2, meta=7),                       # p = 1: survives, seg 2 <= 4
                        SC.make(1, obj=one, seg=4, j=3, meta=0xffff),                  # survives and still ends: seg 5 > 4; the pixel is done
                        SC.make(1, obj=zero, seg=0, j=0, meta=0xfffe, total=(1, 2, 3, 4), light=(1, 1, 1, 1)),   # p = 0: dies
                        SC.make(1, hit=0, j=3, light=(0.5, 0.5, 0.5, 0)),              # a miss ends the path
                        SC.make(1, mode=SC.STEP_END, seg=5, j=1, total=(1, 1, 1, 1), light=(2, 2, 2, 2))])
    r = oracle.shade(arrays, c, 4, 4, 0)
    assert r[:, SC.R_SEG].tolist() == [2, 5, 0, 0, 5]
    assert r[:, SC.R_J].tolist() == [2, 4, 1, 4, 2]
    assert r[:, SC.R_FRESH].tolist() == [0, 1, 1, 1, 1]
    assert r[:, SC.R_RET].tolist() == [0, 1, 0, 1, 0]
    assert r[:, SC.R_NSEG].tolist() == [1, 1, 1, 1, 0]
    assert r[:, SC.R_META].tolist() == [8, 0xffff, 0xffff, 1, 0]
    assert SC.as_f64(r[2, 14:18]).tolist() == [2, 3, 4, 5] and SC.as_f64(r[4, 14:18]).tolist() == [3, 3, 3, 3]
    assert SC.as_f64(r[3, 14:18]).tolist() == [0.5, 0.5, 0.5, 0]   # skybox 0: the miss adds the light it carried
    assert r[0, SC.R_RNG] == SC.step_forward([1], 8)[0] and r[3, SC.R_RNG] == 1 and r[4, SC.R_RNG] == 1


def test_roulette_stepping_counts_the_deaths_it_can_predict(oracle):
    """roulette_expected on materials whose fate is certain: `zero` (p = 0) dies every sample, `one` (p = 1, T = 1) never
    dies unless the roulette draw rounds to 1.0."""
    arrays, names = SC.palette("plain")
    c = SC.cross(SC.make(2, obj=[names.index("zero"), names.index("one")]), SC.make(3, rng=[5, 77, 12345]), SC.make(1, meta=0xfffe))
    e = SC.roulette_expected(oracle, arrays, c, 8)
    assert e[:3, 9].tolist() == [8, 8, 8] and e[:3, 6].tolist() == [1, 1, 1] and e[:3, 5].tolist() == [8, 8, 8]
    assert e[:3, 4].tolist() == SC.step_forward([5, 77, 12345], 96).tolist() and e[:3, 8].tolist() == [0xffff] * 3
    assert not e[3:, 9].any() and e[3:, 4].tolist() == [5, 77, 12345] and e[3:, 8].tolist() == [0xfffe] * 3
