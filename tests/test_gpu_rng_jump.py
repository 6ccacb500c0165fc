"""The RNG jumps of the roulette skip (rt_kernel.hip: lcg_jump / rng_jump / rng_output).

The skip reads a sample's is_spec and roulette values without making the draws between them: the generator's output of
the state 5 and 12 LCG steps on, each reached by one multiply-add.  Function 19 of rt_test_device_units returns those
values for a state both ways -- by jumping, and by calling next_random_number 12 times -- and both must equal the
generator restated in pure Python integers (tests/test_oracle_golden.py: py_next_random_number).
"""
import numpy as np
import pytest

from test_oracle_golden import py_next_random_number

pytestmark = pytest.mark.gpu

FN_RNG_JUMP = 19
OUT5_JUMP, OUT5_STEP, OUT12_JUMP, OUT12_STEP, STATE12_JUMP, STATE12_STEP = range(6)
EDGE_STATES = np.array([0, 1, 0x7fffffff, 0x80000000, 0xffffffff], np.uint32)
N = 1 << 20


def np_step(s):
    """py_next_random_number over an array of states (uint64 arithmetic masked to 32 bits): (new state, output)"""
    s = (s * np.uint64(747796405) + np.uint64(2891336453)) & np.uint64(0xFFFFFFFF)
    r = (((s >> ((s >> np.uint64(28)) + np.uint64(4))) ^ s) * np.uint64(277803737)) & np.uint64(0xFFFFFFFF)
    return s, ((r >> np.uint64(22)) ^ r) & np.uint64(0xFFFFFFFF)


@pytest.fixture(scope="module")
def tracer(rt):
    t = rt.RayTracer(device=0, max_width=64, max_height=64, lib=rt.load_test())
    yield t
    t.close()


def test_jumps_equal_twelve_steps_of_the_generator(tracer):
    states = np.concatenate([EDGE_STATES, np.random.RandomState(20261017).randint(0, 2 ** 32, size=N, dtype=np.uint64).astype(np.uint32)])
    # the reference: twelve steps of the pure-Python generator -- vectorised, and the vectorised form checked against the
    # scalar one on the edge states and a few hundred of the seeded ones
    s, out = states.astype(np.uint64), {}
    for k in range(1, 13):
        s, o = np_step(s)
        out[k] = o
    want = {OUT5_JUMP: out[5], OUT5_STEP: out[5], OUT12_JUMP: out[12], OUT12_STEP: out[12], STATE12_JUMP: s, STATE12_STEP: s}
    for i in list(range(EDGE_STATES.size)) + list(range(EDGE_STATES.size, states.size, 4099)):
        ps, po = int(states[i]), []
        for _ in range(12):
            ps, o = py_next_random_number(ps)
            po.append(o)
        assert (po[4], po[11], ps) == (int(out[5][i]), int(out[12][i]), int(s[i])), hex(int(states[i]))
    got = {}
    for which in range(6):
        got[which] = tracer.device_units(FN_RNG_JUMP, states, np.full(states.size, which, np.uint32)).view(np.uint32)
    for jump, step in ((OUT5_JUMP, OUT5_STEP), (OUT12_JUMP, OUT12_STEP), (STATE12_JUMP, STATE12_STEP)):
        assert np.array_equal(got[jump], got[step]), (jump, step)
    for which in range(6):
        bad = np.flatnonzero(got[which] != want[which].astype(np.uint32))
        assert bad.size == 0, (which, bad.size, hex(int(states[bad[0]])))
