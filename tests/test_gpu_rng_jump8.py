"""The RNG jump of the terminal skip (rt_kernel.hip: lcg_jump / rng_jump<8> / path_terminal).

At a plain material a hit makes a fixed 8 draws -- is_spec, six of rand_unit_sphere, the roulette's own -- so the roulette
value of a segment is the generator's output of the state 8 LCG steps on, reached by one multiply-add before the segment
is traversed.  Function 20 of rt_test_device_units returns that output and that state for a state both ways -- by
jumping, and by calling next_random_number 8 times on the device -- and both must equal the generator restated in pure
Python integers (tests/test_oracle_golden.py: py_next_random_number), over 2^20 seeded states and the edge states.
"""
import numpy as np
import pytest

from test_gpu_rng_jump import EDGE_STATES, N, np_step
from test_oracle_golden import py_next_random_number

pytestmark = pytest.mark.gpu

FN_RNG_JUMP8 = 20
OUT8_JUMP, OUT8_STEP, STATE8_JUMP, STATE8_STEP = range(4)


@pytest.fixture(scope="module")
def tracer(rt):
    t = rt.RayTracer(device=0, max_width=64, max_height=64, lib=rt.load_test())
    yield t
    t.close()


def test_the_jump_equals_eight_steps_of_the_generator(tracer):
    states = np.concatenate([EDGE_STATES, np.random.RandomState(20261019).randint(0, 2 ** 32, size=N, dtype=np.uint64).astype(np.uint32)])
    s, o = states.astype(np.uint64), None
    for _ in range(8):
        s, o = np_step(s)
    # (the vectorised reference against the scalar one on the edge states and a few hundred of the seeded ones)
    for i in list(range(EDGE_STATES.size)) + list(range(EDGE_STATES.size, states.size, 4099)):
        ps, po = int(states[i]), 0
        for _ in range(8):
            ps, po = py_next_random_number(ps)
        assert (po, ps) == (int(o[i]), int(s[i])), hex(int(states[i]))
    want = {OUT8_JUMP: o, OUT8_STEP: o, STATE8_JUMP: s, STATE8_STEP: s}
    got = {w: tracer.device_units(FN_RNG_JUMP8, states, np.full(states.size, w, np.uint32)).view(np.uint32) for w in range(4)}
    assert np.array_equal(got[OUT8_JUMP], got[OUT8_STEP]) and np.array_equal(got[STATE8_JUMP], got[STATE8_STEP])
    for w in range(4):
        bad = np.flatnonzero(got[w] != want[w].astype(np.uint32))
        assert bad.size == 0, (w, bad.size, hex(int(states[bad[0]])))
