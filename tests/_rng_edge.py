"""The RNG of wgsl:195-200 run backwards: the states whose next draw is exactly 0.0 or rounds to 1.0 (shared by
tests/test_gpu_device_units.py and tests/_shade_cases.py)."""
import numpy as np

A_LCG, C_LCG, M_OUT = 747796405, 2891336453, 277803737   # wgsl:195-200


def state_before(output):
    """The RNG state s for which next_random_number(s) returns `output` (the generator is a
    permutation of u32: invert the two xorshifts, the odd multiplications and the LCG step)."""
    w = output ^ (output >> 22)
    x = (w * pow(M_OUT, -1, 2 ** 32)) % 2 ** 32
    k = (x >> 28) + 4                      # the top four bits pass through the xorshift unchanged
    s1, shift = x, k
    while shift < 32:                      # s1 = x ^ (s1 >> k)
        s1 = x ^ (s1 >> k)
        shift += k
    assert ((((s1 >> ((s1 >> 28) + 4)) ^ s1) * M_OUT) % 2 ** 32) == w
    return ((s1 - C_LCG) * pow(A_LCG, -1, 2 ** 32)) % 2 ** 32


def edge_states():
    """States whose next rand() is exactly 0.0 or rounds to 1.0 (r >= 0xffffff80)."""
    return np.array([state_before(0)] + [state_before(r) for r in range(0xffffff80, 0x100000000)], np.uint32)
