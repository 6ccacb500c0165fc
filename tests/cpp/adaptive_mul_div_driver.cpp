// adaptive_mul_div_driver.cpp -- rtad::mul_div_floor of csrc/rt_adaptive.h (the exact floor(a b / d) of the adaptive plan's
// apportionment) against unsigned __int128, on edge operands and on random ones of every size for which the quotient fits 64
// bits (tests/test_adaptive_host.py builds and runs it, with the sanitizers).
#include <cstdint>
#include <cstdio>

#include "../../ray_tracer_2_amd/csrc/rt_adaptive.h"

static uint64_t state = 0x9e3779b97f4a7c15ull;
static uint64_t next() {   // splitmix64
    uint64_t z = (state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

static long checked = 0;
static int check(uint64_t a, uint64_t b, uint64_t d) {
    const unsigned __int128 want = (unsigned __int128)a * b / d;
    if (want >> 64) return 0;   // (outside the function's contract)
    ++checked;
    const uint64_t got = rtad::mul_div_floor(a, b, d);
    if (got == (uint64_t)want) return 0;
    std::printf("mul_div_floor(%llu, %llu, %llu) = %llu, not %llu\n", (unsigned long long)a, (unsigned long long)b, (unsigned long long)d,
                (unsigned long long)got, (unsigned long long)(uint64_t)want);
    return 1;
}

int main() {
    int bad = 0;
    // the edges of the plan's own range: c in 0 .. S < 2^51, R < 2^31
    const uint64_t edge[] = {0u, 1u, 2u, 3u, (1ull << 20), (1ull << 31) - 1u, (1ull << 31), (1ull << 32) - 1u, (1ull << 32), (1ull << 51) - 1u,
                             (1ull << 51), (1ull << 63) - 1u, (1ull << 63), ~0ull - 1u, ~0ull};
    for (uint64_t a : edge)
        for (uint64_t b : edge)
            for (uint64_t d : edge)
                if (d != 0u) bad += check(a, b, d);
    for (uint64_t S : edge)
        if (S != 0u)
            for (uint64_t R : edge) bad += check(S, R, S);   // c = S: the quotient is R itself
    // random operands of random widths; then the plan's shape: c <= S < 2^51, R < 2^31
    for (int i = 0; i < 2000000; ++i) {
        const uint64_t a = next() >> (next() & 63u), b = next() >> (next() & 63u), d = next() >> (next() & 63u);
        if (d != 0u) bad += check(a, b, d);
    }
    for (int i = 0; i < 1000000; ++i) {
        const uint64_t S = (next() >> 13) >> (next() % 40u);
        if (S == 0u) continue;
        const uint64_t c = next() % (S + 1u), R = next() >> 33;
        bad += check(c, R, S);
        bad += check(S, R, S);
    }
    if (bad != 0 || checked < 2000000) {
        std::printf("%d wrong of %ld\n", bad, checked);
        return 1;
    }
    std::printf("mul_div_floor ok: %ld cases\n", checked);
    return 0;
}
