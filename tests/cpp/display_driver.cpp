// display_driver.cpp -- rt_display_host's and rt_auto_exposure_host's restatements (csrc/host/display.cpp:
// rt2::display_host, rt2::auto_exposure_host) under AddressSanitizer and UndefinedBehaviorSanitizer, as a program of its own
// (tests/test_display_host.py builds and runs it; it is never loaded into Python).
//
//   display_driver OUT
//
// Both functions at 1 x 1, 7 x 3 and 257 x 5 on the frame ramp(i) = 2^(i % 40 - 20) * (1 + (i % 7) / 8) over its floats,
// every array in a heap block of exactly its size, so that a read or write one element outside it is reported, with every
// optional pointer (exposure_scale; prev_scale, histogram) on and off and every tone, transfer and layout.  OUT receives the
// 7 x 3 case's picture (REINHARD, white 4, layout 3, exposure 1.5, the meter's scale), the scale and the histogram.
// Then display_host's byte over EVERY float of [0, 1], a million texels a call, the range cut into pieces for up to eight
// threads (each piece starts at the float the one before it ends at): it never decreases, steps 255 times, and the float at
// step k is T[k] of rt_srgb_encode_lut.h.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "../../ray_tracer_2_amd/csrc/rt_display_api.h"

namespace {

const float TABLE[] = {RT_SRGB_ENCODE_T_VALUES};

int fail(const char* what, const std::string& err) {
    fprintf(stderr, "%s: %s\n", what, err.c_str());
    return 1;
}

rt_display_desc display_desc(uint32_t w, uint32_t h, const float* color, uint8_t* out) {
    rt_display_desc d{};
    d.struct_bytes = sizeof(d);
    d.width = w;
    d.height = h;
    d.exposure = 1.0f;
    d.white = 4.0f;
    d.color = color;
    d.out = out;
    return d;
}

int one_size(uint32_t w, uint32_t h, FILE* out_file) {
    const size_t n = (size_t)w * h;
    std::unique_ptr<float[]> color(new float[4 * n]);
    for (size_t i = 0; i < 4 * n; ++i) color[i] = std::ldexp(1.0f + (float)(i % 7) / 8.0f, (int)(i % 40) - 20);
    std::unique_ptr<uint8_t[]> bytes(new uint8_t[4 * n]);
    std::unique_ptr<uint32_t[]> histogram(new uint32_t[256]);
    std::unique_ptr<float[]> scale(new float[1]), prev(new float[1]);
    std::string err;

    rt_auto_exposure_desc m{};
    m.struct_bytes = sizeof(m);
    m.width = w;
    m.height = h;
    m.low_permille = 100;
    m.high_permille = 900;
    m.key = 0.18f;
    m.min_scale = 0x1p-8f;
    m.max_scale = 0x1p8f;
    m.rate = 0.25f;
    m.color = color.get();
    m.scale = scale.get();
    prev[0] = 2.0f;
    for (int with_prev = 1; with_prev >= 0; --with_prev)
        for (int with_histogram = 0; with_histogram < 2; ++with_histogram) {
            m.prev_scale = with_prev ? prev.get() : nullptr;
            m.histogram = with_histogram ? histogram.get() : nullptr;
            if (rt2::auto_exposure_host(&m, err) != RT_OK) return fail("auto_exposure_host", err);
            if (!(scale[0] >= m.min_scale && scale[0] <= m.max_scale)) return fail("auto_exposure_host", "scale outside its clamps");
        }
    // (the last call: no prev_scale, with the histogram)
    uint64_t counted = 0;
    for (int b = 0; b < 256; ++b) counted += histogram[b];
    if (counted != n) return fail("auto_exposure_host", "the histogram does not sum to the texels");

    for (uint32_t tone = 0; tone < 2; ++tone)
        for (uint32_t transfer = 0; transfer < 2; ++transfer)
            for (uint32_t layout = 0; layout < 4; ++layout)
                for (int with_scale = 0; with_scale < 2; ++with_scale) {
                    rt_display_desc d = display_desc(w, h, color.get(), bytes.get());
                    d.tone = tone;
                    d.transfer = transfer;
                    d.layout = layout;
                    d.exposure = 1.5f;
                    d.exposure_scale = with_scale ? scale.get() : nullptr;
                    if (rt2::display_host(&d, err) != RT_OK) return fail("display_host", err);
                }
    // (the last call: REINHARD, LINEAR, layout 3, with the scale) -- the picture the test compares is the sRGB one
    rt_display_desc d = display_desc(w, h, color.get(), bytes.get());
    d.tone = RT_DISPLAY_TONE_REINHARD;
    d.layout = 3;
    d.exposure = 1.5f;
    d.exposure_scale = scale.get();
    if (rt2::display_host(&d, err) != RT_OK) return fail("display_host", err);
    if (out_file) {
        fwrite(bytes.get(), 1, 4 * n, out_file);
        fwrite(scale.get(), sizeof(float), 1, out_file);
        fwrite(histogram.get(), sizeof(uint32_t), 256, out_file);
    }
    printf("%ux%u ok\n", w, h);
    return 0;
}

// The floats with bits FIRST .. LAST: the steps among them are counted into `steps` (the byte of FIRST is where the piece
// starts from, and is returned in `first_byte`, the byte of LAST in `last_byte`).
int sweep_piece(uint32_t FIRST, uint32_t LAST, uint32_t* steps_out, uint32_t* first_byte, uint32_t* last_byte) {
    const uint32_t CHUNK = 1u << 20;
    std::unique_ptr<float[]> color(new float[4 * (size_t)CHUNK]);
    std::unique_ptr<uint8_t[]> bytes(new uint8_t[4 * (size_t)CHUNK]);
    std::string err;
    uint32_t bits = FIRST, previous = 0, steps = 0;
    bool started = false;
    while (bits <= LAST) {
        // three floats a texel, in the colour channels; alpha 1
        const uint64_t left = (uint64_t)LAST - bits + 1u;
        const uint32_t texels = (uint32_t)((left + 2u) / 3u < CHUNK ? (left + 2u) / 3u : CHUNK);
        for (uint32_t p = 0; p < texels; ++p) {
            for (uint32_t k = 0; k < 3; ++k) {
                const uint64_t b = (uint64_t)bits + 3u * p + k;
                const uint32_t u = (uint32_t)(b <= LAST ? b : LAST);
                std::memcpy(&color[4 * (size_t)p + k], &u, sizeof(u));
            }
            color[4 * (size_t)p + 3] = 1.0f;
        }
        rt_display_desc d = display_desc(texels, 1, color.get(), bytes.get());
        if (rt2::display_host(&d, err) != RT_OK) return fail("display_host", err);
        for (uint32_t p = 0; p < texels; ++p)
            for (uint32_t k = 0; k < 3; ++k) {
                const uint32_t byte = bytes[4 * (size_t)p + k];
                if (!started) {
                    started = true;
                    *first_byte = previous = byte;
                }
                if (byte == previous) continue;
                float x;
                std::memcpy(&x, &color[4 * (size_t)p + k], sizeof(x));
                if (byte != previous + 1u || x != TABLE[byte]) {
                    fprintf(stderr, "sweep: byte %u after %u at %a (T[%u] = %a)\n", byte, previous, x, byte, byte < 256 ? TABLE[byte] : 0.0f);
                    return 1;
                }
                previous = byte;
                steps += 1;
            }
        if ((uint64_t)bits + 3ull * texels > LAST) break;
        bits += 3u * texels;
    }
    *steps_out = steps;
    *last_byte = previous;
    return 0;
}

int sweep() {
    const uint32_t LAST = 0x3f800000u;   // (bits of 1.0f)
    const uint32_t hw = std::thread::hardware_concurrency();
    const uint32_t pieces = hw < 1u ? 1u : hw > 8u ? 8u : hw;
    std::vector<uint32_t> steps(pieces, 0u), first(pieces, 0u), last(pieces, 0u);
    std::vector<int> rc(pieces, 0);
    std::vector<std::thread> threads;
    for (uint32_t i = 0; i < pieces; ++i) {
        const uint32_t a = (uint32_t)((uint64_t)LAST * i / pieces), b = (uint32_t)((uint64_t)LAST * (i + 1u) / pieces);
        threads.emplace_back([&, i, a, b] { rc[i] = sweep_piece(a, b, &steps[i], &first[i], &last[i]); });
    }
    for (std::thread& t : threads) t.join();
    uint32_t total = 0;
    for (uint32_t i = 0; i < pieces; ++i) {
        if (rc[i] != 0) return rc[i];
        if (i > 0u && first[i] != last[i - 1u]) return fail("sweep", "the pieces do not meet");
        total += steps[i];
    }
    if (total != 255u || first[0] != 0u || last[pieces - 1u] != 255u) return fail("sweep", "not 255 steps from 0 to 255");
    printf("sweep ok: %u steps\n", total);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: display_driver OUT\n");
        return 2;
    }
    FILE* f = fopen(argv[1], "wb");
    if (!f) return fail("fopen", argv[1]);
    int rc = one_size(1, 1, nullptr);
    if (rc == 0) rc = one_size(7, 3, f);
    if (rc == 0) rc = one_size(257, 5, nullptr);
    fclose(f);
    if (rc == 0) rc = sweep();
    return rc;
}
