// rectify_driver.cpp -- rt_temporal_rectify_host's restatement (csrc/host/rectify.cpp: rt2::rectify_host) as a program of
// its own, for AddressSanitizer and UndefinedBehaviorSanitizer on the CPU (tests/test_rectify_host.py builds and runs it):
//   rectify_driver OUT
// Frames of 1x1, 7x5 and 40x9 on exactly sized heap buffers, at every radius, with the object plane, the moments and
// out_clipped on and off, and with the outputs in the places of the history planes: a read or write outside a plane is the
// sanitizer's to find.  The frames are ramp(i) below with a NaN, an infinity and a short history among them.  OUT receives
// the 7x5 frame's outputs at radius 2 with every plane: out, out_history, out_moments, out_clipped.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>

#include "../../ray_tracer_2_amd/csrc/rt_rectify_api.h"

namespace {

float ramp(size_t i, float lo, float span) { return lo + span * (float)((i * 37u) % 101u) / 101.0f; }

struct Frame {
    uint32_t w, h;
    size_t n;
    std::unique_ptr<float[]> color, history, length, moments, hmoments, out, out_history, out_moments;
    std::unique_ptr<uint32_t[]> object;
    std::unique_ptr<uint8_t[]> clipped;
    Frame(uint32_t w_, uint32_t h_) : w(w_), h(h_), n((size_t)w_ * h_) {
        color.reset(new float[4 * n]); history.reset(new float[4 * n]); length.reset(new float[n]);
        moments.reset(new float[4 * n]); hmoments.reset(new float[4 * n]); out.reset(new float[4 * n]);
        out_history.reset(new float[n]); out_moments.reset(new float[4 * n]); object.reset(new uint32_t[n]); clipped.reset(new uint8_t[n]);
        fill();
    }
    void fill() {
        for (size_t i = 0; i < 4 * n; ++i) {
            color[i] = ramp(i, 0.2f, 0.8f);
            history[i] = ramp(i + 13, 0.3f, 0.6f);
            moments[i] = ramp(i + 5, 0.0f, 2.0f);
            hmoments[i] = ramp(i + 29, 0.0f, 2.0f);
        }
        for (size_t i = 0; i < n; ++i) {
            length[i] = (float)(1 + i % 9);
            object[i] = (uint32_t)((i / 3) % 2);
        }
        if (n > 6) {
            color[4 * 2 + 1] = NAN;
            color[4 * 5 + 3] = INFINITY;
            history[4 * 3] = NAN;
            length[4] = 0.5f;
            hmoments[4 * 6 + 2] = INFINITY;
        }
    }
};

bool run(Frame& f, uint32_t radius, bool object, bool moments, bool clipped, bool in_place) {
    f.fill();
    rt_rectify_desc d{};
    d.struct_bytes = sizeof(d);
    d.width = f.w; d.height = f.h; d.radius = radius;
    d.clip_sigma = 1.0f; d.clip_history = 4.0f;
    d.color = f.color.get(); d.history = f.history.get(); d.history_length = f.length.get();
    d.object = object ? f.object.get() : nullptr;
    d.out = in_place ? f.history.get() : f.out.get();
    d.out_history = in_place ? f.length.get() : f.out_history.get();
    if (moments) {
        d.moments = f.moments.get(); d.history_moments = f.hmoments.get();
        d.out_moments = in_place ? f.hmoments.get() : f.out_moments.get();
    }
    d.out_clipped = clipped ? f.clipped.get() : nullptr;
    std::string err;
    const int rc = rt2::rectify_host(&d, err);
    if (rc != RT_OK) fprintf(stderr, "rectify_host: %d %s\n", rc, err.c_str());
    return rc == RT_OK;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: rectify_driver OUT\n");
        return 2;
    }
    const uint32_t sizes[3][2] = {{1, 1}, {7, 5}, {40, 9}};
    for (const auto& s : sizes) {
        Frame f(s[0], s[1]);
        for (uint32_t radius = 1; radius <= 3; ++radius)
            for (int bits = 0; bits < 16; ++bits)
                if (!run(f, radius, bits & 1, bits & 2, bits & 4, bits & 8)) return 1;
        printf("%ux%u ok\n", s[0], s[1]);
    }
    // an argument error writes nothing and reads nothing
    rt_rectify_desc bad{};
    bad.struct_bytes = sizeof(bad);
    std::string err;
    if (rt2::rectify_host(&bad, err) != RT_ERR_INVALID_ARGUMENT || rt2::rectify_host(nullptr, err) != RT_ERR_INVALID_ARGUMENT) return 1;
    Frame f(7, 5);
    if (!run(f, 2, true, true, true, false)) return 1;
    FILE* o = fopen(argv[1], "wb");
    if (!o) return 1;
    fwrite(f.out.get(), 4, 4 * f.n, o);
    fwrite(f.out_history.get(), 4, f.n, o);
    fwrite(f.out_moments.get(), 4, 4 * f.n, o);
    fwrite(f.clipped.get(), 1, f.n, o);
    fclose(o);
    printf("written\n");
    return 0;
}
