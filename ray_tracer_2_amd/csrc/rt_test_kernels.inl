// rt_test_kernels.inl -- TEST LIBRARY ONLY (-DRT_TEST_ENTRIES=1; included by rt_kernel.hip inside namespace rtd): the kernels
// behind include/rt_test_abi.h with their launchers.
// ---------------------------------------------------------------------------
// Test-only: the device's evaluation of the implementation-defined builtins (rt_transc.h), IEEE
// division / sqrt, the RNG and the texture filter, one element per thread, so that
// tests/test_gpu_device_units.py can compare them bit for bit with the host compile of the same
// headers (the oracle) -- including the edge values whole-image parity tests almost never reach
// (rand() == 0 -> log(0), rand() == 1, trig sign bits at exact zeros, subnormals, inf, NaN).
// fn: 0 log, 1 cos, 2 sin, 3 exp, 4 exp2, 5 log2, 6 pow(x, y), 7 acos, 8 atan2(x, y), 9 sqrt, 10 x / y
// (the oracle's numbering), 11 rand() of RNG state bits x -> float, 12 the generator's u32 output for
// state x, 13 trig_signbits(x), 14 rand_normal_dist() of state x, 15 f32(u32 x) * 2^-32 (rand()'s
// conversion for a raw generator output), 16 normalize(x, y, x*y).x (division by a sqrt), 17 rcp_(x), 18 sqrt_dev(x),
// 19 the roulette skip's RNG jumps for state x, y (bits) selecting: 0 / 1 the generator's output 5 steps on by jumping /
// by stepping, 2 / 3 the output 12 steps on, 4 / 5 the state 12 steps on
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) rt_units_kernel(int fn, const float* __restrict__ x, const float* __restrict__ y,
                                                       float* __restrict__ out, unsigned long long n) {
    const unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float a = x[i], b = y[i];
    float r = 0.0f;
    switch (fn) {
        case 0: r = rtm::log_(a); break;
        case 1: r = rtm::cos_(a); break;
        case 2: r = rtm::sin_(a); break;
        case 3: r = rtm::exp_(a); break;
        case 4: r = rtm::exp2_(a); break;
        case 5: r = rtm::log2_(a); break;
        case 6: r = rtm::pow_(a, b); break;
        case 7: r = rtm::acos_(a); break;
        case 8: r = rtm::atan2_(a, b); break;
        case 9: r = rtm::sqrt_(a); break;
        case 10: r = a / b; break;
        case 11: { uint32_t s = __float_as_uint(a); r = rand_(s); break; }
        case 12: { uint32_t s = __float_as_uint(a); r = __uint_as_float(next_random_number(s)); break; }
        case 13: r = __uint_as_float(rtm::trig_signbits(a)); break;
        case 14: { uint32_t s = __float_as_uint(a); r = rand_normal_dist(s); break; }
        case 15: r = (float)__float_as_uint(a) * 0x1p-32f; break;
        case 16: r = normalize3(f3{a, b, a * b}).x; break;
        case 17: r = rcp_(a); break;
        case 18: r = sqrt_dev(a); break;
        case 19: {  // the roulette skip's jumps against the generator stepped 12 times; y (bits) selects the value
            const uint32_t s0 = __float_as_uint(a), which = __float_as_uint(b);
            uint32_t s = s0, out5 = 0u, out12 = 0u;
            for (int k = 1; k <= 12; ++k) {
                const uint32_t o = next_random_number(s);
                if (k == 5) out5 = o;
                if (k == 12) out12 = o;
            }
            const uint32_t v = which == 0u ? rng_output(rng_jump<5>(s0)) : which == 1u ? out5 : which == 2u ? rng_output(rng_jump<12>(s0))
                             : which == 3u ? out12 : which == 4u ? rng_jump<12>(s0) : s;
            r = __uint_as_float(v);
            break;
        }
        case 20: {  // the terminal skip's jump against the generator stepped 8 times; y (bits) selects the value
            const uint32_t s0 = __float_as_uint(a), which = __float_as_uint(b);
            uint32_t s = s0, out8 = 0u;
            for (int k = 1; k <= 8; ++k) out8 = next_random_number(s);
            const uint32_t v = which == 0u ? rng_output(rng_jump<8>(s0)) : which == 1u ? out8 : which == 2u ? rng_jump<8>(s0) : s;
            r = __uint_as_float(v);
            break;
        }
        default: break;
    }
    out[i] = r;
}

__global__ void __launch_bounds__(256) rt_units_texture_kernel(const uint8_t* rgba8, uint32_t width, uint32_t height,
                                                               const float* srgb_lut, const float* __restrict__ uv,
                                                               float* __restrict__ out, unsigned long long n) {
    const unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    typedef const __attribute__((address_space(1))) uint32_t* GWords;
    typedef const __attribute__((address_space(1))) float* GFloats;
    float o[4];
    rtm::sample_bilinear_words((GWords)(const void*)rgba8, width, height, (GFloats)(const void*)srgb_lut, uv[2 * i], uv[2 * i + 1], o);
    out[4 * i] = o[0]; out[4 * i + 1] = o[1]; out[4 * i + 2] = o[2]; out[4 * i + 3] = o[3];
}

// Every float x the short forms serve: rcp_core(x) against the compiler's IEEE 1.0f / x (which = 0), sqrt_core(x)
// against its sqrt (which = 1), and the sky's shortcuts against their literal forms -- sky_gradient_t (2) and
// ground_to_sky_t (3) for every float in [-1.5, 1.5] plus NaN and the infinities, sun_term (4) for every float in
// [0, 1.5] (max(0, .) never hands it anything negative) -- bit for bit.  out[0] = floats checked, out[1] = mismatches,
// out[2] = a mismatching bit pattern.
__global__ void __launch_bounds__(256) rt_sweep_kernel(int which, unsigned long long* out) {
    unsigned long long checked = 0, bad = 0;
    for (unsigned long long b = (unsigned long long)blockIdx.x * 256u + threadIdx.x; b < (1ull << 32); b += (unsigned long long)gridDim.x * 256u) {
        const float x = __uint_as_float((uint32_t)b);
        bool in_range;
        if (which == 0) in_range = rcp_in_range(x);
        else if (which == 1) in_range = sqrt_in_range(x);
        else if (which == 4) in_range = (x >= 0.0f && x <= 1.5f) || x != x;
        else in_range = rtm::abs_(x) <= 1.5f || x != x || rtm::abs_(x) == __uint_as_float(0x7f800000u);
        if (!in_range) continue;
        float q = which == 0 ? 1.0f / x : which == 1 ? rtm::sqrt_(x) : which == 2 ? sky_gradient_t_literal(x)
                                                     : which == 3 ? ground_to_sky_t_literal(x) : sun_literal(x);
        asm volatile("" : "+v"(q));
        const float f = which == 0 ? rcp_core(x) : which == 1 ? sqrt_core(x) : which == 2 ? sky_gradient_t(x)
                                                 : which == 3 ? ground_to_sky_t(x) : sun_term(x);
        checked += 1;
        const bool both_nan = f != f && q != q;  // (NaN sign and payload are outside the arithmetic contract)
        if (!both_nan && __float_as_uint(f) != __float_as_uint(q)) {
            bad += 1;
            out[2] = b;
        }
    }
    atomicAdd(&out[0], checked);
    if (bad) atomicAdd(&out[1], bad);
}
hipError_t launch_sweep(int which, unsigned long long* out, hipStream_t stream) {
    hipLaunchKernelGGL(rt_sweep_kernel, dim3(4096), dim3(256), 0, stream, which, out);
    return hipGetLastError();
}

// Test-only: intersect_scene for rays the host chooses (rt_test_intersect, tests/test_gpu_intersect.py), one lane per ray,
// with the prologue and stack of rt_debug_kernel and the instantiation launch_render would take (or the one the caller
// forces).  A lane whose `active` byte is 0 stays out of intersect_scene, as lanes do in the partial waves the vote and
// the refill create.  Record per ray (16 words, RT_TEST_ISECT_WORDS): hit, dst, point xyz, normal xyz, u, v, backface,
// winner (mesh index, or n_meshes + sphere index; ~0 on a miss), node tests, triangle tests, instantiation bits, 0.
template <bool LDS, bool TLAS, bool SIMPLE, bool STATS>
__global__ void __launch_bounds__(BLOCK_THREADS) rt_test_intersect_kernel(const RenderArgs a, const float* __restrict__ ro,
                                                                          const float* __restrict__ rd,
                                                                          const uint8_t* __restrict__ active,
                                                                          unsigned long long n, uint32_t* __restrict__ out) {
    uint32_t* stack = stack_of<total_in_lds(LDS)>(block_prologue<LDS>(a));
    const unsigned long long i = (unsigned long long)blockIdx.x * BLOCK_THREADS + threadIdx.x;
    if (i >= n || (active != nullptr && active[i] == 0u)) return;
    const f3 o{ro[3 * i], ro[3 * i + 1], ro[3 * i + 2]}, d{rd[3 * i], rd[3 * i + 1], rd[3 * i + 2]};
    int node_tests = 0, tri_tests = 0;
    Isect unused;
    const Hit h = intersect_scene<LDS, STATS, TLAS, false, SIMPLE>(a, o, d, stack, node_tests, tri_tests, unused);
    uint32_t* r = out + i * 16u;
    r[0] = h.hit ? 1u : 0u;
    r[1] = __float_as_uint(h.dst);
    r[2] = __float_as_uint(h.point.x); r[3] = __float_as_uint(h.point.y); r[4] = __float_as_uint(h.point.z);
    r[5] = __float_as_uint(h.normal.x); r[6] = __float_as_uint(h.normal.y); r[7] = __float_as_uint(h.normal.z);
    r[8] = __float_as_uint(h.u);
    r[9] = __float_as_uint(h.v);
    r[10] = h.backface ? 1u : 0u;
    r[11] = h.hit ? hit_ids_of<SIMPLE>(a, h, unused).object : 0xffffffffu;
    r[12] = (uint32_t)node_tests;
    r[13] = (uint32_t)tri_tests;
    r[14] = (TLAS ? 1u : 0u) | (SIMPLE ? 2u : 0u) | (STATS ? 32u : 0u) | (LDS ? 64u : 0u);
    r[15] = 0u;
}

// simple: the SIMPLE instantiation (few-mesh scenes only: the host checks), stats: the counter instantiation
hipError_t launch_test_intersect(const RenderArgs& a, const float* ro, const float* rd, const uint8_t* active,
                                 unsigned long long n, bool simple, bool stats, uint32_t* out, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const size_t lds = render_lds_bytes(a);
    const uint32_t blocks = (uint32_t)((n + BLOCK_THREADS - 1) / BLOCK_THREADS);
    with_instantiation(a, simple, [&](auto lds_tag, auto tlas_tag, auto simple_tag) {
        constexpr bool LDS = decltype(lds_tag)::value, TLAS = decltype(tlas_tag)::value, SIMPLE = decltype(simple_tag)::value;
        if (stats) launch_k(rt_test_intersect_kernel<LDS, TLAS, SIMPLE, true>, blocks, lds, stream, a, ro, rd, active, n, out);
        else launch_k(rt_test_intersect_kernel<LDS, TLAS, SIMPLE, false>, blocks, lds, stream, a, ro, rd, active, n, out);
    });
    return hipGetLastError();
}

// Test-only: path_end / roulette_skip for lane states the host chooses (rt_test_shade, tests/test_gpu_shade.py), one lane
// per case, with the prologue of the render kernels (the scene staged where LDS, the lane's LDS state) and the product's
// functions themselves, unchanged.  A lane whose `active` byte is 0 stays out of the call, as lanes do in the partial
// waves the vote and the refill create.  Case and record: 32 words each (RT_TEST_SHADE_WORDS, include/rt_test_abi.h).
// TOTAL_LDS is a parameter of its own here: the render kernels take total_in_lds(LDS), the callers that keep the sum in
// registers (-DRT_TOTAL_IN_LDS=0, the experiments' wavefront kernels) the other one.
static_assert(STEP_END == 0u && STEP_TRAVERSE == 3u, "RT_TEST_SHADE_STEP_END / _STEP_TRAVERSE of include/rt_test_abi.h");
template <bool LDS, bool SIMPLE, bool FAST_MISS, bool TOTAL_LDS>
__global__ void __launch_bounds__(BLOCK_THREADS) rt_test_shade_kernel(const RenderArgs a, int which, const uint32_t* __restrict__ cases,
                                                                      const uint8_t* __restrict__ active, unsigned long long n,
                                                                      uint32_t* __restrict__ out) {
    uint32_t* ls = block_prologue<LDS>(a);
    const unsigned long long i = (unsigned long long)blockIdx.x * BLOCK_THREADS + threadIdx.x;
    if (i >= n || (active != nullptr && active[i] == 0u)) return;
    const uint32_t* c = cases + i * 32u;
    auto f = [&](uint32_t k) { return __uint_as_float(c[k]); };
    PixelState s;
    s.x = 0u;
    s.out_row = 0u;
    s.ro = f3{0, 0, 0};
    s.rd = f3{f(0), f(1), f(2)};
    s.T = f4{f(3), f(4), f(5), f(6)};
    s.light = f4{f(7), f(8), f(9), f(10)};
    s.total = f4{f(11), f(12), f(13), f(14)};
    s.rng = c[15];
    s.seg = (int32_t)c[16];
    s.j = (int32_t)c[17];
    s.fresh = false;
    s.meta = c[31];
    if constexpr (TOTAL_LDS) {  // (the lane's LDS state only exists in the launches whose map has it: launch_test_shade)
        ls[0] = c[11]; ls[64] = c[12]; ls[128] = c[13]; ls[192] = c[14];
    }
    Hit hit;
    hit.hit = c[19] != 0u;
    hit.dst = f(20);
    hit.point = f3{f(21), f(22), f(23)};
    hit.normal = f3{f(24), f(25), f(26)};
    hit.u = f(27);
    hit.v = f(28);
    hit.backface = c[29] != 0u;
    hit.mat_off = a.lay.mat_off + c[30] * MATERIAL_BYTES;  // (the host checked the index)
    hit.suspended = false;
    uint32_t n_segments = 0u, more_reused = 0u;
    bool ret;
    if (which == 0) {
        ret = path_end<LDS, TOTAL_LDS, SIMPLE, FAST_MISS>(a, s, ls, c[18], hit, n_segments, &more_reused);
    } else {
        s.fresh = true;  // (the pre-step calls it in front of a sample)
        ret = roulette_skip<LDS, TOTAL_LDS, SIMPLE>(a, s, ls, (hit.mat_off & ~15u) | MEMO_HIT | MEMO_RAY | MEMO_HIT_VALID, n_segments, more_reused);
    }
    f4 total = s.total;
    if constexpr (TOTAL_LDS)
        total = f4{__uint_as_float(ls[0]), __uint_as_float(ls[64]), __uint_as_float(ls[128]), __uint_as_float(ls[192])};
    uint32_t* r = out + i * 32u;
    r[0] = __float_as_uint(s.ro.x); r[1] = __float_as_uint(s.ro.y); r[2] = __float_as_uint(s.ro.z);
    r[3] = __float_as_uint(s.rd.x); r[4] = __float_as_uint(s.rd.y); r[5] = __float_as_uint(s.rd.z);
    r[6] = __float_as_uint(s.T.x); r[7] = __float_as_uint(s.T.y); r[8] = __float_as_uint(s.T.z); r[9] = __float_as_uint(s.T.w);
    r[10] = __float_as_uint(s.light.x); r[11] = __float_as_uint(s.light.y); r[12] = __float_as_uint(s.light.z); r[13] = __float_as_uint(s.light.w);
    r[14] = __float_as_uint(total.x); r[15] = __float_as_uint(total.y); r[16] = __float_as_uint(total.z); r[17] = __float_as_uint(total.w);
    r[18] = s.rng;
    r[19] = (uint32_t)s.seg;
    r[20] = (uint32_t)s.j;
    r[21] = s.fresh ? 1u : 0u;
    r[22] = ret ? 1u : 0u;
    r[23] = n_segments;
    r[24] = s.meta;
    r[25] = (a.many_mesh != 0u ? 1u : 0u) | (SIMPLE ? 2u : 0u) | (FAST_MISS ? 0u : 32u) | (LDS ? 64u : 0u) | (TOTAL_LDS ? 128u : 0u);
    r[26] = more_reused;
    r[27] = 0u; r[28] = 0u; r[29] = 0u; r[30] = 0u; r[31] = 0u;
}

// simple: the SIMPLE instantiation (few-mesh scenes only: the host checks); fast_miss / total_lds: path_end's FAST_MISS /
// TOTAL_LDS.  total_lds needs total_in_lds(a.lds_scene): only then does the launch's LDS map hold the lane state.
hipError_t launch_test_shade(const RenderArgs& a, int which, const uint32_t* cases, const uint8_t* active, unsigned long long n,
                             bool simple, bool fast_miss, bool total_lds, uint32_t* out, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (total_lds && !total_in_lds(a.lds_scene != 0u)) return hipErrorInvalidValue;
    const size_t lds = render_lds_bytes(a);
    const uint32_t blocks = (uint32_t)((n + BLOCK_THREADS - 1) / BLOCK_THREADS);
    with_instantiation(a, simple, [&](auto lds_tag, auto, auto simple_tag) {
        constexpr bool LDS = decltype(lds_tag)::value, SIMPLE = decltype(simple_tag)::value;
        auto go = [&](auto fm_tag, auto tl_tag) {
            launch_k(rt_test_shade_kernel<LDS, SIMPLE, decltype(fm_tag)::value, decltype(tl_tag)::value>, blocks, lds, stream, a, which,
                     cases, active, n, out);
        };
        if (fast_miss && total_lds) go(std::true_type{}, std::true_type{});
        else if (fast_miss) go(std::true_type{}, std::false_type{});
        else if (total_lds) go(std::false_type{}, std::true_type{});
        else go(std::false_type{}, std::false_type{});
    });
    return hipGetLastError();
}

hipError_t launch_units(int fn, const float* x, const float* y, float* out, unsigned long long n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(rt_units_kernel, dim3((uint32_t)((n + 255u) / 256u)), dim3(256), 0, stream, fn, x, y, out, n);
    return hipGetLastError();
}

hipError_t launch_units_texture(const uint8_t* rgba8, uint32_t width, uint32_t height, const float* srgb_lut, const float* uv,
                                float* out, unsigned long long n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(rt_units_texture_kernel, dim3((uint32_t)((n + 255u) / 256u)), dim3(256), 0, stream, rgba8, width, height,
                       srgb_lut, uv, out, n);
    return hipGetLastError();
}
