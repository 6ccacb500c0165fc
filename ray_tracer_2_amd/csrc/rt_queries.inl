// rt_queries.inl -- the ray-query, pick, G-buffer and radiance kernels with their launchers (included by rt_kernel.hip inside
// namespace rtd, behind the render kernels and the launch helpers they share: launch_k, with_instantiation).
// ---------------------------------------------------------------------------
// Ray queries (rt_intersect_rays, rt_occluded_rays, rt_pick; include/rt_abi.h): intersect_scene for rays the host gives,
// on the uploaded scene, in the instantiation a render of it takes (scene_args, with_instantiation).  A persistent grid:
// every workgroup stages an LDS scene once and then takes rays with a grid stride, one lane per ray, with the prologue
// and stack layout of the render kernels.  rays: rt_ray records (32 B: origin, tmax, dir, _p0).  ANY = false writes one
// rt_hit (64 B) per ray, ANY = true one u32 (occluded) per ray.  A ray with a non-finite component, a direction whose
// normalize3 is not finite and non-zero, tmax <= 0 or NaN, or _p0 != 0 gets a miss record.
// ---------------------------------------------------------------------------
template <bool LDS, bool TLAS, bool SIMPLE, bool ANY>
__global__ void __launch_bounds__(BLOCK_THREADS) rt_query_kernel(const RenderArgs a, const float4* __restrict__ rays,
                                                                 unsigned long long n, void* __restrict__ out,
                                                                 uint32_t prune_tmax) {
    uint32_t* stack = stack_of<total_in_lds(LDS)>(block_prologue<LDS>(a));
    const unsigned long long stride = (unsigned long long)gridDim.x * BLOCK_THREADS;
    for (unsigned long long i = (unsigned long long)blockIdx.x * BLOCK_THREADS + threadIdx.x; i < n; i += stride) {
        const float4 r0 = rays[2 * i], r1 = rays[2 * i + 1];
        const f3 ro{r0.x, r0.y, r0.z}, d{r1.x, r1.y, r1.z};
        const float tmax = r0.w;
        const f3 rd = normalize3(d);
        const bool valid = ray_is_valid(ro, d, rd, tmax, fbits(r1.w));
        int node_tests = 0, tri_tests = 0;
        Isect I;
        if constexpr (ANY) {
            bool occluded = false;
            if (valid) occluded = intersect_scene<LDS, false, TLAS, false, SIMPLE, false, true>(a, ro, rd, stack, node_tests, tri_tests, I, tmax, prune_tmax != 0u).hit;
            static_cast<uint32_t*>(out)[i] = occluded ? 1u : 0u;
        } else {
            Hit h{};
            if (valid) h = intersect_scene<LDS, false, TLAS, false, SIMPLE, false, false, true>(a, ro, rd, stack, node_tests, tri_tests, I);
            float4* o = static_cast<float4*>(out) + 4 * i;
            if (valid && h.hit && h.dst < tmax) {
                const HitIds id = hit_ids_of<SIMPLE>(a, h, I);
                o[0] = make_float4(h.dst, __uint_as_float(id.object), __uint_as_float(id.primitive), __uint_as_float(id.flags));
                o[1] = make_float4(h.point.x, h.point.y, h.point.z, id.bary_u);
                o[2] = make_float4(h.normal.x, h.normal.y, h.normal.z, id.bary_v);
                o[3] = make_float4(h.u, h.v, 0.0f, 0.0f);
            } else {
                o[0] = make_float4(__builtin_inff(), __uint_as_float(0xffffffffu), __uint_as_float(0xffffffffu), 0.0f);
                o[1] = o[2] = o[3] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            }
        }
    }
}

// rt_pick: the ray rt_debug_kernel traces for texel (x, y) -- texel_ray_of -- as one rt_ray with tmax = +inf
// (not normalised here: the query kernel's normalize3 is rt_debug_kernel's)
__global__ void rt_pick_ray_kernel(const RenderArgs a, uint32_t x, uint32_t y, float4* __restrict__ ray) {
    const TexelRay r = texel_ray_of(a, a.params.width, a.params.height, x, y);
    ray[0] = make_float4(r.origin.x, r.origin.y, r.origin.z, __builtin_inff());
    ray[1] = make_float4(r.d.x, r.d.y, r.d.z, 0.0f);
}

hipError_t launch_pick_ray(const RenderArgs& a, uint32_t x, uint32_t y, float4* ray, hipStream_t stream) {
    hipLaunchKernelGGL(rt_pick_ray_kernel, dim3(1), dim3(1), 0, stream, a, x, y, ray);
    return hipGetLastError();
}

// any: occlusion (out: u32 per ray), else closest hit (out: rt_hit per ray).  The persistent grid: at least `blocks`
// workgroups (the render's persistent grid), raised to what the query kernel itself keeps resident on compute_units CUs
// -- its registers allow more waves per SIMD than the render kernels' budget (measured: the render's grid of 4 waves
// per SIMD was slower than one workgroup per 256 rays) -- and at most one workgroup per 256 rays.
hipError_t launch_query(const RenderArgs& a, const void* rays, unsigned long long n, void* out, bool any, bool prune_tmax,
                        uint32_t blocks, uint32_t compute_units, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const size_t lds = render_lds_bytes(a);
    const unsigned long long need = (n + BLOCK_THREADS - 1) / BLOCK_THREADS;
    auto go = [&](auto kernel) {
        allow_lds(kernel, lds);  // (before the occupancy is asked for)
        int per_cu = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, BLOCK_THREADS, lds) == hipSuccess && per_cu > 0 &&
            (unsigned long long)per_cu * compute_units > blocks)
            blocks = (uint32_t)per_cu * compute_units;
        if (need < blocks) blocks = (uint32_t)need;
        if (blocks == 0) blocks = 1;
        launch_k(kernel, blocks, lds, stream, a, static_cast<const float4*>(rays), n, out, prune_tmax ? 1u : 0u);
    };
    with_instantiation(a, render_takes_simple(a), [&](auto lds_tag, auto tlas_tag, auto simple_tag) {
        constexpr bool LDS = decltype(lds_tag)::value, TLAS = decltype(tlas_tag)::value, SIMPLE = decltype(simple_tag)::value;
        any ? go(rt_query_kernel<LDS, TLAS, SIMPLE, true>) : go(rt_query_kernel<LDS, TLAS, SIMPLE, false>);
    });
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// First-hit buffers of a frame (rt_render_gbuffer; include/rt_abi.h): for every texel of rows
// [row0, row0 + rows) the ray rt_debug_kernel / rt_pick_ray_kernel generate for it -- the same operations --, validated
// and intersected as rt_query_kernel does it for rt_pick (same instantiation, EXPORT), and the hit written channel by
// channel into the planes that are not NULL (wave-uniform branches: a channel that is off costs nothing, the texture
// filter included).  One wave per chunk of 64 texels (the queries' persistent grid was measured a sixth slower here) -- for
// the few-mesh kernels 64 consecutive texels of the band in row-major order (the planes are tightly packed, so the band is ONE array:
// every store of a wave is one contiguous run for any width), for the many-mesh kernels (TLAS), whose walk gains a fifth
// from coherent rays, a tile of 8x8 texels (runs of 8 texels per row); measured, DESIGN.md section 2.10.
// Every channel is ONE store per lane of the texel's 1, 4, 8, 12 or 16 contiguous bytes (the planes of 2 and 3 floats
// are only 4-byte aligned: global memory takes such a store): lane after lane a run's bytes are contiguous, so one
// instruction fills every 32-byte sector it touches but the run's two ends.
// The wave index is read from the first lane, so the chunk's place in the frame is wave-uniform; a plane is addressed from
// the chunk's first texel in it -- a scalar base, passed through scalar_base so that the compiler keeps it apart from the
// lane's part instead of holding eleven per-lane 64-bit addresses across the walk -- plus the lane's texel within the
// chunk, a 32-bit element index.
// ---------------------------------------------------------------------------
template <class T>
DEV T* scalar_base(T* p) {
    unsigned long long b = reinterpret_cast<unsigned long long>(p);
    asm("" : "+s"(b));  // (no instruction: the value is wave-uniform and lives in a scalar register pair from here on)
    return reinterpret_cast<T*>(b);
}
// The planes are written once and read by nobody in the launch: streaming stores keep them from displacing the scene in L2.
// base: the chunk's first texel in the plane; e: this lane's texel from there.  (global-address-space pointers:
// global_store, not flat_store -- the integer round trip of scalar_base forgets the address space)
#define RT_GLOBAL(T, p) ((__attribute__((address_space(1))) T*)(void*)(p))
template <class T>
DEV void store_plane(T* base, uint32_t e, T v) { __builtin_nontemporal_store(v, RT_GLOBAL(T, base + e)); }
DEV void store_plane(float4* base, uint32_t e, float4 v) {
    typedef float v4f __attribute__((ext_vector_type(4)));
    __builtin_nontemporal_store(v4f{v.x, v.y, v.z, v.w}, RT_GLOBAL(v4f, base + e));
}
DEV void store_plane2(float* base, uint32_t e, float x, float y) {
    typedef float v2f __attribute__((ext_vector_type(2), aligned(4)));
    __builtin_nontemporal_store(v2f{x, y}, RT_GLOBAL(v2f, base + 2u * (size_t)e));
}
DEV void store_plane3(float* base, uint32_t e, float x, float y, float z) {
    typedef float v3f __attribute__((ext_vector_type(3), aligned(4)));
    __builtin_nontemporal_store(v3f{x, y, z}, RT_GLOBAL(v3f, base + 3u * (size_t)e));
}

template <bool LDS, bool TLAS, bool SIMPLE>
__global__ void __launch_bounds__(BLOCK_THREADS) rt_gbuffer_kernel(const RenderArgs a, const GBufferArgs g) {
    constexpr bool TILES = TLAS;
    uint32_t* stack = stack_of<total_in_lds(LDS)>(block_prologue<LDS>(a));
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6)));
    const uint32_t chunk = wave;
    const uint32_t n = g.rows * g.width;  // (<= 2^31 - 1: the host checks)
    const uint32_t tiles_x = (g.width + 7u) >> 3;
    // this lane's texel from the chunk's first one, in the planes (a tile's rows beyond the band wrap: never stored)
    const uint32_t e = TILES ? (lane >> 3) * g.width + (lane & 7u) : lane;
    {
        uint32_t x, yl, first;  // this lane's texel in the band; the chunk's first texel in the planes
        bool inside;
        if constexpr (!TILES) {
            first = chunk * 64u;
            const uint32_t i = first + lane;
            inside = i < n;
            yl = i / g.width;
            x = i - yl * g.width;
        } else {
            const uint32_t ty = chunk / tiles_x, x0 = (chunk - ty * tiles_x) << 3;
            x = x0 + (lane & 7u);
            yl = ty * 8u + (lane >> 3);
            inside = yl < g.rows && x < g.width;
            first = ty * 8u * g.width + x0;
        }
        // wgsl:502-515, as rt_debug_kernel
        const TexelRay ray = texel_ray_of(a, g.width, g.height, x, g.row0 + yl);
        const f3 cam_origin = ray.origin, d = ray.d;
        const f3 rd = normalize3(d);
        // rt_query_kernel's validity of the rt_ray (cam_origin, +inf, d, 0) and its closest hit
        const bool valid = inside && ray_is_valid(cam_origin, d, rd, __builtin_inff(), 0u);
        if (g.dir && inside) store_plane3(scalar_base(g.dir + 3u * (size_t)first), e, rd.x, rd.y, rd.z);  // (before the walk: nothing of the ray outlives it)
        int node_tests = 0, tri_tests = 0;
        Isect I;
        Hit h{};
        if (valid) h = intersect_scene<LDS, false, TLAS, false, SIMPLE, false, false, true>(a, cam_origin, rd, stack, node_tests, tri_tests, I);
        const bool hit = valid && h.hit && h.dst < __builtin_inff();
        const HitIds id = hit_ids_of<SIMPLE>(a, h, I);
        if (g.depth && inside) store_plane(scalar_base(g.depth + first), e, hit ? h.dst : __builtin_inff());
        if (g.object && inside) store_plane(scalar_base(g.object + first), e, hit ? id.object : 0xffffffffu);
        if (g.primitive && inside) store_plane(scalar_base(g.primitive + first), e, hit ? id.primitive : 0xffffffffu);
        if (g.flags && inside) store_plane(scalar_base(g.flags + first), e, hit ? (uint8_t)id.flags : (uint8_t)0u);
        if (g.point && inside) store_plane3(scalar_base(g.point + 3u * (size_t)first), e, hit ? h.point.x : 0.0f, hit ? h.point.y : 0.0f, hit ? h.point.z : 0.0f);
        if (g.normal && inside) store_plane3(scalar_base(g.normal + 3u * (size_t)first), e, hit ? h.normal.x : 0.0f, hit ? h.normal.y : 0.0f, hit ? h.normal.z : 0.0f);
        if (g.bary && inside) store_plane2(scalar_base(g.bary + 2u * (size_t)first), e, hit ? id.bary_u : 0.0f, hit ? id.bary_v : 0.0f);
        if (g.texcoord && inside) store_plane2(scalar_base(g.texcoord + 2u * (size_t)first), e, hit ? h.u : 0.0f, hit ? h.v : 0.0f);
        if (g.albedo) {  // `color` of wgsl:453-458
            float4 color = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (hit) {
                const int flag = ldi<LDS>(a, h.mat_off + M_FLAG), diffuse_index = ldi<LDS>(a, h.mat_off + M_DIFFUSE_IDX);
                if (!SIMPLE && flag == RT_MATERIAL_TEXTURE && diffuse_index != -1) {
                    const f4 s = sample_texture(a, diffuse_index, h.u, h.v);
                    color = make_float4(s.x, s.y, s.z, s.w);
                } else {
                    color = ld4<LDS>(a, h.mat_off + M_COLOR);
                }
            }
            if (inside) store_plane(scalar_base(g.albedo + first), e, color);
        }
        if (g.emission) {  // wgsl:450
            float4 em = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (hit) {
                const float4 ec = ld4<LDS>(a, h.mat_off + M_EMISSION);
                const float es = ldf<LDS>(a, h.mat_off + M_EMISSION_S);
                em = make_float4(ec.x * es, ec.y * es, ec.z * es, ec.w * es);
            }
            if (inside) store_plane(scalar_base(g.emission + first), e, em);
        }
    }
}

// grid: one wave per chunk (the workgroups of the last partial one have waves without a chunk: they stage and leave).
// Measured against the queries' persistent grid, which restages an LDS scene less often: DESIGN.md section 2.10.
hipError_t launch_gbuffer(const RenderArgs& a, const GBufferArgs& g, hipStream_t stream) {
    const uint32_t chunks = gbuffer_chunks(g, a.many_mesh != 0u);
    if (chunks == 0) return hipSuccess;
    const size_t lds = render_lds_bytes(a);
    const uint32_t blocks = (chunks + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
    with_instantiation(a, render_takes_simple(a), [&](auto lds_tag, auto tlas_tag, auto simple_tag) {
        launch_k(rt_gbuffer_kernel<decltype(lds_tag)::value, decltype(tlas_tag)::value, decltype(simple_tag)::value>, blocks, lds,
                 stream, a, g);
    });
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Radiance queries (rt_radiance_rays; include/rt_abi.h): `frag`'s sample loop (wgsl:486-498) for rays
// the host gives, the ray held fixed -- per ray: state = seed; per sample the four draws of the camera jitter (a jump, as
// path_begin makes them for a constant primary ray), then total += trace(ray, &state); out = total / f32(rays_per_pixel).
// rays: rt_path_ray records (32 B: origin, seed, dir, _p0).  One lane per ray in persistent waves with the render kernel's
// refill: a wave claims 64 consecutive rays from a shared counter and hands them to its lanes as they finish theirs
// (ballot + mbcnt), so no lane waits for the wave's slowest ray.  out[i] is ray i's whoever computed it.
// The ray is the same for every sample, so its first hit is the pixel memo's case: with RenderArgs::pixel_cache == 1 the
// lane keeps the hit of sample 0 in its LDS memo (memo_hit_store) and samples 1.. take it from there (memo_hit_load) --
// with them path_end's fast_miss and the pre-step's roulette_skip, which are defined on that memo.  pixel_cache == 0 (the
// host found no room in the LDS): every sample traverses.  Shading, roulette and the sum are path_end's; the ray itself
// is read again from `rays` at every sample (two 16-byte loads) rather than held in six registers across the walk.
// A ray that rt_query_kernel would call invalid (tmax = +INF) gets zeros.
// ---------------------------------------------------------------------------
// the ray of record i, normalised as trace does it (wgsl:400); returns whether a query traces it (ray_is_valid)
template <bool SQ>
DEV bool path_ray_of(const float4* __restrict__ rays, uint32_t i, f3& ro, f3& rd, uint32_t& seed) {
    const float4 r0 = rays[2 * (size_t)i], r1 = rays[2 * (size_t)i + 1];
    const f3 d{r1.x, r1.y, r1.z};
    ro = f3{r0.x, r0.y, r0.z};
    rd = normalize3<SQ>(d);
    seed = fbits(r0.w);
    return ray_is_valid(ro, d, rd, __builtin_inff(), fbits(r1.w));
}

// A lane takes ray i (pixel_begin's counterpart: PixelState::x is the ray's index, the memo holds a ray and no hit yet)
template <bool TOTAL_LDS>
DEV void ray_begin(const RenderArgs& a, PixelState& s, uint32_t* ls, uint32_t i, uint32_t seed) {
    s.x = i;
    s.out_row = 0u;
    s.rng = seed;
    if constexpr (TOTAL_LDS) {
        ls[0] = 0u; ls[64] = 0u; ls[128] = 0u; ls[192] = 0u;  // total = 0
    }
    s.total = f4{0, 0, 0, 0};
    s.j = 0;
    s.fresh = true;
    s.seg = 0;
    s.meta = 0;
    if (a.pixel_cache != 0u) with_memo(a, ls, [&](auto pc) { pc[12 * 64] = MEMO_RAY; });
}

// The start of a sample (path_begin's counterpart for a ray of the host's): the jitter's four draws, the ray, a new path
template <bool SQ>
DEV void ray_path_begin(PixelState& s, const float4* __restrict__ rays) {
    s.rng = rng_jump<4>(s.rng);  // (wgsl:488-492: the two disks' angle and radius draws, never read)
    uint32_t seed;
    (void)path_ray_of<SQ>(rays, s.x, s.ro, s.rd, seed);
    s.T = f4{1, 1, 1, 1};
    s.light = f4{0, 0, 0, 0};
    s.seg = 0;
    s.fresh = false;
}

template <bool LDS, bool TLAS, bool SIMPLE>
__global__ void __launch_bounds__(BLOCK_THREADS) rt_radiance_kernel(const RenderArgs a, const float4* __restrict__ rays, uint32_t n,
                                                                    float4* __restrict__ out, uint32_t* __restrict__ next_ray) {
    constexpr bool TOTAL_LDS = total_in_lds(LDS);
    uint32_t* ls = block_prologue<LDS>(a);
    uint32_t* stack = stack_of<TOTAL_LDS>(ls);
    const uint32_t lane = threadIdx.x & 63u;
    const bool cache_on = a.pixel_cache != 0u;  // wave-uniform
    uint32_t pool_base = 0, pool_left = 0;      // wave-uniform: the rays the wave has claimed and not handed out
    bool exhausted = false, active = false;
    PixelState s;
    ray_begin<TOTAL_LDS>(a, s, ls, 0u, 0u);
    s.T = f4{1, 1, 1, 1};
    s.light = f4{0, 0, 0, 0};
    s.ro = f3{0, 0, 0};
    s.rd = f3{0, 0, 1};
    uint32_t n_segments = 0, more_reused = 0;  // (path_end's counters: nobody reads them here)
    int node_tests = 0, tri_tests = 0;
    for (;;) {
        const unsigned long long idle = __ballot(!active);
        if (idle != 0ull && !exhausted) {
            if (pool_left == 0u) {
                uint32_t t = 0;
                if (lane == 0u) t = atomicAdd(next_ray, 64u);  // (n <= 2^31 - 1 and every wave stops at its first claim beyond n: no wrap)
                t = __builtin_amdgcn_readfirstlane(t);
                if (t >= n) {
                    exhausted = true;
                } else {
                    pool_base = t;
                    pool_left = n - t < 64u ? n - t : 64u;
                }
            }
            if (pool_left != 0u) {
                const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));
                if (!active && rank < pool_left) {
                    const uint32_t i = pool_base + rank;
                    f3 ro, rd;
                    uint32_t seed;
                    if (path_ray_of<!LDS>(rays, i, ro, rd, seed)) {
                        ray_begin<TOTAL_LDS>(a, s, ls, i, seed);
                        active = true;
                    } else {
                        out[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    }
                }
                const uint32_t n_idle = (uint32_t)__popcll(idle);
                const uint32_t took = n_idle < pool_left ? n_idle : pool_left;
                pool_base += took;
                pool_left -= took;
            }
        }
        if (__ballot(active) == 0ull) {
            if (exhausted) break;
            continue;
        }
        if (active) {
            bool done = false;
            if (s.fresh) {
                // The sample's first segment from the memo, then on to its next one in this same iteration (path_step's
                // pre-step): the lanes that are past their ray's first sample join this iteration's traversal.
                uint32_t st = 0u;
                if (cache_on) with_memo(a, ls, [&](auto pc) { st = pc[12 * 64]; });
                const bool memo = (st & MEMO_HIT_VALID) != 0u;
#if RT_ROULETTE_SKIP
                if (memo && a.roulette_skip != 0u && roulette_skip<LDS, TOTAL_LDS, SIMPLE>(a, s, ls, st, n_segments, more_reused)) done = true;
#endif
                if (!done) {
                    ray_path_begin<!LDS>(s, rays);
                    if (memo) {
                        Hit mh;
                        mh.hit = false;
                        mh.suspended = false;
                        memo_hit_load<false, false>(a, s, ls, mh);
                        done = path_end<LDS, TOTAL_LDS, SIMPLE, true>(a, s, ls, STEP_REUSE, mh, n_segments, &more_reused);
                    }
                }
            }
            if (!done && !s.fresh) {
                Isect I;
                const Hit hit = intersect_scene<LDS, false, TLAS, false, SIMPLE>(a, s.ro, s.rd, stack, node_tests, tri_tests, I);
                memo_hit_store<false, false, false>(a, s, ls, hit);  // (the first segment of the ray's first sample)
                done = path_end<LDS, TOTAL_LDS, SIMPLE, true>(a, s, ls, STEP_TRAVERSE, hit, n_segments, &more_reused);
            }
            if (done) {  // wgsl:498, as pixel_finish
                f4 total = s.total;
                if constexpr (TOTAL_LDS)
                    total = f4{__uint_as_float(ls[0]), __uint_as_float(ls[64]), __uint_as_float(ls[128]), __uint_as_float(ls[192])};
                const float r = a.spp_reciprocal, spp = (float)a.params.rays_per_pixel;
                out[s.x] = r != 0.0f ? make_float4(total.x * r, total.y * r, total.z * r, total.w * r)
                                     : make_float4(total.x / spp, total.y / spp, total.z / spp, total.w / spp);
                active = false;
            }
        }
    }
}

// The persistent grid: what the kernel keeps resident on compute_units CUs, at most one wave per 64 rays.  next_ray: a
// zeroed counter of the launch's own.
hipError_t launch_radiance(const RenderArgs& a, const void* rays, uint32_t n, void* out, uint32_t* next_ray, uint32_t compute_units,
                           hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const size_t lds = render_lds_bytes(a);
    const uint32_t need = (n + BLOCK_THREADS - 1) / BLOCK_THREADS;
    with_instantiation(a, a.many_mesh == 0u && a.simple != 0u, [&](auto lds_tag, auto tlas_tag, auto simple_tag) {
        auto kernel = rt_radiance_kernel<decltype(lds_tag)::value, decltype(tlas_tag)::value, decltype(simple_tag)::value>;
        allow_lds(kernel, lds);  // (before the occupancy is asked for)
        int per_cu = 0;
        uint32_t blocks = compute_units * BLOCKS_PER_CU;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, BLOCK_THREADS, lds) == hipSuccess && per_cu > 0)
            blocks = (uint32_t)per_cu * compute_units;
        if (need < blocks) blocks = need;
        launch_k(kernel, blocks, lds, stream, a, static_cast<const float4*>(rays), n, static_cast<float4*>(out), next_ray);
    });
    return hipGetLastError();
}
