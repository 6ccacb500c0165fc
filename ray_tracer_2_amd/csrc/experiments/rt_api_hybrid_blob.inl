// rt_api_hybrid_blob.inl -- a STATEMENT FRAGMENT of rt_upload_scene (rt_api.hip includes it inside the function, with
// -DRT_EXPERIMENTS=1 only): the small blob of the hybrid launches of a deferred-walk sequence (option "hybrid"; DESIGN.md 5.4:
// built, parity-tested, measured no faster) -- the scene without the deferred mesh's BVH and triangles.  Possible when that
// mesh's wide records and triangles are the LAST of their arrays (indices are absolute: the other meshes' then form a prefix) --
// true of scenes that add one big model to a small set.  Reads the packer's results -- `g`, `s` (lay = s.lay) and the staging
// vectors `head` / `tail` --, uploads the small blob and sets the handle's small_ok / small_lay / small_stack_entries.
        std::vector<float4> small;
        SceneLayout sl{};
        uint32_t small_need = 1;
        bool small_ok = false;
        if (s.have_defer) {
            const MeshGeom& dm = g.mesh[s.defer_mesh];
            bool last = dm.wide_base + s.defer_internal == g.n_wide;
            for (uint32_t i = 0; i < n_meshes; ++i)
                if (i != s.defer_mesh) {
                    if (g.mesh[i].tri_hi > dm.tri_lo || g.mesh[i].wide_base > dm.wide_base) last = false;
                    small_need = std::max(small_need, g.mesh[i].need);
                }
            if (last && dm.tri_lo <= n_triangles) {
                const uint32_t nw = dm.wide_base, nt = dm.tri_lo;
                sl = lay;  // (the same leading sections: every offset up to wide_off)
                uint64_t o = lay.wide_off;
                o += (uint64_t)nw * WIDE_REC_BYTES;
                sl.tri_off = (uint32_t)o;    o += (uint64_t)nt * TRI_ISECT_BYTES;
                sl.shade_off = (uint32_t)o;  o += (uint64_t)nt * TRI_SHADE_BYTES;
                sl.bytes = (uint32_t)o;
                if (o <= LDS_BUDGET_BYTES) {
                    small.assign(o / 16, make_float4(0, 0, 0, 0));
                    auto copy_tail = [&](uint32_t dst, uint32_t src, uint64_t bytes) {  // (byte offsets of the two blobs)
                        if (bytes) memcpy((char*)small.data() + dst, (const char*)tail.data() + (src - lay.wide_off), bytes);
                    };
                    if (lay.wide_off) memcpy(small.data(), head.data(), lay.wide_off);
                    copy_tail(sl.wide_off, lay.wide_off, (uint64_t)nw * WIDE_REC_BYTES);
                    copy_tail(sl.tri_off, lay.tri_off, (uint64_t)nt * TRI_ISECT_BYTES);
                    copy_tail(sl.shade_off, lay.shade_off, (uint64_t)nt * TRI_SHADE_BYTES);
                    small_ok = true;
                }
            }
        }
        if (small_ok && (rc = upload(h, h->small_blob, small.data(), small.size())) != RT_OK) return rc;
        h->small_ok = small_ok;
        h->small_lay = sl;
        h->small_stack_entries = small_need;
