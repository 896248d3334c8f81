// render_scene.h -- the host code of a device's scene: everything that creates, checks, updates, reports on or destroys a DevScene
// (included by render.hip at file scope, behind rdev, ensure_ray_slots and the resolve_* rules).  It launches only the small kernels of
// render_update.h, render_instanced.h and render_motion.h (a deforming scene: render_update.h's); the frame loop and the launchers stay in
// render.hip.  One anonymous-namespace part -- the steps the entries share, each stated once, then the creations -- and one extern "C"
// part, the ABI of rodent_render.h.
#pragma once

namespace {

// ---- The steps the entries share ----
// the grid of a kernel that takes one thread per item in workgroups of kBlock
dim3 blocks(int n) { return dim3((unsigned)((n + kBlock - 1) / kBlock)); }

// `count` elements on the device (16 bytes at least), remembered in `owner` (DevScene::allocs, DeformSet::allocs) for the teardown;
// zeroed if asked for, else left as they come
template <typename T> T* device_alloc(std::vector<void*>& owner, size_t count, bool zero = false) {
    T* p = nullptr;
    const size_t bytes = std::max<size_t>(sizeof(T) * count, 16);
    HIP_CHECK(hipMalloc(&p, bytes));
    if (zero) HIP_CHECK(hipMemset(p, 0, bytes));
    owner.push_back(p);
    return p;
}
// ... filled from a host table
template <typename T> T* upload(std::vector<void*>& owner, const T* host, size_t count) {
    T* const p = device_alloc<T>(owner, count);
    if (count) HIP_CHECK(hipMemcpy(p, host, sizeof(T) * count, hipMemcpyHostToDevice));
    return p;
}

// A builder's or a refit's scratch with its `info_words` info words behind it, in one block
char* alloc_scratch_info(std::vector<void*>& owner, int64_t scratch_bytes, int info_words, int32_t*& info) {
    const size_t bytes = (size_t)std::max<int64_t>(scratch_bytes, 0);
    char* const scratch = device_alloc<char>(owner, bytes + 4 * (size_t)info_words);
    info = reinterpret_cast<int32_t*>(scratch + bytes);
    return scratch;
}
// ... for ONE synchronous call: the caller passes `scratch` and `info_dev` to the call and its return code to finish(), which brings the
// info words back (of a call that was accepted), frees the block and gives the verdict: the return code of a call that was refused, else
// the flags info[2], else 0x80000000 for a node count info[0] outside [min_nodes, max_nodes], else 0.
struct BuildScratch {
    std::vector<void*> block; int32_t* info_dev = nullptr; char* scratch; size_t info_bytes;
    BuildScratch(int64_t scratch_bytes, int info_words)
        : scratch(alloc_scratch_info(block, scratch_bytes, info_words, info_dev)), info_bytes(4 * (size_t)info_words) {}
    int32_t finish(int32_t rc, int32_t* info, int32_t min_nodes = 0, int32_t max_nodes = 0x7FFFFFFF) {
        if (rc == RODENT_BUILD_OK) HIP_CHECK(hipMemcpy(info, info_dev, info_bytes, hipMemcpyDeviceToHost));
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipFree(scratch));
        return rc != RODENT_BUILD_OK ? rc : info[2] ? info[2] : info[0] < min_nodes || info[0] > max_nodes ? (int32_t)0x80000000u : 0;
    }
};

// What brackets every device update of the loaded scene (a refit, a move, a deformation): `stream` runs behind the last update,
// whichever stream that took, and RenderDevice::ev_refit marks the end of this one.  Frames need no such wait: a frame call returns when
// its rows are in the film (frame_end), so none is in flight; the next one waits for ev_refit (open_scene).
hipStream_t begin_update(RenderDevice& r, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    HIP_CHECK(hipSetDevice(r.dev));
    if (!r.ev_refit) HIP_CHECK(hipEventCreateWithFlags(&r.ev_refit, hipEventDisableTiming));
    if (r.scene.refit_enqueued) HIP_CHECK(hipStreamWaitEvent(stream, r.ev_refit, 0));
    return stream;
}
void end_update(RenderDevice& r, hipStream_t stream) {
    HIP_CHECK(hipEventRecord(r.ev_refit, stream));
    r.scene.refit_enqueued = true;
}

// The scene's tables as the update kernels take them, and the copy-in of the caller's moved vertices and (if given) normals: a pointer
// that IS the scene's table means the caller wrote in place, no copy.
struct GeometryDev { float4 *vertices, *normals, *face_normals; const int4* indices; };
GeometryDev copy_in_geometry(const DevScene& s, const float* vertices_dev, const float* normals_dev, hipStream_t stream) {
    const GeometryDev g{reinterpret_cast<float4*>(const_cast<float*>(s.dev.vertices)),
        reinterpret_cast<float4*>(const_cast<float*>(s.dev.normals)), reinterpret_cast<float4*>(const_cast<float*>(s.dev.face_normals)),
        reinterpret_cast<const int4*>(s.dev.indices)};
    const size_t bytes = sizeof(float4) * (size_t)s.num_vertices;
    if (vertices_dev != s.dev.vertices) HIP_CHECK(hipMemcpyAsync(g.vertices, vertices_dev, bytes, hipMemcpyDeviceToDevice, stream));
    if (normals_dev && normals_dev != s.dev.normals)
        HIP_CHECK(hipMemcpyAsync(g.normals, normals_dev, bytes, hipMemcpyDeviceToDevice, stream));
    return g;
}

// The tables both creations take from the description as they are, and the per-scene rules behind a creation.
void upload_tables(DevScene& s, const RodentSceneDesc* d) {
    const bool textured = d->num_textures > 0;
    s.dev.vertices = upload(s.allocs, d->vertices, 4 * (size_t)d->num_vertices);
    s.dev.normals = upload(s.allocs, d->normals, 4 * (size_t)d->num_vertices);
    s.dev.face_normals = upload(s.allocs, d->face_normals, 4 * (size_t)d->num_tris);
    s.dev.indices = upload(s.allocs, d->indices, 4 * (size_t)d->num_tris);
    s.dev.materials = upload(s.allocs, d->materials, (size_t)d->num_materials);
    s.dev.light_ids = upload(s.allocs, d->light_ids, (size_t)d->num_tris);
    s.dev.texcoords = upload(s.allocs, d->texcoords, textured ? 4 * (size_t)d->num_vertices : 0);
    s.dev.textures = upload(s.allocs, d->textures, textured ? (size_t)d->num_textures : 0);
    s.dev.texels = upload(s.allocs, d->texels, textured ? (size_t)d->num_texels : 0);
}
void resolve_options(RenderDevice& r) { r.mapping = resolve_mapping(r); r.trace_persistent = resolve_trace(r); resolve_refill(r); }

// The checks of a description's tables that both creations make, each on one entry (every index the kernels follow is checked once on
// the host tables: a corrupt scene must not become an out-of-bounds read in k_shade / trace_one).  The creations differ in the order of
// their checks and in what a failure becomes (abort with a text / a return code), so each keeps its own short loop over these.
bool textures_exist(const RodentMaterial& m, int32_t num_textures) {
    return m.tex_kd >= 0 && m.tex_kd <= num_textures && m.tex_ks >= 0 && m.tex_ks <= num_textures;
}
bool texture_in_pool(const RodentTexture& t, uint32_t num_texels) {
    return t.width > 0 && t.height > 0 && (uint64_t)t.offset + (uint64_t)t.width * (uint64_t)t.height <= num_texels;
}
// triangle t's indices: 0 = in range, 1 = a vertex index is not, 2 = the material index is not
int bad_index(const RodentSceneDesc* d, size_t t) {
    for (int k = 0; k < 3; k++) if ((uint32_t)d->indices[4 * t + k] >= (uint32_t)d->num_vertices) return 1;
    return (uint32_t)d->indices[4 * t + 3] >= (uint32_t)d->num_materials ? 2 : 0;
}
// an emitter's triangles are looked up in the light table by the shader (on_hit: sc.lights[light_ids[prim]]): the entry must exist, in
// the range [first_light, first_light + num_lights) that is the triangle's own (the whole table, or its object's)
bool emitter_without_light(const RodentSceneDesc* d, size_t t, int32_t first_light, int32_t num_lights) {
    return d->materials[d->indices[4 * t + 3]].emissive && (d->light_ids[t] < first_light || d->light_ids[t] >= first_light + num_lights);
}

// Top-of-tree image of the stream traversal kernels (record layout: traversal_device.h build_top_image), `capacity` records of 16 words:
// breadth first from the root; a child that got a slot is a link (kLdsTag + byte offset of its record), the others keep their ids.
std::vector<int32_t> build_image(const Node2* nodes, int capacity) {
    std::vector<int32_t> image((size_t)capacity * 16, 0), slots{1};
    for (size_t k = 0; k < slots.size(); k++) {
        const Node2& nd = nodes[slots[k] - 1];
        int32_t* rec = image.data() + 16 * k;
        memcpy(rec, nd.bounds, 12 * sizeof(float));
        for (int j = 0; j < 2; j++) {
            const int32_t c = nd.child[j];
            rec[12 + j] = c;
            if (c > 0 && (int)slots.size() < capacity) { rec[12 + j] = kLdsTag + (int32_t)slots.size() * (int32_t)sizeof(Node2);
                slots.push_back(c); }
        }
        rec[14] = slots[k];
    }
    return image;
}

// SceneDev::tri_shade records (12 floats per triangle): the face normal, then the three corners' vertex normals, gathered.
std::vector<float> tri_shade(const float* face_normals, const float* normals, const int32_t* indices, int32_t num_tris) {
    std::vector<float> rec(12 * (size_t)num_tris);
    for (int32_t t = 0; t < num_tris; t++) {
        float* o = rec.data() + 12 * (size_t)t;
        const float* fn = face_normals + 4 * (size_t)t;
        o[0] = fn[0]; o[1] = fn[1]; o[2] = fn[2];
        for (int k = 0; k < 3; k++) {
            const float* n = normals + 4 * (size_t)indices[4 * (size_t)t + k];
            o[3 + 3 * k] = n[0]; o[4 + 3 * k] = n[1]; o[5 + 3 * k] = n[2];
        }
    }
    return rec;
}

// SceneDev::tri_shade and ::tri_tex of the tables in `d` (host), uploaded into `s`
void upload_shading_records(DevScene& s, const RodentSceneDesc* d, bool textured) {
    // SceneDev::tri_shade: per triangle face normal + its three vertex normals, gathered (RODENT_HIP_TRI_SHADE=0: not built, the shader
    // goes through indices -> normals)
    static const bool on = [] { const char* e = getenv("RODENT_HIP_TRI_SHADE"); return !e || atoi(e) != 0; }();
    s.dev.tri_shade = nullptr;
    if (on && d->num_tris > 0) {
        const std::vector<float> rec = tri_shade(d->face_normals, d->normals, d->indices, d->num_tris);
        s.dev.tri_shade = reinterpret_cast<const float4*>(upload(s.allocs, rec.data(), rec.size()));
    }
    s.dev.tri_tex = nullptr;
    // SceneDev::tri_tex: the corners' texture coordinates, for resolve_material
    if (on && textured && d->num_tris > 0) {
        std::vector<float> tc(6 * (size_t)d->num_tris);
        for (int32_t t = 0; t < d->num_tris; t++)
            for (int k = 0; k < 3; k++) {
                const float* c = d->texcoords + 4 * (size_t)d->indices[4 * (size_t)t + k];
                tc[6 * (size_t)t + 2 * k] = c[0]; tc[6 * (size_t)t + 2 * k + 1] = c[1];
            }
        s.dev.tri_tex = upload(s.allocs, tc.data(), tc.size());
    }
}

// ---- The flat scene: creation, the lists its device refit needs ----
// rodent_hip_scene_create and rodent_hip_scene_create_device_bvh(_opt / _split): build = NULL uploads the caller's hierarchy
// (desc->nodes / tris), build options build one on the device from the vertices and indices just uploaded (bvh_build.hip; with
// `split`, over pre-split references) and takes a host copy of it; from there on both are the same code: checks, LDS images, per-scene
// rules.
void scene_create(int32_t dev, const RodentSceneDesc* d, const RodentBuildOptions* build, const RodentSplitOptions* split = nullptr,
                  const RodentPlocOptions* ploc = nullptr) {
    RenderDevice& r = rdev(dev);
    rodent_hip_scene_destroy(dev);
    HIP_CHECK(hipSetDevice(dev));
    DevScene& s = r.scene;
    const bool textured = d->num_textures > 0;
    if (textured && (!d->texcoords || !d->textures || !d->texels)) {
        fprintf(stderr, "rodent_hip: scene with textures but without texture data\n"); abort(); }
    upload_tables(s, d);
    RodentSceneDesc built_desc;                 // d with the device-built hierarchy (host copy) in place of the caller's
    std::vector<Node2> built_nodes;
    std::vector<Tri1> built_tris;
    {   // nodes and triangles in ONE allocation: k_trace_refill addresses both from one base with 32-bit offsets (joint_fetch_off)
        // (a device-built hierarchy: room for the builder's max(1, refs - 1) nodes, then its refs triangles; the builder's scratch and
        // info words.  Unsplit: refs = n, 4 info words, info[4] keeps n)
        int32_t refs = d->num_tris, info_words = RODENT_BUILD_INFO_WORDS;
        int64_t scratch_bytes = build ? rodent_hip_build_opt_scratch_bytes(d->num_tris, build) : 0;
        if (split) {
            refs = (int32_t)rodent_hip_build_split_max_refs(d->num_tris, split);
            scratch_bytes = rodent_hip_build_split_scratch_bytes(d->num_tris, build, split);
            info_words = RODENT_BUILD_SPLIT_INFO_WORDS;
        }
        if (ploc) {                                      // the PLOC topology stage, with or without the split front: 8 info words
            scratch_bytes = rodent_hip_build_ploc_scratch_bytes(d->num_tris, build, split, ploc);
            info_words = RODENT_BUILD_SPLIT_INFO_WORDS;
        }
        const size_t node_bytes = sizeof(Node2) * (size_t)(build ? std::max(1, refs - 1) : d->num_nodes);
        const size_t tri_bytes = sizeof(Tri1) * (size_t)(build ? refs : d->num_bvh_tris);
        char* const bvh = device_alloc<char>(s.allocs, node_bytes + tri_bytes);
        s.dev.nodes = reinterpret_cast<const Node2*>(bvh);
        s.dev.tris = reinterpret_cast<const Tri1*>(bvh + node_bytes);
        if (build) {
            int32_t info[RODENT_BUILD_SPLIT_INFO_WORDS] = {0, 0, 0, 0, d->num_tris, 0, 0, 0};
            BuildScratch work(scratch_bytes, info_words);
            Node2* out_nodes = reinterpret_cast<Node2*>(bvh);
            Tri1* out_tris = reinterpret_cast<Tri1*>(bvh + node_bytes);
            const int32_t rc = ploc
                ? rodent_hip_build_bvh2_tri1_ploc(dev, s.dev.vertices, d->num_vertices, s.dev.indices, d->num_tris, build, split, ploc,
                                                  out_nodes, out_tris, work.scratch, work.info_dev, nullptr)
                : split
                ? rodent_hip_build_bvh2_tri1_split(dev, s.dev.vertices, d->num_vertices, s.dev.indices, d->num_tris, build, split,
                                                   out_nodes, out_tris, work.scratch, work.info_dev, nullptr)
                : rodent_hip_build_bvh2_tri1_opt(dev, s.dev.vertices, d->num_vertices, s.dev.indices, d->num_tris, build, out_nodes,
                                                 out_tris, work.scratch, work.info_dev, nullptr);
            const int32_t flags = work.finish(rc, info);
            if (rc != RODENT_BUILD_OK) { fprintf(stderr, "rodent_hip: device BVH build refused (%d)\n", rc); abort(); }
            if (flags) { fprintf(stderr, "rodent_hip: invalid scene: device BVH build flagged the mesh (%d)\n", flags); abort(); }
            built_nodes.resize(info[0]);
            built_tris.resize(info[4]);                  // the references (= num_tris unsplit)
            HIP_CHECK(hipMemcpy(built_nodes.data(), bvh, sizeof(Node2) * built_nodes.size(), hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(built_tris.data(), bvh + node_bytes, sizeof(Tri1) * built_tris.size(), hipMemcpyDeviceToHost));
            built_desc = *d;
            built_desc.nodes = built_nodes.data(); built_desc.num_nodes = info[0];
            built_desc.tris = built_tris.data(); built_desc.num_bvh_tris = info[4];
            d = &built_desc;
        } else {
            if (node_bytes) HIP_CHECK(hipMemcpy(bvh, d->nodes, node_bytes, hipMemcpyHostToDevice));
            if (tri_bytes) HIP_CHECK(hipMemcpy(bvh + node_bytes, d->tris, tri_bytes, hipMemcpyHostToDevice));
        }
        // tri_delta: bytes from the record a node id of 0 would have to triangle 0; 0 = not addressable this way (offsets beyond 32 bits,
        // or an index beyond the 24-bit multiply)
        const unsigned long long delta = sizeof(Node2) + node_bytes, end = delta + tri_bytes;
        s.tri_delta = (end < (1ull << 32) && d->num_nodes < (1 << 24) - 1 && d->num_bvh_tris < (1 << 24)) ? (unsigned)delta : 0u;
    }
    s.dev.lights = upload(s.allocs, d->lights, (size_t)d->num_lights);
    for (int32_t k = 0; k < d->num_materials; k++)
        if (!textures_exist(d->materials[k], d->num_textures)) {
            fprintf(stderr, "rodent_hip: material %d refers to a texture that does not exist\n", k); abort(); }
    auto invalid = [](const char* what) { fprintf(stderr, "rodent_hip: invalid scene: %s\n", what); abort(); };
    if (d->num_vertices <= 0 || d->num_tris <= 0 || d->num_nodes <= 0 || d->num_bvh_tris <= 0 || d->num_materials <= 0
        || d->num_lights < 0) invalid("empty table");
    for (int32_t t = 0; t < d->num_tris; t++) {
        if (const int bad = bad_index(d, (size_t)t)) invalid(bad == 1 ? "vertex index out of range" : "material index out of range");
        if (d->light_ids[t] < 0 || (d->light_ids[t] > 0 && d->light_ids[t] >= d->num_lights)) invalid("light id out of range");
        if (emitter_without_light(d, (size_t)t, 0, d->num_lights)) invalid("emissive triangle without an entry in the light table");
    }
    for (int32_t k = 0; k < d->num_nodes; k++)
        for (int j = 0; j < 2; j++) {
            const int32_t c = d->nodes[k].child[j];
            if ((c > 0 && c > d->num_nodes) || (c < 0 && ~c >= d->num_bvh_tris)) invalid("BVH child id out of range");
        }
    if (d->tris[d->num_bvh_tris - 1].prim_id >= 0) invalid("the last BVH triangle lacks the end-of-leaf bit");
    for (int32_t k = 0; k < d->num_bvh_tris; k++)
        if ((d->tris[k].prim_id & 0x7FFFFFFF) >= d->num_tris
            || (uint32_t)d->tris[k].geom_id
            >= (uint32_t)d->num_materials) invalid("BVH triangle refers to a primitive or material that does not exist");
    for (int32_t k = 0; k < d->num_textures; k++)
        if (!texture_in_pool(d->textures[k], d->num_texels)) invalid("texture outside the texel pool");
    s.dev.num_tris = d->num_tris; s.dev.num_materials = d->num_materials; s.dev.num_lights = d->num_lights;
    // top-of-tree images of the stream traversal kernels (build_image)
    for (const int capacity : {kSceneTopNodes, kPersistTopNodes}) {
        const std::vector<int32_t> image = build_image(d->nodes, capacity);
        (capacity == kSceneTopNodes ? s.dev.top_image : s.dev.top_image_large) =
            reinterpret_cast<const int4*>(upload(s.allocs, image.data(), image.size()));
    }
    upload_shading_records(s, d, textured);
    s.num_nodes = d->num_nodes;
    s.num_bvh_tris = d->num_bvh_tris;
    s.num_vertices = d->num_vertices;
    s.loaded = true;
    resolve_options(r);
}

// The host lists a device update works from, over the objects' triangle and light `ranges` (the whole scene is one range): made from
// tables that never change under an update (indices, light ids, materials: read back here), so they hold for the scene's or the set's life.
struct RefitLists {
    std::vector<int2> lights;                  // {light, the lowest emissive triangle of its range that names it}: by range, then by light
    // with `smooth`: the vertices the ranges' triangles name, ascending, and for vertex verts[j] the corners of ALL triangles that name
    // it, corner_tri[corner_first[j] .. corner_first[j + 1]), ascending (triangle, corner) -- a triangle that names it twice is there twice
    std::vector<int> verts, corner_first, corner_tri;
};
RefitLists refit_lists(const DevScene& s, const std::vector<RodentObjectRange>& ranges, bool smooth) {
    const size_t nv = (size_t)s.num_vertices, nt = (size_t)s.dev.num_tris;
    std::vector<int32_t> indices(4 * nt), light_ids(nt);
    std::vector<RodentMaterial> materials((size_t)s.dev.num_materials);
    HIP_CHECK(hipMemcpy(indices.data(), s.dev.indices, sizeof(int32_t) * indices.size(), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(light_ids.data(), s.dev.light_ids, sizeof(int32_t) * nt, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(materials.data(), s.dev.materials, sizeof(RodentMaterial) * materials.size(), hipMemcpyDeviceToHost));
    RefitLists out;
    for (const RodentObjectRange& g : ranges) {
        std::vector<int> tri((size_t)g.num_lights, -1);
        for (int32_t t = g.first_tri; t < g.first_tri + g.num_tris; t++) {
            const int32_t k = light_ids[t] - g.first_light;
            if (materials[indices[4 * (size_t)t + 3]].emissive && k >= 0 && k < g.num_lights && tri[k] < 0) tri[k] = t;
        }
        for (int32_t k = 0; k < g.num_lights; k++) if (tri[k] >= 0) out.lights.push_back(make_int2(g.first_light + k, tri[k]));
    }
    if (!smooth) return out;
    std::vector<int> slot(nv, -1);
    for (const RodentObjectRange& g : ranges)
        for (size_t c = 4 * (size_t)g.first_tri; c < 4 * (size_t)(g.first_tri + g.num_tris); c++) if (c % 4 != 3) slot[indices[c]] = 0;
    for (size_t v = 0; v < nv; v++) if (slot[v] == 0) { slot[v] = (int)out.verts.size(); out.verts.push_back((int)v); }
    std::vector<int> first(out.verts.size() + 1, 0);
    for (size_t t = 0; t < nt; t++) for (int k = 0; k < 3; k++) { const int j = slot[indices[4 * t + k]]; if (j >= 0) first[(size_t)j + 1]++; }
    for (size_t j = 0; j < out.verts.size(); j++) first[j + 1] += first[j];
    std::vector<int> next(first.begin(), first.end() - 1), tri((size_t)first.back());
    for (size_t t = 0; t < nt; t++) for (int k = 0; k < 3; k++) { const int j = slot[indices[4 * t + k]]; if (j >= 0) tri[next[j]++] = (int)t; }
    out.corner_first = std::move(first); out.corner_tri = std::move(tri);
    return out;
}

// rodent_hip_scene_refit_prepare: one-time and synchronous.  The lists of the whole scene as one range, in this entry's own layout:
// light_tri is indexed by light (-1: none), corner_first runs over ALL vertices.
void refit_prepare(RenderDevice& r, bool smooth_normals) {
    DevScene& s = r.scene;
    HIP_CHECK(hipSetDevice(r.dev));
    const bool corners = smooth_normals && !s.corner_first;
    if (s.refit_info && !corners) return;
    const RefitLists lists = refit_lists(s, {RodentObjectRange{0, s.dev.num_tris, 0, s.dev.num_lights}}, corners);
    if (!s.refit_info) {
        s.refit_scratch = alloc_scratch_info(s.allocs, rodent_hip_refit_scratch_bytes(s.num_nodes, s.num_bvh_tris), RODENT_BUILD_INFO_WORDS,
                                             s.refit_info);
        HIP_CHECK(hipMemset(s.refit_info, 0, 4 * RODENT_BUILD_INFO_WORDS));
        std::vector<int> light_tri((size_t)s.dev.num_lights, -1);
        for (const int2& bound : lists.lights) light_tri[bound.x] = bound.y;
        s.light_tri = upload(s.allocs, light_tri.data(), light_tri.size());
    }
    if (corners) {
        std::vector<int> first((size_t)s.num_vertices + 1, 0);      // (a vertex no triangle names has an empty list)
        for (size_t v = 0, j = 0; v + 1 < first.size(); v++) {
            if (j < lists.verts.size() && lists.verts[j] == (int)v) j++;
            first[v + 1] = lists.corner_first[j];
        }
        s.corner_tri = upload(s.allocs, lists.corner_tri.data(), lists.corner_tri.size());
        s.corner_first = upload(s.allocs, first.data(), first.size());
    }
}

// ---- Which scene an entry works on ----
DevScene& loaded_scene(int32_t dev, const char* entry) {
    DevScene& s = rdev(dev).scene;
    if (!s.loaded) {
        fprintf(stderr, "rodent_hip: %s: no scene loaded on device %d (call rodent_hip_scene_create)\n", entry, dev); abort(); }
    return s;
}
// the refit entries: an instanced scene has no single hierarchy to refit (its instances move with rodent_hip_scene_set_transforms)
DevScene& flat_scene(int32_t dev, const char* entry) {
    DevScene& s = loaded_scene(dev, entry);
    if (s.instanced) { fprintf(stderr, "rodent_hip: %s: the scene on device %d is instanced (move its instances with "
        "rodent_hip_scene_set_transforms)\n", entry, dev); abort(); }
    // ... nor has a deforming scene one that a frame traces (its keys move with rodent_hip_scene_set_motion_keys)
    if (s.deforming) { fprintf(stderr, "rodent_hip: %s: the scene on device %d is a deforming one (move its keys with "
        "rodent_hip_scene_set_motion_keys)\n", entry, dev); abort(); }
    return s;
}
DevScene& deforming_scene(int32_t dev, const char* entry) {
    DevScene& s = loaded_scene(dev, entry);
    if (!s.deforming) { fprintf(stderr, "rodent_hip: %s: the scene on device %d is no deforming one "
        "(rodent_hip_scene_create_deforming)\n", entry, dev); abort(); }
    return s;
}
// (the static-instance entries: a moving scene is "no instanced scene" to them)
DevScene& instanced_scene(int32_t dev, const char* entry) {
    DevScene& s = loaded_scene(dev, entry);
    if (!s.instanced || s.motion) {
        fprintf(stderr, "rodent_hip: %s: the scene on device %d is not instanced (rodent_hip_scene_create_instanced)\n", entry, dev);
        abort(); }
    return s;
}
DevScene& motion_scene(int32_t dev, const char* entry) {
    DevScene& s = loaded_scene(dev, entry);
    if (!s.motion) { fprintf(stderr, "rodent_hip: %s: the scene on device %d has no moving instances (rodent_hip_scene_create_motion)\n",
        entry, dev); abort(); }
    return s;
}

// ---- The instanced and the moving scene ----
// The tables an instanced scene derives from its matrices, enqueued on `stream`: the TLAS and the instance array, slot_of, the world
// lights (rodent_hip_scene_create_instanced, rodent_hip_scene_set_transforms).  Returns rodent_hip_build_tlas's status.
// A moving scene: rodent_hip_build_motion_tlas and the motion forms of the two kernels (the world lights from M0).
int32_t derive_instanced(int32_t dev, DevScene& s, hipStream_t stream) {
    if (s.motion) {
        const int32_t rc = rodent_hip_build_motion_tlas(dev, s.dev.nodes, s.objects, s.num_objects, s.motion_descs, s.num_instances, 1,
                                                        s.tlas_nodes, s.motion_instances, s.tlas_scratch, s.tlas_info, stream);
        if (rc != RODENT_BUILD_OK) return rc;
        hipLaunchKernelGGL(k_motion_slot_of, blocks(s.num_instances), dim3(kBlock), 0, stream, s.motion_instances, s.num_instances,
                           s.slot_of);
        hipLaunchKernelGGL(k_motion_world_lights, blocks(s.dev.num_lights), dim3(kBlock), 0, stream, s.motion_descs, s.light_owner,
                           s.bases, s.object_lights, s.dev.num_lights, s.world_lights);
        HIP_CHECK(hipGetLastError());
        return rc;
    }
    const int32_t rc = rodent_hip_build_tlas(dev, s.dev.nodes, s.objects, s.num_objects, s.descs, s.num_instances, 1, s.tlas_nodes,
                                             s.instances, s.tlas_scratch, s.tlas_info, stream);
    if (rc != RODENT_BUILD_OK) return rc;
    hipLaunchKernelGGL(k_slot_of, blocks(s.num_instances), dim3(kBlock), 0, stream, s.instances, s.num_instances, s.slot_of);
    hipLaunchKernelGGL(k_world_lights, blocks(s.dev.num_lights), dim3(kBlock), 0, stream, s.descs, s.instances, s.slot_of, s.light_owner,
                       s.bases, s.object_lights, s.dev.num_lights, s.world_lights);
    HIP_CHECK(hipGetLastError());
    return rc;
}
// ... inside an update (a move, a deformation): a refusal is the caller's error
void rederive_instanced(int32_t dev, DevScene& s, hipStream_t stream) {
    const int32_t rc = derive_instanced(dev, s, stream);
    if (rc != RODENT_BUILD_OK) { fprintf(stderr, "rodent_hip: top-level rebuild refused (%d)\n", rc); abort(); }
}

// rodent_hip_scene_create_instanced (Desc = RodentInstanceDesc) and rodent_hip_scene_create_motion (RodentMotionInstanceDesc): one
// creation; what differs is the record types, the top-level builder behind derive_instanced and the moving scene's one more refusal.
template <typename Desc>
int32_t create_instanced_scene(int32_t dev, const RodentSceneDesc* d, const RodentObjectRange* objects, int32_t num_objects,
                               const Desc* instances, int32_t num_instances, const RodentBuildOptions* opt_) {
    constexpr bool kMotion = std::is_same<Desc, RodentMotionInstanceDesc>::value;
    const RodentBuildOptions default_opt{2, 0, RODENT_BUILD_DEFAULT_NODE_COST, RODENT_BUILD_DEFAULT_TRI_COST};
    const RodentBuildOptions* opt = opt_ ? opt_ : &default_opt;
    // ---- the refusals: all on the host tables, before anything is enqueued or the current scene touched ----
    if (!d || !objects || !instances || num_objects < 1 || num_instances < 1 || num_instances > RODENT_TLAS_MAX_INSTANCES) return
        RODENT_SCENE_ERR_COUNTS;
    const bool textured = d->num_textures > 0;
    if (d->nodes || d->tris || d->num_nodes || d->num_bvh_tris || !d->vertices || !d->normals || !d->face_normals || !d->indices
        || !d->materials || !d->light_ids || d->num_vertices < 1 || d->num_tris < 1 || d->num_tris > RODENT_BUILD_MAX_TRIS
        || d->num_materials < 1 || d->num_lights < 0 || (d->num_lights > 0 && !d->lights) || d->num_textures < 0
        || (textured && (!d->texcoords || !d->textures || !d->texels))) return RODENT_SCENE_ERR_COUNTS;
    if (rodent_hip_build_opt_scratch_bytes(1, opt) < 0) return RODENT_SCENE_ERR_OPTIONS;
    {
        int64_t tri = 0, light = 0;
        for (int32_t o = 0; o < num_objects; o++) {
            const RodentObjectRange& r = objects[o];
            if (r.first_tri != tri || r.num_tris < 1 || r.first_light != light || r.num_lights < 0) return RODENT_SCENE_ERR_RANGES;
            tri += r.num_tris; light += r.num_lights;
            if (tri > d->num_tris || light > d->num_lights) return RODENT_SCENE_ERR_RANGES;
        }
        if (tri != d->num_tris || light != d->num_lights) return RODENT_SCENE_ERR_RANGES;
    }
    for (int32_t k = 0; k < d->num_materials; k++) if (!textures_exist(d->materials[k], d->num_textures)) return RODENT_SCENE_ERR_TABLE;
    for (int32_t k = 0; k < d->num_textures; k++) if (!texture_in_pool(d->textures[k], d->num_texels)) return RODENT_SCENE_ERR_TABLE;
    for (int32_t o = 0; o < num_objects; o++) {
        const RodentObjectRange& r = objects[o];
        for (int32_t t = r.first_tri; t < r.first_tri + r.num_tris; t++) {
            if (bad_index(d, (size_t)t)) return RODENT_SCENE_ERR_TABLE;
            // (the entry must be the object's own)
            if (emitter_without_light(d, (size_t)t, r.first_light, r.num_lights)) return RODENT_SCENE_ERR_LIGHT;
        }
    }
    int64_t world_lights = 0;
    for (int32_t k = 0; k < num_instances; k++) {
        if (instances[k].object < 0 || instances[k].object >= num_objects) return RODENT_SCENE_ERR_OBJECT;
        world_lights += objects[instances[k].object].num_lights;
    }
    if (world_lights < 1) return RODENT_SCENE_ERR_NO_LIGHT;
    if (world_lights > 0x7FFFFFFF) return RODENT_SCENE_ERR_COUNTS;
    if constexpr (kMotion)                               // lights stay static: an emitter's two keys are equal byte for byte
        for (int32_t k = 0; k < num_instances; k++)
            if (objects[instances[k].object].num_lights > 0
                && std::memcmp(instances[k].object_to_world0, instances[k].object_to_world1, sizeof(float) * 12) != 0)
                return RODENT_SCENE_ERR_MOVING_LIGHT;

    // ---- from here on the device's scene is the new one, or none ----
    RenderDevice& r = rdev(dev);
    rodent_hip_scene_destroy(dev);
    HIP_CHECK(hipSetDevice(dev));
    r.create_flags = 0;
    DevScene& s = r.scene;
    upload_tables(s, d);
    s.object_lights = upload(s.allocs, d->lights, (size_t)d->num_lights);
    const auto fail = [&](int32_t flags) { rodent_hip_scene_destroy(dev); r.create_flags = flags; return RODENT_SCENE_ERR_DEVICE; };
    // every object's hierarchy, built into a block of its own (its node count is known only afterwards), then packed
    std::vector<RodentObject> table((size_t)num_objects);
    std::vector<char*> built((size_t)num_objects, nullptr);
    const auto free_built = [&] { for (char* b : built) if (b) HIP_CHECK(hipFree(b)); };
    int64_t total_nodes = 0;
    // Without treelet passes: ALL objects by one rodent_hip_build_objects call in pack mode (one launch list whatever their number)
    // into a temporary block; the table, the per-object info words and the call's come back in one copy.
    std::vector<RodentRefitRange> plan((size_t)num_objects);
    char* forest = nullptr;                              // nodes (room for max(1, n - 1) each), then, 256-byte aligned, the triangles
    size_t forest_tris = 0;
    int64_t forest_scratch = -1;
    if (opt->treelet_passes == 0) {
        std::vector<int32_t> ids((size_t)num_objects), first((size_t)num_objects), count((size_t)num_objects);
        for (int32_t o = 0; o < num_objects; o++) { ids[o] = o; first[o] = objects[o].first_tri; count[o] = objects[o].num_tris; }
        int32_t totals[2] = {};
        forest_scratch = rodent_hip_build_objects_plan(ids.data(), first.data(), count.data(), num_objects, plan.data(), totals);
    }
    if (forest_scratch >= 0) {
        size_t room = 0;
        for (int32_t o = 0; o < num_objects; o++) room += (size_t)std::max(1, objects[o].num_tris - 1);
        forest_tris = (sizeof(Node2) * room + 255) / 256 * 256;
        const size_t range_bytes = (sizeof(RodentRefitRange) * (size_t)num_objects + 255) / 256 * 256;
        const size_t result_words = 8 * (size_t)num_objects + RODENT_BUILD_INFO_WORDS;    // table, object info, info
        char* work = nullptr;                            // scratch, the range table, the results
        HIP_CHECK(hipMalloc(&forest, forest_tris + sizeof(Tri1) * (size_t)d->num_tris));
        HIP_CHECK(hipMalloc(&work, (size_t)forest_scratch + range_bytes + 4 * result_words));
        RodentRefitRange* ranges_dev = reinterpret_cast<RodentRefitRange*>(work + forest_scratch);
        RodentObject* table_dev = reinterpret_cast<RodentObject*>(work + forest_scratch + range_bytes);
        int32_t* object_info_dev = reinterpret_cast<int32_t*>(table_dev + num_objects);
        int32_t* info_dev = object_info_dev + 4 * (size_t)num_objects;
        HIP_CHECK(hipMemcpy(ranges_dev, plan.data(), sizeof(RodentRefitRange) * (size_t)num_objects, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemset(table_dev, 0, 4 * result_words));
        const int32_t rc = rodent_hip_build_objects(dev, s.dev.vertices, d->num_vertices, s.dev.indices, d->num_tris, opt->max_leaf,
            RODENT_BUILD_OBJECTS_PACK, reinterpret_cast<Node2*>(forest), reinterpret_cast<Tri1*>(forest + forest_tris), table_dev,
            num_objects, ranges_dev, num_objects, d->num_tris, work, object_info_dev, info_dev, nullptr);
        std::vector<int32_t> result(result_words, 0);
        if (rc == RODENT_BUILD_OK) HIP_CHECK(hipMemcpy(result.data(), table_dev, 4 * result_words, hipMemcpyDeviceToHost));
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipFree(work));
        const int32_t* object_info = result.data() + 4 * (size_t)num_objects;
        int32_t bad = rc;
        for (int32_t o = 0; o < num_objects && !bad; o++) {      // the first flagged object in object order, as the loop reports it
            const int32_t nodes_o = object_info[4 * o], n = objects[o].num_tris;
            bad = object_info[4 * o + 2] ? object_info[4 * o + 2] : nodes_o < 1 || nodes_o > std::max(1, n - 1) ? (int32_t)0x80000000u : 0;
        }
        if (!bad) bad = object_info[4 * (size_t)num_objects + 2];
        if (bad) { HIP_CHECK(hipFree(forest)); return fail(bad); }
        for (int32_t o = 0; o < num_objects; o++) {
            std::memcpy(&table[o], result.data() + 4 * (size_t)o, sizeof(RodentObject));
            total_nodes += table[o].num_nodes;
        }
    }
    for (int32_t o = 0; o < num_objects && !forest; o++) {
        const int32_t n = objects[o].num_tris;
        const size_t node_bytes = sizeof(Node2) * (size_t)std::max(1, n - 1), tri_bytes = sizeof(Tri1) * (size_t)n;
        HIP_CHECK(hipMalloc(&built[o], node_bytes + tri_bytes));
        BuildScratch work(rodent_hip_build_opt_scratch_bytes(n, opt), RODENT_BUILD_INFO_WORDS);
        int32_t info[RODENT_BUILD_INFO_WORDS] = {};
        const int32_t rc = rodent_hip_build_bvh2_tri1_opt(dev, s.dev.vertices, d->num_vertices,
            s.dev.indices + 4 * (size_t)objects[o].first_tri, n, opt, reinterpret_cast<Node2*>(built[o]),
            reinterpret_cast<Tri1*>(built[o] + node_bytes), work.scratch, work.info_dev, nullptr);
        if (const int32_t bad = work.finish(rc, info, 1, std::max(1, n - 1))) { free_built(); return fail(bad); }
        table[o] = RodentObject{(int32_t)total_nodes, objects[o].first_tri, info[0], n};
        total_nodes += info[0];
    }
    {   // one allocation: all nodes, then, 256-byte aligned, all triangles (instances.pack_objects)
        const size_t node_bytes = sizeof(Node2) * (size_t)total_nodes, tri_start = (node_bytes + 255) / 256 * 256;
        char* const bvh = device_alloc<char>(s.allocs, tri_start + sizeof(Tri1) * (size_t)d->num_tris);
        if (forest) {                                            // packed tight already: the nodes, then the triangles
            HIP_CHECK(hipMemcpy(bvh, forest, node_bytes, hipMemcpyDeviceToDevice));
            HIP_CHECK(hipMemcpy(bvh + tri_start, forest + forest_tris, sizeof(Tri1) * (size_t)d->num_tris, hipMemcpyDeviceToDevice));
        }
        for (int32_t o = 0; o < num_objects && !forest; o++) {
            const size_t from_tris = sizeof(Node2) * (size_t)std::max(1, objects[o].num_tris - 1);
            HIP_CHECK(hipMemcpy(bvh + sizeof(Node2) * (size_t)table[o].node_offset, built[o], sizeof(Node2) * (size_t)table[o].num_nodes,
                                hipMemcpyDeviceToDevice));
            HIP_CHECK(hipMemcpy(bvh + tri_start + sizeof(Tri1) * (size_t)table[o].tri_offset, built[o] + from_tris,
                                sizeof(Tri1) * (size_t)table[o].num_tris, hipMemcpyDeviceToDevice));
        }
        HIP_CHECK(hipDeviceSynchronize());
        free_built();
        if (forest) HIP_CHECK(hipFree(forest));
        s.dev.nodes = reinterpret_cast<const Node2*>(bvh);
        s.dev.tris = reinterpret_cast<const Tri1*>(bvh + tri_start);
    }
    s.objects = upload(s.allocs, table.data(), table.size());
    s.object_table = table;
    s.object_ranges.assign(objects, objects + num_objects);
    // descriptors (ids = indices), bases and light owners: fixed for the scene's life
    std::vector<Desc> descs(instances, instances + num_instances);
    std::vector<int2> bases((size_t)num_instances);
    std::vector<int> owner((size_t)world_lights);
    int32_t light_base = 0;
    for (int32_t k = 0; k < num_instances; k++) {
        descs[k].instance_id = k;
        for (int32_t& word : descs[k].pad) word = 0;
        const RodentObjectRange& o = objects[descs[k].object];
        bases[k] = make_int2(o.first_tri, light_base - o.first_light);
        for (int32_t j = 0; j < o.num_lights; j++) owner[(size_t)light_base + j] = k;
        light_base += o.num_lights;
    }
    s.motion = kMotion;
    if constexpr (kMotion) s.motion_descs = upload(s.allocs, descs.data(), descs.size());
    else s.descs = upload(s.allocs, descs.data(), descs.size());
    s.bases = upload(s.allocs, bases.data(), bases.size());
    s.light_owner = upload(s.allocs, owner.data(), owner.size());
    s.tlas_nodes = device_alloc<Node2>(s.allocs, (size_t)std::max(1, num_instances - 1), true);
    if constexpr (kMotion) s.motion_instances = device_alloc<RodentMotionInstance>(s.allocs, (size_t)num_instances, true);
    else s.instances = device_alloc<RodentInstance>(s.allocs, (size_t)num_instances, true);
    s.slot_of = device_alloc<int>(s.allocs, (size_t)num_instances, true);
    s.world_lights = device_alloc<RodentLight>(s.allocs, (size_t)world_lights, true);
    s.tlas_scratch = device_alloc<char>(s.allocs, (size_t)std::max<int64_t>(
        kMotion ? rodent_hip_motion_tlas_scratch_bytes(num_instances) : rodent_hip_tlas_scratch_bytes(num_instances), 0), true);
    s.tlas_info = device_alloc<int32_t>(s.allocs, RODENT_BUILD_INFO_WORDS, true);
    s.num_instances = num_instances; s.num_objects = num_objects; s.num_object_lights = d->num_lights;
    s.dev.lights = s.world_lights;
    s.dev.num_tris = d->num_tris; s.dev.num_materials = d->num_materials; s.dev.num_lights = (int32_t)world_lights;
    s.dev.top_image = s.dev.top_image_large = nullptr;         // the instanced kernels stage no image; no other kernel is launched
    HIP_CHECK(hipDeviceSynchronize());
    const int32_t rc = derive_instanced(dev, s, nullptr);
    int32_t info[RODENT_BUILD_INFO_WORDS] = {};
    HIP_CHECK(hipDeviceSynchronize());
    if (rc == RODENT_BUILD_OK) HIP_CHECK(hipMemcpy(info, s.tlas_info, sizeof(info), hipMemcpyDeviceToHost));
    if (rc != RODENT_BUILD_OK || info[2]) return fail(rc != RODENT_BUILD_OK ? rc : info[2]);
    upload_shading_records(s, d, textured);
    s.inst.tlas = s.tlas_nodes; s.inst.instances = s.instances; s.inst.bases = s.bases;
    s.num_nodes = (int)total_nodes; s.num_bvh_tris = d->num_tris; s.num_vertices = d->num_vertices; s.tri_delta = 0;
    s.loaded = true; s.instanced = true;
    ensure_ray_slots(r, 0);
    resolve_options(r);
    return RODENT_SCENE_OK;
}

// ---- The deforming scene ----
// The motion records of the scene's two keys, enqueued on `stream`: rodent_hip_build_motion_bvh2_tri1 over the static key-0 topology
// into the scene's records, with its scratch and info words (rodent_hip_scene_create_deforming, rodent_hip_scene_set_motion_keys).
int32_t derive_deforming(int32_t dev, DevScene& s, hipStream_t stream) {
    return rodent_hip_build_motion_bvh2_tri1(dev, s.dev.vertices, s.vertices1, s.num_vertices, s.dev.indices, s.dev.num_tris, s.dev.nodes,
                                             s.num_nodes, s.dev.tris, s.num_bvh_tris, s.motion_nodes, s.motion_tris, s.motion_scratch,
                                             s.motion_info, stream);
}

// rodent_hip_scene_create_deforming: the refusals on the host tables, then the flat creation's uploads, the topology from key 0 and the
// motion records; a device flag destroys what was half built.
int32_t create_deforming_scene(int32_t dev, const RodentSceneDesc* d, const float* vertices1, const float* normals1,
                               const RodentBuildOptions* opt_) {
    const RodentBuildOptions default_opt{2, 0, RODENT_BUILD_DEFAULT_NODE_COST, RODENT_BUILD_DEFAULT_TRI_COST};
    const RodentBuildOptions* opt = opt_ ? opt_ : &default_opt;
    // ---- the refusals: all on the host tables, before anything is enqueued or the current scene touched ----
    if (!d || !vertices1 || !normals1) return RODENT_SCENE_ERR_COUNTS;
    const bool textured = d->num_textures > 0;
    if (d->nodes || d->tris || d->num_nodes || d->num_bvh_tris || !d->vertices || !d->normals || !d->face_normals || !d->indices
        || !d->materials || !d->light_ids || d->num_vertices < 1 || d->num_tris < 1 || d->num_tris > RODENT_BUILD_MAX_TRIS
        || d->num_materials < 1 || d->num_lights < 0 || (d->num_lights > 0 && !d->lights) || d->num_textures < 0
        || (textured && (!d->texcoords || !d->textures || !d->texels))) return RODENT_SCENE_ERR_COUNTS;
    if (rodent_hip_build_opt_scratch_bytes(1, opt) < 0) return RODENT_SCENE_ERR_OPTIONS;
    for (int32_t k = 0; k < d->num_materials; k++) if (!textures_exist(d->materials[k], d->num_textures)) return RODENT_SCENE_ERR_TABLE;
    for (int32_t k = 0; k < d->num_textures; k++) if (!texture_in_pool(d->textures[k], d->num_texels)) return RODENT_SCENE_ERR_TABLE;
    for (int32_t t = 0; t < d->num_tris; t++) {
        if (bad_index(d, (size_t)t)) return RODENT_SCENE_ERR_TABLE;
        if (d->light_ids[t] < 0 || (d->light_ids[t] > 0 && d->light_ids[t] >= d->num_lights)) return RODENT_SCENE_ERR_TABLE;
        if (emitter_without_light(d, (size_t)t, 0, d->num_lights)) return RODENT_SCENE_ERR_LIGHT;
    }
    for (int32_t t = 0; t < d->num_tris; t++) {             // lights stay static: an emitter's corner rows are equal byte for byte
        if (!d->materials[d->indices[4 * (size_t)t + 3]].emissive) continue;
        for (int k = 0; k < 3; k++) {
            const size_t row = 4 * (size_t)d->indices[4 * (size_t)t + k];
            if (std::memcmp(d->vertices + row, vertices1 + row, sizeof(float) * 4) != 0) return RODENT_SCENE_ERR_MOVING_LIGHT;
        }
    }

    // ---- from here on the device's scene is the new one, or none ----
    RenderDevice& r = rdev(dev);
    rodent_hip_scene_destroy(dev);
    HIP_CHECK(hipSetDevice(dev));
    r.create_flags = 0;
    DevScene& s = r.scene;
    upload_tables(s, d);
    const size_t nv = (size_t)d->num_vertices, nt = (size_t)d->num_tris;
    s.vertices1 = upload(s.allocs, vertices1, 4 * nv);
    s.normals1 = upload(s.allocs, normals1, 4 * nv);
    s.face_normals1 = device_alloc<float>(s.allocs, 4 * nt, true);
    s.dev.lights = upload(s.allocs, d->lights, (size_t)d->num_lights);          // key 0's: lights stay static
    const auto fail = [&](int32_t flags) { rodent_hip_scene_destroy(dev); r.create_flags = flags; return RODENT_SCENE_ERR_DEVICE; };
    // the topology from key 0: nodes (room for max(1, n - 1)) and triangles in one allocation, as the flat creation lays them out
    const size_t node_bytes = sizeof(Node2) * std::max<size_t>(1, nt - 1);
    char* const bvh = device_alloc<char>(s.allocs, node_bytes + sizeof(Tri1) * nt);
    s.dev.nodes = reinterpret_cast<const Node2*>(bvh);
    s.dev.tris = reinterpret_cast<const Tri1*>(bvh + node_bytes);
    int32_t info[RODENT_BUILD_INFO_WORDS] = {};
    {
        BuildScratch work(rodent_hip_build_opt_scratch_bytes(d->num_tris, opt), RODENT_BUILD_INFO_WORDS);
        const int32_t rc = rodent_hip_build_bvh2_tri1_opt(dev, s.dev.vertices, d->num_vertices, s.dev.indices, d->num_tris, opt,
            reinterpret_cast<Node2*>(bvh), reinterpret_cast<Tri1*>(bvh + node_bytes), work.scratch, work.info_dev, nullptr);
        if (const int32_t bad = work.finish(rc, info, 1, (int32_t)std::max<size_t>(1, nt - 1))) return fail(bad);
    }
    s.num_nodes = info[0]; s.num_bvh_tris = d->num_tris; s.num_vertices = d->num_vertices; s.tri_delta = 0;
    s.dev.num_tris = d->num_tris; s.dev.num_materials = d->num_materials; s.dev.num_lights = d->num_lights;
    // the motion records over it, with the scratch and the info words every later rebuild uses
    s.motion_nodes = device_alloc<RodentMotionNode2>(s.allocs, (size_t)s.num_nodes, true);
    s.motion_tris = device_alloc<RodentMotionTri1>(s.allocs, nt, true);
    s.motion_scratch = alloc_scratch_info(s.allocs, rodent_hip_motion_bvh2_scratch_bytes(s.num_nodes, s.num_bvh_tris),
                                          RODENT_BUILD_INFO_WORDS, s.motion_info);
    HIP_CHECK(hipMemset(s.motion_info, 0, 4 * RODENT_BUILD_INFO_WORDS));
    HIP_CHECK(hipDeviceSynchronize());
    const int32_t rc = derive_deforming(dev, s, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    if (rc == RODENT_BUILD_OK) HIP_CHECK(hipMemcpy(info, s.motion_info, sizeof(info), hipMemcpyDeviceToHost));
    if (rc != RODENT_BUILD_OK) return fail(rc);
    if (info[2] || info[0] != s.num_nodes || info[3] != s.num_nodes) return fail(info[2] ? info[2] : (int32_t)0x80000000u);
    // no LDS top images and no gathered shading records: the deforming kernels stage no image, the shader gathers both keys' rows
    s.dev.top_image = s.dev.top_image_large = nullptr;
    s.dev.tri_shade = nullptr; s.dev.tri_tex = nullptr;
    s.loaded = true; s.deforming = true;
    refit_prepare(r, true);                                 // the incidence lists a NULL-normals rodent_hip_scene_set_motion_keys needs
    resolve_options(r);
    return RODENT_SCENE_OK;
}

} // namespace

extern "C" {

void rodent_hip_scene_destroy(int32_t dev) {
    RenderDevice& r = rdev(dev);
    HIP_CHECK(hipSetDevice(dev));
    HIP_CHECK(hipDeviceSynchronize());
    for (void* p : r.scene.allocs) HIP_CHECK(hipFree(p));
    for (void* p : r.scene.deform.allocs) HIP_CHECK(hipFree(p));
    if (r.scene.inst.ray_slots) HIP_CHECK(hipFree(r.scene.inst.ray_slots));
    r.scene = DevScene();
}

void rodent_hip_scene_create(int32_t dev, const RodentSceneDesc* d) { scene_create(dev, d, nullptr); }

void rodent_hip_scene_create_device_bvh(int32_t dev, const RodentSceneDesc* d, int32_t max_leaf) {
    const RodentBuildOptions opt{max_leaf, 0, RODENT_BUILD_DEFAULT_NODE_COST, RODENT_BUILD_DEFAULT_TRI_COST};
    rodent_hip_scene_create_device_bvh_opt(dev, d, &opt);
}

void rodent_hip_scene_create_device_bvh_opt(int32_t dev, const RodentSceneDesc* d, const RodentBuildOptions* opt) {
    if (!opt || rodent_hip_build_opt_scratch_bytes(1, opt) < 0 || d->num_tris < 1 || d->num_tris > RODENT_BUILD_MAX_TRIS
        || d->num_vertices < 1 || d->nodes || d->tris || d->num_nodes || d->num_bvh_tris) {
        fprintf(stderr, "rodent_hip: rodent_hip_scene_create_device_bvh: invalid arguments (max_leaf 1 ... 8, treelet passes 0 ... 3, "
                        "costs in (0, 1e6], 1 ... 2^25 triangles, "
                        "no hierarchy in the description)\n");
        abort();
    }
    scene_create(dev, d, opt);
}

void rodent_hip_scene_create_device_bvh_split(int32_t dev, const RodentSceneDesc* d, const RodentBuildOptions* opt,
                                              const RodentSplitOptions* split) {
    if (!opt || !split || rodent_hip_build_split_scratch_bytes(1, opt, split) < 0 || d->num_tris < 1
        || d->num_tris > RODENT_BUILD_MAX_TRIS || d->num_vertices < 1 || d->nodes || d->tris || d->num_nodes || d->num_bvh_tris) {
        fprintf(stderr, "rodent_hip: rodent_hip_scene_create_device_bvh_split: invalid arguments (max_leaf 1 ... 8, treelet passes "
                        "0 ... 3, costs in (0, 1e6], split budget 0 ... 4, max_pieces 1 ... 64, 1 ... 2^25 triangles, "
                        "no hierarchy in the description)\n");
        abort();
    }
    scene_create(dev, d, opt, split);
}

void rodent_hip_scene_create_device_bvh_ploc(int32_t dev, const RodentSceneDesc* d, const RodentBuildOptions* opt,
                                             const RodentSplitOptions* split, const RodentPlocOptions* ploc) {
    if (!opt || !ploc || d->num_tris < 1 || d->num_tris > RODENT_BUILD_MAX_TRIS
        || rodent_hip_build_ploc_scratch_bytes(d->num_tris, opt, split, ploc) < 0 || d->num_vertices < 1 || d->nodes || d->tris
        || d->num_nodes || d->num_bvh_tris) {
        fprintf(stderr, "rodent_hip: rodent_hip_scene_create_device_bvh_ploc: invalid arguments (max_leaf 1 ... 8, treelet passes "
                        "0 ... 3, costs in (0, 1e6], split budget 0 ... 4, max_pieces 1 ... 64, PLOC radius 1 ... 64, depth limit 0 or "
                        "ceil(log2 references) ... 56 and 56 with treelet passes, wide iterations -1 ... 255, 1 ... 2^25 triangles, "
                        "no hierarchy in the description)\n");
        abort();
    }
    scene_create(dev, d, opt, split, ploc);
}

// The host refit: the caller's tables, the hierarchy refitted in place, the images and shading records remade on the host as the
// creation makes them -- the path the device refit below is held against.
void rodent_hip_scene_refit(int32_t dev, const float* vertices, const float* normals, const float* face_normals,
                            const RodentLight* lights) {
    DevScene& s = flat_scene(dev, "rodent_hip_scene_refit");
    if (!vertices || !normals || !face_normals || (s.dev.num_lights > 0 && !lights)) {
        fprintf(stderr, "rodent_hip: rodent_hip_scene_refit: a NULL table\n"); abort(); }
    HIP_CHECK(hipSetDevice(dev));
    HIP_CHECK(hipDeviceSynchronize());                   // no frame still reads the tables that are overwritten
    const size_t nv = (size_t)s.num_vertices, nt = (size_t)s.dev.num_tris;
    HIP_CHECK(hipMemcpy(const_cast<float*>(s.dev.vertices), vertices, sizeof(float) * 4 * nv, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(const_cast<float*>(s.dev.normals), normals, sizeof(float) * 4 * nv, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(const_cast<float*>(s.dev.face_normals), face_normals, sizeof(float) * 4 * nt, hipMemcpyHostToDevice));
    if (s.dev.num_lights > 0)
        HIP_CHECK(hipMemcpy(const_cast<RodentLight*>(s.dev.lights), lights, sizeof(RodentLight) * (size_t)s.dev.num_lights,
                            hipMemcpyHostToDevice));
    // the hierarchy, in place: rodent_hip_scene_bvh's pointers stay valid
    Node2* nodes = const_cast<Node2*>(s.dev.nodes);
    Tri1* tris = const_cast<Tri1*>(s.dev.tris);
    int32_t info[RODENT_BUILD_INFO_WORDS] = {};
    BuildScratch work(rodent_hip_refit_scratch_bytes(s.num_nodes, s.num_bvh_tris), RODENT_BUILD_INFO_WORDS);
    const int32_t rc = rodent_hip_refit_bvh2_tri1(dev, s.dev.vertices, s.num_vertices, s.dev.indices, s.dev.num_tris, nodes, s.num_nodes,
                                                  tris, s.num_bvh_tris, work.scratch, work.info_dev, nullptr);
    const int32_t bad = work.finish(rc, info, s.num_nodes, s.num_nodes);
    if (rc != RODENT_BUILD_OK) { fprintf(stderr, "rodent_hip: device BVH refit refused (%d)\n", rc); abort(); }
    if (bad) {
        fprintf(stderr, "rodent_hip: invalid scene: device BVH refit flagged the mesh or the hierarchy (flags %d, %d of %d nodes)\n",
                info[2], info[0], s.num_nodes); abort(); }
    // what scene_create derives from positions or bounds, into its existing allocations: both LDS images and the tri_shade records
    std::vector<Node2> host_nodes((size_t)s.num_nodes);
    HIP_CHECK(hipMemcpy(host_nodes.data(), nodes, sizeof(Node2) * host_nodes.size(), hipMemcpyDeviceToHost));
    for (const int capacity : {kSceneTopNodes, kPersistTopNodes}) {
        const std::vector<int32_t> image = build_image(host_nodes.data(), capacity);
        const int4* dst = capacity == kSceneTopNodes ? s.dev.top_image : s.dev.top_image_large;
        HIP_CHECK(hipMemcpy(const_cast<int4*>(dst), image.data(), sizeof(int32_t) * image.size(), hipMemcpyHostToDevice));
    }
    if (s.dev.tri_shade) {
        std::vector<int32_t> indices(4 * nt);
        HIP_CHECK(hipMemcpy(indices.data(), s.dev.indices, sizeof(int32_t) * indices.size(), hipMemcpyDeviceToHost));
        const std::vector<float> rec = tri_shade(face_normals, normals, indices.data(), s.dev.num_tris);
        HIP_CHECK(hipMemcpy(const_cast<float4*>(s.dev.tri_shade), rec.data(), sizeof(float) * rec.size(), hipMemcpyHostToDevice));
    }
}

void rodent_hip_scene_refit_prepare(int32_t dev, int32_t smooth_normals) {
    flat_scene(dev, "rodent_hip_scene_refit_prepare");
    refit_prepare(rdev(dev), smooth_normals != 0);
}

void rodent_hip_scene_refit_device(int32_t dev, const float* vertices_dev, const float* normals_dev, void* stream_) {
    DevScene& s = flat_scene(dev, "rodent_hip_scene_refit_device");
    RenderDevice& r = rdev(dev);
    if (!vertices_dev) { fprintf(stderr, "rodent_hip: rodent_hip_scene_refit_device: NULL vertices\n"); abort(); }
    if (!s.refit_info || (!normals_dev && !s.corner_first)) refit_prepare(r, !normals_dev);
    hipStream_t stream = begin_update(r, stream_);
    const int nv = s.num_vertices, nt = s.dev.num_tris, nl = s.dev.num_lights;
    const GeometryDev g = copy_in_geometry(s, vertices_dev, normals_dev, stream);
    hipLaunchKernelGGL(k_face_normals, blocks(nt), dim3(kBlock), 0, stream, g.vertices, g.indices, nt, g.face_normals);
    if (nl > 0) hipLaunchKernelGGL(k_light_records, blocks(nl), dim3(kBlock), 0, stream, g.vertices, g.indices, s.light_tri, nl,
                                   const_cast<RodentLight*>(s.dev.lights));
    if (!normals_dev) hipLaunchKernelGGL(k_smooth_normals, blocks(nv), dim3(kBlock), 0, stream, g.face_normals, s.corner_first,
                                         s.corner_tri, nv, g.normals);
    // the hierarchy, in place: rodent_hip_scene_bvh's pointers stay valid
    const int32_t rc = rodent_hip_refit_bvh2_tri1(dev, s.dev.vertices, nv, s.dev.indices, nt, const_cast<Node2*>(s.dev.nodes), s.num_nodes,
                                                  const_cast<Tri1*>(s.dev.tris), s.num_bvh_tris, s.refit_scratch, s.refit_info, stream);
    if (rc != RODENT_BUILD_OK) { fprintf(stderr, "rodent_hip: device BVH refit refused (%d)\n", rc); abort(); }
    hipLaunchKernelGGL(k_scene_images, dim3(2), dim3(kWave), 0, stream, s.dev.nodes, const_cast<int4*>(s.dev.top_image),
                       const_cast<int4*>(s.dev.top_image_large));
    if (s.dev.tri_shade) hipLaunchKernelGGL(k_tri_shade, blocks(nt), dim3(kBlock), 0, stream, g.face_normals, g.normals, g.indices, nt,
                                            const_cast<float4*>(s.dev.tri_shade));
    HIP_CHECK(hipGetLastError());
    end_update(r, stream);
}

int32_t rodent_hip_scene_refit_status(int32_t dev, int32_t* info) {
    DevScene& s = flat_scene(dev, "rodent_hip_scene_refit_status");
    int32_t words[RODENT_BUILD_INFO_WORDS] = {s.num_nodes, s.num_bvh_tris, 0, 0};      // before the first refit: a sound one's words
    if (s.refit_enqueued) {
        HIP_CHECK(hipSetDevice(dev));
        HIP_CHECK(hipEventSynchronize(rdev(dev).ev_refit));
        HIP_CHECK(hipMemcpy(words, s.refit_info, sizeof(words), hipMemcpyDeviceToHost));
    }
    if (info) std::copy(words, words + RODENT_BUILD_INFO_WORDS, info);
    return words[2] | (words[0] != s.num_nodes ? (int32_t)0x80000000u : 0);
}

void rodent_hip_scene_tables(int32_t dev, RodentSceneTables* out) {
    const DevScene& s = loaded_scene(dev, "rodent_hip_scene_tables");
    if (!out) return;
    *out = RodentSceneTables{const_cast<float*>(s.dev.vertices), const_cast<float*>(s.dev.normals), const_cast<float*>(s.dev.face_normals),
        const_cast<RodentLight*>(s.dev.lights), reinterpret_cast<float*>(const_cast<float4*>(s.dev.tri_shade)),
        reinterpret_cast<int32_t*>(const_cast<int4*>(s.dev.top_image)),
        reinterpret_cast<int32_t*>(const_cast<int4*>(s.dev.top_image_large)),
        s.num_vertices, s.dev.num_tris, s.dev.num_lights, kSceneTopNodes, kPersistTopNodes};
}

void rodent_hip_scene_bvh(int32_t dev, const Node2** nodes, const Tri1** tris, int32_t* num_nodes, int32_t* num_tris) {
    const DevScene& s = loaded_scene(dev, "rodent_hip_scene_bvh");
    *nodes = s.dev.nodes; *tris = s.dev.tris;
    *num_nodes = s.num_nodes; *num_tris = s.num_bvh_tris;
}

int32_t rodent_hip_scene_create_instanced(int32_t dev, const RodentSceneDesc* d, const RodentObjectRange* objects, int32_t num_objects,
                                          const RodentInstanceDesc* instances, int32_t num_instances, const RodentBuildOptions* opt) {
    return create_instanced_scene(dev, d, objects, num_objects, instances, num_instances, opt);
}

int32_t rodent_hip_scene_create_motion(int32_t dev, const RodentSceneDesc* d, const RodentObjectRange* objects, int32_t num_objects,
                                       const RodentMotionInstanceDesc* instances, int32_t num_instances, const RodentBuildOptions* opt) {
    return create_instanced_scene(dev, d, objects, num_objects, instances, num_instances, opt);
}

int32_t rodent_hip_scene_create_flags(int32_t dev) { return rdev(dev).create_flags; }

void rodent_hip_scene_set_transforms(int32_t dev, const float* object_to_world_dev, void* stream_) {
    DevScene& s = instanced_scene(dev, "rodent_hip_scene_set_transforms");
    RenderDevice& r = rdev(dev);
    if (!object_to_world_dev) { fprintf(stderr, "rodent_hip: rodent_hip_scene_set_transforms: NULL matrices\n"); abort(); }
    hipStream_t stream = begin_update(r, stream_);
    hipLaunchKernelGGL(k_instance_matrices, blocks(12 * s.num_instances), dim3(kBlock), 0, stream, object_to_world_dev, s.num_instances,
                       s.descs);
    rederive_instanced(dev, s, stream);
    end_update(r, stream);
}

void rodent_hip_scene_set_motion_transforms(int32_t dev, const float* m0_dev, const float* m1_dev, void* stream_) {
    DevScene& s = motion_scene(dev, "rodent_hip_scene_set_motion_transforms");
    RenderDevice& r = rdev(dev);
    if (!m0_dev || !m1_dev) { fprintf(stderr, "rodent_hip: rodent_hip_scene_set_motion_transforms: NULL matrices\n"); abort(); }
    hipStream_t stream = begin_update(r, stream_);
    hipLaunchKernelGGL(k_motion_instance_matrices, blocks(24 * s.num_instances), dim3(kBlock), 0, stream, m0_dev, m1_dev, s.num_instances,
                       s.motion_descs);
    rederive_instanced(dev, s, stream);
    end_update(r, stream);
}

int32_t rodent_hip_scene_transforms_status(int32_t dev, int32_t* info) {
    DevScene& s = loaded_scene(dev, "rodent_hip_scene_transforms_status");
    if (!s.motion) instanced_scene(dev, "rodent_hip_scene_transforms_status");       // (it serves a moving scene's moves too)
    int32_t words[RODENT_BUILD_INFO_WORDS] = {};
    HIP_CHECK(hipSetDevice(dev));
    if (s.refit_enqueued) HIP_CHECK(hipEventSynchronize(rdev(dev).ev_refit));
    HIP_CHECK(hipMemcpy(words, s.tlas_info, sizeof(words), hipMemcpyDeviceToHost));
    if (info) std::copy(words, words + RODENT_BUILD_INFO_WORDS, info);
    return words[2];
}

int32_t rodent_hip_scene_deform_prepare(int32_t dev, const int32_t* objects, int32_t num_objects, int32_t smooth_normals) {
    RenderDevice& r = rdev(dev);
    DevScene& s = r.scene;
    // ---- the refusals: on the host, the scene and an earlier set stay as they are ----
    if (!s.loaded || !s.instanced || s.motion) return RODENT_SCENE_ERR_NOT_INSTANCED;
    if (!objects || num_objects < 1) return RODENT_SCENE_ERR_COUNTS;
    std::vector<char> listed((size_t)s.num_objects, 0);
    for (int32_t k = 0; k < num_objects; k++) {
        if (objects[k] < 0 || objects[k] >= s.num_objects || listed[objects[k]]) return RODENT_SCENE_ERR_OBJECT;
        listed[objects[k]] = 1;
    }
    std::vector<int32_t> first_tri((size_t)num_objects), num_tris((size_t)num_objects);
    for (int32_t k = 0; k < num_objects; k++) {
        first_tri[k] = s.object_ranges[objects[k]].first_tri; num_tris[k] = s.object_ranges[objects[k]].num_tris; }
    std::vector<RodentRefitRange> ranges((size_t)num_objects);
    int32_t totals[2] = {};
    const int64_t scratch_bytes = rodent_hip_refit_objects_plan(s.object_table.data(), s.num_objects, objects, first_tri.data(),
                                                                num_tris.data(), num_objects, ranges.data(), totals);
    if (scratch_bytes < 0) return RODENT_SCENE_ERR_COUNTS;
    // ---- from here on the set is the new one ----
    HIP_CHECK(hipSetDevice(dev));
    HIP_CHECK(hipDeviceSynchronize());                   // no update still works in the lists that are replaced
    for (void* p : s.deform.allocs) HIP_CHECK(hipFree(p));
    s.deform = DevScene::DeformSet();
    DevScene::DeformSet& d = s.deform;
    d.ranges = upload(d.allocs, ranges.data(), ranges.size());
    d.scratch = alloc_scratch_info(d.allocs, scratch_bytes, RODENT_BUILD_INFO_WORDS, d.info);
    HIP_CHECK(hipMemset(d.info, 0, 4 * RODENT_BUILD_INFO_WORDS));
    d.num_listed = num_objects; d.num_nodes = totals[0]; d.num_tris = totals[1]; d.smooth = smooth_normals != 0;
    std::vector<RodentObjectRange> listed_ranges;          // in object order
    for (int32_t o = 0; o < s.num_objects; o++) if (listed[o]) listed_ranges.push_back(s.object_ranges[o]);
    // (a light is bound to a triangle of its own object: the creation checked)
    const RefitLists lists = refit_lists(s, listed_ranges, d.smooth);
    d.lights = upload(d.allocs, lists.lights.data(), lists.lights.size()); d.num_lights = (int)lists.lights.size();
    if (d.smooth) {
        d.verts = upload(d.allocs, lists.verts.data(), lists.verts.size()); d.num_verts = (int)lists.verts.size();
        d.corner_first = upload(d.allocs, lists.corner_first.data(), lists.corner_first.size());
        d.corner_tri = upload(d.allocs, lists.corner_tri.data(), lists.corner_tri.size());
    }
    return RODENT_SCENE_OK;
}

void rodent_hip_scene_deform_device(int32_t dev, const float* vertices_dev, const float* normals_dev, const float* object_to_world_dev,
                                    void* stream_) {
    DevScene& s = instanced_scene(dev, "rodent_hip_scene_deform_device");
    RenderDevice& r = rdev(dev);
    DevScene::DeformSet& d = s.deform;
    if (!vertices_dev) { fprintf(stderr, "rodent_hip: rodent_hip_scene_deform_device: NULL vertices\n"); abort(); }
    if (!d.ranges || (!normals_dev && !d.smooth)) {
        fprintf(stderr, "rodent_hip: rodent_hip_scene_deform_device: no deforming set declared (rodent_hip_scene_deform_prepare%s)\n",
                d.ranges ? " with smooth_normals, or pass normals" : ""); abort(); }
    hipStream_t stream = begin_update(r, stream_);
    const GeometryDev g = copy_in_geometry(s, vertices_dev, normals_dev, stream);
    if (object_to_world_dev)
        hipLaunchKernelGGL(k_instance_matrices, blocks(12 * s.num_instances), dim3(kBlock), 0, stream, object_to_world_dev,
                           s.num_instances, s.descs);
    const DeformTris tris{d.ranges, d.num_listed, d.num_tris};
    hipLaunchKernelGGL(k_deform_face_normals, blocks(d.num_tris), dim3(kBlock), 0, stream, g.vertices, g.indices, tris, g.face_normals);
    if (d.num_lights > 0) hipLaunchKernelGGL(k_deform_light_records, blocks(d.num_lights), dim3(kBlock), 0, stream, g.vertices, g.indices,
                                             d.lights, d.num_lights, s.object_lights);
    if (!normals_dev) hipLaunchKernelGGL(k_deform_smooth_normals, blocks(d.num_verts), dim3(kBlock), 0, stream, g.face_normals, d.verts,
                                         d.corner_first, d.corner_tri, d.num_verts, g.normals);
    // the listed objects' hierarchies, in the packed allocation: rodent_hip_scene_bvh's pointers stay valid
    const int32_t rc = rodent_hip_refit_objects(dev, s.dev.vertices, s.num_vertices, s.dev.indices, s.dev.num_tris,
                                                const_cast<Node2*>(s.dev.nodes), const_cast<Tri1*>(s.dev.tris), s.objects, s.num_objects,
                                                d.ranges, d.num_listed, d.num_nodes, d.num_tris, d.scratch, d.info, stream);
    if (rc != RODENT_BUILD_OK) { fprintf(stderr, "rodent_hip: refit of the deforming objects refused (%d)\n", rc); abort(); }
    if (s.dev.tri_shade) hipLaunchKernelGGL(k_deform_tri_shade, blocks(d.num_tris), dim3(kBlock), 0, stream, g.face_normals, g.normals,
                                            g.indices, tris, const_cast<float4*>(s.dev.tri_shade));
    // the objects' boxes changed: the TLAS, slot_of and the world lights, as after a move
    rederive_instanced(dev, s, stream);
    end_update(r, stream);
    d.enqueued = true;
}

int32_t rodent_hip_scene_deform_status(int32_t dev, int32_t* refit_info, int32_t* tlas_info) {
    DevScene& s = instanced_scene(dev, "rodent_hip_scene_deform_status");
    const DevScene::DeformSet& d = s.deform;
    int32_t refit[RODENT_BUILD_INFO_WORDS] = {d.num_nodes, d.num_tris, 0, 0}, tlas[RODENT_BUILD_INFO_WORDS] = {};
    HIP_CHECK(hipSetDevice(dev));
    if (s.refit_enqueued) HIP_CHECK(hipEventSynchronize(rdev(dev).ev_refit));
    if (d.enqueued) HIP_CHECK(hipMemcpy(refit, d.info, sizeof(refit), hipMemcpyDeviceToHost));    // before the first: a sound one's words
    HIP_CHECK(hipMemcpy(tlas, s.tlas_info, sizeof(tlas), hipMemcpyDeviceToHost));
    if (refit_info) std::copy(refit, refit + RODENT_BUILD_INFO_WORDS, refit_info);
    if (tlas_info) std::copy(tlas, tlas + RODENT_BUILD_INFO_WORDS, tlas_info);
    return refit[2] | tlas[2] | (refit[0] < d.num_nodes ? (int32_t)0x80000000u : 0);
}

int32_t rodent_hip_scene_create_deforming(int32_t dev, const RodentSceneDesc* d, const float* vertices1, const float* normals1,
                                          const RodentBuildOptions* opt) {
    return create_deforming_scene(dev, d, vertices1, normals1, opt);
}

void rodent_hip_scene_set_motion_keys(int32_t dev, const float* vertices0_dev, const float* vertices1_dev, const float* normals0_dev,
                                      const float* normals1_dev, void* stream_) {
    DevScene& s = deforming_scene(dev, "rodent_hip_scene_set_motion_keys");
    RenderDevice& r = rdev(dev);
    if (!vertices0_dev || !vertices1_dev || !normals0_dev != !normals1_dev) {
        fprintf(stderr, "rodent_hip: rodent_hip_scene_set_motion_keys: NULL vertices, or one table of normals without the other\n");
        abort(); }
    hipStream_t stream = begin_update(r, stream_);
    const int nv = s.num_vertices, nt = s.dev.num_tris;
    const size_t bytes = sizeof(float4) * (size_t)nv;
    float* const own[4] = {const_cast<float*>(s.dev.vertices), s.vertices1, const_cast<float*>(s.dev.normals), s.normals1};
    const float* const given[4] = {vertices0_dev, vertices1_dev, normals0_dev, normals1_dev};
    for (int k = 0; k < 4; k++)                             // (a key that IS the scene's table was written in place: no copy)
        if (given[k] && given[k] != own[k]) HIP_CHECK(hipMemcpyAsync(own[k], given[k], bytes, hipMemcpyDeviceToDevice, stream));
    if (!normals0_dev) {                                    // smooth normals per key, by rodent_hip_scene_refit_device's rule and kernels
        const int4* indices = reinterpret_cast<const int4*>(s.dev.indices);
        float* const faces[2] = {const_cast<float*>(s.dev.face_normals), s.face_normals1};
        for (int k = 0; k < 2; k++) {
            hipLaunchKernelGGL(k_face_normals, blocks(nt), dim3(kBlock), 0, stream, reinterpret_cast<const float4*>(own[k]), indices, nt,
                               reinterpret_cast<float4*>(faces[k]));
            hipLaunchKernelGGL(k_smooth_normals, blocks(nv), dim3(kBlock), 0, stream, reinterpret_cast<const float4*>(faces[k]),
                               s.corner_first, s.corner_tri, nv, reinterpret_cast<float4*>(own[2 + k]));
        }
    }
    const int32_t rc = derive_deforming(dev, s, stream);
    if (rc != RODENT_BUILD_OK) { fprintf(stderr, "rodent_hip: rebuild of the motion records refused (%d)\n", rc); abort(); }
    HIP_CHECK(hipGetLastError());
    end_update(r, stream);
}

int32_t rodent_hip_scene_motion_keys_status(int32_t dev, int32_t* info) {
    RenderDevice& r = rdev(dev);
    DevScene& s = r.scene;
    int32_t words[RODENT_BUILD_INFO_WORDS] = {};
    if (!s.loaded || !s.deforming) {                        // (never aborts: no such scene has completed nothing)
        if (info) std::copy(words, words + RODENT_BUILD_INFO_WORDS, info);
        return (int32_t)0x80000000u;
    }
    HIP_CHECK(hipSetDevice(dev));
    if (s.refit_enqueued) HIP_CHECK(hipEventSynchronize(r.ev_refit));
    HIP_CHECK(hipMemcpy(words, s.motion_info, sizeof(words), hipMemcpyDeviceToHost));
    if (info) std::copy(words, words + RODENT_BUILD_INFO_WORDS, info);
    return words[2] | (words[0] != s.num_nodes || words[3] != s.num_nodes ? (int32_t)0x80000000u : 0);
}

void rodent_hip_scene_motion_bvh(int32_t dev, const RodentMotionNode2** nodes, const RodentMotionTri1** tris, int32_t* num_nodes,
                                 int32_t* num_tris) {
    const DevScene& s = deforming_scene(dev, "rodent_hip_scene_motion_bvh");
    *nodes = s.motion_nodes; *tris = s.motion_tris;
    *num_nodes = s.num_nodes; *num_tris = s.num_bvh_tris;
}

void rodent_hip_scene_motion_keys(int32_t dev, RodentSceneMotionKeys* out) {
    const DevScene& s = deforming_scene(dev, "rodent_hip_scene_motion_keys");
    if (!out) return;
    *out = RodentSceneMotionKeys{const_cast<float*>(s.dev.vertices), s.vertices1, const_cast<float*>(s.dev.normals), s.normals1,
        s.motion_info, s.num_vertices};
}

void rodent_hip_scene_instances(int32_t dev, RodentSceneInstances* out) {
    DevScene& s = instanced_scene(dev, "rodent_hip_scene_instances");
    if (!out) return;
    ensure_ray_slots(rdev(dev), 0);
    *out = RodentSceneInstances{s.tlas_nodes, s.instances, s.descs, s.objects, s.slot_of, reinterpret_cast<int32_t*>(s.bases),
        s.light_owner, s.world_lights, s.object_lights, s.inst.ray_slots, s.tlas_info, s.num_instances, s.num_objects,
        std::max(1, s.num_instances - 1), s.dev.num_lights, s.num_object_lights, (int32_t)s.ray_slot_cap};
}

void rodent_hip_scene_motion_instances(int32_t dev, RodentSceneMotionInstances* out) {
    DevScene& s = motion_scene(dev, "rodent_hip_scene_motion_instances");
    if (!out) return;
    ensure_ray_slots(rdev(dev), 0);
    *out = RodentSceneMotionInstances{s.tlas_nodes, s.motion_instances, s.motion_descs, s.objects, s.slot_of,
        reinterpret_cast<int32_t*>(s.bases), s.light_owner, s.world_lights, s.object_lights, s.inst.ray_slots, s.tlas_info, s.num_instances,
        s.num_objects, std::max(1, s.num_instances - 1), s.dev.num_lights, s.num_object_lights, (int32_t)s.ray_slot_cap};
}

} // extern "C"
