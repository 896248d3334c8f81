/*
 * rodent_render.h -- C ABI of the MI355X wavefront path tracer (librodent_hip.so).
 *
 * Stands where the reference has the AnyDSL-generated `interface.h` (src/CMakeLists.txt:76-79)
 * plus the `extern "C"` services of src/driver/interface.cpp:565-675.  In the reference the
 * scene is compiled into `render()` by the converter (src/driver/converter.cpp:613-967 emits
 * Impala source); here the scene is DATA: tables uploaded once with rodent_hip_scene_create(),
 * and spp / max path length are run-time values (rodent_hip_render_config) instead of
 * converter flags (converter.cpp:1007-1012).
 *
 * Kept from the reference, same names and meaning:
 *   Settings, get_spp(), render(settings, iter)                 src/dummy_main.impala:3-13
 *   RayStream / PrimaryStream / SecondaryStream (SoA slabs)      src/render/driver.impala:24-61
 *   setup_interface / get_pixels / clear_pixels / cleanup_interface   src/driver/interface.cpp:512-526
 *   rodent_get_film_data, rodent_gpu_get_{first,second}_primary_stream,
 *   rodent_gpu_get_secondary_stream, rodent_gpu_get_tmp_buffer, rodent_present   interface.cpp:567-582,631-663
 * Device ids: `dev` is the HIP device ordinal (the reference packs platform and index,
 * src/render/mapping_gpu.impala:538,596; 0 there means "host").
 * Errors: message on stderr + abort(), like src/driver/common.h:43-59.
 */
#ifndef RODENT_RENDER_H
#define RODENT_RENDER_H

#include <stdint.h>
#include <stddef.h>
#include "rodent_traversal.h"
#include "rodent_instances.h"
#include "rodent_motion.h"

#ifdef __cplusplus
extern "C" {
#endif

struct Vec3 { float x, y, z; };
/* width/height = tan(fov/2), that / ratio (driver.cpp:37-38) */
struct Settings { struct Vec3 eye, dir, up, right; float width, height; };

struct RayStream { int32_t* id; float *org_x, *org_y, *org_z, *dir_x, *dir_y, *dir_z, *tmin, *tmax; };
struct PrimaryStream {
    struct RayStream rays; int32_t *geom_id, *prim_id; float *t, *u, *v;
    uint32_t* rnd; float *mis, *contrib_r, *contrib_g, *contrib_b; int32_t* depth; int32_t size, pad;
};
struct SecondaryStream { struct RayStream rays; int32_t* prim_id; float *color_r, *color_g, *color_b; int32_t size, pad; };

/* ---- scene tables (what the converter bakes into Impala source in the reference) ---- */
enum RodentBsdf { RODENT_BSDF_BLACK = 0, RODENT_BSDF_DIFFUSE = 1, RODENT_BSDF_PHONG = 2,
                  RODENT_BSDF_MIX = 3 /* diffuse (+) phong */, RODENT_BSDF_MIRROR = 4, RODENT_BSDF_GLASS = 5 };
struct RodentMaterial {            /* 64 B; one per geometry id (converter.cpp:858-920) */
    float kd[3]; int32_t type; float ks[3]; float ns; float tf[3]; float ni;
    float mix_k;                   /* lum(ks) / (lum(ks) + lum(kd)) (converter.cpp:900-906); recomputed per hit when textured */
    int32_t emissive;
    /* 0: kd / ks are the constants above; else 1 + index of the map_Kd / map_Ks texture (converter.cpp:881-893) */
    int32_t tex_kd, tex_ks;
};
struct RodentTexture {             /* RGBA8 image, row 0 = bottom row of the file, gamma-corrected (src/driver/image.cpp:10-18,85) */
    int32_t width, height; uint32_t offset /* first texel in the pool */; int32_t pad;
};
struct RodentLight {               /* 80 B; triangle area light (converter.cpp:831-851, light.impala:140-154) */
    float v0[4], v1[4], v2[4]; float n[3]; float inv_area; float color[4];
};
struct RodentSceneDesc {           /* HOST pointers; copied to HBM by rodent_hip_scene_create */
    const float* vertices;         /* float4 per vertex (padded like the GPU targets, converter.cpp:629-632) */
    const float* normals;          /* float4 per vertex */
    const float* face_normals;     /* float4 per triangle */
    const int32_t* indices;        /* int4 per triangle: v0 v1 v2 material (obj.cpp:455-461) */
    const struct Node2* nodes; const struct Tri1* tris;     /* BVH2/Tri1, geom_id = material id */
    const struct RodentMaterial* materials; const struct RodentLight* lights;
    const int32_t* light_ids;      /* per triangle: index into lights (0 if not a light) */
    int32_t num_vertices, num_tris, num_nodes, num_bvh_tris, num_materials, num_lights;
    /* textures (src/render/image.impala:56-92: repeat border, bilinear filter); all three may be NULL when num_textures == 0 */
    const float* texcoords;        /* float4 per vertex: u, v, 0, 0 (converter.cpp:408) */
    const struct RodentTexture* textures; const uint32_t* texels;
    int32_t num_textures; uint32_t num_texels;
};

void    rodent_hip_scene_create(int32_t dev, const struct RodentSceneDesc* desc);   /* replaces the device's current scene */
void    rodent_hip_scene_destroy(int32_t dev);
/* rodent_hip_scene_create with a hierarchy built on the device (rodent_build.h: LBVH, leaves of at most max_leaf = 1 ... 8
 * triangles, 2 = the host builder's threshold) from the vertices and indices it uploads: desc->nodes and desc->tris must be NULL and
 * num_nodes / num_bvh_tris 0.  Everything the library derives from a hierarchy (the per-scene mapping rules, the LDS images) is derived
 * from the built one; the hierarchy is deterministic, so is everything after it. */
void    rodent_hip_scene_create_device_bvh(int32_t dev, const struct RodentSceneDesc* desc, int32_t max_leaf);
/* The same with the options of the optimising builder (rodent_build.h: RodentBuildOptions; treelet_passes = 0 is the call above
 * with opt->max_leaf).  Invalid options abort, as invalid arguments above do. */
struct RodentBuildOptions;
void    rodent_hip_scene_create_device_bvh_opt(int32_t dev, const struct RodentSceneDesc* desc, const struct RodentBuildOptions* opt);
/* The same over pre-split triangle references (rodent_build.h: RodentSplitOptions); the scene's BVH triangle count is the reference
 * count the builder reports.  Invalid options abort. */
struct RodentSplitOptions;
void    rodent_hip_scene_create_device_bvh_split(int32_t dev, const struct RodentSceneDesc* desc, const struct RodentBuildOptions* opt,
                                                 const struct RodentSplitOptions* split);
/* The same with the PLOC topology stage (rodent_build.h: RodentPlocOptions) in place of the LBVH's; `split` may be NULL: no
 * pre-splitting.  Invalid options abort. */
struct RodentPlocOptions;
void    rodent_hip_scene_create_device_bvh_ploc(int32_t dev, const struct RodentSceneDesc* desc, const struct RodentBuildOptions* opt,
                                                const struct RodentSplitOptions* split, const struct RodentPlocOptions* ploc);
/* The current scene after its geometry moved: new HOST tables with the counts given at creation (vertices, normals: num_vertices x 4
 * floats; face_normals: num_tris x 4; lights: num_lights); indices, materials, light ids, textures and the hierarchy's topology stay.
 * Overwrites the device copies in place, refits the hierarchy in place (rodent_build.h: rodent_hip_refit_bvh2_tri1; the pointers of
 * rodent_hip_scene_bvh stay valid) and rebuilds what the scene derives from positions or bounds (the LDS top images, the gathered
 * shading records) in their existing allocations; the rules that depend on node counts stay as they are.  Synchronous: waits for the
 * device before and after.  A flag raised by the refit aborts with a message, as a flagged device build does. */
void    rodent_hip_scene_refit(int32_t dev, const float* vertices, const float* normals, const float* face_normals,
                               const struct RodentLight* lights);
/* ---- moved geometry that is already on the device ----
 * rodent_hip_scene_refit above takes HOST tables the caller computed, waits for the device and walks the hierarchy on the host.  The
 * entries below take moved vertices that live in HBM, derive everything the scene keeps from positions on the device and enqueue it on
 * a stream.  The rules, all in fp32 with every operation rounded on its own (they restate host/mesh.cpp, host/scene.cpp and host/vec.h:
 * a scene loaded from an OBJ without `vn` lines reproduces the loader's own tables; CPU model: tests/scene_update_model.py):
 *   Face normal of triangle t: a = v1 - v0, b = v2 - v0 (through `indices`); c = (a.y b.z - a.z b.y, a.z b.x - a.x b.z,
 *     a.x b.y - a.y b.x); l = sqrt((c.x c.x + c.y c.y) + c.z c.z); the normal is c * (1.0f / l), w = 0.  A degenerate triangle gives
 *     NaN, as on the host: nothing special is done for it.
 *   Smooth vertex normals (normals_dev == NULL): s = (0, 0, 0); for every corner (t, k) that names the vertex, in ascending (t, k)
 *     order, s += face normal of t (a triangle naming a vertex twice counts twice); l2 = (s.x s.x + s.y s.y) + s.z s.z; if
 *     l2 <= FLT_EPSILON or l2 is NaN the normal is (0, 1, 0), otherwise s * (1.0f / sqrt(l2)); w = 0.  A vertex no triangle names gets
 *     (0, 1, 0).  The fixed order comes from incidence lists (offsets + triangle ids) built once, on the host, by the prepare call:
 *     indices never change under a refit.
 *   Light k is bound to the lowest triangle t whose material is emissive and whose light_ids[t] == k; a light no such triangle names
 *     keeps its bytes.  A bound light gets v0, v1, v2 (three floats each; the fourth word stays as stored), and with c and l as above
 *     n = c * (1.0f / l) and inv_area = 1.0f / (0.5f * l).  The colour stays as stored.
 *   tri_shade record t (only when the scene has the table): the face normal's x, y, z, then the three corners' vertex normals, gathered.
 *   Top images (31 and 255 records of 16 words): breadth first from the root, a node's child 0 before its child 1; a child gets a slot
 *     (and becomes a link) only while fewer than `capacity` slots are taken; words 0 .. 11 the bounds, 12 .. 13 the child ids / links,
 *     14 the node's 1-based id, 15 zero; unused records are all zero.  (Computed level by level: the slot of child j of the i-th node of a
 *     level is the count of slots taken before the level's children plus the inner children of the level's earlier nodes, plus one for
 *     j = 1 when child 0 is inner.)
 *
 * rodent_hip_scene_refit_prepare: one-time, synchronous: allocates what rodent_hip_scene_refit_device needs for the current scene (refit
 * scratch and info words; the light -> triangle table; with smooth_normals != 0 the vertex -> triangle incidence lists).  Owned by the
 * scene, freed with it.  Calling it again is harmless (smooth_normals is sticky once set). */
void    rodent_hip_scene_refit_prepare(int32_t dev, int32_t smooth_normals);
/* The scene's geometry moved; all pointers are DEVICE pointers on `dev`.
 *   vertices_dev: num_vertices x 4 floats; may be the scene's own table (rodent_hip_scene_tables), then nothing is copied.
 *   normals_dev:  num_vertices x 4 floats, or NULL: smooth normals are recomputed (rule above).
 * Enqueues on `stream` (NULL = the null stream): the copies, face normals, light records, vertex normals, the in-place BVH2 refit
 * (rodent_hip_refit_bvh2_tri1), both LDS top images and the tri_shade records, into the scene's existing allocations.  After the
 * first call (which prepares if nobody did) it allocates nothing, copies nothing to or from the host and does not wait for the device.
 * A refit starts behind the one before it, and a frame started afterwards (render(), rodent_hip_render_rows / _tiles, the stage-level
 * entries, on any stream) behind the last refit: both are ordered with an event.  A frame call returns when its rows are in the film,
 * so a frame started earlier has finished on the old scene.  No scene loaded or a NULL vertices_dev aborts with a message. */
void    rodent_hip_scene_refit_device(int32_t dev, const float* vertices_dev, const float* normals_dev, void* stream);
/* Waits for the last rodent_hip_scene_refit_device of `dev`, copies the refit's RODENT_BUILD_INFO_WORDS words to info (may be NULL).
 * Returns 0 for a sound refit (no flag, info[0] == node count), else the flags (bit 31 set when nodes are missing).  Never aborts on a
 * flag.  Before the first refit: 0 and a sound refit's words. */
int32_t rodent_hip_scene_refit_status(int32_t dev, int32_t* info);
/* DEVICE pointers of the tables the scene owns, for tools and tests (like rodent_hip_scene_bvh); out may be NULL. */
struct RodentSceneTables { float *vertices, *normals, *face_normals; struct RodentLight* lights; float* tri_shade; /* may be NULL */
                           int32_t *top_image, *top_image_large; int32_t num_vertices, num_tris, num_lights, top_nodes, top_nodes_large; };
void    rodent_hip_scene_tables(int32_t dev, struct RodentSceneTables* out);
/* The current scene's hierarchy on device `dev`: DEVICE pointers (owned by the scene) and counts -- for tests and tools. */
void    rodent_hip_scene_bvh(int32_t dev, const struct Node2** nodes, const struct Tri1** tris, int32_t* num_nodes, int32_t* num_tris);
/* ---- instanced scenes: objects placed by 3 x 4 matrices, rendered through the two-level hierarchy of rodent_instances.h ----
 * CPU model of everything below: tests/instanced_scene_model.py (over tests/instance_model.py).
 * `desc` holds the CONCATENATED tables of all objects, in object space (vertices, normals, face normals, indices with vertex ids into the
 * concatenated vertex table, materials, texture tables, lights, light ids); desc->nodes and desc->tris must be NULL and num_nodes /
 * num_bvh_tris 0.  Object o is the triangle range [first_tri, first_tri + num_tris) and the light range [first_light, first_light +
 * num_lights); the triangle ranges tile [0, desc->num_tris) in order (none empty), the light ranges tile [0, desc->num_lights) in order
 * (empty ones allowed), and light_ids[t] of an emissive triangle lies in its object's light range.
 * Hierarchies: every object's BVH2 / Tri1 is built on the device by rodent_hip_build_bvh2_tri1_opt over indices + 4 * first_tri (opt NULL:
 * max_leaf 2, no treelet passes), so a Tri1's prim_id is OBJECT-LOCAL and its geom_id the material; the builds are packed into one
 * allocation (all nodes, then, 256-byte aligned, all triangles) under a RodentObject table, child ids and leaf indices relative to each
 * object's own first record.  rodent_hip_scene_bvh returns the packed arrays and their total counts.
 * Instances: `instances` is a HOST array; instance ids are the descriptor indices 0 ... n - 1 (the instance_id word of the caller's
 * descriptors is ignored and overwritten).  Object ids are fixed for the life of the scene; only the matrices change afterwards
 * (rodent_hip_scene_set_transforms).  The top-level hierarchy is rodent_hip_build_tlas's with max_leaf 1.
 * Derived tables, all on the device, all rebuilt when the matrices move:
 *   TLAS and RodentInstance array   as rodent_hip_build_tlas writes them.
 *   slot_of[k]                       the leaf-order slot of instance k (one thread per slot j: slot_of[instance_id(j) & 0x7FFFFFFF] = j).
 *   bases[k] = {first_tri(o_k), light_base[k] - first_light(o_k)}, light_base = the exclusive prefix sum of num_lights(o_k) in instance
 *                                    order; built on the host at creation, never changes.
 *   world lights                     sum over k of num_lights(o_k) records (the scene's num_lights): light light_base[k] + j is object
 *                                    light first_light(o_k) + j under instance k; light_owner[l] = k is fixed.  fp32, every operation
 *                                    rounded on its own, m = the instance's object_to_world, w = its world_to_object:
 *     a corner (x, y, z) maps per row to ((m0*x + m1*y) + m2*z) + m3; its fourth word stays as stored;
 *     c = cross(v1' - v0', v2' - v0'), l = sqrt((c.x*c.x + c.y*c.y) + c.z*c.z), inv_area = 1.0f / (0.5f * l), the statements of
 *       rodent_hip_scene_refit_device;
 *     n = n' * (1.0f / sqrt((n'.x*n'.x + n'.y*n'.y) + n'.z*n'.z)), n' = N(n_obj) -- not the cross product of the mapped corners, which a
 *       mirroring matrix would flip to the dark side;  the colour is copied.
 *   N(n) = ((w0.x*n.x + w1.x*n.y) + w2.x*n.z, (w0.y*n.x + w1.y*n.y) + w2.y*n.z, (w0.z*n.x + w1.z*n.y) + w2.z*n.z): the transpose of
 *     world_to_object, i.e. the inverse transpose of the placement.
 * Shading an instanced hit (k_shade<.., true>): the ray's leaf-order slot j (a per-ray int32 array the traversal pass writes), the
 * RodentInstance at j, k = instance_id & 0x7FFFFFFF; gprim = bases[k].x + prim indexes every per-triangle table; the face normal is
 * normalize(N(fn)), the corner normals N(n_i) (NOT normalised), then the flat shader's lerp2 and normalize; org, dir, t, u, v are used as
 * they are (t parametrises both spaces); the emitter of a hit is world light bases[k].y + light_ids[gprim].  That is, bit for bit, the
 * flat shading of the scene baked into world space by those rules.
 * With an instanced scene loaded: the mapping in effect is streaming and trace_persistent, both refill thresholds and the sort by material
 * are 0 in effect, whatever was requested (the per-ray slot array is not moved by the sort; the `_in_effect` getters say so); the stream
 * traversal launches are k_trace_instanced<false> / <true> -- one ray per lane, one 64-entry LDS stack for both levels, no follow-up
 * kernel: a ray whose stack need exceeds rodent_instances.h's bound raises the renderer's overflow flag, on which a frame call aborts.
 * rodent_hip_scene_refit* abort on an instanced scene, as they do on no scene.
 *
 * Returns RODENT_SCENE_OK, or a negative status.  The refusals below are decided on the HOST, before anything is enqueued, and leave the
 * device's current scene as it is; a flag raised on the device (a builder's, RODENT_TLAS_BAD_TRANSFORM for a singular matrix) destroys
 * what was half built -- no scene is loaded then -- and returns RODENT_SCENE_ERR_DEVICE (the flags: rodent_hip_scene_create_flags). */
#define RODENT_SCENE_OK                0
#define RODENT_SCENE_ERR_COUNTS      -20   /* a NULL table, a count < 1, more than 2^22 instances, a hierarchy in the description */
#define RODENT_SCENE_ERR_RANGES      -21   /* the objects' triangle or light ranges do not tile the tables in order */
#define RODENT_SCENE_ERR_LIGHT       -22   /* an emissive triangle names a light outside its object's light range */
#define RODENT_SCENE_ERR_OBJECT      -23   /* an instance names an object outside the table */
#define RODENT_SCENE_ERR_NO_LIGHT    -24   /* no instance places an object that has a light */
#define RODENT_SCENE_ERR_OPTIONS     -25   /* invalid build options */
#define RODENT_SCENE_ERR_TABLE       -26   /* a vertex, material or texture index outside its table */
#define RODENT_SCENE_ERR_DEVICE      -27   /* the device raised a flag while building */
struct RodentObjectRange { int32_t first_tri, num_tris, first_light, num_lights; };   /* 16 B */
int32_t rodent_hip_scene_create_instanced(int32_t dev, const struct RodentSceneDesc* desc, const struct RodentObjectRange* objects,
                                          int32_t num_objects, const struct RodentInstanceDesc* instances, int32_t num_instances,
                                          const struct RodentBuildOptions* opt);
/* The flags of the last rodent_hip_scene_create_instanced that returned RODENT_SCENE_ERR_DEVICE on `dev` (0 otherwise). */
int32_t rodent_hip_scene_create_flags(int32_t dev);
/* The instances moved: object_to_world_dev holds n x 12 floats on the DEVICE, instance k's matrix at 12 k.  Enqueues on `stream`: the
 * copy of the matrices into the scene's descriptor array (the object and id words stay), rodent_hip_build_tlas into the scene's existing
 * buffers and scratch, slot_of, the world lights.  Allocates nothing, copies nothing to or from the host, does not wait for the device.
 * A later call, and a frame started afterwards on any stream, is ordered behind it with the event that orders frames behind
 * rodent_hip_scene_refit_device.  No instanced scene loaded or a NULL pointer aborts with a message. */
void    rodent_hip_scene_set_transforms(int32_t dev, const float* object_to_world_dev, void* stream);
/* Waits for the last rodent_hip_scene_set_transforms and copies the TLAS build's info words to info (RODENT_BUILD_INFO_WORDS ints, may
 * be NULL).  Returns its flags: 0 for a sound rebuild; never aborts.  Before the first call: the creation's words.  With a flag raised the
 * tables are undefined (rodent_instances.h): do not render before a sound rebuild. */
int32_t rodent_hip_scene_transforms_status(int32_t dev, int32_t* info);
/* DEVICE pointers and counts of an instanced scene's tables, for tests and tools; ray_slots is the per-ray slot array (ray_slot_capacity
 * ints; it covers the device's stream slabs as they are when this is called).  No instanced scene loaded aborts. */
struct RodentSceneInstances {
    struct Node2* tlas_nodes; struct RodentInstance* instances; struct RodentInstanceDesc* descs; struct RodentObject* objects;
    int32_t* slot_of; int32_t* bases /* int2 per instance */; int32_t* light_owner; struct RodentLight *lights, *object_lights;
    int32_t* ray_slots; int32_t* tlas_info;
    int32_t num_instances, num_objects, num_tlas_nodes, num_lights, num_object_lights, ray_slot_capacity;
};
void    rodent_hip_scene_instances(int32_t dev, struct RodentSceneInstances* out);
/* ---- geometry that deforms inside the objects of an instanced scene ----
 * Objects of a declared set D get moved vertices; their hierarchies are refitted once, however many instances place them
 * (rodent_instances.h: rodent_hip_refit_objects), and what hangs off the objects' boxes is rebuilt.  The rules are those of "moved
 * geometry that is already on the device" above, restricted to D (CPU model: tests/instanced_deform_model.py):
 *   face normals and tri_shade records   of the triangles in D's triangle ranges; every other triangle keeps its bytes.
 *   smooth vertex normals                of the vertices a triangle of D names, over the corners of ALL the scene's triangles that name
 *                                        the vertex, in ascending (t, k) order: a static triangle that shares the vertex contributes
 *                                        its stored face normal.  A vertex no triangle of D names keeps its bytes.
 *   object lights                        of D's light ranges: a light is bound to the lowest emissive triangle that names it (one of
 *                                        its own object's) and gets that triangle's record; a light nobody names and every light
 *                                        outside D's ranges keeps its bytes.
 *   hierarchies                          the listed objects' nodes and Tri1 records as rodent_hip_refit_objects writes them; the others'
 *                                        keep their bytes.  Topologies stay, so no ray's stack need changes.
 *   TLAS, instance array, slot_of, world lights   rebuilt from the refitted root boxes, the object lights and the matrices, as by
 *                                        rodent_hip_scene_set_transforms.
 * Rows of vertices_dev (and of normals_dev) that no object of D names must equal the scene's: the caller's contract, not checked.
 *
 * rodent_hip_scene_deform_prepare: one-time, synchronous.  Declares D = objects[0 .. num_objects) (a HOST array, any order) and
 * allocates, owned by the scene and freed with it: the range table, the refit's scratch and info words, D's bound lights and, with
 * smooth_normals != 0, D's vertices with their incidence lists.  Calling it again replaces the set.  Returns RODENT_SCENE_OK, or, leaving
 * the scene and an earlier set exactly as they are: RODENT_SCENE_ERR_NOT_INSTANCED (no instanced scene loaded), RODENT_SCENE_ERR_COUNTS
 * (NULL or num_objects < 1), RODENT_SCENE_ERR_OBJECT (an id outside the object table, or one listed twice). */
#define RODENT_SCENE_ERR_NOT_INSTANCED -28
int32_t rodent_hip_scene_deform_prepare(int32_t dev, const int32_t* objects, int32_t num_objects, int32_t smooth_normals);
/* D's geometry moved; all pointers are DEVICE pointers on `dev`.
 *   vertices_dev:        the whole concatenated table, num_vertices x 4 floats, object space; may be the scene's own table
 *                        (rodent_hip_scene_tables), then nothing is copied.
 *   normals_dev:         the whole table, or NULL: smooth normals of D's vertices are recomputed (the set must have been prepared for it).
 *   object_to_world_dev: NULL, or n x 12 floats as for rodent_hip_scene_set_transforms: the instances move too, with ONE TLAS rebuild.
 * Enqueues on `stream`, in this order: the wait for the last update or move, the copies, the matrices, D's face normals, D's light
 * records, D's vertex normals, rodent_hip_refit_objects over D in the scene's packed allocation, D's tri_shade records (when the scene
 * has the table), rodent_hip_build_tlas, slot_of, the world lights, the event.  After the prepare call it allocates nothing, copies
 * nothing to or from the host and does not wait for the device; later calls and frames are ordered behind it as behind
 * rodent_hip_scene_set_transforms.  No instanced scene, no declared set or a NULL vertices_dev aborts with a message. */
void    rodent_hip_scene_deform_device(int32_t dev, const float* vertices_dev, const float* normals_dev, const float* object_to_world_dev,
                                       void* stream);
/* Waits for the last rodent_hip_scene_deform_device and copies the refit's and the TLAS build's info words (RODENT_BUILD_INFO_WORDS ints
 * each, may be NULL).  Returns 0 for a sound update, else the refit's flags | the TLAS flags, with bit 31 set when the refit completed
 * fewer nodes than D holds.  Never aborts on a flag; with one raised the tables are undefined until a sound call.  Before the first
 * call: 0, a sound refit's words and the last TLAS build's. */
int32_t rodent_hip_scene_deform_status(int32_t dev, int32_t* refit_info, int32_t* tlas_info);
/* ---- moving instances in the renderer: a time per path through the motion TLAS of rodent_instances.h ----
 * CPU model of everything below: tests/motion_scene_model.py (over tests/motion_instance_model.py, tests/instanced_scene_model.py and the
 * flat oracle).  A moving scene is an instanced scene whose instances carry TWO placements, M0 at time 0 and M1 at time 1
 * (RodentMotionInstanceDesc); every path draws one time in the shutter interval and sees every instance where that time puts it.
 *
 * The time costs no stream word.  With a moving scene loaded,
 *   PrimaryStream::depth[i]    holds depth | ubits << RODENT_MOTION_DEPTH_BITS: bits 0 .. 7 the depth, bits 8 .. 30 the 23 mantissa bits of
 *                              the path's shutter sample u = randf(&rnd) = ubits * 2^-23 (exactly), bit 31 zero.  Every kernel that
 *                              copies a primary ray (the sort's and the compaction's k_scatter, the shader's fused compaction) carries
 *                              the word as it stands.
 *   SecondaryStream::prim_id[i] holds the shadow ray's time as float bits (no other kernel of the library reads or writes that array).
 * Shutter: t = fminf(close, open + (close - open) * u), the difference, the product and the sum each rounded in fp32, no fma; so
 * open <= t <= close, inside [0, 1], where rodent_instances.h's motion boxes contain; (0, 1), the default, gives t == u bit for bit.
 * Every kernel that needs t recomputes it from ubits and the pair.
 * Generation: after the two draws of the pixel sample a THIRD randf(&rnd) is u; the stored rnd is the state behind that draw and the
 * stored depth word is ubits << 8.  Pixel, origin, direction, tmin, tmax are the flat generation's.
 * Path length: the length in effect is min(requested, RODENT_MOTION_DEPTH_MASK) while a moving scene is loaded (depth never exceeds it,
 * so depth + 1 never carries into the time bits); a flat or static instanced scene loaded afterwards gets what was requested again.
 * Traversal (k_trace_instanced_motion<false|true>): k_trace_instanced's loop and stream I/O; for record j and a ray at time t (from
 * depth[i] >> 8 by the shutter rule in the closest-hit pass, prim_id[i] as float bits in the shadow pass) m = lerp(M0, M1, t) and
 * w = invert(m) by rodent_instances.h's rules; an instance whose interpolated matrix the inverse refuses is skipped for that ray: nothing
 * is pushed, tmax and the hit stay.
 * Shading a moving hit: the slot j from the per-ray slot array, the RodentMotionInstance at j, t from the depth word,
 * w = invert(lerp(M0, M1, t)) -- the function and the inputs of the traversal, hence its 12 floats --, then the instanced shading rules
 * with w and bases[k].  The depth test uses word & 0xFF; the ray that goes on gets (depth + 1) | ubits << 8, the shadow ray the bits of
 * t in prim_id.
 * Lights stay static: an instance whose object has num_lights > 0 must have object_to_world0 == object_to_world1 byte for byte
 * (RODENT_SCENE_ERR_MOVING_LIGHT otherwise).  The world light table is the static one derived from M0: the corners by the world-box rule
 * under M0, n = normalize(N(n_obj)) with w = invert(M0) computed where the lights are derived (a motion record stores no inverse),
 * inv_area and colour as before.  The TRAVERSAL reaches such an emitter through lerp(M0, M0, t) = s * m + t * m, which equals M0 only up
 * to the rounding of that sum (at t = 0 and t = 1 exactly): an emitter's surface as rays hit it and its light record as next-event
 * estimation samples it may differ in the last bits.  The model restates exactly this.
 * Derived tables: slot_of, bases, light_owner as for an instanced scene; the per-ray slot array is the same one.
 * Options in effect are those of an instanced scene (streaming mapping, no persistent kernels, no refill, no sort); overlap and all three
 * fused_compact modes work.  The stage-level entries (hip_generate_rays, hip_traverse_primary / _secondary / _streams, hip_shade,
 * hip_shade_compact, hip_compact_primary) work on a moving scene through the same branches, on streams that hold these words.
 * rodent_hip_scene_set_transforms, _scene_instances, _scene_deform_* and _scene_refit* treat a moving scene
 * as they treat "no instanced scene" (abort, or RODENT_SCENE_ERR_NOT_INSTANCED): objects that deform under the motion TLAS are not built
 * (a single mesh that deforms is: "deforming meshes in the renderer" below).
 *
 * rodent_hip_scene_create_motion: rodent_hip_scene_create_instanced with RodentMotionInstanceDesc records and rodent_hip_build_motion_tlas
 * (max_leaf 1): the same refusals in the same order, then RODENT_SCENE_ERR_MOVING_LIGHT, all on the host, leaving the loaded scene alone;
 * a device flag (either endpoint singular: RODENT_TLAS_BAD_TRANSFORM) returns RODENT_SCENE_ERR_DEVICE, the flags through
 * rodent_hip_scene_create_flags. */
#define RODENT_MOTION_DEPTH_BITS       8
#define RODENT_MOTION_DEPTH_MASK       0xFF
#define RODENT_SCENE_ERR_MOVING_LIGHT -29   /* an instance of an object with lights has object_to_world0 != object_to_world1 */
#define RODENT_SCENE_ERR_SHUTTER      -30   /* not 0 <= open <= close <= 1 (a NaN included) */
int32_t rodent_hip_scene_create_motion(int32_t dev, const struct RodentSceneDesc* desc, const struct RodentObjectRange* objects,
                                       int32_t num_objects, const struct RodentMotionInstanceDesc* instances, int32_t num_instances,
                                       const struct RodentBuildOptions* opt);
/* Both placements moved: m0_dev / m1_dev hold n x 12 floats each on the DEVICE (they may be the same pointer).  The launch list and the
 * promises of rodent_hip_scene_set_transforms: the matrices into the descriptor array, rodent_hip_build_motion_tlas into the scene's
 * buffers, slot_of, the world lights (from M0), the event; nothing allocated, no host copy, no wait.  rodent_hip_scene_transforms_status
 * serves it too.  The static-light rule cannot be checked without a host copy: the CALLER keeps the two keys of every emitter equal.  No
 * moving scene loaded or a NULL pointer aborts with a message. */
void    rodent_hip_scene_set_motion_transforms(int32_t dev, const float* m0_dev, const float* m1_dev, void* stream);
/* DEVICE pointers and counts of a moving scene's tables, for tests and tools (as rodent_hip_scene_instances).  No moving scene aborts. */
struct RodentSceneMotionInstances {
    struct Node2* tlas_nodes; struct RodentMotionInstance* instances; struct RodentMotionInstanceDesc* descs; struct RodentObject* objects;
    int32_t* slot_of; int32_t* bases /* int2 per instance */; int32_t* light_owner; struct RodentLight *lights, *object_lights;
    int32_t* ray_slots; int32_t* tlas_info;
    int32_t num_instances, num_objects, num_tlas_nodes, num_lights, num_object_lights, ray_slot_capacity;
};
void    rodent_hip_scene_motion_instances(int32_t dev, struct RodentSceneMotionInstances* out);
/* The shutter of device `dev` (default (0, 1); rodent_hip_render_defaults restores it).  Anything but 0 <= open <= close <= 1 returns
 * RODENT_SCENE_ERR_SHUTTER and changes nothing.  Without a moving scene it has no effect. */
int32_t rodent_hip_render_shutter(int32_t dev, float open, float close);
void    rodent_hip_render_shutter_in_effect(int32_t dev, float out[2]);
/* The path length the next frame uses: min(requested, 255) with a moving or a deforming scene loaded, else what rodent_hip_render_config
 * was given. */
int32_t rodent_hip_render_max_path_len_in_effect(int32_t dev);
/* ---- deforming meshes in the renderer: a time per path through the motion BVH of rodent_motion.h ----
 * CPU model of everything below: tests/deforming_scene_model.py (over tests/motion_bvh_model.py, tests/scene_update_model.py,
 * tests/motion_scene_model.py and the flat oracle).  A deforming scene is a flat scene that owns TWO keys, its vertex and normal tables at
 * time 0 and at time 1; every path draws one time in the shutter interval and sees the mesh as that time puts it, vertex by vertex.
 *
 * The time travels as in a moving scene (above), word for word: PrimaryStream::depth[i] holds depth | ubits << 8,
 * SecondaryStream::prim_id[i] a shadow ray's time as float bits, the shutter rule gives t, generation draws the third randf, the path
 * length in effect is min(requested, RODENT_MOTION_DEPTH_MASK).
 * Traversal (k_trace_deforming<false|true>): rodent_motion.h's records and rules over the stream I/O of an instanced scene's passes.  For
 * a ray at time t: s = 1 - t once, every bound and every Tri1 float x = s*x0 + t*x1.  The hit record holds key 0's geom_id and prim_id
 * words (prim_id indexes the scene's tables directly); a miss is {num_geometries, -1, tmax as given, 0, 0}.  rodent_motion.h's time rule
 * holds for the stage-level entries, which let a caller write any word: a closest-hit ray with !(0 <= t && t <= 1) stores the miss
 * record without traversal, a shadow ray outside is not occluded and adds its colour (inside the library's own loop t lies in the
 * shutter interval, so the rule never acts there).  A stack overflow raises the flag a frame call aborts on.
 * Shading a deforming hit: t from the depth word, s = 1 - t, lerp(x0, x1) = s*x0 + t*x1 with every operation rounded on its own:
 *   corners       through the index row, v_k(t) = lerp of the two vertex tables' rows, three floats each;
 *   face normal   the moved-geometry rule above on those corners: a = v1(t) - v0(t), b = v2(t) - v0(t), c = a x b,
 *                 l = sqrt((c.x c.x + c.y c.y) + c.z c.z), fn = c * (1.0f / l).  NOT the interpolation of the keys' face normals: a
 *                 triangle that turns over between the keys changes side at the time it is flat, as the traversal's own
 *                 n = cross(e1(t), e2(t)) does;
 *   corner normals n_k(t) = lerp of the two normal tables' rows, NOT normalised; the flat shader's lerp2 and normalize follow;
 *   the rest      org, dir, t, u, v, the point, the material and the textures (prim indexes the tables directly) are the flat shader's;
 *                 the emitter of a hit is lights[light_ids[prim]].
 * This is, bit for bit, the flat shading of the scene baked at the hit's time by those rules.  The depth test uses word & 0xFF; the ray
 * that goes on gets (depth + 1) | ubits << 8, the shadow ray the bits of t in prim_id.
 * Lights stay static: an emissive triangle whose three corner rows (16 bytes each) differ in a byte between the keys is refused
 * (RODENT_SCENE_ERR_MOVING_LIGHT).  The light table is key 0's.  The TRAVERSAL reaches such an emitter through s*x + t*x, which equals x
 * only up to the rounding of that sum (at t = 0 and t = 1 exactly): an emitter's surface as rays hit it and its light record as
 * next-event estimation samples it may differ in the last bits.  The model restates exactly this.
 * Options in effect are those of a moving scene (streaming mapping, no persistent kernels, no refill, no sort); overlap and all three
 * fused_compact modes work.  No LDS top images and no tri_shade / tri_tex records are built (rodent_hip_scene_tables returns NULL for
 * them).  rodent_hip_scene_refit*, _scene_deform_*, _scene_set_transforms, _scene_set_motion_transforms, _scene_instances and
 * _scene_motion_instances treat a deforming scene as they treat "no such scene" (abort, or RODENT_SCENE_ERR_NOT_INSTANCED).  Neither
 * moving emitters, nor more than two keys, nor motion objects under the motion TLAS are built.
 *
 * rodent_hip_scene_create_deforming: `desc` as for rodent_hip_scene_create_device_bvh_opt (HOST tables, nodes / tris NULL, counts 0; its
 * vertices / normals are the mesh at time 0), vertices1 / normals1 HOST tables of num_vertices float4 rows, the mesh at time 1; opt NULL =
 * max_leaf 2, no passes.  Uploads the tables, builds the topology on the device from key 0 (rodent_hip_build_bvh2_tri1_opt) and the
 * motion records over it (rodent_hip_build_motion_bvh2_tri1) into records and scratch the scene owns.  The static key-0 hierarchy stays
 * in the scene as the read-only topology of later rebuilds (rodent_hip_scene_bvh returns it); no frame walks it.
 * Returns RODENT_SCENE_OK or, decided on the host and leaving the loaded scene alone, in this order: RODENT_SCENE_ERR_COUNTS (a NULL
 * table, a count < 1, a hierarchy in the description), RODENT_SCENE_ERR_OPTIONS, RODENT_SCENE_ERR_TABLE (a vertex, material, texture or
 * light index outside its table) or RODENT_SCENE_ERR_LIGHT (an emissive triangle without an entry in the light table) for the first
 * triangle that has either, RODENT_SCENE_ERR_MOVING_LIGHT.  A flag raised on the device, the builder's or the motion build's (a
 * non-finite coordinate at either key: RODENT_BUILD_NON_FINITE), destroys what was half built -- no scene is loaded then -- and returns
 * RODENT_SCENE_ERR_DEVICE, the flags through rodent_hip_scene_create_flags. */
int32_t rodent_hip_scene_create_deforming(int32_t dev, const struct RodentSceneDesc* desc, const float* vertices1, const float* normals1,
                                          const struct RodentBuildOptions* opt);
/* Both keys moved; all pointers are DEVICE pointers on `dev`: num_vertices x 4 floats each.  A key may be the scene's own table of that
 * key (rodent_hip_scene_motion_keys), written in place: then nothing is copied; the two keys may be one pointer.  normals0_dev /
 * normals1_dev: both given, or both NULL: smooth normals are recomputed per key by rodent_hip_scene_refit_device's rule and kernels (face
 * normals of the key, summed over each vertex's incidence list; the lists were prepared at creation).
 * Enqueues on `stream`, in this order: the wait for the last update, the copies, the normals, rodent_hip_build_motion_bvh2_tri1 over the
 * static topology into the scene's records with its scratch, the event.  After creation it allocates nothing, copies nothing to or from
 * the host and does not wait; a frame started afterwards on any stream is ordered behind it.  The emitter rule cannot be checked without a
 * host copy: the CALLER keeps the corner rows of every emissive triangle equal between the keys (and equal to the creation's: the light
 * table is not rederived).  No deforming scene loaded, NULL vertices or one table of normals without the other aborts with a message. */
void    rodent_hip_scene_set_motion_keys(int32_t dev, const float* vertices0_dev, const float* vertices1_dev, const float* normals0_dev,
                                         const float* normals1_dev, void* stream);
/* Waits for the last rodent_hip_scene_set_motion_keys (before the first: nothing to wait for, the creation's words) and copies the four
 * info words of rodent_hip_build_motion_bvh2_tri1 (may be NULL).  Returns its flags, with bit 31 set when info[0] or info[3] differs from
 * the node count (and for "no deforming scene loaded").  Never aborts; with a flag raised the records are undefined until a sound call. */
int32_t rodent_hip_scene_motion_keys_status(int32_t dev, int32_t* info);
/* DEVICE pointers and counts of a deforming scene's motion records, and of its key tables, for tests and tools.  No deforming scene
 * aborts. */
void    rodent_hip_scene_motion_bvh(int32_t dev, const struct RodentMotionNode2** nodes, const struct RodentMotionTri1** tris,
                                    int32_t* num_nodes, int32_t* num_tris);
struct RodentSceneMotionKeys { float *vertices0, *vertices1, *normals0, *normals1; int32_t* info; int32_t num_vertices; };
void    rodent_hip_scene_motion_keys(int32_t dev, struct RodentSceneMotionKeys* out);
void    rodent_hip_render_config(int32_t dev, int32_t spp, int32_t max_path_len);   /* defaults 4 / 64 (converter.cpp:1007-1012) */
/* 0 = streaming wavefront loop (src/render/mapping_gpu.impala:308-369), 1 = persistent-threads megakernel
 * (mapping_gpu.impala:371-474; the reference selects it at configure time with the converter target
 * amdgpu-megakernel / nvvm-megakernel, converter.cpp:30-35,1032-1037; `rodent --target amdgpu-megakernel` here),
 * -1 (default) = chosen per scene when the scene is created: the megakernel for hierarchies of at most
 * RODENT_HIP_AUTO_MEGA_MAX_NODES inner nodes (default 128: the whole tree sits in the traversal kernels' LDS image and the
 * wavefront formulation's stream traffic is all that is left to save; the Cornell box renders 1.45 x faster that way), the
 * streaming loop for larger scenes (1.05 x faster at 306 nodes, 1.4-1.5 x from 5 000 nodes on: profiles/r03_mapping_sweep.txt).  The
 * initial value can also be set with the environment variable
 * RODENT_HIP_MAPPING=auto|streaming|mega.  rodent_hip_render_mapping_in_effect: 0 / 1, what the next frame will use. */
void    rodent_hip_render_mapping(int32_t dev, int32_t mapping);
int32_t rodent_hip_render_mapping_in_effect(int32_t dev);
/* Every rodent_hip_render_* option of the device back to its default, or to what its RODENT_HIP_* environment variable says
 * (the values a fresh process starts with); spp / max_path_len and the scene are kept. */
void    rodent_hip_render_defaults(int32_t dev);
/* Rays per ray stream of the streaming mapping: the reference's constant 1 Mi (mapping_gpu.impala:319) is 32 Mi here
 * by default (larger launches amortise their fill and drain on a 256-CU chip: 7.1 GB of streams out of 288 GB; 0 restores the default). */
void    rodent_hip_render_capacity(int32_t dev, int32_t rays);
/* 1: hit rays are sorted by material before shading and misses dropped, as in the reference (mapping_gpu.impala:166-221,347-357:
 * there every material is its own generated shader and the sort is what makes a launch per material possible).
 * 0 (default): no sort -- the shader here is ONE table-driven kernel; it runs in stream order and ends the rays that missed; one
 * stream copy less per bounce.  Measured on every scene at hand (profiles/r03_sort_sweep.txt: Cornell, the atrium, a room with
 * every BSDF kind on neighbouring walls, a textured room) the unsorted loop is 5 ... 22 % faster, so it is the default; the sort
 * stays one call away.  Same paths, same ray counts; RODENT_HIP_SORT=0|1 sets the initial value, `rodent --sort` / `--no-sort`. */
void    rodent_hip_render_sort(int32_t dev, int32_t enable);
int32_t rodent_hip_render_sort_in_effect(int32_t dev);       /* 0 / 1: what the next frame does (0 for an instanced scene) */
/* Hit records inside the library's own wavefront loop: 1 (default) = one 20-byte record per ray in the memory of the stream's geom_id /
 * prim_id / t / u / v arrays (one 16-byte + one 4-byte store per record instead of five scattered 4-byte stores: the traversal launches'
 * write traffic), 0 = the ABI's five arrays.  The stage-level entry points (hip_traverse_primary, hip_shade, ...) always use the five
 * arrays, and so does the loop when the sort by material is on.  RODENT_HIP_HIT_AOS. */
void    rodent_hip_render_hit_records(int32_t dev, int32_t aos);
/* 1 (default): the shadow rays of a bounce are traced on a second HIP stream beside the compaction, regeneration and the
 * next closest-hit pass; 0: one stream.  Same film up to the order of the atomic adds.  RODENT_HIP_OVERLAP=0|1.
 * (Without effect while the joint traversal launch is in use, rodent_hip_render_trace_persistent below: that loop has one stream.) */
void    rodent_hip_render_overlap(int32_t dev, int32_t enable);
/* 0 (default): rays are moved by the sort (copy_primary_ray, mapping_gpu.impala:136-164) and shaded in place.  1: the sort by
 * material only computes the permutation; the shader gathers its rays through it and writes the sorted stream (one copy of the
 * 18-word stream per bounce less, but a gathering shader: measured 3 % slower on the Cornell box, equal on the atrium).
 * Same paths and film.  RODENT_HIP_FUSED_SORT=0|1. */
void    rodent_hip_render_fused_sort(int32_t dev, int32_t enable);
/* Compaction as part of the shader: every ray that goes on is written straight to its compacted slot of the other stream, one
 * read + write of the 15-word stream per bounce less than shading in place and compacting afterwards.
 * 2 (default): a block of 256 rays takes its slots from one atomic counter (order of the blocks in the new stream = order
 * of arrival; inside a block stream order; the reference's own compaction takes one atomic per RAY, mapping_gpu.impala:293).
 * 1: slots from a single-pass block scan with decoupled look-back -- the stable order of the separate pass, reproducible
 * from run to run, but every block waits for its 64 predecessors (measured: the shader 290 -> 535 us per 8 Mi rays).
 * 0: shade in place, then the separate compaction pass (gpu_compact_primary, mapping_gpu.impala:267-300).
 * Same rays in the stream either way, same film up to the order of the atomic adds.  RODENT_HIP_FUSED_COMPACT=0|1|2. */
void    rodent_hip_render_fused_compact(int32_t dev, int32_t enable);
/* 1 (default): the stream traversal kernels run as 2-wave workgroups that stage the first 31 inner nodes of the scene's BVH
 * (breadth first, built at scene creation) in LDS and fetch those with ds_read instead of through the vector-memory pipeline.
 * 0: one wave per workgroup, every node from memory (rounds 1-2).  Same per-ray visit order, same film.  RODENT_HIP_LDS_IMAGE=0|1. */
void    rodent_hip_render_lds_image(int32_t dev, int32_t enable);
/* Megakernel mapping.  0 (default): the reference's sequence of loops (closest hit, shade, shadow; mapping_gpu.impala:371-474).
 * 1: a lane traces the shadow ray of its path vertex and the path's next ray back to back in ONE wave-level loop (a wave needs max
 * over its lanes of the SUM of the two rays' steps instead of the sum of two maxima) -- measured 6 ... 14 % SLOWER (a path that ends
 * with a shadow ray pending holds its lane for one more loop): an option, not the default.
 * Same paths, same ray counts, same film up to the order of the atomic adds.  RODENT_HIP_MEGA_JOINT=0|1. */
void    rodent_hip_render_mega_joint(int32_t dev, int32_t enable);
/* The stream traversal launches of the streaming loop.
 * 0: 2-wave workgroups with a 31-node image (rodent_hip_render_lds_image), the shadow pass on a second stream (rodent_hip_render_overlap).
 * 1: persistent form (one resident generation of 16-wave workgroups, the first 255 inner nodes in LDS, 64-ray chunks drawn from
 *    striped ticket counters -- traversal.hip's default mapping) for streams of at least 524 288 rays.
 * 2: joint -- the shadow pass of an iteration rides in the NEXT iteration's closest-hit launch: one persistent kernel works through
 *    both ray lists (they depend on the same shader run and on nothing else), one stream, no pass waits for the other's tail.
 * -1 (default): per scene -- 2 for every hierarchy the per-scene mapping rule sends to the streaming loop (+3 ... +9 % on the atrium at
 *    306 ... 142 444 nodes, profiles/r03_joint_sweep.txt), 0 for a tree of a few dozen nodes (Cornell box: 2 is 5 % slower).
 * Same film.  RODENT_HIP_TRACE_PERSISTENT=-1|0|1|2. */
void    rodent_hip_render_trace_persistent(int32_t dev, int32_t enable);
int32_t rodent_hip_render_trace_persistent_in_effect(int32_t dev);   /* 0 / 1 / 2 for the scene that is loaded (0 for an instanced one) */
/* Lane refill in the persistent traversal launches (1 and 2 above).  Thresholds 1 .. 64: a wave whose idle lanes reach that count
 * retires their rays and draws as many new ones from its stripe's counter instead of waiting for the last ray of a 64-ray chunk
 * (k_trace_refill) -- idle_bounce while it draws from the rays the last bounce left, idle_shadow while it draws shadow rays (64 =
 * whole chunks for that kind); the camera rays a launch holds (the host knows where: the rays generated for it) always go chunk
 * by chunk.  0, 0: whole chunks for everything (k_trace_persist).  -1, -1 (default): per scene -- 40, 40 for hierarchies of 16 384
 * nodes and more (atrium: +8 % at 1920 x 1080 x 16 spp, +9 % at 3840 x 2160 x 32 spp; profiles/r03_refill_sweep.txt), off below
 * (every ray is short there: -4 ... -11 %).  Same paths, same ray counts, same film up to the order of the atomic adds.
 * RODENT_HIP_TRACE_REFILL=<both> or <bounce>,<shadow>. */
void    rodent_hip_render_trace_refill(int32_t dev, int32_t idle_bounce, int32_t idle_shadow);
/* idle_bounce | idle_shadow << 8 for the scene that is loaded (0 = whole chunks) */
int32_t rodent_hip_render_trace_refill_in_effect(int32_t dev);
/* In those launches a closest-hit ray's miss record is stored when the ray retires without an accepted triangle (RODENT_HIP_LAZY_MISS=1,
 * the default; 0 = up front, when the ray starts), and a shadow ray that hits both children of a node goes on with child 0
 * (RODENT_HIP_SHADOW_ORDER=1, the default; 0 = the nearer child, 2 = the farther one).  Both are read once per process and every
 * combination has its own kernel: the shadow order does not change which form of the miss record is used.  Either way a miss record is
 * {num_geometries, -1, tmax, 0, 0} with tmax bit for bit as the stream holds it (a NaN's payload, a denormal). */
/* The ray count from which a lone pass takes the persistent kernels (1, 2 above) and from which the loop lets a pending shadow pass ride
 * in the next closest-hit launch: 524 288 by default (below one resident generation of rays the persistent form does not pay); rays < 0
 * restores that, as does rodent_hip_render_defaults.  The renderer's counterpart of rodent_hip_top_min_rays: with 0 a test reaches the
 * persistent kernels with a handful of rays.  Chooses kernels only: same records, same film. */
void    rodent_hip_render_persist_min_rays(int32_t dev, int32_t rays);
int32_t rodent_hip_render_persist_min_rays_in_effect(int32_t dev);
/* The main kernel of the device's newest stream traversal launch (the loop's or a stage-level call's), as the sources spell it:
 * "k_trace_primary<2,31>", "k_trace_secondary<1,0>", "k_trace_persist<2>", "k_trace_refill<1,true>" (shadow order, lazy miss record), ...;
 * "" before the first launch.  A static string. */
const char* rodent_hip_render_trace_kernel_name(int32_t dev);

/* ---- the reference's renderer ABI ---- */
int32_t get_spp(void);
void    render(const struct Settings* settings, int32_t iter);       /* one frame: spp samples per pixel, accumulated into the film */
void    setup_interface(size_t width, size_t height);
float*  get_pixels(void);                                            /* host film, width*height*3 floats, valid after rodent_present */
void    clear_pixels(void);
void    cleanup_interface(void);
void    rodent_get_film_data(int32_t dev, float** pixels, int32_t* width, int32_t* height);   /* DEVICE film */
void    rodent_gpu_get_first_primary_stream(int32_t dev, struct PrimaryStream* primary, int32_t size);
void    rodent_gpu_get_second_primary_stream(int32_t dev, struct PrimaryStream* primary, int32_t size);
void    rodent_gpu_get_secondary_stream(int32_t dev, struct SecondaryStream* secondary, int32_t size);
void    rodent_gpu_get_tmp_buffer(int32_t dev, int32_t** buf, int32_t size);
void    rodent_present(int32_t dev);                                 /* film device -> host */
/* Scene-data services (src/driver/interface.cpp:432-492,584-619; prototypes src/render/driver.impala:11-16): load one of the
 * reference converter's files onto device `dev` and return DEVICE pointers.  Results are cached by (dev, file name), owned
 * by the library and valid until cleanup_interface(); a missing or malformed file prints a message and abort()s like the
 * reference's error().  `dev` is the HIP device index (there is no host device 0 here: nothing is computed on the CPU). */
/* one LZ4 buffer file (data/vertices.bin, ...; src/driver/buffer.h) */
uint8_t* rodent_load_buffer(int32_t dev, const char* file);
/* the matching layout of data/bvh.bin */
void    rodent_load_bvh2_tri1(int32_t dev, const char* file, struct Node2** nodes, struct Tri1** tris);
void    rodent_load_bvh4_tri4(int32_t dev, const char* file, struct Node4** nodes, struct Tri4** tris);
void    rodent_load_bvh8_tri4(int32_t dev, const char* file, struct Node8** nodes, struct Tri4** tris);
/* RGBA8, rows flipped, gamma 2.2 (image.cpp:10-18,85) */
void    rodent_load_png(int32_t dev, const char* file, uint8_t** pixels, int32_t* width, int32_t* height);
void    rodent_load_jpg(int32_t dev, const char* file, uint8_t** pixels, int32_t* width, int32_t* height);
/* Host-side stream slabs with the device slabs' carving, one per calling thread (interface.cpp:341-342,367-373,621-629). */
void    rodent_cpu_get_primary_stream(struct PrimaryStream* primary, int32_t size);
void    rodent_cpu_get_secondary_stream(struct SecondaryStream* secondary, int32_t size);
int64_t clock_us(void);                                              /* interface.cpp:665-673 */

/* ---- additions ---- */
/* Sizes of what the services above loaded (the reference's generated code knows them at compile time):
 * bytes of a loaded buffer (-1 if `file` was not loaded on `dev`); node / primitive counts of a loaded BVH layout. */
int64_t rodent_hip_buffer_size(int32_t dev, const char* file);
void    rodent_hip_bvh_counts(int32_t dev, const char* file, int32_t bvh_width, int32_t* num_nodes, int32_t* num_tris);
void    rodent_hip_set_device(int32_t dev);                          /* device used by render() (the reference bakes it in) */
/* Renders only image rows [y0, y1) (tile sharding across GPUs: seeds depend on absolute (sample, iter, x, y),
 * renderer.impala:28-33, so any tiling reproduces the same samples).  The work is enqueued on `stream`; the call RETURNS WHEN THE
 * ROWS ARE IN THE DEVICE FILM: the wavefront loop reads the stream size back every iteration (as the reference does,
 * mapping_gpu.impala:344-366), so it cannot be asynchronous. */
void    rodent_hip_render_rows(int32_t dev, const struct Settings* settings, int32_t iter, int32_t y0, int32_t y1, void* stream);
/* Renders the interleaved row tiles first_tile, first_tile + tile_stride, ... of tile_rows rows each (the last tile of the film may be
 * shorter): GPU k of K takes first_tile = k, tile_stride = K, which balances the GPUs where contiguous bands do not (SURVEY 8e;
 * the reference deals ~1024-sample tiles dynamically, render/mapping_gpu.impala:374-420).  Same samples, same film as
 * rodent_hip_render_rows over the same rows; synchronous like it. */
void    rodent_hip_render_tiles(int32_t dev, const struct Settings* settings, int32_t iter, int32_t tile_rows, int32_t first_tile,
    int32_t tile_stride, void* stream);
/* Counters of the last render call on this device (render, rodent_hip_render_rows, rodent_hip_render_tiles -- the whole call, however
 * many launches it took): [0] primary rays traced, [1] shadow rays traced, [2] wavefront iterations, [3] rays generated. */
void    rodent_hip_render_counters(int32_t dev, uint64_t* out4);

/* The wavefront stages as separate entry points (the reference's device kernels,
 * src/render/mapping_gpu.impala:18-30,47-80,82-134,166-221,223-265,267-300); all asynchronous on `stream`. */
void    hip_generate_rays(int32_t dev, struct PrimaryStream* primary, int32_t capacity, int32_t first_ray_id, int32_t num_rays,
                          const struct Settings* settings, int32_t iter, int32_t film_width, int32_t film_height,
                          int32_t first_pixel, int32_t spp, void* stream);
void    hip_traverse_primary(int32_t dev, struct PrimaryStream* primary, void* stream);
/* Sorts by geometry id into `other` (stable, deterministic); ray_ends[g] (host, num_geometries+1 ints) receives the
 * exclusive end of bin g like mapping_gpu.impala:203-207.  Synchronises the stream (the reference does too). */
void    hip_sort_primary(int32_t dev, struct PrimaryStream* primary, struct PrimaryStream* other, int32_t* ray_ends, void* stream);
void    hip_shade(int32_t dev, struct PrimaryStream* primary, struct SecondaryStream* secondary, int32_t num_rays, void* stream);
/* The shader in the forms the renderer's own loop launches (rodent_hip_render_fused_sort / _fused_compact): thread i shades ray perm[i]
 * of `from` (perm: DEVICE array of num_rays stream indices, or NULL: ray i), writes its shadow ray at index i of `secondary` and the
 * ray that goes on to its compacted slot of `to` (another stream than `from`, which is left as it is).  mode 1: slots from the look-back
 * scan (stable order), 2: one atomic per workgroup (workgroups in order of arrival).  block: rays per workgroup, 256 / 512 / 1024, 0 =
 * the library's (RODENT_HIP_SHADE_BLOCK).  Rays that missed end here, as in hip_shade.  Returns the new size, also in to->size
 * (synchronises the stream).  Invalid arguments abort. */
int32_t hip_shade_compact(int32_t dev, struct PrimaryStream* from, struct PrimaryStream* to, struct SecondaryStream* secondary,
                          const int32_t* perm, int32_t num_rays, int32_t mode, int32_t block, void* stream);
void    hip_traverse_secondary(int32_t dev, struct SecondaryStream* secondary, void* stream);
/* One stream traversal launch as the renderer's own loop makes it, over a closest-hit pass, a shadow pass, or both in ONE persistent
 * launch (the joint form, whatever rodent_hip_render_trace_persistent says); asynchronous on `stream`.
 * primary / secondary: either may be NULL (that pass is absent); a stream of size 0 is an absent pass too.
 * coherent_from: the closest-hit rays [coherent_from, primary->size) are coherent (camera rays: the lane refill takes them chunk by chunk),
 *   the ones in front of them are not; < 0 = unknown (what hip_traverse_primary passes: a lone closest-hit pass then never refills).
 *   Records do not depend on it.
 * shadow_size_dev: NULL, or a DEVICE int in [0, secondary->size] that the kernels read when they run: only the shadow rays in front of it
 *   are traced, counted and added to the film (the loop's shadow pass behind the sort); the grid covers secondary->size.
 * flags: bit 0 = hit records as 20-byte records {geom_id, prim_id, t, u, v} at words [5 i, 5 i + 5) of the memory that starts at
 *   primary->geom_id, instead of the ABI's five arrays (rodent_hip_render_hit_records).  Needs a stream whose arrays lie one capacity
 *   apart in the order of the struct, as rodent_gpu_get_*_primary_stream carves them.  The caller's struct is not written.
 * Which kernel runs follows the device's options as in the loop (rodent_hip_render_trace_persistent, _trace_refill, _lds_image,
 * _persist_min_rays; the lane refill also needs both streams carved as above): rodent_hip_render_trace_kernel_name tells.
 * Returns 0, or a negative status WITHOUT enqueueing anything: -1 both passes NULL, -2 unknown flag bits or a negative size,
 * -3 coherent_from > primary->size, -4 bit 0 on a stream that is not carved that way. */
int32_t hip_traverse_streams(int32_t dev, struct PrimaryStream* primary, int32_t coherent_from, struct SecondaryStream* secondary,
                             const int32_t* shadow_size_dev, int32_t flags, void* stream);
/* Order-preserving compaction of rays with id >= 0; returns the new size (synchronises the stream). */
int32_t hip_compact_primary(int32_t dev, struct PrimaryStream* primary, struct PrimaryStream* other, void* stream);
/* The binning stage in the forms the renderer's own loop launches (hip_sort_primary and hip_compact_primary are two of them): stable
 * counting sort of the first n rays of `from` by key, n = *size_dev (DEVICE int) if size_dev is given, else max_n.
 * mode 0: key = geom_id, 1: key = (id >= 0 ? 0 : 1).  num_bins: number of keys, 1 ... 1025 (an argument, not the scene's material count:
 * no scene has to be loaded).  Rays with key >= drop_from_bin (1 ... num_bins) are left out; ray i with a smaller key goes to slot
 * d = (rays with a smaller key) + (rays with its key in front of it).
 * perm == NULL: every array of `to` (another stream than `from`) takes from[i] at d, except the five hit arrays when keep_hit == 0 and
 * tmin / tmax when copy_interval == 0; those, and every entry behind the rays kept, stay as they are.
 * perm != NULL (DEVICE array of at least as many ints as rays are kept): perm[d] = i and `to` is not written at all (index-only sort).
 * The loop's sort is (0, G + 1, G, 1, 0, perm or NULL, NULL, n), its compaction (1, 2, 1, 0, 1, NULL, size_dev, max_n).
 * bin_ends (host, num_bins ints) receives the exclusive end of every bin, dropped bins included; returns bin_ends[drop_from_bin - 1], the
 * number of rays kept.  Neither stream's `size` is read or set.  Synchronises the stream.  Invalid arguments abort (as do streams whose
 * `pad` asks for 20-byte hit records).
 * PRECONDITION, not checked: every key of the first n rays lies in [0, num_bins) and *size_dev <= max_n <= the streams' capacity -- the
 * kernels index LDS and the per-block counts with the key. */
int32_t hip_bin_primary(int32_t dev, struct PrimaryStream* from, struct PrimaryStream* to, int32_t mode, int32_t num_bins,
                        int32_t drop_from_bin, int32_t keep_hit, int32_t copy_interval, int32_t* perm, const int32_t* size_dev,
                        int32_t max_n, int32_t* bin_ends, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RODENT_RENDER_H */
