/*
 * rodent_motion.h -- C ABI of deforming meshes under motion (librodent_hip.so): a BVH2 / Tri1 hierarchy with TWO keys per record, the
 * mesh at time 0 and at time 1, and a time per ray.  No reference counterpart; tests/motion_bvh_model.py restates everything below on
 * the CPU and predicts the bytes.  This is the traversal ABI; the renderer over these records is rodent_render.h's "deforming meshes
 * in the renderer".  Motion objects under the motion TLAS: rodent_instances.h, "deforming objects under moving instances".
 *
 * Records: RodentMotionNode2 is a Node2 (rodent_traversal.h) with its 12 bounds twice -- bounds order, child encoding and leaf encoding
 *   unchanged --, RodentMotionTri1 a Tri1 twice; key 0 carries the pad / geom_id / prim_id words (bit 31 of prim_id = last in leaf), the
 *   three w words of key 1 are 0.  A record is read with aligned 16-byte loads: a node takes seven (three per key and the child words),
 *   a triangle six.
 *
 * All arithmetic is fp32, every operation rounded on its own, no fused multiply-add (except inside the unchanged slab and triangle
 * tests, which are those of rodent_traversal.h).
 *
 * Time: every ray carries a float t.  A ray with !(0 <= t && t <= 1) -- a NaN fails the test -- stores the miss record
 *   {-1, tmax as given, 0, 0} without traversal.  This is deliberately stricter than the "used as given" of moving instances
 *   (rodent_instances.h): outside [0, 1] an interpolated bound can be NaN or infinite, and the precondition of the kernels and of the
 *   oracle is "no NaN bound".  -0 and 1 are traced.
 * Value at time t: for every bound and every one of the nine Tri1 floats  s = 1 - t;  x = s*x0 + t*x1  (a subtraction once per ray, two
 *   products and a sum per value).  t = 0 gives x0 and t = 1 gives x1 bit for bit, except for a -0 beside a positive or +0 partner (at
 *   t = -0: beside a negative or -0 partner), which comes out as +0.
 * Triangle at time t: the Tri1 {v0(t), e1(t), e2(t)} with key 0's w words goes unchanged into the triangle test with
 *   n = cross(e1(t), e2(t)), as a static Tri1 does.  e1 and e2 are linear in the corners, so in exact arithmetic the interpolated edges
 *   are the edges of the interpolated triangle.
 * Node at time t: the 12 interpolated bounds go into the unchanged slab test, ordering (te0 < te1, strict) and push.  A slot with
 *   child == 0 is never taken, whatever its bounds; the fuse stores such a slot's bounds as they are, (+inf, -inf), without widening.
 * Stored bounds are widened when the records are made (the kernel adds nothing per ray).  For slot k, axis a, with lo0 hi0 lo1 hi1 from
 *   the two same-topology hierarchies:  M = fmaxf(fmaxf(|lo0|, |hi0|), fmaxf(|lo1|, |hi1|));  e = 2^-19 * M;  both keys store lo_k - e
 *   and hi_k + e.  Why: the corners the kernel intersects are v0(t), v0(t) - e1(t) and v0(t) + e2(t).  Against the exact interpolation of
 *   the two keys' corners they err by the rounding of e1_k = v0_k - v1_k (at most 2^-24 * 2M), by three roundings per interpolated value
 *   (at most 3 * 2^-24 of the operand magnitude, at most 2M for an edge), and by the interpolation of the bound itself; together under
 *   14 * 2^-24 * M < 2^-20 * M, and the factor 2 covers computing e and the subtraction in fp32.  A parent's interpolated box contains
 *   its children's by the same bound.  Domain: no non-zero intermediate below 2^-126 in magnitude and no magnitude above 2^126 -- the
 *   bound is relative and has no room for a denormal's absolute error, as for the instance boxes of rodent_instances.h.
 *   tests/test_motion_bvh_model.py checks containment in exact rational arithmetic (and that no widening at all fails).
 * Stack: the reference's 64 entries, the word that ends the traversal and up to 63 pushed.  A ray whose peak at its own time is at most
 *   63 is traced without a flag; any other ray raises the overflow flag (rodent_hip_check_errors; the synchronous entries abort() on
 *   it), stops where it stands and stores an undefined hit: it never pops a slot it did not push.
 */
#ifndef RODENT_MOTION_H
#define RODENT_MOTION_H

#include <stdint.h>
#include "rodent_build.h"

#ifdef __cplusplus
extern "C" {
#endif

struct RodentMotionNode2 { float bounds0[12]; float bounds1[12]; int32_t child[2]; int32_t pad[6]; };   /* 128 B, one cache line */
struct RodentMotionTri1  { struct Tri1 key0; struct Tri1 key1; };                                       /* 96 B */

/* Fuses two BVH2 / Tri1 hierarchies of ONE topology (the same child words and Tri1 w words) into motion records with the widening
 * above.  DEVICE pointers: nodes0 / nodes1 (num_nodes Node2), tris0 / tris1 (num_bvh_tris Tri1), motion_nodes (num_nodes
 * RodentMotionNode2), motion_tris (num_bvh_tris RodentMotionTri1), info_dev (RODENT_BUILD_INFO_WORDS ints, zeroed at the start of the
 * call).  One elementwise launch, no scratch; asynchronous on `stream`.  Both inputs must carry WHOLE-TRIANGLE boxes: the clipped boxes
 * of a pre-split tree hold for one key only, not between the keys, so refit such a tree first (rodent_hip_refit_bvh2_tri1).
 * info: [0] 0 [1] records fused (num_nodes + num_bvh_tris) [2] flags [3] 0.  RODENT_BUILD_BAD_TOPOLOGY: the two keys' child words or
 * Tri1 w words differ somewhere; such a record takes key 0's words.  Nothing is read or written out of bounds.
 * Checks, in this order, each enqueuing nothing when it fails: RODENT_BUILD_ERR_NUM_NODES (num_nodes < 1 or num_bvh_tris < 1),
 * RODENT_BUILD_ERR_NULL, RODENT_BUILD_ERR_DEVICE. */
int32_t rodent_hip_fuse_motion_bvh2_tri1(int32_t dev, const struct Node2* nodes0, const struct Tri1* tris0, const struct Node2* nodes1,
                                         const struct Tri1* tris1, int32_t num_nodes, int32_t num_bvh_tris,
                                         struct RodentMotionNode2* motion_nodes, struct RodentMotionTri1* motion_tris, int32_t* info_dev,
                                         void* stream);

/* Bytes of device scratch rodent_hip_build_motion_bvh2_tri1 needs (-1 for num_nodes < 1 or num_bvh_tris < 1); any 256-byte aligned
 * buffer of that size, its contents are ignored. */
int64_t rodent_hip_motion_bvh2_scratch_bytes(int32_t num_nodes, int32_t num_bvh_tris);

/* Builds the motion records of the hierarchy nodes / tris (any BVH2 / Tri1 this library or a host builder wrote; read only) over
 * vertices0 at time 0 and vertices1 at time 1 (num_vertices float4 rows each; indices: num_tris int4 rows, the table the prim ids refer
 * to).  All pointers are DEVICE pointers.  Asynchronous on `stream`: nothing is allocated, nothing waits.  The launch list is fixed:
 * two device-to-device copies of the topology into scratch, the refit of rodent_hip_refit_bvh2_tri1 on copy A with vertices0, the same
 * on copy B with vertices1, the fuse.  The output is a pure function of (topology, vertices0, vertices1, indices), byte for byte.
 * Calling it again with moved keys IS the refit of a motion hierarchy: there is no other path.
 * info: [0] nodes completed at key 0 [1] records fused [2] the OR of both refits' flags and the fuse's [3] nodes completed at key 1.
 * A sound call leaves info[0] == info[3] == num_nodes.
 * Checks: those of rodent_hip_refit_bvh2_tri1, in its order (RODENT_BUILD_ERR_NUM_TRIS, RODENT_BUILD_ERR_NUM_VERTICES,
 * RODENT_BUILD_ERR_NUM_NODES, RODENT_BUILD_ERR_NULL, RODENT_BUILD_ERR_DEVICE), each enqueuing nothing when it fails. */
int32_t rodent_hip_build_motion_bvh2_tri1(int32_t dev, const float* vertices0, const float* vertices1, int32_t num_vertices,
                                          const int32_t* indices, int32_t num_tris, const struct Node2* nodes, int32_t num_nodes,
                                          const struct Tri1* tris, int32_t num_bvh_tris, struct RodentMotionNode2* motion_nodes,
                                          struct RodentMotionTri1* motion_tris, void* scratch, int32_t* info_dev, void* stream);

/* Synchronous form on the null stream with its own scratch: copies the info words to `info` (host, may be NULL) and returns
 * RODENT_BUILD_ERR_INPUT when the device raised a flag or a node count differs from num_nodes. */
int32_t rodent_hip_build_motion_bvh2_tri1_sync(int32_t dev, const float* vertices0, const float* vertices1, int32_t num_vertices,
                                               const int32_t* indices, int32_t num_tris, const struct Node2* nodes, int32_t num_nodes,
                                               const struct Tri1* tris, int32_t num_bvh_tris, struct RodentMotionNode2* motion_nodes,
                                               struct RodentMotionTri1* motion_tris, int32_t* info);

/* Traces num_rays rays through the motion records; `times` (DEVICE, one float per ray, required) holds every ray's time.  Enqueued on
 * `stream` without synchronising, like hip_traverse_bvh2_tri1_async; a stack overflow is reported by rodent_hip_check_errors(dev,
 * stream). */
void hip_traverse_motion_bvh2_tri1_async(int32_t dev, const struct RodentMotionNode2* motion_nodes,
                                         const struct RodentMotionTri1* motion_tris, const struct Ray1* rays, const float* times,
                                         struct Hit1* hits, int32_t num_rays, int32_t any_hit, void* stream);

/* Synchronous forms on the null stream: closest hit / any hit.  They abort() on the overflow flag, as the synchronous entries of
 * rodent_traversal.h do. */
void hip_intersect_motion_bvh2_tri1(int32_t dev, const struct RodentMotionNode2* motion_nodes, const struct RodentMotionTri1* motion_tris,
                                    const struct Ray1* rays, const float* times, struct Hit1* hits, int32_t num_rays);
void hip_occluded_motion_bvh2_tri1(int32_t dev, const struct RodentMotionNode2* motion_nodes, const struct RodentMotionTri1* motion_tris,
                                   const struct Ray1* rays, const float* times, struct Hit1* hits, int32_t num_rays);

#ifdef __cplusplus
}
#endif
#endif /* RODENT_MOTION_H */
