/*
 * rodent_instances.h -- C ABI of instanced scenes (librodent_hip.so): a two-level hierarchy built and traced on the device.
 *
 * Objects keep their own BVH2 / Tri1 hierarchies (rodent_traversal.h; of any builder of rodent_build.h or of a host builder).  An
 * INSTANCE places one object in the world by a 3 x 4 matrix; a small top-level hierarchy (TLAS) over the instances is rebuilt on the
 * device whenever the matrices change (rodent_hip_build_tlas: the LBVH stages of rodent_build.h over instance boxes), and
 * hip_traverse_instanced_bvh2_tri1_async carries every ray into object space and back.  No reference counterpart; tests/instance_model.py
 * restates everything below on the CPU and predicts the bytes.
 *
 * Objects: all objects' Node2 records lie in ONE array and all their Tri1 records in another.  Child ids and leaf indices inside an
 *   object stay relative to the object's own first node and first triangle, so packing is concatenation: no id is rewritten.
 * Matrices: 3 x 4, row-major: row a is m[4a .. 4a + 3], the last column the translation.  instance_id is the caller's, in [0, 2^31).
 * TLAS: a plain Node2 array with the encoding of rodent_traversal.h; a leaf ~first points into the RodentInstance array, which is stored
 *   in leaf order; bit 31 of instance_id marks the last instance of a leaf, as bit 31 of prim_id does for Tri1.
 *
 * All arithmetic is fp32 with every operation rounded on its own (no fused multiply-add), except where marked fp64.
 *
 * Inverse (fp64, every operation rounded on its own, in this order; a b c tx / d e f ty / g h i tz = the rows of object_to_world):
 *   c0 = e*i - f*h   c1 = f*g - d*i   c2 = d*h - e*g      det = (a*c0 + b*c1) + c*c2      r = 1 / det
 *   row 0: c0*r   (c*h - b*i)*r   (b*f - c*e)*r
 *   row 1: c1*r   (a*i - c*g)*r   (c*d - a*f)*r
 *   row 2: c2*r   (b*g - a*h)*r   (a*e - b*d)*r
 *   translation of row k (q0 q1 q2): -((q0*tx + q1*ty) + q2*tz).  Each of the 12 entries is then rounded to fp32 once.
 *   RODENT_TLAS_BAD_TRANSFORM: an entry of object_to_world is non-finite, det is 0 or non-finite, or an entry of the rounded inverse is
 *   non-finite.
 * World box of an instance: the object's box is the union of its root node's two child boxes (fminf of the lows, fmaxf of the highs: an
 *   empty slot's (+inf, -inf) drops out).  Its 8 corners (x, y, z) are mapped per row by ((m0*x + m1*y) + m2*z) + m3; the box takes
 *   fminf / fmaxf over the corners, as v + 0 (one bit pattern for a zero).  Each bound is then moved outward by
 *   e = 2^-21 * (((|m0|*X + |m1|*Y) + |m2|*Z) + |m3|), X = fmaxf(|lo_x|, |hi_x|) and so on: lo - e, hi + e.  The rounding error of the
 *   four-term sum is at most gamma_4 ~ 2^-22 times the sum of magnitudes and the factor 2 covers computing e itself in fp32, so the
 *   widened box contains the exact image of the object box -- on this domain: no product m_k * c and no partial sum of the four-term
 *   row sum is a non-zero value below 2^-126 in magnitude (none is rounded as a denormal), and nothing overflows.  The bound is a
 *   relative one and has no room for the absolute rounding error of a denormal (up to 2^-150 per operation): outside the domain the
 *   box may miss a corner by that much.  (Observed in exact arithmetic on random matrices and boxes: with entries and coordinates
 *   around 1e-22 and no translation nearly every box misses a corner; at scales from 1e-18 to 1e15 no failure was found, which is
 *   an observation, not membership of the domain -- a coordinate near 0 can underflow a product at any scale.
 *   tests/test_instance_edge_fixtures.py pins one case on each side.)
 * TLAS build: the sort point of an instance is lo + hi of its world box per axis; from there the LBVH stages of rodent_build.h as they
 *   stand: frame, 30-bit Morton codes, stable radix sort (code, then instance index), Karras, renumbering, bottom-up boxes, emission;
 *   the single-leaf root for num_instances <= max_leaf.  RodentInstance k is the k-th instance in that order: world_to_object, the
 *   object's node_offset and tri_offset, instance_id (bit 31: the last of its leaf), pad = 0.  The output is a pure function of
 *   (the objects' root nodes, the object table, the descriptors, max_leaf), byte for byte.  info: [0] Node2 count [1] depth [2] flags
 *   [3] 0.  An object index outside [0, num_objects) raises RODENT_TLAS_BAD_OBJECT (object 0 is read instead).  With a flag raised the
 *   output is undefined, but nothing is read or written out of bounds.
 * Traversal: the TLAS is walked by the step of mapping_gpu.impala:94-178 on the world ray, pushes, pops and leaves unchanged; the
 *   instances of a leaf are taken in stored order until the marked one.  Entering an instance (rows w of world_to_object):
 *     org' = ((w0*ox + w1*oy) + w2*oz) + w3,  dir' = (w0*dx + w1*dy) + w2*dz,  tmin unchanged, tmax = the ray's current tmax;
 *   directions are never normalised, so t parametrises both spaces; inv_dir and inv_org come from the new ray by the make_ray rule
 *   (intersection.impala:88-99).  The object is traversed from its root with the unchanged BVH2 / Tri1 rules; an accepted triangle sets
 *   hit = {prim_id & 0x7FFFFFFF, t, u, v}, hit_instance = instance_id and the shared tmax = t.  The acceptance test stays <= across
 *   instances: a later hit at an equal t replaces an earlier one.  Any-hit returns at the first acceptance.  A miss stores
 *   {-1, tmax of the ray as given, 0, 0} and instance -1.
 * Stack: one stack of the reference's 64 entries (stack.impala:53-54) serves both levels.  Its slots, bottom up: the word that ends the
 *   traversal, the TLAS entries (the visited leaf's continuation stays among them while its instances are traced), the word that ends
 *   the object's traversal, the object's entries.  With P = the TLAS entries held when an instance is entered + that object's peak
 *   entries for the ray, a ray whose P + 2 never exceeds 64 is traced without a flag; any other ray raises the overflow flag
 *   (rodent_hip_check_errors; the synchronous entries abort() on it), stops where it stands and stores an undefined hit: it never reads
 *   an entry that was not pushed.  A wrong hit without a flag does not occur.
 *
 * ---- moving instances: a time per ray over two-key instance motion (tests/motion_instance_model.py restates this section) ----
 * Motion instance: one object placed by TWO object_to_world matrices, M0 at time 0 and M1 at time 1.
 * Placement at time t: every ray carries a time t (a float, used as given: it is not clamped).  Entry by entry s = 1 - t; m = s*m0 + t*m1:
 *   two products and one sum, each rounded, no fused multiply-add.  So t = 0 gives M0 and t = 1 gives M1, bit for bit -- with one
 *   exception the three operations cannot avoid: an entry -0 whose partner is positive or +0 comes out as 1 * -0 + 0 * m1 = +0 (at
 *   t = -0, where t * m1 is a zero of the opposite sign: an entry -0 whose partner is negative or -0).  The value is the same, and
 *   the inverse differs at most in the sign of a zero of its own.
 * Per-ray inverse: the fp64 cofactor inverse above of the interpolated fp32 matrix, in the order above, each of the 12 entries rounded to
 *   fp32 once -- one function (csrc/instance_inverse.h) for the build stage and for the kernel.  At t = 0 it is bit-equal to what
 *   rodent_hip_build_tlas stores for M0 (but for the zeros just named).
 * Skipped instances: an instance is skipped for a ray iff det is 0 or non-finite or one of the 12 rounded entries is non-finite (a
 *   non-finite entry of the interpolated matrix always makes one of the two so).  It is skipped with no flag: its object is not entered,
 *   tmax and the hit stay as they are.  An interpolation between two sound placements can pass through a singular matrix (a half turn at
 *   t = 0.5): that is the scene's property, not an error.  A NaN time makes every entry NaN, so every instance is skipped for that ray.
 * Object ray: formed from the per-ray inverse exactly as from a stored world_to_object above; everything inside the object is unchanged,
 *   and so are the TLAS walk, the <= rule across instances, the miss record and the stack contract (P + 2 <= 64; a skipped instance
 *   pushes nothing).
 * Motion box of an instance: B0 and B1 are the widened world boxes above under M0 and M1, e0 and e1 their per-axis widenings.  Per axis
 *   lo = fminf(lo0, lo1) - (e0 + e1), hi = fmaxf(hi0, hi1) + (e0 + e1).  Under exact interpolation a corner's image is linear in t, so for
 *   t in [0, 1] it lies in the hull of the two endpoint images, which B0 and B1 contain; the fp32 interpolation moves an entry by at most
 *   about 3 * 2^-24 * max(|m0|, |m1|), which moves a corner's image by less than e0 + e1.  Containment is promised for t in [0, 1] only,
 *   on the domain of the static rule for both matrices.  tests/test_motion_instance_model.py checks it in exact rational arithmetic
 *   (seeded pairs, the edge matrices paired with each other, a half turn; t in {0, 1, 0.5, 2^-24, 1 - 2^-24, a denormal, 33 seeded}):
 *   no counterexample was found, so the widening stands as derived.
 * Sort point: lo + hi of the motion box; from there the LBVH stages as for rodent_hip_build_tlas.  RodentMotionInstance k is the k-th
 *   instance in that order: both matrices as given, the object's offsets, instance_id (bit 31: the last of its leaf), pads = 0.
 * Flags: RODENT_TLAS_BAD_TRANSFORM if either endpoint matrix fails the static checks; RODENT_TLAS_BAD_OBJECT as above.
 *
 * ---- deforming objects under moving instances: one time through both levels (tests/motion_objects_model.py restates this section) ----
 * Motion object set: all objects' RodentMotionNode2 records (rodent_motion.h) lie in ONE array and all their RodentMotionTri1 records in
 *   another; the RodentObject table indexes those arrays (node_offset / tri_offset count motion records); child ids and leaf starts stay
 *   object-local, as in a static set.  An object that does not deform has equal keys.
 * Time: one float per ray serves both levels, and rodent_motion.h's rule wins over "used as given" above: a ray with
 *   !(0 <= t && t <= 1) stores the miss record {-1, tmax as given, 0, 0} and instance -1 without any traversal.  A NaN fails the test; -0
 *   and 1 are traced.  Inside [0, 1] everything of "moving instances" holds unchanged: the entry-wise lerp of the placement, the fp64
 *   cofactor inverse, the silent skip of an instance that is singular or non-finite at that time.
 * Inside an object: rodent_motion.h unchanged, with the same s = 1 - t and t: the interpolated node goes into the unchanged slab test,
 *   ordering and push, the interpolated Tri1 into the unchanged triangle test; a slot with child == 0 is never taken.
 * Across instances: as for static objects: the <= acceptance rule, the shared tmax carried between instances, any-hit returning at the
 *   first acceptance, hit = {prim_id & 0x7FFFFFFF, t, u, v}, hit_instance = instance_id.
 * Stack: one stack of 64 entries serves both levels, in the slot order above.  P = the TLAS entries held on entering an instance + that
 *   object's peak entries at the ray's own time (the interpolated boxes decide what is pushed): a ray whose P + 2 never exceeds 64 is
 *   traced without a flag; any other ray raises the overflow word, stops where it stands and never pops a slot it did not push.
 * Object box of a motion object: fminf of the lows and fmaxf of the highs over the root record's FOUR stored child boxes, two slots at
 *   both keys; an empty slot's (+inf, -inf) drops out.  This is the union U over both keys, on purpose.  Mapping key 0's box by M0 and key
 *   1's box by M1 would NOT bound the motion: a corner's world image is M(t) p(t), with both factors linear in t, so it is quadratic in t
 *   and does not lie in the hull of its two endpoint images.  U contains every corner the kernel intersects at every t in [0, 1]: an
 *   exact interpolation of a vertex lies between its keys, inside the unwidened boxes of both keys' hierarchies, and the stored bounds
 *   were widened by 2^-19 M at fuse time (rodent_motion.h), which covers the three roundings of a corner's fp32 interpolation (and those
 *   of v0 - e1 and v0 + e2).  The motion box of U under (M0, M1) by the rule above then contains the image of all of U under the
 *   fp32-interpolated placement at every t in [0, 1], hence every such corner.  tests/test_motion_objects_model.py checks this in exact
 *   rational arithmetic, and shows that key 0's root box alone fails it.
 * Sort point, LBVH stages, leaf order and the RodentMotionInstance records: those of "moving instances", byte for byte.  The pad word of
 *   an instance record stays 0: static and motion objects are not mixed under one TLAS.
 */
#ifndef RODENT_INSTANCES_H
#define RODENT_INSTANCES_H

#include <stdint.h>
#include "rodent_build.h"

#ifdef __cplusplus
extern "C" {
#endif

struct RodentObject       { int32_t node_offset, tri_offset, num_nodes, num_tris; };              /* 16 B */
struct RodentInstanceDesc { float object_to_world[12]; int32_t object, instance_id, pad[2]; };    /* 64 B, the caller's input */
struct RodentInstance     { float world_to_object[12]; int32_t node_offset, tri_offset,
                            instance_id /* bit 31 = last in leaf */, pad; };                      /* 64 B, what the kernel reads */
struct RodentMotionInstanceDesc { float object_to_world0[12]; float object_to_world1[12];
                                  int32_t object, instance_id, pad[6]; };                         /* 128 B, the caller's input */
struct RodentMotionInstance     { float object_to_world0[12]; float object_to_world1[12]; int32_t node_offset, tri_offset,
                                  instance_id /* bit 31 = last in leaf */, pad; int32_t pad2[4]; }; /* 128 B, one cache line */

#define RODENT_TLAS_MAX_INSTANCES        (1 << 22)

/* error flags in info[2], beside the builders' (rodent_build.h) */
#define RODENT_TLAS_BAD_OBJECT           8     /* an object index outside [0, num_objects) */
#define RODENT_TLAS_BAD_TRANSFORM        16    /* a non-finite entry, a determinant that is 0 or non-finite, a non-finite inverse */

/* return values beside the builders' (RODENT_BUILD_OK, _ERR_MAX_LEAF, _ERR_NULL, _ERR_DEVICE, _ERR_LAUNCH, _ERR_INPUT) */
#define RODENT_TLAS_ERR_NUM_INSTANCES   -14    /* num_instances outside [1, 2^22] */
#define RODENT_TLAS_ERR_NUM_OBJECTS     -15    /* num_objects < 1 */

/* Bytes of device scratch rodent_hip_build_tlas needs (-1 for num_instances outside [1, 2^22]); any 256-byte aligned buffer of that
 * size, its contents are ignored. */
int64_t rodent_hip_tlas_scratch_bytes(int32_t num_instances);

/* Builds the TLAS of num_instances instances.  All pointers are DEVICE pointers: nodes (the objects' Node2 array: only the root node of
 * every object is read), objects (num_objects RodentObject), descs (num_instances RodentInstanceDesc), tlas_nodes (room for
 * max(1, num_instances - 1) Node2), instances (num_instances RodentInstance), scratch (rodent_hip_tlas_scratch_bytes), info_dev
 * (RODENT_BUILD_INFO_WORDS ints, zeroed at the start of the call).  Asynchronous on `stream` like the builders of rodent_build.h: nothing
 * is allocated, nothing waits for the device.  Checks, in this order, each enqueuing nothing when it fails:
 * RODENT_TLAS_ERR_NUM_INSTANCES, RODENT_BUILD_ERR_MAX_LEAF (max_leaf outside [1, 8]), RODENT_TLAS_ERR_NUM_OBJECTS, RODENT_BUILD_ERR_NULL,
 * RODENT_BUILD_ERR_DEVICE. */
int32_t rodent_hip_build_tlas(int32_t dev, const struct Node2* nodes, const struct RodentObject* objects, int32_t num_objects,
                              const struct RodentInstanceDesc* descs, int32_t num_instances, int32_t max_leaf, struct Node2* tlas_nodes,
                              struct RodentInstance* instances, void* scratch, int32_t* info_dev, void* stream);

/* Synchronous form on the null stream with its own scratch: copies the info words to `info` (host, may be NULL) and returns
 * RODENT_BUILD_ERR_INPUT when the device raised a flag. */
int32_t rodent_hip_build_tlas_sync(int32_t dev, const struct Node2* nodes, const struct RodentObject* objects, int32_t num_objects,
                                   const struct RodentInstanceDesc* descs, int32_t num_instances, int32_t max_leaf,
                                   struct Node2* tlas_nodes, struct RodentInstance* instances, int32_t* info);

/* The three above for moving instances (the section "moving instances" at the top): the same argument shape with
 * RodentMotionInstanceDesc in and RodentMotionInstance out, the same host-side refusals in the same order, the same asynchronous
 * contract (nothing is allocated, nothing waits for the device, the info words are zeroed at the start), the same launch list with the
 * motion instance stage in the place of the instance stage. */
int64_t rodent_hip_motion_tlas_scratch_bytes(int32_t num_instances);
int32_t rodent_hip_build_motion_tlas(int32_t dev, const struct Node2* nodes, const struct RodentObject* objects, int32_t num_objects,
                                     const struct RodentMotionInstanceDesc* descs, int32_t num_instances, int32_t max_leaf,
                                     struct Node2* tlas_nodes, struct RodentMotionInstance* instances, void* scratch, int32_t* info_dev,
                                     void* stream);
int32_t rodent_hip_build_motion_tlas_sync(int32_t dev, const struct Node2* nodes, const struct RodentObject* objects, int32_t num_objects,
                                          const struct RodentMotionInstanceDesc* descs, int32_t num_instances, int32_t max_leaf,
                                          struct Node2* tlas_nodes, struct RodentMotionInstance* instances, int32_t* info);

/* ---- refit of deforming objects: a chosen subset of the packed objects, in place, in one launch list ----
 * One RodentRefitRange per listed object: `object` indexes the RodentObject table; first_tri / num_tris cut the object's rows out of
 * the concatenated index table (the prim ids of the object's Tri1 records index these rows); node_start / rec_start are the exclusive
 * prefix sums of the listed objects' num_nodes / num_tris (Tri1 records) in list order. */
struct RodentRefitRange   { int32_t object, first_tri, num_tris, node_start, rec_start, pad[3]; }; /* 32 B */

/* Fills ranges[0 .. num_listed) on the HOST from host arrays: the object table, the listed object ids (any order) and, per listed
 * object, its first row and row count in the index table.  A listed id outside the table gets node and record counts of 0 (the device
 * raises RODENT_TLAS_BAD_OBJECT for it).  totals[0] / totals[1]: the listed objects' nodes / Tri1 records.  Returns the bytes of device
 * scratch rodent_hip_refit_objects needs for these totals (any 256-byte aligned buffer, its contents are ignored), or -1 for a NULL
 * pointer, num_objects < 1, num_listed < 1 or totals beyond 2^31 - 1. */
int64_t rodent_hip_refit_objects_plan(const struct RodentObject* objects, int32_t num_objects, const int32_t* listed,
                                      const int32_t* first_tri, const int32_t* num_tris, int32_t num_listed,
                                      struct RodentRefitRange* ranges, int32_t* totals);

/* Refits the listed objects in place to moved vertices.  All pointers are DEVICE pointers: vertices (num_vertices float4 rows, the
 * concatenated table), indices (num_rows int4 rows, the concatenated table), nodes / tris (the packed arrays the object table points
 * into), objects (num_objects RodentObject), ranges (num_listed RodentRefitRange), scratch (rodent_hip_refit_objects_plan's bytes for
 * total_nodes / total_recs), info_dev (RODENT_BUILD_INFO_WORDS ints, zeroed at the start of the call).  Asynchronous on `stream` like
 * rodent_hip_refit_bvh2_tri1: nothing is allocated, nothing waits for the device; two memsets and three kernels whatever num_listed.
 *
 * For every listed object o the bytes of nodes[node_offset .. + num_nodes) and tris[tri_offset .. + num_tris) are those
 * rodent_hip_refit_bvh2_tri1 writes for that object alone over indices + 4 * first_tri, num_tris rows (the refit rules of
 * rodent_build.h); child ids, leaf starts and prim ids stay object-local; every record of an unlisted object keeps its bytes; the
 * result does not depend on the list's order.  info: [0] nodes completed over all listed objects [1] records rewritten [2] flags [3] 0.
 * A sound call leaves info[0] = total_nodes.
 *
 * Flags: a listed object id outside the table raises RODENT_TLAS_BAD_OBJECT and nothing of that range is touched.  Within an object,
 * what rodent_hip_refit_bvh2_tri1 flags is flagged (RODENT_BUILD_BAD_TOPOLOGY: a child id beyond the object's nodes, the object's root
 * as a child, a leaf start or walk beyond its records, a prim id beyond its rows, a node named twice; RODENT_BUILD_BAD_INDEX,
 * RODENT_BUILD_NON_FINITE) and leaves that object incomplete; the other listed objects come out complete.  A range whose rows leave
 * the index table or whose stretch [node_start, + num_nodes) / [rec_start, + num_tris) leaves the totals raises
 * RODENT_BUILD_BAD_TOPOLOGY and has nothing touched; other faults of the range table (wrong prefix sums, an object listed twice) leave
 * nodes incomplete or bytes undefined inside the listed objects, and nothing is read or written beyond the totals or the objects.
 *
 * Checks, in this order, each enqueuing nothing when it fails: RODENT_BUILD_ERR_NUM_TRIS (num_rows outside [1, 2^25]),
 * RODENT_BUILD_ERR_NUM_VERTICES, RODENT_TLAS_ERR_NUM_OBJECTS, RODENT_BUILD_ERR_NUM_NODES (num_listed < 1, a negative total),
 * RODENT_BUILD_ERR_NULL, RODENT_BUILD_ERR_DEVICE. */
int32_t rodent_hip_refit_objects(int32_t dev, const float* vertices, int32_t num_vertices, const int32_t* indices, int32_t num_rows,
                                 struct Node2* nodes, struct Tri1* tris, const struct RodentObject* objects, int32_t num_objects,
                                 const struct RodentRefitRange* ranges, int32_t num_listed, int32_t total_nodes, int32_t total_recs,
                                 void* scratch, int32_t* info_dev, void* stream);

/* ---- build of the objects' hierarchies: all objects of a new set, or a chosen subset of a packed one, in one launch list ----
 * The forest form of rodent_hip_build_bvh2_tri1 (rodent_build.h): for every listed object the Node2 / Tri1 records are, byte for byte,
 * those rodent_hip_build_bvh2_tri1 writes for that object alone over indices + 4 * first_tri, num_tris rows and max_leaf -- the object's
 * own frame, the order (code, row), Karras' ties by the object's own sorted positions, child ids, leaf starts and prim ids object-local.
 * One RodentRefitRange per listed object, with node_start == rec_start == the exclusive prefix sum of the listed objects' num_tris in list
 * order (rodent_hip_build_objects_plan writes them).  No treelet passes, no pre-splitting, no PLOC.
 *
 * mode RODENT_BUILD_OBJECTS_PACK: the device writes the whole RodentObject of every listed object: node_offset = the sum of num_nodes of
 *   the objects listed before it, tri_offset = rec_start, num_nodes, num_tris.  `nodes` needs room for the sum of max(1, num_tris - 1),
 *   `tris` for total_tris.  With the list 0 .. K - 1 the table and the records are a tight packed set (instances.pack_objects).
 * mode RODENT_BUILD_OBJECTS_IN_PLACE: the device reads node_offset, tri_offset and num_tris of each listed object from the table and
 *   writes only num_nodes; the caller guarantees a node slot of max(1, num_tris - 1) records at node_offset.  Bytes of a slot beyond
 *   num_nodes and every record of an unlisted object keep their contents; the result does not depend on the list's order.
 * object_info[4 j ..] = {Node2 count, depth, flags, 0} of listed object j; info_dev = {total nodes, largest depth, OR of the flags, 0}.
 *
 * Flags: a range with an object id outside the table raises RODENT_TLAS_BAD_OBJECT; a range whose rows leave the index table, whose
 * stretch [rec_start, + num_tris) leaves total_tris, whose node_start differs from its rec_start or (in place) whose num_tris differs
 * from the table's (or whose table offsets are negative) raises RODENT_BUILD_BAD_TOPOLOGY; nothing of a refused range is touched, its
 * node count is 0.  RODENT_BUILD_BAD_INDEX / RODENT_BUILD_NON_FINITE inside one object land in that object's info words (and in
 * info_dev[2]); the other objects come out complete and correct.  Other faults of the range table (wrong prefix sums, an object listed
 * twice) leave bytes undefined inside the listed objects and may raise RODENT_BUILD_BAD_TOPOLOGY; nothing is read or written beyond the
 * totals, the node room or the objects. */
#define RODENT_BUILD_OBJECTS_IN_PLACE    0
#define RODENT_BUILD_OBJECTS_PACK        1
#define RODENT_BUILD_OBJECTS_MAX_LISTED  (1 << 20)

/* Fills ranges[0 .. num_listed) on the HOST from host arrays: the listed object ids (any order) and, per listed object, its first row and
 * row count in the index table.  totals[0]: the listed triangles.  Returns the bytes of device scratch rodent_hip_build_objects needs (any
 * 256-byte aligned buffer, its contents are ignored), or -1 for a NULL pointer, num_listed outside [1, 2^20], a row count < 1 or more than
 * 2^25 listed triangles. */
int64_t rodent_hip_build_objects_plan(const int32_t* listed, const int32_t* first_tri, const int32_t* num_tris, int32_t num_listed,
                                      struct RodentRefitRange* ranges, int32_t* totals);

/* All pointers are DEVICE pointers: vertices (num_vertices float4 rows), indices (num_rows int4 rows; the concatenated tables),
 * nodes / tris (the packed arrays), objects (num_objects RodentObject), ranges (num_listed RodentRefitRange), scratch (the plan's bytes), object_info
 * (4 ints per listed object), info_dev (RODENT_BUILD_INFO_WORDS ints); both info arrays are written by the call.  Asynchronous on `stream`
 * like every builder: nothing is allocated, nothing waits for the device, and the launch list depends on num_listed only through the
 * ceil(log2(num_listed) / 8) extra sort passes.  Checks, in this order, each enqueuing nothing when it fails: RODENT_BUILD_ERR_NUM_TRIS
 * (num_rows outside [1, 2^25]), RODENT_BUILD_ERR_NUM_VERTICES, RODENT_TLAS_ERR_NUM_OBJECTS, RODENT_BUILD_ERR_NUM_NODES (num_listed outside
 * [1, 2^20], total_tris outside [1, 2^25]), RODENT_BUILD_ERR_MAX_LEAF, RODENT_BUILD_ERR_INPUT (an unknown mode), RODENT_BUILD_ERR_NULL,
 * RODENT_BUILD_ERR_DEVICE. */
int32_t rodent_hip_build_objects(int32_t dev, const float* vertices, int32_t num_vertices, const int32_t* indices, int32_t num_rows,
                                 int32_t max_leaf, int32_t mode, struct Node2* nodes, struct Tri1* tris, struct RodentObject* objects,
                                 int32_t num_objects, const struct RodentRefitRange* ranges, int32_t num_listed, int32_t total_tris,
                                 void* scratch, int32_t* object_info, int32_t* info_dev, void* stream);

/* Synchronous form on the null stream with its own scratch: copies both info arrays to the host (object_info: 4 ints per listed object,
 * info: RODENT_BUILD_INFO_WORDS ints; either may be NULL) and returns RODENT_BUILD_ERR_INPUT when the device raised a flag.  It checks
 * RODENT_BUILD_ERR_NUM_NODES and RODENT_BUILD_ERR_DEVICE first (it sizes and allocates the scratch), then as above. */
int32_t rodent_hip_build_objects_sync(int32_t dev, const float* vertices, int32_t num_vertices, const int32_t* indices, int32_t num_rows,
                                      int32_t max_leaf, int32_t mode, struct Node2* nodes, struct Tri1* tris,
                                      struct RodentObject* objects, int32_t num_objects, const struct RodentRefitRange* ranges,
                                      int32_t num_listed, int32_t total_tris, int32_t* object_info, int32_t* info);

/* Traces num_rays rays through the TLAS and the objects below it. DEVICE pointers; hit_instances (one int32_t per ray) may be NULL.
 * Enqueued on `stream` without synchronising, like hip_traverse_bvh2_tri1_async; a stack overflow is reported by
 * rodent_hip_check_errors(dev, stream). */
void hip_traverse_instanced_bvh2_tri1_async(int32_t dev, const struct Node2* tlas_nodes, const struct RodentInstance* instances,
                                            const struct Node2* nodes, const struct Tri1* tris, const struct Ray1* rays,
                                            struct Hit1* hits, int32_t* hit_instances, int32_t num_rays, int32_t any_hit, void* stream);

/* Synchronous forms on the null stream: closest hit / any hit.  They abort() on the overflow flag, as the synchronous entries of
 * rodent_traversal.h do. */
void hip_intersect_instanced_bvh2_tri1(int32_t dev, const struct Node2* tlas_nodes, const struct RodentInstance* instances,
                                       const struct Node2* nodes, const struct Tri1* tris, const struct Ray1* rays, struct Hit1* hits,
                                       int32_t* hit_instances, int32_t num_rays);
void hip_occluded_instanced_bvh2_tri1(int32_t dev, const struct Node2* tlas_nodes, const struct RodentInstance* instances,
                                      const struct Node2* nodes, const struct Tri1* tris, const struct Ray1* rays, struct Hit1* hits,
                                      int32_t* hit_instances, int32_t num_rays);

/* The three above through a motion TLAS (rodent_hip_build_motion_tlas): `times` (DEVICE, one float per ray, required) holds every ray's
 * time; each instance a ray meets is placed, inverted and possibly skipped for that ray by the rules of "moving instances" at the top.
 * The overflow flag is reported as above. */
void hip_traverse_motion_instanced_bvh2_tri1_async(int32_t dev, const struct Node2* tlas_nodes,
                                                   const struct RodentMotionInstance* motion_instances, const struct Node2* nodes,
                                                   const struct Tri1* tris, const struct Ray1* rays, const float* times,
                                                   struct Hit1* hits, int32_t* hit_instances, int32_t num_rays, int32_t any_hit,
                                                   void* stream);
void hip_intersect_motion_instanced_bvh2_tri1(int32_t dev, const struct Node2* tlas_nodes,
                                              const struct RodentMotionInstance* motion_instances, const struct Node2* nodes,
                                              const struct Tri1* tris, const struct Ray1* rays, const float* times, struct Hit1* hits,
                                              int32_t* hit_instances, int32_t num_rays);
void hip_occluded_motion_instanced_bvh2_tri1(int32_t dev, const struct Node2* tlas_nodes,
                                             const struct RodentMotionInstance* motion_instances, const struct Node2* nodes,
                                             const struct Tri1* tris, const struct Ray1* rays, const float* times, struct Hit1* hits,
                                             int32_t* hit_instances, int32_t num_rays);

/* ---- deforming objects under moving instances (the section of that name at the top) ----
 * Bytes of device scratch rodent_hip_build_motion_objects needs: num_nodes / num_recs are the record counts of the PACKED ARRAYS (every
 * object's room; for a tight set listed whole they equal the plan's totals), refit_bytes what rodent_hip_refit_objects_plan returned for
 * the list.  -1 for a count < 1 or refit_bytes < 0.  Any 256-byte aligned buffer of that size, its contents are ignored. */
struct RodentMotionNode2;
struct RodentMotionTri1;
int64_t rodent_hip_motion_objects_scratch_bytes(int32_t num_nodes, int32_t num_recs, int64_t refit_bytes);

/* The forest form of rodent_hip_build_motion_bvh2_tri1 (rodent_motion.h): the two-key records of ALL objects of a packed set, over
 * vertices0 at time 0 and vertices1 at time 1.  DEVICE pointers: both vertex tables (num_vertices float4 rows each, the concatenated
 * tables), indices (num_rows int4 rows), nodes / tris (the packed topology, num_nodes Node2 / num_recs Tri1: only read), objects, ranges
 * (one RodentRefitRange per object, all objects in table order, from rodent_hip_refit_objects_plan, with its totals total_nodes /
 * total_recs), motion_nodes / motion_tris (room for num_nodes / num_recs motion records: record k of the packed arrays becomes motion
 * record k, so the object table serves both), scratch, info_dev (RODENT_BUILD_INFO_WORDS ints).  Asynchronous on `stream`: nothing is
 * allocated, nothing waits for the device.  The launch list is fixed whatever the number of objects: four device-to-device copies (the
 * packed arrays into scratch twice, copy A and copy B), rodent_hip_refit_objects' list on A with vertices0, the same on B with vertices1,
 * a memset of the info words, k_fuse_motion over the packed arrays.
 * info: [0] nodes completed at key 0 [1] records fused (num_nodes + num_recs) [2] the OR of all flags [3] nodes completed at key 1; a
 * sound call leaves [0] == [3] == total_nodes.  Per object the output is byte for byte what rodent_hip_build_motion_bvh2_tri1 writes for
 * that object alone; records outside every object (the unused room of a slotted set) are fused as they lie.  The flags are
 * rodent_hip_refit_objects' at either key and the fuse's; a flagged object is left incomplete, the others come out complete.  Calling it
 * again with moved keys is the refit.
 * Checks: those of rodent_hip_refit_objects in its order, each enqueuing nothing when it fails: RODENT_BUILD_ERR_NUM_TRIS,
 * RODENT_BUILD_ERR_NUM_VERTICES, RODENT_TLAS_ERR_NUM_OBJECTS, RODENT_BUILD_ERR_NUM_NODES (num_listed < 1, a negative total, num_nodes or
 * num_recs < 1, a total beyond its array's count), RODENT_BUILD_ERR_NULL, RODENT_BUILD_ERR_DEVICE. */
int32_t rodent_hip_build_motion_objects(int32_t dev, const float* vertices0, const float* vertices1, int32_t num_vertices,
                                        const int32_t* indices, int32_t num_rows, const struct Node2* nodes, int32_t num_nodes,
                                        const struct Tri1* tris, int32_t num_recs, const struct RodentObject* objects,
                                        int32_t num_objects, const struct RodentRefitRange* ranges, int32_t num_listed,
                                        int32_t total_nodes, int32_t total_recs, struct RodentMotionNode2* motion_nodes,
                                        struct RodentMotionTri1* motion_tris, void* scratch, int32_t* info_dev, void* stream);

/* Synchronous form on the null stream with its own scratch: copies the info words to `info` (host, may be NULL) and returns
 * RODENT_BUILD_ERR_INPUT when the device raised a flag or a node stayed incomplete at either key.  It checks RODENT_BUILD_ERR_NUM_NODES
 * and RODENT_BUILD_ERR_DEVICE first (it sizes and allocates the scratch), then as above. */
int32_t rodent_hip_build_motion_objects_sync(int32_t dev, const float* vertices0, const float* vertices1, int32_t num_vertices,
                                             const int32_t* indices, int32_t num_rows, const struct Node2* nodes, int32_t num_nodes,
                                             const struct Tri1* tris, int32_t num_recs, const struct RodentObject* objects,
                                             int32_t num_objects, const struct RodentRefitRange* ranges, int32_t num_listed,
                                             int32_t total_nodes, int32_t total_recs, struct RodentMotionNode2* motion_nodes,
                                             struct RodentMotionTri1* motion_tris, int32_t* info);

/* rodent_hip_build_motion_tlas / _sync over a motion object set: `nodes` is the objects' RodentMotionNode2 array (only the root record of
 * every object is read).  The same refusals in the same order, the same scratch (rodent_hip_motion_tlas_scratch_bytes), the same launch
 * list; only the instance stage differs, which reads the object box by the rule "Object box of a motion object". */
int32_t rodent_hip_build_motion_tlas_motion_objects(int32_t dev, const struct RodentMotionNode2* nodes,
                                                    const struct RodentObject* objects, int32_t num_objects,
                                                    const struct RodentMotionInstanceDesc* descs, int32_t num_instances,
                                                    int32_t max_leaf, struct Node2* tlas_nodes, struct RodentMotionInstance* instances,
                                                    void* scratch, int32_t* info_dev, void* stream);
int32_t rodent_hip_build_motion_tlas_motion_objects_sync(int32_t dev, const struct RodentMotionNode2* nodes,
                                                         const struct RodentObject* objects, int32_t num_objects,
                                                         const struct RodentMotionInstanceDesc* descs, int32_t num_instances,
                                                         int32_t max_leaf, struct Node2* tlas_nodes,
                                                         struct RodentMotionInstance* instances, int32_t* info);

/* The three motion traversal entries above through a motion TLAS over a motion object set: `times` is required and serves both levels; a
 * ray whose time is not in [0, 1] is a miss without any traversal.  hit_instances may be NULL.  The overflow flag is reported by
 * rodent_hip_check_errors; the synchronous forms abort() on it. */
void hip_traverse_motion_instanced_motion_bvh2_tri1_async(int32_t dev, const struct Node2* tlas_nodes,
                                                          const struct RodentMotionInstance* motion_instances,
                                                          const struct RodentMotionNode2* motion_nodes,
                                                          const struct RodentMotionTri1* motion_tris, const struct Ray1* rays,
                                                          const float* times, struct Hit1* hits, int32_t* hit_instances,
                                                          int32_t num_rays, int32_t any_hit, void* stream);
void hip_intersect_motion_instanced_motion_bvh2_tri1(int32_t dev, const struct Node2* tlas_nodes,
                                                     const struct RodentMotionInstance* motion_instances,
                                                     const struct RodentMotionNode2* motion_nodes,
                                                     const struct RodentMotionTri1* motion_tris, const struct Ray1* rays,
                                                     const float* times, struct Hit1* hits, int32_t* hit_instances, int32_t num_rays);
void hip_occluded_motion_instanced_motion_bvh2_tri1(int32_t dev, const struct Node2* tlas_nodes,
                                                    const struct RodentMotionInstance* motion_instances,
                                                    const struct RodentMotionNode2* motion_nodes,
                                                    const struct RodentMotionTri1* motion_tris, const struct Ray1* rays,
                                                    const float* times, struct Hit1* hits, int32_t* hit_instances, int32_t num_rays);

#ifdef __cplusplus
}
#endif
#endif /* RODENT_INSTANCES_H */
