// instance_inverse.h -- the ONE inverse of instanced scenes (include/rodent_instances.h): bvh_build.hip's instance stages (build_tlas.h)
// store it per instance, traversal.hip's k_instanced_motion (traversal_instanced.h) takes it per ray and per instance of the matrix
// interpolated at the ray's time.  Included inside each translation unit's namespace.  CPU model: tests/instance_model.py (invert).
#pragma once
// world_to_object of object_to_world `m` (rows of 4): the cofactor inverse in fp64 in the header's order, each entry rounded to fp32
// once.  Returns RODENT_TLAS_BAD_TRANSFORM or 0.
__device__ __forceinline__ int invert_affine(const float m[12], float w[12]) {
    bool ok = true;
    for (int k = 0; k < 12; k++) ok = ok && isfinite(m[k]);
    const double a = m[0], b = m[1], c = m[2], tx = m[3], d = m[4], e = m[5], f = m[6], ty = m[7], g = m[8], h = m[9], i = m[10],
                 tz = m[11];
    const double c0 = e * i - f * h, c1 = f * g - d * i, c2 = d * h - e * g;
    const double det = (a * c0 + b * c1) + c * c2;
    const double r = 1.0 / det;
    const double q[9] = {c0 * r, (c * h - b * i) * r, (b * f - c * e) * r,
                         c1 * r, (a * i - c * g) * r, (c * d - a * f) * r,
                         c2 * r, (b * g - a * h) * r, (a * e - b * d) * r};
    for (int k = 0; k < 3; k++) {
        for (int j = 0; j < 3; j++) w[4 * k + j] = (float)q[3 * k + j];
        w[4 * k + 3] = (float)-((q[3 * k] * tx + q[3 * k + 1] * ty) + q[3 * k + 2] * tz);
    }
    ok = ok && det != 0.0 && isfinite(det);
    for (int k = 0; k < 12; k++) ok = ok && isfinite(w[k]);
    return ok ? 0 : RODENT_TLAS_BAD_TRANSFORM;
}

// The placement of a motion instance at time t, entry by entry: s = 1 - t; m = s * m0 + t * m1 -- two products and one sum, each rounded
// (the translation units are compiled with -ffp-contract=off), so t = 0 gives m0 and t = 1 gives m1, bit for bit.  t is used as given.
__device__ __forceinline__ void lerp_affine(const float m0[12], const float m1[12], float t, float m[12]) {
    const float s = 1.0f - t;
    for (int k = 0; k < 12; k++) m[k] = s * m0[k] + t * m1[k];
}
