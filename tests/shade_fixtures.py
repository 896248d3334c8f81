"""Helpers of the per-vertex shader tests (test_shade_oracle.py on the CPU, test_gpu_shade.py on the GPU): stream slabs as word
arrays, what the oracle says a shader run leaves behind, walked paths, and the crafted edge-case vertices.

A stream of the renderer ABI is one slab: its arrays lie `cap` words apart in carve order (include/rodent_render.h).  Here a slab is a
uint32 array (rows, cap): every comparison is a comparison of bit patterns, so a NaN has to be the same NaN."""
import ctypes as C

import numpy as np

from oracle import binding as O

# rows of a primary / secondary slab
ID, ORG, DIR, TMIN, TMAX = 0, slice(1, 4), slice(4, 7), 7, 8
GEOM, PRIM, T, U, V, RND, MIS, CONTRIB, DEPTH = 9, 10, 11, 12, 13, 14, 15, slice(16, 19), 19
S_PRIM, S_COLOR = 9, slice(10, 13)
P_ROWS, S_ROWS = 20, 13
HIT_ROWS = slice(9, 14)
SENTINEL = np.uint32(0xCDCDCDCD)

f32, u32, i32 = np.float32, np.uint32, np.int32
FLT_MAX_REF = f32(3.4028234664e+38)
RAY_OFFSET = f32(0.001)                               # renderer.impala:46
SHADOW_TMAX = f32(f32(1.0) - RAY_OFFSET)


# corpus b of test_gpu_shade.py: the three scenes at 96 x 64, 1 spp, max_path_len 6
CAMERAS = {"cornell": ((0, 1, 2.7), (0, 0, -1), 60), "materials": ((0, 1, 2.6), (0, -0.05, -1), 60),
           "textured": ((0.3, 1.0, 3.2), (-0.1, -0.25, -1), 55)}
W, H, MAXLEN = 96, 64, 6


def camera(name, w=W, h=H):
    from rodent_amd import scene as S
    eye, d, fov = CAMERAS[name]
    return S.camera_settings(eye, d, (0, 1, 0), fov, w, h)


def bits(x):
    return np.ascontiguousarray(x, "<f4").view("<u4")


def word(x):
    return bits(np.array([x], "<f4"))[0]


def as_f32(words):
    return np.ascontiguousarray(words, "<u4").view("<f4")


def slab_cap(stream):
    """Words between two arrays of a carved stream."""
    return (stream.rays.org_x - stream.rays.id) // 4


def read_slab(R, stream, rows):
    cap = slab_cap(stream)
    return R.read_stream_array(stream.rays.id, rows * cap, "<u4").reshape(rows, cap)


def write_slab(R, stream, slab):
    assert slab.shape[1] == slab_cap(stream) and slab.dtype == np.uint32
    R.write_stream_array(stream.rays.id, np.ascontiguousarray(slab))


def read_film(R, dev=0):
    l = R.stage_lib()
    ptr, w, h = C.c_void_p(), C.c_int32(), C.c_int32()
    l.rodent_get_film_data(dev, C.byref(ptr), C.byref(w), C.byref(h))
    return R.read_stream_array(ptr.value, w.value * h.value * 3, "<f4").reshape(h.value * w.value, 3)


def vertices_of(slab, idx):
    """ORACLE_VERTEX records of the primary-slab entries `idx` (they must hold hits)."""
    v = np.zeros(len(idx), O.ORACLE_VERTEX)
    v["org"] = as_f32(slab[ORG][:, idx]).T
    v["dir"] = as_f32(slab[DIR][:, idx]).T
    v["prim"] = slab[PRIM, idx].view("<i4")
    for name, row in (("t", T), ("u", U), ("v", V), ("mis", MIS)):
        v[name] = as_f32(slab[row, idx])
    v["rnd"] = slab[RND, idx]
    v["contrib"] = as_f32(slab[CONTRIB][:, idx]).T
    v["depth"] = slab[DEPTH, idx].view("<i4")
    return v


def slab_of(vertices, ids, scene, cap, fill=SENTINEL):
    """A primary slab whose first len(vertices) entries hold the ORACLE_VERTEX records as hits (geom = indices[4 * prim + 3])."""
    n = len(vertices)
    s = np.full((P_ROWS, cap), fill, "<u4")
    s[ID, :n] = np.asarray(ids, "<i4").view("<u4")
    s[ORG, :n] = bits(vertices["org"].T)
    s[DIR, :n] = bits(vertices["dir"].T)
    s[TMIN, :n] = word(0.001); s[TMAX, :n] = word(FLT_MAX_REF)
    s[GEOM, :n] = scene.indices[vertices["prim"], 3].astype("<i4").view("<u4")
    s[PRIM, :n] = vertices["prim"].view("<u4")
    for name, row in (("t", T), ("u", U), ("v", V), ("mis", MIS)):
        s[row, :n] = bits(vertices[name])
    s[RND, :n] = vertices["rnd"]
    s[CONTRIB, :n] = bits(vertices["contrib"].T)
    s[DEPTH, :n] = vertices["depth"].view("<u4")
    return s


def mark_missed(slab, idx, scene):
    """Turns entries into rays that missed, as the traversal stage records them (geom = number of materials, prim -1)."""
    slab[GEOM, idx] = u32(len(scene.materials)); slab[PRIM, idx] = u32(0xFFFFFFFF)
    slab[T, idx] = word(FLT_MAX_REF); slab[U, idx] = 0; slab[V, idx] = 0


class Expected:
    """What shading the first n entries of primary slab `p` IN PLACE leaves behind, by the oracle: the primary slab, the secondary
    slab (from `s`), per entry the oracle's record (`shade`, valid where `live`) and the emission to add per entry."""

    def __init__(self, scene, p, s, n, max_path_len):
        self.live = np.zeros(p.shape[1], bool)
        self.live[:n] = p[GEOM, :n].view("<i4") < len(scene.materials)
        idx = np.flatnonzero(self.live)
        self.idx = idx
        self.vertices = vertices_of(p, idx)
        self.shade = o = O.shade_vertices(scene, self.vertices, max_path_len)
        self.primary, self.secondary = p.copy(), s.copy()
        P, S = self.primary, self.secondary
        pixel = p[ID, idx]
        P[ID, :n] = u32(0xFFFFFFFF); S[ID, :n] = u32(0xFFFFFFFF)
        b = o["bounce"] != 0; ib = idx[b]
        P[ID, ib] = pixel[b]
        P[ORG, ib] = bits(o["b_org"][b].T); P[DIR, ib] = bits(o["b_dir"][b].T)
        P[TMIN, ib] = word(RAY_OFFSET); P[TMAX, ib] = word(FLT_MAX_REF)
        P[RND, ib] = o["rnd"][b]; P[MIS, ib] = bits(o["mis"][b]); P[CONTRIB, ib] = bits(o["contrib"][b].T)
        P[DEPTH, ib] = (self.vertices["depth"][b] + 1).astype("<i4").view("<u4")
        sh = o["shadow"] != 0; ish = idx[sh]
        S[ID, ish] = pixel[sh]
        S[ORG, ish] = bits(o["s_org"][sh].T); S[DIR, ish] = bits(o["s_dir"][sh].T)
        S[TMIN, ish] = word(RAY_OFFSET); S[TMAX, ish] = word(SHADOW_TMAX)
        S[S_COLOR, ish] = bits(o["s_color"][sh].T)
        self.bounce = np.zeros(p.shape[1], bool); self.bounce[ib] = True
        e = o["emits"] != 0
        self.emit_pixel = pixel[e].view("<i4"); self.emitted = o["emitted"][e]

    def film_after(self, before, inv_spp):
        """The film after the run when no two emitting entries share a pixel: one float32 add per channel."""
        assert len(np.unique(self.emit_pixel)) == len(self.emit_pixel)
        after = before.copy()
        after[self.emit_pixel] = before[self.emit_pixel] + self.emitted * f32(inv_spp)
        return after


def first_difference(got, want, row_names=None):
    """'' if the slabs are equal, else where the first differing word is (row, entry, both words)."""
    if np.array_equal(got, want):
        return ""
    r, c = np.argwhere(got != want)[0]
    return f"{int((got != want).sum())} words differ; first: row {r} entry {c}: got 0x{got[r, c]:08x} ({as_f32(got[r:r + 1, c])[0]!r}), " \
           f"oracle 0x{want[r, c]:08x} ({as_f32(want[r:r + 1, c])[0]!r})"


def sentinel(stream, rows):
    """A slab of `rows` arrays with the stream's capacity, every word the sentinel."""
    return np.full((rows, slab_cap(stream)), SENTINEL, "<u4")


def assert_same(got, want, what):
    diff = first_difference(got, want)
    assert not diff, f"{what}: {diff}"


def compacted(primary_after, to_before, bounce):
    """The stable compaction of an in-place shaded slab into `to_before`: the rows the shader writes, survivors in stream order."""
    out = to_before.copy()
    idx = np.flatnonzero(bounce)
    for rows in (slice(0, 9), slice(14, 20)):                  # everything but the hit records
        out[rows, :len(idx)] = primary_after[rows][:, idx]
    return out, len(idx)


# ---- camera samples and walked paths -----------------------------------------------------------
def generated_slab(cam, iter_, width, height, first_ray_id, num_rays, first_pixel, spp, before, first_dst):
    """What hip_generate_rays leaves in slab `before` behind first_dst (row-band pixel order, mapping_gpu.impala:236-241)."""
    ray = first_ray_id + np.arange(num_rays)
    sample, pixel = ray % spp, first_pixel + ray // spp
    rnd, d = O.emit_samples(cam, iter_, width, height, pixel % width, pixel // width, sample)
    s = before.copy()
    dst = slice(first_dst, first_dst + num_rays)
    s[ID, dst] = pixel.astype("<i4").view("<u4")
    s[ORG, dst] = bits(np.asarray(cam["eye"], "<f4"))[:, None]
    s[DIR, dst] = bits(d.T)
    s[TMIN, dst] = word(0.0); s[TMAX, dst] = word(FLT_MAX_REF)
    s[RND, dst] = rnd; s[MIS, dst] = word(0.0); s[CONTRIB, dst] = word(1.0); s[DEPTH, dst] = 0
    return s


def walk_paths(scene, cam, iter_, spp, max_path_len, width, height, on_bounce=None):
    """The oracle's path tracer restated over emit_samples + traverse + shade_vertices, one bounce of all paths at a time.
    Returns the film (h, w, 3) float32: per pixel the additions happen in oracle_render's order (sample by sample, and along a
    path emission, shadow colour, next vertex), in float32.  on_bounce(bounce, vertices, shade) sees every shaded batch."""
    from rodent_amd import formats as F
    y, x, sample = [a.reshape(-1) for a in np.meshgrid(np.arange(height), np.arange(width), np.arange(spp), indexing="ij")]
    rnd, d = O.emit_samples(cam, iter_, width, height, x, y, sample)
    n = len(rnd)
    v = np.zeros(n, O.ORACLE_VERTEX)
    v["org"] = np.asarray(cam["eye"], "<f4"); v["dir"] = d; v["rnd"] = rnd; v["contrib"] = 1.0
    path = np.arange(n)                                        # index of the path (pixel-major, then sample) of every vertex
    tmin = np.zeros(n, "<f4")
    inv_spp = f32(1.0) / f32(spp)
    # per path: the list of its additions in order; paths of a pixel are consecutive
    adds = [[] for _ in range(n)]
    bounce = 0
    while len(v):
        hits, _ = O.traverse(2, scene.nodes, scene.tris, F.make_rays(v["org"], v["dir"], tmin, FLT_MAX_REF))
        hit = hits["tri_id"] >= 0
        v, path, hits = v[hit], path[hit], hits[hit]
        if not len(v):
            break
        v["prim"] = hits["tri_id"]; v["t"] = hits["t"]; v["u"] = hits["u"]; v["v"] = hits["v"]
        o = O.shade_vertices(scene, v, max_path_len)
        if on_bounce:
            on_bounce(bounce, v, o)
        sh = o["shadow"] != 0
        occl, _ = O.traverse(2, scene.nodes, scene.tris, F.make_rays(o["s_org"][sh], o["s_dir"][sh], RAY_OFFSET, SHADOW_TMAX), any_hit=True)
        lit = np.zeros(len(v), bool); lit[np.flatnonzero(sh)[occl["tri_id"] < 0]] = True
        for k in np.flatnonzero(o["emits"] != 0):
            adds[path[k]].append(o["emitted"][k] * inv_spp)
        for k in np.flatnonzero(lit):
            adds[path[k]].append(o["s_color"][k] * inv_spp)
        b = o["bounce"] != 0
        nv = np.zeros(int(b.sum()), O.ORACLE_VERTEX)
        nv["org"] = o["b_org"][b]; nv["dir"] = o["b_dir"][b]; nv["rnd"] = o["rnd"][b]; nv["mis"] = o["mis"][b]
        nv["contrib"] = o["contrib"][b]; nv["depth"] = v["depth"][b] + 1
        v, path = nv, path[b]
        tmin = np.full(len(v), RAY_OFFSET, "<f4")
        bounce += 1
    film = np.zeros((height * width, 3), "<f4")
    for k, a in enumerate(adds):                               # path order = pixel, then sample: oracle_render's loop nest
        for term in a:
            film[k // spp] += term
    return film.reshape(height, width, 3)


# ---- material classes -----------------------------------------------------------------------------
CLASSES = ("black", "diffuse", "phong", "mix", "mirror", "glass")


def material_class(scene, prim):
    """Per vertex: class name of the material it shades with, plus 'emitter' / 'textured' membership."""
    m = scene.materials[scene.indices[prim, 3]]
    return m["type"], m["emissive"] != 0, (m["tex_kd"] | m["tex_ks"]) != 0


def corpus_counts(scene, vertices, shade):
    """Vertices per material class, emitters, textured materials, back-face hits (entering == false) and depth >= 3."""
    t, emissive, textured = material_class(scene, vertices["prim"])
    fn = scene.face_normals[vertices["prim"], :3].astype("<f4")
    d = vertices["dir"]
    facing = (d[:, 0] * fn[:, 0] + d[:, 1] * fn[:, 1]) + d[:, 2] * fn[:, 2]           # dot() of the oracle, float32, same order
    out = {name: int(((t == k) & ~(emissive & (k == 0))).sum()) for k, name in enumerate(CLASSES)}      # (the lamp's BSDF is black too)
    out["emitter"] = int(emissive.sum()); out["textured"] = int(textured.sum())
    out["leaving"] = int((~(facing <= 0)).sum()); out["deep"] = int((vertices["depth"] >= 3).sum())
    return out


# ---- crafted vertices -----------------------------------------------------------------------------
def _unit(a):
    a = np.asarray(a, np.float64)
    return a / np.sqrt((a * a).sum())


def lum2(c):
    """2 * luminance((c, c, c)) as the shader computes it (float32, source order)."""
    c = f32(c)
    return f32(2.0) * ((c * f32(0.2126) + c * f32(0.7152)) + c * f32(0.0722))


def rr_threshold_contribs():
    """Grey contributions whose 2 * luminance straddles the Russian-roulette clamp 0.75: every float32 within 4 ulp of the
    crossing, so that values just below, at (when one exists) and above are all there."""
    c = f32(0.375)
    while lum2(c) >= f32(0.75):
        c = np.nextafter(c, f32(0))
    while lum2(np.nextafter(c, f32(1))) < f32(0.75):
        c = np.nextafter(c, f32(1))                            # c: the largest value below the clamp
    out = [c]
    for _ in range(3):
        out.insert(0, np.nextafter(out[0], f32(0)))
    for _ in range(4):
        out.append(np.nextafter(out[-1], f32(1)))
    assert lum2(out[3]) < f32(0.75) <= lum2(out[4])
    return out


GLASS_DEGREES = (30.0, 41.0, 41.8, 41.82, 42.5, 60.0)


def crafted_vertices(scene, max_path_len, replication, uv_extra=(), seed=1):
    """Edge-case vertices, one group per edge, every group over every material of the scene and `replication` random states.
    Returns (ORACLE_VERTEX array, group name per vertex).  The hit point is org + dir * t; the oracle and the shader take prim, u, v
    for the surface frame and the material, so a vertex need not be a hit that traversal could produce."""
    rng = np.random.default_rng(seed)
    prims = {}
    for prim in range(scene.num_tris):
        prims.setdefault(int(scene.indices[prim, 3]), prim)
    rows, groups = [], []

    def base(prim):
        v0, v1, v2 = (scene.vertices[scene.indices[prim, k], :3].astype(np.float64) for k in range(3))
        fn = scene.face_normals[prim, :3].astype(np.float64)
        return v0, v1, v2, fn, _unit(v1 - v0)

    def add(group, prim, u=0.3, v=0.4, dir_=None, t=1.5, mis=0.7, contrib=(0.9, 0.8, 0.7), depth=1, point=None, rnds=None):
        v0, v1, v2, fn, tan = base(prim)
        d = np.asarray(_unit(-0.8 * fn + 0.6 * tan) if dir_ is None else dir_, "<f4")
        p = (1.0 - u - v) * v0 + u * v1 + v * v2 if point is None else np.asarray(point, np.float64)
        org = (p - d.astype(np.float64) * min(float(t), 1e30)).astype("<f4")
        for rnd in (rng.integers(0, 2 ** 32, replication, dtype=np.uint64) if rnds is None else rnds):
            rows.append((org, d, prim, t, u, v, int(rnd), mis, contrib, depth)); groups.append(group)

    lamp = scene.lights[0]
    above_lamp = (lamp["v0"][:3].astype(np.float64) + lamp["v1"][:3] + lamp["v2"][:3]) / 3.0 - 0.004 * lamp["n"].astype(np.float64)
    one_up = float(np.nextafter(f32(0.5), f32(1)))
    for geom, prim in sorted(prims.items()):
        v0, v1, v2, fn, tan = base(prim)
        for d in (max_path_len - 1, max_path_len, max_path_len + 1):
            add("depth", prim, depth=d)
        add("contrib0", prim, contrib=(0.0, 0.0, 0.0))
        for c in rr_threshold_contribs():
            add("rr_clamp", prim, contrib=(c, c, c))
        add("rnd", prim, rnds=(0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF))
        for mis in (0.0, 1e30, np.inf):
            add("mis", prim, mis=mis)
        for t in (0.0, 1e30):
            add("t", prim, t=t)
        for u, v in ((0, 0), (1, 0), (0, 1), (0.5, 0), (0, 0.5), (0.5, 0.5), (0.5, one_up)) + tuple(uv_extra):
            add("uv", prim, u=u, v=v)
        add("backface", prim, dir_=_unit(0.8 * fn + 0.6 * tan))
        if scene.materials[geom]["type"] == 5:
            # leaving the glass: the critical angle of Ni = 1.5 is 41.81 degrees from the SHADING normal (interpolated: the slab's
            # corners are shared), turned towards the face normal so that the hit stays a back-face hit
            n0, n1, n2 = (scene.normals[scene.indices[prim, k], :3].astype(np.float64) for k in range(3))
            ns = _unit(0.3 * n0 + 0.3 * n1 + 0.4 * n2)
            ns = ns if ns @ fn > 0 else -ns
            side = fn - (fn @ ns) * ns
            side = _unit(side) if np.abs(side).max() > 1e-6 else tan
            for deg in GLASS_DEGREES:
                a = np.radians(deg)
                add("glass_inside", prim, dir_=np.cos(a) * ns + np.sin(a) * side)
        add("grazing", prim, dir_=_unit(tan - 1e-7 * fn))
        add("grazing", prim, dir_=np.where(np.abs(tan) > 0.5, np.sign(tan), 0.0) if np.abs(fn).max() == 1.0 else tan)
        add("above_lamp", prim, point=above_lamp)
    out = np.zeros(len(rows), O.ORACLE_VERTEX)
    for k, name in enumerate(("org", "dir", "prim", "t", "u", "v", "rnd", "mis", "contrib", "depth")):
        out[name] = [r[k] for r in rows]
    return out, np.array(groups)


def texel_border_uvs(scene):
    """Barycentrics for the textured scene's crafted set: texture coordinates that land exactly on texel borders of the largest
    map (k / width), and barycentrics outside the triangle, whose texture coordinates leave [0, 1) on both sides (repeat border)."""
    w = int(scene.textures["width"].max())
    on_border = tuple((k / (2.5 * w), j / (2.5 * w)) for k, j in ((1, 0), (3, 2), (w // 2, w // 4), (w - 1, 1)))
    return on_border + ((1.25, 0.5), (-0.25, 0.5), (0.5, -0.75), (2.0, 2.0))
