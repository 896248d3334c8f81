"""The CPU model of deforming meshes in the renderer (tests/deforming_scene_model.py) against the rules of include/rodent_render.h: the
conditions of tests/deforming_scene_fixtures.py on the model alone, the model's frame beside the flat oracle's where the two must agree
(every time 0; equal keys), the depth word at the last depths, the creation's refusal of a moved emitter and the host's smooth
normals."""
import copy

import numpy as np
import pytest

import deforming_scene_fixtures as X
import deforming_scene_model as DM
import scene_update_model as SU
import shade_fixtures as SF
from conftest import GOLDEN
from rodent_amd import render as R

F32 = np.float32
FILM_RTOL, FILM_ATOL = 1e-5, 1e-6                        # tests/test_gpu_render.py's
W, H, SPP, MAXLEN = X.W, X.H, X.SPP, X.MAXLEN


@pytest.fixture(scope="module")
def parts(oracle, tmp_path_factory):
    return X.parts(GOLDEN, tmp_path_factory.mktemp("deforming_model"))


def flat_frame(parts, monkeypatch):
    """(film, [primary rays, shadow rays]) of the flat oracle's path tracer (shade_fixtures.walk_paths) over the key-0 scene with the
    model's topology -- given the same random states: the flat walk draws no shutter sample, so its emit_samples is wrapped to hand
    it the state behind the third draw."""
    flat = copy.copy(parts.scene)
    flat.nodes, flat.tris = parts.topology
    emit = SF.O.emit_samples
    monkeypatch.setattr(SF.O, "emit_samples", lambda *a: (lambda rnd, d: (DM.third_draw(rnd)[0], d))(*emit(*a)))
    counts = [W * H * SPP, 0]

    def on_bounce(bounce, v, o):
        counts[0] += int((o["bounce"] != 0).sum()); counts[1] += int((o["shadow"] != 0).sum())
    film = SF.walk_paths(flat, X.camera(), 0, SPP, MAXLEN, W, H, on_bounce=on_bounce)
    monkeypatch.setattr(SF.O, "emit_samples", emit)
    return film, counts


# ---- the conditions -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shutter", X.SHUTTERS)
def test_the_fixtures_meet_their_conditions(parts, shutter):
    frame = X.model_frame(parts, shutter)
    figures = X.check_conditions(parts, frame, shutter)
    print(shutter, frame.counts, figures)
    assert frame.counts[0] > W * H * SPP and frame.counts[1] > 500 and frame.film.mean() > 0.02
    seeded, ubits = X.seeded_rays(parts)
    n = len(seeded) // 4
    assert (DM.shutter_time(ubits[n:2 * n], *shutter) == F32(0.5)).all() and len(seeded) % 64 != 0


def test_the_keys_move_the_boxes_and_the_quad_only(parts):
    k, scene = parts.keys, parts.scene
    movers = np.concatenate([parts.tall, parts.short, parts.quad])
    assert len(parts.tall) == len(parts.short) == 20 and len(parts.quad) == 4
    rest = np.setdiff1d(np.arange(len(k.vertices0)), movers)
    assert k.vertices0[rest].tobytes() == k.vertices1[rest].tobytes() and k.normals0[rest].tobytes() == k.normals1[rest].tobytes()
    assert (k.vertices0[movers, :3] != k.vertices1[movers, :3]).any(1).mean() > 0.7        # (the boxes' feet stay on the floor)
    slide = k.vertices1[parts.short, 0] - k.vertices0[parts.short, 0]
    assert np.allclose(slide, X.SLIDE, atol=1e-6)
    # the quad turns over: its face normal's z changes sign between the keys
    f0, f1 = (SU.face_normals(v, scene.indices)[parts.quad_tris, 2] for v in (k.vertices0, k.vertices1))
    assert (f0 * f1 < 0).all()


# ---- the frame ----------------------------------------------------------------------------------------------------------------------------
def test_shutter_0_0_is_the_flat_frame_of_key_0(parts, monkeypatch):
    """With every time 0 a value is 1 * x0 + 0 * x1 = x0 (a -0 becomes +0, which changes no product's value), the records' widened
    bounds change which nodes a ray visits but no hit, and the face normal from the corners is the converter's own rule: the frame is
    the flat oracle's of the key-0 scene (on this scene the rule's face normals equal the converter's bit for bit, all 38).  Ties:
    none differed -- the ray counts are equal and the films agree within the GPU tests' tolerance."""
    moving = X.model_frame(parts, (0.0, 0.0))
    film, counts = flat_frame(parts, monkeypatch)
    assert moving.counts == counts and counts[0] > W * H * SPP and counts[1] > 500
    assert np.allclose(moving.film, film, rtol=FILM_RTOL, atol=FILM_ATOL) and film.mean() > 0.02


@pytest.mark.parametrize("shutter", [(0.0, 1.0), (0.25, 0.75), (1.0, 1.0)])
def test_equal_keys_give_the_flat_frame_under_any_shutter(parts, monkeypatch, shutter):
    """Both keys equal to key 0: s * x + t * x equals x up to the rounding of that sum, so rays hit where the flat ones do up to the
    last bits; the same paths, the same counts, the film within the tolerance."""
    k = parts.keys
    still = X.model_frame(parts, shutter, keys=DM.Keys(k.vertices0, k.vertices0, k.normals0, k.normals0))
    film, counts = flat_frame(parts, monkeypatch)
    assert still.counts == counts
    assert np.allclose(still.film, film, rtol=FILM_RTOL, atol=FILM_ATOL)


# ---- the depth word -------------------------------------------------------------------------------------------------------------------------
def test_the_depth_word_survives_the_last_depths():
    ubits = np.array([0, 1, 1 << 22, (1 << 23) - 1], np.int64)
    for depth in (0, 254):
        words = DM.pack(np.full(4, depth), ubits)
        d, u = R.unpack_depth_time(words)
        assert (d == depth).all() and np.array_equal(u, ubits) and (words >= 0).all()
        # the shader's step: (depth + 1) | the bits above the depth
        on = ((words & DM.DEPTH_MASK) + 1) | (words & ~np.int32(DM.DEPTH_MASK))
        d, u = R.unpack_depth_time(on)
        assert (d == depth + 1).all() and np.array_equal(u, ubits)
        assert np.array_equal(on, R.pack_depth_time(np.full(4, depth + 1), ubits))
    assert min(300, DM.DEPTH_MASK) == 255


# ---- the refusal and the host's normals -------------------------------------------------------------------------------------------------------
def test_a_moved_emitter_corner_is_a_moving_light(parts):
    scene, k = parts.scene, parts.keys
    assert not DM.moving_light(scene, k.vertices1) and not DM.moving_light(scene, k.vertices0)
    ix = np.asarray(scene.indices).reshape(-1, 4)
    emitters = np.flatnonzero(np.asarray(scene.materials)["emissive"][ix[:, 3]] != 0)
    assert len(emitters) == 2
    for word in range(4):                                                   # one ulp in any word of a corner row, the fourth included
        moved = k.vertices1.copy()
        row = ix[emitters[1], 2]
        moved[row, word] = np.nextafter(moved[row, word], F32(9))
        assert DM.moving_light(scene, moved)
    other = k.vertices1.copy(); other[parts.tall[0], 0] += F32(0.5)
    assert not DM.moving_light(scene, other)


def test_the_hosts_smooth_normals_are_the_models(parts):
    ix = np.asarray(parts.scene.indices)
    for v in (parts.keys.vertices0, parts.keys.vertices1):
        want = SU.smooth_normals(SU.face_normals(v, ix), ix, len(v))
        assert R.smooth_normals(v, ix).tobytes() == want.tobytes()
    assert parts.keys.normals1.tobytes() == R.smooth_normals(parts.keys.vertices1, ix).tobytes()
    v, ix2, _, _ = SU.indexed_soup(200, 7, twice=True)                       # a fan, an unnamed vertex, a degenerate triangle
    assert R.smooth_normals(v, ix2).tobytes() == SU.smooth_normals(SU.face_normals(v, ix2), ix2, len(v)).tobytes()
