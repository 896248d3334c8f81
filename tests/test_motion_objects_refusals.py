"""The return code of the build entries of "deforming objects under moving instances" (include/rodent_instances.h) for every class of
refused argument, alone and in pairs, in the manner of tests/test_motion_bvh_refusals.py.

No GPU is needed and none is touched: every call passes dev = -1, so an otherwise valid call returns RODENT_BUILD_ERR_DEVICE before
anything is allocated, launched or dereferenced; the pointers are dummy non-zero integers.  For each entry, ORDER lists its refusals in
the order the entry tests them, `class: code`: a call with several bad arguments returns the code of the class that comes first; a class
an entry does not list is not looked at before the device, so the call returns -5.
"""
import itertools

import pytest

from rodent_amd import abi

NUM_TRIS, MAX_LEAF, NUM_VERTICES, NULL, DEVICE, NUM_NODES, NUM_INSTANCES, NUM_OBJECTS = -1, -2, -3, -4, -5, -11, -14, -15

OBJECT_POINTERS = ("vertices0", "vertices1", "indices", "nodes", "tris", "objects", "ranges", "motion_nodes", "motion_tris", "scratch",
                   "info_dev")
TLAS_POINTERS = ("motion_nodes", "objects", "descs", "tlas_nodes", "instances", "scratch", "info_dev")
CLASSES = {
    "num_tris": [("num_rows", 0), ("num_rows", (1 << 25) + 1)],
    "num_vertices": [("nv", 0)],
    "num_instances": [("num_instances", 0), ("num_instances", (1 << 22) + 1)],
    "max_leaf": [("max_leaf", 0), ("max_leaf", 9)],
    "num_objects": [("num_objects", 0)],
    "num_nodes": [("num_listed", 0), ("total_nodes", -1), ("total_recs", -1), ("num_nodes", 0), ("num_recs", 0), ("total_nodes", 48),
                  ("total_recs", 60)],
    **{f"null_{p}": [(p, None)] for p in sorted(set(OBJECT_POINTERS + TLAS_POINTERS))},
}
GOOD = dict(num_rows=50, nv=150, num_nodes=47, num_recs=50, num_objects=3, num_listed=3, total_nodes=47, total_recs=50, num_instances=9,
            max_leaf=2, vertices0=0x1000, vertices1=0x1100, indices=0x2000, nodes=0x3000, tris=0x4000, objects=0x9000, ranges=0xA000,
            motion_nodes=0x7000, motion_tris=0x8000, scratch=0x5000, info_dev=0x6000, descs=0xB000, tlas_nodes=0xC000, instances=0xD000)

BUILD = ("vertices0", "vertices1", "nv", "indices", "num_rows", "nodes", "num_nodes", "tris", "num_recs", "objects", "num_objects", "ranges",
         "num_listed", "total_nodes", "total_recs", "motion_nodes", "motion_tris")
TLAS = ("motion_nodes", "objects", "num_objects", "descs", "num_instances", "max_leaf", "tlas_nodes", "instances")
ENTRIES = {
    # the refusals of rodent_hip_refit_objects, in its order
    "rodent_hip_build_motion_objects": (BUILD + ("scratch", "info_dev", "stream"),
                                        {"num_tris": NUM_TRIS, "num_vertices": NUM_VERTICES, "num_objects": NUM_OBJECTS,
                                         "num_nodes": NUM_NODES, **{f"null_{p}": NULL for p in OBJECT_POINTERS}}),
    # (the sync form sizes its scratch first)
    "rodent_hip_build_motion_objects_sync": (BUILD + ("info",), {"num_nodes": NUM_NODES}),
    # the refusals of rodent_hip_build_motion_tlas, in its order
    "rodent_hip_build_motion_tlas_motion_objects": (TLAS + ("scratch", "info_dev", "stream"),
                                                    {"num_instances": NUM_INSTANCES, "max_leaf": MAX_LEAF, "num_objects": NUM_OBJECTS,
                                                     **{f"null_{p}": NULL for p in TLAS_POINTERS}}),
    "rodent_hip_build_motion_tlas_motion_objects_sync": (TLAS + ("info",), {"num_instances": NUM_INSTANCES, "max_leaf": MAX_LEAF}),
}
SIZE = "rodent_hip_motion_objects_scratch_bytes"


def call(l, entry, args, bad):
    a = {**GOOD, **bad, "stream": None, "info": None}
    return getattr(l, entry)(-1, *[a[k] for k in args])


def cases(args):
    """(classes that are bad, {argument: value}) for every single bad value the entry takes and every pair of classes."""
    mine = {c: [(k, v) for k, v in bad if k in args] for c, bad in CLASSES.items()}
    mine = {c: bad for c, bad in mine.items() if bad}
    for c, bad in mine.items():
        for k, v in bad:
            yield (c,), {k: v}
    for (c0, b0), (c1, b1) in itertools.combinations(mine.items(), 2):
        yield (c0, c1), dict([b0[0], b1[0]])


@pytest.fixture(scope="module")
def l(native_build):
    return abi.lib()


@pytest.mark.parametrize("entry", ENTRIES)
def test_refusal_codes_and_their_precedence(l, entry):
    args, order = ENTRIES[entry]
    assert call(l, entry, args, {}) == DEVICE                   # nothing wrong but the device
    rank = list(order)
    count = 0
    for classes, bad in cases(args):
        tested = [c for c in classes if c in order]
        want = order[min(tested, key=rank.index)] if tested else DEVICE
        assert call(l, entry, args, bad) == want, (entry, bad)
        count += 1
    assert count >= 2 * len(order)


def test_the_scratch_entry_refuses_with_minus_one(l):
    size = getattr(l, SIZE)
    refit = l.rodent_hip_refit_scratch_bytes(1000, 1200)
    assert size(47, 50, 256) > 0 and size(1, 1, 0) > 0
    for nodes, recs, bytes_ in ((0, 50, 256), (47, 0, 256), (-1, 50, 256), (47, -5, 256), (47, 50, -1), (0, 0, -1)):
        assert size(nodes, recs, bytes_) == -1
    # room for both copies of the packed topology, both refits' info words and the plan's refit scratch, each on a 256-byte boundary
    assert size(1000, 1200, refit) >= 2 * (1000 * 64 + 1200 * 48) + 32 + refit
    assert size(1000, 1200, refit) % 256 == 0
    # one object listed whole is the single-mesh build's scratch
    assert size(1000, 1200, refit) == l.rodent_hip_motion_bvh2_scratch_bytes(1000, 1200)
