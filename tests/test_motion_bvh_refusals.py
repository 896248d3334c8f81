"""The return code of the motion build, fuse and scratch entries of include/rodent_motion.h for every class of refused argument, alone
and in pairs, in the manner of tests/test_build_refusals.py.

No GPU is needed and none is touched: every call passes dev = -1, so an otherwise valid call returns RODENT_BUILD_ERR_DEVICE before
anything is allocated, launched or dereferenced; the pointers are dummy non-zero integers.  For each entry, ORDER lists its refusals in
the order the entry tests them, `class: code`: a call with several bad arguments returns the code of the class that comes first; a class
an entry does not list is not looked at before the device, so the call returns -5.
"""
import itertools

import pytest

from rodent_amd import abi

NUM_TRIS, NUM_VERTICES, NULL, DEVICE, NUM_NODES = -1, -3, -4, -5, -11

CLASSES = {
    "num_tris": [("n", 0), ("n", (1 << 25) + 1)],
    "num_vertices": [("nv", 0)],
    "num_nodes": [("num_nodes", 0), ("num_bvh_tris", 0), ("num_nodes", -3)],
    **{f"null_{p}": [(p, None)] for p in ("vertices0", "vertices1", "indices", "nodes", "tris", "nodes1", "tris1", "motion_nodes",
                                         "motion_tris", "scratch", "info_dev")},
}
GOOD = dict(n=12, nv=36, num_nodes=11, num_bvh_tris=12, vertices0=0x1000, vertices1=0x1100, indices=0x2000, nodes=0x3000, tris=0x4000,
            nodes1=0x3100, tris1=0x4100, motion_nodes=0x7000, motion_tris=0x8000, scratch=0x5000, info_dev=0x6000)

BUILD = ("vertices0", "vertices1", "nv", "indices", "n", "nodes", "num_nodes", "tris", "num_bvh_tris", "motion_nodes", "motion_tris")
# the refusals of rodent_hip_refit_bvh2_tri1, in its order
REFIT_ORDER = {"num_tris": NUM_TRIS, "num_vertices": NUM_VERTICES, "num_nodes": NUM_NODES}
ENTRIES = {
    "rodent_hip_build_motion_bvh2_tri1": (BUILD + ("scratch", "info_dev", "stream"),
                                          {**REFIT_ORDER, **{f"null_{p}": NULL for p in ("vertices0", "vertices1", "indices", "nodes", "tris",
                                                                                        "motion_nodes", "motion_tris", "scratch",
                                                                                        "info_dev")}}),
    "rodent_hip_build_motion_bvh2_tri1_sync": (BUILD + ("info",), {"num_nodes": NUM_NODES}),
    "rodent_hip_fuse_motion_bvh2_tri1": (("nodes", "tris", "nodes1", "tris1", "num_nodes", "num_bvh_tris", "motion_nodes", "motion_tris",
                                          "info_dev", "stream"),
                                         {"num_nodes": NUM_NODES, **{f"null_{p}": NULL for p in ("nodes", "tris", "nodes1", "tris1",
                                                                                                "motion_nodes", "motion_tris", "info_dev")}}),
}
SIZE = "rodent_hip_motion_bvh2_scratch_bytes"


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
    assert size(11, 12) > 0 and size(1, 1) > 0
    for nodes, recs in ((0, 12), (11, 0), (-1, 12), (11, -5), (0, 0)):
        assert size(nodes, recs) == -1
    # room for both copies of the topology, both refits' info words and one refit scratch, each array on a 256-byte boundary
    assert size(1000, 1200) >= 2 * (1000 * 64 + 1200 * 48) + 32 + l.rodent_hip_refit_scratch_bytes(1000, 1200)
    assert size(1000, 1200) % 256 == 0
