"""The return code of rodent_hip_build_objects / _sync (include/rodent_instances.h) for every class of refused argument, alone and in
pairs, and the plan function's -1 cases and totals.

No GPU is needed and none is touched, in the manner of tests/test_build_refusals.py: every call passes dev = -1, so an otherwise valid
call returns RODENT_BUILD_ERR_DEVICE before anything is allocated, launched or dereferenced; the pointers are dummy non-zero integers.
ORDER lists the refusals in the order the entry tests them; a call with several bad arguments returns the code of the class that comes
first.
"""
import itertools

import numpy as np
import pytest

from rodent_amd import abi, formats as F

NUM_TRIS, MAX_LEAF, NUM_VERTICES, NULL, DEVICE, INPUT, NUM_NODES, NUM_OBJECTS = -1, -2, -3, -4, -5, -7, -11, -15
POINTERS = ("vertices", "indices", "nodes", "tris", "objects", "ranges", "scratch", "object_info", "info_dev")
GOOD = dict(vertices=0x1000, nv=36, indices=0x2000, num_rows=12, max_leaf=2, mode=1, nodes=0x3000, tris=0x4000, objects=0x5000,
            num_objects=3, ranges=0x6000, num_listed=2, total_tris=12, scratch=0x7000, object_info=0x8000, info_dev=0x9000)
CLASSES = {
    "num_rows": [("num_rows", 0), ("num_rows", (1 << 25) + 1)],
    "num_vertices": [("nv", 0)],
    "num_objects": [("num_objects", 0)],
    "counts": [("num_listed", 0), ("num_listed", (1 << 20) + 1), ("total_tris", 0), ("total_tris", (1 << 25) + 1)],
    "max_leaf": [("max_leaf", 0), ("max_leaf", 9)],
    "mode": [("mode", 2), ("mode", -1)],
    **{f"null_{p}": [(p, None)] for p in POINTERS},
}
ORDER = {"num_rows": NUM_TRIS, "num_vertices": NUM_VERTICES, "num_objects": NUM_OBJECTS, "counts": NUM_NODES, "max_leaf": MAX_LEAF,
         "mode": INPUT, **{f"null_{p}": NULL for p in POINTERS}}
ARGS = ("vertices", "nv", "indices", "num_rows", "max_leaf", "mode", "nodes", "tris", "objects", "num_objects", "ranges", "num_listed",
        "total_tris", "scratch", "object_info", "info_dev")


@pytest.fixture(scope="module")
def l(native_build):
    return abi.lib()


def call(l, bad):
    a = {**GOOD, **bad}
    return l.rodent_hip_build_objects(-1, *[a[k] for k in ARGS], None)


def cases():
    for c, bad in CLASSES.items():
        for k, v in bad:
            yield (c,), {k: v}
    for (c0, b0), (c1, b1) in itertools.combinations(CLASSES.items(), 2):
        yield (c0, c1), dict([b0[0], b1[0]])


def test_refusal_codes_and_their_precedence(l):
    assert call(l, {}) == DEVICE                                 # nothing wrong but the device
    rank, count = list(ORDER), 0
    for classes, bad in cases():
        assert call(l, bad) == ORDER[min(classes, key=rank.index)], bad
        count += 1
    assert count >= 2 * len(ORDER)


def test_both_modes_pass_the_checks(l):
    assert call(l, {"mode": 0}) == DEVICE and call(l, {"mode": 1}) == DEVICE


def test_sync_form_checks_the_counts_then_the_device(l):
    a = dict(GOOD)
    sync = lambda **bad: l.rodent_hip_build_objects_sync(-1, *[{**a, **bad}[k] for k in ARGS[:13]], None, None)
    assert sync() == DEVICE
    for k, v in CLASSES["counts"]:
        assert sync(**{k: v}) == NUM_NODES, (k, v)
    assert sync(max_leaf=0) == DEVICE and sync(num_rows=0) == DEVICE      # not looked at before the device


def plan(l, listed, first, count, num_listed=None, null=()):
    listed, first, count = (np.ascontiguousarray(a, np.int32) for a in (listed, first, count))
    k = len(listed) if num_listed is None else num_listed
    ranges, totals = np.zeros(max(len(listed), 1), F.REFIT_RANGE), np.full(2, -7, np.int32)
    ptr = {"listed": listed.ctypes.data, "first": first.ctypes.data, "count": count.ctypes.data, "ranges": ranges.ctypes.data,
           "totals": totals.ctypes.data}
    for name in null:
        ptr[name] = None
    need = l.rodent_hip_build_objects_plan(ptr["listed"], ptr["first"], ptr["count"], k, ptr["ranges"], ptr["totals"])
    return need, ranges, totals


def test_plan_fills_prefix_sums_and_totals(l):
    need, ranges, totals = plan(l, [2, 0, 7], [40, 0, 9], [5, 12, 1])
    assert need > 0 and need % 256 == 0 and totals[0] == 18
    assert ranges["object"].tolist() == [2, 0, 7] and ranges["first_tri"].tolist() == [40, 0, 9]
    assert ranges["num_tris"].tolist() == [5, 12, 1]
    assert ranges["rec_start"].tolist() == [0, 5, 17] and ranges["node_start"].tolist() == [0, 5, 17]
    # more triangles or more objects never need less scratch
    assert plan(l, [0, 1, 2], [0, 5, 17], [5, 12, 2])[0] >= need and plan(l, [0], [0], [18])[0] <= need


def test_plan_refuses_with_minus_one(l):
    for name in ("listed", "first", "count", "ranges", "totals"):
        assert plan(l, [0], [0], [4], null=(name,))[0] == -1, name
    assert plan(l, [0], [0], [4], num_listed=0)[0] == -1
    assert plan(l, [0], [0], [4], num_listed=(1 << 20) + 1)[0] == -1
    assert plan(l, [0, 1], [0, 4], [4, 0])[0] == -1 and plan(l, [0, 1], [0, 4], [4, -3])[0] == -1
    assert plan(l, [0, 1], [0, 0], [1 << 25, 1])[0] == -1
    assert plan(l, [0], [0], [1 << 25])[0] > 0
