"""The return code of the three PLOC entries of include/rodent_build.h for every class of refused argument, alone and in pairs, in the
manner of tests/test_build_refusals.py: no GPU is needed and none is touched, every call passes dev = -1, so an otherwise valid call
returns RODENT_BUILD_ERR_DEVICE before anything is allocated, launched or dereferenced; the pointers are dummy non-zero integers.

ORDER lists an entry's refusals in the order it tests them: the options' checks as the split entry has them (the split options' only
when they are given: NULL means no pre-splitting), a NULL `ploc`, RODENT_BUILD_ERR_PLOC, then the mesh arguments.  A call with several
bad arguments returns the code of the class that comes first."""
import ctypes as C
import itertools

import pytest

from rodent_amd import abi

NUM_TRIS, MAX_LEAF, NUM_VERTICES, NULL, DEVICE, PASSES, COST, SPLIT, PLOC = -1, -2, -3, -4, -5, -8, -9, -10, -16
NAN = float("nan")

CLASSES = {
    "null_opt": [("opt", None)],
    "max_leaf": [("max_leaf", 0), ("max_leaf", 9)],
    "passes": [("passes", -1), ("passes", 4)],
    "cost": [("node_cost", 0.0), ("node_cost", NAN), ("tri_cost", 2e6)],
    "budget": [("budget", -1.0), ("budget", NAN), ("budget", 4.5)],
    "max_pieces": [("max_pieces", 0), ("max_pieces", 65)],
    "null_ploc": [("ploc", None)],
    # out of range; then a limit below clog2(12) = 4, below clog2 of the 24 references the split options allow, and below 56 with passes
    "ploc": [("radius", 0), ("radius", 65), ("depth_limit", -1), ("depth_limit", 57), ("wide_iterations", -2), ("wide_iterations", 256),
             ("depth_limit", 3), ("depth_limit", 55)],
    "num_tris": [("n", 0), ("n", (1 << 25) + 1)],
    "num_vertices": [("nv", 0)],
    **{f"null_{p}": [(p, None)] for p in ("vertices", "indices", "nodes", "tris", "scratch", "info_dev")},
}
GOOD = dict(n=12, nv=36, max_leaf=2, passes=2, node_cost=1.2, tri_cost=1.0, budget=1.0, max_pieces=8, radius=8, depth_limit=0,
            wide_iterations=-1, vertices=0x1000, indices=0x2000, opt=True, split=True, ploc=True, nodes=0x3000, tris=0x4000,
            scratch=0x5000, info_dev=0x6000)
CODES = {"null_opt": NULL, "max_leaf": MAX_LEAF, "passes": PASSES, "cost": COST, "budget": SPLIT, "max_pieces": SPLIT, "null_ploc": NULL,
         "ploc": PLOC, "num_tris": NUM_TRIS, "num_vertices": NUM_VERTICES,
         **{f"null_{p}": NULL for p in ("vertices", "indices", "nodes", "tris", "scratch", "info_dev")}}
OPTIONS = ("null_opt", "max_leaf", "passes", "cost", "budget", "max_pieces", "null_ploc", "ploc")
MESH = ("vertices", "nv", "indices", "n", "opt", "split", "ploc")
ENTRIES = {
    "rodent_hip_build_bvh2_tri1_ploc": (MESH + ("nodes", "tris", "scratch", "info_dev", "stream"), tuple(CODES)),
    "rodent_hip_build_bvh2_tri1_ploc_sync": (MESH + ("nodes", "tris", "info"), OPTIONS + ("num_tris",)),
}
SIZE = "rodent_hip_build_ploc_scratch_bytes"
SIZE_ARGS, SIZE_REFUSING = ("n", "opt", "split", "ploc"), OPTIONS + ("num_tris",)
FIELDS = {"opt": ("max_leaf", "passes", "node_cost", "tri_cost"), "split": ("budget", "max_pieces"),
          "ploc": ("radius", "depth_limit", "wide_iterations")}


def call(l, entry, args, bad, with_split=True):
    a = {**GOOD, **bad}
    opt = abi.BuildOptions(a["max_leaf"], a["passes"], a["node_cost"], a["tri_cost"])
    split = abi.SplitOptions(a["budget"], a["max_pieces"])
    ploc = abi.PlocOptions(a["radius"], a["depth_limit"], a["wide_iterations"])
    given = {"opt": C.byref(opt) if a["opt"] else None, "split": C.byref(split) if with_split else None,
             "ploc": C.byref(ploc) if a["ploc"] else None, "stream": None, "info": None}
    values = [given[k] if k in given else a[k] for k in args]
    return getattr(l, entry)(*values) if entry == SIZE else getattr(l, entry)(-1, *values)


def cases(args, with_split):
    def applies(name):
        return name in args or any(name in FIELDS[s] and s in args for s in FIELDS)
    mine = {c: [(k, v) for k, v in bad if applies(k)] for c, bad in CLASSES.items() if with_split or c not in ("budget", "max_pieces")}
    mine = {c: bad for c, bad in mine.items() if bad}
    for c, bad in mine.items():
        for k, v in bad:
            yield (c,), {k: v}
    for (c0, b0), (c1, b1) in itertools.combinations(mine.items(), 2):
        if b0[0][0] != b1[0][0]:
            yield (c0, c1), dict([b0[0], b1[0]])


@pytest.fixture(scope="module")
def l(native_build):
    return abi.lib()


@pytest.mark.parametrize("with_split", [True, False])
@pytest.mark.parametrize("entry", ENTRIES)
def test_refusal_codes_and_their_precedence(l, entry, with_split):
    args, order = ENTRIES[entry]
    assert call(l, entry, args, {}, with_split) == DEVICE            # nothing wrong but the device
    count = 0
    for classes, bad in cases(args, with_split):
        tested = [c for c in classes if c in order]
        want = CODES[min(tested, key=order.index)] if tested else DEVICE
        assert call(l, entry, args, bad, with_split) == want, (entry, bad)
        count += 1
    assert count >= 2 * len(order)


@pytest.mark.parametrize("with_split", [True, False])
def test_size_entry_refuses_with_minus_one(l, with_split):
    assert call(l, SIZE, SIZE_ARGS, {}, with_split) > 0
    for classes, bad in cases(SIZE_ARGS, with_split):
        got = call(l, SIZE, SIZE_ARGS, bad, with_split)
        assert (got == -1) if any(c in SIZE_REFUSING for c in classes) else (got > 0), bad


def test_depth_limit_against_the_reference_count(l):
    entry, (args, _) = "rodent_hip_build_bvh2_tri1_ploc", ENTRIES["rodent_hip_build_bvh2_tri1_ploc"]
    zero = {"passes": 0}
    # 12 triangles: clog2 = 4; with the split options (budget 1) up to 24 references: clog2 = 5
    assert call(l, entry, args, {**zero, "depth_limit": 4}, with_split=False) == DEVICE
    assert call(l, entry, args, {**zero, "depth_limit": 4}, with_split=True) == PLOC
    assert call(l, entry, args, {**zero, "depth_limit": 5}, with_split=True) == DEVICE
    assert call(l, entry, args, {**zero, "depth_limit": 3}, with_split=False) == PLOC
    assert call(l, entry, args, {"depth_limit": 55}, with_split=False) == PLOC           # below 56 with treelet passes
    assert call(l, entry, args, {"depth_limit": 56}, with_split=False) == DEVICE
    # the limit is held against the reference count only when num_tris is in range: otherwise num_tris is what is refused
    assert call(l, entry, args, {**zero, "depth_limit": 3, "n": 0}, with_split=False) == NUM_TRIS
    assert call(l, entry, args, {**zero, "radius": 0, "n": 0}, with_split=False) == PLOC
    assert call(l, SIZE, SIZE_ARGS, {**zero, "depth_limit": 3}, with_split=False) == -1


def test_python_options_refuse_what_the_library_refuses():
    from rodent_amd import gpubuild
    for kw in ({"radius": 0}, {"radius": 65}, {"radius": 8, "depth_limit": -1}, {"radius": 8, "depth_limit": 57},
               {"radius": 8, "wide_iterations": -2}, {"radius": 8, "wide_iterations": 256}):
        with pytest.raises(gpubuild.BuildError):
            gpubuild.ploc_options(**kw)
    o = gpubuild.ploc_options(16)
    assert (o.radius, o.depth_limit, o.wide_iterations) == (16, 0, -1)
