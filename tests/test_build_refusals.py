"""The return code of every builder and refit entry of include/rodent_build.h for every class of refused argument, alone and in pairs.

No GPU is needed and none is touched: every call passes dev = -1, so an otherwise valid call returns RODENT_BUILD_ERR_DEVICE before anything
is allocated, launched or dereferenced; the pointers are dummy non-zero integers.

Pinned twice: tests/golden/build_refusals.json holds the recorded return value of every case ("entry [(argument, value), ...]": code; for
the size entries the sign), and ORDER states the rule behind the table.  For each entry, ORDER lists its refusals in the order the entry
tests them, `class: code`.  A call with several bad arguments returns the code of the class that comes first; a class an entry does not
list is not looked at before the device, so the call returns -5.  The *_scratch_bytes / _max_refs forms return -1 when any listed class
is bad and a positive count otherwise.
"""
import ctypes as C
import itertools
import json
from pathlib import Path

import pytest

from rodent_amd import abi

NUM_TRIS, MAX_LEAF, NUM_VERTICES, NULL, DEVICE, PASSES, COST, SPLIT, NUM_NODES = -1, -2, -3, -4, -5, -8, -9, -10, -11
NAN = float("nan")

# class -> the bad values of the issue's list (argument name, value); the first of a class stands for it in the pairs
CLASSES = {
    "num_tris": [("n", 0), ("n", (1 << 25) + 1)],
    "max_leaf": [("max_leaf", 0), ("max_leaf", 9)],
    "passes": [("passes", -1), ("passes", 4)],
    "cost": [("node_cost", 0.0), ("node_cost", NAN), ("node_cost", 2e6), ("tri_cost", 0.0), ("tri_cost", NAN), ("tri_cost", 2e6)],
    "budget": [("budget", -1.0), ("budget", NAN), ("budget", 4.5)],
    "max_pieces": [("max_pieces", 0), ("max_pieces", 65)],
    "num_vertices": [("nv", 0)],
    "num_nodes": [("num_nodes", 0), ("num_bvh_tris", 0)],
    **{f"null_{p}": [(p, None)] for p in ("vertices", "indices", "opt", "split", "nodes", "tris", "scratch", "info_dev")},
}
GOOD = dict(n=12, nv=36, max_leaf=2, passes=2, node_cost=1.2, tri_cost=1.0, budget=1.0, max_pieces=8, num_nodes=11, num_bvh_tris=12,
            vertices=0x1000, indices=0x2000, opt=True, split=True, nodes=0x3000, tris=0x4000, scratch=0x5000, info_dev=0x6000)

MESH = ("vertices", "nv", "indices", "n")
OUT = ("nodes", "tris", "scratch", "info_dev", "stream")
OUT_SYNC = ("nodes", "tris", "info")
REFIT = MESH + ("nodes", "num_nodes", "tris", "num_bvh_tris")
ARG_CHECKS = {"num_tris": NUM_TRIS, "max_leaf": MAX_LEAF, "num_vertices": NUM_VERTICES,
              **{f"null_{p}": NULL for p in ("vertices", "indices", "nodes", "tris", "scratch", "info_dev")}}
OPT_CHECKS = {"null_opt": NULL, "max_leaf": MAX_LEAF, "passes": PASSES, "cost": COST}
SPLIT_CHECKS = {"null_split": NULL, "budget": SPLIT, "max_pieces": SPLIT}

# entry -> (its arguments after dev, ORDER); dicts keep the order they are written in
ENTRIES = {
    "rodent_hip_build_bvh2_tri1": (MESH + ("max_leaf",) + OUT, ARG_CHECKS),
    "rodent_hip_build_bvh2_tri1_sync": (MESH + ("max_leaf",) + OUT_SYNC, {"num_tris": NUM_TRIS, "max_leaf": MAX_LEAF}),
    "rodent_hip_build_bvh2_tri1_opt": (MESH + ("opt",) + OUT, {**OPT_CHECKS, **{k: v for k, v in ARG_CHECKS.items() if k != "max_leaf"}}),
    "rodent_hip_build_bvh2_tri1_opt_sync": (MESH + ("opt",) + OUT_SYNC, {**OPT_CHECKS, "num_tris": NUM_TRIS}),
    "rodent_hip_build_bvh2_tri1_split": (MESH + ("opt", "split") + OUT,
                                         {**OPT_CHECKS, **SPLIT_CHECKS, **{k: v for k, v in ARG_CHECKS.items() if k != "max_leaf"}}),
    "rodent_hip_build_bvh2_tri1_split_sync": (MESH + ("opt", "split") + OUT_SYNC, {**OPT_CHECKS, **SPLIT_CHECKS, "num_tris": NUM_TRIS}),
    "rodent_hip_refit_bvh2_tri1": (REFIT + ("scratch", "info_dev", "stream"),
                                   {"num_tris": NUM_TRIS, "num_vertices": NUM_VERTICES, "num_nodes": NUM_NODES,
                                    **{f"null_{p}": NULL for p in ("vertices", "indices", "nodes", "tris", "scratch", "info_dev")}}),
    "rodent_hip_refit_bvh2_tri1_sync": (REFIT + ("info",), {"num_nodes": NUM_NODES}),
}
# size entry -> (its arguments, the classes that make it return -1)
SIZES = {
    "rodent_hip_build_scratch_bytes": (("n",), ("num_tris",)),
    "rodent_hip_build_opt_scratch_bytes": (("n", "opt"), ("num_tris", *OPT_CHECKS)),
    "rodent_hip_build_split_max_refs": (("n", "split"), ("num_tris", *SPLIT_CHECKS)),
    "rodent_hip_build_split_scratch_bytes": (("n", "opt", "split"), ("num_tris", *OPT_CHECKS, *SPLIT_CHECKS)),
    "rodent_hip_refit_scratch_bytes": (("num_nodes", "num_bvh_tris"), ("num_nodes",)),
}
OPT_FIELDS, SPLIT_FIELDS = ("max_leaf", "passes", "node_cost", "tri_cost"), ("budget", "max_pieces")


def applies(name, args):
    """Whether the entry with arguments `args` takes argument `name` (option fields travel inside opt / split)."""
    return name in args or (name in OPT_FIELDS and "opt" in args) or (name in SPLIT_FIELDS and "split" in args)


def call(l, entry, args, bad):
    """One call of `entry` with GOOD overridden by `bad` ({argument: value}); dev = -1 on the entries that take a device."""
    a = {**GOOD, **bad}
    opt = abi.BuildOptions(a["max_leaf"], a["passes"], a["node_cost"], a["tri_cost"])
    split = abi.SplitOptions(a["budget"], a["max_pieces"])
    given = {"opt": C.byref(opt) if a["opt"] else None, "split": C.byref(split) if a["split"] else None, "stream": None, "info": None}
    values = [given[k] if k in given else a[k] for k in args]
    return getattr(l, entry)(*values) if entry in SIZES else getattr(l, entry)(-1, *values)


def cases(args):
    """(classes that are bad, {argument: value}) for every single bad value the entry takes and every pair of classes."""
    mine = {c: [(k, v) for k, v in bad if applies(k, args)] for c, bad in CLASSES.items()}
    mine = {c: bad for c, bad in mine.items() if bad}
    for c, bad in mine.items():
        for k, v in bad:
            yield (c,), {k: v}
    for (c0, b0), (c1, b1) in itertools.combinations(mine.items(), 2):
        yield (c0, c1), dict([b0[0], b1[0]])


def observed(l):
    """{"entry bad arguments": return value (its sign for the size entries)} over every case, in the form of the recorded table."""
    out = {}
    for entry, (args, _) in {**ENTRIES, **SIZES}.items():
        sign = (lambda v: v) if entry in ENTRIES else (lambda v: (v > 0) - (v < 0))
        out[f"{entry} none"] = sign(call(l, entry, args, {}))
        for _, bad in cases(args):
            out[f"{entry} {sorted(bad.items(), key=str)!r}"] = sign(call(l, entry, args, bad))
    return out


@pytest.fixture(scope="module")
def l(native_build):
    return abi.lib()


def test_every_case_returns_its_recorded_code(l):
    recorded = json.loads((Path(__file__).parent / "golden" / "build_refusals.json").read_text())
    got = observed(l)
    assert sorted(recorded) == sorted(got)
    assert {k: v for k, v in got.items() if recorded[k] != v} == {}


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


@pytest.mark.parametrize("entry", SIZES)
def test_size_entries_refuse_with_minus_one(l, entry):
    args, refusing = SIZES[entry]
    assert call(l, entry, args, {}) > 0
    for classes, bad in cases(args):
        got = call(l, entry, args, bad)
        assert (got == -1) if any(c in refusing for c in classes) else (got > 0), (entry, bad)
