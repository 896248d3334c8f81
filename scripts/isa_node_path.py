#!/usr/bin/env python
"""The node-only iteration of every BVH2 step loop of one kernel in a hipcc -S file: the shortest cycle of basic blocks through the block
that holds the node step's stack push (v_max3 / v_min3 ... ds_write_b32 offset:256) -- the path a wave takes when none of its lanes is on
a triangle and no rare block runs.  Branches inside the joint fetch's asm (.Ljoint labels) count as not taken, so both kinds of fetch are
counted.  Per loop: instructions, VALU, branches, v_cndmask, v_mov, saveexec and scratch instructions on the path, and the v_cndmask count
of the node block itself (LAB_NOTES 17, 18).  isa_hist.py gives the loop ranges; this gives the path.

  hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -munsafe-fp-atomics -Iinclude --cuda-device-only -S rodent_amd/csrc/traversal.hip -o t.s
  python scripts/isa_node_path.py t.s k_bvh2_top_autoILb0ELi15ELi255ELi16ELi32ELi0ELb1ELb0ELb1 [-v]
"""
import re, sys, heapq
from collections import Counter

def kernel_body(text, pat):
    for m in re.finditer(r"\n(_Z[^\n:]*):[^\n]*\n(.*?)\n\s*\.end_amdhsa_kernel", text, re.S):
        if pat in m.group(1):
            return m.group(2).split(".section")[0]
    raise SystemExit("no kernel " + pat)

def blocks_of(code):
    blocks, cur, name, n = [], [], "entry", 0
    def flush():
        nonlocal cur, name, n
        blocks.append((name, cur)); n += 1; cur = []; name = f"anon{n}"
    for line in code.split("\n"):
        t = line.strip()
        m = re.match(r"^(\.LBB\d+_\d+):", t)
        if m:
            if cur or name.startswith(".LBB"): flush()
            name = m.group(1); continue
        if line.startswith("\t") and t and not t.startswith((".", ";")):
            cur.append(t)
            if re.match(r"s_(cbranch_\w+|branch) \.LBB", t): flush()
            if t.startswith("s_endpgm"): flush()
    flush()
    return blocks

def main():
    text = open(sys.argv[1]).read()
    code = kernel_body(text, sys.argv[2])
    bl = blocks_of(code)
    idx = {name: i for i, (name, _) in enumerate(bl)}
    succ = []
    for i, (name, ins) in enumerate(bl):
        s = []
        last = ins[-1] if ins else ""
        m = re.match(r"s_(cbranch_\w+|branch) (\.LBB\d+_\d+)", last)
        if m: s.append(idx[m.group(2)])
        if not last.startswith(("s_branch", "s_endpgm")) and i + 1 < len(bl): s.append(i + 1)
        succ.append(s)
    nodes = [i for i, (_, ins) in enumerate(bl) if any(re.match(r"ds_write_b32 v\d+, v\d+ offset:256", x) for x in ins)
        and any(x.startswith("v_max3_f32") or x.startswith("v_max_f32") for x in ins)]
    rows = []
    for N in nodes:
        dist, prev = {}, {}
        pq = [(len(bl[s][1]), s, N) for s in succ[N]]
        heapq.heapify(pq)
        while pq:
            d, u, p = heapq.heappop(pq)
            if u in dist: continue
            dist[u] = d; prev[u] = p
            if u == N: break
            for v in succ[u]: heapq.heappush(pq, (d + len(bl[v][1]), v, u))
        if N not in dist: rows.append((bl[N][0], None)); continue
        path, u = [N], prev[N]
        while u != N: path.append(u); u = prev[u]
        path.reverse()                       # starts behind N ... ends with N
        ins = [x for b in path for x in bl[b][1]]
        op = Counter(x.split()[0] for x in ins)
        valu = sum(v for k, v in op.items() if k.startswith("v_"))
        br = sum(v for k, v in op.items() if k.startswith(("s_cbranch", "s_branch")))
        nb = bl[N][1]
        w = next(i for i, x in enumerate(nb) if re.match(r"ds_write_b32 v\d+, v\d+ offset:256", x))
        lastcmp = max(i for i, x in enumerate(nb[:w]) if x.startswith("v_cmp"))
        rows.append((bl[N][0], len(ins), valu, br, op["v_cndmask_b32_e32"] + op["v_cndmask_b32_e64"], op["v_mov_b32_e32"],
            sum(v for k, v in op.items() if "saveexec" in k), sum(1 for x in ins if x.startswith("scratch_")),
            sum(1 for x in nb if x.startswith("v_cndmask")), [bl[b][0] for b in path]))
    print("block: instr valu branches cndmask v_mov saveexec scratch | cndmask in node block")
    for r in rows:
        print(r[0], *r[1:9], "  path", " ".join(r[9]) if "-v" in sys.argv else "")

main()
