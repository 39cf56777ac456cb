#!/usr/bin/env python3
"""Instruction census of one k_fast instantiation along the fixed paths of a branch walk (no GPU).

    tools/hot_path_asm.sh OUT.s "F F 2 5 F 0 F T"
    python tools/path_census.py OUT.s profiles/r26_hot_path_branches.txt "this tree" [--prices profiles/r27_scalar_port_ubench.txt]

The walk file lists, per case, every branch instruction on the path with its line in OUT.s and whether it is taken
(profiles/r26_hot_path_branches.txt: sections "==== case N, TREE: ...").  The census starts at the label of the first listed
branch's block, follows the listed decisions (any branch that is not listed, or listed out of order, is an error: the assembly is
not the one the walk was made on) and stops behind the last listed branch.  Every instruction on the way falls into one class; the
classes are priced in clocks per SIMD at 5 waves per SIMD from the rows of tools/ubench/issue_rates.hip (--prices), as the
project prices its pipes in DESIGN.md section 5."""
import argparse
import collections
import re

FOUR_CLOCK = re.compile(r"^v_(\w+_f64|\w+_dpp|mov_b32_dpp|readlane_b32|readfirstlane_b32|writelane_b32|mbcnt_\w+|mul_lo_u32|mul_hi_u32|mul_hi_i32|"
                        r"alignbit_b32|lshlrev_b64|lshrrev_b64|ashrrev_i64|mov_b64\w*|mad_u64_u32|mad_i64_i32|cvt_f64_\w+|cvt_\w+_f64\w*|"
                        r"permlane\w+|cmp\w*_[fiu]64\w*|cndmask_b64)$")


def klass(op, args):
    if op.startswith("s_cbranch") or op in ("s_branch", "s_setpc_b64"):
        return "branch"
    if op == "s_waitcnt":
        return "s_waitcnt"
    if op == "s_nop":
        return "s_nop"
    if op.startswith(("s_load", "s_buffer_load", "s_memtime", "s_memrealtime")):
        return "smem"
    if op.startswith("s_"):
        return "salu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "vmem"
    if op.startswith("v_"):
        if "dpp" in args or "row_" in args or "quad_perm" in args or FOUR_CLOCK.match(op.replace("_e32", "").replace("_e64", "")):
            return "valu4"
        return "valu2"
    return "other"


def parse_walk(path, tree):
    cases, cur = collections.OrderedDict(), None
    for l in open(path):
        m = re.match(r"^==== (case \w+), (.*?):", l)
        if m:
            cur = cases.setdefault(m.group(1), []) if m.group(2) == tree else None
            continue
        m = re.match(r"^\s*(\d+)\s+(\.LBB\d+_\d+)\s+(s_\w+)\s+(\.LBB\d+_\d+)\s+(TAKEN|not taken)", l)
        if m and cur is not None:
            cur.append((int(m.group(1)), m.group(2), m.group(3), m.group(4), m.group(5) == "TAKEN"))
    return cases


def prices_of(path):
    rows = {}
    for l in open(path):
        m = re.match(r"^(\S.*?)\s{2,}([\d.]+)\s+([\d.]+)\s+([\d.]+)\s+([\d.]+)\s+([\d.]+)\s*$", l)
        if m:
            rows[m.group(1)] = float(m.group(5))            # the 5 waves per SIMD column
    add = rows["s_add_u32"]
    return {"salu": add, "valu4": rows["v_fma_f64"], "valu2": rows["v_add_u32 (4 indep)"], "lds": rows["ds_read_b32 x4 + wait"],
            # what the second instruction of a pair adds to the s_add_u32 in front of it (a port of its own would add nothing)
            "branch": rows["pair s_add + branch n.t."] - add, "taken": rows["pair s_add + branch n.t."] - add + rows["s_cbranch_scc0 taken +1"] - rows["s_cbranch_scc1 not taken"],
            "s_nop": rows["pair s_add + s_nop 0"] - add, "s_waitcnt": rows["pair s_add + s_waitcnt"] - add}


def census(body, walk):
    label = {m.group(1): i for i, l in enumerate(body) for m in [re.match(r"^(\.LBB\d+_\d+):", l)] if m}
    i, todo = label[walk[0][1]], list(walk)
    count, ops, blocks = collections.Counter(), collections.defaultdict(collections.Counter), []
    block, bc = walk[0][1], collections.Counter()
    while True:
        l = body[i]
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            blocks.append((block, bc)); block, bc = m.group(1), collections.Counter()
        m = re.match(r"^\s+([sv]_\w+|ds_\w+|global_\w+|flat_\w+|buffer_\w+|scratch_\w+)\s*(.*)$", l)
        if m and not l.lstrip().startswith(";"):
            k = klass(m.group(1), m.group(2))
            count[k] += 1; bc[k] += 1; ops[k][re.sub(r"_e(32|64)$", "", m.group(1))] += 1
            if k == "branch":
                line, _, op, target, taken = todo.pop(0)
                if line != i + 1 or op != m.group(1):
                    raise SystemExit(f"line {i + 1}: {l.strip()} is not the walk's next branch ({line} {op})")
                if taken:
                    count["taken"] += 1; bc["taken"] += 1
                    i = label[target] - 1
                if not todo:
                    blocks.append((block, bc))
                    return count, ops, blocks
        i += 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("asm"); ap.add_argument("walk"); ap.add_argument("tree")
    ap.add_argument("--prices", default=None)
    ap.add_argument("--blocks", action="store_true", help="also print the counts block by block")
    a = ap.parse_args()
    body = open(a.asm).read().splitlines()
    price = prices_of(a.prices) if a.prices else None
    cols = ("salu", "branch", "taken", "s_waitcnt", "s_nop", "smem", "valu4", "valu2", "lds", "vmem")
    allops = collections.defaultdict(collections.Counter)
    print(f"{'case':10s}" + "".join(f"{c:>10s}" for c in cols) + f"{'all':>8s}" + ("   scalar port  vector pipe  LDS   (clocks per wave)" if price else ""))
    for name, walk in parse_walk(a.walk, a.tree).items():
        count, ops, blocks = census(body, walk)
        for k, c in ops.items():
            allops[k].update(c)
        total = sum(v for k, v in count.items() if k != "taken")
        row = f"{name:10s}" + "".join(f"{count[c]:10d}" for c in cols) + f"{total:8d}"
        if price:
            sc = count["salu"] * price["salu"] + (count["branch"] - count["taken"]) * price["branch"] + count["taken"] * price["taken"] \
                + count["s_waitcnt"] * price["s_waitcnt"] + count["s_nop"] * price["s_nop"]
            row += f"   {sc:11.0f}  {count['valu4'] * price['valu4'] + count['valu2'] * price['valu2']:11.0f}  {count['lds'] * price['lds']:4.0f}"
        print(row)
        if a.blocks:
            for b, bc in blocks:
                if sum(bc.values()):
                    print(f"    {b:12s}" + "".join(f"{bc[c]:10d}" for c in cols))
    if price:
        print("prices (clocks per SIMD at 5 waves per SIMD): " + " ".join(f"{k} {v:.2f}" for k, v in price.items()))
    print("opcodes by class (all cases together):")
    for k in cols:
        if allops[k]:
            print(f"  {k}: " + " ".join(f"{o} {n}" for o, n in sorted(allops[k].items())))


if __name__ == "__main__":
    main()
