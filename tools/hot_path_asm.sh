#!/bin/bash
# tools/hot_path_asm.sh OUT.s "INSTANTIATION" [FROM TO] — assembly of one k_fast instantiation (compile only, no GPU), with the flags
# of tools/resource_usage.sh.  INSTANTIATION is the template argument list as resource_usage.sh prints it, e.g. "F F 2 5 F 0 F T"
# (M64 REC ENT WAVES TRACE POL WIDE LWT); POLICY and WIDE select the unit (default: policy 0, narrow).  Writes the kernel's
# function body to OUT.s and prints its branch instructions: all of them, those inside the step loop (the widest backward branch), and,
# with FROM and TO (basic-block labels such as .LBB3_12, or regular expressions that match a line), those between the two.
set -e
REPO=$(cd "$(dirname "$0")/.." && pwd)
CSRC=$REPO/optical-networking-gym_amd/csrc
out=$1; inst=$2; from=$3; to=$4
[ -n "$out" ] && [ -n "$inst" ] || { echo "usage: $0 OUT.s \"F F 2 5 F 0 F T\" [FROM TO]" >&2; exit 2; }
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -w -DONGYM_FAST_POLICY=${POLICY:-0} -DONGYM_FAST_WIDE=${WIDE:-0} \
  ${ONGYM_HIP_EXTRA_FLAGS:--mllvm -disable-machine-licm} --cuda-device-only -S -o "$tmp/unit.s" "$CSRC/ongym_fast.hip"
python3 - "$tmp/unit.s" "$out" "$inst" "$from" "$to" <<'PY'
import re, sys
src, out, inst, frm, to = sys.argv[1:6]
mangled = "_ZN5ongym6k_fastI" + "".join(
    {"T": "Lb1E", "F": "Lb0E"}.get(a, "Li%sE" % a) for a in inst.split()) + "EEvPKNS_6ParamsEiP14ongym_step_rec"
lines = open(src).read().splitlines()
a = next((i for i, l in enumerate(lines) if l.startswith(mangled + ":")), None)
if a is None:
    sys.exit("no such instantiation in this unit: " + mangled)
b = next(i for i in range(a, len(lines)) if lines[i].startswith(".Lfunc_end"))
body = lines[a:b]
open(out, "w").write("\n".join(body) + "\n")
br = re.compile(r"^\s+s_(c?branch\w*|setpc_b64)\b")
def count(ls):
    return sum(1 for l in ls if br.match(l))
print(f"{mangled}: {len(body)} lines, {count(body)} branch instructions")
# the step loop: the widest span between a label and a branch back to it (the printer's "Loop Header" comments do not help: the
# step loop's blocks are laid out around its cold arms and it carries no such comment)
label = re.compile(r"^(\.LBB\d+_\d+):")
at = {m.group(1): i for i, l in enumerate(body) for m in [label.match(l)] if m}
best = None
for j, l in enumerate(body):
    m = re.match(r"^\s+s_c?branch\w*\s+(\.LBB\d+_\d+)", l)
    if m and at.get(m.group(1), j) < j and (best is None or j - at[m.group(1)] > best[1] - best[0]):
        best = (at[m.group(1)], j, m.group(1))
if best:
    print(f"step loop {best[2]} (lines {best[0]}..{best[1]}): {count(body[best[0]:best[1] + 1])} branch instructions")
if frm and to:
    def find(pat, start=0):
        rx = re.compile(pat)
        return next(i for i in range(start, len(body)) if rx.search(body[i]))
    i = find(r"^" + re.escape(frm) + ":" if frm.startswith(".LBB") else frm)
    j = find(r"^" + re.escape(to) + ":" if to.startswith(".LBB") else to, i + 1)
    print(f"between {frm} (line {i}) and {to} (line {j}): {count(body[i:j])} branch instructions")
PY
