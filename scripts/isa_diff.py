#!/usr/bin/env python3
"""Per-kernel text comparison of two ISA listings of the renderer's kernels. Usage: isa_diff.py OLD NEW

Each input is a `make -C sphereflake-raytracer_amd isa` listing (build/sf_kernels.s) or an
`llvm-objdump -d --no-show-raw-insn --no-leading-addr` dump of a device code object. The input is split per sf_*
kernel; comments, directives and blank lines are dropped, local labels are renumbered in order of appearance
(their numbers carry the function's position in the file), and a dump's resolved pc-relative address literal is
masked (it moves when a kernel before it changes size). Prints `kernel  n_old  n_new  SAME|DIFF`, lists the
kernels present on one side only, and exits 1 on any DIFF."""
import re
import sys


def kernels(path):
    out, cur = {}, None
    for line in open(path, errors="replace"):
        line = re.split(r";|//", line)[0].strip()
        m = re.match(r"<?(\w+)>?:$", line)                 # `name:` (listing) or `<name>:` (dump)
        if m or line.startswith(".Lfunc_end"):
            cur = out.setdefault(m.group(1), []) if m and m.group(1).startswith("sf_") else None
        elif cur is not None and line and line != "..." and (not line.startswith(".") or line.endswith(":")):
            if cur and cur[-1].startswith("s_getpc_b64"):   # a dump's resolved pc-relative address moves with the layout
                line = re.sub(r"0x[0-9a-f]+$", "pcrel", line)
            cur.append(line)
    for name, body in out.items():
        while body and body[-1] in ("s_nop 0", "s_code_end"):   # alignment padding behind the kernel in a dump
            body.pop()
        labels = {}
        out[name] = [re.sub(r"\.L\w+", lambda l: labels.setdefault(l.group(0), ".L%d" % len(labels)), s) for s in body]
    return out


old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
diff = 0
for k in sorted(old.keys() & new.keys()):
    same = old[k] == new[k]
    diff += not same
    print("%-28s %6d %6d  %s" % (k, len(old[k]), len(new[k]), "SAME" if same else "DIFF"))
for k in sorted(old.keys() - new.keys()):
    print("%-28s %6d      -  only in OLD (removed)" % (k, len(old[k])))
for k in sorted(new.keys() - old.keys()):
    print("%-28s      - %6d  only in NEW (added)" % (k, len(new[k])))
print("%d kernels compared, %d DIFF" % (len(old.keys() & new.keys()), diff))
sys.exit(1 if diff else 0)
