#!/usr/bin/env python3
"""Did a source change move any kernel?  Compare device-only assembly listings kernel by kernel.

    cd gymwipe_amd/csrc
    hipcc $(make -s print-flags) --cuda-device-only -S -o new/FILE.s -x hip FILE.hip      # per file, at both revisions
    python tools/kernel_isa_diff.py old/ct_rollout_sfx.s -- new/ct_rollout_*.s

Each side is one or more `-S` outputs; their kernels are pooled by symbol, so a file may be cut into several (or several merged)
between the two sides.  Per kernel two things are compared:
  * the instruction text: everything from the kernel's label to its descriptor, comments and blank lines dropped, `.LBB<n>_<m>`
    with the function's index <n> taken out and `.Ltmp<n>` renumbered in order of appearance;
  * its resources: the `.amdhsa_` descriptor block and the kernel's entry in the `amdhsa.kernels` metadata (VGPRs, SGPRs, LDS,
    private segment, kernarg layout).
Prints the kernels found on one side only, the kernels that differ with the first line that does, and a count of the rest.
Exit status 0 only if both sides have the same kernels and none differs.  Plain Python, no GPU."""
import re
import sys

LBB = re.compile(r"\.LBB\d+_")
LTMP = re.compile(r"\.Ltmp\d+")


def clean(lines):
    """Comments, trailing blanks and empty lines dropped; local labels made independent of the kernel's place in its file."""
    tmp = {}
    out = []
    for ln in lines:
        ln = ln.split(";", 1)[0].rstrip()
        if not ln.strip():
            continue
        ln = LBB.sub(".LBB_", ln)
        ln = LTMP.sub(lambda m: tmp.setdefault(m.group(0), ".Ltmp#%d" % len(tmp)), ln)
        out.append(ln)
    return out


def kernels_of(path):
    """{symbol: (instruction lines, resource lines)} of one listing."""
    with open(path) as f:
        lines = f.read().split("\n")
    desc_at = {}                                         # symbol -> (first, last) line of its .amdhsa_kernel block
    i = 0
    while i < len(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", lines[i])
        if m:
            j = i
            while not lines[j].strip().startswith(".end_amdhsa_kernel"):
                j += 1
            desc_at[m.group(1)] = (i, j)
            i = j
        i += 1
    label_at = {}
    for i, ln in enumerate(lines):
        m = re.match(r"(\S+):", ln)
        if m and m.group(1) in desc_at:
            label_at[m.group(1)] = i
    # the metadata: items of the `amdhsa.kernels:` list, each keyed by its `.name:`
    meta = {}
    try:
        i = lines.index("amdhsa.kernels:") + 1
    except ValueError:
        i = len(lines)
    item = None
    while i < len(lines) and (lines[i].startswith(" ") or not lines[i]):
        if lines[i].startswith("  - "):
            item = []
        if item is not None:
            item.append(lines[i])
            m = re.match(r"\s+\.name:\s+(\S+)", lines[i])
            if m and lines[i].startswith("    .name:"):
                meta[m.group(1)] = item
        i += 1
    out = {}
    for name, (d0, d1) in desc_at.items():
        if name not in label_at or name not in meta:
            sys.exit("%s: kernel %s has no label or no metadata entry" % (path, name))
        code = [ln for ln in lines[label_at[name] + 1:d0] if not re.match(r"\s*\.(section|p2align)\b", ln)]
        out[name] = (clean(code), clean(lines[d0:d1 + 1]) + clean(meta[name]))
    return out


def side(paths):
    pool = {}
    for p in paths:
        for name, k in kernels_of(p).items():
            if name in pool:
                sys.exit("%s: kernel %s appears in two listings of one side" % (p, name))
            pool[name] = k
    return pool


def first_difference(a, b):
    for i, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return "line %d: %r != %r" % (i + 1, x.strip(), y.strip())
    return "%d lines != %d lines" % (len(a), len(b))


def main(argv):
    if "--" not in argv or argv[0] == "--" or argv[-1] == "--":
        sys.exit(__doc__)
    cut = argv.index("--")
    old, new = side(argv[:cut]), side(argv[cut + 1:])
    only_old, only_new = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    for title, names in (("only in OLD", only_old), ("only in NEW", only_new)):
        print("%s: %d" % (title, len(names)))
        for n in names:
            print("    " + n)
    differ = 0
    for n in sorted(set(old) & set(new)):
        what = [part + ", " + first_difference(o, w)
                for part, o, w in (("instructions", old[n][0], new[n][0]), ("resources", old[n][1], new[n][1])) if o != w]
        if what:
            differ += 1
            print("differs: %s\n    %s" % (n, "\n    ".join(what)))
    same = len(set(old) & set(new)) - differ
    print("kernels: %d OLD, %d NEW; %d differ; %d identical in instructions and resources" % (len(old), len(new), differ, same))
    return 0 if not only_old and not only_new and not differ else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
