#!/usr/bin/env python3
"""Compare the kernels of several translation units with those of one reference translation unit (gfx950 assembly from
`hipcc <the build's flags> --cuda-device-only -S`).
usage: scripts/isa/tu_compare.py <reference.s> <unit.s> [<unit.s> ...] [--diff]
For every kernel symbol (one `.amdhsa_kernel` block) two things are compared after the compiler's per-function label numbers
(.LBB<n>_, .Lfunc_end<n>, .LJTI<n>_, .Ltmp<n>) are normalised and comments dropped: the instruction text, and the kernel descriptor block (registers, spills,
scratch, LDS).  Prints one line per kernel -- unit, `same` or `differs` -- and fails when the units do not hold exactly the reference's
kernels, a kernel is in more than one unit, or a k_solve / k_predict instantiation differs.  --diff prints a unified diff of what differs."""
import difflib, os, re, sys

LABEL = re.compile(r'\.(LBB|Lfunc_end|Lfunc_begin|LJTI|Ltmp|LPC|LCPI)\d+')


def norm(lines):
    """the lines without comments (they carry the function's number too) and with the label numbers taken out"""
    code = (l.split(';')[0].rstrip() for l in lines)
    return [LABEL.sub(lambda m: '.' + m.group(1), l) for l in code if l]


def kernels(path):
    """kernel symbol -> (normalised body lines, normalised descriptor lines)"""
    lines = open(path).read().split('\n')
    out = {}
    desc_at = {m.group(1): i for i, l in enumerate(lines) for m in [re.match(r'\s*\.amdhsa_kernel\s+(\S+)', l)] if m}
    label_at = {m.group(1): i for i, l in enumerate(lines) for m in [re.match(r'^(\w+):', l)] if m and m.group(1) in desc_at}
    for name, d0 in desc_at.items():
        b0 = label_at[name]
        b1 = next(k for k in range(b0, len(lines)) if lines[k].startswith('.Lfunc_end'))
        d1 = next(k for k in range(d0, len(lines)) if '.end_amdhsa_kernel' in lines[k])
        out[name] = (norm(lines[b0:b1]), norm(lines[d0:d1 + 1]))
    return out


def main():
    paths = [a for a in sys.argv[1:] if not a.startswith('--')]
    ref, units = kernels(paths[0]), {os.path.splitext(os.path.basename(p))[0]: kernels(p) for p in paths[1:]}
    misplaced, differ, solver_differ = 0, 0, 0
    for name in sorted(ref):
        holders = [u for u, ks in units.items() if name in ks]
        if len(holders) != 1:
            print("%s %s" % (name, "MISSING" if not holders else "IN " + ",".join(holders)))
            misplaced += 1
            continue
        got = units[holders[0]][name]
        same = got == ref[name]
        print("%s %s %s" % (name, holders[0], "same" if same else "differs"))
        if not same:
            differ += 1
            solver_differ += 1 if re.search(r'k_(solve|predict)I', name) else 0
            if '--diff' in sys.argv:
                for part in (0, 1):
                    sys.stdout.writelines(l + '\n' for l in difflib.unified_diff(ref[name][part], got[part], 'reference', holders[0], lineterm='', n=2))
    extra = sorted({k for ks in units.values() for k in ks} - set(ref))
    for name in extra:
        print("%s NOT IN THE REFERENCE" % name)
    print("# %d kernels in the reference, %d in the units: %d differ (%d of them k_solve / k_predict), %d not in exactly one unit, %d not in the reference" %
          (len(ref), sum(len(ks) for ks in units.values()), differ, solver_differ, misplaced, len(extra)))
    sys.exit(1 if misplaced or extra or solver_differ else 0)


if __name__ == "__main__":
    main()
