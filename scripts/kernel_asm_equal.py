"""Did a change leave every kernel's machine code alone, wherever the kernel now lives?  No GPU needed.

    for u in raymarch scene_bytes; do hipcc <the Makefile's flags> --cuda-device-only -S volym_amd/csrc/$u.hip -o new/$u.s; done   (and before/)
    python scripts/kernel_asm_equal.py before/*.s -- new/*.s

A kernel's code is the text between its label and its .Lfunc_end, without comments (they carry the function's index in its
unit) and without the digits of that index in .LBB<n>_, .LJTI<n>_, .Ltmp<n>, .Lfunc_begin<n>, .Lfunc_end<n>.  Prints the kernels
that differ or exist on one side only; exit status 1 if there are any."""
import re
import sys


def kernels(paths):
    out = {}
    for p in paths:
        txt = open(p).read()
        for name in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", txt, re.M):
            body = txt.split("\n%s:" % name, 1)[1]
            body = body[:re.search(r"^\.Lfunc_end\d+:", body, re.M).start()]
            body = re.sub(r";.*", "", body)
            body = re.sub(r"\.(LBB|LJTI|Ltmp|Lfunc_begin|Lfunc_end)\d+", r".\1", body)
            assert name not in out, "%s is defined in two units" % name
            out[name] = "\n".join(l.rstrip() for l in body.split("\n") if l.strip())
    return out


def main():
    cut = sys.argv.index("--")
    a, b = kernels(sys.argv[1:cut]), kernels(sys.argv[cut + 1:])
    bad = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
    for k in bad:
        print("%s: %s" % ("differs" if k in a and k in b else "only before" if k in a else "only after", k))
    print("%d kernels before, %d after, %d equal" % (len(a), len(b), len(set(a) | set(b)) - len(bad)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
