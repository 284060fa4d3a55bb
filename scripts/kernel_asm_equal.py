"""Did a change leave every kernel's machine code alone, wherever the kernel now lives?  No GPU needed.

    for u in raymarch scene_bytes; do hipcc <the Makefile's flags> --cuda-device-only -S volym_amd/csrc/$u.hip -o new/$u.s; done   (and before/)
    python scripts/kernel_asm_equal.py [--rename OLD=NEW ...] before/*.s -- new/*.s

A kernel's code is the text between its label and its .Lfunc_end, without comments (they carry the function's index in its
unit) and without the digits of that index in .LBB<n>_, .LJTI<n>_, .Ltmp<n>, .Lfunc_begin<n>, .Lfunc_end<n>.  Prints the kernels
that differ or exist on one side only; exit status 1 if there are any.

--rename OLD=NEW: a type or a kernel changed its name.  OLD is replaced by NEW in the names and the code of the kernels before; give
the mangled spelling with its length, as in 13SurfaceSelect=9BoxSelect.  Kernels before that come to share one name -- copies that
became one kernel -- must each equal the kernel of that name after."""
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
    args, renames = sys.argv[1:], []
    while args and args[0] == "--rename":
        renames.append(args[1].split("=", 1))
        args = args[2:]
    cut = args.index("--")
    b = kernels(args[cut + 1:])
    a = []                                                  # (name after the renames, code after them, name before)
    for name, code in kernels(args[:cut]).items():
        new, was = name, name
        for old, to in renames:
            new, code = new.replace(old, to), code.replace(old, to)
        a.append((new, code, was))
    bad = 0
    for new, code, was in sorted(a):
        if b.get(new) != code:
            print("%s: %s" % ("differs" if new in b else "only before", was if new == was else "%s -> %s" % (was, new)))
            bad += 1
        elif new != was:
            print("equal: %s -> %s" % (was, new))
    for k in sorted(set(b) - {new for new, _, _ in a}):
        print("only after: %s" % k)
        bad += 1
    print("%d kernels before, %d after, %d of those before equal" % (len(a), len(b), len(a) - bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
