"""What the *_resources tests of the passes share (no test here): where the units are, which compiler, the Makefile's flags and the
reading of the compiler's kernel-resource-usage remarks."""
import os
import re
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "volym_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def makefile_flags():
    """ARCH and CXXFLAGS as volym_amd/csrc/Makefile states them (the product build, no DEV), warnings dropped"""
    text = open(os.path.join(CSRC, "Makefile")).read()
    var = lambda name: re.search(r"^%s\s*[:?]?=\s*(.*)$" % name, text, re.M).group(1).split()
    return ["--offload-arch=" + var("ARCH")[0]] + [f for f in var("CXXFLAGS") if not f.startswith("-W")]


def makefile_units():
    """the names in the Makefile's UNITS list: the HIP units, one object each"""
    text = open(os.path.join(CSRC, "Makefile")).read()
    return re.search(r"^UNITS\s*:=\s*(.*)$", text, re.M).group(1).split()


def makefile_builds(unit):
    """Does the Makefile compile <unit>.hip with $(HIPFLAGS) and $(HDRS) as a prerequisite, and link its object?  The unit is in UNITS,
    the one pattern rule over UNITS has the prerequisite and the flags, OBJS is derived from UNITS and the library is linked from OBJS."""
    text = open(os.path.join(CSRC, "Makefile")).read()
    rule = re.search(r"^\$\(foreach u,\$\(UNITS\),\$\(HERE\)\$\(u\)\$\(SFX\)\.o\): \$\(HERE\)%\$\(SFX\)\.o: \$\(HERE\)%\.hip(.*)\n"
                     r"\t\$\(HIPCC\) \$\(HIPFLAGS\) \$\(UNITFLAGS\) -c \$< -o \$@$", text, re.M)
    objs = re.search(r"^OBJS\s*:=\s*\$\(foreach u,\$\(UNITS\) \$\(HOST\),\$\(HERE\)\$\(u\)\$\(SFX\)\.o\)$", text, re.M)
    link = re.search(r"^\$\(OUT\): \$\(OBJS\)\n\t\$\(HIPCC\) .*-shared.* \$\^", text, re.M)
    return unit in makefile_units() and rule is not None and "$(HDRS)" in rule.group(1) and objs is not None and link is not None


def only_unit_including(header, unit):
    """<unit> includes <header>, and no other file of csrc does (a non-template __global__ function is defined in exactly one unit)"""
    inc = '#include "%s"' % header
    holders = [f for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".h", ".hpp", ".inc", ".cpp")) and inc in open(os.path.join(CSRC, f)).read()]
    return holders == [unit]


def scene_bytes_holds_no_part_of(header):
    """scene_bytes.hip, the unit the measure pass and the label edits came out of, pastes no .inc onto its end and does not include <header>"""
    scene = open(os.path.join(CSRC, "scene_bytes.hip")).read()
    return re.search(r'#include\s+"[^"]*\.inc"', scene) is None and '#include "%s"' % header not in scene


_COMPILED = {}


def compile_unit(name, extra_flags=()):
    """remarks(...) of volym_amd/csrc/<name>.hip, compiled device-only with the Makefile's flags (and extra_flags) and
    -Rpass-analysis=kernel-resource-usage.  Cached per process: a unit is compiled once however many test files ask."""
    key = (name, tuple(extra_flags))
    if key not in _COMPILED:
        with tempfile.TemporaryDirectory() as tmp:
            cmd = [HIPCC] + makefile_flags() + list(extra_flags) + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-S",
                                                                    os.path.join(CSRC, name + ".hip"), "-o", os.path.join(tmp, name + ".s")]
            p = subprocess.run(cmd, capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-2000:]
        _COMPILED[key] = remarks(p.stderr)
    return _COMPILED[key]


def write_figures(path, lines):
    """print the figures and keep them in `path`; a read-only checkout still checks the bar"""
    print("\n".join(lines))
    try:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
    except OSError:
        pass


def remarks(stderr):
    """{mangled kernel name: {figure: value}} from the kernel-resource-usage remarks"""
    out = {}
    for blk in stderr.split("Function Name: ")[1:]:
        name = blk.split(" [")[0].strip()
        g = lambda k: int(re.search(k + r": (\d+)", blk).group(1))
        out[name] = {"vgpr": g("VGPRs"), "sgpr": g("SGPRs"), "scratch": g(r"ScratchSize \[bytes/lane\]"), "occ": g(r"Occupancy \[waves/SIMD\]"),
                     "lds": g(r"LDS Size \[bytes/block\]")}
    return out
