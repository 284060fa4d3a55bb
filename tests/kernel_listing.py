"""What the *_resources tests of the passes share (no test here): where the units are, which compiler, the Makefile's flags and the
reading of the compiler's kernel-resource-usage remarks."""
import os
import re
import shutil

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "volym_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def makefile_flags():
    """ARCH and CXXFLAGS as volym_amd/csrc/Makefile states them (the product build, no DEV), warnings dropped"""
    text = open(os.path.join(CSRC, "Makefile")).read()
    var = lambda name: re.search(r"^%s\s*[:?]?=\s*(.*)$" % name, text, re.M).group(1).split()
    return ["--offload-arch=" + var("ARCH")[0]] + [f for f in var("CXXFLAGS") if not f.startswith("-W")]


def remarks(stderr):
    """{mangled kernel name: {figure: value}} from the kernel-resource-usage remarks"""
    out = {}
    for blk in stderr.split("Function Name: ")[1:]:
        name = blk.split(" [")[0].strip()
        g = lambda k: int(re.search(k + r": (\d+)", blk).group(1))
        out[name] = {"vgpr": g("VGPRs"), "sgpr": g("SGPRs"), "scratch": g(r"ScratchSize \[bytes/lane\]"), "occ": g(r"Occupancy \[waves/SIMD\]"),
                     "lds": g(r"LDS Size \[bytes/block\]")}
    return out
