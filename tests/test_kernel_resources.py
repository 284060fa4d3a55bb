"""What the compiler made of the march kernels (no GPU: any machine with hipcc).

raymarch_common.hip and raymarch.hip are compiled device-only with the Makefile's own flags, -Rpass-analysis=kernel-resource-usage
and -S, and the listings are checked for what the per-entry reload of the frame parameters (raymarch_device.h, frame_params_here)
is there for:

  * the headline instantiation (raymarch_common.hip) has no scratch, at most 128 VGPRs and four waves per SIMD;
  * its three hot loops -- the classic march, the depth-parallel march, the shading of the queued samples -- hold no v_readlane,
    v_writelane or scratch access;
  * no volym_raymarch_pq_kernel instantiation has more scratch than the build of it at the parent of that change (both listings:
    profiles/param_reload_kernel_resources.txt);
  * the place in the kernel-argument segment that the kernels read FrameParams from is the place the code object's metadata gives
    that argument.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "volym_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
RESOURCES = os.path.join(ROOT, "profiles", "param_reload_kernel_resources.txt")
# the headline instantiation: table mode, uninstrumented, K = 4, flags pinned, linear layout, no importance rendering, 16 waves
HEADLINE = "volym_raymarch_pq_kernelILb1ELb0ELb0ELi4ELb0ELb0ELb0ELi16ELi0ELb0E"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc is not installed")


def makefile_flags():
    """ARCH, CXXFLAGS and COMFLAGS as volym_amd/csrc/Makefile states them (the product build, no DEV)"""
    text = open(os.path.join(CSRC, "Makefile")).read()
    var = lambda name: re.search(r"^%s\s*[:?]?=\s*(.*)$" % name, text, re.M).group(1).split()
    arch = var("ARCH")[0]
    warnings = lambda f: f.startswith("-W")
    return ["--offload-arch=" + arch] + [f for f in var("CXXFLAGS") if not warnings(f)], var("COMFLAGS")


def compile_listing(tmp, unit, extra):
    """-> (the -S listing, the resource-usage remarks) of one unit's device code"""
    flags, _ = makefile_flags()
    out = os.path.join(str(tmp), unit + ".s")
    cmd = [HIPCC] + flags + extra + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-S", os.path.join(CSRC, unit), "-o", out]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    return open(out).read(), p.stderr


@pytest.fixture(scope="module")
def common(tmp_path_factory):
    return compile_listing(tmp_path_factory.mktemp("common"), "raymarch_common.hip", makefile_flags()[1])


@pytest.fixture(scope="module")
def rest(tmp_path_factory):
    return compile_listing(tmp_path_factory.mktemp("rest"), "raymarch.hip", [])


def remarks(stderr):
    """{mangled kernel name: {figure: value}} from the kernel-resource-usage remarks"""
    out = {}
    for blk in stderr.split("Function Name: ")[1:]:
        name = blk.split(" [")[0].strip()
        g = lambda k: int(re.search(k + r": (\d+)", blk).group(1))
        out[name] = {"vgpr": g("VGPRs"), "scratch": g(r"ScratchSize \[bytes/lane\]"), "occ": g(r"Occupancy \[waves/SIMD\]")}
    return out


def kernel_body(listing, needle):
    """instructions of one kernel and the index each label stands in front of, as scripts/isa_loops.py reads a listing"""
    lines = listing.split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith("_ZN") and needle in l.split(":")[0] and ":" in l)
    body, labels = [], {}
    for l in lines[start + 1:]:
        s = l.strip()
        if s.startswith("s_endpgm"):
            body.append(s)
            break
        if not s or s.startswith(";"):
            continue
        m = re.match(r"^(\.LBB\d+_\d+):", s)
        if m:
            labels[m.group(1)] = len(body)
            continue
        if s.startswith("."):
            continue
        body.append(s.split(";")[0].strip())
    return body, labels


def loops(body, labels):
    """(first, last) instruction of every loop: a branch back to a label, as scripts/isa_loops.py finds them"""
    out = []
    for i, ins in enumerate(body):
        m = re.match(r"(s_cbranch\w+|s_branch)\s+(\.LBB\d+_\d+)", ins)
        if m and m.group(2) in labels and labels[m.group(2)] <= i:
            out.append((labels[m.group(2)], i))
    return out


def hot_loops(body, labels):
    """The march loops and the shading loop behind them.  Between the ray set-up of a list entry and the store of its pixels
    nothing is written to global memory, and those three loops are all the heavy code there: the largest loops of at least 80 VALU
    instructions without a global store (the shading loop also sits inside either march loop; the small loops -- the replay of
    empty steps, the waits -- are inside the three or trivial)."""
    cand = []
    for a, b in loops(body, labels):
        seg = body[a:b + 1]
        if any(x.startswith(("global_store", "global_atomic", "flat_store", "buffer_store")) for x in seg):
            continue
        if sum(1 for x in seg if x.startswith("v_")) >= 80:
            cand.append((a, b))
    return sorted(set((a, b) for a, b in cand if not any((c <= a and b <= d) and (c, d) != (a, b) for c, d in cand)))


def kernels_metadata(listing):
    """{mangled name: [(offset, size, value_kind) of every argument]} from the amdhsa.kernels metadata of a listing"""
    meta = listing[listing.index("amdhsa.kernels:"):]
    out = {}
    for blk in re.split(r"\n  - \.agpr_count:", meta)[1:]:
        name = re.search(r"\n    \.name:\s+(\S+)", blk).group(1)
        out[name] = [(int(o), int(s), k) for o, s, k in
                     re.findall(r"- \.offset:\s+(\d+)\n\s+\.size:\s+(\d+)\n\s+\.value_kind:\s+(\w+)", re.sub(r"\n\s+\.(actual_access|address_space|name|is_const):.*", "", blk))]
    return out


def test_headline_instantiation_has_no_scratch(common):
    listing, err = common
    res = {k: v for k, v in remarks(err).items() if HEADLINE in k}
    assert len(res) == 1, list(remarks(err))
    r = next(iter(res.values()))
    print("headline instantiation:", r)
    assert r["scratch"] == 0
    assert r["vgpr"] <= 128
    assert r["occ"] == 4
    body, _ = kernel_body(listing, HEADLINE)
    assert not [x for x in body if x.startswith("scratch_")]


def test_headline_hot_loops_hold_no_spill_code(common):
    listing, _ = common
    body, labels = kernel_body(listing, HEADLINE)
    hot = hot_loops(body, labels)
    for a, b in hot:
        seg = body[a:b + 1]
        print("loop %5d..%5d  valu %4d  salu %4d  mem %3d" % (a, b, sum(x.startswith("v_") for x in seg), sum(x.startswith("s_") for x in seg),
                                                            sum(x.startswith(("global_", "ds_", "buffer_", "flat_", "scratch_")) for x in seg)))
    assert len(hot) == 3, hot        # depth-parallel march, classic march, the shading of what is left in the queue
    # all three fetch voxel bytes (the marches' samples, the shading's six gradient taps) and shade (the LDS atomics of the accumulators)
    assert all(any(x.startswith("global_load_ubyte") for x in body[a:b + 1]) for a, b in hot)
    assert all(sum(x.startswith("ds_add_u32") for x in body[a:b + 1]) >= 3 for a, b in hot)
    for a, b in hot:
        bad = [x for x in body[a:b + 1] if x.startswith(("v_readlane", "v_writelane", "scratch_"))]
        assert not bad, (a, b, bad[:5])


def test_no_instantiation_has_more_scratch_than_its_parent(common, rest):
    # the committed listings: "== parent" and "== change" sections in the format of scripts/kernel_resources.sh; an instantiation is
    # named by its first ten template arguments (the change added an eleventh)
    section, parent = None, {}
    for line in open(RESOURCES):
        if line.startswith("=="):
            section = line.split()[1]
        m = re.match(r"pq_kernel<([^>]*)>.* scratch\s+(\d+)", line)
        if m and section == "parent":
            parent[tuple(a.strip() for a in m.group(1).split(","))[:10]] = int(m.group(2))
    assert len(parent) >= 15, parent
    seen = 0
    for unit in (common, rest):
        for name, r in remarks(unit[1]).items():
            if "volym_raymarch_pq_kernel" not in name:
                continue
            dem = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout
            args = tuple(a.strip() for a in re.search(r"pq_kernel<([^>]*)>", dem).group(1).split(","))[:10]
            args = tuple({"(bool)1": "true", "(bool)0": "false"}.get(a, a) for a in args)
            assert args in parent, (args, "not in profiles/param_reload_kernel_resources.txt: regenerate it")
            print("%-60s scratch %3d (parent %3d)  vgpr %3d" % (", ".join(args), r["scratch"], parent[args], r["vgpr"]))
            assert r["scratch"] <= parent[args], (args, r["scratch"], parent[args])
            seen += 1
    assert seen == len(parent), (seen, len(parent))


def test_frame_params_offset_is_the_code_objects(common, rest):
    checked = 0
    for listing, _ in (common, rest):
        meta = kernels_metadata(listing)
        for name, args in meta.items():
            if "volym_raymarch_pq_kernel" not in name:
                continue
            by_value = [a for a in args if a[2] == "by_value" and a[1] > 256]      # FrameParams: the one large by-value argument
            assert len(by_value) == 1, (name, args)
            lines = listing.split("\n")
            start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
            end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith("s_endpgm"))
            used = [int(m.group(1), 0) for l in lines[start:end] for m in [re.search(r"frame_params_here: kernarg offset (\w+)", l)] if m]
            assert used, name                                                         # every instantiation reloads (RELOAD)
            assert all(u == by_value[0][0] for u in used), (name, used, by_value)
            checked += 1
    assert checked >= 15
