"""The pick calls at the C boundary (no GPU): exported, bound, and the 16-byte record laid out as the header says."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("volym_pick_pass", "volym_read_picks", "volym_pick_device_ptr", "volym_pick")
# struct volym_pick of include/volym_hip.h: (field, offset, size)
LAYOUT = [("t", 0, 4), ("x", 4, 2), ("y", 6, 2), ("z", 8, 2), ("label", 10, 1), ("density", 11, 1), ("status", 12, 1), ("alpha8", 13, 1),
          ("has_labels", 14, 1), ("reserved", 15, 1)]


def test_library_exports_the_four_calls(volym_lib):
    from volym_amd import _lib
    for name in CALLS:
        assert hasattr(volym_lib, name), name
        assert name in _lib.SIGNATURES, name
    assert volym_lib.volym_abi_version() == 2                  # the calls are additions: the ABI version stays


def test_header_declares_them_and_the_record():
    text = open(os.path.join(ROOT, "include", "volym_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in CALLS:
        assert re.search(r"\b%s\s*\(" % name, code), name
    body = re.search(r"struct volym_pick\s*\{(.*?)\}", code, re.S).group(1)
    fields = [f.strip() for decl in body.split(";") if decl.strip() for f in re.sub(r"^\s*\w+\s+", "", decl.strip()).split(",")]
    assert fields == [f for f, _, _ in LAYOUT], fields
    assert "sizeof(struct volym_pick) == 16" in code
    assert re.search(r"#define VOLYM_ABI_VERSION 2\b", code)


def test_record_is_16_bytes_on_both_sides_of_ctypes(tmp_path):
    from volym_amd import _lib
    assert C.sizeof(_lib.Pick) == 16
    for f, off, size in LAYOUT:
        d = getattr(_lib.Pick, f)
        assert (d.offset, d.size) == (off, size), f
    # the C side: the header's own struct through a C compiler
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "volym_hip.h"\nint main(void) {\n  printf("%zu", sizeof(struct volym_pick));\n' +
                   "".join('  printf(" %%zu", offsetof(struct volym_pick, %s));\n' % f for f, _, _ in LAYOUT) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [16] + [off for _, off, _ in LAYOUT], out


def test_pick_dtype_has_the_headers_offsets():
    from volym_amd import _lib
    dt = _lib.PICK_DTYPE
    assert dt.itemsize == 16
    assert list(dt.names) == [f for f, _, _ in LAYOUT]
    for f, off, size in LAYOUT:
        assert dt.fields[f][1] == off and dt.fields[f][0].itemsize == size, f
    assert dt.fields["t"][0] == np.dtype("<f4")
    # a record written through ctypes reads the same through the dtype
    p = _lib.Pick(t=1.5, x=1, y=2, z=3, label=4, density=5, status=2, alpha8=200, has_labels=1, reserved=0)
    r = np.frombuffer(bytes(p), dt)[0]
    assert (float(r["t"]), int(r["x"]), int(r["y"]), int(r["z"]), int(r["label"]), int(r["density"]), int(r["status"]), int(r["alpha8"]),
            int(r["has_labels"])) == (1.5, 1, 2, 3, 4, 5, 2, 200, 1)


def test_python_faces_exist():
    from volym_amd import demo
    for name in ("pick_pass", "read_picks", "pick_device_ptr", "pick"):
        assert callable(getattr(demo.GpuContext, name)), name
    for name in ("pick", "hide_at"):
        assert callable(getattr(demo.Simple, name)), name
