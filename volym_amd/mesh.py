"""Mesh files of a segment's surface: binary STL (two triangles per face, the normal taken from the face's direction) and OBJ
(quads over shared vertices).  The mesh is scene.surface_mesh's: the exact boundary of the solid texels, corners at texel corners."""
import struct

import numpy as np

from . import scene

STL_HEADER = b"volym_amd segment surface (binary STL)".ljust(80, b" ")
_STL_TRIANGLE = np.dtype([("normal", "<f4", (3,)), ("v", "<f4", (3, 3)), ("attr", "<u2")])


def write_stl(path, faces, spacing=(1, 1, 1), origin=(0, 0, 0)):
    """Binary STL of a face list (records of _lib.SURFACE_FACE_DTYPE): 84 + 100 * len(faces) bytes.  Face k becomes triangles 2k
    (corners 0, 1, 2 of its quad) and 2k + 1 (corners 0, 2, 3), both with the unit normal of its direction.  Returns the number
    of triangles."""
    vertices, quads = scene.surface_mesh(faces, spacing, origin)
    tri = np.zeros(2 * len(quads), _STL_TRIANGLE)
    tri["normal"] = np.repeat(scene.SURFACE_FACE_NORMALS[np.asarray(faces)["dir"].astype(np.int64)], 2, axis=0)
    if len(quads):
        tri["v"][0::2] = vertices[quads[:, [0, 1, 2]]]
        tri["v"][1::2] = vertices[quads[:, [0, 2, 3]]]
    with open(path, "wb") as f:
        f.write(STL_HEADER)
        f.write(struct.pack("<I", len(tri)))
        f.write(tri.tobytes())
    return len(tri)


def read_stl(path):
    """(normals float32 [n, 3], triangles float32 [n, 3, 3]) of a binary STL."""
    with open(path, "rb") as f:
        data = f.read()
    n = struct.unpack_from("<I", data, 80)[0]
    if len(data) != 84 + 50 * n:
        raise ValueError("%s: %d bytes, but %d triangles need %d" % (path, len(data), n, 84 + 50 * n))
    tri = np.frombuffer(data, _STL_TRIANGLE, n, 84)
    return tri["normal"].copy(), tri["v"].copy()


def write_obj(path, faces, spacing=(1, 1, 1), origin=(0, 0, 0)):
    """OBJ of a face list: one `v` line per shared vertex (repr of the float64: it reads back to the same number), one `f` line
    of four 1-based indices per face.  Returns (vertices, quads) as written."""
    vertices, quads = scene.surface_mesh(faces, spacing, origin)
    with open(path, "w") as f:
        f.write("# volym_amd segment surface: %d vertices, %d quads\n" % (len(vertices), len(quads)))
        f.writelines("v %r %r %r\n" % (float(x), float(y), float(z)) for x, y, z in vertices)
        f.writelines("f %d %d %d %d\n" % tuple(q) for q in (quads + 1).tolist())
    return vertices, quads


def read_obj(path):
    """(vertices float64 [n, 3], quads int64 [m, 4], 0-based) of an OBJ with `v` and four-index `f` lines."""
    v, q = [], []
    with open(path) as f:
        for line in f:
            w = line.split()
            if w[:1] == ["v"]:
                v.append([float(c) for c in w[1:4]])
            elif w[:1] == ["f"]:
                q.append([int(c.split("/")[0]) - 1 for c in w[1:5]])
    return np.array(v, np.float64).reshape(-1, 3), np.array(q, np.int64).reshape(-1, 4)


def write(path, faces, spacing=(1, 1, 1), origin=(0, 0, 0)):
    """write_stl or write_obj by the file name's ending; anything else raises ValueError."""
    low = str(path).lower()
    if low.endswith(".stl"):
        return write_stl(path, faces, spacing, origin)
    if low.endswith(".obj"):
        return write_obj(path, faces, spacing, origin)
    raise ValueError("a mesh file ends in .stl or .obj, got %r" % (path,))
