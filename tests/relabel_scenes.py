"""The scenes and requests of the relabel tests, shared by tests/test_relabel_host.py (which asserts on the host twin the conditions
the device tests rely on) and tests/test_gpu_relabel.py (which compares the device with the twin).

Scenes A and B are those of tests/measure_scenes.py: 37 x 22 x 19, random density bytes 1..255, five labels in blocks (A) or random
labels over all 256 values (B).  No axis is a multiple of 4 and a row is no multiple of 16, so linear chunks wrap rows and slices.
The ragged scene is tests/test_gpu_crop_box._ragged: 97 x 80 x 71, a shell (1), a core (2) and a blob (5) in air (0).

A Case is a request and the passes it reads: the components request whose ids it takes, the distance request whose map it takes.
`pick` names a piece by what the components pass found in the scene as it stands ("largest": the component with the most texels),
because a piece's number depends on the cuts; resolve() turns it into the ids k..k of the request.
"""
import numpy as np

from tests import measure_scenes as MS
from tests.test_gpu_crop_box import _ragged
from tests.test_gpu_slice import Host

DIMS = MS.DIMS
RAGGED_DIMS = (97, 80, 71)


class Case:
    def __init__(self, name, relabel, components=None, distance=None, pick=None, trivial=False, wraps=False):
        self.name, self.relabel, self.components, self.distance, self.pick, self.trivial = name, relabel, components, distance, pick, trivial
        self.wraps = wraps              # the changed texels share chunks across rows of the linear layout (asserted on the twin)


def scene_a():
    return MS.scene_a()


def scene_b():
    return MS.scene_b()


def scene_ragged():
    dims, vol, labels = _ragged()
    h = Host(dims)
    h.vol, h.labels = vol, labels
    return h


def _select(*labels):
    s = np.zeros(256, np.int64)
    s[list(labels)] = 1
    return s


def cases_a():
    """the requests over scene A: tables alone on the whole volume and on the odd boxes, windows, ids k..k and IDS_EXCEPT, distance
    bands with and without INSIDE, both conditions at once, the identity table, the empty box, the single texel"""
    from volym_amd import _lib, scene
    R, B = scene.Relabel, MS.BOXES
    every = {l: 77 for l in range(5)}
    pieces = scene.Components(B["whole"], 0, 120, _select(3, 4))
    blocks = scene.Components(B["whole"], 0, 1, _select(2))
    outside = scene.Distance(B["whole"], 0, 1, _select(2))
    inside = scene.Distance(B["whole"], _lib.DISTANCE_INSIDE, 1, _select(2), (1, 1, 4))
    part = scene.Distance(B["x 5..30"], 0, 90, _select(1, 4), (1, 4, 1))
    return [
        Case("merge 1, 2 -> 4, whole", R(B["whole"], to={1: 4, 2: 4})),
        Case("swap 0 <-> 3, rows", R(B["rows"], to={0: 3, 3: 0})),
        Case("table, x 3..8", R(B["x 3..8"], to={0: 9, 1: 9, 4: 2})),
        Case("table, x 5..30", R(B["x 5..30"], to={2: 200})),
        Case("window 100..180, whole", R(B["whole"], window=(100, 180), to={l: 7 for l in range(5)})),
        Case("window 1..60 of the uncut bytes, x 5..30", R(B["x 5..30"], _lib.RELABEL_UNCUT, (1, 60), {3: 1, 0: 1})),
        Case("the largest piece of 3 and 4 -> 8", R(B["whole"], _lib.RELABEL_IDS, to={3: 8, 4: 8}), components=pieces, pick="largest"),
        Case("all but the largest piece of 3 and 4 -> 0", R(B["whole"], _lib.RELABEL_IDS | _lib.RELABEL_IDS_EXCEPT, to={3: 0, 4: 0}), components=pieces, pick="largest"),
        Case("pieces 2..40 of 3 -> 6, rows", R(B["rows"], _lib.RELABEL_IDS, to={3: 6}, ids=(2, 40)), components=pieces),
        Case("grow 2 by 2", R(B["whole"], _lib.RELABEL_DISTANCE, to={0: 2, 1: 2, 3: 2, 4: 2}, d2=(0, 4)), distance=outside),
        Case("shrink 2 by 1", R(B["whole"], _lib.RELABEL_DISTANCE, to={2: 0}, d2=(0, 1)), distance=inside),
        Case("the thick core of 2 -> 11", R(B["whole"], _lib.RELABEL_DISTANCE, to={2: 11}, d2=(2, 0xfffffffe)), distance=inside),
        Case("band 1..5 of a map over x 5..30, a box inside it", R(((6, 4, 2), (29, 18, 17)), _lib.RELABEL_DISTANCE, (40, 255), {0: 1, 2: 4, 3: 4}, d2=(1, 5)),
             distance=part),
        Case("the rim of the blocks of 2 but the largest", R(B["x 5..30"], _lib.RELABEL_IDS | _lib.RELABEL_IDS_EXCEPT | _lib.RELABEL_DISTANCE, (30, 255), {2: 12}, d2=(0, 1)),
             components=blocks, distance=inside, pick="largest"),
        Case("pieces 0..9 of 3 within 3 of 2, dry run", R(B["whole"], _lib.RELABEL_IDS | _lib.RELABEL_DISTANCE | _lib.RELABEL_DRY_RUN, to={3: 2}, ids=(0, 9), d2=(0, 9)),
             components=pieces, distance=outside),
        Case("identity", R(B["whole"]), trivial=True),
        Case("identity under a window and ids", R(B["rows"], _lib.RELABEL_IDS, (3, 200), ids=(0, 5)), components=pieces, trivial=True),
        Case("empty box", R(B["empty"], to=every), trivial=True),
        Case("single texel", R(B["texel"], to=every), trivial=True),
    ]


def cases_b():
    """the requests over scene B (every texel breaks a run, every label leaves and arrives)"""
    from volym_amd import _lib, scene
    R, B = scene.Relabel, MS.BOXES
    low = np.zeros(256, np.int64)
    low[:128] = 1
    near = scene.Distance(B["whole"], 0, 200, low)
    pieces = scene.Components(B["rows"], _lib.COMPONENTS_SPLIT_LABELS, 1, low)
    return [
        Case("every label + 1, whole", R(B["whole"], to=(np.arange(256) + 1) % 256)),
        Case("reversed, x 3..8", R(B["x 3..8"], to=255 - np.arange(256))),
        Case("window 50..99, all -> 0, x 5..30", R(B["x 5..30"], window=(50, 99), to=np.zeros(256, np.int64))),
        Case("within 1 of a bright low label: high -> low", R(B["whole"], _lib.RELABEL_DISTANCE, to=np.arange(256) % 128, d2=(1, 1)), distance=near),
        Case("pieces 0..200 (split by label) fold to 16 labels", R(B["rows"], _lib.RELABEL_IDS, to=np.arange(256) % 16, ids=(0, 200)), components=pieces),
    ]


def cases_ragged():
    """the requests over the ragged scene: rows of 97 texels, so a chunk that wraps a row holds texels of both"""
    from volym_amd import _lib, scene
    R = scene.Relabel
    whole = ((0, 0, 0), RAGGED_DIMS)
    mid = ((10, 7, 5), (90, 75, 66))
    slab = ((0, 0, 30), (97, 80, 41))
    core = scene.Distance(mid, 0, 100, _select(2))
    air = scene.Components(slab, 0, 1, _select(0))
    shell = scene.Distance(slab, 0, 100, _select(1))
    return [
        Case("shell -> 7, whole", R(whole, to={1: 7}), wraps=True),
        Case("air and shell -> 3, full rows", R(((0, 3, 2), (97, 77, 69)), to={0: 3, 1: 3}), wraps=True),
        Case("air and shell -> 3, x 40..57", R(((40, 0, 0), (57, 80, 71)), to={0: 3, 1: 3})),
        Case("the darkest air -> 6, whole", R(whole, window=(0, 1), to={0: 6}), wraps=True),
        Case("core, window 198..203", R(mid, window=(198, 203), to={2: 9})),
        Case("the largest piece of air -> 4", R(slab, _lib.RELABEL_IDS, to={0: 4}), components=air, pick="largest", wraps=True),
        Case("every piece of air but the largest -> 4", R(slab, _lib.RELABEL_IDS | _lib.RELABEL_IDS_EXCEPT, to={0: 4}), components=air, pick="largest"),
        Case("air within 60 of the shell -> 1", R(slab, _lib.RELABEL_DISTANCE, to={0: 1}, d2=(1, 3600)), distance=shell, wraps=True),
        Case("grow the core by 3", R(((12, 9, 6), (88, 70, 60)), _lib.RELABEL_DISTANCE, to={0: 2, 1: 2}, d2=(0, 9)), distance=core),
    ]


def snapshots(host, case):
    """the twins' results of the passes `case` reads, in the state `host` is in: {"components": (summary, table, ids) or None,
    "distance": (summary, map) or None}"""
    from volym_amd import scene
    now = scene.cut_volume(host.vol, host.dims, host.cut, host.labels)
    uncut = host.vol if host.ever_cut else None
    comp = dist = None
    if case.components is not None:
        comp = scene.components_volume(now, host.dims, case.components, labels=host.labels, cut=host.cut, uncut=uncut)
    if case.distance is not None:
        dist = scene.distance_volume(now, host.dims, case.distance, labels=host.labels, cut=host.cut, uncut=uncut)
    return {"components": comp, "distance": dist}


def resolve(case, snaps):
    """the request of `case` with its pick turned into ids k..k by the components table of snaps"""
    if case.pick is None:
        return case.relabel
    table = snaps["components"][1]
    assert case.pick == "largest", (case.name, case.pick)
    k = int(np.argmax(table["count"])) if len(table) else 0        # (the first of the largest; under a cut that leaves no piece, no texel has an id)
    return case.relabel.replace(ids=(k, k))


def expect(host, case, snaps=None, relabel=None):
    """the twin's (new_labels [flat], result, request) of `case` in the state `host` is in"""
    from volym_amd import scene
    snaps = snaps or snapshots(host, case)
    r = relabel or resolve(case, snaps)
    now = scene.cut_volume(host.vol, host.dims, host.cut, host.labels)
    comp, dist = snaps["components"], snaps["distance"]
    new, result = scene.relabel_volume(now, host.dims, r, host.labels, ids=None if comp is None else comp[2], ids_box=None if comp is None else case.components.box,
                                       dmap=None if dist is None else dist[1], dmap_box=None if dist is None else case.distance.box, uncut=host.vol)
    return new.ravel(), result, r


def wrapping_chunks(dims, old, new):
    """how many 16-byte chunks of the linear layout hold changed texels of two different rows"""
    nx = dims[0]
    at = np.flatnonzero(np.asarray(old).ravel() != np.asarray(new).ravel())
    chunk, row = at >> 4, at // nx
    order = np.lexsort((row, chunk))
    chunk, row = chunk[order], row[order]
    return int(((chunk[1:] == chunk[:-1]) & (row[1:] != row[:-1])).sum())
