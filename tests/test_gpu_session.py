"""Editing sessions on the device: every label editor, the passes whose snapshots they read, cuts, undo and redo on one context.

The scripts and their host model are those of tests/session_scenes.py, whose conditions (every edit changes texels, every hazard of
the module's list occurs, the journal evicts and gives up where the script says) tests/test_session_host.py asserts on the model.
Everything compared is integer: there is no tolerance anywhere but against the oracle.

After every step: an edit's, undo's or redo's 4128 result bytes against the twin's (a refused undo or redo must come back as E_STATE),
the history's info against scene.LabelHistory's, every label against the model's and the label counts against a bincount; after a
pass, its summary and maps against the twin's, every byte.  At the looks, tests/test_gpu_relabel._look: labels whole and on a sub-box,
measure passes cut and UNCUT against the twin, slices of every z plane and a frame against a reference context that was handed the
model's labels and cuts.  Every script ends with all cuts lifted, a look, and everything undone.

Against the oracle: at the three looks of "ragged" and at the end of "a working day", one frame each in density mode and with
importance rendering (tests/test_gpu_crop_box.PARAMS "base" and "straight") against oracle.render on scene.cut_volume of the model's
volume and of table[labels], at that file's bar (_near: <= 1e-4 per channel on f32, no pixel over it, rgba8 within 1 LSB), three
standing frames bit-equal (_three).

A failure names the script, the step and its description, and VOLYM_SESSION_UPTO=<step> runs the script up to that step alone, e.g.
VOLYM_SESSION_UPTO=17 pytest -m gpu "tests/test_gpu_session.py::test_a_generated_script[0-16]".  More seeds on demand:
VOLYM_EXTRA_SEEDS="1 2 3".
"""
import os

import pytest

from tests import session_scenes as SN
from tests.test_gpu_crop_box import _ctx
from tests.test_gpu_relabel import Reference, _frame_uniforms

pytestmark = pytest.mark.gpu

UPTO = int(os.environ["VOLYM_SESSION_UPTO"]) if os.environ.get("VOLYM_SESSION_UPTO") else None
RUNS = [("a working day", 0), ("a working day", 1), ("give up and go on", 0), ("give up and go on", 1), ("ragged", 0)]


def _session(oracle, script, layout, ctx, ref, in_flight=1, against_oracle=True):
    host = script.host()
    host.upload(ctx)
    return SN.Session(host, bool(layout), ctx, ref, _frame_uniforms(oracle), oracle if against_oracle else None, in_flight,
                      "%s, %s" % (script.name, "bricked" if layout else "linear"))


# ---- 1. the hand-written scripts, both layouts ("ragged": the linear one, whose chunks wrap its rows of 97) ---------------------------
@pytest.mark.parametrize("name,layout", RUNS)
def test_a_script(oracle, volym_lib, name, layout):
    script = SN.scripts()[name]
    steps = script.steps(oracle, bool(layout))
    with _ctx(layout) as ctx, Reference(layout) as ref:
        s = _session(oracle, script, layout, ctx, ref).run(steps, UPTO)
        if UPTO is None:
            s.finish()
            assert sum(t["op"] == "look" and not t["refused"] for t in s.trace) >= 3


# ---- 2. two frames in flight ---------------------------------------------------------------------------------------------------------
def test_a_working_day_with_two_frames_in_flight(oracle, volym_lib):
    """three frames after every edit, undo and redo, so that the slots alternate between them; at the looks the three frames read
    are the reference context's, and the frame read before a pass is the frame read after it"""
    from volym_amd import _lib
    script = SN.scripts()["a working day"]
    steps = script.steps(oracle, False)
    with _ctx(0, [(_lib.OPT_FRAMES_IN_FLIGHT, 2)]) as ctx, Reference(0, reuse=False) as ref:
        s = _session(oracle, script, 0, ctx, ref, in_flight=2, against_oracle=False).run(steps, UPTO)
        if UPTO is None:
            s.finish()


# ---- 3. generated scripts ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SN.SEEDS)
@pytest.mark.parametrize("layout", [0, 1])
def test_a_generated_script(oracle, volym_lib, layout, seed):
    """the cheap checks after every step, a look after every tenth and at the end"""
    script = SN.generated(seed)
    steps = script.steps(oracle, bool(layout))
    with _ctx(layout) as ctx, Reference(layout) as ref:
        s = _session(oracle, script, layout, ctx, ref)
        s.run(steps, UPTO, each=lambda k, step: s.apply(SN.look()) if k % 10 == 9 else None)
        if UPTO is None:
            s.finish()
