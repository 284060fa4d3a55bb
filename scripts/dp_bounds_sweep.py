#!/usr/bin/env python3
"""Frame time vs split threshold and floor, per-tile depth bounds on and off, bonsai and teapot 256^3 @ 1920x1080 (development aid).
Needs the DEV build: make -C volym_amd/csrc DEV=1; VOLYM_HIP_LIB=$PWD/volym_amd/libvolym_hip_dev.so python scripts/dp_bounds_sweep.py"""
import os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from volym_amd import _lib, demo, scene, synth
dims = (256,) * 3
W, H = 1920, 1080
SC = {"bonsai": lambda: synth.synth_bonsai(256), "teapot": lambda: synth.synth_teapot()[0]}
for name, gen in SC.items():
    vol = scene.prepare_volume(gen(), dims, True)
    st = scene.State.with_parameters(W / H, scene.StateParameters.benchmark().replace(raymarching_step_size=0.01)); st.update()
    cu, pu = st.camera_uniforms(), st.parameter_uniforms()
    with demo.GpuContext(W, H, 0) as ctx:
        ctx.set_volume(vol, dims, 0)
        ctx.set_importances(np.zeros(256 ** 3, np.uint8), dims)
        ctx.set_transfer_function(scene.default_lut())
        ctx.update(cu, pu); ctx.time_batch(2000)
        for depth in (1, 0):
            ctx.set_option(123, depth)
            for floor in (64, 104):
                ctx.set_option(119, floor)
                res = []
                for v in (-1, -15, -17, -19, -21, -23, -25, 0):
                    ctx.set_option(_lib.OPT_DEPTH_PARALLEL, v); ctx.update(cu, pu)
                    ctx.time_batch(5); ctx.settle(); ctx.time_batch(300)
                    res.append((v, 1e3 * ctx.time_batch(2000) / 2000))
                print(name, "bounds", depth, "floor", floor, " ".join("%d:%.2f" % r for r in res), flush=True)
