"""The pick rule, restated on the test side (a helper, not a test; TEST INFRASTRUCTURE, NOT PRODUCT CODE).

This is the loop of oracle/oracle_np.py::render, built from that module's own helpers (_sample_volume, _smoothed, _ahead_straight,
_ahead_cone, _sample_tf, _shade, wgsl_pow), with two differences: it marches an arbitrary list of pixels (gx, gy) of the W x H
frame, so that large frames can be sampled by rows, and while it marches it records, per ray, the pick for a given alpha_min:

    a composited sample is an iteration that reaches wgsl:313; the pick is the first composited sample after whose compositing
    alpha >= alpha_min (alpha chain: w = (1 - alpha) * a; alpha += w, f32, in that order).

Every ray still runs to its end, so the frame and the five fetch counters come out as a by-product; tests/test_pick_reference.py
pins them to the C oracle, which pins this loop to the shader without touching the oracle.  Nothing of volym_amd is imported.
"""
import numpy as np

from oracle import oracle_np as N

F = N.F
ZERO, ONE = N.ZERO, N.ONE

# include/volym_hip.h struct volym_pick, field for field (written out here: the product's dtype is what the tests check)
RECORD = np.dtype([("t", "<f4"), ("x", "<u2"), ("y", "<u2"), ("z", "<u2"), ("label", "u1"), ("density", "u1"), ("status", "u1"),
                   ("alpha8", "u1"), ("has_labels", "u1"), ("reserved", "u1")])
NEAR = 1e-6        # a composited sample with |alpha - alpha_min| <= NEAR makes its ray's pick a matter of the last bit


def _unorm8(a):
    q = np.nan_to_num(np.asarray(a, F), nan=0.0)
    return np.where(q >= ONE, 255, np.where(q > ZERO, np.floor(q * F(255.0) + F(0.5)), 0)).astype(np.uint8)


def march(volume, importances, dims, lut, cam, par, W, H, gx, gy, alpha_min, filter=0, labels=None):
    """March the rays of the pixels (gx[i], gy[i]).  -> dict with
         picks     RECORD[n]: the pick of every ray for alpha_min
         near      bool[n]: some composited sample of the ray has |alpha - alpha_min| <= NEAR (never for alpha_min == 0: alpha >= 0 holds
                   for every sample)
         f32, u8   [n, 4]: the pixels, as oracle_np.render computes them
         counters  the five fetch counters of these rays
         hit, d, eye, t_entry   the rays themselves (hit: the ray meets the cube)"""
    s = N._Scene()
    s.vol = np.ascontiguousarray(volume, np.uint8).ravel()
    s.imp = np.ascontiguousarray(importances, np.uint8).ravel()
    s.dims = tuple(int(d) for d in dims)
    nx, ny, nz = s.dims
    lab = None if labels is None else np.ascontiguousarray(labels, np.uint8).ravel()
    s.lut = np.ascontiguousarray(lut, np.uint8).reshape(-1, 4)
    s.tf_n = s.lut.shape[0]
    s.filter = int(filter)
    s.par = par
    s.n_vol = s.n_imp = 0
    s.eye = np.array(list(cam.camera_position), F)
    offs = np.arange(-2, 3).astype(F) * F(0.005)
    sigma = F(1.5)
    s.gauss_w = N.wgsl_exp(-(offs * offs) / (F(2.0) * sigma * sigma))
    ivp = np.array(cam.inverse_view_proj, F)                   # [col][row]
    thr = F(par.density_threshold)
    base = F(par.raymarching_step_size)
    min_step = base * F(0.25)
    a_min = F(alpha_min)

    gx = np.asarray(gx).ravel().astype(F)
    gy = np.asarray(gy).ravel().astype(F)
    n = gx.size
    ndx = (gx / F(W)) * F(2.0) - ONE                          # wgsl:221-229
    ndy = ONE - (gy / F(H)) * F(2.0)
    wp = [((ivp[0][r] * ndx + ivp[1][r] * ndy) + ivp[2][r] * ZERO) + ivp[3][r] * ONE for r in range(4)]
    with np.errstate(divide="ignore", invalid="ignore"):
        dx, dy, dz = N._normalize(wp[0] / wp[3] - s.eye[0], wp[1] / wp[3] - s.eye[1], wp[2] / wp[3] - s.eye[2])
        t1 = [(ZERO - s.eye[i]) / d for i, d in enumerate((dx, dy, dz))]   # wgsl:162-179
        t2 = [(ONE - s.eye[i]) / d for i, d in enumerate((dx, dy, dz))]
    tmin = [np.fmin(a, b) for a, b in zip(t1, t2)]
    tmax = [np.fmax(a, b) for a, b in zip(t1, t2)]
    t_entry = np.fmax(np.fmax(np.fmax(tmin[0], tmin[1]), tmin[2]), ZERO)
    t_exit = np.fmax(np.fmin(np.fmin(tmax[0], tmax[1]), tmax[2]), ZERO)
    with np.errstate(invalid="ignore"):
        miss = t_exit <= t_entry

    acc = np.zeros((n, 3), F)
    acc_a = np.where(miss, ONE, ZERO).astype(F)                # wgsl:238-241
    t = t_entry.astype(F).copy()
    cur = np.full(n, base, F)
    active = ~miss
    counters = {"n_hit": int(active.sum()), "n_steps": 0, "n_dense": 0}

    picks = np.zeros(n, RECORD)
    picks["t"] = F(-1.0)
    picks["status"] = np.where(miss, 0, 1)
    picks["has_labels"] = 0 if lab is None else 1
    picked = np.zeros(n, bool)
    pick_alpha = np.zeros(n, F)
    near = np.zeros(n, bool)

    def record(k_i, px, py, pz):
        """the rays k_i have just composited the sample at (px, py, pz), t[k_i]"""
        if float(a_min) != 0.0:
            near[k_i] |= np.abs(acc_a[k_i].astype(np.float64) - float(a_min)) <= NEAR
        new = ~picked[k_i] & (acc_a[k_i] >= a_min)
        if not new.any():
            return
        r = k_i[new]
        ix, iy, iz = N._texel_nearest(px[new], nx), N._texel_nearest(py[new], ny), N._texel_nearest(pz[new], nz)
        o = ix + nx * (iy + ny * iz)
        picked[r] = True
        pick_alpha[r] = acc_a[r]
        picks["t"][r] = t[r]
        picks["x"][r], picks["y"][r], picks["z"][r] = ix, iy, iz
        picks["density"][r] = s.vol[o]
        picks["label"][r] = 0 if lab is None else lab[o]
        picks["status"][r] = 2

    while True:
        with np.errstate(invalid="ignore"):
            active &= (t < t_exit) & (acc_a < F(0.95))         # wgsl:250
        idx = np.flatnonzero(active)
        if idx.size == 0:
            break
        counters["n_steps"] += int(idx.size)
        ti = t[idx]
        px, py, pz = s.eye[0] + dx[idx] * ti, s.eye[1] + dy[idx] * ti, s.eye[2] + dz[idx] * ti
        if par.use_gaussian_smoothing == 1:
            rho = N._smoothed(s, px, py, pz, dx[idx], dy[idx], dz[idx])
        else:
            rho = N._sample_volume(s, px, py, pz)
        imp = N._sample_importance(s, px, py, pz)              # wgsl:260
        with np.errstate(invalid="ignore"):
            dense = rho >= thr
        cur[idx] = np.where(dense, min_step, np.fmin(base, cur[idx] * F(1.5)))   # wgsl:263-269
        nd = idx[~dense]
        t[nd] = t[nd] + cur[nd]                                 # wgsl:271-274
        if not dense.any():
            continue
        d_i = idx[dense]
        counters["n_dense"] += int(d_i.size)
        px, py, pz, rho, imp = px[dense], py[dense], pz[dense], rho[dense], imp[dense]
        use_alpha = par.use_opacity == 1
        keep = np.ones(d_i.size, bool)
        if par.use_importance_coloring == 1:                   # wgsl:83-92, 279-281
            ca = np.stack([np.fmin(imp * F(1.5), ONE), (ONE - imp) * F(1.2), np.full_like(imp, F(0.2)), imp], 1)
            use_alpha = True
        else:
            if par.use_importance_rendering == 1:              # wgsl:283-295
                fn = N._ahead_cone if par.use_cone_importance_check == 1 else N._ahead_straight
                ahead = fn(s, px, py, pz, dx[d_i], dy[d_i], dz[d_i], t_exit[d_i])
                keep = ~((imp < ONE) & ahead)
                sk = d_i[~keep]
                t[sk] = t[sk] + cur[sk]
            ca = N._sample_tf(s, rho)                           # wgsl:297-303
        if not keep.any():
            continue
        k_i = d_i[keep]
        r, g, b = N._shade(s, px[keep], py[keep], pz[keep], ca[keep, 0], ca[keep, 1], ca[keep, 2])
        if use_alpha:                                           # wgsl:313-318
            alpha = ONE - N.wgsl_pow(ONE - ca[keep, 3], cur[k_i] * F(100.0))
            w = (ONE - acc_a[k_i]) * alpha
            acc[k_i, 0] = acc[k_i, 0] + r * w
            acc[k_i, 1] = acc[k_i, 1] + g * w
            acc[k_i, 2] = acc[k_i, 2] + b * w
            acc_a[k_i] = acc_a[k_i] + w
            record(k_i, px[keep], py[keep], pz[keep])
            t[k_i] = t[k_i] + cur[k_i]                          # wgsl:325
        else:                                                   # wgsl:319-323
            acc[k_i, 0], acc[k_i, 1], acc[k_i, 2] = r, g, b
            acc_a[k_i] = ONE
            record(k_i, px[keep], py[keep], pz[keep])
            active[k_i] = False

    f32 = np.concatenate([acc, acc_a[:, None]], 1).astype(F)
    u8 = _unorm8(f32)
    picks["alpha8"] = np.where(miss, 255, _unorm8(np.where(picked, pick_alpha, acc_a)))
    counters["n_vol"], counters["n_imp"] = s.n_vol, s.n_imp
    return {"picks": picks, "near": near, "f32": f32, "u8": u8, "counters": counters,
            "hit": ~miss, "d": np.stack([dx, dy, dz], 1), "eye": s.eye, "t_entry": t_entry.astype(F)}


def shade_at(volume, dims, lut, cam, filter, eye, d, t):
    """wgsl:297-311 at the positions eye + d * t: the TF colour of the density there, shaded (first-hit mode stores exactly this)"""
    s = N._Scene()
    s.vol = np.ascontiguousarray(volume, np.uint8).ravel()
    s.dims = tuple(int(v) for v in dims)
    s.lut = np.ascontiguousarray(lut, np.uint8).reshape(-1, 4)
    s.tf_n = s.lut.shape[0]
    s.filter = int(filter)
    s.n_vol = s.n_imp = 0
    s.eye = np.array(list(cam.camera_position), F)
    t = np.asarray(t, F)
    px, py, pz = eye[0] + d[:, 0] * t, eye[1] + d[:, 1] * t, eye[2] + d[:, 2] * t
    ca = N._sample_tf(s, N._sample_volume(s, px, py, pz))
    return np.stack(N._shade(s, px, py, pz, ca[:, 0], ca[:, 1], ca[:, 2]), 1)


def frame(volume, importances, dims, lut, cam, par, W, H, alpha_min, filter=0, labels=None, rows=None):
    """march() over whole rows of the frame (all of them, or the list `rows`): every array reshaped to (len(rows), W, ...)"""
    rows = np.arange(H) if rows is None else np.asarray(rows)
    gy, gx = np.meshgrid(rows, np.arange(W), indexing="ij")
    out = march(volume, importances, dims, lut, cam, par, W, H, gx.ravel(), gy.ravel(), alpha_min, filter, labels)
    for k in ("picks", "near", "hit", "t_entry"):
        out[k] = out[k].reshape(rows.size, W)
    for k in ("f32", "u8"):
        out[k] = out[k].reshape(rows.size, W, 4)
    return out
