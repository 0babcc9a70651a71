"""Numpy reference of the scene render (parc_env_render_scene): every drawn character's primitives in the camera-target frame, FK through
the library's own operators (parc_dof_to_rot / parc_forward_kinematics), cast in float64 with render_ref.py's brute-force terrain and
analytic primitives.  Ties go as the kernel breaks them: terrain first, then (env, kind, geom) in order, a later candidate only when
strictly nearer."""
import numpy as np

import render_ref as RR
from parc_amd import lib as L


def still_frame(env, camera_env, eye, target):
    """World origin of the camera-target frame and the eye in it (STILL: eye / target relative to the camera env's origin)."""
    eo = env._scene.env_offsets[camera_env].astype(np.float64)
    o = eo + np.asarray(target, np.float64)
    return o, np.asarray(eye, np.float64) - np.asarray(target, np.float64)


def terrain(env, o, half_window_m=14.0):
    """render_ref.Terrain of a window around the frame origin, heights relative to it, and the grid size."""
    t = env._scene.grid.terrain
    dx, dy = float(t.dxdy[0]), float(t.dxdy[1])
    gx0, gy0 = float(t.min_point[0]) - o[0] - 0.5 * dx, float(t.min_point[1]) - o[1] - 0.5 * dy
    X, Y = t.hf.shape
    ci, cj = int(-gx0 // dx), int(-gy0 // dy)
    r = int(half_window_m / dx)
    win = (min(max(ci - r, 0), X), min(max(ci + r, 0), X), min(max(cj - r, 0), Y), min(max(cj + r, 0), Y))
    return RR.Terrain(np.asarray(t.hf, np.float64) - o[2], gx0, gy0, dx, dy, window=win), (X, Y)


def undecided_exit(ter, shape, O, D):
    """Distance at which each ray leaves the terrain window through a side that is not the grid's rim (inf: never); beyond the rim
    there is no terrain, so leaving through it decides nothing away."""
    i0, i1, j0, j1 = ter.window
    X, Y = shape
    lo = np.array([ter.gx0 + i0 * ter.dx, ter.gy0 + j0 * ter.dy])
    hi = np.array([ter.gx0 + i1 * ter.dx, ter.gy0 + j1 * ter.dy])
    rim_lo, rim_hi = np.array([i0 == 0, j0 == 0]), np.array([i1 == X, j1 == Y])
    with np.errstate(divide="ignore", invalid="ignore"):
        ta = (lo[None] - O[:, :2]) / D[:, :2]
        tb = (hi[None] - O[:, :2]) / D[:, :2]
    leave = np.where(np.isnan(ta), np.inf, np.maximum(ta, tb))
    rim = np.where(D[:, :2] > 0, rim_hi[None], rim_lo[None])
    ax = leave.argmin(axis=1)
    t = leave[np.arange(len(O)), ax]
    return np.where(rim[np.arange(len(O)), ax], np.inf, t)


def characters(env, o, env_ids, draw_ref=True, ref_offset=(0.0, 0.0, 0.0)):
    """[(key = 2 env + kind, env, [primitive dicts])] in key order, positions relative to the frame origin o (float64)."""
    import torch
    lib, h, st = env._lib, env._handle, env._stream()
    env_ids = sorted({int(e) for e in env_ids})
    n = len(env_ids)
    B = env._kin_char_model.get_num_bodies()
    idx = torch.tensor(env_ids, dtype=torch.long, device=env._device)
    offs = env._scene.env_offsets[env_ids].astype(np.float64)

    def fk(root_world, root_rot, jr):
        rel = torch.tensor(root_world - o[None], dtype=torch.float32, device=env._device).contiguous()
        rr = root_rot.contiguous()
        jr = jr.reshape(n, B - 1, 4).contiguous()
        bp = torch.zeros(n, B, 3, device=env._device); br = torch.zeros(n, B, 4, device=env._device)
        L.check(lib.parc_forward_kinematics(h, rel.data_ptr(), rr.data_ptr(), jr.data_ptr(), bp.data_ptr(), br.data_ptr(), n, st))
        torch.cuda.synchronize()
        return bp.double().cpu().numpy(), br.double().cpu().numpy()

    jr = torch.zeros(n, B - 1, 4, device=env._device)
    dof = env._char_dof_pos[idx].contiguous()
    L.check(lib.parc_dof_to_rot(h, dof.data_ptr(), jr.data_ptr(), n, st))
    kinds = [fk(env._char_root_pos[idx].double().cpu().numpy() + offs, env._char_root_rot[idx], jr)]
    if draw_ref:
        rp = env._ref_root_pos[idx].double().cpu().numpy() + np.asarray(ref_offset, np.float64) + offs
        kinds.append(fk(rp, env._ref_root_rot[idx], env._ref_joint_rot[idx]))
    dp = env._scene.cfg.dynamics
    out = []
    for k, e in enumerate(env_ids):
        for kind, (bp, br) in enumerate(kinds):
            if not np.isfinite(bp[k]).all():
                continue
            prims = []
            for gi in range(dp.num_geoms):
                b, typ = dp.geom_body[gi], dp.geom_type[gi]
                q = br[k, b]
                a = bp[k, b] + RR.quat_rotate(q, np.array(dp.geom_pos[gi], np.float64))
                bb = bp[k, b] + RR.quat_rotate(q, np.array(dp.geom_pos2[gi], np.float64))
                prims.append(dict(type=typ, a=a, b=bb, s=list(dp.geom_size[gi]), q=q, id=(16 if kind == 0 else 32) + b))
            out.append((2 * e + kind, e, prims))
    return out


def cast(ter, chars, O, D):
    """Nearest hit: t, id, env (-1 terrain / sky), normal facing the ray."""
    t, ids, n, _ = ter.hit(O, D)
    env = np.full(len(O), -1, np.int64)
    for _, e, prims in chars:
        for p in prims:
            tp, np_ = RR.prim_hit(p, O, D)
            upd = tp < t
            t[upd] = tp[upd]; ids[upd] = p["id"]; n[upd] = np_[upd]; env[upd] = e
    flip = (n * D).sum(-1) > 0
    n[flip] = -n[flip]
    return t, ids, env, n


def shade_ids(ter, chars, O, D, sun):
    """(depth, id with the shadow bit when sun is given, env map) of rays O + t D."""
    t, ids, env, n = cast(ter, chars, O, D)
    hit = np.isfinite(t)
    out = ids.copy()
    if sun is not None and hit.any():
        sun = np.asarray(sun, np.float64) / np.linalg.norm(sun)
        Os = O[hit] + t[hit, None] * D[hit] + RR.SHADOW_OFFSET * n[hit]
        ts, _, _, _ = cast(ter, chars, Os, np.broadcast_to(sun, Os.shape).copy())
        out[np.nonzero(hit)[0][np.isfinite(ts)]] |= RR.SHADOW_BIT
    return t, out.astype(np.uint8), env


def decided_mask(ter, shape, eye, D, dep_np):
    """Pixels the windowed numpy caster decides: a hit before the ray leaves the window through a non-rim side, a ray that never
    leaves it that way, or one that leaves it above every column top."""
    O = np.broadcast_to(eye, D.shape).copy()
    ex = undecided_exit(ter, shape, O, D)
    hmax = float(np.max(ter.hf))
    rising = (D[:, 2] >= 0) & (eye[2] + np.where(np.isfinite(ex), ex, 0) * D[:, 2] > hmax)
    dec = (np.isfinite(dep_np) & (dep_np <= ex)) | ~np.isfinite(ex) | (~np.isfinite(dep_np) & rising)
    return dec, ex


def compare(ids_hip, dep_hip, env_hip, ids_np, dep_np, env_np, decided, exit_np, what):
    """The bounds of test_render_gpu.py, plus env_map on the pixels where the IDs agree."""
    und = ~decided
    assert (dep_hip[und] >= exit_np[und] - 1e-3).all(), (what, "HIP hit inside the window where numpy saw none")
    agree = (ids_hip == ids_np) & decided
    frac = agree.sum() / max(decided.sum(), 1)
    bad = decided & ~agree
    nb = RR.near_boundary(ids_np)
    assert frac >= 0.995, (what, frac, bad.sum())
    assert not (bad & ~nb).any(), (what, np.argwhere(bad & ~nb)[:10])
    fin = agree & np.isfinite(dep_np)
    assert np.array_equal(np.isfinite(dep_hip[agree]), np.isfinite(dep_np[agree])), what
    err = np.abs(dep_hip[fin] - dep_np[fin])
    assert (err <= 1e-4 * dep_np[fin] + 1e-4).all(), (what, err.max())
    emap_ok = env_hip[agree] == env_np[agree]
    assert emap_ok.all(), (what, "env_map", int((~emap_ok).sum()))
    return frac, int(decided.sum()), float(err.max()) if err.size else 0.0
