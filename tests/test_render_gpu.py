"""Renderer on the device (parc_env_render / HipParkourEnv.render) against the numpy reference ray-caster of render_ref.py, on the golden scene.

Bounds (HIP fp32 against numpy float64, the same scene): IDs agree on >= 99.5 % of the pixels the numpy caster decides, every disagreeing
pixel lies within 1 px of an ID boundary of the numpy image (a ray that grazes an edge or a shadow boundary may fall to either side
under fp32 rounding), and where IDs agree the depths agree within 1e-4 relative + 1e-4 m."""
import math
import os

import numpy as np
import pytest

import render_ref as RR
from parc_amd import lib as L

pytestmark = pytest.mark.gpu

W, H = 96, 72
CAM = {"mode": "track", "offset": (0.0, -3.0, 2.5), "fov_y": math.radians(50.0)}
ENVS = [0, 5, 17, 40]
WINDOW_M = 14.0


def _golden_stepped(tmp_path, num_envs=64, env_offsets=None, shift=None):
    import torch
    from gpu_helpers import default_config, write_motion_yaml, inject, golden, GOLDEN_WEIGHTS
    from parc_amd.envs.hip_parkour_env import HipParkourEnv
    g = golden("env_step")
    cfg = default_config()
    cfg["env"]["dm"]["motion_file"] = write_motion_yaml(tmp_path, [str(c) for c in g["clips"]], GOLDEN_WEIGHTS)
    cfg["env"]["hip"]["body_pos_from_fk"] = False
    env = HipParkourEnv(cfg, num_envs, "cuda:0", False, env_offsets=env_offsets)
    inject(env, g, "s0_in_")
    if shift is not None:   # the same world placement from other env origins
        s = torch.tensor(shift, dtype=torch.float32, device="cuda:0")
        env._char_root_pos -= s
        env._char_rigid_body_pos -= s
    env.step(None)
    torch.cuda.synchronize()
    return env


def _numpy_scene(env, e, cam=CAM, draw_ref=True):
    """Terrain window and camera-relative primitives of env e (FK through the library's own operators)."""
    import torch
    lib, h, st = env._lib, env._handle, env._stream()
    t = env._scene.grid.terrain
    root = env._char_root_pos[e].double().cpu().numpy()
    o = root + env._scene.env_offsets[e].astype(np.float64)
    dx, dy = float(t.dxdy[0]), float(t.dxdy[1])
    gx0, gy0 = float(t.min_point[0]) - o[0] - 0.5 * dx, float(t.min_point[1]) - o[1] - 0.5 * dy
    X, Y = t.hf.shape
    ci, cj = int(-gx0 // dx), int(-gy0 // dy)
    r = int(WINDOW_M / dx)
    win = (max(ci - r, 0), min(ci + r, X), max(cj - r, 0), min(cj + r, Y))
    ter = RR.Terrain(np.asarray(t.hf, np.float64) - o[2], gx0, gy0, dx, dy, window=win)
    B = env._kin_char_model.get_num_bodies()

    def fk(root_rel, root_rot, jr):
        rp = torch.tensor(root_rel, dtype=torch.float32, device="cuda:0").reshape(1, 3)
        rr = root_rot.reshape(1, 4).contiguous()
        jr = jr.reshape(1, B - 1, 4).contiguous()
        bp = torch.zeros(1, B, 3, device="cuda:0"); br = torch.zeros(1, B, 4, device="cuda:0")
        L.check(lib.parc_forward_kinematics(h, rp.data_ptr(), rr.data_ptr(), jr.data_ptr(), bp.data_ptr(), br.data_ptr(), 1, st))
        torch.cuda.synchronize()
        return bp[0].double().cpu().numpy(), br[0].double().cpu().numpy()

    jr = torch.zeros(1, B - 1, 4, device="cuda:0")
    dof = env._char_dof_pos[e:e + 1].contiguous()
    L.check(lib.parc_dof_to_rot(h, dof.data_ptr(), jr.data_ptr(), 1, st))
    chars = [(16, fk(np.zeros(3), env._char_root_rot[e], jr))]
    if draw_ref:
        ref_rel = env._ref_root_pos[e].double().cpu().numpy() + np.asarray(env._ref_char_offset) - root
        chars.append((32, fk(ref_rel, env._ref_root_rot[e], env._ref_joint_rot[e])))
    dp = env._scene.cfg.dynamics
    prims = []
    for base, (bp, br) in chars:
        for gi in range(dp.num_geoms):
            b, typ = dp.geom_body[gi], dp.geom_type[gi]
            q = br[b]
            a = bp[b] + RR.quat_rotate(q, np.array(dp.geom_pos[gi], np.float64))
            bb = bp[b] + RR.quat_rotate(q, np.array(dp.geom_pos2[gi], np.float64))
            prims.append(dict(type=typ, a=a, b=bb, s=list(dp.geom_size[gi]), q=q, id=base + b))
    return ter, prims, np.asarray(cam["offset"], np.float64)


def _compare(ids_hip, dep_hip, ids_np, dep_np, exit_np, what, z_exit_above=None):
    # decided: the numpy hit lies inside the window, or the ray never leaves it, or it leaves it rising above every column top
    decided = (np.isfinite(dep_np) & (dep_np <= exit_np)) | ~np.isfinite(exit_np)
    if z_exit_above is not None:
        decided |= ~np.isfinite(dep_np) & z_exit_above
    # rays the numpy window cannot decide: HIP must not have found anything nearer than the window's edge
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
    return frac, int(decided.sum()), float(err.max()) if err.size else 0.0


def test_render_matches_numpy_raycaster(tmp_path):
    import torch
    env = _golden_stepped(tmp_path)
    rgba, dep, idm = env.render(ENVS, W, H, camera=CAM, draw_ref=True, shadows=True, depth=True, ids=True)
    torch.cuda.synchronize()
    assert rgba.shape == (len(ENVS), H, W, 4) and rgba.dtype == torch.uint8 and (rgba[..., 3] == 255).all()
    dep, idm = dep.cpu().numpy(), idm.cpu().numpy()
    sun = np.array(env.render_params().sun_dir, np.float64)
    seen = set()
    for k, e in enumerate(ENVS):
        ter, prims, eye = _numpy_scene(env, e)
        d_np, id_np, ex_np = RR.render(ter, prims, eye, np.zeros(3), W, H, CAM["fov_y"], sun=sun)
        D = RR.camera_rays(eye, np.zeros(3), W, H, CAM["fov_y"])
        hmax = float(np.max(ter.hf))
        rising = (D[..., 2] >= 0) & (eye[2] + np.where(np.isfinite(ex_np), ex_np, 0) * D[..., 2] > hmax)
        frac, n, err = _compare(idm[k], dep[k], id_np, d_np, ex_np, f"env {e}", rising)
        print("env %d: IDs agree on %.4f of %d pixels, max depth error %.2e m" % (e, frac, n, err))
        seen |= set(np.unique(id_np & 0x7F).tolist())
    # the scene shows terrain tops and walls, both characters, and shadows
    assert {1, 2} <= seen and any(16 <= s < 32 for s in seen) and any(s >= 32 for s in seen)
    assert (idm & 0x80).any()


def test_far_env_origins_render_the_same_ids(tmp_path):
    import torch
    near = _golden_stepped(tmp_path)
    off = near._scene.env_offsets.astype(np.float32) + np.array([1000.0, 1000.0, 0.0], np.float32)
    far = _golden_stepped(tmp_path, env_offsets=off, shift=(1000.0, 1000.0, 0.0))
    a = near.render(ENVS, W, H, camera=CAM, depth=True, ids=True)
    b = far.render(ENVS, W, H, camera=CAM, depth=True, ids=True)
    torch.cuda.synchronize()
    ia, ib = a[2].cpu().numpy(), b[2].cpu().numpy()
    for k, e in enumerate(ENVS):
        agree = ia[k] == ib[k]
        assert agree.mean() >= 0.995, (e, agree.mean())
        assert not (~agree & ~RR.near_boundary(ia[k])).any(), e
        print("far origins, env %d: IDs agree on %.4f of the pixels" % (e, agree.mean()))


def _bufs(env):
    return [env._obs_buf, env._reward_buf, env._done_buf, env._char_root_pos, env._char_root_rot, env._char_dof_pos, env._char_dof_vel,
            env._char_contact_forces, env._timestep_buf, env._motion_ids]


def test_render_does_not_change_the_step(tmp_path):
    import torch
    from parc_amd.envs.hip_parkour_env import HipParkourEnv
    from parc_amd.util.path_loader import load_config
    cfg_file = os.path.join(os.path.dirname(__file__), "..", "data", "configs", "tracker_config", "dm_env_default.yaml")
    envs = [HipParkourEnv(load_config(cfg_file), 128, "cuda:0", False, seed=7, enable_dynamics=True) for _ in range(2)]
    for en in envs:
        en.reset()
    torch.manual_seed(0)
    for it in range(6):
        act = envs[0]._char_dof_pos + 0.05 * torch.randn_like(envs[0]._char_dof_pos)
        for n, en in enumerate(envs):
            if it < 3:
                en.step(act.clone())
                en.reset_done()
            else:
                en.step_and_reset_done(act.clone())
            if n == 0:   # render between the steps of one env only
                en.render([0, 3, 127], 64, 48, depth=True, ids=True)
                en.render(None, 16, 16, camera={"mode": "still", "debug_visuals": True}, shadows=False)
        torch.cuda.synchronize()
        for x, y in zip(_bufs(envs[0]), _bufs(envs[1])):
            assert torch.equal(x, y), it


def test_debug_visuals_tint_contacts_red(tmp_path):
    import torch
    env = _golden_stepped(tmp_path)
    e = ENVS[0]
    _, _, idm = env.render([e], W, H, camera=CAM, depth=True, ids=True)
    ids = idm[0].cpu().numpy()
    ids = np.where(ids & 0x80, 0, ids)   # bodies by their lit pixels
    sim = [int(v) - 16 for v, c in zip(*np.unique(ids[(ids >= 16) & (ids < 32)], return_counts=True)) if c >= 10]
    ref = [int(v) - 32 for v, c in zip(*np.unique(ids[ids >= 32], return_counts=True)) if c >= 10]
    assert len(sim) >= 2 and len(ref) >= 2
    env._char_contact_forces[e].zero_()
    env._char_contact_forces[e, sim[0]] = torch.tensor([0.0, 0.0, 5.0], device="cuda:0")
    env._ref_contacts[e].zero_()
    env._ref_contacts[e, ref[0]] = 1.0
    rgba, _, idm = env.render([e], W, H, camera=dict(CAM, debug_visuals=True), depth=True, ids=True)
    img, ids = rgba[0].int().cpu().numpy(), idm[0].cpu().numpy()

    def mean_col(i):
        m = ids == i   # lit pixels of that body only (no shadow bit)
        assert m.sum() >= 3, i
        return img[m][:, :3].mean(axis=0)
    r = mean_col(16 + sim[0]); assert r[0] > r[1] + 40 and r[0] > r[2] + 40, r          # white -> red by |F|
    w = mean_col(16 + sim[1]); assert abs(w[0] - w[1]) < 8 and abs(w[0] - w[2]) < 8, w  # no force: white (grey when shaded)
    r = mean_col(32 + ref[0]); assert r[0] > r[1] + 40 and r[0] > r[2] + 40, r          # green -> red by the target contact
    g = mean_col(32 + ref[1]); assert g[1] > g[0] + 40, g


def test_render_argument_validation(tmp_path):
    from gpu_helpers import default_config
    from parc_amd.envs.hip_parkour_env import HipParkourEnv
    env = _golden_stepped(tmp_path)
    with pytest.raises(L.ParcError, match="k must be"):
        env.render(list(range(64)) + [0], 32, 32)
    with pytest.raises(L.ParcError, match="width and height"):
        env.render([0], 4097, 32)
    with pytest.raises(L.ParcError, match="width and height"):
        env.render([0], 32, 4)
    env2 = HipParkourEnv(default_config(), 8, "cuda:0", False, mirror_ref_state=False)
    env2.reset()
    with pytest.raises(L.ParcError, match="ref_\\* mirrors"):
        env2.render([0], 32, 32, draw_ref=True)
    assert env2.render([0], 32, 32, draw_ref=False).shape == (1, 32, 32, 4)


def test_visualize_writes_png_frames(tmp_path):
    import torch
    from gpu_helpers import default_config
    from parc_amd.envs.hip_parkour_env import HipParkourEnv
    from parc_amd.util.frame_writer import FrameWriter
    env = HipParkourEnv(default_config(), 16, "cuda:0", True)
    fw = FrameWriter(str(tmp_path / "frames"))
    env.set_frame_sink(fw, every=2, size=(48, 32))
    env.camera_env_id = 3
    env.reset()
    for _ in range(2):
        env.step(None)
    fw.close()
    files = sorted(os.listdir(tmp_path / "frames"))
    assert files == ["frame_000000.png", "frame_000001.png"] and fw.dropped == 0     # calls 1 and 3 of 3
    ref = env.render([3], 48, 32)[0].cpu().numpy()
    import struct, zlib
    data = open(tmp_path / "frames" / files[-1], "rb").read()
    w, h = struct.unpack(">II", data[16:24])
    assert (w, h) == (48, 32)
    i = data.index(b"IDAT")
    (n,) = struct.unpack(">I", data[i - 4:i])
    raw = np.frombuffer(zlib.decompress(data[i + 4:i + 4 + n]), np.uint8).reshape(32, 1 + 48 * 4)[:, 1:].reshape(32, 48, 4)
    assert np.array_equal(raw, ref)   # the last frame is the state after the second step
    with pytest.raises(ValueError):
        env.camera_env_id = 16
