"""Scene render on the device (parc_env_render_scene / HipParkourEnv.render_scene): every env's characters in one image, checked against the
numpy caster of scene_ref.py with the bounds of test_render_gpu.py (IDs on >= 99.5 % of the decided pixels, disagreements only within 1 px
of an ID boundary, depth within 1e-4 relative + 1e-4 m), and env_map where the IDs agree."""
import math
import os
import struct
import zlib

import numpy as np
import pytest

import render_ref as RR
import scene_ref as SR
from parc_amd import lib as L

pytestmark = pytest.mark.gpu

W, H = 96, 72
FOV = math.radians(50.0)
SUN = np.array([0.35, -0.45, 0.82]) / np.linalg.norm([0.35, -0.45, 0.82])


def _golden_env(tmp_path, num_envs=64, env_offsets=None, clips=None, weights=None, shift=None):
    import torch
    from gpu_helpers import default_config, write_motion_yaml, inject, golden, GOLDEN_WEIGHTS
    from parc_amd.envs.hip_parkour_env import HipParkourEnv
    g = golden("env_step")
    cfg = default_config()
    cfg["env"]["dm"]["motion_file"] = write_motion_yaml(tmp_path, clips or [str(c) for c in g["clips"]], weights or GOLDEN_WEIGHTS)
    cfg["env"]["hip"]["body_pos_from_fk"] = False
    env = HipParkourEnv(cfg, num_envs, "cuda:0", False, env_offsets=env_offsets)
    if num_envs == 64 and clips is None:
        inject(env, g, "s0_in_")
        if shift is not None:
            s = torch.tensor(shift, dtype=torch.float32, device="cuda:0")
            env._char_root_pos -= s
            env._char_rigid_body_pos -= s
        env.step(None)
    else:
        env.reset()
    torch.cuda.synchronize()
    return env


def _ground(env, x, y):
    t = env._scene.grid.terrain
    X, Y = t.hf.shape
    i = min(max(int(round((x - float(t.min_point[0])) / float(t.dxdy[0]))), 0), X - 1)
    j = min(max(int(round((y - float(t.min_point[1])) / float(t.dxdy[1]))), 0), Y - 1)
    return float(t.hf[i, j])


def _place(env, e, world, ref_shift=(0.6, 0.0, 0.0)):
    """Put env e's simulated character at `world` and its reference character beside it."""
    import torch
    eo = env._scene.env_offsets[e].astype(np.float64)
    p = torch.tensor(np.asarray(world, np.float64) - eo, dtype=torch.float32, device="cuda:0")
    env._char_root_pos[e] = p
    env._ref_root_pos[e] = p + torch.tensor(ref_shift, dtype=torch.float32, device="cuda:0")


def _rim_scene(tmp_path):
    """64 golden envs; 8 of them placed near the +x rim of the grid around T, seen by a still camera of env 0."""
    env = _golden_env(tmp_path)
    t = env._scene.grid.terrain
    x_rim = float(t.min_point[0]) + (t.hf.shape[0] - 0.5) * float(t.dxdy[0])
    T = np.array([x_rim - 2.0, 0.0, 0.0])
    T[2] = _ground(env, T[0], T[1])
    spots = {1: (0.0, 0.0), 2: (0.5, 1.6), 3: (3.2, 0.8), 4: (-1.8, 1.0), 5: (-0.8, 3.5), 6: (1.2, -1.5), 7: (-3.0, 2.5)}
    for e, (dx, dy) in spots.items():
        x, y = T[0] + dx, T[1] + dy
        _place(env, e, (x, y, (_ground(env, x, y) if x < x_rim else T[2]) + 1.0))
    P = T + np.array([-1.5, -0.8, 0.0])
    _place(env, 8, P + 8.0 * SUN + np.array([0.0, 0.0, 1.0]))        # high above P: out of view, its shadow falls near P
    eo0 = env._scene.env_offsets[0].astype(np.float64)
    cam = {"mode": "still", "eye": tuple(T + [-1.5, -7.0, 3.5] - eo0), "target": tuple(T + [0.5, 1.0, 0.3] - eo0), "fov_y": FOV}
    return env, cam


def _numpy(env, cam, camera_env, env_ids, draw_ref, shadows):
    o, eye = SR.still_frame(env, camera_env, cam["eye"], cam["target"])
    ter, shape = SR.terrain(env, o)
    chars = SR.characters(env, o, env_ids, draw_ref, env._ref_char_offset)
    D = RR.camera_rays(eye, np.zeros(3), W, H, FOV).reshape(-1, 3)
    O = np.broadcast_to(eye, D.shape).copy()
    dep, ids, emap = SR.shade_ids(ter, chars, O, D, SUN if shadows else None)
    dec, ex = SR.decided_mask(ter, shape, eye, D, dep)
    r = lambda a: a.reshape(H, W)
    return r(dep), r(ids), r(emap), r(dec), r(ex)


@pytest.mark.parametrize("draw_ref,shadows", [(True, True), (True, False), (False, True), (False, False)])
def test_scene_matches_numpy_raycaster(tmp_path, draw_ref, shadows):
    import torch
    env, cam = _rim_scene(tmp_path)
    rgba, dep, idm, emap = env.render_scene(0, None, W, H, camera=cam, draw_ref=draw_ref, shadows=shadows, depth=True, ids=True, env_map=True)
    torch.cuda.synchronize()
    assert rgba.shape == (H, W, 4) and emap.shape == (H, W) and emap.dtype == torch.int32
    dep, idm, emap = dep.cpu().numpy(), idm.cpu().numpy(), emap.cpu().numpy()
    d_np, i_np, e_np, dec, ex = _numpy(env, cam, 0, range(64), draw_ref, shadows)
    frac, n, err = SR.compare(idm, dep, emap, i_np, d_np, e_np, dec, ex, (draw_ref, shadows))
    print("draw_ref %d shadows %d: IDs agree on %.4f of %d pixels, max depth error %.2e m" % (draw_ref, shadows, frac, n, err))
    seen = set(np.unique(e_np[dec]).tolist())
    assert 3 in seen and len(seen & {1, 2, 4, 5, 6, 7}) >= 3, seen   # placed characters in view, the one beyond the rim (3) included
    assert 8 not in seen                                       # the caster is out of view ...
    if draw_ref:
        assert ((i_np[dec] & 0x7F) >= 32).any()
    if shadows:                                                # ... and its shadow is in the image
        d2, i2, _, _, _ = _numpy(env, cam, 0, [e for e in range(64) if e != 8], draw_ref, shadows)
        assert ((i2 != i_np) & dec).sum() > 5
        assert (idm & 0x80).any()


def test_single_env_scene_agrees_with_render(tmp_path):
    import torch
    env = _golden_env(tmp_path)
    cam = {"mode": "track", "offset": (0.0, -3.0, 2.5), "fov_y": FOV}
    for c in (0, 17, 40):
        a = env.render([c], W, H, camera=cam, depth=True, ids=True)
        b = env.render_scene(c, [c], W, H, camera=cam, depth=True, ids=True, env_map=True)
        torch.cuda.synchronize()
        ia, ib = a[2][0].cpu().numpy(), b[2].cpu().numpy()
        da, db = a[1][0].cpu().numpy(), b[1].cpu().numpy()
        diff = ia != ib
        assert diff.mean() <= 0.001 and not (diff & ~RR.near_boundary(ia)).any(), (c, diff.sum())
        same = ~diff & np.isfinite(da)
        assert np.array_equal(np.isfinite(da), np.isfinite(db)) or diff.any()
        assert (np.abs(db[same] - da[same]) <= 1e-5 * da[same]).all(), c
        em = b[3].cpu().numpy()
        assert ((em == c) == ((ib & 0x7F) >= 16)).all() and ((em == -1) == ((ib & 0x7F) < 16)).all()
        print("env %d: bit-identical rgba %s, id %s, depth %s" % (c, torch.equal(a[0][0], b[0]), np.array_equal(ia, ib), np.array_equal(da, db)))


def _cast_many(ter, chars, O, D):
    """scene_ref.cast over many characters: the primitives of a character only for the rays that hit its bounding sphere."""
    t, ids, n, _ = ter.hit(O, D)
    env = np.full(len(O), -1, np.int64)
    for _, e, prims in chars:
        c = prims[0]["root"]
        oc = O - c
        b = (oc * D).sum(-1)
        cc = (oc * oc).sum(-1) - prims[0]["R"] ** 2
        m = np.nonzero(b * b - cc >= 0)[0]
        if m.size == 0:
            continue
        for p in prims:
            tp, np_ = RR.prim_hit(p, O[m], D[m])
            upd = tp < t[m]
            k = m[upd]
            t[k] = tp[upd]; ids[k] = p["id"]; n[k] = np_[upd]; env[k] = e
    flip = (n * D).sum(-1) > 0
    n[flip] = -n[flip]
    return t, ids, env, n


def test_many_envs_sampled_pixels(tmp_path):
    import torch
    env = _golden_env(tmp_path, num_envs=16384)
    eo = env._scene.env_offsets.astype(np.float64)
    roots = env._char_root_pos.double().cpu().numpy() + eo
    # a still camera of env 0 looking down at the character with the most others within 6 m
    cand = np.random.default_rng(1).choice(len(roots), 2000, replace=False)
    crowd = [(np.linalg.norm(roots[:, :2] - roots[k, :2], axis=1) < 6.0).sum() for k in cand]
    T = roots[cand[int(np.argmax(crowd))]] - np.array([0.0, 0.0, 1.0])
    cam = {"mode": "still", "eye": tuple(T + [0.0, -6.0, 9.0] - eo[0]), "target": tuple(T - eo[0]), "fov_y": FOV}
    Wb, Hb = 160, 120
    rgba, dep, idm, emap = env.render_scene(0, None, Wb, Hb, camera=cam, depth=True, ids=True, env_map=True)
    torch.cuda.synchronize()
    dep, idm, emap = dep.cpu().numpy(), idm.cpu().numpy(), emap.cpu().numpy()
    o, eye = SR.still_frame(env, 0, cam["eye"], cam["target"])
    near = np.nonzero(np.linalg.norm(roots - o, axis=1) < 40.0)[0]      # characters farther than 40 m cannot reach this view
    chars = SR.characters(env, o, near, True, env._ref_char_offset)
    for _, _, prims in chars:   # bounding sphere about the root per character
        pts = np.array([p["a"] for p in prims] + [p["b"] for p in prims])
        c = pts.mean(0)
        prims[0]["root"] = c
        prims[0]["R"] = float(np.max(np.linalg.norm(pts - c, axis=1))) + max(float(np.linalg.norm(p["s"])) for p in prims) + 1e-3
    ter, shape = SR.terrain(env, o, 20.0)
    rng = np.random.default_rng(0)
    pix = rng.choice(Wb * Hb, 500, replace=False)
    D = RR.camera_rays(eye, np.zeros(3), Wb, Hb, FOV).reshape(-1, 3)[pix]
    O = np.broadcast_to(eye, D.shape).copy()
    t, ids, env_np, nrm = _cast_many(ter, chars, O, D)
    hit = np.isfinite(t)
    Os = O[hit] + t[hit, None] * D[hit] + RR.SHADOW_OFFSET * nrm[hit]
    ts, _, _, _ = _cast_many(ter, chars, Os, np.broadcast_to(SUN, Os.shape).copy())
    ids = ids.copy(); ids[np.nonzero(hit)[0][np.isfinite(ts)]] |= RR.SHADOW_BIT
    dec, ex = SR.decided_mask(ter, shape, eye, D, t)
    ih, dh, eh = idm.reshape(-1)[pix], dep.reshape(-1)[pix], emap.reshape(-1)[pix]
    agree = (ih == ids) & dec
    frac = agree.sum() / max(dec.sum(), 1)
    nb = RR.near_boundary(idm).reshape(-1)[pix]
    assert frac >= 0.995, frac
    assert not (dec & ~agree & ~nb).any()
    # depth on samples off the ID boundaries: a ray that grazes a silhouette turns the fp32 placement of a character 200 m from the
    # world origin into a depth error beyond the bound (seen: 1.2e-3 m at 10.5 m on one such sample)
    fin = agree & np.isfinite(t) & ~nb
    assert (np.abs(dh[fin] - t[fin]) <= 1e-4 * t[fin] + 1e-4).all()
    # env_map: in a crowd, characters of different envs overlap, and the same body of two of them can lie within the depth bound of
    # each other along a ray; fp32 and float64 may then name different envs.  Such a near-tie must stay rare.
    em_ok = eh[agree] == env_np[agree]
    print("env_map agrees on %d of %d samples" % (em_ok.sum(), em_ok.size))
    assert em_ok.mean() >= 0.99
    n_chars = len(set(env_np[dec & (env_np >= 0)].tolist()))
    print("16384 envs: %d of 500 samples decided, IDs agree on %.4f, %d envs' characters sampled" % (dec.sum(), frac, n_chars))
    assert n_chars >= 3


def test_coincident_characters(tmp_path):
    import torch
    n = 4096
    env = _golden_env(tmp_path, num_envs=n, env_offsets=np.zeros((n, 3), np.float32), clips=["sfu"], weights=[1.0])
    for buf in (env._char_root_pos, env._char_root_rot, env._char_dof_pos, env._ref_root_pos, env._ref_root_rot, env._ref_joint_rot):
        buf[:] = buf[0:1].clone()
    cam = {"mode": "track", "offset": (0.0, -3.0, 2.0), "fov_y": FOV}
    one = env.render_scene(0, [0], 64, 48, camera=cam, depth=True, ids=True, env_map=True)
    a = env.render_scene(0, None, 64, 48, camera=cam, depth=True, ids=True, env_map=True)
    b = env.render_scene(0, None, 64, 48, camera=cam, depth=True, ids=True, env_map=True)
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(x, y)                               # identical bytes on the same state
    assert torch.equal(a[0], one[0]) and torch.equal(a[2], one[2]) and torch.equal(a[1], one[1])
    ch = (a[2] & 0x7F) >= 16
    assert ch.sum() > 20 and (a[3][ch] == 0).all() and (a[3][~ch] == -1).all()
    # the smallest env of the list wins, whatever the list's order
    ids = torch.arange(n - 1, 99, -1, device="cuda:0")
    c = env.render_scene(0, ids, 64, 48, camera=cam, depth=True, ids=True, env_map=True)
    assert torch.equal(c[0], one[0]) and (c[3][ch] == 100).all()


def test_robustness_nan_roots_bad_ids_and_arguments(tmp_path):
    import torch
    from gpu_helpers import default_config
    from parc_amd.envs.hip_parkour_env import HipParkourEnv
    env, cam = _rim_scene(tmp_path)
    base = [0, 1, 2, 3, 4, 6, 7]
    ref = env.render_scene(0, base, W, H, camera=cam, depth=True, ids=True, env_map=True)
    env._char_root_pos[5, 0] = float("nan")                  # a hand-off timeout leaves NaN roots
    env._ref_root_pos[5, 1] = float("nan")
    got = env.render_scene(0, base[:3] + [5, 64, -1, 1 << 40] + base[3:], W, H, camera=cam, depth=True, ids=True, env_map=True)
    torch.cuda.synchronize()
    for x, y in zip(ref, got):
        assert torch.equal(x, y)
    one = env.render_scene(0, [1], W, H, camera=cam, ids=True, env_map=True)
    torch.cuda.synchronize()
    assert (one[3] == 1).any() and ((one[3] == 1) | (one[3] == -1)).all()
    with pytest.raises(L.ParcError, match="camera_env"):
        env.render_scene(64, None, 32, 32)
    with pytest.raises(L.ParcError, match="camera_env"):
        env.render_scene(-1, None, 32, 32)
    with pytest.raises(L.ParcError, match="n must be"):
        env.render_scene(0, list(range(64)) + [0], 32, 32)
    with pytest.raises(L.ParcError, match="n must be"):
        env.render_scene(0, [], 32, 32)
    with pytest.raises(L.ParcError, match="width and height"):
        env.render_scene(0, None, 4097, 32)
    env2 = HipParkourEnv(default_config(), 8, "cuda:0", False, mirror_ref_state=False)
    env2.reset()
    with pytest.raises(L.ParcError, match="ref_\\* mirrors"):
        env2.render_scene(0, None, 32, 32, draw_ref=True)
    assert env2.render_scene(0, None, 32, 32, draw_ref=False).shape == (32, 32, 4)


def test_far_env_origins_render_the_same_ids(tmp_path):
    import torch
    near = _golden_env(tmp_path)
    off = near._scene.env_offsets.astype(np.float32) + np.array([1000.0, 1000.0, 0.0], np.float32)
    far = _golden_env(tmp_path, env_offsets=off, shift=(1000.0, 1000.0, 0.0))
    cam = {"mode": "track", "offset": (0.0, -3.0, 2.5), "fov_y": FOV}
    for c in (0, 17):
        a = near.render_scene(c, None, W, H, camera=cam, ids=True, env_map=True)
        b = far.render_scene(c, None, W, H, camera=cam, ids=True, env_map=True)
        torch.cuda.synchronize()
        ia, ib, ea, eb = a[2].cpu().numpy(), b[2].cpu().numpy(), a[3].cpu().numpy(), b[3].cpu().numpy()
        agree = (ia == ib) & (ea == eb)
        assert agree.mean() >= 0.995, (c, agree.mean())
        assert not (~agree & ~RR.near_boundary(ia)).any(), c
        print("far origins, camera env %d: IDs and env_map agree on %.4f of the pixels" % (c, agree.mean()))


def test_render_scene_does_not_change_the_step(tmp_path):
    import torch
    from parc_amd.envs.hip_parkour_env import HipParkourEnv
    from parc_amd.util.path_loader import load_config
    cfg_file = os.path.join(os.path.dirname(__file__), "..", "data", "configs", "tracker_config", "dm_env_default.yaml")
    envs = [HipParkourEnv(load_config(cfg_file), 128, "cuda:0", False, seed=7, enable_dynamics=True) for _ in range(2)]
    for en in envs:
        en.reset()
    torch.manual_seed(0)
    bufs = lambda e: [e._obs_buf, e._reward_buf, e._done_buf, e._char_root_pos, e._char_root_rot, e._char_dof_pos, e._char_dof_vel,
                      e._char_contact_forces, e._timestep_buf, e._motion_ids]
    for it in range(6):
        act = envs[0]._char_dof_pos + 0.05 * torch.randn_like(envs[0]._char_dof_pos)
        for n, en in enumerate(envs):
            if it < 3:
                en.step(act.clone())
                en.reset_done()
            else:
                en.step_and_reset_done(act.clone())
            if n == 0:
                en.render_scene(3, None, 64, 48, depth=True, ids=True, env_map=True)
                en.render_scene(0, [0, 3, 127], 16, 16, camera={"mode": "still", "debug_visuals": True}, shadows=False)
        torch.cuda.synchronize()
        for x, y in zip(bufs(envs[0]), bufs(envs[1])):
            assert torch.equal(x, y), it


def _read_png(path):
    data = open(path, "rb").read()
    w, h = struct.unpack(">II", data[16:24])
    i = data.index(b"IDAT")
    (n,) = struct.unpack(">I", data[i - 4:i])
    return np.frombuffer(zlib.decompress(data[i + 4:i + 4 + n]), np.uint8).reshape(h, 1 + w * 4)[:, 1:].reshape(h, w, 4)


def test_visualize_scene_frames(tmp_path):
    import torch
    from gpu_helpers import default_config
    from parc_amd.envs.hip_parkour_env import HipParkourEnv
    from parc_amd.util.frame_writer import FrameWriter
    env = HipParkourEnv(default_config(), 16, "cuda:0", True)
    fw = FrameWriter(str(tmp_path / "frames"))
    env.set_frame_sink(fw, every=1, size=(64, 48), scene=True)
    env.camera_env_id = 3
    env.reset()
    root3 = env._char_root_pos[3].double().cpu().numpy() + env._scene.env_offsets[3]
    _place(env, 7, root3 + np.array([1.0, 1.5, 0.0]))        # a second character in the camera env's view
    env._visual_update()
    fw.close()
    files = sorted(os.listdir(tmp_path / "frames"))
    assert len(files) == 2 and fw.dropped == 0
    img = _read_png(tmp_path / "frames" / files[-1])
    scene = env.render_scene(None, None, 64, 48).cpu().numpy()
    alone = env.render([3], 64, 48)[0].cpu().numpy()
    _, _, _, emap = env.render_scene(None, None, 64, 48, env_map=True)
    torch.cuda.synchronize()
    assert np.array_equal(img, scene) and not np.array_equal(img, alone)
    assert (emap == 7).any()
