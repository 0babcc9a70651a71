#!/usr/bin/env python3
"""Generate the contact-labelling fixtures (``motion_label_*.npz``) from the REAL reference.

Run where the reference checkout is available (the tests only read the fixtures it writes):

    python tests/golden/make_golden_motion_label.py

The reference is driven as in ``make_golden_hesitation.py`` (a ``parc`` package alias, empty module stubs, our data-only ms-file
decoder): ``medit_lib.compute_hf_foot_contacts_and_correct_pen``, ``compute_motion_terrain_hand_contacts``,
``compute_ground_plane_foot_contacts``, ``correct_foot_ground_pen`` and ``MotionLib.calc_motion_frame`` themselves run, on the CPU.
The reference works on ``[T, 34]`` frames (root exp map and joint dofs) that it converts to quaternions first; the fixtures hold those
quaternions, so an implementation that takes quaternions sees the reference's own FK input.  ``gap`` and ``hand_sd``, which the
reference's functions compute but do not return, are recomputed with its own helpers (``get_box_points_batch``, ``get_grid_index``,
``points_hf_sdf``) the way the functions call them.

Each ``.npz`` holds inputs, parameters and recorded results only.  ``settled_feet`` / ``settled_hands`` are the decisions that an fp32
implementation must reproduce (``tests/motion_label_ref.py``); at most 2 % of a case's decisions may be unsettled, which is asserted
here.  ``ref_err`` is the largest difference between the reference's fp32 values and the float64 restatement: the tests allow
``max(1e-5, 4 ref_err)``; the resampling cases record the rotations' figure apart (``ref_err_rot``, radians).  A synthetic case that
misses the cap has its ``contact_eps`` moved in steps of 1e-3; the value used is recorded.  The bundled cases also hold what
``create_terrain_for_motion`` makes of the clip (``flat_*``).  The reference's CPU seconds per case are printed.
"""
import os
import sys
import time
import types

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.dont_write_bytecode = True

for _name in ["trimesh", "trimesh.creation", "wandb", "gym", "gym.spaces", "isaacgym", "isaacgym.gymapi", "isaacgym.gymtorch",
              "isaacgym.gymutil"]:
    sys.modules[_name] = types.ModuleType(_name)
sys.modules["wandb"].run = None
sys.modules["trimesh"].creation = sys.modules["trimesh.creation"]
_parc = types.ModuleType("parc")
_parc.__path__ = [os.path.join(REF, "PARC")]
sys.modules["parc"] = _parc

import numpy as np  # noqa: E402
import torch  # noqa: E402

import motion_label_ref as mr  # noqa: E402
from parc_amd import ms_file  # noqa: E402
from parc_amd.char_model import CharModel  # noqa: E402

import parc.anim.kin_char_model as kcm  # noqa: E402
import parc.anim.motion_lib as motion_lib  # noqa: E402
import parc.util.geom_util as geom_util  # noqa: E402
import parc.util.motion_edit_lib as medit_lib  # noqa: E402
import parc.util.motion_util as motion_util  # noqa: E402
import parc.util.terrain_util as terrain_util  # noqa: E402
import parc.util.torch_util as torch_util  # noqa: E402

torch.set_num_threads(8)
CHAR_FILE = os.path.join(REPO, "data/assets/humanoid.xml")
EPS = 0.04
FEET, HANDS = ("left_foot", "right_foot"), ("left_hand", "right_hand")


def load_clip(name):
    d = ms_file.load_ms_file(os.path.join(REPO, "data/motion_terrains", name + ".pkl"), load_misc=False)
    m, t = d.motion_data, d.terrain_data
    return dict(root_pos=np.asarray(m.root_pos, np.float32), root_rot=np.asarray(m.root_rot, np.float32),
                joint_rot=np.asarray(m.joint_rot, np.float32), contacts=np.asarray(m.body_contacts, np.float32),
                hf=np.asarray(t.hf, np.float32), min_point=np.asarray(t.min_point, np.float32), dx=np.float32(t.dx), fps=np.int32(m.fps))


def frames(c, index):
    index = np.asarray(index, np.int64)
    return dict(c, **{k: np.ascontiguousarray(c[k][index]) for k in ("root_pos", "root_rot", "joint_rot", "contacts")})


def moved(c, dxyz):
    out = dict(c)
    out["root_pos"] = (c["root_pos"] + np.asarray(dxyz, np.float32)).astype(np.float32)
    return out


def through_the_frames(char, c):
    """The clip as the reference's [T, 34] frames, and the clip with the quaternions the reference makes of them."""
    rr, jr = torch.tensor(c["root_rot"]), torch.tensor(c["joint_rot"])
    fr = torch.cat([torch.tensor(c["root_pos"]), torch_util.quat_to_exp_map(rr), char.rot_to_dof(jr)], -1)
    root_pos, root_exp, dof = motion_lib.extract_pose_data(fr)
    out = dict(c, root_rot=torch_util.exp_map_to_quat(root_exp).numpy().astype(np.float32),
               joint_rot=char.dof_to_rot(dof).numpy().astype(np.float32))
    return fr, out


def ref_terrain(c):
    hf = torch.tensor(c["hf"])
    t = terrain_util.SubTerrain(x_dim=hf.shape[0], y_dim=hf.shape[1], dx=float(c["dx"]), dy=float(c["dx"]), min_x=float(c["min_point"][0]),
                                min_y=float(c["min_point"][1]), device="cpu")
    t.hf = hf
    assert np.array_equal(t.min_point.numpy(), c["min_point"]) and float(t.dxdy[0]) == float(c["dx"])
    return t


def ref_fk(char, fr):
    root_pos, root_exp, dof = motion_lib.extract_pose_data(fr)
    return char.forward_kinematics(root_pos, torch_util.exp_map_to_quat(root_exp), char.dof_to_rot(dof))


def ref_gap_terrain(char, fr, terrain):
    """min(box_points_z - cell_heights) per foot, as :504-519 computes it."""
    body_pos, body_rot = ref_fk(char, fr)
    T, out = fr.shape[0], []
    for name in FEET:
        b = char.get_body_id(name)
        g = char._geoms[b][0]
        pts = geom_util.get_box_points_batch(body_pos[:, b], body_rot[:, b], g._dims, g._offset)
        inds = terrain.get_grid_index(pts[..., 0:2])
        h = terrain.hf.unsqueeze(0).expand(T, -1, -1)[torch.arange(0, T, 1).unsqueeze(-1), inds[..., 0], inds[..., 1]]
        out.append(torch.min(pts[..., 2] - h, dim=-1)[0])
    return torch.stack(out, -1).numpy()


def ref_gap_ground(char, fr):
    body_pos, body_rot = ref_fk(char, fr)
    out = []
    for name in FEET:
        b = char.get_body_id(name)
        g = char._geoms[b][0]
        out.append(torch.min(geom_util.get_box_points_batch(body_pos[:, b], body_rot[:, b], g._dims, g._offset)[:, :, 2], dim=-1)[0])
    return torch.stack(out, -1).numpy()


def ref_hand_sd(char, fr, terrain):
    body_pos, _ = ref_fk(char, fr)
    out = []
    for name in HANDS:
        b = char.get_body_id(name)
        sd = terrain_util.points_hf_sdf(body_pos[:, b].unsqueeze(0), terrain.hf.unsqueeze(0), terrain.min_point.unsqueeze(0), terrain.dxdy,
                                        base_z=torch.min(terrain.hf).item() - 10.0, inverted=False, radius=char._geoms[b][0]._dims.item())
        out.append(sd[0])
    return torch.stack(out, -1).numpy()


def terrain_case(char, cm, c, eps, nudge):
    """One case on the clip's terrain: the fixture dict, or None when more than 2 % of its decisions are unsettled and eps may move."""
    fr, c = through_the_frames(char, c)
    terrain = ref_terrain(c)
    t0 = time.time()
    new_fr, ct_feet = medit_lib.compute_hf_foot_contacts_and_correct_pen(fr, terrain, char, contact_eps=eps)
    ct_hands = medit_lib.compute_motion_terrain_hand_contacts(fr, terrain, char, contact_eps=eps)
    dt = time.time() - t0
    gap, sd = ref_gap_terrain(char, fr, terrain), ref_hand_sd(char, fr, terrain)
    feet, hands = mr.label_feet(cm, c, eps), mr.label_hands(cm, c, eps)
    lf, rf, lh, rh = (cm.get_body_id(n) for n in FEET + HANDS)
    contacts = (ct_feet + ct_hands).numpy().astype(np.float32)
    unsettled = max(1.0 - feet["settled"].mean(), 1.0 - hands["settled"].mean())
    if unsettled > mr.MAX_UNSETTLED:
        assert nudge, ("unsettled", unsettled)
        return None
    assert np.array_equal(contacts[:, [lf, rf]][feet["settled"]] > 0.5, feet["contact"][feet["settled"]])
    assert np.array_equal(contacts[:, [lh, rh]][hands["settled"]] > 0.5, hands["contact"][hands["settled"]])
    root_z = new_fr[:, 2].numpy().astype(np.float32)
    ok = feet["settled"].all(-1)
    ref_err = max(np.abs(gap - feet["gap"])[feet["settled"]].max(initial=0.0), np.abs(sd - hands["sd"]).max(),
                  np.abs(root_z - (c["root_pos"][:, 2].astype(np.float64) + feet["lift"]))[ok].max(initial=0.0))
    return dict(c, mode=np.int32(0), contact_eps=np.float64(eps), ground_height=np.float64(0.0), ref_contacts=contacts, ref_root_z=root_z,
                ref_gap=gap.astype(np.float32), ref_hand_sd=sd.astype(np.float32), settled_feet=feet["settled"],
                settled_hands=hands["settled"], ref_err=np.float64(ref_err), ref_seconds=np.float64(dt))


def ground_case(char, cm, c, eps):
    fr, c = through_the_frames(char, c)
    assert len(char._geoms[char.get_body_id(FEET[0])]) == 1   # correct_foot_ground_pen walks every geom: here the first is all
    t0 = time.time()
    ct = medit_lib.compute_ground_plane_foot_contacts(fr, char, contact_eps=eps)
    new_fr = medit_lib.correct_foot_ground_pen(fr, char, ground_height=0.0)
    dt = time.time() - t0
    gap = ref_gap_ground(char, fr)
    g = mr.label_ground(cm, c, eps, 0.0)
    lf, rf, lh, rh = (cm.get_body_id(n) for n in FEET + HANDS)
    contacts = ct.numpy().astype(np.float32)
    assert 1.0 - g["settled"].mean() <= mr.MAX_UNSETTLED
    assert np.array_equal(contacts[:, [lf, rf]][g["settled"]] > 0.5, g["contact"][g["settled"]])
    assert not contacts[:, [lh, rh]].any()
    assert 0 < (g["lift"] > 0).sum() < g["lift"].size and 0 < contacts[:, [lf, rf]].sum() < 2 * g["lift"].size   # the feet cross the plane
    root_z = new_fr[:, 2].numpy().astype(np.float32)
    ref_err = max(np.abs(gap - g["gap"]).max(), np.abs(root_z - (c["root_pos"][:, 2].astype(np.float64) + g["lift"])).max())
    T = contacts.shape[0]
    return dict(c, mode=np.int32(1), contact_eps=np.float64(eps), ground_height=np.float64(0.0), ref_contacts=contacts, ref_root_z=root_z,
                ref_gap=gap.astype(np.float32), ref_hand_sd=np.full((T, 2), np.inf, np.float32), settled_feet=g["settled"],
                settled_hands=np.ones((T, 2), bool), ref_err=np.float64(ref_err), ref_seconds=np.float64(dt))


def side_wall(cm, c):
    """``c`` moved in xy and a cell of its terrain raised so that a hand passes within reach of the cell's side: the best of every
    (hand, frame, side) with the hand 2 cm from that side at that frame.  Returns (clip, frames that touch the wall)."""
    pos, _ = mr.fk(cm, c["root_pos"], c["root_rot"], c["joint_rot"])
    dx, best = float(c["dx"]), None
    for hand in HANDS:
        p = pos[:, cm.get_body_id(hand)]
        r = float(cm._geoms[cm.get_body_id(hand)][0].size[0])
        for m in range(p.shape[0]):
            for axis in (0, 1):
                for side in (-1, 1):
                    u = (p[m, axis] - float(c["min_point"][axis])) / dx
                    edge = np.rint(u) + 0.5 * side                       # the boundary of the hand's cell on that side
                    shift = np.zeros(3)
                    shift[axis] = (edge - side * 0.02 / dx - u) * dx       # hand 2 cm inside its own cell
                    q = p + shift
                    cell = [int(np.clip(np.rint((q[m, a] - float(c["min_point"][a])) / dx), 0, c["hf"].shape[a] - 1)) for a in (0, 1)]
                    cell[axis] += side
                    if not (0 <= cell[0] < c["hf"].shape[0] and 0 <= cell[1] < c["hf"].shape[1]):
                        continue
                    hf = c["hf"].copy()
                    hf[cell[0], cell[1]] = np.float32(p[:, 2].max() + 0.5)
                    sd = mr.terrain_sd(q, hf, c["min_point"], dx, r)
                    ix = np.clip(np.rint((q[:, 0] - float(c["min_point"][0])) / dx), 0, hf.shape[0] - 1).astype(int)
                    iy = np.clip(np.rint((q[:, 1] - float(c["min_point"][1])) / dx), 0, hf.shape[1] - 1).astype(int)
                    wall = (sd < EPS) & (hf[ix, iy] < q[:, 2] - 0.5)
                    if best is None or wall.sum() > best[0]:
                        best = (int(wall.sum()), shift, hf, wall)
    n, shift, hf, wall = best
    assert n >= 3, n
    return dict(moved(c, shift), hf=hf), wall


def label_cases(cm):
    clips = {n: load_clip(n) for n in mr.BUNDLED}
    sfu, civ, teaser, dec = (clips[n] for n in mr.BUNDLED)
    out = [("bundled_" + n, "terrain", clips[n], EPS, False) for n in mr.BUNDLED]
    out.append(("edge_t1", "terrain", frames(sfu, [0]), EPS, True))
    out.append(("edge_t65", "terrain", frames(civ, np.arange(65)), EPS, True))
    out.append(("edge_t129", "terrain", frames(civ, np.arange(129)), EPS, True))
    assert dec["hf"].shape == (18, 15)
    out.append(("off_grid", "terrain", moved(dec, (3.0, -2.0, 0.0)), EPS, True))
    wall_clip, wall = side_wall(cm, sfu)
    out.append(("side_wall", "terrain", dict(wall_clip, wall_frames=wall), EPS, True))
    out.append(("deep_pen", "terrain", moved(teaser, (0.0, 0.0, -0.2)), EPS, True))
    out.append(("eps_000", "terrain", teaser, 0.0, True))
    out.append(("eps_100", "terrain", teaser, 0.1, True))
    for name, c in (("sfu", sfu), ("civilization", civ)):   # shifted in z so that the lowest corner is below the plane in half the frames
        low =mr.label_ground(cm, c, EPS, 0.0)["gap"].min(-1)
        out.append(("ground_" + name, "ground", moved(c, (0.0, 0.0, -float(np.median(low)))), EPS, True))
    return out


def resample_case(char, cm, c, target_fps):
    """change_motion_fps' loop around MotionLib.calc_motion_frame, contacts included."""
    mf = motion_util.MotionFrames(root_pos=torch.tensor(c["root_pos"]), root_rot=torch.tensor(c["root_rot"]),
                                  joint_rot=torch.tensor(c["joint_rot"]), contacts=torch.tensor(c["contacts"]))
    fps = int(c["fps"])
    t0 = time.time()
    mlib = motion_lib.MotionLib.from_frames(mf, char, "cpu", motion_lib.LoopMode.CLAMP, fps, contact_info=True)
    length = mlib._motion_lengths[0].item()
    ids = torch.tensor([0], dtype=torch.int64)
    t, times, rows = 0.0, [], []
    while t < length:
        t_th = torch.tensor([t], dtype=torch.float32)
        root_pos, root_rot, _, _, joint_rot, _, contacts = mlib.calc_motion_frame(ids, t_th)
        rows.append((root_pos[0].numpy(), root_rot[0].numpy(), joint_rot[0].numpy(), contacts[0].numpy()))
        times.append(t_th.item())
        t += 1.0 / target_fps
    dt = time.time() - t0
    ref = dict(zip(("root_pos", "root_rot", "joint_rot", "contacts"), (np.stack(x).astype(np.float32) for x in zip(*rows))))
    mine = mr.resample(c, np.asarray(times, np.float32), length)
    ref_err = max(np.abs(ref["root_pos"] - mine["root_pos"]).max(), np.abs(ref["contacts"] - mine["contacts"]).max())
    # apart: where the half angle between two frames is about 1e-3, rounding decides between slerp and its 0.5 / 0.5 fall-back (:496)
    ref_err_rot = max(mr.quat_angle(ref["root_rot"], mine["root_rot"]).max(), mr.quat_angle(ref["joint_rot"], mine["joint_rot"]).max())
    keep = {k: c[k] for k in ("root_pos", "root_rot", "joint_rot", "contacts", "hf", "min_point", "dx", "fps")}
    return dict(keep, target_fps=np.float64(target_fps), times=np.asarray(times, np.float32), length=np.float32(length),
                ref_err=np.float64(ref_err), ref_err_rot=np.float64(ref_err_rot), ref_seconds=np.float64(dt),
                **{"ref_" + k: v for k, v in ref.items()})


def save(name, fx):
    path = os.path.join(HERE, f"motion_label_{name}.npz")
    np.savez_compressed(path, **fx)
    return path


def main():
    char = kcm.KinCharModel("cpu")
    char.load_char_file(CHAR_FILE)
    cm = CharModel(CHAR_FILE)
    cases = label_cases(cm)
    assert tuple(c[0] for c in cases) == mr.LABEL_FIXTURES
    done = {}
    for name, mode, c, eps, nudge in cases:
        extra = {k: c[k] for k in ("wall_frames",) if k in c}
        c = {k: v for k, v in c.items() if k not in extra}
        for k in range(20):
            fx = ground_case(char, cm, c, eps) if mode == "ground" else terrain_case(char, cm, c, eps + 1e-3 * k, nudge)
            if fx is not None:
                break
        assert fx is not None, name
        fx.update(extra)
        if name.startswith("bundled_"):   # create_terrain_for_motion at its defaults and at the bundled terrains' cell size
            flat = [(0.1, 5.0), (0.4, 5.0), (0.4, 1.3)]
            made = [medit_lib.create_terrain_for_motion(motion_util.MotionFrames(root_pos=torch.tensor(fx["root_pos"])), char, None, dx=d, padding=pd)
                    for d, pd in flat]
            fx.update(flat_params=np.asarray(flat, np.float64), flat_dims=np.asarray([list(t.hf.shape) for t in made], np.int64),
                      flat_min_point=np.stack([t.min_point.numpy() for t in made]).astype(np.float32))
            assert all(not t.hf.any() for t in made)
        done[name] = fx
        lf, rf, lh, rh = (cm.get_body_id(n) for n in FEET + HANDS)
        lifted = int((fx["ref_root_z"] != fx["root_pos"][:, 2]).sum())
        path = save(name, fx)
        print(f"wrote {path} {os.path.getsize(path)} bytes; T {fx['root_pos'].shape[0]} hf {fx['hf'].shape} eps {float(fx['contact_eps'])} "
              f"lifted {lifted} max lift {float((fx['ref_root_z'] - fx['root_pos'][:, 2]).max()):.4f} "
              f"foot contacts {int(fx['ref_contacts'][:, [lf, rf]].sum())} hand contacts {fx['ref_contacts'][:, [lh, rh]].sum(0).astype(int).tolist()} "
              f"unsettled feet {int((~fx['settled_feet']).sum())} hands {int((~fx['settled_hands']).sum())} "
              f"min hand margin {float(np.abs(fx['ref_hand_sd'] - fx['contact_eps']).min()):.2e} ref_err {float(fx['ref_err']):.2e} "
              f"reference {float(fx['ref_seconds']):.3f} s")
    # what the cases are there for
    deep = done["deep_pen"]["ref_root_z"] - done["deep_pen"]["root_pos"][:, 2]   # 52 of 58: in the other six both feet are in the air
    assert (deep > 0).mean() > 0.85 and deep.max() > 0.2
    base = done["bundled_TEASER_TERRAIN"]["ref_contacts"]
    assert not np.array_equal(done["eps_000"]["ref_contacts"], base) and not np.array_equal(done["eps_100"]["ref_contacts"], base)
    sw = done["side_wall"]
    hands = sw["ref_hand_sd"] < sw["contact_eps"]
    assert (hands.any(-1) & sw["wall_frames"]).sum() >= 3
    og = done["off_grid"]
    u = (og["root_pos"][:, :2] - og["min_point"]) / og["dx"]
    assert (u[:, 0] > og["hf"].shape[0] - 1).any() or (u[:, 1] < 0).any()

    civ = load_clip("civilization")
    res = [("resample_20", civ, 20), ("resample_45", civ, 45), ("resample_60", civ, 60), ("resample_30", civ, 30),
           ("resample_t2", frames(civ, [10, 11]), 120)]
    assert tuple(r[0] for r in res) == mr.RESAMPLE_FIXTURES
    for name, c, fps in res:
        fx = resample_case(char, cm, c, fps)
        path = save(name, fx)
        print(f"wrote {path} {os.path.getsize(path)} bytes; T {c['root_pos'].shape[0]} -> {fx['times'].size} at {fps} fps "
              f"ref_err {float(fx['ref_err']):.2e} m {float(fx['ref_err_rot']):.2e} rad reference {float(fx['ref_seconds']):.3f} s")


if __name__ == "__main__":
    main()
