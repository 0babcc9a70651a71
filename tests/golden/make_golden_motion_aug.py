#!/usr/bin/env python3
"""Generate the motion augmenter fixture (``motion_aug.npz``) from the REAL reference.

Run where the reference checkout is available (the tests only read the fixture it writes):

    python tests/golden/make_golden_motion_aug.py [--time PLANS.npz]

Drives the reference's own ``torch_util.rotate_2d_vec`` / ``axis_angle_to_quat`` / ``quat_multiply`` / ``quat_to_exp_map`` /
``exp_map_to_quat``, ``SubTerrain.pad``, ``terrain_util.slice_terrain_around_motion`` and ``add_boxes_to_hf_at_xy_points`` in the order of
``scripts/run_simple_augment_motions.py:144-202``, then ``motion_edit_lib.flip_motion_about_XZ_plane`` and ``SubTerrain.flip_by_XZ_axis``
as ``scripts/parc_2_kin_gen.py:490-495`` does, while ``random.random`` / ``random.randint`` / ``torch.rand`` / ``torch.randint`` /
``torch.multinomial`` are wrapped to record what they return.  The record is turned into a *plan* of derived values with the reference's
own expressions, and the sources, the plans, the reference's outputs and the *unstable* masks of the restatement
(``tests/motion_aug_ref.py``) are written.  Asserted here and written into ``notes``: the restatement reproduces every heightfield (and
``hf_maxmin``) bit for bit outside the mask; frames agree within the tolerances of the restatement's ``compare_variation``; the mask
covers at most 1 % of the fixture's cells; a candidate whose slice bound lies within 1e-3 cell of a rounding tie is dropped and counted;
the restatement's slice shape equals the reference's for every candidate (the ``arange`` ratio is near an integer for all of them, see
``main``).  ``--time PLANS.npz`` only times the reference's functions on the plans that ``tools/bench_motion_aug.py --dump_plans`` wrote
(the CPU baseline recorded in DESIGN.md section 8i) and writes nothing.  The fixture holds data only, no timing.
"""
import contextlib
import io
import json
import os
import random
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

import motion_aug_ref as ref  # noqa: E402
from parc_amd import motion_opt as mo  # noqa: E402
from parc_amd.char_model import CharModel  # noqa: E402

import parc.anim.kin_char_model as kcm  # noqa: E402
import parc.util.motion_edit_lib as medit_lib  # noqa: E402
import parc.util.motion_util as motion_util  # noqa: E402
import parc.util.terrain_util as terrain_util  # noqa: E402
import parc.util.torch_util as torch_util  # noqa: E402

torch.set_num_threads(1)
SEED = 31
PAD = 3
CHAR_FILE = os.path.join(REPO, "data/assets/humanoid.xml")
SETTINGS = dict(terrain_padding_size=PAD, x_scale=[0.8, 1.2], y_scale=[0.8, 1.2], min_h_scale=0.5, max_h_scale=1.5, bad_h_range=[0.9, 1.1],
                min_len=2.0, max_len=6.0, min_angle=0.0, max_angle=6.28318530718, min_num_boxes=1, max_num_boxes=4, min_h=-1.0, max_h=1.0)
# per group: (mode, mirror); per variation of a group: (source, start frame, frame count or None = to the end, (min, max) heading in degrees)
VARIATIONS = [(0, 0, None, (-180.0, 180.0)), (1, 5, 20, (-180.0, 180.0)), (2, 0, None, (0.0, 0.0)), (3, 0, None, (179.9, 179.9)),
              (0, 12, 17, (-179.95, -179.95)), (2, 2, 1, (-180.0, 180.0))]
GROUPS = [(m, mir) for m in ref.MODES for mir in (0, 1)]


def draw_between(lo, hi):
    """One value on [lo, hi] from ``random.random``, scaled as the reference's script scales its draws (u * (hi - lo) + lo, in double)."""
    u = random.random()
    return u * (hi - lo) + lo


@contextlib.contextmanager
def recording(rec):
    """Wrap the generators the script and add_boxes_to_hf_at_xy_points draw from; every returned value goes to ``rec`` in call order."""
    saved = (random.random, random.randint, torch.rand, torch.randint, torch.multinomial)

    def wrap(name, fn, keep):
        def f(*a, **k):
            v = fn(*a, **k)
            rec.append((name, keep(v)))
            return v
        return f

    random.random, random.randint = wrap("random", saved[0], float), wrap("randint", saved[1], int)
    torch.rand, torch.randint = wrap("rand", saved[2], lambda v: v.clone()), wrap("t_randint", saved[3], lambda v: v.clone())
    torch.multinomial = wrap("multinomial", saved[4], lambda v: v.clone())
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            yield
    finally:
        random.random, random.randint, torch.rand, torch.randint, torch.multinomial = saved


def take(rec, name):
    kind, v = rec.pop(0)
    assert kind == name, (kind, name)
    return v


def f32(x):
    return np.float32(x)


# ---- sources ------------------------------------------------------------------------------------------------------------------------
def crop(c, f0, f1, i0, i1, j0, j1):
    dx = f32(c.dx)
    mp = (np.asarray(c.min_point, np.float32) + np.array([i0, j0], np.float32) * dx).astype(np.float32)
    return dict(root_pos=c.root_pos[f0:f1].copy(), root_rot=c.root_rot[f0:f1].copy(), joint_rot=c.joint_rot[f0:f1].copy(),
                contacts=c.contacts[f0:f1].copy(), hf=c.hf[i0:i1, j0:j1].copy(), hf_maxmin=c.hf_maxmin[i0:i1, j0:j1].copy(), min_point=mp, dx=dx)


def synthetic(rng, n, X, Y, start, step, B=15):
    q = rng.standard_normal((n, 4)).astype(np.float32)
    jq = rng.standard_normal((n, B - 1, 4)).astype(np.float32)
    hf = rng.uniform(-0.5, 0.5, (X, Y)).astype(np.float32)
    pos = (np.asarray(start, np.float32) + np.arange(n, dtype=np.float32)[:, None] * np.asarray(step, np.float32)).astype(np.float32)
    return dict(root_pos=pos, root_rot=(q / np.linalg.norm(q, axis=-1, keepdims=True)).astype(np.float32),
                joint_rot=(jq / np.linalg.norm(jq, axis=-1, keepdims=True)).astype(np.float32),
                contacts=(rng.random_sample((n, B)) > 0.5).astype(np.float32), hf=hf,
                hf_maxmin=np.stack([hf + f32(0.3), hf - f32(0.2)], -1).astype(np.float32), min_point=np.array([-0.7, -1.1], np.float32), dx=f32(0.4))


def sources():
    rng = np.random.RandomState(SEED)
    a = mo.clip_from_ms(os.path.join(REPO, "data/motion_terrains/dec2024_teaser_717_1_modified_opt.pkl"))
    b = mo.clip_from_ms(os.path.join(REPO, "data/motion_terrains/civilization.pkl"))
    f0, f1 = 100, 140
    cell = np.rint((b.root_pos[f0:f1, :2] - b.min_point) / b.dx).astype(int)
    i0 = int(np.clip((cell[:, 0].min() + cell[:, 0].max()) // 2 - 12, 0, b.hf.shape[0] - 24))
    j0 = int(np.clip((cell[:, 1].min() + cell[:, 1].max()) // 2 - 12, 0, b.hf.shape[1] - 24))
    walker = synthetic(rng, 10, 6, 6, (0.1, 0.3, 0.9), (0.9, 0.35, 0.01))          # walks off its terrain, past the pad ring
    # hinge joints of the humanoid hold rotations about their axes in real clips; the synthetic ones borrow the bundled clip's joints
    six = synthetic(rng, 6, 5, 7, (0.2, 0.9, 0.8), (0.11, -0.07, 0.02))
    six["joint_rot"], walker["joint_rot"] = a.joint_rot[50:56].copy(), a.joint_rot[60:70].copy()
    return [crop(a, 0, 40, 0, a.hf.shape[0], 0, a.hf.shape[1]), crop(b, f0, f1, i0, i0 + 24, j0, j0 + 24), six, walker], \
        ["dec2024_teaser_717_1_modified_opt[0:40]", f"civilization[{f0}:{f1}] cells [{i0}:{i0 + 24}, {j0}:{j0 + 24}]", "synthetic 6 frames on 5 x 7",
         "synthetic walker off a 6 x 6 terrain"]


def ref_terrain(src):
    hf = torch.tensor(src["hf"], dtype=torch.float32)
    t = terrain_util.SubTerrain(x_dim=hf.shape[0], y_dim=hf.shape[1], dx=float(src["dx"]), dy=float(src["dx"]), min_x=float(src["min_point"][0]),
                                min_y=float(src["min_point"][1]), device="cpu")
    t.hf = hf
    t.hf_maxmin = torch.tensor(src["hf_maxmin"], dtype=torch.float32)
    return t


# ---- one variation through the reference -------------------------------------------------------------------------------------------
def draw_entry(nf, heading_range, mode, mirror, s):
    """A plan entry drawn on the host the way the script draws it: heading (degrees to radians as an fp32 tensor op), the two scales, then
    the mode's values.  The sizes, angles and heights of the boxes are drawn inside the reference's box function and are read from the
    record afterwards (``apply_reference``)."""
    entry = dict(nf=nf, mirror=int(mirror), hscale=f32(1.0), nb=0, box_frame=np.zeros(ref.MAX_BOXES, np.int32), boxes=np.zeros((ref.MAX_BOXES, 4), np.float32))
    degrees = torch.tensor([draw_between(*heading_range)], dtype=torch.float32)
    entry["heading"] = f32((degrees * torch.pi / 180.0)[0].item())
    entry["sx"], entry["sy"] = f32(draw_between(*s["x_scale"])), f32(draw_between(*s["y_scale"]))
    if mode == "HEIGHT_SCALE":
        lo, hi = s["bad_h_range"]
        factor = draw_between(s["min_h_scale"], s["max_h_scale"])
        while lo < factor < hi:                                    # values inside the open bad range are drawn again
            factor = draw_between(s["min_h_scale"], s["max_h_scale"])
        entry["hscale"] = f32(factor)
    elif mode == "BOXES_ALONG_PATH":
        entry["nb"] = random.randint(s["min_num_boxes"], s["max_num_boxes"])
        entry["box_frame"][:entry["nb"]] = torch.randint(0, nf, size=[entry["nb"]], dtype=torch.int64).numpy()
    return entry


def apply_reference(src, start, entry, mode, s, char, fill_boxes=True):
    """(outputs, seconds) of one plan entry through the reference's own functions, called in the order of
    run_simple_augment_motions.py:161-202 and, with the mirror flag, parc_2_kin_gen.py:490-495.  With ``fill_boxes`` the box sizes,
    angles and heights the reference drew are written into ``entry`` with its own scaling expressions."""
    nf = entry["nf"]
    window = slice(start, start + nf)
    pos, quat = torch.tensor(src["root_pos"][window]), torch.tensor(src["root_rot"][window])
    joints, contacts = torch.tensor(src["joint_rot"][window]), torch.tensor(src["contacts"][window])
    terrain = ref_terrain(src)
    heading = torch.tensor([float(entry["heading"])], dtype=torch.float32)
    rec = []
    t0 = time.perf_counter()
    with recording(rec):
        turned_xy = torch_util.rotate_2d_vec(pos[..., 0:2], heading)
        turn = torch_util.axis_angle_to_quat(torch.tensor([0.0, 0.0, 1.0], dtype=torch.float32), heading)
        turned_exp = torch_util.quat_to_exp_map(torch_util.quat_multiply(turn, quat))
        frames = torch.cat([turned_xy, pos[..., 2:3], turned_exp], dim=-1)      # the script's frame layout: xyz, root exp map
        frames[..., 0] *= float(entry["sx"])
        frames[..., 1] *= float(entry["sy"])
        if s["terrain_padding_size"] > 0:
            terrain.pad(padding_size=s["terrain_padding_size"])
        terrain, frames = terrain_util.slice_terrain_around_motion(frames, terrain, padding=terrain.dxdy[0].item() * 2)
        canon_z = float(src["root_pos"][start, 2]) - frames[0, 2].item()
        if mode == "HEIGHT_SCALE":
            terrain.hf = float(entry["hscale"]) * terrain.hf
        elif mode == "BOXES_ALONG_PATH":
            under = torch.tensor(entry["box_frame"][:entry["nb"]], dtype=torch.int64)
            centers = (frames[under, 0:2] - terrain.min_point) / terrain.dxdy
            terrain_util.add_boxes_to_hf_at_xy_points(box_centers=centers, hf=terrain.hf, min_h=s["min_h"], max_h=s["max_h"], min_len=s["min_len"],
                                                      max_len=s["max_len"], min_angle=s["min_angle"], max_angle=s["max_angle"])
        root_pos, root_rot = frames[..., 0:3].clone(), torch_util.exp_map_to_quat(frames[..., 3:6])
        if entry["mirror"]:
            flipped = medit_lib.flip_motion_about_XZ_plane(motion_frames=motion_util.MotionFrames(root_pos=root_pos, root_rot=root_rot, joint_rot=joints,
                                                                                                  contacts=contacts), char_model=char)
            root_pos, root_rot, joints, contacts = flipped.root_pos, flipped.root_rot, flipped.joint_rot, flipped.contacts
            terrain = terrain.torch_copy()
            terrain.flip_by_XZ_axis()
    seconds = time.perf_counter() - t0
    if fill_boxes:
        for b in range(entry["nb"]):                               # add_boxes_to_hf_at_xy_points :944-945, :963 on the recorded uniforms
            sides = take(rec, "rand") * (s["max_len"] - s["min_len"]) + s["min_len"]
            angle = take(rec, "random") * (s["max_angle"] - s["min_angle"]) + s["min_angle"]
            height = take(rec, "random") * (s["max_h"] - s["min_h"]) + s["min_h"]
            entry["boxes"][b] = [sides[0].item(), sides[1].item(), f32(angle), f32(height)]
        assert not rec, f"{len(rec)} recorded draws were not consumed"
    out = dict(root_pos=root_pos.numpy().astype(np.float32), root_rot=root_rot.numpy().astype(np.float32), joint_rot=joints.numpy().astype(np.float32),
               contacts=contacts.numpy().astype(np.float32), hf=terrain.hf.numpy().astype(np.float32).copy(),
               hf_maxmin=terrain.hf_maxmin.numpy().astype(np.float32).copy(), hf_dims=np.array(terrain.hf.shape, np.int32),
               min_point=terrain.min_point.numpy().astype(np.float32).copy(), canon_z=f32(canon_z))
    return out, seconds


def run_reference(src, start, nf, heading_range, mode, mirror, s, char):
    """(plan entry, the reference's outputs) of one freshly drawn variation."""
    entry = draw_entry(nf, heading_range, mode, mirror, s)
    entry["start"] = start
    out, _ = apply_reference(src, start, entry, mode, s, char)
    return entry, out


def time_reference(plans_file, char):
    """The CPU baseline of DESIGN.md section 8i: seconds of the reference's functions, one variation at a time as the reference runs
    them, on the plans that ``tools/bench_motion_aug.py --dump_plans`` wrote (the plans of the GPU measurement: bundled clips, default
    config).  Source, window, heading, scales, height scale, box count and box frames are the plan's; the box sides, angles and heights
    are drawn inside the reference's box function, which takes none (the same work on other values)."""
    from parc_amd import motion_aug as ma
    from parc_amd.motion_lib import fetch_motion_files
    cfg = ma.load_config(os.path.join(REPO, "data/configs/motion_aug/motion_aug_default.yaml"))
    files, _ = fetch_motion_files(os.path.join(REPO, cfg["motions_yaml_path"]))
    clips = [mo.clip_from_ms(f) for f in files]
    srcs = [dict(root_pos=c.root_pos, root_rot=c.root_rot, joint_rot=c.joint_rot, contacts=c.contacts, hf=c.hf, hf_maxmin=c.hf_maxmin,
                 min_point=c.min_point, dx=f32(c.dx)) for c in clips]
    z = np.load(plans_file)
    for mode in ref.MODES:
        plan = {k: z[f"{mode}_{k}"] for k in ref.PLAN_KEYS}
        n = plan["src_clip"].shape[0]
        sec = []
        for v in range(n):
            entry = ref.plan_var(plan, v)
            sec.append(apply_reference(srcs[int(plan["src_clip"][v])], entry["start"], entry, mode, cfg, char, fill_boxes=False)[1])
        sec = np.asarray(sec) * 1e3
        print(f"{mode}: reference CPU, {n} variations one at a time: {sec.sum():.0f} ms in all; per variation median {np.median(sec):.3f} ms "
              f"(min {sec.min():.3f}, p90 {np.percentile(sec, 90):.3f})", flush=True)


def main():
    char = kcm.KinCharModel("cpu")
    char.load_char_file(CHAR_FILE)
    if len(sys.argv) > 2 and sys.argv[1] == "--time":
        return time_reference(sys.argv[2], char)
    model = ref.model_tables(CharModel(CHAR_FILE))
    srcs, src_names = sources()
    torch.manual_seed(SEED); random.seed(SEED); np.random.seed(SEED)
    out, metas = {}, []
    masked = cells = differ_masked = kept = dropped = 0
    count_tie = 1.0
    for k, src in enumerate(srcs):
        for name, a in src.items():
            out[f"src{k}_{name}"] = np.asarray(a, np.float32)
    for g, (mode, mirror) in enumerate(GROUPS):
        plan = {n: [] for n in ("src_clip", "start_frame", "num_frames", "heading", "scale", "mirror", "height_scale", "num_boxes", "box_frame", "boxes")}
        for v, (k, start, nf, heading_range) in enumerate(VARIATIONS):
            src = srcs[k]
            nf = src["root_pos"].shape[0] - start if nf is None else nf
            tries = 0
            while True:
                var, want = run_reference(src, start, nf, heading_range, mode, mirror, SETTINGS, char)
                mine = ref.augment_one(src, var, mode, PAD, True, model)
                # the shape: the slice bounds are grid points, so the arange ratio (max_g + dx - min_g) / dx lies within ~1e-6 of an integer
                # for EVERY variation and a rule that drops those drops all; the count is instead a function of the two rounded cell
                # indices alone (identical fp32 operations on them), asserted here for every candidate, the dropped ones included
                assert tuple(mine["hf_dims"]) == tuple(want["hf_dims"]), (g, v, mine["hf_dims"], want["hf_dims"], mine["info"])
                count_tie = min(count_tie, mine["info"]["count_tie"])
                if mine["info"]["bound_tie"] < ref.BOUND_TIE:
                    dropped += 1
                    tries += 1
                    assert tries < 200, ("no stable candidate", g, v, mine["info"])
                    continue
                break
            kept += 1
            differ_masked += ref.compare_variation(want, mine, f"group {g} variation {v}")
            assert abs(float(want["canon_z"]) - float(mine["canon_z"])) <= 1e-5
            masked += int(mine["unstable"].sum()); cells += mine["unstable"].size
            for name in ("root_pos", "root_rot", "contacts", "hf", "hf_maxmin"):
                out[f"g{g}_v{v}_{name}"] = want[name]
            if mirror:   # without the mirror the joints are the window's, bit for bit (asserted by compare_variation)
                out[f"g{g}_v{v}_joint_rot"] = want["joint_rot"]
            else:
                assert np.array_equal(want["joint_rot"], src["joint_rot"][start:start + nf])
            out[f"g{g}_v{v}_unstable"] = mine["unstable"]
            out[f"g{g}_v{v}_geom"] = np.concatenate([want["min_point"], [want["canon_z"]]]).astype(np.float32)
            for name, val in (("src_clip", k), ("start_frame", start), ("num_frames", nf), ("heading", var["heading"]), ("scale", [var["sx"], var["sy"]]),
                              ("mirror", mirror), ("height_scale", var["hscale"]), ("num_boxes", var["nb"]), ("box_frame", var["box_frame"]),
                              ("boxes", var["boxes"])):
                plan[name].append(val)
        for name, vals in plan.items():
            out[f"g{g}_plan_{name}"] = np.asarray(vals, np.float32 if name in ("heading", "scale", "height_scale", "boxes") else np.int32)
        metas.append(dict(mode=mode, mirror=mirror, variations=len(VARIATIONS)))
    share = masked / cells
    assert share <= ref.MASK_CAP, share
    notes = dict(cells=cells, masked_cells=masked, masked_share=share, cap=ref.MASK_CAP, restatement_differs_in_masked_cells=differ_masked,
                 restatement_differs_outside=0, kept=kept, dropped=dropped, arange_ratio_min_distance_to_integer=count_tie, seed=SEED,
                 sources=src_names)
    np.savez_compressed(os.path.join(HERE, "motion_aug.npz"), groups=json.dumps(metas), settings=json.dumps(SETTINGS), notes=json.dumps(notes), **out)
    print(notes, flush=True)


if __name__ == "__main__":
    main()
