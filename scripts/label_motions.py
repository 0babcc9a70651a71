#!/usr/bin/env python3
"""Contact labelling and penetration lift for raw clips on the GPU: the reference editor's "Automatic Contact Labelling" buttons
(``motionscope/include/contact_editing_gui.py:46-85``) for every ``.pkl`` below a folder, in ONE batched pass.

    python scripts/label_motions.py --inputs DIR --out DIR [--target_fps N] [--ground_height H] [--no_hands] [--no_lift]
        [--keep_existing] [--flat_terrain_dx 0.4 --flat_terrain_padding 5.0] [--config data/configs/motion_label/motion_label_default.yaml]

Every clip is resampled first when ``--target_fps`` is given (``change_motion_fps``), then its feet and hands are labelled on its own
terrain (``compute_hf_foot_contacts_and_correct_pen``, ``compute_motion_terrain_hand_contacts``) and its root is lifted out of the
terrain frame by frame.  With ``--ground_height`` the plane at that height replaces the terrains (``compute_ground_plane_foot_contacts``,
``correct_foot_ground_pen``; the hands are then not labelled).  A clip without a terrain gets the flat one of
``create_terrain_for_motion`` written in (``--flat_terrain_dx``, ``--flat_terrain_padding``) and is labelled on it.  The files keep their
names and their sub-folders below ``--out``; they carry ``body_contacts`` and a terrain, which is what ``preprocess_motions.py``, the
sampler and ``run_tracker.py`` need.  ``misc_data["hf_mask_inds"]`` belongs to the frames before the pass and is not carried over:
``preprocess_motions.py`` recomputes it.  The keys of ``--config`` are the flags' names; a flag given on the command line wins.
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import numpy as np  # noqa: E402

DEFAULTS = dict(char_model="data/assets/humanoid.xml", device="cuda:0", contact_eps=0.04, target_fps=None, ground_height=None,
                no_hands=False, no_lift=False, keep_existing=False, flat_terrain_dx=0.4, flat_terrain_padding=5.0)


def resolve(p):
    return p if os.path.isabs(p) else os.path.join(REPO, p)


def gather(folder):
    out = []
    for root, _, names in sorted(os.walk(folder)):
        out += [os.path.join(root, n) for n in sorted(names) if n.endswith(".pkl")]
    if not out:
        raise ValueError(f"{folder}: no .pkl files")
    return out


def read_clip(path, num_bodies, flat_dx, flat_padding):
    """(OptClip, misc dict or None).  Missing contacts are zeros; a missing terrain is the flat one around the clip."""
    from parc_amd import ms_file
    from parc_amd.motion_label import flat_terrain_for
    from parc_amd.motion_opt import OptClip
    try:
        d = ms_file.load_ms_file(path, load_misc=True)
    except ms_file.UnsafePickleError:
        d = ms_file.load_ms_file(path, load_misc=False)
    m, t = d.motion_data, d.terrain_data
    if m is None:
        raise ValueError(f"{path}: no motion data")
    rp = np.asarray(m.root_pos, np.float32)
    ct = np.zeros((rp.shape[0], num_bodies), np.float32) if m.body_contacts is None else np.asarray(m.body_contacts, np.float32)
    if t is None:
        hf, mn, dx = flat_terrain_for(rp, flat_dx, flat_padding)
        maxmin = None
    else:
        hf, mn, dx = np.asarray(t.hf, np.float32), np.asarray(t.min_point, np.float32), float(t.dx)
        maxmin = None if t.hf_maxmin is None else np.asarray(t.hf_maxmin, np.float32)
    misc = dict(d.misc_data) if isinstance(d.misc_data, dict) else None
    if misc is not None:
        misc.pop("hf_mask_inds", None)
    clip = OptClip(rp, np.asarray(m.root_rot, np.float32), np.asarray(m.joint_rot, np.float32), ct, hf, mn, dx, m.fps,
                   os.path.basename(os.path.splitext(path)[0]), hf_maxmin=maxmin)
    return clip, (misc or None), str(m.loop_mode)


def write_clip(path, clip, misc, loop_mode):
    from parc_amd import ms_file
    fps = clip.fps if float(clip.fps) != int(clip.fps) else int(clip.fps)
    md = ms_file.MSMotionData(root_pos=clip.root_pos, root_rot=clip.root_rot, joint_rot=clip.joint_rot, body_contacts=clip.contacts,
                              fps=fps, loop_mode=loop_mode)
    maxmin = clip.hf_maxmin
    if maxmin is None:   # SubTerrain's defaults (max 1, min -1 in every cell)
        maxmin = np.stack([np.ones_like(clip.hf), -np.ones_like(clip.hf)], -1)
    td = ms_file.MSTerrainData(hf=clip.hf, hf_maxmin=maxmin, min_point=clip.min_point, dx=float(clip.dx))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    ms_file.save_ms_file(ms_file.MSFileData(motion_data=md, terrain_data=td, misc_data=misc), path)


def run(inputs, out, cfg, labeller=None, log=print):
    """One batched pass over every ``.pkl`` below ``inputs``; returns the written paths.  ``labeller``: a ``ContactLabeller`` to reuse."""
    from parc_amd.motion_label import ContactLabeller
    files = gather(inputs)
    h = labeller or ContactLabeller(resolve(cfg["char_model"]), cfg["device"], float(cfg["contact_eps"]))
    read = [read_clip(f, h.B, float(cfg["flat_terrain_dx"]), float(cfg["flat_terrain_padding"])) for f in files]
    clips = [r[0] for r in read]
    if cfg["target_fps"] is not None:
        clips = h.resample(clips, cfg["target_fps"])
    r = h.run(clips, hands=not cfg["no_hands"], correct_pen=not cfg["no_lift"], ground_height=cfg["ground_height"],
              keep_existing=bool(cfg["keep_existing"]))
    off, written = r["packed"]["frame_off"], []
    for i, (f, c) in enumerate(zip(files, clips)):
        sl = slice(int(off[i]), int(off[i + 1]))
        c.root_pos, c.contacts = r["root_pos"][sl].copy(), r["contacts"][sl].copy()
        path = os.path.join(out, os.path.relpath(f, inputs))
        write_clip(path, c, read[i][1], read[i][2])
        written.append(path)
        lift = r["lift"][sl]
        log(f"{path}: {c.num_frames} frames at {c.fps} fps, {int((lift > 0).sum())} lifted (up to {float(lift.max()):.4f} m), "
            f"foot contacts {r['contacts'][sl][:, h.foot_ids].sum(0).astype(int).tolist()}, "
            f"hand contacts {r['contacts'][sl][:, h.hand_ids].sum(0).astype(int).tolist()}")
    log("kernel ms: " + ", ".join(f"{k} {v:.3f}" for k, v in h.kernel_times().items()))
    return written


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--inputs", required=True, help="folder: every .pkl below it")
    ap.add_argument("--out", required=True, help="output folder")
    ap.add_argument("--config", default=None, help="YAML with the keys of data/configs/motion_label/motion_label_default.yaml")
    ap.add_argument("--target_fps", type=float, default=None, help="resample every clip first (change_motion_fps)")
    ap.add_argument("--ground_height", type=float, default=None, help="label against the plane at this height instead of the terrains")
    ap.add_argument("--no_hands", action="store_true", default=None, help="leave the hand columns alone")
    ap.add_argument("--no_lift", action="store_true", default=None, help="label only; the root height stays")
    ap.add_argument("--keep_existing", action="store_true", default=None, help="unlabelled columns keep the clip's contacts instead of 0")
    ap.add_argument("--flat_terrain_dx", type=float, default=None, help="cell size of the terrain made for a clip without one (0.4)")
    ap.add_argument("--flat_terrain_padding", type=float, default=None, help="metres around the root's path (5.0)")
    ap.add_argument("--contact_eps", type=float, default=None, help="metres (0.04)")
    ap.add_argument("--char_model", default=None)
    ap.add_argument("--device", default=None)
    args = ap.parse_args(argv)
    cfg = dict(DEFAULTS)
    if args.config:
        from parc_amd.util import path_loader
        loaded = path_loader.load_config(resolve(args.config))
        unknown = sorted(set(loaded) - set(DEFAULTS))
        if unknown:
            raise ValueError(f"{args.config}: unknown keys {unknown}")
        cfg.update(loaded)
    cfg.update({k: v for k, v in vars(args).items() if k in DEFAULTS and v is not None})
    if cfg["target_fps"] is not None and not cfg["target_fps"] > 0:
        raise ValueError(f"target_fps must be > 0, got {cfg['target_fps']}")
    run(args.inputs, args.out, cfg)


if __name__ == "__main__":
    main()
