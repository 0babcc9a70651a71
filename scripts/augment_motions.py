#!/usr/bin/env python3
"""Motion-terrain augmenter driver: ``num_new_motions`` variations of the clips of ``motions_yaml_path`` in ONE batched run.

    python scripts/augment_motions.py --config data/configs/motion_aug/motion_aug_default.yaml [--no_opt] [--mirror] [--seed N]

Semantics of PARC's ``run_simple_augment_motions.py``: per new motion a source clip (length-weighted), a window of at most
``max_motion_len`` seconds, a random heading and x / y stretch, the terrain padded, sliced around the motion and re-anchored at frame 0,
then ``terrain_aug_type`` (``HEIGHT_SCALE``, ``BOXES_ALONG_PATH`` or ``NONE``); the variations then go through ``num_iters`` iterations
of the kinematic optimiser (body constraints off, as the reference passes ``w_body_constraints=0``) and are written as
``<source>_aug###.pkl`` (loop mode CLAMP, numbered per source from 1).  ``--no_opt`` writes the un-optimised variations; ``--mirror``
additionally writes ``flipped/<name>_flipped.pkl``, the mirrored copy of every written clip.
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import numpy as np  # noqa: E402

from parc_amd import motion_aug as ma  # noqa: E402
from parc_amd import motion_opt as mo  # noqa: E402

REQUIRED = ("motions_yaml_path", "output_folder_path", "char_model", "num_new_motions")


def resolve(p):
    return p if os.path.isabs(p) else os.path.join(REPO, p)


def write_clip(path, clip: mo.OptClip):
    from parc_amd import ms_file
    md = ms_file.MSMotionData(root_pos=clip.root_pos, root_rot=clip.root_rot, joint_rot=clip.joint_rot, body_contacts=clip.contacts,
                              fps=int(clip.fps), loop_mode="CLAMP")
    maxmin = clip.hf_maxmin
    if maxmin is None:   # a clip built in memory: SubTerrain's defaults (max 1, min -1 in every cell)
        maxmin = np.stack([np.ones_like(clip.hf), -np.ones_like(clip.hf)], -1)
    td = ms_file.MSTerrainData(hf=clip.hf, hf_maxmin=maxmin, min_point=np.asarray(clip.min_point, np.float32), dx=float(clip.dx))
    ms_file.save_ms_file(ms_file.MSFileData(motion_data=md, terrain_data=td, misc_data=None), path)


def run(cfg, no_opt=False, mirror=False, seed=0):
    from parc_amd.motion_lib import fetch_motion_files
    missing = [k for k in REQUIRED if k not in cfg]
    if missing:
        raise ValueError(f"missing keys {missing}")
    settings = ma.MotionAugSettings.from_config(cfg)
    device, char_file = cfg.get("device", "cuda:0"), resolve(cfg["char_model"])
    files, _ = fetch_motion_files(resolve(cfg["motions_yaml_path"]))
    aug = ma.MotionAugmenter(char_file, [mo.clip_from_ms(f) for f in files], settings, device)
    clips = aug.augment(int(cfg["num_new_motions"]), seed).to_opt_clips()
    if not no_opt:
        opt_cfg = dict(cfg, w_body_constraints=0.0)
        frames, _ = mo.MotionOptimizer(char_file, device, opt_cfg).optimize(clips, int(cfg.get("num_iters", 3000)), int(cfg.get("log_every", 0)))
        clips = [mo.OptClip(fr["root_pos"], fr["root_rot"], fr["joint_rot"], fr["contacts"], c.hf, c.min_point, c.dx, c.fps, c.name, hf_maxmin=c.hf_maxmin)
                 for c, fr in zip(clips, frames)]
    out_dir = resolve(cfg["output_folder_path"])
    os.makedirs(out_dir, exist_ok=True)
    paths = []
    for c in clips:
        paths.append(os.path.join(out_dir, c.name + ".pkl"))
        write_clip(paths[-1], c)
    if mirror:
        os.makedirs(os.path.join(out_dir, "flipped"), exist_ok=True)
        for c in ma.mirror_clips(clips, char_file, device):
            paths.append(os.path.join(out_dir, "flipped", c.name + ".pkl"))
            write_clip(paths[-1], c)
    print(f"wrote {len(paths)} files to {out_dir}")
    return paths


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--config", required=True)
    ap.add_argument("--no_opt", action="store_true", help="write the variations without the kinematic optimiser")
    ap.add_argument("--mirror", action="store_true", help="also write flipped/<name>_flipped.pkl, the mirrored copy of every clip")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)
    return run(ma.load_config(args.config), args.no_opt, args.mirror, args.seed)


if __name__ == "__main__":
    main()
