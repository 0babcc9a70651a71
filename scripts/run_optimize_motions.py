#!/usr/bin/env python3
"""Kinematic motion optimiser driver: every clip of ``motions_yaml_path`` (one ms file or a dataset YAML) in ONE batched run.

    python scripts/run_optimize_motions.py --config data/configs/motion_opt/motion_opt_default.yaml

Semantics of PARC's ``parc_2_kin_gen.py`` optimisation stage: optional body constraints from the source clip at full rate
(``auto_compute_body_constraints``), the frame stride of ``run_optimize_motions.py`` (constraint ranges ``ceil(s / stride)`` /
``e // stride``, fps ``fps // stride``), then ``num_iters`` Adam iterations.  Writes ``<name>_opt.pkl`` (loop mode CLAMP, the
clip's terrain, constraints in ``misc_data`` as plain arrays) and ``log/log_<name>_opt.txt`` with the loss terms every
``log_every`` iterations.  With ``hf_extras: true`` (or ``--hf_extras``) the files also carry stage 2's
``compute_hf_extra_vals`` of the optimised frames: ``misc_data["hf_mask_inds"]`` and the recomputed ``hf_maxmin`` (default off: the
source bounds are kept).  With ``save_flipped: true`` (or ``--save_flipped``) the mirrored copy of every optimised clip
(``parc_2_kin_gen.py:490-495``) is written beside it as ``flipped/<name>_opt_flipped.pkl``; the copy carries the motion and the terrain only:
``hf_mask_inds`` and the body constraints of ``auto_compute_body_constraints`` (``opt:body_constraints``) are not mirrored into it
(recompute the former with ``scripts/preprocess_motions.py`` on the flipped files).  With ``remove_hesitation: true`` (or
``--remove_hesitation``; default off) the optimised frames of the whole batch first go through ``medit_lib.remove_hesitation_frames``
(``parc_2_kin_gen.py:467-470``; optional keys ``hesitation_val``, ``hesitation_min_seq_len``), so the file, its ``hf_mask_inds`` and the
mirrored copy are those of the shortened clip; the body constraints stay those of the unshortened clip, as in the reference.
"""
import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import numpy as np  # noqa: E402

from parc_amd import motion_opt as mo  # noqa: E402

REQUIRED = ("motions_yaml_path", "output_folder_path", "char_model", "num_iters", "step_size", "max_jerk") + mo.WEIGHT_KEYS


def load_config(path):
    from parc_amd.util import path_loader
    cfg = path_loader.load_config(path)
    if not isinstance(cfg, dict):
        raise ValueError(f"{path}: not a mapping")
    missing = [k for k in REQUIRED if k not in cfg]
    if missing:
        raise ValueError(f"{path}: missing keys {missing}")
    cfg.setdefault("device", "cuda:0")
    cfg.setdefault("frame_stride", 1)
    cfg.setdefault("auto_compute_body_constraints", False)
    cfg.setdefault("log_every", 100)
    cfg.setdefault("hf_extras", False)
    cfg.setdefault("save_flipped", False)
    cfg.setdefault("remove_hesitation", False)
    if int(cfg["frame_stride"]) < 1 or int(cfg["num_iters"]) < 0:
        raise ValueError("frame_stride must be >= 1 and num_iters >= 0")
    return cfg


def resolve(p):
    return p if os.path.isabs(p) else os.path.join(REPO, p)


def write_clip(path, frames, clip: mo.OptClip, constraints: mo.OptClip, hf_extras=None):
    from parc_amd import ms_file
    misc = None
    if len(constraints.cons_body):
        misc = {"opt:body_constraints": {"body": constraints.cons_body.astype(np.int64), "start_frame": constraints.cons_start.astype(np.int64),
                                          "end_frame": constraints.cons_end.astype(np.int64), "point": constraints.cons_point.astype(np.float32)}}
    if hf_extras is not None:   # parc_2_kin_gen.py:472-484: the optimised frames' mask inds and bounds
        misc = dict(misc or {})
        misc["hf_mask_inds"] = [np.ascontiguousarray(a, np.int64) for a in hf_extras["hf_mask_inds"]]
    md = ms_file.MSMotionData(root_pos=frames["root_pos"], root_rot=frames["root_rot"], joint_rot=frames["joint_rot"],
                              body_contacts=frames["contacts"], fps=int(clip.fps), loop_mode="CLAMP")
    maxmin = clip.hf_maxmin if hf_extras is None else hf_extras["hf_maxmin"]
    if maxmin is None:   # a clip built in memory: SubTerrain's defaults (max 1, min -1 in every cell)
        maxmin = np.stack([np.ones_like(clip.hf), -np.ones_like(clip.hf)], -1)
    td = ms_file.MSTerrainData(hf=clip.hf, hf_maxmin=maxmin, min_point=clip.min_point, dx=float(clip.dx))
    ms_file.save_ms_file(ms_file.MSFileData(motion_data=md, terrain_data=td, misc_data=misc), path)


def run(cfg):
    from parc_amd.motion_lib import fetch_motion_files
    files, _ = fetch_motion_files(resolve(cfg["motions_yaml_path"]))
    clips = [mo.clip_from_ms(f) for f in files]
    opt = mo.MotionOptimizer(resolve(cfg["char_model"]), cfg["device"], cfg)
    if cfg["auto_compute_body_constraints"]:
        clips = opt.build_constraints(clips)
    stride = int(cfg["frame_stride"])
    clips = [c.strided(stride) for c in clips]
    out_dir = resolve(cfg["output_folder_path"])
    log_dir = os.path.join(out_dir, "log")
    os.makedirs(log_dir, exist_ok=True)
    logs = [open(os.path.join(log_dir, f"log_{c.name}_opt.txt"), "w") for c in clips]
    for f in logs:
        f.write("iteration\t" + "\t".join(t.name for t in mo.LossType) + "\n")

    def log(it, terms):
        for f, t in zip(logs, terms):
            f.write(f"{it}\t" + "\t".join(f"{v:.6g}" for v in t) + "\n")

    t0 = time.time()
    frames, hist = opt.optimize(clips, int(cfg["num_iters"]), int(cfg["log_every"]), log=log)
    for f, c, h in zip(logs, clips, hist):
        f.write(f"{h[-1][0]}\t" + "\t".join(f"{h[-1][1][t.name]:.6g}" for t in mo.LossType) + "\n")
        f.close()
    if cfg.get("remove_hesitation", False):   # parc_2_kin_gen.py:467-470: before compute_hf_extra_vals and the mirrored copy
        from parc_amd import motion_edit as me
        opt_clips = [mo.OptClip(fr["root_pos"], fr["root_rot"], fr["joint_rot"], fr["contacts"], c.hf, c.min_point, c.dx, c.fps, c.name)
                     for c, fr in zip(clips, frames)]
        remover = me.HesitationRemover(resolve(cfg["char_model"]), cfg["device"], float(cfg.get("hesitation_val", me.HESITATION_VAL)),
                                       int(cfg.get("hesitation_min_seq_len", me.HESITATION_MIN_SEQ_LEN)))
        short, _ = remover.remove(opt_clips)
        for c, s in zip(opt_clips, short):
            print(f"{c.name}: {c.num_frames - s.num_frames} hesitation frames removed ({c.num_frames} -> {s.num_frames})")
        frames = [dict(root_pos=s.root_pos, root_rot=s.root_rot, joint_rot=s.joint_rot, contacts=s.contacts) for s in short]
    extras = [None] * len(clips)
    if cfg["hf_extras"]:
        from parc_amd.motion_terrain import MotionTerrainAnalyzer
        opt_clips = [mo.OptClip(fr["root_pos"], fr["root_rot"], fr["joint_rot"], fr["contacts"], c.hf, c.min_point, c.dx, c.fps, c.name)
                     for c, fr in zip(clips, frames)]
        extras = MotionTerrainAnalyzer(resolve(cfg["char_model"]), cfg["device"]).analyze(opt_clips)
    paths = []
    for c, fr, ex in zip(clips, frames, extras):
        p = os.path.join(out_dir, c.name + "_opt.pkl")
        write_clip(p, fr, c, c, ex)
        paths.append(p)
    if cfg["save_flipped"]:
        from parc_amd.motion_aug import mirror_clips
        opt_clips = [mo.OptClip(fr["root_pos"], fr["root_rot"], fr["joint_rot"], fr["contacts"], c.hf, c.min_point, c.dx, c.fps, c.name + "_opt",
                                hf_maxmin=c.hf_maxmin if ex is None else ex["hf_maxmin"]) for c, fr, ex in zip(clips, frames, extras)]
        os.makedirs(os.path.join(out_dir, "flipped"), exist_ok=True)
        for fc in mirror_clips(opt_clips, resolve(cfg["char_model"]), cfg["device"]):
            p = os.path.join(out_dir, "flipped", fc.name + ".pkl")
            write_clip(p, dict(root_pos=fc.root_pos, root_rot=fc.root_rot, joint_rot=fc.joint_rot, contacts=fc.contacts), fc, mo.OptClip(
                fc.root_pos, fc.root_rot, fc.joint_rot, fc.contacts, fc.hf, fc.min_point, fc.dx))
            paths.append(p)
    print(f"optimised {len(clips)} clips x {cfg['num_iters']} iterations in {time.time() - t0:.2f} s")
    return paths


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--config", required=True)
    ap.add_argument("--hf_extras", action="store_true", help="write hf_mask_inds and recomputed hf_maxmin (config key hf_extras)")
    ap.add_argument("--save_flipped", action="store_true", help="also write flipped/<name>_opt_flipped.pkl, the mirrored copies (config key save_flipped)")
    ap.add_argument("--remove_hesitation", action="store_true",
                    help="drop the hesitation frames of the optimised clips before hf_extras and save_flipped (config key remove_hesitation)")
    args = ap.parse_args(argv)
    cfg = load_config(args.config)
    if args.hf_extras:
        cfg["hf_extras"] = True
    if args.save_flipped:
        cfg["save_flipped"] = True
    if args.remove_hesitation:
        cfg["remove_hesitation"] = True
    return run(cfg)


if __name__ == "__main__":
    main()
