#!/usr/bin/env python3
"""Sample generator-training batches on the GPU and write them where a PARC trainer can read them.

    python scripts/export_generator_batches.py --config data/configs/motion_sampler/motion_sampler_default.yaml \\
        --num_batches 8 --batch_size 64 --out output/gen_batches [--seed 0] [--motion_file FILE] [--device cuda:0]

Writes ``batch_%06d.npz`` (``root_pos``, ``root_rot``, ``joint_pos``, ``joint_rot``, ``contacts`` [, ``floor_heights``], the
concatenated ``features`` [N, T, D], ``hfs`` [N, Gx, Gy], ``target_pos``, ``target_rot``) and ``feature_stats.yaml`` with the
``mean`` / ``std`` layout ``MDM._compute_stats`` writes.  Batch b is ``sample(batch_size, seed + b)``.  Clips too short for a window
are left out and named.
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def usable_clips(motion_file, T):
    """(names kept, names refused) by the window length: a clip needs num_frames - T > 0."""
    from parc_amd import motion_lib
    clips = motion_lib.load_motion_file(motion_file, verbose=False)
    keep = [c.name for c in clips if c.num_frames - T > 0]
    return keep, [c.name for c in clips if c.num_frames - T <= 0]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="data/configs/motion_sampler/motion_sampler_default.yaml")
    ap.add_argument("--num_batches", type=int, required=True)
    ap.add_argument("--batch_size", type=int, default=None)
    ap.add_argument("--out", required=True)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--motion_file", default=None)
    ap.add_argument("--device", default=None)
    a = ap.parse_args(argv)
    from parc_amd import motion_sampler as ms
    from parc_amd.util import path_loader
    cfg = path_loader.load_config(a.config)
    motion_file = a.motion_file or cfg["motion_lib_file"]
    char_file = str(path_loader.resolve_path(cfg["char_file"]))
    keep, refused = usable_clips(motion_file, ms.parse_config(cfg).T)
    for name in refused:
        print(f"refused: {name} is too short for a window of {ms.parse_config(cfg).T} frames")
    if not keep:
        raise SystemExit("no clip is long enough")
    sampler = ms.MotionWindowSampler(cfg, motion_file, char_file, a.device or cfg.get("device", "cuda:0"), exclude=refused)
    files = ms.export_batches(sampler, a.num_batches, a.batch_size or int(cfg.get("batch_size", 64)), a.out, a.seed)
    print(f"wrote {len(files)} batches and feature_stats.yaml to {a.out} ({len(keep)} clips)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
