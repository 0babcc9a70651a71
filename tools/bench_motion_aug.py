#!/usr/bin/env python3
"""Time per launch of the motion-terrain augmenter: hipEvents around each phase, the median (min - p90) of repeated runs
after a warm-up, for the three edit modes on the bundled clips with the default config's settings.  Per mode: ``draw_plan``, the three
phases of ``augment_with`` of that plan (layout + scan, frames + scan, terrain), and the same three of the fused ``augment``.  One JSON
line per mode, appended to --out.

    python tools/bench_motion_aug.py --out profiles/motion_aug_bench.jsonl
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from parc_amd import motion_aug as ma  # noqa: E402
from parc_amd import motion_opt as mo  # noqa: E402


def stats(ms):
    a = np.asarray(ms)
    return {"median": round(float(np.median(a)), 4), "min": round(float(a.min()), 4), "p90": round(float(np.percentile(a, 90)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variations", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--dump_plans", default=None, help="write the first timed plan of every mode to this .npz (the CPU baseline times the same plans)")
    ap.add_argument("--config", default=os.path.join(REPO, "data/configs/motion_aug/motion_aug_default.yaml"))
    args = ap.parse_args()
    from parc_amd.motion_lib import fetch_motion_files
    cfg = ma.load_config(args.config)
    files, _ = fetch_motion_files(os.path.join(REPO, cfg["motions_yaml_path"]))
    clips = [mo.clip_from_ms(f) for f in files]
    n = args.variations
    dumped = {}
    for mode in ma.MODES:
        aug = ma.MotionAugmenter(os.path.join(REPO, cfg["char_model"]), clips, ma.MotionAugSettings.from_config(dict(cfg, terrain_aug_type=mode)))
        with_plan, fused = [], []
        frames = cells = 0
        for it in range(args.warmup + args.repeats):
            plan = aug.draw_plan(n, it)
            if it == args.warmup and args.dump_plans:
                dumped.update({f"{mode}_{k}": v.cpu().numpy() for k, v in plan.items()})
            res = aug.augment_with(plan)
            t = aug.kernel_times()
            frames, cells = int(res.root_pos.shape[0]), int(res.hf.shape[0])
            del res
            res = aug.augment(n, it)
            f = aug.kernel_times()
            del res
            if it >= args.warmup:
                with_plan.append([t[k] for k in ma.KERNELS]); fused.append([f[k] for k in ma.KERNELS[1:]])
        wp, fu = np.asarray(with_plan), np.asarray(fused)
        rec = {"mode": mode, "variations": n, "frames": frames, "cells": cells, "repeats": args.repeats,
               "ms_draw_plan": stats(wp[:, 0]), "ms_augment_with": {k: stats(wp[:, 1 + i]) for i, k in enumerate(ma.KERNELS[1:])},
               "ms_augment_with_launches": stats(wp[:, 1:].sum(axis=1)), "ms_augment_fused": {k: stats(fu[:, i]) for i, k in enumerate(ma.KERNELS[1:])},
               "ms_augment_fused_launches": stats(fu.sum(axis=1)), "us_per_variation_fused": round(float(np.median(fu.sum(axis=1))) * 1e3 / n, 4)}
        print(json.dumps(rec), flush=True)
        if args.out:
            with open(args.out, "a") as f_:
                f_.write(json.dumps(rec) + "\n")
        del aug
    if args.dump_plans:
        np.savez_compressed(args.dump_plans, **dumped)


if __name__ == "__main__":
    main()
