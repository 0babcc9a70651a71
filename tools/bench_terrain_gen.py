#!/usr/bin/env python3
"""Time per kernel of the procedural terrain generator: hipEvents around each launch, the median (min - p90) of repeated
batches after a warm-up, for the three modes with the default config's settings.  Per configuration three timings: ``draw_plan``,
``generate_with`` of that plan, and the fused ``generate``.  One JSON line per configuration, appended to --out.

    python tools/bench_terrain_gen.py --out profiles/terrain_gen_bench.jsonl
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from parc_amd import terrain_gen as tg  # noqa: E402

CONFIGS = [(1024, 16), (16384, 16), (4096, 64)]


def stats(ms):
    a = np.asarray(ms)
    return {"median": round(float(np.median(a)), 4), "min": round(float(a.min()), 4), "p90": round(float(np.percentile(a, 90)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--config", default=os.path.join(REPO, "data/configs/terrain_gen/terrain_gen_default.yaml"))
    args = ap.parse_args()
    cfg = tg.TerrainGenConfig.load(args.config)
    for mode in tg.MODES:
        for n, dim in CONFIGS:
            G = tg.TerrainGenerator(mode, dim, dim, 0.4, settings=cfg.settings(mode))
            draw, gen_with, fused = [], [], []
            for it in range(args.warmup + args.repeats):
                plan = G.draw_plan(n, it)
                G.generate_with(plan)
                t = G.kernel_times()
                G.generate(n, it)
                f = G.kernel_times()["generate"]
                if it >= args.warmup:
                    draw.append(t["draw"]); gen_with.append(t["generate"]); fused.append(f)
            med = float(np.median(fused))
            rec = {"mode": mode, "terrains": n, "grid": [dim, dim], "settings": cfg.settings(mode).to_config(), "repeats": args.repeats,
                   "ms_draw_plan": stats(draw), "ms_generate_with": stats(gen_with), "ms_generate_fused": stats(fused),
                   "terrains_per_s_fused": round(n / (med * 1e-3), 1), "us_per_terrain_fused": round(med * 1e3 / n, 4)}
            print(json.dumps(rec), flush=True)
            if args.out:
                with open(args.out, "a") as f_:
                    f_.write(json.dumps(rec) + "\n")
            del G


if __name__ == "__main__":
    main()
