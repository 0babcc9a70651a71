#!/usr/bin/env python3
"""ms of the rollout selection at N = 32 and N = 1 024 rows (16 candidates per path, one 32 x 32 terrain per
path; default-size model, weights from a seed, one 10-window rollout): ``PathMotionGenerator.select`` + ``to_clips`` (the host-bound
path: the rollout buffer to the host, N clips with their terrains up again, the analyser's six kernels, a numpy sort) alternating with
``PathSelector.select`` + ``to_clips``, on the whole terrain and sliced (the gather of the kept slices included).  Wall clock around a
device synchronise, the median of ``repeats`` with min - max, after a warm-up; a difference is called shown only where the runs do not
overlap.  The selector's per-kernel device times (hipEvents) go beside them.  Prints one JSON line per N and appends it to
``profiles/mdm_select_bench.jsonl``.

    python tools/mdm_select_bench.py [repeats] [rows, comma-separated]
"""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from parc_amd import motion_generator as mg  # noqa: E402
from parc_amd import motion_path_gen as mpg  # noqa: E402
from parc_amd import motion_select as msel  # noqa: E402

DEV = "cuda:0"
K, TOP_K = 16, 4
MAX_LEN = 2.3          # as tools/mdm_path_bench.py: the time limit ends the rollout at the tenth window


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(v):
    return {"median": round(float(np.median(v)), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def verdict(a, b, names):
    if max(a) < min(b):
        return names[0] + " faster"
    if max(b) < min(a):
        return names[1] + " faster"
    return "not shown"


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    sizes = [int(s) for s in sys.argv[2].split(",")] if len(sys.argv) > 2 else [32, 1024]
    cfg = mg.default_config()
    sd = mg.random_state_dict(cfg, 0)
    g = torch.Generator().manual_seed(1)
    mean, std = torch.randn((15, 91), generator=g) * 0.3, torch.rand((15, 91), generator=g) * 1.5 + 0.5
    ps, gs = mpg.MDMPathSettings(max_motion_length=MAX_LEN), mpg.MDMGenSettings()
    rng = np.random.RandomState(0)
    os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
    for n in sizes:
        P = n // K
        hfs = (np.kron(rng.randint(0, 3, (P, 8, 8)), np.ones((4, 4))) * 0.25).astype(np.float32)
        path = np.stack([0.5 * np.arange(24) + 1.0, np.full(24, 6.0), np.zeros(24)], axis=-1).astype(np.float32)
        gen = mg.MDMGenerator.from_state_dict(cfg, sd, mean, std, DEV, max_batch=n)
        pg = mpg.PathMotionGenerator(gen, ps, gs)
        sel = msel.PathSelector(pg)
        pg.set_scene(hfs, np.zeros((P, 2), np.float32), 0.4, [path] * P, K)
        res = pg.rollout(plan={"rel_height": torch.full((P,), 0.8)}, seed=0)
        torch.cuda.synchronize()

        def old():
            for s in pg.select(res, top_k=TOP_K, seed=0):
                pg.to_clips(res, s["rows"])

        def new(sliced):
            for s in sel.select(res, top_k=TOP_K, seed=0, slice_terrain=sliced):
                pg.to_clips(res, s["rows"], terrains=s.get("terrains"))

        t = {"host": [], "device_whole": [], "device_sliced": []}
        kt = {}
        for i in range(reps + 2):                                   # alternating; the first two rounds are the warm-up
            a, b = timed(old), timed(lambda: new(False))
            kt["whole"] = sel.kernel_times()
            c = timed(lambda: new(True))
            kt["sliced"] = sel.kernel_times()
            if i >= 2:
                t["host"].append(a); t["device_whole"].append(b); t["device_sliced"].append(c)
        same = all(np.array_equal(o["rows"], w["rows"]) for o, w in zip(pg.select(res, top_k=TOP_K, seed=0), sel.select(res, top_k=TOP_K, seed=0, slice_terrain=False)))
        line = {"tool": "mdm_select_bench", "rows": n, "paths": P, "frames": int(res.num_frames), "finished": int((res.final_frame >= 0).sum()), "top_k": TOP_K,
                "repeats": reps, "host_select_ms": stats(t["host"]), "device_select_whole_ms": stats(t["device_whole"]),
                "device_select_sliced_ms": stats(t["device_sliced"]), "whole_vs_host": verdict(t["device_whole"], t["host"], ("device", "host")),
                "sliced_vs_host": verdict(t["device_sliced"], t["host"], ("device", "host")),
                "kernels_ms": {m: {k: round(v, 4) for k, v in d.items()} for m, d in kt.items()}, "launches": sel.describe()["launches"],
                "same_rows_as_host_select": bool(same)}
        print(json.dumps(line), flush=True)
        with open(os.path.join(REPO, "profiles", "mdm_select_bench.jsonl"), "a") as f:
            f.write(json.dumps(line) + "\n")
        sel._destroy()
        del sel, pg, gen


if __name__ == "__main__":
    main()
