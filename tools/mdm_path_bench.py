#!/usr/bin/env python3
"""ms per window and per 10-window rollout of path-following generation (default-size model, weights from a seed, guidance on, 3 DDIM
steps) at N = 32 and N = 1 024 rows, against the torch composition the tests use (``tests/mdm_path_ref.py`` around
``MDMGenerator.gen_sequence`` on the same GPU), with the device times of the two wrapper kernels beside the generator's
``cond / forward / update`` (hipEvents).  Each side is timed ``repeats`` times after a warm-up with a device
synchronisation around every timed call; a gap of the medians under three times the larger spread is "not shown" (section 9's rule).
Prints one JSON line per N and appends it to ``profiles/mdm_path_bench.jsonl``.

    python tools/mdm_path_bench.py [repeats] [rows, comma-separated]
"""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import mdm_path_ref as PR  # noqa: E402
from parc_amd import motion_generator as mg  # noqa: E402
from parc_amd import motion_path_gen as mpg  # noqa: E402

DEV = "cuda:0"
WINDOWS = 10
MAX_LEN = 2.3          # 9 + 7 w frames after window w at 30 fps: the time limit ends the rollout at the tenth window


def timed(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def stats(v):
    return {"median": round(float(np.median(v)), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    sizes = [int(s) for s in sys.argv[2].split(",")] if len(sys.argv) > 2 else [32, 1024]
    cfg = mg.default_config()
    sd = mg.random_state_dict(cfg, 0)
    g = torch.Generator().manual_seed(1)
    mean, std = torch.randn((15, 91), generator=g) * 0.3, torch.rand((15, 91), generator=g) * 1.5 + 0.5
    ps, gs = mpg.MDMPathSettings(max_motion_length=MAX_LEN), mpg.MDMGenSettings()
    rng = np.random.RandomState(0)
    hf = (np.kron(rng.randint(0, 3, (8, 8)), np.ones((4, 4))) * 0.25).astype(np.float32)
    path = np.stack([0.5 * np.arange(24) + 200.0, np.full(24, 6.0), np.zeros(24)], axis=-1).astype(np.float32)   # far away: no row is ever done
    os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
    for n in sizes:
        gen = mg.MDMGenerator.from_state_dict(cfg, sd, mean, std, DEV, max_batch=n)
        pg = mpg.PathMotionGenerator(gen, ps, gs)
        pg.set_scene(hf[None], np.zeros((1, 2), np.float32), 0.4, [path], n)
        xT = torch.randn((WINDOWS, n, 15, 91), generator=g).to(DEV)
        plan = {"rel_height": torch.tensor([0.8])}
        res = pg.rollout(plan=plan, noise=xT)
        assert res.windows == WINDOWS, res.windows
        ref = PR.PathRef(cfg, gen.char_model, mean, std, ps, gs, torch.float32, DEV)
        scene = PR.Scene(hf[None], np.zeros((1, 2), np.float32), 0.4, [path], [0] * n, torch.float32, DEV)

        def generate(c, w):
            c = dict(c)
            c["GUIDANCE_PARAMS"] = mg.GuidanceParams(c["GUIDANCE_PARAMS"])
            return gen.gen_sequence(c, gs.ddim_stride, "DDIM", noise=xT[w])

        comp = ref.rollout(scene, generate, [0.8])
        assert comp["windows"] == WINDOWS
        err = max((getattr(res, k) - comp["frames"][k]).abs().max().item() for k in PR.FRAME_KEYS)
        hip = timed(lambda: pg.rollout(plan=plan, noise=xT), reps + 2)[2:]
        kt, gt = pg.kernel_times(), gen.kernel_times()
        torch_ms = timed(lambda: ref.rollout(scene, generate, [0.8]), reps + 2)[2:]
        a, b = stats(hip), stats(torch_ms)
        gap, spread = b["median"] - a["median"], max(a["max"] - a["min"], b["max"] - b["min"])
        shown = (max(hip) < min(torch_ms) or max(torch_ms) < min(hip)) and abs(gap) >= 3 * spread
        line = {"tool": "mdm_path_bench", "rows": n, "windows": WINDOWS, "steps": pg.steps, "repeats": reps, "hip_rollout_ms": a, "torch_composition_ms": b,
                "hip_ms_per_window": round(a["median"] / WINDOWS, 3), "torch_ms_per_window": round(b["median"] / WINDOWS, 3),
                "ratio_torch_over_hip": round(b["median"] / a["median"], 2), "verdict": ("hip faster" if gap > 0 else "torch faster") if shown else "not shown",
                "wrapper_kernels_ms_per_rollout": {k: round(v, 4) for k, v in kt.items()}, "generator_kernels_ms_last_window": {k: round(v, 4) for k, v in gt.items()},
                "launches": pg.describe()["launches"], "max_abs_diff_vs_composition": err}
        print(json.dumps(line), flush=True)
        with open(os.path.join(REPO, "profiles", "mdm_path_bench.jsonl"), "a") as f:
            f.write(json.dumps(line) + "\n")
        del pg, gen


if __name__ == "__main__":
    main()
