#!/usr/bin/env python3
"""ms per batch of the motion-window sampler (``MotionWindowSampler.sample``: draw_plan + window + heightfield kernels) and its
per-kernel split (hipEvents) at 64, 1 024 and 16 384 samples of the default config on the bundled clips (``sfu`` is too short for a
window and is left out).  Per size: warm-up, ``repeats`` timed batches each ended by a device synchronise, median and spread; the bytes a
batch writes (counted from the shapes) over the kernel time, beside the fill rate of ``profiles/r04_hbm_copy_bw.json``.  For
orientation the CPU restatement (``tests/motion_sampler_ref.py``) is timed on 64 samples: a different machine and a different
program, not a ratio.  Prints one JSON line per batch size.

    python tools/motion_sampler_bench.py [repeats] [batch sizes, comma-separated] [--no-cpu]
"""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "scripts"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from parc_amd import motion_sampler as ms  # noqa: E402
from parc_amd.util import path_loader  # noqa: E402


def bytes_per_sample(c, B):
    """floats a default-config sample writes: the motion outputs, the patch, the targets (the plan is read, not counted)."""
    return 4 * (c.T * (3 + 4 + 3 * (B - 1) + 4 * (B - 1) + B) + c.Gx * c.Gy + 7)


def cpu_restatement_ms(sampler, n):
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import helpers
    import motion_sampler_ref as ref
    lib = ref.Library(helpers.load_clips(sampler.clip_names), sampler.extra_vals, [c.weight for c in sampler.clips])
    plan = {k: v.cpu().numpy() for k, v in sampler.draw_plan(n, 1).items()}
    ref.sample_with(lib, sampler.char_model, sampler.cfg, plan)
    t0 = time.perf_counter()
    ref.sample_with(lib, sampler.char_model, sampler.cfg, plan)
    return (time.perf_counter() - t0) * 1e3


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(args[0]) if len(args) > 0 else 50
    sizes = [int(s) for s in args[1].split(",")] if len(args) > 1 else [64, 1024, 16384]
    import export_generator_batches as ex
    cfg = path_loader.load_config(os.path.join(REPO, "data/configs/motion_sampler/motion_sampler_default.yaml"))
    keep, refused = ex.usable_clips(cfg["motion_lib_file"], ms.parse_config(cfg).T)
    s = ms.MotionWindowSampler(cfg, cfg["motion_lib_file"], os.path.join(REPO, cfg["char_file"]), "cuda:0", exclude=refused)
    fill = json.load(open(os.path.join(REPO, "profiles/r04_hbm_copy_bw.json")))["fill_GBps_write"]
    for n in sizes:
        for w in range(5):
            s.sample(n, w)
        torch.cuda.synchronize()
        walls, kts = [], []
        for r in range(reps):
            t0 = time.perf_counter()
            out = s.sample(n, 100 + r)
            torch.cuda.synchronize()
            walls.append((time.perf_counter() - t0) * 1e3)
            kts.append(s.kernel_times())
        kt = {k: float(np.median([x[k] for x in kts])) for k in ms.KERNELS}
        by = bytes_per_sample(s.cfg, s.B) * n
        floor_us = by / (fill * 1e9) * 1e6
        line = {"samples": n, "clips": keep, "refused": refused, "repeats": reps,
                "ms_per_batch_median": round(float(np.median(walls)), 4), "ms_per_batch_min": round(float(np.min(walls)), 4),
                "ms_per_batch_p90": round(float(np.percentile(walls, 90)), 4),
                "kernel_ms": {k: round(v, 4) for k, v in kt.items()}, "ms_kernels": round(sum(kt.values()), 4),
                "bytes_written": by, "write_floor_us_at_fill_rate": round(floor_us, 2), "fill_GBps": fill,
                "GBps_written_over_kernel_time": round(by / (sum(kt.values()) * 1e-3) / 1e9, 1),
                "finite": bool(all(torch.isfinite(t).all().item() for t in (out[1], out[2], out[3], out[0]["ROOT_POS"])))}
        if n == 64 and "--no-cpu" not in sys.argv:
            line["cpu_restatement_ms_other_machine_other_program"] = round(cpu_restatement_ms(s, 64), 1)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
