#!/usr/bin/env python3
"""Per-kernel device time (hipEvents) of the contact labelling (parc_mlabel_run) and of the resampling to 60 fps (parc_mlabel_resample),
and the host time of the whole call, for batches of `civilization` on its own 50 x 50 terrain repeated.  The reference's functions on
ONE such clip on the CPU are the baseline (tests/golden/make_golden_motion_label.py prints their time per case).
Prints one JSON line per batch.

    python tools/motion_label_bench.py [repeats] [clips, comma-separated]      # default 3  1,1024
"""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402

from parc_amd import motion_label as ml  # noqa: E402
from parc_amd import motion_opt as mo  # noqa: E402


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    batches = sys.argv[2] if len(sys.argv) > 2 else "1,1024"
    clip = mo.clip_from_ms(os.path.join(REPO, "data/motion_terrains/civilization.pkl"))
    h = ml.ContactLabeller(os.path.join(REPO, "data/assets/humanoid.xml"), "cuda:0")
    for b in batches.split(","):
        n = int(b)
        h.run([clip] * n)                                     # warm-up
        walls, kts = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            r = h.run([clip] * n)
            walls.append((time.perf_counter() - t0) * 1e3)
            kts.append(h.kernel_times())
        h.resample([clip] * n, 60)
        rs = []
        for _ in range(reps):
            out = h.resample([clip] * n, 60)
            rs.append(h.kernel_times()["resample"])
        kt = {k: round(float(np.median([x[k] for x in kts])), 4) for k in ("feet", "hands")}
        kt["resample"] = round(float(np.median(rs)), 4)
        F = clip.num_frames * n
        print(json.dumps({"clips": n, "frames": F, "terrain": list(clip.hf.shape), "cell_sdfs": 2 * F * clip.hf.size,
                          "lifted_per_clip": int((r["lift"][:clip.num_frames] > 0).sum()), "resampled_frames": sum(c.num_frames for c in out),
                          "kernel_ms": kt, "ms_run_python_incl_packing_and_upload": round(float(np.median(walls)), 2)}), flush=True)


if __name__ == "__main__":
    main()
