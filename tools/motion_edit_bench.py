#!/usr/bin/env python3
"""Per-kernel device time (hipEvents) of the hesitation-frame removal (parc_medit_run + parc_medit_get_frames) and the host time of
the whole call, for batches of one clip repeated: `civilization` wrapped around to the given number of frames (its first frames again
at the end: one hold, removed).  The reference's remove_hesitation_frames on ONE such clip on the CPU is the baseline
(tests/golden/make_golden_hesitation.py prints its time per case).  Prints one JSON line per batch.

    python tools/motion_edit_bench.py [repeats] [clips x frames, comma-separated]      # default 3  1x300,1024x300,1x4096,16x4096
"""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402

from parc_amd import motion_edit as me  # noqa: E402
from parc_amd import motion_opt as mo  # noqa: E402


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    batches = sys.argv[2] if len(sys.argv) > 2 else "1x300,1024x300,1x4096,16x4096"
    src = mo.clip_from_ms(os.path.join(REPO, "data/motion_terrains/civilization.pkl"))
    h = me.HesitationRemover(os.path.join(REPO, "data/assets/humanoid.xml"), "cuda:0")
    flat = (np.zeros((2, 2), np.float32), np.zeros(2, np.float32), 0.5)   # the tool validates a terrain and ignores it
    for b in batches.split(","):
        n, T = (int(x) for x in b.split("x"))
        idx = np.arange(T) % src.num_frames
        clip = mo.OptClip(src.root_pos[idx], src.root_rot[idx], src.joint_rot[idx], src.contacts[idx], *flat)
        h.run([clip] * n)                                     # warm-up
        walls, kts = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            r = h.run([clip] * n)
            walls.append((time.perf_counter() - t0) * 1e3)
            kts.append(h.kernel_times())
        kt = {k: round(float(np.median([x[k] for x in kts])), 4) for k in me.KERNELS}
        print(json.dumps({"clips": n, "frames_per_clip": T, "pairs": n * T * (T - 1) // 2, "kept_per_clip": int(r["counts"][0]),
                          "kernel_ms": kt, "ms_kernels": round(sum(kt.values()), 3),
                          "ms_run_python_incl_packing_and_upload": round(float(np.median(walls)), 2)}), flush=True)


if __name__ == "__main__":
    main()
