#!/usr/bin/env python3
"""ms per motion-terrain analysis (parc_mterr_run + parc_mterr_get_mask_inds, i.e. including the mask-ind download) and its
per-kernel split (hipEvents) for 1, 64, 1 024 copies of the bundled 142-frame clip and 16 384 synth_dataset pseudo-clips (the
bundled clips yaw-rotated with their terrain).  The reference's compute_hf_extra_vals + compute_motion_loss on ONE clip on the CPU
is the baseline.  Prints one JSON line per batch size.

    python tools/motion_terrain_bench.py [repeats] [batch sizes, comma-separated]
"""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402

from parc_amd import motion_opt as mo  # noqa: E402
from parc_amd import motion_terrain as mt  # noqa: E402


def synth_clips(n):
    from parc_amd import motion_lib
    from parc_amd.util import synth_dataset
    base = motion_lib.load_motion_file(os.path.join(REPO, "data/motion_terrains/motions_bundled.yaml"), verbose=False)
    out = []
    for c in synth_dataset.make_library(base, n):
        ct = np.zeros((c.num_frames, c.joint_rot.shape[1] + 1), np.float32) if c.contacts is None else np.asarray(c.contacts, np.float32)
        out.append(mo.OptClip(c.root_pos, c.root_rot, c.joint_rot, ct, np.asarray(c.terrain.hf, np.float32),
                              np.asarray(c.terrain.min_point, np.float32), float(c.terrain.dx)))
    return out


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    sizes = [int(s) for s in sys.argv[2].split(",")] if len(sys.argv) > 2 else [1, 64, 1024, 16384]
    a = mt.MotionTerrainAnalyzer(os.path.join(REPO, "data/assets/humanoid.xml"), "cuda:0")
    base = mo.clip_from_ms(os.path.join(REPO, "data/motion_terrains/dec2024_teaser_717_1_modified_opt.pkl"))
    for n in sizes:
        clips = synth_clips(n) if n > 1024 else [base] * n
        a.run(clips)                                          # warm-up (and the upload)
        L, lib, h = a._L, a._lib, a._h
        F, ncell = int(a._packed["frame_off"][-1]), int(a._packed["hf_off"][-1])
        out, cnt, mm = np.zeros((n, 6), np.float32), np.zeros(F, np.int32), np.zeros((ncell, 2), np.float32)
        tot = mt.C.c_int64()
        walls, kts = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            L.check(lib.parc_mterr_run(h, L.np_f32p(out), L.np_i32p(cnt), L.np_f32p(mm), mt.C.byref(tot)))
            inds = np.empty((tot.value, 2), np.int32)
            L.check(lib.parc_mterr_get_mask_inds(h, L.np_i32p(inds)))
            walls.append((time.perf_counter() - t0) * 1e3)
            kts.append(a.kernel_times())
        t0 = time.perf_counter()
        res = a.analyze(clips)
        py_ms = (time.perf_counter() - t0) * 1e3
        kt = {k: round(float(np.median([x[k] for x in kts])), 4) for k in mt.KERNELS}
        print(json.dumps({"clips": n, "frames": F, "points_per_frame": int(a.points.shape[0]), "cells": ncell, "mask_inds": int(tot.value),
                          "ms_per_analysis": round(float(np.median(walls)), 3), "ms_kernels": round(sum(kt.values()), 3), "kernel_ms": kt,
                          "ms_analyze_python_incl_upload_and_split": round(py_ms, 1),
                          "finite": bool(np.isfinite([r["pen_loss"] for r in res]).all())}), flush=True)


if __name__ == "__main__":
    main()
