#!/usr/bin/env python3
"""Timing of the headless renderer (parc_env_render) and of a roll-out with and without the viewer; GPU only.

    python tools/render_bench.py [--envs 64] [--iters 50] [--out DIR]

(1) k_render per call at 1 / 16 / 64 envs x 320x240, shadows on / off: device events around `iters` back-to-back calls (take
    rocprofv3 --kernel-trace --stats of the same run for the kernel-only figure); (2) env steps per second of a step + reset loop of
    `--envs` envs with visualize off, then on (camera env -> FrameWriter -> PNG in --out).  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from parc_amd.envs import env_builder  # noqa: E402
from parc_amd.util.frame_writer import FrameWriter  # noqa: E402

CFG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "data/configs/tracker_config/dm_env_default.yaml")


def time_render(env, k, shadows, iters, W=320, H=240):
    ids = torch.arange(k, dtype=torch.long, device="cuda:0")
    for _ in range(3):
        env.render(ids, W, H, shadows=shadows)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        env.render(ids, W, H, shadows=shadows)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def rollout(visualize, envs, steps, out_dir):
    env = env_builder.build_env(CFG, envs, "cuda:0", visualize)
    fw = None
    if visualize:
        fw = FrameWriter(out_dir)
        env.set_frame_sink(fw, every=1, size=(320, 240))
    env.reset()
    for _ in range(10):
        env.step_and_reset_done(env._char_dof_pos.clone())
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        env.step_and_reset_done(env._char_dof_pos.clone())
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    res = {"steps_per_s": steps / dt, "env_steps_per_s": steps * envs / dt}
    if fw is not None:
        fw.close()
        res.update(frames_written=fw.written, frames_dropped=fw.dropped)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(tempfile.gettempdir(), "parc_render_bench_frames"))
    ap.add_argument("--render-only", action="store_true")
    a = ap.parse_args()
    env = env_builder.build_env(CFG, 64, "cuda:0", False)
    env.reset()
    for _ in range(3):
        env.step(env._char_dof_pos.clone())
        env.reset_done()
    out = {"render_ms_320x240": {}}
    for k in (1, 16, 64):
        for sh in (True, False):
            out["render_ms_320x240"]["k%d_%s" % (k, "shadows" if sh else "noshadows")] = round(time_render(env, k, sh, a.iters), 4)
    del env
    if not a.render_only:
        out["rollout_visualize_false"] = rollout(False, a.envs, a.steps, a.out)
        out["rollout_visualize_true"] = rollout(True, a.envs, a.steps, a.out)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
