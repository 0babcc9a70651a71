#!/usr/bin/env python3
"""Timing of the headless renderer (parc_env_render) and of a roll-out with and without the viewer; GPU only.

    python tools/render_bench.py [--envs 64] [--iters 50] [--out DIR]

(1) k_render per call at 1 / 16 / 64 envs x 320x240, shadows on / off: device events around `iters` back-to-back calls (take
    rocprofv3 --kernel-trace --stats of the same run for the kernel-only figure); (2) env steps per second of a step + reset loop of
    `--envs` envs with visualize off, then on (camera env -> FrameWriter -> PNG in --out).  Prints one JSON line.
(3) --scene: parc_env_render_scene (all seven launches) per call at 320x240 with every env drawn, at 64 / 4096 / 65536 envs
    (--scene-envs), shadows on / off, with the default track camera of env 0 and with a still camera looking at an empty corner of
    the world (few characters in view); and the roll-out rate with scene frames after every step next to camera-only frames.
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


def time_scene(env, shadows, iters, camera=None, W=320, H=240):
    for _ in range(3):
        env.render_scene(0, None, W, H, camera=camera, shadows=shadows)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        env.render_scene(0, None, W, H, camera=camera, shadows=shadows)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def scene_timings(sizes, iters):
    out = {}
    for n in sizes:
        env = env_builder.build_env(CFG, n, "cuda:0", False)
        env.reset()
        for _ in range(3):
            env.step(env._char_dof_pos.clone())
            env.reset_done()
        eo = env._scene.env_offsets[0]
        # still camera over the world's -x, -y corner beyond every env origin: a handful of characters in view at most
        lo = env._scene.env_offsets.min(axis=0)
        corner = {"mode": "still", "eye": tuple(float(v) for v in (lo + [-30.0, -30.0, 8.0] - eo)),
                  "target": tuple(float(v) for v in (lo + [-20.0, -20.0, 0.0] - eo))}
        _, _, _, em = env.render_scene(0, None, 320, 240, camera=corner, env_map=True)
        _, _, _, em_t = env.render_scene(0, None, 320, 240, env_map=True)
        torch.cuda.synchronize()
        row = {"envs_in_view_track": int(torch.unique(em_t).numel() - 1), "envs_in_view_corner": int(torch.unique(em).numel() - 1)}
        for sh in (True, False):
            tag = "shadows" if sh else "noshadows"
            row["track_" + tag] = round(time_scene(env, sh, iters), 4)
            row["corner_" + tag] = round(time_scene(env, sh, iters, corner), 4)
        out["n%d" % n] = row
        del env
        torch.cuda.empty_cache()
    return out


def rollout(visualize, envs, steps, out_dir, scene=False):
    env = env_builder.build_env(CFG, envs, "cuda:0", visualize)
    fw = None
    if visualize:
        fw = FrameWriter(out_dir)
        env.set_frame_sink(fw, every=1, size=(320, 240), scene=scene)
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
    ap.add_argument("--scene", action="store_true", help="only the scene render timings and the scene roll-out")
    ap.add_argument("--scene-envs", default="64,4096,65536")
    a = ap.parse_args()
    if a.scene:
        out = {"render_scene_ms_320x240": scene_timings([int(v) for v in a.scene_envs.split(",")], a.iters)}
        out["rollout_visualize_camera_env"] = rollout(True, a.envs, a.steps, a.out)
        out["rollout_visualize_scene"] = rollout(True, a.envs, a.steps, a.out, scene=True)
        print(json.dumps(out))
        return
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
