#!/usr/bin/env python3
"""Generate motions along planned paths with the MDM generator on the GPU: stage 2's "generate, score, keep the best".

    python scripts/generate_path_motions.py --paths output/paths --out output/path_motions \\
        (--checkpoint model.ckpt [--use_ema_model] [--feature_stats feature_stats.yaml] | --random_init SEED) \\
        [--config data/configs/mdm_path/mdm_path_default.yaml] [--candidates 32] [--top_k 4] [--max_batch 64] [--seed 0] [--device cuda:0]

Reads the ``paths_*.npz`` batches of ``scripts/plan_paths.py`` (``hf``, ``min_point_offset``, ``dx``, ``points``, ``point_off``).  The
``hf`` of those files is the heightfield the planner searched (simplified when the planner's config says so); it is used as it is.
For every found path ``--candidates`` rows are rolled out (in chunks of whole paths that fit ``--max_batch`` rows), scored on the
whole terrain and sorted; the best ``--top_k`` are written as ``<out>/path_<batch>_<terrain>_<rank>.pkl`` (motion plus terrain, the
container ``scripts/run_optimize_motions.py`` reads; ``misc_data`` holds the losses, ``final_frame`` and ``num_frames``).  One JSON
line is printed: paths, rows, finished rows, windows, seconds.  ``--random_init SEED`` is a dry run: weights from the seed, zero
mean and unit std.  The found paths are numbered through all files in order; path k has the global path id k (the key of its drawn
start) and its row r the global row id ``k * candidates + r`` (the key of its x_T), whatever the chunking.  A run whose ids would pass
2^28 rows is refused before anything is generated.

``--device_select`` scores, filters and ranks on the device (``parc_amd.motion_select``); ``--slice_terrain`` (which implies it) scores
every row on its own slice of the terrain, as the reference does for procedural terrains, and writes that slice into the ``.pkl``.
``--max_contact_loss`` / ``--max_pen_loss`` / ``--max_total_loss`` keep only rows under them (the reference's acceptance test); a path with
fewer than ``--top_k`` such rows is rolled out again with the same ids and ``seed + attempt``, up to ``--max_attempts`` rollouts, then
skipped and counted as ``short_paths`` in the JSON line.
"""
import argparse
import glob
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


MAX_ROW_ID = 1 << 28       # parc_mpath_rollout's row ids


def read_paths(path):
    """``[(terrain index, hf [X, Y], min_point [2], dx, points [n, 3])]`` of the found paths of one ``paths_*.npz``."""
    import numpy as np
    z = np.load(path)
    off, pts, out = z["point_off"], z["points"], []
    for q in range(len(off) - 1):
        p = np.asarray(pts[off[q]:off[q + 1]], np.float32).reshape(-1, 3)
        if len(p) < 2:
            continue
        mp = np.asarray(z["min_point_offset"][q], np.float32)
        p = p.copy()
        p[:, 0:2] += mp
        out.append((q, np.asarray(z["hf"][q], np.float32), mp, float(z["dx"]), p))
    return out


def chunks(items, paths_per_chunk):
    for i in range(0, len(items), paths_per_chunk):
        yield items[i:i + paths_per_chunk]


def file_name(batch, terrain, rank):
    return "path_%04d_%05d_%d.pkl" % (batch, terrain, rank)


def save_clip(clip, path, misc):
    import numpy as np
    from parc_amd import ms_file
    md = ms_file.MSMotionData(root_pos=clip.root_pos, root_rot=clip.root_rot, joint_rot=clip.joint_rot, body_contacts=clip.contacts, fps=int(clip.fps),
                              loop_mode="CLAMP")
    maxmin = np.zeros(clip.hf.shape + (2,), np.float32)
    maxmin[..., 0], maxmin[..., 1] = 1.0, -1.0                 # SubTerrain's default bounds
    td = ms_file.MSTerrainData(hf=clip.hf, hf_maxmin=maxmin, min_point=np.asarray(clip.min_point, np.float32), dx=float(clip.dx))
    ms_file.save_ms_file(ms_file.MSFileData(motion_data=md, terrain_data=td, misc_data=misc), path)


def write_selection(handle, res, ids, final, b, g, sel, out_dir, sliced):
    """The kept rows of one path as ``.pkl`` files, on their slices where the selection made them."""
    clips = handle.to_clips(res, sel["rows"], terrains=sel["terrains"]) if sliced else handle.to_clips(res, sel["rows"])
    for rank, (clip, row) in enumerate(zip(clips, sel["rows"])):
        misc = dict(total_loss=float(sel["total_loss"][rank]), contact_loss=float(sel["contact_loss"][rank]), pen_loss=float(sel["pen_loss"][rank]),
                    final_frame=int(final[row]), num_frames=int(clip.num_frames), row_id=int(ids[row]), path=g[4])
        save_clip(clip, os.path.join(out_dir, file_name(b, g[0], rank)), misc)


def run_device_select(handle, selector, b, group, pids, candidates, top_k, seed, out_dir, stats, slice_terrain, thresholds, max_attempts):
    """One group of paths through ``selector`` (``motion_select.PathSelector``): a path with fewer than ``top_k`` valid rows is rolled out
    again, with the same ids and ``seed + attempt``, until ``max_attempts``; one that still falls short is skipped and counted."""
    import numpy as np
    pending = list(range(len(group)))
    for attempt in range(max_attempts):
        sub = [group[i] for i in pending]
        handle.set_scene(np.stack([g[1] for g in sub]), np.stack([g[2] for g in sub]), sub[0][3], [g[4] for g in sub], candidates)
        sub_pids = pids[pending]
        ids = (sub_pids[:, None] * candidates + np.arange(candidates)[None, :]).reshape(-1)
        res = handle.rollout(seed=seed + attempt, row_ids=ids, path_ids=sub_pids)
        final = res.final_frame.cpu().numpy()
        stats["rows"] += len(ids); stats["finished"] += int((final >= 0).sum()); stats["windows"] += int(res.windows)
        short = []
        for i, g, sel in zip(pending, sub, selector.select(res, top_k=top_k, seed=seed + b + attempt, slice_terrain=slice_terrain, **thresholds)):
            if not sel["enough"]:
                short.append(i)
                continue
            write_selection(handle, res, ids, final, b, g, sel, out_dir, slice_terrain)
        pending = short
        if not pending:
            break
    stats["short_paths"] += len(pending)


def run(handle, files, out_dir, candidates, top_k, seed, max_batch, *, selector=None, slice_terrain=False, max_contact_loss=None, max_pen_loss=None,
        max_total_loss=None, max_attempts=1):
    """The chunking and the naming, on any handle with ``set_scene`` / ``rollout`` / ``select`` / ``to_clips``.  ``selector`` (a
    ``motion_select.PathSelector`` on ``handle``) scores, filters and ranks on the device instead of ``handle.select``; the other keyword
    arguments are its."""
    import numpy as np
    thresholds = dict(max_contact_loss=max_contact_loss, max_pen_loss=max_pen_loss, max_total_loss=max_total_loss)
    if selector is None and (slice_terrain or max_attempts != 1 or any(v is not None for v in thresholds.values())):
        raise SystemExit("--slice_terrain, the loss thresholds and --max_attempts need --device_select")
    if max_attempts < 1:
        raise SystemExit("--max_attempts must be >= 1")
    per_chunk = max_batch // candidates
    if per_chunk < 1:
        raise SystemExit(f"--candidates {candidates} exceeds --max_batch {max_batch}")
    total = sum(int((np.diff(np.load(f)["point_off"]) >= 2).sum()) for f in files)
    if total * candidates > MAX_ROW_ID:
        raise SystemExit(f"{total} paths x --candidates {candidates} rows pass the {MAX_ROW_ID} row ids a run can key: split the run")
    os.makedirs(out_dir, exist_ok=True)
    stats = dict(paths=0, rows=0, finished=0, windows=0)
    if selector is not None:
        stats["short_paths"] = 0
    first = 0                                                  # the global id of the group's first path
    for b, f in enumerate(files):
        for group in chunks(read_paths(f), per_chunk):
            shapes = {g[1].shape for g in group}
            if len(shapes) != 1 or len({g[3] for g in group}) != 1:
                raise SystemExit(f"{f}: the terrains of a batch must share their shape and dx")
            if selector is not None:
                pids = first + np.arange(len(group), dtype=np.int64)
                first += len(group)
                stats["paths"] += len(group)
                run_device_select(handle, selector, b, group, pids, candidates, top_k, seed, out_dir, stats, slice_terrain, thresholds, max_attempts)
                continue
            handle.set_scene(np.stack([g[1] for g in group]), np.stack([g[2] for g in group]), group[0][3], [g[4] for g in group], candidates)
            pids = first + np.arange(len(group), dtype=np.int64)
            first += len(group)
            ids = (pids[:, None] * candidates + np.arange(candidates)[None, :]).reshape(-1)
            res = handle.rollout(seed=seed, row_ids=ids, path_ids=pids)
            final = res.final_frame.cpu().numpy()
            stats["paths"] += len(group); stats["rows"] += len(ids); stats["finished"] += int((final >= 0).sum()); stats["windows"] += int(res.windows)
            for g, sel in zip(group, handle.select(res, top_k=top_k, seed=seed + b)):
                write_selection(handle, res, ids, final, b, g, sel, out_dir, False)
    return stats


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--paths", required=True, help="directory of paths_*.npz; their hf is the heightfield the planner searched, used as it is")
    ap.add_argument("--out", required=True)
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--checkpoint")
    src.add_argument("--random_init", type=int, metavar="SEED")
    ap.add_argument("--use_ema_model", action="store_true")
    ap.add_argument("--feature_stats", default=None)
    ap.add_argument("--config", default=os.path.join(REPO, "data/configs/mdm_path/mdm_path_default.yaml"))
    ap.add_argument("--candidates", type=int, default=None, help="rows per path (default: the config's mdm_batch_size)")
    ap.add_argument("--top_k", type=int, default=None)
    ap.add_argument("--max_motion_length", type=float, default=None)
    ap.add_argument("--max_batch", type=int, default=64)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--device_select", action="store_true", help="score, filter and rank on the device (motion_select.PathSelector), on the whole terrain")
    ap.add_argument("--slice_terrain", action="store_true", help="score every row on its own terrain slice and save that slice (implies --device_select)")
    ap.add_argument("--max_contact_loss", type=float, default=None, help="keep rows under it only (reference default 3.0); implies --device_select")
    ap.add_argument("--max_pen_loss", type=float, default=None, help="(reference default 8.0)")
    ap.add_argument("--max_total_loss", type=float, default=None, help="(reference default 30.0)")
    ap.add_argument("--max_attempts", type=int, default=1, help="rollouts of a path with fewer than --top_k valid rows before it is skipped")
    a = ap.parse_args(argv)
    import numpy as np
    from parc_amd import motion_generator as mg
    from parc_amd import motion_path_gen as mpg
    files = sorted(glob.glob(os.path.join(a.paths, "paths_*.npz")))
    if not files:
        raise SystemExit(f"no paths_*.npz in {a.paths}")
    ps, gs, _ = mpg.load_config(a.config)
    if a.max_motion_length is not None:
        ps.max_motion_length = a.max_motion_length
    candidates = int(a.candidates if a.candidates is not None else ps.mdm_batch_size)
    top_k = min(int(a.top_k if a.top_k is not None else ps.top_k), candidates)
    if a.checkpoint:
        gen = mg.MDMGenerator.load_checkpoint(a.checkpoint, a.use_ema_model, a.device, max_batch=a.max_batch, feature_stats=a.feature_stats)
    else:
        from parc_amd.char_model import CharModel
        cfg = mg.default_config()
        cm = CharModel(mg._char_path(cfg))
        D = mg.frame_dim(cm)
        gen = mg.MDMGenerator(cfg, mg.random_state_dict(cfg, a.random_init, cm), np.zeros((cfg["seq_len"], D), np.float32), np.ones((cfg["seq_len"], D), np.float32),
                              a.device, max_batch=a.max_batch)
    handle = mpg.PathMotionGenerator(gen, ps, gs)
    thresholds = dict(max_contact_loss=a.max_contact_loss, max_pen_loss=a.max_pen_loss, max_total_loss=a.max_total_loss)
    selector = None
    if a.device_select or a.slice_terrain or a.max_attempts != 1 or any(v is not None for v in thresholds.values()):
        from parc_amd.motion_select import PathSelector
        selector = PathSelector(handle)
    t0 = time.perf_counter()
    stats = run(handle, files, a.out, candidates, top_k, a.seed, a.max_batch, selector=selector, slice_terrain=a.slice_terrain, max_attempts=a.max_attempts, **thresholds)
    stats["seconds"] = round(time.perf_counter() - t0, 3)
    print(json.dumps(stats))


if __name__ == "__main__":
    main()
