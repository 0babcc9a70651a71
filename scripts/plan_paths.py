#!/usr/bin/env python3
"""Stage 2's FILE procgen mode without the generator: N random ``dim_x x dim_y`` windows of an input terrain file
(``parc_2_kin_gen.py:292-304``), start / goal drawn near the border, terrain simplified, path planned -- the whole batch on the GPU
(``parc_amd/path_planner.py``).  Writes one ``.npz`` per batch and prints a one-line summary.

    python scripts/plan_paths.py --terrain data/motion_terrains/TEASER_TERRAIN.pkl --num_terrains 1024 --out output/paths

Per batch file: ``hf`` the (simplified) terrains, ``min_point_offset`` each window's min point in the source terrain, ``start`` / ``goal``,
``status`` (0 = found), ``attempt`` (the winning start / goal draw, -1 = none of ``num_attempts`` succeeded), ``cost``, and the node
lists / polylines concatenated with ``node_off`` / ``point_off`` offsets.

``--procgen_mode BOXES | PATHS | STAIRS`` invents the terrains instead (``parc_2_kin_gen.py:260-290``; ``parc_amd/terrain_gen.py``, DESIGN.md
section 8h) at the config's ``new_terrain_dim_x x new_terrain_dim_y``, ``dx``; a terrain on which none of the ``num_attempts`` draws found a
path is generated again with the next round's seed, up to ``--max_terrain_rounds`` (the reference's outer ``terrain_attempt`` loop, run
wide).  The batch file then also holds ``terrain_round`` (the round whose terrain is stored) and ``min_point_offset`` is zeros.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from parc_amd import ms_file  # noqa: E402
from parc_amd import path_planner as pp  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cut_windows(hf, min_point, dx, n, dim_x, dim_y, rng):
    """np.random.randint(0, dims + 1 - dim) per axis; the window's min point is input_terrain.get_point(start cell)."""
    sx = rng.randint(0, hf.shape[0] + 1 - dim_x, size=n)
    sy = rng.randint(0, hf.shape[1] + 1 - dim_y, size=n)
    wins = np.stack([hf[a:a + dim_x, b:b + dim_y] for a, b in zip(sx, sy)]).astype(np.float32)
    off = np.asarray(min_point, np.float32) + np.stack([sx, sy], axis=1).astype(np.float32) * np.float32(dx)
    return wins, off.astype(np.float32)


def plan_generated(planner, gen, cfg, n, seed, max_rounds):
    """Terrains from ``gen`` planned with ``plan_terrains``; the ones without a path are regenerated (round r uses seed + r), at most
    ``max_rounds`` rounds.  Returns (attempt, PathPlan of the n terrains, terrain_round [n], queries run)."""
    hfs = gen.generate(n, seed).cpu().numpy()
    attempt, plan = planner.plan_terrains(hfs, num_attempts=cfg.num_attempts, seed=seed, dx=cfg.dx, dy=cfg.dy)
    rounds = np.zeros(n, np.int32)
    queries = n * cfg.num_attempts
    for r in range(1, max_rounds):
        todo = np.flatnonzero(attempt < 0)
        if not len(todo):
            break
        # terrain t of round r is terrain (seed + r, t): the same terrain whichever other terrains are regenerated with it
        new = gen.generate(n, seed + r).cpu().numpy()[todo]
        a2, p2 = planner.plan_terrains(new, num_attempts=cfg.num_attempts, seed=seed + r, dx=cfg.dx, dy=cfg.dy)
        queries += len(todo) * cfg.num_attempts
        rounds[todo] = r
        attempt[todo] = a2
        for k, t in enumerate(todo):
            plan.nodes[t], plan.points[t] = p2.nodes[k], p2.points[k]
        for name in ("status", "cost", "start", "goal", "hf", "pops"):
            getattr(plan, name)[todo] = getattr(p2, name)
    return attempt, plan, rounds, queries


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--terrain", default=os.path.join(REPO, "data/motion_terrains/TEASER_TERRAIN.pkl"))
    ap.add_argument("--config", default=os.path.join(REPO, "data/configs/path_planner/path_planner_default.yaml"))
    ap.add_argument("--num_terrains", type=int, default=1024, help="terrains per batch")
    ap.add_argument("--num_batches", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default="output/paths")
    ap.add_argument("--procgen_mode", choices=["FILE", "BOXES", "PATHS", "STAIRS"], default="FILE",
                    help="FILE cuts windows out of --terrain; the others generate the terrains on the GPU")
    ap.add_argument("--terrain_config", default=os.path.join(REPO, "data/configs/terrain_gen/terrain_gen_default.yaml"),
                    help="the boxes / paths / stairs settings of the generated modes")
    ap.add_argument("--max_terrain_rounds", type=int, default=3, help="generated modes: rounds of regenerating the terrains without a path")
    args = ap.parse_args()
    cfg = pp.PlannerConfig.load(args.config)
    if args.procgen_mode != "FILE":
        return main_generated(args, cfg)
    td = ms_file.load_ms_file(args.terrain, load_misc=False).terrain_data
    hf = np.asarray(td.hf, np.float32)
    if hf.shape[0] < cfg.new_terrain_dim_x or hf.shape[1] < cfg.new_terrain_dim_y:
        raise SystemExit(f"{args.terrain} is {hf.shape[0]} x {hf.shape[1]} cells, smaller than the {cfg.new_terrain_dim_x} x {cfg.new_terrain_dim_y} window")
    if abs(float(td.dx) - cfg.dx) > 1e-6:
        raise SystemExit(f"{args.terrain} has dx = {td.dx}, the config plans at dx = {cfg.dx}")
    os.makedirs(args.out, exist_ok=True)
    planner = pp.TerrainPathPlanner(args.device, cfg.astar, simplify_terrain=cfg.simplify_terrain, max_expansions=cfg.max_expansions)
    rng = np.random.RandomState(args.seed)
    found = total = queries = 0
    seconds = 0.0
    for b in range(args.num_batches):
        wins, off = cut_windows(hf, td.min_point, td.dx, args.num_terrains, cfg.new_terrain_dim_x, cfg.new_terrain_dim_y, rng)
        t0 = time.perf_counter()
        attempt, plan = planner.plan_terrains(wins, num_attempts=cfg.num_attempts, seed=args.seed * 1000003 + b, dx=cfg.dx, dy=cfg.dy)
        seconds += time.perf_counter() - t0
        ok = attempt >= 0
        nodes = [n if k else n[:0] for n, k in zip(plan.nodes, ok)]
        points = [p if k else p[:0] for p, k in zip(plan.points, ok)]
        np.savez_compressed(os.path.join(args.out, f"paths_{b:04d}.npz"), hf=plan.hf, min_point_offset=off, dx=np.float32(cfg.dx), start=plan.start,
                            goal=plan.goal, status=plan.status, attempt=attempt, cost=plan.cost, nodes=np.concatenate(nodes).astype(np.int32),
                            node_off=np.concatenate([[0], np.cumsum([len(n) for n in nodes])]).astype(np.int64), points=np.concatenate(points),
                            point_off=np.concatenate([[0], np.cumsum([len(p) for p in points])]).astype(np.int64), config=json.dumps(cfg.to_dict()))
        found += int(ok.sum())
        total += len(ok)
        queries += len(ok) * cfg.num_attempts
    print(json.dumps({"terrains": total, "found": found, "queries": queries, "queries_per_s": round(queries / seconds, 1), "out": args.out}))


def main_generated(args, cfg):
    from parc_amd import terrain_gen as tg
    if args.max_terrain_rounds < 1:
        raise SystemExit("--max_terrain_rounds must be >= 1")
    tcfg = tg.TerrainGenConfig.load(args.terrain_config)
    os.makedirs(args.out, exist_ok=True)
    gen = tg.TerrainGenerator(args.procgen_mode, cfg.new_terrain_dim_x, cfg.new_terrain_dim_y, cfg.dx, cfg.dy, settings=tcfg.settings(args.procgen_mode),
                              device=args.device)
    planner = pp.TerrainPathPlanner(args.device, cfg.astar, simplify_terrain=cfg.simplify_terrain, max_expansions=cfg.max_expansions)
    found = total = queries = 0
    seconds = 0.0
    for b in range(args.num_batches):
        t0 = time.perf_counter()
        attempt, plan, rounds, q = plan_generated(planner, gen, cfg, args.num_terrains, (args.seed * 1000003 + b) * args.max_terrain_rounds,
                                                  args.max_terrain_rounds)
        seconds += time.perf_counter() - t0
        ok = attempt >= 0
        nodes = [n if k else n[:0] for n, k in zip(plan.nodes, ok)]
        points = [p if k else p[:0] for p, k in zip(plan.points, ok)]
        np.savez_compressed(os.path.join(args.out, f"paths_{b:04d}.npz"), hf=plan.hf, min_point_offset=np.zeros((len(ok), 2), np.float32),
                            dx=np.float32(cfg.dx), start=plan.start, goal=plan.goal, status=plan.status, attempt=attempt, cost=plan.cost,
                            nodes=np.concatenate(nodes).astype(np.int32),
                            node_off=np.concatenate([[0], np.cumsum([len(n) for n in nodes])]).astype(np.int64), points=np.concatenate(points),
                            point_off=np.concatenate([[0], np.cumsum([len(p) for p in points])]).astype(np.int64), terrain_round=rounds,
                            procgen_mode=args.procgen_mode, config=json.dumps(cfg.to_dict()), terrain_config=json.dumps(tcfg.to_dict()))
        found += int(ok.sum())
        total += len(ok)
        queries += q
    print(json.dumps({"procgen_mode": args.procgen_mode, "terrains": total, "found": found, "queries": queries,
                      "queries_per_s": round(queries / seconds, 1), "out": args.out}))


if __name__ == "__main__":
    main()
