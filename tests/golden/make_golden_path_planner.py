#!/usr/bin/env python3
"""Generate the terrain path planner fixtures (``path_planner_*.npz``) from the REAL reference.

Run where the reference checkout is available (the tests only read the fixtures it writes):

    python tests/golden/make_golden_path_planner.py [case ...]

Drives the reference's own ``construct_navigation_graph``, ``pick_random_start_end_nodes_on_edges``, ``flat_maxpool_2x2``,
``flatten_4x4_near_edge`` and ``run_a_star_on_start_end_nodes`` on random windows of the three bundled terrains, as stage 2's FILE mode
cuts them (``parc_2_kin_gen.py:292-334``).  ``astar.a_star_search`` is wrapped so that the step-cost function is the planner's per-edge
noise (it reads ``from_node`` / ``to_node`` from the caller's frame) and ``max_compute_time`` is effectively infinite.

Every candidate query is also run through the array-based restatement (``tests/path_planner_ref.py``), which reports ``(f, g)`` ties and
the decision margin.  A candidate is KEPT only if it has zero ties and, for ``w_bumpy > 0``, a margin above 1e-5; the restatement must
then agree with the reference exactly (edge sets, nodes, fp32 cost bits, verdict) -- asserted here.  Asserted and written down per file:
at least a third of the queries found and a third not; over all files at least five found paths over a jump edge of three or more
cells, at least four simplified queries with a start / goal index of 0 and four with an index of dim - 1.  Fixtures hold data only.

A case carries its grid ``(X, Y)``, ``dx``, ``dy`` and ``min_point``.  A case whose ``max_cost`` is ``None`` takes it from the reference's
own output: a first pass with the class default lists the costs of the kept found paths, a value just under their median (two decimals)
becomes ``max_cost`` and a second pass with the same draws gives the recorded verdicts; such a file needs at least three FOUND and three
OVER_MAX_COST queries, and its thirds rule counts OVER_MAX_COST with the found paths.  The square files were written before ``dy`` was
stored (readers default it to ``dx``); regenerate single cases by name to leave them as they are.
"""
import json
import os
import random
import sys
import time
import types

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.dont_write_bytecode = True

for _name in ["trimesh", "trimesh.creation", "wandb", "gym", "gym.spaces", "isaacgym", "isaacgym.gymapi", "isaacgym.gymtorch",
              "isaacgym.gymutil"]:
    sys.modules[_name] = types.ModuleType(_name)
sys.modules["wandb"].run = None
sys.modules["trimesh"].creation = sys.modules["trimesh.creation"]
_parc = types.ModuleType("parc")
_parc.__path__ = [os.path.join(REF, "PARC")]
sys.modules["parc"] = _parc

import numpy as np  # noqa: E402
import torch  # noqa: E402

import path_planner_ref as ref  # noqa: E402
from parc_amd import ms_file  # noqa: E402

import parc.motion_synthesis.procgen.astar as astar  # noqa: E402
import parc.util.terrain_util as terrain_util  # noqa: E402

torch.set_num_threads(1)
TERRAINS = ["TEASER_TERRAIN", "civilization", "sfu"]
STAGE2 = dict(ref.DEFAULTS, max_jump_z_diff=0.5, min_jump_z_diff=-1.0, w_bumpy=0.0, uniform_cost_max=0.5, min_start_end_xy_dist=5.0)
DX = 0.4
ORIGIN = (0.0, 0.0)
# (file, (X, Y), dx, dy, min_point, settings, simplify, queries kept, candidates drawn, seed)
CASES = [("default_16", (16, 16), DX, DX, ORIGIN, STAGE2, True, 30, 110, 11),
         ("nosimplify_16", (16, 16), DX, DX, ORIGIN, STAGE2, False, 18, 50, 12),
         ("bumpy_16", (16, 16), DX, DX, ORIGIN, dict(STAGE2, w_bumpy=1.0), True, 18, 50, 13),
         ("classdefaults_16", (16, 16), DX, DX, ORIGIN, dict(ref.DEFAULTS), True, 18, 50, 14),
         ("default_32", (32, 32), DX, DX, ORIGIN, STAGE2, True, 6, 14, 15),
         # off the square: a shifted origin, dx != dy in both orders, jump radii 5 and 3; max_cost None = chosen from the reference's costs
         ("rect_12x20", (12, 20), 0.4, 0.4, (1.7, -2.3),
          dict(STAGE2, min_start_end_xy_dist=3.0, uniform_cost_min=0.1, uniform_cost_max=0.6, max_cost=None), True, 12, 60, 16),
         ("aniso_13x17", (13, 17), 0.4, 0.5, (1.7, -2.3), dict(STAGE2, min_start_end_xy_dist=3.0, max_jump_xy_dist=2.0), True, 12, 60, 17),
         ("aniso_20x11", (20, 11), 0.5, 0.4, (-3.1, 0.9), dict(STAGE2, min_start_end_xy_dist=2.5, max_jump_xy_dist=1.2), True, 12, 60, 18)]

_ctx = {}
_orig_search = astar.a_star_search


def _noise():
    fr = sys._getframe(1)
    a, b = fr.f_locals["from_node"], fr.f_locals["to_node"]
    Y, s = _ctx["Y"], _ctx["settings"]
    return ref.edge_noise(_ctx["seed"], _ctx["query"], int(a.index[0]) * Y + int(a.index[1]), int(b.index[0]) * Y + int(b.index[1]),
                          s["uniform_cost_min"], s["uniform_cost_max"])


def _wrapped_search(*a, **k):
    k["stochastic_step_cost_fn"] = _noise
    k["max_compute_time"] = 1e12
    _ctx["graph"] = k["nav_graph"] = astar.construct_navigation_graph(terrain=a[0], max_z_diff=k["max_z_diff"], max_jump_xy_dist=k["max_jump_xy_dist"],
                                                                     max_jump_z_diff=k["max_jump_z_diff"], min_jump_z_diff=k["min_jump_z_diff"])
    r = _orig_search(*a, **k)
    _ctx["result"] = r
    return r


astar.a_star_search = _wrapped_search


def settings_obj(d):
    s = astar.AStarSettings()
    for k, v in d.items():
        setattr(s, k, v)
    return s


def run_candidate(hf_window, dx, dy, min_point, settings, simplify, seed, query):
    X, Y = hf_window.shape
    terrain = terrain_util.SubTerrain("terrain", x_dim=X, y_dim=Y, dx=dx, dy=dy, min_x=min_point[0], min_y=min_point[1], device="cpu")
    terrain.hf[:, :] = torch.tensor(hf_window)
    start, goal = astar.pick_random_start_end_nodes_on_edges(terrain, min_dist=settings["min_start_end_xy_dist"])
    if simplify:
        terrain_util.flat_maxpool_2x2(terrain=terrain)
        terrain_util.flatten_4x4_near_edge(terrain=terrain, grid_ind=start, height=terrain.hf[start[0], start[1]].item())
        terrain_util.flatten_4x4_near_edge(terrain=terrain, grid_ind=goal, height=terrain.hf[goal[0], goal[1]].item())
    _ctx.update(Y=Y, settings=settings, seed=seed, query=query)
    t0 = time.perf_counter()
    out = astar.run_a_star_on_start_end_nodes(terrain=terrain, start_node=start, end_node=goal, settings=settings_obj(settings))
    seconds = time.perf_counter() - t0
    nodes, cost = _ctx["result"]
    graph = _ctx["graph"]
    edges = [sorted({r * Y + c for r, c in graph[i][j].edges}) for i in range(X) for j in range(Y)]
    if nodes is None:
        status = ref.NO_PATH
    else:
        status = ref.FOUND if out is not False else ref.OVER_MAX_COST
    s, g = tuple(int(v) for v in start), tuple(int(v) for v in goal)
    hf_s = terrain.hf.numpy().astype(np.float32).copy()
    dxf, dyf = float(terrain.dxdy[0].item()), float(terrain.dxdy[1].item())
    origin = terrain.min_point.numpy().astype(np.float32).copy()
    # the restatement: simplification, graph, search, polyline
    mine_hf = ref.simplify(hf_window, s, g) if simplify else hf_window
    assert mine_hf.tobytes() == hf_s.tobytes(), "simplified heightfield differs"
    gr = ref.build_graph(hf_s, dxf, dyf, origin, settings)
    assert ref.edge_sets(gr[0], gr[1]) == edges, "edge sets differ"
    mine = ref.search(hf_s, dxf, dyf, origin, s, g, settings, seed, query, graph=gr)
    keep = mine["ties"] == 0 and (settings["w_bumpy"] == 0.0 or mine["margin"] > 1e-5)
    rec = dict(hf=hf_window, hf_s=hf_s, start=s, goal=g, edges=edges, status=status, seconds=seconds, pops=mine["pops"], margin=mine["margin"],
               nodes=[], cost=np.float32(np.nan), points=np.zeros((0, 3), np.float32), keep=keep, jump=0)
    if nodes is not None:
        rec["nodes"] = [(int(n[0]), int(n[1])) for n in nodes]
        rec["cost"] = np.float32(cost)
        rec["jump"] = max([max(abs(a[0] - b[0]), abs(a[1] - b[1])) for a, b in zip(rec["nodes"][:-1], rec["nodes"][1:])] or [0])
    if status == ref.FOUND:
        rec["points"] = out.numpy().astype(np.float32)
    if keep:
        assert mine["status"] == status, (mine["status"], status)
        if nodes is not None:
            assert mine["nodes"] == rec["nodes"], "node sequence differs"
            if settings["w_bumpy"] == 0.0:
                assert np.float32(mine["cost"]).tobytes() == rec["cost"].tobytes(), "cost bits differ"
            else:
                assert abs(float(mine["cost"]) - float(cost)) <= 1e-5
        if status == ref.FOUND:
            p = ref.polyline(hf_s, dxf, dyf, origin, rec["nodes"])
            assert p.shape == rec["points"].shape and np.abs(p - rec["points"]).max() <= 2e-6, "polyline differs"
    return rec


def on_last(c, shape):
    """A start / goal index of dim - 1 on its own axis."""
    return any(cell[a] == shape[a] - 1 for cell in (c["start"], c["goal"]) for a in (0, 1))


def select(cands, n, simplify, shape, classes=((ref.FOUND,), (ref.NO_PATH, ref.OVER_MAX_COST))):
    """n kept candidates: edge-index and long-jump queries first, then the status classes (found / not found) in turn."""
    pool = [c for c in cands if c["keep"]]
    edge0 = [c for c in pool if 0 in c["start"] + c["goal"]]
    edge1 = [c for c in pool if on_last(c, shape)]
    longj = [c for c in pool if c["status"] == ref.FOUND and c["jump"] >= 3]
    chosen = []

    def take(lst, k):
        for c in lst:
            if k <= 0:
                break
            if not any(c is d for d in chosen):
                chosen.append(c)
                k -= 1

    if simplify:
        take(edge0, min(3, n // 6))
        take(edge1, min(3, n // 6))
    take(longj, min(max(2, n // 5), n // 3))
    groups = [[c for c in pool if c["status"] in cls] for cls in classes]
    while len(chosen) < n:
        counts = [sum(c["status"] in cls for c in chosen) for cls in classes]
        before = len(chosen)
        take(groups[counts.index(min(counts))], 1)          # the class with the fewest so far, the first of equals
        if len(chosen) == before:
            take(pool, 1)
        assert len(chosen) > before, "not enough kept candidates"
    return chosen[:n]


def main():
    terrains = {n: np.asarray(ms_file.load_ms_file(os.path.join(REPO, "data/motion_terrains", n + ".pkl"), load_misc=False).terrain_data.hf, np.float32)
                for n in TERRAINS}
    totals = dict(long_jump=0, edge0=0, edge1=0)
    only = sys.argv[1:]
    for name, shape, dx, dy, min_point, settings, simplify, keep_n, draw_n, seed in CASES:
        if only and name not in only:
            continue
        X, Y = shape
        auto_cost = settings["max_cost"] is None

        def draw_all(settings):
            # the same windows and the same start / goal draws on every pass: both generators restart from the case's seed
            random.seed(seed)
            rng = np.random.RandomState(seed)
            cands = []
            for k in range(draw_n):
                tname = TERRAINS[k % 3]
                T = terrains[tname]
                sx = rng.randint(0, T.shape[0] + 1 - X)
                sy = rng.randint(0, T.shape[1] + 1 - Y)
                rec = run_candidate(T[sx:sx + X, sy:sy + Y].copy(), dx, dy, min_point, settings, simplify, seed, k)
                rec.update(terrain=tname, origin=(sx, sy), query=k)
                cands.append(rec)
                print(name, k, tname, "status", rec["status"], "cost", rec["cost"], "jump", rec["jump"], "pops", rec["pops"], "keep", rec["keep"],
                      f"{rec['seconds']:.2f}s", flush=True)
            return cands

        classes = ((ref.FOUND,), (ref.NO_PATH, ref.OVER_MAX_COST))
        if auto_cost:
            first = draw_all(dict(settings, max_cost=ref.DEFAULTS["max_cost"]))
            costs = sorted(float(c["cost"]) for c in first if c["keep"] and c["status"] == ref.FOUND)
            settings = dict(settings, max_cost=round(costs[len(costs) // 2] - 0.005, 2))     # below the median: it is no path's own cost
            print(name, "found costs", costs[0], "..", costs[-1], "max_cost", settings["max_cost"], flush=True)
            classes = ((ref.FOUND,), (ref.OVER_MAX_COST,), (ref.NO_PATH,))
        cands = draw_all(settings)
        ch = select(cands, keep_n, simplify, shape, classes)
        nf = sum(c["status"] == ref.FOUND for c in ch)
        reached = nf + (sum(c["status"] == ref.OVER_MAX_COST for c in ch) if auto_cost else 0)
        assert 3 * reached >= len(ch) and 3 * (len(ch) - reached) >= len(ch), (name, reached, len(ch))
        assert not auto_cost or (nf >= 3 and reached - nf >= 3), (name, nf, reached)
        totals["long_jump"] += sum(c["status"] == ref.FOUND and c["jump"] >= 3 for c in ch)
        if simplify:
            totals["edge0"] += sum(0 in c["start"] + c["goal"] for c in ch)
            totals["edge1"] += sum(on_last(c, shape) for c in ch)
        edge_off, edge_to, node_off, nodes, point_off, points = [0], [], [0], [], [0], []
        for c in ch:
            for e in c["edges"]:
                edge_to.extend(e)
                edge_off.append(len(edge_to))
            nodes.extend(c["nodes"])
            node_off.append(len(nodes))
            points.append(c["points"])
            point_off.append(point_off[-1] + len(c["points"]))
        notes = dict(kept=len(ch), drawn=draw_n, dropped_for_ties_or_margin=sum(not c["keep"] for c in cands), found=nf,
                     min_margin=min(c["margin"] for c in ch), zero_ties=True,
                     long_jump_paths=int(sum(c["status"] == ref.FOUND and c["jump"] >= 3 for c in ch)), max_cost=settings["max_cost"])
        if auto_cost:
            notes.update(over_max_cost=int(reached - nf), found_costs_first_pass=[costs[0], costs[-1]])
        np.savez_compressed(
            os.path.join(HERE, f"path_planner_{name}.npz"),
            settings=json.dumps(settings), notes=json.dumps(notes), simplify=np.int32(simplify), seed=np.int64(seed), dx=np.float32(dx),
            dy=np.float32(dy), min_point=np.array(min_point, np.float32), terrain=np.array([c["terrain"] for c in ch]), origin=np.array([c["origin"] for c in ch], np.int32),
            query=np.array([c["query"] for c in ch], np.int64), hf=np.stack([c["hf"] for c in ch]), hf_simplified=np.stack([c["hf_s"] for c in ch]),
            start=np.array([c["start"] for c in ch], np.int32), goal=np.array([c["goal"] for c in ch], np.int32),
            edge_off=np.array(edge_off, np.int64), edge_to=np.array(edge_to, np.int16), status=np.array([c["status"] for c in ch], np.int32),
            cost=np.array([c["cost"] for c in ch], np.float32), node_off=np.array(node_off, np.int64),
            nodes=np.array(nodes, np.int32).reshape(-1, 2), point_off=np.array(point_off, np.int64),
            points=np.concatenate(points).astype(np.float32), pops=np.array([c["pops"] for c in ch], np.int32),
            margin=np.array([c["margin"] for c in ch], np.float64), ref_seconds=np.array([c["seconds"] for c in ch], np.float64))
        print(name, notes, flush=True)
    print(totals)
    assert only or (totals["long_jump"] >= 5 and totals["edge0"] >= 4 and totals["edge1"] >= 4), totals


if __name__ == "__main__":
    main()
