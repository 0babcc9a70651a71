"""Terrain path planner, host side (no GPU): the numpy restatement against the reference fixtures, the settings, the ctypes mirrors and
``plan_terrains``' selection rule."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import yaml

import path_planner_ref as ref
from parc_amd import path_planner as pp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SQUARE_CASES = ["default_16", "nosimplify_16", "bumpy_16", "classdefaults_16", "default_32"]
CASES = SQUARE_CASES + ["rect_12x20", "aniso_13x17", "aniso_20x11"]


def fixture(case):
    z = dict(np.load(os.path.join(REPO, "tests/golden", f"path_planner_{case}.npz")))
    z["settings"] = json.loads(str(z["settings"]))
    z["notes"] = json.loads(str(z["notes"]))
    z.setdefault("dy", z["dx"])                  # the square fixtures were written before dy was stored
    return z


def fixture_edges(z, k):
    """Per cell the sorted edge targets of query k."""
    N = z["hf"].shape[1] * z["hf"].shape[2]
    off = z["edge_off"][k * N:(k + 1) * N + 1]
    return [z["edge_to"][off[c]:off[c + 1]].astype(np.int64).tolist() for c in range(N)]


@pytest.mark.parametrize("case", CASES)
def test_restatement_matches_reference(case):
    z = fixture(case)
    s = z["settings"]
    dx, dy = float(z["dx"]), float(z["dy"])
    seed = int(z["seed"])
    for k in range(z["hf"].shape[0]):
        start, goal = tuple(int(v) for v in z["start"][k]), tuple(int(v) for v in z["goal"][k])
        hf = ref.simplify(z["hf"][k], start, goal) if int(z["simplify"]) else z["hf"][k]
        assert hf.tobytes() == z["hf_simplified"][k].tobytes()
        graph = ref.build_graph(hf, dx, dy, z["min_point"], s)
        assert ref.edge_sets(graph[0], graph[1]) == fixture_edges(z, k)
        r = ref.search(hf, dx, dy, z["min_point"], start, goal, s, seed, int(z["query"][k]), graph=graph)
        assert r["ties"] == 0 and r["pops"] == z["pops"][k]
        assert r["status"] == z["status"][k]
        want = z["nodes"][z["node_off"][k]:z["node_off"][k + 1]]
        assert [tuple(n) for n in want.tolist()] == r["nodes"]
        if len(want):
            if s["w_bumpy"] == 0.0:
                assert np.float32(r["cost"]).tobytes() == z["cost"][k].tobytes()
            else:
                assert r["margin"] > 1e-5 and abs(float(r["cost"]) - float(z["cost"][k])) <= 1e-5
        if r["status"] == ref.FOUND:
            pts = ref.polyline(hf, dx, dy, z["min_point"], r["nodes"])
            want_p = z["points"][z["point_off"][k]:z["point_off"][k + 1]]
            assert pts.shape == want_p.shape and np.abs(pts - want_p).max() <= 2e-6


def test_fixture_conditions():
    """What the generator asserted, re-checked on the committed files: found / not found thirds, long jumps, edge-index cells.  The
    totals count the square files alone, as before the rectangular ones came; those are checked file by file below."""
    long_jump = edge0 = edge1 = found = total = 0
    for case in SQUARE_CASES:
        z = fixture(case)
        dim = z["hf"].shape[1]
        assert z["hf"].shape[2] == dim and float(z["dy"]) == float(z["dx"]) and not z["min_point"].any()
        ok = z["status"] == ref.FOUND
        found += ok.sum()
        total += len(ok)
        for k in range(len(ok)):
            n = z["nodes"][z["node_off"][k]:z["node_off"][k + 1]]
            if ok[k] and np.abs(np.diff(n, axis=0)).max() >= 3:
                long_jump += 1
            if int(z["simplify"]):
                sg = np.concatenate([z["start"][k], z["goal"][k]])
                edge0 += (sg == 0).any()
                edge1 += (sg == dim - 1).any()
        assert z["notes"]["zero_ties"] and (z["settings"]["w_bumpy"] == 0.0 or z["margin"].min() > 1e-5)
    assert 3 * found >= total and 3 * (total - found) >= total
    assert long_jump >= 5 and edge0 >= 4 and edge1 >= 4


@pytest.mark.parametrize("case,shape,dx,dy,min_point,radius", [("rect_12x20", (12, 20), 0.4, 0.4, (1.7, -2.3), 8),
                                                               ("aniso_13x17", (13, 17), 0.4, 0.5, (1.7, -2.3), 5),
                                                               ("aniso_20x11", (20, 11), 0.5, 0.4, (-3.1, 0.9), 3)])
def test_rectangular_fixture_conditions(case, shape, dx, dy, min_point, radius):
    """The files off the square: 12 queries at the stated grid, spacing, origin and jump radius, a third reached the goal and a third
    did not, zero ties; rect_12x20's max_cost (chosen from the reference's costs) leaves at least three FOUND and three OVER_MAX_COST."""
    z = fixture(case)
    s, notes = z["settings"], z["notes"]
    assert z["hf"].shape == (12,) + shape and int(z["simplify"]) == 1
    assert (np.float32(z["dx"]), np.float32(z["dy"])) == (np.float32(dx), np.float32(dy)) and z["min_point"].tobytes() == np.array(min_point, np.float32).tobytes()
    assert ref.jump_radius(s, float(z["dx"])) == radius
    assert notes["zero_ties"] and notes["kept"] == 12 and notes["drawn"] >= 12 and "dropped_for_ties_or_margin" in notes and "min_margin" in notes
    assert notes["max_cost"] == s["max_cost"]
    found, over = int((z["status"] == ref.FOUND).sum()), int((z["status"] == ref.OVER_MAX_COST).sum())
    if case == "rect_12x20":
        assert notes["max_cost"] == s["max_cost"] < 1000.0 and found >= 3 and over >= 3 and (s["uniform_cost_min"], s["uniform_cost_max"]) == (0.1, 0.6)
        assert 3 * (found + over) >= 12 and 3 * (12 - found - over) >= 12
        for k in range(12):
            if len(z["nodes"][z["node_off"][k]:z["node_off"][k + 1]]):
                assert (z["status"][k] == ref.OVER_MAX_COST) == bool(z["cost"][k] > np.float32(s["max_cost"]))
                assert (z["point_off"][k + 1] > z["point_off"][k]) == (z["status"][k] == ref.FOUND)
    else:
        assert over == 0 and 3 * found >= 12 and 3 * (12 - found) >= 12


def test_ring_cells_include_outermost_rows():
    cells = ref.ring_cells(16, 16)
    assert len(cells) == 4 * 16 + 12 * 4 and (0, 1) in cells and (15, 14) in cells and (0, 0) not in cells and (5, 5) not in cells


def test_flatten_slices_follow_python():
    """An even index 0 gives the empty slice(-2, 2); an index of dim - 1 gives a block cut at the grid's end."""
    hf = np.arange(256, dtype=np.float32).reshape(16, 16)
    out = ref.simplify(hf, (0, 2), (15, 13))
    pooled = np.repeat(np.repeat(hf.reshape(8, 2, 8, 2).max(axis=(1, 3)), 2, axis=0), 2, axis=1)
    want = pooled.copy()
    want[14:16, 12:16] = pooled[15, 13]                                    # start (0, 2): no write at all; goal: rows 14, 15 only
    assert np.array_equal(out, want)


def test_settings_defaults_and_yaml_round_trip(tmp_path):
    assert pp.AStarSettings().to_config() == ref.DEFAULTS
    cfg = pp.PlannerConfig.load(os.path.join(REPO, "data/configs/path_planner/path_planner_default.yaml"))
    a = cfg.astar
    assert (a.max_jump_z_diff, a.min_jump_z_diff, a.w_bumpy, a.uniform_cost_max, a.min_start_end_xy_dist) == (0.5, -1.0, 0.0, 0.5, 5.0)
    assert (a.max_z_diff, a.max_jump_xy_dist, a.w_z, a.w_xy, a.max_bumpy, a.uniform_cost_min, a.max_cost) == (2.1, 3.0, 0.15, 1.0, 0.2, 0.0, 1000.0)
    assert cfg.simplify_terrain is True and cfg.num_attempts == 10 and (cfg.new_terrain_dim_x, cfg.new_terrain_dim_y, cfg.dx) == (16, 16, 0.4)
    path = tmp_path / "planner.yaml"
    path.write_text(yaml.safe_dump(cfg.to_dict()))
    assert pp.PlannerConfig.load(path) == cfg
    with pytest.raises(ValueError, match="max_jump"):
        pp.AStarSettings.from_config({"max_jump": 1.0})
    assert pp.jump_radius(a, 0.4) == 8


def test_ctypes_mirrors_and_struct_size_refusal():
    from parc_amd import lib as L
    assert C.sizeof(L.ParcPathPlanParams) == 8 * 4 + 12 * 8 + 4 * 4       # 8 words, 12 doubles, 4 ints
    assert L.ParcPathPlanParams.max_z_diff.offset == 32 and L.ParcPathPlanParams.simplify_terrain.offset == 128
    assert C.sizeof(L.ParcPathPlanOutputs) == 8 * 10
    assert [n for n, _ in L.PATHPLAN_OUTPUT_FIELDS] == ["status", "cost", "num_nodes", "nodes", "num_points", "points", "start", "goal", "hf", "pops"]
    assert list(L.PATHPLAN_SETTINGS) == list(ref.DEFAULTS)
    assert (L.PATHPLAN_MAX_DIM, L.PATHPLAN_MAX_JUMP_RADIUS, L.PATHPLAN_JUMP_WORDS) == (pp.MAX_DIM, pp.MAX_JUMP_RADIUS, pp.JUMP_WORDS)
    assert tuple(L.PATHPLAN_STATUS) == pp.STATUS_NAMES and (pp.FOUND, pp.NO_PATH, pp.OVER_MAX_COST, pp.BUDGET) == (ref.FOUND, ref.NO_PATH, ref.OVER_MAX_COST, ref.BUDGET)
    hdr = open(os.path.join(REPO, "include/parc_env.h")).read()
    for name, val in [("PARC_PATHPLAN_MAX_DIM", 64), ("PARC_PATHPLAN_MAX_JUMP_RADIUS", 8), ("PARC_PATHPLAN_JUMP_WORDS", 8), ("PARC_PATHPLAN_FOUND", 0),
                      ("PARC_PATHPLAN_NO_PATH", 1), ("PARC_PATHPLAN_OVER_MAX_COST", 2), ("PARC_PATHPLAN_BUDGET", 3), ("PARC_PATHPLAN_NO_DRAW", 4)]:
        assert f"#define {name} {val} " in hdr or f"#define {name} {val}\n" in hdr
    assert "#define PARC_ABI_VERSION 6" in hdr and L.ABI_VERSION == 6
    for sym in ("parc_pathplan_create", "parc_pathplan_destroy", "parc_pathplan_run", "parc_pathplan_get_graph", "parc_pathplan_kernel_times"):
        assert sym in L.EXPORTED_SYMBOLS and f" {sym}(" in hdr
    # refused before the device is touched: this passes on a machine without a GPU
    lib = L.load()
    p = pp.planner_params(pp.AStarSettings(), 16, 16, 0.4, 0.4)
    p.struct_size -= 8
    h = C.c_void_p()
    with pytest.raises(L.ParcError, match=r"ParcPathPlanParams ABI mismatch \(struct_size\)"):
        L.check(lib.parc_pathplan_create(C.byref(p), C.byref(h)))
    p = pp.planner_params(pp.AStarSettings(), 65, 16, 0.4, 0.4)
    with pytest.raises(L.ParcError, match="PARC_PATHPLAN_MAX_DIM"):
        L.check(lib.parc_pathplan_create(C.byref(p), C.byref(h)))
    p = pp.planner_params(pp.AStarSettings(max_jump_xy_dist=3.3), 16, 16, 0.4, 0.4)
    with pytest.raises(L.ParcError, match="radius of 9 cells, above the limit of 8"):
        L.check(lib.parc_pathplan_create(C.byref(p), C.byref(h)))


def test_first_success_selection():
    F, N, O, B = pp.FOUND, pp.NO_PATH, pp.OVER_MAX_COST, pp.BUDGET
    status = np.array([[N, N, F, F], [F, N, N, N], [N, O, B, N], [O, B, N, F]]).reshape(-1)
    assert pp.select_first_success(status, 4, 4).tolist() == [2, 0, -1, 3]


def test_edges_from_graph_expands_bits():
    nbr = np.zeros((16, 16), np.uint8)
    jump = np.zeros((16, 16, pp.JUMP_WORDS), np.uint32)
    nbr[3, 4] = 0b10000001                       # (-1, 0) and (1, 1)
    k = (5 - (3 - 8)) * 16 + (9 - (4 - 8))       # the window bit of (3, 4) -> (5, 9) at radius 8
    jump[3, 4, k >> 5] = 1 << (k & 31)
    e = pp.edges_from_graph(nbr, jump, 8)
    assert e[3 * 16 + 4] == sorted([2 * 16 + 4, 4 * 16 + 5, 5 * 16 + 9]) and sum(len(x) for x in e) == 3
