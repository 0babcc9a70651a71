"""Terrain path planner on the GPU (parc_pathplan_*): the reference fixtures through the C-ABI, the device draws, and
properties of 16 384-query batches.

Bars: simplified heightfield, graph edge sets, status, node lists exact for every query; cost bit for bit with ``w_bumpy = 0`` and to
1e-5 with ``w_bumpy > 0`` (the fixtures' decision margins exceed 1e-5); point counts exact, coordinates 2e-6."""
import ctypes as C
import os

import numpy as np
import pytest

import path_planner_ref as ref
from parc_amd import path_planner as pp
from test_path_planner_cpu import CASES, REPO, fixture, fixture_edges

pytestmark = pytest.mark.gpu
STAGE2 = dict(ref.DEFAULTS, max_jump_z_diff=0.5, min_jump_z_diff=-1.0, w_bumpy=0.0, uniform_cost_max=0.5, min_start_end_xy_dist=5.0)


def planner(settings, simplify, **kw):
    return pp.TerrainPathPlanner("cuda:0", pp.AStarSettings(**settings), simplify_terrain=simplify, **kw)


@pytest.mark.parametrize("case", CASES)
def test_fixture_through_the_c_abi(case):
    z = fixture(case)
    s = z["settings"]
    dx, dy = float(z["dx"]), float(z["dy"])
    P = planner(s, bool(int(z["simplify"])), min_point=tuple(float(v) for v in z["min_point"]))
    R = pp.jump_radius(P.settings, dx)
    Y = z["hf"].shape[2]
    for k in range(z["hf"].shape[0]):
        # a fixture's queries keep the indices the generator drew them under: one query per run, first_query = its index
        r = P.plan(z["hf"][k:k + 1], z["start"][k:k + 1], z["goal"][k:k + 1], seed=int(z["seed"]), dx=dx, dy=dy, first_query=int(z["query"][k]))
        assert r.hf[0].tobytes() == z["hf_simplified"][k].tobytes(), (case, k)
        nbr, cliff, jump = P.graph(0, 1)
        assert pp.edges_from_graph(nbr[0], jump[0], R) == fixture_edges(z, k), (case, k)
        want_nodes = z["nodes"][z["node_off"][k]:z["node_off"][k + 1]]
        print(case, k, "status", r.status[0], z["status"][k], "cost", r.cost[0], z["cost"][k], "pops", r.pops[0], z["pops"][k])
        assert r.status[0] == z["status"][k], (case, k)
        assert np.array_equal(r.nodes[0], want_nodes), (case, k)
        assert r.pops[0] == z["pops"][k], (case, k)
        assert np.array_equal(r.start[0], z["start"][k]) and np.array_equal(r.goal[0], z["goal"][k])
        if len(want_nodes):
            if s["w_bumpy"] == 0.0:
                assert r.cost[0].tobytes() == z["cost"][k].tobytes(), (case, k)
            else:
                assert abs(float(r.cost[0]) - float(z["cost"][k])) <= 1e-5, (case, k)
        else:
            assert np.isnan(r.cost[0])
        want_p = z["points"][z["point_off"][k]:z["point_off"][k + 1]]
        assert r.points[0].shape == want_p.shape, (case, k)
        if len(want_p):
            assert np.abs(r.points[0] - want_p).max() <= 2e-6, (case, k)


def terrain_windows(n, dim, seed):
    from parc_amd import ms_file
    rng = np.random.RandomState(seed)
    ts = [np.asarray(ms_file.load_ms_file(os.path.join(REPO, "data/motion_terrains", t + ".pkl"), load_misc=False).terrain_data.hf, np.float32)
          for t in ("TEASER_TERRAIN", "civilization", "sfu")]
    out = np.zeros((n, dim, dim), np.float32)
    for k in range(n):
        T = ts[k % 3]
        sx, sy = rng.randint(0, T.shape[0] + 1 - dim), rng.randint(0, T.shape[1] + 1 - dim)
        out[k] = T[sx:sx + dim, sy:sy + dim]
    return out


def test_device_draws():
    """Every start / goal on the ring and far enough apart; the restatement's draws; chi-squared of the start cells over 65 536 draws with
    min_dist = 0 (112 candidates, 111 degrees of freedom, survival 1e-4 for this fixed seed); seeds."""
    hfs = np.zeros((4096, 16, 16), np.float32)
    P = planner(STAGE2, True)
    a = P.plan(hfs, seed=7)
    ring = set(ref.ring_cells(16, 16))
    assert (a.status != pp.NO_DRAW).all()
    assert all(tuple(c) in ring for c in a.start.tolist()) and all(tuple(c) in ring for c in a.goal.tolist())
    d = np.sqrt((((a.start - a.goal).astype(np.float64) * float(np.float32(0.4))) ** 2).sum(axis=1))
    assert d.min() >= 5.0 - 1e-4 - 1e-6
    for q in range(0, 4096, 97):
        s, g = ref.draw_start_goal(7, q, 16, 16, 0.4, 0.4, (0.0, 0.0), 5.0)
        assert tuple(a.start[q]) == s and tuple(a.goal[q]) == g
    b = P.plan(hfs, seed=7)
    assert np.array_equal(a.start, b.start) and np.array_equal(a.goal, b.goal) and a.cost.tobytes() == b.cost.tobytes()
    c = P.plan(hfs, seed=8)
    assert (c.start != a.start).any(axis=1).mean() > 0.9
    shifted = P.plan(hfs[:64], seed=7, first_query=1000)
    assert np.array_equal(shifted.start, a.start[1000:1064]) and np.array_equal(shifted.goal, a.goal[1000:1064])
    P0 = planner(dict(STAGE2, min_start_end_xy_dist=0.0), False)
    n = 65536
    u = P0.plan(np.zeros((n, 16, 16), np.float32), seed=2024)
    cells = ref.ring_cells(16, 16)
    index = {c: i for i, c in enumerate(cells)}
    for name, arr in (("start", u.start), ("goal", u.goal)):
        cnt = np.bincount([index[tuple(c)] for c in arr.tolist()], minlength=len(cells)).astype(np.float64)
        chi = float(((cnt - n / len(cells)) ** 2 / (n / len(cells))).sum())
        print(name, "chi2", chi)
        assert chi < 175.13, (name, chi)   # chi2(111 dof) survival 1e-4


@pytest.mark.parametrize("width", [0.0, 0.5])
def test_properties_at_scale(width):
    n, dx, seed = 16384, 0.4, 31
    s = dict(STAGE2, uniform_cost_max=width)
    hfs = terrain_windows(n, 16, 5)
    P = planner(s, True)
    r = P.plan(hfs, seed=seed, dx=dx)
    R = pp.jump_radius(P.settings, dx)
    nbr, cliff, jump = P.graph(0, n)
    nbr, jump = nbr.reshape(n, -1), jump.reshape(n, 256, pp.JUMP_WORDS)
    reached = (r.status == pp.FOUND) | (r.status == pp.OVER_MAX_COST)
    print("width", width, "found", int((r.status == pp.FOUND).sum()), "no path", int((r.status == pp.NO_PATH).sum()), "mean pops", float(r.pops.mean()))
    assert np.isin(r.status, [pp.FOUND, pp.NO_PATH, pp.OVER_MAX_COST]).all()
    assert (r.status == pp.FOUND).mean() > 0.2 and (r.status == pp.NO_PATH).mean() > 0.1
    qs, a, b, first = [], [], [], []
    for q in np.nonzero(reached)[0]:
        nd = r.nodes[q]
        assert np.array_equal(nd[0], r.start[q]) and np.array_equal(nd[-1], r.goal[q]), q
        c = nd[:, 0].astype(np.int64) * 16 + nd[:, 1]
        assert len(set(c.tolist())) == len(c), q
        qs.append(np.full(len(c) - 1, q)); a.append(c[:-1]); b.append(c[1:]); first.append(np.arange(len(c) - 1))
        if r.status[q] == pp.FOUND:
            for e in (0, -1):
                want = np.array([np.float32(nd[e, 0]) * np.float32(dx), np.float32(nd[e, 1]) * np.float32(dx), r.hf[q][nd[e, 0], nd[e, 1]]], np.float32)
                assert np.array_equal(r.points[q][e], want), q
    for q in np.nonzero(~reached)[0][:200]:
        assert len(r.nodes[q]) == 0 and len(r.points[q]) == 0 and np.isnan(r.cost[q])
    qs, a, b, first = (np.concatenate(v) for v in (qs, a, b, first))
    # every hop is an edge of the returned graph: a neighbour bit, or the window bit of a jump edge
    di, dj = b // 16 - a // 16, b % 16 - a % 16
    adjacent = (np.abs(di) <= 1) & (np.abs(dj) <= 1)
    dirs = {d: k for k, d in enumerate(pp.DIRECTIONS)}
    dbit = np.array([dirs.get((int(x), int(y)), 0) for x, y in zip(di, dj)])
    is_nbr = adjacent & (((nbr[qs, a] >> dbit) & 1) == 1)
    inwin = (di >= -R) & (di < R) & (dj >= -R) & (dj < R)
    k = np.where(inwin, (di + R) * 2 * R + dj + R, 0)
    is_jump = inwin & (((jump[qs, a, k >> 5] >> (k & 31).astype(np.uint32)) & 1) == 1)
    assert (is_nbr | is_jump).all()
    assert (is_jump & ~adjacent).sum() > 100          # long jump edges are in use
    # the returned cost is the fp32 sum of its hops' costs recomputed on the host, in path order
    hop = ref.hop_costs(r.hf, dx, dx, (0.0, 0.0), s, seed, qs, a, b)
    g = np.zeros(n, np.float32)
    for step in range(int(first.max()) + 1):
        m = first == step
        g[qs[m]] = (g[qs[m]] + hop[m]).astype(np.float32)
    assert g[reached].tobytes() == r.cost[reached].tobytes()
    assert ((r.status == pp.OVER_MAX_COST) == (reached & (r.cost > np.float32(s["max_cost"])))).all()
    # 64 queries of the batch, one at a time: the same bits
    for q in range(0, n, n // 64):
        one = P.plan(hfs[q:q + 1], seed=seed, dx=dx, first_query=q)
        assert one.status[0] == r.status[q] and one.cost[0].tobytes() == r.cost[q].tobytes() and one.pops[0] == r.pops[q]
        assert np.array_equal(one.nodes[0], r.nodes[q]) and one.points[0].tobytes() == r.points[q].tobytes()
        assert np.array_equal(one.start[0], r.start[q]) and np.array_equal(one.goal[0], r.goal[q]) and one.hf[0].tobytes() == r.hf[q].tobytes()


def test_walled_in_goal_and_budget():
    """A goal island in a pit deeper than max_z_diff, every other cliff cell farther than max_jump_xy_dist: NO_PATH.  The same search
    cut by the expansion budget: BUDGET."""
    hf = np.full((16, 16), -5.0, np.float32)
    hf[0:3, :] = 0.0                 # the start's plateau; its edge row 2 is 10 cells = 4 m from the island
    hf[12:15, 6:9] = 0.0             # the goal's island
    hfs = np.repeat(hf[None], 8, axis=0)
    starts = np.array([[1, j] for j in range(2, 10)], np.int32)
    goals = np.tile(np.array([[13, 7]], np.int32), (8, 1))
    for width in (0.0, 0.5):
        P = planner(dict(STAGE2, uniform_cost_max=width), False)
        r = P.plan(hfs, starts, goals, seed=3)
        assert (r.status == pp.NO_PATH).all() and np.isnan(r.cost).all() and (r.pops > 40).all()
        assert all(len(x) == 0 for x in r.nodes)
    B = planner(STAGE2, False, max_expansions=10)
    r = B.plan(hfs, starts, goals, seed=3)
    assert (r.status == pp.BUDGET).all() and (r.pops == 10).all()
    hf[3:12, 7] = 0.0                # a bridge: now reachable
    r = planner(STAGE2, False).plan(hf[None], starts[:1], goals[:1], seed=3)
    assert r.status[0] == pp.FOUND and len(r.nodes[0]) >= 12


def test_refusals():
    from parc_amd import lib as L
    lib = L.load()
    h = C.c_void_p()
    p = pp.planner_params(pp.AStarSettings(), 16, 16, 0.4, 0.4)
    p.struct_size += 4
    with pytest.raises(L.ParcError, match=r"ParcPathPlanParams ABI mismatch \(struct_size\)"):
        L.check(lib.parc_pathplan_create(C.byref(p), C.byref(h)))
    with pytest.raises(L.ParcError, match=r"the grid is 80 x 80, the planner takes 4 \.\. 64 cells a side \(PARC_PATHPLAN_MAX_DIM"):
        planner(STAGE2, True).plan(np.zeros((1, 80, 80), np.float32))
    with pytest.raises(L.ParcError, match=r"jump window radius of 13 cells, above the limit of 8 \(PARC_PATHPLAN_MAX_JUMP_RADIUS\)"):
        planner(dict(STAGE2, max_jump_xy_dist=5.0), True).plan(np.zeros((1, 16, 16), np.float32))
    with pytest.raises(L.ParcError, match="outside the grid"):
        planner(STAGE2, True).plan(np.zeros((1, 16, 16), np.float32), [[1, 16]], [[5, 5]])
    big = planner(STAGE2, True).plan(np.zeros((2, 64, 64), np.float32), [[1, 1], [2, 60]], [[62, 62], [61, 3]], seed=1)
    assert (big.status == pp.FOUND).all()


def _same_plan(a, b):
    assert np.array_equal(a.status, b.status) and a.cost.tobytes() == b.cost.tobytes() and np.array_equal(a.pops, b.pops)
    assert np.array_equal(a.start, b.start) and np.array_equal(a.goal, b.goal) and a.hf.tobytes() == b.hf.tobytes()
    assert len(a.nodes) == len(b.nodes) and all(np.array_equal(x, y) for x, y in zip(a.nodes, b.nodes))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a.points, b.points))


def test_a_planner_reused_across_batch_sizes_equals_a_fresh_one():
    """Q = 3, then 5 (the buffers grow), then 2 (they stay) on one handle: each batch as a fresh planner plans it; the graph afterwards
    is the last batch's, and a range beyond it is refused although the buffers are larger."""
    from gpu_helpers import raises_invalid
    hfs = terrain_windows(5, 8, 11)
    starts = np.array([[1, 1], [1, 6], [2, 1], [6, 5], [1, 3]], np.int32)
    goals = np.array([[6, 6], [6, 1], [5, 6], [1, 2], [6, 4]], np.int32)
    P = planner(STAGE2, True)
    for q in (slice(0, 3), slice(0, 5), slice(3, 5)):
        r = P.plan(hfs[q], starts[q], goals[q], seed=13)
        F = planner(STAGE2, True)
        _same_plan(r, F.plan(hfs[q], starts[q], goals[q], seed=13))
    assert np.isin(r.status, [pp.FOUND, pp.NO_PATH, pp.OVER_MAX_COST]).all()
    for x, y in zip(P.graph(0, 2), F.graph(0, 2)):
        assert x.tobytes() == y.tobytes()
    u8 = C.POINTER(C.c_uint8)
    nbr, cliff, jump = np.zeros((2, 8, 8), np.uint8), np.zeros((2, 8, 8), np.uint8), np.zeros((2, 8, 8, pp.JUMP_WORDS), np.uint32)
    raises_invalid(lambda: P._lib.parc_pathplan_get_graph(P._h, 1, 2, nbr.ctypes.data_as(u8), cliff.ctypes.data_as(u8),
                                                          jump.ctypes.data_as(C.POINTER(C.c_uint32))),
                   "pathplan: the query range lies outside the last batch")
    for x, y in zip(P.graph(1, 1), F.graph(1, 1)):
        assert x.tobytes() == y.tobytes()


def test_plan_terrains_first_success():
    hfs = terrain_windows(96, 16, 9)
    P = planner(STAGE2, True)
    attempt, sel = P.plan_terrains(hfs, num_attempts=10, seed=5)
    wide = P.plan(np.repeat(hfs, 10, axis=0), seed=5)
    st = wide.status.reshape(96, 10)
    for t in range(96):
        ok = np.nonzero(st[t] == pp.FOUND)[0]
        assert attempt[t] == (ok[0] if len(ok) else -1)
        if len(ok):
            q = t * 10 + ok[0]
            assert sel.status[t] == pp.FOUND and sel.cost[t].tobytes() == wide.cost[q].tobytes() and np.array_equal(sel.nodes[t], wide.nodes[q])
    assert (attempt >= 0).mean() > 0.5 and (attempt > 0).any()


def test_plan_paths_script(tmp_path):
    """scripts/plan_paths.py on the bundled teaser terrain: every written path starts and ends at its start / goal, walks the written
    terrain, and the windows are cuts of the source terrain at the written offsets."""
    import json
    import subprocess
    import sys
    from parc_amd import ms_file
    out = subprocess.run([sys.executable, os.path.join(REPO, "scripts/plan_paths.py"), "--terrain", os.path.join(REPO, "data/motion_terrains/TEASER_TERRAIN.pkl"),
                          "--num_terrains", "256", "--seed", "4", "--out", str(tmp_path)], check=True, capture_output=True, text=True, timeout=300)
    summary = json.loads(out.stdout.strip().splitlines()[-1])
    z = np.load(tmp_path / "paths_0000.npz")
    ok = z["attempt"] >= 0
    assert summary["terrains"] == 256 and summary["found"] == int(ok.sum()) and summary["queries"] == 2560 and summary["queries_per_s"] > 0
    assert ok.mean() > 0.5 and ((z["status"] == pp.FOUND) == ok).all()
    td = ms_file.load_ms_file(os.path.join(REPO, "data/motion_terrains/TEASER_TERRAIN.pkl"), load_misc=False).terrain_data
    dx = np.float32(z["dx"])
    for t in range(256):
        nd = z["nodes"][z["node_off"][t]:z["node_off"][t + 1]]
        pts = z["points"][z["point_off"][t]:z["point_off"][t + 1]]
        cell = np.rint((z["min_point_offset"][t] - np.asarray(td.min_point, np.float32)) / dx).astype(int)
        src = np.asarray(td.hf, np.float32)[cell[0]:cell[0] + 16, cell[1]:cell[1] + 16]
        assert z["hf"][t].tobytes() == ref.simplify(src, tuple(z["start"][t]), tuple(z["goal"][t])).tobytes()
        if not ok[t]:
            assert len(nd) == 0 and len(pts) == 0
            continue
        assert np.array_equal(nd[0], z["start"][t]) and np.array_equal(nd[-1], z["goal"][t]) and len(pts) >= len(nd)
        hop = np.abs(np.diff(nd, axis=0)).max(axis=1)
        assert hop.min() >= 1 and hop.max() <= 8
        assert np.array_equal(pts[-1], np.array([np.float32(nd[-1, 0]) * dx, np.float32(nd[-1, 1]) * dx, z["hf"][t][nd[-1, 0], nd[-1, 1]]], np.float32))
        step = np.sqrt((np.diff(pts[:, :2], axis=0) ** 2).sum(axis=1))
        # pieces are dist / (steps - 1), steps = ceil(dist / dx): a straight hop of two cells stays one piece of 2 dx, longer hops split finer
        assert step.max() <= 2 * 0.4 + 1e-5
