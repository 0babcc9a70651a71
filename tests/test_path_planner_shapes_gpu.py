"""Terrain path planner on the GPU away from the fixtures' square 16 / 32 grids (parc_pathplan_*): fresh queries on
rectangular, padded and minimal grids with ``dx != dy``, a shifted origin and every jump radius class, each compared with the numpy
restatement (``path_planner_ref``), which ``test_path_planner_cpu`` pins to the reference at rectangular shapes too.

Bars (the sibling file's): start / goal, simplified heightfield, edge sets, cliff flags, status, node lists and pops exact; cost bit for
bit with ``w_bumpy = 0`` and to 1e-5 with ``w_bumpy > 0`` (decision margins above 1e-5, asserted); point counts exact, coordinates 2e-6.
What a case needs from its inputs (zero ties, found and lost quarters, long hops, margins, ties where ties are the point) is asserted
from the restatement's own output, so a change of seeds cannot quietly empty a case."""
import collections
import ctypes as C
import functools
import os

import numpy as np
import pytest

import path_planner_ref as ref
from parc_amd import path_planner as pp
from test_path_planner_cpu import REPO
from test_path_planner_gpu import STAGE2, _same_plan, planner

pytestmark = pytest.mark.gpu
SHIFTED, SHIFTED2 = (1.7, -2.3), (-3.1, 0.9)

# one batch of n device-drawn queries on windows of the bundled terrains; ``over`` = settings on top of STAGE2 as sorted items
Row = collections.namedtuple("Row", "X Y dx dy min_point simplify n seed first_query over")


def row(X, Y, dx, dy, min_point, simplify, n, seed, first_query=0, **over):
    over.setdefault("min_start_end_xy_dist", min(3.0, 0.4 * (min(X, Y) - 3)))
    return Row(X, Y, dx, dy, min_point, simplify, n, seed, first_query, tuple(sorted(over.items())))


def settings_of(r):
    return dict(STAGE2, **dict(r.over))


#      grid    dx   dy   origin   simplify n seed first_query  jump radius R = ceil(max_jump_xy_dist / dx)
SWEEP = [
    row(4, 4, 0.4, 0.4, (0.0, 0.0), False, 8, 101, max_jump_xy_dist=0.0),                                   # R 0, the smallest grid
    row(4, 7, 0.4, 0.5, SHIFTED, True, 8, 102, 40, max_jump_xy_dist=0.4, uniform_cost_min=0.1),            # R 1
    row(5, 64, 0.5, 0.4, SHIFTED2, True, 8, 103, max_jump_xy_dist=2.0),                                     # R 4, the y limit
    row(64, 5, 0.4, 0.5, (0.0, 0.0), False, 8, 104, 7, max_jump_xy_dist=2.8, uniform_cost_min=0.1),        # R 7, the x limit
    row(9, 9, 0.4, 0.4, SHIFTED, True, 8, 105, max_jump_xy_dist=1.2),                                       # R 3: 36 candidates, N = 81
    row(23, 11, 0.4, 0.5, SHIFTED, True, 8, 106, 1000, max_jump_xy_dist=3.0),                               # R 8, N = 253, NP = 256
    row(17, 15, 0.5, 0.4, (0.0, 0.0), False, 8, 107, max_jump_xy_dist=0.4, uniform_cost_min=0.1),           # R 1, N = 255
    row(18, 18, 0.4, 0.4, SHIFTED2, True, 8, 208, max_jump_xy_dist=2.8),                                    # R 7, N = 324, NP = 512
    row(12, 20, 0.4, 0.5, (0.0, 0.0), True, 8, 109, 3, max_jump_xy_dist=1.2, uniform_cost_min=0.1),         # R 3
    row(20, 12, 0.5, 0.4, SHIFTED2, True, 8, 110, max_jump_xy_dist=0.0),                                    # R 0
    row(15, 17, 0.4, 0.4, (0.0, 0.0), False, 8, 214, max_jump_xy_dist=2.0),                                 # R 5: 100 candidates, N = 255
    row(64, 64, 0.4, 0.4, SHIFTED, True, 1, 213, 5, max_jump_xy_dist=3.0, min_start_end_xy_dist=2.0),       # R 8, the largest grid
]
BUMPY = [row(12, 20, 0.4, 0.5, SHIFTED, True, 6, 201, w_bumpy=1.0),
         row(13, 17, 0.5, 0.4, SHIFTED2, True, 6, 202, 11, w_bumpy=1.0, max_jump_xy_dist=2.0)]


def ids(rows):
    return [f"{r.X}x{r.Y}" for r in rows]


@functools.lru_cache(maxsize=None)
def terrains():
    from parc_amd import ms_file
    return [np.asarray(ms_file.load_ms_file(os.path.join(REPO, "data/motion_terrains", t + ".pkl"), load_misc=False).terrain_data.hf, np.float32)
            for t in ("TEASER_TERRAIN", "civilization", "sfu")]


def windows(n, X, Y, seed):
    """``test_path_planner_gpu.terrain_windows`` cut rectangular; the terrains too small for the window are left out of the cycle."""
    rng = np.random.RandomState(seed)
    ts = [T for T in terrains() if T.shape[0] >= X and T.shape[1] >= Y]
    out = np.zeros((n, X, Y), np.float32)
    for k in range(n):
        T = ts[k % len(ts)]
        sx, sy = rng.randint(0, T.shape[0] + 1 - X), rng.randint(0, T.shape[1] + 1 - Y)
        out[k] = T[sx:sx + X, sy:sy + Y]
    return out


def restate_query(r, hf_in, start, goal, query, settings=None, **kw):
    """The restatement's answer for one query of Row r: what every comparison below reads."""
    s = settings if settings is not None else settings_of(r)
    hf = ref.simplify(hf_in, start, goal) if r.simplify else np.array(hf_in, np.float32)
    graph = ref.build_graph(hf, r.dx, r.dy, r.min_point, s)
    res = ref.search(hf, r.dx, r.dy, r.min_point, start, goal, s, r.seed, query, graph=graph, **kw)
    pts = ref.polyline(hf, r.dx, r.dy, r.min_point, res["nodes"]) if res["status"] == ref.FOUND else np.zeros((0, 3), np.float32)
    hop = max([max(abs(a[0] - b[0]), abs(a[1] - b[1])) for a, b in zip(res["nodes"][:-1], res["nodes"][1:])] or [0])
    return dict(start=tuple(start), goal=tuple(goal), hf=hf, graph=graph, res=res, points=pts, hop=hop)


@functools.lru_cache(maxsize=None)
def restated(r):
    """(windows, the restatement's answers) of Row r, computed once per session and left unchanged."""
    hfs = windows(r.n, r.X, r.Y, r.seed)
    hfs.setflags(write=False)
    out = []
    for k in range(r.n):
        sg = ref.draw_start_goal(r.seed, r.first_query + k, r.X, r.Y, r.dx, r.dy, r.min_point, settings_of(r)["min_start_end_xy_dist"])
        assert sg is not None, (r, k)
        out.append(restate_query(r, hfs[k], sg[0], sg[1], r.first_query + k))
    return hfs, out


def planner_of(r, settings=None, **kw):
    return planner(settings if settings is not None else settings_of(r), r.simplify, min_point=r.min_point, **kw)


def check_search(got, k, w, tag, bumpy=False):
    """Query k of a PathPlan against the restatement's answer w: start / goal, heightfield, status, nodes, pops, cost, polyline."""
    res = w["res"]
    print(tag, k, "status", got.status[k], res["status"], "cost", got.cost[k], res["cost"], "pops", got.pops[k], res["pops"], "nodes", len(got.nodes[k]),
          len(res["nodes"]), "points", len(got.points[k]), len(w["points"]), "ties", res["ties"], "margin", res["margin"])
    assert tuple(got.start[k]) == w["start"] and tuple(got.goal[k]) == w["goal"], (tag, k)
    assert got.hf[k].tobytes() == w["hf"].tobytes(), (tag, k)
    assert got.status[k] == res["status"], (tag, k)
    assert [tuple(c) for c in got.nodes[k].tolist()] == res["nodes"], (tag, k)
    assert got.pops[k] == res["pops"], (tag, k)
    if not len(res["nodes"]):
        assert np.isnan(got.cost[k]), (tag, k)
    elif bumpy:
        assert abs(float(got.cost[k]) - float(res["cost"])) <= 1e-5, (tag, k)
    else:
        assert got.cost[k].tobytes() == np.float32(res["cost"]).tobytes(), (tag, k)
    assert got.points[k].shape == w["points"].shape, (tag, k)
    if len(w["points"]):
        assert np.abs(got.points[k] - w["points"]).max() <= 2e-6, (tag, k)


def check_graph(P, r, want, tag):
    R = pp.jump_radius(P.settings, r.dx)
    nbr, cliff, jump = P.graph(0, len(want))
    for k, w in enumerate(want):
        assert pp.edges_from_graph(nbr[k], jump[k], R) == ref.edge_sets(w["graph"][0], w["graph"][1]), (tag, k)
        assert np.array_equal(cliff[k].astype(bool), w["graph"][2]), (tag, k)


# ---- a. the shape sweep -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", SWEEP, ids=ids(SWEEP))
def test_shape_sweep(r):
    """One batch of device-drawn queries per grid: everything the planner returns, and its graph, against the restatement."""
    hfs, want = restated(r)
    assert all(w["res"]["ties"] == 0 for w in want), [w["res"]["ties"] for w in want]
    P = planner_of(r)
    got = P.plan(hfs, seed=r.seed, dx=r.dx, dy=r.dy, first_query=r.first_query)
    tag = f"{r.X}x{r.Y}"
    for k, w in enumerate(want):
        check_search(got, k, w, tag)
    check_graph(P, r, want, tag)


def test_shape_sweep_inputs():
    """What the sweep's seeds must give, from the restatement alone: every setting class on two rows or more, a quarter of the queries
    found and a quarter not, three found paths or more with a hop of three cells or more."""
    radii = collections.Counter(ref.jump_radius(settings_of(r), r.dx) for r in SWEEP)
    jumps = collections.Counter(settings_of(r)["max_jump_xy_dist"] for r in SWEEP)
    assert all(jumps[v] >= 2 for v in (0.0, 0.4, 1.2, 2.0, 2.8, 3.0)) and radii[0] >= 2 and {3, 5} <= set(radii), (jumps, radii)
    assert sum(r.dx > r.dy for r in SWEEP) >= 2 and sum(r.dx < r.dy for r in SWEEP) >= 2
    assert sum(r.min_point != (0.0, 0.0) for r in SWEEP) >= 2 and sum(settings_of(r)["uniform_cost_min"] != 0.0 for r in SWEEP) >= 2
    assert sum(r.simplify for r in SWEEP) >= 2 and sum(not r.simplify for r in SWEEP) >= 2
    assert {(r.X, r.Y) for r in SWEEP} >= {(4, 4), (4, 7), (5, 64), (64, 5), (9, 9), (23, 11), (17, 15), (18, 18), (12, 20), (20, 12), (64, 64)}
    res = [w for r in SWEEP for w in restated(r)[1]]
    found = sum(w["res"]["status"] == ref.FOUND for w in res)
    long_hops = sum(w["res"]["status"] == ref.FOUND and w["hop"] >= 3 for w in res)
    print("queries", len(res), "found", found, "long hops", long_hops)
    assert len(res) == sum(r.n for r in SWEEP) and 4 * found >= len(res) and 4 * (len(res) - found) >= len(res) and long_hops >= 3


# ---- b. the bumpy term off the square -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", BUMPY, ids=ids(BUMPY))
def test_bumpy_off_the_square(r):
    """w_bumpy = 1: the nine patch sums clamp at the borders of a rectangular grid.  The double accumulation leaves the cost within 1e-5
    of the restatement's, so the decisions are comparable only where its margin is larger: asserted for every query."""
    hfs, want = restated(r)
    assert all(w["res"]["ties"] == 0 and w["res"]["margin"] > 1e-5 for w in want), [(w["res"]["ties"], w["res"]["margin"]) for w in want]
    assert any(w["res"]["status"] == ref.FOUND for w in want)
    got = planner_of(r).plan(hfs, seed=r.seed, dx=r.dx, dy=r.dy, first_query=r.first_query)
    for k, w in enumerate(want):
        check_search(got, k, w, f"bumpy {r.X}x{r.Y}", bumpy=True)


# ---- c. ties ------------------------------------------------------------------------------------------------------------------------
def wall_with_two_gaps(Y, gaps):
    hf = np.zeros((12, Y), np.float32)
    hf[6, :] = 3.0
    hf[6, list(gaps)] = 0.0
    return hf


@pytest.mark.parametrize("Y,gaps,transposed", [(21, (3, 17), False), (21, (3, 17), True), (13, (3, 9), False), (13, (3, 9), True)])
def test_ties_pop_in_cell_index_order(Y, gaps, transposed):
    """No noise, dx = dy = 0.5 and a zero origin (exact in fp32), a wall with two gaps mirrored about the start / goal column: mirrored
    cells carry equal (f, g).  The yardstick under ties is the restatement's documented (f, g, cell index) order, which the kernel's
    lane scan and wave butterfly must reproduce -- not the reference's heap, whose order among equal keys is an accident of its pushes."""
    hf, start, goal = wall_with_two_gaps(Y, gaps), (1, Y // 2), (10, Y // 2)
    if transposed:
        hf, start, goal = np.ascontiguousarray(hf.T), start[::-1], goal[::-1]
    r = row(hf.shape[0], hf.shape[1], 0.5, 0.5, (0.0, 0.0), False, 1, 5, uniform_cost_max=0.0)
    w = restate_query(r, hf, start, goal, 0)
    print("ties", w["res"]["ties"], "nodes", w["res"]["nodes"])
    assert w["res"]["ties"] > 0 and w["res"]["status"] == ref.FOUND
    if not transposed:
        assert w["res"]["ties"] == {21: 35, 13: 6}[Y] and (6, gaps[0]) in w["res"]["nodes"]      # through the gap of the lower index
    P = planner_of(r)
    got = P.plan(hf[None], [start], [goal], seed=r.seed, dx=r.dx, dy=r.dy)
    check_search(got, 0, w, f"ties {hf.shape}")
    check_graph(P, r, [w], "ties")


# ---- d. the paths nothing else compares ----------------------------------------------------------------------------------------------
def test_no_draw():
    """min_start_end_xy_dist beyond the grid's diagonal: 1000 draws fail on the device as in the restatement."""
    r = row(12, 20, 0.4, 0.5, SHIFTED, True, 4, 301, 9, min_start_end_xy_dist=100.0)
    s = settings_of(r)
    assert all(ref.draw_start_goal(r.seed, r.first_query + k, r.X, r.Y, r.dx, r.dy, r.min_point, s["min_start_end_xy_dist"]) is None for k in range(r.n))
    got = planner_of(r).plan(windows(r.n, r.X, r.Y, r.seed), seed=r.seed, dx=r.dx, dy=r.dy, first_query=r.first_query)
    assert (got.status == pp.NO_DRAW).all() and np.isnan(got.cost).all() and (got.pops == 0).all()
    assert all(len(x) == 0 for x in got.nodes) and all(len(x) == 0 for x in got.points)


@pytest.mark.parametrize("simplify", [False, True])
def test_start_equals_goal(simplify):
    r = row(13, 17, 0.4, 0.5, SHIFTED, simplify, 4, 302)
    hfs = windows(r.n, r.X, r.Y, r.seed)
    cells = [(1, 1), (6, 8), (12, 16), (11, 2)]            # an inner cell, and border cells outside the draw ring
    got = planner_of(r).plan(hfs, cells, cells, seed=r.seed, dx=r.dx, dy=r.dy)
    for k, c in enumerate(cells):
        w = restate_query(r, hfs[k], c, c, k)
        assert w["res"]["status"] == ref.FOUND and w["res"]["pops"] == 1 and w["res"]["nodes"] == [c] and w["points"].shape == (1, 3)
        check_search(got, k, w, f"start == goal simplify {simplify}")
        assert got.cost[k].tobytes() == np.float32(0.0).tobytes() and np.array_equal(got.points[k], w["points"])


def test_over_max_cost():
    """A lowered max_cost: the path and its cost are still reported, the polyline is not."""
    r = row(12, 20, 0.4, 0.4, SHIFTED, True, 8, 303, uniform_cost_min=0.1, uniform_cost_max=0.6, max_cost=7.0)
    hfs, want = restated(r)
    over = [w["res"]["status"] == ref.OVER_MAX_COST for w in want]
    assert sum(over) >= 2 and sum(w["res"]["status"] == ref.FOUND for w in want) >= 2 and all(w["res"]["ties"] == 0 for w in want)
    got = planner_of(r).plan(hfs, seed=r.seed, dx=r.dx, dy=r.dy)
    for k, w in enumerate(want):
        check_search(got, k, w, "over max cost")
        if over[k]:
            assert len(got.nodes[k]) > 1 and got.cost[k] > np.float32(7.0) and len(got.points[k]) == 0


def test_budget():
    """The expansion budget cuts three real-terrain searches at the same pop in the kernel and in the restatement."""
    r = row(18, 18, 0.4, 0.5, SHIFTED2, True, 3, 304, 2)
    hfs, full = restated(r)
    assert all(w["res"]["pops"] > 10 and w["res"]["ties"] == 0 for w in full)
    got = planner_of(r, max_expansions=10).plan(hfs, seed=r.seed, dx=r.dx, dy=r.dy, first_query=r.first_query)
    for k, w in enumerate(full):
        cut = restate_query(r, hfs[k], w["start"], w["goal"], r.first_query + k, max_expansions=10)
        assert cut["res"]["status"] == ref.BUDGET and cut["res"]["pops"] == 10
        check_search(got, k, cut, "budget")


def trench():
    """12 x 20, a trench too deep to walk through (columns 8 .. 11): every crossing is a jump of five cells, which the polyline splits."""
    hf = np.zeros((12, 20), np.float32)
    hf[:, 8:12] = -3.0
    return hf


def raw_run(P, hfs, starts, goals, seed, first_query=0):
    """parc_pathplan_run on P's handle with rows of P's own max_nodes / max_points, as ``plan`` sizes them, without its length check."""
    from parc_amd import lib as L
    Q, X, Y = hfs.shape
    p = P._params
    shapes = dict(status=(Q,), cost=(Q,), num_nodes=(Q,), nodes=(Q, p.max_nodes), num_points=(Q,), points=(Q, p.max_points, 3), start=(Q, 2),
                  goal=(Q, 2), hf=(Q, X, Y), pops=(Q,))
    arr = {n: np.zeros(shapes[n], np.float32 if t == "f" else np.int32) for n, t in L.PATHPLAN_OUTPUT_FIELDS}
    out = L.ParcPathPlanOutputs()
    for n, t in L.PATHPLAN_OUTPUT_FIELDS:
        setattr(out, n, L.np_f32p(arr[n]) if t == "f" else L.np_i32p(arr[n]))
    s, g = np.ascontiguousarray(starts, np.int32), np.ascontiguousarray(goals, np.int32)
    L.check(P._lib.parc_pathplan_run(P._h, Q, L.np_f32p(np.ascontiguousarray(hfs, np.float32)), L.np_i32p(s), L.np_i32p(g), int(seed), int(first_query), C.byref(out)))
    return arr


@pytest.mark.parametrize("limit", ["max_nodes", "max_points"])
def test_truncated_rows(limit):
    """A path longer than the handle's rows, in the middle of a batch of three: the kernel's writes are bounded by max_nodes / max_points
    (the guards of the walk-back and of the polyline), the counts report the full lengths, the rows hold the path's head, the
    neighbouring queries are untouched, ``plan`` refuses the batch, and the handle then plans a fitting batch."""
    from parc_amd import lib as L
    cap = 6
    r = row(12, 20, 0.4, 0.4, SHIFTED, False, 3, 305)
    hfs = np.repeat(trench()[None], 3, axis=0)
    starts, goals = [(1, 1), (1, 2), (2, 15)], [(3, 3), (10, 17), (5, 17)]
    want = [restate_query(r, hfs[k], starts[k], goals[k], k) for k in range(3)]
    nn, npt = [len(w["res"]["nodes"]) for w in want], [len(w["points"]) for w in want]
    print("nodes", nn, "points", npt)
    assert all(w["res"]["status"] == ref.FOUND and w["res"]["ties"] == 0 for w in want) and want[1]["hop"] >= 5
    assert max(npt[0], npt[2]) <= cap < nn[1] < npt[1]
    P = planner_of(r, **{limit: cap})
    with pytest.raises(L.ParcError, match="construct the planner with larger limits"):
        P.plan(hfs, starts, goals, seed=r.seed, dx=r.dx, dy=r.dy)
    a = raw_run(P, hfs, starts, goals, r.seed)
    assert a["status"].tolist() == [ref.FOUND] * 3 and a["num_nodes"].tolist() == nn
    assert a["cost"].tobytes() == np.array([w["res"]["cost"] for w in want], np.float32).tobytes()
    Y = r.Y
    if limit == "max_nodes":
        assert a["nodes"][1].tolist() == [i * Y + j for i, j in want[1]["res"]["nodes"][:cap]]
        assert a["num_points"][[0, 2]].tolist() == [npt[0], npt[2]]
    else:
        assert a["num_points"].tolist() == npt and a["nodes"][1, :nn[1]].tolist() == [i * Y + j for i, j in want[1]["res"]["nodes"]]
        assert np.abs(a["points"][1] - want[1]["points"][:cap]).max() <= 2e-6
    for k in (0, 2):                # the neighbours' rows, bit for bit as each query gives them alone (the rows' tails are not written)
        solo = raw_run(P, hfs[k:k + 1], starts[k:k + 1], goals[k:k + 1], r.seed, first_query=k)
        for name in ("status", "cost", "num_nodes", "num_points", "start", "goal", "hf", "pops"):
            assert a[name][k].tobytes() == solo[name][0].tobytes(), (name, k)
        assert a["num_nodes"][k] == nn[k] and a["num_points"][k] == npt[k]
        assert a["nodes"][k, :nn[k]].tobytes() == solo["nodes"][0, :nn[k]].tobytes()
        assert a["points"][k, :npt[k]].tobytes() == solo["points"][0, :npt[k]].tobytes()
        assert a["nodes"][k, :nn[k]].tolist() == [i * Y + j for i, j in want[k]["res"]["nodes"]]
        assert np.abs(a["points"][k, :npt[k]] - want[k]["points"]).max() <= 2e-6
    fit = P.plan(hfs[[0, 2]], [starts[0], starts[2]], [goals[0], goals[2]], seed=r.seed, dx=r.dx, dy=r.dy)
    check_search(fit, 0, want[0], "after a truncated batch")
    check_search(fit, 1, restate_query(r, hfs[2], starts[2], goals[2], 1), "after a truncated batch")


# ---- e. one planner object, interleaved shapes -------------------------------------------------------------------------------------------
def test_one_planner_interleaved_shapes():
    """64 x 64, 8 x 8, 64 x 64 again, 12 x 20 on one object: each create sets the search kernel's dynamic-LDS attribute for its own
    grid, and every plan equals a fresh planner's bit for bit; the large and the rectangular ones equal the restatement."""
    big = SWEEP[-1]
    assert (big.X, big.Y) == (64, 64)
    rect = row(12, 20, 0.4, 0.5, big.min_point, big.simplify, 4, 401, **dict(big.over))
    small = row(8, 8, 0.4, 0.4, big.min_point, big.simplify, 4, 402, **dict(big.over))
    P = planner_of(big)
    for r in (big, small, big, rect):
        hfs = restated(r)[0] if r is not small else windows(r.n, r.X, r.Y, r.seed)
        got = P.plan(hfs, seed=r.seed, dx=r.dx, dy=r.dy, first_query=r.first_query)
        _same_plan(got, planner_of(r).plan(hfs, seed=r.seed, dx=r.dx, dy=r.dy, first_query=r.first_query))
        if r is not small:
            for k, w in enumerate(restated(r)[1]):
                check_search(got, k, w, f"interleaved {r.X}x{r.Y}")
        else:
            assert (got.status != pp.NO_DRAW).all()
