"""Array-based numpy restatement of the terrain path planner, the CPU yardstick of ``parc_pathplan_*``.

Everything the reference's ``motion_synthesis/procgen/astar.py`` computes under numpy >= 2 is fp32 (positions come from torch fp32, the
Python-float weights are weak scalars), so the restatement is written in fp32 with the reference's association: open flags plus ``g`` /
``f`` arrays, pop = arg-min over ``(f, g, cell index)``, no heap.  With the per-edge step-cost noise (a pure function of seed, query, from
cell, to cell) the reference's stale heap entries re-expand to no-ops, so this pops the reference's sequence.  ``search`` also reports the
number of ``(f, g)`` ties between different cells and the decision margin (the smallest gap by which a pop or a relaxation was decided).
"""
import math

import numpy as np

F32 = np.float32
FOUND, NO_PATH, OVER_MAX_COST, BUDGET, NO_DRAW = 0, 1, 2, 3, 4
DIRECTIONS = [(-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (-1, 1), (1, -1), (1, 1)]
CROSS = DIRECTIONS[:4]

DEFAULTS = dict(max_z_diff=2.1, max_jump_xy_dist=3.0, max_jump_z_diff=0.3, min_jump_z_diff=-0.7, w_z=0.15, w_xy=1.0, w_bumpy=1.0,
                max_bumpy=0.2, uniform_cost_max=0.25, uniform_cost_min=0.0, min_start_end_xy_dist=4.0, max_cost=1000.0)

DRAW_STREAM = 1 << 62          # counter word of the start / goal draws: (DRAW_STREAM | query, attempt)
MAX_DRAW_ATTEMPTS = 1000


# ---- Philox4x32-10, the library's variant (key = seed, counter = (lo, hi low, hi high, 'PARK')) -------------------------------------
def philox4(seed, ctr_hi, ctr_lo):
    m = 0xFFFFFFFF
    c = [ctr_lo & m, ctr_hi & m, (ctr_hi >> 32) & m, 0x5041524B]
    k0, k1 = seed & m, (seed >> 32) & m
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [((p1 >> 32) ^ c[1] ^ k0) & m, p1 & m, ((p0 >> 32) ^ c[3] ^ k1) & m, p0 & m]
        k0, k1 = (k0 + 0x9E3779B9) & m, (k1 + 0xBB67AE85) & m
    return [F32(x >> 8) * F32(1.0 / 16777216.0) for x in c]


def edge_noise(seed, query, from_cell, to_cell, cost_min, cost_max):
    """fp32(u * fp32(max - min) + fp32(min)), u the first 24-bit uniform of counter (query, from_cell << 16 | to_cell)."""
    u = philox4(seed, query, (from_cell << 16) | to_cell)[0]
    return F32(F32(u * F32(cost_max - cost_min)) + F32(cost_min))


# ---- geometry -----------------------------------------------------------------------------------------------------------------
def positions(hf, dx, dy, min_point):
    """SubTerrain.get_xyz_point for every cell: min_point + ij * dxdy in fp32."""
    X, Y = hf.shape
    x = (F32(min_point[0]) + np.arange(X).astype(F32) * F32(dx)).astype(F32)
    y = (F32(min_point[1]) + np.arange(Y).astype(F32) * F32(dy)).astype(F32)
    return x, y


def ring_cells(X, Y):
    """pick_random_start_end_nodes_on_edges' candidate list, in its order."""
    return [(i, j) for i in range(X) for j in range(Y)
            if (i == 1 or i == 2 or i == X - 2 or i == X - 3) or (j == 1 or j == 2 or j == Y - 2 or j == Y - 3)]


def draw_start_goal(seed, query, X, Y, dx, dy, min_point, min_dist):
    """Both cells uniform over the ring list, redrawn until the xy distance is >= min_dist - 1e-4; None after 1000 attempts."""
    cells = ring_cells(X, Y)
    n = len(cells)
    x, y = positions(np.zeros((X, Y), F32), dx, dy, min_point)
    thr = F32(float(min_dist) - 1e-4)
    for attempt in range(MAX_DRAW_ATTEMPTS):
        u = philox4(seed, DRAW_STREAM | query, attempt)
        s = cells[min(int(u[0] * F32(n)), n - 1)]
        g = cells[min(int(u[1] * F32(n)), n - 1)]
        ddx, ddy = F32(x[s[0]] - x[g[0]]), F32(y[s[1]] - y[g[1]])
        if np.sqrt(F32(F32(ddx * ddx) + F32(ddy * ddy))) >= thr:
            return s, g
    return None


def py_slice(a, n):
    """range of the Python slice a : a + 4 on an axis of n cells."""
    return range(*slice(a, a + 4).indices(n))


def simplify(hf, start, goal):
    """flat_maxpool_2x2, then flatten_4x4_near_edge around the start and around the goal (parc_2_kin_gen.py:317-328)."""
    hf = np.array(hf, F32)
    X, Y = hf.shape
    for i in range(0, X - 1, 2):
        for j in range(0, Y - 1, 2):
            hf[i:i + 2, j:j + 2] = hf[i:i + 2, j:j + 2].max()
    for c in (start, goal):
        h = hf[c[0], c[1]]
        xs = py_slice(c[0] - 2 if c[0] % 2 == 0 else c[0] - 1, X)
        ys = py_slice(c[1] - 2 if c[1] % 2 == 0 else c[1] - 1, Y)
        for i in xs:
            for j in ys:
                hf[i, j] = h
    return hf


def line_indices(x0, y0, x1, y1):
    """terrain_util.get_line_indices (Bresenham, both ends included)."""
    out = []
    ddx, ddy = abs(x1 - x0), abs(y1 - y0)
    sx, sy = (1 if x0 < x1 else -1), (1 if y0 < y1 else -1)
    err = ddx - ddy
    while True:
        out.append((x0, y0))
        if x0 == x1 and y0 == y1:
            return out
        e2 = 2 * err
        if e2 > -ddy:
            err -= ddy
            x0 += sx
        if e2 < ddx:
            err += ddx
            y0 += sy


def jump_radius(settings, dx):
    return int(math.ceil(float(settings["max_jump_xy_dist"]) / float(F32(dx))))


def build_graph(hf, dx, dy, min_point, settings):
    """construct_navigation_graph: (neighbour edges, jump edges) per cell as sorted lists of (i, j), and the cliff flags."""
    hf = np.asarray(hf, F32)
    X, Y = hf.shape
    x, y = positions(hf, dx, dy, min_point)
    mz, mjxy = F32(settings["max_z_diff"]), F32(settings["max_jump_xy_dist"])
    mxj, mnj = F32(settings["max_jump_z_diff"]), F32(settings["min_jump_z_diff"])
    eps = F32(1e-3)
    cliff = np.zeros((X, Y), bool)
    for i in range(1, X - 1):
        for j in range(1, Y - 1):
            cliff[i, j] = any(F32(hf[i, j] - hf[i + a, j + b]) > eps for a, b in CROSS)
    R = jump_radius(settings, dx)
    nbr = [[[] for _ in range(Y)] for _ in range(X)]
    jump = [[[] for _ in range(Y)] for _ in range(X)]
    for i in range(X):
        for j in range(Y):
            for a, b in DIRECTIONS:
                r, c = i + a, j + b
                if 0 <= r < X and 0 <= c < Y and abs(F32(hf[r, c] - hf[i, j])) <= mz:
                    nbr[i][j].append((r, c))
            if not cliff[i, j]:
                continue
            thr = F32(F32(hf[i, j] + mxj) + eps)
            for ii in range(max(i - R, 1), min(i + R, X - 1)):
                for jj in range(max(j - R, 1), min(j + R, Y - 1)):
                    if not cliff[ii, jj]:
                        continue
                    ddx, ddy = F32(x[i] - x[ii]), F32(y[j] - y[jj])
                    if not np.sqrt(F32(F32(ddx * ddx) + F32(ddy * ddy))) <= mjxy:
                        continue
                    dz = F32(hf[ii, jj] - hf[i, j])
                    if not (mnj <= dz <= mxj):
                        continue
                    if all(hf[p, q] < thr for p, q in line_indices(i, j, ii, jj)):
                        jump[i][j].append((ii, jj))
    return nbr, jump, cliff


def edge_sets(nbr, jump):
    """Per cell the sorted set of edge targets as cell indices lists (i * Y + j), the fixtures' form."""
    X, Y = len(nbr), len(nbr[0])
    return [sorted({r * Y + c for r, c in nbr[i][j]} | {r * Y + c for r, c in jump[i][j]}) for i in range(X) for j in range(Y)]


def bumpy_cost(hf, i, j, settings):
    """compute_bumpy_cost (astar.py:237-270) clamped and weighted: nine fp32 patch sums accumulated in double."""
    X, Y = hf.shape
    ci = np.clip(np.arange(-1, 2) + i, 0, X - 1)
    cj = np.clip(np.arange(-1, 2) + j, 0, Y - 1)
    center = hf[np.ix_(ci, cj)]
    mad = 0.0
    for a in range(-1, 2):
        for b in range(-1, 2):
            h = hf[np.ix_(np.clip(np.arange(-1, 2) + i + a, 0, X - 1), np.clip(np.arange(-1, 2) + j + b, 0, Y - 1))]
            s = F32(0.0)
            for v in np.abs(center - h).astype(F32).ravel():
                s = F32(s + v)
            mad += float(s)
    mad = mad / 81
    if mad > settings["max_bumpy"]:
        mad = settings["max_bumpy"]
    return mad * settings["w_bumpy"]


def search(hf, dx, dy, min_point, start, goal, settings, seed, query, graph=None, max_expansions=1 << 30):
    """The array-based search.  Returns a dict: status, cost (fp32), nodes [(i, j)], pops, ties, margin."""
    hf = np.asarray(hf, F32)
    X, Y = hf.shape
    N = X * Y
    nbr, jump, _ = graph if graph is not None else build_graph(hf, dx, dy, min_point, settings)
    x, y = positions(hf, dx, dy, min_point)
    w_z, w_xy = F32(settings["w_z"]), F32(settings["w_xy"])
    cmin, cmax = settings["uniform_cost_min"], settings["uniform_cost_max"]
    use_bumpy = float(settings["w_bumpy"]) != 0.0
    inf = F32(np.inf)
    g = np.full(N, inf, F32)
    f = np.full(N, inf, F32)
    opened = np.zeros(N, bool)
    parent = np.full(N, -1, np.int64)
    gi, gj = goal

    def heur(i, j):
        a, b, c = F32(x[i] - x[gi]), F32(y[j] - y[gj]), F32(hf[i, j] - hf[gi, gj])
        return np.sqrt(F32(F32(F32(a * a) + F32(b * b)) + F32(c * c)))

    s = start[0] * Y + start[1]
    goal_c = gi * Y + gj
    g[s] = F32(0.0)
    f[s] = F32(F32(0.0) + heur(*start))
    opened[s] = True
    pops, ties, margin = 0, 0, float("inf")
    status = NO_PATH
    while opened.any():
        if pops >= max_expansions:
            status = BUDGET
            break
        fo = np.where(opened, f, inf)
        order = np.lexsort((np.arange(N), g, fo))
        c = int(order[0])
        if opened.sum() > 1:
            c2 = int(order[1])
            if fo[c2] == fo[c] and g[c2] == g[c]:
                ties += 1
            margin = min(margin, float(fo[c2]) - float(fo[c]) if fo[c2] != fo[c] else abs(float(g[c2]) - float(g[c])))
        pops += 1
        opened[c] = False
        if c == goal_c:
            status = FOUND
            break
        i, j = divmod(c, Y)
        for r, q in nbr[i][j] + jump[i][j]:
            t = r * Y + q
            adz = abs(F32(hf[r, q] - hf[i, j]))
            z_cost = F32(F32(w_z * adz) * adz)
            a, b = F32(x[r] - x[i]), F32(y[q] - y[j])
            xy_cost = F32(w_xy * F32(F32(a * a) + F32(b * b)))
            total = F32(xy_cost + z_cost)
            total = F32(total + F32(bumpy_cost(hf, r, q, settings) if use_bumpy else 0.0))
            total = F32(total + edge_noise(seed, query, c, t, cmin, cmax))
            tg = F32(g[c] + total)
            if np.isfinite(g[t]) and not (parent[t] == c and tg == g[t]):
                margin = min(margin, abs(float(tg) - float(g[t])))
            if tg < g[t]:
                g[t] = tg
                f[t] = F32(tg + heur(r, q))
                opened[t] = True
                parent[t] = c
    out = dict(status=status, cost=F32(np.nan), nodes=[], pops=pops, ties=ties, margin=margin)
    if status != FOUND:
        return out
    nodes = [goal_c]
    while nodes[-1] != s:
        nodes.append(int(parent[nodes[-1]]))
    out["cost"] = g[goal_c]
    out["nodes"] = [divmod(c, Y) for c in nodes[::-1]]
    if g[goal_c] > F32(settings["max_cost"]):
        out["status"] = OVER_MAX_COST
    return out


def polyline(hf, dx, dy, min_point, nodes):
    """run_a_star_on_start_end_nodes' 3-D polyline (astar.py:408-441): long hops become torch.linspace(prev, cur, steps)[1:]."""
    hf = np.asarray(hf, F32)
    x, y = positions(hf, dx, dy, min_point)
    dxd, dyd = float(F32(dx)), float(F32(dy))
    split = math.sqrt(dxd ** 2 + dyd ** 2) + 1e-3
    pts = []
    cur = None
    for k, (i, j) in enumerate(nodes):
        prev, cur = cur, (x[i], y[j], hf[i, j])
        if k == 0:
            pts.append(cur)
            continue
        a, b = F32(cur[0] - prev[0]), F32(cur[1] - prev[1])
        dist = float(np.sqrt(F32(F32(a * a) + F32(b * b))))
        if dist > split:
            steps = int(math.ceil(dist / dxd))
            cols = []
            for p0, p1 in zip(prev, cur):
                step = F32(F32(p1 - p0) / F32(steps - 1))
                cols.append([F32(p0 + F32(step * F32(n))) if n < steps // 2 else F32(p1 - F32(step * F32(steps - n - 1))) for n in range(steps)])
            pts.extend(zip(*[c[1:] for c in cols]))
        else:
            pts.append(cur)
    return np.array(pts, F32).reshape(-1, 3)


def hop_cost(hf, dx, dy, min_point, settings, seed, query, a, b):
    """fp32 step cost of the edge a -> b (cells as (i, j)), as ``search`` evaluates it."""
    hf = np.asarray(hf, F32)
    Y = hf.shape[1]
    x, y = positions(hf, dx, dy, min_point)
    adz = abs(F32(hf[b] - hf[a]))
    z_cost = F32(F32(F32(settings["w_z"]) * adz) * adz)
    u, v = F32(x[b[0]] - x[a[0]]), F32(y[b[1]] - y[a[1]])
    total = F32(F32(F32(settings["w_xy"]) * F32(F32(u * u) + F32(v * v))) + z_cost)
    total = F32(total + F32(bumpy_cost(hf, b[0], b[1], settings) if float(settings["w_bumpy"]) != 0.0 else 0.0))
    return F32(total + edge_noise(seed, query, a[0] * Y + a[1], b[0] * Y + b[1], settings["uniform_cost_min"], settings["uniform_cost_max"]))


# ---- vectorised hop costs (the property tests at scale) ----------------------------------------------------------------------------
def philox_u0(seed, ctr_hi, ctr_lo):
    """First uniform of ``philox4`` for arrays of counters."""
    m = np.uint64(0xFFFFFFFF)
    sh = np.uint64(32)
    hi, lo = np.asarray(ctr_hi, np.uint64), np.asarray(ctr_lo, np.uint64)
    c0, c1, c2 = lo & m, hi & m, (hi >> sh) & m
    c3 = np.full_like(c0, 0x5041524B)
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = ((p1 >> sh) ^ c1 ^ k0) & m, p1 & m, ((p0 >> sh) ^ c3 ^ k1) & m, p0 & m
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m, (k1 + np.uint64(0xBB67AE85)) & m
    return (c0 >> np.uint64(8)).astype(F32) * F32(1.0 / 16777216.0)


def hop_costs(hfs, dx, dy, min_point, settings, seed, query, a, b):
    """fp32 step costs of the edges a -> b (cell indices) of queries ``query`` (indices into ``hfs`` [Q, X, Y]); ``w_bumpy`` must be 0."""
    assert float(settings["w_bumpy"]) == 0.0
    Y = hfs.shape[2]
    flat = hfs.reshape(hfs.shape[0], -1)
    x, y = positions(hfs[0], dx, dy, min_point)
    adz = np.abs((flat[query, b] - flat[query, a]).astype(F32))
    z_cost = ((F32(settings["w_z"]) * adz).astype(F32) * adz).astype(F32)
    u, v = (x[b // Y] - x[a // Y]).astype(F32), (y[b % Y] - y[a % Y]).astype(F32)
    xy_cost = (F32(settings["w_xy"]) * ((u * u).astype(F32) + (v * v).astype(F32)).astype(F32)).astype(F32)
    total = ((xy_cost + z_cost).astype(F32) + F32(0.0)).astype(F32)
    un = philox_u0(seed, query, (np.asarray(a, np.uint64) << np.uint64(16)) | np.asarray(b, np.uint64))
    noise = ((un * F32(settings["uniform_cost_max"] - settings["uniform_cost_min"])).astype(F32) + F32(settings["uniform_cost_min"])).astype(F32)
    return (total + noise).astype(F32)
