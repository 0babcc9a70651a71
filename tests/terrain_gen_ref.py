"""Numpy restatement of the procedural terrain generators: the reference's ``add_boxes_to_hf2`` (without the
``hf_maxmin`` clamp), ``gen_paths_hf`` and ``add_stairs_to_hf`` / ``draw_box`` (``terrain_util.py``) from a *plan* of derived fp32
values, in fp32 and in the reference's association, batched over terrains.  Next to each heightfield it computes the *unstable* mask:
the cells next to a decision, the only ones where two fp32 implementations may differ (``compare`` applies the rule).

Plan arrays (all fp32, first axis = terrain): ``boxes [Q, B, 6]`` = (cx, cy, lx, ly, angle, h) in index units; ``path_start [Q, P, 2]``,
``path_vy [Q, P]``, ``path_angle [Q, P]``, ``path_turn [Q, P, 1000]``, ``path_height [Q, P]``; ``stairs [Q, S, 7]`` = start xy, end xy,
start height, step height, thickness.
"""
import numpy as np

F = np.float32
PATH_POINTS = 1000
EDGE_EPS = 1e-4          # BOXES: index units; STAIRS: metres
NUDGE = 1e-2             # PATHS: cells
NUDGES = [(a, b) for a in (-1, 0, 1) for b in (-1, 0, 1) if (a, b) != (0, 0)]
MASK_CAP = {"BOXES": 0.01, "STAIRS": 0.01, "PATHS": 0.02}
HEIGHT_TOL = {"BOXES": 0.0, "PATHS": 0.0, "STAIRS": 1e-6}   # STAIRS: the reference forms step heights in double from double draws


def _box_test(x, y, cx, cy, ca, sa, hx, hy, eps):
    """draw_box's / add_boxes_to_hf2's predicate for cells (x, y) [.., X, Y] against boxes with leading axes [..]: (inside, near an edge)."""
    ux, uy = x - cx, y - cy
    rx = (ux * ca - uy * sa) + cx
    ry = (ux * sa + uy * ca) + cy
    x1, x0, y1, y0 = cx + hx, cx - hx, cy + hy, cy - hy
    inside = (rx < x1) & (rx > x0) & (ry < y1) & (ry > y0)
    e = F(eps)
    near_x = (np.abs(rx - x0) < e) | (np.abs(rx - x1) < e)
    near_y = (np.abs(ry - y0) < e) | (np.abs(ry - y1) < e)
    loose_x = (rx < x1 + e) & (rx > x0 - e)
    loose_y = (ry < y1 + e) & (ry > y0 - e)
    return inside, (near_x & loose_y) | (near_y & loose_x)


def boxes_hf(boxes, X, Y):
    """(hf [Q, X, Y], unstable [Q, X, Y]) of ``boxes [Q, B, 6]``: a later box overwrites, the heightfield starts at 0."""
    boxes = np.asarray(boxes, F)
    Q, B = boxes.shape[:2]
    x = np.arange(X, dtype=F)[None, :, None]
    y = np.arange(Y, dtype=F)[None, None, :]
    hf = np.zeros((Q, X, Y), F)
    unstable = np.zeros((Q, X, Y), bool)
    for b in range(B):
        cx, cy, lx, ly, ang, h = (boxes[:, b, k][:, None, None] for k in range(6))
        inside, near = _box_test(x, y, cx, cy, np.cos(ang), np.sin(ang), lx / F(2), ly / F(2), EDGE_EPS)
        hf = np.where(inside, h, hf).astype(F)
        unstable |= near
    return hf, unstable


def stair_steps(stairs, dx):
    """(num_steps int [..], width / dx float64 [..]) of ``stairs [.., 7]``: ceil in double of the fp32 norm over the fp32 dx."""
    s = np.asarray(stairs, F)
    ddx, ddy = s[..., 2] - s[..., 0], s[..., 3] - s[..., 1]
    ratio = np.sqrt(ddx * ddx + ddy * ddy).astype(np.float64) / np.float64(F(dx))
    return np.ceil(ratio).astype(np.int64), ratio


def stairs_hf(stairs, X, Y, dx, dy, min_point=(0.0, 0.0)):
    """(hf, unstable) of ``stairs [Q, S, 7]``: per stair ``num_steps`` boxes ``dx`` wide and ``thickness`` long along start -> end."""
    stairs = np.asarray(stairs, F)
    Q, S = stairs.shape[:2]
    x = (np.arange(X, dtype=F) * F(dx) + F(min_point[0]))[:, None]
    y = (np.arange(Y, dtype=F) * F(dy) + F(min_point[1]))[None, :]
    hf = np.zeros((Q, X, Y), F)
    unstable = np.zeros((Q, X, Y), bool)
    steps, _ = stair_steps(stairs, dx)
    for q in range(Q):
        for s in range(S):
            sx, sy, ex, ey, h0, sh, th = stairs[q, s]
            n = int(steps[q, s])
            if n <= 0:
                continue
            ddx, ddy = ex - sx, ey - sy
            ang = -np.arctan2(ddy, ddx)
            ca, sa = np.cos(ang), np.sin(ang)
            j = np.arange(n, dtype=F)[:, None, None]
            cx, cy = sx + j * (ddx / F(n)), sy + j * (ddy / F(n))
            inside, near = _box_test(x[None], y[None], cx, cy, ca, sa, F(dx) / F(2), th / F(2), EDGE_EPS)
            heights = (np.float64(h0) + np.arange(n, dtype=np.float64) * np.float64(sh)).astype(F)
            for k in range(n):
                hf[q][inside[k]] = heights[k]
            unstable[q] |= near.any(axis=0)
    return hf, unstable


def walk_paths(path_start, path_vy, path_angle, path_turn):
    """The walked points ``[Q, P, 1000, 2]`` (metres): point i is recorded before ``pos += v * dt``; then ``v`` turns by
    ``(turn_i * dt) * 7``."""
    start, vy, ang, turn = (np.asarray(a, F) for a in (path_start, path_vy, path_angle, path_turn))
    dt = F(1.0 / 30.0)
    c, s = np.cos(ang), np.sin(ang)
    vx, vy = F(1.0) * c - vy * s, F(1.0) * s + vy * c
    px, py = start[..., 0].copy(), start[..., 1].copy()
    out = np.zeros(vy.shape + (PATH_POINTS, 2), F)
    for i in range(PATH_POINTS):
        out[..., i, 0], out[..., i, 1] = px, py
        px, py = px + vx * dt, py + vy * dt
        a = (turn[..., i] * dt) * F(7.0)
        ca, sa = np.cos(a), np.sin(a)
        vx, vy = vx * ca - vy * sa, vx * sa + vy * ca
    return out


def maxpool(hf, m):
    """MaxPool2d(2 m + 1, stride 1, padding m) over the last two axes (the padding never wins)."""
    if m == 0:
        return hf.copy()
    X, Y = hf.shape[-2:]
    pad = np.full(hf.shape[:-2] + (X + 2 * m, Y + 2 * m), -np.inf, F)
    pad[..., m:m + X, m:m + Y] = hf
    out = np.full(hf.shape, -np.inf, F)
    for a in range(2 * m + 1):
        for b in range(2 * m + 1):
            out = np.maximum(out, pad[..., a:a + X, b:b + Y])
    return out


def paint_paths(cells, path_height, X, Y, dx, dy, min_point, floor_height, maxpool_size, nudge=(0.0, 0.0)):
    """The pooled heightfield from cell coordinates ``cells [Q, P, 1000, 2]`` = (xy - min_point) / dxdy, optionally nudged."""
    Q, P = cells.shape[:2]
    ix = np.clip(np.rint(cells[..., 0] + F(nudge[0])), 0, X - 1).astype(np.int64)
    iy = np.clip(np.rint(cells[..., 1] + F(nudge[1])), 0, Y - 1).astype(np.int64)
    hf = np.full((Q, X, Y), F(floor_height), F)
    q = np.arange(Q)[:, None]
    for p in range(P):
        hf[q, ix[:, p], iy[:, p]] = np.asarray(path_height, F)[:, p][:, None]
    return maxpool(hf, maxpool_size)


def paths_hf(plan, X, Y, dx, dy, min_point=(0.0, 0.0), floor_height=-3.0, maxpool_size=1):
    """(hf, unstable) of a PATHS plan: unstable = the pooled value changes under one of the eight +-1e-2-cell nudges of every point."""
    xy = walk_paths(plan["path_start"], plan["path_vy"], plan["path_angle"], plan["path_turn"])
    cells = np.stack([(xy[..., 0] - F(min_point[0])) / F(dx), (xy[..., 1] - F(min_point[1])) / F(dy)], axis=-1)
    args = (plan["path_height"], X, Y, dx, dy, min_point, floor_height, maxpool_size)
    hf = paint_paths(cells, *args)
    unstable = np.zeros(hf.shape, bool)
    for a, b in NUDGES:
        unstable |= paint_paths(cells, *args, nudge=(a * NUDGE, b * NUDGE)) != hf
    return hf, unstable


def rounding_cells(mode, plan, X, Y, dx=0.4, dy=None, min_point=(0.0, 0.0), settings=None):
    """The unstable mask alone (the name the sampler's restatement uses for the same idea)."""
    return generate(mode, plan, X, Y, dx, dy, min_point, settings)[1]


def generate(mode, plan, X, Y, dx=0.4, dy=None, min_point=(0.0, 0.0), settings=None):
    """(hf, unstable) of ``plan`` in ``mode``; ``settings`` supplies ``floor_height`` / ``maxpool_size`` for PATHS."""
    dy = dx if dy is None else dy
    if mode == "BOXES":
        return boxes_hf(plan["boxes"], X, Y)
    if mode == "STAIRS":
        return stairs_hf(plan["stairs"], X, Y, dx, dy, min_point)
    if mode == "PATHS":
        s = settings or {}
        return paths_hf(plan, X, Y, dx, dy, min_point, s.get("floor_height", -3.0), int(s.get("maxpool_size", 1)))
    raise ValueError(mode)


def compare(mode, got, want, unstable, what=""):
    """The rule: outside the mask ``got`` equals ``want`` bit for bit (STAIRS: within 1e-6).  Prints and returns how many masked cells
    differed."""
    got, want = np.asarray(got, F), np.asarray(want, F)
    assert got.shape == want.shape == unstable.shape, (got.shape, want.shape, unstable.shape)
    tol = HEIGHT_TOL[mode]
    diff = (np.abs(got.astype(np.float64) - want.astype(np.float64)) > tol) if tol else (got.view(np.uint32) != want.view(np.uint32))
    masked = int((diff & unstable).sum())
    print(f"{what or mode}: {int(unstable.sum())} of {unstable.size} cells masked, {masked} of them differ; {int((diff & ~unstable).sum())} differ outside")
    assert not (diff & ~unstable).any(), f"{what or mode}: cells outside the mask differ at {np.argwhere(diff & ~unstable)[:5].tolist()}"
    return masked


def random_plan(mode, Q, X, Y, dx, settings, rng, dy=None, min_point=(0.0, 0.0)):
    """A host-drawn plan with the ranges of ``settings`` (a dict with the reference's names): test input, not the device's draw."""
    dy = dx if dy is None else dy
    u = lambda *s: rng.random_sample(s).astype(F)  # noqa: E731
    r = lambda a, lo, hi: (a * F(hi - lo) + F(lo)).astype(F)  # noqa: E731
    if mode == "BOXES":
        B = settings["num_boxes"]
        return {"boxes": np.stack([u(Q, B) * F(X), u(Q, B) * F(Y), r(u(Q, B), settings["box_min_len"], settings["box_max_len"]),
                                   r(u(Q, B), settings["box_min_len"], settings["box_max_len"]),
                                   r(u(Q, B), settings["min_box_angle"], settings["max_box_angle"]),
                                   r(u(Q, B), settings["min_box_h"], settings["max_box_h"])], axis=-1).astype(F)}
    if mode == "PATHS":
        P = settings["num_terrain_paths"]
        return {"path_start": (np.stack([u(Q, P) * F(X * dx), u(Q, P) * F(Y * dy)], axis=-1) + np.asarray(min_point, F)).astype(F),
                "path_vy": rng.standard_normal((Q, P)).astype(F), "path_angle": u(Q, P) * F(2 * np.pi),
                "path_turn": rng.standard_normal((Q, P, PATH_POINTS)).astype(F),
                "path_height": r(u(Q, P), settings["path_min_height"], settings["path_max_height"])}
    if mode == "STAIRS":
        S = settings["num_stairs"]
        mx, my = F((X - 1) * dx), F((Y - 1) * dy)
        return {"stairs": np.stack([u(Q, S) * mx + F(min_point[0]), u(Q, S) * my + F(min_point[1]), u(Q, S) * mx + F(min_point[0]),
                                    u(Q, S) * my + F(min_point[1]),
                                    r(u(Q, S), settings["min_stair_start_height"], settings["max_stair_start_height"]),
                                    r(u(Q, S), settings["min_step_height"], settings["max_step_height"]),
                                    r(u(Q, S), settings["min_stair_thickness"], settings["max_stair_thickness"])], axis=-1).astype(F)}
    raise ValueError(mode)
