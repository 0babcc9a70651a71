"""Batched terrain path planner: stage 2's A* search (the reference's ``motion_synthesis/procgen/astar.py`` as
``scripts/parc_2_kin_gen.py:310-337`` drives it) for many small terrains at once on the GPU.

``TerrainPathPlanner(device).plan(hfs)`` plans one path per heightfield ``[Q, X, Y]``: the start / goal cells are injected or drawn on
the device near the border, the terrain is optionally simplified (``flat_maxpool_2x2`` + ``flatten_4x4_near_edge``), the navigation
graph (walk edges within ``max_z_diff``, jump edges between cliff cells with a line of sight) is searched and the path returned as
cells and as the reference's 3-D polyline (``parc_amd/csrc/parc_path_planner.hpp``).  ``plan_terrains`` is the
reference's retry loop run wide.  Two stated differences from the reference: the step-cost noise is a function of
``(seed, query, from cell, to cell)`` instead of a global stream, and ``max_compute_time`` is an expansion budget.  No CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
from typing import List, Optional

import numpy as np

from parc_amd import lib as L
from parc_amd.tool_handle import ToolHandle
from parc_amd.util import path_loader

STATUS_NAMES = L.PATHPLAN_STATUS
FOUND, NO_PATH, OVER_MAX_COST, BUDGET, NO_DRAW = range(len(STATUS_NAMES))
MAX_DIM, MAX_JUMP_RADIUS, JUMP_WORDS = L.PATHPLAN_MAX_DIM, L.PATHPLAN_MAX_JUMP_RADIUS, L.PATHPLAN_JUMP_WORDS
KERNELS = ("prepare", "search", "graph")   # the two phases of the last plan, and the last graph
DIRECTIONS = ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (-1, 1), (1, -1), (1, 1))   # astar.py:112, the bits of the neighbour mask


@dataclasses.dataclass
class AStarSettings:
    """The reference's ``AStarSettings`` (astar.py:12-24), its names and class defaults."""
    max_z_diff: float = 2.1
    max_jump_xy_dist: float = 3.0
    max_jump_z_diff: float = 0.3
    min_jump_z_diff: float = -0.7
    w_z: float = 0.15
    w_xy: float = 1.0
    w_bumpy: float = 1.0
    max_bumpy: float = 0.2
    uniform_cost_max: float = 0.25
    uniform_cost_min: float = 0.0
    min_start_end_xy_dist: float = 4.0
    max_cost: float = 1000.0

    @classmethod
    def from_config(cls, block) -> "AStarSettings":
        """The ``astar:`` block of a stage-2 config; a missing key keeps the class default, an unknown one is an error."""
        names = {f.name for f in dataclasses.fields(cls)}
        unknown = sorted(set(block) - names)
        if unknown:
            raise ValueError(f"unknown astar setting(s): {unknown}")
        return cls(**{k: float(v) for k, v in block.items()})

    def to_config(self) -> dict:
        return dataclasses.asdict(self)


@dataclasses.dataclass
class PlannerConfig:
    """A path planner config file: the ``astar:`` block plus stage 2's terrain and retry keys."""
    astar: AStarSettings
    simplify_terrain: bool = True
    num_attempts: int = 10
    new_terrain_dim_x: int = 16
    new_terrain_dim_y: int = 16
    dx: float = 0.4
    dy: float = 0.4
    max_expansions: int = 65536

    @classmethod
    def from_dict(cls, cfg) -> "PlannerConfig":
        keys = {f.name for f in dataclasses.fields(cls)} - {"astar"}
        return cls(astar=AStarSettings.from_config(cfg.get("astar", {})), **{k: type(getattr(cls, k))(cfg[k]) for k in keys if k in cfg})

    @classmethod
    def load(cls, path) -> "PlannerConfig":
        return cls.from_dict(path_loader.load_config(path))

    def to_dict(self) -> dict:
        d = dataclasses.asdict(self)
        d["astar"] = self.astar.to_config()
        return d


@dataclasses.dataclass
class PathPlan:
    """The planner's outputs for Q queries (numpy, host)."""
    status: np.ndarray            # [Q] FOUND / NO_PATH / OVER_MAX_COST / BUDGET / NO_DRAW
    cost: np.ndarray              # [Q] fp32, NaN unless a path reached the goal
    nodes: List[np.ndarray]       # per query int32 [n, 2] cells (i, j), start and goal included; empty unless a path reached the goal
    points: List[np.ndarray]      # per query fp32 [m, 3] the polyline of a FOUND query
    start: np.ndarray             # [Q, 2]
    goal: np.ndarray              # [Q, 2]
    hf: np.ndarray                # [Q, X, Y] the heightfield searched (simplified when simplify_terrain)
    pops: np.ndarray              # [Q] cells popped

    @property
    def found(self) -> np.ndarray:
        return self.status == FOUND


def planner_params(settings: AStarSettings, dim_x, dim_y, dx, dy, min_point=(0.0, 0.0), simplify_terrain=True, max_expansions=65536,
                   max_nodes=None, max_points=None, device: int = 0):
    """``ParcPathPlanParams`` for one grid shape."""
    p = L.ParcPathPlanParams()
    p.struct_size = C.sizeof(L.ParcPathPlanParams)
    p.device = int(device)
    p.dim_x, p.dim_y = int(dim_x), int(dim_y)
    p.dx, p.dy = float(dx), float(dy)
    p.min_point[0], p.min_point[1] = float(min_point[0]), float(min_point[1])
    for name in L.PATHPLAN_SETTINGS:
        setattr(p, name, float(getattr(settings, name)))
    p.simplify_terrain = int(bool(simplify_terrain))
    p.max_expansions = int(max_expansions)
    cells = int(dim_x) * int(dim_y)
    p.max_nodes = int(max_nodes if max_nodes is not None else cells)
    p.max_points = int(max_points if max_points is not None else cells)
    return p


def jump_radius(settings: AStarSettings, dx) -> int:
    return int(math.ceil(float(settings.max_jump_xy_dist) / float(np.float32(dx))))


def edges_from_graph(nbr, jump, radius):
    """Per cell the sorted edge targets (cell indices) from ``graph``'s neighbour masks ``[X, Y]`` and jump bits ``[X, Y, JUMP_WORDS]``."""
    X, Y = nbr.shape
    W = 2 * radius
    out = []
    for i in range(X):
        for j in range(Y):
            e = {(i + a) * Y + j + b for d, (a, b) in enumerate(DIRECTIONS) if (int(nbr[i, j]) >> d) & 1}
            words = jump[i, j]
            if words.any():
                for k in range(W * W):
                    if (int(words[k >> 5]) >> (k & 31)) & 1:
                        e.add((i - radius + k // W) * Y + j - radius + k % W)
            out.append(sorted(e))
    return out


def select_first_success(status, num_terrains, num_attempts):
    """Per terrain the index of its first FOUND attempt in attempt order (queries laid out ``[terrain][attempt]``), -1 when none: the
    reference's loop stops at the first attempt whose path exists (parc_2_kin_gen.py:310-337)."""
    ok = np.asarray(status).reshape(num_terrains, num_attempts) == FOUND
    first = np.argmax(ok, axis=1)
    return np.where(ok.any(axis=1), first, -1).astype(np.int64)


class TerrainPathPlanner(ToolHandle):
    """``TerrainPathPlanner(device, settings).plan(hfs)``; one handle per grid shape, rebuilt when the shape or ``dx`` changes."""
    PREFIX, KERNELS, DEVICE_CONTEXT = "parc_pathplan", KERNELS, False

    def __init__(self, device="cuda:0", settings: Optional[AStarSettings] = None, simplify_terrain=True, max_expansions=65536,
                 min_point=(0.0, 0.0), max_nodes=None, max_points=None):
        super().__init__(device)
        self.settings = settings if settings is not None else AStarSettings()
        self.simplify_terrain = bool(simplify_terrain)
        self.max_expansions = int(max_expansions)
        self.min_point = (float(min_point[0]), float(min_point[1]))
        self.max_nodes, self.max_points = max_nodes, max_points
        self._key = None
        self._params = None

    def _handle(self, X, Y, dx, dy):
        key = (X, Y, float(np.float32(dx)), float(np.float32(dy)))
        if self._h is None or key != self._key:
            self._destroy()
            p = planner_params(self.settings, X, Y, dx, dy, self.min_point, self.simplify_terrain, self.max_expansions, self.max_nodes,
                               self.max_points, self.device_index)
            self._create_handle(p)
            self._key, self._params = key, p

    def plan(self, hfs, starts=None, goals=None, seed: int = 0, dx: float = 0.4, dy: Optional[float] = None, first_query: int = 0) -> PathPlan:
        """Plan one path per heightfield of ``hfs`` ``[Q, X, Y]``.  ``starts`` / ``goals`` ``[Q, 2]`` inject the cells; without them
        both are drawn on the device from ``(seed, first_query + q)``."""
        hfs = np.ascontiguousarray(hfs, np.float32)
        if hfs.ndim != 3:
            raise ValueError("hfs must be [Q, X, Y]")
        Q, X, Y = hfs.shape
        self._handle(X, Y, dx, dx if dy is None else dy)
        p = self._params
        if (starts is None) != (goals is None):
            raise ValueError("starts and goals go together")
        s = g = None
        if starts is not None:
            s = np.ascontiguousarray(starts, np.int32).reshape(Q, 2)
            g = np.ascontiguousarray(goals, np.int32).reshape(Q, 2)
        shapes = dict(status=(Q,), cost=(Q,), num_nodes=(Q,), nodes=(Q, p.max_nodes), num_points=(Q,), points=(Q, p.max_points, 3), start=(Q, 2),
                      goal=(Q, 2), hf=(Q, X, Y), pops=(Q,))
        arr = {n: np.zeros(shapes[n], np.float32 if t == "f" else np.int32) for n, t in L.PATHPLAN_OUTPUT_FIELDS}
        out = L.ParcPathPlanOutputs()
        for n, t in L.PATHPLAN_OUTPUT_FIELDS:
            setattr(out, n, L.np_f32p(arr[n]) if t == "f" else L.np_i32p(arr[n]))
        self._call("run", Q, L.np_f32p(hfs), L.np_i32p(s) if s is not None else None, L.np_i32p(g) if g is not None else None, int(seed),
                   int(first_query), C.byref(out))
        nn, npt = arr["num_nodes"], arr["num_points"]
        if nn.max(initial=0) > p.max_nodes or npt.max(initial=0) > p.max_points:
            raise L.ParcError(f"a path has {int(nn.max())} cells / {int(npt.max())} points, above max_nodes = {p.max_nodes} / max_points = "
                              f"{p.max_points}: construct the planner with larger limits")
        nodes = [np.stack(np.divmod(arr["nodes"][q, :nn[q]], Y), axis=1).astype(np.int32) for q in range(Q)]
        points = [arr["points"][q, :npt[q]].copy() for q in range(Q)]
        return PathPlan(arr["status"], arr["cost"], nodes, points, arr["start"], arr["goal"], arr["hf"], arr["pops"])

    def graph(self, q0: int = 0, n: int = 1):
        """The navigation graph of queries ``[q0, q0 + n)`` of the last ``plan``: neighbour masks uint8 ``[n, X, Y]`` (bit d =
        ``DIRECTIONS[d]``), cliff flags ``[n, X, Y]``, jump bits uint32 ``[n, X, Y, JUMP_WORDS]`` (``edges_from_graph`` expands them)."""
        X, Y = self._key[0], self._key[1]
        nbr = np.zeros((n, X, Y), np.uint8)
        cliff = np.zeros((n, X, Y), np.uint8)
        jump = np.zeros((n, X, Y, JUMP_WORDS), np.uint32)
        u8 = C.POINTER(C.c_uint8)
        self._call("get_graph", int(q0), int(n), nbr.ctypes.data_as(u8), cliff.ctypes.data_as(u8), jump.ctypes.data_as(C.POINTER(C.c_uint32)))
        return nbr, cliff, jump

    def plan_terrains(self, hfs, num_attempts: int = 10, seed: int = 0, dx: float = 0.4, dy: Optional[float] = None):
        """The reference's retry loop run wide: ``num_attempts`` start / goal draws per terrain, all ``Q x num_attempts`` queries in one
        batch (query index ``terrain * num_attempts + attempt``); per terrain the FIRST successful attempt in attempt order wins.
        Returns ``(attempt [Q] (-1 = none succeeded), PathPlan of the Q winning queries (attempt 0 where none succeeded))``."""
        hfs = np.ascontiguousarray(hfs, np.float32)
        Q = hfs.shape[0]
        plan = self.plan(np.repeat(hfs, num_attempts, axis=0), seed=seed, dx=dx, dy=dy)
        attempt = select_first_success(plan.status, Q, num_attempts)
        pick = np.arange(Q) * num_attempts + np.maximum(attempt, 0)
        sel = PathPlan(plan.status[pick], plan.cost[pick], [plan.nodes[i] for i in pick], [plan.points[i] for i in pick], plan.start[pick],
                       plan.goal[pick], plan.hf[pick], plan.pops[pick])
        return attempt, sel
