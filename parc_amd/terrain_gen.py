"""Batched procedural terrain generator: stage 2's ``BOXES``, ``PATHS`` and ``STAIRS`` procgen modes (the reference's
``terrain_util.add_boxes_to_hf2``, ``gen_paths_hf`` and ``add_stairs_to_hf`` as ``scripts/parc_2_kin_gen.py:247-290`` calls them) for
thousands of small terrains per call on the GPU.

``TerrainGenerator(mode, dim_x, dim_y, dx, settings=..., device=...)`` is one mode and one grid shape.  Every random value of a batch
comes from a *plan* (a dict of device tensors holding the derived fp32 values, ``plan_fields``): ``generate_with(plan)`` is the
deterministic path, ``draw_plan(n, seed)`` fills a plan on the device, ``generate(n, seed)`` does both in one kernel without the plan in
memory.  Terrain ``t`` of a call depends on ``(seed, first_terrain + t)`` only.  Outputs are ``hf [n, X, Y]`` fp32 on the device
(kernels: ``parc_amd/csrc/parc_terrain_gen.hpp``).  No CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
from typing import Dict, Optional

import numpy as np

from parc_amd import lib as L
from parc_amd.tool_handle import PlanCodec, ToolHandle
from parc_amd.util import path_loader

MODES = L.TGEN_MODES
MAX_DIM, MAX_BOXES, MAX_PATHS, MAX_STAIRS, MAX_POOL = L.TGEN_MAX_DIM, L.TGEN_MAX_BOXES, L.TGEN_MAX_PATHS, L.TGEN_MAX_STAIRS, L.TGEN_MAX_POOL
PATH_POINTS, MAX_STEPS, BOX_FLOATS, STAIR_FLOATS = L.TGEN_PATH_POINTS, L.TGEN_MAX_STEPS, L.TGEN_BOX_FLOATS, L.TGEN_STAIR_FLOATS
KERNELS = ("draw", "generate")   # draw_plan; generate_with / generate


class _Settings:
    """``from_config`` / ``to_config`` of a settings block: a missing key keeps the class default, an unknown one is an error."""
    BLOCK = ""

    @classmethod
    def from_config(cls, block):
        fields = {f.name: f.type for f in dataclasses.fields(cls)}
        unknown = sorted(set(block) - set(fields))
        if unknown:
            raise ValueError(f"unknown {cls.BLOCK} setting(s): {unknown}")
        return cls(**{k: (int(v) if fields[k] in (int, "int") else float(v)) for k, v in block.items()})

    def to_config(self) -> dict:
        return dataclasses.asdict(self)


@dataclasses.dataclass
class BoxesSettings(_Settings):
    """The reference's ``ProcGenBoxesSettings`` (parc_2_kin_gen.py:36-43), its names and class defaults."""
    BLOCK = "boxes"
    num_boxes: int = 10
    min_box_h: float = -3.0
    max_box_h: float = 3.0
    box_max_len: float = 10.0
    box_min_len: float = 5.0
    max_box_angle: float = 6.28318530718
    min_box_angle: float = 0.0


@dataclasses.dataclass
class PathsSettings(_Settings):
    """``ProcGenPathsSettings`` (:45-50)."""
    BLOCK = "paths"
    num_terrain_paths: int = 4
    maxpool_size: int = 1
    path_min_height: float = -2.8
    path_max_height: float = 3.0
    floor_height: float = -3.0


@dataclasses.dataclass
class StairsSettings(_Settings):
    """``ProcGenStairsSettings`` (:52-59)."""
    BLOCK = "stairs"
    min_stair_start_height: float = -3.0
    max_stair_start_height: float = 1.0
    min_step_height: float = 0.15
    max_step_height: float = 0.25
    num_stairs: int = 4
    min_stair_thickness: float = 2.0
    max_stair_thickness: float = 8.0


SETTINGS = {"BOXES": BoxesSettings, "PATHS": PathsSettings, "STAIRS": StairsSettings}


@dataclasses.dataclass
class TerrainGenConfig:
    """A terrain generator config file: the ``boxes:`` / ``paths:`` / ``stairs:`` blocks of a stage-2 config."""
    boxes: BoxesSettings = dataclasses.field(default_factory=BoxesSettings)
    paths: PathsSettings = dataclasses.field(default_factory=PathsSettings)
    stairs: StairsSettings = dataclasses.field(default_factory=StairsSettings)

    @classmethod
    def from_dict(cls, cfg) -> "TerrainGenConfig":
        unknown = sorted(set(cfg) - {"boxes", "paths", "stairs"})
        if unknown:
            raise ValueError(f"unknown terrain generator block(s): {unknown}")
        return cls(BoxesSettings.from_config(cfg.get("boxes", {})), PathsSettings.from_config(cfg.get("paths", {})),
                   StairsSettings.from_config(cfg.get("stairs", {})))

    @classmethod
    def load(cls, path) -> "TerrainGenConfig":
        return cls.from_dict(path_loader.load_config(path))

    def to_dict(self) -> dict:
        return dict(boxes=self.boxes.to_config(), paths=self.paths.to_config(), stairs=self.stairs.to_config())

    def settings(self, mode: str):
        return getattr(self, mode.lower())


def plan_fields(mode: str, settings) -> Dict[str, tuple]:
    """Per-terrain shapes of the plan's fp32 arrays of ``mode``, in the order of ``ParcTerrainGenPlan``."""
    if mode == "BOXES":
        return {"boxes": (settings.num_boxes, BOX_FLOATS)}
    if mode == "PATHS":
        P = settings.num_terrain_paths
        return {"path_start": (P, 2), "path_vy": (P,), "path_angle": (P,), "path_turn": (P, PATH_POINTS), "path_height": (P,)}
    if mode == "STAIRS":
        return {"stairs": (settings.num_stairs, STAIR_FLOATS)}
    raise ValueError(f"procgen mode {mode!r}: the generator builds {MODES}")


def check_limits(mode: str, settings, dim_x: int, dim_y: int):
    """The limits of ``parc_tgen_create``, checked before anything is allocated; each message names the macro."""
    plan_fields(mode, settings)
    if not (4 <= dim_x <= MAX_DIM and 4 <= dim_y <= MAX_DIM):
        raise ValueError(f"a {dim_x} x {dim_y} grid: sides must be 4 .. PARC_TGEN_MAX_DIM = {MAX_DIM} cells")
    if mode == "BOXES" and not 1 <= settings.num_boxes <= MAX_BOXES:
        raise ValueError(f"num_boxes = {settings.num_boxes} must be 1 .. PARC_TGEN_MAX_BOXES = {MAX_BOXES}")
    if mode == "PATHS" and not 1 <= settings.num_terrain_paths <= MAX_PATHS:
        raise ValueError(f"num_terrain_paths = {settings.num_terrain_paths} must be 1 .. PARC_TGEN_MAX_PATHS = {MAX_PATHS}")
    if mode == "PATHS" and not 0 <= settings.maxpool_size <= MAX_POOL:
        raise ValueError(f"maxpool_size = {settings.maxpool_size} must be 0 .. PARC_TGEN_MAX_POOL = {MAX_POOL}")
    if mode == "STAIRS" and not 1 <= settings.num_stairs <= MAX_STAIRS:
        raise ValueError(f"num_stairs = {settings.num_stairs} must be 1 .. PARC_TGEN_MAX_STAIRS = {MAX_STAIRS}")


def generator_params(mode: str, settings, dim_x, dim_y, dx, dy=None, min_point=(0.0, 0.0), device: int = 0):
    """``ParcTerrainGenParams`` of one mode and grid shape (the blocks of the other two modes keep their class defaults)."""
    p = L.ParcTerrainGenParams()
    p.struct_size = C.sizeof(L.ParcTerrainGenParams)
    p.device = int(device)
    p.mode = MODES.index(mode)
    p.dim_x, p.dim_y = int(dim_x), int(dim_y)
    p.dx, p.dy = float(dx), float(dx if dy is None else dy)
    p.min_point[0], p.min_point[1] = float(min_point[0]), float(min_point[1])
    blocks = {"BOXES": BoxesSettings(), "PATHS": PathsSettings(), "STAIRS": StairsSettings()}
    blocks[mode] = settings
    for m, fields in (("BOXES", L.TGEN_BOXES_FIELDS), ("PATHS", L.TGEN_PATHS_FIELDS), ("STAIRS", L.TGEN_STAIRS_FIELDS)):
        for name, t in fields:
            setattr(p, name, int(getattr(blocks[m], name)) if t == "i" else float(getattr(blocks[m], name)))
    return p


class TerrainGenerator(ToolHandle):
    """See the module docstring.  ``settings`` is the mode's dataclass (class defaults when omitted)."""
    PREFIX, KERNELS = "parc_tgen", KERNELS

    def __init__(self, mode: str, dim_x: int = 16, dim_y: int = 16, dx: float = 0.4, dy: Optional[float] = None, settings=None,
                 device="cuda:0", min_point=(0.0, 0.0)):
        if mode not in MODES:
            raise ValueError(f"procgen mode {mode!r}: the generator builds {MODES}")
        self.mode = mode
        self.settings = settings if settings is not None else SETTINGS[mode]()
        if not isinstance(self.settings, SETTINGS[mode]):
            raise ValueError(f"{mode} takes {SETTINGS[mode].__name__}, got {type(self.settings).__name__}")
        self.dim_x, self.dim_y = int(dim_x), int(dim_y)
        self.dx, self.dy = float(dx), float(dx if dy is None else dy)
        self.min_point = (float(min_point[0]), float(min_point[1]))
        check_limits(mode, self.settings, self.dim_x, self.dim_y)
        super().__init__(device)
        self.fields = plan_fields(mode, self.settings)
        self._codec = PlanCodec([(k, "f", s) for k, s in self.fields.items()], L.ParcTerrainGenPlan)
        self._create_handle(generator_params(mode, self.settings, self.dim_x, self.dim_y, self.dx, self.dy, self.min_point, self.device_index))

    # ------------------------------------------------------------------ plans
    def empty_plan(self, n: int, zero: bool = True):
        """The plan's device arrays; ``zero=False`` leaves them uninitialised (``draw_plan`` writes every entry)."""
        return self._codec.empty(n, self.device, zero)

    def plan_from_numpy(self, arrays: Dict[str, np.ndarray]):
        """A plan from host arrays ``[n, ...]``; every field of the mode is required."""
        return self._codec.from_numpy(arrays, self.device, required=tuple(self.fields))

    def _plan_struct(self, plan):
        return self._codec.struct(plan, self.device)

    def _hf(self, n):
        import torch
        return torch.empty((n, self.dim_x, self.dim_y), dtype=torch.float32, device=self.device)

    # ------------------------------------------------------------------ generation
    def draw_plan(self, n: int, seed: int, first_terrain: int = 0):
        plan = self.empty_plan(n, zero=False)
        st, _ = self._plan_struct(plan)
        self._call("draw_plan", C.c_uint64(int(seed)), C.c_uint64(int(first_terrain)), C.byref(st), self._stream())
        return plan

    def generate_with(self, plan, validate: bool = False):
        """``hf [n, X, Y]`` of ``plan``.  ``validate`` runs a pass over the plan first and synchronises: a non-finite entry (or a stair
        of more than ``PARC_TGEN_MAX_STEPS`` steps) raises, naming the field, and the generator is not launched."""
        st, n = self._plan_struct(plan)
        hf = self._hf(n)
        self._call("generate_with", C.byref(st), hf.data_ptr(), int(bool(validate)), self._stream())
        return hf

    def generate(self, n: int, seed: int, first_terrain: int = 0):
        if int(n) < 1:
            raise ValueError("n must be >= 1")
        hf = self._hf(int(n))
        self._call("generate", int(n), C.c_uint64(int(seed)), C.c_uint64(int(first_terrain)), hf.data_ptr(), self._stream())
        return hf
