"""Batched motion-terrain augmenter: the reference's ``scripts/run_simple_augment_motions.py`` (a window of a source clip, turned about
the origin, stretched in x and y, on its terrain padded, sliced around the motion and re-anchored at frame 0, with the heights scaled or
rotated boxes dropped under frames of the motion) and stage 2's mirrored copies (``parc_2_kin_gen.py:490-495``) for thousands of
variations per call on the GPU.

``MotionAugmenter(char_file, clips, settings, device)`` holds the source clips (``OptClip``).  Every random value of a batch comes from a
*plan* (a dict of device tensors holding the derived values, ``plan_fields``): ``augment_with(plan)`` is the deterministic path,
``draw_plan(n, seed)`` fills a plan on the device, ``augment(n, seed)`` does both without the plan in memory.  Variation ``v`` of a call
depends on ``(seed, first + v)`` only.  The result keeps the variations concatenated on the device (they differ in frame count and slice
size); ``result.to_opt_clips()`` hands them to ``MotionOptimizer``.  ``mirror_clips(clips)`` is the mirrored copy of every clip, unchanged
otherwise (kernels: ``parc_amd/csrc/parc_motion_aug.hpp``).  No CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
from typing import Dict, List, Optional, Sequence

import numpy as np

from parc_amd import lib as L
from parc_amd.char_model import CharModel
from parc_amd.tool_handle import PlanCodec, ToolHandle, fill_struct
from parc_amd.util import path_loader

MODES = L.MAUG_MODES                                       # TerrainAugmentationType (run_simple_augment_motions.py:19-22)
MAX_DIM, MAX_BOXES, BOX_FLOATS = L.MAUG_MAX_DIM, L.MAUG_MAX_BOXES, L.MAUG_BOX_FLOATS
STATUS_CLAMPED, STATUS_NOT_FINITE = L.MAUG_STATUS_CLAMPED, L.MAUG_STATUS_NOT_FINITE
KERNELS = ("draw", "layout", "frames", "terrain")          # draw_plan, and the three phases of a run
# the keys of the reference script's config that belong to the optimiser and the driver, not to the augmenter
DRIVER_KEYS = ("motions_yaml_path", "device", "char_model", "num_new_motions", "output_folder_path", "num_iters", "step_size", "w_root_pos",
               "w_root_rot", "w_joint_rot", "w_smoothness", "w_penetration", "w_contact", "w_sliding", "w_body_constraints", "w_jerk", "max_jerk",
               "log_every", "use_wandb", "char_point_samples")


@dataclasses.dataclass
class MotionAugSettings:
    """The augmenter's keys of the reference script's config (``run_simple_augment_motions.py:78-108``), under their names."""
    max_motion_len: float = 10.0
    min_heading_angle: float = -180.0       # degrees
    max_heading_angle: float = 180.0
    terrain_padding_size: int = 10
    slice_terrain: bool = True
    x_scale: Sequence[float] = (0.9, 1.1)
    y_scale: Sequence[float] = (0.9, 1.1)
    sample_weight_by_length: bool = True
    terrain_aug_type: str = "HEIGHT_SCALE"
    min_h_scale: float = 0.5                # HEIGHT_SCALE
    max_h_scale: float = 1.5
    bad_h_range: Sequence[float] = (0.0, 0.0)
    min_len: float = 2.0                    # BOXES_ALONG_PATH: side lengths in cells
    max_len: float = 6.0
    min_angle: float = 0.0
    max_angle: float = 6.28318530718
    min_num_boxes: int = 1
    max_num_boxes: int = 4
    min_h: float = -1.0
    max_h: float = 1.0

    @classmethod
    def from_config(cls, cfg: dict) -> "MotionAugSettings":
        """From a config mapping: a missing key keeps the class default, an unknown one is an error (the optimiser's and the driver's
        keys of the same file, ``DRIVER_KEYS``, are left to their readers)."""
        fields = {f.name: f for f in dataclasses.fields(cls)}
        unknown = sorted(set(cfg) - set(fields) - set(DRIVER_KEYS))
        if unknown:
            raise ValueError(f"unknown motion augmenter setting(s): {unknown}")
        kw = {}
        for k, v in cfg.items():
            if k not in fields:
                continue
            if k in ("x_scale", "y_scale", "bad_h_range"):
                if not isinstance(v, (list, tuple)) or len(v) != 2:
                    raise ValueError(f"{k} must be a pair [min, max]")
                kw[k] = (float(v[0]), float(v[1]))
            elif k == "terrain_aug_type":
                kw[k] = str(v)
            elif k in ("slice_terrain", "sample_weight_by_length"):
                kw[k] = bool(v)
            elif k in ("terrain_padding_size", "min_num_boxes", "max_num_boxes"):
                kw[k] = int(v)
            else:
                kw[k] = float(v)
        s = cls(**kw)
        s.check()
        return s

    def to_config(self) -> dict:
        d = dataclasses.asdict(self)
        for k in ("x_scale", "y_scale", "bad_h_range"):
            d[k] = [float(d[k][0]), float(d[k][1])]
        return d

    def check(self):
        """The refusals of ``parc_maug_create``, before anything is allocated; each message names its key or macro."""
        if self.terrain_aug_type not in MODES:
            raise ValueError(f"terrain_aug_type {self.terrain_aug_type!r}: the augmenter builds {MODES}")
        if not self.max_motion_len > 0:
            raise ValueError("max_motion_len must be > 0")
        if not 0 <= self.terrain_padding_size <= MAX_DIM:
            raise ValueError(f"terrain_padding_size = {self.terrain_padding_size} must be 0 .. PARC_MAUG_MAX_DIM = {MAX_DIM}")
        if self.terrain_aug_type == "HEIGHT_SCALE":
            lo, hi, (b0, b1) = np.float32(self.min_h_scale), np.float32(self.max_h_scale), np.float32(self.bad_h_range)
            if not lo <= hi:
                raise ValueError("min_h_scale must be <= max_h_scale")
            cut = b0 < b1 and b0 < hi and b1 > lo
            length = (max(b0, lo) - lo) + (hi - min(b1, hi)) if cut else hi - lo
            if (lo < hi and not length > 0) or (lo == hi and b0 < lo < b1):   # the reference's rejection loop would spin for ever
                raise ValueError(f"bad_h_range ({b0}, {b1}) swallows [min_h_scale, max_h_scale] = [{lo}, {hi}]: no height scale could be drawn")
        if self.terrain_aug_type == "BOXES_ALONG_PATH" and not 0 <= self.min_num_boxes <= self.max_num_boxes <= MAX_BOXES:
            raise ValueError(f"0 <= min_num_boxes <= max_num_boxes = {self.max_num_boxes} <= PARC_MAUG_MAX_BOXES = {MAX_BOXES}")


def load_config(path) -> dict:
    cfg = path_loader.load_config(path)
    if not isinstance(cfg, dict):
        raise ValueError(f"{path}: not a mapping")
    return cfg


def swap_tables(char_model: CharModel):
    """``(joint_swap [B], contact_swap [B])``: the ``left_`` / ``right_`` partner of every joint (by joint name) and of every contact
    body's column of a per-body contacts array (by contact body name), the index itself for the rest: what
    ``flip_motion_about_XZ_plane`` (motion_edit_lib.py:350-390) derives from the names."""
    def mirror_name(name):
        if name.startswith("left_"):
            return "right_" + name[len("left_"):]
        if name.startswith("right_"):
            return "left_" + name[len("right_"):]
        return None

    def pair(names_to_index, table):
        for name, i in names_to_index.items():
            m = mirror_name(name)
            if m is None:
                continue
            if m not in names_to_index:
                raise ValueError(f"Missing symmetric counterpart for {name}")
            table[i] = names_to_index[m]

    B = char_model.get_num_bodies()
    jswap, cswap = np.arange(B, dtype=np.int32), np.arange(B, dtype=np.int32)
    pair({char_model.get_joint(j).name: j for j in range(1, B)}, jswap)
    pair({n: int(i) for n, i in zip(char_model._contact_body_names, char_model.get_contact_body_ids())}, cswap)
    return jswap, cswap


def plan_fields() -> Dict[str, tuple]:
    """``name -> (dtype char "i" / "f", per-variation shape)`` of the plan's arrays, in the order of ``ParcMotionAugPlan``."""
    return {n: (t, s) for n, t, s in L.MAUG_PLAN_FIELDS}


class AugResult:
    """The variations of one run, concatenated on the device: ``frame_off`` / ``cell_off [n + 1]``, ``src_clip [n]``, ``hf_dims [n, 2]``,
    ``hf_geom [n, 4]`` (min x, min y, dx, dy), ``canon_z [n]``, ``root_pos [F, 3]``, ``root_rot [F, 4]``, ``joint_rot [F, J, 4]``,
    ``contacts [F, B]``, ``hf [cells]`` (x-major per variation), ``hf_maxmin [cells, 2]`` or ``None``."""

    def __init__(self, tensors: dict, sources: List, names: List[str]):
        self.__dict__.update(tensors)
        self._tensors, self._sources, self._names = tensors, sources, names
        self.n = int(tensors["src_clip"].shape[0])

    def numpy(self) -> Dict[str, Optional[np.ndarray]]:
        return {k: (None if t is None else t.cpu().numpy()) for k, t in self._tensors.items()}

    def variations(self) -> List[dict]:
        """Per variation, on the host: ``root_pos``, ``root_rot``, ``joint_rot``, ``contacts``, ``hf [X, Y]``, ``hf_maxmin`` or ``None``,
        ``hf_dims``, ``min_point``, ``dx``, ``canon_z``, ``src_clip``."""
        a = self.numpy()
        out = []
        for v in range(self.n):
            f0, f1, c0, c1 = int(a["frame_off"][v]), int(a["frame_off"][v + 1]), int(a["cell_off"][v]), int(a["cell_off"][v + 1])
            X, Y = (int(d) for d in a["hf_dims"][v])
            out.append(dict(root_pos=a["root_pos"][f0:f1], root_rot=a["root_rot"][f0:f1], joint_rot=a["joint_rot"][f0:f1], contacts=a["contacts"][f0:f1],
                            hf=a["hf"][c0:c1].reshape(X, Y), hf_maxmin=None if a["hf_maxmin"] is None else a["hf_maxmin"][c0:c1].reshape(X, Y, 2),
                            hf_dims=a["hf_dims"][v], min_point=a["hf_geom"][v, :2].copy(), dx=np.float32(a["hf_geom"][v, 2]),
                            canon_z=a["canon_z"][v], src_clip=int(a["src_clip"][v])))
        return out

    def to_opt_clips(self, names: Optional[Sequence[str]] = None):
        """``OptClip`` s for ``MotionOptimizer`` (fps of the source clip; ``names`` default to ``<source>_aug###`` counted per source
        from 1, the reference's numbering)."""
        from parc_amd.motion_opt import OptClip
        count: Dict[int, int] = {}
        clips = []
        for v, d in enumerate(self.variations()):
            c = d["src_clip"]
            count[c] = count.get(c, 0) + 1
            name = names[v] if names is not None else f"{self._names[c]}_aug{str(count[c]).zfill(3)}"
            clips.append(OptClip(d["root_pos"].copy(), d["root_rot"].copy(), d["joint_rot"].copy(), d["contacts"].copy(), d["hf"].copy(), d["min_point"],
                                 float(d["dx"]), int(self._sources[c].fps), name,
                                 hf_maxmin=None if d["hf_maxmin"] is None else d["hf_maxmin"].copy()))
        return clips


class MotionAugmenter(ToolHandle):
    """See the module docstring.  ``clips`` are ``OptClip`` s (``motion_opt.clip_from_ms``); ``settings`` a ``MotionAugSettings`` or a
    config mapping.  ``hf_maxmin`` rides along when every clip carries one."""
    PREFIX, KERNELS = "parc_maug", KERNELS

    def __init__(self, char_file: str, clips, settings=None, device="cuda:0"):
        from parc_amd.motion_opt import clip_struct, pack_clips
        if settings is None:
            settings = MotionAugSettings()
        elif isinstance(settings, dict):
            settings = MotionAugSettings.from_config(settings)
        settings.check()
        self.settings = settings
        self.mode = settings.terrain_aug_type
        self.char_file = char_file
        self.char_model = CharModel(char_file)
        self.B = self.char_model.get_num_bodies()
        self.clips = list(clips)
        if not self.clips:
            raise ValueError("no clips")
        self.clip_names = [c.name or f"clip{i}" for i, c in enumerate(self.clips)]
        super().__init__(device)
        self._codec = PlanCodec(L.MAUG_PLAN_FIELDS, L.ParcMotionAugPlan)
        self.joint_swap, self.contact_swap = swap_tables(self.char_model)
        s = settings
        p = L.ParcMotionAugParams()
        p.device = self.device_index
        p.model = L.make_char_model(self.char_model)
        for b in range(L.MAX_BODIES):
            p.joint_swap[b] = int(self.joint_swap[b]) if b < self.B else b
            p.contact_swap[b] = int(self.contact_swap[b]) if b < self.B else b
        p.mode, p.terrain_padding_size = MODES.index(self.mode), int(s.terrain_padding_size)
        p.slice_terrain, p.sample_weight_by_length = int(bool(s.slice_terrain)), int(bool(s.sample_weight_by_length))
        p.min_heading_angle, p.max_heading_angle = float(s.min_heading_angle), float(s.max_heading_angle)
        p.x_scale[0], p.x_scale[1], p.y_scale[0], p.y_scale[1] = (float(v) for v in (*s.x_scale, *s.y_scale))
        p.min_h_scale, p.max_h_scale = float(s.min_h_scale), float(s.max_h_scale)
        p.bad_h_range[0], p.bad_h_range[1] = float(s.bad_h_range[0]), float(s.bad_h_range[1])
        p.min_num_boxes, p.max_num_boxes = int(s.min_num_boxes), int(s.max_num_boxes)
        p.min_len, p.max_len, p.min_angle, p.max_angle, p.min_h, p.max_h = (float(v) for v in (s.min_len, s.max_len, s.min_angle, s.max_angle,
                                                                                                 s.min_h, s.max_h))
        self._create_handle(p)
        pk = pack_clips(self.clips, self.B, self.char_model.get_dof_size())
        st = clip_struct(pk, len(self.clips))
        self.has_maxmin = all(c.hf_maxmin is not None for c in self.clips)
        info = L.ParcMotionAugClipInfo()
        if self.has_maxmin:
            maxmin = np.ascontiguousarray(np.concatenate([np.asarray(c.hf_maxmin, np.float32).reshape(-1, 2) for c in self.clips]))
            if maxmin.shape[0] != pk["hf_off"][-1]:
                raise ValueError("hf_maxmin does not match the heightfields")
            info.hf_maxmin_host = L.np_f32p(maxmin)
        fps = np.array([int(c.fps) for c in self.clips], np.int32)
        self.max_frames = np.array([int(round(int(c.fps) * float(s.max_motion_len))) for c in self.clips], np.int32)   # :152
        info.fps_host, info.max_frames_host = L.np_i32p(fps), L.np_i32p(self.max_frames)
        self._call("set_clips", C.byref(st), C.byref(info))
        self.num_frames = np.diff(pk["frame_off"]).astype(np.int64)
        w = (self.num_frames / fps).astype(np.float32) if s.sample_weight_by_length else np.ones(len(self.clips), np.float32)
        self.weights = w.astype(np.float64) / w.astype(np.float64).sum()

    # ------------------------------------------------------------------ plans
    plan_fields = staticmethod(plan_fields)

    def empty_plan(self, n: int, zero: bool = True):
        return self._codec.empty(n, self.device, zero)

    def plan_from_numpy(self, arrays: Dict[str, np.ndarray]):
        """A plan from host arrays ``[n, ...]``.  ``src_clip``, ``start_frame``, ``num_frames`` are required; a missing ``heading`` is 0,
        ``scale`` 1, ``mirror`` 0, ``height_scale`` 1, and no boxes."""
        return self._codec.from_numpy(arrays, self.device, required=("src_clip", "start_frame", "num_frames"),
                                      defaults=dict(scale=1.0, height_scale=1.0), reject_unknown=True)

    def _plan_struct(self, plan):
        return self._codec.struct(plan, self.device)

    def draw_plan(self, n: int, seed: int, first: int = 0, mirror: bool = False):
        plan = self.empty_plan(n, zero=False)
        st, _ = self._plan_struct(plan)
        self._call("draw_plan", C.c_uint64(int(seed)), C.c_uint64(int(first)), int(bool(mirror)), C.byref(st), self._stream())
        return plan

    # ------------------------------------------------------------------ augmentation
    def _result(self, sizes) -> AugResult:
        import torch
        n, F, cells, J = int(sizes.n), int(sizes.total_frames), int(sizes.total_cells), self.B - 1
        f32, i32, i64 = torch.float32, torch.int32, torch.int64
        shapes = dict(frame_off=((n + 1,), i64), cell_off=((n + 1,), i64), src_clip=((n,), i32), hf_dims=((n, 2), i32), hf_geom=((n, 4), f32),
                      canon_z=((n,), f32), root_pos=((F, 3), f32), root_rot=((F, 4), f32), joint_rot=((F, J, 4), f32), contacts=((F, self.B), f32),
                      hf=((cells,), f32), hf_maxmin=((cells, 2), f32))
        t = {k: torch.empty(s, dtype=d, device=self.device) for k, (s, d) in shapes.items() if k != "hf_maxmin" or sizes.has_maxmin}
        self._call("get_result", C.byref(fill_struct(L.ParcMotionAugOutputs, t)), self._stream())
        t.setdefault("hf_maxmin", None)
        return AugResult(t, self.clips, self.clip_names)

    def augment_with(self, plan, validate: bool = False) -> AugResult:
        """The variations of ``plan``.  ``validate`` runs a pass over the plan first: a non-finite or out-of-range entry raises, naming
        the field, and nothing is launched.  Without it a bad index is clamped into its range (``status()`` tells) and a non-finite
        value stays inside its own variation."""
        st, _ = self._plan_struct(plan)
        sizes = L.ParcMotionAugSizes()
        self._call("augment_with", C.byref(st), int(bool(validate)), self._stream(), C.byref(sizes))
        return self._result(sizes)

    def augment(self, n: int, seed: int, first: int = 0, mirror: bool = False) -> AugResult:
        if int(n) < 1:
            raise ValueError("n must be >= 1")
        sizes = L.ParcMotionAugSizes()
        self._call("augment", int(n), C.c_uint64(int(seed)), C.c_uint64(int(first)), int(bool(mirror)), self._stream(), C.byref(sizes))
        return self._result(sizes)

    def mirror_clips(self, clips):
        """``mirror_clips(clips, ...)`` with this augmenter's character and device."""
        return mirror_clips(clips, self.char_file, self.device)

    def status(self) -> int:
        """The OR of ``STATUS_CLAMPED`` / ``STATUS_NOT_FINITE`` since the last call (synchronises)."""
        v = np.zeros(1, np.int32)
        self._call("plan_status", self._stream(), L.np_i32p(v))
        return int(v[0])


def mirror_plan(num_frames: Sequence[int]) -> Dict[str, np.ndarray]:
    """The plan of ``mirror_clips``: every clip once, its full window, heading 0, scale 1, no edit, mirror on."""
    n = len(num_frames)
    return dict(src_clip=np.arange(n, dtype=np.int32), start_frame=np.zeros(n, np.int32), num_frames=np.asarray(num_frames, np.int32),
                mirror=np.ones(n, np.int32))


def mirror_clips(clips, char_file: str, device="cuda:0"):
    """The mirrored copy of every clip (``flip_motion_about_XZ_plane`` + ``SubTerrain.flip_by_XZ_axis``), unchanged otherwise: same
    frames, same terrain cells, names with ``_flipped`` appended."""
    s = MotionAugSettings(terrain_aug_type="NONE", terrain_padding_size=0, slice_terrain=False)
    aug = MotionAugmenter(char_file, clips, s, device)
    res = aug.augment_with(aug.plan_from_numpy(mirror_plan([c.num_frames for c in clips])), validate=True)
    return res.to_opt_clips([(c.name or f"clip{i}") + "_flipped" for i, c in enumerate(clips)])
