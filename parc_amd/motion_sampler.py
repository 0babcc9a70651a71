"""Motion-window sampler for generator training: the reference's ``MDMHeightfieldContactMotionSampler``
(``PARC/motion_generator/mdm_heightfield_contact_motion_sampler.py``) for a whole batch on the GPU.

``MotionWindowSampler(cfg, motion_file, char_file, device)`` takes the reference's config keys unchanged (see
``data/configs/motion_sampler/motion_sampler_default.yaml``), loads an ms file or a dataset YAML and keeps the library resident on the
device: frames, terrains, ``hf_maxmin`` and the per-frame ``hf_mask_inds`` (CSR).  Files without ``hf_mask_inds`` are analysed on load
with :class:`parc_amd.motion_terrain.MotionTerrainAnalyzer` (one batched run; the files on disk are not touched).  Every random value
of a batch comes from a *plan* (a dict of device tensors holding derived values, ``PLAN_FIELDS``): ``sample_with(plan)`` is the
deterministic path, ``draw_plan(n, seed)`` fills a plan on the device, ``sample(n, seed)`` does both.  Nothing on the sampling path
synchronises with the host (kernels: ``parc_amd/csrc/parc_motion_sampler.hpp``).
"""
from __future__ import annotations

import ctypes as C
import os
import types
import warnings
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from parc_amd import lib as L
from parc_amd.char_model import CharModel
from parc_amd.tool_handle import PlanCodec, ToolHandle, fill_struct

FRAME_COMPONENTS = ("ROOT_POS", "ROOT_ROT", "JOINT_POS", "JOINT_ROT", "CONTACTS", "FLOOR_HEIGHTS")   # MDMFrameType (JOINT_VEL: unused)
RELATIVE_Z, AUG_MODE = L.MSAMP_RELATIVE_Z, L.MSAMP_AUG_MODE
POOL_NONE, POOL_2D, POOL_1D_X, POOL_1D_Y = L.MSAMP_POOL_NONE, L.MSAMP_POOL_2D, L.MSAMP_POOL_1D_X, L.MSAMP_POOL_1D_Y
KERNELS = ("draw", "window", "heightfield")
MAX_FRAMES, MAX_GRID, MAX_TERRAIN_CELLS = L.MSAMP_MAX_FRAMES, L.MSAMP_MAX_GRID, L.MSAMP_MAX_TERRAIN_CELLS
MAX_BOXES, BOX_FLOATS = L.MSAMP_MAX_BOXES, L.MSAMP_BOX_FLOATS
# the plan: (name, torch dtype, per-sample shape; "mb" = max_num_boxes, "gx" / "gy" = the patch), in the order of ParcMotionSamplerPlan
PLAN_FIELDS = [(name, torch.int32 if t == "i" else torch.float32, shape) for name, t, shape in L.MSAMP_PLAN_FIELDS]


def parse_config(cfg: dict) -> types.SimpleNamespace:
    """The reference's keys -> the values the kernels take, computed as the reference computes them (``__init__`` :25-115)."""
    c = types.SimpleNamespace()
    comps = list(cfg["features"]["frame_components"])
    for k in comps:
        if k not in FRAME_COMPONENTS:
            raise ValueError(f"frame component {k!r} is not supported (supported: {FRAME_COMPONENTS})")
    rot_type = cfg["features"].get("rot_type", "DEFAULT")
    if rot_type not in ("DEFAULT", "QUAT"):
        raise ValueError(f"rot_type {rot_type!r}: only DEFAULT (quaternions) is supported")
    c.frame_components = comps
    c.sequence_fps = cfg["sequence_fps"]
    c.sequence_duration = float(cfg["sequence_duration"])
    c.timestep = 1.0 / c.sequence_fps
    c.times = torch.arange(start=0.0, end=c.sequence_duration, step=c.timestep, dtype=torch.float32).numpy().copy()
    c.T = int(c.times.shape[0])
    c.num_prev_states = int(cfg["num_prev_states"])
    if not 1 <= c.num_prev_states <= c.T:
        raise ValueError("num_prev_states must be in [1, T]")
    c.ref_frame = c.num_prev_states - 1
    c.autoregressive = bool(cfg["autoregressive"])
    c.relative_z_style = RELATIVE_Z[cfg["relative_z_style"]]
    c.use_hf_augmentation = bool(cfg["use_hf_augmentation"])
    c.aug_mode = AUG_MODE[cfg["hf_augmentation_mode"]] if c.use_hf_augmentation else AUG_MODE["NONE"]
    hm = cfg["heightmap"]
    g = hm["local_grid"]
    c.dx = float(hm["horizontal_scale"])
    c.num_x_neg, c.num_x_pos, c.num_y_neg, c.num_y_pos = int(g["num_x_neg"]), int(g["num_x_pos"]), int(g["num_y_neg"]), int(g["num_y_pos"])
    c.Gx, c.Gy = c.num_x_neg + 1 + c.num_x_pos, c.num_y_neg + 1 + c.num_y_pos
    # geom_util.get_xy_grid_points around a zero centre (:212-223)
    zero = torch.zeros(2, dtype=torch.float32)
    c.grid_x = torch.linspace(zero[0] - c.dx * c.num_x_neg, zero[0] + c.dx * c.num_x_pos, c.Gx).numpy().astype(np.float32)
    c.grid_y = torch.linspace(zero[1] - c.dx * c.num_y_neg, zero[1] + c.dx * c.num_y_pos, c.Gy).numpy().astype(np.float32)
    c.grid_min = (torch.tensor([-c.num_x_neg, -c.num_y_neg], dtype=torch.float32) * c.dx).numpy()   # _grid_min_point :76
    c.max_h = float(hm["max_h"])
    c.max_num_boxes = int(cfg.get("max_num_boxes", 0)) if c.use_hf_augmentation else 0
    c.box_min_len, c.box_max_len = float(cfg.get("box_min_len", 1)), float(cfg.get("box_max_len", 1))
    c.hf_maxpool_chance = float(cfg.get("hf_maxpool_chance", 0.0))
    c.hf_max_maxpool_size = int(cfg.get("hf_max_maxpool_size", 0))
    c.hf_change_height_chance = float(cfg.get("hf_change_height_chance", 0.0))
    c.future_pos_noise_scale = float(cfg["future_pos_noise_scale"])
    c.future_window_min, c.future_window_max = float(cfg["future_window_min"]), float(cfg["future_window_max"])
    if c.T > MAX_FRAMES or max(c.Gx, c.Gy) > MAX_GRID or c.max_num_boxes > MAX_BOXES:
        raise ValueError(f"limits: T <= {MAX_FRAMES}, patch sides <= {MAX_GRID}, max_num_boxes <= {MAX_BOXES}")
    return c


def pack_mask_inds(per_clip: Sequence[Sequence[np.ndarray]], dims: Sequence[Sequence[int]]):
    """CSR packing of ``hf_mask_inds``: per clip a list (one per frame) of int [K, 2] cells -> (``mask_off`` int64 [F + 1], ``cells``
    int32, cell = i * Y + j), frames in clip order."""
    counts, cells = [], []
    for inds, (X, Y) in zip(per_clip, dims):
        for a in inds:
            a = np.asarray(a).reshape(-1, 2).astype(np.int64)
            if a.size and (a.min() < 0 or a[:, 0].max() >= X or a[:, 1].max() >= Y):
                raise ValueError("hf_mask_inds outside the terrain")
            counts.append(a.shape[0])
            cells.append((a[:, 0] * Y + a[:, 1]).astype(np.int32))
    off = np.zeros(len(counts) + 1, np.int64)
    np.cumsum(counts, out=off[1:])
    return off, (np.ascontiguousarray(np.concatenate(cells)) if cells else np.zeros(0, np.int32))


def unpack_mask_inds(mask_off, cells, frame_off, dims) -> List[List[np.ndarray]]:
    """The inverse of :func:`pack_mask_inds`."""
    out = []
    for c, (X, Y) in enumerate(dims):
        out.append([np.stack([cells[mask_off[f]:mask_off[f + 1]] // Y, cells[mask_off[f]:mask_off[f + 1]] % Y], -1).astype(np.int64)
                    for f in range(int(frame_off[c]), int(frame_off[c + 1]))])
    return out


def check_clip_lengths(names: Sequence[str], num_frames: Sequence[int], T: int):
    """A clip needs ``num_frames - T > 0`` (``get_motion_sequences_for_id`` asserts; the start-time draw would go negative)."""
    short = [f"{n} ({f} frames)" for n, f in zip(names, num_frames) if f - T <= 0]
    if short:
        raise ValueError(f"clips too short for windows of {T} frames: " + ", ".join(short))


def plan_codec(cfg) -> PlanCodec:
    """The plan of a parsed config: ``noise`` is carried only when the augmentation mode is ``NOISE``."""
    return PlanCodec(L.MSAMP_PLAN_FIELDS, L.ParcMotionSamplerPlan, {"mb": cfg.max_num_boxes, "gx": cfg.Gx, "gy": cfg.Gy},
                     optional=() if cfg.aug_mode == AUG_MODE["NOISE"] else ("noise",))


def plan_shapes(n: int, cfg) -> Dict[str, tuple]:
    return {name: (n,) + shape for name, (_, shape) in plan_codec(cfg).fields.items()}


def check_plan(plan: Dict[str, torch.Tensor], cfg) -> int:
    """Lengths and dtypes of a plan's arrays (no device access); returns n."""
    return plan_codec(cfg).struct(plan)[1]


def assemble_features(motion: Dict[str, torch.Tensor], frame_components: Sequence[str]) -> torch.Tensor:
    """``MDM.assemble_mdm_features`` (mdm.py:344-394) with ``rot_type: DEFAULT``: the components, flattened per frame, concatenated in
    ``frame_components`` order -> [n, T, D]."""
    parts = []
    for k in frame_components:
        v = motion[k]
        parts.append(v.reshape(v.shape[0], v.shape[1], -1))
    return torch.cat(parts, dim=-1)


def feature_slices(frame_components: Sequence[str], num_bodies: int) -> Dict[str, slice]:
    width = {"ROOT_POS": 3, "ROOT_ROT": 4, "JOINT_POS": 3 * (num_bodies - 1), "JOINT_ROT": 4 * (num_bodies - 1), "CONTACTS": num_bodies,
             "FLOOR_HEIGHTS": 1}
    out, o = {}, 0
    for k in frame_components:
        out[k] = slice(o, o + width[k])
        o += width[k]
    return out


def write_feature_stats(path: str, mean, std):
    """``feature_stats.yaml`` in the layout ``MDM._compute_stats`` writes (mdm.py:506-511)."""
    import yaml
    with open(path, "w") as f:
        yaml.safe_dump({"mean": np.asarray(mean).tolist(), "std": np.asarray(std).tolist()}, f)


def export_batches(sampler, num_batches: int, batch_size: int, out_dir: str, seed: int = 0):
    """``batch_%06d.npz`` (the motion components, ``features``, ``hfs``, ``target_pos``, ``target_rot``) + ``feature_stats.yaml``."""
    os.makedirs(out_dir, exist_ok=True)
    files = []
    for b in range(num_batches):
        motion, hfs, tp, tr = sampler.sample(batch_size, seed + b)
        arrs = {k.lower(): v.cpu().numpy() for k, v in motion.items()}
        arrs.update(features=sampler.assemble_features(motion).cpu().numpy(), hfs=hfs.cpu().numpy(), target_pos=tp.cpu().numpy(),
                    target_rot=tr.cpu().numpy())
        files.append(os.path.join(out_dir, "batch_%06d.npz" % b))
        np.savez(files[-1], **arrs)
    mean, std = sampler.feature_stats()
    write_feature_stats(os.path.join(out_dir, "feature_stats.yaml"), mean.cpu().numpy(), std.cpu().numpy())
    return files


class MotionWindowSampler(ToolHandle):
    """See the module docstring.  ``extra_vals`` (per clip ``dict(hf_mask_inds=[...], hf_maxmin=[X, Y, 2])`` or ``None``) overrides
    what the files hold; ``exclude`` drops clips by name (e.g. ones too short for a window)."""
    PREFIX, KERNELS = "parc_msamp", KERNELS

    def __init__(self, cfg: dict, motion_file: str, char_file: str, device="cuda:0", extra_vals: Optional[Sequence[Optional[dict]]] = None,
                 exclude: Sequence[str] = ()):
        from parc_amd import motion_lib, ms_file
        super().__init__(device)
        self.cfg = parse_config(cfg)
        self._codec = plan_codec(self.cfg)
        self.char_file = char_file
        self.char_model = CharModel(char_file)
        self.B = self.char_model.get_num_bodies()
        clips = [c for c in motion_lib.load_motion_file(motion_file, verbose=False) if c.name not in set(exclude)]
        if extra_vals is not None and len(extra_vals) != len(clips):
            raise ValueError("extra_vals: one entry per clip")
        self.clip_names = [c.name for c in clips]
        check_clip_lengths(self.clip_names, [c.num_frames for c in clips], self.cfg.T)
        for c in clips:
            if c.terrain is None:
                raise ValueError(f"{c.name}: the sampler needs terrain_data")
            if c.terrain.hf.size > MAX_TERRAIN_CELLS:
                raise ValueError(f"{c.name}: the terrain has {c.terrain.hf.size} cells, above the limit of {MAX_TERRAIN_CELLS}")
            if c.fps != self.cfg.sequence_fps:   # the window's mask frames are round(t0 * sequence_fps) + k, as in the reference (:214-216)
                warnings.warn(f"{c.name}: clip fps {c.fps} differs from sequence_fps {self.cfg.sequence_fps}; the window's hf_mask_inds "
                              "are taken at the reference's frame indices, which are then not the window's frames")
        extra = list(extra_vals) if extra_vals is not None else [None] * len(clips)
        for i, c in enumerate(clips):
            if extra[i] is None:
                misc = ms_file.load_ms_file(c.file, load_misc=True).misc_data
                inds = None if misc is None else misc.get("hf_mask_inds")
                if inds is not None and len(inds) == c.num_frames:
                    extra[i] = dict(hf_mask_inds=[np.asarray(a) for a in inds], hf_maxmin=np.asarray(c.terrain.hf_maxmin, np.float32))
        missing = [i for i in range(len(clips)) if extra[i] is None]
        if missing:   # one batched analysis for every file without hf_mask_inds
            from parc_amd.motion_opt import clip_from_ms
            from parc_amd.motion_terrain import MotionTerrainAnalyzer
            res = MotionTerrainAnalyzer(char_file, device).analyze([clip_from_ms(clips[i].file) for i in missing])
            for i, r in zip(missing, res):
                extra[i] = dict(hf_mask_inds=r["hf_mask_inds"], hf_maxmin=r["hf_maxmin"])
        self.clips, self.extra_vals = clips, extra
        self._create()
        self._upload()

    # ------------------------------------------------------------------ handle
    def _create(self):
        c = self.cfg
        p = L.ParcMotionSamplerParams()
        p.device = self.device_index
        p.model = L.make_char_model(self.char_model)
        p.num_frames, p.times_host = c.T, L.np_f32p(c.times)
        p.timestep, p.sequence_duration = float(np.float32(c.timestep)), c.sequence_duration
        p.ref_frame, p.autoregressive, p.relative_z_style, p.aug_mode = c.ref_frame, int(c.autoregressive), c.relative_z_style, c.aug_mode
        p.grid_dim_x, p.grid_dim_y, p.num_x_neg, p.num_y_neg = c.Gx, c.Gy, c.num_x_neg, c.num_y_neg
        p.grid_x_host, p.grid_y_host = L.np_f32p(c.grid_x), L.np_f32p(c.grid_y)
        p.grid_min_x, p.grid_min_y, p.dx, p.max_h = float(c.grid_min[0]), float(c.grid_min[1]), c.dx, c.max_h
        p.max_num_boxes, p.box_min_len, p.box_max_len = c.max_num_boxes, c.box_min_len, c.box_max_len
        p.hf_maxpool_chance, p.hf_max_maxpool_size, p.hf_change_height_chance = c.hf_maxpool_chance, c.hf_max_maxpool_size, c.hf_change_height_chance
        p.future_pos_noise_scale, p.future_window_min, p.future_window_max = c.future_pos_noise_scale, c.future_window_min, c.future_window_max
        self._create_handle(p)

    def _upload(self):
        from parc_amd.motion_opt import OptClip, clip_struct, pack_clips
        oc = [OptClip(c.root_pos, c.root_rot, c.joint_rot,
                      c.contacts if c.contacts is not None else np.zeros((c.num_frames, self.B), np.float32),
                      np.asarray(c.terrain.hf, np.float32), np.asarray(c.terrain.min_point, np.float32), float(c.terrain.dx), c.fps, c.name)
              for c in self.clips]
        pk = pack_clips(oc, self.B, self.char_model.get_dof_size())
        st = clip_struct(pk, len(oc))
        dims = [c.hf.shape for c in oc]
        mask_off, cells = pack_mask_inds([e["hf_mask_inds"] for e in self.extra_vals], dims)
        maxmin = np.ascontiguousarray(np.concatenate([np.asarray(e["hf_maxmin"], np.float32).reshape(-1, 2) for e in self.extra_vals]))
        if maxmin.shape[0] != pk["hf_off"][-1] or mask_off.shape[0] != pk["frame_off"][-1] + 1:
            raise ValueError("hf_maxmin / hf_mask_inds do not match the clips")
        fps = np.array([c.fps for c in self.clips], np.int32)
        loop = np.array([c.loop_mode for c in self.clips], np.int32)
        w = np.array([c.weight for c in self.clips], np.float64)
        info = L.ParcMotionSamplerClipInfo()
        info.hf_maxmin_host, info.mask_off_host = L.np_f32p(maxmin), mask_off.ctypes.data_as(L.i64p)
        info.mask_cells_host = L.np_i32p(cells) if cells.size else None
        info.fps_host, info.loop_modes_host, info.weights_host = L.np_i32p(fps), L.np_i32p(loop), w.ctypes.data_as(L.f64p)
        self._call("set_clips", C.byref(st), C.byref(info))
        self.packed = pk
        self.num_frames = np.diff(pk["frame_off"]).astype(np.int64)
        self.lengths = np.array([np.float32(1.0 / c.fps * (c.num_frames - 1)) for c in self.clips], np.float32)
        self.loop_modes = loop
        self.weights = w / w.sum()

    # ------------------------------------------------------------------ plans and outputs
    def empty_plan(self, n: int, zero: bool = True) -> Dict[str, torch.Tensor]:
        """The plan's device arrays; ``zero=False`` leaves them uninitialised (``draw_plan`` writes every entry)."""
        return self._codec.empty(n, self.device, zero)

    def plan_from_numpy(self, arrays: Dict[str, np.ndarray]) -> Dict[str, torch.Tensor]:
        """A plan from host arrays (missing augmentation fields are zeros = no augmentation step)."""
        return self._codec.from_numpy(arrays, self.device, required=("motion_id",))

    def _plan_struct(self, plan):
        return self._codec.struct(plan, self.device)

    def _outputs(self, n: int, hf: bool, bounds: bool = False):
        c, J = self.cfg, self.B - 1
        z = lambda *s: torch.empty(s, dtype=torch.float32, device=self.device)  # noqa: E731
        o = dict(root_pos=z(n, c.T, 3), root_rot=z(n, c.T, 4), joint_pos=z(n, c.T, J, 3), joint_rot=z(n, c.T, J, 4), contacts=z(n, c.T, self.B))
        if hf:
            o.update(hfs=z(n, c.Gx, c.Gy), target_pos=z(n, 3), target_rot=z(n, 4))
            if "FLOOR_HEIGHTS" in c.frame_components:
                o["floor_heights"] = z(n, c.T)
            if bounds:
                o["hf_bounds"] = z(n, c.Gx, c.Gy, 2)
        return o, fill_struct(L.ParcMotionSamplerOutputs, o)

    def _motion_dict(self, o):
        names = dict(ROOT_POS="root_pos", ROOT_ROT="root_rot", JOINT_POS="joint_pos", JOINT_ROT="joint_rot", CONTACTS="contacts",
                     FLOOR_HEIGHTS="floor_heights")
        return {k: (o[names[k]].unsqueeze(-1) if k == "FLOOR_HEIGHTS" else o[names[k]]) for k in self.cfg.frame_components if names[k] in o}

    # ------------------------------------------------------------------ sampling
    def sample_with(self, plan: Dict[str, torch.Tensor], return_bounds: bool = False, validate: bool = False):
        """(motion dict keyed by component name, hfs [n, Gx, Gy], target_pos [n, 3], target_rot [n, 4]) of ``plan``; with
        ``return_bounds`` also the per-window bounds [n, Gx, Gy, 2].  ``validate`` synchronises and raises on a bad plan entry."""
        st, n = self._plan_struct(plan)
        o, ost = self._outputs(n, True, return_bounds)
        self._call("sample_with", C.byref(st), C.byref(ost), self._stream())
        if validate:
            self.check_status()
        ret = (self._motion_dict(o), o["hfs"], o["target_pos"], o["target_rot"])
        return ret + (o["hf_bounds"],) if return_bounds else ret

    def draw_plan(self, n: int, seed: int) -> Dict[str, torch.Tensor]:
        plan = self.empty_plan(n, zero=False)
        st, _ = self._plan_struct(plan)
        self._call("draw_plan", C.c_uint64(int(seed)), C.byref(st), self._stream())
        return plan

    def sample(self, n: int, seed: int):
        plan = self.empty_plan(n, zero=False)
        st, _ = self._plan_struct(plan)
        o, ost = self._outputs(n, True)
        self._call("sample", C.c_uint64(int(seed)), C.byref(st), C.byref(ost), self._stream())
        return self._motion_dict(o), o["hfs"], o["target_pos"], o["target_rot"]

    def check_status(self):
        """Synchronises; raises if a kernel met a bad plan entry (motion id, box count, pool) since the last call."""
        v = C.c_int32()
        self._call("plan_status", self._stream(), C.byref(v))
        if v.value:
            raise L.ParcError("bad plan: " + "; ".join(m for b, m in L.MSAMP_STATUS.items() if v.value & b))

    def motion_sequences_for_id(self, i: int) -> Dict[str, torch.Tensor]:
        """``get_motion_sequences_for_id``: the windows starting at frames 0 .. num_frames - T - 1 of clip ``i`` (motion only)."""
        n = int(self.num_frames[i]) - self.cfg.T
        o, ost = self._outputs(n, False)
        self._call("enumerate", int(i), C.byref(ost), self._stream())
        return self._motion_dict(o)

    def assemble_features(self, motion: Dict[str, torch.Tensor]) -> torch.Tensor:
        return assemble_features(motion, [k for k in self.cfg.frame_components if k in motion])

    def feature_stats(self):
        """Mean and std [T, D] over every window of every clip (``MDM._compute_stats``, mdm.py:467-495): a two-pass reduction in fp64
        on the device (sum, then the sum of squared deviations, / (N - 1)), contact columns forced to 0 / 1, std clamped at 1e-5."""
        comps = [k for k in self.cfg.frame_components if k != "FLOOR_HEIGHTS"]
        feats = [assemble_features(self.motion_sequences_for_id(i), comps).double() for i in range(len(self.clips))]
        num = sum(f.shape[0] for f in feats)
        mean = sum(f.sum(dim=0) for f in feats) / num
        var = sum(torch.square(f - mean.unsqueeze(0)).sum(dim=0) for f in feats) / (num - 1)
        mean, std = mean.float(), torch.sqrt(var).float()
        sl = feature_slices(comps, self.B).get("CONTACTS")
        if sl is not None:
            mean[:, sl] = 0.0
            std[:, sl] = 1.0
        return mean, torch.clamp(std, min=1e-5)
