"""Path-following motion generation on the GPU: the reference's world-frame wrapper of the generator (``gen_util.gen_mdm_motion``,
``RELATIVE_TO_ROOT``) and its autoregressive rollout along a planned path (``motion_synthesis/procgen/mdm_path.py``), for N rows at
once.  Rows are P paths times K candidates; path p lies on terrain p.

``PathMotionGenerator(generator, path_settings, gen_settings)`` drives an :class:`~parc_amd.motion_generator.MDMGenerator`.
``set_scene`` uploads terrains and paths, ``rollout`` walks every row from its path's first node to its last, ``select`` scores the rows
with :class:`~parc_amd.motion_terrain.MotionTerrainAnalyzer` and sorts them per path, ``to_clips`` returns them as ``OptClip``.  A window
is one conditions kernel, the sampler's launches and one append kernel; the host reads one int per window
(``parc_amd/csrc/parc_mdm_path.hpp``).  x_T of window ``w`` of a row is ``generator.draw_noise(1, seed,
row_id * KEY_WINDOWS + w)``: a row's motion does not depend on its batch.  No CPU or eager fallback.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from parc_amd import lib as L
from parc_amd.motion_generator import MDMGenerator
from parc_amd.tool_handle import PlanCodec, ToolHandle
from parc_amd.util import path_loader

KERNELS = ("cond", "append")
KEY_WINDOWS = 4096
NOT_FINISHED_PENALTY = 100.0
FRAME_KEYS = ("root_pos", "root_rot", "joint_rot", "contacts")
# the start plan of a rollout without previous frames, per path (both optional: a missing one is drawn on the device / heading_mode)
PLAN_FIELDS = [("rel_height", "f", ()), ("heading", "f", ())]


class _StartPlan(C.Structure):
    _fields_ = [("n", C.c_int32), ("rel_height", C.c_void_p), ("heading", C.c_void_p)]


PLAN = PlanCodec(PLAN_FIELDS, _StartPlan, optional=("heading",))


def _settings_from_config(cls, block, what):
    names = {f.name: f.type for f in dataclasses.fields(cls)}
    unknown = sorted(set(block) - set(names))
    if unknown:
        raise ValueError(f"unknown {what} setting(s): {unknown}")
    casts = {"int": int, "float": float, "bool": bool}
    return cls(**{k: casts[names[k]](v) for k, v in block.items()})


@dataclasses.dataclass
class MDMPathSettings:
    """The reference's ``MDMPathSettings`` (mdm_path.py:19-29), its names and class defaults."""
    next_node_lookahead: int = 7
    rewind_num_frames: int = 5
    end_of_path_buffer: int = 2
    max_motion_length: float = 10.0
    path_batch_size: int = 16
    mdm_batch_size: int = 32
    top_k: int = 4
    w_target: float = 2.0
    w_contact: float = 0.1
    w_pen: float = 0.1

    @classmethod
    def from_config(cls, block) -> "MDMPathSettings":
        """The ``mdm_path:`` block of a config; a missing key keeps the class default, an unknown one is an error."""
        return _settings_from_config(cls, block, "mdm_path")

    def to_config(self) -> dict:
        return dataclasses.asdict(self)


@dataclasses.dataclass
class MDMGenSettings:
    """The reference's ``MDMGenSettings`` (gen_util.py:18-25)."""
    use_prev_state: bool = True
    use_cfg: bool = True
    cfg_scale: float = 0.65
    prev_state_ind_key: bool = True
    target_condition_key: bool = True
    use_ddim: bool = True
    ddim_stride: int = 10

    @classmethod
    def from_config(cls, block) -> "MDMGenSettings":
        return _settings_from_config(cls, block, "mdm_gen")

    def to_config(self) -> dict:
        return dataclasses.asdict(self)


def load_config(path):
    """``(MDMPathSettings, MDMGenSettings, the remaining keys)`` of a ``mdm_path`` config file."""
    cfg = dict(path_loader.load_config(path))
    return MDMPathSettings.from_config(cfg.pop("mdm_path", {})), MDMGenSettings.from_config(cfg.pop("mdm_gen", {})), cfg


@dataclasses.dataclass
class RolloutResult:
    """The frames of N rows on the device, ``[N, num_frames, ...]``; row r's motion is ``frames[r, :final_frame[r]]`` (an unfinished
    row, ``final_frame`` -1, loses its last frame: the reference's slice)."""
    root_pos: torch.Tensor
    root_rot: torch.Tensor
    joint_rot: torch.Tensor
    contacts: torch.Tensor
    final_frame: torch.Tensor     # [N] int32
    done: torch.Tensor            # [N] bool, of the last window
    num_frames: int
    windows: int
    frames_per_window: List[int]

    def frames(self) -> Dict[str, torch.Tensor]:
        return {k: getattr(self, k) for k in FRAME_KEYS}


class PathMotionGenerator(ToolHandle):
    """See the module docstring."""
    PREFIX, KERNELS = "parc_mpath", KERNELS

    def __init__(self, generator: MDMGenerator, path_settings: Optional[MDMPathSettings] = None, gen_settings: Optional[MDMGenSettings] = None):
        if not isinstance(generator, MDMGenerator):
            raise TypeError("generator must be an MDMGenerator")
        super().__init__(generator.device)
        self.generator = generator           # kept alive: the handle drives it
        self.path_settings = ps = path_settings or MDMPathSettings()
        self.gen_settings = gs = gen_settings or MDMGenSettings()
        cfg = generator.cfg
        style = str(cfg.get("relative_z_style", "RELATIVE_TO_ROOT"))
        if style != "RELATIVE_TO_ROOT":
            raise ValueError(f"relative_z_style {style!r}: path-following generation builds RELATIVE_TO_ROOT (RELATIVE_TO_ROOT_FLOOR indexes "
                             "the heightfield with the batch axis in the reference, DESIGN.md section 8k)")
        if not gs.use_ddim:
            raise ValueError("use_ddim must be true: the rollout samples with DDIM")
        cm = generator.char_model
        self.B, self.J = cm.get_num_bodies(), cm.get_num_bodies() - 1
        self.FD = 7 + 4 * self.J + self.B
        self.T, self.nprev, self.D = generator.T, generator.nprev, generator.D
        hm = cfg["heightmap"]
        g = hm["local_grid"]
        p = L.ParcMdmPathParams()
        p.mdm = generator._h
        p.grid_dx = p.grid_dy = float(hm["horizontal_scale"])
        p.num_x_neg, p.num_x_pos, p.num_y_neg, p.num_y_pos = int(g["num_x_neg"]), int(g["num_x_pos"]), int(g["num_y_neg"]), int(g["num_y_pos"])
        p.max_h, p.sequence_fps = float(hm["max_h"]), float(cfg.get("sequence_fps", 30))
        p.left_foot, p.right_foot = cm.get_body_id("left_foot"), cm.get_body_id("right_foot")
        p.next_node_lookahead, p.rewind_num_frames, p.max_motion_length = int(ps.next_node_lookahead), int(ps.rewind_num_frames), float(ps.max_motion_length)
        p.use_prev_state, p.use_cfg, p.cfg_scale = int(gs.use_prev_state), int(gs.use_cfg), float(gs.cfg_scale)
        p.prev_state_ind_key, p.target_condition_key, p.use_ddim, p.ddim_stride = int(gs.prev_state_ind_key), int(gs.target_condition_key), 1, int(gs.ddim_stride)
        self._create_handle(p)
        self.fps = float(p.sequence_fps)
        self.start_frame = self.T - 1 - int(ps.rewind_num_frames)
        self.steps = len(range(0, generator.timesteps, int(gs.ddim_stride)))
        d = self.describe()
        self.max_frames, self.max_windows = d["max_frames"], d["max_windows"]
        self.N = 0
        self._scene = None

    # ------------------------------------------------------------------ the scene
    def set_scene(self, hfs, min_points, dx, paths: Sequence, candidates_per_path: int = 1, dy: Optional[float] = None):
        """Terrains ``hfs`` [P, X, Y] with ``min_points`` [P, 2] and cell size ``dx`` (``dy``), one path [n_p, 3] per terrain; the rows are
        ``candidates_per_path`` consecutive rows per path."""
        hfs = np.ascontiguousarray(hfs, np.float32)
        if hfs.ndim != 3:
            raise ValueError(f"hfs must be [P, X, Y], not {list(hfs.shape)}")
        P = hfs.shape[0]
        mp = np.ascontiguousarray(min_points, np.float32)
        if mp.shape != (P, 2):
            raise ValueError(f"min_points must be [{P}, 2], not {list(mp.shape)}")
        if len(paths) != P:
            raise ValueError(f"paths: {len(paths)} paths for {P} terrains")
        K = int(candidates_per_path)
        if K < 1:
            raise ValueError("candidates_per_path must be >= 1")
        pts = [np.asarray(q, np.float32).reshape(-1, 3) for q in paths]
        counts = np.asarray([q.shape[0] for q in pts], np.int32)
        maxn = max(2, int(counts.max()))
        packed = np.zeros((P, maxn, 3), np.float32)
        for i, q in enumerate(pts):
            packed[i, :q.shape[0]] = q
        row_path = np.repeat(np.arange(P, dtype=np.int32), K)
        self._call("set_scene", L.np_f32p(hfs), P, hfs.shape[1], hfs.shape[2], L.np_f32p(mp), float(dx), float(dx if dy is None else dy), L.np_f32p(packed),
                   L.np_i32p(counts), maxn, L.np_i32p(row_path), int(row_path.size))
        self.N, self.P, self.K = int(row_path.size), P, K
        self._scene = dict(hfs=hfs, min_points=mp, dx=float(dx), paths=pts, row_path=row_path)

    def _need_scene(self):
        if self._scene is None:
            raise ValueError("set_scene first")

    # ------------------------------------------------------------------ frames
    def pack_frames(self, frames: dict) -> torch.Tensor:
        """A frame dict (``root_pos`` [N, n, 3], ``root_rot`` [N, n, 4], ``joint_rot`` [N, n, J, 4], ``contacts`` [N, n, B]) -> [N, n, FD]."""
        missing = [k for k in FRAME_KEYS if k not in frames]
        if missing:
            raise ValueError(f"frames: {missing} missing")
        rp = torch.as_tensor(frames["root_pos"], device=self.device).to(torch.float32)
        n0, n1 = rp.shape[0], rp.shape[1]
        parts = [rp, torch.as_tensor(frames["root_rot"], device=self.device).to(torch.float32),
                 torch.as_tensor(frames["joint_rot"], device=self.device).to(torch.float32).reshape(n0, n1, -1),
                 torch.as_tensor(frames["contacts"], device=self.device).to(torch.float32)]
        out = torch.cat(parts, dim=-1).contiguous()
        if out.shape[-1] != self.FD:
            raise ValueError(f"frames: {out.shape[-1]} values per frame, the character has {self.FD}")
        return out

    def unpack_frames(self, buf: torch.Tensor) -> Dict[str, torch.Tensor]:
        J = self.J
        return {"root_pos": buf[..., 0:3], "root_rot": buf[..., 3:7], "joint_rot": buf[..., 7:7 + 4 * J].reshape(buf.shape[:-1] + (J, 4)),
                "contacts": buf[..., 7 + 4 * J:]}

    def _prev(self, prev_frames):
        prev = self.pack_frames(prev_frames)
        if tuple(prev.shape) != (self.N, self.nprev, self.FD):
            raise ValueError(f"prev_frames must hold [{self.N}, {self.nprev}] frames, not {list(prev.shape[:2])}")
        return prev

    # ------------------------------------------------------------------ the kernels on their own
    def conds(self, prev_frames: dict, first: bool = False, blank: bool = False) -> dict:
        """k_mpath_cond: the condition arrays as the sampler takes them (``OBS_KEY`` divided by max_h, ``PREV_STATE_KEY`` standardised),
        plus ``done``, ``closest_node``, ``target_node`` and the canonical record ``canon`` [N, 8]."""
        self._need_scene()
        prev = self._prev(prev_frames)
        n, dev = self.N, self.device
        f = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)   # noqa: E731
        i = lambda: torch.empty((n,), dtype=torch.int32, device=dev)     # noqa: E731
        t = dict(hf=f(n, L.MDM_GRID, L.MDM_GRID), target=f(n, 2), prev_state=f(n, self.nprev, self.D), obs_flag=i(), target_flag=i(), prev_state_flag=i(),
                 noise_ind=i(), done=i(), closest_node=i(), target_node=i(), canon=f(n, 8))
        st = L.ParcMdmPathCondOut(**{k: v.data_ptr() for k, v in t.items()})
        self._call("conds", prev.data_ptr(), int(first), int(blank), C.byref(st), self._stream())
        return {"OBS_KEY": t["hf"], "TARGET_KEY": t["target"], "PREV_STATE_KEY": t["prev_state"], "OBS_FLAG_KEY": t["obs_flag"].bool(),
                "TARGET_FLAG_KEY": t["target_flag"].bool(), "PREV_STATE_FLAG_KEY": t["prev_state_flag"].bool(),
                "PREV_STATE_NOISE_IND_KEY": t["noise_ind"].bool(), "done": t["done"].bool(), "closest_node": t["closest_node"],
                "target_node": t["target_node"], "canon": t["canon"]}

    def append(self, x, prev_state, noise_ind, canon, frames: torch.Tensor, offset: int, lo: int, hi: int, guided: bool, prev_next: Optional[torch.Tensor] = None,
               done=None, final_frame: Optional[torch.Tensor] = None, total: int = 0):
        """k_mpath_append: frames [lo, hi) of the sample ``x`` [n, T, D] (standardised) into ``frames`` [n, max_frames, FD] at ``offset``,
        frames [start_frame - nprev, start_frame) into ``prev_next`` [n, nprev, FD]."""
        a = L.ParcMdmPathAppendArgs()
        x = torch.as_tensor(x, device=self.device).to(torch.float32).contiguous()
        n = x.shape[0]
        if tuple(x.shape) != (n, self.T, self.D):
            raise ValueError(f"x must be [n, {self.T}, {self.D}]")
        ps = torch.as_tensor(prev_state, device=self.device).to(torch.float32).contiguous()
        ind = torch.as_tensor(noise_ind, device=self.device).to(torch.int32).contiguous()
        cn = torch.as_tensor(canon, device=self.device).to(torch.float32).contiguous()
        if tuple(ps.shape) != (n, self.nprev, self.D) or tuple(ind.shape) != (n,) or tuple(cn.shape) != (n, 8):
            raise ValueError(f"prev_state must be [{n}, {self.nprev}, {self.D}], noise_ind [{n}], canon [{n}, 8]")
        if not (frames.dtype == torch.float32 and frames.is_contiguous() and frames.device == self.device and frames.dim() == 3
                and frames.shape[0] >= n and frames.shape[2] == self.FD):
            raise ValueError(f"frames must be a contiguous float32 tensor [n, max_frames, {self.FD}] on {self.device}")
        a.n, a.x, a.prev_state, a.noise_ind, a.canon = n, x.data_ptr(), ps.data_ptr(), ind.data_ptr(), cn.data_ptr()
        a.guided, a.lo, a.hi, a.offset, a.frames, a.max_frames = int(guided), int(lo), int(hi), int(offset), frames.data_ptr(), int(frames.shape[1])
        if prev_next is not None:
            if not (prev_next.dtype == torch.float32 and prev_next.is_contiguous() and tuple(prev_next.shape) == (n, self.nprev, self.FD)):
                raise ValueError(f"prev_next must be a contiguous float32 tensor [{n}, {self.nprev}, {self.FD}]")
            a.prev_next = prev_next.data_ptr()
        keep = None
        if final_frame is not None:
            keep = torch.as_tensor(done, device=self.device).to(torch.int32).contiguous()
            a.done, a.final_frame, a.total = keep.data_ptr(), final_frame.data_ptr(), int(total)
        self._call("append", C.byref(a), self._stream())
        del keep

    # ------------------------------------------------------------------ the rollout
    def rollout(self, prev_frames: Optional[dict] = None, plan: Optional[dict] = None, seed: Optional[int] = None, row_ids=None, noise=None,
                heading_mode: str = "auto", path_ids=None) -> RolloutResult:
        """``generate_frames_until_end_of_path`` for every row.  ``prev_frames``: the frames to start from, else blank frames placed at
        node 0 (``plan``: ``rel_height`` [P] and optionally ``heading`` [P]; what is missing is drawn from ``seed``, or the heading is
        ``heading_mode`` ``auto`` / ``random``).  ``noise`` [W, N, T, D] injects x_T of every window; otherwise it is drawn from
        ``(seed, row_ids)``; a drawn start is keyed by ``(seed, path_ids)`` [P] (default: the path's place in the scene)."""
        self._need_scene()
        if heading_mode not in ("auto", "random"):
            raise ValueError(f"heading_mode {heading_mode!r}: auto or random")
        n, dev = self.N, self.device
        a = L.ParcMdmPathRolloutArgs()
        keep = []
        if prev_frames is not None:
            prev = self._prev(prev_frames)
            keep.append(prev)
            a.prev_frames = prev.data_ptr()
        have = set()
        if plan is not None:
            plan = {k: torch.as_tensor(v).detach().to("cpu", torch.float32).contiguous() for k, v in plan.items()}
            unknown = sorted(set(plan) - set(PLAN.fields))
            if unknown:
                raise ValueError(f"plan: unknown field(s) {unknown}")
            _, pn = PLAN.struct(plan)
            if pn != self.P:
                raise ValueError(f"plan: rel_height must have shape ({self.P},), got {tuple(plan['rel_height'].shape)}")
            for k in plan:
                v = plan[k].numpy()
                keep.append(v)
                setattr(a, k + "_host", L.np_f32p(v))
            have = set(plan)
        need_seed = noise is None or (prev_frames is None and ("rel_height" not in have or (heading_mode == "random" and "heading" not in have)))
        if need_seed and seed is None:
            raise ValueError("give a `seed`: x_T, the relative root height or the random heading is drawn on the device")
        a.seed = int(seed or 0)
        a.heading_mode = L.MPATH_HEADING_RANDOM if heading_mode == "random" else L.MPATH_HEADING_AUTO
        if noise is not None:
            nz = torch.as_tensor(noise, device=dev).to(torch.float32).contiguous()
            if nz.dim() != 4 or tuple(nz.shape[1:]) != (n, self.T, self.D):
                raise ValueError(f"noise must be [windows, {n}, {self.T}, {self.D}]")
            keep.append(nz)
            a.noise, a.noise_windows = nz.data_ptr(), int(nz.shape[0])
        if row_ids is not None:
            ids = np.ascontiguousarray(row_ids, np.int64)
            if ids.shape != (n,):
                raise ValueError(f"row_ids must have shape ({n},)")
            keep.append(ids)
            a.row_ids_host = ids.ctypes.data_as(L.i64p)
        if path_ids is not None:                                  # the key of a start drawn on the device: the path, not its place in the scene
            pids = np.ascontiguousarray(path_ids, np.int64)
            if pids.shape != (self.P,):
                raise ValueError(f"path_ids must have shape ({self.P},)")
            keep.append(pids)
            a.path_ids_host = pids.ctypes.data_as(L.i64p)
        buf = torch.zeros((n, self.max_frames, self.FD), dtype=torch.float32, device=dev)
        final = torch.empty((n,), dtype=torch.int32, device=dev)
        done = torch.empty((n,), dtype=torch.int32, device=dev)
        a.frames, a.final_frame, a.done = buf.data_ptr(), final.data_ptr(), done.data_ptr()
        self._call("rollout", C.byref(a), self._stream())
        del keep
        d = self.describe()
        W, F = d["windows"], d["frames"]
        nprev, start = self.nprev, self.start_frame
        per = [start] + [start - nprev] * (W - 2) + ([self.T - nprev] if W > 1 else [])
        fr = self.unpack_frames(buf[:, :F])
        return RolloutResult(fr["root_pos"], fr["root_rot"], fr["joint_rot"], fr["contacts"], final, done.bool(), F, W, per)

    def window_key(self, row_id: int, window: int) -> int:
        """The ``first_index`` at which ``generator.draw_noise(1, seed, first_index)`` is x_T of ``window`` of the row ``row_id``."""
        return int(row_id) * KEY_WINDOWS + int(window)

    def describe(self) -> Dict[str, int]:
        out = np.zeros(6, np.int64)
        self._call("describe", out.ctypes.data_as(L.i64p))
        return dict(zip(("max_frames", "max_windows", "frame_floats", "windows", "launches", "frames"), (int(v) for v in out)))

    # ------------------------------------------------------------------ selection
    def row_lengths(self, result: RolloutResult) -> np.ndarray:
        """Frames of every row's motion: ``frames[0:final_frame]`` as Python slices it (-1 drops the last frame)."""
        ff = result.final_frame.cpu().numpy().astype(np.int64)
        return np.where(ff < 0, result.num_frames + ff, np.minimum(ff, result.num_frames))

    def to_clips(self, result: RolloutResult, rows: Optional[Sequence[int]] = None, names: Optional[Sequence[str]] = None, terrains: Optional[Sequence] = None):
        """The rows as ``motion_opt.OptClip`` (what ``MotionOptimizer``, ``MotionTerrainAnalyzer`` and the ms-file writers of the scripts
        take), each on its whole terrain, or on ``terrains[i]`` = ``(hf, min_point)`` where given (the slices of
        ``motion_select.PathSelector.select``)."""
        from parc_amd.motion_opt import OptClip
        self._need_scene()
        rows = list(range(self.N)) if rows is None else [int(r) for r in rows]
        if terrains is not None and len(terrains) != len(rows):
            raise ValueError(f"terrains: {len(terrains)} terrains for {len(rows)} rows")
        lens = self.row_lengths(result)
        idx = torch.as_tensor(rows, dtype=torch.long, device=result.root_pos.device)
        host = {k: v.detach()[idx].cpu().numpy() for k, v in result.frames().items()}   # the named rows only
        sc = self._scene
        clips = []
        for i, r in enumerate(rows):
            p, n = int(sc["row_path"][r]), int(lens[r])
            hf, mp = (sc["hfs"][p], sc["min_points"][p]) if terrains is None else terrains[i]
            clips.append(OptClip(host["root_pos"][i, :n].copy(), host["root_rot"][i, :n].copy(), host["joint_rot"][i, :n].copy(), host["contacts"][i, :n].copy(),
                                 np.array(hf, np.float32), np.array(mp, np.float32), sc["dx"], int(round(self.fps)), names[i] if names else f"row_{r}"))
        return clips

    def select(self, result: RolloutResult, top_k: Optional[int] = None, noise=None, seed: Optional[int] = None, analyzer=None) -> List[dict]:
        """mdm_path.py:386-433 with ``slice_terrain=False``: per path the rows sorted by ``w_contact * contact + w_pen * pen`` (+100
        for a row that never finished, + ``noise`` [N] or standard-normal numbers from ``seed``), the first ``top_k`` kept: ``rows``,
        ``total_loss`` (as sorted, noise included), ``contact_loss``, ``pen_loss``."""
        from parc_amd.motion_generator import _char_path
        from parc_amd.motion_terrain import MotionTerrainAnalyzer
        self._need_scene()
        ps = self.path_settings
        k = int(ps.top_k if top_k is None else top_k)
        if k < 1:
            raise ValueError("top_k must be >= 1")
        if analyzer is None:
            if getattr(self, "_analyzer", None) is None:
                self._analyzer = MotionTerrainAnalyzer(_char_path(self.generator.cfg), self.device)
            analyzer = self._analyzer
        r = analyzer.run(self.to_clips(result))
        out = r["clip_out"]
        pen = np.float32(ps.w_pen) * out[:, 0].astype(np.float32)
        contact = np.float32(ps.w_contact) * out[:, 1].astype(np.float32)
        total = (contact + pen).astype(np.float32)
        total = np.where(result.final_frame.cpu().numpy() < 0, total + np.float32(NOT_FINISHED_PENALTY), total).astype(np.float32)
        if noise is not None:
            nz = np.asarray(torch.as_tensor(noise).detach().cpu().numpy(), np.float32)
            if nz.shape != (self.N,):
                raise ValueError(f"noise must have shape ({self.N},)")
            total = total + nz
        elif seed is not None:
            total = total + torch.randn((self.N,), generator=torch.Generator().manual_seed(int(seed))).numpy()
        sel = []
        for p in range(self.P):
            rows = np.nonzero(self._scene["row_path"] == p)[0]
            order = rows[np.argsort(total[rows], kind="stable")][:k]
            sel.append(dict(path=p, rows=order, total_loss=total[order], contact_loss=contact[order], pen_loss=pen[order]))
        return sel
