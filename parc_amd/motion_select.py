"""Rollout selection on the GPU: the end of the reference's ``generate_frames_until_end_of_path`` (mdm_path.py:386-433, both values of
``slice_terrain``) and the acceptance test of ``parc_2_kin_gen.py:389-404``, on the device buffers a
:class:`~parc_amd.motion_path_gen.PathMotionGenerator` rollout left.

``PathSelector(path_generator).select(result)`` scores every row on its own slice of its terrain (``slice_terrain_around_motion``,
padding 1.2, ``localize=False``; the slice is two index tables into the terrain, never a copy), weights, penalises and ranks the rows of
every path and applies the thresholds, in four launches without a host sync (``parc_amd/csrc/parc_mpath_select.hpp``, DESIGN.md section
8n).  Only the per-row numbers and the sliced heightfields of the kept rows come to the host.  No CPU or eager fallback.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from parc_amd import lib as L
from parc_amd.motion_opt import char_point_samples
from parc_amd.motion_path_gen import NOT_FINISHED_PENALTY, PathMotionGenerator, RolloutResult
from parc_amd.tool_handle import ToolHandle

SDF_PRUNED, SDF_BRUTE = L.MTERR_SDF_PRUNED, L.MTERR_SDF_BRUTE
KERNELS = ("bounds", "fk", "score", "rank", "gather")
SLICE_PADDING = 1.2
STATUS_NONFINITE, STATUS_TOO_LARGE, STATUS_EMPTY = 1, 2, 4
ROW_KEYS = ("contact_loss", "pen_loss", "total_loss", "valid", "status", "num_frames", "slice_min_point", "slice_dims")


class PathSelector(ToolHandle):
    """See the module docstring.  ``points``: (flat [P, 3], body index [P]) replaces ``get_char_point_samples``' defaults."""
    PREFIX, KERNELS = "parc_msel", KERNELS

    def __init__(self, path_generator: PathMotionGenerator, sdf_mode: int = SDF_PRUNED, points=None, slice_padding: float = SLICE_PADDING):
        if not isinstance(path_generator, PathMotionGenerator):
            raise TypeError("path_generator must be a PathMotionGenerator")
        super().__init__(path_generator.device)
        self.pg = pg = path_generator            # kept alive: the handle reads its scene
        cm = pg.generator.char_model
        if points is None:
            _, pts, body = char_point_samples(cm)
        else:
            pts, body = points
        self.points = np.ascontiguousarray(pts, np.float32)
        self.point_body = np.ascontiguousarray(body, np.int32)
        ps = pg.path_settings
        p = L.ParcPathSelectParams()
        p.mpath = pg._h
        p.num_points, p.points_host, p.point_body_host = int(self.points.shape[0]), L.np_f32p(self.points), L.np_i32p(self.point_body)
        for b in range(L.MAX_BODIES):
            p.contact_body_id[b] = b if b < pg.B else -1
        p.w_contact, p.w_pen, p.not_finished_penalty = float(ps.w_contact), float(ps.w_pen), float(NOT_FINISHED_PENALTY)
        p.slice_padding, p.sdf_mode = float(slice_padding), int(sdf_mode)
        self._create_handle(p)

    def _destroy(self):
        super()._destroy()
        self.pg = None

    # ------------------------------------------------------------------ the frames
    def _buffer(self, result: RolloutResult):
        """(tensor that owns the memory, data pointer, frames a row of the buffer holds): the rollout's own buffer where ``result`` is a set of
        views of one (what ``rollout`` returns), else the frames packed anew on the device."""
        pg = self.pg
        rp, FD, F = result.root_pos, pg.FD, int(result.num_frames)
        parts = [rp, result.root_rot, result.joint_rot, result.contacts]
        offs = (0, 3, 7, 7 + 4 * pg.J)
        ok = (rp.dtype == torch.float32 and rp.device == self.device and rp.dim() == 3 and rp.shape[1] == F and rp.stride(2) == 1 and rp.stride(1) == FD
              and rp.stride(0) % FD == 0 and rp.stride(0) >= F * FD)
        ok = ok and all(t.dtype == torch.float32 and t.device == self.device and t.data_ptr() == rp.data_ptr() + 4 * o and t.stride(0) == rp.stride(0)
                        and t.stride(1) == FD and t.stride(-1) == 1 for t, o in zip(parts, offs))
        ok = ok and result.joint_rot.dim() == 4 and result.joint_rot.stride(2) == 4
        if ok:
            return rp, rp.data_ptr(), rp.stride(0) // FD
        buf = pg.pack_frames(result.frames())
        return buf, buf.data_ptr(), int(buf.shape[1])

    # ------------------------------------------------------------------ the run
    def run(self, result: RolloutResult, noise=None, slice_terrain: bool = True, max_contact_loss=None, max_pen_loss=None, max_total_loss=None) -> Dict[str, np.ndarray]:
        """One ``parc_msel_run`` and its results on the host: ``ROW_KEYS`` per row, ``order`` [N] (the rows of path 0 sorted, then those of
        path 1, ...) and ``num_valid`` [P]."""
        pg = self.pg
        pg._need_scene()
        n, P = pg.N, pg.P
        if tuple(result.final_frame.shape) != (n,) or result.root_pos.shape[0] != n:
            raise ValueError(f"result: {result.root_pos.shape[0]} rows, the scene has {n}")
        keep, ptr, stride = self._buffer(result)
        ff = result.final_frame.to(self.device, torch.int32).contiguous()
        a = L.ParcPathSelectArgs()
        a.frames, a.num_frames, a.frame_stride, a.final_frame = ptr, int(result.num_frames), int(stride), ff.data_ptr()
        nz = None
        if noise is not None:
            nz = torch.as_tensor(noise).detach().to(self.device, torch.float32).contiguous()
            if tuple(nz.shape) != (n,):
                raise ValueError(f"noise must have shape ({n},)")
            a.noise = nz.data_ptr()
        a.slice_terrain = int(bool(slice_terrain))
        inf = math.inf
        a.max_contact_loss = inf if max_contact_loss is None else float(max_contact_loss)
        a.max_pen_loss = inf if max_pen_loss is None else float(max_pen_loss)
        a.max_total_loss = inf if max_total_loss is None else float(max_total_loss)
        self._call("run", C.byref(a), self._stream())
        out = dict(contact_loss=np.zeros(n, np.float32), pen_loss=np.zeros(n, np.float32), total_loss=np.zeros(n, np.float32), valid=np.zeros(n, np.int32),
                   status=np.zeros(n, np.int32), num_frames=np.zeros(n, np.int32), slice_min_point=np.zeros((n, 2), np.float32), slice_dims=np.zeros((n, 2), np.int32),
                   order=np.zeros(n, np.int32), num_valid=np.zeros(P, np.int32))
        r = L.ParcPathSelectResults(**{k: (L.np_f32p(v) if v.dtype == np.float32 else L.np_i32p(v)) for k, v in out.items()})
        self._call("results", C.byref(r), self._stream())
        del keep, nz, ff
        return out

    def gather(self, rows: Sequence[int], dims: np.ndarray, status: np.ndarray) -> List[np.ndarray]:
        """The heightfields of the views of ``rows`` of the last run (``dims`` [N, 2], ``status`` [N]: its ``slice_dims`` and ``status``); a
        row with a status bit has no cells."""
        rows = np.ascontiguousarray(rows, np.int32)
        if rows.size == 0:
            return []
        dims = np.where(np.asarray(status)[:, None] != 0, 0, np.asarray(dims))
        sizes = [int(dims[r, 0]) * int(dims[r, 1]) for r in rows]
        flat = np.zeros(max(1, sum(sizes)), np.float32)
        self._call("gather", L.np_i32p(rows), int(rows.size), L.np_f32p(flat), int(flat.size), self._stream())
        out, at = [], 0
        for r, s in zip(rows, sizes):
            out.append(flat[at:at + s].reshape(int(dims[r, 0]), int(dims[r, 1])).copy())
            at += s
        return out

    def describe(self) -> Dict[str, int]:
        out = np.zeros(6, np.int64)
        self._call("describe", out.ctypes.data_as(L.i64p))
        return dict(zip(("launches", "max_rows", "max_frames", "max_slice_dim", "points", "rows"), (int(v) for v in out)))

    # ------------------------------------------------------------------ the selection
    def select(self, result: RolloutResult, top_k: Optional[int] = None, noise=None, seed: Optional[int] = None, slice_terrain: bool = True,
               max_contact_loss=None, max_pen_loss=None, max_total_loss=None) -> List[dict]:
        """Per path a dict: ``path``, ``rows`` (the kept rows), ``total_loss`` (as sorted, noise included), ``contact_loss``, ``pen_loss`` of
        the kept rows, as ``PathMotionGenerator.select``; ``order`` (all rows of the path, sorted), ``num_valid``, ``enough``; with
        ``slice_terrain`` also ``terrains``, the ``(hf, min_point)`` of the kept rows.  With no threshold nothing is filtered: ``rows`` is
        the first ``top_k`` of ``order``.  With any threshold ``rows`` is the first ``top_k`` of the valid rows in sorted order and
        ``enough = num_valid >= top_k``.  ``seed`` draws the noise as ``PathMotionGenerator.select`` does."""
        pg = self.pg
        pg._need_scene()
        k = int(pg.path_settings.top_k if top_k is None else top_k)
        if k < 1:
            raise ValueError("top_k must be >= 1")
        if noise is None and seed is not None:
            noise = torch.randn((pg.N,), generator=torch.Generator().manual_seed(int(seed)))
        filtered = any(v is not None for v in (max_contact_loss, max_pen_loss, max_total_loss))
        r = self.run(result, noise, slice_terrain, max_contact_loss, max_pen_loss, max_total_loss)
        row_path = pg._scene["row_path"]
        sel, at = [], 0
        for p in range(pg.P):
            cnt = int((row_path == p).sum())
            order = r["order"][at:at + cnt].astype(np.int64)
            at += cnt
            rows = (order[r["valid"][order] != 0] if filtered else order)[:k]
            nv = int(r["num_valid"][p])
            sel.append(dict(path=p, rows=rows, total_loss=r["total_loss"][rows], contact_loss=r["contact_loss"][rows], pen_loss=r["pen_loss"][rows], order=order,
                            num_valid=nv, enough=nv >= k))
        if slice_terrain:
            kept = np.concatenate([s["rows"] for s in sel]) if sel else np.zeros(0, np.int64)
            hfs = self.gather(kept, r["slice_dims"], r["status"])
            at = 0
            for s in sel:
                s["terrains"] = [(hfs[at + i], r["slice_min_point"][row].copy()) for i, row in enumerate(s["rows"])]
                at += len(s["rows"])
        self.last_run = r
        return sel
