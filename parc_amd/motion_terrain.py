"""Batched motion-terrain analysis: the reference's ``terrain_util.compute_hf_extra_vals`` (dataset preprocessing and stage 2),
``mdm_path.compute_motion_loss`` with unit weights and the jerk statistics of ``scripts/motion_tests/compute_losses.py``.

B clips of any lengths, each on its own terrain, are packed as for the motion optimiser (``motion_opt.pack_clips``, no constraints)
and analysed in one launch sequence (``parc_amd/csrc/parc_motion_terrain.hpp``).  Per clip: the cells each
frame covers (``hf_mask_inds``, int64 ``[K, 2]`` per frame as the reference stores them), the augmentation bounds ``hf_maxmin``,
``pen_loss`` / ``contact_loss`` against the exact SDF of the whole terrain, ``mean_jerk`` / ``jerk_frac``.  The sample points are
``get_char_point_samples``' defaults, which the reference uses for both passes.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Sequence

import numpy as np

from parc_amd import lib as L
from parc_amd.char_model import CharModel
from parc_amd.motion_opt import model_points_params
from parc_amd.motion_opt import OptClip, char_point_samples, clip_from_ms, clip_struct, pack_clips  # noqa: F401  (re-exported for callers)
from parc_amd.tool_handle import ToolHandle

SDF_PRUNED, SDF_BRUTE = L.MTERR_SDF_PRUNED, L.MTERR_SDF_BRUTE
Z_BUF, JUMP_BUF, MAX_JERK = 3.0, 0.8, 11666.3906
CLIP_OUTPUTS = ("pen_loss", "contact_loss", "mean_jerk", "jerk_frac", "max_root_z", "min_hf")
KERNELS = ("fk", "init", "points", "reduce", "cells", "gather")
MISSING_POINT_VALUE = 99999.9999   # compute_hf_mask_inds' initial lowest point


def analyzer_params(char_model: CharModel, flat_points, point_body, z_buf=Z_BUF, jump_buf=JUMP_BUF, max_jerk=MAX_JERK,
                    sdf_mode=SDF_PRUNED, device: int = 0):
    """``ParcMotionTerrainParams``: every body scored with its own contact column (``compute_motion_loss``' ``contacts[..., b]``)."""
    p = model_points_params(L.ParcMotionTerrainParams(), char_model, flat_points, point_body, device)
    for b in range(char_model.get_num_bodies()):
        p.contact_body_id[b] = b
    p.z_buf, p.jump_buf, p.max_jerk = float(z_buf), float(jump_buf), float(max_jerk)
    p.sdf_mode = int(sdf_mode)
    return p


class MotionTerrainAnalyzer(ToolHandle):
    """``MotionTerrainAnalyzer(char_file, device).analyze(clips)``: ``compute_hf_extra_vals`` + ``compute_motion_loss`` + jerk
    statistics for a whole batch of clips on the GPU.  ``sdf_mode = SDF_BRUTE`` scans every cell for every point (for tests: the
    default ring-pruned search returns the same bits); ``points`` replaces the sampler's points."""
    PREFIX, KERNELS, DEVICE_CONTEXT = "parc_mterr", KERNELS, False

    def __init__(self, char_file: str, device="cuda:0", sdf_mode: int = SDF_PRUNED, points=None):
        super().__init__(device)
        self.char_model = CharModel(char_file)
        if points is None:   # get_char_point_samples' defaults
            _, self.points, self.point_body = char_point_samples(self.char_model)
        else:                # (flat [P, 3], body index [P]), e.g. the reference's own samples
            self.points = np.ascontiguousarray(points[0], np.float32)
            self.point_body = np.ascontiguousarray(points[1], np.int32)
        self.sdf_mode = int(sdf_mode)
        self.B = self.char_model.get_num_bodies()
        self.D = self.char_model.get_dof_size()
        self._key = None
        self._packed = None

    def _handle(self, z_buf, jump_buf, max_jerk):
        key = (float(z_buf), float(jump_buf), float(max_jerk))
        if self._h is None or self._key != key:
            self._destroy()
            self._create_handle(analyzer_params(self.char_model, self.points, self.point_body, *key, sdf_mode=self.sdf_mode,
                                                device=self.device_index))
            self._key = key

    def run(self, clips: Sequence[OptClip], z_buf=Z_BUF, jump_buf=JUMP_BUF, max_jerk=MAX_JERK):
        """The flat outputs of one batched run: ``clip_out`` [C, 6] (``CLIP_OUTPUTS``), ``counts`` [F], ``inds`` int32 [K, 2] in
        frame order, ``hf_maxmin`` [cells, 2] and the packing (``frame_off``, ``hf_off``, ...)."""
        self._handle(z_buf, jump_buf, max_jerk)
        pk = pack_clips(clips, self.B, self.D)
        st = clip_struct(pk, len(clips))
        self._call("set_clips", C.byref(st))
        F, ncell = int(pk["frame_off"][-1]), int(pk["hf_off"][-1])
        out = np.zeros((len(clips), len(CLIP_OUTPUTS)), np.float32)
        counts = np.zeros(F, np.int32)
        maxmin = np.zeros((ncell, 2), np.float32)
        total = C.c_int64()
        self._call("run", L.np_f32p(out), L.np_i32p(counts), L.np_f32p(maxmin), C.byref(total))
        inds = np.zeros((int(total.value), 2), np.int32)
        self._call("get_mask_inds", L.np_i32p(inds) if inds.size else None)
        self._packed = pk
        return dict(packed=pk, clip_out=out, counts=counts, inds=inds, hf_maxmin=maxmin)

    def analyze(self, clips: Sequence[OptClip], z_buf=Z_BUF, jump_buf=JUMP_BUF, max_jerk=MAX_JERK) -> List[dict]:
        """Per clip a dict: the ``CLIP_OUTPUTS`` scores (floats), ``num_frames``, ``hf_mask_inds`` (list of int64 [K, 2], one per
        frame) and ``hf_maxmin`` [X, Y, 2] float32."""
        r = self.run(clips, z_buf, jump_buf, max_jerk)
        pk, counts = r["packed"], r["counts"]
        ind_off = np.zeros(counts.size + 1, np.int64)
        np.cumsum(counts, out=ind_off[1:])
        inds64 = r["inds"].astype(np.int64)
        res = []
        for i, c in enumerate(clips):
            f0, f1 = int(pk["frame_off"][i]), int(pk["frame_off"][i + 1])
            per_frame = [inds64[ind_off[f]:ind_off[f + 1]] for f in range(f0, f1)]
            mm = r["hf_maxmin"][pk["hf_off"][i]:pk["hf_off"][i + 1]].reshape(c.hf.shape[0], c.hf.shape[1], 2).copy()
            d = {k: float(v) for k, v in zip(CLIP_OUTPUTS, r["clip_out"][i])}
            d.update(num_frames=f1 - f0, hf_mask_inds=per_frame, hf_maxmin=mm)
            res.append(d)
        return res

    # ------------------------------------------------------------------ test entries (after run / analyze)
    def min_heights(self):
        """(lowest body point per cell [cells], touched flags [cells]) of the last run, cells in packing order."""
        n = int(self._packed["hf_off"][-1])
        mh, tc = np.zeros(n, np.float32), np.zeros(n, np.int32)
        self._call("get_min_heights", L.np_f32p(mh), L.np_i32p(tc))
        return mh, tc

    def point_sdf(self, frame0: int, num_frames: int):
        """Raw (ground, air) SDF minima [num_frames, P] of the batch's frames [frame0, frame0 + num_frames)."""
        P = self.points.shape[0]
        g, a = np.zeros((num_frames, P), np.float32), np.zeros((num_frames, P), np.float32)
        self._call("point_sdf", int(frame0), int(num_frames), L.np_f32p(g), L.np_f32p(a))
        return g, a
