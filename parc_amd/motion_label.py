"""Batched contact labelling, penetration lift and resampling of raw clips: what the reference's editor does one clip at a time behind
its "Automatic Contact Labelling" buttons (``motionscope/include/contact_editing_gui.py:46-85``), restated from
``util/motion_edit_lib.py``:

* ``compute_hf_foot_contacts_and_correct_pen`` (``:472-524``): a foot touches when a corner of its box is below the height of the cell
  under that corner plus ``contact_eps``; the clip is lifted, frame by frame, by the deepest penetration of either foot;
* ``compute_motion_terrain_hand_contacts`` (``:526-565``): a hand touches when the SDF of the whole terrain at its sphere is below
  ``contact_eps``;
* ``compute_ground_plane_foot_contacts`` / ``correct_foot_ground_pen`` (``:430-470``, ``:567-604``) for clips on flat ground;
* ``change_motion_fps`` (``:752-784``): ``MotionLib.calc_motion_frame`` (CLAMP) at the times of its loop.

Clips of any lengths, each on its own terrain, are packed as for the motion optimiser (``motion_opt.pack_clips``) and go through one
launch sequence (``parc_amd/csrc/parc_motion_label.hpp``).  The labels, ``gap``, ``lift`` and ``hand_sd`` always
come from the pose before the lift, as in the reference.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import replace
from typing import List, Optional, Sequence, Tuple

import numpy as np

from parc_amd import lib as L
from parc_amd.char_model import CharModel, GeomType
from parc_amd.motion_opt import OptClip, clip_struct, pack_clips
from parc_amd.tool_handle import ToolHandle

CONTACT_EPS = 0.04                                   # the reference's default in all four functions
FOOT_BODIES, HAND_BODIES = ("left_foot", "right_foot"), ("left_hand", "right_hand")
FLAT_TERRAIN_DX, FLAT_TERRAIN_PADDING = 0.1, 5.0     # create_terrain_for_motion's defaults
KERNELS = ("feet", "hands", "resample")


def _body_id(cm: CharModel, name: str) -> int:
    names = list(cm.get_body_names())
    if name not in names:
        raise ValueError(f"unknown body {name!r}; the character has {names}")
    return names.index(name)


def labeller_params(cm: CharModel, device: int = 0, contact_eps: float = CONTACT_EPS, foot_bodies: Sequence[str] = FOOT_BODIES,
                    hand_bodies: Sequence[str] = HAND_BODIES) -> L.ParcMotionLabelParams:
    """``ParcMotionLabelParams`` of a character; refuses, naming the body, an unknown body name, a foot whose first geom is not a box
    and a hand whose first geom is not a sphere.  A foot's further box geoms are listed too: the ground-plane lift takes all of them."""
    if len(foot_bodies) != 2 or len(hand_bodies) != 2:
        raise ValueError("foot_bodies and hand_bodies name two bodies each (left, right)")
    p = L.ParcMotionLabelParams()
    p.struct_size = C.sizeof(p)
    p.device = int(device)
    p.model = L.make_char_model(cm)
    p.contact_eps = float(contact_eps)
    q = 0
    for k, name in enumerate(foot_bodies):
        b = _body_id(cm, name)
        geoms = cm._geoms[b]
        if not geoms or geoms[0].shape != GeomType.BOX:
            raise ValueError(f"foot body {name!r}: its first geom must be a box")
        p.foot_body[k] = b
        for g in (g for g in geoms if g.shape == GeomType.BOX):
            if q >= L.MLABEL_MAX_FOOT_BOXES:
                raise ValueError(f"foot body {name!r}: more than {L.MLABEL_MAX_FOOT_BOXES} box geoms on the feet")
            p.box_foot[q] = k
            for d in range(3):
                p.box_offset[q][d], p.box_half[q][d] = float(g.pos[d]), float(g.size[d])
            q += 1
    p.num_foot_boxes = q
    for k, name in enumerate(hand_bodies):
        b = _body_id(cm, name)
        geoms = cm._geoms[b]
        if not geoms or geoms[0].shape != GeomType.SPHERE:
            raise ValueError(f"hand body {name!r}: its first geom must be a sphere")
        p.hand_body[k], p.hand_radius[k] = b, float(geoms[0].size[0])
    return p


def flat_terrain_for(clip, dx: float = FLAT_TERRAIN_DX, padding: float = FLAT_TERRAIN_PADDING) -> Tuple[np.ndarray, np.ndarray, float]:
    """``create_terrain_for_motion`` (``motion_edit_lib.py:244-299``) on the host: ``(hf, min_point, dx)`` of the flat terrain, height 0,
    that covers the root's path with ``padding`` metres around it.  ``clip`` is an ``OptClip`` or a ``[T, 3]`` array of root positions."""
    rp = np.asarray(getattr(clip, "root_pos", clip), np.float32)
    dx = float(dx)
    num_padding = int(round(padding / dx))
    hi_x, hi_y, lo_x, lo_y = float(rp[:, 0].max()), float(rp[:, 1].max()), float(rp[:, 0].min()), float(rp[:, 1].min())
    pos_x, neg_x = int(abs(round(hi_x / dx))) + num_padding, int(abs(round(lo_x / dx))) + num_padding
    pos_y, neg_y = int(abs(round(hi_y / dx))) + num_padding, int(abs(round(lo_y / dx))) + num_padding
    hf = np.zeros((neg_x + pos_x + 1, neg_y + pos_y + 1), np.float32)
    # an fp32 tensor element minus a Python float: the float is rounded to fp32 first
    min_point = np.array([rp[0, 0] - np.float32(dx * neg_x), rp[0, 1] - np.float32(dx * neg_y)], np.float32)
    return hf, min_point, dx


def motion_length(num_frames: int, fps) -> float:
    """``MotionLib``'s length of a clip: ``1 / fps * (frames - 1)`` stored as fp32 (``motion_lib.py:184-186``)."""
    return float(np.float32(1.0 / fps * (num_frames - 1)))


def resample_times(num_frames: int, fps, target_fps) -> np.ndarray:
    """The times of ``change_motion_fps``' loop, fp32: ``t = 0.0; while t < length: ...; t += 1 / target_fps`` in Python floats."""
    if not target_fps > 0:
        raise ValueError(f"target_fps must be > 0, got {target_fps}")
    length, dt, t, out = motion_length(num_frames, fps), 1.0 / target_fps, 0.0, []
    while t < length:
        out.append(t)
        t += dt
    return np.asarray(out, np.float32)


class ContactLabeller(ToolHandle):
    """``ContactLabeller(char_file, device).label(clips)``: the editor's automatic contact labelling for a whole batch of clips on the GPU."""
    PREFIX, KERNELS, DEVICE_CONTEXT = "parc_mlabel", KERNELS, False

    def __init__(self, char_file: str, device="cuda:0", contact_eps: float = CONTACT_EPS, foot_bodies: Sequence[str] = FOOT_BODIES,
                 hand_bodies: Sequence[str] = HAND_BODIES):
        super().__init__(device)
        self.char_model = CharModel(char_file)
        self.B = self.char_model.get_num_bodies()
        self.D = self.char_model.get_dof_size()
        self.contact_eps = float(contact_eps)
        p = labeller_params(self.char_model, self.device_index, contact_eps, foot_bodies, hand_bodies)
        self.foot_ids, self.hand_ids = list(p.foot_body), list(p.hand_body)
        self._create_handle(p)

    def _upload(self, clips: Sequence[OptClip]):
        """set_clips; a clip without a terrain (``hf`` None) is packed with one cell at height 0.  Returns (packing, clips without)."""
        bare = [i for i, c in enumerate(clips) if c.hf is None]
        full = [replace(c, hf=np.zeros((1, 1), np.float32), min_point=np.zeros(2, np.float32), dx=1.0) if c.hf is None else c for c in clips]
        pk = pack_clips(full, self.B, self.D)
        st = clip_struct(pk, len(clips))
        self._call("set_clips", C.byref(st))
        return pk, bare

    def run(self, clips: Sequence[OptClip], hands: bool = True, correct_pen: bool = True, ground_height: Optional[float] = None,
            keep_existing: bool = False):
        """The flat outputs of one batched run: ``contacts`` [F, B], ``gap`` [F, 2] (left, right foot), ``lift`` [F], ``hand_sd`` [F, 2]
        (+inf where the hands were not labelled), the corrected ``root_pos`` [F, 3] and the packing.  With ``ground_height`` the plane at
        that height replaces the terrains and the hands are not labelled; clips without a terrain need it (0.0 when every clip is
        without one)."""
        pk, bare = self._upload(clips)
        if ground_height is None and bare:
            if len(bare) != len(clips):
                raise ValueError(f"clip {bare[0]} ({clips[bare[0]].name!r}) has no terrain: give ground_height, or a terrain "
                                 "(flat_terrain_for)")
            ground_height = 0.0
        ground = ground_height is not None
        self._call("run", int(bool(hands)), int(bool(correct_pen)), int(ground), float(ground_height or 0.0), int(bool(keep_existing)))
        F = int(pk["frame_off"][-1])
        rp, ct = np.zeros((F, 3), np.float32), np.zeros((F, self.B), np.float32)
        gap, lift, sd = np.zeros((F, 2), np.float32), np.zeros(F, np.float32), np.zeros((F, 2), np.float32)
        self._call("get_frames", L.np_f32p(rp), L.np_f32p(ct))
        self._call("get_gap", L.np_f32p(gap))
        self._call("get_lift", L.np_f32p(lift))
        self._call("get_hand_sd", L.np_f32p(sd))
        return dict(packed=pk, contacts=ct, gap=gap, lift=lift, hand_sd=sd, root_pos=rp)

    def label(self, clips: Sequence[OptClip], hands: bool = True, correct_pen: bool = True, ground_height: Optional[float] = None,
              keep_existing: bool = False) -> List[OptClip]:
        """Every clip with its labelled ``contacts`` and, with ``correct_pen``, its lifted root.  Rotations, terrain, fps, name and the
        constraint arrays are carried over."""
        r = self.run(clips, hands, correct_pen, ground_height, keep_existing)
        off = r["packed"]["frame_off"]
        return [replace(c, root_pos=r["root_pos"][off[i]:off[i + 1]].copy(), contacts=r["contacts"][off[i]:off[i + 1]].copy())
                for i, c in enumerate(clips)]

    def resample(self, clips: Sequence[OptClip], target_fps) -> List[OptClip]:
        """``change_motion_fps`` for every clip: its frames at ``resample_times``, fps ``target_fps``.  The output is quaternions (no
        exp-map round trip).  A clip of one frame has length 0 and the reference's loop yields nothing: it is refused, by name."""
        if not target_fps > 0:
            raise ValueError(f"target_fps must be > 0, got {target_fps}")
        for i, c in enumerate(clips):
            if c.num_frames < 2:
                raise ValueError(f"clip {i} ({c.name!r}) has one frame: nothing to resample")
        times = [resample_times(c.num_frames, c.fps, target_fps) for c in clips]
        self._upload(clips)
        off = np.zeros(len(clips) + 1, np.int64)
        off[1:] = np.cumsum([t.size for t in times])
        t_all = np.ascontiguousarray(np.concatenate(times), np.float32)
        lengths = np.asarray([motion_length(c.num_frames, c.fps) for c in clips], np.float32)
        N, J = int(off[-1]), self.B - 1
        rp, rr = np.zeros((N, 3), np.float32), np.zeros((N, 4), np.float32)
        jr, ct = np.zeros((N, J, 4), np.float32), np.zeros((N, self.B), np.float32)
        self._call("resample", off.ctypes.data_as(L.i64p), L.np_f32p(t_all), L.np_f32p(lengths), L.np_f32p(rp), L.np_f32p(rr),
                   L.np_f32p(jr), L.np_f32p(ct))
        none = np.zeros(0, np.int32)   # body constraints hold frame ranges of the old rate: not carried over
        return [replace(c, root_pos=rp[off[i]:off[i + 1]].copy(), root_rot=rr[off[i]:off[i + 1]].copy(),
                        joint_rot=jr[off[i]:off[i + 1]].copy(), contacts=ct[off[i]:off[i + 1]].copy(), fps=target_fps, cons_body=none,
                        cons_start=none, cons_end=none, cons_point=np.zeros((0, 3), np.float32))
                for i, c in enumerate(clips)]
