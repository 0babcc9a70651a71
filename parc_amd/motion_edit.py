"""Batched hesitation-frame removal: the reference's ``medit_lib.remove_hesitation_frames`` (``util/motion_edit_lib.py:804-878``), the
step of stage 2 between the kinematic optimiser and ``compute_hf_extra_vals`` (``scripts/parc_2_kin_gen.py:467-470``).

A generated motion that dithers in front of an obstacle holds passages in which the character stands nearly still.  For every clip:
``d(i, j)`` is the norm of ``body_pos[j] - body_pos[i]`` over all bodies at once; the frames are visited in order, a frame that is not
flagged flags every later frame within ``hesitation_val`` of it, and runs of at least ``hesitation_min_seq_len`` consecutive flagged
frames are dropped.  B clips of any lengths (up to ``MAX_FRAMES`` each) are packed as for the motion optimiser
(``motion_opt.pack_clips``) and go through one launch sequence (``parc_amd/csrc/parc_motion_edit.hpp``).
"""
from __future__ import annotations

import ctypes as C
from typing import List, Sequence, Tuple

import numpy as np

from parc_amd import lib as L
from parc_amd.char_model import CharModel
from parc_amd.motion_opt import OptClip, clip_struct, pack_clips
from parc_amd.tool_handle import ToolHandle

HESITATION_VAL, HESITATION_MIN_SEQ_LEN = 0.15, 4   # remove_hesitation_frames' defaults
MAX_FRAMES, FLAG_WORDS = L.MEDIT_MAX_FRAMES, L.MEDIT_FLAG_WORDS
KERNELS = ("fk", "pairs", "scan", "gather")


def _u64p(a):
    assert a.dtype == np.uint64 and a.flags.c_contiguous
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


def unpack_bits(words: np.ndarray, n: int) -> np.ndarray:
    """The first ``n`` bits of 64-bit words ``[..., W]`` (bit ``j & 63`` of word ``j >> 6``) as booleans ``[..., n]``."""
    w = np.ascontiguousarray(words, np.uint64)
    bits = (w[..., :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)
    return bits.reshape(w.shape[:-1] + (-1,))[..., :n].astype(bool)


class HesitationRemover(ToolHandle):
    """``HesitationRemover(char_file, device).remove(clips)``: ``remove_hesitation_frames`` for a whole batch of clips on the GPU."""
    PREFIX, KERNELS, DEVICE_CONTEXT = "parc_medit", KERNELS, False

    def __init__(self, char_file: str, device="cuda:0", hesitation_val: float = HESITATION_VAL,
                 hesitation_min_seq_len: int = HESITATION_MIN_SEQ_LEN):
        super().__init__(device)
        self.char_model = CharModel(char_file)
        self.B = self.char_model.get_num_bodies()
        self.D = self.char_model.get_dof_size()
        self.hesitation_val, self.hesitation_min_seq_len = float(hesitation_val), int(hesitation_min_seq_len)
        p = L.ParcMotionEditParams()
        p.device = self.device_index
        p.model = L.make_char_model(self.char_model)
        p.hesitation_val, p.hesitation_min_seq_len = self.hesitation_val, self.hesitation_min_seq_len
        self._create_handle(p)
        self._packed = None

    def run(self, clips: Sequence[OptClip]):
        """The flat outputs of one batched run: ``counts`` [C], ``kept`` [F] (clip c's kept source frames from ``frame_off[c]`` on,
        -1 behind the first ``counts[c]``), the gathered ``root_pos`` / ``root_rot`` / ``joint_rot`` / ``contacts`` rows and the packing."""
        pk = pack_clips(clips, self.B, self.D)
        st = clip_struct(pk, len(clips))
        self._call("set_clips", C.byref(st))
        self._packed = pk
        F = int(pk["frame_off"][-1])
        counts, kept, total = np.zeros(len(clips), np.int32), np.zeros(F, np.int32), C.c_int64()
        self._call("run", L.np_i32p(counts), L.np_i32p(kept), C.byref(total))
        n, J = int(total.value), self.B - 1
        rp, rr = np.zeros((n, 3), np.float32), np.zeros((n, 4), np.float32)
        jr, ct = np.zeros((n, J, 4), np.float32), np.zeros((n, self.B), np.float32)
        self._call("get_frames", L.np_f32p(rp), L.np_f32p(rr), L.np_f32p(jr), L.np_f32p(ct))
        return dict(packed=pk, counts=counts, kept=kept, root_pos=rp, root_rot=rr, joint_rot=jr, contacts=ct)

    def remove(self, clips: Sequence[OptClip]) -> Tuple[List[OptClip], List[np.ndarray]]:
        """``(new_clips, kept_indices)``: every clip without its hesitation frames, and per clip the int64 source indices of the frames
        that stay.  The kept rows are copies, bit-identical to the input rows; nothing is re-stitched.  Terrain, ``hf_maxmin``, fps and
        name are carried over.  The constraint arrays pass through unchanged, frame ranges included: the reference also saves the
        constraints of the unshortened clip with the shortened motion (``parc_2_kin_gen.py:467-489``)."""
        r = self.run(clips)
        off = r["packed"]["frame_off"]
        out, inds, o = [], [], 0
        for i, c in enumerate(clips):
            n = int(r["counts"][i])
            inds.append(r["kept"][off[i]:off[i] + n].astype(np.int64))
            sl = slice(o, o + n)
            out.append(OptClip(r["root_pos"][sl].copy(), r["root_rot"][sl].copy(), r["joint_rot"][sl].copy(), r["contacts"][sl].copy(),
                               c.hf, c.min_point, c.dx, c.fps, c.name, c.cons_body, c.cons_start, c.cons_end, c.cons_point, c.hf_maxmin))
            o += n
        return out, inds

    # ------------------------------------------------------------------ test entries (after run / remove)
    def pair_mask(self, clip: int) -> np.ndarray:
        """The pair mask of clip ``clip`` of the last run, booleans [T, T]: ``[i, j]`` is set when ``j > i`` and ``d(i, j) < hesitation_val``."""
        off = self._packed["frame_off"]
        T = int(off[clip + 1] - off[clip])
        rows = np.zeros((T, (T + 63) // 64), np.uint64)
        self._call("get_pair_rows", int(clip), _u64p(rows))
        return unpack_bits(rows, T)

    def flags(self) -> Tuple[List[np.ndarray], List[np.ndarray]]:
        """Per clip of the last run the flagged frames, booleans [T]: after the ordered scan, and after the run filter."""
        off = self._packed["frame_off"]
        n = len(off) - 1
        raw, fil = np.zeros((n, FLAG_WORDS), np.uint64), np.zeros((n, FLAG_WORDS), np.uint64)
        self._call("get_flags", _u64p(raw), _u64p(fil))
        T = [int(off[i + 1] - off[i]) for i in range(n)]
        return [unpack_bits(raw[i], T[i]) for i in range(n)], [unpack_bits(fil[i], T[i]) for i in range(n)]
