#!/usr/bin/env python3
"""Generate the hesitation-frame fixtures (``hesitation_*.npz``) from the REAL reference.

Run where the reference checkout is available (the tests only read the fixtures it writes):

    python tests/golden/make_golden_hesitation.py

The reference is driven as in ``make_golden_motion_terrain.py`` (a ``parc`` package alias, empty module stubs, our data-only ms-file
decoder): ``medit_lib.remove_hesitation_frames`` itself runs, on the CPU.  The frames it keeps are read off the index list it hands to
``MotionFrames.get_slice``.  Each ``.npz`` holds inputs, parameters and kept indices only: ``root_pos`` / ``root_rot`` / ``joint_rot`` /
``contacts``, ``source_index`` (the frame of the source clip or the step of the translation each frame was made from),
``hesitation_val``, ``hesitation_min_seq_len``, ``kept`` and ``margin``.

The margin of a case is the smallest ``|d(i, j) - hesitation_val|`` over its pairs (``tests/hesitation_ref.py``, float64).  Every case
must have a margin of at least 1e-4 m: an fp32 forward kinematics on positions of a few metres errs by about 6e-7 per coordinate, under
5e-6 on the norm of 45 numbers, and the margin is twenty times that, so an fp32 implementation must reproduce the kept frames exactly.
A real-clip case at the default value that misses the margin is moved within [0.12, 0.18]; the cases at 0.3 go to the nearest value
that meets it.  The value used is recorded in the fixture.  No case and no frame is left out.

The cases (``cases()`` below) are those of ``tests/test_motion_edit_gpu.py``: the greedy order, holds in a real clip, other parameters on
real motion, runs across the 64-bit word boundaries of the kernel's masks, and the edges.
"""
import os
import sys
import time
import types

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.dont_write_bytecode = True

for _name in ["trimesh", "trimesh.creation", "wandb", "gym", "gym.spaces", "isaacgym", "isaacgym.gymapi", "isaacgym.gymtorch",
              "isaacgym.gymutil"]:
    sys.modules[_name] = types.ModuleType(_name)
sys.modules["wandb"].run = None
sys.modules["trimesh"].creation = sys.modules["trimesh.creation"]
_parc = types.ModuleType("parc")
_parc.__path__ = [os.path.join(REF, "PARC")]
sys.modules["parc"] = _parc

import numpy as np  # noqa: E402
import torch  # noqa: E402

import hesitation_ref as hr  # noqa: E402
from parc_amd import ms_file  # noqa: E402
from parc_amd.char_model import CharModel  # noqa: E402

import parc.anim.kin_char_model as kcm  # noqa: E402
import parc.util.motion_edit_lib as medit_lib  # noqa: E402
import parc.util.motion_util as motion_util  # noqa: E402

torch.set_num_threads(8)
CHAR_FILE = os.path.join(REPO, "data/assets/humanoid.xml")
DEFAULT_VAL, DEFAULT_LEN = 0.15, 4


def load_clip(name):
    m = ms_file.load_ms_file(os.path.join(REPO, "data/motion_terrains", name + ".pkl"), load_misc=False).motion_data
    return dict(root_pos=np.asarray(m.root_pos, np.float32), root_rot=np.asarray(m.root_rot, np.float32),
                joint_rot=np.asarray(m.joint_rot, np.float32), contacts=np.asarray(m.body_contacts, np.float32))


def reindexed(clip, index):
    index = np.asarray(index, np.int64)
    return dict({k: np.ascontiguousarray(v[index]) for k, v in clip.items()}, source_index=index)


def translated(clip, steps, s):
    """Frame 0 of ``clip``, moved along x by ``steps[k] * s`` in frame k."""
    steps = np.asarray(steps, np.int64)
    out = reindexed(clip, np.zeros(len(steps), np.int64))
    out["root_pos"][:, 0] += (steps.astype(np.float64) * s).astype(np.float32)
    out["source_index"] = steps
    return out


def with_copies(n, copies):
    """Steps 0 .. n - 1 with step ``src`` repeated at every frame of ``copies[src]``."""
    steps = np.arange(n)
    for src, frames in copies.items():
        steps[list(frames)] = src
    return steps


def cases():
    civ = load_clip("civilization")
    T = civ["root_pos"].shape[0]
    out = []
    # 1. the greedy order: d = s k sqrt(15) for frames k apart
    for s in (0.03, 0.012, 0.009):
        out.append((f"greedy_s{int(round(s * 1000)):03d}", translated(civ, np.arange(24), s), DEFAULT_VAL, DEFAULT_LEN, None))
    # 2. holds in a real clip: 4 copies after frame 0, 6 after 59, 2 after 119, 5 at the end
    idx = []
    for f in range(T):
        idx += [f] * (1 + {0: 4, 59: 6, 119: 2, T - 1: 5}.get(f, 0))
    out.append(("civilization_holds", reindexed(civ, idx), DEFAULT_VAL, DEFAULT_LEN, (0.12, 0.18)))
    # 3. other parameters on real motion
    for n in (1, 2):
        out.append((f"civilization_v030_m{n}", reindexed(civ, np.arange(T)), 0.3, n, (0.0, 1.0)))
    # 4. the word boundaries of the masks (bits 63 | 64 and 127 | 128), and holds that end on the last frame
    out.append(("word_61_67", translated(civ, with_copies(140, {60: range(61, 68)}), 0.05), DEFAULT_VAL, DEFAULT_LEN, None))
    out.append(("word_126_128", translated(civ, with_copies(140, {125: range(126, 129)}), 0.05), DEFAULT_VAL, DEFAULT_LEN, None))
    out.append(("word_126_129", translated(civ, with_copies(140, {125: range(126, 130)}), 0.05), DEFAULT_VAL, DEFAULT_LEN, None))
    for n in (63, 64, 65, 129):
        out.append((f"tail_{n}", translated(civ, with_copies(n, {n - 6: range(n - 5, n)}), 0.05), DEFAULT_VAL, DEFAULT_LEN, None))
    # 5. the edges
    out.append(("edge_t1", translated(civ, [0], 0.05), DEFAULT_VAL, DEFAULT_LEN, None))
    out.append(("edge_t2", translated(civ, [0, 0], 0.05), DEFAULT_VAL, 1, None))
    out.append(("edge_t3", translated(civ, [0, 0, 0], 0.05), DEFAULT_VAL, 2, None))
    out.append(("edge_t3_short", translated(civ, [0, 0, 0], 0.05), DEFAULT_VAL, DEFAULT_LEN, None))
    out.append(("repeat_70", translated(civ, np.zeros(70, np.int64), 0.05), DEFAULT_VAL, DEFAULT_LEN, None))
    out.append(("min_len_over_t", translated(civ, np.arange(24), 0.009), DEFAULT_VAL, 100, None))
    return out


def meet_margin(body_pos, val, allowed):
    """``val``, or the nearest value within ``allowed`` (steps of 1e-3) whose margin is at least MARGIN_M."""
    dist = hr.pair_distances(body_pos)
    if hr.margin(dist, val) >= hr.MARGIN_M or allowed is None:
        return val
    for k in range(1, 1000):
        for v in (val - 1e-3 * k, val + 1e-3 * k):
            if allowed[0] <= v <= allowed[1] and hr.margin(dist, v) >= hr.MARGIN_M:
                return round(v, 6)
    raise AssertionError("no value meets the margin")


def reference_kept(char, c, val, min_len):
    """The frames the reference keeps: the argument of its get_slice call.  Returns (kept, seconds)."""
    seen = {}
    orig = motion_util.MotionFrames.get_slice

    def capture(self, in_slice):
        seen["kept"] = list(in_slice)
        return orig(self, in_slice)

    motion_util.MotionFrames.get_slice = capture
    try:
        mf = motion_util.MotionFrames(root_pos=torch.tensor(c["root_pos"]), root_rot=torch.tensor(c["root_rot"]),
                                      joint_rot=torch.tensor(c["joint_rot"]), contacts=torch.tensor(c["contacts"]))
        t0 = time.time()
        new = medit_lib.remove_hesitation_frames(mf, char, hesitation_val=val, hesitation_min_seq_len=min_len)
        dt = time.time() - t0
    finally:
        motion_util.MotionFrames.get_slice = orig
    kept = np.asarray(seen["kept"], np.int64)
    assert new.root_pos.shape[0] == kept.size and np.array_equal(new.root_pos.numpy(), c["root_pos"][kept])
    return kept, dt


def main():
    char = kcm.KinCharModel("cpu")
    char.load_char_file(CHAR_FILE)
    cm = CharModel(CHAR_FILE)
    assert tuple(c[0] for c in cases()) == hr.FIXTURES
    for name, c, val, min_len, allowed in cases():
        bp = hr.body_positions(cm, c["root_pos"], c["root_rot"], c["joint_rot"])
        val = meet_margin(bp, val, allowed)
        mg = hr.margin(hr.pair_distances(bp), val)
        assert mg >= hr.MARGIN_M, (name, mg)
        kept, dt = reference_kept(char, c, val, min_len)
        path = os.path.join(HERE, f"hesitation_{name}.npz")
        np.savez_compressed(path, hesitation_val=np.float64(val), hesitation_min_seq_len=np.int32(min_len), kept=kept, margin=np.float64(mg), **c)
        T = c["root_pos"].shape[0]
        print(f"wrote {path} {os.path.getsize(path)} bytes; T {T} val {val} min_len {min_len} margin {mg:.3g} kept {kept.size} "
              f"reference {dt:.2f} s; kept {kept.tolist() if kept.size <= 30 else '...'}")


if __name__ == "__main__":
    main()
