"""A float64 numpy restatement of the reference's ``medit_lib.remove_hesitation_frames`` (``util/motion_edit_lib.py:804-878``), written
from its five steps:

1. body positions ``[T, B, 3]`` by forward kinematics;
2. ``d(i, j)``: ONE norm of ``body_pos[j] - body_pos[i]`` over all ``B x 3`` numbers;
3. the ordered scan: frame i, unless flagged itself, flags every ``j > i`` with ``d(i, j) < hesitation_val``;
4. runs of consecutive flagged frames shorter than ``hesitation_min_seq_len`` are unflagged again;
5. the frames that are not flagged stay, in order.

It also reports the margin of a clip: the smallest ``|d(i, j) - hesitation_val|`` over all pairs.  Where the margin is far above the
rounding of an fp32 forward kinematics, the pair mask, the flags and the kept frames of an fp32 implementation equal these exactly.
``tests/test_motion_edit_cpu.py`` checks it against the reference fixtures; it is the CPU-side statement of what the HIP kernels
(``parc_motion_edit.hpp``) compute.
"""
import numpy as np

MARGIN_M = 1e-4   # every fixture's margin is at least this (tests/golden/make_golden_hesitation.py asserts it)
# tests/golden/hesitation_<name>.npz, in the order of the generator's cases
FIXTURES = ("greedy_s030", "greedy_s012", "greedy_s009", "civilization_holds", "civilization_v030_m1", "civilization_v030_m2",
            "word_61_67", "word_126_128", "word_126_129", "tail_63", "tail_64", "tail_65", "tail_129", "edge_t1", "edge_t2", "edge_t3",
            "edge_t3_short", "repeat_70", "min_len_over_t")


def qmul(a, b):
    x1, y1, z1, w1 = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    x2, y2, z2, w2 = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2,
                     w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2, w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2], -1)


def qrot(q, v):
    t = 2.0 * np.cross(q[..., :3], v)
    return v + q[..., 3:] * t + np.cross(q[..., :3], t)


def body_positions(cm, root_pos, root_rot, joint_rot):
    """[T, B, 3] in float64 (kin_char_model.py:617-649)."""
    root_pos, root_rot, joint_rot = (np.asarray(a, np.float64) for a in (root_pos, root_rot, joint_rot))
    lt = np.asarray(cm._local_translation, np.float64)
    lr = np.asarray(cm._local_rotation, np.float64)
    pos, rot = [root_pos], [root_rot]
    for j in range(1, cm.get_num_bodies()):
        p = int(cm._parent_indices[j])
        pos.append(pos[p] + qrot(rot[p], np.broadcast_to(lt[j], pos[p].shape)))
        rot.append(qmul(rot[p], qmul(np.broadcast_to(lr[j], rot[p].shape), joint_rot[:, j - 1])))
    return np.stack(pos, 1)


def pair_distances(body_pos):
    """[T, T]: d(i, j), one norm over all bodies and coordinates."""
    flat = body_pos.reshape(body_pos.shape[0], -1)
    return np.sqrt(((flat[None, :, :] - flat[:, None, :]) ** 2).sum(-1))


def margin(dist, hesitation_val):
    """The smallest |d(i, j) - hesitation_val| over the pairs j > i (inf for a clip of one frame)."""
    iu = np.triu_indices(dist.shape[0], 1)
    return float(np.abs(dist[iu] - hesitation_val).min()) if iu[0].size else float("inf")


def run_filter(raw, min_seq_len):
    """``raw`` without its runs of consecutive flagged frames shorter than ``min_seq_len``."""
    flags, T, j = raw.copy(), raw.shape[0], 0
    while j < T:
        if not raw[j]:
            j += 1
            continue
        e = j
        while e < T and raw[e]:
            e += 1
        if e - j < min_seq_len:
            flags[j:e] = False
        j = e
    return flags


def remove_hesitation(body_pos, hesitation_val=0.15, hesitation_min_seq_len=4):
    """dict: ``pair_mask`` [T, T] (j > i and d < val), ``flags_raw`` / ``flags`` [T] (after the scan / after the run filter),
    ``kept`` int64 (the frames that stay) and ``margin``."""
    T = body_pos.shape[0]
    dist = pair_distances(body_pos)
    mask = np.triu(dist < hesitation_val, 1)
    raw = np.zeros(T, bool)
    for i in range(T):
        if not raw[i]:
            raw |= mask[i]
    flags = run_filter(raw, hesitation_min_seq_len)
    return dict(pair_mask=mask, flags_raw=raw, flags=flags, kept=np.nonzero(~flags)[0].astype(np.int64), margin=margin(dist, hesitation_val))


def any_earlier_rule(body_pos, hesitation_val=0.15, hesitation_min_seq_len=4):
    """The WRONG rule, for the tests that tell the two apart: frame j is flagged when ANY earlier frame is near, flagged or not."""
    raw = np.triu(pair_distances(body_pos) < hesitation_val, 1).any(0)
    return np.nonzero(~run_filter(raw, hesitation_min_seq_len))[0].astype(np.int64)
