"""A float64 numpy restatement of the reference editor's automatic contact labelling (``util/motion_edit_lib.py:430-604``) and of
``change_motion_fps`` (``:752-784``), written from their steps:

* feet: the eight corners of a foot's first box; the cell under each corner by ``get_grid_index`` (round half to even of a division,
  clamped); ``contact = any(z < h + eps)``, ``gap = min(z - h)``, ``lift = -min(0, gap_left, gap_right)``;
* hands: ``sd = min over all cells of sdBox(p - centre, half) - r``, each cell a column from ``min(hf) - 10`` up to its height;
* the ground plane: ``contact = any(z - ground - eps < 0)``, ``lift = ground - min(ground, every corner of every box of the feet)``;
* resampling: ``MotionLib.calc_motion_frame`` (CLAMP): lerp of root position and contacts, slerp of the normalised rotations.

It also reports which decisions are settled: a foot decision when ``|min_c(z_c - h_c - eps)| >= MARGIN_M`` and no corner lies within
``MARGIN_CELL`` of a boundary between cells of different height, a hand decision when ``|sd - eps| >= MARGIN_M``.  On a settled decision
an fp32 implementation must give the same flag.  ``tests/test_motion_label_cpu.py`` checks it against the reference fixtures; it is
the CPU-side statement of what the HIP kernels (``parc_motion_label.hpp``) compute.
"""
import os

import numpy as np

MARGIN_M, MARGIN_CELL = 1e-4, 1e-4   # twenty times the error of an fp32 FK at these positions
MAX_UNSETTLED = 0.02                 # the cap on unsettled decisions per case (the generator asserts it)
TOL_M = 1e-5                         # the project's standing fp32 FK parity figure
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# tests/golden/motion_label_<name>.npz, in the order of the generator's cases
BUNDLED = ("sfu", "civilization", "TEASER_TERRAIN", "dec2024_teaser_717_1_opt_dm")
LABEL_FIXTURES = tuple("bundled_" + n for n in BUNDLED) + ("edge_t1", "edge_t65", "edge_t129", "off_grid", "side_wall", "deep_pen",
                                                           "eps_000", "eps_100", "ground_sfu", "ground_civilization")
RESAMPLE_FIXTURES = ("resample_20", "resample_45", "resample_60", "resample_30", "resample_t2")


def load(name):
    with np.load(os.path.join(GOLDEN, f"motion_label_{name}.npz")) as z:
        return {k: z[k] for k in z.files}


def tolerance(fx, key="ref_err"):
    """max(1e-5, 4 x the largest difference between the reference's fp32 result and this restatement, recorded in the fixture): metres,
    or radians for the rotations of the resampling cases (``ref_err_rot``)."""
    return max(TOL_M, 4.0 * float(fx[key]))


def qmul(a, b):   # torch_util.quat_mul is the Hamilton product
    x1, y1, z1, w1 = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    x2, y2, z2, w2 = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2,
                     w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2, w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2], -1)


def qrot(q, v):
    t = 2.0 * np.cross(q[..., :3], v)
    return v + q[..., 3:] * t + np.cross(q[..., :3], t)


def fk(cm, root_pos, root_rot, joint_rot):
    """Body positions [T, B, 3] and rotations [T, B, 4] in float64 (kin_char_model.py:617-649)."""
    root_pos, root_rot, joint_rot = (np.asarray(a, np.float64) for a in (root_pos, root_rot, joint_rot))
    lt, lr = np.asarray(cm._local_translation, np.float64), np.asarray(cm._local_rotation, np.float64)
    pos, rot = [root_pos], [root_rot]
    for j in range(1, cm.get_num_bodies()):
        p = int(cm._parent_indices[j])
        pos.append(pos[p] + qrot(rot[p], np.broadcast_to(lt[j], pos[p].shape)))
        rot.append(qmul(rot[p], qmul(np.broadcast_to(lr[j], rot[p].shape), joint_rot[:, j - 1])))
    return np.stack(pos, 1), np.stack(rot, 1)


def box_corners(pos, rot, offset, half):
    """[T, 8, 3]: offset + (+-hx, +-hy, +-hz), rotated by the body and added to its position (geom_util.py:82-113)."""
    signs = np.array([[sx, sy, sz] for sz in (-1, 1) for sy in (-1, 1) for sx in (-1, 1)], np.float64)
    local = signs * np.asarray(half, np.float64) + np.asarray(offset, np.float64)
    return qrot(rot[:, None, :], np.broadcast_to(local, (pos.shape[0], 8, 3))) + pos[:, None, :]


def foot_boxes(cm, name):
    """(offset, half) of every box geom of a body, its first geom first."""
    from parc_amd.char_model import GeomType
    geoms = cm._geoms[cm.get_body_id(name)]
    assert geoms[0].shape == GeomType.BOX
    return [(np.asarray(g.pos, np.float64), np.asarray(g.size, np.float64)) for g in geoms if g.shape == GeomType.BOX]


def grid_cells(p, mn, d, dim):
    """get_grid_index on one axis, and how far the point is from the nearest cell boundary, in cells."""
    u = (np.asarray(p, np.float64) - mn) / d
    idx = np.clip(np.rint(u), 0, dim - 1).astype(np.int64)
    other = np.clip(np.where(u > np.rint(u), np.rint(u) + 1, np.rint(u) - 1), 0, dim - 1).astype(np.int64)   # the cell across it
    return idx, other, np.abs(np.abs(u - np.rint(u)) - 0.5)


def label_feet(cm, clip, eps, feet=("left_foot", "right_foot")):
    """On the clip's terrain.  dict: ``contact`` [T, 2] bool, ``gap`` [T, 2], ``lift`` [T], ``settled`` [T, 2] bool."""
    pos, rot = fk(cm, clip["root_pos"], clip["root_rot"], clip["joint_rot"])
    hf, mn, d = np.asarray(clip["hf"], np.float64), np.asarray(clip["min_point"], np.float64), float(np.float32(clip["dx"]))
    T = pos.shape[0]
    contact, gap, settled = np.zeros((T, 2), bool), np.zeros((T, 2)), np.zeros((T, 2), bool)
    for k, name in enumerate(feet):
        b = cm.get_body_id(name)
        off, half = foot_boxes(cm, name)[0]
        pts = box_corners(pos[:, b], rot[:, b], off, half)
        ix, ox, ex = grid_cells(pts[..., 0], mn[0], d, hf.shape[0])
        iy, oy, ey = grid_cells(pts[..., 1], mn[1], d, hf.shape[1])
        h = hf[ix, iy]
        near = ((ex < MARGIN_CELL) & (hf[ox, iy] != h)) | ((ey < MARGIN_CELL) & (hf[ix, oy] != h)) | \
               ((ex < MARGIN_CELL) & (ey < MARGIN_CELL) & (hf[ox, oy] != h))
        contact[:, k] = (pts[..., 2] < h + eps).any(-1)
        gap[:, k] = (pts[..., 2] - h).min(-1)
        settled[:, k] = (np.abs((pts[..., 2] - h - eps).min(-1)) >= MARGIN_M) & ~near.any(-1)
    return dict(contact=contact, gap=gap, lift=-np.minimum(0.0, gap.min(-1)), settled=settled)


def sd_box(p, half):
    q = np.abs(p) - half
    return np.linalg.norm(np.maximum(q, 0.0), axis=-1) + np.minimum(q.max(-1), 0.0)


def terrain_sd(points, hf, min_point, dx, radius):
    """points_hf_sdf(..., inverted=False, radius=r) (terrain_util.py:1736-1794): [N] for points [N, 3], over every cell."""
    hf = np.asarray(hf, np.float64)
    X, Y = hf.shape
    base_z = float(hf.min()) - 10.0
    cx = np.linspace(0.0, (X - 1.0) * dx, X) + float(min_point[0])
    cy = np.linspace(0.0, (Y - 1.0) * dx, Y) + float(min_point[1])
    centre = np.stack([np.broadcast_to(cx[:, None], (X, Y)), np.broadcast_to(cy[None, :], (X, Y)), (hf + base_z) / 2.0], -1).reshape(-1, 3)
    half = np.stack([np.full((X, Y), dx / 2.0), np.full((X, Y), dx / 2.0), (hf - base_z) / 2.0], -1).reshape(-1, 3)
    out = np.empty(points.shape[0])
    for n, p in enumerate(np.asarray(points, np.float64)):
        out[n] = sd_box(p[None, :] - centre, half).min() - radius
    return out


def label_hands(cm, clip, eps, hands=("left_hand", "right_hand")):
    """dict: ``contact`` [T, 2] bool, ``sd`` [T, 2], ``settled`` [T, 2] bool."""
    pos, _ = fk(cm, clip["root_pos"], clip["root_rot"], clip["joint_rot"])
    sd = np.stack([terrain_sd(pos[:, cm.get_body_id(n)], clip["hf"], clip["min_point"], float(np.float32(clip["dx"])),
                              float(cm._geoms[cm.get_body_id(n)][0].size[0])) for n in hands], -1)
    return dict(contact=sd < eps, sd=sd, settled=np.abs(sd - eps) >= MARGIN_M)


def label_ground(cm, clip, eps, ground_height=0.0, feet=("left_foot", "right_foot")):
    """On the plane.  dict: ``contact`` [T, 2] bool, ``gap`` [T, 2], ``lift`` [T], ``settled`` [T, 2] bool."""
    pos, rot = fk(cm, clip["root_pos"], clip["root_rot"], clip["joint_rot"])
    T = pos.shape[0]
    contact, gap, low = np.zeros((T, 2), bool), np.zeros((T, 2)), np.full(T, float(ground_height))
    for k, name in enumerate(feet):
        b = cm.get_body_id(name)
        for q, (off, half) in enumerate(foot_boxes(cm, name)):
            z = box_corners(pos[:, b], rot[:, b], off, half)[..., 2]
            low = np.minimum(low, z.min(-1))
            if q == 0:
                contact[:, k] = (z - ground_height - eps < 0.0).any(-1)
                gap[:, k] = (z - ground_height).min(-1)
    return dict(contact=contact, gap=gap, lift=ground_height - low, settled=np.abs(gap - eps) >= MARGIN_M)


def contacts_array(cm, feet, hands=None, feet_names=("left_foot", "right_foot"), hand_names=("left_hand", "right_hand")):
    """The reference's new contact array [T, B]: the feet's columns, the hands' when given, 0 elsewhere."""
    out = np.zeros((feet.shape[0], cm.get_num_bodies()), np.float32)
    for k, n in enumerate(feet_names):
        out[:, cm.get_body_id(n)] = feet[:, k]
    if hands is not None:
        for k, n in enumerate(hand_names):
            out[:, cm.get_body_id(n)] = hands[:, k]
    return out


# ---- resampling ---------------------------------------------------------------------------------------------------------------
def quat_normalize(q):
    q = np.where(q[..., 3:] < 0, -q, q)
    return q / np.maximum(np.linalg.norm(q, axis=-1, keepdims=True), 1e-9)


def slerp(q0, q1, t):
    """torch_util.slerp (:475-499) with its two fall-backs; t broadcasts against q[..., 0]."""
    c = (q0 * q1).sum(-1)
    q1 = np.where((c < 0)[..., None], -q1, q1)
    c = np.abs(c)[..., None]
    t = t[..., None]
    with np.errstate(divide="ignore", invalid="ignore"):
        h = np.arccos(np.minimum(c, 1.0))
        s = np.sqrt(np.maximum(1.0 - c * c, 0.0))
        out = np.sin((1 - t) * h) / s * q0 + np.sin(t * h) / s * q1
    out = np.where(np.abs(s) < 0.001, 0.5 * q0 + 0.5 * q1, out)
    return np.where(np.abs(c) >= 1, q0, out)


def resample(clip, times, length):
    """calc_motion_frame (CLAMP) at ``times`` (seconds) for a clip of MotionLib length ``length``: root_pos, root_rot, joint_rot, contacts."""
    rp, ct = np.asarray(clip["root_pos"], np.float64), np.asarray(clip["contacts"], np.float64)
    rr, jr = quat_normalize(np.asarray(clip["root_rot"], np.float64)), quat_normalize(np.asarray(clip["joint_rot"], np.float64))
    T = rp.shape[0]
    phase = np.clip(np.asarray(times, np.float64) / float(length), 0.0, 1.0)
    i0 = np.minimum((phase * (T - 1)).astype(np.int64), T - 1)
    i1 = np.minimum(i0 + 1, T - 1)
    bl = phase * (T - 1) - i0
    b1 = bl[:, None]
    return dict(root_pos=(1 - b1) * rp[i0] + b1 * rp[i1], root_rot=slerp(rr[i0], rr[i1], bl),
                joint_rot=slerp(jr[i0], jr[i1], np.broadcast_to(b1, jr[i0].shape[:2])), contacts=(1 - b1) * ct[i0] + b1 * ct[i1])


def quat_angle(a, b):
    """The angle of the difference quaternion of unit quaternions, radians: 2 atan2(|v|, |w|) of a (x) conj(b)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d = qmul(a, b * np.array([-1.0, -1.0, -1.0, 1.0]))
    return 2.0 * np.arctan2(np.linalg.norm(d[..., :3], axis=-1), np.abs(d[..., 3]))
