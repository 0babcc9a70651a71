"""Numpy restatement of the motion-terrain augmenter: the reference's ``run_simple_augment_motions.py:144-202``
(window, heading, x / y scale, ``SubTerrain.pad``, ``slice_terrain_around_motion``, ``HEIGHT_SCALE`` / ``BOXES_ALONG_PATH``) and stage 2's
mirrored copies (``flip_motion_about_XZ_plane``, ``flip_by_XZ_axis``) from one *plan* entry, in fp32 and in the reference's association.
Next to each heightfield it computes the *unstable* mask in the sense of ``tests/terrain_gen_ref.py``: cells whose lookup lies within
``NUDGE`` of a rounding tie, and cells within ``EDGE_EPS`` of a box edge, the only ones where two fp32 implementations may differ.

A clip is a dict ``root_pos [n, 3]``, ``root_rot [n, 4]`` (xyzw), ``joint_rot [n, J, 4]``, ``contacts [n, B]``, ``hf [X, Y]``,
``hf_maxmin [X, Y, 2]`` or ``None``, ``min_point [2]``, ``dx``.  A variation is a dict ``start``, ``nf``, ``heading`` (radians), ``sx``,
``sy``, ``mirror``, ``hscale``, ``nb``, ``box_frame [nb]``, ``boxes [nb, 4]`` = (len x, len y in cells, angle, height).  ``model`` holds
``jtype [B]``, ``axis [B, 3]``, ``jswap [B]``, ``cswap [B]``.
"""
import numpy as np

from terrain_gen_ref import _box_test

F = np.float32
MODES = ("HEIGHT_SCALE", "BOXES_ALONG_PATH", "NONE")
MAX_DIM, MAX_BOXES = 128, 16
EDGE_EPS = 1e-4          # index units, as BOXES of the terrain generator
NUDGE = 1e-2             # cells
MASK_CAP = 0.01
BOUND_TIE = 1e-3         # cells: a slice bound, or the cell under frame 0, this close to a rounding tie makes the maker drop the candidate
HINGE, SPHERICAL = 1, 2
POS_TOL = (1e-5, 2.4e-7)  # |d| <= 1e-5 + 2.4e-7 |p|max: the row rule of tests/test_hip_parity.py
QUAT_TOL = 1e-5


# ---- torch_util.py in numpy fp32 ----------------------------------------------------------------------------------------------------
def _f(x):
    return np.asarray(x, F)


def normalize(v):
    n = np.sqrt(np.sum(v * v, axis=-1, dtype=F)).astype(F)
    return (v / np.maximum(n, F(1e-9))[..., None]).astype(F)


def quat_multiply(a, b):   # :608-625, the written-out product
    x1, y1, z1, w1 = (a[..., k] for k in range(4))
    x2, y2, z2, w2 = (b[..., k] for k in range(4))
    return np.stack([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2,
                     w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2, w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2], axis=-1).astype(F)


def axis_angle_to_quat(axis, angle):   # :337-342
    theta = (_f(angle) / F(2))[..., None]
    return normalize(np.concatenate([normalize(_f(axis)) * np.sin(theta), np.cos(theta)], axis=-1).astype(F))


def quat_to_axis_angle(q):   # :70-91
    q = _f(q)
    z = (q[..., 3:] < 0).astype(F)
    q = ((F(1) - F(2) * z) * q).astype(F)
    v = q[..., :3]
    length = np.sqrt(v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2]).astype(F)
    angle = (F(2) * np.arctan2(length, q[..., 3])).astype(F)
    axis = (v / np.maximum(length, F(1e-6))[..., None]).astype(F)
    mask = length > F(1e-5)
    default = np.zeros_like(axis); default[..., 2] = 1
    return np.where(mask[..., None], axis, default).astype(F), np.where(mask, angle, F(0)).astype(F)


def quat_to_exp_map(q):
    axis, angle = quat_to_axis_angle(q)
    return (angle[..., None] * axis).astype(F)


def exp_map_to_quat(e):   # :426-450
    e = _f(e)
    with np.errstate(all="ignore"):
        angle = np.sqrt(e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1] + e[..., 2] * e[..., 2]).astype(F)
        axis = (e / angle[..., None]).astype(F)
        angle = np.arctan2(np.sin(angle), np.cos(angle)).astype(F)
    mask = np.abs(angle) > F(1e-5)
    default = np.zeros_like(e); default[..., 2] = 1
    return axis_angle_to_quat(np.where(mask[..., None], axis, default).astype(F), np.where(mask, angle, F(0)).astype(F))


def quat_close(a, b, tol=QUAT_TOL):
    """Largest component difference of two quaternion arrays up to sign."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.minimum(np.abs(a - b).max(axis=-1), np.abs(a + b).max(axis=-1))


# ---- the mirror ---------------------------------------------------------------------------------------------------------------------
def swap_tables(char_model):
    """(joint_swap [B], contact_swap [B]) of a ``parc_amd.char_model.CharModel``: the ``left_`` / ``right_`` partner of every joint
    (by joint name) and of every contact body's column (by contact body name), itself for the rest."""
    def mirror_name(name):
        if name.startswith("left_"):
            return "right_" + name[5:]
        if name.startswith("right_"):
            return "left_" + name[6:]
        return None

    B = char_model.get_num_bodies()
    jswap, cswap = np.arange(B, dtype=np.int32), np.arange(B, dtype=np.int32)
    jn = {char_model.get_joint(j).name: j for j in range(1, B)}
    for name, j in jn.items():
        m = mirror_name(name)
        if m is not None:
            assert m in jn, f"Missing symmetric counterpart for {name}"
            jswap[j] = jn[m]
    cn = {n: int(i) for n, i in zip(char_model._contact_body_names, char_model.get_contact_body_ids())}
    for name, b in cn.items():
        m = mirror_name(name)
        if m is not None:
            assert m in cn, f"Missing symmetric counterpart for {name}"
            cswap[b] = cn[m]
    return jswap, cswap


def model_tables(char_model):
    jswap, cswap = swap_tables(char_model)
    return dict(jtype=np.asarray(char_model.joint_type_array(), np.int32), axis=np.asarray(char_model.joint_axis_array(), F)[:, :3],
                jswap=jswap, cswap=cswap)


def mirror_frames(root_pos, root_rot, joint_rot, contacts, model):
    """flip_motion_about_XZ_plane (motion_edit_lib.py:343-428) on quaternion frames."""
    root_pos, root_rot, joint_rot, contacts = _f(root_pos).copy(), _f(root_rot), _f(joint_rot), _f(contacts)
    root_pos[:, 1] = root_pos[:, 1] * F(-1)
    e = quat_to_exp_map(root_rot)
    e = np.stack([e[:, 0] * F(-1), (e[:, 1] * F(-1)) * F(-1), e[:, 2] * F(-1)], axis=-1).astype(F)
    out_rot = exp_map_to_quat(e)
    out_j = np.zeros_like(joint_rot)
    B = joint_rot.shape[1] + 1
    for j in range(1, B):
        p = int(model["jswap"][j])
        q = joint_rot[:, p - 1] * np.array([1, -1, 1, -1], F)
        t = int(model["jtype"][p])
        if t == HINGE:
            axis, angle = quat_to_axis_angle(q)
            dot = model["axis"][p][0] * axis[:, 0] + model["axis"][p][1] * axis[:, 1] + model["axis"][p][2] * axis[:, 2]
            angle = np.where(dot < 0, angle * F(-1), angle).astype(F)
            out_j[:, j - 1] = axis_angle_to_quat(np.broadcast_to(model["axis"][j], axis.shape), angle)
        elif t == SPHERICAL:
            out_j[:, j - 1] = exp_map_to_quat(quat_to_exp_map(q))
        else:
            out_j[:, j - 1] = np.array([0, 0, 0, 1], F)
    return root_pos, out_rot, out_j, contacts[:, model["cswap"]].copy()


# ---- the terrain --------------------------------------------------------------------------------------------------------------------
def padded_terrain(clip, pad):
    """SubTerrain.pad (terrain_util.py:236-253): (hf, hf_maxmin or None, min_point) of the padded terrain."""
    hf, mm, dx = _f(clip["hf"]), clip.get("hf_maxmin"), F(clip["dx"])
    mp = _f(clip["min_point"])
    if pad == 0:
        return hf, (None if mm is None else _f(mm)), mp
    php = np.pad(hf, pad, constant_values=F(0))
    pmm = None
    if mm is not None:
        mm = _f(mm)
        pmm = np.stack([np.pad(mm[..., 0], pad, constant_values=mm[..., 0].max()), np.pad(mm[..., 1], pad, constant_values=mm[..., 1].min())], axis=-1)
    return php, pmm, (mp - dx * F(pad)).astype(F)


def _cells(p, mn, dx):
    return ((p - mn) / dx).astype(F)


def _tie(c):
    """Distance of cell coordinates to the nearest rounding tie."""
    return np.abs(np.abs(c - np.floor(c)) - F(0.5))


def grid_index(p, mn, dx, dim):
    with np.errstate(all="ignore"):
        r = np.rint(_cells(_f(p), mn, dx))
    return np.clip(np.nan_to_num(r, nan=0.0, posinf=dim - 1, neginf=0), 0, dim - 1).astype(np.int64)


def arange_points(start, end, step):
    """torch.arange on 0-dim fp32 tensors: ceil((end - start) / step) points in double, point i = start + i * step in double, as fp32."""
    n = int(np.ceil((np.float64(end) - np.float64(start)) / np.float64(step)))
    return (np.float64(start) + np.arange(n, dtype=np.float64) * np.float64(step)).astype(F), n


def slice_bounds(x, y, pmin, dx):
    """(min_g [2], max_g [2], info) of slice_terrain_around_motion :1592-1601 with padding = 2 dx."""
    pad = dx * F(2)
    mn = np.array([x.min(), y.min()], F) - pad
    mx = np.array([x.max(), y.max()], F) + pad
    cmn, cmx = _cells(mn, pmin, dx), _cells(mx, pmin, dx)
    min_g = (np.rint(cmn) * dx + pmin).astype(F)
    max_g = (np.rint(cmx) * dx + pmin).astype(F)
    ratio = (np.float64(max_g + dx) - np.float64(min_g)) / np.float64(dx)
    info = dict(bound_tie=float(min(_tie(cmn).min(), _tie(cmx).min())), count_tie=float(np.abs(ratio - np.rint(ratio)).min()))
    return min_g, max_g, info


def augment_one(clip, var, mode, pad, slice_terrain, model=None):
    """One variation: a dict of the outputs, ``unstable [X, Y]`` and ``info`` (the tie distances the fixture maker screens with)."""
    assert mode in MODES
    s, nf = int(var["start"]), int(var["nf"])
    dx = F(clip["dx"])
    rp = _f(clip["root_pos"])[s:s + nf]
    h = F(var["heading"])
    c, sn = np.cos(h), np.sin(h)
    x = ((rp[:, 0] * c - rp[:, 1] * sn) * F(var["sx"])).astype(F)
    y = ((rp[:, 0] * sn + rp[:, 1] * c) * F(var["sy"])).astype(F)
    hq = axis_angle_to_quat(np.array([0, 0, 1], F), h)
    rot = exp_map_to_quat(quat_to_exp_map(quat_multiply(np.broadcast_to(hq, (nf, 4)), _f(clip["root_rot"])[s:s + nf])))
    jrot, con = _f(clip["joint_rot"])[s:s + nf].copy(), _f(clip["contacts"])[s:s + nf].copy()
    php, pmm, pmin = padded_terrain(clip, pad)
    PX, PY = php.shape
    info = dict(bound_tie=1.0, count_tie=1.0, lookup_tie=1.0)
    if slice_terrain:
        min_g, max_g, b = slice_bounds(x, y, pmin, dx)
        info.update(b)
        xs, X = arange_points(min_g[0], max_g[0] + dx, dx)
        ys, Y = arange_points(min_g[1], max_g[1] + dx, dx)
        canon = np.array([x[0], y[0]], F)
        lmin = (min_g - canon).astype(F)
        ci, cj = _cells(xs, pmin[0], dx), _cells(ys, pmin[1], dx)
        ii, jj = grid_index(xs, pmin[0], dx, PX), grid_index(ys, pmin[1], dx, PY)
        near = (_tie(ci) < F(NUDGE))[:, None] | (_tie(cj) < F(NUDGE))[None, :]
        hf = php[ii[:, None], jj[None, :]].copy()
        mm = None if pmm is None else pmm[ii[:, None], jj[None, :]].copy()
        c0 = _cells(np.zeros(2, F), lmin, dx)                      # get_hf_val_from_points(localised frame 0) on the slice
        i0, j0 = int(grid_index(F(0), lmin[0], dx, X)), int(grid_index(F(0), lmin[1], dx, Y))
        cz = hf[i0, j0]
        if _tie(c0).min() < F(BOUND_TIE) or near[i0, j0]:          # canon_z itself hinges on a tie: every height does
            near[:] = True
        info["bound_tie"] = float(min(info["bound_tie"], _tie(c0).min()))
        info["lookup_tie"] = float(min(_tie(ci).min(), _tie(cj).min()))
    else:
        X, Y, hf, mm = PX, PY, php.copy(), (None if pmm is None else pmm.copy())
        canon, lmin, cz = np.zeros(2, F), pmin.copy(), F(0)
        near = np.zeros((X, Y), bool)
    px, py, pz = (x - canon[0]).astype(F), (y - canon[1]).astype(F), (rp[:, 2] - cz).astype(F)
    hf = (hf - cz).astype(F)
    unstable = near
    if mode == "HEIGHT_SCALE":
        hf = (F(var["hscale"]) * hf).astype(F)
    elif mode == "BOXES_ALONG_PATH":
        gx, gy = np.arange(X, dtype=F)[:, None], np.arange(Y, dtype=F)[None, :]
        for b in range(int(var["nb"])):
            fr = int(var["box_frame"][b])
            lx, ly, ang, bh = (F(v) for v in var["boxes"][b])
            bx, by = (px[fr] - lmin[0]) / dx, (py[fr] - lmin[1]) / dx
            inside, edge = _box_test(gx, gy, bx, by, np.cos(ang), np.sin(ang), lx / F(2), ly / F(2), EDGE_EPS)
            hf = np.where(inside, bh, hf).astype(F)
            unstable = unstable | edge
    root_pos = np.stack([px, py, pz], axis=-1).astype(F)
    min_point = lmin.copy()
    if int(var["mirror"]):
        assert model is not None, "the mirror needs the model tables"
        root_pos, rot, jrot, con = mirror_frames(root_pos, rot, jrot, con, model)
        hf, unstable = hf[:, ::-1].copy(), unstable[:, ::-1].copy()
        mm = None if mm is None else mm[:, ::-1].copy()
        min_point[1] = F(-1.0) * ((lmin[1] + F(Y) * dx) - dx)     # flip_by_XZ_axis
    return dict(root_pos=root_pos, root_rot=rot, joint_rot=jrot, contacts=con, hf=hf, hf_maxmin=mm, hf_dims=np.array([X, Y], np.int32),
                min_point=min_point, dx=dx, canon_z=F(cz), unstable=unstable, info=info)


def compare_hf(got, want, unstable, what=""):
    """terrain_gen_ref.compare's rule: outside the mask bit for bit; returns how many masked cells differed."""
    got, want = np.asarray(got, F), np.asarray(want, F)
    assert got.shape == want.shape == unstable.shape[:got.ndim], (got.shape, want.shape, unstable.shape)
    diff = got.view(np.uint32) != want.view(np.uint32)
    diff &= ~(np.isnan(got) & np.isnan(want))
    assert not (diff & ~unstable).any(), f"{what}: cells outside the mask differ at {np.argwhere(diff & ~unstable)[:5].tolist()}"
    return int((diff & unstable).sum())


def pos_close(got, want):
    """The row rule: |d| <= 1e-5 + 2.4e-7 |p|max over the compared block."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    tol = POS_TOL[0] + POS_TOL[1] * (np.abs(want).max() if want.size else 0.0)
    return float(np.abs(got - want).max() if want.size else 0.0), tol


def compare_variation(got, want, what=""):
    """The rules of the issue for one variation: ``got`` / ``want`` are dicts as ``augment_one`` returns (``want`` carries ``unstable``)."""
    assert tuple(got["hf_dims"]) == tuple(want["hf_dims"]), (what, got["hf_dims"], want["hf_dims"])
    assert got["root_pos"].shape == want["root_pos"].shape, (what, got["root_pos"].shape, want["root_pos"].shape)
    assert np.array_equal(got["contacts"], want["contacts"]), what
    masked = compare_hf(got["hf"], want["hf"], want["unstable"], what + " hf")
    if want.get("hf_maxmin") is not None:
        for k in range(2):
            masked += compare_hf(got["hf_maxmin"][..., k], want["hf_maxmin"][..., k], want["unstable"], what + " hf_maxmin")
    for key in ("min_point", "root_pos"):
        err, tol = pos_close(got[key], want[key])
        assert err <= tol, (what, key, err, tol)
    for key in ("root_rot", "joint_rot"):
        err = float(quat_close(got[key], want[key]).max())
        assert err <= QUAT_TOL, (what, key, err)
    return masked


# ---- the fixture --------------------------------------------------------------------------------------------------------------------
PLAN_KEYS = ("src_clip", "start_frame", "num_frames", "heading", "scale", "mirror", "height_scale", "num_boxes", "box_frame", "boxes")
SRC_KEYS = ("root_pos", "root_rot", "joint_rot", "contacts", "hf", "hf_maxmin", "min_point", "dx")


def plan_var(plan, v):
    """Variation ``v`` of a plan of host arrays, as ``augment_one`` takes it."""
    return dict(start=int(plan["start_frame"][v]), nf=int(plan["num_frames"][v]), heading=F(plan["heading"][v]), sx=F(plan["scale"][v][0]),
                sy=F(plan["scale"][v][1]), mirror=int(plan["mirror"][v]), hscale=F(plan["height_scale"][v]), nb=int(plan["num_boxes"][v]),
                box_frame=np.asarray(plan["box_frame"][v]), boxes=np.asarray(plan["boxes"][v], F))


def load_fixture(path):
    """``(sources, groups, settings, notes)`` of ``motion_aug.npz``: a group is a dict ``mode``, ``mirror``, ``plan`` (host arrays) and
    ``want`` (per variation, the reference's outputs with the restatement's ``unstable`` mask)."""
    import json
    z = np.load(path)
    sources = []
    while f"src{len(sources)}_hf" in z.files:
        k = len(sources)
        sources.append({n: z[f"src{k}_{n}"] for n in SRC_KEYS})
    groups = []
    for g, meta in enumerate(json.loads(str(z["groups"]))):
        plan = {n: z[f"g{g}_plan_{n}"] for n in PLAN_KEYS}
        want = []
        for v in range(meta["variations"]):
            src, s, nf = sources[int(plan["src_clip"][v])], int(plan["start_frame"][v]), int(plan["num_frames"][v])
            w = {n: z[f"g{g}_v{v}_{n}"] for n in ("root_pos", "root_rot", "contacts", "hf", "hf_maxmin", "unstable")}
            w["joint_rot"] = z[f"g{g}_v{v}_joint_rot"] if meta["mirror"] else src["joint_rot"][s:s + nf]
            geom = z[f"g{g}_v{v}_geom"]
            w["min_point"], w["canon_z"], w["hf_dims"] = geom[:2], geom[2], np.array(w["hf"].shape, np.int32)
            want.append(w)
        groups.append(dict(meta, plan=plan, want=want))
    return sources, groups, json.loads(str(z["settings"])), json.loads(str(z["notes"]))
