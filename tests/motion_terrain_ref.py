"""An independent numpy restatement of the motion-terrain analysis (the reference's ``compute_hf_extra_vals``,
``compute_motion_loss`` with unit weights and the jerk statistics of ``compute_losses.py``).

Written from the semantics table of DESIGN.md section 8e: fp32 FK with the factored (Shoemake) quaternion product, the cell of a
point = round half to even of a true fp32 division, clamped; the lowest point per cell; ``hf_maxmin`` in the reference's order; the
exact column-box SDF of the whole terrain, by brute force and by the ring-pruned search.  ``tests/test_motion_terrain_cpu.py``
checks it against the reference fixtures; it is the CPU-side statement of what the HIP kernels (``parc_motion_terrain.hpp``) compute.
"""
import numpy as np

F32 = np.float32
MISSING = F32(99999.9999)


def qmul(a, b):  # the factored product of torch_util.quat_mul
    x1, y1, z1, w1 = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    x2, y2, z2, w2 = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    ww = (z1 + x1) * (x2 + y2)
    yy = (w1 - y1) * (w2 + z2)
    zz = (w1 + y1) * (w2 - z2)
    xx = ww + yy + zz
    qq = F32(0.5) * (xx + (z1 - x1) * (x2 - y2))
    w = qq - ww + (z1 - y1) * (y2 - z2)
    x = qq - xx + (x1 + w1) * (x2 + w2)
    y = qq - yy + (w1 - x1) * (y2 + z2)
    z = qq - zz + (z1 + y1) * (w2 - x2)
    return np.stack([x, y, z, w], -1).astype(F32)


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1).astype(F32)


def qrot(q, v):
    t = F32(2) * cross(q[..., :3], v)
    return (v + q[..., 3:] * t + cross(q[..., :3], t)).astype(F32)


def fk(cm, root_pos, root_rot, joint_rot):
    """[F, B, 3], [F, B, 4] in fp32."""
    B = cm.get_num_bodies()
    pos, rot = [root_pos.astype(F32)], [root_rot.astype(F32)]
    lt = np.asarray(cm._local_translation, F32)
    lr = np.asarray(cm._local_rotation, F32)
    for j in range(1, B):
        p = int(cm._parent_indices[j])
        pos.append((pos[p] + qrot(rot[p], np.broadcast_to(lt[j], pos[p].shape))).astype(F32))
        rot.append(qmul(rot[p], qmul(np.broadcast_to(lr[j], rot[p].shape), joint_rot[:, j - 1].astype(F32))))
    return np.stack(pos, 1), np.stack(rot, 1)


def world_points(pos, rot, points, point_body):
    """[F, P, 3]: quat_rotate(body rot, local point) + body pos."""
    return (qrot(rot[:, point_body], np.broadcast_to(points, (pos.shape[0],) + points.shape)) + pos[:, point_body]).astype(F32)


def grid_index(xy, min_point, dx, dims):
    i = np.rint((xy.astype(F32) - min_point.astype(F32)) / F32(dx)).astype(np.int64)
    return np.clip(i, 0, np.asarray(dims) - 1)


def hf_extra_vals(world, root_pos, hf, min_point, dx, z_buf=3.0, jump_buf=0.8):
    """(per-frame unique cells int64 [K, 2], lowest point per cell, hf_maxmin [X, Y, 2])."""
    X, Y = hf.shape
    inds, mbh = [], np.full(hf.shape, MISSING, F32)
    for f in range(world.shape[0]):
        g = grid_index(world[f, :, :2], min_point, dx, (X, Y))
        np.minimum.at(mbh, (g[:, 0], g[:, 1]), world[f, :, 2])
        inds.append(np.unique(g, axis=0))
    mask = np.zeros(hf.shape, bool)
    for g in inds:
        mask[g[:, 0], g[:, 1]] = True
    max_h, min_h = float(np.max(root_pos[:, 2])), float(np.min(hf))
    mm = np.empty(hf.shape + (2,), F32)
    mm[..., 0] = F32(max_h + z_buf)
    mm[..., 1] = F32(min_h - z_buf)
    mm[mask, 0] = hf[mask]
    mm[mask, 1] = hf[mask]
    jump = ((mbh - hf) >= F32(jump_buf)) & mask
    mm[jump, 0] = mbh[jump] - F32(jump_buf)
    mm[jump, 1] = F32(min_h - z_buf)
    return inds, mbh, mm


def centres(n, d, mn):
    """torch.linspace(0, (n - 1) d, n) + mn on the CPU (step * i below the middle, a fused end - step * (n - 1 - i) above)."""
    end = F32((n - 1) * float(d))
    step = F32(end / F32(n - 1)) if n > 1 else F32(0)
    i = np.arange(n)
    lo = (step * i.astype(F32)).astype(F32)
    hi = (np.float64(end) - np.float64(step) * (n - 1 - i)).astype(F32)
    return (np.where(i < n // 2, lo, hi).astype(F32) + F32(mn)).astype(F32)


def sd_box(p, h):
    q = (np.abs(p) - h).astype(F32)
    out = np.sqrt(np.sum(np.maximum(q, F32(0)) ** 2, -1, dtype=F32)).astype(F32)
    return (out + np.minimum(np.max(q, -1), F32(0))).astype(F32)


def _cell_sdfs(pts, cx, cy, h, dx, base_z):
    """ground / air SDF [N, M] of points [N, 3] to cells with centres cx, cy [M] and heights h [M]."""
    top = F32(-base_z)
    half = np.array([dx / F32(2), dx / F32(2)], F32)
    rel_xy = np.stack([pts[:, None, 0] - cx[None], pts[:, None, 1] - cy[None]], -1).astype(F32)
    gz = (pts[:, None, 2] - (h + base_z)[None] / F32(2)).astype(F32)
    az = (pts[:, None, 2] - (h + top)[None] / F32(2)).astype(F32)
    hg = np.broadcast_to(np.concatenate([np.broadcast_to(half, h.shape + (2,)), ((h - base_z) / F32(2))[:, None]], -1), rel_xy.shape[:2] + (3,))
    ha = np.broadcast_to(np.concatenate([np.broadcast_to(half, h.shape + (2,)), ((top - h) / F32(2))[:, None]], -1), rel_xy.shape[:2] + (3,))
    g = sd_box(np.concatenate([rel_xy, gz[..., None]], -1), hg)
    a = sd_box(np.concatenate([rel_xy, az[..., None]], -1), ha)
    return g, a


def base_z_of(hf):
    return F32(float(np.min(hf)) - 10.0)


def sdf_brute(pts, hf, min_point, dx, chunk=256):
    """Exact (ground, air) SDF minima of points [N, 3] over every cell."""
    X, Y = hf.shape
    cx, cy = centres(X, dx, min_point[0]), centres(Y, dx, min_point[1])
    CX, CY = np.meshgrid(cx, cy, indexing="ij")
    bz = base_z_of(hf)
    g, a = np.empty(len(pts), F32), np.empty(len(pts), F32)
    for s in range(0, len(pts), chunk):
        gg, aa = _cell_sdfs(pts[s:s + chunk], CX.reshape(-1), CY.reshape(-1), hf.reshape(-1).astype(F32), F32(dx), bz)
        g[s:s + chunk], a[s:s + chunk] = gg.min(1), aa.min(1)
    return g, a


def sdf_pruned(pts, hf, min_point, dx):
    """The same minima by the Chebyshev-ring search of DESIGN.md section 8e, one point at a time."""
    X, Y = hf.shape
    cx, cy = centres(X, dx, min_point[0]), centres(Y, dx, min_point[1])
    bz, dx = base_z_of(hf), F32(dx)
    g_out, a_out = np.empty(len(pts), F32), np.empty(len(pts), F32)
    for n, p in enumerate(pts):
        ci, cj = grid_index(p[None, :2], min_point, dx, (X, Y))[0]
        ex, ey = abs(p[0] - cx[ci]), abs(p[1] - cy[cj])
        margin0 = F32(1e-5) * (F32(1) + abs(p[0]) + abs(p[1]) + abs(min_point[0]) + abs(min_point[1]))
        bg = ba = F32(np.inf)
        need_g = need_a = True
        for r in range(max(ci, X - 1 - ci, cj, Y - 1 - cj) + 1):
            if r > 0:
                lb = min(F32(r) * dx - ex - dx / F32(2), F32(r) * dx - ey - dx / F32(2)) - (margin0 + F32(1e-5) * (F32(r) * dx))
                need_g = need_g and not lb > max(bg, F32(0))
                need_a = need_a and not lb > max(ba, F32(0))
                if not (need_g or need_a):
                    break
            cells = [(i, j) for i in range(ci - r, ci + r + 1) for j in range(cj - r, cj + r + 1)
                     if max(abs(i - ci), abs(j - cj)) == r and 0 <= i < X and 0 <= j < Y]
            if not cells:
                continue
            c = np.array(cells)
            gg, aa = _cell_sdfs(p[None].astype(F32), cx[c[:, 0]], cy[c[:, 1]], hf[c[:, 0], c[:, 1]].astype(F32), dx, bz)
            if need_g:
                bg = min(bg, gg.min())
            if need_a:
                ba = min(ba, aa.min())
        g_out[n], a_out[n] = bg, ba
    return g_out, a_out


def scores(world, contacts, point_body, hf, min_point, dx):
    """(pen_loss, contact_loss) of compute_motion_loss with unit weights; every body scored with its own contact column."""
    Fn, P, _ = world.shape
    g, a = sdf_brute(world.reshape(-1, 3), hf, min_point, dx)
    g, a = g.reshape(Fn, P), a.reshape(Fn, P)
    pen = float(np.sum(np.maximum(a, F32(0)), dtype=np.float64))
    con = 0.0
    for b in np.unique(point_body):
        best = np.maximum(g[:, point_body == b], F32(0)).min(1)
        con += float(np.sum(best.astype(np.float64) * contacts[:, b]))
    return pen, con


def jerk_stats(body_pos, max_jerk=11666.3906):
    """(mean_jerk, jerk_frac): fp32 finite differences with dt = 1/30; the count above max_jerk divided by frames - 3."""
    if body_pos.shape[0] < 4:
        return float("nan"), float("nan")
    dt = F32(1.0 / 30.0)
    v = (body_pos[1:] - body_pos[:-1]) / dt
    a = (v[1:] - v[:-1]) / dt
    j = (a[1:] - a[:-1]) / dt
    m = np.sqrt(np.sum(j * j, -1, dtype=F32)).astype(F32)
    return float(np.mean(m, dtype=np.float64)), float(np.count_nonzero(m > F32(max_jerk)) / m.shape[0])
