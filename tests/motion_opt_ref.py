"""An independent torch restatement of the kinematic motion optimiser's loss (the reference's
``motion_terrain_contact_loss_localized``) and of the constraint-point refinement of ``compute_approx_body_constraints``.

Written from the semantics table of DESIGN.md section 8d, not from the reference's code: textbook quaternion algebra, autograd for the
gradient.  ``tests/test_motion_opt_cpu.py`` checks it against the reference fixtures; it is the CPU-side statement of what the HIP kernels
(``parc_motion_opt.hpp``) compute, and a second derivation of the gradients they produce analytically.

Everything is computed in the dtype of ``params`` (``Character`` and ``as_tensors`` take it as an argument; the other inputs are given in
it): float32 as the reference computes, float64 as the yardstick of ``tests/test_motion_opt_terms_*.py``.
"""
import numpy as np
import torch

from parc_amd.char_model import GeomType, JointType

MASK_EPS = 1e-5
HUBER_C, HUBER_C2 = 0.03, 0.0009
JERK_DT = 1.0 / 30.0


def qmul(a, b):
    ax, ay, az, aw = a.unbind(-1)
    bx, by, bz, bw = b.unbind(-1)
    return torch.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                        aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz], -1)


def qconj(q):
    return torch.cat([-q[..., :3], q[..., 3:]], -1)


def qrot(q, v):
    u, w = q[..., :3], q[..., 3:]
    t = 2.0 * torch.linalg.cross(u, v.expand_as(u), dim=-1)
    return v + w * t + torch.linalg.cross(u, t, dim=-1)


def rotation_angle(q):
    """Angle of q after flipping it to w >= 0; 0 (and a zero gradient) where |xyz| <= 1e-5."""
    q = torch.where(q[..., 3:] < 0, -q, q)
    n = torch.linalg.vector_norm(q[..., :3], dim=-1)
    return torch.where(n > MASK_EPS, 2.0 * torch.atan2(n, q[..., 3]), torch.zeros_like(n))


def diff_angle(q0, q1):
    return rotation_angle(qmul(q1, qconj(q0)))


def exp_map_to_quat(e):
    """(sin(th/2) e/|e|, cos(th/2)) with th = |e| wrapped to (-pi, pi]; the identity where |th| <= 1e-5."""
    th0 = torch.linalg.vector_norm(e, dim=-1, keepdim=True)
    th = torch.atan2(torch.sin(th0), torch.cos(th0))
    ok = th.abs() > MASK_EPS
    axis = torch.where(ok, e / torch.where(ok, th0, torch.ones_like(th0)), torch.zeros_like(e))
    half = torch.where(ok, th, torch.zeros_like(th)) * 0.5
    return torch.cat([axis * torch.sin(half), torch.cos(half)], -1)


def hinge_quat(axis, d):
    axis = axis.to(d.dtype)
    half = 0.5 * d.unsqueeze(-1)
    return torch.cat([axis / axis.norm() * torch.sin(half), torch.cos(half)], -1)


class Character:
    def __init__(self, cm, dtype=torch.float32):
        self.cm = cm
        self.B = cm.get_num_bodies()
        self.parent = [int(p) for p in cm._parent_indices]
        self.lt = torch.tensor(cm._local_translation, dtype=dtype)
        self.lr = torch.tensor(cm._local_rotation, dtype=dtype)

    def dof_to_rot(self, dof):
        out = []
        for j in range(1, self.B):
            jt = self.cm._joints[j]
            if jt.joint_type == JointType.HINGE:
                out.append(hinge_quat(torch.tensor(jt.axis, dtype=dof.dtype), dof[..., jt.dof_idx]))
            elif jt.joint_type == JointType.SPHERICAL:
                out.append(exp_map_to_quat(dof[..., jt.dof_idx:jt.dof_idx + 3]))
            else:
                out.append(torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=dof.dtype).expand(dof.shape[:-1] + (4,)))
        return torch.stack(out, -2)

    def fk(self, root_pos, root_rot, joint_rot):
        pos, rot = [root_pos], [root_rot]
        for j in range(1, self.B):
            p = self.parent[j]
            pos.append(pos[p] + qrot(rot[p], self.lt[j]))
            rot.append(qmul(rot[p], qmul(self.lr[j].expand_as(joint_rot[..., j - 1, :]), joint_rot[..., j - 1, :])))
        return torch.stack(pos, -2), torch.stack(rot, -2)


def box_sdf(p, h):
    q = p.abs() - h
    return torch.linalg.vector_norm(q.clamp(min=0.0), dim=-1) + q.max(dim=-1).values.clamp(max=0.0)


def column_sdf(x, hf, x0, y0, min_point, dx, bottom, top):
    """Min over the cells [x0, x0+sx) x [y0, y0+sy) of the box SDF of the columns [bottom, hf] (top is None) or [hf, top]."""
    sx, sy = hf.shape
    i = torch.arange(sx, dtype=x.dtype)
    j = torch.arange(sy, dtype=x.dtype)
    cx = (min_point[0] + x0 * dx) + i * dx
    cy = (min_point[1] + y0 * dx) + j * dx
    lo, hi = (torch.full_like(hf, bottom), hf) if top is None else (hf, torch.full_like(hf, top))
    c = torch.stack([cx[:, None].expand(sx, sy), cy[None, :].expand(sx, sy), (lo + hi) / 2], -1).reshape(-1, 3)
    h = torch.stack([torch.full_like(hf, dx / 2), torch.full_like(hf, dx / 2), (hi - lo) / 2], -1).reshape(-1, 3)
    return box_sdf(x[..., None, :] - c, h).min(dim=-1).values


def patch_start(xy, dims, min_point, dx):
    """Per frame: the cell box of the points' xy +- 2 cells (floor / ceil, clamped); one patch size for the clip (the largest)."""
    lo = torch.floor((xy.min(dim=1).values - 2 * dx - min_point) / dx).long().clamp(min=0)
    hi = torch.minimum(torch.ceil((xy.max(dim=1).values + 2 * dx - min_point) / dx).long(), dims - 1)
    size = torch.minimum((hi - lo + 1).max(dim=0).values.clamp(min=1), dims)
    start = torch.minimum(lo, dims - size).clamp(min=0)
    return start, size


def loss_terms(ch, params, src, pts, pt_body, contacts, contact_id, hf, min_point, dx, cons, w, max_jerk):
    """The nine terms (LossType order) and the weighted total.  params: root_pos [F,3] | root exp map [F,3] | dofs [F,D]."""
    F, B = params.shape[0], ch.B
    rp, re, dof = params[:, :3], params[:, 3:6], params[:, 6:]
    rq, jr = exp_map_to_quat(re), ch.dof_to_rot(dof)
    pos, rot = ch.fk(rp, rq, jr)
    spos, srot = ch.fk(src["root_pos"], src["root_rot"], src["joint_rot"])
    t = [None] * 9
    t[0] = ((rp - src["root_pos"]) ** 2).sum()
    t[1] = (diff_angle(rq, src["root_rot"]) ** 2).sum()
    t[2] = (diff_angle(jr, src["joint_rot"]) ** 2).sum()
    vel_err = (pos[1:] - pos[:-1]) - (spos[1:] - spos[:-1])
    rot_err = diff_angle(rot[1:], rot[:-1]) - diff_angle(srot[1:], srot[:-1])
    vsq, rsq = (vel_err ** 2).sum(-1), rot_err ** 2
    t[3] = vsq.sum() + rsq.sum()
    # points, patch, penetration (air columns up to +10 m) and contact (ground columns down to -10 m)
    x = qrot(rot[:, pt_body], pts) + pos[:, pt_body]
    start, size = patch_start(x[..., :2].detach(), torch.tensor(hf.shape), min_point, dx)
    air, ground = [], []
    for f in range(F):
        sub = hf[start[f, 0]:start[f, 0] + size[0], start[f, 1]:start[f, 1] + size[1]]
        air.append(column_sdf(x[f], sub, start[f, 0], start[f, 1], min_point, dx, None, 10.0))
        ground.append(column_sdf(x[f], sub, start[f, 0], start[f, 1], min_point, dx, -10.0, None))
    air, ground = torch.stack(air), torch.stack(ground)
    t[4] = air.clamp(min=0.0).sum()
    zero = torch.zeros((), dtype=params.dtype)
    t[5] = zero
    if w[5] != 0.0:
        g = ground.clamp(min=0.0)
        for b in range(B):
            if contact_id[b] >= 0:
                t[5] = t[5] + (g[:, pt_body == b].min(dim=1).values * contacts[:, contact_id[b]]).sum()
    # body constraints: hands (sphere geom) |dist to centre - r|, feet (box) the first 18 points, clamp(dist - 1.25 |half|, 0)
    t[7] = zero
    keep = torch.ones(F - 1, B, dtype=params.dtype)
    for b, s, e, cp in cons:
        g = ch.cm._geoms[b][0]
        fr = slice(s, e + 1)
        if g.shape == GeomType.SPHERE:
            ctr = qrot(rot[fr, b], torch.tensor(g.pos, dtype=params.dtype)) + pos[fr, b]
            t[7] = t[7] + (torch.linalg.vector_norm(cp - ctr, dim=-1) - float(g.size[0])).abs().sum()
        elif g.shape == GeomType.BOX:
            r = torch.linalg.vector_norm(torch.tensor(g.size, dtype=params.dtype)) * 1.25
            sole = x[fr][:, pt_body == b][:, :18].reshape(-1, 3)
            t[7] = t[7] + (torch.linalg.vector_norm(cp - sole, dim=-1) - r).clamp(min=0.0).sum()
        else:
            continue
        keep[s:e + 1, b] = 0.0
    t[6] = zero
    if w[6] != 0.0:
        both = torch.minimum(contacts[1:], contacts[:-1]).clamp(min=0.0)
        t[6] = ((torch.sqrt(vsq * keep + HUBER_C2) - HUBER_C) * both).sum() + ((torch.sqrt(rsq * keep + HUBER_C2) - HUBER_C) * both).sum()
    v = pos[1:] - pos[:-1]
    a = v[1:] - v[:-1]
    jerk = a[1:] - a[:-1]
    t[8] = (torch.linalg.vector_norm(jerk, dim=-1) - max_jerk * JERK_DT ** 3).clamp(min=0.0).sum()
    total = sum(wi * ti for wi, ti in zip(w, t))
    return t, total


def refine_constraint_point(p, hf, min_point, dx, steps=1000, lr=0.01):
    """SGD on sdf^2 against the ground columns of the whole terrain, bottom at min(hf) - 10."""
    p = p.clone().requires_grad_(True)
    bottom = float(hf.min()) - 10.0
    for _ in range(steps):
        sd = column_sdf(p[None], hf, 0, 0, min_point, dx, bottom, None)
        (g,) = torch.autograd.grad((sd ** 2).sum(), p)
        with torch.no_grad():
            p -= lr * g
    return p.detach()


def as_tensors(z, dtype=None):
    return {k: torch.tensor(np.asarray(z[k]), dtype=dtype) for k in ("root_pos", "root_rot", "joint_rot")}
