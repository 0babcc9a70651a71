"""Torch restatement of the motion generator's training loss (the reference's ``MDM.motion_difference``, mdm.py:573-692) in the dtype of
its input, the gradient from autograd: the second derivation beside the kernel's analytic one, as ``motion_opt_ref.py`` is for the
optimiser.  float64 is the yardstick of the GPU tests; float32 on the GPU is the shape of the reference's own path (the measurement of
DESIGN.md section 8l).

``MdmLossRef(cfg, loss_fn, dtype, device, mean, std)`` has ``MotionLoss``' interface: ``terms_and_grad(pred, true_motion, target_dir)``
returns the weighted terms [N, 13] and d (sum of a window's terms) / d pred; ``terms(pred, ...)`` is the differentiable forward.
"""
import numpy as np
import torch

from parc_amd import motion_generator as mg
from parc_amd.char_model import CharModel, JointType
from parc_amd.motion_loss import TERM_NAMES, WEIGHT_KEYS, check_loss_config

NT = len(TERM_NAMES)


def quat_mul(a, b):   # torch_util.py:42-59, the factored product
    x1, y1, z1, w1 = a.unbind(-1)
    x2, y2, z2, w2 = b.unbind(-1)
    ww = (z1 + x1) * (x2 + y2)
    yy = (w1 - y1) * (w2 + z2)
    zz = (w1 + y1) * (w2 - z2)
    xx = ww + yy + zz
    qq = 0.5 * (xx + (z1 - x1) * (x2 - y2))
    return torch.stack([qq - xx + (x1 + w1) * (x2 + w2), qq - yy + (w1 - x1) * (y2 + z2), qq - zz + (z1 + y1) * (w2 - x2),
                        qq - ww + (z1 - y1) * (y2 - z2)], dim=-1)


def quat_conj(q):
    return torch.cat([-q[..., :3], q[..., 3:]], dim=-1)


def quat_rotate(q, v):
    qv = q[..., :3]
    t = 2 * torch.cross(qv, v, dim=-1)
    return v + q[..., 3:] * t + torch.cross(qv, t, dim=-1)


def quat_pos(q):
    z = (q[..., 3:] < 0).to(q.dtype)
    return (1 - 2 * z) * q


def quat_diff(q0, q1):
    return quat_mul(q1, quat_conj(q0))


def quat_diff_angle(q0, q1):   # through quat_pos, masked at |v| <= 1e-5
    q = quat_pos(quat_diff(q0, q1))
    length = torch.norm(q[..., 0:3], dim=-1, p=2)
    angle = 2.0 * torch.atan2(length, q[..., 3])
    return torch.where(length > 1e-5, angle, torch.zeros_like(angle))


def quat_to_exp_map_grad_friendly(q):   # axis = v / (|v| + 1e-5), its own mask
    q = quat_pos(q)
    length = torch.norm(q[..., 0:3], dim=-1, p=2)
    angle = 2.0 * torch.atan2(length, q[..., 3])
    axis = q[..., 0:3] / (length.unsqueeze(-1) + 1e-5)
    default = torch.zeros_like(axis)
    default[..., -1] = 1
    mask = length > 1e-5
    angle = torch.where(mask, angle, torch.zeros_like(angle))
    axis = torch.where(mask.unsqueeze(-1), axis, default)
    return angle.unsqueeze(-1) * axis


def _safe_exp_map_to_quat(e):
    """``mg.exp_map_to_quat`` with a finite backward: autograd through the reference's form is NaN at an exactly zero exp map (the axis
    is divided by a zero angle before it is masked); the kernel's gradient is 0 there, and so is this one's."""
    angle = torch.linalg.norm(e, dim=-1)
    zero = angle == 0
    e = torch.where(zero.unsqueeze(-1), torch.ones_like(e), e)
    q = mg.exp_map_to_quat(e)
    ident = torch.zeros_like(q)
    ident[..., 3] = 1
    return torch.where(zero.unsqueeze(-1), ident, q)


def pseudo_huber(x, y):   # mdm.py:103-109
    loss = (x - y) ** 2 + 0.0009
    return torch.sqrt(torch.sum(loss.reshape(loss.shape[0], -1), dim=-1)) - 0.03


def squared_l2(x, y):     # mdm.py:111-114
    loss = (x - y) ** 2
    return torch.sum(loss.reshape(loss.shape[0], -1), dim=-1)


class MdmLossRef:
    def __init__(self, cfg, loss_fn="squared_l2", dtype=torch.float64, device="cpu", mean=None, std=None):
        check_loss_config(cfg, loss_fn)
        self.cfg, self.dtype, self.device = cfg, dtype, torch.device(device)
        self.fn = {"squared_l2": squared_l2, "pseudo_huber": pseudo_huber}[loss_fn]
        self.cm = CharModel(mg._char_path(cfg))
        cm = self.cm
        self.B = cm.get_num_bodies()
        J, nd = self.B - 1, cm.get_dof_size()
        self.D = mg.frame_dim(cm)
        self.sl = {"pos": slice(0, 3), "rot": slice(3, 6), "jpos": slice(6, 6 + 3 * J), "jrot": slice(6 + 3 * J, 6 + 3 * J + nd),
                   "con": slice(6 + 3 * J + nd, self.D)}
        self.w = [float(cfg[k]) for k in WEIGHT_KEYS]
        self.dt = 1.0 / cfg["sequence_fps"]
        self.nprev = int(cfg["num_prev_states"])
        self.use_pos, self.use_target = bool(cfg.get("use_pos_loss", True)), bool(cfg.get("use_target_loss", False))
        self.eps = float(cfg.get("target_dir_len_eps", 0.1))
        t = lambda a: torch.as_tensor(np.asarray(a), dtype=dtype, device=self.device)  # noqa: E731
        self.parent = [int(p) for p in cm._parent_indices]
        self.lt = [t(cm._local_translation[j]) for j in range(self.B)]
        self.lr = [t(cm._local_rotation[j]) for j in range(self.B)]
        self.jt, self.ax, self.di = cm.joint_type_array(), cm.joint_axis_array(), cm.dof_idx_array()
        self.mean = self.std = None
        if mean is not None:
            self.set_stats(mean, std)

    def set_stats(self, mean, std):
        t = lambda a: (a.detach() if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a))).to(self.device, self.dtype)  # noqa: E731
        self.mean, self.std = t(mean), t(std)

    def fk(self, root_pos, root_q, jq):
        pos, rot = [root_pos], [root_q]
        for j in range(1, self.B):
            p = self.parent[j]
            pos.append(pos[p] + quat_rotate(rot[p], self.lt[j].expand_as(root_pos)))
            rot.append(quat_mul(rot[p], quat_mul(self.lr[j].expand_as(root_q), jq[..., j - 1, :])))
        return torch.stack(pos, dim=-2), torch.stack(rot, dim=-2)

    def dof_to_rot(self, dof):
        out = []
        for j in range(1, self.B):
            if self.jt[j] == JointType.HINGE:
                a = torch.as_tensor(self.ax[j], dtype=dof.dtype, device=dof.device).expand(dof.shape[:-1] + (3,))
                out.append(mg._axis_angle_to_quat(a, dof[..., self.di[j]]))
            elif self.jt[j] == JointType.SPHERICAL:
                out.append(_safe_exp_map_to_quat(dof[..., self.di[j]:self.di[j] + 3]))
            else:
                q = torch.zeros(dof.shape[:-1] + (4,), dtype=dof.dtype, device=dof.device)
                q[..., 3] = 1
                out.append(q)
        return torch.stack(out, dim=-2)

    def terms(self, pred, true_motion, target_dir=None):
        """The weighted terms [N, 13] of ``pred`` [N, T, D] (standardised), differentiable."""
        m = {k: torch.as_tensor(v).to(self.device, self.dtype) for k, v in mg._names(true_motion).items() if k in ("ROOT_POS", "ROOT_ROT", "JOINT_ROT", "CONTACTS")}
        T = pred.shape[1]
        f = pred * self.std[:T] + self.mean[:T]
        s, fn, w = self.sl, self.fn, self.w
        rp, rq = f[..., s["pos"]], _safe_exp_map_to_quat(f[..., s["rot"]])
        jp = f[..., s["jpos"]].reshape(f.shape[0], T, self.B - 1, 3)
        jq, con = self.dof_to_rot(f[..., s["jrot"]]), f[..., s["con"]]
        trp, trq, tjq, tcon = m["ROOT_POS"], m["ROOT_ROT"], m["JOINT_ROT"], m["CONTACTS"]
        bp, br = self.fk(rp, rq, jq)
        tbp, tbr = self.fk(trp, trq, tjq)
        dt = self.dt
        zero = torch.zeros(pred.shape[0], dtype=self.dtype, device=self.device)
        out = [None] * NT
        out[0] = w[0] * fn((trp[:, 1:] - trp[:, :-1]) / dt, (rp[:, 1:] - rp[:, :-1]) / dt)
        av = lambda q: quat_to_exp_map_grad_friendly(quat_diff(q[:, :-1], q[:, 1:])) / dt  # noqa: E731
        out[1] = w[1] * fn(av(trq), av(rq))
        out[2] = w[2] * fn(av(tjq), av(jq))
        out[3] = w[3] * fn(trp, rp)
        out[4] = w[4] * fn(quat_diff_angle(trq, rq), 0.0)
        out[5] = w[5] * fn(quat_diff_angle(tjq, jq), 0.0)
        out[6] = w[6] * fn(tcon, con)
        out[7] = w[7] * fn(tbp[..., 1:, :], jp)                       # the predicted joint-position features against the true FK
        if self.use_pos:
            out[8] = w[8] * fn(tbp, bp)
            out[9] = w[9] * fn(quat_diff_angle(tbr, br), 0.0)
            out[10] = w[10] * fn(bp[..., 1:, :], jp)                  # the prediction on both sides
            out[11] = w[11] * fn((tbp[:, 1:] - tbp[:, :-1]) / dt, (bp[:, 1:] - bp[:, :-1]) / dt)
        else:
            out[8] = out[9] = out[10] = out[11] = zero
        if self.use_target:
            td = torch.as_tensor(target_dir).to(self.device, self.dtype).reshape(-1, 2)
            d = rp[:, -1, 0:2] - rp[:, self.nprev - 1, 0:2]
            out[12] = torch.clamp(torch.sum(-td * d, dim=-1), min=-self.eps) * w[12]
        else:
            out[12] = zero
        return torch.stack(out, dim=-1)

    def terms_and_grad(self, pred, true_motion, target_dir=None, term=None):
        """(terms [N, 13], d sum(terms) / d pred); with ``term`` the gradient of that term alone."""
        x = torch.as_tensor(pred).detach().to(self.device, self.dtype).clone().requires_grad_(True)
        with torch.enable_grad():
            t = self.terms(x, true_motion, target_dir)
            total = (t if term is None else t[:, term]).sum()
            g = torch.autograd.grad(total, x, allow_unused=True)[0] if total.requires_grad else None
        return t.detach(), (torch.zeros_like(x) if g is None else g)


# ---- the fixture of tests/golden/make_golden_mdm_loss.py --------------------------------------------------------------------------------
class LossFixture:
    """``mdm_loss.npz``: the reference's ``motion_difference`` on group ``a`` (6 windows of 15 frames, 2 previous states) and group ``b``
    (3 windows of 20 frames, 3 previous states), for both loss functions."""

    def __init__(self, golden_dir):
        import json
        import os
        self.z = np.load(os.path.join(golden_dir, "mdm_loss.npz"))
        self.base_cfg = dict(json.loads(bytes(self.z["cfg_json"]).decode()), char_file="data/assets/humanoid.xml")

    def cfg(self, group, **over):
        return dict(self.base_cfg, num_prev_states=int(self.z[f"{group}_num_prev_states"]), **over)

    def inputs(self, group):
        """(pred [N, T, D], true motion dict, target_dir [N, 2], mean, std) as float32 tensors."""
        t = lambda k: torch.from_numpy(self.z[f"{group}_{k}"])  # noqa: E731
        true = {"ROOT_POS": t("root_pos"), "ROOT_ROT": t("root_rot"), "JOINT_ROT": t("joint_rot"), "CONTACTS": t("contacts")}
        return t("pred"), true, t("target_dir"), t("mean"), t("std")

    def recorded(self, group, loss_fn):
        """(terms [N, 13], err32 [13], grad [N, T, D], the row of the per-term gradients, term_grads [13, T, D]) in float64."""
        t = lambda k: torch.from_numpy(self.z[f"{group}_{loss_fn}_{k}"]).double()  # noqa: E731
        return t("terms"), t("err32"), t("grad"), int(self.z[f"{group}_term_row"]), t("term_grads")


def rows(true_motion, idx):
    return {k: v[idx] for k, v in true_motion.items()}


def only_weight(cfg, k):
    """``cfg`` with every loss weight but term k's at zero."""
    return dict(cfg, **{key: (cfg[key] if i == k else 0.0) for i, key in enumerate(WEIGHT_KEYS)})


def term_grads(ref, pred, true_motion, target_dir=None):
    """(terms [N, 13], the gradient of every term alone [13, N, T, D]) from one graph of ``ref`` (an ``MdmLossRef``): term k's gradient
    under the default weights is the whole gradient under ``only_weight(cfg, k)``."""
    x = torch.as_tensor(pred).detach().to(ref.device, ref.dtype).clone().requires_grad_(True)
    with torch.enable_grad():
        t = ref.terms(x, true_motion, target_dir)
        gs = []
        for k in range(NT):
            tk = t[:, k].sum()
            g = torch.autograd.grad(tk, x, retain_graph=True, allow_unused=True)[0] if tk.requires_grad else None
            gs.append(torch.zeros_like(x) if g is None else g)
    return t.detach(), torch.stack(gs)
