"""The motion generator's training loss on the GPU: the reference's ``MDM.motion_difference`` (``motion_generator/mdm.py:573-692``).

``MotionLoss(cfg, device)`` takes the keys of the reference's ``parc_1_train_gen_default.yaml`` (the thirteen weights, ``use_pos_loss``,
``use_target_loss``, ``target_dir_len_eps``, ``sequence_fps``, ``num_prev_states``, ``char_file``) and a loss function (``squared_l2`` or
``pseudo_huber``).  ``terms_and_grad(pred, true_motion, target_dir)`` is one kernel launch (``parc_amd/csrc/parc_mdm_loss.hpp``,
DESIGN.md section 8l): the weighted per-window value of every term ``[N, 13]`` and the derivative of each window's sum of terms with
respect to the standardised prediction ``[N, T, D]``.  ``MotionLossFn`` hands both to autograd.  There is no eager fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import torch

from parc_amd import lib as L
from parc_amd import motion_generator as mg
from parc_amd.char_model import CharModel
from parc_amd.tool_handle import ToolHandle

# the terms in the order the reference's `losses` dict holds them (mdm.py:618-688), and the config key of each weight
TERM_NAMES = ("VEL_ROOT_POS_LOSS", "VEL_ROOT_ROT_LOSS", "VEL_JOINT_ROT_LOSS", "SIMPLE_ROOT_POS_LOSS", "SIMPLE_ROOT_ROT_LOSS",
              "SIMPLE_JOINT_ROT_LOSS", "SIMPLE_CONTACT_LOSS", "SIMPLE_BODY_POS_LOSS", "FK_BODY_POS_LOSS", "FK_BODY_ROT_LOSS",
              "BODY_POS_CONSISTENCY_LOSS", "VEL_FK_BODY_POS_LOSS", "TARGET_LOSS")
WEIGHT_KEYS = ("w_vel_root_pos", "w_vel_root_rot", "w_vel_joint_rot", "w_simple_root_pos", "w_simple_root_rot", "w_simple_joint_rot",
               "w_simple_contacts", "w_simple_body_pos", "w_body_pos", "w_body_rot", "w_body_pos_consistency", "w_body_vel", "w_target")
FK_TERMS = (8, 9, 10, 11)   # what use_pos_loss switches
NUM_TERMS = L.MLOSS_NUM_TERMS
LOSS_FNS = {"squared_l2": L.MLOSS_SQUARED_L2, "pseudo_huber": L.MLOSS_PSEUDO_HUBER}
KERNELS = ("loss",)


def check_loss_config(cfg: dict, loss_fn: str = "squared_l2"):
    """The refusals that the config alone decides; each message names its key."""
    if cfg.get("use_hf_collision_loss", False):
        raise ValueError("use_hf_collision_loss: true is not built (the heightfield collision term of the generator's loss, DESIGN.md section 8b)")
    feats = cfg.get("features", {})
    if feats.get("rot_type", "DEFAULT") != "DEFAULT":
        raise ValueError(f"features.rot_type {feats.get('rot_type')!r}: the loss builds DEFAULT (root exp map, joint dofs)")
    if tuple(feats.get("frame_components", mg.FRAME_COMPONENTS)) != mg.FRAME_COMPONENTS:
        raise ValueError(f"features.frame_components must be {list(mg.FRAME_COMPONENTS)} in that order")
    if cfg.get("target_type", "XY_DIR") != "XY_DIR":
        raise ValueError(f"target_type {cfg.get('target_type')!r}: the loss builds XY_DIR")
    if loss_fn not in LOSS_FNS:
        raise ValueError(f"loss function {loss_fn!r}: train_loss_fn / test_loss_fn must be one of {sorted(LOSS_FNS)}")
    missing = [k for k in WEIGHT_KEYS if k not in cfg]
    if missing:
        raise ValueError(f"missing loss weights: {missing}")


class MotionLoss(ToolHandle):
    """See the module docstring.  ``mean`` / ``std`` ``[T, D]`` are the feature statistics the prediction is standardised with; they can
    be given here or per call."""
    PREFIX, KERNELS = "parc_mloss", KERNELS

    def __init__(self, cfg: dict, device="cuda:0", loss_fn: str = "squared_l2", mean=None, std=None, char_model: Optional[CharModel] = None):
        check_loss_config(cfg, loss_fn)
        super().__init__(device)
        self.cfg, self.loss_fn = cfg, loss_fn
        self.char_model = char_model or CharModel(mg._char_path(cfg))
        self.B, self.D = self.char_model.get_num_bodies(), mg.frame_dim(self.char_model)
        self.nprev = int(cfg["num_prev_states"])
        p = L.ParcMotionLossParams()
        p.device = self.device_index
        p.model = L.make_char_model(self.char_model)
        p.sequence_fps, p.num_prev_states = float(cfg["sequence_fps"]), self.nprev
        for i, k in enumerate(WEIGHT_KEYS):
            p.weights[i] = float(cfg[k])
        p.use_pos_loss, p.use_target_loss = int(bool(cfg.get("use_pos_loss", True))), int(bool(cfg.get("use_target_loss", False)))
        p.target_dir_len_eps = float(cfg.get("target_dir_len_eps", 0.1))
        p.loss_fn = LOSS_FNS[loss_fn]
        self.use_target = bool(p.use_target_loss)
        self._create_handle(p)
        self.mean = self.std = None
        if mean is not None:
            self.set_stats(mean, std)

    def set_stats(self, mean, std):
        self.mean = torch.as_tensor(mean, dtype=torch.float32).to(self.device).contiguous()
        self.std = torch.as_tensor(std, dtype=torch.float32).to(self.device).contiguous()

    def _f32(self, t, shape, what):
        t = torch.as_tensor(t, device=self.device).to(torch.float32).contiguous()
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{what} must be {list(shape)}, not {list(t.shape)}")
        return t

    def terms_and_grad(self, pred: torch.Tensor, true_motion: Dict[str, torch.Tensor], target_dir=None, mean=None, std=None):
        """``pred`` [N, T, D] standardised; ``true_motion`` as the sampler emits it (``ROOT_POS`` [N, T, 3], ``ROOT_ROT`` [N, T, 4],
        ``JOINT_ROT`` [N, T, B - 1, 4], ``CONTACTS`` [N, T, B]; keys by name or enum member); ``target_dir`` [N, 2] (read with
        ``use_target_loss``).  Returns (terms [N, 13], grad [N, T, D]); no host synchronisation."""
        if pred.dim() != 3 or pred.shape[-1] != self.D:
            raise ValueError(f"pred must be [N, T, {self.D}], not {list(pred.shape)}")
        n, T = int(pred.shape[0]), int(pred.shape[1])
        m = mg._names(true_motion)
        J = self.B - 1
        pred = self._f32(pred.detach(), (n, T, self.D), "pred")
        mean = self.mean if mean is None else mean
        std = self.std if std is None else std
        if mean is None or std is None:
            raise ValueError("the feature mean / std are not set")
        mean, std = self._f32(mean[:T], (T, self.D), "mean"), self._f32(std[:T], (T, self.D), "std")
        rp, rr = self._f32(m["ROOT_POS"], (n, T, 3), "ROOT_POS"), self._f32(m["ROOT_ROT"], (n, T, 4), "ROOT_ROT")
        jr, ct = self._f32(m["JOINT_ROT"], (n, T, J, 4), "JOINT_ROT"), self._f32(m["CONTACTS"], (n, T, self.B), "CONTACTS")
        td = None
        if self.use_target:
            if target_dir is None:
                raise ValueError("use_target_loss needs target_dir")
            td = self._f32(torch.as_tensor(target_dir, device=self.device).reshape(n, 2), (n, 2), "target_dir")
        terms = torch.empty((n, NUM_TERMS), dtype=torch.float32, device=self.device)
        grad = torch.empty((n, T, self.D), dtype=torch.float32, device=self.device)
        a = L.ParcMotionLossArgs()
        a.n, a.num_frames = n, T
        a.pred, a.mean, a.std = pred.data_ptr(), mean.data_ptr(), std.data_ptr()
        a.root_pos, a.root_rot, a.joint_rot, a.contacts = rp.data_ptr(), rr.data_ptr(), jr.data_ptr(), ct.data_ptr()
        a.target_dir = td.data_ptr() if td is not None else None
        a.terms, a.grad = terms.data_ptr(), grad.data_ptr()
        self._call("eval", C.byref(a), self._stream())
        # the inputs stay alive until the launch is queued; the caching allocator keeps their memory for the stream's later work
        del pred, mean, std, rp, rr, jr, ct, td
        return terms, grad

    def __call__(self, pred, true_motion, target_dir=None):
        return MotionLossFn.apply(pred, self, true_motion, target_dir)


class MotionLossFn(torch.autograd.Function):
    """``loss, terms = MotionLossFn.apply(pred, motion_loss, true_motion, target_dir)``: ``loss`` [N] is each window's weighted sum of
    terms (differentiable with respect to ``pred``), ``terms`` [N, 13] the weighted terms (for logging; no gradient).  ``motion_loss``
    is a :class:`MotionLoss` or any object with its ``terms_and_grad``."""

    @staticmethod
    def forward(ctx, pred, motion_loss, true_motion, target_dir):
        terms, grad = motion_loss.terms_and_grad(pred, true_motion, target_dir)
        terms, grad = terms.to(pred.device, pred.dtype), grad.to(pred.device, pred.dtype)   # a float64 yardstick in place of the kernel
        ctx.save_for_backward(grad)
        ctx.mark_non_differentiable(terms)
        return terms.sum(dim=-1), terms

    @staticmethod
    def backward(ctx, grad_out, _grad_terms):
        (grad,) = ctx.saved_tensors
        return grad_out[:, None, None] * grad, None, None, None
