#!/usr/bin/env python3
"""Generate ``mdm_loss.npz`` from the REAL reference: ``MDM.motion_difference`` (motion_generator/mdm.py:573-692) on the CPU.

Run where the reference checkout is available (the tests only read the fixture it writes):

    python tests/golden/make_golden_mdm_loss.py

The reference's ``MDM`` is built as ``make_golden_mdm.py`` builds it (its preamble is imported from there: the ``parc`` package alias
and the module stubs), in fp32 and in float64.  Two groups of windows:

  ``a``  6 windows of 15 frames, ``num_prev_states`` 2: the first six windows of ``motion_sampler_none.npz`` (real windows of the bundled
         clips, canonicalised by the reference's sampler)
  ``b``  3 windows of 20 frames, ``num_prev_states`` 3 (the MDM "edge" shape): frames 40.., 100.., 160.. of the bundled
         ``civilization`` clip, moved so that the first root position is at the origin in x and y

The feature mean is random, the std in [0.1, 0.6].  The prediction is the standardised true features plus normal noise of scale 0.01,
0.3 and 1.0 (rows cycle through the scales); in the last row of each group the root exp map is pushed beyond pi along its own axis.
The target directions are the unit direction of travel of the true window, alternately kept and reversed, so that the target term
clamps in some rows (travel along the target by more than ``target_dir_len_eps``) and not in others; ``use_target_loss`` is on.  For
both loss functions the file holds, per group: the weighted terms of the float64 run (``*_terms``, stored as float32), the largest
fp32-vs-float64 difference per term (``*_err32``), the autograd gradient of the default-weighted total with respect to the
standardised prediction (``*_grad``), and for rows 1 of ``a`` and 0 of ``b`` the gradient of every term alone (``*_term_grads``).
Per group the script takes the first seed from SEED on (recorded as ``*_seed``) at which the reference's fp32 and float64 runs agree to
1e-4 relative on every term (a quaternion on a ``quat_pos`` or mask branch cut breaks that) and to half of the bound the tests hold an
fp32 evaluation to, 2e-5 |ref| + 1e-6, so that an fp32 evaluation in another order of operations still meets that bound.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_mdm as G  # noqa: E402  (the preamble: the reference's modules under the `parc` alias)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from parc.motion_generator.diffusion_util import MDMFrameType, MDMKeyType  # noqa: E402
ref_mdm = G.ref_mdm

SEED = 0
SCALES = (0.01, 0.3, 1.0)
TERMS = ("VEL_ROOT_POS_LOSS", "VEL_ROOT_ROT_LOSS", "VEL_JOINT_ROT_LOSS", "SIMPLE_ROOT_POS_LOSS", "SIMPLE_ROOT_ROT_LOSS", "SIMPLE_JOINT_ROT_LOSS",
         "SIMPLE_CONTACT_LOSS", "SIMPLE_BODY_POS_LOSS", "FK_BODY_POS_LOSS", "FK_BODY_ROT_LOSS", "BODY_POS_CONSISTENCY_LOSS", "VEL_FK_BODY_POS_LOSS",
         "TARGET_LOSS")
GROUPS = {"a": dict(cfg=dict(seq_len=15, num_prev_states=2, d_model=32, num_heads=2, d_hid=32, num_layers=1), term_row=1),
          "b": dict(cfg=dict(seq_len=20, num_prev_states=3, d_model=32, num_heads=2, d_hid=32, num_layers=1), term_row=0)}
LOSS_FNS = {"squared_l2": ref_mdm.squared_l2_loss_fn, "pseudo_huber": ref_mdm.pseudo_huber_loss_fn}


def true_windows(name):
    if name == "a":
        d = np.load(os.path.join(HERE, "motion_sampler_none.npz"))
        return {k: torch.from_numpy(d[k][:6].astype(np.float32)) for k in ("root_pos", "root_rot", "joint_rot", "contacts")}
    from parc_amd import motion_lib
    clip = motion_lib.load_clip(os.path.join(G.REPO, "data/motion_terrains/civilization.pkl"))
    out = {k: [] for k in ("root_pos", "root_rot", "joint_rot", "contacts")}
    for s in (40, 100, 160):
        rp = np.asarray(clip.root_pos[s:s + 20], np.float32).copy()
        rp[:, :2] -= rp[0, :2]
        out["root_pos"].append(rp)
        out["root_rot"].append(np.asarray(clip.root_rot[s:s + 20], np.float32))
        out["joint_rot"].append(np.asarray(clip.joint_rot[s:s + 20], np.float32))
        out["contacts"].append(np.asarray(clip.contacts[s:s + 20], np.float32))
    return {k: torch.from_numpy(np.stack(v)) for k, v in out.items()}


def motion_dict(m, w, dtype):
    """The sampler's component dict; JOINT_POS is the FK of the window (the reference's sampler emits body positions there)."""
    rp, rr, jr = w["root_pos"].to(dtype), w["root_rot"].to(dtype), w["joint_rot"].to(dtype)
    bp, _ = m._kin_char_model.forward_kinematics(rp, rr, jr)
    return {MDMFrameType.ROOT_POS: rp, MDMFrameType.ROOT_ROT: rr, MDMFrameType.JOINT_POS: bp[..., 1:, :], MDMFrameType.JOINT_ROT: jr,
            MDMFrameType.CONTACTS: w["contacts"].to(dtype)}


def run(m, w, pred, tdir, loss_fn, dtype, term_row):
    x = pred.to(dtype).clone().requires_grad_(True)
    true = motion_dict(m, w, dtype)
    losses = m.motion_difference(true, m.extract_motion_features(x), {MDMKeyType.TARGET_KEY: tdir.to(dtype).unsqueeze(1)}, loss_fn)
    terms = torch.stack([losses[ref_mdm.LossType[k]] for k in TERMS], dim=-1)
    grad = torch.autograd.grad(terms.sum(), x, retain_graph=True)[0]
    tg = torch.stack([torch.autograd.grad(terms[term_row, k], x, retain_graph=True)[0][term_row] for k in range(len(TERMS))])
    return terms.detach(), grad, tg


def group(name, grp, seed):
    """The arrays of one group at one seed, or None when fp32 and float64 are too far apart there."""
    arrs = {}
    shape = dict(cfg=grp["cfg"], seed=SEED)
    models = {}
    for dtype in (torch.float32, torch.float64):
        m, cfg = G.build(dtype, shape)
        m._use_target_loss = True
        models[dtype] = m
    m32 = models[torch.float32]
    T, D = cfg["seq_len"], m32._motion_frame_dof
    g = torch.Generator().manual_seed(seed + 10 + len(name))
    mean, std = torch.randn((T, D), generator=g) * 0.3, torch.rand((T, D), generator=g) * 0.5 + 0.1
    for dtype, m in models.items():
        m._mdm_features_mean, m._mdm_features_std = mean.to(dtype), std.to(dtype)
    w = true_windows(name)
    n = w["root_pos"].shape[0]
    x0 = m32.assemble_mdm_features(motion_dict(m32, w, torch.float32))
    scale = torch.tensor([SCALES[i % 3] for i in range(n)])[:, None, None]
    pred = x0 + scale * torch.randn(x0.shape, generator=g)
    e = pred[-1, :, 3:6] * std[:, 3:6] + mean[:, 3:6]                      # the last row: the root exp map beyond pi, along its own axis
    e = e * (3.6 / e.norm(dim=-1, keepdim=True))
    pred[-1, :, 3:6] = (e - mean[:, 3:6]) / std[:, 3:6]
    pred = pred.float()
    travel = w["root_pos"][:, -1, :2] - w["root_pos"][:, cfg["num_prev_states"] - 1, :2]
    tdir = travel / travel.norm(dim=-1, keepdim=True).clamp(min=1e-6)
    tdir = tdir * torch.tensor([1.0 if i % 2 == 0 else -1.0 for i in range(n)])[:, None]
    arrs.update({f"{name}_{k}": v.numpy() for k, v in w.items()})
    arrs.update({f"{name}_pred": pred.numpy(), f"{name}_mean": mean.numpy(), f"{name}_std": std.numpy(), f"{name}_target_dir": tdir.numpy(),
                 f"{name}_num_prev_states": np.int32(cfg["num_prev_states"]), f"{name}_term_row": np.int32(grp["term_row"])})
    for fname, fn in LOSS_FNS.items():
        t32, _, _ = run(m32, w, pred, tdir, fn, torch.float32, grp["term_row"])
        t64, g64, tg64 = run(models[torch.float64], w, pred, tdir, fn, torch.float64, grp["term_row"])
        err = (t32.double() - t64).abs()
        rel = (err / t64.abs().clamp(min=1e-6)).max(dim=0).values
        clamped = (t64[:, -1] == -cfg["target_dir_len_eps"] * cfg["w_target"])
        print(name, fname, "seed", seed, "fp32 vs float64, worst relative per term:", " ".join("%.1e" % r for r in rel.tolist()),
              "| target clamps in rows", clamped.nonzero().flatten().tolist())
        # 1e-4 relative on every term, and half of the bound the tests hold an fp32 evaluation to (2e-5 |ref| + 1e-6), so that an fp32
        # evaluation in another order of operations still meets that bound
        if not ((rel < 1e-4).all() and (err <= 0.5 * (2e-5 * t64.abs() + 1e-6)).all()):
            return None, cfg
        assert clamped.any() and not clamped.all()
        assert torch.isfinite(g64).all() and torch.isfinite(tg64).all()
        arrs[f"{name}_{fname}_terms"] = t64.numpy().astype(np.float32)
        arrs[f"{name}_{fname}_err32"] = err.max(dim=0).values.numpy()
        arrs[f"{name}_{fname}_grad"] = g64.numpy().astype(np.float32)
        arrs[f"{name}_{fname}_term_grads"] = tg64.numpy().astype(np.float32)
    return arrs, cfg


def main(out_dir=HERE):
    arrs = {}
    for name, grp in GROUPS.items():
        for seed in range(SEED, SEED + 20):                                   # "pick another seed until it holds"
            got, cfg = group(name, grp, seed)
            if got is not None:
                break
        assert got is not None, name
        arrs.update(got)
        arrs[f"{name}_seed"] = np.int32(seed)
    import json
    keep = ("sequence_fps", "use_pos_loss", "target_dir_len_eps", "features", "target_type", "w_simple_root_pos",
            "w_simple_root_rot", "w_simple_joint_rot", "w_simple_contacts", "w_simple_body_pos", "w_body_pos_consistency", "w_vel_root_pos",
            "w_vel_root_rot", "w_vel_joint_rot", "w_body_pos", "w_body_rot", "w_body_vel", "w_target")
    arrs["cfg_json"] = np.frombuffer(json.dumps(dict({k: cfg[k] for k in keep}, use_target_loss=True, use_hf_collision_loss=False)).encode(), dtype=np.uint8)
    path = os.path.join(out_dir, "mdm_loss.npz")
    np.savez_compressed(path, **arrs)
    print("mdm_loss.npz", os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 800_000


if __name__ == "__main__":
    main(*sys.argv[1:2])
