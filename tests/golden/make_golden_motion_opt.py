#!/usr/bin/env python3
"""Generate the kinematic motion optimiser fixtures (``motion_opt_*.npz``) from the REAL reference.

Run where the reference checkout is available (the GPU tests only read the fixtures it writes):

    python tests/golden/make_golden_motion_opt.py          # the two per-clip fixtures
    python tests/golden/make_golden_motion_opt.py terms    # motion_opt_terms.npz, from the committed per-clip fixtures

The reference is driven as in ``make_golden.py`` (a ``parc`` package alias, empty module stubs, our data-only ms-file decoder);
in addition ``wandb.run`` is ``None`` and ``trimesh.creation.icosphere`` is the normalised icosahedron (subdivision 0 only), the
one trimesh call the point sampler makes.  Each ``.npz`` holds inputs and outputs only.

Per case (clip, frame stride):
  * ``pts_stage2`` / ``pts_motion_opt``: the sample points of the two sampler configs (flat, body index per point);
  * the body constraints of ``compute_approx_body_constraints`` (computed at full rate, then mapped by the stride as
    ``run_optimize_motions.py`` does) and the full-rate source frames they were computed from;
  * loss terms and autograd gradients of ``motion_terrain_contact_loss_localized`` at state a (target = source), b (perturbed)
    and c (20 reference Adam steps from b), plus state b with ``w_contact = 0``, ``w_sliding = 0`` and no constraints;
  * the loss dict at each of the 20 steps, and (stride-1 case) after 300 steps.

Mode ``terms`` writes ``motion_opt_terms.npz``: for both cases, at state b, the loss dict and the autograd gradient with each of the
nine weights on alone at its stage-2 value (``terms_<clip>`` [9 one-hot runs, 9 terms], ``grad_<clip>`` [9, F, 6 + D]).  Sources, contacts,
terrain, constraints and state b are read back from the committed per-clip fixtures, so both records speak of exactly the same state.
"""
import os
import sys
import types

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, REPO)
sys.dont_write_bytecode = True

for _name in ["trimesh", "trimesh.creation", "wandb", "gym", "gym.spaces", "isaacgym", "isaacgym.gymapi",
              "isaacgym.gymtorch", "isaacgym.gymutil"]:
    sys.modules[_name] = types.ModuleType(_name)
sys.modules["wandb"].run = None
sys.modules["trimesh"].creation = sys.modules["trimesh.creation"]
_parc = types.ModuleType("parc")
_parc.__path__ = [os.path.join(REF, "PARC")]
sys.modules["parc"] = _parc

import numpy as np  # noqa: E402
import torch  # noqa: E402

from parc_amd import motion_opt as mo  # noqa: E402
from parc_amd import ms_file  # noqa: E402


def _icosphere(subdivisions=0, radius=1.0):
    assert subdivisions == 0
    return types.SimpleNamespace(vertices=mo.icosahedron_vertices() * radius)


sys.modules["trimesh.creation"].icosphere = _icosphere

import parc.anim.kin_char_model as kcm  # noqa: E402
import parc.motion_synthesis.motion_opt.motion_optimization as moopt  # noqa: E402
import parc.util.geom_util as geom_util  # noqa: E402
import parc.util.terrain_util as terrain_util  # noqa: E402
import parc.util.torch_util as tu  # noqa: E402

torch.set_num_threads(4)
STAGE2 = dict(sphere_num_subdivisions=0, box_num_slices=2, box_dim_x=3, box_dim_y=6, capsule_num_circle_points=4,
              capsule_num_sphere_subdivisions=0, capsule_num_cylinder_slices=4)
MOTION_OPT = dict(sphere_num_subdivisions=0, box_num_slices=2, box_dim_x=2, box_dim_y=2, capsule_num_circle_points=2,
                  capsule_num_sphere_subdivisions=0, capsule_num_cylinder_slices=1)
WEIGHTS = dict(w_root_pos=1.0, w_root_rot=10.0, w_joint_rot=1.0, w_smoothness=10.0, w_penetration=1000.0, w_contact=1000.0,
               w_sliding=10.0, w_body_constraints=1000.0, w_jerk=1000.0)
MAX_JERK = 1000.0
STEP_SIZE = 0.001
CASES = [("dec2024_teaser_717_1_modified_opt", 1, 300), ("civilization", 4, 0)]


def ref_points(char, cfg):
    c = dict(cfg)
    c["capsule_num_sphere_subdivisons"] = c.pop("capsule_num_sphere_subdivisions")
    pts = geom_util.get_char_point_samples(char, **c)
    flat = torch.cat(pts).numpy().astype(np.float32)
    body = np.concatenate([np.full(p.shape[0], b, np.int32) for b, p in enumerate(pts)])
    return pts, flat, body


def loss_and_grad(state, src, terrain, pts, char, constraints, **w):
    rp, rr, dof = [s.clone().requires_grad_(True) for s in state]
    loss, d = moopt.motion_terrain_contact_loss_localized(
        tgt_root_pos=rp, tgt_root_rot=rr, tgt_joint_dof=dof, terrain=terrain, body_points=pts, char_model=char,
        body_constraints=constraints, max_jerk=MAX_JERK, **src, **w)
    loss.backward()
    terms = np.array([float(d[moopt.LossType(k)]) for k in range(9)], np.float64)
    return terms, float(loss.item()), [x.grad.numpy().copy() for x in (rp, rr, dof)]


def adam_steps(state, n, src, terrain, pts, char, constraints, **w):
    params = [s.clone().requires_grad_(True) for s in state]
    opt = torch.optim.Adam(params, lr=STEP_SIZE)
    hist = []
    for _ in range(n):
        opt.zero_grad()
        loss, d = moopt.motion_terrain_contact_loss_localized(
            tgt_root_pos=params[0], tgt_root_rot=params[1], tgt_joint_dof=params[2], terrain=terrain, body_points=pts,
            char_model=char, body_constraints=constraints, max_jerk=MAX_JERK, **src, **w)
        loss.backward()
        opt.step()
        hist.append([float(d[moopt.LossType(k)]) for k in range(9)])
    return [p.detach().clone() for p in params], np.array(hist, np.float64)


def constraints_to_arrays(cons):
    body, start, end, point = [], [], [], []
    for b, lst in enumerate(cons):
        for c in lst:
            body.append(b); start.append(int(c.start_frame_idx)); end.append(int(c.end_frame_idx))
            point.append(np.asarray(c.constraint_point.detach().numpy(), np.float32))
    return (np.array(body, np.int32), np.array(start, np.int32), np.array(end, np.int32),
            np.array(point, np.float32).reshape(-1, 3))


def perturb(state, n):
    """Deterministic: the root sinks 5-10 cm over the middle third, ~0.05 rad of root / dof noise, no exact zeros."""
    rp, rr, dof = [s.clone() for s in state]
    g = torch.Generator().manual_seed(1234)
    lo, hi = n // 3, max(n // 3 + 1, 2 * n // 3)
    drop = 0.05 + 0.05 * torch.rand(hi - lo, generator=g)
    rp[lo:hi, 2] -= drop
    rr += 0.05 * torch.randn(rr.shape, generator=g)
    dof += 0.05 * torch.randn(dof.shape, generator=g)
    dof[dof == 0] = 1e-3
    rr[rr == 0] = 1e-3
    return rp, rr, dof


def main():
    char = kcm.KinCharModel("cpu")
    char.load_char_file(os.path.join(REPO, "data/assets/humanoid.xml"))
    pts2, flat2, body2 = ref_points(char, STAGE2)
    _, flat_mo, body_mo = ref_points(char, MOTION_OPT)
    for clip, stride, long_iters in CASES:
        d = ms_file.load_ms_file(os.path.join(REPO, "data/motion_terrains", clip + ".pkl"), load_misc=False)
        m, td = d.motion_data, d.terrain_data
        terrain = terrain_util.SubTerrain(x_dim=td.hf.shape[0], y_dim=td.hf.shape[1], dx=td.dx, dy=td.dx,
                                          min_x=float(td.min_point[0]), min_y=float(td.min_point[1]), device="cpu")
        terrain.hf = torch.tensor(np.asarray(td.hf), dtype=torch.float32)
        rp_full = torch.tensor(np.asarray(m.root_pos), dtype=torch.float32)
        rq_full = torch.tensor(np.asarray(m.root_rot), dtype=torch.float32)
        jr_full = torch.tensor(np.asarray(m.joint_rot), dtype=torch.float32)
        ct_full = torch.tensor(np.asarray(m.body_contacts), dtype=torch.float32)
        cons = moopt.compute_approx_body_constraints(rp_full, rq_full, jr_full, ct_full, char, terrain)
        cb, cs_full, ce_full, cp = constraints_to_arrays(cons)
        for lst in cons:
            for c in lst:
                c.start_frame_idx = int(np.ceil(c.start_frame_idx / stride))
                c.end_frame_idx = int(c.end_frame_idx // stride)
        _, cs, ce, _ = constraints_to_arrays(cons)

        rp, rq, jr, ct = rp_full[::stride], rq_full[::stride], jr_full[::stride], ct_full[::stride]
        src_body_pos, src_body_rot = char.forward_kinematics(rp, rq, jr)
        src = dict(src_root_pos=rp, src_root_rot_quat=rq, src_joint_rot=jr, contacts=ct,
                   src_body_vels=src_body_pos[1:] - src_body_pos[:-1],
                   src_body_rot_vels=tu.quat_diff_angle(src_body_rot[1:], src_body_rot[:-1]))
        state_a = (rp.clone(), tu.quat_to_exp_map(rq), char.rot_to_dof(jr))
        state_b = perturb(state_a, rp.shape[0])
        out = dict(clip=np.array(clip), stride=np.int32(stride), fps=np.int32(m.fps // stride),
                   root_pos=rp.numpy(), root_rot=rq.numpy(), joint_rot=jr.numpy(), contacts=ct.numpy(),
                   full_root_pos=rp_full.numpy(), full_root_rot=rq_full.numpy(), full_joint_rot=jr_full.numpy(),
                   full_contacts=ct_full.numpy(),
                   hf=np.asarray(td.hf, np.float32), min_point=np.asarray(td.min_point, np.float32), dx=np.float32(td.dx),
                   pts_stage2=flat2, pts_stage2_body=body2, pts_motion_opt=flat_mo, pts_motion_opt_body=body_mo,
                   cons_body=cb, cons_start_full=cs_full, cons_end_full=ce_full, cons_start=cs, cons_end=ce, cons_point=cp,
                   contact_body_id=np.array([char.get_contact_body_id(char.get_body_name(b))
                                             if char.get_body_name(b) in char._contact_body_names else -1
                                             for b in range(char.get_num_joints())], np.int32),
                   max_jerk=np.float32(MAX_JERK), step_size=np.float32(STEP_SIZE),
                   weights=np.array([WEIGHTS[k] for k in mo.WEIGHT_KEYS], np.float32))
        state_c, hist20 = adam_steps(state_b, 20, src, terrain, pts2, char, cons, **WEIGHTS)
        for tag, st in (("a", state_a), ("b", state_b), ("c", state_c)):
            terms, total, grads = loss_and_grad(st, src, terrain, pts2, char, cons, **WEIGHTS)
            out[f"state_{tag}_root_pos"], out[f"state_{tag}_root_rot"], out[f"state_{tag}_dof"] = [s.numpy() for s in st]
            out[f"terms_{tag}"], out[f"total_{tag}"] = terms, np.float64(total)
            out[f"grad_{tag}_root_pos"], out[f"grad_{tag}_root_rot"], out[f"grad_{tag}_dof"] = grads
        for tag, kw, c in (("no_contact", dict(WEIGHTS, w_contact=0.0), cons), ("no_sliding", dict(WEIGHTS, w_sliding=0.0), cons),
                           ("no_constraints", WEIGHTS, None)):
            terms, total, grads = loss_and_grad(state_b, src, terrain, pts2, char, c, **kw)
            out[f"terms_b_{tag}"] = terms
            out[f"grad_b_{tag}_root_pos"], out[f"grad_b_{tag}_root_rot"], out[f"grad_b_{tag}_dof"] = grads
        out["hist20"] = hist20
        if long_iters:
            _, hist = adam_steps(state_b, long_iters, src, terrain, pts2, char, cons, **WEIGHTS)
            out["hist_long"] = hist[-1:]
            out["long_iters"] = np.int32(long_iters)
        path = os.path.join(HERE, f"motion_opt_{clip}_s{stride}.npz")
        np.savez_compressed(path, **out)
        print("wrote", path, os.path.getsize(path), "bytes; terms b:", out["terms_b"])


def main_terms():
    char = kcm.KinCharModel("cpu")
    char.load_char_file(os.path.join(REPO, "data/assets/humanoid.xml"))
    pts2, flat2, _ = ref_points(char, STAGE2)
    out = {}
    for clip, stride, _ in CASES:
        z = np.load(os.path.join(HERE, f"motion_opt_{clip}_s{stride}.npz"))
        assert np.array_equal(flat2, z["pts_stage2"])
        assert np.array_equal(z["weights"], np.array([WEIGHTS[k] for k in mo.WEIGHT_KEYS], np.float32))
        hf = torch.tensor(z["hf"])
        terrain = terrain_util.SubTerrain(x_dim=hf.shape[0], y_dim=hf.shape[1], dx=float(z["dx"]), dy=float(z["dx"]),
                                          min_x=float(z["min_point"][0]), min_y=float(z["min_point"][1]), device="cpu")
        terrain.hf = hf
        rp, rq, jr, ct = [torch.tensor(z[k]) for k in ("root_pos", "root_rot", "joint_rot", "contacts")]
        src_body_pos, src_body_rot = char.forward_kinematics(rp, rq, jr)
        src = dict(src_root_pos=rp, src_root_rot_quat=rq, src_joint_rot=jr, contacts=ct,
                   src_body_vels=src_body_pos[1:] - src_body_pos[:-1],
                   src_body_rot_vels=tu.quat_diff_angle(src_body_rot[1:], src_body_rot[:-1]))
        cons = [[] for _ in range(char.get_num_joints())]
        for b, s, e, p in zip(z["cons_body"], z["cons_start"], z["cons_end"], z["cons_point"]):
            c = moopt.BodyConstraint()
            c.start_frame_idx, c.end_frame_idx, c.constraint_point = int(s), int(e), torch.tensor(p)
            cons[int(b)].append(c)
        state_b = tuple(torch.tensor(z[f"state_b_{k}"]) for k in ("root_pos", "root_rot", "dof"))
        # the rebuilt inputs reproduce the committed record of the weighted total before anything new is written
        terms, _, grads = loss_and_grad(state_b, src, terrain, pts2, char, cons, **WEIGHTS)
        # (to float32 summation order, which differs between hosts and thread counts)
        g_all, g_ref = np.concatenate(grads, 1), np.concatenate([z[f"grad_b_{k}"] for k in ("root_pos", "root_rot", "dof")], 1)
        print(clip, "rebuilt vs committed, all weights on: terms rel", np.abs(terms / z["terms_b"] - 1).max(),
              "grad", np.abs(g_all - g_ref).max() / np.abs(g_ref).max(), "of max")
        assert np.allclose(terms, z["terms_b"], rtol=1e-6, atol=0) and np.abs(g_all - g_ref).max() <= 1e-6 * np.abs(g_ref).max()
        all_terms, all_grads = [], []
        for key in mo.WEIGHT_KEYS:
            w = {k: (WEIGHTS[k] if k == key else 0.0) for k in mo.WEIGHT_KEYS}
            terms, _, grads = loss_and_grad(state_b, src, terrain, pts2, char, cons, **w)
            all_terms.append(terms)
            all_grads.append(np.concatenate(grads, axis=1).astype(np.float32))
        out[f"terms_{clip}"] = np.array(all_terms, np.float64)
        out[f"grad_{clip}"] = np.array(all_grads, np.float32)
        print(clip, "largest gradient entry per term:", [float(np.abs(g).max()) for g in all_grads])
    path = os.path.join(HERE, "motion_opt_terms.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if sys.argv[1:] == ["terms"]:
        main_terms()
    elif sys.argv[1:]:
        sys.exit("usage: make_golden_motion_opt.py [terms]")
    else:
        main()
