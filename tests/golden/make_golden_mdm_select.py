#!/usr/bin/env python3
"""Generate ``mdm_select.npz`` from the REAL reference: the scoring loop of ``mdm_path.generate_frames_until_end_of_path``
(mdm_path.py:386-433) on hand-made frames, with ``slice_terrain=True`` (``terrain_util.slice_terrain_around_motion``, padding 1.2,
``localize=False``) and ``False``, and the acceptance test of ``parc_2_kin_gen.py:389``.  No generator is needed.

    python tests/golden/make_golden_mdm_select.py

The reference is imported as ``make_golden_mdm_path.py`` imports it (``make_golden_mdm``'s stubs and ``parc`` alias, the icosahedron for
``trimesh.creation.icosphere``).

Scene: two 24 x 20 terrains at dx 0.4.  A: min_point (-3.1, -2.3), plateaus stepped along x and y.  B: min_point (1.3, -2.7), every
cell another height.  Four candidates per path, so eight rows of at most 24 frames: random unit joint quaternions and 0 / 1 contacts
from a seed, straight walks of the root.
  path 0 (A): row 0 inside the terrain; row 1 leaves over +x / +y; row 2 = row 0 bit for bit (a tie the stable order must keep);
              row 3 starts outside -x / -y
  path 1 (B): row 4, 20 frames across the whole terrain and beyond on both sides (its slice is larger than the terrain); row 5
              unfinished (``final_frame`` -1: the slice drops the last frame, the penalty applies); row 6 ``final_frame == num_frames``;
              row 7 a single frame
Recorded per mode (``s/``: sliced, ``w/``: whole terrain): the min point and dims of the terrain every row was scored on, for ``s/`` the
sliced heightfields (packed), the weighted contact / pen losses, the total as sorted (penalty and the recorded noise included), the
sort of every path and the valid flags for ``thresholds``.

The script fails unless the record is a fair yardstick: every padded bound lies >= 1e-3 cells from a rounding boundary; the totals of a
path differ pairwise by more than 100 x (1e-5 |total| + 1e-6), the deliberate tie apart; every threshold lies that far from every loss;
``torch.sort`` kept the tie in row order.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_mdm as G  # noqa: E402,F401  (the module stubs and the parc alias)

import types  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

from parc_amd import motion_opt as mo  # noqa: E402


def _icosphere(subdivisions=0, radius=1.0):                        # the one trimesh call of the point sampler
    assert subdivisions == 0
    return types.SimpleNamespace(vertices=mo.icosahedron_vertices() * radius)


sys.modules["trimesh.creation"].icosphere = _icosphere

import parc.anim.kin_char_model as kcm  # noqa: E402
import parc.motion_synthesis.procgen.mdm_path as ref_path  # noqa: E402
import parc.util.geom_util as geom_util  # noqa: E402
import parc.util.motion_util as motion_util  # noqa: E402
import parc.util.terrain_util as terrain_util  # noqa: E402

REPO = os.path.abspath(os.path.join(HERE, "..", ".."))
SEED = 11
P, K, F, DX, PADDING = 2, 4, 24, 0.4, 1.2
W_CONTACT, W_PEN, PENALTY = 0.1, 0.1, 100.0
NOISE = [0.25, -0.5, 0.25, 1.0, -1.25, 0.625, -0.125, 0.375]      # rows 0 and 2 share theirs: the tie stays a tie
# parc_2_kin_gen_default.yaml's pen and total thresholds; its contact threshold (3.0) passes one row only with these random contact flags
THRESHOLDS = dict(max_contact_loss=12.0, max_pen_loss=8.0, max_total_loss=30.0)
TOL = lambda v: 1e-5 * abs(v) + 1e-6                               # noqa: E731  the tests' tolerance


def scene():
    ax = np.repeat(np.array([0.0, 0.5, -0.25], np.float32), 8)[:, None]
    ay = np.repeat(np.array([0.0, 0.125, -0.125, 0.25], np.float32), 5)[None, :]
    hf_a = (ax + ay).astype(np.float32)
    g = np.random.default_rng(5)
    hf_b = (g.permutation(24 * 20).reshape(24, 20).astype(np.float32) / 256.0 - 0.9).astype(np.float32)
    assert hf_a.shape == hf_b.shape == (24, 20) and len(np.unique(hf_b)) == 480
    return np.stack([hf_a, hf_b]), np.array([[-3.1, -2.3], [1.3, -2.7]], np.float32)


def rows():
    """root xy (start, step) and final_frame per row."""
    walks = [((0.03, 1.02), (0.1, 0.05), 12), ((5.03, 4.02), (0.15, 0.15), 12), None, ((-4.02, -3.03), (0.2, 0.1), 12),
             ((0.33, -3.53), (0.6, 0.48), 20), ((3.02, 0.03), (0.1, 0.05), -1), ((6.03, 1.02), (0.1, -0.05), 24), ((4.03, 2.02), (0.0, 0.0), 1)]
    g = torch.Generator().manual_seed(SEED)
    N = P * K
    pos = torch.zeros((N, F, 3))
    i = torch.arange(F, dtype=torch.float32)
    for r, w in enumerate(walks):
        if w is None:
            continue
        pos[r, :, 0] = w[0][0] + w[1][0] * i
        pos[r, :, 1] = w[0][1] + w[1][1] * i
        pos[r, :, 2] = 1.0 + 0.02 * i + 0.1 * r
    heading = torch.rand((N, F), generator=g) * 6.28 - 3.14
    rot = torch.stack([torch.zeros_like(heading), torch.zeros_like(heading), torch.sin(heading / 2), torch.cos(heading / 2)], dim=-1)
    rot = rot + torch.randn((N, F, 4), generator=g) * 0.1
    rot = rot / rot.norm(dim=-1, keepdim=True)
    jr = torch.randn((N, F, 14, 4), generator=g) * 0.4
    jr[..., 3] = 1.0
    jr = jr / jr.norm(dim=-1, keepdim=True)
    contacts = (torch.rand((N, F, 15), generator=g) > 0.5).float()
    final = torch.tensor([w[2] if w else 0 for w in walks], dtype=torch.int32)
    for t in (pos, rot, jr, contacts):
        t[2] = t[0]
    final[2] = final[0]
    return pos.float(), rot.float(), jr.float(), contacts, final


def make_terrain(hf, min_point):
    t = terrain_util.SubTerrain(x_dim=hf.shape[0], y_dim=hf.shape[1], dx=DX, dy=DX, min_x=float(min_point[0]), min_y=float(min_point[1]), device="cpu")
    t.hf = torch.from_numpy(hf.copy())
    t.min_point = torch.from_numpy(np.asarray(min_point, np.float32).copy())
    return t


def check_bounds(xy, min_point):
    """Every padded bound lies >= 1e-3 cells from a rounding boundary (float64)."""
    xy = xy.double().numpy()
    for v, s in ((xy.min(0), -1.0), (xy.max(0), 1.0)):
        b = np.float32(np.float32(v) + np.float32(s * PADDING)).astype(np.float64)
        u = (b - min_point.astype(np.float64)) / float(np.float32(DX))
        d = np.abs(np.abs(u - np.floor(u)) - 0.5)
        assert (d >= 1e-3).all(), ("a padded bound lies within 1e-3 cells of a rounding boundary", v, u)


def main(out_dir=HERE):
    char = kcm.KinCharModel("cpu")
    char.load_char_file(os.path.join(REPO, "data/assets/humanoid.xml"))
    pts = geom_util.get_char_point_samples(char)
    flat = torch.cat(pts).numpy().astype(np.float32)              # the reference's own samples, as motion_terrain_*.npz keeps them
    body = np.concatenate([np.full(p.shape[0], b, np.int32) for b, p in enumerate(pts)])
    hfs, mps = scene()
    pos, rot, jr, contacts, final = rows()
    N = P * K
    out = dict(hfs=hfs, min_points=mps, dx=np.float32(DX), padding=np.float32(PADDING), w_contact=np.float32(W_CONTACT), w_pen=np.float32(W_PEN),
               penalty=np.float32(PENALTY), root_pos=pos.numpy(), root_rot=rot.numpy(), joint_rot=jr.numpy(), contacts=contacts.numpy().astype(np.uint8),
               points=flat, point_body=body, final_frame=final.numpy(), noise=np.asarray(NOISE, np.float32), candidates=np.int32(K),
               thresholds=np.asarray([THRESHOLDS["max_contact_loss"], THRESHOLDS["max_pen_loss"], THRESHOLDS["max_total_loss"]], np.float32))
    for mode, sliced in (("s", True), ("w", False)):
        contact, pen, total, minp, dims, packed = [], [], [], [], [], []
        for i in range(N):
            terrain = make_terrain(hfs[i // K], mps[i // K])
            sl = slice(0, int(final[i]))                            # mdm_path.py:393
            mf = motion_util.MotionFrames(root_pos=pos[i:i + 1, sl], root_rot=rot[i:i + 1, sl], joint_rot=jr[i:i + 1, sl], body_pos=None, body_rot=None,
                                          contacts=contacts[i:i + 1, sl])
            if sliced:
                check_bounds(mf.root_pos[0, :, 0:2], mps[i // K])
                cur = terrain_util.slice_terrain_around_motion(mf.root_pos, terrain, padding=PADDING, localize=False)
                packed.append(cur.hf.numpy().astype(np.float32).reshape(-1))
            else:
                cur = terrain.torch_copy()
            with torch.no_grad():
                losses = ref_path.compute_motion_loss(mf, None, cur, char, pts, W_CONTACT, W_PEN, 1.0, verbose=False)
            t = losses["total_loss"]
            if final[i] < 0:                                        # :401
                t = t + PENALTY
            total.append(t.reshape(1)); contact.append(losses["contact_loss"].reshape(1)); pen.append(losses["pen_loss"].reshape(1))
            minp.append(cur.min_point.numpy().astype(np.float32)); dims.append(np.asarray(cur.hf.shape, np.int32))
        total, contact, pen = torch.cat(total).float(), torch.cat(contact).float(), torch.cat(pen).float()
        total = total + torch.tensor(NOISE)                         # :417 with the recorded noise
        order = []
        for p in range(P):
            t = total[p * K:(p + 1) * K]
            _, ids = torch.sort(t)                                  # :420
            assert torch.equal(ids, torch.sort(t, stable=True)[1]), "torch.sort did not keep the tie in row order"
            order.append(ids.numpy() + p * K)
            tv = t.double().numpy()
            for a in range(K):
                for b in range(a + 1, K):
                    if p == 0 and (a, b) == (0, 2):
                        assert tv[a] == tv[b], "the deliberate tie is no tie"
                        continue
                    assert abs(tv[a] - tv[b]) > 100 * TOL(max(abs(tv[a]), abs(tv[b]))), (mode, p, a, b, tv)
        th = out["thresholds"].astype(np.float64)
        for name, v, m in (("contact", contact, th[0]), ("pen", pen, th[1]), ("total", total, th[2])):
            d = np.abs(v.double().numpy() - m)
            assert (d > 100 * TOL(m)).all(), (mode, name, "a loss lies within 100 tolerances of its threshold", v)
        valid = (contact < THRESHOLDS["max_contact_loss"]) & (pen < THRESHOLDS["max_pen_loss"]) & (total < THRESHOLDS["max_total_loss"])   # parc_2_kin_gen.py:389
        print(mode, "contact", contact.numpy().round(4).tolist(), "\n  pen", pen.numpy().round(4).tolist(), "\n  total", total.numpy().round(4).tolist(),
              "\n  order", np.concatenate(order).tolist(), "valid", valid.int().tolist(), "dims", [d.tolist() for d in dims])
        assert valid.any() and not valid.all(), (mode, "the thresholds split nothing")
        out.update({f"{mode}/contact": contact.numpy(), f"{mode}/pen": pen.numpy(), f"{mode}/total": total.numpy(), f"{mode}/order": np.concatenate(order).astype(np.int32),
                    f"{mode}/valid": valid.numpy(), f"{mode}/min_point": np.stack(minp), f"{mode}/dims": np.stack(dims)})
        if sliced:
            out["s/hf"] = np.concatenate(packed)
            d = np.stack(dims)
            assert (d[4] > np.array([24, 20])).all(), "row 4's slice is not larger than its terrain"
            assert np.array_equal(packed[0], packed[2])
    path_out = os.path.join(out_dir, "mdm_select.npz")
    np.savez_compressed(path_out, **out)
    limit = os.path.getsize(os.path.join(HERE, "mdm_path.npz"))
    print("mdm_select.npz", os.path.getsize(path_out), "bytes (mdm_path.npz:", limit, ")")
    assert os.path.getsize(path_out) <= limit


if __name__ == "__main__":
    main(*sys.argv[1:2])
