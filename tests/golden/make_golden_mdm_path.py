#!/usr/bin/env python3
"""Generate ``mdm_path.npz`` from the REAL reference: ``gen_util.gen_mdm_motion`` (RELATIVE_TO_ROOT) and
``mdm_path.generate_frames_until_end_of_path`` driven on the CPU with the small model of ``mdm_weights.npz`` (``make_golden_mdm.py``'s
``default`` shape: the same stubs, the same seed, so the same weights; asserted).

    python tests/golden/make_golden_mdm_path.py

Everything is computed twice, in fp32 and in float64 (model, character, terrain, paths and frames in double; the local grid stays the
float32 linspace it is in the reference).  A float tensor is stored as the float64 values in fixed point (``name_q28``, steps of 2^-28)
beside the largest fp32-vs-float64 difference (``name_err32``); heights, node indices, flags and frame counts must agree exactly between
the two runs and are stored once.  Tensors behind exp-map round trips must agree to 1e-4 (another seed otherwise, never a wider bound).

Scene ``steps``: one 24 x 20 terrain at dx 0.4 of three 8 x 20-cell plateaus, a 12-node path, 6 rows (one path, six candidates).  Record ``limit``: blank
start, guidance on, the time limit ends the rollout after exactly 3 windows (x_T seed 215, the first whose rollout meets the boundary
condition below).  Scene ``flat``: the same grid at one height, where that condition holds everywhere.  Records ``mixed`` and ``alldone``
run on it with given previous frames (the rest pose) and guidance off, so every window takes its clean previous state back.  The first
window reads nodes 0 and 1 only; the script runs it, then lays the path's last node under row 0's feet as the second window will see
them.  In ``mixed`` rows 0 .. 2 start together and are done at the second window (``final_frame`` 16), rows 3 .. 5 start 2.5 m away and
never are.  In ``alldone`` every row gets the same x_T, so all are done at once: the all-done exit, where ``final_frame`` stays -1 for
all, as the reference leaves it.  Record ``nodes``: one conditions-only window of ``generate_frames_along_path`` on an 80-node path
(more nodes than a wave has lanes): rows at the start, on a tie between nodes 30 and 31, past node 64, where the lookahead is clamped,
on the last node (done) and 29.5 m beside the path.  Per window: the world
previous frames, the captured conditions, closest / target node, done, x_T, the returned world frames; at the end the concatenated
frames, ``final_frame``, and the selection (losses per row, the injected loss noise, the sorted order).
Every heightfield sample within 1e-3 cells of a cell boundary must have equal heights on both sides (asserted in float64), so one ulp
of sin / cos / atan2 cannot change a height of this scene, and fp32 must reproduce the float64 heights exactly.

Scene ``rough``: a 9 x 13 terrain with every cell at another height, min_point off the origin, 6 rows at headings 0, pi/2, pi - 5e-4,
-2.2, 0.7, 1.9; the last row is 300 m away on the same terrain moved along.  Conditions only.  Per sample the float64 distance to the
nearest cell boundary is stored; fp32 may differ from float64 only at samples nearer than 1e-4 cells, at most 0.5 % of a row (asserted).

It also checks the RELATIVE_TO_ROOT_FLOOR branch of the reference (gen_util.py:72-79) and prints what it finds.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_mdm as G  # noqa: E402  (the module stubs, the parc alias, build())

import numpy as np  # noqa: E402
import torch  # noqa: E402

import parc.motion_generator.gen_util as gen_util  # noqa: E402
import parc.motion_synthesis.procgen.mdm_path as ref_path  # noqa: E402
import parc.util.motion_util as motion_util  # noqa: E402
import parc.util.terrain_util as terrain_util  # noqa: E402
from parc.motion_generator.diffusion_util import MDMFrameType, MDMKeyType, RelativeZStyle  # noqa: E402

from parc_amd import motion_opt as mo  # noqa: E402


def _icosphere(subdivisions=0, radius=1.0):                        # the one trimesh call of the point sampler, as make_golden_motion_terrain.py stubs it
    import types
    assert subdivisions == 0
    return types.SimpleNamespace(vertices=mo.icosahedron_vertices() * radius)


sys.modules["trimesh.creation"].icosphere = _icosphere

N = 6
LIMIT_SEED = 215                                                   # x_T of the limit record: the first seed whose rollout keeps every sample 1e-3 cells from a step
STRIDE = 10
REL_HEIGHT = 0.8125
LOSS_NOISE = [0.25, -0.5, 1.0, -1.25, 0.625, -0.125]
FRAME_KEYS = ("root_pos", "root_rot", "joint_rot", "contacts")


def steps_scene():
    """24 x 20 cells, plateaus at three levels within +-1 m; a 12-node path, nodes 0.5 m apart, across the plateaus."""
    # three plateaus of 8 x 20 cells: two step lines only, so that a rollout whose every sample keeps 1e-3 cells from a step exists
    levels = np.array([[0.0], [0.5], [-0.25]], np.float32)
    hf = np.kron(levels, np.ones((8, 20), np.float32)).astype(np.float32)
    assert hf.shape == (24, 20)
    min_point = np.array([-4.5, -3.75], np.float32)
    dx = 0.4
    xy = np.stack([-3.263 + 0.48 * np.arange(12), -2.1 + 0.14 * np.arange(12)], axis=-1).astype(np.float32)
    ind = np.clip(np.round((xy - min_point) / np.float32(dx)).astype(int), 0, [23, 19])
    path = np.concatenate([xy, hf[ind[:, 0], ind[:, 1]][:, None]], axis=-1).astype(np.float32)
    d = np.linalg.norm(np.diff(xy, axis=0), axis=-1)
    assert (d > 0.4).all() and (d < 0.6).all()
    return hf, min_point, dx, path


def flat_scene():
    """24 x 20 cells at 0.25 m (no step: the boundary condition holds everywhere); a four-node path, nodes 0.5 m apart."""
    hf = np.full((24, 20), 0.25, np.float32)
    path = np.stack([-1.0 + 0.5 * np.arange(4), np.full(4, -1.0), np.full(4, 0.25)], axis=-1).astype(np.float32)
    return hf, np.array([-4.5, -3.75], np.float32), path


def standing(path, at, lateral=None, height=0.85):
    """Previous frames [N, 2, ...] of the rest pose, row r over node at[r] (plus ``lateral`` [N, 2]), heading along +x."""
    n = len(at)
    pos = torch.zeros((n, 2, 3))
    pos[:, :, :] = torch.from_numpy(np.asarray(path, np.float32)[np.asarray(at)])[:, None, :]
    pos[:, :, 2] += height
    if lateral is not None:
        pos[:, :, 0:2] += torch.as_tensor(lateral, dtype=torch.float32)[:, None, :]
    rot = torch.zeros((n, 2, 4))
    rot[..., 3] = 1
    jr = torch.zeros((n, 2, 14, 4))
    jr[..., 3] = 1
    return dict(root_pos=pos, root_rot=rot, joint_rot=jr, contacts=torch.zeros((n, 2, 15)))


def nodes_record(m32, m64, out):
    """One conditions-only window of ``generate_frames_along_path`` on an 80-node path (more nodes than a wave has lanes): rows near the
    start, on a tie between nodes 30 and 31, past node 64, where the lookahead is clamped, on the last node (done) and far off the path."""
    hf, mp, _ = flat_scene()
    path = np.stack([-20.0 + 0.5 * np.arange(80), np.full(80, 0.5), np.full(80, 0.25)], axis=-1).astype(np.float32)
    lateral = np.array([[0.1, 0.1], [0.25, 0.0], [0.1, -0.2], [-0.05, 0.3], [0.0, 0.0], [0.0, 29.5]], np.float32)
    prev = standing(path, [0, 30, 66, 75, 79, 44], lateral)
    caps = {}
    for dtype, m in ((torch.float32, m32), (torch.float64, m64)):
        t = make_terrain(hf, mp, 0.4, dtype)
        pf = motion_util.MotionFrames(root_pos=prev["root_pos"].to(dtype), root_rot=prev["root_rot"].to(dtype), joint_rot=prev["joint_rot"].to(dtype), body_pos=None,
                                      body_rot=None, contacts=prev["contacts"].to(dtype))
        ps, gs = settings(10.0)
        with Capture(m, dtype, None) as cap, torch.no_grad():
            ref_path.generate_frames_along_path(pf, torch.from_numpy(path).to(dtype), t, m._kin_char_model, m, gs, ps, verbose=False)
        caps[dtype] = cap
    a, b = caps[torch.float32].windows[-1], caps[torch.float64].windows[-1]
    done, done32 = b["done"], a["done"]
    assert torch.equal(done, done32) and torch.equal(a["closest"], b["closest"])
    nodes = torch.from_numpy(path)
    tn = torch.argmin((nodes[None].double() - b["target_world"][:, None].double()).abs().sum(-1), dim=-1)
    assert torch.equal(nodes[tn].double(), b["target_world"].double())
    print("nodes: closest", b["closest"].tolist(), "target", tn.tolist(), "done", done.tolist())
    assert b["closest"].tolist() == [0, 30, 66, 75, 79, 44] and tn.tolist() == [7, 37, 73, 79, 79, 51] and done.tolist() == [False] * 4 + [True, False]
    out["nodes/path"] = path
    for k in FRAME_KEYS:
        out[f"nodes/prev_{k}"] = prev[k].numpy()
    out["nodes/closest_node"], out["nodes/target_node"], out["nodes/done"] = b["closest"].numpy().astype(np.int32), tn.numpy().astype(np.int32), done.numpy()
    out["nodes/hf_cell"] = cell_heights(a, b, np.unique(hf), "nodes")
    store(out, "nodes/target", a["target"], b["target"])
    for k in ("ROOT_POS", "ROOT_ROT", "JOINT_POS"):
        store(out, f"nodes/ps_{k}", a["prev_state"][k], b["prev_state"][k])


def rough_scene():
    g = np.random.default_rng(5)
    hf = (g.permutation(9 * 13).reshape(9, 13).astype(np.float32) / 64.0 - 0.9).astype(np.float32)   # every cell another height
    min_point = np.array([1.3, -2.7], np.float32)
    return hf, min_point, 0.4


def make_terrain(hf, min_point, dx, dtype):
    t = terrain_util.SubTerrain(x_dim=hf.shape[0], y_dim=hf.shape[1], dx=dx, dy=dx, min_x=float(min_point[0]), min_y=float(min_point[1]), device="cpu")
    t.hf = torch.from_numpy(hf.copy())
    t.min_point = torch.from_numpy(np.asarray(min_point, np.float32).copy())
    if dtype == torch.float64:
        t.hf, t.min_point, t.dxdy, t.hf_maxmin = t.hf.double(), t.min_point.double(), t.dxdy.double(), t.hf_maxmin.double()
    return t


class Capture:
    """Wraps the reference's functions for one rollout: what goes into and comes out of every window."""

    def __init__(self, m, dtype, x_T):
        self.m, self.dtype, self.x_T, self.windows = m, dtype, x_T, []
        self.full, self.rows, self.sort_in, self.sort_ids = None, [], None, None

    def __enter__(self):
        self.orig = dict(gen=gen_util.gen_mdm_motion, seq=self.m.gen_sequence, closest=ref_path.get_closest_path_node_idx, randn=torch.randn,
                         cat=motion_util.cat_motion_frames, loss=ref_path.compute_motion_loss, sort=torch.sort, randn_like=torch.randn_like,
                         blank=motion_util.MotionFrames.init_blank_frames, along=ref_path.generate_frames_along_path)
        cap, dtype = self, self.dtype

        def gen(target_world_pos, prev_frames, terrain, mdm_model, char_model, mdm_settings, target_dir=None):
            w = dict(prev={k: getattr(prev_frames, k).clone() for k in FRAME_KEYS}, target_world=target_world_pos.clone(), closest=cap.pending_closest)
            cap.pending_closest = None
            cap.windows.append(w)
            out = cap.orig["gen"](target_world_pos=target_world_pos, prev_frames=prev_frames, terrain=terrain, mdm_model=mdm_model, char_model=char_model,
                                  mdm_settings=mdm_settings, target_dir=target_dir)
            w["frames"] = {k: getattr(out, k).clone() for k in FRAME_KEYS}
            return out

        def seq(conds, ddim_stride=None, mode=None):
            w = cap.windows[-1]
            w["hf_z"] = conds[MDMKeyType.OBS_KEY].clone()
            w["target"] = conds[MDMKeyType.TARGET_KEY].clone()
            w["prev_state"] = {k.name: v.clone() for k, v in conds[MDMKeyType.PREV_STATE_KEY].items()}
            w["flags"] = torch.stack([conds[k].clone() for k in (MDMKeyType.OBS_FLAG_KEY, MDMKeyType.TARGET_FLAG_KEY, MDMKeyType.PREV_STATE_FLAG_KEY,
                                                                MDMKeyType.PREV_STATE_NOISE_IND_KEY)], dim=-1)
            w["guided"] = MDMKeyType.GUIDANCE_PARAMS in conds
            if cap.x_T is None:                                   # conditions only
                n = w["hf_z"].shape[0]
                z = lambda *s: torch.zeros((n, 15) + s, dtype=dtype)   # noqa: E731
                q = z(4); q[..., 3] = 1
                jq = z(14, 4); jq[..., 3] = 1
                return {MDMFrameType.ROOT_POS: z(3), MDMFrameType.ROOT_ROT: q, MDMFrameType.JOINT_ROT: jq, MDMFrameType.CONTACTS: z(15)}
            # gen_mdm_motion builds the flags with expand(batch_size); predict_x0 writes them in place under guidance, which this
            # torch refuses for a stride-0 tensor of more than one row: the same values, materialised
            for k in (MDMKeyType.OBS_FLAG_KEY, MDMKeyType.TARGET_FLAG_KEY, MDMKeyType.PREV_STATE_FLAG_KEY, MDMKeyType.PREV_STATE_NOISE_IND_KEY):
                conds[k] = conds[k].clone()
            x = cap.x_T[len(cap.windows) - 1]
            torch.randn = lambda *a, **kw: x.clone().to(dtype)
            try:
                return cap.orig["seq"](conds, ddim_stride, mode=mode) if mode is not None else cap.orig["seq"](conds, ddim_stride)
            finally:
                torch.randn = cap.orig["randn"]

        def along(*a, **kw):
            frames, done = cap.orig["along"](*a, **kw)
            cap.windows[-1]["done"] = done.clone()
            return frames, done

        def closest(root_pos, path_nodes_xyz):
            cap.pending_closest = cap.orig["closest"](root_pos, path_nodes_xyz).clone()
            return cap.pending_closest

        def cat(frames):
            cap.full = cap.orig["cat"](frames)
            cap.per_window = [f.root_pos.shape[1] for f in frames]
            return cap.full

        def loss(motion_frames, *a, **kw):
            a = list(a)
            a[3] = [p.to(dtype) for p in a[3]]                     # body_points: float32 whatever the model's dtype
            out = cap.orig["loss"](motion_frames, *a, **kw)
            cap.rows.append(dict(n=motion_frames.root_pos.shape[1], total=out["total_loss"].clone(), contact=out["contact_loss"].clone(), pen=out["pen_loss"].clone()))
            return out

        def sort(x, *a, **kw):
            r = cap.orig["sort"](x, *a, **kw)
            if cap.sort_in is None and cap.rows:
                cap.sort_in, cap.sort_ids = x.clone(), r[1].clone()
            return r

        def blank(self_, char_model, history_length, batch_size=1):
            cap.orig["blank"](self_, char_model, history_length, batch_size)
            for k in ("root_pos", "root_rot", "joint_rot", "body_pos", "body_rot", "contacts"):
                setattr(self_, k, getattr(self_, k).to(dtype))

        cap.pending_closest = None
        gen_util.gen_mdm_motion = gen
        self.m.gen_sequence = seq
        ref_path.get_closest_path_node_idx = closest
        ref_path.generate_frames_along_path = along
        motion_util.cat_motion_frames = cat
        ref_path.compute_motion_loss = loss
        torch.sort = sort
        torch.randn_like = lambda a, **kw: torch.tensor(LOSS_NOISE, dtype=a.dtype).reshape(a.shape)
        motion_util.MotionFrames.init_blank_frames = blank
        return self

    def __exit__(self, *exc):
        o = self.orig
        gen_util.gen_mdm_motion, ref_path.get_closest_path_node_idx, motion_util.cat_motion_frames = o["gen"], o["closest"], o["cat"]
        ref_path.compute_motion_loss, torch.sort, torch.randn_like, torch.randn = o["loss"], o["sort"], o["randn_like"], o["randn"]
        motion_util.MotionFrames.init_blank_frames, ref_path.generate_frames_along_path = o["blank"], o["along"]
        del self.m.gen_sequence


def settings(max_len, use_cfg=True):
    ps = ref_path.MDMPathSettings()
    ps.mdm_batch_size, ps.max_motion_length = N, max_len
    gs = gen_util.MDMGenSettings()
    gs.use_cfg = use_cfg
    return ps, gs


def x_noise(seed, windows, D):
    g = torch.Generator().manual_seed(1000 + seed)
    return (torch.randn((windows, N, 15, D), generator=g)).half().float()


def rollout(m, dtype, hf, min_point, dx, path, x_T, max_len, prev=None, use_cfg=True):
    import random
    terrain = make_terrain(hf, min_point, dx, dtype)
    nodes = torch.from_numpy(path.copy()).to(dtype)
    ps, gs = settings(max_len, use_cfg)
    pf = None
    if prev is not None:
        pf = motion_util.MotionFrames(root_pos=prev["root_pos"].to(dtype), root_rot=prev["root_rot"].to(dtype), joint_rot=prev["joint_rot"].to(dtype),
                                      body_pos=None, body_rot=None, contacts=prev["contacts"].to(dtype))
    orig_random = random.random
    random.random = lambda: (REL_HEIGHT - 0.7) / (0.9 - 0.7)
    try:
        with Capture(m, dtype, x_T) as cap, torch.no_grad():
            import contextlib
            import io
            with contextlib.redirect_stdout(io.StringIO()):
                ref_path.generate_frames_until_end_of_path(nodes, terrain, m._kin_char_model, m, pf, ps, gs, add_noise_to_loss=True, verbose=False,
                                                           slice_terrain=False, first_heading_mode="auto")
    finally:
        random.random = orig_random
    return cap


def cell_heights(a, b, hf_all, what):
    """The terrain heights the window sampled (hf_z plus the canonical z), as the terrain's own fp32 values; the fp32 run must have
    sampled the same cells."""
    h64 = b["hf_z"].double() + b["prev"]["root_pos"][:, -1, 2].double()[:, None, None]
    h32 = a["hf_z"].double() + a["prev"]["root_pos"][:, -1, 2].double()[:, None, None]
    cell = h64.float().numpy()
    at = np.abs(cell[..., None] - hf_all[None, None, None, :]).argmin(-1)
    assert np.abs(cell - hf_all[at]).max() < 1e-6, what
    assert np.abs(h32.numpy() - hf_all[at]).max() < 1e-4, (what, "the fp32 run sampled other cells than float64")
    return hf_all[at].astype(np.float32)


def pack_rollout(name, c32, c64, out, path, x_T, hf_all):
    """One rollout's record under ``name/``; the integer outputs are asserted equal between the two runs."""
    assert len(c32.windows) == len(c64.windows) and c32.per_window == c64.per_window, name
    W = len(c64.windows)
    put = lambda k, a32, a64: store(out, f"{name}/{k}", a32, a64)   # noqa: E731
    nodes = torch.from_numpy(path)
    for w in range(W):
        a, b = c32.windows[w], c64.windows[w]
        for k in FRAME_KEYS[:3]:
            put(f"w{w}/prev_{k}", a["prev"][k], b["prev"][k])
            put(f"w{w}/out_{k}", a["frames"][k], b["frames"][k])
        out[f"{name}/w{w}/prev_contacts"] = b["prev"]["contacts"].float().numpy()
        put(f"w{w}/out_contacts", a["frames"]["contacts"], b["frames"]["contacts"])
        out[f"{name}/w{w}/hf_cell"] = cell_heights(a, b, hf_all, (name, w))
        put(f"w{w}/target", a["target"], b["target"])
        for k in ("ROOT_POS", "ROOT_ROT", "JOINT_POS"):
            put(f"w{w}/ps_{k}", a["prev_state"][k], b["prev_state"][k])
        assert torch.equal(a["flags"], b["flags"]) and a["guided"] == b["guided"]
        out[f"{name}/w{w}/flags"] = b["flags"].numpy()
        out[f"{name}/w{w}/guided"] = np.bool_(b["guided"])
        tn = torch.argmin((nodes[None, :, :].double() - b["target_world"][:, None, :].double()).abs().sum(-1), dim=-1)
        assert torch.equal(nodes[tn].double(), b["target_world"].double())
        out[f"{name}/w{w}/target_node"] = tn.expand(N).numpy().astype(np.int32) if tn.numel() == 1 else tn.numpy().astype(np.int32)
        if "done" in b:
            assert torch.equal(a["done"], b["done"])
            out[f"{name}/w{w}/done"] = b["done"].numpy()
        if b["closest"] is not None:
            assert torch.equal(a["closest"], b["closest"])
            out[f"{name}/w{w}/closest_node"] = b["closest"].numpy().astype(np.int32)
    for k in FRAME_KEYS:
        put(f"frames_{k}", getattr(c32.full, k), getattr(c64.full, k))
    out[f"{name}/frames_per_window"] = np.asarray(c64.per_window, np.int32)
    out[f"{name}/x_T"] = x_T[:W].numpy().astype(np.float16)
    out[f"{name}/path"] = path
    # final_frame from the slices the selection scored: a row's slice is frames[0:final_frame]; a penalised row never finished
    F = c64.full.root_pos.shape[1]
    final = []
    for cap in (c32, c64):
        raw = torch.cat([r["total"].reshape(1) for r in cap.rows]).double()
        pen = (cap.sort_in.double().reshape(-1) - raw - torch.tensor(LOSS_NOISE).double()) > 50.0
        lens = torch.tensor([r["n"] for r in cap.rows])
        ff = torch.where(pen, torch.full_like(lens, -1), lens)
        assert torch.equal(lens[pen], torch.full_like(lens[pen], F - 1))
        final.append(ff)
    assert torch.equal(final[0], final[1]), (name, final)
    out[f"{name}/final_frame"] = final[1].numpy().astype(np.int32)
    return final[1]


def store(out, key, a32, a64):
    v = a64.double().numpy()
    e = float(np.abs(a32.double().numpy() - v).max()) if v.size else 0.0
    assert e < 1e-4, (key, e, "pick another seed")
    assert np.abs(v).max() < 7.9, key
    out[key + "_q28"] = np.round(v * 2.0 ** 28).astype(np.int32)
    out[key + "_err32"] = np.float64(e)


def check_boundaries(m64, hf, min_point, dx, cap, name):
    """Every sample of every window within 1e-3 cells of a cell boundary has equal heights on both sides (float64)."""
    import parc.util.geom_util as geom_util
    import parc.util.torch_util as torch_util
    g = geom_util.get_xy_grid_points(torch.zeros(2), m64._dx, m64._dy, m64._num_x_neg, m64._num_x_pos, m64._num_y_neg, m64._num_y_pos)
    H = torch.from_numpy(hf).double()
    dims = torch.tensor(hf.shape)
    worst = 1.0
    for w in cap.windows:
        rp, rr = w["prev"]["root_pos"][:, -1:].double(), w["prev"]["root_rot"][:, -1:].double()
        heading = torch_util.calc_heading(rr)
        pts = torch_util.rotate_2d_vec(g.unsqueeze(0), heading.unsqueeze(-1)) + rp[:, :, None, 0:2]
        u = (pts - torch.from_numpy(min_point).double()) / torch.tensor([np.float32(dx), np.float32(dx)]).double()
        for s in (-1e-3, 1e-3):
            for ax in (0, 1):
                v = u.clone()
                v[..., ax] += s
                i0 = torch.clamp(torch.round(u).long(), torch.zeros_like(dims), dims - 1)
                i1 = torch.clamp(torch.round(v).long(), torch.zeros_like(dims), dims - 1)
                assert torch.equal(H[i0[..., 0], i0[..., 1]], H[i1[..., 0], i1[..., 1]]), (name, "a sample lies within 1e-3 cells of a step: another seed / offset")
        worst = min(worst, float((0.5 - (u - torch.round(u)).abs()).abs().min()))
    return worst


def floor_branch_check(m32):
    """RELATIVE_TO_ROOT_FLOOR (gen_util.py:72-79): what terrain.get_hf_val does with the [B, 1, 2] index."""
    hf, mp, dx = rough_scene()
    t = make_terrain(hf, mp, dx, torch.float32)
    xy = torch.tensor([[[2.0, -1.0]], [[3.5, 0.5]], [[2.9, 1.1]]])
    ind = t.get_grid_index(xy)
    want = t.hf[ind[:, 0, 0], ind[:, 0, 1]]
    try:
        got = t.get_hf_val(ind)
        ok = got.shape == want.shape and torch.equal(got.reshape(-1), want)
        print("RELATIVE_TO_ROOT_FLOOR: get_hf_val(ind [3, 1, 2]) returns shape", tuple(got.shape), "- the heights under the roots:", ok,
              "(it indexes hf[ind[0], ind[1]]: rows 0 and 1 of the batch taken as the x and y index arrays)")
    except Exception as ex:  # noqa: BLE001
        print("RELATIVE_TO_ROOT_FLOOR: get_hf_val raises", type(ex).__name__, ex)
    try:
        t.get_hf_val(t.get_grid_index(xy[:1]))
        print("RELATIVE_TO_ROOT_FLOOR: B = 1 does not raise")
    except Exception as ex:  # noqa: BLE001
        print("RELATIVE_TO_ROOT_FLOOR: B = 1 raises", type(ex).__name__)


def rough_record(m32, m64, out):
    hf, mp, dx = rough_scene()
    headings = [0.0, float(np.pi / 2), float(np.pi - 5e-4), -2.2, 0.7, 1.9]
    g = torch.Generator().manual_seed(77)
    J = 14
    jr = torch.randn((N, 2, J, 4), generator=g) * 0.3
    jr[..., 3] = 1.0
    jr = (jr / jr.norm(dim=-1, keepdim=True)).float()
    tilt = torch.randn((N, 2, 4), generator=g) * 0.1
    pos = torch.zeros((N, 2, 3))
    pos[:, :, 0] = mp[0] + 0.4 * 4 + torch.rand((N, 1), generator=g) * 1.2
    pos[:, :, 1] = mp[1] + 0.4 * 6 + torch.rand((N, 1), generator=g) * 1.2
    pos[:, :, 2] = 0.9 + torch.rand((N, 2), generator=g) * 0.2
    pos[:, 0, 0:2] -= 0.05
    off = np.array([300.0, -300.0], np.float32)
    pos[N - 1, :, 0:2] += torch.from_numpy(off)
    pos = pos.float()
    rr = []
    for i, h in enumerate(headings):
        q = torch.tensor([0.0, 0.0, np.sin(h / 2), np.cos(h / 2)]).float().expand(2, 4) + tilt[i] * torch.tensor([1.0, 1.0, 0.0, 0.0])
        rr.append(q / q.norm(dim=-1, keepdim=True))
    rr = torch.stack(rr).float()
    contacts = (torch.rand((N, 2, J + 1), generator=g) > 0.5).float()
    targets = pos[:, -1].clone()
    targets[:, 0:2] += torch.randn((N, 2), generator=g)
    targets[1, 0:2] = pos[1, -1, 0:2]                              # a zero target vector stays zero
    targets = targets.float()
    prev = dict(root_pos=pos, root_rot=rr, joint_rot=jr, contacts=contacts)
    res = {}
    for dtype, m in ((torch.float32, m32), (torch.float64, m64)):
        wins = []
        for rows, shift in ((slice(0, N - 1), np.zeros(2, np.float32)), (slice(N - 1, N), off)):
            t = make_terrain(hf, mp + shift, dx, dtype)
            pf = motion_util.MotionFrames(root_pos=pos[rows].to(dtype), root_rot=rr[rows].to(dtype), joint_rot=jr[rows].to(dtype), body_pos=None, body_rot=None,
                                          contacts=contacts[rows].to(dtype))
            with Capture(m, dtype, None) as cap, torch.no_grad():
                gen_util.gen_mdm_motion(target_world_pos=targets[rows].to(dtype), prev_frames=pf, terrain=t, mdm_model=m, char_model=m._kin_char_model,
                                        mdm_settings=gen_util.MDMGenSettings())
            wins.append(cap.windows[0])
        res[dtype] = {k: torch.cat([w[k] for w in wins]) for k in ("hf_z", "target")}
        res[dtype]["ps"] = {k: torch.cat([w["prev_state"][k] for w in wins]) for k in ("ROOT_POS", "ROOT_ROT", "JOINT_POS")}
    a, b = res[torch.float32], res[torch.float64]
    # the float64 distance of every sample to the nearest cell boundary, in cells
    import parc.util.geom_util as geom_util
    import parc.util.torch_util as torch_util
    gr = geom_util.get_xy_grid_points(torch.zeros(2), m64._dx, m64._dy, m64._num_x_neg, m64._num_x_pos, m64._num_y_neg, m64._num_y_pos)
    heading = torch_util.calc_heading(rr[:, -1:].double())
    pts = torch_util.rotate_2d_vec(gr.unsqueeze(0), heading.unsqueeze(-1)) + pos[:, -1:, None, 0:2].double()
    mps = torch.from_numpy(mp).double().expand(N, 2).clone()
    mps[N - 1] = torch.from_numpy(mp + off).double()             # the moved terrain's min_point is the fp32 sum
    u = (pts - mps[:, None, None, :]) / torch.tensor([np.float32(dx), np.float32(dx)]).double()
    dist = (0.5 - (u - torch.round(u)).abs()).abs().amin(dim=-1)
    diff = (a["hf_z"].double() - b["hf_z"].double()).abs() > 1e-4   # another cell: the heights are at least 1 / 64 apart
    assert not (diff & (dist >= 1e-4)).any(), "fp32 differs from float64 away from a cell boundary"
    assert (diff.reshape(N, -1).sum(-1) <= 0.005 * 961).all(), diff.reshape(N, -1).sum(-1)
    print("rough: fp32 heights differing from float64 per row", diff.reshape(N, -1).sum(-1).tolist(), " samples under 1e-4 cells:",
          (dist < 1e-4).reshape(N, -1).sum(-1).tolist())
    out["rough/hf"], out["rough/min_point"], out["rough/dx"], out["rough/far_offset"] = hf, mp, np.float32(dx), off
    for k in FRAME_KEYS:
        out[f"rough/prev_{k}"] = prev[k].numpy()
    out["rough/targets"] = targets.numpy()
    out["rough/hf_z64"] = b["hf_z"].float().numpy()                # float64 heights are fp32 values minus an fp32 z: stored rounded, exact to 6e-8
    out["rough/boundary_dist"] = dist.float().numpy()
    store(out, "rough/target", a["target"], b["target"])
    for k in ("ROOT_POS", "ROOT_ROT", "JOINT_POS"):
        store(out, f"rough/ps_{k}", a["ps"][k], b["ps"][k])
    out["rough/hf_err32_far"] = np.float64((a["hf_z"][N - 1].double() - b["hf_z"][N - 1].double())[~diff[N - 1]].abs().max())


def main(out_dir=HERE):
    shape = G.SHAPES["default"]
    m32, cfg = G.build(torch.float32, shape)
    m64, _ = G.build(torch.float64, shape)
    w = np.load(os.path.join(HERE, "mdm_weights.npz"))
    for k, v in m32._denoise_model.state_dict().items():
        assert np.array_equal(w[k], v.numpy()), k + ": not the weights of mdm_weights.npz"
    assert np.array_equal(w["features_mean"], m32._mdm_features_mean.numpy())
    assert m32._relative_z_style == RelativeZStyle.RELATIVE_TO_ROOT and m32._sequence_fps == 30
    floor_branch_check(m32)
    D = m32._motion_frame_dof
    hf, mp, dx, path = steps_scene()
    out = {"steps/hf": hf, "steps/min_point": mp, "steps/dx": np.float32(dx), "rel_height": np.float32(REL_HEIGHT), "loss_noise": np.asarray(LOSS_NOISE, np.float32),
           "stride": np.int32(STRIDE), "max_motion_length": np.float32(0.6)}
    # limit: blank start on the steps scene, guidance on, the time limit ends it.  mixed / alldone: the flat scene, a four-node path, given
    # previous frames that stand over the last node (rows 0 .. 2, or all) or over node 0, guidance off (every window takes the clean
    # previous state back)
    fhf, fmp, fpath = flat_scene()
    out.update({"flat/hf": fhf, "flat/min_point": fmp})
    away = np.array([[0.0, 0.0]] * 3 + [[-2.5, 0.5]] * 3, np.float32)
    x_same = x_noise(2, 3, D)
    x_same[:] = x_same[:, :1]                                      # alldone: every row the same noise, so every row the same motion
    starts = {"mixed": (standing(fpath, [0] * 6, away), x_noise(1, 3, D)), "alldone": (standing(fpath, [0] * 6), x_same)}
    done_paths = {}
    for name, (prev, x_T) in starts.items():
        # the first window reads nodes 0 and 1 only: run it, then lay the last node under row 0's feet as the second window will see them
        c = rollout(m64, torch.float64, fhf, fmp, dx, fpath, x_T, 0.6, prev, False)
        p1 = c.windows[1]["prev"]
        kin = m64._kin_char_model
        body, _ = kin.forward_kinematics(p1["root_pos"][:, -1].double(), p1["root_rot"][:, -1].double(), p1["joint_rot"][:, -1].double())
        feet = (body[:, kin.get_body_id("left_foot")] + body[:, kin.get_body_id("right_foot")]) / 2.0
        q = fpath.copy()
        q[3] = feet[0].float().numpy()
        q[2] = (q[1] + q[3]) / 2
        print(name, "feet after the first window", feet.numpy().round(3).tolist())
        done_paths[name] = q
    for name, (h_, mp_, p_, prev, cfg_on, x_T, want) in {
            "limit": (hf, mp, path, None, True, x_noise(LIMIT_SEED, 3, D), lambda ff, W, c: W == 3),
            "mixed": (fhf, fmp, done_paths["mixed"], starts["mixed"][0], False, starts["mixed"][1], lambda ff, W, c: W == 3 and (ff >= 0).any() and (ff < 0).any()),
            "alldone": (fhf, fmp, done_paths["alldone"], starts["alldone"][0], False, starts["alldone"][1],
                        lambda ff, W, c: W == 2 and (ff == -1).all() and bool(c.windows[1]["done"].all()))}.items():
        c64 = rollout(m64, torch.float64, h_, mp_, dx, p_, x_T, 0.6, prev, cfg_on)
        check_boundaries(m64, h_, mp_, dx, c64, name)
        c32 = rollout(m32, torch.float32, h_, mp_, dx, p_, x_T, 0.6, prev, cfg_on)
        sub = {}
        final = pack_rollout(name, c32, c64, sub, p_, x_T, np.unique(h_))
        W = len(c64.windows)
        print(name, "windows", W, "frames per window", c64.per_window, "final_frame", final.tolist(), "done", [w["done"].tolist() for w in c64.windows[1:]])
        assert want(final.numpy(), W, c64), name + ": not the record it is meant to be"
        out.update(sub)
        out[f"{name}/scene"] = np.frombuffer(("steps" if h_ is hf else "flat").encode(), np.uint8)
        out[f"{name}/use_cfg"], out[f"{name}/blank"] = np.bool_(cfg_on), np.bool_(prev is None)
        tot = c32.sort_in.reshape(-1).float().numpy()                  # the selection (slice_terrain=False), fp32: the reference's own precision
        assert np.abs(np.diff(np.sort(tot))).min() > 1e-3, "two totals closer than 1e-3: other loss noise"
        out[f"{name}/sel_total"] = tot
        out[f"{name}/sel_contact"] = torch.cat([r["contact"].reshape(1) for r in c32.rows]).float().numpy()
        out[f"{name}/sel_pen"] = torch.cat([r["pen"].reshape(1) for r in c32.rows]).float().numpy()
        out[f"{name}/sel_order"] = c32.sort_ids.reshape(-1).numpy().astype(np.int32)
        assert torch.equal(c32.sort_ids, c64.sort_ids)
    nodes_record(m32, m64, out)
    rough_record(m32, m64, out)
    path_out = os.path.join(out_dir, "mdm_path.npz")
    np.savez_compressed(path_out, **out)
    print("mdm_path.npz", os.path.getsize(path_out), "bytes (mdm_weights.npz:", os.path.getsize(os.path.join(HERE, "mdm_weights.npz")), ")")
    assert os.path.getsize(path_out) < os.path.getsize(os.path.join(HERE, "mdm_weights.npz"))


if __name__ == "__main__":
    main(*sys.argv[1:2])
