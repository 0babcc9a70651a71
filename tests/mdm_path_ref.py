"""Torch restatement of path-following motion generation: the reference's world-frame wrapper of the generator
(``motion_generator/gen_util.py:27-153``, ``RELATIVE_TO_ROOT``) and its rollout along a path
(``motion_synthesis/procgen/mdm_path.py:129-383``), batched over rows that each have a terrain and a path of their own.  It works in the
dtype it is given (float32, or float64 as the yardstick) on any device.  The generation itself is a callable:
``generate(conds, window) -> component dict`` with ``conds`` keyed as ``MDMGenerator.gen_sequence`` reads them (heights in metres, the
previous state as a component dict, ``GUIDANCE_PARAMS`` the scale or None), so that the same code composes ``MDMGenerator.gen_sequence``
on the GPU and ``mdm_ref.MdmRef`` on the CPU.
"""
import numpy as np
import torch

from parc_amd import motion_generator as mg

FRAME_KEYS = ("root_pos", "root_rot", "joint_rot", "contacts")
DONE_RADIUS = 0.5


def qmul(a, b):
    """torch_util.quat_multiply (the factored product)."""
    x1, y1, z1, w1 = a.unbind(-1)
    x2, y2, z2, w2 = b.unbind(-1)
    ww = (z1 + x1) * (x2 + y2)
    yy = (w1 - y1) * (w2 + z2)
    zz = (w1 + y1) * (w2 - z2)
    xx = ww + yy + zz
    qq = 0.5 * (xx + (z1 - x1) * (x2 - y2))
    w = qq - ww + (z1 - y1) * (y2 - z2)
    x = qq - xx + (x1 + w1) * (x2 + w2)
    y = qq - yy + (w1 - x1) * (y2 + z2)
    z = qq - zz + (z1 + y1) * (w2 - x2)
    return torch.stack([x, y, z, w], dim=-1)


def qrot(q, v):
    qv = q[..., :3]
    t = 2 * torch.cross(qv, v, dim=-1)
    return v + q[..., 3:4] * t + torch.cross(qv, t, dim=-1)


def heading_quat(h):
    """axis_angle_to_quat((0, 0, 1), h) with its two normalisations."""
    half = h / 2
    z = torch.zeros_like(h)
    q = torch.stack([z * torch.sin(half), z * torch.sin(half), torch.sin(half), torch.cos(half)], dim=-1)
    return q / torch.clamp(torch.linalg.norm(q, dim=-1, keepdim=True), min=1e-9)


def calc_heading(q):
    ex = torch.zeros_like(q[..., :3])
    ex[..., 0] = 1
    d = qrot(q, ex)
    return torch.atan2(d[..., 1], d[..., 0])


def rotate_2d(v, a):
    c, s = torch.cos(a), torch.sin(a)
    return torch.stack([v[..., 0] * c - v[..., 1] * s, v[..., 0] * s + v[..., 1] * c], dim=-1)


class Scene:
    """Terrains [P, X, Y] (fp32 values) with min points [P, 2] and a cell size, one path per terrain, the row -> path map."""

    def __init__(self, hfs, min_points, dx, paths, row_path, dtype=torch.float32, device="cpu"):
        self.hfs = torch.as_tensor(np.asarray(hfs, np.float32)).to(device, dtype)
        self.min_points = torch.as_tensor(np.asarray(min_points, np.float32)).to(device, dtype)
        self.dxdy = torch.tensor([np.float32(dx), np.float32(dx)]).to(device, dtype)
        self.counts = torch.tensor([len(p) for p in paths], device=device)
        maxn = int(self.counts.max())
        nodes = np.zeros((len(paths), maxn, 3), np.float32)
        for i, p in enumerate(paths):
            nodes[i, :len(p)] = np.asarray(p, np.float32)
        self.nodes = torch.as_tensor(nodes).to(device, dtype)
        self.row_path = torch.as_tensor(np.asarray(row_path, np.int64)).to(device)
        self.N = int(self.row_path.numel())


class PathRef:
    def __init__(self, cfg, char_model, mean, std, path_settings, gen_settings, dtype=torch.float32, device="cpu"):
        self.cfg, self.cm, self.ps, self.gs, self.dtype, self.device = cfg, char_model, path_settings, gen_settings, dtype, torch.device(device)
        self.T, self.nprev = int(cfg["seq_len"]), int(cfg["num_prev_states"])
        self.mean = torch.as_tensor(np.asarray(mean)).to(self.device, dtype)[:self.T]
        self.std = torch.as_tensor(np.asarray(std)).to(self.device, dtype)[:self.T]
        hm = cfg["heightmap"]
        g, d = hm["local_grid"], hm["horizontal_scale"]
        self.max_h = float(hm["max_h"])
        # geom_util.get_xy_grid_points about a float32 zero centre: the local grid is float32 whatever the run's dtype
        zero = torch.zeros((2,), dtype=torch.float32)
        xs = torch.linspace(zero[0] - d * g["num_x_neg"], zero[0] + d * g["num_x_pos"], g["num_x_neg"] + g["num_x_pos"] + 1)
        ys = torch.linspace(zero[1] - d * g["num_y_neg"], zero[1] + d * g["num_y_pos"], g["num_y_neg"] + g["num_y_pos"] + 1)
        gx, gy = torch.meshgrid(xs, ys, indexing="ij")
        self.grid = torch.stack([gx, gy], dim=-1).to(self.device)
        self.fps = float(cfg.get("sequence_fps", 30))
        self.start = self.T - 1 - int(path_settings.rewind_num_frames)
        self.lf, self.rf = char_model.get_body_id("left_foot"), char_model.get_body_id("right_foot")

    # ---- kinematics -------------------------------------------------------------------------------------------------------------------
    def fk_positions(self, root_pos, root_q, jq):
        cm = self.cm
        pos, rot = [root_pos], [root_q]
        for j in range(1, cm.get_num_bodies()):
            p = int(cm._parent_indices[j])
            lt = torch.as_tensor(np.asarray(cm._local_translation[j]), dtype=self.dtype, device=self.device)
            lr = torch.as_tensor(np.asarray(cm._local_rotation[j]), dtype=self.dtype, device=self.device)
            pos.append(pos[p] + qrot(rot[p], lt.expand_as(root_pos)))
            rot.append(qmul(rot[p], qmul(lr.expand_as(root_q), jq[..., j - 1, :])))
        return torch.stack(pos, dim=-2)

    def blank_frames(self, scene, rel_height, heading=None):
        """mdm_path.py:150-165: identity frames at the origin, the last one at node 0 plus the relative root height, heading auto
        (``heading`` None) or given per path."""
        n, k, J = scene.N, self.nprev, self.cm.get_num_bodies() - 1
        z = lambda *s: torch.zeros(s, dtype=self.dtype, device=self.device)   # noqa: E731
        f = {"root_pos": z(n, k, 3), "root_rot": z(n, k, 4), "joint_rot": z(n, k, J, 4), "contacts": z(n, k, J + 1)}
        f["root_rot"][..., 3] = 1
        f["joint_rot"][..., 3] = 1
        n0, n1 = scene.nodes[:, 0], scene.nodes[:, 1]
        if heading is None:
            h = torch.atan2(n1[:, 1] - n0[:, 1], n1[:, 0] - n0[:, 0])
        else:
            h = torch.as_tensor(heading).to(self.device, self.dtype)
        rel = torch.as_tensor(rel_height).to(self.device, self.dtype)
        rp = scene.row_path
        f["root_pos"][:, -1, 0:2] = n0[rp, 0:2]
        f["root_pos"][:, -1, 2] = (n0[:, 2] + rel)[rp]
        f["root_rot"][:, -1] = heading_quat(h)[rp]
        return f

    # ---- gen_util.gen_mdm_motion up to the generator --------------------------------------------------------------------------------------
    def conds(self, scene, prev, first=False, blank=False):
        rp, rr = prev["root_pos"].to(self.dtype), prev["root_rot"].to(self.dtype)
        jr, ct = prev["joint_rot"].to(self.dtype), prev["contacts"].to(self.dtype)
        n, k = rp.shape[0], self.nprev
        sl = slice(k - 1, k)
        canon_xy = rp[:, sl, 0:2]
        heading = calc_heading(rr[:, sl])                          # [n, 1]
        hq, hqi = heading_quat(heading), heading_quat(-heading)
        root_pos = rp.clone()
        root_pos[..., 0:2] -= canon_xy
        root_pos = qrot(hqi.expand(n, k, 4), root_pos)
        root_rot = qmul(hqi.expand(n, k, 4), rr)
        canon_z = rp[:, sl, 2]
        root_pos[..., 2] -= canon_z
        pts = rotate_2d(self.grid.unsqueeze(0), heading.unsqueeze(-1)) + canon_xy.unsqueeze(1)      # [n, 31, 31, 2]
        pid = scene.row_path
        cell = torch.round((pts - scene.min_points[pid][:, None, None, :]) / scene.dxdy)
        dims = torch.tensor(scene.hfs.shape[1:], device=self.device)
        ind = torch.minimum(torch.maximum(cell.to(torch.int64), torch.zeros_like(dims)), dims - 1)
        hf_z = scene.hfs[pid[:, None, None], ind[..., 0], ind[..., 1]] - canon_z.unsqueeze(-1)
        edge = (cell - (pts - scene.min_points[pid][:, None, None, :]) / scene.dxdy).abs()           # 0.5 = on a cell boundary
        body = self.fk_positions(root_pos, root_rot, jr)
        # the target and the done flag (mdm_path.py:235-273)
        last_pos = rp[:, -1]
        nodes = scene.nodes[pid]                                   # [n, maxn, 3]
        counts = scene.counts[pid]
        d2 = torch.sum(torch.square(last_pos[:, None, 0:2] - nodes[..., 0:2]), dim=-1)
        d2 = torch.where(torch.arange(nodes.shape[1], device=self.device)[None] < counts[:, None], d2, torch.full_like(d2, float("inf")))
        closest = torch.argmin(d2, dim=-1)
        wbody = self.fk_positions(last_pos, rr[:, -1], jr[:, -1])
        feet = (wbody[:, self.lf] + wbody[:, self.rf]) / 2.0
        final = nodes[torch.arange(n, device=self.device), counts - 1]
        done = torch.linalg.norm(feet - final, dim=-1) < DONE_RADIUS
        tn = torch.ones_like(closest) if first else torch.clamp(closest + int(self.ps.next_node_lookahead), max=counts - 1)
        tw = nodes[torch.arange(n, device=self.device), tn]
        target = rotate_2d(tw[:, None, 0:2] - canon_xy, -heading)
        target = torch.nn.functional.normalize(target, dim=-1)
        gs = self.gs
        guided = bool(gs.use_cfg) and not (first and blank)
        ind_val = False if (first and blank) else (True if first else bool(gs.use_prev_state))
        flag = lambda v: torch.full((n,), bool(v), dtype=torch.bool, device=self.device)   # noqa: E731
        return {"OBS_KEY": hf_z, "OBS_FLAG_KEY": flag(True), "TARGET_KEY": target[:, 0], "TARGET_FLAG_KEY": flag(gs.target_condition_key),
                "PREV_STATE_KEY": {"ROOT_POS": root_pos[:, :k], "ROOT_ROT": root_rot[:, :k], "JOINT_POS": body[:, :k, 1:], "JOINT_ROT": jr[:, :k],
                                   "CONTACTS": ct[:, :k]},
                "PREV_STATE_NOISE_IND_KEY": flag(ind_val), "PREV_STATE_FLAG_KEY": flag(gs.prev_state_ind_key),
                "GUIDANCE_PARAMS": float(gs.cfg_scale) if guided else None,
                "closest_node": closest, "target_node": tn, "done": done, "canon_xy": canon_xy, "canon_z": canon_z, "heading": heading, "heading_quat": hq,
                "edge_dist": 0.5 - edge.amax(dim=-1)}

    GEN_KEYS = ("OBS_KEY", "OBS_FLAG_KEY", "TARGET_KEY", "TARGET_FLAG_KEY", "PREV_STATE_KEY", "PREV_STATE_NOISE_IND_KEY", "PREV_STATE_FLAG_KEY", "GUIDANCE_PARAMS")

    def features(self, comp):
        """assemble_mdm_features without the standardisation, in the run's dtype."""
        n0, n1 = comp["ROOT_POS"].shape[:2]
        return torch.cat([comp["ROOT_POS"], mg.quat_to_exp_map(comp["ROOT_ROT"]), comp["JOINT_POS"].reshape(n0, n1, -1),
                          mg.joint_rot_to_dof(self.cm, comp["JOINT_ROT"]), comp["CONTACTS"]], dim=-1)

    def network_units(self, c):
        """(heights clamped and divided by max_h, the previous state standardised): what the conditions kernel writes."""
        k = self.nprev
        return torch.clamp(c["OBS_KEY"], -self.max_h, self.max_h) / self.max_h, (self.features(c["PREV_STATE_KEY"]) - self.mean[:k]) / self.std[:k]

    def uncanon(self, out, c):
        """gen_util.py:131-151."""
        out = mg._names(out)
        n, t = out["ROOT_POS"].shape[:2]
        hq = c["heading_quat"].expand(n, t, 4)
        rot = qmul(hq, out["ROOT_ROT"].to(self.dtype))
        pos = qrot(hq, out["ROOT_POS"].to(self.dtype))
        pos = torch.cat([pos[..., 0:2] + c["canon_xy"], pos[..., 2:3] + c["canon_z"].unsqueeze(-1)], dim=-1)
        return {"root_pos": pos, "root_rot": rot, "joint_rot": out["JOINT_ROT"].to(self.dtype), "contacts": out["CONTACTS"].to(self.dtype)}

    def window(self, scene, prev, generate, w, first=False, blank=False):
        c = self.conds(scene, prev, first, blank)
        out = generate({k: c[k] for k in self.GEN_KEYS}, w)
        return self.uncanon(out, c), c

    # ---- mdm_path.generate_frames_until_end_of_path up to the selection -------------------------------------------------------------------
    def rollout(self, scene, generate, rel_height=None, heading=None, prev_frames=None, keep_windows=False):
        nprev, start, T = self.nprev, self.start, self.T
        blank = prev_frames is None
        prev = self.blank_frames(scene, rel_height, heading) if blank else prev_frames
        sl = lambda f, a, b: {k: v[:, a:b] for k, v in f.items()}   # noqa: E731
        windows = []
        gen, c = self.window(scene, prev, generate, 0, True, blank)
        windows.append(dict(prev=prev, conds=c, frames=gen))
        full = [sl(gen, 0, start)]
        total = start
        dt = 1.0 / self.fps
        final = torch.full((scene.N,), -1, dtype=torch.int64, device=self.device)
        found = torch.zeros((scene.N,), dtype=torch.bool, device=self.device)
        w = 0
        while True:
            w += 1
            prev = sl(gen, start - nprev, start)
            gen, c = self.window(scene, prev, generate, w)
            windows.append(dict(prev=prev, conds=c, frames=gen))
            done = c["done"]
            total += start - nprev
            if bool(torch.all(done)):
                full.append(sl(gen, nprev, T))
                break
            final[torch.logical_and(~found, done)] = total
            found = torch.logical_or(found, done)
            if total * dt > self.ps.max_motion_length:
                full.append(sl(gen, nprev, T))
                break
            full.append(sl(gen, nprev, start))
        frames = {k: torch.cat([f[k] for f in full], dim=1) for k in FRAME_KEYS}
        out = dict(frames=frames, final_frame=final, done=done, windows=w + 1, frames_per_window=[f["root_pos"].shape[1] for f in full],
                   num_frames=frames["root_pos"].shape[1])
        if keep_windows:
            out["window_records"] = windows
        return out


def mdm_ref_generate(ref, path_ref, x_T, stride, timesteps=None):
    """A ``generate`` callable on ``mdm_ref.MdmRef``: x_T [W, N, T, D] injected per window."""
    def generate(c, w):
        hf, prev = path_ref.network_units(c)
        nc = {"hf": hf, "target": c["TARGET_KEY"], "prev": prev, "obs_flag": c["OBS_FLAG_KEY"].clone(), "target_flag": c["TARGET_FLAG_KEY"].clone(),
              "prev_flag": c["PREV_STATE_FLAG_KEY"].clone(), "ind": c["PREV_STATE_NOISE_IND_KEY"].clone(), "scale": c["GUIDANCE_PARAMS"]}
        f = ref.gen_sequence_features(nc, x_T[w].to(ref.dtype), stride, "DDIM", timesteps=timesteps)
        f = f * ref.std + ref.mean
        s = ref.sl
        return {"ROOT_POS": f[..., s["pos"]], "ROOT_ROT": mg.exp_map_to_quat(f[..., s["rot"]]), "JOINT_ROT": mg.joint_dof_to_rot(ref.cm, f[..., s["jrot"]]),
                "CONTACTS": f[..., s["con"]]}
    return generate


# ---- the fixture of tests/golden/make_golden_mdm_path.py --------------------------------------------------------------------------------
class PathFixture:
    """``mdm_path.npz``: ``f64(key)`` the reference's float64 values (from fixed point), ``err32(key)`` the largest difference of the
    reference's own fp32 run from them, ``raw(key)`` what is stored as it is (heights, integers, inputs)."""
    RECORDS = ("limit", "mixed", "alldone")

    def __init__(self, golden_dir):
        import os
        self.z = np.load(os.path.join(golden_dir, "mdm_path.npz"))
        self.hf, self.min_point, self.dx = self.z["steps/hf"], self.z["steps/min_point"], float(self.z["steps/dx"])
        self.rel_height, self.loss_noise = float(self.z["rel_height"]), self.z["loss_noise"]
        self.stride, self.max_motion_length = int(self.z["stride"]), float(self.z["max_motion_length"])

    def f64(self, key):
        return torch.from_numpy(self.z[key + "_q28"].astype(np.float64) / 2.0 ** 28)

    def err32(self, key):
        return float(self.z[key + "_err32"])

    def raw(self, key):
        return self.z[key]

    def windows(self, rec):
        return len(self.z[f"{rec}/frames_per_window"])

    def prev(self, rec, w, dtype=torch.float64):
        d = {k: self.f64(f"{rec}/w{w}/prev_{k}").to(dtype) for k in FRAME_KEYS[:3]}
        d["contacts"] = torch.from_numpy(self.z[f"{rec}/w{w}/prev_contacts"]).to(dtype)
        return d

    def x_T(self, rec):
        return torch.from_numpy(self.z[f"{rec}/x_T"].astype(np.float32))

    def terrain(self, rec):
        """(hf, min_point) of the record's scene: ``steps`` or ``flat``."""
        name = bytes(self.z[f"{rec}/scene"]).decode() if f"{rec}/scene" in self.z.files else "flat"
        return self.z[f"{name}/hf"], self.z[f"{name}/min_point"]

    def blank(self, rec):
        return bool(self.z[f"{rec}/blank"])

    def use_cfg(self, rec):
        return bool(self.z[f"{rec}/use_cfg"])

    def start(self, rec, dtype=torch.float32, device="cpu"):
        """The previous frames the record's rollout was given (None: a blank start)."""
        return None if self.blank(rec) else {k: v.to(device) for k, v in self.prev(rec, 0, dtype).items()}

    def scene(self, rec, dtype=torch.float32, device="cpu", rows=None):
        n = 6 if rows is None else rows
        hf, mp = self.terrain(rec)
        return Scene(hf[None], mp[None], self.dx, [self.z[f"{rec}/path"]], [0] * n, dtype, device)
