"""CPU restatement of the motion generator's inference (the MDM denoiser, the diffusion-rate tables, ``project_dofs`` and both sampling
loops) on ``torch.nn.functional``, from the same state dict the HIP path loads.  It works in the dtype of the tensors it is given
(float32, or float64 as the yardstick).  The attention is the plain definition: packed in-projection, scores / sqrt(head_dim), masked
keys at -inf, softmax, out-projection.  The elementwise rotation conversions are the package's torch helpers (they run outside the
kernels); forward kinematics and the quaternion products are written here.

Conditions are a dict in the network's units: ``hf`` [B, 31, 31] (heights / max_h), ``target`` [B, 2], ``prev`` [B, nprev, D]
(standardised), ``obs_flag`` / ``target_flag`` / ``prev_flag`` / ``ind`` [B] bool, ``scale`` (guidance scale or None).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from parc_amd import motion_generator as mg
from parc_amd.char_model import CharModel

NC = 67   # time, 64 heightfield tokens, target, indicator


def rate_tables(timesteps):
    """The cosine schedule and what the samplers read of it, fp32 on the CPU, every operation in the reference's order."""
    steps = torch.linspace(0, timesteps, timesteps + 1)
    cum = torch.cos(((steps / timesteps) + 0.008) / (1 + 0.008) * 3.1415927410125732 * 0.5) ** 2
    cum = cum / cum[0]
    betas = torch.clip(1 - (cum[1:] / cum[:-1]), 0.0001, 0.9999)
    alphas = 1. - betas
    prod = torch.cumprod(alphas, axis=0)
    prev = F.pad(prod[:-1], (1, 0), value=1.0)
    return {"betas": betas, "sqrt_alphas_cumprod": torch.sqrt(prod), "sqrt_one_minus_alphas_cumprod": torch.sqrt(1. - prod),
            "posterior_std": torch.sqrt(betas * (1. - prev) / (1. - prod)), "posterior_mean_coef1": torch.sqrt(prev) * betas / (1.0 - prod),
            "posterior_mean_coef2": (1. - prev) * torch.sqrt(alphas) / (1.0 - prod)}


def _qmul(a, b):
    ax, ay, az, aw = a.unbind(-1)
    bx, by, bz, bw = b.unbind(-1)
    return torch.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                        aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz], dim=-1)


def _qrot(q, v):
    qv = q[..., :3]
    t = 2 * torch.cross(qv, v, dim=-1)
    return v + q[..., 3:4] * t + torch.cross(qv, t, dim=-1)


class MdmRef:
    def __init__(self, cfg, state_dict, mean, std, dtype=torch.float32, device="cpu"):
        self.cfg, self.dtype, self.device = cfg, dtype, torch.device(device)
        self.sd = {k: v.detach().to(self.device, dtype) for k, v in state_dict.items()}
        self.cm = CharModel(mg._char_path(cfg))
        self.D = mg.frame_dim(self.cm)
        self.T, self.nprev, self.TS = cfg["seq_len"], cfg["num_prev_states"], cfg["diffusion_timesteps"]
        self.d, self.H, self.L = cfg["d_model"], cfg["num_heads"], cfg["num_layers"]
        self.mean = torch.as_tensor(np.asarray(mean)).to(self.device, dtype)[:self.T]
        self.std = torch.as_tensor(np.asarray(std)).to(self.device, dtype)[:self.T]
        self.rates = {k: v.to(self.device, dtype) for k, v in rate_tables(self.TS).items()}   # fp32 values, as the reference holds them
        B = self.cm.get_num_bodies()
        J, nd = B - 1, self.cm.get_dof_size()
        self.sl = {"pos": slice(0, 3), "rot": slice(3, 6), "jpos": slice(6, 6 + 3 * J), "jrot": slice(6 + 3 * J, 6 + 3 * J + nd),
                   "con": slice(6 + 3 * J + nd, self.D)}

    # ---- the network ----------------------------------------------------------------------------------------------------------------
    def _lin(self, key, x):
        return F.linear(x, self.sd[key + ".weight"], self.sd[key + ".bias"])

    def _mlp(self, prefix, n_hidden, x):
        for i in range(n_hidden):
            x = F.silu(self._lin(f"{prefix}.model.{3 * i}", x))
        return self._lin(f"{prefix}.model.{3 * n_hidden}", x)

    def embed_conds(self, c):
        """(tokens [B, 66, d]: heightfield, target, indicator; mask [B, 67 + T], True = the key is left out)"""
        n = c["hf"].shape[0]
        mask = torch.zeros((n, NC + self.T), dtype=torch.bool, device=self.device)
        h = c["hf"].to(self.dtype).reshape(n, 1, 31, 31)
        for i in (0, 2, 4, 6):
            h = F.leaky_relu(F.conv2d(h, self.sd[f"_obs_conv_net._net.{i}.weight"], self.sd[f"_obs_conv_net._net.{i}.bias"]), 0.01)
        tok = F.unfold(h, kernel_size=2, stride=2).permute(0, 2, 1)                       # [n, 64, 256]
        tok = self._lin("_obs_embed", tok) * c["obs_flag"].to(self.dtype)[:, None, None]
        mask[:, 1:65] = ~c["obs_flag"][:, None]
        tgt = self._mlp("_in_mlp_target", len(self.cfg["target_mlp_layers"]), c["target"].to(self.dtype).reshape(n, 1, 2))
        tgt = tgt * c["target_flag"].to(self.dtype)[:, None, None]
        mask[:, 65] = ~c["target_flag"]
        ind = self.sd["_embed_prev_state_noise_indicator.weight"][c["ind"].to(torch.int64)][:, None]
        mask[:, NC:NC + self.nprev] = ~c["prev_flag"][:, None]
        return torch.cat([tok, tgt, ind], dim=1), mask

    def fast_forward(self, x, c, t, tokens, mask):
        """x [B, T, D] is changed in place: its first nprev frames become the clean previous state where ``ind`` is set."""
        n = x.shape[0]
        tt = self._lin("_embed_t.time_embed.2", F.silu(self._lin("_embed_t.time_embed.0", self.sd["_embed_t.sequence_pos_encoder.pe"][0, t])))
        x[:, :self.nprev] = torch.where(c["ind"][:, None, None], c["prev"][:, :self.nprev].to(self.dtype), x[:, :self.nprev])
        frames = self._mlp("_in_mlp_gen_seq", len(self.cfg["in_mlp_layers"]), x)
        h = torch.cat([tt.expand(n, 1, self.d), tokens, frames], dim=1) + self.sd["_in_pos_encoding.pe"]
        hd = self.d // self.H
        for l in range(self.L):
            p = f"_transformer_encoder.layers.{l}."
            qkv = F.linear(h, self.sd[p + "self_attn.in_proj_weight"], self.sd[p + "self_attn.in_proj_bias"])
            q, k, v = [a.reshape(n, -1, self.H, hd).transpose(1, 2) for a in qkv.chunk(3, dim=-1)]
            s = (q @ k.transpose(-1, -2)) / math.sqrt(hd)
            s = s.masked_fill(mask[:, None, None, :], float("-inf"))
            a = (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(n, -1, self.d)
            h = F.layer_norm(h + self._lin(p + "self_attn.out_proj", a), (self.d,), self.sd[p + "norm1.weight"], self.sd[p + "norm1.bias"], 1e-5)
            ff = self._lin(p + "linear2", F.gelu(self._lin(p + "linear1", h)))
            h = F.layer_norm(h + ff, (self.d,), self.sd[p + "norm2.weight"], self.sd[p + "norm2.bias"], 1e-5)
        return self._mlp("_out_mlp", len(self.cfg["out_mlp_layers"]), h[:, NC:])

    def forward(self, x, c, t):
        tokens, mask = self.embed_conds(c)
        return self.fast_forward(x, c, t, tokens, mask)

    def predict_x0(self, x, c, t, tokens, mask):
        """With guidance the flags of ``c`` are left false, as the reference leaves them."""
        if c.get("scale") is None:
            return self.fast_forward(x, c, t, tokens, mask)
        c["ind"][:] = True
        c["prev_flag"][:] = True
        a = self.fast_forward(x, c, t, tokens, mask)
        c["ind"][:] = False
        c["prev_flag"][:] = False
        b = self.forward(x, c, t)
        return a + c["scale"] * (b - a)

    # ---- project_dofs ---------------------------------------------------------------------------------------------------------------
    def fk_positions(self, root_pos, root_q, jq):
        cm = self.cm
        pos, rot = [root_pos], [root_q]
        for j in range(1, cm.get_num_bodies()):
            p = int(cm._parent_indices[j])
            lt = torch.as_tensor(np.asarray(cm._local_translation[j]), dtype=self.dtype, device=self.device)
            lr = torch.as_tensor(np.asarray(cm._local_rotation[j]), dtype=self.dtype, device=self.device)
            pos.append(pos[p] + _qrot(rot[p], lt.expand_as(root_pos)))
            rot.append(_qmul(rot[p], _qmul(lr.expand_as(root_q), jq[..., j - 1, :])))
        return torch.stack(pos, dim=-2)

    def project_dofs(self, x):
        f = x * self.std + self.mean
        s = self.sl
        rq = mg.exp_map_to_quat(f[..., s["rot"]])
        jq = mg.joint_dof_to_rot(self.cm, f[..., s["jrot"]])
        body = self.fk_positions(f[..., s["pos"]], rq, jq)
        out = torch.cat([f[..., s["pos"]], mg.quat_to_exp_map(rq), body[..., 1:, :].reshape(x.shape[0], x.shape[1], -1),
                         mg.joint_rot_to_dof(self.cm, jq), torch.clamp(f[..., s["con"]], 0.0, 1.0)], dim=-1)
        return (out - self.mean) / self.std

    # ---- the loops ------------------------------------------------------------------------------------------------------------------
    def ddim(self, c, x_T, stride, timesteps=None):
        """Every x after a step, the last one the sample."""
        x = x_T.clone().to(self.dtype)
        tokens, mask = self.embed_conds(c)
        r, out = self.rates, []
        for t in (timesteps if timesteps is not None else reversed(range(0, self.TS, stride))):
            x0 = self.project_dofs(self.predict_x0(x, c, t, tokens, mask))
            if t == 0:
                x = x0
            else:
                nt = t - stride
                a, b = r["sqrt_alphas_cumprod"], r["sqrt_one_minus_alphas_cumprod"]
                c0 = a[nt] - (a[t] * b[nt]) / b[t]
                x = c0 * x0 + (b[nt] / b[t]) * x
            out.append(x.clone())
        return out

    def ddpm(self, c, x_T, step_noise, timesteps=None):
        x = x_T.clone().to(self.dtype)
        tokens, mask = self.embed_conds(c)
        r, out = self.rates, []
        for i, t in enumerate(timesteps if timesteps is not None else reversed(range(0, self.TS))):
            x0 = self.project_dofs(self.predict_x0(x, c, t, tokens, mask))
            if t == 0:
                x = x0
            else:
                x = r["posterior_mean_coef1"][t] * x0 + r["posterior_mean_coef2"][t] * x + r["posterior_std"][t] * step_noise[i].to(self.dtype)
            out.append(x.clone())
        return out

    def gen_sequence_features(self, c, x_T, stride, mode="DDIM", step_noise=None, timesteps=None):
        """The standardised [B, T, D] sequence ``gen_sequence`` extracts its components from."""
        prev = c["prev"].to(self.dtype)
        x = (self.ddim(c, x_T, stride, timesteps) if mode == "DDIM" else self.ddpm(c, x_T, step_noise, timesteps))[-1]
        return torch.cat([torch.where(c["ind"][:, None, None], prev[:, :self.nprev], x[:, :self.nprev]), x[:, self.nprev:]], dim=1)


def random_conds(n, T_prev, D, seed, flags=None):
    """Conditions from a seed; ``flags`` [n][4] (obs, target, prev, ind) or every combination cycled."""
    g = torch.Generator().manual_seed(seed)
    combos = [(1, 1, 1, 1), (0, 1, 1, 1), (1, 0, 1, 0), (1, 1, 0, 1), (0, 0, 0, 0), (1, 1, 1, 0)]
    fl = torch.tensor(flags if flags is not None else [combos[i % len(combos)] for i in range(n)], dtype=torch.bool)
    hf = torch.randn((n, 31, 31), generator=g) * 0.4
    hf[0, :3] = 1.0
    tgt = torch.randn((n, 2), generator=g)
    tgt = tgt / tgt.norm(dim=-1, keepdim=True)
    return {"hf": torch.clamp(hf, -1, 1), "target": tgt, "prev": torch.randn((n, T_prev, D), generator=g) * 0.5,
            "obs_flag": fl[:, 0].clone(), "target_flag": fl[:, 1].clone(), "prev_flag": fl[:, 2].clone(), "ind": fl[:, 3].clone(), "scale": None}


def copy_conds(c):
    return {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in c.items()}


def to_keys(c):
    """The dict of this module -> the MDMKeyType names ``MDMGenerator`` reads (network units)."""
    return {"OBS_KEY": c["hf"], "TARGET_KEY": c["target"], "PREV_STATE_KEY": c["prev"], "OBS_FLAG_KEY": c["obs_flag"], "TARGET_FLAG_KEY": c["target_flag"],
            "PREV_STATE_FLAG_KEY": c["prev_flag"], "PREV_STATE_NOISE_IND_KEY": c["ind"]}


# ---- the fixtures of tests/golden/make_golden_mdm.py ------------------------------------------------------------------------------------
class Fixture:
    """A record of the reference: the config, the state dict, the inputs, and per recorded tensor the reference's float64 values
    (``ref64[name]``, from fixed point) and the largest difference of the reference's own fp32 run from them (``err32[name]``).
    ``cases`` / ``weights`` name the files: ``mdm_cases.npz`` / ``mdm_weights.npz`` (the default shape), or one file for both, which
    holds its state dict under ``sd/`` keys (``mdm_edge.npz``)."""

    def __init__(self, golden_dir, cases="mdm_cases.npz", weights="mdm_weights.npz"):
        import json
        import os
        w = np.load(os.path.join(golden_dir, weights))
        c = np.load(os.path.join(golden_dir, cases))
        self.cfg = dict(json.loads(bytes(c["cfg_json"]).decode()), char_file="data/assets/humanoid.xml")
        self.mean, self.std = torch.from_numpy(w["features_mean"]), torch.from_numpy(w["features_std"])
        if weights == cases:
            self.sd = {k[3:]: torch.from_numpy(w[k]) for k in w.files if k.startswith("sd/")}
        else:
            self.sd = {k: torch.from_numpy(w[k]) for k in w.files if k not in ("features_mean", "features_std")}
        self.max_h, self.scale, self.stride = float(c["max_h"]), float(c["scale"]), int(c["stride"])
        self.timesteps = [int(t) for t in c["timesteps"]]
        self.hf_m, self.prev, self.x = [torch.from_numpy(c[k].astype(np.float32)) for k in ("hf_m", "prev", "x")]
        self.step_noise = torch.from_numpy(c["step_noise"].astype(np.float32)) if "step_noise" in c.files else None
        self.target, self.flags, self.mask = torch.from_numpy(c["target"]), torch.from_numpy(c["flags"]), torch.from_numpy(c["mask"])
        self.ref64 = {k[:-4]: torch.from_numpy(c[k].astype(np.float64) / 2.0 ** 28) for k in c.files if k.endswith("_q28")}
        self.err32 = {k[:-6]: float(c[k]) for k in c.files if k.endswith("_err32")}
        self.n = self.x.shape[0]
        self.rates = {k[6:]: torch.from_numpy(c[k]) for k in c.files if k.startswith("rates_")}   # the reference's DiffusionRates(21), fp32 (the default shape's file)

    def conds(self, scale=None):
        f = self.flags
        return {"hf": torch.clamp(self.hf_m, -self.max_h, self.max_h) / self.max_h, "target": self.target.clone(), "prev": self.prev.clone(),
                "obs_flag": f[:, 0].clone(), "target_flag": f[:, 1].clone(), "prev_flag": f[:, 2].clone(), "ind": f[:, 3].clone(), "scale": scale}

    def x_after(self, forced):
        """x after a pass: the clean previous state where the indicator is set (everywhere under guidance)."""
        x = self.x.clone()
        ind = torch.ones_like(self.flags[:, 3]) if forced else self.flags[:, 3]
        x[ind, :self.prev.shape[1]] = self.prev[ind]
        return x

    def as_recorded(self, xs, guided):
        """The x of every step as the reference's ``keep_all_samples`` list shows them: the list holds the very tensor that the next
        pass overwrites in place, so all but the last carry the clean previous state where that pass's indicator is set."""
        xs = torch.stack([x.clone() for x in xs])
        ind = torch.ones_like(self.flags[:, 3]) if guided else self.flags[:, 3]
        xs[:-1, ind, :self.prev.shape[1]] = self.prev[ind].to(xs.dtype)
        return xs
