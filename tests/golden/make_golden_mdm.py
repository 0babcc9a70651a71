#!/usr/bin/env python3
"""Generate the motion-generator fixtures from the REAL reference: ``mdm_weights.npz`` / ``mdm_cases.npz`` (shape ``default``) and
``mdm_edge.npz`` (shape ``edge``, weights and cases in one file).

Run where the reference checkout is available (the tests only read the fixtures it writes):

    python tests/golden/make_golden_mdm.py [default | edge]

Shape ``default``.  The reference's ``MDM`` / ``MDMTransformer`` are instantiated on the CPU as ``make_golden_motion_sampler.py`` drives its sampler (a
``parc`` package alias, empty module stubs) from the reference's default generator config at a small size: d_model 64, 4 heads, d_hid 64,
2 layers, MLP lists [32] / [64] / [64], 15 frames, 21 timesteps.  ``in_proj_weight`` is multiplied by 4 so that the attention is far from
uniform; the feature mean is random, the std in [0.5, 2].  Six rows cover every flag: heightfield off, target off, previous state masked,
the indicator on and off, heights beyond +-max_h.  Every tensor is computed twice, by the model in fp32 and by the same model in float64;
the file keeps the float64 values in fixed point (``name_q28``: int32 steps of 2^-28) and the largest fp32-vs-float64 difference of the
tensor (``name_err32``), the yardstick and the unit of the tests' bounds: embed_conds (tokens, mask), fast_forward at t = 10 and t = 0 with x after the call, predict_x0 with
guidance, project_dofs (of step_noise[0] / 4), ddim_inference and the steps of reverse_diffusion (denoise_one_timestep) at the timesteps [20, 10, 0] with injected x_T and noise (every
intermediate x), gen_sequence with and without guidance; and the reference's ``DiffusionRates`` tables (``rates_*``, fp32).  The script asserts that fp32 and float64 agree to 1e-4 on every tensor (an
exp-map round trip can sit on a branch cut: pick another SEED until it does).

Shape ``edge`` pins the restatement off that shape: d_model 32, 2 heads, d_hid 48 (not d_model), 2 layers, 20 frames (two row tiles of
frames), 3 previous states, MLP lists [] / [40, 24] / [24] (no hidden layer, two, one; widths that are no multiple of 16).  It records
the tokens and the mask, fast_forward at t = 20 (the last row of the timestep table) and t = 0, predict_x0 with guidance at t = 20 and
guided ddim_inference at [20, 10, 0] (every step), in the same format; its state dict is stored under ``sd/`` keys of the same file.
The tokenizer's convolutions alone are 310 KB of the file, so to stay under the size of ``mdm_weights.npz`` two of the computed tensors
are checked but not stored: fast_forward at t = 0 and predict_x0, whose arithmetic the loop's last and first step contain.
"""
import os
import sys
import types

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, REPO)
sys.dont_write_bytecode = True

for _name in ["trimesh", "trimesh.creation", "wandb", "gym", "gym.spaces", "isaacgym", "isaacgym.gymapi", "isaacgym.gymtorch", "isaacgym.gymutil"]:
    sys.modules[_name] = types.ModuleType(_name)
sys.modules["wandb"].run = None
sys.modules["trimesh"].creation = sys.modules["trimesh.creation"]
_parc = types.ModuleType("parc")
_parc.__path__ = [os.path.join(REF, "PARC")]
sys.modules["parc"] = _parc

import numpy as np  # noqa: E402
import torch  # noqa: E402
import yaml  # noqa: E402

import parc.util.path_loader as ref_path_loader  # noqa: E402

ref_path_loader.resolve_path = lambda p: p
import parc.motion_generator.mdm as ref_mdm  # noqa: E402
from parc.motion_generator.diffusion_util import MDMCustomGuidance, MDMFrameType, MDMKeyType  # noqa: E402

torch.set_num_threads(4)
SEED = 0
N = 6
TS3 = [20, 10, 0]
STRIDE = 10
SCALE = 1.5
# per shape: the overrides of the reference's default config, the two timesteps of fast_forward, the timestep of predict_x0, what is
# recorded beyond the network ("loops": project_dofs, both loops plain and guided, gen_sequence; "ddim_guided": that loop only)
SHAPES = {
    "default": dict(cfg=dict(seq_len=15, d_model=64, num_heads=4, d_hid=64, num_layers=2, target_mlp_layers=[32], in_mlp_layers=[64], out_mlp_layers=[64]),
                    forward_ts=(10, 0), guided_t=10, record="loops", seed=0),
    "edge": dict(cfg=dict(seq_len=20, num_prev_states=3, d_model=32, num_heads=2, d_hid=48, num_layers=2, target_mlp_layers=[], in_mlp_layers=[40, 24],
                          out_mlp_layers=[24]),
                 forward_ts=(20, 0), guided_t=20, record="ddim_guided", seed=0, drop=("forward_t0", "predict_x0")),
}
FLAGS = [(1, 1, 1, 1), (0, 1, 1, 1), (1, 0, 1, 0), (1, 1, 0, 1), (0, 0, 0, 0), (1, 1, 1, 0)]   # obs, target, prev, indicator


def build(dtype, shape):
    with open(os.path.join(REF, "data/configs/parc_1_train_gen_default.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg.update(device="cpu", use_wandb=False, char_file=os.path.join(REPO, "data/assets/humanoid.xml"))
    cfg.update(shape["cfg"])
    T = cfg["seq_len"]
    torch.manual_seed(shape["seed"])
    m = ref_mdm.MDM(cfg)
    m._denoise_model.eval()
    with torch.no_grad():
        for k, v in m._denoise_model.state_dict().items():
            if k.endswith("in_proj_weight"):
                v.mul_(4.0)
    g = torch.Generator().manual_seed(shape["seed"] + 1)
    D = m._motion_frame_dof
    m._mdm_features_mean = torch.randn((T, D), generator=g) * 0.3
    m._mdm_features_std = torch.rand((T, D), generator=g) * 1.5 + 0.5
    if dtype == torch.float64:
        m._denoise_model.double()
        m._mdm_features_mean, m._mdm_features_std = m._mdm_features_mean.double(), m._mdm_features_std.double()
        for k, v in vars(m._diffusion_rates).items():
            if isinstance(v, torch.Tensor):
                setattr(m._diffusion_rates, k, v.double())
        kin = m._kin_char_model
        for k, v in vars(kin).items():
            if isinstance(v, torch.Tensor) and v.dtype == torch.float32:
                setattr(kin, k, v.double())
            elif isinstance(v, list) and v and all(isinstance(a, torch.Tensor) for a in v):
                setattr(kin, k, [a.double() if a.dtype == torch.float32 else a for a in v])
        for j in getattr(kin, "_joints", []):
            for k, v in vars(j).items():
                if isinstance(v, torch.Tensor) and v.dtype == torch.float32:
                    setattr(j, k, v.double())
    return m, cfg


def inputs(D, T, nprev, seed):
    g = torch.Generator().manual_seed(seed + 2)
    fl = torch.tensor(FLAGS, dtype=torch.bool)
    hf = torch.randn((N, 31, 31), generator=g) * 1.2
    hf[0, :4] = 4.5                                                # beyond +-max_h = 3
    hf[1, -4:] = -5.0
    tgt = torch.randn((N, 2), generator=g)
    tgt = tgt / tgt.norm(dim=-1, keepdim=True)
    h16 = lambda a: a.half().float()                               # stored as fp16, exactly
    return dict(hf_m=h16(hf), target=tgt, prev=h16(torch.randn((N, nprev, D), generator=g) * 0.5), flags=fl, x=h16(torch.randn((N, T, D), generator=g)),
                step_noise=h16(torch.randn((3, N, T, D), generator=g)))


def conds(m, inp, dtype, scale=None):
    c = {MDMKeyType.OBS_KEY: (torch.clamp(inp["hf_m"], -m._max_h, m._max_h) / m._max_h).unsqueeze(1).to(dtype),
         MDMKeyType.TARGET_KEY: inp["target"].unsqueeze(1).to(dtype), MDMKeyType.PREV_STATE_KEY: inp["prev"].to(dtype),
         MDMKeyType.OBS_FLAG_KEY: inp["flags"][:, 0].clone(), MDMKeyType.TARGET_FLAG_KEY: inp["flags"][:, 1].clone(),
         MDMKeyType.PREV_STATE_FLAG_KEY: inp["flags"][:, 2].clone(), MDMKeyType.PREV_STATE_NOISE_IND_KEY: inp["flags"][:, 3].clone()}
    if scale is not None:
        gp = MDMCustomGuidance()
        gp.obs_cfg_scale = scale
        c[MDMKeyType.GUIDANCE_PARAMS] = gp
    return c


def record(m, inp, dtype, shape):
    out = {}
    net = m._denoise_model
    n = N
    with torch.no_grad():
        c = conds(m, inp, dtype)
        mask = net.create_key_padding_mask(n, "cpu")
        tokens = net.embed_conds(c, mask)
        out["tokens"], out["mask"] = torch.cat(tokens, dim=1), mask
        for t in shape["forward_ts"]:
            x = inp["x"].clone().to(dtype)
            tt = t * torch.ones((n, 1, 1), dtype=torch.int64)
            out[f"forward_t{t}"] = net.fast_forward(x, c, tt, tokens, mask)
            out[f"forward_t{t}_x"] = x
        c = conds(m, inp, dtype, SCALE)
        mask = net.create_key_padding_mask(n, "cpu")
        tokens = net.embed_conds(c, mask)
        x = inp["x"].clone().to(dtype)
        out["predict_x0"] = m.predict_x0(x, c, shape["guided_t"] * torch.ones((n, 1, 1), dtype=torch.int64), tokens, mask)
        out["predict_x0_x"] = x
        if shape["record"] == "ddim_guided":
            c = conds(m, inp, dtype, SCALE)
            c["timesteps"] = TS3
            out["ddim_guided"] = torch.stack(m.ddim_inference(c, noise=inp["x"].clone().to(dtype), stride=STRIDE, keep_all_samples=True)[1:])
            return out
        out["project_dofs"] = m.project_dofs((inp["step_noise"][0] * 0.25).to(dtype))   # an input both precisions hold exactly
        for name, scale in (("plain", None), ("guided", SCALE)):
            c = conds(m, inp, dtype, scale)
            c["timesteps"] = TS3
            xs = m.ddim_inference(c, noise=inp["x"].clone().to(dtype), stride=STRIDE, keep_all_samples=True)
            out[f"ddim_{name}"] = torch.stack(xs[1:])
            # reverse_diffusion draws its noise with randn_like: inject the recorded one
            c = conds(m, inp, dtype, scale)
            seq = iter(inp["step_noise"])
            orig = torch.randn_like
            torch.randn_like = lambda a, **kw: next(seq).to(a.dtype)
            try:
                x = inp["x"].clone().to(dtype)
                mask = net.create_key_padding_mask(n, "cpu")
                tokens = net.embed_conds(c, mask)
                xs = []
                for t in TS3:
                    x = m.denoise_one_timestep(x, c, t * torch.ones((n, 1, 1), dtype=torch.int64), tokens, mask)
                    xs.append(x)
            finally:
                torch.randn_like = orig
            out[f"ddpm_{name}"] = torch.stack(xs)
            # gen_sequence: heights in metres, the previous state as a component dict, x_T injected through torch.randn
            c = conds(m, inp, dtype, scale)
            c[MDMKeyType.OBS_KEY] = inp["hf_m"].clone().to(dtype)
            c[MDMKeyType.TARGET_KEY] = inp["target"].clone().to(dtype)
            c[MDMKeyType.PREV_STATE_KEY] = m.extract_motion_features(inp["prev"].to(dtype))
            c["timesteps"] = TS3
            orig_randn = torch.randn
            torch.randn = lambda *a, **kw: inp["x"].clone().to(dtype)
            try:
                res = m.gen_sequence(c, ddim_stride=STRIDE)
            finally:
                torch.randn = orig_randn
            for comp, v in res.items():
                out[f"gen_{name}_{comp.name}"] = v
    return out


def main(name="default", out_dir=HERE):
    shape = SHAPES[name]
    m32, cfg = build(torch.float32, shape)
    m64, _ = build(torch.float64, shape)
    D, T, nprev = m32._motion_frame_dof, cfg["seq_len"], cfg["num_prev_states"]
    inp = inputs(D, T, nprev, shape["seed"])
    r32, r64 = record(m32, inp, torch.float32, shape), record(m64, inp, torch.float64, shape)
    worst = 0.0
    for k in r32:
        if r32[k].dtype == torch.bool:
            assert torch.equal(r32[k], r64[k]), k
            continue
        e = (r32[k].double() - r64[k].double()).abs().max().item()
        worst = max(worst, e)
        print("%-28s fp32 vs float64 %.3e  (max |v| %.2f)" % (k, e, r64[k].abs().max().item()))
        assert e < 1e-4, (k, e, "pick another SEED")
    # x after a pass is the input with the clean previous state where the pass's indicator is set: asserted here, rebuilt by the tests
    ind = inp["flags"][:, 3]
    want = inp["x"].clone()
    want[ind, :nprev] = inp["prev"][ind]
    assert all(torch.equal(r32[f"forward_t{t}_x"], want) for t in shape["forward_ts"])
    want[:, :nprev] = inp["prev"]
    assert torch.equal(r32["predict_x0_x"], want)
    sd = {k: v.detach().cpu().numpy() for k, v in m32._denoise_model.state_dict().items()}
    weights = dict(features_mean=m32._mdm_features_mean.numpy(), features_std=m32._mdm_features_std.numpy())
    arrs = {"hf_m": inp["hf_m"].numpy(), "target": inp["target"].numpy(), "prev": inp["prev"].numpy(), "flags": inp["flags"].numpy(),
            "x": inp["x"].numpy(), "step_noise": inp["step_noise"].numpy(), "timesteps": np.asarray(TS3, np.int32), "stride": np.int32(STRIDE),
            "scale": np.float32(SCALE), "max_h": np.float32(m32._max_h)}
    for k in ("betas", "sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod", "posterior_std", "posterior_mean_coef1", "posterior_mean_coef2"):
        arrs["rates_" + k] = getattr(m32._diffusion_rates, k).numpy()   # DiffusionRates(21), fp32: compared bit for bit
    for k in ("hf_m", "prev", "x", "step_noise"):
        arrs[k] = arrs[k].astype(np.float16)                       # exact: inputs() rounds them to fp16 values
    # the record: the float64 run in fixed point (int32, 2^-28: every recorded value lies within +-7.9, the step is 3.7e-9), and per
    # tensor the largest difference of the fp32 run from it (name_err32).  The fp32 arrays themselves would double the file.
    for k in r32:
        if k.endswith("_x"):
            continue
        if r32[k].dtype == torch.bool:
            arrs[k] = r32[k].numpy()
            continue
        v = r64[k].double().numpy()
        assert np.abs(v).max() < 7.9, k
        arrs[k + "_q28"] = np.round(v * 2.0 ** 28).astype(np.int32)
        arrs[k + "_err32"] = np.float64(np.abs(r32[k].double().numpy() - v).max())
    keep = ("d_model", "num_heads", "d_hid", "num_layers", "seq_len", "num_prev_states", "diffusion_timesteps", "target_mlp_layers", "in_mlp_layers",
            "out_mlp_layers", "features", "use_heightmap_obs", "use_target_obs", "target_type", "predict_mode", "heightmap", "cnn")
    import json
    arrs["cfg_json"] = np.frombuffer(json.dumps({k: cfg[k] for k in keep}).encode(), dtype=np.uint8)
    if name == "default":
        np.savez_compressed(os.path.join(out_dir, "mdm_weights.npz"), **weights, **sd)
        np.savez_compressed(os.path.join(out_dir, "mdm_cases.npz"), **arrs)
        files = ("mdm_weights.npz", "mdm_cases.npz")
    else:                                                          # one file: the cases, the feature statistics, the state dict under sd/
        # left out: the input no recorded tensor reads, the rate tables (the default file holds the same 21 rows) and the tensors the
        # shape drops to stay under the size of mdm_weights.npz (their fp32-vs-float64 check above still ran)
        for k in [k for k in arrs if k == "step_noise" or k.startswith("rates_") or k.rsplit("_", 1)[0] in shape["drop"]]:
            del arrs[k]
        np.savez_compressed(os.path.join(out_dir, "mdm_%s.npz" % name), **arrs, **weights, **{"sd/" + k: v for k, v in sd.items()})
        files = ("mdm_%s.npz" % name,)
    for f in files:
        print(f, os.path.getsize(os.path.join(out_dir, f)), "bytes")
        # a regenerated fixture is the committed one byte for byte (written elsewhere: compared; written in place: git shows it)
        if os.path.abspath(out_dir) != HERE and os.path.exists(os.path.join(HERE, f)):
            with open(os.path.join(out_dir, f), "rb") as a, open(os.path.join(HERE, f), "rb") as b:
                assert a.read() == b.read(), f + " differs from the committed fixture"
            print(f, "is the committed file byte for byte")
    print("worst fp32 vs float64: %.3e" % worst)


if __name__ == "__main__":
    main(*sys.argv[1:3])
