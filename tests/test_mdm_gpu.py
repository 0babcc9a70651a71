"""The motion generator's inference on the GPU against ``mdm_ref`` on the CPU and, where the fixture holds the
tensor, against the reference's own record (``tests/golden/mdm_cases.npz``).  The yardstick of every comparison is the float64 run; the
bound is ``K`` times what the fp32 run of the same yardstick misses it by, plus 1e-6.  Reads only ``tests/golden/`` and the bundled data."""
import os

import numpy as np
import pytest
import torch

import mdm_ref as R
from parc_amd import motion_generator as mg

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
# twice the largest ratio err(HIP) / err(fp32 reference) that this file prints on the MI355X (DESIGN.md 8j lists them)
K = 4.38
TS3 = [20, 10, 0]


def small_cfg(**kw):
    cfg = mg.default_config()
    cfg.update(d_model=64, num_heads=4, d_hid=64, num_layers=2, target_mlp_layers=[32], in_mlp_layers=[64], out_mlp_layers=[64])
    cfg.update(kw)
    return cfg


def stats(T, D, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((T, D), generator=g) * 0.3, torch.rand((T, D), generator=g) * 1.5 + 0.5


class Case:
    """One model: the HIP generator, the fp32 and the float64 reference, conditions that cover every flag, and an x_T."""

    def __init__(self, cfg, n, seed, max_batch=8):
        self.cfg, self.n = cfg, n
        sd = mg.random_state_dict(cfg, seed)
        for k in sd:
            if k.endswith("in_proj_weight"):
                sd[k] = sd[k] * 4                                  # attention far from uniform
        self.D, self.T = 91, cfg["seq_len"]
        mean, std = stats(self.T, self.D, seed + 1)
        self.gen = mg.MDMGenerator.from_state_dict(cfg, sd, mean, std, DEV, max_batch=max_batch)
        self.r32 = R.MdmRef(cfg, sd, mean, std, torch.float32)
        self.r64 = R.MdmRef(cfg, sd, mean, std, torch.float64)
        self.conds = R.random_conds(n, cfg["num_prev_states"], self.D, seed + 2)
        g = torch.Generator().manual_seed(seed + 3)
        self.x = torch.randn((n, self.T, self.D), generator=g)
        self.step_noise = torch.randn((3, n, self.T, self.D), generator=g)

    def c(self, scale=None):
        c = R.copy_conds(self.conds)
        c["scale"] = scale
        return c

    def dev(self, c):
        return {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in R.to_keys(c).items()}


@pytest.fixture(scope="module")
def small():
    return Case(small_cfg(), 6, 10)


@pytest.fixture(scope="module")
def default():
    return Case(mg.default_config(), 3, 20)


@pytest.fixture(scope="module")
def odd():
    """73 tokens (not a multiple of 16), head_dim 16."""
    return Case(small_cfg(seq_len=6), 3, 30)


@pytest.fixture(scope="module")
def wide_heads():
    """head_dim 64."""
    return Case(small_cfg(d_model=128, num_heads=2), 3, 50)


def close(name, got, r32, r64):
    got, r32, r64 = [np.asarray(torch.as_tensor(a).detach().cpu().double()) for a in (got, r32, r64)]
    ref_err, err = np.abs(r32 - r64).max(), np.abs(got - r64).max()
    print("%-28s ref32-ref64 %.3e  hip-ref64 %.3e  ratio %.2f" % (name, ref_err, err, err / max(ref_err, 1e-30)))
    assert np.isfinite(got).all(), name
    assert err <= K * ref_err + 1e-6, (name, err, ref_err)


def run_all(case):
    gen, n = case.gen, case.n
    # embed_conds
    tok, mask = gen.embed_conds(case.dev(case.c()))
    t32, m32 = case.r32.embed_conds(case.c())
    t64, _ = case.r64.embed_conds(case.c())
    assert torch.equal(mask.cpu(), m32)
    close("embed_conds", tok, t32[:, :65], t64[:, :65])
    # one pass at t = 10 and t = 0: x_0, and x after the call
    for t in (10, 0):
        x = case.x.clone().to(DEV)
        out = gen.forward(x, t)
        x32, x64 = case.x.clone(), case.x.clone().double()
        o32, o64 = case.r32.forward(x32, case.c(), t), case.r64.forward(x64, case.c(), t)
        close("forward t=%d" % t, out, o32, o64)
        assert torch.equal(x.cpu(), x32)
        ind = case.conds["ind"]
        assert torch.equal(x.cpu()[ind, :gen.nprev], case.conds["prev"][ind]) and torch.equal(x.cpu()[~ind], case.x[~ind])
    # guidance
    x = case.x.clone().to(DEV)
    out = gen.predict_x0(x, 10, 1.5)
    x32, x64 = case.x.clone(), case.x.clone().double()
    c32, c64 = case.c(1.5), case.c(1.5)
    o32 = case.r32.predict_x0(x32, c32, 10, *case.r32.embed_conds(c32))
    o64 = case.r64.predict_x0(x64, c64, 10, *case.r64.embed_conds(c64))
    close("predict_x0 guided", out, o32, o64)
    assert torch.equal(x.cpu(), x32)
    inp = o64.float()
    close("project_dofs", gen.project_dofs(inp.to(DEV)), case.r32.project_dofs(inp), case.r64.project_dofs(inp.double()))
    # the loops, every intermediate x
    for scale in (None, 1.5):
        got = gen.ddim_inference(dict(case.dev(case.c()), timesteps=TS3), case.x.to(DEV), 10, keep_all_samples=True, guidance_scale=scale)
        a, b = case.r32.ddim(case.c(scale), case.x, 10, TS3), case.r64.ddim(case.c(scale), case.x, 10, TS3)
        for i in range(3):
            close("ddim %s step %d" % ("guided" if scale else "plain", i), got[i], a[i], b[i])
        got = gen.reverse_diffusion(case.dev(case.c()), case.x.to(DEV), case.step_noise.to(DEV), keep_all_samples=True, guidance_scale=scale, timesteps=TS3)
        a, b = case.r32.ddpm(case.c(scale), case.x, case.step_noise, TS3), case.r64.ddpm(case.c(scale), case.x, case.step_noise, TS3)
        for i in range(3):
            close("ddpm %s step %d" % ("guided" if scale else "plain", i), got[i], a[i], b[i])


@pytest.fixture(scope="module")
def fx():
    return R.Fixture(os.path.join(REPO, "tests/golden"))


def test_every_recorded_tensor_of_the_reference(fx):
    """HIP against the reference's float64 record; the unit of the bound is the reference's own fp32-vs-float64 difference."""
    gen = mg.MDMGenerator.from_state_dict(fx.cfg, fx.sd, fx.mean, fx.std, DEV, max_batch=8)

    def near(name, got):
        err, unit = (got.detach().cpu().double() - fx.ref64[name]).abs().max().item(), fx.err32[name]
        print("%-28s ref32-ref64 %.3e  hip-ref64 %.3e  ratio %.2f" % (name, unit, err, err / unit))
        assert err <= K * unit + 1e-6, (name, err, unit)

    dev = lambda c: {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in R.to_keys(c).items()}
    tok, mask = gen.embed_conds(dev(fx.conds()))
    assert torch.equal(mask.cpu(), fx.mask)
    ind_rows = fx.sd["_embed_prev_state_noise_indicator.weight"][fx.flags[:, 3].long()][:, None]   # the 66th token is a table row
    near("tokens", torch.cat([tok.cpu(), ind_rows], dim=1))
    for t in (10, 0):
        x = fx.x.clone().to(DEV)
        near(f"forward_t{t}", gen.forward(x, t))
        assert torch.equal(x.cpu(), fx.x_after(False))
    x = fx.x.clone().to(DEV)
    near("predict_x0", gen.predict_x0(x, 10, fx.scale))
    assert torch.equal(x.cpu(), fx.x_after(True))
    near("project_dofs", gen.project_dofs((fx.step_noise[0] * 0.25).to(DEV)))
    for name, scale in (("plain", None), ("guided", fx.scale)):
        xs = gen.ddim_inference(dict(dev(fx.conds()), timesteps=fx.timesteps), fx.x.to(DEV), fx.stride, keep_all_samples=True, guidance_scale=scale)
        near(f"ddim_{name}", fx.as_recorded([a.cpu() for a in xs], scale is not None))
        xs = gen.reverse_diffusion(dev(fx.conds()), fx.x.to(DEV), fx.step_noise.to(DEV), keep_all_samples=True, guidance_scale=scale, timesteps=fx.timesteps)
        near(f"ddpm_{name}", fx.as_recorded([a.cpu() for a in xs], scale is not None))
        c = dev(fx.conds())
        c.update(OBS_KEY=fx.hf_m.to(DEV), PREV_STATE_KEY=gen.extract_motion_features(fx.prev.to(DEV)), GUIDANCE_PARAMS=mg.GuidanceParams(scale), timesteps=fx.timesteps)
        out = gen.gen_sequence(c, fx.stride, "DDIM", noise=fx.x.to(DEV))
        for comp, v in out.items():
            near(f"gen_{name}_{comp}", v)


def test_small_model_every_tensor(small):
    run_all(small)


def test_default_size_model(default):
    run_all(default)


def test_73_tokens_head_dim_16(odd):
    run_all(odd)


def test_head_dim_64(wide_heads):
    run_all(wide_heads)


def test_workgroups_walk_several_rows():
    """288 samples, 576 rows under guidance: more than a launch keeps resident, so a workgroup walks several rows through one scratch
    slot (and k_mdm_cond several samples).  Against mdm_ref, and the same bits as the first and the last six samples run on their own."""
    case = Case(small_cfg(), 288, 60, max_batch=288)
    gen = case.gen
    assert gen.describe()["forward_grid"] < 288                     # fewer slots than samples: both kernels loop
    got = gen.ddim_inference(dict(case.dev(case.c()), timesteps=TS3), case.x.to(DEV), 10, keep_all_samples=True, guidance_scale=1.5)
    a, b = case.r32.ddim(case.c(1.5), case.x, 10, TS3), case.r64.ddim(case.c(1.5), case.x, 10, TS3)
    for i in range(3):
        close("288 samples ddim guided step %d" % i, got[i], a[i], b[i])
    for lo in (0, 282):
        ci = {k: (v[lo:lo + 6] if isinstance(v, torch.Tensor) else v) for k, v in case.c().items()}
        part = gen.ddim_inference(dict(case.dev(ci), timesteps=TS3), case.x[lo:lo + 6].to(DEV), 10, guidance_scale=1.5)
        assert torch.equal(part.cpu(), got[2][lo:lo + 6].cpu())


def test_gen_sequence_ddpm(small):
    """``gen_sequence`` in DDPM mode: ``conds["timesteps"]`` as a list of timesteps, and as the reference's int (the start timestep)."""
    case, gen = small, small.gen
    prev_dict = gen.extract_motion_features(case.conds["prev"].to(DEV))
    for ts, steps in ((TS3, TS3), (3, [2, 1, 0])):
        c = case.dev(case.c())
        c.update(OBS_KEY=case.conds["hf"].to(DEV) * gen.max_h, PREV_STATE_KEY=prev_dict, GUIDANCE_PARAMS=None, timesteps=ts)
        out = gen.gen_sequence(c, None, "DDPM", noise=case.x.to(DEV), step_noise=case.step_noise.to(DEV))
        rc = case.c()
        rc["hf"] = (torch.clamp(c["OBS_KEY"], -gen.max_h, gen.max_h) / gen.max_h).cpu()
        rc["prev"] = gen.assemble_mdm_features(prev_dict).cpu()
        f32 = case.r32.gen_sequence_features(R.copy_conds(rc), case.x, 1, "DDPM", case.step_noise, steps)
        f64 = case.r64.gen_sequence_features(R.copy_conds(rc), case.x, 1, "DDPM", case.step_noise, steps)
        got = gen.assemble_mdm_features(out)
        close("gen_sequence ddpm %s" % (ts,), got[:, gen.nprev:], f32[:, gen.nprev:], f64[:, gen.nprev:])
        ind = case.conds["ind"]
        assert torch.equal(got[ind, :gen.nprev].cpu(), gen.assemble_mdm_features(gen.extract_motion_features(rc["prev"].to(DEV)))[ind].cpu())


def test_gen_sequence_components(small):
    """``gen_sequence`` from heights in metres and a component dict: the clean previous state comes back where the indicator is set,
    and under guidance the generated one (the flags are false afterwards)."""
    case, gen = small, small.gen
    prev_feat = case.conds["prev"].to(DEV)
    prev_dict = gen.extract_motion_features(prev_feat)
    hf_m = case.conds["hf"].to(DEV) * gen.max_h * 1.5              # beyond +-max_h: clamped
    for scale in (None, 1.5):
        c = case.dev(case.c())
        c.update(OBS_KEY=hf_m, PREV_STATE_KEY=prev_dict, GUIDANCE_PARAMS=mg.GuidanceParams(scale), timesteps=TS3)
        out = gen.gen_sequence(c, 10, "DDIM", noise=case.x.to(DEV))
        rc = case.c(scale)
        rc["hf"] = (torch.clamp(hf_m, -gen.max_h, gen.max_h) / gen.max_h).cpu()
        rc["prev"] = gen.assemble_mdm_features(prev_dict).cpu()
        f64 = case.r64.gen_sequence_features(R.copy_conds(rc), case.x, 10, "DDIM", timesteps=TS3)
        f32 = case.r32.gen_sequence_features(R.copy_conds(rc), case.x, 10, "DDIM", timesteps=TS3)
        got = gen.assemble_mdm_features(out)
        close("gen_sequence %s" % ("guided" if scale else "plain"), got[:, gen.nprev:], f32[:, gen.nprev:], f64[:, gen.nprev:])
        assert out["ROOT_POS"].shape == (case.n, case.T, 3) and out["JOINT_ROT"].shape == (case.n, case.T, 14, 4)
        if scale is not None:
            assert not c["PREV_STATE_NOISE_IND_KEY"].any() and not c["PREV_STATE_FLAG_KEY"].any()


def test_batch_invariance_bit_for_bit(small):
    """A sample alone, in a batch of 5 and in a shuffled batch: the same bits."""
    case, gen = small, small.gen
    perm = [3, 0, 4, 1, 2]
    full = gen.ddim_inference(dict(case.dev({k: (v[:5] if isinstance(v, torch.Tensor) else v) for k, v in case.c().items()}), timesteps=TS3),
                              case.x[:5].to(DEV), 10, guidance_scale=1.5).cpu()
    cs = {k: (v[perm] if isinstance(v, torch.Tensor) else v) for k, v in case.c().items()}
    shuf = gen.ddim_inference(dict(case.dev(cs), timesteps=TS3), case.x[perm].to(DEV), 10, guidance_scale=1.5).cpu()
    assert torch.equal(shuf, full[perm])
    for i in (0, 3):
        ci = {k: (v[i:i + 1] if isinstance(v, torch.Tensor) else v) for k, v in case.c().items()}
        one = gen.ddim_inference(dict(case.dev(ci), timesteps=TS3), case.x[i:i + 1].to(DEV), 10, guidance_scale=1.5).cpu()
        assert torch.equal(one[0], full[i])


def test_device_drawn_noise(default):
    """x_T and the DDPM noise drawn on the device depend on (seed, index, step) only; x_T is standard normal."""
    case, gen = default, default.gen
    c = case.dev(case.c())
    a = gen.reverse_diffusion(c, seed=7, first_index=100, timesteps=TS3).cpu()
    rev = {k: (v.flip(0) if isinstance(v, torch.Tensor) else v) for k, v in c.items()}
    assert torch.isfinite(a).all()
    # sample 0 of this call has index 102 and the conditions of sample 2 above
    b = gen.reverse_diffusion(rev, seed=7, first_index=102, timesteps=TS3).cpu()
    assert torch.equal(b[0], a[2])
    assert not torch.equal(gen.reverse_diffusion(c, seed=8, first_index=100, timesteps=TS3).cpu(), a)
    # the drawn x_T and step noise, injected, give the same sample: the draws inside the kernels are the ones draw_noise shows
    xt = gen.draw_noise(case.n, 7, 100, 0)
    sn = torch.stack([gen.draw_noise(case.n, 7, 100, i + 1) for i in range(3)])
    assert torch.equal(gen.reverse_diffusion(c, xt, sn, timesteps=TS3).cpu(), a)
    v = gen.draw_noise(64, 11, 0).cpu().double().numpy().ravel()
    n = v.size
    assert n == 64 * 15 * 91
    assert abs(v.mean()) <= 4.0 / np.sqrt(n)                       # four standard errors of the mean and of the variance of N(0, 1)
    assert abs(v.var() - 1.0) <= 4.0 * np.sqrt(2.0 / n)
    assert torch.equal(gen.draw_noise(2, 11, 5).cpu(), gen.draw_noise(64, 11, 0)[5:7].cpu())


def test_kernel_times_finite(small):
    case, gen = small, small.gen
    gen.ddim_inference(dict(case.dev(case.c()), timesteps=TS3), case.x.to(DEV), 10, guidance_scale=1.5)
    t = gen.kernel_times()
    assert set(t) == set(mg.KERNELS) and all(np.isfinite(v) and v > 0 for v in t.values())
    d = gen.describe()
    assert 0 < d["forward_lds_bytes"] <= 160 * 1024 and d["forward_grid"] >= 1


def test_generate_motion_windows_dry_run(small, tmp_path):
    """``scripts/generate_motion_windows.py --random_init`` on two small batches in the exporter's layout: it writes one file per batch,
    finite and of the batch's shapes, and the same files when run again."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("generate_motion_windows", os.path.join(REPO, "scripts/generate_motion_windows.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    g = torch.Generator().manual_seed(40)
    src = tmp_path / "batches"
    src.mkdir()
    for b in range(2):
        comps = small.gen.extract_motion_features((torch.randn((4, 15, 91), generator=g) * 0.3).to(DEV))
        rot = torch.randn((4, 4), generator=g)
        np.savez(src / ("batch_%06d.npz" % b), hfs=(torch.randn((4, 31, 31), generator=g) * 0.5).numpy(), target_pos=torch.randn((4, 3), generator=g).numpy(),
                 target_rot=(rot / rot.norm(dim=-1, keepdim=True)).numpy(), **{k.lower(): v.cpu().numpy() for k, v in comps.items()})
    outs = []
    for name in ("a", "b"):
        assert mod.main(["--batches", str(src), "--out", str(tmp_path / name), "--random_init", "3", "--guidance", "1.5", "--device", DEV]) == 0
        outs.append([np.load(tmp_path / name / ("gen_%06d.npz" % b)) for b in range(2)])
    for za, zb in zip(*outs):
        assert za["root_pos"].shape == (4, 15, 3) and za["root_rot"].shape == (4, 15, 4) and za["joint_rot"].shape == (4, 15, 14, 4)
        assert za["joint_pos"].shape == (4, 15, 14, 3) and za["contacts"].shape == (4, 15, 15)
        for k in za.files:
            assert np.isfinite(za[k]).all() and np.array_equal(za[k], zb[k]), k
    assert not np.array_equal(outs[0][0]["root_pos"], outs[0][1]["root_pos"])
