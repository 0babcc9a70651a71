"""The motion generator's inference on the GPU against ``mdm_ref`` on the CPU and, where the fixture holds the
tensor, against the reference's own records (``tests/golden/mdm_cases.npz``, ``mdm_edge.npz``).  The yardstick of every comparison is the float64 run; the
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
# twice the largest ratio err(HIP) / err(fp32 reference) that this file prints on the MI355X (DESIGN.md 8j lists them): 3.84, project_dofs
# of the default-size model at six samples (at three samples the largest was 2.19 and K 4.38; no shape edge exceeds 2.30)
K = 7.68
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
    """One model: the HIP generator, the fp32 and the float64 reference, conditions that cover every flag (all six combinations from
    n = 6 on), an x_T, and the timesteps its tests run: ``fwd_ts`` the two of a single pass, ``ts`` / ``stride`` the loops' list, which
    holds the last row of the timestep table."""

    def __init__(self, cfg, n, seed, max_batch=8, fwd_ts=(10, 0), ts=TS3, stride=10, mean_std=None):
        self.cfg, self.n = cfg, n
        self.fwd_ts, self.ts, self.stride = tuple(fwd_ts), list(ts), stride
        assert cfg["diffusion_timesteps"] - 1 in self.ts and 0 in self.fwd_ts
        sd = mg.random_state_dict(cfg, seed)
        for k in sd:
            if k.endswith("in_proj_weight"):
                sd[k] = sd[k] * 4                                  # attention far from uniform
        self.D, self.T = 91, cfg["seq_len"]
        mean, std = mean_std if mean_std is not None else stats(self.T, self.D, seed + 1)
        self.gen = mg.MDMGenerator.from_state_dict(cfg, sd, mean, std, DEV, max_batch=max_batch)
        self.r32 = R.MdmRef(cfg, sd, mean, std, torch.float32)
        self.r64 = R.MdmRef(cfg, sd, mean, std, torch.float64)
        self.conds = R.random_conds(n, cfg["num_prev_states"], self.D, seed + 2)
        g = torch.Generator().manual_seed(seed + 3)
        self.x = torch.randn((n, self.T, self.D), generator=g)
        self.step_noise = torch.randn((len(self.ts), n, self.T, self.D), generator=g)

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
    return Case(mg.default_config(), 6, 20)


@pytest.fixture(scope="module")
def odd():
    """73 tokens (not a multiple of 16), head_dim 16."""
    return Case(small_cfg(seq_len=6), 6, 30)


@pytest.fixture(scope="module")
def wide_heads():
    """head_dim 64."""
    return Case(small_cfg(d_model=128, num_heads=2), 6, 50)


# ---- the shape edges (DESIGN.md 8j lists what each reaches); their single passes run the last row of the timestep table ----------------
@pytest.fixture(scope="module")
def tail():
    """15 attention work items on 4 waves (the last round has a wave without work), d_model 48 (LayerNorm with idle lanes), no hidden
    layer in any of the three MLPs, no previous state, d_hid > d_model."""
    return Case(small_cfg(d_model=48, num_heads=3, d_hid=80, num_layers=1, seq_len=6, num_prev_states=0, target_mlp_layers=[], in_mlp_layers=[],
                          out_mlp_layers=[]), 6, 70, fwd_ts=(20, 0))


@pytest.fixture(scope="module")
def long():
    """64 frames: 9 row tiles (MAXMT), 4 row tiles of frames, 18 attention items, two and three hidden layers (both directions of the
    ping-pong), widths that are no multiple of 16, every frame but the last a previous state, d_hid < d_model."""
    return Case(small_cfg(d_model=64, num_heads=2, d_hid=32, num_layers=2, seq_len=64, num_prev_states=63, target_mlp_layers=[8, 8],
                          in_mlp_layers=[40, 24], out_mlp_layers=[24, 40, 56]), 6, 80, fwd_ts=(20, 0))


@pytest.fixture(scope="module")
def t17():
    """17 frames: the residual stream has 99 rows (67 + 32 frame rows) against 96 token rows, 15 of the frame rows dead; d_model 16;
    hidden widths 1 / 17 / 33."""
    return Case(small_cfg(d_model=16, num_heads=1, d_hid=16, num_layers=2, seq_len=17, target_mlp_layers=[1], in_mlp_layers=[17], out_mlp_layers=[33]),
                6, 90, fwd_ts=(20, 0))


@pytest.fixture(scope="module")
def lds15():
    """The largest d_model that fits the LDS at 15 frames (not a multiple of 64), d_hid at its cap."""
    return Case(small_cfg(d_model=352, num_heads=11, d_hid=512, num_layers=1), 6, 100, fwd_ts=(20, 0))


@pytest.fixture(scope="module")
def lds1():
    """PARC_MDM_MAX_D_MODEL with a single frame and no previous state: 65 attention items."""
    return Case(small_cfg(d_model=416, num_heads=13, d_hid=16, num_layers=1, seq_len=1, num_prev_states=0), 6, 110, fwd_ts=(20, 0))


@pytest.fixture(scope="module")
def wide_hidden():
    """A second hidden layer of six column tiles: a wave owns two of them and stores the first before it reads A for the second, so the
    layer must not write the region it reads (with at most four tiles, as in every other case, an in-place layer comes out right)."""
    return Case(small_cfg(in_mlp_layers=[32, 96], out_mlp_layers=[96, 96]), 6, 140, fwd_ts=(20, 0))


@pytest.fixture(scope="module")
def steps():
    """251 diffusion timesteps: six-step loops (the handle's event list is created for four steps)."""
    return Case(small_cfg(num_layers=1, diffusion_timesteps=251), 6, 120, fwd_ts=(250, 0), ts=[250, 200, 150, 100, 50, 0], stride=50)


def close(name, got, r32, r64):
    got, r32, r64 = [np.asarray(torch.as_tensor(a).detach().cpu().double()) for a in (got, r32, r64)]
    ref_err, err = np.abs(r32 - r64).max(), np.abs(got - r64).max()
    print("%-28s ref32-ref64 %.3e  hip-ref64 %.3e  ratio %.2f" % (name, ref_err, err, err / max(ref_err, 1e-30)))
    assert np.isfinite(got).all(), name
    assert ref_err <= 1e-4, (name, ref_err)                        # the yardstick itself sits on a branch cut: another seed, not a wider bound
    assert err <= K * ref_err + 1e-6, (name, err, ref_err)


def run_all(case):
    gen, n = case.gen, case.n
    # embed_conds
    tok, mask = gen.embed_conds(case.dev(case.c()))
    t32, m32 = case.r32.embed_conds(case.c())
    t64, _ = case.r64.embed_conds(case.c())
    assert torch.equal(mask.cpu(), m32)
    close("embed_conds", tok, t32[:, :65], t64[:, :65])
    # one pass at the case's two timesteps: x_0, and x after the call
    for t in case.fwd_ts:
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
    t = case.fwd_ts[0]
    out = gen.predict_x0(x, t, 1.5)
    x32, x64 = case.x.clone(), case.x.clone().double()
    c32, c64 = case.c(1.5), case.c(1.5)
    o32 = case.r32.predict_x0(x32, c32, t, *case.r32.embed_conds(c32))
    o64 = case.r64.predict_x0(x64, c64, t, *case.r64.embed_conds(c64))
    close("predict_x0 guided", out, o32, o64)
    assert torch.equal(x.cpu(), x32)
    inp = o64.float()
    close("project_dofs", gen.project_dofs(inp.to(DEV)), case.r32.project_dofs(inp), case.r64.project_dofs(inp.double()))
    # the loops, every intermediate x
    for scale in (None, 1.5):
        run_ddim(case, scale, case.ts, case.stride)
        run_ddpm(case, scale, case.ts)


def run_ddim(case, scale, ts, stride):
    """every x of a DDIM loop against mdm_ref"""
    got = case.gen.ddim_inference(dict(case.dev(case.c()), timesteps=ts), case.x.to(DEV), stride, keep_all_samples=True, guidance_scale=scale)
    a, b = case.r32.ddim(case.c(scale), case.x, stride, ts), case.r64.ddim(case.c(scale), case.x, stride, ts)
    assert len(got) == len(a) == len(ts)
    for i in range(len(ts)):
        close("ddim %s step %d" % ("guided" if scale else "plain", i), got[i], a[i], b[i])


def run_ddpm(case, scale, ts):
    """every x of a DDPM loop with injected noise against mdm_ref"""
    got = case.gen.reverse_diffusion(case.dev(case.c()), case.x.to(DEV), case.step_noise.to(DEV), keep_all_samples=True, guidance_scale=scale, timesteps=ts)
    a, b = case.r32.ddpm(case.c(scale), case.x, case.step_noise, ts), case.r64.ddpm(case.c(scale), case.x, case.step_noise, ts)
    assert len(got) == len(a) == len(ts)
    for i in range(len(ts)):
        close("ddpm %s step %d" % ("guided" if scale else "plain", i), got[i], a[i], b[i])


@pytest.fixture(scope="module")
def fx():
    return R.Fixture(os.path.join(REPO, "tests/golden"))


@pytest.fixture(scope="module")
def fx_edge():
    return R.Fixture(os.path.join(REPO, "tests/golden"), "mdm_edge.npz", "mdm_edge.npz")


def near_record(fx, name, got):
    err, unit = (got.detach().cpu().double() - fx.ref64[name]).abs().max().item(), fx.err32[name]
    print("%-28s ref32-ref64 %.3e  hip-ref64 %.3e  ratio %.2f" % (name, unit, err, err / unit))
    assert err <= K * unit + 1e-6, (name, err, unit)


def fx_dev(c):
    return {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in R.to_keys(c).items()}


def test_every_recorded_tensor_of_the_edge_reference(fx_edge):
    """HIP against the reference's float64 record off the default shape (``mdm_edge.npz``): d_model 32, d_hid 48, 20 frames (two row
    tiles of frames), 3 previous states, MLP lists [] / [40, 24] / [24]."""
    fx = fx_edge
    gen = mg.MDMGenerator.from_state_dict(fx.cfg, fx.sd, fx.mean, fx.std, DEV, max_batch=8)
    tok, mask = gen.embed_conds(fx_dev(fx.conds()))
    assert torch.equal(mask.cpu(), fx.mask)
    ind_rows = fx.sd["_embed_prev_state_noise_indicator.weight"][fx.flags[:, 3].long()][:, None]   # the 66th token is a table row
    near_record(fx, "tokens", torch.cat([tok.cpu(), ind_rows], dim=1))
    x = fx.x.clone().to(DEV)
    near_record(fx, "forward_t20", gen.forward(x, 20))
    assert torch.equal(x.cpu(), fx.x_after(False))
    xs = gen.ddim_inference(dict(fx_dev(fx.conds()), timesteps=fx.timesteps), fx.x.to(DEV), fx.stride, keep_all_samples=True, guidance_scale=fx.scale)
    near_record(fx, "ddim_guided", fx.as_recorded([a.cpu() for a in xs], True))


def test_every_recorded_tensor_of_the_reference(fx):
    """HIP against the reference's float64 record; the unit of the bound is the reference's own fp32-vs-float64 difference."""
    gen = mg.MDMGenerator.from_state_dict(fx.cfg, fx.sd, fx.mean, fx.std, DEV, max_batch=8)
    near, dev = (lambda name, got: near_record(fx, name, got)), fx_dev
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


def test_tail_dead_wave_no_hidden_layers_no_prev(tail):
    run_all(tail)


def test_long_64_frames_nine_row_tiles(long):
    run_all(long)


def test_t17_frame_rows_past_the_token_rows(t17):
    run_all(t17)


def test_lds15_largest_d_model_at_15_frames(lds15):
    # 96 rows of 352 + 4 floats, and four attention tiles [16][96 + 4] (larger than the frames' [16][96 + 4])
    assert lds15.gen.describe()["forward_lds_bytes"] == 4 * (96 * 356 + 4 * 16 * 100) == 162304
    run_all(lds15)


def test_lds1_max_d_model_one_frame(lds1):
    # 83 rows (67 + 16 frame rows, against 80 token rows) of 416 + 4 floats, and four attention tiles [16][80 + 4]
    assert lds1.gen.describe()["forward_lds_bytes"] == 4 * (83 * 420 + 4 * 16 * 84) == 160944
    run_all(lds1)


def test_hidden_layers_of_six_column_tiles(wide_hidden):
    run_all(wide_hidden)


def test_sampler_six_steps_then_two(steps):
    """Six-step loops on a 251-row table (the event list of a new handle holds four steps), every intermediate x against mdm_ref; the
    kernel times of a six-step run, and of a two-step run after it; six steps of device-drawn DDPM noise."""
    case, gen = steps, steps.gen
    ddpm_ts = [250, 249, 3, 2, 1, 0]
    for scale in (None, 1.5):
        run_ddpm(case, scale, ddpm_ts)
        run_ddim(case, scale, case.ts, case.stride)
    t6 = gen.kernel_times()                                        # of the guided six-step DDIM
    assert set(t6) == set(mg.KERNELS) and all(np.isfinite(v) and v > 0 for v in t6.values()), t6
    gen.ddim_inference(dict(case.dev(case.c()), timesteps=[50, 0]), case.x.to(DEV), 50, guidance_scale=1.5)
    t2 = gen.kernel_times()
    assert all(np.isfinite(v) and v > 0 for v in t2.values()), t2
    assert t2["forward"] < t6["forward"] and t2["update"] < t6["update"], (t2, t6)
    c = case.dev(case.c())
    a = gen.reverse_diffusion(c, seed=7, first_index=100, timesteps=ddpm_ts).cpu()
    assert torch.isfinite(a).all()
    xt = gen.draw_noise(case.n, 7, 100, 0)
    sn = torch.stack([gen.draw_noise(case.n, 7, 100, i + 1) for i in range(6)])
    assert torch.equal(gen.reverse_diffusion(c, xt, sn, timesteps=ddpm_ts).cpu(), a)


def test_project_dofs_at_chosen_poses():
    """``k_mdm_update`` on poses built by hand (mean 0, std 1: the standardised values are the features): the identity, angles past pi
    on the root, the spherical joints and the hinges (every angle at least 0.3 rad from pi and 2 pi), norms under the small-angle
    switch, hinges of alternating sign at a small angle; contacts outside [0, 1]."""
    from parc_amd.char_model import JointType
    T, D = 15, 91
    case = Case(small_cfg(), 4, 130, mean_std=(torch.zeros((T, D)), torch.ones((T, D))))
    cm, s = case.r64.cm, case.r64.sl
    jt, di = cm.joint_type_array(), cm.dof_idx_array()
    sph = [int(di[j]) for j in range(1, cm.get_num_bodies()) if jt[j] == JointType.SPHERICAL]
    hin = [int(di[j]) for j in range(1, cm.get_num_bodies()) if jt[j] == JointType.HINGE]
    assert len(sph) == 8 and len(hin) == 4
    unit = lambda v: v / v.norm(dim=-1, keepdim=True)
    f = torch.arange(T, dtype=torch.float64)
    # a direction per (frame, joint) with no zero component
    dirs = unit(torch.stack([torch.ones((T, 8), dtype=torch.float64), 0.6 + 0.05 * torch.arange(8, dtype=torch.float64).expand(T, 8),
                             (-0.8 + 0.03 * f)[:, None].expand(T, 8)], dim=-1))
    sign = torch.where((torch.arange(T)[:, None] + torch.arange(4)[None, :]) % 2 == 0, 1.0, -1.0).double()
    root_dir = unit(torch.tensor([1.0, 2.0, -2.0], dtype=torch.float64))
    x = torch.zeros((4, T, D), dtype=torch.float64)                # row 0: the identity everywhere
    jr0, c0 = s["jrot"].start, s["con"].start

    def fill(row, root_norm, sph_norm, hinge, contacts):
        x[row, :, s["pos"]] = torch.tensor([0.5, -0.3, 0.9], dtype=torch.float64) * (1 + 0.1 * f)[:, None]
        x[row, :, s["rot"]] = root_norm * root_dir
        for k, d0 in enumerate(sph):
            x[row, :, jr0 + d0:jr0 + d0 + 3] = sph_norm[:, k, None] * dirs[:, k]
        for k, d0 in enumerate(hin):
            x[row, :, jr0 + d0] = hinge[:, k]
        x[row, :, s["con"]] = contacts

    alt = torch.where(torch.arange(D - c0) % 2 == 0, -0.5, 1.7).double()
    fill(1, 4.0, torch.linspace(3.6, 5.5, T * 8, dtype=torch.float64).reshape(T, 8),
         sign * torch.linspace(3.6, 5.5, T * 4, dtype=torch.float64).reshape(T, 4), alt)
    fill(2, 1e-7, torch.full((T, 8), 1e-7, dtype=torch.float64), sign * 1e-7, 0.25)
    fill(3, 0.3, torch.full((T, 8), 0.3, dtype=torch.float64), sign * 0.3, 0.75)
    inp = x.float()
    got = case.gen.project_dofs(inp.to(DEV)).cpu()
    close("project_dofs chosen poses", got, case.r32.project_dofs(inp), case.r64.project_dofs(inp.double()))
    # independently of mdm_ref
    assert torch.equal(got[..., s["con"]], torch.clamp(inp[..., s["con"]], 0.0, 1.0))
    assert (got[0, :, s["rot"]] == 0).all() and (got[0, :, s["jrot"]] == 0).all()
    for row in (1, 3):
        a, b = got[row:row + 1].double(), inp[row:row + 1].double()
        for qa, qb in ((mg.joint_dof_to_rot(cm, a[..., s["jrot"]]), mg.joint_dof_to_rot(cm, b[..., s["jrot"]])),
                       (mg.exp_map_to_quat(a[..., s["rot"]]), mg.exp_map_to_quat(b[..., s["rot"]]))):
            diff = torch.minimum((qa - qb).abs().amax(-1), (qa + qb).abs().amax(-1)).max().item()
            print("row %d rotations rebuilt from the output against the input's: %.3e" % (row, diff))
            assert diff <= 1e-5, (row, diff)


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


def batch_invariance(case):
    gen = case.gen
    perm = [3, 0, 4, 1, 2]
    full = gen.ddim_inference(dict(case.dev({k: (v[:5] if isinstance(v, torch.Tensor) else v) for k, v in case.c().items()}), timesteps=case.ts),
                              case.x[:5].to(DEV), case.stride, guidance_scale=1.5).cpu()
    cs = {k: (v[perm] if isinstance(v, torch.Tensor) else v) for k, v in case.c().items()}
    shuf = gen.ddim_inference(dict(case.dev(cs), timesteps=case.ts), case.x[perm].to(DEV), case.stride, guidance_scale=1.5).cpu()
    assert torch.isfinite(full).all() and torch.equal(shuf, full[perm])
    for i in (0, 3):
        ci = {k: (v[i:i + 1] if isinstance(v, torch.Tensor) else v) for k, v in case.c().items()}
        one = gen.ddim_inference(dict(case.dev(ci), timesteps=case.ts), case.x[i:i + 1].to(DEV), case.stride, guidance_scale=1.5).cpu()
        assert torch.equal(one[0], full[i])


def test_batch_invariance_bit_for_bit(small):
    """A sample alone, in a batch of 5 and in a shuffled batch: the same bits."""
    batch_invariance(small)


def test_batch_invariance_bit_for_bit_tail(tail):
    """The same where a wave of the last attention round has no work: a stale tile would show as a dependence on the neighbour."""
    batch_invariance(tail)


def test_batch_invariance_bit_for_bit_long(long):
    """The same over nine row tiles."""
    batch_invariance(long)


def test_device_drawn_noise(default):
    """x_T and the DDPM noise drawn on the device depend on (seed, index, step) only; x_T is standard normal."""
    case, gen = default, default.gen
    c = case.dev(case.c())
    a = gen.reverse_diffusion(c, seed=7, first_index=100, timesteps=TS3).cpu()
    rev = {k: (v.flip(0) if isinstance(v, torch.Tensor) else v) for k, v in c.items()}
    assert torch.isfinite(a).all()
    # sample 0 of this call has the index and the conditions of the last sample above
    b = gen.reverse_diffusion(rev, seed=7, first_index=100 + case.n - 1, timesteps=TS3).cpu()
    assert torch.equal(b[0], a[case.n - 1])
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
