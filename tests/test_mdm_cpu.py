"""The motion generator without a GPU: the CPU restatement ``mdm_ref`` against the reference's record, the
diffusion-rate tables bit for bit, the checkpoint loader, and the refusals the config decides."""
import os

import numpy as np
import pytest
import torch

import mdm_ref as R
from parc_amd import motion_generator as mg

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# mdm_ref in float64 against the reference in float64, as stored: fixed point with steps of 2^-28 = 3.7e-9 (half a step of rounding),
# on top of float64 rounding through a few hundred operations (1e-13): 1e-8 is under three steps
TOL64 = 1e-8


@pytest.fixture(scope="module")
def fx():
    return R.Fixture(os.path.join(REPO, "tests/golden"))


@pytest.fixture(scope="module")
def ref64(fx):
    return R.MdmRef(fx.cfg, fx.sd, fx.mean, fx.std, torch.float64)


def near(name, got, fx):
    err = (got.double() - fx.ref64[name]).abs().max().item()
    print("%-24s %.3e" % (name, err))
    assert err <= TOL64, (name, err)


def test_ref_network_against_the_record(fx, ref64):
    tokens, mask = ref64.embed_conds(fx.conds())
    assert torch.equal(mask, fx.mask)
    near("tokens", tokens, fx)
    for t in (10, 0):
        x = fx.x.clone().double()
        near(f"forward_t{t}", ref64.fast_forward(x, fx.conds(), t, tokens, mask), fx)
        assert torch.equal(x.float(), fx.x_after(False))
    c = fx.conds(fx.scale)
    x = fx.x.clone().double()
    near("predict_x0", ref64.predict_x0(x, c, 10, *ref64.embed_conds(c)), fx)
    assert torch.equal(x.float(), fx.x_after(True)) and not c["ind"].any() and not c["prev_flag"].any()
    near("project_dofs", ref64.project_dofs((fx.step_noise[0] * 0.25).double()), fx)


def test_ref_loops_against_the_record(fx, ref64):
    for name, scale in (("plain", None), ("guided", fx.scale)):
        near(f"ddim_{name}", fx.as_recorded(ref64.ddim(fx.conds(scale), fx.x, fx.stride, fx.timesteps), scale is not None), fx)
        near(f"ddpm_{name}", fx.as_recorded(ref64.ddpm(fx.conds(scale), fx.x, fx.step_noise, fx.timesteps), scale is not None), fx)


def test_ref_gen_sequence_against_the_record(fx, ref64):
    """The standardised sequence of the restatement, taken apart by the package's ``extract`` arithmetic in float64."""
    cm = ref64.cm
    for name, scale in (("plain", None), ("guided", fx.scale)):
        c = fx.conds(scale)
        # gen_sequence takes the previous state as components: what conditions the model is their re-assembly (an exp map past pi wraps)
        p = fx.prev.double() * ref64.std[:2] + ref64.mean[:2]
        s = ref64.sl
        p = torch.cat([p[..., s["pos"]], mg.quat_to_exp_map(mg.exp_map_to_quat(p[..., s["rot"]])), p[..., s["jpos"]],
                       mg.joint_rot_to_dof(cm, mg.joint_dof_to_rot(cm, p[..., s["jrot"]])), p[..., s["con"]]], dim=-1)
        c["prev"] = (p - ref64.mean[:2]) / ref64.std[:2]
        f = ref64.gen_sequence_features(c, fx.x, fx.stride, "DDIM", timesteps=fx.timesteps)
        f = f * ref64.std + ref64.mean
        s = ref64.sl
        near(f"gen_{name}_ROOT_POS", f[..., s["pos"]], fx)
        near(f"gen_{name}_ROOT_ROT", mg.exp_map_to_quat(f[..., s["rot"]]), fx)
        near(f"gen_{name}_JOINT_POS", f[..., s["jpos"]].reshape(fx.n, -1, 14, 3), fx)
        near(f"gen_{name}_JOINT_ROT", mg.joint_dof_to_rot(cm, f[..., s["jrot"]]), fx)
        near(f"gen_{name}_CONTACTS", f[..., s["con"]], fx)


def test_rate_tables_bit_for_bit(fx):
    """The tables the generator hands to the library carry the bits of the reference's own ``DiffusionRates`` (recorded in the fixture);
    the restatement's are the same."""
    a, b = mg.diffusion_rates(21), R.rate_tables(21)
    assert set(a) == set(b) == set(fx.rates) and len(fx.rates) == 6
    for k in a:
        assert a[k].dtype == torch.float32 and a[k].shape == (21,)
        assert torch.equal(a[k], fx.rates[k]) and torch.equal(b[k], fx.rates[k]), k
    for k, v in mg.diffusion_rates(251).items():
        assert torch.equal(v, R.rate_tables(251)[k]) and torch.isfinite(v).all(), k


def test_positional_tables_bit_for_bit(fx):
    """``positional_table`` (weights from a seed) gives the two tables a reference state dict carries."""
    for key in ("_in_pos_encoding.pe", "_embed_t.sequence_pos_encoder.pe"):
        want = fx.sd[key]
        assert torch.equal(mg.positional_table(want.shape[1], want.shape[2]), want), key


def test_ref_against_the_edge_record():
    """``mdm_ref`` off the default shape, against the reference's record at d_model 32, d_hid 48, 20 frames, 3 previous states and MLP
    lists [] / [40, 24] / [24] (``mdm_edge.npz``): the ``model.{3 i}`` keys of zero, two and one hidden layer, the positional table at
    another length and width, the mask range of three previous states, the last row of the timestep table."""
    fx = R.Fixture(os.path.join(REPO, "tests/golden"), "mdm_edge.npz", "mdm_edge.npz")
    cfg = fx.cfg
    assert (cfg["d_model"], cfg["d_hid"], cfg["seq_len"], cfg["num_prev_states"]) == (32, 48, 20, 3)
    assert (cfg["target_mlp_layers"], cfg["in_mlp_layers"], cfg["out_mlp_layers"]) == ([], [40, 24], [24])
    assert set(fx.ref64) == {"tokens", "forward_t20", "ddim_guided"} and fx.timesteps == [20, 10, 0]
    ref64 = R.MdmRef(cfg, fx.sd, fx.mean, fx.std, torch.float64)
    tokens, mask = ref64.embed_conds(fx.conds())
    assert torch.equal(mask, fx.mask) and mask.shape == (fx.n, 87)
    near("tokens", tokens, fx)
    x = fx.x.clone().double()
    near("forward_t20", ref64.fast_forward(x, fx.conds(), 20, tokens, mask), fx)
    assert torch.equal(x.float(), fx.x_after(False))
    near("ddim_guided", fx.as_recorded(ref64.ddim(fx.conds(fx.scale), fx.x, fx.stride, fx.timesteps), True), fx)
    for key in ("_in_pos_encoding.pe", "_embed_t.sequence_pos_encoder.pe"):
        want = fx.sd[key]
        assert torch.equal(mg.positional_table(want.shape[1], want.shape[2]), want), key
    assert fx.sd["_in_pos_encoding.pe"].shape == (1, 87, 32) and mg.tensor_order(cfg) == [k for k in mg.tensor_order(cfg) if k in fx.sd]


def test_checkpoint_loader_reads_the_reference_layout(fx, tmp_path):
    ema = {k: v + 1 for k, v in fx.sd.items()}
    ck = {"cfg": fx.cfg, "model": fx.sd, "ema_model": ema, "optimizer": {},
          "extra": {"_mdm_features_mean": fx.mean, "_mdm_features_std": fx.std, "_seq_len": 15}}
    path = tmp_path / "model.ckpt"
    torch.save(ck, path)
    cfg, sd, mean, std = mg.read_checkpoint(path)
    assert cfg == fx.cfg and all(torch.equal(sd[k], fx.sd[k]) for k in fx.sd)
    assert np.array_equal(mean, fx.mean.numpy()) and np.array_equal(std, fx.std.numpy())
    _, sd_ema, _, _ = mg.read_checkpoint(path, use_ema_model=True)
    assert all(torch.equal(sd_ema[k], ema[k]) for k in ema)
    from parc_amd.motion_sampler import write_feature_stats
    write_feature_stats(str(tmp_path / "feature_stats.yaml"), fx.mean.numpy() * 2, fx.std.numpy() * 3)
    _, _, mean2, std2 = mg.read_checkpoint(path, feature_stats=str(tmp_path / "feature_stats.yaml"))
    assert np.array_equal(mean2, fx.mean.numpy() * 2) and np.array_equal(std2, fx.std.numpy() * 3)
    del ck["extra"]
    torch.save(ck, path)
    with pytest.raises(ValueError, match="feature mean"):
        mg.read_checkpoint(path)
    assert mg.tensor_order(fx.cfg) == [k for k in mg.tensor_order(fx.cfg) if k in fx.sd]   # every tensor the library takes is in a reference state dict


@pytest.mark.parametrize("change, match", [
    (dict(features=dict(rot_type="ROT_6D", frame_components=list(mg.FRAME_COMPONENTS))), "rot_type"),
    (dict(features=dict(rot_type="DEFAULT", frame_components=["ROOT_POS", "ROOT_ROT", "JOINT_ROT", "CONTACTS"])), "frame_components"),
    (dict(use_heightmap_obs=False), "use_heightmap_obs"),
    (dict(use_target_obs=False), "use_heightmap_obs and use_target_obs"),
    (dict(target_type="XY_POS"), "target_type"),
    (dict(predict_mode="PREDICT_NOISE"), "predict_mode"),
    (dict(cnn=dict(net_name="cnn_tokenizer")), "net_name"),
    (dict(heightmap=dict(local_grid=dict(num_x_neg=10, num_x_pos=10, num_y_neg=15, num_y_pos=15), horizontal_scale=0.2, max_h=3.0)), "local_grid"),
    (dict(in_mlp_layers=256), "in_mlp_layers"),
])
def test_config_refusals(change, match):
    cfg = mg.default_config()
    mg.check_config(cfg)
    cfg.update(change)
    with pytest.raises(ValueError, match=match):
        mg.check_config(cfg)


@pytest.mark.parametrize("change, match", [
    (dict(d_model=72, num_heads=3), "d_model must be a multiple of 16"),
    (dict(d_hid=1024), "d_hid must be a multiple of 16 up to"),
    (dict(d_model=64, num_heads=8), "head_dim"),
    (dict(d_model=256, num_heads=2), "head_dim"),
    (dict(num_layers=9), "num_layers"),
    (dict(seq_len=65), "seq_len"),
    (dict(num_prev_states=15), "num_prev_states"),
    (dict(in_mlp_layers=[2048]), "hidden width"),
    (dict(out_mlp_layers=[64] * 9), "hidden layers"),
    (dict(d_model=512, num_heads=8), "PARC_MDM_MAX_D_MODEL"),
    (dict(d_model=384, num_heads=6), "LDS"),
    (dict(d_model=224, num_heads=7, seq_len=64), "LDS"),
])
def test_shape_refusals_at_create(change, match):
    """``parc_mdm_create`` refuses before it touches a device: no GPU is needed to be told no."""
    from parc_amd.lib import ParcError
    cfg = mg.default_config()
    cfg.update(d_model=64, num_heads=4, d_hid=64, num_layers=1, target_mlp_layers=[16], in_mlp_layers=[16], out_mlp_layers=[16])
    cfg.update(change)
    sd = mg.random_state_dict(cfg, 0)
    T = cfg["seq_len"]
    with pytest.raises((ParcError, ValueError), match=match):
        mg.MDMGenerator.from_state_dict(cfg, sd, np.zeros((T, 91), np.float32), np.ones((T, 91), np.float32), "cuda:0")


def test_weight_count_and_sizes_are_checked():
    from parc_amd.lib import ParcError
    cfg = mg.default_config()
    cfg.update(d_model=64, num_heads=4, d_hid=64, num_layers=1, target_mlp_layers=[16], in_mlp_layers=[16], out_mlp_layers=[16])
    sd = mg.random_state_dict(cfg, 0)
    sd["_obs_embed.weight"] = sd["_obs_embed.weight"][:, :200]
    with pytest.raises(ParcError, match="_obs_embed.weight"):
        mg.MDMGenerator.from_state_dict(cfg, sd, np.zeros((15, 91), np.float32), np.ones((15, 91), np.float32), "cuda:0")
    sd = mg.random_state_dict(cfg, 0)
    with pytest.raises(ParcError, match="std non-zero"):
        mg.MDMGenerator.from_state_dict(cfg, sd, np.zeros((15, 91), np.float32), np.zeros((15, 91), np.float32), "cuda:0")
