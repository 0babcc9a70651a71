"""The generator's trainer without a GPU: ``MDMDenoiser`` against ``mdm_ref`` and the reference's records, and the
training loop on the CPU with the float64 restatement of the loss, on windows of the bundled clips given as batches
(``tests/golden/motion_sampler_none.npz``)."""
import math
import os

import numpy as np
import pytest
import torch

import mdm_loss_ref as LR
import mdm_ref as R
from parc_amd import motion_generator as mg
from parc_amd.motion_trainer import MDMDenoiser, MDMTrainer
from parc_amd.util import path_loader

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests/golden")
TOL64 = 1e-8   # as tests/test_mdm_cpu.py: the record's fixed point (3.7e-9 a step) on top of float64 rounding


def train_cfg(**over):
    """The shipped training config at the MDM fixture's small shape."""
    cfg = path_loader.load_config(os.path.join(REPO, "data/configs/mdm_train/mdm_train_default.yaml"))
    cfg.update(d_model=64, num_heads=4, d_hid=64, num_layers=2, target_mlp_layers=[32], in_mlp_layers=[64], out_mlp_layers=[64], batch_size=12,
               lr=1e-3, use_target_loss=True)
    cfg.update(over)
    return cfg


@pytest.fixture(scope="module")
def batch():
    """12 windows as ``MotionWindowSampler.sample`` returns them."""
    z = np.load(os.path.join(GOLDEN, "motion_sampler_none.npz"))
    t = lambda k: torch.from_numpy(z[k].astype(np.float32))  # noqa: E731
    motion = {"ROOT_POS": t("root_pos"), "ROOT_ROT": t("root_rot"), "JOINT_POS": t("joint_pos"), "JOINT_ROT": t("joint_rot"), "CONTACTS": t("contacts")}
    return motion, t("hfs"), t("target_pos"), t("target_rot")


def window_stats(batch):
    from parc_amd.char_model import CharModel
    cm = CharModel(os.path.join(REPO, "data/assets/humanoid.xml"))
    f = mg.assemble_features(cm, batch[0])
    return mg.feature_stats(f, slice(f.shape[-1] - 15, f.shape[-1]))


def make(batch, seed=0, **over):
    cfg = train_cfg(**over)
    loss = LR.MdmLossRef(dict(cfg, num_prev_states=cfg["num_prev_states"]), cfg["train_loss_fn"], torch.float64, "cpu")
    return MDMTrainer(cfg, None, "cpu", loss=loss, feature_stats=window_stats(batch), seed=seed)


@pytest.mark.parametrize("files", [dict(), dict(cases="mdm_edge.npz", weights="mdm_edge.npz")], ids=["default", "edge"])
def test_denoiser_matches_the_restatement_and_the_record(files):
    fx = R.Fixture(GOLDEN, **files)
    net = MDMDenoiser(fx.cfg, fx.mean.shape[1]).eval()
    sd, order = net.state_dict(), mg.tensor_order(fx.cfg)
    assert sorted(sd) == sorted(order) and all(tuple(sd[k].shape) == tuple(fx.sd[k].shape) for k in order)
    assert torch.equal(sd["_in_pos_encoding.pe"], fx.sd["_in_pos_encoding.pe"])      # the tables the module builds are the checkpoint's
    net.load_state_dict(fx.sd)
    ref64 = R.MdmRef(fx.cfg, fx.sd, fx.mean, fx.std, torch.float64)
    net64 = MDMDenoiser(fx.cfg, fx.mean.shape[1]).double().eval()
    net64.load_state_dict({k: v.double() for k, v in fx.sd.items()})
    tokens, mask = net64.embed_conds(R.to_keys({k: (v.double() if isinstance(v, torch.Tensor) and v.is_floating_point() else v) for k, v in fx.conds().items()}))
    assert torch.equal(mask, fx.mask) and (tokens - fx.ref64["tokens"]).abs().max() <= TOL64
    names = [n for n in ("forward_t10", "forward_t0", "forward_t20") if n in fx.ref64]
    assert names
    for name in names:
        t = int(name.split("_t")[1])
        c = fx.conds()
        with torch.no_grad():
            y32 = net(fx.x.clone(), R.to_keys(c), t)
            c64 = {k: (v.double() if isinstance(v, torch.Tensor) and v.is_floating_point() else v) for k, v in c.items()}
            y64 = net64(fx.x.clone().double(), R.to_keys(c64), torch.full((fx.n,), t))
            want = ref64.forward(fx.x.clone().double(), fx.conds(), t)
        e64, e32, unit = (y64 - fx.ref64[name]).abs().max().item(), (y32.double() - fx.ref64[name]).abs().max().item(), fx.err32[name]
        print(name, "float64 %.2e  fp32 %.2e  the reference's own fp32 %.2e" % (e64, e32, unit))
        assert e64 <= TOL64 and (y64 - want).abs().max() <= TOL64
        # another fp32 evaluation of the same function misses float64 by about what the reference's own fp32 run does: two units
        assert e32 <= 2 * unit + 1e-6


def test_flags_follow_their_chances(batch):
    """3000 draws per flag under a fixed generator; a count k of n draws at chance p is held to |k - n p| <= 4 sqrt(n p (1 - p)) (four
    standard deviations of the binomial: a fair generator fails one flag in 16 000 seeds)."""
    tr = make(batch)
    motion, hfs, tp, trot = batch
    n, off = 0, {"PREV_STATE_FLAG_KEY": 0, "TARGET_FLAG_KEY": 0, "OBS_FLAG_KEY": 0}
    ind = 0
    for _ in range(250):
        conds, x0 = tr.construct_conds(motion, hfs, tp, trot, test=False)
        n += x0.shape[0]
        for k in off:
            off[k] += int((~conds[k]).sum())
        ind += int(tr.draw_noise_indicator(x0.shape[0]).sum())
    assert n == 3000
    for k, p in (("PREV_STATE_FLAG_KEY", 0.15), ("TARGET_FLAG_KEY", 0.025), ("OBS_FLAG_KEY", 0.025)):
        assert abs(off[k] - n * p) <= 4 * math.sqrt(n * p * (1 - p)), (k, off[k])
    assert abs(ind - n * 0.5) <= 4 * math.sqrt(n * 0.25), ind
    conds, _ = tr.construct_conds(motion, hfs, tp, trot, test=True)
    assert all(bool(conds[k].all()) for k in off)
    assert torch.equal(conds["OBS_KEY"], hfs / 3.0) and conds["TARGET_KEY"].shape == (12, 2)


def test_ema_copies_then_decays_and_the_gradient_is_clipped(batch):
    tr = make(batch, EMA=dict(ema_decay=0.9, ema_start=3, ema_update_rate=1))
    for step in (1, 2):
        tr.step(batch)
        assert all(torch.equal(e, p) for e, p in zip(tr.ema_model.parameters(), tr.model.parameters())), step
    before = [e.detach().clone() for e in tr.ema_model.parameters()]
    tr.step(batch)
    moved = 0
    for b, e, p in zip(before, tr.ema_model.parameters(), tr.model.parameters()):
        # the rule, to the two fp32 roundings by which a multiply-then-add and an add-with-scale may differ
        assert torch.allclose(e, b * 0.9 + p.detach() * (1.0 - 0.9), rtol=2.4e-7, atol=1e-9)
        moved += int(not torch.equal(e, p))
    assert moved > 0
    # the loss of an untrained network is far above 1 in gradient norm: the step saw it clipped to 1
    total = torch.sqrt(sum((p.grad.double() ** 2).sum() for p in tr.model.parameters() if p.grad is not None))
    assert float(tr.grad_norm) > 1.0 and abs(float(total) - 1.0) < 1e-4


def test_steps_lower_the_loss_and_the_checkpoint_resumes_bit_equal(batch, tmp_path):
    tr = make(batch, seed=3, dropout=0.0)
    tr.gen.manual_seed(11)
    first = tr.evaluate(batch=batch)[0]
    for _ in range(8):
        tr.step(batch)
    path = tmp_path / "model.ckpt"
    tr.save_checkpoint(path)
    tr.gen.manual_seed(11)
    assert tr.evaluate(batch=batch)[0] < first
    # read_checkpoint reads it; the generator's front end would take these
    cfg, sd, mean, std = mg.read_checkpoint(path)
    assert sorted(sd) == sorted(mg.tensor_order(cfg)) and mean.shape == (15, 91) and np.array_equal(mean, tr.mean.numpy())
    _, ema_sd, _, _ = mg.read_checkpoint(path, use_ema_model=True)
    assert sorted(ema_sd) == sorted(sd)
    # resume: a fresh trainer from another seed continues as the first one does
    tr.load(path)                                                  # (puts the generator back to where the file was written)
    other = make(batch, seed=99, dropout=0.0)
    other.load(path)
    for _ in range(2):
        la, lb = tr.step(batch)[0], other.step(batch)[0]
        assert torch.equal(la, lb)
    for (k, a), b in zip(tr.model.state_dict().items(), other.model.state_dict().values()):
        assert torch.equal(a, b), k
    assert all(torch.equal(a, b) for a, b in zip(tr.ema_model.parameters(), other.ema_model.parameters())) and tr.ema_step == other.ema_step == 10


def test_dropout_masks_come_from_the_trainers_generator(batch):
    a, b = make(batch, seed=5), make(batch, seed=5)
    torch.manual_seed(1)
    la = a.step(batch)[0]
    torch.manual_seed(2)                                           # the global generator does not matter
    lb = b.step(batch)[0]
    assert torch.equal(la, lb)


def test_refused_keys_are_named(batch):
    stats = window_stats(batch)
    for over, key in ((dict(use_hf_collision_loss=True), "use_hf_collision_loss"), (dict(target_type="XY_POS"), "target_type"),
                      (dict(train_loss_fn="l1"), "train_loss_fn"), (dict(predict_mode="PREDICT_NOISE"), "predict_mode")):
        with pytest.raises(ValueError, match=key):
            MDMTrainer(train_cfg(**over), None, "cpu", loss=object(), feature_stats=stats)
    feats = dict(train_cfg()["features"], rot_type="ROT_6D")
    with pytest.raises(ValueError, match="rot_type"):
        MDMTrainer(train_cfg(features=feats), None, "cpu", loss=object(), feature_stats=stats)
    with pytest.raises(ValueError, match="feature_stats"):
        MDMTrainer(train_cfg(), None, "cpu", loss=object())
