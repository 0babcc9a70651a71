"""The generator's trainer on the GPU, end to end at the MDM fixture's small shape (d_model 64, 2 layers, batch 16)
on the bundled clips: steps lower the loss, the checkpoint feeds ``MDMGenerator``, the HIP inference agrees with the module that was
trained, and ``scripts/train_generator.py`` runs."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from parc_amd import motion_generator as mg
from parc_amd.util import path_loader

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
CONFIG = os.path.join(REPO, "data/configs/mdm_train/mdm_train_default.yaml")
SMALL = dict(d_model=64, num_heads=4, d_hid=64, num_layers=2, target_mlp_layers=[32], in_mlp_layers=[64], out_mlp_layers=[64], batch_size=16,
             test_size=16, lr=1e-3, dropout=0.0, obs_dropout=0.0, target_dropout=0.0, prev_state_attention_dropout=0.0, use_target_loss=True)
K = 7.68   # tests/test_mdm_gpu.py: HIP against torch is held to K times the fp32 yardstick's own error, plus 1e-6


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    from parc_amd import motion_lib
    from parc_amd import motion_sampler as ms
    from parc_amd.motion_trainer import MDMTrainer
    cfg = dict(path_loader.load_config(CONFIG), **SMALL)
    T = ms.parse_config(cfg).T
    clips = motion_lib.load_motion_file(str(path_loader.resolve_path(cfg["motion_lib_file"])), verbose=False)
    sampler = ms.MotionWindowSampler(cfg, str(path_loader.resolve_path(cfg["motion_lib_file"])), os.path.join(REPO, cfg["char_file"]), DEV,
                                     exclude=[c.name for c in clips if c.num_frames - T <= 0])
    tr = MDMTrainer(cfg, sampler, DEV, seed=0)
    batch = sampler.sample(16, 7)
    tr.gen.manual_seed(5)
    first = tr.evaluate(batch=batch)[0]
    losses = [float(tr.step(batch)[0]) for _ in range(30)]
    tr.gen.manual_seed(5)
    last = tr.evaluate(batch=batch)[0]
    path = tmp_path_factory.mktemp("ckpt") / "model.ckpt"
    tr.save_checkpoint(path)
    return tr, batch, first, last, losses, path


def test_thirty_steps_lower_the_loss_of_their_batch(trained):
    tr, batch, first, last, losses, _ = trained
    print("evaluate before %.4f after %.4f; training loss %.4f -> %.4f" % (first, last, losses[0], losses[-1]))
    assert np.isfinite(losses).all() and last < first
    assert tr.loss.kernel_times()["loss"] > 0                      # the loss ran as the kernel
    assert tr.mean.shape == (15, 91) and float(tr.std.min()) >= float(np.float32(1e-5))   # the clamp of compute_stats, in fp32


def test_checkpoint_feeds_the_generator_and_the_kernels_agree_with_the_module(trained):
    tr, batch, _, _, _, path = trained
    from parc_amd.motion_trainer import MDMDenoiser
    gen = mg.MDMGenerator.load_checkpoint(path, device=DEV, max_batch=16)
    assert torch.equal(gen.mean.cpu(), tr.mean.cpu())
    motion, hfs, tp, trot = batch
    conds, x_0 = tr.construct_conds(motion, hfs, tp, trot, test=True)
    conds["PREV_STATE_NOISE_IND_KEY"] = torch.arange(16, device=DEV) % 2 == 0
    g = torch.Generator().manual_seed(1)
    x = torch.randn(x_0.shape, generator=g).to(DEV)
    gen.embed_conds(conds)
    hip = gen.forward(x.clone(), 10)
    cpu = {k: v.cpu() for k, v in conds.items()}
    sd = {k: v.cpu() for k, v in tr.model.state_dict().items()}
    m32 = MDMDenoiser(tr.cfg, 91).eval()
    m32.load_state_dict(sd)
    m64 = MDMDenoiser(tr.cfg, 91).double().eval()
    m64.load_state_dict({k: v.double() for k, v in sd.items()})
    with torch.no_grad():
        y32 = m32(x.cpu(), cpu, 10)
        y64 = m64(x.cpu().double(), {k: (v.double() if v.is_floating_point() else v) for k, v in cpu.items()}, 10)
        dev32 = tr.model.eval()(x, conds, 10)
    ref_err, err = (y32.double() - y64).abs().max().item(), (hip.cpu().double() - y64).abs().max().item()
    print("module fp32 - float64 %.3e   HIP - float64 %.3e   module on the GPU - float64 %.3e" % (ref_err, err, (dev32.cpu().double() - y64).abs().max().item()))
    assert ref_err <= 1e-4 and err <= K * ref_err + 1e-6


def test_train_script_writes_a_loadable_checkpoint(tmp_path):
    import yaml
    cfg = dict(path_loader.load_config(CONFIG), **SMALL)
    cfg_path = tmp_path / "cfg.yaml"
    cfg_path.write_text(yaml.safe_dump(cfg))
    r = subprocess.run([sys.executable, os.path.join(REPO, "scripts/train_generator.py"), "--config", str(cfg_path), "--epochs", "1", "--iters_per_epoch", "2",
                        "--checkpoint_dir", str(tmp_path / "out")], capture_output=True, text=True, cwd=REPO, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "final test loss" in r.stdout
    gen = mg.MDMGenerator.load_checkpoint(tmp_path / "out" / "model_final.ckpt", device=DEV, max_batch=4)
    assert gen.T == 15 and gen.D == 91
    assert (tmp_path / "out" / "log.txt").read_text().count("\n") >= 3   # the header, the initial loss, the epoch
