"""Training of the motion generator: the reference's ``MDM.train`` (``motion_generator/mdm.py:1010-1116``) with ``sample_and_compute_losses``,
``construct_conds``, ``forward_diffusion``, the EMA and ``save_checkpoint``.

``MDMDenoiser`` is the denoiser in training form, a ``torch.nn.Module`` whose ``state_dict()`` has the keys and shapes of
``motion_generator.tensor_order(cfg)``: a reference checkpoint loads into it and ``MDMGenerator.from_state_dict`` takes what it trains.
``MDMTrainer(cfg, sampler, device)`` takes the keys of the reference's ``parc_1_train_gen_default.yaml``; its loss is a
:class:`parc_amd.motion_loss.MotionLoss` (one fused kernel for the thirteen terms and their gradient) or any
object with its ``terms_and_grad``.  The network's forward and backward are PyTorch's; the windows come from
:class:`parc_amd.motion_sampler.MotionWindowSampler`.
"""
from __future__ import annotations

import copy
import os
import time
from typing import Dict, Optional

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from parc_amd import motion_generator as mg
from parc_amd.char_model import CharModel
from parc_amd.motion_loss import TERM_NAMES, MotionLossFn, check_loss_config

NUM_COND_TOKENS = 67   # time, 64 heightfield tokens, target, indicator


def _mlp(dims, dropout: float = 0.0) -> nn.Module:
    """Linear, Dropout, SiLU per hidden layer, then the last Linear, under ``.model`` (the keys ``model.{3 i}``)."""
    layers = []
    for i in range(len(dims) - 2):
        layers += [nn.Linear(dims[i], dims[i + 1]), nn.Dropout(dropout), nn.SiLU()]
    layers.append(nn.Linear(dims[-2], dims[-1]))
    m = nn.Module()
    m.model = nn.Sequential(*layers)
    return m


class _Table(nn.Module):
    """A sinusoidal table [1, rows, d_model] as the persistent buffer ``pe``."""

    def __init__(self, rows: int, d_model: int):
        super().__init__()
        self.register_buffer("pe", mg.positional_table(rows, d_model))


class MDMDenoiser(nn.Module):
    """The MDM denoiser (the network ``tests/mdm_ref.py`` restates and ``parc_mdm.hpp`` runs), with its dropouts: the transformer
    layers' own and the one after the positional table at ``cfg["dropout"]``; the MLPs' are 0 as in the reference.  Conditions are a
    dict keyed as ``MDMKeyType`` in the network's units: ``OBS_KEY`` [B, 31, 31] (heights / max_h), ``TARGET_KEY`` [B, 2],
    ``PREV_STATE_KEY`` [B, nprev, D] (standardised), the three flags and ``PREV_STATE_NOISE_IND_KEY`` [B] bool."""

    def __init__(self, cfg: dict, frame_dim: int):
        super().__init__()
        mg.check_config(cfg)
        d, dh, H = int(cfg["d_model"]), int(cfg["d_hid"]), int(cfg["num_heads"])
        self.d, self.T, self.nprev, self.D = d, int(cfg["seq_len"]), int(cfg["num_prev_states"]), int(frame_dim)
        p = float(cfg.get("dropout", 0.0))
        conv = nn.Module()
        conv._net = nn.Sequential(nn.Conv2d(1, 32, 5), nn.LeakyReLU(0.01), nn.Conv2d(32, 32, 5), nn.LeakyReLU(0.01), nn.Conv2d(32, 32, 5),
                                  nn.LeakyReLU(0.01), nn.Conv2d(32, 64, 4), nn.LeakyReLU(0.01))
        self._obs_conv_net = conv
        self._obs_embed = nn.Linear(256, d)
        self._embed_prev_state_noise_indicator = nn.Embedding(2, d)
        et = nn.Module()
        et.sequence_pos_encoder = _Table(int(cfg["diffusion_timesteps"]), d)
        et.time_embed = nn.Sequential(nn.Linear(d, d), nn.SiLU(), nn.Linear(d, d))
        self._embed_t = et
        self._in_pos_encoding = _Table(NUM_COND_TOKENS + self.T, d)
        self._pos_dropout = nn.Dropout(p)
        layer = nn.TransformerEncoderLayer(d, H, dh, p, activation="gelu", batch_first=True)
        self._transformer_encoder = nn.TransformerEncoder(layer, int(cfg["num_layers"]), enable_nested_tensor=False)
        self._in_mlp_target = _mlp([2] + list(cfg["target_mlp_layers"]) + [d])
        self._in_mlp_gen_seq = _mlp([self.D] + list(cfg["in_mlp_layers"]) + [d])
        self._out_mlp = _mlp([d] + list(cfg["out_mlp_layers"]) + [self.D])

    def embed_conds(self, conds: dict):
        """(tokens [B, 66, d]: heightfield, target, indicator; key-padding mask [B, 67 + T], True = the key is left out)"""
        c = mg._names(conds)
        hf = c["OBS_KEY"]
        n = hf.shape[0]
        obs, tgt_on, prev_on = c["OBS_FLAG_KEY"].bool(), c["TARGET_FLAG_KEY"].bool(), c["PREV_STATE_FLAG_KEY"].bool()
        mask = torch.zeros((n, NUM_COND_TOKENS + self.T), dtype=torch.bool, device=hf.device)
        h = self._obs_conv_net._net(hf.reshape(n, 1, mg.GRID, mg.GRID))
        tok = F.unfold(h, kernel_size=2, stride=2).permute(0, 2, 1)                         # [n, 64, 256]
        tok = self._obs_embed(tok) * obs.to(tok.dtype)[:, None, None]
        mask[:, 1:65] = ~obs[:, None]
        tgt = self._in_mlp_target.model(c["TARGET_KEY"].reshape(n, 1, 2)) * tgt_on.to(tok.dtype)[:, None, None]
        mask[:, 65] = ~tgt_on
        ind = self._embed_prev_state_noise_indicator(c["PREV_STATE_NOISE_IND_KEY"].to(torch.int64))[:, None]
        mask[:, NUM_COND_TOKENS:NUM_COND_TOKENS + self.nprev] = ~prev_on[:, None]
        return torch.cat([tok, tgt, ind], dim=1), mask

    def forward(self, x, conds: dict, t):
        """x_0 predicted from ``x`` [B, T, D] at timestep ``t`` (an int, or int64 [B]); where the indicator is set the first nprev
        frames the network reads are the clean previous state (``x`` itself is not changed)."""
        c = mg._names(conds)
        n = x.shape[0]
        tokens, mask = self.embed_conds(c)
        t = torch.as_tensor(t, device=x.device, dtype=torch.int64).reshape(-1).expand(n)
        tt = self._embed_t.time_embed(self._embed_t.sequence_pos_encoder.pe[0, t])[:, None]
        ind = c["PREV_STATE_NOISE_IND_KEY"].bool()
        head = torch.where(ind[:, None, None], c["PREV_STATE_KEY"][:, :self.nprev].to(x.dtype), x[:, :self.nprev])
        frames = self._in_mlp_gen_seq.model(torch.cat([head, x[:, self.nprev:]], dim=1))
        h = self._pos_dropout(torch.cat([tt, tokens, frames], dim=1) + self._in_pos_encoding.pe)
        h = self._transformer_encoder(h, src_key_padding_mask=mask)
        return self._out_mlp.model(h[:, NUM_COND_TOKENS:])


def sequence_length(cfg: dict) -> int:
    """The frames of a window: ``len(arange(0, sequence_duration, 1 / sequence_fps))`` as the sampler counts them."""
    if "seq_len" in cfg:
        return int(cfg["seq_len"])
    return int(torch.arange(start=0.0, end=float(cfg["sequence_duration"]), step=1.0 / cfg["sequence_fps"], dtype=torch.float32).shape[0])


def window_feature_stats(sampler, char_model: CharModel):
    """Mean and std [T, D] in the GENERATOR's layout (root exp map, joint dofs) over every window of every clip of the sampler
    (``MDM.compute_stats``, mdm.py:442-513).  ``sampler.feature_stats()`` itself is in the sampler's quaternion layout."""
    feats = torch.cat([mg.assemble_features(char_model, sampler.motion_sequences_for_id(i)) for i in range(len(sampler.clips))], dim=0)
    B, nd = char_model.get_num_bodies(), char_model.get_dof_size()
    return mg.feature_stats(feats, slice(6 + 3 * (B - 1) + nd, 6 + 3 * (B - 1) + nd + B))


def read_feature_stats(path: str):
    import yaml
    with open(path) as f:
        stats = yaml.safe_load(f)
    return torch.tensor(stats["mean"], dtype=torch.float32), torch.tensor(stats["std"], dtype=torch.float32)


class MDMTrainer:
    """See the module docstring.  ``loss`` / ``test_loss``: objects with ``terms_and_grad(pred, true_motion, target_dir)`` (and
    optionally ``set_stats(mean, std)``); by default :class:`MotionLoss` handles with ``train_loss_fn`` / ``test_loss_fn``.
    ``feature_stats``: ``(mean, std)`` [T, D], or the path of a ``feature_stats.yaml``; by default computed from the sampler's windows.
    Every random draw of a step (the sampler's seed, the flags, t, the noise, the indicator, the dropout masks) comes from one
    ``torch.Generator`` seeded with ``seed``."""

    def __init__(self, cfg: dict, sampler=None, device="cuda:0", loss=None, test_loss=None, feature_stats=None, seed: int = 0):
        cfg = dict(cfg)
        cfg["seq_len"] = sequence_length(cfg) if sampler is None or not hasattr(sampler, "cfg") else int(sampler.cfg.T)
        mg.check_config(cfg)
        check_loss_config(cfg, cfg.get("train_loss_fn", "squared_l2"))
        check_loss_config(cfg, cfg.get("test_loss_fn", "squared_l2"))
        self.cfg, self.sampler, self.device = cfg, sampler, torch.device(device)
        self.char_model = CharModel(mg._char_path(cfg))
        self.D = mg.frame_dim(self.char_model)
        self.T, self.nprev, self.timesteps = int(cfg["seq_len"]), int(cfg["num_prev_states"]), int(cfg["diffusion_timesteps"])
        self.batch_size, self.test_size = int(cfg.get("batch_size", 64)), int(cfg.get("test_size", 128))
        self.max_h = float(cfg["heightmap"]["max_h"])
        self.gen = torch.Generator(device=self.device)
        self.gen.manual_seed(int(seed))
        with torch.random.fork_rng(devices=self._rng_devices()):   # the initial weights are the generator's too
            torch.manual_seed(self._draw_seed())
            self.model = MDMDenoiser(cfg, self.D).to(self.device)
        ema = cfg.get("EMA") or None
        self.use_ema = bool(ema)
        self.ema_step = 0
        if self.use_ema:
            self.ema_decay, self.ema_start, self.ema_update_rate = float(ema["ema_decay"]), int(ema["ema_start"]), int(ema["ema_update_rate"])
            self.ema_model = copy.deepcopy(self.model)
        self.optimizer = torch.optim.AdamW(self.model.parameters(), lr=float(cfg["lr"]), weight_decay=float(cfg["weight_decay"]))
        self.rates = {k: v.to(self.device) for k, v in mg.diffusion_rates(self.timesteps).items()}
        if isinstance(feature_stats, (str, os.PathLike)):
            feature_stats = read_feature_stats(str(feature_stats))
        elif feature_stats is None:
            if sampler is None:
                raise ValueError("feature_stats: give (mean, std), a feature_stats.yaml, or a sampler to compute them from")
            feature_stats = window_feature_stats(sampler, self.char_model)
        mean, std = [torch.as_tensor(np.asarray(a.cpu() if isinstance(a, torch.Tensor) else a), dtype=torch.float32) for a in feature_stats]
        if mean.shape != std.shape or mean.dim() != 2 or mean.shape[0] < self.T or mean.shape[1] != self.D:
            raise ValueError(f"the feature mean / std must be [>= {self.T}][{self.D}] in the generator's layout (root exp map, joint dofs), not {list(mean.shape)}")
        self.mean, self.std = mean[:self.T].to(self.device), std[:self.T].to(self.device)
        if loss is None:
            from parc_amd.motion_loss import MotionLoss
            loss = MotionLoss(cfg, self.device, cfg.get("train_loss_fn", "squared_l2"), char_model=self.char_model)
            if test_loss is None and cfg.get("test_loss_fn", "squared_l2") != cfg.get("train_loss_fn", "squared_l2"):
                test_loss = MotionLoss(cfg, self.device, cfg["test_loss_fn"], char_model=self.char_model)
        self.loss, self.test_loss = loss, (test_loss if test_loss is not None else loss)
        for l in {id(self.loss): self.loss, id(self.test_loss): self.test_loss}.values():
            if hasattr(l, "set_stats"):
                l.set_stats(self.mean, self.std)
        self.num_samples = 0
        from parc_amd.util.logger import Logger
        self.logger = Logger()

    # ------------------------------------------------------------------ random draws
    def _rng_devices(self):
        return [self.device] if self.device.type == "cuda" else []

    def _draw_seed(self) -> int:
        return int(torch.randint(0, 2 ** 31 - 1, (1,), generator=self.gen, device=self.device).item())

    def _rand(self, n):
        return torch.rand((n,), generator=self.gen, device=self.device, dtype=torch.float32)

    def draw_noise_indicator(self, n):
        """mdm.py:699: true = the network reads the clean previous state."""
        return self._rand(n) < float(self.cfg["prev_state_noise_ind_chance"])

    # ------------------------------------------------------------------ features and conditions
    def standardize(self, f):
        return (f - self.mean[:f.shape[1]]) / self.std[:f.shape[1]]

    def forward_diffusion(self, x_0, t, noise):
        """mdm.py:777-788; ``t`` int64 [B]."""
        return self.rates["sqrt_alphas_cumprod"][t][:, None, None] * x_0 + self.rates["sqrt_one_minus_alphas_cumprod"][t][:, None, None] * noise

    def construct_conds(self, motion: dict, hfs, target_pos, target_rot, test: bool):
        """``MDM.construct_conds`` (mdm.py:515-566): (conditions in the network's units, x_0 standardised).  Training draws the
        previous-state, target and heightfield flags, in that order; a test has them all set."""
        x_0 = self.standardize(mg.assemble_features(self.char_model, motion).to(self.device))
        n = x_0.shape[0]
        cfg = self.cfg
        if test:
            prev_on = tgt_on = obs_on = torch.ones((n,), dtype=torch.bool, device=self.device)
        else:
            prev_on = ~(self._rand(n) < float(cfg["prev_state_attention_dropout"]))
            tgt_on = ~(self._rand(n) < float(cfg["target_dropout"]))
            obs_on = ~(self._rand(n) < float(cfg["obs_dropout"]))
        tdir = mg.target_dir(torch.as_tensor(target_pos, device=self.device), torch.as_tensor(target_rot, device=self.device),
                             float(cfg["target_dir_len_eps"]), float(cfg["target_dir_heading_eps"]))
        conds = {"OBS_KEY": torch.as_tensor(hfs, device=self.device).to(torch.float32) / self.max_h, "TARGET_KEY": tdir.to(torch.float32),
                 "PREV_STATE_KEY": x_0[:, :self.nprev], "OBS_FLAG_KEY": obs_on, "TARGET_FLAG_KEY": tgt_on.clone(), "PREV_STATE_FLAG_KEY": prev_on.clone()}
        return conds, x_0

    def _batch(self, batch, n):
        if batch is not None:
            return batch
        if self.sampler is None:
            raise ValueError("no sampler: give the batch")
        return self.sampler.sample(int(n), self._draw_seed())

    def _losses(self, batch, test: bool, loss_obj):
        """``sample_and_compute_loss`` (mdm.py:728-775) on one batch: (mean over the batch of the windows' sums, the terms' means [13])."""
        motion, hfs, tpos, trot = batch
        motion = mg._names(motion)
        with torch.no_grad():
            conds, x_0 = self.construct_conds(motion, hfs, tpos, trot, test)
            n = x_0.shape[0]
            t = torch.randint(0, self.timesteps, (n,), generator=self.gen, device=self.device)
            noise = torch.randn(x_0.shape, generator=self.gen, device=self.device, dtype=torch.float32)
            x_t = self.forward_diffusion(x_0, t, noise)
            conds["PREV_STATE_NOISE_IND_KEY"] = self.draw_noise_indicator(n)
            seed = self._draw_seed()
        with torch.random.fork_rng(devices=self._rng_devices()):
            torch.manual_seed(seed)                                 # the dropout masks
            pred = self.model(x_t, conds, t)
        per_window, terms = MotionLossFn.apply(pred, loss_obj, motion, conds["TARGET_KEY"])
        return per_window.mean(), terms.mean(dim=0)

    # ------------------------------------------------------------------ the loop
    def step(self, batch=None, update: bool = True):
        """One training iteration on ``batch`` (as ``sampler.sample`` returns it) or on a fresh one.  Returns (loss, terms [13]) as
        tensors; with ``update=False`` (the reference's ``test_only``) nothing is changed."""
        self.model.train()
        self.optimizer.zero_grad()
        loss, terms = self._losses(self._batch(batch, self.batch_size), False, self.loss)
        if update:
            loss.backward()
            self.grad_norm = nn.utils.clip_grad_norm_(self.model.parameters(), 1.0)
            self.optimizer.step()
            with torch.no_grad():
                self.update_ema()
        return loss.detach(), terms.detach()

    def update_ema(self):
        """mdm.py:278-285 and EMA.update_model_average: a copy before ``ema_start``, ``ema * decay + (1 - decay) * model`` from then on."""
        if not self.use_ema:
            return
        self.ema_step += 1
        if self.ema_step % self.ema_update_rate == 0:
            if self.ema_step < self.ema_start:
                self.ema_model.load_state_dict(self.model.state_dict())
            else:
                for e, p in zip(self.ema_model.parameters(), self.model.parameters()):
                    e.mul_(self.ema_decay).add_(p, alpha=1.0 - self.ema_decay)

    def evaluate(self, n: Optional[int] = None, batch=None):
        """The no-dropout, no-grad loss of ``sample_and_compute_loss(test=True)`` with the plain one-step prediction (the reference's
        ``test_mode: NONE``; its DDIM test loop is not built): every flag set, t and the noise drawn, the test loss function."""
        was = self.model.training
        self.model.eval()
        with torch.no_grad():
            loss, terms = self._losses(self._batch(batch, n or self.test_size), True, self.test_loss)
        self.model.train(was)
        return float(loss), {k: float(v) for k, v in zip(TERM_NAMES, terms)}

    def _log(self, loss, terms: Dict[str, float], epoch, start_time):
        lg = self.logger
        lg.log("epoch", epoch)
        lg.log("wall time", (time.time() - start_time) / 3600.0)
        lg.log("num samples", self.num_samples)
        lg.log("training loss", loss)
        for k, v in terms.items():
            lg.log(k, v)
        lg.print_log()
        lg.write_log()

    def train(self, epochs: Optional[int] = None, iters_per_epoch: Optional[int] = None, checkpoint_dir: Optional[str] = None, test_only: bool = False):
        """``MDM.train``: the initial test loss (logged as epoch -1), per epoch ``iters_per_epoch`` steps and one log row of the running
        means, ``model_<epoch>.ckpt`` every ``epochs_per_checkpoint`` epochs (epoch > 0), the final test loss; and, beyond the
        reference, ``model_final.ckpt`` at the end.  Returns the final test loss."""
        epochs = int(self.cfg["epochs"] if epochs is None else epochs)
        iters = int(self.cfg["iters_per_epoch"] if iters_per_epoch is None else iters_per_epoch)
        every = int(self.cfg.get("epochs_per_checkpoint", 0))
        if checkpoint_dir is not None:
            os.makedirs(checkpoint_dir, exist_ok=True)
            self.logger.configure_output_file(os.path.join(checkpoint_dir, "log.txt"))
        start = time.time()
        loss, terms = self.evaluate()
        self._log(loss, terms, -1, start)
        print("initial loss =", loss)
        for epoch in range(epochs):
            run_loss, run_terms = 0.0, torch.zeros(len(TERM_NAMES), device=self.device)
            for _ in range(iters):
                l, t = self.step(update=not test_only)
                run_loss += float(l)
                run_terms += t
            self.num_samples += self.batch_size * iters
            self._log(run_loss / iters, {k: float(v) / iters for k, v in zip(TERM_NAMES, run_terms)}, epoch, start)
            if not test_only and every > 0 and epoch % every == 0 and epoch > 0 and checkpoint_dir is not None:
                self.save_checkpoint(os.path.join(checkpoint_dir, f"model_{epoch}.ckpt"))
        final, _ = self.evaluate()
        print("final loss =", final)
        if not test_only and checkpoint_dir is not None:
            self.save_checkpoint(os.path.join(checkpoint_dir, "model_final.ckpt"))
        return final

    # ------------------------------------------------------------------ checkpoints
    def save_checkpoint(self, path):
        """The reference's layout (mdm.py:1161-1189: ``cfg``, ``model``, ``optimizer``, ``ema_model``, ``ema_meta``,
        ``extra._mdm_features_mean`` / ``_std``), which ``motion_generator.read_checkpoint`` reads, plus ``trainer``: what a resumed run
        needs to continue bit for bit (the generator's state, the counters)."""
        ck = {"cfg": self.cfg, "model": self.model.state_dict(), "optimizer": self.optimizer.state_dict(),
              "extra": {"_mdm_features_mean": self.mean.detach().cpu(), "_mdm_features_std": self.std.detach().cpu()},
              "trainer": {"generator_state": self.gen.get_state(), "ema_step": self.ema_step, "num_samples": self.num_samples}}
        if self.use_ema:
            ck["ema_model"] = self.ema_model.state_dict()
            ck["ema_meta"] = {"ema_step": self.ema_step, "ema_decay": self.ema_decay, "ema_start": self.ema_start, "ema_update_rate": self.ema_update_rate}
        torch.save(ck, str(path))

    def load(self, path):
        """Resume from a checkpoint of :meth:`save_checkpoint` or of the reference (``input_model_path``): the weights, the optimiser,
        the EMA, the feature statistics; and from this trainer's own files the generator's state and the counters."""
        ck = torch.load(str(path), map_location=self.device, weights_only=False)
        self.model.load_state_dict(ck["model"])
        if "optimizer" in ck:
            self.optimizer.load_state_dict(ck["optimizer"])
        if self.use_ema:
            self.ema_model.load_state_dict(ck.get("ema_model", ck["model"]))
            self.ema_step = int((ck.get("ema_meta") or {}).get("ema_step") or 0)
        extra = ck.get("extra", {})
        if "_mdm_features_mean" in extra:
            self.mean = torch.as_tensor(np.asarray(extra["_mdm_features_mean"].cpu() if isinstance(extra["_mdm_features_mean"], torch.Tensor)
                                                   else extra["_mdm_features_mean"]), dtype=torch.float32)[:self.T].to(self.device)
            self.std = torch.as_tensor(np.asarray(extra["_mdm_features_std"].cpu() if isinstance(extra["_mdm_features_std"], torch.Tensor)
                                                  else extra["_mdm_features_std"]), dtype=torch.float32)[:self.T].to(self.device)
            for l in {id(self.loss): self.loss, id(self.test_loss): self.test_loss}.values():
                if hasattr(l, "set_stats"):
                    l.set_stats(self.mean, self.std)
        tr = ck.get("trainer")
        if tr is not None:
            self.gen.set_state(tr["generator_state"].cpu())
            self.ema_step, self.num_samples = int(tr["ema_step"]), int(tr["num_samples"])
