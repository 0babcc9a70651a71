"""The generator's training loss without a GPU: the torch restatement ``mdm_loss_ref`` against the reference's
record ``tests/golden/mdm_loss.npz``, and the float32 restatement on every input of ``tests/test_mdm_loss_gpu.py`` within the bounds that
file holds the kernel to (so a failure there is the kernel's); the refusals the config decides."""
import os

import pytest
import torch

import mdm_loss_cases as MC
import mdm_loss_ref as LR
from parc_amd import motion_loss as ML

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOSS_FNS = ("squared_l2", "pseudo_huber")


@pytest.fixture(scope="module")
def fx():
    return LR.LossFixture(os.path.join(REPO, "tests/golden"))


@pytest.mark.parametrize("loss_fn", LOSS_FNS)
@pytest.mark.parametrize("group", ["a", "b"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_restatement_against_the_reference(fx, group, loss_fn, dtype):
    """Terms within 2e-5 |ref| + 1e-6, the gradient of the default-weighted total within 1e-4 max|g64| + 1e-6 per entry, and term by
    term for the row that has per-term gradients."""
    pred, true, td, mean, std = fx.inputs(group)
    ref = LR.MdmLossRef(fx.cfg(group), loss_fn, dtype, "cpu", mean, std)
    t64, _, g64, row, tg64 = fx.recorded(group, loss_fn)
    terms, grad = ref.terms_and_grad(pred, true, td)
    print(group, loss_fn, dtype, "terms", (terms.double() - t64).abs().max().item(), "grad", (grad.double() - g64).abs().max().item())
    assert MC.terms_ok(terms, t64)
    for r in range(pred.shape[0]):                                  # a row's gradient is its own: the bound is per row
        assert MC.grad_ok(grad[r], g64[r]), r
    _, tg = LR.term_grads(ref, pred[row:row + 1], LR.rows(true, slice(row, row + 1)), td[row:row + 1])
    for k in range(LR.NT):
        assert MC.grad_ok(tg[k, 0], tg64[k]), ML.TERM_NAMES[k]
    assert tg64[-1].abs().max() > 0 or group == "b"               # the target row of group a does not clamp, that of group b does


@pytest.mark.parametrize("loss_fn", LOSS_FNS)
def test_float32_restatement_meets_the_gpu_bounds_on_the_gpu_inputs(fx, loss_fn):
    for name, (cfg, pred, true, td, mean, std) in MC.cases(fx).items():
        r64 = LR.MdmLossRef(cfg, loss_fn, torch.float64, "cpu", mean, std)
        r32 = LR.MdmLossRef(cfg, loss_fn, torch.float32, "cpu", mean, std)
        t64, g64 = LR.term_grads(r64, pred, true, td)
        t32, g32 = LR.term_grads(r32, pred, true, td)
        assert torch.isfinite(t64).all() and torch.isfinite(g64).all(), name
        assert MC.terms_ok(t32, t64), (name, (t32.double() - t64).abs().max().item())
        for k in range(LR.NT if name not in MC.NO_GRAD_COMPARISON else 0):
            for r in range(pred.shape[0]):
                assert MC.grad_ok(g32[k, r], g64[k, r]), (name, ML.TERM_NAMES[k], r)


def test_cases_reach_what_they_are_for(fx):
    c = MC.cases(fx)
    cfg, pred, true, td, mean, std = c["a6"]
    r64 = LR.MdmLossRef(cfg, "squared_l2", torch.float64, "cpu", mean, std)
    t = r64.terms(pred.double(), true, td)
    clamped = t[:, -1] == -cfg["target_dir_len_eps"] * cfg["w_target"]
    assert clamped.any() and not clamped.all()
    e = pred[-1, :, 3:6] * std[:, 3:6] + mean[:, 3:6]
    assert (e.norm(dim=-1) > 3.2).all()                            # the root exp map of the last row lies beyond pi
    # pred == true: every angle term is masked to exactly 0 and so is its gradient; everything is finite
    cfg, pred, true, td, mean, std = c["clean"]
    t, g = LR.term_grads(LR.MdmLossRef(cfg, "squared_l2", torch.float64, "cpu", mean, std), pred, true, td)
    for k in (4, 5, 9):
        assert (t[:, k] == 0).all() and (g[k] == 0).all(), ML.TERM_NAMES[k]
    assert torch.isfinite(t).all() and torch.isfinite(g).all()
    # the double cover: negated true quaternions leave the values where they were
    cfg, pred, true, td, mean, std = c["negated"]
    assert MC.terms_ok(r64.terms(pred.double(), true, td), t64 := r64.terms(c["a6"][1].double(), c["a6"][2], td)) and t64.abs().max() > 0


def test_term_reaches_only_its_columns(fx):
    cfg, pred, true, td, mean, std = MC.cases(fx)["a6"]
    _, g = LR.term_grads(LR.MdmLossRef(cfg, "squared_l2", torch.float64, "cpu", mean, std), pred, true, td)
    B = 15
    con = slice(pred.shape[-1] - B, pred.shape[-1])
    k = ML.TERM_NAMES.index("SIMPLE_CONTACT_LOSS")
    assert (g[k][..., :con.start] == 0).all() and g[k][..., con].abs().max() > 0


def test_refusals_name_the_key(fx):
    cfg = fx.cfg("a")
    for over, key in ((dict(use_hf_collision_loss=True), "use_hf_collision_loss"), (dict(features=dict(cfg["features"], rot_type="QUAT")), "rot_type"),
                      (dict(features=dict(cfg["features"], frame_components=["ROOT_POS"])), "frame_components"), (dict(target_type="XY_POS"), "target_type")):
        with pytest.raises(ValueError, match=key):
            ML.check_loss_config(dict(cfg, **over))
    with pytest.raises(ValueError, match="train_loss_fn"):
        ML.check_loss_config(cfg, "l1")
    assert len(ML.TERM_NAMES) == len(ML.WEIGHT_KEYS) == ML.NUM_TERMS == 13


def test_autograd_bridge_on_the_restatement(fx):
    """``MotionLossFn`` around the float64 restatement: the per-window sums, ``terms`` without a gradient, backward = grad_out x grad."""
    pred, true, td, mean, std = fx.inputs("a")
    ref = LR.MdmLossRef(fx.cfg("a"), "squared_l2", torch.float64, "cpu", mean, std)
    x = pred[:4].clone().requires_grad_(True)
    loss, terms = ML.MotionLossFn.apply(x, ref, LR.rows(true, slice(0, 4)), td[:4])
    assert loss.shape == (4,) and not terms.requires_grad and loss.dtype == torch.float32
    loss.mean().backward()
    _, g = ref.terms_and_grad(pred[:4], LR.rows(true, slice(0, 4)), td[:4])
    assert torch.equal(x.grad, g.float() / 4)
