"""The generator's training-loss kernel on the GPU against the reference's record (``tests/golden/mdm_loss.npz``) and
against the float64 restatement ``mdm_loss_ref``, one weight on at a time, on the shapes of ``mdm_loss_cases``.  Bounds: a term within
2e-5 |ref| + 1e-6, a gradient entry within 1e-4 max|g64| + 1e-6 of its row's yardstick (``tests/test_mdm_loss_cpu.py`` holds the float32
restatement to both on the same inputs).  Reads only ``tests/golden/`` and the bundled data."""
import os

import pytest
import torch

import mdm_loss_cases as MC
import mdm_loss_ref as LR
from parc_amd import motion_loss as ML

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
LOSS_FNS = ("squared_l2", "pseudo_huber")


@pytest.fixture(scope="module")
def fx():
    return LR.LossFixture(os.path.join(REPO, "tests/golden"))


@pytest.fixture(scope="module")
def cases(fx):
    return MC.cases(fx)


@pytest.fixture(scope="module")
def yardstick(cases):
    """Per (case, loss function): the float64 restatement's terms [N, 13] and per-term gradients [13, N, T, D], computed once."""
    out = {}
    for name, (cfg, pred, true, td, mean, std) in cases.items():
        for fn in LOSS_FNS:
            out[name, fn] = LR.term_grads(LR.MdmLossRef(cfg, fn, torch.float64, "cpu", mean, std), pred, true, td)
    return out


def dev(true):
    return {k: v.to(DEV) for k, v in true.items()}


def run(cfg, fn, pred, true, td, mean, std):
    ml = ML.MotionLoss(cfg, DEV, fn, mean, std)
    terms, grad = ml.terms_and_grad(pred.to(DEV), dev(true), td.to(DEV))
    return terms.cpu(), grad.cpu()


@pytest.mark.parametrize("loss_fn", LOSS_FNS)
@pytest.mark.parametrize("group", ["a", "b"])
def test_kernel_against_the_reference(fx, group, loss_fn):
    """Term values, the gradient of the default-weighted total, and the per-term gradients of the recorded row."""
    pred, true, td, mean, std = fx.inputs(group)
    t64, _, g64, row, tg64 = fx.recorded(group, loss_fn)
    terms, grad = run(fx.cfg(group), loss_fn, pred, true, td, mean, std)
    print(group, loss_fn, "terms", (terms.double() - t64).abs().max().item(), "grad", (grad.double() - g64).abs().max().item())
    assert MC.terms_ok(terms, t64)
    for r in range(pred.shape[0]):
        assert MC.grad_ok(grad[r], g64[r]), r
    for k in range(ML.NUM_TERMS):
        tk, gk = run(LR.only_weight(fx.cfg(group), k), loss_fn, pred[row:row + 1], LR.rows(true, slice(row, row + 1)), td[row:row + 1], mean, std)
        assert MC.grad_ok(gk[0], tg64[k]), ML.TERM_NAMES[k]
        assert MC.terms_ok(tk[0, k], t64[row, k]) and (tk[0, [i for i in range(ML.NUM_TERMS) if i != k]] == 0).all()


@pytest.mark.parametrize("loss_fn", LOSS_FNS)
@pytest.mark.parametrize("case", ["n1", "t2", "t3", "t20", "negated", "beyond_pi", "a6"])
def test_kernel_against_the_restatement_one_weight_at_a_time(cases, yardstick, case, loss_fn):
    cfg, pred, true, td, mean, std = cases[case]
    t64, g64 = yardstick[case, loss_fn]
    for k in range(ML.NUM_TERMS):
        terms, grad = run(LR.only_weight(cfg, k), loss_fn, pred, true, td, mean, std)
        assert MC.terms_ok(terms[:, k], t64[:, k]), (ML.TERM_NAMES[k], (terms[:, k].double() - t64[:, k]).abs().max().item())
        for r in range(pred.shape[0]):
            assert MC.grad_ok(grad[r], g64[k, r]), (ML.TERM_NAMES[k], r)


def test_double_cover_leaves_the_values(cases, yardstick):
    cfg, pred, true, td, mean, std = cases["negated"]
    terms, _ = run(cfg, "squared_l2", pred, true, td, mean, std)
    assert MC.terms_ok(terms, yardstick["a6", "squared_l2"][0])


def test_a_window_is_bit_identical_alone_or_in_a_batch_of_65(cases):
    cfg, pred, true, td, mean, std = cases["a6"]
    idx = torch.arange(65) % pred.shape[0]
    ml = ML.MotionLoss(cfg, DEV, "pseudo_huber", mean, std)
    t65, g65 = ml.terms_and_grad(pred[idx].to(DEV), dev(LR.rows(true, idx)), td[idx].to(DEV))
    for r in (0, 5, 64):
        i = int(idx[r])
        t1, g1 = ml.terms_and_grad(pred[i:i + 1].to(DEV), dev(LR.rows(true, slice(i, i + 1))), td[i:i + 1].to(DEV))
        assert torch.equal(t1[0], t65[r]) and torch.equal(g1[0], g65[r])
    assert torch.equal(t65[:6], t65[6:12]) and torch.equal(g65[59:65], g65[5:11])


def test_a_nan_row_poisons_only_itself(cases):
    cfg, pred, true, td, mean, std = cases["a6"]
    ml = ML.MotionLoss(cfg, DEV, "squared_l2", mean, std)
    t0, g0 = ml.terms_and_grad(pred.to(DEV), dev(true), td.to(DEV))
    bad = pred.clone()
    bad[2, 7, 0] = float("nan")                                    # a position: a NaN exp map is masked to the identity, as in the reference
    t1, g1 = ml.terms_and_grad(bad.to(DEV), dev(true), td.to(DEV))
    keep = [0, 1, 3, 4, 5]
    assert torch.equal(t0[keep], t1[keep]) and torch.equal(g0[keep], g1[keep])
    assert torch.isnan(t1[2]).any() and torch.isnan(g1[2]).any()


@pytest.mark.parametrize("loss_fn", LOSS_FNS)
def test_pred_equal_to_true_is_masked_to_exact_zeros(cases, loss_fn):
    cfg, pred, true, td, mean, std = cases["clean"]
    terms, grad = run(cfg, loss_fn, pred, true, td, mean, std)
    assert torch.isfinite(terms).all() and torch.isfinite(grad).all()
    for k in (4, 5, 9):                                            # the angle terms: masked at |v| <= 1e-5
        tk, gk = run(LR.only_weight(cfg, k), "squared_l2", pred, true, td, mean, std)
        assert (tk == 0).all() and (gk == 0).all(), ML.TERM_NAMES[k]


def test_target_gradient_is_exactly_zero_where_it_clamps(cases):
    cfg, pred, true, td, mean, std = cases["a6"]
    k = ML.NUM_TERMS - 1
    terms, grad = run(LR.only_weight(cfg, k), "squared_l2", pred, true, td, mean, std)
    clamped = terms[:, k] == torch.tensor(-cfg["target_dir_len_eps"], dtype=torch.float32) * torch.tensor(cfg["w_target"], dtype=torch.float32)
    assert clamped.any() and not clamped.all()
    assert (grad[clamped] == 0).all() and (grad[~clamped].abs().amax(dim=(1, 2)) > 0).all()
    assert (grad[..., 2:] == 0).all()                              # the target reaches the root's x and y alone


def test_use_pos_loss_off_zeroes_the_fk_terms_and_leaves_the_rest(cases):
    cfg, pred, true, td, mean, std = cases["a6"]
    off = dict(cfg, use_pos_loss=False)
    t_off, g_off = run(off, "squared_l2", pred, true, td, mean, std)
    rest = dict(cfg, **{ML.WEIGHT_KEYS[k]: 0.0 for k in ML.FK_TERMS})
    t_rest, g_rest = run(rest, "squared_l2", pred, true, td, mean, std)
    assert (t_off[:, list(ML.FK_TERMS)] == 0).all()
    assert torch.equal(t_off, t_rest) and torch.equal(g_off, g_rest)


def test_a_term_reaches_only_its_columns(cases):
    cfg, pred, true, td, mean, std = cases["a6"]
    D, B = pred.shape[-1], 15
    reach = {"SIMPLE_CONTACT_LOSS": slice(D - B, D), "SIMPLE_ROOT_POS_LOSS": slice(0, 3), "VEL_ROOT_POS_LOSS": slice(0, 3),
             "SIMPLE_ROOT_ROT_LOSS": slice(3, 6), "VEL_ROOT_ROT_LOSS": slice(3, 6), "SIMPLE_BODY_POS_LOSS": slice(6, 6 + 3 * (B - 1)),
             "SIMPLE_JOINT_ROT_LOSS": slice(6 + 3 * (B - 1), D - B), "VEL_JOINT_ROT_LOSS": slice(6 + 3 * (B - 1), D - B)}
    for name, sl in reach.items():
        _, g = run(LR.only_weight(cfg, ML.TERM_NAMES.index(name)), "squared_l2", pred, true, td, mean, std)
        outside = torch.ones(D, dtype=torch.bool)
        outside[sl] = False
        assert (g[..., outside] == 0).all() and g[..., sl].abs().max() > 0, name


def test_autograd_bridge(cases):
    cfg, pred, true, td, mean, std = cases["a6"]
    ml = ML.MotionLoss(cfg, DEV, "squared_l2", mean, std)
    x = pred[:4].to(DEV).requires_grad_(True)
    t4 = dev(LR.rows(true, slice(0, 4)))
    loss, terms = ML.MotionLossFn.apply(x, ml, t4, td[:4].to(DEV))
    assert loss.shape == (4,) and not terms.requires_grad and terms.shape == (4, ML.NUM_TERMS)
    loss.mean().backward()
    t, g = ml.terms_and_grad(x.detach(), t4, td[:4].to(DEV))
    assert torch.equal(x.grad, g / 4) and torch.equal(loss.detach(), t.sum(dim=-1))


def test_refusals_of_the_handle(cases):
    cfg, pred, true, td, mean, std = cases["a6"]
    with pytest.raises(ValueError, match="use_hf_collision_loss"):
        ML.MotionLoss(dict(cfg, use_hf_collision_loss=True), DEV)
    ml = ML.MotionLoss(cfg, DEV, "squared_l2", mean, std)
    from parc_amd.lib import ParcError
    with pytest.raises(ParcError, match="num_frames"):
        ml.terms_and_grad(pred[:, :1].to(DEV), dev({k: v[:, :1] for k, v in true.items()}), td.to(DEV))
