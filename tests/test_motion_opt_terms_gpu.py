"""The motion optimiser's kernels (parc_mopt_*), one loss term at a time, against the float64 torch restatement (tests/motion_opt_ref.py).

test_motion_opt_gpu.py compares the gradient of the weighted total; its bound, 1e-4 of the largest entry, is 7 to 14 in absolute terms
and hides the backward pass of six of the nine terms.  Here one handle per one-hot weight vector isolates a term:
every gradient entry within ``1e-4 max|g64| + 1e-6`` of the float64 restatement of that term, the term values within
``2e-5 |ref| + 1e-6``.  The inputs come from tests/motion_opt_cases.py; tests/test_motion_opt_terms_cpu.py shows on each of them that the
float32 restatement meets the same bound, so a failure here is the kernel's.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import motion_opt_cases as MC  # noqa: E402
from parc_amd import motion_opt as mo  # noqa: E402

pytestmark = pytest.mark.gpu

_HANDLES, _RUNS = {}, {}


def handle(t, sampler="stage2"):
    """The optimiser with only weight ``t`` on (weights are fixed when the handle is created)."""
    if (t, sampler) not in _HANDLES:
        cfg = MC.one_hot(t)
        if sampler != "stage2":
            cfg["char_point_samples"] = MC.SAMPLERS[sampler]
        _HANDLES[t, sampler] = mo.MotionOptimizer(MC.CHAR, "cuda:0", cfg)
    return _HANDLES[t, sampler]


def run(name, t):
    """The kernel's terms [clips, 9] and gradient [frames, 6 + D] on a case with weight ``t`` on alone."""
    if (name, t) not in _RUNS:
        case = MC.case(name)
        opt = handle(t, case.sampler)
        opt.set_clips(case.clips)
        opt.set_params(case.params)
        _RUNS[name, t] = opt.loss_and_grad()
    return _RUNS[name, t]


def compare(name, t):
    """Kernel against the float64 restatement of every clip of the case alone: every gradient entry, all nine term values."""
    case = MC.case(name)
    if case.check is not None:
        case.check(case)
    terms, grad = run(name, t)
    off = case.offsets()
    assert np.isfinite(grad).all() and np.isfinite(terms).all()
    for i in range(len(case.clips)):
        t64, g64 = MC.evaluate(case, i, t)
        g = grad[off[i]:off[i + 1]].astype(np.float64)
        err_g, err_t = np.abs(g - g64), np.abs(terms[i].astype(np.float64) - t64)
        print(f"{name} clip {i} {MC.TERM_NAMES[t]}: gradient error {err_g.max():.3g} = {err_g.max() / MC.grad_bound(g64):.3f} of the bound, "
              f"terms {(err_t / MC.term_bound(t64)).max():.3f} of theirs")
        assert (err_t <= MC.term_bound(t64)).all(), (name, i, terms[i], t64)
        bad = err_g > MC.grad_bound(g64)
        assert not bad.any(), (name, i, MC.TERM_NAMES[t], np.argwhere(bad)[:10], err_g.max(), MC.grad_bound(g64))
    return terms, grad


# ---- 1. each term alone ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", range(9), ids=MC.TERM_NAMES)
@pytest.mark.parametrize("name", ["T", "C"])
def test_each_term_alone(name, t):
    t64, g64 = MC.evaluate(MC.case(name), 0, t)
    assert t64[t] > 0 and (g64 != 0).sum() >= 10
    _, grad = compare(name, t)
    keep = {MC.ROOT_POS: slice(0, 3), MC.ROOT_ROT: slice(3, 6), MC.JOINT_ROT: slice(6, None)}.get(t)
    if keep is not None:       # what the term cannot reach is exactly zero
        rest = grad.copy()
        rest[:, keep] = 0
        assert (rest == 0).all(), np.argwhere(rest != 0)[:10]


# ---- 2, 3. the same rotations written differently -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,t", [c for c in MC.COMPARISONS if c[0] in ("double_cover", "wrapped_exp_maps")],
                         ids=lambda v: MC.TERM_NAMES[v] if isinstance(v, int) else v)
def test_negated_sources_and_wrapped_exp_maps(name, t):
    terms, _ = compare(name, t)
    base = MC.evaluate(MC.case("T"), 0, t)[0]            # the term values are those of T itself
    assert abs(float(terms[0, t]) - base[t]) <= MC.term_bound(base[t]), (terms[0, t], base[t])


# ---- 4, 5, 8, 9. terrain edges, tiny terrains, contact labels, the small sampler --------------------------------------------------------------
@pytest.mark.parametrize("name,t", [c for c in MC.COMPARISONS if c[0] in ("edge_straddle_px", "edge_off_mx", "edge_off_py", "tiny_terrain_2x3",
                                                                           "tiny_terrain_1x1", "contact_labels", "small_sampler")],
                         ids=lambda v: MC.TERM_NAMES[v] if isinstance(v, int) else v)
def test_edges(name, t):
    compare(name, t)


def test_small_sampler_points_are_the_fixtures():
    opt = handle(MC.PEN, "motion_opt")
    z = MC.fixture(MC.TEASER)
    assert opt.points.shape == (108, 3) and opt.points.shape[0] < 256
    np.testing.assert_array_equal(opt.point_body, z["pts_motion_opt_body"])
    np.testing.assert_allclose(opt.points, z["pts_motion_opt"], rtol=0, atol=1e-6)    # test_sampler_matches_reference's bound
    np.testing.assert_array_equal(opt.points, MC.sample_points("motion_opt")[0])       # and exactly what the restatement is given


# ---- 6. short clips in one batch ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", MC.case("short_clips").terms, ids=lambda t: MC.TERM_NAMES[t])
@pytest.mark.parametrize("name", ["short_clips", "short_clips_reversed"])
def test_short_clips_in_one_batch(name, t):
    case = MC.case(name)
    terms, grad = compare(name, t)          # each clip against the restatement of that clip ALONE: a neighbour's frames must not leak in
    off = case.offsets()
    for i, clip in enumerate(case.clips):
        F = clip.num_frames
        if (t == MC.JERK and F <= 3) or (t in (MC.SMOOTH, MC.SLIDING) and F == 1):
            assert terms[i, t] == 0 and (grad[off[i]:off[i + 1]] == 0).all(), (F, terms[i, t])
    assert sorted(c.num_frames for c in case.clips) == [1, 2, 3, 4, 5]


# ---- 7. constraints ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [MC.BODYCONS, MC.SLIDING], ids=lambda t: MC.TERM_NAMES[t])
def test_constraints(t):
    terms, grad = compare("constraints", t)
    plain_terms, plain_grad = compare("constraints_plain", t)
    # a constraint on a capsule body and one with start > end contribute nothing, to the bit
    assert np.array_equal(terms, plain_terms) and np.array_equal(grad, plain_grad)


# ---- 10. Adam past step one ------------------------------------------------------------------------------------------------------------------
def test_adam_twelve_steps():
    import torch
    case = MC.case("T")
    clip, p0 = case.clips[0], case.params
    opt = handle(MC.ROOT_POS)
    opt.set_clips(case.clips)
    opt.set_params(p0)
    opt.step(5)
    opt.step(7)
    got = opt.get_params()
    # the gradient of this term is 2 (rp - src): torch.optim.Adam in float32 on the same loss is the reference
    p = torch.tensor(p0, requires_grad=True)
    src = torch.tensor(clip.root_pos)
    adam = torch.optim.Adam([p], lr=MC.one_hot(MC.ROOT_POS)["step_size"])
    for _ in range(12):
        adam.zero_grad()
        (float(MC.fixture(MC.TEASER)["weights"][MC.ROOT_POS]) * ((p[:, :3] - src) ** 2).sum()).backward()
        adam.step()
    ref = p.detach().numpy()
    err = np.abs(got - ref).max()
    print(f"12 Adam steps: max error {err:.3g} (bound 1.2e-6), moved by {np.abs(ref - p0).max():.3g}")
    assert np.abs(ref[:, :3] - p0[:, :3]).max() > 5e-3        # twelve steps of ~1e-3
    assert err <= 1.2e-6                                        # the one-step bound of 1e-7, twelve times
    assert np.array_equal(got[:, 3:].view(np.int32), p0[:, 3:].view(np.int32))
    opt.set_params(p0)                                          # resets the moments and the step count
    opt.step(12)
    assert np.array_equal(opt.get_params().view(np.int32), got.view(np.int32))
