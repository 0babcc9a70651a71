"""The motion optimiser's torch restatement (tests/motion_opt_ref.py), one loss term at a time (no GPU).

(1) Against the reference: ``tests/golden/motion_opt_terms.npz`` holds the reference's loss dict and autograd gradient at state b of both
fixtures with each weight on alone.  The restatement, in float64 and in float32, is held to it per term on EVERY gradient entry
(``1e-4 max|g_ref| + 1e-6``) and on the term values (``2e-5 |ref| + 1e-6``).  Under the total-gradient bound of test_motion_opt_cpu.py
(7 to 14 absolute) the six small terms could be wrong unseen.

(2) The inputs of tests/test_motion_opt_terms_gpu.py: on every case of tests/motion_opt_cases.py the float32 restatement is within the
per-term gradient bound of the float64 one on every entry, and each case's input conditions hold.  The float64 evaluation is the GPU
tests' reference; that its own float32 evaluation meets the bound shows that the inputs stay clear of argmin, clamp and floor / ceil
flips, where no bound on rounding could hold.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import motion_opt_cases as MC  # noqa: E402

DTYPES = {"float64": torch.float64, "float32": torch.float32}


@pytest.fixture(scope="module")
def record():
    return dict(np.load(os.path.join(MC.REPO, "tests/golden/motion_opt_terms.npz")))


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("t", range(9), ids=MC.TERM_NAMES)
@pytest.mark.parametrize("name,case", [(MC.TEASER, "teaser_whole"), (MC.CIVILIZATION, "C")])
def test_restatement_matches_reference_term_by_term(record, name, case, t, dtype):
    ref_t, ref_g = record["terms_" + MC.CLIP_NAMES[name]][t], record["grad_" + MC.CLIP_NAMES[name]][t].astype(np.float64)
    terms, grad = MC.evaluate(MC.case(case), 0, t, DTYPES[dtype])
    assert ref_t[t] > 0 and (ref_g != 0).sum() >= 10
    err_t, err_g = np.abs(terms - ref_t), np.abs(grad - ref_g)
    print(f"{case} {MC.TERM_NAMES[t]} {dtype}: gradient error {err_g.max() / MC.grad_bound(ref_g):.3f} of the bound, "
          f"terms {(err_t / MC.term_bound(ref_t)).max():.3f}")
    assert (err_t <= MC.term_bound(ref_t)).all(), (terms, ref_t)
    assert (err_g <= MC.grad_bound(ref_g)).all(), (np.argwhere(err_g > MC.grad_bound(ref_g))[:10], err_g.max(), MC.grad_bound(ref_g))


@pytest.mark.parametrize("name", MC.GPU_CASE_NAMES)
def test_gpu_inputs_are_sound(name):
    case = MC.case(name)
    if case.check is not None:
        case.check(case)
    for i in range(len(case.clips)):
        for t in case.terms:
            t64, g64 = MC.evaluate(case, i, t, torch.float64)
            t32, g32 = MC.evaluate(case, i, t, torch.float32)
            err = np.abs(g32 - g64)
            print(f"{name} clip {i} {MC.TERM_NAMES[t]}: float32 restatement {err.max() / MC.grad_bound(g64):.3f} of the gradient bound")
            assert np.isfinite(g64).all() and np.isfinite(t64).all()
            assert (err <= MC.grad_bound(g64)).all(), (name, i, t, err.max(), MC.grad_bound(g64))
            assert (np.abs(t32 - t64) <= MC.term_bound(t64)).all(), (name, i, t, t32, t64)


@pytest.mark.parametrize("t", range(9), ids=MC.TERM_NAMES)
@pytest.mark.parametrize("name", ["T", "C"])
def test_each_term_alone_is_active(name, t):
    terms, g = MC.evaluate(MC.case(name), 0, t)
    assert terms[t] > 0 and (g != 0).sum() >= 10, (terms[t], (g != 0).sum())
    keep = {MC.ROOT_POS: slice(0, 3), MC.ROOT_ROT: slice(3, 6), MC.JOINT_ROT: slice(6, None)}.get(t)
    if keep is not None:       # what the term cannot reach is exactly zero
        rest = g.copy()
        rest[:, keep] = 0
        assert (rest == 0).all()


def test_equivalent_inputs_have_equal_terms():
    """A negated source quaternion and an exp map wrapped past pi are the same rotations: the term values of T, other gradients."""
    base = MC.case("T")
    for name in ("double_cover", "wrapped_exp_maps"):
        case = MC.case(name)
        for t in case.terms:
            a, b = MC.evaluate(case, 0, t)[0], MC.evaluate(base, 0, t)[0]
            assert abs(a[t] - b[t]) <= MC.term_bound(b[t]), (name, t, a[t], b[t])    # the wrapped parameters are rounded to float32
    g_w, g_t = MC.evaluate(MC.case("wrapped_exp_maps"), 0, MC.ROOT_ROT)[1], MC.evaluate(base, 0, MC.ROOT_ROT)[1]
    assert np.abs(g_w - g_t).max() > 0.01 * np.abs(g_t).max()        # d/de at the wrapped point is another gradient


def test_short_clips_have_no_windows():
    case = MC.case("short_clips")
    for i, clip in enumerate(case.clips):
        F = clip.num_frames
        assert F == i + 1
        for t in ([MC.JERK] if F <= 3 else []) + ([MC.SMOOTH, MC.SLIDING] if F == 1 else []):
            terms, g = MC.evaluate(case, i, t)
            assert terms[t] == 0 and (g == 0).all()
        terms, g = MC.evaluate(case, i, MC.BODYCONS)
        assert terms[MC.BODYCONS] > 0 and (g != 0).any()
    terms, g = MC.evaluate(case, 4, MC.JERK)
    assert terms[MC.JERK] > 0 and (g != 0).any()


def test_ignored_constraints_change_nothing():
    a, b = MC.case("constraints"), MC.case("constraints_plain")
    assert len(a.clips[0].cons_body) == len(b.clips[0].cons_body) + 2
    for t in a.terms:
        (ta, ga), (tb, gb) = MC.evaluate(a, 0, t), MC.evaluate(b, 0, t)
        assert np.array_equal(ta, tb) and np.array_equal(ga, gb)
