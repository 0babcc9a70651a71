"""Contact labelling, penetration lift and resampling on the GPU (parc_mlabel_*) against the reference fixtures
(tests/golden/make_golden_motion_label.py) and the float64 restatement (tests/motion_label_ref.py).

A decision is settled when its margin is at least 1e-4 m (and, for a foot, no corner lies within 1e-4 cell of a boundary between cells
of different height): twenty times the error of an fp32 FK at these positions, so the kernel's flag must equal the reference's there.
At most 2 % of a case's decisions are unsettled.  Values are compared within max(1e-5, 4 x the difference between the reference's fp32
result and the restatement, recorded in the fixture); nothing is measured against the kernels."""
import os
from dataclasses import replace

import numpy as np
import pytest

import motion_label_ref as mr
from conftest import REPO
from parc_amd import motion_label as ml
from parc_amd import motion_opt as mo
from parc_amd.lib import ParcError

pytestmark = pytest.mark.gpu

CHAR = os.path.join(REPO, "data/assets/humanoid.xml")
DEV = "cuda:0"
OUTPUTS = ("contacts", "gap", "lift", "hand_sd", "root_pos")


def clip_of(fx, name=""):
    return mo.OptClip(fx["root_pos"], fx["root_rot"], fx["joint_rot"], fx["contacts"], fx["hf"], fx["min_point"], float(fx["dx"]),
                      int(fx["fps"]), name)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


_labellers = {}


def labeller(eps=ml.CONTACT_EPS):
    if float(eps) not in _labellers:
        _labellers[float(eps)] = ml.ContactLabeller(CHAR, DEV, float(eps))
    return _labellers[float(eps)]


def run_of(fx, clip, **kw):
    ground = dict(ground_height=float(fx["ground_height"])) if int(fx["mode"]) == 1 else {}
    return labeller(float(fx["contact_eps"])).run([clip], **ground, **kw)


@pytest.fixture(scope="module")
def cases():
    """name -> (fixture, clip, what the clip gives when it is the whole batch), computed once and left unchanged."""
    out = {}
    for name in mr.LABEL_FIXTURES:
        fx = mr.load(name)
        clip = clip_of(fx, name)
        out[name] = (fx, clip, run_of(fx, clip))
    return out


# cases 1, 3, 4, 5, 6, 7, 8: the bundled clips, the wave edges, off the grid, the side wall, deep penetration, eps variants, the plane
@pytest.mark.parametrize("name", mr.LABEL_FIXTURES)
def test_kernels_equal_the_reference_on_settled_decisions(cases, name):
    fx, clip, r = cases[name]
    h = labeller(float(fx["contact_eps"]))
    tol, sf, sh, ground = mr.tolerance(fx), fx["settled_feet"], fx["settled_hands"], int(fx["mode"]) == 1
    T, z = clip.num_frames, fx["root_pos"][:, 2]
    assert (~sf).mean() <= mr.MAX_UNSETTLED and (~sh).mean() <= mr.MAX_UNSETTLED
    assert r["contacts"].shape == (T, h.B) and r["gap"].shape == (T, 2) and r["lift"].shape == (T,) and r["hand_sd"].shape == (T, 2)
    feet, hands = r["contacts"][:, h.foot_ids], r["contacts"][:, h.hand_ids]
    ok = sf.all(-1)
    print(name, "T", T, "tol", tol, "gap err", np.abs(r["gap"] - fx["ref_gap"])[sf].max(initial=0.0),
          "root z err", np.abs(r["root_pos"][:, 2] - fx["ref_root_z"])[ok].max(initial=0.0),
          "hand_sd err", 0.0 if ground else np.abs(r["hand_sd"] - fx["ref_hand_sd"]).max(),
          "flag differences on unsettled", int((feet != fx["ref_contacts"][:, h.foot_ids])[~sf].sum()))
    assert set(np.unique(r["contacts"])) <= {0.0, 1.0}
    assert np.array_equal(feet[sf], fx["ref_contacts"][:, h.foot_ids][sf])
    assert np.abs(r["gap"] - fx["ref_gap"])[sf].max(initial=0.0) <= tol
    assert np.abs(r["root_pos"][:, 2] - fx["ref_root_z"])[ok].max(initial=0.0) <= tol
    assert np.abs(r["lift"] - (fx["ref_root_z"] - z))[ok].max(initial=0.0) <= tol and (r["lift"] >= 0).all()
    assert np.array_equal(bits(r["root_pos"][:, :2]), bits(fx["root_pos"][:, :2]))
    assert np.array_equal(bits(r["root_pos"][:, 2]), bits(z + r["lift"]))
    if ground:
        assert not hands.any() and np.isinf(r["hand_sd"]).all()
    else:
        assert np.array_equal(hands[sh], fx["ref_contacts"][:, h.hand_ids][sh])
        assert np.abs(r["hand_sd"] - fx["ref_hand_sd"]).max() <= tol
        assert np.array_equal(hands > 0.5, r["hand_sd"] < np.float32(fx["contact_eps"]))
    others = [b for b in range(h.B) if b not in h.foot_ids + h.hand_ids]
    assert not r["contacts"][:, others].any()


def test_kernels_equal_the_restatement(cases):
    cm = labeller().char_model
    for name in ("bundled_dec2024_teaser_717_1_opt_dm", "side_wall", "off_grid"):
        fx, clip, r = cases[name]
        eps, tol = float(fx["contact_eps"]), mr.tolerance(fx)
        feet, hands = mr.label_feet(cm, fx, eps), mr.label_hands(cm, fx, eps)
        assert np.abs(r["gap"] - feet["gap"])[feet["settled"]].max() <= tol and np.abs(r["hand_sd"] - hands["sd"]).max() <= tol
    fx, clip, r = cases["side_wall"]                     # the nearest face is a wall, not a top: a search under the hand alone misses it
    touch = (r["hand_sd"] < np.float32(fx["contact_eps"])).any(-1) & fx["wall_frames"]
    assert touch.sum() >= 3
    fx, clip, r = cases["bundled_dec2024_teaser_717_1_opt_dm"]
    assert r["contacts"][:, labeller().hand_ids].sum(0).tolist() == [20, 20]


# case 2: batch independence
def test_a_clip_gives_the_same_bits_alone_and_in_any_batch(cases):
    names = ["bundled_" + n for n in mr.BUNDLED] + ["edge_t1", "edge_t65", "edge_t129", "off_grid"]
    h = labeller()
    for order in (names, names[::-1]):
        r = h.run([cases[n][1] for n in order])
        off = r["packed"]["frame_off"]
        for i, n in enumerate(order):
            for k in OUTPUTS:
                assert np.array_equal(bits(r[k][off[i]:off[i + 1]]), bits(cases[n][2][k])), (n, k)
    clips = [cases[n][1] for n in names]
    again = h.run(clips, ground_height=0.0)               # and on the plane
    off = again["packed"]["frame_off"]
    for i, c in enumerate(clips):
        one = h.run([c], ground_height=0.0)
        for k in OUTPUTS:
            assert np.array_equal(bits(again[k][off[i]:off[i + 1]]), bits(one[k])), (c.name, k)


# case 6: deep penetration
def test_the_lifted_clip_no_longer_penetrates(cases):
    fx, clip, r = cases["deep_pen"]
    assert (r["lift"] > 0).mean() > 0.85 and r["lift"].max() > 0.2
    again = labeller().run([replace(clip, root_pos=r["root_pos"])])
    tol = mr.tolerance(fx)
    print("gap after the lift", again["gap"].min(), "lift after the lift", again["lift"].max())
    assert again["gap"].min() >= -tol and again["lift"].max() <= tol


# case 7: contact_eps
def test_contact_eps_changes_the_labels(cases):
    base = cases["bundled_TEASER_TERRAIN"][2]["contacts"]
    lo, hi = cases["eps_000"][2]["contacts"], cases["eps_100"][2]["contacts"]
    assert not np.array_equal(lo, base) and not np.array_equal(hi, base)
    assert (lo <= base).all() and (base <= hi).all()
    for k in ("gap", "lift", "hand_sd"):                 # the values do not depend on it
        assert np.array_equal(bits(cases["eps_000"][2][k]), bits(cases["bundled_TEASER_TERRAIN"][2][k]))


def test_options(cases):
    fx, clip, r = cases["bundled_dec2024_teaser_717_1_opt_dm"]
    h = labeller()
    marked = replace(clip, contacts=np.full_like(clip.contacts, 0.25))
    kept = h.run([marked], keep_existing=True)
    others = [b for b in range(h.B) if b not in h.foot_ids + h.hand_ids]
    assert (kept["contacts"][:, others] == 0.25).all()
    assert np.array_equal(kept["contacts"][:, h.foot_ids + h.hand_ids], r["contacts"][:, h.foot_ids + h.hand_ids])
    no_hands = h.run([marked], hands=False, keep_existing=True)
    assert (no_hands["contacts"][:, h.hand_ids] == 0.25).all() and np.isinf(no_hands["hand_sd"]).all()
    assert np.array_equal(no_hands["contacts"][:, h.foot_ids], r["contacts"][:, h.foot_ids])
    assert not h.run([marked], hands=False)["contacts"][:, h.hand_ids + others].any()
    no_lift = h.run([clip], correct_pen=False)
    assert np.array_equal(bits(no_lift["root_pos"]), bits(clip.root_pos))
    for k in ("contacts", "gap", "lift", "hand_sd"):
        assert np.array_equal(bits(no_lift[k]), bits(r[k]))
    new = h.label([clip, cases["bundled_sfu"][1]])
    assert [c.num_frames for c in new] == [clip.num_frames, 15] and new[0].name == clip.name and new[0].hf is clip.hf
    assert np.array_equal(bits(new[0].contacts), bits(r["contacts"])) and np.array_equal(bits(new[0].root_pos), bits(r["root_pos"]))
    assert np.array_equal(bits(new[1].contacts), bits(cases["bundled_sfu"][2]["contacts"]))
    assert h.kernel_times()["feet"] > 0 and h.kernel_times()["hands"] > 0


def test_clips_without_a_terrain_use_the_plane(cases):
    fx, clip, r = cases["ground_sfu"]
    h = labeller()
    bare = replace(clip, hf=None, min_point=None)
    got = h.run([bare])
    for k in OUTPUTS:
        assert np.array_equal(bits(got[k]), bits(r[k])), k
    with pytest.raises(ValueError, match="has no terrain"):
        h.run([bare, cases["bundled_sfu"][1]])
    raised = h.run([clip], ground_height=0.125)           # another height: the same as the clip lowered by it
    moved = h.run([replace(clip, root_pos=clip.root_pos - np.float32([0, 0, 0.125]))], ground_height=0.0)
    tol = mr.tolerance(fx)
    assert np.abs(raised["gap"] - moved["gap"]).max() <= tol and np.abs(raised["lift"] - moved["lift"]).max() <= tol
    settled = np.abs(moved["gap"] - np.float32(fx["contact_eps"])) >= mr.MARGIN_M
    assert np.array_equal(raised["contacts"][:, h.foot_ids][settled], moved["contacts"][:, h.foot_ids][settled])


def test_calls_out_of_order_and_bad_batches_are_refused():
    h = ml.ContactLabeller(CHAR, DEV)
    with pytest.raises(ParcError, match="mlabel: parc_mlabel_set_clips first"):
        h._call("run", 1, 1, 0, 0.0, 0)
    fx = mr.load("edge_t1")
    with pytest.raises(ParcError, match="mlabel: parc_mlabel_run first"):
        h._upload([clip_of(fx)])
        h._call("get_lift", None)
    with pytest.raises(ParcError, match="ground_height must be finite"):
        h.run([clip_of(fx)], ground_height=float("nan"))
    with pytest.raises(ValueError, match="has one frame"):
        h.resample([clip_of(fx, "single")], 30)


# case 9: resampling
@pytest.fixture(scope="module")
def resampled():
    out = {}
    for name in mr.RESAMPLE_FIXTURES:
        fx = mr.load(name)
        clip = clip_of(fx, name)
        out[name] = (fx, clip, labeller().resample([clip], float(fx["target_fps"]))[0])
    return out


@pytest.mark.parametrize("name", mr.RESAMPLE_FIXTURES)
def test_resampling_equals_calc_motion_frame(resampled, name):
    fx, clip, new = resampled[name]
    tol, tol_rot = mr.tolerance(fx), mr.tolerance(fx, "ref_err_rot")
    assert new.num_frames == fx["times"].size and new.fps == float(fx["target_fps"]) and new.hf is clip.hf
    err = dict(root_pos=np.abs(new.root_pos - fx["ref_root_pos"]).max(), contacts=np.abs(new.contacts - fx["ref_contacts"]).max(),
               root_rot=mr.quat_angle(new.root_rot, fx["ref_root_rot"]).max(), joint_rot=mr.quat_angle(new.joint_rot, fx["ref_joint_rot"]).max())
    print(name, clip.num_frames, "->", new.num_frames, "tol", tol, tol_rot, err)
    assert new.joint_rot.shape == (new.num_frames, labeller().B - 1, 4) and new.contacts.shape == (new.num_frames, labeller().B)
    assert err["root_pos"] <= tol and err["contacts"] <= tol
    assert err["root_rot"] <= tol_rot and err["joint_rot"] <= tol_rot


def test_resampling_in_a_batch_and_before_labelling(resampled):
    names = list(mr.RESAMPLE_FIXTURES)[:2] + ["resample_t2"]
    h = labeller()
    both = h.resample([replace(resampled[n][1], fps=30) for n in names], 45.0)
    alone = [h.resample([replace(resampled[n][1], fps=30)], 45.0)[0] for n in names]
    for a, b in zip(both, alone):
        for k in ("root_pos", "root_rot", "joint_rot", "contacts"):
            assert np.array_equal(bits(getattr(a, k)), bits(getattr(b, k))), k
    assert np.array_equal(bits(both[1].root_pos), bits(resampled["resample_45"][2].root_pos))
    labelled = h.label(both)                              # the resampled clips are clips like any other
    assert [c.num_frames for c in labelled] == [c.num_frames for c in both] and h.kernel_times()["resample"] > 0
