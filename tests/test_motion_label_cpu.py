"""Contact labelling on the CPU: the float64 restatement (tests/motion_label_ref.py) against the reference fixtures
(tests/golden/make_golden_motion_label.py), and the host side of parc_amd/motion_label.py, parc_mlabel_create and the script.  No GPU."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import motion_label_ref as mr
from conftest import REPO
from parc_amd import lib as L
from parc_amd import motion_label as ml
from parc_amd.char_model import CharModel

CHAR = os.path.join(REPO, "data/assets/humanoid.xml")
FEET, HANDS = ml.FOOT_BODIES, ml.HAND_BODIES


@pytest.fixture(scope="module")
def char_model():
    return CharModel(CHAR)


def columns(cm, names):
    return [cm.get_body_id(n) for n in names]


@pytest.mark.parametrize("name", mr.LABEL_FIXTURES)
def test_restatement_reproduces_the_reference(char_model, name):
    fx = mr.load(name)
    eps, tol, ground = float(fx["contact_eps"]), mr.tolerance(fx), int(fx["mode"]) == 1
    feet = mr.label_ground(char_model, fx, eps, float(fx["ground_height"])) if ground else mr.label_feet(char_model, fx, eps)
    sf, sh = fx["settled_feet"], fx["settled_hands"]
    print(name, "T", sf.shape[0], "unsettled feet", int((~sf).sum()), "hands", int((~sh).sum()), "tol", tol,
          "gap err", np.abs(feet["gap"] - fx["ref_gap"])[sf].max(initial=0.0))
    assert np.array_equal(feet["settled"], sf)
    assert (~sf).mean() <= mr.MAX_UNSETTLED and (~sh).mean() <= mr.MAX_UNSETTLED
    ref_feet = fx["ref_contacts"][:, columns(char_model, FEET)] > 0.5
    assert np.array_equal(feet["contact"][sf], ref_feet[sf])
    assert np.abs(feet["gap"] - fx["ref_gap"])[sf].max(initial=0.0) <= tol
    ok = sf.all(-1)
    assert np.abs(fx["root_pos"][:, 2].astype(np.float64) + feet["lift"] - fx["ref_root_z"])[ok].max(initial=0.0) <= tol
    ref_hands = fx["ref_contacts"][:, columns(char_model, HANDS)] > 0.5
    if ground:
        assert not ref_hands.any()
    else:
        hands = mr.label_hands(char_model, fx, eps)
        assert np.array_equal(hands["settled"], sh) and np.array_equal(hands["contact"][sh], ref_hands[sh])
        assert np.abs(hands["sd"] - fx["ref_hand_sd"]).max() <= tol
    others = [b for b in range(char_model.get_num_bodies()) if b not in columns(char_model, FEET + HANDS)]
    assert not fx["ref_contacts"][:, others].any()


def test_the_fixtures_hold_what_their_cases_are_for(char_model):
    lh_rh = columns(char_model, HANDS)
    dec = mr.load("bundled_dec2024_teaser_717_1_opt_dm")
    assert dec["hf"].shape == (18, 15) and dec["ref_contacts"][:, lh_rh].sum(0).tolist() == [20, 20]
    lifted = {n: int((mr.load("bundled_" + n)["ref_root_z"] != mr.load("bundled_" + n)["root_pos"][:, 2]).sum()) for n in mr.BUNDLED}
    assert lifted == {"sfu": 9, "civilization": 88, "TEASER_TERRAIN": 13, "dec2024_teaser_717_1_opt_dm": 70}
    assert [mr.load(n)["root_pos"].shape[0] for n in ("edge_t1", "edge_t65", "edge_t129")] == [1, 65, 129]
    base = mr.load("bundled_TEASER_TERRAIN")["ref_contacts"]
    assert all(not np.array_equal(mr.load(n)["ref_contacts"], base) for n in ("eps_000", "eps_100"))
    sw = mr.load("side_wall")      # the nearest face is a wall: the hand touches while the cell under it lies more than 0.5 m below
    assert ((sw["ref_hand_sd"] < sw["contact_eps"]).any(-1) & sw["wall_frames"]).sum() >= 3
    og = mr.load("off_grid")
    pos, _ = mr.fk(char_model, og["root_pos"], og["root_rot"], og["joint_rot"])
    u = (pos[:, lh_rh + columns(char_model, FEET), :2] - og["min_point"]) / float(og["dx"])
    assert (np.rint(u[..., 0]) > 17).any() and (np.rint(u[..., 1]) < 0).any()


@pytest.mark.parametrize("name", mr.RESAMPLE_FIXTURES)
def test_resampling_restatement_and_the_loop_times(name):
    fx = mr.load(name)
    T = fx["root_pos"].shape[0]
    times = ml.resample_times(T, int(fx["fps"]), float(fx["target_fps"]))
    assert times.dtype == np.float32 and np.array_equal(times, fx["times"])          # the frame count of the reference's loop
    assert np.float32(ml.motion_length(T, int(fx["fps"]))) == fx["length"]
    r = mr.resample(fx, times, float(fx["length"]))
    tol, tol_rot = mr.tolerance(fx), mr.tolerance(fx, "ref_err_rot")
    print(name, T, "->", times.size, "tol", tol, tol_rot)
    assert np.abs(r["root_pos"] - fx["ref_root_pos"]).max() <= tol and np.abs(r["contacts"] - fx["ref_contacts"]).max() <= tol
    assert mr.quat_angle(r["root_rot"], fx["ref_root_rot"]).max() <= tol_rot
    assert mr.quat_angle(r["joint_rot"], fx["ref_joint_rot"]).max() <= tol_rot


def test_resample_frame_counts():
    assert [mr.load(n)["times"].size for n in mr.RESAMPLE_FIXTURES] == [169, 380, 507, 254, 5]
    assert ml.resample_times(1, 30, 30).size == 0                                     # length 0: the reference's loop yields nothing


@pytest.mark.parametrize("name", mr.BUNDLED)
def test_flat_terrain_matches_the_reference(name):
    fx = mr.load("bundled_" + name)
    for (dx, padding), dims, mn in zip(fx["flat_params"], fx["flat_dims"], fx["flat_min_point"]):
        hf, min_point, d = ml.flat_terrain_for(fx["root_pos"], float(dx), float(padding))
        assert hf.dtype == np.float32 and not hf.any() and list(hf.shape) == dims.tolist() and d == float(dx)
        assert min_point.dtype == np.float32 and np.array_equal(min_point, mn)


def test_wrapper_refusals(char_model):
    p = ml.labeller_params(char_model)
    assert p.num_foot_boxes == 2 and list(p.box_foot)[:2] == [0, 1] and list(p.foot_body) == columns(char_model, FEET)
    assert list(p.hand_body) == columns(char_model, HANDS) and list(p.hand_radius) == pytest.approx([0.04, 0.04])
    assert list(p.box_half[0]) == pytest.approx([0.0885, 0.045, 0.0275]) and list(p.box_offset[1]) == pytest.approx([0.045, 0.0, -0.0225])
    with pytest.raises(ValueError, match="unknown body 'left_toe'"):
        ml.labeller_params(char_model, foot_bodies=("left_toe", "right_foot"))
    with pytest.raises(ValueError, match="foot body 'left_hand': its first geom must be a box"):
        ml.labeller_params(char_model, foot_bodies=("left_hand", "right_foot"))
    with pytest.raises(ValueError, match="hand body 'right_foot': its first geom must be a sphere"):
        ml.labeller_params(char_model, hand_bodies=("left_hand", "right_foot"))
    for bad in (0, -30):
        with pytest.raises(ValueError, match="target_fps must be > 0"):
            ml.resample_times(10, 30, bad)
        with pytest.raises(ValueError, match="target_fps must be > 0"):
            ml.ContactLabeller.resample(object.__new__(ml.ContactLabeller), [], bad)


def refused(params, message):
    lib = L.load()
    out = C.c_void_p()
    rc = lib.parc_mlabel_create(None if params is None else C.byref(params), C.byref(out))
    assert rc == -1 and lib.parc_last_error().decode() == message and not out.value, lib.parc_last_error().decode()


def test_create_refuses_before_it_touches_a_device(char_model):
    hdr = open(os.path.join(REPO, "include", "parc_env.h")).read()
    for sym in [s for s in L.EXPORTED_SYMBOLS if s.startswith("parc_mlabel_")]:
        assert f" {sym}(" in hdr
    assert len([s for s in L.EXPORTED_SYMBOLS if s.startswith("parc_mlabel_")]) == 10 and L.ABI_VERSION == 6
    refused(None, "mlabel: null argument")
    lib = L.load()
    assert lib.parc_mlabel_create(C.byref(ml.labeller_params(char_model)), None) == -1
    assert lib.parc_last_error().decode() == "mlabel: null argument"
    p = ml.labeller_params(char_model)
    p.struct_size += 1
    refused(p, "ParcMotionLabelParams ABI mismatch (struct_size)")
    for nb in (0, L.MAX_BODIES + 1):
        p = ml.labeller_params(char_model)
        p.model.num_bodies = nb
        refused(p, "mlabel: num_bodies out of range")
    for dof in (-1, L.MAX_DOFS + 1):
        p = ml.labeller_params(char_model)
        p.model.dof_size = dof
        refused(p, "mlabel: dof_size out of range")
    p = ml.labeller_params(char_model)
    p.foot_body[1] = char_model.get_num_bodies()
    refused(p, "mlabel: foot_body out of range")
    p = ml.labeller_params(char_model)
    p.hand_radius[0] = 0.0
    refused(p, "mlabel: hand_radius must be > 0")
    p = ml.labeller_params(char_model)
    p.box_foot[1] = 0
    refused(p, "mlabel: every foot needs a box")
    buf = (C.c_float * 3)(7.0, 7.0, 7.0)
    assert lib.parc_mlabel_kernel_times(None, buf) == -1 and lib.parc_last_error().decode() == "mlabel: null argument"
    assert lib.parc_mlabel_run(None, 1, 1, 0, 0.0, 0) == -1 and lib.parc_last_error().decode() == "mlabel: null handle"


def test_script_help_runs():
    out = subprocess.run([sys.executable, os.path.join(REPO, "scripts", "label_motions.py"), "--help"], capture_output=True, text=True)
    assert out.returncode == 0
    for flag in ("--inputs", "--out", "--target_fps", "--ground_height", "--no_hands", "--no_lift", "--keep_existing", "--flat_terrain_dx",
                 "--flat_terrain_padding"):
        assert flag in out.stdout
