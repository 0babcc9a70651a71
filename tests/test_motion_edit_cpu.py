"""Hesitation-frame removal on the CPU: the float64 restatement (tests/hesitation_ref.py) against the reference fixtures
(tests/golden/make_golden_hesitation.py), and the host side of parc_amd/motion_edit.py and the driver's option.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import hesitation_ref as hr
from conftest import REPO, golden
from parc_amd import lib as L
from parc_amd.char_model import CharModel

CHAR = os.path.join(REPO, "data/assets/humanoid.xml")


@pytest.fixture(scope="module")
def char_model():
    return CharModel(CHAR)


@pytest.fixture(scope="module")
def restated(char_model):
    out = {}
    for name in hr.FIXTURES:
        z = golden("hesitation_" + name)
        bp = hr.body_positions(char_model, z["root_pos"], z["root_rot"], z["joint_rot"])
        out[name] = (z, bp, hr.remove_hesitation(bp, float(z["hesitation_val"]), int(z["hesitation_min_seq_len"])))
    return out


@pytest.mark.parametrize("name", hr.FIXTURES)
def test_restatement_keeps_the_reference_frames(restated, name):
    z, _, r = restated[name]
    print(name, "T", z["root_pos"].shape[0], "margin", r["margin"], "kept", r["kept"].size)
    assert r["margin"] >= hr.MARGIN_M                        # the condition under which kept frames must agree exactly
    assert r["margin"] == pytest.approx(float(z["margin"]), rel=1e-9) or np.isinf(r["margin"])
    assert np.array_equal(r["kept"], z["kept"])
    assert r["kept"][0] == 0 and not r["flags"][0]           # frame 0 is never flagged
    assert np.array_equal(r["flags"], hr.run_filter(r["flags_raw"], int(z["hesitation_min_seq_len"])))


def test_greedy_order_differs_from_the_any_earlier_rule(restated):
    want = {"greedy_s030": list(range(24)), "greedy_s012": list(range(24)), "greedy_s009": [0, 5, 10, 15, 20, 21, 22, 23]}
    for name, kept in want.items():
        z, bp, r = restated[name]
        assert z["kept"].tolist() == kept == r["kept"].tolist()
        step = np.linalg.norm((bp[1] - bp[0]).reshape(-1))   # a pure translation by s: d = s k sqrt(15)
        assert step == pytest.approx(float(name[-3:]) / 1000 * np.sqrt(15), rel=1e-5)
    # s = 0.012: every frame has an earlier one within 0.15 m, but the flagged ones are no anchors: runs of 3, kept.  The wrong rule
    # flags frames 1 .. 23 as one run and removes it
    assert hr.any_earlier_rule(restated["greedy_s012"][1]).tolist() == [0]
    assert hr.any_earlier_rule(restated["greedy_s009"][1]).tolist() == [0]
    assert restated["greedy_s012"][2]["flags_raw"].tolist() == [k % 4 != 0 for k in range(24)]


def test_fixture_kept_counts(restated):
    z = restated["civilization_holds"][0]
    T = z["root_pos"].shape[0]
    assert T == 254 + 4 + 6 + 2 + 5 and z["kept"].size == T - 4 - 6 - 5
    src = z["source_index"]
    assert np.array_equal(src[z["kept"]], np.sort(np.concatenate([np.arange(254), [119, 119]])))   # the hold of 2 stays
    assert restated["word_61_67"][0]["kept"].tolist() == [j for j in range(140) if not 61 <= j <= 67]
    assert restated["word_126_128"][0]["kept"].tolist() == list(range(140))
    assert restated["word_126_129"][0]["kept"].tolist() == [j for j in range(140) if not 126 <= j <= 129]
    for n in (63, 64, 65, 129):
        assert restated[f"tail_{n}"][0]["kept"].tolist() == list(range(n - 5))
    assert restated["repeat_70"][0]["kept"].tolist() == [0] and restated["edge_t1"][0]["kept"].tolist() == [0]
    assert restated["min_len_over_t"][0]["kept"].tolist() == list(range(24))
    for n in (1, 2):                                         # real motion at 0.3 m loses frames, more with the shorter minimum
        assert restated[f"civilization_v030_m{n}"][0]["kept"].size < 254
    assert restated["civilization_v030_m1"][0]["kept"].size < restated["civilization_v030_m2"][0]["kept"].size


def test_bundled_clips_lose_no_frame_at_the_defaults(char_model):
    from parc_amd import ms_file
    for name, want in (("civilization", 3.7e-3), ("dec2024_teaser_717_1_modified_opt", 3.4e-4), ("TEASER_TERRAIN", 6.4e-2), ("sfu", 0.24)):
        m = ms_file.load_ms_file(os.path.join(REPO, "data/motion_terrains", name + ".pkl"), load_misc=False).motion_data
        r = hr.remove_hesitation(hr.body_positions(char_model, m.root_pos, m.root_rot, m.joint_rot))
        print(name, "margin", r["margin"])
        assert r["kept"].size == np.asarray(m.root_pos).shape[0] and r["margin"] == pytest.approx(want, rel=0.05)


def test_unpack_bits_and_limits():
    from parc_amd import motion_edit as me
    w = np.zeros((2, 3), np.uint64)
    w[0, 0] = np.uint64(1) | (np.uint64(1) << np.uint64(63))
    w[1, 2] = np.uint64(1) << np.uint64(1)
    b = me.unpack_bits(w, 130)
    assert b.shape == (2, 130) and np.nonzero(b[0])[0].tolist() == [0, 63] and np.nonzero(b[1])[0].tolist() == [129]
    assert me.MAX_FRAMES == 4096 == 64 * me.FLAG_WORDS
    hdr = open(os.path.join(REPO, "include", "parc_env.h")).read()
    assert "#define PARC_MEDIT_MAX_FRAMES 4096" in hdr and "#define PARC_MEDIT_FLAG_WORDS 64" in hdr


def test_create_validates_before_it_touches_the_device(char_model):
    lib = L.load()
    p = L.ParcMotionEditParams()
    p.device, p.model, p.hesitation_val, p.hesitation_min_seq_len = 0, L.make_char_model(char_model), 0.15, 4
    h = C.c_void_p()
    p.struct_size = C.sizeof(p) - 4
    assert lib.parc_medit_create(C.byref(p), C.byref(h)) == -1 and b"ParcMotionEditParams ABI mismatch" in lib.parc_last_error()
    p.struct_size = C.sizeof(p)
    p.hesitation_min_seq_len = 0
    assert lib.parc_medit_create(C.byref(p), C.byref(h)) == -1 and b"hesitation_min_seq_len" in lib.parc_last_error()
    p.hesitation_min_seq_len, p.hesitation_val = 4, float("nan")
    assert lib.parc_medit_create(C.byref(p), C.byref(h)) == -1 and b"hesitation_val" in lib.parc_last_error()
    assert not h.value


def test_driver_option_is_off_by_default(tmp_path):
    import importlib.util
    spec = importlib.util.spec_from_file_location("run_optimize_motions", os.path.join(REPO, "scripts", "run_optimize_motions.py"))
    rom = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rom)
    cfg = rom.load_config(os.path.join(REPO, "data/configs/motion_opt/motion_opt_default.yaml"))
    assert cfg["remove_hesitation"] is False and "hesitation_val" not in cfg and "hesitation_min_seq_len" not in cfg
