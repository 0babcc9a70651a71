"""Hesitation-frame removal on the GPU (parc_medit_*) against the reference fixtures (tests/golden/make_golden_hesitation.py) and the
float64 restatement (tests/hesitation_ref.py).

Every fixture's margin (the smallest |d(i, j) - hesitation_val| over its pairs) is at least 1e-4 m, twenty times what an fp32 forward
kinematics can move a norm of 45 numbers of a few metres: the kernel's pair mask, flags and kept frames must equal the yardsticks
EXACTLY, and the kept rows are copies of the input rows, bit for bit."""
import os

import numpy as np
import pytest

import hesitation_ref as hr
from conftest import REPO, golden
from parc_amd import motion_edit as me
from parc_amd import motion_opt as mo
from parc_amd.lib import ParcError

pytestmark = pytest.mark.gpu

CHAR = os.path.join(REPO, "data/assets/humanoid.xml")
DEV = "cuda:0"
FLAT = dict(hf=np.zeros((3, 2), np.float32), min_point=np.zeros(2, np.float32), dx=0.5)   # the tool validates a terrain and ignores it


def clip_of(z, name=""):
    return mo.OptClip(z["root_pos"], z["root_rot"], z["joint_rot"], z["contacts"], FLAT["hf"], FLAT["min_point"], FLAT["dx"], 30, name)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def rows_equal(clip, src, kept):
    return all(np.array_equal(bits(getattr(clip, k)), bits(getattr(src, k)[kept])) for k in ("root_pos", "root_rot", "joint_rot", "contacts"))


@pytest.fixture(scope="module")
def cases():
    """name -> (fixture, clip, restatement), computed once and left unchanged."""
    cm = me.CharModel(CHAR)
    out = {}
    for name in hr.FIXTURES:
        z = golden("hesitation_" + name)
        r = hr.remove_hesitation(hr.body_positions(cm, z["root_pos"], z["root_rot"], z["joint_rot"]), float(z["hesitation_val"]),
                                 int(z["hesitation_min_seq_len"]))
        assert r["margin"] >= hr.MARGIN_M and np.array_equal(r["kept"], z["kept"])
        out[name] = (z, clip_of(z, name), r)
    return out


_removers = {}


def remover(val=me.HESITATION_VAL, min_len=me.HESITATION_MIN_SEQ_LEN):
    key = (float(val), int(min_len))
    if key not in _removers:
        _removers[key] = me.HesitationRemover(CHAR, DEV, *key)
    return _removers[key]


def remover_of(z):
    return remover(float(z["hesitation_val"]), int(z["hesitation_min_seq_len"]))


@pytest.fixture(scope="module")
def alone(cases):
    """name -> what the clip gives when it is the whole batch: (new clip, kept, pair mask, raw flags, flags)."""
    out = {}
    for name, (z, clip, _) in cases.items():
        h = remover_of(z)
        new, kept = h.remove([clip])
        raw, fil = h.flags()
        out[name] = (new[0], kept[0], h.pair_mask(0), raw[0], fil[0])
    return out


# cases 1-5: the greedy order, holds in a real clip, parameters on real motion, word boundaries, edges
@pytest.mark.parametrize("name", hr.FIXTURES)
def test_kernel_equals_reference_and_restatement(cases, alone, name):
    z, clip, r = cases[name]
    new, kept, mask, raw, fil = alone[name]
    print(name, "T", clip.num_frames, "margin", r["margin"], "kept", kept.size, "pairs", int(r["pair_mask"].sum()))
    assert np.array_equal(mask, r["pair_mask"])
    assert np.array_equal(raw, r["flags_raw"]) and np.array_equal(fil, r["flags"])
    assert kept.dtype == np.int64 and np.array_equal(kept, z["kept"])
    assert new.num_frames == kept.size and rows_equal(new, clip, kept)
    assert new.hf is clip.hf and new.fps == clip.fps and new.name == name and new.dx == clip.dx


def test_greedy_order_not_any_earlier_frame(cases, alone):
    assert alone["greedy_s030"][1].tolist() == list(range(24)) == alone["greedy_s012"][1].tolist()
    assert alone["greedy_s009"][1].tolist() == [0, 5, 10, 15, 20, 21, 22, 23]
    z, clip, _ = cases["greedy_s012"]
    bp = hr.body_positions(me.CharModel(CHAR), z["root_pos"], z["root_rot"], z["joint_rot"])
    assert hr.any_earlier_rule(bp).tolist() == [0]           # what "flag j if any earlier frame is near" would keep


def test_constraints_and_bounds_pass_through(cases):
    z, clip, _ = cases["civilization_holds"]
    c = mo.OptClip(**{**clip.__dict__})
    c.cons_body, c.cons_start, c.cons_end = np.array([3, 5], np.int32), np.array([0, 100], np.int32), np.array([10, 270], np.int32)
    c.cons_point = np.arange(6, dtype=np.float32).reshape(2, 3)
    c.hf_maxmin = np.ones(c.hf.shape + (2,), np.float32)
    new = remover().remove([c])[0][0]
    assert new.num_frames == z["kept"].size < c.num_frames
    for k in ("cons_body", "cons_start", "cons_end", "cons_point", "hf_maxmin"):
        assert np.array_equal(getattr(new, k), getattr(c, k)), k


# case 6: a clip's result depends neither on the batch nor on its place in it.  One handle has one pair of parameters, so the clips of
# cases 1-5 go in one batch per pair: fourteen at the defaults, the others with their own
def test_batch_independence(cases, alone):
    groups = {}
    for name, (z, _, _) in cases.items():
        groups.setdefault((float(z["hesitation_val"]), int(z["hesitation_min_seq_len"])), []).append(name)
    assert len(groups[(me.HESITATION_VAL, me.HESITATION_MIN_SEQ_LEN)]) == 14
    for key, names in groups.items():
        h = remover(*key)
        for order in (names, names[::-1][1:] + names[::-1][:1]):
            new, kept = h.remove([cases[n][1] for n in order])
            raw, fil = h.flags()
            for i, n in enumerate(order):
                a_new, a_kept, a_mask, a_raw, a_fil = alone[n]
                assert np.array_equal(kept[i], a_kept) and rows_equal(new[i], a_new, np.arange(a_new.num_frames)), (key, n)
                assert np.array_equal(h.pair_mask(i), a_mask) and np.array_equal(raw[i], a_raw) and np.array_equal(fil[i], a_fil), (key, n)


def _translated(z, steps, s=0.05):
    n = len(steps)
    rp = np.repeat(z["root_pos"][:1], n, 0)
    rp[:, 0] += (np.asarray(steps, np.float64) * s).astype(np.float32)
    return mo.OptClip(rp, np.repeat(z["root_rot"][:1], n, 0), np.repeat(z["joint_rot"][:1], n, 0), np.repeat(z["contacts"][:1], n, 0),
                      FLAT["hf"], FLAT["min_point"], FLAT["dx"])


# case 7: the limit.  4096 frames are taken (distinct poses 0.05 m apart, d = 0.19 k, but for two holds: one across words 31 | 32, one
# that ends on the last frame of the last word); 4097 are refused by name, and the handle goes on working
def test_limit_and_refusal(cases, alone):
    z = cases["greedy_s030"][0]
    steps = np.arange(me.MAX_FRAMES)
    steps[2045:2051] = 2044
    steps[4090:] = 4089
    h = remover()
    new, kept = h.remove([cases["tail_65"][1], _translated(z, steps)])
    want = np.array([j for j in range(me.MAX_FRAMES) if not (2045 <= j <= 2050 or j >= 4090)], np.int64)
    assert np.array_equal(kept[1], want) and np.array_equal(kept[0], alone["tail_65"][1])
    raw, fil = h.flags()
    assert np.array_equal(np.nonzero(fil[1])[0], np.setdiff1d(np.arange(me.MAX_FRAMES), want)) and np.array_equal(raw[1], fil[1])
    long_clip = _translated(z, np.arange(me.MAX_FRAMES + 1))
    with pytest.raises(ParcError, match=r"medit: clip 1 has 4097 frames; at most 4096"):
        h.remove([cases["tail_65"][1], long_clip])
    new, kept = h.remove([cases["greedy_s009"][1]])          # usable afterwards
    assert kept[0].tolist() == [0, 5, 10, 15, 20, 21, 22, 23] and rows_equal(new[0], cases["greedy_s009"][1], kept[0])


# case 8: the driver.  Off by default; on, the shortened clip is what hf_extras and save_flipped see
def test_driver_removes_before_extras_and_flip(cases, tmp_path):
    import sys
    sys.path.insert(0, os.path.join(REPO, "scripts"))
    import run_optimize_motions as drv
    from parc_amd import ms_file
    z = cases["civilization_holds"][0]
    src = ms_file.load_ms_file(os.path.join(REPO, "data/motion_terrains/civilization.pkl"), load_misc=False)
    md = ms_file.MSMotionData(root_pos=z["root_pos"], root_rot=z["root_rot"], joint_rot=z["joint_rot"], body_contacts=z["contacts"],
                              fps=int(src.motion_data.fps), loop_mode="CLAMP")
    clip_path = str(tmp_path / "holds.pkl")
    ms_file.save_ms_file(ms_file.MSFileData(motion_data=md, terrain_data=src.terrain_data, misc_data=None), clip_path)
    cfg = drv.load_config(os.path.join(REPO, "data/configs/motion_opt/motion_opt_default.yaml"))
    cfg.update(motions_yaml_path=clip_path, num_iters=0, device=DEV, auto_compute_body_constraints=False, frame_stride=1,
               hf_extras=True, save_flipped=True)
    T, n = z["root_pos"].shape[0], z["kept"].size
    assert n < T
    for on, want in ((True, n), (None, T)):
        c = dict(cfg, output_folder_path=str(tmp_path / ("on" if on else "off")))
        if on:
            c["remove_hesitation"] = True
        else:
            c.pop("remove_hesitation")                       # the key absent: every existing run writes what it wrote
        opt_path, flip_path = drv.run(c)
        d = ms_file.load_ms_file(opt_path)
        m = d.motion_data
        assert m.root_pos.shape[0] == m.root_rot.shape[0] == m.joint_rot.shape[0] == m.body_contacts.shape[0] == want
        assert len(d.misc_data["hf_mask_inds"]) == want
        assert ms_file.load_ms_file(flip_path, load_misc=False).motion_data.root_pos.shape[0] == want
        if on:
            assert np.array_equal(bits(m.body_contacts), bits(z["contacts"][z["kept"]]))
