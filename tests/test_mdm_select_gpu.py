"""Rollout selection on the GPU (``parc_amd/motion_select.py``) against the reference's record
(``tests/golden/mdm_select.npz``, ``make_golden_mdm_select.py``), against ``PathMotionGenerator.select`` and against the analyser on
the materialised slices.  Losses are compared within ``1e-5 |want| + 1e-6`` (the tolerance of ``test_selection`` and
``test_scores_and_point_sdfs_match_reference``); geometry, order and flags exactly."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mdm_ref as R
import mdm_select_ref as SR
from parc_amd import lib as L
from parc_amd import motion_generator as mg
from parc_amd import motion_path_gen as mpg
from parc_amd import motion_select as msel
from parc_amd import terrain as T
from parc_amd.motion_terrain import MotionTerrainAnalyzer

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
DEV = "cuda:0"
CHAR = os.path.join(REPO, "data/assets/humanoid.xml")


def tol(want):
    return 1e-5 * np.abs(want) + 1e-6


@pytest.fixture(scope="module")
def fx():
    return SR.Fixture(GOLDEN)


@pytest.fixture(scope="module")
def gen():
    m = R.Fixture(GOLDEN)
    return mg.MDMGenerator.from_state_dict(m.cfg, m.sd, m.mean, m.std, DEV, max_batch=8)


@pytest.fixture(scope="module")
def pg(gen, fx):
    h = mpg.PathMotionGenerator(gen, mpg.MDMPathSettings(max_motion_length=0.6, w_contact=fx.w_contact, w_pen=fx.w_pen), mpg.MDMGenSettings())
    assert h.max_frames >= fx.F
    return h


@pytest.fixture(scope="module")
def selector(pg, fx):
    return msel.PathSelector(pg, points=(fx.points, fx.point_body), slice_padding=fx.padding)


def scene(pg, fx, paths=None, k=None):
    paths = range(fx.P) if paths is None else paths
    pg.set_scene(fx.hfs[list(paths)], fx.min_points[list(paths)], fx.dx, [fx.paths()[p] for p in paths], fx.K if k is None else k)


def result(pg, fx, rows=None, frames=None, final=None):
    """The fixture's frames (or ``frames``) of ``rows`` as the ``RolloutResult`` a rollout leaves: views of one packed device buffer."""
    rows = list(range(fx.N)) if rows is None else list(rows)
    src = fx.frames if frames is None else frames
    buf = pg.pack_frames({k: torch.from_numpy(np.ascontiguousarray(v[rows])) for k, v in src.items()})
    fr = pg.unpack_frames(buf)
    ff = torch.from_numpy(np.ascontiguousarray((fx.final_frame if final is None else final)[rows])).to(DEV)
    F = buf.shape[1]
    return mpg.RolloutResult(fr["root_pos"], fr["root_rot"], fr["joint_rot"], fr["contacts"], ff, ff >= 0, F, 1, [F])


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


@pytest.fixture(scope="module")
def runs(pg, selector, fx):
    """The selection of the whole fixture per mode, with the recorded noise and thresholds: computed once, left unchanged."""
    scene(pg, fx)
    res = result(pg, fx)
    out = {}
    for mode in ("s", "w"):
        sel = selector.select(res, top_k=fx.K, noise=fx.noise, slice_terrain=mode == "s", **fx.thresholds)
        out[mode] = (sel, {k: np.copy(v) for k, v in selector.last_run.items()})
    return out


@pytest.mark.parametrize("mode", ["s", "w"])
def test_against_the_reference_record(fx, runs, selector, pg, mode):
    sel, r = runs[mode]
    assert not r["status"].any() and np.array_equal(r["num_frames"], [SR.row_length(f, fx.F) for f in fx.final_frame])
    assert np.array_equal(bits(r["slice_min_point"]), bits(fx.rec(mode, "min_point"))) and np.array_equal(r["slice_dims"], fx.rec(mode, "dims"))
    for k, key in (("contact_loss", "contact"), ("pen_loss", "pen"), ("total_loss", "total")):
        want = fx.rec(mode, key)
        err = np.abs(r[k].astype(np.float64) - want)
        print(mode, k, "max err / tol %.3f" % (err / tol(want)).max())
        assert (err <= tol(want)).all(), (mode, k, r[k], want)
    assert np.array_equal(r["order"], fx.rec(mode, "order"))
    assert np.array_equal(r["valid"] != 0, fx.rec(mode, "valid"))
    valid = fx.rec(mode, "valid")
    for p, s in enumerate(sel):
        order = fx.rec(mode, "order")[p * fx.K:(p + 1) * fx.K]
        assert np.array_equal(s["order"], order) and s["path"] == p
        assert np.array_equal(s["rows"], order[valid[order]]) and s["num_valid"] == valid[order].sum() and s["enough"] == (s["num_valid"] >= fx.K)
        assert np.array_equal(s["total_loss"], r["total_loss"][s["rows"]])
        if mode == "s":
            assert len(s["terrains"]) == len(s["rows"])
            for row, (hf, mp) in zip(s["rows"], s["terrains"]):
                assert np.array_equal(bits(hf), bits(fx.sliced_hf(row))) and np.array_equal(bits(mp), bits(fx.rec("s", "min_point")[row])), row
        else:
            assert "terrains" not in s
    if mode == "s":                                                # every row's slice, not the kept ones' only
        scene(pg, fx)
        selector.run(result(pg, fx), fx.noise, True)
        for row, hf in enumerate(selector.gather(np.arange(fx.N), r["slice_dims"], r["status"])):
            assert np.array_equal(bits(hf), bits(fx.sliced_hf(row))), row


def test_against_todays_select(fx, pg, selector, runs):
    """``slice_terrain=False`` gives the rows of ``PathMotionGenerator.select`` on the same result, losses within the tolerance."""
    scene(pg, fx)
    res = result(pg, fx)
    an = MotionTerrainAnalyzer(CHAR, DEV, points=(fx.points, fx.point_body))
    for k in (fx.K, 2):
        old = pg.select(res, top_k=k, noise=fx.noise, analyzer=an)
        new = selector.select(res, top_k=k, noise=fx.noise, slice_terrain=False)
        for o, n in zip(old, new):
            assert np.array_equal(o["rows"], n["rows"]) and n["enough"] and n["num_valid"] == fx.K
            for key in ("total_loss", "contact_loss", "pen_loss"):
                assert (np.abs(n[key].astype(np.float64) - o[key]) <= tol(o[key])).all(), (key, n[key], o[key])
    seeded_old, seeded_new = pg.select(res, top_k=2, seed=7, analyzer=an), selector.select(res, top_k=2, seed=7, slice_terrain=False)
    assert all(np.array_equal(o["rows"], n["rows"]) for o, n in zip(seeded_old, seeded_new))


def test_against_the_analyzer_on_the_materialised_slices(fx, pg, selector, runs):
    """The index-table view against the slice as a heightfield of its own: ``to_clips(terrains=...)`` through ``MotionTerrainAnalyzer``."""
    scene(pg, fx)
    res = result(pg, fx)
    sel = selector.select(res, top_k=fx.K, noise=fx.noise, slice_terrain=True)
    an = MotionTerrainAnalyzer(CHAR, DEV, points=(fx.points, fx.point_body))
    differ = 0
    for s in sel:
        assert len(s["rows"]) == fx.K
        clips = pg.to_clips(res, s["rows"], terrains=s["terrains"])
        for c, (hf, mp) in zip(clips, s["terrains"]):
            assert np.array_equal(c.hf, hf) and np.array_equal(c.min_point, mp)
        out = an.run(clips)["clip_out"]
        pen, con = np.float32(fx.w_pen) * out[:, 0], np.float32(fx.w_contact) * out[:, 1]
        assert (np.abs(s["pen_loss"].astype(np.float64) - pen) <= tol(pen)).all(), (s["pen_loss"], pen)
        assert (np.abs(s["contact_loss"].astype(np.float64) - con) <= tol(con)).all(), (s["contact_loss"], con)
        differ += int((bits(s["pen_loss"]) != bits(pen)).sum() + (bits(s["contact_loss"]) != bits(con)).sum())
    print("losses not bit-equal to the analyser's on the materialised slice: %d of %d" % (differ, 2 * fx.N))
    whole = pg.to_clips(res, [0])                                  # the default is unchanged: the whole terrain
    assert np.array_equal(whole[0].hf, fx.hfs[0]) and np.array_equal(whole[0].min_point, fx.min_points[0])
    with pytest.raises(ValueError, match="terrains"):
        pg.to_clips(res, [0, 1], terrains=sel[0]["terrains"][:1])


def test_brute_and_pruned_give_the_same_bits(fx, pg, runs):
    brute = msel.PathSelector(pg, sdf_mode=msel.SDF_BRUTE, points=(fx.points, fx.point_body), slice_padding=fx.padding)
    scene(pg, fx)
    res = result(pg, fx)
    for mode in ("s", "w"):
        b = brute.run(res, fx.noise, mode == "s", **fx.thresholds)
        for k, v in runs[mode][1].items():
            assert np.array_equal(np.asarray(b[k]).view(np.int32), np.asarray(v).view(np.int32)), (mode, k)


def test_batch_independence(fx, pg, selector, runs):
    """Each row alone (P = 1, K = 1) has the bits it has in the batch; permuting the rows of a path permutes ``order``."""
    for mode in ("s", "w"):
        full = runs[mode][1]
        for row in range(fx.N):
            scene(pg, fx, [fx.row_path[row]], 1)
            one = selector.run(result(pg, fx, [row]), fx.noise[row:row + 1], mode == "s", **fx.thresholds)
            for k in msel.ROW_KEYS:
                assert np.array_equal(np.asarray(one[k]).view(np.int32)[0], np.asarray(full[k]).view(np.int32)[row]), (mode, row, k)
            assert one["order"].tolist() == [0] and one["num_valid"][0] == full["valid"][row]
        perm = np.array([1, 0, 3, 2, 6, 7, 4, 5])                  # within each path; rows 0 and 2 (the tie) keep their order
        scene(pg, fx)
        p = selector.run(result(pg, fx, perm), fx.noise[perm], mode == "s", **fx.thresholds)
        assert np.array_equal(bits(p["total_loss"]), bits(full["total_loss"][perm]))
        assert np.array_equal(perm[p["order"]], full["order"]) and np.array_equal(p["num_valid"], full["num_valid"])


def test_edge_cases(fx, pg, selector, runs):
    full = runs["s"][1]
    frames = {k: v.copy() for k, v in fx.frames.items()}
    frames["root_pos"][1, 3, 0] = np.nan                           # inside row 1's 12 frames
    frames["root_pos"][6, :, 0] = np.linspace(2.0, 2.0 + 0.4 * 1100, fx.F)   # row 6 spans 1 100 cells along x
    scene(pg, fx)
    res = result(pg, fx, frames=frames)
    for sliced in (True, False):
        sel = selector.select(res, top_k=fx.K, noise=fx.noise, slice_terrain=sliced, **fx.thresholds)
        r = selector.last_run
        ref = runs["s" if sliced else "w"][1]
        assert r["status"][1] == msel.STATUS_NONFINITE and r["status"][6] == (msel.STATUS_TOO_LARGE if sliced else 0)
        bad = [1, 6] if sliced else [1]
        for row in bad:
            assert np.isnan([r["total_loss"][row], r["contact_loss"][row], r["pen_loss"][row]]).all() and r["valid"][row] == 0
            p = row // fx.K
            assert sel[p]["order"][-1] == row and row not in sel[p]["rows"]          # ranked last, never kept
        keep = [i for i in range(fx.N) if i not in (1, 6)]
        for k in msel.ROW_KEYS:                                    # the other rows' bits are unchanged
            assert np.array_equal(np.asarray(r[k]).view(np.int32)[keep], np.asarray(ref[k]).view(np.int32)[keep]), (sliced, k)
        if sliced:
            hfs = selector.gather([0, 6, 2], r["slice_dims"], r["status"])
            assert hfs[1].size == 0 and np.array_equal(hfs[0], fx.sliced_hf(0)) and np.array_equal(hfs[2], fx.sliced_hf(2))
    both = {k: v.copy() for k, v in fx.frames.items()}
    both["root_pos"][0, 0, 1] = np.inf
    both["root_pos"][2, 5, 2] = np.nan                             # two NaN rows of one path rank last in row order
    sel = selector.select(result(pg, fx, frames=both), top_k=fx.K, slice_terrain=True)
    assert sel[0]["order"].tolist()[-2:] == [0, 2] and sel[0]["num_valid"] == 2 and not sel[0]["enough"]
    empty = fx.final_frame.copy()
    empty[3] = 0
    sel = selector.select(result(pg, fx, final=empty), top_k=1, slice_terrain=True)
    assert selector.last_run["status"][3] == msel.STATUS_EMPTY and sel[0]["order"][-1] == 3 and sel[0]["enough"]
    # thresholds all off keep everything; top_k above num_valid is not enough
    res = result(pg, fx)
    off = selector.select(res, top_k=fx.K, noise=fx.noise, slice_terrain=True)
    assert all(s["num_valid"] == fx.K and s["enough"] and np.array_equal(s["rows"], s["order"]) for s in off)
    assert np.array_equal(bits(selector.last_run["total_loss"]), bits(full["total_loss"]))
    cut = selector.select(res, top_k=fx.K, noise=fx.noise, slice_terrain=True, **fx.thresholds)
    nv = fx.rec("s", "valid").reshape(fx.P, fx.K).sum(1)
    assert [s["num_valid"] for s in cut] == nv.tolist() and [s["enough"] for s in cut] == (nv >= fx.K).tolist() and not all(s["enough"] for s in cut)
    assert all(len(s["rows"]) == s["num_valid"] for s in cut)
    top1 = selector.select(res, top_k=1, noise=fx.noise, slice_terrain=True, **fx.thresholds)
    assert all(s["enough"] and len(s["rows"]) == 1 and len(s["terrains"]) == 1 for s in top1)


def test_refusals_name_their_argument(fx, gen, pg, selector):
    scene(pg, fx)
    res = result(pg, fx)
    with pytest.raises(ValueError, match="top_k"):
        selector.select(res, top_k=0)
    with pytest.raises(ValueError, match="noise"):
        selector.select(res, noise=np.zeros(fx.N + 1, np.float32))
    with pytest.raises(ValueError, match="rows"):
        selector.select(result(pg, fx, [0, 1]))
    long = {k: np.concatenate([v, v], axis=1)[:, :pg.max_frames + 1] for k, v in fx.frames.items()}
    assert long["root_pos"].shape[1] == pg.max_frames + 1
    with pytest.raises(L.ParcError, match="num_frames"):
        selector.select(result(pg, fx, frames=long))
    a = L.ParcPathSelectArgs()
    buf = pg.pack_frames({k: torch.from_numpy(v) for k, v in fx.frames.items()})
    a.frames, a.final_frame, a.num_frames, a.frame_stride = buf.data_ptr(), res.final_frame.data_ptr(), fx.F + 1, fx.F
    with pytest.raises(L.ParcError, match="frame_stride"):
        selector._call("run", a, selector._stream())
    a.num_frames, a.max_pen_loss = fx.F, float("nan")
    with pytest.raises(L.ParcError, match="threshold"):
        selector._call("run", a, selector._stream())
    many = (np.zeros((L.MOPT_MAX_POINTS + 1, 3), np.float32), np.zeros(L.MOPT_MAX_POINTS + 1, np.int32))
    with pytest.raises(L.ParcError, match="num_points"):
        msel.PathSelector(pg, points=many)
    with pytest.raises(L.ParcError, match="sdf_mode"):
        msel.PathSelector(pg, sdf_mode=7, points=(fx.points, fx.point_body))
    with pytest.raises(TypeError, match="PathMotionGenerator"):
        msel.PathSelector(gen)
    fresh = mpg.PathMotionGenerator(gen, mpg.MDMPathSettings(max_motion_length=0.6), mpg.MDMGenSettings())
    s2 = msel.PathSelector(fresh, points=(fx.points, fx.point_body))
    with pytest.raises(ValueError, match="set_scene"):
        s2.select(res)
    a.max_pen_loss = float("inf")
    with pytest.raises(L.ParcError, match="no scene"):
        s2._call("run", a, s2._stream())
    with pytest.raises(L.ParcError, match="parc_msel_run first"):
        s2.gather([0], np.ones((1, 2), np.int32), np.zeros(1, np.int32))
    s2._destroy()
    fresh._destroy()


def test_launch_count_and_times(fx, pg, selector, runs):
    scene(pg, fx)
    selector.select(result(pg, fx), top_k=1, slice_terrain=True)
    d = selector.describe()
    assert d["launches"] == L.MSEL_RUN_LAUNCHES == 4 and d["rows"] == fx.N and d["max_slice_dim"] == L.MSEL_MAX_SLICE_DIM and d["points"] == len(fx.points)
    assert d["max_rows"] == 8 and d["max_frames"] == pg.max_frames
    ms = selector.kernel_times()
    assert list(ms) == list(msel.KERNELS) and all(v > 0 for v in ms.values())


def test_lifecycle(fx, gen):
    """Create / destroy twice; the selector goes before its ``PathMotionGenerator``."""
    for _ in range(2):
        h = mpg.PathMotionGenerator(gen, mpg.MDMPathSettings(max_motion_length=0.6, w_contact=fx.w_contact, w_pen=fx.w_pen), mpg.MDMGenSettings())
        s = msel.PathSelector(h, points=(fx.points, fx.point_body))
        scene(h, fx)
        sel = s.select(result(h, fx), top_k=1, noise=fx.noise)
        assert [x["rows"][0] for x in sel] == [fx.rec("s", "order")[0], fx.rec("s", "order")[fx.K]]
        s._destroy()
        assert s._h is None and s.pg is None
        s._destroy()
        h._destroy()
    torch.cuda.synchronize()


def test_script_smoke(tmp_path):
    """``generate_path_motions.py --random_init 0 --slice_terrain --max_pen_loss``: the saved terrain is the slice around the saved
    motion, and ``short_paths`` is reported."""
    from parc_amd import ms_file
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    (tmp_path / "paths").mkdir()
    hf = (np.kron(np.arange(16).reshape(4, 4) % 3, np.ones((4, 4))) * 0.2).astype(np.float32)
    mp = np.array([1.5, -2.0], np.float32)
    pts = np.stack([0.8 + 0.5 * np.arange(8), np.full(8, 2.0), np.zeros(8)], axis=-1).astype(np.float32)
    np.savez_compressed(tmp_path / "paths" / "paths_0000.npz", hf=hf[None], min_point_offset=mp[None], dx=np.float32(0.4), points=pts,
                        point_off=np.array([0, len(pts)], np.int64))
    out = tmp_path / "motions"
    run = subprocess.run([sys.executable, os.path.join(REPO, "scripts", "generate_path_motions.py"), "--paths", str(tmp_path / "paths"), "--out", str(out),
                          "--random_init", "0", "--candidates", "3", "--top_k", "2", "--max_motion_length", "1.0", "--max_batch", "4", "--seed", "3",
                          "--slice_terrain", "--max_pen_loss", "1e30", "--max_attempts", "2"], env=env, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    line = json.loads(run.stdout.strip().splitlines()[-1])
    assert line["paths"] == 1 and line["short_paths"] in (0, 1) and line["rows"] in (3, 6)
    files = sorted(os.listdir(out))
    assert len(files) == 2 * (1 - line["short_paths"]) and line["short_paths"] == 0
    t = T.SubTerrain(16, 16, 0.4, 0.4, mp[0], mp[1])
    t.hf = hf
    for f in files:
        d = ms_file.load_ms_file(str(out / f))
        want = T.slice_terrain_around_motion(np.asarray(d.motion_data.root_pos, np.float32), t, padding=1.2, localize=False)
        got = d.terrain_data
        assert np.array_equal(np.asarray(got.hf, np.float32), want.hf) and np.array_equal(np.asarray(got.min_point, np.float32), want.min_point)
        assert tuple(got.hf.shape) == tuple(want.dims) and np.isfinite(d.misc_data["total_loss"])
