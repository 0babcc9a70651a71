"""The rollout selection without a GPU: the numpy mirror ``mdm_select_ref`` against the reference's record
(``tests/golden/mdm_select.npz``, ``make_golden_mdm_select.py``), ``terrain.slice_terrain_around_motion(localize=False)`` against the
recorded slices, and the new flags of ``scripts/generate_path_motions.py`` on fake handles."""
import os
import sys
import types

import numpy as np
import pytest
import torch

import mdm_select_ref as SR
from conftest import REPO
from parc_amd import terrain as T
from parc_amd.char_model import CharModel


def tol(want):
    """The tolerance of ``test_selection`` and ``test_scores_and_point_sdfs_match_reference``."""
    return 1e-5 * np.abs(want) + 1e-6


@pytest.fixture(scope="module")
def fx():
    return SR.Fixture()


@pytest.fixture(scope="module")
def mirror(fx):
    """The mirror's selection per mode, computed once."""
    cm = CharModel(os.path.join(REPO, "data/assets/humanoid.xml"))
    return {mode: SR.select(cm, fx.frames, fx.final_frame, fx.hfs, fx.min_points, fx.dx, fx.row_path, fx.points, fx.point_body, fx.w_contact, fx.w_pen, fx.penalty,
                            fx.padding, mode == "s", fx.noise, **fx.thresholds) for mode in ("s", "w")}


def test_the_fixture_holds_the_rows_it_is_meant_to(fx):
    d, mp = fx.rec("s", "dims"), fx.rec("s", "min_point")
    X, Y = fx.hfs.shape[1:]
    hi = mp + (d - 1) * np.float32(fx.dx)
    t_hi = fx.min_points[fx.row_path] + (np.array([X, Y]) - 1) * np.float32(fx.dx)
    inside = (mp >= fx.min_points[fx.row_path] - 1e-3).all(1) & (hi <= t_hi + 1e-3).all(1)
    assert inside[0] and not inside[1] and not inside[3]
    assert (hi[1] > t_hi[1]).all() and (mp[3] < fx.min_points[0]).all()              # over +x / +y; from outside -x / -y
    assert (d[4] > [X, Y]).all()                                                      # a slice larger than its terrain
    assert fx.final_frame[5] == -1 and fx.final_frame[6] == fx.F and fx.final_frame[7] == 1
    assert all(np.array_equal(v[0], v[2]) for v in fx.frames.values()) and fx.noise[0] == fx.noise[2]   # the tie
    assert (fx.rec("w", "dims") == [X, Y]).all()
    for mode in ("s", "w"):
        o = fx.rec(mode, "order")[:fx.K].tolist()
        assert o.index(2) == o.index(0) + 1                                           # the tie, in row order
        assert 0 < fx.rec(mode, "valid").sum() < fx.N
    assert not np.array_equal(fx.rec("s", "valid"), fx.rec("w", "valid"))             # the slice changes who passes


@pytest.mark.parametrize("mode", ["s", "w"])
def test_mirror_reproduces_the_record(fx, mirror, mode):
    m = mirror[mode]
    assert not m["status"].any()
    assert np.array_equal(m["n"], [SR.row_length(f, fx.F) for f in fx.final_frame])
    assert np.array_equal(m["min_point"], fx.rec(mode, "min_point")) and np.array_equal(m["dims"], fx.rec(mode, "dims"))   # bit for bit
    if mode == "s":
        for r in range(fx.N):
            assert np.array_equal(m["hf"][r], fx.sliced_hf(r)), r
    for k in ("contact", "pen", "total"):
        want = fx.rec(mode, k)
        err = np.abs(m[k].astype(np.float64) - want)
        print(mode, k, "max err / tol %.3f" % (err / tol(want)).max())
        assert (err <= tol(want)).all(), (mode, k, m[k], want)
    assert np.array_equal(m["order"], fx.rec(mode, "order"))
    assert np.array_equal(m["valid"], fx.rec(mode, "valid"))
    assert np.array_equal(m["num_valid"], fx.rec(mode, "valid").reshape(fx.P, fx.K).sum(1))


def test_mirror_edge_rows(fx):
    """NaN last in row order, never valid; a slice over the cap; an empty row."""
    cm = CharModel(os.path.join(REPO, "data/assets/humanoid.xml"))
    fr = {k: v[:4].copy() for k, v in fx.frames.items()}
    fr["root_pos"][1, 3, 0] = np.nan
    fr["root_pos"][3, :, 0] = np.linspace(0, 0.4 * 2400, fx.F)       # its 12 frames span 1 100 cells along x
    ff = np.array([12, 12, 0, 12], np.int32)
    m = SR.select(cm, fr, ff, fx.hfs, fx.min_points, fx.dx, np.zeros(4, np.int64), fx.points, fx.point_body, fx.w_contact, fx.w_pen, fx.penalty, fx.padding, True)
    assert m["status"].tolist() == [0, SR.STATUS_NONFINITE, SR.STATUS_EMPTY, SR.STATUS_TOO_LARGE]
    assert m["order"].tolist() == [0, 1, 2, 3] and m["valid"].tolist() == [True, False, False, False] and m["num_valid"].tolist() == [1]
    assert np.isnan(m["total"][1:]).all()


def test_slice_terrain_localize_false_is_the_recorded_slice(fx):
    for r in range(fx.N):
        p = fx.row_path[r]
        t = T.SubTerrain(fx.hfs.shape[1], fx.hfs.shape[2], fx.dx, fx.dx, fx.min_points[p][0], fx.min_points[p][1])
        t.hf = fx.hfs[p].copy()
        t.hf_maxmin[..., 0] = fx.hfs[p] + 1
        n = SR.row_length(fx.final_frame[r], fx.F)
        s = T.slice_terrain_around_motion(fx.frames["root_pos"][r, :n], t, padding=fx.padding, localize=False)
        assert isinstance(s, T.SubTerrain)
        assert np.array_equal(s.hf, fx.sliced_hf(r)) and np.array_equal(s.min_point, fx.rec("s", "min_point")[r]) and np.array_equal(s.dims, fx.rec("s", "dims")[r])
        assert np.array_equal(s.hf_maxmin[..., 0], s.hf + 1) and s.dxdy.tolist() == t.dxdy.tolist()
        loc, xyz = T.slice_terrain_around_motion(fx.frames["root_pos"][r, :n], t, padding=fx.padding)   # the default is unchanged
        assert loc.hf.shape == s.hf.shape and xyz[0, 0] == 0 and xyz[0, 1] == 0


# ---- the script ----------------------------------------------------------------------------------------------------------------------
class FakeHandle:
    """``PathMotionGenerator`` as the script sees it."""

    def __init__(self):
        self.scenes, self.seeds, self.ids, self.calls = [], [], [], []

    def set_scene(self, hfs, mps, dx, paths, k):
        self.scenes.append((hfs.shape[0], k))
        self.P, self.K = hfs.shape[0], k

    def rollout(self, seed=None, row_ids=None, path_ids=None):
        self.seeds.append(seed)
        self.ids.append(np.asarray(row_ids))
        return types.SimpleNamespace(final_frame=torch.full((self.P * self.K,), 9, dtype=torch.int32), windows=2, path_ids=np.asarray(path_ids))

    def select(self, res, top_k=None, seed=None):
        self.calls.append("select")
        return [dict(path=p, rows=np.arange(p * self.K, p * self.K + top_k), total_loss=np.arange(top_k, dtype=np.float32), contact_loss=np.zeros(top_k, np.float32),
                     pen_loss=np.zeros(top_k, np.float32)) for p in range(self.P)]

    def to_clips(self, res, rows, terrains=None):
        from parc_amd.motion_opt import OptClip
        self.calls.append("clips" if terrains is None else "clips+terrains")
        z = np.zeros
        hfs = [(z((16, 16), np.float32), z(2, np.float32))] * len(rows) if terrains is None else terrains
        return [OptClip(z((9, 3), np.float32), z((9, 4), np.float32), z((9, 14, 4), np.float32), z((9, 15), np.float32), hf, mp, 0.4) for hf, mp in hfs]


class FakeSelector:
    """``PathSelector`` as the script sees it: path id 1 has too few valid rows until its third rollout, path id 2 never has enough."""

    def __init__(self, handle):
        self.h, self.kw, self.tries = handle, [], {}

    def select(self, res, top_k=None, seed=None, slice_terrain=True, max_contact_loss=None, max_pen_loss=None, max_total_loss=None):
        self.kw.append(dict(seed=seed, slice_terrain=slice_terrain, thresholds=(max_contact_loss, max_pen_loss, max_total_loss)))
        out = []
        for p, pid in enumerate(res.path_ids):
            t = self.tries[int(pid)] = self.tries.get(int(pid), 0) + 1
            enough = not (pid == 2 or (pid == 1 and t < 3))
            rows = np.arange(p * self.h.K, p * self.h.K + (top_k if enough else 1))
            d = dict(path=p, rows=rows, total_loss=np.arange(len(rows), dtype=np.float32), contact_loss=np.zeros(len(rows), np.float32), pen_loss=np.zeros(len(rows), np.float32),
                     order=np.arange(p * self.h.K, (p + 1) * self.h.K), num_valid=len(rows), enough=enough)
            if slice_terrain:
                d["terrains"] = [(np.full((5, 7), float(pid), np.float32), np.array([1.5, -2.5], np.float32)) for _ in rows]
            out.append(d)
        return out


@pytest.fixture()
def path_files(tmp_path):
    files = []
    for b in range(2):                                             # 5 terrains per batch, terrain 2 without a path
        pts = [np.arange(9, dtype=np.float32).reshape(3, 3) if q != 2 else np.zeros((0, 3), np.float32) for q in range(5)]
        f = tmp_path / f"paths_{b:04d}.npz"
        np.savez(f, hf=np.zeros((5, 16, 16), np.float32), min_point_offset=np.zeros((5, 2), np.float32), dx=np.float32(0.4), points=np.concatenate(pts),
                 point_off=np.concatenate([[0], np.cumsum([len(p) for p in pts])]))
        files.append(str(f))
    return files


def script():
    sys.path.insert(0, os.path.join(REPO, "scripts"))
    import generate_path_motions as S
    return S


def test_script_default_flags_write_the_same_files(tmp_path, path_files):
    """Without the new flags ``run`` goes through ``handle.select`` and ``to_clips`` without terrains: the files are byte for byte those of
    the loop as it was (restated here), and the JSON keys are the old ones."""
    S = script()
    h = FakeHandle()
    stats = S.run(h, path_files, str(tmp_path / "new"), 3, 2, 0, 8)
    assert stats == dict(paths=8, rows=24, finished=24, windows=8) and set(h.calls) == {"select", "clips"}
    old = FakeHandle()
    os.makedirs(tmp_path / "old")
    first = 0
    for b, f in enumerate(path_files):                             # the loop of the script before the selector
        for group in S.chunks(S.read_paths(f), 8 // 3):
            old.set_scene(np.stack([g[1] for g in group]), np.stack([g[2] for g in group]), group[0][3], [g[4] for g in group], 3)
            pids = first + np.arange(len(group), dtype=np.int64)
            first += len(group)
            ids = (pids[:, None] * 3 + np.arange(3)[None, :]).reshape(-1)
            res = old.rollout(seed=0, row_ids=ids, path_ids=pids)
            final = res.final_frame.cpu().numpy()
            for g, sel in zip(group, old.select(res, top_k=2, seed=0 + b)):
                for rank, (clip, row) in enumerate(zip(old.to_clips(res, sel["rows"]), sel["rows"])):
                    misc = dict(total_loss=float(sel["total_loss"][rank]), contact_loss=float(sel["contact_loss"][rank]), pen_loss=float(sel["pen_loss"][rank]),
                                final_frame=int(final[row]), num_frames=int(clip.num_frames), row_id=int(ids[row]), path=g[4])
                    S.save_clip(clip, os.path.join(tmp_path / "old", S.file_name(b, g[0], rank)), misc)
    names = sorted(os.listdir(tmp_path / "old"))
    assert names == sorted(os.listdir(tmp_path / "new")) and len(names) == 16
    for n in names:
        assert open(tmp_path / "old" / n, "rb").read() == open(tmp_path / "new" / n, "rb").read(), n
    assert [np.array_equal(a, b) for a, b in zip(h.ids, old.ids)] == [True] * 4 and h.seeds == old.seeds


def test_script_device_select_retries_and_counts_short_paths(tmp_path, path_files):
    S = script()
    from parc_amd import ms_file
    h = FakeHandle()
    s = FakeSelector(h)
    stats = S.run(h, path_files[:1], str(tmp_path / "out"), 3, 2, 5, 8, selector=s, slice_terrain=True, max_pen_loss=8.0, max_attempts=3)
    # group 0: path ids 0, 1 -> rollouts of (0, 1), (1), (1); group 1: ids 2, 3 -> (2, 3), (2), (2)
    assert h.scenes == [(2, 3), (1, 3), (1, 3)] * 2 and h.seeds == [5, 6, 7] * 2
    assert [i.tolist() for i in h.ids[:3]] == [[0, 1, 2, 3, 4, 5], [3, 4, 5], [3, 4, 5]]                 # the same ids at every attempt
    assert stats == dict(paths=4, rows=24, finished=24, windows=12, short_paths=1)
    assert all(k["slice_terrain"] and k["thresholds"] == (None, 8.0, None) for k in s.kw) and [k["seed"] for k in s.kw[:3]] == [5, 6, 7]
    assert "select" not in h.calls and set(h.calls) == {"clips+terrains"}
    names = sorted(os.listdir(tmp_path / "out"))
    assert names == sorted(S.file_name(0, q, r) for q in (0, 1, 4) for r in range(2))                      # terrain 3 (path id 2) fell short
    d = ms_file.load_ms_file(str(tmp_path / "out" / S.file_name(0, 1, 0)))
    assert d.terrain_data.hf.shape == (5, 7) and (np.asarray(d.terrain_data.hf) == 1.0).all() and np.asarray(d.terrain_data.min_point).tolist() == [1.5, -2.5]
    assert d.misc_data["row_id"] == 3
    # one attempt: both slow paths fall short; without slicing the clips keep the whole terrain
    h2 = FakeHandle()
    stats = S.run(h2, path_files[:1], str(tmp_path / "out2"), 3, 2, 5, 8, selector=FakeSelector(h2), max_total_loss=30.0)
    assert stats["short_paths"] == 2 and set(h2.calls) == {"clips"} and len(os.listdir(tmp_path / "out2")) == 4
    # the new flags without a selector are refused, before anything is generated
    h3 = FakeHandle()
    for kw in (dict(slice_terrain=True), dict(max_pen_loss=8.0), dict(max_attempts=2)):
        with pytest.raises(SystemExit, match="device_select"):
            S.run(h3, path_files, str(tmp_path / "out3"), 3, 2, 0, 8, **kw)
    with pytest.raises(SystemExit, match="max_attempts"):
        S.run(h3, path_files, str(tmp_path / "out3"), 3, 2, 0, 8, selector=FakeSelector(h3), max_attempts=0)
    assert not h3.scenes and not os.path.exists(tmp_path / "out3")
    with pytest.raises(TypeError):                                  # keyword-only: the positional signature is the old one
        S.run(h3, path_files, str(tmp_path / "out3"), 3, 2, 0, 8, None)
