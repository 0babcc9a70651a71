"""Path-following motion generation without a GPU: the torch restatement ``mdm_path_ref`` against the reference's
record (``tests/golden/mdm_path.npz``), the settings through their YAML, the refusals the host decides, and the script's chunking and
file naming on a fake handle."""
import dataclasses
import os
import sys
import types

import numpy as np
import pytest
import torch

import mdm_path_ref as PR
import mdm_ref as R
from parc_amd import motion_generator as mg
from parc_amd import motion_path_gen as mpg
from parc_amd.char_model import CharModel

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
# the restatement in float64 against the reference in float64 as stored (fixed point, steps of 2^-28 = 3.7e-9), on top of float64
# rounding through three generations: under three steps, the bound test_mdm_cpu.py holds mdm_ref to
TOL64 = 1e-8


@pytest.fixture(scope="module")
def fx():
    return PR.PathFixture(GOLDEN)


@pytest.fixture(scope="module")
def model():
    return R.Fixture(GOLDEN)


@pytest.fixture(scope="module")
def rollouts(fx, model):
    """The records replayed by the restatement in float64, free-running from their start with the recorded x_T."""
    ref64 = R.MdmRef(model.cfg, model.sd, model.mean, model.std, torch.float64)
    out = {}
    for rec in fx.RECORDS:
        pr = PR.PathRef(model.cfg, ref64.cm, model.mean, model.std, mpg.MDMPathSettings(max_motion_length=fx.max_motion_length),
                        mpg.MDMGenSettings(ddim_stride=fx.stride, use_cfg=fx.use_cfg(rec)), torch.float64)
        out[rec] = pr.rollout(fx.scene(rec, torch.float64), PR.mdm_ref_generate(ref64, pr, fx.x_T(rec), fx.stride), [fx.rel_height],
                              prev_frames=fx.start(rec, torch.float64), keep_windows=True)
    return pr, out


def near(name, got, fx, key):
    err = (got.double() - fx.f64(key).reshape(got.shape)).abs().max().item()
    print("%-34s %.3e" % (name, err))
    assert err <= TOL64, (name, err)


def test_ref_integer_outputs_are_exact(fx, rollouts):
    pr, out = rollouts
    for rec in fx.RECORDS:
        r = out[rec]
        assert r["windows"] == fx.windows(rec)
        assert r["frames_per_window"] == fx.raw(f"{rec}/frames_per_window").tolist()
        assert np.array_equal(r["final_frame"].numpy(), fx.raw(f"{rec}/final_frame")), rec
        for w, rw in enumerate(r["window_records"]):
            c = rw["conds"]
            assert np.array_equal(c["target_node"].numpy(), fx.raw(f"{rec}/w{w}/target_node")), (rec, w)
            cell = (c["OBS_KEY"] + c["canon_z"].unsqueeze(-1)).float().numpy()
            assert np.array_equal(cell, fx.raw(f"{rec}/w{w}/hf_cell")), (rec, w)
            if w > 0:
                assert np.array_equal(c["closest_node"].numpy(), fx.raw(f"{rec}/w{w}/closest_node")), (rec, w)
                assert np.array_equal(c["done"].numpy(), fx.raw(f"{rec}/w{w}/done")), (rec, w)
            flags = torch.stack([c[k] for k in ("OBS_FLAG_KEY", "TARGET_FLAG_KEY", "PREV_STATE_FLAG_KEY", "PREV_STATE_NOISE_IND_KEY")], dim=-1)
            assert np.array_equal(flags.numpy(), fx.raw(f"{rec}/w{w}/flags")), (rec, w)
            assert (c["GUIDANCE_PARAMS"] is not None) == bool(fx.raw(f"{rec}/w{w}/guided"))
    assert fx.windows("limit") == 3 and fx.raw("limit/final_frame").tolist() == [-1] * 6
    assert fx.windows("mixed") == 3 and fx.raw("mixed/final_frame").tolist() == [16, 16, 16, -1, -1, -1]
    assert fx.windows("alldone") == 2 and fx.raw("alldone/final_frame").tolist() == [-1] * 6 and fx.raw("alldone/w1/done").all()


def test_ref_nodes_record(fx, model):
    """The 80-node path: closest node (a tie, nodes past 64), the clamped lookahead, done on the last node, as the reference recorded them."""
    z = fx.z
    cm = CharModel(mg._char_path(model.cfg))
    pr = PR.PathRef(model.cfg, cm, model.mean, model.std, mpg.MDMPathSettings(), mpg.MDMGenSettings(), torch.float64)
    scene = PR.Scene(z["flat/hf"][None], z["flat/min_point"][None], fx.dx, [z["nodes/path"]], [0] * 6, torch.float64)
    prev = {k: torch.from_numpy(z[f"nodes/prev_{k}"]).double() for k in PR.FRAME_KEYS}
    c = pr.conds(scene, prev)
    assert c["closest_node"].tolist() == z["nodes/closest_node"].tolist() == [0, 30, 66, 75, 79, 44]
    assert c["target_node"].tolist() == z["nodes/target_node"].tolist() == [7, 37, 73, 79, 79, 51]
    assert c["done"].tolist() == z["nodes/done"].tolist()
    assert np.array_equal((c["OBS_KEY"] + c["canon_z"].unsqueeze(-1)).float().numpy(), z["nodes/hf_cell"])
    near("nodes target", c["TARGET_KEY"], fx, "nodes/target")
    for k in ("ROOT_POS", "ROOT_ROT", "JOINT_POS"):
        near("nodes prev " + k, c["PREV_STATE_KEY"][k], fx, f"nodes/ps_{k}")


def test_ref_tensors_against_the_record(fx, rollouts):
    pr, out = rollouts
    for rec in fx.RECORDS:
        r = out[rec]
        for w, rw in enumerate(r["window_records"]):
            c = rw["conds"]
            near(f"{rec} w{w} target", c["TARGET_KEY"], fx, f"{rec}/w{w}/target")
            for k in ("ROOT_POS", "ROOT_ROT", "JOINT_POS"):
                near(f"{rec} w{w} prev {k}", c["PREV_STATE_KEY"][k], fx, f"{rec}/w{w}/ps_{k}")
            for k in PR.FRAME_KEYS[:3]:
                near(f"{rec} w{w} in {k}", rw["prev"][k], fx, f"{rec}/w{w}/prev_{k}")
            for k in PR.FRAME_KEYS:
                near(f"{rec} w{w} out {k}", rw["frames"][k], fx, f"{rec}/w{w}/out_{k}")
        for k in PR.FRAME_KEYS:
            near(f"{rec} frames {k}", r["frames"][k], fx, f"{rec}/frames_{k}")


def test_ref_rough_scene(fx, model):
    """The wrapper alone on the rough scene in float64: heights exact, target and previous state within the fixed-point step, and the
    recorded boundary distances are the restatement's."""
    z = fx.z
    cm = CharModel(mg._char_path(model.cfg))
    pr = PR.PathRef(model.cfg, cm, model.mean, model.std, mpg.MDMPathSettings(), mpg.MDMGenSettings(), torch.float64)
    tg = z["rough/targets"]
    mps = np.concatenate([np.repeat(z["rough/min_point"][None], 5, 0), (z["rough/min_point"] + z["rough/far_offset"])[None]])
    scene = PR.Scene(np.stack([z["rough/hf"]] * 6), mps, float(z["rough/dx"]), [np.stack([t, t]) for t in tg], np.arange(6), torch.float64)
    prev = {k: torch.from_numpy(z[f"rough/prev_{k}"]).double() for k in PR.FRAME_KEYS}
    c = pr.conds(scene, prev, first=True)
    assert np.array_equal(c["OBS_KEY"].float().numpy(), z["rough/hf_z64"])
    near("rough target", c["TARGET_KEY"], fx, "rough/target")
    for k in ("ROOT_POS", "ROOT_ROT", "JOINT_POS"):
        near("rough prev " + k, c["PREV_STATE_KEY"][k], fx, f"rough/ps_{k}")
    assert np.abs(c["edge_dist"].float().numpy() - z["rough/boundary_dist"]).max() < 1e-6
    assert (c["TARGET_KEY"][1] == 0).all()                         # a zero target vector stays zero


def test_ref_done_exits():
    """The two exits of the loop on a two-node path under the start pose, with a generator that stands still: every row done at the
    second window (the all-done exit: ``final_frame`` stays -1 for all, as the reference leaves it), and one row carried away (the
    others get their ``final_frame``, the time limit ends it)."""
    cfg = mg.default_config()
    cm = CharModel(mg._char_path(cfg))
    D = mg.frame_dim(cm)
    pr = PR.PathRef(cfg, cm, np.zeros((15, D)), np.ones((15, D)), mpg.MDMPathSettings(max_motion_length=0.6), mpg.MDMGenSettings(), torch.float64)
    path = np.array([[0.1, 0.05, 0.0], [0.0, 0.0, 0.0]], np.float32)
    scene = PR.Scene(np.zeros((1, 8, 8), np.float32), np.array([[-1.4, -1.4]], np.float32), 0.4, [path], [0] * 3, torch.float64)

    def stand(away):
        def generate(c, w):
            n = c["TARGET_KEY"].shape[0]
            pos = torch.zeros((n, 15, 3), dtype=torch.float64)
            pos[away, :, 0] = 2.0 * (w + 1)
            q = torch.zeros((n, 15, 4), dtype=torch.float64)
            q[..., 3] = 1
            jq = torch.zeros((n, 15, 14, 4), dtype=torch.float64)
            jq[..., 3] = 1
            return {"ROOT_POS": pos, "ROOT_ROT": q, "JOINT_ROT": jq, "CONTACTS": torch.zeros((n, 15, 15), dtype=torch.float64)}
        return generate
    r = pr.rollout(scene, stand([]), [0.8])
    assert r["windows"] == 2 and r["frames_per_window"] == [9, 13] and r["final_frame"].tolist() == [-1, -1, -1] and r["done"].all()
    r = pr.rollout(scene, stand([1]), [0.8])
    assert r["windows"] == 3 and r["frames_per_window"] == [9, 7, 13] and r["final_frame"].tolist() == [16, -1, 16] and r["done"].tolist() == [True, False, True]


# ---- host logic ---------------------------------------------------------------------------------------------------------------------------
def test_settings_round_trip_through_the_yaml(tmp_path):
    import yaml
    ps, gs, rest = mpg.load_config(os.path.join(REPO, "data/configs/mdm_path/mdm_path_default.yaml"))
    assert ps == mpg.MDMPathSettings() and gs == mpg.MDMGenSettings() and rest == {}
    ps2 = dataclasses.replace(ps, top_k=3, max_motion_length=2.5)
    gs2 = dataclasses.replace(gs, use_cfg=False, ddim_stride=5)
    p = tmp_path / "c.yaml"
    p.write_text(yaml.safe_dump({"mdm_path": ps2.to_config(), "mdm_gen": gs2.to_config()}))
    a, b, _ = mpg.load_config(str(p))
    assert a == ps2 and b == gs2 and isinstance(a.top_k, int) and isinstance(b.use_cfg, bool)
    with pytest.raises(ValueError, match="lookahed"):
        mpg.MDMPathSettings.from_config({"lookahed": 3})
    with pytest.raises(ValueError, match="cfg_scal"):
        mpg.MDMGenSettings.from_config({"cfg_scal": 1.0})


class FakeGenerator(mg.MDMGenerator):
    """An MDMGenerator that never creates its handle: what the front end checks before it reaches the library."""

    def __init__(self, cfg):
        self.cfg, self.device = cfg, torch.device("cpu")

    def __del__(self):
        pass


def test_refusals_name_their_key():
    with pytest.raises(TypeError, match="MDMGenerator"):
        mpg.PathMotionGenerator(object())
    cfg = dict(mg.default_config(), relative_z_style="RELATIVE_TO_ROOT_FLOOR")
    with pytest.raises(ValueError, match="relative_z_style"):
        mpg.PathMotionGenerator(FakeGenerator(cfg))
    with pytest.raises(ValueError, match="use_ddim"):
        mpg.PathMotionGenerator(FakeGenerator(mg.default_config()), gen_settings=mpg.MDMGenSettings(use_ddim=False))


def bare_handle():
    h = mpg.PathMotionGenerator.__new__(mpg.PathMotionGenerator)
    h.device, h.N, h.P, h.nprev, h.FD, h.T, h.D, h._scene, h.J, h.B = torch.device("cpu"), 2, 1, 2, 78, 15, 91, None, 14, 15
    return h


def test_argument_refusals_before_the_library():
    h = bare_handle()
    with pytest.raises(ValueError, match="set_scene"):
        h.rollout(seed=0)
    with pytest.raises(ValueError, match="set_scene"):
        h.conds({})
    with pytest.raises(ValueError, match="hfs"):
        h.set_scene(np.zeros((4, 4)), np.zeros((1, 2)), 0.4, [np.zeros((2, 3))])
    with pytest.raises(ValueError, match="min_points"):
        h.set_scene(np.zeros((1, 4, 4)), np.zeros((2, 2)), 0.4, [np.zeros((2, 3))])
    with pytest.raises(ValueError, match="paths"):
        h.set_scene(np.zeros((1, 4, 4)), np.zeros((1, 2)), 0.4, [])
    with pytest.raises(ValueError, match="candidates_per_path"):
        h.set_scene(np.zeros((1, 4, 4)), np.zeros((1, 2)), 0.4, [np.zeros((2, 3))], 0)
    h._scene = {}
    with pytest.raises(ValueError, match="heading_mode"):
        h.rollout(seed=0, heading_mode="north")
    with pytest.raises(ValueError, match="seed"):
        h.rollout()
    with pytest.raises(ValueError, match="speed"):
        h.rollout(seed=0, plan={"rel_height": torch.zeros(1), "speed": torch.zeros(1)})
    with pytest.raises(ValueError, match="rel_height"):
        h.rollout(seed=0, plan={"rel_height": torch.zeros(3)})
    with pytest.raises(ValueError, match="noise"):
        h.rollout(seed=0, noise=torch.zeros((3, 5, 15, 91)))
    with pytest.raises(ValueError, match="row_ids"):
        h.rollout(seed=0, row_ids=[1, 2, 3])
    with pytest.raises(ValueError, match="joint_rot"):
        h.pack_frames({"root_pos": torch.zeros(2, 2, 3), "root_rot": torch.zeros(2, 2, 4), "contacts": torch.zeros(2, 2, 15)})
    with pytest.raises(ValueError, match="prev_frames"):
        h.conds({"root_pos": torch.zeros(3, 2, 3), "root_rot": torch.zeros(3, 2, 4), "joint_rot": torch.zeros(3, 2, 14, 4), "contacts": torch.zeros(3, 2, 15)})


# ---- the script's chunking and naming ---------------------------------------------------------------------------------------------------------
class FakeHandle:
    def __init__(self):
        self.scenes, self.ids, self.pids = [], [], []

    def set_scene(self, hfs, mps, dx, paths, k):
        self.scenes.append((hfs.shape[0], k))
        self.P, self.K = hfs.shape[0], k

    def rollout(self, seed=None, row_ids=None, path_ids=None):
        self.ids.append(np.asarray(row_ids))
        self.pids.append(np.asarray(path_ids))
        n = self.P * self.K
        return types.SimpleNamespace(final_frame=torch.full((n,), 9, dtype=torch.int32), windows=2)

    def select(self, res, top_k=None, seed=None):
        return [dict(path=p, rows=np.arange(p * self.K, p * self.K + top_k), total_loss=np.arange(top_k, dtype=np.float32),
                     contact_loss=np.zeros(top_k, np.float32), pen_loss=np.zeros(top_k, np.float32)) for p in range(self.P)]

    def to_clips(self, res, rows):
        from parc_amd.motion_opt import OptClip
        z = np.zeros
        return [OptClip(z((9, 3), np.float32), z((9, 4), np.float32), z((9, 14, 4), np.float32), z((9, 15), np.float32), z((16, 16), np.float32),
                        z(2, np.float32), 0.4) for _ in rows]


def test_script_chunks_and_names(tmp_path):
    sys.path.insert(0, os.path.join(REPO, "scripts"))
    import generate_path_motions as S
    from parc_amd import ms_file
    files = []
    for b in range(2):                                             # 5 terrains per batch, terrain 2 without a path
        pts = [np.arange(9, dtype=np.float32).reshape(3, 3) if q != 2 else np.zeros((0, 3), np.float32) for q in range(5)]
        f = tmp_path / f"paths_{b:04d}.npz"
        np.savez(f, hf=np.zeros((5, 16, 16), np.float32), min_point_offset=np.zeros((5, 2), np.float32), dx=np.float32(0.4), points=np.concatenate(pts),
                 point_off=np.concatenate([[0], np.cumsum([len(p) for p in pts])]))
        files.append(str(f))
    h = FakeHandle()
    stats = S.run(h, files, str(tmp_path / "out"), candidates=3, top_k=2, seed=0, max_batch=8)
    assert h.scenes == [(2, 3), (2, 3)] * 2                        # 4 found paths per batch, two paths (6 rows) fit 8
    assert stats == dict(paths=8, rows=24, finished=24, windows=8)
    assert np.array_equal(h.ids[1], 2 * 3 + np.arange(6)) and np.array_equal(np.concatenate(h.pids), np.arange(8))   # numbered through the files
    assert len(np.unique(np.concatenate(h.ids))) == 24
    names = sorted(os.listdir(tmp_path / "out"))
    assert names == sorted(S.file_name(b, q, r) for b in range(2) for q in (0, 1, 3, 4) for r in range(2))
    assert names[0] == "path_0000_00000_0.pkl"
    d = ms_file.load_ms_file(str(tmp_path / "out" / names[0]))
    assert d.motion_data.root_pos.shape == (9, 3) and d.misc_data["final_frame"] == 9 and d.terrain_data.hf.shape == (16, 16)
    with pytest.raises(SystemExit, match="candidates"):
        S.run(h, files, str(tmp_path / "out"), candidates=9, top_k=2, seed=0, max_batch=8)
    n = len(h.scenes)
    with pytest.raises(SystemExit, match="row ids"):            # refused before the first rollout, not in the middle of the output
        S.run(h, files, str(tmp_path / "out2"), candidates=1 << 26, top_k=2, seed=0, max_batch=1 << 27)
    assert len(h.scenes) == n and not os.path.exists(tmp_path / "out2")
