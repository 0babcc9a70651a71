"""Motion-terrain analysis on the GPU (parc_mterr_*) against the reference fixtures (tests/golden/make_golden_motion_terrain.py)."""
import ctypes as C
import os

import numpy as np
import pytest

from parc_amd import motion_opt as mo
from parc_amd import motion_terrain as mt

pytestmark = pytest.mark.gpu

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CHAR = os.path.join(REPO, "data/assets/humanoid.xml")
FIXTURES = ["civilization", "TEASER_TERRAIN", "dec2024_teaser_717_1_modified_opt", "dec2024_lowered", "civilization_zb2_jb05"]
BOUNDARY_M = 1e-5


def fixture(name):
    return dict(np.load(os.path.join(REPO, "tests/golden", f"motion_terrain_{name}.npz")))


def clip_of(z):
    return mo.OptClip(z["root_pos"], z["root_rot"], z["joint_rot"], z["contacts"], z["hf"], z["min_point"], float(z["dx"]))


def bufs(z):
    return dict(z_buf=float(z["z_buf"]), jump_buf=float(z["jump_buf"]), max_jerk=float(z["max_jerk"]))


def ref_inds(z):
    return np.split(z["mask_inds"].astype(np.int64), np.cumsum(z["mask_counts"])[:-1])


def boundary_frames(z, tol=BOUNDARY_M):
    """Frames with a reference sample point within `tol` of a half-cell boundary (the only cells fp32 rounding may move)."""
    bp = z["boundary_points"]
    if bp.size == 0:
        return set()
    dx = float(z["dx"])
    u = (bp[:, 2:4] - z["min_point"].astype(np.float64)) / dx
    d = np.abs(u - np.floor(u) - 0.5) * dx
    return set(bp[(d < tol).any(-1), 0].astype(int).tolist())


def compare_inds(got, ref, allowed):
    """Frames whose cell sets differ; every one must be explained by a boundary point."""
    assert len(got) == len(ref)
    diff = [f for f, (a, b) in enumerate(zip(got, ref)) if not np.array_equal(a, b)]
    unexplained = [f for f in diff if f not in allowed]
    return diff, unexplained


def ref_points():
    z = fixture(FIXTURES[0])
    return z["points"], z["point_body"]


@pytest.fixture(scope="module")
def analyzer():   # on the reference's own sample points (ours agree within 3e-8 m: test_sampler_matches_reference)
    return mt.MotionTerrainAnalyzer(CHAR, "cuda:0", points=ref_points())


@pytest.fixture(scope="module")
def brute():
    return mt.MotionTerrainAnalyzer(CHAR, "cuda:0", sdf_mode=mt.SDF_BRUTE, points=ref_points())


def test_sampler_matches_reference():
    a = mt.MotionTerrainAnalyzer(CHAR, "cuda:0")
    z = fixture(FIXTURES[0])
    np.testing.assert_array_equal(a.point_body, z["point_body"])
    for b in np.unique(a.point_body):   # per body as a set (the icosahedron's vertex order is not pinned)
        p, r = a.points[a.point_body == b], z["points"][z["point_body"] == b]
        assert np.abs(p[:, None] - r[None]).max(-1).min(1).max() <= 1e-6


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


@pytest.mark.parametrize("name", FIXTURES)
def test_mask_inds_and_hf_maxmin_match_reference(analyzer, name):
    z = fixture(name)
    r = analyzer.analyze([clip_of(z)], **bufs(z))[0]
    allowed = boundary_frames(z)
    diff, unexplained = compare_inds(r["hf_mask_inds"], ref_inds(z), allowed)
    print(f"{name}: {len(allowed)} frames with a reference point within {BOUNDARY_M} m of a half-cell boundary; "
          f"{len(diff)} frames differ")
    assert not unexplained, unexplained
    for a in r["hf_mask_inds"]:
        assert a.dtype == np.int64 and a.ndim == 2 and a.shape[1] == 2
    # the bounds must be the reference's bits on every cell no differing frame covers (in either result)
    agree = np.ones(z["hf"].shape, bool)
    for f in diff:
        for c in (r["hf_mask_inds"][f], ref_inds(z)[f]):
            agree[c[:, 0], c[:, 1]] = False
    np.testing.assert_array_equal(r["hf_maxmin"][agree], z["hf_maxmin"][agree])
    mh, tc = analyzer.min_heights()
    touched = tc.reshape(z["hf"].shape).astype(bool)
    ref_touched = z["min_body_heights"] != np.float32(mt.MISSING_POINT_VALUE)
    np.testing.assert_array_equal(touched[agree], ref_touched[agree])
    # the lowest point per cell comes from the device FK, which differs from torch's by an ulp at some points
    sel = touched & agree
    got, ref = mh.reshape(z["hf"].shape)[sel], z["min_body_heights"][sel]
    print(f"{name}: lowest points differ in {(got != ref).sum()} of {got.size} cells, by <= {np.abs(got - ref).max():.3g} m")
    np.testing.assert_allclose(got, ref, atol=1e-6, rtol=0)


@pytest.mark.parametrize("name", FIXTURES)
def test_scores_and_point_sdfs_match_reference(analyzer, name):
    z = fixture(name)
    r = analyzer.analyze([clip_of(z)], **bufs(z))[0]
    for k in ("pen_loss", "contact_loss"):
        assert abs(r[k] - z[k]) <= 1e-5 * abs(z[k]) + 1e-6, (k, r[k], float(z[k]))
    for k in ("mean_jerk", "jerk_frac"):
        assert abs(r[k] - z[k]) <= 1e-5 * abs(z[k]) + 1e-12, (k, r[k], float(z[k]))
    assert r["max_root_z"] == np.float32(z["root_pos"][:, 2].max())
    assert r["min_hf"] == z["hf"].min()
    for i, f in enumerate(z["sdf_frames"]):
        g, a = analyzer.point_sdf(int(f), 1)
        np.testing.assert_allclose(g[0], z["sdf_ground"][i], atol=1e-5, rtol=0)
        np.testing.assert_allclose(a[0], z["sdf_air"][i], atol=1e-5, rtol=0)


def test_pruned_sdf_is_bit_identical_to_brute_force_on_fixtures(analyzer, brute):
    clips = [clip_of(fixture(n)) for n in FIXTURES[:4]]
    a = analyzer.run(clips)
    b = brute.run(clips)
    assert np.array_equal(bits(a["clip_out"]), bits(b["clip_out"]))
    assert np.array_equal(a["inds"], b["inds"]) and np.array_equal(a["hf_maxmin"], b["hf_maxmin"])
    F = int(a["packed"]["frame_off"][-1])
    ga, aa = analyzer.point_sdf(0, F)
    gb, ab = brute.point_sdf(0, F)
    assert np.array_equal(bits(ga), bits(gb)) and np.array_equal(bits(aa), bits(ab))


def _random_step_terrain(n=1001, dx=0.4, seed=0):
    rng = np.random.default_rng(seed)
    blocks = rng.integers(-4, 9, size=(n // 5 + 1, n // 5 + 1)).astype(np.float32) * np.float32(0.5)
    hf = np.kron(blocks, np.ones((5, 5), np.float32))[:n, :n]
    hf += rng.uniform(-0.05, 0.05, size=hf.shape).astype(np.float32)
    return np.ascontiguousarray(hf, np.float32), np.array([-200.0, -150.0], np.float32), dx


def test_pruned_sdf_is_bit_identical_on_a_1001_cell_random_step_terrain(analyzer, brute):
    hf, mn, dx = _random_step_terrain()
    base = clip_of(fixture("dec2024_teaser_717_1_modified_opt"))
    rng = np.random.default_rng(3)
    n = 24
    idx = np.arange(n) % base.num_frames
    rp = base.root_pos[idx].copy()
    ix = rng.integers(0, hf.shape[0], n)
    iy = rng.integers(0, hf.shape[1], n)
    ix[:2], iy[:2] = [0, hf.shape[0] - 1], [0, hf.shape[1] - 1]           # corners
    rp[:, 0] = mn[0] + ix * dx + rng.uniform(-0.5, 0.5, n).astype(np.float32)
    rp[:, 1] = mn[1] + iy * dx + rng.uniform(-0.5, 0.5, n).astype(np.float32)
    rp[:, 2] = hf[ix, iy] + np.linspace(-3.0, 15.0, n).astype(np.float32)   # points from 3 m below to 15 m above
    rp[-1, 0] = mn[0] - 5.0                                                  # off the terrain
    c = mo.OptClip(rp, base.root_rot[idx].copy(), base.joint_rot[idx].copy(), base.contacts[idx].copy(), hf, mn, dx)
    a = analyzer.run([c])
    b = brute.run([c])
    assert np.array_equal(bits(a["clip_out"]), bits(b["clip_out"]))
    assert np.array_equal(a["hf_maxmin"], b["hf_maxmin"])
    ga, aa = analyzer.point_sdf(0, n)
    gb, ab = brute.point_sdf(0, n)
    assert np.array_equal(bits(ga), bits(gb)) and np.array_equal(bits(aa), bits(ab))
    assert (ga > 1.0).any() and (aa > 0.5).any()                              # points well above and well below the surface


def _synthetic_clips(n, seed=0):
    rng = np.random.default_rng(seed)
    bases = [clip_of(fixture(f)) for f in FIXTURES[:3]]
    out = []
    for i in range(n):
        b = bases[i % 3]
        L = [1, 3, 4, 7, 400][i] if i < 5 else int(rng.integers(1, 401))
        idx = np.arange(L) % b.num_frames
        c = mo.OptClip(b.root_pos[idx].copy(), b.root_rot[idx].copy(), b.joint_rot[idx].copy(), b.contacts[idx].copy(),
                       b.hf, b.min_point, b.dx)
        c.root_pos[:, :2] += rng.normal(0, 0.1, 2).astype(np.float32)
        c.root_pos[:, 2] -= np.float32(rng.uniform(0.0, 0.3))
        if i == 6:   # points off the terrain edge
            c.root_pos[:, 0] += np.float32(b.hf.shape[0] * b.dx)
        out.append(c)
    return out


def _same(r1, i, r2, j):
    o1, o2 = r1[i], r2[j]
    for k in mt.CLIP_OUTPUTS:
        assert np.array_equal(np.float32(o1[k]).view(np.int32), np.float32(o2[k]).view(np.int32)), (k, o1[k], o2[k])
    assert np.array_equal(o1["hf_maxmin"], o2["hf_maxmin"])
    assert len(o1["hf_mask_inds"]) == len(o2["hf_mask_inds"])
    for a, b in zip(o1["hf_mask_inds"], o2["hf_mask_inds"]):
        assert np.array_equal(a, b)


def test_batching_is_bit_identical_to_single_runs(analyzer):
    clips = _synthetic_clips(64)
    batch = analyzer.analyze(clips)
    for i, c in enumerate(clips):
        _same(batch, i, analyzer.analyze([c]), 0)
    assert np.isnan(batch[0]["mean_jerk"]) and np.isnan(batch[1]["jerk_frac"]) and np.isfinite(batch[2]["mean_jerk"])   # 1, 3, 4 frames


def test_large_batch_sampled_clips_bit_identical(analyzer):
    clips = _synthetic_clips(1024, seed=1)
    batch = analyzer.analyze(clips)
    for i in [0, 5, 100, 333, 512, 777, 1000, 1023]:
        _same(batch, i, analyzer.analyze([clips[i]]), 0)


def _near_boundary_frames(z, shift, tol):
    """Frames with a sample point (numpy FK of the clip moved by `shift`) within `tol` of a half-cell boundary."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import motion_terrain_ref as ref
    from parc_amd.char_model import CharModel
    rp = z["root_pos"].copy()
    rp[:, :2] += np.float32(shift)
    pos, rot = ref.fk(CharModel(CHAR), rp, z["root_rot"], z["joint_rot"])
    w = ref.world_points(pos, rot, z["points"], z["point_body"])[..., :2].astype(np.float64)
    u = (w - (z["min_point"].astype(np.float64) + shift)) / float(z["dx"])
    return set(np.nonzero((np.abs(u - np.floor(u) - 0.5) * float(z["dx"]) < tol).any(axis=(1, 2)))[0].tolist())


def test_clip_and_terrain_moved_1km(analyzer):
    z = fixture("dec2024_teaser_717_1_modified_opt")   # contact 13 and penetration 456: sums of many terms, each ~6e-5 m coarser 1 km out
    c = clip_of(z)
    far = mo.OptClip(c.root_pos.copy(), c.root_rot, c.joint_rot, c.contacts, c.hf, c.min_point + np.float32(1000.0), c.dx)
    far.root_pos[:, :2] += np.float32(1000.0)
    a, b = analyzer.analyze([c, far])
    diff = [f for f, (x, y) in enumerate(zip(a["hf_mask_inds"], b["hf_mask_inds"])) if not np.array_equal(x, y)]
    # fp32 resolves ~6e-5 m at 1 km and FK adds a few ulps: a differing frame must have a point within 5e-4 m of a half-cell boundary
    near = _near_boundary_frames(z, 0.0, 5e-4) | _near_boundary_frames(z, 1000.0, 5e-4)
    print(f"1 km: {len(diff)} of {len(a['hf_mask_inds'])} frames differ; {len(near)} frames have a point within 5e-4 m of a boundary")
    assert set(diff) <= near, sorted(set(diff) - near)
    for k in ("pen_loss", "contact_loss", "mean_jerk"):
        assert abs(a[k] - b[k]) <= 1e-3 * abs(a[k]), (k, a[k], b[k])


def test_nan_frame_poisons_only_its_clip(analyzer):
    clips = _synthetic_clips(3, seed=2)[2:] + [clip_of(fixture(n)) for n in FIXTURES[:2]]
    clips[1] = mo.OptClip(**{**clips[1].__dict__})
    clips[1].root_pos = clips[1].root_pos.copy()
    clips[1].root_pos[5, 0] = np.nan
    r = analyzer.analyze(clips)
    for k in ("pen_loss", "contact_loss", "mean_jerk", "jerk_frac", "max_root_z"):
        assert np.isnan(r[1][k]), k
    assert len(r[1]["hf_mask_inds"][5]) == 0 and len(r[1]["hf_mask_inds"][4]) > 0
    for i in (0, 2):
        _same(r, i, analyzer.analyze([clips[i]]), 0)
        assert np.isfinite([r[i][k] for k in ("pen_loss", "contact_loss", "max_root_z")]).all()


def test_argument_errors(analyzer):
    from gpu_helpers import SHARED_CLIP_ARRAYS, raises_invalid
    from parc_amd import lib as L
    z = fixture("TEASER_TERRAIN")
    lib = L.load()
    p = mt.analyzer_params(analyzer.char_model, analyzer.points, analyzer.point_body)
    p.struct_size -= 8
    h = C.c_void_p()
    with pytest.raises(L.ParcError, match="struct_size"):
        L.check(lib.parc_mterr_create(C.byref(p), C.byref(h)))
    p = mt.analyzer_params(analyzer.char_model, analyzer.points, analyzer.point_body, sdf_mode=7)
    with pytest.raises(L.ParcError, match="sdf_mode"):
        L.check(lib.parc_mterr_create(C.byref(p), C.byref(h)))
    with pytest.raises(ValueError):
        analyzer.analyze([])
    p = mt.analyzer_params(analyzer.char_model, analyzer.points, analyzer.point_body)
    L.check(lib.parc_mterr_create(C.byref(p), C.byref(h)))
    try:
        with pytest.raises(L.ParcError, match="set_clips first"):
            L.check(lib.parc_mterr_run(h, None, None, None, None))
        pk = mo.pack_clips([clip_of(z)], analyzer.B, analyzer.D)
        st = mt.clip_struct(pk, 0)
        with pytest.raises(L.ParcError, match="num_clips"):
            L.check(lib.parc_mterr_set_clips(h, C.byref(st)))
        bad = dict(pk, hf_dims=np.ascontiguousarray([[z["hf"].shape[0] + 1, z["hf"].shape[1]]], np.int32))
        st = mt.clip_struct(bad, 1)
        with pytest.raises(L.ParcError, match="dims"):
            L.check(lib.parc_mterr_set_clips(h, C.byref(st)))
        bad = dict(pk, hf_geom=np.ascontiguousarray([[0, 0, 0, 0]], np.float32))
        st = mt.clip_struct(bad, 1)
        with pytest.raises(L.ParcError, match="dx"):
            L.check(lib.parc_mterr_set_clips(h, C.byref(st)))
        # one fault per call: the return code and the whole message (the strings of parc_mterr_set_clips)
        nf = int(pk["frame_off"][1])
        faults = [(pk, 0, "mterr: num_clips must be >= 1"),
                  (dict(pk, frame_off=np.array([1, nf + 1], np.int64)), 1, "mterr: offsets must start at 0"),
                  (dict(pk, hf_off=pk["hf_off"] + 1), 1, "mterr: offsets must start at 0"),
                  (dict(pk, frame_off=np.zeros(2, np.int64)), 1, "mterr: clip 0 has no frames"),
                  (dict(pk, hf_dims=np.ascontiguousarray([[z["hf"].shape[0] + 1, z["hf"].shape[1]]], np.int32)), 1,
                   "mterr: heightfield dims / offsets disagree (dims >= 1, at most 2^31 - 1 cells)"),
                  (dict(pk, hf_geom=np.ascontiguousarray([[0, 0, 0, 0.4]], np.float32)), 1, "mterr: dx must be > 0")]
        faults += [(pk, 1, (name, "mterr: null clip array")) for name in SHARED_CLIP_ARRAYS]
        for bad, n, msg in faults:   # `bad` owns the arrays the struct points to
            st = mt.clip_struct(bad, n)
            if isinstance(msg, tuple):   # (field passed as NULL, message)
                setattr(st, msg[0], None)
                msg = msg[1]
            raises_invalid(lambda: lib.parc_mterr_set_clips(h, C.byref(st)), msg)
        st = mt.clip_struct(pk, 1)
        st.cons_off_host = st.cons_body_host = st.cons_range_host = st.cons_point_host = None   # the analyser reads no constraints
        L.check(lib.parc_mterr_set_clips(h, C.byref(st)))
    finally:
        lib.parc_mterr_destroy(h)
    h2 = C.c_void_p()
    p = mt.analyzer_params(analyzer.char_model, analyzer.points, analyzer.point_body)
    p.struct_size -= 8
    created = [(p, "ParcMotionTerrainParams ABI mismatch (struct_size)"),
               (mt.analyzer_params(analyzer.char_model, analyzer.points, analyzer.point_body[::-1]),
                "mterr: point bodies must be in [0, B) and non-decreasing")]
    for p, msg in created:
        raises_invalid(lambda: lib.parc_mterr_create(C.byref(p), C.byref(h2)), msg)
        assert not h2.value


def test_env_step_and_motion_opt_step_unchanged_by_the_analyzer():
    import torch
    from gpu_helpers import default_config
    from parc_amd.envs.hip_parkour_env import HipParkourEnv
    zo = dict(np.load(os.path.join(REPO, "tests/golden/motion_opt_dec2024_teaser_717_1_modified_opt_s1.npz")))
    cfg = {k: float(v) for k, v in zip(mo.WEIGHT_KEYS, zo["weights"])}
    cfg.update(max_jerk=float(zo["max_jerk"]), step_size=float(zo["step_size"]))
    oc = mo.OptClip(zo["root_pos"], zo["root_rot"], zo["joint_rot"], zo["contacts"], zo["hf"], zo["min_point"], float(zo["dx"]))

    def env_and_opt():
        torch.manual_seed(0)
        np.random.seed(0)
        env = HipParkourEnv(default_config(), 8, "cuda:0", False)
        env.reset()
        obs, rew, done, _ = env.step(env._char_dof_pos.clone())
        torch.cuda.synchronize()
        out = [obs.cpu().numpy().copy(), rew.cpu().numpy().copy()]
        del env
        opt = mo.MotionOptimizer(CHAR, "cuda:0", cfg)
        opt.set_clips([oc])
        out.append(opt.step(3))
        out.append(opt.get_params())
        return out

    before = env_and_opt()
    mt.MotionTerrainAnalyzer(CHAR, "cuda:0").analyze(_synthetic_clips(16))
    after = env_and_opt()
    for a, b in zip(before, after):
        assert np.array_equal(a.view(np.int32) if a.dtype == np.float32 else a, b.view(np.int32) if b.dtype == np.float32 else b)


def test_scripts_end_to_end(tmp_path):
    import sys
    import yaml
    sys.path.insert(0, os.path.join(REPO, "scripts"))
    import preprocess_motions as pm
    import run_optimize_motions as drv
    import score_motions as sm
    from parc_amd import ms_file
    names = ("dec2024_teaser_717_1_modified_opt.pkl", "sfu.pkl")
    # the optimiser's opt-in stage-2 extras: the optimised frames' cells and bounds
    cfg = yaml.safe_load(open(os.path.join(REPO, "data/configs/motion_opt/motion_opt_default.yaml")))
    ds = tmp_path / "ds.yaml"
    ds.write_text(yaml.safe_dump({"motions": [{"file": os.path.join(REPO, "data/motion_terrains", f), "weight": 1.0} for f in names]}))
    cfg.update(motions_yaml_path=str(ds), output_folder_path=str(tmp_path / "opt"), num_iters=5, log_every=5)
    (tmp_path / "c.yaml").write_text(yaml.safe_dump(cfg))
    paths = drv.main(["--config", str(tmp_path / "c.yaml"), "--hf_extras"])
    a = mt.MotionTerrainAnalyzer(CHAR, "cuda:0")
    for p in paths:
        d = ms_file.load_ms_file(p)
        m = d.motion_data
        r = a.analyze([mo.OptClip(m.root_pos, m.root_rot, m.joint_rot, m.body_contacts, d.terrain_data.hf, d.terrain_data.min_point,
                                  d.terrain_data.dx)])[0]
        np.testing.assert_array_equal(d.terrain_data.hf_maxmin, r["hf_maxmin"])
        assert len(d.misc_data["hf_mask_inds"]) == m.root_pos.shape[0]
        for x, y in zip(d.misc_data["hf_mask_inds"], r["hf_mask_inds"]):
            assert np.array_equal(x, y)
    # preprocessing in place on copies, then the scores of the same files
    src = tmp_path / "src"
    src.mkdir()
    for f in names:
        (src / f).write_bytes(open(os.path.join(REPO, "data/motion_terrains", f), "rb").read())
    written, _ = pm.main([str(src)])
    assert len(written) == 2
    rows = sm.main([str(src), "--out", str(tmp_path / "s.csv")])
    lines = (tmp_path / "s.csv").read_text().splitlines()
    assert len(rows) == 2 and len(lines) == 1 + 2 + 4
    for f, row in zip(sorted(names), rows):
        z = a.analyze([mo.clip_from_ms(str(src / f))])[0]
        assert row["pen_loss"] == z["pen_loss"] and row["contact_loss"] == z["contact_loss"] and row["final_node_dist"] is None


# ---- the handle across set_clips calls: what a batch leaves behind must not reach the next one --------------------------------------
def _reload_clips():
    """A: the TEASER_TERRAIN fixture clip (58 frames, 102 x 102 cells).  B: its first 8 frames (the analyser takes 1; the jerk window
    needs 4) on a cropped terrain that still holds every cell those frames touch."""
    A = clip_of(fixture("TEASER_TERRAIN"))
    n = 8
    B = mo.OptClip(A.root_pos[:n].copy(), A.root_rot[:n].copy(), A.joint_rot[:n].copy(), A.contacts[:n].copy(),
                   np.ascontiguousarray(A.hf[:80, :60]), A.min_point, A.dx)
    return A, B


def _all_outputs(a, r):
    """run's outputs (r: what MotionTerrainAnalyzer.run returned, mask inds included) and the lowest points, as bit patterns."""
    mh, tc = a.min_heights()
    return [bits(r["clip_out"]), r["counts"], r["inds"], bits(r["hf_maxmin"]), bits(mh), tc]


def _same_outputs(x, y):
    assert len(x) == len(y)
    for i, (p, q) in enumerate(zip(x, y)):
        assert p.shape == q.shape and np.array_equal(p, q), i


@pytest.mark.parametrize("order", ["shrink", "grow"])
def test_a_reload_equals_a_fresh_handle(order):
    """shrink: [A, B] then [B].  grow: [B] then [A, B], where get_mask_inds has to grow its buffer between the two runs."""
    A, B = _reload_clips()
    first, second = ([A, B], [B]) if order == "shrink" else ([B], [A, B])
    a = mt.MotionTerrainAnalyzer(CHAR, "cuda:0", points=ref_points())
    r1 = a.run(first)
    h = a._h
    got = _all_outputs(a, a.run(second))
    assert a._h.value == h.value                     # the same handle served both batches
    fresh = mt.MotionTerrainAnalyzer(CHAR, "cuda:0", points=ref_points())
    _same_outputs(got, _all_outputs(fresh, fresh.run(second)))
    n1, n2 = len(r1["inds"]), len(got[2])
    assert n1 > 0 and n2 > 0 and (n2 > n1) == (order == "grow")


def test_a_rejected_batch_leaves_the_previous_one_usable():
    from gpu_helpers import raises_invalid
    from parc_amd import lib as L
    A, _ = _reload_clips()
    a = mt.MotionTerrainAnalyzer(CHAR, "cuda:0", points=ref_points())
    r = a.run([A])
    before = _all_outputs(a, r)
    g0, a0 = a.point_sdf(3, 2)
    pk = r["packed"]
    bad = dict(pk, hf_geom=np.ascontiguousarray([[0, 0, 0, 0.4]], np.float32))
    st = mt.clip_struct(bad, 1)
    raises_invalid(lambda: a._lib.parc_mterr_set_clips(a._h, C.byref(st)), "mterr: dx must be > 0")
    # the same run again, on the batch the handle still holds (MotionTerrainAnalyzer.run would load it anew)
    out, counts, maxmin = np.zeros_like(r["clip_out"]), np.zeros_like(r["counts"]), np.zeros_like(r["hf_maxmin"])
    total = C.c_int64()
    L.check(a._lib.parc_mterr_run(a._h, L.np_f32p(out), L.np_i32p(counts), L.np_f32p(maxmin), C.byref(total)))
    inds = np.zeros((int(total.value), 2), np.int32)
    L.check(a._lib.parc_mterr_get_mask_inds(a._h, L.np_i32p(inds)))
    _same_outputs(before, _all_outputs(a, dict(clip_out=out, counts=counts, inds=inds, hf_maxmin=maxmin)))
    g1, a1 = a.point_sdf(3, 2)
    assert np.array_equal(bits(g0), bits(g1)) and np.array_equal(bits(a0), bits(a1))
