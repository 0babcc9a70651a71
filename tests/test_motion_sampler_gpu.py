"""The motion-window sampler kernels (parc_msamp_*) against the reference fixtures and the CPU restatement."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, ".."))
sys.path.insert(0, HERE)

from gpu_helpers import write_motion_yaml  # noqa: E402

pytestmark = pytest.mark.gpu

CHAR = os.path.join(REPO, "data/assets/humanoid.xml")
CASES = ["root_boxes", "floor_boxes", "noise", "none"]
TOL = 1e-5   # the bar of tests/test_device_ops_gpu.py for parc_calc_motion_frame / FK against the reference goldens (SURVEY's contract)
MOTION_KEYS = ("root_pos", "root_rot", "joint_pos", "joint_rot", "contacts")
NAMES = dict(root_pos="ROOT_POS", root_rot="ROOT_ROT", joint_pos="JOINT_POS", joint_rot="JOINT_ROT", contacts="CONTACTS")


def fixture(case):
    z = dict(np.load(os.path.join(REPO, "tests/golden", f"motion_sampler_{case}.npz")))
    z["cfg"] = json.loads(str(z["config"]))
    return z


def extra_vals(clip_names):
    """The reference's own hf_mask_inds / hf_maxmin of the fixture clips (tests/golden/motion_terrain_<clip>.npz)."""
    out = []
    for c in clip_names:
        t = np.load(os.path.join(REPO, "tests/golden", f"motion_terrain_{c}.npz"))
        off = np.concatenate([[0], np.cumsum(t["mask_counts"])])
        out.append(dict(hf_mask_inds=[t["mask_inds"][off[f]:off[f + 1]].astype(np.int64) for f in range(len(t["mask_counts"]))],
                        hf_maxmin=t["hf_maxmin"]))
    return out


def plan_of(z):
    return {k[5:]: z[k] for k in z if k.startswith("plan_")}


def close(a, b, tol, what=""):
    """tests/test_device_ops_gpu.py's bar: absolute error against tol + 2 ulp of the value.  Returns the plain maximum error."""
    err = np.abs(a - b) / (1.0 + (2.4e-7 / tol) * np.abs(b))
    print(f"{what}: max abs err {np.abs(a - b).max():.3e}")
    assert np.all(np.isfinite(err)) and err.max() <= tol, f"{what}: max err {err.max()} at {np.unravel_index(err.argmax(), err.shape)}"


_SAMPLERS = {}


def sampler_for(case, tmp_path_factory, weights=(1.0, 1.0)):
    from parc_amd import motion_sampler as ms
    key = (case, tuple(weights))
    if key not in _SAMPLERS:
        z = fixture(case)
        clips = [str(c) for c in z["clips"]]
        y = write_motion_yaml(tmp_path_factory.mktemp("msamp"), clips, weights)
        _SAMPLERS[key] = ms.MotionWindowSampler(z["cfg"], y, CHAR, "cuda:0", extra_vals=extra_vals(clips))
    return _SAMPLERS[key]


def outputs(ret):
    """sample_with's tuple -> dict of numpy arrays."""
    motion, hfs, tp, tr = ret[:4]
    o = {k: motion[NAMES[k]].cpu().numpy() for k in MOTION_KEYS}
    if "FLOOR_HEIGHTS" in motion:
        o["floor_heights"] = motion["FLOOR_HEIGHTS"].cpu().numpy()[..., 0]
    o.update(hfs=hfs.cpu().numpy(), target_pos=tp.cpu().numpy(), target_rot=tr.cpu().numpy())
    if len(ret) > 4:
        o["hf_bounds"] = ret[4].cpu().numpy()
    return o


def bits_equal(a, b):
    return all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in a)


@pytest.mark.parametrize("case", CASES)
def test_sample_with_matches_reference_and_restatement(case, tmp_path_factory):
    """Measured on the MI355X (max abs error against the fixture / the CPU restatement): see DESIGN.md section 8f."""
    import motion_sampler_ref as ref
    import helpers
    from parc_amd.char_model import CharModel
    z = fixture(case)
    s = sampler_for(case, tmp_path_factory)
    o = outputs(s.sample_with(s.plan_from_numpy(plan_of(z)), return_bounds=True, validate=True))
    clips = [str(c) for c in z["clips"]]
    r = ref.sample_with(ref.Library(helpers.load_clips(clips), extra_vals(clips)), CharModel(CHAR), s.cfg, plan_of(z))
    for k in MOTION_KEYS + ("target_pos", "target_rot"):
        close(o[k], z[k], TOL, f"{case} {k} vs reference")
        close(o[k], r[k], TOL, f"{case} {k} vs restatement")
    keep = ~z["skip"]
    assert z["skip"].mean() <= 0.01
    if s.cfg.relative_z_style == 1:   # gather, a difference of two gathered values, max, clamp, select: exact outside the recorded cells
        assert np.array_equal(o["hfs"][keep], z["hfs"][keep])
        assert np.array_equal(o["floor_heights"], z["floor_heights"])
        sub = z["hf_raw"][:, s.cfg.num_x_neg, s.cfg.num_y_neg]
        assert np.array_equal(o["hf_bounds"][keep], (z["bounds_raw"] - sub[:, None, None, None])[keep])
    else:                              # the only inexact input is the reference root z; max-pool, clamp, select are 1-Lipschitz
        close(o["hfs"][keep], z["hfs"][keep], TOL, f"{case} hfs vs reference")
        close(o["hfs"][keep], r["hfs"][keep], TOL, f"{case} hfs vs restatement")


def test_window_bounds_differ_from_clip_bounds_and_match(tmp_path_factory):
    """A sample's per-window bounds differ from the whole-clip hf_maxmin at some cell, and the kernel returns the per-window ones."""
    z = fixture("floor_boxes")
    s = sampler_for("floor_boxes", tmp_path_factory)
    o = outputs(s.sample_with(s.plan_from_numpy(plan_of(z)), return_bounds=True))
    ev = extra_vals([str(c) for c in z["clips"]])
    keep = ~z["skip"]
    sub = z["hf_raw"][:, s.cfg.num_x_neg, s.cfg.num_y_neg]
    window = z["bounds_raw"] - sub[:, None, None, None]
    assert np.array_equal(o["hf_bounds"][keep], window[keep])
    differ = 0
    for i, m in enumerate(z["plan_motion_id"]):
        # the whole-clip bounds the patch would get without the window mask: every touched cell of the clip keeps its hf_maxmin
        mm = ev[m]["hf_maxmin"]
        whole_vals = {tuple(v) for v in mm.reshape(-1, 2).tolist()}
        raw = z["bounds_raw"][i].reshape(-1, 2)
        default = np.array([6.0, -6.0], np.float32)
        is_default = (raw == default).all(-1)
        assert all(tuple(v) in whole_vals for v in raw[~is_default].tolist())      # masked cells carry the clip's values
        differ += int(is_default.sum())                                             # the others carry (2 max_h, -2 max_h), no clip value
        assert not any((np.array(v, np.float32) == default).all() for v in whole_vals)
    assert differ > 0


def test_batch_invariance(tmp_path_factory):
    """Every fixture sample gives the same bits alone, in its batch, and in a shuffled batch of 1 000 copies and mixtures."""
    for case in ("root_boxes", "floor_boxes", "noise"):
        z = fixture(case)
        s = sampler_for(case, tmp_path_factory)
        p = plan_of(z)
        n = len(p["motion_id"])
        full = outputs(s.sample_with(s.plan_from_numpy(p), return_bounds=True))
        for i in range(n):
            one = outputs(s.sample_with(s.plan_from_numpy({k: v[i:i + 1] for k, v in p.items()}), return_bounds=True))
            assert bits_equal(one, {k: v[i:i + 1] for k, v in full.items()}), (case, i)
        order = np.random.RandomState(3).randint(0, n, 1000)
        big = outputs(s.sample_with(s.plan_from_numpy({k: v[order] for k, v in p.items()}), return_bounds=True))
        assert bits_equal(big, {k: v[order] for k, v in full.items()}), case


def test_plan_and_seed_consistency(tmp_path_factory):
    import torch
    for case in ("root_boxes", "noise"):
        s = sampler_for(case, tmp_path_factory)
        a, b = outputs(s.sample(257, 11)), outputs(s.sample(257, 11))
        assert bits_equal(a, b)
        plan = s.draw_plan(257, 11)
        c = outputs(s.sample_with(plan, validate=True))
        assert bits_equal(a, c)
        d = outputs(s.sample(257, 12))
        assert not np.array_equal(a["hfs"], d["hfs"]) and not np.array_equal(a["root_pos"], d["root_pos"])
        plan2 = s.draw_plan(257, 11)
        assert all(torch.equal(plan[k], plan2[k]) for k in plan)
        # a sample's draws depend on (seed, index) only: the first 10 of a longer plan are the same
        plan3 = s.draw_plan(1000, 11)
        assert all(torch.equal(plan[k][:10], plan3[k][:10]) for k in plan)


def within(count, n, p):
    """Binomial bound at 5 sigma, from n and p."""
    return abs(count - n * p) <= 5.0 * np.sqrt(n * p * (1.0 - p))


def test_plan_distributions(tmp_path_factory):
    n = 65536
    s = sampler_for("root_boxes", tmp_path_factory, weights=(1.0, 3.0))
    c = s.cfg
    plan = {k: v.cpu().numpy() for k, v in s.draw_plan(n, 2024).items()}
    mid, t0, tf = plan["motion_id"], plan["t0"], plan["t_future"]
    length = s.lengths[mid]
    assert mid.min() >= 0 and mid.max() < 2
    assert (t0 >= 0).all() and (t0 + np.float32((c.T - 1) / c.sequence_fps) <= length).all()       # every CLAMP window fits
    rem = np.minimum(length - t0, np.float32(c.future_window_max - c.future_window_min))
    eps = 4 * np.finfo(np.float32).eps * (np.abs(t0) + 2.0)                                       # the fp32 rounding of the sum itself
    assert (tf >= t0 + np.float32(c.future_window_min) - eps).all() and (tf <= t0 + np.float32(c.future_window_min) + rem + eps).all()
    assert within((mid == 1).sum(), n, 0.75)
    assert within(plan["change_height"].sum(), n, c.hf_change_height_chance)
    hv = plan["height_value"]
    assert (np.abs(hv) <= c.max_h).all() and within((hv < 0).sum(), n, 0.5)
    for k in range(3):
        assert within((plan["pool_kind"][:, k] != 0).sum(), n, c.hf_maxpool_chance)
    assert within((plan["pool_kind"] != 0).all(1).sum(), n, c.hf_maxpool_chance ** 3)                # the three rolls are independent
    for v in range(c.max_num_boxes + 1):
        assert within((plan["num_boxes"] == v).sum(), n, 1.0 / (c.max_num_boxes + 1))
    assert plan["num_boxes"].min() == 0 and plan["num_boxes"].max() == c.max_num_boxes
    for k in range(3):
        for v in range(c.hf_max_maxpool_size + 1):
            assert within((plan["pool_size"][:, k] == v).sum(), n, 1.0 / (c.hf_max_maxpool_size + 1))
    # the six pool orders: among the samples that use all three pools the kinds are a permutation of (1, 2, 3)
    allp = plan["pool_kind"][(plan["pool_kind"] != 0).all(1)]
    assert (np.sort(allp, 1) == [1, 2, 3]).all()
    codes = allp[:, 0] * 16 + allp[:, 1] * 4 + allp[:, 2]
    assert len(np.unique(codes)) == 6
    for code in np.unique(codes):
        assert within((codes == code).sum(), len(allp), 1.0 / 6.0)
    # where a pool is used, its kind is uniform over the three functions in every slot
    for k in range(3):
        used = plan["pool_kind"][:, k][plan["pool_kind"][:, k] != 0]
        for v in (1, 2, 3):
            assert within((used == v).sum(), len(used), 1.0 / 3.0)
    bx = plan["boxes"]
    assert (bx[..., 0] >= 0).all() and (bx[..., 0] <= c.Gx).all() and (bx[..., 1] <= c.Gy).all()
    assert (bx[..., 2:4] >= c.box_min_len).all() and (bx[..., 2:4] <= c.box_max_len).all()
    assert (bx[..., 4] >= 0).all() and (bx[..., 4] < 2 * np.pi + 1e-6).all() and (np.abs(bx[..., 5]) <= c.max_h).all()
    assert within((bx[..., 0] < c.Gx / 2).sum(), bx[..., 0].size, 0.5) and within((bx[..., 4] < np.pi).sum(), bx[..., 4].size, 0.5)
    fn = plan["future_pos_noise"] / c.future_pos_noise_scale                                       # standard normal
    assert abs(fn.mean()) <= 5.0 / np.sqrt(fn.size) and within((np.abs(fn) < 1.0).sum(), fn.size, 0.6826894921370859)
    assert abs(fn.std() - 1.0) <= 5.0 / np.sqrt(2 * fn.size)
    assert abs(np.corrcoef(fn[:, 0], fn[:, 1])[0, 1]) <= 5.0 / np.sqrt(n) and abs(np.corrcoef(fn[:, 0], fn[:, 2])[0, 1]) <= 5.0 / np.sqrt(n)
    # start times are uniform over [0, length - sequence_duration]
    u = t0 / (length - np.float32(c.sequence_duration))
    assert within((u < 0.5).sum(), n, 0.5) and within((u < 0.1).sum(), n, 0.1)


def test_noise_plan_field_is_uniform(tmp_path_factory):
    s = sampler_for("noise", tmp_path_factory)
    noise = s.draw_plan(4096, 5)["noise"].cpu().numpy()
    assert noise.shape == (4096, 31, 31) and (np.abs(noise) <= s.cfg.max_h).all()
    assert within((noise < 0).sum(), noise.size, 0.5) and within((noise < -1.5).sum(), noise.size, 0.25)
    assert len(np.unique(noise[0])) > 900 and not np.array_equal(noise[0], noise[1])


def test_augmented_output_stays_in_bounds(tmp_path_factory):
    """For random plans every output cell lies within [max(bounds_min, -max_h), min(bounds_max, max_h)] of its own window bounds, and
    the window's masked cells that are not jump cells (bounds max == min) keep the terrain's height exactly."""
    z = fixture("root_boxes")
    s = sampler_for("root_boxes", tmp_path_factory)
    plain = sampler_for("none", tmp_path_factory)
    plan = s.draw_plan(4096, 99)
    o = outputs(s.sample_with(plan, return_bounds=True, validate=True))
    base = outputs(plain.sample_with(plan))
    mx, mn = o["hf_bounds"][..., 0], o["hf_bounds"][..., 1]
    H = np.float32(s.cfg.max_h)
    lo, hi = np.maximum(mn, -H), np.minimum(mx, H)
    ok = lo <= hi                                  # the interval is empty where a cell's bounds lie wholly outside [-max_h, max_h]:
    print("cells whose bounds lie outside [-max_h, max_h]:", int((~ok).sum()), "of", ok.size)
    assert ok.mean() > 0.9
    assert (o["hfs"][ok] >= lo[ok]).all() and (o["hfs"][ok] <= hi[ok]).all()
    assert np.array_equal(o["hfs"][~ok], np.where(mx < -H, -H, H)[~ok])   # there the final clamp leaves the nearer end of [-max_h, max_h]
    fixed = mx == mn
    assert fixed.any() and np.array_equal(o["hfs"][fixed], base["hfs"][fixed])
    changed = (o["hfs"] != base["hfs"]).any(axis=(1, 2))
    assert changed.mean() > 0.5                                                      # the augmentation does change terrain elsewhere
    for k in MOTION_KEYS + ("target_pos", "target_rot"):
        assert np.array_equal(o[k], base[k])


def test_sequences_and_feature_stats(tmp_path_factory):
    z = dict(np.load(os.path.join(REPO, "tests/golden/motion_sampler_stats.npz")))
    s = sampler_for("root_boxes", tmp_path_factory)
    seq = s.motion_sequences_for_id(int(z["seq_clip"]))
    assert seq["ROOT_POS"].shape[0] == int(z["seq_windows"])
    for k in MOTION_KEYS:
        close(seq[NAMES[k]].cpu().numpy()[z["seq_starts"]], z["seq_" + k], TOL, f"sequences {k}")
    # the enumerated windows are the sampled windows at t0 = frame / fps
    t0 = (np.arange(int(z["seq_windows"]), dtype=np.float32) * np.float32(1.0 / 30.0)).astype(np.float32)
    plan = dict(motion_id=np.full(len(t0), int(z["seq_clip"]), np.int32), t0=t0, t_future=t0)
    o = outputs(s.sample_with(s.plan_from_numpy(plan)))
    for k in MOTION_KEYS:
        assert np.array_equal(o[k], seq[NAMES[k]].cpu().numpy())
    mean, std = (t.cpu().numpy() for t in s.feature_stats())
    # The reference accumulates N = 366 fp32 terms per entry in fp32, this project in fp64: the reference's own rounding is at most
    # N eps / 2 = 2.2e-5 relative to the accumulated magnitude for the mean; the std adds the same on the squared deviations (halved by the
    # square root) plus the mean's error.  Bar: 1e-4 relative to max(|value|, 1e-2) for the std, to max(1, max |mean|) for the mean.
    # Measured on the MI355X: see DESIGN.md section 8f.
    em = np.abs(mean - z["mean"]).max() / max(1.0, np.abs(z["mean"]).max())
    es = (np.abs(std - z["std"]) / np.maximum(np.abs(z["std"]), 1e-2)).max()
    print(f"feature_stats: mean rel err {em:.3e}, std rel err {es:.3e}")
    assert em <= 1e-4 and es <= 1e-4
    assert mean.shape == (15, 120) and (mean[:, 105:] == 0).all() and (std[:, 105:] == 1).all() and (std >= np.float32(1e-5)).all()


def test_terrain_at_the_bitset_limit_matches_restatement(tmp_path):
    """A 512 x 512-cell terrain (the limit: 32 KB of window bits in LDS beside the planes) against the CPU restatement, with the
    analysis of the file done on load.  RELATIVE_TO_ROOT_FLOOR: every heightfield operation is exact, so cells are bit-equal outside
    the ones fp32 rounding may move (computed as the fixture generator records them; at most 1 %)."""
    import motion_sampler_ref as ref
    from parc_amd import motion_sampler as ms
    from parc_amd import ms_file
    from parc_amd.char_model import CharModel
    z = fixture("floor_boxes")
    f = ms_file.load_ms_file(os.path.join(REPO, "data/motion_terrains/civilization.pkl"), load_misc=False)
    rng = np.random.RandomState(8)
    hf = (rng.randint(-5, 6, (64, 64)).astype(np.float32) * np.float32(0.2)).repeat(8, 0).repeat(8, 1)     # 3.2 m plateaus
    f.terrain_data.hf = np.ascontiguousarray(hf)
    f.terrain_data.hf_maxmin = np.zeros((512, 512, 2), np.float32)
    f.terrain_data.min_point = np.array([-90.0, -95.0], np.float32)
    path = str(tmp_path / "big_terrain.pkl")
    ms_file.save_ms_file(f, path)
    s = ms.MotionWindowSampler(z["cfg"], path, CHAR, "cuda:0")
    assert s.clips[0].terrain.hf.shape == (512, 512)
    plan = s.draw_plan(96, 21)
    o = outputs(s.sample_with(plan, return_bounds=True, validate=True))
    m = f.motion_data
    clip = dict(name="big_terrain", root_pos=np.asarray(m.root_pos, np.float32), root_rot=np.asarray(m.root_rot, np.float32),
                joint_rot=np.asarray(m.joint_rot, np.float32), contacts=np.asarray(m.body_contacts, np.float32), fps=int(m.fps), loop_mode=0,
                hf=hf, min_point=f.terrain_data.min_point, dx=float(f.terrain_data.dx))
    p = {k: v.cpu().numpy() for k, v in plan.items()}
    r = ref.sample_with(ref.Library([clip], s.extra_vals), CharModel(CHAR), s.cfg, p)
    skip = ref.rounding_cells(s.cfg, p, r["patch_cell_coords"])
    print("cells fp32 rounding may move:", int(skip.sum()), "of", skip.size)
    assert skip.mean() <= 0.01
    assert np.array_equal(o["hfs"][~skip], r["hfs"][~skip]) and np.array_equal(o["hf_bounds"][~skip], r["hf_bounds"][~skip])
    spread = o["hf_bounds"][..., 0] - o["hf_bounds"][..., 1]                   # 4 max_h = 12 where the window does not touch the cell
    touched = np.abs(spread - 12.0) > 1e-3
    assert touched.any(axis=(1, 2)).all() and not touched.all()                 # every window found its masked cells through the bitset
    for k in MOTION_KEYS + ("target_pos", "target_rot"):
        close(o[k], r[k], TOL, f"big terrain {k} vs restatement")


def test_error_paths(tmp_path_factory, tmp_path):
    import torch
    from parc_amd import lib as L
    from parc_amd import motion_sampler as ms
    z = fixture("root_boxes")
    s = sampler_for("root_boxes", tmp_path_factory)
    # a clip too short for a window is refused by name
    y = write_motion_yaml(tmp_path, ["sfu", "civilization"], [1.0, 1.0])
    with pytest.raises(ValueError, match="sfu"):
        ms.MotionWindowSampler(z["cfg"], y, CHAR, "cuda:0")
    # ... and by the library itself (clip index), as is a terrain above the bitset limit
    from parc_amd.motion_opt import OptClip, pack_clips
    from parc_amd.motion_terrain import clip_struct
    import ctypes as C

    def set_clips(nf, X, Y, num_clips=1, null=None, **packed):
        """One clip of nf frames on an X x Y terrain; `packed` replaces arrays of the packing, `null` names a field passed as NULL."""
        B = s.B
        q = np.tile(np.array([0, 0, 0, 1], np.float32), (nf, 1))
        oc = [OptClip(np.zeros((nf, 3), np.float32), q, np.tile(q[:, None], (1, B - 1, 1)), np.zeros((nf, B), np.float32),
                      np.zeros((X, Y), np.float32), np.zeros(2, np.float32), 0.4)]
        pk = dict(pack_clips(oc, B, s.char_model.get_dof_size()), **packed)
        st = clip_struct(pk, num_clips)
        info = L.ParcMotionSamplerClipInfo()
        mm, off = np.zeros((X * Y, 2), np.float32), np.zeros(nf + 1, np.int64)
        fps, loop, w = np.array([30], np.int32), np.array([0], np.int32), np.array([1.0])
        info.hf_maxmin_host, info.mask_off_host, info.mask_cells_host = L.np_f32p(mm), off.ctypes.data_as(L.i64p), None
        info.fps_host, info.loop_modes_host, info.weights_host = L.np_i32p(fps), L.np_i32p(loop), w.ctypes.data_as(L.f64p)
        if null is not None:
            setattr(info if hasattr(info, null) else st, null, None)
        other = ms.MotionWindowSampler.__new__(ms.MotionWindowSampler)
        other.__dict__.update(s.__dict__)
        other._h = None
        other._create()
        try:
            L.check(other._lib.parc_msamp_set_clips(other._h, C.byref(st), C.byref(info)))
        finally:
            other._lib.parc_msamp_destroy(other._h)
            other._h = None

    with pytest.raises(L.ParcError, match="clip 0 is too short: 15 frames"):
        set_clips(15, 4, 4)
    with pytest.raises(L.ParcError, match="262656 cells, above the limit of 262144"):
        set_clips(16, 513, 512)
    set_clips(16, 512, 512)
    # one fault per call: the return code and the whole message (the strings of parc_msamp_set_clips and parc_msamp_create)
    from gpu_helpers import SHARED_CLIP_ARRAYS

    def refused(msg, *a, **k):
        with pytest.raises(L.ParcError) as e:
            set_clips(*a, **k)
        assert str(e.value) == "libparc_env error -1: " + msg

    T = s.cfg.T
    assert T == 15
    i64 = lambda *v: np.array(v, np.int64)  # noqa: E731
    refused("msamp: num_clips must be >= 1", 16, 4, 4, num_clips=0)
    for name in SHARED_CLIP_ARRAYS + ("hf_maxmin_host", "mask_off_host", "fps_host", "loop_modes_host", "weights_host"):
        refused("msamp: null clip array", 16, 4, 4, null=name)
    refused("msamp: offsets must start at 0", 16, 4, 4, frame_off=i64(1, 17))
    refused("msamp: offsets must start at 0", 16, 4, 4, hf_off=i64(1, 17))
    refused("msamp: clip 0 is too short: 15 frames for windows of 15", 15, 4, 4)
    refused("msamp: clip 0 is too short: 0 frames for windows of 15", 16, 4, 4, frame_off=i64(0, 0))
    refused("msamp: heightfield dims / offsets disagree", 16, 4, 4, hf_dims=np.ascontiguousarray([[5, 4]], np.int32))
    refused("msamp: dx must be > 0", 16, 4, 4, hf_geom=np.ascontiguousarray([[0, 0, 0, 0.4]], np.float32))
    refused("msamp: the terrain of clip 0 has 262656 cells, above the limit of 262144 (the window mask is a bitset in LDS)", 16, 513, 512)
    p = L.ParcMotionSamplerParams()
    p.struct_size = C.sizeof(L.ParcMotionSamplerParams) - 8
    h = C.c_void_p()
    with pytest.raises(L.ParcError) as e:
        L.check(s._lib.parc_msamp_create(C.byref(p), C.byref(h)))
    assert str(e.value) == "libparc_env error -1: ParcMotionSamplerParams ABI mismatch (struct_size)" and not h.value
    # num_boxes above max_num_boxes, a motion id outside the library
    p = plan_of(z)
    bad = dict(p, num_boxes=np.full_like(p["num_boxes"], s.cfg.max_num_boxes + 1))
    with pytest.raises(L.ParcError, match="num_boxes"):
        s.sample_with(s.plan_from_numpy(bad), validate=True)
    with pytest.raises(L.ParcError, match="motion_id"):
        s.sample_with(s.plan_from_numpy(dict(p, motion_id=np.full_like(p["motion_id"], 2))), validate=True)
    s.sample_with(s.plan_from_numpy(p), validate=True)                                # the status is cleared by the check
    # plan arrays of the wrong length
    plan = s.plan_from_numpy(p)
    plan["t0"] = plan["t0"][:-1].contiguous()
    with pytest.raises(ValueError, match="t0"):
        s.sample_with(plan)
    with pytest.raises(ValueError, match="boxes"):
        s.plan_from_numpy(dict(p, boxes=p["boxes"][:, :2]))
    plan = s.plan_from_numpy(p)
    plan["pool_size"] = plan["pool_size"].to(torch.int64)
    with pytest.raises(ValueError, match="pool_size"):
        s.sample_with(plan)


def test_nan_frame_poisons_only_its_clip(tmp_path_factory, tmp_path):
    import shutil
    from parc_amd import motion_sampler as ms
    from parc_amd import ms_file
    z = fixture("root_boxes")
    clips = [str(c) for c in z["clips"]]
    s = sampler_for("root_boxes", tmp_path_factory)
    d = tmp_path / "lib"
    d.mkdir()
    for c in clips:
        shutil.copy(os.path.join(REPO, "data/motion_terrains", c + ".pkl"), d / (c + ".pkl"))
    f = ms_file.load_ms_file(str(d / (clips[1] + ".pkl")))
    f.motion_data.root_pos = np.array(f.motion_data.root_pos, np.float32)
    f.motion_data.root_pos[40, 2] = np.nan
    ms_file.save_ms_file(f, str(d / (clips[1] + ".pkl")))
    import yaml
    y = str(tmp_path / "motions.yaml")
    with open(y, "w") as fh:
        yaml.safe_dump({"motions": [{"file": str(d / (c + ".pkl")), "weight": 1.0} for c in clips]}, fh)
    bad = ms.MotionWindowSampler(z["cfg"], y, CHAR, "cuda:0", extra_vals=extra_vals(clips))
    plan = s.draw_plan(2048, 4)
    a, b = outputs(s.sample_with(plan)), outputs(bad.sample_with(plan))
    mid = plan["motion_id"].cpu().numpy()
    assert bits_equal({k: v[mid == 0] for k, v in a.items()}, {k: v[mid == 0] for k, v in b.items()})
    touched = ~np.isfinite(b["root_pos"]).all(axis=(1, 2)) | ~np.isfinite(b["target_pos"]).all(axis=1)
    assert touched.any() and (mid[touched] == 1).all()
    clean = (mid == 1) & ~touched & np.isfinite(b["hfs"]).all(axis=(1, 2))
    same = [i for i in np.flatnonzero(clean) if np.array_equal(a["root_pos"][i], b["root_pos"][i])]
    assert len(same) > 0                                                              # windows of that clip away from the frame are unchanged


def test_export_script_end_to_end(tmp_path):
    import subprocess
    import yaml
    out = tmp_path / "batches"
    r = subprocess.run([sys.executable, os.path.join(REPO, "scripts/export_generator_batches.py"), "--num_batches", "2", "--batch_size", "8",
                        "--out", str(out)], capture_output=True, text=True, cwd=REPO, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "refused: sfu" in r.stdout and "(4 clips)" in r.stdout
    b = np.load(out / "batch_000001.npz")
    assert b["features"].shape == (8, 15, 120) and b["hfs"].shape == (8, 31, 31) and np.isfinite(b["features"]).all()
    st = yaml.safe_load(open(out / "feature_stats.yaml"))
    assert np.asarray(st["mean"]).shape == (15, 120) and np.asarray(st["std"]).shape == (15, 120)


# ---- the handle across set_clips calls: what a library leaves behind must not reach the next one -----------------------------------
def _reload_library(tmp_path):
    """(sampler holding nothing of its own yet, A, B, their extra values).  A: the TEASER_TERRAIN clip (58 frames, 102 x 102 cells).
    B: its first T + 4 frames (a clip needs more than T) on a cropped terrain that still holds every cell those frames mask."""
    import copy
    from parc_amd import motion_sampler as ms
    z = fixture("root_boxes")
    y = write_motion_yaml(tmp_path, ["TEASER_TERRAIN"], [1.0])
    eA = extra_vals(["TEASER_TERRAIN"])[0]
    s = ms.MotionWindowSampler(z["cfg"], y, CHAR, "cuda:0", extra_vals=[eA])
    A = s.clips[0]
    n, X, Y = s.cfg.T + 4, 80, 60
    ter = copy.copy(A.terrain)
    ter.hf = np.ascontiguousarray(np.asarray(A.terrain.hf, np.float32)[:X, :Y])
    B = copy.copy(A)
    B.name, B.terrain, B.weight = "TEASER_TERRAIN_head", ter, 2.0
    B.root_pos, B.root_rot, B.joint_rot, B.contacts = A.root_pos[:n].copy(), A.root_rot[:n].copy(), A.joint_rot[:n].copy(), A.contacts[:n].copy()
    eB = dict(hf_mask_inds=eA["hf_mask_inds"][:n], hf_maxmin=np.ascontiguousarray(eA["hf_maxmin"][:X, :Y]))
    assert all(a[:, 0].max() < X and a[:, 1].max() < Y for a in eB["hf_mask_inds"] if len(a))
    return s, (A, eA), (B, eB)


def _load(s, *clips):
    """parc_msamp_set_clips on the handle s holds, through the wrapper's own upload."""
    s.clips, s.extra_vals = [c for c, _ in clips], [e for _, e in clips]
    s._upload()


def _plan4(s, motion_id):
    """4 windows of an injected plan: start times inside B's 4 window starts, one height change, one box."""
    t0 = (np.arange(4, dtype=np.float32) * np.float32(1.0 / 30.0)).astype(np.float32)
    mb = s.cfg.max_num_boxes
    boxes = np.zeros((4, mb, 6), np.float32)
    boxes[2, 0] = [12.0, 14.0, 4.0, 6.0, 0.7, 0.5]
    return s.plan_from_numpy(dict(motion_id=np.array(motion_id, np.int32), t0=t0, t_future=t0 + np.float32(0.1),
                                  future_pos_noise=np.full((4, 3), 0.01, np.float32), change_height=np.array([0, 1, 0, 0], np.int32),
                                  height_value=np.array([0, 0.4, 0, 0], np.float32), num_boxes=np.array([0, 0, 1, 0], np.int32), boxes=boxes))


def test_a_reload_equals_a_fresh_handle(tmp_path):
    s, A, B = _reload_library(tmp_path)
    _load(s, A, B)
    outputs(s.sample_with(_plan4(s, [0, 1, 1, 0]), return_bounds=True, validate=True))
    _load(s, B)
    got = outputs(s.sample_with(_plan4(s, [0, 0, 0, 0]), return_bounds=True, validate=True))
    fresh, _, _ = _reload_library(tmp_path)
    _load(fresh, B)
    want = outputs(fresh.sample_with(_plan4(fresh, [0, 0, 0, 0]), return_bounds=True, validate=True))
    assert got["hfs"].shape == (4, s.cfg.Gx, s.cfg.Gy) and bits_equal(got, want)
    assert all(np.isfinite(v).all() for v in got.values()) and not np.array_equal(got["hfs"][0], got["hfs"][2])


def test_a_rejected_library_leaves_the_previous_one_usable(tmp_path):
    import copy
    from parc_amd import lib as L
    s, A, _ = _reload_library(tmp_path)
    _load(s, A)
    plan = _plan4(s, [0, 0, 0, 0])
    before = outputs(s.sample_with(plan, return_bounds=True, validate=True))
    ter = copy.copy(A[0].terrain)
    ter.dx = 0.0
    broken = copy.copy(A[0])
    broken.terrain = ter
    with pytest.raises(L.ParcError) as e:
        _load(s, (broken, A[1]))
    assert str(e.value) == "libparc_env error -1: msamp: dx must be > 0"
    after = outputs(s.sample_with(plan, return_bounds=True, validate=True))
    assert bits_equal(before, after)
