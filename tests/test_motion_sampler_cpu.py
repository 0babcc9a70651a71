"""Host side of the motion-window sampler (no GPU): the torch restatement against the reference fixtures, config parsing, the CSR
packing of ``hf_mask_inds``, the plan struct layout, the short-clip refusal, the feature column order and the export file layout."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch
import yaml

from parc_amd import motion_sampler as ms
from parc_amd.char_model import CharModel

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, ".."))
sys.path.insert(0, HERE)
import helpers  # noqa: E402
import motion_sampler_ref as ref  # noqa: E402

CHAR = os.path.join(REPO, "data/assets/humanoid.xml")
CASES = ["root_boxes", "floor_boxes", "noise", "none"]
# off the 31 x 31, 15-frame CLAMP configuration (make_golden_motion_sampler.py shapes): 7 x 32 at 20 fps with T = 20, ref frame 4, 7 boxes;
# 32 x 5 in floor mode; 9 x 11 NOISE; the first two on WRAP copies of the clips with windows and targets across the clip's end
SHAPE_CASES = ["rect_root", "rect_floor", "rect_noise", "wrap_root", "wrap_floor"]
TOL = 1e-5   # the bar of tests/test_device_ops_gpu.py for calc_motion_frame / FK against the reference goldens


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


def library(clip_names, loop_modes=None):
    return ref.Library(helpers.load_clips(clip_names, loop_modes), extra_vals(clip_names))


def plan_of(z):
    return {k[5:]: z[k] for k in z if k.startswith("plan_")}


def close(a, b, tol, what=""):
    """tests/test_device_ops_gpu.py's bar: absolute error against tol + 2 ulp of the value."""
    err = np.abs(a - b) / (1.0 + (2.4e-7 / tol) * np.abs(b))
    assert np.all(np.isfinite(err)) and err.max() <= tol, f"{what}: max err {err.max()} at {np.unravel_index(err.argmax(), err.shape)}"
    return float(np.abs(a - b).max())


@pytest.fixture(scope="module")
def cm():
    return CharModel(CHAR)


@pytest.mark.parametrize("case", CASES + SHAPE_CASES)
def test_restatement_matches_reference(cm, case):
    z = fixture(case)
    cfg = ms.parse_config(z["cfg"])
    o = ref.sample_with(library([str(c) for c in z["clips"]], z.get("loop_modes")), cm, cfg, plan_of(z))
    for k in ("root_pos", "root_rot", "joint_pos", "joint_rot", "contacts", "target_pos", "target_rot"):
        print(case, k, close(o[k], z[k], TOL, k))
    keep = ~z["skip"]
    assert z["skip"].mean() <= 0.01
    if cfg.relative_z_style == 1:   # gather, a difference of two gathered values, max, clamp, select: exact
        assert np.array_equal(o["hfs"][keep], z["hfs"][keep])
        assert np.array_equal(o["floor_heights"], z["floor_heights"])
    else:                            # the only inexact input is the reference root z; max-pool, clamp, select are 1-Lipschitz
        close(o["hfs"][keep], z["hfs"][keep], TOL, "hfs")
    sub = z["hf_raw"][:, cfg.num_x_neg, cfg.num_y_neg] if cfg.relative_z_style == 1 else None
    if sub is not None:
        assert np.array_equal(o["hf_bounds"][keep], (z["bounds_raw"] - sub[:, None, None, None])[keep])


def test_restatement_plan_builder_draws_boxes_over_the_patch(cm):
    """The builder scales box centres by (Gx, Gy), not by a square, so that the GPU edge plans put boxes over the whole long side."""
    cfg = ms.parse_config(fixture("rect_root")["cfg"])
    bx = ref.RefSampler(library([str(c) for c in fixture("rect_root")["clips"]]), cm, cfg).draw_plan(512, 3)["boxes"]
    assert (cfg.Gx, cfg.Gy) == (7, 32) and bx.shape == (512, 7, 6)
    assert bx[..., 0].min() >= 0 and bx[..., 0].max() <= 7 and bx[..., 0].max() > 6.5
    assert bx[..., 1].min() >= 0 and bx[..., 1].max() <= 32 and bx[..., 1].max() > 31 and (bx[..., 1] > 7).mean() > 0.7


def test_restatement_sequences_and_stats(cm):
    z = dict(np.load(os.path.join(REPO, "tests/golden/motion_sampler_stats.npz")))
    cfg = ms.parse_config(fixture("root_boxes")["cfg"])
    lib = library([str(c) for c in z["clips"]])
    o = ref.motion_sequences_for_id(lib, cm, cfg, int(z["seq_clip"]))
    assert o["root_pos"].shape[0] == int(z["seq_windows"])
    for k in ("root_pos", "root_rot", "joint_pos", "joint_rot", "contacts"):
        close(o[k][z["seq_starts"]], z["seq_" + k], TOL, k)
    mean, std = ref.feature_stats(lib, cm, cfg)
    # the reference accumulates 366 fp32 values per entry in fp32: relative error <= N eps / 2 of the accumulated magnitude (2.2e-5);
    # the std adds the cancellation of the squared deviations; bar 1e-4 relative to max(|value|, 1e-2)
    assert np.abs(mean - z["mean"]).max() <= 1e-4 * max(1.0, np.abs(z["mean"]).max())
    assert (np.abs(std - z["std"]) <= 1e-4 * np.maximum(np.abs(z["std"]), 1e-2)).all()


def test_config_parsing():
    cfg = yaml.safe_load(open(os.path.join(REPO, "data/configs/motion_sampler/motion_sampler_default.yaml")))
    c = ms.parse_config(cfg)
    assert (c.T, c.ref_frame, c.Gx, c.Gy) == (15, 1, 31, 31)
    assert c.times.dtype == np.float32 and c.times[0] == 0 and abs(c.times[-1] - 14 / 30) < 1e-6
    assert c.grid_x.shape == (31,) and abs(c.grid_x[10]) < 1e-6 and abs(c.grid_x[0] + 2.0) < 1e-6 and abs(c.grid_y[-1] - 3.0) < 1e-6
    assert c.aug_mode == ms.AUG_MODE["MAXPOOL_AND_BOXES"] and c.relative_z_style == 0 and c.max_num_boxes == 4
    assert (c.hf_maxpool_chance, c.hf_max_maxpool_size, c.hf_change_height_chance) == (0.15, 10, 0.1)
    off = dict(cfg, use_hf_augmentation=False)
    assert ms.parse_config(off).aug_mode == ms.AUG_MODE["NONE"]
    with pytest.raises(ValueError):
        ms.parse_config(dict(cfg, features=dict(frame_components=["JOINT_VEL"])))
    with pytest.raises(ValueError):
        ms.parse_config(dict(cfg, sequence_duration=3.0))   # 90 frames > 64
    with pytest.raises(KeyError):
        ms.parse_config(dict(cfg, relative_z_style="ABSOLUTE"))


def test_mask_inds_csr_round_trip():
    ev = extra_vals(["civilization", "dec2024_teaser_717_1_modified_opt"])
    dims = [(50, 50), (18, 15)]
    off, cells = ms.pack_mask_inds([e["hf_mask_inds"] for e in ev], dims)
    nf = [len(e["hf_mask_inds"]) for e in ev]
    assert off.dtype == np.int64 and cells.dtype == np.int32 and off.shape[0] == sum(nf) + 1 and off[-1] == cells.shape[0]
    back = ms.unpack_mask_inds(off, cells, np.concatenate([[0], np.cumsum(nf)]), dims)
    for e, b in zip(ev, back):
        assert len(b) == len(e["hf_mask_inds"]) and all(np.array_equal(x, y) for x, y in zip(e["hf_mask_inds"], b))
    with pytest.raises(ValueError):
        ms.pack_mask_inds([[np.array([[18, 0]])]], [(18, 15)])


def test_plan_struct_layout():
    from parc_amd import lib as L
    assert [f[0] for f in L.ParcMotionSamplerPlan._fields_] == ["n"] + [f[0] for f in ms.PLAN_FIELDS]
    assert [f[0] for f in L.MSAMP_PLAN_FIELDS] == [f[0] for f in ms.PLAN_FIELDS]
    assert C.sizeof(L.ParcMotionSamplerPlan) == 8 + 8 * len(ms.PLAN_FIELDS)          # int32 n, padding, 11 pointers
    assert L.ParcMotionSamplerPlan.motion_id.offset == 8 and L.ParcMotionSamplerPlan.noise.offset == 8 * len(ms.PLAN_FIELDS)
    assert C.sizeof(L.ParcMotionSamplerOutputs) == 8 * 10
    assert C.sizeof(L.ParcMotionSamplerClipInfo) == 8 * 6
    assert (L.MSAMP_MAX_FRAMES, L.MSAMP_MAX_GRID, L.MSAMP_MAX_TERRAIN_CELLS, L.MSAMP_MAX_BOXES, L.MSAMP_BOX_FLOATS) == \
        (ms.MAX_FRAMES, ms.MAX_GRID, ms.MAX_TERRAIN_CELLS, ms.MAX_BOXES, ms.BOX_FLOATS)
    hdr = open(os.path.join(REPO, "include/parc_env.h")).read()
    for name, v in [("MAX_FRAMES", "64"), ("MAX_GRID", "32"), ("MAX_TERRAIN_CELLS", "(512 * 512)"), ("MAX_BOXES", "64"), ("BOX_FLOATS", "6")]:
        assert f"#define PARC_MSAMP_{name} {v}" in hdr
    assert "#define PARC_ABI_VERSION 6" in hdr.replace("  ", " ") or L.ABI_VERSION == 6
    cfg = ms.parse_config(fixture("noise")["cfg"])
    sh = ms.plan_shapes(5, cfg)
    assert sh["boxes"] == (5, 4, 6) and sh["noise"] == (5, 31, 31) and sh["pool_kind"] == (5, 3) and sh["t0"] == (5,)
    plan = {n: torch.zeros(sh[n], dtype=dt) for n, dt, _ in ms.PLAN_FIELDS}
    assert ms.check_plan(plan, cfg) == 5
    plan["num_boxes"] = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError, match="num_boxes"):
        ms.check_plan(plan, cfg)


def test_short_clip_is_refused_by_name():
    clips = helpers.load_clips(["sfu", "civilization"])
    with pytest.raises(ValueError, match=r"sfu \(15 frames\)"):
        ms.check_clip_lengths([c["name"] for c in clips], [c["root_pos"].shape[0] for c in clips], 15)
    ms.check_clip_lengths(["civilization"], [254], 15)
    sys.path.insert(0, os.path.join(REPO, "scripts"))
    import export_generator_batches as ex
    keep, refused = ex.usable_clips(os.path.join(REPO, "data/motion_terrains/motions_bundled.yaml"), 15)
    assert refused == ["sfu"] and len(keep) == 4


def test_assemble_features_column_order():
    n, T, B = 2, 3, 15
    motion = dict(ROOT_POS=torch.full((n, T, 3), 1.0), ROOT_ROT=torch.full((n, T, 4), 2.0), JOINT_POS=torch.full((n, T, B - 1, 3), 3.0),
                  JOINT_ROT=torch.full((n, T, B - 1, 4), 4.0), CONTACTS=torch.full((n, T, B), 5.0))
    motion["JOINT_POS"][:, :, 1, 2] = 3.5
    comps = ["ROOT_POS", "ROOT_ROT", "JOINT_POS", "JOINT_ROT", "CONTACTS"]
    f = ms.assemble_features(motion, comps)
    assert f.shape == (n, T, 120)
    sl = ms.feature_slices(comps, B)
    assert [(sl[k].start, sl[k].stop) for k in comps] == [(0, 3), (3, 7), (7, 49), (49, 105), (105, 120)]
    for k, v in zip(comps, (1.0, 2.0, 3.0, 4.0, 5.0)):
        assert (f[..., sl[k]] == v).sum() >= f[..., sl[k]].numel() - n * T
    assert (f[..., 7 + 1 * 3 + 2] == 3.5).all()          # joint 1, z: row-major over (joint, xyz)
    g = ms.assemble_features(motion, ["CONTACTS", "ROOT_POS"])
    assert g.shape == (n, T, 18) and (g[..., :15] == 5.0).all()


def test_export_file_layout(cm, tmp_path):
    z = fixture("floor_boxes")
    cfg = ms.parse_config(z["cfg"])
    s = ref.RefSampler(library([str(c) for c in z["clips"]]), cm, cfg)
    files = ms.export_batches(s, 2, 3, str(tmp_path / "out"), seed=5)
    assert [os.path.basename(f) for f in files] == ["batch_000000.npz", "batch_000001.npz"]
    b = np.load(files[1])
    assert set(b.files) == {"root_pos", "root_rot", "joint_pos", "joint_rot", "contacts", "floor_heights", "features", "hfs", "target_pos",
                            "target_rot"}
    assert b["features"].shape == (3, 15, 121) and b["hfs"].shape == (3, 31, 31) and b["target_rot"].shape == (3, 4)
    assert np.array_equal(b["features"][..., :3], b["root_pos"]) and np.array_equal(b["features"][..., 120:], b["floor_heights"])
    st = yaml.safe_load(open(tmp_path / "out" / "feature_stats.yaml"))
    assert sorted(st) == ["mean", "std"] and np.asarray(st["mean"]).shape == (15, 120) and np.asarray(st["std"]).shape == (15, 120)
    assert (np.asarray(st["mean"])[:, 105:] == 0).all() and (np.asarray(st["std"])[:, 105:] == 1).all() and (np.asarray(st["std"]) >= float(np.float32(1e-5))).all()
