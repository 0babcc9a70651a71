"""The motion-window sampler kernels (parc_msamp_*) away from the one configuration the sibling file runs (a
31 x 31 patch, T = 15, ref frame 1, 30 fps, 4 boxes, CLAMP clips): rectangular patches, a window at 20 fps over 30 fps clips, WRAP clips
with windows and targets across the clip's end, and the limits of T, the patch sides, the box count and the pool widths.

Bars (the sibling file's, none new): motion outputs and targets ``close(..., TOL = 1e-5)``; ``hfs``, ``floor_heights`` and ``hf_bounds``
bit for bit in ``RELATIVE_TO_ROOT_FLOOR`` outside the cells fp32 rounding may move (recorded by the fixture generator, or
``motion_sampler_ref.rounding_cells`` for fresh plans; at most 1 % of a case's cells, asserted); ``close`` on ``hfs`` in
``RELATIVE_TO_ROOT``; bit equality between runs of the same plan; 5-sigma binomial bounds from n and p on the draws.

Times on the MI355X (pytest --durations, call phase): the 23 tests take 4.3 s together; the longest are the 32 x 32 pool-width edge
(0.50 s, the restatement's pools on the CPU), ``rect_root`` (0.29 s, the first sampler) and T = 64 (0.13 s); every other test is under 0.13 s."""
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import helpers  # noqa: E402
import motion_sampler_ref as ref  # noqa: E402
from test_motion_sampler_gpu import (CHAR, MOTION_KEYS, NAMES, REPO, TOL, bits_equal, close, extra_vals, fixture, outputs, plan_of,  # noqa: E402
                                     within)

pytestmark = pytest.mark.gpu

CLIPS = ["civilization", "dec2024_teaser_717_1_modified_opt"]     # 254 and 142 frames at 30 fps
SHAPE_CASES = ["rect_root", "rect_floor", "rect_noise", "wrap_root", "wrap_floor"]
TARGETS = ("target_pos", "target_rot")
EDGE = 1e-4                                                      # the generator's margin around a rounding boundary, in cells


# ---- libraries, samplers and restatement outputs, built once -----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def char_model():
    from parc_amd.char_model import CharModel
    return CharModel(CHAR)


@functools.lru_cache(maxsize=None)
def ref_library(loops=(0, 0)):
    return ref.Library(helpers.load_clips(CLIPS, loops), extra_vals(CLIPS))


def library_yaml(tmp_dir, loops):
    """The two clips as a library file; a clip with ``loops[i] = 1`` is a copy whose ``loop_mode`` alone is changed to WRAP."""
    import yaml
    from parc_amd import ms_file
    files = []
    for c, wrap in zip(CLIPS, loops):
        p = os.path.join(REPO, "data/motion_terrains", c + ".pkl")
        if wrap:
            d = ms_file.load_ms_file(p, load_misc=False)
            d.motion_data.loop_mode = "WRAP"
            p = os.path.join(str(tmp_dir), c + "_wrap.pkl")
            ms_file.save_ms_file(d, p)
        files.append(p)
    y = os.path.join(str(tmp_dir), "motions.yaml")
    with open(y, "w") as f:
        yaml.safe_dump({"motions": [{"file": p, "weight": 1.0} for p in files]}, f)
    return y


_SAMPLERS = {}


def make_sampler(cfg, loops, tmp_path_factory):
    """``extra_vals`` is passed in, so no analysis runs."""
    from parc_amd import motion_sampler as ms
    s = ms.MotionWindowSampler(cfg, library_yaml(tmp_path_factory.mktemp("msamp_shapes"), loops), CHAR, "cuda:0", extra_vals=extra_vals(CLIPS))
    assert list(s.loop_modes) == list(loops)
    return s


def sampler_for(case, tmp_path_factory):
    """The sampler of a fixture's configuration and loop modes (the fps warning of the 20 fps cases is checked where they are built
    on purpose, in test_reference_cases)."""
    import warnings
    if case not in _SAMPLERS:
        z = fixture(case)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)
            _SAMPLERS[case] = make_sampler(z["cfg"], tuple(int(v) for v in z["loop_modes"]), tmp_path_factory)
    return _SAMPLERS[case]


@functools.lru_cache(maxsize=None)
def restated(case):
    from parc_amd import motion_sampler as ms
    z = fixture(case)
    return ref.sample_with(ref_library(tuple(int(v) for v in z["loop_modes"])), char_model(), ms.parse_config(z["cfg"]), plan_of(z))


def floor_lookup_unstable(cfg, r, skip):
    """Bool [n, T]: the floor-height lookups fp32 rounding may move, by the generator's scheme: the canonical root's patch cell
    coordinate within EDGE cells of a half-integer, or the cell it reads is itself one of ``skip``."""
    u = (r["root_pos"][..., 0:2].astype(np.float64) - cfg.grid_min.astype(np.float64)) / cfg.dx
    near = (np.abs(u - np.floor(u) - 0.5) < EDGE).any(-1)
    i = np.clip(np.rint(u[..., 0]).astype(np.int64), 0, cfg.Gx - 1)
    j = np.clip(np.rint(u[..., 1]).astype(np.int64), 0, cfg.Gy - 1)
    return near | skip[np.arange(skip.shape[0])[:, None], i, j]


def check_against_restatement(o, r, cfg, plan, what):
    """The sibling file's rules with the restatement as the reference; the skipped cells are ``ref.rounding_cells``."""
    n = len(plan["motion_id"])
    assert o["hfs"].shape == (n, cfg.Gx, cfg.Gy) and o["hf_bounds"].shape == (n, cfg.Gx, cfg.Gy, 2) and o["root_pos"].shape == (n, cfg.T, 3)
    for k in MOTION_KEYS + TARGETS:
        close(o[k], r[k], TOL, f"{what} {k} vs restatement")
    skip = ref.rounding_cells(cfg, plan, r["patch_cell_coords"])
    print(f"{what}: cells fp32 rounding may move: {int(skip.sum())} of {skip.size}")
    assert skip.mean() <= 0.01
    keep = ~skip
    if cfg.relative_z_style == 1:
        assert np.array_equal(o["hfs"][keep], r["hfs"][keep]), what
        assert np.array_equal(o["hf_bounds"][keep], r["hf_bounds"][keep]), what
        if "floor_heights" in r:
            assert o["floor_heights"].shape == (n, cfg.T)
            loose = floor_lookup_unstable(cfg, r, skip)
            print(f"{what}: floor-height lookups fp32 rounding may move: {int(loose.sum())} of {loose.size}")
            assert loose.mean() <= 0.01
            assert np.array_equal(o["floor_heights"][~loose], r["floor_heights"][~loose]), what
    else:
        close(o["hfs"][keep], r["hfs"][keep], TOL, f"{what} hfs vs restatement")
        close(o["hf_bounds"][keep], r["hf_bounds"][keep], TOL, f"{what} hf_bounds vs restatement")
    return skip


# ---- the reference cases ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SHAPE_CASES)
def test_reference_cases(case, tmp_path_factory):
    """``sample_with`` on each fixture's plan against the fixture and the restatement, by the rules of
    test_sample_with_matches_reference_and_restatement.  Measured on the MI355X: DESIGN.md section 8f."""
    z = fixture(case)
    loops = tuple(int(v) for v in z["loop_modes"])
    if z["cfg"]["sequence_fps"] != 30:      # the window's mask frames are then not the window's frames: the wrapper says so, per clip
        with pytest.warns(UserWarning, match="differs from sequence_fps 20"):
            s = _SAMPLERS[case] = make_sampler(z["cfg"], loops, tmp_path_factory)
    else:
        s = sampler_for(case, tmp_path_factory)
    c = s.cfg
    o = outputs(s.sample_with(s.plan_from_numpy(plan_of(z)), return_bounds=True, validate=True))
    r = restated(case)
    assert o["hfs"].shape == (12, c.Gx, c.Gy) == z["hfs"].shape and o["hf_bounds"].shape == (12, c.Gx, c.Gy, 2)
    assert o["root_pos"].shape == (12, c.T, 3) == z["root_pos"].shape and o["joint_rot"].shape == z["joint_rot"].shape
    for k in MOTION_KEYS + TARGETS:
        close(o[k], z[k], TOL, f"{case} {k} vs reference")
        close(o[k], r[k], TOL, f"{case} {k} vs restatement")
    keep = ~z["skip"]
    print(f"{case}: skipped share {z['skip'].mean():.5f}")
    assert z["skip"].mean() <= 0.01
    if c.relative_z_style == 1:
        assert np.array_equal(o["hfs"][keep], z["hfs"][keep])
        assert np.array_equal(o["floor_heights"], z["floor_heights"])
        sub = z["hf_raw"][:, c.num_x_neg, c.num_y_neg]
        assert np.array_equal(o["hf_bounds"][keep], (z["bounds_raw"] - sub[:, None, None, None])[keep])
    else:
        close(o["hfs"][keep], z["hfs"][keep], TOL, f"{case} hfs vs reference")
        close(o["hfs"][keep], r["hfs"][keep], TOL, f"{case} hfs vs restatement")
    if loops[0]:                             # what the WRAP fixtures are for is in them (the generator asserts the same)
        length = s.lengths[z["plan_motion_id"]]
        assert (z["plan_t0"] + c.times[-1] > length).any() and (z["plan_t_future"] > length).any()


# ---- edges against the restatement -------------------------------------------------------------------------------------------------------
def grid(xn, xp, yn, yp):
    return dict(horizontal_scale=0.2, max_h=3.0, local_grid=dict(num_x_neg=xn, num_x_pos=xp, num_y_neg=yn, num_y_pos=yp))


def all_boxes(plan, cfg, lib, rng):
    plan["num_boxes"][:] = cfg.max_num_boxes


def pool_widths(plan, cfg, lib, rng):
    """All three pools on in every sample, the half widths 0, 31, 32 and 40 in every slot: on a side of 32 cells a half width of 31
    already spans the axis, so 32 (= the kernel's clamp) and 40 (above it) must give the same maximum as the restatement's unclamped pool."""
    n = len(plan["motion_id"])
    plan["pool_kind"][:] = np.stack([rng.permutation(3) + 1 for _ in range(n)])
    plan["pool_size"][:] = np.array([0, 31, 32, 40], np.int32)[(np.arange(n)[:, None] + np.arange(3)[None, :]) % 4]
    plan["change_height"][:] = 0           # a constant patch would make every pool a no-op


def wrap_windows(plan, cfg, lib, rng):
    """The restatement's builder draws every start time as for a CLAMP clip; the WRAP clip's samples get start times over [0, length),
    two of them one and three frames before the clip's end, and targets up to 1.5 s later."""
    wrap = np.flatnonzero(lib.loop.numpy()[plan["motion_id"]] == 1)
    assert len(wrap) >= 4
    length = lib.lengths.numpy()[plan["motion_id"]]
    plan["t0"][wrap] = (rng.rand(len(wrap)).astype(np.float32) * length[wrap]).astype(np.float32)
    plan["t0"][wrap[0]], plan["t0"][wrap[1]] = length[wrap[0]] - np.float32(1.0 / 30.0), length[wrap[1]] - np.float32(3.0 / 30.0)
    rem = np.minimum(length - plan["t0"], np.float32(cfg.future_window_max - cfg.future_window_min))
    plan["t_future"][:] = (rng.rand(len(length)).astype(np.float32) * rem + plan["t0"] + np.float32(cfg.future_window_min)).astype(np.float32)


#        name             overrides of the rect_floor configuration (32 x 5, T = 15, ref frame 1, 4 boxes, floor mode)      loops   plan
EDGES = [("T64", dict(sequence_duration=64.0 / 30.0), (0, 0), None),             # every FK lane, 46 KB of LDS, 960 items over 64 lanes
         ("T1", dict(sequence_duration=1.0 / 30.0, num_prev_states=1), (0, 0), None),
         ("ref_last", dict(num_prev_states=15), (0, 0), None),
         ("1x32", dict(heightmap=grid(0, 0, 20, 11)), (0, 0), None),
         ("32x1", dict(heightmap=grid(20, 11, 0, 0)), (0, 0), None),
         ("32x32", dict(heightmap=grid(20, 11, 11, 20)), (0, 0), None),
         ("boxes0", dict(max_num_boxes=0), (0, 0), None),
         ("boxes64", dict(max_num_boxes=64), (0, 0), all_boxes),
         ("pool_widths", dict(heightmap=grid(20, 11, 11, 20), hf_max_maxpool_size=40), (0, 0), pool_widths),
         ("mixed_loops", dict(), (0, 1), wrap_windows),                           # `loop` is read per sample
         ("mixed_loops_root", dict(relative_z_style="RELATIVE_TO_ROOT", heightmap=grid(2, 4, 20, 11)), (1, 0), wrap_windows)]
EDGE_SHAPES = {"T64": (64, 1, 32, 5), "T1": (1, 0, 32, 5), "ref_last": (15, 14, 32, 5), "1x32": (15, 1, 1, 32), "32x1": (15, 1, 32, 1),
               "32x32": (15, 1, 32, 32), "pool_widths": (15, 1, 32, 32), "mixed_loops_root": (15, 1, 7, 32)}
N_EDGE = 24


def edge_case(name):
    """(raw config, parsed config, restatement library, plan) of an edge: a fresh plan from the restatement's builder, fixed seed."""
    from parc_amd import motion_sampler as ms
    _, over, loops, tweak = next(e for e in EDGES if e[0] == name)
    raw = dict(fixture("rect_floor")["cfg"], **over)
    cfg = ms.parse_config(raw)
    lib = ref_library(loops)
    seed = 100 + [e[0] for e in EDGES].index(name)
    plan = ref.RefSampler(lib, char_model(), cfg).draw_plan(N_EDGE, seed)
    if tweak:
        tweak(plan, cfg, lib, np.random.RandomState(seed + 1000))
    return raw, cfg, lib, plan


@pytest.mark.parametrize("name", [e[0] for e in EDGES])
def test_edges_match_restatement(name, tmp_path_factory):
    raw, cfg, lib, plan = edge_case(name)
    if name in EDGE_SHAPES:
        assert (cfg.T, cfg.ref_frame, cfg.Gx, cfg.Gy) == EDGE_SHAPES[name]
    loops = next(e[2] for e in EDGES if e[0] == name)
    s = make_sampler(raw, loops, tmp_path_factory)
    o = outputs(s.sample_with(s.plan_from_numpy(plan), return_bounds=True, validate=True))
    r = ref.sample_with(lib, char_model(), cfg, plan)
    check_against_restatement(o, r, cfg, plan, name)
    if name == "boxes0":
        assert plan["boxes"].shape == (N_EDGE, 0, 6) and (plan["num_boxes"] == 0).all()
    if name == "boxes64":
        assert plan["boxes"].shape == (N_EDGE, 64, 6) and (plan["num_boxes"] == 64).all()
    if name == "pool_widths":                  # the case has something to pool: the patch is not constant, and the pools change it
        plain = ref.sample_with(lib, char_model(), cfg, dict(plan, pool_kind=np.zeros_like(plan["pool_kind"])))
        assert sorted(set(plan["pool_size"].ravel().tolist())) == [0, 31, 32, 40] and (plain["hfs"] != r["hfs"]).any(axis=(1, 2)).mean() > 0.5
    if name.startswith("mixed_loops"):
        wrap = lib.loop.numpy()[plan["motion_id"]] == 1
        length = lib.lengths.numpy()[plan["motion_id"]]
        assert wrap.any() and not wrap.all() and (plan["t0"] + cfg.times[-1] > length)[wrap].any() and (plan["t_future"] > length)[wrap].any()
        # the WRAP offset is there: the same plan on an all-CLAMP library gives other windows for the WRAP samples, the same for the rest
        clamp = ref.sample_with(ref_library((0, 0)), char_model(), cfg, plan)
        moved = (clamp["root_pos"] != r["root_pos"]).any(axis=(1, 2))
        assert moved[wrap].any() and not moved[~wrap].any()


def test_draw_without_autoregression_starts_at_zero(tmp_path_factory):
    """``autoregressive: False``: the drawn start time is 0 for every sample (motion_sampler.py:39-53), and the batch is the
    restatement's for the drawn plan."""
    from parc_amd import motion_sampler as ms
    raw = dict(fixture("rect_floor")["cfg"], autoregressive=False)
    s = make_sampler(raw, (0, 1), tmp_path_factory)
    plan = s.draw_plan(96, 17)
    p = {k: v.cpu().numpy() for k, v in plan.items()}
    assert (p["t0"] == 0).all() and set(p["motion_id"].tolist()) == {0, 1}
    assert (p["t_future"] >= np.float32(s.cfg.future_window_min)).all() and (p["t_future"] <= np.float32(s.cfg.future_window_max)).all()
    o = outputs(s.sample_with(plan, return_bounds=True, validate=True))
    r = ref.sample_with(ref_library((0, 1)), char_model(), ms.parse_config(raw), p)
    check_against_restatement(o, r, s.cfg, p, "not autoregressive")


# ---- batch invariance ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["rect_root", "wrap_floor"])
def test_batch_invariance(case, tmp_path_factory):
    """Every fixture sample gives the same bits alone, in its batch, and in a shuffled batch of 1 000 copies and mixtures."""
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


# ---- draws off the square ------------------------------------------------------------------------------------------------------------------
def uniform_in_bins(x, lo, hi, bins=8):
    """x is uniform on [lo, hi): every one of ``bins`` equal bins holds its binomial share at 5 sigma."""
    x = np.asarray(x).ravel()
    if not ((x >= lo).all() and (x <= hi).all()):
        return False
    idx = np.minimum(((x - lo) / (hi - lo) * bins).astype(np.int64), bins - 1)
    return all(within((idx == b).sum(), x.size, 1.0 / bins) for b in range(bins))


def test_box_draws_follow_each_side(tmp_path_factory):
    """On a 7 x 32 patch box centres are uniform on [0, Gx] and [0, Gy] separately (a swap of the sides fails both), the other box
    values are as on the square, and ``num_boxes`` is uniform on 0 .. 7."""
    s = sampler_for("rect_root", tmp_path_factory)
    c = s.cfg
    assert (c.Gx, c.Gy, c.max_num_boxes) == (7, 32, 7)
    n = 65536
    plan = {k: v.cpu().numpy() for k, v in s.draw_plan(n, 2025).items()}
    bx = plan["boxes"]
    assert bx.shape == (n, 7, 6)
    assert uniform_in_bins(bx[..., 0], 0.0, float(c.Gx)) and uniform_in_bins(bx[..., 1], 0.0, float(c.Gy))
    for b in (0, 6):                                             # the first and the last Philox block of the boxes
        assert uniform_in_bins(bx[:, b, 0], 0.0, float(c.Gx)) and uniform_in_bins(bx[:, b, 1], 0.0, float(c.Gy))
    assert uniform_in_bins(bx[..., 2], c.box_min_len, c.box_max_len) and uniform_in_bins(bx[..., 3], c.box_min_len, c.box_max_len)
    assert uniform_in_bins(bx[..., 4], 0.0, 2 * np.pi + 1e-6) and uniform_in_bins(bx[..., 5], -c.max_h, c.max_h)
    for v in range(8):
        assert within((plan["num_boxes"] == v).sum(), n, 1.0 / 8.0)
    assert plan["num_boxes"].min() == 0 and plan["num_boxes"].max() == 7
    # CLAMP clips at sequence_duration 1.0: every window fits, start times uniform on [0, length - 1]
    length = s.lengths[plan["motion_id"]]
    assert uniform_in_bins(plan["t0"] / (length - np.float32(1.0)), 0.0, 1.0)


def test_noise_field_off_the_square(tmp_path_factory):
    """The NOISE field of a 9 x 11 patch: [n, Gx, Gy], uniform on [-max_h, max_h], and the cells of the last, cut Philox block
    (99 = 4 x 24 + 3) are written like the rest."""
    s = sampler_for("rect_noise", tmp_path_factory)
    c = s.cfg
    assert (c.Gx, c.Gy) == (9, 11)
    n = 8192
    noise = s.draw_plan(n, 6)["noise"].cpu().numpy()
    assert noise.shape == (n, 9, 11) and np.isfinite(noise).all()
    assert uniform_in_bins(noise, -c.max_h, c.max_h)
    flat = noise.reshape(n, 99)
    for cell in (0, 95, 96, 97, 98):                              # the first cell, the last full block's last, the tail
        assert uniform_in_bins(flat[:, cell], -c.max_h, c.max_h), cell
    assert len(np.unique(flat[0])) > 95 and not np.array_equal(flat[0], flat[1])
    # a second draw into fresh memory gives the same field: no cell is left to what the allocation held
    assert np.array_equal(noise, s.draw_plan(n, 6)["noise"].cpu().numpy())


def test_wrap_library_draws_and_samples(tmp_path_factory):
    """On WRAP clips the start time is uniform on [0, length) (the ``u[1] * length`` branch), ``sample`` equals ``draw_plan`` +
    ``sample_with`` bit for bit, and the batch is the restatement's for the drawn plan."""
    s = sampler_for("wrap_floor", tmp_path_factory)
    c = s.cfg
    n = 65536
    plan = {k: v.cpu().numpy() for k, v in s.draw_plan(n, 31).items()}
    length = s.lengths[plan["motion_id"]]
    assert (plan["t0"] >= 0).all() and (plan["t0"] <= length).all()
    assert uniform_in_bins(plan["t0"] / length, 0.0, 1.0)
    for m in (0, 1):
        assert uniform_in_bins((plan["t0"] / length)[plan["motion_id"] == m], 0.0, 1.0)
    past = plan["t0"] + c.times[-1] > length                                         # windows across the end: (T - 1) / fps of the length
    assert within(past[plan["motion_id"] == 0].sum(), (plan["motion_id"] == 0).sum(), float(c.times[-1] / s.lengths[0]))
    rem = np.minimum(length - plan["t0"], np.float32(c.future_window_max - c.future_window_min))
    eps = 4 * np.finfo(np.float32).eps * (np.abs(plan["t0"]) + 2.0)
    lo = plan["t0"] + np.float32(c.future_window_min)
    assert (plan["t_future"] >= lo - eps).all() and (plan["t_future"] <= lo + rem + eps).all() and (plan["t_future"] > length).any()
    # sample = draw_plan + sample_with, and both are the restatement's batch for that plan
    m = 96
    a = outputs(s.sample(m, 31))
    drawn = s.draw_plan(m, 31)
    b = outputs(s.sample_with(drawn, return_bounds=True, validate=True))
    assert bits_equal(a, {k: b[k] for k in a})
    p = {k: v.cpu().numpy() for k, v in drawn.items()}
    assert all(np.array_equal(p[k], plan[k][:m]) for k in p)                         # a sample's draws depend on (seed, index) only
    r = ref.sample_with(ref_library((1, 1)), char_model(), c, p)
    check_against_restatement(b, r, c, p, "wrap draw")
    assert (p["t0"] + c.times[-1] > s.lengths[p["motion_id"]]).any()                 # the 96 do hold a window across the end


# ---- motion_sequences_for_id -----------------------------------------------------------------------------------------------------------------
def test_sequences_on_another_window(tmp_path_factory):
    """T = 20 at 20 fps, ref frame 4: the enumerated windows are ``sample_with`` at ``t0 = frame / fps`` bit for bit, and the restatement's."""
    s = sampler_for("rect_root", tmp_path_factory)
    c = s.cfg
    assert (c.T, c.ref_frame, c.sequence_fps) == (20, 4, 20)
    clip = 1
    seq = s.motion_sequences_for_id(clip)
    n = 142 - 20
    assert seq["ROOT_POS"].shape == (n, 20, 3) and seq["JOINT_ROT"].shape == (n, 20, 14, 4)
    t0 = (np.arange(n, dtype=np.float32) * np.float32(c.timestep)).astype(np.float32)
    o = outputs(s.sample_with(s.plan_from_numpy(dict(motion_id=np.full(n, clip, np.int32), t0=t0, t_future=t0))))
    r = ref.motion_sequences_for_id(ref_library(), char_model(), c, clip)
    for k in MOTION_KEYS:
        got = seq[NAMES[k]].cpu().numpy()
        assert np.array_equal(got.view(np.uint32), o[k].view(np.uint32)), k
        close(got, r[k], TOL, f"sequences {k} vs restatement")
