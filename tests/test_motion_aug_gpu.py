"""Motion-terrain augmenter on the GPU: the kernels against the reference fixture and against the numpy
restatement, the fused path against draw + augment_with, the device draws, properties of drawn variations, the validate pass, and the
way into the optimiser and the scripts.  Reads only ``tests/golden/`` and the bundled data."""
import dataclasses
import importlib.util
import os

import numpy as np
import pytest

import motion_aug_ref as ref
from parc_amd import motion_aug as ma
from parc_amd import motion_opt as mo
from parc_amd.char_model import CharModel

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHAR_FILE = os.path.join(REPO, "data/assets/humanoid.xml")
DEV = "cuda:0"
F = np.float32


@pytest.fixture(scope="module")
def fixture():
    return ref.load_fixture(os.path.join(REPO, "tests/golden/motion_aug.npz"))


@pytest.fixture(scope="module")
def model():
    return ref.model_tables(CharModel(CHAR_FILE))


def opt_clip(src, name, fps=30):
    return mo.OptClip(src["root_pos"], src["root_rot"], src["joint_rot"], src["contacts"], src["hf"], src["min_point"], float(src["dx"]), fps, name,
                      hf_maxmin=src["hf_maxmin"])


def settings_for(mode, base, **kw):
    keys = {f.name for f in dataclasses.fields(ma.MotionAugSettings)}
    return ma.MotionAugSettings(**{**{k: (tuple(v) if isinstance(v, list) else v) for k, v in base.items() if k in keys}, "terrain_aug_type": mode, **kw})


def augmenter(sources, mode, base, **kw):
    return ma.MotionAugmenter(CHAR_FILE, [opt_clip(s, f"src{k}") for k, s in enumerate(sources)], settings_for(mode, base, **kw), DEV)


def within(count, n, p):
    """Binomial bound at 5 sigma, from n and p (tests/test_terrain_gen_gpu.py's helper)."""
    return abs(count - n * p) <= 5.0 * np.sqrt(n * p * (1.0 - p))


def uniform_ok(u, bins=8):
    u = np.asarray(u, np.float64).ravel()
    counts = np.histogram(u, bins=bins, range=(0.0, 1.0))[0]
    return all(within(c, u.size, 1.0 / bins) for c in counts)


def check_against_restatement(aug, sources, plan_np, model, what):
    """augment_with(plan) against ``ref.augment_one`` of every variation, under the fixture's rules; returns the masked-cell count."""
    s = aug.settings
    got = aug.augment_with(aug.plan_from_numpy(plan_np), validate=True).variations()
    masked = 0
    for v, g in enumerate(got):
        want = ref.augment_one(sources[int(plan_np["src_clip"][v])], ref.plan_var(plan_np, v), aug.mode, s.terrain_padding_size, s.slice_terrain, model)
        masked += ref.compare_variation(g, want, f"{what} variation {v}")
        assert abs(float(g["canon_z"]) - float(want["canon_z"])) <= 1e-5
    return masked


# ---- 1. the fixture ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", range(6))
def test_augment_with_matches_reference(fixture, g):
    sources, groups, settings, _ = fixture
    grp = groups[g]
    aug = augmenter(sources, grp["mode"], settings)
    res = aug.augment_with(aug.plan_from_numpy(grp["plan"]), validate=True)
    got = res.variations()
    assert aug.status() == 0 and len(got) == len(grp["want"])
    assert np.array_equal(res.numpy()["src_clip"], grp["plan"]["src_clip"])
    assert np.array_equal(np.diff(res.numpy()["frame_off"]), grp["plan"]["num_frames"])
    for v, (a, want) in enumerate(zip(got, grp["want"])):
        masked = ref.compare_variation(a, want, f"group {g} variation {v}")
        print(f"group {g} variation {v}: {tuple(a['hf_dims'])} cells, {int(want['unstable'].sum())} masked, {masked} of them differ")
        assert abs(float(a["canon_z"]) - float(want["canon_z"])) <= 1e-5
        if not grp["mirror"]:
            assert np.array_equal(a["joint_rot"], want["joint_rot"])       # the window's joints, bit for bit


# ---- 2. fresh plans at the smallest shapes that can go wrong ------------------------------------------------------------------------------
def random_plan(rng, sources, n, mode, mirror=None):
    src = rng.randint(0, len(sources), n).astype(np.int32)
    nfc = np.array([sources[c]["root_pos"].shape[0] for c in src])
    start = (rng.random_sample(n) * nfc).astype(np.int32)
    nf = (1 + rng.random_sample(n) * (nfc - start)).astype(np.int32).clip(1, nfc - start)
    nb = rng.randint(0, ref.MAX_BOXES + 1, n).astype(np.int32) if mode == "BOXES_ALONG_PATH" else np.zeros(n, np.int32)
    boxes = np.stack([rng.uniform(0.5, 6, (n, ref.MAX_BOXES)), rng.uniform(0.5, 6, (n, ref.MAX_BOXES)), rng.uniform(0, 6.28, (n, ref.MAX_BOXES)),
                      rng.uniform(-1, 1, (n, ref.MAX_BOXES))], -1).astype(F)
    return dict(src_clip=src, start_frame=start, num_frames=nf, heading=rng.uniform(-np.pi, np.pi, n).astype(F),
                scale=rng.uniform(0.8, 1.2, (n, 2)).astype(F), mirror=(rng.randint(0, 2, n) if mirror is None else np.full(n, mirror)).astype(np.int32),
                height_scale=rng.uniform(0.5, 1.5, n).astype(F), num_boxes=nb,
                box_frame=(rng.random_sample((n, ref.MAX_BOXES)) * nf[:, None]).astype(np.int32), boxes=boxes)


def straight_clip(span, n=2):
    """A clip walking ``span`` metres along x (and 3.6 m along y) over a 4 x 4 terrain."""
    pos = np.zeros((n, 3), F); pos[:, 0] = np.linspace(0.0, span, n); pos[:, 1] = np.linspace(0.3, 3.9, n); pos[:, 2] = 0.9
    q = np.zeros((n, 4), F); q[:, 3] = 1
    jq = np.zeros((n, 14, 4), F); jq[..., 3] = 1
    hf = np.arange(16, dtype=F).reshape(4, 4) * F(0.1)
    return dict(root_pos=pos, root_rot=q, joint_rot=jq, contacts=np.zeros((n, 15), F), hf=hf, hf_maxmin=np.stack([hf + 1, hf - 1], -1).astype(F),
                min_point=np.array([-0.3, -0.5], F), dx=F(0.4))


def one_variation(nf, **kw):
    p = dict(src_clip=np.zeros(1, np.int32), start_frame=np.zeros(1, np.int32), num_frames=np.full(1, nf, np.int32), heading=np.zeros(1, F),
             scale=np.ones((1, 2), F), mirror=np.zeros(1, np.int32), height_scale=np.ones(1, F), num_boxes=np.zeros(1, np.int32),
             box_frame=np.zeros((1, ref.MAX_BOXES), np.int32), boxes=np.zeros((1, ref.MAX_BOXES, 4), F))
    p.update(kw)
    return p


@pytest.mark.parametrize("mode", ref.MODES)
def test_fresh_plans_match_restatement(fixture, model, mode):
    """70 variations (more than one wave per launch, a ragged tail) of every source: 1-frame windows, the 6-frame clip on 5 x 7, and in
    BOXES_ALONG_PATH PARC_MAUG_MAX_BOXES boxes with one of zero size."""
    sources, _, settings, _ = fixture
    rng = np.random.RandomState(7)
    plan = random_plan(rng, sources, 70, mode)
    plan["num_frames"][:4] = 1                                       # 1-frame windows
    plan["src_clip"][4], plan["start_frame"][4], plan["num_frames"][4] = 2, 0, 6   # the whole 6-frame clip on 5 x 7
    plan["box_frame"][4] = np.minimum(plan["box_frame"][4], 5)
    plan["box_frame"][:4] = 0
    if mode == "BOXES_ALONG_PATH":
        plan["num_boxes"][4:8] = ref.MAX_BOXES
        plan["boxes"][4:8, 3, :2] = 0.0                              # a box of zero size: never hit
    aug = augmenter(sources, mode, settings)
    masked = check_against_restatement(aug, sources, plan, model, mode)
    print(f"{mode}: {masked} masked cells differ")


def test_motion_wholly_outside_its_terrain(fixture, model):
    sources, _, settings, _ = fixture
    far = dict(sources[2], root_pos=(sources[2]["root_pos"] + np.array([40.0, -25.0, 0.0], F)).astype(F))
    for mode in ("HEIGHT_SCALE", "NONE"):
        aug = augmenter([far], mode, settings)
        plan = one_variation(6, height_scale=np.full(1, 1.3, F), mirror=np.ones(1, np.int32))
        check_against_restatement(aug, [far], plan, model, "outside " + mode)
        got = aug.augment_with(aug.plan_from_numpy(plan)).variations()[0]
        assert (got["hf"] == 0).all()                                # the pad ring reads 0.0
        assert (got["hf_maxmin"][..., 0] == far["hf_maxmin"][..., 0].max()).all() and (got["hf_maxmin"][..., 1] == far["hf_maxmin"][..., 1].min()).all()


def test_slice_at_and_past_the_dim_limit(model):
    """A slice exactly PARC_MAUG_MAX_DIM wide runs (as one workgroup: more than 1024 cells); one cell wider is refused, naming the macro."""
    base = dict(terrain_padding_size=2)
    spans = {}
    for span in np.arange(48.0, 52.0, 0.05):
        c = straight_clip(F(span))
        X = int(ref.augment_one(c, ref.plan_var(one_variation(2), 0), "NONE", 2, True, model)["hf_dims"][0])
        spans.setdefault(X, c)
    assert ref.MAX_DIM in spans and ref.MAX_DIM + 1 in spans
    fits, wide = spans[ref.MAX_DIM], spans[ref.MAX_DIM + 1]
    aug = augmenter([fits, wide], "NONE", base)
    got = aug.augment_with(aug.plan_from_numpy(one_variation(2))).variations()[0]
    assert got["hf_dims"][0] == ref.MAX_DIM and got["hf"].size > 1024
    check_against_restatement(aug, [fits, wide], one_variation(2, mirror=np.ones(1, np.int32)), model, "MAX_DIM")
    with pytest.raises(RuntimeError, match="PARC_MAUG_MAX_DIM"):
        aug.augment_with(aug.plan_from_numpy(one_variation(2, src_clip=np.ones(1, np.int32))))
    check_against_restatement(aug, [fits, wide], one_variation(2), model, "after a refusal")   # the handle stays usable


# ---- 3. the fused path, batch invariance, seeds -------------------------------------------------------------------------------------------
DRAW = dict(max_motion_len=0.5, sample_weight_by_length=True)        # windows of 15 frames: shorter than the two 40-frame sources


def same_results(a, b, va=None, vb=None):
    """Bit equality of two results, or of variations ``va`` of ``a`` and ``vb`` of ``b`` (ranges)."""
    a, b = a.numpy(), b.numpy()
    if va is None:
        return all((a[k] is None and b[k] is None) or np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in a)
    for key, off in (("root_pos", "frame_off"), ("root_rot", "frame_off"), ("joint_rot", "frame_off"), ("contacts", "frame_off"), ("hf", "cell_off"),
                     ("hf_maxmin", "cell_off")):
        x = a[key][a[off][va.start]:a[off][va.stop]]
        y = b[key][b[off][vb.start]:b[off][vb.stop]]
        if x.shape != y.shape or not np.array_equal(x.view(np.uint8), y.view(np.uint8)):
            return False
    return all(np.array_equal(a[k][va].view(np.uint8), b[k][vb].view(np.uint8)) for k in ("src_clip", "hf_dims", "hf_geom", "canon_z"))


@pytest.mark.parametrize("mode", ref.MODES)
def test_augment_equals_draw_then_augment_with(fixture, mode):
    sources, _, settings, _ = fixture
    aug = augmenter(sources, mode, settings, **DRAW)
    n, seed = 4096, 11
    fused = aug.augment(n, seed)
    plan = aug.draw_plan(n, seed)
    assert same_results(fused, aug.augment_with(plan, validate=True))
    assert aug.status() == 0
    part = aug.augment(64, seed, first=1000)                         # variation v depends on (seed, first + v) only
    assert same_results(fused, part, range(1000, 1064), range(0, 64))
    mirrored = aug.augment(64, seed, first=1000, mirror=True)
    assert np.array_equal(mirrored.numpy()["hf_dims"], part.numpy()["hf_dims"]) and not same_results(mirrored, part)
    other = {k: v.cpu().numpy() for k, v in aug.draw_plan(n, seed + 1).items()}
    mine = {k: v.cpu().numpy() for k, v in plan.items()}
    assert (other["heading"] != mine["heading"]).all() and (other["scale"] != mine["scale"]).any(axis=1).all()   # another seed changes every variation


# ---- 4. the device draws ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("by_length", [True, False])
def test_device_draws(fixture, by_length):
    sources, _, settings, _ = fixture
    n = 16384
    hs = augmenter(sources, "HEIGHT_SCALE", settings, max_motion_len=0.5, sample_weight_by_length=by_length)
    p = {k: v.cpu().numpy() for k, v in hs.draw_plan(n, 5).items()}
    s = hs.settings
    frames = np.array([c["root_pos"].shape[0] for c in sources])
    w = frames / 30.0 if by_length else np.ones(len(sources))
    assert np.allclose(hs.weights, w / w.sum())
    for c in range(len(sources)):
        assert within((p["src_clip"] == c).sum(), n, hs.weights[c]), c
    win = hs.max_frames[p["src_clip"]]
    assert (win == 15).all()
    nfc = frames[p["src_clip"]]
    longer = nfc > win
    assert (p["num_frames"] == np.minimum(nfc, win)).all() and (p["start_frame"][~longer] == 0).all()
    assert (p["start_frame"] >= 0).all() and (p["start_frame"][longer] <= (nfc - win - 1)[longer]).all()
    for c in np.flatnonzero(frames > 15):                            # uniform on [0, n - max_frames - 1]
        st = p["start_frame"][p["src_clip"] == c]
        assert st.max() == frames[c] - 16 and all(within((st == k).sum(), st.size, 1.0 / (frames[c] - 15)) for k in range(frames[c] - 15))
    deg = p["heading"].astype(np.float64) * 180.0 / np.pi
    assert uniform_ok((deg - s.min_heading_angle) / (s.max_heading_angle - s.min_heading_angle))
    for k, (lo, hi) in enumerate((s.x_scale, s.y_scale)):
        assert uniform_ok((p["scale"][:, k].astype(np.float64) - lo) / (hi - lo))
    h, (b0, b1) = p["height_scale"], (F(s.bad_h_range[0]), F(s.bad_h_range[1]))
    assert not ((h > b0) & (h < b1)).any() and h.min() >= F(s.min_h_scale) and h.max() <= F(s.max_h_scale)
    a, b = s.bad_h_range[0] - s.min_h_scale, s.max_h_scale - s.bad_h_range[1]
    t = np.where(h <= b0, h.astype(np.float64) - s.min_h_scale, a + h.astype(np.float64) - s.bad_h_range[1])   # the allowed set, laid end to end
    assert uniform_ok(np.clip(t / (a + b), 0.0, 1.0 - 1e-12)) and within((h <= b0).sum(), n, a / (a + b))
    assert (p["mirror"] == 0).all() and (p["num_boxes"] == 0).all()
    bx = augmenter(sources, "BOXES_ALONG_PATH", settings, max_motion_len=0.5, sample_weight_by_length=by_length)
    q = {k: v.cpu().numpy() for k, v in bx.draw_plan(n, 5, mirror=True).items()}
    assert (q["mirror"] == 1).all() and np.array_equal(q["src_clip"], p["src_clip"]) and np.array_equal(q["heading"], p["heading"])
    nb = q["num_boxes"]
    assert nb.min() == s.min_num_boxes and nb.max() == s.max_num_boxes
    for k in range(s.min_num_boxes, s.max_num_boxes + 1):
        assert within((nb == k).sum(), n, 1.0 / (s.max_num_boxes - s.min_num_boxes + 1))
    live = np.arange(ref.MAX_BOXES)[None, :] < nb[:, None]
    assert (q["box_frame"] >= 0).all() and (q["box_frame"] < q["num_frames"][:, None]).all()   # box frames within the window
    full = q["box_frame"][live & (q["num_frames"] == 15)[:, None]]
    assert all(within((full == k).sum(), full.size, 1.0 / 15) for k in range(15))
    assert (q["boxes"][~live] == 0).all()
    for k, (lo, hi) in enumerate(((s.min_len, s.max_len), (s.min_len, s.max_len), (s.min_angle, s.max_angle), (s.min_h, s.max_h))):
        assert uniform_ok((q["boxes"][..., k][live].astype(np.float64) - lo) / (hi - lo))


# ---- 5. properties of drawn variations ------------------------------------------------------------------------------------------------------
def test_properties_of_drawn_variations(fixture):
    sources, _, settings, _ = fixture
    n = 4096
    bx = augmenter(sources, "BOXES_ALONG_PATH", settings, **DRAW)
    plain = augmenter(sources, "NONE", settings, **DRAW)
    plan = bx.draw_plan(n, 3)
    a, b = bx.augment_with(plan).numpy(), plain.augment_with(plan).numpy()
    assert np.array_equal(a["hf_dims"], b["hf_dims"]) and np.array_equal(a["root_pos"], b["root_pos"])
    first = a["frame_off"][:-1]
    assert (a["root_pos"][first, :2] == 0).all()                      # frame 0 at xy = 0
    g, dims = b["hf_geom"], b["hf_dims"]
    i0 = np.clip(np.rint((F(0) - g[:, 0]) / g[:, 2]), 0, dims[:, 0] - 1).astype(np.int64)
    j0 = np.clip(np.rint((F(0) - g[:, 1]) / g[:, 3]), 0, dims[:, 1] - 1).astype(np.int64)
    assert (b["hf"][b["cell_off"][:-1] + i0 * dims[:, 1] + j0] == 0).all()   # the terrain under frame 0 reads 0 before the edit
    boxes, nb = plan["boxes"].cpu().numpy(), plan["num_boxes"].cpu().numpy()
    changed = a["hf"] != b["hf"]
    assert changed.any()
    var_of_cell = np.repeat(np.arange(n), np.diff(a["cell_off"]))
    for c in np.flatnonzero(changed):                                # every cell is its pre-edit value or one of its boxes' heights
        v = var_of_cell[c]
        assert a["hf"][c] in boxes[v, :nb[v], 3]


# ---- 6. the validate pass -------------------------------------------------------------------------------------------------------------------
def test_validate_and_bad_entries(fixture):
    sources, _, settings, _ = fixture
    aug = augmenter(sources, "BOXES_ALONG_PATH", settings)
    clean = random_plan(np.random.RandomState(9), sources, 12, "BOXES_ALONG_PATH")
    clean["num_boxes"][:] = np.maximum(clean["num_boxes"], 1)
    want = aug.augment_with(aug.plan_from_numpy(clean), validate=True)
    assert aug.status() == 0
    cases = [("heading", lambda p: p["heading"].__setitem__(3, np.nan), "heading"), ("src_clip", lambda p: p["src_clip"].__setitem__(5, 99), "src_clip"),
             ("start_frame", lambda p: p["start_frame"].__setitem__(2, -1), "start_frame"),
             ("num_frames", lambda p: p["num_frames"].__setitem__(7, 1000), "num_frames"),
             ("scale", lambda p: p["scale"].__setitem__((1, 1), np.inf), "scale"),
             ("num_boxes", lambda p: p["num_boxes"].__setitem__(4, ref.MAX_BOXES + 1), "num_boxes"),
             ("box_frame", lambda p: p["box_frame"].__setitem__((6, 0), 10000), "box_frame"),
             ("boxes", lambda p: p["boxes"].__setitem__((8, 0, 2), np.nan), "boxes"),
             ("mirror", lambda p: p["mirror"].__setitem__(0, 7), "mirror")]
    for name, spoil, field in cases:
        bad = {k: v.copy() for k, v in clean.items()}
        spoil(bad)
        with pytest.raises(RuntimeError, match=rf"bad plan: .*{field}"):
            aug.augment_with(aug.plan_from_numpy(bad), validate=True)
    # without the pass: memory-safe, and the other variations are the clean run's bits
    bad = {k: v.copy() for k, v in clean.items()}
    bad["heading"][3], bad["src_clip"][5], bad["box_frame"][6, 0], bad["num_frames"][7] = np.nan, 99, 10000, 1000
    got = aug.augment_with(aug.plan_from_numpy(bad))
    assert aug.status() == ma.STATUS_CLAMPED | ma.STATUS_NOT_FINITE
    assert tuple(got.numpy()["hf_dims"][3]) == (1, 1)
    for v in range(12):
        if v not in (3, 5, 6, 7):
            assert same_results(want, got, range(v, v + 1), range(v, v + 1)), v
    # an infinite scale is no slice either: 1 x 1, flagged, the rest untouched (its window has y of both signs or one: both give an infinite bound)
    bad = {k: v.copy() for k, v in clean.items()}
    bad["scale"][1, 1], bad["scale"][9, 0] = np.inf, -np.inf
    got = aug.augment_with(aug.plan_from_numpy(bad))
    assert aug.status() == ma.STATUS_NOT_FINITE
    assert tuple(got.numpy()["hf_dims"][1]) == (1, 1) and tuple(got.numpy()["hf_dims"][9]) == (1, 1)
    for v in range(12):
        if v not in (1, 9):
            assert same_results(want, got, range(v, v + 1), range(v, v + 1)), v
    hs = augmenter(sources, "HEIGHT_SCALE", settings)
    bad = {k: v.copy() for k, v in clean.items()}
    bad["height_scale"][2] = np.nan
    with pytest.raises(RuntimeError, match="bad plan: .*height_scale"):
        hs.augment_with(hs.plan_from_numpy(bad), validate=True)
    with pytest.raises(ValueError, match="heading"):
        hs.augment_with({k: v for k, v in hs.plan_from_numpy(clean).items() if k != "heading"})


# ---- 7. into the optimiser and the scripts --------------------------------------------------------------------------------------------------
def load_script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REPO, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def clips_equal(a, b):
    return all(np.array_equal(np.asarray(getattr(a, k), F), np.asarray(getattr(b, k), F)) for k in
               ("root_pos", "root_rot", "joint_rot", "contacts", "hf", "min_point", "hf_maxmin")) and F(a.dx) == F(b.dx) and a.fps == b.fps


def test_variations_feed_the_optimiser(fixture):
    sources, _, settings, _ = fixture
    aug = augmenter(sources, "HEIGHT_SCALE", settings)
    clips = aug.augment(4, 21).to_opt_clips()
    assert [c.name[-7:-3] for c in clips] == ["_aug"] * 4 and all(c.hf.shape == c.hf_maxmin.shape[:2] for c in clips)
    cfg = dict(w_root_pos=1.0, w_root_rot=10.0, w_joint_rot=1.0, w_smoothness=10.0, w_penetration=1000.0, w_contact=1000.0, w_sliding=10.0,
               w_body_constraints=0.0, w_jerk=1000.0, max_jerk=1000.0, step_size=1e-3)
    frames, hist = mo.MotionOptimizer(CHAR_FILE, DEV, cfg).optimize(clips, 2)
    assert len(frames) == 4
    for fr, c, h in zip(frames, clips, hist):
        assert fr["root_pos"].shape == c.root_pos.shape and np.isfinite(fr["root_pos"]).all()
        assert all(np.isfinite(v) for v in h[-1][1].values())


def test_augment_motions_script_and_save_flipped(tmp_path):
    cfg = ma.load_config(os.path.join(REPO, "data/configs/motion_aug/motion_aug_default.yaml"))
    cfg.update(num_new_motions=8, output_folder_path=str(tmp_path / "aug"), device=DEV, terrain_aug_type="BOXES_ALONG_PATH")
    paths = load_script("augment_motions").run(cfg, no_opt=True, mirror=True, seed=4)
    assert len(paths) == 16 and all(os.path.exists(p) for p in paths)
    from parc_amd.motion_lib import fetch_motion_files
    files, _ = fetch_motion_files(os.path.join(REPO, cfg["motions_yaml_path"]))
    aug = ma.MotionAugmenter(CHAR_FILE, [mo.clip_from_ms(f) for f in files], ma.MotionAugSettings.from_config(cfg), DEV)
    want = aug.augment(8, 4).to_opt_clips()
    for p, w in zip(paths[:8], want):
        assert os.path.basename(p) == w.name + ".pkl" and "_aug" in w.name
        assert clips_equal(mo.clip_from_ms(p), w)
    for p, w in zip(paths[8:], aug.mirror_clips(want)):
        assert p.endswith(os.path.join("flipped", w.name + ".pkl")) and w.name.endswith("_flipped")
        assert clips_equal(mo.clip_from_ms(p), w)
    # run_optimize_motions --save_flipped: the file equals mirror_clips of the optimised clip
    ocfg = ma.load_config(os.path.join(REPO, "data/configs/motion_opt/motion_opt_default.yaml"))
    ocfg.update(num_iters=2, output_folder_path=str(tmp_path / "opt"), device=DEV, auto_compute_body_constraints=False, save_flipped=True,
                frame_stride=1, log_every=100, hf_extras=False)
    out = load_script("run_optimize_motions").run(ocfg)
    assert len(out) == 2 and out[1].endswith(os.path.join("flipped", "dec2024_teaser_717_1_modified_opt_opt_flipped.pkl"))
    opt = mo.clip_from_ms(out[0])
    flipped = ma.mirror_clips([opt], CHAR_FILE, DEV)[0]
    assert clips_equal(mo.clip_from_ms(out[1]), flipped)
    assert np.array_equal(flipped.root_pos[:, 1], -opt.root_pos[:, 1]) and np.array_equal(flipped.hf, opt.hf[:, ::-1])
    back = ma.mirror_clips([flipped], CHAR_FILE, DEV)[0]                 # mirror of mirror: positions bit for bit, rotations up to sign
    assert np.array_equal(back.root_pos, opt.root_pos) and np.array_equal(back.hf, opt.hf) and np.array_equal(back.contacts, opt.contacts)
    assert ref.quat_close(back.root_rot, opt.root_rot).max() <= ref.QUAT_TOL and ref.quat_close(back.joint_rot, opt.joint_rot).max() <= ref.QUAT_TOL
