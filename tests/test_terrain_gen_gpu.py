"""The procedural terrain generator kernels (parc_tgen_*) against the reference fixtures and the CPU restatement.

The rule (tests/terrain_gen_ref.compare): outside the *unstable* mask (cells next to a decision) the GPU heightfield equals the
reference's bit for bit; STAIRS within 1e-6, because the reference forms step heights in double from double draws and the plan holds fp32.
Measured on the MI355X: no cell differs from the reference in any fixture (masked cells included) and none from the restatement in the
fresh-plan cases."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, ".."))
sys.path.insert(0, HERE)

import terrain_gen_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

FIXTURES = ["boxes", "paths", "stairs"]
DEV = "cuda:0"
DX = 0.4
_GENS = {}


def fixture(name):
    z = dict(np.load(os.path.join(REPO, "tests/golden", f"terrain_gen_{name}.npz")))
    z["groups"] = json.loads(str(z["groups"]))
    return z


def gen_for(mode, X, Y, settings):
    """One handle per (mode, shape, settings), shared by the tests."""
    from parc_amd import terrain_gen as tg
    key = (mode, X, Y, json.dumps(settings, sort_keys=True))
    if key not in _GENS:
        _GENS[key] = tg.TerrainGenerator(mode, X, Y, DX, settings=tg.SETTINGS[mode].from_config(settings), device=DEV)
    return _GENS[key]


def defaults(mode, **over):
    from parc_amd import terrain_gen as tg
    return dict(tg.SETTINGS[mode]().to_config(), **over)


def within(count, n, p):
    """Binomial bound at 5 sigma, from n and p (tests/test_motion_sampler_gpu.py's helper)."""
    return abs(count - n * p) <= 5.0 * np.sqrt(n * p * (1.0 - p))


def uniform_ok(u, bins=8):
    """Binned count test of values that should be uniform on [0, 1)."""
    u = np.asarray(u, np.float64).ravel()
    counts = np.histogram(u, bins=bins, range=(0.0, 1.0))[0]
    return all(within(c, u.size, 1.0 / bins) for c in counts)


@pytest.mark.parametrize("name", FIXTURES)
def test_generate_with_matches_reference(name):
    z = fixture(name)
    for g, m in enumerate(z["groups"]):
        G = gen_for(m["mode"], m["dim_x"], m["dim_y"], m["settings"])
        pre = f"g{g}_plan_"
        plan = G.plan_from_numpy({k[len(pre):]: z[k] for k in z if k.startswith(pre)})
        hf = G.generate_with(plan, validate=True).cpu().numpy()
        ref.compare(m["mode"], hf, z[f"g{g}_hf"], z[f"g{g}_unstable"], f"{name} group {g} (GPU against the reference)")


# fresh plans against the restatement: odd and non-square grids, the largest grid, the limits of the counts, both ends of the pool range
FRESH = [("BOXES", 5, 7, dict(num_boxes=1, box_min_len=1.0, box_max_len=4.0)), ("BOXES", 12, 20, dict(num_boxes=10)),
         ("BOXES", 64, 64, dict(num_boxes=64, box_max_len=30.0)),
         ("PATHS", 5, 7, dict(num_terrain_paths=1, maxpool_size=0)), ("PATHS", 12, 20, dict(num_terrain_paths=8, maxpool_size=1)),
         ("PATHS", 64, 64, dict(num_terrain_paths=64, maxpool_size=8)),
         ("STAIRS", 5, 7, dict(num_stairs=1)), ("STAIRS", 12, 20, dict(num_stairs=4)), ("STAIRS", 64, 64, dict(num_stairs=16))]


@pytest.mark.parametrize("mode,X,Y,over", FRESH, ids=[f"{m}-{x}x{y}" for m, x, y, _ in FRESH])
def test_fresh_plans_match_restatement(mode, X, Y, over):
    s = defaults(mode, **over)
    Q = 3
    plan = ref.random_plan(mode, Q, X, Y, DX, s, np.random.RandomState(X * 100 + Y))
    if mode == "STAIRS":   # a stair of a single step (shorter than dx), and one of zero length (no step at all)
        plan["stairs"][0, 0, 2:4] = plan["stairs"][0, 0, 0:2] + np.float32([0.17, -0.21])
        assert ref.stair_steps(plan["stairs"][0, 0], DX)[0] == 1
        if s["num_stairs"] > 1:
            plan["stairs"][1, 1, 2:4] = plan["stairs"][1, 1, 0:2]
    want, unstable = ref.generate(mode, plan, X, Y, DX, DX, (0.0, 0.0), s)
    G = gen_for(mode, X, Y, s)
    hf = G.generate_with(G.plan_from_numpy(plan)).cpu().numpy()
    ref.compare(mode, hf, want, unstable, f"{mode} {X} x {Y}")
    assert len(np.unique(want)) > 1   # the case paints something


@pytest.mark.parametrize("mode", ["BOXES", "PATHS", "STAIRS"])
def test_generate_equals_draw_then_generate_with(mode):
    import torch
    G = gen_for(mode, 12, 20, defaults(mode))
    for n, seed, first in ((70, 3, 0), (5, 2 ** 40 + 7, 123456789)):
        plan = G.draw_plan(n, seed, first)
        a, b = G.generate_with(plan), G.generate(n, seed, first)
        assert a.shape == (n, 12, 20) and torch.equal(a.view(torch.int32), b.view(torch.int32))
        plan2 = G.draw_plan(n, seed, first)
        assert all(torch.equal(plan[k].view(torch.int32), plan2[k].view(torch.int32)) for k in plan)


@pytest.mark.parametrize("mode", ["BOXES", "PATHS", "STAIRS"])
def test_batch_invariance_and_seeds(mode):
    """A terrain depends on (seed, first_terrain + position) only."""
    import torch
    G = gen_for(mode, 16, 16, defaults(mode))
    big = G.generate(4096, 17)
    part = G.generate(64, 17, first_terrain=1000)
    assert torch.equal(big[1000:1064].view(torch.int32), part.view(torch.int32))
    for t in (0, 1063, 4095):
        assert torch.equal(big[t].view(torch.int32), G.generate(1, 17, first_terrain=t)[0].view(torch.int32))
    plan_big, plan_part = G.draw_plan(4096, 17), G.draw_plan(64, 17, first_terrain=1000)
    assert all(torch.equal(plan_big[k][1000:1064], plan_part[k]) for k in plan_big)
    other = G.generate(64, 18, first_terrain=1000)
    assert (other != part).flatten(1).any(dim=1).all()                                 # every terrain differs under another seed
    assert len({big[t].cpu().numpy().tobytes() for t in range(256)}) == 256            # and terrains differ from one another


def test_device_draws_boxes_and_stairs():
    X, Y = 12, 20
    s = defaults("BOXES", num_boxes=10, min_box_angle=0.5, max_box_angle=2.5)
    bx = gen_for("BOXES", X, Y, s).draw_plan(4096, 5)["boxes"].cpu().numpy().astype(np.float64)
    eps = 1e-6
    ranges = [(0.0, X), (0.0, Y), (s["box_min_len"], s["box_max_len"]), (s["box_min_len"], s["box_max_len"]),
              (s["min_box_angle"], s["max_box_angle"]), (s["min_box_h"], s["max_box_h"])]
    for k, (lo, hi) in enumerate(ranges):
        v = bx[..., k]
        assert v.min() >= lo - eps and v.max() <= hi + eps, (k, v.min(), v.max())
        assert uniform_ok((v - lo) / (hi - lo)), k
    assert abs(np.corrcoef(bx[..., 0].ravel(), bx[..., 1].ravel())[0, 1]) <= 5.0 / np.sqrt(bx[..., 0].size)
    s = defaults("STAIRS")
    st = gen_for("STAIRS", X, Y, s).draw_plan(4096, 6)["stairs"].cpu().numpy().astype(np.float64)
    mx, my = np.float32(X - 1) * np.float32(DX), np.float32(Y - 1) * np.float32(DX)     # start / end lie in [min_point, get_max_point()]
    ranges = [(0.0, mx), (0.0, my), (0.0, mx), (0.0, my), (s["min_stair_start_height"], s["max_stair_start_height"]),
              (s["min_step_height"], s["max_step_height"]), (s["min_stair_thickness"], s["max_stair_thickness"])]
    for k, (lo, hi) in enumerate(ranges):
        v = st[..., k]
        assert v.min() >= lo - 1e-5 and v.max() <= hi + 1e-5, (k, v.min(), v.max())
        assert uniform_ok((v - lo) / (hi - lo)), k


def test_device_draws_paths():
    X, Y = 12, 20
    s = defaults("PATHS")
    plan = {k: v.cpu().numpy().astype(np.float64) for k, v in gen_for("PATHS", X, Y, s).draw_plan(1024, 9).items()}
    assert plan["path_turn"].shape == (1024, 4, 1000)
    sx, sy = plan["path_start"][..., 0], plan["path_start"][..., 1]
    wx, wy = float(np.float32(X) * np.float32(DX)), float(np.float32(Y) * np.float32(DX))   # dims * dxdy, not get_max_point()
    assert sx.min() >= 0 and sx.max() <= wx + 1e-6 and sy.min() >= 0 and sy.max() <= wy + 1e-6
    assert uniform_ok(sx / wx) and uniform_ok(sy / wy)
    a = plan["path_angle"]
    assert a.min() >= 0 and a.max() <= 2 * np.pi + 1e-6 and uniform_ok(a / (2 * np.pi))
    h = plan["path_height"]
    assert h.min() >= s["path_min_height"] - 1e-6 and h.max() <= s["path_max_height"] + 1e-6
    assert uniform_ok((h - s["path_min_height"]) / (s["path_max_height"] - s["path_min_height"]))
    for z in (plan["path_turn"], plan["path_vy"]):       # standard normals: mean, variance and the tail share within their sampling bounds
        n = z.size
        assert np.isfinite(z).all() and abs(z.mean()) <= 5.0 / np.sqrt(n) and abs(z.var() - 1.0) <= 5.0 * np.sqrt(2.0 / n)
        assert within((np.abs(z) > 2.0).sum(), n, 0.04550026389635842) and within((z < 0).sum(), n, 0.5)
    t = plan["path_turn"]
    assert abs(np.corrcoef(t[..., 0::4].ravel(), t[..., 1::4].ravel())[0, 1]) <= 5.0 / np.sqrt(t.size / 4)   # the cos / sin pair
    assert abs(np.corrcoef(t[..., :-1].ravel(), t[..., 1:].ravel())[0, 1]) <= 5.0 / np.sqrt(t.size)


def test_properties_of_drawn_terrains():
    import torch
    n = 4096
    # BOXES: 0 or one of the terrain's box heights
    G = gen_for("BOXES", 16, 16, defaults("BOXES"))
    plan = G.draw_plan(n, 31)
    hf = G.generate_with(plan)
    assert torch.isfinite(hf).all()
    ok = (hf == 0) | (hf[..., None] == plan["boxes"][:, None, None, :, 5]).any(dim=-1)
    assert ok.all() and (hf != 0).any(dim=2).any(dim=1).float().mean() > 0.9
    # PATHS: the floor or a path height; the output is the max-pool of the un-pooled field of the same plan
    s = defaults("PATHS", maxpool_size=2)
    G, G0 = gen_for("PATHS", 16, 16, s), gen_for("PATHS", 16, 16, dict(s, maxpool_size=0))
    plan = G.draw_plan(n, 32)
    hf, raw = G.generate_with(plan), G0.generate_with(plan)
    assert torch.isfinite(hf).all() and torch.isfinite(raw).all()
    for f in (hf, raw):
        assert ((f == np.float32(s["floor_height"])) | (f[..., None] == plan["path_height"][:, None, None, :]).any(dim=-1)).all()
    assert np.array_equal(ref.maxpool(raw.cpu().numpy(), 2).view(np.uint32), hf.cpu().numpy().view(np.uint32))
    assert (raw != np.float32(s["floor_height"])).flatten(1).any(dim=1).all()          # every terrain has a painted cell (the start cell)
    # STAIRS: every painted value is a step height of one of the terrain's stairs; with a single stair (nothing overwrites it) a cell of
    # step j lies inside step j's box, so the heights rise along the stair
    for ns in (4, 1):
        s = defaults("STAIRS", num_stairs=ns)
        G = gen_for("STAIRS", 16, 16, s)
        plan = G.draw_plan(n, 33)
        hf_t = G.generate_with(plan)
        assert torch.isfinite(hf_t).all()
        st, hf = plan["stairs"].cpu().numpy().astype(np.float64), hf_t.cpu().numpy().astype(np.float64)
        steps = ref.stair_steps(st, DX)[0]
        j = (hf[:, :, :, None] - st[:, None, None, :, 4]) / st[:, None, None, :, 5]      # [Q, X, Y, S] the step index each stair would need
        jr = np.rint(j)
        match = (np.abs(j - jr) * st[:, None, None, :, 5] <= 1e-6) & (jr >= 0) & (jr < steps[:, None, None, :])
        assert ((hf == 0) | match.any(axis=-1)).all()
    last = st[:, -1]
    d = last[:, 2:4] - last[:, 0:2]
    width = np.linalg.norm(d, axis=1)
    u = d / width[:, None]
    xs = np.arange(16) * np.float64(np.float32(DX))
    px = xs[None, :, None] - last[:, 0, None, None]
    py = xs[None, None, :] - last[:, 1, None, None]
    along = px * u[:, 0, None, None] + py * u[:, 1, None, None]
    across = -px * u[:, 1, None, None] + py * u[:, 0, None, None]
    mine = match[..., -1] & (hf != 0)
    centre = jr[..., -1] * (width / steps[:, -1])[:, None, None]
    assert mine.sum() > 512 and (np.abs(along - centre)[mine] <= np.float32(DX) / 2 + 1e-4).all()
    assert (np.abs(across)[mine] <= (last[:, 6] / 2)[:, None, None].repeat(16, 1).repeat(16, 2)[mine] + 1e-4).all()
    assert (st[..., 5] >= s["min_step_height"] - 1e-6).all()                            # positive step heights: j up = height up


def test_refusals():
    import torch
    from parc_amd import lib as L
    from parc_amd import terrain_gen as tg
    with pytest.raises(ValueError, match="PARC_TGEN_MAX_DIM"):
        tg.TerrainGenerator("BOXES", 80, 80, DX, device=DEV)
    with pytest.raises(ValueError, match="PARC_TGEN_MAX_BOXES"):
        tg.TerrainGenerator("BOXES", 16, 16, DX, settings=tg.BoxesSettings(num_boxes=65), device=DEV)
    G = gen_for("PATHS", 16, 16, defaults("PATHS"))
    good = G.draw_plan(4, 1)
    with pytest.raises(ValueError, match=r"path_turn must be torch.float32 \(4, 4, 1000\)"):
        G.generate_with(dict(good, path_turn=good["path_turn"][:, :, :999].contiguous()))
    with pytest.raises(ValueError, match="path_vy must be torch.float32"):
        G.generate_with(dict(good, path_vy=good["path_vy"].double()))
    with pytest.raises(ValueError, match="path_height is missing"):
        G.generate_with({k: v for k, v in good.items() if k != "path_height"})
    with pytest.raises(ValueError, match="path_start must have shape"):
        G.plan_from_numpy({k: (v.cpu().numpy()[:, :3] if k == "path_start" else v.cpu().numpy()) for k, v in good.items()})
    bad = {k: v.clone() for k, v in good.items()}
    bad["path_turn"][2, 1, 500] = float("nan")
    with pytest.raises(L.ParcError, match="path_turn holds a value that is not finite"):
        G.generate_with(bad, validate=True)
    bad = {k: v.clone() for k, v in good.items()}
    bad["path_start"][3, 0, 1] = float("inf")
    with pytest.raises(L.ParcError, match="path_start holds a value that is not finite"):
        G.generate_with(bad, validate=True)
    assert torch.equal(G.generate_with(good, validate=True), G.generate_with(good))     # a good plan passes, and the handle still works
    # without the validate pass a bad entry is handled memory-safely: the other paths and terrains are unaffected
    hf = G.generate_with(bad)
    assert torch.isfinite(hf).all() and torch.equal(hf[:3], G.generate_with(good)[:3])
    S = gen_for("STAIRS", 16, 16, defaults("STAIRS"))
    sp = S.draw_plan(2, 1)
    sp["stairs"][1, 2, 0] = 1e6                                                       # a stair of 2.5 million steps
    with pytest.raises(L.ParcError, match="PARC_TGEN_MAX_STEPS"):
        S.generate_with(sp, validate=True)
    B = gen_for("BOXES", 16, 16, defaults("BOXES"))
    bp = B.draw_plan(2, 1)
    bp["boxes"][0, 0, 4] = float("nan")
    with pytest.raises(L.ParcError, match="boxes holds a value that is not finite"):
        B.generate_with(bp, validate=True)


def test_plan_paths_script_boxes(tmp_path):
    """scripts/plan_paths.py --procgen_mode BOXES: terrains with paths that start and end at their cells, terrain_round within bounds."""
    from parc_amd import path_planner as pp
    out = subprocess.run([sys.executable, os.path.join(REPO, "scripts/plan_paths.py"), "--procgen_mode", "BOXES", "--num_terrains", "64", "--seed", "4",
                          "--out", str(tmp_path)], check=True, capture_output=True, text=True, timeout=300)
    summary = json.loads(out.stdout.strip().splitlines()[-1])
    z = np.load(tmp_path / "paths_0000.npz")
    ok = z["attempt"] >= 0
    assert summary["procgen_mode"] == "BOXES" and summary["terrains"] == 64 and summary["found"] == int(ok.sum()) >= 1
    assert z["hf"].shape == (64, 16, 16) and ((z["status"] == pp.FOUND) == ok).all()
    rounds = z["terrain_round"]
    assert rounds.shape == (64,) and rounds.min() >= 0 and rounds.max() < 3 and (rounds[~ok] == 2).all()
    assert summary["queries"] == 10 * (64 + int((rounds >= 1).sum()) + int((rounds >= 2).sum()))
    assert np.array_equal(z["min_point_offset"], np.zeros((64, 2), np.float32)) and len(np.unique(z["hf"])) > 2
    for t in range(64):
        nd = z["nodes"][z["node_off"][t]:z["node_off"][t + 1]]
        if not ok[t]:
            assert len(nd) == 0
            continue
        assert np.array_equal(nd[0], z["start"][t]) and np.array_equal(nd[-1], z["goal"][t])
        pts = z["points"][z["point_off"][t]:z["point_off"][t + 1]]
        assert len(pts) >= len(nd) and pts[-1, 2] == z["hf"][t][nd[-1, 0], nd[-1, 1]]
