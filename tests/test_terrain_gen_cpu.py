"""Procedural terrain generator, host side (no GPU): the numpy restatement against the reference fixtures, the fixtures' caps, the
settings, the config file, the ctypes mirrors and the script's arguments."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import yaml

import terrain_gen_ref as ref
from parc_amd import terrain_gen as tg

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ["boxes", "paths", "stairs"]


def fixture(name):
    z = dict(np.load(os.path.join(REPO, "tests/golden", f"terrain_gen_{name}.npz")))
    z["groups"] = json.loads(str(z["groups"]))
    z["notes"] = json.loads(str(z["notes"]))
    return z


def group_plan(z, g):
    pre = f"g{g}_plan_"
    return {k[len(pre):]: z[k] for k in z if k.startswith(pre)}


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_matches_reference(name):
    z = fixture(name)
    for g, m in enumerate(z["groups"]):
        hf, unstable = ref.generate(m["mode"], group_plan(z, g), m["dim_x"], m["dim_y"], m["dx"], m["dy"], m["min_point"], m["settings"])
        assert np.array_equal(unstable, z[f"g{g}_unstable"])
        ref.compare(m["mode"], hf, z[f"g{g}_hf"], unstable, f"{name} group {g}")
        assert np.array_equal(ref.rounding_cells(m["mode"], group_plan(z, g), m["dim_x"], m["dim_y"], m["dx"], m["dy"], m["min_point"], m["settings"]),
                              unstable)


def test_fixture_conditions():
    """What the generator asserted, re-checked on the committed files: the mask caps, the shapes and counts the fixtures must have."""
    shapes = {}
    for name in FIXTURES:
        z = fixture(name)
        n = z["notes"]
        mode = n["mode"]
        masked = sum(int(z[f"g{g}_unstable"].sum()) for g in range(len(z["groups"])))
        cells = sum(z[f"g{g}_unstable"].size for g in range(len(z["groups"])))
        assert (masked, cells) == (n["masked_cells"], n["cells"]) and n["cap"] == ref.MASK_CAP[mode]
        assert masked <= ref.MASK_CAP[mode] * cells and n["masked_share"] <= n["cap"]
        assert n["restatement_differs_outside"] == 0 and n["kept"] == sum(m["terrains"] for m in z["groups"]) and n["dropped"] >= 0
        assert n["reference_cpu_seconds_per_terrain"] > 0
        shapes[name] = [(m["terrains"], m["dim_x"], m["dim_y"]) for m in z["groups"]]
        for g, m in enumerate(z["groups"]):
            assert z[f"g{g}_hf"].shape == (m["terrains"], m["dim_x"], m["dim_y"]) and z[f"g{g}_hf"].dtype == np.float32
        assert os.path.getsize(os.path.join(REPO, "tests/golden", f"terrain_gen_{name}.npz")) < 800_000
    assert shapes == {"boxes": [(6, 16, 16), (6, 16, 16), (1, 12, 20)], "paths": [(6, 16, 16), (2, 16, 16), (1, 12, 20)],
                      "stairs": [(8, 16, 16), (1, 12, 20)]}
    b, p, s = fixture("boxes"), fixture("paths"), fixture("stairs")
    assert b["groups"][0]["settings"]["max_box_angle"] == 0.0 and abs(b["groups"][1]["settings"]["max_box_angle"] - 2 * np.pi) < 1e-6
    assert (b["g0_plan_boxes"][..., 4] == 0).all() and (b["g1_plan_boxes"][..., 4] > 0).all()
    assert [m["settings"]["maxpool_size"] for m in p["groups"]] == [1, 3, 1] and p["g0_plan_path_turn"].shape == (6, 4, 1000)
    assert s["g0_plan_stairs"].shape == (8, 4, 7)
    steps, ratio = ref.stair_steps(s["g0_plan_stairs"], 0.4)
    assert (np.abs(ratio - np.rint(ratio)) >= 1e-6).all() and steps.min() >= 1


def test_restatement_semantics():
    """Hand-checkable cases: strict box edges and overwrite order, the walk's first cell and border clamp, a single-step stair."""
    boxes = np.array([[[4.0, 4.0, 4.0, 2.0, 0.0, 1.0], [5.0, 4.0, 2.0, 2.0, 0.0, -1.0]]], np.float32)
    hf, unstable = ref.boxes_hf(boxes, 8, 8)
    want = np.zeros((8, 8), np.float32)
    want[3:6, 4] = 1.0                  # x in (2, 6), y in (3, 5), strictly: 3, 4, 5 x 4
    want[5, 4] = -1.0                   # the later box: x in (4, 6), y in (3, 5)
    assert np.array_equal(hf[0], want) and unstable[0, 2, 4] and unstable[0, 6, 4] and not unstable[0, 3, 4]
    plan = dict(path_start=np.array([[[1.19, 0.8]]], np.float32), path_vy=np.zeros((1, 1), np.float32), path_angle=np.zeros((1, 1), np.float32),
                path_turn=np.zeros((1, 1, 1000), np.float32), path_height=np.array([[2.0]], np.float32))
    hf, _ = ref.paths_hf(plan, 8, 8, 0.4, 0.4, floor_height=-1.0, maxpool_size=0)
    want = np.full((8, 8), -1.0, np.float32)
    want[3:, 2] = 2.0                   # starts at round(2.975) = 3, walks +x at 1 m/s for 33 s: clamps on the border row
    assert np.array_equal(hf[0], want)
    pooled, _ = ref.paths_hf(plan, 8, 8, 0.4, 0.4, floor_height=-1.0, maxpool_size=1)
    want[2:, 1:4] = 2.0
    assert np.array_equal(pooled[0], want)
    stairs = np.array([[[1.1, 1.0, 1.4, 1.0, 0.5, 0.2, 1.0]]], np.float32)      # 0.3 m long: ceil(0.75) = 1 step at the start point
    hf, _ = ref.stairs_hf(stairs, 8, 8, 0.4, 0.4)
    assert ref.stair_steps(stairs, 0.4)[0].tolist() == [[1]] and sorted(set(hf.ravel().tolist())) == [0.0, 0.5]
    assert np.argwhere(hf[0] == 0.5).tolist() == [[3, 2], [3, 3]]                # x in (0.9, 1.3): 1.2; y in (0.5, 1.5): 0.8, 1.2
    stairs[0, 0, 2] = 2.0                                                       # 0.9 m: 3 steps 0.3 m apart, heights 0.5, 0.7, 0.9 in double
    hf, _ = ref.stairs_hf(stairs, 8, 8, 0.4, 0.4)
    assert hf[0, 4, 2] == np.float32(np.float64(np.float32(0.5)) + 2 * np.float64(np.float32(0.2)))


def test_settings_defaults_config_and_unknown_keys(tmp_path):
    assert tg.BoxesSettings().to_config() == dict(num_boxes=10, min_box_h=-3.0, max_box_h=3.0, box_max_len=10.0, box_min_len=5.0,
                                                  max_box_angle=6.28318530718, min_box_angle=0.0)
    assert tg.PathsSettings().to_config() == dict(num_terrain_paths=4, maxpool_size=1, path_min_height=-2.8, path_max_height=3.0, floor_height=-3.0)
    assert tg.StairsSettings().to_config() == dict(min_stair_start_height=-3.0, max_stair_start_height=1.0, min_step_height=0.15,
                                                   max_step_height=0.25, num_stairs=4, min_stair_thickness=2.0, max_stair_thickness=8.0)
    cfg = tg.TerrainGenConfig.load(os.path.join(REPO, "data/configs/terrain_gen/terrain_gen_default.yaml"))
    assert (cfg.boxes.num_boxes, cfg.boxes.min_box_h, cfg.boxes.max_box_h, cfg.boxes.box_min_len, cfg.boxes.box_max_len, cfg.boxes.max_box_angle) == \
        (10, -2.0, 2.0, 5.0, 10.0, 0.0)
    assert (cfg.paths.num_terrain_paths, cfg.paths.maxpool_size, cfg.paths.path_min_height, cfg.paths.path_max_height, cfg.paths.floor_height) == \
        (8, 1, -1.6, 2.0, -2.0)
    assert cfg.stairs == tg.StairsSettings() and isinstance(cfg.paths.maxpool_size, int)
    path = tmp_path / "tgen.yaml"
    path.write_text(yaml.safe_dump(cfg.to_dict()))
    assert tg.TerrainGenConfig.load(path) == cfg and cfg.settings("PATHS") is cfg.paths
    with pytest.raises(ValueError, match="box_len"):
        tg.BoxesSettings.from_config({"box_len": 1.0})
    with pytest.raises(ValueError, match="ramps"):
        tg.TerrainGenConfig.from_dict({"ramps": {}})
    with pytest.raises(ValueError, match="maxpool"):
        tg.TerrainGenConfig.from_dict({"paths": {"maxpool": 2}})


def test_ctypes_mirrors_limits_and_refusals():
    from parc_amd import lib as L
    hdr = open(os.path.join(REPO, "include/parc_env.h")).read()
    macros = dict(PARC_TGEN_MAX_DIM=(tg.MAX_DIM, L.TGEN_MAX_DIM), PARC_TGEN_MAX_BOXES=(tg.MAX_BOXES, L.TGEN_MAX_BOXES),
                  PARC_TGEN_MAX_PATHS=(tg.MAX_PATHS, L.TGEN_MAX_PATHS), PARC_TGEN_MAX_STAIRS=(tg.MAX_STAIRS, L.TGEN_MAX_STAIRS),
                  PARC_TGEN_MAX_POOL=(tg.MAX_POOL, L.TGEN_MAX_POOL), PARC_TGEN_PATH_POINTS=(tg.PATH_POINTS, L.TGEN_PATH_POINTS),
                  PARC_TGEN_MAX_STEPS=(tg.MAX_STEPS, L.TGEN_MAX_STEPS), PARC_TGEN_BOX_FLOATS=(tg.BOX_FLOATS, L.TGEN_BOX_FLOATS),
                  PARC_TGEN_STAIR_FLOATS=(tg.STAIR_FLOATS, L.TGEN_STAIR_FLOATS))
    for name, (a, b) in macros.items():
        m = re.search(rf"#define {name} (\d+)\s", hdr)
        assert m and int(m.group(1)) == a == b, name
    assert (tg.MAX_DIM, tg.MAX_BOXES, tg.MAX_PATHS, tg.MAX_STAIRS, tg.MAX_POOL, tg.PATH_POINTS) == (64, 64, 64, 16, 8, 1000)
    assert ref.PATH_POINTS == tg.PATH_POINTS and tg.BOX_FLOATS == L.MSAMP_BOX_FLOATS
    for k, mode in enumerate(tg.MODES):
        assert re.search(rf"#define PARC_TGEN_{mode} {k}\s", hdr)
    assert tuple(L.TGEN_MODES) == tg.MODES
    assert C.sizeof(L.ParcTerrainGenParams) == 4 * (9 + 7 + 5 + 7) and L.ParcTerrainGenParams.num_boxes.offset == 36
    assert L.ParcTerrainGenParams.num_terrain_paths.offset == 64 and L.ParcTerrainGenParams.num_stairs.offset == 84
    assert C.sizeof(L.ParcTerrainGenPlan) == 8 * 8 and L.TGEN_PLAN_FIELDS == ["boxes", "path_start", "path_vy", "path_angle", "path_turn", "path_height", "stairs"]
    # the struct fields follow the header's order
    body = hdr[hdr.index("/* the ranges parc_tgen_draw_plan draws from"):hdr.index("} ParcTerrainGenParams;")]
    names = [n for n in re.findall(r"\b([a-z_]+)\b(?=\s*[,;])", re.sub(r"/\*.*?\*/", "", body))]
    assert names == [n for n, _ in L.TGEN_BOXES_FIELDS + L.TGEN_PATHS_FIELDS + L.TGEN_STAIRS_FIELDS]
    for cls, fields in ((tg.BoxesSettings, L.TGEN_BOXES_FIELDS), (tg.PathsSettings, L.TGEN_PATHS_FIELDS), (tg.StairsSettings, L.TGEN_STAIRS_FIELDS)):
        assert sorted(cls().to_config()) == sorted(n for n, _ in fields)
    assert "#define PARC_ABI_VERSION 6" in hdr and L.ABI_VERSION == 6
    for sym in ("parc_tgen_create", "parc_tgen_destroy", "parc_tgen_draw_plan", "parc_tgen_generate_with", "parc_tgen_generate", "parc_tgen_kernel_times"):
        assert sym in L.EXPORTED_SYMBOLS and f" {sym}(" in hdr
    # refused before the device is touched: this passes on a machine without a GPU
    lib = L.load()
    h = C.c_void_p()
    p = tg.generator_params("BOXES", tg.BoxesSettings(), 16, 16, 0.4)
    p.struct_size -= 4
    with pytest.raises(L.ParcError, match=r"ParcTerrainGenParams ABI mismatch \(struct_size\)"):
        L.check(lib.parc_tgen_create(C.byref(p), C.byref(h)))
    cases = [("BOXES", tg.BoxesSettings(), 80, 80, "PARC_TGEN_MAX_DIM"), ("BOXES", tg.BoxesSettings(), 3, 16, "PARC_TGEN_MAX_DIM"),
             ("BOXES", tg.BoxesSettings(num_boxes=65), 16, 16, "PARC_TGEN_MAX_BOXES"),
             ("PATHS", tg.PathsSettings(num_terrain_paths=65), 16, 16, "PARC_TGEN_MAX_PATHS"),
             ("PATHS", tg.PathsSettings(maxpool_size=9), 16, 16, "PARC_TGEN_MAX_POOL"),
             ("STAIRS", tg.StairsSettings(num_stairs=17), 16, 16, "PARC_TGEN_MAX_STAIRS")]
    for mode, s, X, Y, macro in cases:
        with pytest.raises(L.ParcError, match=macro):
            L.check(lib.parc_tgen_create(C.byref(tg.generator_params(mode, s, X, Y, 0.4)), C.byref(h)))
        with pytest.raises(ValueError, match=macro):
            tg.check_limits(mode, s, X, Y)
        with pytest.raises(ValueError, match=macro):
            tg.TerrainGenerator(mode, X, Y, 0.4, settings=s)
    with pytest.raises(ValueError, match="FILE"):
        tg.TerrainGenerator("FILE")


def test_plan_paths_help_lists_the_modes():
    out = subprocess.run([sys.executable, os.path.join(REPO, "scripts/plan_paths.py"), "--help"], capture_output=True, text=True, check=True).stdout
    assert "--procgen_mode" in out and "{FILE,BOXES,PATHS,STAIRS}" in out.replace(" ", "")
    assert "--terrain_config" in out and "--max_terrain_rounds" in out
