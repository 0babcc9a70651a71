#!/usr/bin/env python3
"""Generate the procedural terrain generator fixtures (``terrain_gen_{boxes,paths,stairs}.npz``) from the REAL reference.

Run where the reference checkout is available (the tests only read the fixtures it writes):

    python tests/golden/make_golden_terrain_gen.py [boxes|paths|stairs ...]

Drives the reference's own ``terrain_util.add_boxes_to_hf2``, ``gen_paths_hf`` and ``add_stairs_to_hf`` as stage 2 calls them
(``parc_2_kin_gen.py:247-290``) while ``torch.rand`` / ``torch.randn`` / ``random.random`` / ``np.random.random`` are wrapped to record
what they return.  The record is turned into a *plan* of derived fp32 values with the reference's own expressions (in torch, so the
bits are the ones the reference computed), and the plan, the reference's heightfield and the *unstable* mask of the restatement
(``tests/terrain_gen_ref.py``) are written.  Asserted here and written into ``notes``: the restatement reproduces every heightfield
outside the mask (bit for bit; STAIRS within 1e-6); the mask covers at most 1 % (BOXES, STAIRS) / 2 % (PATHS) of a fixture's cells;
stairs whose ``width / dx`` lies within 1e-6 of an integer are dropped (the whole candidate terrain) and counted.  Fixtures hold data only.
"""
import contextlib
import io
import json
import os
import random
import sys
import time
import types

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.dont_write_bytecode = True

for _name in ["trimesh", "trimesh.creation", "wandb", "gym", "gym.spaces", "isaacgym", "isaacgym.gymapi", "isaacgym.gymtorch",
              "isaacgym.gymutil"]:
    sys.modules[_name] = types.ModuleType(_name)
sys.modules["wandb"].run = None
sys.modules["trimesh"].creation = sys.modules["trimesh.creation"]
_parc = types.ModuleType("parc")
_parc.__path__ = [os.path.join(REF, "PARC")]
sys.modules["parc"] = _parc

import numpy as np  # noqa: E402
import torch  # noqa: E402

import terrain_gen_ref as ref  # noqa: E402

import parc.util.terrain_util as terrain_util  # noqa: E402

torch.set_num_threads(1)
DX = 0.4
# the reference's stage-2 default config (data/configs/terrain_gen/terrain_gen_default.yaml)
BOXES = dict(num_boxes=10, min_box_h=-2.0, max_box_h=2.0, box_max_len=10, box_min_len=5, max_box_angle=0.0, min_box_angle=0.0)
PATHS = dict(num_terrain_paths=4, maxpool_size=1, path_min_height=-1.6, path_max_height=2.0, floor_height=-2.0)
STAIRS = dict(min_stair_start_height=-3.0, max_stair_start_height=1.0, min_step_height=0.15, max_step_height=0.25, num_stairs=4,
              min_stair_thickness=2.0, max_stair_thickness=8.0)
# (mode, settings, X, Y, terrains)
GROUPS = {"boxes": [("BOXES", BOXES, 16, 16, 6), ("BOXES", dict(BOXES, max_box_angle=6.28318530718), 16, 16, 6),
                    ("BOXES", dict(BOXES, max_box_angle=6.28318530718), 12, 20, 1)],
          "paths": [("PATHS", PATHS, 16, 16, 6), ("PATHS", dict(PATHS, maxpool_size=3), 16, 16, 2), ("PATHS", PATHS, 12, 20, 1)],
          "stairs": [("STAIRS", STAIRS, 16, 16, 8), ("STAIRS", STAIRS, 12, 20, 1)]}
SEEDS = {"boxes": 21, "paths": 22, "stairs": 23}


@contextlib.contextmanager
def recording(rec):
    """Wrap the four generators the three functions draw from; every returned value is appended to ``rec`` in call order."""
    o_rand, o_randn, o_random, o_nprandom = torch.rand, torch.randn, random.random, np.random.random

    def wrap(name, fn, keep):
        def f(*a, **k):
            v = fn(*a, **k)
            rec.append((name, keep(v)))
            return v
        return f

    torch.rand, torch.randn = wrap("rand", o_rand, lambda v: v.clone()), wrap("randn", o_randn, lambda v: v.clone())
    random.random, np.random.random = wrap("random", o_random, float), wrap("np_random", o_nprandom, float)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            yield
    finally:
        torch.rand, torch.randn, random.random, np.random.random = o_rand, o_randn, o_random, o_nprandom


def take(rec, name, shape=None):
    kind, v = rec.pop(0)
    assert kind == name, (kind, name)
    if shape is not None:
        assert tuple(v.shape) == shape, (tuple(v.shape), shape)
    return v


def f32(x):
    return np.float32(x)


def run_terrain(mode, s, X, Y):
    """One terrain through the reference: (plan entries of this terrain, hf, seconds)."""
    terrain = terrain_util.SubTerrain("terrain", x_dim=X, y_dim=Y, dx=DX, dy=DX, min_x=0.0, min_y=0.0, device="cpu")
    rec = []
    t0 = time.perf_counter()
    with recording(rec):
        if mode == "BOXES":
            terrain_util.add_boxes_to_hf2(terrain.hf, box_max_height=s["max_box_h"], box_min_height=s["min_box_h"], hf_maxmin=None,
                                          num_boxes=s["num_boxes"], box_max_len=s["box_max_len"], box_min_len=s["box_min_len"],
                                          max_angle=s["max_box_angle"], min_angle=s["min_box_angle"])
        elif mode == "PATHS":
            terrain_util.gen_paths_hf(terrain, num_paths=s["num_terrain_paths"], maxpool_size=s["maxpool_size"], floor_height=s["floor_height"],
                                      path_min_height=s["path_min_height"], path_max_height=s["path_max_height"])
        else:
            terrain_util.add_stairs_to_hf(terrain, min_stair_start_height=s["min_stair_start_height"],
                                          max_stair_start_height=s["max_stair_start_height"], min_step_height=s["min_step_height"],
                                          max_step_height=s["max_step_height"], num_stairs=s["num_stairs"],
                                          min_stair_thickness=s["min_stair_thickness"], max_stair_thickness=s["max_stair_thickness"])
    seconds = time.perf_counter() - t0
    hf = terrain.hf.numpy().astype(np.float32).copy()
    plan = {}
    if mode == "BOXES":   # add_boxes_to_hf2 :883-885, :908, the same expressions on the recorded uniforms
        rows = []
        for _ in range(s["num_boxes"]):
            c = take(rec, "rand", (2,)) * torch.tensor(hf.shape, dtype=torch.float32)
            ln = take(rec, "rand", (2,)) * (s["box_max_len"] - s["box_min_len"]) + s["box_min_len"]
            ang = take(rec, "rand", (1,)) * (s["max_box_angle"] - s["min_box_angle"]) + s["min_box_angle"]
            h = take(rec, "rand", (1,)) * (s["max_box_h"] - s["min_box_h"]) + s["min_box_h"]
            rows.append([c[0].item(), c[1].item(), ln[0].item(), ln[1].item(), ang[0].item(), h[0].item()])
        plan["boxes"] = np.array(rows, np.float32)
    elif mode == "PATHS":  # gen_paths_hf :568-581, generate_curvy_path :548-563
        P = s["num_terrain_paths"]
        max_point = terrain.dims * terrain.dxdy + terrain.min_point
        plan = dict(path_start=np.zeros((P, 2), np.float32), path_vy=np.zeros(P, np.float32), path_angle=np.zeros(P, np.float32),
                    path_turn=np.zeros((P, ref.PATH_POINTS), np.float32), path_height=np.zeros(P, np.float32))
        for p in range(P):
            start = take(rec, "rand", (2,)) * (max_point - terrain.min_point) + terrain.min_point
            vel = take(rec, "randn", (2,))
            ang = take(rec, "rand", (1,)) * 2.0 * torch.pi
            turn = torch.cat([take(rec, "randn", (1,)) for _ in range(ref.PATH_POINTS)])
            height = take(rec, "random") * (s["path_max_height"] - s["path_min_height"]) + s["path_min_height"]
            plan["path_start"][p], plan["path_vy"][p], plan["path_angle"][p] = start.numpy(), vel[1].item(), ang[0].item()
            plan["path_turn"][p], plan["path_height"][p] = turn.numpy(), f32(height)
    else:                  # add_stairs_to_hf :1010-1027
        rows = []
        for _ in range(s["num_stairs"]):
            a = take(rec, "rand", (2,)) * (terrain.get_max_point() - terrain.min_point) + terrain.min_point
            b = take(rec, "rand", (2,)) * (terrain.get_max_point() - terrain.min_point) + terrain.min_point
            h0 = take(rec, "np_random") * (s["max_stair_start_height"] - s["min_stair_start_height"]) + s["min_stair_start_height"]
            sh = take(rec, "np_random") * (s["max_step_height"] - s["min_step_height"]) + s["min_step_height"]
            th = take(rec, "np_random") * (s["max_stair_thickness"] - s["min_stair_thickness"]) + s["min_stair_thickness"]
            rows.append([a[0].item(), a[1].item(), b[0].item(), b[1].item(), f32(h0), f32(sh), f32(th)])
        plan["stairs"] = np.array(rows, np.float32)
    assert not rec, f"{len(rec)} recorded draws were not consumed"
    return plan, hf, seconds


def main():
    only = sys.argv[1:]
    for name, groups in GROUPS.items():
        if only and name not in only:
            continue
        seed = SEEDS[name]
        torch.manual_seed(seed); random.seed(seed); np.random.seed(seed)
        out, metas = {}, []
        masked = cells = differ_masked = kept = dropped = 0
        seconds = []
        for g, (mode, s, X, Y, n) in enumerate(groups):
            plans, hfs = [], []
            while len(hfs) < n:
                plan, hf, sec = run_terrain(mode, s, X, Y)
                if mode == "STAIRS":
                    steps, ratio = ref.stair_steps(plan["stairs"], DX)
                    if (np.abs(ratio - np.rint(ratio)) < 1e-6).any():
                        dropped += 1
                        continue
                kept += 1
                plans.append(plan); hfs.append(hf); seconds.append(sec)
            plan = {k: np.stack([p[k] for p in plans]) for k in plans[0]}
            want = np.stack(hfs)
            mine, unstable = ref.generate(mode, plan, X, Y, DX, DX, (0.0, 0.0), s)
            differ_masked += ref.compare(mode, mine, want, unstable, f"{name} group {g}")
            masked += int(unstable.sum()); cells += unstable.size
            out[f"g{g}_hf"], out[f"g{g}_unstable"] = want, unstable
            for k, v in plan.items():
                out[f"g{g}_plan_{k}"] = v
            metas.append(dict(mode=mode, settings=s, dim_x=X, dim_y=Y, dx=DX, dy=DX, min_point=[0.0, 0.0], terrains=n,
                              masked_share=float(unstable.mean())))
        share = masked / cells
        assert share <= ref.MASK_CAP[groups[0][0]], (name, share)
        notes = dict(mode=groups[0][0], cells=cells, masked_cells=masked, masked_share=share, cap=ref.MASK_CAP[groups[0][0]],
                     restatement_differs_in_masked_cells=differ_masked, restatement_differs_outside=0, kept=kept, dropped=dropped,
                     reference_cpu_seconds_per_terrain=float(np.mean(seconds)), seed=seed)
        np.savez_compressed(os.path.join(HERE, f"terrain_gen_{name}.npz"), groups=json.dumps(metas), notes=json.dumps(notes), **out)
        print(name, notes, flush=True)


if __name__ == "__main__":
    main()
