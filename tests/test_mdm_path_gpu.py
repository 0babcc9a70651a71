"""Path-following motion generation on the GPU against the reference's records (``tests/golden/mdm_path.npz``,
``make_golden_mdm_path.py``) and against ``mdm_path_ref``.  The yardstick of a float comparison is the float64 record, the unit the
reference's own fp32-vs-float64 difference; the wrapper's tensors must stay within ``10 x unit + 1e-6`` (10: the level from which
section 8j counts a ratio as a defect), what passes through the generator within the bound of ``test_mdm_gpu.py`` (its ``K``)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mdm_path_ref as PR
import mdm_ref as R
from parc_amd import motion_generator as mg
from parc_amd import motion_path_gen as mpg
from test_mdm_gpu import K

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
DEV = "cuda:0"
WRAP = 10.0


@pytest.fixture(scope="module")
def fx():
    return PR.PathFixture(GOLDEN)


@pytest.fixture(scope="module")
def model():
    return R.Fixture(GOLDEN)


@pytest.fixture(scope="module")
def gen(model):
    return mg.MDMGenerator.from_state_dict(model.cfg, model.sd, model.mean, model.std, DEV, max_batch=8)


@pytest.fixture(scope="module")
def pgs(gen, fx):
    """A handle per guidance setting of the records (``limit``: on; ``mixed`` / ``alldone``: off), on the one generator."""
    return {cfg: mpg.PathMotionGenerator(gen, mpg.MDMPathSettings(max_motion_length=fx.max_motion_length), mpg.MDMGenSettings(ddim_stride=fx.stride, use_cfg=cfg))
            for cfg in (True, False)}


@pytest.fixture(scope="module")
def pg(pgs):
    return pgs[True]


def set_scene(pg, fx, rec, rows=6):
    hf, mp = fx.terrain(rec)
    pg.set_scene(hf[None], mp[None], fx.dx, [fx.raw(f"{rec}/path")], rows)


def handle(pgs, fx, rec, rows=6):
    pg = pgs[fx.use_cfg(rec)]
    set_scene(pg, fx, rec, rows)
    return pg


def ratio(name, got, fx, key, extra=0.0, bound=WRAP):
    got = np.asarray(torch.as_tensor(got).detach().cpu().double())
    want, unit = fx.f64(key).numpy().reshape(got.shape), fx.err32(key)
    err = np.abs(got - want).max()
    print("%-34s unit %.3e  hip-ref64 %.3e  ratio %.2f" % (name, unit, err, err / max(unit, 1e-30)))
    assert np.isfinite(got).all(), name
    assert err <= bound * unit + 1e-6 + extra, (name, err, unit)
    return err / max(unit, 1e-30)


def quat_up_to_sign(got, want):
    got, want = torch.as_tensor(got).double().cpu(), torch.as_tensor(want).double()
    s = torch.sign((got * want).sum(-1, keepdim=True))
    return got * torch.where(s == 0, torch.ones_like(s), s)


def prev_state_key(fx, rec, w):
    """The record's previous-state components as the standardised features the kernel writes: float64 values, and the unit."""
    comp = {k: fx.f64(f"{rec}/w{w}/ps_{k}") for k in ("ROOT_POS", "ROOT_ROT", "JOINT_POS")}
    p = fx.prev(rec, w)
    comp["JOINT_ROT"], comp["CONTACTS"] = p["joint_rot"], p["contacts"]
    return comp


def check_prev_state(name, c, comp, fx, keys, r64, rows=slice(None), extra=0.0):
    """The standardised previous state against the record's components through the float64 assembly; the unit is the largest of the
    components' own, scaled by the smallest std (standardising divides by it)."""
    want = (r64.features(comp) - r64.mean[:2]) / r64.std[:2]
    unit = max(fx.err32(k) for k in keys) / float(r64.std[:2].min())
    err = (c["PREV_STATE_KEY"].cpu().double() - want)[rows].abs().max().item()
    print("%-34s unit %.3e  hip-ref64 %.3e  ratio %.2f" % (name, unit, err, err / max(unit, 1e-30)))
    assert err <= WRAP * unit + 1e-6 + extra / float(r64.std[:2].min()), (name, err, unit)
    return err / max(unit, 1e-30)


def test_conditions_steps(pgs, fx, gen, model):
    """k_mpath_cond on every recorded window: heights bit-equal, nodes and done exact, target and previous state within 10 units."""
    r64 = PR.PathRef(model.cfg, gen.char_model, model.mean, model.std, pgs[True].path_settings, pgs[True].gen_settings, torch.float64)
    worst = 0.0
    seen_done = False
    for rec in fx.RECORDS:
        pg = handle(pgs, fx, rec)
        for w in range(fx.windows(rec)):
            prev = fx.prev(rec, w, torch.float32)
            c = pg.conds(prev, first=w == 0, blank=w == 0 and fx.blank(rec))
            cz = prev["root_pos"][:, -1, 2]
            want_hf = torch.clamp(torch.from_numpy(fx.raw(f"{rec}/w{w}/hf_cell")) - cz[:, None, None], -gen.max_h, gen.max_h) / gen.max_h
            assert torch.equal(c["OBS_KEY"].cpu(), want_hf), (rec, w)
            assert np.array_equal(c["target_node"].cpu().numpy(), fx.raw(f"{rec}/w{w}/target_node")), (rec, w)
            if w > 0:
                assert np.array_equal(c["closest_node"].cpu().numpy(), fx.raw(f"{rec}/w{w}/closest_node")), (rec, w)
                assert np.array_equal(c["done"].cpu().numpy(), fx.raw(f"{rec}/w{w}/done")), (rec, w)
                seen_done |= bool(c["done"].any())
            flags = fx.raw(f"{rec}/w{w}/flags")
            for i, k in enumerate(("OBS_FLAG_KEY", "TARGET_FLAG_KEY", "PREV_STATE_FLAG_KEY", "PREV_STATE_NOISE_IND_KEY")):
                assert np.array_equal(c[k].cpu().numpy(), flags[:, i]), (rec, w, k)
            worst = max(worst, ratio(f"{rec} w{w} target", c["TARGET_KEY"], fx, f"{rec}/w{w}/target"))
            worst = max(worst, check_prev_state(f"{rec} w{w} prev_state", c, prev_state_key(fx, rec, w), fx,
                                                [f"{rec}/w{w}/ps_{k}" for k in ("ROOT_POS", "ROOT_ROT", "JOINT_POS")], r64))
    assert seen_done
    print("conditions, steps scene: worst ratio %.2f" % worst)


def test_conditions_nodes(pg, fx, gen, model):
    """The closest-node reduction and the lookahead clamp on an 80-node path (a strided loop and the whole shuffle tree): rows at the
    start, on a tie (the lower node wins), past node 64, where the lookahead is clamped to the last node, on the last node (done) and
    far off the path; exact against the reference's record."""
    z = fx.z
    hf, mp = z["flat/hf"], z["flat/min_point"]
    pg.set_scene(hf[None], mp[None], fx.dx, [z["nodes/path"]], 6)
    prev = {k: torch.from_numpy(z[f"nodes/prev_{k}"]) for k in PR.FRAME_KEYS}
    c = pg.conds(prev)
    assert c["closest_node"].cpu().tolist() == z["nodes/closest_node"].tolist() == [0, 30, 66, 75, 79, 44]
    assert c["target_node"].cpu().tolist() == z["nodes/target_node"].tolist() == [7, 37, 73, 79, 79, 51]
    assert c["done"].cpu().tolist() == z["nodes/done"].tolist() == [False, False, False, False, True, False]
    cz = prev["root_pos"][:, -1, 2]
    assert torch.equal(c["OBS_KEY"].cpu(), torch.clamp(torch.from_numpy(z["nodes/hf_cell"]) - cz[:, None, None], -gen.max_h, gen.max_h) / gen.max_h)
    far = 2.4e-7 * float(np.abs(z["nodes/prev_root_pos"]).max())   # the roots stand up to 30 m from the origin
    ratio("nodes target", c["TARGET_KEY"], fx, "nodes/target", extra=far)
    r64 = PR.PathRef(model.cfg, gen.char_model, model.mean, model.std, pg.path_settings, pg.gen_settings, torch.float64)
    comp = {k: fx.f64(f"nodes/ps_{k}") for k in ("ROOT_POS", "ROOT_ROT", "JOINT_POS")}
    comp["JOINT_ROT"], comp["CONTACTS"] = prev["joint_rot"].double(), prev["contacts"].double()
    check_prev_state("nodes prev_state", c, comp, fx, [f"nodes/ps_{k}" for k in ("ROOT_POS", "ROOT_ROT", "JOINT_POS")], r64, extra=far)
    # a row whose root is not finite compares with nothing: node 0, no fault
    bad = {k: v.clone() for k, v in prev.items()}
    bad["root_pos"][2] = float("nan")
    cb = pg.conds(bad)
    assert cb["closest_node"].cpu().tolist()[2] == 0 and cb["target_node"].cpu().tolist()[2] == 7
    assert cb["closest_node"].cpu().tolist()[:2] == [0, 30]


def test_conditions_rough(fx, gen, model):
    """The rough scene: a height may differ only at samples nearer than 1e-4 cells to a cell boundary, at most 0.5 % of a row."""
    z = fx.z
    pg = mpg.PathMotionGenerator(gen)
    off = z["rough/far_offset"]
    mps = np.stack([z["rough/min_point"], z["rough/min_point"] + off])
    tg = z["rough/targets"]
    paths = [np.stack([tg[i], tg[i], tg[i]]) for i in range(6)]   # conds with first: the target is node 1
    # a scene of six paths: rows 0 .. 4 on the terrain, row 5 on the copy moved by the far offset
    pg.set_scene(np.stack([z["rough/hf"]] * 5 + [z["rough/hf"]]), np.concatenate([np.repeat(mps[:1], 5, 0), mps[1:]]), float(z["rough/dx"]), paths, 1)
    prev = {k: torch.from_numpy(z[f"rough/prev_{k}"]) for k in PR.FRAME_KEYS}
    c = pg.conds(prev, first=True)
    want = torch.clamp(torch.from_numpy(z["rough/hf_z64"]), -gen.max_h, gen.max_h) / gen.max_h
    got = c["OBS_KEY"].cpu()
    far = 2.4e-7 * float(np.abs(z["rough/prev_root_pos"]).max())
    diff = (got - want).abs() > 1e-6
    dist = torch.from_numpy(z["rough/boundary_dist"])
    print("rough: samples that differ per row", diff.reshape(6, -1).sum(-1).tolist(), "nearer than 1e-4 cells", (dist < 1e-4).reshape(6, -1).sum(-1).tolist())
    assert not (diff & (dist >= 1e-4))[:5].any()
    assert not (diff & (dist >= 1e-4 + far / float(z["rough/dx"])))[5].any()
    assert (diff.reshape(6, -1).sum(-1) <= 0.005 * 961).all()
    for i, extra in ((slice(0, 5), 0.0), (slice(5, 6), far)):
        n = "rough rows 0-4" if extra == 0.0 else "rough far row"
        got_t, want_t = c["TARGET_KEY"][i].cpu().double(), fx.f64("rough/target")[i, 0]
        err = (got_t - want_t).abs().max().item()
        unit = fx.err32("rough/target")
        print("%-34s unit %.3e  hip-ref64 %.3e  ratio %.2f" % (n + " target", unit, err, err / max(unit, 1e-30)))
        assert err <= WRAP * unit + 1e-6 + extra
    # the standardised previous state: tilted roots, a heading near pi, a negative one, the row 300 m away
    r64 = PR.PathRef(model.cfg, gen.char_model, model.mean, model.std, pg.path_settings, pg.gen_settings, torch.float64)
    comp = {k: fx.f64(f"rough/ps_{k}") for k in ("ROOT_POS", "ROOT_ROT", "JOINT_POS")}
    comp["JOINT_ROT"], comp["CONTACTS"] = prev["joint_rot"].double(), prev["contacts"].double()
    keys = [f"rough/ps_{k}" for k in ("ROOT_POS", "ROOT_ROT", "JOINT_POS")]
    check_prev_state("rough rows 0-4 prev_state", c, comp, fx, keys, r64, rows=slice(0, 5))
    check_prev_state("rough far row prev_state", c, comp, fx, keys, r64, rows=slice(5, 6), extra=far)


def window_inputs(pg, fx, rec, w):
    prev = fx.prev(rec, w, torch.float32)
    return prev, pg.conds(prev, first=w == 0, blank=w == 0 and fx.blank(rec))


def test_append(pgs, fx, gen, model):
    """The recorded samples (standardised features rebuilt from the recorded world frames and the canonical record) through
    k_mpath_append: world frames within 10 units at the offsets of a first, a middle and a last window, the next previous state, and
    an untouched guard behind every row.  ``mixed`` runs without guidance with the indicator on: the previous frames must come from
    the clean previous state, whatever the sample holds there."""
    for rec in ("limit", "mixed"):
        append_record(handle(pgs, fx, rec), fx, gen, model, rec)
    append_guard_and_commit(handle(pgs, fx, "limit"), fx)


def append_record(pg, fx, gen, model, rec):
    r64 = PR.PathRef(model.cfg, gen.char_model, model.mean, model.std, pg.path_settings, pg.gen_settings, torch.float64)
    nprev, start, T, FD = pg.nprev, pg.start_frame, pg.T, pg.FD
    maxf = pg.max_frames
    off = 0
    for w, (lo, hi) in enumerate(((0, start), (nprev, start), (nprev, T))):
        prev, c = window_inputs(pg, fx, rec, w)
        # the canonical sample in float64 from the recorded world frames: the inverse of the un-canonicalisation, then the features
        out = {k: fx.f64(f"{rec}/w{w}/out_{k}") for k in PR.FRAME_KEYS}
        c64 = r64.conds(fx.scene(rec, torch.float64), fx.prev(rec, w), w == 0, w == 0)
        hqi = PR.heading_quat(-c64["heading"]).expand(6, T, 4)
        pos = out["root_pos"].clone()
        pos[..., 0:2] -= c64["canon_xy"]
        pos[..., 2] -= c64["canon_z"]
        pos = PR.qrot(hqi, pos)
        rot = PR.qmul(hqi, out["root_rot"])
        body = r64.fk_positions(pos, rot, out["joint_rot"])
        feat = r64.features({"ROOT_POS": pos, "ROOT_ROT": rot, "JOINT_POS": body[..., 1:, :], "JOINT_ROT": out["joint_rot"], "CONTACTS": out["contacts"]})
        x = ((feat - r64.mean) / r64.std).float().to(DEV)
        full = torch.zeros((6, maxf, FD), device=DEV)
        nxt = torch.zeros((6, nprev, FD), device=DEV)
        guided = bool(fx.raw(f"{rec}/w{w}/guided"))
        # limit: the indicator is off (first window) or void under guidance, every frame comes from x.  mixed: the indicator holds
        if bool(c["PREV_STATE_NOISE_IND_KEY"].all()) and not guided:
            x[:, :nprev] += 5.0
        else:
            assert rec == "limit"
        pg.append(x, c["PREV_STATE_KEY"], c["PREV_STATE_NOISE_IND_KEY"], c["canon"], full, off, lo, hi, guided, prev_next=nxt)
        got = pg.unpack_frames(full[:, off:off + hi - lo])
        for k in PR.FRAME_KEYS:
            want, unit = out[k][:, lo:hi], fx.err32(f"{rec}/w{w}/out_{k}")
            g = quat_up_to_sign(got[k], want) if k.endswith("rot") else got[k].cpu().double()
            err = (g - want).abs().max().item()
            print("%-34s unit %.3e  hip-ref64 %.3e  ratio %.2f" % (f"append w{w} {k}", unit, err, err / max(unit, 1e-30)))
            assert err <= WRAP * unit + 1e-6, (w, k, err, unit)
        assert torch.equal(nxt, full[:, off + (start - nprev) - lo:off + start - lo]) if lo <= start - nprev else True
        assert (full[:, :off] == 0).all() and (full[:, off + hi - lo:] == 0).all()
        off += hi - lo


def append_guard_and_commit(pg, fx):
    rec, guard, start, T, FD = "limit", 3, pg.start_frame, pg.T, pg.FD
    # the guard: a row's max_frames is its last frame
    x = torch.zeros((6, T, pg.D), device=DEV)
    tight = torch.full((6 * (start + guard), FD), 7.0, device=DEV)
    rows = tight[:6 * start].reshape(6, start, FD)
    prev, c = window_inputs(pg, fx, rec, 0)
    pg.append(x, c["PREV_STATE_KEY"], c["PREV_STATE_NOISE_IND_KEY"], c["canon"], rows, 0, 0, start, False)
    assert (tight[6 * start:] == 7.0).all() and not (rows == 7.0).any()
    with pytest.raises(Exception, match="max_frames"):
        pg.append(x, c["PREV_STATE_KEY"], c["PREV_STATE_NOISE_IND_KEY"], c["canon"], rows, 1, 0, start, False)
    # final_frame: set where the row is done and still at -1, and only then
    done = torch.tensor([1, 0, 1, 1, 0, 0], dtype=torch.int32, device=DEV)
    final = torch.tensor([-1, -1, 9, -1, 16, -1], dtype=torch.int32, device=DEV)
    pg.append(x, c["PREV_STATE_KEY"], c["PREV_STATE_NOISE_IND_KEY"], c["canon"], rows, 0, 0, start, False, done=done, final_frame=final, total=23)
    assert final.cpu().tolist() == [23, -1, 9, 23, 16, -1]


def hip_window(pg, gen, fx, rec, w, x_T):
    """One window through the three pieces: conditions kernel, the generator's sampler on them, append kernel."""
    prev, c = window_inputs(pg, fx, rec, w)
    guided = bool(fx.raw(f"{rec}/w{w}/guided"))
    x = gen.ddim_inference({k: c[k] for k in ("OBS_KEY", "TARGET_KEY", "PREV_STATE_KEY", "OBS_FLAG_KEY", "TARGET_FLAG_KEY", "PREV_STATE_FLAG_KEY",
                                              "PREV_STATE_NOISE_IND_KEY")}, x_T.to(DEV), fx.stride, guidance_scale=pg.gen_settings.cfg_scale if guided else None)
    full = torch.zeros((6, pg.T, pg.FD), device=DEV)
    pg.append(x, c["PREV_STATE_KEY"], c["PREV_STATE_NOISE_IND_KEY"], c["canon"], full, 0, 0, pg.T, guided)
    return pg.unpack_frames(full)


def test_teacher_forced_windows(pgs, gen, fx):
    """Every recorded window: recorded previous frames and x_T in, world frames out, within the generator's bound."""
    for rec in fx.RECORDS:
        pg = handle(pgs, fx, rec)
        xT = fx.x_T(rec)
        for w in range(fx.windows(rec)):
            got = hip_window(pg, gen, fx, rec, w, xT[w])
            for k in PR.FRAME_KEYS:
                want = fx.f64(f"{rec}/w{w}/out_{k}")
                g = quat_up_to_sign(got[k], want) if k.endswith("rot") else got[k]
                ratio(f"{rec} w{w} {k}", g, fx, f"{rec}/w{w}/out_{k}", bound=K)


def gen_sequence_callable(gen, fx, xT):
    def generate(c, w):
        c = dict(c)
        c["GUIDANCE_PARAMS"] = mg.GuidanceParams(c["GUIDANCE_PARAMS"])
        return gen.gen_sequence(c, fx.stride, "DDIM", noise=xT[w].to(DEV))
    return generate


def composed(pg, gen, fx, rec, xT):
    ref = PR.PathRef(gen.cfg, gen.char_model, gen.mean.cpu(), gen.std.cpu(), pg.path_settings, pg.gen_settings, torch.float32, DEV)
    return ref.rollout(fx.scene(rec, torch.float32, DEV), gen_sequence_callable(gen, fx, xT), [fx.rel_height], prev_frames=fx.start(rec, torch.float32, DEV))


@pytest.fixture(scope="module")
def rollouts(pgs, gen, fx):
    """``rollout`` on every record with the recorded x_T, and what ``describe`` says right after."""
    out = {}
    for rec in fx.RECORDS:
        pg = handle(pgs, fx, rec)
        start = fx.start(rec, torch.float32, DEV)
        res = pg.rollout(prev_frames=start, plan=None if start is not None else {"rel_height": torch.tensor([fx.rel_height])}, noise=fx.x_T(rec).to(DEV))
        out[rec] = (res, pg.describe())
    return out


def test_rollout_is_the_composition(pgs, gen, fx, rollouts):
    """``rollout`` with injected x_T against ``mdm_path_ref`` composing ``MDMGenerator.gen_sequence`` in torch on the device: integer
    outputs exact on the three records (the time limit; rows done at the second window, so their ``final_frame`` is set; the all-done
    exit, which leaves every ``final_frame`` at -1), frames within the generator's bound per window, counted from the window's own
    input."""
    for rec in fx.RECORDS:
        pg = handle(pgs, fx, rec)
        xT = fx.x_T(rec)
        res, d = rollouts[rec]
        ref = composed(pg, gen, fx, rec, xT)
        W = fx.windows(rec)
        assert res.windows == ref["windows"] == W == d["windows"]
        assert res.frames_per_window == ref["frames_per_window"] == fx.raw(f"{rec}/frames_per_window").tolist()
        assert res.num_frames == ref["num_frames"] == d["frames"]
        assert np.array_equal(res.final_frame.cpu().numpy(), fx.raw(f"{rec}/final_frame")), (rec, res.final_frame)
        assert np.array_equal(res.final_frame.cpu().numpy(), ref["final_frame"].cpu().numpy())
        assert torch.equal(res.done.cpu(), ref["done"].cpu())
        assert np.array_equal(res.done.cpu().numpy(), fx.raw(f"{rec}/w{W - 1}/done"))
        assert d["launches"] == W * (2 + 1 + 2 * pg.steps) + int(fx.blank(rec))
        if rec == "mixed":
            assert res.final_frame.cpu().tolist() == [16, 16, 16, -1, -1, -1] and W == 3
        if rec == "alldone":
            assert W == 2 and bool(res.done.all()) and res.final_frame.cpu().tolist() == [-1] * 6
        # per window from its own input: the torch composition of one window on the previous frames the HIP rollout itself used, against
        # the frames the HIP rollout appended; the unit is the reference's fp32-vs-float64 difference of that window
        ref = PR.PathRef(gen.cfg, gen.char_model, gen.mean.cpu(), gen.std.cpu(), pg.path_settings, pg.gen_settings, torch.float32, DEV)
        scene = fx.scene(rec, torch.float32, DEV)
        generate = gen_sequence_callable(gen, fx, xT)
        off = 0
        for w in range(W):
            n = res.frames_per_window[w]
            lo = 0 if w == 0 else pg.nprev
            prev = (fx.start(rec, torch.float32, DEV) or ref.blank_frames(scene, [fx.rel_height])) if w == 0 else {k: getattr(res, k)[:, off - pg.nprev:off] for k in PR.FRAME_KEYS}
            want_w, _ = ref.window(scene, prev, generate, w, w == 0, w == 0 and fx.blank(rec))
            for k in PR.FRAME_KEYS:
                got = getattr(res, k)[:, off:off + n]
                want = want_w[k][:, lo:lo + n].cpu().double()
                g = quat_up_to_sign(got, want) if k.endswith("rot") else got.cpu().double()
                unit = fx.err32(f"{rec}/w{w}/out_{k}")
                err = (g - want).abs().max().item()
                print("%-34s unit %.3e  hip-composition %.3e  ratio %.2f" % (f"{rec} rollout w{w} {k}", unit, err, err / max(unit, 1e-30)))
                assert err <= K * unit + 1e-6, (rec, w, k, err, unit)
            off += n


def test_batch_independence(pg, gen, fx):
    """A row alone, the six together and the six shuffled with their ids kept: bit-identical; the device's x_T is ``draw_noise`` at
    the documented key."""
    ids = np.array([11, 3, 250000, 7, 0, 42], np.int64)
    plan = {"rel_height": torch.tensor([fx.rel_height])}
    set_scene(pg, fx, "limit")
    six = pg.rollout(plan=plan, seed=5, row_ids=ids)
    perm = np.array([4, 2, 5, 0, 3, 1])
    shuf = pg.rollout(plan=plan, seed=5, row_ids=ids[perm])
    for k in PR.FRAME_KEYS:
        assert torch.equal(getattr(shuf, k), getattr(six, k)[perm]), k
    assert torch.equal(shuf.final_frame, six.final_frame[perm])
    set_scene(pg, fx, "limit", rows=1)
    one = pg.rollout(plan=plan, seed=5, row_ids=ids[2:3])
    assert one.windows == six.windows
    for k in PR.FRAME_KEYS:
        assert torch.equal(getattr(one, k)[0], getattr(six, k)[2]), k
    # x_T of window 1 of row id 250000: feed draw_noise at the key as injected noise, the same bits come out
    xT = torch.stack([gen.draw_noise(1, 5, pg.window_key(ids[2], w)) for w in range(one.windows)])
    inj = pg.rollout(plan=plan, noise=xT)
    for k in PR.FRAME_KEYS:
        assert torch.equal(getattr(inj, k), getattr(one, k)), k
    assert not torch.equal(six.root_pos[0], six.root_pos[1])
    # a start drawn on the device (relative root height, random heading) follows the path's id, not its place in the scene
    hf, mp = fx.terrain("limit")
    pa, pb = fx.raw("limit/path"), fx.raw("limit/path")[::-1].copy()
    pg.set_scene(np.stack([hf, hf]), np.stack([mp, mp]), fx.dx, [pa, pb], 2)
    ab = pg.rollout(seed=5, row_ids=[0, 1, 2, 3], path_ids=[70001, 9], heading_mode="random")
    pg.set_scene(np.stack([hf, hf]), np.stack([mp, mp]), fx.dx, [pb, pa], 2)
    ba = pg.rollout(seed=5, row_ids=[2, 3, 0, 1], path_ids=[9, 70001], heading_mode="random")
    assert torch.equal(ab.root_pos[:2], ba.root_pos[2:]) and torch.equal(ab.root_rot[2:], ba.root_rot[:2])
    other = pg.rollout(seed=5, row_ids=[2, 3, 0, 1], path_ids=[10, 70001], heading_mode="random")
    assert not torch.equal(other.root_pos[0, 0], ba.root_pos[0, 0])


def test_selection(pgs, fx, rollouts):
    """``select`` on the rollouts of the limit and the mixed record against the reference's recorded sort with the recorded noise; in
    the mixed record three rows finished and three carry the penalty."""
    for rec in ("limit", "mixed"):
        pg = handle(pgs, fx, rec)
        res = rollouts[rec][0]
        sel = pg.select(res, top_k=6, noise=fx.loss_noise)[0]
        order = fx.raw(f"{rec}/sel_order")
        assert np.array_equal(sel["rows"], order), (sel["rows"], order)
        for k, key in (("total_loss", "sel_total"), ("contact_loss", "sel_contact"), ("pen_loss", "sel_pen")):
            want = fx.raw(f"{rec}/{key}")[order]
            print(rec, k, "got", sel[k], "want", want)
            assert np.all(np.abs(sel[k] - want) <= 1e-5 * np.abs(want) + 1e-6), (rec, k, sel[k], want)
        assert (fx.raw(f"{rec}/sel_total") > 50).any()             # the unfinished-row penalty is in the record
        top = pg.select(res, top_k=2, noise=fx.loss_noise)[0]
        assert np.array_equal(top["rows"], order[:2])
    tot = fx.raw("mixed/sel_total")
    assert (tot > 50).sum() == 3 and (tot < 50).sum() == 3 and set(fx.raw("mixed/sel_order")[:3].tolist()) == {0, 1, 2}
    assert not np.array_equal(fx.raw("mixed/sel_order"), np.argsort(fx.loss_noise))   # the order is the losses', not the noise's


def test_library_refusals(pg, fx, gen):
    """What ``parc_mpath_*`` itself refuses, each naming its argument."""
    from parc_amd import lib as L
    hf, mp = fx.terrain("limit")
    path = fx.raw("limit/path")
    with pytest.raises(L.ParcError, match="max_batch"):
        pg.set_scene(hf[None], mp[None], fx.dx, [path], gen.max_batch + 1)
    with pytest.raises(L.ParcError, match="nodes"):
        pg.set_scene(hf[None], mp[None], fx.dx, [path[:1]], 2)
    bad = path.copy()
    bad[5, 1] = np.inf
    with pytest.raises(L.ParcError, match="non-finite node"):
        pg.set_scene(hf[None], mp[None], fx.dx, [bad], 2)
    nan_hf = hf.copy()
    nan_hf[3, 3] = np.nan
    with pytest.raises(L.ParcError, match="height"):
        pg.set_scene(nan_hf[None], mp[None], fx.dx, [path], 2)
    with pytest.raises(L.ParcError, match="dx"):
        pg.set_scene(hf[None], mp[None], 0.0, [path], 2)
    row_path = np.array([0, 1], np.int32)
    packed, counts = np.ascontiguousarray(path[None]), np.array([len(path)], np.int32)
    with pytest.raises(L.ParcError, match="row_path"):
        pg._call("set_scene", L.np_f32p(hf), 1, hf.shape[0], hf.shape[1], L.np_f32p(mp), fx.dx, fx.dx, L.np_f32p(packed), L.np_i32p(counts), len(path),
                 L.np_i32p(row_path), 2)
    set_scene(pg, fx, "limit")
    with pytest.raises(L.ParcError, match="row_ids"):
        pg.rollout(seed=0, plan={"rel_height": torch.tensor([0.8])}, row_ids=[0, 1, 2, 3, 4, 1 << 28])
    with pytest.raises(L.ParcError, match="noise"):
        pg.rollout(plan={"rel_height": torch.tensor([0.8])}, noise=torch.zeros((1, 6, pg.T, pg.D)))


def test_script_smoke(tmp_path):
    """``generate_path_motions.py --random_init 0`` on two 16 x 16 batches that ``TerrainPathPlanner`` wrote: files appear, reload and
    have ``final_frame`` frames."""
    import json
    from parc_amd import ms_file
    from parc_amd import path_planner as pp
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    planner = pp.TerrainPathPlanner(DEV)
    (tmp_path / "paths").mkdir()
    rng = np.random.RandomState(4)
    for b in range(2):
        hfs = (np.kron(rng.randint(0, 3, (2, 4, 4)), np.ones((4, 4))) * 0.2).astype(np.float32)
        attempt, plan = planner.plan_terrains(hfs, num_attempts=6, seed=b, dx=0.4, dy=0.4)
        points = [p if a >= 0 else p[:0] for p, a in zip(plan.points, attempt)]
        assert (attempt >= 0).any()
        np.savez_compressed(tmp_path / "paths" / f"paths_{b:04d}.npz", hf=plan.hf, min_point_offset=np.array([[1.5, -2.0], [0.0, 0.0]], np.float32),
                            dx=np.float32(0.4), points=np.concatenate(points), point_off=np.concatenate([[0], np.cumsum([len(p) for p in points])]).astype(np.int64))
    out = tmp_path / "motions"
    run = subprocess.run([sys.executable, os.path.join(REPO, "scripts", "generate_path_motions.py"), "--paths", str(tmp_path / "paths"), "--out", str(out),
                          "--random_init", "0", "--candidates", "3", "--top_k", "2", "--max_motion_length", "1.0", "--max_batch", "4", "--seed", "3"],
                         env=env, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    line = json.loads(run.stdout.strip().splitlines()[-1])
    assert line["paths"] >= 1 and line["rows"] == 3 * line["paths"] and line["windows"] >= 2
    files = sorted(os.listdir(out))
    assert len(files) == 2 * line["paths"] and all(f.startswith("path_") and f.endswith(".pkl") for f in files)
    for f in files:
        d = ms_file.load_ms_file(str(out / f))
        n = d.motion_data.root_pos.shape[0]
        assert n == d.misc_data["num_frames"] and d.terrain_data.hf.shape == (16, 16)
        assert d.misc_data["final_frame"] in (-1, n)
