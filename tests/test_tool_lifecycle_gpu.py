"""The life of a tool handle on the GPU, at the smallest inputs that reach each path: what ``kernel_times`` answers before and after a
run, the state guards (``set_clips first`` / ``run first``), a refused batch that leaves the loaded one in place, and a second
``set_clips`` that gives the results of its batch alone.  What the kernels compute is the business of each tool's own test file.

The clip tools (``parc_mopt_*``, ``parc_mterr_*``, ``parc_medit_*``, ``parc_msamp_*``, ``parc_maug_*``) go through every step; the
tools without a batch (``parc_tgen_*``, ``parc_pathplan_*``, ``parc_mdm_*``, ``parc_mpath_*``, ``parc_mloss_*``) through their timings."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import motion_opt_cases as M
from parc_amd import lib as L
from parc_amd import motion_aug as ma
from parc_amd import motion_edit as me
from parc_amd import motion_generator as mg
from parc_amd import motion_loss as ML
from parc_amd import motion_opt as mo
from parc_amd import motion_path_gen as mpg
from parc_amd import motion_sampler as ms
from parc_amd import motion_terrain as mt
from parc_amd import path_planner as pp
from parc_amd import terrain_gen as tg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def small_clip(f0, n):
    """n frames of the civilization fixture on a 4 x 4 cut of its heightfield (the cells stay where they are)."""
    _, clip = M.window(M.fixture(M.CIVILIZATION), "b", f0, f0 + n)
    xs = ys = slice(4, 8)
    mp = (clip.min_point[:2] + np.array([xs.start, ys.start], np.float32) * np.float32(clip.dx)).astype(np.float32)
    return M.copy_clip(clip, hf=np.ascontiguousarray(clip.hf[xs, ys]), min_point=mp)


A, B = small_clip(20, 3), small_clip(30, 5)


def clips_struct(tool, clips, break_dims=False):
    pk = mo.pack_clips(clips, tool.B, tool.char_model.get_dof_size())
    if break_dims:
        pk["hf_dims"][0, 0] += 1                                # 5 x 4 cells against an offset of 16
    return pk, mo.clip_struct(pk, len(clips))


def raises(tool, text, name, *args):
    with pytest.raises(L.ParcError) as e:
        tool._call(name, *args)
    assert str(e.value).endswith(text), str(e.value)


def same(x, y):
    """bit-equal, NaNs included (a clip of three frames has no jerk window)"""
    return x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()


def check_times(times, kernels, ran):
    assert tuple(times) == tuple(kernels)
    for k, v in times.items():
        assert math.isfinite(v) and v >= 0.0, (k, v)
        assert (v > 0.0) == (k in ran), (k, v, ran)


# ---- the optimiser -------------------------------------------------------------------------------------------------------------------
def opt_eval(o):
    t, g = o.loss_and_grad()
    return t.copy(), g.copy(), o.get_params().copy()


def test_mopt_lifecycle():
    o = mo.MotionOptimizer(M.CHAR, DEV, M.one_hot(M.SMOOTH))
    assert o.kernel_times() == dict.fromkeys(mo.KERNELS, 0.0)
    for name, args in (("set_constraint_points", (None,)), ("set_params", (None,)), ("get_params", (None,)), ("loss_and_grad", (None, None)),
                       ("step", (1, None)), ("get_frames", (None, None, None)), ("get_source_body", (None, None)),
                       ("build_constraints", (0, None, None, 0, C.c_float(0.0)))):
        raises(o, "mopt: parc_mopt_set_clips first", name, *args)
    o.set_clips([A, B])
    kept = opt_eval(o)
    _, bad = clips_struct(o, [B], break_dims=True)
    raises(o, "mopt: heightfield dims / offsets disagree", "set_clips", C.byref(bad))
    again = opt_eval(o)
    assert all(same(x, y) for x, y in zip(kept, again))
    o.step(1)
    check_times(o.kernel_times(), mo.KERNELS, mo.KERNELS)
    o.set_clips([B])                                            # a second batch: its results alone
    fresh = mo.MotionOptimizer(M.CHAR, DEV, M.one_hot(M.SMOOTH))
    fresh.set_clips([B])
    assert all(same(x, y) for x, y in zip(opt_eval(o), opt_eval(fresh)))


# ---- the analyser ----------------------------------------------------------------------------------------------------------------------
def terr_run(a, b):
    """b: (clips, frames, cells) of the loaded batch"""
    out, counts, maxmin, total = np.zeros((b[0], len(mt.CLIP_OUTPUTS)), np.float32), np.zeros(b[1], np.int32), np.zeros((b[2], 2), np.float32), C.c_int64()
    a._call("run", L.np_f32p(out), L.np_i32p(counts), L.np_f32p(maxmin), C.byref(total))
    inds = np.zeros((int(total.value), 2), np.int32)
    a._call("get_mask_inds", L.np_i32p(inds) if inds.size else None)
    return out, counts, maxmin, inds


def test_mterr_lifecycle():
    a = mt.MotionTerrainAnalyzer(M.CHAR, DEV)
    a._handle(mt.Z_BUF, mt.JUMP_BUF, mt.MAX_JERK)
    assert a.kernel_times() == dict.fromkeys(mt.KERNELS, 0.0)
    raises(a, "mterr: parc_mterr_set_clips first", "run", None, None, None, None)
    for name, args in (("get_mask_inds", (None,)), ("get_min_heights", (None, None)), ("point_sdf", (0, 1, None, None))):
        raises(a, "mterr: parc_mterr_set_clips first", name, *args)
    pk, st = clips_struct(a, [A, B])
    a._call("set_clips", C.byref(st))
    for name, args in (("get_mask_inds", (None,)), ("get_min_heights", (None, None)), ("point_sdf", (0, 1, None, None))):
        raises(a, "mterr: parc_mterr_run first", name, *args)
    sizes = (2, int(pk["frame_off"][-1]), int(pk["hf_off"][-1]))
    kept = terr_run(a, sizes)
    times = a.kernel_times()
    check_times(times, mt.KERNELS, [k for k in mt.KERNELS if k != mt.KERNELS[5] or kept[3].size])
    _, bad = clips_struct(a, [B], break_dims=True)
    raises(a, "mterr: heightfield dims / offsets disagree (dims >= 1, at most 2^31 - 1 cells)", "set_clips", C.byref(bad))
    assert all(same(x, y) for x, y in zip(kept, terr_run(a, sizes)))
    second = a.run([B])                                         # a second batch: its results alone
    fresh = mt.MotionTerrainAnalyzer(M.CHAR, DEV).run([B])
    for k in ("clip_out", "counts", "inds", "hf_maxmin"):
        assert same(second[k], fresh[k]), k


# ---- the hesitation remover ----------------------------------------------------------------------------------------------------------------
def edit_run(e, C_, F):
    counts, kept, total = np.zeros(C_, np.int32), np.zeros(F, np.int32), C.c_int64()
    e._call("run", L.np_i32p(counts), L.np_i32p(kept), C.byref(total))
    n, J = int(total.value), e.B - 1
    rp, rr, jr, ct = np.zeros((n, 3), np.float32), np.zeros((n, 4), np.float32), np.zeros((n, J, 4), np.float32), np.zeros((n, e.B), np.float32)
    e._call("get_frames", L.np_f32p(rp), L.np_f32p(rr), L.np_f32p(jr), L.np_f32p(ct))
    return counts, kept, rp, rr, jr, ct


def test_medit_lifecycle():
    e = me.HesitationRemover(M.CHAR, DEV)
    assert e.kernel_times() == dict.fromkeys(me.KERNELS, 0.0)
    getters = (("get_frames", (None, None, None, None)), ("get_pair_rows", (0, None)), ("get_flags", (None, None)))
    for name, args in (("run", (None, None, None)),) + getters:
        raises(e, "medit: parc_medit_set_clips first", name, *args)
    pk, st = clips_struct(e, [A, B])
    e._call("set_clips", C.byref(st))
    for name, args in getters:
        raises(e, "medit: parc_medit_run first", name, *args)
    kept = edit_run(e, 2, int(pk["frame_off"][-1]))
    check_times(e.kernel_times(), me.KERNELS, me.KERNELS)
    T = me.MAX_FRAMES + 1
    long_clip = M.copy_clip(A, root_pos=np.repeat(A.root_pos[:1], T, 0), root_rot=np.repeat(A.root_rot[:1], T, 0),
                            joint_rot=np.repeat(A.joint_rot[:1], T, 0), contacts=np.repeat(A.contacts[:1], T, 0))
    _, bad = clips_struct(e, [long_clip])
    with pytest.raises(L.ParcError, match=rf"medit: clip 0 has {T} frames; at most {T - 1} are supported"):
        e._call("set_clips", C.byref(bad))
    assert all(same(x, y) for x, y in zip(kept, edit_run(e, 2, int(pk["frame_off"][-1]))))
    second = e.run([B])                                         # a second batch: its results alone
    fresh = me.HesitationRemover(M.CHAR, DEV).run([B])
    for k in ("counts", "kept", "root_pos", "root_rot", "joint_rot", "contacts"):
        assert same(second[k], fresh[k]), k


# ---- the augmenter ---------------------------------------------------------------------------------------------------------------------------
def aug_plan(g, n):
    return g.plan_from_numpy(dict(src_clip=np.zeros(n, np.int32), start_frame=np.zeros(n, np.int32), num_frames=np.full(n, 3, np.int32)))


def aug_set_clips(g, clips, break_dims=False):
    """parc_maug_set_clips as the wrapper's constructor calls it (these clips carry no hf_maxmin)"""
    pk, st = clips_struct(g, clips, break_dims)
    info = L.ParcMotionAugClipInfo()
    fps = np.array([int(c.fps) for c in clips], np.int32)
    win = np.array([int(round(int(c.fps) * float(g.settings.max_motion_len))) for c in clips], np.int32)
    info.fps_host, info.max_frames_host = L.np_i32p(fps), L.np_i32p(win)
    g._call("set_clips", C.byref(st), C.byref(info))


AUG_OUT = ("frame_off", "cell_off", "src_clip", "hf_dims", "hf_geom", "canon_z", "root_pos", "root_rot", "joint_rot", "contacts", "hf")


def test_maug_lifecycle():
    g = ma.MotionAugmenter(M.CHAR, [A, B])
    raises(g, "maug: nothing augmented yet", "kernel_times", L.np_f32p(np.zeros(4, np.float32)))
    kept = g.augment_with(aug_plan(g, 2))
    torch.cuda.synchronize()
    check_times(g.kernel_times(), ma.KERNELS, ma.KERNELS[1:])  # no draw
    assert g.status() == 0 and g.status() == 0
    with pytest.raises(L.ParcError, match="maug: heightfield dims / offsets disagree$"):
        aug_set_clips(g, [B], break_dims=True)
    again = g.augment_with(aug_plan(g, 2))                      # the library of [A, B] is still loaded
    for k in AUG_OUT:
        assert torch.equal(getattr(kept, k), getattr(again, k)), k
    g.draw_plan(2, seed=3)
    check_times(g.kernel_times(), ma.KERNELS, ma.KERNELS)
    aug_set_clips(g, [B])                                       # a second library: its results alone
    second, fresh = g.augment_with(aug_plan(g, 2)), ma.MotionAugmenter(M.CHAR, [B]).augment_with(aug_plan(g, 2))
    for k in AUG_OUT:
        assert torch.equal(getattr(second, k), getattr(fresh, k)), k


def test_maug_needs_its_clips(monkeypatch):
    call = ma.MotionAugmenter._call                              # a handle whose constructor loads nothing
    monkeypatch.setattr(ma.MotionAugmenter, "_call", lambda self, name, *a: None if name == "set_clips" else call(self, name, *a))
    g = ma.MotionAugmenter(M.CHAR, [A, B])
    monkeypatch.undo()
    st, _ = g._plan_struct(aug_plan(g, 2))
    sizes, u64 = L.ParcMotionAugSizes(), C.c_uint64
    for name, args in (("draw_plan", (u64(1), u64(0), 0, C.byref(st), g._stream())), ("augment_with", (C.byref(st), 0, g._stream(), C.byref(sizes))),
                       ("augment", (2, u64(1), u64(0), 0, g._stream(), C.byref(sizes)))):
        raises(g, "maug: parc_maug_set_clips first", name, *args)
    aug_set_clips(g, [A, B])
    assert g.augment_with(aug_plan(g, 2)).n == 2


# ---- the window sampler ------------------------------------------------------------------------------------------------------------------------
def bare_sampler(tmp_path_factory):
    """The sampler of the rect_root fixture over the two bundled clips, its handle made anew and nothing loaded (the sampler reads
    whole windows, so the clips of 3 and 5 frames are too short for it)."""
    import warnings
    from test_motion_sampler_gpu import fixture
    from test_motion_sampler_shapes_gpu import make_sampler
    z = fixture("rect_root")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        s = make_sampler(z["cfg"], (0, 0), tmp_path_factory)
    s._destroy()
    s._create()
    return s, z


def test_msamp_lifecycle(tmp_path_factory, monkeypatch):
    from test_motion_sampler_gpu import bits_equal, outputs, plan_of
    s, z = bare_sampler(tmp_path_factory)
    raises(s, "msamp: nothing sampled yet", "kernel_times", L.np_f32p(np.zeros(3, np.float32)))
    plan = s.plan_from_numpy(plan_of(z))
    st, n = s._plan_struct(plan)
    full, _ = s._plan_struct(s.empty_plan(n))
    (_, ost), (_, mst), u64 = s._outputs(n, True), s._outputs(1, False), C.c_uint64
    for name, args in (("sample_with", (C.byref(st), C.byref(ost), s._stream())), ("draw_plan", (u64(1), C.byref(full), s._stream())),
                       ("sample", (u64(1), C.byref(full), C.byref(ost), s._stream())), ("enumerate", (0, C.byref(mst), s._stream()))):
        raises(s, "msamp: parc_msamp_set_clips first", name, *args)
    s._upload()
    kept = outputs(s.sample_with(plan))
    times = s.kernel_times()
    check_times({k: times[k] for k in ms.KERNELS[1:]}, ms.KERNELS[1:], ms.KERNELS[1:])
    assert tuple(times) == ms.KERNELS and math.isfinite(times["draw"]) and times["draw"] >= 0.0   # two events with nothing between them
    status = C.c_int32(-1)
    for _ in range(2):
        s._call("plan_status", s._stream(), C.byref(status))
        assert status.value == 0
    pack = mo.pack_clips

    def broken(*a):
        pk = pack(*a)
        pk["hf_dims"][0, 0] += 1
        return pk

    monkeypatch.setattr(mo, "pack_clips", broken)
    with pytest.raises(L.ParcError, match="msamp: heightfield dims / offsets disagree$"):
        s._upload()
    monkeypatch.undo()
    assert bits_equal(kept, outputs(s.sample_with(plan)))       # the library is still loaded
    s.sample(4, seed=2)
    check_times(s.kernel_times(), ms.KERNELS, ms.KERNELS)
    s.clips, s.extra_vals = s.clips[:1], s.extra_vals[:1]      # a second library: its results alone
    s._upload()
    drawn = s.draw_plan(4, seed=5)
    fresh, _ = bare_sampler(tmp_path_factory)
    fresh.clips, fresh.extra_vals = fresh.clips[:1], fresh.extra_vals[:1]
    fresh._upload()
    assert bits_equal(outputs(s.sample_with(drawn)), outputs(fresh.sample_with(drawn)))


# ---- the generator, the path rollout and the loss --------------------------------------------------------------------------------------------
def test_mdm_and_mpath_times():
    from test_mdm_gpu import TS3, Case, small_cfg
    case = Case(small_cfg(), 6, 10)
    gen = case.gen
    raises(gen, "mdm: nothing sampled yet", "kernel_times", L.np_f32p(np.zeros(3, np.float32)))
    gen.ddim_inference(dict(case.dev(case.c()), timesteps=TS3), case.x.to(DEV), 10, guidance_scale=1.5)
    torch.cuda.synchronize()
    check_times(gen.kernel_times(), mg.KERNELS, mg.KERNELS)
    pg = mpg.PathMotionGenerator(gen, mpg.MDMPathSettings(max_motion_length=1.0), mpg.MDMGenSettings(ddim_stride=10))
    raises(pg, "mpath: no rollout yet", "kernel_times", L.np_f32p(np.zeros(2, np.float32)))
    pg.set_scene(np.zeros((1, 16, 16), np.float32), np.zeros((1, 2), np.float32), 0.4, [np.array([[1.0, 1.0, 0.0], [4.0, 4.0, 0.0]], np.float32)], 2)
    res = pg.rollout(plan={"rel_height": torch.tensor([0.9])}, seed=1)
    torch.cuda.synchronize()
    assert res.windows >= 2
    check_times(pg.kernel_times(), mpg.KERNELS, mpg.KERNELS)


def test_mloss_times():
    import mdm_loss_ref as LR
    fx = LR.LossFixture(M.os.path.join(M.REPO, "tests/golden"))
    pred, true, td, mean, std = fx.inputs("a")
    loss = ML.MotionLoss(fx.cfg("a"), DEV, "squared_l2", mean, std)
    raises(loss, "mloss: nothing evaluated yet", "kernel_times", L.np_f32p(np.zeros(1, np.float32)))
    terms, grad = loss.terms_and_grad(pred[:1, :2].contiguous().to(DEV), {k: v[:1, :2].contiguous().to(DEV) for k, v in true.items()}, td[:1].to(DEV))
    torch.cuda.synchronize()
    assert terms.shape[0] == 1 and grad.shape[:2] == (1, 2)
    check_times(loss.kernel_times(), ML.KERNELS, ML.KERNELS)


# ---- the generator and the planner -------------------------------------------------------------------------------------------------------------
def test_tgen_times():
    g = tg.TerrainGenerator("BOXES", dim_x=4, dim_y=4, settings=tg.BoxesSettings(num_boxes=2), device=DEV)
    raises(g, "tgen: nothing generated yet", "kernel_times", L.np_f32p(np.zeros(2, np.float32)))
    g.generate_with(g.empty_plan(2), validate=True)
    torch.cuda.synchronize()
    check_times(g.kernel_times(), tg.KERNELS, tg.KERNELS[1:])  # no draw
    g.draw_plan(2, seed=1)
    check_times(g.kernel_times(), tg.KERNELS, tg.KERNELS)


def test_pathplan_times():
    p = pp.TerrainPathPlanner(DEV)
    hfs = np.zeros((2, 4, 4), np.float32)
    p._handle(4, 4, 0.4, 0.4)
    raises(p, "pathplan: nothing planned yet", "kernel_times", L.np_f32p(np.zeros(3, np.float32)))
    p.plan(hfs, seed=1)
    check_times(p.kernel_times(), pp.KERNELS, pp.KERNELS[:2])  # no graph
