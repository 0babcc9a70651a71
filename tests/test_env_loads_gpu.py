"""-m gpu: parc_env_load_motions / parc_env_load_terrain replace the handle's state atomically (include/parc_env.h).

  * a rejected load (a clip of one frame in a set of another M; a terrain with dx = 0, or with rows for another M) changes nothing: motion
    info and fail rates read back bit-equal, and the handle then computes bit for bit what a twin that never saw the call computes,
    through parc_env_step and through the captured graph of parc_env_step_reset_graph;
  * a reload with another M needs the terrain again (PARC_ERR_STATE until then, fail rates back at 1) and afterwards equals a fresh handle.
8 envs, dynamics off, explicit reset samples (no RNG state is involved); every comparison is of bytes."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
N = 8
ERR_INVALID, ERR_STATE = -1, -3
BOUND = ["_char_root_pos", "_char_root_rot", "_char_root_vel", "_char_root_ang_vel", "_char_dof_pos", "_char_dof_vel", "_char_rigid_body_pos",
         "_char_contact_forces", "_motion_ids", "_motion_terrain_ids", "_motion_time_offsets", "_timestep_buf", "_time_buf", "_ep_num_buf",
         "_obs_buf", "_reward_buf", "_done_buf", "_reward_terms", "_ref_root_pos", "_ref_root_rot", "_ref_root_vel", "_ref_root_ang_vel",
         "_ref_joint_rot", "_ref_dof_pos", "_ref_dof_vel", "_ref_body_pos", "_ref_contacts", "_ray_hfs"]


def _env(tmp_path, sub, clips, weights):
    from gpu_helpers import default_config, write_motion_yaml
    from parc_amd.envs.hip_parkour_env import HipParkourEnv
    d = tmp_path / sub
    d.mkdir(exist_ok=True)
    cfg = default_config()
    cfg["env"]["dm"]["motion_file"] = write_motion_yaml(d, clips, weights)
    return HipParkourEnv(cfg, N, "cuda:0", False)


def _load_motions(env, packed, num_motions, num_frames=None):
    """parc_env_load_motions with the first `num_motions` clips of a packed set (their frames are a prefix of every array)."""
    from parc_amd import lib as L
    nf = np.ascontiguousarray(packed["num_frames"][:num_motions] if num_frames is None else num_frames, np.int32)
    mc = L.ParcMotionClips()
    mc.num_motions = num_motions
    mc.num_frames_host = L.np_i32p(nf); mc.fps_host = L.np_i32p(packed["fps"])
    mc.loop_modes_host = L.np_i32p(packed["loop_modes"]); mc.weights_host = packed["weights"].ctypes.data_as(L.f64p)
    mc.root_pos_host = L.np_f32p(packed["root_pos"]); mc.root_rot_host = L.np_f32p(packed["root_rot"])
    mc.joint_rot_host = L.np_f32p(packed["joint_rot"]); mc.contacts_host = L.np_f32p(packed["contacts"])
    return env._lib.parc_env_load_motions(env._handle, C.byref(mc))


def _load_terrain(env, grid, dx=None, M=None):
    from parc_amd import lib as L
    hf = np.ascontiguousarray(grid.terrain.hf, np.float32)
    mo = np.ascontiguousarray(grid.motion_offsets, np.float32)
    return env._lib.parc_env_load_terrain(env._handle, L.np_f32p(hf), hf.shape[0], hf.shape[1], float(grid.terrain.min_point[0]),
                                          float(grid.terrain.min_point[1]), float(grid.terrain.dxdy[0]) if dx is None else dx,
                                          float(grid.terrain.dxdy[1]), L.np_f32p(mo), mo.shape[0] if M is None else M, mo.shape[1])


def _motion_state(env, M):
    """(lengths, weights, fail rates) of the handle, as bytes."""
    from parc_amd import lib as L
    lengths = np.full(M, -1, np.float32); weights = np.full(M, -1, np.float32); fail = np.full(M, -1, np.float32)
    L.check(env._lib.parc_env_get_motion_info(env._handle, L.np_f32p(lengths), L.np_f32p(weights), M))
    L.check(env._lib.parc_env_get_fail_rates(env._handle, L.np_f32p(fail), M))
    return lengths.tobytes(), weights.tobytes(), fail.tobytes()


def _reset_and_step(env, M, steps=3):
    import torch
    i = torch.arange(N)
    lengths = env._motion_lengths.cpu()
    mids = (i % M).int()
    env.reset_with(i, mids, torch.zeros(N, dtype=torch.int32), (0.05 + 0.1 * i.float()) * lengths[mids.long()],
                   0.01 * torch.stack([i.float(), -i.float()], dim=1))
    for _ in range(steps):
        env.step(None)


def _same(a, b, names):
    import torch
    torch.cuda.synchronize()
    for k in names:
        x, y = getattr(a, k).cpu().numpy(), getattr(b, k).cpu().numpy()
        assert x.tobytes() == y.tobytes(), k
    assert np.isfinite(a._obs_buf.cpu().numpy()).all() and a._obs_buf.abs().sum() > 0


@pytest.mark.parametrize("what", ["motions_one_frame_clip", "terrain_dx_zero", "terrain_other_M"])
def test_a_rejected_load_changes_nothing(tmp_path, what):
    from gpu_helpers import GOLDEN_WEIGHTS
    from helpers import CLIPS4
    from parc_amd import lib as L
    a, b = (_env(tmp_path, s, CLIPS4, GOLDEN_WEIGHTS) for s in ("a", "b"))
    M = 4
    for e in (a, b):
        e.set_fail_rates([0.25, 0.5, 0.75, 0.125])
    before = _motion_state(a, M)

    def rejected():
        if what == "motions_one_frame_clip":      # another M, and the LAST clip is the bad one: every earlier clip was accepted
            nf = a._scene.packed["num_frames"][:3].copy(); nf[2] = 1
            assert _load_motions(a, a._scene.packed, 3, nf) == ERR_INVALID
            assert L.load().parc_last_error().decode() == "every clip needs at least 2 frames"
        elif what == "terrain_dx_zero":
            assert _load_terrain(a, a._scene.grid, dx=0.0) == ERR_INVALID
        else:
            assert _load_terrain(a, a._scene.grid, M=3) == ERR_STATE
        assert _motion_state(a, M) == before == _motion_state(b, M)

    rejected()
    for e in (a, b):
        _reset_and_step(e, M)
    _same(a, b, ["_obs_buf", "_reward_buf", "_done_buf"])
    # the graph step: captured once, then replayed after another rejected call (a replay uses the pointers the capture recorded)
    for e in (a, b):
        L.check(e._lib.parc_env_set_never_done(e._handle, 1))
        e.step_and_reset_done(None)
    _same(a, b, ["_obs_buf", "_reward_buf", "_done_buf"])
    rejected()
    for e in (a, b):
        e.step_and_reset_done(None)
    _same(a, b, ["_obs_buf", "_reward_buf", "_done_buf"])


def test_a_reload_equals_a_fresh_handle(tmp_path):
    import torch
    from helpers import CLIPS4
    from parc_amd import lib as L
    from parc_amd.envs import scene as scene_mod
    from gpu_helpers import default_config, write_motion_yaml
    s2 = [CLIPS4[1], CLIPS4[2]]
    a, b = (_env(tmp_path, s, s2, [1.0, 2.0]) for s in ("a", "b"))        # both from S2's config: the env offsets agree
    (tmp_path / "s1").mkdir()
    cfg1 = default_config()
    cfg1["env"]["dm"]["motion_file"] = write_motion_yaml(tmp_path / "s1", [CLIPS4[0], CLIPS4[2], CLIPS4[3]], [1.5, 1.0, 0.5])
    sc1, sc2 = scene_mod.build_scene(cfg1, N, 0, enable_dynamics=False, verbose=False), a._scene
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    step = lambda: a._lib.parc_env_step(a._handle, None, st)
    # S1 on A: the motions alone leave it without a terrain (M 2 -> 3), then the terrain, one step
    assert _load_motions(a, sc1.packed, 3) == 0
    assert step() == ERR_STATE
    assert _load_terrain(a, sc1.grid) == 0
    assert step() == 0
    fr1 = np.ascontiguousarray([0.25, 0.5, 0.75], np.float32)
    L.check(a._lib.parc_env_set_fail_rates(a._handle, L.np_f32p(fr1), 3))
    # S2 on A
    assert _load_motions(a, sc2.packed, 2) == 0
    assert step() == ERR_STATE
    assert L.load().parc_last_error().decode() == "bind_buffers, load_motions and load_terrain must precede this call"
    assert _motion_state(a, 2) == _motion_state(b, 2)
    assert np.frombuffer(_motion_state(a, 2)[2], np.float32).tolist() == [1.0, 1.0]
    assert _load_terrain(a, sc2.grid) == 0
    # a reload with the same M keeps the terrain
    assert _load_motions(a, sc2.packed, 2) == 0
    for e in (a, b):
        _reset_and_step(e, 2)
    _same(a, b, BOUND + (["_tracking_error"] if a._tracking_error is not None else []))
