"""-m gpu: the row phase of k_env_post after its re-mapping to items (parc_rowmap.hpp: every root item and 48 joint items in pass A, joint
items only in pass B), on the golden scenes of tests/test_hip_parity.py with the same helpers and tolerances, at env counts that leave a
workgroup of four waves partly empty (1, 3, 5: a last block of one wave; 6: block 1 with two waves, whose reward owner is wave 1).  The env
is built as the first n envs of the reference's 64 (``total_envs=64``: same env origins), so rows [0, n) of the golden outputs apply."""
import numpy as np
import pytest

from conftest import golden

pytestmark = pytest.mark.gpu
TOL = 1e-5
COUNTS = [1, 3, 5, 6]
# scene -> (config overrides, mirror_ref_state, observation width).  Targets off (`enable_tar_obs: false`): rows = 2, every item in pass A;
# targets on: 8 rows, the joint items of rows 3.. spill into pass B
SCENES = {
    "env_step": ({}, True, 1312),
    "env_step_global_obs": ({"global_obs": True}, False, 1312),
    "env_step_local_root": ({"track_root": False}, False, 1312),
    "env_step_root_height_obs": ({"global_root_height_obs": True}, False, 1313),
    "env_step_obs_blocks_c0_t0": ({"use_contact_info": False, "enable_tar_obs": False}, False, 577),
    "env_step_obs_blocks_c0_t1": ({"use_contact_info": False, "enable_tar_obs": True}, False, 1207),
    "env_step_obs_blocks_c1_t0": ({"use_contact_info": True, "enable_tar_obs": False}, False, 592),
}


def _env(tmp_path, n, overrides, mirror):
    from gpu_helpers import default_config, write_motion_yaml, GOLDEN_WEIGHTS
    from parc_amd.envs.hip_parkour_env import HipParkourEnv
    cfg = default_config()
    cfg["env"]["dm"]["motion_file"] = write_motion_yaml(tmp_path, [str(c) for c in golden("env_step")["clips"]], GOLDEN_WEIGHTS)
    cfg["env"]["hip"]["body_pos_from_fk"] = False
    cfg["env"].update(overrides)
    return HipParkourEnv(cfg, n, "cuda:0", False, total_envs=64, mirror_ref_state=mirror)


def _inject(env, g, prefix, n):
    """gpu_helpers.inject for the first n of the golden's 64 envs."""
    import torch
    from gpu_helpers import _IN
    for gk, attr in _IN.items():
        t = getattr(env, attr)
        t.copy_(torch.from_numpy(np.ascontiguousarray(g[prefix + gk][:n])).to(t.dtype).to(t.device))
    env.set_fail_rates(g[prefix + "fail_rates"])


def _check_obs(obs, ref, hf0):
    """test_hip_parity's observation check: 1e-5, height samples that a 1-ulp difference moves across a cell edge set aside.  The 64-env
    fixture allows a fraction of 2e-4 of its 64 x 441 samples, i.e. 5 samples; all of them may lie in the rows checked here, so the same
    count bounds a subset of the rows."""
    err = np.abs(obs - ref)
    ray_bad = np.abs(obs[:, hf0:] - ref[:, hf0:]) > TOL
    err[:, hf0:][ray_bad] = 0
    assert ray_bad.sum() < 2e-4 * 64 * 441 and err.max() <= TOL, (ray_bad.sum(), err.max(), np.unravel_index(err.argmax(), err.shape))


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("scene", list(SCENES))
def test_golden_scenes_at_small_env_counts(tmp_path, scene, n):
    import torch
    from gpu_helpers import to_np
    overrides, mirror, width = SCENES[scene]
    g = golden(scene)
    env = _env(tmp_path, n, overrides, mirror)
    assert env._obs_buf.shape == (n, width)
    hf0 = width - 441
    steps = [("s%d_in_" % s, "s%d_out_" % s) for s in range(3)] if scene == "env_step" else [("in_", "out_")]
    if "reset_obs" in g.files and scene != "env_step":   # the observation pass on the reference's reset state (MODE_OBS instantiation)
        _inject(env, g, "reset_", n)
        env._compute_obs()
        torch.cuda.synchronize()
        _check_obs(to_np(env._obs_buf), g["reset_obs"][:n], hf0)
    for pin, pout in steps:
        _inject(env, g, pin, n)
        env.step(None)
        _check_obs(to_np(env._obs_buf), g[pout + "obs"][:n], hf0)
        assert np.array_equal(to_np(env._done_buf), g[pout + "done"][:n])
        assert np.abs(to_np(env._reward_buf) - g[pout + "reward"][:n]).max() <= TOL
        if mirror:   # the ref_* mirrors of row 1's items
            for k in ["ref_root_pos", "ref_root_rot", "ref_joint_rot", "ref_body_pos", "ref_contacts"]:
                assert np.abs(to_np(getattr(env, "_" + k)) - g[pout + k][:n]).max() <= TOL, k


@pytest.mark.parametrize("n", COUNTS)
def test_three_look_ahead_steps_straddle_the_pass_boundary(tmp_path, n):
    """`tar_obs_steps: [1, 2, 3]`: 5 rows x 14 joints = 70 joint items, so pass A ends in the middle of row 3 (item 48 = row 3, slot 7).
    The first three targets of the default configuration are the same three samples: their blocks, and every other block of the row,
    against the reference's golden observation."""
    from gpu_helpers import to_np
    g = golden("env_step")
    env = _env(tmp_path, n, {"tar_obs_steps": [1, 2, 3]}, False)
    width = 136 + 3 * 105 + 3 * 15 + 15 + 441
    assert env._obs_buf.shape == (n, width)
    _inject(env, g, "s0_in_", n)
    env.step(None)
    ref = g["s0_out_obs"][:n]
    # character 136 | targets 6 x 105 | target contacts 6 x 15 | character contacts 15 | 441 heights
    ref3 = np.concatenate([ref[:, :136 + 3 * 105], ref[:, 766:766 + 3 * 15], ref[:, 856:]], axis=1)
    _check_obs(to_np(env._obs_buf), ref3, width - 441)
    assert np.array_equal(to_np(env._done_buf), g["s0_out_done"][:n])
    assert np.abs(to_np(env._reward_buf) - g["s0_out_reward"][:n]).max() <= TOL


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("gl", [False, True])
def test_step_observation_equals_the_recomputed_one(tmp_path, gl, n):
    """The observation a step writes (MODE_STEP instantiation) and the one parc_env_compute_obs recomputes from the state the step left
    (MODE_OBS instantiation; the step has already advanced the timestep): bit for bit."""
    import torch
    from gpu_helpers import to_np
    g = golden("env_step_global_obs" if gl else "env_step")
    env = _env(tmp_path, n, {"global_obs": gl}, False)
    assert env._lib.parc_env_post_kernel(env._handle).decode() == ("k_env_post<MODE,true>" if gl else "k_env_post<MODE,false>")
    _inject(env, g, "in_" if gl else "s0_in_", n)
    env.step(None)
    step_obs = to_np(env._obs_buf).copy()
    env._obs_buf.zero_()
    env._compute_obs()
    torch.cuda.synchronize()
    assert np.array_equal(to_np(env._obs_buf), step_obs)
