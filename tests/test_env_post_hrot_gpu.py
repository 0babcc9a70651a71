"""-m gpu: the heading pass of k_env_post (parc_lanetab.hpp, parc_hrot_fill): the root velocities, the target rows' root offsets and the
key-body offsets of the character and of the targets go through one rotation stream behind the FK phase, each lane's source and destination
from a table built on the host; the root velocities reach the pass and the reward through LDS.  The golden scenes of
tests/test_env_post_rowmap_gpu.py (same helpers, same tolerances) that between them switch every block the pass writes -- heading frame and
global frame, the root height in front of the row, targets on and off, the reward in the local root frame -- at env counts that leave a
workgroup partly empty (1, 5) or give the reward's owner wave no env of its own (6), and the step observation against the recomputed one,
bit for bit, in each instantiation family."""
import numpy as np
import pytest

from conftest import golden
from test_env_post_prefetch_gpu import BITWISE
from test_env_post_rowmap_gpu import TOL, _check_obs, _env, _inject

pytestmark = pytest.mark.gpu
COUNTS = [1, 5, 6]
# scene -> (config overrides, mirror_ref_state, observation width)
SCENES = {
    "env_step": ({}, True, 1312),
    "env_step_global_obs": ({"global_obs": True}, False, 1312),
    "env_step_root_height_obs_global": ({"global_root_height_obs": True, "global_obs": True}, False, 1313),
    "env_step_local_root": ({"track_root": False}, False, 1312),
    "env_step_obs_blocks_c0_t0": ({"use_contact_info": False, "enable_tar_obs": False}, False, 577),
    "env_step_obs_blocks_c0_t1": ({"use_contact_info": False, "enable_tar_obs": True}, False, 1207),
}
VEL_TOL = 3e-5   # tests/test_hip_parity.py::_check_step_outputs: the reference's velocity mirrors


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
        # the reward's root-velocity term reads the character's root velocities from the LDS slots the heading pass reads
        assert np.abs(to_np(env._reward_terms)[3] - g[pout + "r_root_vel_r"][:n]).max() <= TOL
        if mirror:   # the ref_* mirrors: row 1's items, the contact block, and the velocity block
            for k in ["ref_root_pos", "ref_root_rot", "ref_joint_rot", "ref_body_pos", "ref_contacts"]:
                assert np.abs(to_np(getattr(env, "_" + k)) - g[pout + k][:n]).max() <= TOL, k
            for k in ["ref_root_vel", "ref_root_ang_vel", "ref_dof_vel"]:
                assert np.abs(to_np(getattr(env, "_" + k)) - g[pout + k][:n]).max() <= VEL_TOL, k


@pytest.mark.parametrize("n", [1, 6])
@pytest.mark.parametrize("name", list(BITWISE))
def test_step_observation_equals_the_recomputed_one(tmp_path, name, n):
    """The observation a step writes (MODE_STEP) and the one parc_env_compute_obs recomputes from the state the step left (MODE_OBS; the step
    has already advanced the timestep): bit for bit, and no float of the row left unwritten by either (the row is poisoned first)."""
    import torch
    from gpu_helpers import to_np
    overrides, mirror, scene, kernel = BITWISE[name]
    g = golden(scene)
    env = _env(tmp_path, n, overrides, mirror)
    assert env._lib.parc_env_post_kernel(env._handle).decode() == kernel
    _inject(env, g, "s0_in_" if scene == "env_step" else "in_", n)
    env._obs_buf.fill_(float("nan"))
    env.step(None)
    step_obs = to_np(env._obs_buf).copy()
    assert np.isfinite(step_obs).all()
    env._obs_buf.fill_(float("nan"))
    env._compute_obs()
    torch.cuda.synchronize()
    assert np.array_equal(to_np(env._obs_buf), step_obs)
