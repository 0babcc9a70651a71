"""CPU tests of the re-authored dynamics core (parc_amd/csrc/parc_dynamics.hpp built for the host).

PhysX parity is unpinned (closed binary, absent): these are the invariants SURVEY.md §7 asks for instead —
mass properties, momentum in free flight, free fall, PD step response, resting contact on a cell column,
wall contact — run on the same code the HIP kernel compiles."""
import os

import numpy as np
import pytest

from conftest import DATA, golden


@pytest.fixture(scope="module")
def dyn():
    from oracle.binding_dyn import DynOracle
    from parc_amd.envs import scene
    from parc_amd.util import path_loader
    cfg = path_loader.load_config(os.path.join(DATA, "configs/tracker_config/dm_env_default.yaml"))
    sc = scene.build_scene(cfg, 4, verbose=False)
    return DynOracle(sc.cfg), sc


def make_state(n, B=15, D=28, z=5.0):
    st = dict(root_pos=np.zeros((n, 3), np.float32), root_rot=np.zeros((n, 4), np.float32), root_vel=np.zeros((n, 3), np.float32),
              root_ang_vel=np.zeros((n, 3), np.float32), dof_pos=np.zeros((n, D), np.float32), dof_vel=np.zeros((n, D), np.float32),
              contact_force=np.zeros((n, B, 3), np.float32))
    st["root_rot"][:, 3] = 1.0
    st["root_pos"][:, 2] = z
    return st


FLAT = (np.zeros((64, 64), np.float32), (-12.8, -12.8), (0.4, 0.4))


def com_of(oracle, orc_char, d, st):
    mass, com, _, total, _ = d.mass_properties()
    jr = oracle.dof_to_rot(orc_char, st["dof_pos"])
    bp, br = oracle.forward_kinematics(orc_char, st["root_pos"], st["root_rot"], jr)
    n = bp.shape[0]
    c = np.zeros((n, 3))
    for b in range(15):
        off = oracle.quat_rotate(br[:, b], np.tile(com[b], (n, 1)))
        c += mass[b] * (bp[:, b] + off)
    return c / total


def test_mass_properties(dyn):
    d, sc = dyn
    mass, com, inertia, total, ncol = d.mass_properties()
    assert 40.0 < total < 55.0, total           # densities of humanoid.xml give ~50 kg
    assert np.all(mass > 0.05) and ncol == 42
    assert np.all(inertia[:, :3] > 0)
    # symmetric model: left/right limbs have equal masses
    for r, l in [(3, 6), (4, 7), (5, 8), (9, 12), (10, 13), (11, 14)]:
        assert abs(mass[r] - mass[l]) < 1e-5


def test_free_fall_and_momentum(dyn, oracle, orc_char):
    d, sc = dyn
    n = 4
    rng = np.random.default_rng(0)
    st = make_state(n, z=50.0)
    st["dof_pos"][:] = 0.3 * rng.standard_normal((n, 28)).astype(np.float32)
    act = (st["dof_pos"] + 0.2 * rng.standard_normal((n, 28))).astype(np.float32)
    off = np.zeros((n, 3), np.float32)
    c0 = com_of(oracle, orc_char, d, st)
    steps = 30
    for _ in range(steps):
        d.step(*FLAT, st, act, off)
    c1 = com_of(oracle, orc_char, d, st)
    assert np.all(np.isfinite(st["dof_pos"]))
    # internal PD torques cannot move the centre of mass sideways (first-order integrator: O(dt) drift allowed);
    # vertically it is a free fall
    assert np.abs(c1[:, :2] - c0[:, :2]).max() < 1e-2
    nsub = steps * 4
    dt = 1.0 / 120.0
    z_expected = -9.81 * dt * dt * nsub * (nsub + 1) / 2.0   # semi-implicit Euler
    assert np.abs((c1[:, 2] - c0[:, 2]) - z_expected).max() < 5e-3
    assert np.abs(st["contact_force"]).max() == 0.0


def test_pd_step_response_zero_g(dyn, oracle, orc_char):
    d, sc = dyn
    d.set_gravity(0.0)
    try:
        n = 2
        st = make_state(n, z=50.0)
        rng = np.random.default_rng(1)
        lo, hi = sc.action_low.astype(np.float32), sc.action_high.astype(np.float32)
        tgt = (0.25 * rng.uniform(-1, 1, (n, 28)) * np.minimum(np.abs(lo), np.abs(hi))).astype(np.float32)
        tgt[:, [9, 13]] = 0.0
        tgt[:, 9] = 0.8; tgt[:, 13] = -0.8; tgt[:, 17] = 0.6; tgt[:, 24] = 0.6   # hinges inside their ranges
        off = np.zeros((n, 3), np.float32)
        hist = []
        for _ in range(60):
            d.step(*FLAT, st, tgt, off)
            hist.append(np.abs(st["dof_vel"]).max())
        assert np.all(np.isfinite(st["dof_pos"]))
        # hinge angles reach their targets; spherical joints reach the target rotation
        jr = oracle.dof_to_rot(orc_char, st["dof_pos"]); jt = oracle.dof_to_rot(orc_char, tgt)
        ang = oracle.quat_diff_angle(jr.reshape(-1, 4), jt.reshape(-1, 4))
        assert np.abs(ang).max() < 0.03, np.abs(ang).max()
        assert hist[-1] < 0.05 and max(hist) < 60.0   # settles, never explodes
    finally:
        d.set_gravity(-9.81)


def standing_state(n, z):
    st = make_state(n, z=z)
    return st


def test_resting_contact_flat_ground(dyn, oracle, orc_char):
    d, sc = dyn
    n = 2
    st = standing_state(n, 0.95)   # feet a few cm above the ground (root height of the T-pose is ~0.89)
    act = np.zeros((n, 28), np.float32)
    off = np.zeros((n, 3), np.float32)
    _, _, _, total, _ = d.mass_properties()
    fz = []
    for k in range(45):   # 1.5 s
        d.step(*FLAT, st, act, off)
        fz.append(st["contact_force"][:, :, 2].sum(axis=1))
        assert np.all(np.isfinite(st["root_pos"]))
        if np.abs(st["root_rot"][:, :2]).max() > 0.3:
            break   # a passive T-pose eventually topples; the checks below use the standing phase
    fz = np.array(fz)
    k_settled = min(len(fz) - 1, 20)
    # while standing, the ground carries the weight and the feet do not sink
    assert np.all(np.abs(fz[10:k_settled + 1].mean(axis=0) - total * 9.81) < 0.25 * total * 9.81), fz[10:k_settled + 1].mean(axis=0)
    jr = oracle.dof_to_rot(orc_char, st["dof_pos"])
    bp, _ = oracle.forward_kinematics(orc_char, st["root_pos"], st["root_rot"], jr)
    assert bp[:, :, 2].min() > -0.02
    # only the feet touch while standing
    assert np.abs(st["contact_force"][:, 1:9]).max() < 1e-3 or np.abs(st["root_rot"][:, :2]).max() > 0.3


def test_wall_blocks_motion(dyn, oracle, orc_char):
    d, sc = dyn
    hf = np.zeros((64, 64), np.float32)
    hf[40:, :] = 3.0    # a 3 m wall starting at x = -12.8 + 39.5*0.4 = 3.0
    n = 1
    st = make_state(n, z=1.5)
    st["root_vel"][:, 0] = 4.0      # thrown at the wall
    act = np.zeros((n, 28), np.float32)
    off = np.zeros((n, 3), np.float32)
    d.set_gravity(0.0)
    try:
        for _ in range(60):
            d.step(hf, (-12.8, -12.8), (0.4, 0.4), st, act, off)
        assert np.all(np.isfinite(st["root_pos"]))
        assert st["root_pos"][0, 0] < 3.0 + 0.05, st["root_pos"]   # did not tunnel through the wall face at x = 3.0
    finally:
        d.set_gravity(-9.81)


def test_step_edge_supports_foot(dyn, oracle, orc_char):
    """Standing on a raised block: the character rests at block height, not at the surrounding ground."""
    d, sc = dyn
    hf = np.zeros((64, 64), np.float32)
    hf[30:35, 30:35] = 0.8          # 2 m x 2 m block, top at 0.8 m, centred near the origin
    n = 1
    st = make_state(n, z=0.8 + 0.95)
    st["root_pos"][0, 0] = -12.8 + 32 * 0.4
    st["root_pos"][0, 1] = -12.8 + 32 * 0.4
    act = np.zeros((n, 28), np.float32)
    off = np.zeros((n, 3), np.float32)
    for _ in range(15):
        d.step(hf, (-12.8, -12.8), (0.4, 0.4), st, act, off)
    assert 0.8 + 0.8 < st["root_pos"][0, 2] < 0.8 + 1.0, st["root_pos"]


def test_body_that_crossed_a_wall_face_is_pushed_back_not_launched(dyn, oracle, orc_char):
    """Regression: a point whose centre had crossed a wall face (its cell = the wall's cell) used to be pushed out through
    the TOP of the wall, metres away: tens of kN, bodies launched at > 100 m/s.  It must leave sideways, the way it came."""
    d, sc = dyn
    hf = np.zeros((64, 64), np.float32)
    hf[40:, :] = 5.0    # 5 m wall, face at x = 3.0
    n = 3
    st = make_state(n, z=0.95)
    st["root_pos"][:, 0] = [2.55, 2.70, 2.80]   # hands / feet reach or cross the face during the fall
    st["root_vel"][:, 0] = [6.0, 3.0, 1.0]
    act = np.zeros((n, 28), np.float32)
    off = np.zeros((n, 3), np.float32)
    vmax, zmax = 0.0, 0.0
    for _ in range(90):  # 3 s: run into the wall, fall, come to rest at its foot
        d.step(hf, (-12.8, -12.8), (0.4, 0.4), st, act, off)
        assert np.all(np.isfinite(st["root_pos"]))
        vmax = max(vmax, np.linalg.norm(st["root_vel"], axis=1).max())
        zmax = max(zmax, st["root_pos"][:, 2].max())
    assert vmax < 12.0, vmax                       # nothing is launched (free-fall from 1 m is 4.4 m/s, the throw 6 m/s)
    assert zmax < 1.6, zmax                        # and nobody ends up on top of the wall
    assert st["root_pos"][:, 0].max() < 3.0 + 0.3  # the root stays on this side of the face (limbs may dent the wall by < pen_cap)
    assert np.abs(st["contact_force"]).max() < 50.0 * 9.81 * 30.0


def test_own_column_exit_rule():
    """own_column_contact through the host build: geometry only."""
    import ctypes as C
    from oracle.binding_dyn import build
    lib = C.CDLL(build())
    lib.orc_own_column_contact.restype = C.c_float
    lib.orc_own_column_contact.argtypes = [C.POINTER(C.c_float), C.c_float, C.c_float, C.c_float, C.c_float, C.POINTER(C.c_float)]
    n = (C.c_float * 3)()

    def q(tops5, x, y, z, r):  # tops5: own, +x, -x, +y, -y; cell (0,0) centred at the origin, 0.4 m cells
        t = (C.c_float * 5)(*tops5)
        pen = lib.orc_own_column_contact(t, x, y, z, r, n)
        return pen, (n[0], n[1], n[2])
    # above the surface: +z, pen = r - height
    pen, nn = q([1.0, 0, 0, 0, 0], 0.05, 0.0, 1.03, 0.05)
    assert nn == (0.0, 0.0, 1.0) and abs(pen - 0.02) < 1e-6
    # 1 cm inside the -x face of a 5 m wall, free ground on that side: leaves through that face
    pen, nn = q([5.0, 5.0, 0.0, 5.0, 5.0], -0.19, 0.0, 1.0, 0.04)
    assert nn == (-1.0, 0.0, 0.0) and abs(pen - 0.05) < 1e-6
    # toe corner (r = 0) 1 mm inside a 0.4 m riser while pressing 2 mm into the lower step: sideways, not 0.4 m up
    pen, nn = q([0.4, 0.4, 0.002 + 0.1, 0.4, 0.4], -0.199, 0.0, 0.1, 0.0)
    assert nn == (-1.0, 0.0, 0.0) and abs(pen - 0.001) < 1e-6
    # deep inside a plateau (all neighbours as high): only the top is a way out
    pen, nn = q([1.0, 1.0, 1.0, 1.0, 1.0], 0.1, 0.1, 0.7, 0.05)
    assert nn == (0.0, 0.0, 1.0) and abs(pen - 0.35) < 1e-6
    # just under the top of a pillar: up (3 cm) beats sideways (15 cm)
    pen, nn = q([1.0, 0.0, 0.0, 0.0, 0.0], 0.05, 0.0, 0.97, 0.0)
    assert nn == (0.0, 0.0, 1.0) and abs(pen - 0.03) < 1e-6


# ---- edge contacts of shafts and soles (round 3): single rigid bodies built through the same C structs -------------------------
def _single_body(sc, gtype, pos, pos2, size, density=1000.0):
    """DynOracle of ONE free rigid body carrying one geom (type 0 box / 2 capsule as in ParcDynamicsParams)."""
    import copy
    import ctypes as C
    from oracle.binding_dyn import DynOracle
    from parc_amd import lib as L
    cfg = L.ParcEnvConfig.from_buffer_copy(bytes(sc.cfg))
    cfg.model.num_bodies = 1; cfg.model.dof_size = 0
    cfg.model.parent[0] = -1
    dp = cfg.dynamics
    dp.num_geoms = 1; dp.geom_body[0] = 0; dp.geom_type[0] = gtype; dp.geom_density[0] = density
    for a in range(3):
        dp.geom_pos[0][a] = pos[a]; dp.geom_pos2[0][a] = pos2[a]; dp.geom_size[0][a] = size[a]
    return DynOracle(cfg)


def _rigid_state(n, pos, quat=(0, 0, 0, 1)):
    st = dict(root_pos=np.tile(np.asarray(pos, np.float32), (n, 1)), root_rot=np.tile(np.asarray(quat, np.float32), (n, 1)),
              root_vel=np.zeros((n, 3), np.float32), root_ang_vel=np.zeros((n, 3), np.float32), dof_pos=np.zeros((n, 0), np.float32),
              dof_vel=np.zeros((n, 0), np.float32), contact_force=np.zeros((n, 1, 3), np.float32))
    return st


MINP, DX = (-12.8, -12.8), (0.4, 0.4)
X_EDGE = -12.8 + 31.5 * 0.4   # -0.2: the grid line between cells 31 and 32


def _platform(top=1.0):
    hf = np.zeros((64, 64), np.float32)
    hf[32:, :] = top            # platform on x > X_EDGE, pit on x < X_EDGE
    return hf


def test_segment_edge_point_geometry(dyn):
    d, sc = dyn
    assert d.num_segments() == 8 + 4           # eight capsule shafts (arms, thighs, shins; not the stubby clavicles) + the two long sole edges of each foot
    hf = _platform(1.0)
    # horizontal shaft 3 cm above the lip, crossing it at right angles: the candidate is the point over the lip
    q = d.segment_edge_point(hf, MINP, DX, [X_EDGE - 0.15, 0.0, 1.03], [X_EDGE + 0.25, 0.0, 1.03])
    assert q is not None and np.allclose(q[:3], [X_EDGE, 0.0, 1.03], atol=1e-5) and q[3] == 1.0   # 37 % along the segment: full weight
    # inclined shaft (45 degrees, rising towards the platform) whose axis passes 5 cm above the lip measured vertically:
    # the closest point to the edge is NOT the crossing of the grid line but the foot of the perpendicular, 5 / sqrt(2) cm away
    a, b = np.array([X_EDGE - 0.2, 0.1, 0.85]), np.array([X_EDGE + 0.2, 0.1, 1.25])
    q = d.segment_edge_point(hf, MINP, DX, a, b)
    assert q is not None and abs(np.hypot(q[0] - X_EDGE, q[2] - 1.0) - 0.05 / np.sqrt(2)) < 1e-5 and abs(q[1] - 0.1) < 1e-6
    # flat ground on both sides of the line, or a shaft that crosses no line: no candidate
    assert d.segment_edge_point(np.zeros((64, 64), np.float32), MINP, DX, [X_EDGE - 0.15, 0.0, 0.03], [X_EDGE + 0.25, 0.0, 0.03]) is None
    assert d.segment_edge_point(hf, MINP, DX, [X_EDGE + 0.05, 0.0, 1.03], [X_EDGE + 0.30, 0.0, 1.03]) is None
    # towards an end of the segment the candidate fades out (w = 10 min(t, 1 - t)): the end sphere / corner point that sits there takes over
    q = d.segment_edge_point(hf, MINP, DX, [X_EDGE - 0.01, 0.0, 1.03], [X_EDGE + 0.39, 0.0, 1.03])
    assert q is not None and abs(q[3] - 0.25) < 1e-3                                            # 2.5 % along: a quarter of the strength
    assert d.segment_edge_point(hf, MINP, DX, [X_EDGE + 0.001, 0.0, 1.03], [X_EDGE + 0.3, 0.0, 1.5]) is None   # the closest point lies before the end
    # an edge along x (platform on y > Y_EDGE) is found through the y axis
    hf2 = np.zeros((64, 64), np.float32); hf2[:, 32:] = 0.6
    q = d.segment_edge_point(hf2, MINP, DX, [0.3, X_EDGE - 0.1, 0.65], [0.3, X_EDGE + 0.2, 0.65])
    assert q is not None and np.allclose(q[:3], [0.3, X_EDGE, 0.65], atol=1e-5)


def test_shaft_lying_across_a_platform_edge_is_supported(dyn):
    """A capsule (shin-sized: r = 5 cm, 40 cm long) lies on a platform with 15 cm of its length and one end sphere hanging over the
    lip; its centre of mass is over the platform, so it must stay.  With the end spheres alone (the round-2 geometry: counterfactual
    below) only the end on the platform is supported and the shaft rotates through the lip into the pit."""
    d, sc = dyn
    cap = _single_body(sc, 2, (-0.2, 0.0, 0.0), (0.2, 0.0, 0.0), (0.05, 0, 0))
    assert cap.num_segments() == 1
    hf = _platform(1.0)

    def run(o):
        st = _rigid_state(1, (X_EDGE + 0.05, 0.0, 1.0 + 0.05 + 0.002))   # axis 5.2 cm above the top: ends at X_EDGE - 0.15 / + 0.25
        zmin_free_end = 9.9
        for _ in range(45):   # 1.5 s
            o.step(hf, MINP, DX, st, np.zeros((1, 0), np.float32), np.zeros((1, 3), np.float32))
            q = st["root_rot"][0]
            ex = np.array([1 - 2 * (q[1] ** 2 + q[2] ** 2), 2 * (q[0] * q[1] + q[2] * q[3]), 2 * (q[0] * q[2] - q[1] * q[3])])  # body x axis
            zmin_free_end = min(zmin_free_end, (st["root_pos"][0] - 0.2 * ex)[2])
        return st, zmin_free_end
    st, zfree = run(cap)
    assert zfree > 1.0 + 0.05 - 0.01, zfree                              # the hanging end never drops below resting height - 1 cm
    assert abs(st["root_pos"][0, 2] - 1.05) < 0.01 and np.abs(st["root_vel"]).max() < 0.02
    assert abs(st["contact_force"][0, 0, 2] - 9.81 * cap.mass_properties()[3]) < 0.05 * 9.81 * cap.mass_properties()[3]
    cap.set_num_segments(0)
    _, zfree0 = run(cap)
    assert zfree0 < 1.0 + 0.05 - 0.04, zfree0                            # counterfactual: without the shaft contact it swings through the lip


def test_sole_coming_down_on_a_lip_between_its_corners_is_stopped(dyn):
    """A foot-sized box pitched 25 degrees (toe up) is dropped so that the middle of its sole meets the lip of a step: toe corners end
    up above the platform, heel corners over the pit, no corner touches.  The sole edges must be stopped by the lip (penetration of the
    solid's corner stays at the contact compliance scale); with the corners alone the box sinks in by centimetres."""
    d, sc = dyn
    a, b, c = 0.0885, 0.045, 0.0275
    box = _single_body(sc, 0, (0.0, 0.0, 0.0), (0, 0, 0), (a, b, c), density=1141.0 * 20.0)   # loaded like a foot carrying the body (~20 kg)
    assert box.num_segments() == 2
    hf = _platform(1.0)
    th = np.deg2rad(-25.0)                                                  # rotation about +y by -25 deg lifts the +x end (the toe)
    quat = (0.0, np.sin(th / 2), 0.0, np.cos(th / 2))
    Rm = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])

    def corner_depth(st):
        """deepest penetration of the two long sole edges into the solid's corner: min(depth below the top, depth behind the face)"""
        p0 = st["root_pos"][0].astype(np.float64); q = st["root_rot"][0].astype(np.float64)
        x, y, z, w = q
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                      [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        worst = 0.0
        for sy in (-b, b):
            for t in np.linspace(-a, a, 41):
                p = p0 + R @ np.array([t, sy, -c])
                if p[0] > X_EDGE and p[2] < 1.0:
                    worst = max(worst, min(1.0 - p[2], p[0] - X_EDGE))
        return worst

    def run(o):
        mid_sole = Rm @ np.array([0.0, 0.0, -c])                           # sole centre relative to the box centre
        st = _rigid_state(1, (X_EDGE - mid_sole[0], 0.0, 1.0 - mid_sole[2] + 0.01), quat)   # sole centre 1 cm above the lip
        worst = 0.0
        for _ in range(8):                                                 # ~0.27 s: the touch-down
            o.step(hf, MINP, DX, st, np.zeros((1, 0), np.float32), np.zeros((1, 3), np.float32))
            worst = max(worst, corner_depth(st))
        return worst
    w1 = run(box)
    box.set_num_segments(0)
    w0 = run(box)
    assert w1 < 0.012, w1            # stopped at the contact compliance scale
    assert w0 > 0.03 and w0 > 3.0 * w1, (w0, w1)   # counterfactual: corners only -> the lip cuts centimetres into the sole


def test_planted_foot_sticks_under_a_lateral_load_and_slides_beyond_the_cone(dyn):
    """Friction (regularised Coulomb, implicit): a foot-sized box carrying 20 kg rests on flat ground; gravity is tilted so that the
    lateral load is 0.5 of the weight (mu = 1: inside the cone) -- it must not creep (< 1 mm/s; the round-2 'capped viscous' setting,
    dtang = 1e4, creeps at 2.5 mm/s: counterfactual; the value is bounded by fp32, see fill_dyn_model); at 1.3 of the weight (outside the cone) it must slide, accelerating at
    ~ (1.3 - mu) g."""
    d, sc = dyn
    a, b, c = 0.0885, 0.045, 0.0275
    box = _single_body(sc, 0, (0.0, 0.0, 0.0), (0, 0, 0), (a, b, c), density=1141.0 * 20.0)
    flat = np.zeros((64, 64), np.float32)
    g = 9.81

    def creep(o, lateral, seconds=1.0):
        st = _rigid_state(1, (0.03, 0.02, c - 0.002))
        o.set_ext_acc(0.0, 0.0)
        for _ in range(15):                       # settle
            o.step(flat, MINP, DX, st, np.zeros((1, 0), np.float32), np.zeros((1, 3), np.float32))
        o.set_ext_acc(lateral * g, 0.0)
        for _ in range(10):                       # load on, let the transient pass
            o.step(flat, MINP, DX, st, np.zeros((1, 0), np.float32), np.zeros((1, 3), np.float32))
        x0 = st["root_pos"][0, 0].astype(np.float64)
        k = int(round(seconds * 30))
        for _ in range(k):
            o.step(flat, MINP, DX, st, np.zeros((1, 0), np.float32), np.zeros((1, 3), np.float32))
        o.set_ext_acc(0.0, 0.0)
        return (st["root_pos"][0, 0] - x0) / seconds, st
    v_stick, st = creep(box, 0.5)
    assert 0.0 <= v_stick < 1.0e-3, v_stick
    assert abs(st["contact_force"][0, 0, 0] + 0.5 * st["contact_force"][0, 0, 2]) < 0.05 * st["contact_force"][0, 0, 2]   # friction balances the load
    c0 = box.get_contact()
    assert c0["dtang"] == 3.0e4 and c0["mu"] == 1.0
    box.set_contact(c0["kn"], c0["dn"], 1.0e4, c0["mu"])
    v_old, _ = creep(box, 0.5)
    assert v_old > 2.0e-3, v_old                  # what round 2 did
    box.set_contact(c0["kn"], c0["dn"], c0["dtang"], c0["mu"])
    v_slip, st = creep(box, 1.3, seconds=0.5)
    # outside the cone: a = (1.3 - mu) g = 2.9 m/s^2; over [t1, t1 + 0.5] with t1 = 1/3 s: mean speed = a (t1 + 0.25)
    assert 0.6 * 2.9 * (1.0 / 3.0 + 0.25) < v_slip < 1.3 * 2.9 * (1.0 / 3.0 + 0.25), v_slip


def test_jammed_leg_state_stays_bounded():
    """Regression: env 3301 of the 16 384-env cfg-3 settle run (tools/nan_hunt.py, round 3), a shin and a foot jammed between two walls with
    both contacts saturated.  With the friction stiffness at 1e5 N s/m the fp32 joint eliminations lost positive definiteness and the state
    went from 1 m/s to 1e11 m/s within one control step; the shipped value (and twice it) must keep it bounded."""
    import pathlib
    import tempfile
    import test_dynamics_gpu as TG
    from oracle.binding_dyn import DynOracle
    from parc_amd.envs import scene
    z = golden("dyn_jammed_leg_state")
    cfg = TG._cfg3(pathlib.Path(tempfile.mkdtemp()), 1024)
    sc = scene.build_scene(cfg, 16384, 0, 0, None, seed=21, enable_dynamics=True, verbose=False)
    e = int(z["env_id"][0])
    assert np.allclose(sc.env_offsets[e], z["env_offsets"][0])
    d = DynOracle(sc.cfg)
    ter = sc.grid.terrain
    c0 = d.get_contact()
    for dtang in (c0["dtang"], 2.0 * c0["dtang"]):
        d.set_contact(c0["kn"], c0["dn"], dtang, c0["mu"])
        st = dict(root_pos=z["_char_root_pos"].copy(), root_rot=z["_char_root_rot"].copy(), root_vel=z["_char_root_vel"].copy(),
                  root_ang_vel=z["_char_root_ang_vel"].copy(), dof_pos=z["_char_dof_pos"].copy(), dof_vel=z["_char_dof_vel"].copy(),
                  contact_force=np.zeros((1, 15, 3), np.float32))
        for _ in range(10):
            d.step(ter.hf, ter.min_point, ter.dxdy, st, z["act"], z["env_offsets"])
            assert np.isfinite(st["root_pos"]).all()
            assert np.linalg.norm(st["root_vel"]) < 8.0 and np.abs(st["dof_vel"]).max() < 40.0, (dtang, st["root_vel"], np.abs(st["dof_vel"]).max())


def test_contact_geometry_agrees_with_the_physx_recorded_contact_flags(dyn, oracle, orc_char):
    """The one PhysX artefact the reference ships, used where it IS an oracle: `dec2024_teaser_717_1_opt_dm.pkl` holds, per frame, the pose
    PhysX produced and which bodies carried a contact force (`body_contacts`, written by ig_parkour_env.py:664-685,759-796).  Putting the
    character AT each recorded pose and asking this simulator's contact geometry (collision spheres, box corners, shaft / sole-edge
    candidates against the cell columns) which bodies touch the terrain needs no integration, so it does not suffer from the divergence
    of an open-loop replay: it checks shapes, FK, terrain and units against PhysX directly.  PhysX rests at zero penetration, a penalty
    model reports a force only when penetrating, so the shapes are grown by a contact offset (5 - 10 mm; PhysX's own is 20 mm).
    Measured (round 3): 98.9 % of the 142 x 15 (frame, body) flags agree, feet 95.8 %, hands 99.3 %, foot contact rate 0.553 vs 0.553."""
    from parc_amd import ms_file
    from oracle.binding_dyn import DynOracle
    d0, sc = dyn
    f = ms_file.load_ms_file(os.path.join(DATA, "motion_terrains", "dec2024_teaser_717_1_opt_dm.pkl"))
    md, td = f.motion_data, f.terrain_data
    n = md.root_pos.shape[0]
    dof = oracle.rot_to_dof(orc_char, np.ascontiguousarray(md.joint_rot, np.float32))
    ref = md.body_contacts > 0.5
    feet, hands = [11, 14], [5, 8]
    res = {}
    for eps in (0.0, 0.005, 0.01):
        d = DynOracle(sc.cfg)
        d.set_gravity(0.0); d.set_num_substeps(1)       # one substep: the reported force is the one evaluated at the pose itself
        if eps:
            d.inflate(eps)
        st = dict(root_pos=md.root_pos.astype(np.float32).copy(), root_rot=md.root_rot.astype(np.float32).copy(), root_vel=np.zeros((n, 3), np.float32),
                  root_ang_vel=np.zeros((n, 3), np.float32), dof_pos=dof.copy(), dof_vel=np.zeros((n, 28), np.float32),
                  contact_force=np.zeros((n, 15, 3), np.float32))
        d.step(td.hf, td.min_point, (td.dx, td.dx), st, dof.copy(), np.zeros((n, 3), np.float32))
        sim = np.linalg.norm(st["contact_force"], axis=-1) > 1e-5
        res[eps] = dict(all=(sim == ref).mean(), feet=(sim == ref)[:, feet].mean(), hands=(sim == ref)[:, hands].mean(),
                        foot_rate=sim[:, feet].mean(), false_pos=(sim & ~ref).mean())
    print(res, "recorded foot contact rate", ref[:, feet].mean())
    assert res[0.0]["false_pos"] < 0.002                 # at the recorded poses nothing penetrates that PhysX did not report as touching
    for eps in (0.005, 0.01):
        r = res[eps]
        assert r["all"] > 0.98 and r["feet"] > 0.94 and r["hands"] > 0.98, (eps, r)
        assert abs(r["foot_rate"] - ref[:, feet].mean()) < 0.02, (eps, r["foot_rate"], ref[:, feet].mean())


def test_collision_set_that_does_not_fit_the_tables_is_reported(dyn):
    """Round-3 advice: a model with more collision points than the fixed tables hold (DYN_MAXC = 48: the humanoid has 42, one more box adds 8)
    used to be shortened silently -- a contact model that depends on the geom order.  The model builder counts what it could not place
    (`DynModel::truncated`); parc_env_create refuses such a model with PARC_ERR_INVALID (GPU test), the humanoid reports 0."""
    import ctypes as C
    d, sc = dyn
    assert d.truncated() == 0
    cfg2 = type(sc.cfg)()
    C.memmove(C.byref(cfg2), C.byref(sc.cfg), C.sizeof(cfg2))   # a byte copy: the nested structs are values, the pointers stay valid (sc lives on)
    k = cfg2.dynamics.num_geoms
    cfg2.dynamics.geom_body[k] = 2; cfg2.dynamics.geom_type[k] = 0   # a box on the head
    for a in range(3):
        cfg2.dynamics.geom_pos[k][a] = 0.0; cfg2.dynamics.geom_size[k][a] = 0.05
    cfg2.dynamics.geom_density[k] = 1000.0
    cfg2.dynamics.num_geoms = k + 1
    from oracle.binding_dyn import DynOracle
    d2 = DynOracle(cfg2)
    assert d2.truncated() == 2          # 42 + 8 - 48


def test_physx_recorded_transitions_one_step_and_closed_loop(dyn, oracle, orc_char):
    """The PhysX-anchored check of the integrator that needs no policy (round-3 verdict, item 6; tests/physx_transitions.py has the method).
    From every recorded state of `dec2024_teaser_717_1_opt_dm.pkl` (pose from the frames, velocities from the recorded observation stream) the PD
    targets are the ones that put THIS simulator's joints on the recorded next joint angles; what is compared with PhysX is what no target can
    buy: the motion of the unactuated floating base and the set of touching bodies.
      * one step (141 transitions): the root lands within 6.6 mm (median) of where PhysX put it -- closer than the constant-velocity
        extrapolation of the recorded state (7.7 mm) --, contact flags agree on 98 % of the (frame, body) pairs, feet 90 %;
      * closed loop, 10 control steps on the SIMULATED state (47 starts): root height within 1.1 cm (median; free fall would be 54 cm), root position
        5 cm, root rotation 0.13 rad, feet flags 84 %, foot contact rate 0.48 vs 0.57 recorded.  The open-loop replay of the same file
        (tests/test_dynamics_gpu.py) loses 9.7 cm of height and agrees on 72 % of the feet flags: it fails these thresholds;
      * the check discriminates: without friction the root turns 0.43 rad and the feet agreement drops to 68 %; with contacts 100 x softer the
        root sinks 25 cm -- both counterfactuals fail the same thresholds (asserted)."""
    from conftest import golden
    from oracle.binding_dyn import DynOracle
    from physx_transitions import closed_loop, load, one_step
    d0, sc = dyn
    R = load(oracle, orc_char, golden("char_model"))
    r = one_step(DynOracle(sc.cfg), oracle, R)
    assert np.median(r["e_pos"]) < 0.009 and np.median(r["e_pos"]) < np.median(r["e_cv"]) and r["e_pos"].max() < 0.03
    assert np.median(r["e_z"]) < 0.006 and np.median(r["e_rot"]) < 0.015
    assert np.median(r["e_vel"]) < np.median(np.linalg.norm(R["root_vel"][1:] - R["root_vel"][:-1], axis=1))     # beats "the velocity does not change"
    assert r["agree_all"] > 0.97 and r["agree_feet"] > 0.88 and abs(r["foot_rate_sim"] - r["foot_rate_ref"]) < 0.10
    assert r["false_neg"] < 0.02       # a body PhysX reports in contact at both ends of the step and this simulator leaves in the air

    def passes(m):
        return (m["e_z_med"] < 0.03 and m["e_pos_med"] < 0.08 and m["e_rot_med"] < 0.20 and m["agree_all"] > 0.95 and m["agree_feet"] > 0.78
                and abs(m["foot_rate_sim"] - m["foot_rate_ref"]) < 0.15)
    cl = closed_loop(DynOracle(sc.cfg), oracle, R)
    print("closed loop, h = 10:", cl[-1])
    assert passes(cl[-1]), cl[-1]
    assert all(m["e_z_med"] < 0.03 for m in cl)                       # the height never drifts on the way
    # the open-loop replay's own numbers (0.097 m height error, 72 % feet flags) would not pass:
    assert not passes(dict(cl[-1], e_z_med=0.097, agree_feet=0.72))
    # counterfactual models must fail
    for kw in (dict(mu=0.0), dict(kn=5e2, dn=5.0, dtang=3e2)):
        d = DynOracle(sc.cfg)
        c = d.get_contact(); c.update(kw)
        d.set_contact(c["kn"], c["dn"], c["dtang"], c["mu"])
        m = closed_loop(d, oracle, R)[-1]
        assert not passes(m), (kw, m)


def test_contact_manifold_speculative_planes_and_cached_planes(dyn):
    """The contact manifold of round 4 (parc_dynamics.hpp): contacts are discovered in substep 0 of a control step and kept as planes, every
    substep re-evaluates the cached planes; discovery also keeps SPECULATIVE planes (pen > -margin, margin = min(0.02 + 0.0375 s x approach speed,
    0.08 m)).  On single rigid bodies built through the same C structs:
      * a 5 cm sphere coming down at 2 m/s that starts a control step 2.5 cm above the ground (it arrives in the second substep): with the margin it
        is stopped like under discovery in every substep (period 1) -- deepest penetration within 2 mm --; WITHOUT the margin (counterfactual) the
        cached list is empty for the rest of the control step and the sphere is 2 x deeper in the ground before anything pushes back;
      * on flat ground the planes are exact: period 4 and period 1 give the same trajectory sample for sample;
      * a plane outlives its cell until the next discovery (the documented price): a box pushed off a ledge at 1 m/s is carried at most one
        control step's travel further than under period 1, then falls the same way."""
    d, sc = dyn
    flat = np.zeros((64, 64), np.float32)
    ball = lambda: _single_body(sc, 1, (0.0, 0.0, 0.0), (0, 0, 0), (0.05, 0, 0), density=2000.0)

    def drop(o, steps=6):
        st = _rigid_state(1, (0.1, 0.1, 0.05 + 0.025))       # lowest point 2.5 cm above the ground at the start of the control step
        st["root_vel"][0, 2] = -2.0
        deepest = 0.0
        for _ in range(steps):
            o.step(flat, MINP, DX, st, np.zeros((1, 0), np.float32), np.zeros((1, 3), np.float32))
            deepest = max(deepest, 0.05 - st["root_pos"][0, 2])
        return deepest, st
    o4 = ball()
    o1 = ball(); o1.set_manifold_period(1)
    o0 = ball(); o0.set_speculative_margin(0.0, 0.0, 0.0)
    p4, s4 = drop(o4); p1, s1 = drop(o1); p0, _ = drop(o0)
    assert 0.0 < p1 < 0.03 and abs(p4 - p1) < 0.002, (p4, p1)          # caught by the plane it was about to hit
    assert p0 > 2.0 * p1 and p0 > p4 + 0.01, (p0, p4, p1)              # counterfactual: no margin -> the touch-down is seen a control step late
    # on flat ground the cached planes are exact (normal +z, the column top): period 4 and period 1 produce the SAME trajectory, sample for sample
    # (a light single body does not come to rest under this penalty law -- it chatters by 0.3 mm in a five-step cycle, under either period)
    traj = []
    for o in (ball(), o1):
        st = _rigid_state(1, (0.1, 0.1, 0.05))
        zs = []
        for _ in range(60):
            o.step(flat, MINP, DX, st, np.zeros((1, 0), np.float32), np.zeros((1, 3), np.float32))
            zs.append((float(st["root_pos"][0, 2]), float(st["contact_force"][0, 0, 2])))
        traj.append(np.array(zs))
    assert np.abs(traj[0] - traj[1]).max() < 1e-6, np.abs(traj[0] - traj[1]).max()
    assert 0.0490 < traj[0][:, 0].min() and traj[0][:, 0].max() < 0.0500          # it stays within a millimetre of the surface
    # ledge: a foot-sized box slides off a platform at 1 m/s
    a, b, c = 0.0885, 0.045, 0.0275
    hf = _platform(1.0)       # platform on x > X_EDGE, pit on x < X_EDGE

    def slide(period):
        o = _single_body(sc, 0, (0.0, 0.0, 0.0), (0, 0, 0), (a, b, c), density=1141.0)
        o.set_manifold_period(period)
        o.set_contact(5.0e4, 5.0e2, 3.0e4, 0.0)          # frictionless: it keeps its speed
        st = _rigid_state(1, (X_EDGE + 0.30, 0.0, 1.0 + c - 0.0005))
        st["root_vel"][0, 0] = -1.0
        zs = []
        for _ in range(24):
            o.step(hf, MINP, DX, st, np.zeros((1, 0), np.float32), np.zeros((1, 3), np.float32))
            zs.append(float(st["root_pos"][0, 2]))
        return np.array(zs)
    z4, z1 = slide(4), slide(1)
    left4, left1 = int(np.argmax(z4 < 1.0)), int(np.argmax(z1 < 1.0))       # first control step at which the box centre is below the platform top
    assert left1 > 5 and 0 <= left4 - left1 <= 1, (left4, left1)           # carried at most one control step longer
    assert abs(z4[-1] - z1[-1]) < 0.25 * abs(1.0 - z1[-1]) + 0.02, (z4[-1], z1[-1])    # then it falls the same way


def _dyn_with_control_mode(mode):
    from oracle.binding_dyn import DynOracle
    from parc_amd.envs import scene
    from parc_amd.util import path_loader
    cfg = path_loader.load_config(os.path.join(DATA, "configs/tracker_config/dm_env_default.yaml"))
    cfg["env"]["control_mode"] = mode
    sc = scene.build_scene(cfg, 4, verbose=False)
    return DynOracle(sc.cfg), sc


def test_control_modes_vel_torque_pd_exp(dyn, oracle, orc_char):
    """The reference's other control modes (ig_char_env.py:21-26).  No PhysX answer exists for them either (parity unpinned):
    what each mode MEANS is checked -- torque: the clipped action is the joint torque, nothing else drives the joint; vel: the joint's rate goes to
    the clipped action at the rate damping / inertia; pd_exp: the explicit PD torque of the step's first state, target = the action as given,
    limited to the motor efforts, which for soft gains follows the implicit pd drive."""
    n = 2
    off = np.zeros((n, 3), np.float32)
    # ---- torque, zero action = the pd mode without gains: a limp character, bit for bit the same trajectory
    d_tq, sc_tq = _dyn_with_control_mode("torque")
    d_pd, _ = _dyn_with_control_mode("pd")
    d_pd.scale_gains(0.0)
    rng = np.random.default_rng(5)
    st_a = make_state(n, z=1.2); st_a["dof_pos"][:] = 0.2 * rng.standard_normal((n, 28)).astype(np.float32)
    st_b = {k: v.copy() for k, v in st_a.items()}
    for _ in range(20):
        d_tq.step(*FLAT, st_a, np.zeros((n, 28), np.float32), off)
        d_pd.step(*FLAT, st_b, st_b["dof_pos"].copy(), off)
    assert np.abs(st_a["contact_force"]).max() > 0   # it has fallen onto the ground by then
    for k in ("root_pos", "root_rot", "dof_pos", "dof_vel", "contact_force"):
        assert np.array_equal(st_a[k], st_b[k]), k
    # ---- torque: a constant elbow torque in free flight, no gravity: the elbow's rate grows by torque / (effective inertia) per second; the torque is
    # the action clipped to +- the motor effort (70 N m for the elbow, humanoid.xml), and the internal torque leaves the angular momentum alone
    d_tq.set_gravity(0.0)
    eff = sc_tq.action_high.astype(np.float32)
    assert eff[9] == 70.0 and np.array_equal(sc_tq.action_low, -sc_tq.action_high)
    rates, finals = [], []
    for a in (0.5, 1.0, 70.0, 1000.0):
        st = make_state(n, z=50.0)
        act = np.zeros((n, 28), np.float32); act[:, 9] = a
        d_tq.step(*FLAT, st, act, off)
        rates.append(float(st["dof_vel"][0, 9])); finals.append(st)
        assert np.abs(st["root_ang_vel"]).max() > 0 and np.all(np.isfinite(st["dof_vel"]))
    assert rates[0] > 0.1 and abs(rates[1] / rates[0] - 2.0) < 0.01, rates                            # linear in the torque ...
    assert all(np.array_equal(finals[2][k], finals[3][k]) for k in ("dof_pos", "dof_vel", "root_ang_vel"))  # ... up to the motor effort: 1000 N m acts as 70
    # ---- vel: the joint rates settle on the clipped action
    d_v, sc_v = _dyn_with_control_mode("vel")
    d_v.set_gravity(0.0)
    assert np.allclose(sc_v.action_high, 2 * np.pi)
    st = make_state(n, z=50.0)
    act = np.zeros((n, 28), np.float32); act[:, 9] = 1.5; act[:, 13] = -100.0    # elbows: 1.5 rad/s; -100 clips to -2 pi
    act[:, 24] = 0.5                                                              # a knee
    for _ in range(4):
        d_v.step(*FLAT, st, act, off)
    assert abs(st["dof_vel"][0, 9] - 1.5) < 0.05 and abs(st["dof_vel"][0, 13] + 2 * np.pi) < 0.2 and abs(st["dof_vel"][0, 24] - 0.5) < 0.05, st["dof_vel"][0, [9, 13, 24]]
    # ---- pd_exp: with gains small enough for an explicit torque held over a control step, it tracks the implicit pd drive; the target is NOT clipped
    d_e, sc_e = _dyn_with_control_mode("pd_exp")
    d_i, _ = _dyn_with_control_mode("pd")
    for dd in (d_e, d_i):
        dd.set_gravity(0.0); dd.scale_gains(0.02)
    tgt = np.zeros((n, 28), np.float32); tgt[:, 9] = 0.8; tgt[:, 17] = 0.6; tgt[:, 0:3] = [0.2, -0.1, 0.15]; tgt[:, 3:6] = [0.0, 0.3, 0.0]
    st_e = make_state(n, z=50.0); st_i = make_state(n, z=50.0)
    for _ in range(10):
        d_e.step(*FLAT, st_e, tgt, off); d_i.step(*FLAT, st_i, tgt, off)
    moved = np.abs(st_i["dof_pos"]).max()
    assert moved > 0.05 and np.abs(st_e["dof_pos"] - st_i["dof_pos"]).max() < 0.12 * moved, (moved, np.abs(st_e["dof_pos"] - st_i["dof_pos"]).max())
    big = tgt.copy(); big[:, 9] = 50.0        # far outside the pd bounds: pd clips it to 2.52 rad, pd_exp goes the shorter way round to 50 rad (mod 2 pi)
    st_e = make_state(n, z=50.0); st_i = make_state(n, z=50.0)
    st_e["dof_pos"][:, 9] = 1.0; st_i["dof_pos"][:, 9] = 1.0   # (mid range: the joint limit stays out of it)
    d_e.step(*FLAT, st_e, big, off); d_i.step(*FLAT, st_i, big, off)
    want = 49.0 - 2 * np.pi * np.round(49.0 / (2 * np.pi))    # -1.265 rad: the elbow is driven the other way
    assert want < 0 and st_e["dof_vel"][0, 9] < -0.05 and st_i["dof_vel"][0, 9] > 0.05, (st_e["dof_vel"][0, 9], st_i["dof_vel"][0, 9])


def _hinge_chain(sc, control_mode):
    """DynOracle of a three-link chain with two hinge joints (about y), free-floating base: the smallest character pd_1d accepts."""
    from oracle.binding_dyn import DynOracle
    from parc_amd import lib as L
    from parc_amd.envs import scene
    cfg = L.ParcEnvConfig.from_buffer_copy(bytes(sc.cfg))
    m = cfg.model
    m.num_bodies = 3; m.dof_size = 2
    for b, (par, jt, di) in enumerate([(-1, 0, 0), (0, 1, 0), (1, 1, 1)]):   # joint types of parc_dynamics.hpp: 0 root, 1 hinge
        m.parent[b] = par; m.joint_type[b] = jt; m.dof_idx[b] = di
        for a in range(3):
            m.local_translation[b][a] = [0.0, 0.0, -0.4][a] if b > 0 else 0.0
            m.joint_axis[b][a] = [0.0, 1.0, 0.0][a]
        for a in range(4):
            m.local_rotation[b][a] = [0.0, 0.0, 0.0, 1.0][a]
    dp = cfg.dynamics
    dp.num_geoms = 3
    for g in range(3):   # a capsule along -z per link
        dp.geom_body[g] = g; dp.geom_type[g] = 2; dp.geom_density[g] = 1000.0
        for a in range(3):
            dp.geom_pos[g][a] = 0.0; dp.geom_pos2[g][a] = [0.0, 0.0, -0.35][a]; dp.geom_size[g][a] = [0.05, 0.0, 0.0][a]
    for d in range(2):
        dp.dof_stiffness[d] = 60.0; dp.dof_damping[d] = 6.0; dp.dof_armature[d] = 0.01; dp.dof_effort[d] = 40.0
        dp.dof_lower[d] = -3.0; dp.dof_upper[d] = 3.0
        cfg.action_low[d] = -40.0 if control_mode == "torque" else -4.0
        cfg.action_high[d] = 40.0 if control_mode == "torque" else 4.0
    dp.control_mode = scene.CONTROL_MODES[control_mode]
    return DynOracle(cfg)


def _chain_state(n, q, qd):
    st = dict(root_pos=np.zeros((n, 3), np.float32), root_rot=np.zeros((n, 4), np.float32), root_vel=np.zeros((n, 3), np.float32),
              root_ang_vel=np.zeros((n, 3), np.float32), dof_pos=np.tile(np.asarray(q, np.float32), (n, 1)), dof_vel=np.tile(np.asarray(qd, np.float32), (n, 1)),
              contact_force=np.zeros((n, 3, 3), np.float32))
    st["root_rot"][:, 3] = 1.0; st["root_pos"][:, 2] = 50.0
    return st


def test_control_mode_pd_1d_on_a_hinge_chain(dyn):
    """pd_1d (ig_char_env.py:411-421, asserted to be a character of 1-dof joints :246-250): torque = kp (target - dof) - kd dof_vel from the state at
    the start of the control step, limited to the motor effort, target = the action as given.  On a two-hinge chain: (1) the step equals the torque
    mode's step with that torque as the action, bit for bit; (2) pd_exp differs from it exactly when the plain difference and the rotation
    difference differ (|target - dof| > pi: pd_exp goes the shorter way round)."""
    _, sc = dyn
    n = 2
    off = np.zeros((n, 3), np.float32)
    d1, dt_, de = _hinge_chain(sc, "pd_1d"), _hinge_chain(sc, "torque"), _hinge_chain(sc, "pd_exp")
    for d in (d1, dt_, de):
        d.set_gravity(0.0)
    q0, qd0 = [0.3, -0.2], [0.5, -1.0]
    for tgt in ([0.8, -0.6], [2.5, 1.0], [9.0, -0.2]):        # the last one: out of the bounds a pd target would be clipped to, and 8.7 rad away
        a = np.tile(np.asarray(tgt, np.float32), (n, 1))
        s1, s2, s3 = _chain_state(n, q0, qd0), _chain_state(n, q0, qd0), _chain_state(n, q0, qd0)
        tau = np.clip(np.float32(60.0) * (a - s1["dof_pos"]) - np.float32(6.0) * s1["dof_vel"], -40.0, 40.0).astype(np.float32)
        d1.step(*FLAT, s1, a, off); dt_.step(*FLAT, s2, tau, off); de.step(*FLAT, s3, a, off)
        assert np.all(np.isfinite(s1["dof_vel"])) and np.abs(s1["dof_vel"] - np.asarray(qd0, np.float32)).max() > 0.05
        for k in ("dof_pos", "dof_vel", "root_pos", "root_rot", "root_vel", "root_ang_vel"):
            assert np.array_equal(s1[k], s2[k]), (tgt, k)                              # (1)
        if abs(tgt[0] - q0[0]) <= np.pi:                                               # (2) within half a turn the two differences coincide ...
            assert np.array_equal(s1["dof_vel"], s3["dof_vel"]), tgt
    # ... (9.0 - 0.3 = 2 pi + 2.42 rad also gives the same step: both torques sit at the motor limit, on the same side) ... and beyond it they part:
    s_a, s_b = _chain_state(n, q0, qd0), _chain_state(n, q0, qd0)
    far = np.tile(np.asarray([0.3 + 4.0, -0.2], np.float32), (n, 1))                  # 4.0 rad ahead = 2.28 rad behind, the shorter way
    d1.step(*FLAT, s_a, far, off); de.step(*FLAT, s_b, far, off)
    assert s_a["dof_vel"][0, 0] > qd0[0] and s_b["dof_vel"][0, 0] < qd0[0], (s_a["dof_vel"][0], s_b["dof_vel"][0])


def test_dof_drive_pd_feedforward_and_limit_spring():
    """The joint model that the three solvers share (parc_dynamics.hpp, THE JOINT MODEL): the drive of one dof in a substep -- implicit pd or the
    feed-forward torque of the other control modes, then the joint-limit spring -- and the control law of a hinge and of a spherical joint, against
    the formulas written out here in fp32, bit for bit (the host build rounds every operation separately, like numpy's float32 scalars).  The
    formulas are the statements the solvers carried before they shared them: t = kp e - (kd + dt kp) qd limited to +-eff, aug = arm + dt kd +
    dt^2 kp; not pd: t = ff - [vel: kd] qd limited to +-eff, aug = arm + dt [vel: kd]; outside [lo, hi] the spring adds lim_k (lim - cur) - lim_d qd
    to the torque -- after the motor limit -- and dt lim_d + dt^2 lim_k to the augmentation."""
    from oracle.binding_dyn import JointModel
    from parc_amd.envs import scene
    jm = JointModel()
    f = np.float32
    PD, VEL, TORQUE, PD_EXP, PD_1D = (scene.CONTROL_MODES[k] for k in ("pd", "vel", "torque", "pd_exp", "pd_1d"))

    def clampf(x, lo, hi):
        return lo if x < lo else (hi if x > hi else x)

    def ctrl_ff(ctrl, kp, kd, eff, alo, ahi, a, diff, qd0):
        if ctrl == VEL:
            return kd * clampf(a, alo, ahi)
        if ctrl == TORQUE:
            return clampf(a, alo, ahi)
        return clampf(kp * diff - kd * qd0, -eff, eff)

    def hinge_diff(ctrl, a, hang):
        d = a - hang
        if ctrl == PD_EXP:
            d = d - f(6.28318530717958648) * np.rint(d * f(0.159154943091895336))
        return d

    def drive(ctrl, kp, kd, arm, eff, lo, hi, lim_k, lim_d, dt, e, cur, qd):
        t = kp * e - (kd + dt * kp) * qd
        t = clampf(t, -eff, eff)
        aug = arm + dt * kd + dt * dt * kp
        if ctrl != PD:
            kdv = kd if ctrl == VEL else f(0.0)
            t = clampf(e - kdv * qd, -eff, eff)
            aug = arm + dt * kdv
        if cur < lo:
            t = t + (lim_k * (lo - cur) - lim_d * qd); aug = aug + (dt * lim_d + dt * dt * lim_k)
        elif cur > hi:
            t = t + (lim_k * (hi - cur) - lim_d * qd); aug = aug + (dt * lim_d + dt * dt * lim_k)
        return t, aug

    def same(got, want, what):
        got, want = np.asarray(got), np.asarray(want)
        assert got.dtype == np.float32 and want.dtype == np.float32, what
        assert np.array_equal(got, want), (what, got, want)

    kp, kd, arm, eff, lo, hi = f(300.7), f(30.3), f(0.0123), f(150.5), f(-1.1), f(2.3)
    lim_k, lim_d, dt = f(1234.5), f(12.7), f(1.0 / 120.0)
    G = (kp, kd, arm, eff, lo, hi, lim_k, lim_d, dt)
    # ---- pd: in range, beyond either limit, at the motor limit (with and without the spring on top)
    for name, e, cur, qd in [("in range", 0.1, 0.3, 0.7), ("below lo", 0.1, -1.4, 0.7), ("above hi", -0.2, 2.6, -0.4), ("at lo", 0.1, -1.1, 0.7),
                             ("+eff", 1.0, 0.3, 0.7), ("-eff", -1.0, 0.3, 0.7), ("+eff and spring", 1.0, 2.9, 0.7), ("-eff and spring", -1.0, -1.6, -2.0)]:
        e, cur, qd = f(e), f(cur), f(qd)
        got, want = jm.dof_drive(PD, *G, e, cur, qd), drive(PD, *G, e, cur, qd)
        same(got, want, ("pd", name))
        t0 = clampf(kp * e - (kd + dt * kp) * qd, -eff, eff); a0 = arm + dt * kd + dt * dt * kp
        if name in ("in range", "at lo"):
            assert got[0] == t0 and abs(got[0]) < eff and got[1] == a0, name
        elif "eff" in name and "spring" not in name:
            assert got[0] == (eff if name[0] == "+" else -eff) and got[1] == a0, name
        else:
            lim = lo if cur < lo else hi
            assert got[0] == t0 + (lim_k * (lim - cur) - lim_d * qd) and got[0] != t0, name
            assert got[1] == a0 + (dt * lim_d + dt * dt * lim_k) and got[1] > a0, name
            if "spring" in name:
                assert abs(got[0]) > eff, name          # the spring is not a motor: it acts on top of the limited torque
    # ---- the other modes on a hinge: control law (action inside / outside its bounds), then the drive with that torque
    alo, ahi = f(-2.0), f(2.5)
    for ctrl in (VEL, TORQUE, PD_EXP, PD_1D, PD):
        for a in (0.4, -7.0, 9.0):
            for pos, vel in [(0.3, 0.7), (-1.4, -0.5), (2.6, 3.0)]:
                a_, pos_, vel_ = f(a), f(pos), f(vel)
                hang, qd, th = jm.control_hinge(ctrl, kp, kd, eff, alo, ahi, pos_, vel_, a_)
                want = clampf(a_, alo, ahi) if ctrl == PD else ctrl_ff(ctrl, kp, kd, eff, alo, ahi, a_, hinge_diff(ctrl, a_, pos_), vel_)
                same([hang, qd, th], [pos_, vel_, want], ("hinge control", ctrl, a, pos))
                e = th - hang if ctrl == PD else th
                same(jm.dof_drive(ctrl, *G, e, hang, qd), drive(ctrl, *G, e, hang, qd), ("hinge drive", ctrl, a, pos))
    assert jm.control_hinge(VEL, kp, kd, eff, alo, ahi, f(0), f(0), f(9.0))[2] == kd * ahi            # clipped to the bounds, times the damping
    assert jm.control_hinge(TORQUE, kp, kd, eff, alo, ahi, f(0), f(0), f(-7.0))[2] == alo
    t_v, aug_v = jm.dof_drive(VEL, *G, f(20.0), f(0.3), f(0.7))
    t_t, aug_t = jm.dof_drive(TORQUE, *G, f(20.0), f(0.3), f(0.7))
    assert t_v == f(20.0) - kd * f(0.7) and aug_v == arm + dt * kd and t_t == f(20.0) and aug_t == arm   # only vel keeps a damping, implicit
    # ---- pd_exp takes a hinge's difference the shorter way round, pd_1d subtracts: across +-pi they part (soft gains: neither at the motor limit)
    skp, skd = f(20.3), f(1.7)
    for pos, a in [(3.0, -3.0), (-3.1, 3.1), (0.5, 0.5 + 3.2), (0.5, 0.5 - 3.2), (0.5, 0.5 + 3.1)]:
        pos_, a_ = f(pos), f(a)
        t_e = jm.control_hinge(PD_EXP, skp, skd, eff, alo, ahi, pos_, f(0.3), a_)[2]
        t_1 = jm.control_hinge(PD_1D, skp, skd, eff, alo, ahi, pos_, f(0.3), a_)[2]
        same(t_e, ctrl_ff(PD_EXP, skp, skd, eff, alo, ahi, a_, hinge_diff(PD_EXP, a_, pos_), f(0.3)), ("pd_exp", pos, a))
        same(t_1, ctrl_ff(PD_1D, skp, skd, eff, alo, ahi, a_, a_ - pos_, f(0.3)), ("pd_1d", pos, a))
        assert abs(t_e) < eff and abs(t_1) < eff
        if abs(a - pos) > np.pi:
            assert np.sign(t_e) == -np.sign(t_1) and abs(skp * hinge_diff(PD_EXP, a_, pos_)) < skp * f(np.pi), (pos, a, t_e, t_1)
        else:
            assert t_e == t_1, (pos, a)
    # ---- a spherical joint: three dofs with gains of their own
    kp3, kd3, eff3 = np.array([300.7, 20.3, 500.1], np.float32), np.array([30.3, 1.7, 50.9], np.float32), np.array([150.5, 40.0, 2.5], np.float32)
    lo3, hi3 = np.array([-1.2, -0.5, -2.0], np.float32), np.array([1.0, 0.7, 2.5], np.float32)
    pos, vel = np.array([0.3, -0.4, 0.2], np.float32), np.array([0.7, -1.5, 0.1], np.float32)
    for a in (np.array([0.2, 0.1, -0.3], np.float32), np.array([3.0, -0.9, 0.4], np.float32)):    # inside the bounds; two components outside
        clipped = np.minimum(np.maximum(a, lo3), hi3)
        for ctrl in (PD, VEL, TORQUE, PD_EXP):
            jq, qd, tq = jm.control_spherical(ctrl, kp3, kd3, eff3, lo3, hi3, pos, vel, a)
            same(jq, jm.qexp(pos), ("jq", ctrl)); same(qd, vel, ("qd", ctrl))
            if ctrl == PD:
                want = jm.qexp(clipped)
                assert not np.array_equal(want, jm.qexp(a)) or np.array_equal(a, clipped)
            else:
                diff = jm.rot_diff(pos, a) if ctrl == PD_EXP else np.zeros(3, np.float32)          # the action as given, not the clipped one
                want = np.array([ctrl_ff(ctrl, kp3[k], kd3[k], eff3[k], lo3[k], hi3[k], a[k], diff[k], vel[k]) for k in range(3)] + [f(1.0)], np.float32)
                if ctrl == PD_EXP:
                    assert abs(want[2]) == eff3[2] and abs(want[1]) < eff3[1]                       # one dof at its motor limit, one not
            same(tq, want, ("tq", ctrl, a))
    # (the primitives behind it mean what they say: exp map -> quaternion, and the rotation between two poses about one axis is the difference)
    ang = np.linalg.norm(pos.astype(np.float64))
    assert np.abs(jm.qexp(pos) - np.append(np.sin(ang / 2) * pos / ang, np.cos(ang / 2))).max() < 1e-6
    assert np.abs(jm.rot_diff(np.array([0, 0.3, 0], np.float32), np.array([0, 1.1, 0], np.float32)) - [0, 0.8, 0]).max() < 1e-6
