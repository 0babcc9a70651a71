"""Host side of the headless renderer (``parc_env_render``, ``parc_amd/csrc/parc_render.hpp``): camera defaults and the parameter block.

The camera is formed on the device from the state (no host sync); :func:`track_camera` states the same placement on the host for
documentation and tests.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np

from parc_amd import lib as L

# The reference's tracking camera (ig_char_env.py:511-538) sits 5 m behind the character (-y) at an ABSOLUTE height of 3 m, which is under
# the ground on raised terrain; here the eye follows the root: eye = root + offset.  A deliberate deviation.
DEFAULT_TRACK_OFFSET = (0.0, -5.0, 2.0)
DEFAULT_STILL_EYE = (0.0, -5.0, 3.0)
DEFAULT_STILL_TARGET = (0.0, 0.0, 1.0)
DEFAULT_FOV_Y = math.radians(50.0)
DEFAULT_SUN_DIR = (0.35, -0.45, 0.82)
CAMERA_MODES = {"track": L.CAMERA_TRACK, "still": L.CAMERA_STILL}


def make_params(width, height, cam=None, draw_ref=True, shadows=True) -> L.ParcRenderParams:
    """``cam``: dict with any of ``mode`` ("track" | "still"), ``offset``, ``eye``, ``target``, ``fov_y`` (radians), ``sun_dir``,
    ``debug_visuals``, ``ref_offset``; missing keys take the defaults above."""
    cam = dict(cam or {})
    mode = cam.get("mode", "track")
    if mode not in CAMERA_MODES:
        raise ValueError(f"camera mode must be one of {sorted(CAMERA_MODES)}, got {mode!r}")
    p = L.ParcRenderParams()
    p.struct_size = ctypes.sizeof(L.ParcRenderParams)
    p.width, p.height = int(width), int(height)
    p.camera_mode = CAMERA_MODES[mode]
    for name, default in (("offset", DEFAULT_TRACK_OFFSET), ("eye", DEFAULT_STILL_EYE), ("target", DEFAULT_STILL_TARGET),
                          ("sun_dir", DEFAULT_SUN_DIR), ("ref_offset", (0.0, 0.0, 0.0))):
        v = cam.get(name, default)
        if len(v) != 3:
            raise ValueError(f"camera {name} needs three components")
        getattr(p, name)[:] = [float(x) for x in v]
    p.fov_y = float(cam.get("fov_y", DEFAULT_FOV_Y))
    p.draw_ref = int(bool(draw_ref))
    p.shadows = int(bool(shadows))
    p.debug_visuals = int(bool(cam.get("debug_visuals", False)))
    return p


def track_camera(root_pos_local, env_offset, offset=DEFAULT_TRACK_OFFSET):
    """World eye / target of the track camera: target = the env's root in world coordinates (root + env origin), eye = target + offset."""
    target = np.asarray(root_pos_local, np.float64) + np.asarray(env_offset, np.float64)
    return target + np.asarray(offset, np.float64), target


def still_camera(env_offset, eye=DEFAULT_STILL_EYE, target=DEFAULT_STILL_TARGET):
    """World eye / target of the still camera: both given relative to the env's origin."""
    o = np.asarray(env_offset, np.float64)
    return o + np.asarray(eye, np.float64), o + np.asarray(target, np.float64)


def camera_basis(eye, target):
    """forward, right, up of the camera (float64; the kernel's convention, parc_render.hpp header): r = f x z, or f x y when f is
    vertical; u = r x f."""
    f = np.asarray(target, np.float64) - np.asarray(eye, np.float64)
    f = f / np.linalg.norm(f)
    r = np.cross(f, [0.0, 0.0, 1.0])
    if np.linalg.norm(r) < 1e-6:
        r = np.cross(f, [0.0, 1.0, 0.0])
    r = r / np.linalg.norm(r)
    return f, r, np.cross(r, f)
