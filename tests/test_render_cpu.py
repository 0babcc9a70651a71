"""Renderer tests that need no GPU: the numpy reference ray-caster against analytic scenes, the PNG writer, the camera placement and the
C layout of ParcRenderParams (parc_env_render validates it before any device call)."""
import ctypes as C
import math
import struct
import zlib

import numpy as np
import pytest

import render_ref as RR
from parc_amd import lib as L
from parc_amd import render as R
from parc_amd.util.frame_writer import encode_png


def _flat(h, n=21, d=0.5):
    return RR.Terrain(np.full((n, n), h), -n * d / 2, -n * d / 2, d, d)


def test_flat_terrain_straight_down_depth_is_the_height_above_the_ground():
    ter = _flat(0.3)
    eye, W, H = np.array([0.1, -0.2, 4.0]), 16, 12
    depth, ids, _ = RR.render(ter, [], eye, eye - [0, 0, 1], W, H, math.radians(40))
    D = RR.camera_rays(eye, eye - [0, 0, 1], W, H, math.radians(40))
    assert (ids == RR.TOP).all()
    # along each ray: depth * |dir_z| = eye height - h, at every pixel (ray distance, not z-depth)
    np.testing.assert_allclose(depth * -D[..., 2], 4.0 - 0.3, rtol=0, atol=1e-12)
    # the view straight down uses the f x y fallback of the basis: image up = +y, image right = +x
    assert D[0, W // 2, 1] > 0 and D[H // 2, W - 1, 0] > 0


def test_single_raised_column_top_and_wall_pixels_fall_where_the_projection_says():
    n, d = 21, 0.5
    hf = np.zeros((n, n)); hf[10, 10] = 1.0       # cell (10, 10): centre (0, 0), x, y in [-0.25, 0.25], top 1.0
    ter = RR.Terrain(hf, -n * d / 2, -n * d / 2, d, d)
    eye, tgt, W, H, fov = np.array([0.0, -4.0, 2.0]), np.array([0.0, 0.0, 0.5]), 64, 48, math.radians(40)
    depth, ids, _ = RR.render(ter, [], eye, tgt, W, H, fov)
    f, r, u = R.camera_basis(eye, tgt)
    th = math.tan(fov / 2)

    def pixel(p):  # projection of a world point to (column, row)
        v = p - eye
        sx, sy = v @ r / (v @ f), v @ u / (v @ f)
        return sx / (th * W / H) * W / 2 + W / 2 - 0.5, (1 - sy / th) * H / 2 - 0.5

    cx, cy_top = pixel(np.array([0.0, 0.0, 1.0]))          # centre of the top face
    _, cy_wall = pixel(np.array([0.0, -0.25, 0.5]))        # middle of the wall facing the camera
    assert ids[round(cy_top), round(cx)] == RR.TOP and ids[round(cy_wall), round(cx)] == RR.WALL
    # the wall pixel's depth is the distance to the plane y = -0.25
    D = RR.camera_rays(eye, tgt, W, H, fov)[round(cy_wall), round(cx)]
    assert abs(depth[round(cy_wall), round(cx)] - (-0.25 - eye[1]) / D[1]) < 1e-12
    # a column of pixels beside the cell sees only the ground (top faces at height 0) and sky
    _, cy_side = pixel(np.array([0.6, -0.25, 0.5]))
    assert ids[round(cy_side), round(pixel(np.array([0.6, -0.25, 0.5]))[0])] == RR.TOP
    # the wall occupies the rows between the projected top edge and bottom edge of the front face
    _, y_top_edge = pixel(np.array([0.0, -0.25, 1.0]))
    _, y_bot_edge = pixel(np.array([0.0, -0.25, 0.0]))
    col = ids[:, round(cx)]
    rows = np.nonzero(col == RR.WALL)[0]
    assert rows.min() >= math.floor(y_top_edge) and rows.max() <= math.ceil(y_bot_edge)
    assert len(rows) >= round(y_bot_edge - y_top_edge) - 1


def test_sphere_centre_pixel_depth():
    c, rad = np.array([0.3, 2.0, 1.0]), 0.25
    eye = np.array([0.3, -3.0, 1.0])
    W = H = 15
    depth, ids, _ = RR.render(_flat(-5.0), [dict(type=RR.SPHERE, a=c, s=[rad, 0, 0], id=16 + 3)], eye, c, W, H, math.radians(30))
    assert ids[H // 2, W // 2] == 19
    assert abs(depth[H // 2, W // 2] - (np.linalg.norm(c - eye) - rad)) < 1e-12


def test_capsule_and_box_primitives():
    eye = np.array([0.0, -3.0, 0.0])
    D = RR.camera_rays(eye, [0, 0, 0], 9, 9, math.radians(20)).reshape(-1, 3)
    O = np.broadcast_to(eye, D.shape).copy()
    # capsule along x through the origin, radius 0.2: the centre ray enters the cylinder side at y = -0.2
    t, n = RR.prim_hit(dict(type=RR.CAPSULE, a=[-0.5, 0, 0], b=[0.5, 0, 0], s=[0.2, 0, 0]), O, D)
    assert abs(t[40] - 2.8) < 1e-12 and np.allclose(n[40], [0, -1, 0])
    # seen along its axis, the capsule is its end sphere
    t2, _ = RR.prim_hit(dict(type=RR.CAPSULE, a=[0, 0.5, 0], b=[0, 1.5, 0], s=[0.2, 0, 0]), O, D)
    assert abs(t2[40] - (3.5 - 0.2)) < 1e-12
    # a box turned 90 degrees about z: half extent 0.3 along world y
    q = [0, 0, math.sin(math.pi / 4), math.cos(math.pi / 4)]
    t3, n3 = RR.prim_hit(dict(type=RR.BOX, a=[0, 0, 0], s=[0.3, 0.1, 0.1], q=q), O, D)
    assert abs(t3[40] - 2.7) < 1e-9 and np.allclose(n3[40], [0, -1, 0], atol=1e-9)


def test_png_writer_round_trips():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, size=(7, 11, 4), dtype=np.uint8)
    data = encode_png(img)
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, {}
    while pos < len(data):
        (n,) = struct.unpack(">I", data[pos:pos + 4])
        tag, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        (crc,) = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(tag + body) & 0xFFFFFFFF
        chunks[tag] = chunks.get(tag, b"") + body
        pos += 12 + n
    w, h, depth, ctype, _, _, _ = struct.unpack(">IIBBBBB", chunks[b"IHDR"])
    assert (w, h, depth, ctype) == (11, 7, 8, 6) and b"IEND" in chunks
    raw = np.frombuffer(zlib.decompress(chunks[b"IDAT"]), np.uint8).reshape(7, 1 + 11 * 4)
    assert (raw[:, 0] == 0).all()
    assert np.array_equal(raw[:, 1:].reshape(7, 11, 4), img)


def test_track_and_still_camera_placement():
    eye, tgt = R.track_camera([1.0, 2.0, 0.9], [1000.0, -4.0, 0.0])
    assert np.allclose(tgt, [1001.0, -2.0, 0.9]) and np.allclose(eye, [1001.0, -7.0, 2.9])   # default offset (0, -5, 2)
    eye, tgt = R.track_camera([1.0, 2.0, 0.9], [0.0, 0.0, 0.0], offset=(3.0, 0.0, 1.0))
    assert np.allclose(eye, [4.0, 2.0, 1.9]) and np.allclose(tgt, [1.0, 2.0, 0.9])
    eye, tgt = R.still_camera([8.0, 4.0, 0.0], eye=(0.0, -5.0, 3.0), target=(0.0, 0.0, 1.0))
    assert np.allclose(eye, [8.0, -1.0, 3.0]) and np.allclose(tgt, [8.0, 4.0, 1.0])
    f, r, u = R.camera_basis([0, -5, 2], [0, 0, 2])   # looking along +y: right = +x, up = +z
    assert np.allclose(f, [0, 1, 0]) and np.allclose(r, [1, 0, 0]) and np.allclose(u, [0, 0, 1])
    p = R.make_params(320, 240, {"mode": "still", "eye": (1, 2, 3)}, draw_ref=False)
    assert p.camera_mode == L.CAMERA_STILL and list(p.eye) == [1, 2, 3] and p.draw_ref == 0 and p.shadows == 1
    assert list(p.offset) == list(R.DEFAULT_TRACK_OFFSET)
    with pytest.raises(ValueError):
        R.make_params(320, 240, {"mode": "orbit"})


def test_render_params_layout_matches_c_and_is_checked_before_the_device():
    """parc_env_render checks struct_size first: a mirror that is off by 4 bytes is refused with the ABI-mismatch error, no GPU needed."""
    lib = L.load()
    assert C.sizeof(L.ParcRenderParams) == 4 * (4 + 3 + 3 + 3 + 1 + 3 + 3 + 3)
    assert L.ParcRenderParams.fov_y.offset == 4 * 13 and L.ParcRenderParams.draw_ref.offset == 4 * 20
    bad = R.make_params(64, 48)
    bad.struct_size = C.sizeof(L.ParcRenderParams) - 4
    rc = lib.parc_env_render(None, C.byref(bad), None, 1, None, None, None, None)
    assert rc == -1 and b"ParcRenderParams ABI mismatch" in lib.parc_last_error()
    good = R.make_params(64, 48)
    rc = lib.parc_env_render(None, C.byref(good), None, 1, None, None, None, None)
    assert rc == -1 and b"null env" in lib.parc_last_error()
