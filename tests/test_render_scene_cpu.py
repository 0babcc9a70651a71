"""Scene render entry point without a GPU: exported and declared, and its argument checks run before any device call."""
import ctypes as C
import os

from parc_amd import lib as L
from parc_amd import render as R

HEADER = os.path.join(os.path.dirname(__file__), "..", "include", "parc_env.h")


def test_render_scene_is_exported_and_declared():
    assert "parc_env_render_scene" in L.EXPORTED_SYMBOLS
    src = open(HEADER).read()
    assert "int parc_env_render_scene(ParcEnv *env, const ParcRenderParams *p, int32_t camera_env," in src
    lib = L.load()
    assert lib.parc_env_render_scene.argtypes[2] is C.c_int32 and len(lib.parc_env_render_scene.argtypes) == 10


def test_render_scene_checks_struct_size_and_env_before_the_device():
    lib = L.load()
    bad = R.make_params(64, 48)
    bad.struct_size = C.sizeof(L.ParcRenderParams) + 4
    rc = lib.parc_env_render_scene(None, C.byref(bad), 0, None, 1, None, None, None, None, None)
    assert rc == -1 and b"ParcRenderParams ABI mismatch" in lib.parc_last_error()
    good = R.make_params(64, 48)
    rc = lib.parc_env_render_scene(None, C.byref(good), 0, None, 1, None, None, None, None, None)
    assert rc == -1 and b"null env" in lib.parc_last_error()
    rc = lib.parc_env_render_scene(None, None, 0, None, 1, None, None, None, None, None)
    assert rc == -1 and b"null ParcRenderParams" in lib.parc_last_error()
