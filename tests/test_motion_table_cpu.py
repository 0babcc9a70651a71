"""The motion table of parc_env_load_motions (parc_amd/csrc/parc_motion_table.hpp) from a host build of the header the library includes (no
GPU): the four bundled clips against tests/golden/motion_lib.npz, and the refused clips, which must leave the outputs as they were.
Tolerances: lengths 0 and weights 1e-7, as tests/test_hip_parity.py asserts for the same quantities; the integer tables are exact."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO, golden

SHIM = r"""
#include "parc_motion_table.hpp"
#include <cstring>
// the three vectors start as what the caller passes in (its sentinel); returns 0, or 1 with the message in msg[128]
extern "C" int motion_table(int M, const int32_t *nf, const int32_t *fps, const int32_t *loop, const double *w, const float *root_pos,
                            MotionMeta *meta, float *weights, int meta_len, int *frame_motion, int fm_len, int *fm_len_out, char *msg) {
    std::vector<MotionMeta> vm(meta, meta + meta_len);
    std::vector<float> vw(weights, weights + meta_len);
    std::vector<int> vf(frame_motion, frame_motion + fm_len);
    const char *err = parc_motion_table(M, nf, fps, loop, w, root_pos, vm, vw, vf);
    if (vm.size() != vw.size() || vm.size() > (size_t)meta_len || vf.size() > (size_t)fm_len) return -1;
    *fm_len_out = (int)vf.size();
    memcpy(meta, vm.data(), vm.size() * sizeof(MotionMeta));
    memcpy(weights, vw.data(), vw.size() * sizeof(float));
    memcpy(frame_motion, vf.data(), vf.size() * sizeof(int));
    if (err) { strncpy(msg, err, 127); msg[127] = 0; }
    return err ? 1 : 0;
}
extern "C" int motion_meta_bytes(void) { return (int)sizeof(MotionMeta); }
"""
META = np.dtype([("start", "i4"), ("nframes", "i4"), ("length", "f4"), ("loop", "i4"), ("dx", "f4"), ("dy", "f4"), ("dz", "f4"), ("fps", "f4")])
RAW_WEIGHTS = [1.0, 1.5, 2.0, 2.5]   # what the golden library was built with (tests/golden/make_golden.py)
CXX = [os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(REPO, "parc_amd", "csrc")]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("motion_table")
    src = d / "motion_table_host.cpp"
    src.write_text(SHIM)
    so = d / "libmotion_table_host.so"
    subprocess.check_call(CXX + ["-O1", "-fPIC", "-shared", "-o", str(so), str(src)])
    lib = C.CDLL(str(so))
    assert lib.motion_meta_bytes() == META.itemsize == 32
    return lib


def _call(lib, nf, fps, loop, w, root_pos, meta, weights, fm):
    nf, fps, loop = (np.ascontiguousarray(a, np.int32) for a in (nf, fps, loop))
    w = np.ascontiguousarray(w, np.float64)
    root_pos = np.ascontiguousarray(root_pos, np.float32)
    n = C.c_int(-1)
    msg = C.create_string_buffer(128)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = lib.motion_table(len(nf), p(nf), p(fps), p(loop), p(w), p(root_pos), p(meta), p(weights), len(meta), p(fm), len(fm), C.byref(n), msg)
    assert rc in (0, 1)
    return rc, n.value, msg.value.decode()


def _golden_inputs():
    g = golden("motion_lib")
    return g, g["motion_num_frames"], g["motion_fps"], g["motion_loop_modes"], g["frame_root_pos"]


def test_the_bundled_clips_equal_the_golden_library(shim):
    g, nf, fps, loop, rp = _golden_inputs()
    M, F = len(nf), int(rp.shape[0])
    meta = np.zeros(M, META); weights = np.zeros(M, np.float32); fm = np.full(F, -1, np.int32)
    rc, n, msg = _call(shim, nf, fps, loop, RAW_WEIGHTS, rp, meta, weights, fm)
    assert rc == 0 and n == F, msg
    assert np.array_equal(meta["length"], g["motion_lengths"].astype(np.float32)) and g["motion_lengths"].dtype == np.float32   # tolerance 0
    assert np.abs(weights.astype(np.float64) - g["motion_weights"]).max() <= 1e-7
    assert np.array_equal(meta["start"], g["motion_start_idx"]) and np.array_equal(meta["nframes"], nf)
    assert np.array_equal(fm, np.repeat(np.arange(M), nf))
    assert np.array_equal(meta["loop"], loop) and np.array_equal(meta["fps"], fps.astype(np.float32))
    delta = g["motion_root_pos_delta"]
    assert np.array_equal(meta["dx"], delta[:, 0]) and np.array_equal(meta["dy"], delta[:, 1]) and not meta["dz"].any()


@pytest.mark.parametrize("what, message", [("one_frame", "every clip needs at least 2 frames"), ("fps_zero", "fps must be positive"),
                                           ("negative_weight", "motion weights must be >= 0")])
def test_a_refused_clip_leaves_the_outputs_untouched(shim, what, message):
    _, nf, fps, loop, rp = _golden_inputs()
    nf, fps, w = nf.copy(), fps.copy(), list(RAW_WEIGHTS)
    if what == "one_frame":
        nf[-1] = 1           # the LAST clip: everything before it was already accepted
    elif what == "fps_zero":
        fps[-1] = 0
    else:
        w[-1] = -0.5
    M, F = len(nf), int(rp.shape[0])
    meta = np.zeros(M + 2, META); meta.view(np.uint8)[:] = 0xA5
    weights = np.full(M + 2, -7.0, np.float32); fm = np.full(F + 3, -9, np.int32)
    before = meta.copy()
    rc, n, msg = _call(shim, nf, fps, loop, w, rp, meta, weights, fm)
    assert rc == 1 and msg == message
    assert n == F + 3 and meta.tobytes() == before.tobytes() and (weights == -7.0).all() and (fm == -9).all()   # sizes and contents as passed in

