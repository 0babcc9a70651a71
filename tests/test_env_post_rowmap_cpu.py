"""Row phase of k_env_post: the (pass, lane) -> (row, slot) mapping of parc_amd/csrc/parc_rowmap.hpp, from a host build of the header the
kernel includes (no GPU).  Pass A holds every root item (slot 0 = root rotation, slot 15 = root position) and the first 48 joint items,
pass B joint items only; the joint quotient j / (B - 1) is a multiply-shift."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import REPO

SHIM = r"""
#include "parc_rowmap.hpp"
extern "C" unsigned rowmap_mul(int B) { return parc_rowmap_mul(B); }
extern "C" int rowmap_mul_ok(int B, unsigned mul) { return parc_rowmap_mul_ok(B, mul) ? 1 : 0; }
extern "C" int rowmap_item(int pass, int lane, int B, int rows, unsigned mul) {
    return pass == 0 ? parc_rowmap_item<true>(lane, B, rows, mul) : parc_rowmap_item<false>(lane, B, rows, mul);
}
extern "C" int rowmap_max_joint_items(void) { return PARC_ROWMAP_MAX_JOINT_ITEMS; }
"""


@pytest.fixture(scope="module")
def rowmap(tmp_path_factory):
    d = tmp_path_factory.mktemp("rowmap")
    src = d / "rowmap_host.cpp"
    src.write_text(SHIM)
    so = d / "librowmap_host.so"
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-fPIC", "-shared", "-std=c++17", "-Wall", "-Werror",
                           "-I", os.path.join(REPO, "parc_amd", "csrc"), "-o", str(so), str(src)])
    lib = C.CDLL(str(so))
    lib.rowmap_mul.restype = C.c_uint
    lib.rowmap_mul.argtypes = [C.c_int]
    lib.rowmap_mul_ok.argtypes = [C.c_int, C.c_uint]
    lib.rowmap_item.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint]
    return lib


def _items(lib, p, B, S):
    """[(lane, row, slot)] of the live lanes of pass p."""
    mul = lib.rowmap_mul(B)
    out = []
    for lane in range(64):
        item = lib.rowmap_item(p, lane, B, 2 + S, mul)   # row * 16 + slot, -1 = idle lane
        assert item == -1 or 0 <= item < 128, (p, lane, item)
        if item >= 0:
            out.append((lane, item >> 4, item & 15))
    return out


def test_multiply_shift_quotient_equals_the_division(rowmap):
    assert rowmap.rowmap_max_joint_items() == 112
    for B in range(2, 16):
        mul = rowmap.rowmap_mul(B)
        for j in range(112):
            assert (j * mul) >> 16 == j // (B - 1), (B, j, mul)
            assert j * mul < 2 ** 32, (B, j, mul)       # the kernel's product is a 32-bit unsigned one
        assert rowmap.rowmap_mul_ok(B, mul) == 1
        assert rowmap.rowmap_mul_ok(B, mul - 1) == 0   # the create-time check catches a wrong constant: (B - 1) * (mul - 1) < 65536, so j = B - 1 gives row 0


@pytest.mark.parametrize("B", range(2, 16))
@pytest.mark.parametrize("S", range(0, 7))
def test_every_item_is_visited_exactly_once(rowmap, B, S):
    rows = 2 + S
    a, b = _items(rowmap, 0, B, S), _items(rowmap, 1, B, S)
    seen = [(r, s) for _, r, s in a + b]
    # nothing outside the ranges: rows < 2 + S; slot 0, 15 or a joint 1 <= i < B
    for r, s in seen:
        assert 0 <= r < rows, (r, s)
        assert s in (0, 15) or 1 <= s < B, (r, s)
    # each root item exactly once, and only in pass A
    roots = [(r, s) for _, r, s in a if s in (0, 15)]
    assert sorted(roots) == sorted([(r, 0) for r in range(rows)] + [(r, 15) for r in range(rows)])
    assert not [(r, s) for _, r, s in b if s in (0, 15)]
    # each joint item exactly once
    joints = [(r, s) for r, s in seen if s not in (0, 15)]
    assert sorted(joints) == [(r, i) for r in range(rows) for i in range(1, B)]
    # the layout the kernel relies on: root rotations in lanes 0..7, root positions in lanes 8..15 (row = lane & 7), joint item
    # j = lane - 16 (pass A) / 48 + lane (pass B) in row-major order; rows 0 and 1 (character, reference) never reach pass B
    for lane, r, s in a:
        if lane < 16:
            assert r == (lane & 7) and s == (0 if lane < 8 else 15)
        else:
            assert (r, s) == ((lane - 16) // (B - 1), 1 + (lane - 16) % (B - 1))
    for lane, r, s in b:
        assert (r, s) == (((48 + lane) // (B - 1)), 1 + (48 + lane) % (B - 1))
        assert r >= 2
