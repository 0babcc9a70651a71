"""Prefetch phase of k_env_post: the per-lane table of parc_amd/csrc/parc_lanetab.hpp, from a host build of the header the kernel includes
(no GPU).  Every field against the expression the kernel evaluated per wave before the table existed, written out here; every index the
table yields inside its record / tile / buffer, also on the lanes that have no item of their own (the kernel loads there too, without a
branch)."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import REPO

SHIM = r"""
#include "parc_lanetab.hpp"
extern "C" unsigned rowmap_mul(int B) { return parc_rowmap_mul(B); }
extern "C" int rowmap_item(int pass, int lane, int B, int rows, unsigned mul) {
    return pass == 0 ? parc_rowmap_item<true>(lane, B, rows, mul) : parc_rowmap_item<false>(lane, B, rows, mul);
}
extern "C" int lanetab_entry_bytes(void) { return (int)sizeof(ParcLaneEntry); }
extern "C" int lanetab_fill(unsigned *tab, int B, int S, int D, int R, int tile_r, unsigned row_mul, unsigned tile_mul) {
    return parc_lanetab_fill(reinterpret_cast<ParcLaneEntry *>(tab), B, S, D, R, tile_r, row_mul, tile_mul) ? 1 : 0;
}
// fields of one entry, in the order of FIELDS below
extern "C" void lanetab_fields(const unsigned *w, int *out) {
    int n = 0;
    out[n++] = parc_lt_item(w, 0); out[n++] = parc_lt_item(w, 1);
    for (int k = 0; k < 3; ++k) out[n++] = (int)parc_lt_src4(w, k);
    out[n++] = (int)parc_lt_row_slot(w, 0); out[n++] = (int)parc_lt_row_slot(w, 1);
    out[n++] = (int)parc_lt_cv_slot0(w); out[n++] = (int)parc_lt_cv_slot1(w);
    out[n++] = (int)parc_lt_role(w); out[n++] = (int)parc_lt_force_off(w); out[n++] = (int)parc_lt_dof(w);
    for (int i = 0; i < PARC_LANETAB_TILE_CELLS; ++i) { out[n++] = (int)parc_lt_cell_a(w, i); out[n++] = (int)parc_lt_cell_b(w, i); out[n++] = (int)parc_lt_cell_valid(w, i); }
    out[n++] = (int)parc_lt_nray(w);
}
// the ray clamp of the kernel's prefetch: byte offset of slot i, -1 = the slot is not loaded
extern "C" int lanetab_ray_off(int lane, int R, int i) {
    const int top = parc_lt_ray_top(R, i);
    return top >= 0 ? (int)parc_lt_ray_off(lane, i, top) : -1;
}
"""
NFIELDS = 12 + 15 + 1
REC_F4, REC_Q_CONTACT, REC_Q_VEL = 32, 16, 20   # parc_env_tables.hpp: a frame record = 32 float4; #16..19 contacts, #20.. root_vel, root_ang_vel, dof_vel


@pytest.fixture(scope="module")
def lanetab(tmp_path_factory):
    d = tmp_path_factory.mktemp("lanetab")
    src = d / "lanetab_host.cpp"
    src.write_text(SHIM)
    so = d / "liblanetab_host.so"
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-fPIC", "-shared", "-std=c++17", "-Wall", "-Werror",
                           "-I", os.path.join(REPO, "parc_amd", "csrc"), "-o", str(so), str(src)])
    lib = C.CDLL(str(so))
    lib.rowmap_mul.restype = C.c_uint
    lib.rowmap_mul.argtypes = [C.c_int]
    lib.rowmap_item.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint]
    lib.lanetab_fill.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_uint]
    lib.lanetab_fields.argtypes = [C.c_void_p, C.c_void_p]
    assert lib.lanetab_entry_bytes() == 16
    return lib


def _tile_mul(tile_r):
    """parc_env_load_terrain's multiplier: idx / TW == (idx * mul) >> 16 for every cell of the tile."""
    return (65536 + 2 * tile_r) // (2 * tile_r + 1) if tile_r >= 0 else 0


def _table(lib, B, S, D, R, tile_r):
    tab = (C.c_uint * (4 * 64))()
    assert lib.lanetab_fill(tab, B, S, D, R, tile_r, lib.rowmap_mul(B), _tile_mul(tile_r)) == 1
    out = (C.c_int * NFIELDS)()
    rows = []
    for lane in range(64):
        lib.lanetab_fields(C.byref(tab, 16 * lane), out)
        rows.append(list(out))
    return rows


@pytest.mark.parametrize("B", range(2, 16))
def test_every_field_equals_the_expression_the_kernel_evaluated(lanetab, B):
    mul = lanetab.rowmap_mul(B)
    for S in range(0, 7):
        items = [[lanetab.rowmap_item(p, lane, B, 2 + S, mul) for p in (0, 1)] for lane in range(64)]
        for D in (1, 28, 34):
            nvel = 2 + (D + 3) // 4
            for R in (1, 63, 64, 65, 441, 448):
                for tile_r in (-1, 0, 3, 8):
                    TW = 2 * tile_r + 1
                    ncell = TW * TW if tile_r >= 0 else 0
                    tab = _table(lanetab, B, S, D, R, tile_r)
                    for lane in range(64):
                        f = tab[lane]
                        ctx = (B, S, D, R, tile_r, lane)
                        # ---- the two row items, and what each row load is addressed with
                        assert f[0:2] == items[lane], ctx
                        for p in (0, 1):
                            item = items[lane][p]
                            r = max(item, 0) >> 4
                            assert f[2 + p] == 4 * max(r - 1, 0), ctx            # __shfl source of the frame blend (as a byte address)
                            if r >= 1:                                           # the lanes that loaded a record slot
                                assert f[5 + p] == item & 15, ctx
                            if 0 <= item < 15 and p == 0:                        # ... and the k_env_prep slot (row 0, not the root position)
                                assert f[5] == item, ctx
                            assert 0 <= f[5 + p] < 16 and f[2 + p] // 4 <= S, ctx   # in the record, and a sample that exists, on every lane
                        if lane == 0:                                            # lane 0 loads the heading terms every lane reads back
                            assert f[5] == 0, ctx
                        # ---- contact / velocity block
                        contact = lane < 4 * (1 + S)
                        vel = not contact and 32 <= lane < 32 + nvel
                        assert f[4] == 4 * ((lane >> 2) if contact else 0), ctx
                        if contact:
                            assert f[7] == REC_Q_CONTACT + (lane & 3) and f[8] == REC_Q_CONTACT + (lane & 3), ctx
                        elif vel:
                            assert f[7] == REC_Q_VEL + (lane - 32), ctx
                        assert REC_Q_CONTACT <= f[7] < REC_F4 and REC_Q_CONTACT <= f[8] < REC_Q_VEL and f[4] // 4 <= S, ctx
                        # ---- aux load: root velocity (lane 30), root angular velocity (31), contact force of body lane - 32
                        force = 32 <= lane < 32 + B
                        assert f[9] == (1 if lane == 30 else 2 if lane == 31 else 3 if force else 0), ctx
                        assert f[10] == (3 * (lane - 32) if force else 0) and f[10] + 2 < 3 * B, ctx
                        # ---- dof velocity
                        if lane < D:
                            assert f[11] == lane, ctx
                        assert 0 <= f[11] < D, ctx
                        # ---- the five tile cells
                        for i in range(5):
                            idx = lane + 64 * i
                            a, bq, valid = f[12 + 3 * i:15 + 3 * i]
                            assert valid == (1 if idx < ncell else 0), ctx
                            if idx < ncell:
                                assert (a, bq) == (idx // TW, idx % TW), ctx
                            else:
                                assert (a, bq) == (0, 0), ctx
                            assert 0 <= a < max(TW, 1) and 0 <= bq < max(TW, 1), ctx
                        # ---- ray slots inside R
                        assert f[27] == sum(1 for i in range(8) if lane + 64 * i < R), ctx


@pytest.mark.parametrize("R", [1, 63, 64, 65, 441, 448, 512, 513, 4096])
def test_ray_slot_clamp_stays_inside_the_fan(lanetab, R):
    """The prefetch loads ray min(lane + 64 i, R - 1) for every slot that has a ray on some lane (64 i < R) and skips the others; a
    lane's own rays (lane + 64 i < R) are not moved."""
    for lane in range(64):
        for i in range(8):
            off = lanetab.lanetab_ray_off(lane, R, i)
            if 64 * i >= R:
                assert off == -1, (R, lane, i)
            else:
                assert off == 8 * min(lane + 64 * i, R - 1) and 0 <= off <= 8 * (R - 1), (R, lane, i, off)


def test_fill_refuses_what_does_not_fit(lanetab):
    tab = (C.c_uint * (4 * 64))()
    ok = lambda B, S, D, R, tr: lanetab.lanetab_fill(tab, B, S, D, R, tr, lanetab.rowmap_mul(max(B, 2)), _tile_mul(tr))
    assert ok(15, 6, 40, 4096, 8) == 1
    assert ok(16, 6, 40, 441, 8) == 0    # bodies
    assert ok(15, 7, 40, 441, 8) == 0    # rows
    assert ok(15, 6, 41, 441, 8) == 0    # the velocity block would pass the end of the record
    assert ok(15, 6, 0, 441, 8) == 0
    assert ok(15, 6, 40, 0, 8) == 0
    assert ok(15, 6, 40, 441, 9) == 0    # 19 x 19 cells > the 320 of the tile
