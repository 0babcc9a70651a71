"""Heading pass of k_env_post: the per-lane table of parc_amd/csrc/parc_lanetab.hpp (parc_hrot_fill), from a host build of the header the
kernel includes (no GPU).  Every field of every entry against the expression the kernel evaluated in its four separate rotation sites before
the table existed (root velocities in the prefetch phase, a target row's root offset in the row pass, the key bodies of the character and
of the targets in the key-observation phase), written out here; every offset inside its array, also on the lanes that have no item.  Word 2
of the entry (the contact / velocity block behind the row passes) against the lane ranges, guards and destinations the kernel evaluated."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import REPO

SHIM = r"""
#include "parc_lanetab.hpp"
extern "C" int hrot_entry_bytes(void) { return (int)sizeof(ParcHrotEntry); }
extern "C" void hrot_layout(int *out) { out[0] = PARC_HROT_Q_F4; out[1] = PARC_HROT_FK_F4; out[2] = PARC_HROT_RV_F4; out[3] = PARC_HROT_RV_ZERO; out[4] = PARC_HROT_BLOCK_F4; }
extern "C" int hrot_fill(unsigned *tab, int B, int S, int D, int K, const int *key_ids, const int *key_slot, int oc, int off_key, int off_tar, int tar_w,
                         int tar_obs, int tar_contacts, int global_obs, int nst) {
    return parc_hrot_fill(reinterpret_cast<ParcHrotEntry *>(tab), B, S, D, K, key_ids, key_slot, oc, off_key, off_tar, tar_w, tar_obs, tar_contacts, global_obs, nst) ? 1 : 0;
}
// fields of one entry: src, sub, dst, add4, item, adds; contact / velocity block: offset, count, kind, index
extern "C" void hrot_fields(const unsigned *w, int *out) {
    out[0] = (int)parc_hr_src(w); out[1] = (int)parc_hr_sub(w); out[2] = (int)parc_hr_dst(w); out[3] = (int)parc_hr_add4(w);
    out[4] = parc_hr_item(w) ? 1 : 0; out[5] = parc_hr_adds(w) ? 1 : 0;
    out[6] = (int)parc_hr_cv_off(w); out[7] = (int)parc_hr_cv_n(w); out[8] = (int)parc_hr_cv_kind(w); out[9] = (int)parc_hr_cv_idx(w);
}
extern "C" void hrot_cv_kinds(int *out) { out[0] = PARC_HR_CV_NONE; out[1] = PARC_HR_CV_REF; out[2] = PARC_HR_CV_TAR; out[3] = PARC_HR_CV_VEL; }
"""


@pytest.fixture(scope="module")
def hrot(tmp_path_factory):
    d = tmp_path_factory.mktemp("hrot")
    src = d / "hrot_host.cpp"
    src.write_text(SHIM)
    so = d / "libhrot_host.so"
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-fPIC", "-shared", "-std=c++17", "-Wall", "-Werror",
                           "-I", os.path.join(REPO, "parc_amd", "csrc"), "-o", str(so), str(src)])
    lib = C.CDLL(str(so))
    lib.hrot_fill.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p] + [C.c_int] * 8
    lib.hrot_fields.argtypes = [C.c_void_p, C.c_void_p]
    lib.hrot_layout.argtypes = [C.c_void_p]
    assert lib.hrot_entry_bytes() == 12
    return lib


def _layout(B, D, S, K, oc, tar, contact, R=441):
    """parc_env_create's observation layout (ig_parkour_env.py:842-965)."""
    J = B - 1
    off_dofvel = oc + 12 + 6 * J
    off_key = off_dofvel + D
    off_tar = off_key + 3 * K
    tar_w = 3 + 6 + 6 * J + 3 * K
    off_tarc = off_tar + (S * tar_w if tar else 0)
    width = off_tarc + (S * B if tar and contact else 0) + (B if contact else 0) + R
    return dict(off_key=off_key, off_tar=off_tar, tar_w=tar_w, off_tarc=off_tarc, width=width)


def _key_slot(key_ids):
    """parc_env_create: body -> the first key that names it, -1 = not a key body."""
    slot = [-1] * 16
    for k, b in enumerate(key_ids):
        if slot[b] < 0:
            slot[b] = k
    return slot


def _table(lib, B, S, D, key_ids, oc, L, tar, contact, gl):
    K = len(key_ids)
    tab = (C.c_uint * (3 * 64))()
    ids = (C.c_int * 8)(*(list(key_ids) + [0] * (8 - K)))
    slot = (C.c_int * 16)(*_key_slot(key_ids))
    assert lib.hrot_fill(tab, B, S, D, K, ids, slot, oc, L["off_key"], L["off_tar"], L["tar_w"], int(tar), int(tar and contact), int(gl), L["off_tarc"]) == 1
    out = (C.c_int * 10)()
    rows = []
    for lane in range(64):
        lib.hrot_fields(C.byref(tab, 12 * lane), out)
        rows.append(list(out))
    return rows


# name -> (B, D, tar_obs_steps, key body ids, off_char, enable_tar_obs, use_contact_info, global_obs, observation width or None)
CONFIGS = {
    "default": (15, 28, 6, [5, 8, 11, 14], 0, True, True, False, 1312),
    "three_targets": (15, 28, 3, [5, 8, 11, 14], 0, True, True, False, 136 + 3 * 105 + 3 * 15 + 15 + 441),
    "targets_off": (15, 28, 6, [5, 8, 11, 14], 0, False, True, False, 592),
    "root_height": (15, 28, 6, [5, 8, 11, 14], 1, True, True, False, 1313),
    "no_contact_info": (15, 28, 6, [5, 8, 11, 14], 0, True, False, False, 1207),
    "no_contact_no_targets": (15, 28, 6, [5, 8, 11, 14], 0, False, False, False, 577),
    "global_obs": (15, 28, 6, [5, 8, 11, 14], 0, True, True, True, 1312),
    "root_height_global": (15, 28, 6, [5, 8, 11, 14], 1, True, True, True, 1313),
    "one_key": (15, 28, 6, [14], 0, True, True, False, None),
    "eight_keys": (15, 28, 6, [2, 5, 6, 8, 9, 11, 13, 14], 0, True, True, False, None),   # 48 + 8 + 6 + 2 = all 64 lanes
    "eight_keys_one_body_twice": (15, 28, 6, [2, 5, 6, 8, 5, 11, 13, 14], 0, True, True, False, None),   # key 4 shares the FK slot of key 1
    "three_bodies": (3, 4, 6, [1, 2], 0, True, True, False, None),
    "no_keys": (15, 28, 6, [], 0, True, True, False, None),
}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_every_entry_equals_the_expressions_of_the_four_rotation_sites(hrot, name):
    B, D, S, key_ids, oc, tar, contact, gl, width = CONFIGS[name]
    K = len(key_ids)
    L = _layout(B, D, S, K, oc, tar, contact)
    if width is not None:
        assert L["width"] == width
    lay = (C.c_int * 5)()
    hrot.hrot_layout(lay)
    QF, FKF, RVF, RVZ, BLK = list(lay)
    # the kernel's LDS block: s_q[8][16] | s_fk[80] | s_rv[4]; the five tile stores of a lane (320 floats) end with s_fk
    assert (QF, FKF, RVF, BLK) == (0, 8 * 16, 8 * 16 + 80, 8 * 16 + 80 + 4) and 0 <= RVZ < 4 and RVZ not in (0, 1)
    q = lambda r, i: 16 * (QF + 16 * r + i)        # byte offset of s_q[r][i]
    fk = lambda i: 16 * (FKF + i)                  # ... of s_fk[i]
    rv = lambda i: 16 * (RVF + i)
    key_slot = _key_slot(key_ids)
    off_key, off_tar, tar_w = L["off_key"], L["off_tar"], L["tar_w"]

    # what the kernel evaluated, site by site: (source, subtrahend, destination float, destination of the vector it adds or None)
    want = []
    # prefetch phase, role ROOT_VEL / ROOT_ANG_VEL: quat_rotate(hinv, aux) -> s_obs[oc + 6 ..] / s_obs[oc + 9 ..]; no subtraction
    want.append((rv(0), rv(RVZ), oc + 6, None))
    want.append((rv(1), rv(RVZ), oc + 9, None))
    if tar:
        # row_pass<ROOT>, is_pos && !row0 && !row1: res - root_pos -> s_obs[base ..], base = off_tar + (r - 2) tar_w
        for r in range(2, 2 + S):
            want.append((q(r, 15), q(0, 15), off_tar + (r - 2) * tar_w, None))
    # key-observation phase, row == 0: s_fk[key_ids[kk]] - root_pos -> s_obs[off_key + 3 kk ..]
    for kk in range(K):
        want.append((fk(key_ids[kk]), q(0, 15), off_key + 3 * kk, None))
    if tar:
        # ... row >= 1 (r = row + 1): s_fk[32 + (r - 2) 8 + key_slot[key_ids[kk]]] - s_q[r][15] -> s_obs[o ..], o = tb + 3 + 6 B + 3 kk,
        # plus s_obs[tb ..] (not under global_obs), tb = off_tar + (r - 2) tar_w
        for row in range(1, 1 + S):
            r = row + 1
            tb = off_tar + (r - 2) * tar_w
            for kk in range(K):
                want.append((fk(32 + (r - 2) * 8 + key_slot[key_ids[kk]]), q(r, 15), tb + 3 + 6 * B + 3 * kk, None if gl else tb))

    tab = [f[:6] for f in _table(hrot, B, S, D, key_ids, oc, L, tar, contact, gl)]
    got = []
    for lane, (src, sub, dst, add4, item, adds) in enumerate(tab):
        ctx = (name, lane)
        # in bounds on every lane, aligned as the kernel reads them
        assert src % 16 == 0 and sub % 16 == 0 and 0 <= src < 16 * BLK and 0 <= sub < 16 * BLK, ctx
        assert dst % 4 == 0 and add4 % 4 == 0 and 0 <= add4 < 256, ctx
        if not item:
            assert (src, sub, dst, add4, adds) == (0, 0, 0, 0, 0), ctx
            continue
        assert 0 <= dst // 4 and dst // 4 + 3 <= L["off_tarc"], ctx      # the store stays inside the staged row
        # every lane with an item shuffles: the lane it reads must have one too (an inactive lane yields no defined value)
        assert tab[add4 // 4][4] == 1, ctx
        add_dst = None
        if adds:
            s_src, s_sub, s_dst, _, s_item, s_adds = tab[add4 // 4]
            assert s_adds == 0, ctx                                      # the added vector is a root offset as rotated, nothing added to it
            add_dst = s_dst // 4
        else:
            assert add4 == 0, ctx
        got.append((src, sub, dst // 4, add_dst))
    assert sorted(got, key=lambda t: t[2]) == sorted(want, key=lambda t: t[2])
    assert len(got) == 2 + K + (S + S * K if tar else 0)
    # no two items write the same floats
    cells = [d + c for (_, _, d, _) in got for c in range(3)]
    assert len(cells) == len(set(cells))
    # a lane that adds reads the root offset of ITS row: the source of that lane's item is the subtrahend of this one
    for lane, (src, sub, dst, add4, item, adds) in enumerate(tab):
        if adds:
            assert tab[add4 // 4][0] == sub and tab[add4 // 4][1] == q(0, 15), (name, lane)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_contact_and_velocity_block_equals_the_expressions_of_the_kernel(hrot, name):
    """Word 2: the block behind the row passes.  Until the table existed, a lane < 4 (1 + S) took sample s = lane >> 2 and bodies 4 c + k
    (c = lane & 3, k < 4) under `bd < B`: sample 0 to s_refct[bd], target s to orow[off_tarc + (s - 1) B + bd] when the target block and the
    contact blocks exist; a lane in [32, 32 + nvel) that is no contact lane took float4 lane - 32 of the velocity block to s_refvel."""
    B, D, S, key_ids, oc, tar, contact, gl, width = CONFIGS[name]
    L = _layout(B, D, S, len(key_ids), oc, tar, contact)
    kinds = (C.c_int * 4)()
    hrot.hrot_cv_kinds(kinds)
    NONE, REF, TAR, VEL = list(kinds)
    nvel = 2 + (D + 3) // 4
    tab = _table(hrot, B, S, D, key_ids, oc, L, tar, contact, gl)
    row_written = []
    for lane in range(64):
        off, nk, kind, idx = tab[lane][6:10]
        ctx = (name, lane)
        s, c = lane >> 2, lane & 3
        bodies = [4 * c + k for k in range(4) if 4 * c + k < B]
        if lane < 4 * (1 + S) and bodies and s == 0:
            assert (kind, idx, nk) == (REF, c, len(bodies)), ctx
            # the kernel stores all four floats at s_refct[4 c ..]: inside the 16 slots, and a slot >= B has no reader
            assert 4 * idx + 3 < 16, ctx
        elif lane < 4 * (1 + S) and bodies and tar and contact:
            assert (kind, nk) == (TAR, len(bodies)) and off % 4 == 0, ctx
            assert [off // 4 + k for k in range(nk)] == [L["off_tarc"] + (s - 1) * B + bd for bd in bodies], ctx
            row_written += [off // 4 + k for k in range(nk)]
        elif lane >= 4 * (1 + S) and 32 <= lane < 32 + nvel:
            assert (kind, idx) == (VEL, lane - 32) and idx < 12, ctx            # s_refvel has 12 float4
        else:
            assert (off, nk, kind, idx) == (0, 0, NONE, 0), ctx
    # the target-contact block of the row, each float once: [off_tarc, off_tarc + S B)
    want = list(range(L["off_tarc"], L["off_tarc"] + S * B)) if tar and contact else []
    assert sorted(row_written) == want


def test_fill_refuses_what_does_not_fit(hrot):
    tab = (C.c_uint * (3 * 64))()

    def ok(B, S, key_ids, nst=None, slot=None, D=28):
        K = len(key_ids)
        L = _layout(B, D, S, min(K, 8), 0, True, True)
        ids = (C.c_int * 16)(*(list(key_ids) + [0] * (16 - K)))
        sl = (C.c_int * 16)(*(slot if slot is not None else _key_slot([k for k in key_ids if 0 <= k < 16])))
        return hrot.hrot_fill(tab, B, S, D, K, ids, sl, 0, L["off_key"], L["off_tar"], L["tar_w"], 1, 1, 0, L["off_tarc"] if nst is None else nst)

    assert ok(15, 6, [2, 5, 6, 8, 9, 11, 13, 14]) == 1
    assert ok(16, 6, [5, 8]) == 0                          # bodies
    assert ok(15, 7, [5, 8]) == 0                          # rows
    assert ok(15, 6, list(range(9))) == 0                  # key bodies
    assert ok(15, 6, [5, 15]) == 0                         # a key body that is no body
    assert ok(15, 6, [5, 8], slot=[-1] * 16) == 0          # a key body without an FK slot
    assert ok(15, 6, [5, 8], nst=100) == 0                 # a store past the staged row
    assert ok(15, 6, [5, 8], D=41) == 0                    # the velocity block would pass the end of s_refvel
