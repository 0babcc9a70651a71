"""The front end the tool handles share (``parc_amd/tool_handle.py``) and the signature table of ``parc_amd/lib.py``, without a GPU: the
plan codec over the three real field tables, driven through the wrappers' own ``empty_plan`` / ``plan_from_numpy`` / ``_plan_struct``
on objects that hold a codec and no handle."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

from conftest import REPO
from parc_amd import lib as L
from parc_amd import motion_aug as ma
from parc_amd import motion_sampler as ms
from parc_amd import terrain_gen as tg
from parc_amd.tool_handle import PlanCodec, ToolHandle, fill_struct

CPU = torch.device("cpu")
I32, F32 = torch.int32, torch.float32


def shell(cls, codec, **attrs):
    """A wrapper object without a handle: what its plan members read, and nothing else."""
    o = cls.__new__(cls)
    o.__dict__.update(device=CPU, _codec=codec, **attrs)
    return o


def sampler_cfg(aug_mode):
    return types.SimpleNamespace(max_num_boxes=4, Gx=5, Gy=7, aug_mode=ms.AUG_MODE[aug_mode])


def tools():
    """name -> (wrapper shell, the declared plan {field: (dtype, per-item shape)}, required fields, non-zero defaults)"""
    out = {"maug": (shell(ma.MotionAugmenter, PlanCodec(L.MAUG_PLAN_FIELDS, L.ParcMotionAugPlan)),
                    {k: (I32 if t == "i" else F32, s) for k, t, s in L.MAUG_PLAN_FIELDS}, ("src_clip", "start_frame", "num_frames"),
                    dict(scale=1.0, height_scale=1.0))}
    sub = dict(mb=4, gx=5, gy=7)
    for mode in ("NOISE", "MAXPOOL_AND_BOXES"):
        cfg = sampler_cfg(mode)
        want = {k: (I32 if t == "i" else F32, tuple(sub.get(d, d) for d in s)) for k, t, s in L.MSAMP_PLAN_FIELDS if k != "noise" or mode == "NOISE"}
        out["msamp-" + mode] = (shell(ms.MotionWindowSampler, ms.plan_codec(cfg), cfg=cfg), want, ("motion_id",), {})
    settings = dict(BOXES=tg.BoxesSettings(num_boxes=3), PATHS=tg.PathsSettings(num_terrain_paths=2), STAIRS=tg.StairsSettings(num_stairs=5))
    for mode, s in settings.items():
        fields = tg.plan_fields(mode, s)
        codec = PlanCodec([(k, "f", shape) for k, shape in fields.items()], L.ParcTerrainGenPlan)
        out["tgen-" + mode] = (shell(tg.TerrainGenerator, codec, fields=fields), {k: (F32, shape) for k, shape in fields.items()}, tuple(fields), {})
    return out


TOOLS = tools()
CASES = [(name, n) for name in TOOLS for n in (1, 3)]


def host_arrays(want, n, seed=0):
    r = np.random.RandomState(seed)
    return {k: (r.randint(0, 5, (n,) + s).astype(np.int32) if dt == I32 else r.rand(*((n,) + s)).astype(np.float32)) for k, (dt, s) in want.items()}


def test_the_declared_tables_are_the_real_ones():
    assert list(TOOLS["maug"][1]) == [f[0] for f in L.ParcMotionAugPlan._fields_[1:]] == list(ma.plan_fields())
    assert list(TOOLS["msamp-NOISE"][1]) == [f[0] for f in L.ParcMotionSamplerPlan._fields_[1:]] == [f[0] for f in ms.PLAN_FIELDS]
    assert TOOLS["msamp-NOISE"][1]["boxes"] == (F32, (4, 6)) and TOOLS["msamp-NOISE"][1]["noise"] == (F32, (5, 7))
    assert "noise" not in TOOLS["msamp-MAXPOOL_AND_BOXES"][1]
    assert [k for m in ("BOXES", "PATHS", "STAIRS") for k in TOOLS["tgen-" + m][1]] == L.TGEN_PLAN_FIELDS
    assert TOOLS["tgen-PATHS"][1]["path_turn"] == (F32, (2, tg.PATH_POINTS)) and TOOLS["tgen-STAIRS"][1]["stairs"] == (F32, (5, tg.STAIR_FLOATS))


@pytest.mark.parametrize("name,n", CASES)
def test_empty_has_the_declared_dtypes_and_shapes(name, n):
    tool, want, _, _ = TOOLS[name]
    for zero in (True, False):
        plan = tool.empty_plan(n, zero=zero)
        assert list(plan) == list(want)
        for k, (dt, s) in want.items():
            assert plan[k].dtype == dt and tuple(plan[k].shape) == (n,) + s and plan[k].device == CPU and plan[k].is_contiguous(), k
            assert not zero or not plan[k].any(), k


@pytest.mark.parametrize("name,n", CASES)
def test_from_numpy_required_fields_and_defaults(name, n):
    tool, want, required, defaults = TOOLS[name]
    arrays = host_arrays(want, n)
    plan = tool.plan_from_numpy({k: arrays[k].astype(np.float64) for k in arrays})     # any host dtype is taken to the field's own
    assert list(plan) == list(want)
    for k, (dt, s) in want.items():
        assert plan[k].dtype == dt and np.array_equal(plan[k].numpy(), arrays[k]), k
    least = tool.plan_from_numpy({k: arrays[k] for k in required})
    assert list(least) == list(want)
    for k, (dt, s) in want.items():
        fill = arrays[k] if k in required else np.full((n,) + s, defaults.get(k, 0))
        assert least[k].dtype == dt and tuple(least[k].shape) == (n,) + s and np.array_equal(least[k].numpy(), fill), k
    for k in required:
        with pytest.raises(ValueError, match=rf"plan: {k} is missing"):
            tool.plan_from_numpy({j: a for j, a in arrays.items() if j != k})
    assert tool._plan_struct(least)[1] == n


@pytest.mark.parametrize("name,n", CASES)
def test_from_numpy_refusals(name, n):
    tool, want, required, _ = TOOLS[name]
    arrays = host_arrays(want, n)
    codec = tool._codec
    with pytest.raises(ValueError, match=r"plan: unknown field\(s\) \['no_such_field'\]"):
        codec.from_numpy(dict(arrays, no_such_field=np.zeros(n)), CPU, required=required, reject_unknown=True)
    if name == "maug":                                  # the augmenter is the wrapper that refuses one
        with pytest.raises(ValueError, match=r"plan: unknown field\(s\) \['no_such_field'\]"):
            tool.plan_from_numpy(dict(arrays, no_such_field=np.zeros(n)))
    else:
        assert list(tool.plan_from_numpy(dict(arrays, no_such_field=np.zeros(n)))) == list(want)
    last = list(want)[-1]                               # a later field: n comes from the first required one
    s = want[last][1]
    assert s, "every table ends in an array field"
    with pytest.raises(ValueError, match=rf"plan: {last} must have shape \({n}, "):
        tool.plan_from_numpy(dict(arrays, **{last: np.zeros((n,) + s[:-1] + (s[-1] + 1,), np.float32)}))
    if len(want) > 1:                                   # (a plan of one field has that field's n)
        with pytest.raises(ValueError, match=rf"plan: {last} must have shape \({n}, "):
            tool.plan_from_numpy(dict(arrays, **{last: np.zeros((n + 1,) + s, np.float32)}))


@pytest.mark.parametrize("name,n", CASES)
def test_struct_checks_and_pointers(name, n):
    tool, want, _, _ = TOOLS[name]
    plan = tool.plan_from_numpy(host_arrays(want, n, seed=1))
    st, got_n = tool._plan_struct(plan)
    assert got_n == n == st.n
    for field, _ in type(st)._fields_[1:]:              # every present field's pointer, null for the rest of the struct
        assert getattr(st, field) == (plan[field].data_ptr() if field in want else None), field
    first, last = list(want)[0], list(want)[-1]
    dt, s = want[last]
    with pytest.raises(ValueError, match=rf"plan: {last} is missing"):
        tool._plan_struct({k: v for k, v in plan.items() if k != last})
    with pytest.raises(ValueError, match=rf"plan: {first} is missing"):
        tool._plan_struct({k: v for k, v in plan.items() if k != first})
    wide = torch.zeros((n,) + s[:-1] + (2 * s[-1],), dtype=dt)
    with pytest.raises(ValueError, match=rf"plan: {last} must be contiguous on cpu"):
        tool._plan_struct(dict(plan, **{last: wide[..., ::2]}))
    with pytest.raises(ValueError, match=rf"plan: {last} must be {re.escape(str(dt))} \({n}, .*got torch.float64"):
        tool._plan_struct(dict(plan, **{last: plan[last].double()}))
    if len(want) > 1:                                   # (a plan of one field has that field's n)
        with pytest.raises(ValueError, match=rf"plan: {last} must be {re.escape(str(dt))} \({n}, .*got {re.escape(str(dt))} \({n + 1}, "):
            tool._plan_struct(dict(plan, **{last: torch.zeros((n + 1,) + s, dtype=dt)}))
    with pytest.raises(ValueError, match=rf"plan: {last} must be {re.escape(str(dt))} \({n}, .*got {re.escape(str(dt))} \({n}, "):
        tool._plan_struct(dict(plan, **{last: torch.zeros((n,) + s[:-1] + (s[-1] - 1,), dtype=dt)}))
    with pytest.raises(ValueError, match=rf"plan: {last} must be contiguous on cpu"):
        tool._plan_struct(dict(plan, **{last: torch.empty((n,) + s, dtype=dt, device="meta")}))
    assert tool._codec.struct(dict(plan, **{last: wide[..., ::2]}))[1] == n      # without a device: lengths and dtypes only (check_plan)


@pytest.mark.parametrize("n", (1, 3))
def test_sampler_noise_is_carried_only_in_noise_mode(n):
    tool, want, _, _ = TOOLS["msamp-MAXPOOL_AND_BOXES"]
    plan = tool.empty_plan(n)
    assert "noise" not in plan and tool._plan_struct(plan)[0].noise is None
    assert "noise" not in tool.plan_from_numpy(dict(host_arrays(want, n), noise=np.ones((n, 5, 7), np.float32)))
    noise = torch.ones((n, 5, 7))
    assert tool._plan_struct(dict(plan, noise=noise))[0].noise == noise.data_ptr()       # one that is passed is checked and handed on
    with pytest.raises(ValueError, match="plan: noise must be torch.float32"):
        tool._plan_struct(dict(plan, noise=torch.ones((n, 5, 6))))
    assert ms.check_plan(plan, tool.cfg) == n
    noisy = TOOLS["msamp-NOISE"][0]
    with pytest.raises(ValueError, match="plan: noise is missing"):
        noisy._plan_struct(plan)
    full = noisy.empty_plan(n)
    assert noisy._plan_struct(full)[0].noise == full["noise"].data_ptr() and ms.plan_shapes(n, noisy.cfg)["noise"] == (n, 5, 7)


def test_fill_struct_writes_the_given_pointers():
    t = dict(root_pos=torch.zeros(3), hfs=torch.zeros(2))
    st = fill_struct(L.ParcMotionSamplerOutputs, t)
    assert st.root_pos == t["root_pos"].data_ptr() and st.hfs == t["hfs"].data_ptr() and st.hf_bounds is None and st.floor_heights is None


def test_every_declared_function_has_a_signature():
    hdr = open(os.path.join(REPO, "include", "parc_env.h")).read()
    declared = re.findall(r"^(?:const )?[a-z]+(?: [a-z]+)? \*?(parc_[a-z_0-9]+)\(", hdr, re.M)   # `int parc_x(`, `const char *parc_x(`
    assert set(declared) == set(re.findall(r"\b(parc_[a-z_0-9]+)\s*\(", hdr)) and len(declared) == len(set(declared))
    assert list(L.SIGNATURES) == declared == list(L.EXPORTED_SYMBOLS)                     # the header's names, in the header's order
    for name, (restype, argtypes) in L.SIGNATURES.items():
        assert isinstance(argtypes, list), name
        returns_void = re.search(rf"\bvoid\s+{name}\s*\(", hdr) is not None
        assert (restype is None) == returns_void == name.endswith("_destroy"), name
        takes_none = re.search(rf"\b{name}\s*\(\s*void\s*\)", hdr) is not None
        assert (argtypes == []) == takes_none, name
    assert {n for n, (_, a) in L.SIGNATURES.items() if a == []} == {"parc_abi_version", "parc_last_error", "parc_build_flags"}
    lib = L.load()
    for name, (restype, argtypes) in L.SIGNATURES.items():                               # load() applied the table
        fn = getattr(lib, name)
        assert fn.restype == restype and list(fn.argtypes) == argtypes, name


def test_a_failed_create_leaves_no_handle():
    calls = []

    class FakeLib:
        @staticmethod
        def parc_fake_create(params, out):
            calls.append("create")
            raise L.ParcError("refused")

        @staticmethod
        def parc_fake_destroy(h):
            calls.append("destroy")

    class Params(C.Structure):
        _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int32)]

    class Fake(ToolHandle):
        PREFIX, KERNELS = "parc_fake", ("a", "b")

        def __init__(self, fail):
            self._L, self._lib, self.device = L, FakeLib, CPU
            self.params = Params()
            if fail == "before":
                raise ValueError("settings")
            self._create_handle(self.params)

    for fail in ("before", "create"):
        o = Fake.__new__(Fake)
        with pytest.raises(ValueError if fail == "before" else L.ParcError):
            o.__init__(fail)
        assert o._h is None
        o.__del__()
        o._destroy()
        assert o._h is None
    assert calls == ["create"] and o.params.struct_size == C.sizeof(Params)
    o._h = C.c_void_p(1234)                              # a live handle is released once, through <PREFIX>_destroy
    o.__del__()
    o.__del__()
    assert o._h is None and calls == ["create", "destroy"]


# ---- the native side of a handle: what every parc_*_create and parc_*_kernel_times refuses before it touches a device ----------------
CREATES = {"mopt": L.ParcMotionOptParams, "mterr": L.ParcMotionTerrainParams, "medit": L.ParcMotionEditParams, "msamp": L.ParcMotionSamplerParams,
           "maug": L.ParcMotionAugParams, "pathplan": L.ParcPathPlanParams, "tgen": L.ParcTerrainGenParams, "mdm": L.ParcMdmParams,
           "mpath": L.ParcMdmPathParams, "mloss": L.ParcMotionLossParams}
WITH_CHAR = ("mopt", "mterr", "medit", "msamp", "maug", "mdm", "mloss")       # the tools whose parameters hold a ParcCharModel
MIN_TWO_BODIES = ("msamp", "maug", "mdm", "mloss")
CHECK_DOF_SIZE = ("mopt", "mterr", "medit", "mloss")


def refused(pre, params, message):
    """parc_<pre>_create(params) is PARC_ERR_INVALID with exactly `message`, and the out handle stays null."""
    lib = L.load()
    out = C.c_void_p()
    rc = getattr(lib, f"parc_{pre}_create")(None if params is None else C.byref(params), C.byref(out))
    assert rc == -1 and lib.parc_last_error().decode() == message and not out.value, (pre, rc, lib.parc_last_error().decode())


def sized(pre, num_bodies=2, dof_size=0):
    p = CREATES[pre]()
    p.struct_size = C.sizeof(p)
    if pre in WITH_CHAR:
        p.model.num_bodies, p.model.dof_size = num_bodies, dof_size
    return p


def test_the_character_tools_are_the_ones_with_a_model():
    assert sorted(WITH_CHAR) == sorted(pre for pre, t in CREATES.items() if any(f[0] == "model" and f[1] is L.ParcCharModel for f in t._fields_))


@pytest.mark.parametrize("pre", CREATES)
def test_create_refuses_null_and_a_wrong_struct_size(pre):
    refused(pre, None, f"{pre}: null argument")
    p = sized(pre)
    p.struct_size += 1
    refused(pre, p, f"{CREATES[pre].__name__} ABI mismatch (struct_size)")
    lib = L.load()                                          # a null out pointer is the same refusal
    assert getattr(lib, f"parc_{pre}_create")(C.byref(sized(pre)), None) == -1 and lib.parc_last_error().decode() == f"{pre}: null argument"


@pytest.mark.parametrize("pre", WITH_CHAR)
def test_create_checks_the_body_count_against_the_tools_minimum(pre):
    refused(pre, sized(pre, num_bodies=0), f"{pre}: num_bodies out of range")
    refused(pre, sized(pre, num_bodies=L.MAX_BODIES + 1), f"{pre}: num_bodies out of range")
    lib = L.load()
    out = C.c_void_p()
    rc = getattr(lib, f"parc_{pre}_create")(C.byref(sized(pre, num_bodies=1)), C.byref(out))
    assert rc == -1 and not out.value                       # (a zeroed struct is refused by every tool, further down)
    assert (lib.parc_last_error().decode() == f"{pre}: num_bodies out of range") == (pre in MIN_TWO_BODIES), pre


@pytest.mark.parametrize("pre", WITH_CHAR)
def test_create_checks_dof_size_where_the_tool_does(pre):
    lib = L.load()
    out = C.c_void_p()
    for bad in (L.MAX_DOFS + 1, -1):
        rc = getattr(lib, f"parc_{pre}_create")(C.byref(sized(pre, dof_size=bad)), C.byref(out))
        assert rc == -1 and not out.value
        assert (lib.parc_last_error().decode() == f"{pre}: dof_size out of range") == (pre in CHECK_DOF_SIZE), pre


@pytest.mark.parametrize("pre", CREATES)
def test_kernel_times_refuses_a_null_handle(pre):
    lib = L.load()
    buf = (C.c_float * 8)(*([7.0] * 8))
    assert getattr(lib, f"parc_{pre}_kernel_times")(None, buf) == -1 and lib.parc_last_error().decode() == f"{pre}: null argument"
    assert list(buf) == [7.0] * 8
