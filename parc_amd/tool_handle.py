"""What the Python front ends of the tool handles (``parc_mopt_*`` ... ``parc_mdm_*``) share: the handle's life, its calls and timings
(:class:`ToolHandle`), and the plans of the plan-driven tools as dicts of tensors (:class:`PlanCodec`).  A new tool subclasses
``ToolHandle`` with its ``PREFIX`` and ``KERNELS``, lists its functions in ``lib.SIGNATURES`` and, if it takes plans, builds one
``PlanCodec`` over its field table ("The Python front ends").
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from parc_amd import lib as L


class ToolHandle:
    """One ``<PREFIX>_create`` / ``<PREFIX>_destroy`` handle of ``libparc_env.so`` on one device."""
    PREFIX = ""              # "parc_maug", ...
    KERNELS = ()             # the names of <PREFIX>_kernel_times' entries, in its order
    DEVICE_CONTEXT = True    # _call runs under torch.cuda.device(self.device); False where the C side alone selects the device
    _h = None                # None until <PREFIX>_create has returned, and after _destroy

    def __init__(self, device="cuda:0"):
        import torch  # the process must hold one HIP runtime, torch's: loaded before the library
        self._L, self._lib = L, L.load()
        self.device = torch.device(device)
        self.device_index = L.device_index(self.device)

    def _create_handle(self, params):
        params.struct_size = C.sizeof(type(params))
        h = C.c_void_p()
        L.check(getattr(self._lib, self.PREFIX + "_create")(C.byref(params), C.byref(h)))
        self._h = h

    _release = staticmethod(L.destroy_handle)   # held by the class: __del__ may run while the interpreter clears the modules' globals

    def _destroy(self):
        self._release(self, self.PREFIX + "_destroy")

    def __del__(self):
        self._destroy()

    def _stream(self):
        import torch
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _call(self, name: str, *args):
        """``<PREFIX>_<name>(handle, *args)``; a non-zero return code raises ``ParcError`` with the library's message."""
        fn = getattr(self._lib, f"{self.PREFIX}_{name}")
        if self.DEVICE_CONTEXT:
            import torch
            with torch.cuda.device(self.device):
                L.check(fn(self._h, *args))
        else:
            L.check(fn(self._h, *args))

    def kernel_times(self):
        """Device ms of the last run of each of ``KERNELS`` (0 = not run)."""
        ms = np.zeros(len(self.KERNELS), np.float32)
        self._call("kernel_times", L.np_f32p(ms))
        return dict(zip(self.KERNELS, ms.tolist()))


def fill_struct(struct_type, tensors: dict):
    """A struct of device pointers (a plan's outputs) from ``name -> tensor``; the caller keeps the tensors alive."""
    st = struct_type()
    for k, t in tensors.items():
        setattr(st, k, t.data_ptr())
    return st


class PlanCodec:
    """The plan of one handle: ``fields`` is the table ``[(name, "i" | "f", per-item shape)]`` in the order of ``struct_type`` (an
    ``int32 n``, then one pointer per field); a shape may hold names, which ``symbols`` resolves here, once.  A plan is a dict
    ``name -> tensor [n, *shape]``.  The fields in ``optional`` are left out of the plans made here and may be absent from one passed
    in (their pointer stays null); one that is present is checked and passed like the rest."""

    def __init__(self, fields, struct_type, symbols=None, optional=()):
        import torch
        sub = symbols or {}
        self.fields = {k: (torch.int32 if t == "i" else torch.float32, tuple(int(sub.get(d, d)) for d in s)) for k, t, s in fields}
        self.struct_type, self.optional = struct_type, frozenset(optional)
        self.first = next(k for k in self.fields if k not in self.optional)   # the field whose length is the plan's n

    def empty(self, n: int, device, zero: bool = True) -> dict:
        """The plan's arrays on ``device``; ``zero=False`` leaves them uninitialised (for a kernel that writes every entry)."""
        import torch
        make = torch.zeros if zero else torch.empty
        return {k: make((int(n),) + s, dtype=dt, device=device) for k, (dt, s) in self.fields.items() if k not in self.optional}

    def from_numpy(self, arrays: dict, device, required=(), defaults=None, reject_unknown: bool = False) -> dict:
        """A plan from host arrays ``[n, ...]``, n being the length of the first required field.  A missing field is ``defaults``' value,
        else zeros; the optional fields are not taken."""
        import torch
        required = tuple(required) or (self.first,)
        for k in required:
            if k not in arrays:
                raise ValueError(f"plan: {k} is missing")
        unknown = sorted(set(arrays) - set(self.fields))
        if unknown and reject_unknown:
            raise ValueError(f"plan: unknown field(s) {unknown}")
        n = int(np.asarray(arrays[required[0]]).shape[0])
        plan = {}
        for k, (dt, s) in self.fields.items():
            if k in self.optional:
                continue
            if k in arrays:
                a = np.ascontiguousarray(arrays[k], np.int32 if dt == torch.int32 else np.float32)
                if a.shape != (n,) + s:
                    raise ValueError(f"plan: {k} must have shape {(n,) + s}, got {a.shape}")
                plan[k] = torch.from_numpy(a).to(device)
            else:
                plan[k] = torch.full((n,) + s, (defaults or {}).get(k, 0), dtype=dt, device=device)
        return plan

    def struct(self, plan: dict, device=None):
        """``(struct_type over the plan's arrays, n)``: every array is ``[n, *shape]`` of its dtype, and contiguous on ``device``
        (``None``: lengths and dtypes only).  The caller keeps ``plan`` alive."""
        if self.first not in plan:
            raise ValueError(f"plan: {self.first} is missing")
        n = int(plan[self.first].shape[0])
        st = self.struct_type()
        st.n = n
        for k, (dt, s) in self.fields.items():
            x = plan.get(k)
            if x is None:
                if k in self.optional:
                    continue
                raise ValueError(f"plan: {k} is missing")
            if tuple(x.shape) != (n,) + s or x.dtype != dt:
                raise ValueError(f"plan: {k} must be {dt} {(n,) + s}, got {x.dtype} {tuple(x.shape)}")
            if device is not None and (x.device != device or not x.is_contiguous()):
                raise ValueError(f"plan: {k} must be contiguous on {device}")
            setattr(st, k, x.data_ptr())
        return st, n
