// parc_tool_handle.hpp -- the host skeleton of a tool handle (parc_mopt_* .. parc_mloss_*, include/parc_env.h): what
// every tool's C-ABI section repeated around its own validation and launches.  Host code only; included by the tool headers of
// parc_tools.hip and by nothing else.  A tool writes its handle struct (on one of the bases below), its validation, its kernels' arguments
// and its extern "C" functions; the rules below are properties of one function each:
//   launch         a launch is always checked
//   renew          a slot is never left half filled: the old object goes first, the new one is the caller's local until it is installed
//   create         a handle never escapes a failed create, and whatever it owns is released on the device it was made on
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "../../include/parc_env.h"
#include "parc_common.hpp"
#include "parc_char.hpp"

namespace tool {

// k<<<grid, block, lds, st>>>(a...).  The arguments are parameters of the kernel's own types (KA comes from k alone), so they convert
// implicitly, as in a direct launch, and a mistyped one does not compile.
template <typename T> struct as_is { typedef T type; };
template <typename... KA> static int launch(void (*k)(KA...), dim3 grid, dim3 block, size_t lds, hipStream_t st, typename as_is<KA>::type... a) {
    hipLaunchKernelGGL(k, grid, block, lds, st, a...);
    HIPCHK(hipGetLastError());
    return PARC_OK;
}

// ---- the handle ------------------------------------------------------------------------------------------------------------------
// What every handle holds: its device, the arena of create .. destroy, its events.  No destructor selects the device: a base's would
// run after the derived struct's members (a batch, a library) have released their memory.  destroy() selects it, before anything goes.
// So a handle is released through destroy() only: a plain `delete h`, or a unique_ptr with the default deleter, skips the selection.
template <typename Events> struct Handle {
    int device = 0;
    DeviceArena mem;
    Events ev;
};
template <typename Model, typename Events> struct CharHandle : Handle<Events> {   // + the character: the host's copy and the device's (in mem)
    Model host_model;
    Model *d_model = nullptr;
};

template <typename H> static void destroy(H *h) {
    if (h) (void)hipSetDevice(h->device);
    delete h;                             // the members release the rest
}

// a new object of host memory into `owner` (a unique_ptr), without exceptions
template <typename P> static int make(const char *pre, P &owner) {
    owner.reset(new (std::nothrow) typename P::element_type());
    if (!owner) return fail(PARC_ERR_INVALID, std::string(pre) + ": out of host memory");
    return PARC_OK;
}

// ---- create ----------------------------------------------------------------------------------------------------------------------
// first half: the arguments every create refuses first; `type` is the parameter struct's name
template <typename P, typename H> static int create_args(const char *pre, const char *type, const P *p, H **out) {
    if (!p || !out) return fail(PARC_ERR_INVALID, std::string(pre) + ": null argument");
    if (p->struct_size != sizeof(P)) return fail(PARC_ERR_INVALID, std::string(type) + " ABI mismatch (struct_size)");
    return PARC_OK;
}
// ... and, of a tool with a character, the limits of p->model (dof_size where the tool checks it: `dofs`)
template <typename P, typename H> static int create_args(const char *pre, const char *type, const P *p, H **out, int min_bodies, bool dofs) {
    PARC_TRY(create_args(pre, type, p, out));
    const ParcCharModel &cm = p->model;
    if (cm.num_bodies < min_bodies || cm.num_bodies > PARC_MAX_BODIES) return fail(PARC_ERR_INVALID, std::string(pre) + ": num_bodies out of range");
    if (dofs && (cm.dof_size < 0 || cm.dof_size > PARC_MAX_DOFS)) return fail(PARC_ERR_INVALID, std::string(pre) + ": dof_size out of range");
    return PARC_OK;
}
// the tool's model (CharTree, CharPoints or a struct derived from them): zero bytes, then the tree of cm
template <typename Model> static int char_tree(const char *pre, const ParcCharModel &cm, Model &M) {
    model_zero(M);
    return model_tree(pre, cm, M);
}

static int joint_dofs(int joint_type) { return joint_type == PARC_JOINT_HINGE ? 1 : (joint_type == PARC_JOINT_SPHERICAL ? 3 : 0); }

// every joint's dofs lie inside [0, dof_size); `used` = how many there are
static int char_dofs(const char *pre, const ParcCharModel &cm, int &used) {
    used = 0;
    for (int b = 1; b < cm.num_bodies; ++b) {
        const int dd = joint_dofs(cm.joint_type[b]);
        if (dd && (cm.dof_idx[b] < 0 || cm.dof_idx[b] + dd > cm.dof_size)) return fail(PARC_ERR_INVALID, std::string(pre) + ": dof_idx out of range");
        used += dd;
    }
    return PARC_OK;
}
static int char_dofs(const char *pre, const ParcCharModel &cm) {
    int used;
    return char_dofs(pre, cm, used);
}

// second half: the handle, its device selected, then the tool's `fill` (int(H &): the settings it keeps, its device buffers, its events),
// then *out.  Every failure is a plain return: the handle goes with `h`, by destroy().
template <typename H, typename Fill> static int create(const char *pre, int device, H **out, Fill fill) {
    struct Drop { void operator()(H *h) const { destroy(h); } };
    std::unique_ptr<H, Drop> h;
    PARC_TRY(make(pre, h));
    h->device = device;
    HIPCHK(hipSetDevice(device));
    PARC_TRY(fill(*h));
    *out = h.release();
    return PARC_OK;
}
// ... of a CharHandle with DeviceEvents: the model goes up before `fill`, the events are made after it
template <typename H, typename Model, typename Fill> static int create(const char *pre, int device, const Model &M, H **out, Fill fill) {
    return create(pre, device, out, [&](H &h) -> int {
        h.host_model = M;
        PARC_TRY(model_upload(h.mem, M, h.d_model));
        PARC_TRY(fill(h));
        return h.ev.create();
    });
}
template <typename H, typename Model> static int create(const char *pre, int device, const Model &M, H **out) {   // a tool with nothing to add
    return create(pre, device, M, out, [](H &) -> int { return PARC_OK; });
}

// ---- what a handle holds between calls: a batch, a library, a result, a set of buffers -----------------------------------------------
// Replace the object of `slot`: the old one goes first (two would double the peak of device memory), the new one is `fresh`, the
// caller's local.  The caller validates before this and installs last (slot = std::move(fresh)), so a refused argument leaves the old
// object loaded and a failed allocation leaves the slot empty.
template <typename T> static int renew(const char *pre, std::unique_ptr<T> &slot, std::unique_ptr<T> &fresh) {
    slot.reset();
    return make(pre, fresh);
}

static int no_clips(const char *pre) { return fail(PARC_ERR_STATE, std::string(pre) + ": parc_" + pre + "_set_clips first"); }

// the guard of a call that needs the clips loaded (`slot`: the member parc_<pre>_set_clips fills) ...
template <typename H, typename B, typename S> static int check_loaded(const char *pre, H *h, std::unique_ptr<S> B::*slot) {
    if (!h) return fail(PARC_ERR_INVALID, std::string(pre) + ": null handle");
    if (!(h->*slot)) return no_clips(pre);
    return PARC_OK;
}
// ... and of one that reads what parc_<pre>_run left (the slot's `ran`)
template <typename H, typename B, typename S> static int check_ran(const char *pre, H *h, std::unique_ptr<S> B::*slot) {
    PARC_TRY(check_loaded(pre, h, slot));
    if (!(h->*slot)->ran) return fail(PARC_ERR_STATE, std::string(pre) + ": parc_" + pre + "_run first");
    return PARC_OK;
}

// ---- status words ----------------------------------------------------------------------------------------------------------------
struct StatusWords {                      // device ints the kernels OR their findings into, in the handle's arena
    int *d = nullptr;
    int alloc(DeviceArena &mem, int n) { return mem.alloc_fill(d, n); }
    int clear(int i, hipStream_t st) {
        HIPCHK(hipMemsetAsync(d + i, 0, sizeof(int), st));
        return PARC_OK;
    }
    int read(int i, hipStream_t st, int &v) {   // after the work queued on st: synchronises
        HIPCHK(hipMemcpyAsync(&v, d + i, sizeof(int), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        return PARC_OK;
    }
    int take(int i, hipStream_t st, int &v) {   // read, and the word starts anew
        PARC_TRY(read(i, st, v));
        HIPCHK(hipMemset(d + i, 0, sizeof(int)));
        return PARC_OK;
    }
};

// the refusal of a validate pass: bit k of v is names[k]
template <typename Name, size_t N> static int bad_plan(const char *pre, int v, const Name (&names)[N]) {
    std::string msg;
    for (size_t k = 0; k < N; ++k) if (v & (1 << k)) msg += std::string(msg.empty() ? "" : "; ") + names[k];
    return fail(PARC_ERR_INVALID, std::string(pre) + ": bad plan: " + msg);
}

// ---- parc_*_kernel_times -----------------------------------------------------------------------------------------------------------
// of a tool whose run stores its milliseconds: zeros until one ran
template <typename H, typename B, size_t N> static int stored_times(const char *pre, H *h, float (B::*ms)[N], float *out) {
    if (!h || !out) return fail(PARC_ERR_INVALID, std::string(pre) + ": null argument");
    for (size_t k = 0; k < N; ++k) out[k] = (h->*ms)[k];
    return PARC_OK;
}

// of a tool that keeps the events: out[k] = span k where its events were recorded (waiting for its end), else 0; `none_yet`, the tool's
// own wording, where no span was
struct Span { bool recorded; int from, to; };
template <typename Events, size_t N> static int span_times(const char *none_yet, int device, const Events &ev, const Span (&spans)[N], float *out) {
    bool any = false;
    for (const Span &s : spans) any |= s.recorded;
    if (!any) return fail(PARC_ERR_STATE, none_yet);
    HIPCHK(hipSetDevice(device));
    for (size_t k = 0; k < N; ++k) {
        out[k] = 0.f;
        if (!spans[k].recorded) continue;
        HIPCHK(hipEventSynchronize(ev[spans[k].to]));
        PARC_TRY(ev.elapsed(out[k], spans[k].from, spans[k].to));
    }
    return PARC_OK;
}

}  // namespace tool
