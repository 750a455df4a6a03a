// The context's life cycle: nrs_create / nrs_destroy, the options, the debug switches' snapshot of the environment and nrs_debug_set,
// and the small queries on a context.  The one place that reads the environment; the host logic (table, parsing, option handling) is
// nrs_switches.hpp, which host/ctx_check.cpp runs without a device.
#include <new>
#include "nrs_ctx.hpp"

using namespace nrs;

extern char** environ;
namespace nrs {
const DebugOpts& DebugOpts::process() {
    static const DebugOpts snap = [] { DebugOpts d; d.load_environment(environ); return d; }();
    return snap;
}

// The four places the library gives a GPU resource back (nrs_own.hpp): nothing else calls these HIP functions.
void dev_free(void* p) noexcept { if (p) (void)hipFree(p); }
void pin_free(void* p) noexcept { if (p) (void)hipHostFree(p); }
void stream_destroy(ihipStream_t* s) noexcept { if (s) (void)hipStreamDestroy(s); }
void event_destroy(ihipEvent_t* e) noexcept { if (e) (void)hipEventDestroy(e); }
}  // namespace nrs

extern "C" int nrs_debug_set(nrs_ctx* c, const char* name, const char* value) {
    if (!c || !name || strncmp(name, "NRS_", 4) != 0) return NRS_ERR_INVALID;
    c->dbg.set_by_name(name, value);
    return NRS_OK;
}

extern "C" void nrs_options_init(nrs_options* opt) {
    if (!opt) return;
    memset(opt, 0, sizeof(*opt));
    opt->device = -1;
    opt->struct_size = (uint32_t)sizeof(*opt);
}

extern "C" int nrs_create(nrs_ctx** out, const nrs_options* opt) {
    if (!out) return NRS_ERR_INVALID;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return NRS_ERR_NO_DEVICE;
    nrs_ctx* c = new (std::nothrow) nrs_ctx();
    if (!c) return NRS_ERR_ALLOC;
    c->dbg.load_environment(environ);
    if (const int rc = resolve_options(opt, c->dbg, &c->opt)) { delete c; return rc; }
    c->err[0] = 0;
    memset(&c->prof, 0, sizeof(c->prof));
    int dev = c->opt.device;
    if (dev < 0) {
        if (hipGetDevice(&dev) != hipSuccess) { delete c; return NRS_ERR_NO_DEVICE; }
    }
    if (dev >= ndev || hipSetDevice(dev) != hipSuccess) { delete c; return NRS_ERR_NO_DEVICE; }
    c->device = dev;
    if (hipGetDeviceProperties(&c->prop, dev) != hipSuccess) { delete c; return NRS_ERR_NO_DEVICE; }
    if (stream_create(c->main_stream) != hipSuccess || event_create(c->ev0, hipEventDefault) != hipSuccess ||
        event_create(c->ev1, hipEventDefault) != hipSuccess) {
        delete c;                                                  // (what was created goes with it)
        return NRS_ERR_NO_DEVICE;
    }
    c->stream = c->main_stream.get();
    *out = c;
    return NRS_OK;
}

extern "C" void nrs_destroy(nrs_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    nrs::dba_free(c);
    nrs::klt_free(c);
    nrs::shi_free(c);
    nrs::front_free(c);
    nrs::comm_free(c);
    for (auto& s : c->spec_stream) if (s) (void)hipStreamSynchronize(s.get());
    nrs::nd_cache_free(c);
    delete c;                                                      // every buffer, pinned word, event and stream it owns
}

extern "C" const char* nrs_last_error(const nrs_ctx* c) { return c ? c->err : "null context"; }

extern "C" int nrs_device_name(const nrs_ctx* c, char* buf, int32_t len) {
    if (!c || !buf || len <= 0) return NRS_ERR_INVALID;
    snprintf(buf, (size_t)len, "%s (%s, %d CUs)", c->prop.name, c->prop.gcnArchName, c->prop.multiProcessorCount);
    return NRS_OK;
}

extern "C" int nrs_get_profile(const nrs_ctx* c, nrs_profile* out) {
    if (!c || !out) return NRS_ERR_INVALID;
    *out = c->prof;
    return NRS_OK;
}

extern "C" int nrs_reset_profile(nrs_ctx* c) {
    if (!c) return NRS_ERR_INVALID;
    memset(&c->prof, 0, sizeof(c->prof));
    return NRS_OK;
}

extern "C" void* nrs_stream(nrs_ctx* c) { return c ? (void*)c->stream : nullptr; }
