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
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { delete c; return NRS_ERR_NO_DEVICE; }
    if (hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess) {
        delete c;
        return NRS_ERR_NO_DEVICE;
    }
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
    if (c->pin_scal) (void)hipHostFree(c->pin_scal);
    if (c->pin_flags) (void)hipHostFree(c->pin_flags);
    if (c->pin_spec_scal) (void)hipHostFree(c->pin_spec_scal);
    if (c->pin_spec_flags) (void)hipHostFree(c->pin_spec_flags);
    if (c->embwin_pin) (void)hipHostFree(c->embwin_pin);
    for (int j = 0; j < 3; ++j) {
        if (c->spec_stream[j]) { (void)hipStreamSynchronize(c->spec_stream[j]); (void)hipStreamDestroy(c->spec_stream[j]); }
        if (c->spec_join[j]) (void)hipEventDestroy(c->spec_join[j]);
    }
    if (c->spec_fork) (void)hipEventDestroy(c->spec_fork);
    for (int j = 0; j < 4; ++j) if (c->spec_back[j]) (void)hipEventDestroy(c->spec_back[j]);
    if (c->arena_dba.base) (void)hipFree(c->arena_dba.base);
    if (c->arena_trk.base) (void)hipFree(c->arena_trk.base);
    c->release(c->po_uv); c->release(c->po_X); c->release(c->po_err);
    c->release(c->po_level); c->release(c->po_out); c->release(c->po_trace); c->release(c->comm_flag); c->release(c->gather_ws); c->release(c->tap); c->release(c->pack_ws); c->release(c->pack_ws2); c->release(c->pack_ws3); c->release(c->pack_ws4); c->release(c->nd_skin); c->release(c->dba_skin); c->release(c->dba_kft); c->release(c->po_multi);
    nrs::nd_cache_free(c);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
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
