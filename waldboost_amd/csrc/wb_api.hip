// C-ABI glue: error reporting and the ABI version.  (The cascade model handle is wb_model.hip.)
#include "wb_common.h"

static thread_local char g_err[512] = "";

void wb_set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char *wb_last_error(void) { return g_err; }
extern "C" int wb_abi_version(void) { return WB_ABI_VERSION; }
