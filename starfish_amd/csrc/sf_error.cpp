// Error text of the calling thread (sf_last_error) and the version string.  Plain C++: no HIP.
#include <cstdarg>
#include <cstdio>

#include "sf_base.h"

static thread_local char g_err[512] = "";
void sf_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
extern "C" const char* sf_last_error(void) { return g_err; }
extern "C" const char* sf_version(void) { return "starfish_amd 0.1 (gfx950)"; }
