// The library's error state (common.h: err_buf, fail, check_launch) and the two entries that report on the library itself.
#include "common.h"

namespace nerf {

static thread_local char g_err[512] = "";
char* err_buf() { return g_err; }
int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}
int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(NERF_E_HIP, "%s: %s", what, hipGetErrorString(e));
  return NERF_OK;
}

}  // namespace nerf

using namespace nerf;

extern "C" int nerf_abi_version(void) { return NERF_ABI_VERSION; }
extern "C" const char* nerf_last_error(void) { return err_buf(); }
