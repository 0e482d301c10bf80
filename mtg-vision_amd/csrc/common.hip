#include "common.h"

namespace mtgv {
static thread_local std::string g_last_error;
void set_last_error(const std::string& s) { g_last_error = s; }
const char* last_error_cstr() { return g_last_error.c_str(); }

void DevBuf::alloc(size_t floats) {
  release();
  if (floats == 0) return;
  HIP_OK(hipMalloc((void**)&p, floats * sizeof(float)));
  n = floats;
}
void DevBuf::release() {
  if (p) (void)hipFree(p);
  p = nullptr;
  n = 0;
}
}  // namespace mtgv
