// mtgv - error plumbing of the C ABI.  No HIP header: host-only translation units and stand-alone checks include this.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string>
#include <stdexcept>

namespace mtgv {

// ---- error plumbing: C-ABI returns int status, text via mtgv_last_error() ----
void set_last_error(const std::string& s);

struct Error : std::runtime_error {
  int code;
  Error(int c, const std::string& s) : std::runtime_error(s), code(c) {}
};

enum Status : int {
  OK = 0,
  ERR_INVALID = 1,   // bad argument / shape (reference: AssertionError)
  ERR_KEY = 2,       // unknown name (reference: KeyError)
  ERR_RUNTIME = 3,   // HIP failure or bad state (reference: RuntimeError)
};

#define MTGV_CHECK(cond, code, ...)                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      char _b[512];                                                        \
      snprintf(_b, sizeof(_b), __VA_ARGS__);                               \
      throw ::mtgv::Error(code, std::string(_b) + " [" #cond "] at " __FILE__ ":" + std::to_string(__LINE__)); \
    }                                                                      \
  } while (0)

template <class F>
static inline int guarded(F&& f) {
  try {
    f();
    return OK;
  } catch (const Error& e) {
    set_last_error(e.what());
    return e.code;
  } catch (const std::exception& e) {
    set_last_error(e.what());
    return ERR_RUNTIME;
  }
}

static inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
static inline int64_t ceil_div64(int64_t a, int64_t b) { return (a + b - 1) / b; }

}  // namespace mtgv
