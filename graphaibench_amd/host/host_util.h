// host_util.h -- internal helpers of the host C++ mirror.
#pragma once
#include "gaib.h"
#include "gpu_context.h"

namespace gaib_host {
// accumulates wall time into time_ops[op] when GAIB_SYNC_TIMERS=1 (the reference times every op
// around a device-wide sync: cutils.h:18-28; here the sync is opt-in so the default path stays
// asynchronous)
struct OpTimer {
  explicit OpTimer(char op);
  ~OpTimer();
  char op_;
  double t0_;
};

template <typename T>
inline T* dmalloc(size_t n) {
  void* p = nullptr;
  GAIB_OR_DIE(gaib_malloc(gpu_context::get(), (n > 0 ? n : 1) * sizeof(T), &p));
  return static_cast<T*>(p);
}
// the value of option `name` on the process context (gaib_get_option)
inline int64_t option(const char* name) {
  int64_t v = 0;
  GAIB_OR_DIE(gaib_get_option(gpu_context::get(), name, &v));
  return v;
}
// option drop_seed_dev (math_functions.cpp): dropout mask seeds in device memory, read and advanced by gaib_dropout_dev
inline bool drop_seed_dev_option() { return option("drop_seed_dev") != 0; }
inline bool capturing() { return option("capturing") != 0; }  // a recording is open on the process context (gaib_capture_begin)
uint64_t* new_seed_slot(uint64_t seed);  // one 8-byte device slot holding `seed`; allocates and waits: not inside a capture
}  // namespace gaib_host
