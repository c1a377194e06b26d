// env_size.hpp -- the positive-integer environment knob (chunk and piece sizes
// of the bulk engines).  Plain C++, no HIP: the headers that the CPU tests
// compile alone (segments_plan.hpp, the host part of hash_to_curve.hpp) use it.
#pragma once
#include <stddef.h>
#include <stdlib.h>

namespace msm {

// the value of environment variable `name` when it is a positive integer, else 0; read at each call
inline size_t env_size(const char *name) {
  const char *e = getenv(name);
  if (e && *e) {
    const long long v = atoll(e);
    if (v > 0) return (size_t)v;
  }
  return 0;
}

}  // namespace msm
