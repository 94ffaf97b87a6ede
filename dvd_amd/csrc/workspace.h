// Carving one caller-provided buffer into aligned pieces; host only, plain C++ (jpegdec_core.h brings it into a CPU program).
#pragma once
#include <stddef.h>

namespace dvd {

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// take() returns the offset of the next piece and moves `at` behind it, rounded up to `align`; `at` is the total so far.
struct Carver {
  size_t at = 0;
  size_t take(size_t bytes, size_t align = 256) {
    const size_t o = at;
    at += align_up(bytes, align);
    return o;
  }
};

}  // namespace dvd
