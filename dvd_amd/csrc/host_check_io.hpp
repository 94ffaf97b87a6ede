// File input and output of the stand-alone *_host_check.cpp programs; host only.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <vector>

// the whole file; false if it cannot be opened or read
inline bool read_all(const char* path, std::vector<uint8_t>& out) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  out.resize(n > 0 ? (size_t)n : 0);
  const bool ok = n >= 0 && fread(out.data(), 1, out.size(), f) == out.size();
  fclose(f);
  return ok;
}

inline bool write_all(const char* path, const void* p, size_t n) {
  FILE* f = fopen(path, "wb");
  if (!f) return false;
  const bool ok = fwrite(p, 1, n, f) == n;
  return fclose(f) == 0 && ok;
}

// n bytes at p behind what `out` holds: the pieces of a file that write_all then writes at once
inline void append(std::vector<uint8_t>& out, const void* p, size_t n) {
  out.insert(out.end(), (const uint8_t*)p, (const uint8_t*)p + n);
}
