// What the programs that run a kernel's __host__ __device__ routines on the CPU share (tools/bundle_host.cpp,
// tools/triangulate_host.cpp): `program input.bin output.bin`, arrays read and written whole.
#pragma once
#include <cstdio>
#include <vector>

// argv -> the input file open for reading; nullptr after saying on stderr how the program is called or what does not open.
inline std::FILE* open_input(int argc, char** argv, const char* names) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s %s\n", argv[0], names);
    return nullptr;
  }
  std::FILE* in = std::fopen(argv[1], "rb");
  if (!in) std::fprintf(stderr, "cannot open %s\n", argv[1]);
  return in;
}

inline std::FILE* open_output(const char* path) {
  std::FILE* out = std::fopen(path, "wb");
  if (!out) std::fprintf(stderr, "cannot open %s\n", path);
  return out;
}

template <typename T>
static bool read_all(std::FILE* f, std::vector<T>& v) {
  return v.empty() || std::fread(v.data(), sizeof(T), v.size(), f) == v.size();
}

template <typename T>
static void write_all(std::FILE* f, const std::vector<T>& v) {
  if (!v.empty()) std::fwrite(v.data(), sizeof(T), v.size(), f);
}
