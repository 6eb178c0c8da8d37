// Case files of the host drivers (tests/test_host_sanitizers_cpu.py writes them, the drivers read them).
//
// A case directory holds `cases.txt` and raw little-endian arrays.  cases.txt:
//     case <name> <op>
//     i <key> <signed 64-bit integer>
//     a <key> <file name>
//     end
// Every array a driver hands to the library is a heap allocation of EXACTLY the size the header documents, so that the
// sanitizer's red zone starts where the contract ends; a zero-length array is a zero-byte allocation (non-null).
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

namespace host {

constexpr unsigned char CANARY = 0xA5;

struct Case {
  std::string dir, name, op;
  std::map<std::string, int64_t> ints;
  std::map<std::string, std::string> files;
};

[[noreturn]] inline void fail(const Case &c, const std::string &what) {
  std::fprintf(stderr, "MISMATCH case %s (%s): %s\n", c.name.c_str(), c.op.c_str(), what.c_str());
  std::exit(1);
}

inline std::vector<Case> read_cases(const std::string &dir) {
  std::ifstream in(dir + "/cases.txt");
  if (!in) { std::fprintf(stderr, "cannot read %s/cases.txt\n", dir.c_str()); std::exit(2); }
  std::vector<Case> out;
  std::string line;
  bool open = false;
  while (std::getline(in, line)) {
    std::istringstream ls(line);
    std::string tag;
    if (!(ls >> tag)) continue;
    if (tag == "case") {
      out.emplace_back();
      out.back().dir = dir;
      ls >> out.back().name >> out.back().op;
      open = true;
    } else if (tag == "end") {
      open = false;
    } else if (open && tag == "i") {
      std::string k;
      long long v;
      ls >> k >> v;
      out.back().ints[k] = (int64_t)v;
    } else if (open && tag == "a") {
      std::string k, f;
      ls >> k >> f;
      out.back().files[k] = f;
    } else {
      std::fprintf(stderr, "bad line in cases.txt: %s\n", line.c_str());
      std::exit(2);
    }
  }
  if (open) { std::fprintf(stderr, "cases.txt: unterminated case\n"); std::exit(2); }
  return out;
}

inline int64_t geti(const Case &c, const char *key) {
  auto it = c.ints.find(key);
  if (it == c.ints.end()) fail(c, std::string("manifest lacks integer ") + key);
  return it->second;
}
inline int64_t geti(const Case &c, const char *key, int64_t dflt) {
  auto it = c.ints.find(key);
  return it == c.ints.end() ? dflt : it->second;
}
inline bool has(const Case &c, const char *key) { return c.files.count(key) != 0; }

// exactly n elements, never null
template <class T>
T *exact(int64_t n) {
  void *p = std::malloc((size_t)n * sizeof(T));
  if (!p) { std::fprintf(stderr, "out of memory\n"); std::exit(2); }
  return static_cast<T *>(p);
}
template <class T>
T *exact_canary(int64_t n) {
  T *p = exact<T>(n);
  if (n > 0) std::memset(p, CANARY, (size_t)n * sizeof(T));
  return p;
}

// the array `key` of the case, which must hold exactly n elements of T
template <class T>
T *load(const Case &c, const char *key, int64_t n) {
  auto it = c.files.find(key);
  if (it == c.files.end()) fail(c, std::string("manifest lacks array ") + key);
  std::FILE *f = std::fopen((c.dir + "/" + it->second).c_str(), "rb");
  if (!f) fail(c, "cannot open " + it->second);
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  if (n < 0 || (int64_t)bytes != n * (int64_t)sizeof(T))
    fail(c, std::string(key) + ": file holds " + std::to_string(bytes) + " bytes, the case needs " + std::to_string(n * (int64_t)sizeof(T)));
  T *p = exact<T>(n);
  if (bytes > 0 && std::fread(p, 1, (size_t)bytes, f) != (size_t)bytes) fail(c, "short read of " + it->second);
  std::fclose(f);
  return p;
}

// got[0..n) against the array `key`; the first differing element is named
template <class T>
void expect_eq(const Case &c, const char *key, const T *got, int64_t n, const std::string &tag = "") {
  T *want = load<T>(c, key, n);
  for (int64_t i = 0; i < n; ++i)
    if (std::memcmp(&got[i], &want[i], sizeof(T)) != 0)
      fail(c, tag + key + "[" + std::to_string(i) + "]: got " + std::to_string((long long)got[i]) + ", expected " + std::to_string((long long)want[i]));
  std::free(want);
}

template <class T>
void expect_canary(const Case &c, const char *what, const T *p, int64_t n) {
  const unsigned char *b = reinterpret_cast<const unsigned char *>(p);
  for (int64_t i = 0; i < n * (int64_t)sizeof(T); ++i)
    if (b[i] != CANARY) fail(c, std::string(what) + ": byte " + std::to_string(i) + " of an output was written by a refused call");
}

template <class T>
void expect_same(const Case &c, const char *what, const T *a, const T *b, int64_t n) {
  for (int64_t i = 0; i < n; ++i)
    if (std::memcmp(&a[i], &b[i], sizeof(T)) != 0) fail(c, std::string(what) + "[" + std::to_string(i) + "] differs");
}

template <class T>
T *clone(const T *src, int64_t n) {
  T *p = exact<T>(n);
  if (n > 0) std::memcpy(p, src, (size_t)n * sizeof(T));
  return p;
}

inline void expect_rc(const Case &c, const char *call, int got, int64_t want) {
  if ((int64_t)got != want) fail(c, std::string(call) + " returned " + std::to_string(got) + ", expected " + std::to_string((long long)want));
}

}  // namespace host
