// Host driver of csrc/dev_pool.h for tests/test_dev_pool.py: DevPool against a fake HIP runtime (malloc-backed, a set of
// live blocks, a switch that makes the k-th allocation fail), built with g++ under AddressSanitizer and
// UndefinedBehaviorSanitizer.  No GPU, nothing loaded into Python.
//
//   dev_pool_driver               every case; one "<case> ok" line each, exit status 0 iff all passed and nothing is live
//   dev_pool_driver double_free   frees one block twice: the fake runtime must abort (the test expects that)
//   dev_pool_driver unknown_free  frees a pointer the fake runtime never handed out: the same
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <utility>

#include "../../relationprediction_amd/csrc/dev_pool.h"

// ---------------------------------------------------------------- the fake runtime
namespace {
std::map<void*, size_t> g_live;          // block -> bytes
long g_mallocs = 0, g_frees = 0, g_memsets = 0;
long g_fail_at = -1;                     // the allocation with this index (counted from 0 since arm()) fails ...
hipError_t g_fail_with = hipSuccess;     // ... with this error
long g_alloc_index = 0;
hipStream_t g_last_memset_stream = nullptr;
bool g_fail_memset = false;              // the next hipMemsetAsync fails (and writes nothing)

void arm(long k, hipError_t e) {
  g_fail_at = k;
  g_fail_with = e;
  g_alloc_index = 0;
}
void disarm() {
  g_fail_at = -1;
  g_fail_memset = false;
}
size_t live_bytes() {
  size_t n = 0;
  for (const auto& kv : g_live) n += kv.second;
  return n;
}
}  // namespace

extern "C" {
hipError_t hipMalloc(void** ptr, size_t size) {
  if (g_fail_at >= 0 && g_alloc_index++ == g_fail_at) {
    *ptr = reinterpret_cast<void*>(0x1);      // a real runtime leaves garbage behind on failure: the pool must not pass it on
    return g_fail_with;
  }
  if (size == 0) {
    fprintf(stderr, "fake hipMalloc: zero-byte request\n");
    abort();
  }
  void* p = malloc(size);
  memset(p, 0xAB, size);
  g_live[p] = size;
  ++g_mallocs;
  *ptr = p;
  return hipSuccess;
}
hipError_t hipFree(void* ptr) {
  auto it = g_live.find(ptr);
  if (it == g_live.end()) {
    fprintf(stderr, "fake hipFree: %p is not a live block (unknown pointer or double free)\n", ptr);
    abort();
  }
  g_live.erase(it);
  free(ptr);
  ++g_frees;
  return hipSuccess;
}
hipError_t hipMemsetAsync(void* dst, int value, size_t bytes, hipStream_t stream) {
  auto it = g_live.find(dst);
  if (it == g_live.end() || bytes > it->second) {
    fprintf(stderr, "fake hipMemsetAsync: %zu bytes at %p is not inside a live block\n", bytes, dst);
    abort();
  }
  if (g_fail_memset) {
    g_fail_memset = false;
    return hipErrorInvalidValue;
  }
  memset(dst, value, bytes);
  ++g_memsets;
  g_last_memset_stream = stream;
  return hipSuccess;
}
const char* hipGetErrorString(hipError_t e) { return e == hipErrorOutOfMemory ? "out of memory" : "some other error"; }
}

// ---------------------------------------------------------------- the cases
namespace {
using rgcn::DevPool;
int g_failed = 0;
bool g_case_ok = true;

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      printf("  FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);           \
      g_case_ok = false;                                                   \
    }                                                                      \
  } while (0)

// the pool's counts against the driver's own
#define CHECK_COUNTS(pool, nblocks, nbytes)                                \
  do {                                                                     \
    CHECK((pool).blocks() == (int64_t)(nblocks));                          \
    CHECK((pool).bytes() == (int64_t)(nbytes));                            \
  } while (0)

void run(const char* name, void (*fn)()) {
  g_case_ok = true;
  disarm();
  const size_t live_before = g_live.size();
  fn();
  if (g_live.size() != live_before) {
    printf("  FAILED: %zu blocks live after the case (%zu before)\n", g_live.size(), live_before);
    g_case_ok = false;
  }
  printf("%s %s\n", name, g_case_ok ? "ok" : "FAILED");
  if (!g_case_ok) ++g_failed;
}

const hipStream_t kStream = reinterpret_cast<hipStream_t>(0x5151);

void case_zero_elements() {
  DevPool pool;
  double* p = nullptr;
  std::string err;
  CHECK(pool.alloc(&p, 0, false, kStream, &err) == RGCN_OK);
  CHECK(p != nullptr);
  CHECK(g_live.count(p) == 1 && g_live[p] == sizeof(double));      // one element
  CHECK_COUNTS(pool, 1, sizeof(double));
  void* raw = nullptr;
  CHECK(pool.alloc(&raw, 0, false, kStream, &err) == RGCN_OK);     // the byte form: one byte
  CHECK(g_live.count(raw) == 1 && g_live[raw] == 1);
  CHECK_COUNTS(pool, 2, sizeof(double) + 1);
  CHECK(err.empty());
}

void case_zeroing() {
  DevPool pool;
  int32_t *z = nullptr, *n = nullptr;
  const long memsets = g_memsets;
  CHECK(pool.alloc(&z, 100, true, kStream, nullptr) == RGCN_OK);
  CHECK(g_memsets == memsets + 1 && g_last_memset_stream == kStream);
  CHECK(pool.alloc(&n, 100, false, kStream, nullptr) == RGCN_OK);
  CHECK(g_memsets == memsets + 1);                                   // no memset was queued
  bool zeros = true, untouched = true;
  for (int i = 0; i < 100; ++i) {
    zeros = zeros && z[i] == 0;
    untouched = untouched && (uint32_t)n[i] == 0xABABABABu;          // what the fake hipMalloc filled the block with
  }
  CHECK(zeros);
  CHECK(untouched);
  CHECK_COUNTS(pool, 2, 800);
}

void case_release_once() {
  DevPool pool;
  float* p[5];
  size_t bytes = 0;
  for (int i = 0; i < 5; ++i) {
    CHECK(pool.alloc(&p[i], (size_t)(10 + i), false, kStream, nullptr) == RGCN_OK);
    bytes += (size_t)(10 + i) * sizeof(float);
    CHECK_COUNTS(pool, i + 1, bytes);
    CHECK(live_bytes() == bytes);
  }
  const long frees = g_frees;
  pool.release();
  CHECK(g_frees == frees + 5);
  CHECK(g_live.empty());
  CHECK_COUNTS(pool, 0, 0);
  pool.release();                      // idempotent: the fake hipFree would abort on a repeated pointer
  CHECK(g_frees == frees + 5);
  CHECK(pool.alloc(&p[0], 3, false, kStream, nullptr) == RGCN_OK);      // and the pool is usable again
  CHECK_COUNTS(pool, 1, 12);
}

void case_destructor() {
  const long frees = g_frees;
  {
    DevPool pool;
    char* a = nullptr;
    uint64_t* b = nullptr;
    CHECK(pool.alloc(&a, 7, false, kStream, nullptr) == RGCN_OK);
    CHECK(pool.alloc(&b, 2, true, kStream, nullptr) == RGCN_OK);
    CHECK(g_live.size() == 2);
  }
  CHECK(g_frees == frees + 2);
  CHECK(g_live.empty());
}

void case_move() {
  const long frees = g_frees;
  {
    DevPool a;
    float* p = nullptr;
    CHECK(a.alloc(&p, 4, false, kStream, nullptr) == RGCN_OK);
    CHECK(a.alloc(&p, 8, false, kStream, nullptr) == RGCN_OK);
    DevPool b(std::move(a));
    CHECK_COUNTS(a, 0, 0);
    CHECK_COUNTS(b, 2, 48);
    CHECK(g_frees == frees);
    DevPool c;
    CHECK(c.alloc(&p, 1, false, kStream, nullptr) == RGCN_OK);
    c = std::move(b);                  // what c held is freed, b's blocks move over
    CHECK(g_frees == frees + 1);
    CHECK_COUNTS(b, 0, 0);
    CHECK_COUNTS(c, 2, 48);
    a.release();
    b.release();
    CHECK(g_frees == frees + 1);
  }
  CHECK(g_frees == frees + 3);         // each block exactly once
  CHECK(g_live.empty());
}

// a struct that holds a pool beside its pointers, swapped and reset by assignment the way GraphBufs is
struct Bufs {
  DevPool pool;
  int32_t* x = nullptr;
  int tag = 0;
};

void case_swap() {
  Bufs g, g_alt;
  g.tag = 1;
  g_alt.tag = 2;
  CHECK(g.pool.alloc(&g.x, 16, false, kStream, nullptr) == RGCN_OK);
  CHECK(g_alt.pool.alloc(&g_alt.x, 32, false, kStream, nullptr) == RGCN_OK);
  int32_t *x1 = g.x, *x2 = g_alt.x;
  std::swap(g, g_alt);
  CHECK(g.tag == 2 && g.x == x2 && g_alt.tag == 1 && g_alt.x == x1);
  CHECK_COUNTS(g.pool, 1, 128);
  CHECK_COUNTS(g_alt.pool, 1, 64);
  CHECK(g_live.size() == 2);
  g.pool.release();                    // frees the block that travelled with it, and only that one
  CHECK(g_live.size() == 1 && g_live.count(x1) == 1);
  g_alt = Bufs();                      // reset by assignment frees the other
  CHECK(g_live.empty());
  CHECK(g_alt.x == nullptr && g_alt.tag == 0);
  CHECK_COUNTS(g_alt.pool, 0, 0);
}

void fail_kth(int n, int k, hipError_t injected, rgcn_status want) {
  DevPool pool;
  float* p[8] = {};
  std::string err;
  arm(k, injected);
  size_t bytes = 0;
  for (int i = 0; i < n; ++i) {
    err.clear();
    const rgcn_status s = pool.alloc(&p[i], (size_t)(i + 1), true, kStream, &err);
    if (i == k) {
      CHECK(s == want);
      CHECK(p[i] == nullptr);
      CHECK(err.find("hipMalloc of " + std::to_string((i + 1) * sizeof(float)) + " bytes: ") == 0);      // what was asked for
      CHECK(err.find(hipGetErrorString(injected)) != std::string::npos);
    } else {
      CHECK(s == RGCN_OK);
      CHECK(p[i] != nullptr);
      bytes += (size_t)(i + 1) * sizeof(float);
    }
    CHECK_COUNTS(pool, i < k ? i + 1 : i, bytes);        // nothing was recorded for the failed one
    CHECK(g_live.size() == (size_t)pool.blocks() && live_bytes() == bytes);
  }
  for (int i = 0; i < n; ++i)
    if (i != k) CHECK(g_live.count(p[i]) == 1);          // earlier (and later) blocks are still live
  const long frees = g_frees;
  pool.release();
  CHECK(g_frees == frees + n - 1);
  CHECK(g_live.empty());
}

void case_fail_nomem() {
  for (int k = 0; k < 5; ++k) fail_kth(5, k, hipErrorOutOfMemory, RGCN_ERR_NOMEM);
}
void case_fail_other() {
  for (int k = 0; k < 5; ++k) fail_kth(5, k, hipErrorInvalidValue, RGCN_ERR_HIP);
  DevPool pool;                        // a null error string is allowed
  float* p = nullptr;
  arm(0, hipErrorInvalidDevice);
  CHECK(pool.alloc(&p, 4, false, kStream, nullptr) == RGCN_ERR_HIP);
  CHECK(p == nullptr);
  CHECK_COUNTS(pool, 0, 0);
}

// the memset of a zeroed allocation fails: the block goes back, nothing is recorded, the pool stays usable
void case_fail_memset() {
  DevPool pool;
  float *a = nullptr, *b = nullptr;
  std::string err;
  CHECK(pool.alloc(&a, 6, true, kStream, &err) == RGCN_OK);
  const long mallocs = g_mallocs, frees = g_frees;
  g_fail_memset = true;
  CHECK(pool.alloc(&b, 9, true, kStream, &err) == RGCN_ERR_HIP);
  CHECK(b == nullptr);
  CHECK(err.find("hipMemsetAsync of 36 bytes: ") == 0);
  CHECK(g_mallocs == mallocs + 1 && g_frees == frees + 1);      // allocated, then handed back
  CHECK_COUNTS(pool, 1, 24);
  CHECK(g_live.size() == 1 && g_live.count(a) == 1);
  g_fail_at = 0;                       // n = 0: the message names the 0 bytes asked for, not the element allocated
  g_fail_with = hipErrorOutOfMemory;
  g_alloc_index = 0;
  CHECK(pool.alloc(&b, 0, false, kStream, &err) == RGCN_ERR_NOMEM);
  CHECK(err.find("hipMalloc of 0 bytes: ") == 0);
  disarm();
  CHECK(pool.alloc(&b, 9, true, kStream, &err) == RGCN_OK);
  CHECK_COUNTS(pool, 2, 60);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc > 1 && std::string(argv[1]) == "double_free") {
    void* p = nullptr;
    (void)hipMalloc(&p, 8);
    (void)hipFree(p);
    (void)hipFree(p);
    return 0;      // not reached
  }
  if (argc > 1 && std::string(argv[1]) == "unknown_free") {
    int local = 0;
    (void)hipFree(&local);
    return 0;      // not reached
  }
  run("zero_elements", case_zero_elements);
  run("zeroing", case_zeroing);
  run("release_once", case_release_once);
  run("destructor", case_destructor);
  run("move", case_move);
  run("swap", case_swap);
  run("fail_nomem", case_fail_nomem);
  run("fail_other", case_fail_other);
  run("fail_memset", case_fail_memset);
  printf("mallocs=%ld frees=%ld live=%zu\n", g_mallocs, g_frees, g_live.size());
  return g_failed == 0 && g_live.empty() && g_mallocs == g_frees ? 0 : 1;
}
