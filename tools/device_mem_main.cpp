// Driver of tools/device_mem_sanitize.sh and tests/test_device_mem_cpu.py: DevBuf (csrc/device_mem.h) on the host.  The
// five functions the header leaves to context.hip are stand-ins over malloc / free with the same two counters, a switch
// for "the context is gone" and a countdown that makes an allocation fail.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <map>
#include <utility>

#include "device_mem.h"

static std::atomic<int64_t> g_bytes{0}, g_blocks{0};
static std::map<void *, size_t> g_size;
static bool g_live = true;
static int g_fail_in = -1;          // the allocation that many calls from now fails (-1: none)
static int g_syncs = 0;

namespace rlh {
bool device_context_live() { return g_live; }
int device_alloc(void **p, size_t bytes) {
  *p = nullptr;
  if (g_fail_in == 0) { g_fail_in = -1; return 2; }
  if (g_fail_in > 0) --g_fail_in;
  if (bytes == 0) return 0;          // (hipMalloc of nothing: success and a null pointer)
  *p = malloc(bytes);
  if (!*p) return 2;
  g_size[*p] = bytes;
  g_bytes += (int64_t)bytes;
  g_blocks += 1;
  return 0;
}
void device_release(void *p) {
  if (!p || !device_context_live()) return;
  auto it = g_size.find(p);
  if (it == g_size.end()) { fprintf(stderr, "release of a block that is not alive\n"); abort(); }
  g_bytes -= (int64_t)it->second;
  g_blocks -= 1;
  g_size.erase(it);
  free(p);
}
int device_copy_in(void *dst, const void *src, size_t bytes) { memcpy(dst, src, bytes); return 0; }
int device_stream_sync() { ++g_syncs; return 0; }
}  // namespace rlh

using rlh::DevBuf;

static int g_bad = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); ++g_bad; } } while (0)
static bool live(int64_t bytes, int64_t blocks) { return g_bytes == bytes && g_blocks == blocks; }

struct Several { DevBuf<int32_t> a; DevBuf<double> b; DevBuf<void> c; };
static int fill(Several &s) {
  if (int rc = s.a.alloc(10)) return rc;
  if (int rc = s.b.alloc(10)) return rc;
  return s.c.alloc(10);
}

int main() {
  {  // alloc / reset / destructor; the conversions
    DevBuf<int32_t> a;
    CHECK(a.get() == nullptr && a.bytes() == 0 && !a);
    CHECK(a.alloc(100) == 0 && a.bytes() == 400 && live(400, 1));
    int32_t *raw = a;
    CHECK(raw == a.get() && (char *)a == (char *)raw);
    raw[99] = 7;
    CHECK(a.alloc(3) == 0 && a.bytes() == 12 && live(12, 1));          // what it held is released first
    a.reset();
    CHECK(a.get() == nullptr && a.bytes() == 0 && live(0, 0));
    a.reset();                                                          // twice: nothing to do
    DevBuf<void> v;
    CHECK(v.alloc(33) == 0 && v.bytes() == 33);                         // bytes for DevBuf<void>
    ((char *)v)[32] = 1;
    DevBuf<double> d;
    CHECK(d.alloc(5) == 0 && live(33 + 40, 2));
    CHECK(d.alloc(0) == 0 && d.get() == nullptr && live(33, 1));        // nothing asked for: empty, no block
  }
  CHECK(live(0, 0));
  {  // move construction and move assignment onto a non-empty buffer
    DevBuf<int64_t> a, b;
    CHECK(a.alloc(4) == 0 && b.alloc(8) == 0 && live(96, 2));
    int64_t *pa = a;
    DevBuf<int64_t> c(std::move(a));
    CHECK(c.get() == pa && c.bytes() == 32 && a.get() == nullptr && a.bytes() == 0 && live(96, 2));
    b = std::move(c);                                                   // b's 64 bytes go
    CHECK(b.get() == pa && b.bytes() == 32 && c.get() == nullptr && live(32, 1));
    DevBuf<int64_t> &self = b;
    b = std::move(self);
    CHECK(b.get() == pa && live(32, 1));
  }
  CHECK(live(0, 0));
  {  // upload with at_least
    const char text[8] = "1234567";
    DevBuf<char> u;
    CHECK(u.upload(text, 8) == 0 && u.bytes() == 8 && !memcmp(u.get(), text, 8));
    CHECK(u.upload(text, 8, 64) == 0 && u.bytes() == 64 && !memcmp(u.get(), text, 8) && live(64, 1));
    CHECK(u.upload(nullptr, 0, 4) == 0 && u.bytes() == 4 && live(4, 1));    // an empty array still gets its block
    CHECK(u.upload(nullptr, 0) == 0 && u.get() == nullptr && live(0, 0));
  }
  {  // reserve: growing, not growing, after a failed allocation
    DevBuf<char> w;
    g_syncs = 0;
    CHECK(w.reserve(0) == 0 && w.get() == nullptr && g_syncs == 0);
    CHECK(w.reserve(100) == 0 && w.bytes() == 100 && g_syncs == 1 && live(100, 1));
    char *p = w;
    CHECK(w.reserve(60) == 0 && w.reserve(100) == 0 && w.get() == p && w.bytes() == 100 && g_syncs == 1);
    CHECK(w.reserve(101) == 0 && w.bytes() == 101 && g_syncs == 2 && live(101, 1));
    g_fail_in = 0;
    CHECK(w.reserve(500) != 0 && w.get() == nullptr && w.bytes() == 0 && live(0, 0));   // the capacity is 0, not 101
    CHECK(w.reserve(50) == 0 && w.bytes() == 50 && live(50, 1));
  }
  CHECK(live(0, 0));
  {  // a failing allocation in the middle of a struct of several buffers
    for (int k = 0; k < 3; ++k) {
      Several s;
      g_fail_in = k;
      CHECK(fill(s) != 0 && g_blocks == k);
    }
    CHECK(live(0, 0));
    Several s;
    CHECK(fill(s) == 0 && live(40 + 80 + 10, 3));
  }
  CHECK(live(0, 0));
  void *stranded[2] = {nullptr, nullptr};
  {  // release once the context is gone: nothing is freed, nothing crashes, the owners forget their blocks
    DevBuf<float> a, b;
    CHECK(a.alloc(6) == 0 && b.alloc(6) == 0 && live(48, 2));
    stranded[0] = a.get(); stranded[1] = b.get();
    g_live = false;
    a.reset();
    CHECK(a.get() == nullptr && a.bytes() == 0 && live(48, 2));
    CHECK(g_size.count(stranded[0]) == 1);
  }                                                                     // b's destructor
  CHECK(live(48, 2));
  g_live = true;
  for (void *p : stranded) rlh::device_release(p);                      // (the test's own tidying up)
  CHECK(live(0, 0) && g_size.empty());
  printf(g_bad ? "FAILED\n" : "all ok\n");
  return g_bad ? 1 : 0;
}
