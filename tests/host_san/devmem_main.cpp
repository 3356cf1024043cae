// The owners of device memory (QkDevBufT / QkGrowBufT, csrc/qk_devmem.h) over a malloc-backed allocator that counts its calls and
// can be told to fail its n-th allocation.  Built with g++ -fsanitize=address,undefined and run with detect_leaks=1 by
// tests/test_devmem.py: a leak, a double free or a use after free ends the run; prints one line per case, exits 1 on a mismatch.
#include "../../qml-cutensornet_amd/csrc/qk_devmem.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>

namespace {

struct CountingAlloc {
  static int allocs, frees, fail_at;  // fail_at: the allocation (counted from 1) that returns an error; 0 = none
  static int alloc(void** p, size_t bytes) {
    if (++allocs == fail_at) return 2;  // (hipErrorOutOfMemory; *p is left as it was, like hipMalloc)
    *p = std::malloc(bytes ? bytes : 1);
    return *p ? 0 : 2;
  }
  static void free(void* p) { ++frees, std::free(p); }
  static void start(int fail = 0) { allocs = frees = 0, fail_at = fail; }
  static int live() { return allocs - (fail_at > 0 && allocs >= fail_at ? 1 : 0) - frees; }
};
int CountingAlloc::allocs = 0, CountingAlloc::frees = 0, CountingAlloc::fail_at = 0;

using Buf = QkDevBufT<CountingAlloc>;
using Grow = QkGrowBufT<CountingAlloc>;
using A = CountingAlloc;

int failures = 0;
#define CHECK(cond)                                               \
  do {                                                            \
    if (!(cond)) std::printf("FAIL %s:%d: %s\n", __func__, __LINE__, #cond), ++failures; \
  } while (0)

void move_leaves_the_source_empty() {
  A::start();
  {
    Buf a;
    CHECK(!a && a.get() == nullptr);
    CHECK(a.alloc(64) == 0 && a);
    std::memset(a.get(), 0xAB, 64);
    void* const p = a.get();
    Buf b(std::move(a));
    CHECK(!a && a.get() == nullptr && b.get() == p);
    Buf c;
    CHECK(c.alloc(16) == 0);
    c = std::move(b);  // frees c's 16 bytes, takes p
    CHECK(!b && c.get() == p && A::frees == 1);
    CHECK(c.get<unsigned char>()[63] == 0xAB);
  }
  CHECK(A::allocs == 2 && A::frees == 2 && A::live() == 0);
}

void release_passes_ownership() {
  A::start();
  void* kept = nullptr;
  {
    Buf a;
    CHECK(a.alloc(32) == 0);
    kept = a.release();
    CHECK(kept != nullptr && !a);
  }
  CHECK(A::frees == 0 && A::live() == 1);  // the destructor freed nothing
  A::free(kept);
  CHECK(A::live() == 0);
  {
    Buf a;
    CHECK(a.alloc(8) == 0);
    a.reset();
    CHECK(!a && A::frees == 2);
    a.reset();  // empty: nothing to free
    CHECK(A::frees == 2);
    CHECK(a.alloc(8) == 0 && a.alloc(24) == 0);  // alloc on a full buffer frees what it held
    CHECK(A::frees == 3);
  }
  CHECK(A::live() == 0);
}

void ensure_grows_only_for_a_larger_request() {
  A::start();
  {
    Grow g;
    CHECK(g.bytes == 0 && g.get() == nullptr);
    CHECK(g.ensure(0) == 0 && A::allocs == 0);
    CHECK(g.ensure(100) == 0 && g.bytes == 100 && A::allocs == 1);
    void* const p = g.get();
    CHECK(g.ensure(100) == 0 && g.ensure(40) == 0 && g.ensure(0) == 0);  // equal or smaller: the same allocation
    CHECK(g.get() == p && g.bytes == 100 && A::allocs == 1 && A::frees == 0);
    CHECK(g.ensure(101) == 0 && g.bytes == 101);  // larger: freed exactly once, allocated once
    CHECK(A::allocs == 2 && A::frees == 1);
    std::memset(g.get(), 1, 101);
    g.reset();
    CHECK(g.bytes == 0 && g.get() == nullptr && A::frees == 2);
    CHECK(g.ensure(10) == 0 && g.bytes == 10 && A::allocs == 3);  // usable again after a reset (qk_ctx_trim)
    Grow h(std::move(g));
    CHECK(g.bytes == 0 && g.get() == nullptr && h.bytes == 10);
  }
  CHECK(A::live() == 0);
}

void a_failed_ensure_leaves_the_buffer_empty() {
  A::start(2);
  {
    Grow g;
    CHECK(g.ensure(50) == 0 && g.bytes == 50);
    CHECK(g.ensure(500) != 0);  // the old allocation is gone, the new one was refused
    CHECK(g.bytes == 0 && g.get() == nullptr && A::frees == 1);
    CHECK(g.ensure(20) == 0 && g.bytes == 20);  // and a later request starts from nothing
    Buf b;
    A::start(1);
    CHECK(b.alloc(8) != 0 && !b);
    A::start();
  }
  // (the counters were restarted inside the scope: the sanitizer's leak check covers this case)
}

// a call in the engine's style: a kept buffer, four temporaries, one of them handed on to a longer-lived owner on success --
// with an early return at the first failure, as HIP_TRY does
int a_call(Grow& kept, Buf& published) {
  if (kept.ensure(1000) != 0) return 1;
  Buf a, b, c, d;
  if (a.alloc(10) != 0) return 1;
  if (b.alloc(20) != 0) return 1;
  if (kept.ensure(2000) != 0) return 1;
  if (c.alloc(30) != 0) return 1;
  if (d.alloc(40) != 0) return 1;
  published = std::move(c);
  return 0;
}

void failing_the_nth_allocation_leaks_nothing() {
  const int n_allocs = 6;
  for (int n = 0; n <= n_allocs + 1; ++n) {  // 0 and n_allocs + 1: no failure
    A::start(n);
    int rc;
    {
      Grow kept;
      Buf published;
      rc = a_call(kept, published);
      CHECK((rc != 0) == (n >= 1 && n <= n_allocs));
      CHECK(rc != 0 || (published && kept.bytes == 2000));
      CHECK(rc == 0 || !published);
      CHECK(A::live() == (rc == 0 ? 2 : (kept.bytes ? 1 : 0)));  // the temporaries are gone whichever return was taken
    }
    CHECK(A::live() == 0);
    std::printf("ok   fail allocation %d of %d: rc %d, %d allocations, %d frees\n", n, n_allocs, rc, A::allocs, A::frees);
  }
}

}  // namespace

int main() {
  move_leaves_the_source_empty();
  std::printf("ok   move\n");
  release_passes_ownership();
  std::printf("ok   release\n");
  ensure_grows_only_for_a_larger_request();
  std::printf("ok   ensure\n");
  a_failed_ensure_leaves_the_buffer_empty();
  std::printf("ok   failed ensure\n");
  failing_the_nth_allocation_leaks_nothing();
  std::printf("%s\n", failures ? "FAILED" : "devmem: all cases passed");
  return failures ? 1 : 0;
}
