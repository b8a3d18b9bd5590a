// devbuf_host.cpp - the library's owning buffer (csrc/devbuf.h, verbatim) on the host: a counting stand-in for the device allocator that can
// be told to fail its k-th allocation, and the rules every grow site of the library relies on.  A program of its own, meant to be built
// with the address and undefined-behaviour sanitizers (tests/test_devbuf_host.py): a double free or a leak ends it.
#include <stdio.h>
#include <stdlib.h>

#include <utility>

#include "../devbuf.h"

struct fake_mem {
  typedef int error;
  static constexpr int ok = 0;
  static long allocs, frees, fail_at;  // fail_at: the allocation (counted from 1, failures included) that fails; 0 = none
  static long calls;
  static int alloc(void** p, size_t bytes) {
    if (++calls == fail_at) return 2;
    ++allocs;
    *p = malloc(bytes ? bytes : 1);
    return *p ? 0 : 2;
  }
  static void free(void* p) { ++frees, ::free(p); }
};
long fake_mem::allocs = 0, fake_mem::frees = 0, fake_mem::fail_at = 0, fake_mem::calls = 0;
typedef growbuf<unsigned, fake_mem> buf;

static int failed = 0;
#define CHECK(cond)                                                       \
  do {                                                                    \
    if (!(cond)) printf("line %d: %s\n", __LINE__, #cond), failed = 1;    \
  } while (0)

// a group as the library grows one (mul_setup: staging and parking space of a piece): every member to `want`, stopping at the first failure
static int grow_group(buf (&g)[4], size_t want) {
  for (buf& b : g)
    if (int e = b.grow(want)) return e;
  return 0;
}

int main() {
  long a0, f0;
  {
    // grow: smaller or equal keeps the pointer (and what it points to); larger frees once and allocates once
    buf b;
    CHECK(b.p == nullptr && b.n == 0);
    CHECK(b.grow(0) == 0 && b.p == nullptr && fake_mem::allocs == 0);
    CHECK(b.grow(100) == 0 && b.p && b.n == 100 && fake_mem::allocs == 1 && fake_mem::frees == 0);
    for (unsigned i = 0; i < 100; ++i) b.p[i] = i;  // (all 100 elements are there: the sanitizer watches the bounds)
    unsigned* const first = b.p;
    CHECK(b.grow(100) == 0 && b.p == first && b.n == 100);
    CHECK(b.grow(7) == 0 && b.p == first && b.n == 100 && b.p[99] == 99);
    CHECK(fake_mem::allocs == 1 && fake_mem::frees == 0);
    CHECK(b.grow(101) == 0 && b.n == 101 && fake_mem::allocs == 2 && fake_mem::frees == 1);
    b.p[100] = 1;
    // a failed grow leaves the buffer empty - the old buffer freed, nothing held - and a later grow succeeds
    a0 = fake_mem::allocs, f0 = fake_mem::frees;
    fake_mem::fail_at = fake_mem::calls + 1;
    CHECK(b.grow(500) != 0 && b.p == nullptr && b.n == 0 && fake_mem::allocs == a0 && fake_mem::frees == f0 + 1);
    CHECK(b.grow(50) == 0 && b.p && b.n == 50 && fake_mem::allocs == a0 + 1 && fake_mem::frees == f0 + 1);
    // reset: freed once, empty, and harmless on an empty buffer
    b.reset();
    CHECK(b.p == nullptr && b.n == 0 && fake_mem::frees == f0 + 2);
    b.reset();
    CHECK(fake_mem::frees == f0 + 2);
  }
  CHECK(fake_mem::allocs == fake_mem::frees);  // (the empty buffer's destructor freed nothing)
  {
    // move and swap hand the buffer on: one owner at any time, one free in the end
    a0 = fake_mem::allocs, f0 = fake_mem::frees;
    buf a, b;
    CHECK(a.grow(10) == 0 && b.grow(20) == 0);
    unsigned *const pa = a.p, *const pb = b.p;
    a.swap(b);
    CHECK(a.p == pb && a.n == 20 && b.p == pa && b.n == 10 && fake_mem::frees == f0);
    buf c(std::move(a));
    CHECK(c.p == pb && c.n == 20 && a.p == nullptr && a.n == 0 && fake_mem::frees == f0);
    b = std::move(c);  // b's own buffer is freed, c's moves in
    CHECK(b.p == pb && b.n == 20 && c.p == nullptr && c.n == 0 && fake_mem::frees == f0 + 1);
    buf& same = b;
    b = std::move(same);  // onto itself: nothing happens
    CHECK(b.p == pb && b.n == 20 && fake_mem::frees == f0 + 1);
    buf empty;
    empty.swap(b);  // the self-test's pattern: the context's buffer waits in a local ...
    CHECK(b.p == nullptr && b.n == 0 && empty.p == pb);
    CHECK(b.grow(5) == 0);
    empty.swap(b);  // ... and comes back; the local frees what the context held meanwhile
    CHECK(b.p == pb && b.n == 20 && empty.n == 5);
  }
  CHECK(fake_mem::allocs == a0 + 3 && fake_mem::frees == f0 + 3);
  {
    // release: the buffer leaves, nothing is left to free
    a0 = fake_mem::allocs, f0 = fake_mem::frees;
    unsigned* raw;
    {
      buf b;
      CHECK(b.grow(8) == 0);
      raw = b.release();
      CHECK(raw && b.p == nullptr && b.n == 0);
    }
    CHECK(fake_mem::allocs == a0 + 1 && fake_mem::frees == f0);
    fake_mem::free(raw);
  }
  {
    // a group of four whose third allocation fails: its capacity is the smallest member's, and the next grow completes it with exactly
    // the two allocations that are missing
    buf g[4];
    CHECK(grow_group(g, 16) == 0 && held_by_all(g) == 16);
    a0 = fake_mem::allocs, f0 = fake_mem::frees;
    fake_mem::fail_at = fake_mem::calls + 3;
    CHECK(grow_group(g, 64) != 0);
    CHECK(g[0].n == 64 && g[1].n == 64 && g[2].n == 0 && g[2].p == nullptr && g[3].n == 16);
    CHECK(held_by_all(g) == 0 && fake_mem::allocs == a0 + 2 && fake_mem::frees == f0 + 3);
    a0 = fake_mem::allocs, f0 = fake_mem::frees;
    CHECK(grow_group(g, 64) == 0 && held_by_all(g) == 64);
    CHECK(fake_mem::allocs == a0 + 2 && fake_mem::frees == f0 + 1);
    CHECK(grow_group(g, 64) == 0 && grow_group(g, 3) == 0 && fake_mem::allocs == a0 + 2);  // enough already: no allocation
  }
  CHECK(fake_mem::allocs == fake_mem::frees);
  if (failed) return 1;
  printf("devbuf_host: ok (%ld allocations, %ld frees)\n", fake_mem::allocs, fake_mem::frees);
  return 0;
}
