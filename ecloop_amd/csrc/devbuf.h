// devbuf.h - the one owning, growable buffer of the library: every device and page-locked buffer of a context, the shared window tables and
// the scope-local buffers of single calls.  Where the memory comes from is the policy Mem (ecloop_hip.hip has the two: device, pinned):
//   typedef ... error;  static const error ok;  static error alloc(void** p, size_t bytes);  static void free(void* p);
// so this header needs no HIP header and compiles for the host with a counting stand-in (tools/devbuf_host.cpp).
#pragma once
#include <stddef.h>

template <typename T, class Mem>
struct growbuf {
  T* p = nullptr;
  size_t n = 0;  // elements held

  growbuf() = default;
  growbuf(const growbuf&) = delete;
  growbuf& operator=(const growbuf&) = delete;
  growbuf(growbuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr, o.n = 0; }
  growbuf& operator=(growbuf&& o) noexcept {
    if (this != &o) reset(), swap(o);
    return *this;
  }
  ~growbuf() { reset(); }

  void swap(growbuf& o) noexcept {
    T* const op = o.p;
    const size_t on = o.n;
    o.p = p, o.n = n, p = op, n = on;
  }
  void reset() {
    if (p) Mem::free(p);
    p = nullptr, n = 0;
  }
  // the buffer leaves without being freed: the caller owns it now
  T* release() {
    T* const r = p;
    p = nullptr, n = 0;
    return r;
  }
  // room for `want` elements.  Enough already: nothing happens, the contents stay.  Otherwise the old buffer is freed first (contents are
  // never carried over) and a failed allocation leaves the buffer empty, so that the next call starts from a known state.
  typename Mem::error grow(size_t want) {
    if (want <= n) return Mem::ok;
    reset();
    void* q = nullptr;
    const typename Mem::error e = Mem::alloc(&q, want * sizeof(T));
    if (e != Mem::ok) return e;
    p = (T*)q, n = want;
    return Mem::ok;
  }
};

// Buffers that grow together (one per staging slot, one per compute stream) have the capacity of their smallest member: a call that
// failed between two allocations of the group reports what all members hold, and the next call's grow completes the group.
template <typename T, class Mem, size_t K>
static inline size_t held_by_all(const growbuf<T, Mem> (&g)[K]) {
  size_t m = g[0].n;
  for (size_t i = 1; i < K; ++i) m = g[i].n < m ? g[i].n : m;
  return m;
}
