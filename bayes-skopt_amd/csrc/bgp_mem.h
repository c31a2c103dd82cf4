// Who owns libbgp's device and pinned host memory (host code only): grow-only owning buffers and ONE two-pass typed carver.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/bgp.h"

void bgp_set_error(const char* fmt, ...);
void bgp_xfer_drop_pending();

// An owned, grow-only allocation of T: device memory (BgpDev) or pinned host memory (BgpPinned).  It reads as the plain pointer
// it replaces; whoever holds it frees it (release(), or the destructor of the struct it is a member of).
template <class T, bool PINNED>
struct BgpBuf {
  T* p = nullptr;
  size_t cap = 0;  // elements
  BgpBuf() = default;
  BgpBuf(const BgpBuf&) = delete;
  BgpBuf& operator=(const BgpBuf&) = delete;
  ~BgpBuf() { release(); }
  operator T*() const { return p; }
  void release() {
    if (p) (void)(PINNED ? hipHostFree(p) : hipFree(p));
    p = nullptr;
    cap = 0;
  }
  // At least `count` elements: re-allocated (contents lost) only when count > cap, then with exactly `count` elements unless the
  // caller asks for more head room with `alloc`.  A failure leaves the buffer empty, is reported like one of BGP_HIP and, like
  // there, clears the sticky HIP error and drops the pending downloads of the call.
  int ensure(size_t count, size_t alloc = 0) {
    if (count <= cap) return BGP_OK;
    release();
    if (alloc < count) alloc = count;
    const hipError_t e = PINNED ? hipHostMalloc((void**)&p, alloc * sizeof(T), hipHostMallocDefault) : hipMalloc((void**)&p, alloc * sizeof(T));
    if (e != hipSuccess) {
      p = nullptr;
      bgp_set_error("%s of %zu bytes failed: %s", PINNED ? "hipHostMalloc" : "hipMalloc", alloc * sizeof(T), hipGetErrorString(e));
      (void)hipGetLastError();
      bgp_xfer_drop_pending();
      return BGP_ERR_HIP;
    }
    cap = alloc;
    return BGP_OK;
  }
};
template <class T>
using BgpDev = BgpBuf<T, false>;
template <class T>
using BgpPinned = BgpBuf<T, true>;

// The layout of one allocation, written ONCE as a function of take<T>(count) calls.  bgp_carve runs it twice: without a base, to
// size the block, and -- the backing buffer grown to that size -- again to hand out the pointers, so that a layout cannot disagree
// with its size.  Every region starts on a multiple of `align` bytes.
struct BgpCarve {
  char* base = nullptr;
  size_t align, off = 0;
  template <class T>
  T* take(size_t count) {
    T* q = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += (count * sizeof(T) + align - 1) / align * align;
    return q;
  }
};
template <class Layout>
static inline int bgp_carve(BgpDev<char>& buf, size_t align, Layout&& layout) {
  BgpCarve k{nullptr, align};
  layout(k);
  const int rc = buf.ensure(k.off);
  if (rc) return rc;
  k.base = buf;
  k.off = 0;
  layout(k);
  return BGP_OK;
}
