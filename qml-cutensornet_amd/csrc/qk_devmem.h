// qk_devmem.h -- the owners of device memory (included by qk_host.h; every host translation unit allocates through these two types):
//   QkDevBuf   one device allocation, freed by its destructor: a call's temporaries (HIP_TRY returns early) and the members of
//              longer-lived objects (a set's images, the context's fixed buffers).  Move-only; release() hands the pointer on.
//   QkGrowBuf  a QkDevBuf and its size, kept between calls and regrown when a request is larger (the context's scratch buffers).
// Plain C++ over a two-function allocator A (A::alloc returns 0 on success, like hipMalloc), so the ownership rules are tested
// on the CPU over malloc (tests/host_san/devmem_main.cpp); QkHipAlloc below is the only place that names hipMalloc / hipFree.
#pragma once
#include <cstddef>
#include <utility>

template <class A>
class QkDevBufT {
  void* p_ = nullptr;

 public:
  QkDevBufT() = default;
  QkDevBufT(QkDevBufT&& o) noexcept : p_(o.release()) {}
  QkDevBufT& operator=(QkDevBufT&& o) noexcept {
    if (this != &o) reset(), p_ = o.release();
    return *this;
  }
  ~QkDevBufT() { reset(); }
  auto alloc(size_t bytes) {  // frees what it held; empty again when the allocation fails
    reset();
    const auto e = A::alloc(&p_, bytes);
    if (e != decltype(e)()) p_ = nullptr;
    return e;
  }
  template <class T = void>
  T* get() const { return static_cast<T*>(p_); }
  explicit operator bool() const { return p_ != nullptr; }
  void* release() { return std::exchange(p_, nullptr); }  // to a longer-lived owner: this one frees nothing afterwards
  void reset() {
    if (p_) A::free(p_);
    p_ = nullptr;
  }
};

template <class A>
struct QkGrowBufT {
  QkDevBufT<A> buf;
  size_t bytes = 0;
  QkGrowBufT() = default;
  QkGrowBufT(QkGrowBufT&& o) noexcept : buf(std::move(o.buf)), bytes(std::exchange(o.bytes, 0)) {}
  // No-op when `want` fits; otherwise the old allocation is freed BEFORE the new one is made (the two never coexist) -- a caller
  // whose stream may still read the old one synchronises first.  Empty with size 0 when the allocation fails.
  auto ensure(size_t want) -> decltype(buf.alloc(want)) {
    if (want <= bytes) return {};
    bytes = 0;
    const auto e = buf.alloc(want);
    if (e == decltype(e)()) bytes = want;
    return e;
  }
  template <class T = void>
  T* get() const { return buf.template get<T>(); }
  void reset() { buf.reset(), bytes = 0; }
};

#ifdef __HIPCC__
struct QkHipAlloc {
  static hipError_t alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
  static void free(void* p) { (void)hipFree(p); }
};
using QkDevBuf = QkDevBufT<QkHipAlloc>;
using QkGrowBuf = QkGrowBufT<QkHipAlloc>;
#endif
