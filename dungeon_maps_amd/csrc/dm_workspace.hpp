// The caller's workspace, cut into regions: one bump allocator over a byte range (host only).
//
// Every layout of the library is ONE function that takes an Arena and the dimensions and returns
// a struct of pointers.  Run on a measuring arena (no base, no limit) it gives the size the
// *_workspace_bytes functions promise -- used() --, run on the caller's block it gives the
// pointers, so a layout term is written once and the two cannot drift apart.
//
// Every region starts on a kAlign boundary of the range (its START is rounded, not its end: a
// layout's last region ends where its bytes end).  Offsets count from the base; whether the base
// itself is aligned is a separate question -- aligned() -- that each route answers in its own way.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace dm {

class Arena {
 public:
  static constexpr size_t kAlign = 256;
  static constexpr size_t kNoLimit = ~(size_t)0 / kAlign * kAlign;
  static constexpr size_t round_up(size_t v) { return (v + kAlign - 1) / kAlign * kAlign; }

  Arena() : Arena(nullptr, kNoLimit) {}          // measuring: null pointers, used() is the size
  Arena(void* base, size_t bytes)
      : base_(static_cast<unsigned char*>(base)), bytes_(bytes), head_(0), tail_(bytes), ok_(true) {}

  bool aligned() const { return reinterpret_cast<uintptr_t>(base_) % kAlign == 0; }

  // The next `count` objects of T.  NULL when measuring; NULL, and ok() false from then on, when
  // they do not fit.  take<T>(0) is where the next region would start (the rounded cursor).
  template <class T>
  T* take(size_t count) {
    const size_t at = round_up(head_), n = count * sizeof(T);
    if (at > tail_ || n > tail_ - at) return overflow<T>();
    head_ = at + n;
    return at_offset<T>(at);
  }
  // The same from the end of the range.
  template <class T>
  T* take_tail(size_t count) {
    const size_t n = count * sizeof(T);
    if (n > tail_ || (tail_ - n) / kAlign * kAlign < head_) return overflow<T>();
    tail_ = (tail_ - n) / kAlign * kAlign;
    return at_offset<T>(tail_);
  }
  // Bytes between the rounded cursor and the tail: what a region that gets "whatever is left" has.
  size_t rest() const { return ok_ && tail_ > round_up(head_) ? tail_ - round_up(head_) : 0; }
  size_t used() const { return head_ + (bytes_ - tail_); }
  bool ok() const { return ok_; }

 private:
  template <class T>
  T* at_offset(size_t at) const { return base_ ? reinterpret_cast<T*>(base_ + at) : nullptr; }
  template <class T>
  T* overflow() { ok_ = false; return nullptr; }

  unsigned char* base_;
  size_t bytes_, head_, tail_;
  bool ok_;
};

}  // namespace dm
