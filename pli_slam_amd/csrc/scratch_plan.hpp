// The device scratch of one call, carved from a declared plan: every block is declared once, with its element type and count,
// and the total, the block's pointer, the copy that fills an input and the length of a read-back all come from that declaration.
//
//   ScratchPlan plan;
//   auto dq  = plan.in(hostDesc, (size_t)nq * 32);       (an input: the block and its copy from the host, one declaration)
//   auto occ = plan.inOpt(hostOcc, n);                    (an optional input: nullptr for the kernel when it was not passed)
//   auto cnt = plan.add<int>(1);
//   ... commitScratch(c, plan): allocates plan.bytes(), plan.bind(base), issues plan.copies() ...       (capi_host.hpp)
//   kernel(dq, occ, cnt)                                  (a block converts to its pointer)
//   auto best = plan.addIf<int>(hostBest != nullptr, n);  (an optional output)
//   download(c, hostCnt, cnt)                             (a block knows its count)
//
// The plan only records the copies, {offset, source, bytes} in the order of declaration; whoever binds it carries them out, so a
// source must live until those copies have completed.  Not an allocator: nothing is freed and plans do not nest.  Plain C++ (no HIP, no context), so that a
// host compiler can test it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace pli {

constexpr size_t SCRATCH_ALIGN = 256;     // the kernels read descriptors as wide words

class ScratchPlan;

template <typename T>
struct ScratchBlock {
  const ScratchPlan* plan;
  size_t off;                             // bytes from the plan's base
  size_t n;                               // elements, as declared
  bool present = true;                    // false: an optional block that was not asked for (addIf, inOpt), its pointer is null
  inline operator T*() const;             // valid once the plan is bound
};

struct ScratchCopy { size_t off; const void* src; size_t bytes; };      // host -> base + off

class ScratchPlan {
 public:
  // n elements of T on a SCRATCH_ALIGN boundary; a count of 0 still takes a block, so that its pointer is valid and its own
  template <typename T>
  ScratchBlock<T> add(size_t n) {
    const ScratchBlock<T> b{this, total_, n};
    const size_t bytes = (n ? n : 1) * sizeof(T);
    total_ += (bytes + SCRATCH_ALIGN - 1) / SCRATCH_ALIGN * SCRATCH_ALIGN;
    return b;
  }
  // an optional block, for a table that the caller may leave out: add(n) when wanted, else an empty block that converts to nullptr
  template <typename T>
  ScratchBlock<T> addIf(bool wanted, size_t n) {
    ScratchBlock<T> b = add<T>(wanted ? n : 0);
    b.present = wanted;
    return b;
  }
  // an input: add(n), filled from src's n elements when there is a source and n > 0 (a null src: a plain block)
  template <typename T>
  ScratchBlock<T> in(const T* src, size_t n) {
    const ScratchBlock<T> b = add<T>(n);
    if (src && n) copies_.push_back({b.off, src, n * sizeof(T)});
    return b;
  }
  // an optional input: in(src, n) when there is a source and n > 0, else absent like addIf(false, n)
  template <typename T>
  ScratchBlock<T> inOpt(const T* src, size_t n) {
    return src && n ? in(src, n) : addIf<T>(false, 0);
  }
  size_t bytes() const { return total_; }
  const std::vector<ScratchCopy>& copies() const { return copies_; }
  void bind(void* base) { base_ = static_cast<uint8_t*>(base); }     // base: bytes() bytes, SCRATCH_ALIGN aligned
  uint8_t* base() const { return base_; }

 private:
  size_t total_ = 0;
  uint8_t* base_ = nullptr;
  std::vector<ScratchCopy> copies_;
};

template <typename T>
inline ScratchBlock<T>::operator T*() const { return present ? reinterpret_cast<T*>(plan->base() + off) : nullptr; }

}  // namespace pli
