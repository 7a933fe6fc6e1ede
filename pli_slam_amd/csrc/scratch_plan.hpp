// The device scratch of one call, carved from a declared plan: every block is declared once, with its element type and count,
// and both the total and the block's pointer come from that declaration.
//
//   ScratchPlan plan;
//   auto dq  = plan.add<uint8_t>((size_t)nq * 32);
//   auto cnt = plan.add<int>(1);
//   ... allocate plan.bytes(), plan.bind(base) ...       (pli_capi.hip: commitScratch)
//   kernel(dq, cnt)                                       (a block converts to its pointer)
//   auto skip = plan.addIf<uint8_t>(hostSkip != nullptr, n);   (an optional table: nullptr for the kernel when it was not passed)
//
// Not an allocator: nothing is freed and plans do not nest.  Plain C++ (no HIP, no context), so that a host compiler can test it.
#pragma once
#include <cstddef>
#include <cstdint>

namespace pli {

constexpr size_t SCRATCH_ALIGN = 256;     // the kernels read descriptors as wide words

class ScratchPlan;

template <typename T>
struct ScratchBlock {
  const ScratchPlan* plan;
  size_t off;                             // bytes from the plan's base
  bool present = true;                    // false: an optional block that was not asked for (addIf), its pointer is null
  inline operator T*() const;             // valid once the plan is bound
};

class ScratchPlan {
 public:
  // n elements of T on a SCRATCH_ALIGN boundary; a count of 0 still takes a block, so that its pointer is valid and its own
  template <typename T>
  ScratchBlock<T> add(size_t n) {
    const ScratchBlock<T> b{this, total_};
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
  size_t bytes() const { return total_; }
  void bind(void* base) { base_ = static_cast<uint8_t*>(base); }     // base: bytes() bytes, SCRATCH_ALIGN aligned
  uint8_t* base() const { return base_; }

 private:
  size_t total_ = 0;
  uint8_t* base_ = nullptr;
};

template <typename T>
inline ScratchBlock<T>::operator T*() const { return present ? reinterpret_cast<T*>(plan->base() + off) : nullptr; }

}  // namespace pli
