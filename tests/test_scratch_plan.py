"""pli_slam_amd/csrc/scratch_plan.hpp, the plan from which the matcher entry points carve their device scratch, is plain C++: it is
compiled here with g++ (no HIP, no GPU) under AddressSanitizer and UBSan, bound to a host buffer of exactly plan.bytes() bytes, and every
block is written through its own pointer for its declared length.  The copies that a plan records for its inputs (in / inOpt) are
carried out with memcpy from sources of exactly the declared length, so the sanitizer guards both ends of every copy."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include "pli_slam_amd/csrc/scratch_plan.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
using pli::ScratchPlan;

struct Kp { float v[5]; int a, b; };                      // 28 bytes, as pli_keypoint: not a power of two
struct Seen { size_t off, bytes; };

static int fails = 0;
#define CHECK(x) do { if (!(x)) { std::printf("line %d: %s\n", __LINE__, #x); ++fails; } } while (0)

// declares a block, notes where it lies and how many bytes its declaration asked for
template <typename T>
pli::ScratchBlock<T> add(ScratchPlan& plan, std::vector<Seen>& seen, size_t n) {
  const size_t before = plan.bytes();
  auto b = plan.add<T>(n);
  CHECK(b.off == before);                                 // blocks follow each other in the order of declaration
  CHECK(plan.bytes() - before <= (n ? n : 1) * sizeof(T) + 255);     // padding only: less than one alignment unit per block
  seen.push_back({b.off, n * sizeof(T)});
  return b;
}

static void verify(ScratchPlan& plan, const std::vector<Seen>& seen) {
  for (size_t i = 0; i < seen.size(); ++i) {
    CHECK(seen[i].off % 256 == 0);
    CHECK(seen[i].off + seen[i].bytes <= plan.bytes());
    for (size_t j = 0; j < i; ++j) {
      CHECK(seen[i].off != seen[j].off);                  // zero counts included: every block has an offset of its own
      CHECK(seen[j].off + seen[j].bytes <= seen[i].off);
    }
  }
  CHECK(plan.bytes() % 256 == 0);
  // the base as hipMalloc gives it: aligned, and exactly bytes() long (AddressSanitizer guards the end)
  uint8_t* base = static_cast<uint8_t*>(std::aligned_alloc(256, plan.bytes()));
  plan.bind(base);
  for (const Seen& s : seen) std::memset(base + s.off, 0xAB, s.bytes ? s.bytes : 1);
  std::free(base);
}

int main() {
  {   // a one-byte block before an eight-byte-typed one, zero counts in the middle and at the end
    ScratchPlan plan; std::vector<Seen> seen;
    auto flag = add<uint8_t>(plan, seen, 1);
    auto keys = add<unsigned long long>(plan, seen, 3 * 64);
    auto none = add<int>(plan, seen, 0);
    auto none2 = add<double>(plan, seen, 0);
    auto kp = add<Kp>(plan, seen, 1201);
    auto cnt = add<int>(plan, seen, 1);
    auto last = add<uint16_t>(plan, seen, 0);
    verify(plan, seen);
    uint8_t* base = static_cast<uint8_t*>(std::aligned_alloc(256, plan.bytes()));
    plan.bind(base);
    unsigned long long* k = keys; Kp* p = kp; int* c = cnt; int* z = none; double* z2 = none2; uint16_t* l = last; uint8_t* f = flag;
    CHECK(f == base && (uint8_t*)k == base + 256 && (uint8_t*)z == base + 256 + 1536 && (uint8_t*)z2 == (uint8_t*)z + 256);
    CHECK((uintptr_t)k % 8 == 0 && (uintptr_t)p % 256 == 0 && (uint8_t*)z2 != (uint8_t*)z && (uint8_t*)l > (uint8_t*)c);
    k[3 * 64 - 1] = 1; p[1200].b = 2; *c = 3; *z = 4; *z2 = 5; *l = 6; *f = 7;     // first and last elements, and the empty blocks' own one
    CHECK((uint8_t*)(l + 1) <= base + plan.bytes());
    std::free(base);
  }
  {   // an empty plan, and one whose blocks are all empty
    ScratchPlan plan; std::vector<Seen> seen;
    CHECK(plan.bytes() == 0);
    for (int i = 0; i < 5; ++i) add<float>(plan, seen, 0);
    CHECK(plan.bytes() == 5 * 256);
    verify(plan, seen);
  }
  {   // counts around the alignment unit, for element sizes 1, 2, 4, 8 and 28
    for (size_t n : {1, 7, 255, 256, 257, 511, 512, 513, 15360}) {
      ScratchPlan plan; std::vector<Seen> seen;
      add<uint8_t>(plan, seen, n); add<uint8_t>(plan, seen, n * 32); add<uint16_t>(plan, seen, n); add<int>(plan, seen, n);
      add<int>(plan, seen, 2 * n); add<double>(plan, seen, n); add<Kp>(plan, seen, n); add<int>(plan, seen, 1);
      verify(plan, seen);
    }
  }
  {   // optional blocks: one that is wanted is a block like any other, one that is not keeps an offset of its own and gives nullptr
    ScratchPlan plan;
    auto a = plan.add<int>(3);
    auto skipped = plan.addIf<uint8_t>(false, 1000);
    auto wanted = plan.addIf<uint8_t>(true, 1000);
    auto z = plan.add<int>(1);
    CHECK(skipped.off == 256 && wanted.off == 512 && z.off == 512 + 1024 && plan.bytes() == 512 + 1024 + 256);
    uint8_t* base = static_cast<uint8_t*>(std::aligned_alloc(256, plan.bytes()));
    plan.bind(base);
    uint8_t* s = skipped; uint8_t* w = wanted; const uint8_t* cs = skipped; int* pa = a; int* pz = z;
    CHECK(s == nullptr && cs == nullptr && w == base + 512 && (uint8_t*)pa == base && (uint8_t*)pz == base + 512 + 1024);
    w[999] = 1; *pz = 2;
    std::free(base);
  }
  {   // inputs declared with their host source: the recorded copies, carried out with memcpy from sources of exactly the declared length
    static int dummy = 0;
    for (size_t n : {0, 1, 255, 256, 257, 15360}) {
      ScratchPlan plan;
      std::vector<uint8_t> s1(n, 0x11); std::vector<uint16_t> s2(n, 0x2222); std::vector<int> s4(n, 0x44444444);
      std::vector<double> s8(n, 8.0); std::vector<Kp> s28(n, Kp{{1, 2, 3, 4, 5}, 6, 7});
      auto a = plan.in(s1.data(), n);
      auto out = plan.add<int>(n);                         // a block without a source between the inputs
      auto b = plan.in(s2.data(), n);
      auto c = plan.inOpt(s4.data(), n);
      auto plain = plan.in<double>(nullptr, n);            // a null source: a plain block
      auto d = plan.in(s8.data(), n);
      auto absent = plan.inOpt<Kp>(nullptr, n);
      auto e = plan.inOpt(s28.data(), n);
      auto zero = plan.in(&dummy, 0);                      // a source, but nothing to copy
      CHECK(a.n == n && out.n == n && b.n == n && plain.n == n && d.n == n && zero.n == 0);       // a block reports its declared count
      CHECK(c.n == (c.present ? n : 0) && e.n == (e.present ? n : 0) && absent.n == 0);
      CHECK(c.present == (n > 0) && e.present == (n > 0) && !absent.present && a.present && plain.present && zero.present);
      // the list: the blocks with a source and n > 0, in the order of declaration, each for its block's declared bytes at its block
      const struct { size_t off, bytes; const void* src; } want[5] = {{a.off, a.n * 1, s1.data()}, {b.off, b.n * 2, s2.data()},
          {c.off, c.n * 4, s4.data()}, {d.off, d.n * 8, s8.data()}, {e.off, e.n * 28, s28.data()}};
      const auto& copies = plan.copies();
      CHECK(copies.size() == (n ? 5u : 0u));                // a null source or n == 0 records nothing
      for (size_t i = 0; i < copies.size() && i < 5; ++i) {
        CHECK(copies[i].src == want[i].src && copies[i].bytes == want[i].bytes);
        CHECK(copies[i].off >= want[i].off && copies[i].off + copies[i].bytes <= want[i].off + want[i].bytes);
        CHECK(i == 0 || copies[i].off >= copies[i - 1].off + copies[i - 1].bytes);
      }
      uint8_t* base = static_cast<uint8_t*>(std::aligned_alloc(256, plan.bytes()));       // exactly bytes(): ASan guards both ends
      plan.bind(base);
      for (const auto& k : copies) std::memcpy(plan.base() + k.off, k.src, k.bytes);
      uint8_t* pa = a; uint16_t* pb = b; int* pc = c; double* pp = plain; double* pd = d; Kp* pe = e; Kp* pn = absent; int* pz = zero;
      const Kp* cpn = absent;
      CHECK(pa && pb && pp && pd && pz && (int*)out != nullptr);                      // in: the pointer is always valid
      CHECK(pn == nullptr && cpn == nullptr && (pc != nullptr) == (n > 0) && (pe != nullptr) == (n > 0));
      if (n) {
        CHECK(!std::memcmp(pa, s1.data(), n) && !std::memcmp(pb, s2.data(), n * 2) && !std::memcmp(pc, s4.data(), n * 4));
        CHECK(!std::memcmp(pd, s8.data(), n * 8) && !std::memcmp(pe, s28.data(), n * 28));
        CHECK(pe[n - 1].b == 7 && (uint8_t*)(pe + n) <= base + plan.bytes());
      }
      std::free(base);
    }
  }
  if (!fails) std::printf("scratch plan: ok\n");
  return fails ? 1 : 0;
}
'''


def test_scratch_plan_offsets_under_sanitizers(tmp_path):
    src = tmp_path / "plan.cpp"
    src.write_text(SRC)
    exe = str(tmp_path / "plan")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-fno-omit-frame-pointer", "-I", ROOT, str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1 exitcode=66"))
    assert r.returncode == 0 and "scratch plan: ok" in r.stdout and "Sanitizer" not in r.stderr, r.stdout + r.stderr[-3000:]
