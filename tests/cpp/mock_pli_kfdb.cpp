// TEST-ONLY: tests/cpp/mock_pli.cpp (the stand-in for libpli_frontend.so on machines without a GPU, included here as it is, so
// this file is linked INSTEAD of it) plus the keyframe database entry points (pli_kfdb_*) in plain host code with the library's
// argument checks and the library's threading contract (a lock per context).  The adapter's host test
// (tests/test_cpp_kfdb.py) replays recorded worlds on it under -fsanitize=address,undefined.  Nothing here is product code.
#include <cmath>
#include "mock_pli.cpp"

struct MockSlot { bool live = false; std::vector<uint32_t> w; std::vector<double> v; };
struct pli_kfdb { pli_ctx* ctx; std::vector<MockSlot> slots; };

extern "C" {
static bool mockAscending(const uint32_t* w, int n) { for (int i = 1; i < n; ++i) if (w[i] <= w[i - 1]) return false; return true; }
pli_status pli_kfdb_create(pli_ctx* c, pli_kfdb** out) { if (!c || !out) return PLI_ERR_INVALID; Lock l(c); *out = new pli_kfdb{c, {}}; return PLI_OK; }
void pli_kfdb_destroy(pli_kfdb* db) { delete db; }
pli_status pli_kfdb_add(pli_ctx* c, pli_kfdb* db, const uint32_t* w, const double* v, int32_t n, int32_t* slot) {
  if (!c || !db || !slot || n < 0 || (n > 0 && (!w || !v))) return PLI_ERR_INVALID;
  Lock l(c);
  if (n > PLI_BOW_MAX_FEATURES) return PLI_ERR_CAPACITY;
  if (!mockAscending(w, n)) return PLI_ERR_INVALID;
  size_t s = 0;
  while (s < db->slots.size() && db->slots[s].live) ++s;           // the smallest free slot
  if (s == db->slots.size()) db->slots.emplace_back();
  db->slots[s].live = true; db->slots[s].w.assign(w, w + n); db->slots[s].v.assign(v, v + n);
  *slot = (int32_t)s;
  return PLI_OK;
}
pli_status pli_kfdb_erase(pli_ctx* c, pli_kfdb* db, int32_t s) {
  if (!c || !db) return PLI_ERR_INVALID;
  Lock l(c);
  if (s < 0 || s >= (int32_t)db->slots.size() || !db->slots[s].live) return PLI_ERR_INVALID;
  db->slots[s] = MockSlot();
  return PLI_OK;
}
pli_status pli_kfdb_clear(pli_ctx* c, pli_kfdb* db) { if (!c || !db) return PLI_ERR_INVALID; Lock l(c); db->slots.clear(); return PLI_OK; }
pli_status pli_kfdb_stats(const pli_kfdb* db, struct pli_kfdb_stats* out) {
  if (!db || !out) return PLI_ERR_INVALID;
  Lock l(db->ctx);
  std::memset(out, 0, sizeof(*out));
  out->slot_high_water = (int32_t)db->slots.size();
  for (const MockSlot& s : db->slots) if (s.live) { out->live_keyframes++; out->live_words += (int64_t)s.w.size(); }
  out->arena_words = out->arena_capacity = out->live_words;
  return PLI_OK;
}
pli_status pli_kfdb_query(pli_ctx* c, pli_kfdb* db, const uint32_t* qw, const double* qv, int32_t nq, int32_t nslots, int32_t* common,
                          int32_t* first, double* score) {
  if (!c || !db || nq < 0 || nslots < 0 || (nq > 0 && (!qw || !qv)) || (nslots > 0 && (!common || !first || !score))) return PLI_ERR_INVALID;
  Lock l(c);
  if (nq > PLI_BOW_MAX_FEATURES) return PLI_ERR_CAPACITY;
  if (!mockAscending(qw, nq) || nslots != (int32_t)db->slots.size()) return PLI_ERR_INVALID;
  for (int32_t s = 0; s < nslots; ++s) {
    const MockSlot& k = db->slots[s];
    double acc = 0;
    common[s] = 0; first[s] = -1;
    size_t i = 0, j = 0;
    while (i < (size_t)nq && j < k.w.size()) {
      if (qw[i] < k.w[j]) ++i;
      else if (qw[i] > k.w[j]) ++j;
      else {
        const double vi = qv[i], wi = k.v[j];
        acc += std::fabs(vi - wi) - std::fabs(vi) - std::fabs(wi);
        if (first[s] < 0) first[s] = (int32_t)i;
        common[s]++; ++i; ++j;
      }
    }
    score[s] = -acc / 2.0;
  }
  return PLI_OK;
}
}  // extern "C"
