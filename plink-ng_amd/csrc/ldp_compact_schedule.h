// ldp_compact_schedule.h -- the batch schedule of the in-place row compaction behind ldp_restrict_variants() (ldp_compact.hip has the
// kernel, ldp_engine_restrict.cpp the caller).  Plain C++, no device code: tests/sanitize/compact_schedule_check.cpp runs it on the CPU.
//
// Kept row k of the new image comes from row src[k] of the old one; src is strictly increasing, so src[k] >= k, and the image is
// compacted where it lies.  The kept rows are taken in ascending batches of at most batch_rows rows, one after the other in stream
// order.  Writing the destination rows [k0, k1) of a batch destroys old rows below k1 only, and every later batch reads rows
// src[k] >= k >= k1: nothing is read after its slot was overwritten, whatever the batch length.  Within a batch the rows move in
// parallel, so a batch is copied DIRECTLY only when its destination range ends at or before its first source row (k1 <= src[k0]:
// once a batch's worth of rows has been dropped in front of it that always holds); otherwise it goes through the bounce buffer --
// every source row out, then every row in.  The prefix of rows that stay where they are (src[k] == k) is not touched.
#ifndef LDP_COMPACT_SCHEDULE_H
#define LDP_COMPACT_SCHEDULE_H
#include <cstdint>
#include <vector>

namespace ldp {

struct CompactBatch {
  uint32_t k0, k1;  // destination rows [k0, k1); their sources are src[k0 .. k1)
  bool bounce;      // through the bounce buffer (k1 - k0 rows of it)
};

inline void compact_schedule(const uint32_t* src, uint32_t n, uint32_t batch_rows, std::vector<CompactBatch>* out) {
  out->clear();
  if (!batch_rows) {
    batch_rows = 1;
  }
  uint32_t k = 0;
  while ((k < n) && (src[k] == k)) {
    ++k;
  }
  while (k < n) {
    CompactBatch b;
    b.k0 = k;
    b.k1 = (n - k > batch_rows) ? (k + batch_rows) : n;
    b.bounce = b.k1 > src[k];
    out->push_back(b);
    k = b.k1;
  }
}

}  // namespace ldp
#endif
