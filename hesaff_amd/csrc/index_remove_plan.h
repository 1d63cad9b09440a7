// index_remove_plan.h -- the host arithmetic of a removal from the image index (hesaff_index_remove, include/hesaff_amd.h), beside
// index_plan.h: which calls are refused, the gone-flags of a call's image numbers, the renumbering of the images that stay, where the
// scratch of a removal lies, and the bytes a removal holds at its peak.  Pure functions and plain structs, no HIP: capi_index_remove.h
// obtains its numbers here, and tests/native/index_remove_plan_check.cpp checks them on the CPU (tests/test_index_remove_host.py).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "embed_plan.h"   // KeyListArrays
#include "index_plan.h"

namespace hesaff_plan {

// m of n_old images go, 1 <= m <= n_old - 1: an index always holds at least one image (emptying it is hesaff_index_clear)
inline bool index_remove_ok(int64_t n_old, int64_t m) { return n_old >= 1 && n_old <= HS_INDEX_MAX_IMAGES && m >= 1 && m < n_old; }

// what index_remove_flags found wrong with a call's numbers
enum IndexRemoveFault { HS_REMOVE_FINE = 0, HS_REMOVE_OUTSIDE = 1, HS_REMOVE_TWICE = 2 };

// images[m], in any order -> gone[n]: 1 for an image that goes, 0 for one that stays.  The first number outside 0 .. n - 1 or given a
// second time ends the walk: its fault is returned and *offender is that number (gone is then half made and not to be used)
inline IndexRemoveFault index_remove_flags(const int32_t *images, int64_t m, int64_t n, std::vector<uint32_t> &gone, int64_t *offender)
{
   gone.assign((size_t)n, 0u);
   for (int64_t j = 0; j < m; j++) {
      const int64_t i = images[j];
      if (i < 0 || i >= n) { *offender = i; return HS_REMOVE_OUTSIDE; }
      if (gone[(size_t)i]) { *offender = i; return HS_REMOVE_TWICE; }
      gone[(size_t)i] = 1u;
   }
   return HS_REMOVE_FINE;
}

// remap[n]: old image i becomes i - #{removed numbers below i}; -1 for a removed one.  -> the images that stay
inline int64_t index_remove_remap(const uint32_t *gone, int64_t n, int32_t *remap)
{
   int32_t next = 0;
   for (int64_t i = 0; i < n; i++) remap[i] = gone[i] ? -1 : next++;
   return next;
}

// ---- the scratch of a removal, released before the call returns: O(N + K) words, no hash table ----
struct IndexRemoveArrays {
   Span<uint32_t> gone;                  // [n_old]: the call's flags
   Span<uint32_t> remap;                 // [n_old]: the scan of the keep-flags; HS_REMOVE_GONE for a removed image
   Span<uint32_t> cursor;                // [k]: the slots drawn so far from each new posting list
   Span<uint32_t> key_count;             // [k]: embedded: the keys each word keeps (else [1])
   Span<uint32_t> key_offsets;           // [k + 1]: embedded: their scan, copied into the new key lists once those are allocated (else [1])
   Span<uint32_t> key_cursor;            // [k]: embedded: the slots drawn so far from each new key list (else [1])
   Span<uint32_t> block_sums;            // the scans', one per 4096 of max(n_old, k) and one more
   Span<unsigned long long> removed;     // [HS_REMOVE_STRIPES * HS_REMOVE_STRIPE_WORDS]: the keys of the removed images, in partial sums
   Span<uint32_t> kept;                  // [1]: the images that stay (the scan's total)
};
constexpr uint32_t HS_REMOVE_GONE = 0xFFFFFFFFu;   // no image has this number: n <= 2^20
// The removed keys are summed in 64 counters, each on a 128-byte line of its own; a block adds to counter (block % 64) and the host
// adds the 64 up.  One counter took a 64-bit atomic per wavefront on one address: 426 000 of them at 10 000 images removed from
// 100 000, which cost the counting pass 3.4 of its 5.3 ms.
constexpr int HS_REMOVE_STRIPES = 64;
constexpr int HS_REMOVE_STRIPE_WORDS = 16;
inline unsigned long long index_remove_sum(const unsigned long long *stripes)
{
   unsigned long long sum = 0;
   for (int s = 0; s < HS_REMOVE_STRIPES; s++) sum += stripes[(size_t)s * HS_REMOVE_STRIPE_WORDS];
   return sum;
}
inline IndexRemoveArrays index_remove_arrays(StagePlan &p, int64_t n_old, int64_t k, bool embedded)
{
   IndexRemoveArrays r;
   const size_t kk = embedded ? (size_t)k : 0;
   r.gone = p.add<uint32_t>((size_t)n_old);
   r.remap = p.add<uint32_t>((size_t)n_old);
   r.cursor = p.add<uint32_t>((size_t)k);
   r.key_count = p.add<uint32_t>(kk ? kk : 1);
   r.key_offsets = p.add<uint32_t>(kk ? kk + 1 : 1);
   r.key_cursor = p.add<uint32_t>(kk ? kk : 1);
   r.block_sums = p.add<uint32_t>(((size_t)(n_old > k ? n_old : k) + 4095) / 4096 + 1);
   r.removed = p.add<unsigned long long>((size_t)HS_REMOVE_STRIPES * HS_REMOVE_STRIPE_WORDS);
   r.kept = p.add<uint32_t>(1);
   return r;
}
// the bytes a removal holds at its peak beside the old index: the new tables, the new lists (at most the old postings; for an
// embedded index the key lists of at most the old keys as well) and the scratch (n_old = k = 2^20, m = 1, postings_old = keys_old =
// 2^28: plain 2.05 GiB, of which the lists are 2 and the scratch 12 MiB; embedded 5.07 GiB, of which the key lists are 3)
inline size_t index_remove_working_set_bytes(int64_t n_old, int64_t m, int64_t k, int64_t postings_old, int64_t keys_old, bool embedded)
{
   StagePlan a, s, kl;
   index_arrays(a, n_old - m, k);
   index_remove_arrays(s, n_old, k, embedded);
   if (embedded) key_list_arrays(kl, k, keys_old);
   return a.bytes() + s.bytes() + index_lists_bytes(postings_old) + (embedded ? kl.bytes() : 0);
}

} // namespace hesaff_plan
