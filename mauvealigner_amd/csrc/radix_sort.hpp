// radix_sort.hpp -- what the seed pass needs of the project's sort (radix_sort.hip) beyond the exported sort_pairs_u32 / _u32_batch /
// _u64 of common.hpp: the tile of the main sort, which seed_extract_all lays the first pass's histograms out by, and sort_pairs itself
// for wide values, a histogram made on the way in and a partial sort.
#pragma once
#include "common.hpp"
#include "small_sort.hpp"      // RS_ITEMS, RS_TILE

// Stable LSD passes over bits [shift_lo, key_bits) of the n pairs in *keys_io / *vals_io, which point at the result on return (the
// alternates after an odd number of passes).  have_hist0: the tile histograms of the first pass are already in ctx->hist.
// timer_id >= 0: all launches are booked under that id (the small canonical-order sort must not dilute the per-kernel figures of
// the main sort).
// iota (needs have_hist0 and at least one pass): no values come in.  *vals_io holds seed_extract_all's strand bitmap instead -- bit x of its
// 64-bit words for the key at index x, whole tiles of RS_TILE keys, zero behind n -- and the first pass makes the value of key x as
// x | bit << (top bit of ValT).  The bitmap is only read by that pass; the buffer takes the second pass's output like any *vals_io.
template <typename KeyT, typename ValT = uint32_t>
int sort_pairs(mauve_ctx *ctx, uint32_t n, int key_bits, KeyT **keys_io, ValT **vals_io, KeyT *keys_alt, ValT *vals_alt, bool have_hist0,
               int timer_id = -1, int shift_lo = 0, bool iota = false);
// the four instantiations, compiled in radix_sort.hip only
#define RS_SORT_PAIRS(KeyT, ValT) template int sort_pairs<KeyT, ValT>(mauve_ctx *, uint32_t, int, KeyT **, ValT **, KeyT *, ValT *, bool, int, int, bool)
extern RS_SORT_PAIRS(uint32_t, uint32_t);
extern RS_SORT_PAIRS(uint32_t, uint64_t);
extern RS_SORT_PAIRS(uint64_t, uint32_t);
extern RS_SORT_PAIRS(uint64_t, uint64_t);
