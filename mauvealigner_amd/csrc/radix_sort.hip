// radix_sort.hip -- the project's sort on gfx950: stable LSD radix sort of (key, value) pairs, 8-bit digits.
//   tiled_sort.hpp : rs_hist / rs_rowscan / rs_scatter and the pass loop over them, 4096-key tiles (the sorted mer list of all genomes at once)
//   small_sort.hpp : the tile ranking they share with the small-sort engine, and that engine (n <= SS_CAP)
// sort_pairs holds what belongs to the context: its buffers, the timers, and the choice between small sort, raw tile histograms and row scan.
// Callers: the seed pass and the multiplicity pass (seed_pass.hip, through radix_sort.hpp), the chain stage (chain_dev.hip), the DP
// launch list (dp_batch.hip) and the canonical order (seed_finish.hip) through sort_pairs_u32 / _u32_batch / _u64 (common.hpp).
#include "radix_sort.hpp"
#include "tiled_sort.hpp"
#include <algorithm>
#include <cstdlib>

template <typename KeyT, typename ValT>
int sort_pairs(mauve_ctx *ctx, uint32_t n, int key_bits, KeyT **keys_io, ValT **vals_io, KeyT *keys_alt, ValT *vals_alt, bool have_hist0,
               int timer_id, int shift_lo, bool iota)
{
    const int k_hist = timer_id >= 0 ? timer_id : MAUVE_K_SORT_HIST, k_scan = timer_id >= 0 ? timer_id : MAUVE_K_SORT_SCAN,
              k_scat = timer_id >= 0 ? timer_id : MAUVE_K_SORT_SCATTER;
    if (iota && !(have_hist0 && shift_lo < key_bits)) { ctx->err = "sort_pairs: values from the strand bitmap need a first tiled pass"; return MAUVE_ERR_ARG; }
    if (switches().small_sort && !have_hist0 && n >= 1 && n <= SS_CAP) {      // small sort: device-sized tiles, one launch per digit pass
        HIPCHK(ctx, ctx->hist.ensure(ss_ws_words(n) * sizeof(uint32_t)));
        small_sort<KeyT>(ctx->stream, n, key_bits, shift_lo, keys_io, vals_io, keys_alt, vals_alt, ctx->hist.as<uint32_t>(),
                         [&](bool scatter, auto &&launch) { KernelTimer t(ctx, scatter ? k_scat : k_hist, n); launch(); });
        HIPCHK(ctx, hipGetLastError());
        return MAUVE_OK;
    }
    HIPCHK(ctx, ctx->hist.ensure(rs_hist_words(n) * sizeof(uint32_t)));
    HIPCHK(ctx, ctx->totals.ensure(256 * sizeof(uint32_t)));
    // (up to 64 tiles: no row scan launch, the scatter reads the raw tile histograms)
    tiled_sort<KeyT, ValT>(ctx->stream, n, key_bits, shift_lo, keys_io, vals_io, keys_alt, vals_alt, ctx->hist.as<uint32_t>(), ctx->totals.as<uint32_t>(),
                           have_hist0, rs_tiles(n) <= 64, iota, [&](int kind, auto &&launch) {
                               KernelTimer t(ctx, kind == RS_K_HIST ? k_hist : kind == RS_K_SCAN ? k_scan : k_scat, n); launch(); });
    HIPCHK(ctx, hipGetLastError());
    return MAUVE_OK;
}
RS_SORT_PAIRS(uint32_t, uint32_t);
RS_SORT_PAIRS(uint32_t, uint64_t);
RS_SORT_PAIRS(uint64_t, uint32_t);
RS_SORT_PAIRS(uint64_t, uint64_t);

// stable LSD radix sort of (32-bit key, 32-bit value) pairs for the other translation units (chain_dev.hip) ...
int sort_pairs_u32(mauve_ctx *ctx, uint32_t n, int key_bits, uint32_t **keys_io, uint32_t **vals_io, uint32_t *keys_alt, uint32_t *vals_alt,
                   int timer_id)
{
    return sort_pairs<uint32_t>(ctx, n, key_bits, keys_io, vals_io, keys_alt, vals_alt, false, timer_id);
}
// S such sorts of n pairs each, same key_bits, segment s in the n pairs from s * seg_stride of all four buffers (chain_dev.hip: the orders of all
// genomes): one batched small sort, or -- engine off, n beyond its range -- S sorts one after another on the same buffers.  Either way every
// segment gets the permutation and the result-buffer parity of sort_pairs_u32; *keys_io / *vals_io point at segment 0 of the result.
int sort_pairs_u32_batch(mauve_ctx *ctx, uint32_t S, uint32_t n, size_t seg_stride, int key_bits, uint32_t **keys_io, uint32_t **vals_io,
                         uint32_t *keys_alt, uint32_t *vals_alt, int timer_id)
{
    if (S == 0 || n == 0) return MAUVE_OK;
    if (S > 65535u || seg_stride < n) { ctx->err = "sort_pairs_u32_batch: bad segment layout"; return MAUVE_ERR_ARG; }
    if (switches().small_sort && n <= SS_CAP) {
        const int k_hist = timer_id >= 0 ? timer_id : MAUVE_K_SORT_HIST, k_scat = timer_id >= 0 ? timer_id : MAUVE_K_SORT_SCATTER;
        HIPCHK(ctx, ctx->hist.ensure(ss_ws_words_batch(S, n) * sizeof(uint32_t)));
        small_sort_batch<uint32_t>(ctx->stream, S, n, seg_stride, key_bits, 0, keys_io, vals_io, keys_alt, vals_alt, ctx->hist.as<uint32_t>(),
                                   [&](bool scatter, auto &&launch) { KernelTimer t(ctx, scatter ? k_scat : k_hist, (int64_t)S * n); launch(); });
        HIPCHK(ctx, hipGetLastError());
        return MAUVE_OK;
    }
    uint32_t *k0 = *keys_io, *v0 = *vals_io;
    for (uint32_t s = 0; s < S; s++) {
        uint32_t *kk = *keys_io + s * seg_stride, *vv = *vals_io + s * seg_stride;
        int rc = sort_pairs<uint32_t>(ctx, n, key_bits, &kk, &vv, keys_alt + s * seg_stride, vals_alt + s * seg_stride, false, timer_id);
        if (rc) return rc;
        if (s == 0) { k0 = kk; v0 = vv; }
    }
    *keys_io = k0; *vals_io = v0;
    return MAUVE_OK;
}
// ... and of (64-bit key, 32-bit value) pairs (seed_finish.hip)
int sort_pairs_u64(mauve_ctx *ctx, uint32_t n, int key_bits, uint64_t **keys_io, uint32_t **vals_io, uint64_t *keys_alt, uint32_t *vals_alt,
                   int timer_id)
{
    return sort_pairs<uint64_t>(ctx, n, key_bits, keys_io, vals_io, keys_alt, vals_alt, false, timer_id);
}
