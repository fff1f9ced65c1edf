// radix_sort.hip -- the project's sort on gfx950: stable LSD radix sort of (key, value) pairs, 8-bit digits.
//   rs_hist / rs_rowscan / rs_scatter : histogram / row scan / scatter per pass, 4096-key tiles (the sorted mer list of all genomes at once)
//   small_sort.hpp                    : the tile ranking they share with the small-sort engine, and that engine (n <= SS_CAP)
// Callers: the seed pass and the multiplicity pass (seed_pass.hip, through radix_sort.hpp), the chain stage (chain_dev.hip), the DP
// launch list (dp_batch.hip) and the canonical order (seed_finish.hip) through sort_pairs_u32 / _u32_batch / _u64 (common.hpp).
#include "radix_sort.hpp"
#include <algorithm>
#include <cstdlib>

template <typename KeyT>
__global__ void __launch_bounds__(RS_THREADS) rs_hist(const KeyT *__restrict__ keys, uint32_t n, int shift,
                                                      uint32_t *__restrict__ hist, uint32_t nblk)
{
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t base = blockIdx.x * RS_TILE;
    if (base + RS_TILE <= n) {
        // full tile: 16-byte loads, no predication (the order inside a tile does not matter for a histogram)
        constexpr int KPV = 16 / (int)sizeof(KeyT);
        struct alignas(16) Vec { KeyT k[KPV]; };
        const Vec *src = reinterpret_cast<const Vec *>(keys + base);
#pragma unroll
        for (int i = 0; i < RS_ITEMS / KPV; i++) {
            const Vec q = src[i * RS_THREADS + threadIdx.x];
#pragma unroll
            for (int j = 0; j < KPV; j++) atomicAdd(&h[(uint32_t)(q.k[j] >> shift) & 255u], 1u);
        }
    } else {
#pragma unroll
        for (int i = 0; i < RS_ITEMS; i++) {
            const uint32_t idx = base + i * RS_THREADS + threadIdx.x;
            if (idx < n) atomicAdd(&h[(uint32_t)(keys[idx] >> shift) & 255u], 1u);
        }
    }
    __syncthreads();
    hist[threadIdx.x * nblk + blockIdx.x] = h[threadIdx.x];
}

// block d: exclusive scan of row d (length nblk) in place, row total -> totals[d]
// (a wave per quarter of the digit's row, 64 consecutive counts per step -- coalesced loads, a DPP prefix sum, one carry -- instead of a thread per 24
// consecutive counts walking them twice with loads 96 bytes apart: 17 -> 6 us per launch at C3's 6 104 tiles)
__device__ __forceinline__ uint32_t wave_incl_sum_u32(uint32_t v)
{
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int32_t)v, 0x111, 0xf, 0xf, false); v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int32_t)v, 0x112, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int32_t)v, 0x114, 0xf, 0xf, false); v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int32_t)v, 0x118, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int32_t)v, 0x142, 0xa, 0xf, false); v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int32_t)v, 0x143, 0xc, 0xf, false);
    return v;
}
__global__ void __launch_bounds__(256) rs_rowscan(uint32_t *__restrict__ hist, uint32_t nblk,
                                                  uint32_t *__restrict__ totals)
{
    __shared__ uint32_t part[4];                             // (launched with 256 threads: four waves, a quarter of the row each)
    uint32_t *row = hist + (size_t)blockIdx.x * nblk;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t seg = (((nblk + 3) / 4) + 63) & ~63u;           // counts per wave, whole steps of 64
    const uint32_t lo = min((uint32_t)wv * seg, nblk), hi = min(lo + seg, nblk);
    // (eight steps' loads in flight at a time: a loop that waits for one load per step is a chain of L2 latencies, 24 of them at C3)
    uint32_t s = 0;
    for (uint32_t i0 = lo; i0 < hi; i0 += 512) {
        uint32_t v[8];
#pragma unroll
        for (int q = 0; q < 8; q++) { const uint32_t idx = i0 + q * 64 + lane; v[q] = idx < hi ? row[idx] : 0u; }
#pragma unroll
        for (int q = 0; q < 8; q++) s += v[q];
    }
    s = wave_incl_sum_u32(s);
    if (lane == 63) part[wv] = s;
    __syncthreads();
    uint32_t run = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 4; w++) { const uint32_t c = part[w]; if (w < wv) run += c; total += c; }
    for (uint32_t i0 = lo; i0 < hi; i0 += 512) {
        uint32_t v[8];
#pragma unroll
        for (int q = 0; q < 8; q++) { const uint32_t idx = i0 + q * 64 + lane; v[q] = idx < hi ? row[idx] : 0u; }
#pragma unroll
        for (int q = 0; q < 8; q++) {
            const uint32_t idx = i0 + q * 64 + lane;
            const uint32_t inc = wave_incl_sum_u32(v[q]);
            if (idx < hi) row[idx] = run + inc - v[q];
            run += (uint32_t)__builtin_amdgcn_readlane((int32_t)inc, 63);
        }
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = total;
}

// RAW: `hist` holds the raw per-tile digit counts (no rs_rowscan ran): every workgroup sums its digit's row for itself --
// the sorts of the chain / DP front / canonical order have at most a few dozen tiles, where the row scan is one more
// launch of pure latency.
// LDS per workgroup (RS_TILE = 4096): keys + values + 7 KiB of counters -- 39 KiB for 4 + 4 bytes, 55 KiB for 8 + 4 or 4 + 8, 71 KiB for 8 + 8
// (the wide pass with 64-bit keys): 4, 2, 2 workgroups per compute unit of 160 KiB.
// IOTA: the first pass of the seed pass's sort -- no value array comes in, vals_in is the strand bitmap seed_extract_all wrote beside the keys
// (one bit per key, whole tiles) and a key's value is its own index plus that bit (rs_scatter_tile).
template <typename KeyT, bool RAW = false, typename ValT = uint32_t, bool IOTA = false>
__global__ void __launch_bounds__(RS_THREADS) rs_scatter(const KeyT *__restrict__ keys_in,
                                                         const ValT *__restrict__ vals_in,
                                                         KeyT *__restrict__ keys_out,
                                                         ValT *__restrict__ vals_out, uint32_t n, int shift,
                                                         const uint32_t *__restrict__ hist,
                                                         const uint32_t *__restrict__ totals, uint32_t nblk)
{
    __shared__ KeyT s_keys[RS_TILE];
    __shared__ ValT s_vals[RS_TILE];
    __shared__ uint32_t wcount[RS_WAVES][256];
    __shared__ uint32_t gbase[256];       // global output index of this tile's first key of digit d
    __shared__ uint32_t tstart[256];      // tile-local start of digit d
    __shared__ uint32_t scan[256];

    const int tid = threadIdx.x;
    const uint32_t tile_base = blockIdx.x * RS_TILE;
    const uint32_t tile_n = min((uint32_t)RS_TILE, n - tile_base);

    for (int w = 0; w < RS_WAVES; w++) wcount[w][tid] = 0;
    // digit base = exclusive scan of the digit totals
    if (RAW) {
        const uint32_t *row = hist + (size_t)tid * nblk;
        uint32_t tot = 0, before = 0;
        for (uint32_t t = 0; t < nblk; t++) { const uint32_t c = row[t]; tot += c; before += t < blockIdx.x ? c : 0u; }
        uint32_t dummy;
        gbase[tid] = block_excl_scan(tot, &dummy, scan) + before;
    } else {
        uint32_t dummy;
        const uint32_t tot = totals[tid];
        gbase[tid] = block_excl_scan(tot, &dummy, scan) + hist[(size_t)tid * nblk + blockIdx.x];
    }
    __syncthreads();
    if (tile_n == RS_TILE)
        rs_scatter_tile<KeyT, RS_ITEMS, true, ValT, IOTA>(keys_in, vals_in, keys_out, vals_out, tile_base, tile_n, shift, s_keys, s_vals, wcount, gbase, tstart, scan,
                                                          nullptr, 0, 0, reinterpret_cast<const uint64_t *>(vals_in));
    else
        rs_scatter_tile<KeyT, RS_ITEMS, false, ValT, IOTA>(keys_in, vals_in, keys_out, vals_out, tile_base, tile_n, shift, s_keys, s_vals, wcount, gbase, tstart, scan,
                                                           nullptr, 0, 0, reinterpret_cast<const uint64_t *>(vals_in));
}

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
    uint32_t nblk = (n + RS_TILE - 1) / RS_TILE;
    HIPCHK(ctx, ctx->hist.ensure((size_t)nblk * 256 * sizeof(uint32_t)));
    HIPCHK(ctx, ctx->totals.ensure(256 * sizeof(uint32_t)));
    KeyT *kin = *keys_io, *kout = keys_alt; ValT *vin = *vals_io, *vout = vals_alt;
    for (int shift = shift_lo; shift < key_bits; shift += 8) {
        if (!(shift == shift_lo && have_hist0)) { KernelTimer t(ctx, k_hist, n);
          hipLaunchKernelGGL(rs_hist<KeyT>, dim3(nblk), dim3(RS_THREADS), 0, ctx->stream, kin, n, shift,
                             ctx->hist.as<uint32_t>(), nblk); }
        const bool first_iota = iota && shift == shift_lo;      // *vals_io holds the strand bitmap, not values
        if (nblk <= 64) {      // small sort: no row scan launch, the scatter reads the raw tile histograms
            KernelTimer t(ctx, k_scat, n);
            hipLaunchKernelGGL((first_iota ? rs_scatter<KeyT, true, ValT, true> : rs_scatter<KeyT, true, ValT, false>), dim3(nblk), dim3(RS_THREADS), 0, ctx->stream,
                               kin, vin, kout, vout, n, shift, ctx->hist.as<uint32_t>(), ctx->totals.as<uint32_t>(), nblk);
            std::swap(kin, kout); std::swap(vin, vout);
            continue;
        }
        { KernelTimer t(ctx, k_scan, n);
          hipLaunchKernelGGL(rs_rowscan, dim3(256), dim3(256), 0, ctx->stream, ctx->hist.as<uint32_t>(), nblk,
                             ctx->totals.as<uint32_t>()); }
        { KernelTimer t(ctx, k_scat, n);
          hipLaunchKernelGGL((first_iota ? rs_scatter<KeyT, false, ValT, true> : rs_scatter<KeyT, false, ValT, false>), dim3(nblk), dim3(RS_THREADS), 0, ctx->stream,
                             kin, vin, kout, vout, n, shift, ctx->hist.as<uint32_t>(), ctx->totals.as<uint32_t>(), nblk); }
        std::swap(kin, kout); std::swap(vin, vout);
    }
    HIPCHK(ctx, hipGetLastError());
    *keys_io = kin; *vals_io = vin;
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
