// tiled_sort.hpp -- the tiled passes of the project's sort: stable LSD radix sort of (key, value) pairs, 8-bit digits, 4096-key tiles.
//   rs_hist / rs_rowscan / rs_scatter : histogram / row scan / scatter per pass (the sorted mer list of all genomes at once)
//   tiled_sort                        : the pass loop over them, on buffers and a stream of the caller's -- no context, so the stand-alone
//                                       driver tests/cpp/tiled_sort_test.cpp runs exactly what radix_sort.hip's sort_pairs runs
// The tile ranking rs_scatter_tile and the tile size (RS_ITEMS, RS_TILE) are those of small_sort.hpp.
// Compile-time switch, for the driver's bench to take the tile order out (the library is built with the default):
//   RS_SWZ 1: workgroup b of rs_scatter takes tile rs_swz(b) (tile_swz.hpp); 0: tile b
#pragma once
#include "small_sort.hpp"
#include "tile_swz.hpp"

#ifndef RS_SWZ
#define RS_SWZ 1
#endif

__device__ __forceinline__ uint32_t rs_tile_of(uint32_t b, uint32_t nblk) { return RS_SWZ ? rs_swz(b, nblk) : b; }

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
// (a template only so that the header may be included in more than one translation unit)
template <int = 0>
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
// The workgroup's tile is rs_tile_of(blockIdx.x): everything indexed by tile -- the histogram column, the keys, the bitmap word -- goes by it.
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
    const uint32_t tile = rs_tile_of(blockIdx.x, nblk);
    const uint32_t tile_base = tile * RS_TILE;
    const uint32_t tile_n = min((uint32_t)RS_TILE, n - tile_base);

    for (int w = 0; w < RS_WAVES; w++) wcount[w][tid] = 0;
    // digit base = exclusive scan of the digit totals
    if (RAW) {
        const uint32_t *row = hist + (size_t)tid * nblk;
        uint32_t tot = 0, before = 0;
        for (uint32_t t = 0; t < nblk; t++) { const uint32_t c = row[t]; tot += c; before += t < tile ? c : 0u; }
        uint32_t dummy;
        gbase[tid] = block_excl_scan(tot, &dummy, scan) + before;
    } else {
        uint32_t dummy;
        const uint32_t tot = totals[tid];
        gbase[tid] = block_excl_scan(tot, &dummy, scan) + hist[(size_t)tid * nblk + tile];
    }
    __syncthreads();
    if (tile_n == RS_TILE)
        rs_scatter_tile<KeyT, RS_ITEMS, true, ValT, IOTA>(keys_in, vals_in, keys_out, vals_out, tile_base, tile_n, shift, s_keys, s_vals, wcount, gbase, tstart, scan,
                                                          nullptr, 0, 0, reinterpret_cast<const uint64_t *>(vals_in));
    else
        rs_scatter_tile<KeyT, RS_ITEMS, false, ValT, IOTA>(keys_in, vals_in, keys_out, vals_out, tile_base, tile_n, shift, s_keys, s_vals, wcount, gbase, tstart, scan,
                                                           nullptr, 0, 0, reinterpret_cast<const uint64_t *>(vals_in));
}

// workspace of an n-pair tiled sort: hist (32-bit words, rs_hist_words(n) of them) and totals (256 words)
inline uint32_t rs_tiles(uint32_t n) { return (n + RS_TILE - 1) / RS_TILE; }
inline size_t rs_hist_words(uint32_t n) { return (size_t)rs_tiles(n) * 256; }

// Stable LSD passes over bits [shift_lo, key_bits) of the n pairs in *keys_io / *vals_io, which point at the result on return (the
// alternates after an odd number of passes).  hist / totals: the workspace above; have_hist0: hist already holds the tile histograms of
// the first pass (hist[d * tiles + tile]).  raw: no row scan launch, every scatter workgroup sums its digit's row for itself (few tiles).
// iota: the first pass takes the strand bitmap for values (rs_scatter above).  book(kind, launch) calls launch() once (a place to time
// it); kind = RS_K_HIST, RS_K_SCAN or RS_K_SCATTER.
enum { RS_K_HIST = 0, RS_K_SCAN = 1, RS_K_SCATTER = 2 };
template <typename KeyT, typename ValT, typename Book>
inline void tiled_sort(hipStream_t st, uint32_t n, int key_bits, int shift_lo, KeyT **keys_io, ValT **vals_io, KeyT *keys_alt, ValT *vals_alt,
                       uint32_t *hist, uint32_t *totals, bool have_hist0, bool raw, bool iota, Book &&book)
{
    const uint32_t nblk = rs_tiles(n);
    KeyT *kin = *keys_io, *kout = keys_alt; ValT *vin = *vals_io, *vout = vals_alt;
    for (int shift = shift_lo; shift < key_bits; shift += 8) {
        if (!(shift == shift_lo && have_hist0))
            book(RS_K_HIST, [&] { hipLaunchKernelGGL(rs_hist<KeyT>, dim3(nblk), dim3(RS_THREADS), 0, st, kin, n, shift, hist, nblk); });
        const bool first_iota = iota && shift == shift_lo;      // *vals_io holds the strand bitmap, not values
        if (raw)
            book(RS_K_SCATTER, [&] {
                hipLaunchKernelGGL((first_iota ? rs_scatter<KeyT, true, ValT, true> : rs_scatter<KeyT, true, ValT, false>), dim3(nblk), dim3(RS_THREADS), 0, st,
                                   kin, vin, kout, vout, n, shift, hist, totals, nblk); });
        else {
            book(RS_K_SCAN, [&] { hipLaunchKernelGGL(rs_rowscan<>, dim3(256), dim3(256), 0, st, hist, nblk, totals); });
            book(RS_K_SCATTER, [&] {
                hipLaunchKernelGGL((first_iota ? rs_scatter<KeyT, false, ValT, true> : rs_scatter<KeyT, false, ValT, false>), dim3(nblk), dim3(RS_THREADS), 0, st,
                                   kin, vin, kout, vout, n, shift, hist, totals, nblk); });
        }
        KeyT *tk = kin; kin = kout; kout = tk;
        ValT *tv = vin; vin = vout; vout = tv;
    }
    *keys_io = kin; *vals_io = vin;
}
