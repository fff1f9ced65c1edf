// small_sort.hpp -- the tile ranking of the LSD radix sort (8-bit digits, stable, (u32 | u64 key, u32 value) pairs) and the
// small-sort engine built on it.
//
// rs_scatter_tile is the ranking and scatter of one tile, templated on the keys per thread: the main sort of radix_sort.hip
// runs it at 16 (4096-key tiles), the small engine at 1 .. 16.
//
// Small sorts (n <= SS_CAP: the chain's per-genome orders, the DP launch list, the canonical order -- 10^3 .. 10^5 pairs)
// are launch-latency bound: at 4096-key tiles a 56 k-pair sort is 14 workgroups on a 256-CU device, each thread ranking
// 16 keys one after another, and every digit pass is two launches (tile histograms, scatter).  The engine here
//   - sizes the tile to the list (256 .. 2048 keys on 256 threads, see ss_items), so the grid spreads over more CUs;
//   - launches ONE kernel per digit pass after the first: the scatter of pass p adds every key it writes to the tile
//     histogram of pass p + 1 (agent-scope atomic adds, executed at the memory side -- correct across XCDs, and read by
//     the next launch after the kernel boundary); the histogram launch only runs for the first pass;
//   - has no row scan: every workgroup of a scatter sums its digit's counts over the tiles before it for itself
//     (tile-major rows, one coalesced 1 KB load per tile).
// The histograms rotate through three slots of nblk x 256 words: pass p reads slot p % 3, adds into slot (p + 1) % 3 and
// zeroes slot (p + 2) % 3 (last read by pass p - 1, next added to by pass p + 1), so no memset launch is needed.
// The permutation is the one of the tiled sort at any tile size (stable LSD), and the result lands in the buffer the
// pass parity implies: keys_io after an even number of passes, keys_alt after an odd one.
//
// Batched form (small_sort_batch): S independent sorts of n pairs each, same key_bits, the segments at a fixed stride in the
// key, value and alternate buffers (the chain's orders of all genomes, made in one go).  The segment is the grid's y
// dimension: the kernels offset their pointers by it and every segment has histogram slots of its own, so a launch does
// what S launches of the single sort would, to every segment exactly what small_sort does to it: the tile class comes
// from n, not from S * n.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

constexpr int RS_THREADS = 256;
constexpr int RS_WAVES = RS_THREADS / 64;
constexpr int RS_ITEMS = 16;                     // keys per thread of the main sort (tiled_sort.hpp) ...
constexpr int RS_TILE = RS_THREADS * RS_ITEMS;   // ... 4096 keys per workgroup: seed_extract_all lays the first pass's histograms out by it

// block-wide exclusive scan of one value per thread (256 threads); returns the exclusive prefix, *total
// receives the block sum.  One global atomic per block instead of one per wave keeps a single output
// counter far below its ~12 ns-per-atomic serial rate (MI355X_MICROARCH.md "fanin").
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t *total, uint32_t *lds /*[8]*/)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { uint32_t t = __shfl_up(inc, o); if (lane >= o) inc += t; }
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    uint32_t wbase = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < 4; w++) { uint32_t c = lds[w]; if (w < wave) wbase += c; tot += c; }
    __syncthreads();
    *total = tot;
    return wbase + inc - v;
}

// One tile of the scatter: ITEMS keys per thread, RS_THREADS * ITEMS per tile.  FULL: the tile is whole, so no lane is
// ever predicated off (all tiles but the last) -- the loads, ballots and stores compile without exec-mask branches.
// hnext (small engine only): tile-major histogram of the next pass (digit at shift + 8, tiles of 1 << tile_log2 keys),
// which every written key is added to; hbits: bits of a counter index there (8 + bits of the tile number).
// IOTA (the seed pass's first sort pass, radix_sort.hip): there is no vals_in.  The value of the key at index x is x itself plus one
// strand bit in the top bit of ValT, bit x of the bitmap sbits (64-bit words; tile_base is a multiple of 64).  The 64 items (i, lane 0..63)
// of a wave are 64 consecutive indices from a multiple of 64, so their bits are one word: lane j < ITEMS fetches the word of item j -- one
// coalesced load per wave -- and item i reads it from lane i.
template <typename KeyT, int ITEMS, bool FULL, typename ValT = uint32_t, bool IOTA = false>
__device__ __forceinline__ void rs_scatter_tile(const KeyT *__restrict__ keys_in, const ValT *__restrict__ vals_in,
                                                KeyT *__restrict__ keys_out, ValT *__restrict__ vals_out,
                                                uint32_t tile_base, uint32_t tile_n, int shift, KeyT *s_keys, ValT *s_vals,
                                                uint32_t (*wcount)[256], const uint32_t *gbase, uint32_t *tstart, uint32_t *scan,
                                                uint32_t *__restrict__ hnext = nullptr, int tile_log2 = 0, int hbits = 0,
                                                const uint64_t *__restrict__ sbits = nullptr)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // load (wave-striped: wave w owns [w*64*ITEMS, (w+1)*64*ITEMS), item i of lane l is index i*64+l)
    KeyT k[ITEMS]; ValT v[ITEMS]; uint32_t rank[ITEMS];
    const uint32_t wbase = wave * (64 * ITEMS);
    uint32_t sb_lo = 0, sb_hi = 0;
    if (IOTA) {
        // (every word of a tile exists, also behind tile_n: the bitmap is whole tiles long, zero beyond the last key)
        const uint64_t w = lane < ITEMS ? sbits[(size_t)((tile_base + wbase) >> 6) + (uint32_t)lane] : 0ULL;
        sb_lo = (uint32_t)w; sb_hi = (uint32_t)(w >> 32);
    }
#pragma unroll
    for (int i = 0; i < ITEMS; i++) {
        const uint32_t li = wbase + i * 64 + lane;
        const bool ok = FULL || li < tile_n;
        k[i] = ok ? keys_in[tile_base + li] : (KeyT)0;
        if (IOTA) {
            const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int32_t)sb_lo, i), hi = (uint32_t)__builtin_amdgcn_readlane((int32_t)sb_hi, i);
            const uint32_t half = lane < 32 ? lo : hi;
            v[i] = ok ? (ValT)(tile_base + li) | ((ValT)((half >> (lane & 31)) & 1u) << (8 * sizeof(ValT) - 1)) : (ValT)0;
        } else
            v[i] = ok ? vals_in[tile_base + li] : (ValT)0;
    }
    // wave-level multisplit ranking, stable in (i, lane) order.  peers = lanes of row i with the same digit, built
    // as two 32-bit halves from eight ballots (one 3-input bit op per half and bit).  The wave owns
    // wcount[wave][]: every peer reads the running count, then the first peer bumps it -- LDS operations of one
    // wave stay in order, so no atomic and no broadcast is needed.
    uint32_t *wc = wcount[wave];
#pragma unroll
    for (int i = 0; i < ITEMS; i++) {
        const uint32_t li = wbase + i * 64 + lane;
        const bool ok = FULL || li < tile_n;
        const uint32_t d = (uint32_t)(k[i] >> shift) & 255u;
        uint32_t plo, phi;
        if (FULL) { plo = 0xffffffffu; phi = 0xffffffffu; }
        else { const uint64_t a = __ballot(ok); plo = (uint32_t)a; phi = (uint32_t)(a >> 32); }
#pragma unroll
        for (int b = 0; b < 8; b++) {
            const uint64_t m = FULL ? __ballot((d >> b) & 1) : __ballot(ok && ((d >> b) & 1));
            const uint32_t sb = (uint32_t)((int32_t)(d << (31 - b)) >> 31);     // all ones when bit b of d is set
            plo &= ~((uint32_t)m ^ sb); phi &= ~((uint32_t)(m >> 32) ^ sb);
        }
        const uint32_t below = __builtin_amdgcn_mbcnt_hi(phi, __builtin_amdgcn_mbcnt_lo(plo, 0u));
        const uint32_t old = ok ? wc[d] : 0u;
        if (ok && below == 0) wc[d] = old + (uint32_t)__popc(plo) + (uint32_t)__popc(phi);
        rank[i] = old + below;
    }
    __syncthreads();
    // per-digit prefix over the waves, then the tile-level digit starts
    uint32_t c[RS_WAVES], sum = 0;
#pragma unroll
    for (int w = 0; w < RS_WAVES; w++) { c[w] = wcount[w][tid]; }
#pragma unroll
    for (int w = 0; w < RS_WAVES; w++) { uint32_t t = c[w]; wcount[w][tid] = sum; sum += t; }
    {
        uint32_t dummy;
        tstart[tid] = block_excl_scan(sum, &dummy, scan);
    }
    __syncthreads();
    // stage in LDS at the tile-sorted position
#pragma unroll
    for (int i = 0; i < ITEMS; i++) {
        const uint32_t li = wbase + i * 64 + lane;
        if (FULL || li < tile_n) {
            const uint32_t d = (uint32_t)(k[i] >> shift) & 255u;
            const uint32_t pos = tstart[d] + wc[d] + rank[i];
            s_keys[pos] = k[i]; s_vals[pos] = v[i];
        }
    }
    __syncthreads();
    // coalesced write-out: consecutive threads write consecutive addresses inside a digit's run
#pragma unroll
    for (int i = 0; i < ITEMS; i++) {
        const uint32_t pos = i * RS_THREADS + tid;
        if (FULL || pos < tile_n) {
            const KeyT kk = s_keys[pos];
            const uint32_t d = (uint32_t)(kk >> shift) & 255u;
            const uint32_t dst = gbase[d] + (pos - tstart[d]);
            keys_out[dst] = kk; vals_out[dst] = s_vals[pos];
            if (hnext) {
                // the lanes of this store that add to the same counter add once, by the lowest of them: sorted input gives whole tiles
                // of one next digit, and adds to one word serialise (~12 ns each)
                const uint32_t hi = ((dst >> tile_log2) << 8) | ((uint32_t)(kk >> (shift + 8)) & 255u);
                uint64_t peers = __ballot(1);
                for (int b = 0; b < hbits; b++) { const uint64_t m = __ballot((hi >> b) & 1); peers &= ((hi >> b) & 1) ? m : ~m; }
                if ((peers & ((1ULL << lane) - 1)) == 0)
                    (void)__hip_atomic_fetch_add(hnext + hi, (uint32_t)__popcll(peers), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}

// ---- the small-sort engine ----
constexpr uint32_t SS_CAP = 64u * 4096u;    // largest n the engine takes (the tiled RAW path's old range)

// keys per thread for an n-pair sort: 1, 2, 4 or 8 (tiles of 256 .. 2048 keys).  Measured (tests/cpp/small_sort_test.cpp bench,
// DESIGN.md 4): a scatter's workgroups each read all nblk tile histograms, so past ~64 tiles the grid costs more than it spreads;
// the fastest tile was 256 keys at n = 4 k, 512 at 16 k, 1024 at 56 k, 2048 at 131 k and 262 k.
inline int ss_items(uint32_t n)
{
    return n <= 8192u ? 1 : n <= 32768u ? 2 : n <= 98304u ? 4 : 8;
}
inline uint32_t ss_tiles(uint32_t n, int items) { return (n + (uint32_t)(RS_THREADS * items) - 1) / (uint32_t)(RS_THREADS * items); }
// workspace of an n-pair sort (three histogram slots), in 32-bit words
inline size_t ss_ws_words(uint32_t n) { return (size_t)3 * ss_tiles(n, ss_items(n)) * 256; }
// ... of S such sorts in one batch (three slots of S x nblk x 256 words)
inline size_t ss_ws_words_batch(uint32_t S, uint32_t n) { return (size_t)S * ss_ws_words(n); }

// tile histogram of the first pass (tile-major: hist[tile * 256 + digit]); hzero (if any): this tile's row of the next slot := 0
// blockIdx.y: the segment of a batch (keys seg_stride apart, histogram rows of its own behind those of the segments before it)
template <typename KeyT, int ITEMS>
__global__ void __launch_bounds__(RS_THREADS) rs_small_hist(const KeyT *__restrict__ keys, uint32_t n, int shift,
                                                            uint32_t *__restrict__ hist, uint32_t *__restrict__ hzero, size_t seg_stride)
{
    __shared__ uint32_t h[256];
    const int tid = threadIdx.x;
    keys += (size_t)blockIdx.y * seg_stride;
    hist += (size_t)blockIdx.y * gridDim.x * 256;
    if (hzero) hzero += (size_t)blockIdx.y * gridDim.x * 256;
    h[tid] = 0;
    __syncthreads();
    const uint32_t base = blockIdx.x * (uint32_t)(RS_THREADS * ITEMS);
#pragma unroll
    for (int i = 0; i < ITEMS; i++) {
        const uint32_t idx = base + i * RS_THREADS + tid;
        if (idx < n) atomicAdd(&h[(uint32_t)(keys[idx] >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[blockIdx.x * 256 + tid] = h[tid];
    if (hzero) hzero[blockIdx.x * 256 + tid] = 0;
}

// one digit pass: hist = this pass's tile histograms (tile-major, nblk tiles); hnext: next pass's slot (added to), hzero: the
// slot after it (this tile's row := 0); either may be null.  blockIdx.y: the segment of a batch, as in rs_small_hist
template <typename KeyT, int ITEMS, typename ValT = uint32_t>
__global__ void __launch_bounds__(RS_THREADS) rs_small_scatter(const KeyT *__restrict__ keys_in, const ValT *__restrict__ vals_in,
                                                               KeyT *__restrict__ keys_out, ValT *__restrict__ vals_out,
                                                               uint32_t n, int shift, const uint32_t *__restrict__ hist, uint32_t nblk,
                                                               uint32_t *__restrict__ hnext, uint32_t *__restrict__ hzero, int hbits,
                                                               size_t seg_stride)
{
    constexpr int TILE = RS_THREADS * ITEMS;
    __shared__ KeyT s_keys[TILE];
    __shared__ ValT s_vals[TILE];
    __shared__ uint32_t wcount[RS_WAVES][256];
    __shared__ uint32_t gbase[256];       // global output index of this tile's first key of digit d
    __shared__ uint32_t tstart[256];      // tile-local start of digit d
    __shared__ uint32_t scan[8];

    const int tid = threadIdx.x;
    {
        const size_t so = (size_t)blockIdx.y * seg_stride, ho = (size_t)blockIdx.y * nblk * 256;
        keys_in += so; vals_in += so; keys_out += so; vals_out += so;
        hist += ho;
        if (hnext) hnext += ho;
        if (hzero) hzero += ho;
    }
    const uint32_t blk = blockIdx.x, tile_base = blk * TILE;
    const uint32_t tile_n = min((uint32_t)TILE, n - tile_base);
#pragma unroll
    for (int w = 0; w < RS_WAVES; w++) wcount[w][tid] = 0;
    // digit d's total and its count in the tiles before this one: 32 tiles' loads in flight at a time (a batch is an L2 round trip,
    // ~0.25 us: eight at a time made this sum the largest part of a scatter at 200 tiles)
    uint32_t tot = 0, before = 0;
    for (uint32_t t = 0; t < nblk; t += 32) {
        uint32_t c[32];
#pragma unroll
        for (int q = 0; q < 32; q++) c[q] = t + q < nblk ? hist[(t + q) * 256 + tid] : 0u;
#pragma unroll
        for (int q = 0; q < 32; q++) { tot += c[q]; before += t + q < blk ? c[q] : 0u; }
    }
    if (hzero) hzero[blk * 256 + tid] = 0;
    {
        uint32_t dummy;
        gbase[tid] = block_excl_scan(tot, &dummy, scan) + before;
    }
    __syncthreads();
    constexpr int LOG2 = ITEMS == 1 ? 8 : ITEMS == 2 ? 9 : ITEMS == 4 ? 10 : ITEMS == 8 ? 11 : 12;
    static_assert(TILE == 1 << LOG2, "ITEMS must be 1, 2, 4, 8 or 16");
    if (tile_n == (uint32_t)TILE)
        rs_scatter_tile<KeyT, ITEMS, true, ValT>(keys_in, vals_in, keys_out, vals_out, tile_base, tile_n, shift, s_keys, s_vals, wcount, gbase,
                                           tstart, scan, hnext, LOG2, hbits);
    else
        rs_scatter_tile<KeyT, ITEMS, false, ValT>(keys_in, vals_in, keys_out, vals_out, tile_base, tile_n, shift, s_keys, s_vals, wcount, gbase,
                                            tstart, scan, hnext, LOG2, hbits);
}

// S segments seg_stride elements apart (S = 1: the single sort)
template <typename KeyT, int ITEMS, typename ValT, typename Book>
inline void ss_run(hipStream_t st, uint32_t n, int key_bits, int shift_lo, KeyT *kin, ValT *vin, KeyT *kout, ValT *vout,
                   uint32_t *ws, Book &book, uint32_t S = 1, size_t seg_stride = 0)
{
    const uint32_t nblk = ss_tiles(n, ITEMS);
    const size_t slot = (size_t)S * nblk * 256;
    int hbits = 8;                                      // bits of a histogram counter index: digit, tile number
    while ((1u << (hbits - 8)) < nblk) hbits++;
    int p = 0;
    for (int shift = shift_lo; shift < key_bits; shift += 8, p++) {
        uint32_t *h = ws + (p % 3) * slot;
        uint32_t *hnext = shift + 8 < key_bits ? ws + ((p + 1) % 3) * slot : nullptr;
        uint32_t *hzero = shift + 16 < key_bits ? ws + ((p + 2) % 3) * slot : nullptr;
        if (p == 0)
            book(false, [&] { hipLaunchKernelGGL((rs_small_hist<KeyT, ITEMS>), dim3(nblk, S), dim3(RS_THREADS), 0, st, kin, n, shift, h, hnext, seg_stride); });
        book(true, [&] {
            hipLaunchKernelGGL((rs_small_scatter<KeyT, ITEMS, ValT>), dim3(nblk, S), dim3(RS_THREADS), 0, st, kin, vin, kout, vout, n, shift, h, nblk,
                               hnext, hzero, hbits, seg_stride);
        });
        KeyT *tk = kin; kin = kout; kout = tk;
        ValT *tv = vin; vin = vout; vout = tv;
    }
}

// Stable LSD sort of n (1 <= n <= SS_CAP) pairs over bits [shift_lo, key_bits), 8 bits per pass; on return *keys_io / *vals_io
// point at the buffers holding the result (the alternates after an odd number of passes).  ws: ss_ws_words(n) words of
// device memory, contents irrelevant.  book(scatter, launch): calls launch() once (a place to time it); scatter = false
// for the histogram launch.
// small_sort_batch: S such sorts at once (1 <= S <= 65535), segment s in the seg_stride elements from s * seg_stride of every
// buffer (seg_stride >= n); *keys_io / *vals_io point at segment 0 of the result.  ws: ss_ws_words_batch(S, n) words.
template <typename KeyT, typename ValT, typename Book>
inline void small_sort_batch(hipStream_t st, uint32_t S, uint32_t n, size_t seg_stride, int key_bits, int shift_lo, KeyT **keys_io,
                             ValT **vals_io, KeyT *keys_alt, ValT *vals_alt, uint32_t *ws, Book &&book)
{
    KeyT *kin = *keys_io; ValT *vin = *vals_io;
    switch (ss_items(n)) {
    case 1: ss_run<KeyT, 1, ValT>(st, n, key_bits, shift_lo, kin, vin, keys_alt, vals_alt, ws, book, S, seg_stride); break;
    case 2: ss_run<KeyT, 2, ValT>(st, n, key_bits, shift_lo, kin, vin, keys_alt, vals_alt, ws, book, S, seg_stride); break;
    case 4: ss_run<KeyT, 4, ValT>(st, n, key_bits, shift_lo, kin, vin, keys_alt, vals_alt, ws, book, S, seg_stride); break;
    default: ss_run<KeyT, 8, ValT>(st, n, key_bits, shift_lo, kin, vin, keys_alt, vals_alt, ws, book, S, seg_stride); break;
    }
    const int passes = key_bits > shift_lo ? (key_bits - shift_lo + 7) / 8 : 0;
    if (passes & 1) { *keys_io = keys_alt; *vals_io = vals_alt; }
}
template <typename KeyT, typename ValT, typename Book>
inline void small_sort(hipStream_t st, uint32_t n, int key_bits, int shift_lo, KeyT **keys_io, ValT **vals_io, KeyT *keys_alt,
                       ValT *vals_alt, uint32_t *ws, Book &&book)
{
    small_sort_batch<KeyT, ValT>(st, 1, n, 0, key_bits, shift_lo, keys_io, vals_io, keys_alt, vals_alt, ws, book);
}
