// backbone_host.hpp -- the pure host steps of the backbone stage (backbone_dev.hip: bb_*) and of the homology pass in
// front of it (S12b, homology_dev.hip: hom_*), one copy each, with the plain structs host and device share.
// Host only, no HIP include (like host_chain.hpp): tests/cpp/backbone_host_test.cpp compiles it with plain g++.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <utility>
#include <vector>

#include "../../include/mauve_hip.h"
#include "column_counts.hpp"

// ---- S12 ----
struct BbIv { int64_t col0; int64_t ncols; uint32_t gmask; uint32_t npairs; uint32_t iv; uint32_t chunk0; };
struct BbRec { uint32_t iv, packed, c_first, c_last; };       // packed: a | b << 8 | who << 16 | kind << 24 (0 region, 1 island)
struct BbSeg { uint32_t ivx; uint32_t mask; int64_t c1, c2; };  // a component over a maximal run of columns of ivs[ivx]

// backbone / islands of the last alignment (mauve_backbone_fetch hands them out)
struct BackboneResult {
    int N = 0; bool valid = false;
    std::vector<int64_t> seg_iv, seg_col, seg_len, seg_left, seg_right, islands;
    std::vector<uint32_t> seg_mask;
};

// intervals with >= 2 genomes and columns, their chunks; false: an interval is too long for the 32-bit columns of a record
inline bool bb_intervals(int N, int64_t n_iv, const int64_t *left, const int64_t *col_off, std::vector<BbIv> &ivs, uint32_t *chunks, uint32_t *max_pairs)
{
    ivs.clear(); *chunks = 0; *max_pairs = 0;
    for (int64_t iv = 0; iv < n_iv; iv++) {
        uint32_t gm = 0; for (int g = 0; g < N; g++) if (left[iv * N + g]) gm |= 1u << g;
        const int n = __builtin_popcount(gm); const int64_t nc = col_off[iv + 1] - col_off[iv];
        if (n < 2 || nc <= 0) continue;
        if (nc > 0x7fffffff) return false;
        BbIv d{col_off[iv], nc, gm, (uint32_t)(n * (n - 1) / 2), (uint32_t)iv, *chunks};
        *chunks += (uint32_t)((nc + BB_CHUNK - 1) / BB_CHUNK); *max_pairs = std::max(*max_pairs, d.npairs);
        ivs.push_back(d);
    }
    return true;
}

// connected components (>= 2 genomes) of the joined pairs: adj[g] = genomes joined to g (bit g included)
inline void bb_components(const uint32_t *adj, uint32_t gmask, std::vector<uint32_t> &out)
{
    out.clear();
    uint32_t left = gmask;
    while (left) {
        const int g = __builtin_ctz(left);
        uint32_t comp = 1u << g, front = comp;
        while (front) {
            uint32_t nxt = 0;
            for (uint32_t f = front; f; f &= f - 1) nxt |= adj[__builtin_ctz(f)];
            front = nxt & gmask & ~comp; comp |= front;
        }
        left &= ~comp;
        if (comp & (comp - 1)) out.push_back(comp);
    }
}

// canonical order of the records: interval, kind, pair, first column (the append order is not deterministic)
inline void bb_sort_records(std::vector<BbRec> &recs)
{
    std::sort(recs.begin(), recs.end(), [](const BbRec &x, const BbRec &y) {
        if (x.iv != y.iv) return x.iv < y.iv;
        const uint32_t kx = x.packed >> 24, ky = y.packed >> 24; if (kx != ky) return kx < ky;
        const uint32_t px = (x.packed & 0xff) << 8 | (x.packed >> 8 & 0xff), py = (y.packed & 0xff) << 8 | (y.packed >> 8 & 0xff);
        if (px != py) return px < py;
        return x.c_first < y.c_first;
    });
}

// regions -> segments: sweep the boundaries of the open regions, interval by interval; the island records are set aside (recs sorted)
inline void bb_sweep(const std::vector<BbIv> &ivs, const std::vector<BbRec> &recs, std::vector<BbSeg> &segs, std::vector<BbRec> &islands)
{
    segs.clear(); islands.clear();
    size_t r = 0;
    std::vector<std::pair<int64_t, uint32_t>> ev;              // (column, pair code | open << 31)
    std::vector<uint32_t> comps, prev_comps; std::vector<int64_t> prev_start, start;
    for (size_t x = 0; x < ivs.size(); x++) {
        const BbIv &d = ivs[x];
        ev.clear();
        for (; r < recs.size() && recs[r].iv == d.iv; r++) {
            const BbRec &q = recs[r];
            if (q.packed >> 24) { islands.push_back(q); continue; }
            const uint32_t pc = q.packed & 0xffff;
            ev.push_back({(int64_t)q.c_first, pc | 0x80000000u}); ev.push_back({(int64_t)q.c_last + 1, pc});
        }
        std::sort(ev.begin(), ev.end());
        uint32_t adj[32];
        for (int g = 0; g < 32; g++) adj[g] = d.gmask;             // every pair joined until a region opens
        prev_comps.clear(); prev_start.clear();
        size_t e = 0; int64_t at = 0;
        for (;;) {
            // apply the events at column `at`, then the partition holds from `at` to the next event
            for (; e < ev.size() && ev[e].first == at; e++) {
                const int a = (int)(ev[e].second & 0xff), b = (int)(ev[e].second >> 8 & 0xff);
                if (ev[e].second >> 31) { adj[a] &= ~(1u << b); adj[b] &= ~(1u << a); } else { adj[a] |= 1u << b; adj[b] |= 1u << a; }
            }
            if (at >= d.ncols) comps.clear(); else bb_components(adj, d.gmask, comps);
            start.assign(comps.size(), at);
            for (size_t k = 0; k < prev_comps.size(); k++) {
                const auto it = std::find(comps.begin(), comps.end(), prev_comps[k]);
                if (it != comps.end()) start[(size_t)(it - comps.begin())] = prev_start[k];
                else segs.push_back(BbSeg{(uint32_t)x, prev_comps[k], prev_start[k], at - 1});
            }
            prev_comps = comps; prev_start = start;
            if (at >= d.ncols) break;
            at = e < ev.size() ? std::min<int64_t>(ev[e].first, d.ncols) : d.ncols;
        }
    }
}

// The rank queries: columns whose residue counts (from their tile's start) give the sequence coordinates of the segment and island ends.
// The slots are laid out by construction -- interval starts, then two per segment (from q_seg), then two per island (from q_isl) -- so
// nothing has to be sorted or looked up (a column asked twice costs a wave).  slot: empty, or the place of every slot's column in qcol
struct BbQueries { std::vector<int64_t> qcol; std::vector<uint32_t> slot, isl_ivx; size_t q_seg = 0, q_isl = 0; };

inline void bb_query_slots(const std::vector<BbIv> &ivs, const std::vector<BbSeg> &segs, const std::vector<BbRec> &islands, size_t dedupe_above, BbQueries &Q)
{
    std::vector<int64_t> &qcol = Q.qcol;
    qcol.clear(); Q.slot.clear();
    qcol.reserve(ivs.size() + 2 * (segs.size() + islands.size()));
    for (const BbIv &d : ivs) qcol.push_back(d.col0);
    Q.q_seg = qcol.size();
    for (const BbSeg &s : segs) { qcol.push_back(ivs[s.ivx].col0 + s.c1); qcol.push_back(ivs[s.ivx].col0 + s.c2 + 1); }
    Q.q_isl = qcol.size();
    Q.isl_ivx.resize(islands.size());                               // the islands' intervals (records and ivs are both ordered by interval)
    { size_t x = 0; for (size_t k = 0; k < islands.size(); k++) { while (ivs[x].iv != islands[k].iv) x++; Q.isl_ivx[k] = (uint32_t)x; } }
    for (size_t k = 0; k < islands.size(); k++) { const BbIv &d = ivs[Q.isl_ivx[k]]; qcol.push_back(d.col0 + islands[k].c_first); qcol.push_back(d.col0 + (int64_t)islands[k].c_last + 1); }
    // many genomes with many islands ask for the same columns pair after pair: beyond dedupe_above queries (production: a million) they
    // are made unique first (one sort) and every slot is looked up once
    if (qcol.size() > dedupe_above) {
        const std::vector<int64_t> all(qcol);
        std::sort(qcol.begin(), qcol.end()); qcol.erase(std::unique(qcol.begin(), qcol.end()), qcol.end());
        Q.slot.resize(all.size());
        for (size_t k = 0; k < all.size(); k++) Q.slot[k] = (uint32_t)(std::lower_bound(qcol.begin(), qcol.end(), all[k]) - qcol.begin());
    }
}

// The result tables.  tile_cnt [n_tiles][N]: every genome's residues per BB_CHUNK columns of the whole array; qcnt [Q.qcol.size()][N]:
// its residues between the tile start and the query column.  A segment is kept with the genomes that have bases in it, at least 2;
// order: interval, first column, genome set.  B.N is set, B.valid is the caller's
inline void bb_tables(int N, const std::vector<BbIv> &ivs, const std::vector<BbSeg> &segs, const std::vector<BbRec> &islands, const BbQueries &Q, const int64_t *left,
                      const int64_t *right, const int8_t *reverse, const uint32_t *tile_cnt, size_t n_tiles, const uint32_t *qcnt, BackboneResult &B)
{
    B = BackboneResult(); B.N = N;
    std::vector<int64_t> tile_pre((n_tiles + 1) * (size_t)N, 0);   // exclusive prefix of the tile counts
    for (size_t t = 0; t < n_tiles; t++) for (int g = 0; g < N; g++) tile_pre[(t + 1) * N + g] = tile_pre[t * N + g] + tile_cnt[t * N + g];
    auto count_at = [&](int64_t x, size_t k, int g) {                  // residues of g in columns [0, x) of the whole array; k = the query's slot
        if (!Q.slot.empty()) k = Q.slot[k];
        return tile_pre[(size_t)(x / BB_CHUNK) * N + g] + (int64_t)qcnt[k * N + g];
    };
    // signed ends of g's residues in columns [c1, c2] of interval d; kb, ka: the slots of the interval start and of c1 (c2 + 1 follows it)
    auto ends = [&](const BbIv &d, int g, int64_t c1, int64_t c2, size_t kb, size_t ka, int64_t *lo, int64_t *hi) {
        const int64_t base = count_at(d.col0, kb, g), k1 = count_at(d.col0 + c1, ka, g) - base, k2 = count_at(d.col0 + c2 + 1, ka + 1, g) - base - 1;
        if (k2 < k1) return false;
        const int64_t L = left[(int64_t)d.iv * N + g], R = right[(int64_t)d.iv * N + g];
        if (!reverse[(int64_t)d.iv * N + g]) { *lo = L + k1; *hi = L + k2; } else { *lo = -(R - k2); *hi = -(R - k1); }
        return true;
    };
    struct Row { int64_t iv, col, len; uint32_t mask; size_t at; };   // at: the row's ends in lo / hi
    std::vector<Row> rows; std::vector<int64_t> lo, hi;
    for (size_t si = 0; si < segs.size(); si++) {
        const BbSeg &s = segs[si];
        const BbIv &d = ivs[s.ivx];
        int64_t l[32] = {0}, h[32] = {0}; uint32_t got = 0;
        for (int g = 0; g < N; g++) if ((s.mask >> g & 1) && ends(d, g, s.c1, s.c2, s.ivx, Q.q_seg + 2 * si, &l[g], &h[g])) got |= 1u << g;
        if (__builtin_popcount(got) < 2) continue;
        rows.push_back(Row{(int64_t)d.iv, s.c1, s.c2 - s.c1 + 1, got, lo.size()});
        for (int g = 0; g < N; g++) { const bool in = got >> g & 1; lo.push_back(in ? l[g] : 0); hi.push_back(in ? h[g] : 0); }
    }
    auto before = [](const Row &x, const Row &y) { return x.iv != y.iv ? x.iv < y.iv : (x.col != y.col ? x.col < y.col : x.mask < y.mask); };
    if (!std::is_sorted(rows.begin(), rows.end(), before)) std::sort(rows.begin(), rows.end(), before);     // (the sweep hands them out nearly in this order already)
    for (const Row &r : rows) {
        B.seg_iv.push_back(r.iv); B.seg_col.push_back(r.col); B.seg_len.push_back(r.len); B.seg_mask.push_back(r.mask);
        B.seg_left.insert(B.seg_left.end(), lo.begin() + (std::ptrdiff_t)r.at, lo.begin() + (std::ptrdiff_t)(r.at + (size_t)N));
        B.seg_right.insert(B.seg_right.end(), hi.begin() + (std::ptrdiff_t)r.at, hi.begin() + (std::ptrdiff_t)(r.at + (size_t)N));
    }
    B.islands.reserve(islands.size() * 8);
    for (size_t k = 0; k < islands.size(); k++) {
        const BbRec &q = islands[k];
        const int who = (int)(q.packed >> 16 & 0xff);
        int64_t l = 0, h = 0;
        (void)ends(ivs[Q.isl_ivx[k]], who, q.c_first, q.c_last, Q.isl_ivx[k], Q.q_isl + 2 * k, &l, &h);
        const int64_t row[8] = {(int64_t)q.iv, (int64_t)(q.packed & 0xff), (int64_t)(q.packed >> 8 & 0xff), who, (int64_t)q.c_first, (int64_t)q.c_last, l, h};
        B.islands.insert(B.islands.end(), row, row + 8);
    }
}

// ---- S12b ----
constexpr int HOM_SEG = 4096;                     // columns per segment = 64 steps of 64 lanes
struct HomItem { uint32_t ivx, seg; uint8_t a, b; uint16_t pad; };                            // one wave's work: segment `seg` of interval ivx, pair (a, b)
struct HomIv { int64_t col0, ncols; uint32_t iv, nseg; uint32_t seg0, pad; };                  // seg0: the interval's first row in the per-segment tables
struct HomFn { int32_t t, lo, hi, pad; };                                                     // x -> clamp(x + t, lo, hi)
struct HomRun { uint32_t first, nseg; };          // the items of one (interval, pair): consecutive, segment order
struct HomWork { std::vector<HomIv> ivs; std::vector<HomItem> items; std::vector<HomRun> runs; int64_t residues = 0; uint32_t n_segs = 0; };

// work items: (interval with >= 2 genomes, pair, segment of 4096 columns).  lens: the genomes' lengths.  MAUVE_OK, or the error with its text in *err
inline int hom_work_items(int N, int64_t n_iv, const int64_t *left, const int64_t *right, const int64_t *col_off, const int64_t *lens, HomWork &W, const char **err)
{
    W = HomWork();
    for (int64_t iv = 0; iv < n_iv; iv++) {
        int g[MAUVE_MAX_SEQ], n = 0;
        for (int x = 0; x < N; x++) if (left[(size_t)(iv * N + x)]) {
            const int64_t l = left[(size_t)(iv * N + x)], r = right[(size_t)(iv * N + x)];
            if (l < 1 || r < l || r > lens[(size_t)x]) { *err = "apply_homology: an interval lies outside its genome"; return MAUVE_ERR_ARG; }
            g[n++] = x; W.residues += r - l + 1;
        }
        const int64_t nc = col_off[(size_t)iv + 1] - col_off[(size_t)iv];
        if (n < 2 || nc <= 0) continue;
        const int64_t nsg = (nc + HOM_SEG - 1) / HOM_SEG;
        if ((int64_t)W.n_segs + nsg > 0x7fffffff || (int64_t)W.items.size() + nsg * n * (n - 1) / 2 > 0x7fffffff) { *err = "apply_homology: too many segments"; return MAUVE_ERR_LIMIT; }
        W.ivs.push_back(HomIv{col_off[(size_t)iv], nc, (uint32_t)iv, (uint32_t)nsg, W.n_segs, 0u});
        W.n_segs += (uint32_t)nsg;
        for (int x = 0; x < n; x++) for (int y = x + 1; y < n; y++) {
            W.runs.push_back(HomRun{(uint32_t)W.items.size(), (uint32_t)nsg});
            for (int64_t sgi = 0; sgi < nsg; sgi++) W.items.push_back(HomItem{(uint32_t)(W.ivs.size() - 1), (uint32_t)sgi, (uint8_t)g[x], (uint8_t)g[y], 0});
        }
    }
    return MAUVE_OK;
}

// x at every segment start, and the final state of every run (x >= 0: H); the path starts in U: x below go_h
inline void hom_chain_forward(const std::vector<HomRun> &runs, const std::vector<HomFn> &fn, int32_t go_h, std::vector<int32_t> &xin, std::vector<uint8_t> &fin)
{
    xin.resize(fn.size()); fin.resize(runs.size());
    for (size_t r = 0; r < runs.size(); r++) {
        int64_t x = (int64_t)go_h - 1;
        for (uint32_t k = 0; k < runs[r].nseg; k++) {
            const HomFn &f = fn[runs[r].first + k];
            xin[runs[r].first + k] = (int32_t)x;
            x = std::min<int64_t>(std::max<int64_t>(x + f.t, f.lo), f.hi);
        }
        fin[r] = x >= 0;
    }
}

// state at every segment's last column, from the interval's end backwards (smap: bit s = the state in front of the segment when s is behind it)
inline void hom_chain_backward(const std::vector<HomRun> &runs, const std::vector<uint8_t> &smap, const std::vector<uint8_t> &fin, std::vector<uint8_t> &send)
{
    send.resize(smap.size());
    for (size_t r = 0; r < runs.size(); r++) {
        uint32_t e = fin[r];
        for (uint32_t k = runs[r].nseg; k-- > 0;) { send[runs[r].first + k] = (uint8_t)e; e = (smap[runs[r].first + k] >> e) & 1u; }
    }
}
