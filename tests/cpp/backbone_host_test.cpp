// backbone_host_test.cpp -- the host steps of the backbone stage and of the homology pass (csrc/backbone_host.hpp) without a GPU.
//
//   backbone_host_test tables FILE OUT
//     FILE: an alignment with island_gap and the threshold of the unique path (read_alignment).  What the kernels of backbone_dev.hip
//     would hand the host is made by the plainest column walk straight from the rule of DESIGN.md S12 -- region and island records
//     (appended in a shuffled order), per-tile counts, per-query counts -- and goes through
//     bb_sort_records, bb_sweep, bb_query_slots and bb_tables.  The tables go to OUT (the query slots and the queries made, then the
//     seven tables, each as its length and its int64 entries); tests/test_backbone_host_cpu.py compares them with the oracle's.
//   backbone_host_test chains
//     hom_chain_forward / hom_chain_backward on random runs of 1, 2 and 65 segments of random columns, identities included, against a
//     column-by-column evaluation.  Prints OK.
//
// Host-only C++ (g++ -fsanitize=address,undefined), stand-alone.
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <thread>

#include "backbone_host.hpp"

#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #x); std::exit(1); } } while (0)

namespace {

struct Alignment { int N = 0; int64_t n_iv = 0, island_gap = 0; size_t dedupe_above = 0; std::vector<int64_t> left, right, col_off; std::vector<int8_t> reverse; std::vector<uint32_t> cols; };

// FILE: raw int64 words -- N, n_iv, island_gap, dedupe_above, left[n_iv][N], right[n_iv][N], reverse[n_iv][N], col_off[n_iv + 1] --
// then the columns as uint32
Alignment read_alignment(const char *path)
{
    std::FILE *f = std::fopen(path, "rb");
    CHECK(f);
    Alignment A; int64_t h[4];
    CHECK(std::fread(h, 8, 4, f) == 4 && h[0] >= 1 && h[0] <= 32 && h[1] >= 0 && h[2] >= 0 && h[3] >= 0);
    A.N = (int)h[0]; A.n_iv = h[1]; A.island_gap = h[2]; A.dedupe_above = (size_t)h[3];
    const size_t n = (size_t)A.n_iv * A.N;
    std::vector<int64_t> rev(n);
    A.left.resize(n); A.right.resize(n); A.col_off.resize((size_t)A.n_iv + 1);
    CHECK(std::fread(A.left.data(), 8, n, f) == n && std::fread(A.right.data(), 8, n, f) == n && std::fread(rev.data(), 8, n, f) == n);
    CHECK(std::fread(A.col_off.data(), 8, A.col_off.size(), f) == A.col_off.size() && A.col_off[0] == 0);
    A.reverse.assign(rev.begin(), rev.end());
    A.cols.resize((size_t)A.col_off[(size_t)A.n_iv]);
    CHECK(std::fread(A.cols.data(), 4, A.cols.size(), f) == A.cols.size());
    std::fclose(f);
    return A;
}

// S12, one pair of one interval, column by column: a gap run is a maximal stretch of only-a or of only-b columns (neither-columns are
// skipped), an island when it has more than island_gap of them; a gap region is a maximal stretch without a both-column, open when it
// holds an island or touches the first / last column the pair has.  Open regions and islands are what bb_pair_gaps reports
void walk_pair(const Alignment &A, const BbIv &d, int a, int b, std::vector<BbRec> &recs)
{
    auto emit = [&](uint32_t kind, uint32_t who, int64_t c0, int64_t c1) {
        recs.push_back(BbRec{d.iv, (uint32_t)a | (uint32_t)b << 8 | who << 16 | kind << 24, (uint32_t)c0, (uint32_t)c1});
    };
    bool seen_both = false, in_region = false, leading = false, has_island = false;
    int run_of = 0;                                           // 1: only a, 2: only b
    int64_t first = 0, last = 0, run_first = 0, run_last = 0, run_n = 0;
    auto close_run = [&]() { if (run_n > A.island_gap) { has_island = true; emit(1u, (uint32_t)(run_of == 1 ? a : b), run_first, run_last); } };
    for (int64_t c = 0; c < d.ncols; c++) {
        const uint32_t m = A.cols[(size_t)(d.col0 + c)];
        const bool ra = m >> a & 1, rb = m >> b & 1;
        if (!ra && !rb) continue;
        if (ra && rb) {
            if (in_region) { close_run(); if (has_island || leading) emit(0u, 0u, first, last); in_region = false; }
            seen_both = true;
            continue;
        }
        const int of = ra ? 1 : 2;
        if (!in_region) { in_region = true; leading = !seen_both; has_island = false; first = c; run_of = of; run_first = c; run_n = 0; }
        else if (of != run_of) { close_run(); run_of = of; run_first = c; run_n = 0; }
        run_n++; run_last = last = c;
    }
    if (in_region) { close_run(); emit(0u, 0u, first, last); }
}

// a table to OUT: its length, then its int64 entries
void put(std::FILE *f, const std::vector<int64_t> &v) { const int64_t n = (int64_t)v.size(); CHECK(std::fwrite(&n, 8, 1, f) == 1 && (v.empty() || std::fwrite(v.data(), 8, v.size(), f) == v.size())); }

int tables(const char *path, const char *out_path)
{
    const Alignment A = read_alignment(path);
    const int N = A.N;
    std::vector<BbIv> ivs; uint32_t chunks = 0, max_pairs = 0;
    CHECK(bb_intervals(N, A.n_iv, A.left.data(), A.col_off.data(), ivs, &chunks, &max_pairs));
    // what the kernels produce: records in no particular order, tile counts
    // (the pairs are independent: a few threads share them out, only to keep the largest case short)
    struct Job { const BbIv *d; int a, b; };
    std::vector<Job> jobs;
    for (const BbIv &d : ivs)
        for (int a = 0; a < N; a++) for (int b = a + 1; b < N; b++) if ((d.gmask >> a & 1) && (d.gmask >> b & 1)) jobs.push_back(Job{&d, a, b});
    const size_t n_threads = std::min<size_t>(16, std::max<size_t>(1, std::thread::hardware_concurrency()));
    std::vector<std::vector<BbRec>> part(n_threads);
    std::atomic<size_t> next{0};
    std::vector<std::thread> pool;
    for (size_t t = 0; t < n_threads; t++)
        pool.emplace_back([&, t]() { for (size_t j; (j = next++) < jobs.size();) walk_pair(A, *jobs[j].d, jobs[j].a, jobs[j].b, part[t]); });
    for (std::thread &th : pool) th.join();
    std::vector<BbRec> recs;
    for (const std::vector<BbRec> &v : part) recs.insert(recs.end(), v.begin(), v.end());
    std::mt19937 rng(12345);
    std::shuffle(recs.begin(), recs.end(), rng);
    const size_t n_cols = A.cols.size(), n_tiles = (n_cols + BB_CHUNK - 1) / BB_CHUNK;
    std::vector<uint32_t> tile_cnt(n_tiles * (size_t)N, 0);
    for (size_t c = 0; c < n_cols; c++) for (uint32_t m = A.cols[c]; m; m &= m - 1) tile_cnt[c / BB_CHUNK * N + (size_t)__builtin_ctz(m)]++;
    // the host steps
    std::vector<BbSeg> segs; std::vector<BbRec> islands; BbQueries Q; BackboneResult B;
    bb_sort_records(recs);
    bb_sweep(ivs, recs, segs, islands);
    bb_query_slots(ivs, segs, islands, A.dedupe_above, Q);
    const size_t n_slots = ivs.size() + 2 * (segs.size() + islands.size());
    CHECK(Q.slot.empty() ? Q.qcol.size() == n_slots : (Q.slot.size() == n_slots && Q.qcol.size() <= n_slots));
    // bb_rank: every genome's residues between the tile start and the query column -- one walk over the columns with counts that start
    // again at every tile, handed to the queries in column order
    std::vector<uint32_t> qcnt(Q.qcol.size() * (size_t)N + 1, 0), order(Q.qcol.size());
    for (size_t q = 0; q < order.size(); q++) order[q] = (uint32_t)q;
    std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return Q.qcol[x] < Q.qcol[y]; });
    std::vector<uint32_t> run((size_t)N, 0);
    size_t qi = 0;
    for (size_t c = 0; c <= n_cols; c++) {
        if (c % BB_CHUNK == 0) run.assign((size_t)N, 0);
        for (; qi < order.size() && Q.qcol[order[qi]] == (int64_t)c; qi++) std::copy(run.begin(), run.end(), qcnt.begin() + (std::ptrdiff_t)((size_t)order[qi] * N));
        if (c < n_cols) for (uint32_t m = A.cols[c]; m; m &= m - 1) run[(size_t)__builtin_ctz(m)]++;
    }
    CHECK(qi == order.size());
    bb_tables(N, ivs, segs, islands, Q, A.left.data(), A.right.data(), A.reverse.data(), tile_cnt.data(), n_tiles, qcnt.data(), B);
    CHECK(B.N == N && B.seg_left.size() == B.seg_iv.size() * (size_t)N && B.islands.size() == islands.size() * 8);
    std::FILE *f = std::fopen(out_path, "wb");
    CHECK(f);
    put(f, {(int64_t)n_slots, (int64_t)Q.qcol.size()});
    put(f, B.seg_iv); put(f, B.seg_col); put(f, B.seg_len); put(f, std::vector<int64_t>(B.seg_mask.begin(), B.seg_mask.end()));
    put(f, B.seg_left); put(f, B.seg_right); put(f, B.islands);
    CHECK(std::fclose(f) == 0);
    std::printf("OK\n");
    return 0;
}

// ---- the homology chaining ----
constexpr int32_t MINF = -(1 << 30), PINF = 1 << 30;
int64_t clamp64(int64_t x, int64_t lo, int64_t hi) { return x < lo ? lo : (x > hi ? hi : x); }
// g after f, as the kernels compose (hom_compose): two identities stay the identity
HomFn after(const HomFn &g, const HomFn &f)
{
    HomFn r{f.t + g.t, (int32_t)clamp64((int64_t)f.lo + g.t, g.lo, g.hi), (int32_t)clamp64((int64_t)f.hi + g.t, g.lo, g.hi), 0};
    if (f.lo == MINF && g.lo == MINF) r.lo = MINF;
    if (f.hi == PINF && g.hi == PINF) r.hi = PINF;
    return r;
}

int chains()
{
    std::mt19937 rng(2024);
    const int32_t go_h = -3000, go_u = -5000;
    size_t flips = 0, ends_h = 0, n_runs = 0;
    for (int round = 0; round < 40; round++) {
        // a batch of runs of 1, 2 and 65 segments, every segment a few columns: x -> clamp(x + s, go_h + s, -go_u + s), or the identity
        std::vector<HomRun> runs; std::vector<std::vector<HomFn>> seg_cols;
        for (uint32_t nseg : {1u, 2u, 65u, 2u, 1u}) {
            runs.push_back(HomRun{(uint32_t)seg_cols.size(), nseg});
            const int mood = (int)(rng() % 3);                                 // scores drift up, down, or either way: the state changes inside some runs
            for (uint32_t k = 0; k < nseg; k++) {
                std::vector<HomFn> cs(1 + rng() % 9);
                for (HomFn &f : cs) {
                    if (rng() % 10 < 3) { f = HomFn{0, MINF, PINF, 0}; continue; }
                    const int32_t s = (int32_t)(rng() % 2101) - (mood == 0 ? 700 : (mood == 1 ? 1400 : 1050));
                    f = HomFn{s, go_h + s, -go_u + s, 0};
                }
                seg_cols.push_back(cs);
            }
        }
        const size_t n_items = seg_cols.size();
        // forwards: the segments' functions as hom_fn leaves them
        std::vector<HomFn> fn(n_items);
        for (size_t i = 0; i < n_items; i++) { HomFn f{0, MINF, PINF, 0}; for (const HomFn &col : seg_cols[i]) f = after(col, f); fn[i] = f; }
        std::vector<int32_t> xin; std::vector<uint8_t> fin, send;
        hom_chain_forward(runs, fn, go_h, xin, fin);
        CHECK(xin.size() == n_items && fin.size() == runs.size());
        // column by column: x in front of every column, then the states from the last column backwards
        std::vector<uint8_t> smap(n_items), want_send(n_items);
        for (size_t r = 0; r < runs.size(); r++) {
            int64_t x = (int64_t)go_h - 1;
            std::vector<std::vector<uint32_t>> maps(runs[r].nseg);             // per column: bit s = the state in front of it when s is behind it
            for (uint32_t k = 0; k < runs[r].nseg; k++) {
                const size_t i = runs[r].first + k;
                CHECK(xin[i] == x);
                for (const HomFn &col : seg_cols[i]) {
                    const bool none = col.lo == MINF && col.hi == PINF, ph = none || x >= go_h, pu = none || x <= -(int64_t)go_u;
                    maps[k].push_back((ph ? 2u : 0u) | (pu ? 0u : 1u));
                    x = clamp64(x + col.t, col.lo, col.hi);
                }
                uint32_t m = 0;                                                // the segment's map, as hom_pred leaves it: its columns from the last to the first
                for (uint32_t e = 0; e < 2; e++) { uint32_t st = e; for (size_t q = maps[k].size(); q-- > 0;) st = maps[k][q] >> st & 1u; m |= st << e; }
                smap[i] = (uint8_t)m;
            }
            CHECK(fin[r] == (x >= 0 ? 1 : 0));
            uint32_t st = fin[r]; ends_h += st; n_runs++;
            for (uint32_t k = runs[r].nseg; k-- > 0;) {
                want_send[runs[r].first + k] = (uint8_t)st;
                for (size_t q = maps[k].size(); q-- > 0;) { const uint32_t before = maps[k][q] >> st & 1u; flips += before != st; st = before; }
            }
        }
        hom_chain_backward(runs, smap, fin, send);
        CHECK(send == want_send);
    }
    CHECK(flips > 20 && ends_h > 10 && ends_h + 10 < n_runs);                  // the cases are not all one state
    std::printf("OK\n");
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc == 4 && std::string(argv[1]) == "tables") return tables(argv[2], argv[3]);
    if (argc == 2 && std::string(argv[1]) == "chains") return chains();
    std::fprintf(stderr, "usage: backbone_host_test tables FILE OUT | chains\n");
    return 2;
}
