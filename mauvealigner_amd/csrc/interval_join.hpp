// interval_join.hpp -- the pieces of the interval-overlap join that more than one stage uses: feature_dev.hip, which owns
// the join (mauve_range_overlaps), and repeat_score_dev.hip, which stabs the component extents of a repeat map with it (S22).
//   fo_keys   the table as (genome << 31 | lo, table index) pairs, the entries checked; sorted by the project's sort
//   FoHi      the sorted table's hi under its genome: its running maximum (dev_scan.hpp, vmax) is the prefix maximum of hi inside every
//             genome's slice
// and the host steps both share: fm_put (host arrays on their way to the device) and fm_flag_result (the flag word with FM_LIMIT).
#pragma once
#include "common.hpp"
#include "coord_index.hpp"
#include <cstring>
#include <string>

namespace {

constexpr uint32_t FM_LIMIT = 4u;                 // the third bit of the flag word: a position of 2^31 or more
constexpr int64_t FM_MAX_POS = (int64_t)1 << 31, FM_MAX_N = (int64_t)1 << 24;
constexpr int FO_KEY_BITS = 31 + 5;               // position, genome id
static_assert(MAUVE_MAX_SEQ <= 32, "the join's sort key keeps the genome id in 5 bits");
constexpr unsigned long long FO_POS = 0x7fffffffull;

__global__ void __launch_bounds__(256) fo_keys(int64_t m, const int32_t *__restrict__ seq, const int64_t *__restrict__ lo, const int64_t *__restrict__ hi,
                                               unsigned long long *__restrict__ keys, uint32_t *__restrict__ vals, uint32_t *__restrict__ flag)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= m) return;
    const int64_t s = seq[t], a = lo[t], b = hi[t];
    unsigned long long k = 0; uint32_t bad = 0;
    if (s < 0 || s >= MAUVE_MAX_SEQ || a < 1 || a > b) bad = CO_BAD_ARG;
    else if (b >= FM_MAX_POS) bad = FM_LIMIT;
    else k = (unsigned long long)s << 31 | (unsigned long long)a;
    keys[t] = k; vals[t] = (uint32_t)t;
    if (bad) atomicOr(flag, bad);
}

// the sorted table's hi under its genome: the running maximum of this is the prefix maximum of hi inside every genome's slice
struct FoHi {
    const unsigned long long *keys; const uint32_t *vals; const int64_t *hi;
    __device__ unsigned long long value(uint32_t k) const { return (keys[k] & ~FO_POS) | ((unsigned long long)hi[vals[k]] & FO_POS); }
};

// host arrays on their way to the device: page-locked ones directly, pageable ones through the staging, where *used counts what is taken
int fm_put(mauve_ctx *c, void *dst, const void *src, size_t bytes, bool direct, size_t *used)
{
    if (!bytes) return MAUVE_OK;
    if (!direct) { char *h = c->pin_stage.as<char>() + *used; memcpy(h, src, bytes); src = h; *used += up64(bytes); }
    HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    return MAUVE_OK;
}

// the flag word of a stage of this file -> the result of its call
int fm_flag_result(mauve_ctx *c, uint32_t f, const char *who, const char *outside)
{
    if (!(f & CO_BAD_ARG) && (f & FM_LIMIT)) { c->err = std::string(who) + ": a position of 2^31 or more"; return MAUVE_ERR_LIMIT; }
    return co_flag_result(c, f, who, outside);
}

}  // namespace
