// tile_swz.hpp -- the order in which the workgroups of the tiled sort (tiled_sort.hpp) take their tiles.
// Workgroups are dealt round-robin over the 8 XCDs, each with an L2 of its own: with tile = block, the tiles t and t + 1 -- whose runs
// of a digit share a cache line in the output, and whose counters share one in the histogram rows -- always sit behind different L2s,
// and the two partial writes of the line leave for memory unmerged.  rs_swz gives the blocks with equal b % 8 one contiguous ascending
// range of tiles, so neighbours in the output are neighbours in time behind one L2.  A bijection of 0 .. nblk - 1 for every nblk
// (classes below nblk % 8 hold one tile more); an ordering for speed only -- nothing may depend on which XCD a block runs on.
// Plain C++ as well as HIP: tests/cpp/swz_host_test.cpp checks it on the host.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define RS_SWZ_FN __host__ __device__ __forceinline__
#else
#define RS_SWZ_FN inline
#endif

RS_SWZ_FN uint32_t rs_swz(uint32_t b, uint32_t nblk)
{
    const uint32_t q = nblk >> 3, r = nblk & 7u, x = b & 7u;
    return x * q + (x < r ? x : r) + (b >> 3);
}
