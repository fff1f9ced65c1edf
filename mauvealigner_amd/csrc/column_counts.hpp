// column_counts.hpp -- what the stages that count residues in the column array share (aln_view.hip, backbone_dev.hip, homology_dev.hip):
// the tile they count by (plain C++: backbone_host.hpp includes this file from host-only programs) and two device helpers.
#pragma once
#include <cstdint>

constexpr int BB_CHUNK = 4096;            // columns per chunk / per count tile

#ifdef __HIPCC__
// the lanes below p
__device__ __forceinline__ uint64_t below(int p) { return p >= 64 ? ~0ull : (1ull << p) - 1; }

// v: this lane's column of a 64-column word; mine: lane g's count of genome g's residues so far, g < N.  -> mine with the word added
// (every lane of the wave must call.  The running count goes in and out by value: handed over by reference, or added by the caller
// to a returned count, the loop compiles to more instructions than the four copies it replaces did)
__device__ __forceinline__ uint32_t wave_genome_counts(uint32_t v, int N, int lane, uint32_t mine)
{
    for (int g = 0; g < N; g++) { const uint32_t x = (uint32_t)__popcll(__ballot(v >> g & 1)); if (lane == g) mine += x; }
    return mine;
}
#endif
