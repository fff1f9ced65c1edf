// Host check of the tile order of the tiled sort (mauvealigner_amd/csrc/tile_swz.hpp), plain g++, no device.
// For every tile count 1 .. 4200 and for 6104 and 54 200 (the seed pass's sort in C3 and C5): rs_swz is a permutation of 0 .. nblk - 1, every
// value is below nblk, and the tiles of each class b % 8 form one contiguous ascending range.  Prints "ok <counts>" or the first failure, exit 1.
#include "../../mauvealigner_amd/csrc/tile_swz.hpp"
#include <cstdio>
#include <vector>

static bool check(uint32_t nblk)
{
    std::vector<unsigned char> seen(nblk, 0);
    for (uint32_t b = 0; b < nblk; b++) {
        const uint32_t t = rs_swz(b, nblk);
        if (t >= nblk) { printf("FAIL nblk=%u: swz(%u) = %u is not below nblk\n", nblk, b, t); return false; }
        if (seen[t]) { printf("FAIL nblk=%u: tile %u taken twice (block %u)\n", nblk, t, b); return false; }
        seen[t] = 1;
        if (b >= 8 && t != rs_swz(b - 8, nblk) + 1) {
            printf("FAIL nblk=%u: class %u is not contiguous ascending at block %u (%u after %u)\n", nblk, b & 7u, b, t, rs_swz(b - 8, nblk));
            return false;
        }
    }
    // (nblk distinct values below nblk: a permutation)
    return true;
}

int main()
{
    int counts = 0;
    for (uint32_t nblk = 1; nblk <= 4200; nblk++, counts++)
        if (!check(nblk)) return 1;
    for (uint32_t nblk : {6104u, 54200u}) {
        if (!check(nblk)) return 1;
        counts++;
    }
    printf("ok %d tile counts\n", counts);
    return 0;
}
