// Stand-alone check of csrc/orb_groups.h (the level groups of ORB detection), built by tests/test_orb_groups_cpu.py, also
// with the address and undefined-behaviour sanitizers.  For image sizes from 63 x 63 (one FAST tile) to 4095 x 4095
// (the largest rpe_create accepts) -- every size up to 200, then steps of 37, and the limit -- and G = 1 .. 4: the groups
// are consecutive level ranges that cover the twelve levels, so every level is in exactly one; their tile ranges follow
// each other from 0 to the end of the tile table and hold exactly their levels' tiles; an empty group has no level and no
// tile; no group exceeds an equal share by more than the largest level's tiles.  The level sizes and tile counts are
// computed here on their own (orb.cpp's level sizes; the 64 x 64 tiles of [28, w - 31) x [31, h - 31)).
#include <cmath>
#include <cstdio>
#include <vector>

#include "orb_groups.h"

constexpr int NLEVELS = 12, EDGE = 31, TILE_X0 = 28, MAX_DIM = 4095;

static int fast_tiles(int w, int h)
{
    if (w <= 2 * EDGE || h <= 2 * EDGE) return 0;
    return ((h - 2 * EDGE + 63) / 64) * ((w - EDGE - TILE_X0 + 63) / 64);
}

static void level_tiles(int W, int H, int *ntile)
{
    for (int l = 0; l < NLEVELS; ++l) {
        const float inv = 1.0f / (float)std::pow((double)1.1f, (double)l);
        ntile[l] = fast_tiles((int)std::lrint((double)((float)W * inv)), (int)std::lrint((double)((float)H * inv)));
    }
}

static long check(const int *ntile, int G, long &empty_groups)
{
    long bad = 0;
    RpeOrbGroup grp[RPE_ORB_GROUP_MAX + 2];
    const RpeOrbGroup guard = {-7, -7, -7, -7};
    grp[0] = guard; grp[G + 1] = guard;                        // nothing is written outside [0, G)
    RpeOrbGroup *g = grp + 1;
    rpe_orb_groups(ntile, NLEVELS, G, g);
    bad += grp[0].l0 != -7 || grp[0].nt != -7 || grp[G + 1].l0 != -7 || grp[G + 1].nt != -7;
    int total = 0, biggest = 0, tile0[NLEVELS + 1];
    for (int l = 0; l < NLEVELS; ++l) { tile0[l] = total; total += ntile[l]; biggest = ntile[l] > biggest ? ntile[l] : biggest; }
    tile0[NLEVELS] = total;
    int member[NLEVELS] = {};
    bad += g[0].l0 != 0 || g[0].t0 != 0 || g[G - 1].l1 != NLEVELS;
    for (int k = 0; k < G; ++k) {
        bad += g[k].l0 < 0 || g[k].l1 < g[k].l0 || g[k].l1 > NLEVELS;
        if (bad) return bad;
        if (k + 1 < G) bad += g[k + 1].l0 != g[k].l1 || g[k + 1].t0 != g[k].t0 + g[k].nt;      // consecutive, no gap, no overlap
        bad += g[k].t0 != tile0[g[k].l0] || g[k].nt != tile0[g[k].l1] - tile0[g[k].l0];     // exactly its levels' tiles
        for (int l = g[k].l0; l < g[k].l1; ++l) ++member[l];
        if (g[k].l0 == g[k].l1) { bad += g[k].nt != 0; ++empty_groups; }
        bad += (long long)g[k].nt * G > (long long)total + (long long)biggest * G;           // about an equal share
    }
    bad += g[G - 1].t0 + g[G - 1].nt != total;
    for (int l = 0; l < NLEVELS; ++l) bad += member[l] != 1;
    return bad;
}

int main()
{
    std::vector<int> dims;
    for (int d = 63; d <= 200; ++d) dims.push_back(d);
    for (int d = 237; d < MAX_DIM; d += 37) dims.push_back(d);
    dims.push_back(MAX_DIM);
    long cases = 0, bad = 0, empty_groups = 0;
    for (int W : dims)
        for (int H : dims) {
            int ntile[NLEVELS];
            level_tiles(W, H, ntile);
            for (int G = 1; G <= RPE_ORB_GROUP_MAX; ++G, ++cases) bad += check(ntile, G, empty_groups);
        }
    bad += empty_groups == 0;                                  // the sweep did reach empty groups
    // hand-made tables: one level holds nearly everything (its neighbours' groups stay empty), holes between live levels,
    // no tile at all
    const int lopsided[NLEVELS] = {1000, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0}, holes[NLEVELS] = {5, 0, 5, 0, 0, 5, 0, 5, 0, 0, 0, 1};
    const int dead[NLEVELS] = {};
    for (int G = 1; G <= RPE_ORB_GROUP_MAX; ++G, cases += 3)
        bad += check(lopsided, G, empty_groups) + check(holes, G, empty_groups) + check(dead, G, empty_groups);
    std::printf("%ld cases, %ld bad\n", cases, bad);
    return bad != 0;
}
