// orb_groups.h -- the level groups of ORB detection (host-compilable: tests/native/orb_groups_host.cpp).
// A large batch runs fast_nms_kernel once per group of pyramid levels instead of once per handle: that of the first
// group beside the resize of the levels above it, and the selection chain of a finished group (raster_corners,
// retain_fast, harris, retain_harris) beside the FAST launch of the next group, each on a second stream (run_orb,
// rpe_api.hip).  FAST of a level reads that level alone, a level's chain only what FAST wrote for that level, every
// chain kernel is keyed by (level, image) workgroups and the levels' buffers are disjoint, so a group is a level range
// [l0, l1) for the chain and the tile range [t0, t0 + nt) of the FAST tile table for FAST.
#pragma once

#define RPE_ORB_GROUP_MAX 4            // the most groups rpe_orb_groups cuts

struct RpeOrbGroup { int l0, l1, t0, nt; };   // levels [l0, l1), FAST tiles [t0, t0 + nt)

// The one rule.  ntile[l] = FAST tiles of level l (RpeLevel::ntile, levels laid out one after the other in the tile
// table).  Cuts the levels into G consecutive groups of about equal tile count: level l goes to the group that the
// midpoint of its tile run falls into when the whole table is cut into G equal parts, and a level without tiles (the
// dead upper levels of a small image) to the group of the level before it.  Midpoints ascend with the level, so the
// groups are consecutive; every level is in exactly one of them; the tile ranges follow each other from 0 to the
// table's end.  A group may be empty (l0 == l1, nt == 0) -- one level holding most of the tiles leaves its neighbours
// nothing -- and the launchers skip it.
static inline void rpe_orb_groups(const int *ntile, int nlevels, int G, RpeOrbGroup *out)
{
    long long total = 0;
    for (int l = 0; l < nlevels; ++l) total += ntile[l];
    long long before = 0;
    int l = 0;
    for (int g = 0; g < G; ++g) {
        out[g].l0 = l; out[g].t0 = (int)before; out[g].nt = 0;
        // group of a level with tiles: floor(G (before + ntile / 2) / total) < G, in halves to stay in integers
        for (; l < nlevels && !(ntile[l] > 0 && (2 * before + ntile[l]) * G / (2 * total) > g); ++l) {
            out[g].nt += ntile[l];
            before += ntile[l];
        }
        out[g].l1 = l;
    }
}
