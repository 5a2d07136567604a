// Stand-alone check of csrc/fast_entry.h (the two forms of fast_nms_kernel's candidate entries), built by
// tests/test_fast_entry_cpu.py with the address and undefined-behaviour sanitizers.  Phase 1's mapping is written out
// here on its own: lane tid holds dword column c = tid % 18 and first score row r0 = tid / 18; pixel px of the dword in
// pass it lies in score row r0 + 14 it, byte column 4 c + px, and is bit 8 px + it of the lane's masks.
#include <cstdio>
#include <set>
#include <vector>

#include "fast_entry.h"

int main()
{
    long n = 0, bad = 0;
    std::set<unsigned> seen_lane, seen_pixel;
    const unsigned sides[3] = {FAST_ENTRY_DARK, FAST_ENTRY_BRIGHT, FAST_ENTRY_DARK | FAST_ENTRY_BRIGHT};
    // offset / 72 as multiply and shift: every byte offset of the tile a lane can name
    for (unsigned off = 0; off < 70u * 72u; ++off) bad += fast_entry_row_of(off) != off / 72u;
    for (unsigned tid = 0; tid < 252; ++tid) {
        const unsigned r0 = tid / 18, c = tid % 18;
        for (unsigned it = 0; it < 5; ++it)
            for (unsigned px = 0; px < 4; ++px) {
                const unsigned want_ry = r0 + 14 * it, want_bx = 4 * c + px, bit = 8 * px + it;
                bad += fast_entry_bpos(it, px) != bit || bit >= 32;
                for (unsigned s : sides) {
                    const unsigned e = fast_entry_lane(fast_entry_lane_base(tid), bit, s);
                    ++n;
                    bad += e > 0xFFFFu;                                         // a list entry is 16 bits
                    bad += (e & FAST_ENTRY_SIDES) != s;                         // the side flags survive
                    unsigned ry = ~0u, bx = ~0u;
                    fast_entry_decode(e, ry, bx);
                    bad += ry != want_ry || bx != want_bx;
                    bad += fast_entry_offset(e) != 72 * want_ry + want_bx;
                    // the compact form round-trips, and the conversion keeps pixel and flags
                    const unsigned k = fast_entry_to_compact(e);
                    bad += k > 0xFFFFu || k != fast_entry_compact(want_ry, want_bx, s);
                    bad += fast_entry_compact_ry(k) != want_ry || fast_entry_compact_bx(k) != want_bx || (k & FAST_ENTRY_SIDES) != s;
                    if (s == FAST_ENTRY_DARK) {
                        bad += !seen_lane.insert(e).second;                     // all entries are distinct ...
                        bad += !seen_pixel.insert(72 * want_ry + want_bx).second;   // ... and so are the pixels they name
                    }
                }
            }
    }
    bad += seen_lane.size() != 252u * 20u;
    std::printf("%ld entries, %ld bad\n", n, bad);
    return bad != 0;
}
