// Candidate-list entries of fast_nms_kernel (orb_kernels.hip), 16 bits each, in their two forms.  Plain C++ so that the
// host test (tests/test_fast_entry_cpu.py) compiles the very functions the kernel runs.
//
// Phase 1 appends entries in LANE form: what the appending lane has in registers anyway,
//     (tid << 5) | bpos | side flags
// tid  = the lane of the workgroup (< FAST_LANES = 252): dword column c = tid % 18, first score row r0 = tid / 18
// bpos = the bit of the lane's candidate masks: pixel px (0..3) of the lane's dword in pass it (0..4) is bit 8 px + it
//        (a row's four flags are bit 7 of four bytes and drop into place with one shift and one v_bfi / v_and_or)
// so a trip of the append loop is find-first-set, clear the bit, or it into the lane's constant, store.
// The score row is ry = r0 + 14 it, the byte column bx = 4 c + px, and because 72 r0 + 4 c = 4 tid the byte offset of the
// pixel in a 72-byte-pitch tile is  72 ry + bx = (4 tid + px) + 1008 it = bits 3..12 of the entry + 1008 x bits 0..2:
// phase 2 addresses pixels and scores without a division.
//
// A corner that phase 2 keeps is written back in COMPACT form, (ry << 7) | bx | side flags, which is what phase 3 reads.
// Both forms keep the side flags in bits 14 and 15.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FAST_ENTRY_HD __host__ __device__ __forceinline__
#else
#define FAST_ENTRY_HD inline
#endif

constexpr int FAST_ENTRY_NRP = 14;                  // score rows between two passes of a lane
constexpr int FAST_ENTRY_NCOL = 18;                 // dword columns of a tile row
constexpr int FAST_ENTRY_LANES = FAST_ENTRY_NRP * FAST_ENTRY_NCOL;
constexpr int FAST_ENTRY_NPASS = 5;
constexpr int FAST_ENTRY_PITCH = 4 * FAST_ENTRY_NCOL;                   // bytes of a tile row
constexpr unsigned FAST_ENTRY_DARK = 0x4000u, FAST_ENTRY_BRIGHT = 0x8000u, FAST_ENTRY_SIDES = 0xC000u;
constexpr int FAST_ENTRY_TID_SHIFT = 5;
static_assert(8 * 3 + (FAST_ENTRY_NPASS - 1) < (1 << FAST_ENTRY_TID_SHIFT), "bpos = 8 px + it fits the 5 bits below tid");
static_assert(((FAST_ENTRY_LANES - 1) << FAST_ENTRY_TID_SHIFT | 31) < (int)FAST_ENTRY_DARK, "tid and bpos stay below the side flags");
static_assert(FAST_ENTRY_NRP * (FAST_ENTRY_NPASS - 1) + FAST_ENTRY_NRP - 1 < 128 && FAST_ENTRY_PITCH <= 128, "ry and bx fit 7 bits each");
static_assert(FAST_ENTRY_LANES * FAST_ENTRY_PITCH / FAST_ENTRY_NCOL == FAST_ENTRY_NRP * FAST_ENTRY_PITCH, "a pass is 14 tile rows = 1008 bytes");

// ---- lane form
FAST_ENTRY_HD unsigned fast_entry_lane_base(unsigned tid) { return tid << FAST_ENTRY_TID_SHIFT; }
FAST_ENTRY_HD unsigned fast_entry_bpos(unsigned it, unsigned px) { return 8u * px + it; }
FAST_ENTRY_HD unsigned fast_entry_lane(unsigned lane_base, unsigned bpos, unsigned sides) { return lane_base | bpos | sides; }
// byte offset 72 ry + bx of the entry's pixel in a 72-byte-pitch tile whose row 0 is score row 0
FAST_ENTRY_HD unsigned fast_entry_offset(unsigned e) { return ((e >> 3) & 0x3FFu) + (unsigned)(FAST_ENTRY_NRP * FAST_ENTRY_PITCH) * (e & 7u); }
// score row of a byte offset: offset / 72 as multiply and shift, exact for every offset a tile holds (< 70 x 72; checked
// exhaustively by the host test), and what is left is the byte column
FAST_ENTRY_HD unsigned fast_entry_row_of(unsigned off) { return (off * 14564u) >> 20; }
FAST_ENTRY_HD void fast_entry_decode(unsigned e, unsigned &ry, unsigned &bx)
{
    const unsigned off = fast_entry_offset(e);
    ry = fast_entry_row_of(off);
    bx = off - (unsigned)FAST_ENTRY_PITCH * ry;
}

// ---- compact form
FAST_ENTRY_HD unsigned fast_entry_compact(unsigned ry, unsigned bx, unsigned sides) { return (ry << 7) | bx | sides; }
FAST_ENTRY_HD unsigned fast_entry_compact_ry(unsigned e) { return (e >> 7) & 127u; }
FAST_ENTRY_HD unsigned fast_entry_compact_bx(unsigned e) { return e & 127u; }
// lane form -> compact form, the side flags kept
FAST_ENTRY_HD unsigned fast_entry_to_compact(unsigned e)
{
    unsigned ry, bx;
    fast_entry_decode(e, ry, bx);
    return fast_entry_compact(ry, bx, e & FAST_ENTRY_SIDES);
}
