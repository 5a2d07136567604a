// Stand-alone check of csrc/buf_layout.h (where the pieces of a buffer set sit in its block), built by
// tests/test_buf_layout_cpu.py with the address and undefined-behaviour sanitizers.  Piece lists of 1 ... 20 entries with
// sizes from {0, 1, 255, 256, 257, 80 n, 2^33 + 1}: for every length the seven lists of one size each, and LISTS_PER_LENGTH
// lists drawn by a fixed generator.  The expected sums are kept here on their own, in 128 bits.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "buf_layout.h"

static_assert(sizeof(size_t) == 8, "the layout is 64-bit arithmetic");
constexpr int LISTS_PER_LENGTH = 500;
constexpr size_t HUGE_PIECE = ((size_t)1 << 33) + 1;

static uint64_t rng = 0x9E3779B97F4A7C15ull;
static unsigned draw(unsigned n) { rng = rng * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)((rng >> 33) % n); }

static size_t size_of_kind(unsigned kind)
{
    const size_t fixed[6] = {0, 1, 255, 256, 257, HUGE_PIECE};
    return kind < 6 ? fixed[kind] : 80 * (size_t)(1 + draw(100000));       // 80 n: the track-point record
}

static long check(const std::vector<size_t> &bytes)
{
    long bad = 0;
    RpeBufLayout lay;
    unsigned __int128 sum = 0;           // of the aligned sizes so far
    bool huge = false;
    for (size_t b : bytes) {
        const size_t off = lay.place(b);
        if (b == 0) { bad += off != RPE_BUF_NONE; continue; }              // flagged null, and takes no room
        bad += off == RPE_BUF_NONE || off % 256 != 0;
        bad += (unsigned __int128)off != sum;                               // in order, right behind the pieces before it ...
        sum += ((unsigned __int128)(b >> 8) + ((b & 255) != 0)) << 8;
        bad += (unsigned __int128)off + b > sum;                            // ... and inside its own aligned room: no overlap
        bad += (unsigned __int128)lay.end != sum;
        huge = huge || b == HUGE_PIECE;
    }
    const unsigned __int128 want = sum < 256 ? 256 : sum;
    bad += (unsigned __int128)lay.total() != want || lay.total() < 256;
    bad += huge && lay.total() <= ((size_t)1 << 33);                        // did not wrap at 32 bits
    return bad;
}

int main()
{
    long lists = 0, bad = 0;
    for (size_t len = 1; len <= 20; ++len) {
        for (unsigned kind = 0; kind < 7; ++kind, ++lists) bad += check(std::vector<size_t>(len, size_of_kind(kind)));
        for (int k = 0; k < LISTS_PER_LENGTH; ++k, ++lists) {
            std::vector<size_t> bytes(len);
            for (size_t &b : bytes) b = size_of_kind(draw(7));
            bad += check(bytes);
        }
    }
    // the empty list and the all-zero list still make a block
    bad += RpeBufLayout().total() != 256;
    std::printf("%ld lists, %ld bad\n", lists, bad);
    return bad != 0;
}
