"""Hand-made descriptor pairs for the one-pass crossCheck matcher (match_hamming_mfma_kernel elects the trains' nearest
queries down the columns of a 32 x 32 product tile and the queries' nearest trains along its rows, in the same pass).

A pair is random 256-bit rows with structures planted at fixed indices; a structure is planted only where all its indices
fit, so the small pairs keep what their sizes allow.  Train index j sits in column j % 32 of owner tile j // 32; wave
(j // 32) % 8 of round j // 256 owns that tile.  Query index i is row i % 32 of scanned tile i // 32.

  dup trains 3 | 19 | 35, query 7 at 3 bits from them: equal row entries at columns 3 and 19 of one tile (lanes 16 apart) and
      column 3 of the next tile (another wave); the lowest train, 3, must win the row.
  dup trains 40 | 41, 44 | 46, 48 | 52, 50 | 58, queries 8 .. 11 at 2 bits: ties between lanes 1, 2, 4 and 8 apart.
  dup trains 10 | 266 | 299, query 12: ties across rounds (tiles 0, 8 and 9).
  dup queries 5 | 21 | 37 | 261, train 150 at 4 bits: the train elects the lowest query, 5; the others choose train 150 too and
      are rejected.
  queries 13, 14, 290 at 2, 4 and 6 bits from train 200: a train three queries choose; it elects 13 alone.
  trains 210, 280 at 2 and 4 bits from query 30: two trains elect one query; it is matched to 210 and 280 stays single.
  all-zero query 0 | train 1 and all-one query 1 | train 0 (popcounts 0 and 256, distance 0); the all-zero query 2 and the
      all-one train 2 repeat them and lose the tie.

Everything else is random: nearest neighbours around 100 bits, some mutual and some not."""
import numpy as np

from tests import match_model as mm

MAX_MATCHES = 512
NFEATURES = 448                    # kcap = 512: two rounds of 8 owner tiles

# (n1, n2): partial last tiles on both sides; a second round of owners, both ways round; the full structure; empty sides; one row
SIZES = [(33, 65), (300, 40), (40, 300), (300, 300), (0, 40), (40, 0), (1, 1)]


def _flip(row, bits):
    out = row.copy()
    for b in bits:
        out[b >> 3] ^= np.uint8(1 << (b & 7))
    return out


def make(n1, n2, seed=0):
    """(desc1 u8[n1, 32], desc2 u8[n2, 32]) and the names of the structures that fitted"""
    rng = np.random.default_rng(1000 * n1 + n2 + 7 * seed)
    d1 = rng.integers(0, 256, (n1, 32), dtype=np.uint8); d2 = rng.integers(0, 256, (n2, 32), dtype=np.uint8)
    fitted = []

    def plant(name, queries, trains):
        """queries / trains: {index: row}"""
        if all(i < n1 for i in queries) and all(j < n2 for j in trains):
            for i, r in queries.items():
                d1[i] = r
            for j, r in trains.items():
                d2[j] = r
            fitted.append(name)

    if n1 == 1 and n2 == 1:
        d1[0] = 0; d2[0] = 255                                 # distance 256: the top of the key's distance field
        return d1, d2, ["far"]
    base = rng.integers(0, 256, (16, 32), dtype=np.uint8)
    plant("cols_3_19_35", {7: _flip(base[0], [0, 1, 2])}, {3: base[0], 19: base[0], 35: base[0]})
    for k, (a, b) in enumerate([(40, 41), (44, 46), (48, 52), (50, 58)]):
        plant(f"lanes_{b - a}_apart", {8 + k: _flip(base[1 + k], [5, 6])}, {a: base[1 + k], b: base[1 + k]})
    plant("rounds", {12: _flip(base[5], [9])}, {10: base[5], 266: base[5], 299: base[5]})
    plant("dup_queries", {i: base[6] for i in (5, 21, 37, 261)}, {150: _flip(base[6], [1, 2, 3, 4])})
    plant("dup_queries_small", {i: base[7] for i in (6, 22)}, {20: _flip(base[7], [1, 2, 3, 4])})
    plant("crowded_train", {13: _flip(base[8], [0, 1]), 14: _flip(base[8], [2, 3, 4, 5]), 290: _flip(base[8], range(6, 12))}, {200: base[8]})
    plant("crowded_train_small", {15: _flip(base[9], [0, 1]), 16: _flip(base[9], [2, 3, 4, 5])}, {21: base[9]})
    plant("two_electors", {30: base[10]}, {210: _flip(base[10], [0, 1]), 280: _flip(base[10], [3, 4, 5, 6])})
    plant("two_electors_small", {31: base[11]}, {22: _flip(base[11], [0, 1]), 38: _flip(base[11], [3, 4, 5, 6])})
    zeros = np.zeros(32, np.uint8); ones = np.full(32, 255, np.uint8)
    plant("weights", {0: zeros, 1: ones, 2: zeros}, {1: zeros, 0: ones, 2: ones})
    return d1, d2, fitted


def expected(d1, d2):
    return mm.match_hamming(d1, d2, MAX_MATCHES)


def all_pairs():
    """[(name, desc1, desc2)] over SIZES"""
    return [(f"{n1}x{n2}", *make(n1, n2)[:2]) for n1, n2 in SIZES]
