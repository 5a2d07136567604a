"""The brute-force matcher kernels against the NumPy model (tests/match_model.py) on the cases of tests/match_cases.py,
through the C-ABI stage calls rpe_match_hamming and rpe_match_l2: n_matches, qidx, tidx and dist bit for bit.  Every
operation is exact-integer or correctly-rounded float32, so nothing here has a tolerance.

One engine per launch form, at 96 x 96 (the smallest legal image; only the keypoint capacity kcap = nfeatures + 64
matters to a matcher).  Each test recomputes the launcher's arithmetic (rpe_launch_match, rpe_launch_match_l2 in
csrc/match_kernels.hip) from e.kcap and the batch size and asserts the form it means to reach: a change of the dispatch
rule fails here instead of silently moving a case to another kernel."""
import numpy as np
import pytest

from tests import match_cases as mc

pytestmark = pytest.mark.gpu

SPLIT_PAIRS = 64          # RPE_MATCH_SPLIT_PAIRS
QTILE, L2_QTILE = 1024, 256


@pytest.fixture(scope="module")
def capi():
    from relative_pose_estimation_amd import _capi
    assert _capi.load().rpe_device_count() > 0, "no HIP device visible"
    return _capi


def _engine(capi, list_name, nfeatures, max_batch, sift=False, **kw):
    spec = mc.SPECS[list_name]
    if spec.norm == "l2":
        kw["norm_type"] = capi.NORM_L2
    if sift:
        kw["feature_method"] = capi.FEATURE_SIFT
    e = capi.Engine(96, 96, max_batch=max_batch, nfeatures=nfeatures, max_matches=spec.max_matches, **kw)
    assert e.desc_dim == spec.dim and e.kcap == (nfeatures or 16320) + 64
    return e


# ---------------------------------------------------------------- the launchers' arithmetic
def _next_pow2(n):
    p = 64
    while p < n:
        p <<= 1
    return p


def hamming_form(kcap, B):
    """rpe_launch_match, crossCheck on the matrix cores: ("fused" | "split", gridDim.y, rounds of 8 owner tiles)"""
    r0 = (max((2 * 8 * 64 + 16) * 16 + kcap * 2, _next_pow2(kcap) * 4) + 15) // 16
    rounds = ((kcap + 31) // 32 + 7) // 8
    lds_fits = r0 * 16 + kcap * 8 <= 65536
    split = min(rounds, max(1, 256 // B)) if B <= SPLIT_PAIRS else 1
    return ("split" if split > 1 or not lds_fits else "fused"), split, rounds


def hamming_ratio_lds(kcap):
    return QTILE * 32 + kcap * 4


def l2_form(kcap, B):
    """rpe_launch_match_l2 on the matrix cores: (gridDim.x, gridDim.y)"""
    chunks = (kcap + 127) // 128
    return chunks, min(8, max(1, (1024 + chunks * 2 * B - 1) // (chunks * 2 * B)))


def l2_tiles(n_scan, split):
    """tiles per workgroup and the number of workgroups along y that have any"""
    ntq = (n_scan + 31) // 32
    per = (ntq + split - 1) // split
    return per, sum(1 for y in range(split) if y * per < ntq)


# ---------------------------------------------------------------- one call, compared pair by pair
def _check(e, list_name, group, ratio=None):
    spec = mc.SPECS[list_name]
    n1 = [len(c.desc1) for c in group]; n2 = [len(c.desc2) for c in group]
    if spec.norm == "hamming":
        q, t, d, nm = e.match_hamming([c.desc1 for c in group], n1, [c.desc2 for c in group], n2)
    else:
        q, t, d, nm = e.match_l2([c.desc1.astype(np.float32) for c in group], n1, [c.desc2.astype(np.float32) for c in group], n2)
    bad = []
    for i, c in enumerate(group):
        wq, wt, wd = mc.expected(list_name, c, ratio)
        n = int(nm[i])
        same = n == len(wq) and np.array_equal(q[i, :n], wq) and np.array_equal(t[i, :n], wt)
        if same and spec.norm == "hamming":
            same = np.array_equal(d[i, :n], wd)
        elif same:
            same = np.array_equal(d[i, :n].view(np.uint32), wd.view(np.uint32))
        if not same:
            k = min(n, len(wq))
            diff = np.nonzero((q[i, :k] != wq[:k]) | (t[i, :k] != wt[:k]) | (d[i, :k] != wd[:k]))[0]
            first = int(diff[0]) if len(diff) else k
            bad.append((i, c.name, "n_matches", n, "model", len(wq), "first difference at", first,
                        "got", (q[i, first:first + 3].tolist(), t[i, first:first + 3].tolist(), d[i, first:first + 3].tolist()),
                        "model", (wq[first:first + 3].tolist(), wt[first:first + 3].tolist(), wd[first:first + 3].tolist())))
    assert not bad, bad
    return nm


def _in_calls(e, list_name, cases, B, ratio=None):
    for s in range(0, len(cases), B):
        _check(e, list_name, cases[s:s + B], ratio)


# ================================================================= Hamming, crossCheck, matrix cores
@pytest.fixture(scope="module")
def ham96(capi):
    e = _engine(capi, "ham_96", 96, 4)
    yield e
    e.close()


@pytest.fixture(scope="module")
def ham448(capi):
    e = _engine(capi, "ham_448", 448, 4)
    yield e
    e.close()


@pytest.fixture(scope="module")
def ham448_many(capi):
    e = _engine(capi, "ham_448_many", 448, 65)
    yield e
    e.close()


@pytest.fixture(scope="module")
def ham5000(capi):
    e = _engine(capi, "ham_5000", 5000, 65)
    yield e
    e.close()


@pytest.mark.parametrize("B", [4, 1])
def test_hamming_fused_one_round(ham96, B):
    """match_hamming_mfma_kernel<false>: kcap = 160 is 5 owner tiles, one round of 8, so min(rounds, 256 / B) = 1 for every
    B and even a single pair takes the fused kernel (election words in LDS, in-kernel sort).  Empty sides, one row, 31 / 32 /
    33 rows around a tile, and 129 and 160 scanned rows: 5 scanned tiles, one more than the MM_PF = 4 register ring."""
    assert ham96.kcap == 160 and hamming_form(160, B) == ("fused", 1, 1)
    cases = mc.cases("ham_96")
    if B == 1:
        cases = [c for c in cases if c.name.split(":")[2] in ("0x7", "1x1", "33x31", "160x129", "129x160")]
        assert len(cases) == 7
    _in_calls(ham96, "ham_96", cases, B)


def test_hamming_split_two_workgroups(ham448):
    """match_hamming_mfma_kernel<true> + match_hamming_select_kernel, gridDim.y = 2: kcap = 512 is two rounds of owner tiles
    and a single pair may take 256 workgroups.  100 x 100: the second workgroup has no owner tile; 255 / 256 / 257 rows: the
    equal rows 255 | 256 are owned by the two workgroups, and their HBM atomicMin decides."""
    assert ham448.kcap == 512 and hamming_form(512, 1) == ("split", 2, 2)
    _in_calls(ham448, "ham_448", [c for c in mc.cases("ham_448") if len(c.desc1)], 1)


def test_hamming_split_ragged_batch(ham448):
    """the same SPLIT form over a batch of 4 unequal pairs (gridDim = (4, 2)), one of them empty: the HBM election words
    of a pair start at pair * kcap"""
    assert hamming_form(512, 4) == ("split", 2, 2) and hamming_form(512, 3) == ("split", 2, 2)
    c = {x.name.split(":", 1)[1]: x for x in mc.cases("ham_448")}
    _check(ham448, "ham_448", [c["mixed:512x512"], c["mixed:0x100"], c["mixed:100x100"], c["mixed:255x257"]])
    _check(ham448, "ham_448", [c["far:257x255"], c["mixed:256x256"], c["mixed:257x255"]])


def _many(n):
    """n pairs cycling the small cases, the 512 x 512 pair at position 7"""
    cs = mc.cases("ham_448_many")
    big, small = cs[0], cs[1:]
    assert big.name.endswith("512x512")
    group = [small[i % len(small)] for i in range(n)]
    group[7] = big
    return group


def test_hamming_fused_two_rounds(ham448_many):
    """match_hamming_mfma_kernel<false> with 65 pairs (more than RPE_MATCH_SPLIT_PAIRS): split = 1 and kcap = 512 fits LDS,
    so one workgroup per pair walks both rounds of owner tiles itself; the 512 x 512 pair uses both"""
    assert ham448_many.kcap == 512 and hamming_form(512, 65) == ("fused", 1, 2)
    nm = _check(ham448_many, "ham_448_many", _many(65))
    assert nm[7] == 60


def test_hamming_split_at_64_pairs(ham448_many):
    """the same engine and pairs without the last: 64 pairs is the largest batch that splits (256 / 64 = 4 >= 2 rounds:
    gridDim = (64, 2)), and the engine allocated its HBM election words for exactly 64 pairs"""
    assert hamming_form(512, 64) == ("split", 2, 2)
    _check(ham448_many, "ham_448_many", _many(64))


def _one_large(n):
    cs = mc.cases("ham_5000")
    big, small = cs[0], cs[1:]
    assert big.name.endswith("5064x5000") and all(max(len(c.desc1), len(c.desc2)) <= 64 for c in small)
    group = [small[i % len(small)] for i in range(n)]
    group[n // 2] = big
    return group


def test_hamming_hbm_words_one_workgroup(ham5000):
    """match_hamming_mfma_kernel<true> with gridDim.y = 1: 65 pairs do not split, but 8 bytes of election words per keypoint
    do not fit 64 KB of LDS at kcap = 5064, so the HBM form serves the batch and one workgroup walks all 20 rounds of the
    one 5064 x 5000 pair.  The other 64 pairs have at most 64 rows."""
    assert ham5000.kcap == 5064 and hamming_form(5064, 65) == ("split", 1, 20)
    assert hamming_form(4096, 65)[0] == "fused" and hamming_form(4097, 65)[0] == "split"      # where LDS stops fitting
    _check(ham5000, "ham_5000", _one_large(65))


def test_hamming_split_twenty_workgroups(ham5000):
    """match_hamming_mfma_kernel<true>, gridDim.y = 20: one pair of 5064 x 5000, every round of 8 owner tiles in a
    workgroup of its own; the equal rows 255 | 256 and the last two rows of either side sit in different workgroups or
    at the ragged end of the last one"""
    assert hamming_form(5064, 1) == ("split", 20, 20)
    _check(ham5000, "ham_5000", [mc.cases("ham_5000")[0]])


def test_hamming_first_capacity_beyond_lds(capi):
    """kcap = 4097 is the first capacity whose fused form does not fit LDS (the sort size doubles to 8192 keys), in an engine
    of 65 pairs: the launcher's memsets of B x kcap election words and the engine's allocation of them must follow one rule.
    65 pairs: beyond the split limit, the HBM form with one workgroup per pair; then 64 pairs: gridDim = (64, 4).  The pairs
    cycle the small cases of ham_5000 (at most 64 rows: one owner tile or two, so the workgroups y >= 1 have no round);
    each case with both sides >= 2 has a model match."""
    e = _engine(capi, "ham_5000", 4033, 65)
    try:
        assert e.kcap == 4097 and hamming_form(4096, 65)[0] == "fused"
        small = mc.cases("ham_5000")[1:]
        assert all(max(len(c.desc1), len(c.desc2)) <= 64 for c in small)
        assert all(len(mc.expected("ham_5000", c)[0]) >= 1 for c in small if min(len(c.desc1), len(c.desc2)) >= 2)
        assert hamming_form(4097, 65) == ("split", 1, 17)
        _check(e, "ham_5000", [small[i % len(small)] for i in range(65)])
        assert hamming_form(4097, 64) == ("split", 4, 17)
        _check(e, "ham_5000", [small[i % len(small)] for i in range(64)])
    finally:
        e.close()


# ================================================================= Hamming, Lowe ratio (vector ALU)
@pytest.mark.parametrize("ratio", [0.75, 1.0])
def test_hamming_ratio_valu(capi, ratio):
    """match_hamming_ratio_kernel (Lowe ratio) at the largest capacity, kcap = 8064: 32 KB of staging + 4 bytes per keypoint
    = 65 024 B of LDS.  n2 = 1023 / 1024 / 1025 / 2049 trains cross the QTILE = 1024 staging tile once and twice; n2 < 2
    gives nothing; n1 = 257 and 1500 queries take 2 and 6 owner chunks of 256.  ratio = 1.0: best == second is dropped."""
    e = _engine(capi, "ham_8000_ratio", 8000, 2, match_mode=capi.MATCH_RATIO, match_ratio=ratio)
    try:
        assert e.kcap == 8064 and hamming_ratio_lds(e.kcap) == 65024 <= 65536
        _in_calls(e, "ham_8000_ratio", mc.cases("ham_8000_ratio"), 2, ratio)
    finally:
        e.close()


# ================================================================= L2: SIFT (128 bytes, KS = 4) and ORB bytes (32 bytes, KS = 1)
WIDTHS = [pytest.param(True, id="sift"), pytest.param(False, id="orb")]


def _l2_name(sift, what):
    return f"l2_{'sift' if sift else 'orb'}_{what}"


@pytest.mark.parametrize("sift", WIDTHS)
def test_l2_tiles_over_eight_workgroups(capi, sift):
    """match_l2_norms_kernel + match_l2_mfma_kernel<4 | 1> + match_l2_select_kernel, one pair at kcap = 512: grid (4, 8, 2),
    the scanned tiles dealt over 8 workgroups.  1 and 33 scanned rows: 1 and 2 tiles, workgroups y >= 1 / 2 return at once;
    96: 3 tiles, y >= 3 return; 288: 9 tiles, 2 per workgroup, the fifth has one and the last three none; 512: 2 each.
    Owners 127 / 128 / 129 end a workgroup's 4 waves x 32 columns.  KS = 1 (ORB): only wave 0 loads."""
    name = _l2_name(sift, "448")
    e = _engine(capi, name, 448, 4, sift=sift)
    try:
        assert e.kcap == 512 and l2_form(512, 1) == (4, 8)
        assert [l2_tiles(n, 8) for n in (1, 33, 96, 288, 512)] == [(1, 1), (1, 2), (1, 3), (2, 5), (2, 8)]
        _in_calls(e, name, mc.cases(name), 1)
    finally:
        e.close()


@pytest.mark.parametrize("sift", WIDTHS)
def test_l2_prefetch_ring_one_workgroup(capi, sift):
    """match_l2_mfma_kernel at 32 pairs of kcap = 2048: 16 x 2 x 32 = 1024 workgroups without a split, gridDim.y = 1, so one
    workgroup walks all scanned tiles of its pass through the L2M_PF = 3 register ring: 32 .. 161 scanned rows are 1 to 6
    tiles (prologue only, one to three unrolled steps, a second trip of the loop), scanned either way round; the
    other pairs are tiny or empty."""
    name = _l2_name(sift, "1984_ring")
    e = _engine(capi, name, 1984, 32, sift=sift)
    try:
        assert e.kcap == 2048 and l2_form(2048, 32) == (16, 1)
        assert [l2_tiles(n, 1)[0] for n in (32, 33, 65, 97, 129, 161)] == [1, 2, 3, 4, 5, 6]
        cs = list(mc.cases(name))
        _check(e, name, (cs + cs[::-1])[:32])                  # 21 cases; 11 of them again in other pair slots
    finally:
        e.close()


@pytest.mark.parametrize("sift", WIDTHS)
def test_l2_eight_chunks_of_eight_tiles(capi, sift):
    """match_l2_mfma_kernel, one pair of 2048 x 2048 at kcap = 2048: grid (16, 8, 2), every workgroup scans a chunk of 8
    tiles = 256 rows and the 8 chunks meet in a 64-bit atomicMin; the equal rows 255 | 256 straddle the first chunk
    boundary, where the lower index must win across workgroups.  300 x 2048 of near-extreme rows: float32 roots collide
    across chunks.  (An engine of its own: max_matches belongs to the engine, and this list truncates at 100.)"""
    name = _l2_name(sift, "1984_full")
    e = _engine(capi, name, 1984, 1, sift=sift)
    try:
        assert e.kcap == 2048 and l2_form(2048, 1) == (16, 8) and l2_tiles(2048, 8) == (8, 8)
        _in_calls(e, name, mc.cases(name), 1)
    finally:
        e.close()


@pytest.mark.parametrize("ratio", [0.8, 1.0])
@pytest.mark.parametrize("sift", WIDTHS)
def test_l2_ratio(capi, sift, ratio):
    """match_l2_ratio_kernel<8 | 2> (Lowe ratio; the only L2 ratio matcher): n2 = 255 / 256 / 257 / 512 trains cross
    the L2_QTILE = 256 staging tile (512 = kcap: two full tiles), n2 < 2 gives nothing, n1 = 255 / 257 queries are one
    owner chunk and one row more.  Near-extreme rows under ratio = 1.0: best < second must be decided on the float32
    roots, which collide where the integers differ."""
    name = _l2_name(sift, "448_ratio")
    e = _engine(capi, name, 448, 4, sift=sift, match_mode=capi.MATCH_RATIO, match_ratio=ratio)
    try:
        assert e.kcap == 512 == 2 * L2_QTILE
        _in_calls(e, name, mc.cases(name), 4, ratio)
    finally:
        e.close()


def test_l2_select_sorts_16384_keys(capi):
    """match_l2_select_kernel with 128 KB of dynamic LDS: SIFT without a cap (nfeatures = 0) has kcap = 16384, the sort
    array is next_pow2(kcap) 64-bit keys whatever the pair holds, and 8200 queries sort 16384 of them.  70 x 8200 scans
    257 tiles in 4 chunks of 65."""
    e = _engine(capi, "l2_sift_uncapped", 0, 1, sift=True)
    try:
        assert e.kcap == 16384 and _next_pow2(e.kcap) * 8 == 131072 and l2_form(e.kcap, 1) == (128, 4)
        _in_calls(e, "l2_sift_uncapped", mc.cases("l2_sift_uncapped"), 1)
    finally:
        e.close()
