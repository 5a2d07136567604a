"""CPU tests of the pair proposals: the NumPy model (tests/similarity_model.py) against hand-built cases and its own
properties, geometry.pairs_of_candidates, and the loop scene -- ORB of the CPU oracle scored by the model.  The GPU tests
(tests/test_gpu_similarity.py) compare the kernels with this model exactly."""
import numpy as np
import pytest

from relative_pose_estimation_amd import geometry
from tests import similarity_cases as sc
from tests import similarity_model as sm


@pytest.mark.parametrize("name", sorted(sc.HAND_CASES))
def test_model_reproduces_the_hand_built_cases(name):
    descs, step, expected, last = sc.hand_case(name)
    idx = np.arange(len(descs))
    for md, want in expected.items():
        got = sm.score_matrix(descs, idx, idx, step, md)
        assert np.array_equal(got, want), (name, md, got)
    if last is not None:
        md = max(expected)
        got = sm.score_matrix(descs, idx, idx, step, md, last=True)
        assert np.array_equal(got, last), (name, got)
        assert not np.array_equal(got, expected[md]), "the case's ties must matter"


def test_a_duplicate_case_depends_on_the_tie_rule():
    """at least one hand-built case with duplicates changes its score matrix under last=True"""
    assert any(last is not None for _, _, _, last in sc.HAND_CASES.values())
    # and so do the generated tie cases the GPU tests use
    descs = sc.tie_frames(3, [7, 12, 33, 5])
    idx = np.arange(4)
    assert not np.array_equal(sm.score_matrix(descs, idx, idx), sm.score_matrix(descs, idx, idx, last=True))


def test_score_is_symmetric_and_self_pairs_are_pairs():
    for descs in (sc.random_frames(11, [0, 1, 31, 40, 65]), sc.tie_frames(12, [0, 3, 20, 33])):
        idx = np.arange(len(descs))
        for step, md in ((1, 256), (1, 30), (3, 40), (2, 0)):
            S = sm.score_matrix(descs, idx, idx, step, md)          # every entry from its own ordered pair
            assert np.array_equal(S, S.T), (step, md)
            assert (S[0] == 0).all()                                 # an empty sample
            for f in idx:                                            # no more mutual pairs than the smaller sample holds
                assert (S[f] <= len(sm.sample(descs[f], step))).all()
    # distinct descriptors: a frame matches itself completely at distance 0
    d = sc.frame([0, 7, 19, 200])
    assert sm.score(d, d, 1, 0) == 4


def test_step_samples_every_step_th_descriptor():
    d = sc.random_frames(5, [10, 11])
    for step in (1, 2, 3, 4, 5, 10, 11, 12, 1000):
        for n, f in zip((10, 11), d):
            s = sm.sample(f, step)
            assert len(s) == -(-n // step)                           # ceil(n / step), n not a multiple of step included
            assert all(np.array_equal(s[k], f[k * step]) for k in range(len(s)))
        a = [f[::step].copy() for f in d]                            # the packed samples under step 1 give the same score
        assert sm.score(d[0], d[1], step, 256) == sm.score(a[0], a[1], 1, 256)
    assert sm.score(d[0], d[1], 1000, 256) == 1                      # descriptor 0 against descriptor 0


def test_max_distance_bounds():
    descs = sc.random_frames(8, [40, 50], flips=40, dup=0.3)
    d = sm.mutual_distances(descs[0], descs[1])
    assert (d == 0).any() and (d > 0).any()                          # the case has exact duplicates and real distances
    assert sm.score(descs[0], descs[1], 1, 0) == np.count_nonzero(d == 0)
    assert sm.score(descs[0], descs[1], 1, 256) == d.size            # 256 bounds nothing
    far = [sc.frame([0]), sc.frame([256])]                           # all bits differ
    assert sm.score(far[0], far[1], 1, 255) == 0 and sm.score(far[0], far[1], 1, 256) == 1


def test_selection_rules_on_a_written_out_matrix():
    S, q, t = sc.SELECT_SCORES, sc.SELECT_Q, sc.SELECT_T
    # row 0 (slot 0): column 0 is its own slot; 7 (col 4), then the tie 5 = 5 broken by column: 1, 2; column 3 scores 0
    cand, cs, n = sm.candidates(S, q, t, 3)
    assert cand[0].tolist() == [4, 1, 2] and cs[0].tolist() == [7, 5, 5]
    # row 1 (slot 1): columns 1 AND 4 are its own slot (a repeated column); 7 (col 3), 5 (col 0), 1 (col 2)
    assert cand[1].tolist() == [3, 0, 2] and cs[1].tolist() == [7, 5, 1]
    assert n.tolist() == [3, 3, 3, 3]
    # k larger than the eligible count: -1 past the count; min_score cuts the zeros and ones
    cand, cs, n = sm.candidates(S, q, t, 6, min_score=2)
    assert n.tolist() == [3, 2, 1, 2]
    assert cand[2].tolist() == [0, -1, -1, -1, -1, -1] and cs[2].tolist() == [5, -1, -1, -1, -1, -1]
    assert cand[3].tolist() == [1, 4, -1, -1, -1, -1] and cs[3].tolist() == [7, 3, -1, -1, -1, -1]
    # a repeated column is a column like any other: row 0 has both columns of slot 1
    cand, _, _ = sm.candidates(S, q, t, 6)
    assert cand[0].tolist() == [4, 1, 2, 3, -1, -1]
    # exclude without times: time = slot.  Row 0 (slot 0) with exclude = 1 loses the columns of slot 1
    cand, cs, n = sm.candidates(S, q, t, 3, exclude=1)
    assert cand[0].tolist() == [2, 3, -1] and n[0] == 2
    # exclude = 0 excludes equal times only -- nothing more than the own slot here
    assert np.array_equal(sm.candidates(S, q, t, 3, exclude=0)[0], sm.candidates(S, q, t, 3)[0])
    # exclude with times: the rows at times 10, 11, 12, 13, the columns at 10, 20, 12, 13, 11 -- column 1 (slot 1) is far from
    # row 0 now, column 4 (slot 1, time 11) is not
    cand, cs, n = sm.candidates(S, q, t, 3, q_time=[10, 11, 12, 13], t_time=[10, 20, 12, 13, 11], exclude=1)
    assert cand[0].tolist() == [1, 2, 3] and cs[0].tolist() == [5, 5, 0]


def test_pairs_of_candidates():
    S, q, t = sc.SELECT_SCORES, sc.SELECT_Q, sc.SELECT_T
    cand, cs, _ = sm.candidates(S, q, t, 2, min_score=1)
    # rows: 0 -> cols 4 (slot 1, 7), 1 (slot 1, 5); 1 -> 3 (slot 3, 7), 0 (slot 0, 5); 2 -> 0 (slot 0, 5), 1 (slot 1, 1); 3 -> 1 (slot 1, 7), 4 (slot 1, 3)
    pairs, score = geometry.pairs_of_candidates(q, t, cand, cs)
    assert pairs.dtype == np.int32 and score.dtype == np.int32
    # (0, 1) from rows 0 (7, 5) and 1 (5): once, with 7.  (1, 3) from rows 1 (7) and 3 (7, 3): once.  Then (0, 2) 5, (1, 2) 1
    assert pairs.tolist() == [[0, 1], [1, 3], [0, 2], [1, 2]] and score.tolist() == [7, 7, 5, 1]
    # nothing proposed
    pairs, score = geometry.pairs_of_candidates([0, 1], [0, 1], np.full((2, 3), -1), np.full((2, 3), -1))
    assert pairs.shape == (0, 2) and score.shape == (0,)
    with pytest.raises(ValueError):
        geometry.pairs_of_candidates([0], [0], [[0]], [[5]])         # a frame with itself
    with pytest.raises(ValueError):
        geometry.pairs_of_candidates([0], [1], [[1]], [[5]])         # no such column
    with pytest.raises(ValueError):
        geometry.pairs_of_candidates([0, 1], [1], [[0]], [[5]])      # one row for two queries


def test_loop_scene_separates_revisits_from_distractors(oracle):
    """The walk returns to its first four poses (perturbed); three frames of another scene stand by.  Under the model alone every
    revisit pair outscores every pair with a distractor frame, and every revisit frame's best candidate more than 3 frames
    away in time is its twin or a walk neighbour of its twin.  Prints the table DESIGN section 8 quotes."""
    table, S = sc.loop_table(oracle)
    print()
    print(sc.format_loop_table(table))
    frames, K, twin, distract = sc.loop_scene()
    kind = sc.loop_kinds(twin, distract)
    for (step, md), row in table.items():
        assert row["revisit"][0] > row["distractor"][2], (step, md, row)             # min over revisits > max over distractors
    # the visible gap at the default: the weakest revisit scores at least twice the strongest distractor pair
    row = table[(1, sc.LOOP_MAX_DISTANCE)]
    assert row["revisit"][0] >= 2 * row["distractor"][2], row
    n = len(twin)
    idx = np.arange(n, dtype=np.int32)
    for step in (1, 4):
        cand, _, ncand = sm.candidates(S[(step, sc.LOOP_MAX_DISTANCE)], idx, idx, 1, exclude=3)
        for f in np.nonzero(twin >= 0)[0]:
            assert ncand[f] == 1 and abs(int(cand[f, 0]) - int(twin[f])) <= 1, (step, f, cand[f], twin[f])
