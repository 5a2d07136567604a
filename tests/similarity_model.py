"""NumPy model of the pair proposals (include/rpe_amd.h, "pair proposals"), written from the rules: no code shared with
the kernels, no packed keys.  It builds on match_model's hamming_matrix / cross_check, which state cv2's crossCheck rule
on the whole distance matrix.

The score.  The sample of a frame under a stride step >= 1 is its descriptors 0, step, 2 step, ...; score(a, b) is the
number of mutual nearest neighbours between the two samples (both argmins take the lowest index among equal distances)
whose Hamming distance is <= max_distance.  An empty sample gives 0; a self pair is a pair like any other.

The candidates.  Column c is eligible for row r iff the two frames' slots differ, |q_time[r] - t_time[c]| > exclude when
exclude >= 0, and score >= min_score; a row's candidates are its eligible columns by score descending, then column position
ascending, the first k.  cand / cand_score are -1 past the row's count.

`last=True` replaces every first-occurrence argmin by the last occurrence, as in match_model: no kernel does that; the
cases use it to prove that they have ties that matter."""
import numpy as np

from tests import match_model


def sample(desc, step):
    return np.asarray(desc, np.uint8).reshape(-1, 32)[::step]


def mutual_distances(desc_a, desc_b, step=1, last=False):
    """Hamming distances of the mutual nearest neighbours between the two samples (one per mutual pair, any order)"""
    a, b = sample(desc_a, step), sample(desc_b, step)
    if a.shape[0] == 0 or b.shape[0] == 0:
        return np.zeros(0, np.int32)
    D = match_model.hamming_matrix(a, b)
    return match_model.cross_check(D, max(D.shape), last)[2]      # at most min(D.shape) matches: no cut


def score(desc_a, desc_b, step=1, max_distance=256, last=False):
    return int(np.count_nonzero(mutual_distances(desc_a, desc_b, step, last) <= max_distance))


def score_matrix(descs, q_idx, t_idx, step=1, max_distance=256, last=False):
    """int32 [nq, nt]: score(descs[q_idx[r]], descs[t_idx[c]]), every entry from its own ordered pair"""
    memo = {}
    out = np.zeros((len(q_idx), len(t_idx)), np.int32)
    for r, a in enumerate(q_idx):
        for c, b in enumerate(t_idx):
            key = (int(a), int(b))
            if key not in memo:
                memo[key] = score(descs[key[0]], descs[key[1]], step, max_distance, last)
            out[r, c] = memo[key]
    return out


def candidates(scores, q_slots, t_slots, k, q_time=None, t_time=None, exclude=-1, min_score=0):
    """(cand int32 [nq, k], cand_score int32 [nq, k], n_cand int32 [nq]) of a score matrix; times default to the slots"""
    scores = np.asarray(scores)
    q_time = q_slots if q_time is None else q_time
    t_time = t_slots if t_time is None else t_time
    nq, nt = scores.shape
    cand = np.full((nq, k), -1, np.int32); cs = np.full((nq, k), -1, np.int32); n = np.zeros(nq, np.int32)
    for r in range(nq):
        ok = [c for c in range(nt)
              if int(t_slots[c]) != int(q_slots[r]) and (exclude < 0 or abs(int(q_time[r]) - int(t_time[c])) > exclude)
              and int(scores[r, c]) >= min_score]
        ok.sort(key=lambda c: (-int(scores[r, c]), c))
        ok = ok[:k]
        n[r] = len(ok)
        cand[r, :len(ok)] = ok
        cs[r, :len(ok)] = [scores[r, c] for c in ok]
    return cand, cs, n
