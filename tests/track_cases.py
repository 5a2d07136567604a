"""Hand-built match graphs for the multi-view tracks, with the expected tracks written out by hand, and the random-graph
generator.  A case is a dict: n_frames, frame1 / frame2 [P], q / t ragged per-pair keypoint lists, edge ragged per-pair
masks or None, min_len, and the expectation: tracks as lists of (frame, keypoint), dropped_conflict, dropped_short, n_edges.
Shared by test_tracks_cpu.py (the model) and test_gpu_tracks.py (the kernels against the model)."""
import numpy as np


def _case(name, n_frames, pairs, q, t, tracks, conflict=0, short=0, edge=None, min_len=2, n_edges=None):
    f1, f2 = (list(x) for x in zip(*pairs)) if pairs else ([], [])
    if n_edges is None:
        n_edges = sum(len(x) for x in q) if edge is None else sum(int(np.sum(x)) for x in edge)
    return dict(name=name, n_frames=n_frames, frame1=f1, frame2=f2, q=q, t=t, edge=edge, min_len=min_len,
                tracks=tracks, dropped_conflict=conflict, dropped_short=short, n_edges=n_edges)


def chain(n):
    """n frames, one match per consecutive pair, the keypoint index changing from frame to frame: one track of n"""
    return _case(f"chain{n}", n, [(f, f + 1) for f in range(n - 1)], [[f % 7] for f in range(n - 1)], [[(f + 1) % 7] for f in range(n - 1)],
                 [[(f, f % 7) for f in range(n)]])


def cases(KC):
    """the hand-built cases for keypoint capacity KC (>= 32)"""
    L = KC - 1
    lengths = dict(n_frames=5, pairs=[(0, 1), (1, 2), (2, 3), (3, 4)], q=[[3, 10], [3, 10], [3], [3, 20]], t=[[3, 10], [3, 10], [3], [3, 20]])
    len5 = [(f, 3) for f in range(5)]
    len3 = [(0, 10), (1, 10), (2, 10)]
    len2 = [(3, 20), (4, 20)]
    chain5 = dict(n_frames=5, pairs=[(f, f + 1) for f in range(4)], q=[[3]] * 4, t=[[3]] * 4)
    return [
        # two tracks over 5 frames; the second changes its keypoint index in every frame
        _case("chain5", 5, [(f, f + 1) for f in range(4)], [[3, 10 + f] for f in range(4)], [[3, 11 + f] for f in range(4)],
              [[(f, 3) for f in range(5)], [(f, 10 + f) for f in range(5)]]),
        # frame 2 paired with the four others
        _case("star", 5, [(2, 0), (2, 1), (2, 3), (2, 4)], [[5]] * 4, [[0], [1], [3], [4]], [[(0, 0), (1, 1), (2, 5), (3, 3), (4, 4)]]),
        # a pair, its reverse, the pair again, and a self pair with qidx == tidx: a component of one node, dropped as short
        _case("reversed_repeated_self", 3, [(0, 1), (1, 0), (0, 1), (2, 2)], [[1], [2], [1], [4]], [[2], [1], [2], [4]],
              [[(0, 1), (1, 2)]], short=1),
        # A.1-B.1, B.1-C.1, C.1-A.2 (four frames, so that the four nodes are looked at and not dropped by their number)
        _case("conflict_triangle", 4, [(0, 1), (1, 2), (2, 0)], [[1], [1], [1]], [[1], [1], [2]], [], conflict=1),
        _case("conflict_two_train", 3, [(0, 1)], [[1, 2]], [[5, 5]], [], conflict=1),
        _case("conflict_self_pair", 2, [(1, 1)], [[3]], [[4]], [], conflict=1),
        # a conflicting component of five nodes between clean tracks: dropping it shifts the index of every later track
        _case("conflict_shifts_indices", 6, [(0, 1), (1, 2), (2, 3), (3, 0)], [[0, 1, 5], [1, 6], [1, 6], [1]], [[0, 1, 5], [1, 6], [1, 6], [2]],
              [[(0, 0), (1, 0)], [(0, 5), (1, 5)], [(1, 6), (2, 6), (3, 6)]], conflict=1),
        # 3 frames, one component of 7 nodes (more nodes than frames) built from repeated pairs, and a clean track
        _case("pigeonhole", 3, [(0, 1), (1, 2), (0, 1), (0, 1), (1, 2)], [[0, 1, 2], [0, 0, 0], [1], [9], [9]], [[0, 0, 0], [0, 1, 2], [0], [9], [9]],
              [[(0, 9), (1, 9), (2, 9)]], conflict=1),
        _case("min_len2", tracks=[len5, len3, len2], **lengths),
        _case("min_len3", tracks=[len5, len3], short=1, min_len=3, **lengths),
        _case("min_len6", tracks=[], short=3, min_len=6, **lengths),
        # the mask takes the edge between frames 2 and 3 away: two tracks
        _case("edge_mask_cuts", tracks=[[(0, 3), (1, 3), (2, 3)], [(3, 3), (4, 3)]], edge=[[1], [1], [0], [1]], **chain5),
        _case("edge_mask_all_zero", tracks=[], edge=[[0]] * 4, **chain5),
        # pairs without matches between the others
        _case("empty_pairs", 3, [(0, 1), (0, 2), (1, 2), (2, 0)], [[], [4], [], [4]], [[], [4], [], [4]], [[(0, 4), (2, 4)]]),
        # node (1, 1) is named by edge 0 (as image 2) and by the edge of pair 1 (as image 1): the lower edge id gives its xy
        _case("xy_lowest_edge", 3, [(0, 1), (1, 2)], [[1], [1]], [[1], [1]], [[(0, 1), (1, 1), (2, 1)]]),
        # the first edge of node (1, 1) names it on both sides: image 1's point
        _case("xy_both_sides", 2, [(1, 1), (0, 1)], [[1], [1]], [[1], [1]], [[(0, 1), (1, 1)]]),
        # keypoint KC - 1 of frame n_frames - 1: the last node
        _case("last_node", 4, [(2, 3), (0, 3)], [[L], [0]], [[L], [L]], [[(0, 0), (2, L), (3, L)]]),
    ] + [chain(n) for n in (63, 64, 65, 130)]


def edge_points(P, mm):
    """pts1, pts2 f32[P, mm, 2]: a different point for every (match, side), so that obs_xy tells which edge and which side
    it was copied from"""
    eid = np.arange(P * mm, dtype=np.float32).reshape(P, mm)
    return np.stack([eid + 0.25, np.full_like(eid, 1.0)], -1), np.stack([eid + 0.75, np.full_like(eid, 2.0)], -1)


# ---- random graphs ----------------------------------------------------------------------------------------------------------
RANDOM = dict(n_frames=12, n_kp=64, n_pairs=24, n_matches=24, redirect=0.03, min_len=3)
# what every seed 0 .. 9 must give (asserted on the model's output, so a changed generator cannot pass empty)
RANDOM_FLOORS = dict(n_tracks=59, dropped_conflict=6, dropped_short=28)
RANDOM_LONGEST = (11, 12)


def random_graph(seed):
    """12 frames of 64 keypoints: a hidden permutation per frame takes the 64 scene points to keypoint indices; 24 pairs of two
    distinct frames with 24 matches each between the two images of a scene point; 3 % of the matches redirected to a random
    train keypoint.  The pairs are those of a window of 2 over the 12 frames taken as a ring ((f, f + 1) and (f, f + 2)), in
    a shuffled order; the 24 scene points of a pair are drawn with replacement, so a pair repeats a match now and then.  With
    these choices every seed 0 .. 9 clears RANDOM_FLOORS and RANDOM_LONGEST (pairs of two random frames leave a seed or two
    below them)."""
    g = RANDOM
    rng = np.random.default_rng(seed)
    F = g["n_frames"]
    perm = [rng.permutation(g["n_kp"]) for _ in range(F)]
    ring = [(f, (f + 1) % F) for f in range(F)] + [(f, (f + 2) % F) for f in range(F)]
    assert len(ring) == g["n_pairs"]
    f1, f2, q, t = [], [], [], []
    for k in rng.permutation(g["n_pairs"]):
        a, b = ring[k]
        pts = rng.integers(0, g["n_kp"], g["n_matches"])
        qi, ti = perm[a][pts].copy(), perm[b][pts].copy()
        wrong = rng.random(g["n_matches"]) < g["redirect"]
        ti[wrong] = rng.integers(0, g["n_kp"], int(wrong.sum()))
        f1.append(int(a)); f2.append(int(b)); q.append(qi.tolist()); t.append(ti.tolist())
    return dict(name=f"random{seed}", n_frames=g["n_frames"], frame1=f1, frame2=f2, q=q, t=t, edge=None, min_len=g["min_len"])
