"""Plain Python / NumPy model of the multi-view tracks (include/rpe_amd.h, "multi-view tracks"), written from the header's
rule: a dictionary union-find over the nodes that have an edge, the one-keypoint-per-frame filter, min_len, and the two
orders (tracks by smallest node id, observations by node id).  Independent of the kernels' atomics, scans and ranks; used by
test_tracks_cpu.py and test_gpu_tracks.py.  Every output is an integer or a copied f32: all comparisons are exact."""
import numpy as np

EDGES_USABLE, EDGES_RANSAC, EDGES_ALL = 0, 1, 2
COUNTS = ("n_tracks", "n_obs", "n_edges", "dropped_conflict", "dropped_short", "n_frames_seen")
ARRAYS = ("track_start", "obs_frame", "obs_kp", "obs_xy", "match_track")


def pad(rows, mm, width=0, dtype=np.int32, fill=0):
    """ragged per-pair lists -> [P, mm] (or [P, mm, width])"""
    out = np.full((len(rows), mm) + ((width,) if width else ()), fill, dtype)
    for p, r in enumerate(rows):
        r = np.asarray(r, dtype).reshape((-1, width) if width else (-1,))
        out[p, :len(r)] = r
    return out


def run_edges(run, edge_rule, use_pair=None):
    """bool[P, mm]: the edges of a run (tests.scale_model.Run: match indices, masks, statuses and counts as the C-ABI
    returns them) under edge_rule and use_pair"""
    P, mm = run.qidx.shape
    e = np.zeros((P, mm), bool)
    for p in range(P):
        if use_pair is not None and not use_pair[p]:
            continue
        n = min(max(int(run.n_matches[p]), 0), mm)
        if edge_rule == EDGES_ALL:
            e[p, :n] = True
        elif run.status[p] == 0:
            e[p, :n] = run.ransac_mask[p, :n] & (run.pose_mask[p, :n] if edge_rule == EDGES_USABLE else True)
    return e


def build_tracks(n_frames, KC, frame1, frame2, qidx, tidx, edge, pts1=None, pts2=None, min_len=2):
    """The tracks of P pairs: pair p joins frames frame1[p], frame2[p]; qidx, tidx i32[P, mm]; edge bool[P, mm] = the
    matches that are edges (everything the rule asks of a match, i < n_matches included); pts1, pts2 f32[P, mm, 2] or
    None.  Returns the dict of _capi.Engine.build_tracks."""
    qidx = np.asarray(qidx); tidx = np.asarray(tidx); edge = np.asarray(edge).astype(bool)
    P, mm = qidx.shape if qidx.ndim == 2 else (0, 0)
    parent, first = {}, {}

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    n_edges = 0
    edge_nodes = {}
    for p in range(P):
        for i in range(mm):
            if not edge[p, i]:
                continue
            n_edges += 1
            eid = p * mm + i
            a = int(frame1[p]) * KC + int(qidx[p, i]); b = int(frame2[p]) * KC + int(tidx[p, i])
            edge_nodes[eid] = a
            for side, node in ((0, a), (1, b)):            # ascending edge id, image 1 first: the first writer wins
                parent.setdefault(node, node)
                first.setdefault(node, (p, i, side))
            ra, rb = find(a), find(b)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
    comps = {}
    for node in parent:
        comps.setdefault(find(node), []).append(node)
    tracks, conflict, short = [], 0, 0
    for root in sorted(comps, key=lambda r: min(comps[r])):
        nodes = sorted(comps[root])
        frames = [n // KC for n in nodes]
        if len(set(frames)) != len(frames):
            conflict += 1
        elif len(nodes) < min_len:
            short += 1
        else:
            tracks.append(nodes)
    track_of_node = {n: k for k, nodes in enumerate(tracks) for n in nodes}
    obs = [n for nodes in tracks for n in nodes]
    xy = np.zeros((len(obs), 2), np.float32)
    if pts1 is not None:
        for o, n in enumerate(obs):
            p, i, side = first[n]
            xy[o] = (pts2 if side else pts1)[p][i]
    mt = np.full((P, mm), -1, np.int32)
    for eid, a in edge_nodes.items():
        mt[eid // mm, eid % mm] = track_of_node.get(a, -1)
    out = {'track_start': np.cumsum([0] + [len(t) for t in tracks]).astype(np.int32),
           'obs_frame': np.array([n // KC for n in obs], np.int32), 'obs_kp': np.array([n % KC for n in obs], np.int32),
           'obs_xy': xy, 'match_track': mt,
           'n_tracks': len(tracks), 'n_obs': len(obs), 'n_edges': n_edges, 'dropped_conflict': conflict, 'dropped_short': short,
           'n_frames_seen': len(set(n // KC for n in obs))}
    return out


def as_lists(tracks):
    """the tracks of a dict as lists of (frame, keypoint)"""
    s = tracks['track_start']
    return [[(int(f), int(k)) for f, k in zip(tracks['obs_frame'][s[j]:s[j + 1]], tracks['obs_kp'][s[j]:s[j + 1]])]
            for j in range(len(s) - 1)]


def assert_equal(got, want, what=""):
    """every output of the two dicts, exactly (obs_xy by its bits)"""
    assert set(got) == set(COUNTS) | set(ARRAYS), (what, sorted(got))
    for k in COUNTS:
        assert int(got[k]) == int(want[k]), (what, k, got[k], want[k])
    for k in ARRAYS:
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape, g.dtype, w.dtype)
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8)), (what, k)
