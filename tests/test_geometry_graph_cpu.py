"""The host helpers that turn a chain and its loop pairs into the graphs of Engine.optimise_graphs (geometry.chain_edges,
loop_edges, graphs_of_groups, edges_of_graphs): pure NumPy, no library.  Group boundaries, failed pairs, dropped cross-group
loops, the weights, and that the chain has zero residual under its own edges."""
import numpy as np
import pytest

from relative_pose_estimation_amd import geometry
from tests import bundle_math_model as mm
from tests import pose_graph_model as pg


def _chain(n=10, seed=3):
    rng = np.random.default_rng(seed)
    R = np.zeros((n, 3, 3)); T = np.zeros((n, 3)); R[0] = np.eye(3)
    for f in range(n - 1):
        M = mm.rodrigues(rng.normal(size=3) * 0.05)
        R[f + 1] = M @ R[f]; T[f + 1] = M @ T[f] + rng.normal(size=3) * (0.1 if f == 4 else 1.0)
    return R, T


def test_chain_edges_follow_the_groups_and_carry_the_chain():
    R, T = _chain()
    group = np.array([0, 0, 0, 0, 1, 1, 1, -1, 2, 2])
    e = geometry.chain_edges(R, T, group)
    assert e['i'].tolist() == [0, 1, 2, 4, 5, 8] and e['j'].tolist() == [1, 2, 3, 5, 6, 9]      # none across a boundary, none at -1
    assert (e['kind'] == geometry.EDGE_METRIC).all() and e['i'].dtype == np.int32 and e['kind'].dtype == np.int32
    assert e['R'].shape == (6, 3, 3) and e['t'].shape == (6, 3) and e['w'].shape == (6, 2)
    # zero residual at the start: the rows of the model on the chain's own poses
    r = pg.edge_rows(R[e['i']], T[e['i']], R[e['j']], T[e['j']], e['R'], e['t'], e['w'][:, 0], e['w'][:, 1], e['kind'], jac=False)
    assert np.abs(r).max() < 1e-9
    assert np.abs(np.einsum("nab,ncb->nac", e['R'], e['R']) - np.eye(3)).max() < 1e-12
    # weights: w_rot = 1 / rad(0.5 deg); w_trans = 1 / (rad(2 deg) * max(|m|, the group's median |m|))
    assert np.allclose(e['w'][:, 0], 1.0 / np.deg2rad(0.5))
    length = np.linalg.norm(e['t'], axis=1)
    for grp, sel in ((0, slice(0, 3)), (1, slice(3, 5)), (2, slice(5, 6))):
        med = np.median(length[sel])
        assert np.allclose(e['w'][sel, 1], 1.0 / (np.deg2rad(2.0) * np.maximum(length[sel], med)))
    assert length[3] < np.median(length[3:5]) and e['w'][3, 1] < 1.0 / (np.deg2rad(2.0) * length[3])   # the short step: the median's weight
    e2 = geometry.chain_edges(R, T, group, sigma_rot_deg=1.0, sigma_dir_deg=4.0)
    assert np.allclose(e2['w'], e['w'] / 2.0)


def test_chain_edges_of_degenerate_chains():
    R, T = _chain(3)
    assert geometry.chain_edges(R, T, [-1, -1, -1])['i'].size == 0
    assert geometry.chain_edges(R[:1], T[:1], [0])['i'].size == 0
    still = geometry.chain_edges(np.stack([np.eye(3)] * 3), np.zeros((3, 3)), [0, 0, 0])          # a group that never moves
    assert (still['w'][:, 1] == 0.0).all() and (still['w'][:, 0] > 0).all()
    with pytest.raises(ValueError, match="chain_edges: .*one entry per frame"):
        geometry.chain_edges(R, T, [0, 0])
    with pytest.raises(ValueError, match="chain_edges: the sigmas"):
        geometry.chain_edges(R, T, [0, 0, 0], sigma_rot_deg=0.0)


def test_loop_edges_keep_ok_pairs_inside_one_group():
    group = np.array([0, 0, 0, 0, 1, 1, 1, -1, 0, 0])
    pairs = np.array([(0, 8), (1, 9), (0, 5), (7, 8), (2, 9), (3, 8), (4, 6), (2, 2), (1, 8)])
    P = len(pairs)
    rng = np.random.default_rng(4)
    R = np.stack([mm.rodrigues(rng.normal(size=3) * 0.1) for _ in range(P)])
    t = rng.normal(size=(P, 3, 1)); t /= np.linalg.norm(t, axis=1, keepdims=True)
    status = np.zeros(P, int); status[4] = 2                                 # a failed pair
    t[8] = 0.0                                                               # a pose without a direction
    inl = np.array([50, 9, 50, 50, 50, 50, 50, 50, 50])
    e, dropped = geometry.loop_edges(pairs, R, t, status, group)
    assert dropped.tolist() == [2, 3, 4, 7, 8] and dropped.dtype == np.int32    # across groups, group -1, failed, i == j, zero t
    assert e['i'].tolist() == [0, 1, 3, 4] and e['j'].tolist() == [8, 9, 8, 6]
    assert (e['kind'] == geometry.EDGE_DIRECTION).all()
    assert np.array_equal(e['R'], R[[0, 1, 5, 6]]) and np.array_equal(e['t'], t[[0, 1, 5, 6], :, 0])
    assert np.allclose(e['w'], [1.0 / np.deg2rad(0.5), 1.0 / np.deg2rad(2.0)])
    e, dropped = geometry.loop_edges(pairs, R, t, status, group, min_inliers=10, inliers=inl)
    assert dropped.tolist() == [1, 2, 3, 4, 7, 8] and e['i'].tolist() == [0, 3, 4]
    e, dropped = geometry.loop_edges(np.zeros((0, 2), int), np.zeros((0, 3, 3)), np.zeros((0, 3)), np.zeros(0, int), group)
    assert e['i'].size == 0 and dropped.size == 0 and e['R'].shape == (0, 3, 3)
    with pytest.raises(ValueError, match="loop_edges: .*one entry per pair"):
        geometry.loop_edges(pairs, R[:3], t, status, group)
    with pytest.raises(ValueError, match="loop_edges: a pair names a frame outside"):
        geometry.loop_edges(np.array([(0, 10)]), R[:1], t[:1], status[:1], group)


def test_graphs_of_groups_and_the_deal_of_the_edges():
    group = np.array([0, 0, 0, 0, 1, 1, 1, -1, 0, 0, 3])
    graphs = geometry.graphs_of_groups(group)
    assert graphs == [[0, 1, 2, 3, 8, 9], [4, 5, 6]]                         # group 3 has one frame, -1 is no group
    assert geometry.graphs_of_groups([-1, -1]) == [] and geometry.graphs_of_groups([]) == []
    assert geometry.graphs_of_groups([2, 2, 0, 0]) == [[0, 1], [2, 3]]       # in the order of the groups' first frames
    R, T = _chain(11)
    chain = geometry.chain_edges(R, T, group)
    loops, _ = geometry.loop_edges([(0, 8), (4, 6)], np.stack([np.eye(3)] * 2), [[0, 0, 1.0]] * 2, [0, 0], group)
    per = geometry.edges_of_graphs(graphs, chain, loops)
    assert [p['i'].tolist() for p in per] == [[0, 1, 2, 8, 0], [4, 5, 4]] and [p['j'].tolist() for p in per] == [[1, 2, 3, 9, 8], [5, 6, 6]]
    assert per[0]['kind'].tolist() == [0, 0, 0, 0, 1] and per[0]['R'].shape == (5, 3, 3) and per[0]['w'].shape == (5, 2)
    # what the helpers build is what the model takes: the graph of group 0 is solved and only its loop edge pulls
    out = pg.optimise(R, T, graphs, per)
    assert out['used_edges'].tolist() == [5, 3] and out['frames'].tolist() == [6, 3]
    assert out['edge_chi'][0][:4, 0].max() < 1e-9 < out['edge_chi'][0][4, 0]
