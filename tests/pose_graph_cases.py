"""The pose-graph scenes of the tests: the loop scene of the accuracy table (a camera on a circle whose last frames see the
first ones again) and the hand-built graphs, each the smallest shape at which pg_solve_kernel can still go wrong.  Pure
NumPy; a case is the keyword arguments of Engine.optimise_graphs / pose_graph_model.optimise."""
import numpy as np

from relative_pose_estimation_amd import geometry
from tests import bundle_math_model as mm
from tests import pose_graph_model as pg

SIGMA_ROT, SIGMA_DIR = 0.5, 2.0                       # the helpers' defaults, degrees
W_ROT, W_DIR = 1.0 / np.deg2rad(SIGMA_ROT), 1.0 / np.deg2rad(SIGMA_DIR)


def _small_rot(rng, sigma_rad):
    return mm.rodrigues(rng.normal(size=3) * sigma_rad)


def _perturb_dir(rng, v, sigma_rad):
    n = np.linalg.norm(v)
    d = v / n + rng.normal(size=3) * sigma_rad
    return d / np.linalg.norm(d) * n


def loop_scene(n, loops, seed, wrong=0, rot_noise_deg=0.3, dir_noise=0.02, scale_drift=0.01):
    """A camera on a circle of radius 10, looking along the tangent; the last `loops` frames come round to the first ones
    again, half a step short of them.  The chain integrates noisy steps (rotation noise, direction noise, scale drift per
    step) from frame 0 at the truth; chain edges are geometry.chain_edges of that chain, loop edges are direction edges
    (k, n - loops + k) with the same noise; `wrong` more loop edges carry an unrelated pose.  Returns a dict: the case
    ('R_abs', 'T_abs', 'graphs', 'edges') and 'R_true', 'T_true'."""
    rng = np.random.default_rng(seed)
    th = 2.0 * np.pi * np.arange(n) / (n - loops + 0.5)
    Rt = np.stack([mm.rodrigues([0.0, -a, 0.0]) for a in th])
    C = np.stack([10.0 * np.cos(th), np.zeros(n), 10.0 * np.sin(th)], 1)
    Tt = -np.einsum("fab,fb->fa", Rt, C)
    R = np.zeros((n, 3, 3)); T = np.zeros((n, 3)); R[0] = Rt[0]; T[0] = Tt[0]
    scale = 1.0
    for f in range(n - 1):
        Mt = Rt[f + 1] @ Rt[f].T
        mt = Tt[f + 1] - Mt @ Tt[f]
        M = _small_rot(rng, np.deg2rad(rot_noise_deg)) @ Mt
        scale *= 1.0 + scale_drift * rng.normal()
        m = scale * _perturb_dir(rng, mt, dir_noise)
        R[f + 1] = M @ R[f]; T[f + 1] = M @ T[f] + m
    group = np.zeros(n, np.int32)
    chain = geometry.chain_edges(R, T, group, SIGMA_ROT, SIGMA_DIR)
    pairs, Rl, tl = [], [], []
    for k in range(loops):
        i, j = k, n - loops + k
        Mt = Rt[j] @ Rt[i].T
        mt = Tt[j] - Mt @ Tt[i]
        pairs.append((i, j)); Rl.append(_small_rot(rng, np.deg2rad(rot_noise_deg)) @ Mt)
        tl.append(_perturb_dir(rng, mt, dir_noise) / np.linalg.norm(mt))
    for k in range(wrong):
        i = int(rng.integers(0, n // 3)); j = int(rng.integers(n // 2, n))
        v = rng.normal(size=3)
        pairs.append((i, j)); Rl.append(_small_rot(rng, 1.0)); tl.append(v / np.linalg.norm(v))
    loop, dropped = geometry.loop_edges(pairs, Rl, tl, np.zeros(len(pairs), int), group, sigma_rot_deg=SIGMA_ROT, sigma_dir_deg=SIGMA_DIR)
    assert dropped.size == 0
    graphs = geometry.graphs_of_groups(group)
    return dict(R_abs=R, T_abs=T, graphs=graphs, edges=geometry.edges_of_graphs(graphs, chain, loop), R_true=Rt, T_true=Tt)


def scene_errors(R, T, R_true, T_true):
    """(rotation errors in degrees, centre errors) per frame"""
    rot = np.array([mm.rot_angle_deg(a, b) for a, b in zip(R, R_true)])
    c = -np.einsum("fji,fj->fi", R, T); ct = -np.einsum("fji,fj->fi", R_true, T_true)
    return rot, np.sqrt(((c - ct) ** 2).sum(1))


def _case(sc, **kw):
    return dict({k: sc[k] for k in ('R_abs', 'T_abs', 'graphs', 'edges')}, **kw)


def _edges(i, j, R, t, w, kind):
    return geometry._edge_dict(i, j, R, t, w, kind)


def two_frames():
    """1: two frames, one metric edge that disagrees with the start"""
    R = np.stack([np.eye(3), mm.rodrigues([0.02, -0.01, 0.03])]); T = np.array([[0.0, 0.0, 0.0], [1.0, 0.1, -0.2]])
    e = _edges([0], [1], [mm.rodrigues([0.0, 0.05, 0.0])], [[1.2, 0.0, 0.0]], [[W_ROT, 10.0]], [pg.EDGE_METRIC])
    return dict(R_abs=R, T_abs=T, graphs=[[0, 1]], edges=[e])


def loop12():
    """2: a 12-frame loop with 2 direction loop edges"""
    return _case(loop_scene(12, 2, 5))


def big300():
    """3: 300 free frames and 306 used edges: more than one item per lane in both kinds of reduction, a second chunk that is
    not full"""
    return _case(loop_scene(301, 6, 6), cg_iters=16, max_iters=3)


def hub():
    """4: a free hub frame with 40 incident edges, the first of them to the fixed frame"""
    rng = np.random.default_rng(7)
    n = 41
    R = np.stack([_small_rot(rng, 0.3) for _ in range(n)]); T = rng.uniform(-5, 5, (n, 3))
    others = [0] + list(range(2, n))
    M = np.stack([_small_rot(rng, 0.01) @ R[k] @ R[1].T for k in others])
    m = np.stack([T[k] - (R[k] @ R[1].T) @ T[1] + rng.normal(size=3) * 0.05 for k in others])
    e = _edges([1] * 40, others, M, m, [[W_ROT, 5.0]] * 40, [pg.EDGE_METRIC] * 40)
    return dict(R_abs=R, T_abs=T, graphs=[list(range(n))], edges=[e])


def reversed_and_duplicates():
    """5: every second chain edge given as (j, i) with the inverse measurement, and the loop edges given twice"""
    sc = loop_scene(12, 2, 7)
    e = {k: v.copy() for k, v in sc['edges'][0].items()}
    for k in range(0, 11, 2):
        M, m = e['R'][k].copy(), e['t'][k].copy()
        e['i'][k], e['j'][k] = e['j'][k], e['i'][k]
        e['R'][k] = M.T; e['t'][k] = -M.T @ m
    dup = {k: np.concatenate([v, v[11:]]) for k, v in e.items()}
    return _case(dict(sc, edges=[dup]))


def fixed_middle():
    """6: fixed frames in the middle of the loop"""
    fx = np.zeros(12, np.uint8); fx[[5, 9]] = 1
    return _case(loop_scene(12, 2, 8), fixed=[fx])


def unreachable():
    """7: frames 8 .. 11 are joined to each other and to no fixed frame: inactive, their edges unused"""
    sc = loop_scene(12, 2, 9)
    e = sc['edges'][0]
    keep = np.flatnonzero(~((e['i'] < 8) ^ (e['j'] < 8)))                   # no edge between the two parts
    e = {k: v[keep] for k, v in e.items()}
    e['R'][0] = mm.rodrigues([0.0, 0.03, 0.0]) @ e['R'][0]                  # something to do in the active part
    return _case(dict(sc, edges=[e]))


def three_graphs():
    """8: three graphs of different sizes in one call; frame 11 is the last of the first and the fixed one of the second; the
    third names its frames in descending order"""
    sc = loop_scene(30, 3, 10)
    all_e = sc['edges'][0]
    graphs = [list(range(0, 12)), list(range(11, 19)), [25, 24, 23, 22, 21, 20]]
    edges = geometry.edges_of_graphs(graphs, all_e)
    for g, (a, b) in enumerate(((0, 11), (11, 18), (25, 20))):              # a loop edge of each graph's own, off the chain
        Ra, Rb, Ta, Tb = sc['R_true'][a], sc['R_true'][b], sc['T_true'][a], sc['T_true'][b]
        M = Rb @ Ra.T
        m = Tb - M @ Ta
        extra = _edges([a], [b], [M], [m / np.linalg.norm(m)], [[W_ROT, W_DIR]], [pg.EDGE_DIRECTION])
        edges[g] = {k: np.concatenate([edges[g][k], extra[k]]) for k in extra}
    return dict(R_abs=sc['R_abs'], T_abs=sc['T_abs'], graphs=graphs, edges=edges)


def coincident():
    """9: a direction edge between coincident centres: its three translation rows and their derivatives are zero at the first
    linearisation.  The metric edge (1, 2) pulls frame 2 along the measured direction, so the rows that come alive with the
    first step are small"""
    R = np.stack([np.eye(3), mm.rodrigues([0.0, 0.2, 0.0]), mm.rodrigues([0.1, 0.0, -0.1])])
    T = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.5], [0.0, 0.0, 0.0]])
    M01 = mm.rodrigues([0.0, 0.22, 0.01]); M12 = mm.rodrigues([0.01, 0.0, 0.0]) @ R[2] @ R[1].T
    e = _edges([0, 1, 0], [1, 2, 2], [M01, M12, R[2]], [[1.1, 0.0, 0.5], T[2] - (R[2] @ R[1].T) @ T[1] + np.array([0.0, 0.0, 0.05]), [0.0, 0.0, 1.0]],
               [[W_ROT, 10.0], [W_ROT, 10.0], [W_ROT, W_DIR]], [pg.EDGE_METRIC, pg.EDGE_METRIC, pg.EDGE_DIRECTION])
    return dict(R_abs=R, T_abs=T, graphs=[[0, 1, 2]], edges=[e])


def rotation_170():
    """10: a measured rotation 170 degrees from the start: the chordal rows still pull the right way"""
    R = np.stack([np.eye(3), np.eye(3)]); T = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]])
    e = _edges([0], [1], [mm.rodrigues([0.0, 0.0, np.deg2rad(170.0)])], [[1.0, 0.0, 0.0]], [[W_ROT, 10.0]], [pg.EDGE_METRIC])
    return dict(R_abs=R, T_abs=T, graphs=[[0, 1]], edges=[e], max_iters=40)


def huber_wrong_edges():
    """11: Huber on, three wrong loop edges, and the bound set to the s of the first loop edge at the input: exactly at the
    bound it still has weight 1"""
    sc = loop_scene(24, 3, 11, wrong=3)
    e = sc['edges'][0]
    k = 23                                                                  # the first loop edge
    R, T = sc['R_abs'], sc['T_abs']
    i, j = e['i'][k:k + 1], e['j'][k:k + 1]
    res = pg.edge_rows(R[i], T[i], R[j], T[j], e['R'][k:k + 1], e['t'][k:k + 1], e['w'][k:k + 1, 0], e['w'][k:k + 1, 1], e['kind'][k:k + 1], jac=False)
    bound = float(pg.huber_terms(res, 0.0)[0][0])
    return _case(sc, huber=bound)


def codes():
    """12: every code in one call: NO_EDGES (no edges at all; an edge between two fixed frames only), UNDERDETERMINED (a free
    frame held by rotation-only edges), REJECTED (an exact, noise-free start: the gradient is zero to the bit), OK"""
    I = np.eye(3)
    R = np.stack([I] * 10); T = np.array([[float(f), 2.0 * f, 0.0] for f in range(10)])
    R[9] = mm.rodrigues([0.0, 0.1, 0.0])
    none = _edges([], [], np.zeros((0, 3, 3)), np.zeros((0, 3)), np.zeros((0, 2)), [])
    both_fixed = _edges([2], [3], [I], [[1.0, 2.0, 0.0]], [[W_ROT, 10.0]], [pg.EDGE_METRIC])
    rot_only = _edges([4, 5], [5, 6], [I, mm.rodrigues([0.0, 0.0, 0.01])], [[1.0, 2.0, 0.0], [1.0, 2.0, 0.0]], [[W_ROT, 10.0], [W_ROT, 0.0]],
                      [pg.EDGE_METRIC, pg.EDGE_METRIC])
    exact = _edges([0, 1], [1, 2], [I, I], [[1.0, 2.0, 0.0], [1.0, 2.0, 0.0]], [[W_ROT, 10.0]] * 2, [pg.EDGE_METRIC] * 2)
    ok = _edges([7, 8], [8, 9], [I, I], [[1.0, 2.0, 0.1], [1.0, 2.0, 0.0]], [[W_ROT, 10.0]] * 2, [pg.EDGE_METRIC] * 2)
    return dict(R_abs=R, T_abs=T, graphs=[[0, 1], [2, 3], [4, 5, 6], [0, 1, 2], [7, 8, 9]], edges=[none, both_fixed, rot_only, exact, ok],
                fixed=[None, np.array([0, 1], np.uint8), None, None, None])


CODES_EXPECTED = [pg.GRAPH_NO_EDGES, pg.GRAPH_NO_EDGES, pg.GRAPH_UNDERDETERMINED, pg.GRAPH_REJECTED, pg.GRAPH_OK]

CASES = {"two_frames": two_frames, "loop12": loop12, "big300": big300, "hub": hub, "reversed_and_duplicates": reversed_and_duplicates,
         "fixed_middle": fixed_middle, "unreachable": unreachable, "three_graphs": three_graphs, "coincident": coincident,
         "rotation_170": rotation_170, "huber_wrong_edges": huber_wrong_edges, "codes": codes}

_MODEL = {}


def model_result(name):
    """pose_graph_model.optimise of a case, computed once and shared"""
    if name not in _MODEL:
        _MODEL[name] = pg.optimise(**CASES[name]())
    return _MODEL[name]
