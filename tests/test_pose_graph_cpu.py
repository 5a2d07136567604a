"""tests/pose_graph_model.py, the float64 model of rpe_optimise_graphs, on its own: its Jacobians against central differences,
the Cayley map, what the hand-built cases of tests/pose_graph_cases.py are meant to show, and the accuracy table of DESIGN
section 8 (printed; run with -s to see it).  No GPU, no library."""
import numpy as np
import pytest

from tests import bundle_math_model as mm
from tests import pose_graph_cases as pc
from tests import pose_graph_model as pg


def _rot(rng, s=3.0):
    ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
    return mm.rodrigues(ax * rng.uniform(-s, s))


def test_jacobians_agree_with_central_differences():
    """every column of both Jacobians of both kinds of edge, the update being the rule's own (Cayley, T + d)"""
    rng = np.random.default_rng(1)
    n, eps = 200, 1e-6
    Ri = np.stack([_rot(rng) for _ in range(n)]); Rj = np.stack([_rot(rng) for _ in range(n)])
    Ti = rng.uniform(-5, 5, (n, 3)); Tj = rng.uniform(-5, 5, (n, 3))
    M = np.stack([_rot(rng) for _ in range(n)]); m = rng.normal(size=(n, 3))
    wr = rng.uniform(10, 200, n); wt = rng.uniform(0.5, 50, n); kind = np.arange(n) % 2
    r, JiW, JjW, JiD, JjD = pg.edge_rows(Ri, Ti, Rj, Tj, M, m, wr, wt, kind)
    assert (kind == pg.EDGE_DIRECTION).sum() == n // 2

    def rows(dwi, ddi, dwj, ddj):
        return pg.edge_rows(pg.cayley(dwi, Ri), Ti + ddi, pg.cayley(dwj, Rj), Tj + ddj, M, m, wr, wt, kind, jac=False)

    Z = np.zeros((n, 3))
    scale = np.abs(r).max() + 1.0
    for c in range(3):
        d = Z.copy(); d[:, c] = eps
        for which, (JW, JD) in enumerate(((JiW, JiD), (JjW, JjD))):
            args_w = [(d, Z, Z, Z), (Z, Z, d, Z)][which]; args_d = [(Z, d, Z, Z), (Z, Z, Z, d)][which]
            neg = lambda a: tuple(-x for x in a)
            fd_w = (rows(*args_w) - rows(*neg(args_w))) / (2 * eps)
            fd_d = (rows(*args_d) - rows(*neg(args_d))) / (2 * eps)
            assert np.abs(fd_w - JW[:, :, c]).max() <= 1e-6 * scale * 10, (which, c)
            assert np.abs(fd_d[:, 9:] - JD[:, :, c]).max() <= 1e-6 * scale * 10, (which, c)
            assert np.abs(fd_d[:, :9]).max() == 0.0                          # the rotation rows do not see d: structurally zero


def test_cayley_map_is_a_rotation_and_agrees_with_exp_to_second_order():
    rng = np.random.default_rng(2)
    n = 500
    w = rng.normal(size=(n, 3)) * 10.0 ** rng.uniform(-6, 2, (n, 1))
    C = pg.cayley(w, np.tile(np.eye(3), (n, 1, 1)))
    assert np.abs(np.einsum("nab,ncb->nac", C, C) - np.eye(3)).max() < 1e-13
    assert np.abs(np.linalg.det(C) - 1.0).max() < 1e-13
    small = rng.normal(size=(50, 3)) * 1e-2
    for v, c in zip(small, pg.cayley(small, np.tile(np.eye(3), (50, 1, 1)))):
        assert np.abs(c - mm.rodrigues(v)).max() < 2.0 * np.linalg.norm(v) ** 3      # third-order difference


def test_reduction_rule_sums_every_item_once():
    rng = np.random.default_rng(3)
    for n in (0, 1, 63, 64, 255, 256, 257, 300, 513, 1100):
        v = rng.integers(-1000, 1000, n).astype(np.float64)                  # integers: every order gives the same sum
        assert pg.reduce256(v) == v.sum()
    v = rng.normal(size=700)
    assert abs(pg.reduce256(v) - v.sum()) < 1e-10


# ---------------------------------------------------------------- the hand-built cases do what they are meant to
@pytest.mark.parametrize("name", [n for n in pc.CASES if n != "codes"])
def test_case_is_solved_and_lowers_its_cost(name):
    out = pc.model_result(name)
    assert (out['code'] == pg.GRAPH_OK).all(), out['code']
    assert (out['accepted'] >= 1).all() and (out['cost'][:, 1] < out['cost'][:, 0]).all()
    case = pc.CASES[name]()
    for g, frames in enumerate(case['graphs']):
        assert pg_bits(out['R'][g][0], case['R_abs'][frames[0]]) and pg_bits(out['T'][g][0], case['T_abs'][frames[0]])
        assert np.abs(np.einsum("nab,ncb->nac", out['R'][g], out['R'][g]) - np.eye(3)).max() < 1e-12


def pg_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float64).view(np.uint64), np.ascontiguousarray(b, np.float64).view(np.uint64))


def test_cases_reach_the_paths_they_name():
    big = pc.model_result("big300")
    assert big['free'][0] == 300 and big['used_edges'][0] == 306 and big['iterations'][0] <= 3
    hub = pc.model_result("hub")
    assert hub['free'][0] == 40 and hub['used_edges'][0] == 40
    dup = pc.model_result("reversed_and_duplicates")
    assert dup['used_edges'][0] == 11 + 4
    fx = pc.model_result("fixed_middle"); case = pc.CASES["fixed_middle"]()
    assert fx['free'][0] == 9
    for p in (5, 9):
        assert pg_bits(fx['R'][0][p], case['R_abs'][p]) and pg_bits(fx['T'][0][p], case['T_abs'][p])
    un = pc.model_result("unreachable"); case = pc.CASES["unreachable"]()
    assert un['free'][0] == 7 and un['unused_edges'][0] == 3 and (un['edge_used'][0][-3:] == 0).all()
    assert pg_bits(un['R'][0][8:], case['R_abs'][8:]) and pg_bits(un['T'][0][8:], case['T_abs'][8:])
    assert (un['edge_chi'][0][-3:] == 0).all()
    three = pc.model_result("three_graphs")
    assert three['frames'].tolist() == [12, 8, 6]
    assert not pg_bits(three['R'][0][11], three['R'][1][0])                  # the shared frame: moved in one graph, fixed in the other
    co = pc.model_result("coincident"); case = pc.CASES["coincident"]()
    e = case['edges'][0]
    r = pg.edge_rows(case['R_abs'][[0]], case['T_abs'][[0]], case['R_abs'][[2]], case['T_abs'][[2]], e['R'][2:], e['t'][2:], e['w'][2:, 0],
                     e['w'][2:, 1], e['kind'][2:], jac=False)
    assert (r[0, 9:] == 0.0).all() and co['edge_chi'][0][2, 1] > 0.0
    r170 = pc.model_result("rotation_170"); case = pc.CASES["rotation_170"]()
    assert mm.rot_angle_deg(r170['R'][0][1], case['edges'][0]['R'][0]) < 1.0     # from 170 degrees away


def test_huber_case_has_an_edge_exactly_at_the_bound_and_downweights_the_wrong_edges():
    case = pc.CASES["huber_wrong_edges"]()
    out = pc.model_result("huber_wrong_edges")
    chi = out['edge_chi'][0]
    assert chi[23, 0] == case['huber']                                       # s <= huber: weight 1 at the first linearisation
    assert (chi[26:, 1] > case['huber']).all() and (chi[26:, 1] > 10 * np.median(chi[:26, 1])).all()   # the wrong edges stand out


def test_every_code():
    out = pc.model_result("codes"); case = pc.CASES["codes"]()
    assert out['code'].tolist() == pc.CODES_EXPECTED
    assert out['used_edges'].tolist() == [0, 0, 2, 2, 2] and out['unused_edges'].tolist() == [0, 1, 0, 0, 0]
    assert out['iterations'].tolist()[:4] == [0, 0, 0, 20] and out['accepted'].tolist()[:4] == [0, 0, 0, 0]
    assert out['cost'][3].tolist() == [0.0, 0.0] and out['pcg_iterations'][3] == 0
    for g in range(4):                                                      # every code but OK returns the input bits
        fr = case['graphs'][g]
        assert pg_bits(out['R'][g], case['R_abs'][fr]) and pg_bits(out['T'][g], case['T_abs'][fr])
        assert pg_bits(out['edge_chi'][g][:, 0], out['edge_chi'][g][:, 1])


# ---------------------------------------------------------------- the accuracy table
SEEDS = (5, 6, 7)
SCENES = {"48 frames, 6 loops": dict(n=48, loops=6), "12 frames, 2 loops": dict(n=12, loops=2)}


def _run_scene(seed, huber, wrong, n, loops):
    sc = pc.loop_scene(n, loops, seed, wrong=wrong)
    out = pg.optimise(sc['R_abs'], sc['T_abs'], sc['graphs'], sc['edges'], huber=huber)
    before = pc.scene_errors(sc['R_abs'], sc['T_abs'], sc['R_true'], sc['T_true'])
    after = pc.scene_errors(out['R'][0], out['T'][0], sc['R_true'], sc['T_true'])
    return before, after, out


@pytest.fixture(scope="module")
def table():
    rows = {}
    for name, kw in SCENES.items():
        for wrong in (0, 3):
            if wrong and kw['n'] != 48:
                continue
            for seed in SEEDS:
                for huber in (0.0, 2.0):
                    rows[(name, wrong, seed, huber)] = _run_scene(seed, huber, wrong, **kw)
    return rows


def test_accuracy_table(table):
    print("\nscene | wrong edges | seed | rot deg median/worst: chain -> plain -> Huber 2 | centre median/worst: chain -> plain -> Huber 2"
          " | LM steps, PCG iterations: plain, Huber")
    for (name, wrong, seed, huber), (before, _, _) in table.items():
        if huber != 0.0:
            continue
        _, ap, op = table[(name, wrong, seed, 0.0)]; _, ah, oh = table[(name, wrong, seed, 2.0)]
        f = lambda e: "%.2f/%.2f" % (np.median(e), e.max())
        print("%s | %d | %d | %s -> %s -> %s | %s -> %s -> %s | %d, %d; %d, %d" % (
            name, wrong, seed, f(before[0]), f(ap[0]), f(ah[0]), f(before[1]), f(ap[1]), f(ah[1]),
            op['accepted'][0], op['pcg_iterations'][0], oh['accepted'][0], oh['pcg_iterations'][0]))
    clean = [k for k in table if k[1] == 0 and k[3] == 0.0]
    assert len({k[2] for k in clean}) >= 3
    pooled_before = np.concatenate([table[k][0][0] for k in clean]); pooled_after = np.concatenate([table[k][1][0] for k in clean])
    assert np.median(pooled_after) < np.median(pooled_before)
    wrong_plain = np.concatenate([table[k][1][0] for k in table if k[1] == 3 and k[3] == 0.0])
    wrong_huber = np.concatenate([table[k][1][0] for k in table if k[1] == 3 and k[3] == 2.0])
    assert np.median(wrong_huber) < np.median(wrong_plain)
