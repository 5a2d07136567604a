#!/usr/bin/env python3
"""What rpe_optimise_graphs costs ("Pose graphs"): the loop scene of tests/pose_graph_cases.py (a camera
on a circle, chain edges from geometry.chain_edges, direction loop edges) in three sizes:

  one48      one graph of 48 frames, 6 loop edges
  one1000    one graph of 1000 frames, 999 chain + 100 loop edges
  many48     64 graphs of 48 frames in one call (64 seeds)

The time per call is the host clock around the C call on arrays prepared once: it uploads the poses, the measurements and the
host's tables, runs pg_solve_kernel (one workgroup per graph) and ends in the wait of its fetch, every output fetched.
Warm-up calls first; median and min / max of the repetitions; two calls are asserted equal bit for bit.  The kernel's own
device time comes from `rocprofv3 --kernel-trace --stats -- python tools/bench_pose_graphs.py --no-dense`, in a run of its
own.  The comparison is a dense NumPy Levenberg-Marquardt on the same normal equations (the model's rows and blocks,
np.linalg.solve of the damped 6 n-square system per step instead of the PCG) on this machine's CPU.  Prints one JSON line.

    python tools/bench_pose_graphs.py [--reps 9] [--warmup 2] [--no-dense] [--huber 2.0]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _stats(v):
    v = np.asarray(v) * 1e3
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(v.min()), 4), "max_ms": round(float(v.max()), 4), "n": len(v)}


def dense_lm(case, huber, max_iters=20):
    """the model's rule with np.linalg.solve of the whole damped system in place of the PCG; one graph.  Returns (seconds in
    all, seconds inside np.linalg.solve, LM iterations, steps accepted, cost before, cost after)"""
    from tests import bundle_math_model as mm
    from tests import pose_graph_model as pg
    frames = case['graphs'][0]
    R, T = case['R_abs'][frames].copy(), case['T_abs'][frames].copy()
    e = case['edges'][0]
    pos = {f: p for p, f in enumerate(frames)}
    ei = np.array([pos[int(f)] for f in e['i']]); ej = np.array([pos[int(f)] for f in e['j']])
    n = len(frames) - 1                                                      # frame 0 fixed, every other free and active
    st = dict(R=R, T=T, solve_s=0.0, x=None)
    t0 = time.perf_counter()

    def rows(R, T, jac):
        return pg.edge_rows(R[ei], T[ei], R[ej], T[ej], e['R'], e['t'], e['w'][:, 0], e['w'][:, 1], e['kind'], jac)

    def cost_of(R, T):
        return float(pg.huber_terms(rows(R, T, False), huber)[2].sum())

    def step(lam):
        res, JiW, JjW, JiD, JjD = rows(st['R'], st['T'], True)
        h = pg.huber_terms(res, huber)[1]
        Aii, Ajj, Aij = pg.block(h, JiW, JiD, JiW, JiD), pg.block(h, JjW, JjD, JjW, JjD), pg.block(h, JiW, JiD, JjW, JjD)
        gi, gj = pg.grad(h, JiW, JiD, res), pg.grad(h, JjW, JjD, res)
        H = np.zeros((6 * n, 6 * n)); g = np.zeros(6 * n)
        for k in range(len(ei)):
            a, b = ei[k] - 1, ej[k] - 1
            if a >= 0:
                H[6 * a:6 * a + 6, 6 * a:6 * a + 6] += Aii[k]; g[6 * a:6 * a + 6] += gi[k]
            if b >= 0:
                H[6 * b:6 * b + 6, 6 * b:6 * b + 6] += Ajj[k]; g[6 * b:6 * b + 6] += gj[k]
            if a >= 0 and b >= 0:
                H[6 * a:6 * a + 6, 6 * b:6 * b + 6] += Aij[k]; H[6 * b:6 * b + 6, 6 * a:6 * a + 6] += Aij[k].T
        H[np.arange(6 * n), np.arange(6 * n)] *= 1.0 + lam
        t1 = time.perf_counter()
        try:
            st['x'] = np.linalg.solve(H, -g).reshape(n, 6)
        except np.linalg.LinAlgError:
            return False
        finally:
            st['solve_s'] += time.perf_counter() - t1
        return True

    def trial(lam):
        Rn, Tn = st['R'].copy(), st['T'].copy()
        Rn[1:] = pg.cayley(st['x'][:, :3], st['R'][1:]); Tn[1:] = st['T'][1:] + st['x'][:, 3:]
        st['Rn'], st['Tn'] = Rn, Tn
        return cost_of(Rn, Tn)

    def accept():
        st['R'], st['T'] = st['Rn'], st['Tn']

    c0 = cost_of(R, T)
    c1, iters, acc, _ = mm.lm_loop(c0, max_iters, step, trial, lambda: float(np.linalg.norm(st['x'])), accept)
    return time.perf_counter() - t0, st['solve_s'], iters, acc, c0, c1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--huber", type=float, default=2.0)
    ap.add_argument("--no-dense", action="store_true", help="skip the dense NumPy comparison (profiling runs)")
    a = ap.parse_args()

    from relative_pose_estimation_amd import _capi
    from tests import pose_graph_cases as pc

    def many(n_graphs, n, loops):
        scs = [pc.loop_scene(n, loops, 100 + s) for s in range(n_graphs)]
        edges = []
        for s, sc in enumerate(scs):
            e = {k: v.copy() for k, v in sc['edges'][0].items()}
            e['i'] = e['i'] + s * n; e['j'] = e['j'] + s * n
            edges.append(e)
        return dict(R_abs=np.concatenate([sc['R_abs'] for sc in scs]), T_abs=np.concatenate([sc['T_abs'] for sc in scs]),
                    graphs=[list(range(s * n, (s + 1) * n)) for s in range(n_graphs)], edges=edges)

    pick = lambda sc: {k: sc[k] for k in ('R_abs', 'T_abs', 'graphs', 'edges')}
    cases = {"one48": pick(pc.loop_scene(48, 6, 5)), "one1000": pick(pc.loop_scene(1000, 100, 5)), "many48": many(64, 48, 6)}
    e = _capi.Engine(640, 480, max_batch=1, nfeatures=64, max_matches=32)
    out = {"huber": a.huber, "max_iters": 20, "cg_iters": 32, "cg_tol": 1e-3}
    calls = {}
    for name, case in cases.items():
        res = e.optimise_graphs(huber=a.huber, **case)
        again = e.optimise_graphs(huber=a.huber, **case)
        for key in ("code", "iterations", "accepted", "pcg_iterations", "cost"):
            assert np.array_equal(np.ascontiguousarray(res[key]).view(np.uint8), np.ascontiguousarray(again[key]).view(np.uint8)), key
        assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(res["R"] + res["T"], again["R"] + again["T"]))
        out[name + "_job"] = {"graphs": len(case['graphs']), "frames": int(res['frames'].sum()), "edges": int(res['used_edges'].sum()),
                              "codes": dict(zip(_capi.GRAPH_NAMES, np.bincount(res['code'], minlength=4).tolist())),
                              "iterations_max": int(res['iterations'].max()), "accepted_sum": int(res['accepted'].sum()),
                              "pcg_max": int(res['pcg_iterations'].max()), "pcg_sum": int(res['pcg_iterations'].sum()),
                              "cost_before": float(res['cost'][:, 0].sum()), "cost_after": float(res['cost'][:, 1].sum())}
        # the arrays of the C call, prepared once
        gl = [np.asarray(g, np.int32) for g in case['graphs']]
        ed = case['edges']
        gs = np.zeros(len(gl) + 1, np.int32); gs[1:] = np.cumsum([len(g) for g in gl])
        es = np.zeros(len(gl) + 1, np.int32); es[1:] = np.cumsum([len(x['i']) for x in ed])
        cat = lambda k, dt: np.ascontiguousarray(np.concatenate([x[k] for x in ed]), dt)
        ins = [np.ascontiguousarray(case['R_abs'], np.float64), np.ascontiguousarray(case['T_abs'], np.float64), gs, np.concatenate(gl).astype(np.int32),
               es, cat('i', np.int32), cat('j', np.int32), cat('R', np.float64), cat('t', np.float64), cat('w', np.float64), cat('kind', np.int32)]
        nf, ne, ng = int(gs[-1]), int(es[-1]), len(gl)
        ob = [np.zeros((nf, 9)), np.zeros((nf, 3)), np.zeros((ng, 4), np.int32), np.zeros((ng, 4), np.int32), np.zeros((ng, 2)), np.zeros((ne, 2)),
              np.zeros(ne, np.uint8)]

        def call(ins=ins, ob=ob, ng=ng, nF=len(case['R_abs'])):
            p = [C.c_void_p(b.ctypes.data) for b in ins]
            rc = e.lib.rpe_optimise_graphs(e.h, nF, p[0], p[1], ng, p[2], p[3], None, p[4], p[5], p[6], p[7], p[8], p[9], p[10], a.huber, 20, 32, 1e-3,
                                           *[C.c_void_p(b.ctypes.data) for b in ob])
            assert rc == 0, e.lib.rpe_last_error(e.h)
        calls[name] = call
        out[name + "_job"]["bytes_up"] = int(sum(b.nbytes for b in ins)); out[name + "_job"]["bytes_down"] = int(sum(b.nbytes for b in ob))
    times = {name: [] for name in calls}
    for r in range(a.warmup + a.reps):
        for name, call in calls.items():
            t0 = time.perf_counter(); call(); t1 = time.perf_counter()
            if r >= a.warmup:
                times[name].append(t1 - t0)
    for name in calls:
        out[name] = _stats(times[name])
    e.close()
    if not a.no_dense:
        for name in ("one48", "one1000"):
            s, solve_s, iters, acc, c0, c1 = dense_lm(cases[name], a.huber)
            out[name + "_dense_numpy"] = {"total_s": round(s, 4), "solve_s": round(solve_s, 4), "iterations": iters, "accepted": acc,
                                          "solve_ms_per_step": round(1e3 * solve_s / max(iters, 1), 3), "cost_before": c0, "cost_after": c1}
        t0 = time.perf_counter()
        many_dense = [dense_lm(dict(cases["many48"], graphs=[g], edges=[ed]), a.huber) for g, ed in zip(cases["many48"]['graphs'], cases["many48"]['edges'])]
        out["many48_dense_numpy"] = {"total_s": round(time.perf_counter() - t0, 4), "solve_s": round(sum(m[1] for m in many_dense), 4),
                                     "iterations": int(sum(m[2] for m in many_dense))}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
