"""A float64 model of rpe_optimise_graphs, written from the rule in include/rpe_amd.h ("pose graphs"), not from the kernel:
the active set, the twelve rows of an edge with their Jacobians, the Huber weight, the explicit block-sparse normal equations,
the block-Jacobi PCG, the Cayley update, the Levenberg-Marquardt loop (bundle_math_model.lm_loop) and the codes.

The rule promises equal bits, so the model keeps every association: a 3-vector dot product is (a0*b0 + a1*b1) + a2*b2,
every other sum starts at +0.0 and adds in ascending order, a frame's gather runs over its used edges in ascending number, and
every reduction over a graph's frames or edges runs lane-strided over 256 lanes, then the butterfly inside each wave of 64,
then the four wave totals (reduce256).  It is vectorised over edges and frames with elementwise NumPy operations only, one
rounding per operation, which keeps the bits."""
import numpy as np

from tests import bundle_math_model as mm

GRAPH_OK, GRAPH_NO_EDGES, GRAPH_UNDERDETERMINED, GRAPH_REJECTED = 0, 1, 2, 3
EDGE_METRIC, EDGE_DIRECTION = 0, 1


def _dot3(a0, a1, a2, b0, b1, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


def _sum(terms):
    """+0.0, then the terms in ascending order"""
    acc = np.zeros_like(np.asarray(terms[0], np.float64))
    for t in terms:
        acc = acc + t
    return acc


def reduce256(items):
    """the reduction of the rule over one value per item"""
    items = np.asarray(items, np.float64).reshape(-1)
    part = np.zeros(256)
    with np.errstate(all="ignore"):
        for c in range(0, len(items), 256):
            chunk = items[c:c + 256]
            part[:len(chunk)] = part[:len(chunk)] + chunk
        v = part.reshape(4, 64)
        lane = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            v = v + v[:, lane ^ o]
        return float(((v[0, 0] + v[1, 0]) + v[2, 0]) + v[3, 0])


def cayley(w, R):
    """C(w) R over n frames: w (n, 3), R (n, 3, 3)"""
    w = np.asarray(w, np.float64).reshape(-1, 3); R = np.asarray(R, np.float64).reshape(-1, 3, 3)
    with np.errstate(all="ignore"):
        a0, a1, a2 = w[:, 0] / 2.0, w[:, 1] / 2.0, w[:, 2] / 2.0
        n2 = _dot3(a0, a1, a2, a0, a1, a2)
        f = 2.0 / (1.0 + n2)
        C = np.zeros((len(w), 3, 3))
        C[:, 0, 0] = 1.0 + f * (a0 * a0 - n2); C[:, 0, 1] = f * (a0 * a1 - a2); C[:, 0, 2] = f * (a0 * a2 + a1)
        C[:, 1, 0] = f * (a1 * a0 + a2); C[:, 1, 1] = 1.0 + f * (a1 * a1 - n2); C[:, 1, 2] = f * (a1 * a2 - a0)
        C[:, 2, 0] = f * (a2 * a0 - a1); C[:, 2, 1] = f * (a2 * a1 + a0); C[:, 2, 2] = 1.0 + f * (a2 * a2 - n2)
        Rn = np.zeros_like(R)
        for r in range(3):
            for c in range(3):
                Rn[:, r, c] = _dot3(C[:, r, 0], C[:, r, 1], C[:, r, 2], R[:, 0, c], R[:, 1, c], R[:, 2, c])
    return Rn


def edge_rows(Ri, Ti, Rj, Tj, M, m, w_rot, w_trans, kind, jac=True):
    """The rows of n edges: r (n, 12); with jac JiW, JjW (n, 12, 3): the rows by w_i, w_j, and JiD, JjD (n, 3, 3): the
    translation rows by d_i, d_j (the rotation rows' d columns are structurally zero and are not held)"""
    n = len(Ri)
    kind = np.asarray(kind)
    with np.errstate(all="ignore"):
        Q = np.zeros((n, 3, 3)); D = np.zeros((n, 3, 3))
        for r in range(3):
            for c in range(3):
                Q[:, r, c] = _dot3(Rj[:, r, 0], Rj[:, r, 1], Rj[:, r, 2], Ri[:, c, 0], Ri[:, c, 1], Ri[:, c, 2])
        q = np.stack([_dot3(Q[:, r, 0], Q[:, r, 1], Q[:, r, 2], Ti[:, 0], Ti[:, 1], Ti[:, 2]) for r in range(3)], 1)
        p = Tj - q
        for r in range(3):
            for c in range(3):
                D[:, r, c] = _dot3(Q[:, r, 0], Q[:, r, 1], Q[:, r, 2], M[:, c, 0], M[:, c, 1], M[:, c, 2])
        a = w_rot / np.sqrt(2.0)
        res = np.zeros((n, 12))
        JiW = np.zeros((n, 12, 3)); JjW = np.zeros((n, 12, 3)); JiD = np.zeros((n, 3, 3)); JjD = np.zeros((n, 3, 3))
        for k in range(3):
            k1, k2 = (k + 1) % 3, (k + 2) % 3
            for r in range(3):
                res[:, 3 * k + r] = a * (D[:, r, k] - (1.0 if r == k else 0.0))
            if jac:
                v0, v1, v2 = a * D[:, 0, k], a * D[:, 1, k], a * D[:, 2, k]
                JjW[:, 3 * k, 1] = v2; JjW[:, 3 * k, 2] = -v1
                JjW[:, 3 * k + 1, 0] = -v2; JjW[:, 3 * k + 1, 2] = v0
                JjW[:, 3 * k + 2, 0] = v1; JjW[:, 3 * k + 2, 1] = -v0
                for r in range(3):
                    for c in range(3):
                        JiW[:, 3 * k + r, c] = a * (D[:, r, k2] * M[:, k1, c] - D[:, r, k1] * M[:, k2, c])
        Pj = np.zeros((n, 3, 3)); Pi = np.zeros((n, 3, 3))
        Pj[:, 0, 1] = -q[:, 2]; Pj[:, 0, 2] = q[:, 1]; Pj[:, 1, 0] = q[:, 2]; Pj[:, 1, 2] = -q[:, 0]; Pj[:, 2, 0] = -q[:, 1]; Pj[:, 2, 1] = q[:, 0]
        for r in range(3):
            Pi[:, r, 0] = Q[:, r, 2] * Ti[:, 1] - Q[:, r, 1] * Ti[:, 2]
            Pi[:, r, 1] = Q[:, r, 0] * Ti[:, 2] - Q[:, r, 2] * Ti[:, 0]
            Pi[:, r, 2] = Q[:, r, 1] * Ti[:, 0] - Q[:, r, 0] * Ti[:, 1]
        # metric
        met = kind == EDGE_METRIC
        nn = np.sqrt(_dot3(p[:, 0], p[:, 1], p[:, 2], p[:, 0], p[:, 1], p[:, 2]))
        live = nn > 0.0                                                     # direction rows exist
        mn = np.sqrt(_dot3(m[:, 0], m[:, 1], m[:, 2], m[:, 0], m[:, 1], m[:, 2]))
        u = p / nn[:, None]
        zero = np.zeros(n)
        for r in range(3):
            rm = w_trans * (p[:, r] - m[:, r])
            rd = w_trans * (u[:, r] - m[:, r] / mn)
            res[:, 9 + r] = np.where(met, rm, np.where(live, rd, zero))
            if jac:
                N = [((1.0 if r == c else 0.0) - u[:, r] * u[:, c]) / nn for c in range(3)]
                for c in range(3):
                    jm = w_trans * Pj[:, r, c]; im = w_trans * Pi[:, r, c]
                    jd = w_trans * _dot3(N[0], N[1], N[2], Pj[:, 0, c], Pj[:, 1, c], Pj[:, 2, c])
                    idr = w_trans * _dot3(N[0], N[1], N[2], Pi[:, 0, c], Pi[:, 1, c], Pi[:, 2, c])
                    JjW[:, 9 + r, c] = np.where(met, jm, np.where(live, jd, zero))
                    JiW[:, 9 + r, c] = np.where(met, im, np.where(live, idr, zero))
                    djm = w_trans if r == c else zero
                    JjD[:, r, c] = np.where(met, djm, np.where(live, w_trans * N[c], zero))
                    dim_ = -(w_trans * Q[:, r, c])
                    did = -(w_trans * _dot3(N[0], N[1], N[2], Q[:, 0, c], Q[:, 1, c], Q[:, 2, c]))
                    JiD[:, r, c] = np.where(met, dim_, np.where(live, did, zero))
    if jac:
        return res, JiW, JjW, JiD, JjD
    return res


def huber_terms(res, huber):
    """(s, h, cost term) per edge"""
    with np.errstate(all="ignore"):
        s2 = _sum([res[:, k] * res[:, k] for k in range(12)])
        s = np.sqrt(s2)
        plain = (s <= huber) | (huber == 0.0)
        h = np.where(plain, 1.0, huber / s)
        c = np.where(plain, s2, (2.0 * huber) * s - huber * huber)
    return s, h, c


def _col(W, D, row, a):
    return W[:, row, a] if a < 3 else D[:, row - 9, a - 3]


def block(h, AW, AD, BW, BD):
    """h A'B per edge (n, 6, 6): all 12 rows for two w columns, the translation rows otherwise"""
    out = np.zeros((len(h), 6, 6))
    with np.errstate(all="ignore"):
        for a in range(6):
            for b in range(6):
                rows = range(12) if a < 3 and b < 3 else range(9, 12)
                out[:, a, b] = h * _sum([_col(AW, AD, r, a) * _col(BW, BD, r, b) for r in rows])
    return out


def grad(h, W, D, res):
    out = np.zeros((len(h), 6))
    with np.errstate(all="ignore"):
        for a in range(6):
            rows = range(12) if a < 3 else range(9, 12)
            out[:, a] = h * _sum([_col(W, D, r, a) * res[:, r] for r in rows])
    return out


def _dot6(a, b):
    with np.errstate(all="ignore"):
        return _sum([a[:, k] * b[:, k] for k in range(6)])


def _matvec6(A, p):
    """rows of A (n, 6, 6) times p (n, 6)"""
    with np.errstate(all="ignore"):
        return np.stack([_sum([A[:, a, b] * p[:, b] for b in range(6)]) for a in range(6)], 1)


# ---------------------------------------------------------------- the active set
def active_set(F, fixed, ei, ej, w_trans):
    """fixed: bools per position (position 0 is forced); ei, ej: positions.  Returns a dict: fidx (free index per position or
    -1), free_pos, used (bool per edge), used_edge (positions in the edge list), adj: per free frame a list of
    (used-edge number, side, free index of the other end or -1) in ascending used-edge number, and the code found (or -1)"""
    fixed = np.array(fixed, bool).copy(); fixed[0] = True
    nb = [[] for _ in range(F)]
    for a, b in zip(ei, ej):
        nb[a].append(b); nb[b].append(a)
    active = fixed.copy()
    stack = list(np.flatnonzero(fixed))
    while stack:
        p = stack.pop()
        for q in nb[p]:
            if not active[q]:
                active[q] = True; stack.append(q)
    fidx = np.full(F, -1)
    free_pos = np.flatnonzero(active & ~fixed)
    fidx[free_pos] = np.arange(len(free_pos))
    used = np.zeros(len(ei), bool); used_edge = []
    adj = [[] for _ in free_pos]
    has_trans = np.zeros(len(free_pos), bool)
    for k, (a, b) in enumerate(zip(ei, ej)):
        if not (active[a] and active[b]) or (fidx[a] < 0 and fidx[b] < 0):
            continue
        u = len(used_edge); used[k] = True; used_edge.append(k)
        for side, (me, other) in enumerate(((a, b), (b, a))):
            if fidx[me] >= 0:
                adj[fidx[me]].append((u, side, fidx[other]))
                has_trans[fidx[me]] |= w_trans[k] > 0.0
    code = -1
    if not used_edge:
        code = GRAPH_NO_EDGES
    elif not has_trans.all():
        code = GRAPH_UNDERDETERMINED
    return dict(fidx=fidx, free_pos=free_pos, used=used, used_edge=np.array(used_edge, int), adj=adj, code=code)


# ---------------------------------------------------------------- one graph
def solve_graph(R0, T0, fixed, ei, ej, M, m, w, kind, huber=0.0, max_iters=20, cg_iters=32, cg_tol=1e-3):
    """One graph from its own arrays: R0 (F, 3, 3), T0 (F, 3), edges by graph position.  Returns a dict: R, T, counts[4],
    info[4], cost[2], chi (E, 2), used (E,)"""
    R0 = np.array(R0, np.float64).reshape(-1, 3, 3); T0 = np.array(T0, np.float64).reshape(-1, 3)
    F, E = len(R0), len(ei)
    ei = np.asarray(ei, int).reshape(-1); ej = np.asarray(ej, int).reshape(-1)
    M = np.asarray(M, np.float64).reshape(E, 3, 3); m = np.asarray(m, np.float64).reshape(E, 3)
    w = np.asarray(w, np.float64).reshape(E, 2); kind = np.asarray(kind, int).reshape(-1)
    A = active_set(F, np.zeros(F, bool) if fixed is None else fixed, ei, ej, w[:, 1])
    fpos, ue = A['free_pos'], A['used_edge']
    nf, nu = len(fpos), len(ue)
    ui, uj = ei[ue], ej[ue]
    uM, um, uwr, uwt, uk = M[ue], m[ue], w[ue, 0], w[ue, 1], kind[ue]
    chi = np.zeros((E, 2))
    counts = np.array([F, nf, nu, E - nu], np.int32)

    def rows(R, T, jac):
        return edge_rows(R[ui], T[ui], R[uj], T[uj], uM, um, uwr, uwt, uk, jac)

    def cost_of(R, T):
        s, _, c = huber_terms(rows(R, T, False), huber)
        return reduce256(c), s

    cost0, s0 = cost_of(R0, T0) if nu else (0.0, np.zeros(0))
    chi[ue, 0] = s0; chi[ue, 1] = s0
    out = dict(R=R0.copy(), T=T0.copy(), counts=counts, cost=np.array([cost0, cost0]), chi=chi, used=A['used'])
    if A['code'] >= 0:
        out['info'] = np.array([A['code'], 0, 0, 0], np.int32)
        return out
    # the adjacency as arrays: entry -> frame, used edge, side, other; depth d of frame k -> entry
    deg = np.array([len(a) for a in A['adj']])
    ent = np.full((nf, deg.max()), -1)
    au, aside, aother = [], [], []
    for k, lst in enumerate(A['adj']):
        for d, (u, side, o) in enumerate(lst):
            ent[k, d] = len(au); au.append(u); aside.append(side); aother.append(o)
    au = np.array(au); aside = np.array(aside, bool); aother = np.array(aother)
    st = dict(R=R0.copy(), T=T0.copy(), lin=None, x=None, Rn=None, Tn=None, npcg=0)

    def linearise():
        res, JiW, JjW, JiD, JjD = rows(st['R'], st['T'], True)
        _, h, _ = huber_terms(res, huber)
        Aii = block(h, JiW, JiD, JiW, JiD); Ajj = block(h, JjW, JjD, JjW, JjD); Aij = block(h, JiW, JiD, JjW, JjD)
        gi = grad(h, JiW, JiD, res); gj = grad(h, JjW, JjD, res)
        own = np.where(aside[:, None, None], Ajj[au], Aii[au])                 # per adjacency entry: the frame's side
        gown = np.where(aside[:, None], gj[au], gi[au])
        cross = np.where(aside[:, None, None], np.transpose(Aij[au], (0, 2, 1)), Aij[au])
        H = np.zeros((nf, 6, 6)); g = np.zeros((nf, 6))
        with np.errstate(all="ignore"):
            for d in range(ent.shape[1]):
                k = np.flatnonzero(deg > d)
                H[k] = H[k] + own[ent[k, d]]; g[k] = g[k] + gown[ent[k, d]]
        st['lin'] = (H, g, cross)

    def step(lam):
        if st['lin'] is None:
            linearise()
        H0, g, cross = st['lin']
        with np.errstate(all="ignore"):
            H = H0.copy()
            for a in range(6):
                H[:, a, a] = H[:, a, a] + lam * H[:, a, a]
            L, ok = mm.cholesky(H)
            if not ok.all():
                return False
            r = -g
            z = mm.cholesky_solve(L, r)
            p = z.copy(); x = np.zeros((nf, 6))
            rz = reduce256(_dot6(r, z)); rz0 = rz
            tol2 = cg_tol * cg_tol
            moved = False
            for _ in range(cg_iters):
                hp = _matvec6(H, p)
                for d in range(ent.shape[1]):
                    k = np.flatnonzero((deg > d))
                    e = ent[k, d]
                    sel = aother[e] >= 0
                    k, e = k[sel], e[sel]
                    if len(k):
                        hp[k] = hp[k] + _matvec6(cross[e], p[aother[e]])
                pHp = reduce256(_dot6(p, hp))
                if not (pHp > 0.0):
                    break
                alpha = np.float64(rz) / np.float64(pHp)
                x = x + alpha * p; r = r - alpha * hp
                z = mm.cholesky_solve(L, r)
                rzn = reduce256(_dot6(r, z))
                moved = True; st['npcg'] += 1
                if rzn <= tol2 * rz0:
                    break
                beta = np.float64(rzn) / np.float64(rz)
                p = z + beta * p
                rz = rzn
        st['x'] = x
        return moved

    def trial(lam):
        Rn, Tn = st['R'].copy(), st['T'].copy()
        Rn[fpos] = cayley(st['x'][:, :3], st['R'][fpos])
        with np.errstate(all="ignore"):
            Tn[fpos] = st['T'][fpos] + st['x'][:, 3:]
        st['Rn'], st['Tn'] = Rn, Tn
        return cost_of(Rn, Tn)[0]

    def step_norm():
        with np.errstate(all="ignore"):
            return float(np.sqrt(np.float64(reduce256(_dot6(st['x'], st['x'])))))

    def accept():
        st['R'], st['T'], st['lin'] = st['Rn'], st['Tn'], None

    cost, iters, acc = cost0, 0, 0
    if mm.finite(cost0):
        cost, iters, acc, _ = mm.lm_loop(cost0, max_iters, step, trial, step_norm, accept)
    take = acc > 0 and bool(np.isfinite(st['R'][fpos]).all() and np.isfinite(st['T'][fpos]).all())
    out['info'] = np.array([GRAPH_OK if take else GRAPH_REJECTED, iters, acc, st['npcg']], np.int32)
    if take:
        out['R'], out['T'] = st['R'], st['T']
        out['cost'] = np.array([cost0, cost])
        chi[ue, 1] = cost_of(st['R'], st['T'])[1]
    return out


# ---------------------------------------------------------------- the call
def optimise(R_abs, T_abs, graphs, edges, fixed=None, huber=0.0, max_iters=20, cg_iters=32, cg_tol=1e-3):
    """Engine.optimise_graphs on the CPU: graphs a list of frame lists, edges one dict per graph of 'i', 'j' (frame indices),
    'R', 't', 'w', 'kind'; fixed None or a list of byte arrays, one per graph.  Returns the same dict."""
    R_abs = np.asarray(R_abs, np.float64).reshape(-1, 3, 3); T_abs = np.asarray(T_abs, np.float64).reshape(-1, 3)
    res = []
    for g, frames in enumerate(graphs):
        frames = [int(f) for f in frames]
        pos = {f: p for p, f in enumerate(frames)}
        e = edges[g]
        ei = [pos[int(f)] for f in np.asarray(e['i']).reshape(-1)]; ej = [pos[int(f)] for f in np.asarray(e['j']).reshape(-1)]
        fx = None if fixed is None or fixed[g] is None else np.asarray(fixed[g]).reshape(-1) != 0
        res.append(solve_graph(R_abs[frames], T_abs[frames], fx, ei, ej, e['R'], e['t'], e['w'], e['kind'], huber, max_iters,
                               cg_iters, cg_tol))
    cat = lambda key, shape: np.concatenate([r[key].reshape(shape) for r in res]) if res else np.zeros(shape)
    counts = np.stack([r['counts'] for r in res]); info = np.stack([r['info'] for r in res])
    return {'R': [r['R'] for r in res], 'T': [r['T'] for r in res], 'code': info[:, 0], 'iterations': info[:, 1],
            'accepted': info[:, 2], 'pcg_iterations': info[:, 3], 'frames': counts[:, 0], 'free': counts[:, 1],
            'used_edges': counts[:, 2], 'unused_edges': counts[:, 3], 'cost': np.stack([r['cost'] for r in res]),
            'edge_chi': [r['chi'] for r in res], 'edge_used': [r['used'].astype(np.uint8) for r in res]}
