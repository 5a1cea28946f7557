"""NumPy oracle of pn_icp_information and pn_pose_graph_optimize, written from include/pointnet_hip.h (the multiway-registration
section): the information sums of a set of partners, the edge residual, its Jacobians, the Levenberg-Marquardt loop, and the
graphs the CPU and GPU tests share.  Vectorised over edges; the solve of a step is NumPy's Cholesky, so the oracle and the device
agree to rounding, not bit for bit."""
import functools

import numpy as np

MAX_ITERS, SINGULAR, BAD_EDGE = 1, 2, 4
TRIES = 10


# ---- small Lie-group helpers, vectorised over a leading axis ---------------------------------------------------
def hat(w):
    w = np.asarray(w, np.float64)
    o = np.zeros(w.shape[:-1] + (3, 3))
    o[..., 0, 1], o[..., 0, 2] = -w[..., 2], w[..., 1]
    o[..., 1, 0], o[..., 1, 2] = w[..., 2], -w[..., 0]
    o[..., 2, 0], o[..., 2, 1] = -w[..., 1], w[..., 0]
    return o


def _series(w, a, b):
    """I + a K + b K^2, K = [w]_x"""
    K = hat(w)
    return np.eye(3) + a[..., None, None] * K + b[..., None, None] * (K @ K)


def rodrigues(w):
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w, axis=-1)
    small = th < 1e-12
    t = np.where(small, 1.0, th)
    a = np.where(small, 1.0, np.sin(t) / t)
    b = np.where(small, 0.0, 2.0 * (np.sin(0.5 * t) / t) ** 2)
    return _series(w, a, b)


def D(delta):
    """the update D(delta) = [Rodrigues(delta_omega) | delta_v] as (.., 4, 4)"""
    delta = np.asarray(delta, np.float64)
    T = np.zeros(delta.shape[:-1] + (4, 4))
    T[..., :3, :3] = rodrigues(delta[..., :3])
    T[..., :3, 3] = delta[..., 3:]
    T[..., 3, 3] = 1.0
    return T


def inv(T):
    """the inverse of [R t] with R a rotation"""
    T = np.asarray(T, np.float64)
    o = np.zeros_like(T)
    Rt = np.swapaxes(T[..., :3, :3], -1, -2)
    o[..., :3, :3] = Rt
    o[..., :3, 3] = -(Rt @ T[..., :3, 3:4])[..., 0]
    o[..., 3, 3] = 1.0
    return o


def rotvec(R):
    """-> (omega, theta): s = vee(R - R^T) / 2, c = (tr R - 1) / 2, theta = atan2(|s|, c), omega = s theta / |s| (s when |s| < 1e-12)"""
    s = 0.5 * np.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], -1)
    c = 0.5 * (np.trace(R, axis1=-2, axis2=-1) - 1.0)
    sn = np.linalg.norm(s, axis=-1)
    th = np.arctan2(sn, c)
    f = np.where(sn < 1e-12, 1.0, th / np.where(sn < 1e-12, 1.0, sn))
    return s * f[..., None], th


def edge_error(X, edges, Z):
    """E_k = Z_k^-1 X_i^-1 X_j for every edge -> (E, 4, 4)"""
    X, Z = np.asarray(X, np.float64), np.asarray(Z, np.float64)
    return inv(Z) @ inv(X[edges[:, 0]]) @ X[edges[:, 1]]


def residuals(X, edges, Z):
    """-> (r (E, 6), E_k (E, 4, 4), theta (E,))"""
    Ek = edge_error(X, edges, Z)
    om, th = rotvec(Ek[:, :3, :3])
    return np.concatenate([om, Ek[:, :3, 3]], 1), Ek, th


def weights(edge_weight, E):
    if edge_weight is None:
        return np.ones(E)
    w = np.asarray(edge_weight, np.float64)
    return np.where(np.isfinite(w) & (w > 0.0), w, 0.0)


def cost(X, edges, Z, info, w):
    """sum_k w_k r_k^T Lambda_k r_k over the live edges"""
    live = w > 0.0
    r = residuals(X, edges[live], Z[live])[0]
    return float(np.sum(w[live] * np.einsum("ep,epq,eq->e", r, info[live], r)))


def jacobians(X, edges, Z):
    """-> (r (E, 6), J_i (E, 6, 6), J_j (E, 6, 6))"""
    r, Ek, th = residuals(X, edges, Z)
    small = th < 1e-4
    t = np.where(small, 1.0, th)
    b = np.where(small, 1.0 / 12.0, 1.0 / (t * t) - (1.0 + np.cos(t)) / (2.0 * t * np.sin(t)))
    Jj = np.zeros((len(edges), 6, 6))
    Jj[:, :3, :3] = _series(r[:, :3], np.full(len(edges), 0.5), b)
    Jj[:, 3:, 3:] = Ek[:, :3, :3]
    T = inv(X[edges[:, 1]]) @ X[edges[:, 0]]
    Ad = np.zeros((len(edges), 6, 6))
    Ad[:, :3, :3] = Ad[:, 3:, 3:] = T[:, :3, :3]
    Ad[:, 3:, :3] = hat(T[:, :3, 3]) @ T[:, :3, :3]
    return r, -Jj @ Ad, Jj


def check_edges(K, edges):
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    return bool(np.all((e >= 0) & (e < K)) and np.all(e[:, 0] != e[:, 1]))


def optimize(K, edges, Z, info, poses, edge_weight=None, max_iters=50, tol=1e-10, lambda0=1e-3):
    """pn_pose_graph_optimize -> (poses (K, 4, 4), cost (2,), iters, status)"""
    edges = np.asarray(edges, np.int64).reshape(-1, 2)
    Z, info = np.asarray(Z, np.float64), np.asarray(info, np.float64)
    X = np.array(poses, np.float64)
    if not check_edges(K, edges):
        return X, np.full(2, np.nan), 0, BAD_EDGE
    E, n = len(edges), 6 * (K - 1)
    w = weights(edge_weight, E)
    live = w > 0.0
    el, Zl, Wl = edges[live], Z[live], w[live, None, None] * info[live]
    c0 = c = cost(X, edges, Z, info, w)
    lam, it, status = float(lambda0), 0, MAX_ITERS
    rows = 6 * (el - 1)[:, :, None] + np.arange(6)                     # (E, 2, 6): the unknowns of an edge's two nodes
    while it < max_iters:
        it += 1
        r, Ji, Jj = jacobians(X, el, Zl)
        J = np.concatenate([Ji, Jj], 2)                                # (E, 6, 12)
        Hb = np.swapaxes(J, 1, 2) @ Wl @ J                             # (E, 12, 12)
        gb = (np.swapaxes(J, 1, 2) @ Wl @ r[:, :, None])[:, :, 0]      # (E, 12)
        idx = rows.reshape(-1, 12)
        ok = np.repeat(el > 0, 6, axis=1)                              # node 0 has no unknowns
        H, g = np.zeros((n, n)), np.zeros(n)
        m = ok[:, :, None] & ok[:, None, :]
        np.add.at(H, (np.broadcast_to(idx[:, :, None], m.shape)[m], np.broadcast_to(idx[:, None, :], m.shape)[m]), Hb[m])
        np.add.at(g, idx[ok], gb[ok])
        accepted, d = False, None
        for _ in range(TRIES):
            Hd = H + lam * np.diag(np.diag(H))
            try:
                if not np.all(np.isfinite(Hd)):
                    raise np.linalg.LinAlgError
                L = np.linalg.cholesky(Hd)
            except np.linalg.LinAlgError:
                return X, np.array([c0, c]), it, SINGULAR
            y = np.linalg.solve(L, -g)
            d = np.linalg.solve(L.T, y)
            Xn = X.copy()
            Xn[1:] = X[1:] @ D(d.reshape(K - 1, 6))
            Xn[1:, 3] = X[1:, 3]
            cn = cost(Xn, edges, Z, info, w)
            if cn <= c:
                X, c, lam, accepted = Xn, cn, max(lam / 10.0, 1e-12), True
                break
            lam *= 10.0
        if not accepted or np.abs(d).max() < tol:
            status = 0
            break
    return X, np.array([c0, c]), it, status


def information(q, d2=None):
    """the (29,) sums of pn_icp_information over the partners q (n, 3) fp32 with their d2 (n,) fp32 (default 0), and the same sums
    of the terms' magnitudes -> (sums, magnitudes)"""
    q = np.asarray(q, np.float32).astype(np.float64).reshape(-1, 3)
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    one, zero = np.ones(len(q)), np.zeros(len(q))
    t = np.stack([one, y * y + z * z, -(x * y), -(x * z), zero, -z, y, x * x + z * z, -(y * z), z, zero, -x, x * x + y * y, -y, x, zero,
                  one, zero, zero, one, zero, one] + [zero] * 6 + [zero if d2 is None else np.asarray(d2, np.float32).astype(np.float64)], 1)
    return t.sum(0), np.abs(t).sum(0)


def info_matrix(sums):
    """the symmetric (.., 6, 6) matrix of (.., 29) sums"""
    sums = np.asarray(sums)
    iu = np.triu_indices(6)
    M = np.zeros(sums.shape[:-1] + (6, 6))
    M[..., iu[0], iu[1]] = sums[..., 1:22]
    M[..., iu[1], iu[0]] = sums[..., 1:22]
    return M


# ---- the test graphs -----------------------------------------------------------------------------------------
def random_pose(rng, angle_deg, trans):
    a = rng.normal(size=3)
    a *= np.deg2rad(angle_deg) * rng.random() / np.linalg.norm(a)
    return D(np.concatenate([a, rng.uniform(-trans, trans, 3)]))


def _spd(rng, n=200):
    q = rng.uniform(-3, 3, (n, 3)).astype(np.float32)
    return info_matrix(information(q)[0])


def _edges(rng, K, E):
    """the chain (a, a + 1) and E - (K - 1) distinct further pairs i < j, a fixed draw"""
    chain = [(a, a + 1) for a in range(K - 1)]
    rest = [(i, j) for i in range(K) for j in range(i + 2, K)]
    pick = rng.permutation(len(rest))[:E - len(chain)]
    return np.array(chain + [rest[p] for p in sorted(pick)], np.int32)


@functools.lru_cache(maxsize=None)
def graph(K, E, kind="noisy", seed=0):
    """A graph of K nodes and E edges -> dict(K, edges (E, 2) int32, Z, info, truth (K, 4, 4), start (K, 4, 4)); shared, not to be
    written to.  ``kind``: "consistent" (exact edges, the start a perturbed truth), "noisy" (every edge off by up to 1 degree and
    5 cm, the start the composed chain), "drift" (the chain edges share one bias of 0.6 degrees and 3 cm, the loop closures are
    exact up to a tenth of the noise, the start the composed chain)."""
    rng = np.random.default_rng(1000 * K + E + seed)
    truth = np.stack([np.eye(4)] + [random_pose(rng, 60, 5) for _ in range(K - 1)])
    edges = _edges(rng, K, E)
    Z = inv(truth[edges[:, 0]]) @ truth[edges[:, 1]]
    info = np.stack([_spd(rng) for _ in range(E)])
    if kind == "consistent":
        start = truth.copy()
        for a in range(1, K):
            start[a] = truth[a] @ random_pose(rng, 5, 0.3)
    else:
        if kind == "noisy":
            Z = np.stack([z @ random_pose(rng, 1.0, 0.05) for z in Z])
        else:
            bias = D(np.concatenate([np.deg2rad(0.6) * np.array([0.5, -0.6, 0.62]), [0.03, -0.02, 0.01]]))
            Z = np.stack([z @ (bias if k < K - 1 else random_pose(rng, 0.1, 0.005)) for k, z in enumerate(Z)])
        start = np.stack([np.eye(4)] * K)
        for a in range(1, K):
            start[a] = start[a - 1] @ Z[a - 1]
    out = dict(K=K, edges=edges, Z=Z, info=info, truth=truth, start=start)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def numeric_gradient(X, edges, Z, info, w, h=1e-6):
    """the central-difference gradient of the true cost in the update's own parametrisation, (6 (K - 1),)"""
    K = len(X)
    g = np.zeros(6 * (K - 1))
    for a in range(1, K):
        for m in range(6):
            d = np.zeros(6)
            d[m] = h
            Xp, Xm = np.array(X), np.array(X)
            Xp[a], Xm[a] = X[a] @ D(d), X[a] @ D(-d)
            g[6 * (a - 1) + m] = (cost(Xp, edges, Z, info, w) - cost(Xm, edges, Z, info, w)) / (2 * h)
    return g


def node_error(X, truth):
    return float(np.abs(np.asarray(X) - truth).max())


def sensitivity(g, trials, **kw):
    """the problem's own sensitivity to last-bit changes of its input: the largest pose difference between the oracle's result and
    its results with every Z entry perturbed by a relative 2^-50, over ``trials`` fixed seeds -> (s, the unperturbed result)"""
    base = optimize(g["K"], g["edges"], g["Z"], g["info"], g["start"], **kw)
    s = 0.0
    for t in range(trials):
        rng = np.random.default_rng(77 + t)
        Zp = g["Z"] * (1.0 + rng.uniform(-1, 1, g["Z"].shape) * 2.0 ** -50)
        s = max(s, float(np.abs(optimize(g["K"], g["edges"], Zp, g["info"], g["start"], **kw)[0] - base[0]).max()))
    return s, base
