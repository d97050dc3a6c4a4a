"""References and input builders shared by the cone-projection tests (test_gpu_cone_proj.py, test_gpu_cone_dproj.py): numpy restatements of the closed forms,
inputs built AWAY from kinks by construction (never filtered), and the deliberate kink points."""
import numpy as np

from cvxpylayers_amd import problems as P
from oracle import oracle

RHOS = (-2.0, -0.5, 0.5, 2.0)          # t = rho ||z||: inside the polar, between (both signs of t), inside the cone
Q_DIMS = [1, 2, 5, 16, 17, 64, 65]     # both lane shapes of the kernel (<= 16: a 16-lane row, else a wave), one and two strides of 64
ROWS_SOC = {"z": 2, "l": 3, "q": Q_DIMS}
PSD_ORDERS = [[1], [2], [3, 5], [16], [17], [33], [39], [40]]      # tile edges of KP = 16 / 32 / 48; 40: the first order on the Jacobi path
TRIPLES = {"ep": 2, "p": [0.3, -0.6]}
SPECIAL_TRIPLES = [[0.0, 0.0, 0.0], [0.0, 1.0, 1.0], [1.0, 0.0, 0.0], [-1.0, 0.0, 2.0], [0.0, -1.0, 1.0], [0.0, 0.0, -1.0], [5.0, -3.0, 0.0],
                   [-0.144356093, 1.42172124e-04, -1.18506858e-02], [700.0, 1.0, 1.0], [-1e6, 1e-6, 1.0]]          # tests/test_expcone_host.py


def rows_of(cones):
    return P.cone_rows(cones)


# ---- zero / nonnegative rows and second-order cones -----------------------------------------------------------------------------------------------------
def soc_proj(v):
    t, z = v[0], v[1:]
    nz = np.linalg.norm(z)
    if len(v) == 1:
        return np.maximum(v, 0.0)
    if nz <= t:
        return v.copy()
    if nz <= -t:
        return np.zeros_like(v)
    c = 0.5 * (t + nz)
    return np.concatenate([[c], c * z / nz])


def soc_dproj(v, h):
    """D Pi(v) h, inclusive boundaries: the identity on the cone (and its boundary), 0 on the polar (and its boundary)"""
    t, z = v[0], v[1:]
    nz = np.linalg.norm(z)
    if len(v) == 1:
        return h.copy() if t >= 0 else np.zeros_like(h)
    if nz <= t:
        return h.copy()
    if nz <= -t:
        return np.zeros_like(h)
    zh = z / nz
    J = np.empty((len(v), len(v)))
    J[0, 0] = 0.5; J[0, 1:] = 0.5 * zh; J[1:, 0] = 0.5 * zh
    J[1:, 1:] = 0.5 * ((1 + t / nz) * np.eye(len(z)) - (t / nz) * np.outer(zh, zh))
    return J @ h


def rows_soc_input(rng, B, cones=ROWS_SOC):
    """(B, m): rows away from 0, every second-order cone at t = rho ||z|| with rho cycling through RHOS over cones and instances"""
    z, l = cones.get("z", 0), cones.get("l", 0)
    v = np.empty((B, rows_of(cones)))
    v[:, :z + l] = rng.standard_normal((B, z + l)) + np.where(rng.random((B, z + l)) < 0.5, -0.2, 0.2)
    v[:, :z + l] = np.where(np.abs(v[:, :z + l]) < 0.1, 0.3, v[:, :z + l])
    r = z + l
    for c, d in enumerate(cones.get("q", [])):
        for i in range(B):
            rho = RHOS[(c + i) % 4]
            zz = rng.standard_normal(d - 1) * 10 ** rng.uniform(-1, 1)
            v[i, r] = rho * np.linalg.norm(zz) if d > 1 else rho
            v[i, r + 1:r + d] = zz
        r += d
    return v


def rows_soc_ref(v, cones=ROWS_SOC, dual=False):
    z, l = cones.get("z", 0), cones.get("l", 0)
    out = np.empty_like(v)
    out[:, :z] = v[:, :z] if dual else 0.0
    out[:, z:z + l] = np.clip(v[:, z:z + l], 0.0, None)
    r = z + l
    for d in cones.get("q", []):
        for i in range(v.shape[0]):
            out[i, r:r + d] = soc_proj(v[i, r:r + d])
        r += d
    return out


def rows_soc_dref(v, h, cones=ROWS_SOC, dual=False):
    z, l = cones.get("z", 0), cones.get("l", 0)
    out = np.empty_like(v)
    out[:, :z] = h[:, :z] if dual else 0.0
    w = v[:, z:z + l]
    out[:, z:z + l] = np.where(w > 0, 1.0, np.where(w < 0, 0.0, 0.5)) * h[:, z:z + l]
    r = z + l
    for d in cones.get("q", []):
        for i in range(v.shape[0]):
            out[i, r:r + d] = soc_dproj(v[i, r:r + d], h[i, r:r + d])
        r += d
    return out


def soc_spans(cones):
    r = cones.get("z", 0) + cones.get("l", 0)
    spans = []
    for d in cones.get("q", []):
        spans.append((r, r + d)); r += d
    return spans


# ---- PSD blocks -----------------------------------------------------------------------------------------------------------------------------------------
def spectrum(kind, k, flip=1.0):
    i = np.arange(k)
    mixed = flip * np.where(i % 2 == 0, 1.0, -1.0) * (0.1 + 0.05 * i)       # |w_i| >= 0.1, gaps >= 0.05, both signs (k >= 2)
    if kind == "mixed":
        return mixed
    if kind == "positive":
        return 0.1 + 0.05 * i
    if kind == "negative":
        return -(0.1 + 0.05 * i)
    if kind == "zero":
        return np.zeros(k)
    if kind == "rank_one":
        return np.where(i == 0, 1.5, 0.0)
    if kind == "repeated":
        w = mixed.copy(); w[:min(k, 3)] = 0.7
        return w
    raise ValueError(kind)


def psd_matrices(rng, B, k, kind):
    """(B, k, k) symmetric S = Q diag(w) Q^T with the prescribed spectrum (sign pattern flipped on odd instances), and w"""
    S = np.empty((B, k, k)); W = np.empty((B, k))
    for b in range(B):
        Q, _ = np.linalg.qr(rng.standard_normal((k, k)))
        w = spectrum(kind, k, flip=1.0 if b % 2 == 0 else -1.0)
        S[b] = (Q * w) @ Q.T; S[b] = 0.5 * (S[b] + S[b].T); W[b] = w
    return S, W


def psd_proj(S):
    w, V = np.linalg.eigh(S)
    return (V * np.maximum(w, 0.0)[..., None, :]) @ np.swapaxes(V, -1, -2)


def psd_divdiff(w):
    """the convention: 1 for two positive eigenvalues, 0 for two non-positive ones, (p_i - p_j) / (w_i - w_j) otherwise"""
    p = np.maximum(w, 0.0)
    wi, wj = w[:, None], w[None, :]
    both_pos, both_non = (wi > 0) & (wj > 0), (wi <= 0) & (wj <= 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        D = (p[:, None] - p[None, :]) / (wi - wj)
    return np.where(both_pos, 1.0, np.where(both_non, 0.0, D))


def psd_dproj(S, H):
    w, V = np.linalg.eigh(S)
    return V @ (psd_divdiff(w) * (V.T @ H @ V)) @ V.T


def psd_input(rng, B, orders, kind):
    """v (B, m) for cones {"s": orders}, the matrices per block"""
    mats = [psd_matrices(rng, B, k, kind)[0] for k in orders]
    return np.concatenate([P.sym_to_svec(S) for S in mats], axis=1), mats


def psd_split(v, orders):
    out, r = [], 0
    for k in orders:
        n = k * (k + 1) // 2
        out.append(P.svec_to_sym(v[:, r:r + n], k)); r += n
    return out


# ---- exponential / power triples ------------------------------------------------------------------------------------------------------------------------
def triple_points(rng, n, cones=TRIPLES):
    nt = cones.get("ep", 0) + len(cones.get("p", []))
    return (rng.standard_normal((n, nt, 3)) * 10 ** rng.uniform(-2, 2, size=(n, nt, 1))).reshape(n, 3 * nt)


def triples_ref(v, cones=TRIPLES, dual=False):
    out = np.empty_like(v)
    nep = cones.get("ep", 0)
    for i in range(v.shape[0]):
        for c in range(v.shape[1] // 3):
            w = v[i, 3 * c:3 * c + 3]
            out[i, 3 * c:3 * c + 3] = oracle.proj_exp(w, dual=dual) if c < nep else oracle.proj_pow(w, cones["p"][c - nep], dual=dual)
    return out


def triples_jac(v, cones=TRIPLES, dual=False):
    """(n, ntri, 3, 3) oracle Jacobians"""
    nep = cones.get("ep", 0)
    nt = v.shape[1] // 3
    J = np.empty((v.shape[0], nt, 3, 3))
    for i in range(v.shape[0]):
        for c in range(nt):
            w = v[i, 3 * c:3 * c + 3]
            J[i, c] = oracle.dproj_exp(w, dual=dual) if c < nep else oracle.dproj_pow(w, cones["p"][c - nep], dual=dual)
    return J
