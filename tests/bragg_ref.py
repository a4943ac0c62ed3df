"""fp64 numpy restatement of the Bragg intensity (include/mtd_abi.h "Bragg intensity"; csrc/bragg.hip), straight from the definition:

    q_k   = 2 pi (h b1' + k b2' + l b3'),  b_i' the reciprocal rows of the global box (b_i' . a_j = delta_ij)
    rho_k = sum_j a(type_j) exp(i q_k . r_j),  A1 = sum_j |a_j|,  A2 = sum_j a_j^2
    s = sum_k w_k |rho_k|^2 / A1^2             (modulus: s = sum_k w_k |rho_k| / A1)
    S_k = |rho_k|^2 / A2
    ds/dr_j = a_j sum_k q_k (-alpha_k sin(q_k . r_j) + beta_k cos(q_k . r_j)),  (alpha_k, beta_k) = ds / d(Re, Im) rho_k

Nothing here is shared with the kernels: the phase is the plain Cartesian product q_k . r_j in radians, numpy's sin and cos.
`sums` / `from_sums` split the work the way a domain-decomposed run does: every rank sums its own particles, the 2K + 2 sums are added,
and value, S_k and coefficients follow from the totals.  lamellar_value restates cv.lamellar on the same inputs, for comparison."""
import numpy as np


def lattice(L, xy=0.0, xz=0.0, yz=0.0):
    """the lattice vectors a_1, a_2, a_3 of a HOOMD box as the rows of a matrix"""
    L = np.full(3, float(L)) if np.isscalar(L) else np.asarray(L, dtype=np.float64)
    return np.array([[L[0], 0.0, 0.0], [xy * L[1], L[1], 0.0], [xz * L[2], yz * L[2], L[2]]])


def wave_vectors(hkl, L, tilt=None):
    """q_k[K, 3] = 2 pi hkl . B with the rows of B reciprocal to the lattice vectors"""
    B = np.linalg.inv(lattice(L, **(tilt or {}))).T                       # rows b_i': b_i' . a_j = delta_ij
    return 2.0 * np.pi * np.asarray(hkl, dtype=np.float64).reshape(-1, 3) @ B


def sums(pos, types, coeff, hkl, L, tilt=None):
    """this rank's 2K + 2 sums: Re rho_0, Im rho_0, ..., A1, A2"""
    a = np.asarray(coeff, dtype=np.float64)[np.asarray(types, dtype=np.int64)] if len(pos) else np.zeros(0)
    phi = np.asarray(pos, dtype=np.float64).reshape(-1, 3) @ wave_vectors(hkl, L, tilt).T             # [N, K]
    out = np.empty(2 * phi.shape[1] + 2)
    out[0:-2:2] = (a[:, None] * np.cos(phi)).sum(axis=0)
    out[1:-2:2] = (a[:, None] * np.sin(phi)).sum(axis=0)
    out[-2], out[-1] = np.abs(a).sum(), (a * a).sum()
    return out


def from_sums(total, weights, modulus=False):
    """dict(s, S, rho, grad, A1, A2) from the (summed) 2K + 2 sums; rho and grad are [K, 2]"""
    total = np.asarray(total, dtype=np.float64)
    K = (len(total) - 2) // 2
    w = np.full(K, 1.0 / K) if weights is None else np.asarray(weights, dtype=np.float64)
    rho = total[:2 * K].reshape(K, 2).copy()
    A1, A2 = total[-2], total[-1]
    m2 = (rho * rho).sum(axis=1)
    m = np.sqrt(m2)
    if A1 == 0.0:
        return dict(s=0.0, S=np.zeros(K), rho=rho, grad=np.zeros((K, 2)), A1=A1, A2=A2, w=w)
    if modulus:
        s = float((w * m).sum() / A1)
        with np.errstate(invalid="ignore", divide="ignore"):
            grad = np.where(m[:, None] > 0.0, w[:, None] * rho / (m[:, None] * A1), 0.0)
    else:
        s = float((w * m2).sum() / A1 ** 2)
        grad = 2.0 * w[:, None] * rho / A1 ** 2
    return dict(s=s, S=m2 / A2 if A2 > 0.0 else np.zeros(K), rho=rho, grad=grad, A1=A1, A2=A2, w=w)


def gradient(pos, types, coeff, hkl, L, grad, tilt=None):
    """ds/dr_j[N, 3] of the particles given, with the coefficients (alpha_k, beta_k) of the whole system"""
    a = np.asarray(coeff, dtype=np.float64)[np.asarray(types, dtype=np.int64)] if len(pos) else np.zeros(0)
    q = wave_vectors(hkl, L, tilt)
    phi = np.asarray(pos, dtype=np.float64).reshape(-1, 3) @ q.T
    amp = -grad[:, 0] * np.sin(phi) + grad[:, 1] * np.cos(phi)            # [N, K]
    return a[:, None] * (amp @ q)


def compute(pos, types, coeff, hkl, L, weights=None, modulus=False, tilt=None, bias=1.0, ranks=None):
    """dict(s, S, rho, grad, A1, A2, w, dsdr, F); ranks: a list of index arrays, the split of the particles over the ranks of a
    domain-decomposed run (None: one rank) — the sums are formed per rank and added in the order given"""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    types = np.asarray(types, dtype=np.int64)
    parts = [np.arange(len(pos))] if ranks is None else ranks
    total = np.zeros(2 * len(hkl) + 2)
    for idx in parts:
        total += sums(pos[idx], types[idx], coeff, hkl, L, tilt)
    r = from_sums(total, weights, modulus)
    r["dsdr"] = gradient(pos, types, coeff, hkl, L, r["grad"], tilt)
    r["F"] = -bias * r["dsdr"]
    return r


def value(pos, types, coeff, hkl, L, weights=None, modulus=False, tilt=None):
    return from_sums(sums(pos, types, coeff, hkl, L, tilt), weights, modulus)["s"]


def lamellar_value(pos, types, coeff, hkl, L, tilt=None):
    """cv.lamellar on the same inputs: s = (1 / N) sum_k Re rho_k"""
    return sums(pos, types, coeff, hkl, L, tilt)[0:-2:2].sum() / len(pos)


def cubic_lattice(n, a=1.0):
    """n^3 simple-cubic sites in a box of edge n a centred on the origin"""
    i = np.arange(n)
    ix, iy, iz = np.meshgrid(i, i, i, indexing="ij")
    pos = (np.stack([ix, iy, iz], axis=-1).reshape(-1, 3) + 0.5) * a - 0.5 * n * a
    return pos, iz.reshape(-1), float(n * a)
