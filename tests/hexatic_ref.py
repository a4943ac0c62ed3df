"""fp64 numpy restatement of the bond-orientational order (cv.hexatic, include/mtd_abi.h "Bond-orientational order") FROM THE DEFINITION:
explicit complex sums over the entries of every row, the closed-form gradient G of one entry, and gradient and virial in the scatter
form (an entry (i, j) gives +g_ij to r_j and -g_ij to r_i, half of its virial to each end) — not the gather with the parity of B that
the GPU pass evaluates.

    entries (i, j): both of the type, j != i, j a central particle, 0 < r = |d| <= r_cut, d = minImage(r_j - r_i)
    (u, v): the two components that follow the axis cyclically (z -> (x, y), x -> (y, z), y -> (z, x))
    f(r) = 1 (r <= r_on), (1 + cos(pi (r - r_on) / (r_cut - r_on))) / 2 beyond
    z = (u + i v) / r      B = z^k      n_i = sum_j f      S_i = sum_j f B
    psi_i = S_i / n_i where n_i >= N_MIN, else 0 with zero gradient      c_i = |psi_i|^2
    local:  v_i = g(n_i) h(c_i), s = (1 / N_t) sum_i v_i      global:  Psi = (1 / N_t) sum_i psi_i, s = |Psi|^2
    G(d) = f' B d/r + f [ (k z^(k-1) / r) (e_u + i e_v) - (k B / r^2) d ]
"""
import numpy as np

from pair_entropy_ref import brute_nlist, min_image      # noqa: F401
from tetrahedral_ref import PAIRS6, g_of, h_of, row_entries, window      # noqa: F401

N_MIN = 1e-12
MAX_K = 12
AXES = {"x": 0, "y": 1, "z": 2}


def params(type_id, r_cut, r_on, k=6, axis=2, global_order=False, switch=None, gate=None):
    """axis: 0, 1, 2 or "x", "y", "z"; switch: None or (c0, p); gate: None or (n_lo, n_hi)"""
    return dict(type=int(type_id), r_cut=float(r_cut), r_on=float(r_on), k=int(k), axis=AXES.get(axis, axis), global_order=bool(global_order),
                switch=switch, gate=gate)


def compute(pos, types, L, nl, par, tilt=None, bias=1.0):
    """returns dict(s, sums, local, switched, coordination, psi, Psi, grad, virial, virial_sum, r, n_t, entries)
    sums         (4,): sum v_i, N_t, sum Re psi_i, sum Im psi_i
    local        (N,): c_i (0 for particles of another type)
    switched     (N,): v_i = g(n_i) h(c_i) (c_i in global mode)
    coordination (N,): n_i
    psi          (N,) complex: psi_i;  Psi: their mean over the centres of the type
    grad         (N, 3): ds/dr, the scatter form
    virial       (N, 6): -(bias / (2 N_t)) sum over the entries that end at the particle, as centre or as neighbour, of g_a d_b
    r            the distances of the entries that take part (the tests' condition on the inputs)
    entries      dict(i, j, d, g): the entries that take part and g_ij = d(N_t s)/dd_ij of each"""
    pos, types = np.asarray(pos, dtype=np.float64), np.asarray(types)
    N = len(nl[0])
    k, ax = par["k"], par["axis"]
    iu, iv = (ax + 1) % 3, (ax + 2) % 3
    i, j, d, r = row_entries(pos, types, nl, L, par, tilt=tilt)
    f, df = window(r, par)
    z = (d[:, iu] + 1j * d[:, iv]) / r
    B = z ** k
    n = np.bincount(i, weights=f, minlength=N)
    S = np.bincount(i, weights=f * B.real, minlength=N) + 1j * np.bincount(i, weights=f * B.imag, minlength=N)
    ok = n >= N_MIN
    ns = np.where(ok, n, 1.0)
    psi = np.where(ok, S / ns, 0.0)
    c = psi.real ** 2 + psi.imag ** 2
    of_t = types[:N] == par["type"]
    n_t = int(of_t.sum())
    Psi = psi[of_t].sum() / n_t if n_t else 0.0j
    if par["global_order"]:
        assert par["switch"] is None and par["gate"] is None
        v = c.copy()
        s = abs(Psi) ** 2
        alpha = np.where(ok, 2.0 * Psi / ns, 0.0)
        beta = np.where(ok, -2.0 * (np.conj(Psi) * psi).real / ns, 0.0)
    else:
        h, dh = h_of(c, par["switch"])
        g, dg = g_of(n, par["gate"])
        v = np.where(ok, g * h, 0.0)
        s = float(v.sum()) / n_t if n_t else 0.0
        alpha = np.where(ok, 2.0 * g * dh * psi / ns, 0.0)
        beta = np.where(ok, dg * h - 2.0 * g * dh * c / ns, 0.0)
    # G of every entry, three complex components
    e_uv = np.zeros((3,), dtype=np.complex128)
    e_uv[iu], e_uv[iv] = 1.0, 1.0j
    G = (df * B / r)[:, None] * d + f[:, None] * ((k * z ** (k - 1) / r)[:, None] * e_uv[None, :] - (k * B / (r * r))[:, None] * d)
    ge = (np.conj(alpha[i])[:, None] * G).real + (beta[i] * df / r)[:, None] * d
    grad = np.zeros((N, 3))
    virial = np.zeros((N, 6))
    if n_t:
        for a in range(3):
            grad[:, a] = (np.bincount(j, weights=ge[:, a], minlength=N) - np.bincount(i, weights=ge[:, a], minlength=N)) / n_t
        for c6, (a, b) in enumerate(PAIRS6):
            w = ge[:, a] * d[:, b]
            virial[:, c6] = -0.5 * bias / n_t * (np.bincount(i, weights=w, minlength=N) + np.bincount(j, weights=w, minlength=N))
    sums = np.array([v[of_t].sum(), float(n_t), psi[of_t].real.sum(), psi[of_t].imag.sum()])
    return dict(s=float(s), sums=sums, n_t=n_t, local=c, switched=v, coordination=n, psi=psi, Psi=complex(Psi), grad=grad, virial=virial,
                virial_sum=virial.sum(axis=0), r=r, entries=dict(i=i, j=j, d=d, g=ge))


def value(pos, types, L, nl, par, tilt=None):
    return compute(pos, types, L, nl, par, tilt=tilt)["s"]


def box_nlist(pos, L, r_cut):
    """util.build_nlist for an orthorhombic box with three different lengths (a layer's box is not cubic): full list, rows ascending"""
    from scipy.spatial import cKDTree
    L = np.broadcast_to(np.asarray(L, dtype=np.float64), (3,))
    p = np.mod(np.asarray(pos, dtype=np.float64) + L / 2, L)
    p = np.where(p >= L, p - L, p)
    pairs = cKDTree(p, boxsize=L).query_pairs(r_cut, output_type="ndarray")
    N = len(p)
    i = np.concatenate([pairs[:, 0], pairs[:, 1]])
    j = np.concatenate([pairs[:, 1], pairs[:, 0]])
    order = np.lexsort((j, i))
    i, j = i[order], j[order]
    n_neigh = np.bincount(i, minlength=N).astype(np.uint32)
    head = np.zeros(N, dtype=np.uint32)
    head[1:] = np.cumsum(n_neigh)[:-1]
    return head, n_neigh, j.astype(np.uint32)


def triangular_layer(nx, ny, phi0=0.0, lz=4.0):
    """nx x ny particles (ny even) of a triangular monolayer with nearest-neighbour distance 1 in the plane z = 0, periodic in the box
    (nx, ny sqrt(3) / 2, lz).  phi0 rotates an ISOLATED copy about z (the periodic box does not rotate with it: use a box that no
    bond crosses).  Returns positions centred on 0 and the box lengths"""
    assert ny % 2 == 0
    ix, iy = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    x = (ix + 0.5 * (iy % 2)).reshape(-1).astype(np.float64)
    y = (iy * (np.sqrt(3.0) / 2.0)).reshape(-1)
    L = np.array([float(nx), ny * np.sqrt(3.0) / 2.0, float(lz)])
    pos = np.stack([x - L[0] / 2 + 0.25, y - L[1] / 2 + 0.25 * np.sqrt(3.0), np.zeros_like(x)], axis=1)
    if phi0:
        cs, sn = np.cos(phi0), np.sin(phi0)
        pos = pos @ np.array([[cs, -sn, 0.0], [sn, cs, 0.0], [0.0, 0.0, 1.0]]).T
    return pos, L
