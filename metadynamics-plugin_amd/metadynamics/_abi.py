"""ctypes binding of libmtd_hip.so (include/mtd_abi.h) — the C-ABI drop-in boundary.

The library is the product: if it is missing or does not load this module raises, it never falls
back to a CPU path.  Device buffers are passed as raw addresses (``tensor.data_ptr()``).
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
PKG_ROOT = os.path.dirname(_HERE)
REPO_ROOT = os.path.dirname(PKG_ROOT)
LIB_PATH = os.environ.get("MTD_LIB_OVERRIDE") or os.path.join(PKG_ROOT, "lib", "libmtd_hip.so")  # override: diagnostic builds only
HEADER_PATH = os.path.join(REPO_ROOT, "include", "mtd_abi.h")

MTD_MAX_CV = 8
MTD_MAX_MODES = 64
MTD_MAX_TYPES = 16
MTD_METAD_MAX_CV = 6
MTD_F32, MTD_F64 = 0, 1
MODE_STANDARD, MODE_WELL_TEMPERED = 0, 1

ARRAY_NAMES = ["grid", "grid_delta", "reweighted", "weight", "sigma_grid", "sigma_grid_delta",
               "hist", "hist_delta", "hist_gauss", "hist_gauss_delta"]


class MtdError(RuntimeError):
    pass


class Box(C.Structure):
    _fields_ = [("L", C.c_double * 3), ("lo", C.c_double * 3),
                ("xy", C.c_double), ("xz", C.c_double), ("yz", C.c_double),
                ("periodic", C.c_ubyte * 3), ("_pad", C.c_ubyte * 5)]

    @classmethod
    def make(cls, L, lo=None, xy=0.0, xz=0.0, yz=0.0):
        if isinstance(L, (int, float)):
            L = [float(L)] * 3
        L = [float(x) for x in L]
        if lo is None:
            lo = [-0.5 * x for x in L]
        b = cls()
        b.L[:] = L
        b.lo[:] = [float(x) for x in lo]
        b.xy, b.xz, b.yz = float(xy), float(xz), float(yz)
        b.periodic[:] = [1, 1, 1]
        return b


class LamellarSet(C.Structure):
    _fields_ = [("n_cv", C.c_uint), ("n_types", C.c_uint), ("n_modes", C.c_uint),
                ("first", C.c_uint * (MTD_MAX_CV + 1)),
                ("hkl", (C.c_int * 3) * MTD_MAX_MODES),
                ("coeff", (C.c_double * MTD_MAX_TYPES) * MTD_MAX_CV),
                ("trig_mode", C.c_int)]

    @classmethod
    def make(cls, cvs, trig_mode=0):
        """cvs: list of (lattice_vectors [(h,k,l)...], mode coefficients per type [a_0, a_1, ...]);
        trig_mode: 0 the process default, 1 hardware sine / cosine, 2 ocml sinpi / cospi (mtd_abi.h)."""
        s = cls()
        s.trig_mode = int(trig_mode)
        if not 1 <= len(cvs) <= MTD_MAX_CV:
            raise MtdError("between 1 and %d lamellar CVs can be fused" % MTD_MAX_CV)
        n_types = len(cvs[0][1])
        k = 0
        s.first[0] = 0
        for c, (lattice, mode) in enumerate(cvs):
            if len(mode) != n_types:
                raise MtdError("cv.lamellar: Number of mode parameters has to equal the number of particle types!")
            if len(lattice) == 0:
                raise MtdError("cv.lamellar: List of supplied latice vectors is empty.")
            for hkl in lattice:
                if len(hkl) != 3:
                    raise MtdError("cv.lamellar: List of input lattice vectors not a list of triples.")
                if k >= MTD_MAX_MODES:
                    raise MtdError("too many Fourier modes (max %d)" % MTD_MAX_MODES)
                s.hkl[k][:] = [int(x) for x in hkl]
                k += 1
            s.first[c + 1] = k
            for t, a in enumerate(mode):
                s.coeff[c][t] = float(a)
        s.n_cv, s.n_types, s.n_modes = len(cvs), n_types, k
        return s


class QlLocalOptions(C.Structure):
    """mtd_ql_local_options: all-zero is the plain variable; c0, p count with switch_on, n_lo, n_hi with gate_on"""
    _fields_ = [("average", C.c_int), ("switch_on", C.c_int), ("c0", C.c_double), ("p", C.c_uint), ("gate_on", C.c_int),
                ("n_lo", C.c_double), ("n_hi", C.c_double)]

    @classmethod
    def make(cls, average=False, switch=None, gate=None):
        """switch: (c0, p) or None; gate: (n_lo, n_hi) or None"""
        o = cls()
        o.average = int(bool(average))
        if switch is not None:
            o.switch_on, o.c0, o.p = 1, float(switch[0]), int(switch[1])
        if gate is not None:
            o.gate_on, o.n_lo, o.n_hi = 1, float(gate[0]), float(gate[1])
        return o


class QlLocalBonds(C.Structure):
    """mtd_ql_local_bonds: all-zero is off; the ramp of the solid-bond count, -1 <= d_lo < d_hi <= 1"""
    _fields_ = [("on", C.c_int), ("d_lo", C.c_double), ("d_hi", C.c_double)]

    @classmethod
    def make(cls, bonds=None):
        """bonds: (d_lo, d_hi) or None"""
        o = cls()
        if bonds is not None:
            o.on, o.d_lo, o.d_hi = 1, float(bonds[0]), float(bonds[1])
        return o


class ClusterParams(C.Structure):
    """mtd_cluster_params: all-zero is off; nodes are the particles with v >= v_min, linked within r_link"""
    _fields_ = [("on", C.c_int), ("v_min", C.c_double), ("r_link", C.c_double)]

    @classmethod
    def make(cls, cluster=None):
        """cluster: (v_min, r_link) or None"""
        o = cls()
        if cluster is not None:
            o.on, o.v_min, o.r_link = 1, float(cluster[0]), float(cluster[1])
        return o


MTD_CLUSTER_NONE = 0xffffffff
MTD_ES_MAX_ENV, MTD_ES_MAX_VEC = 4, 64


class EsParams(C.Structure):
    """mtd_es_params: the template environments (packed one after the other), sigma_env, the window, lambda and the optional switch"""
    _fields_ = [("n_env", C.c_uint), ("n_vec", C.c_uint * MTD_ES_MAX_ENV), ("vec", (C.c_double * 3) * MTD_ES_MAX_VEC),
                ("sigma_env", C.c_double), ("r_on", C.c_double), ("r_cut", C.c_double), ("lam", C.c_double),
                ("switch_on", C.c_int), ("c0", C.c_double), ("p", C.c_uint)]

    @classmethod
    def make(cls, templates, sigma_env, r_on, r_cut, lam=100.0, switch=None):
        """templates: a list of environments, each a list of 3-vectors; switch: (c0, p) or None.  Nothing is checked here beyond the
        capacity of the arrays: the entry points refuse what they do not take"""
        o = cls()
        o.n_env = len(templates)
        k = 0
        for e, env in enumerate(templates):
            if e < MTD_ES_MAX_ENV:
                o.n_vec[e] = len(env)
            for t in env:
                if e < MTD_ES_MAX_ENV and k < MTD_ES_MAX_VEC:
                    o.vec[k][:] = [float(x) for x in t]
                k += 1
        o.sigma_env, o.r_on, o.r_cut, o.lam = float(sigma_env), float(r_on), float(r_cut), float(lam)
        if switch is not None:
            o.switch_on, o.c0, o.p = 1, float(switch[0]), int(switch[1])
        return o


MTD_PEL_MAX_BINS = 128


class PelParams(C.Structure):
    """mtd_pel_params: the histogram, the particle type, the optional average window and the optional switch"""
    _fields_ = [("r_max", C.c_double), ("sigma_r", C.c_double), ("n_bins", C.c_uint), ("type", C.c_uint), ("average_on", C.c_int),
                ("a_on", C.c_double), ("a_cut", C.c_double), ("switch_on", C.c_int), ("c0", C.c_double), ("p", C.c_uint)]

    @classmethod
    def make(cls, r_max, sigma_r, n_bins, type_id, average=None, switch=None):
        """average: (a_on, a_cut) or None; switch: (c0, p) or None.  Nothing is checked here: the entry points refuse what they do not take"""
        o = cls()
        o.r_max, o.sigma_r, o.n_bins, o.type = float(r_max), float(sigma_r), int(n_bins), int(type_id)
        if average is not None:
            o.average_on, o.a_on, o.a_cut = 1, float(average[0]), float(average[1])
        if switch is not None:
            o.switch_on, o.c0, o.p = 1, float(switch[0]), int(switch[1])
        return o


class PelCall(C.Structure):
    """mtd_pel_call: particles, box, list, scratch and stream of one step (RowCall with n_global in the place of n_ghost)"""
    _fields_ = [("n_particles", C.c_uint), ("n_global", C.c_uint), ("d_postype", C.c_void_p), ("dtype", C.c_int), ("box", C.POINTER(Box)),
                ("d_head_list", C.c_void_p), ("d_n_neigh", C.c_void_p), ("d_nlist", C.c_void_p), ("d_scratch", C.c_void_p),
                ("stream", C.c_void_p)]


MTD_DSF_MAX_Q = 8
MTD_DSF_MAX_SPECTRUM = 256


class DsfParams(C.Structure):
    """mtd_dsf_params: the particle type, the cut-off, the wave numbers of the peaks and their weights"""
    _fields_ = [("type", C.c_uint), ("r_cut", C.c_double), ("n_q", C.c_uint), ("q", C.c_double * MTD_DSF_MAX_Q),
                ("c", C.c_double * MTD_DSF_MAX_Q)]

    @classmethod
    def make(cls, type_id, r_cut, q, c=None, n_q=None):
        """q, c: up to MTD_DSF_MAX_Q numbers each (weights default to 1); n_q overrides the count (to hand over a refused one).
        Nothing is checked here: the entry points refuse what they do not take"""
        o = cls()
        q = [float(v) for v in q]
        c = [1.0] * len(q) if c is None else [float(v) for v in c]
        o.type, o.r_cut, o.n_q = int(type_id), float(r_cut), len(q) if n_q is None else int(n_q)
        for k in range(min(len(q), MTD_DSF_MAX_Q)):
            o.q[k], o.c[k] = q[k], c[k]
        return o


class RowCall(C.Structure):
    """mtd_row_call (mtd_dsf_call, mtd_coord_call, mtd_tet_call): particles, ghosts, box, list, scratch and stream of one step"""
    _fields_ = [("n_particles", C.c_uint), ("n_ghost", C.c_uint), ("d_postype", C.c_void_p), ("dtype", C.c_int), ("box", C.POINTER(Box)),
                ("d_head_list", C.c_void_p), ("d_n_neigh", C.c_void_p), ("d_nlist", C.c_void_p), ("d_scratch", C.c_void_p),
                ("stream", C.c_void_p)]


DsfCall = CoordCall = RowCall

MTD_COORD_MAX_M = 32


class CoordParams(C.Structure):
    """mtd_coord_params: the two particle types, the rational switching function, the cut-off and the optional switch on n_i"""
    _fields_ = [("type_a", C.c_uint), ("type_b", C.c_uint), ("r_0", C.c_double), ("d_0", C.c_double), ("n", C.c_uint), ("m", C.c_uint),
                ("r_cut", C.c_double), ("switch_on", C.c_int), ("c0", C.c_double), ("p", C.c_uint), ("less", C.c_int)]

    @classmethod
    def make(cls, type_a, type_b, r_0, r_cut, d_0=0.0, n=6, m=12, switch=None):
        """switch: None or (c0, p[, less]).  Nothing is checked here: the entry points refuse what they do not take"""
        o = cls()
        o.type_a, o.type_b, o.r_0, o.d_0, o.n, o.m, o.r_cut = int(type_a), int(type_b), float(r_0), float(d_0), int(n), int(m), float(r_cut)
        if switch is not None:
            o.switch_on, o.c0, o.p = 1, float(switch[0]), int(switch[1])
            o.less = int(bool(switch[2])) if len(switch) > 2 else 0
        return o


TetCall = RowCall

MTD_TET_W_MIN = 1e-12


class TetParams(C.Structure):
    """mtd_tet_params: the particle type, the window, cos0, the normalisation and the optional switch and gate on t_i and n_i"""
    _fields_ = [("type", C.c_uint), ("r_cut", C.c_double), ("r_on", C.c_double), ("cos0", C.c_double), ("normalise", C.c_int),
                ("switch_on", C.c_int), ("c0", C.c_double), ("p", C.c_uint), ("gate_on", C.c_int), ("n_lo", C.c_double), ("n_hi", C.c_double)]

    @classmethod
    def make(cls, type_id, r_cut, r_on, cos0=-1.0 / 3.0, normalise=True, switch=None, gate=None):
        """switch: None or (c0, p); gate: None or (n_lo, n_hi).  Nothing is checked here: the entry points refuse what they do not take"""
        o = cls()
        o.type, o.r_cut, o.r_on, o.cos0, o.normalise = int(type_id), float(r_cut), float(r_on), float(cos0), int(bool(normalise))
        if switch is not None:
            o.switch_on, o.c0, o.p = 1, float(switch[0]), int(switch[1])
        if gate is not None:
            o.gate_on, o.n_lo, o.n_hi = 1, float(gate[0]), float(gate[1])
        return o


HexCall = RowCall

MTD_HEX_MAX_K = 12
MTD_HEX_N_MIN = 1e-12


class HexParams(C.Structure):
    """mtd_hex_params: the particle type, the fold k, the axis (0, 1, 2: the layer normal), the window, the mode and the optional
    switch and gate on c_i and n_i"""
    _fields_ = [("type", C.c_uint), ("k", C.c_uint), ("axis", C.c_uint), ("r_cut", C.c_double), ("r_on", C.c_double),
                ("global_order", C.c_int), ("switch_on", C.c_int), ("c0", C.c_double), ("p", C.c_uint), ("gate_on", C.c_int),
                ("n_lo", C.c_double), ("n_hi", C.c_double)]

    @classmethod
    def make(cls, type_id, r_cut, r_on, k=6, axis=2, global_order=False, switch=None, gate=None):
        """switch: None or (c0, p); gate: None or (n_lo, n_hi).  Nothing is checked here: the entry points refuse what they do not take"""
        o = cls()
        o.type, o.k, o.axis, o.r_cut, o.r_on, o.global_order = int(type_id), int(k), int(axis), float(r_cut), float(r_on), int(bool(global_order))
        if switch is not None:
            o.switch_on, o.c0, o.p = 1, float(switch[0]), int(switch[1])
        if gate is not None:
            o.gate_on, o.n_lo, o.n_hi = 1, float(gate[0]), float(gate[1])
        return o


MTD_BRAGG_MAX_MODES = 16
MTD_TRIG_DEFAULT, MTD_TRIG_HARDWARE, MTD_TRIG_ACCURATE = 0, 1, 2


class BraggParams(C.Structure):
    """mtd_bragg_params: the lattice vectors, the amplitude of every particle type, the weights, the form and the trigonometry"""
    _fields_ = [("n_modes", C.c_uint), ("hkl", (C.c_int * 3) * MTD_BRAGG_MAX_MODES), ("n_types", C.c_uint), ("coeff", C.c_double * MTD_MAX_TYPES),
                ("weights", C.c_double * MTD_BRAGG_MAX_MODES), ("modulus", C.c_int), ("trig_mode", C.c_int)]

    @classmethod
    def make(cls, hkl, coeff, weights=None, modulus=False, trig_mode=0, n_modes=None, n_types=None):
        """hkl: up to MTD_BRAGG_MAX_MODES triples; coeff: a(t) per type; weights default to 1 / K; n_modes, n_types override the counts (to
        hand over refused ones).  Nothing is checked here: the entry points refuse what they do not take"""
        o = cls()
        weights = [1.0 / len(hkl)] * len(hkl) if weights is None else [float(w) for w in weights]
        o.n_modes = len(hkl) if n_modes is None else int(n_modes)
        o.n_types = len(coeff) if n_types is None else int(n_types)
        for k in range(min(len(hkl), MTD_BRAGG_MAX_MODES)):
            o.hkl[k][:] = [int(x) for x in hkl[k]]
            o.weights[k] = weights[k]
        for t in range(min(len(coeff), MTD_MAX_TYPES)):
            o.coeff[t] = float(coeff[t])
        o.modulus, o.trig_mode = int(bool(modulus)), int(trig_mode)
        return o


class BraggCall(C.Structure):
    """mtd_bragg_call: particles, the GLOBAL box, the particle count of all ranks, scratch and stream of one step"""
    _fields_ = [("n_particles", C.c_uint), ("d_postype", C.c_void_p), ("dtype", C.c_int), ("global_box", C.POINTER(Box)), ("n_global", C.c_uint),
                ("d_scratch", C.c_void_p), ("stream", C.c_void_p)]


MTD_PROBE_BOX, MTD_PROBE_SPHERE, MTD_PROBE_CYLINDER = 0, 1, 2


class ProbeParams(C.Structure):
    """mtd_probe_params: the shape, its FRACTIONAL centre and sizes, the smoothing and the weight of every particle type"""
    _fields_ = [("shape", C.c_int), ("axis", C.c_int), ("centre", C.c_double * 3), ("half_width", C.c_double * 3), ("radius", C.c_double),
                ("sigma_s", C.c_double), ("r_c", C.c_double), ("n_types", C.c_uint), ("coeff", C.c_double * MTD_MAX_TYPES)]

    @staticmethod
    def fractional(centre, box):
        """f with centre = lo + f_0 a_1 + f_1 a_2 + f_2 a_3 in a Box (back-substitution: the lattice matrix is triangular)"""
        x, y, z = (float(centre[d]) - box.lo[d] for d in range(3))
        f2 = z / box.L[2]
        f1 = (y - f2 * box.yz * box.L[2]) / box.L[1]
        f0 = (x - f1 * box.xy * box.L[1] - f2 * box.xz * box.L[2]) / box.L[0]
        return [f0, f1, f2]

    @classmethod
    def make(cls, shape, centre_frac, sigma_s, r_c=None, half_width=None, radius=0.0, axis=0, coeff=(1.0,), n_types=None):
        """shape: "box" | "sphere" | "cylinder" or the enum value; centre_frac: fractional coordinates (see `fractional`); r_c defaults to
        2 sigma_s; half_width: three numbers for a box, one for a cylinder (its half-length), inf for unbounded.  Nothing is checked here:
        the entry points refuse what they do not take"""
        o = cls()
        o.shape = {"box": MTD_PROBE_BOX, "sphere": MTD_PROBE_SPHERE, "cylinder": MTD_PROBE_CYLINDER}.get(shape, shape)
        o.axis = int(axis)
        o.centre[:] = [float(x) for x in centre_frac]
        if half_width is None:
            half_width = [float("inf")] * 3
        elif not hasattr(half_width, "__len__"):
            half_width = [float(half_width) if d == o.axis else float("inf") for d in range(3)]
        o.half_width[:] = [float(x) for x in half_width]
        o.radius = float(radius)
        o.sigma_s = float(sigma_s)
        o.r_c = 2.0 * float(sigma_s) if r_c is None else float(r_c)
        o.n_types = len(coeff) if n_types is None else int(n_types)
        for t in range(min(len(coeff), MTD_MAX_TYPES)):
            o.coeff[t] = float(coeff[t])
        return o


class ProbeCall(C.Structure):
    """mtd_probe_call: particles, the GLOBAL box, the particle count of all ranks, scratch and stream of one step"""
    _fields_ = [("n_particles", C.c_uint), ("d_postype", C.c_void_p), ("dtype", C.c_int), ("global_box", C.POINTER(Box)), ("n_global", C.c_uint),
                ("d_scratch", C.c_void_p), ("stream", C.c_void_p)]


_vp = C.c_void_p
_dp = C.POINTER(C.c_double)
_up = C.POINTER(C.c_uint)
_ip = C.POINTER(C.c_int)

_SIGNATURES = {
    "mtd_abi_version": (C.c_int, []),
    "mtd_status_string": (C.c_char_p, [C.c_int]),
    "mtd_device_count": (C.c_int, []),
    "mtd_lamellar_scratch_doubles": (C.c_size_t, [C.c_uint]),
    "mtd_calculate_fourier_modes": (C.c_int, [C.c_uint, _ip, C.c_uint, _vp, C.c_int, _dp, C.c_uint, _vp, _vp,
                                               C.POINTER(Box), _vp]),
    "mtd_lamellar_cv_partials": (C.c_int, [C.POINTER(LamellarSet), C.c_uint, _vp, C.c_int, C.POINTER(Box), _vp,
                                            _up, _vp]),
    "mtd_reduce_partials": (C.c_int, [_vp, C.c_uint, C.c_uint, C.c_uint, C.c_double, C.c_double, _vp, _vp]),
    "mtd_compute_sq_forces": (C.c_int, [C.c_uint, _vp, _vp, C.c_int, C.c_uint, _ip, _dp, C.c_uint, C.c_uint,
                                         C.c_double, C.POINTER(Box), _vp]),
    "mtd_lamellar_forces": (C.c_int, [C.POINTER(LamellarSet), C.c_uint, _vp, C.POINTER(_vp), C.c_int, C.c_uint,
                                       _vp, C.POINTER(Box), _vp]),
    "mtd_lamellar_set_fast_trig": (C.c_int, [C.c_int]),
    "mtd_lamellar_get_fast_trig": (C.c_int, []),
    "mtd_debug_sph_harmonics": (C.c_int, [C.c_uint, C.c_uint, _vp, _vp]),
    "mtd_rccl_last_error": (C.c_char_p, []),
    "mtd_mesh_clear_rider": (C.c_int, [_vp, C.POINTER(C.c_int)]),
    "mtd_mesh_assign_info": (C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_uint), _vp]),
    "mtd_mesh_transform_info": (C.c_int, [_vp, C.POINTER(C.c_int)]),
    "mtd_mesh_forces_update_bias": (C.c_int, [_vp, _vp, C.c_uint, C.POINTER(LamellarSet), _up, C.c_uint, _vp, _vp, C.POINTER(_vp), C.c_int, C.c_uint,
                                              C.POINTER(Box), C.c_uint, _vp]),
    "mtd_mesh_set_lamellar_rider": (C.c_int, [_vp, _vp, _vp, _vp, C.c_uint, _vp, C.POINTER(C.c_uint), _vp]),
    "mtd_ql_symmetrize_half_list": (C.c_int, [C.c_uint, _vp, _vp, _vp, _vp, _vp, _vp, C.c_size_t, C.POINTER(C.c_size_t), _vp]),
    "mtd_debug_index_decode": (C.c_int, [C.c_uint, _vp, C.c_uint, _vp, _vp, _vp]),
    "mtd_update_grid": (C.c_int, [C.c_uint, _up, C.c_uint, _vp, _vp, _dp, _dp, _dp, C.c_double, C.c_double, _vp]),
    "mtd_metad_create": (C.c_int, [C.POINTER(_vp), C.c_uint, _dp, _dp, _dp, _up, C.c_double, C.c_double,
                                    C.c_double, C.c_uint, C.c_int, C.c_int]),
    "mtd_metad_destroy": (C.c_int, [_vp]),
    "mtd_metad_set_stride": (C.c_int, [_vp, C.c_uint]),
    "mtd_metad_set_add_hills": (C.c_int, [_vp, C.c_int]),
    "mtd_metad_set_mode": (C.c_int, [_vp, C.c_int]),
    "mtd_metad_set_sigma_inv": (C.c_int, [_vp, _dp]),
    "mtd_metad_reset_histogram": (C.c_int, [_vp, _vp]),
    "mtd_metad_set_cv_source": (C.c_int, [_vp, C.c_uint, _vp, C.c_uint, C.c_uint, C.c_uint, C.c_double, C.c_double]),
    "mtd_metad_set_cv_value": (C.c_int, [_vp, C.c_uint, C.c_double]),
    "mtd_metad_bias_device": (_vp, [_vp]),
    "mtd_metad_cv_device": (_vp, [_vp]),
    "mtd_metad_update_bias": (C.c_int, [_vp, C.c_uint, _vp]),
    "mtd_metad_update_phase_a": (C.c_int, [_vp, C.c_uint, _ip, _vp]),
    "mtd_metad_update_phase_b": (C.c_int, [_vp, C.c_int, _vp]),
    "mtd_metad_delta_buffers": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_vp), _up]),
    "mtd_metad_get_state": (C.c_int, [_vp, _dp, _dp, _dp, _dp, _up, _up, _vp]),
    "mtd_metad_sigma_determinant": (C.c_double, [_vp]),
    "mtd_metad_num_elements": (C.c_uint, [_vp]),
    "mtd_metad_get_array": (C.c_int, [_vp, C.c_int, _vp, _vp]),
    "mtd_metad_set_array": (C.c_int, [_vp, C.c_int, _vp, _vp]),
    "mtd_metad_set_num_gaussians": (C.c_int, [_vp, C.c_uint, _vp]),
    "mtd_metad_device_array": (_vp, [_vp, C.c_int]),
    "mtd_fused_cv_pass": (C.c_int, [_vp, C.POINTER(LamellarSet), C.c_uint, _vp, C.c_int, C.POINTER(Box), _vp, _up, _vp]),
    "mtd_fused_force_pass": (C.c_int, [_vp, C.POINTER(LamellarSet), C.c_uint, _vp, C.POINTER(_vp), C.c_int, C.c_uint,
                                        C.POINTER(Box), C.c_uint, _vp]),
    "mtd_fused_step": (C.c_int, [_vp, C.POINTER(LamellarSet), C.c_uint, _vp, C.POINTER(_vp), C.c_int, C.c_uint, C.POINTER(Box), _vp,
                                  C.c_uint, _vp]),
    "mtd_fused_step_launches": (C.c_uint, [_vp]),
    "mtd_fused_step_set_mode": (C.c_int, [_vp, C.c_int]),
    "mtd_profile_force_begin": (C.c_int, [C.c_uint]),
    "mtd_profile_force_end": (C.c_int, [_dp, C.c_uint, _up]),
    "mtd_comm_create": (C.c_int, [C.POINTER(_vp), C.c_uint, C.c_uint, C.c_uint]),
    "mtd_comm_handle": (C.c_int, [_vp, _vp]),
    "mtd_comm_connect": (C.c_int, [_vp, _vp]),
    "mtd_comm_allreduce_small": (C.c_int, [_vp, _vp, C.c_uint, _vp]),
    "mtd_comm_status": (C.c_int, [_vp, _up, _vp]),
    "mtd_comm_share": (C.c_int, [_vp, C.c_size_t, C.POINTER(_vp), _up, _vp]),
    "mtd_comm_open": (C.c_int, [_vp, C.c_uint, _vp, C.POINTER(_vp)]),
    "mtd_comm_world": (C.c_uint, [_vp]),
    "mtd_comm_rank": (C.c_uint, [_vp]),
    "mtd_comm_destroy": (C.c_int, [_vp]),
    "mtd_metad_set_comm": (C.c_int, [_vp, _vp]),
    "mtd_rccl_unique_id": (C.c_int, [_vp]),
    "mtd_rccl_create": (C.c_int, [C.POINTER(_vp), _vp, C.c_uint, C.c_uint]),
    "mtd_comm_allreduce_large": (C.c_int, [_vp, _vp, C.c_size_t, C.c_int, _vp]),
    "mtd_rccl_world": (C.c_uint, [_vp]),
    "mtd_rccl_rank": (C.c_uint, [_vp]),
    "mtd_rccl_destroy": (C.c_int, [_vp]),
    "mtd_metad_update_bias_walkers": (C.c_int, [_vp, _vp, C.c_uint, _vp]),
    "mtd_fused_force_pass_slots": (C.c_int, [_vp, C.POINTER(LamellarSet), _up, C.c_uint, _vp, C.POINTER(_vp), C.c_int, C.c_uint,
                                              C.POINTER(Box), C.c_uint, _vp]),
    "mtd_mesh_create": (C.c_int, [C.POINTER(_vp), C.c_uint, C.c_uint, C.c_uint, _dp, C.c_uint, C.c_uint]),
    "mtd_mesh_destroy": (C.c_int, [_vp]),
    "mtd_mesh_set_bug_compat": (C.c_int, [_vp, C.c_int]),
    "mtd_mesh_set_keep_fourier": (C.c_int, [_vp, C.c_int]),
    "mtd_mesh_set_cv_event": (C.c_int, [_vp, _vp]),
    "mtd_mesh_num_cells": (C.c_uint, [_vp]),
    "mtd_mesh_set_table": (C.c_int, [_vp, _dp, _dp, C.c_uint, C.c_double, C.c_double]),
    "mtd_mesh_set_use_table": (C.c_int, [_vp, C.c_int]),
    "mtd_mesh_qmax": (C.c_int, [_vp, C.POINTER(Box), C.c_uint, _dp, _vp]),
    "mtd_mesh_virial": (C.c_int, [_vp, C.POINTER(Box), C.c_uint, C.c_double, _dp, _vp]),
    "mtd_mesh_assign": (C.c_int, [_vp, C.c_uint, _vp, C.c_int, C.POINTER(Box), _vp]),
    "mtd_mesh_exchange_buffer": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(C.c_size_t)]),
    "mtd_mesh_spectral": (C.c_int, [_vp, C.POINTER(Box), C.c_uint, C.POINTER(_vp), _up, _vp]),
    "mtd_mesh_compute_cv": (C.c_int, [_vp, C.c_uint, _vp, C.c_int, C.POINTER(Box), C.c_uint, C.POINTER(_vp), _up, _vp]),
    "mtd_mesh_forces": (C.c_int, [_vp, C.c_uint, _vp, _vp, C.c_int, C.POINTER(Box), C.c_uint, _vp, C.c_double, _vp]),
    "mtd_mesh_slab_bytes": (C.c_int, [_vp, C.c_uint, C.POINTER(C.c_size_t)]),
    "mtd_mesh_slab_attach": (C.c_int, [_vp, _vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)]),
    "mtd_mesh_slab_compute_cv": (C.c_int, [_vp, C.c_uint, _vp, C.c_int, C.POINTER(Box), C.c_uint, C.POINTER(_vp), _vp]),
    "mtd_mesh_get_array": (C.c_int, [_vp, C.c_int, _vp, _vp]),
    "mtd_ql_scratch_doubles": (C.c_size_t, [C.c_uint]),
    "mtd_ql_accumulate_local": (C.c_int, [C.c_uint, _vp, C.c_int, C.POINTER(Box), _vp, _vp, _vp, C.c_int, C.c_double, C.c_double,
                                           C.c_uint, C.c_uint, C.c_uint, _vp, C.POINTER(_vp), _up, _vp]),
    "mtd_ql_finalize": (C.c_int, [C.c_int, C.c_uint, _dp, C.c_uint, _vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), _vp]),
    "mtd_ql_finalize_update_bias": (C.c_int, [_vp, C.c_int, C.c_uint, _dp, C.c_uint, _vp, C.c_uint, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), _vp]),
    "mtd_metad_grid_touched": (C.c_int, [_vp, _vp]),
    "mtd_comm_pull_bytes": (C.c_size_t, [C.c_size_t]),
    "mtd_comm_pull_attach": (C.c_int, [_vp, C.c_size_t, C.POINTER(_vp), C.POINTER(_vp)]),
    "mtd_comm_allreduce_pull": (C.c_int, [_vp, _vp, C.c_size_t, _vp]),
    "mtd_ql_accumulate": (C.c_int, [C.c_uint, _vp, C.c_int, C.POINTER(Box), _vp, _vp, _vp, C.c_int, C.c_double, C.c_double, C.c_uint,
                                     C.c_uint, _dp, C.c_uint, _vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), _vp]),
    "mtd_ql_set_half_list_exact": (C.c_int, [C.c_int]),
    "mtd_ql_forces": (C.c_int, [C.c_uint, _vp, _vp, C.c_int, C.POINTER(Box), _vp, _vp, _vp, C.c_int, C.c_double, C.c_double, C.c_uint,
                                 C.c_uint, _dp, C.c_uint, _vp, _vp, C.c_double, _vp]),
    "mtd_ql_forces_virial": (C.c_int, [C.c_uint, _vp, _vp, C.c_int, C.POINTER(Box), _vp, _vp, _vp, C.c_int, C.c_double, C.c_double, C.c_uint,
                                        C.c_uint, _dp, C.c_uint, _vp, _vp, C.c_double, _vp, _vp, C.c_uint]),
    "mtd_ql_local_scratch_doubles": (C.c_size_t, [C.c_uint, C.c_uint]),
    "mtd_ql_local_accumulate": (C.c_int, [C.c_uint, _vp, C.c_int, C.POINTER(Box), _vp, _vp, _vp, C.c_double, C.c_double, C.c_uint, C.c_uint,
                                           _dp, C.c_uint, _vp, C.POINTER(_vp), _up, C.POINTER(_vp), C.POINTER(_vp), _vp]),
    "mtd_ql_local_forces": (C.c_int, [C.c_uint, _vp, _vp, C.c_int, C.POINTER(Box), _vp, _vp, _vp, C.c_double, C.c_double, C.c_uint, C.c_uint,
                                       _dp, C.c_uint, _vp, _vp, C.c_double, _vp]),
    "mtd_ql_local_scratch_doubles_opt": (C.c_size_t, [C.c_uint, C.c_uint, C.c_size_t, C.POINTER(QlLocalOptions)]),
    "mtd_ql_local_accumulate_opt": (C.c_int, [C.c_uint, _vp, C.c_int, C.POINTER(Box), _vp, _vp, _vp, C.c_double, C.c_double, C.c_uint, C.c_uint,
                                               _dp, C.c_uint, _vp, C.POINTER(_vp), _up, C.POINTER(_vp), C.POINTER(_vp), _vp,
                                               C.POINTER(QlLocalOptions), C.POINTER(_vp)]),
    "mtd_ql_local_forces_opt": (C.c_int, [C.c_uint, _vp, _vp, C.c_int, C.POINTER(Box), _vp, _vp, _vp, C.c_double, C.c_double, C.c_uint, C.c_uint,
                                           _dp, C.c_uint, _vp, _vp, C.c_double, _vp, C.POINTER(QlLocalOptions)]),
    "mtd_ql_local_forces_virial": (C.c_int, [C.c_uint, _vp, _vp, C.c_int, C.POINTER(Box), _vp, _vp, _vp, C.c_double, C.c_double, C.c_uint, C.c_uint,
                                              _dp, C.c_uint, _vp, _vp, C.c_double, _vp, C.POINTER(QlLocalOptions), _vp, C.c_uint]),
    "mtd_ql_local_scratch_doubles_bonds": (C.c_size_t, [C.c_uint, C.c_uint, C.c_size_t, C.POINTER(QlLocalOptions), C.POINTER(QlLocalBonds)]),
    "mtd_ql_local_accumulate_bonds": (C.c_int, [C.c_uint, _vp, C.c_int, C.POINTER(Box), _vp, _vp, _vp, C.c_double, C.c_double, C.c_uint, C.c_uint,
                                                 _dp, C.c_uint, _vp, C.POINTER(_vp), _up, C.POINTER(_vp), C.POINTER(_vp), _vp,
                                                 C.POINTER(QlLocalOptions), C.POINTER(_vp), C.POINTER(QlLocalBonds), C.POINTER(_vp)]),
    "mtd_ql_local_forces_bonds": (C.c_int, [C.c_uint, _vp, _vp, C.c_int, C.POINTER(Box), _vp, _vp, _vp, C.c_double, C.c_double, C.c_uint, C.c_uint,
                                             _dp, C.c_uint, _vp, _vp, C.c_double, _vp, C.POINTER(QlLocalOptions), _vp, C.c_uint,
                                             C.POINTER(QlLocalBonds)]),
    "mtd_cluster_scratch_bytes": (C.c_size_t, [C.c_uint]),
    "mtd_cluster_largest": (C.c_int, [C.c_uint, _vp, C.c_int, C.POINTER(Box), _vp, _vp, _vp, C.c_uint, _vp, C.POINTER(ClusterParams), _vp,
                                       C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), _vp]),
    "mtd_ql_local_accumulate_cluster": (C.c_int, [C.c_uint, _vp, C.c_int, C.POINTER(Box), _vp, _vp, _vp, C.c_double, C.c_double, C.c_uint, C.c_uint,
                                                   _dp, C.c_uint, _vp, C.POINTER(_vp), _up, C.POINTER(_vp), C.POINTER(_vp), _vp,
                                                   C.POINTER(QlLocalOptions), C.POINTER(_vp), C.POINTER(QlLocalBonds), C.POINTER(_vp),
                                                   C.POINTER(ClusterParams), _vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)]),
    "mtd_pe_scratch_doubles": (C.c_size_t, [C.c_uint]),
    "mtd_pe_accumulate": (C.c_int, [C.c_uint, _vp, C.c_int, C.POINTER(Box), _vp, _vp, _vp, C.c_double, C.c_double, C.c_uint, C.c_uint, _vp,
                                     C.POINTER(_vp), _up, _vp]),
    "mtd_pe_finalize": (C.c_int, [C.POINTER(Box), C.c_double, C.c_double, C.c_uint, _vp, C.POINTER(_vp), C.POINTER(_vp), _vp]),
    "mtd_pe_forces": (C.c_int, [C.c_uint, _vp, _vp, C.c_int, C.POINTER(Box), _vp, _vp, _vp, C.c_double, C.c_double, C.c_uint, C.c_uint, _vp, _vp,
                                 C.c_double, _vp, _vp, C.c_uint]),
    "mtd_es_scratch_doubles": (C.c_size_t, [C.c_uint]),
    "mtd_es_accumulate": (C.c_int, [C.c_uint, C.c_uint, _vp, C.c_int, C.POINTER(Box), _vp, _vp, _vp, C.c_uint, C.POINTER(EsParams), C.c_uint, _vp,
                                     C.POINTER(_vp), _up, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), _vp]),
    "mtd_es_forces": (C.c_int, [C.c_uint, C.c_uint, _vp, _vp, C.c_int, C.POINTER(Box), _vp, _vp, _vp, C.c_uint, C.POINTER(EsParams), C.c_uint, _vp,
                                 _vp, C.c_double, _vp, _vp, C.c_uint]),
    "mtd_pel_scratch_doubles": (C.c_size_t, [C.c_uint, C.c_uint]),
    "mtd_pel_accumulate": (C.c_int, [C.POINTER(PelParams), C.POINTER(PelCall), C.POINTER(_vp), _up, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)]),
    "mtd_pel_forces": (C.c_int, [C.POINTER(PelParams), C.POINTER(PelCall), _vp, _vp, C.c_double, _vp, C.c_uint]),
    "mtd_dsf_scratch_doubles": (C.c_size_t, [C.c_uint]),
    "mtd_dsf_set_store_gradient": (C.c_int, [C.c_int]),
    "mtd_dsf_accumulate": (C.c_int, [C.POINTER(DsfParams), C.POINTER(DsfCall), C.POINTER(_vp), _up]),
    "mtd_dsf_finalize": (C.c_int, [C.POINTER(DsfParams), C.POINTER(DsfCall), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)]),
    "mtd_dsf_forces": (C.c_int, [C.POINTER(DsfParams), C.POINTER(DsfCall), _vp, _vp, C.c_double, _vp, C.c_uint]),
    "mtd_dsf_spectrum": (C.c_int, [C.POINTER(DsfParams), C.POINTER(DsfCall), C.c_double, C.c_double, C.c_uint, C.POINTER(_vp), _up]),
    "mtd_dsf_spectrum_finalize": (C.c_int, [C.POINTER(DsfCall), C.c_double, C.c_double, C.c_uint, C.POINTER(_vp)]),
    "mtd_coord_scratch_doubles": (C.c_size_t, [C.c_uint]),
    "mtd_coord_set_compiled_pair": (C.c_int, [C.c_int]),
    "mtd_coord_accumulate": (C.c_int, [C.POINTER(CoordParams), C.POINTER(CoordCall), C.POINTER(_vp), _up]),
    "mtd_coord_accumulate_cluster": (C.c_int, [C.POINTER(CoordParams), C.POINTER(CoordCall), C.POINTER(ClusterParams), _vp, C.POINTER(_vp), _up,
                                               C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)]),
    "mtd_coord_finalize": (C.c_int, [C.POINTER(CoordParams), C.POINTER(CoordCall), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)]),
    "mtd_coord_forces": (C.c_int, [C.POINTER(CoordParams), C.POINTER(CoordCall), _vp, _vp, C.c_double, _vp, C.c_uint]),
    "mtd_tet_scratch_doubles": (C.c_size_t, [C.c_uint]),
    "mtd_tet_accumulate": (C.c_int, [C.POINTER(TetParams), C.POINTER(TetCall), C.POINTER(_vp), _up]),
    "mtd_tetrahedral_accumulate_cluster": (C.c_int, [C.POINTER(TetParams), C.POINTER(TetCall), C.POINTER(ClusterParams), _vp, C.POINTER(_vp),
                                                     _up, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)]),
    "mtd_tet_finalize": (C.c_int, [C.POINTER(TetParams), C.POINTER(TetCall), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)]),
    "mtd_tet_forces": (C.c_int, [C.POINTER(TetParams), C.POINTER(TetCall), _vp, _vp, C.c_double, _vp, C.c_uint]),
    "mtd_hex_scratch_doubles": (C.c_size_t, [C.c_uint]),
    "mtd_hex_accumulate": (C.c_int, [C.POINTER(HexParams), C.POINTER(HexCall), C.POINTER(_vp), _up]),
    "mtd_hex_finalize": (C.c_int, [C.POINTER(HexParams), C.POINTER(HexCall), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp),
                                   C.POINTER(_vp)]),
    "mtd_hex_forces": (C.c_int, [C.POINTER(HexParams), C.POINTER(HexCall), _vp, _vp, C.c_double, _vp, C.c_uint]),
    "mtd_bragg_scratch_doubles": (C.c_size_t, [C.c_uint]),
    "mtd_bragg_accumulate": (C.c_int, [C.POINTER(BraggParams), C.POINTER(BraggCall), C.POINTER(_vp), _up]),
    "mtd_bragg_finalize": (C.c_int, [C.POINTER(BraggParams), C.POINTER(BraggCall), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)]),
    "mtd_bragg_forces": (C.c_int, [C.POINTER(BraggParams), C.POINTER(BraggCall), _vp, _vp, C.c_double]),
    "mtd_probe_scratch_doubles": (C.c_size_t, [C.c_uint]),
    "mtd_probe_accumulate": (C.c_int, [C.POINTER(ProbeParams), C.POINTER(ProbeCall), C.POINTER(_vp), _up]),
    "mtd_probe_finalize": (C.c_int, [C.POINTER(ProbeParams), C.POINTER(ProbeCall), C.POINTER(_vp), C.POINTER(_vp)]),
    "mtd_probe_forces": (C.c_int, [C.POINTER(ProbeParams), C.POINTER(ProbeCall), _vp, _vp, C.c_double, _vp, C.c_uint]),
    "mtd_probe_local": (C.c_int, [C.POINTER(ProbeParams), C.POINTER(ProbeCall), _vp]),
    "mtd_nlist_create": (C.c_int, [C.POINTER(_vp)]),
    "mtd_nlist_destroy": (C.c_int, [_vp]),
    "mtd_nlist_build": (C.c_int, [_vp, C.c_uint, C.c_uint, _vp, C.c_int, C.POINTER(Box), C.c_double, C.c_int, C.c_int,
                                   C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(C.c_size_t), _vp]),
    "mtd_nlist_check": (C.c_int, [_vp, _vp, C.c_int, C.POINTER(Box), C.c_double, _ip, _vp]),
    "mtd_nlist_cells": (C.c_int, [_vp, _up]),
    "mtd_wte_scratch_doubles": (C.c_size_t, [C.c_uint]),
    "mtd_wte_energy_partials": (C.c_int, [C.c_uint, _vp, C.c_int, _vp, _up, _vp]),
    "mtd_wte_scale_netforce": (C.c_int, [C.c_uint, _vp, _vp, _vp, C.c_uint, C.c_int, _vp, C.c_double, C.c_int, _vp]),
    "mtd_wrapper_scale_forces": (C.c_int, [C.c_uint, _vp, _vp, _vp, C.c_uint, C.c_int, _vp, C.c_double, C.c_int, _vp]),
    "mtd_sigma_scratch_doubles": (C.c_size_t, []),
    "mtd_sigma_products": (C.c_int, [C.c_uint, C.POINTER(C.c_void_p), C.c_uint, C.c_int, C.c_double, _vp, _dp, _vp]),
    "mtd_sigma_inverse": (C.c_int, [C.c_uint, _dp, _dp]),
}

_lib = None


def load():
    """Load libmtd_hip.so; raises MtdError when the HIP library has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise MtdError("libmtd_hip.so not found at %s — build it with __graft_entry__.build() "
                           "(make -C metadynamics-plugin_amd/csrc); there is no CPU fallback." % LIB_PATH)
        # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.so (SONAME
        # libamdhip64.so.7).  A process that uses torch as well (the test / bench harness) imports it
        # FIRST: the dynamic linker then satisfies this library's DT_NEEDED with that already-loaded copy,
        # so torch tensors, streams and RCCL buffers and our kernels share one runtime; loaded the other
        # way round two runtimes would coexist.
        # (torch is never imported from here: a process without it loads the HIP runtime libmtd_hip.so links against)
        # The xGMI mailbox and the slab mesh share device buffers between the processes of a node with hipIpcGetMemHandle; on
        # hosts whose driver only supports dmabuf IPC the runtime must be told BEFORE it initialises (it reads the variable
        # once), or the export fails with "invalid argument" and every rank falls back to the RCCL all-reduce.  Set here when
        # nobody chose a value (a process that initialised HIP before importing this module has to export it itself:
        # xgmi.connect reports the value it ran with).
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            if not hasattr(lib, name):
                continue  # optional blocks are bound by their own modules
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def bind(name, restype, argtypes):
    """Bind an additional entry point (used by the mesh / steinhardt modules)."""
    fn = getattr(load(), name)
    fn.restype = restype
    fn.argtypes = argtypes
    return fn


def check(rc):
    if rc != 0:
        msg = load().mtd_status_string(int(rc))
        raise MtdError("libmtd_hip: %s (status %d)" % (msg.decode() if msg else "?", rc))


def declared_symbols():
    """Every function name include/mtd_abi.h declares (for the export test)."""
    import re
    text = open(HEADER_PATH).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mtd_[a-z0-9_]+)\s*\(", text)))


def ptr(t):
    """Device (or host) address of a torch tensor / numpy array / int / None."""
    if t is None:
        return None
    if isinstance(t, int):
        return t
    if hasattr(t, "data_ptr"):
        return t.data_ptr()
    return t.ctypes.data
