"""Collective variables — the reference's ``hoomd.metadynamics.cv`` API (metadynamics/cv.py) over the MI355X host classes.

Class names, constructor arguments, ``set_grid`` / ``set_params`` and the error behaviour follow the reference
(file:line citations refer to /root/reference/metadynamics/cv.py).  There is no CPU class to choose
(cv.py:260-265 picks LamellarOrderParameter vs ...GPU by ``exec_conf.isCUDAEnabled()``): the GPU class is the only one.
"""
from . import _metadynamics
from . import context


class _collective_variable(object):
    """Base class (cv.py:11-170): a collective variable is a force with grid / umbrella parameters."""

    def __init__(self, sigma, name=None):
        self.name = name
        self.force_name = "cv" if name is None else str(name)
        self.enabled = True
        self.log = True
        self.sigma = sigma
        self.cv_min = 0.0
        self.cv_max = 0.0
        self.num_points = 0
        self.grid_set = False
        self.ftm_min = 0.0
        self.ftm_max = 0.0
        self.ftm_parameters_set = False
        self.umbrella = False
        self.reweight = False
        self.cpp_force = None
        context.current.forces.append(self)

    def set_grid(self, cv_min, cv_max, num_points):                 # cv.py:70-86
        self.cv_min = cv_min
        self.cv_max = cv_max
        self.num_points = int(num_points)
        self.grid_set = True

    def enable_histograms(self, ftm_min, ftm_max):                  # cv.py:88-103
        self.ftm_min = ftm_min
        self.ftm_max = ftm_max
        self.ftm_parameters_set = True

    def set_params(self, sigma=None, kappa=None, cv0=None, umbrella=None, width_flat=None, scale=None, reweight=None):
        """cv.py:105-170"""
        if sigma is not None:
            self.sigma = sigma
        if umbrella is not None:
            modes = {"no_umbrella": (self.cpp_force.umbrella.no_umbrella, False),
                     "linear": (self.cpp_force.umbrella.linear, True),
                     "harmonic": (self.cpp_force.umbrella.harmonic, True),
                     "wall": (self.cpp_force.umbrella.wall, True),
                     "gaussian": (self.cpp_force.umbrella.gaussian, True)}
            if umbrella not in modes:
                raise RuntimeError("Error setting parameters of collective variable.")   # cv.py:150-152
            cpp_umbrella, flag = modes[umbrella]
            self.reweight = flag
            self.umbrella = flag
            self.cpp_force.setUmbrella(cpp_umbrella)
        if kappa is not None:
            self.cpp_force.setKappa(kappa)
        if width_flat is not None:
            self.cpp_force.setWidthFlat(width_flat)
        if cv0 is not None:
            self.cpp_force.setMinimum(cv0)
        if scale is not None:
            self.cpp_force.setScale(scale)
        if reweight is not None:
            self.reweight = reweight

    def update_coeffs(self):
        pass


def _mode_vector(mode, what):
    if type(mode) != type(dict()):
        raise RuntimeError("Error creating collective variable.")    # cv.py:236-238
    pdata = context.current.system_definition.getParticleData()
    out = []
    for i in range(pdata.getNTypes()):
        t = pdata.getNameByType(i)
        if t not in mode.keys():
            raise RuntimeError("Error creating collective variable.")   # cv.py:245-247: missing mode amplitude
        out.append(float(mode[t]))
    return out


class lamellar(_collective_variable):
    """Lamellar order parameter (cv.py:173-272): s = (1/N) sum_i sum_j a(type_j) cos(q_i . r_j)."""

    def __init__(self, mode, lattice_vectors, name=None, sigma=1.0):
        if name is not None:
            name = "_" + name
            suffix = name
        else:
            suffix = ""
        _collective_variable.__init__(self, sigma, name)
        if len(lattice_vectors) == 0:
            raise RuntimeError("Error creating collective variable.")   # cv.py:232-234
        cpp_mode = _mode_vector(mode, "cv.lamellar")
        cpp_lattice_vectors = _metadynamics.std_vector_int3()
        for l in lattice_vectors:
            if len(l) != 3:
                raise RuntimeError("Error creating collective variable.")   # cv.py:252-254
            cpp_lattice_vectors.append(_metadynamics.make_int3(int(l[0]), int(l[1]), int(l[2])))
        self.cpp_force = _metadynamics.LamellarOrderParameterGPU(context.current.system_definition, cpp_mode,
                                                                 cpp_lattice_vectors, suffix)

    def set_trig_mode(self, mode):
        """this build: the trigonometry of this variable's kernels — "hardware" (v_sin_f32 / v_cos_f32, like the reference's
        fast::sin / fast::cos), "accurate" (sinpi / cospi; also the mode for unwrapped coordinates far outside the box) or
        "default" (the process-wide default).  Variables evaluated in one fused launch run accurately if any of them asks to."""
        codes = {"default": 0, "hardware": 1, "accurate": 2}
        if mode not in codes:
            raise RuntimeError("Error setting parameters of collective variable.")
        self.cpp_force.setTrigMode(codes[mode])


class bragg(_collective_variable):
    """this build (no reference counterpart; include/mtd_abi.h "Bragg intensity"): the intensity of chosen Bragg peaks,
    CV = sum_k weights[k] |rho_k|^2 / A1^2 with rho_k = sum_j a(type_j) exp(i q_k . r_j) over all particles and A1 = sum_j |a(type_j)|,
    or with ``modulus=True`` CV = sum_k weights[k] |rho_k| / A1.  ``mode`` and ``lattice_vectors`` are those of ``cv.lamellar`` (at most
    16 vectors), ``weights`` default to 1 / K each, and both forms then lie between 0 and 1: 1 for a perfect density wave, O(1 / N) for
    random positions (O(1 / sqrt N) with ``modulus``).

    ``cv.lamellar`` takes the real part of rho_k and so depends on where the density wave sits in the box: a bias on it must both order
    the system and hold the pattern at the origin, and lamellae or a crystal that form at any other phase get no credit.  This variable
    does not change when all particles are shifted together; it is oriented, unlike ``cv.debye_structure_factor``, and costs O(N K)
    without a neighbour list.  It is what order-disorder studies of block copolymers and the interface-pinning method bias.

    The bias force is the exact gradient (no factor 2 of ``cv.lamellar``'s quirk) and sums to zero over the particles.  The variable
    depends on fractional coordinates only, so the bias force has NO VIRIAL and none is written: a constant-pressure run needs no
    correction.  With ``modulus=True`` the gradient has a cusp where a peak vanishes; the force stays bounded there.
    Works in domain-decomposed runs with any split of the particles."""

    def __init__(self, mode, lattice_vectors, weights=None, modulus=False, name=None, sigma=1.0):
        if name is not None:
            name = "_" + name
            suffix = name
        else:
            suffix = ""
        _collective_variable.__init__(self, sigma, name)
        try:
            if len(lattice_vectors) == 0 or len(lattice_vectors) > 16:
                raise ValueError
            cpp_mode = _mode_vector(mode, "cv.bragg")
            cpp_lattice_vectors = _metadynamics.std_vector_int3()
            for l in lattice_vectors:
                if len(l) != 3:
                    raise ValueError
                cpp_lattice_vectors.append(_metadynamics.make_int3(int(l[0]), int(l[1]), int(l[2])))
            weights = self._weights(weights, len(lattice_vectors))
            self.cpp_force = _metadynamics.BraggIntensity(context.current.system_definition, cpp_mode, cpp_lattice_vectors, weights,
                                                          bool(modulus), suffix)
        except (TypeError, ValueError, AttributeError, RuntimeError):
            context.current.forces.remove(self)                      # refused: the run must not find a half-made variable
            raise RuntimeError("Error creating collective variable.")
        self.lattice_vectors = [tuple(int(x) for x in l) for l in lattice_vectors]
        self.weights = weights
        self.modulus = bool(modulus)

    @staticmethod
    def _weights(weights, n):
        """None: 1 / n each; else n finite numbers"""
        if weights is None:
            return [1.0 / n] * n
        weights = [float(weights)] if not hasattr(weights, "__len__") else [float(w) for w in weights]
        inf = float("inf")
        if len(weights) != n or not all(-inf < w < inf for w in weights):
            raise ValueError
        return weights

    def set_weights(self, weights):
        """one weight per lattice vector (None: 1 / K each); the value of the current time step is formed anew"""
        try:
            weights = self._weights(weights, len(self.lattice_vectors))
        except (TypeError, ValueError):
            raise RuntimeError("Error setting parameters of collective variable.")
        self.cpp_force.setWeights(weights)
        self.weights = weights

    def set_trig_mode(self, mode):
        """the trigonometry of this variable's kernels: "hardware", "accurate" or "default", as ``cv.lamellar.set_trig_mode``"""
        codes = {"default": 0, "hardware": 1, "accurate": 2}
        if mode not in codes:
            raise RuntimeError("Error setting parameters of collective variable.")
        self.cpp_force.setTrigMode(codes[mode])

    def get_structure_factors(self):
        """S_k = |rho_k|^2 / sum_j a_j^2 of every lattice vector at the current time step: N for a perfect density wave, about 1 for
        random positions"""
        return self.cpp_force.getStructureFactors(context.current.system.getCurrentTimeStep())

    def get_amplitudes(self):
        """(Re rho_k, Im rho_k) of every lattice vector at the current time step, an array of shape (K, 2)"""
        return self.cpp_force.getAmplitudes(context.current.system.getCurrentTimeStep())


class probe_volume(_collective_variable):
    """this build (no reference counterpart; include/mtd_abi.h "Probe volume"): the coarse-grained number of particles in a region fixed
    in space, CV = sum_i a(type_i) h(min_image(r_i - centre)), the variable of the INDUS method (Patel, Varilly, Chandler, Garde,
    J. Stat. Phys. 145, 265 (2011)).  Every other variable here is a property of the whole box; this one says where: it is biased to empty
    a cavity next to a surface, to fill or drain a pore, to drive cavitation at a chosen place, to hold a slab at a given filling.

    ``shape`` is "box" (``half_widths``: three numbers along the lab axes, ``float("inf")`` for an unbounded one: a slab, a channel),
    "sphere" (``radius``) or "cylinder" (``axis`` "x" | "y" | "z", ``radius``, ``half_length``, by default unbounded).  h is the sharp
    indicator smoothed with a truncated, shifted Gaussian of width ``sigma_s`` and cut-off ``r_c`` (default 2 sigma_s, the paper's
    choice); the box uses the paper's product form, sphere and cylinder are smoothed RADIALLY, which is not the paper's three-dimensional
    convolution (the two agree for sigma_s << radius).  ``weights`` maps type names to a(t); the default is 1 for every type, the usual
    use 1 for one type and 0 for the rest.  Arguments that do not belong to the shape raise.

    The region with its shell must fit the minimum-image cell of the box (orthorhombic: half-width + r_c <= L / 2 on every bounded axis;
    see the header for tilted boxes); this is checked at every step.  ``centre`` is taken in the box of the moment it is given and
    follows the box affinely afterwards; the sizes stay lengths.

    The bias force is the exact gradient, -bias a_i grad h, zero outside region and shell.  The region is an external object: THE BIAS
    FORCES DO NOT SUM TO ZERO.  Virial (``get_virial``, while the pressure flag is set): -bias a_i (d_a h d_b + d_b h d_a) / 2 per
    particle, the derivative for positions, box and centre strained together.  Works in domain-decomposed runs with any split of the
    particles; ghosts are not counted."""

    _cv = "cv.probe_volume"
    _SHAPES = {"box": 0, "sphere": 1, "cylinder": 2}
    _AXES = {"x": 0, "y": 1, "z": 2, 0: 0, 1: 1, 2: 2}

    def __init__(self, shape, centre, sigma_s, r_c=None, half_widths=None, radius=None, axis=None, half_length=None, weights=None,
                 name=None, sigma=1.0):
        if name is not None:
            name = "_" + name
            suffix = name
        else:
            suffix = ""
        _collective_variable.__init__(self, sigma, name)
        try:
            region = self._region(shape, centre, sigma_s, r_c, half_widths, radius, axis, half_length)
            cpp_weights = self._weights(weights)
            self.cpp_force = _metadynamics.ProbeVolume(context.current.system_definition, *region, cpp_weights, suffix)
        except (TypeError, ValueError, AttributeError, KeyError, RuntimeError):
            context.current.forces.remove(self)                      # refused: the run must not find a half-made variable
            raise RuntimeError("Error creating collective variable.")
        self.weights = cpp_weights

    @classmethod
    def _region(cls, shape, centre, sigma_s, r_c, half_widths, radius, axis, half_length):
        """the arguments of ProbeVolume / setRegion: (shape, centre, half_widths[3], radius, axis, sigma_s, r_c); ValueError for arguments
        that are missing or do not belong to the shape"""
        inf = float("inf")
        code = cls._SHAPES[shape]
        centre = [float(x) for x in centre]
        if len(centre) != 3:
            raise ValueError
        sigma_s = float(sigma_s)
        r_c = 2.0 * sigma_s if r_c is None else float(r_c)
        if shape == "box":
            if half_widths is None or radius is not None or axis is not None or half_length is not None:
                raise ValueError
            w = [float(x) for x in half_widths]
            if len(w) != 3:
                raise ValueError
            return code, centre, w, 0.0, 0, sigma_s, r_c
        if half_widths is not None or radius is None:
            raise ValueError
        if shape == "sphere":
            if axis is not None or half_length is not None:
                raise ValueError
            return code, centre, [inf] * 3, float(radius), 0, sigma_s, r_c
        if axis is None:
            raise ValueError
        ax = cls._AXES[axis]
        w = [inf] * 3
        w[ax] = inf if half_length is None else float(half_length)
        return code, centre, w, float(radius), ax, sigma_s, r_c

    @staticmethod
    def _weights(weights):
        """None: 1 for every type; else a mapping that names every particle type (nothing is assumed for a type left out: ValueError)"""
        pdata = context.current.system_definition.getParticleData()
        names = [pdata.getNameByType(i) for i in range(pdata.getNTypes())]
        if weights is None:
            return [1.0] * len(names)
        if set(weights.keys()) != set(names):
            raise ValueError
        return [float(weights[t]) for t in names]

    def set_region(self, shape, centre, sigma_s, r_c=None, half_widths=None, radius=None, axis=None, half_length=None):
        """another region, between runs (a probe volume is commonly moved or grown in stages); the arguments of the constructor.  A
        region that is refused leaves the variable as it was"""
        try:
            region = self._region(shape, centre, sigma_s, r_c, half_widths, radius, axis, half_length)
            self.cpp_force.setRegion(*region)
        except (TypeError, ValueError, KeyError, RuntimeError):
            raise RuntimeError("Error setting parameters of collective variable.")

    def set_weights(self, weights):
        """a(t) for every type name (None: 1 for all)"""
        try:
            cpp_weights = self._weights(weights)
            self.cpp_force.setWeights(cpp_weights)
        except (TypeError, ValueError, AttributeError, RuntimeError):
            raise RuntimeError("Error setting parameters of collective variable.")
        self.weights = cpp_weights

    def get_count(self):
        """N_v = sum_i a(type_i) [particle i inside the sharp region] at the current time step (a diagnostic: it is not biased)"""
        return self.cpp_force.getCount(context.current.system.getCurrentTimeStep())

    def get_local(self):
        """h_i of every local particle at the current positions, without the weight of its type: 1 inside, 0 outside, between in the shell"""
        return self.cpp_force.getLocal(context.current.system.getCurrentTimeStep())

    def get_virial(self, per_particle=False):
        """the virial of the bias force the last step wrote, with the return convention of the neighbour-row variables: the six sums
        xx, xy, xz, yy, yz, zz as float64, or with ``per_particle=True`` the (6, N) array.  The sums are -bias times the symmetrised
        derivative of the variable under a strain of positions, box and centre.  Only while the pressure flag is set; else this raises."""
        return _neighbour_variable.get_virial(self, per_particle)


class aspect_ratio(_collective_variable):
    """cv.py:275-305"""

    def __init__(self, dir1, dir2, name="", sigma=1.0):
        _collective_variable.__init__(self, sigma, name)
        self.cpp_force = _metadynamics.AspectRatio(context.current.system_definition, int(dir1), int(dir2))


class density(_collective_variable):
    """cv.py:308-338 (group = all particles)"""

    def __init__(self, group=None, sigma=1.0):
        name = "all" if group is None else str(group)
        _collective_variable.__init__(self, sigma, name)
        self.cpp_force = _metadynamics.Density(context.current.system_definition, name)


class potential_energy(_collective_variable):
    """Well-tempered ensemble: the potential energy as collective variable (cv.py:469-497)."""

    def __init__(self, sigma=1.0):
        name = "cv_potential_energy"
        _collective_variable.__init__(self, sigma, name)
        self.enabled = False                                          # cv.py:486-487: not a regular ForceCompute
        self.cpp_force = _metadynamics.WellTemperedEnsemble(context.current.system_definition, name)


class mesh(_collective_variable):
    """Particle-mesh order parameter (cv.py:350-466)."""

    def __init__(self, mode, nx, ny=None, nz=None, name=None, sigma=1.0, zero_modes=None):
        if name is not None:
            name = "_" + name
        if ny is None:
            ny = nx
        if nz is None:
            nz = nx
        _collective_variable.__init__(self, sigma, name)
        cpp_mode = _mode_vector(mode, "cv.mesh")
        cpp_zero_modes = _metadynamics.std_vector_int3()
        if zero_modes is not None:
            for l in zero_modes:
                if len(l) != 3:
                    raise RuntimeError("Error creating collective variable.")   # cv.py:403-405
                cpp_zero_modes.append(_metadynamics.make_int3(int(l[0]), int(l[1]), int(l[2])))
        self.cpp_force = _metadynamics.OrderParameterMeshGPU(context.current.system_definition, int(nx), int(ny), int(nz),
                                                             cpp_mode, cpp_zero_modes)

    def set_decomposition(self, kind):
        """this build, domain-decomposed runs: "replicated" (default: every rank keeps the whole mesh, the ranks sum their
        assignments) or "slab" (the mesh itself is decomposed over the ranks; ny and nz multiples of the number of ranks)"""
        if kind not in ("replicated", "slab"):
            raise RuntimeError("Error setting parameters of collective variable.")
        self.cpp_force.setSlabDecomposition(kind == "slab")

    def set_params(self, use_table=None, **args):                  # cv.py:423-436
        if use_table is not None:
            self.cpp_force.setUseTable(use_table)
        _collective_variable.set_params(self, **args)

    def set_kernel(self, func, kmin, kmax, width, coeff=dict()):   # cv.py:438-466
        Ktable, dKtable = [], []
        dk = (kmax - kmin) / float(width - 1)
        for i in range(0, width):
            k = kmin + dk * i
            (K, dK) = func(k, kmin, kmax, **coeff)
            Ktable.append(K)
            dKtable.append(dK)
        self.cpp_force.setTable(Ktable, dKtable, kmin, kmax)


class _neighbour_variable(_collective_variable):
    """What the variables over the rows of a neighbour list share (steinhardt, steinhardt_local, pair_entropy, environment_similarity):
    the frame of their constructors, ``get_rcut`` and ``get_virial``.  A subclass sets ``self.type``, ``self.nlist`` and ``self.r_cut``
    (what the list must reach) and names itself in ``_cv`` for the error texts."""

    _cv = None

    def _begin(self, sigma, name):
        """registers the variable; returns the suffix of its log quantities"""
        _collective_variable.__init__(self, sigma, name)
        return "" if name is None else "_" + name

    def _full_list(self):
        # cv.py:584-585: the reference forces full storage when HOOMD runs on the GPU — this build always does
        self.nlist.cpp_nlist.setStorageMode(_metadynamics.NeighborList.storageMode.full)

    def _attach(self, type_id):
        if getattr(self.nlist, "device", False):
            self.nlist._attach(type_id)               # a device-built list only needs the pairs of this CV's type (get_rcut)

    def get_rcut(self):
        """the cut-off this CV asks of the neighbour list, by type pair — only (type, type) interacts, up to ``r_cut`` (pair_entropy:
        r_max + 4 sigma_r).  (cv.py:603-617; the reference body refers to an undefined ``nl``; this returns the plain dict it was
        building.)"""
        names = context.current.type_names
        return {(a, b): (self.r_cut if a == b == self.type else -1.0) for i, a in enumerate(names) for b in names[i:]}

    def get_virial(self, per_particle=False):
        """the virial of the bias force the last step wrote (include/mtd_abi.h): the six sums xx, xy, xz, yy, yz, zz as float64, or with
        ``per_particle=True`` the (6, N) array, half of every pair at each of its ends.  What the sums are the derivative of is said
        under "Virial" in the variable's own docstring.  In a domain-decomposed run every rank holds the rows of its local particles.
        It is formed only while the pressure flag of the particle data is set (a constant-pressure run); without the flag this raises."""
        pdata = context.current.system_definition.getParticleData()
        if not pdata.getPressureFlag():
            raise RuntimeError("%s: the virial is computed only while the pressure flag is set" % self._cv)
        import numpy as np
        n = pdata.getN()
        v = np.asarray(self.cpp_force.getVirial(), dtype=np.float64)[:, :n]
        return v.copy() if per_particle else v.sum(axis=1)


class steinhardt(_neighbour_variable):
    """Steinhardt Ql (cv.py:540-617): CV = sum_l Ql_ref[l] * Q_l over particles of one type within r_cut.

    Virial (``get_virial``; mtd_ql_forces_virial): it is the virial of the force that is applied: the full-list force keeps only the
    central terms of the gradient (as the reference's), so the sums are -1/2 * bias * ds/d(strain), not -bias * ds/d(strain)."""

    _cv = "cv.steinhardt"

    def __init__(self, r_cut, r_on, lmax, Ql_ref, nlist, type, name=None, sigma=1.0):
        suffix = self._begin(sigma, name)
        self.type = type
        self.nlist = nlist
        self.r_cut = r_cut
        self._full_list()
        type_list = context.current.type_names
        if type not in type_list:
            raise RuntimeError("Error creating collective variable.")     # cv.py:591-593
        self.cpp_force = _metadynamics.SteinhardtQl(context.current.system_definition, float(r_cut), float(r_on), int(lmax),
                                                    nlist.cpp_nlist, type_list.index(type), [float(q) for q in Ql_ref], suffix)
        self._attach(type_list.index(type))

class _local_options(type):
    """``cv.steinhardt_local(..., average=False, switch=None, gate=None, bonds=None, cluster=None)``: the options are keyword arguments of the CALL.  They
    are taken off here and applied to the finished object, so that ``__init__`` keeps the argument list of the variable without options,
    which tests/test_ql_local_abi.py pins.  The price: ``inspect.signature(cv.steinhardt_local)`` and ``help()`` do not show the
    options, and subclasses inherit this metaclass.  Once that test may change, move the keywords into ``__init__`` (ending with a
    call of ``set_options``) and delete this class."""

    def __call__(cls, *args, average=False, switch=None, gate=None, bonds=None, cluster=None, **kwargs):
        obj = super().__call__(*args, **kwargs)
        try:
            obj.set_options(average=average, switch=switch, gate=gate, bonds=bonds, cluster=cluster)
        except RuntimeError:
            context.current.forces.remove(obj)                       # refused: the run must not find a half-made variable
            raise
        return obj


def _with_cluster(set_options):
    """``set_options(..., cluster=None)``: the fifth option, taken off in front of the four that tests/test_ql_local_bonds_ref.py pins as
    the parameter list of ``set_options`` (``inspect.signature`` follows ``__wrapped__`` to the function below and shows those four) and
    applied behind them.  Once that test may change, make ``cluster`` a fifth parameter of ``set_options`` and delete this decorator."""
    import functools

    @functools.wraps(set_options)
    def with_cluster(self, *args, cluster=None, **kwargs):
        try:
            cl = None if cluster is None else (float(cluster["v_min"]), float(cluster["r_link"]))
            if cl is not None and (set(cluster.keys()) != {"v_min", "r_link"} or not abs(cl[0]) < float("inf") or not 0.0 < cl[1] < float("inf")):
                raise ValueError
            self.cpp_force.clearCluster()
            set_options(self, *args, **kwargs)
            if cl is not None:
                self.cpp_force.setCluster(*cl)         # refuses the average and an r_link beyond the reach of a device-built list
        except (TypeError, KeyError, ValueError, AttributeError, RuntimeError):
            raise RuntimeError("Error creating collective variable.")
    return with_cluster


class steinhardt_local(_neighbour_variable, metaclass=_local_options):
    """this build (no reference counterpart): the LOCAL Steinhardt order parameter.  The harmonics are summed over one particle's own
    neighbours, turned into the rotational invariant per particle and averaged:
    CV = (1 / N) sum_i sum_l Ql_ref[l] * q_l^2(i),  q_l^2(i) = 4 pi / (2l + 1) sum_m |sum_j f(r_ij) Y_lm(r_ij)|^2 / (sum_j f(r_ij))^2
    over particles of one type within r_cut (smoothing and conventions of cv.steinhardt; not square-rooted).  Needs a full list.

    Options (keyword arguments of the call, include/mtd_abi.h "Local Steinhardt bond order"):
    ``average=True``: the Lechner-Dellago neighbour average, qbar_lm(i) = [q_lm(i) + sum_j f_ij q_lm(j)] / (1 + n_i), before the invariant;
    ``switch=dict(c0=..., p=...)``: h(c) = x^p / (1 + x^p), x = max(c, 0) / c0 per particle — CV * N is then the smooth number of solid-like
    particles; ``gate=dict(n_lo=..., n_hi=...)``: a smoothstep in the coordination n_i that takes under-coordinated particles out.
    CV = (1 / N) sum_i g(n_i) h(c_i).
    ``bonds=dict(d_lo=..., d_hi=...)``: the solid-bond count of ten Wolde, Ruiz-Montero and Frenkel.  d_ij is the normalised scalar product
    of the q vectors of i and j (weights Ql_ref[l] 4 pi / (2l + 1), all >= 0), a bond counts with the smoothstep sigma of d_ij from d_lo to
    d_hi (-1 <= d_lo < d_hi <= 1), b_i = sum_j f(r_ij) sigma(d_ij), and switch and gate act on it: CV = (1 / N) sum_i g(n_i) h(b_i).
    With ``Ql_ref = e_6``, ``bonds=dict(d_lo=0.5, d_hi=0.7)`` and ``switch=dict(c0=6.5, p=12)``, CV * N is the smooth number of solid
    particles of the literature.  Not together with ``average``.
    ``cluster=dict(v_min=..., r_link=...)``: the LARGEST CLUSTER of solid particles, what seeding and umbrella studies of nucleation bias
    (ten Wolde, Ruiz-Montero and Frenkel; PLUMED's DFSCLUSTERING followed by CLUSTER_NATOMS or CLUSTER_PROPERTIES ... SUM).  Nodes are the
    particles of the type with v_i >= v_min, two nodes are linked when one lists the other within r_link (minimum image), the clusters are
    the connected components, the largest is the one with most members (a tie goes to the one that holds the smallest particle index),
    and CV = (1 / N) sum_{i in the largest cluster} v_i.  With the bond count and the switch above CV * N is the smooth size of the largest
    nucleus.  Membership is piecewise constant, so the force is the gradient of the v_i of the members alone (PLUMED's treatment): the
    variable JUMPS when clusters merge or split, by the size of the smaller one.  Single-domain runs only: a cluster would be cut at a domain
    boundary.  ``get_switched()`` stays unmasked — it is the solid-ness the clusters are built from; ``get_cluster_mask()``,
    ``get_cluster_labels()`` and ``get_largest_cluster()`` give the rest.  r_link must lie within the reach of a device-built list.  Not
    together with ``average``.

    Virial: ``get_virial`` (mtd_ql_local_forces_virial)."""

    _cv = "cv.steinhardt_local"

    def __init__(self, r_cut, r_on, lmax, Ql_ref, nlist, type, name=None, sigma=1.0):
        suffix = self._begin(sigma, name)
        self.type = type
        self.nlist = nlist
        self.r_cut = r_cut
        self._full_list()
        type_list = context.current.type_names
        if type not in type_list:
            raise RuntimeError("Error creating collective variable.")
        self.cpp_force = _metadynamics.SteinhardtLocal(context.current.system_definition, float(r_cut), float(r_on), int(lmax),
                                                       nlist.cpp_nlist, type_list.index(type), [float(q) for q in Ql_ref], suffix)
        self._attach(type_list.index(type))

    def get_local(self):
        """c_i = sum_l Ql_ref[l] q_l^2(i) of every particle at the current time step (0 for particles of another type)"""
        return self.cpp_force.getLocalValues(context.current.system.getCurrentTimeStep())

    def get_coordination(self):
        """n_i = sum_j f(r_ij): the smoothed number of neighbours of every particle at the current time step"""
        return self.cpp_force.getCoordination(context.current.system.getCurrentTimeStep())

    def get_switched(self):
        """v_i = g(n_i) h(c_i) of every particle at the current time step: what the CV averages (c_i itself without options, g(n_i) h(b_i)
        with bonds)"""
        return self.cpp_force.getSwitchedValues(context.current.system.getCurrentTimeStep())

    def get_bonds(self):
        """b_i = sum_j f(r_ij) sigma(d_ij): the smooth number of solid bonds of every particle at the current time step (needs ``bonds``)"""
        return self.cpp_force.getBondCounts(context.current.system.getCurrentTimeStep())

    def get_cluster_labels(self):
        """uint32 per particle: the smallest particle index of its cluster, 0xffffffff for a particle that is not solid (needs ``cluster``)"""
        return self.cpp_force.getClusterLabels(context.current.system.getCurrentTimeStep())

    def get_cluster_mask(self):
        """w_i: 1.0 for the members of the largest cluster, 0.0 for everybody else (needs ``cluster``)"""
        return self.cpp_force.getClusterMask(context.current.system.getCurrentTimeStep())

    def get_largest_cluster(self):
        """(root, members, n_clusters, n_nodes): the smallest particle index of the largest cluster and its member count, the number of
        clusters and of solid particles; root is 0xffffffff and members 0 when nothing is solid (needs ``cluster``)"""
        return self.cpp_force.getLargestCluster(context.current.system.getCurrentTimeStep())

    @_with_cluster
    def set_options(self, average=False, switch=None, gate=None, bonds=None):
        """set all options (the defaults switch them off), ``cluster=dict(v_min=..., r_link=...)`` among them as a keyword; takes effect
        with the next step"""
        try:
            sw = None if switch is None else (float(switch["c0"]), int(switch["p"]))
            gt = None if gate is None else (float(gate["n_lo"]), float(gate["n_hi"]))
            if sw is not None and (set(switch.keys()) != {"c0", "p"} or int(switch["p"]) != switch["p"] or not sw[0] > 0.0 or sw[1] < 1):
                raise ValueError
            if gt is not None and (set(gate.keys()) != {"n_lo", "n_hi"} or not 0.0 <= gt[0] < gt[1]):
                raise ValueError
            bd = None if bonds is None else (float(bonds["d_lo"]), float(bonds["d_hi"]))
            if bd is not None and (set(bonds.keys()) != {"d_lo", "d_hi"} or not -1.0 <= bd[0] < bd[1] <= 1.0 or average):
                raise ValueError
            self.cpp_force.clearBonds()
            if sw is None:
                self.cpp_force.clearSwitch()
            else:
                self.cpp_force.setSwitch(*sw)
            if gt is None:
                self.cpp_force.clearGate()
            else:
                self.cpp_force.setGate(*gt)
            self.cpp_force.setAverage(bool(average))
            if bd is not None:
                self.cpp_force.setBonds(*bd)
        except (TypeError, KeyError, ValueError, AttributeError, RuntimeError):
            raise RuntimeError("Error creating collective variable.")


class pair_entropy(_neighbour_variable):
    """this build (no reference counterpart; include/mtd_abi.h "Pair entropy"): the two-body excess entropy of the particles of one type
    from a Gaussian-smoothed radial distribution function (Piaggi, Valsson and Parrinello, PRL 119, 015701; PLUMED's PAIRENTROPY),
    CV = -2 pi rho int_0^r_max [g ln g - g + 1] r^2 dr in units of k_B, on ``n_bins`` midpoints with Gaussians of width ``sigma_r``.
    It needs no knowledge of the target structure and is normally biased together with ``cv.potential_energy`` on a 2-d grid.
    Needs a full list that reaches ``r_max + 4 * sigma_r`` (``get_rcut``); works in domain-decomposed runs; n_bins <= 256.

    Virial (``get_virial``; mtd_pe_forces): half of every pair at each of its ends, and the explicit volume term spread evenly over the
    particles of the type.  The sums are -bias * dS/d(strain)."""

    _cv = "cv.pair_entropy"

    def __init__(self, r_max, sigma_r, n_bins, nlist, type, name=None, sigma=1.0):
        suffix = self._begin(sigma, name)
        try:
            type_list = context.current.type_names
            r_max, sigma_r = float(r_max), float(sigma_r)
            if type not in type_list or int(n_bins) != n_bins or not 1 <= int(n_bins) <= 256 or not 0.0 < r_max < float("inf") \
                    or not 0.0 < sigma_r < float("inf") or float(nlist.r_cut) < r_max + 4.0 * sigma_r:
                raise ValueError
            self.type = type
            self.nlist = nlist
            self.r_max, self.sigma_r, self.n_bins = r_max, sigma_r, int(n_bins)
            self.r_cut = r_max + 4.0 * sigma_r
            self._full_list()
            self.cpp_force = _metadynamics.PairEntropy(context.current.system_definition, r_max, sigma_r, int(n_bins), nlist.cpp_nlist,
                                                       type_list.index(type), suffix)
        except (TypeError, ValueError, AttributeError, RuntimeError):
            context.current.forces.remove(self)                      # refused: the run must not find a half-made variable
            raise RuntimeError("Error creating collective variable.")
        self._attach(type_list.index(type))

    def get_gr(self):
        """(r_b, g_b): the bin midpoints and the smoothed radial distribution function of the current time step"""
        import numpy as np
        r_b = (np.arange(self.n_bins) + 0.5) * (self.r_max / self.n_bins)
        return r_b, np.asarray(self.cpp_force.getGr(context.current.system.getCurrentTimeStep()))


class pair_entropy_local(_neighbour_variable):
    """this build (no reference counterpart; include/mtd_abi.h "Local pair entropy"): the local-entropy fingerprint of Piaggi and Parrinello
    (J. Chem. Phys. 147, 114112; PLUMED's PAIRENTROPIES).  Every particle of ``type`` gets the pair entropy s_i of its OWN smoothed
    g_i(r), s_i = -2 pi rho int_0^r_max [g_i ln g_i - g_i + 1] r^2 dr (<= 0, strongly negative in a crystal) on ``n_bins`` midpoints with
    Gaussians of width ``sigma_r``.  ``average=dict(r_on=..., r_cut=...)`` replaces it by its average over the particle and its first
    shell, sbar_i = (s_i + sum_j f_a(r_ij) s_j) / (1 + sum_j f_a(r_ij)) with the cosine window f_a; ``switch=dict(c0=..., p=...)``
    counts it, v_i = x^p / (1 + x^p), x = max(-sbar_i, 0) / c0.  CV = (1 / N) sum_i v_i: with both options CV * N is the smooth number of
    solid-like particles, with no reference value, template or orientation to name.
    Needs a full list that reaches ``r_max + 4 * sigma_r`` (``get_rcut``); single-domain runs only; n_bins <= 128; the average window
    must end inside ``r_max + 4 * sigma_r``.

    Virial (``get_virial``; mtd_pel_forces): half of every pair at each of its ends, and the explicit volume term of s_k on the diagonal
    of particle k.  The sums are -bias * dCV/d(strain)."""

    _cv = "cv.pair_entropy_local"

    def __init__(self, r_max, sigma_r, n_bins, nlist, type, average=None, switch=None, name=None, sigma=1.0):
        suffix = self._begin(sigma, name)
        try:
            type_list = context.current.type_names
            r_max, sigma_r = float(r_max), float(sigma_r)
            if type not in type_list or int(n_bins) != n_bins or not 1 <= int(n_bins) <= 128 or not 0.0 < r_max < float("inf") \
                    or not 0.0 < sigma_r < float("inf") or float(nlist.r_cut) < r_max + 4.0 * sigma_r:
                raise ValueError
            self.type = type
            self.nlist = nlist
            self.r_max, self.sigma_r, self.n_bins = r_max, sigma_r, int(n_bins)
            self.r_cut = r_max + 4.0 * sigma_r
            options = (self._average(average), self._switch(switch))
            self._full_list()
            self.cpp_force = _metadynamics.PairEntropyLocal(context.current.system_definition, r_max, sigma_r, int(n_bins), nlist.cpp_nlist,
                                                            type_list.index(type), suffix)
            self._apply(*options)
        except (TypeError, ValueError, KeyError, AttributeError, RuntimeError):
            context.current.forces.remove(self)                      # refused: the run must not find a half-made variable
            raise RuntimeError("Error creating collective variable.")
        self._attach(type_list.index(type))

    def _average(self, average):
        if average is None:
            return None
        av = (float(average["r_on"]), float(average["r_cut"]))
        if set(average.keys()) != {"r_on", "r_cut"} or not 0.0 <= av[0] < av[1] <= self.r_cut:
            raise ValueError
        return av

    @staticmethod
    def _switch(switch):
        if switch is None:
            return None
        sw = (float(switch["c0"]), int(switch["p"]))
        if set(switch.keys()) != {"c0", "p"} or int(switch["p"]) != switch["p"] or not 0.0 < sw[0] < float("inf") or sw[1] < 1:
            raise ValueError
        return sw

    def _apply(self, av, sw):
        if av is None:
            self.cpp_force.clearAverage()
        else:
            self.cpp_force.setAverage(*av)
        if sw is None:
            self.cpp_force.clearSwitch()
        else:
            self.cpp_force.setSwitch(*sw)

    def set_options(self, average=None, switch=None):
        """replaces BOTH options (``None`` switches one off); takes effect with the next step.  A refused argument leaves the options as
        they were"""
        try:
            options = (self._average(average), self._switch(switch))
            self._apply(*options)
        except (TypeError, KeyError, ValueError, AttributeError, RuntimeError):
            raise RuntimeError("Error creating collective variable.")

    def get_local(self):
        """s_i of every particle at the current time step (0 for particles of another type)"""
        return self.cpp_force.getLocalValues(context.current.system.getCurrentTimeStep())

    def get_averaged(self):
        """sbar_i of every particle at the current time step (s_i itself without an average)"""
        return self.cpp_force.getAveragedValues(context.current.system.getCurrentTimeStep())

    def get_switched(self):
        """v_i of every particle at the current time step: what the CV averages (sbar_i itself without a switch)"""
        return self.cpp_force.getSwitchedValues(context.current.system.getCurrentTimeStep())


class debye_structure_factor(_neighbour_variable):
    """this build (no reference counterpart; include/mtd_abi.h "Debye structure factor"): the intensity of diffraction peaks from the
    Debye scattering function of the particles of one type (Niu, Piaggi, Invernizzi and Parrinello, PNAS 115, 5348 (2018)),
    I(Q) = 1 + (1 / N) sum_{i != j} w(r_ij) sin(Q r_ij) / (Q r_ij) over the pairs within ``r_cut`` with the window
    w(r) = sin(pi r / r_cut) / (pi r / r_cut).  ``q`` is one wave number or a sequence of up to 8, read off an experimental or computed
    diffraction pattern (``get_spectrum`` gives the pattern of the current configuration); CV = sum_p weights[p] * I(q[p]), weights 1.0
    each by default, and two peaks with weights of opposite sign select one polymorph against another.  It needs no template, no
    reference value and no orientation, and is invariant under rotation and translation.  The reach of the list is the resolution of
    the variable: the contrast between crystal and liquid grows with ``r_cut``.
    Needs a full list that reaches ``r_cut`` (``get_rcut``); works in domain-decomposed runs.

    The window is the published one: it vanishes at ``r_cut`` but its slope does not, so the bias force is discontinuous there, by
    sinc(Q r_cut) / r_cut per pair and peak, divided by N.

    Virial (``get_virial``; mtd_dsf_forces): half of every pair at each of its ends, no explicit volume term (the normalisation is the
    particle number, not a density).  The sums are -bias * dCV/d(strain)."""

    _cv = "cv.debye_structure_factor"

    def __init__(self, q, r_cut, nlist, type, weights=None, name=None, sigma=1.0):
        suffix = self._begin(sigma, name)
        try:
            type_list = context.current.type_names
            q = [float(q)] if not hasattr(q, "__len__") else [float(v) for v in q]
            weights = [1.0] * len(q) if weights is None else \
                ([float(weights)] if not hasattr(weights, "__len__") else [float(v) for v in weights])
            r_cut = float(r_cut)
            inf = float("inf")
            if type not in type_list or not 1 <= len(q) <= 8 or len(weights) != len(q) or not all(0.0 < v < inf for v in q) \
                    or not all(-inf < v < inf for v in weights) or not 0.0 < r_cut < inf or float(nlist.r_cut) < r_cut:
                raise ValueError
            self.type = type
            self.nlist = nlist
            self.q, self.weights = q, weights
            self.r_cut = r_cut
            self._full_list()
            self.cpp_force = _metadynamics.DebyeStructureFactor(context.current.system_definition, q, weights, r_cut, nlist.cpp_nlist,
                                                                type_list.index(type), suffix)
        except (TypeError, ValueError, AttributeError, RuntimeError):
            context.current.forces.remove(self)                      # refused: the run must not find a half-made variable
            raise RuntimeError("Error creating collective variable.")
        self._attach(type_list.index(type))

    def get_intensities(self):
        """I(q[p]) of every peak at the current time step"""
        return self.cpp_force.getIntensities(context.current.system.getCurrentTimeStep())

    def get_local(self):
        """s_i of every particle at the current time step, sum_p weights[p] * (1 + sum_j w sin(q r) / (q r)) over its own row (0 for
        particles of another type); the CV is their mean over the particles of the type"""
        return self.cpp_force.getLocalValues(context.current.system.getCurrentTimeStep())

    def get_spectrum(self, q_min, q_max, n_q):
        """(Q_m, I(Q_m)) on ``n_q`` (1 .. 256) equally spaced wave numbers from ``q_min`` > 0 to ``q_max`` at the current time step: a
        diagnostic to find the peak positions of a configuration; it is not biased"""
        import numpy as np
        q_min, q_max = float(q_min), float(q_max)
        if int(n_q) != n_q or not 1 <= int(n_q) <= 256 or not 0.0 < q_min <= q_max < float("inf"):
            raise RuntimeError("cv.debye_structure_factor: a spectrum needs 0 < q_min <= q_max and 1 <= n_q <= 256")
        n_q = int(n_q)
        dq = (q_max - q_min) / (n_q - 1) if n_q > 1 else 0.0
        return q_min + np.arange(n_q) * dq, np.asarray(self.cpp_force.getSpectrum(context.current.system.getCurrentTimeStep(), q_min, q_max, n_q))


class _largest_cluster(object):
    """``set_cluster`` and the three read-backs of the variables that restrict their sum to the largest cluster of particles with
    v_i >= v_min (cv.coordination, cv.tetrahedral; include/mtd_abi.h "Clusters").  cv.steinhardt_local has the option as a keyword of
    its own."""

    def set_cluster(self, cluster):
        """``dict(v_min=..., r_link=...)`` (exactly these keys; v_min finite, 0 < r_link < inf and within the reach of a device-built list)
        or ``None`` (off); takes effect with the next step.  A refused call leaves the option as it was"""
        try:
            if cluster is None:
                self.cpp_force.clearCluster()
                return
            cl = (float(cluster["v_min"]), float(cluster["r_link"]))
            if set(cluster.keys()) != {"v_min", "r_link"} or not abs(cl[0]) < float("inf") or not 0.0 < cl[1] < float("inf"):
                raise ValueError
            self.cpp_force.setCluster(*cl)                # everything is checked before anything is changed
        except (TypeError, KeyError, ValueError, AttributeError, RuntimeError):
            raise RuntimeError("Error creating collective variable.")

    def get_cluster_labels(self):
        """uint32 per particle: the smallest particle index of its cluster, 0xffffffff for a particle that is not solid (needs ``cluster``)"""
        return self.cpp_force.getClusterLabels(context.current.system.getCurrentTimeStep())

    def get_cluster_mask(self):
        """w_i: 1.0 for the members of the largest cluster, 0.0 for everybody else (needs ``cluster``)"""
        return self.cpp_force.getClusterMask(context.current.system.getCurrentTimeStep())

    def get_largest_cluster(self):
        """(root, members, n_clusters, n_nodes): the smallest particle index of the largest cluster and its member count, the number of
        clusters and of solid particles; root is 0xffffffff and members 0 when nothing is solid (needs ``cluster``)"""
        return self.cpp_force.getLargestCluster(context.current.system.getCurrentTimeStep())


class coordination(_neighbour_variable, _largest_cluster):
    """this build (no reference counterpart; include/mtd_abi.h "Coordination number"): the coordination number of the particles of
    ``type`` (A) by those of ``partner`` (B; ``None``: A itself) through the rational switching function of PLUMED's COORDINATION,
    s(r) = (1 - x^n) / (1 - x^m) with x = max(r - d_0, 0) / r_0, stretched so that it is 1 up to ``d_0`` and 0 at ``r_cut``
    (``None``: the reach of the list): n_i = sum_{j of type B} s(r_ij), CV = (1 / N_A) sum_i g(n_i) with g(c) = c or, with
    ``switch=dict(c0=..., p=...[, less=True])``, h(c) = y^p / (1 + y^p), y = c / c0 (1 - h with ``less``) — CV * N_A is then the smooth
    number of A particles with at least (at most) c0 B neighbours.  1 <= n < m <= 32.  The function has no singularity at x = 1: it is
    evaluated as a quotient of geometric sums.
    Needs a full list that reaches ``r_cut`` (``get_rcut``); with two types a device-built list builds all pairs.  The plain variable
    works in domain-decomposed runs, a switch does not (g' of a ghost neighbour would have to be exchanged).

    The stretched function vanishes at ``r_cut`` but its slope does not, so the bias force is discontinuous there, by
    |s'(r_cut)| / (1 - s(r_cut)) per pair, divided by N_A.

    ``set_cluster(dict(v_min=..., r_link=...))``: the LARGEST CLUSTER of "liquid-like" particles, the variable of ten Wolde and Frenkel
    for vapour-liquid nucleation and of nucleation from solution (with ``less`` in the switch: of cavitation).  Needs a switch.  Nodes are
    the particles of ``type`` with v_i >= v_min, two nodes are linked when one lists the other within r_link, and
    CV = (1 / N_A) sum_{i in the largest cluster} v_i, N_A still all particles of the type: CV * N_A is the smooth size of the largest
    cluster and does not charge for the small embryos of a large box.  Membership is piecewise constant, so the force is the gradient of
    the v_i of the members alone: the variable JUMPS when clusters merge or split.  Single-domain runs only.  ``get_switched()`` stays
    unmasked — it is what the clusters are built from; ``get_cluster_mask()``, ``get_cluster_labels()`` and ``get_largest_cluster()``
    give the rest.  With two types the nodes are the ``type`` particles only and the list must hold their pairs up to r_link (a
    device-built list with two attached types builds all pairs).  ``set_switch(None)`` is refused while the option is on.

    Virial (``get_virial``; mtd_coord_forces): half of every pair at each of its ends, no explicit volume term (the normalisation is
    the particle number, not a density).  The sums are -bias * dCV/d(strain)."""

    _cv = "cv.coordination"

    def __init__(self, r_0, nlist, type, partner=None, d_0=0.0, n=6, m=12, r_cut=None, switch=None, name=None, sigma=1.0):
        suffix = self._begin(sigma, name)
        try:
            type_list = context.current.type_names
            partner = type if partner is None else partner
            r_0, d_0 = float(r_0), float(d_0)
            r_cut = float(nlist.r_cut) if r_cut is None else float(r_cut)
            inf = float("inf")
            if type not in type_list or partner not in type_list or int(n) != n or int(m) != m or not 1 <= int(n) < int(m) <= 32 \
                    or not 0.0 < r_0 < inf or not 0.0 <= d_0 < r_cut < inf or float(nlist.r_cut) < r_cut:
                raise ValueError
            sw = self._switch(switch)
            self.type, self.partner = type, partner
            self.nlist = nlist
            self.r_0, self.d_0, self.n, self.m, self.r_cut = r_0, d_0, int(n), int(m), r_cut
            self._full_list()
            self.cpp_force = _metadynamics.CoordinationNumber(context.current.system_definition, r_0, d_0, int(n), int(m), r_cut,
                                                              nlist.cpp_nlist, type_list.index(type), type_list.index(partner), suffix)
            if sw is not None:
                self.cpp_force.setSwitch(*sw)
        except (TypeError, ValueError, KeyError, AttributeError, RuntimeError):
            context.current.forces.remove(self)                      # refused: the run must not find a half-made variable
            raise RuntimeError("Error creating collective variable.")
        self._attach(type_list.index(type))
        self._attach(type_list.index(partner))                       # (two types: a device-built list then builds all pairs)

    @staticmethod
    def _switch(switch):
        """the checks of cv.environment_similarity._switch, with the optional ``less``"""
        if switch is None:
            return None
        sw = (float(switch["c0"]), int(switch["p"]), bool(switch.get("less", False)))
        if not {"c0", "p"} <= set(switch.keys()) <= {"c0", "p", "less"} or int(switch["p"]) != switch["p"] \
                or not 0.0 < sw[0] < float("inf") or sw[1] < 1:
            raise ValueError
        return sw

    def get_rcut(self):
        """the cut-off this CV asks of the neighbour list, by type pair: ``r_cut`` for the pair {type, partner}, -1 for every other"""
        names = context.current.type_names
        pair = {self.type, self.partner}
        return {(a, b): (self.r_cut if {a, b} == pair else -1.0) for i, a in enumerate(names) for b in names[i:]}

    def get_local(self):
        """n_i of every particle at the current time step (0 for particles that are not of ``type``)"""
        return self.cpp_force.getLocalValues(context.current.system.getCurrentTimeStep())

    def get_switched(self):
        """v_i = g(n_i) of every particle at the current time step: what the CV averages (n_i itself without a switch)"""
        return self.cpp_force.getSwitchedValues(context.current.system.getCurrentTimeStep())

    def set_switch(self, switch):
        """``dict(c0=..., p=...[, less=True])`` or ``None`` (no switch); takes effect with the next step"""
        try:
            sw = self._switch(switch)
            if sw is None:
                self.cpp_force.clearSwitch()
            else:
                self.cpp_force.setSwitch(*sw)
        except (TypeError, KeyError, ValueError, AttributeError, RuntimeError):
            raise RuntimeError("Error creating collective variable.")


class tetrahedral(_neighbour_variable, _largest_cluster):
    """this build (no reference counterpart; include/mtd_abi.h "Tetrahedral order"): the three-body bond-angle order of the particles of
    ``type``, the variable of ice, silicon, germanium, mW water and clathrates.  With f the cosine window between ``r_on`` and ``r_cut``
    and u_ij the unit vector from i to its neighbour j,
    A_i = sum_{j<k} f_ij f_ik (u_ij.u_ik - cos0)^2,  W_i = sum_{j<k} f_ij f_ik,  t_i = 1 - A_i / (W_i (1/3 + cos0^2)).
    With ``cos0 = -1/3`` t_i is the tetrahedral order parameter of Chau and Hardin and of Errington and Debenedetti as a weighted mean over
    ALL pairs of neighbours inside the window (the nearest-four form of the literature is not differentiable): 1 on a diamond lattice,
    3/11 on fcc, 0 for uniformly random directions.  CV = (1 / N_type) sum_i g(n_i) h(t_i); ``switch=dict(c0=..., p=...)``:
    h(t) = x^p / (1 + x^p), x = max(t, 0) / c0 — CV * N_type is then the smooth number of tetrahedral particles;
    ``gate=dict(n_lo=..., n_hi=...)`` (1 <= n_lo < n_hi): a smoothstep in the coordination n_i = sum_j f_ij.  ``normalise=False``: CV is
    the mean of A_i itself, the three-body penalty of Stillinger and Weber; switch and gate are refused then.  Rotation invariant, unlike
    ``cv.environment_similarity("diamond")``.

    Needs a full list that reaches ``r_cut``; single-domain runs only (the force on a particle reads a table row of its neighbours,
    which a ghost does not have).  A particle with no or one neighbour has t_i = 0.

    Known property: without a gate a particle whose pair weight W_i is tiny but not zero (a second neighbour just entering the window)
    has a bounded t_i and a gradient of order 1 / f, inherent to a weighted mean.  The gate with n_lo >= 1 removes it; dilute systems
    should use the gate.

    ``set_cluster(dict(v_min=..., r_link=...))``: the LARGEST CLUSTER of tetrahedral particles, the ice, silicon or mW-water nucleus.
    Needs ``normalise``.  Nodes are the particles of the type with v_i >= v_min, two nodes are linked when one lists the other within
    r_link, and CV = (1 / N_type) sum_{i in the largest cluster} v_i, N_type still all particles of the type.  Membership is piecewise
    constant, so the force is the gradient of the v_i of the members alone: the variable JUMPS when clusters merge or split.
    Single-domain runs only.  ``get_switched()`` stays unmasked — it is what the clusters are built from; ``get_cluster_mask()``,
    ``get_cluster_labels()`` and ``get_largest_cluster()`` give the rest.

    Virial (``get_virial``; mtd_tet_forces): half of every entry at each of its ends, no explicit volume term.  The pair term is not
    parallel to the pair vector, so one particle's six components are not those of a symmetric matrix; their sum over the particles is,
    and it is -bias * dCV/d(strain)."""

    _cv = "cv.tetrahedral"

    def __init__(self, r_cut, r_on, nlist, type, cos0=-1.0 / 3.0, normalise=True, switch=None, gate=None, name=None, sigma=1.0):
        suffix = self._begin(sigma, name)
        try:
            type_list = context.current.type_names
            r_cut, r_on, cos0 = float(r_cut), float(r_on), float(cos0)
            if type not in type_list or not 0.0 <= r_on < r_cut < float("inf") or not -1.0 <= cos0 <= 1.0 or float(nlist.r_cut) < r_cut:
                raise ValueError
            normalise = bool(normalise)
            sw, gt = self._options(switch, gate, normalise)
            self.type = type
            self.nlist = nlist
            self.r_cut, self.r_on, self.cos0, self.normalise = r_cut, r_on, cos0, normalise
            self._full_list()
            self.cpp_force = _metadynamics.TetrahedralOrder(context.current.system_definition, r_cut, r_on, cos0, normalise, nlist.cpp_nlist,
                                                            type_list.index(type), suffix)
            self._apply(sw, gt)
        except (TypeError, ValueError, KeyError, AttributeError, RuntimeError):
            context.current.forces.remove(self)                      # refused: the run must not find a half-made variable
            raise RuntimeError("Error creating collective variable.")
        self._attach(type_list.index(type))

    @staticmethod
    def _options(switch, gate, normalise):
        """the checks of cv.steinhardt_local.set_options, with n_lo >= 1; both options need the normalised variable"""
        sw = None if switch is None else (float(switch["c0"]), int(switch["p"]))
        gt = None if gate is None else (float(gate["n_lo"]), float(gate["n_hi"]))
        if sw is not None and (set(switch.keys()) != {"c0", "p"} or int(switch["p"]) != switch["p"] or not 0.0 < sw[0] < float("inf")
                               or sw[1] < 1):
            raise ValueError
        if gt is not None and (set(gate.keys()) != {"n_lo", "n_hi"} or not 1.0 <= gt[0] < gt[1] < float("inf")):
            raise ValueError
        if not normalise and (sw is not None or gt is not None):
            raise ValueError
        return sw, gt

    def _apply(self, sw, gt):
        if sw is None:
            self.cpp_force.clearSwitch()
        else:
            self.cpp_force.setSwitch(*sw)
        if gt is None:
            self.cpp_force.clearGate()
        else:
            self.cpp_force.setGate(*gt)

    def get_local(self):
        """t_i of every particle at the current time step (A_i with ``normalise=False``; 0 for particles of another type)"""
        return self.cpp_force.getLocalValues(context.current.system.getCurrentTimeStep())

    def get_switched(self):
        """v_i = g(n_i) h(t_i) of every particle at the current time step: what the CV averages"""
        return self.cpp_force.getSwitchedValues(context.current.system.getCurrentTimeStep())

    def get_coordination(self):
        """n_i = sum_j f(r_ij): the smoothed number of neighbours of every particle at the current time step"""
        return self.cpp_force.getCoordination(context.current.system.getCurrentTimeStep())

    def set_options(self, switch=None, gate=None):
        """replaces switch and gate (the defaults switch them off); takes effect with the next step.  A refused call leaves both as they
        were"""
        try:
            sw, gt = self._options(switch, gate, self.normalise)     # everything is checked before anything is changed
            self._apply(sw, gt)
        except (TypeError, KeyError, ValueError, AttributeError, RuntimeError):
            raise RuntimeError("Error creating collective variable.")


class hexatic(_neighbour_variable):
    """this build (no reference counterpart; include/mtd_abi.h "Bond-orientational order"): the k-fold bond-orientational order psi_k of
    the particles of ``type`` about the lab axis ``axis`` ("x", "y" or "z"), the order WITHIN a layer: 2-d melting and freezing (liquid,
    hexatic, solid), monolayers at interfaces, confined films, the in-layer order of smectic-B and lamellar phases.  With f the cosine
    window between ``r_on`` and ``r_cut``, d_ij the vector from i to its neighbour j and (u, v) its two components that follow the axis
    cyclically (z: (x, y); x: (y, z); y: (z, x)),
    z_ij = (u_ij + i v_ij) / r_ij,  psi_i = sum_j f_ij z_ij^k / sum_j f_ij,  c_i = |psi_i|^2.
    z^k = sin^k(theta) e^{i k phi} is the SECTORAL harmonic: for a bond in the plane it is the textbook e^{i k phi}, a bond out of the
    plane is de-weighted by sin^k(theta), and a bond along the axis is an ordinary point (the unweighted form has a 1 / rho singularity
    there).  This is the definition: |psi_i| < 1 on a rippled but perfect layer is intended.
    CV = (1 / N_type) sum_i g(n_i) h(c_i); ``switch=dict(c0=..., p=...)``: h(c) = x^p / (1 + x^p), x = max(c, 0) / c0 — CV * N_type is
    then the smooth number of ordered particles; ``gate=dict(n_lo=..., n_hi=...)`` (0 <= n_lo < n_hi): a smoothstep in the coordination
    n_i = sum_j f_ij.  ``global_order=True``: CV = |Psi|^2, Psi = (1 / N_type) sum_i psi_i — the phase coherence over the box that tells
    a hexatic or a solid from a polycrystal; switch and gate are refused then.  k = 6 on a perfect triangular monolayer: 1, whatever its
    in-plane orientation; k = 4 on perfect fcc about a cube axis: 1/36.

    The variable SELECTS THE LAYER NORMAL: unlike ``cv.steinhardt_local`` it is not rotation invariant, and the bias exerts a torque
    that turns the layers' normal towards ``axis``.

    Needs a full list that reaches ``r_cut``; single-domain runs only (the force on a particle reads a table row of its neighbours,
    which a ghost does not have).  A particle without neighbours has psi_i = 0.

    Known property: without a gate a particle whose shell is nearly empty (its coordination n_i tiny but not zero) has a bounded psi_i
    and a jump-free but steep gradient of order 1 / f, inherent to a weighted mean.  The gate removes it; dilute systems should use the
    gate.

    Virial (``get_virial``; mtd_hex_forces): half of every entry at each of its ends, no explicit volume term.  The pair term is not
    parallel to the pair vector and the variable is not rotation invariant, so neither one particle's six components nor their sum are
    those of a symmetric matrix: the stored (a, b), a <= b, are -bias * dCV/d(strain) under x_a -> x_a + eps x_b."""

    _cv = "cv.hexatic"
    _axes = {"x": 0, "y": 1, "z": 2}
    _max_k = 12                                                      # MTD_HEX_MAX_K

    def __init__(self, r_cut, r_on, nlist, type, k=6, axis="z", global_order=False, switch=None, gate=None, name=None, sigma=1.0):
        suffix = self._begin(sigma, name)
        try:
            type_list = context.current.type_names
            r_cut, r_on = float(r_cut), float(r_on)
            if type not in type_list or not 0.0 <= r_on < r_cut < float("inf") or float(nlist.r_cut) < r_cut:
                raise ValueError
            if int(k) != k or not 1 <= int(k) <= self._max_k or axis not in self._axes:
                raise ValueError
            global_order = bool(global_order)
            sw, gt = self._options(switch, gate, global_order)
            self.type = type
            self.nlist = nlist
            self.r_cut, self.r_on, self.k, self.axis, self.global_order = r_cut, r_on, int(k), axis, global_order
            self._full_list()
            self.cpp_force = _metadynamics.HexaticOrder(context.current.system_definition, int(k), self._axes[axis], r_cut, r_on, global_order,
                                                        nlist.cpp_nlist, type_list.index(type), suffix)
            self._apply(sw, gt)
        except (TypeError, ValueError, KeyError, AttributeError, RuntimeError):
            context.current.forces.remove(self)                      # refused: the run must not find a half-made variable
            raise RuntimeError("Error creating collective variable.")
        self._attach(type_list.index(type))

    @staticmethod
    def _options(switch, gate, global_order):
        """the checks of cv.steinhardt_local.set_options, with n_lo >= 0; neither option with ``global_order``"""
        sw = None if switch is None else (float(switch["c0"]), int(switch["p"]))
        gt = None if gate is None else (float(gate["n_lo"]), float(gate["n_hi"]))
        if sw is not None and (set(switch.keys()) != {"c0", "p"} or int(switch["p"]) != switch["p"] or not 0.0 < sw[0] < float("inf")
                               or sw[1] < 1):
            raise ValueError
        if gt is not None and (set(gate.keys()) != {"n_lo", "n_hi"} or not 0.0 <= gt[0] < gt[1] < float("inf")):
            raise ValueError
        if global_order and (sw is not None or gt is not None):
            raise ValueError
        return sw, gt

    def _apply(self, sw, gt):
        if sw is None:
            self.cpp_force.clearSwitch()
        else:
            self.cpp_force.setSwitch(*sw)
        if gt is None:
            self.cpp_force.clearGate()
        else:
            self.cpp_force.setGate(*gt)

    def get_local(self):
        """c_i = |psi_i|^2 of every particle at the current time step (0 for particles of another type)"""
        return self.cpp_force.getLocalValues(context.current.system.getCurrentTimeStep())

    def get_switched(self):
        """v_i = g(n_i) h(c_i) of every particle at the current time step: what the CV averages (c_i with ``global_order``)"""
        return self.cpp_force.getSwitchedValues(context.current.system.getCurrentTimeStep())

    def get_coordination(self):
        """n_i = sum_j f(r_ij): the smoothed number of neighbours of every particle at the current time step"""
        return self.cpp_force.getCoordination(context.current.system.getCurrentTimeStep())

    def get_psi(self):
        """psi_i of every particle at the current time step as an (N, 2) array of (Re, Im)"""
        return self.cpp_force.getPsi(context.current.system.getCurrentTimeStep())

    def get_global_psi(self):
        """(Re, Im) of Psi = (1 / N_type) sum_i psi_i at the current time step, with and without ``global_order``"""
        return self.cpp_force.getGlobalPsi(context.current.system.getCurrentTimeStep())

    def set_options(self, switch=None, gate=None):
        """replaces switch and gate (the defaults switch them off); takes effect with the next step.  Refused with ``global_order``; a
        refused call leaves both as they were"""
        try:
            sw, gt = self._options(switch, gate, self.global_order)  # everything is checked before anything is changed
            self._apply(sw, gt)
        except (TypeError, KeyError, ValueError, AttributeError, RuntimeError):
            raise RuntimeError("Error creating collective variable.")


def environment_templates(structure, a):
    """the template environments of a cubic lattice with the conventional lattice constant ``a``, for ``cv.environment_similarity``:
    ``"fcc"`` 12 vectors of length a / sqrt(2), ``"bcc"`` 14 vectors (the 8 nearest of length a sqrt(3) / 2 and the 6 second neighbours of
    length a, as PLUMED), ``"sc"`` 6 vectors of length a: one list of 3-vectors each; ``"diamond"``: a list of TWO environments of 4
    vectors of length a sqrt(3) / 4, (1, 1, 1)-type and its inverse, one per sublattice"""
    a = float(a)
    if not 0.0 < a < float("inf"):
        raise RuntimeError("cv.environment_templates: the lattice constant must be positive")

    def family(v):
        out = []
        for p in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
            for sx in (1.0, -1.0):
                for sy in (1.0, -1.0):
                    for sz in (1.0, -1.0):
                        t = (sx * v[p[0]] * a + 0.0, sy * v[p[1]] * a + 0.0, sz * v[p[2]] * a + 0.0)
                        if t not in out:
                            out.append(t)
        return [list(t) for t in out]

    if structure == "fcc":
        return family((0.5, 0.5, 0.0))
    if structure == "bcc":
        return family((0.5, 0.5, 0.5)) + family((1.0, 0.0, 0.0))
    if structure == "sc":
        return family((1.0, 0.0, 0.0))
    if structure == "diamond":
        first = [[s[0] * a / 4.0, s[1] * a / 4.0, s[2] * a / 4.0] for s in ((1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1))]
        return [first, [[-x + 0.0 for x in t] for t in first]]
    raise RuntimeError("cv.environment_templates: structure must be 'fcc', 'bcc', 'sc' or 'diamond'")


class environment_similarity(_neighbour_variable):
    """this build (no reference counterpart; include/mtd_abi.h "Environment similarity"): the environment similarity kernel of Piaggi and
    Parrinello (J. Chem. Phys. 150, 244119; PLUMED's ENVIRONMENTSIMILARITY).  Every particle's neighbourhood is compared with one or more
    template environments, each a list of lattice vectors in the LAB frame (``cv.environment_templates``):
    k^e_i = (1 / M_e) sum_j f(r_ij) sum_m exp(-|d_ij - T^e_m|^2 / 4 sigma_env^2), d_ij the vector from i to j, f the cosine window between
    ``r_on`` and ``r_cut``; k_i is k^1_i or, with several environments, their smooth maximum (1 / lam) ln sum_e exp(lam k^e_i);
    CV = (1 / N) sum_i h(k_i) with h(k) = k or, with ``switch=dict(c0=..., p=...)``, x^p / (1 + x^p), x = k / c0 — CV * N is then the
    smooth number of particles in the template's structure AND orientation.  ``templates``: a list of 3-vectors (one environment) or a list
    of such lists (at most 4 environments, 32 vectors each, 64 in all, every vector shorter than ``r_cut``).  Needs a full list that
    reaches ``r_cut``.  Domain-decomposed runs: one environment without a switch only.

    Virial (``get_virial``; mtd_es_forces): half of every entry at each of its ends.  The sums are -bias * dCV/d(eps_ab) under
    x_a += eps x_b of positions and box with the templates held fixed: the tensor is NOT symmetric, and xy, xz, yz are the off-diagonals a
    HOOMD box can deform along."""

    _cv = "cv.environment_similarity"

    def __init__(self, templates, sigma_env, r_cut, r_on, nlist, type, lam=100.0, switch=None, name=None, sigma=1.0):
        suffix = self._begin(sigma, name)
        try:
            type_list = context.current.type_names
            sigma_env, r_cut, r_on, lam = float(sigma_env), float(r_cut), float(r_on), float(lam)
            envs = [[[float(x) for x in t] for t in env] for env in self._environments(templates)]
            if type not in type_list or not 1 <= len(envs) <= 4 or sum(len(env) for env in envs) > 64 \
                    or not 0.0 < sigma_env < float("inf") or not 0.0 <= r_on < r_cut < float("inf") or not 0.0 < lam < float("inf") \
                    or float(nlist.r_cut) < r_cut:
                raise ValueError
            for env in envs:
                if not 1 <= len(env) <= 32:
                    raise ValueError
                for t in env:
                    if len(t) != 3 or not 0.0 < t[0] * t[0] + t[1] * t[1] + t[2] * t[2] < r_cut * r_cut:
                        raise ValueError
            sw = self._switch(switch)
            self.type = type
            self.nlist = nlist
            self.templates, self.sigma_env, self.r_cut, self.r_on, self.lam = envs, sigma_env, r_cut, r_on, lam
            self._full_list()
            self.cpp_force = _metadynamics.EnvironmentSimilarity(context.current.system_definition, envs, sigma_env, r_cut, r_on, lam,
                                                                 nlist.cpp_nlist, type_list.index(type), suffix)
            if sw is not None:
                self.cpp_force.setSwitch(*sw)
        except (TypeError, ValueError, KeyError, IndexError, AttributeError, RuntimeError):
            context.current.forces.remove(self)                      # refused: the run must not find a half-made variable
            raise RuntimeError("Error creating collective variable.")
        self._attach(type_list.index(type))

    @staticmethod
    def _environments(templates):
        """a list of 3-vectors is one environment, a list of such lists several"""
        templates = [t for t in templates]
        if len(templates) == 0:
            raise ValueError
        first = [x for x in templates[0]]
        if len(first) == 0:
            raise ValueError
        if hasattr(first[0], "__len__"):
            return [[list(t) for t in env] for env in templates]
        return [[list(t) for t in templates]]

    @staticmethod
    def _switch(switch):
        if switch is None:
            return None
        sw = (float(switch["c0"]), int(switch["p"]))
        if set(switch.keys()) != {"c0", "p"} or int(switch["p"]) != switch["p"] or not 0.0 < sw[0] < float("inf") or sw[1] < 1:
            raise ValueError
        return sw

    def get_local(self):
        """k_i of every particle at the current time step (0 for particles of another type)"""
        return self.cpp_force.getLocalValues(context.current.system.getCurrentTimeStep())

    def get_environments(self):
        """k^e_i of every particle and environment at the current time step, shape (N, E)"""
        return self.cpp_force.getEnvironmentValues(context.current.system.getCurrentTimeStep())

    def get_switched(self):
        """v_i = h(k_i) of every particle at the current time step: what the CV averages (k_i itself without a switch)"""
        return self.cpp_force.getSwitchedValues(context.current.system.getCurrentTimeStep())

    def set_switch(self, switch):
        """``dict(c0=..., p=...)`` or ``None`` (no switch); takes effect with the next step"""
        try:
            sw = self._switch(switch)
            if sw is None:
                self.cpp_force.clearSwitch()
            else:
                self.cpp_force.setSwitch(*sw)
        except (TypeError, KeyError, ValueError, AttributeError, RuntimeError):
            raise RuntimeError("Error creating collective variable.")


class nlist_cell(object):
    """Stand-in for ``hoomd.md.nlist.cell``: HOOMD's NeighborList is not part of the plugin.

    ``device=False`` (default): the list is built on the host with a periodic KD-tree (cubic boxes) whenever ``update`` is called
    and handed to the device in HOOMD's layout; without a call of ``update`` or ``set_lists`` a run raises.
    ``device=True``: the list is built on the GPU (cell list, any box of ``mtd_box``, ghosts, half or full storage) with
    ``r_list = r_cut + r_buff``, first when a run needs it and again whenever a particle has moved by more than ``r_buff / 2``
    since the last build, which is checked every ``check_period`` steps.  ``update`` then forces a rebuild and copies the arrays back."""

    def __init__(self, r_cut, r_buff=0.4, check_period=1, device=False):
        self.r_cut = float(r_cut)
        self.r_buff = float(r_buff)
        self.check_period = int(check_period)
        self.device = bool(device)
        self._type, self._types = -1, set()
        self.cpp_nlist = _metadynamics.NeighborList(context.current.system_definition)
        if self.device:
            if self.check_period < 1:
                raise RuntimeError("nlist_cell: check_period must be at least 1")
            self.cpp_nlist.setDeviceBuild(self.r_cut, self.r_buff, self.check_period, self._type)

    def _attach(self, type_id):
        """a cv.steinhardt uses this list: build only the pairs of its type; two CVs of different types need all pairs"""
        self._types.add(int(type_id))
        self._type = int(type_id) if len(self._types) == 1 else -1
        self.cpp_nlist.setDeviceBuild(self.r_cut, self.r_buff, self.check_period, self._type)

    def set_lists(self, head_list, n_neigh, nlist):
        """hand over a list in HOOMD's layout: neighbours of i are nlist[head_list[i] : head_list[i] + n_neigh[i]]"""
        self.cpp_nlist.setLists(head_list, n_neigh, nlist)

    def update(self):
        """rebuild from the current positions: on the device when ``device=True``, else cubic boxes with a host-side periodic
        KD-tree; returns (head_list, n_neigh, nlist) as host arrays"""
        if self.device:
            self.cpp_nlist.forceRebuild()
            self.cpp_nlist.compute(context.current.system.getCurrentTimeStep())
            return self.cpp_nlist.getLists()
        import numpy as np
        from scipy.spatial import cKDTree
        pdata = context.current.system_definition.getParticleData()
        L = np.asarray(pdata.getGlobalBox().getL())
        n_local = pdata.getN()
        # (a shard: the ghost particles sit behind the local ones; heads for the local particles only, entries may index ghosts)
        p = np.mod(np.asarray(pdata.getPositions()[:, :3], dtype=np.float64) + L / 2, L)
        p[p >= L] = 0.0
        pairs = cKDTree(p, boxsize=L).query_pairs(self.r_cut, output_type="ndarray")
        i = np.concatenate([pairs[:, 0], pairs[:, 1]])
        j = np.concatenate([pairs[:, 1], pairs[:, 0]])
        keep = i < n_local
        i, j = i[keep], j[keep]
        order = np.lexsort((j, i))
        i, j = i[order], j[order]
        p = p[:n_local]
        n_neigh = np.bincount(i, minlength=len(p)).astype(np.uint32)
        head = np.zeros(len(p), dtype=np.uint32)
        head[1:] = np.cumsum(n_neigh)[:-1]
        lists = (head, n_neigh, j.astype(np.uint32))
        self.set_lists(*lists)
        return lists


class wrap(_collective_variable):
    """Force wrapper (cv.py:500-537): the energy of an arbitrary force as collective variable."""

    def __init__(self, force, sigma=1.0):
        from . import force as _force_module
        if not isinstance(force, _force_module._force):
            raise RuntimeError("cv.wrap needs a md._force instance as argument.")          # cv.py:518-519
        name = "cv_" + force.name
        _collective_variable.__init__(self, sigma, name)
        self.force = force
        self.cpp_force = _metadynamics.CollectiveWrapper(context.current.system_definition, force.cpp_force, name)
        self.log = force.log

    # cv.py:531-537 call themselves recursively and name an undefined ``force``; the evident intent is kept
    def disable(self, log=False):
        self.enabled = False
        self.log = log
        self.force.enabled = False
        self.force.log = log

    def enable(self):
        self.enabled = True
        self.force.enabled = True
