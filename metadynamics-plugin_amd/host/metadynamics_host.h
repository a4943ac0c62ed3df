// metadynamics_host.h — host-side mirror of the reference plugin's C++ classes for the hot path.
//
// Same class names, method names, argument meaning and error behaviour as the reference
// (CollectiveVariable.h, LamellarOrderParameterGPU.h, WellTemperedEnsemble.h, AspectRatio.h, Density.h,
// IntegratorMetaDynamics.h); the bodies call libmtd_hip.so through include/mtd_abi.h instead of the
// CUDA drivers, and the per-step hand-off between CVs and the integrator stays in device memory:
//
//   reference                                   here
//   Scalar getCurrentValue(t) [D2H + host sum]  enqueueCurrentValue(t, engine, slot)  (async, device)
//                                               getCurrentValue(t) = the same + lazy read-back
//   setBiasFactor(Scalar)  [host scalar]        setBiasFactorDevice(const double*)    (device pointer)
//                                               setBiasFactor(Scalar) kept for umbrella / derivatives
#pragma once

#include <fstream>
#include <memory>
#include <string>
#include <vector>

#include "mini_hoomd.h"
#include "prof.h"

namespace mtdhost
{

class IntegratorMetaDynamics;

//! CollectiveVariable.h:32-196
class CollectiveVariable : public ForceCompute
    {
    public:
        enum umbrella_Enum
            {
            no_umbrella = 0,
            linear,
            harmonic,
            wall,
            gaussian
            };

        CollectiveVariable(std::shared_ptr<SystemDefinition> sysdef, const std::string &name);
        virtual ~CollectiveVariable() {}

        //! CollectiveVariable.h:55 — synchronising read-back of the CV value
        virtual double getCurrentValue(unsigned int timestep) { return 0.0; }

        //! device-resident form of getCurrentValue: make `engine` take CV `slot` from this variable.
        //! Default: the host value of getCurrentValue() travels in the next launch's arguments.
        virtual void enqueueCurrentValue(unsigned int timestep, mtd_metad *engine, unsigned int slot);
        //! A variable that is the ONLY one of the grid may run the engine's update itself, fused with the tail of its own value
        //! (cv.steinhardt: mtd_ql_finalize_update_bias): true = updateBiasPotential(timestep) is enqueued, the integrator skips
        //! mtd_metad_update_bias; false (default) = nothing fused, the integrator goes on with enqueueCurrentValue
        virtual bool enqueueValueAndBias(unsigned int timestep, mtd_metad *engine) { return false; }

        virtual void setBiasFactor(double bias)                        // CollectiveVariable.h:63-66
            {
            m_bias = bias;
            m_bias_device = nullptr;
            }
        //! the bias factor stays in device memory (written by the grid engine, read by the force kernels)
        virtual void setBiasFactorDevice(const double *d_bias) { m_bias_device = d_bias; }

        void setUmbrella(umbrella_Enum umbrella)                       // CollectiveVariable.h:71-76
            {
            m_umbrella = umbrella;
            if (umbrella == no_umbrella) m_bias = 0.0;
            }
        void setKappa(double kappa) { m_kappa = kappa; }
        void setWidthFlat(double width) { m_width_flat = width; }
        void setScale(double scale) { m_scale = scale; }
        void setMinimum(double cv0) { m_cv0 = cv0; }
        std::string getName() { return m_cv_name; }

        void computeDerivatives(unsigned int timestep)                // CollectiveVariable.h:120-125
            {
            setBiasFactor(1.0);
            computeBiasForces(timestep);
            }
        virtual bool canComputeDerivatives() { return true; }
        double getUmbrellaPotential(unsigned int timestep);           // CollectiveVariable.cc:68-106
        virtual bool requiresNetForce() { return false; }
        bool hasUmbrella() const { return m_umbrella != no_umbrella; }
        //! a domain-decomposed run (m_pdata->getDomainDecomposition() in the reference): this rank holds a shard of the
        //! particles and the per-step sums are reduced over the ranks of the execution configuration's mailbox
        bool distributed() const { return m_exec_conf->getMailbox() != nullptr; }

        std::vector<std::string> getProvidedLogQuantities() override
            {
            return {"umbrella_energy_" + m_cv_name};
            }
        double getLogValue(const std::string &quantity, unsigned int timestep) override
            {
            if (quantity == "umbrella_energy_" + m_cv_name) return getUmbrellaPotential(timestep);
            throw std::runtime_error("Error querying log quantity");     // CollectiveVariable.h:168-170
            }

    protected:
        void computeForces(unsigned int timestep) override;            // CollectiveVariable.cc:22-66
        virtual void computeBiasForces(unsigned int timestep) {}
        //! Where a force pass writes the per-particle virial of the bias force: the virial array in a constant-pressure run (the pressure
        //! flag), nullptr otherwise — and a virial array somebody has allocated earlier is then zeroed, so that a stale virial is never read
        void *virialTarget();

        double m_bias;
        const double *m_bias_device;
        std::string m_cv_name;

    private:
        umbrella_Enum m_umbrella;
        double m_cv0, m_kappa, m_width_flat, m_scale;
    };

//! LamellarOrderParameterGPU.h / LamellarOrderParameter.h:30-101
class LamellarOrderParameterGPU : public CollectiveVariable
    {
    public:
        LamellarOrderParameterGPU(std::shared_ptr<SystemDefinition> sysdef, const std::vector<double> &mode,
                                  const std::vector<int3> &lattice_vectors, const std::string &suffix = "");
        void computeBiasForces(unsigned int timestep) override;        // LamellarOrderParameterGPU.cc:99-132
        double getCurrentValue(unsigned int timestep) override;        // LamellarOrderParameter.h:75-79 (always recomputes, Q4)
        void enqueueCurrentValue(unsigned int timestep, mtd_metad *engine, unsigned int slot) override;
        std::vector<std::string> getProvidedLogQuantities() override
            {
            auto l = CollectiveVariable::getProvidedLogQuantities();
            l.push_back(m_log_name);
            return l;
            }
        double getLogValue(const std::string &quantity, unsigned int timestep) override
            {
            if (quantity == m_log_name) return getCurrentValue(timestep);
            return CollectiveVariable::getLogValue(quantity, timestep);
            }
        const std::vector<double> &getMode() const { return m_mode; }
        const std::vector<int3> &getLatticeVectors() const { return m_lattice_vectors; }
        //! this build: trigonometry of THIS variable's kernels (MTD_TRIG_DEFAULT / _HARDWARE / _ACCURATE, mtd_abi.h); variables
        //! that share a fused launch take the accurate functions as soon as one of them asks for them
        void setTrigMode(int mode)
            {
            if (mode != MTD_TRIG_DEFAULT && mode != MTD_TRIG_HARDWARE && mode != MTD_TRIG_ACCURATE)
                throw std::runtime_error("cv.lamellar: trig mode must be 0 (default), 1 (hardware) or 2 (accurate)");
            m_set.trig_mode = mode;
            }
        int getTrigMode() const { return m_set.trig_mode; }

    protected:
        void enqueuePartials();
        std::string m_log_name;
        std::vector<double> m_mode;
        std::vector<int3> m_lattice_vectors;
        mtd_lamellar_set m_set;
        DeviceBuffer m_partials, m_cv_dev;
        unsigned int m_n_partials;
        double m_cv;
        unsigned int m_cv_last_updated;
    };

//! WellTemperedEnsemble.h:20-113
class WellTemperedEnsemble : public CollectiveVariable
    {
    public:
        WellTemperedEnsemble(std::shared_ptr<SystemDefinition> sysdef, const std::string &name);
        bool requiresNetForce() override { return true; }
        double getCurrentValue(unsigned int timestep) override;        // WellTemperedEnsemble.h:50-54
        void enqueueCurrentValue(unsigned int timestep, mtd_metad *engine, unsigned int slot) override;
        void computeBiasForces(unsigned int timestep) override;        // WellTemperedEnsemble.cc:135-188
        std::vector<std::string> getProvidedLogQuantities() override
            {
            auto l = CollectiveVariable::getProvidedLogQuantities();
            l.push_back(m_log_name);
            return l;
            }
        double getLogValue(const std::string &quantity, unsigned int timestep) override
            {
            if (quantity == m_log_name) return getCurrentValue(timestep);
            return CollectiveVariable::getLogValue(quantity, timestep);
            }

    protected:
        void enqueuePartials();
        double m_pe;
        std::string m_log_name;
        DeviceBuffer m_partials, m_sum;
        unsigned int m_n_partials;
    };

//! OrderParameterMeshGPU.h / OrderParameterMesh.h:20-180 (single rank: no ghost cells, no dfft)
class OrderParameterMeshGPU : public CollectiveVariable
    {
    public:
        OrderParameterMeshGPU(std::shared_ptr<SystemDefinition> sysdef, unsigned int nx, unsigned int ny, unsigned int nz,
                              std::vector<double> mode, std::vector<int3> zero_modes);
        virtual ~OrderParameterMeshGPU();
        double getCurrentValue(unsigned int timestep) override;        // OrderParameterMesh.cc:925-968 (cached per timestep)
        void enqueueCurrentValue(unsigned int timestep, mtd_metad *engine, unsigned int slot) override;
        void computeBiasForces(unsigned int timestep) override;        // OrderParameterMesh.cc:1052-1075
        //! convolution-kernel table: stored like the reference, which never applies it to the mesh (Q7)
        void setTable(const std::vector<double> &K, const std::vector<double> &d_K, double kmin, double kmax);   // :148-189
        void setUseTable(bool use_table);                             // OrderParameterMesh.h:60-63
        //! this build: false = interpolation function as intended instead of the reference's unsigned division (Q6)
        void setBugCompatible(bool on);
        //! this build, domain-decomposed runs: true = the mesh is DECOMPOSED into slabs over the ranks (mtd_mesh_slab_*: the
        //! reference's ghost-cell exchange + distributed FFT, OrderParameterMesh.cc:263-316, 659-746); false (default) = every
        //! rank keeps the whole mesh and the ranks sum their assignments (M + 1 doubles per step, :630).  Before the first step.
        void setSlabDecomposition(bool on);
        bool getSlabDecomposition() const { return m_slab; }
        //! the lamellar CVs of a mixed set (and the engine's deferred grid pass) ride in this mesh's next particle pass
        //! (mtd_mesh_set_lamellar_rider); false when the mesh cannot carry them or is already up to date for `timestep`
        bool armLamellarRider(unsigned int timestep, mtd_metad *engine, const mtd_lamellar_set *set, double *d_partials,
                              unsigned int *n_partials);
        //! true when riders armed earlier are still waiting (nothing consumed them): they are disarmed
        bool clearRider();
        //! The end of a mixed set's step in ONE launch (mtd_mesh_forces_update_bias): the grid engine's launch — scalar chain, first
        //! grid pass, the lamellar CVs' forces — inside this variable's force pass.  false: the shapes do not allow it (the caller
        //! runs the engine's launch, the force pass follows in computeBiasForces as always).  true: the forces of `timestep` are
        //! written (with the bias factor of this very step) and marked as computed.
        bool forcesWithBiasUpdate(unsigned int timestep, mtd_metad *engine, unsigned int mesh_slot, const mtd_lamellar_set *set,
                                  const unsigned int *slots, void *const *lamellar_forces);
        std::vector<std::string> getProvidedLogQuantities() override
            {
            auto l = CollectiveVariable::getProvidedLogQuantities();
            for (const char *n : {"cv_mesh", "qx_max", "qy_max", "qz_max", "sq_max"}) l.push_back(n);   // OrderParameterMesh.cc:118-122
            return l;
            }
        double getLogValue(const std::string &quantity, unsigned int timestep) override;   // :1077-1106

    private:
        void enqueueCV(unsigned int timestep);
        void attachSlab();
        bool m_slab = false, m_slab_attached = false;
        const double *m_slab_sum = nullptr;
        void needFourierMesh();
        bool m_keep_fourier;
        void computeQmax(unsigned int timestep);                      // :1108-1179
        void computeVirial();                                         // :970-1050
        unsigned int m_q_max_last_computed;
        double m_q_max[3], m_sq_max;
        mtd_mesh *m_mesh;
        std::vector<double> m_mode;
        std::vector<int3> m_zero_modes;          // stored and never read, like the reference (OrderParameterMesh.cc:59-63)
        std::vector<double> m_table, m_table_d;
        double m_k_min, m_k_max, m_delta_k;
        bool m_use_table, m_is_first_step;
        const double *m_partials;
        unsigned int m_n_partials, m_cv_last_updated;
        double m_cv;
        DeviceBuffer m_cv_dev;
    };

//! CollectiveWrapper.h / CollectiveWrapper.cc:13-188: the energy of any ForceCompute as collective variable
class CollectiveWrapper : public CollectiveVariable
    {
    public:
        CollectiveWrapper(std::shared_ptr<SystemDefinition> sysdef, std::shared_ptr<ForceCompute> fc, const std::string &name);
        double getCurrentValue(unsigned int timestep) override;        // CollectiveWrapper.h: computeCV then m_energy
        void enqueueCurrentValue(unsigned int timestep, mtd_metad *engine, unsigned int slot) override;
        void computeBiasForces(unsigned int timestep) override;        // CollectiveWrapper.cc:136-179
        std::vector<std::string> getProvidedLogQuantities() override
            {
            auto l = CollectiveVariable::getProvidedLogQuantities();
            l.push_back(m_cv_name);
            return l;
            }
        double getLogValue(const std::string &quantity, unsigned int timestep) override
            {
            if (quantity == m_cv_name) return getCurrentValue(timestep);
            return CollectiveVariable::getLogValue(quantity, timestep);
            }

    private:
        void enqueuePartials(unsigned int timestep);
        std::shared_ptr<ForceCompute> m_fc;
        double m_energy;
        DeviceBuffer m_partials, m_sum;
        unsigned int m_n_partials;
    };

//! SteinhardtQl.h:15-98 (the reference class is host-only; this one runs the same arithmetic on the device)
class SteinhardtQl : public CollectiveVariable
    {
    public:
        SteinhardtQl(std::shared_ptr<SystemDefinition> sysdef, double rcut, double ron, unsigned int lmax,
                     std::shared_ptr<NeighborList> nlist, unsigned int type, const std::vector<double> &Ql_ref,
                     const std::string &log_suffix = "");
        double getCurrentValue(unsigned int timestep) override;        // SteinhardtQl.h:44-48
        void enqueueCurrentValue(unsigned int timestep, mtd_metad *engine, unsigned int slot) override;
        bool enqueueValueAndBias(unsigned int timestep, mtd_metad *engine) override;
        //! this build: the steps of this variable can be replayed from a captured graph (no half-list scratch from a pool, no list rebuild
        //! pending; a device-built list reads its rebuild flag on the host every check, which a replayed graph would skip)
        bool graphSafe() { return !m_nlist->isDeviceBuild() && lists().mode != 1; }
        void computeBiasForces(unsigned int timestep) override;        // SteinhardtQl.cc:203-339
        std::vector<std::string> getProvidedLogQuantities() override;  // SteinhardtQl.h:34-42
        double getLogValue(const std::string &quantity, unsigned int timestep) override;   // :49-67

    private:
        void computeCV(unsigned int timestep);                         // SteinhardtQl.cc:62-201
        void accumulateSums(unsigned int timestep);                    // :62-171 + the sum over the ranks (:183-191): Q'_lm in m_scratch
        double m_rcut, m_ron;
        unsigned int m_lmax;
        std::shared_ptr<NeighborList> m_nlist;
        unsigned int m_type;
        std::vector<double> m_Ql_ref, m_Ql;
        unsigned int m_cv_last_updated;
        bool m_have_computed;
        double m_value;
        DeviceBuffer m_scratch;
        const double *m_d_value, *m_d_Ql, *m_d_Qlm;
        // half lists: the symmetric full list the half list stands for (mtd_ql_symmetrize_half_list), rebuilt when the
        // neighbour list changes; the passes then run in the symmetric-full-list mode (no atomics in the force pass)
        struct Lists
            {
            const unsigned int *head, *n_neigh, *nlist;
            int mode;                                                 // half_nlist of the mtd_ql_* calls
            };
        Lists lists();
        DeviceBuffer m_sym_head, m_sym_nneigh, m_sym_nlist, m_sym_work;
        unsigned int m_sym_version;
        bool m_sym_ok;
    };

//! What the variables that walk the rows of a FULL neighbour list share (SteinhardtLocal, PairEntropy, EnvironmentSimilarity,
//! PairEntropyLocal, DebyeStructureFactor, CoordinationNumber, TetrahedralOrder, HexaticOrder): the list, the particle type, the scratch the passes leave their results
//! in and its growth, "this step is computed already", the refusals of a list that does not fit, the call block of a step, the
//! all-reduce of a step's sums, the opening of a force pass, the value as one device double, the synchronising read-backs and the
//! cv_<name> log quantity.  A subclass supplies computeCV (its checks in its own order: full list, distributed, reach, then the list's
//! compute) and the force pass.  SteinhardtQl stays outside: its lists have a mode and a symmetrised copy.
class NeighbourVariable : public CollectiveVariable
    {
    public:
        std::vector<std::string> getProvidedLogQuantities() override;  //!< the umbrella's and cv_<name>
        double getLogValue(const std::string &quantity, unsigned int timestep) override;
        //! For a variable whose value is ONE device double that computeCV leaves at m_d_value (PairEntropy, DebyeStructureFactor,
        //! CoordinationNumber): the synchronising read-back, and that double as the engine's source, no host synchronisation.  The
        //! variables that average block sums override both
        double getCurrentValue(unsigned int timestep) override;
        void enqueueCurrentValue(unsigned int timestep, mtd_metad *engine, unsigned int slot) override;

    protected:
        //! `kind` ("pair_entropy"): the variable is called kind + log_suffix and its messages begin with "cv.<kind>: "
        NeighbourVariable(std::shared_ptr<SystemDefinition> sysdef, const char *kind, const std::string &log_suffix,
                          std::shared_ptr<NeighborList> nlist, unsigned int type);
        virtual void computeCV(unsigned int timestep) = 0;
        //! the results in the scratch are those of `timestep` / now are / are no longer anybody's (an option has changed)
        bool fresh(unsigned int timestep) const { return m_have_computed && m_cv_last_updated == timestep; }
        void computed(unsigned int timestep)
            {
            m_have_computed = true;
            m_cv_last_updated = timestep;
            }
        void invalidate() { m_have_computed = false; }
        void requireFullList() const;                                  //!< throws for a half list
        void requireReach(double r_cut, const char *what) const;       //!< throws when a device-built list is shorter than r_cut (`what` names it)
        struct Lists
            {
            const unsigned int *head, *n_neigh, *nlist;
            };
        Lists lists() const;
        //! the call block of this step's passes (include/mtd_abi.h, mtd_row_call): particles, ghosts, `box`, the list, m_scratch, the stream
        mtd_row_call rowCall(const mtd_box *box) const;
        //! m_scratch holds at least `bytes`; when it had to grow nothing in it is any step's (computeCV forms it anew: invalidate)
        void growScratch(size_t bytes);
        //! a domain-decomposed run adds the ranks' n_sums doubles at d_sums: the same bits everywhere afterwards
        void reduceOverRanks(double *d_sums, unsigned int n_sums);
        //! The opening of every computeBiasForces: the "Force" range, computeCV unless this step is computed, the list, the box and where
        //! the virial goes (CollectiveVariable::virialTarget)
        struct ForcePass
            {
            ForcePass(NeighbourVariable &cv, unsigned int timestep);
            ProfRange range;
            mtd_box box;
            void *virial;
            };
        //! computeCV, then synchronising copies: n doubles at d_src; one double; the sum of the block sums times 1 / N_global (through m_sum).
        //! A caller that hands on a pointer computeCV sets calls computeCV itself first
        std::vector<double> readBack(const double *d_src, size_t n, const char *what, unsigned int timestep);
        double readValue(const double *d_src, unsigned int timestep);
        double readPartials(const double *d_partials, unsigned int n_partials, unsigned int timestep);
        //! The largest-cluster option of a variable whose accumulate takes mtd_cluster_params (include/mtd_abi.h "Clusters";
        //! CoordinationNumber, TetrahedralOrder — SteinhardtLocal keeps its own members): the parameters, a scratch that grows and never
        //! shrinks, and where the cluster pass of the last computeCV left mask, labels and summary
        struct LargestCluster
            {
            mtd_cluster_params par = {0, 0.0, 0.0};
            DeviceBuffer scratch;
            const double *d_w = nullptr;
            const unsigned int *d_label = nullptr, *d_summary = nullptr;
            };
        //! v_min finite, r_link > 0 and within the reach of a device-built list, else throws and leaves the option as it was; both invalidate
        void setLargestCluster(LargestCluster &cl, double v_min, double r_link);
        void clearLargestCluster(LargestCluster &cl);
        //! at compute time: NULL with the option off; else the reach checked again (the list may have changed) and the scratch grown
        void *largestClusterScratch(LargestCluster &cl);
        //! throws without the option; computeCV, then a synchronising copy of n words at *d_src (read after computeCV has set it)
        std::vector<unsigned int> readClusterWords(const LargestCluster &cl, const unsigned int *const *d_src, size_t n, const char *what,
                                                   unsigned int timestep);
        std::vector<double> readClusterMask(const LargestCluster &cl, unsigned int timestep);

        std::string m_prefix;                                         // "cv.<kind>: "
        std::shared_ptr<NeighborList> m_nlist;
        unsigned int m_type;
        DeviceBuffer m_scratch, m_sum;                                 // (m_sum: one double, sized by the variables that reduce block sums)
        const double *m_d_value;                                       // the value inside m_scratch, where it is one double (see getCurrentValue)

    private:
        unsigned int m_cv_last_updated;
        bool m_have_computed;
    };

//! Local Steinhardt bond order (no reference counterpart; include/mtd_abi.h "Local Steinhardt bond order"): the harmonics summed
//! over one particle's own neighbours, squared per particle, averaged over the particles: s = (1/N_global) sum_i sum_l Ql_ref[l] q_l^2(i)
class SteinhardtLocal : public NeighbourVariable
    {
    public:
        SteinhardtLocal(std::shared_ptr<SystemDefinition> sysdef, double rcut, double ron, unsigned int lmax,
                        std::shared_ptr<NeighborList> nlist, unsigned int type, const std::vector<double> &Ql_ref,
                        const std::string &log_suffix = "");
        double getCurrentValue(unsigned int timestep) override;
        //! device-resident: the block sums of c_i become the engine's source of this variable, no host synchronisation
        void enqueueCurrentValue(unsigned int timestep, mtd_metad *engine, unsigned int slot) override;
        void computeBiasForces(unsigned int timestep) override;
        std::vector<double> getLocalValues(unsigned int timestep);     //!< c_i of every local particle (0 for other types)
        std::vector<double> getCoordination(unsigned int timestep);    //!< n_i = sum_j f(r_ij)
        //! the options of mtd_ql_local_options; every change invalidates the cached step
        void setAverage(bool on);                                      //!< neighbour-averaged qbar_lm(i) in place of q_lm(i)
        void setSwitch(double c0, unsigned int p);                     //!< h(c) = x^p / (1 + x^p), x = max(c, 0) / c0
        void clearSwitch();
        void setGate(double n_lo, double n_hi);                        //!< g(n) = smoothstep from n_lo to n_hi
        void clearGate();
        std::vector<double> getSwitchedValues(unsigned int timestep);  //!< v_i = g(n_i) h(c_i) (c_i without options; h(b_i) with bonds)
        //! the solid-bond count of mtd_ql_local_bonds: switch and gate then act on b_i = sum_j f sigma(d_ij); not with the average
        void setBonds(double d_lo, double d_hi);                       //!< sigma = smoothstep of d_ij from d_lo to d_hi, -1 <= d_lo < d_hi <= 1
        void clearBonds();
        std::vector<double> getBondCounts(unsigned int timestep);      //!< b_i of every local particle; throws without bonds
        //! the largest cluster of mtd_cluster_params (include/mtd_abi.h "Clusters"): the variable becomes (1/N) sum of v_i over the largest
        //! connected cluster of particles with v_i >= v_min, linked within r_link; not with the average.  getSwitchedValues stays unmasked
        void setCluster(double v_min, double r_link);                  //!< v_min finite, r_link > 0 and within the reach of a device-built list
        void clearCluster();
        //! the only places that read the cluster pass back; all three throw without the option
        std::vector<unsigned int> getClusterLabels(unsigned int timestep);   //!< smallest index of i's cluster, MTD_CLUSTER_NONE for a non-node
        std::vector<double> getClusterMask(unsigned int timestep);           //!< w_i: 1 for the members of the largest cluster, else 0
        std::vector<unsigned int> getLargestCluster(unsigned int timestep);  //!< {root, members, number of clusters, number of nodes}

    private:
        void computeCV(unsigned int timestep) override;
        std::vector<unsigned int> readBackWords(const unsigned int *d_src, size_t n, const char *what, unsigned int timestep);
        double m_rcut, m_ron;
        unsigned int m_lmax;
        std::vector<double> m_Ql_ref;
        const double *m_d_partials, *m_d_c, *m_d_n, *m_d_v, *m_d_b;
        unsigned int m_n_partials;
        mtd_ql_local_options m_opt;
        mtd_ql_local_bonds m_bonds;
        mtd_cluster_params m_cluster;
        DeviceBuffer m_cluster_scratch;                                // grown like m_scratch, never shrinks
        const double *m_d_w;
        const unsigned int *m_d_label, *m_d_summary;
    };

//! Pair entropy (no reference counterpart; include/mtd_abi.h "Pair entropy"): S2 from a Gaussian-smoothed g(r) of one particle type.
//! Works domain-decomposed: the only exchange is one allreduceSmall of the n_bins + 1 sums.
class PairEntropy : public NeighbourVariable
    {
    public:
        PairEntropy(std::shared_ptr<SystemDefinition> sysdef, double r_max, double sigma_r, unsigned int n_bins,
                    std::shared_ptr<NeighborList> nlist, unsigned int type, const std::string &log_suffix = "");
        void computeBiasForces(unsigned int timestep) override;
        std::vector<double> getGr(unsigned int timestep);              //!< g_b of the n_bins bins (r_b = (b + 1/2) r_max / n_bins)
        double getRCut() const { return m_r_max + 4.0 * m_sigma_r; }   //!< what the neighbour list must reach

    private:
        void computeCV(unsigned int timestep) override;
        double m_r_max, m_sigma_r;
        unsigned int m_n_bins;
        const double *m_d_g;
    };

//! Environment similarity (no reference counterpart; include/mtd_abi.h "Environment similarity"): every particle's neighbourhood compared
//! with template environments in a fixed orientation, s = (1/N_global) sum_i h(k_i).  Domain-decomposed runs: the plain variable (one
//! environment, no switch) only — beta of a ghost neighbour would have to be exchanged otherwise.
class EnvironmentSimilarity : public NeighbourVariable
    {
    public:
        //! templates: the environments, each a list of 3-vectors
        EnvironmentSimilarity(std::shared_ptr<SystemDefinition> sysdef, const std::vector<std::vector<std::vector<double>>> &templates,
                              double sigma_env, double r_cut, double r_on, double lambda, std::shared_ptr<NeighborList> nlist,
                              unsigned int type, const std::string &log_suffix = "");
        double getCurrentValue(unsigned int timestep) override;
        //! device-resident: the block sums of v_i become the engine's source of this variable, no host synchronisation
        void enqueueCurrentValue(unsigned int timestep, mtd_metad *engine, unsigned int slot) override;
        void computeBiasForces(unsigned int timestep) override;
        std::vector<double> getLocalValues(unsigned int timestep);         //!< k_i of every local particle (0 for other types)
        std::vector<double> getEnvironmentValues(unsigned int timestep);   //!< k^e_i, N x E row-major
        std::vector<double> getSwitchedValues(unsigned int timestep);      //!< v_i = h(k_i)
        unsigned int getNumEnvironments() const { return m_par.n_env; }
        double getRCut() const { return m_par.r_cut; }                     //!< what the neighbour list must reach
        //! h(k) = x^p / (1 + x^p), x = k / c0; every change invalidates the cached step
        void setSwitch(double c0, unsigned int p);
        void clearSwitch();

    private:
        void computeCV(unsigned int timestep) override;
        mtd_es_params m_par;
        const double *m_d_partials, *m_d_k, *m_d_ke, *m_d_v;
        unsigned int m_n_partials;
    };

//! Local pair entropy (no reference counterpart; include/mtd_abi.h "Local pair entropy"): the pair entropy s_i of every particle's own g_i(r),
//! optionally averaged over the first shell and counted through a switch, s = (1/N_global) sum_i v_i.  Single-domain runs only: the force
//! on a particle reads W_j, alpha_j and s_j of its neighbours, which a ghost does not have.
class PairEntropyLocal : public NeighbourVariable
    {
    public:
        PairEntropyLocal(std::shared_ptr<SystemDefinition> sysdef, double r_max, double sigma_r, unsigned int n_bins,
                         std::shared_ptr<NeighborList> nlist, unsigned int type, const std::string &log_suffix = "");
        double getCurrentValue(unsigned int timestep) override;
        //! device-resident: the block sums of v_i become the engine's source of this variable, no host synchronisation
        void enqueueCurrentValue(unsigned int timestep, mtd_metad *engine, unsigned int slot) override;
        void computeBiasForces(unsigned int timestep) override;
        //! the options of mtd_pel_params; every change invalidates the cached step
        void setAverage(double a_on, double a_cut);                    //!< sbar_i over the cosine window a_on .. a_cut <= getRCut()
        void clearAverage();
        void setSwitch(double c0, unsigned int p);                     //!< v_i = h(-sbar_i), h(c) = x^p / (1 + x^p), x = max(c, 0) / c0
        void clearSwitch();
        std::vector<double> getLocalValues(unsigned int timestep);     //!< s_i of every local particle (0 for other types)
        std::vector<double> getAveragedValues(unsigned int timestep);  //!< sbar_i (s_i without the average)
        std::vector<double> getSwitchedValues(unsigned int timestep);  //!< v_i (sbar_i without the switch)
        double getRCut() const { return m_par.r_max + 4.0 * m_par.sigma_r; }   //!< what the neighbour list must reach

    private:
        void computeCV(unsigned int timestep) override;
        mtd_pel_call call(const mtd_box *box);
        mtd_pel_params m_par;
        const double *m_d_partials, *m_d_s, *m_d_sbar, *m_d_v;
        unsigned int m_n_partials;
    };

//! Debye structure factor (no reference counterpart; include/mtd_abi.h "Debye structure factor"): the weighted intensities of diffraction
//! peaks at given wave numbers from the Debye scattering function of one particle type.  Works domain-decomposed: the only exchange is
//! one allreduceSmall of the P + 1 sums (and of the n_q + 1 sums of a spectrum).
class DebyeStructureFactor : public NeighbourVariable
    {
    public:
        DebyeStructureFactor(std::shared_ptr<SystemDefinition> sysdef, const std::vector<double> &q, const std::vector<double> &weights,
                             double r_cut, std::shared_ptr<NeighborList> nlist, unsigned int type, const std::string &log_suffix = "");
        void computeBiasForces(unsigned int timestep) override;
        std::vector<double> getIntensities(unsigned int timestep);     //!< I_p of the P peaks
        std::vector<double> getLocalValues(unsigned int timestep);     //!< s_i of every local particle (0 for other types)
        //! I(Q_m) on n_q equally spaced wave numbers q_min .. q_max: a diagnostic, all-reduced in a distributed run, not biased
        std::vector<double> getSpectrum(unsigned int timestep, double q_min, double q_max, unsigned int n_q);
        double getRCut() const { return m_par.r_cut; }                 //!< what the neighbour list must reach

    private:
        void computeCV(unsigned int timestep) override;
        mtd_dsf_call call(const mtd_box *box);                         //!< rowCall behind a scratch grown to this step's particle count
        mtd_dsf_params m_par;
        const double *m_d_intensity, *m_d_local;
    };

//! Coordination number (no reference counterpart; include/mtd_abi.h "Coordination number"): the mean number of partners of type B around
//! the particles of type A through a rational switching function, plain or counted through a switch on every particle's number.  The
//! plain variable works domain-decomposed: the only exchange is one allreduceSmall of two sums.  With a switch: single-domain runs only,
//! the force on a particle reads g'(n_j) of its neighbours, which a ghost does not have.
class CoordinationNumber : public NeighbourVariable
    {
    public:
        CoordinationNumber(std::shared_ptr<SystemDefinition> sysdef, double r_0, double d_0, unsigned int n, unsigned int m, double r_cut,
                           std::shared_ptr<NeighborList> nlist, unsigned int type_a, unsigned int type_b, const std::string &log_suffix = "");
        void computeBiasForces(unsigned int timestep) override;
        std::vector<double> getLocalValues(unsigned int timestep);     //!< n_i of every local particle (0 for particles not of type A)
        std::vector<double> getSwitchedValues(unsigned int timestep);  //!< v_i = g(n_i) (n_i without a switch)
        //! h(c) = y^p / (1 + y^p), y = c / c0, or 1 - h with `less`; every change invalidates the cached step
        void setSwitch(double c0, unsigned int p, bool less);
        void clearSwitch();                                            //!< throws while a cluster is on
        double getRCut() const { return m_par.r_cut; }                 //!< what the neighbour list must reach
        //! the largest cluster of mtd_cluster_params (include/mtd_abi.h "Clusters"): the variable becomes (1/N_A) sum of v_i over the
        //! largest connected cluster of A particles with v_i >= v_min, linked within r_link; needs a switch; single-domain only.
        //! getSwitchedValues stays unmasked
        void setCluster(double v_min, double r_link);                  //!< v_min finite, r_link > 0 and within the reach of a device-built list
        void clearCluster();
        //! the only places that read the cluster pass back; all three throw without the option
        std::vector<unsigned int> getClusterLabels(unsigned int timestep);   //!< smallest index of i's cluster, MTD_CLUSTER_NONE for a non-node
        std::vector<double> getClusterMask(unsigned int timestep);           //!< w_i: 1 for the members of the largest cluster, else 0
        std::vector<unsigned int> getLargestCluster(unsigned int timestep);  //!< {root, members, number of clusters, number of nodes}

    private:
        void computeCV(unsigned int timestep) override;
        mtd_coord_call call(const mtd_box *box);                       //!< rowCall behind a scratch grown to this step's particle count
        mtd_coord_params m_par;
        const double *m_d_local, *m_d_switched;
        LargestCluster m_cluster;
    };

//! Tetrahedral order (no reference counterpart; include/mtd_abi.h "Tetrahedral order"): the bond-angle order t_i of every particle from the
//! moments of its neighbour row, optionally counted through a switch and gated by the coordination, or the three-body penalty A_i;
//! s = (1/N_t) sum_i v_i.  Single-domain runs only: the force on a particle reads the adjoint row of its neighbours, which a ghost does
//! not have.
class TetrahedralOrder : public NeighbourVariable
    {
    public:
        TetrahedralOrder(std::shared_ptr<SystemDefinition> sysdef, double r_cut, double r_on, double cos0, bool normalise,
                         std::shared_ptr<NeighborList> nlist, unsigned int type, const std::string &log_suffix = "");
        void computeBiasForces(unsigned int timestep) override;
        std::vector<double> getLocalValues(unsigned int timestep);     //!< t_i of every local particle (A_i when not normalised; 0 for other types)
        std::vector<double> getSwitchedValues(unsigned int timestep);  //!< v_i = g(n_i) h(t_i) (t_i without options; A_i when not normalised)
        std::vector<double> getCoordination(unsigned int timestep);    //!< n_i = sum_j f(r_ij)
        //! the switch and the gate of mtd_ql_local_options, with n_lo >= 1; both need `normalise`; every change invalidates the cached step
        void setSwitch(double c0, unsigned int p);                     //!< h(t) = x^p / (1 + x^p), x = max(t, 0) / c0
        void clearSwitch();
        void setGate(double n_lo, double n_hi);                        //!< g(n) = smoothstep from n_lo to n_hi
        void clearGate();
        double getRCut() const { return m_par.r_cut; }                 //!< what the neighbour list must reach
        //! the largest cluster of mtd_cluster_params (include/mtd_abi.h "Clusters"): the variable becomes (1/N_t) sum of v_i over the
        //! largest connected cluster of particles with v_i >= v_min, linked within r_link; needs `normalise`.  getSwitchedValues stays
        //! unmasked
        void setCluster(double v_min, double r_link);                  //!< v_min finite, r_link > 0 and within the reach of a device-built list
        void clearCluster();
        //! the only places that read the cluster pass back; all three throw without the option
        std::vector<unsigned int> getClusterLabels(unsigned int timestep);   //!< smallest index of i's cluster, MTD_CLUSTER_NONE for a non-node
        std::vector<double> getClusterMask(unsigned int timestep);           //!< w_i: 1 for the members of the largest cluster, else 0
        std::vector<unsigned int> getLargestCluster(unsigned int timestep);  //!< {root, members, number of clusters, number of nodes}

    private:
        void computeCV(unsigned int timestep) override;
        mtd_tet_call call(const mtd_box *box);                         //!< rowCall behind a scratch grown to this step's particle count
        mtd_tet_params m_par;
        const double *m_d_local, *m_d_switched, *m_d_coordination;
        LargestCluster m_cluster;
    };

//! Bond-orientational order (no reference counterpart; include/mtd_abi.h "Bond-orientational order"): the k-fold order psi_i of every
//! particle about a lab axis, the layer normal, from the sectoral harmonics of its neighbour row; s = (1/N_t) sum_i g(n_i) h(|psi_i|^2),
//! or with `global_order` s = |(1/N_t) sum_i psi_i|^2.  Single-domain runs only: the force on a particle reads the adjoint row of its
//! neighbours, which a ghost does not have.
class HexaticOrder : public NeighbourVariable
    {
    public:
        HexaticOrder(std::shared_ptr<SystemDefinition> sysdef, unsigned int k, unsigned int axis, double r_cut, double r_on, bool global_order,
                     std::shared_ptr<NeighborList> nlist, unsigned int type, const std::string &log_suffix = "");
        void computeBiasForces(unsigned int timestep) override;
        std::vector<double> getLocalValues(unsigned int timestep);     //!< c_i = |psi_i|^2 of every local particle (0 for other types)
        std::vector<double> getSwitchedValues(unsigned int timestep);  //!< v_i = g(n_i) h(c_i) (c_i without options and with global_order)
        std::vector<double> getCoordination(unsigned int timestep);    //!< n_i = sum_j f(r_ij)
        std::vector<double> getPsi(unsigned int timestep);             //!< psi_i as N interleaved (Re, Im) pairs
        std::vector<double> getGlobalPsi(unsigned int timestep);       //!< (Re, Im) of Psi = (1/N_t) sum_i psi_i, in both modes
        //! the switch and the gate of mtd_ql_local_options, with n_lo >= 0; neither with `global_order`; every change invalidates the
        //! cached step
        void setSwitch(double c0, unsigned int p);                     //!< h(c) = x^p / (1 + x^p), x = max(c, 0) / c0
        void clearSwitch();
        void setGate(double n_lo, double n_hi);                        //!< g(n) = smoothstep from n_lo to n_hi
        void clearGate();
        double getRCut() const { return m_par.r_cut; }                 //!< what the neighbour list must reach

    private:
        void computeCV(unsigned int timestep) override;
        mtd_hex_call call(const mtd_box *box);                         //!< rowCall behind a scratch grown to this step's particle count
        mtd_hex_params m_par;
        const double *m_d_local, *m_d_switched, *m_d_coordination, *m_d_psi;
    };

//! Bragg intensity (no reference counterpart; include/mtd_abi.h "Bragg intensity"): s = sum_k w_k |rho_k|^2 / A1^2 (or sum_k w_k |rho_k| / A1)
//! over chosen reciprocal-lattice vectors of the global box — the lamellar variable without its dependence on where the density wave
//! sits.  A plain CollectiveVariable on purpose: not a LamellarOrderParameterGPU (the integrator would fuse it into the lamellar
//! launches, which sum Re rho_k) and not a NeighbourVariable (there is no list).  The integrator takes its value as one device double
//! (enqueueCurrentValue) and hands the bias factor back on the device.  Computed once per time step; an option that changes invalidates.
//! Works domain-decomposed with any split of the particles: the only exchange is one allreduceSmall of the 2K + 2 sums.  The bias force
//! has no virial (the phases depend on fractional coordinates only), and none is written.
class BraggIntensity : public CollectiveVariable
    {
    public:
        BraggIntensity(std::shared_ptr<SystemDefinition> sysdef, const std::vector<double> &mode, const std::vector<int3> &lattice_vectors,
                       const std::vector<double> &weights, bool modulus, const std::string &suffix = "");
        double getCurrentValue(unsigned int timestep) override;
        void enqueueCurrentValue(unsigned int timestep, mtd_metad *engine, unsigned int slot) override;
        void computeBiasForces(unsigned int timestep) override;
        std::vector<std::string> getProvidedLogQuantities() override
            {
            auto l = CollectiveVariable::getProvidedLogQuantities();
            l.push_back(m_cv_name);
            return l;
            }
        double getLogValue(const std::string &quantity, unsigned int timestep) override
            {
            if (quantity == m_cv_name) return getCurrentValue(timestep);
            return CollectiveVariable::getLogValue(quantity, timestep);
            }
        std::vector<double> getStructureFactors(unsigned int timestep);    //!< S_k = |rho_k|^2 / A2
        std::vector<double> getAmplitudes(unsigned int timestep);          //!< Re rho_0, Im rho_0, Re rho_1, ...: 2 K numbers
        void setWeights(const std::vector<double> &weights);               //!< K finite numbers
        std::vector<double> getWeights() const { return std::vector<double>(m_par.weights, m_par.weights + m_par.n_modes); }
        void setTrigMode(int mode);                                        //!< MTD_TRIG_DEFAULT / _HARDWARE / _ACCURATE, as cv.lamellar
        int getTrigMode() const { return m_par.trig_mode; }
        bool getModulus() const { return m_par.modulus != 0; }

    private:
        void computeCV(unsigned int timestep);
        mtd_bragg_call call(const mtd_box *box);
        std::vector<double> readBack(const double *const *d_src, size_t n, const char *what, unsigned int timestep);
        mtd_bragg_params m_par;
        DeviceBuffer m_scratch;
        const double *m_d_value, *m_d_structure, *m_d_amplitudes;
        unsigned int m_cv_last_updated;
        bool m_have_computed;
    };

//! Probe volume (no reference counterpart; include/mtd_abi.h "Probe volume"): the smoothed number of particles in a box, slab, sphere or
//! cylinder fixed in space, s = sum_i a(type_i) h(min_image(r_i - c)) — the variable of the INDUS method.  A plain CollectiveVariable like
//! BraggIntensity: one device double for the integrator, the bias factor back on the device, computed once per time step, any split of
//! the particles over ranks (one allreduceSmall of two sums; ghosts are not counted).  Unlike every other variable here the bias forces do
//! NOT sum to zero (the region is an external object), and there is a virial: written per particle while the pressure flag is set, for
//! positions, box and centre strained together.  The centre is kept in fractional coordinates of the global box it was given in (at
//! construction or setRegion) and follows the box; widths, radius, sigma_s and r_c are lengths.  The region is checked against the box at
//! every step (the fit rule of the header): a box that has shrunk below it throws.
class ProbeVolume : public CollectiveVariable
    {
    public:
        //! shape: mtd_probe_shape; centre: Cartesian, in the current global box; half_widths: three numbers (box; +inf: unbounded) —
        //! a cylinder reads half_widths[axis] as its half-length; weights: one per particle type
        ProbeVolume(std::shared_ptr<SystemDefinition> sysdef, int shape, const std::vector<double> &centre, const std::vector<double> &half_widths,
                    double radius, int axis, double sigma_s, double r_c, const std::vector<double> &weights, const std::string &suffix = "");
        double getCurrentValue(unsigned int timestep) override;
        void enqueueCurrentValue(unsigned int timestep, mtd_metad *engine, unsigned int slot) override;
        void computeBiasForces(unsigned int timestep) override;
        std::vector<std::string> getProvidedLogQuantities() override
            {
            auto l = CollectiveVariable::getProvidedLogQuantities();
            l.push_back(m_cv_name);
            return l;
            }
        double getLogValue(const std::string &quantity, unsigned int timestep) override
            {
            if (quantity == m_cv_name) return getCurrentValue(timestep);
            return CollectiveVariable::getLogValue(quantity, timestep);
            }
        //! between runs (a probe volume is commonly moved or grown in stages); both throw and leave the variable as it was when refused
        void setRegion(int shape, const std::vector<double> &centre, const std::vector<double> &half_widths, double radius, int axis,
                       double sigma_s, double r_c);
        void setWeights(const std::vector<double> &weights);
        std::vector<double> getWeights() const { return std::vector<double>(m_par.coeff, m_par.coeff + m_par.n_types); }
        std::vector<double> getFractionalCentre() const { return std::vector<double>(m_par.centre, m_par.centre + 3); }
        double getCount(unsigned int timestep);                            //!< N_v: the weighted count inside the sharp region
        std::vector<double> getLocal(unsigned int timestep);               //!< h_i of every local particle, without the weight of its type

    private:
        void computeCV(unsigned int timestep);
        mtd_probe_call call(const mtd_box *box);
        double readOne(const double *const *d_src, const char *what, unsigned int timestep);
        mtd_probe_params m_par;
        DeviceBuffer m_scratch, m_local;
        const double *m_d_value, *m_d_count;
        unsigned int m_cv_last_updated;
        bool m_have_computed;
    };

//! AspectRatio.h / AspectRatio.cc:5-130 — box-shape CV, external virial only
class AspectRatio : public CollectiveVariable
    {
    public:
        AspectRatio(std::shared_ptr<SystemDefinition> sysdef, unsigned int dir1, unsigned int dir2);
        double getCurrentValue(unsigned int timestep) override;        // AspectRatio.cc:24-57
        void computeBiasForces(unsigned int timestep) override;        // AspectRatio.cc:59-130
        bool canComputeDerivatives() override { return false; }

    private:
        unsigned int m_dir1, m_dir2;
    };

//! Density.h / Density.cc:5-54 — N/V, external virial only (group = all particles here)
class Density : public CollectiveVariable
    {
    public:
        Density(std::shared_ptr<SystemDefinition> sysdef, const std::string &suffix);
        double getCurrentValue(unsigned int timestep) override;        // Density.cc:20-27
        void computeBiasForces(unsigned int timestep) override;        // Density.cc:29-54
        bool canComputeDerivatives() override { return false; }
    };

//! IntegratorMetaDynamics.h:66-383 (grid mode; the non-grid Gaussian resummation is unreachable from the
//! Python API, integrate.py:266-267 always calls setGrid(True))
class IntegratorMetaDynamics
    {
    public:
        enum Enum
            {
            mode_standard,
            mode_well_tempered
            };

        IntegratorMetaDynamics(std::shared_ptr<SystemDefinition> sysdef, double deltaT, double W, double T_shift, double T,
                               unsigned int stride, bool add_bias = true, const std::string &filename = "",
                               bool overwrite = false, const Enum mode = mode_standard);
        virtual ~IntegratorMetaDynamics();

        virtual void update(unsigned int timestep);                   // IntegratorMetaDynamics.cc:219-312
        virtual void prepRun(unsigned int timestep);                  // :121-217

        void registerCollectiveVariable(std::shared_ptr<CollectiveVariable> cv, double sigma, double cv_min = 0.0,
                                        double cv_max = 0.0, int num_points = 0);   // .h:117-134
        void removeAllVariables() { m_variables.clear(); }
        //! forces HOOMD's System would hand to computeNetForce (every ForceCompute, CVs included)
        void addForceCompute(std::shared_ptr<ForceCompute> f) { m_forces.push_back(f); }
        void removeForceComputes() { m_forces.clear(); }

        std::vector<std::string> getProvidedLogQuantities() { return m_log_names; }
        double getLogValue(const std::string &quantity, unsigned int timestep);     // .h:161-189

        void setGrid(bool use_grid);                                   // :778-815
        void setMode(Enum mode);
        void setStride(unsigned int stride);
        bool isInitialized() { return m_is_initialized; }
        void dumpGrid(const std::string &filename1, const std::string &filename2, unsigned int period);   // :817-829
        void restartFromGridFile(const std::string &filename) { m_restart_filename = filename; }
        void setAddHills(bool add_bias);
        void setAdaptive(bool adaptive) { m_adaptive = adaptive; }   // IntegratorMetaDynamics.h:248-251
        //! the inverse width matrix of the last deposit (row major n_cv x n_cv)
        std::vector<double> getSigmaInv() const { return m_sigma_inv; }
        //! hills deposited so far (m_num_gaussians, IntegratorMetaDynamics.cc:440)
        unsigned int getNumGaussians();
        void setSigmaG(double sigma_g) { m_sigma_g = sigma_g; }
        void setMultipleWalkers(bool multiple) { m_multiple_walkers = multiple; }
        void resetHistogram();                                         // :1195-1203

        //! this build's own knobs
        //! Steps of the stand-alone run loop as a HIP graph (System::run): the number of consecutive update() calls after which
        //! the sequence of launches repeats itself with the same arguments — lcm(2, stride): the mesh CV alternates between two
        //! sets of tile cursors, a deposit comes every `stride` steps — or 0 when the steps cannot be replayed from a capture:
        //! anything that reads a value back on the host or changes arguments from step to step (hills file, grid dumps, adaptive
        //! widths, umbrellas, walkers, a domain decomposition's exchange numbers, box CVs, the potential energy, wrapped computes),
        //! and pure lamellar sets, whose two-launch step measures SLOWER from a graph (profiles/r4/graph_ab.log).
        unsigned int graphPeriod() const;
        void setFusedPath(bool enable) { m_allow_fused = enable; }     // default on: two launches per step for lamellar CVs
        bool usedFusedPath() const { return std::strcmp(m_route.step, "fused") == 0; }
        //! What the most recent step did, written by the step's functions as they ran: "<step> sums=<sums> engine=<engine>" with
        //! step fused | generic; sums (the lamellar sums of a mixed set) - | launch_a | rider | rider_then_launch_a; engine (who
        //! enqueued the grid engine's launch) fused_step | lamellar_slots | mesh_merged | walkers | self | own.  Empty before the first step.
        std::string lastStepRoute() const;
        mtd_metad *getEngine() { return m_engine; }
        //! CV values and dV/ds_c of the most recent bias update (synchronises)
        std::vector<double> getCurrentValues();
        std::vector<double> getBiasFactors();

    private:
        struct CollectiveVariableItem                                  // IntegratorMetaDynamics.h:21-28
            {
            std::shared_ptr<CollectiveVariable> m_cv;
            double m_sigma, m_cv_min, m_cv_max;
            unsigned int m_num_points;
            // the variable's kind, cast once at registration: at most one is set, none for every other kind
            std::shared_ptr<LamellarOrderParameterGPU> m_lamellar;
            std::shared_ptr<OrderParameterMeshGPU> m_mesh;
            std::shared_ptr<SteinhardtQl> m_steinhardt;
            //! a lamellar variable that may take the launches lamellar variables share (an umbrella adds to a HOST bias factor)
            bool sharesLamellarLaunches() const { return m_lamellar && !m_lamellar->hasUmbrella(); }
            };
        //! What one step of the variable set does, decided once per step (planStep); the functions of the step only read it
        struct StepPlan
            {
            bool fused_lamellar = false;             //!< the pure lamellar step (stepFusedLamellar), else stepGeneric
            std::vector<unsigned int> lam_slots;     //!< the lamellar variables that share launches: all of a pure set, those of a mixed set
            std::shared_ptr<OrderParameterMeshGPU> mesh;   //!< the mesh variable if the set has exactly one, and its slot
            unsigned int mesh_slot = 0;
            bool mesh_rider = false;                 //!< that mesh may carry the lamellar sums in its assignment (armLamellarRider)
            bool mesh_engine = false;                //!< that mesh may carry the engine's launch in its force pass (forcesWithBiasUpdate)
            bool single = false;                     //!< one variable, which may update the engine itself (enqueueValueAndBias)
            bool walkers = false, adaptive = false;
            };

        void updateBiasPotential(unsigned int timestep);               // :314-588
        void computeNetForce(unsigned int timestep);
        void openOutputFile();                                         // :74-96
        void writeFileHeader();                                        // :98-119
        void setupGrid();                                              // :590-661 (device side: mtd_metad_create)
        void readGrid(const std::string &filename);                    // :928-1000
        void writeGrid(const std::string &filename, unsigned int timestep);   // :831-926
        StepPlan planStep() const;
        void stepFusedLamellar(const StepPlan &plan, unsigned int timestep);
        void stepGeneric(const StepPlan &plan, unsigned int timestep);
        const char *enqueueEngine(const StepPlan &plan, unsigned int timestep, bool self_updated);
        void buildLamellarSet(const std::vector<unsigned int> &slots);
        void setMixedLamellarSources(const std::vector<unsigned int> &slots, unsigned int n_partials);
        void mixedLamellarCvPass(const std::vector<unsigned int> &slots);

        std::shared_ptr<SystemDefinition> m_sysdef;
        std::shared_ptr<ParticleData> m_pdata;
        std::shared_ptr<ExecutionConfiguration> m_exec_conf;
        double m_deltaT, m_W, m_T_shift;
        unsigned int m_stride;
        std::vector<CollectiveVariableItem> m_variables;
        std::vector<std::shared_ptr<ForceCompute>> m_forces;
        std::vector<std::string> m_log_names;
        bool m_is_initialized;
        std::string m_filename;
        bool m_overwrite, m_is_appending;
        std::ofstream m_file;
        std::string m_delimiter;
        bool m_use_grid, m_add_bias;
        std::string m_restart_filename, m_grid_fname1, m_grid_fname2;
        unsigned int m_grid_period, m_cur_file;
        double m_sigma_g;
        bool m_adaptive;
        void computeSigma();                                           // :1205-1294
        std::vector<double> m_sigma_inv;
        DeviceBuffer m_sigma_scratch, m_sigma_exchange;
        double m_temp;
        Enum m_mode;
        bool m_multiple_walkers, m_warned_single_walker;

        mtd_metad *m_engine;
        bool m_allow_fused;
        struct { const char *step, *sums, *engine; } m_route = {"", "-", "-"};
        mtd_lamellar_set m_fused_set;
        DeviceBuffer m_fused_partials;
        std::vector<void *> m_fused_force_ptrs;
    };

//! the part of HOOMD's System the plugin relies on: the run loop calling Integrator::update once per step
class System
    {
    public:
        System(std::shared_ptr<SystemDefinition> sysdef, unsigned int initial_tstep) : m_sysdef(sysdef), m_cur_tstep(initial_tstep) {}
        void setIntegrator(std::shared_ptr<IntegratorMetaDynamics> integrator) { m_integrator = integrator; }
        std::shared_ptr<IntegratorMetaDynamics> getIntegrator() { return m_integrator; }
        ~System();
        void run(unsigned int nsteps);
        unsigned int getCurrentTimeStep() const { return m_cur_tstep; }
        //! this build: replay runs of at least four periods from a HIP graph where the integrator allows it
        //! (IntegratorMetaDynamics::graphPeriod).  OFF by default — measured slower than plain launches for every configuration of
        //! BASELINE.json (profiles/r4/graph_ab.log); MTD_GRAPH=1 or setGraphMode(1) switches it on
        void setGraphMode(int mode) { m_graph_mode = mode; }           // -1 default (environment), 0 off, 1 on
        //! steps of the last run() that were replayed from a graph (0: plain launches), and the period of the step sequence
        //! (a graph holds several periods, ~24 steps)
        unsigned int lastRunGraphSteps() const { return m_last_graph_steps; }
        unsigned int lastRunGraphPeriod() const { return m_last_graph_period; }

    private:
        unsigned int runGraph(unsigned int nsteps, unsigned int period);
        std::shared_ptr<SystemDefinition> m_sysdef;
        std::shared_ptr<IntegratorMetaDynamics> m_integrator;
        unsigned int m_cur_tstep;
        int m_graph_mode = -1;
        hipStream_t m_graph_stream = nullptr;
        unsigned int m_last_graph_steps = 0, m_last_graph_period = 0;
    };

} // namespace mtdhost
