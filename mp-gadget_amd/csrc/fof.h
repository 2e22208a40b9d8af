// fof.h -- friends-of-friends group finder (see fof.hip)
#pragma once
#include "mpg_common.h"
#include "tree_build.h"

namespace mpg {

struct FofInput {
    int64_t n = 0;                       // particles (caller order)
    const double *pos = nullptr;         // [n][3]
    const double *vel = nullptr;         // [n][3] or null
    const float *mass = nullptr;         // [n]
    const uint8_t *type = nullptr;       // [n] or null (all type 1)
    const uint8_t *flags = nullptr;      // bit 0 IsGarbage, bit 1 Swallowed; or null
    const unsigned long long *id = nullptr; // [n] P[].ID
    const double *hsml = nullptr;        // [n] or null: the search-radius hint of gas / stars / black holes (fof.c:1285-1289)
    double box = 0, LL = 0;              // FOFHaloComovingLinkingLength
    int minlen = 32;                     // FOFHaloMinLength
    int secondary_mask = 1 + 16 + 32;    // FOFSecondaryLinkTypes
};

// device arrays to receive the group table (any may be null); groups are in MinID order like fof.Group
struct FofTable {
    unsigned long long *MinID;
    int *Length, *GrNr, *LenType; // LenType[g][6]
    double *Mass, *MassType;      // MassType[g][6]
    double *CM, *Vel, *Jmom;      // [g][3]
    double *Imom;                 // [g][9]
    float *FirstPos;              // [g][3]
};

// the sub-grid half of add_particle_to_group (fof.c:647-676): device columns in particle order, any may be null (its terms are 0;
// without density no group gets a seed)
struct FofSubgridIn {
    const double *sfr, *metallicity; // SphP.Sfr; SphP / StarP.Metallicity
    const float *metals;             // [n][9] SphP / StarP.Metals
    const uint8_t *heiii;            // P.HeIIIionized
    const double *bh_mass, *bh_mdot; // BHP.Mass, BHP.Mdot
    const double *density, *delaytime;
    int WindDecouple;
};
constexpr int FOF_NSUB = 24; // Sfr, GasMetalMass, GasMetalElemMass[9], MassHeIonized, StellarMetalMass, StellarMetalElemMass[9], BH_Mass, BH_Mdot
struct FofSubgridTable { // device arrays of ngroups entries, any may be null
    double *Sfr, *GasMetalMass, *StellarMetalMass, *GasMetalElemMass, *StellarMetalElemMass, *MassHeIonized, *BH_Mass, *BH_Mdot, *MaxDens;
    long long *seed_index;
};
struct FofSeedPar { // fof.c:1356-1365 and blackhole.c:1039-1111
    double MinFoFMass, MinMStar, SeedMass, MaxSeedMass, SeedDynMass;
    double pl_norm, pl_p0, pl_inv; // the power law's pow(Max, 1 + x) - pow(Seed, 1 + x), pow(Seed, 1 + x), 1 / (1 + x)
    double atime;
    const double *rnd; // RandTable.Table
    uint64_t rndsize;
};
struct FofSeedCols { // blackhole_make_one's columns, particle order; null outputs are skipped
    const unsigned long long *id;
    const uint8_t *tb_hydro;
    const double *pos;
    const uint8_t *type_in; // the column the type test reads
    const float *mass_in;
    uint8_t *type;
    float *mass;
    double *bh_mass, *mseed, *mdot, *formationtime;
    unsigned long long *swallowid;
    double *bh_density;
    uint8_t *tb_dynfric;
    double *minpotpos, *dfaccel, *df_surroundingvel, *dragaccel, *df_surroundingrmsvel, *df_surroundingdensity;
    int *jumptominpot, *countprogs;
    double *mtrack, *kineticfdbkenergy, *vdisp;
};

struct FofEngine {
    int64_t ngroups = 0;
    // the particle count of the last run() (-1: none since the particles were bound, or the catalogue is a rank's part of a shared one);
    // whether subgrid() has run on it
    int64_t cat_n = -1;
    bool sub_done = false;
    DevBuf<double> s_sum;                  // [ngroups][FOF_NSUB]
    DevBuf<unsigned long long> s_maxbits;  // the bits of MaxDens (positive doubles order as their bits)
    DevBuf<long long> s_seed, seed_g;      // seed_index per group; the marked groups
    // the sub-grid sums, MaxDens and seed_index of the groups of the last run(); `in.n` particles as then
    void subgrid(int64_t n, const float *mass, const uint8_t *type, const FofSubgridIn &in, const FofSubgridTable &out, hipStream_t st);
    // fof_seed: marks the groups and lists them in group order; returns the length of the list.  With room (<= cap) the list is written to
    // d_group / d_particle (either may be null) and, with cols, the particles are converted; *nwarn = the reference's mass warnings.
    // *notgas: a listed row is no gas (blackhole.c:1057); nothing was converted then.
    int64_t seed(const FofSeedPar &par, const FofSeedCols *cols, int64_t cap, long long *d_particle, long long *d_group, int64_t *nwarn, bool *notgas,
                 hipStream_t st);
    // fof_set_escapefraction (fof.c:832-870): escfrac[i] = the Mass of row i's group for gas and stars (0 outside every group); other rows untouched
    void set_escapefraction(int64_t n, const uint8_t *type, double *escfrac, hipStream_t st);
    DevBuf<int> parent, root_of, val, list, sidx, ord_a, ord_b, g_grnr, g_lentype;
    DevBuf<unsigned long long> minid, label, slabel, run_label, g_minid, cnt;
    DevBuf<unsigned> run_count, run_start, g_len, g_start, lenkey_a, lenkey_b, err;
    DevBuf<uint8_t> keep;
    DevBuf<float> g_first;
    DevBuf<double> g_acc;
    DevBuf<long long> p_grnr;
    DevBuf<char> tmp;
    // the tree must hold the particles of the primary link types (force_tree_rebuild_mask); returns the number of groups
    int64_t run(TreeBuilder &tree, const FofInput &in, hipStream_t st);
    // the two halves of run(), used separately when groups span ranks (dist_fof.hip): labels of all in.n particles; then the catalogue
    // of the first n of them (also_keep: sorted labels whose runs are reported whatever their length; finish = false leaves raw sums)
    void compute_labels(TreeBuilder &tree, const FofInput &in, hipStream_t st);
    int64_t catalogue(const FofInput &in, int64_t n, const unsigned long long *also_keep, int64_t nalso, bool finish, hipStream_t st);
    static constexpr int NQ_ = 27; // doubles per group in g_acc (fof.hip NQ)
    void export_groups(const FofTable &out, hipStream_t st);
};

} // namespace mpg
