// fof_catalogue.h -- the group catalogue of fof_save_groups on the device (see fof_catalogue.hip): the particle-in-group order, the block
// gather with the reference's getters, the group-table blocks in GrNr order
//
// THE ONE DEFINED DIFFERENCE: rows of equal (type, GrNr) keep ASCENDING PARTICLE INDEX (a stable radix sort of (key, index) pairs); the
// reference's qsort_openmp with order_by_type_and_grnr (fofpetaio.c:202-218, :389) leaves the order of equal keys unspecified.
#pragma once
#include "fof.h"
#include "host_table.h"
#include "mpg_common.h"

namespace mpg {

// element types of a source column / of a block in the file (the values of MPG_DT_* in include/mpgadget_hip.h)
enum CatDtype { CAT_F8 = 0, CAT_F4 = 1, CAT_U1 = 2, CAT_U4 = 3, CAT_U8 = 4, CAT_I4 = 5, CAT_I8 = 6, CAT_NDTYPE = 7 };
// the getter (MPG_CONV_*): SIMPLE_GETTER, GTPosition (petaio.c:744-753), GTVelocity (petaio.c:803-817), GTGroupID (petaio.c:887)
enum CatConv { CAT_NONE = 0, CAT_POSITION = 1, CAT_VELOCITY = 2, CAT_GROUPID = 3, CAT_NCONV = 4 };
constexpr int CAT_WRAP_TRIPS = 64; // the bound of each of the two wrap loops; a row that needs more is an error, never a longer loop

inline int cat_itemsize(int dt)
{
    static const int size[CAT_NDTYPE] = {8, 4, 1, 4, 8, 4, 8};
    return dt >= 0 && dt < CAT_NDTYPE ? size[dt] : 0;
}
inline const char *cat_dtype_name(int dt)
{
    static const char *name[CAT_NDTYPE] = {"f8", "f4", "u1", "u4", "u8", "i4", "i8"};
    return dt >= 0 && dt < CAT_NDTYPE ? name[dt] : "?";
}

struct CatConvPar {
    double off[3]; // CurrentParticleOffset
    double box;    // PartManager->BoxSize
    double fac;    // 1 / atime with UsePeculiarVelocity, else 1
};

// the members of struct Group the FOFGroups/* blocks hold (fofpetaio.c:464-536), in the order of fof_register_io_blocks (fofpetaio.c:538-568)
enum CatGroupField {
    GF_GroupID, GF_Mass, GF_MassCenterPosition, GF_FirstPos, GF_MinID, GF_Imom, GF_Jmom, GF_MassCenterVelocity, GF_LengthByType, GF_MassByType,
    GF_MassHeIonized, GF_StarFormationRate, GF_GasMetalMass, GF_StellarMetalMass, GF_GasMetalElemMass, GF_StellarMetalElemMass, GF_BlackholeMass,
    GF_BlackholeAccretionRate, GF_COUNT
};
struct CatGroupBlock {
    const char *name;
    int dtype, nmemb;
    bool metal; // registered only with MetalReturnOn
};
const CatGroupBlock &cat_group_block(int field);

struct CatalogueEngine {
    DevBuf<unsigned long long> key_a, key_b, cnt; // (type, GrNr) keys; cnt: count[6], in_group[6], the error word
    DevBuf<int> idx_a, perm;
    DevBuf<char> tmp, stage; // rocPRIM's scratch; the ONE device buffer every block is gathered into
    HostBuf<char> h_stage;   // ... and the ONE pinned buffer it is copied to
    hipEvent_t ev[2] = {};
    double last_ms[3] = {0, 0, 0}; // the order; the sum of the gathers; the group blocks (device times of the last call of each)
    ~CatalogueEngine()
    {
        for(hipEvent_t e : ev)
            if(e)
                (void)hipEventDestroy(e);
    }
    void tic(hipStream_t st);
    double toc(hipStream_t st); // ms since tic (synchronises the stream)

    // fof_select_func + petaio_build_selection + order_by_type_and_grnr: perm[n] (the first sum(count) entries are the order), count[6] the
    // selected rows per type, in_group[6] the rows with GrNr >= 0 per type whatever their flags.  grnr_bits: the bits of the largest GrNr
    // (32: unknown).  sort = false: the counts only.  Throws when a selected row's GrNr does not fit grnr_bits.
    void pig_order(int64_t n, const long long *grnr, const uint8_t *type, const uint8_t *flags, int grnr_bits, bool sort, int *perm_out,
                   int64_t count[6], int64_t in_group[6], hipStream_t st);
    // out[j][k] = getter(src[perm[j]][k]) for j < count, src a column of nrows rows.  Returns -1, or the first row j that is refused:
    // *bad_index tells whether perm[j] lies outside the column (nothing is read there) or the POSITION wrap gave up.  `out` (device) is
    // scratch after a refusal.  Adds its device time to last_ms[1].
    int64_t gather(const int *perm, int64_t count, int64_t nrows, const void *src, int src_dtype, int nmemb, int dtype, int conv, const CatConvPar &par,
                   void *out, bool *bad_index, hipStream_t st);
    // out[GrNr[g] - 1] = getter(Group[g]) of the engine's table (sub-grid members: zeros unless fof.sub_done); returns the first group
    // (MinID order) that is refused - a wrap that gave up, a GrNr outside 1..ngroups - or -1.  Adds its device time to last_ms[2].
    int64_t group_block(const FofEngine &fof, int field, const CatConvPar &par, void *out, hipStream_t st);
};

} // namespace mpg
