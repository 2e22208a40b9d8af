// fof_catalogue.hip -- the group catalogue fof_save_groups writes at every snapshot with SnapshotWithFOF (run.c:696-722, fof.c:1157-1163,
// fofpetaio.c), from device-resident columns on ONE rank: nothing but the blocks of the file crosses to the host.
//   k_cat_keys         fof_select_func (fofpetaio.c:33-36) + the IsGarbage test and the counts of petaio_build_selection (petaio.c:117-154)
//                      + the key of order_by_type_and_grnr (fofpetaio.c:202-218); NumPartInGroupTotal of fof_write_header (fofpetaio.c:432-436)
//   (rocPRIM radix)    the order itself: (key, index) pairs, stable, over the key bits in use
//   k_cat_gather       petaio_build_buffer with the getters of the particle blocks: SIMPLE_GETTER, GTPosition (petaio.c:744-753), GTVelocity
//                      (petaio.c:803-817), GTGroupID (petaio.c:887)
//   k_cat_group_block  mpsort by GrNr (fofpetaio.c:44-45) + build_buffer_fof with the getters of fofpetaio.c:464-536: one scatter, GrNr being
//                      a permutation of 1..ngroups (fof.c:1127-1134)
// and the writer on top (mpg_dev_fof_save_groups: fof_save_particles, fofpetaio.c:38-159, with fof_write_header, :419-461).
// DEFINED DIFFERENCE: rows of equal (type, GrNr) keep ascending particle index; the reference's qsort_openmp leaves their order unspecified.
// The two wrap loops of the position getters are the reference's repeated subtraction (not an fmod: the bits match), bounded at
// CAT_WRAP_TRIPS trips each; a value that needs more, or is not finite, fails the call with its row named.
// All three kernels stream: one thread per OUTPUT element, so a wave stores 64 consecutive elements (the gather) or whole rows (the
// scatter); no LDS, no atomics but the per-type counters (one per wave and type) and the error words.
#include "engine_internal.h"
#include "fof_catalogue.h"
#include <algorithm>
#include <rocprim/rocprim.hpp>

namespace mpg {

namespace {

constexpr unsigned long long NOROW = ~0ull;
// words of CatalogueEngine::cnt
constexpr int C_COUNT = 0, C_INGROUP = 6, C_ERR_WRAP = 12, C_ERR_INDEX = 13, C_WORDS = 14;

// key = type << gbits | GrNr for a selected row, 6 << gbits (behind every type) for the others
__global__ void __launch_bounds__(256) k_cat_keys(int64_t n, const long long *__restrict__ grnr, const uint8_t *__restrict__ type,
                                                  const uint8_t *__restrict__ flags, int gbits, unsigned long long *__restrict__ keys,
                                                  int *__restrict__ idx, unsigned long long *__restrict__ cnt)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int t = 7;
    bool ingroup = false, sel = false;
    if(i < n) {
        const long long g = grnr[i];
        t = type ? type[i] : 1;
        ingroup = g >= 0 && t < 6;                       // fof_write_header: no test of the flags; rows of the engine's type 7 are skipped
        sel = ingroup && !(flags && (flags[i] & 3));     // IsGarbage (petaio.c:130) and Swallowed (fofpetaio.c:35)
        unsigned long long key = 6ull << gbits;
        if(sel) {
            if((unsigned long long)g >> gbits)
                atomicMin(&cnt[C_ERR_WRAP], (unsigned long long)i);
            else
                key = ((unsigned long long)t << gbits) | (unsigned long long)g;
        }
        if(keys) {
            keys[i] = key;
            idx[i] = (int)i;
        }
    }
    for(int k = 0; k < 6; k++) { // (every lane of the wave arrives here)
        const unsigned long long mi = __builtin_amdgcn_ballot_w64(ingroup && t == k);
        const unsigned long long ms = __builtin_amdgcn_ballot_w64(sel && t == k);
        if((threadIdx.x & 63) == 0) {
            if(mi)
                atomicAdd(&cnt[C_INGROUP + k], (unsigned long long)__popcll(mi));
            if(ms)
                atomicAdd(&cnt[C_COUNT + k], (unsigned long long)__popcll(ms));
        }
    }
}

__device__ __forceinline__ double pick3(const double v[3], int k) { return k == 0 ? v[0] : (k == 1 ? v[1] : v[2]); }

// while(out > Box) out -= Box; while(out <= 0) out += Box; (petaio.c:750-751) in double, each loop bounded; false: the row is refused
__device__ __forceinline__ bool wrap_double(double &x, double box)
{
    bool ok = isfinite(x);
    int t = 0;
    while(x > box && t < CAT_WRAP_TRIPS) {
        x -= box;
        t++;
    }
    ok = ok && !(x > box);
    t = 0;
    while(x <= 0 && t < CAT_WRAP_TRIPS) {
        x += box;
        t++;
    }
    return ok && !(x <= 0);
}
// the same on a FLOAT `out` (GTFirstPos, fofpetaio.c:479-481): the comparisons promote it to double, every -= / += rounds back to float
__device__ __forceinline__ bool wrap_float(float &x, double box)
{
    bool ok = isfinite(x);
    int t = 0;
    while((double)x > box && t < CAT_WRAP_TRIPS) {
        x = (float)((double)x - box);
        t++;
    }
    ok = ok && !((double)x > box);
    t = 0;
    while((double)x <= 0 && t < CAT_WRAP_TRIPS) {
        x = (float)((double)x + box);
        t++;
    }
    return ok && !((double)x <= 0);
}

// out[j][k] = getter(src[perm[j]][k]); thread e = j nmemb + k
template <typename S, typename D, int CONV>
__global__ void __launch_bounds__(256) k_cat_gather(int64_t total, int nmemb, int64_t nrows, const int *__restrict__ perm, const S *__restrict__ src,
                                                    CatConvPar par, D *__restrict__ out, unsigned long long *__restrict__ cnt)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(e >= total)
        return;
    const int64_t j = nmemb == 1 ? e : e / nmemb;
    const int k = (int)(e - j * nmemb);
    const int64_t i = perm[j];
    if(i < 0 || i >= nrows) { // (an index outside the column: nothing is read)
        atomicMin(&cnt[C_ERR_INDEX], (unsigned long long)j);
        return;
    }
    const S v = src[i * nmemb + k];
    if(CONV == CAT_POSITION) {
        double x = (double)v - pick3(par.off, k);
        if(!wrap_double(x, par.box))
            atomicMin(&cnt[C_ERR_WRAP], (unsigned long long)j);
        out[e] = (D)x;
    }
    else if(CONV == CAT_VELOCITY)
        out[e] = (D)(par.fac * (double)v);
    else
        out[e] = (D)v;
}

struct CatGroupSrc {
    const double *acc, *sub; // [g][FofEngine::NQ_], [g][FOF_NSUB] or null (no sub-grid call on this catalogue: zeros)
    const int *lentype, *grnr;
    const unsigned long long *minid;
    const float *first;
};

// out[GrNr[g] - 1][k] = getter(Group[g])[k]; thread e = g nmemb + k.  Offsets in acc: Mass 0, MassType 1, CM 7, Vel 10, Jmom 13, Imom 16
// (fof.hip); in sub: Sfr 0, GasMetalMass 1, GasMetalElemMass 2, MassHeIonized 11, StellarMetalMass 12, StellarMetalElemMass 13, BH_Mass 22,
// BH_Mdot 23 (k_fof_subgrid_export)
__global__ void __launch_bounds__(256) k_cat_group_block(int64_t total, int nmemb, int field, CatGroupSrc s, CatConvPar par, void *__restrict__ out,
                                                         unsigned long long *__restrict__ cnt)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if(e >= total)
        return;
    const int64_t g = nmemb == 1 ? e : e / nmemb;
    const int k = (int)(e - g * nmemb);
    const int64_t r = (int64_t)s.grnr[g] - 1;
    if(r < 0 || r * nmemb >= total) { // (no permutation of 1..ngroups: nothing is written)
        atomicMin(&cnt[C_ERR_INDEX], (unsigned long long)g);
        return;
    }
    const int64_t o = r * nmemb + k;
    const double *a = s.acc + (size_t)g * FofEngine::NQ_;
    const double *b = s.sub ? s.sub + (size_t)g * FOF_NSUB : nullptr;
    int ia = -1, ib = -1; // the plain f4 casts: the member's place in acc or in sub
    switch(field) {
    case GF_GroupID:
        ((uint32_t *)out)[o] = (uint32_t)s.grnr[g];
        return;
    case GF_MinID:
        ((unsigned long long *)out)[o] = s.minid[g];
        return;
    case GF_LengthByType:
        ((uint32_t *)out)[o] = (uint32_t)s.lentype[6 * g + k];
        return;
    case GF_MassCenterPosition: {
        double x = a[7 + k] - pick3(par.off, k);
        if(!wrap_double(x, par.box))
            atomicMin(&cnt[C_ERR_WRAP], (unsigned long long)g);
        ((double *)out)[o] = x;
        return;
    }
    case GF_FirstPos: {
        float x = (float)((double)s.first[3 * g + k] - pick3(par.off, k));
        if(!wrap_float(x, par.box))
            atomicMin(&cnt[C_ERR_WRAP], (unsigned long long)g);
        ((float *)out)[o] = x;
        return;
    }
    case GF_MassCenterVelocity:
        ((float *)out)[o] = (float)(par.fac * a[10 + k]);
        return;
    case GF_Mass: ia = 0; break;
    case GF_MassByType: ia = 1 + k; break;
    case GF_Jmom: ia = 13 + k; break;
    case GF_Imom: ia = 16 + k; break;
    case GF_StarFormationRate: ib = 0; break;
    case GF_GasMetalMass: ib = 1; break;
    case GF_GasMetalElemMass: ib = 2 + k; break;
    case GF_MassHeIonized: ib = 11; break;
    case GF_StellarMetalMass: ib = 12; break;
    case GF_StellarMetalElemMass: ib = 13 + k; break;
    case GF_BlackholeMass: ib = 22; break;
    case GF_BlackholeAccretionRate: ib = 23; break;
    default: return;
    }
    ((float *)out)[o] = ia >= 0 ? (float)a[ia] : (b ? (float)b[ib] : 0.f);
}

template <typename S, typename D, int CONV>
void launch_gather(int64_t total, int nmemb, int64_t nrows, const int *perm, const void *src, const CatConvPar &par, void *out, unsigned long long *cnt,
                   hipStream_t st)
{
    hipLaunchKernelGGL((k_cat_gather<S, D, CONV>), dim3(nblk(total)), dim3(256), 0, st, total, nmemb, nrows, perm, (const S *)src, par, (D *)out, cnt);
}
template <typename S, int CONV, typename... A> void gather_dst(int dtype, A... a)
{
    switch(dtype) {
    case CAT_F8: return launch_gather<S, double, CONV>(a...);
    case CAT_F4: return launch_gather<S, float, CONV>(a...);
    case CAT_U1: return launch_gather<S, uint8_t, CONV>(a...);
    case CAT_U4: return launch_gather<S, uint32_t, CONV>(a...);
    case CAT_U8: return launch_gather<S, unsigned long long, CONV>(a...);
    case CAT_I4: return launch_gather<S, int32_t, CONV>(a...);
    }
    fail(__FILE__, __LINE__, "catalogue gather: unsupported block dtype");
}
template <typename... A> void gather_plain(int src_dtype, int dtype, A... a)
{
    switch(src_dtype) {
    case CAT_F8: return gather_dst<double, CAT_NONE>(dtype, a...);
    case CAT_F4: return gather_dst<float, CAT_NONE>(dtype, a...);
    case CAT_U1: return gather_dst<uint8_t, CAT_NONE>(dtype, a...);
    case CAT_U8: return gather_dst<unsigned long long, CAT_NONE>(dtype, a...);
    case CAT_I4: return gather_dst<int32_t, CAT_NONE>(dtype, a...);
    case CAT_I8: return gather_dst<long long, CAT_NONE>(dtype, a...);
    }
    fail(__FILE__, __LINE__, "catalogue gather: unsupported source dtype");
}

int bits_of(int64_t v)
{
    int b = 1;
    while(b < 32 && (v >> b))
        b++;
    return b;
}

} // namespace

const CatGroupBlock &cat_group_block(int field)
{
    static const CatGroupBlock table[GF_COUNT] = {
        {"GroupID", CAT_U4, 1, false},           {"Mass", CAT_F4, 1, false},
        {"MassCenterPosition", CAT_F8, 3, false}, {"FirstPos", CAT_F4, 3, false},
        {"MinID", CAT_U8, 1, false},             {"Imom", CAT_F4, 9, false},
        {"Jmom", CAT_F4, 3, false},              {"MassCenterVelocity", CAT_F4, 3, false},
        {"LengthByType", CAT_U4, 6, false},      {"MassByType", CAT_F4, 6, false},
        {"MassHeIonized", CAT_F4, 1, false},     {"StarFormationRate", CAT_F4, 1, false},
        {"GasMetalMass", CAT_F4, 1, true},       {"StellarMetalMass", CAT_F4, 1, true},
        {"GasMetalElemMass", CAT_F4, 9, true},   {"StellarMetalElemMass", CAT_F4, 9, true},
        {"BlackholeMass", CAT_F4, 1, false},     {"BlackholeAccretionRate", CAT_F4, 1, false},
    };
    MPG_CHECK(field >= 0 && field < GF_COUNT, "catalogue: no such group block");
    return table[field];
}

void CatalogueEngine::tic(hipStream_t st)
{
    for(hipEvent_t &e : ev)
        if(!e)
            MPG_HIP(hipEventCreate(&e));
    MPG_HIP(hipEventRecord(ev[0], st));
}

double CatalogueEngine::toc(hipStream_t st)
{
    MPG_HIP(hipEventRecord(ev[1], st));
    MPG_HIP(hipEventSynchronize(ev[1]));
    float ms = 0;
    MPG_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
    return ms;
}

void CatalogueEngine::pig_order(int64_t n, const long long *grnr, const uint8_t *type, const uint8_t *flags, int grnr_bits, bool sort, int *perm_out,
                                int64_t count[6], int64_t in_group[6], hipStream_t st)
{
    for(int k = 0; k < 6; k++)
        count[k] = in_group[k] = 0;
    last_ms[0] = 0;
    if(n <= 0)
        return;
    MPG_CHECK(n < ((int64_t)1 << 31), "catalogue order: more than 2^31 - 1 rows");
    const int gbits = grnr_bits < 1 ? 1 : (grnr_bits > 32 ? 32 : grnr_bits);
    cnt.reserve(C_WORDS);
    if(sort) {
        key_a.reserve((size_t)n + 1);
        key_b.reserve((size_t)n + 1);
        idx_a.reserve((size_t)n + 1);
    }
    tic(st);
    MPG_HIP(hipMemsetAsync(cnt.p, 0, C_ERR_WRAP * sizeof(unsigned long long), st));
    MPG_HIP(hipMemsetAsync(cnt.p + C_ERR_WRAP, 0xff, 2 * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(k_cat_keys, dim3(nblk(n)), dim3(256), 0, st, n, grnr, type, flags, gbits, sort ? key_a.p : nullptr, sort ? idx_a.p : nullptr, cnt.p);
    MPG_HIP(hipGetLastError());
    if(sort) { // stable, over the bits in use: GrNr and the three bits of the type (6 = not selected, behind everything)
        size_t b = 0;
        MPG_HIP(rocprim::radix_sort_pairs(nullptr, b, key_a.p, key_b.p, idx_a.p, perm_out, (size_t)n, 0, gbits + 3, st));
        tmp.reserve(b + 16);
        MPG_HIP(rocprim::radix_sort_pairs((void *)tmp.p, b, key_a.p, key_b.p, idx_a.p, perm_out, (size_t)n, 0, gbits + 3, st));
    }
    unsigned long long h[C_WORDS];
    MPG_HIP(hipMemcpyAsync(h, cnt.p, sizeof(h), hipMemcpyDeviceToHost, st));
    last_ms[0] = toc(st);
    MPG_HIP(hipStreamSynchronize(st));
    MPG_CHECK(h[C_ERR_WRAP] == NOROW, "catalogue order: GrNr of row " + std::to_string(h[C_ERR_WRAP]) + " does not fit " + std::to_string(gbits) + " bits");
    for(int k = 0; k < 6; k++) {
        count[k] = (int64_t)h[C_COUNT + k];
        in_group[k] = (int64_t)h[C_INGROUP + k];
    }
}

static void reset_errors(CatalogueEngine &c, hipStream_t st)
{
    c.cnt.reserve(C_WORDS);
    MPG_HIP(hipMemsetAsync(c.cnt.p + C_ERR_WRAP, 0xff, 2 * sizeof(unsigned long long), st));
}
// -1, or the first refused row with *bad_index telling why (synchronises the stream)
static int64_t read_errors(CatalogueEngine &c, bool *bad_index, hipStream_t st)
{
    unsigned long long h[2];
    MPG_HIP(hipMemcpyAsync(h, c.cnt.p + C_ERR_WRAP, sizeof(h), hipMemcpyDeviceToHost, st));
    MPG_HIP(hipStreamSynchronize(st));
    *bad_index = h[1] != NOROW;
    if(h[1] != NOROW)
        return (int64_t)h[1];
    return h[0] == NOROW ? -1 : (int64_t)h[0];
}

int64_t CatalogueEngine::gather(const int *perm_in, int64_t count, int64_t nrows, const void *src, int src_dtype, int nmemb, int dtype, int conv,
                                const CatConvPar &par, void *out, bool *bad_index, hipStream_t st)
{
    *bad_index = false;
    if(count <= 0)
        return -1;
    const int64_t total = count * nmemb;
    reset_errors(*this, st);
    tic(st);
    if(conv == CAT_POSITION) { // (f64 -> f8 only: GTPosition works in double)
        MPG_CHECK(src_dtype == CAT_F8 && dtype == CAT_F8 && nmemb == 3, "catalogue gather: POSITION is a [3] f64 column into an f8 block");
        launch_gather<double, double, CAT_POSITION>(total, nmemb, nrows, perm_in, src, par, out, cnt.p, st);
    }
    else if(conv == CAT_VELOCITY) {
        MPG_CHECK((src_dtype == CAT_F8 || src_dtype == CAT_F4) && dtype == CAT_F4, "catalogue gather: VELOCITY is an f64 or f32 column into an f4 block");
        if(src_dtype == CAT_F8)
            launch_gather<double, float, CAT_VELOCITY>(total, nmemb, nrows, perm_in, src, par, out, cnt.p, st);
        else
            launch_gather<float, float, CAT_VELOCITY>(total, nmemb, nrows, perm_in, src, par, out, cnt.p, st);
    }
    else
        gather_plain(src_dtype, dtype, total, nmemb, nrows, perm_in, src, par, out, cnt.p, st);
    MPG_HIP(hipGetLastError());
    last_ms[1] += toc(st);
    return read_errors(*this, bad_index, st);
}

int64_t CatalogueEngine::group_block(const FofEngine &fof, int field, const CatConvPar &par, void *out, hipStream_t st)
{
    const CatGroupBlock &b = cat_group_block(field);
    const int64_t ng = fof.ngroups;
    if(ng <= 0)
        return -1;
    const CatGroupSrc s{fof.g_acc.p, fof.sub_done ? fof.s_sum.p : nullptr, fof.g_lentype.p, fof.g_grnr.p, fof.g_minid.p, fof.g_first.p};
    reset_errors(*this, st);
    tic(st);
    hipLaunchKernelGGL(k_cat_group_block, dim3(nblk(ng * b.nmemb)), dim3(256), 0, st, ng * b.nmemb, b.nmemb, field, s, par, out, cnt.p);
    MPG_HIP(hipGetLastError());
    last_ms[2] += toc(st);
    bool bad_index;
    return read_errors(*this, &bad_index, st);
}

} // namespace mpg

// ---- C-ABI (include/mpgadget_hip.h) ----------------------------------------------------------------------------------------------------------
static_assert(MPG_DT_F8 == CAT_F8 && MPG_DT_F4 == CAT_F4 && MPG_DT_U1 == CAT_U1 && MPG_DT_U4 == CAT_U4 && MPG_DT_U8 == CAT_U8 && MPG_DT_I4 == CAT_I4 &&
                  MPG_DT_I8 == CAT_I8,
              "mpg dtype codes");
static_assert(MPG_CONV_NONE == CAT_NONE && MPG_CONV_POSITION == CAT_POSITION && MPG_CONV_VELOCITY == CAT_VELOCITY && MPG_CONV_GROUPID == CAT_GROUPID,
              "mpg conversion codes");

namespace {

std::string block_name(const mpg_catalogue_block *b)
{
    return "block " + std::to_string(b->ptype) + "/" + (b->name ? b->name : "(null)");
}

// the descriptor alone (no device work): shapes, types and the pairs a conversion takes
void check_block(const char *who, const mpg_catalogue_block *b)
{
    const std::string w = std::string(who) + ": ";
    MPG_CHECK(b->name && *b->name && !strpbrk(b->name, " \t\n/"), w + "a block without a usable name");
    MPG_CHECK(b->ptype >= 0 && b->ptype < 6, w + block_name(b) + ": ptype is 0..5");
    MPG_CHECK(b->nmemb >= 1 && b->nmemb <= 64, w + block_name(b) + ": nmemb is 1..64");
    MPG_CHECK(b->conv >= 0 && b->conv < CAT_NCONV, w + block_name(b) + ": unknown conversion");
    const int s = b->src_dtype, d = b->dtype;
    MPG_CHECK(s == CAT_F8 || s == CAT_F4 || s == CAT_U1 || s == CAT_U8 || s == CAT_I4 || s == CAT_I8, w + block_name(b) + ": source dtype is f8, f4, u1, u8, i4 or i8");
    MPG_CHECK(d == CAT_F8 || d == CAT_F4 || d == CAT_U1 || d == CAT_U4 || d == CAT_U8 || d == CAT_I4, w + block_name(b) + ": block dtype is f8, f4, u1, u4, u8 or i4");
    if(b->conv == CAT_POSITION)
        MPG_CHECK(s == CAT_F8 && d == CAT_F8 && b->nmemb == 3, w + block_name(b) + ": POSITION is a [3] f64 column into an f8 block");
    if(b->conv == CAT_VELOCITY)
        MPG_CHECK((s == CAT_F8 || s == CAT_F4) && d == CAT_F4, w + block_name(b) + ": VELOCITY is an f64 or f32 column into an f4 block");
    if(b->conv == CAT_GROUPID)
        MPG_CHECK(s == CAT_I8 && d == CAT_U4 && b->nmemb == 1, w + block_name(b) + ": GROUPID is the int64 GrNr column into a u4 block");
    else
        MPG_CHECK(b->d_data, w + block_name(b) + ": no column");
}

CatConvPar conv_par(const mpg_engine *eng, const mpg_fof_catalogue_params *par)
{
    CatConvPar c;
    for(int d = 0; d < 3; d++)
        c.off[d] = par->CurrentParticleOffset[d];
    c.box = eng->box;
    c.fac = par->UsePeculiarVelocity ? 1.0 / par->atime : 1.0; // petaio.c:807-811
    return c;
}

// the errors of mpg_dev_fof_subgrid
void need_catalogue(const mpg_engine *eng, const char *who)
{
    const std::string w = std::string(who) + ": ";
    MPG_CHECK(eng->fof.cat_n >= 0, w + "no mpg_dev_fof_fof since the particles were bound");
    MPG_CHECK(eng->fof.cat_n == eng->n, w + "the bound particle count differs from that of the last mpg_dev_fof_fof");
}

std::string refusal(const char *who, const mpg_catalogue_block *b, int64_t row, bool bad_index, double box)
{
    char buf[256];
    if(bad_index)
        snprintf(buf, sizeof(buf), ": row %lld of the order names a particle outside the bound ones; nothing of the block was written", (long long)row);
    else
        snprintf(buf, sizeof(buf), ": row %lld is not finite or lies more than %d boxes (BoxSize %g) outside; nothing of the block was written",
                 (long long)row, CAT_WRAP_TRIPS, box);
    return std::string(who) + ": " + block_name(b) + buf;
}

} // namespace

int mpg_dev_fof_pig_order(mpg_engine *eng, const int64_t *d_grnr, const unsigned char *d_flags, int *d_perm, int64_t count[6], int64_t in_group[6])
{
    API_BEGIN
    MPG_CHECK(eng && count && in_group && (d_perm || eng->n == 0), "fof_pig_order: null argument");
    MPG_CHECK(eng->d_pos || eng->n == 0, "fof_pig_order: no particles bound (mpg_dev_bind_particles)");
    int bits = 32;
    const long long *grnr = (const long long *)d_grnr;
    if(!grnr) {
        need_catalogue(eng, "fof_pig_order");
        grnr = eng->fof.p_grnr.p;
        bits = bits_of(eng->fof.ngroups);
    }
    MPG_HIP(hipSetDevice(eng->device));
    eng->cat.pig_order(eng->n, grnr, eng->d_type, d_flags, bits, true, d_perm, count, in_group, eng->stream);
    API_END
}

int mpg_dev_gather_block(mpg_engine *eng, const int *d_perm, int64_t count, const mpg_catalogue_block *block, const mpg_fof_catalogue_params *params,
                         void *d_out)
{
    API_BEGIN
    MPG_CHECK(eng && block && params && count >= 0 && (count == 0 || (d_perm && d_out)), "gather_block: bad argument");
    check_block("gather_block", block);
    MPG_CHECK(eng->d_pos || eng->n == 0, "gather_block: no particles bound (mpg_dev_bind_particles)");
    MPG_CHECK(block->conv != CAT_POSITION || eng->box > 0, "gather_block: POSITION needs the BoxSize of the bound particles");
    MPG_CHECK(block->conv != CAT_VELOCITY || !params->UsePeculiarVelocity || params->atime > 0, "gather_block: atime must be positive");
    const void *src = block->d_data;
    if(block->conv == CAT_GROUPID && !src) {
        need_catalogue(eng, "gather_block");
        src = eng->fof.p_grnr.p;
    }
    MPG_HIP(hipSetDevice(eng->device));
    CatalogueEngine &c = eng->cat;
    c.last_ms[1] = 0;
    if(count > 0) {
        const CatConvPar cp = conv_par(eng, params);
        const bool can_fail = block->conv == CAT_POSITION; // (a refused block leaves d_out untouched: such a block passes through the stage)
        const size_t bytes = (size_t)count * block->nmemb * cat_itemsize(block->dtype);
        void *out = d_out;
        if(can_fail) {
            c.stage.reserve(bytes);
            out = c.stage.p;
        }
        bool bad_index = false;
        const int64_t row = c.gather(d_perm, count, eng->n, src, block->src_dtype, block->nmemb, block->dtype, block->conv == CAT_GROUPID ? CAT_NONE : block->conv,
                                     cp, out, &bad_index, eng->stream);
        // (an index outside the column skips its element: a direct gather has by then written the others)
        MPG_CHECK(row < 0, refusal("gather_block", block, row, bad_index, cp.box));
        if(can_fail) {
            MPG_HIP(hipMemcpyAsync(d_out, c.stage.p, bytes, hipMemcpyDeviceToDevice, eng->stream));
            MPG_HIP(hipStreamSynchronize(eng->stream));
        }
    }
    API_END
}

int mpg_dev_fof_save_groups(mpg_engine *eng, const char *path, const mpg_fof_catalogue_params *par, const mpg_catalogue_block *blocks, int nblocks,
                            const unsigned char *d_flags)
{
    API_BEGIN
    // ---- everything that can be refused without device work or a file ----
    MPG_CHECK(eng && path && *path && par && nblocks >= 0 && (blocks || nblocks == 0), "fof_save_groups: bad argument");
    need_catalogue(eng, "fof_save_groups");
    MPG_CHECK(par->nfile >= 1, "fof_save_groups: nfile must be at least 1");
    MPG_CHECK(par->atime > 0 && par->hubble > 0, "fof_save_groups: atime and hubble must be positive");
    MPG_CHECK(eng->box > 0, "fof_save_groups: the bound particles have no BoxSize");
    const int nb = par->SaveParticles ? nblocks : 0;
    for(int b = 0; b < nb; b++) {
        check_block("fof_save_groups", &blocks[b]);
        for(int a = 0; a < b; a++)
            MPG_CHECK(blocks[a].ptype != blocks[b].ptype || strcmp(blocks[a].name, blocks[b].name) != 0, "fof_save_groups: " + block_name(&blocks[b]) + " is listed twice");
    }
    MPG_HIP(hipSetDevice(eng->device));
    CatalogueEngine &c = eng->cat;
    FofEngine &fof = eng->fof;
    const int64_t n = eng->n, ng = fof.ngroups;
    const CatConvPar cp = conv_par(eng, par);
    c.last_ms[0] = c.last_ms[1] = c.last_ms[2] = 0;
    // ---- the order and the counts (fofpetaio.c:120-124, :432-436) ----
    int64_t count[6], in_group[6], offset[6] = {0, 0, 0, 0, 0, 0};
    if(nb > 0)
        c.perm.reserve((size_t)n + 1);
    c.pig_order(n, fof.p_grnr.p, eng->d_type, d_flags, bits_of(ng), nb > 0, c.perm.p, count, in_group, eng->stream);
    for(int t = 1; t < 6; t++)
        offset[t] = offset[t - 1] + count[t - 1];
    // ---- ONE device buffer and ONE pinned buffer for every block ----
    size_t bytes = 0;
    for(int f = 0; f < GF_COUNT; f++) {
        const CatGroupBlock &g = cat_group_block(f);
        bytes = std::max(bytes, (size_t)ng * g.nmemb * cat_itemsize(g.dtype));
    }
    for(int b = 0; b < nb; b++)
        bytes = std::max(bytes, (size_t)count[blocks[b].ptype] * blocks[b].nmemb * cat_itemsize(blocks[b].dtype));
    c.stage.reserve(bytes + 16);
    c.h_stage.reserve(bytes + 16);
    auto download = [&](size_t nbytes) {
        if(nbytes > 0)
            MPG_HIP(hipMemcpyAsync(c.h_stage.p, c.stage.p, nbytes, hipMemcpyDeviceToHost, eng->stream));
        MPG_HIP(hipStreamSynchronize(eng->stream));
    };
    // ---- writing starts: Header (fof_write_header, fofpetaio.c:419-461) ----
    {
        uint64_t npart[6], totng = (uint64_t)ng;
        for(int t = 0; t < 6; t++)
            npart[t] = (uint64_t)in_group[t];
        double RSD = 1.0 / (par->atime * par->hubble);
        const int pecvel = par->UsePeculiarVelocity ? 1 : 0;
        if(!pecvel)
            RSD /= par->atime;
        const double box = eng->box;
        bigfile_set_attr(path, "Header", "NumPartInGroupTotal", "u8", npart, 6);
        bigfile_set_attr(path, "Header", "NumFOFGroupsTotal", "u8", &totng, 1);
        bigfile_set_attr(path, "Header", "RSDFactor", "f8", &RSD, 1);
        bigfile_set_attr(path, "Header", "MassTable", "f8", par->MassTable, 6);
        bigfile_set_attr(path, "Header", "Time", "f8", &par->atime, 1);
        bigfile_set_attr(path, "Header", "BoxSize", "f8", &box, 1);
        bigfile_set_attr(path, "Header", "OmegaLambda", "f8", &par->OmegaLambda, 1);
        bigfile_set_attr(path, "Header", "Omega0", "f8", &par->Omega0, 1);
        bigfile_set_attr(path, "Header", "HubbleParam", "f8", &par->HubbleParam, 1);
        bigfile_set_attr(path, "Header", "CMBTemperature", "f8", &par->CMBTemperature, 1);
        bigfile_set_attr(path, "Header", "OmegaBaryon", "f8", &par->OmegaBaryon, 1);
        bigfile_set_attr(path, "Header", "UsePeculiarVelocity", "i4", &pecvel, 1);
    }
    // ---- FOFGroups/* in GrNr order (fofpetaio.c:58-71) ----
    for(int f = 0; f < GF_COUNT; f++) {
        const CatGroupBlock &g = cat_group_block(f);
        if(g.metal && !par->MetalReturnOn)
            continue;
        const std::string name = std::string("FOFGroups/") + g.name;
        const int64_t bad = c.group_block(fof, f, cp, c.stage.p, eng->stream);
        MPG_CHECK(bad < 0, "fof_save_groups: block " + name + ": group " + std::to_string(bad) +
                               " (MinID order) has no GrNr of 1..ngroups, or its position is not finite or more than 64 boxes outside; nothing of the block was written");
        download((size_t)ng * g.nmemb * cat_itemsize(g.dtype));
        bigfile_write_block(path, name.c_str(), cat_dtype_name(g.dtype), g.nmemb, ng > 0 ? par->nfile : 0, ng, cat_dtype_name(g.dtype), c.h_stage.p);
    }
    // ---- <ptype>/<name>, count[ptype] rows each (fofpetaio.c:128-142); an empty block is created with NFILE: 0 (petaio.c:673-676) ----
    for(int b = 0; b < nb; b++) {
        const mpg_catalogue_block &B = blocks[b];
        const int64_t rows = count[B.ptype];
        const void *src = B.conv == CAT_GROUPID && !B.d_data ? (const void *)fof.p_grnr.p : B.d_data;
        bool bad_index = false;
        const int64_t row = c.gather(c.perm.p + offset[B.ptype], rows, n, src, B.src_dtype, B.nmemb, B.dtype, B.conv == CAT_GROUPID ? CAT_NONE : B.conv, cp,
                                     c.stage.p, &bad_index, eng->stream);
        MPG_CHECK(row < 0, refusal("fof_save_groups", &B, row, bad_index, cp.box));
        download((size_t)rows * B.nmemb * cat_itemsize(B.dtype));
        const std::string name = std::to_string(B.ptype) + "/" + B.name;
        bigfile_write_block(path, name.c_str(), cat_dtype_name(B.dtype), B.nmemb, rows > 0 ? par->nfile : 0, rows, cat_dtype_name(B.dtype), c.h_stage.p);
    }
    API_END
}

int mpg_fof_catalogue_get_times(mpg_engine *eng, double ms[3])
{
    API_BEGIN
    MPG_CHECK(eng && ms, "null argument");
    for(int k = 0; k < 3; k++)
        ms[k] = eng->cat.last_ms[k];
    API_END
}
