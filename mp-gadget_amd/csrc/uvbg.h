// uvbg.h -- excursion-set reionisation (see uvbg.hip): the meshes, plans and constants of calculate_uvbg (libgadget/uvbg.c, petapm.c:381-577)
#pragma once
#include "../../include/mpgadget_hip.h"
#include "mpg_common.h"
#include "pm.h"
#include <vector>

namespace mpg {

namespace uvbg {
// physconst.h
constexpr double SOLAR_MASS = 1.989e33;
constexpr double PLANCK = 6.6262e-27;
constexpr double PROTONMASS = 1.6726e-24;
constexpr double SEC_PER_YEAR = 3.155e7;
constexpr double HYDROGEN_MASSFRAC = 0.76;
constexpr float FLOAT_REL_TOL = (float)1e-5; // uvbg.c:30
constexpr int MAX_R_ITERATIONS = 10000;      // petapm.c:410
constexpr int MAX_DIM = 1290;                // the reference's int total_n_cells overflows above (uvbg.c:209)
constexpr int SUM_BLOCKS = 1024;             // most blocks of a pass over the cells: the order of the neutral-fraction sums follows from dim alone
} // namespace uvbg

// the constants of one reion_loop_pm call (uvbg.c:319-371), taken on the host in the reference's own fp64 operations
struct UvbgCellPar {
    double R, rtom, deltax_conv, pixel_volume, inv_eff, eff, J21c;
    double sfr_unit_m, sfr_unit_t; // UnitMass_in_g / SOLAR_MASS, UnitTime_in_s / SEC_PER_YEAR
    double sfr_time;               // ReionSFRTimescale * hubble_time
    int use_sfr;
};

struct UvbgEngine {
    int dim = 0, batch = 0; // of the meshes and plans held; dim of the last call (0: none)
    FftPlan plan_r2c, plan_c2r;
    DevBuf<double> dep;   // [3][dim^3] as deposited: mass, stars, SFR
    DevBuf<double> real;  // [batch][dim^3] the filtered grids of a radius
    DevBuf<double> unf;   // [batch][2 dim^2 (dim/2+1)] the unfiltered spectra, divided by dim^3
    DevBuf<double> filt;  // the same, filtered (the inverse transform's input, which it may overwrite)
    DevBuf<float> J21, xHI;
    DevBuf<double> partial; // [SUM_BLOCKS][3] then the 3 totals
    DevBuf<unsigned> err;
    // the deposit: rows sorted by base cell (keys, row indices; ping-pong), the first sorted row of every cell
    DevBuf<unsigned> key_a, key_b, idx_a, idx_b, cell_start;
    DevBuf<char> sort_tmp;
    void ensure(int dim, int batch);
    // petapm_reion_c2r's radii (petapm.c:426-499): depends on nothing the device computes
    static std::vector<double> radii(double Rmax, double Rmin, double Rdelta, double box, int dim);
    // uvbg.c:471-594 on device columns; returns false when an escape fraction came out negative
    bool run(int64_t n, const double *pos, const float *mass, const uint8_t *type, double box, const mpg_uvbg_params &par, const mpg_uvbg_columns &cols,
             const std::vector<double> &R, double xhi[2], hipStream_t st);
    void destroy()
    {
        plan_r2c.destroy();
        plan_c2r.destroy();
    }
    ~UvbgEngine() { destroy(); }
};

} // namespace mpg
