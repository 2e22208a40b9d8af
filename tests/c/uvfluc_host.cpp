// The HOST build of the UV-fluctuation table's read and of the local background (cool::uvf_zreion and cool::local_setup of csrc/cooling.h,
// which the kernels of csrc/cooling.hip and csrc/sfr.hip run) as a stand-alone program: reads one file of float64 values
// (tests/test_uvfluc_restated.py writes it), writes per point zreion and the nine members of the local struct UVBG.  No GPU call is made.
#include "../../mp-gadget_amd/csrc/cooling.h"
#include <cstdio>
#include <vector>

using namespace mpg;
using namespace mpg::cool;

int main(int argc, char **argv)
{
    if(argc != 3)
        return 2;
    FILE *f = fopen(argv[1], "rb");
    if(!f)
        return 3;
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<double> in(bytes / sizeof(double));
    if(fread(in.data(), sizeof(double), in.size(), f) != in.size())
        return 4;
    fclose(f);
    size_t k = 0;
    auto next = [&]() { return in.at(k++); };
    const int64_t n = (int64_t)next();
    UvfView U;
    U.nside = (long long)next();
    const double box = next();
    U.step = (box - 0) / (U.nside - 1);
    for(int d = 0; d < 3; d++)
        U.off[d] = next();
    Setup S{};
    S.redshift = next();
    double *uv = &S.uvbg.J_UV;
    for(int j = 0; j < 9; j++)
        uv[j] = next();
    // the table in an allocation of exactly its size, so that a build with a sanitizer sees any read outside it
    std::vector<double> table((size_t)U.nside * U.nside * U.nside);
    for(double &t : table)
        t = next();
    U.table = table.data();
    std::vector<double> out;
    for(int64_t i = 0; i < n; i++) {
        const double x[3] = {next(), next(), next()};
        const double z = uvf_zreion(U, x);
        const Setup L = local_setup(S, z);
        out.push_back(z);
        const double *lu = &L.uvbg.J_UV;
        out.insert(out.end(), lu, lu + 9);
    }
    f = fopen(argv[2], "wb");
    if(!f || fwrite(out.data(), sizeof(double), out.size(), f) != out.size())
        return 5;
    fclose(f);
    return 0;
}
