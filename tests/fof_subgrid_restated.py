"""numpy restatement of the sub-grid half of the group catalogue and of black-hole seeding, written from the cited lines:
add_particle_to_group (libgadget/fof.c:631-676, the members of struct Group of fof.h:42-59), winds_is_particle_decoupled (winds.c:114-120),
the marks of fof_seed (fof.c:1356-1365), bh_powerlaw_seed_mass and blackhole_make_one (blackhole.c:1039-1111).

It works on a GIVEN membership - group[i] = the index of particle i's group in MinID order, -1 for none - and holds no FOF of its own.

Two modes of the sums:
  "ld"   every sum in np.longdouble over exact terms; MaxDens / seed_index by the engine's defined rule (largest density, ties to the
         smaller particle index).
  "ref"  the reference's own order and types: the members of a group one after the other (in particle order: one of the orders its
         qsort on MinID alone may leave), sequential sums in fp64, in float32 for GasMetalElemMass, StellarMetalElemMass and MassHeIonized
         (fof.h:48-52, with the float product Metals[j] * Mass), and the FIRST strict maximum of the density (:671).
IDs are unsigned 64-bit: ID + 23 wraps (Python integers masked to 64 bits).  The random table is data: get_random_number(id) = table[id % size].
Not a test module: imported by test_fof_subgrid_restated.py (runs anywhere) and test_gpu_fof_subgrid.py (the HIP path)."""
import numpy as np

NMETALS = 9
M64 = (1 << 64) - 1
SUMS = ("Sfr", "GasMetalMass", "GasMetalElemMass", "MassHeIonized", "StellarMetalMass", "StellarMetalElemMass", "BH_Mass", "BH_Mdot")
FLOAT_MEMBERS = ("GasMetalElemMass", "StellarMetalElemMass", "MassHeIonized")                       # fof.h:48-52
COLUMNS = ("sfr", "metallicity", "metals", "heiii_ionized", "bh_mass", "bh_mdot", "density", "delaytime")


class SeedError(RuntimeError):
    """endrun(7772): only gas turns into black holes (blackhole.c:1057-1058)"""


def group_index(grnr, group_grnr):
    """group[i] in MinID order from P[].GrNr (numbers from 1 by length, -1: none) and the table's GrNr column"""
    inv = np.full(len(group_grnr) + 1, -1, np.int64)
    inv[np.asarray(group_grnr, np.int64)] = np.arange(len(group_grnr))
    grnr = np.asarray(grnr, np.int64)
    return np.where(grnr > 0, inv[np.maximum(grnr, 0)], -1)


def _col(P, k, n):
    """a column of the particle table; one that is absent or None reads as zeros (the engine's NULL)"""
    a = P.get(k)
    if a is not None:
        return np.asarray(a)
    return np.zeros((n, NMETALS), np.float32) if k == "metals" else np.zeros(n, np.uint8 if k == "heiii_ionized" else np.float64)


def decoupled(P, i, wind_decouple):
    """winds_is_particle_decoupled, winds.c:114-120 (for a gas row)"""
    return bool(wind_decouple) and P.get("delaytime") is not None and P["delaytime"][i] > 0


def group_sums(group, ngroups, mass, ptype, P, wind_decouple=0, mode="ld"):
    """-> dict: the eight sums ([ngroups] or [ngroups][9]), MaxDens, seed_index (int64, -1: none) and, for the bounds, Length and
    abs_<sum> = the sum of |term| of every sum (np.longdouble).  mass: float32 P.Mass, ptype: P.Type, P: dict of the COLUMNS."""
    assert mode in ("ld", "ref")
    n = len(mass)
    mass = np.asarray(mass, np.float32)
    c = {k: _col(P, k, n) for k in COLUMNS}
    have_density = P.get("density") is not None
    wide = np.longdouble if mode == "ld" else np.float64
    out = {}
    for k in SUMS:
        shape = (ngroups, NMETALS) if k.endswith("ElemMass") else (ngroups,)
        out[k] = np.zeros(shape, np.float32 if (mode == "ref" and k in FLOAT_MEMBERS) else wide)
        out["abs_" + k] = np.zeros(shape, np.longdouble)
    out["MaxDens"] = np.zeros(ngroups)
    out["seed_index"] = np.full(ngroups, -1, np.int64)
    out["Length"] = np.zeros(ngroups, np.int64)

    group = np.asarray(group, np.int64)
    ptype = np.asarray(ptype, np.int64)
    ld = np.longdouble
    np.add.at(out["Length"], group[group >= 0], 1)
    eligible = (group >= 0) & (ptype == 0) & have_density
    if have_density and wind_decouple and P.get("delaytime") is not None:
        eligible &= ~(np.asarray(P["delaytime"]) > 0)                    # winds.c:114-120

    def exact_terms(k, rows):
        """the exact terms of sum k for `rows` (long double: a product of a 53-bit and a 24-bit number rounds at 2^-64)"""
        m = mass[rows].astype(ld)
        if k == "MassHeIonized":
            return m * (c["heiii_ionized"][rows] != 0)
        if k in ("GasMetalMass", "StellarMetalMass"):
            return c["metallicity"][rows].astype(ld) * m
        if k in ("GasMetalElemMass", "StellarMetalElemMass"):
            return c["metals"][rows].astype(ld) * m[:, None]
        return c[{"Sfr": "sfr", "BH_Mass": "bh_mass", "BH_Mdot": "bh_mdot"}[k]][rows].astype(ld)

    of_type = {"Sfr": 0, "GasMetalMass": 0, "GasMetalElemMass": 0, "MassHeIonized": 0, "StellarMetalMass": 4, "StellarMetalElemMass": 4,
               "BH_Mass": 5, "BH_Mdot": 5}
    for k in SUMS:
        rows = np.nonzero((group >= 0) & (ptype == of_type[k]))[0]
        e = exact_terms(k, rows)
        np.add.at(out["abs_" + k], group[rows], np.abs(e))
        if mode == "ld":
            np.add.at(out[k], group[rows], e)
    if mode == "ld":
        # the engine's defined rule: the largest density > 0 among the eligible rows, ties to the smaller particle index
        rows = np.nonzero(eligible & (c["density"] > 0))[0]
        for i in rows[np.lexsort((-rows, c["density"][rows]))]:         # ascending density, descending index: the last write wins
            out["MaxDens"][group[i]] = c["density"][i]
            out["seed_index"][group[i]] = i
        return out
    # "ref": the members one after the other (particle order), every expression in the reference's types
    f4, f8 = np.float32, np.float64
    for i in np.nonzero((group >= 0) & np.isin(ptype, (0, 4, 5)))[0]:
        g, m, t = group[i], mass[i], ptype[i]
        if t == 0:                                                       # :647-654
            out["MassHeIonized"][g] = f4(out["MassHeIonized"][g] + f4(m * f4(c["heiii_ionized"][i] != 0)))
            out["Sfr"][g] += f8(c["sfr"][i])
            out["GasMetalMass"][g] += f8(c["metallicity"][i]) * f8(m)
            out["GasMetalElemMass"][g] = out["GasMetalElemMass"][g] + c["metals"][i].astype(f4) * m      # float * float, float +=
        if t == 4:                                                       # :655-660
            out["StellarMetalMass"][g] += f8(c["metallicity"][i]) * f8(m)
            out["StellarMetalElemMass"][g] = out["StellarMetalElemMass"][g] + c["metals"][i].astype(f4) * m
        if t == 5:                                                       # :662-666
            out["BH_Mdot"][g] += f8(c["bh_mdot"][i])
            out["BH_Mass"][g] += f8(c["bh_mass"][i])
        if eligible[i] and c["density"][i] > out["MaxDens"][g]:         # :670-676: the first row on a strict >
            out["MaxDens"][g] = c["density"][i]
            out["seed_index"][g] = i
    return out


def first_strict_maximum(order, group, ngroups, ptype, P, wind_decouple=0):
    """MaxDens / seed_index as fof.c:670-676 leaves them when the members arrive in `order` (a permutation of the particles): the first
    row on a strict >.  Among equal maxima the result follows the order of arrival, which the reference's qsort leaves unspecified."""
    maxdens = np.zeros(ngroups)
    seed = np.full(ngroups, -1, np.int64)
    if P.get("density") is None:
        return maxdens, seed
    for i in order:
        g = int(group[i])
        if g >= 0 and int(ptype[i]) == 0 and not decoupled(P, i, wind_decouple) and P["density"][i] > maxdens[g]:
            maxdens[g] = P["density"][i]
            seed[g] = i
    return maxdens, seed


def sum_bound(length, abs_sum, eps=2.0 ** -52):
    """|sum - exact| <= L eps sum|term|: L - 1 additions in any order err by (L - 1) (eps / 2) sum|term| to first order, one rounding of
    the term itself by (eps / 2) sum|term|; the factor 2 covers the higher orders"""
    length = np.asarray(length, np.longdouble)
    return (length[:, None] if np.ndim(abs_sum) == 2 else length) * np.longdouble(eps) * abs_sum


def seed_marks(group_mass, group_masstype, group_lentype, seed_index, par):
    """fof.c:1356-1365 -> the marked groups, in group order"""
    marked = ((np.asarray(group_mass) >= par["MinFoFMassForNewSeed"]) & (np.asarray(group_masstype)[:, 4] >= par["MinMStarForNewSeed"])
              & (np.asarray(group_lentype)[:, 5] == 0) & (np.asarray(seed_index) >= 0))
    return np.nonzero(marked)[0]


def bh_powerlaw_seed_mass(ident, table, par):
    """blackhole.c:1039-1053"""
    w = float(table[((int(ident) + 23) & M64) % len(table)])
    x1 = 1 + par["SeedBlackHoleMassIndex"]
    norm = np.power(np.float64(par["MaxSeedBlackHoleMass"]), x1) - np.power(np.float64(par["SeedBlackHoleMass"]), x1)
    return float(np.power(w * norm + np.power(np.float64(par["SeedBlackHoleMass"]), x1), 1. / x1))


def blackhole_make_one(i, cols, pos, atime, table, par):
    """blackhole.c:1056-1111 on the columns of `cols` (numpy arrays in particle order, changed in place; slots_convert is type = 5).
    Returns 1 when the reference prints its mass warning (:1105), else 0."""
    if cols["type"][i] != 0:
        raise SeedError("Only Gas turns into blackholes, what's wrong?")
    cols["type"][i] = 5
    if par["MaxSeedBlackHoleMass"] > 0:
        cols["bh_mass"][i] = bh_powerlaw_seed_mass(cols["id"][i], table, par)
    else:
        cols["bh_mass"][i] = par["SeedBlackHoleMass"]
    cols["mseed"][i] = cols["bh_mass"][i]
    cols["mdot"][i] = 0
    cols["formationtime"][i] = atime
    cols["swallowid"][i] = np.uint64(M64)
    cols["bh_density"][i] = 0
    cols["tb_dynfric"][i] = cols["tb_hydro"][i]
    cols["minpotpos"][i] = pos[i]
    for k in ("dfaccel", "df_surroundingvel", "dragaccel"):
        cols[k][i] = 0
    cols["df_surroundingrmsvel"][i] = 0
    cols["df_surroundingdensity"][i] = 0
    cols["jumptominpot"][i] = 0
    cols["countprogs"][i] = 1
    if par["SeedBHDynMass"] > 0:
        cols["mtrack"][i] = cols["mass"][i]
        cols["mass"][i] = par["SeedBHDynMass"]                             # (P.Mass is a float)
    else:
        cols["mtrack"][i] = -1
    warn = int(float(cols["mass"][i]) < cols["bh_mass"][i] or float(cols["mass"][i]) < cols["mtrack"][i])
    cols["kineticfdbkenergy"][i] = 0
    cols["vdisp"][i] = 0
    return warn


def fof_seed(group_mass, group_masstype, group_lentype, seed_index, cols, pos, atime, table, par):
    """fof.c:1345-1449 on one rank -> (seed particles, seed groups, warnings); every seed row is tested before any is converted"""
    groups = seed_marks(group_mass, group_masstype, group_lentype, seed_index, par)
    parts = np.asarray(seed_index, np.int64)[groups]
    if cols is None:
        return parts, groups, 0
    if np.any(cols["type"][parts] != 0):
        raise SeedError("Only Gas turns into blackholes, what's wrong?")
    nwarn = sum(blackhole_make_one(int(i), cols, pos, atime, table, par) for i in parts)
    return parts, groups, nwarn
