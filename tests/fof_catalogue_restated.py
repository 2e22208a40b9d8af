"""numpy restatement of the group catalogue fof_save_groups writes (fofpetaio.c, petaio.c), what tests/test_gpu_fof_catalogue.py compares
csrc/fof_catalogue.hip with, bit for bit.  It cites the reference's lines and holds none of its text.

  pig_order        fof_select_func (fofpetaio.c:33-36), the IsGarbage test and the counts of petaio_build_selection (petaio.c:117-154),
                   order_by_type_and_grnr (fofpetaio.c:202-218) with equal keys in ascending index (the engine's defined choice; the
                   reference's qsort leaves it open); NumPartInGroupTotal as fof_write_header counts it (fofpetaio.c:432-436)
  wrap_double      the two loops of GTPosition / GTMassCenterPosition / GTBlackholeMinPotPos (petaio.c:750-751, fofpetaio.c:499-500,
                   petaio.c:881-882), explicit, in double
  wrap_float       the same loops on the FLOAT out of GTFirstPos (fofpetaio.c:479-481): compared as double, stored back as float
  gather           petaio_build_buffer with SIMPLE_GETTER / GTPosition (petaio.c:744-753) / GTVelocity (petaio.c:803-817) / GTGroupID (:887)
  group_blocks     the getters of fofpetaio.c:464-536 on the table sorted by GrNr (fofpetaio.c:44-45)
  header           fof_write_header, fofpetaio.c:440-459
Each wrap loop is bounded at WRAP_TRIPS trips like the engine's; a value that needs more, or is not finite, is refused (WrapError)."""
import numpy as np

WRAP_TRIPS = 64
NP = dict(f8=np.float64, f4=np.float32, u1=np.uint8, u4=np.uint32, u8=np.uint64, i4=np.int32, i8=np.int64)


class WrapError(Exception):
    def __init__(self, row):
        Exception.__init__(self, "row %d" % row)
        self.row = row


def pig_order(grnr, ptype, flags=None):
    """-> perm (indices of the selected rows by (type, GrNr, index)), count[6], in_group[6]"""
    grnr, ptype = np.asarray(grnr, np.int64), np.asarray(ptype, np.int64)
    flags = np.zeros(len(grnr), np.uint8) if flags is None else np.asarray(flags, np.uint8)
    ingroup = (grnr >= 0) & (ptype < 6)                                   # (rows of the engine's type 7 are skipped)
    sel = ingroup & ((flags & 1) == 0) & ((flags & 2) == 0)
    idx = np.nonzero(sel)[0]
    perm = idx[np.lexsort((idx, grnr[idx], ptype[idx]))]
    count = np.array([(sel & (ptype == t)).sum() for t in range(6)], np.int64)
    in_group = np.array([(ingroup & (ptype == t)).sum() for t in range(6)], np.int64)
    return perm.astype(np.int64), count, in_group


def wrap_double_one(x, box):
    """-> (wrapped, ok)"""
    x, box = float(x), float(box)
    ok = np.isfinite(x)
    t = 0
    while x > box and t < WRAP_TRIPS:
        x -= box
        t += 1
    ok = ok and not x > box
    t = 0
    while x <= 0 and t < WRAP_TRIPS:
        x += box
        t += 1
    return x, bool(ok and not x <= 0)


def wrap_float_one(x, box):
    """the loops on a float: every comparison in double, every -= / += rounded back to float"""
    x, box = np.float32(x), np.float64(box)
    ok = np.isfinite(x)
    t = 0
    while np.float64(x) > box and t < WRAP_TRIPS:
        x = np.float32(np.float64(x) - box)
        t += 1
    ok = ok and not np.float64(x) > box
    t = 0
    while np.float64(x) <= 0 and t < WRAP_TRIPS:
        x = np.float32(np.float64(x) + box)
        t += 1
    return x, bool(ok and not np.float64(x) <= 0)


def _wrap_rows(a, box, one, dtype):
    a = np.asarray(a)
    out = np.empty(a.shape, dtype)
    flat, src = out.reshape(-1), a.reshape(-1)
    per_row = a.shape[1] if a.ndim == 2 else 1
    first_bad = None
    for e in range(src.size):
        flat[e], ok = one(src[e], box)
        if not ok and first_bad is None:
            first_bad = e // per_row
    if first_bad is not None:
        raise WrapError(first_bad)
    return out


def get_position(pos, offset, box):
    """out = Pos - CurrentParticleOffset in double, then the two loops"""
    with np.errstate(invalid="ignore"):
        return _wrap_rows(np.asarray(pos, np.float64) - np.asarray(offset, np.float64)[None, :], box, wrap_double_one, np.float64)


def get_firstpos(firstpos, offset, box):
    """out = (float)(FirstPos - offset), then the loops on the float"""
    out = (np.asarray(firstpos, np.float32).astype(np.float64) - np.asarray(offset, np.float64)[None, :]).astype(np.float32)
    return _wrap_rows(out, box, wrap_float_one, np.float32)


def velocity_factor(atime, UsePeculiarVelocity):
    return 1.0 / atime if UsePeculiarVelocity else 1.0


def get_velocity(vel, atime, UsePeculiarVelocity):
    """(float)(fac * Vel), the product in double"""
    return (velocity_factor(atime, UsePeculiarVelocity) * np.asarray(vel).astype(np.float64)).astype(np.float32)


def cast(a, dtype):
    """a C conversion from the column's type to the block's (SIMPLE_GETTER)"""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(a).astype(NP[dtype])


def gather(perm, column, dtype, conv="NONE", offset=(0, 0, 0), box=0.0, atime=1.0, UsePeculiarVelocity=1):
    rows = np.asarray(column)[np.asarray(perm, np.int64)]
    if conv == "POSITION":
        return get_position(rows, offset, box)
    if conv == "VELOCITY":
        return get_velocity(rows, atime, UsePeculiarVelocity)
    return cast(rows, dtype)                                              # NONE and GROUPID (GrNr as u4)


SUBGRID_OF = dict(StarFormationRate="Sfr", MassHeIonized="MassHeIonized", BlackholeMass="BH_Mass", BlackholeAccretionRate="BH_Mdot",
                  GasMetalMass="GasMetalMass", StellarMetalMass="StellarMetalMass", GasMetalElemMass="GasMetalElemMass",
                  StellarMetalElemMass="StellarMetalElemMass")
METAL_BLOCKS = ("GasMetalMass", "StellarMetalMass", "GasMetalElemMass", "StellarMetalElemMass")


def group_blocks(G, sub, offset, box, atime, UsePeculiarVelocity, MetalReturnOn):
    """G: the table of dev_fof_groups (MinID order, numpy); sub: that of dev_fof_subgrid or None (zeros) -> {block: array in GrNr order}"""
    order = np.argsort(G["GrNr"], kind="stable")
    ng = len(order)
    out = dict(GroupID=G["GrNr"].astype(np.uint32), MinID=G["MinID"].view(np.uint64) if G["MinID"].dtype != np.uint64 else G["MinID"],
               Mass=G["Mass"].astype(np.float32), MassByType=G["MassType"].astype(np.float32), Imom=G["Imom"].reshape(ng, 9).astype(np.float32),
               Jmom=G["Jmom"].astype(np.float32), LengthByType=G["LenType"].astype(np.uint32),
               MassCenterVelocity=get_velocity(G["Vel"], atime, UsePeculiarVelocity))
    if ng:
        out["MassCenterPosition"] = get_position(G["CM"], offset, box)
        out["FirstPos"] = get_firstpos(G["FirstPos"], offset, box)
    else:
        out["MassCenterPosition"], out["FirstPos"] = np.zeros((0, 3)), np.zeros((0, 3), np.float32)
    for name, key in SUBGRID_OF.items():
        if name in METAL_BLOCKS and not MetalReturnOn:
            continue
        shape = (ng, 9) if name.endswith("ElemMass") else (ng,)
        out[name] = np.zeros(shape, np.float32) if sub is None else np.asarray(sub[key]).reshape(shape).astype(np.float32)
    return {k: v[order] for k, v in out.items()}


def header(in_group, ngroups, box, atime, hubble, UsePeculiarVelocity, MassTable, OmegaLambda, Omega0, HubbleParam, CMBTemperature, OmegaBaryon):
    rsd = 1.0 / (atime * hubble)
    if not UsePeculiarVelocity:
        rsd /= atime
    return dict(NumPartInGroupTotal=np.asarray(in_group, np.uint64), NumFOFGroupsTotal=np.uint64(ngroups), RSDFactor=rsd,
                MassTable=np.asarray(MassTable, np.float64), Time=atime, BoxSize=box, OmegaLambda=OmegaLambda, Omega0=Omega0, HubbleParam=HubbleParam,
                CMBTemperature=CMBTemperature, OmegaBaryon=OmegaBaryon, UsePeculiarVelocity=np.int32(1 if UsePeculiarVelocity else 0))
