"""The FOF group catalogue on disk: what fof_save_groups writes at every snapshot with SnapshotWithFOF (fof.c:1157-1163,
fofpetaio.c:38-159) - `Header`, the `FOFGroups/*` blocks in GrNr order and the particles-in-group blocks `<type>/<name>` sorted by
(type, GrNr) - from device-resident columns on one rank (Engine.dev_fof_save_groups; csrc/fof_catalogue.hip).

The two block tables are DATA: one row per block the reference registers, in the order of its registration, with the condition under which
it does.  PIG_BLOCKS: register_io_blocks(..., WriteGroupID = 1, MetalReturnOn), petaio.c:986-1080; GROUP_BLOCKS: fof_register_io_blocks,
fofpetaio.c:538-568 (these the engine writes itself from its group table).

`required` is 1 for a block registered with IO_REG and 0 for IO_REG_NONFATAL, IO_REG_WRONLY and IO_REG_TYPE.  Blocks whose getter COMPUTES
(InternalEnergy, NeutralHydrogenFraction, the helium fractions, StarFormationRate) are plain optional columns here: the caller computes them
with the calls that exist (mpg_dev_cooling_state, the Sfr column) and hands them in; this module computes nothing."""
import os
from collections import namedtuple

from . import snapshot
from .engine import EngineError, catalogue_block, fof_catalogue_params

Block = namedtuple("Block", "ptype name dtype nmemb conv required cond derived")
ALWAYS = "always"
CONDITIONS = (ALWAYS, "MetalReturnOn", "OutputPotential", "OutputTimebins", "DensityIndependentSph", "OutputHeliumFractions", "ExcursionSetReionOn")
# the reference's defaults (IO.OutputPotential 1, IO.OutputTimebins 0, DensityIndependentSphOn 1, IO.OutputHeliumFractions 0, no excursion set)
DEFAULT_OPTIONS = dict(MetalReturnOn=1, OutputPotential=1, OutputTimebins=0, DensityIndependentSph=1, OutputHeliumFractions=0, ExcursionSetReionOn=0)


def _b(ptype, name, dtype, nmemb=1, required=1, cond=ALWAYS, conv="NONE", derived=False):
    return Block(ptype, name, dtype, nmemb, conv, required, cond, derived)


def _pig_table():
    t = []
    for i in range(6):                                                       # petaio.c:991-1006
        t += [_b(i, "Mass", "f4"), _b(i, "Position", "f8", 3, conv="POSITION"), _b(i, "Velocity", "f4", 3, conv="VELOCITY"), _b(i, "ID", "u8"),
              _b(i, "Potential", "f4", required=0, cond="OutputPotential"), _b(i, "GroupID", "u4", required=0, conv="GROUPID"),
              _b(i, "TimeBinHydro", "u4", required=0, cond="OutputTimebins"), _b(i, "TimeBinGravity", "u4", required=0, cond="OutputTimebins")]
    t += [_b(0, "Generation", "u1"), _b(4, "Generation", "u1"), _b(5, "Generation", "u1"),                                    # :1008-1010
          _b(0, "SmoothingLength", "f4"), _b(0, "Density", "f4"), _b(0, "EgyWtDensity", "f4", cond="DensityIndependentSph"),  # :1012-1016
          _b(0, "InternalEnergy", "f4", derived=True), _b(0, "ElectronAbundance", "f4"),                                      # :1021-1024
          _b(0, "NeutralHydrogenFraction", "f4", required=0, derived=True),                                                   # :1025
          _b(0, "HeliumIFraction", "f4", required=0, cond="OutputHeliumFractions", derived=True),                             # :1027-1031
          _b(0, "HeliumIIFraction", "f4", required=0, cond="OutputHeliumFractions", derived=True),
          _b(0, "HeliumIIIFraction", "f4", required=0, cond="OutputHeliumFractions", derived=True),
          _b(0, "HeIIIIonized", "u1", required=0), _b(0, "StarFormationRate", "f4", required=0, derived=True),                # :1033-1036
          _b(0, "DelayTime", "f4", required=0), _b(4, "BirthDensity", "f4", required=0), _b(4, "StarFormationTime", "f4", required=0),  # :1038-1041
          _b(0, "Metallicity", "f4", required=0), _b(4, "Metallicity", "f4", required=0),                                     # :1042-1043
          _b(0, "Metals", "f4", 9, required=0, cond="MetalReturnOn"), _b(4, "Metals", "f4", 9, required=0, cond="MetalReturnOn"),  # :1044-1050
          _b(4, "LastEnrichmentMyr", "f4", required=0, cond="MetalReturnOn"), _b(4, "TotalMassReturned", "f4", required=0, cond="MetalReturnOn"),
          _b(4, "SmoothingLength", "f4", required=0, cond="MetalReturnOn"),
          _b(5, "StarFormationTime", "f4", required=0), _b(5, "BlackholeMass", "f4"), _b(5, "BlackholeDensity", "f4"),       # :1054-1063
          _b(5, "BlackholeAccretionRate", "f4"), _b(5, "BlackholeProgenitors", "i4"), _b(5, "BlackholeMinPotPos", "f8", 3, conv="POSITION"),
          _b(5, "BlackholeJumpToMinPot", "i4"), _b(5, "BlackholeMtrack", "f4"), _b(5, "BlackholeMseed", "f4", required=0),
          _b(5, "BlackholeKineticFdbkEnergy", "f4", required=0),
          _b(5, "SmoothingLength", "f4", required=0), _b(5, "Swallowed", "u1", required=0), _b(5, "BlackholeSwallowID", "u8", required=0),  # :1066-1072
          _b(5, "BlackholeSwallowTime", "f4", required=0),
          _b(0, "J21", "f4", required=0, cond="ExcursionSetReionOn"), _b(0, "ZReionized", "f4", required=0, cond="ExcursionSetReionOn")]  # :1075-1080
    return tuple(t)


PIG_BLOCKS = _pig_table()
G = "FOFGroups"
GROUP_BLOCKS = (                                                             # fofpetaio.c:545-567
    _b(G, "GroupID", "u4"), _b(G, "Mass", "f4"), _b(G, "MassCenterPosition", "f8", 3), _b(G, "FirstPos", "f4", 3), _b(G, "MinID", "u8"),
    _b(G, "Imom", "f4", 9), _b(G, "Jmom", "f4", 3), _b(G, "MassCenterVelocity", "f4", 3, required=0), _b(G, "LengthByType", "u4", 6),
    _b(G, "MassByType", "f4", 6), _b(G, "MassHeIonized", "f4"), _b(G, "StarFormationRate", "f4"),
    _b(G, "GasMetalMass", "f4", cond="MetalReturnOn"), _b(G, "StellarMetalMass", "f4", cond="MetalReturnOn"),
    _b(G, "GasMetalElemMass", "f4", 9, cond="MetalReturnOn"), _b(G, "StellarMetalElemMass", "f4", 9, cond="MetalReturnOn"),
    _b(G, "BlackholeMass", "f4"), _b(G, "BlackholeAccretionRate", "f4"))
# the attributes of Header with their types (fof_write_header, fofpetaio.c:448-459)
HEADER_ATTRS = (("NumPartInGroupTotal", "u8", 6), ("NumFOFGroupsTotal", "u8", 1), ("RSDFactor", "f8", 1), ("MassTable", "f8", 6), ("Time", "f8", 1),
                ("BoxSize", "f8", 1), ("OmegaLambda", "f8", 1), ("Omega0", "f8", 1), ("HubbleParam", "f8", 1), ("CMBTemperature", "f8", 1),
                ("OmegaBaryon", "f8", 1), ("UsePeculiarVelocity", "i4", 1))


def _active(table, options):
    opt = dict(DEFAULT_OPTIONS)
    bad = set(options) - set(opt)
    if bad:
        raise EngineError("fof catalogue: unknown option(s) %s" % sorted(bad))
    opt.update(options)
    return [b for b in table if b.cond == ALWAYS or opt[b.cond]]


def pig_blocks(**options):
    """The particle blocks the reference registers under `options` (DEFAULT_OPTIONS), in the order it writes them: by type, then by
    registration (order_by_type, petaio.c:967-982, :1084)."""
    act = _active(PIG_BLOCKS, options)
    return sorted(act, key=lambda b: (b.ptype, act.index(b)))


def group_blocks(**options):
    return _active(GROUP_BLOCKS, options)


def build_descriptors(columns, ptypes=(0, 1, 2, 3, 4, 5), **options):
    """The mpg_catalogue_block descriptors of `columns` - {name: tensor} (one column in particle order serves every type that has the block)
    or {(ptype, name): tensor} (that type alone; it wins) - in the reference's order.  Refuses a column no active block takes, and names a
    required block that is left out.  GroupID needs no column (the GrNr of the last dev_fof_fof).  Touches no engine."""
    blocks = [b for b in pig_blocks(**options) if b.ptype in ptypes]
    used, out, missing = set(), [], []
    for b in blocks:
        key = (b.ptype, b.name) if (b.ptype, b.name) in columns else b.name
        col = columns.get(key)
        if col is not None:
            used.add(key)
        elif b.conv != "GROUPID":
            if b.required and not b.derived:
                missing.append("%d/%s" % (b.ptype, b.name))
            continue
        out.append((b, col))
    unknown = [k for k in columns if k not in used and columns[k] is not None]
    if unknown:
        raise EngineError("fof catalogue: no block of the table takes the column(s) %s" % sorted("%d/%s" % k if isinstance(k, tuple) else k for k in unknown))
    if missing:
        raise EngineError("fof catalogue: required block(s) left out: %s" % ", ".join(missing))
    return [catalogue_block(b.name, b.ptype, col, b.dtype, b.conv) for b, col in out]


def save_fof_catalogue(engine, path, columns, atime, hubble, flags=None, CurrentParticleOffset=(0.0, 0.0, 0.0), UsePeculiarVelocity=1, SaveParticles=1,
                       nfile=1, ptypes=(0, 1, 2, 3, 4, 5), header=None, **options):
    """fof_save_groups for the groups of the engine's last dev_fof_fof (and dev_fof_subgrid): `columns` are device tensors in particle order
    keyed as build_descriptors takes them; header: dict of MassTable, OmegaLambda, Omega0, HubbleParam, CMBTemperature, OmegaBaryon;
    options: the switches of DEFAULT_OPTIONS (MetalReturnOn also decides the four metal blocks of FOFGroups)."""
    desc = build_descriptors(columns, ptypes, **options) if SaveParticles else []
    opt = dict(DEFAULT_OPTIONS, **options)
    par = fof_catalogue_params(atime, hubble, CurrentParticleOffset, UsePeculiarVelocity, opt["MetalReturnOn"], SaveParticles, nfile, **(header or {}))
    engine.dev_fof_save_groups(path, par, desc, flags=flags)


def _blocks_under(path, sub):
    d = os.path.join(path, sub)
    return sorted(f for f in os.listdir(d) if os.path.exists(os.path.join(d, f, "header"))) if os.path.isdir(d) else []


def read_fof_catalogue(path):
    """(header, groups, parts): the twelve attributes, {block: array} of FOFGroups, {ptype: {block: array}} of the particle blocks found."""
    header = {}
    for name, dt, nm in HEADER_ATTRS:
        v = snapshot.get_attr(path, "Header", name, dt, nm)
        header[name] = v if nm > 1 else v[0]
    groups = {b: snapshot.read_block(path, "FOFGroups/" + b) for b in _blocks_under(path, "FOFGroups")}
    parts = {}
    for t in range(6):
        names = _blocks_under(path, str(t))
        if names:
            parts[t] = {b: snapshot.read_block(path, "%d/%s" % (t, b)) for b in names}
    return header, groups, parts


def block_info(path):
    """{block: dict(dtype, nmemb, nfile, size)} of every block of the catalogue but Header"""
    out = {}
    for sub in ["FOFGroups"] + [str(t) for t in range(6)]:
        for b in _blocks_under(path, sub):
            out["%s/%s" % (sub, b)] = snapshot.block_info(path, "%s/%s" % (sub, b))
    return out


__all__ = ["PIG_BLOCKS", "GROUP_BLOCKS", "HEADER_ATTRS", "pig_blocks", "group_blocks", "build_descriptors", "save_fof_catalogue", "read_fof_catalogue",
           "block_info", "Block"]
