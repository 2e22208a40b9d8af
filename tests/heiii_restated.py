"""numpy restatement of the helium reionisation by quasar bubbles (libgadget/cooling_qso_lightup.c), written from the cited lines, over ALL
pairs (no tree): gaussian_rng :280-286, build_qso_candidate_list :290-311, choose_QSO_halo :348-363 (one rank: ncand_before = 0),
gas_ionization_fraction :367-382, ionize_single_particle :388-408, ionize_all_part :476-518 with the pair test of treewalk.c:962-999, and
turn_on_quasars :523-638.

Two independent forms:
  (a) sequential   the literal loop: one bubble at a time, every gas row tested against it, the list shortened by hand.
  (b) batched      the choices and radii of the whole loop first; then per batch of B iterations the FIRST bubble that covers each row, the
                   counts as a histogram, the loop replayed on the counts, the rows of the bubbles before the stop ionised
                   (include/mpgadget_hip.h).  B = None takes the whole sequence as one batch.
Both keep the reference's two quirks: the candidate at list position 0 ionises nothing but is consumed (:505), and the choice that empties
the list is never lit (:581-585).
Not a test module: imported by test_heiii_restated.py (runs anywhere) and test_gpu_heiii.py (the HIP path)."""
import math

import numpy as np

from veldisp_restated import nearest

GAMMA_MINUS1 = 5.0 / 3.0 - 1          # physconst.h:35-36
HYDROGEN_MASSFRAC = 0.76              # physconst.h:38
PROTONMASS = 1.6726e-24
HEMASS = 4.002602                     # cooling_qso_lightup.c:46
M64 = (1 << 64) - 1
NOTHING_TO_DO, NO_CANDIDATES, REACHED, EXHAUSTED, INSUFFICIENT = range(5)
REASONS = ("nothing to do", "no candidates", "reached", "exhausted", "insufficient")


class HeiiiError(RuntimeError):
    """what the engine returns as an error: no gas, a radius that is not positive and finite, log(0)"""


def rnd(table, seed):
    """get_random_number, system.c:55-61"""
    return float(table[(int(seed) & M64) % len(table)])


def bubble_radius(par, table, minid):
    """gaussian_rng, :280-286, seeded with the group's MinID"""
    u1, u2 = rnd(table, minid), rnd(table, int(minid) + 1)
    if u1 == 0:
        raise HeiiiError("u1 == 0")
    z1 = math.sqrt(-2 * math.log(u1)) * math.cos(2 * math.pi * u2)
    r = par["mean_bubble"] + math.sqrt(par["var_bubble"]) * z1
    if not (math.isfinite(r) and r > 0):
        raise HeiiiError("radius %r" % r)
    return r


def heat(d, st):
    """Entropy + deltau / uu_in_cgs / entropytou of every row (:398-406); rows of zero density are never asked for"""
    a3inv = 1 / math.pow(st["atime"], 3)
    deltau = st["qso_inst_heating"] * ((1 - HYDROGEN_MASSFRAC) / (PROTONMASS * HEMASS))
    with np.errstate(all="ignore"):
        entropytou = np.power(d["density"] * a3inv, GAMMA_MINUS1) / GAMMA_MINUS1
        delta = deltau / st["uu_in_cgs"] / entropytou
    return delta


def r2_to(d, centre):
    dist = nearest(np.asarray(centre, np.float64) - d["pos"], d["box"])
    return dist[:, 0] * dist[:, 0] + dist[:, 1] * dist[:, 1] + dist[:, 2] * dist[:, 2]


def candidates(d, par):
    return [g for g in range(len(d["gmass"])) if not d["gmass"][g] < par["qso_candidate_min_mass"] and not d["gmass"][g] > par["qso_candidate_max_mass"]]


def _start(d, par, st):
    if st["n_gas_tot"] <= 0:
        raise HeiiiError("n_gas_tot")
    flag = d["flag"].copy()
    ent = d["entropy"].copy()
    gas = d["type"] == 0
    delta = heat(d, st)
    res = dict(n_ionized_before=int((gas & (flag != 0)).sum()), flash_ionized=0, iterations=0, tot_n_ionized=0)
    if st["desired_ion_frac"] > par["heIIIreion_finish_frac"]:           # :539-548
        rows = gas & (flag == 0)
        flag[rows] = 1
        ent[rows] = ent[rows] + delta[rows]
        res["flash_ionized"] = int(rows.sum())
    res["initionfrac"] = res["curionfrac"] = int((gas & (flag != 0)).sum()) / st["n_gas_tot"]          # :367-382
    return flag, ent, gas, delta, res


def sequential(d, par, st, table):
    """form (a).  Returns (flag, entropy, result, records); a record is (position, group, radius, count, curionfrac)."""
    flag, ent, gas, delta, res = _start(d, par, st)
    desired, ngt = st["desired_ion_frac"], st["n_gas_tot"]
    cur = res["curionfrac"]
    records = []
    cand = candidates(d, par) if cur < desired else []                   # :559-562
    ncand = ncand_tot = len(cand)
    if ncand_tot == 0:                                                   # :568-572
        res["stop_reason"] = NO_CANDIDATES if cur < desired else NOTHING_TO_DO
        return flag, ent, res, records
    it = 0
    reason = REACHED
    while cur < desired:
        qso = int(rnd(table, st["TotNgroups"] + it) * ncand_tot)         # :351-353
        ncand_tot -= 1
        new_qso = qso if 0 <= qso < ncand else -1
        if ncand_tot <= 0:                                               # :581-585
            reason = EXHAUSTED
            break
        group, radius, count = -1, 0.0, 0
        if new_qso > 0:                                                  # :505
            group = cand[new_qso]
            radius = bubble_radius(par, table, d["gminid"][group])
            r2 = r2_to(d, d["gcm"][group])
            rows = gas & ~(r2 > radius * radius) & (flag == 0)           # treewalk.c:970-991, :443, :392
            flag[rows] = 1
            ent[rows] = ent[rows] + delta[rows]
            count = int(rows.sum())
        cur += count / ngt                                               # :591
        res["tot_n_ionized"] += count
        records.append((new_qso, group, radius, count, cur))
        if count < 0.01 * st["non_overlapping_bubble_number"] and it > 10:   # :618
            reason = INSUFFICIENT
            break
        if new_qso >= 0:                                                 # :624-627
            del cand[new_qso]
            ncand -= 1
        it += 1
    res.update(curionfrac=cur, iterations=len(records), stop_reason=reason)
    return flag, ent, res, records


def choice_sequence(d, par, st, table):
    """every choice the loop can make, with the radii: [(position, group, radius)]; ends before the choice that empties the list"""
    slots = candidates(d, par)
    seq = []
    total = len(slots)
    for it in range(total):
        left = total - it
        qso = int(rnd(table, st["TotNgroups"] + it) * left)
        if left - 1 <= 0:
            break
        pos = qso if 0 <= qso < len(slots) else -1
        if pos > 0:
            g = slots[pos]
            seq.append((pos, g, bubble_radius(par, table, d["gminid"][g])))
        else:
            seq.append((pos, -1, 0.0))
        if pos >= 0:
            slots = slots[:pos] + slots[pos + 1:]
    return seq


def batched(d, par, st, table, B=None):
    """form (b)"""
    flag, ent, gas, delta, res = _start(d, par, st)
    desired, ngt = st["desired_ion_frac"], st["n_gas_tot"]
    cur = res["curionfrac"]
    records = []
    if not cur < desired:
        res["stop_reason"] = NOTHING_TO_DO
        return flag, ent, res, records
    if not candidates(d, par):
        res["stop_reason"] = NO_CANDIDATES
        return flag, ent, res, records
    seq = choice_sequence(d, par, st, table)
    B = max(len(seq), 1) if B is None else B
    reason = None
    n = len(flag)
    for it0 in range(0, len(seq), B):
        if not cur < desired:
            break
        chunk = seq[it0:it0 + B]
        first = np.full(n, len(chunk), np.int64)
        takes_part = gas & (flag == 0)
        for k in reversed(range(len(chunk))):                            # the earliest cover survives
            pos, g, radius = chunk[k]
            if pos > 0:
                inside = takes_part & ~(r2_to(d, d["gcm"][g]) > radius * radius)
                first[inside] = k
        counts = np.bincount(first, minlength=len(chunk) + 1)
        lit = 0
        for k in range(len(chunk)):
            if not cur < desired:
                reason = REACHED
                break
            c = int(counts[k])
            cur += c / ngt
            res["tot_n_ionized"] += c
            records.append((chunk[k][0], chunk[k][1], chunk[k][2], c, cur))
            lit = k + 1
            if c < 0.01 * st["non_overlapping_bubble_number"] and it0 + k > 10:
                reason = INSUFFICIENT
                break
        rows = first < lit
        flag[rows] = 1
        ent[rows] = ent[rows] + delta[rows]
        if reason is not None:
            break
    if reason is None:
        reason = EXHAUSTED if cur < desired else REACHED
    res.update(curionfrac=cur, iterations=len(records), stop_reason=reason)
    return flag, ent, res, records


# ---- inputs shared by the two test modules ---------------------------------------------------------------------------------------------
ATIME = 0.22
TABLE_SIZE = 10007
TOTNGROUPS = 161
POS0_ITERATION = 2          # the iteration whose choice is list position 0


def heiii_scene(pos_gas, box, seed):
    """A particle table: the gas, with garbage rows (type 7), rows that became stars (4) or black holes (5) since, some dark matter, and a
    twentieth of the rows already ionised (stars among them: they do not count).  161 groups, about 100 of them inside the mass window
    [100, 1000] - one exactly on each bound -, centred near gas positions or anywhere, one in a corner of the box, one in the emptiest spot; one MinID
    above 2^63.  The random table makes the choice of iteration POS0_ITERATION list position 0, gives the corner group the largest radius
    (0.6 box) and the group in the void the smallest (0.03 box) when mean_bubble = 0.3 box, var_bubble = (0.09 box)^2."""
    rng = np.random.RandomState(seed)
    pos_gas = np.array(pos_gas, np.float64)
    ng = len(pos_gas)
    ndm = 37
    pos = np.mod(np.concatenate([pos_gas, box * rng.random_sample((ndm, 3))]), box)
    pos[pos <= 0] += box
    pos = np.ascontiguousarray(pos)
    n = len(pos)
    assert n % 64 != 0
    ptype = np.concatenate([np.zeros(ng, np.uint8), np.ones(ndm, np.uint8)])
    pick = rng.choice(ng, 60, replace=False)
    garbage, stars, bhs = pick[:25], pick[25:55], pick[55:]
    ptype[garbage], ptype[stars], ptype[bhs] = 7, 4, 5
    flag = (rng.random_sample(n) < 0.05).astype(np.uint8)
    flag[stars[:10]] = 1                                        # ionised, then became stars: not counted, not touched
    flag[garbage[:5]] = 1
    density = ng / box ** 3 * np.exp(0.5 * rng.standard_normal(n))
    entropy = 1.0 + rng.random_sample(n)
    # groups
    ngr = TOTNGROUPS
    at = rng.choice(ng, ngr, replace=False)
    gcm = pos_gas[at] + 0.02 * box * rng.standard_normal((ngr, 3))
    anywhere = rng.random_sample(ngr) < 0.5                      # half of the centres anywhere in the box: bubbles off the clusters as well
    gcm[anywhere] = box * rng.random_sample((int(anywhere.sum()), 3))
    gcm = np.mod(gcm, box)
    gmass = np.where(rng.random_sample(ngr) < 0.62, 100 + 900 * rng.random_sample(ngr), np.where(rng.random_sample(ngr) < 0.5, 99.999, 1000.001))
    gmass[rng.random_sample(ngr) < 0.1] = 5000.0
    inwin = np.nonzero((gmass >= 100) & (gmass <= 1000))[0]
    gmass[inwin[3]], gmass[inwin[7]] = 100.0, 1000.0            # exactly on the bounds: both are candidates
    corner, void, big = int(inwin[5]), int(inwin[9]), int(inwin[11])
    gcm[corner] = box * np.array([2e-4, 0.9997, 3e-4])
    # the emptiest of a set of trial points: the smallest bubble there covers nothing
    trial = box * rng.random_sample((400, 3))
    dmin = [np.sqrt((nearest(t - pos_gas, box) ** 2).sum(1).min()) for t in trial]
    gcm[void] = trial[int(np.argmax(dmin))]
    gcm = np.ascontiguousarray(gcm)
    gminid = rng.randint(1, 1 << 48, ngr).astype(np.uint64)
    gminid[big] += np.uint64(1 << 63)
    table = rng.random_sample(TABLE_SIZE)
    table[table == 0] = 0.5
    choice_slots = set((TOTNGROUPS + it) % TABLE_SIZE for it in range(ngr))

    def slots_of(g):
        return set(((int(gminid[g]) + j) & M64) % TABLE_SIZE for j in (0, 1))
    for g in (corner, void):                                     # the table entries written below belong to that group alone
        while True:
            others = set(choice_slots)
            for h in range(ngr):
                if h != g:
                    others |= slots_of(h)
            if len(slots_of(g)) == 2 and not slots_of(g) & others:
                break
            gminid[g] = np.uint64(rng.randint(1, 1 << 48))
    pos0_slot = (TOTNGROUPS + POS0_ITERATION) % TABLE_SIZE
    assert not any(pos0_slot in slots_of(g) for g in range(ngr))

    def set_z(g, z, sign):                                       # radius = mean + sigma z: u2 = 0 or 1/2, u1 = exp(-z^2 / 2)
        table[int(gminid[g]) % TABLE_SIZE] = math.exp(-z * z / 2)
        table[(int(gminid[g]) + 1) % TABLE_SIZE] = 0.0 if sign > 0 else 0.5
    set_z(corner, (0.6 - 0.3) / 0.09, +1)
    set_z(void, (0.3 - 0.03) / 0.09, -1)
    table[(TOTNGROUPS + POS0_ITERATION) % TABLE_SIZE] = 0.0      # the choice of that iteration is list position 0
    return dict(pos=pos, type=ptype, box=float(box), n=n, ng=ng, density=density, entropy=entropy, flag=flag, gmass=gmass, gcm=gcm, gminid=gminid,
                table=table, corner=corner, void=void, big=big, garbage=garbage, stars=stars, bhs=bhs)


SCENES = dict(zel=12, clust=12)    # seeds
_cache = {}


def scene(ics, name):
    """the 16^3 gas of ics.hydro_pair(16), the clustered 4096-gas set ics.s_clust(16)"""
    if name not in _cache:
        if name == "zel":
            pos, _, typ, box = ics.hydro_pair(16)
            pg = pos[typ == 0]
        else:
            pg, _, box = ics.s_clust(16, seed=3)
        _cache[name] = heiii_scene(pg, box, SCENES[name])
    return _cache[name]


def params(d, **over):
    p = dict(qso_candidate_min_mass=100.0, qso_candidate_max_mass=1000.0, mean_bubble=0.3 * d["box"], var_bubble=(0.09 * d["box"]) ** 2,
             heIIIreion_finish_frac=0.995)
    p.update(over)
    return p


def step(d, **over):
    s = dict(atime=ATIME, desired_ion_frac=0.6, qso_inst_heating=2.9e-11, uu_in_cgs=1e10, n_gas_tot=d["ng"], non_overlapping_bubble_number=0,
             TotNgroups=TOTNGROUPS)
    s.update(over)
    return s


def case(d, name):
    """(parameters, step, expected stop reason) of the named case"""
    box = d["box"]
    if name == "main":                     # desired reached mid-list; list position 0 chosen at iteration POS0_ITERATION, inside the lit range
        return params(d), step(d, desired_ion_frac=0.93), REACHED
    if name == "exhausted":                # a narrow mass window and small bubbles: the list runs out, the last candidate unlit
        return params(d, qso_candidate_min_mass=100.0, qso_candidate_max_mass=200.0, mean_bubble=0.08 * box, var_bubble=(0.01 * box) ** 2), \
            step(d, desired_ion_frac=0.9), EXHAUSTED
    if name == "insufficient":             # tiny bubbles: the first iteration after the tenth that ionises fewer than 0.01 N rows ends the loop
        return params(d, mean_bubble=0.06 * box, var_bubble=(0.015 * box) ** 2), step(d, desired_ion_frac=0.9, non_overlapping_bubble_number=100), INSUFFICIENT
    if name == "nothing":
        return params(d), step(d, desired_ion_frac=0.01), NOTHING_TO_DO
    if name == "nocand":
        return params(d, qso_candidate_min_mass=1e6, qso_candidate_max_mass=2e6), step(d), NO_CANDIDATES
    if name == "flash":                    # every gas row ionised at once; the loop then runs on counts of zero
        return params(d), step(d, desired_ion_frac=0.999, non_overlapping_bubble_number=100), INSUFFICIENT
    raise KeyError(name)


CASES = ("main", "exhausted", "insufficient", "nothing", "nocand", "flash")


def restated(ics, sname, cname):
    """(scene, parameters, step, (flag, entropy, result, records)) of form (a), computed once"""
    key = (sname, cname)
    if key not in _cache:
        d = scene(ics, sname)
        par, st, _ = case(d, cname)
        _cache[key] = (d, par, st, sequential(d, par, st, d["table"]))
    return _cache[key]


def conditions(d, par, st, out, cname):
    """what the committed seeds must satisfy for the GPU comparison to be one of equal integers (asserted, no row left out); returns the
    margins and the overlap numbers"""
    flag, ent, res, records = out
    _, _, want = case(d, cname)
    assert res["stop_reason"] == want, (cname, REASONS[res["stop_reason"]])
    gas = np.nonzero(d["type"] == 0)[0]
    sub = dict(pos=d["pos"][gas], box=d["box"])
    info = dict(gap=float("inf"), multi=0, notfirst=0, rmin=float("inf"), rmax=0.0)
    cand = candidates(d, par)
    radii = {}
    for g in cand:                                               # EVERY candidate: any of them may enter a batch
        rad = bubble_radius(par, d["table"], d["gminid"][g])
        assert rad > 0
        radii[g] = rad
        r = np.sqrt(r2_to(sub, d["gcm"][g]))
        info["gap"] = min(info["gap"], float(np.abs(r - rad).min() / rad))
    assert info["gap"] > 1e-10, info["gap"]
    if cname == "main":
        lit = [(k, rec[1]) for k, rec in enumerate(records) if rec[0] > 0]
        assert res["tot_n_ionized"] >= 500
        assert 0 < len(records) < len(cand) - 1                 # mid-list
        assert records[POS0_ITERATION][0] == 0 and records[POS0_ITERATION][3] == 0 and POS0_ITERATION < len(records) - 1
        cover = np.zeros(len(gas), np.int64)
        firstg = np.full(len(gas), -1, np.int64)
        ming = np.full(len(gas), 1 << 40, np.int64)
        for k, g in lit:
            inside = ~(r2_to(sub, d["gcm"][g]) > radii[g] * radii[g])
            cover += inside
            firstg[inside & (firstg < 0)] = g
            ming[inside] = np.minimum(ming[inside], g)
        info["multi"] = int((cover >= 2).sum())
        info["notfirst"] = int(((cover >= 2) & (firstg != ming)).sum())
        assert info["multi"] >= 100 and info["notfirst"] >= 5, info
        rr = [rec[2] / d["box"] for rec in records if rec[0] > 0]
        info["rmin"], info["rmax"] = min(rr), max(rr)
        allr = [radii[g] / d["box"] for g in cand]
        assert min(allr) < 0.031 and max(allr) > 0.599 and max(allr) > 0.5      # the wrap, and a radius above half the box
        assert len(cand) >= 80 and d["gmass"][cand].min() == 100.0 and d["gmass"][cand].max() == 1000.0
        assert d["big"] in cand and int(d["gminid"][d["big"]]) > 1 << 63
        void_r2 = r2_to(sub, d["gcm"][d["void"]])
        assert (void_r2 > radii[d["void"]] ** 2).all()          # one bubble covers nothing
    if cname == "exhausted":
        assert len(records) == len(cand) - 1 >= 3
    if cname == "insufficient":
        assert len(records) > 12
    if cname == "flash":
        assert res["flash_ionized"] > 1000 and res["tot_n_ionized"] == 0
    return info
